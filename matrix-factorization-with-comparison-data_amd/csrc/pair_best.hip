// pair_best.hip — per column i of a row, the admissible partner j with the largest s_ij |g_i - g_j|^2 on gfx950: the
// arg-max a D-optimal comparison design needs per iteration (fifth follow-on; include/mfcd.h:
// mfcd_pair_best_rows; mfcd/design.py).
//
// For row r (scores a, truth x, table g = G + r * g_row_stride of k rows of d columns) and every column i,
//   best_val_i = max over admissible j != i of s_ij q_ij,   s_ij = sigmoid'(a_i - a_j),   q_ij = |g_i - g_j|^2,
// and best_j_i the smallest j that attains it.  q_ij = max(n_i + n_j - 2 g_i . g_j, 0): the products ride the fp32 matrix
// pipe, the squared norms n come from a pre-pass (f64 sum in the order of the columns, rounded to fp32 once).  The caller
// centres the table, so the cancellation is at the size of the table's spread.
//
// One workgroup of 256 threads per (row, tile of kBestTile = 128 columns i); wave w owns the 32 columns i of its
// quarter.  The columns j stream through LDS in stages of kBestJ = 64, a chunk of at most 128 columns of d at a time.
// v_mfma_f32_32x32x2_f32 is oriented with M = j and N = i: the A operand is g_j from LDS (lane l: row l & 31 of the
// block of 32), the B operand g_i from registers (lane l: its own column i = l & 31), and the accumulator's column is i.
// A lane then owns one i and sixteen j per block of 32 x 32, forms their scores and keeps a running (max, arg j) in
// registers.  The order of the K steps is free as long as both operands agree: half-wave h takes the columns
// [h KC / 2, (h + 1) KC / 2) of the chunk, so that a lane's K steps are consecutive floats of its LDS row and come in by
// 16-byte reads.
//
// A lane visits its j in ascending order and replaces its maximum only by a strictly larger score; the two half-waves of
// a column are combined once at the end by one cross-lane exchange, the tie going to the smaller j.  No atomics, no LDS
// reduction, every result has one owner: two calls are bit-equal and a row does not depend on its neighbours.
//
// Finiteness: the pre-pass stores NaN as the norm of a table row with a non-finite entry; every workgroup stages the
// whole row of a, x and n and sees any non-finite entry (an fp32 overflow of a norm included), and the row is stored as
// NaN / -1.
#include "common.h"
#include "pairs_common.h"

namespace {

constexpr int kBestThreads = 256;
constexpr int kBestTile = 128;                         // columns i per workgroup (mfcd/pairs.py: BEST_TILE)
constexpr int kBestJ = 64;                             // columns j per LDS stage
constexpr int kBestMaxD = 256;
constexpr int64_t kBestNormBytes = 64 << 20;           // bounds the workspace: the norms of a block of rows
constexpr int64_t kBestMaxRows = 32768;                // rows per launch: the pre-pass has one grid row per table

inline int best_tiles(int k) { return (k + kBestTile - 1) / kBestTile; }
inline int best_chunk_rows(int rows, int k)
{
    const int64_t fit = kBestNormBytes / ((int64_t)k * (int64_t)sizeof(float));   // >= 16
    return pair_chunk_rows(rows, best_tiles(k), fit < kBestMaxRows ? fit : kBestMaxRows);
}

struct BestArgs {
    const float *A, *X, *G;
    int64_t lda, ldx, g_row_stride, ldg;
    LawArgs law;
    int k, d, T;
    const float *nrm;              // [rows or 1][k]
    int64_t nrm_stride;            // 0: one table for every row
    float *val;
    int32_t *arg;
    int64_t ldv, ldj;
};

// n_j = |g_j|^2 of every table row: f64 sum in the order of the columns, rounded once; NaN for a non-finite row.
// Grid (ceil(k / 256), tables).
__global__ __launch_bounds__(kBestThreads) void best_norm_kernel(const float *__restrict__ G, int64_t g_row_stride, int64_t ldg,
                                                                 int k, int d, float *__restrict__ nrm)
{
    const int j = blockIdx.x * kBestThreads + threadIdx.x;
    if (j >= k) return;
    const float *g = G + (int64_t)blockIdx.y * g_row_stride + (int64_t)j * ldg;
    double s = 0.0;
    bool bad = false;
    for (int p = 0; p < d; ++p) {
        const float v = g[p];
        bad |= is_nonfinite_bits(v);
        s += (double)v * (double)v;                    // exact product
    }
    nrm[(int64_t)blockIdx.y * k + j] = bad ? __uint_as_float(0x7fc00000u) : (float)s;
}

template <int KC, int NC, bool HW, bool HM, bool HL>
__global__ __launch_bounds__(kBestThreads) void pair_best_kernel(BestArgs g)
{
    constexpr int H = KC / 2;                          // K steps per chunk: columns per half-wave
    constexpr int VW = H % 4 == 0 ? 4 : 2;             // floats per LDS read
    constexpr int LD = KC + VW;                        // consecutive rows start VW banks apart
    __shared__ __attribute__((aligned(16))) float bt[kBestJ * LD];
    __shared__ float ta[kBestJ], tx[kBestJ], tn[kBestJ];
    __shared__ float2 tab[HW ? kBestJ : 1];
    __shared__ int lab[HL ? kBestJ : 1];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
    const int k = g.k, d = g.d;
    const int64_t r = blockIdx.x / g.T;
    const int I = (int)(blockIdx.x - r * g.T);
    const float *a = g.A + r * g.lda, *x = g.X ? g.X + r * g.ldx : nullptr;
    const float *tbl = g.G + r * g.g_row_stride, *nrm = g.nrm + r * g.nrm_stride;
    const int32_t *lb = HL ? g.law.labels + r * g.law.label_stride : nullptr;
    const int ig = I * kBestTile + wave * 32 + l31;
    const bool in = ig < k;                            // a column past k is computed and never stored
    const float ai = in ? a[ig] : 0.0f, ni = in ? nrm[ig] : 0.0f;
    const float xi = HM && in ? x[ig] : 0.0f;
    const float ali = HW && in ? g.law.alpha[ig] : 0.0f, bei = HW && in ? g.law.beta[ig] : 0.0f;
    const int li = HL && in ? lb[ig] : 0;
    const float mg = g.law.margin;

    float gi[NC * H];                                  // the B operand: g_i, the lane's K steps of every chunk
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int s = 0; s < H; ++s) {
            const int p = c * KC + half * H + s;       // pad columns are zeros
            gi[c * H + s] = in && p < d ? tbl[(int64_t)ig * g.ldg + p] : 0.0f;
        }

    float bv = -1.0f;                                  // every score is >= +0: no partner yet
    int bj = -1, bad = 0;
    for (int jb = 0; jb < k; jb += kBestJ) {
        f32x16 acc[2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[b][q] = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            __syncthreads();                           // the previous chunk's and stage's readers are done
            if (c == 0 && tid < kBestJ) {
                const int j = jb + tid;
                const bool inj = j < k;
                const float va = inj ? a[j] : 0.0f, vx = x && inj ? x[j] : 0.0f, vn = inj ? nrm[j] : 0.0f;
                bad |= (int)(is_nonfinite_bits(va) || is_nonfinite_bits(vx) || is_nonfinite_bits(vn));
                ta[tid] = va;
                tx[tid] = vx;
                tn[tid] = vn;
                if (HW) tab[tid] = make_float2(inj ? g.law.alpha[j] : 0.0f, inj ? g.law.beta[j] : 0.0f);
                if (HL) lab[tid] = inj ? lb[j] : 0;
            }
#pragma unroll
            for (int t = 0; t < kBestJ * KC / kBestThreads; ++t) {
                const int e = t * kBestThreads + tid, jj = e / KC, p = e % KC, j = jb + jj, col = c * KC + p;
                bt[jj * LD + p] = j < k && col < d ? tbl[(int64_t)j * g.ldg + col] : 0.0f;   // pad rows and columns are zeros
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const float *row = bt + (b * 32 + l31) * LD + half * H;
#pragma unroll
                for (int s0 = 0; s0 < H; s0 += VW) {
                    float v[VW];
                    if constexpr (VW == 4) {
                        const float4 t = *reinterpret_cast<const float4 *>(row + s0);
                        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
                    } else {
                        const float2 t = *reinterpret_cast<const float2 *>(row + s0);
                        v[0] = t.x, v[1] = t.y;
                    }
#pragma unroll
                    for (int u = 0; u < VW; ++u)
                        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[u], gi[c * H + s0 + u], acc[b], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 16; ++q) {             // ascending j
                const int jj = b * 32 + tile_row(q, half), j = jb + jj;
                const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(ai - ta[jj]));   // exp(-|da|) <= 1
                const float h = __builtin_amdgcn_rcpf(1.0f + e);
                const float s = e * h * h;
                const float qd = fmaxf(fmaf(-2.0f, acc[b][q], ni + tn[jj]), 0.0f);
                const float sc = __fmul_rn(s, qd);
                bool ok = j != ig && j < k;            // the diagonal and the pad columns
                if (HW || HM || HL) {
                    float alj = 0.0f, bej = 0.0f;
                    if constexpr (HW) {
                        alj = tab[jj].x;
                        bej = tab[jj].y;
                    }
                    ok = ok && law_weight<HW, HM, HL>(HM ? xi - tx[jj] : 0.0f, ali, bei, li, alj, bej, HL ? lab[jj] : 0, mg) > 0.0f;
                }
                if (ok && sc > bv) {                   // strictly larger: the smallest j among equal scores stays
                    bv = sc;
                    bj = j;
                }
            }
    }

    bad = __syncthreads_or(bad);
    const float ov = __shfl_xor(bv, 32, MFCD_WAVE);    // the other half of the column's j
    const int oj = __shfl_xor(bj, 32, MFCD_WAVE);
    if (oj >= 0 && (ov > bv || (ov == bv && oj < bj))) {
        bv = ov;
        bj = oj;
    }
    if (half == 0 && in) {
        g.val[r * g.ldv + ig] = bad ? __uint_as_float(0x7fc00000u) : bj < 0 ? 0.0f : bv;
        g.arg[r * g.ldj + ig] = bad ? -1 : bj;
    }
}

}  // namespace

extern "C" size_t mfcd_pair_best_workspace_bytes(int rows, int k, int d)
{
    if (rows < 0 || k < 1 || k > kPairMaxCols || d < 1 || d > kBestMaxD) return 0;
    const int R = best_chunk_rows(rows, k);
    return align_up((size_t)(R > 0 ? R : 1) * (size_t)k * sizeof(float));
}

extern "C" int mfcd_pair_best_rows(const float *A, int64_t lda, const float *X, int64_t ldx, const float *G,
                                   int64_t g_row_stride, int64_t ldg, int d, int rows, int k, const mfcd_pair_law *law,
                                   float *best_val, int64_t ldv, int32_t *best_j, int64_t ldj, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    if (!A || !G || !best_val || !best_j || rows < 0 || k < 1 || k > kPairMaxCols || d < 1 || d > kBestMaxD) return MFCD_EINVAL;
    if (lda < k || ldv < k || ldj < k || (X && ldx < k) || ldg < d) return MFCD_EINVAL;
    if (g_row_stride != 0 && g_row_stride < (int64_t)k * ldg) return MFCD_EINVAL;
    const void *v = best_val, *j = best_j;
    if (v == (const void *)A || v == (const void *)X || v == (const void *)G || v == j) return MFCD_EINVAL;
    if (j == (const void *)A || j == (const void *)X || j == (const void *)G) return MFCD_EINVAL;
    LawArgs la = {};
    if (law) {
        if (law_args(law, k, &la)) return MFCD_EINVAL;
        if (law->use_margin && !X) return MFCD_EINVAL;
    }
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_pair_best_workspace_bytes(rows, k, d)) return MFCD_EWORKSPACE;
    const int T = best_tiles(k), R = best_chunk_rows(rows, k);
    const bool per_row = g_row_stride != 0;
    float *nrm = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    // stream order keeps one block's norms apart from the next's
    return pair_chunks(rows, R, [&](int r0, int nr) {
        const float *tbl = G + (int64_t)r0 * g_row_stride;
        if (per_row || r0 == 0) {
            hipLaunchKernelGGL(best_norm_kernel, dim3((unsigned)((k + kBestThreads - 1) / kBestThreads), (unsigned)(per_row ? nr : 1)),
                               dim3(kBestThreads), 0, st, tbl, g_row_stride, ldg, k, d, nrm);
            MFCD_HIP_TRY(hipGetLastError());
        }
        BestArgs g;
        g.A = A + (int64_t)r0 * lda;
        g.X = X ? X + (int64_t)r0 * ldx : nullptr;
        g.G = tbl;
        g.lda = lda;
        g.ldx = ldx;
        g.g_row_stride = g_row_stride;
        g.ldg = ldg;
        g.law = law_rows(la, r0);
        g.k = k;
        g.d = d;
        g.T = T;
        g.nrm = nrm;
        g.nrm_stride = per_row ? k : 0;
        g.val = best_val + (int64_t)r0 * ldv;
        g.arg = best_j + (int64_t)r0 * ldj;
        g.ldv = ldv;
        g.ldj = ldj;
        const dim3 grid((unsigned)((int64_t)nr * T)), block(kBestThreads);
        law_dispatch(la, law && law->use_margin != 0, [&](auto hw, auto hm, auto hl) {
            if (d <= 4) hipLaunchKernelGGL((pair_best_kernel<4, 1, hw(), hm(), hl()>), grid, block, 0, st, g);
            else if (d <= 32) hipLaunchKernelGGL((pair_best_kernel<32, 1, hw(), hm(), hl()>), grid, block, 0, st, g);
            else if (d <= 64) hipLaunchKernelGGL((pair_best_kernel<64, 1, hw(), hm(), hl()>), grid, block, 0, st, g);
            else if (d <= 128) hipLaunchKernelGGL((pair_best_kernel<128, 1, hw(), hm(), hl()>), grid, block, 0, st, g);
            else hipLaunchKernelGGL((pair_best_kernel<128, 2, hw(), hm(), hl()>), grid, block, 0, st, g);
        });
        return (int)hipGetLastError();
    });
}
