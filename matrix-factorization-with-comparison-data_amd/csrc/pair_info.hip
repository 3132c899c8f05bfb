// pair_info.hip — the row Laplacian of the pair kernels applied to all d columns of an item table at once on gfx950
// (fourth follow-on; include/mfcd.h: mfcd_pair_hvp_multi_rows).
//
// For row r (scores a, truth x) and every column i of the row, with b~ the row's gathered item vectors minus their column
// mean,
//   z_i = sum over j != i of c_ij (b~_i - b~_j) = deg_i b~_i - sum over j of c_ij b~_j,   c_ij = w_ij sigmoid'(a_i - a_j),
// and deg_i = sum over j != i of c_ij.  It is mfcd_pair_law_hvp_rows for d directions in one pass: the weight c_ij — one exp
// and one reciprocal per ordered pair — is generated once, in registers, and the d multiply-adds per pair ride the fp32
// matrix pipe.
//
// One workgroup of 256 threads per (row, tile of kInfoTile = 128 columns i, chunk of at most 128 columns of d); wave w
// owns the 32 columns i of its quarter.  The columns j stream through LDS in stages of kInfoJ = 64: (a, x, alpha, beta,
// label) of the stage and the stage's centred rows of B.  v_mfma_f32_32x32x2_f32 takes A[i][kk] from lane (i = l & 31,
// kk = l >> 5), so in step s of a stage lane l generates exactly one weight, c of (its i, column 2 s + kk), and the ND
// tiles of 32 columns of d reuse it against B[kk][p] = b~ of that column from LDS.  The column j = i and the pad columns
// past the row's end have their weight set to 0.
//
// Rounding: the fp32 MFMA accumulators and the lane's fp32 partial of deg are widened to f64 after every stage, i.e.
// after at most 64 terms (32 for deg), as the other pair kernels do; z_i = deg_i b~_i - sum is formed in f64 from the two
// f64 sums and rounded to fp32 once.  b~ is formed in f64 from the f64 column mean of a pre-pass and rounded to fp32 once,
// so the cancellation of the Laplacian form is that of values of the size of the spread of B, not of its offset.
//
// No atomics: every sum has one owner and a fixed order; the pre-pass adds a column's entries in eight interleaved
// slices and the slices in order.  The pre-pass also checks every index against the table's rows before anything is
// gathered and every entry it adds for finiteness; a row so flagged, or with a non-finite entry in a or x (every
// workgroup stages the whole row and sees it), is stored as NaN.
#include "common.h"
#include "pairs_common.h"

namespace {

constexpr int kInfoThreads = 256;
constexpr int kInfoTile = 128;                         // columns i per workgroup (mfcd/pairs.py: INFO_TILE)
constexpr int kInfoJ = 64;                             // columns j per LDS stage = terms per fp32 accumulator run
constexpr int kInfoMaxD = 256;
constexpr int kInfoChunkD = 128;                       // columns of d per workgroup
constexpr int kInfoMaxRows = 4096;                     // rows per launch: bounds the workspace at 8.2 MiB
constexpr int kInfoSlices = 8;                         // interleaved slices of the centre's sums
constexpr size_t kInfoRowBytes = kInfoMaxD * sizeof(double) + (kInfoMaxD / 32) * sizeof(int);

inline int info_tiles(int k) { return (k + kInfoTile - 1) / kInfoTile; }
inline int info_chunk_rows(int rows, int T) { return pair_chunk_rows(rows, T, kInfoMaxRows); }

struct InfoArgs {
    const float *A, *X, *B;
    int64_t lda, ldx, ldb;
    const int32_t *index;          // nullptr: column j reads row j of B
    int64_t index_stride;          // 0: one index vector for every row
    LawArgs law;
    int k, d, T, per_row;          // per_row: a centre and a flag per row (else one for all)
    const double *ctr;             // [rows or 1][kInfoMaxD]
    const int *flag;               // [rows or 1][kInfoMaxD / 32]
    float *Z, *deg;
    int64_t ldz, ldd;
};

// Column means of the gathered table, in f64, and the row's flag.  Grid (centres, 32-column groups of d).
__global__ __launch_bounds__(kInfoThreads) void info_centre_kernel(const float *__restrict__ B, int64_t ldb, int mB, int d,
                                                                   const int32_t *__restrict__ index, int64_t index_stride,
                                                                   int k, double *__restrict__ ctr, int *__restrict__ flag)
{
    __shared__ double part[kInfoSlices][32];
    const int tid = threadIdx.x, c32 = tid & 31, sl = tid >> 5, p = blockIdx.y * 32 + c32;
    const int64_t c = blockIdx.x;
    const int32_t *idx = index ? index + c * index_stride : nullptr;
    double sum = 0.0;
    int bad = 0;
    for (int j = sl; j < k; j += kInfoSlices) {
        const int b = idx ? idx[j] : j;
        if ((unsigned)b >= (unsigned)mB) {             // checked before the gather
            bad = 1;
            continue;
        }
        if (p < d) {
            const float v = B[(int64_t)b * ldb + p];
            bad |= (int)is_nonfinite_bits(v);
            sum += (double)v;
        }
    }
    part[sl][c32] = sum;
    bad = __syncthreads_or(bad);
    if (sl == 0) {
        double s = 0.0;
        for (int w = 0; w < kInfoSlices; ++w) s += part[w][c32];   // fixed order
        if (p < d) ctr[c * kInfoMaxD + p] = s / (double)k;
        if (tid == 0) flag[c * (kInfoMaxD / 32) + blockIdx.y] = bad;
    }
}

template <int ND, bool HW, bool HM, bool HL>
__global__ __launch_bounds__(kInfoThreads) void pair_info_kernel(InfoArgs g)
{
    constexpr int DC = 32 * ND;                        // columns of d of this workgroup
    constexpr int LD = DC % 64 == 0 ? DC + 32 : DC;    // the two rows a step reads fall into different halves of the banks
    constexpr int JPT = kInfoJ * DC / kInfoThreads;    // rows of the stage a thread fills
    __shared__ float bt[kInfoJ * LD];
    __shared__ float ta[kInfoJ], tx[kInfoJ];
    __shared__ float2 tab[HW ? kInfoJ : 1];
    __shared__ int lab[HL ? kInfoJ : 1];
    __shared__ double degs[kInfoThreads / 64][32];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
    const int k = g.k, d = g.d;
    const int64_t r = blockIdx.x / g.T;
    const int I = (int)(blockIdx.x - r * g.T);
    const int dc0 = blockIdx.y * kInfoChunkD;
    const int64_t c = g.per_row ? r : 0;
    const float *a = g.A + r * g.lda, *x = g.X ? g.X + r * g.ldx : nullptr;
    const int32_t *idx = g.index ? g.index + r * g.index_stride : nullptr;
    const int32_t *lb = HL ? g.law.labels + r * g.law.label_stride : nullptr;
    const float nanf32 = __uint_as_float(0x7fc00000u);
    const int i0 = I * kInfoTile + wave * 32, ig = i0 + l31;

    int bad = 0;                                       // the same for every thread: the row's index or B rows are bad
    for (int y = 0; y < (d + 31) / 32; ++y) bad |= g.flag[c * (kInfoMaxD / 32) + y];
    if (!bad) {
        const bool in = ig < k;                        // a column past k is computed and never stored
        const float ai = in ? a[ig] : 0.0f;
        const float xi = HM && in ? x[ig] : 0.0f;
        const float ali = HW && in ? g.law.alpha[ig] : 0.0f, bei = HW && in ? g.law.beta[ig] : 0.0f;
        const int li = HL && in ? lb[ig] : 0;
        const float mg = g.law.margin;
        const int fp = tid % DC, fj = tid / DC;        // the stage's loader: column fp of the chunk, rows fj + q * (256 / DC)
        const double cfp = dc0 + fp < d ? g.ctr[c * kInfoMaxD + dc0 + fp] : 0.0;

        f32x16 acc[ND];
        double accd[ND][16], dacc = 0.0;
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                acc[nd][q] = 0.0f;
                accd[nd][q] = 0.0;
            }

        for (int jb = 0; jb < k; jb += kInfoJ) {
            __syncthreads();                           // the previous stage's readers are done
            if (tid < kInfoJ) {
                const int j = jb + tid;
                const bool inj = j < k;
                const float va = inj ? a[j] : 0.0f, vx = x && inj ? x[j] : 0.0f;
                bad |= (int)(is_nonfinite_bits(va) || is_nonfinite_bits(vx));
                ta[tid] = va;
                tx[tid] = vx;
                if (HW) tab[tid] = make_float2(inj ? g.law.alpha[j] : 0.0f, inj ? g.law.beta[j] : 0.0f);
                if (HL) lab[tid] = inj ? lb[j] : 0;
            }
#pragma unroll
            for (int q = 0; q < JPT; ++q) {
                const int jj = fj + q * (kInfoThreads / DC), j = jb + jj;
                float v = 0.0f;                        // pad rows and pad columns are zeros
                if (j < k && dc0 + fp < d) {
                    const int b = idx ? idx[j] : j;    // in range: the pre-pass checked the whole row
                    v = (float)((double)g.B[(int64_t)b * g.ldb + dc0 + fp] - cfp);
                }
                bt[jj * LD + fp] = v;
            }
            __syncthreads();
            float dg = 0.0f;                           // <= 32 terms
#pragma unroll 4
            for (int s = 0; s < kInfoJ / 2; ++s) {
                const int jj = 2 * s + half, j = jb + jj;
                const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * fabsf(ai - ta[jj]));   // exp(-|da|) <= 1
                const float h = __builtin_amdgcn_rcpf(1.0f + e);
                float cw = e * h * h;
                if (HW || HM || HL) {
                    float alj = 0.0f, bej = 0.0f;
                    if constexpr (HW) {
                        alj = tab[jj].x;
                        bej = tab[jj].y;
                    }
                    cw = __fmul_rn(law_weight<HW, HM, HL>(HM ? xi - tx[jj] : 0.0f, ali, bei, li, alj, bej, HL ? lab[jj] : 0, mg),
                                   cw);
                }
                cw = (j == ig || j >= k) ? 0.0f : cw;  // the diagonal and the pad columns
                dg += cw;
#pragma unroll
                for (int nd = 0; nd < ND; ++nd)
                    acc[nd] = __builtin_amdgcn_mfma_f32_32x32x2f32(cw, bt[jj * LD + nd * 32 + l31], acc[nd], 0, 0, 0);
            }
            dacc += (double)dg;
#pragma unroll
            for (int nd = 0; nd < ND; ++nd)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    accd[nd][q] += (double)acc[nd][q];
                    acc[nd][q] = 0.0f;
                }
        }

        bad = __syncthreads_or(bad);
        const double dtot = dacc + __shfl_xor(dacc, 32, MFCD_WAVE);   // the two halves of the columns j: the same bits in both
        if (half == 0) degs[wave][l31] = dtot;
        __syncthreads();
        if (g.deg && blockIdx.y == 0 && half == 0 && in) g.deg[r * g.ldd + ig] = bad ? nanf32 : (float)dtot;
#pragma unroll
        for (int nd = 0; nd < ND; ++nd) {
            const int p = dc0 + nd * 32 + l31;
            const double cp = p < d ? g.ctr[c * kInfoMaxD + p] : 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = tile_row(q, half), i = i0 + row;
                if (i < k && p < d) {
                    const int b = idx ? idx[i] : i;
                    const float bi = (float)((double)g.B[(int64_t)b * g.ldb + p] - cp);
                    float z = (float)(degs[wave][row] * (double)bi - accd[nd][q]);   // rounded to fp32 once
                    z = z == 0.0f ? 0.0f : z;          // a column without weight: +0, not -0
                    g.Z[(r * k + i) * g.ldz + p] = bad ? nanf32 : z;
                }
            }
        }
    } else {
        if (g.deg && blockIdx.y == 0 && half == 0 && ig < k) g.deg[r * g.ldd + ig] = nanf32;
        for (int nd = 0; nd < ND; ++nd) {
            const int p = dc0 + nd * 32 + l31;
            for (int q = 0; q < 16; ++q) {
                const int i = i0 + tile_row(q, half);
                if (i < k && p < d) g.Z[(r * k + i) * g.ldz + p] = nanf32;
            }
        }
    }
}

}  // namespace

extern "C" size_t mfcd_pair_hvp_multi_workspace_bytes(int rows, int k, int d)
{
    if (rows < 0 || k < 1 || k > kPairMaxCols || d < 1 || d > kInfoMaxD) return 0;
    const int R = info_chunk_rows(rows, info_tiles(k));
    return align_up((size_t)(R > 0 ? R : 1) * kInfoRowBytes);
}

extern "C" int mfcd_pair_hvp_multi_rows(const float *A, int64_t lda, const float *X, int64_t ldx, const float *B, int64_t ldb,
                                        int mB, int d, const int32_t *index, int64_t index_stride, int rows, int k,
                                        const mfcd_pair_law *law, float *Z, int64_t ldz, float *deg, int64_t ldd,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (!A || !B || !Z || rows < 0 || k < 1 || k > kPairMaxCols || d < 1 || d > kInfoMaxD || mB < 1) return MFCD_EINVAL;
    if (lda < k || ldb < d || ldz < d || (X && ldx < k) || (deg && ldd < k)) return MFCD_EINVAL;
    if (index ? (index_stride != 0 && index_stride < k) : k != mB) return MFCD_EINVAL;
    if (Z == A || Z == X || Z == B || Z == deg || (const void *)Z == (const void *)index) return MFCD_EINVAL;
    if (deg && (deg == A || deg == X || deg == B || (const void *)deg == (const void *)index)) return MFCD_EINVAL;
    LawArgs la = {};
    if (law) {
        if (law_args(law, k, &la)) return MFCD_EINVAL;
        if (law->use_margin && !X) return MFCD_EINVAL;
    }
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_pair_hvp_multi_workspace_bytes(rows, k, d)) return MFCD_EWORKSPACE;
    const int T = info_tiles(k), R = info_chunk_rows(rows, T);
    const bool per_row = index && index_stride != 0;
    double *ctr = (double *)workspace;
    int *flag = (int *)((char *)workspace + (size_t)R * kInfoMaxD * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    // stream order keeps one chunk's centres apart from the next's
    return pair_chunks(rows, R, [&](int r0, int nr) {
        const int32_t *ix = index ? index + (int64_t)r0 * index_stride : nullptr;
        if (per_row || r0 == 0) {
            hipLaunchKernelGGL(info_centre_kernel, dim3((unsigned)(per_row ? nr : 1), (unsigned)((d + 31) / 32)),
                               dim3(kInfoThreads), 0, st, B, ldb, mB, d, ix, index_stride, k, ctr, flag);
            MFCD_HIP_TRY(hipGetLastError());
        }
        InfoArgs g;
        g.A = A + (int64_t)r0 * lda;
        g.X = X ? X + (int64_t)r0 * ldx : nullptr;
        g.B = B;
        g.lda = lda;
        g.ldx = ldx;
        g.ldb = ldb;
        g.index = ix;
        g.index_stride = index_stride;
        g.law = law_rows(la, r0);
        g.k = k;
        g.d = d;
        g.T = T;
        g.per_row = per_row ? 1 : 0;
        g.ctr = ctr;
        g.flag = flag;
        g.Z = Z + (int64_t)r0 * k * ldz;
        g.deg = deg ? deg + (int64_t)r0 * ldd : nullptr;
        g.ldz = ldz;
        g.ldd = ldd;
        const dim3 grid((unsigned)((int64_t)nr * T), (unsigned)((d + kInfoChunkD - 1) / kInfoChunkD)), block(kInfoThreads);
        law_dispatch(la, law && law->use_margin != 0, [&](auto hw, auto hm, auto hl) {
            if (d <= 32) hipLaunchKernelGGL((pair_info_kernel<1, hw(), hm(), hl()>), grid, block, 0, st, g);
            else if (d <= 64) hipLaunchKernelGGL((pair_info_kernel<2, hw(), hm(), hl()>), grid, block, 0, st, g);
            else hipLaunchKernelGGL((pair_info_kernel<4, hw(), hm(), hl()>), grid, block, 0, st, g);
        });
        return (int)hipGetLastError();
    });
}
