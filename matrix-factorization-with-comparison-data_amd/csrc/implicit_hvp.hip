// implicit_hvp.hip — the Hessian of the implicit-feedback risk of implicit.hip in score space, applied to a direction
// (include/mfcd.h: mfcd_implicit_hvp_rows).  For a requested row with scores a, direction y, observed
// columns P, barred columns E and N = [0, m) \ (P u E), with w_ij = sigma'(a_j - a_i) for i in P \ E, j in N:
//   q_i = coef sum_j w_ij (y_i - y_j),   q_j = coef sum_i w_ij (y_j - y_i),   deg_c = coef sum of w over c's partners,
// and 0 for a barred column: a bipartite weighted Laplacian and its diagonal.  The second-order twin of
// mfcd_implicit_rows' gradient, and its decomposition.
//
// No reference counterpart: the reference trains on sampled triplets only.
//
// Form built: PREPARE (implicit_common.h), then per block of rows SLABS, COLUMNS, POSITIVES and FINISH.
//   slabs      factor mode: topk_scores_kernel twice, the scores A B^T and the direction Ay By^T, one slab region each;
//              dense mode: the rows of X and Y are the slabs.
//   columns    implicit_hvp_col_kernel, one workgroup per (row, chunk of kImpChunk columns): implicit_col_kernel's
//              ownership.  A thread owns kImpChunk / 256 columns; the row's admissible positives stream through LDS in
//              tiles of kImpTile with a_i and y_i.  A column that is no negative carries score -inf and direction 0: its
//              weight and its difference's product are exactly 0 without a class branch.  The thread stores its
//              negatives' q and deg and the barred columns' zeros, and the workgroup leaves the number of admissible
//              columns whose score or direction is inf or NaN: w = 0 swallows an inf score, so NaN would not propagate.
//   positives  implicit_hvp_pos_kernel, one workgroup per (slot, row), the slot as the slow index (§3.17): a group of
//              256 / pow2ceil(nt) lanes per positive of the tile, the row's chunks staged in LDS one after the other
//              (scores and directions), 16-byte LDS reads, a fixed reduction tree; the positive's owner stores.
//   finish     implicit_hvp_finish_kernel, one workgroup per row: the chunks' counts in order, and NaN rows of q and deg
//              when one is not 0.
// Per pair: the difference of the scores, one v_exp_f32, one reciprocal, w = e h h (pairs_common.h: pair_curvature), the
// difference of the directions and one FMA; no log.  The difference y_. - y_. is formed per pair, so a constant direction
// gives exactly +0.  Every sum has one owner and a fixed order, no fp32 run is longer than 64 terms before it is added to
// an f64 sum, and there is no atomic of any kind: two calls are bit-equal, and a row's outputs do not depend on the other
// rows, on its place in the call, or on where a slab ends.
#include "implicit_common.h"
#include "pairs_common.h"

namespace {

// One workgroup per (row r0 + blockIdx.x / chunks, chunk blockIdx.x % chunks) of a launch.
template <bool DEG>
__global__ __launch_bounds__(kImpThreads) void implicit_hvp_col_kernel(const ImplicitArgs a, int r0)
{
    __shared__ unsigned char cls[kImpChunk];        // 0 negative, 1 positive, 2 barred
    __shared__ float pa[kImpTile], py[kImpTile];
    __shared__ int plive[kImpTile];                  // 0: a barred positive
    __shared__ int red[kImpThreads / MFCD_WAVE];
    const int tid = threadIdx.x;
    const int r = r0 + (int)(blockIdx.x / (unsigned)a.chunks), chunk = (int)(blockIdx.x % (unsigned)a.chunks);
    if (a.status[r] != 0) return;
    const int64_t pb = a.pos_off[r], L = a.pos_off[r + 1] - pb;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const int id = a.row_ids ? a.row_ids[r] : r;
    const int64_t at = a.by_id ? id : r - r0;
    const float *row = a.S + at * a.ld, *dir = a.SY + at * a.ldy;
    const int c0 = chunk * kImpChunk;
    const int len = min(kImpChunk, a.m - c0);

    for (int j = tid; j < kImpChunk; j += kImpThreads) cls[j] = 0;
    __syncthreads();
    implicit_mark(cls, c0, len, a.pos_items, pb, pb + L, 1, tid);
    __syncthreads();                                 // a barred positive is barred
    implicit_mark(cls, c0, len, a.excl_items, eb, ee, 2, tid);
    __syncthreads();

    float aj[kImpOwn], yj[kImpOwn], run_q[kImpOwn], run_d[kImpOwn];
    bool neg[kImpOwn];
    double acc_q[kImpOwn], acc_d[kImpOwn];
    int bad = 0;
#pragma unroll
    for (int c = 0; c < kImpOwn; ++c) {
        const int j = tid + kImpThreads * c;
        const bool in = j < len;
        const bool adm = in && cls[j] != 2;          // a barred column's score and direction are never read
        const float s = adm ? row[c0 + j] : 0.0f, y = adm ? dir[c0 + j] : 0.0f;
        neg[c] = in && cls[j] == 0;
        bad += (int)(adm && (is_nonfinite_bits(s) || is_nonfinite_bits(y)));
        aj[c] = neg[c] ? s : -INFINITY;              // weight exactly 0 ...
        yj[c] = neg[c] ? y : 0.0f;                   // ... times a finite difference
        run_q[c] = run_d[c] = 0.0f;
        acc_q[c] = acc_d[c] = 0.0;
    }

    for (int64_t p0 = 0; p0 < L; p0 += kImpTile) {
        const int nt = (int)min((int64_t)kImpTile, L - p0);
        __syncthreads();                             // the previous tile is done with pa, py, plive
        if (tid < nt) {
            const int c = a.pos_items[pb + p0 + tid];
            const bool barred = is_barred(a.excl_items, eb, ee, c);
            pa[tid] = barred ? 0.0f : row[c];
            py[tid] = barred ? 0.0f : dir[c];
            plive[tid] = barred ? 0 : 1;
        }
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            if (plive[i]) {                          // uniform
                const float ai = pa[i], yi = py[i];
#pragma unroll
                for (int c = 0; c < kImpOwn; ++c) {
                    const float w = pair_curvature(aj[c] - ai);
                    run_q[c] = fmaf(w, yj[c] - yi, run_q[c]);
                    if (DEG) run_d[c] += w;
                }
            }
            if ((i & 63) == 63 || i + 1 == nt) {     // a column's run: at most 64 positives
#pragma unroll
                for (int c = 0; c < kImpOwn; ++c) {
                    acc_q[c] += (double)run_q[c];
                    run_q[c] = 0.0f;
                    if (DEG) {
                        acc_d[c] += (double)run_d[c];
                        run_d[c] = 0.0f;
                    }
                }
            }
        }
    }
    const double cf = a.coef ? (double)a.coef[r] : 1.0;
#pragma unroll
    for (int c = 0; c < kImpOwn; ++c) {
        const int j = tid + kImpThreads * c;
        if (j < len && cls[j] != 1) {                // negatives and barred columns; a positive's elements are the positive pass's
            a.g[(int64_t)r * a.ldg + c0 + j] = neg[c] ? (float)(cf * acc_q[c]) + 0.0f : 0.0f;   // a zero is +0 under any coef
            if (DEG) a.deg[(int64_t)r * a.ldd + c0 + j] = neg[c] ? (float)(cf * acc_d[c]) + 0.0f : 0.0f;
        }
    }
    bad = wave_sum_xor(bad);
    if ((tid & (MFCD_WAVE - 1)) == 0) red[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0) {
        bad = 0;
        for (int w = 0; w < kImpThreads / MFCD_WAVE; ++w) bad += red[w];
        a.bad[(int64_t)(r - r0) * a.chunks + chunk] = bad;
    }
}

// One workgroup per (row r0 + blockIdx.x % nb, slot blockIdx.x / nb): the row's tiles slot, slot + slots, ...; the slot
// is the slow index, as in implicit_pos_kernel.
template <bool DEG>
__global__ __launch_bounds__(kImpThreads) void implicit_hvp_pos_kernel(const ImplicitArgs a, int r0, int nb)
{
    __shared__ __attribute__((aligned(16))) float sc[kImpChunk];
    __shared__ __attribute__((aligned(16))) float sy[kImpChunk];
    __shared__ unsigned char cls[kImpChunk];
    __shared__ float pa[kImpTile], py[kImpTile];
    __shared__ int pcol[kImpTile];                   // the positive's column, -1: barred
    __shared__ double red_q[kImpThreads], red_d[DEG ? kImpThreads : 1];
    const int tid = threadIdx.x;
    const int r = r0 + (int)(blockIdx.x % (unsigned)nb), slot = (int)(blockIdx.x / (unsigned)nb);
    if (a.status[r] != 0) return;
    const int64_t pb = a.pos_off[r], L = a.pos_off[r + 1] - pb;
    if ((int64_t)slot * kImpTile >= L) return;
    const int64_t eb = a.excl_off ? a.excl_off[r] : 0, ee = a.excl_off ? a.excl_off[r + 1] : 0;
    const int id = a.row_ids ? a.row_ids[r] : r;
    const int64_t at = a.by_id ? id : r - r0;
    const float *row = a.S + at * a.ld, *dir = a.SY + at * a.ldy;
    const double cf = a.coef ? (double)a.coef[r] : 1.0;

    for (int64_t p0 = (int64_t)slot * kImpTile; p0 < L; p0 += (int64_t)a.slots * kImpTile) {
        const int nt = (int)min((int64_t)kImpTile, L - p0);
        __syncthreads();                             // the previous tile is done with pa, py, pcol
        if (tid < nt) {
            const int c = a.pos_items[pb + p0 + tid];
            const bool barred = is_barred(a.excl_items, eb, ee, c);
            pa[tid] = barred ? 0.0f : row[c];
            py[tid] = barred ? 0.0f : dir[c];
            pcol[tid] = barred ? -1 : c;
        }
        __syncthreads();
        int shift = 8;                               // G = 256 / pow2ceil(nt) lanes per positive
        while ((kImpThreads >> shift) < nt) --shift;
        const int G = 1 << shift, gi = tid >> shift, l = tid & (G - 1);
        const bool live = gi < nt && pcol[gi] >= 0;
        const float ai = live ? pa[gi] : 0.0f, yi = live ? py[gi] : 0.0f;
        double acc_q = 0.0, acc_d = 0.0;
        for (int chunk = 0; chunk < a.chunks; ++chunk) {
            const int c0 = chunk * kImpChunk;
            const int len = min(kImpChunk, a.m - c0), quads = (len + 3) >> 2;
            __syncthreads();                         // the previous chunk is done with sc, sy, cls
            for (int j = tid; j < kImpChunk; j += kImpThreads) cls[j] = 0;
            __syncthreads();
            implicit_mark(cls, c0, len, a.pos_items, pb, pb + L, 1, tid);
            implicit_mark(cls, c0, len, a.excl_items, eb, ee, 1, tid);   // either list: no negative
            __syncthreads();
            for (int j = tid; j < 4 * quads; j += kImpThreads) {
                const bool ng = j < len && cls[j] == 0;
                sc[j] = ng ? row[c0 + j] : -INFINITY;
                sy[j] = ng ? dir[c0 + j] : 0.0f;
            }
            __syncthreads();
            if (live) {
                for (int q0 = l; q0 < quads; q0 += 16 * G) {   // 16 quads: fp32 runs of at most 64 terms
                    float run_q = 0.0f, run_d = 0.0f;
                    for (int q = q0; q < quads && q < q0 + 16 * G; q += G) {
                        const float4 s = reinterpret_cast<const float4 *>(sc)[q];
                        const float4 y = reinterpret_cast<const float4 *>(sy)[q];
                        const float w0 = pair_curvature(s.x - ai), w1 = pair_curvature(s.y - ai);
                        const float w2 = pair_curvature(s.z - ai), w3 = pair_curvature(s.w - ai);
                        run_q = fmaf(w0, yi - y.x, run_q);
                        run_q = fmaf(w1, yi - y.y, run_q);
                        run_q = fmaf(w2, yi - y.z, run_q);
                        run_q = fmaf(w3, yi - y.w, run_q);
                        if (DEG) run_d += (w0 + w1) + (w2 + w3);
                    }
                    acc_q += (double)run_q;
                    if (DEG) acc_d += (double)run_d;
                }
            }
        }
        const int sub = G < MFCD_WAVE ? G : MFCD_WAVE;   // the group's lanes of one wave, then its waves in index order
        for (int off = 1; off < sub; off <<= 1) {
            acc_q += __shfl_xor(acc_q, off, MFCD_WAVE);
            if (DEG) acc_d += __shfl_xor(acc_d, off, MFCD_WAVE);
        }
        __syncthreads();                             // the previous tile is done with red_q, red_d
        if ((tid & (sub - 1)) == 0) {
            red_q[tid / sub] = acc_q;
            if (DEG) red_d[tid / sub] = acc_d;
        }
        __syncthreads();
        if (tid < nt && pcol[tid] >= 0) {
            const int W = G / sub;
            double tq = 0.0, td = 0.0;
            for (int w = 0; w < W; ++w) {
                tq += red_q[tid * W + w];
                if (DEG) td += red_d[tid * W + w];
            }
            a.g[(int64_t)r * a.ldg + pcol[tid]] = (float)(cf * tq) + 0.0f;
            if (DEG) a.deg[(int64_t)r * a.ldd + pcol[tid]] = (float)(cf * td) + 0.0f;
        }
    }
}

// One workgroup per row of a block: the chunks in order.
__global__ __launch_bounds__(kImpThreads) void implicit_hvp_finish_kernel(const ImplicitArgs a, int r0)
{
    const int tid = threadIdx.x;
    const int r = r0 + (int)blockIdx.x;
    if (a.status[r] != 0) return;
    const int32_t *p = a.bad + (int64_t)blockIdx.x * a.chunks;
    int bad = 0;
    for (int k = tid; k < a.chunks; k += kImpThreads) bad |= (int)(p[k] != 0);
    if (!__syncthreads_or(bad)) return;
    for (int j = tid; j < a.m; j += kImpThreads) {
        a.g[(int64_t)r * a.ldg + j] = __uint_as_float(0x7FC00000u);
        if (a.deg) a.deg[(int64_t)r * a.ldd + j] = __uint_as_float(0x7FC00000u);
    }
}

inline size_t implicit_hvp_bytes(int rows, int m, bool dense)
{
    return 2 * implicit_slab_bytes(rows, m, dense) +
           align_up((size_t)implicit_block_rows(rows, m, dense) * (size_t)implicit_chunks(m) * sizeof(int32_t));
}

}  // namespace

extern "C" size_t mfcd_implicit_hvp_rows_workspace_bytes(int rows, int m, int d)
{
    if (!implicit_sizes_ok(rows, m, d)) return 0;
    return implicit_hvp_bytes(rows, m, d == 0);
}

extern "C" int mfcd_implicit_hvp_rows(const float *X, int64_t ldx, const float *Y, int64_t ldy, const float *A, const float *B,
                                      const float *Ay, const float *By, int d, const int32_t *row_ids, int rows, int n, int m,
                                      const int64_t *pos_off, const int32_t *pos_items, int64_t entries,
                                      const int64_t *excl_off, const int32_t *excl_items, int64_t excl_entries,
                                      const float *coef, float *q, int64_t ldq, float *deg, int64_t ldd, int32_t *status,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    const bool dense = X != nullptr;
    if (dense ? (!Y || A || B || Ay || By) : (Y || !A || !B || !Ay || !By || d < 1)) return MFCD_EINVAL;
    if (!implicit_sizes_ok(rows, m, dense ? 0 : d) || entries < 0 || n < 1 || excl_entries < 0) return MFCD_EINVAL;
    if (dense && (ldx < m || ldy < m)) return MFCD_EINVAL;
    if (ldq < m || (deg && ldd < m)) return MFCD_EINVAL;
    if (!dense && ((int64_t)n * d >= ((int64_t)1 << 40) || (int64_t)m * d >= ((int64_t)1 << 40))) return MFCD_EINVAL;
    if (rows > 0 && (!pos_off || !q || !status)) return MFCD_EINVAL;
    if (entries > 0 && !pos_items) return MFCD_EINVAL;
    if ((excl_off == nullptr) != (excl_items == nullptr)) return MFCD_EINVAL;
    const size_t need = implicit_hvp_bytes(rows, m, dense);
    {
        const size_t rb = (size_t)rows * 4, fa = dense ? 0 : (size_t)n * d * 4, fb = dense ? 0 : (size_t)m * d * 4;
        const struct { const void *p; size_t bytes; } out[] = {{q, (size_t)rows * (size_t)ldq * 4},
                                                               {deg, (size_t)rows * (size_t)ldd * 4}, {status, rb},
                                                               {workspace, need}},
            in[] = {{X, (size_t)n * (size_t)(dense ? ldx : 0) * 4}, {Y, (size_t)n * (size_t)(dense ? ldy : 0) * 4}, {A, fa},
                    {B, fb}, {Ay, fa}, {By, fb}, {row_ids, rb}, {pos_off, rb * 2 + 8}, {pos_items, (size_t)entries * 4},
                    {excl_off, rb * 2 + 8}, {excl_items, (size_t)excl_entries * 4}, {coef, rb}};
        for (int i = 0; i < 4; ++i) {
            for (const auto &v : in)
                if (implicit_overlap(out[i].p, out[i].bytes, v.p, v.bytes)) return MFCD_EINVAL;
            for (int j = 0; j < i; ++j)
                if (implicit_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return MFCD_EINVAL;
        }
    }
    if (((uintptr_t)X | (uintptr_t)Y | (uintptr_t)A | (uintptr_t)B | (uintptr_t)Ay | (uintptr_t)By | (uintptr_t)row_ids |
         (uintptr_t)pos_items | (uintptr_t)excl_items | (uintptr_t)coef | (uintptr_t)q | (uintptr_t)deg | (uintptr_t)status) & 3)
        return MFCD_EALIGN;
    if (((uintptr_t)pos_off | (uintptr_t)excl_off) & 7) return MFCD_EALIGN;
    if (workspace && ((uintptr_t)workspace & 255)) return MFCD_EALIGN;
    if (!workspace || workspace_bytes < need) return MFCD_EWORKSPACE;
    if (rows == 0) return 0;

    hipStream_t st = (hipStream_t)stream;
    const size_t slab = implicit_slab_bytes(rows, m, dense);
    float *SX = static_cast<float *>(workspace), *SYs = reinterpret_cast<float *>(static_cast<char *>(workspace) + slab);
    ImplicitArgs a = {};
    a.S = dense ? X : SX;
    a.ld = dense ? ldx : slab_ld(m);
    a.SY = dense ? Y : SYs;
    a.ldy = dense ? ldy : slab_ld(m);
    a.by_id = dense ? 1 : 0;
    a.row_ids = row_ids; a.rows = rows; a.n = n; a.m = m; a.chunks = implicit_chunks(m);
    a.slots = std::min((m + kImpTile - 1) / kImpTile, kImpMaxSlots);
    a.pos_off = pos_off; a.pos_items = pos_items; a.entries = entries;
    a.excl_off = excl_off; a.excl_items = excl_items; a.excl_entries = excl_entries;
    a.coef = coef; a.g = q; a.ldg = ldq; a.deg = deg; a.ldd = ldd; a.status = status;
    a.bad = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + 2 * slab);
    hipLaunchKernelGGL(implicit_prepare_kernel, dim3((unsigned)rows), dim3(kImpThreads), 0, st, a);
    MFCD_HIP_TRY(hipGetLastError());

    const int rb = implicit_block_rows(rows, m, dense);
    for (int r0 = 0; r0 < rows; r0 += rb) {
        const int nb = rows - r0 < rb ? rows - r0 : rb;
        if (!dense) {
            const dim3 grid((unsigned)((m + kBlk - 1) / kBlk), (unsigned)((nb + kBlk - 1) / kBlk));
            hipLaunchKernelGGL(topk_scores_kernel, grid, dim3(256), 0, st, A, B, row_ids ? row_ids + r0 : nullptr, r0, nb, n,
                               m, d, SX, a.ld);
            MFCD_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(topk_scores_kernel, grid, dim3(256), 0, st, Ay, By, row_ids ? row_ids + r0 : nullptr, r0, nb,
                               n, m, d, SYs, a.ldy);
            MFCD_HIP_TRY(hipGetLastError());
        }
        const dim3 cols((unsigned)((int64_t)nb * a.chunks)), poss((unsigned)((int64_t)nb * a.slots));
        if (deg) {
            hipLaunchKernelGGL(implicit_hvp_col_kernel<true>, cols, dim3(kImpThreads), 0, st, a, r0);
            MFCD_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(implicit_hvp_pos_kernel<true>, poss, dim3(kImpThreads), 0, st, a, r0, nb);
        } else {
            hipLaunchKernelGGL(implicit_hvp_col_kernel<false>, cols, dim3(kImpThreads), 0, st, a, r0);
            MFCD_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(implicit_hvp_pos_kernel<false>, poss, dim3(kImpThreads), 0, st, a, r0, nb);
        }
        MFCD_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(implicit_hvp_finish_kernel, dim3((unsigned)nb), dim3(kImpThreads), 0, st, a, r0);
        MFCD_HIP_TRY(hipGetLastError());
    }
    return 0;
}
