// pair_ragged.hip — the all-pairs statistics, gradient and Hessian-vector product of pairs.hip over ragged rows
// (include/mfcd.h: mfcd_pair_ragged_stats, mfcd_pair_ragged_grad, mfcd_pair_ragged_hvp).  A row is a CSR slice: entries [row_off[r], row_off[r+1])
// of the value array x and of the score array a; all L (L - 1) / 2 pairs among a row's entries are visited, per row, and
// no pair is ever materialised.  The per-pair arithmetic is pairs_common.h's, the functions pairs.hip runs.
//
// A row is cut into tiles of kRagTile = 256 entries, one entry per thread, and one 256-thread workgroup takes one tile: it
// finds its row by binary search in tile_off (the prefix sum of the rows' tile counts), keeps its own entry in registers
// and streams the row's tiles through 2 KiB of LDS, every lane reading the same (a_j, x_j) — a broadcast.  A workgroup of
// a 100-entry row idles 156 lanes, not 924 as under the dense kernels' 1024-column tile, and its two waves that hold no
// entry skip the pair loops (they only help to stage the tiles): the work is granular in waves of 64 entries.
//   statistics  tile I against the tiles J >= I (each unordered pair once; the diagonal tile masked to i < j); one
//               fixed-size partial per tile; a one-wave finishing kernel per row adds the row's partials in order.
//   gradient    tile I against EVERY tile J, so a thread owns its sum and stores it itself (no finishing kernel).
//   Hessian     times a vector y, and its diagonal: the gradient's decomposition, (a, y) in LDS, x beside it under SKIP.
// A first kernel (one wave per row) validates every row before any entry of it is read and writes status[r]: 0, or 2 for
//   not (0 <= row_off[r] <= row_off[r+1] <= entries),  a length above 2^20,  a tile range that is not
//   ceil(L / 256) tiles inside [0, n_tiles),  or a tile of the range that the search does not lead back to the row.
// The tile kernels read status[r] and return for a row that failed: no address is formed from its offsets.
// fp32 runs of at most 64 terms are widened to f64; no floating-point atomics; every sum has a fixed order that depends
// on the row alone, so two calls are bit-equal and a row's bytes do not depend on its place in the call.
#include <cmath>

#include "common.h"
#include "pairs_common.h"

namespace {

constexpr int kRagTile = 256;                          // entries per tile = threads per workgroup (mfcd_pair_ragged_tile)
constexpr int kRagFlush = 64;                          // columns, = terms per accumulator, between two widenings to f64

struct RagArgs {
    const float *a, *x;
    int64_t entries;
    const int64_t *row_off, *tile_off;
    int rows;
    int64_t n_tiles;
    float scale;
    int32_t *status;
};

// One wave per row: the validation of the header, before anything reads the row.
__global__ __launch_bounds__(256) void ragged_status_kernel(const RagArgs g)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * (256 / MFCD_WAVE) + (threadIdx.x >> 6);
    if (rr >= g.rows) return;
    const int r = (int)rr;
    const int64_t b = g.row_off[r], e = g.row_off[r + 1], s0 = g.tile_off[r], s1 = g.tile_off[r + 1];
    bool ok = b >= 0 && e >= b && e <= g.entries && e - b <= kPairMaxCols && s0 >= 0 && s1 >= s0 && s1 <= g.n_tiles;
    if (ok) ok = s1 - s0 == (e - b + kRagTile - 1) / kRagTile;
    if (ok)                                            // at most 4096 tiles
        for (int64_t t = s0 + lane; t < s1; t += MFCD_WAVE) ok &= trip_find_row(g.tile_off, g.rows, t) == r;
    ok = __ballot(!ok) == 0;
    if (lane == 0) g.status[r] = ok ? 0 : 2;
}

// The tile's row and place in it, or false: nothing of a row that failed validation is touched.
struct RagTile {
    int r, I, T, len;   // row, tile of the row, tiles of the row, entries of the row
    int64_t b;          // the row's first entry
};

__device__ __forceinline__ bool ragged_tile(const RagArgs &g, int64_t t, RagTile *out)
{
    const int r = trip_find_row(g.tile_off, g.rows, t);
    if (g.status[r] != 0) return false;
    const int64_t s0 = g.tile_off[r], s1 = g.tile_off[r + 1];
    if (t < s0 || t >= s1) return false;
    out->r = r;
    out->I = (int)(t - s0);
    out->T = (int)(s1 - s0);
    out->b = g.row_off[r];
    out->len = (int)(g.row_off[r + 1] - out->b);
    return true;
}

// Columns [jb, je) of the LDS tile against this thread's entry; DIAG: the tile is the thread's own, column j pairs with
// entry tid only for tid < j.  SKIP: a pair tied in x leaves the sums (the counts follow their own rule).
template <int WHAT, bool SKIP, bool DIAG>
__device__ __forceinline__ void ragged_run(const float2 *tile, int jn, float ai, float xi, int tid, float scale,
                                           unsigned (&cnt)[4], double (&acc)[6])
{
    for (int jb = 0; jb < jn; jb += kRagFlush) {
        const int je = jb + kRagFlush < jn ? jb + kRagFlush : jn;
        float f[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // at most kRagFlush terms each
#pragma unroll 4
        for (int j = jb; j < je; ++j) {
            const float2 v = tile[j];
            const bool valid = !DIAG || tid < j;
            if (SKIP) {
                pair_term<(WHAT & 1), DIAG>(ai, xi, v.x, v.y, valid, scale, cnt, f);
                pair_term<(WHAT & 2), true>(ai, xi, v.x, v.y, valid && (xi < v.y || xi > v.y), scale, cnt, f);
            } else {
                pair_term<WHAT, DIAG>(ai, xi, v.x, v.y, valid, scale, cnt, f);
            }
        }
        if (WHAT & 2) {
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += (double)f[q];
        }
    }
}

template <int WHAT, bool SKIP>
__global__ __launch_bounds__(kRagTile) void ragged_tiles_kernel(const RagArgs g, int64_t t0, PairPartial *__restrict__ part)
{
    __shared__ float2 tile[kRagTile];
    const int tid = threadIdx.x;
    const int64_t t = t0 + blockIdx.x;
    RagTile w;
    if (!ragged_tile(g, t, &w)) return;                // uniform over the workgroup
    const float *a = g.a + w.b, *x = g.x + w.b;

    const int p = w.I * kRagTile + tid;
    float ai = 0.0f, xi = 0.0f;
    unsigned n_nan = 0, n_inf = 0;
    if (p < w.len) {
        ai = a[p];
        xi = x[p];
        n_nan = (unsigned)(ai != ai || xi != xi);
        n_inf = (unsigned)(is_nonfinite_bits(ai) || is_nonfinite_bits(xi));
    }

    // a wave whose 64 entries all lie past the row's end has no pair: a row of 60 entries costs one wave's work, not four
    const bool wave_live = w.I * kRagTile + (tid & ~63) < w.len;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};                // <= len <= 2^20 pairs per thread
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int J = w.I; J < w.T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
        const int pj = J * kRagTile + tid;
        float2 v = make_float2(ai, xi);                // J == I: the tile is this workgroup's own entries
        if (J != w.I) v = pj < w.len ? make_float2(a[pj], x[pj]) : make_float2(0.0f, 0.0f);
        tile[tid] = v;
        __syncthreads();
        const int jn = w.len - J * kRagTile < kRagTile ? w.len - J * kRagTile : kRagTile;   // entries of tile J that exist
        // a thread past the row's end only meets columns of its own tile at or below its own: tid < j bars them
        if (!wave_live) continue;                      // the wave only helps to stage the tiles
        if (J != w.I) ragged_run<WHAT, SKIP, false>(tile, jn, ai, xi, tid, g.scale, cnt, acc);
        else ragged_run<WHAT, SKIP, true>(tile, jn, ai, xi, tid, g.scale, cnt, acc);
    }

    long long c6[6] = {(long long)cnt[0], (long long)cnt[1], (long long)cnt[2], (long long)cnt[3], (long long)n_nan,
                       (long long)n_inf};
    pair_block_sum<kRagTile / 64>(tid, c6, acc, [&](const long long(&c)[6], const double(&s)[6]) {
        PairPartial out;
        for (int q = 0; q < 4; ++q) out.c[q] = c[q];
        out.bad[0] = c[4];
        out.bad[1] = c[5];
        out.s[0] = 0.6931471805599453 * s[0] + s[1];
        out.s[1] = 0.6931471805599453 * s[2] + s[3];
        out.s[2] = s[4];
        out.s[3] = s[5];
        part[t] = out;
    });
}

// One wave per row: lane l adds the partials of the row's tiles l, l + 64, ... in order, then the lanes are added in a
// fixed tree; or the outputs of a row that failed validation.
__global__ __launch_bounds__(256) void ragged_finish_kernel(const RagArgs g, const PairPartial *__restrict__ part, int what,
                                                            int64_t *__restrict__ counts, double *__restrict__ sums)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 / MFCD_WAVE) + (threadIdx.x >> 6);
    if (r >= g.rows) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (g.status[r] != 0) {
        if (lane < 4) {
            if (what & 1) counts[r * 4 + lane] = -1;
            if (what & 2) sums[r * 4 + lane] = qnan;
        }
        return;
    }
    const int64_t s0 = g.tile_off[r], s1 = g.tile_off[r + 1];
    const long long len = g.row_off[r + 1] - g.row_off[r], n0 = len * (len - 1) / 2;
    long long c6[6] = {0, 0, 0, 0, 0, 0};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = s0 + lane; t < s1; t += MFCD_WAVE) {
        const PairPartial &p = part[t];
        for (int q = 0; q < 4; ++q) c6[q] += p.c[q];
        c6[4] += p.bad[0];
        c6[5] += p.bad[1];
        for (int q = 0; q < 4; ++q) s[q] += p.s[q];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) c6[q] = wave_sum_xor(c6[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = wave_sum_xor(s[q]);
    if (lane == 0) {
        if (what & 1)
            for (int q = 0; q < 4; ++q) counts[r * 4 + q] = c6[4] ? -1 : q < 2 ? c6[q] : n0 - c6[q];
        if (what & 2)
            for (int q = 0; q < 4; ++q) sums[r * 4 + q] = c6[5] ? qnan : s[q];
    }
}

// g_e = sum over the other entries l of e's row of w_el (sigmoid(a_e - a_l) - sigmoid(scale (x_e - x_l))), w_el = 1, or
// with SKIP [x_e != x_l].  The column l == e needs no mask: both differences are +-0 there and the term is exactly +0.
template <bool SKIP>
__global__ __launch_bounds__(kRagTile) void ragged_grad_kernel(const RagArgs g, int64_t t0, float *__restrict__ G)
{
    __shared__ float2 tile[kRagTile];
    const int tid = threadIdx.x;
    RagTile w;
    if (!ragged_tile(g, t0 + blockIdx.x, &w)) return;  // uniform over the workgroup
    const float *a = g.a + w.b, *x = g.x + w.b;

    const int p = w.I * kRagTile + tid;
    const float ai = p < w.len ? a[p] : 0.0f, xi = p < w.len ? x[p] : 0.0f;   // past the end: computed, never stored
    const bool wave_live = w.I * kRagTile + (tid & ~63) < w.len;           // as in the statistics kernel
    int bad = 0;                                       // the workgroup stages the whole row: it sees every entry
    double acc = 0.0;
    for (int J = 0; J < w.T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
        const int pj = J * kRagTile + tid;
        const float2 v = pj < w.len ? make_float2(a[pj], x[pj]) : make_float2(0.0f, 0.0f);
        bad |= (int)(is_nonfinite_bits(v.x) || is_nonfinite_bits(v.y));
        tile[tid] = v;
        __syncthreads();
        const int jn = w.len - J * kRagTile < kRagTile ? w.len - J * kRagTile : kRagTile;   // pad columns stay out
        if (!wave_live) continue;                      // the wave only helps to stage the tiles
        for (int jb = 0; jb < jn; jb += kRagFlush) {
            const int je = jb + kRagFlush < jn ? jb + kRagFlush : jn;
            float f = 0.0f;
#pragma unroll 4
            for (int j = jb; j < je; ++j) {
                const float2 u = tile[j];
                const float term = pair_sigmoid(ai - u.x) - pair_sigmoid(g.scale * (xi - u.y));
                f += SKIP && !(xi < u.y || xi > u.y) ? 0.0f : term;
            }
            acc += (double)f;
        }
    }
    bad = __syncthreads_or(bad);
    if (p < w.len) G[w.b + p] = bad ? __uint_as_float(0x7fc00000u) : (float)acc;   // rounded to fp32 once
}

// q_e = sum over the other entries l of e's row of w_el s_el (y_e - y_l), s_el = sigmoid'(a_e - a_l), and with DEG
// deg_e = sum over l != e of w_el s_el: the row Laplacian L(a) of the ragged risk applied to y, and its diagonal.  The
// decomposition is ragged_grad_kernel's, the pair is pairs.hip's hvp_run's (pair_curvature, the difference of y formed
// first, then one fma).  Columns [0, jn) of the LDS tile against this thread's entry.  OWN: the tile is the thread's own;
// its own column (column tid) adds exactly 0 to q but 1/4 to deg, so with DEG s is zeroed there — a compare the other
// tiles do not carry.  SKIP: a pair tied in x has w = 0.
template <bool DEG, bool SKIP, bool OWN>
__device__ __forceinline__ void ragged_hvp_run(const float2 *tile, const float *tx, int jn, float ai, float yi, float xi,
                                               int tid, double &acc, double &dacc)
{
    for (int jb = 0; jb < jn; jb += kRagFlush) {
        const int je = jb + kRagFlush < jn ? jb + kRagFlush : jn;
        float f = 0.0f, d = 0.0f;                      // at most kRagFlush terms each
#pragma unroll 4
        for (int j = jb; j < je; ++j) {
            const float2 v = tile[j];
            float s = pair_curvature(ai - v.x);
            if (SKIP) {
                const float xj = tx[j];
                s = (xi < xj || xi > xj) ? s : 0.0f;
            }
            if (DEG && OWN) s = j == tid ? 0.0f : s;
            f = fmaf(s, yi - v.y, f);
            if (DEG) d += s;
        }
        acc += (double)f;
        if (DEG) dacc += (double)d;
    }
}

template <bool DEG, bool SKIP>
__global__ __launch_bounds__(kRagTile) void ragged_hvp_kernel(const RagArgs g, const float *__restrict__ Y, int64_t t0,
                                                              float *__restrict__ Q, float *__restrict__ Dg)
{
    __shared__ float2 tile[kRagTile];                  // (a, y)
    __shared__ float tx[SKIP ? kRagTile : 1];
    const int tid = threadIdx.x;
    RagTile w;
    if (!ragged_tile(g, t0 + blockIdx.x, &w)) return;  // uniform over the workgroup
    const float *a = g.a + w.b, *y = Y + w.b, *x = SKIP ? g.x + w.b : nullptr;

    const int p = w.I * kRagTile + tid;
    const bool in = p < w.len;                         // past the end: computed, never stored
    const float ai = in ? a[p] : 0.0f, yi = in ? y[p] : 0.0f, xi = SKIP && in ? x[p] : 0.0f;
    const bool wave_live = w.I * kRagTile + (tid & ~63) < w.len;           // as in the statistics kernel
    int bad = 0;                                       // the workgroup stages the whole row: it sees every entry
    double acc = 0.0, dacc = 0.0;
    for (int J = 0; J < w.T; ++J) {
        __syncthreads();                               // the previous tile's readers are done
        const int pj = J * kRagTile + tid;
        const bool inj = pj < w.len;
        const float2 v = inj ? make_float2(a[pj], y[pj]) : make_float2(0.0f, 0.0f);
        bad |= (int)(is_nonfinite_bits(v.x) || is_nonfinite_bits(v.y));
        tile[tid] = v;
        if (SKIP) {
            const float vx = inj ? x[pj] : 0.0f;
            bad |= (int)is_nonfinite_bits(vx);
            tx[tid] = vx;
        }
        __syncthreads();
        const int jn = w.len - J * kRagTile < kRagTile ? w.len - J * kRagTile : kRagTile;   // pad columns stay out
        if (!wave_live) continue;                      // the wave only helps to stage the tiles
        if (J != w.I) ragged_hvp_run<DEG, SKIP, false>(tile, tx, jn, ai, yi, xi, tid, acc, dacc);
        else ragged_hvp_run<DEG, SKIP, true>(tile, tx, jn, ai, yi, xi, tid, acc, dacc);
    }
    bad = __syncthreads_or(bad);
    if (in) {                                          // rounded to fp32 once
        Q[w.b + p] = bad ? __uint_as_float(0x7fc00000u) : (float)acc;
        if (DEG) Dg[w.b + p] = bad ? __uint_as_float(0x7fc00000u) : (float)dacc;
    }
}

// The checks the three entries share → 0, or MFCD_EINVAL; fills the kernels' arguments.  need_x: whether x is read (the
// Hessian reads it under the skip flag only, and has no scale: it passes 0).
inline int ragged_args(const float *a, const float *x, bool need_x, int64_t entries, const int64_t *row_off, int rows,
                       const int64_t *tile_off, int64_t n_tiles, double scale, int flags, int32_t *status, RagArgs *out)
{
    if (rows < 0 || entries < 0 || n_tiles < 0 || !row_off || !tile_off || !status) return MFCD_EINVAL;
    if (entries > 0 && (!a || (need_x && !x))) return MFCD_EINVAL;
    if (flags & ~MFCD_RAGGED_SKIP_TIES) return MFCD_EINVAL;
    if (!std::isfinite(scale) || !std::isfinite((float)scale)) return MFCD_EINVAL;
    *out = RagArgs{a, x, entries, row_off, tile_off, rows, n_tiles, (float)scale, status};
    return 0;
}

// What every entry launches: the validation of the rows, then launch(t0, grid) over the tiles in blocks of kPairMaxBlocks.
template <class F>
int ragged_launch(const RagArgs &g, hipStream_t st, F launch)
{
    hipLaunchKernelGGL(ragged_status_kernel, dim3((unsigned)(((int64_t)g.rows + 3) / 4)), dim3(256), 0, st, g);
    MFCD_HIP_TRY(hipGetLastError());
    return pair_chunks(g.n_tiles, kPairMaxBlocks, [&](int64_t t0, int64_t nb) {
        launch(t0, dim3((unsigned)nb));
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" int mfcd_pair_ragged_tile(void) { return kRagTile; }

extern "C" size_t mfcd_pair_ragged_workspace_bytes(int rows, int64_t n_tiles)
{
    if (rows < 0 || n_tiles < 0 || n_tiles > (int64_t)1 << 40) return 0;
    return align_up((size_t)(n_tiles > 0 ? n_tiles : 1) * sizeof(PairPartial));
}

extern "C" int mfcd_pair_ragged_stats(const float *a, const float *x, int64_t entries, const int64_t *row_off, int rows,
                                      const int64_t *tile_off, int64_t n_tiles, double scale, int flags, int what,
                                      int64_t *counts, double *sums, int32_t *status, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    RagArgs g;
    if (ragged_args(a, x, true, entries, row_off, rows, tile_off, n_tiles, scale, flags, status, &g)) return MFCD_EINVAL;
    if (what < 1 || what > 3 || ((what & 1) && !counts) || ((what & 2) && !sums)) return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    const size_t need = mfcd_pair_ragged_workspace_bytes(rows, n_tiles);
    if (need == 0) return MFCD_EINVAL;
    if (workspace_bytes < need) return MFCD_EWORKSPACE;
    PairPartial *part = (PairPartial *)workspace;
    hipStream_t st = (hipStream_t)stream;
    void (*const kernels[2][3])(RagArgs, int64_t, PairPartial *) = {
        {ragged_tiles_kernel<1, false>, ragged_tiles_kernel<2, false>, ragged_tiles_kernel<3, false>},
        {ragged_tiles_kernel<1, true>, ragged_tiles_kernel<2, true>, ragged_tiles_kernel<3, true>}};
    const auto tiles = kernels[(flags & MFCD_RAGGED_SKIP_TIES) != 0][what - 1];
    if (int rc = ragged_launch(g, st, [&](int64_t t0, dim3 grid) {
            hipLaunchKernelGGL(tiles, grid, dim3(kRagTile), 0, st, g, t0, part);
        }))
        return rc;
    hipLaunchKernelGGL(ragged_finish_kernel, dim3((unsigned)(((int64_t)rows + 3) / 4)), dim3(256), 0, st, g, part, what,
                       counts, sums);
    return (int)hipGetLastError();
}

extern "C" int mfcd_pair_ragged_grad(const float *a, const float *x, int64_t entries, const int64_t *row_off, int rows,
                                     const int64_t *tile_off, int64_t n_tiles, double scale, int flags, float *g_out,
                                     int32_t *status, void *stream)
{
    RagArgs g;
    if (ragged_args(a, x, true, entries, row_off, rows, tile_off, n_tiles, scale, flags, status, &g)) return MFCD_EINVAL;
    if (entries > 0 && !g_out) return MFCD_EINVAL;
    if (g_out && (g_out == a || g_out == x)) return MFCD_EINVAL;
    if (n_tiles > (int64_t)1 << 40) return MFCD_EINVAL;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const auto kernel = flags & MFCD_RAGGED_SKIP_TIES ? ragged_grad_kernel<true> : ragged_grad_kernel<false>;
    return ragged_launch(g, st, [&](int64_t t0, dim3 grid) {
        hipLaunchKernelGGL(kernel, grid, dim3(kRagTile), 0, st, g, t0, g_out);
    });
}

extern "C" int mfcd_pair_ragged_hvp(const float *a, const float *x, const float *y, int64_t entries, const int64_t *row_off,
                                    int rows, const int64_t *tile_off, int64_t n_tiles, int flags, float *q, float *deg,
                                    int32_t *status, void *stream)
{
    const bool skip = (flags & MFCD_RAGGED_SKIP_TIES) != 0;   // x is read under the skip flag only
    RagArgs g;
    if (ragged_args(a, x, skip, entries, row_off, rows, tile_off, n_tiles, 0.0, flags, status, &g)) return MFCD_EINVAL;
    if (entries > 0 && (!y || !q)) return MFCD_EINVAL;
    if (q && (q == a || q == y || q == x || q == deg)) return MFCD_EINVAL;
    if (deg && (deg == a || deg == y || deg == x)) return MFCD_EINVAL;
    if (n_tiles > (int64_t)1 << 40) return MFCD_EINVAL;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const auto kernel = deg ? (skip ? ragged_hvp_kernel<true, true> : ragged_hvp_kernel<true, false>)
                            : (skip ? ragged_hvp_kernel<false, true> : ragged_hvp_kernel<false, false>);
    return ragged_launch(g, st, [&](int64_t t0, dim3 grid) {
        hipLaunchKernelGGL(kernel, grid, dim3(kRagTile), 0, st, g, y, t0, q, deg);
    });
}
