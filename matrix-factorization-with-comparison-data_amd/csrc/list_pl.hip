// list_pl.hip — the Plackett–Luce loss of ranked lists over ragged rows and its gradient in the scores
// (include/mfcd.h: mfcd_list_pl).  A row is a CSR slice of the score array a, in rank order, best first;
// its first `stages` = min(depth, L - 1) entries are choices out of what remains:
//     lse_k = log sum_{l >= k} exp(a_l)                       a reverse scan
//     loss  = sum_{k < stages} (lse_k - a_k)
//     N_l   = log sum_{k <= l, k < stages} exp(-lse_k)        a forward scan
//     g_l   = exp(a_l + N_l) - [l < stages]
//     hits  = #{k < stages : a_k >= a_l for every l >= k}
// Both scans run over the log-sum-exp monoid kept as (max, sum scaled by exp(-max)) pairs in f64, joined as an online
// softmax joins them: every exponent is <= 0, so nothing overflows and no suffix sum underflows to 0, whatever the spread
// of the scores (exp(a - row max) followed by a plain suffix sum loses exactly the well-fitted rows).  A pair is never
// folded into one number on the way: the forward scan takes exp(-lse_k) as (-max_k, 1 / sum_k), the loss term is
// (max_k - a_k) + log sum_k and g_l = exp(a_l + M_l) S_l - [l < stages], so scores of the size of 3e38, next to which a
// log of a count would vanish even in f64, lose nothing.  g is rounded to fp32 once.
//
// A row is cut into tiles of kPlTile = 256 entries, one entry per thread, one 256-thread workgroup per tile, which finds
// its row by binary search in tile_off as pair_ragged.hip does.  Reduce-then-scan over a row's tiles, in stream order:
//   status      one wave per row: validation, before anything reads the row; the outputs of failed and of empty rows
//   aggregate   per tile of a row of >= 2 tiles: the tile's reverse aggregate and whether it holds a non-finite score
//   carry 1     one wave per such row: the aggregate of the tiles after each tile, the row's non-finite flag
//   middle      per tile of such a row: lse_k, the tile's loss and hit partials, its forward aggregate
//   carry 2     one wave per such row: the aggregate of the tiles before each tile; the row's loss and hits, the
//               partials added in tile order
//   final       per tile: g of a row of >= 2 tiles; a row of one tile does both scans here and writes all its outputs,
//               its workgroups return at once from the two passes above
// No workgroup waits on another: every dependency is a kernel boundary.  No floating-point atomics; every sum has one
// owner and a fixed order that depends on the row alone, so two calls are bit-equal, a row's bytes do not depend on its
// place in the call, and what = 1 / what = 2 are the matching halves of what = 3.  The tile kernels read status[r] and
// return for a row that failed: no address is formed from its offsets.
#include "list_common.h"

namespace {

struct PlTileRec {                                     // the workspace's record of one tile of a row of >= 2 tiles
    Lse rev, rev_carry;                                // the tile's reverse aggregate; that of the row's later tiles
    Lse fwd, fwd_carry;                                // the tile's forward aggregate; that of the row's earlier tiles
    double loss;                                       // sum of lse_k - a_k over the tile's stages
    long long hits;
    int bad, pad;                                      // a non-finite score in the tile
};

struct PlArgs {
    const float *a;
    int64_t entries;
    const int64_t *row_off, *tile_off;
    const int32_t *depth;
    int rows;
    int64_t n_tiles;
    int what;
    double *loss;
    int64_t *counts;
    float *g;
    int32_t *status;
    PlTileRec *tiles;
    int32_t *row_bad;
};

// One wave per row: the validation of the header, before anything reads the row, and the outputs of a row that failed
// or has no tile.
__global__ __launch_bounds__(256) void pl_status_kernel(const PlArgs g)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * kPlWaves + (threadIdx.x >> 6);
    if (rr >= g.rows) return;
    const int r = (int)rr;
    const bool ok = pl_row_valid(g.row_off, g.tile_off, g.depth, g.rows, g.entries, g.n_tiles, r, lane);
    if (lane != 0) return;
    g.status[r] = ok ? 0 : 2;
    if ((g.what & 1) && (!ok || g.row_off[r + 1] == g.row_off[r])) {
        g.loss[r] = ok ? 0.0 : pl_qnan();
        g.counts[2 * (int64_t)r] = g.counts[2 * (int64_t)r + 1] = ok ? 0 : -1;
    }
}

// Sums over the workgroup → thread 0: the waves by the xor butterfly, the wave sums in ascending order.
__device__ __forceinline__ void pl_block_sum(double &x, long long &c, int tid, double (&shx)[kPlWaves],
                                             long long (&shc)[kPlWaves])
{
    x = wave_sum_xor(x);
    c = wave_sum_xor(c);
    __syncthreads();
    if ((tid & 63) == 0) {
        shx[tid >> 6] = x;
        shc[tid >> 6] = c;
    }
    __syncthreads();
    x = shx[0];
    c = shc[0];
    for (int w = 1; w < kPlWaves; ++w) {
        x += shx[w];
        c += shc[w];
    }
}

// PHASE 0: aggregate, 1: middle, 2: final (the header).
template <int PHASE>
__global__ __launch_bounds__(kPlTile) void pl_tile_kernel(const PlArgs g, int64_t t0)
{
    __shared__ Lse sh[kPlWaves];
    __shared__ double shx[kPlWaves];
    __shared__ long long shc[kPlWaves];
    const int tid = threadIdx.x;
    const int64_t t = t0 + blockIdx.x;
    PlTile w;
    if (!pl_tile(g, t, &w)) return;                    // uniform over the workgroup, as every return below
    const bool single = w.T == 1;
    if (PHASE < 2 && single) return;
    if (PHASE == 2 && !single && !(g.what & 2)) return;

    const int p = w.I * kPlTile + tid;
    const bool in = p < w.len;
    const float af = in ? g.a[w.b + p] : 0.0f;
    const double ai = (double)af;
    const Lse own = in ? Lse{ai, 1.0} : lse_none();
    PlTileRec *rec = g.tiles + t;                      // t < n_tiles: the row passed validation

    if (PHASE == 0) {
        const int bad = __syncthreads_or((int)(in && is_nonfinite_bits(af)));
        const Lse agg = pl_block_join(own, tid, sh);
        if (tid == 0) {
            rec->rev = agg;
            rec->bad = bad;
        }
        return;
    }

    int bad;
    if (single) bad = __syncthreads_or((int)(in && is_nonfinite_bits(af)));
    else bad = g.row_bad[w.r];
    if (bad) {                                         // the row's loss and counts: here if single, else carry 2's
        if (PHASE == 2) {
            if ((g.what & 2) && in) g.g[w.b + p] = __uint_as_float(0x7fc00000u);
            if (single && (g.what & 1) && tid == 0) {
                g.loss[w.r] = pl_qnan();
                g.counts[2 * (int64_t)w.r] = g.counts[2 * (int64_t)w.r + 1] = -1;
            }
        }
        return;
    }

    const Lse suf = pl_block_scan<true>(own, single ? lse_none() : rec->rev_carry, tid, sh);
    const bool staged = in && p < w.stages;            // suf.s >= 1 there: p's own term

    if (PHASE == 1 || (single && (g.what & 1))) {
        double term = staged ? (suf.m - ai) + log(suf.s) : 0.0;   // lse_p - a_p, the two large parts cancelled first
        long long hit = (long long)(staged && ai >= suf.m);  // suf.m is the largest score from p on, p's own included
        pl_block_sum(term, hit, tid, shx, shc);
        if (tid == 0) {
            if (PHASE == 1) {
                rec->loss = term;
                rec->hits = hit;
            } else {
                g.loss[w.r] = term;
                g.counts[2 * (int64_t)w.r] = w.stages;
                g.counts[2 * (int64_t)w.r + 1] = hit;
            }
        }
    }

    const Lse mine = staged ? Lse{-suf.m, 1.0 / suf.s} : lse_none();   // exp(-lse_p), max and sum still apart
    if (PHASE == 1) {
        const Lse agg = pl_block_join(mine, tid, sh);
        if (tid == 0) rec->fwd = agg;
        return;
    }
    if (!(g.what & 2)) return;
    const Lse pre = pl_block_scan<false>(mine, single ? lse_none() : rec->fwd_carry, tid, sh);
    if (!in) return;
    float out = 0.0f;                                  // no stage: exactly +0
    // a_p + pre.m <= 0: pre.m is minus the smallest suffix maximum of the stages up to p, none of them below a_p
    if (w.stages > 0) out = (float)(exp(ai + pre.m) * pre.s - (staged ? 1.0 : 0.0));
    g.g[w.b + p] = out;
}

// One wave per row of >= 2 tiles, 64 tiles at a time.  SECOND = false: rev_carry of every tile, from the row's end, and
// the row's non-finite flag.  SECOND = true: fwd_carry of every tile, from the row's start, and the row's loss and counts.
template <bool SECOND>
__global__ __launch_bounds__(256) void pl_carry_kernel(const PlArgs g)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * kPlWaves + (threadIdx.x >> 6);
    if (rr >= g.rows) return;
    const int r = (int)rr;
    if (g.status[r] != 0) return;
    const int64_t s0 = g.tile_off[r];
    const int T = (int)(g.tile_off[r + 1] - s0);
    if (T < 2) return;
    PlTileRec *rec = g.tiles + s0;
    if (SECOND && g.row_bad[r]) {
        if ((g.what & 1) && lane == 0) {
            g.loss[r] = pl_qnan();
            g.counts[2 * (int64_t)r] = g.counts[2 * (int64_t)r + 1] = -1;
        }
        return;
    }
    const int chunks = (T + MFCD_WAVE - 1) / MFCD_WAVE;
    Lse run = lse_none();
    int bad = 0;
    double loss = 0.0;
    long long hits = 0;
    for (int c = 0; c < chunks; ++c) {
        const int q = (SECOND ? c : chunks - 1 - c) * MFCD_WAVE + lane;
        const bool in = q < T;
        const Lse own = in ? (SECOND ? rec[q].fwd : rec[q].rev) : lse_none();
        const Lse inc = lse_wave_scan<!SECOND>(own, lane);
        const int nb = SECOND ? lane - 1 : lane + 1;   // the exclusive scan: the neighbour's inclusive one
        Lse exc = lse_shfl(inc, nb & (MFCD_WAVE - 1));
        if (nb < 0 || nb >= MFCD_WAVE) exc = lse_none();
        exc = lse_join(exc, run);
        if (in) {
            if (SECOND) rec[q].fwd_carry = exc;
            else rec[q].rev_carry = exc;
        }
        run = lse_join(lse_shfl(inc, SECOND ? MFCD_WAVE - 1 : 0), run);
        if (SECOND) {
            loss += wave_sum_xor(in ? rec[q].loss : 0.0);
            hits += wave_sum_xor(in ? rec[q].hits : 0ll);
        } else {
            bad |= (int)(__ballot(in && rec[q].bad != 0) != 0);
        }
    }
    if (lane != 0) return;
    if (!SECOND) {
        g.row_bad[r] = bad;
    } else if (g.what & 1) {
        const int64_t len = g.row_off[r + 1] - g.row_off[r];
        const int64_t depth = g.depth ? g.depth[r] : len;
        g.loss[r] = loss;
        g.counts[2 * (int64_t)r] = depth < len - 1 ? depth : len - 1;
        g.counts[2 * (int64_t)r + 1] = hits;
    }
}

inline size_t pl_tiles_bytes(int64_t n_tiles) { return align_up((size_t)(n_tiles > 0 ? n_tiles : 1) * sizeof(PlTileRec)); }

}  // namespace

extern "C" int mfcd_list_pl_tile(void) { return kPlTile; }

extern "C" size_t mfcd_list_pl_workspace_bytes(int rows, int64_t n_tiles)
{
    if (rows < 0 || n_tiles < 0 || n_tiles > (int64_t)1 << 40) return 0;
    return pl_tiles_bytes(n_tiles) + align_up((size_t)(rows > 0 ? rows : 1) * sizeof(int32_t));
}

extern "C" int mfcd_list_pl(const float *a, int64_t entries, const int64_t *row_off, const int32_t *depth, int rows,
                            const int64_t *tile_off, int64_t n_tiles, int what, double *loss, int64_t *counts, float *g_out,
                            int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    if (rows < 0 || entries < 0 || n_tiles < 0 || !row_off || !tile_off || !status) return MFCD_EINVAL;
    if (entries > 0 && !a) return MFCD_EINVAL;
    if (what < 1 || what > 3 || ((what & 1) && (!loss || !counts))) return MFCD_EINVAL;
    if ((what & 2) && entries > 0 && (!g_out || g_out == a)) return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    const size_t need = mfcd_list_pl_workspace_bytes(rows, n_tiles);
    if (need == 0) return MFCD_EINVAL;
    if (workspace_bytes < need) return MFCD_EWORKSPACE;
    PlArgs g{a, entries, row_off, tile_off, depth, rows, n_tiles, what, loss, counts, g_out, status,
             (PlTileRec *)workspace, (int32_t *)((char *)workspace + pl_tiles_bytes(n_tiles))};
    hipStream_t st = (hipStream_t)stream;
    const dim3 row_grid((unsigned)(((int64_t)rows + kPlWaves - 1) / kPlWaves));
    const auto tiles = [&](void (*kernel)(PlArgs, int64_t)) {
        return pair_chunks(n_tiles, kPairMaxBlocks, [&](int64_t t0, int64_t nb) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(kPlTile), 0, st, g, t0);
            return (int)hipGetLastError();
        });
    };
    hipLaunchKernelGGL(pl_status_kernel, row_grid, dim3(256), 0, st, g);
    MFCD_HIP_TRY(hipGetLastError());
    if (n_tiles >= 2) {                                // a row of >= 2 tiles needs that many
        if (int rc = tiles(pl_tile_kernel<0>)) return rc;
        hipLaunchKernelGGL(pl_carry_kernel<false>, row_grid, dim3(256), 0, st, g);
        MFCD_HIP_TRY(hipGetLastError());
        if (int rc = tiles(pl_tile_kernel<1>)) return rc;
        hipLaunchKernelGGL(pl_carry_kernel<true>, row_grid, dim3(256), 0, st, g);
        MFCD_HIP_TRY(hipGetLastError());
    }
    return tiles(pl_tile_kernel<2>);
}
