// list_pl_hvp.hip — the Hessian of the Plackett–Luce list loss in the scores, applied to a score-space vector, and its
// diagonal (include/mfcd.h: mfcd_list_pl_hvp).  Rows, depth and stages as in list_pl.hip.  With
//     p_{k,l} = exp(a_l - lse_k) for l >= k,      ybar_k = sum_{j >= k} p_{k,j} y_j
//     q_l   = sum_{k <= l, k < stages} p_{k,l} (y_l - ybar_k)
//     deg_l = sum_{k <= l, k < stages} p_{k,l} (1 - p_{k,l})
// these are list_pl.hip's two scans with a linear payload riding along (list_common.h: LseY).  The reverse scan joins
// (a_j, 1, y_j) into (m_k, s_k, t_k), t_k = sum_{j >= k} exp(a_j - m_k) y_j, so ybar_k = t_k / s_k; the forward scan joins
// the stages' (-m_k, 1 / s_k, ybar_k / s_k) into (M_l, S_l, W_l) and q_l = exp(a_l + M_l) (y_l S_l - W_l), the exponent
// <= 0 as in the gradient.  The diagonal takes a second forward scan, of (-2 m_k, 1 / s_k^2) into (M2_l, S2_l):
// deg_l = exp(a_l + M_l) S_l - exp(2 a_l + M2_l) S2_l, held at 0 from below (it feeds a Jacobi preconditioner).  m and s
// never see the payload: deg does not depend on y, and q is the same with or without deg.  All of it f64; q and deg are
// rounded to fp32 once.
//
// The decomposition is list_pl.hip's: status, then for rows of >= 2 tiles aggregate, carry 1, middle, carry 2, and the
// final pass, in which a row of one tile does everything.  Every dependency is a kernel boundary, no workgroup waits on
// another, no floating-point atomics, every sum has one owner and an order that depends on the row alone.
#include "list_common.h"

namespace {

struct HvTileRec {                                     // the workspace's record of one tile of a row of >= 2 tiles
    LseY rev, rev_carry;                               // the tile's reverse aggregate; that of the row's later tiles
    LseY fwd, fwd_carry;                               // the tile's forward aggregate; that of the row's earlier tiles
    Lse fwd2, fwd2_carry;                              // the same of the diagonal's second scan (deg asked for)
    int bad, pad;                                      // a non-finite score or y in the tile
};

struct HvArgs {
    const float *a, *y;
    int64_t entries;
    const int64_t *row_off, *tile_off;
    const int32_t *depth;
    int rows;
    int64_t n_tiles;
    float *q, *deg;
    int32_t *status;
    HvTileRec *tiles;
    int32_t *row_bad;
};

// One wave per row: the validation of the header, before anything reads the row.  A failed row gets no output.
__global__ __launch_bounds__(256) void hv_status_kernel(const HvArgs g)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * kPlWaves + (threadIdx.x >> 6);
    if (rr >= g.rows) return;
    const int r = (int)rr;
    const bool ok = pl_row_valid(g.row_off, g.tile_off, g.depth, g.rows, g.entries, g.n_tiles, r, lane);
    if (lane == 0) g.status[r] = ok ? 0 : 2;
}

// PHASE 0: aggregate, 1: middle, 2: final (the header).
template <int PHASE>
__global__ __launch_bounds__(kPlTile) void hv_tile_kernel(const HvArgs g, int64_t t0)
{
    __shared__ LseY sh[kPlWaves];
    __shared__ Lse sh2[kPlWaves];
    const int tid = threadIdx.x;
    const int64_t t = t0 + blockIdx.x;
    PlTile w;
    if (!pl_tile(g, t, &w)) return;                    // uniform over the workgroup, as every return before the last
    const bool single = w.T == 1;
    if (PHASE < 2 && single) return;

    const int p = w.I * kPlTile + tid;
    const bool in = p < w.len;
    const float af = in ? g.a[w.b + p] : 0.0f, yf = in ? g.y[w.b + p] : 0.0f;
    const double ai = (double)af, yi = (double)yf;
    const LseY own = in ? LseY{ai, 1.0, yi} : LseY::none();
    const int nonfinite = (int)(in && (is_nonfinite_bits(af) || is_nonfinite_bits(yf)));
    HvTileRec *rec = g.tiles + t;                      // t < n_tiles: the row passed validation

    if (PHASE == 0) {
        const int bad = __syncthreads_or(nonfinite);
        const LseY agg = pl_block_join(own, tid, sh);
        if (tid == 0) {
            rec->rev = agg;
            rec->bad = bad;
        }
        return;
    }

    int bad;
    if (single) bad = __syncthreads_or(nonfinite);
    else bad = g.row_bad[w.r];
    if (bad) {
        if (PHASE == 2 && in) {
            g.q[w.b + p] = __uint_as_float(0x7fc00000u);
            if (g.deg) g.deg[w.b + p] = __uint_as_float(0x7fc00000u);
        }
        return;
    }

    const LseY suf = pl_block_scan<true>(own, single ? LseY::none() : rec->rev_carry, tid, sh);
    const bool staged = in && p < w.stages;            // suf.s >= 1 there: p's own term
    const double inv = 1.0 / suf.s;                    // read where staged only
    const LseY mine = staged ? LseY{-suf.m, inv, (suf.t / suf.s) * inv} : LseY::none();   // exp(-lse_p) (1, ybar_p)
    const Lse mine2 = staged ? Lse{-2.0 * suf.m, inv * inv} : Lse::none();                // exp(-2 lse_p)

    if (PHASE == 1) {
        const LseY agg = pl_block_join(mine, tid, sh);
        if (tid == 0) rec->fwd = agg;
        if (g.deg) {
            const Lse agg2 = pl_block_join(mine2, tid, sh2);
            if (tid == 0) rec->fwd2 = agg2;
        }
        return;
    }

    const LseY pre = pl_block_scan<false>(mine, single ? LseY::none() : rec->fwd_carry, tid, sh);
    Lse pre2 = Lse::none();
    if (g.deg) pre2 = pl_block_scan<false>(mine2, single ? Lse::none() : rec->fwd2_carry, tid, sh2);
    if (!in) return;
    float q = 0.0f, dg = 0.0f;                         // no stage: exactly +0
    if (w.stages > 0) {
        // a_p + pre.m <= 0: pre.m is minus the smallest suffix maximum of the stages up to p, none of them below a_p;
        // pre2.m is twice it
        const double e1 = exp(ai + pre.m);
        q = (float)(e1 * (yi * pre.s - pre.t));
        if (g.deg) {
            const double h = e1 * pre.s - exp(2.0 * ai + pre2.m) * pre2.s;
            dg = (float)(h > 0.0 ? h : 0.0);
        }
    }
    g.q[w.b + p] = q;
    if (g.deg) g.deg[w.b + p] = dg;
}

// One wave: the exclusive scan of a row's T tile aggregates, 64 at a time, from the row's start (FORWARD) or its end.
template <bool FORWARD, class E>
__device__ __forceinline__ void hv_carry_scan(HvTileRec *rec, int T, int lane, E HvTileRec::*agg, E HvTileRec::*carry)
{
    const int chunks = (T + MFCD_WAVE - 1) / MFCD_WAVE;
    E run = E::none();
    for (int c = 0; c < chunks; ++c) {
        const int q = (FORWARD ? c : chunks - 1 - c) * MFCD_WAVE + lane;
        const bool in = q < T;
        const E own = in ? rec[q].*agg : E::none();
        const E inc = lse_wave_scan<!FORWARD>(own, lane);
        const int nb = FORWARD ? lane - 1 : lane + 1;  // the exclusive scan: the neighbour's inclusive one
        E exc = lse_shfl(inc, nb & (MFCD_WAVE - 1));
        if (nb < 0 || nb >= MFCD_WAVE) exc = E::none();
        exc = lse_join(exc, run);
        if (in) rec[q].*carry = exc;
        run = lse_join(lse_shfl(inc, FORWARD ? MFCD_WAVE - 1 : 0), run);
    }
}

// One wave per row of >= 2 tiles.  SECOND = false: rev_carry of every tile and the row's non-finite flag.  SECOND =
// true: fwd_carry (and fwd2_carry) of every tile.
template <bool SECOND>
__global__ __launch_bounds__(256) void hv_carry_kernel(const HvArgs g)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * kPlWaves + (threadIdx.x >> 6);
    if (rr >= g.rows) return;
    const int r = (int)rr;
    if (g.status[r] != 0) return;
    const int64_t s0 = g.tile_off[r];
    const int T = (int)(g.tile_off[r + 1] - s0);
    if (T < 2) return;
    HvTileRec *rec = g.tiles + s0;
    if (SECOND) {
        if (g.row_bad[r]) return;
        hv_carry_scan<true>(rec, T, lane, &HvTileRec::fwd, &HvTileRec::fwd_carry);
        if (g.deg) hv_carry_scan<true>(rec, T, lane, &HvTileRec::fwd2, &HvTileRec::fwd2_carry);
    } else {
        hv_carry_scan<false>(rec, T, lane, &HvTileRec::rev, &HvTileRec::rev_carry);
        int bad = 0;
        for (int q = lane; q - lane < T; q += MFCD_WAVE) bad |= (int)(__ballot(q < T && rec[q].bad != 0) != 0);
        if (lane == 0) g.row_bad[r] = bad;
    }
}

inline size_t hv_tiles_bytes(int64_t n_tiles) { return align_up((size_t)(n_tiles > 0 ? n_tiles : 1) * sizeof(HvTileRec)); }

}  // namespace

extern "C" size_t mfcd_list_pl_hvp_workspace_bytes(int rows, int64_t n_tiles)
{
    if (rows < 0 || n_tiles < 0 || n_tiles > (int64_t)1 << 40) return 0;
    return hv_tiles_bytes(n_tiles) + align_up((size_t)(rows > 0 ? rows : 1) * sizeof(int32_t));
}

extern "C" int mfcd_list_pl_hvp(const float *a, const float *y, int64_t entries, const int64_t *row_off, const int32_t *depth,
                                int rows, const int64_t *tile_off, int64_t n_tiles, float *q, float *deg, int32_t *status,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (rows < 0 || entries < 0 || n_tiles < 0 || !row_off || !tile_off || !status) return MFCD_EINVAL;
    if (entries > 0 && (!a || !y || !q)) return MFCD_EINVAL;
    if (q && (q == a || q == y)) return MFCD_EINVAL;
    if (deg && (deg == q || deg == a || deg == y)) return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    const size_t need = mfcd_list_pl_hvp_workspace_bytes(rows, n_tiles);
    if (need == 0) return MFCD_EINVAL;
    if (workspace_bytes < need) return MFCD_EWORKSPACE;
    HvArgs g{a, y, entries, row_off, tile_off, depth, rows, n_tiles, q, deg, status,
             (HvTileRec *)workspace, (int32_t *)((char *)workspace + hv_tiles_bytes(n_tiles))};
    hipStream_t st = (hipStream_t)stream;
    const dim3 row_grid((unsigned)(((int64_t)rows + kPlWaves - 1) / kPlWaves));
    const auto tiles = [&](void (*kernel)(HvArgs, int64_t)) {
        return pair_chunks(n_tiles, kPairMaxBlocks, [&](int64_t t0, int64_t nb) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(kPlTile), 0, st, g, t0);
            return (int)hipGetLastError();
        });
    };
    hipLaunchKernelGGL(hv_status_kernel, row_grid, dim3(256), 0, st, g);
    MFCD_HIP_TRY(hipGetLastError());
    if (n_tiles >= 2) {                                // a row of >= 2 tiles needs that many
        if (int rc = tiles(hv_tile_kernel<0>)) return rc;
        hipLaunchKernelGGL(hv_carry_kernel<false>, row_grid, dim3(256), 0, st, g);
        MFCD_HIP_TRY(hipGetLastError());
        if (int rc = tiles(hv_tile_kernel<1>)) return rc;
        hipLaunchKernelGGL(hv_carry_kernel<true>, row_grid, dim3(256), 0, st, g);
        MFCD_HIP_TRY(hipGetLastError());
    }
    return tiles(hv_tile_kernel<2>);
}
