// list_common.h — what the ranked-list kernels share (list_pl.hip: mfcd_list_pl; list_pl_hvp.hip: mfcd_list_pl_hvp): the
// log-sum-exp monoid with its one join, the wave and workgroup scans over it, the validation of a row's header and the
// tile's way to its row.  DESIGN §3.20, §3.21.
#pragma once
#include <cmath>

#include "common.h"
#include "pairs_common.h"

namespace {

constexpr int kPlTile = 256;                           // entries per tile = threads per workgroup (mfcd_list_pl_tile)
constexpr int kPlWaves = kPlTile / MFCD_WAVE;

// An element of the monoid: log of a sum of exponentials, as m + log(s).  The identity has s = 0 and an m below every
// finite score and every -lse: joined with anything its side is scaled by exp(-huge) = 0, with itself by exp(0) = 1.
struct Lse {
    double m, s;
    static __device__ __forceinline__ Lse none() { return Lse{-1.0e300, 0.0}; }
    // `keep` holds the larger maximum hi, `fade` is scaled by e = exp(its maximum - hi)
    static __device__ __forceinline__ Lse mix(double hi, const Lse keep, const Lse fade, double e)
    {
        return Lse{hi, keep.s + fade.s * e};
    }
    static __device__ __forceinline__ Lse shfl(const Lse v, int src)
    {
        return Lse{__shfl(v.m, src, MFCD_WAVE), __shfl(v.s, src, MFCD_WAVE)};
    }
};
__device__ __forceinline__ Lse lse_none() { return Lse::none(); }

// The same with a linear payload riding along: t = sum of exp(a_j - m) y_j beside s = sum of exp(a_j - m), scaled by the
// same factor in every join, so t / s is the softmax-weighted mean of y.  m and s do not depend on t.
struct LseY {
    double m, s, t;
    static __device__ __forceinline__ LseY none() { return LseY{-1.0e300, 0.0, 0.0}; }
    static __device__ __forceinline__ LseY mix(double hi, const LseY keep, const LseY fade, double e)
    {
        return LseY{hi, keep.s + fade.s * e, keep.t + fade.t * e};
    }
    static __device__ __forceinline__ LseY shfl(const LseY v, int src)
    {
        return LseY{__shfl(v.m, src, MFCD_WAVE), __shfl(v.s, src, MFCD_WAVE), __shfl(v.t, src, MFCD_WAVE)};
    }
};

// The join: one exp; symmetric in its arguments bit for bit.
template <class E>
__device__ __forceinline__ E lse_join(const E x, const E y)
{
    const bool xb = x.m >= y.m;
    const double hi = xb ? x.m : y.m, lo = xb ? y.m : x.m;
    const double e = exp(lo - hi);
    return xb ? E::mix(hi, x, y, e) : E::mix(hi, y, x, e);
}

template <class E>
__device__ __forceinline__ E lse_shfl(const E v, int src)
{
    return E::shfl(v, src);
}

// Inclusive scan over the wave's lanes: towards higher lanes (a prefix), or with REVERSE towards lower ones (a suffix).
template <bool REVERSE, class E>
__device__ __forceinline__ E lse_wave_scan(E v, int lane)
{
#pragma unroll
    for (int off = 1; off < MFCD_WAVE; off <<= 1) {
        const int src = REVERSE ? lane + off : lane - off;
        const E t = lse_shfl(v, src & (MFCD_WAVE - 1));
        if (REVERSE ? src < MFCD_WAVE : src >= 0) v = lse_join(t, v);
    }
    return v;
}

__device__ __forceinline__ double pl_qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// One wave per row: whether the row's header holds, before anything reads the row; the same answer in every lane.
__device__ __forceinline__ bool pl_row_valid(const int64_t *row_off, const int64_t *tile_off, const int32_t *depth,
                                             int rows, int64_t entries, int64_t n_tiles, int r, int lane)
{
    const int64_t b = row_off[r], e = row_off[r + 1], s0 = tile_off[r], s1 = tile_off[r + 1];
    bool ok = b >= 0 && e >= b && e <= entries && e - b <= kPairMaxCols && s0 >= 0 && s1 >= s0 && s1 <= n_tiles;
    if (ok) ok = s1 - s0 == (e - b + kPlTile - 1) / kPlTile;
    if (ok && depth) ok = depth[r] >= 0 && depth[r] <= e - b;
    if (ok)                                            // at most 4096 tiles
        for (int64_t t = s0 + lane; t < s1; t += MFCD_WAVE) ok &= trip_find_row(tile_off, rows, t) == r;
    return __ballot(!ok) == 0;
}

// The tile's row and place in it, or false: nothing of a row that failed validation is touched.  Args: the kernel's
// argument block, with tile_off, rows, status, row_off and depth.
struct PlTile {
    int r, I, T, len, stages;
    int64_t b;
};

template <class Args>
__device__ __forceinline__ bool pl_tile(const Args &g, int64_t t, PlTile *out)
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
    const int depth = g.depth ? g.depth[r] : out->len;
    out->stages = depth < out->len - 1 ? depth : out->len - 1;
    return true;
}

// The join of the workgroup's 256 elements, in thread 0 (the other threads' return value is not used): the waves by an
// xor butterfly, then the four wave values in order.
template <class E>
__device__ __forceinline__ E pl_block_join(E v, int tid, E (&sh)[kPlWaves])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = lse_join(v, lse_shfl(v, (tid & 63) ^ off));
    __syncthreads();                                   // the previous use's readers are done
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    E out = sh[0];
    for (int w = 1; w < kPlWaves; ++w) out = lse_join(out, sh[w]);
    return out;
}

// Inclusive scan over the workgroup's 256 elements in thread order (REVERSE: a suffix), joined with `carry`, what lies
// beyond the tile on the side the scan comes from.
template <bool REVERSE, class E>
__device__ __forceinline__ E pl_block_scan(E v, const E carry, int tid, E (&sh)[kPlWaves])
{
    const int lane = tid & 63, wave = tid >> 6;
    v = lse_wave_scan<REVERSE>(v, lane);
    __syncthreads();                                   // the previous use's readers are done
    if (lane == (REVERSE ? 0 : MFCD_WAVE - 1)) sh[wave] = v;
    __syncthreads();
    E rest = carry;                                    // the waves beyond this one, the farthest first
    if (REVERSE) {
        for (int w = kPlWaves - 1; w > wave; --w) rest = lse_join(rest, sh[w]);
    } else {
        for (int w = 0; w < wave; ++w) rest = lse_join(rest, sh[w]);
    }
    return lse_join(v, rest);
}

}  // namespace
