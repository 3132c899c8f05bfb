// triplet_hess.hip — gradient and Hessian-vector product of the sampled BTL objective with respect to both tables
// (include/mfcd.h: mfcd_triplet_rows).  A row's records are cut into row-relative segments of kTripSeg
// records.  The main kernel gives one wave to a segment: a group of L lanes holds one record's vectors, 64 / L records
// are in flight, and the wave's sums go to the workspace in f64.  The finish kernel gives one wave to a row: every
// output element has one owner, which adds the row's segments in ascending order and then the l2 term.  No LDS, no
// barriers, no atomics; every sum has a fixed order.
#include <cmath>

#include "common.h"
#include "foldin_common.h"

namespace {

constexpr int kTripMaxD = 256;
constexpr int kTripSeg = 256;       // records per segment
constexpr int kTripWaves = 4;       // independent waves per workgroup
constexpr int kTagNoRow = -2;       // no row owns the segment (inconsistent offsets)
constexpr int kTagBadRecords = -1;  // a record of the segment fails validation

struct TripArgs {
    const double *U, *V, *P, *Q;
    int n, m, d;
    const mfcd_sample *rec;
    const int64_t *row_off, *seg_off;
    const int32_t *row_id;
    int rows;
    int64_t n_seg;
    double l2;
    int gauss_newton;
    double *out, *diag, *loss;
    int32_t *status;
    double *part_out, *part_diag, *part_loss;   // [n_seg][d], [n_seg][d], [n_seg]
    int32_t *seg_tag;                           // [n_seg]: the owning row, or a kTag value
};

struct TripRow {
    int own;
    int64_t b, e, s0, s1;
    bool ok;
};

// What row r owns, and whether its offsets are consistent; the main and the finish kernel decide it by this one rule.
__device__ __forceinline__ TripRow trip_row(const TripArgs &a, int side, int r)
{
    TripRow w;
    w.own = a.row_id ? a.row_id[r] : r;
    w.b = a.row_off[r];
    w.e = a.row_off[r + 1];
    w.s0 = a.seg_off[r];
    w.s1 = a.seg_off[r + 1];
    w.ok = (unsigned)w.own < (unsigned)(side ? a.m : a.n) && w.b >= 0 && w.e >= w.b && w.s0 >= 0 && w.s1 <= a.n_seg;
    if (w.ok) {
        const int64_t len = w.e - w.b;
        w.ok = w.s1 - w.s0 == len / kTripSeg + (len % kTripSeg != 0);
    }
    return w;
}

// Sum over the L lanes of a group (L a power of two), xor offsets L/2 -> 1; every lane of the group gets the value.
template <int L>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, MFCD_WAVE);
    return v;
}

// Sum over the 64 / L groups of the wave, xor offsets L -> 32: the same lane of every group.
template <int L>
__device__ __forceinline__ double across_groups(double v)
{
#pragma unroll
    for (int off = L; off < MFCD_WAVE; off <<= 1) v += __shfl_xor(v, off, MFCD_WAVE);
    return v;
}

// The two gather policies.  Both give, per record: a (the vector the dot products are taken with), delta = V[i] - V[j],
// in pass 1 ad (the direction's row beside a) and dq = Q[i] - Q[j], and the sign sigma the contribution carries.
// side 0 (users): a = U[own] held in registers, delta gathered.  side 1 (items): a = U[u] gathered, delta =
// sigma (V[own] - V[other]) with V[own] held in registers.
template <int SIDE>
struct TripGather;

template <>
struct TripGather<0> {
    static __device__ __forceinline__ bool record_is_bad(const TripArgs &a, const mfcd_sample q, int own)
    {
        return q.u != own || (unsigned)q.i >= (unsigned)a.m || (unsigned)q.j >= (unsigned)a.m ||
               !(q.z >= 0.0f && q.z <= 1.0f);
    }
    static __device__ __forceinline__ const double *own_table(const TripArgs &a) { return a.U; }
    static __device__ __forceinline__ const double *own_direction(const TripArgs &a) { return a.P; }
};

template <>
struct TripGather<1> {
    static __device__ __forceinline__ bool record_is_bad(const TripArgs &a, const mfcd_sample q, int own)
    {
        return (unsigned)q.u >= (unsigned)a.n || (unsigned)q.i >= (unsigned)a.m || (unsigned)q.j >= (unsigned)a.m ||
               (q.i != own && q.j != own) || !(q.z >= 0.0f && q.z <= 1.0f);
    }
    static __device__ __forceinline__ const double *own_table(const TripArgs &a) { return a.V; }
    static __device__ __forceinline__ const double *own_direction(const TripArgs &a) { return a.Q; }
};

// One wave per segment.  L lanes per record, E elements per lane (column g + e L of lane g of the group).
template <int SIDE, int PASS, int L, int E>
__global__ __launch_bounds__(kTripWaves * MFCD_WAVE) void triplet_rows_segments(const TripArgs a)
{
    using G = TripGather<SIDE>;
    constexpr int NG = MFCD_WAVE / L;
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t s = (int64_t)blockIdx.x * kTripWaves + (threadIdx.x >> 6);
    if (s >= a.n_seg) return;
    const int d = a.d;

    const int r = trip_find_row(a.seg_off, a.rows, s);
    const TripRow w = trip_row(a, SIDE, r);
    if (!w.ok || s < w.s0 || s >= w.s1) {
        if (lane == 0) a.seg_tag[s] = kTagNoRow;
        return;
    }
    const int64_t t0 = w.b + (s - w.s0) * kTripSeg;
    const int len = (int)(w.e - t0 < kTripSeg ? w.e - t0 : kTripSeg);      // 1 .. kTripSeg

    // validation of the whole segment before any gather
    bool bad = false;
    for (int t = lane; t < len; t += MFCD_WAVE) bad |= G::record_is_bad(a, a.rec[t0 + t], w.own);
    if (__ballot(bad) != 0) {
        if (lane == 0) a.seg_tag[s] = kTagBadRecords;
        return;
    }

    const int grp = lane / L, g = lane % L;
    double own[E], dir[E];
    bool col[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int c = g + e * L;
        col[e] = c < d;
        own[e] = col[e] ? G::own_table(a)[(int64_t)w.own * d + c] : 0.0;
        dir[e] = PASS && col[e] ? G::own_direction(a)[(int64_t)w.own * d + c] : 0.0;
    }

    double acc[E], dg[E], loss = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = dg[e] = 0.0;

    for (int base = 0; base < len; base += NG) {         // wave-uniform trip count: the shuffles see every lane
        const int t = base + grp;
        const bool live = t < len;
        mfcd_sample q{0, 0, 0, 0.0f};
        if (live) q = a.rec[t0 + t];
        double av[E], delta[E], ad[E], dq[E];
        double sigma = 1.0;
        if constexpr (SIDE == 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c = g + e * L;
                const bool on = live && col[e];
                av[e] = own[e];
                ad[e] = dir[e];
                delta[e] = on ? a.V[(int64_t)q.i * d + c] - a.V[(int64_t)q.j * d + c] : 0.0;
                dq[e] = PASS && on ? a.Q[(int64_t)q.i * d + c] - a.Q[(int64_t)q.j * d + c] : 0.0;
            }
        } else {
            sigma = (double)((q.i == w.own) - (q.j == w.own));          // 0 for i = j: the record adds nothing here
            const int other = q.i == w.own ? q.j : q.i;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int c = g + e * L;
                const bool on = live && col[e];
                av[e] = on ? a.U[(int64_t)q.u * d + c] : 0.0;
                ad[e] = PASS && on ? a.P[(int64_t)q.u * d + c] : 0.0;
                delta[e] = on ? sigma * (own[e] - a.V[(int64_t)other * d + c]) : 0.0;
                dq[e] = PASS && on ? sigma * (dir[e] - a.Q[(int64_t)other * d + c]) : 0.0;
            }
        }
        double xs = 0.0, ys = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            xs = fma(av[e], delta[e], xs);
            if constexpr (PASS) ys = fma(ad[e], delta[e], fma(av[e], dq[e], ys));
        }
        const FoldLogit f(group_sum<L>(xs));
        const double z = (double)q.z, res = f.p() - z, wt = f.weight();
        if constexpr (PASS) {
            const double wy = wt * group_sum<L>(ys), rr = a.gauss_newton ? 0.0 : res;
            if (live && sigma != 0.0) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if constexpr (SIDE == 0) acc[e] += fma(wy, delta[e], rr * dq[e]);
                    else acc[e] += sigma * fma(wy, av[e], rr * ad[e]);
                }
            }
        } else {
            if (live && sigma != 0.0) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if constexpr (SIDE == 0) {
                        acc[e] = fma(res, delta[e], acc[e]);
                        dg[e] = fma(wt * delta[e], delta[e], dg[e]);
                    } else {
                        acc[e] = fma(sigma * res, av[e], acc[e]);
                        dg[e] = fma(wt * av[e], av[e], dg[e]);
                    }
                }
                loss += f.term(z);
            }
        }
    }

    // the groups' sums in a fixed order, then group 0 stores the segment's partial sums
#pragma unroll
    for (int e = 0; e < E; ++e) {
        acc[e] = across_groups<L>(acc[e]);
        if constexpr (!PASS) dg[e] = across_groups<L>(dg[e]);
    }
    if constexpr (!PASS && SIDE == 0) loss = across_groups<L>(loss);
    if (grp == 0) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int c = g + e * L;
            if (!col[e]) continue;
            a.part_out[s * d + c] = acc[e];
            if constexpr (!PASS) a.part_diag[s * d + c] = dg[e];
        }
        if constexpr (!PASS && SIDE == 0)
            if (g == 0) a.part_loss[s] = loss;
    }
    if (lane == 0) a.seg_tag[s] = r;
}

// One wave per row: the row's segments added in ascending order, then the l2 term; or the NaN row.
template <int SIDE, int PASS>
__global__ __launch_bounds__(kTripWaves * MFCD_WAVE) void triplet_rows_finish(const TripArgs a)
{
    using G = TripGather<SIDE>;
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * kTripWaves + (threadIdx.x >> 6);
    if (rr >= a.rows) return;
    const int r = (int)rr, d = a.d;
    const TripRow w = trip_row(a, SIDE, r);
    bool bad = !w.ok;
    if (!bad)
        for (int64_t s = w.s0 + lane; s < w.s1; s += MFCD_WAVE) bad |= a.seg_tag[s] != r;
    bad = __ballot(bad) != 0;
    const bool want_diag = !PASS && a.diag, want_loss = !PASS && SIDE == 0 && a.loss;
    if (bad) {
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        for (int c = lane; c < d; c += MFCD_WAVE) {
            a.out[(int64_t)r * d + c] = qnan;
            if (want_diag) a.diag[(int64_t)r * d + c] = qnan;
        }
        if (lane == 0) {
            if (want_loss) a.loss[r] = qnan;
            a.status[r] = 2;
        }
        return;
    }
    const double *base = PASS ? G::own_direction(a) : G::own_table(a);
    for (int c = lane; c < d; c += MFCD_WAVE) {
        const double reg = a.l2 * base[(int64_t)w.own * d + c];
        double so = 0.0, sd = 0.0;
        for (int64_t s = w.s0; s < w.s1; ++s) {
            so += a.part_out[s * d + c];
            if (want_diag) sd += a.part_diag[s * d + c];
        }
        a.out[(int64_t)r * d + c] = w.s1 > w.s0 ? so + reg : reg;
        if (want_diag) a.diag[(int64_t)r * d + c] = sd + a.l2;
    }
    if (lane == 0) {
        if (want_loss) {
            double sl = 0.0;
            for (int64_t s = w.s0; s < w.s1; ++s) sl += a.part_loss[s];
            a.loss[r] = sl;
        }
        a.status[r] = 0;
    }
}

template <int SIDE, int PASS, int L, int E>
int trip_launch_le(const TripArgs &a, hipStream_t stream)
{
    if (a.n_seg > 0) {
        const unsigned blocks = (unsigned)((a.n_seg + kTripWaves - 1) / kTripWaves);
        hipLaunchKernelGGL((triplet_rows_segments<SIDE, PASS, L, E>), dim3(blocks), dim3(kTripWaves * MFCD_WAVE), 0, stream, a);
        MFCD_HIP_TRY(hipGetLastError());
    }
    const unsigned blocks = (unsigned)(((int64_t)a.rows + kTripWaves - 1) / kTripWaves);
    hipLaunchKernelGGL((triplet_rows_finish<SIDE, PASS>), dim3(blocks), dim3(kTripWaves * MFCD_WAVE), 0, stream, a);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

// L = min(64, next power of two >= d); E = ceil(d / 64)
template <int SIDE, int PASS>
int trip_launch(const TripArgs &a, hipStream_t stream)
{
    const int d = a.d;
    if (d > 192) return trip_launch_le<SIDE, PASS, 64, 4>(a, stream);
    if (d > 128) return trip_launch_le<SIDE, PASS, 64, 3>(a, stream);
    if (d > 64) return trip_launch_le<SIDE, PASS, 64, 2>(a, stream);
    if (d > 32) return trip_launch_le<SIDE, PASS, 64, 1>(a, stream);
    if (d > 16) return trip_launch_le<SIDE, PASS, 32, 1>(a, stream);
    if (d > 8) return trip_launch_le<SIDE, PASS, 16, 1>(a, stream);
    if (d > 4) return trip_launch_le<SIDE, PASS, 8, 1>(a, stream);
    if (d > 2) return trip_launch_le<SIDE, PASS, 4, 1>(a, stream);
    if (d > 1) return trip_launch_le<SIDE, PASS, 2, 1>(a, stream);
    return trip_launch_le<SIDE, PASS, 1, 1>(a, stream);
}

inline bool trip_sizes_ok(int rows, int d, int64_t n_seg)
{
    return rows >= 0 && d >= 1 && d <= kTripMaxD && n_seg >= 0 && n_seg <= (int64_t)1 << 31;
}

}  // namespace

extern "C" int mfcd_triplet_rows_segment(void) { return kTripSeg; }

extern "C" size_t mfcd_triplet_rows_workspace_bytes(int rows, int d, int64_t n_seg)
{
    if (!trip_sizes_ok(rows, d, n_seg)) return 0;
    const size_t vec = align_up(sizeof(double) * (size_t)n_seg * d);
    return 256 + 2 * vec + align_up(sizeof(double) * (size_t)n_seg) + align_up(sizeof(int32_t) * (size_t)n_seg);
}

extern "C" int mfcd_triplet_rows(int side, int pass, int gauss_newton, const double *U, int n, const double *V, int m, int d,
                                 const double *P, const double *Q, const mfcd_sample *records, const int64_t *row_off,
                                 const int32_t *row_id, int rows, const int64_t *seg_off, int64_t n_seg, double l2,
                                 double *out, double *diag, double *loss, int32_t *status, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if ((side != 0 && side != 1) || (pass != 0 && pass != 1) || (gauss_newton != 0 && gauss_newton != 1)) return MFCD_EINVAL;
    if (!U || !V || !row_off || !seg_off || !out || !status || n < 1 || m < 1 || !trip_sizes_ok(rows, d, n_seg)) return MFCD_EINVAL;
    if (pass == 1 && (!P || !Q)) return MFCD_EINVAL;
    if (n_seg > 0 && !records) return MFCD_EINVAL;
    if (!row_id && rows > (side ? m : n)) return MFCD_EINVAL;
    if (!(l2 > 0.0) || !std::isfinite(l2)) return MFCD_EINVAL;
    const size_t row_bytes = (size_t)rows * d * sizeof(double);
    const size_t ub = (size_t)n * d * sizeof(double), vb = (size_t)m * d * sizeof(double);
    const struct { const void *p; size_t bytes; } written[] = {{out, row_bytes}, {pass == 0 ? diag : nullptr, row_bytes},
                                                              {pass == 0 && side == 0 ? loss : nullptr, (size_t)rows * sizeof(double)}};
    for (const auto &o : written) {
        if (!o.p) continue;
        if (o.p == U || o.p == V || fold_overlap(o.p, o.bytes, U, ub) || fold_overlap(o.p, o.bytes, V, vb)) return MFCD_EINVAL;
        if (pass == 1 && (o.p == P || o.p == Q || fold_overlap(o.p, o.bytes, P, ub) || fold_overlap(o.p, o.bytes, Q, vb)))
            return MFCD_EINVAL;
    }
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_triplet_rows_workspace_bytes(rows, d, n_seg)) return MFCD_EWORKSPACE;

    const size_t vec = align_up(sizeof(double) * (size_t)n_seg * d);
    char *ws = (char *)workspace + 256;
    TripArgs a;
    a.U = U; a.V = V; a.P = pass ? P : nullptr; a.Q = pass ? Q : nullptr;
    a.n = n; a.m = m; a.d = d;
    a.rec = records; a.row_off = row_off; a.seg_off = seg_off; a.row_id = row_id;
    a.rows = rows; a.n_seg = n_seg; a.l2 = l2; a.gauss_newton = gauss_newton;
    a.out = out; a.diag = pass == 0 ? diag : nullptr; a.loss = pass == 0 && side == 0 ? loss : nullptr; a.status = status;
    a.part_out = (double *)ws;
    a.part_diag = (double *)(ws + vec);
    a.part_loss = (double *)(ws + 2 * vec);
    a.seg_tag = (int32_t *)(ws + 2 * vec + align_up(sizeof(double) * (size_t)n_seg));
    const hipStream_t st = (hipStream_t)stream;
    if (side == 0) return pass ? trip_launch<0, 1>(a, st) : trip_launch<0, 0>(a, st);
    return pass ? trip_launch<1, 1>(a, st) : trip_launch<1, 0>(a, st);
}
