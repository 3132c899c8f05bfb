// ragged.hip — the two table kernels around the ragged pair kernels (include/mfcd.h: mfcd_ragged_dot,
// mfcd_ragged_gather_sum): the scores of a ratings table's entries from the factor tables, and the carry of
// a per-entry coefficient back to a factor table.  Rows are CSR slices, entries [row_off[r], row_off[r+1]).
//
// dot         a_e = R[r] . C[idx_e]: one 256-thread workgroup per row, R[r] in LDS, one entry per thread at a time; fp32
//             products rounded apart and added in ascending column order.
// gather-sum  out[r] = sum over the row's entries of coef * T[idx_e]: triplet_hess.hip's scheme.  A row is cut into
//             segments of kRagSeg entries; one wave per segment writes the segment's sums to the workspace in f64
//             (products of two fp32 values are exact there); one owner per output element adds a row's segments in
//             ascending order and rounds to fp32 once.  An item with a hundred thousand ratings is spread over hundreds
//             of waves.  No LDS, no atomics; every sum has a fixed order that depends on the row alone.
// Every index is validated before any gather: an invalid row gets status 2 and a NaN slice / row, and no address is
// formed from a value that failed.
#include <cmath>

#include "common.h"

namespace {

constexpr int kRagMaxD = 256;
constexpr int kRagSeg = 256;        // entries per segment (mfcd_ragged_segment)
constexpr int kRagWaves = 4;        // independent waves per workgroup
constexpr int kDotThreads = 256;

template <bool VEC4>
__global__ __launch_bounds__(kDotThreads) void ragged_dot_kernel(const float *__restrict__ R, const float *__restrict__ C,
                                                                 int n_c, int d, int64_t entries,
                                                                 const int64_t *__restrict__ row_off,
                                                                 const int32_t *__restrict__ idx, float *__restrict__ a,
                                                                 int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float own[kRagMaxD];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t b = row_off[r], e = row_off[r + 1];
    if (!(b >= 0 && e >= b && e <= entries)) {         // uniform: there is no slice to mark
        if (tid == 0) status[r] = 2;
        return;
    }
    int bad = 0;                                       // the whole row, before any gather
    for (int64_t p = b + tid; p < e; p += kDotThreads) bad |= (int)((unsigned)idx[p] >= (unsigned)n_c);
    bad = __syncthreads_or(bad);
    if (bad) {
        for (int64_t p = b + tid; p < e; p += kDotThreads) a[p] = __uint_as_float(0x7fc00000u);
        if (tid == 0) status[r] = 2;
        return;
    }
    for (int c = tid; c < d; c += kDotThreads) own[c] = R[r * d + c];
    __syncthreads();
    for (int64_t p = b + tid; p < e; p += kDotThreads) {
        const float *row = C + (int64_t)idx[p] * d;
        float acc = 0.0f;
        if (VEC4) {
            for (int c = 0; c < d; c += 4) {
                const float4 u = *(const float4 *)(own + c), v = *(const float4 *)(row + c);
                acc += u.x * v.x;                      // products rounded apart (contraction is off), ascending columns
                acc += u.y * v.y;
                acc += u.z * v.z;
                acc += u.w * v.w;
            }
        } else {
            for (int c = 0; c < d; ++c) acc += own[c] * row[c];
        }
        a[p] = acc;
    }
    if (tid == 0) status[r] = 0;
}

struct GatherArgs {
    const float *T;
    int t_rows, d;
    int64_t entries;
    const int64_t *row_off, *seg_off;
    int rows;
    int64_t n_seg;
    const int32_t *idx;
    const float *coef;
    const int64_t *perm;
    float *out;
    int32_t *status;
    double *part;        // [n_seg][d]
    int32_t *seg_tag;    // [n_seg]: the owning row, or -1
};

struct GatherRow {
    int64_t b, e, s0, s1;
    bool ok;
};

// What row r owns, and whether its offsets are consistent; both kernels decide it by this one rule.
__device__ __forceinline__ GatherRow gather_row(const GatherArgs &g, int r)
{
    GatherRow w;
    w.b = g.row_off[r];
    w.e = g.row_off[r + 1];
    w.s0 = g.seg_off[r];
    w.s1 = g.seg_off[r + 1];
    w.ok = w.b >= 0 && w.e >= w.b && w.e <= g.entries && w.s0 >= 0 && w.s1 >= w.s0 && w.s1 <= g.n_seg;
    if (w.ok) w.ok = w.s1 - w.s0 == (w.e - w.b + kRagSeg - 1) / kRagSeg;
    return w;
}

// One wave per segment.  A group of LW lanes holds one entry's table row, E columns per lane (column l + k LW of lane l
// of the group); 64 / LW entries are in flight, group q takes entries q, q + 64 / LW, ... of the segment in order.
template <int LW, int E>
__global__ __launch_bounds__(kRagWaves * MFCD_WAVE) void ragged_gather_segments(const GatherArgs g)
{
    constexpr int NG = MFCD_WAVE / LW;
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t s = (int64_t)blockIdx.x * kRagWaves + (threadIdx.x >> 6);
    if (s >= g.n_seg) return;
    const int d = g.d;
    const int r = trip_find_row(g.seg_off, g.rows, s);
    const GatherRow w = gather_row(g, r);
    if (!w.ok || s < w.s0 || s >= w.s1) {
        if (lane == 0) g.seg_tag[s] = -1;
        return;
    }
    const int64_t p0 = w.b + (s - w.s0) * kRagSeg;
    const int len = (int)(w.e - p0 < kRagSeg ? w.e - p0 : kRagSeg);        // 1 .. kRagSeg

    bool bad = false;                                  // the whole segment, before any gather
    for (int t = lane; t < len; t += MFCD_WAVE) {
        bad |= (unsigned)g.idx[p0 + t] >= (unsigned)g.t_rows;
        if (g.perm) bad |= (uint64_t)g.perm[p0 + t] >= (uint64_t)g.entries;
    }
    if (__ballot(bad) != 0) {
        if (lane == 0) g.seg_tag[s] = -1;
        return;
    }

    const int grp = lane / LW, l = lane % LW;
    double acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = 0.0;
    for (int t = grp; t < len; t += NG) {
        const int64_t p = p0 + t;
        const double c = (double)g.coef[g.perm ? g.perm[p] : p];
        const float *row = g.T + (int64_t)g.idx[p] * d;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int col = l + k * LW;
            if (col < d) acc[k] += c * (double)row[col];                   // the product is exact in f64
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) {                      // the groups' sums in a fixed order: the same lane of every group
#pragma unroll
        for (int off = LW; off < MFCD_WAVE; off <<= 1) acc[k] += __shfl_xor(acc[k], off, MFCD_WAVE);
    }
    if (grp == 0) {
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int col = l + k * LW;
            if (col < d) g.part[s * d + col] = acc[k];
        }
    }
    if (lane == 0) g.seg_tag[s] = r;
}

// One wave per row: every output element has one owner, which adds the row's segments in ascending order; or the NaN row.
__global__ __launch_bounds__(kRagWaves * MFCD_WAVE) void ragged_gather_finish(const GatherArgs g)
{
    const int lane = threadIdx.x & (MFCD_WAVE - 1);
    const int64_t rr = (int64_t)blockIdx.x * kRagWaves + (threadIdx.x >> 6);
    if (rr >= g.rows) return;
    const int r = (int)rr, d = g.d;
    const GatherRow w = gather_row(g, r);
    bool bad = !w.ok;
    if (!bad)
        for (int64_t s = w.s0 + lane; s < w.s1; s += MFCD_WAVE) bad |= g.seg_tag[s] != r;
    bad = __ballot(bad) != 0;
    for (int c = lane; c < d; c += MFCD_WAVE) {
        double sum = 0.0;
        if (!bad)
            for (int64_t s = w.s0; s < w.s1; ++s) sum += g.part[s * d + c];
        g.out[(int64_t)r * d + c] = bad ? __uint_as_float(0x7fc00000u) : (float)sum;   // rounded to fp32 once
    }
    if (lane == 0) g.status[r] = bad ? 2 : 0;
}

template <int LW, int E>
void gather_launch_le(const GatherArgs &g, hipStream_t st)
{
    const unsigned blocks = (unsigned)((g.n_seg + kRagWaves - 1) / kRagWaves);
    hipLaunchKernelGGL((ragged_gather_segments<LW, E>), dim3(blocks), dim3(kRagWaves * MFCD_WAVE), 0, st, g);
}

// LW = min(64, next power of two >= d); E = ceil(d / 64)
void gather_launch(const GatherArgs &g, hipStream_t st)
{
    const int d = g.d;
    if (d > 192) gather_launch_le<64, 4>(g, st);
    else if (d > 128) gather_launch_le<64, 3>(g, st);
    else if (d > 64) gather_launch_le<64, 2>(g, st);
    else if (d > 32) gather_launch_le<64, 1>(g, st);
    else if (d > 16) gather_launch_le<32, 1>(g, st);
    else if (d > 8) gather_launch_le<16, 1>(g, st);
    else if (d > 4) gather_launch_le<8, 1>(g, st);
    else if (d > 2) gather_launch_le<4, 1>(g, st);
    else if (d > 1) gather_launch_le<2, 1>(g, st);
    else gather_launch_le<1, 1>(g, st);
}

inline bool gather_sizes_ok(int rows, int d, int64_t n_seg)
{
    return rows >= 0 && d >= 1 && d <= kRagMaxD && n_seg >= 0 && n_seg <= (int64_t)1 << 31;
}

}  // namespace

extern "C" int mfcd_ragged_segment(void) { return kRagSeg; }

extern "C" int mfcd_ragged_dot(const float *R, int n_r, const float *C, int n_c, int d, int64_t entries,
                               const int64_t *row_off, int rows, const int32_t *idx, float *a, int32_t *status,
                               void *stream)
{
    if (!R || !C || !row_off || !status || n_r < 1 || n_c < 1 || d < 1 || d > kRagMaxD || entries < 0) return MFCD_EINVAL;
    if (rows < 0 || rows > n_r) return MFCD_EINVAL;
    if (entries > 0 && (!idx || !a)) return MFCD_EINVAL;
    if (a && (a == R || a == C)) return MFCD_EINVAL;
    if (rows == 0) return 0;
    const bool vec4 = (d & 3) == 0 && ((uintptr_t)C & 15) == 0;
    if (vec4)
        hipLaunchKernelGGL(ragged_dot_kernel<true>, dim3((unsigned)rows), dim3(kDotThreads), 0, (hipStream_t)stream, R, C, n_c,
                           d, entries, row_off, idx, a, status);
    else
        hipLaunchKernelGGL(ragged_dot_kernel<false>, dim3((unsigned)rows), dim3(kDotThreads), 0, (hipStream_t)stream, R, C, n_c,
                           d, entries, row_off, idx, a, status);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" size_t mfcd_ragged_gather_sum_workspace_bytes(int rows, int d, int64_t n_seg)
{
    if (!gather_sizes_ok(rows, d, n_seg)) return 0;
    return 256 + align_up(sizeof(double) * (size_t)n_seg * d) + align_up(sizeof(int32_t) * (size_t)n_seg);
}

extern "C" int mfcd_ragged_gather_sum(const float *T, int t_rows, int d, int64_t entries, const int64_t *row_off, int rows,
                                      const int32_t *idx, const float *coef, const int64_t *perm, const int64_t *seg_off,
                                      int64_t n_seg, float *out, int32_t *status, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    if (!T || !row_off || !seg_off || !out || !status || t_rows < 1 || entries < 0 || !gather_sizes_ok(rows, d, n_seg))
        return MFCD_EINVAL;
    if (n_seg > 0 && (!idx || !coef)) return MFCD_EINVAL;
    if (out == T || out == coef) return MFCD_EINVAL;
    if (rows == 0) return 0;
    if (!workspace) return MFCD_EINVAL;
    if (workspace_bytes < mfcd_ragged_gather_sum_workspace_bytes(rows, d, n_seg)) return MFCD_EWORKSPACE;
    char *ws = (char *)workspace + 256;
    GatherArgs g;
    g.T = T; g.t_rows = t_rows; g.d = d; g.entries = entries;
    g.row_off = row_off; g.seg_off = seg_off; g.rows = rows; g.n_seg = n_seg;
    g.idx = idx; g.coef = coef; g.perm = perm; g.out = out; g.status = status;
    g.part = (double *)ws;
    g.seg_tag = (int32_t *)(ws + align_up(sizeof(double) * (size_t)n_seg * d));
    const hipStream_t st = (hipStream_t)stream;
    if (n_seg > 0) {
        gather_launch(g, st);
        MFCD_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(ragged_gather_finish, dim3((unsigned)(((int64_t)rows + kRagWaves - 1) / kRagWaves)),
                       dim3(kRagWaves * MFCD_WAVE), 0, st, g);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}
