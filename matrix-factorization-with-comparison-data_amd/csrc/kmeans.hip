// kmeans.hip — the two steps of Lloyd's k-means over row-major fp32 points [P][dim] on gfx950 (the `cluster` sampling
// strategy, generation_data.py:229-247: sklearn KMeans over the item columns, then two items from different clusters).
// The iteration itself, k-means++ and the empty-cluster rule live on the host side (mfcd/cluster.py).
//
//   assign   label[p] = argmax_c (p . c - |c|^2 / 2) = argmin_c |p - c|^2, lowest index among equals.  P x k x dim
//            multiply-adds: 128 points x 64 centres per workgroup on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32, a
//            k-ordered fmaf chain — the tile of topk.hip's score kernel with one operand at most 64 rows tall), a wave
//            per 32 points, operands staged through LDS 32 coordinates at a time, any dim.  The argmax is taken in the
//            epilogue across the lanes that hold one point's scores: nothing of size P x k exists.  |c|^2 / 2 comes
//            from a prologue kernel (f64 sum, rounded once).  dist2 is formed directly, sum (p_q - c_q)^2 in fp32
//            against the chosen centre: no cancellation, exactly 0 for a point that IS its centre.  Few points of
//            many coordinates (the item columns of a dense X) would fill a fraction of the chip that way: below
//            kDeepBelowBlocks such workgroups, from kDeepMinDim coordinates on, a workgroup takes 32 points and its
//            waves split the coordinates (kmeans_assign_deep_kernel).
//   update   centre[c] = mean of its members in f64, fixed order: a STORE pass — one wave per (chunk of points, 64
//            coordinates) adds its points one after the other into per-cluster f64 columns in LDS (a lane owns a
//            column: no atomics) and stores them as a slab — and a SUM pass over the chunks in ascending order, one
//            division, one rounding to fp32.  No floating-point atomics: two calls are bit-equal.
// Safety: every loop bound is a launch argument; a label is compared against k before it addresses anything; LDS
// tiles are sized by kMaxK and the tile constants alone.
#include "common.h"

namespace {

constexpr int kMaxK = 64;                            // centres of one call: two 32-column MFMA tiles
constexpr int kMaxP = 1 << 22;
constexpr int kPts = 128, kKC = 32, kLD = kKC + 1;   // assign: points per workgroup, coordinates per LDS stage, padded row
constexpr int kDeepMinDim = 256, kDeepBelowBlocks = 256;   // assign, few points of many coordinates: the deep kernel
constexpr int kCols = 64;                            // update: coordinates per wave (one LDS column per lane)
constexpr int kChunkPts = 128, kMaxChunks = 512;     // update: points per chunk at least / chunks at most
constexpr size_t kSlabBytes = (size_t)64 << 20;      // update: the f64 slab (but at least one chunk)

// hn[c] = |centre c|^2 / 2: one wave per centre, f64 partial sums per lane in coordinate order, then a butterfly
__global__ __launch_bounds__(MFCD_WAVE) void kmeans_half_norms_kernel(const float *__restrict__ C, int dim,
                                                                      float *__restrict__ hn)
{
    const int lane = threadIdx.x;
    const float *row = C + (int64_t)blockIdx.x * dim;
    double s = 0.0;
    for (int q = lane; q < dim; q += MFCD_WAVE) {
        const double v = (double)row[q];
        s += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, MFCD_WAVE);   // inline: wave_sum_xor changes this kernel's ISA
    if (lane == 0) hn[blockIdx.x] = (float)(0.5 * s);
}

// argmax over the centres of one wave's 32 points: a lane holds the products with centre l31 (acc0) and 32 + l31 (acc1)
// of 16 points; the 32 lanes of a half hold one point's scores.  Score = product - |c|^2 / 2; (value, index) butterfly
// inside the half, larger value first, then the lower index.  lab32[row] = the label of the wave's point `row`.
__device__ __forceinline__ void pick_labels(const f32x16 &acc0, const f32x16 &acc1, int k, const float *__restrict__ hn,
                                            int lane, int *lab32)
{
    const int half = lane >> 5, l31 = lane & 31;
    const bool two = k > 32;
    const float ninf = -__builtin_inff();
    const bool ok0 = l31 < k, ok1 = 32 + l31 < k;
    const float h0 = ok0 ? hn[l31] : 0.0f, h1 = ok1 ? hn[32 + l31] : 0.0f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        float v = ok0 ? acc0[reg] - h0 : ninf;
        int idx = l31;
        if (two) {
            const float v1 = ok1 ? acc1[reg] - h1 : ninf;
            if (v1 > v) {
                v = v1;
                idx = 32 + l31;
            }
        }
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const float ov = __shfl_xor(v, off, MFCD_WAVE);
            const int oi = __shfl_xor(idx, off, MFCD_WAVE);
            if (ov > v || (ov == v && oi < idx)) {
                v = ov;
                idx = oi;
            }
        }
        if (l31 == 0) lab32[tile_row(reg, half)] = min(idx, k - 1);   // (centre 0 always competes: idx < k already)
    }
}

// The workgroup's `npts` labels lab_s[] (all in [0, k)) go out: labels, the count of changed ones, and dist2 — a wave
// per point, lanes over the coordinates.  Called by every thread, after a barrier behind lab_s and *changed_s = 0.
__device__ __forceinline__ void write_points(const float *__restrict__ pts, int P, int dim, const float *__restrict__ C,
                                             int p0, int npts, const int *lab_s, int32_t *__restrict__ labels,
                                             float *__restrict__ dist2, int32_t *__restrict__ changed, int *changed_s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    if (tid < npts) {
        const int p = p0 + tid;
        if (p < P) {
            const int l = lab_s[tid];
            if (changed && labels[p] != l) atomicAdd(changed_s, 1);
            labels[p] = l;
        }
    }
    if (dist2) {
        for (int r = wave; r < npts; r += waves) {
            const int p = p0 + r;
            if (p >= P) break;
            const float *x = pts + (int64_t)p * dim, *c = C + (int64_t)lab_s[r] * dim;
            float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};     // four independent chains: eight loads in flight per lane
            int q = lane;
            for (; q + 3 * MFCD_WAVE < dim; q += 4 * MFCD_WAVE) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float t = x[q + j * MFCD_WAVE] - c[q + j * MFCD_WAVE];
                    s4[j] = fmaf(t, t, s4[j]);
                }
            }
            for (; q < dim; q += MFCD_WAVE) {
                const float t = x[q] - c[q];
                s4[0] = fmaf(t, t, s4[0]);
            }
            const float s = wave_sum64((s4[0] + s4[1]) + (s4[2] + s4[3]));
            if (lane == 0) dist2[p] = s;
        }
    }
    __syncthreads();
    if (tid == 0 && changed && *changed_s) atomicAdd(changed, *changed_s);
}

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float *__restrict__ pts, int P, int dim,
                                                            const float *__restrict__ C, int k,
                                                            const float *__restrict__ hn, int32_t *__restrict__ labels,
                                                            float *__restrict__ dist2, int32_t *__restrict__ changed)
{
    __shared__ float Ps[kPts * kLD], Cs[kMaxK * kLD];
    __shared__ int lab_s[kPts];
    __shared__ int changed_s;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
    const int p0 = blockIdx.x * kPts, wr = wave * 32;
    const bool two = k > 32;                      // the second tile of centres exists (uniform)
    // loader: thread -> coordinate lk of the stage, rows lr + 8 i
    const int lk = tid & 31, lr = tid >> 5;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;

    for (int k0 = 0; k0 < dim; k0 += kKC) {
        const int kk = k0 + lk;
        const bool kok = kk < dim;
#pragma unroll
        for (int i = 0; i < kPts / 8; ++i) {
            const int p = p0 + lr + 8 * i;
            Ps[(lr + 8 * i) * kLD + lk] = kok && p < P ? pts[(int64_t)p * dim + kk] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kMaxK / 8; ++i) {
            const int c = lr + 8 * i;
            Cs[c * kLD + lk] = kok && c < k ? C[(int64_t)c * dim + kk] : 0.0f;
        }
        __syncthreads();
        const int steps = (min(kKC, dim - k0) + 1) >> 1;   // MFMA k index: step s, lane half h -> k0 + 2 s + h
        for (int s = 0; s < steps; ++s) {
            const float a = Ps[(wr + l31) * kLD + 2 * s + half];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Cs[l31 * kLD + 2 * s + half], acc0, 0, 0, 0);
            if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Cs[(32 + l31) * kLD + 2 * s + half], acc1, 0, 0, 0);
        }
        __syncthreads();
    }

    if (tid == 0) changed_s = 0;      // (ordered before its use by the barriers of the stage loop / below)
    pick_labels(acc0, acc1, k, hn, lane, lab_s + wr);
    __syncthreads();
    write_points(pts, P, dim, C, p0, kPts, lab_s, labels, dist2, changed, &changed_s);
}

// The same for few points of many coordinates (the item columns of a dense X): 32 points per workgroup, and the
// stages of 32 coordinates dealt round robin to its WAVES waves, each with its own LDS stage and the next stage's loads
// in flight under the MFMAs; the WAVES partial products of a (point, centre) are added in wave order through LDS.
// TWO: the second tile of centres exists (k > 32).  Dynamic LDS: WAVES * deep_stage_floats(TWO) floats.
constexpr int deep_stage_floats(bool two) { return (32 + (two ? 64 : 32)) * kLD; }

template <int WAVES, bool TWO>
__global__ __launch_bounds__(64 * WAVES) void kmeans_assign_deep_kernel(const float *__restrict__ pts, int P, int dim,
                                                                       const float *__restrict__ C, int k,
                                                                       const float *__restrict__ hn,
                                                                       int32_t *__restrict__ labels,
                                                                       float *__restrict__ dist2,
                                                                       int32_t *__restrict__ changed)
{
    extern __shared__ __attribute__((aligned(16))) float stage[];   // per wave: 32 point rows, then the centre rows
    __shared__ int lab_s[32];
    __shared__ int changed_s;
    constexpr int kStage = deep_stage_floats(TWO);
    static_assert(kStage >= (TWO ? 2 : 1) * 16 * 64, "a wave's partial products fit its stage");
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31, wave = tid >> 6;
    const int p0 = blockIdx.x * 32;
    float *Ps = stage + wave * kStage, *Cs = Ps + 32 * kLD;
    // loader of a wave: lane -> coordinate l31 of the stage, rows half + 2 i
    float pa[16], pc[TWO ? 32 : 16];
    auto fetch = [&](int st) __attribute__((always_inline)) {
        const int kk = st * kKC + l31;
        const bool kok = kk < dim;          // (false for every stage past the last: no loads, zeros)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = half + 2 * i, p = p0 + r;
            pa[i] = kok && p < P ? pts[(int64_t)p * dim + kk] : 0.0f;
            pc[i] = kok && r < k ? C[(int64_t)r * dim + kk] : 0.0f;
            if constexpr (TWO) pc[16 + i] = kok && 32 + r < k ? C[(int64_t)(32 + r) * dim + kk] : 0.0f;
        }
    };
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
    const int nst = (dim + kKC - 1) / kKC;
    fetch(wave);
    for (int st0 = 0; st0 < nst; st0 += WAVES) {            // the same trip count for every wave
        const int st = st0 + wave;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = half + 2 * i;
            Ps[r * kLD + l31] = pa[i];
            Cs[r * kLD + l31] = pc[i];
            if constexpr (TWO) Cs[(32 + r) * kLD + l31] = pc[16 + i];
        }
        __syncthreads();
        fetch(st + WAVES);
        const int steps = st < nst ? (min(kKC, dim - st * kKC) + 1) >> 1 : 0;
        for (int s = 0; s < steps; ++s) {
            const float a = Ps[l31 * kLD + 2 * s + half];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Cs[l31 * kLD + 2 * s + half], acc0, 0, 0, 0);
            if constexpr (TWO)
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Cs[(32 + l31) * kLD + 2 * s + half], acc1, 0, 0, 0);
        }
        __syncthreads();
    }
    // partial products of the waves -> the wave's own stage, summed by wave 0 in wave order
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        Ps[reg * 64 + lane] = acc0[reg];
        if constexpr (TWO) Ps[(16 + reg) * 64 + lane] = acc1[reg];
    }
    if (tid == 0) changed_s = 0;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float s0 = stage[reg * 64 + lane], s1 = TWO ? stage[(16 + reg) * 64 + lane] : 0.0f;
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {
                s0 += stage[w * kStage + reg * 64 + lane];
                if constexpr (TWO) s1 += stage[w * kStage + (16 + reg) * 64 + lane];
            }
            acc0[reg] = s0;
            acc1[reg] = s1;
        }
        pick_labels(acc0, acc1, k, hn, lane, lab_s);
    }
    __syncthreads();
    write_points(pts, P, dim, C, p0, 32, lab_s, labels, dist2, changed, &changed_s);
}

// STORE pass of update: chunk g = blockIdx.y of the points, coordinates blockIdx.x * 64 + lane.  slab[g][c][q] = the
// f64 sum of coordinate q over the chunk's members of cluster c, added in ascending point order; cnt_slab[g][c] =
// their number.
__global__ __launch_bounds__(kCols) void kmeans_partial_kernel(const float *__restrict__ pts, int P, int dim,
                                                               const int32_t *__restrict__ labels, int k, int chunk,
                                                               double *__restrict__ slab, int32_t *__restrict__ cnt_slab)
{
    __shared__ double sums[kMaxK * kCols];
    __shared__ int cnt[kMaxK];
    const int lane = threadIdx.x, g = blockIdx.y;
    const int64_t q = (int64_t)blockIdx.x * kCols + lane;
    const bool col = q < dim;
    for (int c = 0; c < k; ++c) sums[c * kCols + lane] = 0.0;
    if (lane < kMaxK) cnt[lane] = 0;
    __syncthreads();
    const int p_lo = g * chunk, p_hi = min(P, p_lo + chunk);
    for (int p = p_lo; p < p_hi; p += 16) {      // sixteen loads in flight, then their additions in point order
        int lab[16];
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int pp = min(p + j, p_hi - 1);
            lab[j] = p + j < p_hi ? labels[pp] : -1;
            v[j] = col ? pts[(int64_t)pp * dim + q] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((unsigned)lab[j] < (unsigned)k) {             // a label outside [0, k) is skipped
                sums[lab[j] * kCols + lane] += (double)v[j];
                if (lane == 0) cnt[lab[j]] += 1;
            }
        }
    }
    __syncthreads();
    if (col)
        for (int c = 0; c < k; ++c) slab[((int64_t)g * k + c) * dim + q] = sums[c * kCols + lane];
    if (blockIdx.x == 0 && lane < k) cnt_slab[g * k + lane] = cnt[lane];
}

// SUM pass: cluster c = blockIdx.y, 64 coordinates per workgroup; wave w adds the chunks g = w, w + 4, ... in ascending
// order (eight loads in flight), and the four partial sums are added as (0 + 1) + (2 + 3): one fixed order
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double *__restrict__ slab,
                                                            const int32_t *__restrict__ cnt_slab, int G, int dim, int k,
                                                            float *__restrict__ C, int32_t *__restrict__ counts)
{
    __shared__ double part_s[4][kCols];
    __shared__ int n_s[4];
    const int c = blockIdx.y, lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * kCols + lane;
    int n = 0;
    for (int g = threadIdx.x; g < G; g += 256) n += cnt_slab[g * k + c];
    n = wave_sum64_i(n);
    if (lane == 0) n_s[part] = n;
    double s = 0.0;
    if (q < dim) {
        for (int g0 = part; g0 < G; g0 += 32) {
            double v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int g = g0 + 4 * j;
                v[j] = g < G ? slab[((int64_t)g * k + c) * dim + q] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[j];
        }
    }
    part_s[part][lane] = s;
    __syncthreads();
    n = (n_s[0] + n_s[1]) + (n_s[2] + n_s[3]);
    if (part == 0) {
        if (q < dim && n > 0)                                 // a cluster with no member keeps its centre
            C[(int64_t)c * dim + q] =
                (float)(((part_s[0][lane] + part_s[1][lane]) + (part_s[2][lane] + part_s[3][lane])) / (double)n);
        if (q == 0) counts[c] = n;
    }
}

inline bool kmeans_sizes_ok(int64_t P, int64_t dim, int64_t k)
{
    return k >= 1 && k <= kMaxK && dim >= 1 && dim <= ((int64_t)1 << 30) && P >= 1 && P <= kMaxP &&
           P * dim < ((int64_t)1 << 40);
}

struct Plan {
    int G, chunk;                 // update: chunks of the points, points per chunk
    size_t hn_off, cnt_off, slab_off, total;
};

inline Plan kmeans_plan(int P, int dim, int k)
{
    Plan pl;
    int64_t G = ((int64_t)P + kChunkPts - 1) / kChunkPts;
    if (G > kMaxChunks) G = kMaxChunks;
    int64_t cap = (int64_t)(kSlabBytes / ((size_t)k * (size_t)dim * 8));
    if (cap < 1) cap = 1;
    if (G > cap) G = cap;
    pl.chunk = (int)(((int64_t)P + G - 1) / G);
    pl.G = (int)(((int64_t)P + pl.chunk - 1) / pl.chunk);
    pl.hn_off = 0;
    pl.cnt_off = align_up((size_t)kMaxK * 4);
    pl.slab_off = pl.cnt_off + align_up((size_t)pl.G * k * 4);
    pl.total = pl.slab_off + align_up((size_t)pl.G * k * dim * 8);
    return pl;
}

template <int WAVES, bool TWO>
int launch_deep(const float *pts, int P, int dim, const float *C, int k, const float *hn, int32_t *labels, float *dist2,
                int32_t *changed, hipStream_t st)
{
    constexpr size_t lds = (size_t)WAVES * deep_stage_floats(TWO) * 4;
    static size_t allowed = 0;
    MFCD_HIP_TRY(allow_dynamic_lds((const void *)kmeans_assign_deep_kernel<WAVES, TWO>, lds, allowed));
    hipLaunchKernelGGL((kmeans_assign_deep_kernel<WAVES, TWO>), dim3((unsigned)((P + 31) / 32)), dim3(64 * WAVES), lds, st,
                       pts, P, dim, C, k, hn, labels, dist2, changed);
    return 0;
}

}  // namespace

extern "C" int mfcd_kmeans_max_k(void) { return kMaxK; }

extern "C" size_t mfcd_kmeans_workspace_bytes(int64_t P, int64_t dim, int k)
{
    if (!kmeans_sizes_ok(P, dim, k)) return 0;
    return kmeans_plan((int)P, (int)dim, k).total;
}

extern "C" int mfcd_kmeans_assign(const float *points, int64_t P, int64_t dim, const float *centres, int k,
                                  int32_t *labels, float *dist2, int32_t *changed, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    if (!kmeans_sizes_ok(P, dim, k) || !points || !centres || !labels) return MFCD_EINVAL;
    if (((uintptr_t)points | (uintptr_t)centres | (uintptr_t)labels | (uintptr_t)dist2 | (uintptr_t)changed) & 3)
        return MFCD_EALIGN;
    if (!workspace || workspace_bytes < align_up((size_t)kMaxK * 4)) return MFCD_EWORKSPACE;
    if ((uintptr_t)workspace & 255) return MFCD_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    float *hn = static_cast<float *>(workspace);
    if (changed) MFCD_HIP_TRY(hipMemsetAsync(changed, 0, 4, st));
    hipLaunchKernelGGL(kmeans_half_norms_kernel, dim3((unsigned)k), dim3(MFCD_WAVE), 0, st, centres, (int)dim, hn);
    if (dim >= kDeepMinDim && (P + kPts - 1) / kPts < kDeepBelowBlocks) {
        const int rc = k > 32 ? launch_deep<4, true>(points, (int)P, (int)dim, centres, k, hn, labels, dist2, changed, st)
                              : launch_deep<8, false>(points, (int)P, (int)dim, centres, k, hn, labels, dist2, changed, st);
        if (rc) return rc;
    }
    else
        hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)((P + kPts - 1) / kPts)), dim3(256), 0, st, points, (int)P,
                           (int)dim, centres, k, hn, labels, dist2, changed);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mfcd_kmeans_update(const float *points, int64_t P, int64_t dim, const int32_t *labels, int k,
                                  float *centres, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!kmeans_sizes_ok(P, dim, k) || !points || !labels || !centres || !counts) return MFCD_EINVAL;
    if (((uintptr_t)points | (uintptr_t)centres | (uintptr_t)labels | (uintptr_t)counts) & 3) return MFCD_EALIGN;
    const Plan pl = kmeans_plan((int)P, (int)dim, k);
    if (!workspace || workspace_bytes < pl.total) return MFCD_EWORKSPACE;
    if ((uintptr_t)workspace & 255) return MFCD_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    char *base = static_cast<char *>(workspace);
    int32_t *cnt_slab = reinterpret_cast<int32_t *>(base + pl.cnt_off);
    double *slab = reinterpret_cast<double *>(base + pl.slab_off);
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)((dim + kCols - 1) / kCols), (unsigned)pl.G), dim3(kCols), 0,
                       st, points, (int)P, (int)dim, labels, k, pl.chunk, slab, cnt_slab);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)((dim + kCols - 1) / kCols), (unsigned)k), dim3(256), 0, st, slab,
                       cnt_slab, pl.G, (int)dim, k, centres, counts);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}
