// streaming.hip — fused optimiser step for triplet-comparison MF on gfx950 (streaming form), and the unfused
// building blocks of the split forms (mfcd_batch_coefficients .. mfcd_adam_dense) over the same kernels.
//
// One launch = one optimiser step of the reference loop (structure.py:847-851):
//   gather U[u],V[i],V[j] -> x -> sigmoid -> BCE backward coefficient g_t
//   -> row gradients accumulated in LDS (no dense gradient in HBM)
//   -> dense Adam with coupled L2 over every element (torch/optim/adam.py _single_tensor_adam).
//
// Ownership decomposition (no inter-workgroup communication inside a launch):
//   workgroup b owns a fixed flat range of E elements of one table (U or V) and the Adam moments
//   of that range.  It scans the batch (B 16-byte records), and for every sample that touches one
//   of its rows recomputes that sample's x_t from the INPUT copy of the tables and accumulates the
//   row gradient in LDS, in batch order (deterministic; all contributions to one row are handled
//   by one wave).  Parameters are ping-ponged (read Uin/Vin, write Uout/Vout) so that a workgroup
//   may read rows other workgroups are updating in the same launch; m and v are updated in place.
//   HBM traffic per element is the 24-byte minimum: read p,m,v, write p,m,v.
//
// Roofline: HBM-bound streaming; algorithmic bytes per step = 24*(n+m)*d + 12*B*d + 16*B.
#include "common.h"
#include "train_common.h"

using mfcd_detail::Plan;
using mfcd_detail::launch_streaming_step;
using mfcd_detail::make_plan;

namespace {

template <int VEC>
__device__ __forceinline__ void load_vec(const float *p, float (&r)[VEC])
{
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    } else {
        r[0] = *p;
    }
}

template <int VEC>
__device__ __forceinline__ void load_vec(const mfcd_bf16 *p, float (&r)[VEC])
{
    if constexpr (VEC == 4) {
        const uint2 t = *reinterpret_cast<const uint2 *>(p);   // 4 bf16 = 8 bytes
        r[0] = __uint_as_float(t.x << 16); r[1] = __uint_as_float(t.x & 0xffff0000u);
        r[2] = __uint_as_float(t.y << 16); r[3] = __uint_as_float(t.y & 0xffff0000u);
    } else {
        r[0] = (float)*p;
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(mfcd_bf16 *p, const float (&r)[VEC])
{
    if constexpr (VEC == 4) {   // round to nearest even, once per step (the defined rounding point)
        const unsigned short b0 = __builtin_bit_cast(unsigned short, (mfcd_bf16)r[0]);
        const unsigned short b1 = __builtin_bit_cast(unsigned short, (mfcd_bf16)r[1]);
        const unsigned short b2 = __builtin_bit_cast(unsigned short, (mfcd_bf16)r[2]);
        const unsigned short b3 = __builtin_bit_cast(unsigned short, (mfcd_bf16)r[3]);
        *reinterpret_cast<uint2 *>(p) = make_uint2((unsigned)b0 | ((unsigned)b1 << 16), (unsigned)b2 | ((unsigned)b3 << 16));
    } else {
        *p = (mfcd_bf16)r[0];
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *p, const float (&r)[VEC])
{
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
        *p = r[0];
    }
}

// E = 256 * VEC * CHUNKS elements per workgroup.
// MODE 0: the fused step.  MODE 1 (data-parallel, before the all-reduce): only this rank's dense gradient,
// Gu/Gv[e] = sum of the local samples' row gradients (no Adam, parameters untouched).  MODE 2 (after the
// all-reduce): Adam from the dense gradient Gu/Gv, no batch scan.  MODE 3 (row-sharded state, mfcd_shard_*): the
// tables are this rank's SHARDS (rows [u_off, u_off + n) of U, [v_off, v_off + m) of V), the batch names GLOBAL rows,
// and the three rows of every sample come from the exchange buffer g_in = xbuf[role][g_stride][d] (the rows as they
// were before this step, gathered from their owners), so the update is in place; workgroup 0 also forms every
// sample's BCE term, which makes the step's loss available on every rank without a collective.
template <int VEC, int CHUNKS, int MODE = 0, typename TP = float>
__global__ __launch_bounds__(256) void train_step_kernel(
    const TP *__restrict__ Uin, const TP *__restrict__ Vin, TP *__restrict__ Uout,
    TP *__restrict__ Vout, float *__restrict__ mU, float *__restrict__ vU, float *__restrict__ mV,
    float *__restrict__ vV, const mfcd_sample *__restrict__ batch, const float *__restrict__ g_in,
    int Bk, float inv_batch, int n, int m, int d, int blocksU, AdamConst ac,
    float *__restrict__ loss_terms, float *__restrict__ Gu, float *__restrict__ Gv, int g_stride, int u_off = 0,
    int v_off = 0)
{
    constexpr int E = 256 * VEC * CHUNKS;
    extern __shared__ __attribute__((aligned(16))) float sg[];  // [(row_hi-row_lo)*d] sparse row gradients

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool isV = (int)blockIdx.x >= blocksU;
    const int tb = isV ? (int)blockIdx.x - blocksU : (int)blockIdx.x;
    const int64_t cnt = (int64_t)(isV ? m : n) * d;
    const int64_t e0 = (int64_t)tb * E;
    const int64_t e1 = (e0 + E < cnt) ? e0 + E : cnt;
    const int row_lo = (int)(e0 / d);
    const int row_hi = (int)((e1 + d - 1) / d);
    const int sg_off = (int)(e0 - (int64_t)row_lo * d);  // position of element e0 inside sg

    const TP *__restrict__ Pin = isV ? Vin : Uin;
    TP *__restrict__ Pout = isV ? Vout : Uout;
    float *__restrict__ M1 = isV ? mV : mU;
    float *__restrict__ M2 = isV ? vV : vU;
    float *__restrict__ G = isV ? Gv : Gu;

    // ---- phase 0: put this workgroup's p, m, v loads in flight before touching the batch ----
    float pr[CHUNKS][VEC], mr[CHUNKS][VEC], vr[CHUNKS][VEC];
    if constexpr (MODE != 1) {
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int64_t e = e0 + (int64_t)(c * 256 + tid) * VEC;
            if (e < e1) {
                load_vec<VEC>(Pin + e, pr[c]);
                load_vec<VEC>(M1 + e, mr[c]);
                load_vec<VEC>(M2 + e, vr[c]);
            }
        }
    }

    // ---- phase 1: which samples of the batch touch my rows? ----
    int any = 0;
    for (int base = 0; MODE != 2 && base < Bk; base += MFCD_WAVE) {
        const int t = base + lane;
        if (t < Bk) {
            mfcd_sample s = batch[t];
            if constexpr (MODE == 3) { s.u -= u_off; s.i -= v_off; s.j -= v_off; }   // global -> shard-local rows
            if (isV)
                any |= (s.i >= row_lo && s.i < row_hi) | (s.j >= row_lo && s.j < row_hi);
            else
                any |= (s.u >= row_lo && s.u < row_hi);
        }
    }
    if constexpr (MODE != 2) any = __syncthreads_or(any);

    if constexpr (MODE == 3) {
        // every rank holds all three rows of every sample: workgroup 0 records all BCE terms (same dot-product order as
        // the owner-recorded term of MODE 0)
        if (blockIdx.x == 0 && loss_terms) {
            const float *xb = reinterpret_cast<const float *>(g_in);
            for (int t = wave; t < Bk; t += 4) {
                const float *ur = xb + (int64_t)t * d, *vi = xb + ((int64_t)g_stride + t) * d,
                            *vj = xb + ((int64_t)2 * g_stride + t) * d;
                float acc = 0.0f;
                for (int k = lane; k < d; k += MFCD_WAVE) acc += ur[k] * (vi[k] - vj[k]);
                const float p = sigmoid_f32(wave_sum64(acc));
                if (lane == 0) loss_terms[t] = bce_term_f32(p, batch[t].z);
            }
        }
    }

    if (MODE != 2 && any) {
        const int nsg = (row_hi - row_lo) * d;
        for (int k = tid; k < nsg; k += 256) sg[k] = 0.0f;
        __syncthreads();
        // every wave walks the batch in order and takes the rows congruent to its id (mod 4)
        for (int base = 0; base < Bk; base += MFCD_WAVE) {
            const int t = base + lane;
            mfcd_sample s;
            s.u = s.i = s.j = -1;
            s.z = 0.0f;
            if (t < Bk) {
                s = batch[t];
                if constexpr (MODE == 3) { s.u -= u_off; s.i -= v_off; s.j -= v_off; }
            }
            const bool hu = !isV && s.u >= row_lo && s.u < row_hi && ((s.u - row_lo) & 3) == wave;
            const bool hi = isV && s.i >= row_lo && s.i < row_hi && ((s.i - row_lo) & 3) == wave;
            const bool hj = isV && s.j >= row_lo && s.j < row_hi && ((s.j - row_lo) & 3) == wave;
            const unsigned long long mu = __ballot(hu), mi = __ballot(hi), mj = __ballot(hj);
            unsigned long long mask = mu | mi | mj;
            while (mask) {
                const int tl = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int uu = __shfl(s.u, tl, MFCD_WAVE), ii = __shfl(s.i, tl, MFCD_WAVE),
                          jj = __shfl(s.j, tl, MFCD_WAVE);
                const float zz = __shfl(s.z, tl, MFCD_WAVE);
                // MODE 3: the rows of sample base + tl as gathered before this step — always fp32 in the exchange buffer
                // (bf16 tables are widened exactly by the pack kernels)
                using XT = typename std::conditional<MODE == 3, float, TP>::type;
                const XT *ur, *vi, *vj;
                if constexpr (MODE == 3) {
                    ur = g_in + (int64_t)(base + tl) * d;
                    vi = g_in + ((int64_t)g_stride + base + tl) * d;
                    vj = g_in + ((int64_t)2 * g_stride + base + tl) * d;
                } else {
                    ur = Uin + (int64_t)uu * d;
                    vi = Vin + (int64_t)ii * d;
                    vj = Vin + (int64_t)jj * d;
                }
                float g;
                if (MODE != 3 && g_in) {
                    g = g_in[(base + tl) * g_stride];   // stride 2: interleaved {g, term} pairs of the DP exchange
                } else {
                    float acc = 0.0f;
                    for (int k = lane; k < d; k += MFCD_WAVE) acc += ldf(ur, k) * (ldf(vi, k) - ldf(vj, k));
                    const float p = sigmoid_f32(wave_sum64(acc));
                    g = bce_sigmoid_backward_f32(p, zz, inv_batch);
                    // the workgroup that owns the first element of row u records the loss term
                    if (MODE != 3 && ((mu >> tl) & 1ull) && loss_terms && lane == 0) {
                        const int64_t first = (int64_t)uu * d;
                        if (first >= e0 && first < e1) loss_terms[base + tl] = bce_term_f32(p, zz);
                    }
                }
                if ((mu >> tl) & 1ull) {
                    float *dst = sg + (int64_t)(uu - row_lo) * d;
                    for (int k = lane; k < d; k += MFCD_WAVE) dst[k] += g * (ldf(vi, k) - ldf(vj, k));
                }
                if ((mi >> tl) & 1ull) {
                    float *dst = sg + (int64_t)(ii - row_lo) * d;
                    for (int k = lane; k < d; k += MFCD_WAVE) dst[k] += g * ldf(ur, k);
                }
                if ((mj >> tl) & 1ull) {
                    float *dst = sg + (int64_t)(jj - row_lo) * d;
                    for (int k = lane; k < d; k += MFCD_WAVE) dst[k] += -(g * ldf(ur, k));
                }
            }
        }
        __syncthreads();
    }

    // ---- phase 2: dense Adam over my range (MODE 1: write the dense gradient instead) ----
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
        const int loc = (c * 256 + tid) * VEC;
        const int64_t e = e0 + loc;
        if (e < e1) {
            float gs[VEC];
            if constexpr (MODE == 2) {
                load_vec<VEC>(G + e, gs);
            } else if (any) {
                load_vec<VEC>(sg + sg_off + loc, gs);
            } else {
#pragma unroll
                for (int q = 0; q < VEC; ++q) gs[q] = 0.0f;
            }
            if constexpr (MODE == 1) {
                store_vec<VEC>(G + e, gs);
            } else {
                float po[VEC], mo[VEC], vo[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    po[q] = pr[c][q];
                    mo[q] = mr[c][q];
                    vo[q] = vr[c][q];
                    adam_update(po[q], mo[q], vo[q], gs[q], ac.st, ac.sc);
                }
                store_vec<VEC>(Pout + e, po);
                store_vec<VEC>(M1 + e, mo);
                store_vec<VEC>(M2 + e, vo);
            }
        }
    }
}

// One wave per sample: sigmoid output, BCE term and backward coefficient (split DP form).
__global__ __launch_bounds__(256) void coeff_kernel(const float *__restrict__ U, const float *__restrict__ V,
                                                    const mfcd_sample *__restrict__ batch, int B, int d,
                                                    float inv_batch, float *__restrict__ g_out,
                                                    float *__restrict__ term_out, float *__restrict__ p_out)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= B) return;
    const mfcd_sample s = batch[t];
    const float p = sigmoid_f32(wave_score(U, V, s.u, s.i, s.j, d, lane));
    if (lane == 0) {
        if (g_out) g_out[t] = bce_sigmoid_backward_f32(p, s.z, inv_batch);
        if (term_out) term_out[t] = bce_term_f32(p, s.z);
        if (p_out) p_out[t] = p;
    }
}

// out[k] = mean(terms[k*B .. min((k+1)*B,N))) — one wave per batch, fixed summation order.
// With `samples` set, terms[] holds sigmoid outputs p and the BCE term is formed here from p and the label
// (the resident kernel keeps the logs off its critical path); otherwise terms[] holds ready BCE terms.
// segs != nullptr (mfcd_train_steps_local_multi): a flat (model, step) grid; block b is step b - blk_begin of the model
// of the segment it falls in, and the arguments before `segs` are that model's.
__global__ __launch_bounds__(64) void batch_mean_kernel(const float *__restrict__ terms,
                                                        const mfcd_sample *__restrict__ samples, int64_t N, int B,
                                                        float *__restrict__ out,
                                                        const mfcd_detail::MeanSeg *__restrict__ segs, int nseg)
{
    int64_t blk = blockIdx.x;
    if (segs) {
        const mfcd_detail::MeanSeg &sg = segs[mfcd_detail::find_seg(segs, nseg, blk)];
        terms = sg.terms; samples = sg.samples; N = sg.N; B = sg.B; out = sg.out;
        blk -= sg.blk_begin;
    }
    const int lane = threadIdx.x;
    const int64_t off = blk * B;
    const int b = (int)((N - off) < B ? (N - off) : B);
    float acc = 0.0f;
    for (int t = lane; t < b; t += MFCD_WAVE)
        acc += samples ? bce_term_f32(terms[off + t], samples[off + t].z) : terms[off + t];
    acc = wave_sum64(acc);
    if (lane == 0) out[blk] = acc / (float)b;
}
constexpr const mfcd_detail::MeanSeg *kNoSegs = nullptr;

template <int VEC, int CHUNKS, int MODE, typename TP>
void launch_step(const Plan &pl, hipStream_t st, const TP *Uin, const TP *Vin, TP *Uout, TP *Vout,
                 float *mU, float *vU, float *mV, float *vV, const mfcd_sample *batch, const float *g_in, int Bk,
                 float inv_batch, int n, int m, int d, const AdamConst &ac, float *loss_terms, float *Gu, float *Gv,
                 int g_stride, int u_off, int v_off)
{
    hipLaunchKernelGGL((train_step_kernel<VEC, CHUNKS, MODE, TP>), dim3(pl.blocksU + pl.blocksV), dim3(256), pl.lds, st,
                       Uin, Vin, Uout, Vout, mU, vU, mV, vV, batch, g_in, Bk, inv_batch, n, m, d, pl.blocksU, ac,
                       loss_terms, Gu, Gv, g_stride, u_off, v_off);
}

}  // namespace

namespace mfcd_detail {

Plan make_plan(const void *const *ptrs, int nptrs, int n, int m, int d)
{
    Plan pl;
    bool al16 = (d % 4) == 0;
    for (int k = 0; k < nptrs; ++k) al16 = al16 && ((reinterpret_cast<uintptr_t>(ptrs[k]) & 15u) == 0);
    pl.vec = al16 ? 4 : 1;
    const int64_t total = (int64_t)(n + m) * d;
    pl.chunks = 1;
    // at most 4 chunks (16 KiB of each array per workgroup): measured at C3 / C4 / C5 size (profiles/r02_stream_chunks.txt),
    // 8 chunks cost 4-10 % (fewer workgroups in flight per CU: the per-workgroup LDS tile doubles)
    while (pl.chunks < 4 && total / (256 * pl.vec * pl.chunks) > 2048) pl.chunks *= 2;
    pl.E = 256 * pl.vec * pl.chunks;
    pl.blocksU = (int)(((int64_t)n * d + pl.E - 1) / pl.E);
    pl.blocksV = (int)(((int64_t)m * d + pl.E - 1) / pl.E);
    pl.lds = sizeof(float) * (size_t)(pl.E + 2 * d);
    return pl;
}

template <int MODE, typename TP>
void launch_streaming_step(const Plan &pl, hipStream_t st, const TP *Uin, const TP *Vin, TP *Uout, TP *Vout, float *mU,
                           float *vU, float *mV, float *vV, const mfcd_sample *batch, const float *g_in, int Bk,
                           float inv_batch, int n, int m, int d, const AdamConst &ac, float *loss_terms, float *Gu,
                           float *Gv, int g_stride, int u_off, int v_off)
{
#define MFCD_CASE(V, C)                                                                                              \
    if (pl.vec == V && pl.chunks == C)                                                                               \
        return launch_step<V, C, MODE, TP>(pl, st, Uin, Vin, Uout, Vout, mU, vU, mV, vV, batch, g_in, Bk, inv_batch, \
                                           n, m, d, ac, loss_terms, Gu, Gv, g_stride, u_off, v_off);
    MFCD_CASE(4, 1) MFCD_CASE(4, 2) MFCD_CASE(4, 4)
    MFCD_CASE(1, 1) MFCD_CASE(1, 2) MFCD_CASE(1, 4)
#undef MFCD_CASE
}

// the (MODE, TP) pairs other units launch (MODE 1 and 2 are instantiated by the entry points below)
#define MFCD_INST(MODE, TP)                                                                                         \
    template void launch_streaming_step<MODE, TP>(const Plan &, hipStream_t, const TP *, const TP *, TP *, TP *,    \
                                                  float *, float *, float *, float *, const mfcd_sample *,         \
                                                  const float *, int, float, int, int, int, const AdamConst &,     \
                                                  float *, float *, float *, int, int, int);
MFCD_INST(0, float) MFCD_INST(0, mfcd_bf16) MFCD_INST(3, float) MFCD_INST(3, mfcd_bf16)
#undef MFCD_INST

int launch_batch_means(const float *terms, const mfcd_sample *samples, int64_t N, int B, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(batch_mean_kernel, dim3((unsigned)((N + B - 1) / B)), dim3(64), 0, st, terms, samples, N, B, out,
                       kNoSegs, 0);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

int launch_batch_means_multi(const MeanSeg *segs_dev, int nseg, int64_t blocks, hipStream_t st)
{
    hipLaunchKernelGGL(batch_mean_kernel, dim3((unsigned)blocks), dim3(64), 0, st, (const float *)nullptr,
                       (const mfcd_sample *)nullptr, (int64_t)0, 1, (float *)nullptr, segs_dev, nseg);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mfcd_detail

namespace {

size_t streaming_bytes(int64_t N, int n, int m, int d)   // mfcd_apply_step's own (unregistered) workspace
{
    return kStatusBytes + align_up(sizeof(float) * (size_t)n * d) + align_up(sizeof(float) * (size_t)m * d) +
           align_up(sizeof(float) * (size_t)(N > 0 ? N : 1));
}

}  // namespace

extern "C" int mfcd_batch_coefficients(const float *U, const float *V, const mfcd_sample *samples, int B, int n,
                                       int m, int d, int batch_divisor, float *g_out, float *term_out,
                                       float *p_out, void *stream)
{
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (B < 0 || batch_divisor <= 0) return MFCD_EINVAL;
    if (B == 0) return 0;
    if (!samples) return MFCD_EINVAL;
    hipLaunchKernelGGL(coeff_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, U, V, samples, B, d,
                       1.0f / (float)batch_divisor, g_out, term_out, p_out);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mfcd_apply_step(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                               const mfcd_sample *samples, const float *g, int B, int64_t step, int n, int m, int d,
                               double lr, double beta1, double beta2, double eps, double weight_decay,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (!mU || !vU || !mV || !vV || B < 0 || step < 1 || !workspace) return MFCD_EINVAL;
    if (B > 0 && (!samples || !g)) return MFCD_EINVAL;
    if (workspace_bytes < streaming_bytes(B, n, m, d)) return MFCD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace + kStatusBytes;
    float *Ualt = (float *)ws;
    ws += align_up(sizeof(float) * (size_t)n * d);
    float *Valt = (float *)ws;
    const void *ptrs[] = {U, V, mU, vU, mV, vV, Ualt, Valt};
    const Plan pl = make_plan(ptrs, 8, n, m, d);
    const AdamConst ac = adam_const({lr, beta1, beta2, eps, weight_decay}, step);
    launch_streaming_step<0, float>(pl, st, U, V, Ualt, Valt, mU, vU, mV, vV, samples, g, B, 0.0f, n, m, d, ac,
                                    nullptr);
    MFCD_HIP_TRY(hipGetLastError());
    MFCD_HIP_TRY(hipMemcpyAsync(U, Ualt, sizeof(float) * (size_t)n * d, hipMemcpyDeviceToDevice, st));
    MFCD_HIP_TRY(hipMemcpyAsync(V, Valt, sizeof(float) * (size_t)m * d, hipMemcpyDeviceToDevice, st));
    return 0;
}

extern "C" int mfcd_dense_grad(const float *U, const float *V, const mfcd_sample *samples, int B, int n, int m, int d,
                               int batch_divisor, float *gradU, float *gradV, float *term_out, void *stream)
{
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (!gradU || !gradV || B < 0 || batch_divisor <= 0) return MFCD_EINVAL;
    if (B > 0 && !samples) return MFCD_EINVAL;
    const void *ptrs[] = {U, V, gradU, gradV};
    const Plan pl = make_plan(ptrs, 4, n, m, d);
    AdamConst ac{};
    launch_streaming_step<1, float>(pl, (hipStream_t)stream, U, V, (float *)nullptr, (float *)nullptr, nullptr, nullptr,
                                    nullptr, nullptr, samples, nullptr, B, 1.0f / (float)batch_divisor, n, m, d, ac,
                                    term_out, gradU, gradV);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mfcd_dense_grad_from_coefficients(const float *U, const float *V, const mfcd_sample *samples,
                                                 const float *g, int B, int n, int m, int d, float *gradU,
                                                 float *gradV, void *stream)
{
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (!gradU || !gradV || B < 0) return MFCD_EINVAL;
    if (B > 0 && (!samples || !g)) return MFCD_EINVAL;
    const void *ptrs[] = {U, V, gradU, gradV};
    const Plan pl = make_plan(ptrs, 4, n, m, d);
    AdamConst ac{};
    launch_streaming_step<1, float>(pl, (hipStream_t)stream, U, V, (float *)nullptr, (float *)nullptr, nullptr, nullptr,
                                    nullptr, nullptr, samples, g, B, 0.0f, n, m, d, ac, nullptr, gradU, gradV);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mfcd_adam_dense(float *U, float *V, float *mU, float *vU, float *mV, float *vV, const float *gradU,
                               const float *gradV, int64_t step, int n, int m, int d, double lr, double beta1,
                               double beta2, double eps, double weight_decay, void *stream)
{
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (!mU || !vU || !mV || !vV || !gradU || !gradV || step < 1) return MFCD_EINVAL;
    const void *ptrs[] = {U, V, mU, vU, mV, vV, gradU, gradV};
    const Plan pl = make_plan(ptrs, 8, n, m, d);
    const AdamConst ac = adam_const({lr, beta1, beta2, eps, weight_decay}, step);
    // element-wise: reading and writing the same element in place is safe (no gather in this mode)
    launch_streaming_step<2, float>(pl, (hipStream_t)stream, U, V, U, V, mU, vU, mV, vV, nullptr, nullptr, 0, 0.0f, n,
                                    m, d, ac, nullptr, const_cast<float *>(gradU), const_cast<float *>(gradV));
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}
