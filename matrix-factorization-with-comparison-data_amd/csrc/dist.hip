// dist.hip — the multi-GPU training loops (G1): data-parallel (mfcd_dp_*) and row-sharded (mfcd_shard_*), with RCCL
// bound at run time (rccl_dyn.h).  The fused step of every rank is the streaming form's (streaming.hip).
#include <cstring>
#include <vector>

#include "common.h"
#include "rccl_dyn.h"
#include "train_common.h"

using mfcd_detail::Plan;
using mfcd_detail::launch_streaming_step;
using mfcd_detail::make_plan;

// ---------------------------------------------------------------------------------------------------------------
// Data-parallel training loop, native: per optimiser step one coefficient kernel over this rank's shard, ONE RCCL
// all-gather (in place) of B {g, term} pairs per rank, one fused step kernel over the whole global batch — all
// enqueued from here on one stream with no host synchronisation (replaces the per-step Python loop of mfcd/dist.py
// for the "allgather" exchange; same protocol, same results).
namespace {

// One multi-GPU training call as its extern "C" entry (mfcd_dp_train_steps*, mfcd_shard_train_steps*) received it;
// MFCD_DIST_CALL packs the arguments of those four entries, which share their parameter names
struct DistCall {
    AdamTables t;
    const mfcd_sample *samples;
    int64_t N, step0;
    int B, rank, world, n, m, d;
    AdamHyper h;
    float *loss_per_step;
    void *workspace, *comm, *stream;
    size_t workspace_bytes;
};
#define MFCD_DIST_CALL                                                                                      \
    DistCall{{U, V, mU, vU, mV, vV}, samples, N, step0, B, rank, world, n, m, d, {lr, beta1, beta2, eps, weight_decay}, \
             loss_per_step, workspace, comm, stream, workspace_bytes}

// Data-parallel exchange slot of one rank for one step: B interleaved pairs {g_t, BCE term_t}; one wave per slot entry.
// Entries past the rank's (possibly short or empty) shard are written as {0, 0} so that the gathered buffer of a
// step is fully defined.
template <typename TP>
__global__ __launch_bounds__(256) void dp_coeff_kernel(const TP *__restrict__ U, const TP *__restrict__ V,
                                                       const mfcd_sample *__restrict__ shard, int myB, int B, int d,
                                                       float inv_batch, float2 *__restrict__ slot)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= B) return;
    if (t >= myB) {
        if (lane == 0) slot[t] = make_float2(0.0f, 0.0f);
        return;
    }
    const mfcd_sample s = shard[t];
    const float p = sigmoid_f32(wave_score(U, V, s.u, s.i, s.j, d, lane));
    if (lane == 0) slot[t] = make_float2(bce_sigmoid_backward_f32(p, s.z, inv_batch), bce_term_f32(p, s.z));
}

// out[k] = mean of the BCE terms of global batch k from the gathered exchange buffer xbuf[k][world*B] (pairs);
// one wave per step, fixed summation order (identical on every rank).
__global__ __launch_bounds__(64) void dp_loss_kernel(const float2 *__restrict__ xbuf, int64_t N, int Bg,
                                                     float *__restrict__ out)
{
    const int lane = threadIdx.x;
    const int64_t off = (int64_t)blockIdx.x * Bg;
    const int b = (int)((N - off) < Bg ? (N - off) : Bg);
    float acc = 0.0f;
    for (int t = lane; t < b; t += MFCD_WAVE) acc += xbuf[off + t].y;
    acc = wave_sum64(acc);
    if (lane == 0) out[blockIdx.x] = acc / (float)b;
}

}  // namespace

extern "C" int mfcd_dp_unique_id(void *id_out, size_t id_bytes)
{
    if (!id_out || id_bytes < sizeof(ncclUniqueId)) return MFCD_EINVAL;
    const mfcd_detail::RcclApi &R = mfcd_detail::rccl();
    if (!R.ok) return MFCD_ERCCL;
    ncclUniqueId id;
    if (R.GetUniqueId(&id) != ncclSuccess) return MFCD_ERCCL;
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

extern "C" int mfcd_dp_comm_create(const void *id, size_t id_bytes, int rank, int world, void **comm_out)
{
    if (!id || id_bytes < sizeof(ncclUniqueId) || !comm_out || world < 1 || rank < 0 || rank >= world) return MFCD_EINVAL;
    const mfcd_detail::RcclApi &R = mfcd_detail::rccl();
    if (!R.ok) return MFCD_ERCCL;
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    if (R.CommInitRank(&comm, world, uid, rank) != ncclSuccess) return MFCD_ERCCL;
    *comm_out = (void *)comm;
    return 0;
}

extern "C" int mfcd_dp_comm_destroy(void *comm)
{
    if (!comm) return 0;
    const mfcd_detail::RcclApi &R = mfcd_detail::rccl();
    if (!R.ok) return MFCD_ERCCL;
    return R.CommDestroy((ncclComm_t)comm) == ncclSuccess ? 0 : MFCD_ERCCL;
}

extern "C" size_t mfcd_dp_workspace_bytes(int64_t N, int B, int world, int n, int m, int d)
{
    if (N < 0 || B <= 0 || world < 1 || n <= 0 || m <= 0 || d <= 0) return 0;
    const int64_t Bg = (int64_t)B * world, nsteps = (N + Bg - 1) / Bg;
    return kStatusBytes + align_up(sizeof(float) * (size_t)n * d) + align_up(sizeof(float) * (size_t)m * d) +
           align_up(sizeof(float2) * (size_t)(nsteps > 0 ? nsteps : 1) * (size_t)Bg);
}

namespace {
template <typename TP>   // fp32 or bf16 factor tables; the moments, the coefficients on the wire and the arithmetic are fp32
int run_dp_train_steps(const DistCall &c)
{
    TP *U = (TP *)c.t.U, *V = (TP *)c.t.V;
    float *mU = c.t.mU, *vU = c.t.vU, *mV = c.t.mV, *vV = c.t.vV, *loss_per_step = c.loss_per_step;
    const mfcd_sample *samples = c.samples;
    const int64_t N = c.N, step0 = c.step0;
    const int B = c.B, rank = c.rank, world = c.world, n = c.n, m = c.m, d = c.d;
    void *workspace = c.workspace, *comm = c.comm;
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (!mU || !vU || !mV || !vV || N < 0 || B <= 0 || world < 1 || rank < 0 || rank >= world || step0 < 0)
        return MFCD_EINVAL;
    if (N == 0) return 0;
    if (!samples || !workspace) return MFCD_EINVAL;
    if (c.workspace_bytes < mfcd_dp_workspace_bytes(N, B, world, n, m, d)) return MFCD_EWORKSPACE;
    const mfcd_detail::RcclApi *R = nullptr;
    if (comm) {
        R = &mfcd_detail::rccl();
        if (!R->ok) return MFCD_ERCCL;
    }
    hipStream_t st = (hipStream_t)c.stream;
    const int64_t Bg = (int64_t)B * world, nsteps = (N + Bg - 1) / Bg;
    char *ws = (char *)workspace + kStatusBytes;
    TP *Ualt = (TP *)ws;
    ws += align_up(sizeof(float) * (size_t)n * d);
    TP *Valt = (TP *)ws;
    ws += align_up(sizeof(float) * (size_t)m * d);
    float2 *xbuf = (float2 *)ws;   // [nsteps][world][B] pairs = global sample order inside a step
    const void *ptrs[] = {U, V, mU, vU, mV, vV, Ualt, Valt};
    const Plan pl = make_plan(ptrs, 8, n, m, d);
    for (int64_t k = 0; k < nsteps; ++k) {
        const int64_t lo = k * Bg, hi = (lo + Bg < N) ? lo + Bg : N;
        const int nglob = (int)(hi - lo);          // divisor of the mean (structure.py:849): the GLOBAL batch
        const bool even = (k & 1) == 0;
        const TP *Uc = even ? U : Ualt, *Vc = even ? V : Valt;
        float2 *xk = xbuf + (size_t)k * Bg;
        // ranks this process computes: its own; or, without a communicator, every rank in turn (replicas are
        // bit-identical, so this reproduces the gathered buffer exactly: single-process rehearsal of any world size)
        const int r0 = comm ? rank : 0, r1 = comm ? rank + 1 : world;
        for (int r = r0; r < r1; ++r) {
            const int64_t mylo = (lo + (int64_t)r * B < hi) ? lo + (int64_t)r * B : hi;
            const int64_t myhi = (mylo + B < hi) ? mylo + B : hi;
            hipLaunchKernelGGL(dp_coeff_kernel<TP>, dim3((B + 3) / 4), dim3(256), 0, st, Uc, Vc, samples + mylo,
                               (int)(myhi - mylo), B, d, 1.0f / (float)nglob, xk + (size_t)r * B);
        }
        if (comm) {   // also on a one-rank communicator: the call path is the same at every world size
            if (R->AllGather(xk + (size_t)rank * B, xk, (size_t)B * 2, ncclFloat, (ncclComm_t)comm, st) != ncclSuccess)
                return MFCD_ERCCL;
        }
        const AdamConst ac = adam_const(c.h, step0 + k + 1);
        launch_streaming_step<0, TP>(pl, st, Uc, Vc, even ? Ualt : U, even ? Valt : V, mU, vU, mV, vV, samples + lo,
                                     (const float *)xk, nglob, 0.0f, n, m, d, ac, nullptr, nullptr, nullptr, 2);
    }
    MFCD_HIP_TRY(hipGetLastError());
    if (nsteps & 1) {
        MFCD_HIP_TRY(hipMemcpyAsync(U, Ualt, sizeof(TP) * (size_t)n * d, hipMemcpyDeviceToDevice, st));
        MFCD_HIP_TRY(hipMemcpyAsync(V, Valt, sizeof(TP) * (size_t)m * d, hipMemcpyDeviceToDevice, st));
    }
    if (loss_per_step) {
        hipLaunchKernelGGL(dp_loss_kernel, dim3((unsigned)nsteps), dim3(64), 0, st, xbuf, N, (int)Bg, loss_per_step);
        MFCD_HIP_TRY(hipGetLastError());
    }
    return 0;
}
}  // namespace

extern "C" int mfcd_dp_train_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                                   const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0,
                                   int n, int m, int d, double lr, double beta1, double beta2, double eps,
                                   double weight_decay, float *loss_per_step, void *workspace, size_t workspace_bytes,
                                   void *comm, void *stream)
{
    return run_dp_train_steps<float>(MFCD_DIST_CALL);
}

extern "C" int mfcd_dp_train_steps_bf16(uint16_t *U, uint16_t *V, float *mU, float *vU, float *mV, float *vV,
                                        const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0,
                                        int n, int m, int d, double lr, double beta1, double beta2, double eps,
                                        double weight_decay, float *loss_per_step, void *workspace,
                                        size_t workspace_bytes, void *comm, void *stream)
{
    return run_dp_train_steps<mfcd_bf16>(MFCD_DIST_CALL);
}

// ---------------------------------------------------------------------------------------------------------------
// Row-sharded training (strong scaling): rank r holds rows [lo_r, hi_r) of U, V and of their Adam
// moments; the batch stays the reference's B (structure.py:668) and every rank sees the same records, so the run equals
// the single-GPU run with the same B.  Per optimiser step: (1) every rank writes the rows of the batch it owns into an
// exchange buffer xbuf[role][B][d] (zeros elsewhere), (2) ONE all-reduce(sum) of the buffer taken as 32-bit integers —
// exactly one rank contributes non-zero bits per row, so the sum reproduces the rows bit for bit — (3) the fused step
// (MODE 3 of train_step_kernel) over the shard, in place, with the dense Adam sweep over 1/R of the state.
namespace {

template <typename TP>
__global__ __launch_bounds__(256) void shard_pack_kernel(const TP *__restrict__ Us, const TP *__restrict__ Vs,
                                                         const mfcd_sample *__restrict__ batch, int Bk, int Bcap, int d,
                                                         int u_off, int nu, int v_off, int nv, float *__restrict__ xbuf,
                                                         int merge)
{
    // merge = 0: every row of the buffer is written (zeros where this rank owns nothing): the input of the all-reduce;
    // merge = 1: only owned rows are written on top of what is there (single-process rehearsal of the all-reduce)
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);   // (role, t)
    if (w >= 3 * Bcap) return;
    const int role = w / Bcap, t = w - role * Bcap;
    const TP *src = nullptr;
    if (t < Bk) {
        const mfcd_sample s = batch[t];
        const int row = role == 0 ? s.u - u_off : (role == 1 ? s.i : s.j) - v_off;
        if (row >= 0 && row < (role == 0 ? nu : nv)) src = (role == 0 ? Us : Vs) + (int64_t)row * d;
    }
    if (merge && !src) return;
    float *dst = xbuf + (int64_t)w * d;
    for (int k = lane; k < d; k += MFCD_WAVE) dst[k] = src ? ldf(src, k) : 0.0f;   // bf16 rows widen exactly
}

// Exchange rows of the NEXT batch, rolled forward over the step that is about to run (the look-ahead rule of the
// resident form): a row that the current batch does not touch changes in that step by the dense update with
// a zero sparse gradient alone, a pure function of its (p, m, v) — so its value AFTER the step can be put on the wire
// BEFORE the step runs, and the collective of batch k+1 overlaps the step of batch k.  Same adam_update, same operation
// order as the step kernel: the rolled value equals the in-place one bit for bit (rehearsal tests).  The caller
// guarantees that no row of `next` is named by the current batch (mfcd_shard_collisions).
template <typename TP>
__global__ __launch_bounds__(256) void shard_pack_ahead_kernel(const TP *__restrict__ Us, const TP *__restrict__ Vs,
                                                               const float *__restrict__ mU, const float *__restrict__ vU,
                                                               const float *__restrict__ mV, const float *__restrict__ vV,
                                                               const mfcd_sample *__restrict__ next, int Bk, int Bcap,
                                                               int d, int u_off, int nu, int v_off, int nv, AdamConst ac,
                                                               float *__restrict__ xbuf, int merge)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);   // (role, t)
    if (w >= 3 * Bcap) return;
    const int role = w / Bcap, t = w - role * Bcap;
    int64_t src = -1;
    if (t < Bk) {
        const mfcd_sample s = next[t];
        const int row = role == 0 ? s.u - u_off : (role == 1 ? s.i : s.j) - v_off;
        if (row >= 0 && row < (role == 0 ? nu : nv)) src = (int64_t)row * d;
    }
    if (merge && src < 0) return;
    float *dst = xbuf + (int64_t)w * d;
    const TP *P = role == 0 ? Us : Vs;
    const float *M1 = role == 0 ? mU : mV, *M2 = role == 0 ? vU : vV;
    for (int k = lane; k < d; k += MFCD_WAVE) {
        float v = 0.0f;
        if (src >= 0) {
            float p = ldf(P, src + k), m1 = M1[src + k], m2 = M2[src + k];
            adam_update(p, m1, m2, 0.0f, ac.st, ac.sc);
            if constexpr (sizeof(TP) == 2) p = (float)(mfcd_bf16)p;   // the step's one rounding point (store_vec)
            v = p;
        }
        dst[k] = v;
    }
}

// flags[k] = 1 when batch k+1 names a row that batch k names too (same table), 0 otherwise and for the last batch.
__global__ __launch_bounds__(256) void shard_collisions_kernel(const mfcd_sample *__restrict__ samples, int64_t N, int B,
                                                               int64_t nsteps, uint8_t *__restrict__ flags)
{
    const int64_t k = blockIdx.x;
    __shared__ int hit;
    if (threadIdx.x == 0) hit = 0;
    __syncthreads();
    if (k + 1 < nsteps) {
        const int64_t o0 = k * B, o1 = (k + 1) * B;
        const int b0 = (int)((N - o0) < B ? (N - o0) : B), b1 = (int)((N - o1) < B ? (N - o1) : B);
        int mine = 0;
        for (int64_t pr = threadIdx.x; pr < (int64_t)b0 * b1 && !mine; pr += 256) {
            const mfcd_sample a = samples[o0 + pr / b1], b = samples[o1 + pr % b1];
            mine = (a.u == b.u) | (a.i == b.i) | (a.i == b.j) | (a.j == b.i) | (a.j == b.j);
        }
        if (mine) hit = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) flags[k] = (uint8_t)hit;
}

void shard_range(int rows, int rank, int world, int *lo, int *hi)
{
    *lo = (int)((int64_t)rows * rank / world);
    *hi = (int)((int64_t)rows * (rank + 1) / world);
}

struct ShardRows { int u_lo, u_hi, v_lo, v_hi; };   // one rank holds rows [u_lo, u_hi) of U and [v_lo, v_hi) of V

size_t shard_xbuf_bytes(int B, int d) { return align_up(sizeof(float) * 3 * (size_t)B * d); }

// BCE terms of a batch from the exchange buffer alone: what workgroup 0 of the MODE 3 step records, for a rank whose
// shard is EMPTY (more ranks than rows) and therefore launches no step kernel.  Same dot-product order.
__global__ __launch_bounds__(256) void shard_terms_kernel(const float *__restrict__ xb, const mfcd_sample *__restrict__ batch,
                                                          int Bk, int Bcap, int d, float *__restrict__ loss_terms)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= Bk) return;
    const float *ur = xb + (int64_t)t * d, *vi = xb + ((int64_t)Bcap + t) * d, *vj = xb + ((int64_t)2 * Bcap + t) * d;
    float acc = 0.0f;
    for (int k = lane; k < d; k += MFCD_WAVE) acc += ur[k] * (vi[k] - vj[k]);
    const float p = sigmoid_f32(wave_sum64(acc));
    if (lane == 0) loss_terms[t] = bce_term_f32(p, batch[t].z);
}

}  // namespace

extern "C" int mfcd_shard_rows(int rows, int rank, int world, int *lo, int *hi)
{
    if (rows <= 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return MFCD_EINVAL;
    shard_range(rows, rank, world, lo, hi);
    return 0;
}

extern "C" size_t mfcd_shard_workspace_bytes(int64_t N, int B, int d)
{
    if (N < 0 || B <= 0 || d <= 0) return 0;
    const size_t nsteps = (size_t)((N + B - 1) / B);
    return 2 * shard_xbuf_bytes(B, d) + align_up(sizeof(float) * (size_t)(N > 0 ? N : 1)) + align_up(nsteps + 1);
}

extern "C" int mfcd_shard_collisions(const mfcd_sample *samples, int64_t N, int B, uint8_t *flags_dev, void *stream)
{
    if (N < 0 || B <= 0) return MFCD_EINVAL;
    if (N == 0) return 0;
    if (!samples || !flags_dev) return MFCD_EINVAL;
    const int64_t nsteps = (N + B - 1) / B;
    hipLaunchKernelGGL(shard_collisions_kernel, dim3((unsigned)nsteps), dim3(256), 0, (hipStream_t)stream, samples, N, B,
                       nsteps, flags_dev);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mfcd_shard_pack_ahead(const float *U_shard, const float *V_shard, const float *mU, const float *vU,
                                     const float *mV, const float *vV, const mfcd_sample *next_batch, int Bk, int B,
                                     int64_t step, int d, int u_lo, int u_hi, int v_lo, int v_hi, double lr, double beta1,
                                     double beta2, double eps, double weight_decay, float *xbuf, void *stream)
{
    if (!next_batch || !xbuf || Bk < 0 || B <= 0 || Bk > B || d <= 0 || d > MFCD_MAX_D || u_hi < u_lo || v_hi < v_lo ||
        step < 1)
        return MFCD_EINVAL;
    if ((u_hi > u_lo && (!U_shard || !mU || !vU)) || (v_hi > v_lo && (!V_shard || !mV || !vV))) return MFCD_EINVAL;
    const AdamConst ac = adam_const({lr, beta1, beta2, eps, weight_decay}, step);
    hipLaunchKernelGGL(shard_pack_ahead_kernel<float>, dim3((3 * B + 3) / 4), dim3(256), 0, (hipStream_t)stream, U_shard, V_shard,
                       mU, vU, mV, vV, next_batch, Bk, B, d, u_lo, u_hi - u_lo, v_lo, v_hi - v_lo, ac, xbuf, 0);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mfcd_shard_pack(const float *U_shard, const float *V_shard, const mfcd_sample *batch, int Bk, int B,
                               int d, int u_lo, int u_hi, int v_lo, int v_hi, float *xbuf, void *stream)
{
    if (!batch || !xbuf || Bk < 0 || B <= 0 || Bk > B || d <= 0 || d > MFCD_MAX_D || u_hi < u_lo || v_hi < v_lo)
        return MFCD_EINVAL;
    if ((u_hi > u_lo && !U_shard) || (v_hi > v_lo && !V_shard)) return MFCD_EINVAL;
    hipLaunchKernelGGL(shard_pack_kernel<float>, dim3((3 * B + 3) / 4), dim3(256), 0, (hipStream_t)stream, U_shard, V_shard,
                       batch, Bk, B, d, u_lo, u_hi - u_lo, v_lo, v_hi - v_lo, xbuf, 0);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}

namespace {
template <typename TP>
int shard_apply_t(const AdamTables &t, const mfcd_sample *batch, int Bk, int B, const float *xbuf, int64_t step, int d,
                  const ShardRows &rows, const AdamHyper &h, float *loss_terms, void *stream)
{
    TP *U_shard = (TP *)t.U, *V_shard = (TP *)t.V;
    float *mU = t.mU, *vU = t.vU, *mV = t.mV, *vV = t.vV;
    if (!batch || !xbuf || Bk <= 0 || B <= 0 || Bk > B || d <= 0 || d > MFCD_MAX_D || step < 1) return MFCD_EINVAL;
    const int nu = rows.u_hi - rows.u_lo, nv = rows.v_hi - rows.v_lo;
    if (nu < 0 || nv < 0) return MFCD_EINVAL;
    if (nu + nv == 0) {   // this rank owns no row (world > rows): nothing to update, only the step's loss terms
        if (loss_terms) {
            hipLaunchKernelGGL(shard_terms_kernel, dim3((Bk + 3) / 4), dim3(256), 0, (hipStream_t)stream, xbuf, batch, Bk,
                               B, d, loss_terms);
            MFCD_HIP_TRY(hipGetLastError());
        }
        return 0;
    }
    if ((nu > 0 && (!U_shard || !mU || !vU)) || (nv > 0 && (!V_shard || !mV || !vV))) return MFCD_EINVAL;
    const void *ptrs[] = {U_shard, V_shard, mU, vU, mV, vV, xbuf};
    // an empty table side is legal (a rank may own rows of one table only when world > rows): one dummy row count
    const Plan pl = make_plan(ptrs, 7, nu > 0 ? nu : 0, nv > 0 ? nv : 0, d);
    const AdamConst ac = adam_const(h, step);
    launch_streaming_step<3, TP>(pl, (hipStream_t)stream, U_shard, V_shard, U_shard, V_shard, mU, vU, mV, vV, batch, xbuf,
                                 Bk, 1.0f / (float)Bk, nu, nv, d, ac, loss_terms, nullptr, nullptr, B, rows.u_lo, rows.v_lo);
    MFCD_HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int mfcd_shard_apply(float *U_shard, float *V_shard, float *mU, float *vU, float *mV, float *vV,
                                const mfcd_sample *batch, int Bk, int B, const float *xbuf, int64_t step, int d,
                                int u_lo, int u_hi, int v_lo, int v_hi, double lr, double beta1, double beta2,
                                double eps, double weight_decay, float *loss_terms, void *stream)
{
    return shard_apply_t<float>({U_shard, V_shard, mU, vU, mV, vV}, batch, Bk, B, xbuf, step, d, {u_lo, u_hi, v_lo, v_hi},
                                {lr, beta1, beta2, eps, weight_decay}, loss_terms, stream);
}

namespace {
template <typename TP>   // fp32 or bf16 factor shards; the exchange buffer, the moments and the arithmetic are fp32
int run_shard_train_steps(const DistCall &c)
{
    const AdamTables &t = c.t;
    const mfcd_sample *samples = c.samples;
    const int64_t N = c.N, step0 = c.step0;
    const int B = c.B, rank = c.rank, world = c.world, n = c.n, m = c.m, d = c.d;
    void *workspace = c.workspace, *comm = c.comm, *stream = c.stream;
    if (n <= 0 || m <= 0 || d <= 0 || d > MFCD_MAX_D || N < 0 || B <= 0 || world < 1 || rank < 0 || rank >= world ||
        step0 < 0)
        return MFCD_EINVAL;
    if (N == 0) return 0;
    if (!samples || !workspace || !t.U || !t.V || !t.mU || !t.vU || !t.mV || !t.vV) return MFCD_EINVAL;
    if (c.workspace_bytes < mfcd_shard_workspace_bytes(N, B, d)) return MFCD_EWORKSPACE;
    const mfcd_detail::RcclApi *R = nullptr;
    if (comm) {
        R = &mfcd_detail::rccl();
        if (!R->ok || !R->AllReduce) return MFCD_ERCCL;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t xb = shard_xbuf_bytes(B, d);
    float *xbufs[2] = {(float *)workspace, (float *)((char *)workspace + xb)};
    float *terms = (float *)((char *)workspace + 2 * xb);
    uint8_t *flags_dev = (uint8_t *)((char *)terms + align_up(sizeof(float) * (size_t)N));
    const int64_t nsteps = (N + B - 1) / B;
    // with a communicator the table pointers are this rank's SHARDS; without one they are the FULL tables and this
    // process plays every rank in turn (single-process rehearsal of any world size; exact, the protocol is the same)
    const int r0 = comm ? rank : 0, r1 = comm ? rank + 1 : world;
    struct RankShard : ShardRows { AdamTables t; };   // a rank's rows and where they start
    auto shard_of = [&](int r) {
        RankShard s{{}, t};
        shard_range(n, r, world, &s.u_lo, &s.u_hi);
        shard_range(m, r, world, &s.v_lo, &s.v_hi);
        if (!comm) s.t = t.from<TP>((int64_t)s.u_lo * d, (int64_t)s.v_lo * d);
        return s;
    };
    // rows of batch k as they are NOW into xbuf (after step k-1 has run)
    auto pack_now = [&](int64_t k, float *xbuf) -> int {
        const int64_t off = k * B;
        const int Bk = (int)((N - off) < B ? (N - off) : B);
        for (int r = r0; r < r1; ++r) {
            const RankShard s = shard_of(r);
            hipLaunchKernelGGL(shard_pack_kernel<TP>, dim3((3 * B + 3) / 4), dim3(256), 0, st, (const TP *)s.t.U,
                               (const TP *)s.t.V, samples + off, Bk, B, d, s.u_lo, s.u_hi - s.u_lo, s.v_lo, s.v_hi - s.v_lo,
                               xbuf, (comm || r == r0) ? 0 : 1);
        }
        MFCD_HIP_TRY(hipGetLastError());
        return 0;
    };
    // rows of batch k+1 as they will be after step k, which has not run yet (no row shared with batch k)
    auto pack_ahead = [&](int64_t k, float *xbuf) -> int {
        const int64_t off = (k + 1) * B;
        const int Bk = (int)((N - off) < B ? (N - off) : B);
        const AdamConst ac = adam_const(c.h, step0 + k + 1);
        for (int r = r0; r < r1; ++r) {
            const RankShard s = shard_of(r);
            hipLaunchKernelGGL(shard_pack_ahead_kernel<TP>, dim3((3 * B + 3) / 4), dim3(256), 0, st, (const TP *)s.t.U,
                               (const TP *)s.t.V, (const float *)s.t.mU, (const float *)s.t.vU, (const float *)s.t.mV,
                               (const float *)s.t.vV, samples + off, Bk, B, d, s.u_lo, s.u_hi - s.u_lo, s.v_lo,
                               s.v_hi - s.v_lo, ac, xbuf, (comm || r == r0) ? 0 : 1);
        }
        MFCD_HIP_TRY(hipGetLastError());
        return 0;
    };
    auto apply = [&](int64_t k, const float *xbuf) -> int {
        const int64_t off = k * B;
        const int Bk = (int)((N - off) < B ? (N - off) : B);
        for (int r = r0; r < r1; ++r) {
            const RankShard s = shard_of(r);
            if (int rc = shard_apply_t<TP>(s.t, samples + off, Bk, B, xbuf, step0 + k + 1, d, s, c.h,
                                           r == r0 ? terms + off : nullptr, stream))
                return rc;
        }
        return 0;
    };

    // 1 (default): pipelined where there is a collective to hide (world > 1) and in the comm-less rehearsal; a one-rank
    // communicator takes the strict chain (measured, C4 on a one-rank group: the two stream hops of a pipelined step cost
    // 10 us more than they hide when the collective is a local copy); 2 forces the pipelined chain (tests, timing)
    const int pipe = mfcd_detail::g_tune.shard_pipeline;
    if (pipe == 0 || nsteps < 2 || (pipe == 1 && comm && world == 1)) {
        // the strict chain: pack -> all-reduce -> step, one stream
        for (int64_t k = 0; k < nsteps; ++k) {
            if (int rc = pack_now(k, xbufs[0])) return rc;
            if (comm && R->AllReduce(xbufs[0], xbufs[0], (size_t)3 * B * d, ncclUint32, ncclSum, (ncclComm_t)comm, st) !=
                            ncclSuccess)
                return MFCD_ERCCL;
            if (int rc = apply(k, xbufs[0])) return rc;
        }
    } else {
        // Pipelined exchange: where batch k+1 shares no row with batch k, its rows are packed AHEAD of step k (rolled
        // forward over it) and their all-reduce runs on a side stream underneath step k; only the pairs of batches that
        // do share a row keep the strict chain.  Which pairs those are is a property of the sample stream alone (the
        // same on every rank): one kernel marks them, the host reads the marks once per call (the one host wait of this
        // entry point; the enqueue pattern — hence the collective sequence of every rank — depends on them).
        if (int rc = mfcd_shard_collisions(samples, N, B, flags_dev, stream)) return rc;
        std::vector<uint8_t> collide((size_t)nsteps);
        MFCD_HIP_TRY(hipMemcpyAsync(collide.data(), flags_dev, (size_t)nsteps, hipMemcpyDeviceToHost, st));
        MFCD_HIP_TRY(hipStreamSynchronize(st));
        hipStream_t cs = nullptr;
        hipEvent_t packed[2] = {nullptr, nullptr}, reduced[2] = {nullptr, nullptr};
        int rc = 0;
        auto fail = [&](int code) { if (!rc) rc = code; };
        if (comm) {
            if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return MFCD_EINVAL;
            for (int e = 0; e < 2; ++e) {
                if (hipEventCreateWithFlags(&packed[e], hipEventDisableTiming) != hipSuccess) fail(MFCD_EINVAL);
                if (hipEventCreateWithFlags(&reduced[e], hipEventDisableTiming) != hipSuccess) fail(MFCD_EINVAL);
            }
        }
        // the collective of the buffer just packed on `st`, on the side stream; `st` meets it again at wait_reduced
        auto reduce_async = [&](int b) {
            if (!comm || rc) return;
            if (hipEventRecord(packed[b], st) != hipSuccess || hipStreamWaitEvent(cs, packed[b], 0) != hipSuccess)
                return fail(MFCD_EINVAL);
            if (R->AllReduce(xbufs[b], xbufs[b], (size_t)3 * B * d, ncclUint32, ncclSum, (ncclComm_t)comm, cs) != ncclSuccess)
                return fail(MFCD_ERCCL);
            if (hipEventRecord(reduced[b], cs) != hipSuccess) fail(MFCD_EINVAL);
        };
        auto wait_reduced = [&](int b) {
            if (comm && !rc && hipStreamWaitEvent(st, reduced[b], 0) != hipSuccess) fail(MFCD_EINVAL);
        };
        // a collective on the main stream itself: no overlap wanted, so no stream hops (the first batch, and every
        // batch that shares a row with the one before it: the strict chain, at the strict chain's cost).  Never concurrent
        // with a side-stream collective on the same communicator: `st` has met every earlier one by then, and the next
        // one on the side stream waits for an event recorded on `st` after this call.
        bool on_side[2] = {false, false};
        auto reduce_inline = [&](int b) {
            on_side[b] = false;
            if (!comm || rc) return;
            if (R->AllReduce(xbufs[b], xbufs[b], (size_t)3 * B * d, ncclUint32, ncclSum, (ncclComm_t)comm, st) != ncclSuccess)
                fail(MFCD_ERCCL);
        };
        if (!rc) fail(pack_now(0, xbufs[0]));
        reduce_inline(0);
        for (int64_t k = 0; k < nsteps && !rc; ++k) {
            const int cur = (int)(k & 1), nxt = cur ^ 1;
            const bool more = k + 1 < nsteps, ahead = more && !collide[(size_t)k];
            if (ahead) {                      // batch k+1 goes on the wire before step k runs
                fail(pack_ahead(k, xbufs[nxt]));
                reduce_async(nxt);
                on_side[nxt] = true;
            }
            if (on_side[cur]) wait_reduced(cur);
            if (!rc) fail(apply(k, xbufs[cur]));
            if (more && !ahead) {             // a shared row: batch k+1 is packed from the updated state
                if (!rc) fail(pack_now(k + 1, xbufs[nxt]));
                reduce_inline(nxt);
            }
        }
        if (comm) {
            // every collective was met by `st` (wait_reduced precedes each step), so nothing is pending on the side stream
            for (int e = 0; e < 2; ++e) {
                if (packed[e]) (void)hipEventDestroy(packed[e]);
                if (reduced[e]) (void)hipEventDestroy(reduced[e]);
            }
            (void)hipStreamDestroy(cs);
        }
        if (rc) return rc;
    }
    if (c.loss_per_step) return mfcd_detail::launch_batch_means(terms, nullptr, N, B, c.loss_per_step, st);
    return 0;
}
}  // namespace

extern "C" int mfcd_shard_train_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                                      const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0,
                                      int n, int m, int d, double lr, double beta1, double beta2, double eps,
                                      double weight_decay, float *loss_per_step, void *workspace, size_t workspace_bytes,
                                      void *comm, void *stream)
{
    return run_shard_train_steps<float>(MFCD_DIST_CALL);
}

extern "C" int mfcd_shard_train_steps_bf16(uint16_t *U, uint16_t *V, float *mU, float *vU, float *mV, float *vV,
                                           const mfcd_sample *samples, int64_t N, int B, int rank, int world,
                                           int64_t step0, int n, int m, int d, double lr, double beta1, double beta2,
                                           double eps, double weight_decay, float *loss_per_step, void *workspace,
                                           size_t workspace_bytes, void *comm, void *stream)
{
    return run_shard_train_steps<mfcd_bf16>(MFCD_DIST_CALL);
}