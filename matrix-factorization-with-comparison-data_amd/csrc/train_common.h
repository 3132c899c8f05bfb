// Shared between the forms of the optimiser step: streaming (streaming.hip), resident (resident.hip), local (local.hip),
// big (big.hip), the fused-step entry (train.hip) and the multi-GPU loops (dist.hip).
#pragma once
#include "common.h"

struct AdamStatic {
    float w1;   // 1 - beta1
    float b2;   // beta2
    float w2;   // 1 - beta2
    float eps;
    float wd;
};

// Per-step bias-correction scalars, computed on the host in f64 exactly as Python does in
// torch/optim/adam.py (1 - beta**step, lr / bc1, bc2 ** 0.5) and rounded to fp32 where ATen would.
struct StepScalars {
    float neg_step_size;  // -(lr / (1 - beta1^t))
    float bc2_sqrt;       // sqrt(1 - beta2^t)
    float inv_bc2_sqrt;   // 1 / sqrt(1 - beta2^t), rounded from f64 (used by the fast flavour only)
    float pad;
};

struct AdamConst {
    AdamStatic st;
    StepScalars sc;
};

// One training call's hyper-parameters as the caller passed them, and its six tables (U, V: fp32 or bf16 elements)
struct AdamHyper { double lr, beta1, beta2, eps, wd; };
struct AdamTables {
    void *U, *V;
    float *mU, *vU, *mV, *vV;
    template <typename TP>   // from element uo of the U side and vo of the V side on (shard rehearsal on full tables)
    AdamTables from(int64_t uo, int64_t vo) const { return {(TP *)U + uo, (TP *)V + vo, mU + uo, vU + uo, mV + vo, vV + vo}; }
};

// host-side Adam constants (f64 as Python computes them, rounded where ATen rounds)
inline AdamStatic adam_static(const AdamHyper &h)
{
    AdamStatic a;
    a.w1 = (float)(1.0 - h.beta1);
    a.b2 = (float)h.beta2;
    a.w2 = (float)(1.0 - h.beta2);
    a.eps = (float)h.eps;
    a.wd = (float)h.wd;
    return a;
}

inline StepScalars step_scalars(const AdamHyper &h, int64_t step)
{
    // bias corrections in f64 as Python does (adam.py: 1 - beta**step, lr / bc1, bc2 ** 0.5)
    const double bc1 = 1.0 - pow(h.beta1, (double)step), bc2 = 1.0 - pow(h.beta2, (double)step);
    StepScalars s;
    s.neg_step_size = (float)(-(h.lr / bc1));
    s.bc2_sqrt = (float)sqrt(bc2);
    s.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    s.pad = 0.0f;
    return s;
}

inline AdamConst adam_const(const AdamHyper &h, int64_t step) { return {adam_static(h), step_scalars(h, step)}; }

constexpr size_t kStatusBytes = 256;  // workspace[0..3] = int32 status word (sticky: set by an aborting resident launch)

// the table arguments every training entry point checks first
inline int check_common(const void *U, const void *V, int n, int m, int d)
{
    if (!U || !V || n <= 0 || m <= 0 || d <= 0 || d > MFCD_MAX_D) return MFCD_EINVAL;
    if ((reinterpret_cast<uintptr_t>(U) & 3u) || (reinterpret_cast<uintptr_t>(V) & 3u)) return MFCD_EALIGN;
    return 0;
}

// One element of torch.optim.Adam's single-tensor step (coupled L2).  The operation sequence is pinned
// (explicit fmaf, contraction off) so that every inlined copy rounds identically — the resident kernel relies on
// a rolled-forward copy of a row matching the in-place update bit for bit — and it mirrors ATen's CPU kernels:
//   grad.add(param, alpha=wd)            -> fma(wd, p, g)                    (vec::fmadd)
//   exp_avg.lerp_(grad, 1-b1)            -> fma(1-b1, g - m, m)              (weight < 0.5 branch, vec::fmadd)
//   exp_avg_sq.mul_(b2).addcmul_(g,g,1-b2) -> (v*b2) + ((1-b2)*g)*g          (no fma)
//   denom = sqrt(v)/bc2_sqrt + eps ;  param.addcdiv_(m, denom, -step_size)  -> p + ((-step_size)*m)/denom
__device__ __forceinline__ void adam_update(float &p, float &m1, float &m2, float gsparse, const AdamStatic &ac,
                                            const StepScalars &sc)
{
#pragma clang fp contract(off)
    const float g = __builtin_fmaf(ac.wd, p, gsparse);
    m1 = __builtin_fmaf(ac.w1, g - m1, m1);
    const float v_scaled = m2 * ac.b2;
    const float gg = (ac.w2 * g) * g;
    m2 = v_scaled + gg;
    const float den = sqrtf(m2) / sc.bc2_sqrt + ac.eps;
    const float num = sc.neg_step_size * m1;
    p = p + num / den;
}

// Fast flavour of the same update for the register-resident kernel, where the step is bound by VALU cycles:
// identical op order, but the square root is the hardware v_sqrt_f32 (<= 1 ulp) and the two divisions are a
// reciprocal multiply with one Newton correction of the quotient (q = q0 + (a - b*q0)*r, <= 1 ulp, almost always
// the correctly rounded quotient) instead of the ~52-cycle IEEE expansions.  The update term therefore differs
// from the IEEE flavour by at most a few ulp (~1e-10 absolute per step at lr = 1e-3).
__device__ __forceinline__ float div_newton(float a, float b, float r /* ~ 1/b */)
{
#pragma clang fp contract(off)
    const float q0 = a * r;
    const float e = __builtin_fmaf(-b, q0, a);
    return __builtin_fmaf(e, r, q0);
}

__device__ __forceinline__ void adam_update_fast(float &p, float &m1, float &m2, float gsparse, const AdamStatic &ac,
                                                 const StepScalars &sc)
{
#pragma clang fp contract(off)
    const float g = __builtin_fmaf(ac.wd, p, gsparse);
    m1 = __builtin_fmaf(ac.w1, g - m1, m1);
    const float v_scaled = m2 * ac.b2;
    const float gg = (ac.w2 * g) * g;
    m2 = v_scaled + gg;
    const float sq = __builtin_amdgcn_sqrtf(m2);
    const float den = div_newton(sq, sc.bc2_sqrt, sc.inv_bc2_sqrt) + ac.eps;
    const float num = sc.neg_step_size * m1;
    p = p + div_newton(num, den, __builtin_amdgcn_rcpf(den));
}

// The fast flavour on TWO elements at once with gfx950's packed fp32 instructions (v_pk_fma_f32, v_pk_mul_f32,
// v_pk_add_f32: one issue slot for both halves).  Every packed operation rounds each half exactly like its scalar
// counterpart and the operation sequence is the one above, so the results are bit-identical to two calls of
// adam_update_fast; only the square roots and reciprocals stay scalar.  20 issue slots per pair instead of 36.
typedef float mfcd_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ mfcd_f2 f2_splat(float x) { return (mfcd_f2){x, x}; }
__device__ __forceinline__ mfcd_f2 f2_fma(mfcd_f2 a, mfcd_f2 b, mfcd_f2 c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ mfcd_f2 div_newton2(mfcd_f2 a, mfcd_f2 b, mfcd_f2 r)
{
#pragma clang fp contract(off)
    const mfcd_f2 q0 = a * r;
    const mfcd_f2 e = f2_fma(-b, q0, a);
    return f2_fma(e, r, q0);
}

__device__ __forceinline__ void adam_update_fast2(float &pa, float &pb, float &m1a, float &m1b, float &m2a, float &m2b,
                                                  float ga, float gb, const AdamStatic &ac, const StepScalars &sc)
{
#pragma clang fp contract(off)
    mfcd_f2 p = {pa, pb}, m1 = {m1a, m1b}, m2 = {m2a, m2b};
    const mfcd_f2 g = f2_fma(f2_splat(ac.wd), p, (mfcd_f2){ga, gb});
    m1 = f2_fma(f2_splat(ac.w1), g - m1, m1);
    const mfcd_f2 v_scaled = m2 * f2_splat(ac.b2);
    const mfcd_f2 gg = (f2_splat(ac.w2) * g) * g;
    m2 = v_scaled + gg;
    const mfcd_f2 sq = {__builtin_amdgcn_sqrtf(m2.x), __builtin_amdgcn_sqrtf(m2.y)};
    const mfcd_f2 den = div_newton2(sq, f2_splat(sc.bc2_sqrt), f2_splat(sc.inv_bc2_sqrt)) + f2_splat(ac.eps);
    const mfcd_f2 num = f2_splat(sc.neg_step_size) * m1;
    const mfcd_f2 rc = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    p = p + div_newton2(num, den, rc);
    pa = p.x; pb = p.y; m1a = m1.x; m1b = m1.y; m2a = m2.x; m2b = m2.y;
}

// Q elements of one thread: pairs through the packed form when FAST && PACKED, scalar otherwise.
template <bool FAST, int Q, bool PACKED>
__device__ __forceinline__ void adam_update_q(float (&p)[Q], float (&m1)[Q], float (&m2)[Q], const float (&g)[Q],
                                              const AdamStatic &ac, const StepScalars &sc);

template <bool FAST>
__device__ __forceinline__ void adam_update_t(float &p, float &m1, float &m2, float gsparse, const AdamStatic &ac,
                                              const StepScalars &sc)
{
    if constexpr (FAST) adam_update_fast(p, m1, m2, gsparse, ac, sc);
    else adam_update(p, m1, m2, gsparse, ac, sc);
}

template <bool FAST, int Q, bool PACKED>
__device__ __forceinline__ void adam_update_q(float (&p)[Q], float (&m1)[Q], float (&m2)[Q], const float (&g)[Q],
                                              const AdamStatic &ac, const StepScalars &sc)
{
    if constexpr (FAST && PACKED && Q % 2 == 0) {
#pragma unroll
        for (int q = 0; q < Q; q += 2)
            adam_update_fast2(p[q], p[q + 1], m1[q], m1[q + 1], m2[q], m2[q + 1], g[q], g[q + 1], ac, sc);
    } else {
#pragma unroll
        for (int q = 0; q < Q; ++q) adam_update_t<FAST>(p[q], m1[q], m2[q], g[q], ac, sc);
    }
}

namespace mfcd_detail {

// ---- local form (local.hip): one workgroup, parameters in LDS ----
constexpr int64_t kLocalMaxElems = 8192;   // (n+m)*d: above this one CU's vector ALU is slower than the multi-CU resident form
constexpr size_t kLocalMaxLds = (size_t)160 * 1024;   // one CU's LDS
bool local_applies(int64_t N, int B, int n, int m, int d);
int launch_local_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV, const mfcd_sample *samples,
                       int64_t N, int B, int n, int m, int d, const StepScalars *sc_dev, const AdamStatic &ac,
                       float *loss_terms, int K, hipStream_t st);

// Arguments of one model's local-form launch: the kernel's by-value argument, and one entry of the device-side
// descriptor table of the batched form (one model per workgroup).
struct LocalArgs {
    float *U, *V, *mU, *vU, *mV, *vV;
    const mfcd_sample *samples;
    const StepScalars *sc;   // [K+1] (the last entry is a pad: the kernel reads step k+1's scalars during step k)
    float *loss_terms;       // [N] sigmoid outputs (the batch-mean kernel forms the BCE terms)
    int64_t N;
    int B, n, m, d, K;
    int Tpad, Rpad, Bpad;    // LDS carve-up (elements / rows / batch, each padded to a multiple of 4)
    int lps_shift;           // lanes per sample in phase A = 1 << lps_shift
    AdamStatic ac;
};

// batched local form (mfcd_train_steps_local_multi): QL = local_ql of the largest model; local_multi_fill sets a
// model's LDS carve-up and lane-group width at that QL and returns the dynamic LDS it needs there
int local_ql(int n, int m, int d);
size_t local_multi_fill(LocalArgs &a, int ql);
int launch_local_multi(const LocalArgs *tab_dev, int R, int ql, bool small_batch, size_t lds_bytes, hipStream_t st);
constexpr int kLocalSmallBatch = 1024;   // batches of at most this many records: one staging slot per thread

// one segment of a flat multi-model grid: blocks [blk_begin, next segment's blk_begin) belong to one model
struct MeanSeg {       // batch_mean_kernel (streaming.hip): the per-step batch means of one model
    const float *terms;
    const mfcd_sample *samples;
    float *out;
    int64_t N, blk_begin;
    int B, pad;
};
struct EvalSeg {       // eval_batches_kernel (eval.hip): the validation batches of one model
    const float *U, *V;
    const mfcd_sample *samples;
    float *loss;
    int32_t *correct;
    int64_t N, blk_begin;
    int B, d;
};

// index of the segment block `blk` belongs to (segments sorted by blk_begin, the first one starting at 0)
template <typename Seg>
__device__ __forceinline__ int find_seg(const Seg *segs, int nseg, int64_t blk)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].blk_begin <= blk) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

int launch_eval_multi(const EvalSeg *segs_dev, int nseg, int64_t blocks, int max_B, hipStream_t st);

// ---- streaming form (streaming.hip): one launch of train_step_kernel per optimiser step ----
struct Plan {
    int vec, chunks, E, blocksU, blocksV;
    size_t lds;
};
// ptrs: the arrays the step reads and writes (vec = 4 needs every one of them 16-byte aligned)
Plan make_plan(const void *const *ptrs, int nptrs, int n, int m, int d);

// One train_step_kernel<VEC, CHUNKS, MODE, TP> launch with the plan's instance (MODE: see the kernel).  Instantiated for
// MODE 0 and 3 with fp32 and bf16 tables, 1 and 2 with fp32.  Error checking is the caller's (hipGetLastError).
template <int MODE, typename TP>
void launch_streaming_step(const Plan &pl, hipStream_t st, const TP *Uin, const TP *Vin, TP *Uout, TP *Vout, float *mU,
                           float *vU, float *mV, float *vV, const mfcd_sample *batch, const float *g_in, int Bk,
                           float inv_batch, int n, int m, int d, const AdamConst &ac, float *loss_terms,
                           float *Gu = nullptr, float *Gv = nullptr, int g_stride = 1, int u_off = 0, int v_off = 0);

// batch_mean_kernel: out[k] = mean of the BCE terms of batch k of N samples, k < ceil(N / B); terms[] holds sigmoid
// outputs p when `samples` is set, ready BCE terms otherwise
int launch_batch_means(const float *terms, const mfcd_sample *samples, int64_t N, int B, float *out, hipStream_t st);
// the same over a flat multi-model grid of `blocks` batches (segs_dev: device copy of the segment table)
int launch_batch_means_multi(const MeanSeg *segs_dev, int nseg, int64_t blocks, hipStream_t st);

struct ResidentPlan {
    bool ok;
    int Q, NW, blocks;
    int lookahead;   // 0, 4 or 8: the instantiation the launch uses
    bool fast_math;
    bool bf16;       // bf16 factor tables
    int tshift;      // look-ahead form: log2(steps per chunk of the per-wave event lists)
};

constexpr unsigned kSpinLimitDefault = 1u << 22;  // polls before a wave gives up (~seconds); sets status = 1

// process-wide tuning knobs (mfcd_set_tuning; experiments and tests only, defaults are the measured best)
struct Tuning {
    int lookahead = -1;          // -1 auto (4, or 0 for tiny tables), 0 off, else the window depth 2 .. 16
    unsigned spin_limit = kSpinLimitDefault;   // polls before a wave gives up and sets the status word
    int shard_pipeline = 1;      // row-sharded loop: 1 = exchange of batch k+1 under step k where no row is shared
};
extern Tuning g_tune;

extern int g_resident_math;

int set_uvt_split(int v);    // uvt.hip
int set_uvt_target_wgs(int v);   // uvt.hip
int set_uvt_min_stages(int v);   // uvt.hip

// The resident slice rule, in one place: the slices of Q registers per array (64*Q elements, whole rows) whose wave
// count the chip can hold at the design's waves per CU (16 for Q <= 2, 8 above) and kResidentMaxWaves, in ascending Q.
// Geometry only: no tuning knob, no occupancy query.  The workspace layout asks "any?", the event lists are laid out
// for the first, the plan walks them with the occupancy of the actual code object.
struct ResidentSlices {
    int count;
    struct { int Q, waves; } at[5];
};
ResidentSlices resident_slices(int n, int m, int d, int num_cus);

// ev_tshift: chunk length of the event lists the WORKSPACE was laid out for (ResidentEvents::tshift; 0 = no lists, the
// look-ahead form is then not planned)
ResidentPlan plan_resident(int64_t N, int B, int n, int m, int d, int num_cus, bool bf16 = false, int ev_tshift = -1);
int resident_lookahead(int64_t N, int B, int n, int m);

// Geometry of the per-wave event lists of the look-ahead form (resident_kernel.h) for tables of this shape and batch
// size: a function of the shape alone (the smallest slice that fits, never of a tuning knob), so that a workspace
// planned once serves every call.  tshift = 0: the lists do not apply (a wave would see a hit nearly every step).
struct ResidentEvents {
    int tshift;        // log2(steps per chunk), 4 .. 8
    int waves;         // owner waves the arrays are laid out for
    int rows_per_wave;
};
ResidentEvents resident_events(int B, int n, int m, int d, int num_cus);
constexpr int kResidentEventCap = 64;          // entries per (wave, chunk) list = one per lane (resident_kernel.h)
constexpr int kResidentEventLook = 16;         // deepest look-ahead window: boundary copies per chunk
inline int64_t resident_event_chunks(int64_t K, int tshift) { return (K >> tshift) + 2; }

// stage tables of up to this many bytes travel in the prologue kernel's own argument segment: the host buffer they are
// built in is read at launch time only (no pinned slot, no event)
size_t train_inline_stage_bytes();

// Pointers needed only at a few points of a resident launch.  They live in device memory (workspace, directly in front
// of the call's step scalars) and are (re)read with scalar loads there, so they do not occupy SGPRs during the step loop
// (with them passed by value the kernel needed > 102 SGPRs and spilled scalars into VGPR lanes on every step).
struct ResidentCold {
    float *U, *V, *mU, *vU, *mV, *vV;
    int *status;                     // 0 = ok, 1 = a bounded spin expired (sticky: never cleared by a launch)
    unsigned long long spin_limit;   // polls before a wave gives up
    unsigned *ev_cnt;                // [waves][nch_cap] entries appended to list (wave, chunk); all-zero between launches
                                     // (every wave clears its own counters at the end of a launch)
    uint4 *ev_ent;                   // [waves][nch_cap][kEventCap] entries
    long long nch_cap;               // chunks per wave the two arrays are laid out for
    long long tshift;                // log2(steps per chunk)
    float *loss_out;                 // [K] batch-mean BCE per step, formed inside the launch (look-ahead form); may be null
    unsigned long long pad[3];       // 128 bytes
};
static_assert(sizeof(ResidentCold) == 128, "eight 16-byte units of the stage table (resident.hip: kInlineStageUnits)");

// One kernel in front of a resident / local / multi-model launch: the host-built stage table -> workspace, and (tr
// given, tr->xs set) the translated samples + (tr->look > 0) the per-wave event lists of the resident form.
struct StageCopy {
    const void *host;      // the table as the host built it (read at launch time when it travels in the kernel arguments)
    const void *devview;   // the pinned slot `host` is, as the device addresses it; null: it fits the kernel arguments
    void *dev;
    size_t bytes;
};
struct SampleTranslation {
    const mfcd_sample *samples;
    int64_t N;
    int B, n, m, rows_per_wave, tshift, look;
    int64_t nch_cap;
    mfcd_sample *xs;
    unsigned *ev_cnt;
    void *ev_ent;
};
int launch_train_prologue(const StageCopy &sc, const SampleTranslation *tr, hipStream_t st);

// cold_dev: device copy of the call's ResidentCold; xs: the call's samples translated to virtual row ids
int launch_resident_steps(const ResidentPlan &pl, const void *cold_dev, const mfcd_sample *xs, int64_t N, int B, int n,
                          int m, int d, const StepScalars *sc_dev, const AdamStatic &ac, unsigned long long *mailbox,
                          unsigned tag_base, void *loss_terms, unsigned long long *dbg, int K, hipStream_t st);
constexpr int kResidentMaxWaves = 4096;   // 256 CUs x 16 waves: upper bound of ResidentPlan::NW (workspace sizing)

}  // namespace mfcd_detail
