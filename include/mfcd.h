/*
 * mfcd.h — C-ABI of libmfcd_hip.so: the MI355X (gfx950) hot path of triplet-comparison matrix
 * factorisation.  Plain pointers and sizes only; no torch types.
 *
 * The reference (MayeulCassier/Matrix-Factorization-With-Comparison-Data) is pure Python on
 * PyTorch and has no FFI layer of its own; each entry point below replaces the PyTorch op
 * sequence of the cited reference lines (paths into the reference repository).  The Python
 * binding a maintainer would add is shown in INTEGRATION.md; the in-tree one is
 * matrix-factorization-with-comparison-data_amd/mfcd/_lib.py (ctypes).
 *
 * Conventions
 *  - every pointer except `scalars_host`-style arguments is a DEVICE pointer borrowed from the
 *    caller; the library allocates nothing persistent and frees nothing it did not allocate;
 *  - every entry returns 0 on success, a positive hipError_t, or a negative MFCD_E* code;
 *    mfcd_error_string() renders either;
 *  - all work is enqueued on `stream` (a hipStream_t, may be NULL = default stream); no entry
 *    synchronises the host with the device except where its comment says so (mfcd_train_steps_timed;
 *    the bounded run-ahead of mfcd_train_steps; mfcd_shard_train_steps reads its collision marks once per call;
 *    mfcd_train_steps_big copies its per-step table from the stack);
 *  - factor tables are row-major contiguous fp32: U [n][d], V [m][d];
 *  - a sample is the 16-byte record mfcd_sample {int32 u, i, j; float z} (reference batch tuple
 *    (u, i, j, z), structure.py:527-531, with the label already cast to fp32 as at 849);
 *    0 <= u < n, 0 <= i,j < m are validated by mfcd_check_samples, not by the hot kernels.
 */
#ifndef MFCD_H
#define MFCD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFCD_ABI_VERSION 4

#define MFCD_EINVAL (-1)   /* bad argument (null pointer, non-positive size, d out of range)   */
#define MFCD_EWORKSPACE (-2) /* workspace smaller than mfcd_*_workspace_bytes says             */
#define MFCD_EALIGN (-3)   /* a table pointer is not 4-byte aligned                            */
#define MFCD_EINDEX (-4)   /* a sample indexes outside [0,n) x [0,m)^2 (mfcd_check_samples)     */
#define MFCD_ERCCL (-5)    /* RCCL is not loadable in this process, or an RCCL call failed      */
#define MFCD_ESTATE (-6)   /* the workspace was not initialised (mfcd_train_workspace_init) or was
                              planned for other n, m, d                                         */

#define MFCD_MAX_D 1024

typedef struct mfcd_sample {
    int32_t u, i, j;
    float z;
} mfcd_sample;

int mfcd_abi_version(void);
const char *mfcd_error_string(int code);

/*
 * Validates 0<=u<n, 0<=i<m, 0<=j<m for N samples.  Writes the number of bad records to
 * *bad_count_dev (device int32).  The reference raises IndexError from U[u]/V[i]
 * (structure.py:787-789); the Python host turns a non-zero count into the same exception.
 */
int mfcd_check_samples(const mfcd_sample *samples, int64_t N, int n, int m, int32_t *bad_count_dev,
                       void *stream);

/*
 * Forward + BCE over N samples in consecutive batches of B (last one short), no gradient.
 * Replaces, per batch, model(u,i,j) (structure.py:773-795) + F.binary_cross_entropy(pred,
 * z.float()) (structure.py:864 validation loop, 908 evaluate_model) + (pred > 0.5) == z
 * (structure.py:912-915).
 *   loss_per_batch[k]    fp32 mean BCE of batch k (what loss.item() returns)
 *   correct_per_batch[k] int32 count of matches in batch k            (nullable)
 *   p_out[t]             fp32 sigmoid output per sample               (nullable)
 * Number of batches = ceil(N/B).
 */
int mfcd_eval_batches(const float *U, const float *V, const mfcd_sample *samples, int64_t N, int B,
                      int n, int m, int d, float *loss_per_batch, int32_t *correct_per_batch,
                      float *p_out, void *stream);

/*
 * Workspace of mfcd_train_steps: caller-owned device memory, PLANNED once for a capacity and then reused by every
 * call that fits it (no per-call re-initialisation, no per-call allocation):
 *
 *   bytes = mfcd_train_workspace_bytes(N_cap, B, n, m, d)       N_cap = most samples one call will pass (an epoch)
 *   mfcd_train_workspace_init(ws, bytes, N_cap, B, n, m, d, stream)
 *        once after allocating it (256-byte aligned), and again after a reported abort; zero-fills it on `stream`
 *        and registers the host-side state that belongs to it (pinned staging ring, launch counter).  One workspace
 *        serves one model on one stream and is driven by one host thread at a time; use one per model / stream.
 *   mfcd_train_steps(..., ws, bytes, stream)                    any N <= N_cap with ceil(N/B) <= ceil(N_cap/B_plan),
 *        the same n, m, d; MFCD_ESTATE for an unregistered workspace or other n, m, d, MFCD_EWORKSPACE past the capacity
 *   mfcd_train_workspace_release(ws)                            before freeing it (also releases a workspace
 *        registered by mfcd_multi_workspace_init)
 *
 * The first 4 bytes are an int32 status word: 0 = ok, 1 = a bounded in-kernel wait of the resident form expired
 * (U, V, m, v are then undefined).  It is STICKY: no call clears it, so an abort in any earlier call is still
 * visible when the host finally looks (after the stream has drained); only mfcd_train_workspace_init resets it.
 */
size_t mfcd_train_workspace_bytes(int64_t N_cap, int B, int n, int m, int d);
int mfcd_train_workspace_init(void *workspace, size_t workspace_bytes, int64_t N_cap, int B, int n, int m,
                              int d, void *stream);
int mfcd_train_workspace_release(void *workspace);

/*
 * Which form of the fused step mfcd_train_steps uses (process-wide):
 *   0 auto (default)  local where it applies; else resident where it applies and the call has at least
 *                     3 steps; else streaming
 *   1 streaming       one launch per optimiser step, state streamed through HBM (any size, any d)
 *   2 resident        one persistent launch per call, p/m/v held in registers, rows exchanged through
 *                     tagged 8-byte granules; needs d a power of two <= 256, 12*(n+m)*d bytes of state that
 *                     fit the register files, and every wave of the grid resident at once (asked of the
 *                     runtime's occupancy query per instantiation); MFCD_EINVAL from mfcd_train_steps otherwise
 *   3 local           tiny problems ((n+m)*d <= 8192, B <= 4096, any d): one persistent launch of ONE
 *                     workgroup, parameters in LDS, moments in registers, workgroup barriers only;
 *                     1.2-5.7x faster than the resident form wherever it applies; MFCD_EINVAL otherwise
 * All forms compute the same step (same summation order per row); results agree to fp32 rounding.
 */
int mfcd_set_train_path(int mode);

/*
 * Arithmetic flavour of Adam inside the RESIDENT and LOCAL forms, where the step is bound by vector-ALU cycles
 * (process-wide; the streaming form is HBM-bound and always uses the IEEE flavour):
 *   1 fast (default)  same operation order, but sqrt is the hardware v_sqrt_f32 (<= 1 ulp) and the two
 *                     divisions are reciprocal-multiply with one Newton correction (<= 1 ulp) instead of
 *                     the IEEE-rounded expansions; the update differs by a few ulp (~1e-10 per step)
 *   0 ieee            every operation IEEE-rounded, as ATen's CPU kernels
 * Either flavour is deterministic and keeps every parity test within the stated tolerances.
 */
int mfcd_set_resident_math(int fast);

/*
 * Tuning knobs for experiments and tests (process-wide; the defaults are the measured best and what every
 * published number uses).  They replace the environment variables the round-1 build read on every launch.
 * Keys 1, 2, 4, 6, 7, 8 and 12 are retired and not reused: like any unknown key they return MFCD_EINVAL.
 */
#define MFCD_TUNE_RESIDENT_LOOKAHEAD 3  /* -1 auto (default: 4), 0 off, 2 .. 16 = depth of the window in steps */
#define MFCD_TUNE_RESIDENT_SPIN_LIMIT 5 /* polls before a wave gives up; 0 = default (2^22)                    */
#define MFCD_TUNE_UVT_TARGET_WGS 9      /* UV^T pass: workgroups the column split aims for (default 512)       */
#define MFCD_TUNE_UVT_SPLIT 11          /* UV^T pass, d in {32, 64, 128, 256}: 1 (default) = bf16x3 split product on the bf16 matrix pipe, 0 = fp32 MFMA */
#define MFCD_TUNE_SHARD_PIPELINE 13     /* row-sharded native loop: 1 (default) = exchange of batch k+1 under step k when world > 1, 2 = always, 0 = strict chain */
#define MFCD_TUNE_UVT_MIN_STAGES 10     /* UV^T pass: column stages a workgroup sweeps at least (default 8)    */
int mfcd_set_tuning(int key, int64_t value);

/*
 * What mfcd_train_steps would do for a call of these sizes under the current settings (no launch; for
 * benchmarks and logs, so that they do not re-derive the plan).
 */
typedef struct mfcd_train_plan {
    int32_t form;                 /* 1 streaming, 2 resident, 3 local */
    int32_t resident_q;           /* registers per array and lane (slice = 64*q elements)        */
    int32_t resident_waves;       /* owner waves = slices                                         */
    int32_t resident_blocks;      /* workgroups of 4 waves                                        */
    int32_t resident_lookahead;   /* 0, 4 or 8                                                    */
    int32_t fast_math;            /* resident / local: Adam flavour                               */
    int32_t streaming_vec;        /* floats per lane and access (4 unless d % 4 != 0)             */
    int32_t streaming_chunks;
    int32_t streaming_blocks;     /* workgroups per step launch                                   */
    int32_t device_cus;
    int32_t reserved[6];
} mfcd_train_plan;
int mfcd_train_plan_query(int64_t N, int B, int n, int m, int d, int bf16_factors, mfcd_train_plan *out);

/*
 * Runs ceil(N/B) sequential optimiser steps on the device, consuming `samples` in order in
 * batches of B (last one short, divisor = actual batch size).  One step replaces
 * structure.py:847-851: zero_grad, forward, BCE(mean), backward (gather + scatter-add of row
 * gradients into U and V) and torch.optim.Adam.step() (coupled L2 weight decay, bias-corrected,
 * dense over every row; torch/optim/adam.py _single_tensor_adam).
 *   U,V,mU,vU,mV,vV  parameters and Adam moments (exp_avg, exp_avg_sq), updated in place
 *   step0            optimiser steps already taken (Adam's `step` before this call)
 *   loss_per_step[k] fp32 batch-mean BCE of step k (structure.py:852 loss.item())
 * No dense gradient is materialised.  The host is never made to wait for the device, with one bound: a workspace's
 * fifth queued call waits until its first has started (the pinned staging ring of per-step scalars has four slots).
 */
int mfcd_train_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                     const mfcd_sample *samples, int64_t N, int B, int64_t step0, int n, int m,
                     int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                     float *loss_per_step, void *workspace, size_t workspace_bytes, void *stream);

/*
 * bf16 factor storage (BASELINE.json configs[2]; the reference has no such mode, the rounding points are defined
 * here and in oracle/mfcd_oracle.c): U [n][d], V [m][d] are bf16 in HBM; each step reads them as such, does all
 * arithmetic and keeps the Adam moments in fp32, and rounds the updated parameters to the nearest bf16 (ties to
 * even) once, when they are written back.  Streaming form (20 bytes per element per step instead of 24) or, where
 * it applies, the resident form: the register copy is rounded after every update, the same
 * rounding point, so both forms agree with the oracle's definition.
 */
int mfcd_train_steps_bf16(uint16_t *U, uint16_t *V, float *mU, float *vU, float *mV, float *vV,
                          const mfcd_sample *samples, int64_t N, int B, int64_t step0, int n, int m,
                          int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                          float *loss_per_step, void *workspace, size_t workspace_bytes, void *stream);
int mfcd_eval_batches_bf16(const uint16_t *U, const uint16_t *V, const mfcd_sample *samples, int64_t N,
                           int B, int n, int m, int d, float *loss_per_batch,
                           int32_t *correct_per_batch, float *p_out, void *stream);

/*
 * Diagnostic twin of mfcd_train_steps for bench.py's roofline figure: identical work, but every step
 * launch is bracketed by its own pair of HIP events on `stream`, and the call WAITS for the last one.
 * kernel_us_host[3] (HOST memory) receives the average / min / max step-kernel duration in microseconds.
 * Not for the training loop (it synchronises and the events perturb launch pacing).
 */
int mfcd_train_steps_timed(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                           const mfcd_sample *samples, int64_t N, int B, int64_t step0, int n, int m,
                           int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                           float *loss_per_step, void *workspace, size_t workspace_bytes, void *stream,
                           float *kernel_us_host);

/*
 * Prepared calls: everything about a training call that does not change from call to call — the six table pointers,
 * the table shape and dtype, the batch size, the Adam hyper-parameters and the planned workspace — bound ONCE into a
 * handle, so that the per-call boundary is five scalars (round-2 review: a 20-step call spent ~24 us of its ~50 us in
 * argument marshalling on the host side of the boundary).  mfcd_train_call_run(handle, ...) is mfcd_train_steps /
 * mfcd_train_steps_bf16 with the bound arguments: same forms, same results, same stream semantics.  The handle borrows
 * the pointers (nothing is copied or owned); release it before the tables, the moments or the workspace go away, and
 * prepare a new one when any bound value changes (a learning-rate schedule, a re-planned workspace).
 * Replaces, on the reference side, the per-epoch body of train_model (structure.py:845-852).
 */
int mfcd_train_call_prepare(void *U, void *V, float *mU, float *vU, float *mV, float *vV, int bf16_factors, int B,
                            int n, int m, int d, double lr, double beta1, double beta2, double eps,
                            double weight_decay, void *workspace, size_t workspace_bytes, void **handle_out);
int mfcd_train_call_run(void *handle, const mfcd_sample *samples, int64_t N, int64_t step0, float *loss_per_step,
                        void *stream);
/*
 * Stage a LATER call of the same handle: run its prologue (stage table, sample translation, per-wave event lists of the
 * resident form) NOW on `side_stream`, into the workspace's second set of prologue regions, so that it overlaps the step
 * kernel of the call that is running.  The matching mfcd_train_call_run (same samples, N, step0, loss_per_step) then
 * launches its step kernel only.  The CALLER orders the streams: `side_stream` must not start this before the launch
 * two calls back has finished (it used the same set), and the main stream must wait for `side_stream` before the
 * matching run.  A no-op (returns 0) for calls that would not take the resident look-ahead form; a staged prologue that
 * is never run is simply overwritten by the next one.
 */
int mfcd_train_call_stage(void *handle, const mfcd_sample *samples, int64_t N, int64_t step0, float *loss_per_step,
                          void *side_stream);
int mfcd_train_call_release(void *handle);

/*
 * Batched local form: R independent fp32 models trained in ONE launch, one workgroup (one CU) per model, each
 * running the local form's per-workgroup code unchanged (mfcd_set_train_path mode 3) on its own tables, records,
 * batch size, hyper-parameters and Adam step count.  Every model's results (loss_per_step, U, V, the moments) are
 * bit-identical to what mfcd_train_steps gives for that model on its own.  Workgroups never wait on each other, so R
 * may exceed the number of CUs (the hardware queues the rest).  Replaces, for a repetition / parameter scan of the
 * reference (structure.py:352-387, 413-450), R consecutive calls of the per-epoch body of train_model (845-852).
 *
 * mfcd_local_model: one model's call, HOST memory; 136 bytes (mfcd_local_model_bytes() reports the size the library
 * was built with).  The fields mean what the arguments of mfcd_train_steps of the same names mean; loss_per_step
 * ([ceil(N/B)] fp32, device) is required.  The tables of different models must not overlap.
 */
typedef struct mfcd_local_model {
    float *U, *V, *mU, *vU, *mV, *vV;    /* device; parameters and Adam moments, updated in place              */
    const mfcd_sample *samples;          /* device; N records consumed in order, batches of B (last one short) */
    int64_t N;                           /* >= 1                                                               */
    int64_t step0;                       /* Adam steps already taken                                           */
    int32_t B, n, m, d;
    double lr, beta1, beta2, eps, weight_decay;
    float *loss_per_step;                /* device; [ceil(N/B)] batch-mean BCE per step                       */
} mfcd_local_model;
size_t mfcd_local_model_bytes(void);

/*
 * Workspace of the multi-model entries: caller-owned device memory (256-byte aligned) of
 *   mfcd_train_local_multi_workspace_bytes(models, R, &stage)   training: descriptors, per-step scalars, loss terms
 *   mfcd_eval_multi_workspace_bytes(R, &stage)                 validation: descriptors
 * bytes (0 = bad sizes), registered once with mfcd_multi_workspace_init(ws, bytes, stage), which reserves the pinned
 * staging ring (four slots of `stage` bytes) the descriptors travel through; release it with
 * mfcd_train_workspace_release(ws).  A workspace planned for one set of models serves every later call whose own
 * query is no larger (the epochs of a run: only step0 and the records move).  One workspace per stream, driven by one
 * host thread at a time; calls on it are stream-ordered, so a training call and a validation call need one each.
 */
size_t mfcd_train_local_multi_workspace_bytes(const mfcd_local_model *models, int R, size_t *stage_bytes_out);
size_t mfcd_eval_multi_workspace_bytes(int R, size_t *stage_bytes_out);
int mfcd_multi_workspace_init(void *workspace, size_t workspace_bytes, size_t stage_bytes);

/*
 * Runs ceil(N_r/B_r) optimiser steps for each of the R models of `models` (host array): one prologue kernel copies the
 * descriptors and the per-step bias-correction scalars (built by the same host code as mfcd_train_steps') from the
 * pinned ring to the workspace, one launch of R workgroups trains the models, one launch over the flat (model, step)
 * grid forms every model's batch means.  MFCD_EINVAL, with nothing launched and no table touched, if ANY model is one
 * mfcd_train_steps would not put on the local form under the current mfcd_set_train_path (auto or local; fp32
 * tables, (n+m)*d <= 8192, the batch fits the lane groups and the LDS); MFCD_ESTATE for a workspace not registered
 * by mfcd_multi_workspace_init, MFCD_EWORKSPACE for one smaller than the query says.  The Adam flavour is
 * mfcd_set_resident_math's.  No host synchronisation and no allocation per call, with the bound of mfcd_train_steps:
 * a workspace's fifth queued call waits until its first has started.
 */
int mfcd_train_steps_local_multi(const mfcd_local_model *models, int R, void *workspace, size_t workspace_bytes,
                                 void *stream);

/*
 * mfcd_eval_batches over R models at once (fp32 tables): one launch, one workgroup per (model, batch), the same
 * per-workgroup code, so loss_per_batch / correct_per_batch equal mfcd_eval_batches' for each model bit for bit.
 * mfcd_eval_model: one model's pass, HOST memory; 64 bytes (mfcd_eval_model_bytes()); correct_per_batch is
 * nullable, a model with N = 0 has no batch.  Replaces the validation loop of train_model (structure.py:858-868) of
 * R experiments.  Same workspace rules and error codes as the training entry above.
 */
typedef struct mfcd_eval_model {
    const float *U, *V;                  /* device; U [n][d], V [m][d]                                          */
    const mfcd_sample *samples;          /* device; N records in batches of B (last one short)                 */
    int64_t N;
    int32_t B, n, m, d;                  /* 1 <= B <= 16384, 1 <= d <= MFCD_MAX_D                               */
    float *loss_per_batch;               /* device; [ceil(N/B)] mean BCE per batch                             */
    int32_t *correct_per_batch;          /* device; [ceil(N/B)] matches per batch, nullable                    */
} mfcd_eval_model;
size_t mfcd_eval_model_bytes(void);
int mfcd_eval_batches_multi(const mfcd_eval_model *models, int R, void *workspace, size_t workspace_bytes,
                            void *stream);

/*
 * Split form for data-parallel training (one exchange step between the two calls):
 * mfcd_batch_coefficients computes, for B samples of ONE batch, the sigmoid output, the BCE
 * term and the backward coefficient g_t = dL/dx_t with divisor `batch_divisor` (the GLOBAL
 * batch size), i.e. structure.py:848-850 up to the scalar per sample.
 */
int mfcd_batch_coefficients(const float *U, const float *V, const mfcd_sample *samples, int B,
                            int n, int m, int d, int batch_divisor, float *g_out, float *term_out,
                            float *p_out, void *stream);

/*
 * One dense Adam step given per-sample coefficients for a (global) batch of B samples:
 * applies  dU[u]+=g(V[i]-V[j]), dV[i]+=gU[u], dV[j]-=gU[u]  in batch order on top of the
 * weight-decay gradient and updates U,V,m,v in place (structure.py:850-851).
 * `step` is Adam's 1-based step number.  workspace: mfcd_train_workspace_bytes(B,B,n,m,d) bytes of scratch
 * (no initialisation needed: this entry keeps no state in it).
 */
int mfcd_apply_step(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                    const mfcd_sample *samples, const float *g, int B, int64_t step, int n, int m,
                    int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Data-parallel form with the dense exchange the north star names (RCCL all-reduce of the factor
 * gradients): mfcd_dense_grad overwrites gradU [n][d], gradV [m][d] with THIS rank's share of the batch
 * gradient (structure.py:848-850; divisor = the GLOBAL batch size; rows no local sample touches are 0);
 * term_out[t] (nullable) receives the BCE term of local sample t.  After the caller has summed the
 * buffers over ranks, mfcd_adam_dense applies torch.optim.Adam's step (structure.py:851) from them.
 */
int mfcd_dense_grad(const float *U, const float *V, const mfcd_sample *samples, int B, int n, int m,
                    int d, int batch_divisor, float *gradU, float *gradV, float *term_out,
                    void *stream);
/*
 * Backward of the model's forward for ANY loss on its output (autograd support of MatrixFactorization.forward,
 * structure.py:773-795): g[t] = dLoss/dx_t for B samples (x_t = the pre-sigmoid score); overwrites gradU [n][d],
 * gradV [m][d] with  dU[u]+=g(V[i]-V[j]), dV[i]+=g U[u], dV[j]-=g U[u]  accumulated in batch order (what
 * autograd's index_put_(accumulate=True) builds); rows no sample touches are 0.
 */
int mfcd_dense_grad_from_coefficients(const float *U, const float *V, const mfcd_sample *samples,
                                      const float *g, int B, int n, int m, int d, float *gradU,
                                      float *gradV, void *stream);
int mfcd_adam_dense(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                    const float *gradU, const float *gradV, int64_t step, int n, int m, int d,
                    double lr, double beta1, double beta2, double eps, double weight_decay,
                    void *stream);

/*
 * Data-parallel training loop, native (one process per GPU; RCCL is bound at run time, the library has no link-time
 * dependency on it).  Sharding as SURVEY section 8e: a GLOBAL batch of B*world samples per optimiser step, rank r owns
 * the contiguous slice [r*B, (r+1)*B) of it, the divisor of the mean is the global batch size, every rank applies the
 * same gathered quantities in the same order, so replicas stay bit-identical and the run equals the single-GPU run
 * with batch_size = B*world (structure.py:840-852 with a larger DataLoader batch).  Per step: one coefficient
 * kernel over the rank's shard, ONE in-place ncclAllGather of B {g_t, BCE term_t} float pairs per rank, one fused
 * step kernel over the global batch; everything is enqueued on `stream`, nothing synchronises the host.
 *
 *   mfcd_dp_unique_id      rank 0: fills a 128-byte ncclUniqueId, which the caller distributes to the other ranks
 *   mfcd_dp_comm_create    every rank (current HIP device): ncclCommInitRank -> opaque communicator handle
 *   mfcd_dp_comm_destroy
 *   mfcd_dp_train_steps    `samples` is the GLOBAL stream of N samples (identical on every rank);
 *                          loss_per_step[k] = mean BCE of global batch k (identical on every rank);
 *                          comm == NULL: no collective is issued and this process computes every rank's shard
 *                          itself (exact, because replicas are identical): single-process rehearsal of any world
 *                          size, and the whole of the work when world == 1.
 */
int mfcd_dp_unique_id(void *id_out, size_t id_bytes);
int mfcd_dp_comm_create(const void *id, size_t id_bytes, int rank, int world, void **comm_out);
int mfcd_dp_comm_destroy(void *comm);
size_t mfcd_dp_workspace_bytes(int64_t N, int B, int world, int n, int m, int d);
int mfcd_dp_train_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                        const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0, int n,
                        int m, int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                        float *loss_per_step, void *workspace, size_t workspace_bytes, void *comm, void *stream);
/* the same loop over bf16 factor tables (BASELINE configs[2]; moments, wire format and arithmetic stay fp32; equals
 * mfcd_train_steps_bf16's streaming form with batch_size = B * world) */
int mfcd_dp_train_steps_bf16(uint16_t *U, uint16_t *V, float *mU, float *vU, float *mV, float *vV,
                        const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0, int n,
                        int m, int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                        float *loss_per_step, void *workspace, size_t workspace_bytes, void *comm, void *stream);

/*
 * Row-sharded training: STRONG scaling with the reference's batch size (structure.py:668, B = 64), results equal to
 * the single-GPU run.  Rank r of `world` holds rows [lo_r, hi_r) = mfcd_shard_rows(rows, r, world) of U and of V and of
 * their Adam moments (1/world of the state and of the dense Adam sweep); every rank sees the same sample stream.
 * Per optimiser step: the ranks write the rows of the batch they own into an exchange buffer xbuf[3][B][d] (role u, i,
 * j; zeros elsewhere), ONE all-reduce(sum) of that buffer taken as 32-bit integers reproduces every row bit for bit
 * (exactly one rank contributes non-zero bits per row), then the fused step runs over the shard in place, reading the
 * samples' rows from the buffer.  Every rank forms every sample's BCE term, so the step losses need no collective.
 * The arithmetic per element is that of mfcd_train_steps' streaming form: results are bit-identical to it.
 *
 *   mfcd_shard_pack / mfcd_shard_apply   the two halves of a step, for a caller that owns the collective
 *                                        (mfcd/dist.py over torch.distributed: RCCL, or gloo in the CPU tests)
 *   mfcd_shard_train_steps               the native loop (RCCL bound at run time, communicator from
 *                                        mfcd_dp_comm_create); table pointers are the rank's SHARDS.
 *                                        comm == NULL: the pointers are the FULL tables and this process plays every
 *                                        rank in turn (single-process rehearsal of any world size).
 *   mfcd_shard_pack_ahead                PIPELINED exchange (round 3): the rows of the NEXT batch as they will be
 *                                        after the step `step` that has not run yet — a row the current batch does
 *                                        not name changes in that step by the dense update with a zero sparse
 *                                        gradient, a pure function of its (p, m, v), computed here with the step
 *                                        kernel's own arithmetic (bit-identical) — so the all-reduce of batch k+1 can
 *                                        run underneath step k.  Only legal when no row of the next batch is named
 *                                        by the current one:
 *   mfcd_shard_collisions                flags[k] (uint8, device) = 1 when batch k+1 shares a row with batch k.
 * mfcd_shard_train_steps takes the pipelined chain by default when world > 1 (MFCD_TUNE_SHARD_PIPELINE 0 restores
 * pack -> all-reduce -> step on one stream everywhere, 2 pipelines on a one-rank communicator too): the collectives of
 * free pairs on a side stream, two exchange buffers, the strict chain — on the main stream, no stream hops — across
 * colliding pairs; it reads the collision flags on the host once per call (its one host wait).  Results are
 * bit-identical in both chains.
 * xbuf / workspace: mfcd_shard_workspace_bytes(N, B, d) bytes (the buffers come first, 3*B*d floats each).
 * u_lo..v_hi are GLOBAL row bounds of the shard; batch records name global rows.
 */
int mfcd_shard_rows(int rows, int rank, int world, int *lo, int *hi);
size_t mfcd_shard_workspace_bytes(int64_t N, int B, int d);
int mfcd_shard_pack(const float *U_shard, const float *V_shard, const mfcd_sample *batch, int Bk, int B, int d,
                    int u_lo, int u_hi, int v_lo, int v_hi, float *xbuf, void *stream);
int mfcd_shard_apply(float *U_shard, float *V_shard, float *mU, float *vU, float *mV, float *vV,
                     const mfcd_sample *batch, int Bk, int B, const float *xbuf, int64_t step, int d, int u_lo,
                     int u_hi, int v_lo, int v_hi, double lr, double beta1, double beta2, double eps,
                     double weight_decay, float *loss_terms, void *stream);
int mfcd_shard_collisions(const mfcd_sample *samples, int64_t N, int B, uint8_t *flags_dev, void *stream);
int mfcd_shard_pack_ahead(const float *U_shard, const float *V_shard, const float *mU, const float *vU,
                          const float *mV, const float *vV, const mfcd_sample *next_batch, int Bk, int B, int64_t step,
                          int d, int u_lo, int u_hi, int v_lo, int v_hi, double lr, double beta1, double beta2,
                          double eps, double weight_decay, float *xbuf, void *stream);
int mfcd_shard_train_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                           const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0, int n,
                           int m, int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                           float *loss_per_step, void *workspace, size_t workspace_bytes, void *comm, void *stream);
/* the native loop over bf16 factor shards (exchange buffer, moments and arithmetic stay fp32; bit-identical to
 * mfcd_train_steps_bf16's streaming form with the same batch size) */
int mfcd_shard_train_steps_bf16(uint16_t *U, uint16_t *V, float *mU, float *vU, float *mV, float *vV,
                           const mfcd_sample *samples, int64_t N, int B, int rank, int world, int64_t step0, int n,
                           int m, int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                           float *loss_per_step, void *workspace, size_t workspace_bytes, void *comm, void *stream);

/*
 * Dense UV^T pass against X [n][m] fp32 without materialising UV^T (MFMA fp32 tiles, fused
 * epilogue).  Replaces the GEMM + reductions of compute_reconstruction_error
 * (structure.py:940-952) and of compute_alpha_and_norm_ratios (structure.py:982-996, 1003-1009,
 * 1038-1064):
 *   row_stats [n][8] f64, with a = (UV^T)[r][.] - rowmean(UV^T)[r], c = X[r][.] - rowmean(X)[r]:
 *       [0] sum a*c   [1] sum a*a   [2] sum c*c   [3] rowmean(UV^T)[r]   [4] rowmean(X)[r]
 *       [5] sum x*x   [6],[7] reserved (0)
 *   scal [4] f64: [0] ||(UV^T - colmean) - sX||_F^2   [1] ||sX||_F^2   [2],[3] reserved
 * workspace: mfcd_uvt_workspace_bytes(n,m,d).
 */
size_t mfcd_uvt_workspace_bytes(int n, int m, int d);
int mfcd_uvt_stats(const float *U, const float *V, const float *X, int n, int m, int d, double s,
                   double *row_stats, double *scal, void *workspace, size_t workspace_bytes,
                   void *stream);
/*
 * The same pass computing only what the caller reads: what = 1 the per-row sums (compute_alpha_and_norm_ratios,
 * structure.py:982-1064; `scal` may be NULL), what = 2 the global sums (compute_reconstruction_error,
 * structure.py:940-952; `row_stats` may be NULL), what = 3 both (= mfcd_uvt_stats).  The epilogue's vector work shares
 * its lanes with the fp32 MFMA, so the narrower passes are faster (7 / 4 / 10 packed operations per pair of outputs).
 */
int mfcd_uvt_stats_select(const float *U, const float *V, const float *X, int n, int m, int d, double s,
                          int what, double *row_stats, double *scal, void *workspace,
                          size_t workspace_bytes, void *stream);

/*
 * The pass in row SLABS, for a ground truth kept as factors (X = A B^T at BASELINE C4 / C5 size would be 16 / 7.5 GiB;
 * SURVEY 8f N3): the caller forms rows [row0, row0 + nrows) of X with a plain library GEMM into X_slab [nrows][m] and
 * calls this once per slab.  U, V are the FULL tables (the column centring of U V^T needs every row of U);
 * row_stats_slab [nrows][8] are final for those rows; scal_slab [4] holds this slab's SHARE of the two global sums —
 * the caller adds the shares (f64, slab order) to get what mfcd_uvt_stats returns.
 * workspace: mfcd_uvt_slab_workspace_bytes(n, m, d, nrows) for the largest nrows used.
 */
size_t mfcd_uvt_slab_workspace_bytes(int n, int m, int d, int nrows);
int mfcd_uvt_stats_slab(const float *U, const float *V, const float *X_slab, int n, int m, int d, double s,
                        int what, int row0, int nrows, double *row_stats_slab, double *scal_slab,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * k rows of UV^T: out[r][c] = sum_k U[row_ids[r]][k] * V[c][k]   (structure.py:389-392 computes
 * the full product to read two rows).  row_ids is a device array; a row id outside [0, n) yields a row of NaN
 * (the Python host validates the ids and raises IndexError, as U[row] would).
 */
int mfcd_uvt_rows(const float *U, const float *V, const int32_t *row_ids, int k, int n, int m,
                  int d, float *out, void *stream);

/*
 * BTL label generation on the device (replaces BTLPreferenceDataset._generate_labels,
 * structure.py:493-519, and the host-side packing of the records): for each of T triplets (int32 u, i, j)
 * score = sigmoid(scale * (X[u][i] - X[u][j])) in fp32, K Bernoulli(score) draws, and
 *   soft == 0: K consecutive mfcd_sample records per triplet with labels 0/1 (out holds T*K records)
 *   soft != 0: one record per triplet with z = mean of the K draws       (out holds T records)
 * X is dense [n][m] fp32, or NULL with the factors A [n][dx], B [m][dx] of X = A B^T given instead (C4/C5 sizes).
 * Randomness: Philox4x32-10 keyed by `seed`, counter = (triplet index, draw group): reproducible for a seed,
 * independent of launch geometry; NOT the reference's CPU generator stream (distributional parity only).
 * Indices are not validated here (mfcd_check_samples on the output does that).
 */
int mfcd_generate_labels(const int32_t *triplets, int64_t T, const float *X, int n, int m, const float *A,
                         const float *B, int dx, double scale, int K, int soft, uint64_t seed,
                         mfcd_sample *out, void *stream);

/*
 * Per-row Spearman rank correlation: rho[r] = Pearson correlation of the average ranks
 * (scipy.stats.rankdata semantics: ties share the mean of their positions; -0.0 ties with +0.0) of row r of A
 * [rows][lda] and row r of X [rows][ldx], m <= mfcd_spearman_max_columns() (20448: BASELINE configs[4]'s 20000 fits) columns each.  Replaces the
 * reference's Python loop of scipy.stats.spearmanr over the rows of the centred U V^T and X (structure.py:1023-1031);
 * the caller forms the rows of U V^T with a plain library GEMM.  One workgroup per row: bitonic sort in LDS, exact
 * integer sums of the doubled centred ranks, rho in f64 (NaN for a constant row, as scipy).  Deterministic.
 */
int mfcd_spearman_max_columns(void);
int mfcd_spearman_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m,
                       double *rho, void *stream);
/*
 * The same for rows of ANY length (BASELINE configs[3]: m = 65536 items do not fit a workgroup's LDS): blocks of rows
 * are sorted in global memory by one device-wide segmented radix sort of (key, column) pairs per matrix, then one
 * workgroup per row forms the run-averaged ranks and the exact integer sums as above (bit-identical to
 * mfcd_spearman_rows where both apply).  workspace: mfcd_spearman_long_workspace_bytes(rows, m) bytes (28 bytes per
 * element of a row block of about 256 MiB; 0 = sizes out of range).
 */
size_t mfcd_spearman_long_workspace_bytes(int rows, int m);
int mfcd_spearman_rows_long(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m, double *rho,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Triplet sampling on the device (replaces the per-attempt rejection loops of generation_data.py:16-224
 * — choose_items_random 16-26, _by_proximity 29-43, _by_margin 46-84, _by_variance 87-99, _by_popularity 103-128,
 * _by_svd_projection 164-174 (the draw loop), _top_k 205-219).  One call evaluates `attempts` attempts
 * [attempt0, attempt0 + attempts) of the law and keeps what the reference's loop keeps: the first `want` triplets, in
 * attempt order, that pass the law's filter, are not among `barred_keys` and were not produced by an earlier attempt.
 * A triplet's key is (u * m + i) * m + j (int64); barred_keys holds the caller's `exclude` set plus the keys returned
 * by earlier calls of the same request, in any order.
 *
 *   law        MFCD_LAW_UNIFORM   u ~ U[0,n), i, j ~ U[0,m)                         (random; margin with use_margin)
 *              MFCD_LAW_ITEM_CDF  i, j from the item law whose cumulative sums are cdf[m] (f64, cdf[m-1] == 1):
 *                                 pair_rule 0 = numpy choice(m, size=2, replace=False, p) (popularity),
 *                                 pair_rule 1 = sequential draw without replacement (torch.multinomial; variance)
 *              MFCD_LAW_LISTS     i = list_i[u * list_row_stride + U[0,k)], j likewise from list_j; pair_rule 1 makes
 *                                 the two positions distinct (top_k, svd); list_row_stride = k for per-user tables
 *                                 (proximity, top_k), 0 for one list shared by all users (svd)
 *              MFCD_LAW_GROUPS    (g1, g2) a uniform ordered pair of distinct groups among k >= 2, i uniform in group
 *                                 g1, j uniform in group g2 (cluster, generation_data.py:241-243).  The struct's fields
 *                                 are reused: list_i = the list_row_stride item ids grouped (ascending inside a group),
 *                                 list_j = k + 1 ascending int32 offsets into it, k = the number of groups.  The
 *                                 caller validates the tables (mfcd/sampling.py: group_tables); on the device a group
 *                                 of length <= 0, a position outside [0, list_row_stride) or an item id outside [0, m)
 *                                 rejects the attempt and nothing is read outside the tables.  Uses a third Philox
 *                                 draw group; the draws of the other laws are unchanged by it.
 *   users      NULL (u over all n users) or n_users user ids to draw u from (svd: the top users)
 *   use_margin keep only |X[u][i] - X[u][j]| <= margin (fp32 difference, as generation_data.py:72-73); X dense
 *              [n][m] fp32, or NULL with the factors A [n][dx], B [m][dx] of X = A B^T
 * Attempts with i == j are rejected in every law.  Outputs (device): triplets_out [want][3] int32 and keys_out [want]
 * in attempt order; counts_out[0] = triplets written (<= want), counts_out[1] = attempts consumed (the attempt that
 * completed the request + 1, or `attempts`).  Randomness: Philox4x32-10 keyed by `seed`, counter = (attempt index, draw
 * group): reproducible, independent of launch geometry and of how a request is cut into calls; NOT the reference's
 * generator streams — distributional parity (the seeded host forms in generation_data.py replay those).
 * attempts + n_barred < 2^32 - 1.  workspace: mfcd_sample_workspace_bytes(attempts, n_barred) bytes (0 = bad sizes).
 */
#define MFCD_LAW_UNIFORM 0
#define MFCD_LAW_ITEM_CDF 1
#define MFCD_LAW_LISTS 2
#define MFCD_LAW_GROUPS 3

typedef struct mfcd_sampler {
    int32_t law, n, m, pair_rule;
    const double *cdf;
    const int32_t *list_i, *list_j;
    int32_t k, list_row_stride;
    const int32_t *users;
    int32_t n_users, use_margin;
    double margin;
    const float *X, *A, *B;
    int32_t dx, reserved;
} mfcd_sampler;

size_t mfcd_sample_workspace_bytes(int64_t attempts, int64_t n_barred);
int mfcd_sample_triplets(const mfcd_sampler *law, const int64_t *barred_keys, int64_t n_barred, int64_t attempt0,
                         int64_t attempts, uint64_t seed, int64_t want, int32_t *triplets_out, int64_t *keys_out,
                         int64_t *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Register-resident optimiser steps for states of up to 8 388 608 elements at d = 64 (round 3, opt-in: BASELINE
 * configs[3], n = m = 65536, d = 64, is exactly 1 024 SIMDs x 64 lanes x 128 rows).  The step of mfcd_train_steps
 * (structure.py:845-852) with the arithmetic of its streaming form (bit-identical results), as ONE persistent launch of
 * two waves per SIMD: exp_avg / exp_avg_sq of a wave's 64 rows in 128 registers per lane, the
 * parameters in LDS, rows exchanged per step through tagged granules (publish right before use).  fp32 tables, d == 64,
 * n + m <= 131072, B <= 64; a batch may name at most mfcd_train_big_slots() (8) distinct rows of one wave's 64-row slice (else status 2 and the call is void:
 * streams that concentrate on a few rows belong to the streaming form).  The call waits once on the host (its per-step
 * table is copied from the stack).  workspace: mfcd_train_big_workspace_bytes(N, B) — status word (int32, first 4
 * bytes; mfcd_train_big_status reads it: 0 ok, 1 a bounded wait expired, 2 too many rows of one wave in a batch), the
 * per-step scalars, N loss terms and the 1536-byte mailbox slot of every sample.
 */
size_t mfcd_train_big_workspace_bytes(int64_t N, int B);
int mfcd_train_steps_big(float *U, float *V, float *mU, float *vU, float *mV, float *vV, const mfcd_sample *samples,
                         int64_t N, int B, int64_t step0, int n, int m, int d, double lr, double beta1, double beta2,
                         double eps, double weight_decay, float *loss_per_step, void *workspace, size_t workspace_bytes,
                         void *stream);
int mfcd_train_big_status(const void *workspace, int *status_out, void *stream);
/* pre-check of a sample stream for the form above: *max_out_dev (device int32) = the largest number of row references
 * one wave's 64-row slice receives from one batch (an upper bound of the distinct rows); the form takes the call when
 * it is <= mfcd_train_big_slots(). */
int mfcd_train_big_slots(void);
int mfcd_train_big_check(const mfcd_sample *samples, int64_t N, int B, int n, int m, int *max_out_dev, void *stream);

/*
 * The k best and / or k worst columns of requested rows of a score matrix, without forming the matrix (no reference
 * counterpart as one function: the samplers call torch.topk(row, k) per attempt, generation_data.py:36-37, 212-213;
 * the recommendation extensions of structure.py need the same lists of U V^T).  Scores are either dense,
 * X [n][ldx] fp32, or (X == NULL) the fp32 products A[r] . B[c] of factors A [n][d], B [m][d], 1 <= d <= MFCD_MAX_D,
 * formed on the exact fp32 MFMA, once per (row, column): selection and the returned values see the same number.
 *   row_ids    `rows` row numbers (device), any order, repeats allowed; NULL = rows 0 .. rows-1.  A number outside
 *              [0, n) yields an empty result (index -1, value NaN) for that row.
 *   ends       1 best, 2 worst, 3 both (the scores are formed once).
 *   best_*     [rows][k]: the k largest scores of the row in descending order; worst_* the k smallest in ascending
 *              order.  Equal scores are ordered by ascending column; -0.0 equals +0.0.  NaN ranks above +inf for
 *              `best` (torch.topk's convention) and after every number for `worst`.  *_val (nullable) is the score
 *              that was compared.  Deterministic: two calls are bit-equal.
 *   excl_off, excl_items   optional CSR (device): columns excl_items[excl_off[r] .. excl_off[r + 1]) (ascending) are
 *              absent for requested row r, for both ends.  If fewer than k columns remain, the tail is -1 / NaN.
 * Limits: 1 <= k <= min(m, mfcd_topk_max_k()) (8192), m <= 4 194 304, any `rows` (the entry loops over slabs of rows).
 * MFCD_EINVAL outside them, with nothing launched.
 * workspace: mfcd_topk_rows_workspace_bytes(rows, m, d, k, ends) bytes, 256-byte aligned (d = 0 for the dense mode,
 * which needs none: 256 is returned; 0 = sizes out of range).  Factor mode: one slab of whole score rows of at most
 * 128 MiB (at least 128 rows); nothing of size n x m exists.  No allocation and no host wait.
 */
int mfcd_topk_max_k(void);
size_t mfcd_topk_rows_workspace_bytes(int rows, int m, int d, int k, int ends);
int mfcd_topk_rows(const float *X, int64_t ldx, const float *A, const float *B, int d, const int32_t *row_ids,
                   int rows, int n, int m, int k, int ends, const int64_t *excl_off, const int32_t *excl_items,
                   int32_t *best_idx, float *best_val, int32_t *worst_idx, float *worst_val, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * The two steps of Lloyd's k-means over row-major fp32 points [P][dim] (the `cluster` sampling strategy,
 * generation_data.py:229-247: sklearn KMeans over the item columns; the points are the columns of a dense X, or the
 * rows of B R^T with A^T A = R^T R for X = A B^T, which have the same pairwise distances).  The iteration, k-means++
 * and the empty-cluster rule are the host's (mfcd/cluster.py).
 *   assign   labels[p] = the nearest of the k centres [k][dim], the lowest index among equals, chosen as the argmax of
 *            p . c - |c|^2 / 2 with the products on the exact fp32 MFMA; nothing of size P x k is stored.  dist2
 *            (nullable) [P] = the fp32 squared distance to the chosen centre.  changed (nullable, device int32) = how
 *            many labels differ from the `labels` passed in.
 *   update   centres[c] = the mean of the points labelled c, summed in f64 in a fixed order and rounded once to fp32;
 *            counts[c] = their number.  A cluster without members keeps its centre and gets count 0; a label outside
 *            [0, k) is skipped.  No floating-point atomics: two calls are bit-equal.
 * Limits: 1 <= k <= the max_k entry below (64), 1 <= dim <= 2^30, 1 <= P <= 4 194 304, P * dim < 2^40; MFCD_EINVAL
 * outside them, with nothing launched.  workspace: as the workspace_bytes entry says (0 = sizes out of range), 256-byte
 * aligned, the same buffer for both steps.  No allocation and no host wait.
 */
int mfcd_kmeans_max_k(void);
size_t mfcd_kmeans_workspace_bytes(int64_t P, int64_t dim, int k);
int mfcd_kmeans_assign(const float *points, int64_t P, int64_t dim, const float *centres, int k, int32_t *labels,
                       float *dist2, int32_t *changed, void *workspace, size_t workspace_bytes, void *stream);
int mfcd_kmeans_update(const float *points, int64_t P, int64_t dim, const int32_t *labels, int k, float *centres,
                       int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Exact all-pairs statistics of score rows against ground-truth rows (no reference counterpart: the reference estimates
 * the test loss and accuracy of a model from a split of a few hundred sampled triplets, structure.py:369-390; these are
 * the population values those estimate, with the exact Kendall counts from the same pass).  Row r of A [rows][lda] holds
 * model scores a (the caller forms rows of U V^T with a plain library GEMM), row r of X [rows][ldx] the ground truth x,
 * m columns each, fp32, rows may be strided.  Everything is over the n0 = m (m - 1) / 2 unordered pairs i < j of a row.
 *   what     1 counts only, 2 sums only, 3 both; outputs are per row
 *   counts   [rows][4] int64, exact: C concordant ((a_i < a_j and x_i < x_j) or (a_i > a_j and x_i > x_j)), D discordant,
 *            Ta pairs with a_i == a_j, Tx pairs with x_i == x_j (a pair tied in both rows is in Ta and in Tx).  Decided by
 *            comparing the values themselves, never by the sign of a difference or of a product; -0.0 equals +0.0, +-inf
 *            compare as numbers; a NaN anywhere in either row sets the row's four counts to -1.  Kendall's
 *            tau-b = (C - D) / sqrt((n0 - Ta)(n0 - Tx)), pairwise accuracy = C / (n0 - Tx).
 *   sums     [rows][4] f64, with da = a_i - a_j, t = scale (x_i - x_j), q = sigmoid(t),
 *            softplus(v) = max(v, 0) + log1p(exp(-|v|)):
 *              risk        softplus(da) - q da: the BCE of p = sigmoid(da) against the label law q, unclamped (ATen clamps
 *                          the logs at -100, which differs only for |da| > 100)
 *              bayes_risk  softplus(t) - q t
 *              exp_acc     q if a_i > a_j, 1 - q if a_i < a_j, 0.5 if equal: the expectation of (p > 0.5) == z over hard
 *                          labels z and both orders of the pair
 *              bayes_acc   max(q, 1 - q)
 *            Per-pair arithmetic is fp32 (hardware exp / log / reciprocal, arranged so that no term cancels), at most
 *            64 terms are added in fp32 before widening, the rest is f64.  Any non-finite entry in either row makes
 *            the row's four sums NaN (the counts still follow their own rule).
 * One 256-thread workgroup per (row, tile of 1024 columns) visits the tile's pairs with itself and every later tile and
 * writes one fixed-size partial; a finishing kernel adds a row's partials in a fixed order.  No floating-point atomics:
 * two calls are bit-equal, and what = 1 / what = 2 are bit-equal to the matching half of what = 3.
 * Limits: rows >= 0 (0 = success, nothing launched), 1 <= m <= 1 048 576, lda, ldx >= m, what in {1, 2, 3}, scale finite;
 * MFCD_EINVAL outside them, a missing output of a requested `what` included, before anything touches the device.
 * workspace: as the workspace_bytes entry says (80 bytes per (row, tile), at most 80 MiB: longer inputs go through in
 * blocks of rows; 0 = sizes out of range), 256-byte aligned.  No allocation and no host wait.
 */
size_t mfcd_pair_stats_workspace_bytes(int rows, int m);
int mfcd_pair_stats_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m, double scale, int what,
                         int64_t *counts, double *sums, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The gradient of the `risk` sum above with respect to the scores (no reference counterpart: the reference descends the
 * BCE of sampled triplets, structure.py:845-852; this is the gradient of the population risk those samples estimate).
 * Row r of G [rows][ldg] receives, for every column i < m,
 *     g_i = sum over j != i of  sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j)),
 * the derivative of sums[r][0] of mfcd_pair_stats_rows with respect to a_i; columns >= m of G are not written.
 * One 256-thread workgroup per (row, tile of 1024 columns) visits the tile's pairs with EVERY tile of the row, so each
 * thread owns its sums and stores them itself (each unordered pair is visited twice; there is no workspace, no
 * finishing kernel and no atomic).  Per-pair arithmetic is fp32 on the hardware exp and reciprocal, with only exp of a
 * non-positive argument taken and sigmoid(|v|) = 1 / (1 + e), sigmoid(-|v|) = e / (1 + e) selected by the sign, so no
 * finite row overflows; an accumulator adds at most 64 terms in fp32 before it is widened to f64, and g_i is rounded to
 * fp32 once, on the store.  A row with a non-finite entry in A or X gets an all-NaN row of G.  Two calls are bit-equal,
 * and a row's result does not depend on the other rows of the call or on lda, ldx, ldg.
 * Limits: rows >= 0 (0 = success, nothing launched), 1 <= m <= 1 048 576, lda, ldx, ldg >= m, scale finite (as a float
 * too), G neither A nor X; MFCD_EINVAL outside them, before anything touches the device.  Long inputs go through in
 * blocks of rows.  No allocation and no host wait.
 */
int mfcd_pair_grad_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m, double scale, float *G,
                        int64_t ldg, void *stream);

/*
 * The two entries above under a pair law (no reference counterpart: per sampling strategy, the risk that the strategy's
 * own test split estimates, and the gradient of that risk).  The unordered pair {i, j} of a row carries the weight
 *     w_ij = (alpha_i beta_j + alpha_j beta_i, or 1 without alpha / beta)
 *            * [ |x_i - x_j| <= margin ]     if use_margin: the fp32 difference of the raw x (not scaled) against the
 *                                            margin, as mfcd_sample_triplets decides it; the entry rounds the margin down
 *                                            to the largest fp32 <= it once, which decides every pair identically
 *            * [ label_i != label_j ]        if labels
 * An ordered attempt law P(i, j) enters a symmetric loss only through P(i, j) + P(j, i), which is this family for every
 * device strategy of mfcd_sample_triplets.
 *   alpha, beta   fp32 [m] device vectors shared by all rows, both or neither; every entry finite and >= 0.  The caller
 *                 keeps every entry either 0 or within 1e-6 of the largest (mfcd/pairs.py: PairLaw scales the largest to
 *                 1 and zeroes smaller ones), so that every product is a normal fp32 number.
 *   labels        int32 device labels: label_stride = 0, one vector [m] for all rows; label_stride >= m, row r reads
 *                 labels + r * label_stride.  NULL: no label factor.
 *   support       [rows] int64: the exact number of pairs i < j with w > 0
 *   sums          [rows][5] f64: W = sum of w, then risk, bayes_risk, exp_acc, bayes_acc of mfcd_pair_stats_rows, each the
 *                 sum of w * term.  Without alpha / beta W equals the support exactly.  A row with W = 0 has sums of
 *                 exactly +0; a row with a non-finite entry in A or X has five NaN (its support is still counted).
 *   G             [rows][ldg] fp32: g_i = sum over j != i of w_ij (sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j))), the
 *                 derivative of sums[r][1] with respect to a_i; exactly +0 where no pair of i has weight; all NaN for a
 *                 row with a non-finite entry; columns >= m are not written.
 * Kernels, arithmetic and determinism are those of the two entries above: one 256-thread workgroup per (row, tile of
 * 1024 columns), the weight folded into every term by one fma, at most 64 terms in an fp32 run, f64 beyond, a finishing
 * kernel with a fixed order for the sums, no floating-point atomics, two calls bit-equal, a row independent of its
 * neighbours and of the leading dimensions.  The kernels are compiled per combination of the three factors: an absent
 * factor costs nothing.
 * Limits: those of the two entries above, and a law that is not NULL; MFCD_EINVAL also when exactly one of alpha / beta
 * is given, when use_margin is set with a negative or NaN margin, or when labels are given with a label_stride that is
 * neither 0 nor >= m; all before anything touches the device.  workspace: as the workspace_bytes entry says (56 bytes
 * per (row, tile), longer inputs go through in blocks of rows; 0 = sizes out of range), 256-byte aligned.  No allocation
 * and no host wait.
 */
typedef struct mfcd_pair_law {
    const float *alpha, *beta;
    const int32_t *labels;
    int64_t label_stride;
    int32_t use_margin, reserved;
    double margin;
} mfcd_pair_law;
size_t mfcd_pair_law_stats_workspace_bytes(int rows, int m);
int mfcd_pair_law_stats_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m, double scale,
                             const mfcd_pair_law *law, int64_t *support, double *sums, void *workspace,
                             size_t workspace_bytes, void *stream);
int mfcd_pair_law_grad_rows(const float *A, int64_t lda, const float *X, int64_t ldx, int rows, int m, double scale,
                            const mfcd_pair_law *law, float *G, int64_t ldg, void *stream);

/*
 * The Hessian of the `risk` sums above with respect to the scores, applied to a vector (no reference counterpart: the
 * curvature of the population risk, for second-order steps on it).  The risk sum of a row is a function of the score
 * differences alone, so its Hessian is the weighted graph Laplacian L(a): row r of Q [rows][ldq] receives, for every
 * column i < m,
 *     q_i = sum over j != i of  w_ij s_ij (y_i - y_j),     s_ij = sigmoid'(a_i - a_j) = p (1 - p),  p = sigmoid(a_i - a_j),
 * with y row r of Y and w_ij = 1 for the plain entry, the weight of mfcd_pair_law for the law entry.  deg is optional
 * (NULL: not computed, and the kernel compiled without it runs): row r of deg [rows][ldd] receives the diagonal of L,
 *     deg_i = sum over j != i of  w_ij s_ij,
 * with the column j = i excluded by a mask (its s is 1/4 whatever its weight).  Neither the labels' law nor `scale`
 * enters a second derivative; X is read by the law entry only, for the margin factor and for the finiteness rule.
 * Columns >= m of Q and deg are not written.
 * Kernel: the decomposition of mfcd_pair_grad_rows — one 256-thread workgroup per (row, tile of 1024 columns) against
 * EVERY tile of the row, four elements per thread in registers, each thread owning and storing its sums; no workspace,
 * no finishing kernel, no atomic.  Per ordered pair s = e h h with e = exp(-|a_i - a_j|), h = 1 / (1 + e): one hardware
 * exp and one reciprocal, symmetric in the sign, nothing selected and nothing cancelled; the term is s (y_i - y_j) with
 * the difference formed first, so a constant row of Y gives a row of Q of exactly +0, and a column whose every weight is
 * 0 gives exactly +0 in Q and deg.  An accumulator adds at most 64 terms in fp32 before it is widened to f64; q_i and
 * deg_i are rounded to fp32 once, on the store.  A row with a non-finite entry in A or Y (or X, for the law entry) gets
 * an all-NaN row of Q and of deg.  Two calls are bit-equal, Q does not depend on whether deg is asked for, and a row's
 * result does not depend on the other rows of the call or on the leading dimensions.  The law's flags compile to
 * kernels of their own as for the two law entries above: an absent factor costs nothing.
 * Limits: rows >= 0 (0 = success, nothing launched), 1 <= m <= 1 048 576, lda, ldy, ldq (ldx; ldd with deg) >= m, Q and
 * deg none of the inputs nor each other, and the law rules of mfcd_pair_law_grad_rows; MFCD_EINVAL outside them, before
 * anything touches the device.  Long inputs go through in blocks of rows.  No allocation and no host wait.
 */
int mfcd_pair_hvp_rows(const float *A, int64_t lda, const float *Y, int64_t ldy, int rows, int m, float *Q, int64_t ldq,
                       float *deg, int64_t ldd, void *stream);
int mfcd_pair_law_hvp_rows(const float *A, int64_t lda, const float *X, int64_t ldx, const float *Y, int64_t ldy, int rows,
                           int m, const mfcd_pair_law *law, float *Q, int64_t ldq, float *deg, int64_t ldd, void *stream);

/*
 * The same Laplacian applied to every column of an item table in one pass (no reference counterpart): the multi-column
 * form of mfcd_pair_law_hvp_rows, from which the d x d matrix a row's Laplacian induces on the item vectors,
 * H_r = B_r^T L(a_r) B_r, is one batched GEMM away (mfcd/pairs.py: pair_info_rows).  For row r of A [rows][lda] (and of X,
 * read for the law's margin and the finiteness rule only; NULL is allowed when the law has no margin) and every column
 * i < k of the row, row (r, i) of Z [rows][k][ldz] receives the d numbers
 *     z_i = sum over j != i of  w_ij s_ij (b_i - b_j),     s_ij = sigmoid'(a_i - a_j),
 * b_j = row index[r][j] of B [mB][ldb] (fp32, d columns), w the weight of the mfcd_pair_law struct; law = NULL is the
 * plain risk, w = 1.  index: int32; index_stride = 0, one vector [k] for all rows; index_stride >= k, row r reads index + r *
 * index_stride; NULL: column j is row j of B, and k must equal mB.  deg is optional: row r of deg [rows][ldd] receives
 * deg_i = sum over j != i of w_ij s_ij.  The column j = i contributes to neither.
 * Kernel (csrc/pair_info.hip): one 256-thread workgroup per (row, tile of 128 columns i, chunk of at most 128 columns of
 * d); the columns j stream through LDS in stages of 64; every lane generates one weight per v_mfma_f32_32x32x2_f32 step
 * (one exp, one reciprocal, as mfcd_pair_hvp_rows) and every further 32 columns of d reuse it: z_i = deg_i b~_i - sum
 * over j of c_ij b~_j on the fp32 matrix pipe.  b~ is B gathered and centred: a pre-pass forms the column mean of the
 * row's gathered table in f64 (one per row under a per-row index, one for all otherwise), and b~ = b - mean is formed
 * in f64 and rounded to fp32 once; z does not depend on the centre in exact arithmetic (L 1 = 0), and without it the
 * Laplacian form would cancel at the size of B's offset.  The fp32 accumulators are widened to f64 after every stage
 * (at most 64 terms; 32 for deg), z_i is formed from the f64 sums and rounded to fp32 once.
 * The pre-pass checks every index against mB before anything is gathered: a row that names an index outside [0, mB) is
 * all NaN (Z and deg), as is a row with a non-finite entry in A, in X (when given), or in a row of B it uses.  A column
 * without a weighted pair gets exactly +0.  No floating-point atomics, every sum has one owner and a fixed order: two
 * calls are bit-equal, a row's result does not depend on the other rows, on the leading dimensions or on deg being
 * asked for.
 * Limits: rows >= 0 (0 = success, nothing launched), 1 <= k <= 1 048 576, 1 <= d <= 256, mB >= 1, lda (ldx with X, ldd
 * with deg) >= k, ldb, ldz >= d, index_stride 0 or >= k, Z and deg none of the inputs nor each other, the law rules of
 * mfcd_pair_law_grad_rows for a law that is not NULL, and X not NULL under a law with a margin; MFCD_EINVAL outside them
 * and MFCD_EWORKSPACE for a short workspace, before anything touches the device.  workspace: as the workspace_bytes
 * entry says (2080 bytes per row of a block of at most 4096 rows; 0 = sizes out of range), 256-byte aligned.  Long inputs
 * go through in blocks of rows.  No allocation and no host wait.
 */
size_t mfcd_pair_hvp_multi_workspace_bytes(int rows, int k, int d);
int mfcd_pair_hvp_multi_rows(const float *A, int64_t lda, const float *X, int64_t ldx, const float *B, int64_t ldb, int mB,
                             int d, const int32_t *index, int64_t index_stride, int rows, int k, const mfcd_pair_law *law,
                             float *Z, int64_t ldz, float *deg, int64_t ldd, void *workspace, size_t workspace_bytes,
                             void *stream);

/*
 * Per column, the most informative admissible partner (no reference counterpart): the arg-max a D-optimal comparison
 * design needs per iteration (mfcd/design.py).  For row r of A [rows][lda] and every column i < k,
 *     best_val[r][i] = max over admissible j != i of  s_ij |g_i - g_j|^2,     s_ij = sigmoid'(a_i - a_j),
 *     best_j[r][i]   = the j that attains it, the smallest j among equal scores,
 * with g_j row j of the row's table G + r * g_row_stride, [k][ldg] fp32 with d columns; g_row_stride = 0 is one table
 * for all rows.  The pair (i, j) is admissible when the weight of the mfcd_pair_law struct is > 0: the law gives the
 * support only, its magnitude does not enter the score; law = NULL admits every pair.  X is read for the law's margin
 * and the finiteness rule only and may be NULL when the law has no margin.  A column without an admissible partner
 * (k = 1 included) gets the value +0 and the index -1.  A row with a non-finite entry in A, in X (when given) or in a row
 * of its table — or whose table has a row whose squared norm overflows fp32 — is all NaN / -1; the other rows are
 * untouched.  Columns >= k are not written.
 * Kernel (csrc/pair_best.hip): one 256-thread workgroup per (row, tile of 128 columns i); the columns j stream through
 * LDS in stages of 64, at most 128 columns of d at a time; the products g_i . g_j ride v_mfma_f32_32x32x2_f32 oriented so
 * that the accumulator's column is i, and |g_i - g_j|^2 = max(n_i + n_j - 2 g_i . g_j, 0) with the squared norms n of a
 * pre-pass (f64 sum in the order of the columns, rounded to fp32 once).  The table is NOT centred here: the caller
 * subtracts the column mean, so that the cancellation is at the size of the table's spread.  s = e h h with
 * e = exp(-|a_i - a_j|), h = 1 / (1 + e), as mfcd_pair_hvp_rows.  A lane owns one i and sixteen j per 32 x 32 block and
 * keeps a running (max, arg) in registers; the two half-waves of a column are combined once, the tie to the smaller j.
 * No atomics, every result has one owner: two calls are bit-equal, and a row's result does not depend on the other rows,
 * on the leading dimensions or on its place in the call.  An odd d is padded with zero columns inside the kernel.
 * Limits: rows >= 0 (0 = success, nothing launched), 1 <= k <= 1 048 576, 1 <= d <= 256, lda, ldv, ldj (ldx with X) >= k,
 * ldg >= d, g_row_stride 0 or >= k * ldg, the outputs none of the inputs nor each other, the law rules of
 * mfcd_pair_law_grad_rows for a law that is not NULL, and X not NULL under a law with a margin; MFCD_EINVAL outside them
 * and MFCD_EWORKSPACE for a short workspace, before anything touches the device.  workspace: as the workspace_bytes
 * entry says (4 k bytes per row of a block of rows of at most 64 MiB; 0 = sizes out of range), 256-byte aligned.  Long
 * inputs go through in blocks of rows.  No allocation and no host wait.
 */
size_t mfcd_pair_best_workspace_bytes(int rows, int k, int d);
int mfcd_pair_best_rows(const float *A, int64_t lda, const float *X, int64_t ldx, const float *G, int64_t g_row_stride,
                        int64_t ldg, int d, int rows, int k, const mfcd_pair_law *law, float *best_val, int64_t ldv,
                        int32_t *best_j, int64_t ldj, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The exact user step of the BTL fit, "fold-in" (no reference counterpart: the reference only ever moves U and V
 * together, structure.py:845-852): with the item table V [m][d] held fixed, row r of U_out is the minimiser of
 *     f(u) = sum over t of  softplus(x_t) - z_t x_t  +  (l2 / 2) |u|^2,     x_t = u . delta_t,  delta_t = V[i_t] - V[j_t],
 * over the records t in records[row_off[r] .. row_off[r + 1]).  row_off is an ascending device array of rows + 1
 * entries; the records' u field is not read (grouping is the caller's job); z may be any value in [0, 1].  The sum is
 * not a mean and l2 > 0 is required: the Hessian is then positive definite and the minimiser unique, also for separable
 * labels.  The algorithm is fixed (tests/foldin_model.py restates it):
 *   1. u starts at U_init[r], or at 0 when U_init is NULL.
 *   2. Per iteration p_t = sigmoid(x_t), g = sum (p_t - z_t) delta_t + l2 u, H = sum p_t (1 - p_t) delta_t delta_t^T
 *      + l2 I, and H s = -g is solved by Cholesky.
 *   3. Backtracking with t = 1, 1/2, 1/4, ... until f(u + t s) <= f(u) + 1e-4 t g.s, at most 30 halvings; then
 *      u <- u + t s.  The test is taken on the decrease f(u + t s) - f(u) summed term by term in f64 — with
 *      h = t s . delta_t, softplus(x_t + h) - softplus(x_t) = log1p(p_t expm1(h)) for |h| < 1, the difference of the two
 *      values otherwise, plus l2 (t u.s + t^2 |s|^2 / 2) — not on two rounded values of f: next to the minimiser the
 *      decrease of a full Newton step is below the last bit of f, and a warm start from an fp32 row would otherwise
 *      have its steps halved at random.  A step so small that this sum is itself at its rounding level is accepted when
 *      the two values of f satisfy the test (at the latest when u + t s == u).
 *   4. Status 0 (converged) when |t s|_inf <= xtol |u|_inf for the new u, or when s is exactly 0.
 *   5. Status 1 (stopped) after max_iter iterations, when 30 halvings did not decrease f, or when a pivot of the
 *      Cholesky factor is not positive; u is then the last accepted iterate.
 * Precision: the iterate, x_t, p_t, g, H, f and the solve are f64; V is read as fp32 and widened exactly, so delta_t is
 * exact.  U_out is the f64 iterate rounded once to fp32, objective[r] (nullable) is f at the f64 iterate,
 * iters_status[r] = {iterations taken, status}.
 * Status 2 is a row with invalid data — an i or j outside [0, m), a z that is NaN or outside [0, 1], a non-finite entry
 * in a V row the row uses or in its U_init row, records == NULL for a row with records, row_off descending: U_out[r] is
 * all NaN, the objective NaN, 0 iterations.  Indices are validated before any gather, so nothing is read outside the
 * tables.  A row without records has u = 0, objective 0, 0 iterations and status 0, whatever its U_init.
 * One workgroup per row (256 threads, one wave for d <= 16) runs the whole iteration: comparisons are staged in LDS
 * mfcd_fold_in_chunk() at a time, threads own the gradient entries and 4 x 4 blocks of the Hessian, which is formed on
 * the f64 vector pipe, and the Cholesky factor lives in LDS.  No floating-point atomics: two calls are bit-equal, and a
 * row's outputs depend only on its own records, its U_init row, V and the scalars, not on the other rows of the call or
 * on its position in it.
 * Limits: 1 <= d <= mfcd_fold_in_max_d() = 64, m >= 1, rows >= 0 (0 = success, nothing launched), l2 finite and > 0,
 * 1 <= max_iter <= 1000, xtol finite and >= 0, U_out overlapping neither V nor U_init; MFCD_EINVAL outside them and
 * MFCD_EWORKSPACE for a short workspace, both before anything touches the device.  workspace: as the workspace_bytes
 * entry says (256: the kernel stages nothing in device memory; 0 = sizes out of range).  No allocation and no host wait.
 * Wider tables (d up to 256): mfcd_fold_in_users_cg below solves the same problem without forming the Hessian.
 */
int mfcd_fold_in_max_d(void);
int mfcd_fold_in_chunk(void);
size_t mfcd_fold_in_workspace_bytes(int rows, int d);
int mfcd_fold_in_users(const float *V, int m, int d, const mfcd_sample *records, const int64_t *row_off, int rows,
                       double l2, const float *U_init, int max_iter, double xtol, float *U_out, double *objective,
                       int32_t *iters_status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The exact item step (no reference counterpart).  A comparison couples two item rows, but with U and the other items
 * held fixed, item k's row minimises a logistic regression with an offset over the comparisons that hold k:
 *     f_k(v) = sum over t of  softplus(x_t) - z_t x_t  +  (l2 / 2) |v|^2,     x_t = sigma_t (U[u_t] . v) + c_t,
 *     sigma_t = [i_t = k] - [j_t = k]  (+1, -1, or 0 for a comparison of k with itself),
 *     c_t = -sigma_t (U[u_t] . V[o_t]),  o_t the other item of the comparison.
 * Row r solves item k = row_item[r] (row_item NULL: k = r, and then rows <= m) over records[row_off[r] .. row_off[r + 1])
 * in the mfcd_sample layout; every one of them must have i = k or j = k (a comparison appears once in the row of each of
 * its two items; grouping is the caller's job).  The start is V[k].  The solve is the iteration of the user step above,
 * unchanged — steps 2 to 5 with delta_t = sigma_t U[u_t] and the x chain started at c_t instead of 0 — and v* is its
 * result.  Outputs: V_out[r] = v_old + theta (v* - v_old), formed in f64 and rounded once to fp32; objective2 (nullable)
 * [rows][2] = {f_k(v_old), f_k(v*)}; iters_status as for users.  theta = 1 is the exact minimiser of one item against
 * the given rows of all others.  With theta = 1/2 every item may be moved in one call and the total objective
 * F(U, V) = sum of all terms + (l2 / 2)(|U|^2 + |V|^2) still falls: every loss term depends on two item rows only, so by
 * convexity F(V_new) <= F(V) - (1/2) sum over k of (f_k(v_k) - f_k(v*_k)).
 * Precision: c_t is an f64 fma chain over the d products (double)U[u_t][k] (double)V[o_t][k], k ascending, formed once
 * per call and kept in the workspace; delta_t is exact; everything else as for users.
 * Status 2 (V_out[r] all NaN, both objectives NaN, 0 iterations): row_item[r] outside [0, m); a u outside [0, n) or an i
 * or j outside [0, m); a record with neither i nor j equal to k; a z that is NaN or outside [0, 1]; a non-finite entry in
 * V[k], in a U row the row uses or in a V[o_t] row it uses; records == NULL for a row with records, row_off descending
 * or negative, or records that end beyond the 8 bytes per record the workspace has room for.  Indices are validated
 * before any gather.  A row without records has v* = 0: V_out[r] = (1 - theta) v_old, objective2 = {(l2 / 2) |v_old|^2,
 * 0}, 0 iterations, status 0.
 * Same kernel as the user step with another staging rule: one workgroup per row, no floating-point atomics, no
 * communication between workgroups; two calls are bit-equal, and a row's outputs do not depend on the other rows of the
 * call or on its position in it (two rows may name one item and then agree bit for bit).
 * Limits: 1 <= d <= 64 (wider tables: mfcd_item_step_cg below), n >= 1, m >= 1, rows >= 0 (0 = success, nothing
 * launched), l2 finite and > 0, 0 < theta <= 1,
 * max_iter and xtol as for users, V_out [rows][d] overlapping neither U nor V; MFCD_EINVAL outside them and
 * MFCD_EWORKSPACE for a workspace below the size for 0 records, both before anything touches the device.  workspace: as
 * the workspace_bytes entry says for the number of records (256 + 8 per record, rounded up to 256; 0 = sizes out of
 * range); the host cannot see row_off, so a workspace too short for a row's records shows as status 2 of that row.  No
 * allocation and no host wait.
 */
size_t mfcd_item_step_workspace_bytes(int rows, int d, int64_t records);
int mfcd_item_step(const float *U, int n, const float *V, int m, int d, const mfcd_sample *records,
                   const int64_t *row_off, const int32_t *row_item, int rows, double l2, double theta, int max_iter,
                   double xtol, float *V_out, double *objective2, int32_t *iters_status, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * The two exact block steps for 1 <= d <= mfcd_fold_in_cg_max_d() = 256 (no reference counterpart): the problems of
 * mfcd_fold_in_users and mfcd_item_step, solved by damped Newton whose step comes from conjugate gradients on
 * Hessian-vector products, so that no d x d matrix is formed or factored.  The narrow widths are accepted too, so the
 * two solvers can be compared where both apply.  The objective f, delta_t, c_t, sigma_t, the start (U_init[r] or 0; V[k]),
 * the validation rules and status 2 with its NaN row, the rows without records, theta and the two objectives of the
 * item step, the line search (step 3 above) and the precision rules are those of the two entries above.  Three things
 * differ (tests/foldin_cg_model.py restates them):
 *   The step.  H s = -g with H = sum w_t delta_t delta_t^T + l2 I, w_t = p_t (1 - p_t), by preconditioned CG from
 *     s = 0.  H is applied only as q = sum_t w_t (delta_t . p) delta_t + l2 p.  The preconditioner is Jacobi,
 *     diag(H)_k = sum_t w_t delta_t[k]^2 + l2.  CG stops when |r|_2 <= eta |g|_2 with eta = 1e-3, or after 4 d + 50
 *     iterations; the iterate it then holds is a descent direction (every CG iterate from s = 0 is), and the line search
 *     takes it as it is, with g.s of that iterate in the Armijo rule.
 *   The order of an iteration.  Every pass forms f, g and the diagonal at the current u; then the stop rule; then, if
 *     fewer than max_iter solves were made, a CG solve, the line search and u <- u + t s.  iters_status[r][0] counts
 *     the CG solves, so a start that is already certified reports 0 iterations; cg_iters[r] (nullable) is the total of
 *     CG iterations of the row — the number that tells why a row was slow.
 *   The certificate.  The Cholesky form stops on a Newton step below xtol, which certifies a row only because an exact
 *     Newton step converges quadratically; an inexact step does not.  Here f is l2-strongly convex, so for every u
 *     |u - u*|_2 <= |g(u)|_2 / l2, and status 0 is given when |g|_2 <= l2 gtol |u|_inf on the gradient of a pass, which
 *     implies |u - u*|_inf <= gtol |u|_inf.  With the default gtol = 2^-26 and the one fp32 rounding of the output
 *     (2^-24), U_out is within 2^-22 |u*|_inf of the minimiser.  g = 0 exactly passes.  A row whose minimiser is exactly
 *     0 is certified only from the start 0 (|u|_inf shrinks with |g|_2), as in the Cholesky form.  Where l2 is so small
 *     that the rounding floor of g, about 2^-53 sum |p_t - z_t| |delta_t|, lies above l2 gtol |u|_inf, the test cannot
 *     be met: the row ends with status 1 and its last iterate.
 *   Status 1 (stopped): max_iter solves made and the gradient of the next pass not certified; 30 halvings without
 *     decrease; or p.q not positive or not finite inside CG.  u is the last accepted iterate, the objective is f there.
 * objective (users) is f at the f64 iterate, objective2 (items) = {f_k(v_old), f_k(v*)}, both from a gradient pass.
 * One workgroup of 256 threads per row, no floating-point atomics, every sum with one owner and a fixed order: two
 * calls are bit-equal, and a row's outputs depend only on its own records, its start row, the tables and the scalars.
 * A row of at most mfcd_fold_in_cg_resident(d) comparisons keeps its delta_t (and w_t, x_t) in LDS for the whole solve;
 * a longer one is gathered again on every pass, mfcd_fold_in_cg_chunk(d) comparisons at a time, and keeps w_t, x_t and
 * s . delta_t in the workspace.  Which of the two a row takes depends on its length and d alone; both numbers are 0 for
 * d outside [1, 256].
 * Limits: 1 <= d <= 256, gtol finite and >= 0 in place of xtol, cg_iters NULL or [rows]; everything else as for the two
 * entries above, MFCD_EINVAL and MFCD_EWORKSPACE before anything touches the device.  workspace: as the workspace_bytes
 * entries say for the number of records (256 + 24 per record for users, 256 + 32 per record for items, rounded up to
 * 256; 0 = sizes out of range); the host cannot see row_off, so it requires the size for 0 records, and a row whose
 * records end beyond the room the workspace has is status 2 of that row, for users as for items.  No allocation and no
 * host wait.
 */
int mfcd_fold_in_cg_max_d(void);
int mfcd_fold_in_cg_chunk(int d);
int mfcd_fold_in_cg_resident(int d);
size_t mfcd_fold_in_cg_workspace_bytes(int rows, int d, int64_t records);
int mfcd_fold_in_users_cg(const float *V, int m, int d, const mfcd_sample *records, const int64_t *row_off, int rows,
                          double l2, const float *U_init, int max_iter, double gtol, float *U_out, double *objective,
                          int32_t *iters_status, int32_t *cg_iters, void *workspace, size_t workspace_bytes,
                          void *stream);
size_t mfcd_item_step_cg_workspace_bytes(int rows, int d, int64_t records);
int mfcd_item_step_cg(const float *U, int n, const float *V, int m, int d, const mfcd_sample *records,
                      const int64_t *row_off, const int32_t *row_item, int rows, double l2, double theta, int max_iter,
                      double gtol, float *V_out, double *objective2, int32_t *iters_status, int32_t *cg_iters,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gradient and Hessian-vector product of the sampled BTL objective with respect to both tables (no reference
 * counterpart; tests/newton_model.py restates the arithmetic):
 *   F(U, V) = sum_t softplus(x_t) - z_t x_t + (l2 / 2)(|U|^2 + |V|^2),   x_t = U[u_t] . (V[i_t] - V[j_t]).
 * With delta_t = V[i_t] - V[j_t], p_t = sigmoid(x_t), r_t = p_t - z_t, w_t = p_t (1 - p_t), sigma_t = [i_t = k] - [j_t = k]
 * and a direction (P [n][d], Q [m][d]),  y_t = P[u_t] . delta_t + U[u_t] . (Q[i_t] - Q[j_t]):
 *   pass 0, side 0:  out[r] = sum_t r_t delta_t + l2 U[u],  diag[r][c] = sum_t w_t delta_t[c]^2 + l2,
 *                    loss[r] = sum_t softplus(x_t) - z_t x_t        (the sum of loss over all users is F's data term)
 *   pass 0, side 1:  out[r] = sum_t sigma_t r_t U[u_t] + l2 V[k],  diag[r][c] = sum_t sigma_t^2 w_t U[u_t][c]^2 + l2
 *   pass 1, side 0:  out[r] = sum_t (w_t y_t delta_t + r_t (Q[i_t] - Q[j_t])) + l2 P[u]
 *   pass 1, side 1:  out[r] = sum_t sigma_t (w_t y_t U[u_t] + r_t P[u_t]) + l2 Q[k]
 * the sums over the records of row r, which owns table row u = k = row_id[r] (NULL: r).  gauss_newton = 1 drops the two
 * r_t terms of pass 1 (the product is then positive semidefinite; the exact one need not be).  diag is the diagonal of
 * the row's own block of the Hessian.  records / row_off are those of mfcd_fold_in_users (side 0: the comparisons sorted
 * by user) and of mfcd_item_step (side 1: every comparison once in the row of its i and once in the row of its j; one
 * with i = j appears twice in one row and adds exactly nothing there).
 * Segments.  A row's records are cut into row-relative segments of S = mfcd_triplet_rows_segment() records: segment s of
 * row r covers records [row_off[r] + s S, ...).  The caller passes seg_off [rows + 1], the prefix sum of
 * ceil(len_r / S), and its total n_seg (the host cannot see row_off, and the entry has no host wait).  A first kernel
 * gives one wave to every segment: it finds its row by binary search in seg_off and writes the segment's sums to the
 * workspace in f64.  A second kernel gives every output element one owner, which adds the row's segments in ascending
 * order and then the l2 term.  Inside a wave a group of L = min(64, next power of two >= d) lanes holds one record, so
 * 64 / L records are in flight; dot products are cross-lane sums in a fixed order, and so are the sums over the groups.
 * No floating-point atomics.  So two calls are bit-equal; a row's outputs depend only on its own records, the table
 * rows they name and the scalars, not on the row's place in the call or on the other rows; and a long row is spread over
 * many waves.  All tables, directions, outputs and arithmetic are f64.
 * Validation, before any gather: side 0: u = the row's user, i and j in [0, m); side 1: u in [0, n), i and j in [0, m),
 * i or j the row's item; z in [0, 1] and not NaN; the row's own index in range; row_off[r] >= 0 and <= row_off[r + 1];
 * seg_off[r + 1] - seg_off[r] = ceil(len_r / S) inside [0, n_seg].  A row that fails gets status 2, an all-NaN out and
 * diag and a NaN loss, and nothing is read outside the tables; the other rows are not touched by it.  Non-finite table
 * entries are not looked for: they propagate by arithmetic.  A row without records gets out = l2 x (its row of the
 * table, or of the direction in pass 1) exactly, diag = l2, loss = 0, status 0.
 * Limits: side, pass and gauss_newton in {0, 1}, 1 <= d <= 256, n >= 1, m >= 1, rows >= 0 (0 = success, nothing
 * launched), rows <= n (m) where row_id is NULL, 0 <= n_seg <= 2^31, l2 finite and > 0, P and Q in pass 1 (ignored in
 * pass 0), records where n_seg > 0; diag (pass 0) and loss (pass 0, side 0) may be NULL and are ignored elsewhere; out,
 * diag and loss overlapping none of U, V, P, Q; MFCD_EINVAL outside them and MFCD_EWORKSPACE for a workspace below
 * mfcd_triplet_rows_workspace_bytes(rows, d, n_seg) (256 + (2 d + 1) doubles and one int32 per segment, each region
 * rounded up to 256; 0 = sizes out of range), both before anything touches the device.  No allocation and no host wait.
 */
int mfcd_triplet_rows_segment(void);
size_t mfcd_triplet_rows_workspace_bytes(int rows, int d, int64_t n_seg);
int mfcd_triplet_rows(int side, int pass, int gauss_newton, const double *U, int n, const double *V, int m, int d,
                      const double *P, const double *Q, const mfcd_sample *records, const int64_t *row_off,
                      const int32_t *row_id, int rows, const int64_t *seg_off, int64_t n_seg, double l2, double *out,
                      double *diag, double *loss, int32_t *status, void *workspace, size_t workspace_bytes,
                      void *stream);

/*
 * The statistics of mfcd_pair_stats_rows over ragged rows (no reference counterpart: the reference's Draft/ loads a
 * ratings table, 20 to 737 ratings per user, and never scores a model on it; this is the exact BTL risk and the exact
 * Kendall counts of a model on the ratings a user gave).  CSR layout: row r owns entries [row_off[r], row_off[r + 1]) of
 * x [entries] (the observed values) and of a [entries] (the model's scores of the same entries), fp32; row_off is int64
 * [rows + 1].  Everything is over the n0 = L (L - 1) / 2 unordered pairs among a row's L entries; no pair is formed in
 * memory.
 *   counts, sums, what, scale   per row, exactly as mfcd_pair_stats_rows defines them with m replaced by L: the same
 *            comparison rules, the same per-pair functions (csrc/pairs_common.h), fp32 runs of at most 64 terms widened
 *            to f64; a NaN in the row gives counts -1, any non-finite entry NaN sums.  A row of 0 or 1 entries gives zero
 *            counts and +0 sums.
 *   flags    bit 0, MFCD_RAGGED_SKIP_TIES: pairs with x_k == x_l (compared as values: -0.0 equals +0.0) leave the four
 *            sums, as a ratings table's ties carry no preference; the row's support is then n0 - Tx.  The counts are
 *            not affected.
 *   status   [rows] int32: 0, or 2 for a row that fails validation; such a row has counts -1 and NaN sums.
 * Tiles.  A row is cut into tiles of TILE = mfcd_pair_ragged_tile() = 256 entries.  The caller passes tile_off
 * [rows + 1], the prefix sum of ceil(L_r / TILE), and its total n_tiles (the host cannot see row_off, and the entry has
 * no host wait).  A first kernel validates every row before any entry of it is read: 0 <= row_off[r] <= row_off[r + 1]
 * <= entries, L <= 1 048 576, tile_off[r + 1] - tile_off[r] = ceil(L / TILE) inside [0, n_tiles], and every tile of the
 * row found by the binary search over tile_off.  Then one 256-thread workgroup per tile, one entry per thread, finds its
 * row by that search and visits its tile's pairs with itself and with every later tile of the row, read from LDS as a
 * broadcast; it writes one fixed-size partial, and a finishing kernel (one wave per row) adds a row's partials in a
 * fixed order.  No address is formed from the offsets of a row that failed.  No floating-point atomics: two calls are
 * bit-equal, what = 1 / what = 2 are bit-equal to the matching half of what = 3, and a row's outputs do not depend on
 * the other rows of the call or on its position in it.
 * Limits: rows >= 0 (0 = success, nothing launched), entries >= 0, n_tiles >= 0, what in {1, 2, 3} with its outputs
 * present, flags in {0, 1}, scale finite (as a float too), a and x where entries > 0, row_off, tile_off and status;
 * MFCD_EINVAL outside them and MFCD_EWORKSPACE for a short workspace, before anything touches the device.  workspace:
 * mfcd_pair_ragged_workspace_bytes(rows, n_tiles), 80 bytes per tile (less than a twenty-fifth of the tiles' own
 * entries; 0 = sizes out of range), 256-byte aligned; launches are cut to 2^20 workgroups.  No allocation and no host
 * wait.
 */
#define MFCD_RAGGED_SKIP_TIES 1
int mfcd_pair_ragged_tile(void);
size_t mfcd_pair_ragged_workspace_bytes(int rows, int64_t n_tiles);
int mfcd_pair_ragged_stats(const float *a, const float *x, int64_t entries, const int64_t *row_off, int rows,
                           const int64_t *tile_off, int64_t n_tiles, double scale, int flags, int what, int64_t *counts,
                           double *sums, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The gradient of the `risk` sum above with respect to the scores, on the same layout (no reference counterpart).  Entry
 * e of g [entries] receives
 *     g_e = sum over the other entries l of e's row of  w_el (sigmoid(a_e - a_l) - sigmoid(scale (x_e - x_l))),
 * w_el = 1, or under MFCD_RAGGED_SKIP_TIES [x_e != x_l]; the arithmetic is mfcd_pair_grad_rows' (csrc/pairs_common.h),
 * rounded to fp32 once.  The same validation kernel runs first; then one workgroup per tile visits its tile's pairs with
 * EVERY tile of the row, so each thread owns its sum and stores it itself: no workspace, no finishing kernel, no atomic.
 * A row that fails validation gets status 2 and none of its entries of g is written; a row with a non-finite entry gets
 * an all-NaN slice (status 0) and the other rows are untouched; a row of one entry gets exactly +0.  Two calls are
 * bit-equal and a row's slice does not depend on the other rows or on its position.
 * Limits: those above, g where entries > 0, g neither a nor x; MFCD_EINVAL outside them, before anything touches the
 * device.  No allocation and no host wait.
 */
int mfcd_pair_ragged_grad(const float *a, const float *x, int64_t entries, const int64_t *row_off, int rows,
                          const int64_t *tile_off, int64_t n_tiles, double scale, int flags, float *g, int32_t *status,
                          void *stream);

/*
 * The Hessian of the `risk` sum above with respect to the scores, applied to a vector y [entries], on the same layout
 * (no reference counterpart): mfcd_pair_hvp_rows over ragged rows.  Entry e receives
 *     q_e   = sum over the other entries l of e's row of  w_el s_el (y_e - y_l),   s_el = sigmoid'(a_e - a_l),
 *     deg_e = sum over the other entries l of e's row of  w_el s_el                (deg may be NULL: not computed),
 * w_el = 1, or under MFCD_RAGGED_SKIP_TIES [x_e != x_l]: the row Laplacian L(a) applied to y, and its diagonal.  Neither
 * the scale nor the label law enters a second derivative, so there is no `scale`; x is read under the skip flag only (it
 * may be NULL without it).  The arithmetic is mfcd_pair_hvp_rows' (csrc/pairs_common.h: pair_curvature, the difference
 * of y formed first, one fma), in fp32 runs of at most 64 columns counted from the row's start, widened to f64 and
 * rounded to fp32 once: on rows of one length q and deg are bit-equal to mfcd_pair_hvp_rows'.  The decomposition is
 * mfcd_pair_ragged_grad's: the same validation kernel, one workgroup per tile against EVERY tile of the row, no
 * workspace, no finishing kernel, no atomic.  An entry's own column adds exactly 0 to q and is masked out of deg.
 * A row that fails validation gets status 2 and none of its entries of q or deg is written; a row with a non-finite a or
 * y (or x under the skip flag) gets all-NaN slices (status 0) and the other rows are untouched; a row of one entry and
 * a y constant over the row give exactly +0 in q.  Two calls are bit-equal, q does not depend on whether deg is asked
 * for, and a row's slices do not depend on the other rows or on its position.
 * Limits: those of mfcd_pair_ragged_grad without x and scale; a, y, q and under the skip flag x where entries > 0; q
 * and deg distinct from the inputs and from each other; MFCD_EINVAL outside them, before anything touches the device.
 * No allocation and no host wait.
 */
int mfcd_pair_ragged_hvp(const float *a, const float *x, const float *y, int64_t entries, const int64_t *row_off, int rows,
                         const int64_t *tile_off, int64_t n_tiles, int flags, float *q, float *deg, int32_t *status,
                         void *stream);

/*
 * The scores of a ratings table's entries (no reference counterpart): a_e = R[r] . C[idx_e] for the entries of row r,
 * R [n_r][d] and C [n_c][d] fp32 factor tables, idx int32 [entries] (the item of an entry).  One 256-thread workgroup
 * per row; fp32 products, each rounded, added in ascending column order.  Before any gather the row's offsets
 * (0 <= row_off[r] <= row_off[r + 1] <= entries) and every idx of the row (in [0, n_c)) are checked: an invalid row gets
 * status 2 and, where its offsets are valid, an all-NaN slice of a.
 * Limits: 1 <= d <= 256, 0 <= rows <= n_r, n_c >= 1, entries >= 0, idx and a where entries > 0, a neither R nor C;
 * MFCD_EINVAL outside them, before anything touches the device.  No allocation and no host wait.
 */
int mfcd_ragged_dot(const float *R, int n_r, const float *C, int n_c, int d, int64_t entries, const int64_t *row_off,
                    int rows, const int32_t *idx, float *a, int32_t *status, void *stream);

/*
 * The carry of a per-entry coefficient to a factor table (no reference counterpart):
 *     out[r] = sum over the entries e of row r of  coef[perm ? perm[e] : e] * T[idx_e],
 * T [t_rows][d] fp32, out [rows][d] fp32.  With coef the gradient of mfcd_pair_ragged_grad it is called once by user
 * (T = V, idx the entries' items) and once by item on the transposed layout (T = U, idx the entries' users, perm [entries]
 * int64 mapping a transposed position to its CSR entry).
 * Segments, as mfcd_triplet_rows: a row is cut into segments of S = mfcd_ragged_segment() = 256 entries, the caller
 * passes seg_off [rows + 1], the prefix sum of ceil(L_r / S), and n_seg.  One wave per segment adds coef * T in f64
 * (the product of two fp32 values is exact there) and writes the segment's d sums to the workspace; a second kernel
 * gives every output element one owner, which adds the row's segments in ascending order and rounds to fp32 once: an
 * item with a hundred thousand ratings is spread over hundreds of waves.  No floating-point atomics: two calls are
 * bit-equal and a row depends only on its own entries.
 * Validation, before any gather: the row's offsets and segment range (as above), every idx in [0, t_rows), every perm
 * in [0, entries).  A row that fails gets status 2 and an all-NaN row of out.  A row without entries gets +0.
 * Limits: 1 <= d <= 256, rows >= 0 (0 = success, nothing launched), 0 <= n_seg <= 2^31, t_rows >= 1, idx and coef where
 * n_seg > 0, out neither T nor coef; MFCD_EINVAL outside them and MFCD_EWORKSPACE for a workspace below
 * mfcd_ragged_gather_sum_workspace_bytes(rows, d, n_seg) (256 + d doubles and one int32 per segment, each region rounded
 * up to 256; 0 = sizes out of range), before anything touches the device.  No allocation and no host wait.
 */
int mfcd_ragged_segment(void);
size_t mfcd_ragged_gather_sum_workspace_bytes(int rows, int d, int64_t n_seg);
int mfcd_ragged_gather_sum(const float *T, int t_rows, int d, int64_t entries, const int64_t *row_off, int rows,
                           const int32_t *idx, const float *coef, const int64_t *perm, const int64_t *seg_off,
                           int64_t n_seg, float *out, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream);

/*
 * The exact user step on a ratings table in one launch (no reference counterpart): what mfcd/ratings_exact.py's
 * ratings_user_step computes with a chain of small launches per Newton iteration.  Row r owns entries
 * [row_off[r], row_off[r+1]) of idx (int32, the entry's item: a row of V [m][d]) and x (its rating), L of them.  With V
 * fixed, U_out[r] minimises
 *     f(u) = coef * R_r(a) + (l2 / 2) |u|^2,   a_e = u . v_e,
 *     R_r(a) = sum over the pairs e < l of the row of  w_el [softplus(a_e - a_l) - sigmoid(scale (x_e - x_l)) (a_e - a_l)],
 * w_el = 1, or [x_e != x_l] under MFCD_RAGGED_SKIP_TIES: R_r is the `risk` sum of mfcd_pair_ragged_stats.  U_init = NULL
 * starts every row at 0 (the fold-in of users who were not in training) and is bit-equal to a zero U_init.
 * Algorithm (mfcd/population.py's _newton with solver "direct", per row; tests/ratings_foldin_model.py restates it):
 *   1. u = U_init[r] or 0, t = 1, iterations = 0.
 *   2. g = coef sum_e g_e v~_e + l2 u, g_e = sum over l != e of w_el (sigmoid(a_e - a_l) - sigmoid(scale (x_e - x_l))).
 *      |g|_2 <= gtol l2 |u|_inf: status 0.  Otherwise iterations == max_newton: status 1.
 *   3. If u moved since the direction was formed, or there is none yet:
 *      H = coef sum_{e<l} w_el sigmoid'(a_e - a_l)(v~_e - v~_l)(v~_e - v~_l)^T + l2 I, p = -H^{-1} g by Cholesky in LDS; a
 *      pivot that is not positive: p = -g / mean(diag H).
 *   4. f_t = f(u + t p), iterations += 1.  f_t <= f + 1e-4 t (g . p) (a NaN f_t fails): u += t p, t = min(2 t, 1).
 *      Otherwise t /= 2, the direction is kept, and t < 2^-12 ends the row with status 1.  Back to 2.
 *      The inequality is evaluated twice and either evaluation accepts, as in mfcd_fold_in_users: on the two values of
 *      f, and on the decrease f(u + t p) - f(u) summed pair by pair (softplus(a + h) - softplus(a) = log1p(sigmoid(a)
 *      expm1(h)) for |h| < 1), which resolves decreases below the fp32 rounding of f itself.
 * Precision: u, g, H, the solves, f and every dot product over d are f64.  v~_e is the gathered row minus the row's f64
 * column mean, rounded to fp32 once (everything above depends on differences of the v_e only); a_e is an f64 chain over
 * k rounded to fp32 once; the pair arithmetic is fp32, csrc/pairs_common.h's (pair_sigmoid, pair_curvature, the risk
 * terms of pair_term), in runs of at most 64 terms widened to f64; Z = (D - C) V~ is formed per entry in fp32 runs of 64
 * columns on the vector pipe, widened to f64 and rounded to fp32 once, and H = V~^T Z is added in f64.  U_out is the f64
 * iterate rounded to fp32 once.
 * Outputs: objective [rows][2] = {f at the start, f at the returned row}; grad_ratio [rows] = |g|_2 / (l2 |u|_inf) at
 * the returned row; iters_status [rows][2] = {iterations, status}; info [rows][d][d] = sum_{e<l} w_el sigmoid'(a_e - a_l)
 * (v~_e - v~_l)(v~_e - v~_l)^T at the returned row, without coef and ridge ([p][q] and [q][p] bit-equal; one more Hessian
 * pass, taken only when info is not NULL; with max_newton = 0 the information at the start row).  objective, grad_ratio
 * and info may be NULL, and a row's other outputs do not depend on it.
 * Statuses: 0 certified; 1 stopped (iteration cap, or no Armijo decrease); 2 invalid data: offsets that are not
 * 0 <= row_off[r] <= row_off[r+1] <= entries, an idx outside [0, m), a non-finite x, V row or U_init row — all checked
 * before any gather, no address is formed from a bad index or offset — the row, its objective, grad_ratio and info
 * are NaN, 0 iterations; 3: the row is longer than mfcd_ratings_fold_in_max_len(), outputs as for 2, nothing of the row
 * is read.  A row without a supporting pair (L < 2; under the skip flag all x equal) is answered in closed form: row
 * +0, status 0, 0 iterations, objective {(l2 / 2) |U_init[r]|^2, 0}, grad_ratio 0, info +0.
 * One 256-thread workgroup owns a row from start to finish; no floating-point atomics, every sum has one owner and a
 * fixed order that depends on the row alone: two calls are bit-equal and a row's outputs do not depend on the other
 * rows or on its position.  No allocation and no host wait.
 * mfcd_ratings_fold_in_max_len() = 3072: one workgroup takes a whole row, and a very long row would hold a compute unit
 * for a long time.  Measured on one MI355X (profiles/ratings_fold_in.txt, one row of 1024 entries, d = 64): a Hessian
 * pass runs at 0.34 G ordered pairs/s on its compute unit and a value-and-gradient pass at 0.52 G/s, 4.9 ns per ordered
 * pair for an iteration of one pass each; a row of 3072 entries at max_newton = 20 then takes 3072^2 x 20 x 4.9 ns =
 * 0.92 s, one of 4096 entries 1.6 s.  It is not a tuning knob.
 * workspace: mfcd_ratings_fold_in_workspace_bytes(rows, d, entries) = 256 whatever the sizes (0 = sizes out of range):
 * a row's state lives in its workgroup's LDS and nothing is staged in HBM; calls of more than 2^20 rows go through in
 * launches of 2^20.
 * Limits: 1 <= d <= mfcd_ratings_fold_in_max_d() = 64, m >= 1, rows >= 0 (0 = success, nothing launched), entries >= 0,
 * flags 0 or MFCD_RAGGED_SKIP_TIES, scale finite as a float, coef and l2 finite and > 0, gtol finite and >= 0,
 * 0 <= max_newton <= 1000, V, row_off, U_out and iters_status not NULL, idx and x where entries > 0, U_out and info
 * overlapping none of V, idx, x, row_off, U_init nor each other; MFCD_EINVAL outside them and MFCD_EWORKSPACE for a short
 * workspace, both before anything touches the device.
 */
int mfcd_ratings_fold_in_max_d(void);
int mfcd_ratings_fold_in_max_len(void);
size_t mfcd_ratings_fold_in_workspace_bytes(int rows, int d, int64_t entries);
int mfcd_ratings_fold_in_users(const float *V, int m, int d, const int32_t *idx, const float *x, int64_t entries,
                               const int64_t *row_off, int rows, double scale, int flags, double coef, double l2,
                               const float *U_init, int max_newton, double gtol, float *U_out, double *objective,
                               double *grad_ratio, int32_t *iters_status, double *info, void *workspace,
                               size_t workspace_bytes, void *stream);

/*
 * Where given columns of a row stand among the row's admissible columns (no reference counterpart): the rank of every
 * held-out entry in the user's full ordered list of items, training items barred — what recall@k, hit rate, NDCG@k, MRR
 * and AUC over the whole catalogue are computed from (mfcd/ranking.py).  Nothing is sorted and nothing n x m is formed.
 * Scores as mfcd_topk_rows takes them: X [n][ldx] fp32, or (X == NULL) A [n][d] . B [m][d], 1 <= d <= MFCD_MAX_D, through
 * the same fp32 MFMA kernel and the same bounded slab of whole score rows, so every score is formed once and is the number
 * mfcd_topk_rows compares.  row_ids: `rows` row numbers (device), any order, repeats allowed; NULL = rows 0 .. rows-1.
 * Two CSR lists are indexed by requested row r:
 *   tgt_off int64 [rows+1], tgt_items int32 [entries]          the columns to rank, in any order, repeats allowed
 *   excl_off int64 [rows+1], excl_items int32 [excl_entries]   the row's barred columns, strictly ascending; both NULL =
 *                                                              nothing is barred
 * Order: mfcd_topk_rows' `best` order — key = ~sortable_key(score), -0.0 equals +0.0, NaN above +inf, equal keys by
 * ascending column: a total order on (key, column).  A column is admissible for a row when it is not barred there.
 *   rank [entries]        the number of admissible columns c != t of the row that precede the entry's column t: the
 *                         position t has in mfcd_topk_rows' list under the same exclusion list
 *   ties [entries]        the number of admissible c != t whose key equals t's
 *   score [entries]       nullable; the score that was compared
 *   admissible [rows]     m minus the number of the row's barred columns
 *   status [rows]         0, or 2: invalid data
 * An entry whose own column is barred for its row gets rank -1 and ties -1 (its score is still the column's); the row's
 * other targets are ordinary admissible columns, and a repeated target gets equal results.
 * Status 2: offsets that are not 0 <= off[r] <= off[r+1] <= entries (excl_entries), a target or barred column outside
 * [0, m), a barred list that is not strictly ascending, a row id outside [0, n), or more than 1 048 576 targets in the row
 * — all checked before anything is gathered, and no address is formed from a value that failed.  The row's admissible is
 * -1 and, where its target offsets are valid, its entries are rank -1, ties -1, score NaN; other rows are unaffected.
 * Entries that lie in no valid row's slice are not written.  The rows' target slices are taken to be disjoint (the rows of
 * one CSR list, or repeats of a row with a copy of its slice): an entry shared by two rows would receive both rows' counts.
 * All accumulation is integer (a key comparison per (target, column), counts added by integer atomics into outputs the
 * entry initialises itself): two calls are bit-equal, and a row's outputs depend neither on the other rows, nor on its
 * position in the call, nor on where a slab ends.  No allocation and no host wait.
 * Limits: rows >= 0 and entries >= 0 (0 of either is success; with rows > 0, admissible and status are still written),
 * 1 <= m <= 4 194 304, n >= 1, pointers present where the counts are positive, excl_off and excl_items both or neither,
 * outputs overlapping neither the inputs nor each other; MFCD_EINVAL outside them and MFCD_EWORKSPACE for a short
 * workspace, both before anything touches the device.
 * workspace: factor mode, mfcd_rank_entries_workspace_bytes(rows, m, d, entries) bytes, 256-byte aligned: the slab, at
 * most 128 MiB (at least 128 rows), whatever n and entries are; 0 = sizes out of range (d = 0 included).  The dense mode
 * needs none (NULL, 0).
 */
size_t mfcd_rank_entries_workspace_bytes(int rows, int m, int d, int64_t entries);
int mfcd_rank_entries(const float *X, int64_t ldx, const float *A, const float *B, int d, const int32_t *row_ids, int rows,
                      int n, int m, const int64_t *tgt_off, const int32_t *tgt_items, int64_t entries,
                      const int64_t *excl_off, const int32_t *excl_items, int64_t excl_entries, int32_t *rank,
                      int32_t *ties, float *score, int32_t *admissible, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream);

/*
 * The exact observed-versus-unobserved logistic risk of rows of a score matrix (no reference counterpart): what a model
 * trained on implicit feedback (clicks, purchases, "rated at all") minimises, and the logistic surrogate of the per-user
 * AUC that mfcd/ranking.py reports (mfcd/implicit.py).  For a requested row with observed columns P, barred columns E and
 * N = [0, m) \ (P u E), over all |P \ E| |N| pairs exactly (BPR without the sampling), a = the row's scores:
 *   R = sum over i in P \ E, j in N of softplus(a_j - a_i)
 * Scores, row_ids, rows, n, m as mfcd_rank_entries takes them (dense X [n][ldx], or X == NULL and A [n][d] . B [m][d]
 * through the same fp32 MFMA kernel and bounded slab, so the numbers compared are those mfcd_topk_rows and
 * mfcd_rank_entries compare).  Two CSR lists are indexed by requested row r, both strictly ascending within a row:
 *   pos_off int64 [rows+1], pos_items int32 [entries]          the row's observed columns
 *   excl_off int64 [rows+1], excl_items int32 [excl_entries]   the row's barred columns; both NULL = nothing is barred
 * coef: nullable fp32 [rows], the factor of the row's gradient; NULL = 1.
 *   status [rows]       0, or 2: invalid data
 *   counts [rows][4]    int64: pos = |P \ E|, neg = |N|, inverted = the pairs (i, j) whose j precedes i in mfcd_topk_rows'
 *                       `best` order (key = ~sortable_key(score), -0.0 equals +0.0, NaN above +inf, equal keys by ascending
 *                       column), tied = the pairs with equal keys
 *   sums [rows]         f64: R, in natural log.  NULL = the prepare pass alone: status, pos and neg are written (inverted
 *                       and tied as 0), no score is read, X, A, B, g and the workspace may be NULL
 *   g [rows][ldg]       nullable fp32: the gradient of coef_r R_r with respect to the score row, columns [0, m): a negative
 *                       column j gets coef sum_{i in P \ E} sigma(a_j - a_i), a positive column i gets
 *                       -coef sum_{j in N} sigma(a_j - a_i), a barred column 0.  Every one of the m elements of every
 *                       requested row is written: the caller passes uninitialised memory.
 * Status 2: offsets that are not 0 <= off[r] <= off[r+1] <= entries (excl_entries), an item outside [0, m), a list that is
 * not strictly ascending, a row id outside [0, n), or more than 1 048 576 observed columns in the row — all checked before
 * anything is gathered, and no address is formed from a value that failed.  Such a row gets counts -1, sum NaN and a NaN
 * gradient row; other rows are unaffected.
 * A score that is inf or NaN at a column that is not barred: sum NaN and an all-NaN gradient row, status 0 (the pair
 * gradients' rule); the integer counts still follow the key order.  Scores at barred columns are never used.
 * Deterministic: no floating-point atomic, every float sum has one owner and a fixed order, every fp32 run is at most 64
 * terms before it is added to an f64 sum; sigma and softplus come from exp(-|v|) only, one exp and one reciprocal per pair.
 * Two calls are bit-equal, and a row's outputs depend neither on the other rows, nor on its position in the call, nor on
 * where a slab ends.  No allocation and no host wait.
 * Limits: rows >= 0 (0 is success), entries >= 0, 1 <= m <= 4 194 304, n >= 1, 1 <= d <= MFCD_MAX_D in factor mode,
 * ldx >= m, ldg >= m, pointers present where the counts are positive, excl_off and excl_items both or neither, outputs
 * overlapping neither the inputs nor each other; MFCD_EINVAL outside them, MFCD_EALIGN for a misaligned pointer and
 * MFCD_EWORKSPACE for a short workspace, all before anything touches the device.
 * workspace: mfcd_implicit_rows_workspace_bytes(rows, m, d) bytes (d = 0: the dense mode), 256-byte aligned: the factor
 * mode's slab (at most 128 MiB, at least 128 rows) and the per-(row, chunk) partials of one block of rows (at most
 * 40 MiB); 0 = sizes out of range.  mfcd_implicit_chunk(): the columns per workgroup of the column pass;
 * mfcd_implicit_tile(): the observed columns per tile.
 */
int mfcd_implicit_chunk(void);
int mfcd_implicit_tile(void);
size_t mfcd_implicit_rows_workspace_bytes(int rows, int m, int d);
int mfcd_implicit_rows(const float *X, int64_t ldx, const float *A, const float *B, int d, const int32_t *row_ids, int rows,
                       int n, int m, const int64_t *pos_off, const int32_t *pos_items, int64_t entries,
                       const int64_t *excl_off, const int32_t *excl_items, int64_t excl_entries, const float *coef,
                       int64_t *counts, double *sums, float *g, int64_t ldg, int32_t *status, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * The Hessian of mfcd_implicit_rows' risk with respect to the score row, applied to a direction (no reference
 * counterpart; mfcd/implicit.py, mfcd/implicit_exact.py).  Rows, lists, coef, status and limits as mfcd_implicit_rows takes
 * them.  For a requested row with scores a, direction y and the weights
 *   w_ij = sigma(a_j - a_i) sigma(a_i - a_j)   for i in P \ E, j in N
 * the outputs are a bipartite weighted Laplacian applied to y, and its diagonal:
 *   q [rows][ldq]       fp32, columns [0, m): a positive column i gets coef sum_{j in N} w_ij (y_i - y_j), a negative
 *                       column j gets coef sum_{i in P \ E} w_ij (y_j - y_i), a barred column 0
 *   deg [rows][ldd]     nullable fp32: coef times the sum of w over the column's partners (the Jacobi preconditioner of
 *                       a solve with the operator); a barred column 0.  q does not depend on whether deg is asked for.
 * Every one of the m elements of every requested row is written: the caller passes uninitialised memory.
 * Scores and direction both come dense — X [n][ldx], Y [n][ldy], addressed by row id; A, B, Ay, By NULL — or both by
 * factors of one width d — X == Y == NULL, scores A [n][d] . B [m][d], direction Ay [n][d] . By [m][d], each through
 * mfcd_topk_rows' score kernel into a bounded slab of its own, in blocks of rows; nothing n x m is formed.  Inputs may
 * alias one another (a user step passes B == By, an item step A == Ay).
 * The difference of the direction is formed per pair: a constant direction row gives q exactly +0, as does a row with
 * pos neg = 0.  Status 2 (see mfcd_implicit_rows): NaN rows of q and deg.  A score or a direction that is inf or NaN at
 * a column that is not barred: NaN rows of q and deg, status 0; values at barred columns are never used.
 * Deterministic: no atomic, one writer per output, fp32 runs of at most 64 terms before an f64 sum, one exp and one
 * reciprocal per pair and pass.  Two calls are bit-equal, and a row's outputs depend neither on the other rows, nor on
 * its position in the call, nor on where a slab ends.  No allocation and no host wait.
 * MFCD_EINVAL, MFCD_EALIGN and MFCD_EWORKSPACE as for mfcd_implicit_rows, before anything touches the device.
 * workspace: mfcd_implicit_hvp_rows_workspace_bytes(rows, m, d) bytes (d = 0: the dense mode), 256-byte aligned: the two
 * slabs of the factor mode and one int32 per (row, chunk) of a block of rows; 0 = sizes out of range.
 */
size_t mfcd_implicit_hvp_rows_workspace_bytes(int rows, int m, int d);
int mfcd_implicit_hvp_rows(const float *X, int64_t ldx, const float *Y, int64_t ldy, const float *A, const float *B,
                           const float *Ay, const float *By, int d, const int32_t *row_ids, int rows, int n, int m,
                           const int64_t *pos_off, const int32_t *pos_items, int64_t entries, const int64_t *excl_off,
                           const int32_t *excl_items, int64_t excl_entries, const float *coef, float *q, int64_t ldq,
                           float *deg, int64_t ldd, int32_t *status, void *workspace, size_t workspace_bytes,
                           void *stream);

/*
 * The exact user step on implicit feedback in one launch (no reference counterpart): what mfcd/implicit_exact.py's
 * implicit_user_step computes with a chain of small launches per Newton iteration; the serving-time fold-in of a user
 * who was not in training.  The two CSR lists are mfcd_implicit_rows': pos_off / pos_items the row's observed columns,
 * excl_off / excl_items its barred columns (both NULL = nothing is barred), both strictly ascending within a row.  With
 * P = observed \ barred, N = [0, m) \ (observed u barred) and V [m][d] fixed, U_out[r] minimises
 *     f(u) = coef_r * sum over i in P, j in N of softplus(a_j - a_i) + (l2 / 2) |u|^2,   a_c = u . v_c.
 * coef: f64 [rows] on the device, NULL = 1.  U_init = NULL starts every row at 0 and is bit-equal to a zero U_init.
 * Algorithm (mfcd/population.py's _newton with solver "direct", per row; tests/implicit_foldin_model.py restates it):
 *   1. u = U_init[r] or 0, t = 1, iterations = 0.
 *   2. g = coef (sum_j g_j v~_j - sum_i G_i v~_i) + l2 u, g_j = sum_i sigmoid(a_j - a_i), G_i = sum_j sigmoid(a_j - a_i).
 *      |g|_2 <= gtol l2 |u|_inf: status 0.  Otherwise iterations == max_newton: status 1.
 *   3. If u moved since the direction was formed, or there is none yet:
 *      H = coef sum_{i,j} sigmoid'(a_i - a_j)(v~_i - v~_j)(v~_i - v~_j)^T + l2 I, p = -H^{-1} g by Cholesky in LDS; a
 *      pivot that is not positive: p = -g / mean(diag H).
 *   4. f_t = f(u + t p), iterations += 1.  f_t <= f + 1e-4 t (g . p) (a NaN f_t fails): u += t p, t = min(2 t, 1).
 *      Otherwise t /= 2, the direction is kept, and t < 2^-12 ends the row with status 1.  Back to 2.
 *      The inequality is taken on the two values of f; when that fails, on the decrease f(u + t p) - f(u) summed pair
 *      by pair (softplus(a + h) - softplus(a) = log1p(sigmoid(a) expm1(h)) for |h| < 1), which resolves decreases below
 *      the fp32 rounding of f itself.  Either evaluation accepts, as in mfcd_ratings_fold_in_users; the second is
 *      evaluated only when the first fails, which decides the same thing.  It changes the outcome where coef times the
 *      risk (fp32) outweighs the ridge part (f64) of f; where the ridge dominates, the values alone decide the same.
 * The sum of step 3 is formed by its bipartite structure, with w_ij = sigmoid'(a_i - a_j), D_i = sum_j w_ij,
 * D_j = sum_i w_ij, y_j = sum_i w_ij v~_i:  (T + T^T) / 2,  T = sum_i v~_i (D_i v~_i)^T + sum_j v~_j (D_j v~_j - 2 y_j)^T.
 * Precision: u, g, H, the solves, f and every dot product over d are f64.  v~_c is V[c] minus the f64 mean of the rows
 * of V that P names, rounded to fp32 once (everything above depends on differences of the v_c only); a_c is an f64 chain
 * over k rounded to fp32 once, formed again from V in every pass: nothing per column is kept.  The pair arithmetic is
 * fp32, csrc/pairs_common.h's, in runs of at most 64 terms widened to f64; y_j is formed per column in fp32 runs of 64
 * positives on the vector pipe, widened to f64, and D_j v~_j - 2 y_j is rounded to fp32 once; T is added in f64.  U_out
 * is the f64 iterate rounded to fp32 once.
 * Outputs, as mfcd_ratings_fold_in_users': objective [rows][2] = {f at the start, f at the returned row}; grad_ratio
 * [rows] = |g|_2 / (l2 |u|_inf) at the returned row; iters_status [rows][2] = {iterations, status}; info [rows][d][d] =
 * the sum of step 3 at the returned row, without coef and ridge ([p][q] and [q][p] bit-equal; one more Hessian pass,
 * taken only when info is not NULL; with max_newton = 0 the information at the start row).  objective, grad_ratio and
 * info may be NULL, and a row's other outputs do not depend on it.
 * Statuses: 0 certified; 1 stopped (iteration cap, or no Armijo decrease); 2 invalid data: offsets that are not
 * 0 <= off[r] <= off[r+1] <= entries (excl_entries), an item outside [0, m), a list that is not strictly ascending, a
 * non-finite V row of an admissible column, a non-finite U_init row, a coef that is not finite and positive — the lists
 * are checked before any gather, no address is formed from a value that failed — the row, its objective, grad_ratio
 * and info are NaN, 0 iterations; 3: more than mfcd_implicit_fold_in_max_pos() admissible positives, or |P| |N| above
 * mfcd_implicit_fold_in_max_pairs(): outputs as for 2.  Status 3 is decided from the list lengths wherever they decide
 * it (always when nothing is barred: at least pos_len - excl_len positives, m - pos_len - excl_len negatives), and then
 * nothing of the row beyond them is read; otherwise from the counts, after the lists were checked.  A row with
 * |P| |N| = 0 is answered in closed form: row +0, status 0, 0 iterations, objective {(l2 / 2) |U_init[r]|^2, 0},
 * grad_ratio 0, info +0.
 * One 256-thread workgroup owns a row from start to finish; threads own columns, in stages of
 * mfcd_implicit_fold_in_chunk() = 2048 columns; no floating-point atomics, every sum has one owner and a fixed order
 * that depends on the row alone: two calls are bit-equal and a row's outputs depend neither on the other rows, nor on
 * its position, nor on which optional outputs are asked for.  No allocation and no host wait.
 * Caps: mfcd_implicit_fold_in_max_pos() = 4608 (16 bytes of LDS per admissible positive);
 * mfcd_implicit_fold_in_max_pairs() = 11 534 336 (11 x 2^20): one workgroup takes a whole row, and a row at the cap
 * should stay under a second at max_newton = 20.  Measured on one MI355X (profiles/implicit_fold_in.txt, one row of
 * 1024 observed items among 8192, d = 64): a value-and-gradient pass runs at 2.28 G pairs/s on its compute unit and a
 * Hessian pass at 0.270 G pairs/s, 4.15 ns per pair for an iteration of one pass each, so a row at the cap takes
 * 11 534 336 x 20 x 4.15 ns = 0.96 s (2^24 pairs: 1.39 s).  It is not a tuning knob.  implicit_user_step takes rows of
 * any size.  The cap bounds the pair work only: every pass also re-forms m scores of width d from V, about five times
 * per iteration, which no cap bounds — a short row in a very large catalogue is not held under a second by it (10
 * observed items of 65 536 at d = 64: 129 ms for 256 rows side by side, nearly all of it scoring).
 * workspace: mfcd_implicit_fold_in_workspace_bytes(rows, m, d) = 256 whatever the sizes (0 = sizes out of range): a
 * row's state lives in its workgroup's LDS; calls of more than 2^20 rows go through in launches of 2^20.
 * Limits: 1 <= d <= mfcd_implicit_fold_in_max_d() = 64, 1 <= m <= 4 194 304, rows >= 0 (0 = success, nothing launched),
 * entries >= 0, excl_off and excl_items both or neither (excl_entries 0 without them), l2 finite and > 0, gtol finite and
 * >= 0, 0 <= max_newton <= 1000, V, pos_off, U_out and iters_status not NULL, pos_items where entries > 0, the outputs
 * overlapping none of the inputs nor each other; MFCD_EINVAL outside them and MFCD_EWORKSPACE for a short workspace,
 * both before anything touches the device.
 */
int mfcd_implicit_fold_in_max_d(void);
int mfcd_implicit_fold_in_max_pos(void);
int64_t mfcd_implicit_fold_in_max_pairs(void);
int mfcd_implicit_fold_in_chunk(void);
size_t mfcd_implicit_fold_in_workspace_bytes(int rows, int m, int d);
int mfcd_implicit_fold_in_users(const float *V, int m, int d, const int64_t *pos_off, const int32_t *pos_items,
                                int64_t entries, const int64_t *excl_off, const int32_t *excl_items, int64_t excl_entries,
                                int rows, const double *coef, double l2, const float *U_init, int max_newton, double gtol,
                                float *U_out, double *objective, double *grad_ratio, int32_t *iters_status, double *info,
                                void *workspace, size_t workspace_bytes, void *stream);

/*
 * The Plackett–Luce loss of ranked lists and its gradient in the scores, over ragged rows (no reference counterpart: the
 * reference's BTL triplet is a list of two).  CSR layout as mfcd_pair_ragged_stats: row r owns entries
 * [row_off[r], row_off[r + 1]) of a [entries], the model's scores of the L items shown to it, in rank order, best first.
 * depth [rows] int32 (NULL: every row fully ranked) is the number of ranked positions, 0 <= depth <= L: the entries past
 * it are an unordered tail, shown and not ranked.  stages = min(depth, L - 1): the choice out of one item carries
 * nothing.  Per row, with k, l counted from 0,
 *     lse_k = log sum_{l >= k} exp(a_l)
 *     loss  = sum_{k < stages} (lse_k - a_k)                       the negative log-likelihood of the stages' choices
 *     g_l   = sum_{k <= l, k < stages} exp(a_l - lse_k) - [l < stages]         its gradient in a_l
 *     hits  = the stages k with a_k >= a_l for every l >= k         (the choices the model would have made; ties count)
 *   what     bit 1: loss [rows] f64 and counts [rows][2] int64 = (stages, hits); bit 2: g [entries] fp32.
 *   status   [rows] int32: 0, or 2 for a row that fails validation.
 * Arithmetic.  Both sums are scans over the log-sum-exp monoid: lse is a reverse scan of a, and with
 * N_l = log sum_{k <= l, k < stages} exp(-lse_k), a forward scan, g_l = exp(a_l + N_l) - [l < stages].  An element is a
 * (max, sum scaled by exp(-max)) pair in f64, joined as an online softmax joins them, so every exponent is <= 0: nothing
 * overflows, and no suffix sum underflows to 0 however far apart the scores lie (exp(a - row max) followed by a plain
 * suffix sum does, for exactly the confident, well-fitted rows).  A pair stays a pair to the end: exp(-lse_k) enters the
 * forward scan as (-max_k, 1 / sum_k), the loss term is (max_k - a_k) + log sum_k, g_l = exp(a_l + M_l) S_l - [l < stages].
 * exp, log and the sums are f64; g is rounded to fp32 once.  tests/list_pl_model.py is the same function in numpy
 * (np.logaddexp.accumulate in both directions; it folds each pair into one f64, so it loses the log of a count next to
 * a score of the size of 1e17 or more, where the kernel does not).
 * Tiles.  A row is cut into tiles of TILE = mfcd_list_pl_tile() = 256 entries; the caller passes tile_off [rows + 1], the
 * prefix sum of ceil(L_r / TILE), and its total n_tiles (the host cannot see row_off, and the entry has no host wait).  A
 * first kernel validates every row before any entry of it is read: 0 <= row_off[r] <= row_off[r + 1] <= entries,
 * L <= 1 048 576, 0 <= depth[r] <= L, tile_off[r + 1] - tile_off[r] = ceil(L / TILE) inside [0, n_tiles], and every tile
 * of the row found by the binary search over tile_off.  Then one 256-thread workgroup per tile, one entry per thread.  A
 * row of one tile does both scans in its workgroup.  A longer row (a full catalogue is one row) is reduced, then
 * scanned: the tiles' reverse aggregates, a one-wave pass per row that turns them into carries, a tile pass that forms
 * lse_k, the tile's loss and hit partials and its forward aggregate, a second one-wave pass that forms the forward
 * carries and adds the row's partials in tile order, and the tile pass that writes g.  Every dependency is a kernel
 * boundary: no workgroup waits on another.  No floating-point atomics, every sum has one owner and a fixed order that
 * depends on the row alone: two calls are bit-equal, what = 1 / what = 2 are bit-equal to the matching half of what = 3,
 * and a row's outputs do not depend on the other rows of the call or on its position in it.
 * Rows.  A row that fails validation gets status 2, a NaN loss, counts -1 and none of its entries of g written; no address
 * is formed from its offsets.  A row with a non-finite score gets a NaN loss, counts -1, an all-NaN slice of g and status
 * 0; the other rows are untouched.  L <= 1 or depth 0 gives a +0 loss, counts (0, 0) and +0 in g.
 * Limits: rows >= 0 (0 = success, nothing launched), entries >= 0, 0 <= n_tiles <= 2^40, what in {1, 2, 3} with its
 * outputs present (g where entries > 0, and not a), a where entries > 0, row_off, tile_off and status; MFCD_EINVAL
 * outside them and MFCD_EWORKSPACE for a short workspace, before anything touches the device.  workspace:
 * mfcd_list_pl_workspace_bytes(rows, n_tiles), 88 bytes per tile and 4 per row, each region rounded up to 256 (0 = sizes
 * out of range), 256-byte aligned; launches are cut to 2^20 workgroups.  No allocation and no host wait.
 */
int mfcd_list_pl_tile(void);
size_t mfcd_list_pl_workspace_bytes(int rows, int64_t n_tiles);
int mfcd_list_pl(const float *a, int64_t entries, const int64_t *row_off, const int32_t *depth, int rows,
                 const int64_t *tile_off, int64_t n_tiles, int what, double *loss, int64_t *counts, float *g,
                 int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The Hessian of mfcd_list_pl's loss in the scores, applied to a score-space vector y [entries], and its diagonal: the
 * second-order twin of mfcd_list_pl on the same layout (a, row_off, depth, tile_off, n_tiles as there; no reference
 * counterpart).  Per row, with p_{k,l} = exp(a_l - lse_k) for l >= k, the softmax of stage k over what remains,
 *     ybar_k = sum_{j >= k} p_{k,j} y_j                                     a softmax-weighted mean: |ybar_k| <= max |y|
 *     q_l    = sum_{k <= l, k < stages} p_{k,l} (y_l - ybar_k)              H y, H = sum_k (diag(p_k) - p_k p_k^T)
 *     deg_l  = sum_{k <= l, k < stages} p_{k,l} (1 - p_{k,l})               H_ll >= 0
 *   q        [entries] fp32.  deg [entries] fp32 or NULL: the diagonal is formed only where it is asked for.
 *   status   [rows] int32: 0, or 2 for a row that fails validation.
 * Arithmetic.  The gradient's two scans over the same monoid with a linear payload riding along.  The reverse scan joins
 * (a_j, 1, y_j) into (m_k, s_k, t_k), t_k = sum_{j >= k} exp(a_j - m_k) y_j: s and t are scaled by the same factor in
 * every join (one exp per join, as in mfcd_list_pl), and ybar_k = t_k / s_k.  The forward scan joins the stages'
 * (-m_k, 1 / s_k, ybar_k / s_k) into (M_l, S_l, W_l): q_l = exp(a_l + M_l) (y_l S_l - W_l), the exponent <= 0.  The
 * diagonal takes a second forward scan, of (-2 m_k, 1 / s_k^2) into (M2_l, S2_l):
 * deg_l = exp(a_l + M_l) S_l - exp(2 a_l + M2_l) S2_l, held at 0 from below.  All of it f64, q and deg rounded to fp32
 * once; nothing under- or overflows for finite fp32 a and y.  m and s never see the payload, so deg does not depend on y
 * and q is bit-equal with and without deg.  tests/list_pl_hvp_model.py is the same function in numpy by another route.
 * Tiles, validation and the decomposition are mfcd_list_pl's: the status pass before any entry is read; a row of one tile
 * does everything in its workgroup in the last launch; a longer row goes through aggregate, carry, middle, carry and the
 * final pass, every dependency a kernel boundary, no workgroup waiting on another.  No floating-point atomics, every sum
 * has one owner and an order that depends on the row alone: two calls are bit-equal and a row's outputs do not depend on
 * the other rows of the call or on its position in it.
 * Rows.  A row that fails validation gets status 2 and none of its entries of q or deg written.  A row with a non-finite
 * score or a non-finite entry of y gets an all-NaN slice of q (and deg) and status 0; the other rows are untouched.
 * L <= 1 or depth 0 gives +0.
 * Limits: rows >= 0 (0 = success, nothing launched), entries >= 0, 0 <= n_tiles <= 2^40; a, y and q where entries > 0;
 * q is neither a nor y, deg none of q, a, y; row_off, tile_off and status; MFCD_EINVAL outside them and MFCD_EWORKSPACE
 * for a short workspace, before anything touches the device.  workspace: mfcd_list_pl_hvp_workspace_bytes(rows, n_tiles),
 * 136 bytes per tile and 4 per row, each region rounded up to 256 (0 = sizes out of range), 256-byte aligned; launches
 * are cut to 2^20 workgroups.  No allocation and no host wait.
 */
size_t mfcd_list_pl_hvp_workspace_bytes(int rows, int64_t n_tiles);
int mfcd_list_pl_hvp(const float *a, const float *y, int64_t entries, const int64_t *row_off, const int32_t *depth,
                     int rows, const int64_t *tile_off, int64_t n_tiles, float *q, float *deg, int32_t *status,
                     void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MFCD_H */
