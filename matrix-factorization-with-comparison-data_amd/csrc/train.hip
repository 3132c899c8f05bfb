// train.hip — the fused-step entry of the C-ABI (mfcd_train_steps*, mfcd_train_call_*): registered workspaces (layout,
// registry, pinned staging ring), the knobs, and the choice between the streaming (streaming.hip), resident
// (resident.hip) and local (local.hip) forms; also the batched local form and the multi-model eval pass, which share the
// workspace registry.
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "train_common.h"

namespace {

int g_train_path = 0;  // 0 auto, 1 streaming, 2 resident, 3 local (mfcd_set_train_path)

int device_cus()
{
    static int cached = 0;
    if (!cached) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            cached = cus;
        else {
            (void)hipGetLastError();
            cached = 256;  // MI355X
        }
    }
    return cached;
}

constexpr size_t kColdBytes = sizeof(mfcd_detail::ResidentCold);  // directly in front of the scalar table
constexpr size_t kDbgBytes = 256 + 2 * 16 * 256 * 8 * 8;  // [8] who gave up first + 2 banks of [<=4096 waves][8] u64 of the diagnostic builds (tools/)
constexpr size_t kMaxMailboxBytes = (size_t)24 << 30;  // beyond this the resident form is not planned
constexpr int kTagStepBits = 21;    // granule tag = launch id << 21 | (step + 1)
constexpr unsigned kMaxLaunchId = (1u << (32 - kTagStepBits)) - 1;

// Fixed carve-up of a registered workspace (mfcd_train_workspace_init), a function of the CAPACITY it was planned for:
//   status | dbg | stage (ResidentCold + K_cap+1 step scalars) | terms [N_cap] (8-byte tagged granules) | event-list
//   counters (resident; kept all-zero between launches) | event-list entries |
//   { U_alt, V_alt (streaming) } overlapping { translated samples, mailbox (resident) }
// Every call with N <= N_cap and ceil(N/B) <= K_cap uses these offsets, so nothing has to be re-initialised per call.
// the regions the prologue kernel writes: stage table, list counters, list entries, translated samples
struct PrologueRegions { size_t stage_off, evcnt_off, event_off, xs_off; };

struct TrainLayout {
    size_t dbg_off, stage_bytes, terms_off, evcnt_bytes, event_bytes;
    size_t ualt_off, valt_off, mailbox_off, mailbox_bytes, total;
    size_t alt_end;  // end of the streaming members of the union (U_alt, V_alt)
    // set[0] sits in the carve-up above; set[1] (two_sets only, behind everything else) lets a call's prologue be STAGED
    // on a side stream under the previous call's step kernel (mfcd_train_call_stage)
    PrologueRegions set[2];
    bool two_sets;
    int64_t K_cap;
    int64_t nch_cap;                    // chunks per wave of the event lists
    mfcd_detail::ResidentEvents ev;     // geometry of the event lists (tshift 0: none)
    bool resident;   // the resident regions exist
};

TrainLayout train_layout(int64_t N_cap, int B, int n, int m, int d)
{
    TrainLayout L{};
    const int64_t Nc = N_cap > 0 ? N_cap : 1;
    L.K_cap = (Nc + B - 1) / B;
    size_t off = kStatusBytes;
    L.dbg_off = off;
    off += kDbgBytes;
    L.set[0].stage_off = off;
    L.stage_bytes = kColdBytes + sizeof(StepScalars) * (size_t)(L.K_cap + 1);   // one pad entry: the kernel reads step k+1
    off += align_up(L.stage_bytes);
    L.terms_off = off;
    off += align_up(sizeof(unsigned long long) * (size_t)Nc);
    L.mailbox_bytes = sizeof(unsigned long long) * (size_t)Nc * 3 * (size_t)d;
    // any slice at all (geometry only: the layout must not depend on a tuning knob)
    L.resident = mfcd_detail::resident_slices(n, m, d, device_cus()).count > 0 && L.mailbox_bytes <= kMaxMailboxBytes &&
                 L.K_cap < ((int64_t)1 << 31) - 64;
    L.ev = L.resident ? mfcd_detail::resident_events(B, n, m, d, device_cus()) : mfcd_detail::ResidentEvents{0, 0, 0};
    L.nch_cap = L.ev.tshift ? mfcd_detail::resident_event_chunks(L.K_cap, L.ev.tshift) : 0;
    L.set[0].evcnt_off = off;
    L.evcnt_bytes = sizeof(unsigned) * (size_t)L.ev.waves * (size_t)L.nch_cap;
    off += align_up(L.evcnt_bytes);
    L.set[0].event_off = off;
    L.event_bytes = (size_t)16 * mfcd_detail::kResidentEventCap * (size_t)L.ev.waves * (size_t)L.nch_cap;
    off += align_up(L.event_bytes);
    // streaming members of the union
    size_t a_off = off;
    L.ualt_off = a_off;
    a_off += align_up(sizeof(float) * (size_t)n * d);
    L.valt_off = a_off;
    a_off += align_up(sizeof(float) * (size_t)m * d);
    // resident members of the union
    size_t b_off = off;
    L.set[0].xs_off = b_off;
    L.mailbox_off = b_off;
    if (L.resident) {
        b_off += align_up(sizeof(mfcd_sample) * (size_t)Nc);
        L.mailbox_off = b_off;
        b_off += align_up(L.mailbox_bytes);
    }
    L.alt_end = a_off;
    L.total = a_off > b_off ? a_off : b_off;
    L.two_sets = L.resident && L.ev.tshift != 0;
    if (L.two_sets) {
        size_t c = align_up(L.total);
        L.set[1].stage_off = c; c += align_up(L.stage_bytes);
        L.set[1].evcnt_off = c; c += align_up(L.evcnt_bytes);
        L.set[1].event_off = c; c += align_up(L.event_bytes);
        L.set[1].xs_off = c; c += align_up(sizeof(mfcd_sample) * (size_t)Nc);
        L.total = c;
    }
    return L;
}

// ---- registered workspaces: the host-side state that belongs to one caller-owned workspace ----
// (one per model / stream; replaces the process-wide staging buffer of round 1).  A workspace is driven by one host
// thread at a time; the registry itself is guarded.
constexpr int kStageSlots = 4;

struct StageSlot {
    void *host = nullptr;      // pinned
    void *devview = nullptr;   // the same memory as the device addresses it
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    // whoever reads the slot is on `st` by now: it is free again once the stream has passed this point
    int release(hipStream_t st)
    {
        MFCD_HIP_TRY(hipEventRecord(ev, st));
        pending = true;
        return 0;
    }
};

struct WsState {
    size_t bytes = 0;
    int device = 0;
    int64_t N_cap = 0;
    int B = 0, n = 0, m = 0, d = 0;
    TrainLayout L{};
    unsigned launch_id = 0;    // resident launches so far (mod kMaxLaunchId): the tag base of the next one
    // prologue staged ahead of its call (mfcd_train_call_stage): which call it belongs to and which set of regions it wrote.
    // The call is named by the inputs of what the prologue wrote: the samples it translated, the tables and loss buffer
    // its descriptor points at, and the lr / betas its step table was built from
    struct Staged {
        bool valid = false;
        const void *samples = nullptr, *U = nullptr;
        int64_t N = 0, step0 = 0;
        float *loss = nullptr;
        double lr = 0.0, beta1 = 0.0, beta2 = 0.0;
        int set = 0;
        bool same_call(const Staged &o) const
        {
            return samples == o.samples && U == o.U && N == o.N && step0 == o.step0 && loss == o.loss && lr == o.lr &&
                   beta1 == o.beta1 && beta2 == o.beta2;
        }
    } staged;
    int last_set = 0;             // set of regions the most recently enqueued persistent launch reads
    bool lists_dirty[2] = {false, false};   // a prologue filled this set's event lists and no launch has consumed them (the
                                  // launch zeroes the counters it read): a staged prologue whose call never came.  The
                                  // next prologue into the set zeroes the counters first instead of appending to them
    bool terms_dirty = false;     // a call that keeps plain fp32 terms (streaming / local / generic resident) wrote the term
                                  // region: zeroed before the next launch that reads it as tagged granules
    bool mailbox_dirty = false;   // a streaming-form call wrote U_alt / V_alt over the head of the mailbox (same union):
                                  // fp32 bit patterns there could pass for tagged granules, so the next resident launch
                                  // zeroes that prefix first
    StageSlot slot[kStageSlots];
    unsigned next = 0;

    // which set of prologue-written regions this call uses: the one its prologue was staged into (if this is the
    // staged call), the other one when staging now, else the set of the last launch (free again in stream order).
    // *hit: `call` is the staged call (only where may_hit)
    int claim_set(const Staged &call, bool may_hit, bool stage_only, bool *hit)
    {
        *hit = !stage_only && may_hit && staged.valid && staged.same_call(call);
        const int set = *hit ? staged.set : (stage_only ? 1 - last_set : last_set);
        if (!stage_only && staged.valid && staged.set == set && !*hit) staged.valid = false;   // overwritten below
        return set;
    }

    // in front of a prologue that fills this set's event lists (lists_dirty)
    int clear_lists(int set, char *base, hipStream_t st)
    {
        if (lists_dirty[set]) {
            MFCD_HIP_TRY(hipMemsetAsync(base + L.set[set].evcnt_off, 0, L.evcnt_bytes, st));
            lists_dirty[set] = false;
        }
        return 0;
    }

    // tag base of the next resident launch
    int next_tag_base(char *base, hipStream_t st, unsigned *tag_base)
    {
        if (launch_id >= kMaxLaunchId) {   // the launch ids wrap: forget every granule of the past, once
            MFCD_HIP_TRY(hipMemsetAsync(base + L.mailbox_off, 0, L.mailbox_bytes, st));
            MFCD_HIP_TRY(hipMemsetAsync(base + L.terms_off, 0, sizeof(unsigned long long) * (size_t)N_cap, st));
            launch_id = 0;
        }
        *tag_base = ++launch_id << kTagStepBits;
        return 0;
    }

    // in front of a resident launch (mailbox_dirty, terms_dirty)
    int clear_dirty(char *base, hipStream_t st)
    {
        if (mailbox_dirty) {
            if (L.alt_end > L.mailbox_off) {
                const size_t nb = L.alt_end - L.mailbox_off;
                MFCD_HIP_TRY(hipMemsetAsync(base + L.mailbox_off, 0, nb < L.mailbox_bytes ? nb : L.mailbox_bytes, st));
            }
            mailbox_dirty = false;
        }
        if (terms_dirty) {   // a form that keeps plain fp32 terms ran on this workspace: no stale bit pattern may
                             // pass for a tagged term
            MFCD_HIP_TRY(hipMemsetAsync(base + L.terms_off, 0, sizeof(unsigned long long) * (size_t)N_cap, st));
            terms_dirty = false;
        }
        return 0;
    }

    ~WsState()
    {
        for (auto &s : slot) {
            if (s.ev) (void)hipEventDestroy(s.ev);
            if (s.host) (void)hipHostFree(s.host);
        }
    }
};

std::mutex g_ws_mu;
std::unordered_map<void *, std::unique_ptr<WsState>> g_ws;

WsState *find_ws(void *workspace)
{
    std::lock_guard<std::mutex> lock(g_ws_mu);
    auto it = g_ws.find(workspace);
    return it == g_ws.end() ? nullptr : it->second.get();
}

// A staging slot nobody reads any more, at least `need` bytes.  Blocks only when kStageSlots calls of this workspace
// are still queued on the device (bounded run-ahead of the host), never behind the previous call.
int stage_reserve(StageSlot &s, size_t need);

int stage_acquire(WsState &S, size_t need, StageSlot **out)
{
    StageSlot &s = S.slot[S.next++ % kStageSlots];
    if (s.pending) {
        MFCD_HIP_TRY(hipEventSynchronize(s.ev));
        s.pending = false;
    }
    if (int rc = stage_reserve(s, need)) return rc;
    *out = &s;
    return 0;
}

// pinned memory and event of one slot (both are created when the workspace is initialised: a pinned allocation costs
// ~0.1-0.2 ms of host time, which must not land on a training call)
int stage_reserve(StageSlot &s, size_t need)
{
    if (!s.ev) MFCD_HIP_TRY(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (s.cap < need) {
        if (s.host) (void)hipHostFree(s.host);
        s.host = nullptr;
        s.cap = need < 4096 ? 4096 : need;
        // device-visible and coherent: the prologue kernel reads the slot directly over the host link
        if (hipHostMalloc(&s.host, s.cap, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            MFCD_HIP_TRY(hipHostMalloc(&s.host, s.cap, hipHostMallocDefault));
        }
        MFCD_HIP_TRY(hipHostGetDevicePointer(&s.devview, s.host, 0));
    }
    return 0;
}

}  // namespace

extern "C" int mfcd_set_train_path(int mode)
{
    if (mode < 0 || mode > 3) return MFCD_EINVAL;
    g_train_path = mode;
    return 0;
}

extern "C" int mfcd_set_resident_math(int fast)
{
    if (fast != 0 && fast != 1) return MFCD_EINVAL;
    mfcd_detail::g_resident_math = fast;
    return 0;
}

extern "C" int mfcd_set_tuning(int key, int64_t value)
{
    mfcd_detail::Tuning &t = mfcd_detail::g_tune;
    switch (key) {
        case MFCD_TUNE_RESIDENT_LOOKAHEAD:
            if (value < -1 || value == 1 || value > 16) return MFCD_EINVAL;
            t.lookahead = (int)value;
            return 0;
        case MFCD_TUNE_RESIDENT_SPIN_LIMIT:
            if (value < 0 || value > 0x7fffffff) return MFCD_EINVAL;
            t.spin_limit = value == 0 ? mfcd_detail::kSpinLimitDefault : (unsigned)value;
            return 0;
        case MFCD_TUNE_UVT_SPLIT: return mfcd_detail::set_uvt_split((int)value);
        case MFCD_TUNE_UVT_TARGET_WGS: return mfcd_detail::set_uvt_target_wgs((int)value);
        case MFCD_TUNE_UVT_MIN_STAGES: return mfcd_detail::set_uvt_min_stages((int)value);
        case MFCD_TUNE_SHARD_PIPELINE:
            if (value < 0 || value > 2) return MFCD_EINVAL;
            t.shard_pipeline = (int)value;
            return 0;
        default: return MFCD_EINVAL;
    }
}


extern "C" size_t mfcd_train_workspace_bytes(int64_t N, int B, int n, int m, int d)
{
    if (N < 0 || B <= 0 || n <= 0 || m <= 0 || d <= 0) return 0;
    return train_layout(N, B, n, m, d).total;
}

extern "C" int mfcd_train_workspace_init(void *workspace, size_t workspace_bytes, int64_t N_cap, int B, int n, int m,
                                         int d, void *stream)
{
    if (!workspace || N_cap < 0 || B <= 0 || n <= 0 || m <= 0 || d <= 0 || d > MFCD_MAX_D) return MFCD_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return MFCD_EALIGN;
    const TrainLayout L = train_layout(N_cap, B, n, m, d);
    if (workspace_bytes < L.total) return MFCD_EWORKSPACE;
    // status word, touch strings, mailbox tags: everything a launch polls or ORs into starts from zero, once
    MFCD_HIP_TRY(hipMemsetAsync(workspace, 0, L.total, (hipStream_t)stream));
    auto S = std::make_unique<WsState>();
    S->bytes = workspace_bytes;
    (void)hipGetDevice(&S->device);
    S->N_cap = N_cap > 0 ? N_cap : 1;
    S->B = B; S->n = n; S->m = m; S->d = d;
    S->L = L;
    for (auto &sl : S->slot)
        if (int rc = stage_reserve(sl, L.stage_bytes)) return rc;
    std::lock_guard<std::mutex> lock(g_ws_mu);
    g_ws[workspace] = std::move(S);
    return 0;
}

extern "C" int mfcd_train_workspace_release(void *workspace)
{
    std::unique_ptr<WsState> dead;
    {
        std::lock_guard<std::mutex> lock(g_ws_mu);
        auto it = g_ws.find(workspace);
        if (it == g_ws.end()) return 0;
        dead = std::move(it->second);
        g_ws.erase(it);
    }
    for (auto &s : dead->slot)   // a slot a queued prologue still reads must outlive it
        if (s.pending) (void)hipEventSynchronize(s.ev);
    return 0;
}

namespace {

// "auto": the persistent launch has a fixed cost (prologue kernel, slice load / store: ~10 us at C2) that a call of
// fewer steps than this does not earn back against one streaming launch per step
constexpr int64_t kShortCallSteps = 3;

// form of the fused step a call with these sizes takes under the current settings
struct FormChoice {
    int form;   // 1 streaming, 2 resident, 3 local, <0 error
    mfcd_detail::ResidentPlan rp;
};

FormChoice choose_form(bool f32, bool resident_planned, int ev_tshift, int64_t N, int B, int n, int m, int d)
{
    FormChoice c{};
    const int64_t nsteps = (N + B - 1) / B;
    const bool local_ok = f32 && nsteps <= 0x7fffffff && mfcd_detail::local_applies(N, B, n, m, d);
    if (g_train_path == 3) {
        c.form = local_ok ? 3 : MFCD_EINVAL;
        return c;
    }
    if (g_train_path == 0 && local_ok) {   // measured 1.2-5.7x faster than the resident form wherever it applies
        c.form = 3;
        return c;
    }
    bool resident_ok = false;
    if (resident_planned && g_train_path != 1 && N > 0 && nsteps <= 0x7fffffff &&
        nsteps + 1 < ((int64_t)1 << kTagStepBits)) {
        c.rp = mfcd_detail::plan_resident(N, B, n, m, d, device_cus(), !f32, ev_tshift);
        resident_ok = c.rp.ok;
    }
    if (g_train_path == 2) {
        c.form = resident_ok ? 2 : MFCD_EINVAL;
        return c;
    }
    c.form = (resident_ok && nsteps >= kShortCallSteps) ? 2 : 1;
    return c;
}

// what mfcd_train_call_prepare binds: everything of a call but its samples, step and loss buffer
struct TrainCall {
    AdamTables t;
    int bf16, B, n, m, d;
    AdamHyper h;
    void *workspace;
    size_t workspace_bytes;
};

// ---- persistent forms: ONE launch for all nsteps (resident.hip / local.hip) behind ONE prologue kernel ----
int run_persistent(WsState &S, const TrainCall &c, const FormChoice &fc, const mfcd_sample *samples, int64_t N,
                   int64_t step0, float *loss_per_step, hipStream_t st, float *timing_us, bool stage_only)
{
    using mfcd_detail::ResidentCold;
    const TrainLayout &L = S.L;
    const int B = c.B, n = c.n, m = c.m, d = c.d;
    const int64_t nsteps = (N + B - 1) / B;
    char *base = (char *)c.workspace;
    const bool resident = fc.form == 2;
    // look-ahead form (B <= 64): the batch means are formed inside the launch; otherwise by batch_mean_kernel
    const bool means_inside = resident && fc.rp.lookahead > 0;
    // the set of prologue regions this call uses; staged_hit: its prologue already ran into them, on the side stream
    const WsState::Staged call{true, samples, c.t.U, N, step0, loss_per_step, c.h.lr, c.h.beta1, c.h.beta2, 0};
    bool staged_hit = false;
    const int set = S.claim_set(call, means_inside && !timing_us, stage_only, &staged_hit);
    const PrologueRegions &R = L.set[set];
    ResidentCold *cold_dev = (ResidentCold *)(base + R.stage_off);
    const StepScalars *sc_dev = (const StepScalars *)(cold_dev + 1);
    const mfcd_detail::SampleTranslation tr{samples, N, B, n, m, resident ? 64 * fc.rp.Q / d : 0, fc.rp.tshift,
                                            means_inside ? fc.rp.lookahead : 0, L.nch_cap,
                                            resident ? (mfcd_sample *)(base + R.xs_off) : nullptr,
                                            (unsigned *)(base + R.evcnt_off), base + R.event_off};
    // the stage table (ResidentCold, step scalars): short calls build it on this thread's stack and it travels in the
    // prologue's kernel arguments; longer ones build it in a pinned slot that the prologue reads over the host link
    const size_t need = kColdBytes + sizeof(StepScalars) * (size_t)(nsteps + 1);
    alignas(16) unsigned char inline_stage[4096];
    const bool stage_inline = need <= mfcd_detail::train_inline_stage_bytes() && need <= sizeof(inline_stage);
    StageSlot *slot = nullptr;
    if (!staged_hit && !stage_inline)
        if (int rc = stage_acquire(S, need, &slot)) return rc;
    char *const stage_host = slot ? (char *)slot->host : (char *)inline_stage;
    if (!staged_hit) {
        ResidentCold cold{};
        cold.U = (float *)c.t.U; cold.V = (float *)c.t.V;
        cold.mU = c.t.mU; cold.vU = c.t.vU; cold.mV = c.t.mV; cold.vV = c.t.vV;
        cold.status = (int *)base; cold.spin_limit = mfcd_detail::g_tune.spin_limit;
        cold.ev_cnt = tr.ev_cnt; cold.ev_ent = (uint4 *)tr.ev_ent;
        cold.nch_cap = L.nch_cap; cold.tshift = fc.rp.tshift;
        cold.loss_out = means_inside ? loss_per_step : nullptr;
        std::memcpy(stage_host, &cold, sizeof(cold));
        StepScalars *sc_host = (StepScalars *)(stage_host + sizeof(cold));
        for (int64_t k = 0; k <= nsteps; ++k) sc_host[k] = step_scalars(c.h, step0 + k + 1);
        if (means_inside)
            if (int rc = S.clear_lists(set, base, st)) return rc;
    }
    // a call that launches: its tag base and the clears of what other forms left (ahead of the prologue, as before)
    unsigned tag_base = 0;
    if (!stage_only) {
        if (resident) {
            if (int rc = S.next_tag_base(base, st, &tag_base)) return rc;
            if (int rc = S.clear_dirty(base, st)) return rc;
        }
        if (!means_inside) S.terms_dirty = true;
    }
    if (!staged_hit) {
        if (stage_only) S.lists_dirty[set] = true;   // until the staged call's launch has read the lists
        if (int rc = mfcd_detail::launch_train_prologue({stage_host, slot ? slot->devview : nullptr, cold_dev, need},
                                                        &tr, st))
            return rc;
    }
    if (stage_only) {
        // the prologue of a LATER call, on the caller's side stream: that call finds it by what it was built from
        if (slot)
            if (int rc = slot->release(st)) return rc;
        S.staged = call;
        S.staged.set = set;
        return 0;
    }
    if (staged_hit) S.staged.valid = false;   // consumed (the caller ordered the streams)
    if (resident) {
        S.last_set = set;
        S.lists_dirty[set] = false;      // the launch below reads the lists and leaves their counters at zero
    }

    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timing_us) {
        MFCD_HIP_TRY(hipEventCreate(&e0));
        MFCD_HIP_TRY(hipEventCreate(&e1));
        MFCD_HIP_TRY(hipEventRecord(e0, st));
    }
    const AdamStatic as = adam_static(c.h);
    void *terms = base + L.terms_off;
    int rc = 0;
    if (resident)
        rc = mfcd_detail::launch_resident_steps(fc.rp, cold_dev, tr.xs, N, B, n, m, d, sc_dev, as,
                                                (unsigned long long *)(base + L.mailbox_off), tag_base, terms,
                                                (unsigned long long *)(base + L.dbg_off), (int)nsteps, st);
    else
        rc = mfcd_detail::launch_local_steps((float *)c.t.U, (float *)c.t.V, c.t.mU, c.t.vU, c.t.mV, c.t.vV, samples, N, B,
                                             n, m, d, sc_dev, as, (float *)terms, (int)nsteps, st);
    if (rc) return rc;
    if (timing_us) MFCD_HIP_TRY(hipEventRecord(e1, st));
    if (loss_per_step && !means_inside)
        rc = mfcd_detail::launch_batch_means((const float *)terms, samples, N, B, loss_per_step, st);
    if (rc) return rc;
    // recorded behind the call's last launch so that the record does not sit between two launches (any later point of
    // the stream implies the prologue is done)
    if (slot)
        if (int rc = slot->release(st)) return rc;
    if (timing_us) {
        MFCD_HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        MFCD_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        timing_us[0] = timing_us[1] = timing_us[2] = ms * 1e3f / (float)nsteps;  // whole launch / steps
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    return 0;
}

// ---- streaming form: one launch per optimiser step ----
template <typename TP>
int run_streaming(WsState &S, const TrainCall &c, const mfcd_sample *samples, int64_t N, int64_t step0,
                  float *loss_per_step, hipStream_t st, float *timing_us)
{
    const TrainLayout &L = S.L;
    const int B = c.B, n = c.n, m = c.m, d = c.d;
    const int64_t nsteps = (N + B - 1) / B;
    char *base = (char *)c.workspace;
    TP *U = (TP *)c.t.U, *V = (TP *)c.t.V;
    if (L.resident) S.mailbox_dirty = S.terms_dirty = true;
    TP *Ualt = (TP *)(base + L.ualt_off);
    TP *Valt = (TP *)(base + L.valt_off);
    float *terms = (float *)(base + L.terms_off);

    const void *ptrs[] = {U, V, c.t.mU, c.t.vU, c.t.mV, c.t.vV, Ualt, Valt};
    const mfcd_detail::Plan pl = mfcd_detail::make_plan(ptrs, 8, n, m, d);
    std::vector<hipEvent_t> ev;
    if (timing_us) {
        ev.resize(2 * (size_t)nsteps);
        for (auto &e : ev) MFCD_HIP_TRY(hipEventCreate(&e));
    }
    for (int64_t k = 0; k < nsteps; ++k) {
        const int64_t off = k * B;
        const int Bk = (int)((N - off) < B ? (N - off) : B);
        const AdamConst ac = adam_const(c.h, step0 + k + 1);
        const bool even = (k & 1) == 0;
        if (timing_us) MFCD_HIP_TRY(hipEventRecord(ev[2 * k], st));
        mfcd_detail::launch_streaming_step<0, TP>(pl, st, even ? U : Ualt, even ? V : Valt, even ? Ualt : U,
                                                  even ? Valt : V, c.t.mU, c.t.vU, c.t.mV, c.t.vV, samples + off,
                                                  nullptr, Bk, 1.0f / (float)Bk, n, m, d, ac, terms + off);
        if (timing_us) MFCD_HIP_TRY(hipEventRecord(ev[2 * k + 1], st));
    }
    MFCD_HIP_TRY(hipGetLastError());
    if (nsteps & 1) {
        MFCD_HIP_TRY(hipMemcpyAsync(U, Ualt, sizeof(TP) * (size_t)n * d, hipMemcpyDeviceToDevice, st));
        MFCD_HIP_TRY(hipMemcpyAsync(V, Valt, sizeof(TP) * (size_t)m * d, hipMemcpyDeviceToDevice, st));
    }
    if (loss_per_step)
        if (int rc = mfcd_detail::launch_batch_means(terms, nullptr, N, B, loss_per_step, st)) return rc;
    if (timing_us) {
        MFCD_HIP_TRY(hipEventSynchronize(ev.back()));
        double sum = 0.0;
        float mn = 1e30f, mx = 0.0f;
        for (int64_t k = 0; k < nsteps; ++k) {
            float ms = 0.0f;
            MFCD_HIP_TRY(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
            sum += ms;
            mn = ms < mn ? ms : mn;
            mx = ms > mx ? ms : mx;
        }
        timing_us[0] = (float)(sum / (double)nsteps * 1e3);
        timing_us[1] = mn * 1e3f;
        timing_us[2] = mx * 1e3f;
        for (auto &e : ev) (void)hipEventDestroy(e);
    }
    return 0;
}

// Shared body of mfcd_train_steps* and mfcd_train_call_*, fp32 or bf16 tables.  With `timing_us` set, every step launch
// is bracketed by its own pair of HIP events on the launch stream and the host waits for them at the end.  stage_only:
// only the prologue, of a later call of the same arguments, on `stream` (mfcd_train_call_stage).
int run_call(const TrainCall &c, const mfcd_sample *samples, int64_t N, int64_t step0, float *loss_per_step,
             void *stream, float *timing_us, bool stage_only = false)
{
    if (int rc = check_common(c.t.U, c.t.V, c.n, c.m, c.d)) return rc;
    if (!c.t.mU || !c.t.vU || !c.t.mV || !c.t.vV || N < 0 || c.B <= 0 || step0 < 0) return MFCD_EINVAL;
    if (N == 0) return 0;
    if (!samples || !c.workspace) return MFCD_EINVAL;
    WsState *S = find_ws(c.workspace);
    if (!S) return MFCD_ESTATE;   // mfcd_train_workspace_init has not been called on this workspace
    const int64_t nsteps = (N + c.B - 1) / c.B;
    if (c.n != S->n || c.m != S->m || c.d != S->d) return MFCD_ESTATE;
    if (N > S->N_cap || nsteps > S->L.K_cap || c.workspace_bytes < S->L.total) return MFCD_EWORKSPACE;
    const TrainLayout &L = S->L;
    hipStream_t st = (hipStream_t)stream;

    // bf16 factor tables: streaming or resident form (the local form is fp32 only)
    const FormChoice fc = choose_form(!c.bf16, L.resident, L.ev.tshift, N, c.B, c.n, c.m, c.d);
    if (fc.form < 0) return fc.form;

    if (stage_only && !(fc.form == 2 && fc.rp.lookahead > 0 && L.two_sets)) return 0;   // nothing to stage for this form
    if (fc.form == 2 || fc.form == 3)
        return run_persistent(*S, c, fc, samples, N, step0, loss_per_step, st, timing_us, stage_only);
    if (c.bf16) return run_streaming<mfcd_bf16>(*S, c, samples, N, step0, loss_per_step, st, timing_us);
    return run_streaming<float>(*S, c, samples, N, step0, loss_per_step, st, timing_us);
}

}  // namespace

extern "C" int mfcd_train_plan_query(int64_t N, int B, int n, int m, int d, int bf16_factors, mfcd_train_plan *out)
{
    if (!out || N < 0 || B <= 0 || n <= 0 || m <= 0 || d <= 0 || d > MFCD_MAX_D) return MFCD_EINVAL;
    std::memset(out, 0, sizeof(*out));
    const TrainLayout L = train_layout(N, B, n, m, d);
    const FormChoice fc = choose_form(!bf16_factors, L.resident, L.ev.tshift, N > 0 ? N : 1, B, n, m, d);
    if (fc.form < 0) return fc.form;
    out->form = fc.form;
    if (fc.form == 2) {
        out->resident_q = fc.rp.Q;
        out->resident_waves = fc.rp.NW;
        out->resident_blocks = fc.rp.blocks;
        out->resident_lookahead = fc.rp.lookahead;
        out->fast_math = fc.rp.fast_math ? 1 : 0;
    } else if (fc.form == 3) {
        out->fast_math = mfcd_detail::g_resident_math != 0;
    } else {
        const void *none[] = {nullptr};
        // alignment of real pointers can only lower vec to 1
        const mfcd_detail::Plan pl = mfcd_detail::make_plan(none, 0, n, m, d);
        out->streaming_vec = pl.vec;
        out->streaming_chunks = pl.chunks;
        out->streaming_blocks = pl.blocksU + pl.blocksV;
    }
    out->device_cus = device_cus();
    return 0;
}

extern "C" int mfcd_train_steps(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                                const mfcd_sample *samples, int64_t N, int B, int64_t step0, int n, int m, int d,
                                double lr, double beta1, double beta2, double eps, double weight_decay,
                                float *loss_per_step, void *workspace, size_t workspace_bytes, void *stream)
{
    const TrainCall c{{U, V, mU, vU, mV, vV}, 0, B, n, m, d, {lr, beta1, beta2, eps, weight_decay}, workspace, workspace_bytes};
    return run_call(c, samples, N, step0, loss_per_step, stream, nullptr);
}

extern "C" int mfcd_train_steps_bf16(uint16_t *U, uint16_t *V, float *mU, float *vU, float *mV, float *vV,
                                     const mfcd_sample *samples, int64_t N, int B, int64_t step0, int n, int m, int d,
                                     double lr, double beta1, double beta2, double eps, double weight_decay,
                                     float *loss_per_step, void *workspace, size_t workspace_bytes, void *stream)
{
    const TrainCall c{{U, V, mU, vU, mV, vV}, 1, B, n, m, d, {lr, beta1, beta2, eps, weight_decay}, workspace, workspace_bytes};
    return run_call(c, samples, N, step0, loss_per_step, stream, nullptr);
}

extern "C" int mfcd_train_steps_timed(float *U, float *V, float *mU, float *vU, float *mV, float *vV,
                                      const mfcd_sample *samples, int64_t N, int B, int64_t step0, int n, int m,
                                      int d, double lr, double beta1, double beta2, double eps, double weight_decay,
                                      float *loss_per_step, void *workspace, size_t workspace_bytes, void *stream,
                                      float *kernel_us_host)
{
    if (!kernel_us_host) return MFCD_EINVAL;
    const TrainCall c{{U, V, mU, vU, mV, vV}, 0, B, n, m, d, {lr, beta1, beta2, eps, weight_decay}, workspace, workspace_bytes};
    return run_call(c, samples, N, step0, loss_per_step, stream, kernel_us_host);
}

extern "C" int mfcd_train_call_prepare(void *U, void *V, float *mU, float *vU, float *mV, float *vV, int bf16_factors,
                                       int B, int n, int m, int d, double lr, double beta1, double beta2, double eps,
                                       double weight_decay, void *workspace, size_t workspace_bytes, void **handle_out)
{
    if (!handle_out) return MFCD_EINVAL;
    *handle_out = nullptr;
    if (int rc = check_common(U, V, n, m, d)) return rc;
    if (!mU || !vU || !mV || !vV || B <= 0 || !workspace) return MFCD_EINVAL;
    WsState *S = find_ws(workspace);
    if (!S) return MFCD_ESTATE;
    if (n != S->n || m != S->m || d != S->d) return MFCD_ESTATE;
    if (workspace_bytes < S->L.total) return MFCD_EWORKSPACE;
    *handle_out = new TrainCall{{U, V, mU, vU, mV, vV}, bf16_factors ? 1 : 0, B, n, m, d,
                                {lr, beta1, beta2, eps, weight_decay}, workspace, workspace_bytes};
    return 0;
}

extern "C" int mfcd_train_call_run(void *handle, const mfcd_sample *samples, int64_t N, int64_t step0,
                                   float *loss_per_step, void *stream)
{
    const TrainCall *c = (const TrainCall *)handle;
    if (!c) return MFCD_EINVAL;
    return run_call(*c, samples, N, step0, loss_per_step, stream, nullptr);
}

extern "C" int mfcd_train_call_stage(void *handle, const mfcd_sample *samples, int64_t N, int64_t step0,
                                     float *loss_per_step, void *side_stream)
{
    const TrainCall *c = (const TrainCall *)handle;
    if (!c) return MFCD_EINVAL;
    return run_call(*c, samples, N, step0, loss_per_step, side_stream, nullptr, true);
}

extern "C" int mfcd_train_call_release(void *handle)
{
    delete (TrainCall *)handle;
    return 0;
}

// ---- batched local form and multi-model validation pass (include/mfcd.h: mfcd_train_steps_local_multi,
// mfcd_eval_batches_multi).  A multi-model workspace is registered like a training workspace (same registry, same pinned
// staging ring) but with n = m = d = 0, so that neither kind of call accepts the other kind's workspace. ----
namespace {

// per-model validation of the batched local form: what mfcd_train_steps would put on the local form (choose_form)
bool local_model_ok(const mfcd_local_model &md)
{
    if (check_common(md.U, md.V, md.n, md.m, md.d)) return false;
    if (!md.mU || !md.vU || !md.mV || !md.vV || !md.samples || !md.loss_per_step || md.N <= 0 || md.B <= 0 ||
        md.step0 < 0)
        return false;
    const FormChoice fc = choose_form(true, false, 0, md.N, md.B, md.n, md.m, md.d);
    return fc.form == 3;
}

struct MultiLayout {   // stage region: LocalArgs[R] | MeanSeg[R] | StepScalars[sum(K_r + 1)] ; then the loss terms
    size_t seg_off, sc_off, stage_bytes, terms_off, total;
    int64_t steps, samples;
};

MultiLayout local_multi_layout(const mfcd_local_model *models, int R)
{
    MultiLayout L{};
    for (int r = 0; r < R; ++r) {
        L.steps += (models[r].N + models[r].B - 1) / models[r].B;
        L.samples += models[r].N;
    }
    L.seg_off = align_up(sizeof(mfcd_detail::LocalArgs) * (size_t)R, 16);
    L.sc_off = L.seg_off + align_up(sizeof(mfcd_detail::MeanSeg) * (size_t)R, 16);
    L.stage_bytes = L.sc_off + sizeof(StepScalars) * (size_t)(L.steps + R);
    L.terms_off = align_up(L.stage_bytes);
    L.total = L.terms_off + align_up(sizeof(float) * (size_t)L.samples);
    return L;
}

size_t eval_multi_stage_bytes(int R) { return align_up(sizeof(mfcd_detail::EvalSeg) * (size_t)R, 16); }

bool eval_model_ok(const mfcd_eval_model &md)
{
    if (!md.U || !md.V || md.n <= 0 || md.m <= 0 || md.d <= 0 || md.d > MFCD_MAX_D || md.N < 0 || md.B <= 0 ||
        md.B > 16384)
        return false;
    return md.N == 0 || (md.samples && md.loss_per_batch);
}

WsState *find_multi_ws(void *workspace)
{
    WsState *S = workspace ? find_ws(workspace) : nullptr;
    return S && S->n == 0 ? S : nullptr;
}

}  // namespace

extern "C" size_t mfcd_local_model_bytes(void) { return sizeof(mfcd_local_model); }
extern "C" size_t mfcd_eval_model_bytes(void) { return sizeof(mfcd_eval_model); }

extern "C" size_t mfcd_train_local_multi_workspace_bytes(const mfcd_local_model *models, int R, size_t *stage_bytes_out)
{
    if (!models || R <= 0) return 0;
    for (int r = 0; r < R; ++r)
        if (models[r].N <= 0 || models[r].B <= 0) return 0;
    const MultiLayout L = local_multi_layout(models, R);
    if (stage_bytes_out) *stage_bytes_out = L.stage_bytes;
    return L.total;
}

extern "C" size_t mfcd_eval_multi_workspace_bytes(int R, size_t *stage_bytes_out)
{
    if (R <= 0) return 0;
    if (stage_bytes_out) *stage_bytes_out = eval_multi_stage_bytes(R);
    return align_up(eval_multi_stage_bytes(R));
}

extern "C" int mfcd_multi_workspace_init(void *workspace, size_t workspace_bytes, size_t stage_bytes)
{
    if (!workspace || workspace_bytes == 0 || stage_bytes == 0 || stage_bytes > workspace_bytes) return MFCD_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return MFCD_EALIGN;
    auto S = std::make_unique<WsState>();
    S->bytes = workspace_bytes;
    (void)hipGetDevice(&S->device);
    for (auto &sl : S->slot)
        if (int rc = stage_reserve(sl, stage_bytes)) return rc;
    std::lock_guard<std::mutex> lock(g_ws_mu);
    g_ws[workspace] = std::move(S);
    return 0;
}

extern "C" int mfcd_train_steps_local_multi(const mfcd_local_model *models, int R, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    using mfcd_detail::LocalArgs;
    using mfcd_detail::MeanSeg;
    if (!models || R <= 0 || !workspace) return MFCD_EINVAL;
    // every check comes before the first launch: a rejected call touches no table
    int ql = 1, max_B = 0;
    for (int r = 0; r < R; ++r) {
        if (!local_model_ok(models[r])) return MFCD_EINVAL;
        const int q = mfcd_detail::local_ql(models[r].n, models[r].m, models[r].d);
        ql = q > ql ? q : ql;
        max_B = models[r].B > max_B ? models[r].B : max_B;
    }
    const MultiLayout L = local_multi_layout(models, R);
    if (L.steps > 0x7fffffff) return MFCD_EINVAL;
    WsState *S = find_multi_ws(workspace);
    if (!S) return MFCD_ESTATE;   // mfcd_multi_workspace_init has not been called on this workspace
    if (workspace_bytes < L.total || S->bytes < L.total) return MFCD_EWORKSPACE;
    StageSlot *slot = nullptr;
    if (int rc = stage_acquire(*S, L.stage_bytes, &slot)) return rc;

    char *base = (char *)workspace, *host = (char *)slot->host;
    LocalArgs *tab = (LocalArgs *)host;
    MeanSeg *segs = (MeanSeg *)(host + L.seg_off);
    StepScalars *sc = (StepScalars *)(host + L.sc_off);
    int64_t k0 = 0, t0 = 0, blk0 = 0;
    size_t lds = 0;
    for (int r = 0; r < R; ++r) {
        const mfcd_local_model &md = models[r];
        const int64_t K = (md.N + md.B - 1) / md.B;
        const AdamHyper h{md.lr, md.beta1, md.beta2, md.eps, md.weight_decay};
        for (int64_t k = 0; k <= K; ++k) sc[k0 + k] = step_scalars(h, md.step0 + k + 1);
        LocalArgs a{};
        a.U = md.U; a.V = md.V; a.mU = md.mU; a.vU = md.vU; a.mV = md.mV; a.vV = md.vV;
        a.samples = md.samples;
        a.sc = (const StepScalars *)(base + L.sc_off) + k0;
        a.loss_terms = (float *)(base + L.terms_off) + t0;
        a.N = md.N; a.B = md.B; a.n = md.n; a.m = md.m; a.d = md.d; a.K = (int)K;
        a.ac = adam_static(h);
        const size_t need = mfcd_detail::local_multi_fill(a, ql);
        lds = need > lds ? need : lds;
        tab[r] = a;
        MeanSeg sg{};
        sg.terms = a.loss_terms; sg.samples = md.samples; sg.out = md.loss_per_step;
        sg.N = md.N; sg.B = md.B; sg.blk_begin = blk0;
        segs[r] = sg;
        k0 += K + 1;
        t0 += md.N;
        blk0 += K;
    }
    if (lds > mfcd_detail::kLocalMaxLds) return MFCD_EINVAL;   // (not reached: every model fits at QL = 8)

    hipStream_t st = (hipStream_t)stream;
    if (int rc = mfcd_detail::launch_train_prologue({host, slot->devview, base, L.stage_bytes}, nullptr, st)) return rc;
    if (int rc = mfcd_detail::launch_local_multi((const LocalArgs *)base, R, ql, max_B <= mfcd_detail::kLocalSmallBatch,
                                                 lds, st))
        return rc;
    if (int rc = mfcd_detail::launch_batch_means_multi((const MeanSeg *)(base + L.seg_off), R, L.steps, st)) return rc;
    return slot->release(st);
}

extern "C" int mfcd_eval_batches_multi(const mfcd_eval_model *models, int R, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    using mfcd_detail::EvalSeg;
    if (!models || R <= 0 || !workspace) return MFCD_EINVAL;
    for (int r = 0; r < R; ++r)
        if (!eval_model_ok(models[r])) return MFCD_EINVAL;
    WsState *S = find_multi_ws(workspace);
    if (!S) return MFCD_ESTATE;
    const size_t stage_bytes = eval_multi_stage_bytes(R);
    if (workspace_bytes < stage_bytes || S->bytes < stage_bytes) return MFCD_EWORKSPACE;
    StageSlot *slot = nullptr;
    if (int rc = stage_acquire(*S, stage_bytes, &slot)) return rc;
    EvalSeg *segs = (EvalSeg *)slot->host;
    int nseg = 0, max_B = 1;
    int64_t blocks = 0;
    for (int r = 0; r < R; ++r) {
        const mfcd_eval_model &md = models[r];
        if (md.N == 0) continue;   // no batch: no segment
        EvalSeg sg{};
        sg.U = md.U; sg.V = md.V; sg.samples = md.samples; sg.loss = md.loss_per_batch;
        sg.correct = md.correct_per_batch;
        sg.N = md.N; sg.B = md.B; sg.d = md.d; sg.blk_begin = blocks;
        segs[nseg++] = sg;
        blocks += (md.N + md.B - 1) / md.B;
        max_B = md.B > max_B ? md.B : max_B;
    }
    if (blocks == 0) return 0;
    if (blocks > 0x7fffffff) return MFCD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = mfcd_detail::launch_train_prologue({segs, slot->devview, workspace, stage_bytes}, nullptr, st)) return rc;
    if (int rc = mfcd_detail::launch_eval_multi((const EvalSeg *)workspace, nseg, blocks, max_B, st)) return rc;
    return slot->release(st);
}