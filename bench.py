#!/usr/bin/env python3
"""bench.py — triplet-updates/s of the fused MI355X training step at BASELINE.json's C2
(n=m=4096, d=64, p=0.01, random triplets, fp32, B=64, Adam lr=1e-3 wd=1e-5).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]   (N>1: launched by torch.distributed.run)

A "step" is one optimiser step = one pass of the hot path over one batch of 64 synthetic triplets.
Steps are consumed the way train_model consumes them: epoch by epoch (1049 steps per epoch at C2, the
last batch short), a fresh permutation per epoch, and the no-grad validation pass after every complete
epoch.  Inputs are resident in HBM when the timed region starts.
Prints ONE JSON line (rank 0).

A plain run measures the headline only: set-up, the untimed clock ramp, W warm-up steps, the K timed steps
(`value`, `ms_per_step`; `roofline` from the timed region's own event pairs when it holds >= 256 steps), the
outputs if --dump-outputs is given, the line.  --full adds what takes runs of its own: `roofline.kernel_only`,
`steady_state`, `uvt` and `cpu_baseline` (--no-extras / --no-cpu-baseline drop some of them again), and on the
multi-GPU path the phase split, cost model and C4 sub-record.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("OMP_NUM_THREADS", "4")  # the reference's own setting (structure.py:3)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_F32_PEAK_TF = 157.3  # same guide: v_mfma_f32_32x32x2_f32 at 64 FLOP/clk/SIMD (155 TF measured)
MFMA_BF16_PEAK_TF = 2500.0  # dense bf16 MFMA peak (task statement / same guide); the UV^T pass issues THREE bf16 products per fp32 product
# Vector-issue roofline of the register-resident form (same guide, cycle constants): 256 CUs x 4 SIMD-32 at 2.4 GHz;
# a wave64 VALU instruction occupies its SIMD for 2 cycles, a transcendental (v_rcp / v_sqrt) for 8.
SIMDS, CLOCK_GHZ, CYC_PLAIN, CYC_TRANS = 1024, 2.4, 2, 8
# csrc/train_common.h adam_update_fast: 16 plain fp32 instructions + v_sqrt + v_rcp per element register of a wave
ADAM_FAST_PLAIN, ADAM_FAST_TRANS = 16, 2

C2 = dict(n=4096, m=4096, d=64, p=0.01, s=1.0, K=1, B=64, lr=1e-3, wd=1e-5)
# BASELINE.json configs[3], the configuration named for data parallelism (rehearsal only: --workload C4)
C4 = dict(n=65536, m=65536, d=64, p=0.0005, s=1.0, K=4, B=64, lr=1e-3, wd=1e-5)
# BASELINE.json configs[2] (timing rehearsal: uniform triplets at its count; its margin sampler yields ~11 k, tests use it)
C3 = dict(n=16384, m=16384, d=128, p=0.001, s=1.0, K=1, B=64, lr=1e-3, wd=1e-5)
WORKLOADS = {"C2": C2, "C3": C3, "C4": C4}


def make_workload(cfg, seed):
    """Synthetic C2 inputs: rank-d "base"-law X kept factored (X = A B^T, entry std ~0.5),
    int(n*m*p/2) unique uniform triplets, hard BTL labels, 80/10/10 split, U,V ~ N(0, 1/d)."""
    n, m, d = cfg["n"], cfg["m"], cfg["d"]
    g = torch.Generator().manual_seed(seed)
    import generation_data as gd
    A, Bf = gd.generate_embedding_factors(n, m, d, "cpu", generator=g)
    rng = np.random.default_rng(seed)
    want = int(n * m * cfg["p"] / 2)
    keys = np.empty(0, dtype=np.int64)
    while keys.size < want:
        u = rng.integers(0, n, want)
        i = rng.integers(0, m, want)
        j = rng.integers(0, m, want)
        ok = i != j
        k = (u[ok].astype(np.int64) * m + i[ok]) * m + j[ok]
        keys = np.unique(np.concatenate([keys, k]))
    keys = rng.permutation(keys)[:want]
    u, i, j = keys // (m * m), (keys // m) % m, keys % m
    A, Bf = A.numpy().astype(np.float64), Bf.numpy().astype(np.float64)
    diff = np.einsum("td,td->t", A[u], Bf[i] - Bf[j])
    prob = 1.0 / (1.0 + np.exp(-cfg["s"] * diff))
    n_tr, n_va = int(0.8 * want), int(0.1 * want)
    K = int(cfg.get("K", 1))

    def labelled(lo, hi, reps):   # K independent hard labels per training triplet (structure.py:493-519, soft_label=False)
        idx = np.repeat(np.arange(lo, hi), reps)
        z = (rng.random(idx.size) < prob[idx]).astype(np.float64)
        return np.stack([u[idx], i[idx], j[idx], z], 1).astype(np.float64)

    U0 = (torch.randn(n, d, generator=g) / np.sqrt(d)).numpy()
    V0 = (torch.randn(m, d, generator=g) / np.sqrt(d)).numpy()
    return labelled(0, n_tr, K), labelled(n_tr, n_tr + n_va, 1), U0, V0


def algorithmic_bytes_per_step(cfg):
    """24*(n+m)*d [p,m,v read+write] + 12*B*d [three gathered rows] + 16*B [records]."""
    return 24 * (cfg["n"] + cfg["m"]) * cfg["d"] + 12 * cfg["B"] * cfg["d"] + 16 * cfg["B"]


def algorithmic_valu_cycles_per_step(cfg):
    """Vector-issue cycles one optimiser step NEEDS when the state lives in registers: the dense Adam update of every
    element, nothing else (row exchange, bookkeeping and waits are overhead, not work): (n+m)*d/64 wave-registers x
    (16 plain x 2 cycles + 2 transcendental x 8 cycles)."""
    regs = (cfg["n"] + cfg["m"]) * cfg["d"] / 64.0
    return regs * (ADAM_FAST_PLAIN * CYC_PLAIN + ADAM_FAST_TRANS * CYC_TRANS)


def offline_traffic(cfg, plan, abytes):
    """`traffic_offline`: the newest committed counter measurement of this kernel (profiles/r*_pmc_traffic.json, made by
    tools/pmc_summary.py from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes with the guide's gfx950
    correction).  No counter pass can run inside this process, so `traffic` itself stays null; this names the file the
    figure comes from and its ratio to the algorithmic bytes."""
    import glob
    if cfg.get("name", "C2") != "C2" or plan["form_name"] != "resident":
        return None
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            rec = json.load(f)
        b = float(rec["hbm_bytes_per_step"])
        return {"file": os.path.relpath(files[-1], ROOT), "bytes_per_step": int(b),
                "ratio_to_algorithmic": round(b / abytes, 4), "kernel_config": rec.get("config")}
    except Exception:
        return None


def offline_kernel_stats(cfg, plan, steps_per_launch):
    """`kernel_only.rocprof_offline`: the dominant kernel's average duration in the newest committed
    `rocprofv3 --kernel-trace --stats` summary of this command (profiles/r*_bench_c2_driver_cmd_kernel_stats.csv for the
    driver's 20-step call, r*_bench_c2_kernel_stats.csv for whole epochs), and the roofline fraction at that duration.
    The live HIP-event pair reads a few microseconds more per launch: it brackets the launch's dispatch and completion
    signalling as well."""
    import csv
    import glob
    if cfg.get("name", "C2") != "C2" or plan["form_name"] != "resident":
        return None
    pat = "r*_bench_c2_driver_cmd_kernel_stats.csv" if steps_per_launch == 20 else \
        ("r*_bench_c2_kernel_stats.csv" if steps_per_launch >= 1049 else None)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pat))) if pat else []
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            rows = [r for r in csv.DictReader(f) if "resident_train_kernel" in r["Name"]]
        row = max(rows, key=lambda r: int(r["Calls"]))
        avg_us = float(row["AverageNs"]) / 1e3
        launch_steps = 20 if steps_per_launch == 20 else 1049
        frac = algorithmic_valu_cycles_per_step(cfg) * launch_steps / (avg_us * 1e-6) / 1e9 / (1024 * 2.4)
        return {"file": os.path.relpath(files[-1], ROOT), "calls": int(row["Calls"]), "avg_us_per_launch": round(avg_us, 2),
                "steps_per_launch": launch_steps, "frac_at_that_duration": round(frac, 4),
                "note": "offline profile of the same command on the same kernel build; the launches it averages are mostly "
                        "the untimed clock ramp's (identical calls)" if steps_per_launch == 20 else
                        "offline profile of the same command; averages include the shorter event-pair sample launch"}
    except Exception:
        return None


def roofline_record(cfg, plan, period_us, kernel_us=None, kernel_step_us=None):
    """`roofline` object for the form that actually ran (engine.train_plan), per optimiser step.
    Streaming form: HBM-bound, achieved = algorithmic bytes / time.  Resident / local forms: the state never leaves
    registers (LDS), so the byte model does not apply; the bound is vector issue, achieved = the Adam update's own
    issue cycles / time against 1024 SIMDs x 2.4 GHz, and the HBM-equivalent rate is reported beside it, labelled.
    `time` is the DOMINANT KERNEL's launch duration per optimiser step (`kernel_step_us`: HIP event pair directly around
    that launch, mfcd_train_steps_timed) when it was measured, else the whole call's period (`period_us`: event pair
    around the call, prologue / batch-mean launches and gaps included), which is always reported as `call_level`."""
    abytes = algorithmic_bytes_per_step(cfg)
    call_period_us = period_us
    if kernel_step_us:
        period_us = kernel_step_us
    hbm_equiv = abytes / (period_us * 1e-6) / 1e9
    if plan["form_name"] == "streaming":
        rec = {"bound": "hbm", "achieved": round(hbm_equiv, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(hbm_equiv / HBM_PEAK_GBS, 4), "traffic": None,
               "algorithmic_bytes_per_launch": abytes,
               "kernel": f"train_step_kernel<VEC={plan['streaming_vec']},CHUNKS={plan['streaming_chunks']}> "
                         f"({plan['streaming_blocks']} workgroups; one launch per optimiser step)"}
    else:
        cyc = algorithmic_valu_cycles_per_step(cfg)
        simds = SIMDS if plan["form_name"] in ("resident", "big-resident") else 4      # the local form runs on ONE CU
        peak = simds * CLOCK_GHZ                                     # G issue-cycles per second
        ach = cyc / (period_us * 1e-6) / 1e9
        kern = (f"resident_train_kernel<D={cfg['d']},Q={plan['resident_q']},LOOK={plan['resident_lookahead']},"
                f"{'fast' if plan['fast_math'] else 'ieee'}> ({plan['resident_waves']} waves; persistent: one launch per "
                "call, figures are per optimiser step = launch time / steps)") if plan["form_name"] == "resident" else \
               (f"big_train_kernel<{'fast' if plan['fast_math'] else 'ieee'}> (csrc/big.hip: 1024 waves, one per SIMD, 128 rows "
                "each; moments in 256 registers per lane, parameters in LDS; persistent: one launch per call, figures are "
                "per optimiser step = call time / steps)") if plan["form_name"] == "big-resident" else \
               "local_train_kernel (one workgroup, parameters in LDS; persistent: one launch per call)"
        rec = {"bound": "valu-issue", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "Gcycle/s",
               "frac": round(ach / peak, 4), "traffic": None,
               "algorithmic_valu_cycles_per_launch_step": round(cyc, 1),
               "valu_cycle_prices": {"plain_fp32": CYC_PLAIN, "transcendental": CYC_TRANS,
                                     "adam_fast_instructions": [ADAM_FAST_PLAIN, ADAM_FAST_TRANS]},
               "hbm_equivalent": {"GBps": round(hbm_equiv, 1), "frac_of_8TBps": round(hbm_equiv / HBM_PEAK_GBS, 4),
                                  "algorithmic_bytes_per_step": abytes,
                                  "note": "bytes a streaming step would move; this form keeps them in registers"},
               "traffic_note": "null: no counter pass ran inside this process; offline rocprofv3 --pmc figures for this "
                               "kernel are under profiles/ (README there names the file per round)",
               "kernel": kern}
    rec["traffic_offline"] = offline_traffic(cfg, plan, abytes)
    rec["priced_on"] = ("dominant kernel's launch duration / steps per launch (HIP event pair around the launch)"
                        if kernel_step_us else "whole call period (HIP event pair around the call)")
    rec["launch_period_us"] = round(call_period_us, 3)
    full = (abytes / (call_period_us * 1e-6) / 1e9 / HBM_PEAK_GBS) if rec["bound"] == "hbm" else \
        (algorithmic_valu_cycles_per_step(cfg) / (call_period_us * 1e-6) / 1e9 / rec["peak"])
    rec["call_level"] = {"us_per_step": round(call_period_us, 3), "frac": round(full, 4),
                         "includes": "every launch of the call (prologue, step kernel, batch mean) and the gaps"}
    if kernel_us is not None:
        rec["kernel_us_event_pairs"] = {k: round(v, 3) for k, v in zip(("avg", "min", "max"), kernel_us)}
    return rec


class Runner:
    """Consumes optimiser steps exactly like mfcd.engine.fit, but in step-counted slices."""

    def __init__(self, cfg, dev, seed, dtype=torch.float32):
        import structure as S
        from mfcd import engine
        self.engine, self.cfg, self.dev = engine, cfg, dev
        tr, va, U0, V0 = make_workload(cfg, seed)
        model = S.MatrixFactorization(cfg["n"], cfg["m"], cfg["d"], dtype=dtype)
        with torch.no_grad():
            model.U.copy_(torch.from_numpy(U0))
            model.V.copy_(torch.from_numpy(V0))
        self.model = model.to(dev)
        self.opt = torch.optim.Adam(self.model.parameters(), lr=cfg["lr"], weight_decay=cfg["wd"])
        self.bind = engine.AdamBinding(self.model, self.opt)
        self.train = engine.SampleStore(tr, cfg["n"], cfg["m"], dev)
        self.val = engine.SampleStore(va, cfg["n"], cfg["m"], dev)
        self.gen = torch.Generator().manual_seed(seed + 1)
        self.steps_per_epoch = (self.train.N + cfg["B"] - 1) // cfg["B"]
        self.stream, self.pos = None, 0
        self.pre = engine.StreamPrefetch(dev)   # next epoch's record stream is built under the running step kernel
        self.train_events = []  # (start, stop, launches) around each fused-step call in the timed region
        self.launched = []      # events behind the last two enqueued calls on the measured model
        # the workspace is planned ONCE for an epoch (as engine.fit does): no call of the run re-plans or re-initialises it
        engine.reserve_workspace(self.train.N, cfg["B"], cfg["n"], cfg["m"], cfg["d"], dev)
        self.event_pool = [torch.cuda.Event(enable_timing=True) for _ in range(64)]
        self.loss_bufs = {}
        self.last_loss, self.call_lengths = None, []

    def _event(self):
        return self.event_pool.pop() if self.event_pool else torch.cuda.Event(enable_timing=True)

    def reset_events(self):
        self.train_events = []

    def open_epoch(self):
        """Host-side part of an epoch start: draw the permutation, build the record stream (no-op inside an epoch)."""
        if self.stream is None:
            if self.pre.pending is None:
                self.pre.start(self.train, torch.randperm(self.train.N, generator=self.gen))
            self.stream, self.pos = self.pre.take(), 0

    def run(self, steps, record=False, bind=None):
        """Enqueue `steps` optimiser steps (+ a validation pass after every completed epoch). No host sync.
        Returns the number of training samples consumed.  `bind`: step a scratch model instead (clock_ramp)."""
        B, consumed = self.cfg["B"], 0
        bind = bind or self.bind
        while steps > 0:
            self.open_epoch()
            left = self.steps_per_epoch - self.pos
            take = min(left, steps)
            lo, hi = self.pos * B, min(self.train.N, (self.pos + take) * B)
            if record:
                e0, e1 = self._event(), self._event()
                e0.record()
            buf = self.loss_bufs.get(take)      # per call length, as a training loop keeps one per epoch
            if buf is None:
                buf = self.loss_bufs[take] = torch.empty(take, dtype=torch.float32, device=self.dev)
            self.engine.train_steps(bind, self.stream[lo:hi], B, loss_out=buf, defer_step=True)
            if bind is self.bind:
                self.last_loss = buf            # the per-step losses the most recent call on the measured model returned
                self.call_lengths.append(take)
            if record:
                e1.record()
                self.train_events.append((e0, e1, take))
            # an event behind each enqueued call on the workspace (whichever model it stepped): a staged prologue writes the
            # set of regions that the call BEFORE the most recent one may still be reading.  Short calls record none (the
            # driver's 20-step region stays free of it); a stage after one then waits for everything enqueued so far
            ev = None
            if take >= 256:
                ev = self.launched[0] if len(self.launched) == 2 and self.launched[0] is not None else torch.cuda.Event()
                ev.record()
            self.launched = (self.launched + [ev])[-2:]
            consumed += hi - lo
            self.pos += take
            steps -= take
            if self.pos == self.steps_per_epoch and self.pre.pending is None:
                # the epoch's last steps are enqueued: start building the next epoch's stream underneath them, and stage
                # the prologue of the call that will consume it (as mfcd.engine.fit does); if the next call turns out
                # not to be that whole epoch, the staged prologue is simply not used
                nxt = self.loss_bufs.get(self.steps_per_epoch)
                stage = None
                if bind is self.bind and nxt is not None:
                    stage = lambda rec, side: self.engine.stage_next_call(bind, rec, B, nxt, side)   # noqa: E731
                after = self.launched[0] if len(self.launched) == 2 else None
                if len(self.launched) == 2 and after is None:
                    after = torch.cuda.Event()
                    after.record()
                self.pre.start(self.train, torch.randperm(self.train.N, generator=self.gen), after=after, stage=stage)
            if self.pos == self.steps_per_epoch:  # structure.py:858-868
                self.engine.eval_batches(self.model.U.data, self.model.V.data, self.val.dev, B)
                self.stream = None
        return consumed

    def kernel_sample(self, launches=512):
        """[avg, min, max] µs of single step-kernel launches, each bracketed by its own HIP event pair."""
        B = self.cfg["B"]
        order = torch.randperm(self.train.N, generator=self.gen)
        stream = self.train.ordered(order)[: launches * B]
        out = [0.0, 0.0, 0.0]
        self.bind.flush()
        self.engine.train_steps(self.bind, stream, B, kernel_us=out)
        self.last_sample_records = stream          # the records that launch consumed (chain_model below)
        return out


def chain_depth(records, B, n):
    """Longest chain of dependent samples in a record stream (int [N, >= 3] rows of u, i, j): a sample's update reads its
    three rows as the previous step left them, so it hangs on the latest earlier sample that named any of them
    (tools/sim_chain_depth.py, tools/exp_chain_depth.py)."""
    r = np.asarray(records)[:, :3].astype(np.int64)
    depth = np.zeros(int(max(r[:, 0].max() + 1, n)) + int(r[:, 1:].max()) + 1, dtype=np.int64)
    off = int(max(r[:, 0].max() + 1, n))
    longest = 0
    for k in range(0, r.shape[0], B):
        a, b, c = r[k:k + B, 0], r[k:k + B, 1] + off, r[k:k + B, 2] + off
        dd = np.maximum(np.maximum(depth[a], depth[b]), depth[c]) + 1
        new = depth.copy()
        np.maximum.at(new, np.concatenate([a, b, c]), np.concatenate([dd, dd, dd]))
        depth = new
        longest = max(longest, int(dd.max()))
    return longest


# resident kernel at C2 shape: time per chain link and per-step floor, measured by tools/exp_chain_depth.py
CHAIN_LINK_US, CHAIN_FLOOR_US, CHAIN_FILE = 1.43, 0.36, "profiles/r03_chain_depth_experiment.txt"


def chain_model(cfg, plan, records, steps, measured_us):
    """`kernel_only.chain_model`: what the measured law of the resident kernel (launch time = floor per step
    + hand-off latency per link of the sample stream's dependency chain) predicts for the very records the sampled
    launch consumed, beside what was measured.  C2 shape only (the constants were measured there)."""
    if cfg.get("name", "C2") != "C2" or plan["form_name"] != "resident" or records is None:
        return None
    try:
        depth = chain_depth(records.cpu().numpy(), cfg["B"], cfg["n"])
        pred = CHAIN_FLOOR_US * steps + CHAIN_LINK_US * depth
        return {"chain_depth": depth, "link_us": CHAIN_LINK_US, "floor_us_per_step": CHAIN_FLOOR_US,
                "predicted_kernel_us": round(pred, 1), "measured_kernel_us": round(measured_us, 2),
                "measured_over_predicted": round(measured_us / pred, 3), "constants_from": CHAIN_FILE,
                "note": "a launch is bound by its stream's dependency chain: one producer -> consumer hand-off per link "
                        "on top of the vector-issue floor; the prediction excludes the launch's start and drain (~3 us)"}
    except Exception:
        return None


def host_cpu_share():
    """(usable cores, how that was found, CPU model string).  A container sees every hardware thread of the host in its
    affinity mask but is scheduled on a cgroup CPU quota (the GPU box: 256 threads visible, 16 cores' worth of quota);
    OpenMP teams larger than the quota only add contention (round 2's "all cores" figure was 262 updates/s at 256
    threads against 330 k at 16), so the baseline's "all host cores" run uses min(affinity, quota)."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota, how = None, "sched_getaffinity"
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                      # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = f.read().split()[:2]
            if q != "max":
                quota = max(1, int(float(q) / float(per) + 0.5))
    except Exception:
        try:                                                           # cgroup v1
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                quota = max(1, int(q / per + 0.5))
        except Exception:
            pass
    cores = aff
    if quota is not None and quota < aff:
        cores, how = quota, "cgroup cpu quota"
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.lower().startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except Exception:
        pass
    return cores, how, aff, model


def cpu_baseline(cfg, seed, budget_s=12.0):
    """The CPU oracle ("port") timed on this box's host cores on a bounded sample of the same workload."""
    import shutil
    import tempfile
    from oracle import oracle as O
    from oracle import torch_port
    tr, _, U0, V0 = make_workload(cfg, seed)
    B = cfg["B"]
    tmp = tempfile.mkdtemp(prefix="mfcd_orc_")
    try:
        try:
            lib = O.build(force=True, archflags="-march=native", out=os.path.join(tmp, "liborc_native.so"))
        except Exception:
            lib = O.build()
        orc = O.COracle(lib)
        ncpu, share_from, visible, cpu_model = host_cpu_share()
        results = {}
        # 1 thread, the reference's own 4 (structure.py:3), 16, and ALL usable host cores (the cgroup share when the box
        # exposes more hardware threads than it schedules; a box without a quota reports its affinity mask, capped at 64
        # threads: the sweep is 0.5 M elements per step and does not scale past that)
        for threads in sorted({1, min(ncpu, 4), min(ncpu, 16), min(ncpu, 64)}):
            st = O.new_state(U0, V0)
            probe = tr[: 32 * B]
            t0 = time.perf_counter()
            orc.train_steps(st, probe[:, 0], probe[:, 1], probe[:, 2], probe[:, 3], B, 0, lr=cfg["lr"], wd=cfg["wd"],
                            threads=threads)
            per = (time.perf_counter() - t0) / 32
            nsteps = int(max(64, min(200000, (budget_s / 4) / max(per, 1e-6))))
            reps = (nsteps * B + len(tr) - 1) // len(tr)
            sample = np.tile(tr, (reps, 1))[: nsteps * B]   # several epochs' worth of the same workload
            t0 = time.perf_counter()
            orc.train_steps(st, sample[:, 0], sample[:, 1], sample[:, 2], sample[:, 3], B, 32, lr=cfg["lr"],
                            wd=cfg["wd"], threads=threads)
            dt = time.perf_counter() - t0
            results[threads] = (len(sample) / dt, nsteps, dt)
        best = max(results, key=lambda k: results[k][0])
        # torch-op port at the reference's own OMP_NUM_THREADS=4 (structure.py:3), ~3 s
        old = torch.get_num_threads()
        torch.set_num_threads(min(4, ncpu))
        U, V = torch.from_numpy(U0.copy()), torch.from_numpy(V0.copy())
        state = {k: torch.zeros_like(U if k.endswith("U") else V) for k in ("mU", "vU", "mV", "vV")}
        nst = 600
        smp = tr[: nst * B]
        u, i, j = (torch.from_numpy(smp[:, c].astype(np.int64)) for c in range(3))
        z = torch.from_numpy(smp[:, 3].copy())
        torch_port.train_steps(U, V, state, u[:64 * 20], i[:64 * 20], j[:64 * 20], z[:64 * 20], B, 0)
        t0 = time.perf_counter()
        torch_port.train_steps(U, V, state, u, i, j, z, B, 20)
        tp = len(smp) / (time.perf_counter() - t0)
        torch.set_num_threads(old)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    v, nsteps, dt = results[best]
    allc = min(ncpu, 64)
    return {"value": round(v, 1), "unit": "triplet-updates/s", "cores": int(best), "kind": "port",
            "sample": f"{nsteps} optimiser steps (B={B}) of the {cfg.get('name', 'C2')} workload in {dt:.1f}s, C oracle "
                      f"(oracle/mfcd_oracle.c, -O3 -march=native, OpenMP Adam sweep); host has "
                      f"{ncpu} usable cores ({share_from}; {visible} hardware threads visible)",
            "cpu_model": cpu_model,
            "by_threads": {str(k): round(r[0], 1) for k, r in results.items()},
            "all_cores": {"cores": int(allc), "value": round(results[allc][0], 1), "from": share_from},
            "torch_op_port_4thr": round(tp, 1),
            "reference_vs_port": "profiles/r02_reference_vs_port_cpu.txt (build container: the unmodified reference's "
                                 "step time beside this port's, same data)"}


REAL_STDOUT_FD = None


class _StdoutToStderr:
    """Route fd 1 to stderr while the benchmark runs (RCCL prints a version banner on stdout) so that the ONE JSON
    line is the only thing this script ever writes to stdout."""

    def __enter__(self):
        global REAL_STDOUT_FD
        sys.stdout.flush()
        self.saved = os.dup(1)
        REAL_STDOUT_FD = self.saved      # for a watchdog that has to print the line from inside the run (mfcd/dist.py)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        global REAL_STDOUT_FD
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        REAL_STDOUT_FD = None
        return False


def clock_ramp(runner, seconds, call_steps=20):
    """UNTIMED, in front of the warm-up steps and the timed region: keep the chip busy for `seconds` with the same fused-step calls on a SCRATCH
    copy of the model (the measured model and its optimiser are not touched).  A GPU that has sat idle while the host
    prepared the inputs answers its first launches at idle clocks and wake-up latency (measured on this pool: the first
    20-step call after 0.5 s of idling takes 4-5x the time of the fortieth, tools/diag_short_calls.py); a benchmark of
    --steps 20 would measure that instead of the code.  Returns what was done, for the JSON line."""
    import copy
    engine, cfg = runner.engine, runner.cfg
    scratch = copy.deepcopy(runner.model)
    opt = torch.optim.Adam(scratch.parameters(), lr=cfg["lr"], weight_decay=cfg["wd"])
    bind = engine.AdamBinding(scratch, opt)
    saved = (runner.stream, runner.pos, runner.pre.pending, runner.gen.get_state())
    if runner.stream is None:       # the ramp walks the same code path as the timed region: Runner.run, events included
        runner.stream, runner.pos = runner.train.dev, 0
    t0 = time.perf_counter()
    calls = 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(16):
            runner.pos = 0
            runner.run(call_steps, record=True, bind=bind)
        calls += 16
        torch.cuda.synchronize()
        runner.event_pool.extend(e for a, b, _ in runner.train_events for e in (a, b))
        runner.reset_events()
    runner.stream, runner.pos, runner.pre.pending = saved[0], saved[1], saved[2]
    runner.gen.set_state(saved[3])
    return {"untimed": True, "seconds": round(time.perf_counter() - t0, 3), "calls": calls,
            "call_steps": call_steps,
            "what": f"{call_steps}-step fused calls (the timed region's call length) on a scratch copy of the model, directly "
                    "in front of the warm-up steps and the timed region"}


def uvt_record(dev, U2, V2):
    """Dense UV^T metric pass (mfcd_uvt_stats; d in {32, 64, 128, 256}: bf16x3 split product on the bf16 matrix pipe with fp32
    accumulation, fused epilogue, X read once) timed with HIP events at C2, C3 and C5 sizes: whole pass (every launch of
    the call, host syncs between groups of passes included).  Two rooflines beside each other: the X read against HBM
    (4 n m bytes, the pass's only large operand) and the three bf16 products against the dense bf16 MFMA peak; the
    nominal 2 n m d flops per second are kept for comparison with round 2's fp32-MFMA form (peak 157.3 TF)."""
    from mfcd import metrics
    out = {"hbm_peak_GBps": HBM_PEAK_GBS, "mfma_bf16_peak_TFLOPs": MFMA_BF16_PEAK_TF, "mfma_f32_peak_TFLOPs": MFMA_F32_PEAK_TF,
           "dtype": "f32 in / f32 out; products as three bf16 x bf16 -> f32 MFMAs (v_mfma_f32_32x32x16_bf16) on two-term "
                    "bf16 expansions of U and V (16 significant bits each)",
           "data": "synthetic (Gaussian X, U, V)"}
    shapes = [("C2", 4096, 4096, 64, 100), ("C3", 16384, 16384, 128, 10), ("C5", 100000, 20000, 256, 3)]   # passes per sync
    g = torch.Generator(device=dev).manual_seed(123)
    for name, n, m, d, reps in shapes:
        try:
            if name == "C2":
                U, V = U2, V2
            else:
                U = torch.randn(n, d, device=dev, generator=g) / d ** 0.5
                V = torch.randn(m, d, device=dev, generator=g) / d ** 0.5
            X = torch.empty(n, m, device=dev)
            for r0 in range(0, n, 8192):                       # generated in slabs: no second n x m temporary
                X[r0:r0 + 8192].normal_(0.0, 0.5, generator=g)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(what):
                """Average pass time over >= 0.25 s of back-to-back passes, after an untimed 0.25 s of the same (a chip
                that idled while X was generated runs its first passes 10-25 % slower: tools/exp_uvt_sustained.py)."""
                res = None
                for phase in range(2):
                    t0, k = time.perf_counter(), 0
                    e0.record()
                    while True:
                        for _ in range(reps):
                            res = metrics.uvt_stats(U, V, X, 1.0, what=what)
                        k += reps
                        torch.cuda.synchronize()
                        if time.perf_counter() - t0 >= 0.25:
                            break
                    e1.record()
                    torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / k, res

            def fractions(us):
                nominal = 2.0 * n * m * d / (us * 1e-6) / 1e12
                xgb = 4.0 * n * m / (us * 1e-6) / 1e9
                return {"pass_us": round(us, 1), "nominal_TFLOPs": round(nominal, 1),
                        "x_read_GBps": round(xgb, 1), "frac_of_hbm_peak": round(xgb / HBM_PEAK_GBS, 4),
                        "issued_bf16_TFLOPs": round(3 * nominal, 1),
                        "frac_of_bf16_mfma_peak": round(3 * nominal / MFMA_BF16_PEAK_TF, 4),
                        "vs_f32_mfma_peak": round(nominal / MFMA_F32_PEAK_TF, 4)}

            us, (rs, sc) = timed(3)
            out[name] = dict({"n": n, "m": m, "d": d}, **fractions(us))
            out[name]["finite"] = bool(torch.isfinite(sc[:2]).all().item())
            # the passes the two metric functions actually issue: rows only (compute_alpha_and_norm_ratios) and
            # global error only (compute_reconstruction_error), mfcd_uvt_stats_select
            for what, key in ((1, "rows_only"), (2, "error_only")):
                usw, _ = timed(what)
                out[name][key] = fractions(usw)
            del X
            torch.cuda.empty_cache()
        except Exception as e:   # a box with less free memory still reports the smaller shapes
            out[name] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return out


DUMP_LIMIT_BYTES = 60 << 20      # every file of a dump together, .npy headers included, stays under 64 MB


def dump_outputs(runner, out_dir):
    """--dump-outputs: what the timed path handed its caller after its last step, as float32 `out_dir/<name>.npy` —
    the factor tables U and V and the Adam moments of both (the fused step updates the caller's model and
    torch.optim.Adam state in place), and `loss`, the per-step batch-mean losses of the timed region's last call.
    When the tables would take the files past DUMP_LIMIT_BYTES in all (C4), each table keeps a fixed, seeded sample
    of its rows, the same in every run and for every table of the same height.  Returns a summary."""
    os.makedirs(out_dir, exist_ok=True)
    U, V, mU, vU, mV, vV = runner.bind.tensors()
    tables = {"U": U, "V": V, "U_exp_avg": mU, "U_exp_avg_sq": vU, "V_exp_avg": mV, "V_exp_avg_sq": vV}
    loss = runner.last_loss.float().cpu().numpy()
    table_bytes = sum(t.numel() * 4 for t in tables.values())
    keep = min(1.0, (DUMP_LIMIT_BYTES - loss.nbytes - 8 * 4096) / table_bytes)
    rows = {}
    for name, t in tables.items():
        n = t.shape[0]
        if keep < 1.0 and n not in rows:
            k = int(n * keep)
            rows[n] = torch.from_numpy(np.sort(np.random.default_rng(n).choice(n, k, replace=False))).to(t.device)
        a = (t.index_select(0, rows[n]) if keep < 1.0 else t).float().cpu().numpy()
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    np.save(os.path.join(out_dir, "loss.npy"), loss)
    return {"dir": out_dir, "files": sorted(tables) + ["loss"], "dtype": "float32",
            "rows_kept": "all" if keep >= 1.0 else {str(n): int(r.numel()) for n, r in rows.items()}}


def relaunch_multi_gpu(n_gpus):
    """`python bench.py --gpus N` outside torch.distributed.run: start N ranks ourselves (one process per GPU, RCCL over
    xGMI), relay rank 0's JSON line and exit with the children's status.  Runs BEFORE this process touches the GPU."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: the only mode this pool's driver supports
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{") and ln.rstrip().endswith("}")]
    if proc.returncode != 0 or not lines:
        sys.stderr.write(proc.stdout)
        raise SystemExit(proc.returncode or 1)
    print(lines[-1], flush=True)
    raise SystemExit(0)


def main():
    ap = build_parser()
    args = ap.parse_args()
    if args.dump_outputs and (args.gpus > 1 or args.dp_mode):
        ap.error("--dump-outputs covers the single-GPU path only (no --dp-mode, --gpus 1)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_multi_gpu(args.gpus)
    with _StdoutToStderr():
        out, is_printer = _run(args)
    if is_printer:
        print(json.dumps(out), flush=True)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10490)   # 10 epochs of C2
    ap.add_argument("--warmup", type=int, default=1049)   # 1 epoch
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: the kernel-only sample and its offline / "
                         "chain-model records, steady_state, uvt and cpu_baseline (multi-GPU: phase split, cost model, "
                         "C4 sub-record)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed (factor tables, Adam moments, the last call's "
                         "losses) as float32 DIR/<name>.npy; see dump_outputs()")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline record")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the steady_state and uvt records (profiling runs)")
    ap.add_argument("--steady-epochs", type=int, default=5, help="full epochs of the steady_state record (>= 3)")
    ap.add_argument("--clock-ramp", type=float, default=0.3, metavar="SECONDS",
                    help="untimed busy phase on scratch state in front of the timed region (0 = none); see clock_ramp()")
    ap.add_argument("--dp-mode", choices=["native", "allgather", "allreduce", "shard", "selftest"], default=None,
                    help="form of the multi-GPU path (default native: the loop inside libmfcd_hip.so with one RCCL "
                         "all-gather per step, global batch 64*R; allgather / allreduce: the per-step torch.distributed "
                         "loops; shard: row-sharded state, global batch 64, results equal to one GPU; selftest: "
                         "launcher + rendezvous only, gloo on CPU); given with --gpus 1 it rehearses that path on a "
                         "one-rank group")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="C2",
                    help="C2 (default): the configuration the metric is quoted on; C4: BASELINE.json configs[3], for "
                         "rehearsing the data-parallel path at the size it is named for")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tune", action="append", default=[], metavar="KNOB=VALUE",
                    help="experiment knob of include/mfcd.h (mfcd_set_tuning), e.g. --tune resident_lookahead=8; "
                         "tools/ sweeps only, every published number uses the defaults")
    ap.add_argument("--train-path", choices=["auto", "streaming", "resident", "local"], default="auto")
    ap.add_argument("--factor-dtype", choices=["f32", "bf16"], default="f32",
                    help="bf16: factor tables stored as bf16 (BASELINE configs[2]); moments and arithmetic stay fp32")
    return ap


def _run(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world and args.gpus > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with matching values (or without "
                         "torch.distributed.run: bench.py starts the ranks itself)")
    cfg = dict(WORKLOADS[args.workload])
    cfg["name"] = args.workload

    if args.dp_mode == "selftest":   # launcher + rendezvous check without a GPU (tests/test_dist_cpu.py)
        import torch.distributed as dist
        dist.init_process_group("gloo")
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        dist.barrier()
        dist.destroy_process_group()
        return {"metric": "launcher-selftest", "n_gpus": world, "sum_of_ranks_plus_one": float(t.item())}, rank == 0

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if world > 1 or args.dp_mode:
        import torch.distributed as dist
        from mfcd import dist as mdist
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        else:
            dist.init_process_group("nccl", device_id=dev)
        if args.tune:
            from mfcd import engine as _eng
            _eng.set_tuning(**{k: int(v) for k, v in (kv.split("=", 1) for kv in args.tune)})
        out = mdist.bench_data_parallel(cfg, dev, args.steps, args.warmup, args.seed, mode=args.dp_mode or "native",
                                        extras=args.full)
        dist.destroy_process_group()
        return out, rank == 0

    from mfcd import engine
    if args.tune:
        engine.set_tuning(**{k: int(v) for k, v in (kv.split("=", 1) for kv in args.tune)})
    engine.set_train_path(args.train_path)
    bf16 = args.factor_dtype == "bf16"
    runner = Runner(cfg, dev, args.seed, torch.bfloat16 if bf16 else torch.float32)
    # order: host-side build of the first epoch's record stream (the chip idles), the untimed clock ramp on a scratch copy
    # of the model, the W warm-up steps on the measured model, then the timed region.  The warm-up call sits directly in
    # front of the timed one: the first launch after the ramp's bursts of queued calls pays ~9 us of runtime housekeeping on
    # the host (tools/exp_driver_first.py), which is not part of a step
    runner.open_epoch()
    ramp = clock_ramp(runner, args.clock_ramp, max(1, min(args.steps, runner.steps_per_epoch))) if args.clock_ramp > 0 else None
    runner.run(args.warmup)
    torch.cuda.synchronize()
    runner.call_lengths = []
    t0 = time.perf_counter()
    # a HIP event pair around a call costs ~10 us of host + queue time (tools/exp_driver_call.py: 61 -> 51 us for the
    # driver's 20-step call): long runs are bracketed inside the timed region, a short one by an identical call right after
    in_region = args.steps >= 256
    consumed = runner.run(args.steps, record=in_region)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    engine.check_status()   # a resident launch that gave up on a bounded wait would invalidate the number
    timed_calls = runner.call_lengths
    dumped = dump_outputs(runner, args.dump_outputs) if args.dump_outputs else None
    if not in_region and args.full:
        runner.run(args.steps, record=True)
        torch.cuda.synchronize()

    launches = sum(k for _, _, k in runner.train_events)
    train_ms = sum(a.elapsed_time(b) for a, b, _ in runner.train_events)
    period_us = train_ms * 1e3 / max(launches, 1)          # HIP events around the fused-step calls, gaps included
    # the form the timed calls took: the longest call of the timed region decides what the record describes
    longest = max((k for _, _, k in runner.train_events), default=max(timed_calls))
    plan = engine.train_plan(min(longest * cfg["B"], runner.train.N), cfg["B"], cfg["n"], cfg["m"], cfg["d"], bf16=bf16)
    big = getattr(runner.bind, "_big", None)
    used_big = bool(big) and big.ws is not None and longest >= engine.BIG_MIN_STEPS     # engine.train_steps took csrc/big.hip
    if used_big:
        # (the library's plan describes its own forms; the arithmetic flavour is the resident forms' global switch)
        plan = dict(plan, form_name="big-resident", fast_math=engine.train_plan(64 * 300, 64, 4096, 4096, 64)["fast_math"])
    out = {
        "metric": "triplet-updates/sec", "value": round(consumed / dt, 1), "unit": "triplet-updates/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3 / args.steps, 6),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (bf16 factor storage)" if bf16 else "f32", "data": "synthetic",
        "config": {"workload": f"{cfg['name']}: n={cfg['n']} m={cfg['m']} d={cfg['d']} p={cfg['p']} K={cfg['K']} random triplets, "
                               f"B={cfg['B']}, Adam lr=1e-3 wd=1e-5, {runner.steps_per_epoch} steps/epoch + validation "
                               "pass per epoch", "global_batch": cfg["B"],
                   "train_samples": runner.train.N, "parallelism": "single", "step_form": plan["form_name"]},
    }
    kstep = kone = None
    # (the timed twin exists for the library's own forms; the big form is priced on the call)
    if args.full and not bf16 and not used_big:
        # the dominant kernel alone, for a call of the timed call's length: HIP event pair directly around its launch inside
        # the library (mfcd_train_steps_timed).  This is the figure a `rocprofv3 --kernel-trace --stats` of the same command
        # shows as that kernel's average duration, and what `achieved` / `frac` are priced on; `call_level` brackets the
        # whole call (prologue and batch-mean kernels and the gaps between the three launches included)
        klen = max(1, min(longest, runner.steps_per_epoch))
        kstep, _, _ = runner.kernel_sample(launches=klen)
        per_launch = 1 if plan["form_name"] == "streaming" else klen      # streaming: one launch per optimiser step
        kone = {"steps_per_launch": per_launch, "kernel_launch_us": round(kstep * per_launch, 2),
                "kernel_us_per_step": round(kstep, 4)}
    if runner.train_events:     # (a plain run of fewer than 256 steps records no event pair: no roofline without --full)
        out["roofline"] = roofline_record(cfg, plan, period_us, kernel_step_us=kstep)
        out["roofline"]["period_from"] = ("HIP event pairs around the calls of the timed region" if in_region else
                                          "HIP event pair around an identical call issued right after the timed region")
    if kone:
        off = offline_kernel_stats(cfg, plan, kone["steps_per_launch"])
        if off:
            kone["rocprof_offline"] = off
        cm = chain_model(cfg, plan, getattr(runner, "last_sample_records", None), klen, kone["kernel_launch_us"])
        if cm:
            kone["chain_model"] = cm
        out["roofline"]["kernel_only"] = kone
    if ramp:
        out["clock_ramp"] = ramp
    if dumped:
        out["outputs"] = dumped
    if args.full and not args.no_extras:
        # ---- steady state: whole epochs in this same process (what a training run sees; --steps may be far shorter) ----
        E = max(3, args.steady_epochs)
        runner.run(runner.steps_per_epoch - runner.pos if runner.stream is not None else 0)   # finish the open epoch
        runner.run(runner.steps_per_epoch)                                                     # one untimed epoch
        torch.cuda.synchronize()
        # two windows of E epochs each, back to back; the record is the faster one (both are listed): the host of the GPU
        # box is a shared 16-core slice, and a single multi-millisecond hiccup of the enqueueing thread (seen once in
        # round 3: 1.54 us/step of wall time over a window whose HIP events said 0.63) would otherwise be read as the code
        windows = []
        for _ in range(2):
            runner.reset_events()
            t1 = time.perf_counter()
            got = runner.run(E * runner.steps_per_epoch, record=True)
            torch.cuda.synchronize()
            dts_w = time.perf_counter() - t1
            engine.check_status()
            k_w = sum(k for _, _, k in runner.train_events)
            ev_w = sum(a.elapsed_time(b) for a, b, _ in runner.train_events) * 1e3 / max(k_w, 1)
            windows.append((got / dts_w, dts_w, ev_w, got))
            runner.event_pool.extend(e for a, b, _ in runner.train_events for e in (a, b))
        best = max(windows, key=lambda w: w[0])
        _, dts, ev_us, got = best
        splan = engine.train_plan(runner.train.N, cfg["B"], cfg["n"], cfg["m"], cfg["d"], bf16=bf16)
        kavg, kmin, kmax = (runner.kernel_sample(launches=min(512, runner.steps_per_epoch)) if not bf16 else
                            (ev_us, ev_us, ev_us))   # the timed twin exists for fp32 tables only
        out["steady_state"] = {
            "epochs": E, "steps": E * runner.steps_per_epoch, "value": round(got / dts, 1), "unit": "triplet-updates/s",
            "us_per_step_wall": round(dts * 1e6 / (E * runner.steps_per_epoch), 4),
            "us_per_step_events": round(ev_us, 4), "includes": "per-epoch shuffle, prologue, validation pass",
            "windows_updates_per_s": [round(w[0], 1) for w in windows],
            "step_form": splan["form_name"],
            "roofline": roofline_record(cfg, splan, ev_us, (kavg, kmin, kmax), kernel_step_us=None if bf16 else kavg)}
        out["uvt"] = uvt_record(dev, runner.model.U.data, runner.model.V.data)
    runner.bind.flush()     # (the Adam step counters were deferred; ADVICE r2: never leave them stale)
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, args.seed)
    return out, True


if __name__ == "__main__":
    main()
