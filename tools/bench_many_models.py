"""Many small models per launch: structure.train_models (the batched local form, one CU per model) against the same
models trained one after another with train_model, at C1 (n = m = 256, d = 8, 1310 train records, B = 64) and at the
notebooks' default (n = m = 1000, d = 2, p = 0.5: 200 000 train records), for R in {1, 16, 64, 256}; then one
run_experiment(reps=8) end to end with and without set_concurrent_experiments(8).

  aggregate  triplet-updates/s = R * train records * epochs / host seconds (the timed work ends in a synchronise)
  kernel     device-event time of one mfcd_train_steps_local_multi call (prologue copy + training launch + batch
             means) divided by the steps of a model

    python tools/bench_many_models.py [--rs 1,16,64,256] [--epochs-c1 5] [--epochs-nb 1] [--skip-experiment]
One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import structure as S  # noqa: E402
from mfcd import _lib  # noqa: E402

CONFIGS = {"C1": dict(n=256, m=256, d=8, N=1310, Nv=163), "notebook": dict(n=1000, m=1000, d=2, N=200000, Nv=25000)}


class ArrayDataset(torch.utils.data.Dataset):
    def __init__(self, rows):
        self.data = rows

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, k):
        r = self.data[k]
        return int(r[0]), int(r[1]), int(r[2]), float(r[3])


def rows(rng, n, m, N):
    u, i = rng.integers(0, n, N), rng.integers(0, m, N)
    j = (i + 1 + rng.integers(0, m - 1, N)) % m
    return np.stack([u, i, j, rng.integers(0, 2, N)], 1).astype(np.float64)


def setup(cfg, R, seed):
    rng = np.random.default_rng(seed)
    n, m, d = cfg["n"], cfg["m"], cfg["d"]
    loaders = []
    for _ in range(R):
        tr = torch.utils.data.DataLoader(ArrayDataset(rows(rng, n, m, cfg["N"])), batch_size=64, shuffle=True)
        va = torch.utils.data.DataLoader(ArrayDataset(rows(rng, n, m, cfg["Nv"])), batch_size=64, shuffle=False)
        loaders.append((tr, va))
    return loaders


def fresh(cfg, R):
    models = [S.MatrixFactorization(cfg["n"], cfg["m"], cfg["d"]).to("cuda") for _ in range(R)]
    opts = [torch.optim.Adam(mo.parameters(), lr=1e-3, weight_decay=1e-5) for mo in models]
    return models, opts


class MultiTimer:
    """Device events around every mfcd_train_steps_local_multi call made through the bound library."""

    def __init__(self):
        self.L = _lib.load()
        self.orig = self.L.mfcd_train_steps_local_multi
        self.events = []

    def __enter__(self):
        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = self.orig(*args)
            e1.record()
            self.events.append((e0, e1))
            return rc
        self.L.mfcd_train_steps_local_multi = timed
        return self

    def __exit__(self, *exc):
        self.L.mfcd_train_steps_local_multi = self.orig

    def us(self):
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) * 1e3 for e0, e1 in self.events]


def bench_config(name, cfg, R, epochs):
    loaders = setup(cfg, R, seed=R)
    K = -(-cfg["N"] // 64)
    updates = R * cfg["N"] * epochs
    # warm-up: first launches, workspace planning, pinned staging
    models, opts = fresh(cfg, R)
    S.train_models(models, [t for t, _ in loaders], [v for _, v in loaders], opts, "cuda", num_epochs=1)
    S.train_model(models[0], loaders[0][0], loaders[0][1], opts[0], "cuda", num_epochs=1)
    torch.cuda.synchronize()

    models, opts = fresh(cfg, R)
    torch.cuda.synchronize()
    with MultiTimer() as mt:
        t0 = time.perf_counter()
        S.train_models(models, [t for t, _ in loaders], [v for _, v in loaders], opts, "cuda", num_epochs=epochs)
        torch.cuda.synchronize()
        dt_many = time.perf_counter() - t0
    call_us = mt.us()

    models, opts = fresh(cfg, R)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for mo, op, (tr, va) in zip(models, opts, loaders):
        S.train_model(mo, tr, va, op, "cuda", num_epochs=epochs)
    torch.cuda.synchronize()
    dt_serial = time.perf_counter() - t0
    rec = {"config": name, "R": R, "epochs": epochs, "train_records": cfg["N"], "steps_per_epoch": K,
           "many_s": round(dt_many, 5), "many_updates_per_s": round(updates / dt_many),
           "serial_s": round(dt_serial, 5), "serial_updates_per_s": round(updates / dt_serial),
           "speedup": round(dt_serial / dt_many, 2),
           "multi_call_us": round(float(np.median(call_us)), 2) if call_us else None,
           "multi_us_per_step": round(float(np.median(call_us)) / K, 3) if call_us else None}
    print(json.dumps(rec), flush=True)
    del models, opts, loaders
    torch.cuda.empty_cache()


def bench_experiment(name, kw, reps=8):
    out = {"experiment": name, "reps": reps, **{k: kw[k] for k in ("n", "m", "d", "p", "num_epochs")}}
    for k in (1, reps):
        S.set_concurrent_experiments(k)
        try:
            torch.manual_seed(0)
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            S.run_experiment(device="cuda", reps=reps, **kw)
            torch.cuda.synchronize()
            out[f"k{k}_s"] = round(time.perf_counter() - t0, 4)
        finally:
            S.set_concurrent_experiments(1)
    out["speedup"] = round(out["k1_s"] / out[f"k{reps}_s"], 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rs", default="1,16,64,256")
    ap.add_argument("--epochs-c1", type=int, default=5)
    ap.add_argument("--epochs-nb", type=int, default=1)
    ap.add_argument("--configs", default="C1,notebook")
    ap.add_argument("--skip-experiment", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import contextlib
    with contextlib.redirect_stderr(open(os.devnull, "w")):   # tqdm bars of train_model
        for name in a.configs.split(","):
            for R in (int(x) for x in a.rs.split(",")):
                bench_config(name, CONFIGS[name], R, a.epochs_c1 if name == "C1" else a.epochs_nb)
        if not a.skip_experiment:
            bench_experiment("C1", dict(n=256, m=256, d=8, p=0.05, s=1.0, lr=1e-3, weight_decay=1e-5, num_epochs=30))
            bench_experiment("notebook", dict(n=1000, m=1000, d=2, p=0.5, s=1.0, lr=1e-3, weight_decay=1e-5,
                                              num_epochs=3))


if __name__ == "__main__":
    main()
