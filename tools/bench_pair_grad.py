"""Diagnostic: time mfcd_pair_grad_rows (mfcd/pairs.py: pair_grad_rows) and one fused step of pairs.fit_population
against a chunked torch formulation of the same gradient, and write the table to profiles/pair_grad.txt (or --out PATH).

  shapes   the notebooks' 1000 x 1000 with d = 2, C2 (4096 x 4096, d = 64)
  kernel   pair_grad_rows on given score / truth rows
  step     one step of fit_population: score GEMM, pair_grad_rows, two gradient GEMMs, mfcd_adam_dense
  torch    sigmoid(a[:, :, None] - a[:, None, :]) - sigmoid(scale (x[:, :, None] - x[:, None, :])) summed over j, over
           as many rows per block as keep four fp32 temporaries of that shape within 1 GiB; it does not use the entry.
           Measured on about TORCH_SECONDS of blocks and scaled to the shape's rows
  fit      wall time of a 2000-step fit at the notebooks' size (one host wait, at the end)

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  `--kernel-only N` issues N calls of pair_grad_rows at 1000 x 1000 and nothing else (the target of a
counters-only rocprofv3 --pmc pass).  Usage: bench_pair_grad.py [--out PATH] [--kernel-only N]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from pair_bench_common import LANE_SLOTS_PER_S, ROOT, SECONDS, dev, stretch  # noqa: E402

from mfcd import engine, pairs  # noqa: E402

TORCH_SECONDS = float(os.environ.get("PAIRS_BENCH_TORCH_SECONDS", "1.0"))
TEMP_ELEMS = (1 << 30) // (4 * 4)                 # four fp32 temporaries within 1 GiB
CASES = (("notebooks 1000 x 1000 d=2", 1000, 1000, 2), ("C2 4096 x 4096 d=64", 4096, 4096, 64))


def torch_grad(A, X, scale, budget_s):
    """The torch formulation over the first rows for about `budget_s` seconds → (rows done, seconds, G of those rows)."""
    rows, m = A.shape
    rper = max(1, TEMP_ELEMS // (m * m))
    out = []
    torch.cuda.synchronize()
    start = time.perf_counter()
    r0 = 0
    while r0 < rows:
        a, x = A[r0:r0 + rper], X[r0:r0 + rper]
        t = torch.sigmoid(a[:, :, None] - a[:, None, :]) - torch.sigmoid(scale * (x[:, :, None] - x[:, None, :]))
        out.append(t.sum(2))                                     # the diagonal is 0.5 - 0.5
        r0 = min(rows, r0 + rper)
        torch.cuda.synchronize()
        if time.perf_counter() - start >= budget_s:
            break
    return r0, time.perf_counter() - start, torch.cat(out)


def model_and_truth(n, m, d, lr=0.05):
    import structure as S
    g = torch.Generator(device=dev).manual_seed(n + m + d)
    X = torch.randn(n, m, device=dev, generator=g)
    model = S.MatrixFactorization(n, m, d).to(dev)
    return model, torch.optim.Adam(model.parameters(), lr=lr), X


def main():
    args = sys.argv[1:]
    if "--kernel-only" in args:
        calls = int(args[args.index("--kernel-only") + 1])
        model, _, X = model_and_truth(1000, 1000, 2)
        A = (model.U.data @ model.V.data.t()).contiguous()
        for _ in range(calls):
            pairs.pair_grad_rows(A, X, 1.0)
        torch.cuda.synchronize()
        return
    out_path = os.path.join(ROOT, "profiles", "pair_grad.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_grad.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds (HIP events)",
             "# kernel: mfcd_pair_grad_rows alone; step: one step of pairs.fit_population (score GEMM, kernel, two gradient "
             "GEMMs, mfcd_adam_dense)",
             f"# torch: chunked broadcast differences, four fp32 temporaries within 1 GiB, about {TORCH_SECONDS} s of blocks "
             "after an untimed block, scaled to all rows",
             "# ordered pairs: rows x m x (m - 1), what the kernel visits; slots/pair: VALU issue slots per ordered pair "
             "implied by the rate at 1024 SIMDs x 32 lanes x 2.4 GHz",
             "# ratio: torch ms / kernel ms; max dev: largest difference between the two gradients on the rows torch ran, "
             "per pair (divided by m - 1)",
             f"{'shape':26s} {'ordered pairs':>13s} {'kernel ms':>10s} {'rounds':>17s} {'Gpairs/s':>9s} {'slots/pair':>10s} "
             f"{'step ms':>9s} {'torch ms':>10s} {'rows run':>8s} {'ratio':>8s} {'max dev':>9s}"]
    print("\n".join(lines), flush=True)
    for name, n, m, d in CASES:
        model, opt, X = model_and_truth(n, m, d)
        A = (model.U.data @ model.V.data.t()).contiguous()
        ours = lambda: pairs.pair_grad_rows(A, X, 1.0)  # noqa: E731
        binding = engine.AdamBinding(model, opt)
        step = lambda: pairs.fit_population(binding, X, 1.0, 1)  # noqa: E731
        torch_grad(A, X, 1.0, 0.0)
        rounds, steps, tdone = [], [], []
        for _ in range(2):
            stretch(ours, SECONDS)
            rounds.append(stretch(ours, SECONDS))
            stretch(step, SECONDS / 2)
            steps.append(stretch(step, SECONDS))
            tdone.append(torch_grad(A, X, 1.0, TORCH_SECONDS))
        ms = min(rounds)
        nrun, secs, tg = min(tdone, key=lambda t: t[1] / t[0])
        torch_ms = secs / nrun * n * 1e3
        dev_max = float((ours()[:nrun] - tg).abs().max()) / (m - 1)
        npairs = n * m * (m - 1)
        rate = npairs / (ms * 1e-3)
        line = (f"{name:26s} {npairs:13.3e} {ms:10.3f} {rounds[0]:8.3f}/{rounds[1]:8.3f} {rate / 1e9:9.1f} "
                f"{LANE_SLOTS_PER_S / rate:10.1f} {min(steps):9.3f} {torch_ms:10.1f} {nrun:8d} {torch_ms / ms:7.1f}x "
                f"{dev_max:9.2e}")
        print(line, flush=True)
        lines.append(line)
        del model, opt, X, A, binding, step, ours
        torch.cuda.empty_cache()
    model, opt, X = model_and_truth(1000, 1000, 2)
    pairs.fit_population((model, opt), X, 1.0, 20)                # untimed
    torch.cuda.synchronize()
    start = time.perf_counter()
    at, risks = pairs.fit_population((model, opt), X, 1.0, 2000, log_every=500)
    torch.cuda.synchronize()
    wall = time.perf_counter() - start
    line = (f"# fit: 2000 steps at 1000 x 1000, d = 2, Adam lr 0.05, log_every 500: {wall:.3f} s wall "
            f"({wall / 2000 * 1e3:.3f} ms per step); risk after {at} steps: {[round(r, 6) for r in risks]}")
    print(line, flush=True)
    lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
