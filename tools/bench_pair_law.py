"""Diagnostic: time the pair-law kernels (mfcd/pairs.py: pair_law_stats_rows, pair_law_grad_rows) beside the unweighted
kernels they are forms of (pair_stats_rows "sums", pair_grad_rows) in the same run, and one fused step of pairs.fit_law,
and write the table to profiles/pair_law.txt (or --out PATH).

  shapes   the notebooks' 1000 x 1000, C2 (4096 x 4096, all rows), 256 rows of C5 width (m = 20000)
  laws     full     alpha / beta (log-uniform in [1e-6, 1]), a margin that admits about half of the pairs, three labels
           weights  alpha / beta only
  ratio    weighted ms / unweighted ms of the same kernel on the same rows; slots/pair: VALU issue slots per pair the
           kernel visits (unordered for the sums, ordered for the gradient) implied by the rate at 1024 SIMDs x 32 lanes
           x 2.4 GHz
  step     one step of fit_law under the full law (score GEMM, kernel, two gradient GEMMs, mfcd_adam_dense), at
           1000 x 1000 (d = 2) and C2 (d = 64), beside one step of fit_population

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  Usage: bench_pair_law.py [--out PATH]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from pair_bench_common import LANE_SLOTS_PER_S, ROOT, SECONDS, best, dev  # noqa: E402

from mfcd import engine, pairs  # noqa: E402

CASES = (("notebooks 1000 x 1000", 1000, 1000), ("C2 4096 x 4096", 4096, 4096), ("C5 width 256 x 20000", 256, 20000))
STEPS = (("notebooks 1000 x 1000 d=2", 1000, 1000, 2), ("C2 4096 x 4096 d=64", 4096, 4096, 64))


def laws(m, g):
    """(full, weights only) for rows of m standard-normal columns: |x_i - x_j| <= 0.95 holds for about half of the pairs."""
    alpha, beta = (10.0 ** (-6.0 * torch.rand(m, generator=g)) for _ in range(2))
    labels = torch.randint(0, 3, (m,), generator=g)
    return (pairs.PairLaw(alpha=alpha, beta=beta, margin=0.95, labels=labels, device=dev),
            pairs.PairLaw(alpha=alpha, beta=beta, device=dev))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "pair_law.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_law.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds (HIP events)",
             "# sums: mfcd_pair_law_stats_rows beside mfcd_pair_stats_rows (what = sums), pairs = rows x m (m - 1) / 2; grad: "
             "mfcd_pair_law_grad_rows beside mfcd_pair_grad_rows, pairs = rows x m (m - 1)",
             "# full: alpha / beta, margin 0.95 on standard-normal x, three labels; weights: alpha / beta only; share: pairs "
             "with w > 0 under the full law",
             "# ratio: law ms / unweighted ms; slots/pair: VALU issue slots per visited pair at 1024 SIMDs x 32 lanes x "
             "2.4 GHz",
             f"{'shape':22s} {'kernel':>6s} {'plain ms':>9s} {'slots/pair':>10s} {'full ms':>9s} {'ratio':>6s} "
             f"{'slots/pair':>10s} {'weights ms':>10s} {'ratio':>6s} {'slots/pair':>10s} {'share':>6s}"]
    print("\n".join(lines), flush=True)
    g = torch.Generator().manual_seed(1)
    for name, rows, m in CASES:
        A = torch.randn(rows, m, generator=g).to(dev)
        X = torch.randn(rows, m, generator=g).to(dev)
        full, weights = laws(m, g)
        share = float(pairs.pair_law_stats_rows(A, X, full)[0].sum()) / (rows * m * (m - 1) / 2)
        for kernel, npairs, plain, law in (
                ("sums", rows * m * (m - 1) / 2, lambda: pairs.pair_stats_rows(A, X, 1.0, "sums"),
                 lambda w: pairs.pair_law_stats_rows(A, X, w, 1.0)),
                ("grad", rows * m * (m - 1), lambda: pairs.pair_grad_rows(A, X, 1.0),
                 lambda w: pairs.pair_law_grad_rows(A, X, w, 1.0))):
            ms = [best(plain), best(lambda: law(full)), best(lambda: law(weights))]
            slots = [LANE_SLOTS_PER_S / (npairs / (t * 1e-3)) for t in ms]
            line = (f"{name:22s} {kernel:>6s} {ms[0]:9.3f} {slots[0]:10.1f} {ms[1]:9.3f} {ms[1] / ms[0]:6.2f} {slots[1]:10.1f} "
                    f"{ms[2]:10.3f} {ms[2] / ms[0]:6.2f} {slots[2]:10.1f} {share:6.3f}")
            print(line, flush=True)
            lines.append(line)
        del A, X, full, weights
        torch.cuda.empty_cache()
    import structure as S
    for name, n, m, d in STEPS:
        X = torch.randn(n, m, generator=g).to(dev)
        model = S.MatrixFactorization(n, m, d).to(dev)
        binding = engine.AdamBinding(model, torch.optim.Adam(model.parameters(), lr=0.05))
        full, _ = laws(m, g)
        plain_ms = best(lambda: pairs.fit_population(binding, X, 1.0, 1))
        # fit_law computes the law's total weight once per call (one host wait): several steps per call, per-step time
        law_ms = best(lambda: pairs.fit_law(binding, X, 1.0, 8, full)) / 8
        line = (f"# step, {name}: fit_population {plain_ms:.3f} ms; fit_law under the full law {law_ms:.3f} ms per step "
                f"(calls of 8 steps, the total-weight pass included)")
        print(line, flush=True)
        lines.append(line)
        del X, model, binding, full
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
