"""Diagnostic: time the pair Hessian-vector kernels (mfcd/pairs.py: pair_hvp_rows, pair_law_hvp_rows) beside the gradient
kernels of the same decomposition (pair_grad_rows, pair_law_grad_rows) in the same run, the table-level product and the
exact block steps built on them (mfcd/population.py), and write the table to profiles/pair_hvp.txt (or --out PATH).

  shapes    the notebooks' 1000 x 1000, C2 (4096 x 4096, all rows), 256 rows of C5 width (m = 20000)
  kernels   plain and under the full law of bench_pair_law.py (alpha / beta, a margin that admits about half of the
            pairs, three labels), each without and with deg; ratio: hvp ms / gradient ms of the same rows; slots/pair:
            VALU issue slots per ordered pair implied by the rate at 1024 SIMDs x 32 lanes x 2.4 GHz
  product   one population_hvp (exact: Hessian and gradient kernel, four GEMMs back), at 1000 x 1000 (d = 2) and C2 (d = 64)
  truth     for the product, the steps and the fit: X = U* V*^T with standard-normal factors of the model's rank scaled by
            d^(-1/4), so that X has unit-variance entries and a structure the model can fit; the model starts at its
            own random initialisation
  steps     one population_user_step and one population_item_step from the initial tables (their sum is one alternating
            sweep): wall ms, Newton and CG iterations, statuses
  fit       wall time and final F of fit_population_exact beside fit_population's 2000-step Adam run from the same start
            at 1000 x 1000, F = risk + (l2 / 2)(|U|^2 + |V|^2) taken by the same function for both
  identity  --parent-lib PATH (a libmfcd_hip.so built from the parent commit): the outputs of every pair entry
            (pair_bench_common.py: digest), hashed in a child process per library and compared

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  Usage: bench_pair_hvp.py [--out PATH] [--parent-lib PATH] | --digest
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from pair_bench_common import LANE_SLOTS_PER_S, ROOT, SECONDS, best, dev, digest, full_law, identity_lines, wall  # noqa: E402

from mfcd import pairs, population  # noqa: E402

CASES = (("notebooks 1000 x 1000", 1000, 1000), ("C2 4096 x 4096", 4096, 4096), ("C5 width 256 x 20000", 256, 20000))
# (name, n, m, d, l2): l2 is Adam's weight_decay; F holds it as a SUM over the table entries beside a MEAN risk, so the
# value at which the penalty of a fitted model stays below what the fit gains falls with the size of the tables
STEPS = (("notebooks 1000 x 1000 d=2", 1000, 1000, 2, 1e-4), ("C2 4096 x 4096 d=64", 4096, 4096, 64, 1e-5))


def objective(U, V, X, l2):
    with torch.no_grad():
        return float(pairs.population_risk(U, V, X, 1.0).double() + 0.5 * l2 * ((U.double() ** 2).sum() + (V.double() ** 2).sum()))


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        return digest()
    out_path = os.path.join(ROOT, "profiles", "pair_hvp.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_hvp.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds (HIP events)",
             "# grad: mfcd_pair_grad_rows / mfcd_pair_law_grad_rows; hvp, hvp+deg: mfcd_pair_hvp_rows / mfcd_pair_law_hvp_rows "
             "without and with deg, on the same rows; ordered pairs = rows x m (m - 1)",
             "# law: alpha / beta, margin 0.95 on standard-normal x, three labels; ratio: ms / grad ms; slots: VALU issue slots "
             "per ordered pair at 1024 SIMDs x 32 lanes x 2.4 GHz",
             f"{'shape':22s} {'form':>5s} {'grad ms':>9s} {'slots':>6s} {'hvp ms':>9s} {'ratio':>6s} {'slots':>6s} "
             f"{'hvp+deg ms':>10s} {'ratio':>6s} {'slots':>6s}"]
    print("\n".join(lines), flush=True)
    g = torch.Generator().manual_seed(1)
    for name, rows, m in CASES:
        A, X, Y = (torch.randn(rows, m, generator=g).to(dev) for _ in range(3))
        law = full_law(m, g)
        npairs = rows * m * (m - 1)
        for form, fns in (("plain", (lambda: pairs.pair_grad_rows(A, X, 1.0), lambda: pairs.pair_hvp_rows(A, Y),
                                     lambda: pairs.pair_hvp_rows(A, Y, True))),
                          ("law", (lambda: pairs.pair_law_grad_rows(A, X, law, 1.0),
                                   lambda: pairs.pair_law_hvp_rows(A, X, Y, law),
                                   lambda: pairs.pair_law_hvp_rows(A, X, Y, law, True)))):
            ms = [best(fn) for fn in fns]
            slots = [LANE_SLOTS_PER_S / (npairs / (t * 1e-3)) for t in ms]
            line = (f"{name:22s} {form:>5s} {ms[0]:9.3f} {slots[0]:6.1f} {ms[1]:9.3f} {ms[1] / ms[0]:6.2f} {slots[1]:6.1f} "
                    f"{ms[2]:10.3f} {ms[2] / ms[0]:6.2f} {slots[2]:6.1f}")
            print(line, flush=True)
            lines.append(line)
        del A, X, Y, law
        torch.cuda.empty_cache()
    import structure as S
    for name, n, m, d, L2 in STEPS:
        Us, Vs = torch.randn(n, d, generator=g) / d ** 0.25, torch.randn(m, d, generator=g) / d ** 0.25
        X = (Us @ Vs.t()).to(dev)
        torch.manual_seed(n + d)
        model = S.MatrixFactorization(n, m, d).to(dev)
        U, V = model.U.data, model.V.data
        dU, dV = torch.randn_like(U), torch.randn_like(V)
        hvp_ms = best(lambda: pairs.population_hvp(U, V, X, dU, dV))
        gn_ms = best(lambda: pairs.population_hvp(U, V, X, dU, dV, gauss_newton=True))
        population.population_user_step(U, V, X, 1.0, L2, max_newton=1)       # untimed
        ures, ums = wall(lambda: population.population_user_step(U, V, X, 1.0, L2))
        ires, ims = wall(lambda: population.population_item_step(ures.rows, V, X, 1.0, L2))
        st = torch.bincount(ures.status, minlength=3).tolist()
        for line in (
                f"# {name}, X = U* V*^T, l2 = {L2}: population_hvp {hvp_ms:.3f} ms exact, {gn_ms:.3f} ms Gauss-Newton",
                f"#   user step {ums:.1f} ms: Newton iterations max {int(ures.newton_iters.max())} (mean "
                f"{float(ures.newton_iters.float().mean()):.1f}), CG iterations max {int(ures.cg_iters.max())} (mean "
                f"{float(ures.cg_iters.float().mean()):.1f}), rows with status 0 / 1 / 2: {st[0]} / {st[1]} / {st[2]}, "
                f"largest grad_ratio {float(ures.grad_ratio.max()):.2e}",
                f"#   item step {ims:.1f} ms: Newton iterations {int(ires.newton_iters)}, CG iterations {int(ires.cg_iters)}, "
                f"status {int(ires.status)}, grad_ratio {float(ires.grad_ratio):.2e}; one alternating sweep "
                f"{ums + ims:.1f} ms, F {float(ures.objective_before.sum() + 0.5 * L2 * (V.double() ** 2).sum()):.6f} -> "
                f"{float(ires.objective_after + 0.5 * L2 * (ures.rows.double() ** 2).sum()):.6f} (risk of the ideal scores "
                f"{float(pairs.population_risk(Us.to(dev), Vs.to(dev), X, 1.0)):.6f})"):
            print(line, flush=True)
            lines.append(line)
        if n == 1000:
            U0, V0 = U.clone(), V.clone()
            for sweeps in (1, 3, 10):
                Ue, Ve = U0.clone(), V0.clone()
                res, ms = wall(lambda: population.fit_population_exact(Ue, Ve, X, 1.0, L2, sweeps))
                line = (f"#   fit_population_exact, {sweeps:2d} sweeps: {ms / 1e3:.3f} s wall, F {float(res.objective_start):.6f} -> "
                        f"{objective(Ue, Ve, X, L2):.6f}")
                print(line, flush=True)
                lines.append(line)
            opt = torch.optim.Adam(model.parameters(), lr=0.05, weight_decay=L2)
            _, ms = wall(lambda: pairs.fit_population((model, opt), X, 1.0, 2000))
            line = (f"#   fit_population, 2000 Adam steps (lr 0.05, weight_decay {L2}) from the same start: {ms / 1e3:.3f} s "
                    f"wall, F {objective(U0, V0, X, L2):.6f} -> {objective(model.U.data, model.V.data, X, L2):.6f}")
            print(line, flush=True)
            lines.append(line)
        del X, model
        torch.cuda.empty_cache()
    if "--parent-lib" in args:
        extra = identity_lines(args[args.index("--parent-lib") + 1])
        print("\n".join(extra), flush=True)
        lines += extra
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
