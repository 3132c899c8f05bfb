"""Diagnostic: time the multi-column pair Laplacian kernel (mfcd/pairs.py: pair_hvp_multi_rows, pair_info_rows) beside d
calls of the single-vector kernel on the same rows in the same run, the direct user step beside the Newton-CG one
(mfcd/population.py: population_user_step, solver="direct" / "cg"), and write the table to profiles/pair_info.txt (or
--out PATH).

  kernels   1000 x 1000 with d = 2, C2 (4096 x 4096, d = 64), 256 rows of C5 width (20 000 columns) with d = 256; plain
            and under the full law of bench_pair_law.py; multi: one pair_hvp_multi_rows (Z alone; with deg; and
            pair_info_rows, which adds the f64 GEMM); single: one pair_hvp_rows / pair_law_hvp_rows, and d times that;
            the two forms take turns, stretch by stretch.  slots/pair: VALU issue slots per ordered pair implied by the
            rate at 1024 SIMDs x 32 lanes x 2.4 GHz; MFMA/pair: the fp32 matrix instructions the kernel issues per
            ordered pair by construction (not a counter).  No hardware counters are taken by this tool.
  steps     population_user_step with solver="cg" and solver="direct" on the same inputs in the same process, taking
            turns, at 1000 x 1000 (d = 2, l2 = 1e-4) and C2 (d = 64, l2 = 1e-5) from the model's random start with
            X = U* V*^T as in bench_pair_hvp.py: wall ms (min of two), Newton and CG iterations, statuses, the largest
            distance between the two solvers' rows
  identity  --parent-lib PATH (a libmfcd_hip.so built from the parent commit): the outputs of every pair entry
            (pair_bench_common.py: digest), hashed in a child process per library and compared
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 10490 --warmup 1049 in
            this tree and in DIR, taking turns, --bench-runs N runs each (default 3)

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  Usage: bench_pair_info.py [--out PATH] [--parent-lib PATH] [--parent-tree DIR] | --digest
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from pair_bench_common import (LANE_SLOTS_PER_S, ROOT, SECONDS, alternated, bench_lines, dev, digest, full_law,  # noqa: E402
                               identity_lines, wall)

from mfcd import pairs, population  # noqa: E402

KERNELS = (("notebooks 1000 x 1000", 1000, 1000, 2), ("C2 4096 x 4096", 4096, 4096, 64),
           ("C5 width 256 x 20000", 256, 20000, 256))
STEPS = (("notebooks 1000 x 1000 d=2", 1000, 1000, 2, 1e-4), ("C2 4096 x 4096 d=64", 4096, 4096, 64, 1e-5))


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        return digest()
    out_path = os.path.join(ROOT, "profiles", "pair_info.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_info.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds, the forms taking turns (HIP events)",
             "# multi: mfcd_pair_hvp_multi_rows, Z [rows, m, d] alone / with deg; info: pair_info_rows (multi + the f64 GEMM to "
             "[rows, d, d]); hvp: ONE mfcd_pair_hvp_rows / mfcd_pair_law_hvp_rows on the same rows, d x hvp: d times that",
             "# law: alpha / beta, margin 0.95 on standard-normal x, three labels; ratio: multi ms / (d x hvp ms); slots: VALU "
             "issue slots per ordered pair at 1024 SIMDs x 32 lanes x 2.4 GHz implied by the multi rate; MFMA/pair: fp32 matrix "
             "instructions per ordered pair by construction (chunks of d x tiles of 32 columns / 64); no counters taken",
             f"{'shape':22s} {'d':>4s} {'form':>5s} {'multi ms':>10s} {'+deg ms':>10s} {'info ms':>10s} {'hvp ms':>9s} "
             f"{'d x hvp ms':>11s} {'ratio':>6s} {'slots':>7s} {'MFMA/pair':>9s}"]
    print("\n".join(lines), flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(1)
    for name, rows, m, d in KERNELS:
        A, X, Y = (torch.randn(rows, m, generator=g).to(dev) for _ in range(3))
        B = torch.randn(m, d, generator=g).to(dev)
        law = full_law(m, g)
        npairs = rows * m * (m - 1)
        chunks = (d + 127) // 128
        mfma = chunks * (1 if d <= 32 else 2 if d <= 64 else 4) / 64.0
        for form, fns in (("plain", (lambda: pairs.pair_hvp_multi_rows(A, B), lambda: pairs.pair_hvp_rows(A, Y),
                                     lambda: pairs.pair_hvp_multi_rows(A, B, deg=True), lambda: pairs.pair_info_rows(A, B))),
                          ("law", (lambda: pairs.pair_hvp_multi_rows(A, B, X, law), lambda: pairs.pair_law_hvp_rows(A, X, Y, law),
                                   lambda: pairs.pair_hvp_multi_rows(A, B, X, law, deg=True),
                                   lambda: pairs.pair_info_rows(A, B, X, law)))):
            multi, single, withdeg, info = alternated(fns)
            torch.cuda.empty_cache()
            emit(f"{name:22s} {d:4d} {form:>5s} {multi:10.3f} {withdeg:10.3f} {info:10.3f} {single:9.3f} {d * single:11.3f} "
                 f"{multi / (d * single):6.3f} {LANE_SLOTS_PER_S / (npairs / (multi * 1e-3)):7.1f} {mfma:9.4f}")
        del A, X, Y, B, law
        torch.cuda.empty_cache()
    import structure as S
    for name, n, m, d, L2 in STEPS:
        Us, Vs = torch.randn(n, d, generator=g) / d ** 0.25, torch.randn(m, d, generator=g) / d ** 0.25
        X = (Us @ Vs.t()).to(dev)
        torch.manual_seed(n + d)
        model = S.MatrixFactorization(n, m, d).to(dev)
        U, V = model.U.data, model.V.data
        found = {"cg": [], "direct": []}
        for solver in found:
            population.population_user_step(U, V, X, 1.0, L2, max_newton=1, solver=solver)       # untimed
        for _ in range(2):
            for solver in found:
                found[solver].append(wall(lambda: population.population_user_step(U, V, X, 1.0, L2, solver=solver)))
        emit(f"# {name}, X = U* V*^T, l2 = {L2}: population_user_step from the model's random start, the solvers taking turns")
        for solver, runs in found.items():
            res, ms = runs[0][0], min(t for _, t in runs)
            st = torch.bincount(res.status, minlength=3).tolist()
            emit(f"#   solver={solver:6s} {ms:9.1f} ms (runs {', '.join(f'{t:.1f}' for _, t in runs)}): Newton iterations max "
                 f"{int(res.newton_iters.max())} (mean {float(res.newton_iters.float().mean()):.1f}), CG iterations max "
                 f"{int(res.cg_iters.max())}, rows with status 0 / 1 / 2: {st[0]} / {st[1]} / {st[2]}, largest grad_ratio "
                 f"{float(res.grad_ratio.max()):.2e}, sum of objective_after {float(res.objective_after.sum()):.9f}")
        a, b = found["cg"][0][0], found["direct"][0][0]
        emit(f"#   direct / cg time {min(t for _, t in found['direct']) / min(t for _, t in found['cg']):.3f}; largest "
             f"|row(direct) - row(cg)| {float((a.rows - b.rows).abs().max()):.2e} at largest |row| {float(a.rows.abs().max()):.2e}")
        del X, model
        torch.cuda.empty_cache()
    if "--parent-lib" in args:
        for line in identity_lines(args[args.index("--parent-lib") + 1]):
            emit(line)
    if "--parent-tree" in args:
        runs = int(args[args.index("--bench-runs") + 1]) if "--bench-runs" in args else 3
        for line in bench_lines(args[args.index("--parent-tree") + 1], runs):
            emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
