"""Diagnostic: time the one-launch ratings fold-in (mfcd/ratings_foldin.py; csrc/ratings_foldin.hip) beside the lockstep
solver it restates (mfcd/ratings_exact.py: ratings_user_step with U = None) on the same inputs in the same process, and
write the table to profiles/ratings_fold_in.txt (or --out PATH).

  ml100k    bench_pair_ragged.py's MovieLens-100k-shaped synthetic table (943 x 1682, 100 000 entries), d = 16
  notebook  1000 x 1000 observed with p = 0.25, d = 2
  large     20 000 x 20 000, 2 M entries, long-tailed rows, d = 64; the longest row the kernel takes, alone
  widths    one row of 1024 entries at d = 1 .. 64: the time of a call with max_newton = 0 and info (one value pass and
            one Hessian pass) and without info (one value pass): what a Hessian pass costs per ordered pair in each form
  identity  --parent-lib PATH (a build of the parent commit): the existing pair entries hashed under both libraries
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported, the two solvers taking turns; the large table: wall time of one call, the second of two.
Usage: bench_ratings_fold_in.py [--out PATH] [--parent-lib PATH] [--parent-tree DIR] [--bench-runs N] [--skip-large]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pair_bench_common import SECONDS, alternated, bench_lines, identity_lines, wall  # noqa: E402
from bench_pair_ragged import long_tailed, ml100k_shaped, strided  # noqa: E402
from mfcd import ratings, ratings_exact, ratings_foldin  # noqa: E402
import structure as S  # noqa: E402

dev = torch.device("cuda:0")
L2, GTOL = 1e-3, 1e-3


def summary(res):
    st, it = res.status, res.newton_iters
    return (f"certified {float((st == 0).double().mean()):.3f}, stopped {float((st == 1).double().mean()):.3f}, refused "
            f"{float((st >= 2).double().mean()):.3f}; Newton iterations mean {float(it.double().mean()):.2f}, max {int(it.max())}; "
            f"objective {float(res.objective_before.sum()):.6f} -> {float(res.objective_after.nan_to_num().sum()):.6f}")


def compare(name, V, data, emit, timed=True):
    lock = lambda: ratings_exact.ratings_user_step(None, V, data, 1.0, L2, gtol=GTOL)    # noqa: E731
    kern = lambda: ratings_foldin.ratings_fold_in_users(None, V, data, 1.0, L2, gtol=GTOL)    # noqa: E731
    with_info = lambda: ratings_foldin.ratings_fold_in_users(None, V, data, 1.0, L2, gtol=GTOL, info=True)    # noqa: E731
    a, b = lock(), kern()
    if timed:
        ms = alternated([lock, kern, with_info])
    else:
        ms = [wall(fn)[1] for fn in (lock, kern, with_info)]
    both = (a.status == 0) & (b.status == 0)
    gap = float((a.rows - b.rows)[both].abs().max() / a.rows[both].abs().max()) if bool(both.any()) else float("nan")
    emit(f"  lockstep ratings_user_step: {ms[0]:9.3f} ms; {summary(a)}")
    emit(f"  one-launch kernel:          {ms[1]:9.3f} ms; {summary(b)}")
    emit(f"  kernel with info:           {ms[2]:9.3f} ms; lockstep / kernel {ms[0] / ms[1]:.1f}; largest difference of two "
         f"certified rows / largest entry {gap:.2e}")
    return b


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "ratings_fold_in.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_ratings_fold_in.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(1)
    # 1. MovieLens-100k-shaped
    u, i, v, n, m = ml100k_shaped(np.random.default_rng(0))
    data = ratings.RatingsData(u, i, v, n, m).to(dev)
    V = (torch.randn(m, 16, generator=g) / 4.0).to(dev)
    emit(f"ml100k-shaped: {n} x {m}, {data.entries} entries, {data.pairs} pairs, d = 16, N(0, 1/d) V, s = 1, l2 = {L2}, gtol = "
         f"{GTOL}; per user {data.lengths.min()} .. {data.lengths.max()}")
    compare("ml100k", V, data, emit)
    # 2. the notebooks' shape
    Ut, Vt = torch.randn(1000, 2, generator=g), torch.randn(1000, 2, generator=g)
    data = S.observe_ratings((Ut @ Vt.t()).to(dev), 0.25, levels=5)
    V = Vt.to(dev)
    emit(f"notebook: 1000 x 1000 observed with p = 0.25 in five levels, {data.entries} entries, {data.pairs} pairs, d = 2; per "
         f"user {data.lengths.min()} .. {data.lengths.max()}")
    compare("notebook", V, data, emit)
    # 3. large, long-tailed
    if "--skip-large" not in args:
        rng = np.random.default_rng(0)
        n = m = 20000
        cap = ratings_foldin.max_len()
        L = long_tailed(n, 2000000, 5, 5000, rng)
        u, i, v = strided(n, m, L, rng)
        data = ratings.RatingsData(u, i, v, n, m).to(dev)
        V = (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"large: {n} x {m}, {data.entries} entries, {data.pairs} pairs, d = 64; per user {L.min()} .. {L.max()} (median "
             f"{int(np.median(L))}), {int((L > cap).sum())} rows above the kernel's cap of {cap}; wall time of one call")
        res = compare("large", V, data, emit, timed=False)
        tail = int(np.argmax(np.where(L <= cap, L, 0)))
        sel = u == tail
        one = ratings.RatingsData(np.zeros(int(sel.sum()), np.int64), i[sel], v[sel], 1, m).to(dev)
        coef = 1.0 / data.support(False)
        fn = lambda: ratings_foldin.ratings_fold_in_users(None, V, one, 1.0, L2, coef=coef, gtol=GTOL)    # noqa: E731
        fn()
        alone, ms1 = wall(fn)
        emit(f"  the longest row taken ({int(L[tail])} entries) alone: {ms1:.3f} ms, {int(alone.newton_iters[0])} iterations, "
             f"status {int(alone.status[0])} (in the table: {int(res.newton_iters[tail])} iterations)")
    # 4. what a pass costs per ordered pair, by width
    emit("one row of 1024 entries (1 047 552 ordered pairs), one workgroup: a call with max_newton = 0, ms; Hessian pass = with "
         "info - without")
    rng = np.random.default_rng(2)
    one = ratings.RatingsData(np.zeros(1024, np.int64), np.arange(1024), rng.integers(1, 6, 1024).astype(np.float32), 1, 1024).to(dev)
    for d in (1, 2, 4, 5, 16, 17, 32, 33, 64):
        V = (torch.randn(1024, d, generator=g) / d ** 0.5).to(dev)
        U = torch.randn(1, d, generator=g).to(dev)
        ms = alternated([lambda: ratings_foldin.ratings_fold_in_users(U, V, one, 1.0, L2, coef=1e-6, max_newton=0),
                         lambda: ratings_foldin.ratings_fold_in_users(U, V, one, 1.0, L2, coef=1e-6, max_newton=0, info=True)])
        emit(f"  d = {d:2d}: value pass {ms[0]:.3f}, with the Hessian pass {ms[1]:.3f}; Hessian pass "
             f"{1024 * 1023 / (ms[1] - ms[0]) / 1e6:.2f} G ordered pairs/s per compute unit, value pass "
             f"{1024 * 1023 / ms[0] / 1e6:.2f} (launch and host time included)")
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
