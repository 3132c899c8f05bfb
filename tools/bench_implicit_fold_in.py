"""Diagnostic: time the one-launch implicit fold-in (mfcd/implicit_foldin.py; csrc/implicit_foldin.hip) beside the lockstep
solver it restates (mfcd/implicit_exact.py: implicit_user_step with U = None) on the same inputs in the same process, and
write the table to profiles/implicit_fold_in.txt (or --out PATH).

  ml100k    bench_pair_ragged.py's MovieLens-100k-shaped synthetic table (943 x 1682, 100 000 entries), d = 16: the fold-in
            of 256 new users (rows of the same table, as a CSR pair of their own, under the table's normaliser), and all
            943 users
  notebook  1000 x 1000 observed with p = 0.25, d = 2
  large     256 users of the 20 000 x 20 000, 2 M-entry long-tailed table, d = 64 
  factored  256 users of the 65 536-item shape with 10 observed items per user, d = 64 
  rates     one row (1024 observed of 8192 items: 7 340 032 pairs) with max_newton = 0, without info (one value-and-
            gradient pass) and with info (one more Hessian pass): the two pass rates on one compute unit, from which
            mfcd_implicit_fold_in_max_pairs() is set
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns; with
            --bench-swap the parent goes first in every second turn

Tables: zero start, item vectors N(0, 1/d), l2 = 1e-2 / n, gtol = 1e-3.  Timing as DESIGN 3.4: HIP events around >= SECONDS
of back-to-back calls after an untimed stretch, two rounds, both reported, the two solvers taking turns.
Usage: bench_implicit_fold_in.py [--out PATH] [--parent-tree DIR] [--bench-runs N] [--bench-swap] [--skip-large]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pair_bench_common import SECONDS, bench_lines, rounds  # noqa: E402
from bench_pair_ragged import long_tailed, ml100k_shaped, strided  # noqa: E402
from mfcd import implicit, implicit_exact, implicit_foldin, ratings  # noqa: E402

dev = torch.device("cuda:0")
GTOL = 1e-3


def summary(res):
    st, it = res.status.cpu().numpy(), res.newton_iters.cpu().numpy()
    return (f"certified {int((st == 0).sum())}, stopped {int((st == 1).sum())}, invalid {int((st == 2).sum())}, refused "
            f"{int((st == 3).sum())} of {st.size}; Newton iterations mean {it.mean():.2f}, max {int(it.max())}")


def compare(V, data, l2, coef, emit):
    lock = lambda: implicit_exact.implicit_user_step(None, V, data, l2, coef=coef, gtol=GTOL)    # noqa: E731
    kern = lambda: implicit_foldin.implicit_fold_in_users(None, V, data, l2, coef=coef, gtol=GTOL)    # noqa: E731
    a, b = lock(), kern()
    ms = rounds([lock, kern])
    both = (a.status == 0) & (b.status == 0)
    gap = float((a.rows - b.rows)[both].abs().max() / a.rows[both].abs().max()) if bool(both.any()) else float("nan")
    emit(f"  lockstep implicit_user_step: rounds {ms[0][0]:9.3f} {ms[0][1]:9.3f} ms; {summary(a)}; CG iterations in all "
         f"rows {int(a.cg_iters.sum())}")
    emit(f"  one-launch kernel:           rounds {ms[1][0]:9.3f} {ms[1][1]:9.3f} ms; {summary(b)}")
    spread = max(abs(ms[0][0] - ms[0][1]), abs(ms[1][0] - ms[1][1]))
    emit(f"  lockstep / kernel {min(ms[0]) / min(ms[1]):.2f} (min of the rounds); lockstep - kernel "
         f"{min(ms[0]) - min(ms[1]):.3f} ms against {spread:.3f} ms between a solver's two rounds; largest difference of two "
         f"certified rows / largest entry {gap:.2e}")
    return b


def table_coef(n, m, data):
    return float(implicit._Plan(n, m, dev, data, None, "pairs", None).coef64.max())


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "implicit_fold_in.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"# {torch.cuda.get_device_name(0)}, {cus} CUs; python tools/bench_implicit_fold_in.py: >= {SECONDS} s per stretch "
             "after an untimed stretch, two rounds, the solvers taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit(f"caps: max_pos {implicit_foldin.max_pos()}, max_pairs {implicit_foldin.max_pairs()}")
    g = torch.Generator().manual_seed(1)
    # 1. MovieLens-100k-shaped
    u, i, v, n, m = ml100k_shaped(np.random.default_rng(0))
    table = ratings.RatingsData(u, i, v, n, m).to(dev)
    data = (table.row_off, table.item)
    V = (torch.randn(m, 16, generator=g) / 4.0).to(dev)
    l2 = 1e-2 / n
    c = table_coef(n, m, data)
    emit(f"ml100k-shaped: {n} x {m}, {table.entries} observed entries, d = 16, N(0, 1/d) V, l2 = {l2:.3e}, gtol = {GTOL}, "
         f"coef = 1 / pairs = {c:.3e}")
    emit(" the fold-in of 256 new users:")
    compare(V, (data[0][:257].contiguous(), data[1]), l2, c, emit)
    emit(" all 943 users:")
    compare(V, data, l2, c, emit)
    # 2. the notebooks' shape
    n = m = 1000
    mask = torch.rand(n, m, generator=g) < 0.25
    uu, ii = mask.nonzero(as_tuple=True)
    table = ratings.RatingsData(uu.numpy(), ii.numpy(), np.ones(uu.numel(), np.float32), n, m).to(dev)
    data = (table.row_off, table.item)
    V = (torch.randn(m, 2, generator=g) / 2.0 ** 0.5).to(dev)
    emit(f"notebook: 1000 x 1000 observed with p = 0.25, {table.entries} entries, d = 2, l2 = {1e-2 / n:.3e}")
    compare(V, data, 1e-2 / n, table_coef(n, m, data), emit)
    if "--skip-large" not in args:
        # 3. 256 users of the large, long-tailed table
        rng = np.random.default_rng(0)
        n = m = 20000
        L = long_tailed(n, 2000000, 5, 5000, rng)
        u, i, v = strided(n, m, L, rng)
        table = ratings.RatingsData(u, i, v, n, m).to(dev)
        data = (table.row_off, table.item)
        V = (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        c = table_coef(n, m, data)
        pn = L[:256].astype(np.int64) * (m - L[:256])
        emit(f"large: 256 users of {n} x {m}, {table.entries} entries, d = 64, l2 = {1e-2 / n:.3e}; observed per user "
             f"{L[:256].min()} .. {L[:256].max()} (median {int(np.median(L[:256]))}), pairs per user up to {pn.max()}, "
             f"{int((pn > implicit_foldin.max_pairs()).sum())} users above the pairs cap")
        compare(V, (data[0][:257].contiguous(), data[1]), 1e-2 / n, c, emit)
        # 4. 256 users of the factored shape
        n = m = 65536
        rng = np.random.default_rng(1)
        users = np.repeat(np.arange(256), 10)
        items = (rng.integers(0, m, 256)[users] + np.tile(np.arange(10) * 1087, 256)) % m      # 10 distinct items per user
        table = ratings.RatingsData(users, items, np.ones(users.size, np.float32), 256, m).to(dev)
        V = (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        c = 1.0 / (n * 10.0 * (m - 10))                      # the whole table's 1 / pairs
        emit(f"factored: 256 users of {n} x {m}, 10 observed items per user, d = 64, l2 = {1e-2 / n:.3e}, coef = {c:.3e}")
        compare(V, (table.row_off, table.item), 1e-2 / n, c, emit)
    # 5. the two pass rates on one compute unit
    m, npos = 8192, 1024
    pairs = npos * (m - npos)
    one = (torch.tensor([0, npos], dtype=torch.int64, device=dev), torch.arange(0, 8 * npos, 8, dtype=torch.int32, device=dev))
    emit(f"one row of {npos} observed items among {m} ({pairs} pairs), one workgroup: a call with max_newton = 0, ms, min of two "
         "rounds (launch and host time included)")
    for d in (2, 16, 32, 64):
        V = (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
        U = torch.randn(1, d, generator=g).to(dev)
        ms = [min(r) for r in rounds(
            [lambda: implicit_foldin.implicit_fold_in_users(U, V, one, 1e-3, coef=1e-7, max_newton=0),
             lambda: implicit_foldin.implicit_fold_in_users(U, V, one, 1e-3, coef=1e-7, max_newton=0, info=True)])]
        hess = ms[1] - ms[0]
        emit(f"  d = {d:2d}: value pass {ms[0]:.3f}, with the Hessian pass {ms[1]:.3f}; value pass {pairs / ms[0] / 1e6:.3f} G "
             f"pairs/s, Hessian pass {pairs / hess / 1e6:.3f} G pairs/s on one compute unit; one of each "
             f"{(ms[0] + hess) * 1e6 / pairs:.3f} ns per pair; pairs in 1 s at max_newton = 20: "
             f"{pairs / (20 * (ms[0] + hess) * 1e-3):.3e}")
    if "--parent-tree" in args:
        runs = int(args[args.index("--bench-runs") + 1]) if "--bench-runs" in args else 3
        for line in bench_lines(args[args.index("--parent-tree") + 1], runs, "--bench-swap" in args):
            emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
