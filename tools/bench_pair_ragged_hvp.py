"""Diagnostic: time the ragged pair Hessian-vector kernel and the exact ratings steps built on it (mfcd/ratings.py,
mfcd/ratings_exact.py) and write the table to profiles/pair_ragged_hvp.txt (or --out PATH).

  equal     4096 rows of L = 1024: pair_ragged_hvp without and with deg beside pair_ragged_grad, and beside the dense
            pair_hvp_rows / pair_grad_rows, on the same data in the same run
  ml100k    bench_pair_ragged.py's MovieLens-100k-shaped synthetic table (943 x 1682, 100 000 entries, d = 16): the same
            three ragged calls, and the same product by padded, masked, chunked torch ops
  steps     on that table: one exact user step, one exact item step and one sweep of fit_ratings_exact, wall time with
            Newton / CG iteration counts and the share of certified rows
  identity  --parent-lib PATH (a build of the parent commit): the existing pair entries hashed under both libraries
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  Usage: bench_pair_ragged_hvp.py [--out PATH] [--parent-lib PATH] [--parent-tree DIR] [--bench-runs N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pair_bench_common import alternated, bench_lines, identity_lines, wall  # noqa: E402
from bench_pair_ragged import D, SECONDS, TORCH_BYTES, ml100k_shaped  # noqa: E402
from mfcd import pairs, ratings, ratings_exact  # noqa: E402
import structure as S  # noqa: E402

dev = torch.device("cuda:0")
L2 = 1e-3


def torch_hvp(a_pad, y_pad, mask):
    """The ragged product by padded, masked library ops, rows in chunks of 1 GiB of L x L temporaries."""
    rows, k = a_pad.shape
    per = max(1, TORCH_BYTES // (k * k * 4))
    out = torch.empty_like(a_pad)
    for r0 in range(0, rows, per):
        a, y, w = a_pad[r0:r0 + per], y_pad[r0:r0 + per], mask[r0:r0 + per]
        p = torch.sigmoid(a[:, :, None] - a[:, None, :])
        s = p.mul_(1.0 - p).mul_(w[:, None, :])
        out[r0:r0 + per] = (s * (y[:, :, None] - y[:, None, :])).sum(2) * w
    return out


def kernel_line(tag, ms, pairs_):
    return (f"  {tag}: hvp {ms[0]:.3f} ms, hvp + deg {ms[1]:.3f} ms, gradient {ms[2]:.3f} ms; hvp / gradient {ms[0] / ms[2]:.3f}, "
            f"with deg {ms[1] / ms[2]:.3f}; hvp: {2 * pairs_ / ms[0] / 1e6:.1f} G ordered pairs/s")


def step_line(name, res, ms):
    status = res.status.reshape(-1)
    return (f"  {name}: {ms:.1f} ms; Newton iterations max {int(res.newton_iters.max())}, CG iterations max "
            f"{int(res.cg_iters.max())} (mean {float(res.cg_iters.double().mean()):.1f}); certified "
            f"{float((status == 0).double().mean()):.3f}, stopped {float((status == 1).double().mean()):.3f}; objective "
            f"{float(res.objective_before.sum()):.6f} -> {float(res.objective_after.sum()):.6f}")


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "pair_ragged_hvp.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_ragged_hvp.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    # 1. equal rows
    rows, m = 4096, 1024
    g = torch.Generator().manual_seed(1)
    A, X, Y = (1.5 * torch.randn(rows, m, generator=g)).to(dev), torch.randn(rows, m, generator=g).to(dev), \
        torch.randn(rows, m, generator=g).to(dev)
    data = S.observe_ratings(X, 1.0)
    a, y = A.reshape(-1).contiguous(), Y.reshape(-1).contiguous()
    rq, rd, _ = ratings.pair_ragged_hvp(a, y, data, deg=True)
    dq, dd = pairs.pair_hvp_rows(A, Y, True)
    same = torch.equal(rq.reshape(rows, m), dq), torch.equal(rd.reshape(rows, m), dd)
    ms = alternated([lambda: ratings.pair_ragged_hvp(a, y, data), lambda: ratings.pair_ragged_hvp(a, y, data, deg=True),
                     lambda: ratings.pair_ragged_grad(a, data, 1.0), lambda: pairs.pair_hvp_rows(A, Y),
                     lambda: pairs.pair_hvp_rows(A, Y, True), lambda: pairs.pair_grad_rows(A, X, 1.0)])
    n_pairs = rows * m * (m - 1) // 2
    emit(f"equal rows: {rows} rows of L = {m} ({n_pairs} pairs), ragged beside dense on the same data")
    emit(kernel_line("ragged", ms[:3], n_pairs))
    emit(kernel_line("dense ", ms[3:], n_pairs))
    emit(f"  ragged / dense: hvp {ms[0] / ms[3]:.3f}, hvp + deg {ms[1] / ms[4]:.3f} (q bit-equal: {same[0]}, deg bit-equal: {same[1]})")
    del A, X, Y, a, y, data, rq, rd, dq, dd
    torch.cuda.empty_cache()
    # 2. MovieLens-100k-shaped
    u, i, v, n, m = ml100k_shaped(np.random.default_rng(0))
    data = ratings.RatingsData(u, i, v, n, m).to(dev)
    torch.manual_seed(3)
    model = S.MatrixFactorization(n, m, D).to(dev)
    U, V = model.U.data, model.V.data
    a = ratings.ragged_scores(U, V, data)[0]
    y = torch.randn(data.entries, generator=g).to(dev)
    L = data.lengths
    emit(f"ml100k-shaped: {n} x {m}, {data.entries} entries, {data.pairs} pairs, d = {D}; per user {L.min()} .. {L.max()} "
         f"(median {int(np.median(L))}); tiles {data.n_tiles}")
    for skip in (False, True):
        ms = alternated([lambda: ratings.pair_ragged_hvp(a, y, data, skip), lambda: ratings.pair_ragged_hvp(a, y, data, skip, True),
                         lambda: ratings.pair_ragged_grad(a, data, 1.0, skip)])
        emit(kernel_line(f"skip_ties={skip}", ms, data.pairs))
        if not skip:
            plain = ms
    k = int(L.max())
    pos = torch.from_numpy(np.arange(data.entries) - np.repeat(np.cumsum(L) - L, L)).to(dev)
    at = data.user.long()
    a_pad, y_pad, mask = (torch.zeros((n, k), device=dev) for _ in range(3))
    a_pad[at, pos], y_pad[at, pos], mask[at, pos] = a, y, 1.0
    ref = torch_hvp(a_pad, y_pad, mask)[at, pos]
    err = float(((ratings.pair_ragged_hvp(a, y, data)[0] - ref).abs() / (L.max() - 1)).max())
    tms = min(wall(lambda: torch_hvp(a_pad, y_pad, mask))[1] for _ in range(3))
    emit(f"  the same product by padded ({n} x {k}), masked torch ops in chunks of 1 GiB: {tms:.3f} ms "
         f"({tms / plain[0]:.1f} x the kernel); largest difference of the mean term {err:.2e}")
    del a_pad, y_pad, mask, ref
    torch.cuda.empty_cache()
    # 3. the exact steps on the same table
    emit(f"exact steps on the ml100k-shaped table, N(0, 1/d) tables, s = 1, l2 = {L2}, gtol = 1e-3 (wall time of one call, the "
         "second of two)")
    for name, fn in (("user step", lambda: ratings_exact.ratings_user_step(U, V, data, 1.0, L2)),
                     ("item step", lambda: ratings_exact.ratings_item_step(U, V, data, 1.0, L2))):
        fn()
        res, ms1 = wall(fn)
        emit(step_line(name, res, ms1))
    fit, ms1 = wall(lambda: ratings_exact.fit_ratings_exact(U.clone(), V.clone(), data, 1.0, L2, 1))
    emit(f"  one sweep (fit_ratings_exact): {ms1:.1f} ms; F {float(fit.objective_start):.6f} -> "
         f"{fit.history[0, 0].item():.6f} -> {fit.history[0, 1].item():.6f}; users certified "
         f"{float((fit.user_status == 0).double().mean()):.3f}, item status {int(fit.item_status)}")
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
