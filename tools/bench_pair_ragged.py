"""Diagnostic: time the ragged pair kernels and the ratings step (mfcd/ratings.py) and write the table to
profiles/pair_ragged.txt (or --out PATH).

  equal     4096 rows of L = 1024: pair_ragged_grad / pair_ragged_stats beside the dense pair_grad_rows / pair_stats_rows on
            the same data in the same run; the per-pair work is the same, so the ratio is the cost of the ragged
            decomposition (256-entry tiles, one entry per thread, the row search, the validation kernel)
  ml100k    a MovieLens-100k-shaped synthetic table: 943 x 1682, 100 000 entries, 20 to 737 per user, long-tailed; one
            fused step split by call, the whole step from fit_ratings, and the same score gradient by padded, masked,
            chunked torch ops; the lane utilisation the length histogram implies at 256- and 1024-entry tiles
  large     20 000 x 20 000, 2 M entries, longest row about 5 000, one item rated by every user (an item cannot have more
            ratings than there are users: 79 segments); time per step and the gather-sums' share; and the item-side
            gather-sum alone on 120 000 users x 100 items with one item rated by all of them (469 segments)
  identity  --parent-lib PATH (a build of the parent commit): the existing pair entries hashed under both libraries
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  Usage: bench_pair_ragged.py [--out PATH] [--parent-lib PATH] [--parent-tree DIR] [--bench-runs N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pair_bench_common import alternated, bench_lines, identity_lines, stretch, wall  # noqa: E402
from mfcd import engine, pairs, ratings  # noqa: E402
import structure as S  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("PAIRS_BENCH_SECONDS", "0.5"))
D = 16
TORCH_BYTES = 1 << 30


def long_tailed(n, total, lo, hi, rng):
    """n lengths in [lo, hi] summing to `total`, log-normal."""
    w = np.exp(rng.normal(0.0, 1.0, n))
    L = np.clip(lo + w / w.sum() * (total - lo * n), lo, hi).astype(np.int64)
    while L.sum() != total:                               # spread the rounding over the rows that have room
        room = np.flatnonzero(L < hi) if L.sum() < total else np.flatnonzero(L > lo)
        pick = rng.choice(room, min(room.size, abs(int(total - L.sum()))), replace=False)
        L[pick] += 1 if L.sum() < total else -1
    return L


def ml100k_shaped(rng):
    n, m = 943, 1682
    L = long_tailed(n, 100000, 20, 737, rng)
    pop = 1.0 / (1.0 + np.arange(m)) ** 0.8
    pop /= pop.sum()
    items = np.concatenate([rng.choice(m, k, replace=False, p=pop) for k in L])
    return np.repeat(np.arange(n), L), items, rng.integers(1, 6, L.sum()).astype(np.float32), n, m


def strided(n, m, L, rng, everyone=True):
    """Row u rates L_u distinct items (offset_u + k step_u) mod m, step_u coprime with m; item 0 is rated by every row."""
    steps = np.array([s for s in range(1, 200) if np.gcd(s, m) == 1])
    users = np.repeat(np.arange(n), L)
    k = np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)
    off = rng.integers(1, m, n) if not everyone else np.zeros(n, dtype=np.int64)
    items = (off[users] + k * steps[rng.integers(0, steps.size, n)][users]) % m
    return users, items, rng.integers(1, 6, L.sum()).astype(np.float32)


def torch_grad(a_pad, x_pad, mask, s):
    """The ragged gradient by padded, masked library ops, rows in chunks of 1 GiB of L x L temporaries."""
    rows, k = a_pad.shape
    per = max(1, TORCH_BYTES // (k * k * 4))
    out = torch.empty_like(a_pad)
    for r0 in range(0, rows, per):
        a, x, w = a_pad[r0:r0 + per], x_pad[r0:r0 + per], mask[r0:r0 + per]
        t = torch.sigmoid(a[:, :, None] - a[:, None, :]).sub_(torch.sigmoid(s * (x[:, :, None] - x[:, None, :])))
        out[r0:r0 + per] = (t * w[:, None, :]).sum(2) * w
    return out


def utilisation(L, tile):
    return L.sum() / ((-(-L // tile)) * tile).sum()


def step_lines(name, data, emit, torch_form):
    g = torch.Generator().manual_seed(3)
    model = S.MatrixFactorization(data.n, data.m, D).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    U, V = model.U.data, model.V.data
    a = ratings.ragged_scores(U, V, data)[0]
    coef = torch.randn(data.entries, generator=g).to(dev)
    binding = engine.AdamBinding(model, opt)
    ratings.fit_ratings(binding, data, 1.0, 2)                                   # untimed: the optimizer's state exists
    calls = [lambda: ratings.ragged_scores(U, V, data), lambda: ratings.pair_ragged_grad(a, data, 1.0),
             lambda: ratings.ragged_gather_sum(coef, data, V, "user"), lambda: ratings.ragged_gather_sum(coef, data, U, "item"),
             lambda: ratings.pair_ragged_stats(a, data, 1.0, "both"), lambda: ratings.fit_ratings(binding, data, 1.0, 1)]
    ms = alternated(calls)
    L = data.lengths
    items = np.diff(data.col_off.cpu().numpy())
    emit(f"{name}: {data.n} x {data.m}, {data.entries} entries, {data.pairs} pairs, d = {D}; per user {L.min()} .. {L.max()} "
         f"(median {int(np.median(L))}), per item {items.min()} .. {items.max()}; tiles {data.n_tiles}, lane utilisation "
         f"{utilisation(L, 256):.3f} at 256-entry tiles ({utilisation(L, 1024):.3f} at 1024); of the waves that run the pair loops "
         f"{utilisation(L, 64):.3f}")
    emit(f"  ms per call: scores {ms[0]:.3f}, gradient {ms[1]:.3f}, gather-sum by user {ms[2]:.3f}, by item {ms[3]:.3f}, "
         f"stats (both) {ms[4]:.3f}; one fused step (fit_ratings, Adam included) {ms[5]:.3f}; gather-sums' share of the "
         f"step {(ms[2] + ms[3]) / ms[5]:.2f}; gradient: {2 * data.pairs / ms[1] / 1e6:.1f} G ordered pairs/s")
    if torch_form:
        k = int(L.max())
        pos = torch.from_numpy(np.arange(data.entries) - np.repeat(np.cumsum(L) - L, L)).to(dev)
        rows = data.user.long()
        a_pad, x_pad, mask = (torch.zeros((data.n, k), device=dev) for _ in range(3))
        a_pad[rows, pos], x_pad[rows, pos], mask[rows, pos] = a, data.value, 1.0
        ref = torch_grad(a_pad, x_pad, mask, 1.0)[rows, pos]
        got = ratings.pair_ragged_grad(a, data, 1.0)[0]
        err = float(((got - ref).abs() / (L.max() - 1)).max())
        tms = min(wall(lambda: torch_grad(a_pad, x_pad, mask, 1.0))[1] for _ in range(3))
        emit(f"  the same gradient by padded ({data.n} x {k}), masked torch ops in chunks of 1 GiB: {tms:.3f} ms "
             f"({tms / ms[1]:.1f} x the kernel); largest difference of the mean term {err:.2e}")
    emit("  packing several short rows (L <= 64) into one workgroup: not tried")


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "pair_ragged.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_ragged.py: >= {SECONDS} s per stretch after an untimed "
             "stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(0)
    # 1. equal rows
    rows, m = 4096, 1024
    g = torch.Generator().manual_seed(1)
    A, X = (1.5 * torch.randn(rows, m, generator=g)).to(dev), torch.randn(rows, m, generator=g).to(dev)
    data = S.observe_ratings(X, 1.0)
    a = A.reshape(-1).contiguous()
    same = torch.equal(ratings.pair_ragged_grad(a, data, 1.0)[0].reshape(rows, m), pairs.pair_grad_rows(A, X, 1.0))
    same_counts = torch.equal(ratings.pair_ragged_stats(a, data, 1.0, "counts")[0], pairs.pair_stats_rows(A, X, 1.0, "counts")[0])
    ms = alternated([lambda: ratings.pair_ragged_grad(a, data, 1.0), lambda: pairs.pair_grad_rows(A, X, 1.0),
                     lambda: ratings.pair_ragged_stats(a, data, 1.0, "both"), lambda: pairs.pair_stats_rows(A, X, 1.0, "both")])
    emit(f"equal rows: {rows} rows of L = {m} ({rows * m * (m - 1) // 2} pairs), ragged beside dense on the same data")
    emit(f"  gradient: ragged {ms[0]:.3f} ms, dense {ms[1]:.3f} ms, ratio {ms[0] / ms[1]:.3f} (gradients bit-equal: {same})")
    emit(f"  stats (both): ragged {ms[2]:.3f} ms, dense {ms[3]:.3f} ms, ratio {ms[2] / ms[3]:.3f} (counts equal: {same_counts})")
    del A, X, a, data
    torch.cuda.empty_cache()
    # 2. MovieLens-100k-shaped
    u, i, v, n, m = ml100k_shaped(rng)
    step_lines("ml100k-shaped", ratings.RatingsData(u, i, v, n, m).to(dev), emit, True)
    # 3. long-tailed large
    n = m = 20000
    L = long_tailed(n, 2000000, 5, 5000, rng)
    u, i, v = strided(n, m, L, rng)
    step_lines("large", ratings.RatingsData(u, i, v, n, m).to(dev), emit, False)
    n, m = 120000, 100
    u, i, v = strided(n, m, np.full(n, 10, dtype=np.int64), rng)
    data = ratings.RatingsData(u, i, v, n, m).to(dev)
    U = torch.randn(n, D, generator=g).to(dev)
    coef = torch.randn(data.entries, generator=g).to(dev)
    ms = stretch(lambda: ratings.ragged_gather_sum(coef, data, U, "item"), SECONDS)
    emit(f"gather-sum by item alone: {n} users x {m} items, {data.entries} entries, item 0 rated by all {n} users "
         f"({-(-n // 256)} segments), d = {D}: {ms:.3f} ms")
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
