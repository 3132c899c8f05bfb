"""Diagnostic: time the entry ranks of held-out ratings (mfcd/ranking.py: rank_entries; csrc/rank_entries.hip) beside the
same ranks by chunked torch ops in the same process, and write the table to profiles/ranking.txt (or --out PATH).

  ml100k    bench_pair_ragged.py's MovieLens-100k-shaped synthetic table (943 x 1682, 100 000 entries) split 0.8 / 0.2, d = 16
  large     20 000 x 20 000, 2 M entries, long-tailed rows, split 0.8 / 0.2, d = 64
  factored  n = m = 65 536, d = 64, 10 targets per user, 50 barred items per user
  torch form   per chunk of entries: the row block U[rows] @ V.T, barred columns set to -inf, one T x m comparison
               (row > t).sum() + ((row == t) & (column < t's)).sum()  — the padded form; its GEMM rounds differently, so the
               number of entries whose rank differs from the kernel's is reported, not asserted
  shares    the same rows in dense mode (prepare + count only, on a precomputed block of scores) against factor mode
            (slab + prepare + count): the difference is the score slab's write
  fill      lanes of a count workgroup that hold a target, over the tiles of the table's test rows
  identity  --parent-lib PATH (a build of the parent commit): mfcd_topk_rows hashed under both libraries
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported, the forms taking turns; the large torch forms: wall time of one call, the second of two.
Usage: bench_ranking.py [--out PATH] [--parent-lib PATH] [--parent-tree DIR] [--bench-runs N] [--skip-large] | --digest
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda:0")
TORCH_ELEMS = 1 << 27              # elements of the torch form's T x m temporaries per chunk


def torch_ranks(A, B, t_off, t_items, e_off, e_items):
    """The ranks by library ops, entries in chunks of at most TORCH_ELEMS / m (each chunk forms the score rows it needs)."""
    m = B.shape[0]
    entries = t_items.numel()
    row_of = torch.repeat_interleave(torch.arange(t_off.numel() - 1, device=dev), t_off[1:] - t_off[:-1])
    e_row = torch.repeat_interleave(torch.arange(e_off.numel() - 1, device=dev), e_off[1:] - e_off[:-1])
    cols = torch.arange(m, device=dev)
    rank = torch.empty(entries, dtype=torch.int64, device=dev)
    step = max(1, TORCH_ELEMS // m)
    for e0 in range(0, entries, step):
        e1 = min(entries, e0 + step)
        r0, r1 = int(row_of[e0]), int(row_of[e1 - 1]) + 1
        S = A[r0:r1] @ B.t()
        rows_e, t = row_of[e0:e1] - r0, t_items[e0:e1].long()
        st = S[rows_e, t]
        b0, b1 = int(e_off[r0]), int(e_off[r1])
        S[e_row[b0:b1] - r0, e_items[b0:b1].long()] = float("-inf")
        mine = S[rows_e]
        rank[e0:e1] = (mine > st[:, None]).sum(1) + ((mine == st[:, None]) & (cols[None, :] < t[:, None])).sum(1)
    return rank


def lane_fill(lengths):
    """Share of a count workgroup's 256 lanes that hold a target, over the tiles of rows of these target counts."""
    busy = tiles = 0
    for T in lengths:
        for p0 in range(0, int(T), 256):
            nt = min(256, int(T) - p0)
            busy += nt * (256 >> max(nt - 1, 0).bit_length())
            tiles += 1
    return busy / (256.0 * max(tiles, 1))


def compare(name, A, B, train, test, emit, timed=True, share_rows=None):
    from pair_bench_common import alternated, wall
    from mfcd import ranking
    kern = lambda: ranking.rank_entries((A, B), test, train)    # noqa: E731
    ref = lambda: torch_ranks(A, B, test.row_off, test.item, train.row_off, train.item)    # noqa: E731
    res, want = kern(), ref()
    differ = res.rank.long() != want
    if timed:
        ms = alternated([kern, ref])
    else:
        ms = [alternated([kern])[0], min(wall(ref)[1], wall(ref)[1])]
    emit(f"  mfcd_rank_entries: {ms[0]:10.3f} ms    torch form: {ms[1]:10.3f} ms    torch / kernel {ms[1] / ms[0]:.1f}")
    emit(f"  entries whose rank differs from the torch form's (its GEMM rounds the scores differently): {int(differ.sum())} of "
         f"{differ.numel()}, largest difference {int((res.rank.long() - want).abs().max()) if differ.numel() else 0}; status 0 "
         f"in {int((res.status == 0).sum())} of {res.status.numel()} rows")
    rows = torch.arange(A.shape[0] if share_rows is None else share_rows, device=dev)
    t_sub = ranking._csr(test, rows, rows.numel(), test.n, test.m, dev, "targets")
    e_sub = ranking._csr(train, rows, rows.numel(), test.n, test.m, dev, "exclude")
    X = A[:rows.numel()] @ B.t()
    fact = lambda: ranking.rank_entries((A, B), t_sub, e_sub, rows=rows)    # noqa: E731
    dense = lambda: ranking.rank_entries(X, t_sub, e_sub)    # noqa: E731
    ms = alternated([fact, dense])
    emit(f"  shares, rows 0 .. {rows.numel() - 1}: factor mode {ms[0]:.3f} ms, dense mode on precomputed scores (prepare + count) "
         f"{ms[1]:.3f} ms: the score slab is {100.0 * (ms[0] - ms[1]) / ms[0]:.0f} % of the call (host time of both included)")
    lengths = (test.row_off[1:] - test.row_off[:-1]).cpu().numpy()
    emit(f"  targets per row {lengths.min()} .. {lengths.max()} (median {int(np.median(lengths))}); lane fill of the count "
         f"workgroups {100.0 * lane_fill(lengths):.1f} %")


def _topk_digest():
    """sha256 of mfcd_topk_rows' outputs on edge shapes, both modes, all ends, exclusion lists, two slabs → one JSON line."""
    import ctypes
    from mfcd import _lib, topk
    lib = ctypes.CDLL(_lib.LIB_PATH)                    # a library of an earlier commit lacks the entries added since
    for name in [k for k in _lib.SIGNATURES if not hasattr(lib, k)]:
        del _lib.SIGNATURES[name]
    g = torch.Generator().manual_seed(1)
    out = {}

    def sha(res):
        h = hashlib.sha256()
        flat = []
        for part in res:
            flat += list(part) if isinstance(part, tuple) else [part]
        for t in flat:
            h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()

    for n, m, d, k in ((5, 1, 1, 1), (257, 1000, 3, 10), (300, 5000, 64, 100), (300, 5000, 100, 4097), (64, 40000, 256, 8192),
                       (500, 70001, 2, 7)):
        A, B = torch.randn(n, d, generator=g).to(dev), torch.randn(m, d, generator=g).to(dev)
        pairs = torch.stack((torch.randint(0, n, (4 * n,), generator=g), torch.randint(0, m, (4 * n,), generator=g)), 1)
        for mode, X in (("factor", (A, B)), ("dense", A @ B.t())):
            out[f"mfcd_topk_rows, {mode}, both ends, values @ {n} x {m}, d = {d}, k = {k}"] = sha(
                topk.topk_rows(X, k, ends="both", values=True))
            out[f"mfcd_topk_rows, {mode}, best, exclude @ {n} x {m}, d = {d}, k = {k}"] = sha(
                [topk.topk_rows(X, k, ends="best", exclude=pairs, values=True)])
            out[f"mfcd_topk_rows, {mode}, worst, rows @ {n} x {m}, d = {d}, k = {k}"] = sha(
                [topk.topk_rows(X, k, rows=torch.arange(n - 1, -1, -2), ends="worst")])
    print(json.dumps(out))


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        return _topk_digest()
    from pair_bench_common import SECONDS, bench_lines, identity_lines
    from bench_pair_ragged import long_tailed, ml100k_shaped, strided
    from mfcd import ratings
    out_path = os.path.join(ROOT, "profiles", "ranking.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_ranking.py: >= {SECONDS} s per stretch after an untimed "
             "stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(1)
    u, i, v, n, m = ml100k_shaped(np.random.default_rng(0))
    train, test = ratings.RatingsData(u, i, v, n, m).to(dev).split([0.8, 0.2])
    A, B = (torch.randn(n, 16, generator=g) / 4.0).to(dev), (torch.randn(m, 16, generator=g) / 4.0).to(dev)
    emit(f"ml100k-shaped: {n} x {m}, d = 16, {test.entries} held-out entries ranked, {train.entries} training entries barred")
    compare("ml100k", A, B, train, test, emit)
    if "--skip-large" not in args:
        rng = np.random.default_rng(0)
        n = m = 20000
        L = long_tailed(n, 2000000, 5, 5000, rng)
        u, i, v = strided(n, m, L, rng)
        train, test = ratings.RatingsData(u, i, v, n, m).to(dev).split([0.8, 0.2])
        A, B = (torch.randn(n, 64, generator=g) / 8.0).to(dev), (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"large: {n} x {m}, d = 64, {test.entries} held-out entries ranked, {train.entries} training entries barred; the "
             "torch form: wall time of one call")
        compare("large", A, B, train, test, emit, timed=False)
        n = m = 65536
        rng = np.random.default_rng(1)
        users = np.repeat(np.arange(n), 60)
        items = (rng.integers(0, m, n)[users] + np.tile(np.arange(60) * 1087, n)) % m      # 60 distinct items per user
        data = ratings.RatingsData(users, items, np.ones(users.size, np.float32), n, m).to(dev)
        train, test = data.split([5.0 / 6.0, 1.0 / 6.0])
        A, B = (torch.randn(n, 64, generator=g) / 8.0).to(dev), (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"factored: {n} x {m}, d = 64, {test.entries} entries ranked (10 per user), {train.entries} barred (50 per user); "
             "the torch form: wall time of one call; shares on the first 4096 rows (a dense 65 536^2 matrix is 16 GiB)")
        compare("factored", A, B, train, test, emit, timed=False, share_rows=4096)
    if "--parent-lib" in args:
        for line in identity_lines(args[args.index("--parent-lib") + 1], os.path.abspath(__file__), "mfcd_topk_rows"):
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
