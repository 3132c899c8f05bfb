"""What the bench_pair*.py tools share: the timing loops, the full law they time under, and the comparison
of a build against a build of the parent commit.

  stretch, rounds, alternated, best, wall   HIP-event and wall-clock timing
  full_law                          alpha / beta over six decades, margin 0.95, three labels
  digest                            sha256 of the outputs of every pair entry → one JSON line: the six dense entries
                                    (statistics as counts, sums and both; the Hessian-vector entries with and without
                                    deg), mfcd_pair_hvp_multi_rows, mfcd_pair_best_rows and the three ragged entries
                                    (with and without skip-ties and deg), on edge shapes, on inputs long enough for a
                                    second launch block of every host loop, and on the three shapes the tools time
  identity_lines                    `digest` (or another tool's --digest) under the library in use and under a parent
                                    build, one child process each
  bench_lines                       bench.py in this tree and in a built checkout of the parent, taking turns

Usage of its own: pair_bench_common.py --digest (the library is MFCD_LIB, or the tree's).
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mfcd import pairs  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("PAIRS_BENCH_SECONDS", "0.5"))
LANE_SLOTS_PER_S = 1024 * 32 * 2.4e9              # VALU lanes x nominal clock
SHAPES = (("notebooks 1000 x 1000", 1000, 1000), ("C2 4096 x 4096", 4096, 4096), ("C5 width 256 x 20000", 256, 20000))


def stretch(fn, seconds):
    """Milliseconds per call over at least `seconds` of back-to-back calls (HIP events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total, per = 0, 0.0, 1
    while total < seconds * 1e3:
        t0.record()
        for _ in range(per):
            fn()
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        total += ms
        calls += per
        per = max(1, min(64, int(per * 0.05 * 1e3 / max(ms, 1e-3))))
    return total / calls


def rounds(fns):
    """Per function the ms per call of its two rounds' stretches, the functions taking turns within a round."""
    found = [[] for _ in fns]
    for _ in range(2):
        for k, fn in enumerate(fns):
            stretch(fn, SECONDS / 2)
            found[k].append(stretch(fn, SECONDS))
    return found


def alternated(fns):
    """min over two rounds of every function's stretch, the functions taking turns within a round."""
    return [min(t) for t in rounds(fns)]


def best(fn):
    """min over two rounds of one function's stretch."""
    return alternated([fn])[0]


def full_law(m, g, rows=None):
    """The law the tools time under; rows: one label row per row of the call instead of one for all."""
    alpha, beta = (10.0 ** (-6.0 * torch.rand(m, generator=g)) for _ in range(2))
    labels = torch.randint(0, 3, (m,) if rows is None else (rows, m), generator=g)
    return pairs.PairLaw(alpha=alpha, beta=beta, margin=0.95, labels=labels, device=dev)


def wall(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - start) * 1e3


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def _dense(out, tag, A, X, Y, laws):
    """The six dense entries on one set of rows."""
    out[f"mfcd_pair_stats_rows @ {tag}"] = _sha(*(t for what in ("both", "counts", "sums")
                                                  for t in pairs.pair_stats_rows(A, X, 1.0, what) if t is not None))
    out[f"mfcd_pair_grad_rows @ {tag}"] = _sha(pairs.pair_grad_rows(A, X, 1.0))
    out[f"mfcd_pair_hvp_rows @ {tag}"] = _sha(*pairs.pair_hvp_rows(A, Y, True), pairs.pair_hvp_rows(A, Y))
    for name, law in laws.items():
        out[f"mfcd_pair_law_stats_rows, {name} @ {tag}"] = _sha(*pairs.pair_law_stats_rows(A, X, law, 1.0))
        out[f"mfcd_pair_law_grad_rows, {name} @ {tag}"] = _sha(pairs.pair_law_grad_rows(A, X, law, 1.0))
        out[f"mfcd_pair_law_hvp_rows, {name} @ {tag}"] = _sha(*pairs.pair_law_hvp_rows(A, X, Y, law, True),
                                                               pairs.pair_law_hvp_rows(A, X, Y, law))


def _tables(out, tag, rows, k, d, g, law, entries):
    """mfcd_pair_hvp_multi_rows without an index, with one for all rows and with one per row; mfcd_pair_best_rows with
    one table for all rows and with one per row; each plain and under `law`."""
    A, X = (torch.randn(rows, k, generator=g).to(dev) for _ in range(2))
    B = torch.randn(k + 3, d, generator=g).to(dev)
    G = torch.randn(rows, k, d, generator=g).to(dev)
    index = torch.randint(0, k + 3, (rows, k), generator=g)
    for form, x, lw in (("plain", None, None), ("full law", X, law)):
        if "mfcd_pair_hvp_multi_rows" in entries:
            for what, b, ix in (("no index", B[:k], None), ("one index", B, index[0]), ("index per row", B, index)):
                out[f"mfcd_pair_hvp_multi_rows, {form}, {what} @ {tag}"] = _sha(
                    *pairs.pair_hvp_multi_rows(A, b, x, lw, ix, True), pairs.pair_hvp_multi_rows(A, b, x, lw, ix))
        if "mfcd_pair_best_rows" in entries:
            for what, tbl in (("one table", G[0]), ("table per row", G)):
                out[f"mfcd_pair_best_rows, {form}, {what} @ {tag}"] = _sha(*pairs.pair_best_rows(A, tbl, x, lw))


def _ragged(out, tag, lengths, g):
    """The three ragged entries on a table whose user u rates items 0 .. lengths[u] - 1 with one of five values."""
    from mfcd import ratings
    lengths = np.asarray(lengths, dtype=np.int64)
    users = np.repeat(np.arange(lengths.size), lengths)
    items = np.arange(users.size) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    values = torch.randint(1, 6, (users.size,), generator=g).float().numpy()
    data = ratings.RatingsData(users, items, values, lengths.size, max(int(lengths.max()), 1)).to(dev)
    a, y = (torch.randn(users.size, generator=g).to(dev) for _ in range(2))
    for skip in (False, True):
        form = "skip ties" if skip else "all pairs"
        out[f"mfcd_pair_ragged_stats, {form} @ {tag}"] = _sha(*(t for what in ("both", "counts", "sums")
                                                                for t in ratings.pair_ragged_stats(a, data, 1.0, what, skip)
                                                                if t is not None))
        out[f"mfcd_pair_ragged_grad, {form} @ {tag}"] = _sha(*ratings.pair_ragged_grad(a, data, 1.0, skip))
        out[f"mfcd_pair_ragged_hvp, {form} @ {tag}"] = _sha(*ratings.pair_ragged_hvp(a, y, data, skip, True),
                                                            *ratings.pair_ragged_hvp(a, y, data, skip))


def digest():
    """sha256 of the outputs of every pair entry the library has → one JSON line."""
    import ctypes
    from mfcd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)                    # a library of an earlier commit lacks the entries added since
    for name in [k for k in _lib.SIGNATURES if not hasattr(lib, k)]:
        del _lib.SIGNATURES[name]
    entries = set(_lib.SIGNATURES)
    g = torch.Generator().manual_seed(1)
    out = {}
    # edge shapes: one and two columns of a tile, a tile plus one column, three tiles (a J strictly between I and the end)
    for m in (2, 65, 1025, 2049):
        wide = [torch.randn(3, m + 5, generator=g).to(dev) for _ in range(3)]
        alpha, beta = (10.0 ** (-6.0 * torch.rand(m, generator=g)) for _ in range(2))
        labels = torch.randint(0, 3, (3, m), generator=g)
        laws = {"empty law": pairs.PairLaw(), "weights": pairs.PairLaw(alpha=alpha, beta=beta, device=dev),
                "margin": pairs.PairLaw(margin=0.95), "labels": pairs.PairLaw(labels=labels, device=dev),
                "full law": pairs.PairLaw(alpha=alpha, beta=beta, margin=0.95, labels=labels[0], device=dev)}
        _dense(out, f"3 x {m}", *(t[:, :m].contiguous() for t in wide), laws)
        _dense(out, f"3 x {m} strided", *(t[:, :m] for t in wide), laws)
    for k in (2, 65, 129):
        for d in (2, 33, 129):
            _tables(out, f"3 x {k}, d = {d}", 3, k, d, g, full_law(k, g), entries)
    if "mfcd_pair_ragged_stats" in entries:
        _ragged(out, "rows of 0, 1, 2, 64, 65, 256, 257, 513", (0, 1, 2, 64, 65, 256, 257, 513), g)
    # the host loops' second launch block
    rows = (1 << 20) + 3
    A, X, Y = (torch.randn(rows, 2, generator=g).to(dev) for _ in range(3))
    _dense(out, f"{rows} x 2", A, X, Y, {"full law, labels per row": full_law(2, g, rows)})
    del A, X, Y
    _tables(out, "4099 x 2, d = 2", 4099, 2, 2, g, full_law(2, g, 4099), entries & {"mfcd_pair_hvp_multi_rows"})
    _tables(out, "32771 x 2, d = 2", 32771, 2, 2, g, full_law(2, g, 32771), entries & {"mfcd_pair_best_rows"})
    if "mfcd_pair_ragged_stats" in entries:
        _ragged(out, f"{rows} rows of 1 and 2", 1 + (np.arange(rows) & 1), g)
    torch.cuda.empty_cache()
    # the shapes the tools time
    for name, rows, m in SHAPES:
        A, X, Y = (torch.randn(rows, m, generator=g).to(dev) for _ in range(3))
        _dense(out, name, A, X, Y, {"full law": full_law(m, g)})
        del A, X, Y
        torch.cuda.empty_cache()
    print(json.dumps(out))


def identity_lines(parent_lib, script=None, what="every pair entry"):
    """`digest` under the library in use and under `parent_lib`, each in a child process of its own.  script: another tool
    whose --digest prints such a JSON line of `what` (bench_ranking.py: mfcd_topk_rows)."""
    found = {}
    for tag, lib in (("this build", None), ("parent build", os.path.abspath(parent_lib))):
        env = dict(os.environ)
        env.pop("MFCD_LIB", None)
        if lib:
            env["MFCD_LIB"] = lib
        done = subprocess.run([sys.executable, os.path.abspath(script or __file__), "--digest"], env=env, capture_output=True,
                              text=True, check=True, timeout=600)
        found[tag] = json.loads(done.stdout.strip().splitlines()[-1])
    lines = [f"# identity: outputs of {what}, this build against a build of the parent commit (sha256 of every "
             "output tensor, first 12 digits; an entry the parent lacks: -)"]
    for key, a in found["this build"].items():
        b = found["parent build"].get(key)
        verdict = "bit-identical" if a == b else "new entry" if b is None else "DIFFERENT"
        lines.append(f"#   {key:78s} {a[:12]} {b[:12] if b else '-':12s} {verdict}")
    return lines


def bench_lines(parent_tree, runs, swap=False):
    """bench.py in this tree and in `parent_tree`, taking turns; swap: the parent goes first in every second turn."""
    trees = (("this commit", ROOT), ("its parent", os.path.abspath(parent_tree)))
    found = {"this commit": [], "its parent": []}
    for turn in range(runs):
        for tag, tree in (trees[::-1] if swap and turn % 2 else trees):
            env = dict(os.environ)
            env.pop("MFCD_LIB", None)
            done = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10490", "--warmup", "1049"], cwd=tree,
                                  env=env, capture_output=True, text=True, check=True, timeout=600)
            found[tag].append(json.loads(done.stdout.strip().splitlines()[-1])["value"] / 1e6)
    lines = [f"# bench.py --gpus 1 --steps 10490 --warmup 1049 in this tree and in a built checkout of the parent commit, {runs} "
             f"runs each, the commits taking turns on one GPU{', the order swapping from turn to turn' if swap else ''}; M triplet-updates/s"]
    for tag, vals in found.items():
        med = sorted(vals)[len(vals) // 2]
        lines.append(f"#   {tag:12s} " + " ".join(f"{v:8.2f}" for v in vals) + f"   median {med:8.2f}   spread "
                     f"{100.0 * (max(vals) - min(vals)) / med:4.1f}%")
    return lines


if __name__ == "__main__":
    if "--digest" in sys.argv[1:]:
        digest()
