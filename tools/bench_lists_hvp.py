"""Diagnostic: time the list Hessian-vector kernel and the exact steps on ranked lists (mfcd/lists.py, mfcd/lists_exact.py;
csrc/list_pl_hvp.hip) and write the table to profiles/lists_hvp.txt (or --out PATH).  The three shapes are
tools/bench_lists.py's.

Per shape: ms per call of `pl_hvp_rows` without and with the diagonal beside `pl_rows(..., "both")`, the forms taking
turns; the same product by library ops (the lists padded to the longest, torch.logcumsumexp on the flipped matrix, the
gradient by autograd with its graph kept and the product by a second backward) with its largest difference from the
kernel's q.  On the first shape: one exact user step, one exact item step and one sweep of `fit_lists_exact` from a fresh
model, the fold-in of 256 new users, the share of rows certified, and `fit_lists` (Adam with the same weight decay) from
the same start until it reaches the F the sweep reached.

  identity  --parent-lib PATH (libmfcd_hip.so of a build of the parent commit): sha256 of mfcd_list_pl's outputs on
            tests/test_lists.py's case() under both libraries, each in a child process (--digest prints one)
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns, the order
            swapping from turn to turn

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported; the steps by wall clock around one call after an untimed one.
Usage: bench_lists_hvp.py [--out PATH] [--parent-lib PATH] [--parent-tree DIR] [--bench-runs N] | --digest
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__)),
                os.path.join(ROOT, "tests")]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pair_bench_common import _sha, alternated, bench_lines, identity_lines, wall  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("PAIRS_BENCH_SECONDS", "0.5"))
PAD = -1.0e30                  # a padded score: exp(PAD - anything) is 0, and PAD - PAD is 0, not NaN
L2 = 1e-3


def digest():
    """sha256 of mfcd_list_pl's outputs (what = 3, 1 and 2) on tests/test_lists.py's case() → one JSON line."""
    import ctypes
    from mfcd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)                    # a library of an earlier commit lacks the entries added since
    for name in [k for k in _lib.SIGNATURES if not hasattr(lib, k)]:
        del _lib.SIGNATURES[name]
    import test_lists as TL
    _, a, off, depth, _ = TL.case()
    out = {}
    for what in (3, 1, 2):
        got = TL.run(dev, a, off, depth, what=what)
        out[f"mfcd_list_pl, what = {what} @ test_lists.case(): {off.size - 1} rows, {a.size} entries"] = _sha(
            *(torch.from_numpy(t) for t in got if t is not None))
    print(json.dumps(out))


def torch_hvp(a_pad, y_pad, shown, staged):
    """H y in the padded scores by library ops: the gradient with its graph, then the gradient of g . y."""
    x = a_pad.detach().requires_grad_(True)
    z = torch.where(shown, x, torch.full_like(x, PAD))
    lse = torch.logcumsumexp(z.flip(1), 1).flip(1)
    loss = torch.where(staged, lse - z, torch.zeros_like(z)).sum()
    g = torch.autograd.grad(loss, x, create_graph=True)[0]
    return torch.autograd.grad((g * y_pad).sum(), x)[0]


def shape_lines(name, lists, d, emit):
    import structure as S
    from mfcd import lists as ML
    torch.manual_seed(0)
    model = S.MatrixFactorization(lists.n, lists.m, d).to(dev)
    U, V = model.U.data, model.V.data
    a = ML.list_scores(U, V, lists)[0].mul_(4.0).contiguous()                   # a spread of a few units, as after a fit
    y = torch.randn(lists.entries, generator=torch.Generator().manual_seed(1)).to(dev)
    L = lists.lengths
    k = int(L.max())
    pos = torch.from_numpy(np.arange(lists.entries) - np.repeat(np.cumsum(L) - L, L)).to(dev)
    rows = lists.user.long()
    a_pad, y_pad = torch.zeros((lists.n, k), device=dev), torch.zeros((lists.n, k), device=dev)
    shown = torch.zeros((lists.n, k), dtype=torch.bool, device=dev)
    a_pad[rows, pos], y_pad[rows, pos], shown[rows, pos] = a, y, True
    staged = torch.arange(k, device=dev)[None, :] < torch.from_numpy(lists.user_stages).to(dev)[:, None]
    ms = alternated([lambda: ML.pl_hvp_rows(a, y, lists), lambda: ML.pl_hvp_rows(a, y, lists, True),
                     lambda: ML.pl_rows(a, lists, "both"), lambda: torch_hvp(a_pad, y_pad, shown, staged)])
    emit(f"{name}: {lists.n} lists over {lists.m} items, {lists.entries} entries, {lists.stages} stages, d = {d}; lengths "
         f"{L.min()} .. {L.max()} (median {int(np.median(L))}); tiles {lists.n_tiles}")
    emit(f"  ms per call: pl_hvp_rows {ms[0]:.3f}, with deg {ms[1]:.3f}; pl_rows value and gradient {ms[2]:.3f}; the product "
         f"over the gradient {ms[0] / ms[2]:.2f} x, deg adds {ms[1] / ms[0] - 1.0:+.0%}; {lists.entries / ms[0] / 1e6:.2f} G entries/s")
    q = ML.pl_hvp_rows(a, y, lists)[0]
    q_t = torch_hvp(a_pad, y_pad, shown, staged)[rows, pos]
    emit(f"  the same product by padded ({lists.n} x {k}) torch.logcumsumexp and a double backward: {ms[3]:.3f} ms "
         f"({ms[3] / ms[0]:.2f} x the kernel); largest difference of q {float((q_t - q).abs().max()):.2e} at a largest |q| of "
         f"{float(q.abs().max()):.2e}")
    return model


def exact_lines(lists, d, emit):
    """Exact steps and fold-in on one shape, beside Adam from the same start to the same F."""
    import structure as S
    from mfcd import lists as ML, lists_exact as LE

    def fresh():
        torch.manual_seed(0)
        return S.MatrixFactorization(lists.n, lists.m, d).to(dev)

    def F(U, V):
        with torch.no_grad():
            return float(ML.pl_risk(U, V, lists).double() + 0.5 * L2 * ((U.double() ** 2).sum() + (V.double() ** 2).sum()))

    model = fresh()
    U, V = model.U.data, model.V.data
    LE.lists_user_step(U, V, lists, L2)                                         # untimed
    user, t_user = wall(lambda: LE.lists_user_step(U, V, lists, L2))
    item, t_item = wall(lambda: LE.lists_item_step(U, V, lists, L2))
    emit(f"exact steps on the first shape from a fresh model, l2 = {L2:g}, gtol = 1e-3 (wall clock, one call after an "
         f"untimed one):")
    emit(f"  user step {t_user:.1f} ms: {float((user.status == 0).double().mean()):.3f} of the rows certified, Newton "
         f"iterations at most {int(user.newton_iters.max())}, CG iterations in all at most {int(user.cg_iters.max())}; F "
         f"{float(user.objective_before.sum()) + 0.5 * L2 * float((V.double() ** 2).sum()):.6f} -> "
         f"{float(user.objective_after.sum()) + 0.5 * L2 * float((V.double() ** 2).sum()):.6f}")
    emit(f"  item step {t_item:.1f} ms: status {int(item.status)}, Newton iterations {int(item.newton_iters)}, CG iterations "
         f"{int(item.cg_iters)}; F {float(item.objective_before) + 0.5 * L2 * float((U.double() ** 2).sum()):.6f} -> "
         f"{float(item.objective_after) + 0.5 * L2 * float((U.double() ** 2).sum()):.6f}")
    start = F(U, V)
    fit, t_fit = wall(lambda: LE.fit_lists_exact(U, V, lists, L2, 1))
    target = float(fit.history[0, 1])
    emit(f"  one sweep of fit_lists_exact {t_fit:.1f} ms: F {start:.6f} -> {float(fit.history[0, 0]):.6f} -> {target:.6f}; "
         f"{float((fit.user_status == 0).double().mean()):.3f} of the users certified, item status {int(fit.item_status)}")
    # Adam from the same start, the same ridge as coupled weight decay, until F is at the sweep's
    model = fresh()
    opt = torch.optim.Adam(model.parameters(), lr=0.05, weight_decay=L2)
    ML.fit_lists((model, opt), lists, 1)
    model, steps, chunk, cap = fresh(), 0, 25, 5000
    opt = torch.optim.Adam(model.parameters(), lr=0.05, weight_decay=L2)
    torch.cuda.synchronize()
    import time
    t0, now = time.perf_counter(), F(model.U.data, model.V.data)
    while now > target and steps < cap:
        ML.fit_lists((model, opt), lists, chunk)
        steps += chunk
        now = F(model.U.data, model.V.data)
    torch.cuda.synchronize()
    t_adam = (time.perf_counter() - t0) * 1e3
    emit(f"  fit_lists (Adam, lr 0.05, weight decay {L2:g}) from the same start, F read every {chunk} steps: F = {now:.6f} after "
         f"{steps} steps, {t_adam:.1f} ms" + ("" if now <= target else f" — the sweep's F not reached within {cap} steps"))
    # fold-in of 256 users who were not in training: the first 256 lists, as new users against the fitted V
    off = lists.row_off.cpu().numpy()
    e = int(off[256])
    new = ML.RankedLists(lists.user.cpu().numpy()[:e], lists.item.cpu().numpy()[:e], lists.position.cpu().numpy()[:e], 256,
                         lists.m).to(dev)
    coef = 1.0 / lists.stages
    LE.lists_user_step(None, V, new, L2, coef)
    fold, t_fold = wall(lambda: LE.lists_user_step(None, V, new, L2, coef))
    emit(f"  fold-in of 256 new users ({new.entries} entries) against the fitted V: {t_fold:.1f} ms, "
         f"{float((fold.status == 0).double().mean()):.3f} of the rows certified, Newton iterations at most "
         f"{int(fold.newton_iters.max())}")


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        return digest()
    from bench_pair_ragged import long_tailed
    from mfcd import lists as ML
    out_path = os.path.join(ROOT, "profiles", "lists_hvp.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_lists_hvp.py: >= {SECONDS} s per stretch after an untimed "
             "stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(0)
    n, m = 943, 1682
    L = long_tailed(n, 100000, 20, 737, rng)
    items = np.concatenate([rng.choice(m, k, replace=False) for k in L])
    position = np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)
    first = ML.RankedLists(np.repeat(np.arange(n), L), items, position, n, m).to(dev)
    shape_lines("ml100k-shaped", first, 16, emit)
    n = m = 20000
    coprime = np.array([s for s in range(1, 200) if np.gcd(s, m) == 1])       # 100 steps stay below m: distinct items
    start, step = rng.integers(0, m, n), coprime[rng.integers(0, coprime.size, n)]
    items = (start[:, None] + step[:, None] * np.arange(100)[None, :]) % m
    users, position = np.repeat(np.arange(n), 100), np.tile(np.arange(100), n)
    shape_lines("slates of 100", ML.RankedLists(users, items.reshape(-1), position, n, m).to(dev), 64, emit)
    n = m = 4096
    items = np.argsort(rng.random((n, m)), axis=1)
    users, position = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
    shape_lines("full catalogue, depth 10", ML.RankedLists(users, items.reshape(-1), position, n, m, depth=10).to(dev), 64, emit)
    torch.cuda.empty_cache()
    exact_lines(first, 16, emit)
    if "--parent-lib" in args:
        for line in identity_lines(args[args.index("--parent-lib") + 1], os.path.abspath(__file__),
                                   "mfcd_list_pl on tests/test_lists.py's case()"):
            emit(line)
    if "--parent-tree" in args:
        runs = int(args[args.index("--bench-runs") + 1]) if "--bench-runs" in args else 3
        for line in bench_lines(args[args.index("--parent-tree") + 1], runs, swap=True):
            emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
