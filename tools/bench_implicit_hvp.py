"""Diagnostic: time the implicit-feedback Hessian-vector kernel (mfcd/implicit.py: implicit_hvp_rows; csrc/implicit_hvp.hip)
beside mfcd_implicit_rows with the gradient and beside the same product by chunked torch ops in the same process, time the
exact block steps built on it (mfcd/implicit_exact.py), and write the table to profiles/implicit_hvp.txt (or --out PATH).

  shapes    those of tools/bench_implicit.py: ml100k (943 x 1682, 100 000 entries, d = 16), large (20 000 x 20 000, 2 M
            entries, long-tailed rows, d = 64), factored (n = m = 65 536, d = 64, 10 observed items per user)
  product   on rows 0 .. min(n, 4096) - 1: the dense-mode call on precomputed scores and direction with and without deg,
            mfcd_implicit_rows with the gradient on the same scores, and the user step's factor-mode call (B = By = V)
            beside mfcd_implicit_rows' factor-mode call; (positive, negative) pairs per second and compute unit
  torch form   per chunk of rows one rows x L x m broadcast of sigmoid'(a_j - a_i) (y_i - y_j) under the (positive,
               negative) mask, summed over both axes; on the two large shapes on the first ROWS_SUB rows only
  steps     on the ml100k-shaped table, l2 = 1e-2 / n: one user step, one item step and one sweep of fit_implicit_exact
            from a table of small random entries, and the fold-in of 256 new users (rows of the same table, as a CSR pair
            of their own) — wall time of one call, the second of two, with Newton and CG iteration counts

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported, the forms taking turns; the steps and the large torch forms: wall time of one call.
--digest: sha256 of every output of mfcd_implicit_rows on the shapes of tests/test_implicit.py → one JSON line (the
library is MFCD_LIB, or the tree's).  --parent-lib PATH (libmfcd_hip.so of the parent commit): the digest under both
libraries.  --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns.

Usage: bench_implicit_hvp.py [--out PATH] [--skip-large] [--parent-lib PATH] [--parent-tree DIR] [--bench-runs N] [--digest]
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

dev = torch.device("cuda:0")
TORCH_ELEMS = 1 << 26              # elements of the torch form's rows x L x m temporaries per chunk
ROWS_SUB = 512


def digest():
    """sha256 of counts, sums, g and status of mfcd_implicit_rows: the dense cases of tests/test_implicit.py (every m, every
    variant; with the gradient, without, and the prepare pass), its exact factor cases and a call with rows and coef."""
    import ctypes
    import hashlib
    from mfcd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)                    # a library of an earlier commit lacks the entries added since
    for name in [k for k in _lib.SIGNATURES if not hasattr(lib, k)]:
        del _lib.SIGNATURES[name]
    from mfcd import implicit
    import test_implicit as T

    def sha(*results):
        h = hashlib.sha256()
        for res in results:
            for t in res:
                if t is not None:
                    h.update(t.cpu().numpy().tobytes())
        return h.hexdigest()

    out = {}
    for m in T._ms():
        X = torch.from_numpy(T._scores(m)).to(dev)
        for variant in T.VARIANTS:
            P, E = T._dev_lists(m, variant, dev)
            out[f"dense m={m} {variant}"] = sha(implicit.implicit_rows(X, P, E, grad=True), implicit.implicit_rows(X, P, E),
                                                implicit.implicit_rows(X, P, E, prepare_only=True))
        for d in (1, 2, 33):
            rng = np.random.default_rng(31 * m + d)
            variant = T.VARIANTS[(m + d) % 3]
            rows = X.shape[0]
            A = torch.from_numpy((rng.integers(-2, 3, (rows + 3, d)) * 0.5).astype(np.float32)).to(dev)
            B = torch.from_numpy(rng.standard_normal((m, d)).astype(np.float32)).to(dev)
            ids = rng.permutation(rows + 3)[:rows]
            coef = torch.from_numpy(rng.uniform(0.5, 2.0, rows).astype(np.float32)).to(dev)
            P, E = T._dev_lists(m, variant, dev)
            out[f"factors m={m} d={d} {variant}, rows and coef"] = sha(implicit.implicit_rows((A, B), P, E, rows=ids, grad=True,
                                                                                             coef=coef))
    print(json.dumps(out))


def torch_product(S, Y, off, items, coef, rows):
    """q of rows [0, rows) of the score rows S and direction rows Y by library ops → fp32 [rows, m]."""
    m = S.shape[1]
    lens = off[1:rows + 1] - off[:rows]
    lens_h = lens.cpu().numpy()
    out = torch.empty((rows, m), device=dev)
    r0 = 0
    while r0 < rows:
        r1, width = r0, 0                              # as many rows as fit: (r1 - r0) x max L x m <= TORCH_ELEMS
        while r1 < rows and (r1 - r0 + 1) * max(width, int(lens_h[r1]), 1) * m <= TORCH_ELEMS:
            width = max(width, int(lens_h[r1]), 1)
            r1 += 1
        r1 = max(r1, r0 + 1)
        width = max(width, int(lens_h[r0]), 1)
        nb = r1 - r0
        k = torch.arange(width, device=dev)[None, :]
        valid = k < lens[r0:r1, None]
        idx = torch.where(valid, items[(off[r0:r1, None] + k).clamp(max=items.numel() - 1)].long(), torch.zeros_like(k))
        neg = torch.ones((nb, m), dtype=torch.bool, device=dev)
        neg[torch.arange(nb, device=dev)[:, None].expand_as(idx)[valid], idx[valid]] = False
        s = torch.sigmoid(S[r0:r1, None, :] - torch.gather(S[r0:r1], 1, idx)[:, :, None])
        w = s * (1.0 - s) * (valid[:, :, None] & neg[:, None, :]).float()
        t = w * (Y[r0:r1, None, :] - torch.gather(Y[r0:r1], 1, idx)[:, :, None])      # w (y_j - y_i)
        q = t.sum(1)
        q.scatter_add_(1, idx, -t.sum(2) * valid.float())
        out[r0:r1] = q * coef[r0:r1, None]
        r0 = r1
    return out


def products(name, U, V, data, emit, sub=None):
    from pair_bench_common import alternated, wall
    from mfcd import implicit
    n, m, d = U.shape[0], V.shape[0], U.shape[1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator().manual_seed(2)
    rows_x = min(n, 4096)
    x_data = (data.row_off[:rows_x + 1].contiguous(), data.item)
    plan = implicit._Plan(rows_x, m, dev, x_data, None, "pairs", None)
    pairs = int((plan.counts[:, 0] * plan.counts[:, 1]).sum())
    coef = plan.coef
    Ux = U[:rows_x].contiguous()
    Px = (torch.randn(rows_x, d, generator=g) / 4.0).to(dev)
    X, Y = (Ux @ V.t()).contiguous(), (Px @ V.t()).contiguous()
    with_deg = lambda: implicit.implicit_hvp_rows(X, Y, x_data, coef=coef, deg=True)    # noqa: E731
    without = lambda: implicit.implicit_hvp_rows(X, Y, x_data, coef=coef)    # noqa: E731
    grad = lambda: implicit.implicit_rows(X, x_data, grad=True, coef=coef)    # noqa: E731
    f_hvp = lambda: implicit.implicit_hvp_rows((Ux, V), (Px, V), x_data, coef=coef, deg=True)    # noqa: E731
    f_grad = lambda: implicit.implicit_rows((Ux, V), x_data, grad=True, coef=coef)    # noqa: E731
    t_deg, t_no, t_grad, t_fh, t_fg = alternated([with_deg, without, grad, f_hvp, f_grad])
    rate = lambda ms: pairs / ms / 1e6 / cus    # noqa: E731
    emit(f"  rows 0 .. {rows_x - 1} ({pairs:.3e} pairs), dense mode on precomputed scores: product with deg {t_deg:.3f} ms "
         f"({rate(t_deg):.3f} G pairs/s per CU), without {t_no:.3f} ms ({rate(t_no):.3f}); mfcd_implicit_rows with the gradient "
         f"{t_grad:.3f} ms ({rate(t_grad):.3f}); product with deg / gradient {t_deg / t_grad:.2f}; {cus} CUs")
    emit(f"  factor mode (the user step's call, two slabs): product with deg {t_fh:.3f} ms; mfcd_implicit_rows with the "
         f"gradient (one slab) {t_fg:.3f} ms; the slabs' share (factor minus dense) {t_fh - t_deg:.3f} and {t_fg - t_grad:.3f} ms")
    rows = rows_x if sub is None else sub
    ref = lambda: torch_product(X, Y, x_data[0], x_data[1], coef, rows)    # noqa: E731
    if sub is None:
        k_ms, t_ms = alternated([without, ref])
    else:
        s_data = (data.row_off[:rows + 1].contiguous(), data.item)
        kern = lambda: implicit.implicit_hvp_rows(X[:rows], Y[:rows], s_data, coef=coef[:rows].contiguous())    # noqa: E731
        k_ms = alternated([kern])[0]
        t_ms = min(wall(ref)[1], wall(ref)[1])
    want, got = ref(), without()[0][:rows]
    emit(f"  rows 0 .. {rows - 1}: product without deg {k_ms:10.3f} ms    torch form {t_ms:10.3f} ms    torch / kernel "
         f"{t_ms / k_ms:.1f}" + ("" if sub is None else "    (torch form: wall time of one call)"))
    emit(f"  against the torch form on those rows: largest |q - q'| {float((got - want).abs().max()):.2e} of "
         f"{float(want.abs().max()):.2e}")


def steps(U, V, data, emit):
    from pair_bench_common import wall
    from mfcd import implicit_exact
    n, m = U.shape[0], V.shape[0]
    l2 = 1e-2 / n

    def second(fn):
        wall(fn)
        return wall(fn)

    res, ms = second(lambda: implicit_exact.implicit_user_step(U, V, data, l2))
    emit(f"  l2 = {l2:.3e}; one user step from the table given: {ms:.1f} ms; Newton iterations at most "
         f"{int(res.newton_iters.max())}, CG iterations in all rows {int(res.cg_iters.sum())}, statuses "
         f"{np.bincount(res.status.cpu().numpy(), minlength=3).tolist()} (certified, stopped, invalid), objective "
         f"{float(res.objective_before.sum()):.6f} -> {float(res.objective_after.sum()):.6f}")
    res, ms = second(lambda: implicit_exact.implicit_item_step(U, V, data, l2))
    emit(f"  one item step: {ms:.1f} ms; Newton {int(res.newton_iters)}, CG {int(res.cg_iters)}, status {int(res.status)}, "
         f"objective {float(res.objective_before):.6f} -> {float(res.objective_after):.6f}")
    res, ms = second(lambda: implicit_exact.fit_implicit_exact(U.clone(), V.clone(), data, l2, 1))
    emit(f"  one sweep of fit_implicit_exact: {ms:.1f} ms; F {float(res.objective_start):.6f} -> "
         f"{res.history[0, 0].item():.6f} -> {res.history[0, 1].item():.6f}")
    new = (data[0][:257].contiguous(), data[1])
    from mfcd import implicit
    c = float(implicit._Plan(n, m, dev, data, None, "pairs", None).coef64.max())
    res, ms = second(lambda: implicit_exact.implicit_user_step(None, V, new, l2, coef=c))
    emit(f"  fold-in of 256 new users under the table's normaliser: {ms:.1f} ms; Newton iterations at most "
         f"{int(res.newton_iters.max())}, CG iterations in all rows {int(res.cg_iters.sum())}, statuses "
         f"{np.bincount(res.status.cpu().numpy(), minlength=3).tolist()}")


def main():
    args = sys.argv[1:]
    if "--digest" in args:
        return digest()
    from pair_bench_common import SECONDS, bench_lines, identity_lines
    from bench_pair_ragged import long_tailed, ml100k_shaped, strided
    from mfcd import ratings
    out_path = os.path.join(ROOT, "profiles", "implicit_hvp.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_implicit_hvp.py: >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(1)
    u, i, v, n, m = ml100k_shaped(np.random.default_rng(0))
    data = ratings.RatingsData(u, i, v, n, m).to(dev)
    U, V = (torch.randn(n, 16, generator=g) / 4.0).to(dev), (torch.randn(m, 16, generator=g) / 4.0).to(dev)
    emit(f"ml100k-shaped: {n} x {m}, d = 16, {data.entries} observed entries")
    products("ml100k", U, V, data, emit)
    steps(U, V, (data.row_off, data.item), emit)
    if "--skip-large" not in args:
        rng = np.random.default_rng(0)
        n = m = 20000
        L = long_tailed(n, 2000000, 5, 5000, rng)
        u, i, v = strided(n, m, L, rng)
        data = ratings.RatingsData(u, i, v, n, m).to(dev)
        U, V = (torch.randn(n, 64, generator=g) / 8.0).to(dev), (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"large: {n} x {m}, d = 64, {data.entries} observed entries; the torch form on the first {ROWS_SUB} rows")
        products("large", U, V, data, emit, sub=ROWS_SUB)
        n = m = 65536
        rng = np.random.default_rng(1)
        users = np.repeat(np.arange(n), 10)
        items = (rng.integers(0, m, n)[users] + np.tile(np.arange(10) * 1087, n)) % m      # 10 distinct items per user
        data = ratings.RatingsData(users, items, np.ones(users.size, np.float32), n, m).to(dev)
        U, V = (torch.randn(n, 64, generator=g) / 8.0).to(dev), (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"factored: {n} x {m}, d = 64, {data.entries} observed entries (10 per user); the torch form on the first "
             f"{ROWS_SUB} rows")
        products("factored", U, V, data, emit, sub=ROWS_SUB)
    emit("parent comparison: this change adds csrc/implicit_hvp.hip and moves implicit.hip's prepare kernel, marking, argument "
         "struct and host rules into csrc/implicit_common.h, so implicit.hip is rebuilt from changed source; "
         "scores_common.h, pairs_common.h and every other translation unit are byte-identical to the parent's")
    if "--parent-lib" in args:
        for line in identity_lines(args[args.index("--parent-lib") + 1], os.path.abspath(__file__),
                                   "mfcd_implicit_rows (counts, sums, g, status) on the shapes of tests/test_implicit.py"):
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
