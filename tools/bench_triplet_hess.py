"""Diagnostic: time the triplet gradient / Hessian-vector kernel (include/mfcd.h: mfcd_triplet_rows) and the joint Newton
fit built on it (mfcd/newton.py), and write the table to profiles/triplet_hess.txt (or --out PATH).

  kernel   one gradient pass (F, gradient and Jacobi diagonal of both tables: mfcd.newton.triplet_pass) and one
           Hessian-vector product over both sides (triplet_hvp) at
             notebook   n = m = 1000, d = 2, 200 000 comparisons
             C2         n = m = 4096, d = 64, 67 108 comparisons
             C3         n = m = 16384, d = 128, 107 373 comparisons
           each beside the same quantities by torch f64 gathers and index_add_ in the same process, and as a fraction of
           the gather-bytes bound: per record 4 rows x d x 8 B on the user side of a product and twice that on the item
           side (every comparison is a record of two item rows), half of both for a gradient pass, at 6.3 TB/s
  fit      fit_newton against fit_alternating from the same start at n = m = 1000, d = 2, 200 000 comparisons, weight
           decay 1e-4 (l2 = 20), labels from a rank-2 truth: time and F of both, and the number of sweeps alternation
           needs to reach Newton's F (of 200)
  --dump DIR [--tree CHECKOUT]
           write every output of the four exact block steps (fold_in_users and fold_in_items through both solvers) on
           fixed inputs as .npy files, with the package of CHECKOUT (default: this one); two such directories are compared
           byte for byte by `python tools/dump_fold_in.py --compare A B`, which is how the record at the end of
           profiles/triplet_hess.txt was made

Timing as tools/bench_fold_in.py.  Usage: bench_triplet_hess.py [--out PATH] | --dump DIR [--tree CHECKOUT]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else ROOT
sys.path[:0] = [TREE, os.path.join(TREE, "matrix-factorization-with-comparison-data_amd"), os.path.join(TREE, "tools")]
import torch  # noqa: E402

import bench_fold_in as B  # noqa: E402
from mfcd import alternating, foldin  # noqa: E402

dev = B.dev
HBM = 6.3e12


def comparisons(n, m, d, N, g, rank=None):
    """→ (U0, V0 fp32, u, i, j, z) on the device: uniform comparisons, labels from a truth of width `rank` (default d)."""
    r = d if rank is None else rank
    A, Bt = 3.0 * torch.randn(n, r, generator=g).to(dev), (torch.randn(m, r, generator=g) / r ** 0.5).to(dev)
    u, i = torch.randint(0, n, (N,), generator=g).to(dev), torch.randint(0, m, (N,), generator=g).to(dev)
    j = (i + 1 + torch.randint(0, m - 1, (N,), generator=g).to(dev)) % m
    z = (torch.rand(N, generator=g).to(dev) < torch.sigmoid((A[u] * (Bt[i] - Bt[j])).sum(1))).float()
    U0, V0 = (torch.randn(n, d, generator=g) / d ** 0.5).to(dev), (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
    return U0, V0, u, i, j, z


def torch_pass(U, V, u, i, j, z, l2):
    delta, a = V[i] - V[j], U[u]
    x = (a * delta).sum(1)
    p = torch.sigmoid(x)
    r, w = (p - z).unsqueeze(1), (p * (1.0 - p)).unsqueeze(1)
    gU = (l2 * U).index_add_(0, u, r * delta)
    gV = (l2 * V).index_add_(0, i, r * a).index_add_(0, j, -r * a)
    DU = torch.full_like(U, l2).index_add_(0, u, w * delta * delta)
    DV = torch.full_like(V, l2).index_add_(0, i, w * a * a).index_add_(0, j, w * a * a)
    F = torch.sum(torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs())) - z * x) + 0.5 * l2 * (torch.sum(U * U) + torch.sum(V * V))
    return F, gU, gV, DU, DV


def torch_hvp(U, V, u, i, j, z, P, Q, l2):
    delta, dq, a, ad = V[i] - V[j], Q[i] - Q[j], U[u], P[u]
    p = torch.sigmoid((a * delta).sum(1))
    r = (p - z).unsqueeze(1)
    wy = (p * (1.0 - p) * ((ad * delta).sum(1) + (a * dq).sum(1))).unsqueeze(1)
    HU = (l2 * P).index_add_(0, u, wy * delta + r * dq)
    tv = wy * a + r * ad
    return HU, (l2 * Q).index_add_(0, i, tv).index_add_(0, j, -tv)


def kernel_level(emit):
    from mfcd import newton
    g = torch.Generator().manual_seed(11)
    emit(f"{'size':34s} {'what':>10s} {'kernel ms':>10s} {'torch ms':>10s} {'ratio':>7s} {'bound ms':>9s} {'of bound':>9s} {'max rel diff':>13s}")
    for name, n, m, d, N in (("notebook 1000x1000 d=2 N=200000", 1000, 1000, 2, 200000),
                             ("C2 4096x4096 d=64 N=67108", 4096, 4096, 64, 67108),
                             ("C3 16384x16384 d=128 N=107373", 16384, 16384, 128, 107373)):
        U0, V0, u, i, j, z = comparisons(n, m, d, N, g)
        U, V, zd, l2 = U0.double(), V0.double(), z.double(), 1e-4 * N
        P, Q = torch.randn(n, d, generator=g).to(dev).double(), torch.randn(m, d, generator=g).to(dev).double()
        by_user, by_item = newton.group_rows(u, i, j, z, n, m)
        ours, theirs = newton.triplet_pass(U, V, by_user, by_item, l2), torch_pass(U, V, u, i, j, zd, l2)
        diff = max(float(((a - b).abs().max() / b.abs().max())) for a, b in zip(ours, theirs))
        k, t = B.timed(lambda: newton.triplet_pass(U, V, by_user, by_item, l2)), B.timed(lambda: torch_pass(U, V, u, i, j, zd, l2))
        bound = 48.0 * N * d / HBM * 1e3
        emit(f"{name:34s} {'gradient':>10s} {k:10.4f} {t:10.4f} {t / k:7.2f} {bound:9.5f} {bound / k:9.4f} {diff:13.2e}")
        ours, theirs = newton.triplet_hvp(U, V, by_user, by_item, P, Q, l2), torch_hvp(U, V, u, i, j, zd, P, Q, l2)
        diff = max(float(((a - b).abs().max() / b.abs().max())) for a, b in zip(ours, theirs))
        k = B.timed(lambda: newton.triplet_hvp(U, V, by_user, by_item, P, Q, l2))
        t = B.timed(lambda: torch_hvp(U, V, u, i, j, zd, P, Q, l2))
        bound = 96.0 * N * d / HBM * 1e3
        emit(f"{name:34s} {'product':>10s} {k:10.4f} {t:10.4f} {t / k:7.2f} {bound:9.5f} {bound / k:9.4f} {diff:13.2e}")


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def fit_level(emit):
    from mfcd import newton
    g = torch.Generator().manual_seed(12)
    n = m = 1000
    d, N, wd = 2, 200000, 1e-4
    U0, V0, u, i, j, z = comparisons(n, m, d, N, g, rank=2)
    l2 = wd * N
    newton.fit_newton(U0, V0, u, i, j, z, l2, max_iter=2)                      # warm-up
    res, ms = wall(lambda: newton.fit_newton(U0, V0, u, i, j, z, l2))
    F_newton = float(res.history[-1])
    emit(f"fit_newton      1000x1000 d=2 N=200000 l2={l2:g}: {ms:9.1f} ms, status {res.status}, {len(res.history)} outer iterations, "
         f"{res.products} Hessian products, F {float(res.history[0])!r} -> {F_newton!r}, |g|_inf {float(res.grad_inf[-1]):.3e}")
    alternating.fit_alternating(U0, V0, u, i, j, z, l2, sweeps=1)             # warm-up
    alt10, ms10 = wall(lambda: alternating.fit_alternating(U0, V0, u, i, j, z, l2, sweeps=10))
    alt, ms200 = wall(lambda: alternating.fit_alternating(U0, V0, u, i, j, z, l2, sweeps=200))
    ends = alt.history[:, -1]
    reached = torch.nonzero(ends <= F_newton).reshape(-1)
    emit(f"fit_alternating same start: 10 sweeps {ms10:9.1f} ms, F {float(alt10.history[-1, -1])!r}; 200 sweeps {ms200:9.1f} ms, "
         f"F {float(ends[-1])!r}; sweeps to reach Newton's F: {int(reached[0]) + 1 if reached.numel() else 'not within 200'}; "
         f"F(alternating, 200) - F(Newton) = {float(ends[-1]) - F_newton:.3e}")


def dump(out):
    """Every output of the four exact block steps on fixed inputs, one .npy each."""
    import numpy as np
    os.makedirs(out, exist_ok=True)
    g = torch.Generator().manual_seed(13)
    count = 0
    for d in (2, 16, 64, 100):
        n, m, N = 300, 200, 20000
        U0, V0, u, i, j, z = comparisons(n, m, d, N, g)
        by_user, by_item = foldin.group_by_user(u, i, j, z, n), foldin.group_by_item(u, i, j, z, m)
        for method in ("cholesky", "cg") if d <= 64 else ("cg",):
            res = foldin.fold_in_users(V0, *by_user, 0.5, U0, method=method)
            it = foldin.fold_in_items(U0, V0, *by_item, 0.5, None, 0.5) if method == "cholesky" else \
                foldin.fold_in_items_cg(U0, V0, *by_item, 0.5, None, 0.5)
            for side, r in (("user", res), ("item", it)):
                for k, t in enumerate(tuple(r) + (r.cg_iters,)):
                    if t is not None:
                        np.save(os.path.join(out, f"{side}_d{d}_{method}_{k}.npy"), t.cpu().numpy())
                        count += 1
    from mfcd import _lib
    print(f"{count} files written to {out} with {_lib.LIB_PATH}")


def main():
    args = sys.argv[1:]
    if "--dump" in args:
        return dump(args[args.index("--dump") + 1])
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "triplet_hess.txt")
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_triplet_hess.py: kernel rows timed as tools/bench_fold_in.py "
             "(one warm-up, then stretches or the faster of two calls); all tables f64",
             "# gradient = triplet_pass (two kernel calls: F, gradient and diagonal of both tables); product = triplet_hvp (two "
             "kernel calls); torch = f64 gathers + index_add_ in the same process; bound = gather bytes / 6.3 TB/s",
             "# max rel diff: kernel against torch, per output, largest |a - b|_inf / |b|_inf"]
    print("\n".join(lines), flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    kernel_level(emit)
    emit("")
    fit_level(emit)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
