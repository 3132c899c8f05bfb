"""Diagnostic: time the Newton-CG form of the exact block steps (mfcd/foldin.py: fold_in_users / fold_in_items above
d = 64, fold_in_items_cg; include/mfcd.h: mfcd_fold_in_users_cg, mfcd_item_step_cg) and write the table to
profiles/fold_in_cg.txt (or --out PATH).

  sizes    C3          n = m = 16384, d = 128, 268 435 comparisons with uniform users and items: the user step, one item
                       step of all items (theta = 1/2, U from the user step), one alternating sweep (1 + 2 steps)
           C5 shape    n = 100 000, m = 20 000, d = 256, 2 000 000 comparisons: the user step and the item step
           long rows   256 users x 10 000 comparisons, m = 4096, d = 256
           C2          n = m = 4096, d = 64, 167 772 comparisons: the user step through both solvers
  data     as tools/bench_fold_in.py: V ~ N(0, 1 / d), hard labels from a hidden u0 ~ N(0, 9 I) per user, start at 0,
           l2 = 1e-5 x the number of comparisons
  torch    bench_fold_in.torch_solve (padded, masked, batched f64 Newton with a Cholesky solve) for the user step at C3
           and C2, in the same run; it needs rows x d^2 doubles for the Hessians, which is why it is not run at the C5
           shape (52 GB) and why the long rows are left to --with-torch-long
  columns  ms per call; outer iterations (CG solves; Newton iterations for the other two solvers) and CG iterations per
           row with comparisons, mean and most; ns per (comparison x CG iteration), the work being the sum over the rows
           of comparisons x CG iterations (comparisons x iterations for the other two)

Timing as tools/bench_fold_in.py.  Usage: bench_fold_in_cg.py [--out PATH] [--with-torch-long]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import bench_fold_in as B  # noqa: E402
from mfcd import alternating, foldin  # noqa: E402

dev = B.dev


def stats(lengths, iters, cg):
    have = lengths > 0
    itd, work_it = iters.double(), cg if cg is not None else iters
    work = float((lengths * work_it.double()).sum())
    cols = f"{float(itd[have].mean()):8.2f} {int(iters.max()):5d} "
    cols += f"{float(cg.double()[have].mean()):9.1f} {int(cg.max()):6d}" if cg is not None else f"{'':9s} {'':6s}"
    return cols, work


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "fold_in_cg.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_fold_in_cg.py: timing as tools/bench_fold_in.py (>= {B.SECONDS} s "
             "per stretch after an untimed stretch, min of two rounds; longer calls: one warm-up, the faster of two)",
             "# cg: mfcd_fold_in_users_cg / mfcd_item_step_cg (max_iter 200); cholesky: mfcd_fold_in_users; torch: "
             "bench_fold_in.torch_solve, host waits included; alternating: fit_alternating, 1 sweep = 1 user + 2 item steps",
             "# outer = CG solves (Newton iterations for cholesky and torch) per row with comparisons; work = sum over rows of "
             "comparisons x CG iterations (x iterations for cholesky and torch); |dU|: torch against the line above, relative per row",
             f"{'size':40s} {'solver':>11s} {'ms/call':>10s} {'outer':>8s} {'most':>5s} {'cg mean':>9s} {'most':>6s} "
             f"{'ns/(cmp x it)':>13s} {'|dU|':>9s}"]
    print("\n".join(lines), flush=True)

    def emit(name, solver, ms, lengths, iters, cg, du=None):
        cols, work = stats(lengths, iters, cg)
        line = (f"{name:40s} {solver:>11s} {ms:10.3f} {cols} {ms * 1e6 / max(work, 1.0):13.4f} "
                f"{'' if du is None else format(du, '9.1e'):>9s}")
        print(line, flush=True)
        lines.append(line)

    def users(name, V, rec, off, l2, method, with_torch):
        lengths = (off[1:] - off[:-1]).double()
        kw = dict(max_iter=200, method=method)
        res = foldin.fold_in_users(V, rec, off, l2, **kw)
        assert int(res.status.max()) == 0, f"{name}: a row did not converge"
        emit(name, method, B.timed(lambda: foldin.fold_in_users(V, rec, off, l2, **kw)), lengths, res.iters, res.cg_iters)
        if with_torch:
            Ut, _, it = B.torch_solve(V, rec, off, l2)
            du = float(((Ut - res.U).abs().max(1)[0] / res.U.abs().max(1)[0].clamp_(min=1e-30)).max())
            emit(name, "torch", B.timed(lambda: B.torch_solve(V, rec, off, l2)), lengths, it, None, du)
            del Ut
        return res

    def items(name, U, V, irec, ioff, l2):
        lengths = (ioff[1:] - ioff[:-1]).double()
        res = foldin.fold_in_items_cg(U, V, irec, ioff, l2, None, 0.5, 200)
        assert int(res.status.max()) == 0, f"{name}: a row did not converge"
        emit(name, "cg", B.timed(lambda: foldin.fold_in_items_cg(U, V, irec, ioff, l2, None, 0.5, 200)), lengths, res.iters,
             res.cg_iters)

    g = torch.Generator().manual_seed(1)
    # ---- C3 ----
    n = m = 16384
    V, rec, off = B.make(n, m, 128, None, 268435, g)
    l2 = 1e-5 * rec.shape[0]
    res = users("C3 n=m=16384 d=128 268435 rec, users", V, rec, off, l2, "auto", True)
    u, i, j = rec[:, 0].long(), rec[:, 1].long(), rec[:, 2].long()
    z = rec[:, 3].contiguous().view(torch.float32)
    irec, ioff = foldin.group_by_item(u, i, j, z, m)
    items("C3, all items (theta 1/2)", res.U, V, irec, ioff, l2)
    U0 = torch.zeros(n, 128, device=dev)
    ms = B.timed(lambda: alternating.fit_alternating(U0, V, u, i, j, z, l2, sweeps=1, item_steps=2, max_iter=200))
    line = f"{'C3, one alternating sweep from U = 0':40s} {'alternating':>11s} {ms:10.3f}"
    print(line, flush=True)
    lines.append(line)
    del V, rec, off, res, irec, ioff, U0
    torch.cuda.empty_cache()
    # ---- the C5 shape ----
    n, m = 100000, 20000
    V, rec, off = B.make(n, m, 256, None, 2000000, g)
    l2 = 1e-5 * rec.shape[0]
    res = users("C5 shape 100000x20000 d=256 2e6 rec, users", V, rec, off, l2, "auto", False)
    irec, ioff = foldin.group_by_item(rec[:, 0].long(), rec[:, 1].long(), rec[:, 2].long(),
                                      rec[:, 3].contiguous().view(torch.float32), m)
    items("C5 shape, all items (theta 1/2)", res.U, V, irec, ioff, l2)
    del V, rec, off, res, irec, ioff
    torch.cuda.empty_cache()
    # ---- long rows ----
    V, rec, off = B.make(256, 4096, 256, 10000, None, g)
    users("long rows 256 x 10000 d=256", V, rec, off, 1e-5 * rec.shape[0], "auto", "--with-torch-long" in args)
    del V, rec, off
    torch.cuda.empty_cache()
    # ---- C2 through both solvers ----
    V, rec, off = B.make(4096, 4096, 64, None, 167772, g)
    l2 = 1e-5 * rec.shape[0]
    users("C2 n=m=4096 d=64 167772 rec, users", V, rec, off, l2, "cg", False)
    users("C2 n=m=4096 d=64 167772 rec, users", V, rec, off, l2, "cholesky", True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
