"""Diagnostic: time the item step (mfcd/foldin.py: fold_in_items, include/mfcd.h: mfcd_item_step) and one alternating
sweep (mfcd/alternating.py: fit_alternating, sweeps = 1, item_steps = 2) beside the same iterations done with torch ops
on the same GPU, and write the table to profiles/item_step.txt (or --out PATH).

  sizes    notebooks   n = m = 1000, d = 2, 200 000 comparisons (400 per item on average)
           C2          n = m = 4096, d = 64, 167 772 comparisons (about 82 per item)
  data     users and items uniform, hard labels from hidden tables with logits ~ N(0, 2); the step starts at tables
           0.1 N(0, I); l2 = 1e-5 x the number of comparisons (structure.refit_items' rule at weight_decay 1e-5)
  torch    rows padded to the longest and masked, batched f64 Newton on x = v . delta + c: bmm for the scores, the
           gradient and the Hessian, torch.linalg.cholesky / cholesky_solve, the same backtracking (its Armijo test on
           the two values of f) and the same stopping rule, all rows iterated until the last one stops; building the
           padded delta and c is part of the call, as gathering them is part of the kernel's.  The torch sweep is the
           torch user step (c = 0, delta = V[i] - V[j]) and two torch item steps, with the three F evaluations
  columns  ms per call; iterations (mean and most over the rows with records; for a sweep: of its three steps
           together); ns per (record x iteration), with the sum over the rows of records x iterations taken as the work
           of either solver (an item step reads every comparison twice: 2 N records)

Timing as tools/bench_fold_in.py (its stretch / best / timed are used): HIP events, >= SECONDS per stretch after an
untimed one, the smaller of two rounds.
Usage: bench_item_step.py [--out PATH]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import torch  # noqa: E402

import bench_fold_in as B  # noqa: E402
from mfcd import alternating, foldin  # noqa: E402

dev = B.dev
XTOL, MAX_ITER, HALVINGS = B.XTOL, B.MAX_ITER, B.HALVINGS


def make(n, m, d, N, g):
    """→ (U, V, u, i, j, z) on the device: the start tables and the comparisons."""
    u, i = torch.randint(0, n, (N,), generator=g), torch.randint(0, m, (N,), generator=g)
    j = (i + 1 + torch.randint(0, m - 1, (N,), generator=g)) % m
    Uh, Vh = (torch.randn(k, d, generator=g) / d ** 0.25 for k in (n, m))
    x = (Uh[u] * (Vh[i] - Vh[j])).sum(1)
    z = (torch.rand(N, generator=g) < torch.sigmoid(x)).float()
    U, V = 0.1 * torch.randn(n, d, generator=g), 0.1 * torch.randn(m, d, generator=g)
    return tuple(t.to(dev) for t in (U, V, u, i, j, z))


def padded(rec, off):
    """Row-major padding of grouped records → (index [rows, L] into the records, mask [rows, L], lengths)."""
    lengths = off[1:] - off[:-1]
    slot = torch.arange(int(lengths.max()), device=dev).unsqueeze(0)
    mask = slot < lengths.unsqueeze(1)
    return (off[:-1].unsqueeze(1) + slot).clamp_(max=max(rec.shape[0] - 1, 0)), mask, lengths


def torch_newton(D, c, z, mask, v, l2):
    """Batched damped Newton on f(v) = sum softplus(x) - z x + (l2 / 2) |v|^2, x = D v + c, padded and masked, from v →
    (v*, f(start), f(v*), iterations)."""
    rows, d = v.shape

    def f_of(w):
        x = torch.bmm(D, w.unsqueeze(2)).squeeze(2) + c
        terms = (torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs())) - z * x) * mask
        return terms.sum(1) + 0.5 * l2 * (w * w).sum(1)

    f = f_start = f_of(v)
    active = mask.any(1)
    iters = torch.zeros(rows, dtype=torch.int32, device=dev)
    eye = l2 * torch.eye(d, dtype=torch.float64, device=dev)
    for _ in range(MAX_ITER):
        if not bool(active.any()):
            break
        iters += active.int()
        p = torch.sigmoid(torch.bmm(D, v.unsqueeze(2)).squeeze(2) + c)
        g = torch.bmm(D.transpose(1, 2), ((p - z) * mask).unsqueeze(2)).squeeze(2) + l2 * v
        H = torch.bmm(D.transpose(1, 2), D * (p * (1.0 - p) * mask).unsqueeze(2)) + eye
        s = -torch.cholesky_solve(g.unsqueeze(2), torch.linalg.cholesky(H)).squeeze(2)
        gs = (g * s).sum(1)
        t = torch.ones(rows, dtype=torch.float64, device=dev)
        todo = active & (s != 0).any(1)
        active = todo.clone()
        accepted = torch.zeros_like(todo)
        f_new, v_new = f.clone(), v.clone()
        for _h in range(HALVINGS + 1):
            trial = v + t.unsqueeze(1) * s
            f_trial = f_of(trial)
            ok = todo & (f_trial <= f + 1e-4 * t * gs)
            v_new[ok], f_new[ok] = trial[ok], f_trial[ok]
            accepted |= ok
            todo &= ~ok
            if not bool(todo.any()):
                break
            t = torch.where(todo, t * 0.5, t)
        step = t * s.abs().max(1)[0]
        v, f = v_new, f_new
        active &= accepted & ~(step <= XTOL * v.abs().max(1)[0])
    return v, f_start, f, iters


def torch_item_step(U, V, rec, off, l2, theta):
    at, mask, _ = padded(rec, off)
    Ud, Vd = U.double(), V.double()
    u, i, j = (rec[:, k].long()[at] for k in range(3))
    own = torch.arange(V.shape[0], device=dev).unsqueeze(1)
    sigma = ((i == own).double() - (j == own).double()) * mask
    D = sigma.unsqueeze(2) * Ud[u]
    c = -sigma * (Ud[u] * Vd[torch.where(i == own, j, i)]).sum(2)
    z = rec[:, 3].contiguous().view(torch.float32).double()[at] * mask
    v, _, _, iters = torch_newton(D, c, z, mask, Vd.clone(), l2)
    return (Vd + theta * (v - Vd)).float(), iters


def torch_user_step(U, V, rec, off, l2):
    at, mask, _ = padded(rec, off)
    Vd = V.double()
    D = (Vd[rec[:, 1].long()[at]] - Vd[rec[:, 2].long()[at]]) * mask.unsqueeze(2)
    z = rec[:, 3].contiguous().view(torch.float32).double()[at] * mask
    v, _, _, iters = torch_newton(D, torch.zeros_like(z), z, mask, U.double(), l2)
    return v.float(), iters


def torch_sweep(U, V, data, by_user, by_item, l2):
    F = []
    U, it_u = torch_user_step(U, V, by_user[0], by_user[1], l2)
    F.append(foldin.total_objective(U, V, *data, l2))
    its = [it_u]
    for _ in range(2):
        V, it = torch_item_step(U, V, by_item[0], by_item[1], l2, 0.5)
        F.append(foldin.total_objective(U, V, *data, l2))
        its.append(it)
    return U, V, torch.stack(F), its


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "item_step.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    cases = (("notebooks n=m=1000 d=2 200000 cmp", 1000, 1000, 2, 200000),
             ("C2 n=m=4096 d=64 167772 cmp", 4096, 4096, 64, 167772))
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_item_step.py: >= {B.SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds (HIP events); calls longer than that: one warm-up, the faster of two",
             "# item step: mfcd_item_step through foldin.fold_in_items, all m items at theta = 1/2 from tables 0.1 N(0, I); "
             "sweep: alternating.fit_alternating(sweeps=1, item_steps=2), grouping included; torch: padded, masked, batched "
             "f64 Newton with the same line search and stopping rule (tools/bench_item_step.py), host waits included",
             "# work = sum over rows of records x iterations taken (by that solver; an item step has 2 N records); |dV|: "
             "largest difference of the two results relative to the largest entry of the row",
             f"{'size':36s} {'what':>9s} {'solver':>7s} {'ms/call':>10s} {'iters mean':>10s} {'most':>5s} "
             f"{'ns/(rec x it)':>13s} {'|dV|':>9s}"]
    print("\n".join(lines), flush=True)
    g = torch.Generator().manual_seed(1)

    def work_of(pairs):
        """[(lengths, iters)] → (work, mean iterations over rows with records, most)."""
        work = sum(float((ln.double() * it.double()).sum()) for ln, it in pairs)
        have = torch.cat([it[ln > 0].double() for ln, it in pairs])
        return work, float(have.mean()), int(have.max())

    for name, n, m, d, N in cases:
        U, V, u, i, j, z = make(n, m, d, N, g)
        data = (u, i, j, z)
        l2 = 1e-5 * N
        by_user, by_item = foldin.group_by_user(*data, n), foldin.group_by_item(*data, m)
        len_u, len_i = by_user[1][1:] - by_user[1][:-1], by_item[1][1:] - by_item[1][:-1]
        rows_out = []
        # one item step
        res = foldin.fold_in_items(U, V, by_item[0], by_item[1], l2, None, 0.5)
        assert int(res.status.max()) == 0, "a row did not converge"
        ms = B.timed(lambda: foldin.fold_in_items(U, V, by_item[0], by_item[1], l2, None, 0.5))
        rows_out.append(("item step", "kernel", ms, [(len_i, res.iters)], None))
        Vt, it = torch_item_step(U, V, by_item[0], by_item[1], l2, 0.5)
        scale = res.V.abs().max(1)[0].clamp_(min=1e-30)
        dv = float(((Vt - res.V).abs().max(1)[0] / scale).max())
        ms = B.timed(lambda: torch_item_step(U, V, by_item[0], by_item[1], l2, 0.5))
        rows_out.append(("item step", "torch", ms, [(len_i, it)], dv))
        # one sweep: a user step and two item steps
        a = foldin.fold_in_users(V, by_user[0], by_user[1], l2, U)
        b = foldin.fold_in_items(a.U, V, by_item[0], by_item[1], l2, None, 0.5)
        c = foldin.fold_in_items(a.U, b.V, by_item[0], by_item[1], l2, None, 0.5)
        one = alternating.fit_alternating(U, V, *data, l2, sweeps=1, item_steps=2)
        assert torch.equal(one.V, c.V) and int(one.user_status.max()) == 0 and int(one.item_status.max()) == 0
        ms = B.timed(lambda: alternating.fit_alternating(U, V, *data, l2, sweeps=1, item_steps=2))
        rows_out.append(("sweep", "kernel", ms, [(len_u, a.iters), (len_i, b.iters), (len_i, c.iters)], None))
        Ut, Vt, Ft, its = torch_sweep(U, V, data, by_user, by_item, l2)
        scale = one.V.abs().max(1)[0].clamp_(min=1e-30)
        dv = float(((Vt - one.V).abs().max(1)[0] / scale).max())
        ms = B.timed(lambda: torch_sweep(U, V, data, by_user, by_item, l2))
        rows_out.append(("sweep", "torch", ms, [(len_u, its[0]), (len_i, its[1]), (len_i, its[2])], dv))
        hist = [float(one.objective_start)] + one.history.reshape(-1).tolist()
        for what, solver, t_ms, pairs, dv in rows_out:
            work, mean, most = work_of(pairs)
            line = (f"{name:36s} {what:>9s} {solver:>7s} {t_ms:10.3f} {mean:10.2f} {most:5d} {t_ms * 1e6 / work:13.4f} "
                    f"{'' if dv is None else format(dv, '9.1e'):>9s}")
            print(line, flush=True)
            lines.append(line)
        line = f"# {name}: l2 = {l2:g}, F at the start and after the sweep's three sub-steps: " + " ".join(f"{x:.6f}" for x in hist)
        print(line, flush=True)
        lines.append(line)
        del U, V, data, by_user, by_item, res, a, b, c, one, Ut, Vt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
