"""Diagnostic: time the fold-in solve (mfcd/foldin.py: fold_in_users, include/mfcd.h: mfcd_fold_in_users) beside the
same solve done with torch ops on the same GPU, and write the table to profiles/fold_in.txt (or --out PATH).

  sizes    notebooks   n = m = 1000, d = 2, 250 comparisons per user
           C2          n = m = 4096, d = 64, 167 772 comparisons with uniform users (about 41 per user)
           long rows   256 users x 100 000 comparisons, m = 4096, d = 64
  data     V ~ N(0, 1 / d), hard labels from a hidden u0 ~ N(0, 9 I) per user, start at 0, l2 = 1e-5 x the number of
           comparisons (structure.refit_users' rule at weight_decay 1e-5)
  torch    rows padded to the longest user and masked, batched f64 Newton: bmm for the scores, the gradient and the
           Hessian, torch.linalg.cholesky / cholesky_solve, the same backtracking (its Armijo test on the two values of f,
           not on the term-wise decrease) and the same stopping rule, all rows
           iterated until the last one stops (a row that has stopped keeps its iterate)
  columns  ms per call; iterations (mean and most over the users with comparisons); ns per (comparison x iteration),
           with the sum over the users of comparisons x iterations taken as the work of either solver

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported; a call that takes longer than SECONDS is timed as one warm-up call and the faster of two.
Usage: bench_fold_in.py [--out PATH] [--skip-torch-long]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import torch  # noqa: E402

from mfcd import foldin  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("FOLD_IN_BENCH_SECONDS", "0.5"))
XTOL, MAX_ITER, HALVINGS = 2.0 ** -30, 50, 30


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


def best(fn):
    rounds = []
    for _ in range(2):
        stretch(fn, SECONDS / 2)
        rounds.append(stretch(fn, SECONDS))
    return min(rounds)


def make(n, m, d, per_user, total, g):
    """per_user comparisons for each of n users, or `total` comparisons with uniform users → (V, records, row_off)."""
    V = (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
    if per_user is not None:
        u = torch.arange(n).repeat_interleave(per_user)
    else:
        u = torch.randint(0, n, (total,), generator=g)
    N = u.numel()
    i = torch.randint(0, m, (N,), generator=g)
    j = (i + 1 + torch.randint(0, m - 1, (N,), generator=g)) % m
    u, i, j = u.to(dev), i.to(dev), j.to(dev)
    U0 = 3.0 * torch.randn(n, d, generator=g).to(dev)
    x = (U0[u] * (V[i] - V[j])).sum(1)
    z = (torch.rand(N, generator=g).to(dev) < torch.sigmoid(x)).float()
    return (V,) + foldin.group_by_user(u, i, j, z, n)


def torch_solve(V, rec, off, l2):
    """The same algorithm with torch ops: rows padded to the longest user, masked, batched in f64."""
    rows, d = off.numel() - 1, V.shape[1]
    lengths = off[1:] - off[:-1]
    L = int(lengths.max())
    slot = torch.arange(L, device=dev).unsqueeze(0)
    mask = slot < lengths.unsqueeze(1)                                       # [rows, L]
    at = (off[:-1].unsqueeze(1) + slot).clamp_(max=max(rec.shape[0] - 1, 0))
    Vd = V.double()
    D = (Vd[rec[:, 1].long()[at]] - Vd[rec[:, 2].long()[at]]) * mask.unsqueeze(2)   # [rows, L, d], 0 in the padding
    z = rec[:, 3].contiguous().view(torch.float32).double()[at] * mask

    def f_of(u):
        x = torch.bmm(D, u.unsqueeze(2)).squeeze(2)
        terms = (torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs())) - z * x) * mask
        return terms.sum(1) + 0.5 * l2 * (u * u).sum(1)

    u = torch.zeros(rows, d, dtype=torch.float64, device=dev)
    f = f_of(u)
    active = lengths > 0
    iters = torch.zeros(rows, dtype=torch.int32, device=dev)
    eye = l2 * torch.eye(d, dtype=torch.float64, device=dev)
    for _ in range(MAX_ITER):
        if not bool(active.any()):
            break
        iters += active.int()
        x = torch.bmm(D, u.unsqueeze(2)).squeeze(2)
        p = torch.sigmoid(x)
        g = torch.bmm(D.transpose(1, 2), ((p - z) * mask).unsqueeze(2)).squeeze(2) + l2 * u
        H = torch.bmm(D.transpose(1, 2), D * (p * (1.0 - p) * mask).unsqueeze(2)) + eye
        s = -torch.cholesky_solve(g.unsqueeze(2), torch.linalg.cholesky(H)).squeeze(2)
        gs = (g * s).sum(1)
        t = torch.ones(rows, dtype=torch.float64, device=dev)
        todo = active & (s != 0).any(1)
        active = todo.clone()                                                # a step of exactly 0: converged
        accepted = torch.zeros_like(todo)
        f_new, u_new = f.clone(), u.clone()
        for _h in range(HALVINGS + 1):
            trial = u + t.unsqueeze(1) * s
            f_trial = f_of(trial)
            ok = todo & (f_trial <= f + 1e-4 * t * gs)
            u_new[ok], f_new[ok] = trial[ok], f_trial[ok]
            accepted |= ok
            todo &= ~ok
            if not bool(todo.any()):
                break
            t = torch.where(todo, t * 0.5, t)
        step = t * s.abs().max(1)[0]
        u, f = u_new, f_new
        active &= accepted & ~(step <= XTOL * u.abs().max(1)[0])
    return u.float(), f, iters


def timed(fn):
    """ms per call: stretches for a short call, one warm-up and the faster of two for a long one."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    first = t0.elapsed_time(t1)
    if first < SECONDS * 1e3 / 4:
        return best(fn)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return min(first, t0.elapsed_time(t1))


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "fold_in.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    cases = (("notebooks n=m=1000 d=2 250/user", 1000, 1000, 2, 250, None),
             ("C2 n=m=4096 d=64 167772 rec", 4096, 4096, 64, None, 167772),
             ("long rows 256 x 100000 d=64", 256, 4096, 64, 100000, None))
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_fold_in.py: >= {SECONDS} s per stretch after an untimed "
             "stretch, min of two rounds (HIP events); calls longer than that: one warm-up, the faster of two",
             "# kernel: mfcd_fold_in_users through foldin.fold_in_users; torch: padded, masked, batched f64 Newton with the "
             "same line search and stopping rule (tools/bench_fold_in.py: torch_solve), host waits included",
             "# work = sum over users of comparisons x iterations taken (by that solver); |dU|: largest difference of the two "
             "solutions relative to the largest entry of the row",
             f"{'size':34s} {'solver':>7s} {'ms/call':>10s} {'iters mean':>10s} {'most':>5s} {'ns/(cmp x it)':>13s} {'|dU|':>9s}"]
    print("\n".join(lines), flush=True)
    g = torch.Generator().manual_seed(1)
    for name, n, m, d, per_user, total in cases:
        V, rec, off = make(n, m, d, per_user, total, g)
        l2 = 1e-5 * rec.shape[0]
        lengths = (off[1:] - off[:-1]).double()
        res = foldin.fold_in_users(V, rec, off, l2)
        assert int(res.status.max()) == 0, "a row did not converge"
        ms = timed(lambda: foldin.fold_in_users(V, rec, off, l2))
        rows_out = [("kernel", ms, res.iters, None)]
        if not (per_user == 100000 and "--skip-torch-long" in args):
            Ut, ft, it = torch_solve(V, rec, off, l2)
            scale = res.U.abs().max(1)[0].clamp_(min=1e-30)
            du = float(((Ut - res.U).abs().max(1)[0] / scale).max())
            rows_out.append(("torch", timed(lambda: torch_solve(V, rec, off, l2)), it, du))
            del Ut, ft
        for solver, t_ms, it, du in rows_out:
            itd = it.double()
            work = float((lengths * itd).sum())
            have = lengths > 0
            line = (f"{name:34s} {solver:>7s} {t_ms:10.3f} {float(itd[have].mean()):10.2f} {int(it.max()):5d} "
                    f"{t_ms * 1e6 / work:13.4f} {'' if du is None else format(du, '9.1e'):>9s}")
            print(line, flush=True)
            lines.append(line)
        del V, rec, off, res
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
