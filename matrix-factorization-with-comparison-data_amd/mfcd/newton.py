"""Joint second-order fit of the regularised BTL objective on sampled comparisons
    F(U, V) = sum_t softplus(x_t) - z_t x_t + (l2 / 2)(|U|^2 + |V|^2),   x_t = U[u_t] . (V[i_t] - V[j_t]),
on the device kernel include/mfcd.h: mfcd_triplet_rows, which forms the gradient, the Jacobi diagonal and the exact (or
Gauss-Newton) Hessian-vector product of F with respect to both tables, every output row with one owner and no
floating-point atomics.  `group_rows` / `segment_rows` prepare the comparisons, `triplet_rows` is the kernel call,
`triplet_pass` and `triplet_hvp` put the user and the item side together, and `fit_newton` is a trust-region Newton-CG
iteration on them (tests/newton_model.py restates it in numpy).  mfcd.alternating descends the same F one block at a
time; this module moves both tables at once.

The data term of F is invariant under U -> U A, V -> V A^-T and the penalty under orthogonal A, so the minimisers form an
O(d) orbit and the joint Hessian is singular along d (d - 1) / 2 directions at every one of them.  The gradient is
orthogonal to the orbit, and CG started from 0 stays in the range of the Hessian: it solves the system all the same, which
a factorisation would not.  There is no CPU form of any of this."""
import collections

import torch

from . import _lib, foldin

Rows = collections.namedtuple("Rows", ("records", "row_off", "seg_off", "n_seg"))
Rows.__doc__ = """One side's comparisons as mfcd_triplet_rows reads them: `records` / `row_off` of foldin.group_by_user
(or group_by_item), and `seg_off` / `n_seg` of `segment_rows(row_off)`."""

NewtonResult = collections.namedtuple("NewtonResult", ("U", "V", "history", "grad_inf", "cg_iters", "products", "status"))
NewtonResult.__doc__ = """What `fit_newton` returns: U fp32 [n, d] and V fp32 [m, d], the f64 iterate rounded once;
history f64 [iterations], F at the iterate every outer iteration starts from; grad_inf f64 [iterations], |grad F|_inf
there; cg_iters int64 [iterations], the Hessian products of each CG solve (shorter by one when the last iteration only
certifies); products, the total of Hessian products (an int); status, 0 certified or 1 stopped (an int)."""

CERTIFIED, STOPPED = 0, 1
CG_BLOCK = 8                  # CG iterations between two reads of the `done` flag
PRED_FLOOR = 2.0 ** -44


def segment_rows(row_off):
    """row_off int64 [rows + 1] → (seg_off int64 [rows + 1] on its device, n_seg): the prefix sum of ceil(len_r / S) with
    S = mfcd_triplet_rows_segment(), and its total.  Torch ops; the one host read here happens once per grouping."""
    S = _lib.load().mfcd_triplet_rows_segment()
    lengths = row_off[1:] - row_off[:-1]
    seg_off = torch.zeros_like(row_off)
    seg_off[1:] = torch.cumsum((lengths + (S - 1)) // S, 0)
    return seg_off, int(seg_off[-1])


def group_rows(u, i, j, z, n, m):
    """Comparisons (u, i, j, z) on one device → (by_user, by_item), two `Rows`: grouped once per side by
    foldin.group_by_user / group_by_item and cut into segments."""
    by_user = foldin.group_by_user(u, i, j, z, n)
    by_item = foldin.group_by_item(u, i, j, z, m)
    return Rows(*by_user, *segment_rows(by_user[1])), Rows(*by_item, *segment_rows(by_item[1]))


def _as_rows(by):
    return by if isinstance(by, Rows) else Rows(by[0], by[1], *segment_rows(by[1]))


def _f64_table(t, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2:
        raise _lib.MfcdError(f"the triplet kernel needs {name} as a float64 [rows, d] tensor on a GPU device (there is no "
                             "CPU fallback)")
    return t.detach().contiguous()


def triplet_rows(side, pas, U, V, rows, l2, P=None, Q=None, gauss_newton=False, row_id=None):
    """One call of mfcd_triplet_rows.  side 0 users / 1 items; pas 0 gradient / 1 Hessian-vector product; U f64 [n, d],
    V f64 [m, d] (and the direction P, Q of the same shapes for pas = 1) on a GPU; `rows` a `Rows` of that side; row_id
    int32 [rows] (None: row r owns table row r) → (out f64 [rows, d], diag f64 [rows, d] or None, loss f64 [rows] or None,
    status int32 [rows]).  diag exists for pas = 0 and loss for pas = 0, side = 0.  Rows with invalid data get status 2
    and NaN.  Nothing waits for the device."""
    L = _lib.load()
    U, V = _f64_table(U, "U"), _f64_table(V, "V")
    dev = U.device
    (n, d), m = U.shape, V.shape[0]
    if V.shape[1] != d or V.device != dev:
        raise _lib.MfcdError("U and V must have one width and one device")
    if not 1 <= d <= 256:
        raise _lib.MfcdError(f"d = {d} is outside the triplet kernel's range [1, 256]")
    if pas:
        P, Q = _f64_table(P, "P"), _f64_table(Q, "Q")
        if P.shape != U.shape or Q.shape != V.shape or P.device != dev or Q.device != dev:
            raise _lib.MfcdError("the direction (P, Q) must have the shapes and the device of (U, V)")
    records, row_off, seg_off, n_seg = rows
    for t, dtype in ((records, torch.int32), (row_off, torch.int64), (seg_off, torch.int64)):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype:
            raise _lib.MfcdError("the triplet kernel needs int32 [N, 4] records and int64 offsets on the tables' device "
                                 "(mfcd.newton.group_rows makes them)")
    records, row_off, seg_off = records.contiguous(), row_off.contiguous(), seg_off.contiguous()
    nrows = row_off.numel() - 1
    if records.dim() != 2 or records.shape[1] != 4 or nrows < 0 or seg_off.numel() != nrows + 1:
        raise _lib.MfcdError("records must be [N, 4] and seg_off as long as row_off")
    if row_id is not None:
        if not torch.is_tensor(row_id) or tuple(row_id.shape) != (nrows,) or row_id.dtype != torch.int32:
            raise _lib.MfcdError(f"row_id must be an int32 [{nrows}] tensor")
        row_id = row_id.to(dev).contiguous()
    out = torch.empty((nrows, d), dtype=torch.float64, device=dev)
    dg = torch.empty((nrows, d), dtype=torch.float64, device=dev) if not pas else None
    ls = torch.empty(nrows, dtype=torch.float64, device=dev) if not pas and side == 0 else None
    status = torch.empty(nrows, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_triplet_rows_workspace_bytes(nrows, d, int(n_seg)), dev)
    _lib.check(L.mfcd_triplet_rows(int(side), int(pas), int(bool(gauss_newton)), U.data_ptr(), n, V.data_ptr(), m, d,
                                   _lib.ptr(P) if pas else None, _lib.ptr(Q) if pas else None,
                                   records.data_ptr() if records.numel() else None, row_off.data_ptr(), _lib.ptr(row_id),
                                   nrows, seg_off.data_ptr(), int(n_seg), float(l2), out.data_ptr(), _lib.ptr(dg),
                                   _lib.ptr(ls), status.data_ptr(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return out, dg, ls, status


def triplet_pass(U, V, by_user, by_item, l2):
    """U f64 [n, d], V f64 [m, d] on a GPU, the two sides' `Rows` (of `group_rows`; a (records, row_off) pair is cut into
    segments here, at the price of a host read) → (F, gU, gV, DU, DV): the objective (a 0-dim f64 tensor: the users' row
    losses plus (l2 / 2)(|U|^2 + |V|^2), summed with torch.sum), its gradient and the Jacobi diagonal of its Hessian,
    from one kernel call per side.  A side with invalid data makes F and its gradient NaN."""
    gU, DU, loss, _ = triplet_rows(0, 0, U, V, _as_rows(by_user), l2)
    gV, DV, _, _ = triplet_rows(1, 0, U, V, _as_rows(by_item), l2)
    F = torch.sum(loss) + 0.5 * float(l2) * (torch.sum(U * U) + torch.sum(V * V))
    return F, gU, gV, DU, DV


def triplet_hvp(U, V, by_user, by_item, P, Q, l2, gauss_newton=False):
    """→ (HU, HV): the Hessian of F at (U, V) applied to the direction (P, Q), f64; with `gauss_newton` the positive
    semidefinite part sum_t w_t (grad x_t)(grad x_t)^T + l2 I of it."""
    HU = triplet_rows(0, 1, U, V, _as_rows(by_user), l2, P, Q, gauss_newton)[0]
    HV = triplet_rows(1, 1, U, V, _as_rows(by_item), l2, P, Q, gauss_newton)[0]
    return HU, HV


def _steihaug(product, g, D, radius, tol, cap):
    """Preconditioned CG on H s = -g from s = 0 inside |s|_M <= radius, M = diag(D), until |r|_{M^-1} <= tol, a direction
    of non-positive curvature or the boundary (both end on the boundary along p), or `cap` products.  Every decision is a
    device-side mask, so the iterations after the end of a solve change nothing; the host reads the `done` flag once per
    CG_BLOCK iterations.  → (s, hit, iterations), the last two 0-dim tensors."""
    s, r = torch.zeros_like(g), g.clone()
    p = -r / D
    rz = torch.sum(r * r / D)
    done = torch.zeros((), dtype=torch.bool, device=g.device)
    hit, iters, r2 = done.clone(), torch.zeros((), dtype=torch.int64, device=g.device), radius * radius
    k = 0
    while k < cap:
        for _ in range(min(CG_BLOCK, cap - k)):
            k += 1
            Hp = product(p)
            pHp = torch.sum(p * Hp)
            live = ~done
            broken = ~torch.isfinite(pHp)
            alpha = torch.where(pHp > 0, rz / pHp, torch.zeros_like(pHp))
            s_new = s + alpha * p
            cross = ~broken & ((pHp <= 0) | (torch.sum(D * s_new * s_new) >= r2))
            a, b, c = torch.sum(D * p * p), torch.sum(D * s * p), torch.sum(D * s * s) - r2
            tau = (-b + torch.sqrt(torch.clamp(b * b - a * c, min=0.0))) / a
            r_new = r + alpha * Hp
            z = r_new / D
            rz_new = torch.sum(r_new * z)
            ends = broken | cross | (torch.sqrt(rz_new) <= tol)
            step = live & ~broken & ~cross
            s = torch.where(live & cross, s + tau * p, torch.where(step, s_new, s))
            r = torch.where(step, r_new, r)
            go = live & ~ends
            p = torch.where(go, -z + (rz_new / rz) * p, p)
            rz = torch.where(go, rz_new, rz)
            hit = hit | (live & cross)
            iters = iters + live
            done = done | ends
        if bool(done):
            break
    return s, hit, iters


def fit_newton(U, V, u, i, j, z, l2, max_iter=100, gtol=2.0 ** -26, cg_cap=None):
    """U [n, d], V [m, d] on a GPU (any float type; d <= 256), comparisons (u, i, j, z), l2 > 0 → NewtonResult: a
    trust-region Newton-CG descent of F in both tables at once, on an f64 iterate that is rounded to fp32 once, on output.

    Every outer iteration starts from a gradient pass (F, g and the Jacobi diagonal M of the Hessian) and stops with status
    0 when |g|_inf <= gtol l2 max(|U|_inf, |V|_inf).  Otherwise Steihaug CG, preconditioned by M and with the trust
    region in the M-norm, solves H s = -g with the exact Hessian to |r|_{M^-1} <= eta |g|_{M^-1}, eta = min(0.1,
    |g|_{M^-1}^(1/2)); non-positive curvature and a step across the radius end on the boundary; at most 2 (n + m) d
    iterations (`cg_cap`).  The first radius is |M^-1 g|_M.  One more product gives pred = -(g.s + s.Hs / 2) and a
    gradient pass at the trial point act = F - F_trial.  Where pred <= 2^-44 |F| the ratio is at its rounding level: the
    step is accepted if |g|_{M^-1} fell (and F keeps the lower of the two values, which differ by their rounding alone),
    otherwise radius <- |s|_M / 4.  Elsewhere rho = act / pred: rho < 1/4 gives radius <- |s|_M / 4, rho > 3/4 on the
    boundary doubles it, and the step is accepted when rho > 1e-4.  Status 1 after `max_iter` outer iterations, or at an
    F or a gradient that is not finite (invalid comparisons make them NaN).

    The vector algebra is torch f64 on the device and every branch of the iteration is a device-side mask; the host reads
    one flag per 8 CG iterations and one set of three scalars per outer iteration.  The inputs are not modified.
    Deterministic: two runs are bit-equal."""
    if not torch.is_tensor(U) or not torch.is_tensor(V) or not U.is_cuda or not V.is_cuda:
        raise _lib.MfcdError("fit_newton needs U and V on a GPU device (there is no CPU fallback)")
    if U.dim() != 2 or V.dim() != 2 or U.shape[1] != V.shape[1]:
        raise _lib.MfcdError("fit_newton needs U [n, d] and V [m, d]")
    if not float(l2) > 0.0:
        raise ValueError("l2 must be > 0")
    dev = V.device
    (n, d), m = U.shape, V.shape[0]
    l2, gtol = float(l2), float(gtol)
    cap = 2 * (n + m) * d if cg_cap is None else int(cg_cap)
    u, i, j, z = (torch.as_tensor(t).reshape(-1).to(dev) for t in (u, i, j, z))
    by_user, by_item = group_rows(u, i, j, z, n, m)
    cut = n * d

    def split(v):
        return v[:cut].view(n, d), v[cut:].view(m, d)

    def grad_at(v):
        F, gU, gV, DU, DV = triplet_pass(*split(v), by_user, by_item, l2)
        return F, torch.cat((gU.reshape(-1), gV.reshape(-1))), torch.cat((DU.reshape(-1), DV.reshape(-1)))

    def product_at(v):
        return lambda q: torch.cat([h.reshape(-1) for h in triplet_hvp(*split(v), by_user, by_item, *split(q), l2)])

    x = torch.cat((U.detach().to(dev).double().reshape(-1), V.detach().double().reshape(-1)))
    F, g, D = grad_at(x)
    radius, history, grad_inf, cg_iters, status = None, [], [], [], STOPPED
    for _ in range(int(max_iter)):
        Fh, ginf, xmax = torch.stack((F, g.abs().max(), x.abs().max())).tolist()       # the one read of this iteration
        history.append(F)
        grad_inf.append(ginf)
        if not (Fh == Fh and abs(Fh) != float("inf") and ginf == ginf and ginf != float("inf")):
            break
        if ginf <= gtol * l2 * xmax:
            status = CERTIFIED
            break
        gnorm = torch.sqrt(torch.sum(g * g / D))
        if radius is None:
            radius = gnorm                                                              # |M^-1 g|_M
        tol = torch.clamp(torch.sqrt(gnorm), max=0.1) * gnorm
        product = product_at(x)
        s, hit, iters = _steihaug(product, g, D, radius, tol, cap)
        cg_iters.append(iters)
        pred = -(torch.sum(g * s) + 0.5 * torch.sum(s * product(s)))
        xt = x + s
        Ft, gt, Dt = grad_at(xt)
        snorm = torch.sqrt(torch.sum(D * s * s))
        floor = pred <= PRED_FLOOR * F.abs()               # the ratio act / pred is at its rounding level
        rho = (F - Ft) / pred
        accept = torch.where(floor, torch.sqrt(torch.sum(gt * gt / D)) < gnorm, rho > 1e-4)
        shrink = torch.where(floor, ~accept, rho < 0.25)
        grow = ~floor & ~shrink & (rho > 0.75) & hit
        radius = torch.where(shrink, 0.25 * snorm, torch.where(grow, 2.0 * radius, radius))
        Ft = torch.where(floor, torch.minimum(F, Ft), Ft)
        x, F, g, D = (torch.where(accept, new, old) for new, old in ((xt, x), (Ft, F), (gt, g), (Dt, D)))
    Uf, Vf = split(x)
    cg = torch.stack(cg_iters) if cg_iters else torch.zeros(0, dtype=torch.int64, device=dev)
    return NewtonResult(Uf.float(), Vf.float(), torch.stack(history), torch.tensor(grad_inf, dtype=torch.float64, device=dev),
                        cg, int(cg.sum()) + len(cg_iters), status)
