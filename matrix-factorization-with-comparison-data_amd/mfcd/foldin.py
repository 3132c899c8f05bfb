"""The exact block steps of the BTL fit on the device (include/mfcd.h: mfcd_fold_in_users, mfcd_item_step and their
_cg forms).  With the item table V held fixed, every user's row is the minimiser of its own l2-regularised logistic
regression on delta_t = V[i_t] - V[j_t]; with U and the other items held fixed, an item's row is the minimiser of a
logistic regression with an offset over the comparisons that hold it.  Both are found by a damped Newton iteration, one
workgroup per row, in one of two forms (`method`): "cholesky" factors the d x d Hessian in LDS (d <= 64), "cg" takes the
step from conjugate gradients on Hessian-vector products (d <= 256); "auto" is cholesky wherever it applies.

`group_by_user` / `group_by_item` sort comparisons (stable) into the records and row offsets the kernel reads;
`fold_in_users` / `fold_in_items` / `fold_in_items_cg` are the kernel calls; `row_objective` and `total_objective` form
the objectives with torch ops in f64 (diagnostics, not second solvers).  There is no CPU form of the solves."""
import collections

import torch

from . import _lib

class FoldInResult(collections.namedtuple("FoldInResult", ("U", "objective", "iters", "status"))):
    """What `fold_in_users` returns, all on V's device: U fp32 [rows, d]; objective f64 [rows], the sum over the row's
    comparisons of softplus(x) - z x plus (l2 / 2) |u|^2 at the solution; iters int32 [rows] (Newton iterations; CG
    solves for the CG form); status int32 [rows]: 0 converged, 1 stopped (iteration cap or a line search without
    decrease), 2 invalid data (the row is NaN).  The attribute `cg_iters` (not a field of the tuple) is int32 [rows],
    the CG iterations of each row, for the CG form and None for the Cholesky form."""
    cg_iters = None

CONVERGED, STOPPED, INVALID = 0, 1, 2
METHODS = ("auto", "cholesky", "cg")


def _use_cg(L, d, method, what):
    """Which solver a call of width d takes: False the Cholesky form, True the CG form; MfcdError beyond both."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    top = L.mfcd_fold_in_cg_max_d() if method != "cholesky" else L.mfcd_fold_in_max_d()
    if not 1 <= d <= top:
        raise _lib.MfcdError(f"d = {d} is outside {what}'s range [1, {top}]"
                             + (" (method=\"cholesky\")" if method == "cholesky" else ""))
    return method == "cg" or (method == "auto" and d > L.mfcd_fold_in_max_d())


def _check_records(name, maker, records, row_off):
    """The records and offsets of a call of `name` as tensors; `maker` is the function that makes them."""
    if not torch.is_tensor(records) or not records.is_cuda or records.dtype != torch.int32 or records.dim() != 2 \
            or records.shape[1] != 4 or not torch.is_tensor(row_off) or not row_off.is_cuda \
            or row_off.dtype != torch.int64 or row_off.dim() != 1 or row_off.numel() < 1:
        raise _lib.MfcdError(f"{name} needs int32 [N, 4] records and int64 [rows + 1] offsets on the GPU "
                             f"(mfcd.foldin.{maker} makes them)")


def _solve(L, method, what, result, dev, rows, d, cholesky, cg, head, max_iter):
    """One call of the entry `method` selects at width d → `result` of (the rows, the columns of the objective, iters,
    status), its attribute `cg_iters` (not a field of the tuple) set for the CG form.  `cholesky` and `cg`: the form's
    (entry, workspace bytes, stop tolerance).  `head`: the entry's arguments before max_iter; what follows them is the
    same for all four entries but for cg_iters."""
    use_cg = _use_cg(L, d, method, what)
    entry, ws_bytes, tol = cg if use_cg else cholesky
    out = torch.empty((rows, d), dtype=torch.float32, device=dev)
    objective = torch.empty((rows, len(result._fields) - 3), dtype=torch.float64, device=dev)
    info = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    cg_iters = torch.empty(rows, dtype=torch.int32, device=dev) if use_cg else None
    ws = _lib.workspace(ws_bytes, dev)
    _lib.check(entry(*head, int(max_iter), float(tol), out.data_ptr(), objective.data_ptr(), info.data_ptr(),
                     *((cg_iters.data_ptr(),) if use_cg else ()), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    res = result(out, *objective.unbind(1), info[:, 0], info[:, 1])
    res.cg_iters = cg_iters
    return res


def group_by_user(u, i, j, z, n):
    """Comparisons (u, i, j, z) as four tensors of one length on one device → (records int32 [N, 4] in the 16-byte
    mfcd_sample layout, z as fp32 bits; row_off int64 [n + 1]), on that device: the comparisons sorted by user with a
    stable sort, so that a user's comparisons keep their order, and user r's are records[row_off[r]:row_off[r + 1]]
    (an empty range for a user without any).  IndexError for a user outside [0, n)."""
    u, i, j, z = (torch.as_tensor(t).reshape(-1) for t in (u, i, j, z))
    if not (u.numel() == i.numel() == j.numel() == z.numel()):
        raise ValueError("u, i, j and z must have one length")
    n = int(n)
    u = u.to(torch.int64)
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= n):
        raise IndexError(f"a user number lies outside [0, {n})")
    order = torch.sort(u, stable=True)[1]
    zbits = z.to(device=u.device, dtype=torch.float32).view(torch.int32)
    rec = torch.stack((u.to(torch.int32), i.to(device=u.device, dtype=torch.int32),
                       j.to(device=u.device, dtype=torch.int32), zbits), dim=1)[order].contiguous()
    row_off = torch.zeros(n + 1, dtype=torch.int64, device=u.device)
    row_off[1:] = torch.cumsum(torch.bincount(u, minlength=n), 0)
    return rec, row_off


def fold_in_users(V, records, row_off, l2, U_init=None, max_iter=50, xtol=2.0 ** -30, gtol=2.0 ** -26, method="auto"):
    """V fp32 [m, d] on a GPU, `records` / `row_off` as `group_by_user` returns them (rows = len(row_off) - 1), l2 > 0 →
    FoldInResult: per row the minimiser of sum_t softplus(u . delta_t) - z_t u . delta_t + (l2 / 2) |u|^2 by the Newton
    iteration include/mfcd.h fixes, started at U_init (fp32 [rows, d]; None: at 0).  method: "cholesky" (d <= 64; stops
    on a step below xtol |u|_inf), "cg" (d <= 256; stops on |g|_2 <= l2 gtol |u|_inf), "auto": cholesky for d <= 64 and
    cg above.  Rows with invalid data get status 2 and NaN; nothing is read outside the tables.  Deterministic, and a
    row's result does not depend on the other rows.  Nothing waits for the device."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")
    if not torch.is_tensor(V) or not V.is_cuda or V.dtype != torch.float32 or V.dim() != 2:
        raise _lib.MfcdError("fold_in_users needs V as a float32 [m, d] tensor on a GPU device (there is no CPU fallback)")
    _check_records("fold_in_users", "group_by_user", records, row_off)
    L = _lib.load()
    dev = V.device
    V = V.detach().contiguous()
    records, row_off = records.to(dev).contiguous(), row_off.to(dev).contiguous()
    m, d = V.shape
    rows = row_off.numel() - 1
    if U_init is not None:
        if not torch.is_tensor(U_init) or tuple(U_init.shape) != (rows, d) or U_init.dtype != torch.float32:
            raise _lib.MfcdError(f"U_init must be a float32 [{rows}, {d}] tensor")
        U_init = U_init.detach().to(dev).contiguous()
    head = (V.data_ptr(), m, d, records.data_ptr() if records.numel() else None, row_off.data_ptr(), rows, float(l2),
            _lib.ptr(U_init))
    return _solve(L, method, "the fold-in kernel", FoldInResult, dev, rows, d,
                  (L.mfcd_fold_in_users, L.mfcd_fold_in_workspace_bytes(rows, d), xtol),
                  (L.mfcd_fold_in_users_cg, L.mfcd_fold_in_cg_workspace_bytes(rows, d, records.shape[0]), gtol),
                  head, max_iter)


def row_objective(U, V, records, row_off, l2):
    """The objective of `fold_in_users` at the rows of U, with torch ops in f64 → f64 [rows] on the device."""
    rows = row_off.numel() - 1
    Ud, Vd = U.detach().double(), V.detach().double()
    lengths = row_off[1:] - row_off[:-1]
    owner = torch.repeat_interleave(torch.arange(rows, device=row_off.device), lengths)
    i, j = records[:, 1].long(), records[:, 2].long()
    z = records[:, 3].contiguous().view(torch.float32).double()
    x = (Ud[owner] * (Vd[i] - Vd[j])).sum(1)
    terms = torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs())) - z * x
    f = torch.zeros(rows, dtype=torch.float64, device=U.device).index_add_(0, owner, terms)
    return f + 0.5 * float(l2) * (Ud * Ud).sum(1)


class ItemStepResult(collections.namedtuple("ItemStepResult", ("V", "objective_start", "objective", "iters", "status"))):
    """What `fold_in_items` returns, all on V's device: V fp32 [rows, d], the rows v_old + theta (v* - v_old);
    objective_start / objective f64 [rows], the item's objective f_k at v_old and at v*; iters int32 [rows]; status int32
    [rows] as in FoldInResult, and the attribute `cg_iters` likewise."""
    cg_iters = None


def group_by_item(u, i, j, z, m):
    """Comparisons (u, i, j, z) as four tensors of one length on one device → (records int32 [2 N, 4], row_off int64
    [m + 1]) on that device, for `fold_in_items`: every comparison appears once in the row of its i and once in the row of
    its j (so one with i = j appears twice in one row), item k's are records[row_off[k]:row_off[k + 1]].  The sort is
    stable: a row keeps the order of the comparisons, and of the two copies of one comparison the i-copy comes first.
    IndexError for an item outside [0, m)."""
    u, i, j, z = (torch.as_tensor(t).reshape(-1) for t in (u, i, j, z))
    if not (u.numel() == i.numel() == j.numel() == z.numel()):
        raise ValueError("u, i, j and z must have one length")
    m = int(m)
    dev = i.device
    i, j = i.to(torch.int64), j.to(device=dev, dtype=torch.int64)
    for t in (i, j):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= m):
            raise IndexError(f"an item number lies outside [0, {m})")
    zbits = z.to(device=dev, dtype=torch.float32).view(torch.int32)
    rec = torch.stack((u.to(device=dev, dtype=torch.int32), i.to(torch.int32), j.to(torch.int32), zbits), dim=1)
    key = torch.stack((i, j), dim=1).reshape(-1)                 # comparison t: its i-copy at 2 t, its j-copy at 2 t + 1
    order = torch.sort(key, stable=True)[1]
    rec = rec[order >> 1].contiguous()
    row_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    row_off[1:] = torch.cumsum(torch.bincount(key, minlength=m), 0)
    return rec, row_off


def fold_in_items(U, V, records, row_off, l2, row_item=None, theta=1.0, max_iter=50, xtol=2.0 ** -30):
    """U fp32 [n, d] and V fp32 [m, d] on a GPU, `records` / `row_off` as `group_by_item` returns them (rows =
    len(row_off) - 1), l2 > 0 → ItemStepResult.  Row r solves item k = row_item[r] (int32 [rows]; None: k = r): with U and
    the other rows of V fixed, v* minimises sum_t softplus(x_t) - z_t x_t + (l2 / 2) |v|^2 over the row's records,
    x_t = +-U[u_t] . (v - V[other item]), by the Newton iteration include/mfcd.h fixes, started at V[k]; the row returned
    is V[k] + theta (v* - V[k]).  theta = 1: the exact minimiser of each row on its own; theta = 1/2: all items may move
    in one call and the total objective still falls.  The solver is chosen by d as `fold_in_users` does with
    method="auto": the Cholesky form with `xtol` for d <= 64, the CG form with its default gtol above, up to 256
    (`fold_in_items_cg` is the CG form for any d <= 256, with gtol as a parameter).  Rows with invalid data get status 2
    and NaN; nothing is read outside the tables.  Deterministic, and a row's result does not depend on the other rows.
    Nothing waits for the device."""
    return _fold_in_items(U, V, records, row_off, l2, row_item, theta, max_iter, xtol, 2.0 ** -26, "auto")


def fold_in_items_cg(U, V, records, row_off, l2, row_item=None, theta=1.0, max_iter=50, gtol=2.0 ** -26):
    """`fold_in_items` by the CG form (include/mfcd.h: mfcd_item_step_cg) for any 1 <= d <= 256: a row is certified when
    |g|_2 <= l2 gtol |v|_inf.  The result's attribute `cg_iters` holds the CG iterations of each row."""
    return _fold_in_items(U, V, records, row_off, l2, row_item, theta, max_iter, 2.0 ** -30, gtol, "cg")


def _fold_in_items(U, V, records, row_off, l2, row_item, theta, max_iter, xtol, gtol, method):
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 for t in (U, V)) \
            or U.shape[1] != V.shape[1]:
        raise _lib.MfcdError("fold_in_items needs U [n, d] and V [m, d] as float32 tensors on a GPU device (there is no "
                             "CPU fallback)")
    _check_records("fold_in_items", "group_by_item", records, row_off)
    L = _lib.load()
    dev = V.device
    U, V = U.detach().to(dev).contiguous(), V.detach().contiguous()
    records, row_off = records.to(dev).contiguous(), row_off.to(dev).contiguous()
    (n, d), m = U.shape, V.shape[0]
    rows = row_off.numel() - 1
    if row_item is not None:
        if not torch.is_tensor(row_item) or tuple(row_item.shape) != (rows,) or row_item.dtype != torch.int32:
            raise _lib.MfcdError(f"row_item must be an int32 [{rows}] tensor")
        row_item = row_item.to(dev).contiguous()
    head = (U.data_ptr(), n, V.data_ptr(), m, d, records.data_ptr() if records.numel() else None, row_off.data_ptr(),
            _lib.ptr(row_item), rows, float(l2), float(theta))
    nrec = records.shape[0]
    return _solve(L, method, "the item step", ItemStepResult, dev, rows, d,
                  (L.mfcd_item_step, L.mfcd_item_step_workspace_bytes(rows, d, nrec), xtol),
                  (L.mfcd_item_step_cg, L.mfcd_item_step_cg_workspace_bytes(rows, d, nrec), gtol), head, max_iter)


def total_objective(U, V, u, i, j, z, l2):
    """F = sum_t softplus(x_t) - z_t x_t + (l2 / 2)(|U|^2 + |V|^2), x_t = U[u_t] . (V[i_t] - V[j_t]), with torch ops in
    f64 → a 0-dim f64 tensor on U's device.  Only torch.sum reductions: the value is the same from call to call."""
    Ud, Vd = U.detach().double(), V.detach().double()
    u, i, j = (torch.as_tensor(t).reshape(-1).to(device=Ud.device, dtype=torch.int64) for t in (u, i, j))
    z = torch.as_tensor(z).reshape(-1).to(device=Ud.device, dtype=torch.float64)
    x = torch.sum(Ud[u] * (Vd[i] - Vd[j]), 1)
    terms = torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs())) - z * x
    return torch.sum(terms) + 0.5 * float(l2) * (torch.sum(Ud * Ud) + torch.sum(Vd * Vd))
