"""The exact user step of the BTL fit on the device (include/mfcd.h: mfcd_fold_in_users): with the item table V held
fixed, every user's row is the minimiser of its own l2-regularised logistic regression on delta_t = V[i_t] - V[j_t], found
by a damped Newton iteration, one workgroup per user.

`group_by_user` sorts comparisons by user (stable) into the records and row offsets the kernel reads; `fold_in_users` is
the kernel call; `row_objective` forms the same objective at given rows with torch ops in f64 (a diagnostic, not a
second solver).  There is no CPU form of the solve."""
import collections

import torch

from . import _lib

FoldInResult = collections.namedtuple("FoldInResult", ("U", "objective", "iters", "status"))
FoldInResult.__doc__ = """What `fold_in_users` returns, all on V's device: U fp32 [rows, d]; objective f64 [rows], the sum
over the row's comparisons of softplus(x) - z x plus (l2 / 2) |u|^2 at the solution; iters int32 [rows]; status int32
[rows]: 0 converged, 1 stopped (iteration cap or a line search without decrease), 2 invalid data (the row is NaN)."""

CONVERGED, STOPPED, INVALID = 0, 1, 2


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


def fold_in_users(V, records, row_off, l2, U_init=None, max_iter=50, xtol=2.0 ** -30):
    """V fp32 [m, d] on a GPU, `records` / `row_off` as `group_by_user` returns them (rows = len(row_off) - 1), l2 > 0 →
    FoldInResult: per row the minimiser of sum_t softplus(u . delta_t) - z_t u . delta_t + (l2 / 2) |u|^2 by the Newton
    iteration include/mfcd.h fixes, started at U_init (fp32 [rows, d]; None: at 0).  Rows with invalid data get status 2
    and NaN; nothing is read outside the tables.  Deterministic, and a row's result does not depend on the other rows.
    Nothing waits for the device."""
    if not torch.is_tensor(V) or not V.is_cuda or V.dtype != torch.float32 or V.dim() != 2:
        raise _lib.MfcdError("fold_in_users needs V as a float32 [m, d] tensor on a GPU device (there is no CPU fallback)")
    if not torch.is_tensor(records) or not records.is_cuda or records.dtype != torch.int32 or records.dim() != 2 \
            or records.shape[1] != 4 or not torch.is_tensor(row_off) or not row_off.is_cuda \
            or row_off.dtype != torch.int64 or row_off.dim() != 1 or row_off.numel() < 1:
        raise _lib.MfcdError("fold_in_users needs int32 [N, 4] records and int64 [rows + 1] offsets on the GPU "
                             "(mfcd.foldin.group_by_user makes them)")
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
    U = torch.empty((rows, d), dtype=torch.float32, device=dev)
    objective = torch.empty(rows, dtype=torch.float64, device=dev)
    info = torch.empty((rows, 2), dtype=torch.int32, device=dev)
    need = L.mfcd_fold_in_workspace_bytes(rows, d)
    if need == 0:
        raise _lib.MfcdError(f"d = {d} is outside the fold-in kernel's range [1, {L.mfcd_fold_in_max_d()}]")
    ws = _lib.workspace(need, dev)
    _lib.check(L.mfcd_fold_in_users(V.data_ptr(), m, d, records.data_ptr() if records.numel() else None,
                                    row_off.data_ptr(), rows, float(l2), _lib.ptr(U_init), int(max_iter), float(xtol),
                                    U.data_ptr(), objective.data_ptr(), info.data_ptr(), _lib.ptr(ws), ws.numel(),
                                    _lib.stream_ptr(dev)))
    return FoldInResult(U, objective, info[:, 0], info[:, 1])


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
