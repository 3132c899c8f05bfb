"""The k best / k worst columns of rows of a score matrix on the device (include/mfcd.h: mfcd_topk_rows).

The matrix is a dense fp32 GPU tensor, or a product A @ B.T given by its factors — a `generation_data.FactoredMatrix`
or a pair (A, B) of GPU tensors — of which nothing of size n x m is ever formed (BASELINE C4: 16 GiB dense).  Order:
best first / worst first, equal scores by ascending column (a stable sort of the row), NaN above +inf for `best`.
There is no CPU form.
"""
import numpy as np
import torch

from . import _lib
from .rows import resolve

_ENDS = {"best": 1, "worst": 2, "both": 3}


def max_k():
    return int(_lib.load().mfcd_topk_max_k())


def _resolve(X, device):
    """→ (dense or None, A or None, B or None, n, m, d, device): fp32, factors contiguous, a dense X with unit column
    stride and rows that do not overlap (its row stride may exceed m)."""
    X = resolve(X, device, gpu_only=True)
    if X.factored:
        X = X.map(lambda t: t.float().contiguous())
    else:
        X = X.map(torch.Tensor.float)
        if X.dense.stride(1) != 1 or X.dense.stride(0) < X.m:
            X = X.map(torch.Tensor.contiguous)
    return X.dense, X.A, X.B, X.n, X.m, X.d, X.device


def exclude_csr(pairs, row_ids, n, m, device):
    """CSR form of a set of barred (row, column) pairs for the requested rows → (offsets int64 [rows + 1], items int32),
    both on `device`.  `pairs`: array-like / tensor / set of (u, i) or (u, i, j) rows — a triplet bars both of its items
    for its user; pairs outside the table are ignored.  `row_ids`: int64 device tensor of the requested rows."""
    if isinstance(pairs, (set, frozenset)):
        pairs = sorted(pairs)
    p = torch.as_tensor(np.asarray(pairs) if not torch.is_tensor(pairs) else pairs).to(device=device, dtype=torch.int64)
    p = p.reshape(-1, p.shape[-1]) if p.numel() else p.reshape(0, 2)
    if p.shape[1] == 3:
        p = torch.cat((p[:, :2], p[:, [0, 2]]))
    elif p.shape[1] != 2:
        raise ValueError("exclude must hold (u, i) or (u, i, j) rows")
    p = p[(p[:, 0] >= 0) & (p[:, 0] < n) & (p[:, 1] >= 0) & (p[:, 1] < m)]
    keys = torch.unique(p[:, 0] * m + p[:, 1])                     # sorted: by row, then ascending column
    users, items = keys // m, (keys % m).to(torch.int32)
    counts = torch.bincount(users, minlength=n)
    start = torch.cumsum(counts, 0) - counts                       # first entry of every row of the table
    lens = counts[row_ids]
    off = torch.zeros(row_ids.numel() + 1, dtype=torch.int64, device=device)
    off[1:] = torch.cumsum(lens, 0)
    total = int(off[-1])
    src = torch.repeat_interleave(start[row_ids] - off[:-1], lens) + torch.arange(total, device=device)
    return off.contiguous(), items[src].contiguous() if total else torch.zeros(1, dtype=torch.int32, device=device)


def topk_rows(X, k, rows=None, ends="best", exclude=None, values=False, device=None):
    """Indices (int32 device tensors [len(rows), k]) of the k best / worst columns of rows of X.

    X        dense fp32 GPU tensor [n, m], a FactoredMatrix, or a pair (A, B) of GPU tensors (X = A @ B.T)
    rows     None (every row) or row numbers in [0, n), any order
    ends     "best" → idx, "worst" → idx, "both" → (best_idx, worst_idx)
    exclude  None; pairs (u, i) / triplets (u, i, j) as a set, array or tensor (see `exclude_csr`); or a ready CSR pair
             (offsets int64 [len(rows) + 1], items int32) of device tensors.  Barred columns are absent for their row;
             when fewer than k remain the tail is index -1, value NaN
    values   also return the fp32 scores: "best" / "worst" → (idx, val), "both" → ((idx, val), (idx, val))
    """
    if ends not in _ENDS:
        raise ValueError(f"ends must be one of {sorted(_ENDS)}, got {ends!r}")
    e = _ENDS[ends]
    Xd, A, B, n, m, d, dev = _resolve(X, device)
    L = _lib.load()
    k = int(k)
    if not 1 <= k <= min(m, max_k()):
        raise ValueError(f"k = {k} outside [1, min(m = {m}, {max_k()})]")
    if rows is None:
        ids, ids64, nrows = None, None, n
    else:
        ids64 = torch.as_tensor(rows).reshape(-1).to(device=dev, dtype=torch.int64)
        nrows = ids64.numel()
        if nrows and (int(ids64.min()) < 0 or int(ids64.max()) >= n):
            raise IndexError(f"row number out of range for a matrix of {n} rows")
        ids = ids64.to(torch.int32).contiguous()
    mk = lambda dt: torch.empty((nrows, k), dtype=dt, device=dev)   # noqa: E731
    bi, wi = (mk(torch.int32) if e & 1 else None), (mk(torch.int32) if e & 2 else None)
    bv, wv = (mk(torch.float32) if values and e & 1 else None), (mk(torch.float32) if values and e & 2 else None)
    if nrows:
        off = items = None
        if exclude is not None:
            if isinstance(exclude, tuple) and len(exclude) == 2 and all(torch.is_tensor(t) for t in exclude) \
                    and exclude[0].dim() == 1 and exclude[0].numel() == nrows + 1:
                off = exclude[0].to(device=dev, dtype=torch.int64).contiguous()
                items = exclude[1].to(device=dev, dtype=torch.int32).contiguous()
                if items.numel() == 0:
                    items = torch.zeros(1, dtype=torch.int32, device=dev)
            else:
                off, items = exclude_csr(exclude, torch.arange(n, device=dev) if ids64 is None else ids64, n, m, dev)
        nbytes = L.mfcd_topk_rows_workspace_bytes(nrows, m, d, k, e)
        if nbytes == 0:
            raise _lib.MfcdError(f"topk_rows: sizes out of range (rows {nrows}, m {m}, d {d}, k {k})")
        ws = _lib.workspace(nbytes, dev)
        _lib.check(L.mfcd_topk_rows(Xd.data_ptr() if Xd is not None else None, Xd.stride(0) if Xd is not None else 0,
                                    _lib.ptr(A), _lib.ptr(B), d,
                                    _lib.ptr(ids), nrows, n, m, k, e, _lib.ptr(off), _lib.ptr(items), _lib.ptr(bi),
                                    _lib.ptr(bv), _lib.ptr(wi), _lib.ptr(wv), _lib.ptr(ws), ws.numel(),
                                    _lib.stream_ptr(dev)))
    best, worst = ((bi, bv) if values else bi), ((wi, wv) if values else wi)
    return (best, worst) if e == 3 else best if e == 1 else worst
