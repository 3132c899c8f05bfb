"""Exact all-pairs statistics of score rows against ground-truth rows on the device (include/mfcd.h:
mfcd_pair_stats_rows): the Kendall counts C, D, Ta, Tx as exact integers and the sums of the BTL population risk, its
Bayes floor, the expected accuracy and its Bayes ceiling over the m (m - 1) / 2 item pairs of every row.

`pair_stats_rows` is the kernel call; `pairwise_from_counts` turns its outputs into per-row values on the host (f64);
`pairwise_metrics` forms the score rows of a model block by block and is what structure.compute_pairwise_metrics
returns.  There is no CPU form.
"""
import numpy as np
import torch

from . import _lib

TILE = 1024          # columns per workgroup tile of the kernel (csrc/pairs.hip: kPairTile)
_WHAT = {"counts": 1, "sums": 2, "both": 3}
_ws = {}


def _workspace(nbytes, device):
    buf = _ws.get(device)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws[device] = buf
    return buf


def pair_stats_rows(A, X, scale=1.0, what="both"):
    """Two [rows, m] fp32 GPU matrices (rows may be strided views): scores A, ground truth X →
    (counts int64 [rows, 4] = C, D, Ta, Tx or None, sums f64 [rows, 4] = risk, bayes_risk, exp_acc, bayes_acc or None),
    on the device.  what: "counts", "sums" or "both".  A row with a NaN has counts -1; a row with a non-finite entry has
    NaN sums.  Deterministic: two calls are bit-equal."""
    if what not in _WHAT:
        raise ValueError(f"what must be one of {sorted(_WHAT)}, got {what!r}")
    w = _WHAT[what]
    if not torch.is_tensor(A) or not torch.is_tensor(X) or A.dim() != 2 or X.shape != A.shape \
            or A.dtype != torch.float32 or X.dtype != torch.float32 or not A.is_cuda or not X.is_cuda:
        raise _lib.MfcdError("pair_stats_rows needs two float32 GPU matrices of the same shape (no CPU fallback)")
    L = _lib.load()
    rows, m = A.shape
    if A.stride(1) != 1 or X.stride(1) != 1:
        A, X = A.contiguous(), X.contiguous()
    counts = torch.empty((rows, 4), dtype=torch.int64, device=A.device) if w & 1 else None
    sums = torch.empty((rows, 4), dtype=torch.float64, device=A.device) if w & 2 else None
    if rows == 0:
        return counts, sums
    need = L.mfcd_pair_stats_workspace_bytes(rows, m)
    if need == 0:
        raise _lib.MfcdError(f"rows of {m} columns are outside the pair kernel's range [1, 1048576]")
    ws = _workspace(need, A.device)
    _lib.check(L.mfcd_pair_stats_rows(A.data_ptr(), A.stride(0) if rows > 1 else m, X.data_ptr(),
                                      X.stride(0) if rows > 1 else m, rows, m, float(scale), w, _lib.ptr(counts),
                                      _lib.ptr(sums), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(A.device)))
    return counts, sums


def _host(t):
    return None if t is None else t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def pairwise_from_counts(counts, sums, m):
    """Per-row values (float64 numpy arrays, NaN where undefined) from the outputs of `pair_stats_rows`; either of
    `counts` / `sums` may be None, and its keys are then absent.  With n0 = m (m - 1) / 2:
      kendall_tau        (C - D) / sqrt((n0 - Ta)(n0 - Tx)): tau-b; NaN when a factor is 0 (a constant row, m < 2) or the
                         row held a NaN
      pairwise_accuracy  C / (n0 - Tx): the share of the pairs X orders that the scores order the same way
      risk, bayes_risk, expected_accuracy, bayes_accuracy    sums / n0"""
    n0 = m * (m - 1) // 2
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        if counts is not None:
            c = _host(counts).astype(np.int64).reshape(-1, 4)
            C, D, Ta, Tx = (c[:, k].astype(np.float64) for k in range(4))     # exact: every count is below 2^53
            da, dx = (n0 - c[:, 2]).astype(np.float64), (n0 - c[:, 3]).astype(np.float64)
            ok = (c[:, 0] >= 0) & (da > 0) & (dx > 0)
            tau = (C - D) / (np.sqrt(da) * np.sqrt(dx))
            out["kendall_tau"] = np.where(ok, tau, np.nan)
            out["pairwise_accuracy"] = np.where((c[:, 0] >= 0) & (dx > 0), C / dx, np.nan)
        if sums is not None:
            s = _host(sums).astype(np.float64).reshape(-1, 4)
            for k, name in enumerate(("risk", "bayes_risk", "expected_accuracy", "bayes_accuracy")):
                out[name] = s[:, k] / n0 if n0 > 0 else np.full(s.shape[0], np.nan)
    return out


_KEYS = ("kendall_tau", "pairwise_accuracy", "expected_log_likelihood", "bayes_log_likelihood", "expected_accuracy",
         "bayes_accuracy")


def pairwise_metrics(U, V, X, s=1.0, users=None, row_block=2048):
    """structure.compute_pairwise_metrics on factor tables: score rows U[r0:r1] @ V^T (and A[r0:r1] @ B^T for a
    factored X) are formed `row_block` at a time by a plain library GEMM and go through `pair_stats_rows`."""
    if not torch.is_tensor(U) or not U.is_cuda:
        raise _lib.MfcdError("pairwise metrics need the model on a GPU (there is no CPU fallback)")
    dev = U.device
    U, V = U.detach().float(), V.detach().float()
    n, m = U.shape[0], V.shape[0]
    if tuple(X.shape) != (n, m):
        raise ValueError(f"X must be [{n},{m}], got {tuple(X.shape)}")
    factored = _lib.is_factored(X)
    if factored:
        XA, XB = X.A.to(dev), X.B.to(dev)
    else:
        if not torch.is_tensor(X):
            raise TypeError("X must be a dense GPU tensor or a FactoredMatrix")
        X = X.to(dev).float()
    if users is None:
        ids = torch.arange(n, device=dev)
    else:
        ids = torch.as_tensor(users).reshape(-1).to(device=dev, dtype=torch.int64)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise IndexError(f"user number out of range for a model of {n} users")
    k = ids.numel()
    row_block = max(1, int(row_block))
    counts = torch.empty((k, 4), dtype=torch.int64, device=dev)
    sums = torch.empty((k, 4), dtype=torch.float64, device=dev)
    Vt = V.t()
    for r0 in range(0, k, row_block):
        sel = ids[r0:r0 + row_block]
        whole = users is None
        scores = (U[r0:r0 + row_block] if whole else U[sel]) @ Vt
        if factored:
            truth = (XA[r0:r0 + row_block] if whole else XA[sel]) @ XB.t()
        else:
            truth = X[r0:r0 + row_block] if whole else X[sel]
        counts[r0:r0 + row_block], sums[r0:r0 + row_block] = pair_stats_rows(scores, truth, s, "both")
    per = pairwise_from_counts(counts, sums, m)
    per["expected_log_likelihood"] = -per.pop("risk")          # the sign of the result dict's log_likelihoods
    per["bayes_log_likelihood"] = -per.pop("bayes_risk")
    out = {}
    for name in _KEYS:
        v = per[name]
        good = v[~np.isnan(v)]
        out[name] = float(good.mean()) if good.size else 0.0
        out[name + "_per_user"] = v
    return out
