"""Exact all-pairs statistics of score rows against ground-truth rows on the device (include/mfcd.h:
mfcd_pair_stats_rows): the Kendall counts C, D, Ta, Tx as exact integers and the sums of the BTL population risk, its
Bayes floor, the expected accuracy and its Bayes ceiling over the m (m - 1) / 2 item pairs of every row.

`pair_stats_rows` is the kernel call; `pairwise_from_counts` turns its outputs into per-row values on the host (f64);
`pairwise_metrics` forms the score rows of a model block by block and is what structure.compute_pairwise_metrics
returns.

The risk can also be minimised: `pair_grad_rows` (mfcd_pair_grad_rows) is its gradient with respect to the score rows,
`population_risk` the mean risk as a differentiable scalar of the factor tables, `fit_population` the fused loop of
risk gradient and Adam step.  There is no CPU form of any of it.
"""
import numpy as np
import torch

from . import _lib
from .rows import RowBlocks

TILE = 1024          # columns per workgroup tile of the kernel (csrc/pairs.hip: kPairTile)
_WHAT = {"counts": 1, "sums": 2, "both": 3}


def pair_stats_rows(A, X, scale=1.0, what="both"):
    """Two [rows, m] fp32 GPU matrices (rows may be strided views): scores A, ground truth X →
    (counts int64 [rows, 4] = C, D, Ta, Tx or None, sums f64 [rows, 4] = risk, bayes_risk, exp_acc, bayes_acc or None),
    on the device.  what: "counts", "sums" or "both".  A row with a NaN has counts -1; a row with a non-finite entry has
    NaN sums.  Deterministic: two calls are bit-equal."""
    if what not in _WHAT:
        raise ValueError(f"what must be one of {sorted(_WHAT)}, got {what!r}")
    w = _WHAT[what]
    A, X, rows, m, lda, ldx = _lib.row_pair(A, X, "pair_stats_rows")
    L = _lib.load()
    counts = torch.empty((rows, 4), dtype=torch.int64, device=A.device) if w & 1 else None
    sums = torch.empty((rows, 4), dtype=torch.float64, device=A.device) if w & 2 else None
    if rows == 0:
        return counts, sums
    need = L.mfcd_pair_stats_workspace_bytes(rows, m)
    if need == 0:
        raise _lib.MfcdError(f"rows of {m} columns are outside the pair kernel's range [1, 1048576]")
    ws = _lib.workspace(need, A.device)
    _lib.check(L.mfcd_pair_stats_rows(A.data_ptr(), lda, X.data_ptr(), ldx, rows, m, float(scale), w, _lib.ptr(counts),
                                      _lib.ptr(sums), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(A.device)))
    return counts, sums


def pair_grad_rows(A, X, scale=1.0):
    """Two [rows, m] fp32 GPU matrices (rows may be strided views): scores A, ground truth X → G fp32 [rows, m] on the
    device, g_i = sum over j != i of sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j)): the gradient of the `risk` sum of
    `pair_stats_rows` with respect to the scores.  A row with a non-finite entry is all NaN.  Deterministic."""
    A, X, rows, m, lda, ldx = _lib.row_pair(A, X, "pair_grad_rows")
    L = _lib.load()
    G = torch.empty((rows, m), dtype=torch.float32, device=A.device)
    if rows == 0:
        return G
    if not 1 <= m <= 1 << 20:
        raise _lib.MfcdError(f"rows of {m} columns are outside the pair kernel's range [1, 1048576]")
    _lib.check(L.mfcd_pair_grad_rows(A.data_ptr(), lda, X.data_ptr(), ldx, rows, m, float(scale), G.data_ptr(), m,
                                     _lib.stream_ptr(A.device)))
    return G


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
    src = RowBlocks(U.detach(), V.detach(), X, users, row_block, "pairwise metrics")
    m = src.m
    counts = torch.empty((src.k, 4), dtype=torch.int64, device=src.dev)
    sums = torch.empty((src.k, 4), dtype=torch.float64, device=src.dev)
    for r0, r1 in src.blocks():
        counts[r0:r1], sums[r0:r1] = pair_stats_rows(src.scores(r0, r1), src.truth(r0, r1), s, "both")
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


class _PopulationRisk(torch.autograd.Function):
    """mean over the users of a RowBlocks and over the n0 pairs of the BTL risk, as a function of the factor tables.
    Backward recomputes a block's scores instead of keeping n x m of them, takes dRisk/dscores from `pair_grad_rows`
    and carries it to the tables with two library GEMMs per block, accumulating in block order."""

    @staticmethod
    def forward(ctx, U, V, src, s):
        total = torch.zeros((), dtype=torch.float64, device=src.dev)
        for r0, r1 in src.blocks():
            total += pair_stats_rows(src.scores(r0, r1), src.truth(r0, r1), s, "sums")[1][:, 0].sum()
        ctx.src, ctx.s = src, s
        return (total / (src.k * (src.m * (src.m - 1) // 2))).float()

    @staticmethod
    def backward(ctx, grad_out):
        src = ctx.src
        coef = grad_out.float() / (src.k * (src.m * (src.m - 1) // 2))
        dU_rows = torch.empty((src.k, src.U.shape[1]), dtype=torch.float32, device=src.dev)
        dV = torch.zeros_like(src.V)
        for r0, r1 in src.blocks():
            G = pair_grad_rows(src.scores(r0, r1), src.truth(r0, r1), ctx.s).mul_(coef)
            torch.mm(G, src.V, out=dU_rows[r0:r1])
            dV.addmm_(G.t(), src.rows_of(src.U, r0, r1))
        if src.whole:
            dU = dU_rows
        else:       # a user named twice counts twice; accumulate=True adds in the order of `users`
            dU = torch.zeros_like(src.U).index_put_((src.ids,), dU_rows, accumulate=True)
        return dU, dV, None, None


def population_risk(U, V, X, s=1.0, users=None, row_block=2048):
    """The exact BTL population risk of the model U V^T against the label law q = sigmoid(s (x_i - x_j)): the mean, over
    the chosen users (None: every user; a user named twice counts twice) and over all m (m - 1) / 2 item pairs, of
    q (-log p) + (1 - q)(-log(1 - p)) with p = sigmoid(a_i - a_j) → 0-dim fp32 device tensor, differentiable with respect
    to fp32 `U` and `V`.  X: a dense GPU tensor or a FactoredMatrix.  Rows are formed `row_block` users at a time."""
    if torch.is_tensor(U) and U.is_cuda and (U.dtype != torch.float32 or V.dtype != torch.float32):
        raise _lib.MfcdError("the population risk takes float32 factor tables")
    src = RowBlocks(U.detach(), V.detach(), X, users, row_block, "the population risk")
    if src.m < 2:
        raise ValueError("the population risk needs at least two items (m >= 2)")
    if src.k == 0:
        raise ValueError("the population risk needs at least one user")
    return _PopulationRisk.apply(U, V, src, float(s))


def fit_population(binding, X, s, steps, log_every=0, row_block=2048):
    """`steps` steps of Adam on the exact population risk of every user (see `population_risk`), fused: per step the
    score blocks, `pair_grad_rows` and two library GEMMs per block into dense gradients, then one mfcd_adam_dense —
    coupled-L2 Adam on the caller's torch.optim.Adam state, which stays valid (binding: an engine.AdamBinding, or a
    (model, optimizer) pair one is made from; fp32 tables only).  Nothing waits for the device inside the loop.
    log_every = k > 0: the risk after 0, k, 2k, ... steps (taken before the next step, from the same score blocks) and
    after the last step is written to a device buffer and read once at the end → (steps taken, risks) as Python lists;
    log_every = 0 → ([], [])."""
    from . import engine
    if not isinstance(binding, engine.AdamBinding):
        binding = engine.AdamBinding(*binding)
    for name, t in zip(("model.U", "model.V"), binding.tensors()[:2]):
        engine._require_cuda_param(t, name)                    # fp32 only: bf16 tables are refused here
    L = _lib.load()
    U, V, mU, vU, mV, vV = binding.tensors()
    src = RowBlocks(U, V, X, None, row_block, "the population fit")
    n, m, d, dev = src.n, src.m, U.shape[1], src.dev
    if m < 2:
        raise ValueError("the population risk needs at least two items (m >= 2)")
    steps, k = int(steps), int(log_every)
    n0 = m * (m - 1) // 2
    inv = 1.0 / (n * n0)
    at = ([t for t in range(0, steps, k)] + [steps]) if k > 0 else []
    log = torch.zeros(max(len(at), 1), dtype=torch.float64, device=dev)
    gU, gV = torch.empty_like(U), torch.empty_like(V)
    ptrs = [_lib.ptr(t) for t in (U, V, mU, vU, mV, vV, gU, gV)]
    lr, b1, b2, eps, wd = binding.hyper()
    stream = _lib.stream_ptr(dev)
    blocks = src.blocks()

    def risk_into(slot, scores, truth):
        slot += pair_stats_rows(scores, truth, s, "sums")[1][:, 0].sum()

    try:
        for t in range(steps):
            logging = k > 0 and t % k == 0
            for b, (r0, r1) in enumerate(blocks):
                scores, truth = src.scores(r0, r1), src.truth(r0, r1)
                if logging:
                    risk_into(log[t // k], scores, truth)
                G = pair_grad_rows(scores, truth, s).mul_(inv)
                torch.mm(G, V, out=gU[r0:r1])
                if b == 0:
                    torch.mm(G.t(), U[r0:r1], out=gV)
                else:
                    gV.addmm_(G.t(), U[r0:r1])
            _lib.check(L.mfcd_adam_dense(*ptrs, binding.step + 1, n, m, d, lr, b1, b2, eps, wd, stream))
            binding.advance(1, defer=True)
    finally:
        binding.flush()         # an interrupt must not leave the moments ahead of the optimizer's `step` tensors
    if k <= 0:
        return [], []
    for r0, r1 in blocks:
        risk_into(log[len(at) - 1], src.scores(r0, r1), src.truth(r0, r1))
    return at, (log[:len(at)] * inv).cpu().tolist()       # the one device->host transfer of the run
