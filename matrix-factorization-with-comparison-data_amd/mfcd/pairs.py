"""Exact all-pairs statistics of score rows against ground-truth rows on the device (include/mfcd.h:
mfcd_pair_stats_rows): the Kendall counts C, D, Ta, Tx as exact integers and the sums of the BTL population risk, its
Bayes floor, the expected accuracy and its Bayes ceiling over the m (m - 1) / 2 item pairs of every row.

`pair_stats_rows` is the kernel call; `pairwise_from_counts` turns its outputs into per-row values on the host (f64);
`pairwise_metrics` forms the score rows of a model block by block and is what structure.compute_pairwise_metrics
returns.

The risk can also be minimised: `pair_grad_rows` (mfcd_pair_grad_rows) is its gradient with respect to the score rows,
`population_risk` the mean risk as a differentiable scalar of the factor tables, `fit_population` the fused loop of
risk gradient and Adam step.  There is no CPU form of any of it.

All of it also exists under a pair law (`PairLaw`; `strategy_law` builds the one a sampling strategy draws its attempts
from): `pair_law_stats_rows` / `pair_law_grad_rows` are the weighted kernel calls, and `law_risk`, `law_metrics` and
`fit_law` are `population_risk`, `pairwise_metrics` and `fit_population` under it.  The law's risk is normalised
globally, by the weight of all users.

Second order: `pair_hvp_rows` / `pair_law_hvp_rows` (mfcd_pair_hvp_rows, mfcd_pair_law_hvp_rows) apply the Hessian of a
row's risk sum, a weighted graph Laplacian, to a vector, and `population_hvp` carries it to the factor tables: the
Hessian-vector product of `population_risk` / `law_risk`.  mfcd/population.py builds the exact block steps on it.

`pair_hvp_multi_rows` (mfcd_pair_hvp_multi_rows) applies the same Laplacian to all d columns of an item table in one
pass, `pair_info_rows` contracts the result to the d x d matrix H_r = B_r^T L(a_r) B_r the Laplacian induces on a user's
row, and `user_information` forms it for the users of a model: the Hessian of a user's risk sum in u (at="model") or the
Fisher information of the law's comparisons about the row (at="truth").

`pair_best_rows` (mfcd_pair_best_rows) finds, per column, the admissible partner with the largest
sigmoid'(a_i - a_j) |g_i - g_j|^2 on a table the caller centres: the arg-max mfcd/design.py builds the D-optimal
comparison design of a user on.
"""
import collections
import copy
import ctypes

import numpy as np
import torch

from . import _lib
from .rows import RowBlocks

TILE = 1024          # columns per workgroup tile of the kernel (csrc/pairs.hip: kPairTile)
INFO_TILE = 128     # columns per workgroup tile of the multi-column kernel (csrc/pair_info.hip: kInfoTile)
INFO_MAX_D = 256    # its widest item table (kInfoMaxD)
BEST_TILE = 128     # columns per workgroup tile of the arg-max kernel (csrc/pair_best.hip: kBestTile)
BEST_MAX_D = 256    # its widest table (kBestMaxD)
_INFO_Z_BYTES = 256 << 20   # `pair_info_rows` takes rows in chunks whose Z stays under this
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


class PairLaw:
    """A weight on the item pairs of every user: the law a population risk is taken under.  For a user whose truth row,
    restricted to the law's columns, is x, the unordered pair {i, j} of those columns weighs
        w_ij = (alpha_i beta_j + alpha_j beta_i, or 1)  *  [|x_i - x_j| <= margin]  *  [label_i != label_j],
    each factor present only if given (include/mfcd.h: mfcd_pair_law).
      alpha, beta   [k] non-negative finite weights, both or neither.  Each vector is scaled so that its largest entry is
                    1 (the risk does not change) and positive entries below 1e-6 of the largest are set to 0, so that
                    every product is a normal fp32 number.
      labels        int [k] shared by all users, or [n, k], one row per user of the model
      margin        a non-negative float, compared with the fp32 difference of the raw (unscaled) x
      columns       the item numbers the law lives on: [k] shared, or [n, k] per user; None: all m items in order
      users         the users the law is over (None: every user)
    Validated once, here (ValueError); the tensors stay on `device` (None: where they are) as long as the law lives."""

    def __init__(self, alpha=None, beta=None, labels=None, margin=None, columns=None, users=None, device=None):
        if (alpha is None) != (beta is None):
            raise ValueError("a pair law takes alpha and beta together or neither")
        k = None
        if columns is not None:
            columns = torch.as_tensor(columns)
            if columns.dim() not in (1, 2) or columns.dtype.is_floating_point or columns.shape[-1] < 1:
                raise ValueError(f"columns must be item numbers [k] or [n, k], got {tuple(columns.shape)}")
            if int(columns.min()) < 0:
                raise ValueError("a column number is negative")
            columns = columns.to(torch.int64)
            k = columns.shape[-1]
            self.max_column = int(columns.max())
        if alpha is not None:
            vs = []
            for name, v in (("alpha", alpha), ("beta", beta)):
                v = torch.as_tensor(v).detach().double().reshape(-1).cpu()
                if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
                    raise ValueError(f"{name} must be finite and non-negative")
                if k is not None and v.numel() != k:
                    raise ValueError(f"{name} has {v.numel()} entries for {k} columns")
                k = v.numel()
                top = float(v.max()) if k else 0.0
                if top > 0:
                    v = v / top
                    v = torch.where(v < 1e-6, torch.zeros_like(v), v)
                vs.append(v.float().contiguous())
            alpha, beta = vs
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.dim() not in (1, 2) or labels.dtype.is_floating_point or (k is not None and labels.shape[-1] != k):
                raise ValueError(f"labels must be integers [k] or [n, k] with k = {k}, got {tuple(labels.shape)}")
            if labels.dim() == 2 and columns is not None and columns.dim() == 2 and labels.shape[0] != columns.shape[0]:
                raise ValueError(f"{labels.shape[0]} label rows for {columns.shape[0]} column rows")
            labels = labels.to(torch.int32).contiguous()
        if margin is not None:
            margin = float(margin)
            if not margin >= 0.0:
                raise ValueError(f"the margin must be a non-negative number, got {margin}")
        if users is not None:
            users = torch.as_tensor(users).reshape(-1).to(torch.int64)
        dev = None if device is None else torch.device(device)
        put = (lambda t: t) if dev is None else (lambda t: t.to(dev))
        self.alpha, self.beta = (None, None) if alpha is None else (put(alpha), put(beta))
        self.labels = None if labels is None else put(labels)
        self.columns = None if columns is None else put(columns)
        self.users = None if users is None else put(users)
        self.margin = margin
        if dev is None and alpha is not None:           # follow the other tensors, if any is on a device
            for t in (self.labels, self.columns, self.users):
                if t is not None and t.is_cuda:
                    self.alpha, self.beta = self.alpha.to(t.device), self.beta.to(t.device)
                    break
        self.k = k if k is not None else (None if labels is None else labels.shape[-1])

    @property
    def trivial(self):
        """Every pair of every user with weight 1: the unweighted kernels' law."""
        return all(t is None for t in (self.alpha, self.labels, self.margin, self.columns, self.users))

    def per_user(self):
        return (self.labels is not None and self.labels.dim() == 2) or (self.columns is not None and self.columns.dim() == 2)

    def for_rows(self, ids):
        """The law of the rows of users `ids` (an index tensor): per-user labels and columns restricted to them."""
        law = copy.copy(self)
        if self.labels is not None and self.labels.dim() == 2:
            law.labels = self.labels[ids].contiguous()
        if self.columns is not None and self.columns.dim() == 2:
            law.columns = self.columns[ids]
        return law

    def take(self, rows):
        """A block [b, m] restricted to the law's columns → [b, k]."""
        if self.columns is None:
            return rows
        return rows[:, self.columns] if self.columns.dim() == 1 else torch.gather(rows, 1, self.columns)

    def put_back(self, Gk, m):
        """The transpose of `take`: [b, k] → [b, m], adding where a column is named twice (at most two addends per
        destination for a law of `strategy_law`, so the sum does not depend on their order)."""
        if self.columns is None:
            return Gk
        cols = self.columns if self.columns.dim() == 2 else self.columns.expand(Gk.shape[0], -1)
        return torch.zeros((Gk.shape[0], m), dtype=Gk.dtype, device=Gk.device).scatter_add_(1, cols, Gk)

    def _c(self, rows, m):
        """The filled mfcd_pair_law of a call on `rows` rows of `m` columns."""
        c = _lib.PairLawC()
        for t in (self.alpha, self.beta):
            if t is not None and t.numel() != m:
                raise ValueError(f"the law has {t.numel()} weights for rows of {m} columns")
        if self.labels is not None:
            lab = self.labels
            if lab.shape[-1] != m or (lab.dim() == 2 and lab.shape[0] != rows):
                raise ValueError(f"labels {tuple(lab.shape)} do not fit {rows} rows of {m} columns")
            c.labels, c.label_stride = _lib.ptr(lab), (m if lab.dim() == 2 else 0)
        c.alpha, c.beta = _lib.ptr(self.alpha), _lib.ptr(self.beta)
        c.use_margin, c.margin = (0, 0.0) if self.margin is None else (1, self.margin)
        return c


def pair_law_stats_rows(A, X, law, scale=1.0):
    """`pair_stats_rows`' sums under a `PairLaw`, for rows already restricted to the law's columns (include/mfcd.h:
    mfcd_pair_law_stats_rows) → (support int64 [rows]: the pairs i < j with w > 0, exact; sums f64 [rows, 5] = W, risk,
    bayes_risk, exp_acc, bayes_acc, each the sum of w * term), on the device.  A row without weight has sums of exactly
    +0, a row with a non-finite entry NaN sums.  Deterministic: two calls are bit-equal."""
    A, X, rows, m, lda, ldx = _lib.row_pair(A, X, "pair_law_stats_rows")
    L = _lib.load()
    c = law._c(rows, m)
    support = torch.empty(rows, dtype=torch.int64, device=A.device)
    sums = torch.empty((rows, 5), dtype=torch.float64, device=A.device)
    if rows == 0:
        return support, sums
    need = L.mfcd_pair_law_stats_workspace_bytes(rows, m)
    if need == 0:
        raise _lib.MfcdError(f"rows of {m} columns are outside the pair kernel's range [1, 1048576]")
    ws = _lib.workspace(need, A.device)
    _lib.check(L.mfcd_pair_law_stats_rows(A.data_ptr(), lda, X.data_ptr(), ldx, rows, m, float(scale), ctypes.byref(c),
                                          _lib.ptr(support), _lib.ptr(sums), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr(A.device)))
    return support, sums


def pair_law_grad_rows(A, X, law, scale=1.0):
    """`pair_grad_rows` under a `PairLaw`, for rows already restricted to the law's columns (mfcd_pair_law_grad_rows) →
    G fp32 [rows, m], g_i = sum over j != i of w_ij (sigmoid(a_i - a_j) - sigmoid(scale (x_i - x_j))): the gradient of
    the `risk` sum of `pair_law_stats_rows`.  Exactly +0 where no pair of i has weight; a row with a non-finite entry is
    all NaN.  Deterministic."""
    A, X, rows, m, lda, ldx = _lib.row_pair(A, X, "pair_law_grad_rows")
    L = _lib.load()
    c = law._c(rows, m)
    G = torch.empty((rows, m), dtype=torch.float32, device=A.device)
    if rows == 0:
        return G
    if not 1 <= m <= 1 << 20:
        raise _lib.MfcdError(f"rows of {m} columns are outside the pair kernel's range [1, 1048576]")
    _lib.check(L.mfcd_pair_law_grad_rows(A.data_ptr(), lda, X.data_ptr(), ldx, rows, m, float(scale), ctypes.byref(c),
                                         G.data_ptr(), m, _lib.stream_ptr(A.device)))
    return G


def _range_check(m):
    if not 1 <= m <= 1 << 20:
        raise _lib.MfcdError(f"rows of {m} columns are outside the pair kernel's range [1, 1048576]")


def pair_hvp_rows(A, Y, deg=False):
    """Two [rows, m] fp32 GPU matrices (rows may be strided views): scores A, directions Y → Q fp32 [rows, m] on the
    device, q_i = sum over j != i of s_ij (y_i - y_j) with s_ij = sigmoid'(a_i - a_j): the Hessian of the `risk` sum of
    `pair_stats_rows` with respect to the scores (a graph Laplacian; it depends on neither X nor the scale), applied to
    the row of Y.  deg=True → (Q, deg), deg_i = sum over j != i of s_ij, the Hessian's diagonal.  A constant row of Y
    gives exactly +0; a row with a non-finite entry is all NaN.  Deterministic, and Q does not depend on `deg`."""
    A, Y, rows, m, lda, ldy = _lib.row_pair(A, Y, "pair_hvp_rows")
    L = _lib.load()
    Q = torch.empty((rows, m), dtype=torch.float32, device=A.device)
    D = torch.empty((rows, m), dtype=torch.float32, device=A.device) if deg else None
    if rows:
        _range_check(m)
        _lib.check(L.mfcd_pair_hvp_rows(A.data_ptr(), lda, Y.data_ptr(), ldy, rows, m, Q.data_ptr(), m, _lib.ptr(D), m,
                                        _lib.stream_ptr(A.device)))
    return (Q, D) if deg else Q


def pair_law_hvp_rows(A, X, Y, law, deg=False):
    """`pair_hvp_rows` under a `PairLaw`, for rows already restricted to the law's columns (mfcd_pair_law_hvp_rows):
    q_i = sum over j != i of w_ij s_ij (y_i - y_j), deg_i = sum over j != i of w_ij s_ij, the Hessian of the `risk` sum
    of `pair_law_stats_rows` and its diagonal.  X enters through the law's margin only.  Exactly +0 where no pair of i
    has weight; a row with a non-finite entry in A, X or Y is all NaN.  Deterministic."""
    A, X, rows, m, lda, ldx = _lib.row_pair(A, X, "pair_law_hvp_rows")
    A, Y, _, _, lda, ldy = _lib.row_pair(A, Y, "pair_law_hvp_rows")
    L = _lib.load()
    c = law._c(rows, m)
    Q = torch.empty((rows, m), dtype=torch.float32, device=A.device)
    D = torch.empty((rows, m), dtype=torch.float32, device=A.device) if deg else None
    if rows:
        _range_check(m)
        _lib.check(L.mfcd_pair_law_hvp_rows(A.data_ptr(), lda, X.data_ptr(), ldx, Y.data_ptr(), ldy, rows, m,
                                            ctypes.byref(c), Q.data_ptr(), m, _lib.ptr(D), m, _lib.stream_ptr(A.device)))
    return (Q, D) if deg else Q


def pair_hvp_multi_rows(A, B, X=None, law=None, index=None, deg=False):
    """`pair_law_hvp_rows` for every column of an item table at once (mfcd_pair_hvp_multi_rows): scores A [rows, k] and
    an item table B [mB, d] (fp32, on the GPU, d <= 256) → Z fp32 [rows, k, d],
        z_i = sum over j != i of w_ij s_ij (b_i - b_j),   s_ij = sigmoid'(a_i - a_j),
    with b_j = B[index[j]] (index: int [k] shared by all rows, or [rows, k]; None: column j is row j of B and k = mB) and
    w the weight of `law` on rows already restricted to its columns (None: the plain risk, w = 1).  X [rows, k] enters
    through the law's margin and the finiteness rule only; it may be None unless the law has a margin.  deg=True →
    (Z, deg), deg_i = sum over j != i of w_ij s_ij, fp32 [rows, k].  The kernel centres the gathered table (f64 column
    mean) before it forms the Laplacian's difference.  Exactly +0 where no pair of i has weight; a row with a non-finite
    entry in A, X or a row of B it uses, or with an index outside [0, mB), is all NaN.  Deterministic, a row does not
    depend on its neighbours, and Z does not depend on `deg`."""
    who = "pair_hvp_multi_rows"
    if X is None:
        A, _, rows, k, lda, _ = _lib.row_pair(A, A, who)
        ldx = 0
    else:
        A, X, rows, k, lda, ldx = _lib.row_pair(A, X, who)
    if not torch.is_tensor(B) or B.dim() != 2 or B.dtype != torch.float32 or not B.is_cuda:
        raise _lib.MfcdError(f"{who} needs the item table as a float32 GPU matrix (no CPU fallback)")
    if B.stride(1) != 1:
        B = B.contiguous()
    mB, d = B.shape
    ldb = B.stride(0) if mB > 1 else d
    stride = 0
    if index is not None:
        index = torch.as_tensor(index)
        if index.dtype.is_floating_point or index.dim() not in (1, 2) or index.shape[-1] != k \
                or (index.dim() == 2 and index.shape[0] != rows):
            raise ValueError(f"index must be integers [{k}] or [{rows}, {k}], got {tuple(index.shape)}")
        stride = k if index.dim() == 2 else 0
        index = index.to(device=A.device, dtype=torch.int32).contiguous()
    elif k != mB:
        raise ValueError(f"without an index the rows need one column per row of B: {k} columns, {mB} rows")
    c = None if law is None else law._c(rows, k)
    if law is not None and law.margin is not None and X is None:
        raise ValueError("a law with a margin needs X")
    L = _lib.load()
    Z = torch.empty((rows, k, d), dtype=torch.float32, device=A.device)
    D = torch.empty((rows, k), dtype=torch.float32, device=A.device) if deg else None
    if rows:
        _range_check(k)
        if not 1 <= d <= INFO_MAX_D:
            raise _lib.MfcdError(f"an item table of {d} columns is outside the kernel's range [1, {INFO_MAX_D}]")
        ws = _lib.workspace(L.mfcd_pair_hvp_multi_workspace_bytes(rows, k, d), A.device)
        _lib.check(L.mfcd_pair_hvp_multi_rows(A.data_ptr(), lda, None if X is None else X.data_ptr(), ldx, B.data_ptr(), ldb,
                                              mB, d, _lib.ptr(index), stride, rows, k,
                                              None if c is None else ctypes.byref(c), Z.data_ptr(), d, _lib.ptr(D), k,
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr(A.device)))
    return (Z, D) if deg else Z


def pair_best_rows(A, G, X=None, law=None):
    """Per column the most informative admissible partner (mfcd_pair_best_rows): scores A [rows, k] and a table G, fp32
    on the GPU, [rows, k, d] (one table per row) or [k, d] (one for all rows), d <= 256 →
    (val fp32 [rows, k], j int32 [rows, k]),
        val_i = max over admissible j != i of s_ij |g_i - g_j|^2,   s_ij = sigmoid'(a_i - a_j),
    and j_i the smallest j that attains it.  A pair is admissible when the weight of `law` (on rows already restricted
    to its columns; None: every pair) is > 0; the weight's size does not enter.  X [rows, k] enters through the law's
    margin and the finiteness rule only; it may be None unless the law has a margin.  The kernel forms |g_i - g_j|^2
    from squared norms and fp32 matrix products: the caller centres the table.  A column without an admissible partner
    has (+0, -1); a row with a non-finite entry in A, X or its table is all (NaN, -1).  Deterministic, and a row does
    not depend on its neighbours."""
    who = "pair_best_rows"
    if X is None:
        A, _, rows, k, lda, _ = _lib.row_pair(A, A, who)
        ldx = 0
    else:
        A, X, rows, k, lda, ldx = _lib.row_pair(A, X, who)
    if not torch.is_tensor(G) or G.dtype != torch.float32 or not G.is_cuda or G.dim() not in (2, 3):
        raise _lib.MfcdError(f"{who} needs the table as a float32 GPU tensor [k, d] or [rows, k, d] (no CPU fallback)")
    if G.shape[-2] != k or (G.dim() == 3 and G.shape[0] != rows):
        raise ValueError(f"the table must be [{k}, d] or [{rows}, {k}, d], got {tuple(G.shape)}")
    G = G.contiguous()
    d = G.shape[-1]
    c = None if law is None else law._c(rows, k)
    if law is not None and law.margin is not None and X is None:
        raise ValueError("a law with a margin needs X")
    L = _lib.load()
    val = torch.empty((rows, k), dtype=torch.float32, device=A.device)
    arg = torch.empty((rows, k), dtype=torch.int32, device=A.device)
    if rows:
        _range_check(k)
        if not 1 <= d <= BEST_MAX_D:
            raise _lib.MfcdError(f"a table of {d} columns is outside the kernel's range [1, {BEST_MAX_D}]")
        ws = _lib.workspace(L.mfcd_pair_best_workspace_bytes(rows, k, d), A.device)
        _lib.check(L.mfcd_pair_best_rows(A.data_ptr(), lda, None if X is None else X.data_ptr(), ldx, G.data_ptr(),
                                         k * d if G.dim() == 3 else 0, d, d, rows, k,
                                         None if c is None else ctypes.byref(c), val.data_ptr(), k, arg.data_ptr(), k,
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr(A.device)))
    return val, arg


def pair_info_rows(A, B, X=None, law=None, index=None):
    """The d x d matrix a row's Laplacian induces on the item vectors, H_r = B~_r^T L(a_r) B~_r = sum over i < j of
    w_ij s_ij (b_i - b_j)(b_i - b_j)^T → f64 [rows, d, d] on the device; the arguments are `pair_hvp_multi_rows`'.
    H_r = B~_r^T Z_r with B~ the gathered table minus its f64 column mean, contracted in f64 by a batched library GEMM,
    rows taken in chunks so that a chunk's Z stays under 256 MiB; symmetrised, so H[p][q] and H[q][p] are bit-equal.  A
    NaN row of Z gives a NaN matrix."""
    if not torch.is_tensor(A) or A.dim() != 2 or not torch.is_tensor(B) or B.dim() != 2 or not A.is_cuda or not B.is_cuda:
        raise _lib.MfcdError("pair_info_rows needs float32 GPU matrices (no CPU fallback)")
    rows, k = A.shape
    mB, d = B.shape
    idx = None if index is None else torch.as_tensor(index).to(device=A.device, dtype=torch.int64)
    per_row = idx is not None and idx.dim() == 2
    B64 = B.double()
    if not per_row:
        G = B64 if idx is None else B64[idx.clamp(0, mB - 1)]      # a bad index makes every row NaN in the kernel
        shared = (G - G.mean(0, keepdim=True)).t().contiguous()    # [d, k]
    H = torch.empty((rows, d, d), dtype=torch.float64, device=A.device)
    per = max(1, _INFO_Z_BYTES // max(1, k * d * 4))
    for r0 in range(0, rows, per):
        r1 = min(rows, r0 + per)
        lb = law
        if law is not None and law.per_user():
            lb = law.for_rows(torch.arange(r0, r1, device=A.device))
        Z = pair_hvp_multi_rows(A[r0:r1], B, None if X is None else X[r0:r1], lb, idx[r0:r1] if per_row else idx).double()
        if per_row:
            G = B64[idx[r0:r1].clamp(0, mB - 1)]                   # [b, k, d]; a row with a bad index is NaN in Z
            Hc = torch.bmm((G - G.mean(1, keepdim=True)).transpose(1, 2), Z)
        else:
            Hc = torch.matmul(shared, Z)
        H[r0:r1] = 0.5 * (Hc + Hc.transpose(1, 2))
    return H


class UserInformation(collections.namedtuple("UserInformation", ("info", "weight", "status"))):
    """What `user_information` returns, on the model's device: info f64 [k, d, d], weight f64 [k] (the user's W: the sum
    of the law's pair weights, m (m - 1) / 2 for the plain risk), status int32 [k] (0; 2: a non-finite score or truth
    row, the matrix is NaN)."""


def user_information(U, V, X, s=1.0, law=None, users=None, at="model", row_block=2048):
    """For every user named (None: every user; the law's users under a law) the d x d matrix
        H_u = sum over the law's pairs i < j of w_ij sigmoid'(a_i - a_j) (v_i - v_j)(v_i - v_j)^T
    → UserInformation.  at="model": a = U[u] V^T, and H_u is the Hessian of the user's risk sum in the row u (the
    Gauss-Newton and the exact Hessian coincide: the scores are linear in u).  at="truth": a = s X[u], and H_u / W_u is
    the Fisher information about the row that one comparison carries when it is drawn from the law and labelled with
    probability sigmoid(s (x_i - x_j)).  Blocks are formed as `law_metrics` forms them; a law's per-user columns go to
    the kernel as its index.  A user with a non-finite row gets status 2 and a NaN matrix; the others are untouched."""
    if at not in ("model", "truth"):
        raise ValueError(f"at must be 'model' or 'truth', got {at!r}")
    if not all(torch.is_tensor(t) and t.is_cuda for t in (U, V)):
        raise _lib.MfcdError("the user information needs U and V on a GPU device (there is no CPU fallback)")
    if U.dtype != torch.float32 or V.dtype != torch.float32:
        raise _lib.MfcdError("the user information takes float32 factor tables")
    plain = law is None or law.trivial
    if plain:
        src = RowBlocks(U.detach(), V.detach(), X, users, row_block, "the user information")
    else:
        src = _law_src(U.detach(), V.detach(), X, users, row_block, law, "the user information")
    d = V.shape[1]
    table = src.V.contiguous()
    info = torch.empty((src.k, d, d), dtype=torch.float64, device=src.dev)
    weight = torch.full((src.k,), src.m * (src.m - 1) / 2.0, dtype=torch.float64, device=src.dev)
    for r0, r1 in src.blocks():
        if plain:
            lb, truth = None, src.truth(r0, r1)
            scores = src.scores(r0, r1) if at == "model" else None
        else:
            lb, scores, truth = _law_block(src, law, r0, r1)
            weight[r0:r1] = pair_law_stats_rows(truth, truth, lb, s)[1][:, 0]
        if at == "truth":
            scores = truth * float(s)
        info[r0:r1] = pair_info_rows(scores, table, truth, lb, None if lb is None else lb.columns)
    status = torch.where(torch.isnan(info).flatten(1).any(1), 2, 0).to(torch.int32)
    return UserInformation(info, weight, status)


def strategy_law(X, num_triplets, strategy, device, popularity_method="zipf", alpha=1.5, k=None, n_clusters=10, seed=0):
    """The pair law a sampling strategy draws its attempts from, symmetrised (the loss of an ordered pair with label z is
    that of the swapped pair with 1 - z, so an attempt law P(i, j) enters only through P(i, j) + P(j, i)) → PairLaw on
    `device`.  The set-up of every strategy is the one `sampling.build_law` uses; `num_triplets` sets the margin's
    threshold and svd's rank.  X: dense or a FactoredMatrix (nothing n x m is formed for a factored X; `svd` takes a
    dense X only).
      random                 every pair, weight 1 (the unweighted kernels)
      margin                 pairs with |x_i - x_j| <= the threshold
      popularity, variance   alpha = p / (1 - p), beta = p: two draws without replacement have P(i, j) = p_i p_j / (1 - p_i)
      top_k                  each user's k best items
      proximity              each user's k best then k worst items, one from each list; an item in both never pairs
                             with itself
      cluster                items of different k-means clusters, alpha = beta = 1 / |cluster|
      svd                    the top items, for the top users only
    `user_similarity` has no attempt law (its loop depends on the set built so far): ValueError."""
    import generation_data as _gd
    from . import sampling
    device = torch.device(device)
    m = X.shape[1]
    if strategy == "random":
        return PairLaw(device=device)
    if strategy == "margin":
        return PairLaw(margin=float(_gd._margin_threshold(X, num_triplets)), device=device)
    if strategy in ("popularity", "variance"):
        p = sampling.item_probs(X, strategy, device, popularity_method, alpha)
        return PairLaw(alpha=p / (1.0 - p), beta=p, device=device)
    if strategy == "top_k":
        return PairLaw(columns=sampling.item_lists(X, strategy, k, device)[1], device=device)
    if strategy == "proximity":
        kk, best, worst = sampling.item_lists(X, strategy, k, device)
        cols = torch.cat((best, worst), dim=1)
        first = torch.cat((torch.ones(kk), torch.zeros(kk)))
        return PairLaw(alpha=first, beta=1.0 - first, labels=cols, columns=cols, device=device)
    if strategy == "cluster":
        kk, labels = sampling.cluster_labels(X, n_clusters, seed, device)
        w = 1.0 / torch.bincount(labels.long(), minlength=kk).double()[labels.long()]
        return PairLaw(alpha=w, beta=w, labels=labels, device=device)
    if strategy == "svd":
        top_users, top_items = _gd._svd_top_sets(X, num_triplets)
        return PairLaw(columns=top_items.astype(np.int64), users=top_users.astype(np.int64), device=device)
    if strategy == "user_similarity":
        raise ValueError("user_similarity has no attempt law: its loop depends on the set built so far")
    raise ValueError(f"no pair law for triplet sampling strategy: {strategy}")


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


_LAW_KEYS = ("expected_log_likelihood", "bayes_log_likelihood", "expected_accuracy", "bayes_accuracy")


def _law_src(U, V, X, users, row_block, law, what):
    """RowBlocks over the law's users (users=None) with the law checked against the model's shape."""
    src = RowBlocks(U, V, X, law.users if users is None else users, row_block, what)
    if law.columns is not None and law.max_column >= src.m:
        raise IndexError(f"the law names column {law.max_column} of a model of {src.m} items")
    for t in (law.columns, law.labels):
        if t is not None and t.dim() == 2 and t.shape[0] != src.n:
            raise ValueError(f"the law has {t.shape[0]} per-user rows for a model of {src.n} users")
    return src


def _law_block(src, law, r0, r1):
    """A block's law, scores and truth, restricted to the law's columns."""
    lb = law.for_rows(src.ids[r0:r1]) if law.per_user() else law
    return lb, lb.take(src.scores(r0, r1)), lb.take(src.truth(r0, r1))


def law_metrics(U, V, X, law, s=1.0, users=None, row_block=2048):
    """`pairwise_metrics` under a `PairLaw` (structure.compute_law_metrics): the four likelihood / accuracy values
    weighted by the law, from `pair_law_stats_rows`; there are no Kendall keys.  The plain key is normalised globally,
    sum over the users of the weighted sum / sum over the users of W (NaN for a law without weight; users with a
    non-finite row stay out); the `_per_user` arrays are normalised per user (NaN where W_u = 0).  users=None: the
    law's users."""
    if law.trivial:
        out = pairwise_metrics(U, V, X, s, users, row_block)
        return {k: v for k, v in out.items() if k.startswith(_LAW_KEYS)}
    src = _law_src(U.detach(), V.detach(), X, users, row_block, law, "pairwise metrics")
    sums = torch.empty((src.k, 5), dtype=torch.float64, device=src.dev)
    for r0, r1 in src.blocks():
        lb, scores, truth = _law_block(src, law, r0, r1)
        sums[r0:r1] = pair_law_stats_rows(scores, truth, lb, s)[1]
    h = _host(sums)
    good = ~np.isnan(h[:, 1])
    W = h[good, 0].sum()
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for q, name in enumerate(_LAW_KEYS, start=1):
            sign = -1.0 if q <= 2 else 1.0
            out[name] = float(sign * h[good, q].sum() / W) if W > 0 else float("nan")
            out[name + "_per_user"] = np.where(h[:, 0] > 0, sign * h[:, q] / h[:, 0], np.nan)
    return out


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


class _LawRisk(torch.autograd.Function):
    """_PopulationRisk under a PairLaw: sum over the users of the weighted risk sums / sum over the users of W.  Blocks
    are gathered to the law's columns, the k-column gradient is scattered back; 1 / sum W stays on the device."""

    @staticmethod
    def forward(ctx, U, V, src, s, law):
        total = torch.zeros(5, dtype=torch.float64, device=src.dev)
        for r0, r1 in src.blocks():
            lb, scores, truth = _law_block(src, law, r0, r1)
            total += pair_law_stats_rows(scores, truth, lb, s)[1].sum(0)
        ctx.src, ctx.s, ctx.law, ctx.inv_w = src, s, law, (1.0 / total[0]).float()
        return (total[1] / total[0]).float()               # 0 / 0 = NaN: a law without weight

    @staticmethod
    def backward(ctx, grad_out):
        src, law = ctx.src, ctx.law
        coef = grad_out.float() * ctx.inv_w
        dU_rows = torch.empty((src.k, src.U.shape[1]), dtype=torch.float32, device=src.dev)
        dV = torch.zeros_like(src.V)
        for r0, r1 in src.blocks():
            lb, scores, truth = _law_block(src, law, r0, r1)
            G = lb.put_back(pair_law_grad_rows(scores, truth, lb, ctx.s).mul_(coef), src.m)
            torch.mm(G, src.V, out=dU_rows[r0:r1])
            dV.addmm_(G.t(), src.rows_of(src.U, r0, r1))
        if src.whole:
            dU = dU_rows
        else:
            dU = torch.zeros_like(src.U).index_put_((src.ids,), dU_rows, accumulate=True)
        return dU, dV, None, None, None


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


def law_risk(U, V, X, law, s=1.0, users=None, row_block=2048):
    """`population_risk` under a `PairLaw`, normalised globally: the sum over the users and the law's pairs of w * loss
    divided by the sum of w → 0-dim fp32 device tensor, differentiable with respect to fp32 `U` and `V`.  It is not a
    mean of per-user values: under `margin` a user with more close pairs is drawn more often.  users=None: the law's
    users (every user if it names none).  A law without weight gives NaN; nothing waits for the device.  The law of
    `random` is `population_risk` itself."""
    if law.trivial:
        return population_risk(U, V, X, s, users, row_block)
    if torch.is_tensor(U) and U.is_cuda and (U.dtype != torch.float32 or V.dtype != torch.float32):
        raise _lib.MfcdError("the population risk takes float32 factor tables")
    src = _law_src(U.detach(), V.detach(), X, users, row_block, law, "the population risk")
    if src.k == 0:
        raise ValueError("the population risk needs at least one user")
    return _LawRisk.apply(U, V, src, float(s), law)


def law_weight_total(src, law, s=1.0):
    """Sum over the users of a RowBlocks of W, the law's pair weight → 0-dim f64 device tensor.  W depends on X alone
    (truth rows stand in for the scores).  A user with a non-finite truth row stays out, as in `law_metrics`: its W is
    NaN, and `law_risk` — which sums plainly — is NaN as a whole for such an input, so the Hessian product and the exact
    steps that use this total have no finite risk to agree with there; they normalise by the users that have one."""
    total = torch.zeros((), dtype=torch.float64, device=src.dev)
    for r0, r1 in src.blocks():
        lb = law.for_rows(src.ids[r0:r1]) if law.per_user() else law
        truth = lb.take(src.truth(r0, r1))
        total += torch.nansum(pair_law_stats_rows(truth, truth, lb, s)[1][:, 0])
    return total


def population_hvp(U, V, X, dU, dV, s=1.0, law=None, users=None, row_block=2048, gauss_newton=False):
    """The Hessian of `population_risk` (law=None or a trivial law) or of `law_risk` at the fp32 tables (U, V), applied
    to the direction (dU [n, d], dV [m, d]) → (HU [n, d], HV [m, d]) fp32 on the device.  With A = U V^T,
    Y = dU V^T + U dV^T, L the row Laplacians of `pair_hvp_rows`, G the score gradients of `pair_grad_rows` and c the
    risk's normaliser (1 / (users x pairs), or 1 / sum of W under a law),
        HU = c (L Y V + G dV),     HV = c ((L Y)^T U + G^T dU).
    gauss_newton=True drops the two G terms (and the gradient kernel): the product is then positive semidefinite.
    Block by block as `population_risk`: per block the scores, Y by two GEMMs, the kernel(s) and the GEMMs back.  users:
    None = every user (the law's users under a law); rows of HU of users not named are 0, a user named twice counts
    twice.  Under a law a user with a non-finite truth row stays out of c (`law_weight_total`; `law_risk` itself is NaN
    then) and its own rows of the product are NaN.  Nothing waits for the device inside the block loop; a `users` list
    is range-checked on the host once, before it."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (U, V, dU, dV)):
        raise _lib.MfcdError("the population Hessian needs the tables and the direction on a GPU (there is no CPU fallback)")
    if any(t.dtype != torch.float32 for t in (U, V, dU, dV)):
        raise _lib.MfcdError("the population Hessian takes float32 factor tables and directions")
    if dU.shape != U.shape or dV.shape != V.shape:
        raise ValueError(f"the direction must have the tables' shapes {tuple(U.shape)}, {tuple(V.shape)}")
    U, V, dU, dV = (t.detach() for t in (U, V, dU, dV))
    plain = law is None or law.trivial
    if plain:
        src = RowBlocks(U, V, X, users, row_block, "the population Hessian")
        if src.m < 2:
            raise ValueError("the population risk needs at least two items (m >= 2)")
    else:
        src = _law_src(U, V, X, users, row_block, law, "the population Hessian")
    if src.k == 0:
        raise ValueError("the population risk needs at least one user")
    coef = 1.0 / (src.k * (src.m * (src.m - 1) // 2)) if plain else (1.0 / law_weight_total(src, law, s)).float()
    HU_rows = torch.empty((src.k, U.shape[1]), dtype=torch.float32, device=src.dev)
    HV = torch.zeros_like(src.V)
    dVt = dV.t()
    for r0, r1 in src.blocks():
        Ub, dUb = src.rows_of(src.U, r0, r1), src.rows_of(dU, r0, r1)
        Y = torch.addmm(dUb @ src.Vt, Ub, dVt)
        if plain:
            scores, truth = Ub @ src.Vt, (None if gauss_newton else src.truth(r0, r1))
            Q = pair_hvp_rows(scores, Y)
            G = None if gauss_newton else pair_grad_rows(scores, truth, s)
        else:
            lb, scores, truth = _law_block(src, law, r0, r1)
            Q = lb.put_back(pair_law_hvp_rows(scores, truth, lb.take(Y), lb), src.m)
            G = None if gauss_newton else lb.put_back(pair_law_grad_rows(scores, truth, lb, s), src.m)
        torch.mm(Q, src.V, out=HU_rows[r0:r1])
        HV.addmm_(Q.t(), Ub)
        if G is not None:
            HU_rows[r0:r1].addmm_(G, dV)
            HV.addmm_(G.t(), dUb)
    HU_rows *= coef
    HV *= coef
    if src.whole:
        return HU_rows, HV
    return torch.zeros_like(src.U).index_put_((src.ids,), HU_rows, accumulate=True), HV


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


def fit_law(binding, X, s, steps, law, log_every=0, row_block=2048):
    """`fit_population` on the risk of `law_risk`: descends and logs the law's globally normalised risk over the law's
    users, blocks gathered to the law's columns and the gradient scattered back.  The law's total weight is a function of
    X alone: it is computed once, before the loop (the one host wait; ValueError if it is 0).  The gradient rows of users
    outside the law stay zero; weight decay still moves them, as the reference's dense Adam does.  The law of `random`
    is `fit_population` itself."""
    from . import engine
    if law.trivial:
        return fit_population(binding, X, s, steps, log_every, row_block)
    if not isinstance(binding, engine.AdamBinding):
        binding = engine.AdamBinding(*binding)
    for name, t in zip(("model.U", "model.V"), binding.tensors()[:2]):
        engine._require_cuda_param(t, name)                    # fp32 only: bf16 tables are refused here
    L = _lib.load()
    U, V, mU, vU, mV, vV = binding.tensors()
    src = _law_src(U, V, X, None, row_block, law, "the population fit")
    n, m, d, dev = src.n, src.m, U.shape[1], src.dev
    steps, k = int(steps), int(log_every)
    blocks = src.blocks()
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for r0, r1 in blocks:                                   # W depends on X alone: truth rows stand in for the scores
        lb = law.for_rows(src.ids[r0:r1]) if law.per_user() else law
        truth = lb.take(src.truth(r0, r1))
        total += pair_law_stats_rows(truth, truth, lb, s)[1][:, 0].sum()
    total = float(total)                                    # the one host wait, outside the loop
    if not total > 0:
        raise ValueError("the law gives no pair of any user a weight: there is no risk to descend")
    inv = 1.0 / total
    at = ([t for t in range(0, steps, k)] + [steps]) if k > 0 else []
    log = torch.zeros(max(len(at), 1), dtype=torch.float64, device=dev)
    gU, gV = torch.zeros_like(U), torch.empty_like(V)
    ptrs = [_lib.ptr(t) for t in (U, V, mU, vU, mV, vV, gU, gV)]
    lr, b1, b2, eps, wd = binding.hyper()
    stream = _lib.stream_ptr(dev)

    def risk_into(slot, lb, scores, truth):
        slot += pair_law_stats_rows(scores, truth, lb, s)[1][:, 1].sum()

    try:
        for t in range(steps):
            logging = k > 0 and t % k == 0
            if not src.whole:
                gU.zero_()
            for b, (r0, r1) in enumerate(blocks):
                lb, scores, truth = _law_block(src, law, r0, r1)
                if logging:
                    risk_into(log[t // k], lb, scores, truth)
                G = lb.put_back(pair_law_grad_rows(scores, truth, lb, s).mul_(inv), m)
                Ub = src.rows_of(U, r0, r1)
                if src.whole:
                    torch.mm(G, V, out=gU[r0:r1])
                else:                                       # users outside the law keep a zero gradient row
                    gU.index_add_(0, src.ids[r0:r1], G @ V)
                if b == 0:
                    torch.mm(G.t(), Ub, out=gV)
                else:
                    gV.addmm_(G.t(), Ub)
            _lib.check(L.mfcd_adam_dense(*ptrs, binding.step + 1, n, m, d, lr, b1, b2, eps, wd, stream))
            binding.advance(1, defer=True)
    finally:
        binding.flush()         # an interrupt must not leave the moments ahead of the optimizer's `step` tensors
    if k <= 0:
        return [], []
    for r0, r1 in blocks:
        risk_into(log[len(at) - 1], *_law_block(src, law, r0, r1))
    return at, (log[:len(at)] * inv).cpu().tolist()       # the one device->host transfer of the run
