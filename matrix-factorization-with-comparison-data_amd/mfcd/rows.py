"""A score matrix as the row kernels' host code meets it: `ScoreMatrix` is X [n, m] as a dense tensor or as factors with
X = A @ B.T, and `resolve` makes one from a dense tensor, a `generation_data.FactoredMatrix` (told by `_lib.is_factored`:
this package does not import that module) or a pair (A, B).  It moves and checks and converts nothing: every caller asks
for the dtype and the contiguity its kernel takes.  `RowBlocks` forms rows of U V^T and of X a block at a time."""
import torch

from . import _lib


def blocks(k, block):
    """[(r0, r1)] covering [0, k) in steps of `block`, the last one ragged."""
    return [(r0, min(r0 + block, k)) for r0 in range(0, k, block)]


class ScoreMatrix:
    """X [n, m] on `device`: `dense`, or `A` [n, d] and `B` [m, d] with X = A @ B.T (the other side is None)."""

    def __init__(self, dense=None, A=None, B=None):
        self.dense, self.A, self.B = dense, A, B
        self.factored = dense is None
        self.n, self.m, self.d = (A.shape[0], B.shape[0], A.shape[1]) if self.factored else (*dense.shape, 0)
        self.device = A.device if self.factored else dense.device

    def rows(self, r0, r1=None):
        """Rows [r0, r1), or the rows an index tensor `r0` names, as a dense block (one GEMM for factors)."""
        sel = r0 if r1 is None else slice(r0, r1)
        return self.A[sel] @ self.B.t() if self.factored else self.dense[sel]

    def map(self, fn):
        """The same matrix with `fn` applied to its tensor(s), e.g. a dtype or a layout."""
        return ScoreMatrix(A=fn(self.A), B=fn(self.B)) if self.factored else ScoreMatrix(fn(self.dense))


def resolve(X, device=None, gpu_only=False):
    """→ ScoreMatrix.  With `device` the tensors move there, without they stay.  `gpu_only` (top-k's rule): tensors
    handed over as such (dense, or a pair) have to be on a GPU already and stay there whatever `device` says; the
    factors of a FactoredMatrix, a host object, go to `device` (None: the current GPU)."""
    host = _lib.is_factored(X)
    if host or (isinstance(X, (tuple, list)) and len(X) == 2):
        parts = [("A", X.A if host else X[0]), ("B", X.B if host else X[1])]
    elif torch.is_tensor(X):
        parts = [("X", X)]
    else:
        raise TypeError("X must be a dense GPU tensor, a FactoredMatrix or a pair (A, B) of GPU tensors")
    if gpu_only and host:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _lib.MfcdError("a factored X needs a GPU device (there is no CPU fallback)")
    elif gpu_only:
        device = None                              # they stay where they are
    for name, t in parts:
        if not torch.is_tensor(t) or (gpu_only and not host and not t.is_cuda):
            raise _lib.MfcdError(f"{name} must be a GPU tensor (got "
                                 f"{'a CPU tensor' if torch.is_tensor(t) else type(t).__name__}; there is no CPU fallback)")
        if t.dim() != 2:
            raise ValueError(f"{name} must have two dimensions, got {tuple(t.shape)}")
    ts = [t.detach() if device is None else t.detach().to(device) for _, t in parts]
    if len(ts) == 1:
        return ScoreMatrix(ts[0])
    A, B = ts
    if A.shape[1] != B.shape[1] or A.device != B.device:
        raise ValueError(f"factors do not match: A {tuple(A.shape)} on {A.device}, B {tuple(B.shape)} on {B.device}")
    return ScoreMatrix(A=A, B=B)


class RowBlocks:
    """The chosen users' score rows U[u] V^T and ground-truth rows X[u] (A[u] B^T for a factored X), formed `row_block`
    users at a time by plain library GEMMs; nothing n x m is formed for a factored X."""

    def __init__(self, U, V, X, users, row_block, what):
        if not torch.is_tensor(U) or not U.is_cuda:
            raise _lib.MfcdError(f"{what} need the model on a GPU (there is no CPU fallback)")
        self.dev = dev = U.device
        self.U, self.V = U.float(), V.float()
        n, m = U.shape[0], V.shape[0]
        if not torch.is_tensor(X) and not _lib.is_factored(X):
            raise TypeError("X must be a dense GPU tensor or a FactoredMatrix")
        if tuple(X.shape) != (n, m):
            raise ValueError(f"X must be [{n},{m}], got {tuple(X.shape)}")
        X = resolve(X, dev)
        self.X = X if X.factored else X.map(torch.Tensor.float)
        self.whole = users is None
        if self.whole:
            self.ids = torch.arange(n, device=dev)
        else:
            self.ids = torch.as_tensor(users).reshape(-1).to(device=dev, dtype=torch.int64)
            if self.ids.numel() and (int(self.ids.min()) < 0 or int(self.ids.max()) >= n):
                raise IndexError(f"user number out of range for a model of {n} users")
        self.n, self.m, self.k = n, m, self.ids.numel()
        self.row_block = max(1, int(row_block))
        self.Vt = self.V.t()

    def blocks(self):
        return blocks(self.k, self.row_block)

    def rows_of(self, table, r0, r1):
        return table[r0:r1] if self.whole else table[self.ids[r0:r1]]

    def scores(self, r0, r1):
        return self.rows_of(self.U, r0, r1) @ self.Vt

    def truth(self, r0, r1):
        return self.X.rows(r0, r1) if self.whole else self.X.rows(self.ids[r0:r1])
