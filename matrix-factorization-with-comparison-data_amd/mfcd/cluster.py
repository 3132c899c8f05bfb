"""k-means over item vectors on the device (include/mfcd.h: mfcd_kmeans_assign, mfcd_kmeans_update; csrc/kmeans.hip).

What the `cluster` sampling strategy needs in front of its attempt loop (generation_data.py:229-247: sklearn KMeans
over the item columns of X): the points of the items, k-means++ seeding, and Lloyd iterations with sklearn's rule for
empty clusters.  The two steps of an iteration are HIP kernels; the loop reads one small tensor per iteration.  Parity
with sklearn is not bitwise and not promised: the generator stream and the plain (not greedy) seeding are this
module's own, as for every device law of mfcd/sampling.py.  There is no CPU form of `assign`, `update` and `kmeans`.
"""
import torch

from . import _lib
from .rows import resolve


def max_k():
    return int(_lib.load().mfcd_kmeans_max_k())


def item_points(X, device):
    """One fp32 point per item, row-major [m, dim] on `device`: the item columns of a dense X [n, m] (dim = n), or, for
    a FactoredMatrix X = A B^T (A [n, dx], B [m, dx]), the rows of B R^T with A^T A = R^T R (dim = dx) — an isometry:
    |R (b_i - b_j)| = |A (b_i - b_j)|, so the distances between these rows are those between the columns of X."""
    X = resolve(X)
    if X.factored:                                      # d x d algebra in f64, on the factors' own device
        A, B = X.A.double(), X.B.double()
        G = A.t() @ A
        R, info = torch.linalg.cholesky_ex(G, upper=True)
        if int(info) != 0:                              # A without full column rank: G = Q diag(w) Q^T, R = diag(sqrt w) Q^T
            w, Q = torch.linalg.eigh(G)
            R = torch.sqrt(w.clamp_min(0.0))[:, None] * Q.t()
        return (B @ R.t()).float().to(device).contiguous()
    return X.dense.to(device=device, dtype=torch.float32).t().contiguous()


def _checked(points, centres):
    for t, name in ((points, "points"), (centres, "centres")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.MfcdError(f"{name} must be a GPU tensor (there is no CPU fallback)")
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 tensor with two dimensions")
    P, dim = points.shape
    k = centres.shape[0]
    if centres.shape[1] != dim or centres.device != points.device:
        raise ValueError(f"centres {tuple(centres.shape)} on {centres.device} do not match points {tuple(points.shape)} "
                         f"on {points.device}")
    nbytes = _lib.load().mfcd_kmeans_workspace_bytes(P, dim, k)
    if nbytes == 0:
        raise ValueError(f"k-means sizes out of range: {P} points, dim {dim}, k = {k} (1 <= k <= {max_k()})")
    return P, dim, k, _lib.workspace(nbytes, points.device)


def assign(points, centres, labels=None, dist2=False, changed=None):
    """labels[p] = the nearest centre (lowest index among equals) → labels, or (labels, dist2) with `dist2=True`.
    `labels`: an int32 [P] tensor to overwrite (a new one if None); `changed`: an int32 device tensor of one element
    that receives how many labels differ from the ones passed in."""
    P, dim, k, ws = _checked(points, centres)
    dev = points.device
    if labels is None:
        labels = torch.full((P,), -1, dtype=torch.int32, device=dev)
    d2 = torch.empty(P, dtype=torch.float32, device=dev) if dist2 else None
    _lib.check(_lib.load().mfcd_kmeans_assign(_lib.ptr(points), P, dim, _lib.ptr(centres), k, _lib.ptr(labels),
                                              _lib.ptr(d2), _lib.ptr(changed), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr(dev)))
    return (labels, d2) if dist2 else labels


def update(points, labels, centres):
    """centres[c] ← the mean of the points labelled c, in place (an empty cluster keeps its centre) → counts int32 [k]."""
    P, dim, k, ws = _checked(points, centres)
    counts = torch.empty(k, dtype=torch.int32, device=points.device)
    _lib.check(_lib.load().mfcd_kmeans_update(_lib.ptr(points), P, dim, _lib.ptr(labels), k, _lib.ptr(centres),
                                              _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device)))
    return counts


def _plus_plus(points, k, seed):
    """Plain k-means++: the first centre uniform, every next one drawn with probability proportional to the squared
    distance to the nearest centre so far (`assign`'s dist2 against the newest centre, min-ed into the running one)."""
    P, dev = points.shape[0], points.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    centres = torch.empty((k, points.shape[1]), dtype=torch.float32, device=dev)
    centres[0] = points[torch.randint(P, (1,), generator=gen, device=dev)]
    near = None
    for t in range(1, k):
        d2 = assign(points, centres[t - 1:t], dist2=True)[1]
        near = d2 if near is None else torch.minimum(near, d2)
        w = near + (near.sum() <= 0).float()                       # every point on a centre already: uniform
        centres[t] = points[torch.multinomial(w, 1, generator=gen)]
    return centres


def kmeans(points, k, seed, init=None, max_iter=300):
    """Lloyd's k-means of fp32 GPU points [P, dim] → (labels int32 [P], centres fp32 [k, dim], iterations run).

    Initial centres: `init` [k, dim], else plain k-means++ from a device generator seeded with `seed`.  Iterations
    assign → update until no label changes or `max_iter`.  A cluster left without members takes the point farthest from
    its own centre (largest dist2, lowest index among equals; several empty clusters in descending distance), as
    sklearn relocates them, and the loop goes on.  The labels are those of the last assign step; after convergence
    they are the assignment of the returned centres."""
    k = int(k)
    P = points.shape[0]
    if P < k:
        raise ValueError(f"n_samples={P} should be >= n_clusters={k}.")
    if init is None:
        centres = _plus_plus(points, k, seed)
    else:
        centres = torch.as_tensor(init).to(device=points.device, dtype=torch.float32).contiguous().clone()
        if centres.shape != (k, points.shape[1]):
            raise ValueError(f"init must have shape {(k, points.shape[1])}, got {tuple(centres.shape)}")
    labels = torch.full((P,), -1, dtype=torch.int32, device=points.device)
    changed = torch.zeros(1, dtype=torch.int32, device=points.device)
    n_iter = 0
    for n_iter in range(1, int(max_iter) + 1):
        _, d2 = assign(points, centres, labels, dist2=True, changed=changed)
        counts = update(points, labels, centres)
        n_changed, n_empty = torch.stack((changed[0], (counts == 0).sum().int())).tolist()   # the loop's host wait
        if n_empty:
            far = torch.sort(d2, descending=True, stable=True)[1][:n_empty]
            labels[far] = torch.nonzero(counts == 0).reshape(-1).int()
            update(points, labels, centres)
        elif n_changed == 0:
            break
    return labels, centres, n_iter
