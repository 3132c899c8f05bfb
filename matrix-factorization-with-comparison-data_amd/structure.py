"""MI355X-native drop-in for the reference module of the same name.

Same function names, argument meaning, return types and `.pkl` layout as
MayeulCassier/Matrix-Factorization-With-Comparison-Data `structure.py` (cited below as ref:LINE),
so `Runs.ipynb` / `Plots.ipynb` work unchanged — but the training step, the evaluation pass and the
dense UV^T metrics run as hand-written gfx950 kernels behind the C-ABI in include/mfcd.h.
This file is host glue only; it holds no arithmetic of the hot path and has no CPU fallback:
`device` must name a GPU.
"""
import itertools
import os
import pickle

os.environ.setdefault("OMP_NUM_THREADS", "4")  # the reference pins this at import (ref:3); host work here is tiny

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

from generation_data import *  # noqa: F401,F403  (ref:17 re-exports every sampler/generator name)
import generation_data as _gd
from mfcd import alternating as _alternating
from mfcd import design as _design
from mfcd import engine as _engine
from mfcd import foldin as _foldin
from mfcd import implicit as _implicit
from mfcd import implicit_exact as _implicit_exact
from mfcd import implicit_foldin as _implicit_foldin
from mfcd import lists as _lists
from mfcd import lists_exact as _lists_exact
from mfcd import metrics as _metrics
from mfcd import newton as _newton
from mfcd import pairs as _pairs
from mfcd import population as _population
from mfcd import ranking as _ranking
from mfcd import ratings as _ratings
from mfcd import ratings_exact as _ratings_exact
from mfcd import ratings_foldin as _ratings_foldin
from mfcd import sampling as _sampling
from mfcd import topk as _topk

if torch.get_num_threads() > 16:  # imported after torch: keep the host-side pool small (GPU boxes expose 100s of cores)
    torch.set_num_threads(4)

try:  # progress bars are cosmetic (ref:840)
    from tqdm import tqdm as _tqdm
except Exception:  # pragma: no cover
    _tqdm = None


# ------------------------------------------------------------------------------------------------
# model (ref:746-795)
# ------------------------------------------------------------------------------------------------
class MatrixFactorization(nn.Module):
    """BTL comparison model: P(u prefers i over j) = sigmoid(U[u] . (V[i] - V[j])).

    Parameters `.U [n_users, d]`, `.V [n_items, d]`, fp32, drawn N(0, 1/d) in this order (ref:770-771).
    Calling the module evaluates the forward kernel; `train_model` fuses forward, backward and Adam on the device
    for torch.optim.Adam and runs the reference's per-batch loop over the same kernels for any other optimiser."""

    def __init__(self, n_users, n_items, d, dtype=torch.float32):
        """`dtype=torch.bfloat16` (extension, BASELINE configs[2]) stores the factors in bf16: same fp32 draws,
        rounded to nearest even; training then keeps fp32 Adam moments and rounds once per step."""
        super().__init__()
        scale = torch.sqrt(torch.tensor(d, dtype=torch.float32))
        self.U = nn.Parameter((torch.randn(n_users, d) / scale).to(dtype))
        self.V = nn.Parameter((torch.randn(n_items, d) / scale).to(dtype))

    def forward(self, u, i, j):
        """ref:773-795 on the forward kernel.  fp32 factors that require grad get an autograd graph (custom Function:
        backward = sigmoid backward + the scatter-accumulate kernel), so `loss.backward()` on the result fills
        `.U.grad` / `.V.grad` as it does in the reference; bf16 factors and no-grad contexts return a plain tensor."""
        rec = _engine.records_from_indices(u, i, j, self.U.shape[0], self.V.shape[0], self.U.device)
        if torch.is_grad_enabled() and self.U.dtype == torch.float32 and (self.U.requires_grad or self.V.requires_grad):
            return _engine.TripletForward.apply(self.U, self.V, rec)
        _, _, p = _engine.eval_batches(self.U.data, self.V.data, rec, min(max(rec.shape[0], 1), 4096), want_p=True)
        return p


# ------------------------------------------------------------------------------------------------
# training / evaluation (ref:812-921)
# ------------------------------------------------------------------------------------------------
def _need_gpu(device):
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"device={device!r}: this build runs the triplet hot path on an MI355X only; "
                           "pass device='cuda' (there is deliberately no CPU fallback)")


def train_model(model, train_loader, val_loader, optimizer, device, num_epochs=100, is_last=False,
                open_browser=False):
    """ref:812-878.  Returns (train_losses, val_losses), one Python float per epoch
    (mean over batches of the batch-mean BCE; the short last batch weighs like any other).
    `is_last` / `open_browser` only ever fed the reference's disabled TensorBoard block."""
    _need_gpu(device)
    model.train()
    progress = (lambda it: _tqdm(it, desc="Training Progress")) if _tqdm is not None else None
    if _engine.fused_step_applies(model, optimizer):
        out = _engine.fit(model, train_loader, val_loader, optimizer, num_epochs, progress)
    else:   # any other optimiser (or Adam flags the fused step does not implement): the generic loop, same kernels
        out = _engine.fit_generic(model, train_loader, val_loader, optimizer, num_epochs, progress)
    model.eval()
    return out


def train_models(models, train_loaders, val_loaders, optimizers, device, num_epochs=100):
    """Extension (not in the reference): `[train_model(*args, device, num_epochs) for args in zip(...)]` in one go, with
    the same results, optimizer states and RNG use.  The models the batched local form takes (fp32, torch.optim.Adam, the
    tiny sizes the local form covers: n = m = 1000 at d = 2, n = m = 256 at d = 8) train side by side, one CU each, in a
    fixed number of launches per epoch; every other model trains alone in its place (mfcd.engine.fit_many)."""
    _need_gpu(device)
    for model in models:
        model.train()
    out = _engine.fit_many(models, train_loaders, val_loaders, optimizers, num_epochs)
    for model in models:
        model.eval()
    return out


def evaluate_model(model, test_loader, device):
    """ref:881-921 → (mean batch BCE, accuracy of (p > 0.5) against the labels)."""
    _need_gpu(device)
    model.eval()
    return _engine.evaluate(model, test_loader)


def compute_reconstruction_error(model, X, s):
    """ref:925-955 → ||(UV^T - column mean) - sX||_F / ||sX||_F as a float."""
    return _metrics.reconstruction_error(model.U.data, model.V.data, X, s)


def compute_alpha_and_norm_ratios(model, X_init):
    """ref:958-1082 → the 14-tuple in the reference's order."""
    return _metrics.alpha_and_norm_ratios(model.U.data, model.V.data, X_init)


def recommend_items(model, users=None, k=10, exclude=None):
    """Extension (not in the reference): the k items the model ranks highest for each of `users` (None: every user), best
    first → int32 [len(users), k] tensor on the model's device (include/mfcd.h mfcd_topk_rows over U, V: the rows of
    U V^T are never formed).  Equal scores are ordered by item number.  `exclude`: a set / array / tensor of (u, i) or
    (u, i, j) rows — what u has been shown; a triplet bars both of its items for its user — which are left out; a user
    with fewer than k items left gets -1 in the tail."""
    _need_gpu(model.U.device)
    return _topk.topk_rows((model.U.data, model.V.data), k, rows=users, ends="best", exclude=exclude)


def compute_topk_overlap(model, X, k=10):
    """Extension (not in the reference): how much of X's top-k per user the model's top-k recovers →
    (mean over users, per-user float64 numpy array) of |top-k(U V^T row) ∩ top-k(X row)| / k.  X: a dense GPU tensor or a
    `FactoredMatrix` (nothing n x m is formed for either side).  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    dev = model.U.device
    mine = _topk.topk_rows((model.U.data, model.V.data), k, ends="best").long()
    if torch.is_tensor(X):
        X = X.to(dev)
    theirs = _topk.topk_rows(X, k, ends="best", device=dev).long()
    if mine.shape != theirs.shape:
        raise ValueError(f"X must be [{model.U.shape[0]},{model.V.shape[0]}], got {tuple(X.shape)}")
    m = model.V.shape[0]
    row = torch.arange(mine.shape[0], device=dev).unsqueeze(1) * m
    hit = torch.isin((mine + row).reshape(-1), (theirs + row).reshape(-1)).reshape(mine.shape)
    per_user = (hit.sum(1).double() / k).cpu().numpy()
    return float(per_user.mean()), per_user


def compute_pairwise_metrics(model, X, s=1.0, users=None, row_block=2048):
    """Extension (not in the reference): what the sampled test split estimates, computed exactly over ALL item pairs
    i < j of a user (include/mfcd.h mfcd_pair_stats_rows), with the model's score row a = U[u] V^T, the ground truth
    x = X[u] and the label law q = sigmoid(s (x_i - x_j)).  Returns a dict; every key also exists with the suffix
    `_per_user` as a float64 numpy array holding NaN where the value is undefined, and the plain key is the mean over the
    users where it is defined (0.0 if there are none, as the Spearman mean):
      kendall_tau              Kendall's tau-b of a and x from the exact pair counts (NaN: a constant row, or a NaN in it)
      pairwise_accuracy        share of the pairs that x orders which a orders the same way
      expected_log_likelihood  minus the mean of q (-log p) + (1 - q)(-log(1 - p)), p = sigmoid(a_i - a_j): the expected
                               value of the result dict's `log_likelihoods` over all pairs, unclamped
      bayes_log_likelihood     the same for the ideal scores a = s x: no model can exceed it
      expected_accuracy        expected accuracy of (p > 0.5) against hard labels drawn from q
      bayes_accuracy           mean of max(q, 1 - q): its ceiling
    X: a dense GPU tensor or a `FactoredMatrix` (rows are formed `row_block` at a time; nothing n x m is formed for a
    factored X).  users: None = every user, else user numbers, returned in that order — the cost is O(m^2) per user, so
    pass a sample at BASELINE C4 / C5 sizes.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _pairs.pairwise_metrics(model.U.data, model.V.data, X, s, users, row_block)


def population_risk(model, X, s=1.0, users=None, row_block=2048):
    """Extension (not in the reference): the quantity the sampled experiments estimate, as a differentiable scalar — the
    mean over `users` (None: every user; a user named twice counts twice) and over ALL item pairs of the BCE of
    p = sigmoid(a_i - a_j), a = U[u] V^T, under the label law q = sigmoid(s (x_i - x_j)); minus
    `compute_pairwise_metrics`' expected_log_likelihood.  Returns a 0-dim fp32 tensor on the model's device;
    `population_risk(...).backward()` fills `model.U.grad` / `model.V.grad` (include/mfcd.h mfcd_pair_grad_rows and two
    library GEMMs per block of `row_block` users), so any torch optimiser can descend it.  fp32 models only.
    X: a dense GPU tensor or a `FactoredMatrix`.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _pairs.population_risk(model.U, model.V, X, s, users, row_block)


def train_model_population(model, X, s, optimizer, device, num_steps=1000, log_every=100, row_block=2048):
    """Extension (not in the reference): `train_model` with unlimited comparisons — `num_steps` full-batch optimiser steps
    on `population_risk(model, X, s)` over every user: what the model and its weight decay converge to when sampling
    error is gone.  Returns (steps, risks) as Python lists: the risk after steps[k] = 0, log_every, 2 log_every, ...
    optimiser steps and after the last one (two empty lists for log_every = 0), read from the device once at the end.
    torch.optim.Adam takes the fused loop (mfcd.pairs.fit_population: risk gradient, GEMMs and one dense Adam kernel
    per step, the optimizer's state updated in place); any other optimiser runs zero_grad / population_risk / backward /
    step.  Not part of the result dict / .pkl layout."""
    _need_gpu(device)
    model.train()
    if _engine.fused_step_applies(model, optimizer):
        out = _pairs.fit_population(_engine.AdamBinding(model, optimizer), X, s, num_steps, log_every, row_block)
    else:
        at, seen = [], []
        for t in range(int(num_steps)):
            optimizer.zero_grad()
            loss = population_risk(model, X, s, None, row_block)
            loss.backward()
            optimizer.step()
            if log_every > 0 and t % log_every == 0:
                at.append(t)
                seen.append(loss.detach())
        if log_every > 0:
            with torch.no_grad():
                at.append(int(num_steps))
                seen.append(population_risk(model, X, s, None, row_block))
        out = (at, torch.stack(seen).double().cpu().tolist() if seen else [])
    model.eval()
    return out


def sampling_law(X, num_triplets, strategy="random", **kw):
    """Extension (not in the reference): the law `get_triplets_from_X(X, num_triplets, strategy, **kw)` draws its attempts
    from, as a weight on every user's item pairs → mfcd.pairs.PairLaw on the GPU (device=..., default: X's if it is on
    one), for `law_risk`, `train_model_law` and `compute_law_metrics`: the exact value a test split drawn with that
    strategy estimates, and what training with it converges to with unlimited comparisons.  kw: popularity_method,
    alpha, k, n_clusters, seed, as the strategy takes them.  `user_similarity` has no such law (ValueError): its loop
    depends on the set built so far.  Not part of the result dict / .pkl layout."""
    device = kw.pop("device", None)
    if device is None:
        device = X.device if torch.is_tensor(X) and X.is_cuda else torch.device("cuda")
    _need_gpu(device)
    return _pairs.strategy_law(X, int(num_triplets), strategy, device, **kw)


def compute_law_metrics(model, X, law, s=1.0, users=None, row_block=2048):
    """Extension (not in the reference): `compute_pairwise_metrics` under a `sampling_law` — expected_log_likelihood,
    bayes_log_likelihood, expected_accuracy and bayes_accuracy with every item pair weighted by the law (include/mfcd.h
    mfcd_pair_law_stats_rows); there are no Kendall keys.  The plain key is normalised by the weight of all users (NaN
    for a law without weight), the `_per_user` arrays by each user's own (NaN where that is 0).  users=None: the law's
    users.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _pairs.law_metrics(model.U.data, model.V.data, X, law, s, users, row_block)


def law_risk(model, X, law, s=1.0, users=None, row_block=2048):
    """Extension (not in the reference): `population_risk` under a `sampling_law` — the sum over the users and item pairs
    of w * BCE divided by the sum of w, the exact value that a test split drawn with the law's strategy estimates (a
    global normalisation, not a mean of per-user values: under `margin` a user with more close pairs is drawn more
    often).  Returns a 0-dim fp32 tensor on the model's device; `.backward()` fills `model.U.grad` / `model.V.grad`
    (include/mfcd.h mfcd_pair_law_grad_rows).  users=None: the law's users.  NaN for a law without weight.  Not part of
    the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _pairs.law_risk(model.U, model.V, X, law, s, users, row_block)


def train_model_law(model, X, s, optimizer, device, law, num_steps=1000, log_every=100, row_block=2048):
    """Extension (not in the reference): `train_model_population` on `law_risk(model, X, law, s)` — what training with the
    law's sampling strategy converges to with unlimited comparisons.  Returns (steps, risks) as `train_model_population`
    does, the risks being the law's.  torch.optim.Adam takes the fused loop (mfcd.pairs.fit_law), any other optimiser
    zero_grad / law_risk / backward / step.  Users outside the law get no gradient, only weight decay; a law without
    weight is a ValueError on the fused path.  Not part of the result dict / .pkl layout."""
    _need_gpu(device)
    model.train()
    if _engine.fused_step_applies(model, optimizer):
        out = _pairs.fit_law(_engine.AdamBinding(model, optimizer), X, s, num_steps, law, log_every, row_block)
    else:
        at, seen = [], []
        for t in range(int(num_steps)):
            optimizer.zero_grad()
            loss = law_risk(model, X, law, s, None, row_block)
            loss.backward()
            optimizer.step()
            if log_every > 0 and t % log_every == 0:
                at.append(t)
                seen.append(loss.detach())
        if log_every > 0:
            with torch.no_grad():
                at.append(int(num_steps))
                seen.append(law_risk(model, X, law, s, None, row_block))
        out = (at, torch.stack(seen).double().cpu().tolist() if seen else [])
    model.eval()
    return out


def observe_ratings(X, p, levels=None, seed=0):
    """Extension (not in the reference): a ratings table from a dense X — every entry is kept with probability p, drawn
    from a private CPU torch.Generator(seed) (the global torch and numpy RNG states are not touched, so the host
    pipeline's draw order stays what it is).  levels=k replaces the kept values by the ratings 1..k, cut at the global
    k-quantiles of the kept values.  Returns an mfcd.ratings.RatingsData on X's device: what `ratings_risk`,
    `train_model_ratings` and `compute_ratings_metrics` take, to ask how reconstruction degrades with p and k.  Not part
    of the result dict / .pkl layout."""
    if not torch.is_tensor(X) or X.dim() != 2:
        raise ValueError("observe_ratings takes a dense [n, m] tensor")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError("p must lie in [0, 1]")
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    keep = torch.rand(X.shape, generator=gen) < float(p)
    users, items = keep.nonzero(as_tuple=True)
    values = X.detach().cpu().float()[keep].numpy()
    if levels is not None:
        k = int(levels)
        if k < 1:
            raise ValueError("levels must be >= 1")
        edges = np.quantile(values.astype(np.float64), np.arange(1, k) / k) if values.size else np.zeros(k - 1)
        values = 1.0 + np.searchsorted(edges, values.astype(np.float64), side="right")
    return _ratings.RatingsData(users.numpy(), items.numpy(), values, X.shape[0], X.shape[1]).to(X.device)


def load_ratings(path, sep=None):
    """Extension (not in the reference): reads a text file of `user item value [ignored columns]` lines (sep=None: any
    white space, the layout of MovieLens' u.data) with numpy; the user and item ids are mapped to 0..n-1 and 0..m-1 in
    the order of their sorted unique values.  Returns (data, user_ids, item_ids): an mfcd.ratings.RatingsData on the CPU
    (`.to(device)` moves it) and the id of every row and column.  Not part of the result dict / .pkl layout."""
    table = np.loadtxt(path, delimiter=sep, usecols=(0, 1, 2), ndmin=2, dtype=np.float64)
    user_ids, users = np.unique(table[:, 0], return_inverse=True)
    item_ids, items = np.unique(table[:, 1], return_inverse=True)
    if (user_ids == np.round(user_ids)).all() and (item_ids == np.round(item_ids)).all():
        user_ids, item_ids = user_ids.astype(np.int64), item_ids.astype(np.int64)
    data = _ratings.RatingsData(users.reshape(-1), items.reshape(-1), table[:, 2], user_ids.size, item_ids.size)
    return data, user_ids, item_ids


def ratings_risk(model, data, s=1.0, skip_ties=False):
    """Extension (not in the reference): the exact BTL risk of the model on a ratings table as a differentiable scalar —
    over every user and ALL pairs of items that user rated, the BCE of p = sigmoid(a_k - a_l) under the label law
    q = sigmoid(s (x_k - x_l)), divided by the number of such pairs of all users (skip_ties: pairs with equal ratings
    carry no preference and stay out).  Returns a 0-dim fp32 tensor on the model's device; `.backward()` fills
    `model.U.grad` / `model.V.grad` (include/mfcd.h mfcd_pair_ragged_grad, mfcd_ragged_gather_sum).  fp32 models only;
    data: an mfcd.ratings.RatingsData on the model's device.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _ratings.ratings_risk(model.U, model.V, data, s, skip_ties)


def train_model_ratings(model, data, s, optimizer, device, num_steps=1000, log_every=100, skip_ties=False):
    """Extension (not in the reference): `train_model_population` on `ratings_risk(model, data, s)` — full-batch optimiser
    steps on the exact risk of the observed ratings.  Returns (steps, risks) as `train_model_population` does.
    torch.optim.Adam takes the fused loop (mfcd.ratings.fit_ratings), any other optimiser zero_grad / ratings_risk /
    backward / step.  Not part of the result dict / .pkl layout."""
    _need_gpu(device)
    model.train()
    if _engine.fused_step_applies(model, optimizer):
        out = _ratings.fit_ratings(_engine.AdamBinding(model, optimizer), data, s, num_steps, log_every, skip_ties)
    else:
        at, seen = [], []
        for t in range(int(num_steps)):
            optimizer.zero_grad()
            loss = ratings_risk(model, data, s, skip_ties)
            loss.backward()
            optimizer.step()
            if log_every > 0 and t % log_every == 0:
                at.append(t)
                seen.append(loss.detach())
        if log_every > 0:
            with torch.no_grad():
                at.append(int(num_steps))
                seen.append(ratings_risk(model, data, s, skip_ties))
        out = (at, torch.stack(seen).double().cpu().tolist() if seen else [])
    model.eval()
    return out


def compute_ratings_metrics(model, data, s=1.0, skip_ties=False):
    """Extension (not in the reference): `compute_pairwise_metrics` on a ratings table, typically a held-out split
    (`data.split`): the same keys and `_per_user` arrays, every user's values over the pairs among the items that user
    rated (include/mfcd.h mfcd_pair_ragged_stats); a user without a pair is NaN and stays out of the means.  skip_ties:
    the likelihood and accuracy keys over the pairs with different ratings only.  Not part of the result dict / .pkl
    layout."""
    _need_gpu(model.U.device)
    return _ratings.ratings_metrics(model.U.data, model.V.data, data, s, skip_ties)


def observe_rankings(X, length, depth=None, s=1.0, seed=0):
    """Extension (not in the reference): ranked lists from a dense X — every user is shown `length` items, a uniform draw
    without replacement, and orders them by s x + Gumbel noise, an exact Plackett–Luce draw with scores s x (s = inf: the
    noiseless order); depth=K keeps the order of the best K only, the rest is an unordered tail.  The draw comes from a
    private torch.Generator(seed) on X's device (the global torch and numpy RNG states are not touched).  Returns an
    mfcd.lists.RankedLists on X's device: what `rankings_risk`, `train_model_rankings` and `compute_rankings_metrics`
    take.  Not part of the result dict / .pkl layout."""
    return _lists.sample_rankings(X, length, depth, s, seed)


def load_rankings(path, sep=None, depth=None):
    """Extension (not in the reference): reads a text file of `user item position [ignored columns]` lines (sep=None: any
    white space) with numpy; the user and item ids are mapped to 0..n-1 and 0..m-1 in the order of their sorted unique
    values, as `load_ratings` maps them; a user's items are ordered by position, smallest first = best.  Returns
    (lists, user_ids, item_ids): an mfcd.lists.RankedLists on the CPU (`.to(device)` moves it) and the id of every row
    and column.  Not part of the result dict / .pkl layout."""
    table = np.loadtxt(path, delimiter=sep, usecols=(0, 1, 2), ndmin=2, dtype=np.float64)
    user_ids, users = np.unique(table[:, 0], return_inverse=True)
    item_ids, items = np.unique(table[:, 1], return_inverse=True)
    if (user_ids == np.round(user_ids)).all() and (item_ids == np.round(item_ids)).all():
        user_ids, item_ids = user_ids.astype(np.int64), item_ids.astype(np.int64)
    if (table[:, 2] != np.round(table[:, 2])).any():
        raise ValueError("positions must be integers")
    lists = _lists.RankedLists(users.reshape(-1), items.reshape(-1), table[:, 2].astype(np.int64), user_ids.size,
                               item_ids.size, depth)
    return lists, user_ids, item_ids


def rankings_risk(model, lists):
    """Extension (not in the reference): the Plackett–Luce risk of the model on ranked lists as a differentiable scalar —
    over every user the negative log-likelihood of the list as a sequence of softmax choices out of the items that
    remain, divided by the number of such choices of all users.  Returns a 0-dim fp32 tensor on the model's device;
    `.backward()` fills `model.U.grad` / `model.V.grad` (include/mfcd.h mfcd_list_pl, mfcd_ragged_gather_sum).  fp32
    models only; lists: an mfcd.lists.RankedLists on the model's device.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _lists.pl_risk(model.U, model.V, lists)


def train_model_rankings(model, lists, optimizer, device, num_steps=1000, log_every=100):
    """Extension (not in the reference): `train_model_ratings` on `rankings_risk(model, lists)` — full-batch optimiser
    steps on the Plackett–Luce risk of the ranked lists.  Returns (steps, risks) as `train_model_population` does.
    torch.optim.Adam takes the fused loop (mfcd.lists.fit_lists), any other optimiser zero_grad / rankings_risk /
    backward / step.  Not part of the result dict / .pkl layout."""
    _need_gpu(device)
    model.train()
    if _engine.fused_step_applies(model, optimizer):
        out = _lists.fit_lists(_engine.AdamBinding(model, optimizer), lists, num_steps, log_every)
    else:
        at, seen = [], []
        for t in range(int(num_steps)):
            optimizer.zero_grad()
            loss = rankings_risk(model, lists)
            loss.backward()
            optimizer.step()
            if log_every > 0 and t % log_every == 0:
                at.append(t)
                seen.append(loss.detach())
        if log_every > 0:
            with torch.no_grad():
                at.append(int(num_steps))
                seen.append(rankings_risk(model, lists))
        out = (at, torch.stack(seen).double().cpu().tolist() if seen else [])
    model.eval()
    return out


def compute_rankings_metrics(model, lists):
    """Extension (not in the reference): the model's metrics on ranked lists, typically a held-out split (`lists.split`):
    `choice_log_likelihood`, `choice_accuracy`, `uniform_log_likelihood` (the all-equal model's, in closed form) and
    `kendall_tau` among the ranked entries, each as the mean over the users and as a `_per_user` array (include/mfcd.h
    mfcd_list_pl, mfcd_pair_ragged_stats); a user whose list records no choice is NaN and stays out of the means.
    Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _lists.pl_metrics(model.U.data, model.V.data, lists)


def rankings_hvp(model, lists, dU, dV, gauss_newton=False):
    """Extension (not in the reference): `ratings_hvp` on ranked lists — the Hessian of `rankings_risk(model, lists)`
    with respect to the factor tables, applied to the direction (dU [n, d], dV [m, d]) → (HU, HV) fp32 on the model's
    device (include/mfcd.h mfcd_list_pl_hvp, per user the sum over the list's stages of diag(p) - p p^T of the softmax
    over what remains, carried to the tables by mfcd_ragged_dot and mfcd_ragged_gather_sum).  gauss_newton=True drops
    the terms that hold the risk's gradient: the product is then positive semidefinite.  fp32 models only.  Not part of
    the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _lists.pl_hvp(model.U.data, model.V.data, dU, dV, lists, gauss_newton)


def fit_users_rankings(V_or_model, lists, weight_decay, coef=None):
    """Extension (not in the reference): fold-in on ranked lists — with the item table held fixed, the vectors of the
    users of `lists` from one ranked list each: for every user the minimiser of  c * (the Plackett–Luce loss of the
    user's list) + (wd / 2) |u|^2,  started at zero (mfcd.lists_exact.lists_user_step: Newton-CG on mfcd_list_pl_hvp).
    The users need not have been in training; lists.m must be the number of rows of V.  V_or_model: a model or a bare
    fp32 V [m, d] on the GPU.  c = 1 / lists.stages, or `coef`: pass the training lists' 1 / stages so that the ridge
    weighs as it did in training.  Returns the PopulationStepResult (rows [lists.n, d], status 0 certified / 1 stopped /
    2 invalid, newton_iters, cg_iters, objective_before, objective_after, grad_ratio); a user whose list records no
    choice gets the zero row.  weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    V = V_or_model.V.data if hasattr(V_or_model, "V") and hasattr(V_or_model, "U") else V_or_model
    if not torch.is_tensor(V):
        raise TypeError("fit_users_rankings takes a model or its V table")
    _need_gpu(V.device)
    return _lists_exact.lists_user_step(None, V, lists, float(weight_decay), coef)


def refit_users_rankings(model, lists, weight_decay):
    """Extension (not in the reference): `refit_users_ratings` on ranked lists — for the model's own V, the best response
    of every user's row on  F = rankings_risk + (wd / 2)(|U|^2 + |V|^2),  the objective whose stationary points
    `train_model_rankings` approaches under Adam's coupled weight decay, by mfcd.lists_exact.lists_user_step started at
    `model.U`.  Returns (result, gain): the PopulationStepResult and, per user, gain = objective_before -
    objective_after >= 0: what the trained row still had to gain in F with V fixed.  weight_decay must be > 0.  The
    model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _lists_exact.lists_user_step(model.U.data, model.V.data, lists, float(weight_decay))
    return result, result.objective_before - result.objective_after


def refit_items_rankings(model, lists, weight_decay):
    """Extension (not in the reference): the mirror of `refit_users_rankings` — for the model's own U, the minimiser over
    all of V of F (one problem: a user's list couples its items), by mfcd.lists_exact.lists_item_step started at
    `model.V`.  Returns (result, gain) with result.rows the best-response V [m, d] and gain the 0-dim decrease of F.
    weight_decay must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.V.device)
    result = _lists_exact.lists_item_step(model.U.data, model.V.data, lists, float(weight_decay))
    return result, result.objective_before - result.objective_after


def train_model_rankings_exact(model, lists, weight_decay, sweeps=10):
    """Extension (not in the reference): `train_model_rankings` by exact block steps instead of Adam — `sweeps` sweeps of
    one exact user step and one exact item step of  F = rankings_risk + (wd / 2)(|U|^2 + |V|^2)
    (mfcd.lists_exact.fit_lists_exact), each a Newton-CG solve on the list Hessian, in place on the model's tables.
    Returns F after every sub-step as a list of [after the user step, after the item step] per sweep; it does not
    increase.  fp32 models only; weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _lists_exact.fit_lists_exact(model.U.data, model.V.data, lists, float(weight_decay), sweeps)
    model.eval()
    return result.history.cpu().tolist()


def compute_ranking_metrics(model, test, train=None, ks=(10,), min_value=None, users=None):
    """Extension (not in the reference): where the held-out ratings land in every user's ranking of the FULL catalogue —
    recall@k, precision@k, hit@k and ndcg@k for every k of `ks`, mrr, mean_rank and auc, with the items of `train` left
    out of the user's list as `recommend_items(exclude=...)` leaves them out (include/mfcd.h mfcd_rank_entries: the rank
    of every test entry among the user's admissible items, counted by integer comparisons; no row is sorted and nothing
    n x m is formed).  test, train: mfcd.ratings.RatingsData on the model's device, typically the two parts of
    `data.split`; min_value: only test entries with value >= min_value are targets, the others stay ordinary candidates.
    Returns a dict in the convention of `compute_pairwise_metrics`: every key is the mean over the users that have a
    target, every key with the suffix `_per_user` a float64 numpy array (NaN for users without one; users: None = every
    user, else user numbers, returned in that order), plus the counts `users`, `targets`, `dropped_barred` (targets that
    are in `train` themselves) and `dropped_invalid`.  auc follows the order (score, then item number) with no half
    credit for ties (mfcd.ranking.ranking_metrics has the formulas).  `model` may also be a dense GPU tensor X or a
    `FactoredMatrix`: on a table made by `observe_ratings` the truth's own ranking gives the ceiling.  Not part of the
    result dict / .pkl layout."""
    if isinstance(model, nn.Module):
        _need_gpu(model.U.device)
        model = (model.U.data, model.V.data)
    return _ranking.ranking_metrics(model, test, train, ks, min_value, users)


def implicit_positives(data, min_value=None):
    """Extension (not in the reference): the observed items of every user as the CSR pair (offsets int64 [n + 1], items
    int32) that the implicit-feedback functions take — every entry of `data` (an mfcd.ratings.RatingsData), or
    with `min_value` only the entries whose value is >= min_value: the user's other ratings are then ordinary unobserved
    items, as in `compute_ranking_metrics`.  The pair is on the table's device.  Not part of the result dict / .pkl
    layout."""
    if min_value is None:
        return data.row_off, data.item
    keep = data.value >= float(min_value)
    off = torch.zeros(data.n + 1, dtype=torch.int64, device=data.device)
    off[1:] = torch.cumsum(torch.bincount(data.user[keep].long(), minlength=data.n), 0)
    return off, data.item[keep].contiguous()


def implicit_risk(model, data, exclude=None, normalize="pairs", min_value=None):
    """Extension (not in the reference): the exact observed-versus-unobserved logistic risk of the model on implicit
    feedback as a differentiable scalar — over every user, every observed item i and ALL items j the user has not
    observed, softplus(a_j - a_i): BPR with the sampling removed, the logistic surrogate of the `auc` of
    `compute_ranking_metrics` (include/mfcd.h mfcd_implicit_rows; nothing n x m is formed).  normalize="pairs" divides
    the users' sums by the number of all pairs, normalize="user" averages every user's own mean.  exclude: items barred
    per user (an mfcd.ratings.RatingsData or a CSR pair), neither observed nor unobserved.  min_value: only ratings >=
    min_value are observed items.  Returns a 0-dim fp32 tensor on the model's device; `.backward()` fills `model.U.grad`
    / `model.V.grad`.  fp32 models only.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _implicit.implicit_risk(model.U, model.V, implicit_positives(data, min_value), exclude, normalize)


def train_model_implicit(model, data, optimizer, device, num_steps=1000, log_every=100, exclude=None, normalize="pairs",
                         min_value=None):
    """Extension (not in the reference): `train_model_ratings` on `implicit_risk(model, data, exclude, normalize)` —
    full-batch optimiser steps on the exact risk of the observed items against all unobserved ones.  Returns (steps,
    risks) as `train_model_ratings` does.  torch.optim.Adam takes the fused loop (mfcd.implicit.fit_implicit), any other
    optimiser zero_grad / implicit_risk / backward / step.  Not part of the result dict / .pkl layout."""
    _need_gpu(device)
    model.train()
    pos = implicit_positives(data, min_value)
    if _engine.fused_step_applies(model, optimizer):
        out = _implicit.fit_implicit(_engine.AdamBinding(model, optimizer), pos, num_steps, log_every, exclude, normalize)
    else:
        at, seen = [], []
        for t in range(int(num_steps)):
            optimizer.zero_grad()
            loss = _implicit.implicit_risk(model.U, model.V, pos, exclude, normalize)
            loss.backward()
            optimizer.step()
            if log_every > 0 and t % log_every == 0:
                at.append(t)
                seen.append(loss.detach())
        if log_every > 0:
            with torch.no_grad():
                at.append(int(num_steps))
                seen.append(_implicit.implicit_risk(model.U, model.V, pos, exclude, normalize))
        out = (at, torch.stack(seen).double().cpu().tolist() if seen else [])
    model.eval()
    return out


def compute_implicit_metrics(model, data, exclude=None, min_value=None):
    """Extension (not in the reference): the exact per-user `auc`, `auc_midrank` (half credit for tied pairs) and
    `log_likelihood` of the model on implicit feedback, over all (observed, unobserved) pairs of every user, with the
    counts pos, neg, inverted and tied (include/mfcd.h mfcd_implicit_rows; mfcd.implicit.implicit_metrics has the
    formulas).  Typically data is a held-out split and exclude the training split.  Every key is the mean over the
    users that have a pair, every key with the suffix `_per_user` a numpy array (NaN for a user without one).  `model`
    may also be a dense GPU tensor X or a `FactoredMatrix`.  Not part of the result dict / .pkl layout."""
    if isinstance(model, nn.Module):
        _need_gpu(model.U.device)
        model = (model.U.data, model.V.data)
    return _implicit.implicit_metrics(model, None, implicit_positives(data, min_value), exclude)


def implicit_hvp(model, data, dU, dV, exclude=None, normalize="pairs", min_value=None, gauss_newton=False):
    """Extension (not in the reference): `population_hvp` on implicit feedback — the Hessian of `implicit_risk(model, data,
    exclude, normalize)` with respect to the factor tables, applied to the direction (dU [n, d], dV [m, d]) → (HU, HV) f64
    on the model's device (include/mfcd.h mfcd_implicit_hvp_rows, the bipartite Laplacian of every user's observed-versus-
    unobserved risk, and library GEMMs per block of users; nothing n x m is formed).  gauss_newton=True drops the terms
    that hold the risk's gradient: the product is then positive semidefinite.  fp32 models only.  Not part of the result
    dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _implicit.implicit_hvp(model.U.data, model.V.data, dU, dV, implicit_positives(data, min_value), exclude, normalize,
                                  None, gauss_newton)


def fit_users_implicit(V_or_model, data, weight_decay, exclude=None, coef=None, min_value=None):
    """Extension (not in the reference): fold-in on implicit feedback — with the item table held fixed, the vectors of the
    users of `data` from their observed items alone: for every user the minimiser of  c_u * (the user's observed-versus-
    unobserved risk sum) + (wd / 2) |u|^2,  started at zero (mfcd.implicit_exact.implicit_user_step: Newton-CG on
    mfcd_implicit_hvp_rows).  The users need not have been in training; data.m must be the number of rows of V.
    V_or_model: a model or a bare fp32 V [m, d] on the GPU.  c_u = 1 / (the pairs of `data`), or `coef` (a scalar or one
    value per user): pass the training table's normaliser so that the ridge weighs as it did in training.  Returns the
    PopulationStepResult (rows [data.n, d], ready for `recommend_items`; status 0 certified / 1 stopped / 2 invalid,
    newton_iters, cg_iters, objective_before, objective_after, grad_ratio); a user without a pair gets the zero row.
    weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    V = V_or_model.V.data if hasattr(V_or_model, "V") and hasattr(V_or_model, "U") else V_or_model
    if not torch.is_tensor(V):
        raise TypeError("fit_users_implicit takes a model or its V table")
    _need_gpu(V.device)
    return _implicit_exact.implicit_user_step(None, V, implicit_positives(data, min_value), float(weight_decay), exclude,
                                              coef=coef)


def refit_users_implicit(model, data, weight_decay, exclude=None, normalize="pairs", min_value=None):
    """Extension (not in the reference): `refit_users_ratings` on implicit feedback — for the model's own V, the best
    response of every user's row on  F = implicit_risk + (wd / 2)(|U|^2 + |V|^2),  the objective whose stationary points
    `train_model_implicit` approaches under Adam's coupled weight decay, by mfcd.implicit_exact.implicit_user_step
    started at `model.U`.  Returns (result, gain): the PopulationStepResult and, per user, gain = objective_before -
    objective_after >= 0: what the trained row still had to gain in F with V fixed.  weight_decay must be > 0.  The
    model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _implicit_exact.implicit_user_step(model.U.data, model.V.data, implicit_positives(data, min_value),
                                                float(weight_decay), exclude, normalize)
    return result, result.objective_before - result.objective_after


def fold_in_users_implicit(V_or_model, data, weight_decay, exclude=None, coef=None, min_value=None):
    """Extension (not in the reference): `fit_users_implicit` in one launch — the same problem, start (zero), normaliser
    and PopulationStepResult, solved by mfcd.implicit_foldin.implicit_fold_in_users: one workgroup per user runs the whole
    damped Newton iteration with the user's d x d Hessian in LDS (include/mfcd.h mfcd_implicit_fold_in_users), d <= 64;
    the serving-time step, its rows ready for `recommend_items`.  `cg_iters` is all zeros, and a user beyond
    mfcd_implicit_fold_in_max_pos() admissible observed items or mfcd_implicit_fold_in_max_pairs() pairs gets status 3
    and a NaN row (`fit_users_implicit` takes any size).  weight_decay must be > 0.  Not part of the result dict / .pkl
    layout."""
    V = V_or_model.V.data if hasattr(V_or_model, "V") and hasattr(V_or_model, "U") else V_or_model
    if not torch.is_tensor(V):
        raise TypeError("fold_in_users_implicit takes a model or its V table")
    _need_gpu(V.device)
    return _implicit_foldin.implicit_fold_in_users(None, V, implicit_positives(data, min_value), float(weight_decay),
                                                   exclude, coef=coef)


def refit_users_implicit_kernel(model, data, weight_decay, exclude=None, normalize="pairs", min_value=None):
    """Extension (not in the reference): `refit_users_implicit` in one launch — (result, gain) with the same meaning, the
    users' best responses started at `model.U`, by mfcd.implicit_foldin.implicit_fold_in_users (d <= 64).  weight_decay
    must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _implicit_foldin.implicit_fold_in_users(model.U.data, model.V.data, implicit_positives(data, min_value),
                                                     float(weight_decay), exclude, normalize)
    return result, result.objective_before - result.objective_after


def implicit_user_information(model, data, exclude=None, min_value=None):
    """Extension (not in the reference): `user_information` on implicit feedback — for every user of `data` the d x d
    Hessian of the user's observed-versus-unobserved risk sum in the user's row at the model's tables, H_u = sum over the
    user's (observed, unobserved) pairs of sigmoid'(a_i - a_j) (v_i - v_j)(v_i - v_j)^T → mfcd.pairs.UserInformation
    (info f64 [n, d, d], weight f64 [n] the user's pairs, status int32 [n]) on the model's device (one call of
    mfcd_implicit_fold_in_users without a Newton iteration; d <= 64).  fp32 models only.  Not part of the result dict /
    .pkl layout."""
    _need_gpu(model.U.device)
    return _implicit_foldin.implicit_user_information(model.U.data, model.V.data, implicit_positives(data, min_value),
                                                      exclude)


def refit_items_implicit(model, data, weight_decay, exclude=None, normalize="pairs", min_value=None):
    """Extension (not in the reference): the mirror of `refit_users_implicit` — for the model's own U, the minimiser over
    all of V of F (one problem: a user's pairs couple the items), by mfcd.implicit_exact.implicit_item_step started at
    `model.V`.  Returns (result, gain) with result.rows the best-response V [m, d] and gain the 0-dim decrease of F.
    weight_decay must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.V.device)
    result = _implicit_exact.implicit_item_step(model.U.data, model.V.data, implicit_positives(data, min_value),
                                                float(weight_decay), exclude, normalize)
    return result, result.objective_before - result.objective_after


def train_model_implicit_exact(model, data, weight_decay, sweeps=10, exclude=None, normalize="pairs", min_value=None):
    """Extension (not in the reference): `train_model_implicit` by exact block steps instead of Adam — `sweeps` sweeps of
    one exact user step and one exact item step of  F = implicit_risk + (wd / 2)(|U|^2 + |V|^2)
    (mfcd.implicit_exact.fit_implicit_exact), each a Newton-CG solve on mfcd_implicit_hvp_rows, in place on the model's
    tables.  Returns F after every sub-step as a list of [after the user step, after the item step] per sweep; it does
    not increase.  fp32 models only; weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _implicit_exact.fit_implicit_exact(model.U.data, model.V.data, implicit_positives(data, min_value),
                                                float(weight_decay), sweeps, exclude, normalize)
    model.eval()
    return result.history.cpu().tolist()


def ratings_hvp(model, data, dU, dV, s=1.0, skip_ties=False, gauss_newton=False):
    """Extension (not in the reference): `population_hvp` on a ratings table — the Hessian of `ratings_risk(model, data,
    s, skip_ties)` with respect to the factor tables, applied to the direction (dU [n, d], dV [m, d]) → (HU, HV) fp32 on
    the model's device (include/mfcd.h mfcd_pair_ragged_hvp, the Laplacian of every user's pair risk over the items that
    user rated, carried to the tables by mfcd_ragged_dot and mfcd_ragged_gather_sum).  gauss_newton=True drops the terms
    that hold the risk's gradient: the product is then positive semidefinite.  fp32 models only.  Not part of the result
    dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _ratings.ratings_hvp(model.U.data, model.V.data, dU, dV, data, s, skip_ties, gauss_newton)


def fit_users_ratings(V_or_model, data, weight_decay, s=1.0, skip_ties=False, coef=None):
    """Extension (not in the reference): fold-in on ratings — with the item table held fixed, the vectors of the users
    of `data` from their ratings alone: for every user the minimiser of  c * (the user's all-pairs BTL risk sum) +
    (wd / 2) |u|^2,  started at zero (mfcd.ratings_exact.ratings_user_step: Newton-CG on mfcd_pair_ragged_hvp).  The
    users need not have been in training; data.m must be the number of rows of V.  V_or_model: a model or a bare fp32 V
    [m, d] on the GPU.  c = 1 / data.support(skip_ties), or `coef`: pass the training table's 1 / support so that the
    ridge weighs as it did in training.  Returns the PopulationStepResult (rows [data.n, d], status 0 certified / 1
    stopped / 2 invalid, newton_iters, cg_iters, objective_before, objective_after, grad_ratio); a user without a pair
    gets the zero row.  weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    V = V_or_model.V.data if hasattr(V_or_model, "V") and hasattr(V_or_model, "U") else V_or_model
    if not torch.is_tensor(V):
        raise TypeError("fit_users_ratings takes a model or its V table")
    _need_gpu(V.device)
    return _ratings_exact.ratings_user_step(None, V, data, s, float(weight_decay), skip_ties, coef)


def refit_users_ratings(model, data, s, weight_decay, skip_ties=False):
    """Extension (not in the reference): `refit_users_population` on a ratings table — for the model's own V, the best
    response of every user's row on  F = ratings_risk + (wd / 2)(|U|^2 + |V|^2),  the objective whose stationary points
    `train_model_ratings` approaches under Adam's coupled weight decay, by mfcd.ratings_exact.ratings_user_step started
    at `model.U`.  Returns (result, gain): the PopulationStepResult and, per user, gain = objective_before -
    objective_after >= 0: what the trained row still had to gain in F with V fixed.  weight_decay must be > 0.  The
    model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _ratings_exact.ratings_user_step(model.U.data, model.V.data, data, s, float(weight_decay), skip_ties)
    return result, result.objective_before - result.objective_after


def fold_in_users_ratings(V_or_model, data, weight_decay, s=1.0, skip_ties=False, coef=None):
    """Extension (not in the reference): `fit_users_ratings` in one launch — the same problem, start (zero), normaliser
    and PopulationStepResult, solved by mfcd.ratings_foldin.ratings_fold_in_users: one workgroup per user runs the whole
    damped Newton iteration with the user's d x d Hessian in LDS (include/mfcd.h mfcd_ratings_fold_in_users), d <= 64;
    `cg_iters` is all zeros, and a user with more ratings than mfcd_ratings_fold_in_max_len() gets status 3 and a NaN
    row (`fit_users_ratings` takes any length).  weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    V = V_or_model.V.data if hasattr(V_or_model, "V") and hasattr(V_or_model, "U") else V_or_model
    if not torch.is_tensor(V):
        raise TypeError("fold_in_users_ratings takes a model or its V table")
    _need_gpu(V.device)
    return _ratings_foldin.ratings_fold_in_users(None, V, data, s, float(weight_decay), skip_ties, coef)


def refit_users_ratings_kernel(model, data, s, weight_decay, skip_ties=False):
    """Extension (not in the reference): `refit_users_ratings` in one launch — (result, gain) with the same meaning, the
    users' best responses started at `model.U`, by mfcd.ratings_foldin.ratings_fold_in_users (d <= 64).  weight_decay
    must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _ratings_foldin.ratings_fold_in_users(model.U.data, model.V.data, data, s, float(weight_decay), skip_ties)
    return result, result.objective_before - result.objective_after


def ratings_user_information(model, data, s=1.0, skip_ties=False):
    """Extension (not in the reference): `user_information` on a ratings table — for every user of `data` the d x d
    Hessian of the user's all-pairs risk sum in the user's row at the model's tables, H_u = sum over the pairs of the
    user's items of w sigmoid'(a_e - a_l) (v_e - v_l)(v_e - v_l)^T → mfcd.pairs.UserInformation (info f64 [n, d, d],
    weight f64 [n] the user's support, status int32 [n]) on the model's device (one call of
    mfcd_ratings_fold_in_users without a Newton iteration; d <= 64).  fp32 models only.  Not part of the result dict /
    .pkl layout."""
    _need_gpu(model.U.device)
    return _ratings_foldin.ratings_user_information(model.U.data, model.V.data, data, s, skip_ties)


def refit_items_ratings(model, data, s, weight_decay, skip_ties=False):
    """Extension (not in the reference): the mirror of `refit_users_ratings` — for the model's own U, the minimiser over
    all of V of F (one problem: a user's pairs couple the items), by mfcd.ratings_exact.ratings_item_step started at
    `model.V`.  Returns (result, gain) with result.rows the best-response V [m, d] and gain the 0-dim decrease of F.
    weight_decay must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.V.device)
    result = _ratings_exact.ratings_item_step(model.U.data, model.V.data, data, s, float(weight_decay), skip_ties)
    return result, result.objective_before - result.objective_after


def train_model_ratings_exact(model, data, s, weight_decay, sweeps=10, skip_ties=False):
    """Extension (not in the reference): `train_model_ratings` by exact block steps instead of Adam — `sweeps` sweeps of
    one exact user step and one exact item step of  F = ratings_risk + (wd / 2)(|U|^2 + |V|^2)
    (mfcd.ratings_exact.fit_ratings_exact), each a Newton-CG solve on the ragged pair Hessian, in place on the model's
    tables.  Returns F after every sub-step as a list of [after the user step, after the item step] per sweep; it does
    not increase.  fp32 models only; weight_decay must be > 0.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _ratings_exact.fit_ratings_exact(model.U.data, model.V.data, data, s, float(weight_decay), sweeps, skip_ties)
    model.eval()
    return result.history.cpu().tolist()


def population_hvp(model, X, dU, dV, s=1.0, law=None, users=None, row_block=2048, gauss_newton=False):
    """Extension (not in the reference): the Hessian of `population_risk(model, X, s)` (or of `law_risk` under a
    `sampling_law`) with respect to the factor tables, applied to the direction (dU [n, d], dV [m, d]) → (HU, HV) fp32 on
    the model's device: the curvature that second-order steps on the population objective use (include/mfcd.h
    mfcd_pair_hvp_rows, the Laplacian of every user's pair risk, and library GEMMs per block of `row_block` users).
    gauss_newton=True drops the terms that hold the risk's gradient: the product is then positive semidefinite.  fp32
    models only.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _pairs.population_hvp(model.U.data, model.V.data, X, dU, dV, s, law, users, row_block, gauss_newton)


def refit_users_population(model, X, s, weight_decay, law=None, users=None, solver="cg"):
    """Extension (not in the reference): `refit_users` with unlimited comparisons — for the model's own V, the best
    response of every user's row on  F = population_risk (or law_risk) + (wd / 2)(|U|^2 + |V|^2),  the objective whose
    stationary points `train_model_population` / `train_model_law` approach under Adam's coupled weight decay, by
    mfcd.population.population_user_step started at `model.U`.  Returns (result, gain): the PopulationStepResult (rows,
    status 0 certified / 1 stopped / 2 invalid, newton_iters, cg_iters, objective_before, objective_after, grad_ratio)
    and, per user, gain = objective_before - objective_after >= 0: what the trained row still had to gain in F with V
    fixed.  weight_decay must be > 0.  The model is not changed.  solver="direct": every Newton direction from the row's
    d x d Hessian and a Cholesky solve instead of CG (d <= 256).  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _population.population_user_step(model.U.data, model.V.data, X, s, float(weight_decay), law, users,
                                              solver=solver)
    return result, result.objective_before - result.objective_after


def refit_items_population(model, X, s, weight_decay, law=None):
    """Extension (not in the reference): the mirror of `refit_users_population` — for the model's own U, the minimiser
    over all of V of F (one problem: pairs couple the items), by mfcd.population.population_item_step started at
    `model.V`.  Returns (result, gain) with result.rows the best-response V [m, d] and gain the 0-dim decrease of F.
    weight_decay must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.V.device)
    result = _population.population_item_step(model.U.data, model.V.data, X, s, float(weight_decay), law)
    return result, result.objective_before - result.objective_after


def train_model_population_exact(model, X, s, weight_decay, sweeps=10, law=None, user_solver="cg"):
    """Extension (not in the reference): `train_model_population` by exact block steps instead of Adam — `sweeps` sweeps of
    one exact user step and one exact item step of  F = population_risk (or law_risk) + (wd / 2)(|U|^2 + |V|^2)
    (mfcd.population.fit_population_exact), each a Newton-CG solve on the pair Hessian, in place on the model's tables.
    Returns F after every sub-step as a list of [after the user step, after the item step] per sweep; it does not
    increase.  fp32 models only; weight_decay must be > 0.  user_solver: "cg" or "direct", the user steps' solver
    (mfcd.population.population_user_step).  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    result = _population.fit_population_exact(model.U.data, model.V.data, X, s, float(weight_decay), sweeps, law,
                                              user_solver=user_solver)
    model.eval()
    return result.history.cpu().tolist()


def user_information(model, X, s=1.0, law=None, users=None, at="model"):
    """Extension (not in the reference): for every user the d x d matrix the pair Laplacian induces on the user's row,
    H_u = sum over the law's item pairs of w_ij sigmoid'(a_i - a_j) (v_i - v_j)(v_i - v_j)^T (include/mfcd.h
    mfcd_pair_hvp_multi_rows, one kernel pass for all d columns, and one batched GEMM) → mfcd.pairs.UserInformation
    (info f64 [k, d, d], weight f64 [k], status int32 [k]) on the model's device.  at="model": a = U[u] V^T, the Hessian of
    the user's risk sum in u; at="truth": a = s X[u], and info / weight is the Fisher information about the row that one
    comparison drawn from the law carries.  law: a `sampling_law` (None: every pair, weight 1); users=None: the law's
    users.  fp32 models only.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _pairs.user_information(model.U.data, model.V.data, X, s, law, users, at)


def strategy_information(model_or_V, X, s, num_triplets, strategies=("random", "margin", "popularity", "variance", "top_k",
                                                                     "proximity", "cluster"), users=None):
    """Extension (not in the reference): how much the comparisons of each sampling strategy say about a user's row,
    without training a model → dict strategy → f64 numpy [k, d]: per user, the ascending eigenvalues of the
    per-comparison Fisher information H_u / W_u at the truth (`user_information(..., at="truth")` under
    `sampling_law(X, num_triplets, strategy)`, with the item table of `model_or_V`: a model or V [m, d]).  NaN marks a
    user without weight (or with a non-finite row).  Which design criterion to read off — the trace of the inverse, the
    log-determinant, the smallest eigenvalue — is the caller's choice.  Not part of the result dict / .pkl layout."""
    V = model_or_V.V.data if hasattr(model_or_V, "V") else model_or_V
    _need_gpu(V.device)
    V = V.detach().float()
    U = torch.zeros((X.shape[0], V.shape[1]), dtype=torch.float32, device=V.device)     # at="truth" reads no scores of U
    out = {}
    for strategy in strategies:
        law = sampling_law(X, num_triplets, strategy, device=V.device)
        res = _pairs.user_information(U, V, X, s, law, users, "truth")
        per = res.info / res.weight[:, None, None]                                     # 0 / 0 = NaN: a user without weight
        good = torch.isfinite(per).flatten(1).all(1)
        eye = torch.eye(V.shape[1], dtype=torch.float64, device=V.device)
        eig = torch.linalg.eigvalsh(torch.where(good[:, None, None], per, eye))
        out[strategy] = torch.where(good[:, None], eig, torch.full_like(eig, float("nan"))).cpu().numpy()
    return out


def _truth_tables(model_or_V, X):
    """(U, V) fp32 on V's device for the calls that read no scores of U (at="truth")."""
    V = model_or_V.V.data if hasattr(model_or_V, "V") else model_or_V
    _need_gpu(V.device)
    V = V.detach().float()
    if hasattr(model_or_V, "U"):
        return model_or_V.U.data.detach().float(), V
    return torch.zeros((X.shape[0], V.shape[1]), dtype=torch.float32, device=V.device), V


def optimal_design(model_or_V, X, s, law=None, users=None, at="truth", prior=None):
    """Extension (not in the reference): the D-optimal comparison design of every user — the probability measure on the
    user's item pairs that maximises log det(prior + sum_p xi_p sigmoid'(a_i - a_j)(v_i - v_j)(v_i - v_j)^T), the upper
    bound `strategy_information` lacks — by pairwise Frank-Wolfe on the device (mfcd.design.user_design; include/mfcd.h
    mfcd_pair_best_rows finds the most informative pair of every user per iteration) → mfcd.design.UserDesign with the
    support `pairs`, its `weights`, the mass `rest` left on the start measure, `info`, `logdet`, and the certificate
    `gap` >= log det at the optimum - `logdet`.  model_or_V: a model, or V [m, d] (at="truth" reads no scores of U).
    law: a `sampling_law` restricts the pairs to its support and is the start measure (None: every pair).  prior: None,
    a scalar tau (tau I) or [k, d, d].  fp32 models only.  Not part of the result dict / .pkl layout."""
    U, V = _truth_tables(model_or_V, X)
    if at != "truth" and not hasattr(model_or_V, "U"):
        raise ValueError("at='model' needs a model, not a bare V")
    return _design.user_design(U, V, X, s, law, users, at, prior)


def strategy_efficiency(model_or_V, X, s, num_triplets, strategies=("random", "margin", "popularity", "variance", "top_k",
                                                                     "proximity", "cluster"), users=None, prior=None):
    """Extension (not in the reference): how far each sampling strategy's comparisons are from the most informative ones
    possible, per user → dict strategy → f64 numpy [k]: the D-efficiency exp((Phi_strategy - Phi*) / d) with
    Phi = log det(prior + per-comparison Fisher information at the truth) — Phi_strategy of the strategy's law
    (`strategy_information`'s matrix), Phi* of `optimal_design` over ALL pairs — plus the key "gap": the design's
    certificate per user.  Phi* is taken from the design found, which is at most `gap` below the optimum: the true
    efficiency lies within a factor exp(gap / d) of the reported one (reported >= true >= reported exp(-gap / d)), and
    no reported value exceeds exp(gap / d).  NaN marks a user without weight under the strategy, or an information matrix that is not positive
    definite (add a prior).  Not part of the result dict / .pkl layout."""
    U, V = _truth_tables(model_or_V, X)
    d = V.shape[1]
    best = _design.user_design(U, V, X, s, None, users, "truth", prior)
    M0 = _design._prior(prior, best.info.shape[0], d, V.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=V.device)
    out = {}
    for strategy in strategies:
        law = sampling_law(X, num_triplets, strategy, device=V.device)
        res = _pairs.user_information(U, V, X, s, law, users, "truth")
        if res.info.shape[0] != best.info.shape[0]:
            raise ValueError(f"the law of {strategy} names its own users: give `users`")
        chol, bad = torch.linalg.cholesky_ex(M0 + res.info / res.weight[:, None, None])
        phi = torch.where(bad == 0, 2.0 * chol.diagonal(dim1=1, dim2=2).log().sum(1), nan)
        out[strategy] = torch.exp((phi - best.logdet) / d).cpu().numpy()
    out["gap"] = best.gap.cpu().numpy()
    return out


def informative_pairs(model, X, k, s=1.0, law=None, users=None, prior=None):
    """Extension (not in the reference): for every user the k comparisons worth asking next — at the model's scores
    a = U[u] V^T and P = (prior + H_u)^-1, with H_u the user's information under `law` (`user_information`), the k
    anchor items i with the largest  max over j of sigmoid'(a_i - a_j)(v_i - v_j)^T P (v_i - v_j)  and each one's best
    partner j (include/mfcd.h mfcd_pair_best_rows, then mfcd_topk_rows over its values) → (i int32 [users, k],
    j int32 [users, k], score fp32 [users, k]) on the model's device, positions in the law's columns.  prior: None, a
    scalar or [users, d, d]; a user whose prior + H_u is not positive definite gets -1 / -1 / NaN.  Not part of the
    result dict / .pkl layout."""
    _need_gpu(model.U.device)
    return _design.informative_pairs(model.U.data, model.V.data, X, k, s, law, users, prior)


def _comparisons(data, n, m, device):
    """The comparisons the exact steps take → (u, i, j, z) on `device`: a DataLoader's dataset is read through
    mfcd.engine.dataset_records and packed as the training path packs it; a (u, i, j, z) tuple is taken as it is."""
    if isinstance(data, (tuple, list)) and len(data) == 4:
        return tuple(torch.as_tensor(t).reshape(-1).to(device) for t in data)
    rows = _engine.dataset_records(data.dataset if hasattr(data, "dataset") else data)
    rec = torch.from_numpy(_engine.pack_records(rows, n, m)).to(device)
    return rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3].contiguous().view(torch.float32)


def _grouped_comparisons(data, n, m, device):
    """The comparisons of `fit_users` / `refit_users` → (records, row_off, n) on `device`, grouped by user.  n = None:
    max(u) + 1."""
    u, i, j, z = _comparisons(data, n, m, device)
    if n is None:
        n = int(u.max()) + 1 if u.numel() else 0
    return _foldin.group_by_user(u, i, j, z, n) + (n,)


def fit_users(V_or_model, data, l2, U_init=None):
    """Extension (not in the reference): fold-in — with the item table held fixed, the exact minimiser of every user's
    own objective  sum over the user's comparisons of softplus(x) - z x + (l2 / 2) |u|^2,  x = u . (V[i] - V[j])  (a sum,
    not a mean; l2 > 0), by one Newton solve per user on the device (include/mfcd.h mfcd_fold_in_users; d <= 256).
    V_or_model: a model (its V and its number of users) or a bare fp32 V [m, d] on the GPU (n = max(u) + 1).  data: a
    DataLoader from `split_dataset_from_triplets`, or a tuple of (u, i, j, z) tensors; the users need not have been in
    training.  U_init: fp32 [n, d] start rows (None: 0).  Returns mfcd.foldin.FoldInResult with tensors U [n, d],
    objective [n], iters [n], status [n] (0 converged, 1 stopped, 2 invalid data) on V's device; a user without
    comparisons gets the zero row.  Not part of the result dict / .pkl layout."""
    is_model = hasattr(V_or_model, "V") and hasattr(V_or_model, "U")
    V = V_or_model.V.data if is_model else V_or_model
    if not torch.is_tensor(V):
        raise TypeError("fit_users takes a model or its V table")
    _need_gpu(V.device)
    rec, off, _ = _grouped_comparisons(data, V_or_model.U.shape[0] if is_model else None, V.shape[0], V.device)
    return _foldin.fold_in_users(V, rec, off, l2, U_init)


def refit_users(model, train_loader, weight_decay):
    """Extension (not in the reference): the exact U-step on the model's own V — `fit_users` on the training comparisons,
    warm-started from `model.U` — as a yardstick for the optimiser: how far the trained U is from the best U for the
    trained V.  The reference descends  mean over the N training records of BCE + (wd / 2)(|U|^2 + |V|^2)  (coupled L2 is
    Adam's weight_decay; structure.py:845-852 of the reference).  Multiplied by N, the part of it that depends on user
    u's row is  sum over u's records of BCE + (wd N / 2) |U[u]|^2, and BCE(sigmoid(x), z) = softplus(x) - z x, so the
    row objective of `fit_users` with  l2 = weight_decay * N  has the same minimiser.  weight_decay must be > 0.
    Returns (result, objective_at_model): the FoldInResult and, per user, the same objective at `model.U[u]` formed with
    torch ops in f64 (mfcd.foldin.row_objective).  objective_at_model - result.objective >= 0 is the diagnostic: what
    each user's row still had to gain with V fixed.  The model is not changed.  Not part of the result dict / .pkl
    layout."""
    _need_gpu(model.U.device)
    U, V = model.U.data, model.V.data
    rec, off, _ = _grouped_comparisons(train_loader, U.shape[0], V.shape[0], V.device)
    l2 = float(weight_decay) * rec.shape[0]
    result = _foldin.fold_in_users(V, rec, off, l2, U.float().contiguous())
    return result, _foldin.row_objective(U, V, rec, off, l2)


def _tables(model_or_UV, who):
    """(U, V) of a model or of a (U, V) pair of tensors."""
    if hasattr(model_or_UV, "U") and hasattr(model_or_UV, "V"):
        return model_or_UV.U.data, model_or_UV.V.data
    if isinstance(model_or_UV, (tuple, list)) and len(model_or_UV) == 2 and all(torch.is_tensor(t) for t in model_or_UV):
        return tuple(model_or_UV)
    raise TypeError(f"{who} takes a model or a (U, V) pair of tensors")


def fit_items(model_or_UV, data, l2, items=None):
    """Extension (not in the reference): fold-in for items — with U and the other items held fixed, the exact minimiser
    of an item's own objective  sum over the comparisons that hold item k of softplus(x) - z x + (l2 / 2) |V[k]|^2,
    x = U[u] . (V[i] - V[j])  (a sum, not a mean; l2 > 0), by one Newton solve per item on the device (include/mfcd.h
    mfcd_item_step at theta = 1; d <= 256), started at the item's row.  model_or_UV: a model or a (U, V) pair of fp32
    tensors on the GPU.  data: a DataLoader from `split_dataset_from_triplets`, or a tuple of (u, i, j, z) tensors.
    items: the item numbers to solve (a sequence or an integer tensor, each once; None: all m).  Several items named
    together are solved independently, each against the *given* rows of all the others — not jointly: the rows returned
    are not a joint minimiser over the named items when comparisons couple them.  An item that was not in training is a
    zero row appended to V before the call (V must have a row for every item the comparisons name).  Returns
    mfcd.foldin.ItemStepResult with tensors V [rows, d] (the solved rows, in the order of `items`), objective_start
    [rows] (the item's objective at its given row), objective [rows], iters [rows], status [rows] (0 converged, 1
    stopped, 2 invalid data); an item without comparisons gets the zero row.  Not part of the result dict / .pkl
    layout."""
    U, V = _tables(model_or_UV, "fit_items")
    _need_gpu(V.device)
    m = V.shape[0]
    u, i, j, z = _comparisons(data, U.shape[0], m, V.device)
    rec, off = _foldin.group_by_item(u, i, j, z, m)
    row_item = None
    if items is not None:
        items = torch.as_tensor(items).reshape(-1).to(device=V.device, dtype=torch.int64)
        if items.numel() and (int(items.min()) < 0 or int(items.max()) >= m):
            raise IndexError(f"an item number lies outside [0, {m})")
        if torch.unique(items).numel() != items.numel():
            raise ValueError("fit_items: an item is named twice")
        lengths = off[items + 1] - off[items]
        new_off = torch.zeros(items.numel() + 1, dtype=torch.int64, device=V.device)
        new_off[1:] = torch.cumsum(lengths, 0)
        total = int(new_off[-1])
        src = torch.arange(total, device=V.device) + torch.repeat_interleave(off[items] - new_off[:-1], lengths,
                                                                              output_size=total)
        rec, off, row_item = rec[src].contiguous(), new_off, items.to(torch.int32)
    return _foldin.fold_in_items(U.float(), V.float(), rec, off, l2, row_item, 1.0)


def refit_items(model, train_loader, weight_decay):
    """Extension (not in the reference): the exact step of every item on the model's own tables — `fit_items` on the
    training comparisons with  l2 = weight_decay * N  (the mirror of `refit_users`: the reference's objective times N,
    restricted to the terms that hold V[k]).  Returns (result, gap): the ItemStepResult and, per item,
    gap = result.objective_start - result.objective >= 0, what the item's row still had to gain with U and the other
    items fixed.  Both objectives come from the kernel's f64 sums.  Items move one at a time in this diagnostic: the gaps
    do not add up to what a joint move would gain.  weight_decay must be > 0.  The model is not changed.  Not part of
    the result dict / .pkl layout."""
    _need_gpu(model.V.device)
    u, i, j, z = _comparisons(train_loader, model.U.shape[0], model.V.shape[0], model.V.device)
    result = fit_items(model, (u, i, j, z), float(weight_decay) * u.numel())
    return result, result.objective_start - result.objective


def refit_alternating(model, train_loader, weight_decay, sweeps=10, item_steps=2):
    """Extension (not in the reference): exact-block descent of the regularised empirical objective from the trained
    tables — mfcd.alternating.fit_alternating on the training comparisons with  l2 = weight_decay * N, so that
    F = N x (mean BCE + (wd / 2)(|U|^2 + |V|^2)), N times what the reference's optimiser descends.  Each sweep is one
    exact user step and `item_steps` simultaneous half steps of all items; F falls at every sub-step.  Returns
    (result, F_at_model): the AlternatingResult (tables, F after every sub-step, statuses of the last sweep) and F at
    the model's tables; F_at_model - result.history[-1, -1] is how much of F the optimiser had left to these sweeps.
    weight_decay must be > 0.  The model is not changed.  Not part of the result dict / .pkl layout."""
    _need_gpu(model.V.device)
    U, V = model.U.data, model.V.data
    u, i, j, z = _comparisons(train_loader, U.shape[0], V.shape[0], V.device)
    result = _alternating.fit_alternating(U, V, u, i, j, z, float(weight_decay) * u.numel(), sweeps, item_steps)
    return result, result.objective_start


def refit_newton(model, train_loader, weight_decay, max_iter=100):
    """Extension (not in the reference): joint second-order descent of the regularised empirical objective from the
    trained tables — mfcd.newton.fit_newton on the training comparisons with  l2 = weight_decay * N, so that
    F = N x (mean BCE + (wd / 2)(|U|^2 + |V|^2)), N times what the reference's optimiser descends.  Both tables move at
    once, by trust-region Newton-CG on the exact Hessian-vector product of F; status 0 certifies a stationary point
    (|grad F|_inf <= 2^-26 l2 max|.|_inf).  Returns (result, F_at_model): the NewtonResult (tables, F and |grad F|_inf of
    every outer iteration, CG iterations, status) and F at the model's tables; F_at_model - result.history[-1] is how
    much of F the optimiser had left, and result.grad_inf[0] how far the model is from a stationary point of its own
    training objective.  weight_decay must be > 0; d <= 256.  The model is not changed.  Not part of the result dict /
    .pkl layout."""
    _need_gpu(model.V.device)
    U, V = model.U.data, model.V.data
    u, i, j, z = _comparisons(train_loader, U.shape[0], V.shape[0], V.device)
    result = _newton.fit_newton(U, V, u, i, j, z, float(weight_decay) * u.numel(), max_iter)
    return result, result.history[0]


def compute_ground_truth_metrics(test_loader, X, device):
    """ref:1085-1127: MSE between sigmoid(X[u,i]-X[u,j]) (no scale) and the labels, per batch, and
    the accuracy of (diff > 0).  Two-element gather per sample, once per experiment: torch ops on
    `device`, not a kernel."""
    return _ground_truth_metrics(test_loader, X)


def _ground_truth_metrics(test_loader, X, order=None):
    """compute_ground_truth_metrics; `order`: a pre-drawn (order, batch_size) of test_loader instead of drawing one."""
    rows = torch.from_numpy(_engine.dataset_records(test_loader.dataset)).to(X.device)
    order, bs = _engine.epoch_order(test_loader) if order is None else order  # same RNG draw as iterating the loader
    rows = rows[order.to(X.device)]
    u, i, j = rows[:, 0].long(), rows[:, 1].long(), rows[:, 2].long()
    z = rows[:, 3].float()
    diff = X[u, i] - X[u, j]
    se = (torch.sigmoid(diff) - z) ** 2
    total, loss_sum, nb = rows.shape[0], 0.0, 0
    for off in range(0, total, bs):
        loss_sum += se[off:off + bs].mean().item()
        nb += 1
    correct = ((diff > 0).float() == z).sum().item()
    return loss_sum / max(nb, 1), (correct / total if total > 0 else 0.0)


# ------------------------------------------------------------------------------------------------
# data (ref:465-742)
# ------------------------------------------------------------------------------------------------
_LABEL_DEVICE = None


def set_label_device(device):
    """Extension (not in the reference): draw BTL labels on `device` (a GPU) from now on; None (default) restores the
    host path, which consumes torch's CPU generator exactly like the reference."""
    global _LABEL_DEVICE
    if device is not None:
        _need_gpu(device)
    _LABEL_DEVICE = None if device is None else torch.device(device)


class BTLPreferenceDataset(Dataset):
    """ref:465-531.  `.data` is a list of (u, i, j, label) tuples.  Labels are drawn with ONE
    vectorised torch.bernoulli call over all rows, which consumes the CPU generator exactly like the
    reference's one-call-per-row loop (same serial kernel, same order).

    The rows are kept as one float64 [N, 4] array (what the device path uploads); the Python list of
    tuples behind `.data` is only built when somebody reads `.data`, and from then on that list is
    the source of truth (callers may edit or replace it, as they can with the reference's)."""

    def __init__(self, triplets, X, scale=1.0, K=1, soft_label=False, train=False):
        """With `set_label_device(device)` in force (extension; off by default) the labels are drawn and the records
        built ON that GPU (mfcd_generate_labels) — same law per label, Philox stream keyed by one int64
        taken from torch's global generator instead of the CPU Mersenne-Twister stream, so runs are reproducible but
        not bit-comparable with the reference; nothing of the dataset touches host memory unless `.data` is read."""
        self.X, self.scale, self.soft_label = X, scale, soft_label
        self._data = None
        self._dev = None
        device_labels = _LABEL_DEVICE
        if device_labels is not None:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            self._dev = _engine.generate_labels(triplets, X, scale=scale, K=K, soft=bool(soft_label and train),
                                                seed=seed, device=device_labels)
            self._rows = None
            return
        self._rows = self._label_rows(triplets, K, train)

    def _label_rows(self, triplets, K, train):
        idx = np.asarray(list(triplets) if not isinstance(triplets, (list, np.ndarray)) else triplets,
                         dtype=np.int64).reshape(-1, 3)
        if idx.shape[0] == 0:
            return np.empty((0, 4), dtype=np.float64)
        it = torch.from_numpy(idx)
        if isinstance(self.X, _gd.FactoredMatrix):     # X kept as factors (C4 / C5 sizes): entries on demand, fp32
            diff = torch.from_numpy(self.X.entries(idx[:, 0], idx[:, 1]) - self.X.entries(idx[:, 0], idx[:, 2]))
        else:
            Xc = self.X.detach()
            dev_idx = it.to(Xc.device)
            diff = (Xc[dev_idx[:, 0], dev_idx[:, 1]] - Xc[dev_idx[:, 0], dev_idx[:, 2]]).to("cpu")
        score = torch.sigmoid(self.scale * diff)                          # ref:509 (fp32, CPU op as there)
        draws = torch.bernoulli(score.repeat_interleave(K)).view(idx.shape[0], K)
        if self.soft_label and train:                                   # ref:510-513
            # torch.mean of K fp32 0/1 draws, then .item() -> Python float
            rows = np.empty((idx.shape[0], 4), dtype=np.float64)
            rows[:, :3] = idx
            rows[:, 3] = draws.mean(dim=1).double().numpy()
            return rows
        rows = np.empty((idx.shape[0] * K, 4), dtype=np.float64)         # ref:516-518: K rows per triplet
        rows[:, :3] = np.repeat(idx, K, axis=0)
        rows[:, 3] = draws.reshape(-1).double().numpy()
        return rows

    def _generate_labels(self, triplets, K, train=False):
        """ref:493-519 → list of (u, i, j, label)."""
        return self._tuples(self._label_rows(triplets, K, train))

    @staticmethod
    def _tuples(rows):
        ints = rows[:, :3].astype(np.int64)
        return list(zip(ints[:, 0].tolist(), ints[:, 1].tolist(), ints[:, 2].tolist(), rows[:, 3].tolist()))

    def _mfcd_records(self):
        """float64 [N, 4] rows for the device path, or None once `.data` has been handed out."""
        if self._rows is None and self._dev is not None and self._data is None:
            rec = self._dev.cpu().numpy()
            rows = np.empty((rec.shape[0], 4), dtype=np.float64)
            rows[:, :3] = rec[:, :3]
            rows[:, 3] = rec[:, 3].copy().view(np.float32)
            self._rows = rows
        return self._rows

    def _mfcd_device_records(self):
        """int32 [N, 4] device records when the labels were drawn on the device and `.data` was never handed out."""
        return self._dev if self._data is None else None

    @property
    def data(self):
        if self._data is None:
            self._data, self._rows = self._tuples(self._mfcd_records()), None
        return self._data

    @data.setter
    def data(self, value):
        self._data, self._rows = value, None

    def __len__(self):
        if self._data is not None:
            return len(self._data)
        return self._rows.shape[0] if self._rows is not None else self._dev.shape[0]

    def __getitem__(self, idx):
        if self._data is not None:
            return self._data[idx]
        r = self._mfcd_records()[idx]
        return (int(r[0]), int(r[1]), int(r[2]), float(r[3]))


_STRATEGIES = {
    "random": lambda X, k, ex, **kw: _gd.choose_items_random(X, num_triplets=k, exclude=ex),
    "proximity": lambda X, k, ex, **kw: _gd.choose_items_by_proximity(X, k, ex),
    "margin": lambda X, k, ex, **kw: _gd.choose_items_by_margin(X, k, ex),
    "variance": lambda X, k, ex, **kw: _gd.choose_items_by_variance(X, k, ex),
    "popularity": lambda X, k, ex, **kw: _gd.choose_items_by_popularity(
        X, k, ex, method=kw["popularity_method"], alpha=kw["alpha"]),
    "top_k": lambda X, k, ex, **kw: _gd.choose_items_top_k(X, k, ex),
    "cluster": lambda X, k, ex, **kw: _gd.choose_items_cluster_based(X, k, ex, n_clusters=kw["n_clusters"]),
    "user_similarity": lambda X, k, ex, **kw: _gd.choose_items_by_user_similarity(X, k, ex),
    "svd": lambda X, k, ex, **kw: _gd.choose_items_by_svd_projection(X, k, ex),
}


_SAMPLER_DEVICE = None


def set_sampler_device(device):
    """Extension (not in the reference): draw triplets ON `device` (a GPU; include/mfcd.h mfcd_sample_triplets) from now
    on for the strategies that have a device law (random, margin, popularity, variance, proximity, top_k, svd, cluster);
    user_similarity ("Not used" in the reference's own comments) and None (default) use the host samplers, which consume
    torch's / numpy's generators exactly like the reference.  `cluster` runs k-means on the device (mfcd/cluster.py:
    k-means++ seeded from the request's seed, Lloyd steps in HIP) where the host form calls sklearn's KMeans: the same
    law per attempt given a partition, but the partition is not sklearn's where k-means has several optima.  A
    `FactoredMatrix` ground truth is taken by random, margin, popularity, variance, proximity, top_k and cluster
    (proximity / top_k read their per-user lists from mfcd_topk_rows over the factors, variance and cluster work from
    the factors' d x d Gram forms; a dense X keeps torch.topk / torch.var and their tie order)."""
    global _SAMPLER_DEVICE
    if device is not None:
        _need_gpu(device)
    _SAMPLER_DEVICE = None if device is None else torch.device(device)


def get_triplets_from_X(X, num_triplets, strategy="random", exclude=None, popularity_method="zipf", alpha=1.5,
                        n_clusters=10):
    """ref:533-588 → set of unique (u, i, j)."""
    if strategy not in _STRATEGIES:
        raise ValueError(f"Unknown triplet sampling strategy: {strategy}")
    if _SAMPLER_DEVICE is not None and strategy in _sampling.DEVICE_STRATEGIES:
        kw = dict(popularity_method=popularity_method, alpha=alpha) if strategy == "popularity" else \
            dict(n_clusters=n_clusters) if strategy == "cluster" else {}
        rows = _sampling.sample_triplets(X, num_triplets, strategy, exclude, device=_SAMPLER_DEVICE, **kw).cpu().numpy()
        return set(zip(rows[:, 0].tolist(), rows[:, 1].tolist(), rows[:, 2].tolist()))
    found = _STRATEGIES[strategy](X, num_triplets, exclude or set(), popularity_method=popularity_method,
                                  alpha=alpha, n_clusters=n_clusters)
    return set(found)


_FACTOR_GENERATORS = ("structured", "svd", "correlated", "graph", "social", "temporal", "hierarchical", "gmm")


def generate_X(n, m, d, device, generation="base", **kwargs):
    """ref:590-663 → ground-truth preference matrix [n, m] fp32 on `device`."""
    if generation == "base":
        return _gd.generate_embeddings(n, m, d, device=device)
    if generation == "low_rank":
        A, B, S = _gd.generate_low_rank_matrix(n, m, d, rank=kwargs.get("rank", d), device=device)
        return (A * S) @ B.t()
    if generation == "clustered":
        return _gd.generate_clustered_matrix_from_embeddings(n, m, d, device=device)
    if generation in _FACTOR_GENERATORS:
        A, B = getattr(_gd, f"generate_{generation}_embeddings")(n, m, d, device=device)
        return A @ B.t()
    raise ValueError(f"Unknown generation method: {generation}")


def split_dataset_from_triplets(X, num_triplets, scale=1.0, K=1, train_ratio=0.8, val_ratio=0.1, batch_size=64,
                                strategy="random", popularity_method="zipf", alpha=1.5, soft_label=False):
    """ref:666-742 → (train_loader, val_loader, test_loader).

    With BOTH `set_sampler_device` and `set_label_device` in force (and a strategy that has a device law) the whole
    chain — triplets, the seed-42 80/10/10 split, the top-up of the test part to 500 rows, the labels and the 16-byte
    records — stays in HBM ("dataset materialisation on device"); `.data` of the datasets still yields the
    reference's list of tuples when somebody reads it."""
    if _SAMPLER_DEVICE is not None and _LABEL_DEVICE is not None and strategy in _sampling.DEVICE_STRATEGIES:
        kw = dict(popularity_method=popularity_method, alpha=alpha) if strategy == "popularity" else {}
        trip = _sampling.sample_triplets(X, num_triplets, strategy, None, device=_SAMPLER_DEVICE, **kw)
        total = trip.shape[0]
        if total < num_triplets:
            print(f"⚠️ Only {total} triplets generated for strategy: {strategy} (target={num_triplets})")
        n_train, n_val = int(train_ratio * total), int(val_ratio * total)
        order = torch.randperm(total, generator=torch.Generator().manual_seed(42)).to(trip.device)   # random_split's draw
        tr, va, te = trip[order[:n_train]], trip[order[n_train:n_train + n_val]], trip[order[n_train + n_val:]]
        if te.shape[0] * K < 500:                                                                # ref:721
            more = _sampling.sample_triplets(X, (500 + K - 1) // K - te.shape[0], strategy, trip,
                                             device=_SAMPLER_DEVICE, **kw)
            te = torch.cat((te, more))
        mk = lambda t, train: BTLPreferenceDataset(t, X, scale=scale, K=K, soft_label=soft_label, train=train)  # noqa: E731
        return (DataLoader(mk(tr, True), batch_size=batch_size, shuffle=True),
                DataLoader(mk(va, False), batch_size=batch_size, shuffle=False),
                DataLoader(mk(te, False), batch_size=batch_size, shuffle=False))
    triplets = list(get_triplets_from_X(X, num_triplets, strategy=strategy, popularity_method=popularity_method,
                                        alpha=alpha))
    if len(triplets) < num_triplets:
        print(f"⚠️ Only {len(triplets)} triplets generated for strategy: {strategy} (target={num_triplets})")
    total = len(triplets)
    n_train, n_val = int(train_ratio * total), int(val_ratio * total)
    parts = torch.utils.data.random_split(triplets, [n_train, n_val, total - n_train - n_val],
                                          generator=torch.Generator().manual_seed(42))      # ref:710-713
    tr, va, te = ([triplets[k] for k in part.indices] for part in parts)
    min_test = 500                                                                           # ref:721
    if len(te) * K < min_test:
        te = te + list(get_triplets_from_X(X, (min_test + K - 1) // K - len(te), strategy=strategy,
                                           popularity_method=popularity_method, alpha=alpha,
                                           exclude=set(tr + va + te)))
    mk = lambda t, train: BTLPreferenceDataset(t, X, scale=scale, K=K, soft_label=soft_label, train=train)  # noqa: E731
    return (DataLoader(mk(tr, True), batch_size=batch_size, shuffle=True),
            DataLoader(mk(va, False), batch_size=batch_size, shuffle=False),
            DataLoader(mk(te, False), batch_size=batch_size, shuffle=False))


# ------------------------------------------------------------------------------------------------
# experiment drivers (ref:81-450, 1154-1269): API / .pkl contract only
# ------------------------------------------------------------------------------------------------
_RESULT_KEYS = ("reconstruction_errors", "log_likelihoods", "accuracy", "gt_log_likelihoods", "gt_accuracy",
                "train_losses", "val_losses", "alpha", "norm_X", "norm_ratio", "reconstruction_error_scaled",
                "pearson_corr", "pearson_std", "spearman_corr", "spearman_std", "svd_error_scaled", "slopes",
                "pearson_corr_matrix", "spearman_corr_matrix", "reconstruction_error_scaled_per_row",
                "alpha_per_row", "sampled_UVT_rows", "sampled_X_rows")


_CONCURRENT = 1


def set_concurrent_experiments(k):
    """Extension (not in the reference): with k > 1, `run_experiment` (reps > 1) and the single-process
    `parameter_scan` run their experiments in groups of up to k: each experiment's host phase (ground truth, split,
    model init, every epoch order, the test orders and the randperm of ref:390) in the serial RNG order, then ONE
    `train_models` for the group (the models train side by side on the GPU's CUs), then each experiment's metrics.
    Results, pickles and the final torch / numpy RNG states equal the serial run's.  1 (default) is the serial path."""
    global _CONCURRENT
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"set_concurrent_experiments: k must be a positive integer (got {k!r})")
    _CONCURRENT = int(k)


class _Experiment:
    """One repetition of run_experiment between its host phase and its metrics (grouped path)."""

    def __init__(self, n, m, d, p, s, device, lr, weight_decay, num_epochs, K, strategy, popularity_method, alpha,
                 soft_label, generation):
        # ref:358-390 in the order the serial loop draws from torch's / numpy's generators
        self.s, self.device, self.num_epochs = s, device, num_epochs
        self.X = generate_X(n, m, d, device, generation=generation)
        self.loaders = split_dataset_from_triplets(self.X, int(n * m * p / 2), scale=s, K=K, strategy=strategy,
                                                   popularity_method=popularity_method, alpha=alpha,
                                                   soft_label=soft_label)
        self.model = MatrixFactorization(n, m, d).to(device)
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        train_loader, val_loader, test_loader = self.loaders
        self.orders = _engine.draw_orders(train_loader, val_loader, num_epochs)   # train_model
        self.test_order = _engine.epoch_order(test_loader)                        # evaluate_model
        self.rows = torch.randperm(self.X.shape[0])[:2]                           # ref:390
        self.gt_order = _engine.epoch_order(test_loader)                          # compute_ground_truth_metrics
        self.losses = None

    def finish(self, res):
        _need_gpu(self.device)
        model, X, test_loader = self.model, self.X, self.loaders[2]
        model.eval()
        test_loss, test_acc = _engine.evaluate(model, test_loader, order=self.test_order)
        rec_error = compute_reconstruction_error(model, X, self.s)
        m14 = compute_alpha_and_norm_ratios(model, X)
        gt_loss, gt_acc = _ground_truth_metrics(test_loader, X, self.gt_order)
        _record(res, X, model, self.losses, test_loss, test_acc, rec_error, m14, self.rows, gt_loss, gt_acc)


def _train_group(exps):
    """train_models over a group of experiments, replaying their pre-drawn epoch orders."""
    for ex in exps:
        _need_gpu(ex.device)
    models = [ex.model for ex in exps]
    for model in models:
        model.train()
    out = _engine.fit_many(models, [ex.loaders[0] for ex in exps], [ex.loaders[1] for ex in exps],
                           [ex.optimizer for ex in exps], [ex.num_epochs for ex in exps],
                           orders=[ex.orders for ex in exps])
    for ex, losses in zip(exps, out):
        ex.model.eval()
        ex.losses = losses


def _record(res, X, model, losses, test_loss, test_acc, rec_error, m14, rows, gt_loss, gt_acc):
    t_losses, v_losses = losses
    for key, val in zip(("alpha", "norm_X", "norm_ratio", "reconstruction_error_scaled", "pearson_corr",
                         "pearson_std", "spearman_corr", "spearman_std", "svd_error_scaled", "slopes",
                         "pearson_corr_matrix", "spearman_corr_matrix", "reconstruction_error_scaled_per_row",
                         "alpha_per_row"), m14):
        res[key].append(val)
    res["train_losses"].append(t_losses)
    res["val_losses"].append(v_losses)
    res["accuracy"].append(test_acc)
    res["log_likelihoods"].append(-test_loss)
    res["reconstruction_errors"].append(rec_error)
    res["gt_log_likelihoods"].append(-gt_loss)
    res["gt_accuracy"].append(gt_acc)
    res["sampled_X_rows"].append(X[rows.to(X.device)].cpu().numpy())
    res["sampled_UVT_rows"].append(_metrics.uvt_rows(model.U.data, model.V.data, rows).cpu().numpy())


def _run_grouped(jobs, k, on_done):
    """jobs: (announce, make, res, last) per experiment in serial order — announce() (or None) prints what starts,
    make() (None: no repetition) runs the experiment's host phase, res is the result dict its metrics go to, last marks
    the final repetition of a configuration (on_done() follows its metrics).  Runs them in groups of up to k."""
    for a in range(0, len(jobs), k):
        group = jobs[a:a + k]
        exps = []
        for announce, make, _, _ in group:
            if announce is not None:
                announce()
            exps.append(make() if make is not None else None)
        live = [ex for ex in exps if ex is not None]
        if live:
            _train_group(live)
        for ex, (_, _, res, last) in zip(exps, group):
            if ex is not None:
                ex.finish(res)
            if last:
                on_done()


def _experiment_jobs(res, reps, announce=None, **kw):
    make = lambda: _Experiment(**kw)   # noqa: E731
    if reps <= 0:
        return [(announce, None, res, True)]
    return [(announce if rep == 0 else None, make, res, rep == reps - 1) for rep in range(reps)]


def run_experiment(n, m, d, p, s, device, lr, weight_decay, reps=5, num_epochs=100, open_browser=False, K=1,
                   d1=None, strategy="random", popularity_method="zipf", alpha=1.5, soft_label=False,
                   generation="base"):
    """ref:306-450 → dict with the 23 keys of ref:420-444, one list entry per repetition.
    Under `set_concurrent_experiments(k)` with k > 1 the repetitions run in groups of up to k (same results)."""
    res = {k: [] for k in _RESULT_KEYS}
    if _CONCURRENT > 1 and reps > 1:
        jobs = _experiment_jobs(res, reps, n=n, m=m, d=d, p=p, s=s, device=device, lr=lr, weight_decay=weight_decay,
                                num_epochs=num_epochs, K=K, strategy=strategy, popularity_method=popularity_method,
                                alpha=alpha, soft_label=soft_label, generation=generation)
        _run_grouped(jobs, _CONCURRENT, lambda: None)
        return res
    for rep in range(reps):
        X = generate_X(n, m, d, device, generation=generation)
        loaders = split_dataset_from_triplets(X, int(n * m * p / 2), scale=s, K=K, strategy=strategy,
                                              popularity_method=popularity_method, alpha=alpha,
                                              soft_label=soft_label)
        train_loader, val_loader, test_loader = loaders
        model = MatrixFactorization(n, m, d).to(device)
        optimizer = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
        t_losses, v_losses = train_model(model, train_loader, val_loader, optimizer, device, num_epochs=num_epochs,
                                         is_last=(rep == reps - 1), open_browser=open_browser)
        test_loss, test_acc = evaluate_model(model, test_loader, device)
        rec_error = compute_reconstruction_error(model, X, s)
        m14 = compute_alpha_and_norm_ratios(model, X)
        rows = torch.randperm(X.shape[0])[:2]                                     # ref:390 (global generator)
        gt_loss, gt_acc = compute_ground_truth_metrics(test_loader, X, device)
        _record(res, X, model, (t_losses, v_losses), test_loss, test_acc, rec_error, m14, rows, gt_loss, gt_acc)
    return res


def _to_python(v):
    if isinstance(v, (np.float32, np.float64)):
        return float(v)
    if isinstance(v, np.integer):
        return int(v)
    return v


def _append_pickle(path, new_items):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    old = []
    if os.path.exists(path):
        with open(path, "rb") as f:
            old = pickle.load(f)
    old.extend(new_items)
    with open(path, "wb") as f:
        pickle.dump(old, f)
    print(f"✅ Saved {len(new_items)} new experiments to {path}")


_SCAN_KEYS = ("n", "m", "d", "p", "lr", "weight_decay", "num_epochs", "reps", "s", "K", "d1", "strategy",
              "popularity_method", "alpha", "soft_label", "generation")


def parameter_scan(n=1000, m=1000, d=2, p=0.5, s=1.0, device='cpu', lr=1e-3, weight_decay=1e-5, num_epochs=30,
                   reps=1, strategy="random", open_browser=False, linear=False, K=1, d1=None, save_path=None,
                   save_every=None, popularity_method="zipf", alpha=1.5, soft_label=False, generation="base"):
    """ref:81-255.  Scalar-or-list hyper-parameters → Cartesian product (default) or synchronised
    linear scan; each experiment yields {'params': ..., 'results': run_experiment(...)}.  With
    `save_path` the list is pickled (appending every `save_every` experiments) and, like the
    reference, the function then returns an empty list (ref:200-202)."""
    given = dict(n=n, m=m, d=d, p=p, lr=lr, weight_decay=weight_decay, num_epochs=num_epochs, reps=reps, s=s, K=K,
                 d1=d1, strategy=strategy, popularity_method=popularity_method, alpha=alpha, soft_label=soft_label,
                 generation=generation)
    grid, lists, synchronised = _normalise_grid({k: given[k] for k in _SCAN_KEYS})
    rank, world = _scan_ranks()
    if save_path and os.path.exists(save_path) and rank == 0:
        print(f"🧹 Removing existing file at {save_path}")
        os.remove(save_path)
    if not linear:
        configs = [dict(zip(grid.keys(), combo)) for combo in itertools.product(*grid.values())]
    elif synchronised:
        configs = [{k: (v[t] if len(v) > 1 else v[0]) for k, v in grid.items()} for t in range(len(lists[0]))]
    else:
        raise ValueError("The linear scan is not possible because the parameters are not synchronized.")
    def run_one(cfg, dev):
        print(f"\nRunning experiment with parameters: {cfg}")
        return run_experiment(n=cfg["n"], m=cfg["m"], d=cfg["d"], p=cfg["p"], s=cfg["s"], device=dev,
                              lr=cfg["lr"], weight_decay=cfg["weight_decay"], reps=cfg["reps"],
                              num_epochs=cfg["num_epochs"], open_browser=open_browser, K=cfg["K"], d1=cfg["d1"],
                              strategy=cfg["strategy"], popularity_method=cfg["popularity_method"],
                              alpha=cfg["alpha"], soft_label=cfg["soft_label"], generation=cfg["generation"])

    if world > 1:
        return scan_over_ranks(configs, run_one, rank, world, device, save_path, save_every)
    pending = []
    if _CONCURRENT > 1:    # experiments of consecutive configurations grouped (set_concurrent_experiments)
        jobs, done = [], []
        for cfg in configs:
            res = {k: [] for k in _RESULT_KEYS}
            kw = dict(n=cfg["n"], m=cfg["m"], d=cfg["d"], p=cfg["p"], s=cfg["s"], device=device, lr=cfg["lr"],
                      weight_decay=cfg["weight_decay"], num_epochs=cfg["num_epochs"], K=cfg["K"],
                      strategy=cfg["strategy"], popularity_method=cfg["popularity_method"], alpha=cfg["alpha"],
                      soft_label=cfg["soft_label"], generation=cfg["generation"])
            announce = lambda cfg=cfg: print(f"\nRunning experiment with parameters: {cfg}")   # noqa: E731
            jobs += _experiment_jobs(res, cfg["reps"], announce, **kw)
            done.append((cfg, res))
        finished = iter(done)

        def on_done():
            nonlocal pending
            cfg, res = next(finished)
            pending.append({"params": cfg, "results": res})
            if save_path and save_every and len(pending) >= save_every:
                _append_pickle(save_path, pending)
                pending = []
        _run_grouped(jobs, _CONCURRENT, on_done)
        if save_path and pending:
            _append_pickle(save_path, pending)
            pending = []
        return pending
    for cfg in configs:
        pending.append({"params": cfg, "results": run_one(cfg, device)})
        if save_path and save_every and len(pending) >= save_every:
            _append_pickle(save_path, pending)
            pending = []
    if save_path and pending:
        _append_pickle(save_path, pending)
        pending = []
    return pending


def _scan_ranks():
    """(rank, world) when the caller runs one process per GPU under torch.distributed, else (0, 1)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def scan_over_ranks(configs, run_one, rank, world, device, save_path=None, save_every=None, group=None):
    """the experiments of a scan are independent, so under `torchrun --nproc-per-node R` (one process
    per GPU, process group initialised by the caller) rank r runs experiments r, r+R, r+2R, ... on ITS GPU and rank 0
    collects them (one `gather_object` of plain Python results at the end; no data-path collective).  Rank 0 returns /
    pickles the list in the order of `configs`, exactly as the serial scan would; the other ranks return [].
    Not reproduced: the serial scan lets the global RNG state run on from one experiment into the next, so an experiment's
    random data here equals the serial run's only for rank 0's first experiment (seed per experiment for replay)."""
    import torch.distributed as dist
    dev = device
    if isinstance(device, str) and device == "cuda":
        dev = f"cuda:{int(os.environ.get('LOCAL_RANK', rank)) % max(torch.cuda.device_count(), 1)}"
    mine = [(k, {"params": configs[k], "results": run_one(configs[k], dev)}) for k in range(rank, len(configs), world)]
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(mine, gathered, dst=0, group=group)
    if rank != 0:
        return []
    done = [entry for _, entry in sorted((kv for part in gathered for kv in part), key=lambda kv: kv[0])]
    if not save_path:
        return done
    chunk = save_every if save_every else len(done)
    for a in range(0, len(done), max(chunk, 1)):
        _append_pickle(save_path, done[a:a + chunk])
    return []


def print_return_structure_types(obj, prefix="root"):
    """ref:258-302: debugging aid that prints the type tree of a nested result object."""
    if isinstance(obj, dict):
        for key, val in obj.items():
            print_return_structure_types(val, f"{prefix}.{key}")
    elif isinstance(obj, (list, tuple)):
        kinds = {type(e).__name__ for e in obj}
        inner = "empty" if not obj else (kinds.pop() if len(kinds) == 1 else "mixed")
        print(f"{prefix}: {type(obj).__name__}[{inner}]")
    elif isinstance(obj, torch.Tensor):
        print(f"{prefix}: torch.Tensor")
    else:
        print(f"{prefix}: {type(obj).__name__}")


def _normalise_grid(given):
    """Scalar-or-list kwargs → ({name: list}, lists_that_were_lists); NumPy scalars become Python ones (ref:128-148)."""
    grid = {}
    for key, v in given.items():
        if isinstance(v, np.ndarray):
            v = list(v)
        elif isinstance(v, list):
            v = [_to_python(x) for x in v]
        else:
            v = _to_python(v)
        grid[key] = v
    lists = [v for v in grid.values() if isinstance(v, list)]
    synchronised = len(lists) <= 1 or all(len(v) == len(lists[0]) for v in lists)
    grid = {k: (v if isinstance(v, (list, tuple)) else [v]) for k, v in grid.items()}
    return grid, lists, synchronised


def evaluate_ground_truth(n, m, p, d, s, device, K, reps=1, strategy="random", popularity_method="zipf", alpha=1.5,
                          soft_label=False, generation="base"):
    """ref:1154-1200 → (losses, accuracies) of the ground-truth matrix itself, one entry per repetition."""
    losses, accuracies = [], []
    for _ in range(reps):
        X = generate_X(n, m, d, device, generation=generation)
        _, _, test_loader = split_dataset_from_triplets(X, int(n * m * p / 2), scale=s, K=K, strategy=strategy,
                                                        popularity_method=popularity_method, alpha=alpha,
                                                        soft_label=soft_label)
        gt_loss, gt_acc = compute_ground_truth_metrics(test_loader, X, device)
        losses.append(gt_loss)
        accuracies.append(gt_acc)
    return losses, accuracies


def parameter_scan_ground_truth(n, m, p, d, s, device, K, linear=False, reps=1, strategy="random",
                                popularity_method="zipf", alpha=1.5, soft_label=False, generation="base"):
    """ref:1203-1269 → [{'params': ..., 'results': {'gt_loss': [...], 'gt_accuracy': [...]}}, ...].
    A linear scan over unsynchronised lists silently becomes a Cartesian scan, as in the reference."""
    grid, lists, synchronised = _normalise_grid(dict(n=n, m=m, p=p, d=d, s=s, K=K, strategy=strategy,
                                                     popularity_method=popularity_method, alpha=alpha,
                                                     soft_label=soft_label, generation=generation))
    if linear and synchronised:
        configs = [{k: (v[t] if len(v) > 1 else v[0]) for k, v in grid.items()} for t in range(len(lists[0]))]
    else:
        configs = [dict(zip(grid.keys(), combo)) for combo in itertools.product(*grid.values())]
    out = []
    for cfg in (_tqdm(configs, desc="Training Progress") if _tqdm is not None else configs):
        gt_loss, gt_accuracy = evaluate_ground_truth(**cfg, device=device, reps=reps)
        out.append({"params": cfg, "results": {"gt_loss": gt_loss, "gt_accuracy": gt_accuracy}})
    return out
