"""The D-optimal comparison design of every user on the device: over probability measures xi on a user's admissible
item pairs,
    maximise  Phi(xi) = log det(M0 + M(xi)),   M(xi) = sum_p xi_p s_p delta_p delta_p^T,
    s_p = sigmoid'(a_i - a_j),   delta_p = v_i - v_j,
the upper bound every sampling strategy's per-comparison information (`pairs.user_information`) is measured against.
The problem is concave; its gradient coordinate for the pair p is g_p = s_p delta_p^T P delta_p with P = (M0 + M)^-1,
and gap = max_p g_p - tr(P M) bounds Phi* - Phi(xi) from above (Kiefer-Wolfowitz), a certificate of the kind
`fold_in_users` and `fit_newton` give.

`user_design` is pairwise Frank-Wolfe, batched over the users of a row block, in f64 but for the one kernel call per
iteration: max_p g_p over all pairs of every user is `pairs.pair_best_rows` (include/mfcd.h: mfcd_pair_best_rows) on the
table G = (B - column mean) L with P = L L^T.  The algorithm is fixed (tests/design_model.py restates it):
  start     the law's own normalised information H_u / W_u of `pairs.user_information` (law None: uniform over all
            pairs), kept as ONE dense atom of mass `rest`; a weight per pair is never stored.
  iterate   1. C = M0 + M = Lc Lc^T, L = Lc^-T.  2. G, rounded to fp32 once.  3. the kernel, then the largest of
            best_val: the pair (i*, j*).  4. g* re-evaluated in f64 at that pair.  5. the held atom q (the start
            measure included) with the smallest gradient tr(P A_q).  6. mass gamma in [0, w_q] moves from q to the
            new pair; gamma maximises log det(C + gamma (A_new - A_q)) by bisection on the sign of its derivative
            phi'(gamma) = sum_k lambda_k / (1 + gamma lambda_k), lambda the eigenvalues of Lc^-1 (A_new - A_q) Lc^-T; a trial
            point that is not positive definite (some 1 + gamma lambda_k <= 0) counts as phi' < 0.
  stop      gap = g* - tr(P M) <= gtol d: status 0.  max_iter moves made: status 1, with the gap reached (no speed of
            convergence is promised).  M0 + M(start) not positive definite to f64 Cholesky: status 2, NaN outputs.
The host reads the device once per `_CHECK_EVERY` iterations.  There is no CPU form."""
import collections

import torch

from . import _lib
from . import pairs as P_
from .rows import RowBlocks

_BISECTIONS = 50
_CHECK_EVERY = 8
_G_BYTES = 128 << 20         # a row block's table G [users, k, d] (f64 product and fp32 copy, 12 bytes per entry) stays under this


class UserDesign(collections.namedtuple("UserDesign", ("pairs", "weights", "rest", "info", "logdet", "logdet_start", "gap",
                                                        "iters", "status"))):
    """What `user_design` returns, on the model's device, k users: pairs int32 [k, atoms, 2] (i < j, positions in the
    law's columns; padded with -1), weights f64 [k, atoms] (0 on the padding), rest f64 [k] (the mass left on the start
    measure), info f64 [k, d, d] = rest M(start) + sum of w A_p, logdet, logdet_start f64 [k] (of M0 + info and of
    M0 + M(start)), gap f64 [k], iters int32 [k], status int32 [k] (0 converged, 1 max_iter reached, 2 invalid)."""


def _dsigmoid(v):
    e = torch.exp(-v.abs())
    return e / (1.0 + e) ** 2


def _default_max_iter(d):
    return 100 + 25 * d


def _prior(prior, k, d, dev):
    eye = torch.eye(d, dtype=torch.float64, device=dev)
    if prior is None:
        return torch.zeros((k, d, d), dtype=torch.float64, device=dev)
    if not torch.is_tensor(prior):
        return (float(prior) * eye).expand(k, d, d)
    if tuple(prior.shape) != (k, d, d):
        raise ValueError(f"prior must be a scalar or [{k}, {d}, {d}], got {tuple(prior.shape)}")
    return prior.to(device=dev, dtype=torch.float64)


class _Block:
    """One row block's problem: scores a, truth x (fp32, restricted to the law's columns), the gathered item vectors
    B (f64, [k, d] shared or [users, k, d]), the start measure Ms and the prior M0."""

    def __init__(self, a, x, law, B, Ms, M0):
        self.a, self.x, self.law, self.B, self.Ms, self.M0 = a, x, law, B, Ms, M0
        self.a64 = a.double()
        self.Bc = B - B.mean(-2, keepdim=True)
        self.rows = torch.arange(a.shape[0], device=a.device)

    def item(self, i):
        return self.B[i] if self.B.dim() == 2 else self.B[self.rows, i]

    def best_pair(self, L):
        """The kernel's arg-max at P = L L^T → (lo, hi, found): positions i < j per user."""
        G = torch.matmul(self.Bc, L).float()
        val, arg = P_.pair_best_rows(self.a, G, self.x, self.law)
        i = val.max(dim=1)[1]
        j = arg.gather(1, i[:, None])[:, 0].long()
        found = j >= 0
        j = j.clamp_min(0)
        return torch.minimum(i, j), torch.maximum(i, j), found


def _solve_block(blk, gtol, max_iter):
    a64, Ms, M0 = blk.a64, blk.Ms, blk.M0
    n, d = Ms.shape[0], Ms.shape[1]
    dev = Ms.device
    cap = max(1, max_iter)
    eye = torch.eye(d, dtype=torch.float64, device=dev)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    _, bad = torch.linalg.cholesky_ex(M0 + Ms)
    invalid = (bad != 0) | ~torch.isfinite(Ms).flatten(1).all(1)
    Ms = torch.where(invalid[:, None, None], eye, Ms)                      # keeps the batch finite; NaN at the end
    M0 = torch.where(invalid[:, None, None], torch.zeros_like(Ms), M0)
    rest = torch.ones(n, dtype=torch.float64, device=dev)
    aw = torch.zeros((n, cap), dtype=torch.float64, device=dev)            # the atoms: mass, pair, delta, curvature
    ap = torch.full((n, cap, 2), -1, dtype=torch.int64, device=dev)
    ad = torch.zeros((n, cap, d), dtype=torch.float64, device=dev)
    asq = torch.zeros((n, cap), dtype=torch.float64, device=dev)
    cnt = torch.zeros(n, dtype=torch.int64, device=dev)
    done = invalid.clone()
    gap_out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    iters = torch.zeros(n, dtype=torch.int32, device=dev)
    it = 0
    def measure(rest, aw):                                                 # M(xi): two batched GEMM operands, nothing n x cap x d x d
        return rest[:, None, None] * Ms + (ad * (aw * asq)[:, :, None]).transpose(1, 2) @ ad

    while True:
        M = measure(rest, aw)
        Lc = torch.linalg.cholesky_ex(M0 + M)[0]
        Linv = torch.linalg.solve_triangular(Lc, eye.expand(n, d, d), upper=False)
        L = Linv.transpose(1, 2)
        P = L @ Linv
        lo, hi, found = blk.best_pair(L)
        delta = blk.item(lo) - blk.item(hi)
        s_new = _dsigmoid(a64.gather(1, lo[:, None])[:, 0] - a64.gather(1, hi[:, None])[:, 0])
        g_new = s_new * ((delta[:, None, :] @ P)[:, 0] * delta).sum(1)     # g* in f64
        gq = asq * ((ad @ P) * ad).sum(2)
        g_rest = (P * Ms).sum((1, 2))
        gap = g_new - (rest * g_rest + (aw * gq).sum(1))
        gap_out = torch.where(done, gap_out, gap)
        done = done | (gap <= gtol * d) | ~found
        if it == max_iter or (it % _CHECK_EVERY == _CHECK_EVERY - 1 and bool(done.all())):   # the host read
            break
        active = ~done
        cand = torch.cat((torch.where(aw > 0, gq, inf), torch.where(rest > 0, g_rest, inf)[:, None]), dim=1)
        q = cand.argmin(dim=1)
        from_rest = q == cap
        qc = q.clamp_max(cap - 1)[:, None]
        top = torch.where(from_rest, rest, aw.gather(1, qc)[:, 0])
        dq = ad.gather(1, qc[:, :, None].expand(n, 1, d))[:, 0]
        A_q = torch.where(from_rest[:, None, None], Ms, asq.gather(1, qc)[:, 0, None, None] * dq[:, :, None] * dq[:, None, :])
        D = s_new[:, None, None] * delta[:, :, None] * delta[:, None, :] - A_q
        D = torch.where(active[:, None, None], D, torch.zeros_like(D))
        E = Linv @ D @ L
        lam = torch.linalg.eigvalsh(0.5 * (E + E.transpose(1, 2)))

        def slope(gm):                                                     # phi'(gamma); -1 where not positive definite
            t = 1.0 + gm[:, None] * lam
            return torch.where((t > 0).all(1), (lam / t).sum(1), -torch.ones_like(gm))

        glo, ghi = torch.zeros_like(top), top.clone()
        for _ in range(_BISECTIONS):
            mid = 0.5 * (glo + ghi)
            up = slope(mid) > 0
            glo, ghi = torch.where(up, mid, glo), torch.where(up, ghi, mid)
        gm = torch.where(slope(top) >= 0, top, glo)
        gm = torch.where(active, gm, torch.zeros_like(gm))
        match = (ap[:, :, 0] == lo[:, None]) & (ap[:, :, 1] == hi[:, None])
        has = match.any(1)
        slot = torch.where(has, match.to(torch.int8).argmax(1), cnt.clamp_max(cap - 1))[:, None]
        write = active & ~has
        rest = torch.where(from_rest, rest - gm, rest)
        aw = aw.scatter_add(1, qc, torch.where(from_rest, torch.zeros_like(gm), -gm)[:, None])
        aw = aw.scatter_add(1, slot, gm[:, None])

        def put(t, value):                                                 # `value` into the slot of the rows that write
            idx = slot.reshape((n, 1) + (1,) * (t.dim() - 2)).expand((n, 1) + tuple(t.shape[2:]))
            keep = write.reshape((n,) + (1,) * (value.dim() - 1))
            return t.scatter(1, idx, torch.where(keep, value, t.gather(1, idx)[:, 0])[:, None])

        ap, ad, asq = put(ap, torch.stack((lo, hi), 1)), put(ad, delta), put(asq, s_new)
        cnt = cnt + write.to(torch.int64)
        iters = iters + active.to(torch.int32)
        it += 1
    converged = done & ~invalid & (gap_out <= gtol * d)
    status = torch.where(invalid, 2, torch.where(converged, 0, 1)).to(torch.int32)
    info = measure(rest, aw)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    logdet = 2.0 * torch.linalg.cholesky_ex(M0 + info)[0].diagonal(dim1=1, dim2=2).log().sum(1)
    logdet0 = 2.0 * torch.linalg.cholesky_ex(M0 + Ms)[0].diagonal(dim1=1, dim2=2).log().sum(1)
    order = torch.argsort((aw > 0).to(torch.int8), dim=1, descending=True, stable=True)   # the held atoms first
    aw = aw.gather(1, order)
    ap = ap.gather(1, order[:, :, None].expand(n, cap, 2))
    ap = torch.where((aw > 0)[:, :, None], ap, torch.full_like(ap, -1))
    wipe = lambda t: torch.where(invalid.reshape((n,) + (1,) * (t.dim() - 1)), nan, t)
    aw = torch.where(invalid[:, None], torch.zeros_like(aw), aw)
    ap = torch.where(invalid[:, None, None], torch.full_like(ap, -1), ap)
    return (ap.to(torch.int32), aw, wipe(rest), wipe(info), wipe(logdet), wipe(logdet0), wipe(gap_out), iters, status)


def _problem_blocks(U, V, X, s, law, users, at, row_block, what):
    """(RowBlocks, generator over its row blocks of (r0, r1, scores, truth, the block's law, B f64, H f64 [b, d, d],
    weight f64 [b])): what `pairs.user_information` forms per block — scores and truth restricted to the law's columns,
    the information matrix H_u and the law's weight W_u — and the gathered item vectors, [k, d] shared or [b, k, d]."""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (U, V)):
        raise _lib.MfcdError(f"{what} needs U and V on a GPU device (there is no CPU fallback)")
    if U.dtype != torch.float32 or V.dtype != torch.float32:
        raise _lib.MfcdError(f"{what} takes float32 factor tables")
    d = V.shape[1]
    if not 1 <= d <= P_.BEST_MAX_D:
        raise ValueError(f"a model of {d} columns is outside the range [1, {P_.BEST_MAX_D}] of {what}")
    plain = law is None or law.trivial
    k_cols = V.shape[0] if plain or law.columns is None else law.columns.shape[-1]
    if row_block is None:
        row_block = max(1, min(2048, _G_BYTES // max(1, k_cols * d * 12)))
    if plain:
        src = RowBlocks(U.detach(), V.detach(), X, users, row_block, what)
    else:
        src = P_._law_src(U.detach(), V.detach(), X, users, row_block, law, what)
    table = src.V.contiguous()
    V64 = table.double()

    def blocks():
        for r0, r1 in src.blocks():
            if plain:
                lb, truth = None, src.truth(r0, r1)
                scores = src.scores(r0, r1) if at == "model" else None
                weight = torch.full((r1 - r0,), src.m * (src.m - 1) / 2.0, dtype=torch.float64, device=src.dev)
            else:
                lb, scores, truth = P_._law_block(src, law, r0, r1)
                weight = P_.pair_law_stats_rows(truth, truth, lb, s)[1][:, 0]
            if at == "truth":
                scores = truth * float(s)
            cols = None if lb is None else lb.columns
            H = P_.pair_info_rows(scores, table, truth, lb, cols)
            yield r0, r1, scores.contiguous(), truth.contiguous(), lb, V64 if cols is None else V64[cols], H, weight

    return src, blocks()


def informative_pairs(U, V, X, k, s=1.0, law=None, users=None, prior=None, row_block=None):
    """For every user named, at the model's scores a = U[u] V^T and P = (prior + H_u)^-1 with H_u the user's information
    matrix under `law` (`pairs.user_information`, at="model"), the k anchor items with the largest
    best_val_i = max over admissible j of s_ij (v_i - v_j)^T P (v_i - v_j) and each one's partner: one
    `pairs.pair_best_rows`, then `topk.topk_rows` over its values → (i int32 [users, k], j int32 [users, k], score fp32
    [users, k]), positions in the law's columns, the best first.  A pair can appear twice, once from either end.  A user
    whose prior + H_u is not positive definite gets -1, -1, NaN."""
    from . import topk
    src, blocks = _problem_blocks(U, V, X, s, law, users, "model", row_block, "the informative pairs")
    d, dev = V.shape[1], src.dev
    M0 = _prior(prior, src.k, d, dev)
    eye = torch.eye(d, dtype=torch.float64, device=dev)
    out = []
    for r0, r1, scores, truth, lb, B, H, _ in blocks:
        C = M0[r0:r1] + H
        Lc, bad = torch.linalg.cholesky_ex(C)
        invalid = (bad != 0) | ~torch.isfinite(C).flatten(1).all(1)
        Lc = torch.where(invalid[:, None, None], eye, Lc)
        L = torch.linalg.solve_triangular(Lc, eye.expand_as(Lc), upper=False).transpose(1, 2)
        G = torch.matmul(B - B.mean(-2, keepdim=True), L).float()
        val, arg = P_.pair_best_rows(scores, G, truth, lb)
        val = torch.where(torch.isnan(val), torch.zeros_like(val), val)
        i, score = topk.topk_rows(val, k, ends="best", values=True)
        j = arg.gather(1, i.long().clamp_min(0))
        nobody = invalid[:, None] | (j < 0)
        out.append((torch.where(nobody, -1, i), torch.where(nobody, -1, j),
                    torch.where(nobody, float("nan"), score)))
    if not out:
        return (torch.zeros((0, int(k)), dtype=torch.int32, device=dev), torch.zeros((0, int(k)), dtype=torch.int32, device=dev),
                torch.zeros((0, int(k)), dtype=torch.float32, device=dev))
    return tuple(torch.cat([o[q] for o in out]) for q in range(3))


def user_design(U, V, X, s=1.0, law=None, users=None, at="truth", prior=None, gtol=1e-3, max_iter=None, row_block=None):
    """The D-optimal design of every user named (None: every user; the law's users under a law) → UserDesign.  The
    scores are those of `pairs.user_information`: at="truth", a = s X[u] (the design for learning the row from labelled
    comparisons); at="model", a = U[u] V^T.  law: the admissible pairs are the pairs the `PairLaw` gives a weight > 0,
    and the start measure is the law itself; None: every pair, uniform start.  prior: None, a scalar tau (M0 = tau I) or
    f64 [k, d, d].  gtol: stop at gap <= gtol d.  max_iter: None = 100 + 25 d.  row_block: users per batch (None: what
    keeps a batch's table G under 128 MiB).  fp32 tables on a GPU only."""
    if at not in ("model", "truth"):
        raise ValueError(f"at must be 'model' or 'truth', got {at!r}")
    if not gtol > 0:
        raise ValueError(f"gtol must be positive, got {gtol}")
    if max_iter is not None and int(max_iter) < 0:
        raise ValueError(f"max_iter must not be negative, got {max_iter}")
    src, blocks = _problem_blocks(U, V, X, s, law, users, at, row_block, "the design")
    d, dev = V.shape[1], src.dev
    max_iter = _default_max_iter(d) if max_iter is None else int(max_iter)
    M0 = _prior(prior, src.k, d, dev)
    out = []
    for r0, r1, scores, truth, lb, B, H, weight in blocks:
        blk = _Block(scores, truth, lb, B, H / weight[:, None, None], M0[r0:r1])           # 0 / 0 = NaN: no weight
        out.append(_solve_block(blk, float(gtol), max_iter))
    if not out:
        z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        return UserDesign(z(0, 0, 2, dt=torch.int32), z(0, 0), z(0), z(0, d, d), z(0), z(0), z(0), z(0, dt=torch.int32),
                          z(0, dt=torch.int32))
    parts = [torch.cat([o[q] for o in out]) for q in range(9)]             # every block has max_iter atom slots
    atoms = int((parts[1] > 0).sum(1).max())                               # the one host read of the assembly
    parts[0], parts[1] = parts[0][:, :atoms].contiguous(), parts[1][:, :atoms].contiguous()
    return UserDesign(*parts)
