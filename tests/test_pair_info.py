"""GPU tests of the multi-column pair Laplacian kernel and of what is built on it (include/mfcd.h:
mfcd_pair_hvp_multi_rows; mfcd/pairs.py: pair_hvp_multi_rows, pair_info_rows, user_information; the direct user step of
mfcd/population.py; structure.user_information, structure.strategy_information) against the float64 model of
tests/pair_info_model.py.

Shapes: m in {1, 2, 63, 64, 65, T-1, T, T+1, 2T+3} with T = pairs.INFO_TILE (the workgroup's tile of columns i; the
stage of columns j is 64, which 63, 64, 65 straddle) and d in {1, 2, 3, 31, 32, 33, 64, 65, 256} (32 columns per matrix
tile, 32 / 64 / 128 columns per workgroup, a second chunk of columns past 128): every m at d in {3, 64}, every d at m in
{65, T+1}.  Score rows: the eight kinds of test_pair_grad.case_rows; B standard normal, rounded to fp32.

Tolerance (pair_info_model.bounds): with b~ = B minus the f64 column mean of the row's gathered table, beta_ij,p =
|b~_ip| + |b~_jp| and c_ij = w_ij s_ij,
    |Z_ip - z_ip|  <=  2e-5 sum_j c_ij beta_ij,p + 2e-6 sum_j w_ij beta_ij,p,
    |H_pq - h_pq|  <=  sum over i < j of w_ij (2e-5 s_ij + 2e-6) beta_ij,p beta_ij,q
(the second follows from the first through H = B~^T Z), the project's fp32 pair tolerance applied to a sum of magnitudes
that dominates both the difference form and the centred Laplacian form term by term; deg as in test_pair_hvp.py.  A
worst-case count of the kernel's roundings lies inside it.  Per weight c_ij, relative: what test_pair_hvp.py counts for
s and the weight's product, under 12 * 2^-24 = 7e-7 (3e-6 for the row of scores in {-60, 0, 60}, whose underflowing s
the 2e-6 term covers).  b~ is rounded to fp32 once from an f64 difference: 2^-24 of |b~|, in both b~_i and b~_j.  The
matrix pipe adds the products c b~_j of a stage, at most 64, in an fp32 chain (one rounding per fused multiply-add, each
at most 2^-24 of the partial sum of magnitudes): at most 64 * 2^-24 = 3.8e-6 of sum_j c_ij |b~_j|; deg adds at most 32
terms in fp32 per lane and stage: 1.9e-6 of deg_i, which enters as deg_i |b~_i| = sum_j c_ij |b~_ip|.  The f64 sums,
the f64 product deg_i b~_i and the store add 2^-24.  Together under 7e-6 (9e-6 for the wide row) of sum_j c_ij
beta_ij,p, against 2e-5: the flush period of 64 columns is short enough.  The references are computed once per module
and shared."""
import functools

import numpy as np
import pytest
import torch

import pair_hvp_model as HM
import pair_info_model as IM
import pair_law_model as LM
from test_pair_grad import _distinct, case_rows
from test_pair_hvp import GTOL, L2, _step_law, user_minimisers
from test_pair_law import grid, law_parts, make_law, spec_of

pytestmark = pytest.mark.gpu

RTOL, ATOL = IM.RTOL, IM.ATOL
DS = [1, 2, 3, 31, 32, 33, 64, 65, 256]


def _tile():
    from mfcd import pairs
    return pairs.INFO_TILE


def _ms():
    T = _tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]


def _shapes():
    T = _tile()
    return sorted({(m, d) for m in _ms() for d in (3, 64)} | {(m, d) for m in (65, T + 1) for d in DS})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def table(m, d, offset=0.0):
    rng = np.random.default_rng(4000 + 1000 * d + m)
    return (rng.standard_normal((m, d)) + offset).astype(np.float32)


def row_weights(X, spec, r):
    if spec is None:
        return None
    lab = spec.get("labels")
    return LM.weights(X[r], spec.get("alpha"), spec.get("beta"), spec.get("margin"),
                      None if lab is None else lab[r] if np.ndim(lab) == 2 else lab)


def reference(A, X, B, spec=None, index=None):
    """(z [rows, k, d], deg [rows, k], H [rows, d, d], z_bound, H_bound) of the model; B [mB, d], index None, [k] or
    [rows, k]."""
    out = []
    for r in range(len(A)):
        Br = B if index is None else B[index[r] if np.ndim(index) == 2 else index]
        w = row_weights(X, spec, r)
        z, deg, H = IM.info_row(A[r], Br, w, None if X is None else X[r])
        zb, Hb = IM.bounds(np.nan_to_num(A[r]), np.nan_to_num(Br), w)
        out.append((z, deg, H, zb, Hb))
    return tuple(np.stack([o[q] for o in out]) for q in range(5))


@functools.lru_cache(maxsize=None)
def plain_reference(m, d, offset=0.0):
    A, X = case_rows(m)
    return reference(A, X, table(m, d, offset))


def run(dev, A, B, X=None, law=None, index=None, deg=True):
    from mfcd import pairs
    out = pairs.pair_hvp_multi_rows(to(dev, A), to(dev, B), None if X is None else to(dev, X), law,
                                    None if index is None else to(dev, index), deg)
    Z, D = out if deg else (out, None)
    rows, k = A.shape
    assert Z.dtype == torch.float32 and tuple(Z.shape) == (rows, k, B.shape[1])
    assert D is None or (D.dtype == torch.float32 and tuple(D.shape) == (rows, k))
    return (Z.cpu().numpy(), D.cpu().numpy()) if deg else (Z.cpu().numpy(),)


def info(dev, A, B, X=None, law=None, index=None):
    from mfcd import pairs
    H = pairs.pair_info_rows(to(dev, A), to(dev, B), None if X is None else to(dev, X), law,
                             None if index is None else to(dev, index))
    assert H.dtype == torch.float64 and tuple(H.shape) == (A.shape[0], B.shape[1], B.shape[1])
    return H.cpu().numpy()


def check(got, want, m, what, slack=1.0):
    """Z and deg of the kernel (and H, if given) against the model's, within `slack` times the bounds."""
    Z, D, H = got
    z, deg, h, zb, hb = want
    if m == 1:
        for t in (Z, D) + (() if H is None else (H,)):
            assert t.tobytes() == np.zeros_like(t).tobytes(), what            # exactly +0
        return
    err_z = np.abs(Z.astype(np.float64) - z)
    bound_d = RTOL * deg / (m - 1) + ATOL
    err_d = np.abs(D.astype(np.float64) - deg) / (m - 1)
    live = zb > 0
    msg = (f"{what}: z max error / bound {(err_z[live] / zb[live]).max() if live.any() else 0.0:.3f}, "
           f"deg max error / bound {(err_d / bound_d).max():.3f}")
    if H is not None:
        err_h = np.abs(H - h)
        msg += f", H max error / bound {(err_h / hb).max():.3f}, largest |H| {np.abs(h).max():.3e}"
    print(msg)
    assert (err_z <= slack * zb).all(), what
    assert (err_d <= slack * bound_d).all(), what
    if H is not None:
        assert (err_h <= slack * hb).all(), what
        assert (H == H.transpose(0, 2, 1)).all(), what                        # symmetrised: bit-equal
    dead = deg == 0                                                            # no pair of the column has weight: exactly +0
    assert Z[dead].tobytes() == np.zeros_like(Z[dead]).tobytes() and D[dead].tobytes() == np.zeros_like(D[dead]).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", _shapes())
def test_kernel_matches_the_f64_model(dev, m, d):
    A, X = case_rows(m)
    B = table(m, d)
    Z, D = run(dev, A, B)
    assert np.isfinite(Z).all() and np.isfinite(D).all()
    check((Z, D, info(dev, A, B)), plain_reference(m, d), m, f"m={m} d={d}")


@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 64)])
def test_an_offset_of_the_table_stays_within_the_same_bound(dev, m, d):
    """B + 1000, rounded to fp32 and given to both sides: the bound is centred, so it is that of a table of spread 1 (its
    entries now sit on a grid of 6e-5); a centre formed or subtracted in fp32 would miss it by orders of magnitude."""
    A, X = case_rows(m)
    B = table(m, d, 1000.0)
    assert np.abs(B).min() > 990
    want = plain_reference(m, d, 1000.0)
    assert want[4].max() <= 4 * plain_reference(m, d)[4].max()
    Z, D = run(dev, A, B)
    check((Z, D, info(dev, A, B)), want, m, f"offset m={m} d={d}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the law kinds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(65, 3), (65, 64), (_tile() + 1, 3), (_tile() + 1, 64)])
@pytest.mark.parametrize("kind", ["weights", "margin_half", "shared_labels", "row_labels", "all"])
def test_law_kernel_matches_the_f64_model(dev, kind, m, d):
    A, X = case_rows(m)
    kw, on_grid = law_parts(kind, m, 8)
    kw = dict(kw)
    X = grid(X) if on_grid else X.copy()
    if "alpha" in kw:                                           # a column whose every weight is 0
        kw["alpha"], kw["beta"] = kw["alpha"].copy(), kw["beta"].copy()
        kw["alpha"][5] = kw["beta"][5] = 0.0
    elif "margin" in kw:
        X[:, 5] = 50.0                                          # farther than the margin from every other x
    law = make_law(dev, kw, slice(0, 8))
    B = table(m, d)
    Z, D = run(dev, A, B, X, law)
    assert np.isfinite(Z).all() and np.isfinite(D).all()
    want = reference(A, X, B, spec_of(law))
    if "alpha" in kw or "margin" in kw:
        assert (want[1][:, 5] == 0).all() and (want[1] > 0).any()
    check((Z, D, info(dev, A, B, X, law)), want, m, f"{kind} m={m} d={d}")
    assert run(dev, A, B, X, law, deg=False)[0].tobytes() == Z.tobytes()
    if "margin" not in kw:                                      # X is read for finiteness only: without it, the same bits
        assert run(dev, A, B, None, law)[0].tobytes() == Z.tobytes()


@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 64)])
def test_a_law_of_ones_is_the_null_law_entry(dev, m, d):
    import ctypes
    from mfcd import _lib
    A, X = case_rows(m)
    B = table(m, d)
    plain = run(dev, A, B)
    Ad, Bd = to(dev, A), to(dev, B)
    alpha, beta = torch.ones(m, device=dev), torch.full((m,), 0.5, device=dev)  # w = 1/2 + 1/2 (PairLaw would rescale beta)
    c = _lib.PairLawC()
    c.alpha, c.beta = alpha.data_ptr(), beta.data_ptr()
    Zd, Dd = torch.empty((8, m, d), device=dev), torch.empty((8, m), device=dev)
    L = _lib.load()
    ws = _lib.workspace(L.mfcd_pair_hvp_multi_workspace_bytes(8, m, d), dev)
    _lib.check(L.mfcd_pair_hvp_multi_rows(Ad.data_ptr(), m, None, 0, Bd.data_ptr(), d, m, d, None, 0, 8, m, ctypes.byref(c),
                                          Zd.data_ptr(), d, Dd.data_ptr(), m, ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(dev)))
    ones = (Zd.cpu().numpy(), Dd.cpu().numpy())
    want = plain_reference(m, d)
    check(ones + (None,), want, m, f"law of ones m={m} d={d}")
    assert (np.abs(ones[0].astype(np.float64) - plain[0]) <= 2 * want[3]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 64)])
def test_an_index_gives_what_the_gathered_table_gives(dev, m, d):
    A, X = case_rows(m)
    rng = np.random.default_rng(60 + m)
    big = table(m + 9, d)
    shared = rng.permutation(m + 9)[:m].astype(np.int64)
    shared[7], shared[m - 1] = shared[3], shared[0]             # repeated entries
    Z, D = run(dev, A, big, index=shared)
    base = run(dev, A, np.ascontiguousarray(big[shared]))
    assert Z.tobytes() == base[0].tobytes() and D.tobytes() == base[1].tobytes()
    check((Z, D, info(dev, A, big, index=shared)), reference(A, X, big, None, shared), m, f"shared index m={m} d={d}")
    per = np.stack([rng.integers(0, m + 9, m) for _ in range(8)]).astype(np.int64)
    per[2] = shared
    Zp, Dp = run(dev, A, big, index=per)
    Hp = info(dev, A, big, index=per)
    for r in range(8):
        one = run(dev, A[r:r + 1], np.ascontiguousarray(big[per[r]]))
        assert Zp[r:r + 1].tobytes() == one[0].tobytes() and Dp[r:r + 1].tobytes() == one[1].tobytes(), r
    assert Zp[2].tobytes() == Z[2].tobytes()
    check((Zp, Dp, Hp), reference(A, X, big, None, per), m, f"per-row index m={m} d={d}")
    # an index out of range: that row is NaN (nothing is gathered through it), the others are bit-equal
    bad = per.copy()
    bad[1, 4], bad[6, m - 1] = m + 9, -1
    Zb, Db = run(dev, A, big, index=bad)
    Hb = info(dev, A, big, index=bad)
    good = [0, 2, 3, 4, 5, 7]
    assert np.isnan(Zb[[1, 6]]).all() and np.isnan(Db[[1, 6]]).all() and np.isnan(Hb[[1, 6]]).all()
    assert Zb[good].tobytes() == Zp[good].tobytes() and Db[good].tobytes() == Dp[good].tobytes()
    assert Hb[good].tobytes() == Hp[good].tobytes()
    sbad = shared.copy()
    sbad[m // 2] = 1 << 30
    assert all(np.isnan(t).all() for t in run(dev, A, big, index=sbad))         # a shared index: every row names it
    with pytest.raises(ValueError):
        run(dev, A, big)                                                        # no index: k must equal mB
    with pytest.raises(ValueError):
        run(dev, A, big, index=per[:3])


# ---------------------------------------------------------------------------------------------------------------------
# 4. consistency with the single-vector kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 33)])
def test_every_column_agrees_with_the_single_vector_kernel(dev, m, d):
    from mfcd import pairs
    A, X = case_rows(m)
    kw, _ = law_parts("weights", m, 8)
    law = make_law(dev, kw)
    B = table(m, d)
    Z, D = run(dev, A, B, X, law)
    Ad, Xd = to(dev, A), to(dev, X)
    spec = spec_of(law)
    want = reference(A, X, B, spec)
    for c in range(d):
        Y = np.tile(B[:, c], (8, 1))
        Q, Dq = pairs.pair_law_hvp_rows(Ad, Xd, to(dev, Y), law, True)
        Q, Dq = Q.cpu().numpy().astype(np.float64), Dq.cpu().numpy().astype(np.float64)
        mag = np.stack([HM.pair_hvp(A[r], Y[r], row_weights(X, spec, r))[2] for r in range(8)])
        bound_q = RTOL * mag + ATOL * (m - 1) * np.abs(Y).max(axis=1, keepdims=True)   # test_pair_hvp.check, not per term
        assert (np.abs(Z[:, :, c] - Q) <= want[3][:, :, c] + bound_q).all(), c
        assert (np.abs(D - Dq) <= 2 * (RTOL * want[1] + ATOL * (m - 1))).all(), c


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism and isolation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(65, 3), (2 * _tile() + 3, 64), (_tile() + 1, 256)])
def test_two_calls_rows_alone_strided_views_and_deg_or_not_are_bit_equal(dev, m, d):
    from mfcd import _lib, pairs
    A, X = case_rows(m)
    B = table(m, d)
    Z, D = run(dev, A, B)
    again = run(dev, A, B)
    assert again[0].tobytes() == Z.tobytes() and again[1].tobytes() == D.tobytes()
    assert run(dev, A, B, deg=False)[0].tobytes() == Z.tobytes()               # deg = NULL: the same Z
    assert run(dev, A, B, X)[0].tobytes() == Z.tobytes()                       # X without a law: finiteness only
    for r in range(8):                                                         # a row does not depend on its neighbours
        one = run(dev, A[r:r + 1], B)
        assert one[0].tobytes() == Z[r:r + 1].tobytes() and one[1].tobytes() == D[r:r + 1].tobytes(), r
    wideA = torch.full((8, m + 5), 7.0, device=dev)
    wideB = torch.full((m, d + 3), -7.0, device=dev)
    wideA[:, 2:2 + m], wideB[:, 1:1 + d] = to(dev, A), to(dev, B)
    va, vb = wideA[:, 2:2 + m], wideB[:, 1:1 + d]
    assert va.stride(0) == m + 5 and (m == 1 or vb.stride(0) == d + 3)
    sz, sd = pairs.pair_hvp_multi_rows(va, vb, deg=True)
    assert sz.cpu().numpy().tobytes() == Z.tobytes() and sd.cpu().numpy().tobytes() == D.tobytes()
    # ldz > d, ldd > k through the C entry: the same bits, and the padding is left alone
    ldz, ldd = d + 7, m + 3
    wideZ, wideD = torch.full((8, m, ldz), -123.0, device=dev), torch.full((8, ldd), -321.0, device=dev)
    L = _lib.load()
    ws = _lib.workspace(L.mfcd_pair_hvp_multi_workspace_bytes(8, m, d), dev)
    _lib.check(L.mfcd_pair_hvp_multi_rows(va.data_ptr(), va.stride(0), None, 0, vb.data_ptr(), vb.stride(0), m, d, None, 0, 8,
                                          m, None, wideZ.data_ptr(), ldz, wideD.data_ptr(), ldd, ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(dev)))
    hz, hd = wideZ.cpu().numpy(), wideD.cpu().numpy()
    assert np.ascontiguousarray(hz[:, :, :d]).tobytes() == Z.tobytes() and (hz[:, :, d:] == -123.0).all()
    assert np.ascontiguousarray(hd[:, :m]).tobytes() == D.tobytes() and (hd[:, m:] == -321.0).all()
    empty = pairs.pair_hvp_multi_rows(to(dev, A)[:0], to(dev, B), deg=True)
    assert tuple(empty[0].shape) == (0, m, d) and tuple(empty[1].shape) == (0, m)
    assert tuple(pairs.pair_info_rows(to(dev, A)[:0], to(dev, B)).shape) == (0, d, d)
    H = info(dev, A, B)
    assert info(dev, A, B).tobytes() == H.tobytes()


def test_a_non_finite_row_is_all_nan_and_its_neighbours_are_untouched(dev):
    T = _tile()
    m, d = T + 37, 5
    rng = np.random.default_rng(5)
    A = np.stack([_distinct(m, rng) for _ in range(8)])
    X = np.stack([_distinct(m, rng) for _ in range(8)])
    big = table(m + 16, d).copy()
    index = np.stack([rng.permutation(m)[:m] for _ in range(8)]).astype(np.int64)   # rows m .. m + 15 are named below only
    index[4, 9], index[5, m - 1] = m + 1, m + 2
    law = make_law(dev, dict(labels=rng.integers(0, 3, m)))                    # no margin: x is read for finiteness only
    clean = run(dev, A, big, X, law, index) + (info(dev, A, big, X, law, index),)
    assert all(np.isfinite(t).all() for t in clean)
    A[1, 3] = np.inf                                           # first tile: the second tile's workgroup must see it
    A[3, T + 30] = np.nan                                      # second tile: the first tile's workgroup must see it
    big[m + 1, d - 1] = np.nan                                 # rows of B that one user only names
    big[m + 2, 0] = -np.inf
    big[m + 3, 0] = np.nan                                     # a row of B that nobody names
    got = run(dev, A, big, X, law, index) + (info(dev, A, big, X, law, index),)
    for t, c in zip(got, clean):
        assert np.isnan(t[[1, 3, 4, 5]]).all()
        assert t[[0, 2, 6, 7]].tobytes() == c[[0, 2, 6, 7]].tobytes()
    X[6, 5] = np.nan
    X[7, T + 1] = np.inf
    got = run(dev, A, big, X, law, index) + (info(dev, A, big, X, law, index),)
    for t, c in zip(got, clean):
        assert np.isnan(t[[1, 3, 4, 5, 6, 7]]).all() and t[[0, 2]].tobytes() == c[[0, 2]].tobytes()
    want = reference(A[[0, 2]], X[[0, 2]], big, spec_of(law), index[[0, 2]])
    check(tuple(t[[0, 2]] for t in got), want, m, "neighbours of bad rows")


# ---------------------------------------------------------------------------------------------------------------------
# 6. user_information and strategy_information
# ---------------------------------------------------------------------------------------------------------------------
def check_information(res, rows, d, delta, what):
    """info / weight / status against the model's user rows.  `delta`: the largest error of a score the device forms by
    its own fp32 GEMM; it moves s_ij = sigmoid'(a_i - a_j) by at most 2 delta s_ij (|log s|' <= 1), which the bound
    carries as 2e-5 + 2 delta in place of 2e-5."""
    info, weight, status = (t.cpu().numpy() for t in res)
    assert info.dtype == np.float64 and info.shape == (len(rows), d, d) and status.dtype == np.int32
    for r, (a, B, w, x, W) in enumerate(rows):
        h = IM.info_row(a, B, w, x)[2]
        hb = IM.bounds(a, B, w)[1] * (1.0 + 2.0 * delta / RTOL)
        err = np.abs(info[r] - h)
        print(f"{what} user row {r}: H max error / bound {(err / hb).max():.3f}, W {W}")
        assert (err <= hb).all() and status[r] == 0, (what, r)
        np.testing.assert_allclose(weight[r], W, rtol=1e-6)


@pytest.mark.parametrize("shape", ["n12_m40_d3", "n5_mT5_d2"])
def test_user_information_matches_the_model(dev, shape):
    import structure as S
    from mfcd import pairs
    n, m, d = (12, 40, 3) if shape == "n12_m40_d3" else (5, _tile() + 5, 2)
    rng = np.random.default_rng(41)
    U = rng.standard_normal((n, d)).astype(np.float32)
    V = rng.standard_normal((m, d)).astype(np.float32)
    X = rng.standard_normal((n, m)).astype(np.float32)
    s = 0.7
    model = S.MatrixFactorization(n, m, d).to(dev)
    with torch.no_grad():
        model.U.copy_(to(dev, U))
        model.V.copy_(to(dev, V))
    Xd = to(dev, X)
    delta = (d + 1) * 2.0 ** -24 * (np.abs(U) @ np.abs(V).T).max()             # an fp32 dot product of d terms
    k = 7
    cols = np.stack([rng.permutation(m)[:k] for _ in range(n)])
    cols[1, 3] = cols[1, 0]                                                     # a column named twice
    law = pairs.PairLaw(alpha=rng.uniform(0.2, 1.0, k), beta=rng.uniform(0.2, 1.0, k), labels=rng.integers(0, 3, (n, k)),
                        columns=cols, users=[0, 2, n - 1], device=dev)
    users = [n - 1, 0, 2, n - 1, 1]
    for at in ("model", "truth"):
        dl = delta if at == "model" else 0.0
        res = S.user_information(model, Xd, s, at=at)
        check_information(res, IM.user_rows(U, V, X, s, None, None, at), d, dl, f"{shape} plain at={at}")
        sub = pairs.user_information(model.U.data, model.V.data, Xd, s, None, users, at, row_block=2)
        check_information(sub, IM.user_rows(U, V, X, s, None, users, at), d, dl, f"{shape} users at={at}")
        assert torch.equal(sub.info[0], sub.info[3])                            # a user named twice, in two blocks
        got = S.user_information(model, Xd, s, law, at=at)
        check_information(got, IM.user_rows(U, V, X, s, spec_of(law), None, at), d, dl, f"{shape} law at={at}")
    # at="truth" is at="model" when U V^T = s X exactly in fp32: integer tables, s a power of two
    Ui = rng.integers(-2, 3, (n, d)).astype(np.float32)
    Vi = rng.integers(-2, 3, (m, d)).astype(np.float32)
    Xi = to(dev, (Ui @ Vi.T) * 4.0)
    a_model = pairs.user_information(to(dev, Ui), to(dev, Vi), Xi, 0.25, law, at="model")
    a_truth = pairs.user_information(to(dev, Ui), to(dev, Vi), Xi, 0.25, law, at="truth")
    assert all(torch.equal(p, q) for p, q in zip(a_model, a_truth))
    # status 2 isolates a bad row
    Xbad = Xd.clone()
    Xbad[2, 1] = float("nan")
    clean = S.user_information(model, Xd, s)
    bad = S.user_information(model, Xbad, s)
    others = [u for u in range(n) if u != 2]
    assert bad.status.tolist() == [2 if u == 2 else 0 for u in range(n)] and bool(torch.isnan(bad.info[2]).all())
    assert torch.equal(bad.info[others], clean.info[others])


def test_strategy_information_is_the_spectrum_of_the_models_information(dev):
    import structure as S
    n, m, d, s, N = 6, 40, 3, 0.7, 500
    rng = np.random.default_rng(17)
    V = rng.standard_normal((m, d)).astype(np.float32)
    X = rng.standard_normal((n, m)).astype(np.float32)
    Xd, Vd = to(dev, X), to(dev, V)
    out = S.strategy_information(Vd, Xd, s, N, strategies=("random", "popularity", "top_k"))
    assert list(out) == ["random", "popularity", "top_k"]
    U0 = np.zeros((n, d), dtype=np.float32)
    for strategy, eig in out.items():
        assert eig.dtype == np.float64 and eig.shape == (n, d)
        law = S.sampling_law(Xd, N, strategy, device=dev)
        spec = None if law.trivial else spec_of(law)
        for r, (a, B, w, x, W) in enumerate(IM.user_rows(U0, V, X, s, spec, None, "truth")):
            if strategy == "random":
                assert W == m * (m - 1) // 2
            want = np.linalg.eigvalsh(IM.info_row(a, B, w, x)[2] / W)
            tol = np.linalg.norm(IM.bounds(a, B, w)[1]) / W                    # Weyl: |d lambda| <= |E|_2 <= |E|_F
            print(f"{strategy} user {r}: eigenvalues {np.round(eig[r], 6).tolist()}, max error / bound "
                  f"{np.abs(eig[r] - want).max() / tol:.3f}")
            assert (np.abs(eig[r] - want) <= tol).all() and (np.diff(eig[r]) >= 0).all()
    model = S.MatrixFactorization(n, m, d).to(dev)
    with torch.no_grad():
        model.V.copy_(Vd)
    np.testing.assert_allclose(S.strategy_information(model, Xd, s, N, strategies=("random",), users=[4, 1])["random"],
                               out["random"][[4, 1]], rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the direct user step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_law", [False, True], ids=["plain", "law"])
@pytest.mark.parametrize("m", [40, 1029])
def test_direct_user_step_reaches_the_models_minimiser(dev, m, with_law):
    """test_pair_hvp.test_user_step_reaches_the_models_minimiser with solver="direct": the same inputs, certificate and
    distances."""
    from mfcd import population
    Ustar, V, X = HM.solver_inputs(m)
    prob, Uopt, noise = user_minimisers(m, with_law)
    law = _step_law(m, dev) if with_law else None
    U0, Vd, Xd = torch.zeros(8, 3, device=dev), to(dev, V), to(dev, X)
    res = population.population_user_step(U0, Vd, Xd, 1.0, L2, law, solver="direct")
    rows = res.rows.cpu().numpy().astype(np.float64)
    assert res.rows.dtype == torch.float32 and res.status.tolist() == [0] * 8
    assert res.cg_iters.tolist() == [0] * 8
    V64 = V.astype(np.float64)
    gnorm = np.array([np.linalg.norm(prob.user_grad(rows[r], V64, r, L2)) for r in range(8)])
    bound = GTOL * L2 * np.abs(rows).max(axis=1) + noise
    dist = np.linalg.norm(rows - Uopt, axis=1)
    print(f"m={m} law={with_law}: Newton {res.newton_iters.tolist()}, |grad| / bound {np.round(gnorm / bound, 3).tolist()}, "
          f"|u - u*| / (bound / l2) {np.round(dist / (bound / L2), 3).tolist()}")
    assert (gnorm <= bound).all()
    assert (dist <= bound / L2).all()                            # strong convexity, modulus l2
    before, after = res.objective_before.cpu().numpy(), res.objective_after.cpu().numpy()
    assert (after <= before).all() and (res.grad_ratio.cpu().numpy() <= GTOL).all()
    f_model = np.array([prob.user_objective(rows[r], V64, r, L2) for r in range(8)])
    np.testing.assert_allclose(after, f_model, rtol=RTOL, atol=ATOL)
    # a user with a NaN truth row: status 2, a NaN row; its neighbours as without it
    Xbad = Xd.clone()
    Xbad[3, m // 2] = float("nan")
    bad = population.population_user_step(U0, Vd, Xbad, 1.0, L2, law, solver="direct")
    others = [0, 1, 2, 4, 5, 6, 7]
    assert bad.status.tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and bool(torch.isnan(bad.rows[3]).all())
    if not with_law:
        base, pick = res, others
    else:
        base = population.population_user_step(U0, Vd, Xd, 1.0, L2, law, users=others, solver="direct")
        pick = list(range(7))
    got, want = bad.rows[others].cpu().numpy(), base.rows[pick].cpu().numpy()
    if with_law:                                                 # 1 / sum W of seven users: see the test this one mirrors
        np.testing.assert_array_max_ulp(got, want, maxulp=4)
    else:
        assert got.tobytes() == want.tobytes()
    assert bad.newton_iters[others].tolist() == base.newton_iters[pick].tolist()
    np.testing.assert_allclose(bad.objective_after[others].cpu().numpy(), base.objective_after[pick].cpu().numpy(),
                               rtol=1e-6 if with_law else 0, atol=0)
    assert (bad.grad_ratio[others].cpu().numpy() <= GTOL).all() and (base.grad_ratio[pick].cpu().numpy() <= GTOL).all()
    assert base.status[pick].tolist() == [0] * 7
    assert bad.cg_iters.tolist() == [0] * 8


def test_direct_sweep_descends_and_reaches_the_cg_sweeps_objective(dev):
    import structure as S
    from mfcd import population
    Ustar, V, X = HM.solver_inputs(40)
    rng = np.random.default_rng(8)
    U0 = (0.3 * rng.standard_normal((8, 3))).astype(np.float32)
    V0 = (0.3 * rng.standard_normal((40, 3))).astype(np.float32)
    Xd = to(dev, X)
    cg = population.fit_population_exact(to(dev, U0), to(dev, V0), Xd, 1.0, L2, 1)
    direct = population.fit_population_exact(to(dev, U0), to(dev, V0), Xd, 1.0, L2, 1, user_solver="direct")
    start, hist = float(direct.objective_start), direct.history[0].tolist()
    print(f"F: start {start:.7f}, direct {np.round(hist, 7).tolist()}, cg {np.round(cg.history[0].tolist(), 7).tolist()}")
    assert float(cg.objective_start) == start and hist[0] <= start and hist[1] <= hist[0]
    assert direct.user_status.tolist() == [0] * 8
    np.testing.assert_allclose(hist, cg.history[0].tolist(), rtol=RTOL, atol=ATOL)
    prob = HM.Problem(X, 1.0)
    Un, Vn = (t.cpu().numpy().astype(np.float64) for t in (direct.U, direct.V))
    np.testing.assert_allclose(hist[1], prob.objective(Un, Vn, L2), rtol=RTOL, atol=ATOL)
    model = S.MatrixFactorization(8, 40, 3).to(dev)
    with torch.no_grad():
        model.U.copy_(to(dev, U0))
        model.V.copy_(to(dev, V0))
    np.testing.assert_allclose(S.train_model_population_exact(model, Xd, 1.0, L2, sweeps=1, user_solver="direct"), [hist],
                               rtol=1e-9)
    refit, gain = S.refit_users_population(model, Xd, 1.0, L2, solver="direct")
    assert refit.cg_iters.tolist() == [0] * 8 and bool((gain >= 0).all())
    with pytest.raises(ValueError):
        population.population_user_step(torch.zeros(8, 257, device=dev), torch.zeros(40, 257, device=dev), Xd, 1.0, L2,
                                        solver="direct")
