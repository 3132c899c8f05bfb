"""GPU tests of the pair arg-max kernel (include/mfcd.h: mfcd_pair_best_rows; mfcd/pairs.py: pair_best_rows) against the
float64 model of tests/pair_best_model.py.

Shapes: m in {1, 2, 65, T+1, 2T+3} with T = pairs.BEST_TILE (the workgroup's tile of columns i; the stage of columns j is
64) and d in {1, 3, 33, 64, 256} (the kernel's K chunks are 4, 32, 64, 128 and 2 x 128 columns): every m at d in {3, 64},
every d at m in {65, T+1}.  Score rows: the eight kinds of test_pair_grad.case_rows; tables standard normal, fp32.

Tolerance (pair_best_model.scores): E_ij = (2e-5 s_ij + 2e-6) sum_p (|g_ip| + |g_jp|)^2, the project's fp32 pair tolerance
applied to a sum of magnitudes that dominates both the difference form and the Gram form.  A count of the kernel's
roundings lies inside it: s as in test_pair_hvp.py, under 12 * 2^-24 = 7e-7 relative (the 2e-6 term covers an
underflowing s); the matrix pipe adds the d products of g_i . g_j in an fp32 chain, at most d * 2^-24 of
sum_p |g_ip g_jp| <= sum_p (|g_ip| + |g_jp|)^2 / 4, doubled by the factor 2: at most 256 * 2^-24 / 2 = 7.6e-6 of the
magnitude sum at d = 256; the two norms, their sum, the fused n - 2 dot and the product with s add 5 * 2^-24.  The
kernel's choice is held to the same bound: with (val, j) the kernel's,
    j is admissible and != i,   |val - S64[i, j]| <= E[i, j],   S64[i, j] >= max_j' (S64[i, j'] - E[i, j']) - E[i, j],
with no near-tie exclusions.  The references are computed once per module and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pair_best_model as BM
from test_pair_grad import case_rows
from test_pair_info import row_weights, to
from test_pair_law import grid, law_parts, make_law, spec_of

pytestmark = pytest.mark.gpu

DS = [1, 3, 33, 64, 256]


def _tile():
    from mfcd import pairs
    return pairs.BEST_TILE


def _ms():
    T = _tile()
    return [1, 2, 65, T + 1, 2 * T + 3]


def _shapes():
    T = _tile()
    return sorted({(m, d) for m in _ms() for d in (3, 64)} | {(m, d) for m in (65, T + 1) for d in DS})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def tables(m, d):
    """[8, m, d] fp32: one table per row; the first is also the shared one."""
    return np.random.default_rng(5000 + 1000 * d + m).standard_normal((8, m, d)).astype(np.float32)


def reference(A, X, G, spec=None):
    """[(S64, E, adm)] per row; G [m, d] or [rows, m, d]."""
    return [BM.scores(np.nan_to_num(A[r]), G[r] if G.ndim == 3 else G, row_weights(X, spec, r)) for r in range(len(A))]


@functools.lru_cache(maxsize=None)
def plain_reference(m, d, per_row):
    A, X = case_rows(m)
    return reference(A, X, tables(m, d) if per_row else tables(m, d)[0])


def run(dev, A, G, X=None, law=None):
    from mfcd import pairs
    val, arg = pairs.pair_best_rows(to(dev, A), to(dev, G), None if X is None else to(dev, X), law)
    assert val.dtype == torch.float32 and arg.dtype == torch.int32 and tuple(val.shape) == A.shape == tuple(arg.shape)
    return val.cpu().numpy(), arg.cpu().numpy()


def check(got, want, what):
    """The kernel's (val, j) of every row against the model's scores, within the bound E."""
    val, arg = got
    worst_v, worst_c = 0.0, -np.inf
    for r, (S64, E, adm) in enumerate(want):
        k = S64.shape[0]
        has = adm.any(axis=1)
        none = ~has
        assert (arg[r][none] == -1).all() and val[r][none].tobytes() == np.zeros(none.sum(), np.float32).tobytes(), what
        i = np.flatnonzero(has)
        j = arg[r][i].astype(np.int64)
        assert ((j >= 0) & (j < k) & (j != i)).all() and adm[i, j].all(), f"{what} row {r}: an inadmissible partner"
        err = np.abs(val[r][i].astype(np.float64) - S64[i, j])
        top = np.where(adm, S64 - E, -np.inf).max(axis=1)[i]
        short = top - E[i, j] - S64[i, j]
        worst_v = max(worst_v, (err / E[i, j]).max(initial=0.0))
        worst_c = max(worst_c, (short / E[i, j]).max(initial=-np.inf))
        assert (err <= E[i, j]).all(), f"{what} row {r}: value error / bound {(err / E[i, j]).max():.3f}"
        assert (short <= 0).all(), f"{what} row {r}: the chosen pair is short of the best by {(short / E[i, j]).max():.3f} bounds"
    print(f"{what}: value error / bound {worst_v:.3f}, choice shortfall / bound {worst_c:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("m,d", _shapes())
def test_kernel_matches_the_f64_model(dev, m, d, per_row):
    A, X = case_rows(m)
    G = tables(m, d) if per_row else tables(m, d)[0]
    val, arg = run(dev, A, G)
    assert np.isfinite(val).all()
    check((val, arg), plain_reference(m, d, per_row), f"m={m} d={d} per_row={per_row}")
    if m == 1:
        assert (arg == -1).all() and val.tobytes() == np.zeros_like(val).tobytes()
    withx = run(dev, A, G, X)                                   # X is read for finiteness only
    assert withx[0].tobytes() == val.tobytes() and withx[1].tobytes() == arg.tobytes()


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "per_row"])
@pytest.mark.parametrize("m,d", [(65, 3), (65, 64), (_tile() + 1, 3), (_tile() + 1, 64)])
@pytest.mark.parametrize("kind", ["weights", "margin_half", "shared_labels", "row_labels", "all"])
def test_law_kernel_matches_the_f64_model(dev, kind, m, d, per_row):
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
    G = tables(m, d) if per_row else tables(m, d)[0]
    val, arg = run(dev, A, G, X, law)
    want = reference(A, X, G, spec_of(law))
    if "alpha" in kw or "margin" in kw:                         # the column without an admissible partner: +0 / -1
        assert not any(adm[5].any() for _, _, adm in want) and (arg[:, 5] == -1).all()
        assert val[:, 5].tobytes() == np.zeros(8, np.float32).tobytes()
    assert any((adm.sum(axis=1) < m - 1).any() and adm.any() for _, _, adm in want)      # the law does exclude pairs
    check((val, arg), want, f"{kind} m={m} d={d} per_row={per_row}")
    if "margin" not in kw:                                      # X is read for finiteness only: without it, the same bits
        bare = run(dev, A, G, None, law)
        assert bare[0].tobytes() == val.tobytes() and bare[1].tobytes() == arg.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. exact ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 3), (2 * _tile() + 3, 3), (_tile() + 1, 64), (65, 256)])
def test_ties_go_to_the_smallest_j_exactly(dev, m, d):
    """A constant score row (s = 1/4 exactly) and a table of small integers: every product, norm and score is exact in
    fp32, many columns share their maximum, and value and index equal the model bit for bit."""
    rng = np.random.default_rng(300 + m + d)
    A = np.full((2, m), 0.75, dtype=np.float32)
    G = rng.integers(-2, 3, (2, m, d)).astype(np.float32)
    G[1, :, 1:] = 0.0                                           # one live column: ties everywhere
    val, arg = run(dev, A, G)
    for r in range(2):
        S64, _, adm = BM.scores(A[r], G[r])
        v, j = BM.best(S64, adm)
        ties = int((np.isclose(S64, v[:, None]) & adm).sum(axis=1).max())
        assert ties >= 2 or r == 0                              # the table with one live column ties at any d
        assert val[r].tobytes() == v.astype(np.float32).tobytes() and (v.astype(np.float32) == v).all(), f"row {r}"
        assert (arg[r] == j).all(), f"row {r}: {np.flatnonzero(arg[r] != j)[:5]}"


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism, independence of the rows, leading dimensions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 64), (2 * _tile() + 3, 33)])
def test_rows_are_deterministic_and_independent(dev, m, d):
    from mfcd import _lib, pairs
    A, X = case_rows(m)
    G = tables(m, d)
    base = run(dev, A, G)
    again = run(dev, A, G)
    assert base[0].tobytes() == again[0].tobytes() and base[1].tobytes() == again[1].tobytes()
    for r in (0, 7):                                            # a row alone
        one = run(dev, A[r:r + 1], G[r:r + 1])
        assert one[0].tobytes() == base[0][r:r + 1].tobytes() and one[1].tobytes() == base[1][r:r + 1].tobytes()
    perm = np.random.default_rng(1).permutation(8)              # another place in the call
    moved = run(dev, A[perm], G[perm])
    assert moved[0].tobytes() == base[0][perm].tobytes() and moved[1].tobytes() == base[1][perm].tobytes()
    wide = torch.zeros((8, m + 13), device=dev)                 # a strided view of the scores
    wide[:, 3:3 + m] = to(dev, A)
    v, j = pairs.pair_best_rows(wide[:, 3:3 + m], to(dev, G))
    assert v.cpu().numpy().tobytes() == base[0].tobytes() and j.cpu().numpy().tobytes() == base[1].tobytes()
    # the entry itself with every leading dimension larger than it has to be: columns >= m stay as they were
    L = _lib.load()
    ldg, ldv, ldj, stride = d + 3, m + 5, m + 7, m * (d + 3) + 11
    Gw = torch.full((8 * stride,), 7.0, device=dev)
    Gw.as_strided((8, m, d), (stride, ldg, 1)).copy_(to(dev, G))
    vw, jw = torch.full((8, ldv), -5.0, device=dev), torch.full((8, ldj), -9, dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.mfcd_pair_best_workspace_bytes(8, m, d), dev)
    _lib.check(L.mfcd_pair_best_rows(wide[:, 3:].data_ptr(), wide.stride(0), None, 0, Gw.data_ptr(), stride, ldg, d, 8, m, None,
                                     vw.data_ptr(), ldv, jw.data_ptr(), ldj, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    assert vw[:, :m].cpu().numpy().tobytes() == base[0].tobytes() and jw[:, :m].cpu().numpy().tobytes() == base[1].tobytes()
    assert bool((vw[:, m:] == -5.0).all()) and bool((jw[:, m:] == -9).all())
    empty = pairs.pair_best_rows(to(dev, A)[:0], to(dev, G)[:0])
    assert tuple(empty[0].shape) == (0, m) and tuple(empty[1].shape) == (0, m)


@pytest.mark.parametrize("m,d", [(65, 3), (_tile() + 1, 64)])
def test_a_non_finite_row_is_nan_and_its_neighbours_are_untouched(dev, m, d):
    A, X = case_rows(m)
    G = tables(m, d)
    base = run(dev, A, G, X)
    A2, X2, G2 = A.copy(), X.copy(), G.copy()
    A2[1, m // 2] = np.inf
    X2[3, 0] = np.nan
    G2[5, m - 1, d - 1] = -np.inf
    G2[6, 0, 0] = np.nan
    val, arg = run(dev, A2, G2, X2)
    hit = np.array([1, 3, 5, 6])
    clean = np.setdiff1d(np.arange(8), hit)
    assert np.isnan(val[hit]).all() and (arg[hit] == -1).all()
    assert val[clean].tobytes() == base[0][clean].tobytes() and arg[clean].tobytes() == base[1][clean].tobytes()
    shared = G[0].copy()                                        # one table for all rows: every row is NaN
    shared[m // 3, 0] = np.nan
    val, arg = run(dev, A, shared)
    assert np.isnan(val).all() and (arg == -1).all()
