"""GPU tests of the dense UV^T pass (csrc/uvt.hip; include/mfcd.h: mfcd_uvt_stats, _select, _slab, mfcd_uvt_rows)
against the plain f64 model of tests/uvt_model.py, row by row under the bounds derived there: all six row outputs, both
global sums, the reserved outputs exactly zero, NaN where the model gives NaN.  Input families (uvt_model.family):
benign, offset, outlier_first, cancelling, wide_range, mixed_rows, degenerate (+ all-zero V).

Shapes.  TC = stage width of the tiled form (d = 32: 128, 64 / 128: 64, 256: 32).  Tiled: n in {32, 33, 129} (one full
wave, a ragged wave, a second row block with three idle waves), m in {4, TC-4, TC+4, TC+1, 4 TC + 20, 16 TC + 20}: a
single short stage, a ragged second stage, the scalar-X instantiation, and with uvt_min_stages = 1 five splits and nine
splits (the XCD-mapped grid) with a ragged last split of 20 columns; n = 33 meets every m, 32 and 129 five of them.
Generic: d in {1, 2, 3, 5, 8, 16, 24, 100}, n in {1, 31, 33}, m in {1, 2, 3, 31, 33, 100}, and d = 64 with 16 rows.  What form runs and how the columns are cut is
uvt_model.form_for / plan, which tests/test_uvt_cpu.py holds to the library's own plan.

NOT covered here: the finishing kernels of passes with n m > 2^26 (uvt_final_tiled_kernel in both grid shapes and
uvt_scal_kernel behind it).  Reaching them needs a 256 MiB X, which an f64 model cannot follow in a few seconds; the
full-size C3 / C5 cases of tests/test_hip_parity.py remain their only coverage.

Every case records its largest error / bound ratio per family, form and output; `pytest -s` prints the table at the
end (profiles/uvt_accuracy.txt is one such run)."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import uvt_model as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

S = 1.1
RATIOS = {}          # (family, form) -> [max ratio of row outputs 0..5, scal 0, scal 1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    if RATIOS:
        print("\nlargest error / bound per family and form: row_stats[0..5], scal[0], scal[1]")
        for (fam, form), r in sorted(RATIOS.items()):
            print(f"  {fam:14s} {form:8s} " + " ".join(f"{v:8.2e}" for v in r))


@contextlib.contextmanager
def knobs(uvt_split=1, uvt_target_wgs=512, uvt_min_stages=8):
    from mfcd import engine
    try:
        engine.set_tuning(uvt_split=uvt_split, uvt_target_wgs=uvt_target_wgs, uvt_min_stages=uvt_min_stages)
        yield
    finally:
        engine.set_tuning(uvt_split=1, uvt_target_wgs=512, uvt_min_stages=8)


@functools.lru_cache(maxsize=64)
def _inputs(fam, n, m, d):
    U, V, X = M.family(fam, n, m, d)
    return U, V, X, M.model(U, V, X, S)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _hold(fam, form, got_rows, got_scal, mdl, bnd, what=3, label=""):
    rr, rsc, problems = M.check(got_rows, got_scal, mdl, bnd, what)
    worst = np.concatenate([rr.max(axis=0), rsc])
    key = (fam, form)
    RATIOS[key] = np.maximum(RATIOS.get(key, np.zeros(8)), np.where(np.isfinite(worst), worst, 9.99e99))
    print(f"{label} {fam} {form}: error/bound rows {np.array2string(rr.max(axis=0), precision=3)} scal {np.array2string(rsc, precision=3)}")
    assert not problems, (label, fam, problems)
    assert (rr <= 1.0).all(), (label, fam, form, "rows, outputs", np.argwhere(rr > 1.0)[:6].tolist(), rr.max(axis=0))
    assert (rsc <= 1.0).all(), (label, fam, form, rsc)


def _run(dev, fam, n, m, d, uvt_split, min_stages=8, what=3):
    """One pass on family data under the given knobs, compared with the model.  -> (rows, scal) numpy."""
    from mfcd import metrics
    U, V, X, mdl = _inputs(fam, n, m, d)
    form, cps = M.form_for(n, m, d, uvt_split, min_stages=min_stages)
    with knobs(uvt_split=uvt_split, uvt_min_stages=min_stages):
        rs, sc = metrics.uvt_stats(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev), S, what)
    rs, sc = _np(rs), _np(sc)
    _hold(fam, form, rs, sc, mdl, M.bounds(U, V, X, S, form, cps, what), what, f"n={n} m={m} d={d} st={min_stages} what={what}")
    return rs, sc


def _tiled_shapes(d):
    tc = M.tiled_tc(d)
    return ([(33, mm, 8) for mm in (4, tc - 4, tc + 4, tc + 1)] + [(33, 4 * tc + 20, 1), (33, 16 * tc + 20, 1)]
            + [(32, tc + 1, 8), (32, 4 * tc + 20, 1), (129, tc - 4, 8), (129, tc + 4, 8), (129, 16 * tc + 20, 1)])


TILED = [(d, sp) for d in (32, 64, 128, 256) for sp in (1, 0)]


@pytest.mark.parametrize("d,uvt_split", TILED)
def test_tiled_forms_hold_the_row_bounds_at_every_shape(dev, d, uvt_split):
    tc = M.tiled_tc(d)
    assert M.plan(33, 4 * tc + 20, d, 512, 1)[2] == 5 and M.plan(129, 16 * tc + 20, d, 512, 1)[2] == 9
    for n, m, st in _tiled_shapes(d):
        for fam in ("benign", "offset"):
            _run(dev, fam, n, m, d, uvt_split, st)


@pytest.mark.parametrize("d,uvt_split", TILED)
def test_tiled_forms_hold_the_row_bounds_on_every_family(dev, d, uvt_split):
    for fam in M.FAMILIES:
        _run(dev, fam, 129, 4 * M.tiled_tc(d) + 20, d, uvt_split, 1)


@pytest.mark.parametrize("d,uvt_split", TILED)
def test_tiled_narrow_passes(dev, d, uvt_split):
    """what = 1: the rows are bit-equal to the full pass's; what = 2: the two sums hold the model's bounds (the error-only
    pass adds x^2 itself)."""
    n, m = 129, 4 * M.tiled_tc(d) + 20
    for fam in ("offset", "mixed_rows"):
        rs3, sc3 = _run(dev, fam, n, m, d, uvt_split, 1, 3)
        rs1, sc1 = _run(dev, fam, n, m, d, uvt_split, 1, 1)
        rs2, sc2 = _run(dev, fam, n, m, d, uvt_split, 1, 2)
        assert sc1 is None and rs2 is None
        assert np.array_equal(rs1, rs3)


GENERIC = [(1, 1, 1), (1, 33, 100), (2, 31, 2), (2, 33, 33), (3, 33, 3), (3, 31, 100), (5, 31, 33), (5, 1, 31),
           (8, 33, 31), (8, 31, 100), (16, 33, 33), (16, 1, 3), (24, 31, 31), (24, 33, 100), (100, 33, 100), (100, 31, 1),
           (64, 16, 100)]


@pytest.mark.parametrize("d,n,m", GENERIC)
def test_generic_form_holds_the_row_bounds(dev, d, n, m):
    assert M.form_for(n, m, d)[0] == "generic"
    for fam in ("benign", "offset", "mixed_rows"):
        _run(dev, fam, n, m, d, 1)


def _off_by_one_float(a, dev):
    """The array as a view one float into a larger device buffer: same values, data pointer off a 16-byte boundary."""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=dev)
    buf[1:] = torch.from_numpy(a).to(dev).reshape(-1)
    v = buf[1:].view(*a.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("d,n,m", [(64, 129, 100), (8, 33, 100)])
def test_tables_off_a_16_byte_boundary(dev, d, n, m):
    """U, V one float into a larger buffer: d = 64 leaves the tiled form for uvt_main_kernel<0> under the tiled plan's
    column split; d = 8 leaves the MFMA instantiation."""
    from mfcd import metrics
    for fam in ("benign", "offset", "mixed_rows"):
        U, V, X, mdl = _inputs(fam, n, m, d)
        form, cps = M.form_for(n, m, d, tables_aligned=False)
        assert form == "generic"
        rs, sc = metrics.uvt_stats(_off_by_one_float(U, dev), _off_by_one_float(V, dev), torch.from_numpy(X).to(dev), S)
        _hold(fam, "generic", _np(rs), _np(sc), mdl, M.bounds(U, V, X, S, form, cps), label=f"unaligned tables d={d}")


@pytest.mark.parametrize("d,n,m", [(64, 129, 100), (256, 33, 52), (8, 33, 100)])
def test_x_off_a_16_byte_boundary_with_m_a_multiple_of_4(dev, d, n, m):
    from mfcd import metrics
    assert m % 4 == 0
    for fam in ("benign", "offset"):
        U, V, X, mdl = _inputs(fam, n, m, d)
        form, cps = M.form_for(n, m, d, x_aligned=False)
        assert form == ("fp32" if d >= 32 else "generic")
        rs, sc = metrics.uvt_stats(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), _off_by_one_float(X, dev), S)
        _hold(fam, form, _np(rs), _np(sc), mdl, M.bounds(U, V, X, S, form, cps), label=f"unaligned X d={d}")


# ---------------------------------------------------------------------------------------------------------------------
# slab entry
# ---------------------------------------------------------------------------------------------------------------------
CUTS = [0, 1, 34, 97, 111, 130, 131]      # slabs of 1, 33, 63, 14, 19 and 1 rows at odd row0


@pytest.mark.parametrize("uvt_split", (1, 0))
def test_slab_passes_at_odd_cuts_hold_the_model(dev, uvt_split):
    """mfcd_uvt_stats_slab through dist.hip_slab_pass: every slab's rows and share against the MODEL (not the dense pass);
    slabs of fewer than 32 rows run the generic form inside a table that plans tiled; the last slab is one row.  The
    first 34 rows of U carry a large offset, so a slab's own column mean is far from the table's: a pass that centred
    with the slab's rows would miss the share's bound by orders of magnitude (asserted on the model)."""
    from mfcd import dist as mdist
    n, d, m = CUTS[-1], 64, 4 * 64 + 20
    for fam in ("benign", "offset"):
        U, V, X = M.family(fam, n, m, d)
        U = U.copy()
        U[:34] += np.float32(3.0)
        Ud, Vd, Xd = (torch.from_numpy(t).to(dev) for t in (U, V, X))
        total, total_bound = np.zeros(2), np.zeros(2)
        with knobs(uvt_split=uvt_split, uvt_min_stages=1):
            for r0, r1 in zip(CUTS[:-1], CUTS[1:]):
                rows = slice(r0, r1)
                form, cps = M.form_for(r1 - r0, m, d, uvt_split, min_stages=1)
                assert form == ("generic" if r1 - r0 < 32 else ("split" if uvt_split else "fp32"))
                rs, share = mdist.hip_slab_pass(Ud, Vd, Xd[r0:r1], r0, S, 3)
                mdl = M.model(U, V, X, S, rows=rows)
                bnd = M.bounds(U, V, X, S, form, cps, rows=rows)
                _hold(fam, form, _np(rs), _np(share), mdl, bnd, label=f"slab [{r0},{r1})")
                if fam == "benign":                               # (offset: X is up to 1e4, the error sum is mostly X)
                    own = M.model(U[rows], V, X[rows], S)[1]      # centred with the slab's own rows: must be far off
                    assert abs(own[0] - mdl[1][0]) > 1e3 * bnd[1][0], (r0, r1)
                total += _np(share)[:2]
                total_bound += bnd[1]
            if fam == "offset":
                # the same claim on this family: rows 13 and 26 have |X| ~ 0.01 (X does not drown the error sum there),
                # one in the shifted part of U and one outside it, each as a slab of its own
                for r0 in (13, 39):
                    rows = slice(r0, r0 + 1)
                    assert np.abs(X[rows]).max() < 0.1
                    rs, share = mdist.hip_slab_pass(Ud, Vd, Xd[r0:r0 + 1], r0, S, 3)
                    mdl, bnd = M.model(U, V, X, S, rows=rows), M.bounds(U, V, X, S, "generic", None, rows=rows)
                    _hold(fam, "generic", _np(rs), _np(share), mdl, bnd, label=f"slab [{r0},{r0 + 1})")
                    own = M.model(U[rows], V, X[rows], S)[1]
                    assert abs(own[0] - mdl[1][0]) > 1e3 * bnd[1][0], r0
        full = M.model(U, V, X, S)[1]
        assert (np.abs(total - full[:2]) <= total_bound).all(), (total, full, total_bound)


@pytest.mark.parametrize("slab_rows", (33, 65))
def test_factored_ground_truth_in_slabs_holds_the_model(dev, slab_rows):
    """metrics.uvt_stats_factored: X = A B^T formed slab by slab.  A and B hold small integers, so every entry of X is
    exact in fp32 whatever the GEMM's order and the model sees the X the kernel saw.  131 rows in slabs of 33 (the last has
    32) and of 65 (the last is a single row)."""
    from generation_data import FactoredMatrix
    from mfcd import metrics
    n, m, d = 131, 100, 64
    rng = np.random.default_rng(5)
    A, B = rng.integers(-4, 5, (n, 4)).astype(np.float32), rng.integers(-4, 5, (m, 4)).astype(np.float32)
    X = A @ B.T
    U, V, _ = M.family("benign", n, m, d)
    FX = FactoredMatrix(torch.from_numpy(A), torch.from_numpy(B))
    rs, sc = metrics.uvt_stats_factored(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), FX, S, 3, slab_rows)
    rs, sc = _np(rs), _np(sc)
    Bs = np.zeros(2)
    cuts = list(range(0, n, slab_rows)) + [n]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        rows = slice(r0, r1)
        form, cps = M.form_for(r1 - r0, m, d)
        mdl, bnd = M.model(U, V, X, S, rows=rows), M.bounds(U, V, X, S, form, cps, rows=rows)
        rr, _, problems = M.check(rs[rows], None, mdl, bnd, what=1)
        assert not problems and (rr <= 1.0).all(), (r0, r1, rr.max(axis=0))
        Bs += bnd[1]
    full = M.model(U, V, X, S)[1]
    assert (np.abs(sc[:2] - full[:2]) <= Bs).all() and (sc[2:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# non-finite values, determinism, bf16 tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n,m,uvt_split", [(64, 129, 276, 1), (64, 129, 276, 0), (5, 33, 100, 1)])
def test_non_finite_inputs_stay_in_their_rows(dev, d, n, m, uvt_split):
    """One NaN and one +Inf in X, one NaN in U (ordinary arithmetic on NaN: nothing is indexed with a bad value).  Outputs
    the model leaves finite are bit-equal to the clean run's; where the model gives NaN because of a NaN input the pass
    gives NaN; in the row with the +Inf every output the model makes NaN or infinite is non-finite (inf - inf and
    inf - finite meet in another order in the shifted sums than in the model's: NaN there may be an infinity here and the
    other way round); the error sum and ||sX||^2 are NaN as the model says.  Tiled form with the tail (five splits), and
    the generic form."""
    from mfcd import metrics
    U, V, X, _ = _inputs("benign", n, m, d)
    U2, X2 = U.copy(), X.copy()
    X2[3, 17], X2[20, 40], U2[10, 2] = np.nan, np.inf, np.nan
    want, wsc, _ = M.model(U2, V, X2, S)
    assert np.isnan(wsc[:2]).all() and np.isfinite(want[[0, 1, 2, 4, 5, n - 1]]).all()
    assert np.isnan(want[3, [0, 2, 4, 5]]).all() and np.isnan(want[10, [0, 1, 3]]).all() and np.isinf(want[20, [4, 5]]).all()
    with knobs(uvt_split=uvt_split, uvt_min_stages=1):
        clean, _ = metrics.uvt_stats(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev), S)
        got, gsc = metrics.uvt_stats(torch.from_numpy(U2).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(X2).to(dev), S)
    clean, got, gsc = _np(clean), _np(got), _np(gsc)
    fin, nan, inf = np.isfinite(want), np.isnan(want), np.isinf(want)
    assert np.array_equal(got[fin], clean[fin])
    inf_row = np.zeros_like(fin)
    inf_row[20, [0, 2, 4, 5]] = True                 # the outputs of that row that depend on X: exactly its non-finite ones
    assert np.array_equal((nan | inf)[20], inf_row[20])
    assert np.isnan(got[nan & ~inf_row]).all()
    assert (~np.isfinite(got[inf_row])).all()
    assert np.isnan(gsc[:2]).all() and (gsc[2:] == 0).all()


def test_two_calls_are_bit_equal_at_the_nine_split_grid(dev):
    """The tail finishes a row block in whichever workgroup arrives last: every sum has a fixed order all the same.  Also
    after a pass of another shape has used the stream's workspace."""
    from mfcd import metrics
    n, m, d = 129, 16 * 64 + 20, 64
    U, V, X, _ = _inputs("offset", n, m, d)
    Ud, Vd, Xd = (torch.from_numpy(t).to(dev) for t in (U, V, X))
    o = [torch.from_numpy(t).to(dev) for t in _inputs("benign", 33, 100, 64)[:3]]
    for uvt_split in (1, 0):
        with knobs(uvt_split=uvt_split, uvt_min_stages=1):
            assert M.plan(n, m, d, 512, 1)[2] == 9
            a = metrics.uvt_stats(Ud, Vd, Xd, S)
            b = metrics.uvt_stats(Ud, Vd, Xd, S)
            metrics.uvt_stats(o[0], o[1], o[2], 0.7)
            c = metrics.uvt_stats(Ud, Vd, Xd, S)
        for other in (b, c):
            assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])


@pytest.mark.parametrize("d,n,m", [(64, 129, 276), (5, 33, 100)])
def test_bf16_tables_equal_their_fp32_widening(dev, d, n, m):
    from mfcd import metrics
    U, V, X, _ = _inputs("benign", n, m, d)
    Ub, Vb, Xd = torch.from_numpy(U).to(dev).bfloat16(), torch.from_numpy(V).to(dev).bfloat16(), torch.from_numpy(X).to(dev)
    a = metrics.uvt_stats(Ub, Vb, Xd, S)
    b = metrics.uvt_stats(Ub.float(), Vb.float(), Xd, S)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    Uw, Vw = Ub.float().cpu().numpy(), Vb.float().cpu().numpy()
    form, cps = M.form_for(n, m, d)
    _hold("benign", form, _np(a[0]), _np(a[1]), M.model(Uw, Vw, X, S), M.bounds(Uw, Vw, X, S, form, cps), label="bf16 tables")


# ---------------------------------------------------------------------------------------------------------------------
# mfcd_uvt_rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (33, 100, 5), (64, 257, 64), (40, 31, 256)])
def test_uvt_rows_against_f64(dev, n, m, d):
    """Per element within gamma(d) (|U| |V|^T)[row]: uvt_rows_kernel adds d products to acc = 0 in fp32; fused or not, a
    product passes through at most d roundings (the first addition, to 0, is exact).  The fp32 output is compared in
    f64.  Ids repeated and negative; no id -> [0, m]."""
    from mfcd import metrics
    for fam in ("benign", "cancelling", "wide_range"):
        U, V, _ = M.family(fam, n, m, d)
        Ud, Vd = torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev)
        ids = np.array([0, n - 1, -1, -n, n // 2, 0, n // 2, -(n // 2) - 1])
        got = metrics.uvt_rows(Ud, Vd, ids).cpu().numpy()
        assert got.shape == (len(ids), m) and got.dtype == np.float32
        U6, V6 = U.astype(np.float64), V.astype(np.float64)
        want = (U6 @ V6.T)[ids]
        tol = M.gamma(d) * (np.abs(U6) @ np.abs(V6).T)[ids]
        assert (np.abs(got - want) <= tol).all(), (fam, np.abs(got - want).max())
        empty = metrics.uvt_rows(Ud, Vd, np.zeros(0, dtype=np.int64))
        assert tuple(empty.shape) == (0, m)
    with pytest.raises(IndexError):
        metrics.uvt_rows(Ud, Vd, [n])


# ---------------------------------------------------------------------------------------------------------------------
# host metrics on degenerate rows, against the reference's own results (oracle/make_golden_metrics.py)
# ---------------------------------------------------------------------------------------------------------------------
M14 = ["alpha", "norm_X", "norm_ratio", "rec_scaled", "pearson_mean", "pearson_std", "spearman_mean", "spearman_std",
       "svd_err", "slopes", "correlations", "spearman_scores", "rec_scaled_per_row", "alpha_per_row"]


@pytest.mark.parametrize("variant", ("degenerate", "degenerate_v0"))
def test_host_metrics_filter_degenerate_rows_as_the_reference_does(dev, variant):
    """Constant X rows (0, 0.3, 1000), zero U rows, and V = 0: the drop-in compute_alpha_and_norm_ratios /
    compute_reconstruction_error against what the reference returned on the same inputs, with the tolerances of
    test_e2e_train_eval_metrics_match_reference.  The list lengths encode which rows each filter kept: exact."""
    import structure as S_
    g = dict(np.load(os.path.join(GOLDEN, "metrics_degenerate.npz"), allow_pickle=False))
    U, V, X = g[f"{variant}.U"], g[f"{variant}.V"], g[f"{variant}.X"]
    model = S_.MatrixFactorization(U.shape[0], V.shape[0], U.shape[1])
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(U))
        model.V.copy_(torch.from_numpy(V))
    model = model.to(dev)
    Xd = torch.from_numpy(X).to(dev)
    ref_err, got_err = float(g[f"{variant}.rec_error"]), S_.compute_reconstruction_error(model, Xd, float(g["s"]))
    assert got_err == pytest.approx(ref_err, abs=1e-5)
    res = S_.compute_alpha_and_norm_ratios(model, Xd)
    assert len(res) == 14
    for nm, v in zip(M14, res):
        ref = g[f"{variant}.m14_{nm}"]
        v = np.asarray(v, dtype=np.float64)
        assert v.shape == ref.shape, (nm, v.shape, ref.shape)
        scale = max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0)
        np.testing.assert_allclose(v, ref, rtol=0, atol=1e-4 * scale, err_msg=nm)
