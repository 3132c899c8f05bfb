"""CPU-only checks of what tests/test_uvt.py compares the UV^T pass with (tests/uvt_model.py): the f64 model agrees with
the C oracle and with a second f64 formulation, the derived bounds hold for the fp32 emulation of the tiled form on
every input family (100 % of rows), every deliberate error of the emulation breaks a bound on some family, and the
Python copy of the library's column-split plan is the library's.

The gap this closes: on `benign` data (what tests/test_hip_parity.py and tests/test_rows.py feed the pass) the older
rule, |error| <= 2e-5 * max over rows |column|, ACCEPTS the tiled form with its shift x0 removed
(test_old_rule_on_benign_accepts_no_shift); the per-row bounds reject it on `offset` and `degenerate`.
profiles/uvt_accuracy_mutations.txt records which family catches which error."""
import functools

import numpy as np
import pytest

import uvt_model as M

N, MM, D, S = 24, 300, 32, 1.1          # 300 = 9 tiles + 12 columns: the last split is ragged at every cols_per_split
CPS = (32, 128, MM)

# families whose bounds each deliberate error must break (profiles/uvt_accuracy_mutations.txt); at least these
CATCHES = {
    "no_shift": ("offset", "degenerate", "degenerate_v0"),
    "drop_mid_hi": ("benign", "offset", "outlier_first", "cancelling", "wide_range", "mixed_rows", "degenerate"),
    "ragged_mask_off_by_one": M.FAMILIES,
    "ns_is_cols_per_split": M.FAMILIES,
    "mean_not_rounded": M.FAMILIES,
    "colmean_for_rowmean": ("benign", "offset", "outlier_first", "cancelling", "wide_range", "mixed_rows", "degenerate"),
}


@functools.lru_cache(maxsize=None)
def _case(fam):
    U, V, X = M.family(fam, N, MM, D)
    return U, V, X, M.model(U, V, X, S)


@functools.lru_cache(maxsize=None)
def _bounds(fam, form, cps):
    U, V, X, _ = _case(fam)
    return M.bounds(U, V, X, S, form, cps)


def _worst(fam, form, cps, mutation=None):
    U, V, X, mdl = _case(fam)
    rs, sc = M.emulate(U, V, X, S, cps, form, mutation)
    rr, rsc, problems = M.check(rs, sc, mdl, _bounds(fam, form, cps))
    return rr, rsc, problems


def test_model_equals_the_c_oracle_on_benign(orc):
    """The oracle forms the product in fp32 (a d-step chain) and rounds a, c and s x to fp32: [0], [1] and the error sum
    lie within the generic form's bounds; its sum c^2 and ||sX||^2 also carry the fp32 rounding of c and of s x
    (2 u relative each) and of s itself."""
    U, V, X, (rs, sc, _) = _case("benign")
    ref_rows, err2, ref2 = orc.uvt_stats(U, V, X, S)
    B, Bs = M.bounds(U, V, X, S, "generic")
    assert (np.abs(ref_rows[:, 0] - rs[:, 0]) <= B[:, 0]).all()
    assert (np.abs(ref_rows[:, 1] - rs[:, 1]) <= B[:, 1]).all()
    assert (np.abs(ref_rows[:, 2] - rs[:, 2]) <= B[:, 2] + 4 * M.U32 * rs[:, 2]).all()
    assert abs(err2 - sc[0]) <= Bs[0]
    s32 = float(np.float32(S))
    assert abs(ref2 - sc[1]) <= Bs[1] + (4 * M.U32 + abs(s32 * s32 - S * S) / (S * S)) * sc[1]


@pytest.mark.parametrize("fam", M.FAMILIES)
def test_model_equals_a_second_f64_formulation(fam):
    """Two-pass, centre with the exact means, then sum (math.fsum), against the model's one expression: f64 rounding
    only, relative to the sums of absolute values."""
    U, V, X, (rs, sc, iv) = _case(fam)
    rs2, sc2 = M.model_two_pass(U, V, X, S)
    U6, V6, X6 = (t.astype(np.float64) for t in (U, V, X))
    G = U6 @ V6.T
    A = np.abs(U6) @ np.abs(V6).T                                  # what an entry of G can lose to cancellation
    a, c = np.abs(G - rs[:, 3:4]), np.abs(X6 - rs[:, 4:5])
    eps = 64 * MM * M.U64                                          # a few roundings per term, m terms
    ga = eps * A                                                   # error of an entry of G, either route
    assert np.array_equal(rs2[:, 3:5], rs[:, 3:5])                 # the fp32 means themselves
    assert np.array_equal(rs2[:, 6:8], rs[:, 6:8]) and (rs[:, 6:8] == 0).all() and (sc[2:] == 0).all()
    dmu = eps * np.abs(rs[:, 4:5])                                 # error of an entry of X - mean, either route
    tol = np.stack([(a * dmu + ga * c + ga * dmu).sum(1) + eps * (a * c).sum(1),
                    (2 * a * ga + ga * ga).sum(1) + eps * (a * a).sum(1),
                    (2 * c * dmu + dmu * dmu).sum(1) + eps * (c * c).sum(1)], axis=1)
    assert (np.abs(rs2[:, :3] - rs[:, :3]) <= tol).all(), np.abs(rs2[:, :3] - rs[:, :3]).max(axis=0)
    assert (np.abs(rs2[:, 5] - rs[:, 5]) <= 2 * eps * rs[:, 5]).all()
    e = np.abs(G - (V6 @ M.f32r(U6.mean(0)))[None, :] - S * X6)
    assert abs(sc2[0] - sc[0]) <= eps * (e * e).sum() + (2 * e * ga).sum() + (ga * ga).sum()
    assert abs(sc2[1] - sc[1]) <= eps * sc[1]
    assert (iv[:, :, 0] < rs[:, 3:5]).all() and (rs[:, 3:5] < iv[:, :, 1]).all()


@pytest.mark.parametrize("form", ("fp32", "split"))
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_emulation_stays_within_the_bounds_on_every_row(fam, form):
    for cps in CPS:
        rr, rsc, problems = _worst(fam, form, cps)
        print(f"{fam} {form} cols_per_split={cps}: error/bound rows {np.round(rr.max(axis=0), 3)} scal {np.round(rsc, 3)}")
        assert not problems, problems
        assert (rr <= 1.0).all(), (cps, np.argwhere(rr > 1.0)[:8].tolist(), rr.max(axis=0))
        assert (rsc <= 1.0).all(), (cps, rsc)


def test_emulation_within_bounds_at_d64_and_an_odd_split_width():
    """d = 64 (four k blocks of the split product) and the width the issue's table used (m = 1056, 256 per split)."""
    for fam in ("offset", "cancelling", "wide_range"):
        U, V, X = M.family(fam, 8, 1056, 64)
        mdl = M.model(U, V, X, S)
        for form in ("fp32", "split"):
            rs, sc = M.emulate(U, V, X, S, 256, form)
            rr, rsc, problems = M.check(rs, sc, mdl, M.bounds(U, V, X, S, form, 256))
            assert not problems and (rr <= 1.0).all() and (rsc <= 1.0).all(), (fam, form, rr.max(axis=0), rsc)


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_every_deliberate_error_breaks_a_bound(mutation):
    forms = ("split",) if mutation == "drop_mid_hi" else ("fp32", "split")
    caught = set()
    for fam in M.FAMILIES:
        for form in forms:
            for cps in CPS:
                rr, rsc, problems = _worst(fam, form, cps, mutation)
                if (rr > 1.0).any() or (rsc > 1.0).any() or problems:
                    caught.add(fam)
    print(mutation, "caught by", sorted(caught))
    assert caught, mutation
    assert set(CATCHES[mutation]) <= caught, (mutation, sorted(set(CATCHES[mutation]) - caught))


def test_old_rule_on_benign_accepts_no_shift():
    """THE GAP: the rule of the older tests — every column within 2e-5 of the largest row's value — passes the tiled form
    without its shift on benign data, in both forms and at every split width; the per-row bounds reject the same error
    on `offset` and `degenerate`."""
    U, V, X, (rs, sc, _) = _case("benign")
    for form in ("fp32", "split"):
        for cps in CPS:
            got, gsc = M.emulate(U, V, X, S, cps, form, "no_shift")
            for col in range(6):
                assert np.abs(got[:, col] - rs[:, col]).max() <= 2e-5 * np.abs(rs[:, col]).max(), (form, cps, col)
            assert abs(gsc[0] - sc[0]) <= 2e-5 * sc[0] and abs(gsc[1] - sc[1]) <= 2e-5 * sc[1]
    for fam in ("offset", "degenerate"):
        rr, _, _ = _worst(fam, "fp32", 128, "no_shift")
        assert (rr > 1.0).any(), fam


def test_old_rule_does_not_look_at_small_rows():
    """mixed_rows: an error of 100 % in the smallest row's sums is 1e-24 of the column's largest value."""
    U, V, X, (rs, _, _) = _case("mixed_rows")
    small = int(np.argmin(rs[:, 1]))
    wrong = rs.copy()
    wrong[small, :3] *= 2.0
    for col in range(3):
        assert np.abs(wrong[:, col] - rs[:, col]).max() <= 2e-5 * np.abs(rs[:, col]).max()
    B, _ = M.bounds(U, V, X, S, "split", 128)
    assert (np.abs(wrong[small, :3] - rs[small, :3]) > B[small, :3]).all()


def _align(x):
    return (x + 255) & ~255


def _workspace_bytes(n, m, d, splits, tiled, split_table):
    """plan_ws's layout (csrc/uvt.hip) for a plan with `splits` column splits."""
    rt = (n + 31) // 32
    n_err, nblk = splits * rt, (n + 255) // 256
    sizes = [8 * 2 * 256 * d, 4 * 2 * d, 4 * n, 4 * m, 4 * n, 8 * n, 8 * n, 8 * (6 if tiled else 2) * n * splits, 8 * n_err,
             8 * n_err, 8 * 2 * max(nblk, rt), 4 * (1 + rt), 8 * 8 * n, 8 * 4]
    if tiled and split_table:
        tc = M.tiled_tc(d)
        sizes.append(((m + tc - 1) // tc * tc + tc) * d * 4)
    return sum(_align(b) for b in sizes)


def test_python_plan_is_the_librarys_plan():
    """bounds() needs the first column of every split: uvt_model.plan must cut the columns as plan_ws does.  The split
    count shows in the workspace size (six doubles per split and row), so the two are compared through it, at the
    shapes and knob settings tests/test_uvt.py uses.  (Calls the built library, like the other host-logic tests: on a
    checkout where build() has not run it fails with MfcdError.  plan_ws, run_uvt and this layout move together.)"""
    from mfcd import _lib, engine
    L = _lib.load()
    shapes = [(n, m, d) for d in (32, 64, 128, 256) for n in (32, 33, 129)
              for m in (4, M.tiled_tc(d) - 4, M.tiled_tc(d) + 4, M.tiled_tc(d) + 1, 4 * M.tiled_tc(d) + 20,
                        16 * M.tiled_tc(d) + 20)]
    shapes += [(1, 1, 1), (31, 33, 5), (33, 100, 100), (16, 96, 64), (4096, 4096, 64), (300, 20000, 128)]
    try:
        for split, wgs, mst in ((1, 512, 8), (0, 512, 8), (1, 512, 1), (0, 4096, 2), (1, 256, 16)):
            engine.set_tuning(uvt_split=split, uvt_target_wgs=wgs, uvt_min_stages=mst)
            for n, m, d in shapes:
                tiled, cps, splits = M.plan(n, m, d, wgs, mst)
                assert splits == (m + cps - 1) // cps and (not tiled or cps % M.tiled_tc(d) == 0)
                assert L.mfcd_uvt_workspace_bytes(n, m, d) == _workspace_bytes(n, m, d, splits, tiled, split), (n, m, d, wgs, mst)
    finally:
        engine.set_tuning(uvt_split=1, uvt_target_wgs=512, uvt_min_stages=8)
    # the shapes the GPU tests rely on for their grids
    assert M.plan(129, 4 * 64 + 20, 64, 512, 1)[2] == 5 and M.plan(129, 16 * 64 + 20, 64, 512, 1)[2] == 9
    assert M.form_for(129, 100, 64) == ("split", 128) and M.form_for(129, 65, 64)[0] == "fp32"
    assert M.form_for(16, 100, 64)[0] == "generic" and M.form_for(129, 100, 64, tables_aligned=False)[0] == "generic"
