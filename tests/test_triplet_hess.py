"""GPU tests of the triplet gradient / Hessian-vector kernel (include/mfcd.h: mfcd_triplet_rows; mfcd/newton.py:
triplet_rows) against the f64 numpy model of tests/newton_model.py (rows_pass).

Inputs: 9 users and 9 items, U, V, P, Q ~ N(0, 1) in f64, soft labels (multiples of 1/4).  With S =
mfcd_triplet_rows_segment() a call has seven rows of the lengths {0, 1, 3, S - 1, S, S + 1, 2 S + 3}: the empty row, less
than a segment, the segment's edges and three segments; every row with records holds one comparison of an item with
itself.  d in {2, 3, 64, 100, 256} covers a lane group narrower than the wave, a width that is no power of two, the
whole wave, and two and four elements per lane.

Tolerance, per row r: |out - ref|_inf <= (K + 4 d + 64) 2^-52 A_r, and the same for diag and loss, where K is the
longest row of the call and A_r the model's sum of the absolute values of the row's terms, the l2 term included (for out
and diag the largest such sum over the row's columns).  It is the f64 bound of a sum of K terms, each with a dot product
of d terms in it, and the device's exp at 1 ulp."""
import functools

import numpy as np
import pytest
import torch

import newton_model as NM

pytestmark = pytest.mark.gpu

N_USERS, M_ITEMS = 9, 9
DS = (2, 3, 64, 100, 256)
L2 = 0.375


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def segment():
    from mfcd import _lib
    return _lib.load().mfcd_triplet_rows_segment()


def row_lengths():
    S = segment()
    return [0, 1, 3, S - 1, S, S + 1, 2 * S + 3]


@functools.lru_cache(maxsize=None)
def case(d, side):
    """→ (U, V, P, Q, rec, row_off): one ragged call of seven rows, row r owning table row r."""
    rng = np.random.default_rng(100 * d + side)
    U, P = rng.standard_normal((N_USERS, d)), rng.standard_normal((N_USERS, d))
    V, Q = rng.standard_normal((M_ITEMS, d)), rng.standard_normal((M_ITEMS, d))
    lengths = row_lengths()
    chunks = []
    for r, T in enumerate(lengths):
        other, z = rng.integers(0, M_ITEMS, T), rng.integers(0, 5, T) / 4.0
        if side == 0:
            u, i, j = np.full(T, r), rng.integers(0, M_ITEMS, T), other
            if T:
                j[T // 2] = i[T // 2]
        else:
            first = rng.random(T) < 0.5
            u = rng.integers(0, N_USERS, T)
            i, j = np.where(first, r, other), np.where(first, other, r)
            if T:
                i[T // 2] = j[T // 2] = r
        chunks.append(NM.records(u, i, j, z))
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    return U, V, P, Q, np.concatenate(chunks), off


@functools.lru_cache(maxsize=None)
def reference(d, side, pas, gn):
    U, V, P, Q, rec, off = case(d, side)
    return NM.rows_pass(side, pas, gn, U, V, P, Q, rec, off, None, L2)


def to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, d, side, pas, gn, rec=None, off=None, seg=None, row_id=None):
    """One kernel call on the case's tables → [out, diag, loss, status] as numpy arrays (None where there is none)."""
    from mfcd import newton
    U, V, P, Q, rec0, off0 = case(d, side)
    rec, off = rec0 if rec is None else rec, off0 if off is None else off
    seg = NM.segment_rows(off, segment()) if seg is None else seg
    rows = newton.Rows(to(dev, rec), to(dev, off), to(dev, seg[0]), seg[1])
    got = newton.triplet_rows(side, pas, to(dev, U), to(dev, V), rows, L2, to(dev, P) if pas else None,
                              to(dev, Q) if pas else None, bool(gn), to(dev, row_id))
    return [None if t is None else t.cpu().numpy() for t in got]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


PASSES = ((0, 0), (1, 0), (1, 1))            # (pass, gauss_newton)


@pytest.mark.parametrize("side", [0, 1], ids=["users", "items"])
@pytest.mark.parametrize("d", DS)
def test_parity_with_the_model_and_bit_equal_repeats(dev, d, side):
    U, V, P, Q, rec, off = case(d, side)
    factor = (max(row_lengths()) + 4 * d + 64) * 2.0 ** -52
    worst = 0.0
    for pas, gn in PASSES:
        ref = reference(d, side, pas, gn)
        out, diag, loss, status = run(dev, d, side, pas, gn)
        assert (status == 0).all(), (pas, gn, status)
        pairs = [("out", out, ref.out, ref.abs_out.max(1))]
        if pas == 0:
            pairs.append(("diag", diag, ref.diag, ref.abs_diag.max(1)))
            if side == 0:
                pairs.append(("loss", loss[:, None], ref.loss[:, None], ref.abs_loss))
            else:
                assert loss is None
        else:
            assert diag is None and loss is None
        for name, got, want, A in pairs:
            err = np.abs(got - want).max(1)
            share = np.where(err > 0, err / (factor * np.maximum(A, 1e-300)), 0.0)
            print(f"d={d} side={side} pass={pas} gn={gn} {name}: worst row {share.argmax()} at {share.max():.3f} of the bound")
            worst = max(worst, share.max())
            assert (err <= factor * A).all(), (pas, gn, name, share)
        # the empty row: l2 x its row of the table (of the direction in pass 1) exactly, diag = l2, loss = 0
        base = (P if side == 0 else Q) if pas else (U if side == 0 else V)
        assert bits(out[0]) == bits(L2 * base[0])
        if pas == 0:
            assert (diag[0] == L2).all() and (side == 1 or loss[0] == 0.0)
        again = run(dev, d, side, pas, gn)
        for a, b in zip((out, diag, loss, status), again):
            assert (a is None and b is None) or bits(a) == bits(b), (pas, gn)
    assert not np.array_equal(reference(d, side, 1, 0).out, reference(d, side, 1, 1).out)     # two different products
    print(f"worst share of the parity bound: {worst:.3f}")


@pytest.mark.parametrize("side", [0, 1], ids=["users", "items"])
@pytest.mark.parametrize("d", DS)
def test_rows_do_not_depend_on_their_place_in_the_call(dev, d, side):
    """A permuted subset of the rows through row_id, with regrouped records: bit-equal row for row to the full call."""
    U, V, P, Q, rec, off = case(d, side)
    perm = np.array([5, 2, 6, 0, 3])
    sub_rec = np.concatenate([rec[off[r]:off[r + 1]] for r in perm])
    sub_off = np.concatenate(([0], np.cumsum([off[r + 1] - off[r] for r in perm]))).astype(np.int64)
    for pas, gn in PASSES:
        full = run(dev, d, side, pas, gn)
        part = run(dev, d, side, pas, gn, sub_rec, sub_off, row_id=perm.astype(np.int32))
        assert (part[3] == 0).all()
        for a, b in zip(full[:3], part[:3]):
            assert (a is None and b is None) or bits(a[perm]) == bits(b), (pas, gn)


@pytest.mark.parametrize("side", [0, 1], ids=["users", "items"])
@pytest.mark.parametrize("d", [3, 100])
def test_invalid_rows_get_status_2_and_leave_their_neighbours_alone(dev, d, side):
    """Row 3: an item index out of range; row 2: a record of another owner; row 5: z = 1.5 in its second segment; row 4:
    a segment count that does not fit its length.  Rows 0, 1 and 6 stay bit-equal to the clean call."""
    U, V, P, Q, rec, off = case(d, side)
    S = segment()
    bad = rec.copy()
    bad[off[3] + 7, 2 if side == 0 else (2 if bad[off[3] + 7, 1] == 3 else 1)] = M_ITEMS
    if side == 0:
        bad[off[2] + 1, 0] = 3
    else:
        bad[off[2] + 1, 1:3] = (4, 5)
    bad[off[6] - 1, 3] = np.array([1.5], dtype=np.float32).view(np.int32)[0]
    seg_off, n_seg = NM.segment_rows(off, S)
    seg_off = seg_off.copy()
    seg_off[5:] += 1
    for pas, gn in PASSES:
        clean = run(dev, d, side, pas, gn)
        out, diag, loss, status = run(dev, d, side, pas, gn, bad, off, (seg_off, n_seg + 1))
        assert status.tolist() == [0, 0, 2, 2, 2, 2, 0], (pas, gn, status)
        for r in (2, 3, 4, 5):
            assert np.isnan(out[r]).all() and (diag is None or np.isnan(diag[r]).all()) and (loss is None or np.isnan(loss[r]))
        for a, b in zip(clean[:3], (out, diag, loss)):
            assert (a is None and b is None) or bits(a[[0, 1, 6]]) == bits(b[[0, 1, 6]]), (pas, gn)
    # an own index out of range, offsets that run backwards, segments beyond n_seg: status 2, nothing else
    row_id = np.arange(7, dtype=np.int32)
    row_id[1] = N_USERS if side == 0 else M_ITEMS
    out, _, _, status = run(dev, d, side, 0, 0, row_id=row_id)
    assert status.tolist() == [0, 2, 0, 0, 0, 0, 0] and np.isnan(out[1]).all()
    back = off.copy()
    back[3] = back[2] - 1
    _, _, _, status = run(dev, d, side, 0, 0, off=back, seg=NM.segment_rows(off, S))
    assert status.tolist() == [0, 0, 2, 2, 0, 0, 0]
    _, _, _, status = run(dev, d, side, 0, 0, seg=(NM.segment_rows(off, S)[0], n_seg - 1))
    assert status.tolist() == [0, 0, 0, 0, 0, 0, 2]


def test_both_sides_give_the_passes_of_the_plain_model(dev):
    """triplet_pass / triplet_hvp on plain comparisons, grouped by mfcd.newton.group_rows: F, the gradient, the diagonal
    and both products against the plain model, within the row bound at the longest row."""
    from mfcd import newton
    n, m, d, N = 30, 20, 5, 4000
    U0, V0, u, i, j, z = NM.make_fit_case(n, m, d, N)
    U, V = U0.astype(np.float64), V0.astype(np.float64)
    rng = np.random.default_rng(2)
    P, Q = rng.standard_normal(U.shape), rng.standard_normal(V.shape)
    j[:5] = i[:5]
    by_user, by_item = newton.group_rows(*(to(dev, a) for a in (u, i, j, z)), n, m)
    ref_u, ref_i = NM.group_by_user(u, i, j, z, n), NM.group_by_item(u, i, j, z, m)
    assert np.array_equal(by_user.records.cpu().numpy(), ref_u[0]) and np.array_equal(by_item.records.cpu().numpy(), ref_i[0])
    K = int(np.diff(ref_i[1]).max())
    assert K > segment() and by_item.n_seg > m                      # rows of more than one segment
    factor = (K + 4 * d + 64) * 2.0 ** -52
    F, gU, gV, DU, DV = (t.cpu().numpy() for t in newton.triplet_pass(to(dev, U), to(dev, V), by_user, by_item, L2))
    rF, rgU, rgV, rDU, rDV = NM.gradient(U, V, u, i, j, z, L2)
    ru, ri = NM.rows_pass(0, 0, 0, U, V, None, None, *ref_u, None, L2), NM.rows_pass(1, 0, 0, U, V, None, None, *ref_i, None, L2)
    assert abs(F - rF) <= (N + 4 * d + 64) * 2.0 ** -52 * (ru.abs_loss.sum() + rF)
    for got, want, A in ((gU, rgU, ru.abs_out), (gV, rgV, ri.abs_out), (DU, rDU, ru.abs_diag), (DV, rDV, ri.abs_diag)):
        assert (np.abs(got - want) <= 2 * factor * A.max(1, keepdims=True)).all()
    for gn in (False, True):
        HU, HV = (t.cpu().numpy() for t in newton.triplet_hvp(to(dev, U), to(dev, V), by_user, by_item, to(dev, P), to(dev, Q), L2, gn))
        rHU, rHV = NM.hvp(U, V, u, i, j, z, P, Q, L2, gn)
        hu = NM.rows_pass(0, 1, gn, U, V, P, Q, *ref_u, None, L2)
        hi = NM.rows_pass(1, 1, gn, U, V, P, Q, *ref_i, None, L2)
        assert (np.abs(HU - rHU) <= 2 * factor * hu.abs_out.max(1, keepdims=True)).all()
        assert (np.abs(HV - rHV) <= 2 * factor * hi.abs_out.max(1, keepdims=True)).all()
