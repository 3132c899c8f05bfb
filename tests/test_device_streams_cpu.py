"""CPU tests of oracle/device_streams.py, the model of the device random streams ("The device random
streams") that tests/test_device_streams.py holds the two kernels to.

Two kinds of test.  The model itself: Philox against the published Random123 vectors, its integer and fp32 helpers
against Python's exact arithmetic, triplets pinned from an independent transcription, the keep rule's cutting
property.  And the fitness of the inputs the GPU tests use: an exact comparison is a fair demand only where the device's
arithmetic has no freedom, so no cdf lookup may fall within 1e-12 of an edge, and at most 1e-4 of a label case's draws
may fall inside the band in which the fp32 sigmoid decides.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import device_streams as D


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32-10 (kat_vectors of the Random123 distribution)."""
    kats = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
            ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
            ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
             (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for counter, key, want in kats:
        assert tuple(int(w) for w in D.philox4x32_10(counter, key)) == want
    # vectorised over the counter: each lane is the scalar function of its own counter
    words = D.philox4x32_10((np.array([0, 0xFFFFFFFF, 0x243F6A88], dtype=np.uint64), np.array([0, 0xFFFFFFFF, 0x85A308D3]),
                             np.array([0, 0xFFFFFFFF, 0x13198A2E]), np.array([0, 0xFFFFFFFF, 0x03707344])),
                            (np.array([0, 0xFFFFFFFF, 0xA4093822]), np.array([0, 0xFFFFFFFF, 0x299F31D0])))
    assert [tuple(int(w[r]) for w in words) for r in range(3)] == [k[2] for k in kats]


def test_multiply_high_and_the_conversions_against_python_integers():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.integers(0, 2 ** 64, 2000, dtype=np.uint64),
                        np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)])
    b = np.concatenate([rng.integers(0, 2 ** 64, 2000, dtype=np.uint64),
                        np.array([2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32 + 1, 2 ** 32, 2, 2 ** 64 - 1], dtype=np.uint64)])
    assert D.mulhi64(a, b).tolist() == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    for r in (1, 2, 37, 65000, 2_000_000_000, 2 ** 31 - 1):
        assert D.below(a, r).tolist() == [(int(x) * r) >> 64 for x in a]
    assert D.pair64(np.uint64(0x89ABCDEF), np.uint64(0x01234567)) == 0x0123456789ABCDEF
    assert D.unit53(a).tolist() == [(int(x) >> 11) / 2.0 ** 53 for x in a]
    assert D.unit53(np.uint64(2 ** 64 - 1)) < 1.0


def test_fma32_rounds_the_exact_sum_once():
    """fmaf as one rounding of a*b + c: against exact rationals, on random numbers and on sums that a product rounded
    to f64 first would round the other way (the exact sum sits just off an fp32 tie)."""
    rng = np.random.default_rng(2)
    a = (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(np.float32)
    b = (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-3, 4, 4000)).astype(np.float32)
    # 1 + 2^-24 is an fp32 tie.  4097 * 16773121 = 2^36 + 1 and (2^18 - 1)(2^18 + 1) = 2^36 - 1, so these products are
    # 2^-24 + 2^-60 and 2^-24 - 2^-60: the 2^-60 is below an f64 ulp of the sum, yet it decides the fp32 rounding
    a = np.concatenate([a, np.float32([4097 * 2.0 ** -30, -4097 * 2.0 ** -30, (2 ** 18 - 1) * 2.0 ** -30])])
    b = np.concatenate([b, np.float32([16773121 * 2.0 ** -30, 16773121 * 2.0 ** -30, (2 ** 18 + 1) * 2.0 ** -30])])
    c = np.concatenate([c, np.float32([1.0, -1.0, 1.0 + 2.0 ** -23])])

    def exact(x, y, z):
        s = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        if s == 0:
            return np.float32(0.0)
        # round the rational to 24 significant bits, ties to even
        e = 0
        while abs(s) * Fraction(2) ** -e >= 2 ** 24:
            e += 1
        while abs(s) * Fraction(2) ** -e < 2 ** 23:
            e -= 1
        q = abs(s) * Fraction(2) ** -e
        f = q.numerator // q.denominator
        rest = q - f
        if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and f % 2):
            f += 1
        return np.float32(float(Fraction(f) * Fraction(2) ** e) * (1 if s > 0 else -1))

    got = D.fma32(a, b, c)
    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got, want)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (naive[-3:] != want[-3:]).all()                    # the three cases do tell the two roundings apart


PINNED_SEED = 0x0123456789ABCDEF


def test_pinned_triplets_of_the_uniform_law():
    """Computed from a second transcription of the contract: they pin the stream against model and kernel drifting
    together, on both sides of the counter's low word."""
    law = D.Law(1000, 100)
    u, i, j, ok = D.sample_attempts(law, PINNED_SEED, 0, 4)
    assert np.stack([u, i, j], 1).tolist() == [[993, 15, 16], [189, 77, 18], [388, 81, 94], [586, 98, 71]]
    u, i, j, ok = D.sample_attempts(law, PINNED_SEED, 2 ** 32 - 2, 4)
    assert np.stack([u, i, j], 1).tolist() == [[296, 52, 20], [732, 8, 81], [83, 19, 13], [445, 76, 56]]
    assert ok.all()
    # an attempt is a function of (seed, index) alone: any window shows the same attempts
    whole = D.sample_attempts(law, PINNED_SEED, 2 ** 32 - 100, 300)
    for start, count in ((2 ** 32 - 100, 1), (2 ** 32 - 1, 2), (2 ** 32 + 57, 143)):
        part = D.sample_attempts(law, PINNED_SEED, start, count)
        lo = start - (2 ** 32 - 100)
        assert all(np.array_equal(w[lo:lo + count], p) for w, p in zip(whole, part))
    # both halves of the key count
    other = D.sample_attempts(law, PINNED_SEED ^ (1 << 32), 0, 64)
    assert not np.array_equal(other[0], D.sample_attempts(law, PINNED_SEED, 0, 64)[0])


def test_keep_first_is_the_reference_loop():
    keys = np.array([5, 7, 5, 9, 7, 11, 3, 3, 13], dtype=np.int64)
    ok = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1], dtype=bool)
    kept, used = D.keep_first(keys, ok, [], 100)
    assert kept.tolist() == [0, 1, 5, 6, 8] and used == 9
    kept, used = D.keep_first(keys, ok, [11, 7, 7, 11], 100)           # barred keys repeat, in any order
    assert kept.tolist() == [0, 6, 8] and used == 9
    kept, used = D.keep_first(keys, ok, [], 3)
    assert kept.tolist() == [0, 1, 5] and used == 6                    # the attempt that completed the request + 1
    kept, used = D.keep_first(keys, ok, [], 5)
    assert kept.tolist() == [0, 1, 5, 6, 8] and used == 9              # completed by the very last attempt
    kept, used = D.keep_first(keys, ok, [], 1)
    assert kept.tolist() == [0] and used == 1


@pytest.mark.parametrize("cuts", [(1000,), (257, 4000), (1, 2), (3999, 4999)])
def test_keep_first_does_not_depend_on_how_a_request_is_cut(cuts):
    """[0, A) in one call == the same attempts in two or three calls with the kept keys appended to `barred`."""
    law = D.Law(40, 12, margin=0.8, X=np.random.default_rng(3).standard_normal((40, 12)))
    A, seed, barred0 = 5000, 0xABCDEF0123456789, [100, 7, 100]
    u, i, j, ok = D.sample_attempts(law, seed, 0, A)
    keys = D.triplet_keys(u, i, j, law.m)
    assert 0 < ok.sum() < A and len(set(keys[ok].tolist())) < ok.sum()          # the filter and repeats both occur
    whole, used = D.keep_first(keys, ok, barred0, A)
    barred, kept = list(barred0), []
    for lo, hi in zip((0,) + cuts, cuts + (A,)):
        part, part_used = D.keep_first(keys[lo:hi], ok[lo:hi], barred, A)
        assert part_used == hi - lo
        kept += (part + lo).tolist()
        barred += keys[lo:hi][part].tolist()
    assert kept == whole.tolist() and used == A
    # and a request that is met stops there, wherever the cuts fall
    want = len(whole) // 2
    assert D.keep_first(keys, ok, barred0, want)[1] == whole[want - 1] + 1


def test_groups_law_rejects_what_a_malformed_table_offers():
    m, k = 30, 4
    members = np.arange(m, dtype=np.int32)
    members[12] = m                                                     # an item id outside [0, m)
    offsets = np.array([0, 10, 10, 22, 30], dtype=np.int32)           # group 1 is empty
    law = D.Law(100, m, D.LAW_GROUPS, list_i=members, list_j=offsets, k=k, list_row_stride=m)
    u, i, j, ok = D.sample_attempts(law, 9, 0, 20000)
    assert 0.3 < ok.mean() < 0.5                                        # 6 of 12 ordered group pairs, less id m
    assert i[ok].max() < m and j[ok].max() < m and (i[~ok] == 0).all() and (j[~ok] == 0).all()
    good = D.Law(100, m, D.LAW_GROUPS, list_i=np.arange(m), list_j=[0, 10, 15, 22, 30], k=k, list_row_stride=m)
    u, i, j, ok = D.sample_attempts(good, 9, 0, 20000)
    group_of = np.repeat(np.arange(k), (10, 5, 7, 8))
    assert ok.all() and (group_of[i] != group_of[j]).all()


def test_margin_filter_keeps_a_difference_equal_to_the_margin():
    A, B = D.integer_factors(50, 20, 4, 1)
    law = D.Law(50, 20, margin=3.0, A=A, B=B)
    u, i, j, ok = D.sample_attempts(law, 4, 0, 5000)
    diff = np.abs((A[u].astype(np.float64) * (B[i].astype(np.float64) - B[j])).sum(1))
    assert np.array_equal(ok, (diff <= 3.0) & (i != j)) and (diff[ok] == 3.0).any() and (diff[~ok] == 4.0).any()


@pytest.mark.parametrize("pair_rule", [0, 1])
@pytest.mark.parametrize("name", sorted(D.cdf_inputs()))
def test_cdf_inputs_of_the_gpu_tests_are_exact(name, pair_rule):
    """No uniform and no inverted x of these attempts comes within 1e-12 of a cdf edge (rounding freedom in forming x
    is about 1e-16): whichever way a compiler orders that arithmetic, the same item comes out."""
    cdf, attempts = D.cdf_inputs()[name]
    assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all()
    points = np.concatenate([D.cdf_lookups(cdf, pair_rule, D.CDF_SEED, attempt0, count)
                             for attempt0, count in ((0, attempts),) + D.EDGE_WINDOWS])
    edges = np.concatenate([[0.0], cdf])
    gap = np.abs(points[:, None] - edges[None, :]).min()
    print(f"{name} rule {pair_rule}: {len(points)} lookups, closest approach to an edge {gap:.3g}")
    assert gap > 1e-12
    # the inputs do what they are there for: zero-mass items are never drawn, every other item is
    u, i, j, ok = D.sample_attempts(D.Law(500, len(cdf), D.LAW_ITEM_CDF, pair_rule, cdf=cdf), D.CDF_SEED, 0, attempts)
    mass = np.diff(edges)
    assert ok.all() and (i != j).all() and not (mass[i] == 0).any() and not (mass[j] == 0).any()
    assert set(i.tolist()) | set(j.tolist()) == set(np.flatnonzero(mass > 0).tolist())


@pytest.mark.parametrize("name", sorted(D.label_inputs()))
def test_label_inputs_of_the_gpu_tests_stay_under_the_ambiguity_cap(name):
    trip, X, scale, K = D.label_inputs()[name]
    rows, z, ambiguous = D.labels(trip, X, scale, K, False, D.LABEL_SEED)
    assert rows.shape == (len(trip) * K, 3) and z.shape == (len(trip) * K,) and ambiguous.shape == (len(trip), K)
    assert ambiguous.size <= 100000
    print(f"{name}: {int(ambiguous.sum())} of {ambiguous.size} draws ambiguous")
    assert ambiguous.sum() <= 1e-4 * ambiguous.size
    soft_rows, soft_z, _ = D.labels(trip, X, scale, K, True, D.LABEL_SEED)
    assert np.array_equal(soft_rows, trip) and np.array_equal(soft_z, z.reshape(-1, K).sum(1) / np.float32(K))


def test_label_draws_take_word_q_of_group_g():
    uni = D.label_draws(D.LABEL_SEED, 300, 9)
    assert uni.dtype == np.float32 and uni.min() >= 0.0 and uni.max() < 1.0
    assert np.array_equal(uni[:, :5], D.label_draws(D.LABEL_SEED, 300, 5))         # a longer K extends a shorter one
    t = 257
    for g in range(3):
        words = D.philox4x32_10((t, 0, g, D.TAG_LABELS), (D.LABEL_SEED & 0xFFFFFFFF, D.LABEL_SEED >> 32))
        for q in range(4):
            if 4 * g + q < 9:
                assert float(uni[t, 4 * g + q]) == (int(words[q]) >> 8) / 2.0 ** 24
    sat = D.label_inputs()["saturated_T5000_K5"]
    arg = np.float32(sat[2]) * D.score_difference(sat[0][:, 0], sat[0][:, 1], sat[0][:, 2], X=sat[1])
    assert (np.abs(arg) > 100).sum() > 50                                           # saturated scores are present


def test_label_bit_probe_sits_between_the_24_bit_uniform_and_the_23_bit_one():
    """Fitness of the GPU test's probe: at each probed draw the f64 score lies between the 23-bit uniform and the 24-bit
    one, further than the band from both, and every score is 1/2 or at most 2^-6 (where that band is derived)."""
    T, K = 20000, 5
    trip, X, rows, draws = D.label_bit_probe(D.LABEL_SEED, T, K)
    assert len(rows) > 300
    p = 1.0 / (1.0 + np.exp(-X[:, 0].astype(np.float64)))
    assert ((p == 0.5) | (p <= 2.0 ** -6)).all() and (p[rows] >= 2.0 ** -11).all()
    above = D.label_draws(D.LABEL_SEED, T, K).astype(np.float64)[rows, draws] - p[rows]      # the 24-bit uniform - score
    assert (above > D.SMALL_SCORE_BAND).all() and (above < 2.0 ** -24 - D.SMALL_SCORE_BAND).all()
    rec, z, ambiguous = D.labels(trip, X, 1.0, K, False, D.LABEL_SEED, band=D.SMALL_SCORE_BAND)
    assert not ambiguous[rows, draws].any() and (z.reshape(T, K)[rows, draws] == 0).all()
    assert ambiguous.sum() <= 1e-4 * ambiguous.size
