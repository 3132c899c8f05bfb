"""CPU model of the two device random streams ("The device random streams"): numpy only.

`mfcd_sample_triplets` (csrc/sampler.hip) and `mfcd_generate_labels` (csrc/labels.hip) are pure functions of
(seed, index) through Philox4x32-10, so their output has one right answer.  This module computes it from the contract
in DESIGN.md and include/mfcd.h: which counter a draw uses, which words of it, how 64 bits become an integer below r or
a unit double, the laws, the filters, and the reference loop's keep rule written as that loop (a set and a for).  The
device code switches FMA contraction off (csrc/common.h), so numpy's IEEE arithmetic is the same arithmetic; the one
library function on the path, the fp32 sigmoid of the labels, is modelled in f64 with a derived ambiguity band.

The last section holds the inputs that both tests/test_device_streams_cpu.py (are they fair inputs for an exact
comparison?) and tests/test_device_streams.py (the comparison, on the GPU) use.
"""
import numpy as np

LAW_UNIFORM, LAW_ITEM_CDF, LAW_LISTS, LAW_GROUPS = 0, 1, 2, 3
TAG_LABELS, TAG_SAMPLER = 0x6D666364, 0x73616D70          # fourth counter word: "mfcd", "samp"
AMBIGUITY_BAND = 2.0 ** -21                               # |uniform - p64| within which the fp32 sigmoid may decide

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 and the three conversions
# ---------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter: four 32-bit words (arrays broadcast against each other), key: two
    → the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(w, dtype=np.uint64) & _M32 for w in counter))
    k0, k1 = (np.asarray(w, dtype=np.uint64) & _M32 for w in key)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def pair64(lo, hi):
    """A 64-bit draw from two words: hi<<32 | lo."""
    return (np.asarray(hi, dtype=np.uint64) << _S32) | np.asarray(lo, dtype=np.uint64)


def mulhi64(a, b):
    """High 64 bits of the 128-bit product of two uint64 arrays."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    al, ah, bl, bh = a & _M32, a >> _S32, b & _M32, b >> _S32
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def below(bits, r):
    """Integer in [0, r) from 64 random bits: the high 64 bits of bits * r."""
    return mulhi64(bits, np.uint64(r)).astype(np.int64)


def unit53(bits):
    """Unit double from 64 random bits: (bits >> 11) * 2^-53."""
    return (np.asarray(bits, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------------
# fp32 arithmetic of the two gathers
# ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, exactly: the product of two fp32 numbers is exact in f64; the f64 sum is
    turned into a round-to-odd sum (the rounding error from TwoSum decides), which rounds to fp32 as the exact sum
    does."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    away = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, away), s)
    return s.astype(np.float32)


def score_difference(u, i, j, X=None, A=None, B=None):
    """The fp32 number X[u][i] - X[u][j] as both kernels form it: one fp32 subtraction of two entries of a dense X, or of
    two fmaf chains over the factors of X = A B^T (k ascending, from 0.0f)."""
    if X is not None:
        X = np.asarray(X, dtype=np.float32)
        return X[u, i] - X[u, j]
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    xi = np.zeros(len(u), dtype=np.float32)
    xj = np.zeros(len(u), dtype=np.float32)
    for q in range(A.shape[1]):
        xi = fma32(A[u, q], B[i, q], xi)
        xj = fma32(A[u, q], B[j, q], xj)
    return xi - xj


# ---------------------------------------------------------------------------------------------------------------------
# The sampler
# ---------------------------------------------------------------------------------------------------------------------
class Law:
    """The fields of mfcd_sampler (include/mfcd.h) with numpy arrays for its pointers."""

    def __init__(self, n, m, law=LAW_UNIFORM, pair_rule=0, cdf=None, list_i=None, list_j=None, k=0, list_row_stride=0,
                 users=None, margin=None, X=None, A=None, B=None):
        self.n, self.m, self.law, self.pair_rule = int(n), int(m), int(law), int(pair_rule)
        self.cdf = None if cdf is None else np.ascontiguousarray(cdf, dtype=np.float64)
        self.list_i = None if list_i is None else np.ascontiguousarray(list_i, dtype=np.int32)
        self.list_j = None if list_j is None else np.ascontiguousarray(list_j, dtype=np.int32)
        self.k, self.list_row_stride = int(k), int(list_row_stride)
        self.users = None if users is None else np.ascontiguousarray(users, dtype=np.int32)
        self.margin = None if margin is None else float(margin)          # None: no filter (use_margin = 0)
        self.X = None if X is None else np.ascontiguousarray(X, dtype=np.float32)
        self.A = None if A is None else np.ascontiguousarray(A, dtype=np.float32)
        self.B = None if B is None else np.ascontiguousarray(B, dtype=np.float32)


def cdf_pick(cdf, x):
    """searchsorted(cdf, x, side='right'), clamped to the catalogue."""
    return np.minimum(np.searchsorted(cdf, x, side="right"), len(cdf) - 1).astype(np.int64)


def cdf_redraw(cdf, i, bits):
    """The second item of a pair drawn without replacement, given the first: `bits` inverted through the cdf with item
    i's mass cut out → (x, j, ok); x is the point of the original cdf that was looked up."""
    m = len(cdf)
    start = np.where(i > 0, cdf[np.maximum(i - 1, 0)], 0.0)
    mass = cdf[i] - start
    x = unit53(bits) * (1.0 - mass)
    x = np.where(x >= start, x + mass, x)
    j = cdf_pick(cdf, x)
    j = np.where(j == i, np.where(i + 1 < m, i + 1, i - 1), j)      # x landed on i's upper edge after rounding
    return x, j, ((1.0 - mass) > 0.0) & (j >= 0)


def sampler_words(seed, attempt0, attempts, group):
    """The four words of draw group `group` for attempts [attempt0, attempt0 + attempts)."""
    t = np.uint64(attempt0) + np.arange(int(attempts), dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((t & _M32, t >> _S32, group, TAG_SAMPLER), (seed & 0xFFFFFFFF, seed >> 32))


def sample_attempts(law, seed, attempt0, attempts):
    """Attempts [attempt0, attempt0 + attempts) of a law → (u, i, j, ok), int64 / bool arrays of that length.  (u, i, j)
    of a rejected attempt are whatever the draws gave (0, 0 for a rejected attempt of the groups law)."""
    g0 = sampler_words(seed, attempt0, attempts, 0)
    g1 = sampler_words(seed, attempt0, attempts, 1)
    bu, b0, b1 = pair64(g0[0], g0[1]), pair64(g0[2], g0[3]), pair64(g1[0], g1[1])
    m = law.m
    u = law.users[below(bu, len(law.users))].astype(np.int64) if law.users is not None else below(bu, law.n)
    ok = np.ones(int(attempts), dtype=bool)
    if law.law == LAW_UNIFORM:
        i, j = below(b0, m), below(b1, m)
    elif law.law == LAW_ITEM_CDF:
        i = cdf_pick(law.cdf, unit53(b0))
        j = cdf_pick(law.cdf, unit53(b1)) if law.pair_rule == 0 else i.copy()
        again = j == i
        b2 = pair64(g1[2], g1[3]) if law.pair_rule == 0 else b1
        _, j2, ok2 = cdf_redraw(law.cdf, i, b2)
        j = np.where(again, j2, j)
        ok = np.where(again, ok2, True)
    elif law.law == LAW_GROUPS:
        g2 = sampler_words(seed, attempt0, attempts, 2)
        k, length = law.k, law.list_row_stride
        members, offsets = law.list_i.astype(np.int64), law.list_j.astype(np.int64)
        first = below(b0, k)
        second = below(b1, k - 1)
        second = second + (second >= first)
        lo1, n1 = offsets[first], offsets[first + 1] - offsets[first]
        lo2, n2 = offsets[second], offsets[second + 1] - offsets[second]
        ok = (n1 > 0) & (n2 > 0)
        pi = lo1 + mulhi64(pair64(g2[0], g2[1]), np.where(ok, n1, 1).astype(np.uint64)).astype(np.int64)
        pj = lo2 + mulhi64(pair64(g2[2], g2[3]), np.where(ok, n2, 1).astype(np.uint64)).astype(np.int64)
        i, j = members[np.clip(pi, 0, length - 1)], members[np.clip(pj, 0, length - 1)]
        ok = ok & (pi >= 0) & (pi < length) & (pj >= 0) & (pj < length) & (i >= 0) & (i < m) & (j >= 0) & (j < m)
        i, j = np.where(ok, i, 0), np.where(ok, j, 0)
    elif law.law == LAW_LISTS:
        k = law.k
        row = u * law.list_row_stride
        pi = below(b0, k)
        if law.pair_rule == 0:
            pj = below(b1, k)
        else:
            pj = below(b1, k - 1)
            pj = pj + (pj >= pi)
        i, j = law.list_i.reshape(-1)[row + pi].astype(np.int64), law.list_j.reshape(-1)[row + pj].astype(np.int64)
    else:
        raise ValueError(f"no such law: {law.law}")
    ok = ok & (i != j)
    if law.margin is not None:
        diff = score_difference(np.where(ok, u, 0), np.where(ok, i, 0), np.where(ok, j, 0), law.X, law.A, law.B)
        ok = ok & (np.abs(diff).astype(np.float64) <= law.margin)       # an fp32 difference, compared in f64
    return u, i, j, ok


def triplet_keys(u, i, j, m):
    """(u * m + i) * m + j as int64."""
    m = np.uint64(m)
    return ((u.astype(np.uint64) * m + i.astype(np.uint64)) * m + j.astype(np.uint64)).astype(np.int64)


def keep_first(keys, ok, barred, want):
    """The reference loop's keep rule over one block of attempts: the first `want` attempts, in order, that pass the
    filter, are not barred and repeat no earlier attempt → (their indices, attempts consumed)."""
    seen = set(int(b) for b in barred)
    kept = []
    for a, (key, good) in enumerate(zip(keys.tolist(), ok.tolist())):
        if not good or key in seen:
            continue
        seen.add(key)
        kept.append(a)
        if len(kept) == want:
            return np.asarray(kept, dtype=np.int64), a + 1
    return np.asarray(kept, dtype=np.int64), len(keys)


def sample_triplets(law, seed, attempt0, attempts, want, barred=()):
    """What one call of mfcd_sample_triplets must return → (triplets int32 [got, 3], keys int64 [got], got, attempts
    consumed)."""
    u, i, j, ok = sample_attempts(law, seed, attempt0, attempts)
    keys = triplet_keys(u, i, j, law.m)
    kept, used = keep_first(keys, ok, barred, want)
    return np.stack([u[kept], i[kept], j[kept]], axis=1).astype(np.int32), keys[kept], len(kept), used


# ---------------------------------------------------------------------------------------------------------------------
# The labels
# ---------------------------------------------------------------------------------------------------------------------
def label_draws(seed, T, K):
    """The K uniforms of each of T triplets, float32 [T, K] (24-bit values, exact in fp32): draw 4 g + q is word q of
    draw group g."""
    t = np.arange(int(T), dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.empty((int(T), int(K)), dtype=np.float32)
    for g in range((K + 3) // 4):
        words = philox4x32_10((t & _M32, t >> _S32, g, TAG_LABELS), (seed & 0xFFFFFFFF, seed >> 32))
        for q in range(min(4, K - 4 * g)):
            out[:, 4 * g + q] = (words[q] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return out


def labels(trip, X, scale, K, soft, seed, band=AMBIGUITY_BAND):
    """The records of mfcd_generate_labels → (rows int64 [N, 3], z float32 [N], ambiguous bool [T, K]); N = T * K hard
    rows or T soft rows.  X is a dense matrix or the pair (A, B) of X = A B^T.  The score's argument is the device's
    own fp32 number fl32(fl32(scale) * diff); its sigmoid is taken in f64, and a draw within AMBIGUITY_BAND of it is
    marked: there the device's fp32 sigmoid may decide either way (`band`: a narrower one, where the caller has derived it)."""
    trip = np.asarray(trip, dtype=np.int64).reshape(-1, 3)
    u, i, j = trip[:, 0], trip[:, 1], trip[:, 2]
    diff = score_difference(u, i, j, A=X[0], B=X[1]) if isinstance(X, tuple) else score_difference(u, i, j, X=X)
    arg = (np.float32(scale) * diff).astype(np.float64)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-arg))
    uni = label_draws(seed, len(trip), K).astype(np.float64)
    z = uni < p[:, None]
    ambiguous = np.abs(uni - p[:, None]) <= band
    if soft:
        return trip, z.sum(axis=1).astype(np.float32) / np.float32(K), ambiguous
    return np.repeat(trip, K, axis=0), z.reshape(-1).astype(np.float32), ambiguous


# ---------------------------------------------------------------------------------------------------------------------
# Inputs of the tests (CPU: fitness of the inputs; GPU: the comparison)
# ---------------------------------------------------------------------------------------------------------------------
def _cdf_of(p):
    cdf = np.cumsum(np.asarray(p, dtype=np.float64))
    return cdf / cdf[-1]


def cdf_inputs():
    """name → (cdf, attempts): the item laws of the GPU tests.  Zero-mass items first, inside and last; two items;
    one item holding 1 - 2^-20 of the mass."""
    zipf = np.arange(1, 38, dtype=np.float64) ** -1.5
    edges = zipf.copy()
    edges[[0, 17, 36]] = 0.0
    inner = zipf.copy()
    inner[[5, 6]] = 0.0
    heavy = np.full(9, 2.0 ** -23)
    heavy[4] = 1.0 - 2.0 ** -20
    return {
        "zipf37_zero_first_interior_last": (_cdf_of(edges), 70001),
        "zipf37_two_zero_items": (_cdf_of(inner), 70001),
        "two_items": (_cdf_of([0.3, 0.7]), 2000),
        # nearly every attempt redraws here, from a uniform scaled by 1 - mass = 2^-20 onto edges 2^-23 apart: a gap
        # of 1e-12 is a relative 1e-6 of that range, which 70 001 redraws do not all keep; 6 001 do
        "one_item_nearly_all": (_cdf_of(heavy), 6001),
    }


CDF_SEED = 0x5EED00D15EA5E001
# (attempt0, attempts) of the short calls every law is also replayed over: one attempt, a ragged last workgroup on
# both sides of 256, the counter's low word wrapping, its high word set
EDGE_WINDOWS = ((0, 1), (0, 255), (0, 257), (2 ** 32 - 100, 300), (2 ** 40, 257), (2 ** 40 + 12345, 1))


def cdf_lookups(cdf, pair_rule, seed, attempt0, attempts):
    """Every point at which the item-cdf law of these attempts looks the cdf up or compares with one of its edges: the
    first draw, the second (pair_rule 0), and for a redraw the scaled uniform (compared with the cut's start) and the
    inverted x."""
    g0 = sampler_words(seed, attempt0, attempts, 0)
    g1 = sampler_words(seed, attempt0, attempts, 1)
    x0, x1 = unit53(pair64(g0[2], g0[3])), unit53(pair64(g1[0], g1[1]))
    i = cdf_pick(cdf, x0)
    again = np.ones(len(i), dtype=bool) if pair_rule else cdf_pick(cdf, x1) == i
    bits = pair64(g1[0], g1[1]) if pair_rule else pair64(g1[2], g1[3])
    x, _, _ = cdf_redraw(cdf, i, bits)
    start = np.where(i > 0, cdf[np.maximum(i - 1, 0)], 0.0)
    scaled = unit53(bits) * (1.0 - (cdf[i] - start))
    points = [x0, x[again], scaled[again]]
    if not pair_rule:
        points.append(x1)
    return np.concatenate(points)


def integer_factors(n, m, dx, seed, span=3):
    """Factors with small integer entries: every fmaf chain over them is exact in fp32."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-span, span + 1, (n, dx)).astype(np.float32),
            rng.integers(-span, span + 1, (m, dx)).astype(np.float32))


LABEL_SEED = 0xC0FFEE1234567890


def label_inputs():
    """name → (trip, X or (A, B), scale, K): the label cases of the GPU tests (each at most 100 000 draws)."""
    n, m = 300, 200
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((n, m)).astype(np.float32)
    Xs = X.copy()
    Xs[:, :8] *= 60.0                                   # columns whose differences saturate the sigmoid
    A, B = integer_factors(n, m, 6, 5)

    def trip(T):
        return np.stack([rng.integers(0, n, T), rng.integers(0, m, T), rng.integers(0, m, T)], axis=1)

    return {
        "dense_T20000_K5": (trip(20000), X, 1.7, 5),
        "dense_T20000_K4": (trip(20000), X, 1.7, 4),
        "dense_T10000_K9": (trip(10000), X, 0.6, 9),
        "dense_T257_K9": (trip(257), X, 1.7, 9),
        "dense_T1_K1": (trip(1), X, 1.7, 1),
        "saturated_T5000_K5": (trip(5000), Xs, 1.7, 5),
        "integer_factors_T20000_K5": (trip(20000), (A, B), 0.125, 5),
        "integer_factors_saturated_T5000_K4": (trip(5000), (A, B), 9.0, 4),
    }


SMALL_SCORE_BAND = 2.0 ** -26


def label_bit_probe(seed, T, K):
    """An input that tells the 24-bit uniform from a shorter one → (trip, X, rows, draws).  Triplet t is (t, 0, 1) on an
    X of T rows and two columns, scale 1, so the score's argument is X[t][0] itself.  Where one of row t's K uniforms is
    an odd multiple of 2^-24 in [2^-10, 2^-6], X[t][0] is the logit of that uniform - 2^-25, midway between it and the
    23-bit uniform below: the label of that draw is 0 only if bit 0 of the 24 counts.  Elsewhere X[t][0] = 0 (score
    exactly 1/2 on any arithmetic).  Scores are either 1/2 or <= 2^-6, where the device's sigmoid (expf within 1 ulp,
    an add and a divide: 2^-22 relative) is within 2^-28 of the f64 one, so here the band is SMALL_SCORE_BAND."""
    uni = label_draws(seed, T, K).astype(np.float64)
    odd = np.rint(uni * 2.0 ** 24).astype(np.int64) % 2 == 1
    fit = odd & (uni >= 2.0 ** -10) & (uni <= 2.0 ** -6)
    rows = np.flatnonzero(fit.any(axis=1))
    draws = fit[rows].argmax(axis=1)
    target = uni[rows, draws] - 2.0 ** -25
    X = np.zeros((T, 2), dtype=np.float32)
    X[rows, 0] = np.log(target / (1.0 - target)).astype(np.float32)
    trip = np.stack([np.arange(T), np.zeros(T, dtype=np.int64), np.ones(T, dtype=np.int64)], axis=1)
    return trip, X, rows, draws
