"""GPU tests that replay the device random streams exactly: mfcd_sample_triplets (csrc/sampler.hip) and
mfcd_generate_labels (csrc/labels.hip) against oracle/device_streams.py, the CPU model written from the contract in
DESIGN.md, "The device random streams".

Both kernels are pure functions of (seed, index) through Philox4x32-10, so there is one right answer.  The sampler is
held to it with no tolerance: triplets, keys, the number written and the attempts consumed.  The labels are held to it
on every draw outside a derived band: the model feeds the device's own fp32 argument to an f64 sigmoid; what remains on
the device is expf (1 ulp in ROCm's device library), one fp32 add and one correctly rounded fp32 divide, under 3 ulp of
a value <= 1 (1.8e-7), and the band is 2^-21 (4.8e-7, eight steps of the 24-bit uniform).  That the inputs used here
are fair ones (no cdf lookup within 1e-12 of an edge, at most 1e-4 of a case's draws inside the band) is asserted
without a GPU in tests/test_device_streams_cpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import device_streams as D

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15              # both halves of the key non-zero
BLOCK = 70001                          # attempts of a full case: ragged, 274 workgroups


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# the laws, as the model's Law; _fill puts one into a mfcd_sampler
# ---------------------------------------------------------------------------------------------------------------------
def _lists_law(pair_rule):
    n, m, k = 300, 50, 7
    rng = np.random.default_rng(21)
    best = np.stack([rng.permutation(m)[:k] for _ in range(n)])
    if pair_rule:
        return D.Law(n, m, D.LAW_LISTS, 1, list_i=best, list_j=best, k=k, list_row_stride=k)
    other = np.stack([rng.permutation(m)[:k] for _ in range(n)])            # overlaps `best`: i == j occurs
    return D.Law(n, m, D.LAW_LISTS, 0, list_i=best, list_j=other, k=k, list_row_stride=k)


def _groups_law(malformed):
    m, k = 60, 4
    rng = np.random.default_rng(22)
    members = rng.permutation(m).astype(np.int32)
    offsets = [0, 30, 45, 55, 60]
    if malformed:
        members[33] = m                                                     # an item id outside [0, m)
        offsets = [0, 30, 30, 55, 60]                                       # group 1 is empty
    return D.Law(6000, m, D.LAW_GROUPS, list_i=members, list_j=offsets, k=k, list_row_stride=m)


def _margin_dense_law(margin=0.5):
    return D.Law(200, 50, margin=margin, X=np.random.default_rng(23).standard_normal((200, 50)))


def _margin_factors_law():
    A, B = D.integer_factors(50, 20, 4, 1)                                 # |diff| is an integer: some equal 3 exactly
    return D.Law(50, 20, margin=3.0, A=A, B=B)


LAWS = {
    "uniform": lambda: (D.Law(1000, 100), BLOCK),
    "uniform_users": lambda: (D.Law(1000, 100, users=[977, 3, 500, 3, 41, 999, 0, 612, 77, 250, 8]), BLOCK),
    "uniform_small_support": lambda: (D.Law(50, 37), BLOCK),               # 66 600 triplets exist: want exceeds them
    "lists_per_user_rule0": lambda: (_lists_law(0), BLOCK),
    "lists_per_user_rule1": lambda: (_lists_law(1), BLOCK),
    "lists_shared_users": lambda: (D.Law(1000, 100, D.LAW_LISTS, 1, list_i=[90, 4, 17, 55, 2, 99, 31, 68, 0],
                                         list_j=[90, 4, 17, 55, 2, 99, 31, 68, 0], k=9, list_row_stride=0,
                                         users=[5, 999, 17, 640, 2, 313, 800, 44, 71, 123, 456]), BLOCK),
    "groups": lambda: (_groups_law(False), BLOCK),
    "groups_empty_group_and_bad_id": lambda: (_groups_law(True), BLOCK),
    "margin_dense": lambda: (_margin_dense_law(), BLOCK),
    "margin_integer_factors": lambda: (_margin_factors_law(), BLOCK),
    "uniform_63_bit_keys": lambda: (D.Law(2_000_000_000, 65_000), BLOCK),  # keys up to 8.45e18 (limit 9.2e18)
}
for _name, (_cdf, _attempts) in D.cdf_inputs().items():
    for _rule in (0, 1):
        LAWS[f"cdf_{_name}_rule{_rule}"] = (lambda c=_cdf, r=_rule, a=_attempts:
                                            (D.Law(500, len(c), D.LAW_ITEM_CDF, r, cdf=c), a))


def _fill(c, law, hold, dev):
    """The model's Law into a mfcd_sampler; `hold` keeps the device tensors alive and returns their pointers."""
    def put(a):
        return None if a is None else hold(torch.from_numpy(a).to(dev))
    c.law, c.n, c.m, c.pair_rule = law.law, law.n, law.m, law.pair_rule
    c.cdf, c.list_i, c.list_j = put(law.cdf), put(law.list_i), put(law.list_j)
    c.k, c.list_row_stride = law.k, law.list_row_stride
    c.users, c.n_users = put(law.users), 0 if law.users is None else len(law.users)
    c.use_margin, c.margin = int(law.margin is not None), 0.0 if law.margin is None else law.margin
    c.X, c.A, c.B = put(law.X), put(law.A), put(law.B)
    c.dx = 0 if law.A is None else law.A.shape[1]


def _device_call(dev, law, seed, attempt0, attempts, want, barred=()):
    """One call of the C entry → (triplets [got, 3], keys [got], got, attempts consumed), on the host."""
    from mfcd import _lib
    L = _lib.load()
    keep = []

    def hold(t):
        keep.append(t)
        return _lib.ptr(t)

    c = _lib.Sampler()
    _fill(c, law, hold, dev)
    bar = torch.from_numpy(np.asarray(barred, dtype=np.int64)).to(dev) if len(barred) else None      # none: NULL
    E = 0 if bar is None else bar.numel()
    ws_bytes = L.mfcd_sample_workspace_bytes(attempts, E)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    trip = torch.full((want, 3), -7, dtype=torch.int32, device=dev)
    keys = torch.full((want,), -7, dtype=torch.int64, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    _lib.check(L.mfcd_sample_triplets(ctypes.byref(c), _lib.ptr(bar), E, attempt0, attempts, seed, want,
                                      _lib.ptr(trip), _lib.ptr(keys), _lib.ptr(counts), _lib.ptr(ws), ws_bytes,
                                      _lib.stream_ptr(dev)))
    got, used = (int(v) for v in counts.tolist())
    assert 0 <= got <= want, (got, want)
    assert (trip[got:] == -7).all() and (keys[got:] == -7).all()            # nothing written past the count
    return trip[:got].cpu().numpy(), keys[:got].cpu().numpy(), got, used


def _replay(dev, law, seed, attempt0, attempts, want, barred=(), label=""):
    """The device call equals the model's, with no tolerance → the model's result."""
    model = D.sample_triplets(law, seed, attempt0, attempts, want, barred)
    device = _device_call(dev, law, seed, attempt0, attempts, want, barred)
    where = (label, hex(seed), attempt0, attempts, want)
    assert device[2] == model[2], ("counts_out[0]", where, device[2], model[2])
    assert device[3] == model[3], ("counts_out[1]", where, device[3], model[3])
    assert np.array_equal(device[0], model[0]), ("triplets_out", where, _first_difference(device[0], model[0]))
    assert np.array_equal(device[1], model[1]), ("keys_out", where, _first_difference(device[1], model[1]))
    return model


def _first_difference(a, b):
    rows = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
    return (len(rows), int(rows[0]), a[rows[0]].tolist(), b[rows[0]].tolist()) if len(rows) else None


# ---------------------------------------------------------------------------------------------------------------------
# 1. every law: a full block, ragged and one-attempt blocks, the counter's high word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAWS))
def test_every_law_replays_the_model(dev, name):
    law, attempts = LAWS[name]()
    seed = D.CDF_SEED if name.startswith("cdf_") else SEED                 # the seed whose cdf lookups the CPU test cleared
    trip, keys, got, used = _replay(dev, law, seed, 0, attempts, attempts, label=name)
    assert 0 < got and used == attempts
    for attempt0, count in D.EDGE_WINDOWS:
        _replay(dev, law, seed, attempt0, count, count, label=name)


def test_rejecting_laws_do_reject_what_they_should(dev):
    """The inputs are there for a reason: the model's own account of the two cases that must reject, not fault."""
    law, attempts = LAWS["groups_empty_group_and_bad_id"]()
    u, i, j, ok = D.sample_attempts(law, SEED, 0, attempts)
    assert 0.3 < ok.mean() < 0.5 and (i[ok] < law.m).all()                 # 6 of 12 ordered group pairs survive, less id m
    law, attempts = LAWS["margin_integer_factors"]()
    u, i, j, ok = D.sample_attempts(law, SEED, 0, attempts)
    diff = np.abs(D.score_difference(u, i, j, A=law.A, B=law.B))
    assert ((diff == 3.0) & ok).sum() > 100 and ((diff == 4.0) & ~ok).sum() > 100    # attempts land exactly on the margin


# ---------------------------------------------------------------------------------------------------------------------
# 2. the key: both words
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "groups", "lists_per_user_rule1"])
def test_both_words_of_the_seed_key_the_stream(dev, name):
    law, _ = LAWS[name]()
    low = 0x0000000012345678
    rows = [_replay(dev, law, seed, 0, 3001, 3001, label=name)[0]
            for seed in (low, low | (1 << 32), low | (0xFFFFFFFF << 32), low ^ 1)]
    for a in range(4):
        for b in range(a):
            assert not np.array_equal(rows[a][:50], rows[b][:50])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the keep rule at its edges
# ---------------------------------------------------------------------------------------------------------------------
def test_want_at_its_edges(dev):
    law, _ = LAWS["uniform_small_support"]()
    u, i, j, ok = D.sample_attempts(law, SEED, 0, 20000)
    keepers = D.keep_first(D.triplet_keys(u, i, j, law.m), ok, (), 20000)[0]
    t = np.flatnonzero(np.diff(keepers) >= 2)[-1]                          # a block that ends on an attempt not kept
    kept, last, attempts = int(t) + 1, int(keepers[t]) + 1, int(keepers[t + 1])
    assert last < attempts and 10000 < kept < attempts - 100               # repeats occur
    assert _replay(dev, law, SEED, 0, attempts, attempts, label="all")[2:] == (kept, attempts)
    assert _replay(dev, law, SEED, 0, attempts, 1, label="want 1")[2:] == (1, 1 + int(np.argmax(ok)))
    assert _replay(dev, law, SEED, 0, attempts, kept, label="want = kept")[2:] == (kept, last)
    assert _replay(dev, law, SEED, 0, attempts, kept + 1, label="want = kept + 1")[2:] == (kept, attempts)
    # the request completed by the block's very last attempt, and missed by one in the same block
    assert _replay(dev, law, SEED, 0, last, kept, label="last attempt completes")[2:] == (kept, last)
    assert _replay(dev, law, SEED, 0, last, kept + 1, label="last attempt, one short")[2:] == (kept, last)
    assert _replay(dev, law, SEED, 0, last - 1, kept, label="one attempt short")[2:] == (kept - 1, last - 1)


def test_barred_keys_unsorted_repeated_and_overlapping(dev):
    law, _ = LAWS["uniform_small_support"]()
    attempts = 20000
    trip, keys, kept, used = D.sample_triplets(law, SEED, 0, attempts, attempts)
    rng = np.random.default_rng(31)
    mine = rng.choice(keys, 3000, replace=False)                           # what the block would otherwise produce
    foreign = rng.integers(0, 50 * 37 * 37, 2000)                          # any key, drawn here or not
    barred = np.concatenate([mine, foreign, mine[:700], foreign[:300], keys[:1], keys[-1:]])
    barred = barred[rng.permutation(len(barred))]
    assert (np.diff(barred) < 0).any() and len(set(barred.tolist())) < len(barred)
    t2, k2, kept2, used2 = _replay(dev, law, SEED, 0, attempts, attempts, barred, label="barred")
    assert kept2 <= kept - 3000 and not (set(k2.tolist()) & set(barred.tolist()))
    # a request met in spite of them, and one barred key alone
    _replay(dev, law, SEED, 0, attempts, kept2 // 2, barred, label="barred, met")
    assert _replay(dev, law, SEED, 0, attempts, 5, keys[:1], label="one barred key")[1][0] == keys[1]


@pytest.mark.parametrize("name", ["uniform_small_support", "margin_dense", "groups_empty_group_and_bad_id"])
def test_cutting_a_request_into_calls_changes_nothing(dev, name):
    law, _ = LAWS[name]()
    A, A1, barred0 = 20000, 7013, [11, 5, 11]                              # A1 is no multiple of 256
    whole = _replay(dev, law, SEED, 0, A, A, barred0, label=name)
    first = _device_call(dev, law, SEED, 0, A1, A, barred0)
    second = _device_call(dev, law, SEED, A1, A - A1, A, barred0 + first[1].tolist())
    assert first[3] == A1 and second[3] == A - A1
    assert np.array_equal(np.concatenate([first[0], second[0]]), whole[0])
    assert np.array_equal(np.concatenate([first[1], second[1]]), whole[1])
    # and a met request stops at the same attempt, counted from its own call's start
    want = whole[2] - 10
    stop = D.sample_triplets(law, SEED, 0, A, want, barred0)[3]
    assert stop > A1
    tail = _device_call(dev, law, SEED, A1, A - A1, want - first[2], barred0 + first[1].tolist())
    assert tail[2:] == (want - first[2], stop - A1) and np.array_equal(tail[0], whole[0][first[2]:want])


# ---------------------------------------------------------------------------------------------------------------------
# 4. sampling.run_law: blocks, budgets, the margin strategy's rounding
# ---------------------------------------------------------------------------------------------------------------------
def _host_law(dev, law):
    from mfcd import sampling
    host = sampling._Law(law.n, law.m, dev)
    _fill(host.c, law, host.hold, dev)
    return host


def test_run_law_over_three_blocks_is_one_keep_first(dev):
    """Every one of the 15 600 triplets of a small catalogue is asked for: a coupon collector's request, which the
    model says takes more than two blocks of 65 536 attempts.  Whatever the blocks, the rows are the model's keep-first
    over [0, attempts) and `attempts` is the attempt that completed the request + 1."""
    from mfcd import sampling
    law, want = D.Law(10, 40), 10 * 40 * 39
    trip, keys, got, used = D.sample_triplets(law, SEED, 0, 6 * 65536, want)
    assert got == want and used > 2 * 65536, used                          # at least three blocks
    rows, attempts = sampling.run_law(_host_law(dev, law), want, None, SEED)
    assert attempts == used
    assert np.array_equal(rows.cpu().numpy(), trip)


def test_run_law_margin_rounding_and_spent_budget(dev):
    from mfcd import sampling
    law = _margin_dense_law(0.05)
    # a request that is met: the attempts are reported in whole blocks of 500
    trip, keys, got, used = D.sample_triplets(law, SEED, 0, 3000, 40)
    assert got == 40 and used % 500 and used < 2500
    host = _host_law(dev, law)
    host.budget, host.block_multiple = 2750, 500
    rows, attempts = sampling.run_law(host, 40, None, SEED)
    assert attempts == -(-used // 500) * 500 and np.array_equal(rows.cpu().numpy(), trip)
    # a budget that is spent: 2 750 rounds up to 3 000 attempts, all of them evaluated
    trip, keys, got, used = D.sample_triplets(law, SEED, 0, 3000, 5000)
    assert 40 < got < 5000 and used == 3000
    rows, attempts = sampling.run_law(host, 5000, None, SEED)
    assert attempts == 3000 and np.array_equal(rows.cpu().numpy(), trip)
    # the same with an exclusion set, handed over as rows
    exclude = {tuple(r) for r in trip[::3].tolist()}
    rest = D.sample_triplets(law, SEED, 0, 3000, 5000, sampling.triplet_keys(sorted(exclude), law.m))
    rows, attempts = sampling.run_law(host, 5000, exclude, SEED)
    assert attempts == 3000 and np.array_equal(rows.cpu().numpy(), rest[0]) and rest[2] == got - len(exclude)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the label stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def label_cases():
    return D.label_inputs()


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("name", sorted(D.label_inputs()))
def test_labels_replay_the_model(dev, label_cases, name, soft):
    import generation_data as gd
    from mfcd import engine
    trip, X, scale, K = label_cases[name]
    Xd = gd.FactoredMatrix(*(torch.from_numpy(f) for f in X)) if isinstance(X, tuple) else torch.from_numpy(X).to(dev)
    rec = engine.generate_labels(trip, Xd, scale=scale, K=K, soft=soft, seed=D.LABEL_SEED, device=dev).cpu().numpy()
    rows, z, ambiguous = D.labels(trip, X, scale, K, soft, D.LABEL_SEED)
    assert ambiguous.sum() <= 1e-4 * ambiguous.size                        # the cap (proved on the CPU for these inputs)
    assert rec.shape == (len(rows), 4) and np.array_equal(rec[:, :3], rows)
    got = rec[:, 3].copy().view(np.float32)
    sure = ~ambiguous.any(axis=1) if soft else ~ambiguous.reshape(-1)
    wrong = np.flatnonzero((got != z) & sure)
    assert len(wrong) == 0, (name, soft, len(wrong), wrong[:5], got[wrong[:5]], z[wrong[:5]])
    if not soft:
        assert set(np.unique(got).tolist()) <= {0.0, 1.0}


def test_label_uniform_keeps_all_24_bits(dev):
    """A shorter uniform, (w >> 9) * 2^-23 say, moves a draw by at most 2^-24: inside the 2^-21 band, so no test above can
    see it.  The probe (oracle/device_streams.py: label_bit_probe) puts scores of at most 2^-6 midway between a draw's
    24-bit uniform and the 23-bit one below it; down there the fp32 sigmoid is within 2^-28 of the f64 one (2^-22
    relative: expf 1 ulp, an add, a divide), the band is 2^-26, and the probed draws are outside it (asserted on the
    CPU): their labels are 0 only if all 24 bits count."""
    from mfcd import engine
    T, K = 20000, 5
    trip, X, rows, draws = D.label_bit_probe(D.LABEL_SEED, T, K)
    rec = engine.generate_labels(trip, torch.from_numpy(X).to(dev), scale=1.0, K=K, seed=D.LABEL_SEED, device=dev)
    got = rec.cpu().numpy()[:, 3].copy().view(np.float32).reshape(T, K)
    _, z, ambiguous = D.labels(trip, X, 1.0, K, False, D.LABEL_SEED, band=D.SMALL_SCORE_BAND)
    assert len(rows) > 300 and not ambiguous[rows, draws].any()
    assert (got[rows, draws] == 0).all(), int((got[rows, draws] != 0).sum())
    assert np.array_equal(got[~ambiguous], z.reshape(T, K)[~ambiguous])


def test_label_key_uses_both_words_of_the_seed(dev, label_cases):
    from mfcd import engine
    trip, X, scale, K = label_cases["dense_T257_K9"]
    Xd = torch.from_numpy(X).to(dev)
    low = D.LABEL_SEED & 0xFFFFFFFF
    for seed in (low, low | (1 << 32), D.LABEL_SEED ^ 1):
        rec = engine.generate_labels(trip, Xd, scale=scale, K=K, seed=seed, device=dev).cpu().numpy()
        rows, z, ambiguous = D.labels(trip, X, scale, K, False, seed)
        sure = ~ambiguous.reshape(-1)
        assert sure.mean() > 0.999 and np.array_equal(rec[:, 3].copy().view(np.float32)[sure], z[sure]), hex(seed)
