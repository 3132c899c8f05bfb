"""CPU-only tests: the C-ABI library loads and exports what include/mfcd.h declares, the host data
pipeline consumes torch/numpy RNG exactly like the reference (checked against golden fixtures), and
the drop-in module keeps the reference's names and signatures."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_golden


def test_library_exports_every_declared_symbol():
    from mfcd import _lib
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    declared = set(re.findall(r"\b(mfcd_[a-z_0-9]+)\s*\(", header))
    declared.discard("mfcd_sample")
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    L = _lib.load()  # binds each symbol; AttributeError if one is missing
    assert L.mfcd_abi_version() == 4
    assert L.mfcd_error_string(0).decode() == "success"
    assert L.mfcd_error_string(-1).decode().startswith("mfcd:")
    # pure host helpers may be called without a GPU
    assert L.mfcd_train_workspace_bytes(1000, 64, 16, 16, 8) >= 2 * 16 * 8 * 4 + 4000
    # an unregistered workspace is refused before anything touches the device; tuning setters validate their input
    assert L.mfcd_set_tuning(_lib.TUNE_KEYS["resident_lookahead"], 17) == -1
    assert L.mfcd_set_tuning(_lib.TUNE_KEYS["resident_lookahead"], -1) == 0
    for key, former_default in ((1, 0), (2, 16), (4, 0), (6, 3), (7, 2), (8, 0), (12, 1)):   # retired keys
        assert L.mfcd_set_tuning(key, former_default) == -1, key
    assert L.mfcd_train_workspace_release(None) == 0
    assert L.mfcd_error_string(-6).decode().startswith("mfcd: workspace not initialised")
    plan = _lib.TrainPlan()
    import ctypes
    assert L.mfcd_train_plan_query(67108, 64, 4096, 4096, 64, 0, ctypes.byref(plan)) == 0
    assert (plan.form, plan.resident_q, plan.resident_waves, plan.resident_lookahead) == (2, 2, 4096, 4)
    assert L.mfcd_train_plan_query(64, 64, 4096, 4096, 64, 0, ctypes.byref(plan)) == 0 and plan.form == 1   # short call
    assert L.mfcd_train_plan_query(67108, 64, 65536, 65536, 64, 0, ctypes.byref(plan)) == 0 and plan.form == 1
    assert L.mfcd_train_plan_query(1310, 64, 256, 256, 8, 0, ctypes.byref(plan)) == 0 and plan.form == 3
    assert L.mfcd_train_plan_query(107373, 64, 16384, 16384, 128, 1, ctypes.byref(plan)) == 0    # C3, bf16 tables
    assert (plan.form, plan.resident_q, plan.resident_waves, plan.fast_math) == (2, 32, 2048, 1)
    assert L.mfcd_uvt_workspace_bytes(100, 100, 8) > 0


def test_resident_plans_follow_the_slice_rule_and_layouts_ignore_the_knobs():
    """Over the grid of tools/plan_table.py, with the resident form forced: wherever the library plans it, the plan is a
    slice of the one rule (csrc/resident.hip: resident_slices) - whole rows per wave, the wave count of that slice, at
    most 4096 waves, four waves per workgroup.  And the workspace size, which the same rule decides, is a function of the
    sizes alone: the same under every train path and every look-ahead setting."""
    import ctypes
    import importlib.util
    from mfcd import _lib
    spec = importlib.util.spec_from_file_location("plan_table", os.path.join(ROOT, "tools", "plan_table.py"))
    grid = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(grid)
    L = _lib.load()
    cases = [(N, B, n, m, d) for n, m, d in grid.SHAPES for B in grid.BATCHES
             for N in (B, 3 * B, 40 * B, 300 * B + 5)]
    planned = 0
    try:
        assert L.mfcd_set_train_path(2) == 0
        plan = _lib.TrainPlan()
        for N, B, n, m, d in cases:
            for bf16 in (0, 1):
                rc = L.mfcd_train_plan_query(N, B, n, m, d, bf16, ctypes.byref(plan))
                assert rc in (0, -1), (rc, N, B, n, m, d)
                if rc == 0:
                    planned += 1
                    q, waves = plan.resident_q, plan.resident_waves
                    assert plan.form == 2 and (64 * q) % d == 0, (q, N, B, n, m, d)
                    assert waves == -(-(n + m) * d // (64 * q)) and waves <= 4096, (q, waves, N, B, n, m, d)
                    assert plan.resident_blocks == -(-waves // 4), (waves, plan.resident_blocks)
        assert planned > len(cases)          # (more than half of the grid: the check is not vacuous)
        sizes = {c: L.mfcd_train_workspace_bytes(*c) for c in cases}
        for path in range(4):
            assert L.mfcd_set_train_path(path) == 0
            for look in (-1, 0, 4, 8):
                assert L.mfcd_set_tuning(_lib.TUNE_KEYS["resident_lookahead"], look) == 0
                for c in cases:
                    assert L.mfcd_train_workspace_bytes(*c) == sizes[c] > 0, (path, look, c)
    finally:
        L.mfcd_set_train_path(0)
        L.mfcd_set_tuning(_lib.TUNE_KEYS["resident_lookahead"], -1)


def test_missing_library_is_loud(monkeypatch):
    from mfcd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(PKG, "does_not_exist.so"))
    with pytest.raises(_lib.MfcdError, match="no CPU fallback"):
        _lib.load()


def test_cpu_tensors_are_rejected():
    import structure as S
    from mfcd import _lib, engine
    model = S.MatrixFactorization(8, 8, 4)
    opt = torch.optim.Adam(model.parameters())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.train_model(model, None, None, opt, "cpu", num_epochs=1)
    with pytest.raises(_lib.MfcdError):
        engine.AdamBinding(model, opt)
    with pytest.raises(_lib.MfcdError):
        engine.eval_batches(model.U.data, model.V.data, torch.zeros((0, 4), dtype=torch.int32), 64)


@pytest.mark.parametrize("name,seed", [("e2e_c1.npz", 0), ("e2e_soft_k3.npz", 1), ("e2e_hard_k2_d16.npz", 2)])
def test_data_pipeline_is_rng_identical_to_reference(name, seed):
    """generate_X -> split_dataset_from_triplets -> model init -> per-epoch order, all bit-equal to what the
    reference produced from the same seeds (fixtures from oracle/make_golden.py)."""
    import structure as S
    from mfcd.batching import epoch_order
    g = load_golden(name)
    n, m, d, K = int(g["n"]), int(g["m"]), int(g["d"]), int(g["K"])
    torch.manual_seed(seed)
    np.random.seed(seed)
    X = S.generate_X(n, m, d, "cpu")
    np.testing.assert_allclose(X.numpy(), g["X"], rtol=0, atol=1e-6)
    X = torch.from_numpy(g["X"])  # continue from the reference's X so later comparisons are exact
    loaders = S.split_dataset_from_triplets(X, int(n * m * float(g["p"]) / 2), scale=float(g["s"]), K=K,
                                            soft_label=bool(g["soft_label"]))
    for nm, ld in zip(("train", "val", "test"), loaders):
        np.testing.assert_array_equal(np.asarray(ld.dataset.data, dtype=np.float64), g[nm + "_data"])
    model = S.MatrixFactorization(n, m, d)
    np.testing.assert_array_equal(model.U.detach().numpy(), g["U0"])
    np.testing.assert_array_equal(model.V.detach().numpy(), g["V0"])
    np.testing.assert_array_equal(torch.get_rng_state().numpy(), g["rng_state_before_train"])
    train, val, _ = loaders
    rows = np.asarray(train.dataset.data, dtype=np.float64)
    for e in range(int(g["epochs"])):
        order, bs = epoch_order(train)
        assert bs == 64
        np.testing.assert_array_equal(rows[order.numpy()], g["epoch_stream"][e])
        epoch_order(val)
    np.testing.assert_array_equal(torch.get_rng_state().numpy(), g["rng_state_after_train"])


def test_epoch_order_equals_dataloader_iteration():
    """epoch_order must visit samples exactly as iterating the DataLoader does, for both samplers."""
    from mfcd.batching import epoch_order
    data = [(k, k + 1, k + 2, float(k % 2)) for k in range(203)]

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(data)

        def __getitem__(self, k):
            return data[k]
    for shuffle, drop_last in ((True, False), (False, False), (True, True)):
        ld = torch.utils.data.DataLoader(DS(), batch_size=64, shuffle=shuffle, drop_last=drop_last)
        torch.manual_seed(5)
        seen = torch.cat([b[0] for b in ld]).tolist()
        after_iter = torch.get_rng_state()
        torch.manual_seed(5)
        order, bs = epoch_order(ld)
        assert order.tolist() == seen and bs == 64
        assert torch.equal(torch.get_rng_state(), after_iter)


def test_pack_records_layout_and_bounds():
    from mfcd.batching import pack_records
    rec = pack_records([[1, 2, 3, 0.25], [0, 5, 4, 1.0]], n=2, m=6)
    assert rec.dtype == np.int32 and rec.shape == (2, 4) and rec.flags.c_contiguous and rec.itemsize * 4 == 16
    assert rec[0, :3].tolist() == [1, 2, 3] and rec[:, 3].view(np.float32).tolist() == [0.25, 1.0]
    assert pack_records([[-1, -1, 0, 0.0]], n=2, m=6)[0, :3].tolist() == [1, 5, 0]  # Python-style negatives
    with pytest.raises(IndexError):
        pack_records([[2, 0, 1, 0.0]], n=2, m=6)
    with pytest.raises(IndexError):
        pack_records([[0, 6, 1, 0.0]], n=2, m=6)
    assert pack_records(np.zeros((0, 4)), 2, 2).shape == (0, 4)


REFERENCE_SIGNATURES = {
    # name: parameter list of the reference (structure.py:81-85, 306, 476, 533-534, 590, 666-669, 766, 812, 881, 925,
    # 958, 1085, 1154, 1203)
    "parameter_scan": ["n", "m", "d", "p", "s", "device", "lr", "weight_decay", "num_epochs", "reps", "strategy",
                       "open_browser", "linear", "K", "d1", "save_path", "save_every", "popularity_method", "alpha",
                       "soft_label", "generation"],
    "run_experiment": ["n", "m", "d", "p", "s", "device", "lr", "weight_decay", "reps", "num_epochs", "open_browser",
                       "K", "d1", "strategy", "popularity_method", "alpha", "soft_label", "generation"],
    "get_triplets_from_X": ["X", "num_triplets", "strategy", "exclude", "popularity_method", "alpha", "n_clusters"],
    "generate_X": ["n", "m", "d", "device", "generation", "kwargs"],
    "split_dataset_from_triplets": ["X", "num_triplets", "scale", "K", "train_ratio", "val_ratio", "batch_size",
                                    "strategy", "popularity_method", "alpha", "soft_label"],
    "train_model": ["model", "train_loader", "val_loader", "optimizer", "device", "num_epochs", "is_last",
                    "open_browser"],
    "evaluate_model": ["model", "test_loader", "device"],
    "compute_reconstruction_error": ["model", "X", "s"],
    "compute_alpha_and_norm_ratios": ["model", "X_init"],
    "compute_ground_truth_metrics": ["test_loader", "X", "device"],
    "evaluate_ground_truth": ["n", "m", "p", "d", "s", "device", "K", "reps", "strategy", "popularity_method",
                              "alpha", "soft_label", "generation"],
    "parameter_scan_ground_truth": ["n", "m", "p", "d", "s", "device", "K", "linear", "reps", "strategy",
                                    "popularity_method", "alpha", "soft_label", "generation"],
    "print_return_structure_types": ["obj", "prefix"],
}


def test_drop_in_module_keeps_reference_signatures():
    import structure as S
    for name, params in REFERENCE_SIGNATURES.items():
        assert list(inspect.signature(getattr(S, name)).parameters) == params, name
    mf = inspect.signature(S.MatrixFactorization.__init__).parameters
    assert list(mf)[:4] == ["self", "n_users", "n_items", "d"]
    assert all(p.default is not inspect.Parameter.empty for p in list(mf.values())[4:])  # extensions are optional (dtype)
    assert list(inspect.signature(S.BTLPreferenceDataset.__init__).parameters) == [
        "self", "triplets", "X", "scale", "K", "soft_label", "train"]
    d = inspect.signature(S.parameter_scan).parameters
    assert (d["n"].default, d["d"].default, d["lr"].default, d["weight_decay"].default, d["num_epochs"].default) == \
        (1000, 2, 1e-3, 1e-5, 30)
    assert inspect.signature(S.split_dataset_from_triplets).parameters["batch_size"].default == 64
    for name in ("choose_items_random", "choose_items_by_margin", "choose_items_by_popularity", "choose_items_top_k",
                 "choose_items_by_proximity", "choose_items_by_variance", "choose_items_by_svd_projection",
                 "choose_items_cluster_based", "choose_items_by_user_similarity", "generate_embeddings",
                 "generate_low_rank_matrix", "generate_gmm_embeddings"):
        assert callable(getattr(S, name)), name  # `from generation_data import *` re-export (structure.py:17)
    with pytest.raises(ValueError):
        S.get_triplets_from_X(torch.zeros(4, 4), 1, strategy="nope")
    with pytest.raises(ValueError):
        S.generate_X(4, 4, 2, "cpu", generation="nope")
    with pytest.raises(ValueError):
        S.parameter_scan(n=[4, 5], m=[4, 5, 6], linear=True)


def test_samplers_respect_uniqueness_and_exclude():
    import structure as S
    torch.manual_seed(0)
    np.random.seed(0)
    X = torch.randn(30, 20)
    for strategy in ("random", "popularity", "top_k", "proximity", "variance", "margin"):
        first = S.get_triplets_from_X(X, 40, strategy=strategy)
        assert isinstance(first, set) and len(first) <= 40
        assert all(0 <= u < 30 and 0 <= i < 20 and 0 <= j < 20 and i != j for u, i, j in first), strategy
        if strategy != "margin":
            assert len(first) == 40
            more = S.get_triplets_from_X(X, 20, strategy=strategy, exclude=first)
            assert not (more & first), strategy


def test_labels_follow_btl_statistics():
    import structure as S
    torch.manual_seed(1)
    X = torch.tensor([[2.0, -2.0], [0.0, 0.0]])
    ds = S.BTLPreferenceDataset([(0, 0, 1), (1, 0, 1)] * 2000, X, scale=1.0, K=1)
    lab = np.array([r[3] for r in ds.data]).reshape(-1, 2)
    assert abs(lab[:, 0].mean() - 1 / (1 + np.exp(-4.0))) < 0.02 and abs(lab[:, 1].mean() - 0.5) < 0.03
    soft = S.BTLPreferenceDataset([(0, 0, 1)] * 50, X, K=4, soft_label=True, train=True)
    assert len(soft) == 50 and all(r[3] in (0.0, 0.25, 0.5, 0.75, 1.0) for r in soft.data)
    hard = S.BTLPreferenceDataset([(0, 0, 1)] * 50, X, K=4, soft_label=True, train=False)
    assert len(hard) == 200 and all(r[3] in (0.0, 1.0) for r in hard.data)


@pytest.mark.parametrize("dim,k", [(40, 3), (257, 8), (64, 64), (5, 9)])
def test_haar_columns_equal_scipy_ortho_group(dim, k):
    """The panel form of the "base" generator draws the same normals and yields the same leading columns as
    scipy.stats.ortho_group.rvs (what generation_data.py:365-366 of the reference calls)."""
    import generation_data as G
    from scipy.stats import ortho_group
    np.random.seed(dim + k)
    want = ortho_group.rvs(dim=dim)[:, :k]
    after_full = np.random.normal()
    np.random.seed(dim + k)
    got = G._haar_columns(dim, k)
    assert np.random.normal() == after_full, "numpy RNG left in a different state"
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("n,m,k,n_excl", [(30, 30, 200, 0), (17, 23, 300, 50), (64, 8, 400, 100), (5, 4, 60, 0)])
def test_vectorised_random_sampler_equals_one_at_a_time_loop(n, m, k, n_excl):
    """Same triplets in the same list order and the same generator state as the reference's per-attempt loop
    (generation_data.py:16-26), including rejections (i == j, excluded, duplicate)."""
    import generation_data as G
    X = torch.zeros(n, m)
    torch.manual_seed(n * m + k)
    excl = set(G._choose_items_random_serial(n, m, n_excl, set()))
    torch.manual_seed(k)
    want = G._choose_items_random_serial(n, m, k, excl)
    state_want = torch.get_rng_state()
    torch.manual_seed(k)
    got = G.choose_items_random(X, k, excl)
    assert got == want
    assert torch.equal(torch.get_rng_state(), state_want)


def _sampler_call(G, strategy, X, want, excl, k, method, alpha):
    if strategy == "random":
        return G.choose_items_random(X, want, excl)
    if strategy == "proximity":
        return G.choose_items_by_proximity(X, want, excl, **({"k": k} if k > 0 else {}))
    if strategy == "popularity":
        return G.choose_items_by_popularity(X, want, excl, method=method, alpha=alpha)
    if strategy == "variance":
        return G.choose_items_by_variance(X, want, excl)
    if strategy == "cluster":
        return G.choose_items_cluster_based(X, want, excl, n_clusters=k)
    return G.choose_items_top_k(X, want, excl, **({"k": k} if k > 0 else {}))


def _golden_sampler_cases():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "samplers.npz"))
    return z, [str(x) for x in z["names"]]


@pytest.mark.parametrize("name", _golden_sampler_cases()[1])
def test_seeded_samplers_reproduce_the_reference_lists(name):
    """tests/golden/samplers.npz holds what the UNMODIFIED reference loops returned (oracle/make_golden_samplers.py:
    generation_data.py:16-26, 29-43, 87-99, 103-128, 189-224, 229-247): the bulk forms (and the two loops kept as loops) return the same triplets in the same list order
    and leave torch's and numpy's global generators in the same state (probed with one draw each)."""
    import generation_data as G
    z, _ = _golden_sampler_cases()
    n, m, want, seed, k = (int(v) for v in z[f"{name}.meta"])
    X = torch.from_numpy(z[f"{name}.X"])
    excl = set(map(tuple, z[f"{name}.exclude"].tolist()))
    torch.manual_seed(seed)
    np.random.seed(seed)
    got = _sampler_call(G, str(z[f"{name}.strategy"]), X, want, excl, k, str(z[f"{name}.method"]),
                        float(z[f"{name}.alpha"][0]))
    assert [list(t) for t in got] == z[f"{name}.triplets"].tolist()
    after = [float(torch.rand(1, dtype=torch.float64)), float(np.random.random_sample())]
    assert after == z[f"{name}.after"].tolist()


@pytest.mark.parametrize("strategy,n,m,want,n_excl,k", [
    ("proximity", 64, 150, 900, 100, 100), ("proximity", 300, 40, 2500, 0, 7), ("proximity", 9, 7, 40, 10, 3),
    ("top_k", 64, 150, 900, 100, None), ("top_k", 5, 6, 400, 0, None), ("top_k", 300, 64, 5000, 300, None),
    ("popularity", 50, 200, 3000, 200, None), ("popularity", 8, 5, 100, 20, None)])
def test_bulk_samplers_equal_their_one_at_a_time_loops(strategy, n, m, want, n_excl, k):
    """Sizes beyond the fixtures (several blocks, rejected words, exhausted attempt budgets): same list, same state of
    both generators as the restated per-attempt loops — which the fixtures above hold against the reference."""
    import generation_data as G
    X = torch.randn(n, m, generator=torch.Generator().manual_seed(n + m))
    probs = G._popularity_probs(m, "zipf", 1.5)
    serial = {"proximity": lambda w, e: G._choose_items_by_proximity_serial(X, w, e, k),
              "top_k": lambda w, e: G._choose_items_top_k_serial(X, w, e, k),
              "popularity": lambda w, e: G._choose_items_by_popularity_serial(n, m, probs, w, e)}[strategy]
    bulk = {"proximity": lambda w, e: G.choose_items_by_proximity(X, w, e, k),
            "top_k": lambda w, e: G.choose_items_top_k(X, w, e, k),
            "popularity": lambda w, e: G.choose_items_by_popularity(X, w, e)}[strategy]
    torch.manual_seed(1)
    np.random.seed(1)
    excl = set(serial(n_excl, set()))
    torch.manual_seed(want)
    np.random.seed(want)
    expect = serial(want, excl)
    state = (torch.get_rng_state(), np.random.get_state())
    torch.manual_seed(want)
    np.random.seed(want)
    got = bulk(want, excl)
    assert got == expect
    assert torch.equal(torch.get_rng_state(), state[0])
    now = np.random.get_state()
    assert np.array_equal(now[1], state[1][1]) and now[2] == state[1][2]


@pytest.mark.parametrize("n,m,want,n_excl,max_attempts", [
    (40, 30, 300, 0, 5_000_000), (40, 30, 300, 80, 5_000_000), (40, 30, 600, 0, 400), (6, 5, 110, 20, 200_700)])
@pytest.mark.parametrize("factored", [False, True])
def test_margin_sampler_equals_a_per_attempt_walk_over_the_same_draws(factored, n, m, want, n_excl, max_attempts,
                                                                      monkeypatch, capsys):
    """generation_data.py:46-84 draws from an unseeded numpy Generator; with `default_rng` replaced by a seeded one, the
    bulk form returns the list and prints the message of a walk, one attempt at a time, over the same draws: the same
    pass sizes, every attempt tested against `exclude` and the set so far, the counter advanced by blocks of 500 and
    stopped with the block that completes the request.  The last two cases spend their budget (in one pass, and in two
    with more asked than `exclude` leaves), so the warning is compared too."""
    import generation_data as G
    gen = torch.Generator().manual_seed(n + m + want)
    A, B = torch.randn(n, 4, generator=gen), torch.randn(m, 4, generator=gen)
    X = G.FactoredMatrix(A, B) if factored else A @ B.t()
    monkeypatch.setattr(np.random, "default_rng", lambda: np.random.Generator(np.random.PCG64(want + n_excl)))
    excl = set(G.choose_items_by_margin(X, want, set(), max_attempts=max_attempts)[:n_excl])
    assert len(excl) == n_excl
    capsys.readouterr()
    got = G.choose_items_by_margin(X, want, excl, max_attempts=max_attempts)
    printed = capsys.readouterr().out

    head = X.rows(0, min(10, n)) if factored else X[:min(10, n)].numpy()
    margin = np.mean(head.max(axis=1) - head.min(axis=1)) * want / (n * m)
    rng = np.random.default_rng()
    found, attempts = set(), 0
    while len(found) < want and attempts < max_attempts:
        size = 500 * max(1, min(400, -(-(max_attempts - attempts) // 500)))
        us = rng.integers(0, n, size=size)
        ij = rng.integers(0, m, size=(size, 2))
        close = np.abs(G._x_pair_diff(X, us, ij[:, 0], ij[:, 1])) <= margin
        for a, t in enumerate(zip(us.tolist(), ij[:, 0].tolist(), ij[:, 1].tolist())):
            if a % 500 == 0:
                if len(found) >= want:
                    break
                attempts += 500
            if len(found) < want and t[1] != t[2] and close[a] and t not in excl and t not in found:
                found.add(t)
    expect = "" if len(found) >= want else (
        f"⚠️ Only {len(found)} triplets generated (target={want}, margin={margin:.4f}) after {attempts} "
        f"attempts.maximum : {float((A if factored else X).max())}\n")
    assert got == list(found)
    assert printed == expect
    assert (len(found) < want) == (max_attempts < 5_000_000)


def test_svd_sampler_draws_distinct_allowed_triplets_from_the_top_sets():
    """generation_data.py:131-179 (unseeded numpy Generator: no draw order to keep): every triplet comes from the
    top-30 % users / items by projection norm, is unique, respects `exclude`, and a request larger than the support
    ends at the reference's 5x attempt budget with its warning."""
    import generation_data as G
    import scipy.sparse.linalg as spla
    torch.manual_seed(5)
    X = torch.randn(60, 8) @ torch.randn(8, 90)
    want = 1500
    got = G.choose_items_by_svd_projection(X, want, set())
    assert len(got) == len(set(got)) == want and all(i != j for _, i, j in got)
    rank = int(want / (60 * 90) * 90)
    Us, S, Vt = spla.svds(X.numpy(), k=rank)
    top_u = set(np.argsort(np.linalg.norm(Us * S, axis=1))[-18:].tolist())
    top_i = set(np.argsort(np.linalg.norm(Vt.T * S, axis=1))[-27:].tolist())
    assert {u for u, _, _ in got} <= top_u and {i for _, i, _ in got} | {j for _, _, j in got} <= top_i
    more = G.choose_items_by_svd_projection(X, want, set(got))
    assert not set(more) & set(got)


def _golden_generator_cases():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "generators.npz"))
    return z, [str(c) for c in z["cases"]]


@pytest.mark.parametrize("k,case", list(enumerate(_golden_generator_cases()[1])))
def test_ground_truth_generators_reproduce_the_reference_matrices(k, case, monkeypatch):
    """tests/golden/generators.npz holds what the UNMODIFIED reference's generate_X returned per `generation` keyword
    under fixed torch / numpy / `random` seeds (oracle/make_golden_generators.py; structure.py:590-663 over
    generation_data.py:346-715): the restated generators draw in the same order and return the same matrix, and leave
    the three generators in the same state.  (The host side of generate_X is device-agnostic: built on the CPU here.)
    The one `torch.svd` call ("svd") is replayed from the fixture after its argument is checked bit for bit: the signs
    and last bits of a LAPACK SVD differ between hosts (CPU model, math-library code path), and the matrix with them."""
    import random
    import generation_data as G
    z, _ = _golden_generator_cases()
    g, n, m, d, rank = case.split(":")
    n, m, d, rank = int(n), int(m), int(d), int(rank)
    svd_calls = []
    if f"{k}.svd_in" in z.files:
        live_svd = torch.svd

        def replay_svd(a, *args, **kw):
            np.testing.assert_array_equal(a.numpy(), z[f"{k}.svd_in"])
            svd_calls.append(a)
            # the live call's memory layout (LAPACK's column-major factors: torch's randn_like draws in layout order)
            live = live_svd(a, *args, **kw)
            return tuple(torch.empty_strided(t.shape, t.stride(), dtype=t.dtype).copy_(
                torch.from_numpy(z[f"{k}.svd_{w}"])) for t, w in zip(live, "USV"))
        monkeypatch.setattr(torch, "svd", replay_svd)
    torch.manual_seed(300 + k)
    np.random.seed(300 + k)
    random.seed(300 + k)
    if g == "base":
        X = G.generate_embeddings(n, m, d, device="cpu")
    elif g == "low_rank":
        A, B, S = G.generate_low_rank_matrix(n, m, d, rank=rank if rank > 0 else d, device="cpu")
        X = (A * S) @ B.t()
    elif g == "clustered":
        X = G.generate_clustered_matrix_from_embeddings(n, m, d, device="cpu")
    else:
        A, B = getattr(G, f"generate_{g}_embeddings")(n, m, d, device="cpu")
        X = A @ B.t()
    want = z[f"{k}.X"]
    assert len(svd_calls) == (1 if f"{k}.svd_in" in z.files else 0)
    assert tuple(X.shape) == want.shape
    np.testing.assert_allclose(X.numpy(), want, rtol=0, atol=1e-6 * max(1.0, float(np.abs(want).max())))
    after = [float(torch.rand(1, dtype=torch.float64)), float(np.random.random_sample()), random.random()]
    assert after == z[f"{k}.after"].tolist()


def test_graph_generator_is_the_one_documented_deviation():
    """The reference raises TypeError for generation="graph" (recorded in the fixture: a stray comma makes `noise` a
    tuple, generation_data.py:565); the restated generator implements the evident intent instead — stated in its
    docstring — and must at least return finite factors of the right shapes."""
    import generation_data as G
    z, _ = _golden_generator_cases()
    assert str(z["graph_raises"]) == "TypeError"
    torch.manual_seed(0)
    A, B = G.generate_graph_embeddings(12, 9, 5, device="cpu")
    assert A.shape == (12, 5) and B.shape == (9, 5) and bool(torch.isfinite(A).all()) and bool(torch.isfinite(B).all())


def test_dataset_rows_and_lazy_data_list():
    import structure as S
    from mfcd.batching import dataset_records
    torch.manual_seed(3)
    X = torch.randn(6, 5)
    trip = [(0, 1, 2), (5, 4, 0), (3, 3, 1)]
    ds = S.BTLPreferenceDataset(trip, X, K=2)
    assert len(ds) == 6 and ds[1][:3] == (0, 1, 2) and isinstance(ds[1][3], float) and isinstance(ds[1][0], int)
    rows = dataset_records(ds)
    assert rows.shape == (6, 4) and rows.dtype == np.float64
    data = ds.data                                   # materialises the reference's list of tuples
    assert isinstance(data, list) and data[2][:3] == (5, 4, 0) and all(type(v) is int for v in data[2][:3])
    np.testing.assert_array_equal(np.asarray(data), rows)
    ds.data[0] = (1, 1, 1, 0.5)                      # callers may edit the list; the device path must see it
    assert dataset_records(ds)[0].tolist() == [1.0, 1.0, 1.0, 0.5] and ds[0] == (1, 1, 1, 0.5)
    ds.data = [(2, 2, 3, 1.0)]
    assert len(ds) == 1 and dataset_records(ds).tolist() == [[2.0, 2.0, 3.0, 1.0]]


class _OnGpu(torch.Tensor):
    """A CPU tensor that answers `is_cuda`: `row_pair` reads shapes, dtypes and strides and touches no memory."""
    is_cuda = property(lambda self: True)


def test_row_pair_checks_and_leading_dimensions():
    from mfcd import _lib
    m = 5
    A, X = torch.zeros(3, m), torch.ones(3, m)
    for a, x in ((A, X),                                                    # CPU tensors
                 (A.as_subclass(_OnGpu), X),
                 (A.as_subclass(_OnGpu), X.double().as_subclass(_OnGpu)),   # dtype mismatch
                 (A.as_subclass(_OnGpu), X[:, :-1].as_subclass(_OnGpu)),    # shape mismatch
                 (A.as_subclass(_OnGpu), None)):
        with pytest.raises(_lib.MfcdError, match=r"somebody needs two float32 GPU matrices of the same shape \(no CPU fallback\)"):
            _lib.row_pair(a, x, "somebody")
    wide = torch.arange(3 * 2 * m, dtype=torch.float32).reshape(3, 2 * m).as_subclass(_OnGpu)
    a, x, rows, cols, lda, ldx = _lib.row_pair(wide[:, :m], X.as_subclass(_OnGpu), "somebody")
    assert (rows, cols, lda, ldx) == (3, m, 2 * m, m) and a.data_ptr() == wide.data_ptr()       # a view: no copy
    a, x, rows, cols, lda, ldx = _lib.row_pair(wide[1:2, :m], X[1:2].as_subclass(_OnGpu), "somebody")
    assert (rows, cols, lda, ldx) == (1, m, m, m)                          # one row: its stride says nothing
    a, x, rows, cols, lda, ldx = _lib.row_pair(wide[:, 0:2 * m:2], X.as_subclass(_OnGpu), "somebody")
    assert (lda, ldx) == (m, m) and a.is_contiguous() and torch.equal(a, wide[:, 0:2 * m:2])   # column stride 2: copied


def test_score_matrix_resolver_on_host_objects():
    from mfcd import rows, topk
    for bad in (None, 3.5, "X", [1, 2, 3], object()):
        with pytest.raises(TypeError, match="X must be a dense GPU tensor, a FactoredMatrix or a pair"):
            rows.resolve(bad)
        with pytest.raises(TypeError, match="X must be a dense GPU tensor, a FactoredMatrix or a pair"):
            topk.topk_rows(bad, 1)

    class Duck:
        A, B, shape = torch.zeros(7, 3, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64), (7, 4)

    X = rows.resolve(Duck())
    assert (X.n, X.m, X.d, X.factored, X.dense) == (7, 4, 3, True, None) and X.device.type == "cpu"
    assert X.A.dtype == torch.float64                                       # moved and checked, never converted
    assert torch.equal(X.rows(2, 5), Duck.A[2:5] @ Duck.B.t()) and X.rows(torch.tensor([6, 0, 6])).shape == (3, 4)
    D = rows.resolve(torch.arange(12.0).reshape(3, 4))
    assert (D.n, D.m, D.d, D.factored) == (3, 4, 0, False) and torch.equal(D.rows(1, 3), D.dense[1:3])
    P = rows.resolve((Duck.A, Duck.B))
    assert (P.n, P.m, P.d) == (7, 4, 3)
    with pytest.raises(ValueError):
        rows.resolve((Duck.A, torch.ones(4, 2)))                            # inner dimensions differ
    with pytest.raises(ValueError):
        rows.resolve(torch.zeros(5))
    assert rows.blocks(70, 32) == [(0, 32), (32, 64), (64, 70)] and rows.blocks(0, 32) == []
