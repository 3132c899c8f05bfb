"""Many small models per launch (mfcd.engine.fit_many, structure.train_models / set_concurrent_experiments, include/mfcd.h:
mfcd_train_steps_local_multi, mfcd_eval_batches_multi): every model's results bit-identical to training it alone."""
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import load_golden

MFCD_EINVAL, MFCD_ESTATE = -1, -6


class ArrayDataset(torch.utils.data.Dataset):
    """(u, i, j, z) rows kept as a float64 [N, 4] array (what the device path uploads)."""

    def __init__(self, rows):
        self.data = np.ascontiguousarray(rows, dtype=np.float64)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, k):
        r = self.data[k]
        return int(r[0]), int(r[1]), int(r[2]), float(r[3])


def _rows(rng, n, m, N, soft=False):
    u, i = rng.integers(0, n, N), rng.integers(0, m, N)
    j = (i + 1 + rng.integers(0, m - 1, N)) % m
    z = rng.integers(0, 4, N) / 3.0 if soft else rng.integers(0, 2, N).astype(np.float64)
    return np.stack([u, i, j, z], 1).astype(np.float64)


def _case(seed, n, m, d, N, B, lr=1e-3, wd=1e-5, soft=False, Nv=None, dtype=torch.float32, opt="adam"):
    """(initial U, V, loaders, optimiser factory) of one model; `make()` returns a fresh (model, optimizer) pair."""
    import structure as S
    rng = np.random.default_rng(seed)
    U0 = torch.from_numpy((rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32))
    V0 = torch.from_numpy((rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32))
    train = torch.utils.data.DataLoader(ArrayDataset(_rows(rng, n, m, N, soft)), batch_size=B, shuffle=True)
    val = torch.utils.data.DataLoader(ArrayDataset(_rows(rng, n, m, N // 8 if Nv is None else Nv)), batch_size=B,
                                      shuffle=False)

    def make():
        model = S.MatrixFactorization(n, m, d, dtype=dtype)
        with torch.no_grad():
            model.U.copy_(U0.to(dtype))
            model.V.copy_(V0.to(dtype))
        model = model.to("cuda")
        if opt == "sgd":
            o = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=wd)
        else:
            o = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
        return model, o
    return make, train, val


def _state(model, opt):
    st = [model.U.data.clone(), model.V.data.clone()]
    for p in (model.U, model.V):
        s = opt.state[p]
        st += [s[k].clone() for k in sorted(s) if isinstance(s[k], torch.Tensor)]
    return st


def _serial_vs_batched(cases, epochs, seed=7):
    """Train every case serially with train_model and together with train_models from the same RNG state; assert
    bit-identical losses, tables, optimizer state and RNG state afterwards.  Returns the batched models."""
    import structure as S
    # (the models are made first: MatrixFactorization's initial draw would otherwise move the epoch orders)
    serial_pairs = [make() for make, _, _ in cases]
    pairs = [make() for make, _, _ in cases]
    torch.manual_seed(seed)
    before = torch.get_rng_state()
    serial = []
    for (model, opt), (_, train, val) in zip(serial_pairs, cases):
        out = S.train_model(model, train, val, opt, "cuda", num_epochs=epochs)
        serial.append((out, _state(model, opt)))
    after_serial = torch.get_rng_state()
    torch.set_rng_state(before)
    outs = S.train_models([p[0] for p in pairs], [c[1] for c in cases], [c[2] for c in cases], [p[1] for p in pairs],
                          "cuda", num_epochs=epochs)
    assert torch.equal(torch.get_rng_state(), after_serial), "RNG stream diverged"
    assert len(outs) == len(cases)
    for r, ((ref_out, ref_state), out, (model, opt)) in enumerate(zip(serial, outs, pairs)):
        assert out[0] == ref_out[0], f"model {r}: train losses"
        assert out[1] == ref_out[1], f"model {r}: val losses"
        assert all(isinstance(x, float) for x in out[0] + out[1])
        got = _state(model, opt)
        assert len(got) == len(ref_state)
        for k, (a, b) in enumerate(zip(got, ref_state)):
            assert torch.equal(a, b), f"model {r}: state tensor {k}"
        assert not model.training
    return pairs


# --------------------------------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------------------------------
def test_new_names_exist_and_reference_signatures_are_untouched():
    import structure as S
    from mfcd import batching, engine
    from test_host_logic import REFERENCE_SIGNATURES
    for name, params in REFERENCE_SIGNATURES.items():
        assert list(inspect.signature(getattr(S, name)).parameters) == params, name
    assert list(inspect.signature(S.train_models).parameters) == [
        "models", "train_loaders", "val_loaders", "optimizers", "device", "num_epochs"]
    assert inspect.signature(S.train_models).parameters["num_epochs"].default == 100
    assert list(inspect.signature(S.set_concurrent_experiments).parameters) == ["k"]
    assert list(inspect.signature(engine.fit_many).parameters) == [
        "models", "train_loaders", "val_loaders", "optimizers", "num_epochs", "orders"]
    assert callable(batching.draw_orders) and callable(engine.batched_applies)


def test_concurrent_experiments_default_to_one():
    import structure as S
    assert S._CONCURRENT == 1
    for bad in (0, -2, 1.5, True, "3"):
        with pytest.raises(ValueError):
            S.set_concurrent_experiments(bad)
    S.set_concurrent_experiments(4)
    try:
        assert S._CONCURRENT == 4
    finally:
        S.set_concurrent_experiments(1)
    assert S._CONCURRENT == 1


def test_descriptor_mirrors_match_the_library():
    from mfcd import _lib, engine
    L = _lib.load()
    assert L.mfcd_local_model_bytes() == ctypes.sizeof(_lib.LocalModel) == 136
    assert L.mfcd_eval_model_bytes() == ctypes.sizeof(_lib.EvalModel) == 64
    assert engine._numpy_mirror(_lib.LocalModel).itemsize == ctypes.sizeof(_lib.LocalModel)
    assert engine._numpy_mirror(_lib.EvalModel).itemsize == ctypes.sizeof(_lib.EvalModel)
    # the numpy mirror writes the fields where the C struct has them
    tab = np.zeros(2, dtype=engine._numpy_mirror(_lib.LocalModel))
    tab["N"], tab["step0"], tab["d"], tab["lr"], tab["loss_per_step"] = [5, 6], [7, 8], [2, 3], [0.5, 0.25], [64, 128]
    c = (_lib.LocalModel * 2).from_buffer_copy(tab.tobytes())
    assert (c[1].N, c[1].step0, c[1].d, c[1].lr, c[1].loss_per_step) == (6, 8, 3, 0.25, 128)


def _host_table(n, m, d, N=640, B=64):
    from mfcd import _lib, engine
    tab = np.zeros(1, dtype=engine._numpy_mirror(_lib.LocalModel))
    for k, name in enumerate(("U", "V", "mU", "vU", "mV", "vV", "samples", "loss_per_step")):
        tab[name] = 4096 * (k + 1)          # never dereferenced: the host rejects the call first
    tab["N"], tab["B"], tab["n"], tab["m"], tab["d"] = N, B, n, m, d
    tab["lr"], tab["beta1"], tab["beta2"], tab["eps"] = 1e-3, 0.9, 0.999, 1e-8
    return tab


def test_multi_entry_validates_on_the_host():
    """A model the local form does not take is refused before anything is looked up or launched; a valid table on an
    unregistered workspace is refused too (both without a GPU)."""
    from mfcd import _lib
    L = _lib.load()
    ok = _host_table(256, 256, 8)
    both = np.concatenate([ok, _host_table(1000, 1000, 8)])
    fake_ws = 1 << 20
    assert L.mfcd_train_steps_local_multi(both.ctypes.data, 2, fake_ws, 1 << 30, None) == MFCD_EINVAL
    assert L.mfcd_train_steps_local_multi(ok.ctypes.data, 1, fake_ws, 1 << 30, None) == MFCD_ESTATE
    assert L.mfcd_train_steps_local_multi(ok.ctypes.data, 0, fake_ws, 1 << 30, None) == MFCD_EINVAL
    big_batch = _host_table(64, 64, 8, B=512)          # 3B hits > 2 per lane group of 8 lanes
    assert L.mfcd_train_steps_local_multi(big_batch.ctypes.data, 1, fake_ws, 1 << 30, None) == MFCD_EINVAL
    stage = ctypes.c_size_t(0)
    total = L.mfcd_train_local_multi_workspace_bytes(both.ctypes.data, 2, ctypes.byref(stage))
    assert total >= stage.value + 4 * (640 + 640) and stage.value >= 2 * 136
    assert L.mfcd_eval_multi_workspace_bytes(0, None) == 0
    assert L.mfcd_eval_multi_workspace_bytes(3, ctypes.byref(stage)) >= stage.value >= 3 * 64


def test_order_predraw_equals_consecutive_epoch_orders():
    from mfcd.batching import draw_orders, epoch_order
    train = torch.utils.data.DataLoader(ArrayDataset(np.zeros((37, 4))), batch_size=8, shuffle=True)
    val = torch.utils.data.DataLoader(ArrayDataset(np.zeros((11, 4))), batch_size=4, shuffle=False)
    torch.manual_seed(3)
    ref = []
    for _ in range(4):
        ref.append(epoch_order(train))
        ref.append(epoch_order(val))
    end = torch.get_rng_state()
    torch.manual_seed(3)
    got = draw_orders(train, val, 4)
    assert torch.equal(torch.get_rng_state(), end)
    assert len(got) == len(ref) == 8
    for (a, ba), (b, bb) in zip(got, ref):
        assert ba == bb and torch.equal(a, b)
    assert draw_orders(train, val, 0) == []


# --------------------------------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------------------------------
@pytest.fixture(params=["fast", "ieee"])
def flavour(request):
    from mfcd import _lib, engine
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    _lib.load()
    engine.set_resident_math(request.param)
    yield request.param
    engine.set_resident_math("fast")


def _mixed_shapes():
    return [_case(1, 256, 256, 8, 1310, 64),                          # C1
            _case(2, 1000, 1000, 2, 2000, 64),                        # the notebooks' default shape
            _case(3, 120, 90, 5, 700, 64, soft=True, lr=3e-3),       # d = 5, soft labels
            _case(4, 300, 200, 1, 900, 200, wd=1e-3),                 # d = 1, B = 200
            _case(5, 150, 150, 2, 1000, 200, lr=5e-3, wd=0.0),        # B = 200
            _case(6, 40, 70, 16, 333, 64, lr=2e-3, wd=1e-4, Nv=0)]    # no validation records


@pytest.mark.gpu
def test_batched_training_equals_serial_training(flavour):
    from mfcd import engine
    cases = _mixed_shapes()
    for make, train, val in cases:
        model, opt = make()
        assert engine.batched_applies(model, opt, len(train.dataset), train.batch_size)
    _serial_vs_batched(cases, epochs=3)


@pytest.mark.gpu
def test_batched_fixtures_match_the_reference_goldens():
    """The three e2e fixtures trained together in ONE fit_many call (5, 3 and 3 epochs), each with the orders its own
    fixture's RNG state draws, against the reference's results at the tolerances of the single-model e2e test."""
    import structure as S
    from mfcd import engine
    from mfcd.batching import draw_orders
    names = ["e2e_c1.npz", "e2e_soft_k3.npz", "e2e_hard_k2_d16.npz"]
    gs = [load_golden(nm) for nm in names]
    models, opts, trains, vals, orders, epochs = [], [], [], [], [], []
    for g in gs:
        model = S.MatrixFactorization(g["U0"].shape[0], g["V0"].shape[0], g["U0"].shape[1])
        with torch.no_grad():
            model.U.copy_(torch.from_numpy(g["U0"]))
            model.V.copy_(torch.from_numpy(g["V0"]))
        model = model.to("cuda")
        opt = torch.optim.Adam(model.parameters(), lr=float(g["lr"]), weight_decay=float(g["wd"]))
        train = torch.utils.data.DataLoader(ArrayDataset(g["train_data"]), batch_size=64, shuffle=True)
        val = torch.utils.data.DataLoader(ArrayDataset(g["val_data"]), batch_size=64, shuffle=False)
        torch.set_rng_state(torch.from_numpy(g["rng_state_before_train"]))
        orders.append(draw_orders(train, val, int(g["epochs"])))
        assert bool((torch.get_rng_state().numpy() == g["rng_state_after_train"]).all()), "RNG stream diverged"
        assert engine.batched_applies(model, opt, len(train.dataset), 64)
        models.append(model); opts.append(opt); trains.append(train); vals.append(val); epochs.append(int(g["epochs"]))
    outs = engine.fit_many(models, trains, vals, opts, epochs, orders=orders)
    for g, (tl, vl), model, opt in zip(gs, outs, models, opts):
        lr = float(g["lr"])
        assert len(tl) == len(vl) == int(g["epochs"])
        np.testing.assert_allclose(tl, g["train_losses"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(vl, g["val_losses"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(model.U.data.cpu().numpy(), g["U_final"], rtol=0, atol=2e-3 * lr)
        np.testing.assert_allclose(model.V.data.cpu().numpy(), g["V_final"], rtol=0, atol=2e-3 * lr)
        assert float(opt.state[model.U]["step"]) == float(g["adam_step"])


@pytest.mark.gpu
def test_mixed_batch_keeps_every_model_identical_to_serial():
    """Models the batched launch does not take (bf16 factors, a non-Adam optimiser, a resident-form shape) train alone
    in their place; the rest together — all identical to serial training."""
    from mfcd import engine
    cases = [_case(11, 256, 256, 8, 1310, 64),
             _case(12, 64, 48, 4, 500, 64, dtype=torch.bfloat16),
             _case(13, 80, 60, 4, 400, 64, opt="sgd", lr=1e-2),
             _case(14, 1000, 1000, 8, 1500, 64),
             _case(15, 1000, 1000, 2, 1200, 64, lr=2e-3)]
    taken = []
    for make, train, val in cases:
        model, opt = make()
        taken.append(engine.batched_applies(model, opt, len(train.dataset), train.batch_size))
    assert taken == [True, False, False, False, True]
    _serial_vs_batched(cases, epochs=2, seed=11)


@pytest.mark.gpu
def test_more_models_than_compute_units():
    cases = [_case(100 + r, 20 + r % 7, 18 + r % 5, 1 + r % 3, 150 + r % 50, 32 + 8 * (r % 5), lr=1e-3 * (1 + r % 4))
             for r in range(300)]
    _serial_vs_batched(cases, epochs=2, seed=5)


def _equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")
    if isinstance(a, float) and isinstance(b, float) and a != a:
        return b != b
    return type(a) is type(b) and a == b


def _rng_states():
    return torch.get_rng_state(), np.random.get_state()


def _same_rng(x, y):
    assert torch.equal(x[0], y[0]), "torch RNG state"
    assert x[1][0] == y[1][0] and np.array_equal(x[1][1], y[1][1]) and x[1][2:] == y[1][2:], "numpy RNG state"


@pytest.mark.gpu
def test_concurrent_experiments_equal_the_serial_run(tmp_path):
    import structure as S
    kw = dict(n=40, m=30, d=2, p=0.5, s=1.0, device="cuda", lr=1e-3, weight_decay=1e-5, reps=3, num_epochs=2)
    runs = []
    for k in (1, 3):
        S.set_concurrent_experiments(k)
        try:
            torch.manual_seed(21)
            np.random.seed(21)
            res = S.run_experiment(**kw)
            runs.append((res, _rng_states()))
        finally:
            S.set_concurrent_experiments(1)
    (a, ra), (b, rb) = runs
    assert a.keys() == b.keys()
    for key in a:
        assert len(a[key]) == 3 and _equal(a[key], b[key]), key
    _same_rng(ra, rb)

    files = []
    for k in (1, 3):
        path = str(tmp_path / f"scan_k{k}.pkl")
        S.set_concurrent_experiments(k)
        try:
            torch.manual_seed(4)
            np.random.seed(4)
            ret = S.parameter_scan(n=40, m=30, d=[2, 3], p=0.5, device="cuda", num_epochs=[1, 2], reps=2,
                                   save_path=path, save_every=1)
            files.append((path, ret, _rng_states()))
        finally:
            S.set_concurrent_experiments(1)
    (pa, reta, ra), (pb, retb, rb) = files
    assert reta == retb == []
    with open(pa, "rb") as f:
        la = pickle.load(f)
    with open(pb, "rb") as f:
        lb = pickle.load(f)
    assert len(la) == 4 and _equal(la, lb)
    with open(pa, "rb") as f, open(pb, "rb") as g:
        assert f.read() == g.read()
    _same_rng(ra, rb)
    assert os.path.getsize(pa) > 0


@pytest.mark.gpu
def test_multi_entry_rejects_a_non_local_model_and_touches_nothing():
    from mfcd import _lib, engine
    L = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    tabs = []
    for n, m, d in ((256, 256, 8), (1000, 1000, 8)):         # the second one is on the resident form
        t = [torch.randn(r, d, generator=g).to(dev) for r in (n, m, n, n, m, m)]
        tabs.append((n, m, d, t))
    rec = torch.zeros((640, 4), dtype=torch.int32, device=dev)
    loss = torch.full((16,), 7.0, device=dev)
    tv = np.zeros(2, dtype=engine._numpy_mirror(_lib.LocalModel))
    for r, (n, m, d, t) in enumerate(tabs):
        for name, x in zip(("U", "V", "mU", "vU", "mV", "vV"), t):
            tv[name][r] = x.data_ptr()
        tv["samples"][r], tv["loss_per_step"][r] = rec.data_ptr(), loss.data_ptr()
        tv["N"][r], tv["B"][r], tv["n"][r], tv["m"][r], tv["d"][r] = 640, 64, n, m, d
        tv["lr"][r], tv["beta1"][r], tv["beta2"][r], tv["eps"][r] = 1e-3, 0.9, 0.999, 1e-8
    stage = ctypes.c_size_t(0)
    nbytes = L.mfcd_train_local_multi_workspace_bytes(tv.ctypes.data, 2, ctypes.byref(stage))
    ws = engine._multi_workspace(L, nbytes, stage.value, dev)
    before = [[x.clone() for x in t] for _, _, _, t in tabs]
    try:
        assert L.mfcd_train_steps_local_multi(tv.ctypes.data, 2, ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr(dev)) == MFCD_EINVAL
        torch.cuda.synchronize()
        for (_, _, _, t), b in zip(tabs, before):
            assert all(torch.equal(x, y) for x, y in zip(t, b))
        assert bool((loss == 7.0).all())
        # the valid model alone goes through, and does update its tables
        assert L.mfcd_train_steps_local_multi(tv[:1].copy().ctypes.data, 1, ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr(dev)) == 0
        torch.cuda.synchronize()
        assert not torch.equal(tabs[0][3][0], before[0][0])
        assert all(torch.equal(x, y) for x, y in zip(tabs[1][3], before[1]))
    finally:
        L.mfcd_train_workspace_release(ws.data_ptr())
