"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C-ABI, against
(a) golden vectors from the unmodified reference and (b) the CPU oracle on the same seeded inputs.

Stated fp32 tolerances (the GPU sums a d-term dot product in wave-shuffle order, ATen in SIMD order,
and hipcc contracts a*b+c into FMA; everything else is the same arithmetic):
  sigmoid outputs / losses      rtol 2e-5, atol 2e-7
  parameters after k steps      atol 2e-3*lr (= 2e-6 at lr 1e-3; k <= 5 epochs of C1), moments rtol 1e-3
  epoch losses                  atol 2e-6
  dense metrics                 atol 1e-4 (the north-star bound), typically < 1e-6
"""
import numpy as np
import pytest
import torch

from conftest import E2ES, KATS, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()  # fail loudly if the HIP library is not built
    return torch.device("cuda:0")


def form_applies(N, B, n, m, d):
    """Whether the form the `path` fixture has forced takes a call of these sizes: the library's own answer
    (engine.train_plan = mfcd_train_plan_query under the forced path; MFCD_EINVAL means "does not apply")."""
    from mfcd import _lib, engine
    try:
        engine.train_plan(N, B, n, m, d)
    except _lib.MfcdError as e:
        assert str(e) == _lib.load().mfcd_error_string(-1).decode(), e      # MFCD_EINVAL, nothing else
        return False
    return True


@pytest.fixture(params=["streaming", "resident", "resident-ieee", "local"])
def path(request, dev):
    """Run a training test once per form of the fused step (include/mfcd.h: mfcd_set_train_path), the resident form
    in both arithmetic flavours (mfcd_set_resident_math: fast is the default)."""
    from mfcd import engine
    form = request.param.split("-")[0]
    engine.set_train_path(form)
    engine.set_resident_math("ieee" if request.param.endswith("ieee") else "fast")
    yield form
    engine.set_train_path("auto")
    engine.set_resident_math("fast")


def _model_from(U0, V0, dev, lr, wd):
    import structure as S
    n, d = U0.shape
    model = S.MatrixFactorization(n, V0.shape[0], d)
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(U0))
        model.V.copy_(torch.from_numpy(V0))
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
    return model, opt


def _records(u, i, j, z, n, m, dev):
    from mfcd.engine import SampleStore
    rows = np.stack([np.asarray(u, np.float64), np.asarray(i, np.float64), np.asarray(j, np.float64),
                     np.asarray(z, np.float64)], 1)
    return SampleStore(rows, n, m, dev)


class ListDataset(torch.utils.data.Dataset):
    def __init__(self, rows):
        self.data = [(int(r[0]), int(r[1]), int(r[2]), float(r[3])) for r in rows]

    def __len__(self):
        return len(self.data)

    def __getitem__(self, k):
        return self.data[k]


# --------------------------------------------------------------------------------------------------
# (a) golden vectors
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KATS)
def test_kat_steps_match_reference(dev, path, name):
    from mfcd import engine
    g = load_golden(name)
    (n, d), m = g["U0"].shape, g["V0"].shape[0]
    if not all(form_applies(len(g[f"u{k}"]), len(g[f"u{k}"]), n, m, d) for k in range(int(g["n_steps"]))):
        assert path in ("resident", "local"), "the streaming form takes every shape"
        pytest.skip({"resident": "resident form needs d to be a power of two",
                     "local": "local form needs (n+m)*d <= 8192"}[path])
    lr, wd = float(g["lr"]), float(g["wd"])
    model, opt = _model_from(g["U0"], g["V0"], dev, lr, wd)
    bind = engine.AdamBinding(model, opt)
    n, m = g["U0"].shape[0], g["V0"].shape[0]
    for k in range(int(g["n_steps"])):
        st = _records(g[f"u{k}"], g[f"i{k}"], g[f"j{k}"], g[f"z{k}"], n, m, dev)
        _, _, p = engine.eval_batches(model.U.data, model.V.data, st.dev, st.N, want_p=True)
        np.testing.assert_allclose(p.cpu().numpy(), g[f"p{k}"], rtol=RTOL, atol=ATOL)
        loss = engine.train_steps(bind, st.dev, st.N)
        assert loss.numel() == 1
        ref_loss = float(g[f"loss{k}"])
        assert abs(float(loss[0]) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
        su, sv = opt.state[model.U], opt.state[model.V]
        np.testing.assert_allclose(model.U.data.cpu().numpy(), g[f"U{k + 1}"], rtol=1e-6, atol=2e-7)
        np.testing.assert_allclose(model.V.data.cpu().numpy(), g[f"V{k + 1}"], rtol=1e-6, atol=2e-7)
        np.testing.assert_allclose(su["exp_avg"].cpu().numpy(), g[f"mU{k + 1}"], rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(sv["exp_avg"].cpu().numpy(), g[f"mV{k + 1}"], rtol=1e-4, atol=1e-9)
        np.testing.assert_allclose(su["exp_avg_sq"].cpu().numpy(), g[f"vU{k + 1}"], rtol=2e-4, atol=1e-13)
        np.testing.assert_allclose(sv["exp_avg_sq"].cpu().numpy(), g[f"vV{k + 1}"], rtol=2e-4, atol=1e-13)
        assert float(su["step"]) == k + 1 == float(sv["step"])


def test_saturated_terms_and_zero_gradient(dev):
    """p rounds to 0/1 -> loss term exactly 100 and zero sparse gradient (weight decay only)."""
    from mfcd import engine
    g = load_golden("kat_saturated_d8.npz")
    model, opt = _model_from(g["U0"], g["V0"], dev, float(g["lr"]), float(g["wd"]))
    st = _records(g["u0"], g["i0"], g["j0"], g["z0"], 24, 24, dev)
    _, _, p = engine.eval_batches(model.U.data, model.V.data, st.dev, st.N, want_p=True)
    p = p.cpu().numpy()
    sat = (g["p0"] == 0.0) | (g["p0"] == 1.0)
    assert sat.sum() >= 5
    np.testing.assert_array_equal(p[sat], g["p0"][sat])


@pytest.mark.parametrize("name", E2ES)
def test_e2e_train_eval_metrics_match_reference(dev, path, name):
    """train_model / evaluate_model / metric functions of the drop-in module on the reference's own data."""
    import structure as S
    g = load_golden(name)
    lr, wd, E, s = float(g["lr"]), float(g["wd"]), int(g["epochs"]), float(g["s"])
    model, opt = _model_from(g["U0"], g["V0"], dev, lr, wd)
    mk = lambda rows, sh: torch.utils.data.DataLoader(ListDataset(rows), batch_size=64, shuffle=sh)  # noqa: E731
    train, val, test = mk(g["train_data"], True), mk(g["val_data"], False), mk(g["test_data"], False)
    torch.set_rng_state(torch.from_numpy(g["rng_state_before_train"]))
    tl, vl = S.train_model(model, train, val, opt, "cuda", num_epochs=E)
    assert bool((torch.get_rng_state().numpy() == g["rng_state_after_train"]).all()), "RNG stream diverged"
    np.testing.assert_allclose(tl, g["train_losses"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(vl, g["val_losses"], rtol=0, atol=2e-6)
    assert isinstance(tl, list) and isinstance(tl[0], float) and len(tl) == E
    U, V = model.U.data.cpu().numpy(), model.V.data.cpu().numpy()
    ptol = 2e-3 * lr  # parameter differences scale with the step size: 2e-6 at the default lr = 1e-3
    np.testing.assert_allclose(U, g["U_final"], rtol=0, atol=ptol)
    np.testing.assert_allclose(V, g["V_final"], rtol=0, atol=ptol)
    # north-star: UV^T reconstruction MSE vs the reference's factors
    mse = float(np.mean((U @ V.T - g["U_final"] @ g["V_final"].T) ** 2))
    assert mse < 1e-10
    assert float(opt.state[model.U]["step"]) == float(g["adam_step"])
    te_loss, te_acc = S.evaluate_model(model, test, "cuda")
    assert te_loss == pytest.approx(float(g["test_loss"]), abs=2e-6)
    assert te_acc == pytest.approx(float(g["test_acc"]), abs=1e-12)
    X = torch.from_numpy(g["X"]).to(dev)
    assert S.compute_reconstruction_error(model, X, s) == pytest.approx(float(g["rec_error"]), abs=1e-5)
    res = S.compute_alpha_and_norm_ratios(model, X)
    names = ["alpha", "norm_X", "norm_ratio", "rec_scaled", "pearson_mean", "pearson_std", "spearman_mean",
             "spearman_std", "svd_err", "slopes", "correlations", "spearman_scores", "rec_scaled_per_row",
             "alpha_per_row"]
    assert len(res) == 14
    for nm, v in zip(names, res):
        ref = g["m14_" + nm]
        v = np.asarray(v, dtype=np.float64)
        assert v.shape == ref.shape, nm
        scale = max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0)
        np.testing.assert_allclose(v, ref, rtol=0, atol=1e-4 * scale, err_msg=nm)
    gl, ga = S.compute_ground_truth_metrics(test, X, "cuda")
    assert gl == pytest.approx(float(g["gt_loss"]), abs=1e-6)
    assert ga == pytest.approx(float(g["gt_acc"]), abs=1e-12)
    from mfcd import metrics
    rows = metrics.uvt_rows(model.U.data, model.V.data, g["sampled_idx"]).cpu().numpy()
    np.testing.assert_allclose(rows, (U @ V.T)[g["sampled_idx"]], rtol=1e-5, atol=1e-6)


def assert_close_with_rare_outliers(actual, desired, atol, lr, what, frac=2e-4):
    """All elements within `atol`, except that a fraction <= `frac` may differ by up to 5 % of one Adam step (lr):
    where the sparse gradient nearly cancels wd*p, the sign of a ~1e-9 total gradient is rounding noise and Adam's
    m/sqrt(v) turns it into a +-lr-sized move (same sensitivity in the reference itself between CPU builds)."""
    diff = np.abs(np.asarray(actual, np.float64) - np.asarray(desired, np.float64))
    bad = diff > atol
    assert bad.mean() <= frac, f"{what}: {bad.sum()} of {bad.size} elements beyond {atol}"
    assert diff.max() <= 0.05 * lr + atol, f"{what}: max diff {diff.max()}"


# --------------------------------------------------------------------------------------------------
# (b) oracle on seeded inputs, including BASELINE's C2 size, and size-independent properties
# --------------------------------------------------------------------------------------------------
def _synthetic(n, m, d, N, seed, soft=False):
    rng = np.random.default_rng(seed)
    U0 = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    V0 = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    u, i = rng.integers(0, n, N), rng.integers(0, m, N)
    j = (i + 1 + rng.integers(0, max(m - 1, 1), N)) % m
    z = rng.integers(0, 5, N) / 4.0 if soft else rng.integers(0, 2, N).astype(np.float64)
    return U0, V0, u, i, j, z


@pytest.mark.parametrize("n,m,d,N,B,soft", [
    (4096, 4096, 64, 67108, 64, False),   # C2 of BASELINE.json: one full epoch, 1049 steps, last batch 36
    (300, 200, 128, 3000, 64, True),
    (1000, 1000, 2, 5000, 64, False),     # notebook default d=2
    (64, 64, 5, 999, 64, True),           # odd d -> scalar path
    (2, 3, 8, 640, 64, False),            # every batch hits every row many times
    (500, 400, 16, 2000, 200, False),     # B > 64
    (128, 96, 256, 130, 1, False),        # B = 1
    (2048, 1024, 32, 4096, 4096, False),  # one huge batch
    (40, 30, 100, 900, 200, True),        # tiny tables, d > 64 and not a power of two, B > 64
    (100, 60, 4, 4000, 2000, False),      # tiny tables, B > one workgroup's threads
    (24, 16, 100, 900, 64, True),         # local form: 13 column chunks per lane group
    (50, 40, 16, 800, 80, False),         # local form: both hit slots of a lane group on the same table
    (300, 212, 16, 3000, 64, False),      # local form at its largest (8 elements per thread)
])
def test_train_epoch_matches_oracle(dev, orc, path, n, m, d, N, B, soft):
    from mfcd import engine
    from oracle import oracle as O
    if not form_applies(N, B, n, m, d):
        assert path in ("resident", "local"), "the streaming form takes every shape"
        pytest.skip(f"{path} form does not apply to this shape")
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=n + d + N, soft=soft)
    lr, wd = 1e-3, 1e-5
    model, opt = _model_from(U0, V0, dev, lr, wd)
    bind = engine.AdamBinding(model, opt)
    st = _records(u, i, j, z, n, m, dev)
    loss = engine.train_steps(bind, st.dev, B).cpu().numpy()
    ref = O.new_state(U0, V0)
    ref_loss = orc.train_steps(ref, u, i, j, z, B, 0, lr=lr, wd=wd, threads=4)
    np.testing.assert_allclose(loss, ref_loss, rtol=2e-5, atol=2e-6)
    nsteps = len(ref_loss)
    tol = 2e-6 + 2e-8 * nsteps
    assert_close_with_rare_outliers(model.U.data.cpu().numpy(), ref["U"], tol, lr, "U")
    assert_close_with_rare_outliers(model.V.data.cpu().numpy(), ref["V"], tol, lr, "V")
    mU, vV = opt.state[model.U]["exp_avg"].cpu().numpy(), opt.state[model.V]["exp_avg_sq"].cpu().numpy()
    assert (np.abs(mU - ref["mU"]) > 1e-6).mean() <= 2e-4
    assert (np.abs(vV - ref["vV"]) > 2e-3 * np.abs(ref["vV"]) + 1e-12).mean() <= 2e-4
    vl, vc, vp = engine.eval_batches(model.U.data, model.V.data, st.dev, B, want_p=True)
    rl, rc, rp = orc.eval_batches(model.U.data.cpu().numpy(), model.V.data.cpu().numpy(), u, i, j, z, B)
    np.testing.assert_allclose(vp.cpu().numpy(), rp, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(vl.cpu().numpy(), rl, rtol=2e-5, atol=2e-6)
    # hard labels: counts agree except where p sits within rounding of 0.5
    near = np.abs(rp - 0.5) < 1e-6
    assert abs(int(vc.sum()) - int(rc.sum())) <= int(near.sum())


def test_properties_at_c2_size(dev, path):
    if path == "local":
        pytest.skip("C2 does not fit one workgroup")
    _properties_at_c2_size(dev)


def _properties_at_c2_size(dev):
    """Size-independent properties at BASELINE C2: run-to-run bit reproducibility, call-splitting
    invariance (k steps in one call == the same steps over two calls), lr=0 & wd=0 leaves U,V untouched."""
    from mfcd import engine
    n = m = 4096
    d, N, B = 64, 64 * 300 + 17, 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=7)
    st = _records(u, i, j, z, n, m, dev)

    def run(splits):
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        bind = engine.AdamBinding(model, opt)
        losses = [engine.train_steps(bind, st.dev[a:b], B).clone() for a, b in splits]
        return model.U.data.clone(), model.V.data.clone(), torch.cat(losses), opt.state[model.U]["exp_avg_sq"].clone()

    a = run([(0, N)])
    b = run([(0, N)])
    c = run([(0, 64 * 101), (64 * 101, N)])  # odd number of steps in the first call exercises the ping-pong copy
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two identical runs differ"
    for x, y in zip(a, c):
        assert torch.equal(x, y), "splitting the call changed the result"
    model, opt = _model_from(U0, V0, dev, 0.0, 0.0)
    bind = engine.AdamBinding(model, opt)
    engine.train_steps(bind, st.dev[:6400], B)
    assert torch.equal(model.U.data.cpu(), torch.from_numpy(U0)) and torch.equal(model.V.data.cpu(), torch.from_numpy(V0))
    assert bind.step == 100


def test_untouched_rows_move_by_weight_decay_only(dev, orc, path):
    if path == "local":
        pytest.skip("shape does not fit one workgroup")
    """Dense Adam is not optional (SURVEY §7): rows outside the batch still move through wd*p."""
    from mfcd import engine
    n = m = 512
    d = 64
    U0, V0, *_ = _synthetic(n, m, d, 1, seed=3)
    model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
    bind = engine.AdamBinding(model, opt)
    st = _records([5], [7], [9], [1.0], n, m, dev)
    engine.train_steps(bind, st.dev, 64)
    dU = np.abs(model.U.data.cpu().numpy() - U0)
    untouched = np.delete(dU, 5, axis=0)
    assert untouched[np.abs(np.delete(U0, 5, axis=0)) > 0.05].min() > 9e-4  # ~lr on the first step
    assert untouched.max() < 1.1e-3


def test_empty_and_error_paths(dev):
    from mfcd import _lib, engine
    import structure as S
    U0, V0, u, i, j, z = _synthetic(32, 32, 8, 10, seed=1)
    model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
    bind = engine.AdamBinding(model, opt)
    empty = _records([], [], [], [], 32, 32, dev)
    out = engine.train_steps(bind, empty.dev, 64)
    assert out.numel() == 0 and bind.step == 0
    assert torch.equal(model.U.data.cpu(), torch.from_numpy(U0))
    with pytest.raises(IndexError):
        _records([32], [0], [1], [1.0], 32, 32, dev)
    with pytest.raises(RuntimeError):  # no CPU fallback
        S.train_model(model, None, None, opt, "cpu", num_epochs=1)
    cpu_model = S.MatrixFactorization(8, 8, 4)
    cpu_opt = torch.optim.Adam(cpu_model.parameters())
    with pytest.raises(_lib.MfcdError):
        engine.AdamBinding(cpu_model, cpu_opt)
    with pytest.raises(NotImplementedError):
        engine.AdamBinding(model, torch.optim.SGD(model.parameters(), lr=0.1))
    L = _lib.load()
    assert L.mfcd_train_steps(None, None, None, None, None, None, None, 1, 64, 0, 4, 4, 4, 1e-3, .9, .999, 1e-8, 0.,
                              None, None, 0, None) == -1
    assert L.mfcd_error_string(-2).decode().startswith("mfcd: workspace")


_UVT_SHAPES = [(4096, 4096, 64), (1000, 777, 8), (300, 5000, 128), (257, 95, 2), (96, 64, 256),
               (130, 70, 24), (301, 203, 64), (1003, 333, 256), (70, 517, 32), (33, 40, 128)]
# split = 0 (d in {32, 64, 128, 256}): the fp32 MFMA product instead of the default bf16x3 split, the reference's own
# arithmetic (mfcd_set_tuning(MFCD_TUNE_UVT_SPLIT, 0))
_UVT_CASES = [(n, m, d, 1) for n, m, d in _UVT_SHAPES] + \
             [(n, m, d, 0) for n, m, d in _UVT_SHAPES if d in (32, 64, 128, 256)]


@pytest.mark.parametrize("n,m,d,split", _UVT_CASES,
                         ids=[f"{n}-{m}-{d}" + ("" if split else "-fp32") for n, m, d, split in _UVT_CASES])
def test_uvt_stats_match_oracle(dev, orc, n, m, d, split):
    from mfcd import engine, metrics
    rng = np.random.default_rng(n + m + d)
    U = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    V = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    A = rng.standard_normal((n, d)).astype(np.float32)
    Bm = rng.standard_normal((m, d)).astype(np.float32)
    X = (A @ Bm.T / np.sqrt(d) * 0.5 + 0.1).astype(np.float32)
    s = 1.7
    try:
        engine.set_tuning(uvt_split=split)
        rs, scal = metrics.uvt_stats(torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(X).to(dev), s)
        rs, scal = rs.cpu().numpy(), scal.cpu().numpy()
    finally:
        engine.set_tuning(uvt_split=1)
    if n * m <= 1 << 21:
        ref_rs, err2, ref2 = orc.uvt_stats(U, V, X, s)
    else:  # f64 numpy statement of the same sums for the large case
        G = U.astype(np.float64) @ V.astype(np.float64).T
        Xd = X.astype(np.float64)
        a = G - G.mean(1, keepdims=True)
        c = Xd - Xd.mean(1, keepdims=True)
        ref_rs = np.stack([(a * c).sum(1), (a * a).sum(1), (c * c).sum(1)], 1)
        err2 = float((((G - G.mean(0, keepdims=True)) - s * Xd) ** 2).sum())
        ref2 = float(((s * Xd) ** 2).sum())
    for col in range(3):
        scale = np.abs(ref_rs[:, col]).max()
        np.testing.assert_allclose(rs[:, col], ref_rs[:, col], rtol=0, atol=2e-5 * scale)
    assert scal[0] == pytest.approx(err2, rel=2e-5)
    assert scal[1] == pytest.approx(ref2, rel=2e-5)


def test_forms_agree_and_resident_rejects_unsupported_shapes(dev):
    from mfcd import _lib, engine
    n, m, d, N, B = 128, 96, 32, 64 * 40 + 5, 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=11, soft=True)
    st = _records(u, i, j, z, n, m, dev)
    outs = {}
    try:
        for mode in ("streaming", "resident", "local"):
            engine.set_train_path(mode)
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B)
            engine.check_status()
            outs[mode] = (model.U.data.cpu().numpy(), model.V.data.cpu().numpy(), loss.cpu().numpy())
        for other in ("resident", "local"):
            for a, b in zip(outs["streaming"], outs[other]):
                np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)
        engine.set_train_path("resident")
        U0, V0, u, i, j, z = _synthetic(40, 40, 5, 64, seed=2)
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        with pytest.raises(_lib.MfcdError):
            engine.train_steps(engine.AdamBinding(model, opt), _records(u, i, j, z, 40, 40, dev).dev, 64)
    finally:
        engine.set_train_path("auto")


@pytest.mark.parametrize("mode", ["allgather", "allreduce"])
def test_data_parallel_hip_backend_single_rank(dev, mode):
    """mfcd.dist with the product backend (HipCompute) on a one-rank RCCL group: both exchange forms must
    reproduce the fused step (the multi-rank logic itself is covered on CPU/gloo in test_dist_cpu.py)."""
    import os
    import torch.distributed as dist
    from mfcd import dist as mdist, engine
    n, m, d, N, B = 700, 500, 64, 64 * 30 + 21, 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=21)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).cpu().numpy()
        ref_U, ref_V = model.U.data.cpu().numpy(), model.V.data.cpu().numpy()
    finally:
        engine.set_train_path("auto")
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        bind = engine.AdamBinding(model, opt)
        losses = mdist.train_steps_dp(mdist.HipCompute(bind), st.dev, B, mode=mode).cpu().numpy()
    finally:
        if created:
            dist.destroy_process_group()
    assert bind.step == len(ref_loss) == 31
    np.testing.assert_allclose(losses, ref_loss, rtol=2e-5, atol=2e-6)
    # both split forms equal the fused step bit for bit (tests/test_step_parts.py: identities 3 and 4), step after step
    assert np.array_equal(model.U.data.cpu().numpy(), ref_U)
    assert np.array_equal(model.V.data.cpu().numpy(), ref_V)


@pytest.mark.parametrize("world,N,shape", [(1, 64 * 9 + 5, None), (2, 64 * 2 * 7 + 70, None), (3, 64 * 3 * 5 + 130, None),
                                           (8, 64 * 8 * 3 + 1, None), (8, 64 * 8 * 4 + 77, (65536, 65536, 64))])
def test_native_dp_loop_single_process_rehearsal(dev, world, N, shape):
    """mfcd_dp_train_steps without a communicator computes every rank's shard in this process (replicas are
    identical, so that IS the gathered buffer): shard bounds, padding of short / empty shards and the global divisor
    must make the run bit-identical to the fused streaming step with batch_size = 64 * world.  Last case: world 8 at
    BASELINE configs[3] (C4) table shape, the configuration the data-parallel form is named for."""
    from mfcd import dist as mdist, engine
    (n, m, d), B = shape or (300, 260, 32), 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=100 + world)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B * world).cpu().numpy()
        ref_U, ref_V = model.U.data.cpu().numpy(), model.V.data.cpu().numpy()
    finally:
        engine.set_train_path("auto")
    model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
    bind = engine.AdamBinding(model, opt)
    losses = mdist.NativeDP(bind, simulate_world=world).train_steps(st.dev, B).cpu().numpy()
    assert bind.step == len(ref_loss) == (N + B * world - 1) // (B * world)
    np.testing.assert_allclose(losses, ref_loss, rtol=1e-6, atol=1e-7)      # same terms, different summation tree
    np.testing.assert_array_equal(model.U.data.cpu().numpy(), ref_U)
    np.testing.assert_array_equal(model.V.data.cpu().numpy(), ref_V)


@pytest.mark.parametrize("world,n,m,d,N", [(1, 300, 260, 32, 64 * 9 + 5), (3, 300, 260, 32, 64 * 3 * 5 + 130),
                                           (8, 16384, 16384, 128, 64 * 8 * 3 + 1)])
def test_native_dp_loop_with_bf16_factor_tables(dev, world, n, m, d, N):
    """VERDICT r2 missing item 5: mfcd_dp_train_steps_bf16 — the data-parallel loop over bf16 factor tables (BASELINE
    configs[2]'s storage; last case its table shape at world 8) — is bit-identical to mfcd_train_steps_bf16's streaming
    form with batch_size = 64 * world (tables and both moments), whose rounding points the oracle's bf16 mode defines."""
    import structure as S
    from mfcd import dist as mdist, engine
    B = 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=200 + world)
    st = _records(u, i, j, z, n, m, dev)

    def fresh():
        model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16)
        with torch.no_grad():
            model.U.copy_(torch.from_numpy(U0))
            model.V.copy_(torch.from_numpy(V0))
        model = model.to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
        return model, opt
    engine.set_train_path("streaming")
    try:
        model, opt = fresh()
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B * world).cpu().numpy()
    finally:
        engine.set_train_path("auto")
    m2, o2 = fresh()
    bind = engine.AdamBinding(m2, o2)
    losses = mdist.NativeDP(bind, simulate_world=world).train_steps(st.dev, B).cpu().numpy()
    assert m2.U.dtype == torch.bfloat16 and bind.step == len(ref_loss)
    np.testing.assert_allclose(losses, ref_loss, rtol=1e-6, atol=1e-7)
    assert torch.equal(m2.U.data, model.U.data) and torch.equal(m2.V.data, model.V.data)
    for prm, prm2 in ((model.U, m2.U), (model.V, m2.V)):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[prm][key], o2.state[prm2][key]), key


def test_native_dp_loop_over_rccl_single_rank(dev):
    """The native loop with a real RCCL communicator (created inside libmfcd_hip.so from an ncclUniqueId carried over
    torch.distributed) on a one-rank group reproduces the fused streaming step bit for bit."""
    import os
    import torch.distributed as dist
    from mfcd import dist as mdist, engine
    n, m, d, N, B = 700, 500, 64, 64 * 30 + 21, 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=21)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).cpu().numpy()
        ref_U, ref_V = model.U.data.cpu().numpy(), model.V.data.cpu().numpy()
    finally:
        engine.set_train_path("auto")
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        created = True
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        bind = engine.AdamBinding(model, opt)
        ndp = mdist.NativeDP(bind)
        assert ndp.comm is not None and ndp.world == 1
        losses = ndp.train_steps(st.dev, B).cpu().numpy()
        ndp.close()
    finally:
        if created:
            dist.destroy_process_group()
    np.testing.assert_allclose(losses, ref_loss, rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(model.U.data.cpu().numpy(), ref_U)
    np.testing.assert_array_equal(model.V.data.cpu().numpy(), ref_V)


def _describe(o):
    if isinstance(o, dict):
        return {"type": "dict", "items": {k: _describe(v) for k, v in o.items()}}
    if isinstance(o, (list, tuple)):
        d = {"type": type(o).__name__, "len": len(o)}
        if len(o):
            d["elem0"] = _describe(o[0])
        return d
    if isinstance(o, np.ndarray):
        return {"type": "ndarray", "dtype": str(o.dtype), "shape": list(o.shape)}
    mod = type(o).__module__
    return {"type": type(o).__name__ if mod == "builtins" else mod + "." + type(o).__name__}


def test_run_experiment_and_parameter_scan_keep_the_pkl_layout(dev, tmp_path):
    """The 23-key result dict (structure.py:420-444) and the pickled list of {'params','results'} (172-200) have the
    same keys, nesting, lengths and leaf types as the reference produced (tests/golden/result_schema.json)."""
    import json
    import os
    import pickle
    import structure as S
    from conftest import GOLDEN
    schema = json.load(open(os.path.join(GOLDEN, "result_schema.json")))
    torch.manual_seed(3)
    np.random.seed(3)
    res = S.run_experiment(40, 30, 4, 0.5, 1.0, "cuda", 1e-3, 1e-5, reps=2, num_epochs=2)
    assert _describe(res) == schema["run_experiment"]
    assert 0.0 <= res["accuracy"][0] <= 1.0 and 0.3 < res["train_losses"][0][0] < 1.5
    path = str(tmp_path / "sub" / "scan.pkl")
    ret = S.parameter_scan(n=40, m=30, d=[2, 4], p=0.5, device="cuda", num_epochs=1, reps=1, save_path=path, save_every=1)
    assert ret == []                                   # the reference returns [] once it has saved (structure.py:200-202)
    with open(path, "rb") as f:
        saved = pickle.load(f)
    assert _describe(saved) == schema["parameter_scan_saved"]
    assert saved[0]["params"] == schema["parameter_scan_saved_params0"]
    ret2 = S.parameter_scan(n=40, m=30, d=2, p=0.5, device="cuda", num_epochs=1, reps=1)
    assert len(ret2) == 1 and set(ret2[0]) == {"params", "results"}
    losses, accs = S.evaluate_ground_truth(40, 30, 0.5, 4, 1.0, "cuda", K=1, reps=2)
    assert len(losses) == len(accs) == 2 and all(0.5 < a <= 1.0 for a in accs)
    scan = S.parameter_scan_ground_truth(40, 30, 0.5, [2, 4], 1.0, "cuda", 1)
    assert len(scan) == 2 and set(scan[0]["results"]) == {"gt_loss", "gt_accuracy"}


def test_full_pipeline_reproduces_reference_run_from_seeds(dev):
    """generate_X -> split -> model -> train_model -> metrics, from the same seeds the reference used for fixture
    e2e_c1 (C1 of BASELINE.json): everything host-side is RNG-identical, so the trained factors must match too."""
    import structure as S
    g = load_golden("e2e_c1.npz")
    torch.manual_seed(0)
    np.random.seed(0)
    X = S.generate_X(256, 256, 8, "cuda")
    train, val, test = S.split_dataset_from_triplets(X, int(256 * 256 * 0.05 / 2), scale=1.0, K=1)
    model = S.MatrixFactorization(256, 256, 8).to("cuda")
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    tl, vl = S.train_model(model, train, val, opt, "cuda", num_epochs=5)
    np.testing.assert_allclose(tl, g["train_losses"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(vl, g["val_losses"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(model.U.data.cpu().numpy(), g["U_final"], rtol=0, atol=2e-6)
    te_loss, te_acc = S.evaluate_model(model, test, "cuda")
    assert te_loss == pytest.approx(float(g["test_loss"]), abs=2e-6) and te_acc == pytest.approx(float(g["test_acc"]), abs=1e-12)
    assert S.compute_reconstruction_error(model, X, 1.0) == pytest.approx(float(g["rec_error"]), abs=1e-5)


@pytest.mark.parametrize("n,m,d,N", [(4096, 4096, 64, 64 * 200 + 9), (300, 200, 128, 64 * 50), (64, 48, 8, 64 * 60 + 1),
                                      (1000, 1000, 2, 64 * 40), (6, 5, 16, 64 * 30),
                                      (16384, 16384, 128, 64 * 60 + 3),      # C3: 32 registers per array, LDS accumulators
                                      (8192, 8192, 64, 64 * 50)])            # 16 registers per array
def test_lookahead_publishing_is_bit_identical(dev, n, m, d, N):
    """Look-ahead publishing only changes WHEN a row is handed over, never its value: the resident kernel with and
    without it must agree bit for bit (small tables make rows recur inside the window, the deferred-publish case)."""
    from mfcd import engine
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=n + d)
    st = _records(u, i, j, z, n, m, dev)
    outs = []
    engine.set_train_path("resident")
    try:
        for look in (0, 4):
            engine.set_tuning(resident_lookahead=look)
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, 64)
            engine.check_status()
            outs.append((model.U.data.clone(), model.V.data.clone(), loss.clone(),
                         opt.state[model.V]["exp_avg_sq"].clone()))
    finally:
        engine.set_tuning(resident_lookahead=-1)
        engine.set_train_path("auto")
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_planned_workspace_is_reused_without_reinitialisation(dev):
    """A workspace planned for an epoch serves calls of every length that fits it with no per-call re-initialisation:
    short and long resident calls interleaved (different touch-string strides, mailbox slots reused under new launch
    ids) must give exactly what the same steps give in one call, and the buffer must not be re-planned."""
    from mfcd import engine
    n = m = 1024
    d, B = 64, 64
    N = B * 400 + 11
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=5)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("resident")
    try:
        def run(cuts):
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            bind = engine.AdamBinding(model, opt)
            engine.reserve_workspace(N, B, n, m, d, dev)
            buf = engine.workspace_for(dev).buf
            out = [engine.train_steps(bind, st.dev[a:b], B).clone() for a, b in zip(cuts[:-1], cuts[1:])]
            assert engine.workspace_for(dev).buf is buf, "the planned workspace was replaced"
            engine.check_status()
            return model.U.data.clone(), model.V.data.clone(), torch.cat(out), opt.state[model.U]["exp_avg"].clone()
        whole = run([0, N])
        pieces = run([0, B * 5, B * 25, B * 26, B * 300, B * 303, N])
        for a, b in zip(whole, pieces):
            assert torch.equal(a, b)
    finally:
        engine.set_train_path("auto")


def test_resident_abort_is_sticky_and_reported(dev):
    """an abort in a NON-final call must not be masked by later calls.  A spin limit of one poll round makes
    the first wave that has to wait give up; two more calls follow on the same workspace; check_status must still
    raise, and the next call after that must run on a fresh workspace."""
    from mfcd import _lib, engine
    n = m = 4096
    d, B = 64, 64
    N = B * 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=9)
    st = _records(u, i, j, z, n, m, dev)
    model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
    bind = engine.AdamBinding(model, opt)
    engine.set_train_path("resident")
    try:
        engine.check_status()
        engine.set_tuning(resident_spin_limit=1, resident_lookahead=0)   # publish right before use: waits are certain
        engine.train_steps(bind, st.dev, B)
        engine.set_tuning(resident_spin_limit=0, resident_lookahead=-1)
        engine.train_steps(bind, st.dev, B)
        engine.train_steps(bind, st.dev[: B * 3], B)
        with pytest.raises(_lib.MfcdError, match="aborted"):
            engine.check_status()
        engine.check_status()                                  # reported once; the workspace was dropped
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        engine.train_steps(engine.AdamBinding(model, opt), st.dev, B)
        engine.check_status()
        assert torch.isfinite(model.U.data).all()
    finally:
        engine.set_tuning(resident_spin_limit=0, resident_lookahead=-1)
        engine.set_train_path("auto")


def test_auto_takes_the_streaming_form_for_very_short_calls(dev):
    from mfcd import engine
    assert engine.train_plan(64 * 2, 64, 4096, 4096, 64)["form_name"] == "streaming"
    plan = engine.train_plan(64 * 1049, 64, 4096, 4096, 64)
    assert plan["form_name"] == "resident" and plan["resident_q"] == 2 and plan["resident_waves"] == 4096
    assert engine.train_plan(1310, 64, 256, 256, 8)["form_name"] == "local"
    assert engine.train_plan(64 * 1049, 64, 4096, 4096, 64, bf16=True)["form_name"] == "resident"   # bf16 tables too
    c3 = engine.train_plan(107373, 64, 16384, 16384, 128, bf16=True)                # BASELINE configs[2]
    assert (c3["form_name"], c3["resident_q"], c3["resident_waves"]) == ("resident", 32, 2048)
    assert engine.train_plan(107373, 64, 65536, 65536, 64)["form_name"] == "streaming"             # C4: HBM-bound


@pytest.mark.parametrize("name,n,m,d,steps", [
    ("C3-shape", 16384, 16384, 128, 24),      # BASELINE configs[2] shape (fp32 factors here)
    ("C4-shape", 65536, 65536, 64, 16),       # BASELINE configs[3] shape
    ("C5-shape", 100000, 20000, 256, 8),      # BASELINE configs[4] shape
])
def test_streaming_step_at_baseline_full_sizes(dev, orc, name, n, m, d, steps):
    """BASELINE.json's larger shapes (fp32): a few optimiser steps of the streaming form against the oracle, plus
    run-to-run bit reproducibility.  (bf16 factors of configs[2] are a later row)"""
    from mfcd import engine
    from oracle import oracle as O
    B = 64
    N = B * steps - 7
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=d + steps)
    u[:40] = u[0]            # force duplicate users / items inside the first batch
    i[:20] = i[0]
    j[:20] = (i[0] + 1) % m
    st = _records(u, i, j, z, n, m, dev)
    outs = []
    for _ in range(2):
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B)
        outs.append((model.U.data.clone(), model.V.data.clone(), loss.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    ref = O.new_state(U0, V0)
    ref_loss = orc.train_steps(ref, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=8)
    np.testing.assert_allclose(outs[0][2].cpu().numpy(), ref_loss, rtol=2e-5, atol=2e-6)
    assert_close_with_rare_outliers(outs[0][0].cpu().numpy(), ref["U"], 2e-6, 1e-3, name + " U")
    assert_close_with_rare_outliers(outs[0][1].cpu().numpy(), ref["V"], 2e-6, 1e-3, name + " V")


@pytest.mark.parametrize("n,m,d,steps", [(16384, 16384, 128, 24), (300, 200, 64, 60), (50, 40, 8, 40)])
def test_bf16_factor_storage_matches_oracle_rounding_points(dev, orc, n, m, d, steps):
    """BASELINE configs[2] ("bf16 factors"; first case = its shape): U, V stored as bf16, fp32 moments and arithmetic,
    one round-to-nearest-even per step.  The reference has no such mode, so the ORACLE defines the rounding points
    (parity unpinned by the reference).  A last-bit fp32 difference can flip a bf16 rounding, so the check is:
    almost every element bit-equal, the rest within ONE bf16 ulp; losses within 1e-4 of the oracle and within 2e-2
    of the fp32 run."""
    from mfcd import engine
    from oracle import oracle as O
    import structure as S
    B = 64
    N = B * steps - 5
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=9 + d)
    U0, V0 = orc.round_bf16(U0.copy()), orc.round_bf16(V0.copy())
    st = _records(u, i, j, z, n, m, dev)
    model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16)
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(U0))
        model.V.copy_(torch.from_numpy(V0))
    model = model.to(dev)
    assert model.U.dtype == torch.bfloat16 and torch.equal(model.U.data.float().cpu(), torch.from_numpy(U0))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    bind = engine.AdamBinding(model, opt)
    assert opt.state[model.U]["exp_avg"].dtype == torch.float32
    loss = engine.train_steps(bind, st.dev, B).cpu().numpy()
    ref = O.new_state(U0, V0)
    ref_loss = orc.train_steps(ref, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=8, bf16_factors=True)
    np.testing.assert_allclose(loss, ref_loss, rtol=0, atol=1e-4)
    for nm, got in (("U", model.U.data.float().cpu().numpy()), ("V", model.V.data.float().cpu().numpy())):
        want = ref[nm]
        diff = np.abs(got - want)
        ulp = np.maximum(np.abs(want), 1e-30) * 2.0 ** -7          # >= one bf16 ulp of the value
        assert (diff > 0).mean() < 2e-3, f"{nm}: {(diff > 0).mean():.2e} of the elements differ"
        assert np.all(diff <= ulp), f"{nm}: an element differs by more than one bf16 ulp"
    # eval pass on bf16 tables
    vl, _, vp = engine.eval_batches(model.U.data, model.V.data, st.dev, B, want_p=True)
    _, _, rp = orc.eval_batches(model.U.data.float().cpu().numpy(), model.V.data.float().cpu().numpy(), u, i, j, z, B)
    np.testing.assert_allclose(vp.cpu().numpy(), rp, rtol=RTOL, atol=ATOL)
    # against the fp32 run from the same (bf16-representable) start
    f32 = O.new_state(U0, V0)
    f32_loss = orc.train_steps(f32, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=8)
    np.testing.assert_allclose(loss, f32_loss, rtol=0, atol=2e-2)


# --------------------------------------------------------------------------------------------------
# (e) VERDICT r1 item 1: the configurations no -m gpu test had reached
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,m,d", [("C3", 16384, 16384, 128), ("C5", 100000, 20000, 256)])
def test_uvt_stats_at_baseline_full_sizes(dev, orc, name, n, m, d):
    """mfcd_uvt_stats at BASELINE C3 / C5 size (structure.py:925-955, 982-996).  The oracle cannot sweep 2e9 entries
    in seconds, so: (1) the per-row sums of 256 random rows against the oracle ON those rows (they depend only on
    U[r], V and X[r]); (2) the two global sums against an independent blocked float64 evaluation (torch.matmul in f64,
    row blocks, nothing shared with the kernel); (3) two runs bit-equal."""
    from mfcd import metrics
    g = torch.Generator(device=dev).manual_seed(1000 + d)
    U = torch.randn(n, d, device=dev, generator=g) / d ** 0.5
    V = torch.randn(m, d, device=dev, generator=g) / d ** 0.5
    X = torch.empty(n, m, device=dev)
    for r0 in range(0, n, 8192):
        X[r0:r0 + 8192].normal_(0.0, 0.5, generator=g)
    X += 0.25 * (U @ V.t()) if n * m <= (1 << 28) else 0.0      # some correlation where the temporary is affordable
    s = 0.7
    rs, sc = metrics.uvt_stats(U, V, X, s)
    rs2, sc2 = metrics.uvt_stats(U, V, X, s)
    assert torch.equal(rs, rs2) and torch.equal(sc, sc2), "the pass is not run-to-run deterministic"
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(d))[:256].sort().values
    ref_rows, _, _ = orc.uvt_stats(U[rows.to(dev)].cpu().numpy(), V.cpu().numpy(), X[rows.to(dev)].cpu().numpy(), s)
    got = rs[rows.to(dev)].cpu().numpy()
    np.testing.assert_allclose(got[:, 0], ref_rows[:, 0], rtol=2e-5, atol=2e-5 * np.abs(ref_rows[:, 0]).max())
    np.testing.assert_allclose(got[:, 1], ref_rows[:, 1], rtol=2e-5)
    np.testing.assert_allclose(got[:, 2], ref_rows[:, 2], rtol=2e-5)
    # global sums, independent f64 evaluation in row blocks (structure.py:940-952)
    Vd = V.double()
    cm = (U.double().mean(dim=0, keepdim=True) @ Vd.t())        # column mean of U V^T = mean_r(U) V^T
    err2 = torch.zeros((), dtype=torch.float64, device=dev)
    ref2 = torch.zeros((), dtype=torch.float64, device=dev)
    blk = 2048
    for r0 in range(0, n, blk):
        Xb = X[r0:r0 + blk].double()
        G = U[r0:r0 + blk].double() @ Vd.t()
        err2 += ((G - cm) - s * Xb).pow(2).sum()
        ref2 += (s * Xb).pow(2).sum()
        del G, Xb
    assert float(sc[0]) == pytest.approx(float(err2), rel=2e-5)
    assert float(sc[1]) == pytest.approx(float(ref2), rel=2e-5)
    # the rows-only and error-only passes at these sizes finish in the separate final kernels (no fold into the tail)
    rs1, _ = metrics.uvt_stats(U, V, X, s, what=1)
    _, sc2 = metrics.uvt_stats(U, V, X, s, what=2)
    assert torch.equal(rs1, rs)
    assert float(sc2[0]) == pytest.approx(float(sc[0]), rel=1e-12)
    assert float(sc2[1]) == pytest.approx(float(sc[1]), rel=1e-6)


def _sampled_stream(strategy, n, m, d, want, seed, steps, B=64):
    """`steps` batches of a training stream drawn the way the pipeline draws it at BASELINE C3 / C5: factored "base"
    X (generation_data.generate_embedding_factors), the build's own sampler for the strategy, BTL labels, a seeded
    permutation as the epoch order.  Returns (u, i, j, z) numpy arrays of steps*B - 5 samples."""
    import generation_data as gd
    import structure as S
    torch.manual_seed(seed)
    np.random.seed(seed)
    A, Bf = gd.generate_embedding_factors(n, m, d, "cpu", generator=torch.Generator().manual_seed(seed))
    FX = gd.FactoredMatrix(A, Bf)
    if strategy == "margin":
        trip = gd.choose_items_by_margin(FX, want, set())
    else:
        trip = gd.choose_items_by_popularity(FX, want, set(), method="zipf", alpha=1.5)
    ds = S.BTLPreferenceDataset(trip, FX, scale=1.0, K=1, soft_label=False, train=True)
    rows = ds._mfcd_records()
    order = torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(seed + 1)).numpy()
    rows = rows[order[: steps * B - 5]]
    return rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64), rows[:, 3].copy()


@pytest.mark.parametrize("name,strategy,n,m,d,want,steps,bf16", [
    ("C3 margin fp32", "margin", 16384, 16384, 128, 134217, 24, False),
    ("C3 margin bf16 factors", "margin", 16384, 16384, 128, 134217, 24, True),
    ("C5 popularity", "popularity", 100000, 20000, 256, 60000, 8, False),
])
def test_sampler_streams_at_baseline_full_sizes(dev, orc, name, strategy, n, m, d, want, steps, bf16, capsys):
    """BASELINE configs[2] (margin-sampled, bf16 factors) and configs[4] (Zipf popularity: item 0 sits in ~40 % of the
    samples of EVERY batch, so one row takes dozens of serial accumulations per step) through the fused step, against
    the oracle on the same stream.  Triplet count reduced as VERDICT r1 allows (margin: the reference's own 5 M attempt
    cap yields ~11 k at this density; popularity: 60 k of the 500 k)."""
    from mfcd import engine
    from oracle import oracle as O
    import structure as S
    B = 64
    u, i, j, z = _sampled_stream(strategy, n, m, d, want, seed=17, steps=steps, B=B)
    if strategy == "popularity":
        assert np.mean((i == 0) | (j == 0)) > 0.3, "the Zipf head is missing from the stream"
    assert len(u) >= (steps - 1) * B
    rng = np.random.default_rng(3)
    U0 = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    V0 = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    st = _records(u, i, j, z, n, m, dev)
    if bf16:
        U0, V0 = orc.round_bf16(U0.copy()), orc.round_bf16(V0.copy())
        model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16)
        with torch.no_grad():
            model.U.copy_(torch.from_numpy(U0))
            model.V.copy_(torch.from_numpy(V0))
        model = model.to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    else:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
    # bf16 tables take the resident form at C3 size; its IEEE flavour is the one that must match the oracle to the
    # bf16 ulp (the fast flavour's allowance: test_resident_form_with_bf16_factor_tables)
    engine.set_resident_math("ieee" if bf16 else "fast")
    try:
        loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).cpu().numpy()
        engine.check_status()
    finally:
        engine.set_resident_math("fast")
    ref = O.new_state(U0, V0)
    ref_loss = orc.train_steps(ref, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=8, bf16_factors=bf16)
    if bf16:
        np.testing.assert_allclose(loss, ref_loss, rtol=0, atol=1e-4)
        for nm, got in (("U", model.U.data.float().cpu().numpy()), ("V", model.V.data.float().cpu().numpy())):
            diff = np.abs(got - ref[nm])
            assert (diff > 0).mean() < 2e-3 and np.all(diff <= np.maximum(np.abs(ref[nm]), 1e-30) * 2.0 ** -7), nm
    else:
        np.testing.assert_allclose(loss, ref_loss, rtol=2e-5, atol=2e-6)
        assert_close_with_rare_outliers(model.U.data.cpu().numpy(), ref["U"], 2e-6, 1e-3, name + " U")
        assert_close_with_rare_outliers(model.V.data.cpu().numpy(), ref["V"], 2e-6, 1e-3, name + " V")


@pytest.mark.parametrize("form", ["streaming", "resident", "resident-ieee", "local"])
def test_zipf_head_stream_through_every_form(dev, orc, form):
    """The duplicate-row stress of a popularity stream (one item row hit by ~25 of the 64 samples of every batch) on
    the forms a uniform stream never stresses that way: the resident form's owner wave of that row hits and publishes
    on EVERY step; the local form's claim rounds run ~25 deep."""
    from mfcd import engine
    from oracle import oracle as O
    n, m, d = (4096, 4096, 64) if form != "local" else (300, 212, 16)
    steps, B = (300, 64) if form != "local" else (120, 64)
    u, i, j, z = _sampled_stream("popularity", n, m, d, 40000 if form != "local" else 9000, seed=23, steps=steps, B=B)
    assert np.mean((i == 0) | (j == 0)) > 0.3
    rng = np.random.default_rng(4)
    U0 = (rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)
    V0 = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path(form.split("-")[0])
    engine.set_resident_math("ieee" if form.endswith("ieee") else "fast")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).cpu().numpy()
        engine.check_status()
    finally:
        engine.set_train_path("auto")
        engine.set_resident_math("fast")
    ref = O.new_state(U0, V0)
    ref_loss = orc.train_steps(ref, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=4)
    np.testing.assert_allclose(loss, ref_loss, rtol=2e-5, atol=2e-6)
    tol = 2e-6 + 2e-8 * len(ref_loss)
    assert_close_with_rare_outliers(model.U.data.cpu().numpy(), ref["U"], tol, 1e-3, form + " U")
    assert_close_with_rare_outliers(model.V.data.cpu().numpy(), ref["V"], tol, 1e-3, form + " V")


# --------------------------------------------------------------------------------------------------
# (f) SURVEY 8f N4: Spearman rank kernel
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,m", [(64, 5), (33, 100), (64, 1000), (48, 3001), (256, 4096), (24, 16384), (3, 2), (12, 16385),
                                    (16, 20000), (8, 20448)])   # 20000 = BASELINE configs[4]; 20448 = the kernel's limit
def test_spearman_rows_match_scipy(dev, rows, m):
    """mfcd_spearman_rows against scipy's own spearmanr, row by row (the reference's call, structure.py:1028), and the
    oracle's vectorised restatement: continuous rows, heavily tied rows (five distinct values, as ratings), rows with
    -0.0 / +0.0, a constant row (NaN in both), strided inputs; bit-reproducible."""
    from scipy.stats import spearmanr
    from mfcd import metrics
    from oracle import oracle as O
    rng = np.random.default_rng(rows * 100003 + m)
    A = rng.standard_normal((rows, m)).astype(np.float32)
    X = (0.6 * A + rng.standard_normal((rows, m))).astype(np.float32)
    X[1] = np.round(X[1] * 2.0) / 2.0                     # ties in one operand
    A[2], X[2] = rng.integers(0, 5, m).astype(np.float32), rng.integers(0, 5, m).astype(np.float32)   # ties in both
    A[0, : m // 2] = 0.0
    A[0, 0] = -0.0                                        # -0.0 must tie with +0.0
    if rows > 3:
        X[3] = 1.25                                       # constant row -> NaN
    pad = np.full((rows, m + 7), 99.0, dtype=np.float32)  # strided: rows of a wider matrix
    pad[:, :m] = A
    Ad, Xd = torch.from_numpy(pad).to(dev)[:, :m], torch.from_numpy(X).to(dev)
    rho = metrics.spearman_rows(Ad, Xd)
    rho2 = metrics.spearman_rows(Ad, Xd)
    got = rho.cpu().numpy()
    assert np.array_equal(got, rho2.cpu().numpy(), equal_nan=True)
    want = O.spearman_rows(A, X)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        direct = np.array([spearmanr(A[r], X[r]).correlation for r in range(min(rows, 8))])
    np.testing.assert_allclose(got[: len(direct)], direct, rtol=0, atol=1e-12, equal_nan=True)
    if rows > 3:
        assert np.isnan(got[3])


# --------------------------------------------------------------------------------------------------
# (g) SURVEY 8f N1: label generation on the device
# --------------------------------------------------------------------------------------------------
def test_device_label_generation_follows_the_btl_law(dev):
    """mfcd_generate_labels (structure.py:493-519 on the device).  The stream is Philox, not the reference's CPU
    generator, so parity is DISTRIBUTIONAL: every label is Bernoulli(sigmoid(s (X[u,i] - X[u,j]))).  Checked: record
    layout (K consecutive rows per triplet / one soft row), empirical frequencies per probability bucket within
    4.5 sigma, soft labels on the K-grid with the right mean, reproducibility per seed, dense X == factored X."""
    import generation_data as gd
    import structure as S
    from mfcd import engine
    n, m, d, T, K, s = 300, 200, 8, 60000, 4, 1.7
    A, Bf = gd.generate_embedding_factors(n, m, d, "cpu", generator=torch.Generator().manual_seed(5))
    FX = gd.FactoredMatrix(A, Bf)
    X = FX.dense()
    rng = np.random.default_rng(11)
    trip = np.stack([rng.integers(0, n, T), rng.integers(0, m, T), rng.integers(0, m, T)], 1)
    rec = engine.generate_labels(trip, X.to(dev), scale=s, K=K, soft=False, seed=123, device=dev).cpu().numpy()
    assert rec.shape == (T * K, 4)
    assert np.array_equal(rec[:, :3], np.repeat(trip, K, axis=0))
    z = rec[:, 3].copy().view(np.float32)
    assert set(np.unique(z)) <= {0.0, 1.0}
    p = 1.0 / (1.0 + np.exp(-s * (X.numpy()[trip[:, 0], trip[:, 1]] - X.numpy()[trip[:, 0], trip[:, 2]]).astype(np.float64)))
    pk = np.repeat(p, K)
    for lo in np.arange(0.0, 1.0, 0.1):
        sel = (pk >= lo) & (pk < lo + 0.1)
        if sel.sum() < 200:
            continue
        want, sd = pk[sel].mean(), np.sqrt((pk[sel] * (1 - pk[sel])).sum()) / sel.sum()
        assert abs(z[sel].mean() - want) < 4.5 * sd, (lo, z[sel].mean(), want, sd)
    # the K draws of one triplet are independent: their agreement rate matches p^2 + (1-p)^2
    zz = z.reshape(T, K)
    agree = (zz[:, 0] == zz[:, 1]).mean()
    assert abs(agree - np.mean(p * p + (1 - p) * (1 - p))) < 0.01
    again = engine.generate_labels(trip, X.to(dev), scale=s, K=K, soft=False, seed=123, device=dev).cpu().numpy()
    other = engine.generate_labels(trip, X.to(dev), scale=s, K=K, soft=False, seed=124, device=dev).cpu().numpy()
    assert np.array_equal(rec, again) and not np.array_equal(rec, other)
    fact = engine.generate_labels(trip, FX, scale=s, K=K, soft=False, seed=123, device=dev).cpu().numpy()
    assert (fact[:, 3] != rec[:, 3]).mean() < 1e-3          # same uniforms, scores equal up to fp32 rounding
    soft = engine.generate_labels(trip, X.to(dev), scale=s, K=K, soft=True, seed=123, device=dev).cpu().numpy()
    zs = soft[:, 3].copy().view(np.float32)
    assert soft.shape == (T, 4) and set(np.unique(zs)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    np.testing.assert_allclose(zs, zz.mean(axis=1), rtol=0, atol=0)      # same draws, averaged
    # through the dataset / loader classes into a training call
    S.set_label_device(dev)
    try:
        torch.manual_seed(9)
        ds = S.BTLPreferenceDataset(trip[:5000], X.to(dev), scale=s, K=2, soft_label=False, train=True)
        assert len(ds) == 10000 and isinstance(ds[3], tuple) and len(ds[3]) == 4
        torch.manual_seed(9)
        ds2 = S.BTLPreferenceDataset(trip[:5000], X.to(dev), scale=s, K=2)
        assert ds.data == ds2.data                                       # same global seed -> same labels
        loader = torch.utils.data.DataLoader(S.BTLPreferenceDataset(trip[:5000], X.to(dev), K=2), batch_size=64,
                                             shuffle=True)
    finally:
        S.set_label_device(None)
    store = engine.SampleStore.from_loader(loader, n, m, dev)
    assert store.host is None and store.N == 10000
    model = S.MatrixFactorization(n, m, d).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    tl, vl = S.train_model(model, loader, loader, opt, dev, num_epochs=2)
    assert len(tl) == 2 and np.isfinite(tl).all() and tl[1] < tl[0]
    with pytest.raises(IndexError):
        engine.generate_labels(np.array([[n, 0, 1]]), X.to(dev), device=dev)


# --------------------------------------------------------------------------------------------------
# (g2) SURVEY 8f N2: triplet sampling on the device
# --------------------------------------------------------------------------------------------------
def _chi2_ok(counts, probs, label, z=5.0):
    """Pearson chi-square of observed counts against a law, accepted within z sigma of its mean (dof, var 2 dof)."""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    keep = probs * counts.sum() >= 5
    c = np.append(counts[keep], counts[~keep].sum())
    q = np.append(probs[keep], probs[~keep].sum())
    c, q = c[q > 0], q[q > 0]
    stat = (((c - q * c.sum()) ** 2) / (q * c.sum())).sum()
    dof = len(c) - 1
    assert stat < dof + z * np.sqrt(2 * dof) + 10, (label, stat, dof)


def test_device_samplers_follow_the_laws_of_the_reference_loops(dev, capsys):
    """mfcd_sample_triplets (generation_data.py:16-224 on the device).  Philox stream, so parity is DISTRIBUTIONAL, as
    for the labels: per strategy the structural contract of the reference loop (unique, i != j, inside the strategy's
    candidate sets, `exclude` respected, attempt budgets and warnings) and chi-square tests of the marginals against the
    law the loop draws from — for popularity the law of numpy's choice(size=2, replace=False, p), computed in closed
    form; the host samplers, which replay the reference's generators, pass the same checks."""
    import generation_data as gd
    from mfcd import sampling
    torch.manual_seed(3)
    n, m = 6000, 40
    X = torch.randn(n, m)
    Xd = X.to(dev)

    def draw(strategy, want, exclude=None, seed=7, X_=Xd, **kw):
        rows = sampling.sample_triplets(X_, want, strategy, exclude, device=dev, seed=seed, **kw).cpu().numpy()
        assert rows.dtype == np.int32 and rows.ndim == 2 and rows.shape[1] == 3
        assert len({tuple(r) for r in rows.tolist()}) == rows.shape[0], strategy          # distinct
        nn, mm = X_.shape
        assert (rows[:, 1] != rows[:, 2]).all() and rows.min() >= 0
        assert rows[:, 0].max() < nn and rows[:, 1:].max() < mm
        return rows

    # random: uniform marginals, exclusion, reproducibility, independence of how the request is cut into blocks
    r = draw("random", 50000)
    assert r.shape[0] == 50000
    _chi2_ok(np.bincount(r[:, 1], minlength=m), np.full(m, 1 / m), "random i")
    _chi2_ok(np.bincount(r[:, 2], minlength=m), np.full(m, 1 / m), "random j")
    _chi2_ok(np.bincount(r[:, 0] % 97, minlength=97), np.bincount(np.arange(n) % 97) / n, "random u")
    assert np.array_equal(r, draw("random", 50000)) and not np.array_equal(r, draw("random", 50000, seed=8))
    assert np.array_equal(r[:1000], draw("random", 1000))              # attempt order: a shorter request is a prefix
    barred = {tuple(t) for t in r[:20000].tolist()}
    r2 = draw("random", 30000, exclude=barred)
    assert not ({tuple(t) for t in r2.tolist()} & barred)
    small = torch.randn(5, 4)
    full = draw("random", 60, X_=small.to(dev))                        # the whole support: 5 * 4 * 3
    assert full.shape[0] == 60
    with pytest.raises(ValueError):
        draw("random", 61, X_=small.to(dev))                           # the reference would spin forever

    # popularity: numpy's choice(size=2, replace=False, p): a ~ p; b ~ p, redrawn from p without a only if b == a
    pm = gd._popularity_probs(m, "zipf", 1.5)
    r = draw("popularity", 40000, popularity_method="zipf", alpha=1.5)
    assert r.shape[0] == 40000
    pair = np.outer(pm, pm) * (1 + (pm / (1 - pm))[:, None])
    np.fill_diagonal(pair, 0.0)
    assert abs(pair.sum() - 1) < 1e-12
    # kept triplets are DISTINCT draws: with n = 6000 users, 40 000 of them, duplicates of the head pair are frequent,
    # so the marginals are compared on the attempt law restricted to first occurrences: use few draws per (i, j) cell
    r_few = draw("popularity", 3000, popularity_method="zipf", alpha=1.5, seed=11)
    _chi2_ok(np.bincount(r_few[:, 1], minlength=m), pair.sum(axis=1), "popularity i")
    _chi2_ok(np.bincount(r_few[:, 2], minlength=m), pair.sum(axis=0), "popularity j")
    host = np.asarray(gd.choose_items_by_popularity(X, 3000, set()))
    _chi2_ok(np.bincount(host[:, 2], minlength=m), pair.sum(axis=0), "popularity j (host form)")

    # variance: sequential draw without replacement from var / sum(var)
    pv = torch.var(X, dim=0).double().numpy()
    pv /= pv.sum()
    r = draw("variance", 3000)
    seq = np.outer(pv, pv) / (1 - pv)[:, None]
    np.fill_diagonal(seq, 0.0)
    _chi2_ok(np.bincount(r[:, 1], minlength=m), seq.sum(axis=1), "variance i")
    _chi2_ok(np.bincount(r[:, 2], minlength=m), seq.sum(axis=0), "variance j")

    # proximity: i among the user's k best, j among the k worst, positions uniform
    k = 8
    best = torch.topk(X, k, dim=1)[1].numpy()
    worst = torch.topk(-X, k, dim=1)[1].numpy()
    r = draw("proximity", 30000, k=k)
    pos_i = (best[r[:, 0]] == r[:, 1:2]).argmax(axis=1)
    pos_j = (worst[r[:, 0]] == r[:, 2:3]).argmax(axis=1)
    assert (best[r[:, 0], pos_i] == r[:, 1]).all() and (worst[r[:, 0], pos_j] == r[:, 2]).all()
    _chi2_ok(np.bincount(pos_i, minlength=k), np.full(k, 1 / k), "proximity position i")
    _chi2_ok(np.bincount(pos_j, minlength=k), np.full(k, 1 / k), "proximity position j")

    # top_k: both among the k best (k = max(5, m // 10)), ordered pairs of distinct positions uniform; 3x budget
    k = 5
    best = torch.topk(X, k, dim=1)[1].numpy()
    r = draw("top_k", 30000)
    pos_i = (best[r[:, 0]] == r[:, 1:2]).argmax(axis=1)
    pos_j = (best[r[:, 0]] == r[:, 2:3]).argmax(axis=1)
    assert (best[r[:, 0], pos_i] == r[:, 1]).all() and (best[r[:, 0], pos_j] == r[:, 2]).all()
    cell = pos_i * k + pos_j
    probs = np.full(k * k, 1 / (k * (k - 1)))
    probs[::k + 1] = 0
    _chi2_ok(np.bincount(cell, minlength=k * k), probs, "top_k positions")
    capsys.readouterr()
    short = draw("top_k", 500, X_=torch.randn(6, 30).to(dev))          # support 6 * 5 * 4 = 120 < 500
    assert short.shape[0] <= 120 and "Only" in capsys.readouterr().out

    # margin: every kept pair within the adaptive margin, acceptance rate as the host form's
    want = 4000
    r = draw("margin", want)
    head = X[:10].numpy()
    margin = np.mean(head.max(axis=1) - head.min(axis=1)) * want / (n * m)
    xs = X.numpy()
    assert (np.abs(xs[r[:, 0], r[:, 1]] - xs[r[:, 0], r[:, 2]]) <= margin).all() and r.shape[0] == want
    FX = gd.FactoredMatrix(torch.randn(n, 6), torch.randn(m, 6))
    capsys.readouterr()
    rf = sampling.sample_triplets(FX, 200000, "margin", None, device=dev, seed=5, max_attempts=100000).cpu().numpy()
    out = capsys.readouterr().out
    assert "Only" in out and "after 100000 attempts" in out            # budget in blocks of 500, the reference's message
    head = FX.rows(0, 10)
    margin = np.mean(head.max(axis=1) - head.min(axis=1)) * 200000 / (n * m)
    assert 0 < rf.shape[0] < 200000 and (np.abs(FX.pair_diff(rf[:, 0], rf[:, 1], rf[:, 2])) <= margin * (1 + 1e-5)).all()

    # svd: users / items from the top-30 % projection-norm sets, 5x budget
    Xs = (torch.randn(200, 6) @ torch.randn(6, 90))
    r = draw("svd", 1500, X_=Xs.to(dev))
    import scipy.sparse.linalg as spla
    Us, Sv, Vt = spla.svds(Xs.numpy(), k=int(1500 / (200 * 90) * 200))
    top_u = set(np.argsort(np.linalg.norm(Us * Sv, axis=1))[-60:].tolist())
    top_i = set(np.argsort(np.linalg.norm(Vt.T * Sv, axis=1))[-27:].tolist())
    assert r.shape[0] == 1500 and set(r[:, 0].tolist()) <= top_u and set(r[:, 1].tolist()) | set(r[:, 2].tolist()) <= top_i


def test_device_sampler_feeds_the_reference_pipeline(dev):
    """structure.set_sampler_device + set_label_device: split_dataset_from_triplets (structure.py:666-742) with triplets
    and labels made on the GPU keeps the split sizes, the >= 500 test rows top-up, disjoint splits, and trains."""
    import structure as S
    n, m, d = 400, 300, 8
    X = S.generate_X(n, m, d, dev)
    S.set_sampler_device(dev)
    S.set_label_device(dev)
    try:
        torch.manual_seed(0)
        for strategy in ("random", "popularity", "top_k", "proximity", "margin"):
            tr, va, te = S.split_dataset_from_triplets(X, 3000, scale=1.0, K=2, strategy=strategy)
            for ld in (tr, va, te):      # triplets, split, labels and records were made in HBM; nothing on the host yet
                assert ld.dataset._mfcd_device_records() is not None and ld.dataset._rows is None, strategy
            rows = [np.asarray(ld.dataset.data)[:, :3].astype(np.int64) for ld in (tr, va, te)]
            sets = [{tuple(r) for r in x.tolist()} for x in rows]
            total = sum(len(s_) for s_ in sets)
            assert not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2]), strategy
            assert len(te.dataset) >= 500 and total <= 3000 + 250, strategy
            if strategy != "margin":
                assert len(sets[0]) == 2400 and len(sets[1]) == 300, strategy
        torch.manual_seed(1)
        a = S.get_triplets_from_X(X, 500, strategy="random")
        torch.manual_seed(1)
        assert a == S.get_triplets_from_X(X, 500, strategy="random")   # seeded through torch's global generator
        assert isinstance(a, set) and all(type(v) is int for t in a for v in t)
        tr, va, te = S.split_dataset_from_triplets(X, 1000, K=1, strategy="top_k")      # test part topped up to 500 (ref:721)
        parts = [{tuple(r[:3]) for r in np.asarray(ld.dataset.data).astype(np.int64).tolist()} for ld in (tr, va, te)]
        assert [len(p_) for p_ in parts] == [800, 100, 500] and not (parts[2] & (parts[0] | parts[1]))
        import generation_data as gd
        FX = gd.FactoredMatrix(*gd.generate_embedding_factors(2000, 1500, 8, "cpu", generator=torch.Generator().manual_seed(3)))
        ftr, fva, fte = S.split_dataset_from_triplets(FX, 20000, K=4, strategy="popularity", soft_label=True)
        assert len(ftr.dataset) == 16000 and len(fva.dataset) == 2000 * 4 and len(fte.dataset) == 2000 * 4
        assert ftr.dataset._mfcd_device_records().is_cuda
        tr, va, te = S.split_dataset_from_triplets(X, 6000, K=1, strategy="random")
    finally:
        S.set_sampler_device(None)
        S.set_label_device(None)
    model = S.MatrixFactorization(n, m, d).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=1e-5)
    tl, vl = S.train_model(model, tr, va, opt, dev, num_epochs=3)
    assert np.isfinite(tl).all() and tl[-1] < tl[0]


@pytest.mark.parametrize("n,m,N,B", [(16384, 16384, 64 * 12 + 5, 64), (30000, 20000, 64 * 30 + 1, 64),
                                     (65536, 65536, 64 * 40 + 9, 64), (8192, 8192, 16 * 50 + 3, 16)])
@pytest.mark.parametrize("flavour", ["ieee", "fast"])
def test_big_resident_form_is_bit_identical_to_the_streaming_step(dev, n, m, N, B, flavour):
    """mfcd_train_steps_big (moments of the whole model in registers, parameters in LDS, one wave per SIMD; third case:
    BASELINE configs[3]'s full table shape, 8 388 608 elements).  IEEE flavour: the streaming form's arithmetic —
    parameters, both moments and the step losses equal it BIT FOR BIT, over two calls (state written back and reloaded).
    Fast flavour (default; the resident form's hardware sqrt / rcp / exp2 with one Newton step): within the resident
    form's own tolerance of the streaming result."""
    from mfcd import engine
    d = 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=n % 97 + B)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        bind = engine.AdamBinding(model, opt)
        ref1 = engine.train_steps(bind, st.dev, B).clone()
        ref2 = engine.train_steps(bind, st.dev, B).clone()
    finally:
        engine.set_train_path("auto")
    m2, o2 = _model_from(U0, V0, dev, 1e-3, 1e-5)
    big = engine.BigResident(engine.AdamBinding(m2, o2))
    engine.set_resident_math(flavour)
    try:
        l1 = big.train_steps(st.dev, B).clone()
        big.status()
        l2 = big.train_steps(st.dev, B).clone()
        big.status()
    finally:
        engine.set_resident_math("fast")
    if flavour == "ieee":
        assert torch.equal(l1, ref1) and torch.equal(l2, ref2)
        assert torch.equal(m2.U.data, model.U.data) and torch.equal(m2.V.data, model.V.data)
        for prm, prm2 in ((model.U, m2.U), (model.V, m2.V)):
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[prm][key], o2.state[prm2][key]), key
    else:
        np.testing.assert_allclose(l2.cpu().numpy(), ref2.cpu().numpy(), rtol=2e-5, atol=2e-6)
        for nm, got, want in (("U", m2.U, model.U), ("V", m2.V, model.V)):
            assert_close_with_rare_outliers(got.data.cpu().numpy(), want.data.cpu().numpy(), 2e-6, 1e-3, nm)


def test_auto_takes_the_big_resident_form_for_c4_sized_states(dev):
    """engine.train_steps under "auto": a C4-shaped fp32 model (state beyond the regular resident form, d = 64) runs
    calls of >= 256 steps through the big resident form (pre-check of the stream included), shorter calls and
    `set_big_resident("off")` through the streaming form; results agree with the streaming form within the resident
    tolerance, and the fast path of later calls does not bypass the choice."""
    from mfcd import engine
    n = m = 65536
    d, B = 64, 64
    N = B * 300
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=77)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_big_resident("off")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        b0 = engine.AdamBinding(model, opt)
        engine.train_steps(b0, st.dev[: B * 20], B)
        ref = engine.train_steps(b0, st.dev, B).clone()
        assert getattr(b0, "_big", None) in (None, False) or b0._big.ws is None
    finally:
        engine.set_big_resident("auto")
    m2, o2 = _model_from(U0, V0, dev, 1e-3, 1e-5)
    b2 = engine.AdamBinding(m2, o2)
    engine.train_steps(b2, st.dev[: B * 20], B)            # short: streaming (and sets the binding's fast path)
    assert b2._big.ws is None
    got = engine.train_steps(b2, st.dev, B).clone()        # long: the big form, although a fast path exists
    assert b2._big.ws is not None and b2.step == 320
    engine.check_status()
    np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=2e-5, atol=2e-6)
    for nm, a, b in (("U", m2.U, model.U), ("V", m2.V, model.V)):
        assert_close_with_rare_outliers(a.data.cpu().numpy(), b.data.cpu().numpy(), 2e-6, 1e-3, nm)
    # a C2-shaped model is never offered the form
    U1, V1, u1, i1, j1, z1 = _synthetic(4096, 4096, 64, B * 300, seed=5)
    m3, o3 = _model_from(U1, V1, dev, 1e-3, 1e-5)
    b3 = engine.AdamBinding(m3, o3)
    engine.train_steps(b3, _records(u1, i1, j1, z1, 4096, 4096, dev).dev, B)
    assert b3._big is False


def test_train_model_on_a_c4_sized_model_goes_through_the_big_resident_form(dev):
    """structure.train_model (epoch loop, shuffling, validation passes, staged prologues of mfcd.engine.fit) on a C4-shaped
    model with epochs of 300 steps: the big resident form carries the epochs, and losses / factors agree with the run that
    streams (`set_big_resident("off")`) within the resident tolerance."""
    import structure as S
    from mfcd import engine
    n = m = 65536
    d, B = 64, 64
    N = B * 300 + 17
    U0, V0, u, i, j, z = _synthetic(n, m, d, N + 640, seed=91)
    rows = np.stack([u, i, j, z], 1)
    mk = lambda r, sh: torch.utils.data.DataLoader(ListDataset(r), batch_size=B, shuffle=sh)   # noqa: E731
    out = {}
    for mode in ("off", "auto"):
        engine.set_big_resident(mode)
        try:
            torch.manual_seed(3)
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            tl, vl = S.train_model(model, mk(rows[:N], True), mk(rows[N:], False), opt, dev, num_epochs=3)
            engine.check_status()
        finally:
            engine.set_big_resident("auto")
        out[mode] = (np.asarray(tl), np.asarray(vl), model.U.data.cpu().numpy(), model.V.data.cpu().numpy(),
                     float(opt.state[model.U]["step"]))
    assert out["auto"][4] == out["off"][4] == 3 * 301
    np.testing.assert_allclose(out["auto"][0], out["off"][0], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(out["auto"][1], out["off"][1], rtol=2e-5, atol=2e-6)
    assert_close_with_rare_outliers(out["auto"][2], out["off"][2], 3e-6, 1e-3, "U")
    assert_close_with_rare_outliers(out["auto"][3], out["off"][3], 3e-6, 1e-3, "V")


def test_auto_streams_a_c4_sized_model_when_the_stream_concentrates_on_few_rows(dev):
    """A Zipf-head stream (item 0 in ~40 % of the samples, hundreds of references into one wave's slice per batch) fails
    the big form's pre-check: "auto" must stream such calls — bit-identical to the forced streaming path — and say
    nothing."""
    from mfcd import engine
    n = m = 65536
    d, B = 64, 64
    N = B * 260
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=12)
    rng = np.random.default_rng(5)
    i = np.where(rng.random(N) < 0.4, 0, i)
    j = np.where(i == j, (j + 1) % m, j)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).clone()
    finally:
        engine.set_train_path("auto")
    m2, o2 = _model_from(U0, V0, dev, 1e-3, 1e-5)
    b2 = engine.AdamBinding(m2, o2)
    got = engine.train_steps(b2, st.dev, B).clone()
    engine.check_status()
    assert b2._big is not False and b2._big.ws is None          # offered, pre-check said no, never launched
    assert torch.equal(got, ref) and torch.equal(m2.U.data, model.U.data) and torch.equal(m2.V.data, model.V.data)


def test_big_resident_form_refuses_streams_that_concentrate_on_one_wave(dev):
    """A small table puts dozens of a batch's rows into one wave's slice: the form says so (status 2 -> MfcdError)
    instead of running out of gradient slots; shapes it does not take raise NotImplementedError."""
    from mfcd import engine, _lib
    U0, V0, u, i, j, z = _synthetic(300, 200, 64, 64 * 3, seed=4)
    st = _records(u, i, j, z, 300, 200, dev)
    mdl, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
    big = engine.BigResident(engine.AdamBinding(mdl, opt))
    big.train_steps(st.dev, 64)
    with pytest.raises(_lib.MfcdError):
        big.status()
    U1, V1, *_ = _synthetic(50, 40, 32, 64, seed=5)
    m1, o1 = _model_from(U1, V1, dev, 1e-3, 1e-5)
    with pytest.raises(NotImplementedError):
        engine.BigResident(engine.AdamBinding(m1, o1))


# --------------------------------------------------------------------------------------------------
# (h) VERDICT r1 item 5: row-sharded state, batch 64 (strong scaling), results equal to one GPU
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,n,m,d,N", [(w, *shp) for w in (1, 2, 3, 8) for shp in
                                           ((300, 200, 64, 64 * 40 + 7), (37, 29, 5, 64 * 12 + 1), (5, 3, 16, 64 * 6))] +
                         [(8, 65536, 65536, 64, 64 * 6 + 5)])       # world 8 at BASELINE configs[3] (C4) table shape
def test_row_sharded_rehearsal_is_bit_identical_to_the_streaming_step(dev, world, n, m, d, N):
    """mfcd_shard_train_steps without a communicator plays every rank in this process (pack of the owned rows ->
    union of the packs = what the integer all-reduce yields -> fused step per shard, in place).  With the batch kept at
    B = 64 the result must equal mfcd_train_steps' streaming form BIT FOR BIT: parameters, both moments, step losses.
    Shapes: aligned rows; odd d (rows straddle workgroups, scalar path); fewer rows than ranks (empty shards)."""
    from mfcd import dist as mdist, engine
    B = 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=world * 7 + d)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).clone()
    finally:
        engine.set_train_path("auto")
    model2, opt2 = _model_from(U0, V0, dev, 1e-3, 1e-5)
    bind2 = engine.AdamBinding(model2, opt2)
    loss = mdist.NativeShard(bind2, simulate_world=world).train_steps(st.dev, B)
    assert bind2.step == (N + B - 1) // B
    assert torch.equal(loss, ref_loss)
    assert torch.equal(model2.U.data, model.U.data) and torch.equal(model2.V.data, model.V.data)
    for prm, prm2 in ((model.U, model2.U), (model.V, model2.V)):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[prm][key], opt2.state[prm2][key]), key


@pytest.mark.parametrize("world", [1, 3, 8])
def test_pipelined_shard_exchange_equals_the_strict_chain(dev, world):
    """the exchange of batch k+1 runs under step k wherever the two batches share no row — its rows
    are packed AHEAD of step k, rolled forward over it with the step kernel's own dense update (zero sparse gradient).
    At a shape where both kinds of pair occur (about a quarter of the consecutive batches share no row) the pipelined
    chain (default), the strict chain (MFCD_TUNE_SHARD_PIPELINE 0) and the single-GPU streaming step agree BIT FOR
    BIT; the device collision marks equal the host form the Python-level loop uses."""
    from mfcd import _lib, dist as mdist, engine
    n, m, d, B, N = 20000, 15000, 16, 64, 64 * 60 + 9
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=world + 40)
    st = _records(u, i, j, z, n, m, dev)
    nsteps = (N + B - 1) // B
    flags = torch.full((nsteps,), 7, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().mfcd_shard_collisions(_lib.ptr(st.dev), N, B, _lib.ptr(flags), _lib.stream_ptr(dev)))
    want = mdist.batch_collisions(st.dev.cpu().numpy(), B)
    assert np.array_equal(flags.cpu().numpy().astype(bool), want) and not want[-1]
    free = int((~want[:-1]).sum())
    assert 5 <= free <= nsteps - 6, free                       # both kinds of pair are exercised
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).clone()
    finally:
        engine.set_train_path("auto")
    runs = {}
    for chain in (1, 0):
        engine.set_tuning(shard_pipeline=chain)
        try:
            mk, ok = _model_from(U0, V0, dev, 1e-3, 1e-5)
            loss = mdist.NativeShard(engine.AdamBinding(mk, ok), simulate_world=world).train_steps(st.dev, B).clone()
        finally:
            engine.set_tuning(shard_pipeline=1)
        runs[chain] = (mk, ok, loss)
    for chain, (mk, ok, loss) in runs.items():
        assert torch.equal(loss, ref_loss), chain
        assert torch.equal(mk.U.data, model.U.data) and torch.equal(mk.V.data, model.V.data), chain
        for prm, prm2 in ((model.U, mk.U), (model.V, mk.V)):
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[prm][key], ok.state[prm2][key]), (chain, key)


@pytest.mark.parametrize("world,n,m,d,N,chain", [(1, 300, 200, 64, 64 * 20 + 7, 1), (3, 300, 200, 64, 64 * 20 + 7, 1),
                                                 (8, 20000, 15000, 16, 64 * 40 + 9, 1), (8, 20000, 15000, 16, 64 * 40 + 9, 0),
                                                 (8, 16384, 16384, 128, 64 * 5 + 3, 1)])
def test_row_sharded_loop_with_bf16_factor_tables(dev, world, n, m, d, N, chain):
    """VERDICT r2 missing item 5: mfcd_shard_train_steps_bf16 — bf16 factor shards (BASELINE configs[2]'s storage; last
    case its table shape), fp32 exchange buffer / moments / arithmetic, both chains (the pipelined one rolls a row
    forward and rounds it to bf16 exactly where the step kernel does) — is bit-identical to mfcd_train_steps_bf16's
    streaming form with the same batch size: tables, both moments, step losses."""
    import structure as S
    from mfcd import dist as mdist, engine
    B = 64
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=300 + world + d)
    st = _records(u, i, j, z, n, m, dev)

    def fresh():
        model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16)
        with torch.no_grad():
            model.U.copy_(torch.from_numpy(U0))
            model.V.copy_(torch.from_numpy(V0))
        model = model.to(dev)
        return model, torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    engine.set_train_path("streaming")
    try:
        model, opt = fresh()
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).clone()
    finally:
        engine.set_train_path("auto")
    engine.set_tuning(shard_pipeline=chain)
    try:
        m2, o2 = fresh()
        loss = mdist.NativeShard(engine.AdamBinding(m2, o2), simulate_world=world).train_steps(st.dev, B)
    finally:
        engine.set_tuning(shard_pipeline=1)
    assert m2.U.dtype == torch.bfloat16 and torch.equal(loss, ref_loss)
    assert torch.equal(m2.U.data, model.U.data) and torch.equal(m2.V.data, model.V.data)
    for prm, prm2 in ((model.U, m2.U), (model.V, m2.V)):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[prm][key], o2.state[prm2][key]), key


def test_row_sharded_halves_over_a_one_rank_rccl_group(dev):
    """The split form (pack -> torch.distributed all_reduce of the int32 view -> apply) and the native loop over an
    RCCL communicator, each on a one-rank group: same bits as the streaming step."""
    import os
    import torch.distributed as dist
    from mfcd import dist as mdist, engine
    n, m, d, B, N = 128, 96, 32, 64, 64 * 9 + 5
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=21)
    st = _records(u, i, j, z, n, m, dev)
    engine.set_train_path("streaming")
    try:
        model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
        ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).clone()
    finally:
        engine.set_train_path("auto")
    created = not dist.is_initialized()
    if created:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29536")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        m2, o2 = _model_from(U0, V0, dev, 1e-3, 1e-5)
        b2 = engine.AdamBinding(m2, o2)
        shard = mdist.RowShard(b2, 0, 1)
        loss = mdist.train_steps_sharded(mdist.HipShardCompute(shard), st.dev, B, 0, b2.hyper())
        shard.gather()
        np.testing.assert_allclose(loss.cpu().numpy(), ref_loss.cpu().numpy(), rtol=2e-6, atol=1e-7)
        assert torch.equal(m2.U.data, model.U.data) and torch.equal(m2.V.data, model.V.data)
        m3, o3 = _model_from(U0, V0, dev, 1e-3, 1e-5)
        b3 = engine.AdamBinding(m3, o3)
        try:
            nat = mdist.NativeShard(b3)
        except Exception as e:   # RCCL not loadable inside the library on this box: the split form above is the path
            pytest.skip(f"native RCCL loop unavailable: {e}")
        loss3 = nat.train_steps(st.dev, B)
        nat.gather()
        nat.close()
        assert torch.equal(loss3, ref_loss)
        assert torch.equal(m3.U.data, model.U.data) and torch.equal(m3.V.data, model.V.data)
        # the pipelined exchange over a real communicator (side stream, two buffers, events): a shape where most
        # consecutive batches share no row, both chains of the native loop and both of the Python-level loop
        n, m, d, N = 30000, 30000, 32, 64 * 50 + 3
        U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=22)
        st = _records(u, i, j, z, n, m, dev)
        assert (~mdist.batch_collisions(st.dev.cpu().numpy(), B)[:-1]).sum() > 10
        engine.set_train_path("streaming")
        try:
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            ref_loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).clone()
        finally:
            engine.set_train_path("auto")
        for chain in (2, 1, 0):              # 2: pipelined on this one-rank communicator too (1 = auto: strict here)
            engine.set_tuning(shard_pipeline=chain)
            try:
                m4, o4 = _model_from(U0, V0, dev, 1e-3, 1e-5)
                nat = mdist.NativeShard(engine.AdamBinding(m4, o4))
                loss4 = nat.train_steps(st.dev, B).clone()
                nat.gather()
                nat.close()
            finally:
                engine.set_tuning(shard_pipeline=1)
            assert torch.equal(loss4, ref_loss), chain
            assert torch.equal(m4.U.data, model.U.data) and torch.equal(m4.V.data, model.V.data), chain
            m5, o5 = _model_from(U0, V0, dev, 1e-3, 1e-5)
            b5 = engine.AdamBinding(m5, o5)
            shard = mdist.RowShard(b5, 0, 1)
            mdist.train_steps_sharded(mdist.HipShardCompute(shard), st.dev, B, 0, b5.hyper(), pipelined=bool(chain))
            shard.gather()
            assert torch.equal(m5.U.data, model.U.data) and torch.equal(m5.V.data, model.V.data), chain
    finally:
        if created:
            dist.destroy_process_group()


# --------------------------------------------------------------------------------------------------
# (i) boundary B1: autograd-capable forward, generic optimisers, index validation
# --------------------------------------------------------------------------------------------------
def test_forward_builds_an_autograd_graph_and_any_optimiser_trains(dev):
    """MatrixFactorization.forward (structure.py:773-795) must support `loss.backward()` as in the reference; gradients
    against plain fp32 torch ops of the same formula; `train_model` with SGD (not fused) against the eager torch loop;
    more samples than one kernel batch; out-of-range indices raise IndexError like U[u]."""
    import torch.nn.functional as F
    import structure as S
    n, m, d, N = 200, 150, 16, 20000
    rng = np.random.default_rng(2)
    torch.manual_seed(4)
    model = S.MatrixFactorization(n, m, d).to(dev)
    u = torch.from_numpy(rng.integers(0, n, N))
    i = torch.from_numpy(rng.integers(0, m, N))
    j = torch.from_numpy((i.numpy() + 1 + rng.integers(0, m - 1, N)) % m)
    z = torch.from_numpy(rng.integers(0, 2, N).astype(np.float32)).to(dev)
    p = model(u, i, j)                                   # N > 16384: several kernel batches
    assert p.shape == (N,) and p.requires_grad
    loss = F.binary_cross_entropy(p, z)
    loss.backward()
    U2 = model.U.detach().clone().requires_grad_(True)
    V2 = model.V.detach().clone().requires_grad_(True)
    ud, idd, jd = u.to(dev), i.to(dev), j.to(dev)
    p2 = torch.sigmoid((U2[ud] * (V2[idd] - V2[jd])).sum(dim=1))
    F.binary_cross_entropy(p2, z).backward()
    np.testing.assert_allclose(p.detach().cpu().numpy(), p2.detach().cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(model.U.grad.cpu().numpy(), U2.grad.cpu().numpy(), rtol=1e-4, atol=2e-7)
    np.testing.assert_allclose(model.V.grad.cpu().numpy(), V2.grad.cpu().numpy(), rtol=1e-4, atol=2e-7)
    with torch.no_grad():
        assert not model(u[:10], i[:10], j[:10]).requires_grad
    with pytest.raises(IndexError):
        model(torch.tensor([n]), torch.tensor([0]), torch.tensor([1]))
    from mfcd import metrics
    with pytest.raises(IndexError):
        metrics.uvt_rows(model.U.data, model.V.data, [0, n])
    # a non-Adam optimiser goes through the generic loop (same kernels), against the eager torch loop
    rows = np.stack([u.numpy()[:3000], i.numpy()[:3000], j.numpy()[:3000], z.cpu().numpy()[:3000]], 1).astype(np.float64)
    loader = torch.utils.data.DataLoader(ListDataset(rows), batch_size=64, shuffle=False)
    torch.manual_seed(5)
    ma = S.MatrixFactorization(n, m, d).to(dev)
    Ub, Vb = ma.U.detach().clone().requires_grad_(True), ma.V.detach().clone().requires_grad_(True)
    opt_a = torch.optim.SGD(ma.parameters(), lr=0.5, momentum=0.9)
    opt_b = torch.optim.SGD([Ub, Vb], lr=0.5, momentum=0.9)
    tl, vl = S.train_model(ma, loader, loader, opt_a, dev, num_epochs=2)
    ref = []
    rt = torch.from_numpy(rows).to(dev)
    for _ in range(2):
        tot = 0.0
        for off in range(0, 3000, 64):
            b = rt[off:off + 64]
            opt_b.zero_grad()
            pb = torch.sigmoid((Ub[b[:, 0].long()] * (Vb[b[:, 1].long()] - Vb[b[:, 2].long()])).sum(1))
            lb = F.binary_cross_entropy(pb, b[:, 3].float())
            lb.backward()
            opt_b.step()
            tot += lb.item()
        ref.append(tot / 47)
    np.testing.assert_allclose(tl, ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ma.U.detach().cpu().numpy(), Ub.detach().cpu().numpy(), rtol=0, atol=5e-6)
    assert len(vl) == 2 and vl[1] < vl[0]


@pytest.mark.parametrize("n,m,d,steps", [(16384, 16384, 128, 40), (4096, 4096, 64, 120), (2048, 1024, 256, 60)])
def test_resident_form_with_bf16_factor_tables(dev, orc, n, m, d, steps):
    """BASELINE configs[2] in the RESIDENT form (first case = its shape: 2048 waves x 32 registers per array, row
    gradients in LDS): bf16 tables in HBM, fp32 registers rounded to bf16 after every update — the rounding point the
    oracle defines.
      IEEE flavour: parameters, moments and losses must match the oracle as the streaming bf16 form does (almost every
        element bit-equal, the rest within one bf16 ulp) — the machinery is exact.
      fast flavour (default; v_sqrt / Newton-corrected rcp, a few fp32 ulp per update): an fp32 ulp can flip a bf16
        rounding (2^-8 relative), and Adam turns a flipped input into a move of up to ~lr on the few elements of TOUCHED
        rows whose gradient nearly cancels (measured with tools/diag_bf16_resident.py: 1.8e-4 of the elements, touched
        rows only, the oracle reacts the same way to a one-ulp input change).  Accepted: <= 2e-3 of the elements
        beyond one bf16 ulp, none beyond 5 lr (rows hit again keep diverging for a few steps), mean difference <= 2e-7,
        untouched rows within one bf16 ulp, losses within 1e-4.
    Also the fp32 resident run at the same shape against the fp32 oracle."""
    from mfcd import engine
    from oracle import oracle as O
    import structure as S
    B = 64
    N = B * steps - 7
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=31 + d)
    st = _records(u, i, j, z, n, m, dev)
    Ub, Vb = orc.round_bf16(U0.copy()), orc.round_bf16(V0.copy())

    def run_bf16():
        model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16)
        with torch.no_grad():
            model.U.copy_(torch.from_numpy(Ub))
            model.V.copy_(torch.from_numpy(Vb))
        model = model.to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
        loss = engine.train_steps(engine.AdamBinding(model, opt), st.dev, B).cpu().numpy()
        engine.check_status()
        return loss, model.U.data.float().cpu().numpy(), model.V.data.float().cpu().numpy()

    engine.set_train_path("resident")
    try:
        assert engine.train_plan(N, B, n, m, d, bf16=True)["form_name"] == "resident"
        engine.set_resident_math("ieee")
        exact = run_bf16()
        engine.set_resident_math("fast")
        fast = run_bf16()
        m32, o32 = _model_from(U0, V0, dev, 1e-3, 1e-5)
        loss32 = engine.train_steps(engine.AdamBinding(m32, o32), st.dev, B).cpu().numpy()
        engine.check_status()
    finally:
        engine.set_resident_math("fast")
        engine.set_train_path("auto")
    ref = O.new_state(Ub, Vb)
    ref_loss = orc.train_steps(ref, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=8, bf16_factors=True)
    touched = {"U": np.zeros(n, bool), "V": np.zeros(m, bool)}
    touched["U"][u] = True
    touched["V"][i] = True
    touched["V"][j] = True
    start = {"U": Ub, "V": Vb}
    for flavour, (loss, gU, gV) in (("ieee", exact), ("fast", fast)):
        np.testing.assert_allclose(loss, ref_loss, rtol=0, atol=1e-4, err_msg=flavour)
        for nm, got in (("U", gU), ("V", gV)):
            diff = np.abs(got - ref[nm])
            # one bf16 ulp at the magnitude the element HAD: a flipped rounding keeps its absolute size while an element
            # decays towards zero (dense Adam moves it by ~lr per step), so the ulp of the final value is the wrong ruler
            ulps = diff / (np.maximum(np.abs(ref[nm]), np.abs(start[nm])) * 2.0 ** -7 + 1e-30)
            if flavour == "ieee":
                assert (diff > 0).mean() < 2e-3, f"{nm}: {(diff > 0).mean():.2e} of the elements differ"
                assert ulps.max() <= 1.0, f"{nm} ieee: {int((ulps > 1).sum())} elements beyond one bf16 ulp, worst {ulps.max():.1f}"
            else:
                assert (ulps > 1).mean() <= 2e-3, f"{nm} fast: {(ulps > 1).mean():.2e} of the elements beyond one bf16 ulp"
                assert diff.max() <= 5e-3, f"{nm} fast: max difference {diff.max():.2e}"      # a few Adam steps (lr = 1e-3)
                assert diff.mean() <= 2e-7, f"{nm} fast: mean difference {diff.mean():.2e}"
                assert ulps[~touched[nm]].max(initial=0.0) <= 1.0, f"{nm} fast: an untouched row differs by more than one bf16 ulp"
    r32 = O.new_state(U0, V0)
    r32_loss = orc.train_steps(r32, u, i, j, z, B, 0, lr=1e-3, wd=1e-5, threads=8)
    np.testing.assert_allclose(loss32, r32_loss, rtol=2e-5, atol=2e-6)
    assert_close_with_rare_outliers(m32.U.data.cpu().numpy(), r32["U"], 2e-6 + 2e-8 * steps, 1e-3, "fp32 resident U")
    assert_close_with_rare_outliers(m32.V.data.cpu().numpy(), r32["V"], 2e-6 + 2e-8 * steps, 1e-3, "fp32 resident V")


@pytest.mark.parametrize("n,m,d", [(4096, 4096, 64), (1003, 333, 256), (300, 5000, 128), (257, 95, 2), (640, 512, 32)])
def test_uvt_select_computes_only_what_is_asked_with_the_same_sums(dev, orc, n, m, d):
    """mfcd_uvt_stats_select: the rows-only pass (what compute_alpha_and_norm_ratios reads) and the error-only pass
    (what compute_reconstruction_error reads) against the full pass: row sums bit-equal (same arithmetic, less of it), the error sum
    to f64 rounding (the same shares added in another order), ||sX||^2 (a different summation path in the error-only pass) to 1e-6."""
    from mfcd import metrics
    rng = np.random.default_rng(n + d)
    U = torch.from_numpy((rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)).to(dev)
    V = torch.from_numpy((rng.standard_normal((m, d)) / np.sqrt(d)).astype(np.float32)).to(dev)
    X = torch.from_numpy((rng.standard_normal((n, m)) * 0.5 + 0.3).astype(np.float32)).to(dev)
    rs3, sc3 = metrics.uvt_stats(U, V, X, 0.8, what=3)
    rs1, none1 = metrics.uvt_stats(U, V, X, 0.8, what=1)
    none2, sc2 = metrics.uvt_stats(U, V, X, 0.8, what=2)
    assert none1 is None and none2 is None
    assert torch.equal(rs1, rs3)
    assert float(sc2[0]) == pytest.approx(float(sc3[0]), rel=1e-12)   # same f64 shares, summed by one workgroup
    assert float(sc2[1]) == pytest.approx(float(sc3[1]), rel=1e-6)
    ref_rows, err2, ref2 = orc.uvt_stats(U.cpu().numpy(), V.cpu().numpy(), X.cpu().numpy(), 0.8)
    assert float(sc2[0]) == pytest.approx(err2, rel=2e-5) and float(sc2[1]) == pytest.approx(ref2, rel=2e-5)
    np.testing.assert_allclose(rs1[:, 1].cpu().numpy(), ref_rows[:, 1], rtol=2e-5)


@pytest.mark.parametrize("n,m,d,dx,slab", [(3000, 2000, 64, 16, 1024), (1111, 777, 128, 8, 500), (700, 300, 8, 4, 256)])
def test_uvt_pass_over_a_factored_ground_truth_equals_the_dense_pass(dev, n, m, d, dx, slab):
    """X kept as factors goes through the pass in row slabs (mfcd_uvt_stats_slab).  With the slab's rows
    formed by the same GEMM, per-row sums and the global sums (added slab by slab in f64) must equal the dense pass to
    fp32 rounding; compute_reconstruction_error accepts the factored X."""
    import generation_data as gd
    import structure as S
    from mfcd import metrics
    A, Bf = gd.generate_embedding_factors(n, m, dx, "cpu", generator=torch.Generator().manual_seed(n))
    FX = gd.FactoredMatrix(A, Bf)
    torch.manual_seed(1)
    model = S.MatrixFactorization(n, m, d).to(dev)
    U, V = model.U.data, model.V.data
    rs_f, sc_f = metrics.uvt_stats_factored(U, V, FX, 0.9, what=3, slab_rows=slab)
    # dense X assembled from the SAME slab products
    X = torch.cat([(A[r0:r0 + slab].to(dev) @ Bf.to(dev).t()) for r0 in range(0, n, slab)])
    rs_d, sc_d = metrics.uvt_stats(U, V, X, 0.9, what=3)
    # the slab pass splits the columns by ITS row count, so per-tile fp32 sums group differently: fp32-rounding level
    a, b = rs_f.cpu().numpy(), rs_d.cpu().numpy()
    for col in range(6):
        np.testing.assert_allclose(a[:, col], b[:, col], rtol=2e-5, atol=2e-5 * np.abs(b[:, col]).max(), err_msg=f"row_stats[{col}]")
    np.testing.assert_allclose(sc_f.cpu().numpy()[:2], sc_d.cpu().numpy()[:2], rtol=2e-6)
    assert S.compute_reconstruction_error(model, FX, 0.9) == pytest.approx(S.compute_reconstruction_error(model, X, 0.9), rel=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,d,cuts", [(3000, 2048, 64, [0, 1500, 3000]), (2500, 1000, 128, [0, 700, 700, 2500]),
                                        (4096, 4096, 64, [0, 512, 1024, 1536, 2048, 2560, 3072, 3584, 4096])])
def test_row_block_sharded_uvt_pass_rehearsal_and_one_rank_group(dev, orc, n, m, d, cuts):
    """SURVEY 8e G1 (eval pass): X sharded by row blocks.  Rehearsal in one process: every rank's block through
    mfcd_uvt_stats_slab, shares added in rank order, against the one-pass result (per-tile fp32 sums group by the slab's
    own column split: fp32-rounding level, as for the factored form) and against the oracle; then the collective form
    itself on a one-rank RCCL group, which must reproduce the plain pass's assembly."""
    import os
    import torch.distributed as dist
    from mfcd import dist as mdist, metrics
    g = torch.Generator().manual_seed(n + d)
    U = (torch.randn(n, d, generator=g) / d ** 0.5).to(dev)
    V = (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
    X = (torch.randn(n, m, generator=g) * 0.5 + 0.1).to(dev)
    rs_d, sc_d = metrics.uvt_stats(U, V, X, 0.9)
    blocks, scal = [], torch.zeros(4, dtype=torch.float64, device=dev)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            rs, share = mdist.hip_slab_pass(U, V, X[lo:hi], lo, 0.9, 3)
            blocks.append(rs)
            scal += share
    rs_s = torch.cat(blocks)
    a, b = rs_s.cpu().numpy(), rs_d.cpu().numpy()
    for col in range(6):
        scale = np.abs(b[:, col]).max() + 1e-30
        assert np.abs(a[:, col] - b[:, col]).max() <= 2e-5 * scale, col
    np.testing.assert_allclose(scal[:2].cpu().numpy(), sc_d[:2].cpu().numpy(), rtol=2e-6)
    if n * m <= 4_000_000:
        ref_rows, err2, ref2 = orc.uvt_stats(U.cpu().numpy(), V.cpu().numpy(), X.cpu().numpy(), 0.9)
        assert float(scal[0]) == pytest.approx(err2, rel=2e-5) and float(scal[1]) == pytest.approx(ref2, rel=2e-5)
    created = not dist.is_initialized()
    if created:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29537")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        rs1, sc1 = mdist.uvt_stats_sharded(U, V, X, 0, 0.9, what=3)
        one, share = mdist.hip_slab_pass(U, V, X, 0, 0.9, 3)
        assert torch.equal(rs1, one) and torch.equal(sc1, share)
        err = mdist.reconstruction_error_sharded(U, V, X, 0, 0.9)
        assert err == pytest.approx(metrics.reconstruction_error(U, V, X, 0.9), rel=1e-6)
        with pytest.raises(ValueError):
            mdist.uvt_stats_sharded(U, V, X[: n // 2], 0, 0.9)      # blocks must tile all rows
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.gpu
def test_uvt_column_split_knobs_change_the_grouping_not_the_result(dev, orc):
    """MFCD_TUNE_UVT_TARGET_WGS / MFCD_TUNE_UVT_MIN_STAGES only move the column split: per-row sums and global sums agree
    to fp32 rounding of the per-tile partial sums across settings, and with the oracle."""
    from mfcd import engine, metrics
    n, m, d = 2048, 4096, 64
    g = torch.Generator().manual_seed(77)
    U = (torch.randn(n, d, generator=g) / d ** 0.5).to(dev)
    V = (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
    X = (torch.randn(n, m, generator=g) * 0.5 - 0.2).to(dev)
    ref_rows, err2, ref2 = orc.uvt_stats(U.cpu().numpy(), V.cpu().numpy(), X.cpu().numpy(), 1.1)
    try:
        outs = []
        for wgs, mst in ((512, 8), (4096, 8), (4096, 2), (256, 16)):
            engine.set_tuning(uvt_target_wgs=wgs, uvt_min_stages=mst)
            rs, sc = metrics.uvt_stats(U, V, X, 1.1)
            outs.append((rs.cpu().numpy(), sc.cpu().numpy()))
            assert float(sc[0]) == pytest.approx(err2, rel=2e-5) and float(sc[1]) == pytest.approx(ref2, rel=2e-5)
        base_rows, base_sc = outs[0]
        for rows, sc in outs[1:]:
            for col in range(6):
                scale = np.abs(base_rows[:, col]).max() + 1e-30
                assert np.abs(rows[:, col] - base_rows[:, col]).max() <= 2e-5 * scale, col
            np.testing.assert_allclose(sc[:2], base_sc[:2], rtol=2e-6)
        with pytest.raises(Exception):
            engine.set_tuning(uvt_target_wgs=1)
    finally:
        engine.set_tuning(uvt_target_wgs=512, uvt_min_stages=8)


@pytest.mark.gpu
def test_models_of_different_shapes_keep_their_own_planned_workspaces(dev):
    """Two models of different table shapes trained alternately on one stream: each keeps its planned workspace (no
    re-plan per call), results equal training each alone; beyond six shapes per stream the least recently used
    workspace is released and its sticky status word is still checked."""
    from mfcd import engine
    shapes = [(512, 384, 32), (300, 700, 16)]
    data = []
    for n, m, d in shapes:
        U0, V0, u, i, j, z = _synthetic(n, m, d, 64 * 12 + 5, seed=n)
        data.append((U0, V0, _records(u, i, j, z, n, m, dev)))

    def alone(k):
        model, opt = _model_from(data[k][0], data[k][1], dev, 1e-3, 1e-5)
        bind = engine.AdamBinding(model, opt)
        for _ in range(3):
            engine.train_steps(bind, data[k][2].dev, 64)
        return model.U.data.clone(), model.V.data.clone()

    ref = [alone(0), alone(1)]
    models = [_model_from(U0, V0, dev, 1e-3, 1e-5) for U0, V0, _ in data]
    binds = [engine.AdamBinding(mo, op) for mo, op in models]
    bufs = [None, None]
    for rep in range(3):
        for k in (0, 1):
            engine.train_steps(binds[k], data[k][2].dev, 64)
            ws = engine.workspace_for(dev, shapes[k])
            if bufs[k] is None:
                bufs[k] = ws.buf
            assert ws.buf is bufs[k], "a model's workspace was re-planned by the other model's calls"
    for k in (0, 1):
        assert torch.equal(models[k][0].U.data, ref[k][0]) and torch.equal(models[k][0].V.data, ref[k][1])
    for extra in range(7):                                   # more shapes than the per-stream cap: LRU release
        n, m, d = 128 + 64 * extra, 128, 8
        U0, V0, u, i, j, z = _synthetic(n, m, d, 64 * 3, seed=extra)
        mo, op = _model_from(U0, V0, dev, 1e-3, 1e-5)
        engine.train_steps(engine.AdamBinding(mo, op), _records(u, i, j, z, n, m, dev).dev, 64)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    assert sum(1 for key in engine._workspaces if key[0] == idx) <= 6 * len({key[1] for key in engine._workspaces if key[0] == idx})
    engine.check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rank-d", "rank-d + noise", "full rank, flat spectrum"])
def test_singular_value_error_from_the_top_of_the_spectrum_equals_the_dense_solver(dev, kind):
    """svd_error_scaled (structure.py:1011-1017) needs only the min(d, n, m) largest singular values of the centred X and
    its Frobenius norm (the rest of UV^T's spectrum is zero).  The block-iteration path must agree with the dense
    eigen-solver path to 1e-9 where it accepts its result, and hand over to the dense path where the spectrum does not
    let it converge."""
    from mfcd import metrics
    n, m, d = 700, 900, 16
    g = torch.Generator().manual_seed(5)
    A, Bm = torch.randn(n, d, generator=g), torch.randn(m, d, generator=g)
    X = (A @ Bm.t()) / d ** 0.5
    if kind == "rank-d + noise":
        X = X + 0.05 * torch.randn(n, m, generator=g)
    if kind == "full rank, flat spectrum":
        X = torch.randn(n, m, generator=g)
    X = X.to(dev).contiguous()
    U = (torch.randn(n, d, generator=g) / d ** 0.5).to(dev)
    V = (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
    xm = X.mean(1)
    ok = np.ones(n, dtype=bool)
    metrics._x_top_cache.clear(); metrics._x_spectrum_cache.clear()
    _, fast, failed = metrics.spearman_and_svd(U, V, xm, X, 0.7, ok)
    took_fast = metrics._x_top_cache._val is not None
    assert not failed
    real = metrics._x_top_spectrum
    metrics._x_top_spectrum = lambda *a, **k: None          # force the dense path
    try:
        _, dense, failed2 = metrics.spearman_and_svd(U, V, xm, X, 0.7, ok)
    finally:
        metrics._x_top_spectrum = real
    assert not failed2
    assert fast == pytest.approx(dense, rel=1e-9, abs=1e-12)
    if kind == "rank-d":
        assert took_fast, "a rank-d matrix must converge in the block iteration"
    if kind == "full rank, flat spectrum":
        assert not took_fast, "a flat spectrum must be handed to the dense solver"


# --------------------------------------------------------------------------------------------------
# round 3: parity holes named by the round-2 review
# --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["rank-d", "rank-d + noise"])
def test_alpha_and_norm_ratios_at_2048_squared_match_the_oracle(dev, kind):
    """compute_alpha_and_norm_ratios (structure.py:958-1082) at 2048 x 2048, d = 64 against the oracle's restatement
    (numpy SVDs of the centred matrices, scipy ranks): all 14 outputs at the north-star bound 1e-4 (scaled by the
    magnitude of the reference value), in particular svd_err, which the product path takes from a block iteration on
    the top of X's spectrum.  Fixture sizes (<= 256^2) could not tell a wrong tail term from a right one."""
    import structure as S
    from oracle import oracle as O
    n = m = 2048
    d = 64
    g = torch.Generator().manual_seed(77 if kind == "rank-d" else 78)
    A, Bm = torch.randn(n, d, generator=g), torch.randn(m, d, generator=g)
    X = (A @ Bm.t()) / (2.0 * d ** 0.5)
    if kind == "rank-d + noise":
        X = X + 0.05 * torch.randn(n, m, generator=g)
    U0 = (0.6 * A / d ** 0.25 + 0.3 * torch.randn(n, d, generator=g) / d ** 0.5).numpy().astype(np.float32)
    V0 = (0.6 * Bm / d ** 0.25 + 0.3 * torch.randn(m, d, generator=g) / d ** 0.5).numpy().astype(np.float32)
    model, _ = _model_from(U0, V0, dev, 1e-3, 0.0)
    Xd = X.to(dev).contiguous()
    res = S.compute_alpha_and_norm_ratios(model, Xd)
    ref = O.alpha_and_norm_ratios(U0, V0, X.numpy())
    names = ["alpha", "norm_X", "norm_ratio", "rec_scaled", "pearson_mean", "pearson_std", "spearman_mean",
             "spearman_std", "svd_err", "slopes", "correlations", "spearman_scores", "rec_scaled_per_row",
             "alpha_per_row"]
    assert len(res) == len(ref) == 14
    for nm, v, r in zip(names, res, ref):
        v, r = np.asarray(v, dtype=np.float64), np.asarray(r, dtype=np.float64)
        assert v.shape == r.shape, nm
        scale = max(1.0, float(np.max(np.abs(r))) if r.size else 1.0)
        np.testing.assert_allclose(v, r, rtol=0, atol=1e-4 * scale, err_msg=nm)
    assert 0.0 < res[8] < 1.0 and res[8] != 1.0          # the SVD branch ran (1.0 is the swallowed-failure value)


@pytest.mark.gpu
def test_x_spectrum_cache_is_tied_to_the_matrix_not_to_its_address(dev):
    """same-shape ground truths created one after the other (run_experiment's repetitions) tend to get the
    same device block back from the caching allocator; the spectrum cache must not hand X_1's singular values to X_2.
    Each svd_err is compared with the dense route on a fresh cache."""
    from mfcd import metrics
    n, m, d = 512, 384, 16
    g = torch.Generator().manual_seed(5)
    U = (torch.randn(n, d, generator=g) / d ** 0.5).to(dev)
    V = (torch.randn(m, d, generator=g) / d ** 0.5).to(dev)
    ok = np.ones(n, dtype=bool)
    seen_ptrs, got, want = [], [], []
    for rep in range(4):
        X = ((torch.randn(n, d, generator=g) @ torch.randn(d, m, generator=g)) * (0.2 + 0.1 * rep)).to(dev).contiguous()
        seen_ptrs.append(X.data_ptr())
        xm = X.mean(1)
        _, e_fast, failed = metrics.spearman_and_svd(U, V, xm, X, 0.8, ok)
        assert not failed
        got.append(e_fast)
        Xc = (X - xm[:, None]).double()
        s1 = torch.linalg.svdvals(Xc)
        Vc = (V - V.mean(0, keepdim=True)).double()
        s2 = torch.linalg.svdvals(U.double() @ Vc.t())
        k = min(len(s1), len(s2))
        want.append(float(torch.linalg.norm(0.8 * s2[:k] - s1[:k]) / (torch.linalg.norm(s1[:k]) + 1e-8)))
        del X, Xc
    assert len(set(seen_ptrs)) < len(seen_ptrs), "the allocator did not reuse a block: the test did not test anything"
    np.testing.assert_allclose(got, want, rtol=1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,m", [(6, 20449), (5, 32768), (4, 65536)])    # 65536 = BASELINE configs[3]'s item count
def test_spearman_rows_longer_than_the_lds_kernel_match_scipy(dev, rows, m):
    """Rows longer than mfcd_spearman_max_columns() (20448) take mfcd_spearman_rows_long (segmented device sort of row
    blocks in global memory, then the LDS kernel's own rank / exact-sum pass per row).  Same checks as the kernel's test:
    scipy.stats.spearmanr row by row, ties in one and in both operands, -0.0 / +0.0, a constant row (NaN); the plain-torch
    formulation (metrics.spearman_rows_sorted, off the product path) agrees too, and two calls are bit-equal."""
    from scipy.stats import spearmanr
    from mfcd import metrics
    rng = np.random.default_rng(m)
    A = rng.standard_normal((rows, m)).astype(np.float32)
    X = (0.6 * A + rng.standard_normal((rows, m))).astype(np.float32)
    X[1] = np.round(X[1] * 2.0) / 2.0
    A[2], X[2] = rng.integers(0, 5, m).astype(np.float32), rng.integers(0, 5, m).astype(np.float32)
    A[0, : m // 2] = 0.0
    A[0, 0] = -0.0
    X[3] = 1.25
    Ad, Xd = torch.from_numpy(A).to(dev), torch.from_numpy(X).to(dev)
    got = metrics.spearman_rows_any(Ad, Xd).cpu().numpy()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np.array([spearmanr(A[r], X[r]).correlation for r in range(rows)])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, equal_nan=True)
    assert np.isnan(got[3])
    assert np.array_equal(got, metrics.spearman_rows_long(Ad, Xd).cpu().numpy(), equal_nan=True)
    np.testing.assert_allclose(got, metrics.spearman_rows_sorted(Ad, Xd).cpu().numpy(), rtol=0, atol=1e-12, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,m", [(37, 1000), (9, 20000), (300, 4097)])
def test_long_row_spearman_path_equals_the_lds_kernel_bit_for_bit(dev, rows, m):
    """Where both apply (m <= 20448) the global-memory path must return the LDS kernel's value exactly: same keys, same
    run rule, same exact integer sums — including rows cut into several sort blocks, strided inputs, ties and NaN."""
    from mfcd import metrics
    rng = np.random.default_rng(rows + m)
    A = rng.standard_normal((rows, m + 5)).astype(np.float32)
    X = np.round(rng.standard_normal((rows, m)) * 3.0).astype(np.float32) / 3.0
    A[1, 7] = np.nan
    X[2] = -0.0
    Ad, Xd = torch.from_numpy(A).to(dev)[:, :m], torch.from_numpy(X).to(dev)
    a = metrics.spearman_rows(Ad, Xd).cpu().numpy()
    b = metrics.spearman_rows_long(Ad, Xd).cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True) and np.isnan(a[1]) and np.isnan(a[2]) and np.isfinite(a[0])


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1000, 20000, 30000])
def test_spearman_of_a_row_with_nan_is_nan_as_scipy(dev, m):
    """scipy.stats.spearmanr returns NaN when either operand holds a NaN (nan_policy='propagate'); both
    device paths (LDS kernel, long-row sort path) must do the same instead of ranking NaN as the largest value."""
    from mfcd import metrics
    rng = np.random.default_rng(m)
    A = rng.standard_normal((4, m)).astype(np.float32)
    X = rng.standard_normal((4, m)).astype(np.float32)
    A[1, m // 3] = np.nan
    X[2, m - 1] = np.nan
    got = metrics.spearman_rows_any(torch.from_numpy(A).to(dev), torch.from_numpy(X).to(dev)).cpu().numpy()
    assert np.isfinite(got[0]) and np.isfinite(got[3])
    assert np.isnan(got[1]) and np.isnan(got[2])


@pytest.mark.gpu
def test_bf16_tables_with_a_generic_optimiser_are_refused_or_widened_never_overrun(dev):
    """the dense-gradient kernel is fp32-only.  bf16 factor tables must never reach it as raw pointers
    (it would read and write twice the tables' size): the autograd route widens exactly and returns bf16 gradients
    that match the fp32 computation on the widened tables; fit_generic refuses bf16 up front."""
    import structure as S
    from mfcd import engine, _lib
    n, m, d, N = 50, 40, 16, 100
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=3)
    rec = _records(u, i, j, z, n, m, dev).dev
    Ub = torch.from_numpy(U0).to(dev).bfloat16()
    Vb = torch.from_numpy(V0).to(dev).bfloat16()
    g = torch.linspace(-1, 1, N, device=dev)
    guard = torch.full((n * d,), 7.0, device=dev)           # sits near the outputs in the allocator's pool
    gU, gV = engine.dense_grad_from_coefficients(Ub, Vb, rec, g)
    assert gU.dtype == torch.bfloat16 and gU.shape == Ub.shape and gV.shape == Vb.shape
    rU, rV = engine.dense_grad_from_coefficients(Ub.float(), Vb.float(), rec, g)
    assert torch.equal(gU, rU.bfloat16()) and torch.equal(gV, rV.bfloat16())
    assert bool((guard == 7.0).all())
    model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    rows = np.stack([u, i, j, z], 1)
    mk = lambda r: torch.utils.data.DataLoader(ListDataset(r), batch_size=64, shuffle=False)  # noqa: E731
    with pytest.raises(_lib.MfcdError):
        engine.fit_generic(model, mk(rows), mk(rows[:10]), opt, 1)


@pytest.mark.gpu
def test_row_block_sharded_uvt_pass_rehearsal_at_c5_shape(dev, orc):
    """SURVEY 8e G1 at BASELINE configs[4] (C5: 100000 x 20000, d = 256): the eight row blocks an 8-rank run would
    hold, each through mfcd_uvt_stats_slab, shares added in rank order, against the one-pass result (fp32-rounding
    level: per-tile sums group by each slab's own column split) and against the oracle on 128 sampled rows."""
    from mfcd import dist as mdist, metrics
    n, m, d, world = 100000, 20000, 256, 8
    g = torch.Generator(device=dev).manual_seed(4242)
    U = torch.randn(n, d, device=dev, generator=g) / d ** 0.5
    V = torch.randn(m, d, device=dev, generator=g) / d ** 0.5
    X = torch.empty(n, m, device=dev)
    for r0 in range(0, n, 8192):
        X[r0:r0 + 8192].normal_(0.1, 0.5, generator=g)
    rs_d, sc_d = metrics.uvt_stats(U, V, X, 0.9)
    cuts = [n * r // world for r in range(world + 1)]
    blocks, scal = [], torch.zeros(4, dtype=torch.float64, device=dev)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rs, share = mdist.hip_slab_pass(U, V, X[lo:hi], lo, 0.9, 3)
        blocks.append(rs)
        scal += share
    rs_s = torch.cat(blocks)
    for col in range(6):
        scale = float(rs_d[:, col].abs().max()) + 1e-30
        assert float((rs_s[:, col] - rs_d[:, col]).abs().max()) <= 2e-5 * scale, col
    np.testing.assert_allclose(scal[:2].cpu().numpy(), sc_d[:2].cpu().numpy(), rtol=2e-6)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(8))[:128].sort().values.to(dev)
    ref_rows, _, _ = orc.uvt_stats(U[rows].cpu().numpy(), V.cpu().numpy(), X[rows].cpu().numpy(), 0.9)
    got = rs_s[rows].cpu().numpy()
    np.testing.assert_allclose(got[:, 1], ref_rows[:, 1], rtol=2e-5)
    np.testing.assert_allclose(got[:, 2], ref_rows[:, 2], rtol=2e-5)


# Shapes of the staged-prologue tests: (n, m, d, samples per call).  The first is the one each test was written at; the
# other two are resident look-ahead calls, whose prologue IS staged (second set of prologue regions, claim_set,
# lists_dirty): 40 steps, whose step table travels in the prologue's kernel arguments, and 300 steps (> 223), whose
# table goes through a pinned slot.
STAGED_LOOKAHEAD = [(4096, 4096, 8, 64 * 40 + 17), (4096, 4096, 8, 64 * 300 + 5)]


def _assert_prologue_is_staged(n, m, d, N):
    from mfcd import engine
    assert engine.train_plan(N, 64, n, m, d)["resident_lookahead"] > 0   # the form whose prologue is staged


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,d,N", [(640, 512, 64, 64 * 150 + 17)] + STAGED_LOOKAHEAD)
def test_staged_prologue_gives_the_same_run(dev, monkeypatch, n, m, d, N):
    """engine.fit stages every epoch's prologue (sample translation, per-wave event lists) on a side stream under the
    previous epoch's step kernel (mfcd_train_call_stage, second set of prologue regions).  Same inputs to the same step
    kernel: the run must be BIT-identical to one whose prologues all run in-stream, epoch losses included, and the
    staged descriptor must not leak into a call on other samples."""
    from mfcd import engine
    U0, V0, u, i, j, z = _synthetic(n, m, d, N, seed=31)
    rows = np.stack([u, i, j, z], 1)
    mk = lambda r, sh: torch.utils.data.DataLoader(ListDataset(r), batch_size=64, shuffle=sh)   # noqa: E731
    engine.set_train_path("resident")
    try:
        if (n, m, d, N) in STAGED_LOOKAHEAD:
            _assert_prologue_is_staged(n, m, d, N)
        outs = []
        for staged in (True, False):
            if not staged:
                monkeypatch.setattr(engine, "stage_next_call", lambda *a, **k: False)
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            torch.manual_seed(7)
            tl, vl = engine.fit(model, mk(rows, True), mk(rows[:640], False), opt, 5)
            # a call on OTHER samples right after: must not pick up a staged prologue
            extra = engine.train_steps(engine.AdamBinding(model, opt), _records(u[:640], i[:640], j[:640], z[:640], n, m, dev).dev, 64)
            outs.append((tl, vl, model.U.data.clone(), model.V.data.clone(), extra.clone(),
                         opt.state[model.U]["exp_avg_sq"].clone()))
        engine.check_status()
    finally:
        engine.set_train_path("auto")
    a, b = outs
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,d,N", [(640, 512, 64, 64 * 150 + 17)] + STAGED_LOOKAHEAD)
def test_abandoned_staged_prologue_leaves_no_trace(dev, n, m, d, N):
    """A staged prologue whose call never comes (the caller went on with other samples, or with another step count)
    leaves its set's per-wave event lists filled: the next prologue into that set must start from empty lists, not
    append to them (train.hip: WsState::lists_dirty).  Stage A, abandon it, run B in-stream, stage C over A's set, run
    C: BIT-identical to the same two calls with nothing staged."""
    from mfcd import engine
    U0, V0, u, i, j, z = _synthetic(n, m, d, 3 * N, seed=33)
    recs = [_records(u[k * N:(k + 1) * N], i[k * N:(k + 1) * N], j[k * N:(k + 1) * N], z[k * N:(k + 1) * N], n, m, dev).dev
            for k in range(3)]
    side = torch.cuda.Stream(device=dev)
    engine.set_train_path("resident")
    try:
        if (n, m, d, N) in STAGED_LOOKAHEAD:
            _assert_prologue_is_staged(n, m, d, N)
        outs = []
        for staged in (True, False):
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            bind = engine.AdamBinding(model, opt)
            nb = (N + 63) // 64
            loss = [torch.empty(nb, device=dev) for _ in range(3)]
            engine.train_steps(bind, recs[1], 64, loss_out=loss[1])          # makes the prepared call
            torch.cuda.synchronize()
            if staged:
                assert engine.stage_next_call(bind, recs[0], 64, loss[0], side)      # A: never run
                torch.cuda.synchronize()
            engine.train_steps(bind, recs[1], 64, loss_out=loss[1])          # B, in-stream
            torch.cuda.synchronize()
            if staged:
                assert engine.stage_next_call(bind, recs[2], 64, loss[2], side)      # C over A's set
                torch.cuda.synchronize()
            engine.train_steps(bind, recs[2], 64, loss_out=loss[2])
            torch.cuda.synchronize()
            outs.append((model.U.data.clone(), model.V.data.clone(), loss[1].clone(), loss[2].clone()))
        engine.check_status()
    finally:
        engine.set_train_path("auto")
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,d,N", [(4096, 4096, 64, 64 * 150 + 17)] + STAGED_LOOKAHEAD)
def test_staged_prologue_follows_a_changed_learning_rate(dev, n, m, d, N):
    """A staged prologue's step table holds the step scalars of the lr / betas current when it was staged.  A caller
    that changes the learning rate between staging and the call (a schedule writing param_groups) gets a new prepared
    call; that call must build its own prologue, not take the staged table: stage at lr = a, switch to lr = b, run:
    BIT-identical to the same call run unstaged at lr = b, losses and both moments included."""
    from mfcd import engine
    U0, V0, u, i, j, z = _synthetic(n, m, d, 2 * N, seed=35)
    recs = [_records(u[k * N:(k + 1) * N], i[k * N:(k + 1) * N], j[k * N:(k + 1) * N], z[k * N:(k + 1) * N], n, m, dev).dev
            for k in range(2)]
    side = torch.cuda.Stream(device=dev)
    engine.set_train_path("resident")
    try:
        _assert_prologue_is_staged(n, m, d, N)
        outs = []
        for staged in (True, False):
            model, opt = _model_from(U0, V0, dev, 1e-3, 1e-5)
            bind = engine.AdamBinding(model, opt)
            nb = (N + 63) // 64
            loss = [torch.empty(nb, device=dev) for _ in range(2)]
            engine.train_steps(bind, recs[0], 64, loss_out=loss[0])          # makes the prepared call at lr = a
            torch.cuda.synchronize()
            if staged:
                assert engine.stage_next_call(bind, recs[1], 64, loss[1], side)      # step table built at lr = a
                torch.cuda.synchronize()
            opt.param_groups[0]["lr"] = 3e-3                                     # lr = b
            engine.train_steps(bind, recs[1], 64, loss_out=loss[1])
            torch.cuda.synchronize()
            st = [opt.state[p][k].clone() for p in (model.U, model.V) for k in ("exp_avg", "exp_avg_sq")]
            outs.append([loss[1].clone(), model.U.data.clone(), model.V.data.clone()] + st)
        engine.check_status()
    finally:
        engine.set_train_path("auto")
    for x, y in zip(*outs):
        assert torch.equal(x, y)
