"""GPU tests of evaluation (csrc/eval.hip) and of the split step kernels (csrc/streaming.hip: coefficients, dense gradient,
Adam from a dense gradient, the step from given coefficients) against the f64 stage models of tests/step_model.py,
element by element under the bounds derived there ((E), (K), (DG), (AD), (AS)), and of the bit-identities the code
promises between these entries and the fused streaming step.

(a) Every entry is called on the inputs step_model builds (tests/test_step_parts_cpu.py holds the numpy emulation and the
    C oracle to the same bounds on the same inputs): through mfcd.engine where it has a wrapper, through mfcd._lib with
    torch tensors otherwise.  No excluded elements; a zero bound demands the exact value.
(b) Shapes: both access widths of make_plan (d % 4, misaligned views), its chunk counts 1, 2, 4, partial last blocks,
    the U / V seam, rows that span workgroups, batches of 1 .. 16384 samples (evaluation's documented maximum: 128 KiB
    of dynamic LDS), short last batches, null outputs.
(c) Identities, asserted bit for bit: see the tests named test_identity_*.
(d) `pytest -s` prints the largest error / bound per part and output at the end (profiles/step_parts_accuracy.txt is one
    such run).  A call that fails ends the session: nothing more is started on the device."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import step_model as M
from test_step import _binding, _read, forced

pytestmark = pytest.mark.gpu

RATIOS = {}          # (part, variant) -> {output: largest ratio}
MFCD_EWORKSPACE = -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    if RATIOS:
        print("\nlargest error / bound per part and output (correct: 0 = the one admissible count, 1 = an end of the interval)")
        for (part, variant), r in sorted(RATIOS.items()):
            print(f"  {part:15s} {variant:12s} " + " ".join(f"{k} {v:8.2e}" for k, v in sorted(r.items())))


@contextlib.contextmanager
def device_calls(label):
    """The calls of one case and the wait for them: a failed launch or a device fault ends the session."""
    try:
        yield
        torch.cuda.synchronize()
    except AssertionError:
        raise
    except Exception as e:
        pytest.exit(f"{label}: the call itself failed, stopping the session: {type(e).__name__}: {e}", returncode=3)


def _hold(part, variant, label, ratios, got=None, mdl=None, bnd=None):
    """Record the ratios and assert that every one is at most 1."""
    f = RATIOS.setdefault((part, variant), {})
    for k, r in ratios.items():
        v = float(np.max(r)) if np.size(r) else 0.0
        f[k] = max(f.get(k, 0.0), v if np.isfinite(v) else 9.99e99)
    for k, r in ratios.items():
        if np.size(r) and not float(np.max(r)) <= 1.0:
            where = np.argwhere(np.asarray(r) > 1.0)[:4].tolist()
            detail = [(e, float(np.asarray(got[k])[tuple(e)]), float(np.asarray(mdl[k])[tuple(e)]),
                       float(np.asarray(bnd[k])[tuple(e)])) for e in where] if got is not None else where
            raise AssertionError((part, variant, label, k, float(np.max(r)), detail))


def _t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _rec(data, n, m, dev, s=slice(None)):
    from mfcd import engine
    return engine.records_from_indices(data["u"][s], data["i"][s], data["j"][s], n, m, dev, data["z"][s])


def _rec_batch(batch, n, m, dev):
    from mfcd import engine
    return engine.records_from_indices(batch[0], batch[1], batch[2], n, m, dev, batch[3])


def _misaligned(a, dev):
    """A contiguous device copy of `a` that starts one float into a larger buffer (4-byte, not 16-byte aligned)."""
    buf = torch.empty(a.size + 5, dtype=torch.float32, device=dev)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _state_dev(st, dev, misaligned=False):
    return {k: (_misaligned(st[k], dev) if misaligned else _t(st[k], dev)) for k in M.TABLES}


def _state_np(sd):
    return {k: sd[k].cpu().numpy() for k in M.TABLES}


# ---- raw entries (mfcd._lib, as mfcd/dist.py calls them) -------------------------------------------------------------
def _eval_raw(U, V, rec, B, want):
    """mfcd_eval_batches(_bf16) with correct_per_batch and p_out present or both null -> (loss, correct, p)."""
    from mfcd import _lib
    L = _lib.load()
    (n, d), m, N = U.shape, V.shape[0], rec.shape[0]
    nb = (N + B - 1) // B
    loss = torch.empty(max(nb, 1), dtype=torch.float32, device=U.device)
    corr = torch.empty(max(nb, 1), dtype=torch.int32, device=U.device) if want else None
    p = torch.empty(max(N, 1), dtype=torch.float32, device=U.device) if want else None
    fn = L.mfcd_eval_batches_bf16 if U.dtype == torch.bfloat16 else L.mfcd_eval_batches
    _lib.check(fn(_lib.ptr(U), _lib.ptr(V), _lib.ptr(rec), N, B, n, m, d, _lib.ptr(loss), _lib.ptr(corr), _lib.ptr(p),
                  _lib.stream_ptr(U.device)))
    return loss[:nb], corr, p


def _coefficients(U, V, rec, divisor, want=(True, True, True)):
    from mfcd import _lib
    L = _lib.load()
    (n, d), m, B = U.shape, V.shape[0], rec.shape[0]
    outs = [torch.full((max(B, 1),), -7.0, dtype=torch.float32, device=U.device) if w else None for w in want]
    _lib.check(L.mfcd_batch_coefficients(_lib.ptr(U), _lib.ptr(V), _lib.ptr(rec), B, n, m, d, divisor,
                                         *[_lib.ptr(o) for o in outs], _lib.stream_ptr(U.device)))
    return [o[:B] if o is not None else None for o in outs]


def _dense_grad(U, V, rec, divisor, gU=None, gV=None):
    from mfcd import _lib
    L = _lib.load()
    (n, d), m, B = U.shape, V.shape[0], rec.shape[0]
    gU = torch.full_like(U, 3.0) if gU is None else gU
    gV = torch.full_like(V, 3.0) if gV is None else gV
    term = torch.full((max(B, 1),), -7.0, dtype=torch.float32, device=U.device)
    _lib.check(L.mfcd_dense_grad(_lib.ptr(U), _lib.ptr(V), _lib.ptr(rec), B, n, m, d, divisor, _lib.ptr(gU), _lib.ptr(gV),
                                 _lib.ptr(term), _lib.stream_ptr(U.device)))
    return gU, gV, term[:B]


def _adam_dense(sd, gU, gV, step, h):
    from mfcd import _lib
    L = _lib.load()
    (n, d), m = sd["U"].shape, sd["V"].shape[0]
    _lib.check(L.mfcd_adam_dense(*[_lib.ptr(sd[k]) for k in M.TABLES], _lib.ptr(gU), _lib.ptr(gV), step, n, m, d, h["lr"],
                                 h["beta1"], h["beta2"], h["eps"], h["wd"], _lib.stream_ptr(gU.device)))


def apply_bytes(B, n, m, d):
    """streaming.hip streaming_bytes: the scratch mfcd_apply_step needs."""
    al = lambda x: (x + 255) & ~255          # noqa: E731
    return 256 + al(4 * n * d) + al(4 * m * d) + al(4 * max(B, 1))


def _apply_step(sd, rec, g, step, h, ws=None, nbytes=None):
    """-> the entry's return code (0 = ok)."""
    from mfcd import _lib
    L = _lib.load()
    (n, d), m, B = sd["U"].shape, sd["V"].shape[0], (rec.shape[0] if rec is not None else 0)
    nbytes = apply_bytes(B, n, m, d) if nbytes is None else nbytes
    ws = torch.empty(apply_bytes(B, n, m, d), dtype=torch.uint8, device=sd["U"].device) if ws is None else ws
    return L.mfcd_apply_step(*[_lib.ptr(sd[k]) for k in M.TABLES], _lib.ptr(rec), _lib.ptr(g), B, step, n, m, d, h["lr"],
                             h["beta1"], h["beta2"], h["eps"], h["wd"], _lib.ptr(ws), nbytes, _lib.stream_ptr(sd["U"].device))


def _fused_streaming_step(st, start, h, batch, bf16, dev):
    """One fused streaming step (engine.train_steps) from the state st -> (tables after, loss)."""
    from mfcd import engine
    n, m = st["U"].shape[0], st["V"].shape[0]
    with forced("streaming", "ieee"):
        model, opt, binding = _binding(st, start, h, bf16, dev)
        rec = _rec_batch(batch, n, m, dev)
        plan = engine.train_plan(len(batch[0]), len(batch[0]), n, m, st["U"].shape[1], bf16)
        assert plan["form_name"] == "streaming", plan
        loss = engine.train_steps(binding, rec, len(batch[0])).cpu().numpy()
        out = _read(model, opt)
    return out, loss


# ---- evaluation ------------------------------------------------------------------------------------------------------
def _eval_one(dev, d, N, B, fam, bf16):
    from mfcd import engine
    n, m = M.EVAL_ROWS[d]
    data = M.eval_input(d, N, B, fam, bf16)
    mdl, bnd = M.eval_model(data["U"], data["V"], data, B)
    tdt = torch.bfloat16 if bf16 else torch.float32
    U, V, rec = _t(data["U"], dev, tdt), _t(data["V"], dev, tdt), _rec(data, n, m, dev)
    label = f"eval d{d} N{N} B{B} {fam} {'bf16' if bf16 else 'f32'}"
    with device_calls(label):
        loss, corr, p = engine.eval_batches(U, V, rec, B, want_p=True)
        loss0, _, _ = _eval_raw(U, V, rec, B, want=False)
    got = dict(loss=loss.cpu().numpy(), correct=corr.cpu().numpy(), p=p.cpu().numpy())
    assert got["loss"].shape == mdl["loss"].shape and got["p"].shape == (N,)
    _hold("eval", ("bf16 " if bf16 else "f32 ") + fam, label, M.eval_check(got, mdl, bnd), got, mdl, bnd)
    assert np.array_equal(loss0.cpu().numpy(), got["loss"]), label      # the null outputs change nothing
    assert (got["p"][mdl["zero"]] == 0.5).all(), label
    return got


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", M.EVAL_D)
def test_evaluation_holds_the_model(dev, d, bf16):
    for dd, N, B, fam in M.eval_cases():
        if dd == d:
            _eval_one(dev, d, N, B, fam, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,B", M.EVAL_NB_BIG)
def test_evaluation_at_the_largest_batches(dev, N, B, bf16):
    """B = 8192 and the documented maximum B = 16384: 64 and 128 KiB of dynamic LDS."""
    for fam in M.EVAL_FAMILIES:
        _eval_one(dev, 8, N, B, fam, bf16)


def test_evaluation_of_several_models_in_one_launch_equals_each_alone(dev):
    """mfcd_eval_batches_multi: five models of different (n, m, d, N, B), one with N = 0 in the middle, one with a single
    short batch, one with B = 16384, and the first listed twice: loss_per_batch and correct_per_batch of every entry
    are bit-equal to the model's own mfcd_eval_batches call."""
    from mfcd import _lib, engine
    L = _lib.load()
    specs = [(2, 17, 16, "soft"), (3, 0, 64, "uniform"), (64, 5, 64, "half"), (8, 16384 + 7, 16384, "uniform"),
             (256, 64 * 9 + 5, 64, "saturated")]
    specs.append(specs[0])
    tab = np.zeros(len(specs), dtype=engine._numpy_mirror(_lib.EvalModel))
    keep, outs, alone = [], [], []
    with device_calls("eval multi"):
        for r, (d, N, B, fam) in enumerate(specs):
            n, m = M.EVAL_ROWS[d]
            data = M.eval_input(d, max(N, 1), B, fam)
            U, V = _t(data["U"], dev), _t(data["V"], dev)
            rec = _rec(data, n, m, dev)[:N].contiguous()
            nb = (N + B - 1) // B
            loss = torch.full((max(nb, 1),), -7.0, dtype=torch.float32, device=dev)
            corr = torch.full((max(nb, 1),), -7, dtype=torch.int32, device=dev)
            keep.append((U, V, rec))
            outs.append((loss, corr, nb))
            alone.append(engine.eval_batches(U, V, rec, B) if N else None)
            tab[r] = (U.data_ptr(), V.data_ptr(), rec.data_ptr() if N else 0, N, B, n, m, d, loss.data_ptr(), corr.data_ptr())
        stage = ctypes.c_size_t(0)
        ws = engine._multi_workspace(L, L.mfcd_eval_multi_workspace_bytes(len(specs), ctypes.byref(stage)), stage.value, dev)
        _lib.check(L.mfcd_eval_batches_multi(tab.ctypes.data, len(specs), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    for (loss, corr, nb), ref, spec in zip(outs, alone, specs):
        if ref is None:
            assert float(loss[0]) == -7.0 and int(corr[0]) == -7
            continue
        assert np.array_equal(loss[:nb].cpu().numpy(), ref[0].cpu().numpy()), spec
        assert np.array_equal(corr[:nb].cpu().numpy(), ref[1].cpu().numpy()), spec
    L.mfcd_train_workspace_release(ws.data_ptr())


# ---- coefficients ----------------------------------------------------------------------------------------------------
def test_coefficients_hold_the_model(dev):
    for d, B, div, fam, want in M.coef_cases():
        data = M.part_family(fam, 50, 40, d, B, B)
        batch = M.batch_of(data, B, 0)
        mdl, bnd = M.coef_model(data["U"], data["V"], batch, div)
        label = f"coef d{d} B{B} div{div} {fam} {want}"
        with device_calls(label):
            g, term, p = _coefficients(_t(data["U"], dev), _t(data["V"], dev), _rec(data, 50, 40, dev), div, want)
        got = {k: (v.cpu().numpy() if v is not None else None) for k, v in (("g", g), ("term", term), ("p", p))}
        assert [v is not None for v in (g, term, p)] == list(want)
        _hold("coef", fam, label, M._ratios(got, mdl, bnd, ("g", "term", "p")), got, mdl, bnd)


# ---- dense gradient --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["dense_grad", "grad_from_coef"])
def test_dense_gradient_holds_the_model(dev, entry):
    from mfcd import engine
    for case in M.grad_cases():
        label, n, m, d, B, fam, seed = case
        data = M.grad_input(case)
        batch = M.batch_of(data, B, 0)
        U, V, rec = _t(data["U"], dev), _t(data["V"], dev), _rec_batch(batch, n, m, dev)
        with device_calls(f"{entry} {label}"):
            if entry == "dense_grad":
                mdl, bnd = M.grad_model(data["U"], data["V"], batch, divisor=B)
                gU, gV, term = _dense_grad(U, V, rec, B)
                got = dict(gradU=gU.cpu().numpy(), gradV=gV.cpu().numpy(), term=term.cpu().numpy())
            else:
                g = M.signed_coefficients(B)
                mdl, bnd = M.grad_model(data["U"], data["V"], batch, g=g)
                gU, gV = engine.dense_grad_from_coefficients(U, V, rec, _t(g, dev))
                got = dict(gradU=gU.cpu().numpy(), gradV=gV.cpu().numpy())
        _hold(entry, fam, label, M._ratios(got, mdl, bnd, ("gradU", "gradV", "term")), got, mdl, bnd)


# ---- Adam from a dense gradient --------------------------------------------------------------------------------------
ADAM = M.adam_cases()


@pytest.mark.parametrize("case", ADAM, ids=[c[0] for c in ADAM])
def test_adam_from_a_dense_gradient_holds_the_model(dev, case):
    label, n, m, d, start, h, aligned = case
    st, gU, gV, step, special = M.adam_input(case)
    mdl, bnd = M.adam_model(st, gU, gV, h, step)
    sd = _state_dev(st, dev, misaligned=not aligned)
    with device_calls(f"adam_dense {label}"):
        _adam_dense(sd, _t(gU, dev), _t(gV, dev), step, h)
    got = _state_np(sd)
    _hold("adam_dense", f"v{M.plan(n, m, d, aligned)[0]}c{M.plan(n, m, d, aligned)[1]}", label,
          M.check_tables(got, mdl, bnd), got, mdl, bnd)
    for T, g in (("U", gU), ("V", gV)):          # the non-finite gradient elements: exactly these elements are not finite
        bad = ~np.isfinite(g)
        assert bad.sum() >= 1 and np.array_equal(~np.isfinite(got[T]), bad) and np.array_equal(~np.isfinite(got["m" + T]), bad)
        assert np.isnan(got[T][bad]).all() and np.isnan(got["m" + T][np.isnan(g)]).all()
    if h["lr"] == 0.0:                            # every parameter keeps its bits while the moments move
        fin = np.isfinite(gU)
        assert np.array_equal(got["U"][fin], st["U"][fin]) and np.array_equal(got["V"][np.isfinite(gV)], st["V"][np.isfinite(gV)])
        assert not np.array_equal(got["mU"][fin], st["mU"][fin]) and not np.array_equal(got["vU"][fin], st["vU"][fin])


# ---- the step from given coefficients --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.STREAMING, ids=[c["label"] for c in M.STREAMING])
def test_apply_step_holds_the_model(dev, case):
    h, n, m = case["hyper"], case["n"], case["m"]
    data, st, step = M.case_inputs(case)
    for k in (0, case["steps"] - 1):              # a full batch and the last one (short where the case has one)
        batch = M.batch_of(data, case["B"], k)
        rec = _rec_batch(batch, n, m, dev)
        g_model = M.coef_model(st["U"], st["V"], batch, len(batch[0]))[0]["g"].astype(np.float32)
        with device_calls(f"apply_step {case['label']}"):
            g_kernel = _coefficients(_t(st["U"], dev), _t(st["V"], dev), rec, len(batch[0]), (True, False, False))[0].cpu().numpy()
        for src, g in (("model g", g_model), ("kernel g", g_kernel)):
            mdl, bnd = M.apply_model(st, batch, g, h, step)
            sd = _state_dev(st, dev)
            with device_calls(f"apply_step {case['label']} {src}"):
                assert _apply_step(sd, rec, _t(g, dev), step, h) == 0
            got = _state_np(sd)
            _hold("apply_step", src, f"{case['label']} batch {k}", M.check_tables(got, mdl, bnd), got, mdl, bnd)


def test_apply_step_workspace_check_and_empty_batch(dev):
    case = M.STREAMING[0]
    h, n, m, d = case["hyper"], case["n"], case["m"], case["d"]
    data, st, step = M.case_inputs(case)
    batch = M.batch_of(data, case["B"], 0)
    rec, g = _rec_batch(batch, n, m, dev), _t(M.signed_coefficients(len(batch[0])), dev)
    need = apply_bytes(len(batch[0]), n, m, d)
    sd = _state_dev(st, dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    with device_calls("apply_step, workspace one byte short"):
        assert _apply_step(sd, rec, g, step, h, ws, need - 1) == MFCD_EWORKSPACE
    assert all(np.array_equal(_state_np(sd)[k], st[k]) for k in M.TABLES) and int(ws.max()) == 0
    with device_calls("apply_step, exact workspace"):
        assert _apply_step(sd, rec, g, step, h, ws, need) == 0
    assert not np.array_equal(_state_np(sd)["U"], st["U"])
    # B = 0: a pure weight-decay / moment step
    empty = tuple(np.zeros(0, np.int64) for _ in range(3)) + (np.zeros(0, np.float32),)
    mdl, bnd = M.apply_model(st, empty, np.zeros(0, np.float32), h, step)
    sd = _state_dev(st, dev)
    with device_calls("apply_step, B = 0"):
        assert _apply_step(sd, None, None, step, h) == 0
    got = _state_np(sd)
    _hold("apply_step", "B = 0", case["label"], M.check_tables(got, mdl, bnd), got, mdl, bnd)
    assert not np.array_equal(got["U"], st["U"]) and not np.array_equal(got["mV"], st["mV"])


# ---- sample validation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 255, 257, 2048 * 256 + 777])
def test_check_samples_counts_exactly(dev, N):
    """mfcd_check_samples: each way to be out of range, one in the last record, several bad fields in one record counted
    once, and the all-valid case; N = 2048 * 256 + 777 is past the grid (2048 blocks of 256): the stride loop runs."""
    from mfcd import _lib
    L = _lib.load()
    n, m = 37, 23
    rng = np.random.default_rng([17, N])
    rec = np.stack([rng.integers(0, n, N), rng.integers(0, m, N), rng.integers(0, m, N), np.zeros(N, np.int64)], axis=1).astype(np.int32)
    bad_dev = torch.full((1,), -1, dtype=torch.int32, device=dev)

    def count(r):
        t = torch.from_numpy(r).to(dev) if len(r) else None
        with device_calls(f"check_samples N = {N}"):
            _lib.check(L.mfcd_check_samples(_lib.ptr(t), len(r), n, m, _lib.ptr(bad_dev), _lib.stream_ptr(dev)))
            return int(bad_dev.item())

    assert count(rec) == 0
    if N == 0:
        return
    ways = [(0, -1), (0, n), (1, -1), (1, m), (2, -1), (2, m)]
    for col, val in ways:                          # one bad field, in the last record
        r = rec.copy()
        r[N - 1, col] = val
        assert count(r) == 1, (col, val)
    r = rec.copy()
    r[N - 1] = (-5, m + 3, -1, 0)                  # three bad fields in one record: counted once
    assert count(r) == 1
    if N >= 255:
        r = rec.copy()
        pos = rng.choice(N, size=min(N, 101), replace=False)
        for k, t in enumerate(pos):
            col, val = ways[k % 6]
            r[t, col] = val
            if k % 7 == 0:
                r[t, (col + 1) % 3] = -1
        r[0, 0], r[N - 1, 2] = n, m
        assert count(r) == len(set(pos.tolist()) | {0, N - 1})


# ---- identities the code promises ------------------------------------------------------------------------------------
IDENT = [c for c in M.STREAMING if c["label"] in ("d5", "d100", "d256", "B200", "2x3x8", "sat", "multi_wg", "fuzz")]


@pytest.mark.parametrize("case", IDENT, ids=[c["label"] for c in IDENT])
def test_identity_1_p_of_evaluation_equals_p_of_the_coefficient_kernel(dev, case):
    """Both are sigmoid_f32(wave_score(..)) of the same rows (eval.hip, streaming.hip coeff_kernel)."""
    from mfcd import engine
    data, st, _ = M.case_inputs(case)
    U, V, rec = _t(st["U"], dev), _t(st["V"], dev), _rec(data, case["n"], case["m"], dev)
    with device_calls(f"identity 1 {case['label']}"):
        p_eval = engine.eval_batches(U, V, rec, case["B"], want_p=True)[2].cpu().numpy()
        p_coef = _coefficients(U, V, rec, case["B"], (False, False, True))[2].cpu().numpy()
    assert np.array_equal(p_eval, p_coef)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", IDENT, ids=[c["label"] for c in IDENT])
def test_identity_2_evaluation_loss_before_a_step_equals_the_steps_loss(dev, case, bf16):
    """loss_per_batch[k] of evaluation on the state before step k == the loss the one-step streaming call reports for
    batch k: the same terms summed by a wave in the same order (eval.hip, streaming.hip batch_mean_kernel)."""
    from mfcd import engine
    h, B, n, m = case["hyper"], case["B"], case["n"], case["m"]
    data, st0, _ = M.case_inputs(case, bf16)
    rec = _rec(data, n, m, dev)
    with forced("streaming", "ieee"):
        model, opt, binding = _binding(st0, case["start"], h, bf16, dev)
        for k in range(case["steps"]):
            s = slice(k * B, min((k + 1) * B, case["N"]))
            with device_calls(f"identity 2 {case['label']} step {k}"):
                before = engine.eval_batches(model.U.data, model.V.data, rec[s], B)[0].cpu().numpy()
                loss = engine.train_steps(binding, rec[s], B).cpu().numpy()
            assert before.shape == loss.shape == (1,) and np.array_equal(before, loss), (k, before, loss)
    assert case["N"] % B == 0 or s.stop - s.start < B


@pytest.mark.parametrize("case", IDENT, ids=[c["label"] for c in IDENT])
def test_identity_3_and_4_split_forms_equal_the_fused_step(dev, case):
    """(3) mfcd_batch_coefficients(divisor = b) + mfcd_apply_step == one fused streaming step, all six tables.
    (4) mfcd_dense_grad(divisor = b) + mfcd_adam_dense == the same step, and mfcd_dense_grad_from_coefficients fed the
    g_out of (3) == mfcd_dense_grad.  Full first batch and the last (short) batch of the case."""
    from mfcd import engine
    h, n, m = case["hyper"], case["n"], case["m"]
    data, st, step = M.case_inputs(case)
    for k in (0, case["steps"] - 1):
        batch = M.batch_of(data, case["B"], k)
        b = len(batch[0])
        fused, fused_loss = _fused_streaming_step(st, case["start"], h, batch, False, dev)
        rec = _rec_batch(batch, n, m, dev)
        with device_calls(f"identity 3/4 {case['label']} batch {k}"):
            U, V = _t(st["U"], dev), _t(st["V"], dev)
            g, term, _ = _coefficients(U, V, rec, b)
            s3 = _state_dev(st, dev)
            assert _apply_step(s3, rec, g, step, h) == 0
            gU, gV, term4 = _dense_grad(U, V, rec, b)
            gU2, gV2 = engine.dense_grad_from_coefficients(U, V, rec, g)
            s4 = _state_dev(st, dev)
            _adam_dense(s4, gU, gV, step, h)
        s3, s4 = _state_np(s3), _state_np(s4)
        for name in M.TABLES:
            assert np.array_equal(s3[name], fused[name]), ("coefficients + apply_step", case["label"], k, name)
            assert np.array_equal(s4[name], fused[name]), ("dense_grad + adam_dense", case["label"], k, name)
        assert torch.equal(gU, gU2) and torch.equal(gV, gV2)
        # every sample's term is recorded by the workgroup that owns the head of its U row: the two entries agree
        assert torch.equal(term, term4)


def test_identity_5_misaligned_views_equal_the_aligned_run(dev):
    """mfcd_adam_dense and mfcd_dense_grad on tables that start one float into a buffer take the scalar path of make_plan
    at d = 64; element for element the arithmetic is the same, so the results equal the aligned (vector) run's."""
    case = next(c for c in ADAM if c[0] == "misaligned")
    label, n, m, d, start, h, aligned = case
    st, gU, gV, step, _ = M.adam_input(case)
    a, b = _state_dev(st, dev), _state_dev(st, dev, misaligned=True)
    with device_calls("identity 5, adam_dense"):
        _adam_dense(a, _t(gU, dev), _t(gV, dev), step, h)
        _adam_dense(b, _misaligned(gU, dev), _misaligned(gV, dev), step, h)
    a, b = _state_np(a), _state_np(b)
    for name in M.TABLES:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    data = M.part_family("ij_cross", n, m, d, 32, 32)
    rec = _rec(data, n, m, dev)
    with device_calls("identity 5, dense_grad"):
        ga = _dense_grad(_t(data["U"], dev), _t(data["V"], dev), rec, 32)
        gb = _dense_grad(_misaligned(data["U"], dev), _misaligned(data["V"], dev), rec, 32,
                         _misaligned(np.full((n, d), 3.0, np.float32), dev), _misaligned(np.full((m, d), 3.0, np.float32), dev))
    assert all(torch.equal(x, y) for x, y in zip(ga, gb)) and float(ga[0].abs().max()) > 0.0
