"""GPU tests of the fused optimiser step (include/mfcd.h: mfcd_train_steps, _bf16, _big through mfcd.engine) against the
plain f64 model of tests/step_model.py, element by element under the bounds derived there.

(a) Resynchronised chains.  Every case of step_model.CASES is run as calls of exactly ONE step; before each call the
    kernel's own U, V and moments are read back, the model is evaluated from exactly that state, and all six tables and
    the loss are held to the bounds.  No propagation analysis and no excluded elements: an ill-conditioned element (the
    sparse gradient nearly cancels wd P) has a large bound, every other one a bound of a few 1e-6 lr.  Forms and
    flavours are forced in turn: streaming; resident fast / ieee; local fast / ieee; big fast / ieee (engine.
    set_big_resident("force")); fp32 and bf16 tables where the form has them.  Chains start fresh, from preset moments
    at step 500, and at step 10^6 (optimizer.state filled before AdamBinding is made).
(b) Split invariance.  On the collision-heavy small shapes one call of k steps is bit-identical to k calls of one step
    (tables, moments, losses), k odd, beyond two look-ahead windows, with a short last batch: this carries (a) to
    multi-step calls, where the resident forms' wave-to-wave hand-offs live.
(c) Shapes (step_model.CASES): the smallest that reach each path; the resident cases name the slice size Q they are
    meant for and engine.train_plan must agree, so that every (Q, d) pair of resident_inst.hip a plan can pick on this
    chip is met; both the look-ahead and the generic instantiation occur.
(d) `pytest -s` prints the largest error / bound per form, flavour, family and output at the end
    (profiles/step_accuracy.txt is one such run)."""
import contextlib

import numpy as np
import pytest
import torch

import step_model as M

pytestmark = pytest.mark.gpu

RATIOS = {}          # (form, flavour, tables, family) -> [7] largest ratio per output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    if RATIOS:
        print("\n(bf16 U, V: 0 = the one admissible value, 1 = an end of the admissible interval)")
        print("largest error / bound per form, flavour, tables and family: " + " ".join(f"{k:>8s}" for k in M.OUTPUTS))
        for key, r in sorted(RATIOS.items()):
            print("  {:9s} {:4s} {:4s} {:10s}                       ".format(*key) + " ".join(f"{v:8.2e}" for v in r))


@contextlib.contextmanager
def forced(form, flavour):
    from mfcd import engine
    try:
        engine.set_big_resident("force" if form == "big" else "off")
        engine.set_train_path("auto" if form == "big" else form)
        engine.set_resident_math(flavour)
        yield
    finally:
        engine.set_train_path("auto")
        engine.set_resident_math("fast")
        engine.set_big_resident("auto")


def _binding(st, start, h, bf16, dev):
    """A model, a torch.optim.Adam and the engine's binding around the state `st` (moments preset when start > 0)."""
    import structure as S
    from mfcd import engine
    n, d = st["U"].shape
    m = st["V"].shape[0]
    model = S.MatrixFactorization(n, m, d, dtype=torch.bfloat16) if bf16 else S.MatrixFactorization(n, m, d)
    with torch.no_grad():
        model.U.copy_(torch.from_numpy(st["U"]))
        model.V.copy_(torch.from_numpy(st["V"]))
    model = model.to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"])
    if start:
        for p, T in ((model.U, "U"), (model.V, "V")):
            opt.state[p] = {"step": torch.tensor(float(start)), "exp_avg": torch.from_numpy(st["m" + T]).to(dev),
                            "exp_avg_sq": torch.from_numpy(st["v" + T]).to(dev)}
    binding = engine.AdamBinding(model, opt)
    assert binding.step == start
    return model, opt, binding


def _read(model, opt):
    out = {"U": model.U.data.float().cpu().numpy(), "V": model.V.data.float().cpu().numpy()}
    for p, T in ((model.U, "U"), (model.V, "V")):
        out["m" + T] = opt.state[p]["exp_avg"].cpu().numpy()
        out["v" + T] = opt.state[p]["exp_avg_sq"].cpu().numpy()
    return out


def _call(binding, rec, B, form, case, bf16):
    """One engine.train_steps call that must take `form` -> losses (numpy)."""
    from mfcd import engine
    N = rec.shape[0]
    if form == "big":
        assert engine._big_for(binding, N, B, rec) is not None, "the big form refused the call"
    else:
        plan = engine.train_plan(N, B, case["n"], case["m"], case["d"], bf16)
        assert plan["form_name"] == form, (form, plan)
        if form == "resident":
            assert plan["resident_q"] == case["Q"], (case["label"], plan)
    try:
        loss = engine.train_steps(binding, rec, B).cpu().numpy()
        if form != "streaming":
            engine.check_status()
    except Exception as e:      # a failed launch, a device fault, an expired wait: nothing more is started on the device
        pytest.exit(f"{M.case_id(case)}: the call itself failed, stopping the session: {type(e).__name__}: {e}", returncode=3)
    return loss


CHAINS = [(c, fl, bf) for c in M.CASES for fl, bf in c["combos"]]


@pytest.mark.parametrize("case,flavour,bf16", CHAINS,
                         ids=[f"{M.case_id(c)}-{fl}-{'bf16' if bf else 'f32'}" for c, fl, bf in CHAINS])
def test_one_step_calls_hold_the_model_from_the_kernels_own_state(dev, case, flavour, bf16):
    from mfcd import engine
    form, h, B = case["form"], case["hyper"], case["B"]
    data, st0, step0 = M.case_inputs(case, bf16)
    rec = engine.records_from_indices(data["u"], data["i"], data["j"], case["n"], case["m"], dev, data["z"])
    key = (form, flavour, "bf16" if bf16 else "f32", case["family"])
    with forced(form, flavour):
        model, opt, binding = _binding(st0, case["start"], h, bf16, dev)
        for k in range(case["steps"]):
            st = _read(model, opt)
            if k == 0:
                assert all(np.array_equal(st[name], st0[name]) for name in M.TABLES)
            batch = M.batch_of(data, B, k)
            loss = _call(binding, rec[k * B:k * B + len(batch[0])], B, form, case, bf16)
            got = _read(model, opt)
            assert loss.shape == (1,) and binding.step == step0 + k
            got["loss"] = float(loss[0])
            mdl = M.model(st, batch, h, step0 + k)
            bnd = M.bounds(st, batch, h, step0 + k, form, flavour, mdl)
            ratios = M.check(got, mdl, bnd, bf16)
            r = M.worst(ratios)
            RATIOS[key] = np.maximum(RATIOS.get(key, np.zeros(7)), np.where(np.isfinite(r), r, 9.99e99))
            print(f"{M.case_id(case)} {flavour} {'bf16' if bf16 else 'f32'} step {step0 + k}: " + " ".join(f"{v:.3g}" for v in r))
            for name, v in zip(M.OUTPUTS, r):
                if not v <= 1.0:
                    where = np.argwhere(np.asarray(ratios[name]) > 1.0)[:4].tolist() if name != "loss" else []
                    detail = [(e, float(got[name][tuple(e)]), float(mdl[name][tuple(e)]), float(bnd[name][tuple(e)])) for e in where]
                    raise AssertionError((M.case_id(case), flavour, bf16, step0 + k, name, v, detail))
        engine.check_status()


def test_the_resident_cases_reach_every_slice_size_and_both_instantiations(dev):
    """engine.train_plan for the one-step calls of every resident chain: the slice size each case is meant for, every
    (Q, d) pair a plan can pick on this chip, and both the look-ahead and the generic kernel."""
    from mfcd import engine
    pairs, looks = set(), set()
    for case in M.RESIDENT:
        for flavour, bf16 in case["combos"]:
            with forced("resident", flavour):
                plan = engine.train_plan(case["B"], case["B"], case["n"], case["m"], case["d"], bf16)
            assert plan["form_name"] == "resident" and plan["resident_q"] == case["Q"], (case["label"], plan)
            assert plan["fast_math"] == (flavour == "fast")
            pairs.add((plan["resident_q"], case["d"]))
            looks.add((plan["resident_lookahead"] > 0, flavour, bf16))
    assert pairs == ({(1, d) for d in (2, 4, 8, 16, 32, 64)} | {(2, d) for d in (2, 4, 8, 16, 32, 64, 128)} | {(4, 256)}
                     | {(Q, d) for Q in (16, 32) for d in (2, 4, 8, 16, 32, 64, 128, 256)})
    assert looks == {(look, fl, bf) for look in (False, True) for fl, bf in M.ALL4}, looks


SPLITS = [(c, fl, bf) for c in M.SPLIT for fl, bf in c["combos"]]


@pytest.mark.parametrize("case,flavour,bf16", SPLITS,
                         ids=[f"{M.case_id(c)}-{fl}-{'bf16' if bf else 'f32'}" for c, fl, bf in SPLITS])
def test_one_call_of_k_steps_equals_k_calls_of_one_step(dev, case, flavour, bf16):
    from mfcd import engine
    form, h, B, N = case["form"], case["hyper"], case["B"], case["N"]
    data, st0, step0 = M.case_inputs(case, bf16)
    assert case["steps"] % 2 == 1 and case["steps"] >= 9 and N % B != 0
    rec = engine.records_from_indices(data["u"], data["i"], data["j"], case["n"], case["m"], dev, data["z"])
    with forced(form, flavour):
        model, opt, binding = _binding(st0, case["start"], h, bf16, dev)
        whole_loss = _call(binding, rec, B, form, case, bf16)
        whole = _read(model, opt)
        model, opt, binding = _binding(st0, case["start"], h, bf16, dev)
        losses = [_call(binding, rec[o:o + B], B, form, case, bf16) for o in range(0, N, B)]
        single = _read(model, opt)
        engine.check_status()
    assert len(losses) == case["steps"] == len(whole_loss)
    assert np.array_equal(np.concatenate(losses), whole_loss)
    for name in M.TABLES:
        assert np.array_equal(whole[name], single[name]), (M.case_id(case), flavour, bf16, name,
                                                           int((whole[name] != single[name]).sum()))
