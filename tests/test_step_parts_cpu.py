"""CPU tests of the parts of tests/step_model.py (evaluation, coefficients, dense gradient, Adam from a dense gradient, the
step from given coefficients): the numpy fp32 emulation of every part and the C oracle's forward, grad, adam and
eval_batches stay inside the derived bounds on every input tests/test_step_parts.py runs on the GPU; the f64 model alone
leaves at most 1 evaluation sample in 1000 undecided (and at most 2 per batch); every deliberate error of PART_FAULTS is
rejected; and for every part and output the largest emulation ratio is above 0.01, so that the bound is not so wide that
a subtly wrong kernel would pass.

`pytest -s` prints the largest error / bound per part and output (profiles/step_parts_accuracy_cpu.txt is one such run)."""
import functools

import numpy as np
import pytest

import step_model as M

PARTS = ("eval", "coef", "dense_grad", "grad_from_coef", "adam_dense", "apply_step")
FIGURES = {}        # (who, part) -> {output: largest ratio}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if FIGURES:
        print("\nlargest error / bound per part and output (correct: 0 = the one admissible count, 1 = an end of the interval)")
        for (who, part), r in sorted(FIGURES.items()):
            print(f"  {who:9s} {part:15s} " + " ".join(f"{k} {v:8.2e}" for k, v in sorted(r.items())))


def _note(who, part, ratios):
    f = FIGURES.setdefault((who, part), {})
    for k, r in ratios.items():
        v = float(np.max(r)) if np.size(r) else 0.0
        f[k] = max(f.get(k, 0.0), v if np.isfinite(v) else 9.99e99)
    return max([float(np.max(r)) for r in ratios.values() if np.size(r)] + [0.0])


def _first_batch(data, B):
    return M.batch_of(data, B, 0)


def _apply_cases():
    """The streaming shapes: (case, state, batch, step, coefficients from the f64 model rounded to fp32)."""
    for case in M.STREAMING:
        data, st, step = M.case_inputs(case)
        for k in (0, case["steps"] - 1):          # a full batch and the last (short where the case has one)
            batch = M.batch_of(data, case["B"], k)
            mdl, _ = M.coef_model(st["U"], st["V"], batch, len(batch[0]))
            yield case, st, batch, step, mdl["g"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _run(part, fault=None, orc=None):
    """Every input of `part` through its emulation (with `fault`) and, where there is one, the C oracle -> the largest
    ratio of the emulation.  Fills FIGURES when fault is None."""
    top = 0.0
    who = "emulate"

    def note(w, ratios):
        return _note(w, part, ratios) if fault is None else max([float(np.max(r)) for r in ratios.values() if np.size(r)] + [0.0])

    if part == "eval":
        for d, N, B, fam in M.eval_cases():
            if fault is not None and (N > 1000 or d > 100):
                continue
            for bf16 in (False, True):
                data = M.eval_input(d, N, B, fam, bf16)
                mdl, bnd = M.eval_model(data["U"], data["V"], data, B)
                got = M.emu_eval(data["U"], data["V"], data, B, fault)
                top = max(top, note(who, M.eval_check(got, mdl, bnd)))
                if orc is not None and fault is None:
                    loss, corr, p = orc.eval_batches(data["U"], data["V"], data["u"], data["i"], data["j"], data["z"], B)
                    r = M.eval_check(dict(p=p, loss=loss, correct=corr), mdl, bnd)
                    _, term = orc.forward(data["U"], data["V"], data["u"], data["i"], data["j"], data["z"])
                    r["term"] = M._ratio(term, mdl["term"], bnd["term"])
                    note("c oracle", r)
    elif part == "coef":
        for d, B, div, fam, _ in M.coef_cases():
            data = M.part_family(fam, 50, 40, d, B, B)
            batch = _first_batch(data, B)
            mdl, bnd = M.coef_model(data["U"], data["V"], batch, div)
            got = M.emu_coef(data["U"], data["V"], batch, div, fault)
            top = max(top, note(who, M._ratios(got, mdl, bnd, ("g", "term", "p"))))
            if orc is not None and fault is None:
                p, term = orc.forward(data["U"], data["V"], *batch)
                note("c oracle", M._ratios(dict(p=p, term=term), mdl, bnd, ("term", "p")))
    elif part in ("dense_grad", "grad_from_coef"):
        for case in M.grad_cases():
            label, n, m, d, B, fam, seed = case
            if fault is not None and B > 1000:
                continue
            data = M.grad_input(case)
            batch = _first_batch(data, B)
            E = M.plan(n, m, d)[2]
            if part == "dense_grad":
                mdl, bnd = M.grad_model(data["U"], data["V"], batch, divisor=B)
                co = M.emu_coef(data["U"], data["V"], batch, B)
                got = M.emu_grad(data["U"], data["V"], batch, co["g"], fault, E)
                got["term"] = co["term"]
                if orc is not None and fault is None:
                    _, _, dU, dV = orc.grad(data["U"], data["V"], *batch)
                    note("c oracle", M._ratios(dict(gradU=dU, gradV=dV), mdl, bnd, ("gradU", "gradV")))
            else:
                g = M.signed_coefficients(B)
                mdl, bnd = M.grad_model(data["U"], data["V"], batch, g=g)
                got = M.emu_grad(data["U"], data["V"], batch, g, fault, E)
            top = max(top, note(who, M._ratios(got, mdl, bnd, ("gradU", "gradV", "term"))))
    elif part == "adam_dense":
        for case in M.adam_cases():
            label, n, m, d, start, h, aligned = case
            if fault is not None and n * d > 10 ** 5:
                continue
            st, gU, gV, step, special = M.adam_input(case)
            mdl, bnd = M.adam_model(st, gU, gV, h, step)
            got = M.emu_adam(st, gU, gV, h, step, fault, M.plan(n, m, d, aligned)[2])
            top = max(top, note(who, M.check_tables(got, mdl, bnd)))
            if orc is not None and fault is None:
                s2 = {k: np.array(v, dtype=np.float32) for k, v in st.items()}
                for T, g in (("U", gU), ("V", gV)):
                    orc.adam(s2[T], s2["m" + T], s2["v" + T], g, step, lr=h["lr"], betas=(h["beta1"], h["beta2"]),
                             eps=h["eps"], wd=h["wd"])
                note("c oracle", M.check_tables(s2, mdl, bnd))
    elif part == "apply_step":
        for case, st, batch, step, g in _apply_cases():
            h = case["hyper"]
            mdl, bnd = M.apply_model(st, batch, g, h, step)
            got = M.emu_apply(st, batch, g, h, step, fault, M.plan(case["n"], case["m"], case["d"])[2])
            top = max(top, note(who, M.check_tables(got, mdl, bnd)))
        case = M.STREAMING[0]                      # B = 0: a pure weight-decay / moment step
        _, st, step = M.case_inputs(case)
        empty = tuple(np.zeros(0, np.int64) for _ in range(3)) + (np.zeros(0, np.float32),)
        mdl, bnd = M.apply_model(st, empty, np.zeros(0, np.float32), case["hyper"], step)
        got = M.emu_apply(st, empty, np.zeros(0, np.float32), case["hyper"], step, fault, 256)
        top = max(top, note(who, M.check_tables(got, mdl, bnd)))
    return top


def test_the_cases_cover_what_they_claim():
    # both access widths and every chunk count of make_plan, for the Adam entry; the misaligned case is scalar at d = 64
    plans = {M.plan(n, m, d, al)[:2] for _, n, m, d, _, _, al in M.adam_cases()}
    assert plans == {(v, c) for v in (1, 4) for c in (1, 2, 4)}, plans
    assert M.plan(37, 41, 64, False)[0] == 1 and M.plan(37, 41, 64, True)[0] == 4
    # M.plan is make_plan: wherever the library reports a streaming plan (a host-side query, no GPU) the two agree
    import ctypes
    from mfcd import _lib
    L, q, seen = _lib.load(), _lib.TrainPlan(), set()
    for n, m, d in [c[1:4] for c in M.adam_cases()] + [(n, m, d) for d, (n, m, _) in M.GRAD_SHAPES.items()]:
        assert L.mfcd_train_plan_query(64, 64, n, m, d, 0, ctypes.byref(q)) == 0
        if q.form == 1:
            vec, chunks, E = M.plan(n, m, d)
            assert (q.streaming_vec, q.streaming_chunks) == (vec, chunks), (n, m, d)
            assert q.streaming_blocks == -(-n * d // E) - (-m * d // E)
            seen.add((vec, chunks))
    assert seen == {(v, c) for v in (1, 4) for c in (1, 2, 4)}, seen
    for _, n, m, d, _, _, al in M.adam_cases():
        E = M.plan(n, m, d, al)[2]
        if n > 3:                                  # a partial last U block: V starts in a block of its own
            assert (n * d) % E != 0
    # the dense gradient: rows that span workgroups (d = 1023, 1024), several blocks per table, both widths
    for d, (n, m, B) in M.GRAD_SHAPES.items():
        vec, _, E = M.plan(n, m, d)
        assert vec == (4 if d % 4 == 0 else 1) and n * d > E and m * d > E
    assert M.plan(9, 8, 1023)[2] == 256 and 1023 > 3 * 256
    # the half family holds what it is for
    data = M.eval_input(64, 64 * 9 + 5, 64, "half")
    mdl, bnd = M.eval_model(data["U"], data["V"], data, 64)
    z = data["z"]
    assert all((mdl["zero"] & (z == lab)).any() for lab in (0.0, 1.0, 0.5))
    assert (mdl["zero"] & (data["i"] == data["j"])).any() and (mdl["zero"] & (data["u"] == 0) & (data["i"] != data["j"])).any()
    near = ~mdl["zero"] & (np.abs(mdl["p"] - 0.5) < 1e-6)
    assert (near & mdl["decided"] & (mdl["p"] > 0.5)).any() and (near & mdl["decided"] & (mdl["p"] < 0.5)).any()
    assert (~mdl["decided"]).sum() == 2 and (mdl["p"][~mdl["decided"]] != 0.5).all()
    assert (mdl["p"][mdl["zero"]] == 0.5).all() and (bnd["p"][mdl["zero"]] == 0.0).all()
    # every subset of the three nullable outputs of the coefficient entry
    assert {s for *_, s in M.coef_cases()} == set(M.COEF_SUBSETS) and len(set(M.COEF_SUBSETS)) == 8
    assert {(B, div // B) for _, B, div, _, _ in M.coef_cases()} == {(B, k) for B in M.COEF_B for k in (1, 8)}


def test_undecided_samples_are_rare():
    """On the f64 model alone: over all evaluation inputs together at most 1 sample in 1000 is undecided (|p - 0.5| <=
    dp and not of the exact-zero kind), and no batch holds more than 2."""
    total = undecided = 0
    for d, N, B, fam in M.eval_cases():
        for bf16 in (False, True):
            data = M.eval_input(d, N, B, fam, bf16)
            mdl, _ = M.eval_model(data["U"], data["V"], data, B)
            total += N
            undecided += int((~mdl["decided"]).sum())
            assert (mdl["hi"] - mdl["lo"]).max() <= 2, (d, N, B, fam, bf16)
    print(f"undecided evaluation samples: {undecided} of {total}")
    assert undecided * 1000 <= total, (undecided, total)


@pytest.mark.parametrize("part", PARTS)
def test_emulation_and_c_oracle_hold_the_bounds(orc, part):
    top = _run(part, None, orc)
    for (who, p), r in FIGURES.items():
        if p == part:
            assert all(v <= 1.0 for v in r.values()), (who, part, r)
    assert top <= 1.0


# the parts a fault is looked for in: every fault must be rejected in each of them
POWER = {
    "match_ge_half": ("eval",),
    "match_rounded_label": ("eval",),
    "short_batch_by_B": ("eval",),
    "divisor_ignored": ("coef",),
    "flip_j_sign": ("dense_grad", "grad_from_coef", "apply_step"),
    "drop_second_hit": ("dense_grad", "grad_from_coef", "apply_step"),
    "partial_block_unwritten": ("dense_grad", "adam_dense"),
    "seam": ("grad_from_coef", "adam_dense", "apply_step"),
    "bias_from_step0": ("adam_dense", "apply_step"),
    "param_not_updated": ("adam_dense", "apply_step"),
}


@pytest.mark.parametrize("fault", M.PART_FAULTS)
def test_every_injected_fault_is_rejected(fault):
    assert set(POWER) == set(M.PART_FAULTS) and len(M.PART_FAULTS) == 10
    tops = {part: _run(part, fault) for part in POWER[fault]}
    print(f"{fault}: largest error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in tops.items()))
    assert all(v > 1.0 for v in tops.values()), tops


def test_the_bounds_are_tight(orc):
    """For every part and output the largest emulation ratio over all cases is above 0.01."""
    for part in PARTS:
        _run(part, None, orc)
        r = FIGURES[("emulate", part)]
        assert r and all(v > 0.01 for v in r.values()), (part, r)
