"""Writes tests/golden/step_fuzz61_t275.npz: the inputs of trial 275 of `tools/fuzz_parity.py 400 61` (n = 7,
m = 11, d = 16, B = 64, N = 1462), drawn again with the fuzzer's own sequence of generator calls
(tests/step_model.py: fuzz_case(replay=True)).  python oracle/make_golden_step.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import step_model as M  # noqa: E402

g = M.fuzz_case(replay=True)
assert (g["U"].shape, g["V"].shape, g["B"], len(g["u"]), g["lr"], g["wd"]) == ((7, 16), (11, 16), 64, 1462, 1e-3, 1e-5)
np.savez(os.path.join(M.GOLDEN, "step_fuzz61_t275.npz"), **g)
print("wrote step_fuzz61_t275.npz")
