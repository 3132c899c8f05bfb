#!/usr/bin/env python3
"""CPU sweep behind profiles/uvt_accuracy_mutations.txt and the emulation figures of profiles/uvt_accuracy.txt: the
fp32 emulation of the tiled UV^T pass (tests/uvt_model.py: emulate) against the derived bounds on every input family,
both product forms and three split widths, unmodified and with each deliberate error.  No GPU.

Usage:  python tools/uvt_accuracy_sweep.py [n m d]        (default 24 300 32, the shape of tests/test_uvt_cpu.py)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import uvt_model as M  # noqa: E402


def main():
    n, m, d = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (24, 300, 32)
    s, widths = 1.1, (32, 128, m)
    print(f"n = {n}, m = {m}, d = {d}, s = {s}, cols_per_split in {widths}, SAFETY = {M.SAFETY}")
    print("\nemulation, unmodified: largest error / bound over rows and split widths; row_stats[0..5], scal[0], scal[1]")
    caught = {mu: {} for mu in M.MUTATIONS}
    for fam in M.FAMILIES:
        U, V, X = M.family(fam, n, m, d)
        mdl = M.model(U, V, X, s)
        for form in ("fp32", "split"):
            worst = np.zeros(8)
            for cps in widths:
                bnd = M.bounds(U, V, X, s, form, cps)
                rr, rsc, problems = M.check(*M.emulate(U, V, X, s, cps, form), mdl, bnd)
                assert not problems, problems
                worst = np.maximum(worst, np.concatenate([rr.max(axis=0), rsc]))
                for mu in M.MUTATIONS:
                    if mu == "drop_mid_hi" and form != "split":
                        continue
                    r2, s2, p2 = M.check(*M.emulate(U, V, X, s, cps, form, mu), mdl, bnd)
                    outs = [f"[{c}]" for c in range(6) if (r2[:, c] > 1.0).any()] + [f"scal[{c}]" for c in range(2) if s2[c] > 1.0]
                    if outs:
                        caught[mu].setdefault(fam, set()).update(outs)
            print(f"  {fam:14s} {form:6s} " + " ".join(f"{v:8.2e}" for v in worst))
    print("\ndeliberate errors: families whose bounds they break, and through which outputs")
    for mu in M.MUTATIONS:
        print(f"  {mu}")
        for fam in M.FAMILIES:
            print(f"      {fam:14s} " + (" ".join(sorted(caught[mu][fam])) if fam in caught[mu] else "- (within every bound)"))
    U, V, X = M.family("benign", n, m, d)
    rs, sc, _ = M.model(U, V, X, s)
    print("\nolder rule on benign, |error| <= 2e-5 * max over rows |column|, emulation WITHOUT the shift (no_shift):")
    for form in ("fp32", "split"):
        for cps in widths:
            got, _ = M.emulate(U, V, X, s, cps, form, "no_shift")
            rel = [np.abs(got[:, c] - rs[:, c]).max() / np.abs(rs[:, c]).max() for c in range(6)]
            print(f"  {form:6s} cols_per_split {cps:4d}: " + " ".join(f"{v:8.2e}" for v in rel)
                  + ("   accepted" if max(rel) <= 2e-5 else "   REJECTED"))


if __name__ == "__main__":
    main()
