#!/usr/bin/env python3
"""Golden vectors for the dense metric functions on DEGENERATE rows (TEST INFRASTRUCTURE — needs the reference checkout).

Imports the *unmodified* reference and runs its compute_alpha_and_norm_ratios (structure.py:958-1082) and
compute_reconstruction_error (structure.py:925-955) on the `degenerate` input family of tests/uvt_model.py at
(n, m, d) = (48, 96, 8) — constant X rows (0, 0.3, 1000), zero U rows — and on its all-zero-V variant (cold start).
What the reference returns, including what its except path leaves, is stored with the inputs in
tests/golden/metrics_degenerate.npz (data only); tests/test_uvt.py holds the drop-in module to it.

The reference filters rows with `np.std(row) > 1e-8`, `dot(x, x) > 1e-8` and `dot(u, u) > 1e-8` on fp32 rows centred
in fp32.  Every row generated here is at least a factor 100 away from those thresholds on either side (asserted
below), so which rows a filter keeps does not depend on rounding.

Usage:  OMP_NUM_THREADS=4 PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_metrics.py <reference directory>
"""
import os
import sys
import types

os.environ.setdefault("OMP_NUM_THREADS", "4")
sys.dont_write_bytecode = True
_stub = types.ModuleType("torch.utils.tensorboard")      # imported at structure.py:10, used only under `if False`
_stub.SummaryWriter = object
sys.modules["torch.utils.tensorboard"] = _stub
HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.path.append(os.path.join(HERE, "..", "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import structure as R  # noqa: E402  (the reference)
import uvt_model as M  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "metrics_degenerate.npz")
N, MM, D, S = 48, 96, 8, 1.1
M14 = ["alpha", "norm_X", "norm_ratio", "rec_scaled", "pearson_mean", "pearson_std", "spearman_mean", "spearman_std",
       "svd_err", "slopes", "correlations", "spearman_scores", "rec_scaled_per_row", "alpha_per_row"]


def _clear_of(value, threshold, what):
    assert value < threshold / 100 or value > threshold * 100, (what, value)


def main():
    out = {"s": np.asarray(S)}
    for variant in ("degenerate", "degenerate_v0"):
        U, V, X = M.family(variant, N, MM, D)
        model = types.SimpleNamespace(U=torch.from_numpy(U.copy()), V=torch.from_numpy(V.copy()))
        Xt = torch.from_numpy(X.copy())
        # the rows exactly as the reference centres them (fp32 tensors), against its three thresholds
        G = torch.matmul(model.U, model.V.t())
        G -= torch.mean(G, dim=1, keepdim=True)
        Xc = Xt.clone()
        Xc -= torch.mean(Xc, dim=1, keepdim=True)
        kept, alpha_rows = [0, 0, 0], []
        for r in range(N):
            x, u = Xc[r].numpy(), G[r].numpy()
            for k, (v, nm) in enumerate(((np.std(x), "std x"), (np.std(u), "std u"), (np.dot(x, x), "x.x"), (np.dot(u, u), "u.u"))):
                _clear_of(float(v), 1e-8, (variant, r, nm))
            kept[0] += np.std(x) > 1e-8 and np.std(u) > 1e-8
            kept[1] += np.dot(x, x) > 1e-8 and np.std(u) > 1e-8
            kept[2] += np.dot(u, u) > 1e-8
            alpha_rows.append(np.dot(x, u) / np.dot(u, u) if np.dot(u, u) > 1e-8 else 0.0)
        res = R.compute_alpha_and_norm_ratios(model, Xt)
        assert len(res) == 14
        for nm, v in zip(M14, res):
            out[f"{variant}.m14_{nm}"] = np.asarray(v, dtype=np.float64)
        assert len(res[10]) == kept[0] and len(res[9]) == kept[1] and len(res[13]) == N
        # which rows took alpha_i = 0.0: the u.u filter, row by row
        assert sum(isinstance(v, float) and v == 0.0 for v in res[13]) == N - kept[2]
        assert np.array_equal(np.asarray(res[13], dtype=np.float64), np.asarray(alpha_rows, dtype=np.float64))
        out[f"{variant}.rec_error"] = np.asarray(R.compute_reconstruction_error(model, Xt, S), dtype=np.float64)
        out[f"{variant}.U"], out[f"{variant}.V"], out[f"{variant}.X"] = U, V, X
        print(variant, "rows kept by the correlation / slope / alpha_i filters:", kept, "of", N,
              "| pearson_mean", res[4], "svd_err", res[8], "rec_error", float(out[f"{variant}.rec_error"]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
