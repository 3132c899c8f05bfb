"""Plans and workspace layouts as a table: one line per (train path, table dtype, shape, B, N) with the return code of
mfcd_train_plan_query, every mfcd_train_plan field and every workspace size the library computes for that case.  Two
builds of the library plan alike exactly when their tables are equal (diff the outputs).  Needs no GPU: without one the
library plans for the 256-CU fallback and an unknown occupancy; on an MI355X both are the real ones."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")]
from mfcd import _lib  # noqa: E402

SHAPES = [(256, 256, 8), (4096, 4096, 64), (16384, 16384, 128), (65536, 65536, 64), (100000, 20000, 256),   # C1 .. C5
          (7, 11, 16), (4096, 4096, 8), (500, 500, 256), (3000, 3200, 256)]   # ..., Q = 4, Q = 16 (C3 is the Q = 32 case)
BATCHES = (1, 64, 128, 4096)
MODELS = 3          # models of the multi-model workspaces
WORLDS = (2, 8)     # ranks of the data-parallel workspace


def lines():
    L = _lib.load()
    fields = [k for k, _ in _lib.TrainPlan._fields_ if k != "reserved"]
    for path in range(4):
        _lib.check(L.mfcd_set_train_path(path))
        for bf16 in (0, 1):
            for n, m, d in SHAPES:
                for B in BATCHES:
                    for N in (B, 3 * B, 40 * B, 300 * B + 5):
                        plan = _lib.TrainPlan()
                        rc = L.mfcd_train_plan_query(N, B, n, m, d, bf16, ctypes.byref(plan))
                        models = (_lib.LocalModel * MODELS)()
                        for md in models:
                            md.N, md.B = N, B
                        stage_t, stage_e = ctypes.c_size_t(0), ctypes.c_size_t(0)
                        multi_t = L.mfcd_train_local_multi_workspace_bytes(ctypes.cast(models, ctypes.c_void_p), MODELS,
                                                                           ctypes.byref(stage_t))
                        multi_e = L.mfcd_eval_multi_workspace_bytes(MODELS, ctypes.byref(stage_e))
                        sizes = [("train_ws", L.mfcd_train_workspace_bytes(N, B, n, m, d))]
                        sizes += [(f"dp_ws_w{w}", L.mfcd_dp_workspace_bytes(N, B, w, n, m, d)) for w in WORLDS]
                        sizes += [("shard_ws", L.mfcd_shard_workspace_bytes(N, B, d)),
                                  ("big_ws", L.mfcd_train_big_workspace_bytes(N, B)),
                                  ("local_multi_ws", multi_t), ("local_multi_stage", stage_t.value),
                                  ("eval_multi_ws", multi_e), ("eval_multi_stage", stage_e.value)]
                        yield " ".join([f"path={path} bf16={bf16} n={n} m={m} d={d} B={B} N={N} rc={rc}"] +
                                       [f"{k}={int(getattr(plan, k))}" for k in fields] +
                                       [f"{k}={int(v)}" for k, v in sizes])
    _lib.check(L.mfcd_set_train_path(0))


if __name__ == "__main__":
    for line in lines():
        print(line)
