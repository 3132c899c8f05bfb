"""Diagnostic: write every output of the user step and of the item step (mfcd/foldin.py: fold_in_users, fold_in_items at
theta = 1/2) as .npy files, for the inputs of tests/test_fold_in.py and tests/test_item_step.py at d = 2, 16 and 64 (all
three label kinds, both starts, both l2), so that two builds of the library can be compared byte for byte: run it once per build with another --out (MFCD_LIB selects the library, as for
every tool), then `python tools/dump_fold_in.py --compare DIR_A DIR_B`.

Usage: dump_fold_in.py --out DIR | --compare DIR_A DIR_B
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

NAMES = ("U", "objective", "iters", "status")
ITEM_NAMES = ("V", "objective_start", "objective", "iters", "status")


def compare(a, b):
    files = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert files and files == sorted(f for f in os.listdir(b) if f.endswith(".npy")), "the two directories hold other files"
    differ = [f for f in files if open(os.path.join(a, f), "rb").read() != open(os.path.join(b, f), "rb").read()]
    print(f"{len(files)} files compared, {len(differ)} differ" + ("" if not differ else ": " + " ".join(differ)))
    return 1 if differ else 0


def main():
    args = sys.argv[1:]
    if args[:1] == ["--compare"]:
        return compare(args[1], args[2])
    out = args[args.index("--out") + 1]
    import torch
    import foldin_model as FM
    import itemstep_model as IM
    from mfcd import _lib, foldin
    dev = torch.device("cuda:0")
    T = _lib.load().mfcd_fold_in_chunk()
    os.makedirs(out, exist_ok=True)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    count = 0
    for d in (2, 16, 64):
        for labels in FM.LABELS:
            for start in (False, True):
                seed = 1000 * d + 10 * FM.LABELS.index(labels) + int(start)      # tests/test_fold_in.py: case()
                V, rec, off, U0 = FM.make_case(d, labels, FM.row_lengths(T), seed, start)
                for l2 in (1e-3, 1.0):
                    res = foldin.fold_in_users(to(V), to(rec), to(off), l2, to(U0))
                    for name, t in zip(NAMES, res):
                        np.save(os.path.join(out, f"d{d}_{labels}_{'init' if start else 'zero'}_l2_{l2:g}_{name}.npy"),
                                t.cpu().numpy())
                        count += 1
                seed = 5000 + 1000 * d + 10 * IM.LABELS.index(labels) + int(start)      # tests/test_item_step.py: case()
                U, Vi, rec, off, items = IM.make_case(d, labels, FM.row_lengths(T), seed, start)
                for l2 in (1e-3, 1.0):
                    res = foldin.fold_in_items(to(U), to(Vi), to(rec), to(off), l2, to(items), 0.5)
                    for name, t in zip(ITEM_NAMES, res):
                        np.save(os.path.join(out, f"item_d{d}_{labels}_{'init' if start else 'zero'}_l2_{l2:g}_{name}.npy"),
                                t.cpu().numpy())
                        count += 1
    print(f"{count} files written to {out} with {_lib.LIB_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
