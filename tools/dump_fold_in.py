"""Diagnostic: write every output of the per-row Newton kernels as .npy files, so that two builds of the library can be
compared byte for byte: run it once per build with another --out (MFCD_LIB selects the library, as for every tool), then
`python tools/dump_fold_in.py --compare DIR_A DIR_B`.  What is written:
  the Cholesky user and item step (mfcd/foldin.py: fold_in_users, fold_in_items at theta = 1/2) for the inputs of
      tests/test_fold_in.py and tests/test_item_step.py at d = 2, 16 and 64;
  their CG forms (fold_in_users(method="cg"), fold_in_items_cg at theta = 1/2), cg_iters included, for the inputs of
      tests/test_fold_in_cg.py and tests/test_item_step_cg.py (foldin_cg_model's case makers) at d = 2, 65 and 256;
      all three label kinds, both starts and both l2 for these four;
  the ratings user step (mfcd/ratings_foldin.py: ratings_fold_in_users with info=True) for the families of
      tests/test_ratings_foldin.py at d = 1, 3, 16, 17, 33 and 64, all pairs and skip-ties, from zero and from the
      family's far start: every field of the result and the information matrices.

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
    import foldin_cg_model as CG
    import foldin_model as FM
    import itemstep_model as IM
    import ratings_foldin_model as RF
    from mfcd import _lib, foldin, ratings, ratings_foldin
    dev = torch.device("cuda:0")
    L = _lib.load()
    T = L.mfcd_fold_in_chunk()
    os.makedirs(out, exist_ok=True)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    count = 0

    def save(stem, named):
        nonlocal count
        for name, t in named:
            np.save(os.path.join(out, f"{stem}_{name}.npy"), t.cpu().numpy())
            count += 1

    for d in (2, 16, 64):
        for labels in FM.LABELS:
            for start in (False, True):
                seed = 1000 * d + 10 * FM.LABELS.index(labels) + int(start)      # tests/test_fold_in.py: case()
                V, rec, off, U0 = FM.make_case(d, labels, FM.row_lengths(T), seed, start)
                for l2 in (1e-3, 1.0):
                    res = foldin.fold_in_users(to(V), to(rec), to(off), l2, to(U0))
                    save(f"d{d}_{labels}_{'init' if start else 'zero'}_l2_{l2:g}", zip(NAMES, res))
                seed = 5000 + 1000 * d + 10 * IM.LABELS.index(labels) + int(start)      # tests/test_item_step.py: case()
                U, Vi, rec, off, items = IM.make_case(d, labels, FM.row_lengths(T), seed, start)
                for l2 in (1e-3, 1.0):
                    res = foldin.fold_in_items(to(U), to(Vi), to(rec), to(off), l2, to(items), 0.5)
                    save(f"item_d{d}_{labels}_{'init' if start else 'zero'}_l2_{l2:g}", zip(ITEM_NAMES, res))
    for d in (2, 65, 256):
        cap = L.mfcd_fold_in_cg_chunk(d), L.mfcd_fold_in_cg_resident(d)
        for labels in FM.LABELS:
            for start in (False, True):
                V, rec, off, U0 = CG.user_case(d, labels, start, *cap)
                U, Vi, irec, ioff, items = CG.item_case(d, labels, start, *cap)
                for l2 in CG.L2S:
                    tag = f"d{d}_{labels}_{'init' if start else 'zero'}_l2_{l2:g}"
                    res = foldin.fold_in_users(to(V), to(rec), to(off), l2, to(U0), CG.DEVICE_MAX_ITER, method="cg")
                    save(f"cg_{tag}", zip(NAMES + ("cg_iters",), tuple(res) + (res.cg_iters,)))
                    res = foldin.fold_in_items_cg(to(U), to(Vi), to(irec), to(ioff), l2, to(items), 0.5, CG.DEVICE_MAX_ITER)
                    save(f"cg_item_{tag}", zip(ITEM_NAMES + ("cg_iters",), tuple(res) + (res.cg_iters,)))
    for d in (1, 3, 16, 17, 33, 64):
        for skip in (False, True):
            fam = RF.family(d, skip)
            data = ratings.RatingsData(fam.users, fam.items, fam.values, fam.n, RF.M_ITEMS).to(dev)
            for start in (None, fam.start):
                res, H = ratings_foldin.ratings_fold_in_users(to(start), to(fam.V), data, RF.SCALE, RF.L2, skip, info=True)
                save(f"ratings_d{d}_{'skip' if skip else 'all'}_{'zero' if start is None else 'far'}",
                     zip(res._fields + ("info",), tuple(res) + (H,)))
    print(f"{count} files written to {out} with {_lib.LIB_PATH}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
