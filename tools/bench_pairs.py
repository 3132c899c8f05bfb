"""Diagnostic: time mfcd_pair_stats_rows (mfcd/pairs.py) for what = counts, sums, both, against a blocked torch
formulation of the same numbers, and write the table to profiles/pair_stats.txt (or --out PATH).

  shapes   C2 (4096 x 4096, all rows), the notebooks' 1000 x 1000, 256 rows of C5 width (m = 20000)
  torch    broadcast differences da = a[:, :, None] - a[:, None, :] (and dx) over all ordered pairs of as many rows —
           or, where one row does not fit, as many columns i of one row — as keep six fp32 temporaries of that shape
           within 1 GiB; sums over i != j are halved.  It does not use the new entry.  Its time per row does not depend
           on the row, so it is measured on the first TORCH_SECONDS of blocks and scaled to the shape's rows: the table
           says how many rows were run.
  model    achieved pairs/s and the VALU issue slots per pair that rate implies at 1024 SIMDs x 32 lanes x 2.4 GHz,
           beside the estimate made before the kernel existed (under 10 for counts, 40-50 with the transcendentals)

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two alternated rounds,
the smaller one reported.  Usage: bench_pairs.py [--out PATH] [case name ...]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from pair_bench_common import LANE_SLOTS_PER_S, ROOT, SECONDS, dev, stretch  # noqa: E402

from mfcd import pairs  # noqa: E402

TORCH_SECONDS = float(os.environ.get("PAIRS_BENCH_TORCH_SECONDS", "1.0"))
TEMP_ELEMS = (1 << 30) // (6 * 4)                 # six fp32 temporaries within 1 GiB
ESTIMATE = {"counts": "<10", "sums": "40-50", "both": "40-50"}
CASES = (("C2 4096 x 4096", 4096, 4096), ("notebooks 1000 x 1000", 1000, 1000), ("C5 width 256 x 20000", 256, 20000))


def torch_block(a, x, scale, what):
    """(counts [r, 4] f64 or None, sums [r, 4] f64 or None) contributed by columns i of a[r, ci] against all of the row
    arow[r, m]: sums over all ordered pairs (i, j), j over the whole row, the diagonal included (the caller removes it)."""
    (ai, arow), (xi, xrow) = a, x
    da = ai[:, :, None] - arow[:, None, :]
    dx = xi[:, :, None] - xrow[:, None, :]
    counts = sums = None
    if what & 1:
        sa, sx = torch.sign(da), torch.sign(dx)
        prod = sa * sx
        counts = torch.stack([(prod > 0).sum((1, 2)), (prod < 0).sum((1, 2)), (sa == 0).sum((1, 2)),
                              (sx == 0).sum((1, 2))], 1).double()
    if what & 2:
        t = dx * scale
        q = torch.sigmoid(t)
        risk = torch.nn.functional.softplus(da) - q * da
        bayes = torch.nn.functional.softplus(t) - q * t
        eacc = torch.where(da > 0, q, torch.where(da < 0, 1 - q, torch.full_like(q, 0.5)))
        bacc = torch.maximum(q, 1 - q)
        sums = torch.stack([v.sum((1, 2), dtype=torch.float64) for v in (risk, bayes, eacc, bacc)], 1)
    return counts, sums


def torch_rows(A, X, scale, what, budget_s):
    """The torch formulation over the first rows of A / X for about `budget_s` seconds → (rows done, seconds, counts,
    sums) with the diagonal removed and the ordered pairs halved."""
    rows, m = A.shape
    rper = max(1, TEMP_ELEMS // (m * m))
    cper = m if rper * m * m <= TEMP_ELEMS else max(1, TEMP_ELEMS // m)
    out_c, out_s = [], []
    torch.cuda.synchronize()
    start = time.perf_counter()
    r0 = 0
    while r0 < rows:
        r1 = min(rows, r0 + rper)
        c = torch.zeros((r1 - r0, 4), dtype=torch.float64, device=dev)
        s = torch.zeros((r1 - r0, 4), dtype=torch.float64, device=dev)
        for c0 in range(0, m, cper):
            bc, bs = torch_block((A[r0:r1, c0:c0 + cper], A[r0:r1]), (X[r0:r1, c0:c0 + cper], X[r0:r1]), scale, what)
            if bc is not None:
                c += bc
            if bs is not None:
                s += bs
        c[:, 2:] -= m                                            # the diagonal ties with itself in both rows
        s -= torch.tensor([0.6931471805599453 * m, 0.6931471805599453 * m, 0.5 * m, 0.5 * m], dtype=torch.float64, device=dev)
        out_c.append(c / 2)
        out_s.append(s / 2)
        r0 = r1
        torch.cuda.synchronize()
        if time.perf_counter() - start >= budget_s:
            break
    return r0, time.perf_counter() - start, torch.cat(out_c), torch.cat(out_s)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "pair_stats.txt")
    if "--out" in args:
        k = args.index("--out")
        out_path = args[k + 1]
        del args[k:k + 2]
    lines = [f"# {torch.cuda.get_device_name(0)}; mfcd_pair_stats_rows: >= {SECONDS} s per stretch after an untimed stretch, "
             "min of two alternated rounds (HIP events)",
             f"# torch: blocked broadcast differences, six fp32 temporaries within 1 GiB, about {TORCH_SECONDS} s of blocks "
             "after an untimed block, scaled to all rows",
             "# slots/pair: VALU issue slots per pair implied by the achieved rate at 1024 SIMDs x 32 lanes x 2.4 GHz; "
             "estimate: the figure written down before the kernel existed",
             "# ratio: torch ms / kernel ms; max dev: largest difference between the two results on the rows torch ran "
             "(counts: absolute, sums: per pair)",
             f"{'shape':24s} {'what':7s} {'pairs':>10s} {'kernel ms':>10s} {'rounds':>17s} {'Gpairs/s':>9s} {'slots/pair':>10s} "
             f"{'estimate':>8s} {'torch ms':>11s} {'rows run':>8s} {'ratio':>8s} {'max dev':>9s}"]
    print("\n".join(lines), flush=True)
    for name, rows, m in CASES:
        if args and not any(a in name for a in args):
            continue
        g = torch.Generator(device=dev).manual_seed(rows + m)
        A = torch.randn(rows, m, device=dev, generator=g)
        X = torch.randn(rows, m, device=dev, generator=g)
        npairs = rows * (m * (m - 1) // 2)
        for what, w in (("counts", 1), ("sums", 2), ("both", 3)):
            ours = lambda: pairs.pair_stats_rows(A, X, 1.0, what)  # noqa: E731
            rounds = []
            torch_rows(A, X, 1.0, w, 0.0)                                     # one untimed block
            tdone = []
            for _ in range(2):
                stretch(ours, SECONDS)
                rounds.append(stretch(ours, SECONDS))
                tdone.append(torch_rows(A, X, 1.0, w, TORCH_SECONDS))
            ms = min(rounds)
            nrun, secs, tc, ts = min(tdone, key=lambda t: t[1] / t[0])
            torch_ms = secs / nrun * rows * 1e3
            c, s = ours()
            dev_max = 0.0                                                     # largest deviation between the two, per pair
            if c is not None:
                dev_max = max(dev_max, float((c[:nrun].double() - tc).abs().max()))
            if s is not None:
                dev_max = max(dev_max, float(((s[:nrun] - ts).abs() / (m * (m - 1) // 2)).max()))
            rate = npairs / (ms * 1e-3)
            line = (f"{name:24s} {what:7s} {npairs:10.3e} {ms:10.3f} {rounds[0]:8.3f}/{rounds[1]:8.3f} {rate / 1e9:9.1f} "
                    f"{LANE_SLOTS_PER_S / rate:10.1f} {ESTIMATE[what]:>8s} {torch_ms:11.1f} {nrun:8d} {torch_ms / ms:7.1f}x "
                    f"{dev_max:9.2e}")
            print(line, flush=True)
            lines.append(line)
        del A, X
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
