"""Diagnostic: time mfcd_topk_rows (mfcd/topk.py) against what exists without it.

  dense mode   C3 (16384^2): against the torch.topk calls mfcd/sampling.py: build_law makes for a dense X
               (k = 100 both ends: two calls; k = 1638 best: one)
  factor mode  C3 (d = 128), C4 (d = 64), C5 (d = 256): against a 2048-row slab GEMM A[r0:r1] @ B.T followed by
               torch.topk per slab, and against the floor 2 n m d / 157.3 TF (fp32 MFMA, one pass over the scores: the
               slab form computes every score once) plus the output write at 8 TB/s

Timing as DESIGN 3.4: HIP events around >= 0.25 s of back-to-back calls after an untimed 0.25 s of the same; the two
sides of a comparison alternate inside this one process, two rounds each.  Usage: bench_topk.py [case name ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd")]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import torch  # noqa: E402

from mfcd import topk  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("TOPK_BENCH_SECONDS", "0.25"))
SLAB = 2048


def stretch(fn, seconds):
    """Milliseconds per call over at least `seconds` of back-to-back calls (HIP events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, total, per = 0, 0.0, 1
    while total < seconds * 1e3:
        t0.record()
        for _ in range(per):
            fn()
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        total += ms
        calls += per
        per = max(1, min(64, int(per * 0.05 * 1e3 / max(ms, 1e-3))))     # ~50 ms between event pairs
    return total / calls


def compare(name, ours, other, floor_ms, other_name):
    res = {"ours": [], "other": []}
    for _ in range(2):
        for key, fn in (("ours", ours), ("other", other)):
            stretch(fn, SECONDS)                                            # untimed
            res[key].append(stretch(fn, SECONDS))
    a, b = min(res["ours"]), min(res["other"])
    floor = f"  floor {floor_ms:8.3f} ms ({floor_ms / a * 100:4.1f}% of it reached)" if floor_ms else ""
    print(f"{name:34s} topk_rows {a:9.3f} ms (rounds {res['ours'][0]:.3f} / {res['ours'][1]:.3f})   {other_name} {b:9.3f} ms "
          f"(rounds {res['other'][0]:.3f} / {res['other'][1]:.3f})   ratio {b / a:5.2f}x{floor}", flush=True)


def dense_cases(only):
    n = m = 16384
    X = torch.randn(n, m, device=dev)
    for k, ends in ((100, "both"), (1638, "best")):
        name = f"dense C3 k={k} {ends}"
        if only and not any(o in name for o in only):
            continue
        if ends == "both":
            other = lambda: (torch.topk(X, k=k, dim=1)[1].to(torch.int32), torch.topk(-X, k=k, dim=1)[1].to(torch.int32))  # noqa: E731
        else:
            other = lambda: torch.topk(X, k=k, dim=1)[1].to(torch.int32)  # noqa: E731
        compare(name, lambda: topk.topk_rows(X, k, ends=ends), other, 0.0, "torch.topk")
    del X
    torch.cuda.empty_cache()


def factor_cases(only):
    for cname, n, m, d, k, ends in (("C3", 16384, 16384, 128, 100, "both"), ("C4", 65536, 65536, 64, 100, "both"),
                                    ("C4", 65536, 65536, 64, 6553, "best"), ("C5", 100000, 20000, 256, 2000, "best")):
        name = f"factor {cname} d={d} k={k} {ends}"
        if only and not any(o in name for o in only):
            continue
        A = torch.randn(n, d, device=dev) / d ** 0.5
        B = torch.randn(m, d, device=dev) / d ** 0.5

        def other():
            out = torch.empty((n, k), dtype=torch.int32, device=dev)
            low = torch.empty((n, k), dtype=torch.int32, device=dev) if ends == "both" else None
            for r0 in range(0, n, SLAB):
                S = A[r0:r0 + SLAB] @ B.t()
                out[r0:r0 + SLAB] = torch.topk(S, k=k, dim=1)[1]
                if low is not None:
                    low[r0:r0 + SLAB] = torch.topk(-S, k=k, dim=1)[1]
            return out, low

        nends = 2 if ends == "both" else 1
        floor_ms = (2.0 * n * m * d / 157.3e12 + 4.0 * n * k * nends / 8e12) * 1e3
        compare(name, lambda: topk.topk_rows((A, B), k, ends=ends), other, floor_ms, f"{SLAB}-row GEMM + torch.topk")
        del A, B
        torch.cuda.empty_cache()


if __name__ == "__main__":
    only = sys.argv[1:]
    print(f"# {torch.cuda.get_device_name(0)}; >= {SECONDS} s per stretch after an untimed stretch, min of two alternated rounds",
          flush=True)
    dense_cases(only)
    factor_cases(only)
