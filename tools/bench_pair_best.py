"""Diagnostic: time the pair arg-max kernel (mfcd/pairs.py: pair_best_rows) beside the same arg-max by chunked torch ops
in the same run, record one `design.user_design` fit per shape, and write the table to profiles/pair_best.txt (or --out
PATH).

  kernels   1000 x 1000 with d = 2, C2 (4096 x 4096, d = 64), 256 rows of C5 width (20 000 columns) with d = 256; one
            table per row, as the design calls it.  torch: per chunk of rows (the k x k temporaries under 1 GiB) the
            squared distances n_i + n_j - 2 G G^T by one batched GEMM, clamped at 0, times sigmoid'(a_i - a_j) from
            exp and reciprocal, the diagonal masked, max over j.  MFMA bound: the v_mfma_f32_32x32x2_f32 the kernel
            issues by construction (tiles of 32 x 32 pairs x padded d / 2, 64 cycles per SIMD each) at 1024 SIMDs x
            2.4 GHz; VALU bound (d = 2 only): 15 vector instructions per ordered pair counted in the source (the score
            and the running maximum) at 1024 SIMDs x 32 lanes x 2.4 GHz, the rate bench_pair_info.py uses.  No hardware
            counters are taken by this tool.
  fits      user_design at the truth, law None: 1000 x 1000 (d = 2, all users) and C2 (d = 64, 256 users, max_iter 300):
            wall seconds, iterations, statuses, the largest gap
  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 10490 --warmup 1049 in
            this tree and in DIR, taking turns, --bench-runs N runs each (default 3)

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported; the torch form is one call per round.  Usage: bench_pair_best.py [--out PATH] [--parent-tree DIR]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import torch  # noqa: E402

from pair_bench_common import bench_lines, stretch, wall  # noqa: E402
from mfcd import design, pairs  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("PAIRS_BENCH_SECONDS", "0.5"))
SIMD_CYCLES_PER_S = 1024 * 2.4e9
LANE_SLOTS_PER_S = 1024 * 32 * 2.4e9              # as bench_pair_info.py
VALU_PER_PAIR = 15
KERNELS = (("notebooks 1000 x 1000", 1000, 1000, 2), ("C2 4096 x 4096", 4096, 4096, 64),
           ("C5 width 256 x 20000", 256, 20000, 256))
TORCH_BYTES = 1 << 30


def torch_best(A, G):
    """The kernel's definition by library ops, rows in chunks."""
    rows, k = A.shape
    per = max(1, TORCH_BYTES // (k * k * 4))
    val = torch.empty((rows, k), dtype=torch.float32, device=A.device)
    arg = torch.empty((rows, k), dtype=torch.int64, device=A.device)
    eye = torch.eye(k, dtype=torch.bool, device=A.device)
    for r0 in range(0, rows, per):
        a, g = A[r0:r0 + per], G[r0:r0 + per]
        n = (g * g).sum(2)
        q = torch.baddbmm(n[:, :, None] + n[:, None, :], g, g.transpose(1, 2), alpha=-2.0).clamp_min_(0.0)
        e = torch.exp(-(a[:, :, None] - a[:, None, :]).abs_())
        q.mul_(e).div_(e.add_(1.0).square_())
        q.masked_fill_(eye, -1.0)
        val[r0:r0 + per], arg[r0:r0 + per] = q.max(dim=2)
    return val, arg


def padded_d(d):
    return 4 if d <= 4 else 32 if d <= 32 else 64 if d <= 64 else 128 if d <= 128 else 256


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "pair_best.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_pair_best.py: kernel >= {SECONDS} s per stretch after an "
             "untimed stretch, min of two rounds (HIP events); torch: one call per round, min of two (wall), taking turns",
             "# kernel: mfcd_pair_best_rows with one table per row; torch: squared distances by baddbmm x sigmoid' then max, rows in "
             "chunks of 1 GiB of k x k temporaries; agree: columns whose torch arg-max scores within 1e-4 relative of the kernel's",
             "# MFMA bound: v_mfma_f32_32x32x2_f32 issued by construction x 64 cycles / (1024 SIMDs x 2.4 GHz); VALU bound: "
             f"{VALU_PER_PAIR} vector instructions per ordered pair (counted in the source) at 32 lanes per SIMD and cycle; no counters taken",
             f"{'shape':22s} {'d':>4s} {'kernel ms':>10s} {'torch ms':>10s} {'torch/kernel':>12s} {'MFMA bound ms':>13s} {'of MFMA':>8s} "
             f"{'VALU bound ms':>13s} {'of VALU':>8s} {'agree':>7s}"]
    print("\n".join(lines), flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(1)
    for name, rows, m, d in KERNELS:
        A = (1.5 * torch.randn(rows, m, generator=g)).to(dev)
        G = torch.empty((rows, m, d), dtype=torch.float32, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(2))
        val, arg = pairs.pair_best_rows(A, G)                                  # untimed, and the agreement check
        tv, _ = torch_best(A[:8], G[:8])
        agree = float(((tv - val[:8]).abs() <= 1e-4 * val[:8].abs() + 1e-6).float().mean())
        kern, tor = [], []
        for _ in range(2):
            stretch(lambda: pairs.pair_best_rows(A, G), SECONDS / 2)
            kern.append(stretch(lambda: pairs.pair_best_rows(A, G), SECONDS))
            tor.append(wall(lambda: torch_best(A, G))[1])
        kern, tor = min(kern), min(tor)
        tiles = rows * ((m + 127) // 128 * 4) * ((m + 63) // 64 * 2)
        mfma = tiles * (padded_d(d) // 2) * 64 / SIMD_CYCLES_PER_S * 1e3
        valu = rows * m * (m - 1) * VALU_PER_PAIR / LANE_SLOTS_PER_S * 1e3
        emit(f"{name:22s} {d:4d} {kern:10.3f} {tor:10.3f} {tor / kern:12.2f} {mfma:13.3f} {mfma / kern:8.3f} "
             + (f"{valu:13.3f} {valu / kern:8.3f}" if d <= 4 else f"{'-':>13s} {'-':>8s}") + f" {agree:7.4f}")
        del A, G, val, arg
        torch.cuda.empty_cache()
    for name, n, m, d, users, max_iter in (("notebooks 1000 x 1000 d=2", 1000, 1000, 2, None, None),
                                           ("C2 4096 x 4096 d=64, 256 users", 4096, 4096, 64, torch.arange(256), 300)):
        V = torch.randn(m, d, generator=g).to(dev)
        X = (1.5 * torch.randn(n, m, generator=g)).to(dev)
        U = torch.zeros((n, d), device=dev)
        design.user_design(U, V, X, 1.0, users=torch.arange(2), max_iter=2)   # untimed
        res, ms = wall(lambda: design.user_design(U, V, X, 1.0, users=users, max_iter=max_iter))
        st = torch.bincount(res.status, minlength=3).tolist()
        emit(f"# user_design {name}, law None, at the truth, gtol 1e-3, max_iter {max_iter or 100 + 25 * d}: {ms / 1e3:.2f} s; "
             f"iterations max {int(res.iters.max())} (mean {float(res.iters.float().mean()):.1f}); users with status 0 / 1 / 2: "
             f"{st[0]} / {st[1]} / {st[2]}; largest gap {float(res.gap.max()):.3e} (gtol d = {1e-3 * d:.1e}); atoms max "
             f"{res.pairs.shape[1]}; uniform D-efficiency mean {float(torch.exp((res.logdet_start - res.logdet) / d).mean()):.3f}")
        del V, X, U, res
        torch.cuda.empty_cache()
    if "--parent-tree" in args:
        runs = int(args[args.index("--bench-runs") + 1]) if "--bench-runs" in args else 3
        for line in bench_lines(args[args.index("--parent-tree") + 1], runs):
            emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
