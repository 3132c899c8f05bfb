"""Diagnostic: time the implicit-feedback risk (mfcd/implicit.py; csrc/implicit.hip) — value plus both table gradients per
call — beside the same quantities by chunked torch ops in the same process, and write the table to profiles/implicit.txt
(or --out PATH).

  ml100k    bench_pair_ragged.py's MovieLens-100k-shaped synthetic table (943 x 1682, 100 000 entries), d = 16
  large     20 000 x 20 000, 2 M entries, long-tailed rows, d = 64
  factored  n = m = 65 536, d = 64, 10 observed items per user
  kernel form  one sweep of mfcd.implicit._Plan: per row block mfcd_implicit_rows with the gradient, g V and g^T U
  torch form   per chunk of rows: the row block U[rows] @ V.T, the class masks, one rows x L x m broadcast of
               softplus / sigmoid of (a_j - a_i) under the (positive, negative) mask, summed over both axes, then the
               same two GEMMs.  On the two large shapes it is timed on the first ROWS_SUB rows only (the whole table is
               4e10 pairs of temporaries), next to the kernel form on the same rows
  step      one fused fit_implicit step split: the sweep with factor-mode calls, the same calls alone, the calls in
            dense mode on precomputed scores (what is left is the score slab), the GEMMs (sweep minus calls), mfcd_adam_dense
  rate      (positive, negative) pairs per second and compute unit of the dense-mode call without and with the gradient,
            next to mfcd_pair_ragged_grad's ordered pairs per second and compute unit on the same table's ratings
  fill      lanes of a positive-pass workgroup that work on a positive, over the tiles of the table's rows

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported, the forms taking turns; the large torch forms: wall time of one call, the second of two.
--parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns, appended to the table.

Usage: bench_implicit.py [--out PATH] [--skip-large] [--parent-tree DIR] [--bench-runs N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda:0")
TORCH_ELEMS = 1 << 26              # elements of the torch form's rows x L x m temporaries per chunk
ROWS_SUB = 512


def torch_form(U, V, off, items, coef, rows):
    """Value and table gradients of rows [0, rows) by library ops → (risk f64, dU [rows, d], dV)."""
    m = V.shape[0]
    lens = (off[1:rows + 1] - off[:rows])
    dU, dV = torch.empty((rows, U.shape[1]), device=dev), torch.zeros_like(V)
    risk = torch.zeros((), dtype=torch.float64, device=dev)
    r0 = 0
    lens_h = lens.cpu().numpy()
    while r0 < rows:
        r1, width = r0, 0                              # as many rows as fit: (r1 - r0) x max L x m <= TORCH_ELEMS
        while r1 < rows and (r1 - r0 + 1) * max(width, int(lens_h[r1]), 1) * m <= TORCH_ELEMS:
            width = max(width, int(lens_h[r1]), 1)
            r1 += 1
        r1 = max(r1, r0 + 1)
        width = max(width, int(lens_h[r0]), 1)
        nb = r1 - r0
        S = U[r0:r1] @ V.t()
        k = torch.arange(width, device=dev)[None, :]
        valid = k < lens[r0:r1, None]
        idx = torch.where(valid, items[(off[r0:r1, None] + k).clamp(max=items.numel() - 1)].long(), torch.zeros_like(k))
        neg = torch.ones((nb, m), dtype=torch.bool, device=dev)
        neg[torch.arange(nb, device=dev)[:, None].expand_as(idx)[valid], idx[valid]] = False
        v = S[:, None, :] - torch.gather(S, 1, idx)[:, :, None]
        w = (valid[:, :, None] & neg[:, None, :]).float()
        risk += ((torch.nn.functional.softplus(v) * w).sum((1, 2)).double() * coef[r0:r1].double()).sum()
        sg = torch.sigmoid(v) * w
        g = sg.sum(1)
        g.scatter_add_(1, idx, -sg.sum(2) * valid.float())
        g *= coef[r0:r1, None]
        dU[r0:r1] = g @ V
        dV.addmm_(g.t(), U[r0:r1])
        r0 = r1
    return risk, dU, dV


def lane_fill(lengths):
    """Share of a positive-pass workgroup's 256 lanes that work on a positive, over the tiles of rows of these lengths."""
    busy = tiles = 0
    for L in lengths:
        for p0 in range(0, int(L), 256):
            nt = min(256, int(L) - p0)
            busy += nt * (256 >> max(nt - 1, 0).bit_length())
            tiles += 1
    return busy / (256.0 * max(tiles, 1))


def compare(name, U, V, data, emit, sub=None, split=True):
    from pair_bench_common import alternated, wall
    from mfcd import _lib, implicit, ratings
    n, m, d = U.shape[0], V.shape[0], U.shape[1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = implicit._Plan(n, m, dev, data, None, "pairs", None)
    pairs = int((plan.counts[:, 0] * plan.counts[:, 1]).sum())
    kern = lambda: plan.sweep(U, V, True)    # noqa: E731
    risk, dU, dV = kern()
    full = alternated([kern])[0]
    emit(f"  kernel form, all {n} rows ({pairs:.3e} pairs, row blocks of {plan.row_block}): {full:10.3f} ms per value + "
         f"gradients    risk {float(risk):.6f}")
    rows = n if sub is None else sub
    if sub is None:
        ref = lambda: torch_form(U, V, data.row_off, data.item, plan.coef, rows)    # noqa: E731
        ms = alternated([kern, ref])
        k_ms, t_ms = ms
    else:
        sub_data = (data.row_off[:rows + 1].contiguous(), data.item)
        sub_plan = implicit._Plan(rows, m, dev, sub_data, None, "pairs", None)
        sub_plan.coef, sub_plan.coef64 = plan.coef[:rows].contiguous(), plan.coef64[:rows].contiguous()
        kern_sub = lambda: sub_plan.sweep(U[:rows], V, True)    # noqa: E731
        ref = lambda: torch_form(U, V, data.row_off, data.item, plan.coef, rows)    # noqa: E731
        k_ms = alternated([kern_sub])[0]
        t_ms = min(wall(ref)[1], wall(ref)[1])
        kern = kern_sub
    want = ref()
    got = kern()
    emit(f"  rows 0 .. {rows - 1}: kernel form {k_ms:10.3f} ms    torch form {t_ms:10.3f} ms    torch / kernel {t_ms / k_ms:.1f}"
         + ("" if sub is None else "    (torch form: wall time of one call)"))
    emit(f"  against the torch form on those rows: risk {float(got[0]):.8f} vs {float(want[0]):.8f}; largest |dU - dU'| "
         f"{float((got[1] - want[1]).abs().max()):.2e} of {float(want[1].abs().max()):.2e}, largest |dV - dV'| "
         f"{float((got[2] - want[2]).abs().max()):.2e} of {float(want[2].abs().max()):.2e}"
         + ("" if sub is None else " (dV: the rows of the subset only)"))
    lengths = (data.row_off[1:] - data.row_off[:-1]).cpu().numpy()
    emit(f"  positives per row {lengths.min()} .. {lengths.max()} (median {int(np.median(lengths))}); lane fill of the positive "
         f"pass {100.0 * lane_fill(lengths):.1f} %")
    if not split:
        return
    # the fused step, split
    L = _lib.load()
    rows_x = min(n, 4096)
    Ux = U[:rows_x]
    X = (Ux @ V.t()).contiguous()
    x_data = (data.row_off[:rows_x + 1].contiguous(), data.item)
    ids = torch.arange(rows_x, device=dev)
    coef = plan.coef[:rows_x].contiguous()
    x_pairs = int((plan.counts[:rows_x, 0] * plan.counts[:rows_x, 1]).sum())
    fact = lambda: implicit.implicit_rows((U, V), x_data, rows=ids, grad=True, coef=coef)    # noqa: E731
    dense = lambda: implicit.implicit_rows(X, x_data, grad=True, coef=coef)    # noqa: E731
    stats = lambda: implicit.implicit_rows(X, x_data)    # noqa: E731
    xp = implicit._Plan(rows_x, m, dev, x_data, None, "pairs", None)
    sweep = lambda: xp.sweep(Ux, V, True)    # noqa: E731
    mU, vU, mV, vV = (torch.zeros_like(t) for t in (U, U, V, V))
    Uc, Vc = U.clone(), V.clone()
    gU, gV = torch.randn_like(U) * 1e-3, torch.randn_like(V) * 1e-3
    ptrs = [_lib.ptr(t) for t in (Uc, Vc, mU, vU, mV, vV, gU, gV)]
    adam = lambda: _lib.check(L.mfcd_adam_dense(*ptrs, 1, n, m, d, 1e-3, 0.9, 0.999, 1e-8, 0.0, _lib.stream_ptr(dev)))    # noqa: E731
    t_sweep, t_fact, t_dense, t_stats, t_adam = alternated([sweep, fact, dense, stats, adam])
    emit(f"  one fused step on rows 0 .. {rows_x - 1} ({x_pairs:.3e} pairs): sweep {t_sweep:.3f} ms = scores (factor-mode calls "
         f"minus dense-mode calls) {t_fact - t_dense:.3f} + kernel (dense-mode call on precomputed scores) {t_dense:.3f} + "
         f"GEMMs (sweep minus factor-mode calls) {t_sweep - t_fact:.3f}; mfcd_adam_dense on the whole tables {t_adam:.3f} ms "
         "(host time of every call included)")
    emit(f"  pair rate of the dense-mode call: {x_pairs / t_stats / 1e6 / cus:.3f} G pairs/s per CU without the gradient "
         f"({t_stats:.3f} ms, one exp per pair), {x_pairs / t_dense / 1e6 / cus:.3f} G pairs/s per CU with it ({t_dense:.3f} ms, "
         f"two); {cus} CUs")
    if hasattr(data, "value"):
        a = ratings.ragged_scores(U, V, data)[0]
        rag = lambda: ratings.pair_ragged_grad(a, data)    # noqa: E731
        t_rag = alternated([rag])[0]
        ordered = int((lengths.astype(np.int64) * (lengths.astype(np.int64) - 1)).sum())
        emit(f"  mfcd_pair_ragged_grad on the same table's ratings in this run: {ordered:.3e} ordered pairs in {t_rag:.3f} ms = "
             f"{ordered / t_rag / 1e6 / cus:.3f} G ordered pairs/s per CU")


def main():
    args = sys.argv[1:]
    from pair_bench_common import SECONDS, bench_lines
    from bench_pair_ragged import long_tailed, ml100k_shaped, strided
    from mfcd import ratings
    out_path = os.path.join(ROOT, "profiles", "implicit.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_implicit.py: >= {SECONDS} s per stretch after an untimed "
             "stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    g = torch.Generator().manual_seed(1)
    u, i, v, n, m = ml100k_shaped(np.random.default_rng(0))
    data = ratings.RatingsData(u, i, v, n, m).to(dev)
    U, V = (torch.randn(n, 16, generator=g) / 4.0).to(dev), (torch.randn(m, 16, generator=g) / 4.0).to(dev)
    emit(f"ml100k-shaped: {n} x {m}, d = 16, {data.entries} observed entries")
    compare("ml100k", U, V, data, emit)
    if "--skip-large" not in args:
        rng = np.random.default_rng(0)
        n = m = 20000
        L = long_tailed(n, 2000000, 5, 5000, rng)
        u, i, v = strided(n, m, L, rng)
        data = ratings.RatingsData(u, i, v, n, m).to(dev)
        U, V = (torch.randn(n, 64, generator=g) / 8.0).to(dev), (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"large: {n} x {m}, d = 64, {data.entries} observed entries; the torch form on the first {ROWS_SUB} rows")
        compare("large", U, V, data, emit, sub=ROWS_SUB)
        n = m = 65536
        rng = np.random.default_rng(1)
        users = np.repeat(np.arange(n), 10)
        items = (rng.integers(0, m, n)[users] + np.tile(np.arange(10) * 1087, n)) % m      # 10 distinct items per user
        data = ratings.RatingsData(users, items, np.ones(users.size, np.float32), n, m).to(dev)
        U, V = (torch.randn(n, 64, generator=g) / 8.0).to(dev), (torch.randn(m, 64, generator=g) / 8.0).to(dev)
        emit(f"factored: {n} x {m}, d = 64, {data.entries} observed entries (10 per user); the torch form on the first "
             f"{ROWS_SUB} rows")
        compare("factored", U, V, data, emit, sub=ROWS_SUB)
    emit("parent comparison: this change adds csrc/implicit.hip and declarations to include/mfcd.h; scores_common.h, "
         "pairs_common.h and every existing translation unit are byte-identical to the parent's, so no existing entry was "
         "rebuilt from changed source")
    if "--parent-tree" in args:
        runs = int(args[args.index("--bench-runs") + 1]) if "--bench-runs" in args else 3
        for line in bench_lines(args[args.index("--parent-tree") + 1], runs):
            emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
