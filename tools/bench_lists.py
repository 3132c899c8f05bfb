"""Diagnostic: time the Plackett–Luce list kernel and the ranked-list step (mfcd/lists.py; csrc/list_pl.hip) beside the same
loss and gradient by padded torch ops, and write the table to profiles/lists.txt (or --out PATH).

  ml100k    943 lists of 20 to 737 out of 1682 items, long-tailed as MovieLens 100k, fully ranked, d = 16
  slates    20 000 lists of 100 out of 20 000 items, fully ranked, d = 64: every row one tile
  catalogue 4 096 lists of the whole catalogue of 4 096 with depth 10, d = 64: every row 16 tiles, the carry passes

Per shape: the lane fill of the 256-entry tiles; ms per call of the scores, the kernel (value and gradient; gradient
alone), the two gather-sums and one fused step (fit_lists, Adam included); the same value and gradient in the scores by
torch (the lists padded to the longest, torch.logcumsumexp on the flipped matrix, autograd) in the same process; and the
largest difference of the kernel's g from the f64 model (np.logaddexp.accumulate in both directions on the same fp32
scores) in units of an fp32 rounding of g.

  bench     --parent-tree DIR (a built checkout of the parent commit): bench.py in both trees, taking turns, the order
            swapping from turn to turn

Timing as DESIGN 3.4: HIP events around >= SECONDS of back-to-back calls after an untimed stretch, two rounds, the
smaller one reported.  Usage: bench_lists.py [--out PATH] [--parent-tree DIR] [--bench-runs N]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "matrix-factorization-with-comparison-data_amd"), os.path.dirname(os.path.abspath(__file__))]
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_pair_ragged import long_tailed  # noqa: E402
from pair_bench_common import alternated, bench_lines  # noqa: E402
from mfcd import engine, lists as ML, ratings  # noqa: E402
import structure as S  # noqa: E402

dev = torch.device("cuda:0")
SECONDS = float(os.environ.get("PAIRS_BENCH_SECONDS", "0.5"))
PAD = -1.0e30                  # a padded score: exp(PAD - anything) is 0, and PAD - PAD is 0, not NaN


def model_g(a, L, stages):
    """The f64 model's g of rows of one length: a [rows, L] f64, stages per row."""
    lse = np.logaddexp.accumulate(a[:, ::-1], axis=1)[:, ::-1]
    staged = np.arange(L)[None, :] < stages[:, None]
    N = np.logaddexp.accumulate(np.where(staged, -lse, -np.inf), axis=1)
    return np.exp(a + N) - staged


def torch_form(a_pad, shown, staged):
    """Value and gradient in the padded scores by library ops."""
    x = a_pad.detach().requires_grad_(True)
    y = torch.where(shown, x, torch.full_like(x, PAD))
    lse = torch.logcumsumexp(y.flip(1), 1).flip(1)
    loss = torch.where(staged, lse - y, torch.zeros_like(y)).sum()
    return loss, torch.autograd.grad(loss, x)[0]


def shape_lines(name, lists, d, emit):
    model = S.MatrixFactorization(lists.n, lists.m, d).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    U, V = model.U.data, model.V.data
    a = ML.list_scores(U, V, lists)[0].mul_(4.0).contiguous()                   # a spread of a few units, as after a fit
    g = ML.pl_rows(a, lists, "grad")[2]
    binding = engine.AdamBinding(model, opt)
    ML.fit_lists(binding, lists, 2)                                             # untimed: the optimizer's state exists
    L = lists.lengths
    k = int(L.max())
    pos = torch.from_numpy(np.arange(lists.entries) - np.repeat(np.cumsum(L) - L, L)).to(dev)
    rows = lists.user.long()
    a_pad = torch.zeros((lists.n, k), device=dev)
    shown = torch.zeros((lists.n, k), dtype=torch.bool, device=dev)
    a_pad[rows, pos], shown[rows, pos] = a, True
    staged = torch.arange(k, device=dev)[None, :] < torch.from_numpy(lists.user_stages).to(dev)[:, None]
    calls = [lambda: ML.list_scores(U, V, lists), lambda: ML.pl_rows(a, lists, "both"), lambda: ML.pl_rows(a, lists, "grad"),
             lambda: ratings.ragged_gather_sum(g, lists, V, "user"), lambda: ratings.ragged_gather_sum(g, lists, U, "item"),
             lambda: ML.fit_lists(binding, lists, 1), lambda: torch_form(a_pad, shown, staged)]
    ms = alternated(calls)
    emit(f"{name}: {lists.n} lists over {lists.m} items, {lists.entries} entries, {lists.stages} stages, d = {d}; lengths "
         f"{L.min()} .. {L.max()} (median {int(np.median(L))}); tiles {lists.n_tiles}, lane fill "
         f"{lists.entries / (256.0 * max(lists.n_tiles, 1)):.3f}")
    emit(f"  ms per call: scores {ms[0]:.3f}, list kernel value and gradient {ms[1]:.3f} (gradient alone {ms[2]:.3f}), "
         f"gather-sum by user {ms[3]:.3f}, by item {ms[4]:.3f}; one fused step (fit_lists, Adam included) {ms[5]:.3f}; the "
         f"list kernel's share of the step {ms[2] / ms[5]:.2f}; {lists.entries / ms[1] / 1e6:.2f} G entries/s")
    loss_t, g_t = torch_form(a_pad, shown, staged)
    loss_k = ML.pl_rows(a, lists, "loss")[0].sum()
    emit(f"  the same value and gradient by padded ({lists.n} x {k}) torch.logcumsumexp and autograd: {ms[6]:.3f} ms "
         f"({ms[6] / ms[1]:.2f} x the kernel); loss {float(loss_t.detach()):.6e} against the kernel's {float(loss_k):.6e}, "
         f"largest difference of g {float((g_t[rows, pos] - g).abs().max()):.2e}")
    ah, gh, worst = a.cpu().numpy().astype(np.float64), g.cpu().numpy(), 0.0
    off = lists.row_off.cpu().numpy()
    for length in np.unique(L[L > 0]):                                          # the model, the rows of one length at a time
        sel = np.flatnonzero(L == length)
        idx = off[sel][:, None] + np.arange(length)[None, :]
        want = model_g(ah[idx], int(length), lists.user_stages[sel])
        big = np.abs(want) >= 1e-3                                              # below, the model's own error shows
        worst = max(worst, float((np.abs(gh[idx] - want)[big] / (np.abs(want[big]) * 2.0 ** -24)).max(initial=0.0)))
    emit(f"  largest |g - f64 model| over |g| >= 1e-3 in units of 2^-24 |g| (<= 1: a correctly rounded g): {worst:.3f}")


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "lists.txt")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
    lines = [f"# {torch.cuda.get_device_name(0)}; python tools/bench_lists.py: >= {SECONDS} s per stretch after an untimed "
             "stretch, min of two rounds, the forms taking turns (HIP events); no counters taken"]
    print(lines[0], flush=True)

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(0)
    n, m = 943, 1682
    L = long_tailed(n, 100000, 20, 737, rng)
    items = np.concatenate([rng.choice(m, k, replace=False) for k in L])
    position = np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)
    shape_lines("ml100k-shaped", ML.RankedLists(np.repeat(np.arange(n), L), items, position, n, m).to(dev), 16, emit)
    n = m = 20000
    coprime = np.array([s for s in range(1, 200) if np.gcd(s, m) == 1])       # 100 steps stay below m: distinct items
    start, step = rng.integers(0, m, n), coprime[rng.integers(0, coprime.size, n)]
    items = (start[:, None] + step[:, None] * np.arange(100)[None, :]) % m
    users, position = np.repeat(np.arange(n), 100), np.tile(np.arange(100), n)
    shape_lines("slates of 100", ML.RankedLists(users, items.reshape(-1), position, n, m).to(dev), 64, emit)
    n = m = 4096
    items = np.argsort(rng.random((n, m)), axis=1)
    users, position = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
    shape_lines("full catalogue, depth 10", ML.RankedLists(users, items.reshape(-1), position, n, m, depth=10).to(dev), 64, emit)
    if "--parent-tree" in args:
        runs = int(args[args.index("--bench-runs") + 1]) if "--bench-runs" in args else 3
        for line in bench_lines(args[args.index("--parent-tree") + 1], runs, swap=True):
            emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
