"""GPU tests of what the row kernels' host code shares (mfcd/_lib.py: workspace; mfcd/rows.py): one scratch buffer per
(device, stream) that every module's kernels take in turn, and the slab loop of the factored UV^T pass.

Every kernel called here documents that two calls are bit-equal, so every comparison is exact.  Shapes: pair statistics
at m = 1025 (two column tiles: the diagonal and the off-diagonal path); top-k over factors with ragged n, m, d;
the long Spearman form one column past the LDS kernel's limit; k-means at ragged sizes and at dim = 256 (the deep
assignment kernel)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mfcd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_workspace_is_one_growing_buffer_per_device_and_stream(dev):
    from mfcd import _lib
    first = _lib.workspace(1000, dev)
    assert first.dtype == torch.uint8 and first.device == dev and first.numel() >= 1000
    assert _lib.workspace(10, dev).data_ptr() == first.data_ptr()            # a smaller request: the same buffer
    assert _lib.workspace(10, "cuda").data_ptr() == first.data_ptr()         # the current device by another name
    grown = _lib.workspace(first.numel() + 1, dev)
    assert grown.numel() > first.numel()
    assert _lib.workspace(1, dev).data_ptr() == grown.data_ptr() and grown.data_ptr() % 256 == 0
    s2 = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s2):
        other = _lib.workspace(10, dev)
        assert other.numel() >= 256                                          # the floor
        assert _lib.workspace(256, dev).data_ptr() == other.data_ptr()
    assert other.data_ptr() != grown.data_ptr()                              # both alive: not one block handed out twice
    assert _lib.workspace(1, dev).data_ptr() == grown.data_ptr()             # back on the first stream


def test_row_pair_on_strided_and_single_row_views(dev):
    """`_lib.row_pair` on real GPU views, and the kernels behind it: a [3, 2 m] tensor cut to [:, :m] goes in as a view with
    lda = 2 m, one row of it with lda = m, a column-strided view as a copy; every result equals the contiguous copy's."""
    from mfcd import _lib, metrics, pairs
    m = 1025
    g = torch.Generator().manual_seed(6)
    wide, X = torch.randn(3, 2 * m, generator=g).to(dev), torch.randn(3, m, generator=g).to(dev)
    a, x, rows, cols, lda, ldx = _lib.row_pair(wide[:, :m], X, "test")
    assert (rows, cols, lda, ldx) == (3, m, 2 * m, m) and a.data_ptr() == wide.data_ptr()
    assert _lib.row_pair(wide[1:2, :m], X[1:2], "test")[2:] == (1, m, m, m)
    a, x, rows, cols, lda, ldx = _lib.row_pair(wide[:, ::2], X, "test")
    assert (lda, ldx) == (m, m) and a.is_contiguous()
    for view, truth in ((wide[:, :m], X), (wide[1:2, :m], X[1:2]), (wide[:, ::2], X)):
        flat = view.contiguous()
        for fn in (lambda p, q: pairs.pair_stats_rows(p, q, 0.5, "both"), lambda p, q: (pairs.pair_grad_rows(p, q, 0.5),),
                   lambda p, q: (metrics.spearman_rows(p, q),), lambda p, q: (metrics.spearman_rows_long(p, q),)):
            for got, want in zip(fn(view, truth), fn(flat, truth)):
                assert torch.equal(got, want)
    with pytest.raises(_lib.MfcdError, match="no CPU fallback"):
        _lib.row_pair(wide[:, :m], X.cpu(), "test")


def _calls(dev):
    """name -> a call returning a tuple of tensors; inputs are made once, here."""
    from mfcd import cluster, metrics, pairs, topk
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev)           # noqa: E731
    pa, px = rnd(3, 1025), rnd(3, 1025)
    fa, fb = rnd(5, 33), rnd(129, 33)
    sa, sx = rnd(2, 20449), rnd(2, 20449)
    kms = [(rnd(129, 33), rnd(33, 33)), (rnd(40, 256), rnd(5, 256))]

    def km(pts, C):
        C = C.clone()                                                       # update writes the centres in place
        labels, d2 = cluster.assign(pts, C, dist2=True)
        return labels, d2, cluster.update(pts, labels, C), C

    both = lambda r: (r[0][0], r[0][1], r[1][0], r[1][1])                   # noqa: E731
    return {
        "pair_stats_rows": lambda: pairs.pair_stats_rows(pa, px, 0.5, "both"),
        "topk_rows": lambda: both(topk.topk_rows((fa, fb), 5, ends="both", values=True)),
        "spearman_rows_long": lambda: (metrics.spearman_rows_long(sa, sx),),
        "kmeans 129x33 k33": lambda: km(*kms[0]),
        "kmeans 40x256 k5": lambda: km(*kms[1]),
        "pair_stats_rows again": lambda: pairs.pair_stats_rows(pa, px, 0.5, "both"),
    }


def test_kernels_that_share_the_scratch_buffer_leave_nothing_behind(dev):
    from mfcd import _lib
    calls = _calls(dev)
    _lib._workspaces.clear()
    chained = {name: [t.clone() for t in call()] for name, call in calls.items()}     # one buffer, taken in turn
    torch.cuda.synchronize()
    assert len(_lib._workspaces) == 1
    for a, b in zip(chained["pair_stats_rows"], chained["pair_stats_rows again"]):
        assert torch.equal(a, b)
    for name in reversed(list(calls)):                                                 # alone: a fresh buffer each
        _lib._workspaces.clear()
        for q, (a, b) in enumerate(zip(chained[name], calls[name]())):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, q)   # bits: NaN too


def test_factored_uvt_pass_is_its_slabs_in_order(dev):
    """uvt_stats_factored at n = 70, slab_rows = 32 (a ragged last slab) against the library called slab by slab here:
    X's rows from A[r0:r1] @ B^T, the global sums added in slab order in f64."""
    import generation_data as gd
    from mfcd import _lib, metrics
    L = _lib.load()
    n, m, d, slab = 70, 130, 8, 32
    g = torch.Generator().manual_seed(9)
    U, V = torch.randn(n, d, generator=g).to(dev), torch.randn(m, d, generator=g).to(dev)
    FX = gd.FactoredMatrix(torch.randn(n, 3, generator=g), torch.randn(m, 3, generator=g))
    A, B = FX.A.to(dev), FX.B.to(dev)
    rows = torch.empty((n, 8), dtype=torch.float64, device=dev)
    scal = torch.zeros(4, dtype=torch.float64, device=dev)
    share = torch.empty(4, dtype=torch.float64, device=dev)
    ws = torch.empty(L.mfcd_uvt_slab_workspace_bytes(n, m, d, slab), dtype=torch.uint8, device=dev)
    for r0 in range(0, n, slab):
        r1 = min(n, r0 + slab)
        Xs = (A[r0:r1] @ B.t()).contiguous()
        _lib.check(L.mfcd_uvt_stats_slab(U.data_ptr(), V.data_ptr(), Xs.data_ptr(), n, m, d, 0.9, 3, r0, r1 - r0,
                                         rows[r0:r1].data_ptr(), share.data_ptr(), ws.data_ptr(), ws.numel(),
                                         ctypes.c_void_p(_lib.stream_ptr(dev))))
        scal += share
    got_rows, got_scal = metrics.uvt_stats_factored(U, V, FX, 0.9, what=3, slab_rows=slab)
    assert torch.equal(got_rows[:, :6], rows[:, :6])                  # the columns in use (include/mfcd.h); none is NaN
    assert torch.equal(got_scal, scal)
    only = metrics.uvt_stats_factored(U, V, FX, 0.9, what=2, slab_rows=slab)
    assert only[0] is None and only[1].shape == (4,)
