"""CPU-only checks of the cluster strategy's host side (mfcd/cluster.py, mfcd/sampling.py: group_tables, the factored
forms of generation_data.py): the C entry points are declared and bound and refuse bad sizes before anything is launched,
the group tables are built and validated on the host, and a FactoredMatrix is taken by the variance and cluster samplers
through d x d forms of its factors."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

KMEANS_ENTRIES = ("mfcd_kmeans_max_k", "mfcd_kmeans_workspace_bytes", "mfcd_kmeans_assign", "mfcd_kmeans_update")


def test_kmeans_entry_points_and_groups_law_are_declared_and_bound():
    from mfcd import _lib, sampling
    header = open(os.path.join(ROOT, "include", "mfcd.h")).read()
    for name in KMEANS_ENTRIES:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
    assert re.search(r"#define MFCD_LAW_GROUPS 3\b", header)
    assert re.search(r"#define MFCD_ABI_VERSION 4\b", header)
    assert _lib.load().mfcd_abi_version() == 4
    assert sampling.LAW_GROUPS == 3 and "cluster" in sampling.DEVICE_STRATEGIES


def test_kmeans_entries_refuse_sizes_out_of_range():
    from mfcd import _lib
    L = _lib.load()
    kmax = L.mfcd_kmeans_max_k()
    assert kmax >= 64
    assert L.mfcd_kmeans_workspace_bytes(1000, 70, 20) > 0
    assert L.mfcd_kmeans_workspace_bytes(4194304, 64, kmax) > 0
    assert L.mfcd_kmeans_workspace_bytes(65536, 64, 20) <= 128 << 20
    buf = torch.zeros(4096, dtype=torch.uint8)               # host memory: never touched, the sizes are refused first
    p = buf.data_ptr()
    for P, dim, k in ((10, 3, 0), (100, 3, kmax + 1), (10, 0, 2), (0, 3, 2), (4194305, 3, 2), (10, 3, -1)):
        assert L.mfcd_kmeans_workspace_bytes(P, dim, k) == 0, (P, dim, k)
        assert L.mfcd_kmeans_assign(p, P, dim, p, k, p, None, None, p, 4096, None) == -1, (P, dim, k)
        assert L.mfcd_kmeans_update(p, P, dim, p, k, p, p, p, 4096, None) == -1, (P, dim, k)
    assert L.mfcd_kmeans_assign(None, 10, 3, None, 2, None, None, None, None, 0, None) == -1
    assert L.mfcd_kmeans_update(None, 10, 3, None, 2, None, None, None, 0, None) == -1


def test_group_tables():
    from mfcd import sampling
    labels = [2, 0, 2, 1, 2, 0, 2, 2, 1]
    members, offsets = sampling.group_tables(labels, 3)
    assert members.dtype == torch.int32 and offsets.dtype == torch.int32
    assert members.tolist() == [1, 5, 3, 8, 0, 2, 4, 6, 7] and offsets.tolist() == [0, 2, 4, 9]
    members, offsets = sampling.group_tables(torch.tensor(labels, dtype=torch.int32), 3)
    assert members.tolist() == [1, 5, 3, 8, 0, 2, 4, 6, 7] and offsets.tolist() == [0, 2, 4, 9]
    with pytest.raises(ValueError):
        sampling.group_tables(labels, 4)                     # group 3 is empty
    with pytest.raises(ValueError):
        sampling.group_tables([0, 1, 3], 3)                  # label >= k
    with pytest.raises(ValueError):
        sampling.group_tables([0, -1, 1], 2)


def _factored(n, m, dx, seed):
    import generation_data as gd
    g = torch.Generator().manual_seed(seed)
    return gd.FactoredMatrix(torch.randn(n, dx, generator=g) + 0.5, torch.randn(m, dx, generator=g))


def test_factored_variance_matches_the_dense_variance():
    import generation_data as gd
    FX = _factored(500, 80, 6, 0)
    got = gd._factored_column_variances(FX)
    want = torch.var(FX.A @ FX.B.t(), dim=0).double()
    assert got.dtype == torch.float64 and got.shape == (80,)
    rel = float(((got - want).abs() / want).max())
    assert rel <= 1e-5, rel


def test_item_points_of_factors_keep_the_columns_distances():
    from mfcd import cluster
    FX = _factored(500, 80, 6, 1)
    pts = cluster.item_points(FX, "cpu")
    assert pts.dtype == torch.float32 and pts.shape == (80, 6) and pts.is_contiguous()
    cols = (FX.A.double() @ FX.B.double().t()).t()
    want, got = torch.cdist(cols, cols), torch.cdist(pts.double(), pts.double())
    off = ~torch.eye(80, dtype=torch.bool)
    rel = float(((got - want).abs()[off] / want[off]).max())
    assert rel <= 1e-5, rel
    dense = torch.randn(7, 5)
    assert torch.equal(cluster.item_points(dense, "cpu"), dense.t().contiguous())
    # factors without full column rank: the Gram form still has a square root
    A = torch.randn(50, 3)
    low = _factored(50, 20, 4, 2)
    low.A = torch.cat((A, A[:, :1]), dim=1).contiguous()
    cols = (low.A.double() @ low.B.double().t()).t()
    pts = cluster.item_points(low, "cpu").double()
    assert float((torch.cdist(pts, pts) - torch.cdist(cols, cols)).abs().max()) <= 1e-4 * float(torch.cdist(cols, cols).max())


def test_host_variance_and_cluster_samplers_take_a_factored_matrix():
    import generation_data as gd
    from mfcd import cluster
    from sklearn.cluster import KMeans
    n, m, dx = 300, 40, 4
    g = torch.Generator().manual_seed(5)
    centres = 30.0 * torch.randn(4, dx, generator=g)
    B = centres[torch.arange(m) % 4] + 0.1 * torch.randn(m, dx, generator=g)       # four well separated item groups
    FX = gd.FactoredMatrix(torch.randn(n, dx, generator=g), B)
    torch.manual_seed(0)
    np.random.seed(0)
    for name, rows in (("variance", gd.choose_items_by_variance(FX, 400, set())),
                       ("cluster", gd.choose_items_cluster_based(FX, 400, set(), n_clusters=4))):
        assert len(rows) == 400 and len(set(rows)) == 400, name
        r = np.asarray(rows)
        assert (r[:, 1] != r[:, 2]).all() and r.min() >= 0 and r[:, 0].max() < n and r[:, 1:].max() < m, name
        if name == "cluster":
            labels = KMeans(n_clusters=4, n_init="auto", random_state=0).fit_predict(cluster.item_points(FX, "cpu").numpy())
            assert len(set(labels.tolist())) == 4 and (labels[r[:, 1]] != labels[r[:, 2]]).all()
