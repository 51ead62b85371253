"""CPU: the embedding-instance contract's numpy restatement (tests/_dbscan_reference.py) against the goldens that the reference's own
get_instances_from_embeddings / get_instance_annotations produced with sklearn (tests/golden/make_golden_dbscan.py), and the host-only
parts of the C ABI: shape queries, error codes that must come back before any launch, exported names.  No GPU calls."""
import glob
import os

import numpy as np
import pytest

from tests import _dbscan_reference as R
from tests.conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "dbscan")          # tests/golden/*.npz itself is globbed as module cases
MU_OK, MU_ERR_ARG, MU_ERR_SHAPE, MU_ERR_WORKSPACE = 0, -1, -2, -4
GOLDENS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "dbscan_*.npz")))


def test_goldens_are_present():
    assert len(GOLDENS) >= 3


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_equals_the_reference(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    nc, eps, ms = int(g["num_classes"]), float(g["eps"]), int(g["min_samples"])
    assert float(g["margin"]) > 1e-6                       # no pair near enough to the threshold for sklearn's arithmetic to matter
    assert abs(R.margin(g["cls"], g["emb"], nc, eps) - float(g["margin"])) <= 1e-12
    cov = R.rule_coverage(g["cls"], g["emb"], nc, eps, ms)
    assert cov["noise"] and cov["small_class"] and cov["two_clusters"] and cov["shared_border"], cov
    r = R.instances(g["cls"][None], g["emb"][None], nc, eps, ms, 64)
    assert np.array_equal(r["ids"][0], g["ids"])
    ann = R.annotations(r["ids"][0], g["cls"])
    assert len(ann) == len(g["score"]) == int(r["count"][0])
    for k, (bbox, cat, score) in enumerate(ann):
        assert bbox == g["bbox"][k].tolist() and cat == int(g["category_id"][k]) and score == float(g["score"][k]) == 1.0
        row = r["table"][0, k]                            # the table says the same
        assert row[0] == cat and [row[2], row[3], row[4] - row[2], row[5] - row[3]] == bbox
    assert np.array_equal(r["order"][0, :len(ann)], np.arange(1, len(ann) + 1))


def test_restatement_by_hand():
    """1-D points, eps 0.5: results worked out by hand in the comments"""
    #   pixel      0     1     2     3     4     5     6     7
    x = np.array([1.0, 0.0, 0.5, 5.0, 0.25, 2.0, 1.5, 9.0])
    cls = np.array([[1, 1, 1, 1, 1, 1, 1, 2]])
    # neighbour counts (|a - b| <= 0.5): 1.0:{1.0,0.5,1.5}=3 core; 0.0:{0,0.5,0.25}=3 core; 0.5:{1.0,0,0.5,0.25}=4 core; 5.0: 1 noise;
    # 0.25:{0,0.5,0.25}=3 core; 2.0:{2.0,1.5}=2 border of 1.5's cluster; 1.5:{1.0,2.0,1.5}=3 core.  All cores are chained: one cluster.
    ids = R.label_image(cls, x.reshape(1, 8, 1), 3, 0.5, 3)
    assert ids.tolist() == [[1, 1, 1, 0, 1, 1, 1, 0]]
    # min_samples 4: only 0.5 is core; 1.0, 0.0, 0.25 are its border points; 1.5, 2.0, 5.0 are noise
    ids = R.label_image(cls, x.reshape(1, 8, 1), 3, 0.5, 4)
    assert ids.tolist() == [[1, 1, 1, 0, 1, 0, 0, 0]]
    r = R.instances(cls[None], x.reshape(1, 1, 8, 1), 3, 0.5, 4, 2)
    assert r["table"][0].tolist() == [[1, 4, 0, 0, 4, 0, 0, 1], [0] * 8] and r["count"].tolist() == [1]
    # a shared border point goes to the cluster with the lower first core point, and a cluster's first pixel may be a border point
    # (0.85 has three neighbours with itself -- 0.4 and 1.3, both core -- and min_samples is 4)
    x = np.array([0.85, 0.0, 0.0, 0.0, 0.4, 1.3, 1.7, 1.7, 1.7])
    ids = R.label_image(np.ones((1, 9), np.int32), x.reshape(1, 9, 1), 2, 0.5, 4)
    assert ids.tolist() == [[1, 1, 1, 1, 1, 2, 2, 2, 2]]
    ids = R.label_image(np.ones((1, 9), np.int32), (1.7 - x).reshape(1, 9, 1), 2, 0.5, 4)
    assert ids.tolist() == [[1, 1, 1, 1, 1, 2, 2, 2, 2]]


def _lib():
    from maskunet_amd import _lib
    return _lib.load()


def test_entry_points_are_in_the_binding_table_and_exported():
    import maskunet_amd
    from maskunet_amd import _lib
    for n in ("mu_dbscan_workspace_bytes", "mu_dbscan_supported", "mu_dbscan_instances"):
        assert n in _lib.SIGNATURES and hasattr(_lib.load(), n)
    assert len(_lib.SIGNATURES["mu_dbscan_instances"][1]) == 23
    assert "instances_from_embeddings" in maskunet_amd.__all__ and callable(maskunet_amd.instances_from_embeddings)


def test_supported_and_workspace_are_host_only_and_monotone():
    lib = _lib()
    assert lib.mu_dbscan_supported(128, 128, 16, 19, 1024) == MU_OK
    assert lib.mu_dbscan_supported(256, 256, 64, 1024, 4096) == MU_OK
    assert lib.mu_dbscan_supported(1, 1, 1, 1, 1) == MU_OK
    prev = 0
    for B, H, W, C, K in [(1, 1, 1, 1, 1), (1, 16, 16, 2, 1), (1, 16, 16, 19, 64), (2, 16, 16, 19, 64), (2, 128, 128, 19, 64),
                          (2, 128, 128, 150, 1024), (64, 128, 128, 150, 1024), (64, 256, 256, 1024, 4096)]:
        n = lib.mu_dbscan_workspace_bytes(B, H, W, C, K)
        assert n > 0 and n % 4 == 0 and n >= prev
        prev = n
    assert lib.mu_dbscan_workspace_bytes(0, 16, 16, 19, 64) == 0
    assert lib.mu_dbscan_workspace_bytes(1, 256, 257, 19, 64) == 0


@pytest.mark.parametrize("args", [(256, 257, 16, 19, 64), (65537, 1, 16, 19, 64), (0, 16, 16, 19, 64), (16, 16, 0, 19, 64),
                                  (16, 16, 65, 19, 64), (16, 16, 16, 0, 64), (16, 16, 16, 1025, 64), (16, 16, 16, 19, 0),
                                  (16, 16, 16, 19, 4097)])
def test_limits_are_shape_errors(args):
    lib = _lib()
    H, W, D, C, K = args
    assert lib.mu_dbscan_supported(*args) == MU_ERR_SHAPE
    if H > 0 and W > 0:
        # also from the entry point itself, with (never dereferenced) non-null pointers: the check precedes every HIP call
        fake = 4096
        assert lib.mu_dbscan_instances(fake, fake, 1, H, W, D, H * W, D * H * W, H * W, 1, 0, C, 0.5, 5, K, fake, fake, fake, fake,
                                       fake, fake, 1 << 30, None) == MU_ERR_SHAPE


def test_null_pointers_and_bad_arguments_return_before_any_launch():
    lib = _lib()
    fake = 4096
    args = [fake, fake, 1, 16, 16, 16, 256, 4096, 256, 1, 0, 19, 0.5, 5, 8, fake, fake, fake, fake, fake, fake, 1 << 20, None]
    for i in (0, 1, 15, 16, 17, 18, 19, 20):
        a = list(args)
        a[i] = None
        assert lib.mu_dbscan_instances(*a) == MU_ERR_ARG, i
    for i in (2, 3, 4, 6):                                 # B, H, W, inner
        a = list(args)
        a[i] = 0
        assert lib.mu_dbscan_instances(*a) == MU_ERR_ARG, i
    a = list(args)
    a[10] = 7                                              # dtype
    assert lib.mu_dbscan_instances(*a) == MU_ERR_ARG
    for i, v in ((12, 0.0), (12, -1.0), (13, 0), (13, -3)):                      # eps, min_samples
        a = list(args)
        a[i] = v
        assert lib.mu_dbscan_instances(*a) == MU_ERR_SHAPE, (i, v)
    a = list(args)
    a[21] = lib.mu_dbscan_workspace_bytes(1, 16, 16, 19, 8) - 1
    assert lib.mu_dbscan_instances(*a) == MU_ERR_WORKSPACE


def test_cpu_tensors_raise():
    import torch
    import maskunet_amd
    with pytest.raises(RuntimeError):
        maskunet_amd.instances_from_embeddings(torch.zeros(1, 8, 8, dtype=torch.int64), torch.zeros(1, 4, 8, 8), num_classes=3)
