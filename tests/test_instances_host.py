"""CPU: the instance-extraction contract's numpy reference against scipy, and the host-only parts of the C ABI (shape queries, error
codes that must come back before any launch, exported names).  No GPU calls."""
import numpy as np
import pytest

from tests import _cc_reference as R

MU_OK, MU_ERR_ARG, MU_ERR_SHAPE, MU_ERR_WORKSPACE = 0, -1, -2, -4


@pytest.mark.parametrize("name", sorted(R.patterns()) + sorted(R.random_maps()))
def test_reference_agrees_with_scipy(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    g = R.patterns()[name] if name in R.patterns() else R.random_maps()[name][0]
    r = R.instances(g[None], None, 4096)
    ids = r["ids"][0]
    total = 0
    for c in np.unique(g):
        if c <= 0:
            continue
        lab, n = ndimage.label(g == c, structure=np.ones((3, 3)))
        total += n
        # same partition: every scipy component is exactly one instance of class c, numbered in the same (first pixel) order
        ours = [k for k in range(1, int(r["count"][0]) + 1) if r["table"][0, k - 1, 0] == c]
        assert len(ours) == n
        for j, k in enumerate(ours):
            assert np.array_equal(lab == j + 1, ids == k)
            assert r["table"][0, k - 1, 7] == j + 1                   # class_rank
            assert r["table"][0, k - 1, 1] == int((lab == j + 1).sum())
    assert r["count"][0] == total
    assert np.array_equal(ids > 0, g > 0)
    if name in R.EXPECTED_COUNTS:
        assert total == R.EXPECTED_COUNTS[name]


def test_reference_table_and_order_by_hand():
    g = np.array([[[1, 0, 2, 2], [0, 1, 0, 2], [3, 0, 0, 0]]], np.int32)
    p = np.array([[[.5, 0, .25, .25], [0, 1., 0, 1.], [.75, 0, 0, 0]]])
    r = R.instances(g, p, 4)
    assert r["ids"].tolist() == [[[1, 0, 2, 2], [0, 1, 0, 2], [3, 0, 0, 0]]]
    assert r["table"][0].tolist() == [[1, 2, 0, 0, 1, 1, 0, 1], [2, 3, 2, 0, 3, 1, 2, 1], [3, 1, 0, 2, 0, 2, 8, 1], [0] * 8]
    assert r["score"][0].tolist() == [0.75, 0.5, 0.75, 0.0]
    assert r["order"][0].tolist() == [1, 3, 2, 0]
    assert R.instances(g, None, 2)["count"][0] == 3 and R.class_rank_mask(g, 2).tolist() == [[[1, 0, 1, 1], [0, 1, 0, 1], [-1, 0, 0, 0]]]


def _lib():
    from maskunet_amd import _lib
    return _lib.load()


def test_supported_and_workspace_are_host_only_and_monotone():
    lib = _lib()
    assert lib.mu_instances_supported(128, 128, 1024) == MU_OK
    assert lib.mu_instances_supported(256, 256, 4096) == MU_OK
    assert lib.mu_instances_supported(1, 1, 1) == MU_OK
    prev = 0
    for B, H, W, K in [(1, 1, 1, 1), (1, 16, 16, 1), (1, 16, 16, 64), (2, 16, 16, 64), (2, 128, 128, 64), (2, 128, 128, 1024),
                       (64, 128, 128, 1024), (64, 256, 256, 1024), (64, 256, 256, 4096)]:
        n = lib.mu_instances_workspace_bytes(B, H, W, K)
        assert n > 0 and n >= prev
        prev = n


def test_more_than_65536_pixels_is_a_shape_error():
    lib = _lib()
    assert lib.mu_instances_supported(256, 257, 1024) == MU_ERR_SHAPE
    assert lib.mu_instances_supported(257, 256, 1024) == MU_ERR_SHAPE
    assert lib.mu_instances_supported(65536, 1, 1024) == MU_OK
    assert lib.mu_instances_supported(65537, 1, 1024) == MU_ERR_SHAPE


@pytest.mark.parametrize("max_inst", [0, 4097, -1])
def test_max_instances_out_of_range_is_a_shape_error(max_inst):
    lib = _lib()
    assert lib.mu_instances_supported(16, 16, max_inst) == MU_ERR_SHAPE
    # also from the entry point itself, with (never dereferenced) non-null pointers: the check precedes every HIP call
    fake = 4096
    assert lib.mu_instances(fake, None, 1, 16, 16, max_inst, fake, fake, fake, fake, fake, fake, 1 << 20, None) == MU_ERR_SHAPE
    assert lib.mu_instances(fake, None, 1, 256, 257, 16, fake, fake, fake, fake, fake, fake, 1 << 20, None) == MU_ERR_SHAPE


def test_null_pointers_and_bad_sizes_return_before_any_launch():
    lib = _lib()
    fake = 4096
    args = [fake, None, 1, 16, 16, 8, fake, fake, fake, fake, fake, fake, 1 << 20, None]
    for i in (0, 6, 7, 8, 9, 10, 11):
        a = list(args)
        a[i] = None
        assert lib.mu_instances(*a) == MU_ERR_ARG, i
    for i in (2, 3, 4):
        a = list(args)
        a[i] = 0
        assert lib.mu_instances(*a) == MU_ERR_ARG, i
    a = list(args)
    a[12] = lib.mu_instances_workspace_bytes(1, 16, 16, 8) - 1
    assert lib.mu_instances(*a) == MU_ERR_WORKSPACE
    assert lib.mu_argmax_prob(None, 16, 4, 16, 64, 16, 1, 2.0, fake, None, 0, None) == MU_ERR_ARG
    assert lib.mu_argmax_prob(fake, 16, 4, 16, 64, 16, 1, 2.0, None, None, 0, None) == MU_ERR_ARG
    assert lib.mu_argmax_prob(fake, 0, 4, 16, 64, 16, 1, 2.0, fake, None, 0, None) == MU_ERR_ARG
    assert lib.mu_argmax_prob(fake, 16, 0, 16, 64, 16, 1, 2.0, fake, None, 0, None) == MU_ERR_ARG
    assert lib.mu_argmax_prob(fake, 16, 4, 16, 64, 16, 1, 0.0, fake, None, 0, None) == MU_ERR_ARG
    assert lib.mu_argmax_prob(fake, 16, 4, 16, 64, 16, 1, 2.0, fake, None, 7, None) == MU_ERR_ARG


def test_names_are_exported():
    import maskunet_amd
    for n in ("predict_instances", "instances_from_labels", "generate_instance_mask"):
        assert n in maskunet_amd.__all__ and callable(getattr(maskunet_amd, n))
