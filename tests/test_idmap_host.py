"""CPU: the id-map instance contract's numpy restatement (tests/_idmap_reference.py) against the reference's own
get_instance_annotations (golden vectors, tests/golden/idmap) and against hand-worked medians, and the host-only parts of the C ABI and
of the Python wrapper (shape queries, error codes that must come back before any launch, exported names).  No GPU calls."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import _cc_reference as CC
from tests import _idmap_reference as R

MU_OK, MU_ERR_ARG, MU_ERR_SHAPE, MU_ERR_WORKSPACE = 0, -1, -2, -4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idmap")


def check_against_golden(got, g, b=0):
    """got: one side (numpy dict); g: a golden file.  Annotation k of the reference is id k + 1."""
    n = len(g["category_id"])
    assert got["count"][b] == n
    assert np.array_equal(got["ids"][b], g["masks"])
    t = got["table"][b, :n]
    assert np.array_equal(t[:, 0], g["category_id"])
    assert np.array_equal(t[:, 1], g["area"])
    bbox = np.stack([t[:, 2], t[:, 3], t[:, 4] - t[:, 2], t[:, 5] - t[:, 3]], 1).astype(np.float64)      # the reference's: no + 1
    assert np.array_equal(bbox, g["bbox"])
    assert (got["table"][b, n:] == 0).all() and got["invalid"][b] == 0


def golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def test_goldens_are_present():
    assert golden_names() == sorted(R.GOLDEN)


@pytest.mark.parametrize("name", sorted(R.GOLDEN))
def test_restatement_equals_the_reference(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    id_map, sem = R.GOLDEN[name]()
    assert np.array_equal(id_map, g["id_map"]) and np.array_equal(sem, g["sem"]), "the generator and the stored inputs differ"
    check_against_golden(R.instances(g["id_map"], g["sem"], 64, 256), g)


def test_medians_by_hand():
    v, sem, M, cap = R.cases()["median_by_hand"]
    r = R.instances(v, sem, M, cap)
    assert r["count"][0] == 5
    assert r["table"][0, :5, 0].tolist() == R.MEDIAN_BY_HAND == [13, 129, 127, 255, 4]
    assert r["table"][0, :5, 1].tolist() == [4, 2, 4, 1, 3]
    assert r["table"][0, :5, 7].tolist() == [1, 1, 1, 1, 1]
    for k in range(5):                                         # the contract's formula is int(np.median(..))
        assert r["table"][0, k, 0] == int(np.median(sem[0][v[0] == k + 1]))


def test_numbering_values_ranks_and_dropped_pixels_by_hand():
    v = np.array([[[-3, 0, 5, -1], [2, 2, 0, -3]]], np.int64)
    sem = np.array([[[1, 1, 1, 1], [2, 1, 1, 1]]], np.int32)
    r = R.instances(v, sem, 3, 19)
    assert r["ids"].tolist() == [[[1, 0, 4, 2], [3, 3, 0, 1]]] and r["count"][0] == 4
    assert r["values"][0].tolist() == [-3, -1, 2]
    assert r["table"][0].tolist() == [[1, 2, 0, 0, 3, 1, 0, 1], [1, 1, 3, 0, 3, 0, 3, 2], [1, 2, 0, 1, 1, 1, 4, 3]]     # {1,2} -> 1
    assert r["score"][0].tolist() == [1.0, 1.0, 1.0] and r["order"][0].tolist() == [1, 2, 3]
    sem[0, 0, 0], sem[0, 0, 1] = 19, -1                        # drops one pixel of -3; the zero pixel is not an error
    r = R.instances(v, sem, 8, 19)
    assert r["ids"].tolist() == [[[0, 0, 4, 2], [3, 3, 0, 1]]] and r["invalid"][0] == 1
    assert r["table"][0, 0].tolist() == [1, 1, 3, 1, 3, 1, 7, 1]
    v[0, 0, 2] = 2 ** 31
    r = R.instances(v, sem, 8, 19)
    assert r["ids"].tolist() == [[[0, 0, 0, 2], [3, 3, 0, 1]]] and r["invalid"][0] == 3 and r["count"][0] == 3


def test_connected_components_are_a_different_partition():
    """why the producer is needed: two touching cars are one component, a car in two pieces is two"""
    v, sem = R.touching_and_split()
    by_id = R.instances(v, sem, 8, 2)
    by_component = CC.instances(sem, None, 8)
    assert by_id["count"][0] == 3 and by_component["count"][0] == 3      # equal by accident of the scene: 2 + 1 against 1 + 2
    assert sorted(by_id["table"][0, :3, 1].tolist()) == [30, 30, 36]
    assert sorted(by_component["table"][0, :3, 1].tolist()) == [16, 20, 60]
    v[0, 10:14, 7:12] = 0                                      # without the second piece the counts differ too
    sem = (v != 0).astype(np.int32)
    assert R.instances(v, sem, 8, 2)["count"][0] == 3 and CC.instances(sem, None, 8)["count"][0] == 2


def _lib():
    from maskunet_amd import _lib
    return _lib.load()


def test_supported_limits():
    lib = _lib()
    assert lib.mu_id_instances_supported(1, 1, 1, 1) == MU_OK
    assert lib.mu_id_instances_supported(256, 256, 4096, 1024) == MU_OK
    assert lib.mu_id_instances_supported(65536, 1, 1024, 256) == MU_OK
    for bad in [(256, 257, 16, 19), (65537, 1, 16, 19), (0, 4, 16, 19), (4, 0, 16, 19), (4, 4, 0, 19), (4, 4, 4097, 19), (4, 4, 16, 0),
                (4, 4, 16, 1025), (4, 4, -1, 19), (4, 4, 16, -1)]:
        assert lib.mu_id_instances_supported(*bad) == MU_ERR_SHAPE, bad
        assert lib.mu_id_instances_workspace_bytes(1, *bad) == 0, bad


def test_workspace_query_is_positive_a_multiple_of_four_and_monotone():
    lib = _lib()
    prev = 0
    for B, H, W, M, C in [(1, 1, 1, 1, 1), (1, 16, 16, 1, 19), (1, 16, 16, 64, 19), (2, 16, 16, 64, 19), (2, 128, 128, 64, 19),
                          (2, 128, 128, 1024, 256), (64, 128, 128, 1024, 256), (64, 256, 256, 4096, 1024)]:
        n = lib.mu_id_instances_workspace_bytes(B, H, W, M, C)
        assert n > 0 and n % 4 == 0 and n >= prev
        prev = n
    assert lib.mu_id_instances_workspace_bytes(0, 16, 16, 8, 19) == 0


def test_null_pointers_and_bad_sizes_return_before_any_launch():
    lib = _lib()
    fake = 4096
    args = [fake, 0, fake, 1, 16, 16, 8, 19] + [fake] * 8 + [1 << 24, None]
    for i in (0, 2, 8, 9, 10, 11, 12, 13, 14, 15):
        a = list(args)
        a[i] = None
        assert lib.mu_id_instances(*a) == MU_ERR_ARG == -1, i
    for i in (3, 4, 5):
        a = list(args)
        a[i] = 0
        assert lib.mu_id_instances(*a) == MU_ERR_ARG, i
    for kind in (-1, 3):
        a = list(args)
        a[1] = kind
        assert lib.mu_id_instances(*a) == MU_ERR_ARG, kind
    for i, val in [(6, 0), (6, 4097), (7, 0), (7, 1025), (4, 65537)]:
        a = list(args)
        a[i] = val
        assert lib.mu_id_instances(*a) == MU_ERR_SHAPE, (i, val)
    a = list(args)
    a[16] = lib.mu_id_instances_workspace_bytes(1, 16, 16, 8, 19) - 1
    assert lib.mu_id_instances(*a) == MU_ERR_WORKSPACE


def test_wrapper_argument_errors():
    import maskunet_amd
    f = maskunet_amd.instances_from_id_map
    v, c = torch.zeros((1, 4, 4), dtype=torch.int64), torch.zeros((1, 4, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="on the GPU"):
        f(v, c)
    with pytest.raises(RuntimeError, match="on the GPU"):
        f(v.numpy(), c)


def test_names_are_exported_and_instances_keeps_its_positional_form():
    import maskunet_amd
    assert "instances_from_id_map" in maskunet_amd.__all__ and callable(maskunet_amd.instances_from_id_map)
    t = torch.zeros(1)
    old = maskunet_amd.Instances(t, t, t, t, t, t)
    assert old.prob is None and old.values is None and old.invalid is None
    assert maskunet_amd.Instances(t, t, t, t, t, t, t).values is None
    from maskunet_amd import _lib
    assert (_lib.MU_IDMAP_I32, _lib.MU_IDMAP_I64, _lib.MU_IDMAP_RGB8) == (0, 1, 2)
