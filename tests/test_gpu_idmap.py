"""GPU: ground-truth instances from dataset id maps (mu_id_instances, maskunet_amd.instances_from_id_map) against the numpy restatement
of the contract in tests/_idmap_reference.py and the golden vectors of the reference's get_instance_annotations.  The path has no
floating-point result: ids, counts, values, invalid bits, every table column, scores and order are compared with ==.  Memory
discipline as in test_gpu_instances.py: outputs pre-filled with a sentinel, the workspace exactly the queried size, 4 KiB guard bands
around every buffer, inputs verified untouched."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _idmap_reference as R
from tests._device_buffers import Guarded, call, side_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_KEYS = ("ids", "table", "score", "count", "order", "values", "invalid")
KIND = {"i32": (0, torch.int32), "i64": (1, torch.int64), "rgb8": (2, torch.uint8)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idmap")


def run(id_map, sem, max_inst, class_cap, kind="i64"):
    """raw mu_id_instances on numpy inputs -> dict of numpy outputs; checks guards and untouched inputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, H, W = sem.shape
    code, dtype = KIND[kind]
    if kind == "i32":
        assert ((id_map >= R.I32_MIN) & (id_map <= R.I32_MAX)).all()
    g_map = Guarded(id_map.size, dtype, id_map, "id map")
    g_sem = Guarded(sem.size, torch.int32, sem, "semantic map")
    shapes = {"ids": ((B, H, W), torch.int32), "table": ((B, max_inst, 8), torch.int32), "score": ((B, max_inst), torch.float32),
              "count": ((B,), torch.int32), "order": ((B, max_inst), torch.int32), "values": ((B, max_inst), torch.int32),
              "invalid": ((B,), torch.int32)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    assert lib.mu_id_instances_supported(H, W, max_inst, class_cap) == 0
    nws = lib.mu_id_instances_workspace_bytes(B, H, W, max_inst, class_cap)
    assert nws > 0 and nws % 4 == 0
    call("mu_id_instances", g_map, code, g_sem, B, H, W, max_inst, class_cap, *[outs[k] for k in OUT_KEYS],
         Guarded(nws // 4, torch.int32, name="workspace"), nws)
    for k in OUT_KEYS:
        outs[k].all_written()
    return {k: outs[k].host(shapes[k][0]) for k in OUT_KEYS}


def same(got, ref):
    print(f"count {got['count'].tolist()} (reference {ref['count'].tolist()}), invalid {got['invalid'].tolist()}")
    for k in OUT_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
    for j, col in enumerate(("class", "area", "x_min", "y_min", "x_max", "y_max", "first_pixel", "class_rank")):
        assert np.array_equal(got["table"][:, :, j], ref["table"][:, :, j]), f"table column {col}"
    for k in OUT_KEYS:
        assert np.array_equal(got[k], ref[k]), k


@functools.lru_cache(maxsize=None)
def _cases():
    out = R.cases()
    for v, sem, _, _ in out.values():
        v.setflags(write=False)
        sem.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    v, sem, M, cap = _cases()[name]
    ref = R.instances(v, sem, M, cap)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_cases_through_the_c_abi(name):
    v, sem, M, cap = _cases()[name]
    ref = _reference(name)
    same(run(v, sem, M, cap), ref)
    B, H, W = sem.shape
    if name == "1x1_zero":
        assert ref["count"][0] == 0 and ref["ids"][0, 0, 0] == 0
    if name == "1x1_value":
        assert ref["count"][0] == 1 and ref["values"][0, 0] == -9 and ref["table"][0, 0].tolist() == [3, 1, 0, 0, 0, 0, 0, 1]
    if name == "one_id_256x256":
        assert ref["table"][0, 0].tolist() == [26, 65536, 0, 0, 255, 255, 0, 1]
    if name == "batch_of_three":
        assert len(set(ref["count"].tolist())) > 1 or not np.array_equal(ref["ids"][0], ref["ids"][1])
    if name == "extreme_keys":
        assert ref["values"][0, :4].tolist() == [R.I32_MIN, -1, 1, R.I32_MAX] and ref["count"][0] == 4
    if name in ("top_byte_only", "low_byte_only", "three_bytes_shared"):
        d = np.unique(v[v != 0])
        x = np.bitwise_or.reduce(d & 0xffffffff) ^ np.bitwise_and.reduce(d & 0xffffffff)
        assert x != 0 and (x & ~{"top_byte_only": 0xff000000, "low_byte_only": 0xff, "three_bytes_shared": 0xff}[name]) == 0
        assert ref["count"][0] > 64
    if name == "zero_among_negatives":
        assert ref["values"][0, :4].tolist() == [-3, -1, 2, 5] and ref["ids"][0].tolist() == [[1, 0, 4, 2], [3, 3, 0, 1]]
    if name == "distinct_64x64":
        assert ref["count"][0] == M == 4096 and (ref["table"][0, :, 1] == 1).all()
    if name == "distinct_65x64":
        assert ref["count"][0] == 4160 > M and ref["ids"].max() == 4160 and (ref["order"][0] == np.arange(1, M + 1)).all()
    if name == "distinct_256x256_one_row":
        assert ref["count"][0] == 65536 and M == 1 and sorted(ref["ids"].reshape(-1).tolist()) == list(range(1, 65537))
    if name == "split_and_touching":
        assert ref["count"][0] == 3 and ref["table"][0, :3, 1].tolist() == [36, 30, 30]
    if name == "alternating_columns":
        assert ref["count"][0] == 2 and ref["table"][0, :2, 1].tolist() == [96, 96]
    if name == "median_by_hand":
        assert ref["table"][0, :5, 0].tolist() == R.MEDIAN_BY_HAND
    if name == "median_1024_classes":
        assert ref["table"][0, 0, 1] == 65536 and len(np.unique(sem)) == 1024
        assert ref["table"][0, 0, 0] == int(np.median(sem))
    if name == "class_cap_one":
        assert ref["invalid"][0] == 0 and (ref["table"][0, :ref["count"][0], 0] == 0).all()


def test_invalid_classes_and_ids_outside_int32():
    v, sem, M, cap = R.invalid_case()
    ref = R.instances(v, sem, M, cap)
    assert ref["invalid"].tolist() == [1, 0, 2]
    assert (ref["ids"][0, 0, 0:2] == 0).all() and (ref["ids"][0, 6, 0:4] == 0).all() and (ref["ids"][0, 7, 0:2] == 0).all()
    k = ref["ids"][0, 7, 2]
    assert k > 0 and ref["table"][0, k - 1, 1] == 2 and ref["values"][0, k - 1] == 4002
    assert (ref["ids"][2, 0:2, 0:3] == 0).all() and (ref["ids"][2, 2, 0:2] == 0).all()
    assert ref["values"][2, 0] == R.I32_MIN and ref["values"][2, ref["count"][2] - 1] == R.I32_MAX
    same(run(v, sem, M, cap, "i64"), ref)
    # both reasons in one image
    v2, sem2 = v[2:].copy(), sem[2:].copy()
    sem2[0, 5, 5] = 19
    v2[0, 5, 5] = 77
    ref2 = R.instances(v2, sem2, M, cap)
    assert ref2["invalid"].tolist() == [3]
    same(run(v2, sem2, M, cap, "i64"), ref2)


def test_the_three_kinds_agree():
    rng = np.random.default_rng(71)
    pool = np.array([0, 0, 1, 255, 256, 65535, 65536, 65537, (1 << 24) - 1, 26001, 26002, 7], np.int64)
    v = np.kron(pool[rng.integers(0, len(pool), (2, 7, 9))], np.ones((3, 3), np.int64))[:, :19, :25]
    sem = rng.integers(0, 19, v.shape).astype(np.int32)
    ref = R.instances(v, sem, 16, 19)
    assert np.array_equal(ref["ids"], R.instances(R.rgb_of(v), sem, 16, 19)["ids"])
    same(run(v, sem, 16, 19, "i64"), ref)
    same(run(v, sem, 16, 19, "i32"), ref)
    same(run(R.rgb_of(v), sem, 16, 19, "rgb8"), ref)


def test_two_runs_are_bit_identical():
    for name in ("batch_of_three", "distinct_65x64", "median_1024_classes"):
        v, sem, M, cap = _cases()[name]
        a, b = run(v, sem, M, cap), run(v, sem, M, cap)
        for k in OUT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.GOLDEN))
def test_goldens_through_the_python_api(name):
    import maskunet_amd
    from tests.test_idmap_host import check_against_golden
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    inst = maskunet_amd.instances_from_id_map(torch.from_numpy(g["id_map"]).to(DEV), torch.from_numpy(g["sem"]).to(DEV), 64, 256)
    assert inst.prob is None and inst.classes.dtype == torch.int32 and np.array_equal(inst.classes.cpu().numpy(), g["sem"])
    got = side_of(inst)
    check_against_golden(got, g)
    same(got, R.instances(g["id_map"], g["sem"], 64, 256))
    for d, c, box in zip(inst.to_reference(0), g["category_id"], g["bbox"]):       # equal scores: ascending id = the reference's order
        assert d["category_id"] == c and d["bbox"] == box.tolist() and d["score"] == 1.0


def test_python_api_dtypes_defaults_and_non_contiguous_inputs():
    import maskunet_amd
    v, sem = R.blocky(81, 2, 40, 36)
    big_v, big_s = torch.from_numpy(np.repeat(np.repeat(v, 2, 1), 2, 2)).to(DEV), torch.from_numpy(sem.transpose(0, 2, 1).copy()).to(DEV)
    tv, ts = big_v[:, ::2, ::2], big_s.transpose(1, 2).long()                      # strided views of larger tensors, int64 classes
    assert not tv.is_contiguous() and not ts.is_contiguous()
    inst = maskunet_amd.instances_from_id_map(tv, ts)
    assert inst.table.shape == (2, 1024, 8) and inst.values.shape == (2, 1024) and inst.invalid.shape == (2,)
    same(side_of(inst), R.instances(v, sem, 1024, 256))
    fits = np.clip(v, R.I32_MIN, R.I32_MAX)
    inst = maskunet_amd.instances_from_id_map(torch.from_numpy(fits.astype(np.int32)).to(DEV), torch.from_numpy(sem).to(DEV), 32, 19)
    same(side_of(inst), R.instances(fits, sem, 32, 19))
    img = R.rgb_of(np.abs(fits) % (1 << 24))
    wide = torch.from_numpy(np.concatenate([img, img], -1)).to(DEV)[..., :3]       # a non-contiguous colour image
    assert not wide.is_contiguous()
    same(side_of(maskunet_amd.instances_from_id_map(wide, torch.from_numpy(sem).to(DEV), 32, 19)), R.instances(img, sem, 32, 19))


def test_python_api_errors():
    import maskunet_amd
    f = maskunet_amd.instances_from_id_map
    v = torch.zeros((1, 8, 8), dtype=torch.int64, device=DEV)
    c = torch.zeros((1, 8, 8), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="on the GPU"):
        f(v.cpu(), c)
    with pytest.raises(RuntimeError, match="on the GPU"):
        f(v, c.cpu())
    with pytest.raises(RuntimeError, match="uint8"):
        f(v.to(torch.int16), c)
    with pytest.raises(RuntimeError, match="uint8"):
        f(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=DEV), c)
    with pytest.raises(RuntimeError, match="uint8"):
        f(v[0], c)
    with pytest.raises(RuntimeError, match="semantic map"):
        f(v, c.float())
    with pytest.raises(RuntimeError, match="differ"):
        f(v, torch.zeros((1, 8, 9), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="differ"):
        f(torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=DEV), c)
    for kw in ({"max_instances": 0}, {"max_instances": 4097}, {"class_cap": 0}, {"class_cap": 1025}):
        with pytest.raises(RuntimeError, match="4096"):
            f(v, c, **kw)
    with pytest.raises(RuntimeError, match="65536"):
        f(torch.zeros((1, 256, 257), dtype=torch.int32, device=DEV), torch.zeros((1, 256, 257), dtype=torch.int32, device=DEV))


def test_match_instances_against_the_host_reference():
    import maskunet_amd
    from tests import _match_reference as MR
    from tests.test_gpu_match import OUT_KEYS as MATCH_KEYS
    C = 19
    v, sem, labels = R.things_case(91, 3, 37, 29, C)
    gt = maskunet_amd.instances_from_id_map(torch.from_numpy(v).to(DEV), torch.from_numpy(sem).to(DEV), 64, C)
    pred = maskunet_amd.instances_from_labels(torch.from_numpy(np.roll(labels, 1, 2)).to(DEV), max_instances=256)
    m = maskunet_amd.match_instances(pred, gt, C, max_queries=200)
    ref = MR.match(side_of(pred), side_of(gt), C, max_queries=200)
    print(f"coco matches per threshold {(ref['det_gt'] > 0).sum((0, 2)).tolist()}, panoptic {(ref['pq_gt'] > 0).sum()}")
    assert (ref["det_gt"][:, 0] > 0).sum() >= 20 and (ref["pq_gt"] > 0).sum() >= 20 and not ref["overflow"].any()
    for k in MATCH_KEYS:
        assert np.array_equal(getattr(m, k).cpu().numpy(), ref[k]), k


def test_rle_export_against_the_host_reference():
    import maskunet_amd
    from tests import _rle_reference as RR
    g = np.load(os.path.join(GOLDEN, "idmap_cityscapes_32x32.npz"))
    inst = maskunet_amd.instances_from_id_map(torch.from_numpy(g["id_map"]).to(DEV), torch.from_numpy(g["sem"]).to(DEV), 16, 256)
    rles = inst.rle()
    n = len(g["category_id"])
    assert rles.counts_list(0)[:n] == [RR.encode(g["masks"] == k + 1) for k in range(n)]
    assert rles.to_coco(0) == [{"size": [32, 32], "counts": RR.string(RR.encode(g["masks"] == k + 1))} for k in range(n)]
    assert rles.area[0, :n].tolist() == g["area"].tolist()


def test_panoptic_quality_changes_with_the_ground_truth_partition():
    """A perfect prediction of two touching cars (30 pixels each) and one car in two pieces (16 + 20 pixels), class 1.
    Against the id-map ground truth every car matches at IoU 1: tp 3, fp 0, fn 0.  Against connected components of the class map the
    touching cars are ONE ground truth of 60 pixels (IoU 30 / 60 = 0.5, not above 0.5: no match for either) and the pieces are two
    (16 / 36 < 0.5; 20 / 36 > 0.5: one match): tp 1, fp 2, fn 2."""
    import maskunet_amd
    v, sem = R.touching_and_split()
    tv, ts = torch.from_numpy(v).to(DEV), torch.from_numpy(sem).to(DEV)
    pred = maskunet_amd.instances_from_id_map(tv, ts, 8, 2)
    stats = []
    for gt in (maskunet_amd.instances_from_id_map(tv, ts, 8, 2), maskunet_amd.instances_from_labels(ts, max_instances=8)):
        pq = maskunet_amd.PanopticQuality(2)
        pq.update(maskunet_amd.match_instances(pred, gt, 2))
        r = pq.compute()
        stats.append((int(r["tp"][1]), int(r["fp"][1]), int(r["fn"][1])))
    assert stats == [(3, 0, 0), (1, 2, 2)]


def test_coco_masks_ids_become_instances():
    """what tests/test_gpu_poly.py::as_instances builds on the host around coco_masks(...).ids: ids, areas and counts"""
    import maskunet_amd
    rect = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]
    ann = [[[rect(2, 2, 14, 14)], [rect(10, 10, 20, 20)], [rect(15, 15, 30, 32)], [rect(40, 40, 50, 50)]], [[rect(1, 1, 9, 5)]], []]
    r = maskunet_amd.coco_masks(ann, [(33, 31), (12, 12), (5, 6)], (33, 31))
    B, M = 3, 16
    ids = r.ids
    count = ids.view(B, -1).max(1).values.to(torch.int32)
    areas = torch.stack([torch.bincount(ids[b].view(-1).long(), minlength=M + 1)[1:] for b in range(B)]).to(torch.int32)
    present = [sorted(set(ids[b].view(-1).tolist()) - {0}) for b in range(B)]
    assert present[0] == [1, 2, 3] and present[1] == [1] and present[2] == []     # every id present: the numbering is the identity
    cat = torch.tensor([[0, 3, 5, 7, 9], [0, 4, 0, 0, 0], [0, 0, 0, 0, 0]], device=DEV)                # category table, row 0 = no annotation
    sem = torch.gather(cat, 1, ids.view(B, -1).long()).view_as(ids)
    inst = maskunet_amd.instances_from_id_map(ids, sem, M, 19)
    assert torch.equal(inst.ids, ids.to(torch.int32)) and torch.equal(inst.count, count)
    assert torch.equal(inst.table[:, :, 1], areas) and inst.invalid.tolist() == [0, 0, 0]
    assert inst.table[0, :3, 0].tolist() == [3, 5, 7] and inst.table[1, 0, 0].tolist() == 4
    assert torch.equal(inst.values[:, :3], torch.tensor([[1, 2, 3], [1, 0, 0], [0, 0, 0]], dtype=torch.int32, device=DEV))
