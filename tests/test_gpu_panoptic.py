"""GPU: panoptic segments (mu_panoptic, maskunet_amd.panoptic_segments) against the numpy restatement of the contract in
tests/_panoptic_reference.py.  Everything is integer, or fp32 copied through: every comparison is ==.  Memory discipline as in
test_gpu_instances.py: outputs pre-filled with a sentinel, the workspace exactly the queried size, 4 KiB guard bands around every
buffer, inputs verified untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import _panoptic_reference as R
from tests._device_buffers import Guarded, call, side_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
IN_KEYS = ("cls", "ids", "table", "score", "count", "kind", "category")
PARAMS = {"label_divisor": 1000, "stuff_area_limit": 0, "thing_area_limit": 0, "score_threshold": 0.0, "max_seg": 16, "bgr": 0}


def run(inputs, **kw):
    """raw mu_panoptic on numpy inputs -> dict of numpy outputs; checks guards, untouched inputs and that every byte was written"""
    from maskunet_amd import _lib
    lib = _lib.load()
    p = dict(PARAMS, **kw)
    B, H, W = inputs["cls"].shape
    max_inst, C, S = inputs["table"].shape[1], len(inputs["kind"]), p["max_seg"]
    i32, f32 = torch.int32, torch.float32
    g_in = [Guarded(inputs[k].size, f32 if k == "score" else i32, inputs[k], k) for k in IN_KEYS]
    shapes = {"seg": ((B, H, W), i32), "seg_cls": ((B, H, W), i32), "table": ((B, S, 8), i32), "score": ((B, S), f32),
              "count": ((B,), i32), "order": ((B, S), i32), "source": ((B, S), i32), "values": ((B, S), i32), "id_map": ((B, H, W), i32),
              "rgb": ((B, H, W, 3), torch.uint8), "invalid": ((B,), i32)}
    assert tuple(shapes) == R.OUT_KEYS
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    assert lib.mu_panoptic_supported(H, W, max_inst, C, S, p["label_divisor"], p["stuff_area_limit"], p["thing_area_limit"]) == 0
    nws = lib.mu_panoptic_workspace_bytes(B, H, W, max_inst, C, S)
    assert nws > 0 and nws % 8 == 0
    call("mu_panoptic", *g_in, B, H, W, max_inst, C, p["label_divisor"], p["stuff_area_limit"], p["thing_area_limit"],
         float(p["score_threshold"]), S, p["bgr"], *outs.values(), Guarded(nws // 8, torch.int64, name="workspace"), nws)
    got = {k: outs[k].host(shapes[k][0]) for k in shapes}
    for k in shapes:
        if k != "rgb" or not (got["rgb"] == outs["rgb"].sent).any():       # 0xA5 is a legal colour byte; equality with the reference covers it
            outs[k].all_written()
    return got


def same(got, ref):
    print(f"count {got['count'].tolist()} (reference {ref['count'].tolist()}), invalid {got['invalid'].tolist()}")
    for k in R.OUT_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
    for j, col in enumerate(("class", "area", "x_min", "y_min", "x_max", "y_max", "first_pixel", "class_rank")):
        assert np.array_equal(got["table"][:, :, j], ref["table"][:, :, j]), f"table column {col}"
    for k in R.OUT_KEYS:
        assert np.array_equal(got[k], ref[k]), k


@functools.lru_cache(maxsize=None)
def _cases():
    out = R.cases()
    for inputs, _ in out.values():
        for a in inputs.values():
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name):
    inputs, params = _cases()[name]
    ref = R.segments(**inputs, **params)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_cases_through_the_c_abi(name):
    inputs, params = _cases()[name]
    ref = _reference(name)
    same(run(inputs, **params), ref)
    n, inv = ref["count"].tolist(), ref["invalid"].tolist()
    if name.startswith("1x1"):
        assert n == [0 if name == "1x1_void" else 1]
    if name == "1x1_stuff_under_an_instance":
        assert ref["source"][0, 0] == 0 and ref["values"][0, 0] == 5000
    if name.startswith("distinct_64x64"):
        m = params["max_seg"]
        assert n == [4096] and inv == [0 if m == 4096 else 2] and np.array_equal(ref["seg"], inputs["ids"])
        assert (ref["id_map"] != 0).sum() == m
    if name == "256x256":
        assert n[0] > 64 and inv == [0] and ref["table"][0, :n[0], 1].max() > 1024
    if name == "33x31_few_rows":
        assert inv == [2] and ref["seg"].max() == n[0] > params["max_seg"]
    if name == "one_class_stuff":
        assert n == [1] and ref["table"][0, 0].tolist() == [0, 13 * 9, 0, 0, 8, 12, 0, 1]
    if name == "1024_classes":
        assert ref["table"][0, :n[0], 0].max() > 900 and inv == [0]
    if name == "batch_of_three_void_in_the_middle":
        assert n[1] == 0 and n[0] > 0 and n[2] > 0 and not ref["seg"][1].any() and not ref["rgb"][1].any()
    if name == "count_past_max_inst":
        assert inv == [4] and int(inputs["count"][0]) > inputs["table"].shape[1]
    if name == "count_zero":
        assert n[0] > 0 and not ref["source"].any()
    if name == "label_divisor_one":
        assert inv == [1] and ref["values"][0, :3].tolist() == [7, 0, 0]
    if name == "stuff_value_2_24_minus_1":
        assert inv == [0] and ref["values"][0, 0] == (1 << 24) - 1 and (ref["rgb"][0, 0, 0] == 255).all()
    if name == "stuff_value_2_24":
        assert inv == [1] and n == [1] and not ref["values"].any() and not ref["rgb"].any() and ref["seg"].any()
    if name == "thing_value_2_24_minus_1_and_2_24":
        assert inv == [1] and ref["values"][0, :3].tolist() == [14, (1 << 24) - 1, 0]
    if name.startswith("thing_area_limit"):
        assert n == [1 if name.endswith("5") else 3]
    if name.startswith("stuff_area_limit"):
        assert n == [2 if name.endswith("7") else 3]
    if name == "score_threshold_equal":
        assert n == [2] and ref["source"][0, :2].tolist() == [0, 2]
    if name == "score_threshold_one_ulp_above":
        assert n == [1] and ref["seg"][0, 2:, 2:4].tolist() == [[0, 0], [0, 0]]       # the dropped thing is void, not stuff


def test_null_pointers_and_unsupported_shapes_refuse_before_launch():
    from maskunet_amd import _lib
    lib = _lib.load()
    inputs, params = _cases()["hand_4x6"]
    B, H, W = inputs["cls"].shape
    g_in = [Guarded(inputs[k].size, torch.float32 if k == "score" else torch.int32, inputs[k], k) for k in IN_KEYS]
    sizes = [B * H * W, B * H * W, B * 4 * 8, B * 4, B, B * 4, B * 4, B * 4, B * H * W, B * H * W * 3, B]
    dtypes = [torch.int32] * 3 + [torch.float32] + [torch.int32] * 5 + [torch.uint8, torch.int32]
    outs = [Guarded(n, d, name=k) for n, d, k in zip(sizes, dtypes, R.OUT_KEYS)]
    ws = Guarded(4, torch.int64, name="workspace")

    def rc(ins=g_in, os=outs, w=ws, nws=32, dims=(B, H, W, 4, 3), scal=(1000, 0, 0, 0.0, 4, 0)):
        args = [a.p if isinstance(a, Guarded) else a for a in (*ins, *dims, *scal[:3], float(scal[3]), *scal[4:], *os, w, nws)]
        return getattr(lib, "mu_panoptic")(*args, _lib.stream())

    for j in range(len(g_in)):
        assert rc(ins=[None if i == j else g for i, g in enumerate(g_in)]) == -1
    for j in range(len(outs)):
        assert rc(os=[None if i == j else g for i, g in enumerate(outs)]) == -1
    assert rc(w=None) == -1 and rc(scal=(1000, 0, 0, 0.0, 4, 2)) == -1
    assert rc(nws=24) == -4
    for dims in ((B, 256, 257, 4, 3), (B, H, W, 0, 3), (B, H, W, 4097, 3), (B, H, W, 4, 0), (B, H, W, 4, 1025)):
        assert rc(dims=dims) == -2 and lib.mu_panoptic_workspace_bytes(*dims, 4) == 0
    for scal in ((0, 0, 0, 0.0, 4, 0), (1000, -1, 0, 0.0, 4, 0), (1000, 0, -1, 0.0, 4, 0), (1000, 0, 0, 0.0, 0, 0), (1000, 0, 0, 0.0, 4097, 0)):
        assert rc(scal=scal) == -2
    torch.cuda.synchronize()
    for g in (*g_in, *outs, ws):
        g.check()
        if g.data is None:
            assert bool((g.t == g.sent).all()), f"{g.name} was written by a refused call"
    assert rc() == 0                                           # the same arguments, complete: accepted
    torch.cuda.synchronize()


def test_two_runs_are_bit_identical():
    for name in ("33x31", "distinct_64x64_max_seg_4095", "256x256"):
        inputs, params = _cases()[name]
        a, b = run(inputs, **params), run(inputs, **params)
        for k in R.OUT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


# ------------------------------------------------------------------------------------------------
# through the Python API
THINGS = (False, False, True, True, False, True)              # six classes: 0 void, 1 and 4 stuff, 2, 3 and 5 things
CATEGORY = (0, 11, 22, 33, 44, 55)


def reference_of(inst, things=THINGS, void=(0,), category=CATEGORY, **kw):
    """the restatement fed the same Instances"""
    s = side_of(inst)
    kind = np.array([R.VOID if c in void else R.THING if t else R.STUFF for c, t in enumerate(things)], np.int32)
    return R.segments(inst.classes.cpu().numpy(), s["ids"], s["table"], s["score"], s["count"], kind, np.asarray(category, np.int32), **kw)


def pan_side(pan):
    names = {"seg": "seg", "seg_cls": "seg_cls", "table": "table", "score": "scores", "count": "count", "order": "order", "source": "source",
             "values": "values", "id_map": "id_map", "rgb": "rgb", "invalid": "invalid"}
    return {k: getattr(pan, f).cpu().numpy() for k, f in names.items()}


def blocky_logits(seed, B, C, H, W, dtype, cell=5):
    """logits whose arg-max is constant over cells, with margins that give a spread of probabilities"""
    rng = np.random.default_rng(seed)
    gh, gw = -(-H // cell), -(-W // cell)
    g = rng.integers(0, C, (B, gh, gw))
    cls = np.kron(g, np.ones((cell, cell), np.int64))[:, :H, :W]
    x = rng.normal(0, 0.3, (B, C, H, W))
    x += 1.5 * (np.arange(C)[None, :, None, None] == cls[:, None])
    return torch.from_numpy(x).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_predicted_instances_become_segments(dtype):
    import maskunet_amd
    logits = blocky_logits(5, 2, 6, 24, 20, dtype)
    inst = maskunet_amd.predict_instances(logits, max_instances=256)
    kw = dict(label_divisor=1000, stuff_area_limit=30, thing_area_limit=4, score_threshold=0.6)
    pan = maskunet_amd.panoptic_segments(inst, THINGS, category_ids=CATEGORY, max_segments=64, **kw)
    ref = reference_of(inst, max_seg=64, **kw)
    print(f"instances {inst.count.tolist()} -> segments {ref['count'].tolist()}")
    assert (ref["count"] >= 4).all() and (ref["count"] < inst.count.cpu().numpy()).all() and (ref["source"] > 0).any()
    same(pan_side(pan), ref)
    both = maskunet_amd.predict_panoptic(logits, THINGS, max_instances=256, category_ids=CATEGORY, max_segments=64, **kw)
    same(pan_side(both), ref)
    for b in range(2):
        assert pan.segments_info(b) == R.segments_info(ref, b, CATEGORY)
    assert pan.annotation(1, 139) == {"image_id": 139, "file_name": "139.png", "segments_info": R.segments_info(ref, 1, CATEGORY)}
    assert pan.annotation(0, 7, "x.png")["file_name"] == "x.png"


def test_embedding_instances_become_segments():
    import maskunet_amd
    rng = np.random.default_rng(6)
    g = rng.integers(0, 6, (2, 5, 4))
    cls = np.kron(g, np.ones((5, 5), np.int64))
    centre = rng.normal(0, 4, (2, 5, 4, 8))
    emb = np.kron(centre.transpose(0, 3, 1, 2), np.ones((5, 5))) + rng.normal(0, 0.01, (2, 8, 25, 20))
    inst = maskunet_amd.instances_from_embeddings(torch.from_numpy(cls).to(DEV), torch.from_numpy(emb).float().to(DEV), num_classes=6,
                                                  max_instances=64)
    pan = maskunet_amd.panoptic_segments(inst, THINGS, category_ids=CATEGORY, max_segments=32)
    ref = reference_of(inst, max_seg=32)
    assert (inst.count > 4).all().item() and (ref["source"] > 0).any() and (ref["invalid"] == 0).all()
    same(pan_side(pan), ref)


def idmap_inputs():
    """an id map whose instance 26001 lies across a class boundary: its median class (3, a thing) differs from the class of a third of
    its pixels (1, stuff), and those pixels go with the thing"""
    sem = np.ones((1, 12, 10), np.int64)
    v = np.zeros((1, 12, 10), np.int64)
    sem[0, 2:8, 2:6] = 3
    v[0, 2:8, 1:7] = 26001                                     # 36 pixels: 24 of class 3, 12 of class 1
    sem[0, 9:, :5] = 4
    v[0, 9:, :5] = 4000                                        # a stuff class the dataset gives an id of its own
    sem[0, 0, 9] = 2
    v[0, 0, 9] = 22005
    return v, sem


def test_id_map_instances_become_segments():
    import maskunet_amd
    v, sem = idmap_inputs()
    inst = maskunet_amd.instances_from_id_map(torch.from_numpy(v).to(DEV), torch.from_numpy(sem).to(DEV), 16, 6)
    pan = maskunet_amd.panoptic_segments(inst, THINGS, category_ids=CATEGORY, max_segments=8)
    ref = reference_of(inst, max_seg=8)
    same(pan_side(pan), ref)
    assert ref["count"].tolist() == [4] and ref["table"][0, :4, :2].tolist() == [[1, 120 - 36 - 15 - 1, ], [2, 1], [3, 36], [4, 15]]
    assert (ref["seg_cls"][0, 2:8, 1:7] == 3).all() and ref["values"][0, :4].tolist() == [11000, 22001, 33001, 44000]
    assert pan.segments_info(0)[1] == {"id": 22001, "category_id": 22, "area": 1, "bbox": [9, 0, 1, 1], "iscrowd": 0}


@pytest.mark.parametrize("bgr", [False, True])
def test_round_trip_through_the_id_map_kernel(bgr):
    """instances_from_id_map reads the image panoptic_segments wrote and finds the same partition: it numbers the distinct values in
    ascending order, so its id j is our segment with the j-th smallest value"""
    import maskunet_amd
    logits = blocky_logits(8, 2, 6, 24, 20, torch.float32)
    pan = maskunet_amd.predict_panoptic(logits, THINGS, max_instances=256, category_ids=CATEGORY, max_segments=64, bgr=bgr)
    assert pan.invalid.tolist() == [0, 0] and (pan.count > 4).all().item()
    rgb = pan.rgb.flip(-1) if bgr else pan.rgb                 # the reader takes R,G,B
    back = maskunet_amd.instances_from_id_map(rgb, pan.instances.classes, 64, 6)
    assert torch.equal(back.count, pan.count) and back.invalid.tolist() == [0, 0]
    seg, ids = pan.seg.cpu().numpy(), back.ids.cpu().numpy()
    for b in range(2):
        n = int(pan.count[b])
        values = pan.values[b, :n].cpu().numpy()
        assert len(set(values.tolist())) == n
        ours = np.argsort(values) + 1                          # ours[j - 1] = our number of their id j
        assert np.array_equal(back.values[b, :n].cpu().numpy(), values[ours - 1])
        assert np.array_equal(back.table[b, :n, 0].cpu().numpy(), pan.table[b, :n, 0].cpu().numpy()[ours - 1])
        lut = np.zeros(n + 1, np.int32)
        lut[1:] = ours
        assert np.array_equal(lut[ids[b]], seg[b])
    assert np.array_equal(R.rgb2id(pan.rgb.cpu().numpy(), bgr), pan.id_map.cpu().numpy())


def test_panoptic_quality_of_a_split_stuff_class():
    """6 x 8 pixels, class 1 stuff, class 2 a thing.  Ground truth: stuff = columns 0-3 (24 pixels, one piece), one thing of 9 pixels.
    Prediction: the same thing; of the stuff, row 2 is missing (void), which leaves pieces of 8 and 12 pixels.
    Connected components on both sides: the pieces have IoU 8 / 24 and 12 / 24, neither above 0.5, and touch no void: class 1 has
    tp 0, fp 2, fn 1.  Panoptic segments on both sides: ONE predicted stuff segment of 20 pixels, IoU 20 / 24: tp 1, fp 0, fn 0.
    The thing matches at IoU 1 either way: tp 1, fp 0, fn 0."""
    import maskunet_amd
    gt = np.zeros((1, 6, 8), np.int64)
    gt[0, :, :4] = 1
    gt[0, :3, 5:] = 2
    pred = gt.copy()
    pred[0, 2, :4] = 0
    things = (False, False, True)
    sides = [maskunet_amd.instances_from_labels(torch.from_numpy(a).to(DEV), max_instances=8) for a in (pred, gt)]
    assert sides[0].count.tolist() == [3] and sides[1].count.tolist() == [2]
    stats = []
    for p, g in (sides, [maskunet_amd.panoptic_segments(s, things, max_segments=8).instances for s in sides]):
        pq = maskunet_amd.PanopticQuality(3, things)
        pq.update(maskunet_amd.match_instances(p, g, 3))
        r = pq.compute()
        stats.append([(int(r["tp"][c]), int(r["fp"][c]), int(r["fn"][c])) for c in (1, 2)])
    assert stats == [[(0, 2, 1), (1, 0, 0)], [(1, 0, 0), (1, 0, 0)]]
    assert r["iou_sum"][1] == 20 / 24 and r["Stuff"]["pq"] == 20 / 24 and r["Things"]["pq"] == 1.0


def test_rle_areas_equal_table_areas():
    import maskunet_amd
    pan = maskunet_amd.predict_panoptic(blocky_logits(9, 2, 6, 24, 20, torch.float16), THINGS, max_instances=256, max_segments=64)
    table = torch.cat([torch.zeros((2, 1), dtype=torch.int32, device=DEV), pan.table[:, :, 1]], 1)        # area by segment number
    want = torch.gather(table, 1, pan.order.long())
    assert (pan.count > 4).all().item()
    for rles in (maskunet_amd.encode_rle(pan.seg, pan.order), pan.instances.rle()):
        assert torch.equal(rles.area.to(torch.int32), want)


def test_refusals_launch_nothing(monkeypatch):
    import maskunet_amd
    from maskunet_amd import panoptic
    launched = []
    monkeypatch.setattr(panoptic, "call", lambda name, *a: launched.append(name))
    inst = maskunet_amd.instances_from_labels(torch.zeros((1, 8, 8), dtype=torch.int64, device=DEV), max_instances=8)
    f = maskunet_amd.panoptic_segments
    host = maskunet_amd.Instances(*(t.cpu() for t in (inst.classes, inst.ids, inst.table, inst.scores, inst.count, inst.order)))
    with pytest.raises(RuntimeError, match="on the GPU"):
        f(host, THINGS)
    with pytest.raises(TypeError, match="Instances"):
        f(inst.ids, THINGS)
    with pytest.raises(ValueError, match="one boolean per class"):
        f(inst, ())
    with pytest.raises(ValueError, match="one id per class"):
        f(inst, THINGS, category_ids=(1, 2, 3))
    with pytest.raises(ValueError, match="thing and as void"):
        f(inst, THINGS, void=(0, 2))
    with pytest.raises(ValueError, match="outside"):
        f(inst, THINGS, void=(6,))
    for kw in ({"max_segments": 0}, {"max_segments": 4097}, {"label_divisor": 0}, {"stuff_area_limit": -1}, {"thing_area_limit": -1}):
        with pytest.raises(RuntimeError, match="4096"):
            f(inst, THINGS, **kw)
    with pytest.raises(RuntimeError, match="1024"):
        f(inst, (False,) * 1025)
    assert launched == []
    f(inst, THINGS)
    assert launched == ["mu_panoptic"]


def test_two_calls_are_bit_identical():
    import maskunet_amd
    inst = maskunet_amd.predict_instances(blocky_logits(10, 3, 6, 33, 31, torch.float32), max_instances=256)
    a, b = (pan_side(maskunet_amd.panoptic_segments(inst, THINGS, max_segments=32, score_threshold=0.55)) for _ in range(2))
    for k in R.OUT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
