"""GPU: semantic evaluation at the labels' own resolution (mu_sem_eval_native, maskunet_amd.metrics.semantic_eval_native) against the
fp32 restatement of its contract in tests/_native_eval_reference.py, which tests/test_native_eval_host.py pins to torch.

Every output is an integer and is compared with ==: no tolerance anywhere.  Memory discipline as in the other post-processing tests:
every buffer between guard bands, outputs pre-filled with a sentinel, the workspace exactly the queried size; class-map bytes outside
the accepted images' spans (gaps between images, refused images) must keep their sentinel.  The refused images are ordinary validated
inputs: no test provokes a fault."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import _native_eval_reference as R
from tests._device_buffers import Guarded, call

pytestmark = pytest.mark.gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "maskunet_hip.h")
K = {k: int(v) for k, v in re.findall(r"#define (MU_SEM_NATIVE_[A-Z_]+) (\d+)", open(HEADER).read())}
TH, TW = K["MU_SEM_NATIVE_TILE_H"], K["MU_SEM_NATIVE_TILE_W"]
TDT = {"fp32": torch.float32, "fp16": torch.float16}
SOURCES = [(1, 1), (1, 7), (8, 8), (16, 12)]
# 213 / 214: with a source of 16x12 the window share is the whole MU_SEM_NATIVE_WINDOW_BYTES, and C = 214 is the first class count whose
# (C+1) x C counters no longer fit beside it (checked in test_every_path_is_reached); 193 is the first above mu_sem_eval's own switch
CLASSES = [1, 2, 19, 150, 193, 213, 214, 256]


def lds_plan(C, h, w):
    """(window share in floats, confusion counters in LDS) as the header states the rule"""
    share = min(K["MU_SEM_NATIVE_WINDOW_BYTES"], C * ((h * w) | 1) * 4)
    return share // 4, (3 * C + ((C + 1) * C + 1) // 2) * 4 + share <= K["MU_SEM_NATIVE_LDS_BYTES"]


def tiles_in_lds(C, h, w, H, W):
    """per tile of an H x W image: does its source window fit the LDS share"""
    share, _ = lds_plan(C, h, w)
    y0, y1, _, _ = R.taps(h, H)
    x0, x1, _, _ = R.taps(w, W)
    out = []
    for Y0 in range(0, H, TH):
        for X0 in range(0, W, TW):
            wy = y1[min(Y0 + TH, H) - 1] - y0[Y0] + 1
            wx = x1[min(X0 + TW, W) - 1] - x0[X0] + 1
            out.append(C * ((int(wy) * int(wx)) | 1) <= share)
    return out


def batch_sizes(h, w):
    """the ragged batch of every case: 1x1, the identity, 37x53, x4, x8, 5x3 (downscaling), 1x200, 200x1, one row and one column more than
    whole tiles"""
    return [(1, 1), (h, w), (37, 53), (4 * h, 4 * w), (8 * h, 8 * w), (5, 3), (1, 200), (200, 1), (TH + 1, 2 * TW + 1)]


def void_values(C, ignore):
    """label bytes that are void: the ignore value if it is a byte, and (C < 255) the first and the last value >= C"""
    return ([ignore] if 0 <= ignore <= 255 else []) + ([C, 254] if C < 255 else [])


def pack(sizes, rng, C, ignore, void_image=2):
    """(data, offsets, sizes): every image starts at an odd byte, 6 more bytes lie between images 1 and 2; labels hold 0, C - 1, the ignore
    value and (C < 255) values >= C; image `void_image` is wholly void"""
    void = void_values(C, ignore)
    offsets, chunks, at = [], [], 0
    for i, (H, W) in enumerate(sizes):
        gap = (1 if at % 2 == 0 else 2) + (6 if i == 2 else 0)
        chunks.append(np.full(gap, 0x5A, np.uint8))
        at += gap
        offsets.append(at)
        lab = rng.integers(0, C, H * W)
        kind = rng.random(H * W)
        if i == void_image and void:
            lab = rng.choice(void, H * W)
        else:
            if void:
                lab[kind < 0.15] = rng.choice(void, int((kind < 0.15).sum()))
            lab[0], lab[-1] = 0, C - 1
        chunks.append(lab.astype(np.uint8))
        at += H * W
    offsets.append(at)
    assert all(o % 2 == 1 for o in offsets[:-1])
    return np.concatenate(chunks), np.asarray(offsets, np.int64), np.asarray(sizes, np.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def case(C, h, w, kind="normal", ignore=255):
    """(x [B,C,h,w] fp32 holding fp16-exact values, data, offsets, sizes, max_h, max_w, restatement), computed once and left unchanged"""
    sizes = batch_sizes(h, w) if kind == "normal" else [(h, w), (4 * h, 4 * w), (8 * h, 8 * w), (max(h // 2, 1), max(w // 2, 1)), (2 * h, 4 * w)]
    rng = np.random.default_rng(7 * C + 100 * h + w)
    if kind == "normal":
        x = rng.standard_normal((len(sizes), C, h, w)).astype(np.float16).astype(np.float32)
    else:
        x = R.grid_logits(len(sizes), C, h, w)
    data, offsets, sz = pack(sizes, rng, C, ignore)
    max_h, max_w = int(sz[:, 0].max()), int(sz[:, 1].max())
    ref = R.native_eval(x, data, offsets, sz, max_h, max_w, ignore)
    assert ref["valid"].all()
    if void_values(C, ignore):                                  # image 2 is wholly void: it has predictions and nothing else
        assert not ref["img_counts"][2, [0, 2]].any() and ref["img_counts"][2, 1].sum() == sizes[2][0] * sizes[2][1]
        assert ref["confusion"][C].sum() >= sizes[2][0] * sizes[2][1]
    for a in (x, data, offsets, sz, *(v for v in ref.values() if isinstance(v, np.ndarray))):
        a.setflags(write=False)
    return x, data, offsets, sz, max_h, max_w, ref


def run(x, data, offsets, sizes, max_h, max_w, dtype, layout, ignore=255, want_classes=True, conf=None):
    """raw mu_sem_eval_native; returns the outputs as numpy arrays (and the Guarded confusion buffer for a second call)"""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, C, h, w = x.shape
    tdt = TDT[dtype]
    if layout == "nchw":
        logits, args = np.array(x), (h * w, C * h * w, h * w, 1)
    else:                                                       # [B,h,w,Cp]: the padded channels hold a LARGER value than any real one
        Cp = (C + 8) // 8 * 8
        logits = np.full((B, h, w, Cp), 100.0, np.float32)
        logits[..., :C] = x.transpose(0, 2, 3, 1)
        args = (B * h * w, 0, 1, Cp)
    g_x = Guarded(logits.size, tdt, logits, "logits")
    g_lab = Guarded(data.size, torch.uint8, np.array(data), "labels")
    g_off = Guarded(B + 1, torch.int64, np.array(offsets), "offsets")
    g_siz = Guarded(2 * B, torch.int32, np.array(sizes), "sizes")
    g_counts = Guarded(B * 3 * C, torch.int32, name="img_counts")
    g_valid = Guarded(B, torch.uint8, name="valid")
    g_cls = Guarded(data.size, torch.uint8, name="classes")
    if conf is None:
        conf = Guarded((C + 1) * C, torch.int64, name="confusion")
        conf.t.zero_()
    nws = lib.mu_sem_eval_native_workspace_bytes(B, C, h, w, max_h, max_w)
    assert nws > 0 and nws % 8 == 0
    call("mu_sem_eval_native", g_x, B, C, h, w, *args, g_lab, g_off, g_siz, max_h, max_w, ignore, g_counts, conf, g_valid,
         g_cls if want_classes else None, Guarded(nws // 8, torch.int64, name="workspace"), nws, _lib.dt(tdt))
    g_cls.check()
    g_counts.all_written()
    return {"img_counts": g_counts.host((B, 3, C)), "confusion": conf.host((C + 1, C)), "valid": g_valid.host(), "classes": g_cls.host(),
            "conf_buffer": conf}


def check(what, got, ref, classes=True):
    assert np.array_equal(got["valid"], ref["valid"]), what + ": valid"
    if classes:                                                 # pred in every accepted span, the sentinel everywhere else
        assert np.array_equal(got["classes"], ref["classes"]), what + ": class map"
    else:
        assert (got["classes"] == 0xA5).all(), what + ": class map written although NULL was passed"
    assert np.array_equal(got["img_counts"], ref["img_counts"]), what + ": img_counts"
    assert np.array_equal(got["confusion"], ref["confusion"]), what + ": confusion"


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_dtype_and_layout_equals_the_restatement(src, C):
    x, data, offsets, sizes, max_h, max_w, ref = case(C, *src)
    for dtype in ("fp32", "fp16"):
        for layout in ("nchw", "nhwc"):
            check(f"{src} C={C} {dtype} {layout}", run(x, data, offsets, sizes, max_h, max_w, dtype, layout), ref)


@pytest.mark.parametrize("C", [2, 19, 150])
@pytest.mark.parametrize("src", [(8, 8), (16, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_take_the_first_maximum(src, C):
    """the exact cases of the host test: dyadic logits at x1, x4, x8, x1/2 and a mixed 2 x 4, every image with exact ties at the top"""
    x, data, offsets, sizes, max_h, max_w, ref = case(C, *src, kind="grid")
    for b, (H, W) in enumerate(sizes.tolist()):
        assert R.top_ties(R.upsample(x[b], H, W)) >= 1, (b, H, W)
    for dtype, layout in (("fp32", "nhwc"), ("fp16", "nchw")):
        check(f"ties {src} C={C} {dtype} {layout}", run(x, data, offsets, sizes, max_h, max_w, dtype, layout), ref)


def test_every_path_is_reached():
    """the cases above reach the window in LDS and the taps from global memory, the counters in LDS and the per-pixel global atomics"""
    sizes = batch_sizes(16, 12)
    for C in (150, 256):
        fits = [f for H, W in sizes for f in tiles_in_lds(C, 16, 12, H, W)]
        assert any(fits) and not all(fits), C
    assert all(f for C in (1, 2, 19) for src in SOURCES for H, W in batch_sizes(*src) for f in tiles_in_lds(C, *src, H, W))
    assert lds_plan(213, 16, 12) == (K["MU_SEM_NATIVE_WINDOW_BYTES"] // 4, True) and not lds_plan(214, 16, 12)[1]
    assert lds_plan(256, 1, 7)[1] and not lds_plan(256, 8, 8)[1] and lds_plan(193, 16, 12)[1]
    # the two window paths give the same results: 150 classes from a 16x12 source take the global taps for the identity image, 19 of
    # the same logits never do, and where channel 0..18 dominate both launches predict the same classes
    x, data, offsets, sizes_, max_h, max_w, ref = case(150, 16, 12)
    boosted = np.array(x)
    boosted[:, :19] += 16.0
    boosted = boosted.astype(np.float16).astype(np.float32)     # the launches below store fp16: keep the values exact in it
    want = R.native_eval(boosted, data, offsets, sizes_, max_h, max_w, 255)
    a = run(boosted, data, offsets, sizes_, max_h, max_w, "fp16", "nhwc")
    b = run(np.ascontiguousarray(boosted[:, :19]), data, offsets, sizes_, max_h, max_w, "fp16", "nhwc")
    check("C=150 16x12: tiles of both window paths in one launch", a, want)
    assert all(int(p.max()) < 19 for p in want["pred"]) and a["classes"].tobytes() == b["classes"].tobytes()


def refusal_case(reason):
    """the batch of case(19, 8, 8) with image 4 (and for a negative offset, by the span rule, image 3) refused"""
    x, data, offsets, sizes, max_h, max_w, _ = case(19, 8, 8)
    offsets, sizes = np.array(offsets), np.array(sizes)
    if reason == "size":
        sizes[4] = (0, 5)
    elif reason == "too large":
        sizes[4, 0] = max_h + 1
    elif reason == "offset":
        offsets[4] = -3
    else:
        sizes[4, 1] += 1                                        # inside the bounds, but one column more than its bytes hold
        assert sizes[4, 1] <= max_w and sizes[4, 0] * sizes[4, 1] > offsets[5] - offsets[4]
    return x, data, offsets, sizes, max_h, max_w


@pytest.mark.parametrize("reason", ["size", "too large", "offset", "span"])
def test_a_refused_image_in_the_middle(reason):
    x, data, offsets, sizes, max_h, max_w = refusal_case(reason)
    base = case(19, 8, 8)[-1]
    ref = R.native_eval(x, data, offsets, sizes, max_h, max_w, 255)
    refused = [3, 4] if reason == "offset" else [4]
    assert [b for b in range(len(sizes)) if not ref["valid"][b]] == refused
    keep = [b for b in range(len(sizes)) if b not in refused]
    assert np.array_equal(ref["img_counts"][keep], base["img_counts"][keep]) and not ref["img_counts"][refused].any()
    for dtype, layout in (("fp16", "nhwc"), ("fp32", "nchw")):
        got = run(x, data, offsets, sizes, max_h, max_w, dtype, layout)
        check(f"refused ({reason}) {dtype} {layout}", got, ref)
        assert not got["valid"][refused].any() and not got["img_counts"][refused].any()
        assert np.array_equal(got["img_counts"][keep], base["img_counts"][keep])              # the neighbours are unaffected
        o0, (H0, W0) = int(case(19, 8, 8)[2][4]), case(19, 8, 8)[3][4]
        assert (got["classes"][o0:o0 + H0 * W0] == 0xA5).all()                                # the refused span keeps its sentinel


@pytest.mark.parametrize("C,src", [(19, (8, 8)), (150, (16, 12)), (256, (8, 8))], ids=["lds", "lds-150", "global"])
def test_confusion_is_added_to_and_img_counts_are_overwritten(C, src):
    x, data, offsets, sizes, max_h, max_w, ref = case(C, *src)
    pre = (np.arange((C + 1) * C, dtype=np.int64).reshape(C + 1, C) % 7 + 1) * ((1 << 33) + 12345)
    conf = Guarded((C + 1) * C, torch.int64, name="confusion")
    conf.t.copy_(torch.from_numpy(pre.reshape(-1)))
    a = run(x, data, offsets, sizes, max_h, max_w, "fp16", "nhwc", conf=conf)
    assert np.array_equal(a["confusion"], pre + ref["confusion"])
    b = run(x, data, offsets, sizes, max_h, max_w, "fp16", "nhwc", conf=conf)
    assert np.array_equal(b["confusion"], pre + 2 * ref["confusion"])
    assert np.array_equal(b["img_counts"], ref["img_counts"])


@pytest.mark.parametrize("C,src,layout", [(150, (16, 12), "nhwc"), (256, (8, 8), "nchw"), (19, (1, 7), "nchw")])
def test_two_launches_are_byte_identical(C, src, layout):
    x, data, offsets, sizes, max_h, max_w, ref = case(C, *src)
    a, b = (run(x, data, offsets, sizes, max_h, max_w, "fp32", layout) for _ in range(2))
    for k in ("img_counts", "confusion", "valid", "classes"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_the_class_map_is_optional_and_ignore_index_may_be_none():
    x, data, offsets, sizes, max_h, max_w, ref = case(19, 8, 8)
    check("classes_or_null = NULL", run(x, data, offsets, sizes, max_h, max_w, "fp16", "nhwc", want_classes=False), ref, classes=False)
    x, data, offsets, sizes, max_h, max_w, ref = case(19, 8, 8, ignore=-100)
    assert ref["confusion"][19].sum() > 0 and not ref["confusion"][19].sum() == ref["confusion"].sum()       # void only through labels >= C
    check("ignore_index = -100", run(x, data, offsets, sizes, max_h, max_w, "fp32", "nchw", ignore=-100), ref)
    other = R.native_eval(x, data, offsets, sizes, max_h, max_w, 1 << 40)
    assert np.array_equal(other["confusion"], ref["confusion"])
    check("ignore_index = 2^40", run(x, data, offsets, sizes, max_h, max_w, "fp32", "nchw", ignore=1 << 40), ref)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------

def label_maps(C, sizes, seed):
    rng = np.random.default_rng(seed)
    maps = [rng.integers(0, C, (H, W)).astype(np.uint8) for H, W in sizes]
    for m in maps:
        m[rng.random(m.shape) < 0.1] = 255
    return maps


def reference_of(x, maps, ignore=255):
    offsets = np.concatenate([[0], np.cumsum([m.size for m in maps])]).astype(np.int64)
    sizes = np.asarray([m.shape for m in maps], np.int32)
    return R.native_eval(x, np.concatenate([m.reshape(-1) for m in maps]), offsets, sizes, int(sizes[:, 0].max()), int(sizes[:, 1].max()), ignore, fill=0)


@pytest.mark.parametrize("route", ["module_output", "plain_nchw", "padded_nhwc"])
def test_semantic_eval_native_and_class_maps(route):
    from maskunet_amd import ops, pack_images, semantic_eval_native
    from maskunet_amd.losses import _nhwc_source
    C, h, w = 19, 16, 12
    sizes = [(37, 53), (16, 12), (5, 3), (64, 96), (1, 1)]
    x = np.random.default_rng(11).standard_normal((len(sizes), C, h, w)).astype(np.float16).astype(np.float32)
    maps = label_maps(C, sizes, 12)
    ref = reference_of(x, maps)
    labels = pack_images(maps, device="cuda")
    nhwc = torch.full((len(sizes), h, w, 32), 100.0, dtype=torch.float16, device="cuda")
    nhwc[..., :C] = torch.from_numpy(x.transpose(0, 2, 3, 1).copy()).cuda()
    if route == "module_output":
        out = ops.to_nchw(nhwc, C)
        assert _nhwc_source(out) is not None
        batch = semantic_eval_native(out, labels, classes=True)
    elif route == "plain_nchw":
        batch = semantic_eval_native(torch.from_numpy(x).cuda(), labels, classes=True)
    else:
        batch = semantic_eval_native(nhwc, labels, num_classes=C, classes=True)
    assert np.array_equal(batch.img_counts.cpu().numpy(), ref["img_counts"])
    assert np.array_equal(batch.confusion.cpu().numpy(), ref["confusion"])
    assert batch.valid.cpu().tolist() == [1] * len(sizes)
    assert np.array_equal(batch.classes.cpu().numpy(), ref["classes"])
    views = batch.class_maps()
    for v, p, (H, W) in zip(views, ref["pred"], sizes):
        assert tuple(v.shape) == (H, W) and np.array_equal(v.cpu().numpy(), p)
        assert v.untyped_storage().data_ptr() == batch.classes.untyped_storage().data_ptr()   # a view, not a copy
    assert semantic_eval_native(torch.from_numpy(x).cuda(), labels).classes is None


def test_semantic_metrics_update_native_over_two_updates():
    from maskunet_amd import PackedImages, SemanticMetrics, metrics_from_counts, pack_images
    C, h, w = 19, 8, 8
    rng = np.random.default_rng(21)
    acc = SemanticMetrics(C, ignore_index=255)
    conf, counts = np.zeros((C + 1, C), np.int64), []
    for i, sizes in enumerate([[(21, 30), (8, 8), (64, 64)], [(5, 3), (33, 17)]]):
        x = rng.standard_normal((len(sizes), C, h, w)).astype(np.float16).astype(np.float32)
        maps = label_maps(C, sizes, 30 + i)
        ref = reference_of(x, maps)
        labels = pack_images(maps, device="cuda")
        if i == 1:                                              # the second image of the second update is refused: its height is 0
            bad = labels.sizes.clone()
            bad[1, 0] = 0
            labels = PackedImages(labels.data, labels.offsets, bad, 1, labels.max_h, labels.max_w)
            sz = np.asarray(sizes, np.int32)
            sz[1, 0] = 0
            off = np.concatenate([[0], np.cumsum([m.size for m in maps])]).astype(np.int64)
            ref = R.native_eval(x, np.concatenate([m.reshape(-1) for m in maps]), off, sz, labels.max_h, labels.max_w, 255)
            assert ref["valid"].tolist() == [1, 0]
        batch = acc.update_native(torch.from_numpy(x).cuda().half(), labels)
        assert batch.confusion is acc.confusion and batch.classes is None
        conf += ref["confusion"]
        counts.append(ref["img_counts"][ref["valid"] != 0])
    got = acc.compute()
    want = metrics_from_counts(conf, counts, [np.zeros((len(c), 2)) for c in counts])
    assert got.pop("refused") == 1 and set(got) == set(want)
    for k, r in want.items():
        if k == "reference":
            assert np.isnan(got[k]["loss"]) and got[k]["batch_miou"] == r["batch_miou"] and got[k]["image_miou"] == r["image_miou"]
        else:
            assert np.array_equal(got[k], r), k
    with pytest.raises(RuntimeError, match="cannot be mixed"):
        acc.update(torch.zeros(1, C, 8, 8, device="cuda"), torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda"))
