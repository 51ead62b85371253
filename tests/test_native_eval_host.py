"""CPU: the fp32 restatement of the native-resolution semantic evaluation (tests/_native_eval_reference.py, the rule of mu_sem_eval_native
in include/maskunet_hip.h) pinned to torch's F.interpolate(.., mode="bilinear", align_corners=False) + torch.argmax -- with == where the
arithmetic is exact (dyadic logits, power-of-two scale factors, real ties at the top) and at every pixel with a clear winner elsewhere --
its counts through metrics_from_counts against a brute-force confusion matrix, the refusals of the Python layer and of the C entry point
before any launch, and the header against the binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _native_eval_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maskunet_hip.h")
MU_ERR_ARG, MU_ERR_SHAPE, MU_ERR_WORKSPACE = -1, -2, -4


def torch_upsample(x, H, W):
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(x))[None], size=(H, W), mode="bilinear", align_corners=False)[0]


# ---- 1. exact cases: values and arg-max == torch, with real ties ----------------------------------------------------------------

@pytest.mark.parametrize("C", [2, 19, 150])
@pytest.mark.parametrize("h,w,H,W", [(16, 16, 16, 16), (16, 16, 64, 64), (16, 16, 64, 128), (16, 12, 128, 96), (8, 8, 64, 64), (16, 12, 8, 6),
                                     (8, 8, 4, 4), (1, 8, 8, 32)], ids=lambda v: str(v))
def test_exact_cases_equal_torch_bit_for_bit(C, h, w, H, W):
    x = R.grid_logits(1, C, h, w)[0]
    v = R.upsample(x, H, W)
    t = torch_upsample(x, H, W)
    ties = R.top_ties(v)
    print(f"{h}x{w} -> {H}x{W}, C = {C}: {ties} of {H * W} pixels have an exact tie at the top")
    assert ties >= 1
    assert v.tobytes() == t.numpy().tobytes()
    assert np.array_equal(R.first_argmax(v), torch.argmax(t, dim=0).numpy())


# ---- 2. general cases: the arg-max equals torch's wherever the winner is clear ---------------------------------------------------

@pytest.mark.parametrize("C", [19, 150])
@pytest.mark.parametrize("h,w,H,W", [(16, 12, 37, 53), (8, 8, 21, 30)], ids=lambda v: str(v))
def test_general_cases_agree_with_torch_where_the_top_two_gap_is_clear(C, h, w, H, W):
    x = np.random.default_rng(C + h).standard_normal((C, h, w)).astype(np.float32)
    v = R.upsample(x, H, W)
    t = torch_upsample(x, H, W)
    v64 = np.sort(R.upsample(x, H, W, np.float64), axis=0)
    clear = (v64[-1] - v64[-2]) > 1e-4
    left_out = 1.0 - clear.mean()
    dv = float(np.abs(v.astype(np.float64) - t.numpy()).max())
    print(f"{h}x{w} -> {H}x{W}, C = {C}: {left_out:.3%} of the pixels left out (condition: at most 1 %); values differ from torch by at most {dv:.2e}")
    assert left_out <= 0.01
    assert np.array_equal(R.first_argmax(v)[clear], torch.argmax(t, dim=0).numpy()[clear])
    assert np.abs(v.astype(np.float64) - R.upsample(x, H, W, np.float64)).max() <= 1e-5        # the fp32 rule is the float64 formula, rounded


# ---- 3. metrics: the restatement's counts through metrics_from_counts against a brute-force confusion matrix ----------------------

def ragged(sizes, rng, C, ignore=255, odd=True):
    """label bytes of a ragged batch: (data, offsets, sizes) with odd image starts and a gap; labels hold the ignore value and, for
    C < 255, values >= C"""
    offsets, chunks, at = [], [], 0
    for i, (H, W) in enumerate(sizes):
        gap = (1 if (at % 2 == 0) == odd else 0) + (6 if i == 2 else 0)
        chunks.append(np.full(gap, 0x5A, np.uint8))
        at += gap
        offsets.append(at)
        lab = rng.integers(0, C, H * W)
        kind = rng.random(H * W)
        lab[kind < 0.10] = ignore
        if C < 255:
            lab[(kind >= 0.10) & (kind < 0.15)] = rng.integers(C, 255)
        chunks.append(lab.astype(np.uint8))
        at += H * W
    offsets.append(at)
    return np.concatenate(chunks), np.asarray(offsets, np.int64), np.asarray(sizes, np.int32).reshape(-1, 2)


def test_metrics_from_counts_against_a_brute_force_confusion():
    from maskunet_amd.metrics import metrics_from_counts
    C, h, w = 19, 16, 12
    rng = np.random.default_rng(3)
    sizes = [(37, 53), (16, 12), (5, 3), (64, 48)]
    x = rng.standard_normal((len(sizes), C, h, w)).astype(np.float32)
    data, offsets, sz = ragged(sizes, rng, C)
    ref = R.native_eval(x, data, offsets, sz, 64, 53, 255)
    assert ref["valid"].tolist() == [1, 1, 1, 1]
    m = metrics_from_counts(ref["confusion"], [ref["img_counts"]], [np.zeros((len(sizes), 2))])
    conf = np.zeros((C, C), np.int64)
    for b, (H, W) in enumerate(sizes):                        # brute force, pixel by pixel
        pred = R.first_argmax(R.upsample(x[b], H, W)).reshape(-1)
        lab = data[offsets[b]:offsets[b] + H * W]
        for t, p in zip(lab.tolist(), pred.tolist()):
            if t != 255 and t < C:
                conf[t, p] += 1
    tp = np.diag(conf)
    union = conf.sum(0) + conf.sum(1) - tp
    assert np.array_equal(m["confusion"][:C], conf) and np.array_equal(m["tp"], tp)
    assert m["confusion"][C].sum() == sum(H * W for H, W in sizes) - conf.sum()
    iou = tp[union > 0] / union[union > 0]
    assert abs(m["miou"] - iou.mean()) <= 1e-12 and abs(m["pixel_accuracy"] - tp.sum() / conf.sum()) <= 1e-12
    assert np.isnan(m["reference"]["loss"])                  # no loss is defined at native resolution
    per_image = []
    for b, (H, W) in enumerate(sizes):
        I, P, L = ref["img_counts"][b].astype(np.float64)
        U = P + L - I
        per_image.append(np.mean((I[U > 0] + 1e-6) / (U[U > 0] + 1e-6)))
    assert abs(m["reference"]["image_miou"] - np.mean(per_image)) <= 1e-12


def test_restatement_refuses_like_the_contract():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 5, 4, 4)).astype(np.float32)
    data, offsets, sizes = ragged([(6, 5), (7, 3), (2, 9)], rng, 5)
    base = R.native_eval(x, data, offsets, sizes, 7, 9, 255)
    # a negative offsets[1] also leaves image 0 a negative span: the contract refuses both
    for what, (o, s, mh, valid) in {"size": (offsets, sizes, 6, [1, 0, 1]),
                                    "offset": (np.array([offsets[0], -1, offsets[2], offsets[3]]), sizes, 7, [0, 0, 1]),
                                    "span": (offsets, np.array([[6, 5], [7, 5], [2, 9]], np.int32), 7, [1, 0, 1])}.items():
        got = R.native_eval(x, data, o, s, mh, 9, 255)
        assert got["valid"].tolist() == valid and got["pred"][1] is None and not got["img_counts"][1].any(), what
        keep = [b for b in range(3) if valid[b]]
        assert np.array_equal(got["img_counts"][keep], base["img_counts"][keep])
        a, b = int(offsets[1]), int(offsets[2])
        assert (got["classes"][a:b] == 0xA5).all() and np.array_equal(got["classes"][b:], base["classes"][b:])


# ---- 4. refusals before any launch ------------------------------------------------------------------------------------------------

def packed(sizes, channels=1):
    from maskunet_amd import pack_images
    return pack_images([np.zeros((H, W) if channels == 1 else (H, W, channels), np.uint8) for H, W in sizes])


def test_python_layer_refuses_before_any_launch():
    from maskunet_amd import semantic_eval_native
    lab = packed([(5, 7), (9, 4)])
    with pytest.raises(RuntimeError, match="1 <= num_classes <= 256"):
        semantic_eval_native(torch.zeros(2, 257, 8, 8), lab)
    with pytest.raises(RuntimeError, match="1 <= num_classes <= 256"):
        semantic_eval_native(torch.zeros(2, 0, 8, 8), lab)
    with pytest.raises(RuntimeError, match="1 <= num_classes <= 256"):
        semantic_eval_native(torch.zeros(2, 8, 8, 32), lab, num_classes=0)
    with pytest.raises(RuntimeError, match="h \\* w <= 65536"):
        semantic_eval_native(torch.zeros(2, 2, 256, 257), lab)
    with pytest.raises(RuntimeError, match="one channel"):
        semantic_eval_native(torch.zeros(2, 19, 8, 8), packed([(5, 7), (9, 4)], 3))
    with pytest.raises(RuntimeError, match="PackedImages"):
        semantic_eval_native(torch.zeros(2, 19, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="neither"):
        semantic_eval_native(torch.zeros(3, 19, 8, 8), lab)
    for bad in (torch.zeros(19, 19, dtype=torch.int64), torch.zeros(20, 19, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="confusion must be"):
            semantic_eval_native(torch.zeros(2, 19, 8, 8), lab, confusion=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        semantic_eval_native(torch.zeros(2, 19, 8, 8), lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        semantic_eval_native(torch.zeros(2, 8, 8, 32), lab, num_classes=19, confusion=torch.zeros(20, 19, dtype=torch.int64))


def test_one_metrics_object_takes_one_kind_of_update(monkeypatch):
    from maskunet_amd import SemanticMetrics, metrics
    C = 4
    counts, loss, valid = torch.zeros(2, 3, C, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.float64), torch.tensor([1, 0], dtype=torch.uint8)
    counts[0, :, 1] = 5
    monkeypatch.setattr(metrics, "semantic_eval", lambda o, l, n, i, t, c, conf: metrics.SemanticBatch(counts, loss, conf))
    monkeypatch.setattr(metrics, "semantic_eval_native", lambda o, l, n, i, c, conf: metrics.SemanticNativeBatch(counts, conf, valid, None, None, None))
    out = torch.zeros(2, C, 8, 8)
    a = SemanticMetrics(C)
    a.update(out, None)
    with pytest.raises(RuntimeError, match="cannot be mixed"):
        a.update_native(out, None)
    assert "refused" not in a.compute()
    b = SemanticMetrics(C)
    b.update_native(out, None)
    b.update_native(out, None)
    with pytest.raises(RuntimeError, match="cannot be mixed"):
        b.update(out, None)
    got = b.compute()
    assert got["refused"] == 2 and np.isnan(got["reference"]["loss"]) and got["reference"]["image_miou"] == 1.0
    b.reset()
    b.update(out, None)                                      # after reset() either kind is taken again
    with pytest.raises(RuntimeError, match="class map"):
        metrics.SemanticNativeBatch(counts, None, valid, None, None, None).class_maps()


def test_entry_point_refuses_before_any_launch():
    from maskunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 8
    nws = lib.mu_sem_eval_native_workspace_bytes(2, 19, 8, 8, 40, 50)
    assert nws > 0

    def run(**kw):
        a = dict(logits=p, B=2, C=19, h=8, w=8, inner=128, outer=0, cs=1, ps=32, labels=p, offsets=p, sizes=p, max_h=40, max_w=50, ignore=255,
                 counts=p, conf=p, valid=p, classes=None, ws=p, nws=nws, dtype=_lib.MU_F16)
        a.update(kw)
        return lib.mu_sem_eval_native(*a.values(), None)

    for name in ("logits", "labels", "offsets", "sizes", "counts", "conf", "valid", "ws"):
        assert run(**{name: None}) == MU_ERR_ARG, name
    assert run(ws=p + 4) == MU_ERR_ARG
    assert run(B=0) == MU_ERR_ARG and run(inner=0) == MU_ERR_ARG and run(dtype=2) == MU_ERR_ARG and run(dtype=7) == MU_ERR_ARG
    assert run(max_h=0) == MU_ERR_ARG and run(max_w=0) == MU_ERR_ARG and run(max_h=16385) == MU_ERR_ARG and run(max_w=16385) == MU_ERR_ARG
    assert run(C=0) == MU_ERR_SHAPE and run(C=257) == MU_ERR_SHAPE and run(h=0) == MU_ERR_SHAPE and run(w=0) == MU_ERR_SHAPE
    assert run(h=256, w=257) == MU_ERR_SHAPE
    assert run(B=8192, max_h=16384, max_w=16384, nws=1 << 30) == MU_ERR_SHAPE          # 8192 * 1024 * 256 tiles = 2^31
    assert run(nws=nws - 1) == MU_ERR_WORKSPACE and run(nws=0) == MU_ERR_WORKSPACE


def test_queries_are_host_only():
    from maskunet_amd import _lib
    lib = _lib.load()
    sup = lib.mu_sem_eval_native_supported
    assert [sup(c, 8, 8) for c in (-1, 0, 1, 150, 256, 257)] == [MU_ERR_SHAPE, MU_ERR_SHAPE, 0, 0, 0, MU_ERR_SHAPE]
    assert sup(19, 256, 256) == 0 and sup(19, 1, 65536) == 0 and sup(19, 1, 65537) == MU_ERR_SHAPE and sup(19, 0, 5) == MU_ERR_SHAPE
    q = lib.mu_sem_eval_native_workspace_bytes
    assert q(8, 19, 128, 128, 1024, 2048) > 0 and q(8, 19, 128, 128, 1024, 2048) % 8 == 0 and q(1, 1, 1, 1, 1, 1) > 0
    assert q(0, 19, 8, 8, 10, 10) == 0 and q(2, 257, 8, 8, 10, 10) == 0 and q(2, 19, 256, 257, 10, 10) == 0
    assert q(2, 19, 8, 8, 0, 10) == 0 and q(2, 19, 8, 8, 10, 16385) == 0


# ---- 5. header and binding --------------------------------------------------------------------------------------------------------

def test_header_declares_the_three_symbols_and_the_binding_matches():
    from maskunet_amd import _lib
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"int": _lib.I, "long": _lib.L, "float": _lib.F}
    for name in ("mu_sem_eval_native_supported", "mu_sem_eval_native_workspace_bytes", "mu_sem_eval_native"):
        m = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name + " is not declared in maskunet_hip.h"
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        want = [_lib.P if "*" in a else ctype[a.split()[0]] for a in args]
        assert _lib.SIGNATURES[name] == (ctype[m.group(1)], want), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "This is the formula of torch's upsample_bilinear2d(align_corners=False).  It agrees with torch bit for bit where the arithmetic is" in src
    assert "exact, and only to within rounding elsewhere" in src
    consts = {k: int(v) for k, v in re.findall(r"#define (MU_SEM_NATIVE_[A-Z_]+) (\d+)", src)}
    assert consts["MU_SEM_NATIVE_TILE_H"] * consts["MU_SEM_NATIVE_TILE_W"] < 65536           # two 16-bit counters per LDS word
    assert consts["MU_SEM_NATIVE_WINDOW_BYTES"] <= consts["MU_SEM_NATIVE_LDS_BYTES"] <= 160 * 1024
    assert (3 * 256 + (257 * 256 + 1) // 2) * 4 <= consts["MU_SEM_NATIVE_LDS_BYTES"]          # the counters of C = 256 alone fit


def test_public_names():
    import maskunet_amd
    for name in ("semantic_eval_native", "SemanticNativeBatch"):
        assert name in maskunet_amd.__all__ and hasattr(maskunet_amd, name)
    assert hasattr(maskunet_amd.SemanticMetrics, "update_native")
