"""GPU: Pillow's antialiased bilinear resize of a ragged batch on the device (mu_pil_resize_u8_nhwc, maskunet_amd.images) against the numpy
restatement in tests/_pil_reference.py and, at 128x128, against the committed bytes of a real Pillow (tests/golden/pil/).  The contract is
integer arithmetic on fp64-derived integer coefficients, so every comparison is ==: the resized bytes, dst = byte / 255 bit for bit in fp32
and fp16, zero padding channels, swap_rb, u8_out = NULL, valid.  ONE ragged batch per channel count (and three very wide images beside it, for the rows that span several LDS tiles); the references are
computed once and shared.  Memory discipline as in test_gpu_poly.py: outputs pre-filled with a sentinel, 4 KiB guard bands around every buffer, inputs
verified untouched.  The refused images are ordinary validated inputs: no test provokes a fault."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _pil_reference as R
from tests._device_buffers import Guarded, call

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pil")
MAX_H, MAX_W = 2048, 1000                              # the bounds of the valid images
# (h, w) the device is told, (h, w) of the bytes that are really there: all three get valid = 0 and zeros, the neighbours are unaffected
REFUSED = [((1001, 10), (1001, 10)),                   # taller than 100 widths
           ((0, 5), (0, 0)),                           # no rows
           ((8, 1001), (8, 1001))]                     # w > max_w
# where the refused images sit among the 17 valid ones: first, in the middle, last
SLOTS = (0, 9, 19)
CP = 32
# beside the batch: rows wider than one LDS tile of the resample kernel (2042 pixels at C = 3, 2032 at C = 1), so that the horizontal sum of
# an output column runs over two and three tiles; image index WIDE0 + k
WIDE = [(2, 2500), (3, 4100), (5, 2043)]
WIDE0 = 100


@functools.lru_cache(maxsize=None)
def fixtures():
    return R.load_fixtures(GOLDEN)[0]


@functools.lru_cache(maxsize=None)
def image(i, C):
    """image i of the batch (an index into R.SIZES; its content rotates with i), refused image i - len(R.SIZES), or wide image i - WIDE0"""
    if i >= WIDE0:
        return R.pattern(*WIDE[i - WIDE0], C, R.kind_of(i))
    if i < len(R.SIZES):
        return R.pattern(*R.SIZES[i], C, R.kind_of(i))
    h, w = REFUSED[i - len(R.SIZES)][1]
    return R.pattern(h, w, C, "noise") if h else np.zeros((0, 0, C) if C > 1 else (0, 0), np.uint8)


def told_size(i):
    if i >= WIDE0:
        return WIDE[i - WIDE0]
    return R.SIZES[i] if i < len(R.SIZES) else REFUSED[i - len(R.SIZES)][0]


@functools.lru_cache(maxsize=None)
def expected(i, C, out_hw):
    """(bytes [Hd, Wd, C], valid) of image i at out_hw: the restatement, checked against Pillow's own bytes where a fixture exists"""
    Hd, Wd = out_hw
    if i >= WIDE0:
        return R.resize(image(i, C), out_hw).reshape(Hd, Wd, C), 1
    if i >= len(R.SIZES):
        return np.zeros((Hd, Wd, C), np.uint8), 0
    h, w = R.SIZES[i]
    ref = R.resize(image(i, C), out_hw)
    fx = fixtures().get(R.fixture_key(h, w, C, R.kind_of(i), Hd, Wd))
    assert out_hw != (128, 128) or fx is not None
    if fx is not None:
        assert np.array_equal(ref, fx), f"restatement and Pillow fixture differ for {(h, w, C, out_hw)}"
    return ref.reshape(Hd, Wd, C), 1


@functools.lru_cache(maxsize=None)
def order(which):
    """the images of the batch as indices: 'a' = R.SIZES in order with the refused ones at SLOTS; 'b' = another order, so that every image
    meets another start alignment mod 16; 'wide' = the images of WIDE; a single index = that image alone"""
    if isinstance(which, int):
        return (which,)
    if which == "wide":
        return tuple(range(WIDE0, WIDE0 + len(WIDE)))
    n = len(R.SIZES)
    idx = list(range(n))
    if which == "b":
        idx = idx[5:] + idx[:5]
        idx[1], idx[-2] = idx[-2], idx[1]
    for k, slot in enumerate(SLOTS):
        idx.insert(slot, n + k)
    return tuple(idx)


def run(which, C, out_hw, dtype, swap_rb=0, with_u8=True, max_hw=(MAX_H, MAX_W)):
    """one call through the C ABI on guarded buffers -> (bytes or None, dst, valid) as numpy, and the image indices"""
    from maskunet_amd import _lib
    idx = order(which)
    Hd, Wd = out_hw
    B = len(idx)
    flat = [image(i, C).reshape(-1) for i in idx]
    offsets = np.concatenate([[0], np.cumsum([f.size for f in flat])]).astype(np.int64)
    sizes = np.asarray([told_size(i) for i in idx], np.int32)
    src = Guarded(int(offsets[-1]), torch.uint8, np.concatenate(flat), "src")
    off = Guarded(B + 1, torch.int64, offsets, "offsets")
    siz = Guarded(2 * B, torch.int32, sizes, "sizes")
    dst = Guarded(B * Hd * Wd * CP, dtype, name="dst")
    u8 = Guarded(B * Hd * Wd * C, torch.uint8, name="u8_out") if with_u8 else None
    valid = Guarded(B, torch.uint8, name="valid")
    nbytes = _lib.load().mu_pil_resize_workspace_bytes(B, *max_hw, Hd, Wd)
    assert nbytes > 0
    ws = Guarded(nbytes, torch.uint8, name="workspace")
    call("mu_pil_resize_u8_nhwc", src, off, siz, B, C, *max_hw, swap_rb, dst, u8, valid, Hd, Wd, CP, _lib.dt(dtype), ws, nbytes)
    dst.all_written()
    return (u8.host((B, Hd, Wd, C)) if with_u8 else None), dst.host((B, Hd, Wd, CP)), valid.host(), idx


def check(got_u8, got_dst, got_valid, idx, C, out_hw, dtype, swap_rb=0):
    np_dtype = np.float32 if dtype == torch.float32 else np.float16
    bits = np.uint32 if dtype == torch.float32 else np.uint16
    for b, i in enumerate(idx):
        want, ok = expected(i, C, out_hw)
        if swap_rb and C == 3:
            want = want[:, :, ::-1]
        what = f"image {b} = {told_size(i)} x {C} -> {out_hw}"
        assert int(got_valid[b]) == ok, what
        if got_u8 is not None:
            bad = got_u8[b] != want
            assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ, first at {tuple(np.argwhere(bad)[0])}"
        unit = R.to_unit(want, np_dtype)
        assert np.array_equal(got_dst[b, :, :, :C].view(bits), unit.view(bits)), f"{what}: dst is not byte / 255"
        assert not got_dst[b, :, :, C:].view(bits).any(), f"{what}: padding channels are not +0"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("out_hw", R.OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 3])
def test_ragged_batch(C, out_hw, dtype):
    u8, dst, valid, idx = run("a", C, out_hw, dtype)
    assert valid.tolist() == [0 if i >= len(R.SIZES) else 1 for i in idx] and valid.sum() == len(R.SIZES)
    check(u8, dst, valid, idx, C, out_hw, dtype)


@pytest.mark.parametrize("out_hw", R.OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 3])
def test_other_packing_order(C, out_hw):
    """the same images at other start alignments: the head and tail of the 16-byte loads"""
    starts = lambda which: {i: o % 16 for i, o in zip(order(which), np.cumsum([0] + [image(i, C).size for i in order(which)]))}
    a, b = starts("a"), starts("b")
    assert sum(a[i] != b[i] for i in range(len(R.SIZES))) >= len(R.SIZES) // 2
    u8, dst, valid, idx = run("b", C, out_hw, torch.float16)
    check(u8, dst, valid, idx, C, out_hw, torch.float16)


@pytest.mark.parametrize("C", [1, 3])
def test_swap_rb_and_no_u8_out(C):
    u8, dst, valid, idx = run("a", C, (128, 128), torch.float32, swap_rb=1, with_u8=False)
    check(None, dst, valid, idx, C, (128, 128), torch.float32, swap_rb=1)
    u8, dst, valid, idx = run("a", C, (96, 80), torch.float16, swap_rb=1)
    check(u8, dst, valid, idx, C, (96, 80), torch.float16, swap_rb=1)


@pytest.mark.parametrize("i", [R.SIZES.index(s) for s in [(480, 640), (5, 7), (3, 1000), (2048, 64)]] + [len(R.SIZES)],
                         ids=["480x640", "5x7", "3x1000", "2048x64", "refused"])
def test_single_image(i):
    for out_hw in ((128, 128), (3, 5)):
        u8, dst, valid, idx = run(i, 3, out_hw, torch.float16)
        check(u8, dst, valid, idx, 3, out_hw, torch.float16)


@pytest.mark.parametrize("out_hw", [(3, 5), (2, 1), (4, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 3])
def test_rows_wider_than_one_tile(C, out_hw):
    """2500 .. 4100 taps per output column at Wd = 1; two workgroups of columns whose windows start in different tiles at Wd = 70"""
    u8, dst, valid, idx = run("wide", C, out_hw, torch.float32, max_hw=(5, 4100))
    check(u8, dst, valid, idx, C, out_hw, torch.float32)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def test_resize_pil_to_nhwc_list_and_uniform_tensor():
    from maskunet_amd import pack_images, resize_pil_to_nhwc
    idx = [R.SIZES.index(s) for s in [(427, 640), (5, 7), (97, 213), (128, 128)]]
    imgs = [torch.from_numpy(image(i, 3)).to(DEV) for i in idx]
    y, u8, valid = resize_pil_to_nhwc(imgs, (128, 128), torch.float16, return_u8=True)
    assert y.shape == (4, 128, 128, 32) and y.dtype == torch.float16 and u8.shape == (4, 128, 128, 3) and valid.tolist() == [1] * 4
    check(u8.cpu().numpy(), y.cpu().numpy(), valid.cpu().numpy(), idx, 3, (128, 128), torch.float16)
    # host images and a device: one copy; grey images; (y, valid) without the bytes
    y1, v1 = resize_pil_to_nhwc([image(i, 1) for i in idx], (96, 80), torch.float32, device=DEV)
    check(None, y1.cpu().numpy(), v1.cpu().numpy(), idx, 1, (96, 80), torch.float32)
    # a uniform [B, H, W, C] tensor; bgr
    i = R.SIZES.index((480, 640))
    t = torch.from_numpy(np.stack([image(i, 3), image(i, 3)[::-1, ::-1].copy()])).to(DEV)
    y2, u2, v2 = resize_pil_to_nhwc(t, (128, 128), torch.float32, bgr=True, return_u8=True)
    assert v2.tolist() == [1, 1]
    assert np.array_equal(u2[0].cpu().numpy(), expected(i, 3, (128, 128))[0][:, :, ::-1])
    assert np.array_equal(u2[1].cpu().numpy(), R.resize(t[1].cpu().numpy(), (128, 128))[:, :, ::-1])
    # a packed batch is taken as it is; a refused image reports valid = 0 and does not raise
    p = pack_images([torch.from_numpy(image(len(R.SIZES), 3)).to(DEV), imgs[1]])
    y3, v3 = resize_pil_to_nhwc(p, (128, 128), torch.float16)
    assert v3.tolist() == [0, 1] and not y3[0].any()
    with pytest.raises(ValueError, match="RGBA"):
        resize_pil_to_nhwc(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=DEV))


@functools.lru_cache(maxsize=None)
def model():
    import maskunet_amd
    torch.manual_seed(3)
    m = maskunet_amd.UNet(3, 5).to(DEV).eval()
    rng_keep = [(torch.arange(2 * k).reshape(2, k) * 7 % 3 != 0).to(torch.uint8).to(DEV) for k in (4096, 1024, 256, 1024, 4096, 16384)]
    m.set_keep_masks(rng_keep)
    return m


def test_forward_u8_pil_equals_forward_of_the_reference_resize():
    m = model()
    idx = [R.SIZES.index(s) for s in [(480, 640), (51, 333)]]
    imgs = [torch.from_numpy(image(i, 3)).to(DEV) for i in idx]
    host = np.stack([R.to_unit(expected(i, 3, (128, 128))[0]).transpose(2, 0, 1) for i in idx])          # ToTensor: CHW float32
    with torch.no_grad():
        a = m.forward_u8(imgs, resample="pil", check=True)
        b = m(torch.from_numpy(host).to(DEV))
        assert torch.equal(a, b)
        bgr = m.forward_u8([im.flip(-1) for im in imgs], bgr=True, resample="pil")
        assert torch.equal(bgr, b)
        with pytest.raises(RuntimeError, match="refused"):
            m.forward_u8([torch.from_numpy(image(len(R.SIZES), 3)).to(DEV)], resample="pil", check=True)
        with pytest.raises(ValueError, match="resample"):
            m.forward_u8(imgs[0][None], resample="lanczos")


def test_forward_u8_cv2_is_unchanged():
    from maskunet_amd import ops
    m = model()
    t = torch.from_numpy(np.stack([image(R.SIZES.index((97, 213)), 3)] * 2)).to(DEV)
    with torch.no_grad():
        today = m._finish(m.forward_nhwc(ops.resize_u8_to_nhwc(t, (128, 128), m.compute_dtype, bgr=True)))
        assert torch.equal(m.forward_u8(t, bgr=True), today) and torch.equal(m.forward_u8(t, bgr=True, resample="cv2"), today)
        pil = m.forward_u8(t, bgr=True, resample="pil")
    assert not torch.equal(pil, today)                       # the two rules are different inputs to the network


# ---- repeatability ----------------------------------------------------------------------------------------------------------------
def test_repeatable_and_graph_capturable():
    from maskunet_amd import pack_images, resize_pil_to_nhwc
    idx = [R.SIZES.index(s) for s in [(640, 480), (1, 7), (300, 128), (3, 1000)]]
    p = pack_images([torch.from_numpy(image(i, 3)).to(DEV) for i in idx])
    y0, u0, v0 = resize_pil_to_nhwc(p, (128, 128), torch.float16, return_u8=True)
    y1, u1, v1 = resize_pil_to_nhwc(p, (128, 128), torch.float16, return_u8=True)
    assert torch.equal(u0, u1) and torch.equal(y0.view(torch.int16), y1.view(torch.int16)) and torch.equal(v0, v1)
    check(u0.cpu().numpy(), y0.cpu().numpy(), v0.cpu().numpy(), idx, 3, (128, 128), torch.float16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg, ug, vg = resize_pil_to_nhwc(p, (128, 128), torch.float16, return_u8=True)
    for t in (yg, ug, vg):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ug, u0) and torch.equal(yg.view(torch.int16), y0.view(torch.int16)) and torch.equal(vg, v0)
