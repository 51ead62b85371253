"""GPU: the ragged cv2 sample preparation (mu_cv2_resize_ragged_u8_nhwc, mu_cv2_nearest_ragged, mu_panoptic_targets, maskunet_amd.targets)
against the numpy restatement in tests/_targets_reference.py, whose resizes are oracle/cv2_resize_oracle.py's, and -- the images -- against
mu_resize_u8_nhwc called per image on the same bytes.  Everything is integer arithmetic on fp64-derived indices and coefficients, so every
comparison is ==: bytes, dst = byte / 255 bit for bit in fp32 and fp16, +0 padding channels, int64 targets, valid.  The C ABI is called on
guarded buffers (tests/_device_buffers.py): outputs pre-filled with a sentinel, 4 KiB guard bands, inputs verified untouched.  ONE ragged
batch per channel count; the references are computed once and shared.  The refused images are ordinary validated inputs (no rows, wider
than max_w, a slot shorter than h * w * C, a misaligned 16-bit start, a table out of order): no test provokes a fault."""
import functools

import numpy as np
import pytest
import torch

from tests import _targets_reference as R
from tests._device_buffers import Guarded, call, side_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_SIZES = [(8, 8), (5, 3), (128, 128)]                   # (Wd, Hd), like cv2
CP = 8                                                     # the kernel's own granularity (two fp32 vectors, one fp16 vector per pixel)
# (h, w) of the valid images: degenerate ones; 5x7 upscales everywhere, so its left taps collapse; per output size one image exactly 2x in
# both axes (the INTER_AREA shortcut, decided per image: its neighbours take none), one 2x in one axis only and one at the output size
# (the identity); then the mixed ones
SIZES = [(1, 1), (1, 9), (9, 1), (5, 7),
         (16, 16), (6, 10), (256, 256),
         (16, 8), (6, 5), (256, 128),
         (8, 8), (3, 5), (128, 128),
         (97, 213), (3, 1000), (300, 128)]
MAX_H, MAX_W = 300, 1000                                   # the bounds of the valid images
# (h, w) the device is told, (h, w) of the bytes that are there
REFUSED = [((0, 5), (0, 0)),                               # no rows
           ((8, 1001), (8, 1001)),                         # w > max_w
           ((10, 10), (10, 9))]                            # a slot shorter than h * w * C
NV = len(SIZES)
SLOTS = (0, 8, NV + 2)                                     # where the refused images sit: first, in the middle, last
BIG = 100                                                  # image index of the largest reference-sized image, 1024 x 2048 (Cityscapes), alone
BIG_HW = (1024, 2048)


def np_of(dtype):
    return (np.float32, np.uint32) if dtype == torch.float32 else (np.float16, np.uint16)


@functools.lru_cache(maxsize=None)
def image(i, C):
    """valid image i, refused image i - NV, or the big one: uint8 [h, w, C]"""
    h, w = BIG_HW if i == BIG else (SIZES[i] if i < NV else REFUSED[i - NV][1])
    return (R.noise(h, w, C, salt=i) >> 9).astype(np.uint8)


def told_size(i):
    return BIG_HW if i == BIG else (SIZES[i] if i < NV else REFUSED[i - NV][0])


@functools.lru_cache(maxsize=None)
def expected(i, C, out):
    """(bytes [Hd, Wd, C], valid) of image i at out = (Wd, Hd) by the oracle"""
    if i != BIG and i >= NV:
        return np.zeros((out[1], out[0], C), np.uint8), 0
    return R.image_bytes(image(i, C), out), 1


@functools.lru_cache(maxsize=None)
def order(which):
    if isinstance(which, int):
        return (which,)
    idx = list(range(NV))
    if which == "b":                                       # another order: other start alignments mod 16
        idx = idx[3:] + idx[:3]
        idx[1], idx[-2] = idx[-2], idx[1]
    for k, slot in enumerate(SLOTS):
        idx.insert(slot, NV + k)
    return tuple(idx)


def starts(which, C):
    idx = order(which)
    return dict(zip(idx, np.cumsum([0] + [image(i, C).size for i in idx]).tolist()))


def ragged(arrays, told):
    """flat bytes, offsets, sizes of a batch as three Guarded inputs"""
    flat = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]
    offsets = np.concatenate([[0], np.cumsum([f.size for f in flat])]).astype(np.int64)
    return (Guarded(int(offsets[-1]), torch.uint8, np.concatenate(flat), "src"), Guarded(len(flat) + 1, torch.int64, offsets, "offsets"),
            Guarded(2 * len(flat), torch.int32, np.asarray(told, np.int32), "sizes"))


def run_images(which, C, out, dtype, swap_rb=0, with_u8=True, max_hw=(MAX_H, MAX_W)):
    from maskunet_amd import _lib
    idx = order(which)
    Wd, Hd = out
    B = len(idx)
    src, off, siz = ragged([image(i, C) for i in idx], [told_size(i) for i in idx])
    dst = Guarded(B * Hd * Wd * CP, dtype, name="dst")
    u8 = Guarded(B * Hd * Wd * C, torch.uint8, name="u8_out") if with_u8 else None
    valid = Guarded(B, torch.uint8, name="valid")
    call("mu_cv2_resize_ragged_u8_nhwc", src, off, siz, B, C, *max_hw, swap_rb, dst, u8, valid, Hd, Wd, CP, _lib.dt(dtype))
    dst.all_written()
    valid.all_written()
    return (u8.host((B, Hd, Wd, C)) if with_u8 else None), dst.host((B, Hd, Wd, CP)), valid.host(), idx


@functools.lru_cache(maxsize=None)
def uniform(i, C, out, dtype, swap_rb):
    """what mu_resize_u8_nhwc gives for image i alone as [1, h, w, C]: (bytes, dst) as numpy"""
    from maskunet_amd import _lib
    Wd, Hd = out
    h, w = told_size(i)
    src = torch.from_numpy(image(i, C)).to(DEV)
    dst = torch.empty((Hd, Wd, CP), dtype=dtype, device=DEV)
    u8 = torch.empty((Hd, Wd, C), dtype=torch.uint8, device=DEV)
    _lib.call("mu_resize_u8_nhwc", src.data_ptr(), 1, h, w, C, swap_rb, dst.data_ptr(), u8.data_ptr(), Hd, Wd, CP, _lib.dt(dtype), _lib.stream())
    return u8.cpu().numpy(), dst.cpu().numpy()


def check_images(got_u8, got_dst, got_valid, idx, C, out, dtype, swap_rb=0):
    ft, bits = np_of(dtype)
    for b, i in enumerate(idx):
        want, ok = expected(i, C, out)
        if swap_rb and C == 3:
            want = want[:, :, ::-1]
        what = f"image {b} = {told_size(i)} x {C} -> {out}"
        assert int(got_valid[b]) == ok, what
        if got_u8 is not None:
            bad = got_u8[b] != want
            assert not bad.any(), f"{what}: {int(bad.sum())} bytes differ from the oracle, first at {tuple(np.argwhere(bad)[0])}"
        assert np.array_equal(got_dst[b, :, :, :C].view(bits), R.to_unit(want, ft).view(bits)), f"{what}: dst is not byte / 255"
        assert not got_dst[b, :, :, C:].view(bits).any(), f"{what}: padding channels are not +0"
        if ok:                                             # and the uniform kernel on the same bytes, bit for bit
            u_u8, u_dst = uniform(i, C, out, dtype, swap_rb)
            if got_u8 is not None:
                assert np.array_equal(got_u8[b], u_u8), f"{what}: bytes differ from mu_resize_u8_nhwc"
            assert np.array_equal(got_dst[b].view(bits), u_dst.view(bits)), f"{what}: dst differs from mu_resize_u8_nhwc"


# ---- images -----------------------------------------------------------------------------------------------------------------------
def test_the_batch_holds_the_shapes_it_claims():
    for Wd, Hd in OUT_SIZES:
        assert [s for s in SIZES if s == (2 * Hd, 2 * Wd)] and (2 * Hd, Wd) in SIZES and (Hd, Wd) in SIZES
        assert sum(s == (2 * Hd, 2 * Wd) for s in SIZES) == 1
    idx = order("a")
    assert idx[0] >= NV and idx[-1] >= NV and idx[8] >= NV and len(idx) == NV + 3
    for C in (1, 3):
        a, b = starts("a", C), starts("b", C)
        assert sum(a[i] % 16 != b[i] % 16 for i in range(NV)) > NV // 2


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("out", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 3])
def test_ragged_batch(C, out, dtype):
    u8, dst, valid, idx = run_images("a", C, out, dtype)
    assert valid.tolist() == [0 if i >= NV else 1 for i in idx] and valid.sum() == NV
    check_images(u8, dst, valid, idx, C, out, dtype)
    i2 = idx.index(SIZES.index((2 * out[1], 2 * out[0])))  # the image that took the shortcut: (a + b + c + d + 2) >> 2
    a = image(idx[i2], C).astype(np.int64)
    assert np.array_equal(u8[i2], ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    assert np.array_equal(u8[idx.index(SIZES.index((out[1], out[0])))], image(SIZES.index((out[1], out[0])), C))       # the identity


@pytest.mark.parametrize("out", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 3])
def test_other_packing_order(C, out):
    u8, dst, valid, idx = run_images("b", C, out, torch.float16)
    check_images(u8, dst, valid, idx, C, out, torch.float16)


@pytest.mark.parametrize("C", [1, 3])
def test_swap_rb_and_no_u8_out(C):
    u8, dst, valid, idx = run_images("a", C, (128, 128), torch.float32, swap_rb=1, with_u8=False)
    check_images(None, dst, valid, idx, C, (128, 128), torch.float32, swap_rb=1)
    u8, dst, valid, idx = run_images("a", C, (5, 3), torch.float16, swap_rb=1)
    check_images(u8, dst, valid, idx, C, (5, 3), torch.float16, swap_rb=1)


def test_largest_reference_image_alone():
    u8, dst, valid, idx = run_images(BIG, 3, (128, 128), torch.float16, swap_rb=1, max_hw=BIG_HW)
    check_images(u8, dst, valid, idx, 3, (128, 128), torch.float16, swap_rb=1)


def test_image_arguments_are_refused_before_any_launch():
    from maskunet_amd import _lib
    lib = _lib.load()
    src, off, siz = ragged([image(3, 3)], [told_size(3)])
    dst, valid = Guarded(8 * 8 * CP, torch.float16, name="dst"), Guarded(1, torch.uint8, name="valid")
    good = [src.p, off.p, siz.p, 1, 3, 5, 7, 0, dst.p, None, valid.p, 8, 8, CP, _lib.MU_F16, _lib.stream()]
    def rc(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.mu_cv2_resize_ragged_u8_nhwc(*a)
    assert rc(a0=None) == -1 and rc(a1=None) == -1 and rc(a2=None) == -1 and rc(a8=None) == -1 and rc(a10=None) == -1
    assert rc(a3=0) == -1 and rc(a14=2) == -1
    assert rc(a4=2) == -2 and rc(a4=4) == -2 and rc(a13=4) == -2 and rc(a13=0) == -2
    assert rc(a5=0) == -2 and rc(a6=16385) == -2 and rc(a11=0) == -2 and rc(a12=16385) == -2
    torch.cuda.synchronize()
    for g in (src, off, siz, dst, valid):
        g.check()
    assert bool((dst.t == dst.sent).all()) and bool((valid.t == valid.sent).all())
    assert lib.mu_cv2_ragged_supported(1, 16384, 16384, 16384, 16384) == 0 and lib.mu_cv2_ragged_supported(2 ** 12, 1, 1, 16384, 16384) == -2


# ---- id maps ----------------------------------------------------------------------------------------------------------------------
MAP_SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (16, 16), (97, 213), (3, 1000), (8, 8), (6, 5)]
KIND_DTYPE = {0: np.uint8, 1: np.uint16, 2: np.int32, 3: np.uint8, 4: np.uint8}
KIND_NAMES = {0: "u8", 1: "u16", 2: "i32", 3: "rgb8", 4: "bgr8"}


@functools.lru_cache(maxsize=None)
def id_map(j, kind):
    """map j of a kind.  u8: labels around the 19 classes and 255; u16: Cityscapes-style class * 1000 + instance up to 65535; i32: both
    signs and values far above 65535; rgb8 / bgr8: three bytes per pixel, ids up to 2^24 - 1"""
    h, w = MAP_SIZES[j]
    n = R.noise(h, w, 3, salt=10 * kind + j)
    if kind == 0:
        v = n[:, :, 0] % 40
        return np.where(v > 34, 255, v).astype(np.uint8)
    if kind == 1:
        return (n[:, :, 0] % 65536).astype(np.uint16)
    if kind == 2:
        return ((n[:, :, 0] % 9000001).astype(np.int64) - 3000000).astype(np.int32)
    return (n >> 7).astype(np.uint8)


def map_values(j, kind):
    m = id_map(j, kind)
    if kind < 3:
        return m.astype(np.int64)
    return R.rgb2id(m if kind == 3 else m[:, :, ::-1])


def run_nearest(kind, out, divisor=1, n_classes=0, fill=255, refuse=True, misalign=None):
    """one call on guarded buffers -> (dst [B, Hd, Wd], valid, want [B, Hd, Wd], want_valid).  refuse: the three refused maps first, in the
    middle and last.  misalign = j: one pad byte in front of map j (its start is odd; padding behind it re-aligns the others)"""
    bpp = 3 if kind >= 3 else np.dtype(KIND_DTYPE[kind]).itemsize
    Wd, Hd = out
    parts, told, want, ok, offsets, pos = [], [], [], [], [], 0
    def add(arr, size, good, pad=0):
        nonlocal pos
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        back = (max(bpp, 2) - 1) if pad else 0                # front + back = one element: the maps behind stay aligned
        parts.append(np.concatenate([np.zeros(pad, np.uint8), raw, np.zeros(back, np.uint8)]))
        offsets.append(pos + pad)
        pos += raw.size + pad + back
        told.append(size)
        ok.append(good)
    def add_refused(k):
        th, tw = REFUSED[k][0]
        h, w = REFUSED[k][1]
        add(np.zeros((h, w, bpp), np.uint8), (th, tw), 0)
        want.append(np.full((Hd, Wd), fill, np.int64))
    for j in range(len(MAP_SIZES)):
        if refuse and j in (0, 4):
            add_refused(0 if j == 0 else 1)
        bad = misalign == j
        add(id_map(j, kind), MAP_SIZES[j], 0 if bad else 1, pad=1 if bad else 0)
        want.append(np.full((Hd, Wd), fill, np.int64) if bad else
                    R.labels(map_values(j, kind), out, divisor, n_classes if n_classes else None, fill))
    if refuse:
        add_refused(2)
    B = len(parts)
    offsets.append(pos)
    src = Guarded(pos, torch.uint8, np.concatenate(parts), "src")
    off = Guarded(B + 1, torch.int64, np.asarray(offsets, np.int64), "offsets")
    siz = Guarded(2 * B, torch.int32, np.asarray(told, np.int32), "sizes")
    dst, valid = Guarded(B * Hd * Wd, torch.int64, name="dst"), Guarded(B, torch.uint8, name="valid")
    call("mu_cv2_nearest_ragged", src, off, siz, kind, B, MAX_H, MAX_W, divisor, n_classes, fill, dst, valid, Hd, Wd)
    dst.all_written()
    valid.all_written()
    return dst.host((B, Hd, Wd)), valid.host(), np.stack(want), np.asarray(ok, np.uint8)


def check_nearest(got, valid, want, ok):
    assert valid.tolist() == ok.tolist()
    for b in range(len(ok)):
        assert np.array_equal(got[b], want[b]), f"map {b} (valid {ok[b]}): {int((got[b] != want[b]).sum())} elements differ"


@pytest.mark.parametrize("out", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4], ids=lambda k: KIND_NAMES[k])
def test_nearest_every_kind(kind, out):
    got, valid, want, ok = run_nearest(kind, out)
    assert ok.sum() == len(MAP_SIZES) and len(ok) == len(MAP_SIZES) + 3 and ok[0] == 0 and ok[-1] == 0
    check_nearest(got, valid, want, ok)
    if kind >= 2:
        assert want.max() > 65535                          # values beyond 16 bits arrive whole
    if kind == 2:
        assert want.min() < 0


def test_nearest_floor_division_of_negative_values():
    got, valid, want, ok = run_nearest(2, (128, 128), divisor=1000)
    check_nearest(got, valid, want, ok)
    b = 5 + 2                                              # map 5 = 97 x 213, two refused maps in front of it
    resized = R.labels(map_values(5, 2), (128, 128))
    toward_zero = np.fix(resized / 1000.0).astype(np.int64)
    assert (resized < 0).any() and (toward_zero != want[b]).any() and np.array_equal(np.floor(resized / 1000.0).astype(np.int64), want[b])
    got, valid, want, ok = run_nearest(2, (5, 3), divisor=1000, n_classes=19, fill=-100)
    check_nearest(got, valid, want, ok)


def test_nearest_class_cleanups():
    got, valid, want, ok = run_nearest(0, (128, 128), n_classes=19, fill=255)           # np.where((m >= 0) & (m < 19), m, 255)
    check_nearest(got, valid, want, ok)
    assert set(np.unique(want)) == set(range(19)) | {255}
    got, valid, want, ok = run_nearest(1, (128, 128), divisor=1000, n_classes=19, fill=255)          # instanceIds // 1000, then >= 19 -> 255
    check_nearest(got, valid, want, ok)
    j = MAP_SIZES.index((97, 213))
    b = j + 2                                              # two refused maps sit in front of it
    assert np.array_equal(got[b], R.city_instance_semantic(id_map(j, 1), (128, 128)))
    got, valid, want, ok = run_nearest(1, (8, 8), divisor=1000)                          # the division alone
    check_nearest(got, valid, want, ok)


def test_nearest_misaligned_u16_start_is_refused():
    j = MAP_SIZES.index((5, 7))
    got, valid, want, ok = run_nearest(1, (8, 8), fill=-5, misalign=j)
    assert ok.tolist().count(0) == 4 and ok.sum() == len(MAP_SIZES) - 1
    check_nearest(got, valid, want, ok)
    got, valid, want, ok = run_nearest(2, (5, 3), refuse=False, misalign=j)
    assert ok.tolist().count(0) == 1
    check_nearest(got, valid, want, ok)
    got, valid, want, ok = run_nearest(3, (5, 3), refuse=False, misalign=j)             # bytes need no alignment: a pad byte changes nothing
    assert valid.all() and np.array_equal(got[j], R.labels(map_values(j, 3), (5, 3)))


def test_nearest_arguments_are_refused_before_any_launch():
    from maskunet_amd import _lib
    lib = _lib.load()
    src, off, siz = ragged([id_map(3, 1)], [MAP_SIZES[3]])
    dst, valid = Guarded(64, torch.int64, name="dst"), Guarded(1, torch.uint8, name="valid")
    good = [src.p, off.p, siz.p, 1, 1, 5, 7, 1, 0, 255, dst.p, valid.p, 8, 8, _lib.stream()]
    def rc(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.mu_cv2_nearest_ragged(*a)
    assert rc(a0=None) == -1 and rc(a1=None) == -1 and rc(a2=None) == -1 and rc(a10=None) == -1 and rc(a11=None) == -1
    assert rc(a3=5) == -1 and rc(a3=-1) == -1 and rc(a4=0) == -1 and rc(a7=0) == -1 and rc(a8=-1) == -1
    assert rc(a0=src.p + 1) == -1 and rc(a0=src.p + 2, a3=2) == -1                      # a misaligned base
    assert rc(a5=0) == -2 and rc(a6=16385) == -2 and rc(a12=0) == -2 and rc(a13=16385) == -2
    torch.cuda.synchronize()
    assert bool((dst.t == dst.sent).all()) and bool((valid.t == valid.sent).all())


# ---- panoptic targets -------------------------------------------------------------------------------------------------------------
def seg_max():
    from maskunet_amd import _lib
    return _lib.MU_PANOPTIC_SEG_MAX


SPAN = [0, 5, 255, 256, 300, 65535, 65536, 70000, 1234567, 16777215]       # ids over all three bytes, id 0 among them


@functools.lru_cache(maxsize=None)
def pan_case(name):
    """(png uint8 [h, w, 3] RGB, told (h, w), segments as (ids, labels) in TABLE order, expect refused)"""
    cap = seg_max()
    pick = lambda h, w, ids, salt: R.id2rgb(np.asarray(ids, np.int64)[R.noise(h, w, 1, salt)[:, :, 0] % len(ids)])
    if name == "span":                                     # 255 and 70000 are not listed: 0 / 0; id 0 is in the PNG and not listed
        return pick(37, 53, SPAN, 1), (37, 53), ([5, 256, 300, 65535, 65536, 1234567, 16777215], [1, 2, 3, 4, 5, 6, 7]), False
    if name == "zero_listed":                              # id 0 is a listed segment
        return pick(16, 16, SPAN, 2), (16, 16), ([0, 5, 70000], [9, 1, 133]), False
    if name == "no_segments":
        return pick(5, 7, SPAN, 3), (5, 7), ([], []), False
    if name in ("cap", "cap_plus_1"):                      # ids 3, 6, .. 3 n; the PNG also holds ids in between
        n = cap if name == "cap" else cap + 1
        png = R.id2rgb(R.noise(97, 213, 1, 4)[:, :, 0] % (3 * cap + 9))
        return png, (97, 213), ([3 * (k + 1) for k in range(n)], [k % 200 + 1 for k in range(n)]), name != "cap"
    if name == "equal_ids":                                # not STRICTLY ascending
        return pick(9, 1, SPAN, 5), (9, 1), ([5, 300, 300, 70000], [1, 2, 3, 4]), True
    if name == "descending":
        return pick(1, 9, SPAN, 6), (1, 9), ([5, 70000, 300], [1, 2, 3]), True
    if name == "no_rows":
        return np.zeros((0, 0, 3), np.uint8), (0, 5), ([5], [1]), True
    if name == "short":
        return pick(10, 9, SPAN, 7), (10, 10), ([5], [1]), True
    if name == "one":                                      # a table of one row, a 1 x 1 image
        return R.id2rgb(np.full((1, 1), 300)), (1, 1), ([300], [77]), False
    raise KeyError(name)


BATCH = ("no_rows", "span", "zero_listed", "no_segments", "cap_plus_1", "cap", "equal_ids", "one", "descending", "span", "short")


def pan_expected(name, out, swap_rb, fill):
    png, told, (ids, labels), refused = pan_case(name)
    if refused:
        return np.full((out[1], out[0]), fill, np.int64), np.zeros((out[1], out[0]), np.int64), 0
    segs = [{"id": i, "category_id": l} for i, l in zip(ids, labels)]
    sem, inst = R.coco_panoptic_targets(png, segs, out)
    return sem, inst, 1


def run_panoptic(names, out, swap_rb=0, fill=255, seg_offsets=None, empty_tables=False):
    """swap_rb: the device gets the PNGs as cv2.imread leaves them (BGR) and must give what the RGB bytes give"""
    Wd, Hd = out
    cases = [pan_case(n) for n in names]
    B = len(cases)
    src, off, siz = ragged([c[0][:, :, ::-1] if swap_rb else c[0] for c in cases], [c[1] for c in cases])
    ids = [] if empty_tables else [i for c in cases for i in c[2][0]]
    labels = [] if empty_tables else [l for c in cases for l in c[2][1]]
    so = seg_offsets if seg_offsets is not None else np.concatenate([[0], np.cumsum([0 if empty_tables else len(c[2][0]) for c in cases])])
    S = len(ids)
    g_ids, g_lab = Guarded(S, torch.int32, np.asarray(ids, np.int32), "seg_ids"), Guarded(S, torch.int32, np.asarray(labels, np.int32), "seg_labels")
    g_so = Guarded(B + 1, torch.int32, np.asarray(so, np.int32), "img_seg_offsets")
    sem, inst, valid = (Guarded(B * Hd * Wd, torch.int64, name="semantic"), Guarded(B * Hd * Wd, torch.int64, name="instance"),
                        Guarded(B, torch.uint8, name="valid"))
    call("mu_panoptic_targets", src, off, siz, g_ids, g_lab, g_so, B, S, MAX_H, MAX_W, swap_rb, fill, sem, inst, valid, Hd, Wd)
    for g in (sem, inst, valid):
        g.all_written()
    return sem.host((B, Hd, Wd)), inst.host((B, Hd, Wd)), valid.host()


@pytest.mark.parametrize("swap_rb", [0, 1], ids=["rgb", "bgr"])
@pytest.mark.parametrize("out", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_panoptic_batch(out, swap_rb):
    sem, inst, valid = run_panoptic(BATCH, out, swap_rb=swap_rb)
    assert valid.tolist() == [0 if pan_case(n)[3] else 1 for n in BATCH] and valid[0] == 0 and valid[-1] == 0
    for b, n in enumerate(BATCH):
        w_sem, w_inst, ok = pan_expected(n, out, swap_rb, 255)
        assert np.array_equal(sem[b], w_sem), f"{n}: semantic"
        assert np.array_equal(inst[b], w_inst), f"{n}: instance"
    if out == (128, 128) and not swap_rb:
        b = BATCH.index("span")
        assert set(np.unique(inst[b])) == {0, 5, 256, 300, 65535, 65536, 1234567, 16777215}             # 255, 70000 and 0 itself: unlisted
        assert set(np.unique(sem[BATCH.index("zero_listed")])) == {0, 1, 9, 133}
        assert not sem[BATCH.index("no_segments")].any() and not inst[BATCH.index("no_segments")].any()
        cap = BATCH.index("cap")
        assert inst[cap].max() > 3 * (seg_max() - 50) and (inst[cap] % 3 == 0).all() and (inst[cap] == 0).any()


def test_panoptic_other_fill_and_no_tables_at_all():
    sem, inst, valid = run_panoptic(("short", "one", "span"), (5, 3), fill=-1)
    assert valid.tolist() == [0, 1, 1] and (sem[0] == -1).all() and not inst[0].any() and (sem[1] == 77).all() and (inst[1] == 300).all()
    # S = 0 for the whole call: null tables, every valid image is 0 / 0
    names = ("span", "no_rows", "one")
    sem, inst, valid = run_panoptic(names, (8, 8), empty_tables=True)
    assert valid.tolist() == [1, 0, 1]
    assert not sem[0].any() and not inst[0].any() and (sem[1] == 255).all() and not inst[1].any() and not sem[2].any() and not inst[2].any()


def test_panoptic_table_offsets_out_of_order_or_out_of_range():
    names = ("one", "zero_listed", "one", "one")           # rows: [300] [0 5 70000] [300] [300], S = 6
    w_sem, w_inst, _ = pan_expected("zero_listed", (8, 8), 0, 255)
    # image 1 starts behind its end; image 3 ends beyond S; image 0 is untouched, image 2 reads rows [2, 5) = 5 70000 300: descending
    sem, inst, valid = run_panoptic(names, (8, 8), seg_offsets=[0, 4, 2, 5, 7])
    assert valid.tolist() == [0, 0, 0, 0]                  # image 0 holds rows [0, 4) = 300 0 5 70000: not ascending either
    sem, inst, valid = run_panoptic(names, (8, 8), seg_offsets=[0, 1, 4, 5, 7])
    assert valid.tolist() == [1, 1, 1, 0] and np.array_equal(sem[1], w_sem) and np.array_equal(inst[1], w_inst)
    assert (sem[3] == 255).all() and not inst[3].any() and (inst[0] == 300).all()
    sem, inst, valid = run_panoptic(names, (8, 8), seg_offsets=[-1, 1, 4, 5, 6])
    assert valid.tolist() == [0, 1, 1, 1]


def test_panoptic_arguments_are_refused_before_any_launch():
    from maskunet_amd import _lib
    lib = _lib.load()
    src, off, siz = ragged([pan_case("one")[0]], [(1, 1)])
    t = Guarded(3, torch.int32, [300, 77, 0], "tables")
    so = Guarded(2, torch.int32, [0, 1], "img_seg_offsets")
    sem, inst, valid = Guarded(64, torch.int64, name="semantic"), Guarded(64, torch.int64, name="instance"), Guarded(1, torch.uint8, name="valid")
    good = [src.p, off.p, siz.p, t.p, t.p + 4, so.p, 1, 1, 1, 1, 0, 255, sem.p, inst.p, valid.p, 8, 8, _lib.stream()]
    def rc(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.mu_panoptic_targets(*a)
    for k in (0, 1, 2, 3, 4, 5, 12, 13, 14):
        assert rc(**{f"a{k}": None}) == -1, k
    assert rc(a6=0) == -1 and rc(a7=-1) == -1
    assert rc(a8=0) == -2 and rc(a9=16385) == -2 and rc(a15=0) == -2 and rc(a16=16385) == -2
    torch.cuda.synchronize()
    assert bool((sem.t == sem.sent).all()) and bool((inst.t == inst.sent).all()) and bool((valid.t == valid.sent).all())
    assert rc() == 0 and rc(a3=None, a4=None, a7=0) == 0   # the good call; S = 0 with null tables
    torch.cuda.synchronize()


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
PY_IMAGES = [SIZES.index(s) for s in [(97, 213), (5, 7), (256, 256), (128, 128), (3, 1000)]]


def test_resize_cv2_to_nhwc_list_uniform_and_packed():
    from maskunet_amd import PackedImages, ops, pack_images, resize_cv2_to_nhwc
    imgs = [torch.from_numpy(image(i, 3)).to(DEV) for i in PY_IMAGES]
    y, u8, valid = resize_cv2_to_nhwc(imgs, (128, 128), torch.float16, return_u8=True)
    assert y.shape == (5, 128, 128, 32) and y.dtype == torch.float16 and u8.shape == (5, 128, 128, 3) and valid.tolist() == [1] * 5
    for b, i in enumerate(PY_IMAGES):
        want = expected(i, 3, (128, 128))[0]
        assert np.array_equal(u8[b].cpu().numpy(), want)
        assert np.array_equal(y[b, :, :, :3].cpu().numpy().view(np.uint16), R.to_unit(want, np.float16).view(np.uint16)) and not y[b, :, :, 3:].any()
        one = ops.resize_u8_to_nhwc(imgs[b][None], (128, 128), torch.float16)
        assert torch.equal(y[b].view(torch.int16), one[0].view(torch.int16))
    # host images and a device: one copy; grey images; size = (width, height); (y, valid) without the bytes
    y1, v1 = resize_cv2_to_nhwc([image(i, 1) for i in PY_IMAGES], (5, 3), torch.float32, device=DEV)
    assert y1.shape == (5, 3, 5, 32) and v1.tolist() == [1] * 5
    for b, i in enumerate(PY_IMAGES):
        assert np.array_equal(y1[b, :, :, :1].cpu().numpy().view(np.uint32), R.to_unit(expected(i, 1, (5, 3))[0]).view(np.uint32))
    # a uniform [B, H, W, C] tensor, bgr: what the uniform wrapper gives
    t = torch.from_numpy(np.stack([image(PY_IMAGES[0], 3), image(PY_IMAGES[0], 3)[::-1, ::-1].copy()])).to(DEV)
    y2, u2, v2 = resize_cv2_to_nhwc(t, (128, 128), torch.float32, bgr=True, return_u8=True)
    yu, uu = ops.resize_u8_to_nhwc(t, (128, 128), torch.float32, bgr=True, return_u8=True)
    assert v2.tolist() == [1, 1] and torch.equal(u2, uu) and torch.equal(y2.view(torch.int32), yu.view(torch.int32))
    assert np.array_equal(u2[0].cpu().numpy(), expected(PY_IMAGES[0], 3, (128, 128))[0][:, :, ::-1])
    # a packed batch is taken as it is; an image whose slot is too short reports valid = 0 and does not raise
    p = pack_images(imgs[:2])
    short = PackedImages(p.data, p.offsets, torch.tensor([[98, 213], [5, 7]], dtype=torch.int32, device=DEV), 3, 98, 213)
    y3, v3 = resize_cv2_to_nhwc(short, (8, 8), torch.float16)
    assert v3.tolist() == [0, 1] and not y3[0].any()
    assert np.array_equal(y3[1, :, :, :3].cpu().numpy().view(np.uint16), R.to_unit(expected(PY_IMAGES[1], 3, (8, 8))[0], np.float16).view(np.uint16))
    with pytest.raises(ValueError, match="size"):
        resize_cv2_to_nhwc(imgs, (0, 8), torch.float16)
    with pytest.raises(ValueError, match="size"):
        resize_cv2_to_nhwc(imgs, (8, 16385), torch.float16)


def test_resize_labels_cv2_list_uniform_and_packed():
    from maskunet_amd import ops, pack_maps, resize_labels_cv2
    for kind in (0, 1, 2, 3):
        maps = [id_map(j, kind) for j in range(len(MAP_SIZES))]
        got, valid = resize_labels_cv2([torch.from_numpy(m).to(DEV) for m in maps], (128, 128))
        assert got.dtype == torch.int64 and got.shape == (len(maps), 128, 128) and bool(valid.all())
        for j in range(len(maps)):
            assert np.array_equal(got[j].cpu().numpy(), R.labels(map_values(j, kind), (128, 128))), (kind, j)
        host, v = resize_labels_cv2(maps, (5, 3), device=DEV)                            # host arrays: one copy
        assert torch.equal(host, resize_labels_cv2(pack_maps(maps, DEV), (5, 3))[0]) and bool(v.all())
        assert np.array_equal(host[5].cpu().numpy(), R.labels(map_values(5, kind), (5, 3)))
    # the Cityscapes lines
    ids16 = [id_map(j, 1) for j in (5, 3)]
    sem, _ = resize_labels_cv2(ids16, (128, 128), divisor=1000, num_classes=19, device=DEV)
    assert np.array_equal(sem[0].cpu().numpy(), R.city_instance_semantic(ids16[0], (128, 128)))
    lab, _ = resize_labels_cv2([id_map(5, 0)], (128, 128), num_classes=19, fill=255, device=DEV)
    assert np.array_equal(lab[0].cpu().numpy(), R.labels(id_map(5, 0), (128, 128), num_classes=19))
    neg, _ = resize_labels_cv2([id_map(5, 2)], (8, 8), divisor=1000, device=DEV)
    assert np.array_equal(neg[0].cpu().numpy(), R.labels(id_map(5, 2), (8, 8), divisor=1000)) and int(neg.min()) < 0
    # a uniform uint8 tensor: the uniform wrapper's result
    t = torch.from_numpy(np.stack([id_map(5, 0), id_map(5, 0)[::-1].copy()])).to(DEV)
    got, valid = resize_labels_cv2(t, (128, 128))
    assert torch.equal(got, ops.resize_labels_u8(t, (128, 128))) and valid.tolist() == [1, 1]
    t16 = torch.from_numpy(np.stack([id_map(5, 1)] * 2)).to(DEV)                         # uint16 on the device
    assert np.array_equal(resize_labels_cv2(t16, (5, 3))[0][1].cpu().numpy(), R.labels(id_map(5, 1), (5, 3)))
    with pytest.raises(ValueError, match="divisor"):
        resize_labels_cv2(t, (8, 8), divisor=0)
    with pytest.raises(ValueError, match="divisor"):
        resize_labels_cv2(t, (8, 8), num_classes=0)


PY_PAN = ("span", "zero_listed", "no_segments", "cap", "one")


def pan_segments_info(name, shuffle=False):
    ids, labels = pan_case(name)[2]
    segs = [{"id": int(i), "category_id": int(l)} for i, l in zip(ids, labels)]
    if shuffle and len(segs) > 2:                          # the JSON's order is not sorted, and holds a duplicate the later entry of which stays
        segs = [dict(segs[1], category_id=250)] + segs[::-1]
    return segs


def test_panoptic_targets_and_instances_from_id_map():
    from maskunet_amd import PanopticTargets, instances_from_id_map, pack_images, panoptic_targets
    pngs = [pan_case(n)[0] for n in PY_PAN]
    infos = [pan_segments_info(n, shuffle=True) for n in PY_PAN]
    t = panoptic_targets([torch.from_numpy(p).to(DEV) for p in pngs], infos, (128, 128))
    assert isinstance(t, PanopticTargets) and t.semantic.dtype == torch.int64 and t.semantic.shape == (5, 128, 128) and t.valid.tolist() == [1] * 5
    want = [R.coco_panoptic_targets(p, s, (128, 128)) for p, s in zip(pngs, infos)]
    w_sem, w_inst = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    assert np.array_equal(t.semantic.cpu().numpy(), w_sem) and np.array_equal(t.instance.cpu().numpy(), w_inst)
    # host PNGs as cv2.imread leaves them, a cat2label, another fill; a packed batch
    cat2label = {c: (c * 7) % 150 for c in range(256)}
    tb = panoptic_targets([np.ascontiguousarray(p[:, :, ::-1]) for p in pngs], infos, (5, 3), cat2label=cat2label, bgr=True, fill=-1, device=DEV)
    for b, (p, s) in enumerate(zip(pngs, infos)):
        sem, inst = R.coco_panoptic_targets(p, s, (5, 3), cat2label)
        assert np.array_equal(tb.semantic[b].cpu().numpy(), sem) and np.array_equal(tb.instance[b].cpu().numpy(), inst)
    tp = panoptic_targets(pack_images(pngs, DEV), infos, (128, 128))
    assert torch.equal(tp.semantic, t.semantic) and torch.equal(tp.instance, t.instance)
    with pytest.raises(KeyError):
        panoptic_targets(pngs, infos, (8, 8), cat2label={1: 1}, device=DEV)
    with pytest.raises(ValueError, match="entries"):
        panoptic_targets(pngs, infos[:-1], (8, 8), device=DEV)
    # the consumer: ground-truth instances of the device-built targets == those of the reference-built targets uploaded from numpy
    a = instances_from_id_map(t.instance, t.semantic, max_instances=1024)
    b = instances_from_id_map(torch.from_numpy(w_inst).to(DEV), torch.from_numpy(w_sem).to(DEV), max_instances=1024)
    sa, sb = side_of(a), side_of(b)
    assert sa.keys() == sb.keys() and int(sa["count"].max()) > 100
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k


@functools.lru_cache(maxsize=None)
def model():
    import maskunet_amd
    torch.manual_seed(3)
    m = maskunet_amd.UNet(3, 5).to(DEV).eval()
    m.set_keep_masks([(torch.arange(2 * k).reshape(2, k) * 7 % 3 != 0).to(torch.uint8).to(DEV) for k in (4096, 1024, 256, 1024, 4096, 16384)])
    return m


def test_forward_u8_cv2_of_a_list_equals_forward_of_the_reference_resize():
    from maskunet_amd import PackedImages, ops, pack_images
    m = model()
    idx = [SIZES.index(s) for s in [(97, 213), (256, 256)]]
    imgs = [torch.from_numpy(image(i, 3)).to(DEV) for i in idx]
    host = np.stack([R.to_unit(expected(i, 3, (128, 128))[0]).transpose(2, 0, 1) for i in idx])          # ToTensor: CHW float32
    with torch.no_grad():
        b = m(torch.from_numpy(host).to(DEV))
        a = m.forward_u8(imgs, resample="cv2", check=True)
        assert torch.equal(a, b)
        assert torch.equal(m.forward_u8(tuple(imgs)), b) and torch.equal(m.forward_u8(pack_images(imgs)), b)
        assert torch.equal(m.forward_u8([im.flip(-1) for im in imgs], bgr=True), b)
        # a uniform tensor takes the path it took before
        t = torch.stack([imgs[0], imgs[0].flip(0)])
        today = m._finish(m.forward_nhwc(ops.resize_u8_to_nhwc(t, (128, 128), m.compute_dtype, bgr=True)))
        assert torch.equal(m.forward_u8(t, bgr=True), today) and torch.equal(m.forward_u8([t[0], t[1]], bgr=True), today)
        p = pack_images(imgs)
        short = PackedImages(p.data, p.offsets, torch.tensor([[97, 213], [257, 256]], dtype=torch.int32, device=DEV), 3, 257, 256)
        m.forward_u8(short)                                # a refused image enters as zeros and raises only on request
        with pytest.raises(RuntimeError, match=r"refused images \[1\]"):
            m.forward_u8(short, check=True)


# ---- repeatability ----------------------------------------------------------------------------------------------------------------
def test_repeatable_and_graph_capturable():
    from maskunet_amd import pack_images, pack_maps, panoptic_targets, resize_cv2_to_nhwc, resize_labels_cv2
    p = pack_images([torch.from_numpy(image(i, 3)).to(DEV) for i in PY_IMAGES])
    maps = pack_maps([id_map(j, 1) for j in range(len(MAP_SIZES))], DEV)
    pngs = pack_images([pan_case(n)[0] for n in PY_PAN], DEV)
    infos = [pan_segments_info(n) for n in PY_PAN]

    def all_three():
        y, u8, v0 = resize_cv2_to_nhwc(p, (128, 128), torch.float16, return_u8=True)
        lab, v1 = resize_labels_cv2(maps, (128, 128), divisor=1000, num_classes=19)
        t = panoptic_targets(pngs, infos, (128, 128))
        return [y.view(torch.int16), u8, v0, lab, v1, t.semantic, t.instance, t.valid]

    first, second = all_three(), all_three()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert np.array_equal(first[1][0].cpu().numpy(), expected(PY_IMAGES[0], 3, (128, 128))[0])
    assert np.array_equal(first[3][5].cpu().numpy(), R.city_instance_semantic(id_map(5, 1), (128, 128)))
    torch.cuda.synchronize()
    # panoptic_targets copies the segment tables from the host, which is no graph work: the three KERNELS are captured, the third on
    # tables uploaded beforehand
    from maskunet_amd import _lib
    from maskunet_amd.targets import pack_segments
    ids, labels, so = pack_segments(infos)
    tables = torch.from_numpy(np.concatenate([so, ids, labels])).to(DEV)
    B, S = len(PY_PAN), ids.size
    sem = torch.empty((B, 128, 128), dtype=torch.int64, device=DEV)
    inst, pv = torch.empty_like(sem), torch.empty(B, dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y, u8, v0 = resize_cv2_to_nhwc(p, (128, 128), torch.float16, return_u8=True)
        lab, v1 = resize_labels_cv2(maps, (128, 128), divisor=1000, num_classes=19)
        _lib.call("mu_panoptic_targets", pngs.data.data_ptr(), pngs.offsets.data_ptr(), pngs.sizes.data_ptr(), tables[B + 1:].data_ptr(),
                  tables[B + 1 + S:].data_ptr(), tables.data_ptr(), B, S, pngs.max_h, pngs.max_w, 0, 255, sem.data_ptr(), inst.data_ptr(),
                  pv.data_ptr(), 128, 128, _lib.stream())
    outs = [y.view(torch.int16), u8, v0, lab, v1, sem, inst, pv]
    for t in outs:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))
