"""Pillow's antialiased bilinear resize of 8-bit images, restated in numpy: `Image.resize((Wd, Hd), Image.BILINEAR)` as torchvision's
`T.Resize((Hd, Wd))` runs it on a PIL image (the reference's coco_instance.py:43-47).  No torch, nothing of maskunet_amd.

The rule (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal/Vertical_8bpc), checked byte for
byte against Pillow 12.2.0 (tests/golden/pil/, tests/test_pil_resize_host.py):

  one axis n_in -> n_out, all in fp64 and every operation rounded on its own:
      scale = n_in / n_out;  fs = max(scale, 1.0);  support = fs;  ss = 1.0 / fs;  ksize = 2 * ceil(support) + 1
      output index xx:  center = (xx + 0.5) * scale
                        xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), n_in);  n = xmax - xmin
                        w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|)   for x < n
                        ww = w[0] + w[1] + ..  (ascending);  w[x] /= ww  if ww != 0
                        k[x] = (int)(0.5 + w[x] * 2^22)
  one pass:   out = clamp((2^21 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255)        (int32 suffices)
  two passes: horizontal, then vertical, each only if that axis changes size; the intermediate is rounded to uint8.
  channels are independent (L and RGB; RGBA is premultiplied by Pillow and NOT covered).
  an image with h > 100 * w that shrinks vertically is outside the contract (Pillow 12 resizes those vertically first): `refused`.

Inputs come from `pattern`, a pure integer formula, so that the committed fixtures hold Pillow's OUTPUT bytes only.
"""
import math

import numpy as np

PRECISION_BITS = 22
KINDS = ("noise", "binary", "ramp")

# the ragged batch of the GPU tests and of the fixtures: (h, w) source sizes inside the contract ...
SIZES = [(1, 1), (1, 7), (7, 1), (5, 7),                    # degenerate
         (127, 129), (128, 128),                            # either side of the identity
         (128, 300), (300, 128),                            # one pass only (at 128x128)
         (97, 213),                                         # odd upscale on one axis, downscale on the other
         (480, 640), (427, 640), (640, 480),                # COCO shapes
         (3, 1000),                                         # 334 taps per output column at Hd = 3 .. 669 per row
         (1000, 10), (400, 4),                              # the 100:1 limit
         (51, 333),                                         # mixed
         (2048, 64)]                                        # 33 taps, long vertical bands
# ... and the output sizes (Hd, Wd)
OUT_SIZES = [(128, 128), (3, 5), (96, 80), (256, 256)]


def kind_of(i, rot=0):
    """content of image i of the batch: the kinds rotate over the images"""
    return KINDS[(i + rot) % 3]


def pattern(h, w, c, kind):
    """uint8 [h, w, c] (c = 1: [h, w]) from integer arithmetic alone: 'noise' (a 32-bit multiplicative hash of the position),
    'binary' (0 / 255 from one bit of it: exercises the clamp and the rounding) or 'ramp'."""
    y, x, ch = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(c, dtype=np.uint64), indexing="ij")
    if kind == "ramp":
        v = (x * np.uint64(3) + y * np.uint64(5) + ch * np.uint64(40)) & np.uint64(255)
    else:
        m = np.uint64(0xFFFFFFFF)
        v = (y * np.uint64(73856093) + x * np.uint64(19349663) + ch * np.uint64(83492791) + np.uint64(h * 131 + w * 31 + 7)) & m
        v = ((v ^ (v >> np.uint64(15))) * np.uint64(0x2C1B3C6D)) & m
        v = ((v ^ (v >> np.uint64(12))) * np.uint64(0x297A2D39)) & m
        v = v ^ (v >> np.uint64(15))
        if kind == "noise":
            v = (v >> np.uint64(8)) & np.uint64(255)
        elif kind == "binary":
            v = ((v >> np.uint64(13)) & np.uint64(1)) * np.uint64(255)
        else:
            raise ValueError(f"unknown kind {kind!r}")
    v = v.astype(np.uint8)
    return v[:, :, 0] if c == 1 else v


def coefficients(n_in, n_out):
    """(xmin int32 [n_out], n int32 [n_out], k int32 [n_out, ksize]) of one axis; k is zero beyond n."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    ksize = 2 * int(math.ceil(support)) + 1
    xmin = np.zeros(n_out, np.int32)
    cnt = np.zeros(n_out, np.int32)
    k = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        n = hi - lo
        w = [max(0.0, 1.0 - abs((x + lo - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], cnt[xx] = lo, n
        for x in range(n):
            k[xx, x] = int(0.5 + w[x] * (1 << PRECISION_BITS))
    return xmin, cnt, k


def _pass(src, n_out, axis, rounded=True):
    """one pass along `axis` of an integer (or, with rounded=False upstream, float) [h, w, c] array"""
    n_in = src.shape[axis]
    xmin, cnt, k = coefficients(n_in, n_out)
    a = np.moveaxis(src, axis, 0)
    acc = np.zeros((n_out,) + a.shape[1:], np.float64 if a.dtype.kind == "f" else np.int64)
    tail = (1,) * (a.ndim - 1)
    for t in range(k.shape[1]):
        idx = np.minimum(xmin + t, n_in - 1)                 # k is 0 where t >= n
        acc += a[idx] * k[:, t].reshape((-1,) + tail).astype(acc.dtype)
    if not rounded:
        return np.moveaxis(acc / float(1 << PRECISION_BITS), 0, axis)
    if acc.dtype.kind == "f":
        out = np.clip(np.floor(acc / float(1 << PRECISION_BITS) + 0.5), 0, 255).astype(np.int64)
    else:
        out = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def refused(h, w, Hd, Wd):
    """outside the contract: no size, or a tall image that Pillow 12 resizes vertically first"""
    return h < 1 or w < 1 or (h > 100 * w and Hd < h)


def resize(img, size, order="hv", float_intermediate=False):
    """uint8 [h, w] or [h, w, c] -> uint8 [Hd, Wd(, c)], size = (Hd, Wd).  order / float_intermediate exist for the tests that show that
    both matter: 'vh' runs the vertical pass first, float_intermediate keeps the first pass unrounded."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    Hd, Wd = int(size[0]), int(size[1])
    h, w = img.shape[:2]
    if refused(h, w, Hd, Wd):
        raise ValueError(f"a {h}x{w} image to {Hd}x{Wd} is outside the contract")
    a = img.astype(np.int64).reshape(h, w, -1)
    passes = [(1, Wd, w), (0, Hd, h)]
    if order == "vh":
        passes.reverse()
    passes = [p for p in passes if p[1] != p[2]]
    for i, (axis, n_out, _) in enumerate(passes):
        last = i == len(passes) - 1
        a = _pass(a, n_out, axis, rounded=last or not float_intermediate)
    return a.astype(np.uint8).reshape((Hd, Wd) + img.shape[2:])


def to_unit(u8, dtype=np.float32):
    """ToTensor: float32(byte) / float32(255) by IEEE division, then round-to-nearest-even to fp16 for fp16 storage"""
    return (u8.astype(np.float32) / np.float32(255.0)).astype(dtype)


def fixture_key(h, w, c, kind, Hd, Wd):
    return f"{h}x{w}x{c}_{kind}_to_{Hd}x{Wd}"


def fixture_cases():
    """(h, w, c, kind, Hd, Wd) of every committed fixture: the whole batch at 128x128 (kinds as the GPU tests rotate them, rot = 0) and
    at 3x5; a COCO shape, the tap-heavy, the 100:1 and the small images at 96x80; three single-channel ones at 256x256 (upscale)."""
    at_96 = {(480, 640), (3, 1000), (1000, 10), (97, 213), (5, 7)}
    at_256 = {(480, 640), (97, 213), (5, 7)}
    for c in (1, 3):
        for i, (h, w) in enumerate(SIZES):
            for Hd, Wd in OUT_SIZES:
                if ((Hd, Wd) in ((128, 128), (3, 5)) or ((Hd, Wd) == (96, 80) and (h, w) in at_96)
                        or ((Hd, Wd) == (256, 256) and c == 1 and (h, w) in at_256)):
                    yield h, w, c, kind_of(i), Hd, Wd


def load_fixtures(directory):
    """{key: uint8 array} of tests/golden/pil/*.npz plus the Pillow version string that made them"""
    import glob
    import os
    out, version = {}, None
    for path in sorted(glob.glob(os.path.join(directory, "pil_*.npz"))):
        with np.load(path) as z:
            for name in z.files:
                if name == "pillow_version":
                    version = str(z[name])
                else:
                    out[name] = z[name]
    return out, version
