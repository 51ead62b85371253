"""Image preparation of the COCO instance loader on the device: Pillow's antialiased bilinear resize of a ragged batch.

The reference prepares a COCO image with T.ToPILImage() -> T.Resize((128, 128)) -> T.ToTensor() (coco_instance.py:43-47,68), i.e. Pillow's
Image.resize(.., BILINEAR) with its antialiasing support -- not cv2.resize(.., INTER_LINEAR), which ops.resize_u8_to_nhwc restates -- and
COCO images have sizes of their own.  Here the decoded bytes of all images go to the device as ONE flat buffer with a size per image and
mu_pil_resize_u8_nhwc does the rest in two launches; include/maskunet_hip.h holds the contract, pinned to the bytes of Pillow 12.2.0
(tests/golden/pil/).  The host side only packs arrays.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import call, dt, ptr, stream

MAX_SIDE = 16384
MAX_OUT_PIXELS = 65536


@dataclass
class PackedImages:
    """A ragged batch as mu_pil_resize_u8_nhwc takes it; the three tensors live on one device (or all on the host)."""
    data: torch.Tensor           # uint8 [sum h * w * C]   the images' bytes, HWC, one after the other
    offsets: torch.Tensor        # int64 [B+1]             byte offset of every image in data
    sizes: torch.Tensor          # int32 [B,2]             (height, width)
    channels: int                # C of every image
    max_h: int                   # the bounds the host passes
    max_w: int


def _pad32(c):
    return (c + 31) // 32 * 32


def pack_images(images, device=None) -> PackedImages:
    """images: a list of uint8 [h, w, C] or [h, w] (C = 1) numpy arrays or tensors, all on the host or all on one device, or one uniform
    uint8 [B, H, W, C] tensor.  C is 1 or 3 for every image (Pillow resizes RGBA premultiplied: refused).  One torch.cat, and at most one
    host-to-device copy -- bytes, offsets and sizes travel in one buffer -- with no per-image launch.  device=None leaves the result where
    the images are."""
    dev = None if device is None else torch.device(device)
    if isinstance(images, (torch.Tensor, np.ndarray)) and images.ndim == 4:
        t = torch.as_tensor(images)
        if t.dtype != torch.uint8:
            raise ValueError(f"images must be uint8, got {t.dtype}")
        B, H, W, C = t.shape
        if B < 1:
            raise ValueError("pack_images needs at least one image")
        flat, shapes = [t.contiguous().reshape(-1)], [(H, W)] * B
    else:
        if isinstance(images, (torch.Tensor, np.ndarray)):
            raise ValueError("pack_images expects a list of [h, w, C] / [h, w] images or one [B, H, W, C] tensor")
        images = list(images)
        if not images:
            raise ValueError("pack_images needs at least one image")
        ts = [torch.as_tensor(im) for im in images]
        for t in ts:
            if t.dtype != torch.uint8 or t.dim() not in (2, 3):
                raise ValueError(f"every image must be uint8 [h, w, C] or [h, w], got {t.dtype} {tuple(t.shape)}")
        chans = {1 if t.dim() == 2 else int(t.shape[2]) for t in ts}
        if len(chans) != 1:
            raise ValueError(f"the images of one call share a channel count, got {sorted(chans)}")
        C = chans.pop()
        if len({t.device for t in ts}) != 1:
            raise ValueError("the images of one call live on one device (or all on the host)")
        flat, shapes = [t.contiguous().reshape(-1) for t in ts], [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    if C not in (1, 3):
        raise ValueError(f"C = {C}: the Pillow resize takes 1 or 3 channels (Pillow resizes RGBA premultiplied, which this rule does not restate)")
    sizes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    if bool((sizes < 1).any()) or bool((sizes > MAX_SIDE).any()):
        raise ValueError(f"image sides must lie in [1, {MAX_SIDE}], got heights {sizes[:, 0].min()}..{sizes[:, 0].max()}, widths {sizes[:, 1].min()}..{sizes[:, 1].max()}")
    offsets = np.zeros(sizes.shape[0] + 1, dtype=np.int64)
    np.cumsum(sizes[:, 0] * sizes[:, 1] * C, out=offsets[1:])
    meta = torch.from_numpy(np.concatenate([offsets.view(np.uint8), sizes.astype(np.int32).reshape(-1).view(np.uint8)]))
    nb_off, nb_meta = offsets.size * 8, meta.numel()         # sizes follow the offsets: both stay aligned, the bytes come last
    src_dev = flat[0].device
    if src_dev.type == "cpu":
        buf = torch.cat([meta] + flat)                       # the one cat; then the one copy
        if dev is not None and dev.type != "cpu":
            buf = buf.to(dev)
        meta, data = buf[:nb_meta], buf[nb_meta:]
    else:
        if dev is not None and dev != src_dev and not (dev.type == src_dev.type and dev.index is None):
            raise ValueError(f"the images live on {src_dev}, not on {dev}")
        meta = meta.to(src_dev)
        data = flat[0] if len(flat) == 1 else torch.cat(flat)
    return PackedImages(data, meta[:nb_off].view(torch.int64), meta[nb_off:].view(torch.int32).view(-1, 2), C,
                        int(sizes[:, 0].max()), int(sizes[:, 1].max()))


def resize_pil_to_nhwc(images, size=(128, 128), dtype=torch.float32, bgr=False, return_u8=False, device=None):
    """Decoded image bytes of ANY sizes -> the network input [B, Hd, Wd, pad32(C)] in `dtype` by the reference's COCO transform
    T.ToPILImage() -> T.Resize(size) -> T.ToTensor(): Pillow's antialiased bilinear resize, byte for byte, then byte / 255.  size =
    (height, width) like torchvision.  images: what pack_images takes, or a PackedImages; bgr=True swaps channels 0 and 2 (cv2.imread
    bytes).  Returns (y, valid) or (y, u8, valid): u8 [B, Hd, Wd, C] are the resized bytes, valid uint8 [B] is 0 for an image the kernel
    refused (taller than 100 widths and shrinking vertically: Pillow 12 treats those differently), whose outputs are zero.  Host images
    need `device`.  Never synchronises with the device.  No gradient."""
    packed = images if isinstance(images, PackedImages) else pack_images(images, device)
    if packed.data.device.type != "cuda":
        raise RuntimeError("maskunet_amd: tensors must live on the GPU (the HIP path has no CPU fallback); pass device= for host images")
    Hd, Wd = int(size[0]), int(size[1])
    if Hd < 1 or Wd < 1 or Hd * Wd > MAX_OUT_PIXELS:
        raise ValueError(f"size[0] * size[1] must lie in [1, {MAX_OUT_PIXELS}], got {(Hd, Wd)}")
    dev, B, C = packed.data.device, packed.sizes.shape[0], packed.channels
    Cp = _pad32(C)
    y = torch.empty((B, Hd, Wd, Cp), dtype=dtype, device=dev)
    u8 = torch.empty((B, Hd, Wd, C), dtype=torch.uint8, device=dev) if return_u8 else None
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        nbytes = lib.mu_pil_resize_workspace_bytes(B, packed.max_h, packed.max_w, Hd, Wd)
        ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
        call("mu_pil_resize_u8_nhwc", ptr(packed.data), ptr(packed.offsets), ptr(packed.sizes), B, C, packed.max_h, packed.max_w,
             int(bool(bgr)), ptr(y), ptr(u8), ptr(valid), Hd, Wd, Cp, dt(y), ptr(ws), ws.numel(), stream())
    return (y, u8, valid) if return_u8 else (y, valid)
