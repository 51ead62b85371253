"""Sample preparation of the loaders that read with OpenCV, on the device, for ragged batches.

Nine reference scripts load with cv2; eight of them also prepare their samples with it (the COCO instance loader resizes with Pillow:
images.resize_pil_to_nhwc, coco.coco_masks).  Their images and label maps have sizes of their own, their id maps are 8, 16 or 32 bits
wide, and the two COCO panoptic loaders build their targets from a PNG and a JSON list per sample.  Here a batch goes from decoded bytes
to (input, semantic target, instance target) in three launches:

    resize_cv2_to_nhwc   cv2.cvtColor(BGR2RGB) -> cv2.resize(.., INTER_LINEAR) -> ToTensor()            mu_cv2_resize_ragged_u8_nhwc
    resize_labels_cv2    cv2.resize(.., INTER_NEAREST) -> .long() with `// 1000` and the class clean-ups   mu_cv2_nearest_ragged
    panoptic_targets     rgb2id -> the segments_info loop -> two INTER_NEAREST resizes -> .long()          mu_panoptic_targets

include/maskunet_hip.h holds the contracts.  The resize rules are the restated OpenCV 4.10 ones that ops.resize_u8_to_nhwc and
ops.resize_labels_u8 run for uniform batches: exact against that restatement, not pinned to bytes of a real cv2 build (cv2 is not
vendored by the reference).  The host side only packs arrays; nothing here synchronises with the device.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import call, dt, ptr, stream
from .images import MAX_SIDE, PackedImages, _pad32, pack_images

SEG_MAX = _lib.MU_PANOPTIC_SEG_MAX
_NO_GPU = "maskunet_amd: tensors must live on the GPU (the HIP path has no CPU fallback); pass device= for host data"
_KIND_OF = {torch.uint8: _lib.MU_MAP_U8, torch.uint16: _lib.MU_MAP_U16, torch.int32: _lib.MU_MAP_I32}
_BPP = {_lib.MU_MAP_U8: 1, _lib.MU_MAP_U16: 2, _lib.MU_MAP_I32: 4, _lib.MU_MAP_RGB8: 3, _lib.MU_MAP_BGR8: 3}


@dataclass
class PackedMaps:
    """A ragged batch of id maps as mu_cv2_nearest_ragged takes it; the three tensors live on one device (or all on the host)."""
    data: torch.Tensor           # uint8 [sum h * w * bytes per pixel]   the maps' bytes, one after the other
    offsets: torch.Tensor        # int64 [B+1]                           byte offset of every map in data
    sizes: torch.Tensor          # int32 [B,2]                           (height, width)
    kind: int                    # MU_MAP_U8 / _U16 / _I32 / _RGB8
    max_h: int                   # the bounds the host passes
    max_w: int


@dataclass
class PanopticTargets:
    semantic: torch.Tensor       # int64 [B,Hd,Wd]   the segment's label; 0 where the pixel's id is not listed; `fill` in a refused image
    instance: torch.Tensor       # int64 [B,Hd,Wd]   the segment's id; 0 where it is not listed and in a refused image
    valid: torch.Tensor          # uint8 [B]         0 for an image the kernel refused


def _as_bytes(t):
    """the elements of a tensor as a flat uint8 tensor (torch's uint16 has few operators: everything travels as bytes)"""
    return t.contiguous().reshape(-1).view(torch.uint8)


def pack_maps(maps, device=None) -> PackedMaps:
    """maps: a list of [h, w] uint8 / uint16 / int32 arrays or tensors, or of [h, w, 3] uint8 ones (RGB-coded ids, three bytes per pixel),
    all of one kind and all on the host or all on one device; or one uniform [B, H, W] tensor of those types, or one uint8 [B, H, W, 3]
    tensor.  One torch.cat and at most one host-to-device copy, built like pack_images: offsets and sizes lead the buffer, so every map
    starts element-aligned.  device=None leaves the result where the maps are."""
    dev = None if device is None else torch.device(device)
    if isinstance(maps, (torch.Tensor, np.ndarray)):
        t = torch.as_tensor(maps)
        if t.dim() not in (3, 4) or (t.dim() == 4 and t.shape[3] != 3):
            raise ValueError(f"pack_maps expects a list of maps, one [B, H, W] tensor or one [B, H, W, 3] tensor, got {tuple(t.shape)}")
        if t.shape[0] < 1:
            raise ValueError("pack_maps needs at least one map")
        ts, rgb = [t], t.dim() == 4
        shapes = [(int(t.shape[1]), int(t.shape[2]))] * int(t.shape[0])
    else:
        ts = [torch.as_tensor(m) for m in maps]
        if not ts:
            raise ValueError("pack_maps needs at least one map")
        for t in ts:
            if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3):
                raise ValueError(f"every map must be [h, w] or [h, w, 3], got {tuple(t.shape)}")
        if len({t.dim() for t in ts}) != 1 or len({t.dtype for t in ts}) != 1:
            raise ValueError("the maps of one call share an element type and a layout")
        if len({t.device for t in ts}) != 1:
            raise ValueError("the maps of one call live on one device (or all on the host)")
        rgb = ts[0].dim() == 3
        shapes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    dtype = ts[0].dtype
    if rgb and dtype != torch.uint8:
        raise ValueError(f"[h, w, 3] maps must be uint8, got {dtype}")
    if dtype not in _KIND_OF:
        raise ValueError(f"maps must be uint8, uint16 or int32, got {dtype}")
    kind = _lib.MU_MAP_RGB8 if rgb else _KIND_OF[dtype]
    sizes = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    if bool((sizes < 1).any()) or bool((sizes > MAX_SIDE).any()):
        raise ValueError(f"map sides must lie in [1, {MAX_SIDE}], got heights {sizes[:, 0].min()}..{sizes[:, 0].max()}, widths {sizes[:, 1].min()}..{sizes[:, 1].max()}")
    offsets = np.zeros(sizes.shape[0] + 1, dtype=np.int64)
    np.cumsum(sizes[:, 0] * sizes[:, 1] * _BPP[kind], out=offsets[1:])
    meta = torch.from_numpy(np.concatenate([offsets.view(np.uint8), sizes.astype(np.int32).reshape(-1).view(np.uint8)]))
    nb_off, nb_meta = offsets.size * 8, meta.numel()         # 8 * (2 B + 1) bytes: the maps behind them stay aligned for every kind
    flat = [_as_bytes(t) for t in ts]
    src_dev = flat[0].device
    if src_dev.type == "cpu":
        buf = torch.cat([meta] + flat)                       # the one cat; then the one copy
        if dev is not None and dev.type != "cpu":
            buf = buf.to(dev)
        meta, data = buf[:nb_meta], buf[nb_meta:]
    else:
        if dev is not None and dev != src_dev and not (dev.type == src_dev.type and dev.index is None):
            raise ValueError(f"the maps live on {src_dev}, not on {dev}")
        meta = meta.to(src_dev)
        data = flat[0] if len(flat) == 1 else torch.cat(flat)
    return PackedMaps(data, meta[:nb_off].view(torch.int64), meta[nb_off:].view(torch.int32).view(-1, 2), kind,
                      int(sizes[:, 0].max()), int(sizes[:, 1].max()))


def _out_size(size, B, max_h, max_w):
    """(Hd, Wd) of a cv2-style size = (width, height), refused on the host where the kernels would refuse it"""
    Wd, Hd = int(size[0]), int(size[1])
    if _lib.load().mu_cv2_ragged_supported(B, max_h, max_w, Hd, Wd) != 0:
        raise ValueError(f"size = (width, height) and the image sides must lie in [1, {MAX_SIDE}] and the batch within 2^31 blocks, "
                         f"got size {(Wd, Hd)}, sides up to {(max_h, max_w)}, B = {B}")
    return Hd, Wd


def _on_gpu(packed):
    if packed.data.device.type != "cuda":
        raise RuntimeError(_NO_GPU)
    return packed.data.device


def resize_cv2_to_nhwc(images, size=(128, 128), dtype=torch.float32, bgr=False, return_u8=False, device=None):
    """Decoded image bytes of ANY sizes -> the network input [B, Hd, Wd, pad32(C)] in `dtype` by the cv2 loaders' pipeline
    cv2.cvtColor(BGR2RGB) (bgr=True: cv2.imread bytes) -> cv2.resize(.., size, INTER_LINEAR) -> ToTensor(): for every image exactly the
    bytes ops.resize_u8_to_nhwc gives for it alone.  size = (width, height) like cv2.  images: what pack_images takes, or a PackedImages.
    Returns (y, valid) or (y, u8, valid): u8 [B, Hd, Wd, C] are the resized bytes, valid uint8 [B] is 0 for an image the kernel refused
    (its slot of a hand-made PackedImages too short, its size outside the bounds), whose outputs are zero.  Host images need `device`.
    Never synchronises with the device.  No gradient."""
    packed = images if isinstance(images, PackedImages) else pack_images(images, device)
    dev = _on_gpu(packed)
    B, C = packed.sizes.shape[0], packed.channels
    Hd, Wd = _out_size(size, B, packed.max_h, packed.max_w)
    Cp = _pad32(C)
    y = torch.empty((B, Hd, Wd, Cp), dtype=dtype, device=dev)
    u8 = torch.empty((B, Hd, Wd, C), dtype=torch.uint8, device=dev) if return_u8 else None
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        call("mu_cv2_resize_ragged_u8_nhwc", ptr(packed.data), ptr(packed.offsets), ptr(packed.sizes), B, C, packed.max_h, packed.max_w,
             int(bool(bgr)), ptr(y), ptr(u8), ptr(valid), Hd, Wd, Cp, dt(y), stream())
    return (y, u8, valid) if return_u8 else (y, valid)


def resize_labels_cv2(maps, size=(128, 128), divisor=1, num_classes=None, fill=255, device=None):
    """Id maps of ANY sizes -> (int64 [B, Hd, Wd], valid): torch.from_numpy(cv2.resize(m, size, interpolation=cv2.INTER_NEAREST)).long()
    with the Cityscapes clean-ups folded in.  divisor > 1 is `m // divisor` (Python's floor division; city_instance.py:85 divides by 1000
    before the resize, which commutes with it); num_classes = n replaces every value outside [0, n) by `fill` (np.where((m >= 0) &
    (m < 19), m, 255), city_semantic.py:84; mask[mask >= n] = 255, city_instance.py:106).  maps: what pack_maps takes, or a PackedMaps.
    size = (width, height).  Every element of a refused map (valid = 0) is `fill`.  Never synchronises.  No gradient."""
    packed = maps if isinstance(maps, PackedMaps) else pack_maps(maps, device)
    dev = _on_gpu(packed)
    B = packed.sizes.shape[0]
    Hd, Wd = _out_size(size, B, packed.max_h, packed.max_w)
    divisor, n = int(divisor), 0 if num_classes is None else int(num_classes)
    if divisor < 1 or divisor >= 2 ** 31 or n < (0 if num_classes is None else 1) or n >= 2 ** 31:
        raise ValueError(f"divisor and num_classes must be positive int32 values, got {divisor}, {num_classes}")
    out = torch.empty((B, Hd, Wd), dtype=torch.int64, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        call("mu_cv2_nearest_ragged", ptr(packed.data), ptr(packed.offsets), ptr(packed.sizes), packed.kind, B, packed.max_h, packed.max_w,
             divisor, n, int(fill), ptr(out), ptr(valid), Hd, Wd, stream())
    return out, valid


def pack_segments(segments_info, cat2label=None):
    """The segment tables of mu_panoptic_targets on the host: segments_info is the panoptic JSON's list of dicts with "id" and "category_id"
    per image.  Returns int32 numpy arrays (seg_ids [S], seg_labels [S], img_seg_offsets [B+1]); the ids of one image are strictly
    ascending, and of two entries with one id the later one stays, as the reference's loop lets it overwrite the earlier
    (coco_panoptic.py:78-85).  cat2label: dict, None = identity; a category that is not in it raises KeyError as the reference does."""
    ids, labels, offsets = [], [], [0]
    for segs in segments_info:
        table = {}
        for seg in segs:
            cat = seg["category_id"]
            table[int(seg["id"])] = int(cat if cat2label is None else cat2label[cat])
        if len(table) > SEG_MAX:
            raise ValueError(f"an image has {len(table)} segments, more than the {SEG_MAX} the kernel's table holds")
        for k in sorted(table):
            ids.append(k)
            labels.append(table[k])
        offsets.append(len(ids))
    both = np.asarray([ids, labels], dtype=np.int64).reshape(2, -1)
    if both.size and (both.min() < -2 ** 31 or both.max() >= 2 ** 31):
        raise ValueError("segment ids and labels must fit int32")
    return both[0].astype(np.int32), both[1].astype(np.int32), np.asarray(offsets, dtype=np.int32)


def panoptic_targets(pngs, segments_info, size=(128, 128), cat2label=None, bgr=False, fill=255, device=None) -> PanopticTargets:
    """The targets of the COCO panoptic loader (coco_panoptic.py:70-95; .semantic alone is coco_semantic.py:70-86) from the decoded panoptic
    PNGs and the JSON's segments_info: id = rgb2id of the pixel, semantic = label of the segment with that id, instance = the id, both 0
    where the id is not listed, sampled by cv2.resize(.., size, INTER_NEAREST), as int64 [B, Hd, Wd].  pngs: a list of uint8 [h, w, 3]
    images or one [B, H, W, 3] tensor (what pack_images takes), or a PackedImages; bgr=True takes cv2.imread bytes.  size = (width,
    height).  segments_info: per image the list of dicts with "id" and "category_id"; cat2label as in pack_segments.  An image the kernel
    refuses (valid = 0) has semantic = fill and instance = 0.  The result feeds instances_from_id_map(t.instance, t.semantic),
    CrossEntropyLoss, InstanceContrastiveLoss and SemanticMetrics as it is.  One small host-to-device copy for the tables; never
    synchronises.  No gradient."""
    seg_ids, seg_labels, seg_off = pack_segments(segments_info, cat2label)       # first: a KeyError costs no copy
    packed = pngs if isinstance(pngs, PackedImages) else pack_images(pngs, device)
    dev = _on_gpu(packed)
    B, S = packed.sizes.shape[0], int(seg_ids.size)
    if packed.channels != 3:
        raise ValueError(f"panoptic PNGs have 3 channels, got {packed.channels}")
    if seg_off.size != B + 1:
        raise ValueError(f"segments_info has {seg_off.size - 1} entries for {B} images")
    Hd, Wd = _out_size(size, B, packed.max_h, packed.max_w)
    tables = torch.from_numpy(np.concatenate([seg_off, seg_ids, seg_labels])).to(dev)    # the one copy
    t_off, t_ids, t_labels = tables[:B + 1], tables[B + 1:B + 1 + S], tables[B + 1 + S:]
    semantic = torch.empty((B, Hd, Wd), dtype=torch.int64, device=dev)
    instance = torch.empty((B, Hd, Wd), dtype=torch.int64, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        call("mu_panoptic_targets", ptr(packed.data), ptr(packed.offsets), ptr(packed.sizes), ptr(t_ids) if S else None,
             ptr(t_labels) if S else None, ptr(t_off), B, S, packed.max_h, packed.max_w, int(bool(bgr)), int(fill), ptr(semantic),
             ptr(instance), ptr(valid), Hd, Wd, stream())
    return PanopticTargets(semantic, instance, valid)
