"""COCO ground truth from an annotation file's `segmentation` fields, rasterised on the device.

The reference builds it per image on the host (coco_instance.py:52-83, 331-338): annToMask of every annotation (frPoly per polygon, their
union, decode; crowd annotations carry an RLE at the image's size), cv2.resize(.., INTER_NEAREST) of every mask to 128x128 and
torch.sum over the masks into the label map its CrossEntropyLoss trains on.  Here the parsed vertex lists and counts -- a few kilobytes per
image -- go to the device and mu_coco_masks does the rest: one workgroup per annotation, no dense full-size mask ever exists in memory.
`ids` is the id map decode_rle would give, so it feeds match_instances / InstanceAP / PanopticQuality unchanged.

The rasterisation is restated from the published maskApi.c (rleFrPoly), NOT pinned to pycocotools (which is not available where this
project is tested); include/maskunet_hip.h holds the contract.  The host side only packs arrays.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream
from .rle import rle_counts_from_string

MAX_PIXELS = 1 << 19
_INT32_MAX = 2 ** 31 - 1


@dataclass
class CocoMasks:
    """Device tensors of one coco_masks call; A = the annotations of all images, image after image."""
    cover: torch.Tensor          # int64 [B,Ho,Wo]  how many valid annotations cover the pixel (the reference's combined_mask)
    ids: torch.Tensor            # int32 [B,Ho,Wo]  the largest (row within the image + 1) among them, else 0
    area: torch.Tensor           # int32 [A]        set pixels at the ORIGINAL size
    valid: torch.Tensor          # int32 [A]        0 = the annotation was rejected and paints nothing
    masks: torch.Tensor | None   # uint8 [A,Ho,Wo]  only with masks=True


def pack_annotations(annotations, sizes):
    """The CSR arrays of mu_coco_masks, on the host (numpy): xy fp64 [2 * points], poly_offsets [P+1] (in points), ann_poly_offsets [A+1],
    rle_counts, ann_rle_offsets [A+1], img_ann_offsets [B+1], sizes int32 [B,2].  annotations: a list (images) of lists of COCO
    `segmentation` values, each a list of polygons (flat [x0, y0, x1, y1, ..]) or a dict whose `counts` is a list of integers or a
    compressed string; sizes: (height, width) per image."""
    sizes = np.asarray(sizes.cpu().numpy() if isinstance(sizes, torch.Tensor) else sizes, dtype=np.int64).reshape(-1, 2)
    if len(annotations) != sizes.shape[0] or sizes.shape[0] < 1:
        raise ValueError(f"{len(annotations)} images of annotations and {sizes.shape[0]} sizes: one (height, width) per image, at least one")
    if bool((sizes < 1).any()) or bool((sizes > _INT32_MAX).any()):
        raise ValueError("sizes must be positive")
    xy, poly_off, ann_poly, counts, ann_rle, img_ann = [], [0], [0], [], [0], [0]
    n_points = 0
    for b, segs in enumerate(annotations):
        h, w = int(sizes[b, 0]), int(sizes[b, 1])
        for seg in segs:
            if isinstance(seg, dict):
                if "size" in seg and list(seg["size"]) != [h, w]:
                    raise ValueError(f"RLE of size {list(seg['size'])} in an image of {[h, w]}")
                c = seg["counts"]
                c = rle_counts_from_string(c) if isinstance(c, (str, bytes)) else [int(v) for v in c]
                if not c:
                    raise ValueError("RLE without counts")
                counts.append(np.clip(np.asarray(c, dtype=np.int64), -1, _INT32_MAX))
            elif isinstance(seg, (list, tuple)):
                for poly in seg:
                    p = np.asarray(poly, dtype=np.float64).reshape(-1)
                    if p.size % 2:
                        raise ValueError(f"polygon with {p.size} coordinates: x, y pairs expected")
                    xy.append(p)
                    n_points += p.size // 2
                    poly_off.append(n_points)
            else:
                raise TypeError(f"segmentation must be a list of polygons or an RLE dict, got {type(seg).__name__}")
            ann_poly.append(len(poly_off) - 1)
            ann_rle.append(ann_rle[-1] + (counts[-1].size if isinstance(seg, dict) else 0))
        img_ann.append(len(ann_poly) - 1)
    if n_points > 2 ** 30 - 1 or ann_rle[-1] > _INT32_MAX:
        raise ValueError("too many points or counts for one call")
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    return {"xy": np.concatenate(xy) if xy else np.zeros(0, np.float64), "poly_offsets": i32(poly_off), "ann_poly_offsets": i32(ann_poly),
            "rle_counts": np.concatenate(counts).astype(np.int32) if counts else np.zeros(0, np.int32), "ann_rle_offsets": i32(ann_rle),
            "img_ann_offsets": i32(img_ann), "sizes": sizes.astype(np.int32)}


def coco_masks(annotations, sizes, out_hw=(128, 128), masks=False, device=None, max_points=1 << 20) -> CocoMasks:
    """Masks and training targets of a batch of COCO annotations at out_hw (the reference: 128x128), see CocoMasks.  An image without
    annotations gives zeros.  An annotation is rejected (valid = 0) if a coordinate is not finite or beyond 2^24 / 5, a polygon walks
    more than max_points upsampled points, or its counts are negative or do not sum to height * width.  Images of one call may differ in
    size; height * width <= 2^19 each and out_hw[0] * out_hw[1] <= 65536.  Never synchronises with the device."""
    packed = pack_annotations(annotations, sizes)
    Ho, Wo, max_points = int(out_hw[0]), int(out_hw[1]), int(max_points)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError("maskunet_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")
    lib = _lib.load()
    hw = packed["sizes"].astype(np.int64)
    if lib.mu_coco_masks_supported(Ho, Wo, max_points) != 0 or bool((hw[:, 0] * hw[:, 1] > MAX_PIXELS).any()):
        raise RuntimeError(f"maskunet_amd: mu_coco_masks failed with MU_ERR_SHAPE: COCO masks need height * width <= {MAX_PIXELS} per "
                           f"image, out_hw[0] * out_hw[1] <= 65536 and 1 <= max_points <= 2097152, got sizes up to "
                           f"{int((hw[:, 0] * hw[:, 1]).max())} pixels, out_hw={(Ho, Wo)}, max_points={max_points}")
    t = {k: torch.from_numpy(v).to(dev) for k, v in packed.items()}
    B, A, P = hw.shape[0], packed["ann_poly_offsets"].size - 1, packed["poly_offsets"].size - 1
    r = CocoMasks(torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev), torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev),
                  torch.empty(A, dtype=torch.int32, device=dev), torch.empty(A, dtype=torch.int32, device=dev),
                  torch.empty((A, Ho, Wo), dtype=torch.uint8, device=dev) if masks else None)
    with torch.cuda.device(dev):
        ws = torch.empty(lib.mu_coco_masks_workspace_bytes(B, A, Ho, Wo), dtype=torch.uint8, device=dev)
        call("mu_coco_masks", ptr(t["xy"]), ptr(t["poly_offsets"]), ptr(t["ann_poly_offsets"]), ptr(t["rle_counts"]),
             ptr(t["ann_rle_offsets"]), ptr(t["img_ann_offsets"]), ptr(t["sizes"]), B, A, P, packed["xy"].size // 2, packed["rle_counts"].size,
             Ho, Wo, max_points, ptr(r.cover), ptr(r.ids), ptr(r.masks), ptr(r.area), ptr(r.valid), ptr(ws), ws.numel(), stream())
    return r
