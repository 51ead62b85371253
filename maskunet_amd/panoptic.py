"""Panoptic segments on the device: the stage save_predictions / evaluate_panoptic (coco_panoptic.py:388-439) leave open.

The reference writes every prediction as a COCO panoptic PNG (panopticapi's id2rgb) and lists it in predictions.json for pq_compute,
with `segments_info` left empty ("You need to fill instance details").  panoptic_segments fills it: the semantic map and the instances
of any producer (predict_instances, instances_from_labels, instances_from_embeddings, instances_from_id_map) are merged into segments
by one kernel, one workgroup per image (mu_panoptic), and nothing crosses to the host until the caller asks for the host lists.

The rule (include/maskunet_hip.h) restates panopticapi's published format -- id2rgb, segments_info, ONE segment per
stuff class and image -- and the usual semantic + instance merge; it is not pinned to the package.  For a pixel with instance id k and
class c:
  thing   k is an instance whose table class is a thing: the pixel belongs to thing candidate k, kept iff its area >= thing_area_limit
          and its score >= score_threshold.  The pixels of a candidate that is not kept are void; they do not become stuff.
  stuff   otherwise, c is a stuff class: kept iff the image has at least max(stuff_area_limit, 1) such pixels, and all of them are
          one segment, connected or not.
  void    everything else.
Kept segments are numbered 1..count by their first pixel in raster order.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._lib import call, ptr, stream
from .instances import Instances, predict_instances


@dataclass
class Panoptic:
    """Device tensors of one call.  The per-segment rows hold segments 1..min(count, max_segments); the rest is zero.  `count` is the
    true number of segments per image and `seg` is always complete, also past max_segments."""
    seg: torch.Tensor            # int32 [B,H,W]   0 = void, else the segment number
    seg_cls: torch.Tensor        # int32 [B,H,W]   the segment's class (the instance's class of a thing), 0 on void
    table: torch.Tensor          # int32 [B,max_segments,8]   instances.TABLE_COLUMNS; class_rank counts the kept segments of the class
    scores: torch.Tensor         # fp32  [B,max_segments]     the source instance's score of a thing, 1.0 of stuff
    count: torch.Tensor          # int32 [B]
    order: torch.Tensor          # int32 [B,max_segments]     segments by descending score (ties: ascending number), padded with 0
    source: torch.Tensor         # int32 [B,max_segments]     the input instance id of a thing, 0 of stuff
    values: torch.Tensor         # int32 [B,max_segments]     COCO segment id: category * label_divisor + (class_rank of a thing, 0 of
                                 #                            stuff); 0 where that id is not representable (invalid bit 0)
    id_map: torch.Tensor         # int32 [B,H,W]   `values` of the pixel's segment, 0 on void
    rgb: torch.Tensor            # uint8 [B,H,W,3] panopticapi's id2rgb of id_map: R = v & 255, G = (v >> 8) & 255, B = v >> 16
    invalid: torch.Tensor        # int32 [B]  bit 0 = a segment id <= 0, >= 2^24 or a thing rank >= label_divisor (its pixels are 0 in
                                 #            id_map and black), bit 1 = more than max_segments segments (rows past it dropped, their
                                 #            pixels likewise), bit 2 = pixels of an instance past the input's max_instances (void)
    category: torch.Tensor       # int32 [num_classes]  the dataset's category id of every class (`category_ids`)
    bgr: bool = False            # the channel order of `rgb`

    @property
    def instances(self):
        """The segments as an `Instances`, which match_instances, coco_match, PanopticQuality, encode_rle and Instances.rle() take
        as they are."""
        return Instances(self.seg_cls, self.seg, self.table, self.scores, self.count, self.order, None, self.values, self.invalid)

    def segments_info(self, image):
        """panopticapi's `segments_info` of one image, on the host, in segment order: {"id", "category_id", "area", "bbox", "iscrowd"}
        with bbox = [x_min, y_min, x_max - x_min + 1, y_max - y_min + 1] -- COCO's box, a single pixel is [x, y, 1, 1].  This differs
        from Instances.to_reference, which keeps the reference's boxes without the +1.  "category_id" is the dataset's id of the class
        (`category_ids`).  Synchronises."""
        table = self.table[image].cpu().tolist()
        values = self.values[image].cpu().tolist()
        category = self.category.cpu().tolist()
        out = []
        for r in range(min(int(self.count[image]), len(table))):
            c, area, x0, y0, x1, y1, _, _ = table[r]
            out.append({"id": values[r], "category_id": category[c], "area": area, "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1],
                        "iscrowd": 0})
        return out

    def annotation(self, image, image_id, file_name=None):
        """One entry of predictions.json's "annotations" (coco_panoptic.py:425-429): `file_name` defaults to f"{image_id}.png", as the
        reference writes it.  Synchronises."""
        return {"image_id": image_id, "file_name": f"{image_id}.png" if file_name is None else file_name,
                "segments_info": self.segments_info(image)}


_tables = {}


def _class_tables(things, void, category_ids, device):
    """(kind, category) int32 [num_classes] on the device; one upload per distinct argument set"""
    key = (things, void, category_ids, device.type, device.index)
    t = _tables.get(key)
    if t is None:
        kind = [0 if c in void else 2 if th else 1 for c, th in enumerate(things)]
        t = _tables[key] = (torch.tensor(kind, dtype=torch.int32, device=device), torch.tensor(category_ids, dtype=torch.int32, device=device))
    return t


def panoptic_segments(inst, things, void=(0,), category_ids=None, label_divisor=1000, stuff_area_limit=0, thing_area_limit=0,
                      score_threshold=0.0, max_segments=1024, bgr=False) -> Panoptic:
    """The panoptic segments of an `Instances` (module docstring for the rule).  `things`: one boolean per class; `void`: the classes
    that are neither thing nor stuff (class 0 is background in this project); `category_ids`: the dataset's category id per class, the
    inverse of the reference's cat2label, the identity by default.

    `rgb` is stored R,G,B -- what PIL.Image.fromarray(rgb).save(..) needs -- or B,G,R with bgr=True, which is what cv2.imwrite needs to
    put a correct panoptic PNG on disk.  The reference hands the R,G,B array of id2rgb to cv2.imwrite (coco_panoptic.py:394-397) and so
    writes files with R and B swapped; that is not copied.  Writing the file stays host work.  Never synchronises."""
    if not isinstance(inst, Instances):
        raise TypeError("panoptic_segments expects an Instances")
    if not (inst.ids.is_cuda and inst.classes.is_cuda) or inst.ids.dim() != 3 or tuple(inst.ids.shape) != tuple(inst.classes.shape):
        raise RuntimeError("panoptic_segments expects the class map and the ids [B,H,W] of an Instances on the GPU")
    things = tuple(bool(t) for t in things)
    void = tuple(sorted({int(c) for c in void}))
    C = len(things)
    if C < 1:
        raise ValueError("things: one boolean per class")
    category_ids = tuple(range(C)) if category_ids is None else tuple(int(c) for c in category_ids)
    if len(category_ids) != C:
        raise ValueError(f"category_ids: one id per class, got {len(category_ids)} for {C} classes")
    if any(c < 0 or c >= C for c in void):
        raise ValueError(f"void lists a class outside [0, {C})")
    both = [c for c in void if things[c]]
    if both:
        raise ValueError(f"classes {both} are listed as thing and as void")
    B, H, W = inst.ids.shape
    max_inst = inst.table.shape[1]
    lib = _lib.load()
    max_segments, label_divisor, stuff_area_limit, thing_area_limit = int(max_segments), int(label_divisor), int(stuff_area_limit), int(thing_area_limit)
    if B < 1 or lib.mu_panoptic_supported(H, W, max_inst, C, max_segments, label_divisor, stuff_area_limit, thing_area_limit) != 0:
        raise RuntimeError("maskunet_amd: panoptic segments need B >= 1, H*W <= 65536, 1 <= max_instances <= 4096, 1 <= max_segments <= 4096, "
                           "1 <= classes <= 1024, label_divisor >= 1 and area limits >= 0; got "
                           f"{B}x{H}x{W}, {max_inst}, {max_segments}, {C} classes, {label_divisor}, {stuff_area_limit}, {thing_area_limit}")
    dev = inst.ids.device
    kind, category = _class_tables(things, void, category_ids, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    cls, ids, table, score, count = (t.contiguous() for t in (inst.classes, inst.ids, inst.table, inst.scores, inst.count))
    out = (torch.empty((B, H, W), **i32), torch.empty((B, H, W), **i32), torch.empty((B, max_segments, 8), **i32),
           torch.empty((B, max_segments), dtype=torch.float32, device=dev), torch.empty(B, **i32), torch.empty((B, max_segments), **i32),
           torch.empty((B, max_segments), **i32), torch.empty((B, max_segments), **i32), torch.empty((B, H, W), **i32),
           torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev), torch.empty(B, **i32))
    ws = torch.empty(lib.mu_panoptic_workspace_bytes(B, H, W, max_inst, C, max_segments), dtype=torch.uint8, device=dev)
    call("mu_panoptic", ptr(cls), ptr(ids), ptr(table), ptr(score), ptr(count), ptr(kind), ptr(category), B, H, W, max_inst, C,
         label_divisor, stuff_area_limit, thing_area_limit, float(score_threshold), max_segments, int(bool(bgr)), *map(ptr, out), ptr(ws),
         ws.numel(), stream())
    return Panoptic(*out, category, bool(bgr))


def predict_panoptic(outputs, things, temperature=0.5, max_instances=1024, **kw) -> Panoptic:
    """panoptic_segments(predict_instances(outputs, temperature, max_instances), things, **kw): the module output [B,C,H,W] to panoptic
    segments without leaving the device."""
    return panoptic_segments(predict_instances(outputs, temperature, max_instances), things, **kw)
