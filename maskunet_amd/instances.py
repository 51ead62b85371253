"""Instance post-processing of the `*_instance.py` / `*_panoptic.py` scripts on the device.

The reference pulls softmax(outputs / 0.5) to the host and labels it there per class with cv2.connectedComponents
(get_instances_from_mask, ade_instance.py:367-397; evaluate_instances, ade_instance.py:399-425; generate_instance_mask,
ade_panoptic.py:36-47).  Here the logits are read once on the device (mu_argmax_prob) and one workgroup per image labels the class
map, gathers the per-instance statistics and sorts the scores (mu_instances); nothing crosses to the host until the caller asks.

Class 0 is background, and so is every negative value.  An instance is a maximal 8-connected set of pixels of one non-zero class;
ids run 1..count within an image, ordered by each instance's first pixel in raster order.

The 3-head model (`UNet(c_in, c_out, embed_dim=16)`) is evaluated differently: evaluate_instances (city_instance.py:451-482) clusters
the embedding head per predicted class with sklearn's DBSCAN (get_instances_from_embeddings / get_instance_annotations,
city_instance.py:405-449).  instances_from_embeddings does that on the device (mu_dbscan_instances) and returns the same `Instances`.

The ground truth of that script is an id map the dataset supplies (get_instance_annotations(gt_inst, gt_sem), city_instance.py:472-474):
instances_from_id_map (mu_id_instances) numbers its distinct values and takes each instance's class as the median of the semantic map.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._lib import call, dt, ptr, stream
from .losses import _nhwc_source

TABLE_COLUMNS = ("class", "area", "x_min", "y_min", "x_max", "y_max", "first_pixel", "class_rank")


@dataclass
class Instances:
    """Device tensors of one call.  `table` rows / `scores` / `order` hold ids 1..min(count, max_instances); the rest is zero.
    `count` is the true number of instances per image and `ids` is always complete, also past max_instances."""
    classes: torch.Tensor        # int32 [B,H,W]   class map (arg-max of the logits, or the labels)
    ids: torch.Tensor            # int32 [B,H,W]   0 = background, else the instance id
    table: torch.Tensor          # int32 [B,max_instances,8]   TABLE_COLUMNS; row k-1 describes id k
    scores: torch.Tensor         # fp32  [B,max_instances]     mean probability of the instance's class over its pixels (1.0: labels, embeddings)
    count: torch.Tensor          # int32 [B]
    order: torch.Tensor          # int32 [B,max_instances]     ids by descending score (ties: ascending id), padded with 0
    prob: torch.Tensor | None = None     # fp32 [B,H,W] probability of the arg-max class (None for label input)
    values: torch.Tensor | None = None   # int32 [B,max_instances]  the id map's value of id k in row k-1 (instances_from_id_map only)
    invalid: torch.Tensor | None = None  # int32 [B]  instances_from_id_map only: bit 0 = pixels dropped for a class outside [0, class_cap),
                                         #            bit 1 = for an int64 id outside int32; 0 = clean

    def top(self, max_queries):
        """(ids, scores) [B, max_queries] of the reference's sorted(instances, key=score, reverse=True)[:max_queries]; id 0 (score 0)
        pads images with fewer instances.  No host synchronisation."""
        ids = self.order[:, :max_queries]
        sc = torch.gather(self.scores, 1, (ids - 1).clamp_(min=0).long())
        return ids, torch.where(ids > 0, sc, torch.zeros_like(sc))

    def to_reference(self, image, max_queries=None):
        """The reference's list of dicts for one image, on the host, best score first: `bbox` = [x_min, y_min, x_max - x_min,
        y_max - y_min] (no +1, as the reference), `category_id`, `score`, and a boolean `mask` where the reference has the
        pycocotools RLE."""
        order = self.order[image].cpu().tolist()
        table = self.table[image].cpu().tolist()
        scores = self.scores[image].cpu().tolist()
        ids = self.ids[image].cpu()
        if max_queries is not None:
            order = order[:max_queries]
        out = []
        for k in order:
            if k == 0:
                break
            c, _, x0, y0, x1, y1, _, _ = table[k - 1]
            out.append({"bbox": [float(x0), float(y0), float(x1 - x0), float(y1 - y0)], "category_id": int(c),
                        "score": float(scores[k - 1]), "mask": (ids == k).numpy()})
        return out

    def rle(self, max_queries=None):
        """The COCO run-length masks (maskunet_amd.rle.RLEs) of the reference's sorted(...)[:max_queries]: row k of image b is the
        instance order[b, k], the rows past an image's instances are empty.  Encoded on the device; never synchronises."""
        from .rle import encode_rle
        sel = self.order if max_queries is None else self.order[:, :max_queries]
        return encode_rle(self.ids, sel, max_id=self.order.shape[1])


def _class_map(t, what):
    """the contiguous int32 copy of an int64 / int32 [B,H,W] class map on the GPU; `what` is the complaint otherwise"""
    if t.dim() != 3 or t.dtype not in (torch.int64, torch.int32) or not t.is_cuda:
        raise RuntimeError(what)
    return t.to(torch.int32).contiguous()


def _strided_source(t):
    """(x, inner, outer, cs, ps) of a module output [B,C,H,W]: the NHWC tensor an untouched output was converted from, else the
    contiguous NCHW tensor, with the pixel / channel strides the kernels take"""
    B, C, H, W = t.shape
    src = _nhwc_source(t)
    if src is not None and src[0].is_contiguous():
        x = src[0].detach()
        return x, B * H * W, 0, 1, x.shape[-1]
    return t.detach().contiguous(), H * W, C * H * W, H * W, 1


def _argmax_prob(logits, temperature):
    """(classes int32, prob fp32) [B,H,W]: the first arg-max of the logits [B,C,H,W] and softmax(logits / temperature) of it"""
    B, C, H, W = logits.shape
    x, inner, outer, cs, ps = _strided_source(logits)
    classes = torch.empty((B, H, W), dtype=torch.int32, device=x.device)
    prob = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    call("mu_argmax_prob", ptr(x), B * H * W, C, inner, outer, cs, ps, 1.0 / float(temperature), ptr(classes), ptr(prob), dt(x), stream())
    return classes, prob


def _outputs(B, H, W, max_instances, device):
    """ids, table, scores, count, order: the five tensors every producer fills"""
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.empty((B, H, W), **i32), torch.empty((B, max_instances, 8), **i32),
            torch.empty((B, max_instances), dtype=torch.float32, device=device), torch.empty(B, **i32), torch.empty((B, max_instances), **i32))


def _label(classes, prob, max_instances):
    B, H, W = classes.shape
    lib = _lib.load()
    max_instances = int(max_instances)
    if lib.mu_instances_supported(H, W, max_instances) != 0:
        raise RuntimeError(f"maskunet_amd: instances need H*W <= 65536 and 1 <= max_instances <= 4096, got {H}x{W}, {max_instances}")
    out = _outputs(B, H, W, max_instances, classes.device)
    ws = torch.empty(lib.mu_instances_workspace_bytes(B, H, W, max_instances), dtype=torch.uint8, device=classes.device)
    call("mu_instances", ptr(classes), ptr(prob), B, H, W, max_instances, *map(ptr, out), ptr(ws), ws.numel(), stream())
    return Instances(classes, *out, prob)


def predict_instances(outputs, temperature=0.5, max_instances=1024):
    """evaluate_instances' post-processing (ade_instance.py:408-419) of the module output `outputs` [B,C,H,W] (fp32 or fp16): class =
    first arg-max of the logits, probability = softmax(outputs / temperature) of that class, instances and their mean-probability
    scores.  An untouched output of a maskunet_amd module is read through the NHWC tensor it was converted from.  Never synchronises."""
    if outputs.dim() != 4 or not outputs.is_cuda:
        raise RuntimeError("predict_instances expects the module output [B,C,H,W] on the GPU")
    if not temperature > 0:
        raise ValueError("temperature must be positive")
    return _label(*_argmax_prob(outputs, temperature), max_instances)


def instances_from_labels(labels, max_instances=1024):
    """Instances of an int64 / int32 class map [B,H,W] (the ground-truth side: every score is 1.0)."""
    return _label(_class_map(labels, "instances_from_labels expects an int64 / int32 [B,H,W] class map on the GPU"), None, max_instances)


def instances_from_id_map(instance_mask, semantic_mask, max_instances=1024, class_cap=256):
    """Ground-truth instances of an id map the dataset supplies: get_instance_annotations(gt_inst, gt_sem) (city_instance.py:431-449).
    `instance_mask`: int32 / int64 [B,H,W] (Cityscapes instanceIds, coco_masks(...).ids) or a uint8 [B,H,W,3] RGB image, read as
    R + 256 G + 65536 B (panopticapi's rgb2id of a COCO panoptic PNG).  `semantic_mask`: int32 / int64 [B,H,W].  Id k is the set of
    pixels with the k-th distinct non-zero value in ascending signed order (np.unique), connected or not; its class is
    int(np.median(semantic_mask[mask])); every score is 1.0; `values` holds the value of each id.  A pixel of a non-zero id whose class
    is outside [0, class_cap), or whose int64 id does not fit int32, is dropped (counts as id 0) and reported in `invalid`.
    Never synchronises."""
    m, c = instance_mask, semantic_mask
    if not (torch.is_tensor(m) and torch.is_tensor(c) and m.is_cuda and c.is_cuda):
        raise RuntimeError("instances_from_id_map expects the id map and the semantic map on the GPU")
    rgb = m.dtype == torch.uint8
    if not ((rgb and m.dim() == 4 and m.shape[-1] == 3) or (m.dtype in (torch.int64, torch.int32) and m.dim() == 3)):
        raise RuntimeError("instances_from_id_map expects an int64 / int32 [B,H,W] id map or a uint8 [B,H,W,3] RGB image")
    classes = _class_map(c, "instances_from_id_map expects an int64 / int32 [B,H,W] semantic map")
    if tuple(m.shape[:3]) != tuple(c.shape):
        raise RuntimeError("the id map and the semantic map differ in batch or image size")
    B, H, W = c.shape
    lib = _lib.load()
    max_instances, class_cap = int(max_instances), int(class_cap)
    if B < 1 or lib.mu_id_instances_supported(H, W, max_instances, class_cap) != 0:
        raise RuntimeError("maskunet_amd: id-map instances need B >= 1, H*W <= 65536, 1 <= max_instances <= 4096 and "
                           f"1 <= class_cap <= 1024, got {B}x{H}x{W}, {max_instances}, {class_cap}")
    kind = _lib.MU_IDMAP_RGB8 if rgb else (_lib.MU_IDMAP_I64 if m.dtype == torch.int64 else _lib.MU_IDMAP_I32)
    m = m.contiguous()
    dev = classes.device
    out = _outputs(B, H, W, max_instances, dev)
    values = torch.empty((B, max_instances), dtype=torch.int32, device=dev)
    invalid = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mu_id_instances_workspace_bytes(B, H, W, max_instances, class_cap), dtype=torch.uint8, device=dev)
    call("mu_id_instances", ptr(m), kind, ptr(classes), B, H, W, max_instances, class_cap, *map(ptr, out), ptr(values), ptr(invalid),
         ptr(ws), ws.numel(), stream())
    return Instances(classes, *out, None, values, invalid)


def generate_instance_mask(semantic_mask, max_instances=1024):
    """generate_instance_mask of the panoptic datasets (ade_panoptic.py:36-47): an int32 map in which every pixel holds the 1-based
    number of its connected component WITHIN ITS CLASS (numbers restart per class -- the reference's quirk, and what it feeds to
    InstanceContrastiveLoss); 0 = background, -1 = instance past `max_instances`.  Components of a class are numbered by their first
    pixel in raster order.  Accepts [H,W] or [B,H,W]."""
    squeeze = semantic_mask.dim() == 2
    r = instances_from_labels(semantic_mask[None] if squeeze else semantic_mask, max_instances)
    B = r.ids.shape[0]
    lut = torch.cat([torch.zeros((B, 1), dtype=torch.int32, device=r.ids.device), r.table[:, :, 7]], 1)      # id -> class_rank
    ids = r.ids.view(B, -1).long()
    over = ids > max_instances
    out = torch.gather(lut, 1, ids.clamp(max=max_instances))
    out = torch.where(over, torch.full_like(out, -1), out).view_as(r.ids)
    return out[0] if squeeze else out


def instances_from_embeddings(semantic, embeddings, eps=0.5, min_samples=5, temperature=0.5, max_instances=1024, num_classes=None):
    """evaluate_instances' post-processing of the 3-head model (city_instance.py:459-475): per image and per class c >= 1,
    DBSCAN(eps, min_samples) over the embeddings of the class's pixels; ids run over (class ascending, clusters by their lowest core
    point), noise is 0, every score is 1.0 (so `top()` is ascending id, as the reference's stable sort).
    `semantic`: the logits [B,C,H,W] (class = first arg-max, `prob` = softmax(logits / temperature) of it, num_classes defaults to C)
    or an int32 / int64 class map [B,H,W] (num_classes required).  `embeddings`: [B,D,H,W], fp32 or fp16, finite.  Untouched module
    outputs are read through the NHWC tensors they were converted from.  Never synchronises."""
    if embeddings.dim() != 4 or not embeddings.is_cuda or not semantic.is_cuda:
        raise RuntimeError("instances_from_embeddings expects the module outputs on the GPU: semantic [B,C,H,W] or [B,H,W], embeddings [B,D,H,W]")
    B, D, H, W = embeddings.shape
    prob = None
    if semantic.dim() == 4:
        if not temperature > 0:
            raise ValueError("temperature must be positive")
        if tuple(semantic.shape[0:1] + semantic.shape[2:]) != (B, H, W):
            raise RuntimeError("semantic and embeddings differ in batch or image size")
        num_classes = semantic.shape[1] if num_classes is None else int(num_classes)
        classes, prob = _argmax_prob(semantic, temperature)
    else:
        what = "semantic must be the logits [B,C,H,W] or an int64 / int32 class map [B,H,W] of the embeddings' size"
        classes = _class_map(semantic, what)
        if tuple(semantic.shape) != (B, H, W):
            raise RuntimeError(what)
        if num_classes is None:
            raise ValueError("num_classes is required with a class map")
        num_classes = int(num_classes)
    lib = _lib.load()
    max_instances, min_samples = int(max_instances), int(min_samples)
    if lib.mu_dbscan_supported(H, W, D, num_classes, max_instances) != 0 or min_samples < 1 or not eps > 0:
        raise RuntimeError("maskunet_amd: embedding instances need H*W <= 65536, 1 <= D <= 64, 1 <= num_classes <= 1024, "
                           f"1 <= max_instances <= 4096, min_samples >= 1, eps > 0; got {H}x{W}, D={D}, {num_classes} classes, "
                           f"{max_instances}, {min_samples}, {eps}")
    e, inner, outer, cs, ps = _strided_source(embeddings)
    out = _outputs(B, H, W, max_instances, e.device)
    ws = torch.empty(lib.mu_dbscan_workspace_bytes(B, H, W, num_classes, max_instances), dtype=torch.uint8, device=e.device)
    call("mu_dbscan_instances", ptr(classes), ptr(e), B, H, W, D, inner, outer, cs, ps, dt(e), num_classes, float(eps), min_samples,
         max_instances, *map(ptr, out), ptr(ws), ws.numel(), stream())
    return Instances(classes, *out, prob)
