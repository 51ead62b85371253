"""Semantic evaluation of a validation set on the device: the counterpart of InstanceAP / PanopticQuality for the semantic side.

Every reference script validates with

    outputs = model(inputs); loss = criterion(outputs, labels); total_val_iou += mean_iou(outputs, labels, c_out)
    total_val_loss += loss.item()                                                  (ade_semantic.py:450-457, one sync per batch)

and the instance / panoptic ones add softmax(outputs / 0.5) + argmax (ade_instance.py:408-411) and a per-image
compute_iou_for_image on the host (city_panoptic.py:212-222).  `semantic_eval` takes all of it from ONE read of the logits
(mu_sem_eval): per-image class counts, per-image cross-entropy sums, a running confusion matrix and, on request, the class map and
probability that the instance labelling consumes.  `SemanticMetrics` accumulates updates without ever synchronising; `compute()`
brings the counters to the host once and derives the dataset-level metrics (the precision / recall / F1 / Jaccard that the scripts
import from sklearn, pixel accuracy) and the three numbers the scripts print.  All host arithmetic is `metrics_from_counts`.

The scripts score the network-size class map against labels resized down to it.  `semantic_eval_native` /
`SemanticMetrics.update_native` score at each label map's OWN size instead, as the datasets define mIoU: bilinear upsampling, arg-max
and counting in one kernel over a ragged batch of label maps (mu_sem_eval_native), into the same accumulator.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import call, dt, ptr, stream, workspace
from .instances import _label, _strided_source

LDS_MAX_CLASSES = 192        # MU_SEM_EVAL_LDS_MAX_C of include/maskunet_hip.h: up to here a workgroup keeps the confusion counters in LDS


@dataclass
class SemanticBatch:
    """Device tensors of one semantic_eval call (contract: mu_sem_eval in include/maskunet_hip.h)."""
    img_counts: torch.Tensor             # int32 [B,3,C]  per image I_c, P_c, L_c (P over every pixel, I and L over non-void ones)
    img_loss: torch.Tensor               # fp64  [B,2]    per image: sum of the cross-entropy over non-void pixels, their number
    confusion: torch.Tensor              # int64 [C+1,C]  row = label (C: void), column = prediction; the tensor that was added into
    classes: torch.Tensor | None = None  # int32 [B,H,W]  first arg-max of the logits
    prob: torch.Tensor | None = None     # fp32  [B,H,W]  softmax(outputs / temperature) of that class

    def instances(self, max_instances=1024):
        """The Instances that predict_instances gives for the same output, from the class map and probability of this sweep."""
        if self.classes is None:
            raise RuntimeError("SemanticBatch.instances needs the class map: call semantic_eval / update with classes=True")
        return _label(self.classes, self.prob, max_instances)


def _source(outputs, labels, num_classes):
    """(x, C, inner, outer, cs, ps) of the logits: the module output [B,C,H,W] (through its NHWC source when untouched), or a
    channel-padded NHWC tensor [B,H,W,Cp] when num_classes says how many channels are real"""
    B, H, W = labels.shape
    if outputs.shape[0] == B and tuple(outputs.shape[2:]) == (H, W) and num_classes in (None, outputs.shape[1]):
        x, inner, outer, cs, ps = _strided_source(outputs)
        return x, outputs.shape[1], inner, outer, cs, ps
    if num_classes is not None and tuple(outputs.shape[:3]) == (B, H, W) and outputs.shape[3] >= num_classes:
        x = outputs.detach().contiguous()
        return x, int(num_classes), B * H * W, 0, 1, x.shape[3]
    raise RuntimeError(f"semantic_eval: outputs {tuple(outputs.shape)} are neither [B,C,H,W] nor (with num_classes) a channel-padded "
                       f"[B,H,W,Cp] for labels {tuple(labels.shape)}")


def semantic_eval(outputs, labels, num_classes=None, ignore_index=-100, temperature=0.5, classes=False, confusion=None):
    """One sweep over the logits of a validation batch.  outputs: the module output [B,C,H,W] (fp32 or fp16; an untouched output is
    read through the NHWC tensor it was converted from) or a channel-padded NHWC tensor [B,H,W,Cp] with `num_classes` given;
    labels: int64 [B,H,W].  A pixel is void if its label is `ignore_index` or lies outside [0, C).  `confusion`: an int64 [C+1,C]
    tensor to add into (a new zeroed one otherwise).  classes=True also returns the class map and softmax(outputs / temperature) of
    it.  Never synchronises."""
    if not (torch.is_tensor(outputs) and torch.is_tensor(labels) and outputs.is_cuda and labels.is_cuda):
        raise RuntimeError("semantic_eval expects the outputs and the labels on the GPU (the HIP path has no CPU fallback)")
    if outputs.dim() != 4 or labels.dim() != 3 or labels.dtype != torch.int64:
        raise RuntimeError("semantic_eval expects outputs [B,C,H,W] and int64 labels [B,H,W]")
    if not temperature > 0:
        raise ValueError("temperature must be positive")
    B, H, W = labels.shape
    x, C, inner, outer, cs, ps = _source(outputs, labels, num_classes)
    lib = _lib.load()
    if B < 1 or H * W < 1 or lib.mu_sem_eval_supported(C) != 0:
        raise RuntimeError(f"maskunet_amd: semantic evaluation needs B >= 1, H*W >= 1 and 1 <= num_classes <= 4096, got {B}x{H}x{W}, {C}")
    dev = x.device
    labels = labels.contiguous()
    if confusion is None:
        confusion = torch.zeros((C + 1, C), dtype=torch.int64, device=dev)
    elif confusion.dtype != torch.int64 or tuple(confusion.shape) != (C + 1, C) or not confusion.is_cuda or not confusion.is_contiguous():
        raise RuntimeError(f"confusion must be a contiguous int64 [{C + 1},{C}] tensor on the GPU")
    img_counts = torch.empty((B, 3, C), dtype=torch.int32, device=dev)
    img_loss = torch.empty((B, 2), dtype=torch.float64, device=dev)
    cls = torch.empty((B, H, W), dtype=torch.int32, device=dev) if classes else None
    prob = torch.empty((B, H, W), dtype=torch.float32, device=dev) if classes else None
    nws = lib.mu_sem_eval_workspace_bytes(B, H * W, C)
    ws = workspace(nws, dev)
    call("mu_sem_eval", ptr(x), ptr(labels), B, H * W, C, inner, outer, cs, ps, int(ignore_index), 1.0 / float(temperature),
         ptr(img_counts), ptr(img_loss), ptr(confusion), ptr(cls), ptr(prob), ptr(ws), nws, dt(x), stream())
    return SemanticBatch(img_counts, img_loss, confusion, cls, prob)


@dataclass
class SemanticNativeBatch:
    """Device tensors of one semantic_eval_native call (contract: mu_sem_eval_native in include/maskunet_hip.h)."""
    img_counts: torch.Tensor             # int32 [B,3,C]  per image I_c, P_c, L_c at the image's own label size; zero for a refused image
    confusion: torch.Tensor              # int64 [C+1,C]  row = label (C: void), column = prediction; the tensor that was added into
    valid: torch.Tensor                  # uint8 [B]      0 for an image the kernel refused (size outside the bounds, short byte span)
    classes: torch.Tensor | None         # uint8, flat    the class maps, laid out like the labels' bytes (zero where nothing is written)
    offsets: torch.Tensor                # int64 [B+1]    of the labels: byte offset of every image in `classes`
    sizes: torch.Tensor                  # int32 [B,2]    (H_b, W_b)

    def class_maps(self):
        """The per-image [H_b, W_b] views of `classes` (no copy of the maps; None for a refused image).  Brings offsets, sizes and
        valid to the host: this SYNCHRONISES."""
        if self.classes is None:
            raise RuntimeError("SemanticNativeBatch.class_maps needs the class map: call semantic_eval_native / update_native with classes=True")
        off, sizes, ok = self.offsets.cpu().tolist(), self.sizes.cpu().tolist(), self.valid.cpu().tolist()
        return [self.classes[o:o + H * W].view(H, W) if v else None for o, (H, W), v in zip(off, sizes, ok)]


def _source_native(outputs, B, num_classes):
    """(C, h, w, nhwc) of the logits of semantic_eval_native, from the shapes alone: [B,C,h,w] when num_classes is None or equals
    shape[1] (tried first, as _source does), else a channel-padded [B,h,w,Cp] with num_classes real channels"""
    if outputs.shape[0] == B and num_classes in (None, outputs.shape[1]):
        return int(outputs.shape[1]), int(outputs.shape[2]), int(outputs.shape[3]), False
    if outputs.shape[0] == B and num_classes is not None and outputs.shape[3] >= num_classes:
        return int(num_classes), int(outputs.shape[1]), int(outputs.shape[2]), True
    raise RuntimeError(f"semantic_eval_native: outputs {tuple(outputs.shape)} are neither [B,C,h,w] nor (with num_classes) a channel-padded "
                       f"[B,h,w,Cp] for a batch of {B} label maps")


def semantic_eval_native(outputs, labels, num_classes=None, ignore_index=255, classes=False, confusion=None):
    """Semantic evaluation at the labels' own resolution, as ADE20K, Cityscapes and COCO define mIoU: the logits of every image are
    upsampled bilinearly (the formula of F.interpolate(.., mode="bilinear", align_corners=False)) to the size of that image's label map
    and the first arg-max is counted there, in one kernel that never writes the upsampled logits (mu_sem_eval_native).  outputs: the
    module output [B,C,h,w] (fp32 or fp16; an untouched output is read through the NHWC tensor it was converted from) or a
    channel-padded NHWC tensor [B,h,w,Cp] with `num_classes` given; labels: a PackedImages of B single-channel label maps of any sizes
    (pack_images, once per batch).  A pixel is void if its label is `ignore_index` or >= C.  `confusion`: an int64 [C+1,C] tensor to add
    into (a new zeroed one otherwise).  classes=True also returns the class maps at native resolution.  Never synchronises."""
    from .images import PackedImages
    if not torch.is_tensor(outputs) or outputs.dim() != 4 or not isinstance(labels, PackedImages):
        raise RuntimeError("semantic_eval_native expects outputs [B,C,h,w] (or [B,h,w,Cp] with num_classes) and the labels as a PackedImages")
    if labels.channels != 1:
        raise RuntimeError(f"semantic_eval_native: label maps have one channel, got a PackedImages of {labels.channels}")
    B = int(labels.sizes.shape[0])
    C, h, w, nhwc = _source_native(outputs, B, num_classes)
    lib = _lib.load()
    if B < 1 or lib.mu_sem_eval_native_supported(C, h, w) != 0:
        raise RuntimeError(f"maskunet_amd: native-resolution semantic evaluation needs B >= 1, 1 <= num_classes <= 256 and "
                           f"1 <= h * w <= 65536, got B = {B}, {C} classes, {h}x{w}")
    if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (C + 1, C) or not confusion.is_contiguous()):
        raise RuntimeError(f"confusion must be a contiguous int64 [{C + 1},{C}] tensor on the GPU")
    if not (outputs.is_cuda and labels.data.is_cuda and labels.offsets.is_cuda and labels.sizes.is_cuda
            and (confusion is None or confusion.is_cuda)):
        raise RuntimeError("semantic_eval_native expects the outputs and the labels on the GPU (the HIP path has no CPU fallback)")
    if nhwc:
        x = outputs.detach().contiguous()
        inner, outer, cs, ps = B * h * w, 0, 1, x.shape[3]
    else:
        x, inner, outer, cs, ps = _strided_source(outputs)
    dev = x.device
    if confusion is None:
        confusion = torch.zeros((C + 1, C), dtype=torch.int64, device=dev)
    img_counts = torch.empty((B, 3, C), dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    cls = torch.zeros_like(labels.data) if classes else None
    nws = lib.mu_sem_eval_native_workspace_bytes(B, C, h, w, labels.max_h, labels.max_w)
    ws = workspace(nws, dev)
    call("mu_sem_eval_native", ptr(x), B, C, h, w, inner, outer, cs, ps, ptr(labels.data), ptr(labels.offsets), ptr(labels.sizes),
         labels.max_h, labels.max_w, int(ignore_index), ptr(img_counts), ptr(confusion), ptr(valid), ptr(cls), ptr(ws), nws, dt(x), stream())
    return SemanticNativeBatch(img_counts, confusion, valid, cls, labels.offsets, labels.sizes)


def _ratio(num, den):
    """num / den in float64, 0 where den == 0 (sklearn's zero_division=0)"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape, np.float64), where=den != 0)


def _iou_mean(counts, smooth, empty):
    """mean over the classes with a non-empty union of (I + smooth) / (U + smooth), U = P + L - I; `empty` if there is none"""
    I, P, L = (np.asarray(c, np.float64) for c in counts)
    U = P + L - I
    seen = U > 0
    return float(np.mean((I[seen] + smooth) / (U[seen] + smooth))) if seen.any() else empty


def metrics_from_counts(confusion, per_update_img_counts, per_update_img_loss, smooth=1e-6):
    """All host arithmetic of SemanticMetrics.compute(), on numpy arrays: confusion int64 [C+1,C] (row C = void labels), and per
    update img_counts [B_i,3,C] and img_loss [B_i,2].  Returns a dict (float64 unless noted):
      confusion int64 [C+1,C]; tp, fp, fn, support int64 [C] over the non-void pixels; iou, precision, recall, f1 [C] (0 where the
      denominator is 0); present = tp + fp + fn > 0; miou, macro_precision, macro_recall, macro_f1: means over the present classes
      (sklearn's average="macro"); weighted_iou / _precision / _recall / _f1: weighted by support (average="weighted");
      pixel_accuracy = sum tp / non-void pixels; mean_accuracy = mean recall over the classes with support;
      reference = the numbers the scripts print: batch_miou (mean over the updates of mean_iou of that batch, city_panoptic.py:225-236),
      image_miou (mean over the images of compute_iou_for_image, :212-222; an image with no class is 1.0) and loss (mean over the
      updates of sum loss / sum count; NaN for an update without a counted pixel, as torch)."""
    conf = np.asarray(confusion).astype(np.int64)
    C = conf.shape[1]
    if conf.shape != (C + 1, C):
        raise ValueError(f"confusion must be [C+1,C], got {conf.shape}")
    real = conf[:C]
    tp = np.diag(real).copy()
    support = real.sum(axis=1)
    fp = real.sum(axis=0) - tp
    fn = support - tp
    present = (tp + fp + fn) > 0
    per_class = {"iou": _ratio(tp, tp + fp + fn), "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
                 "f1": _ratio(2 * tp, 2 * tp + fp + fn)}
    out = {"confusion": conf, "tp": tp, "fp": fp, "fn": fn, "support": support, "present": present, **per_class}
    n = int(support.sum())
    for name, v in per_class.items():
        out["miou" if name == "iou" else "macro_" + name] = float(v[present].mean()) if present.any() else 0.0
        out["weighted_" + name] = float(_ratio((v * support).sum(), n))
    out["pixel_accuracy"] = float(_ratio(tp.sum(), n))
    has = support > 0
    out["mean_accuracy"] = float(per_class["recall"][has].mean()) if has.any() else 0.0
    batch, image, loss = [], [], []
    for counts, ls in zip(per_update_img_counts, per_update_img_loss):
        counts, ls = np.asarray(counts).astype(np.int64), np.asarray(ls, np.float64)
        batch.append(_iou_mean(counts.sum(axis=0), smooth, float("nan")))
        image += [_iou_mean(c, smooth, 1.0) for c in counts]
        s, k = ls[:, 0].sum(), ls[:, 1].sum()
        loss.append(s / k if k > 0 else float("nan"))
    mean = lambda v: float(np.mean(v)) if len(v) else float("nan")
    out["reference"] = {"batch_miou": mean(batch), "image_miou": mean(image), "loss": mean(loss)}
    return out


class SemanticMetrics:
    """Accumulates semantic_eval over a validation set: `update(outputs, labels)` per batch, `compute()` at the end.  The confusion
    matrix is one device int64 tensor that every update adds into; the per-image tensors stay on the device until compute().  No
    update synchronises.  (Across ranks: all-reduce `confusion` and gather the per-image tensors; not done here.)
    `update_native(outputs, packed_labels)` feeds the same accumulator at the labels' own resolution (semantic_eval_native); one
    metrics object takes one kind of update only."""

    def __init__(self, num_classes, ignore_index=-100, temperature=0.5, smooth=1e-6):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("num_classes must be positive")
        self.ignore_index, self.temperature, self.smooth = int(ignore_index), float(temperature), float(smooth)
        self.confusion = None
        self._seen = []
        self._native = None              # True / False once an update has been taken

    def _begin(self, native, device):
        if self._native is not None and self._native != native:
            raise RuntimeError("SemanticMetrics takes one kind of update: update() and update_native() cannot be mixed (reset() first)")
        if self.confusion is None:
            self.confusion = torch.zeros((self.num_classes + 1, self.num_classes), dtype=torch.int64, device=device)

    def update(self, outputs, labels, classes=False):
        """One validation batch; returns its SemanticBatch (with the class map and probability when classes=True)."""
        self._begin(False, outputs.device)
        batch = semantic_eval(outputs, labels, self.num_classes, self.ignore_index, self.temperature, classes, self.confusion)
        self._seen.append((batch.img_counts, batch.img_loss))
        self._native = False
        return batch

    def update_native(self, outputs, labels, classes=False):
        """One validation batch at the labels' own resolution: labels is the PackedImages of the batch's label maps (pack_images once
        per batch).  Returns its SemanticNativeBatch (with the native-resolution class maps when classes=True).  An ignore_index
        outside [0, 255] means that no label value is void by itself."""
        self._begin(True, outputs.device)
        batch = semantic_eval_native(outputs, labels, self.num_classes, self.ignore_index, classes, self.confusion)
        self._seen.append((batch.img_counts, batch.valid))
        self._native = True
        return batch

    def reset(self):
        self.confusion = None
        self._seen = []
        self._native = None

    def compute(self):
        """metrics_from_counts of everything seen; the one place that copies to the host.  After update_native no loss is defined (the
        img_loss entries are zero, so reference["loss"] is NaN), the per-image numbers run over the images the kernel accepted, and
        `refused` counts the others."""
        if not self._seen:
            raise RuntimeError("compute() before any update()")
        conf = self.confusion.cpu().numpy()
        if not self._native:
            return metrics_from_counts(conf, [c.cpu().numpy() for c, _ in self._seen], [ls.cpu().numpy() for _, ls in self._seen], self.smooth)
        ok = [v.cpu().numpy() != 0 for _, v in self._seen]
        counts = [c.cpu().numpy()[k] for (c, _), k in zip(self._seen, ok)]
        out = metrics_from_counts(conf, counts, [np.zeros((len(c), 2)) for c in counts], self.smooth)
        out["refused"] = int(sum(int((~k).sum()) for k in ok))
        return out
