"""Scoring of `Instances` on the device: the second half of evaluate_instances / evaluate_panoptic_metrics.

The reference RLE-encodes every instance mask on the host, writes all of them to JSON and hands the files to pycocotools (mask IoU of
every detection / ground-truth pair per category, greedy matching at ten IoU thresholds) and to panopticapi (`pq_compute`: segments
match at IoU > 0.5) (ade_panoptic.py:520-586, city_instance.py:451-500).  Both rest on the intersection counts of two id maps, which
mu_instance_pairs tabulates in one pass; mu_instance_match does both matchings over that table, and the two accumulators below turn the
per-batch device results into AP and PQ at the end of an evaluation.  Nothing here needs RLE.

match_instances / InstanceAP give COCOeval's stats[0] on ground truth without crowd regions.  coco_match / CocoEval are COCOeval in full
over the same pair table (mu_coco_match): iscrowd, annotated areas, the area ranges, the maxDets ladder and all twelve stats
(coco_instance.py:361-367, ade_instance.py:441-447), and PanopticQuality takes either result.

The contract is restated from the published algorithms (COCOeval.evaluateImg / accumulate, maskUtils.iou,
panopticapi.evaluation.pq_compute_single_core); it is not pinned to the packages themselves.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream
from .instances import Instances


def _thresholds(iou_thresholds):
    t = np.linspace(0.5, 0.95, 10) if iou_thresholds is None else np.asarray(iou_thresholds, np.float64).reshape(-1)
    if t.size < 1 or t.size > 32 or not bool(((t > 0) & (t <= 1)).all()):
        raise ValueError("iou_thresholds: 1 to 32 values in (0, 1]")
    return np.ascontiguousarray(t, np.float64)


@dataclass
class Matches:
    """Device tensors of one match_instances call.  Row k of every [.., K] tensor is the detection `pred.order[b, k]`; rows that are not
    evaluated detections are zero."""
    det_valid: torch.Tensor      # int32 [B,K]    1 = an evaluated detection
    det_class: torch.Tensor      # int32 [B,K]
    det_score: torch.Tensor      # fp32  [B,K]
    det_gt: torch.Tensor         # int32 [B,T,K]  COCO: the matched ground-truth id per threshold, 0 = none
    det_iou: torch.Tensor        # fp64  [B,T,K]  and the IoU of that match
    gt_per_class: torch.Tensor   # int32 [B,num_classes]  ground truths that take part
    pq_gt: torch.Tensor          # int32 [B,K]    panoptic: the matched ground-truth id, 0 = none
    pq_iou: torch.Tensor         # fp64  [B,K]
    pq_fp: torch.Tensor          # int32 [B,K]    1 = an unmatched detection that counts as a false positive
    overflow: torch.Tensor       # int32 [B]      count > max_instances on either side: this image's results are unspecified
    pairs: torch.Tensor | None = None       # int32 [B,H*W,3]  (pred id, gt id, intersection) sorted by (pred id, gt id)
    n_pairs: torch.Tensor | None = None     # int32 [B]


def match_instances(pred, gt, num_classes, iou_thresholds=None, max_queries=None, max_dets=100):
    """COCO and panoptic matching of two `Instances` of equal [B,H,W] (any producer on either side).  The detections of an image are
    `pred.order[b, :max_queries]`; of each class the first `max_dets` are evaluated.  Classes 1..num_classes-1 take part, pixels of
    every other ground-truth instance are void.  Never synchronises."""
    if not isinstance(pred, Instances) or not isinstance(gt, Instances):
        raise TypeError("match_instances expects two Instances")
    if pred.ids.dim() != 3 or tuple(pred.ids.shape) != tuple(gt.ids.shape):
        raise RuntimeError(f"match_instances: pred and gt differ in [B,H,W]: {tuple(pred.ids.shape)} and {tuple(gt.ids.shape)}")
    if not pred.ids.is_cuda or pred.ids.device != gt.ids.device:
        raise RuntimeError("match_instances: both Instances must live on the same GPU (the HIP path has no CPU fallback)")
    thr = _thresholds(iou_thresholds)
    B, H, W = pred.ids.shape
    Mp, Mg = pred.table.shape[1], gt.table.shape[1]
    K = Mp if max_queries is None else min(int(max_queries), Mp)
    num_classes, max_dets, T = int(num_classes), int(max_dets), int(thr.size)
    lib = _lib.load()
    if lib.mu_instance_match_supported(H, W, Mp, Mg, num_classes, K, max_dets, T) != 0:
        raise RuntimeError("maskunet_amd: instance matching needs H*W <= 65536, 1 <= max_instances <= 4096 on both sides, "
                           "1 <= num_classes <= 1024, max_queries >= 1, max_dets >= 1, 1 to 32 thresholds; got "
                           f"{H}x{W}, {Mp} / {Mg}, {num_classes} classes, max_queries={max_queries}, max_dets={max_dets}, {T}")
    dev = pred.ids.device
    i32 = dict(dtype=torch.int32, device=dev)
    pairs = torch.empty((B, H * W, 3), **i32)
    n_pairs = torch.empty(B, **i32)
    ws = torch.empty(max(lib.mu_instance_pairs_workspace_bytes(B, H, W, Mp, Mg), lib.mu_instance_match_workspace_bytes(B, K)),
                     dtype=torch.uint8, device=dev)
    m = Matches(torch.empty((B, K), **i32), torch.empty((B, K), **i32), torch.empty((B, K), dtype=torch.float32, device=dev),
                torch.empty((B, T, K), **i32), torch.empty((B, T, K), dtype=torch.float64, device=dev),
                torch.empty((B, num_classes), **i32), torch.empty((B, K), **i32), torch.empty((B, K), dtype=torch.float64, device=dev),
                torch.empty((B, K), **i32), torch.empty(B, **i32), pairs, n_pairs)
    tensors = [pred.ids, gt.ids, pred.table, pred.scores, pred.order, pred.count, gt.table, gt.count]
    p_ids, g_ids, p_table, p_score, p_order, p_count, g_table, g_count = [t.contiguous() for t in tensors]
    call("mu_instance_pairs", ptr(p_ids), ptr(g_ids), B, H, W, Mp, Mg, ptr(pairs), ptr(n_pairs), ptr(ws), ws.numel(), stream())
    call("mu_instance_match", ptr(pairs), ptr(n_pairs), ptr(p_table), ptr(p_score), ptr(p_order), ptr(p_count), ptr(g_table),
         ptr(g_count), B, H, W, Mp, Mg, num_classes, K, max_dets, thr.ctypes.data_as(ctypes.c_void_p), T, ptr(m.det_valid),
         ptr(m.det_class), ptr(m.det_score), ptr(m.det_gt), ptr(m.det_iou), ptr(m.gt_per_class), ptr(m.pq_gt), ptr(m.pq_iou),
         ptr(m.pq_fp), ptr(m.overflow), ptr(ws), ws.numel(), stream())
    return m


COCO_AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
COCO_AREA_LABELS = ("all", "small", "medium", "large")


def _area_ranges(area_ranges):
    a = np.asarray(COCO_AREA_RANGES if area_ranges is None else area_ranges, np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= 4 or not bool((a[:, 0] <= a[:, 1]).all()):
        raise ValueError("area_ranges: 1 to 4 pairs [lo, hi] with lo <= hi")
    return np.ascontiguousarray(a)


def _max_dets(max_dets):
    m = [int(v) for v in np.asarray(max_dets).reshape(-1)]
    if not m or m[0] < 1 or any(b <= a for a, b in zip(m, m[1:])):
        raise ValueError("max_dets: positive and ascending, COCO's is (1, 10, 100)")
    return tuple(m)


@dataclass
class CocoMatches:
    """Device tensors of one coco_match call.  Rows as in `Matches`; A = area ranges, T = thresholds."""
    det_valid: torch.Tensor        # int32 [B,K]      1 = an evaluated detection
    det_class: torch.Tensor        # int32 [B,K]
    det_rank: torch.Tensor         # int32 [B,K]      its rank among the evaluated rows of its class in the image, from 0
    det_score: torch.Tensor        # fp32  [B,K]
    det_gt: torch.Tensor           # int32 [B,A,T,K]  COCO: the matched ground-truth id, 0 = none
    det_iou: torch.Tensor          # fp64  [B,A,T,K]
    det_ignore: torch.Tensor       # uint8 [B,A,T,K]  COCOeval's dtIg
    gt_counted: torch.Tensor       # int32 [B,A,num_classes]  non-ignored ground truths (npig)
    pq_gt_per_class: torch.Tensor  # int32 [B,num_classes]    ground truths that take part and are not crowd
    pq_gt: torch.Tensor            # int32 [B,K]
    pq_iou: torch.Tensor           # fp64  [B,K]
    pq_fp: torch.Tensor            # int32 [B,K]
    overflow: torch.Tensor         # int32 [B]
    pairs: torch.Tensor | None = None
    n_pairs: torch.Tensor | None = None


def coco_match(pred, gt, num_classes, crowd=None, gt_area=None, iou_thresholds=None, area_ranges=None, max_queries=None,
               max_dets=(1, 10, 100)):
    """COCOeval.evaluateImg in full, and panopticapi's matching with its crowd rules, of two `Instances` of equal [B,H,W].  `crowd`
    (bool or int [B, gt.table.shape[1]]; row g-1 belongs to ground-truth id g) marks iscrowd ground truths, `gt_area` (floating, same
    shape) replaces their pixel area in the area-range test only (COCO's annotated `area` is measured at the original image size).
    Defaults are COCO's ten thresholds, four area ranges and maxDets ladder; the largest of `max_dets` is the per-(image, class) cut,
    `CocoEval` applies the smaller ones through `det_rank`.  Never synchronises."""
    if not isinstance(pred, Instances) or not isinstance(gt, Instances):
        raise TypeError("coco_match expects two Instances")
    if pred.ids.dim() != 3 or tuple(pred.ids.shape) != tuple(gt.ids.shape):
        raise RuntimeError(f"coco_match: pred and gt differ in [B,H,W]: {tuple(pred.ids.shape)} and {tuple(gt.ids.shape)}")
    if not pred.ids.is_cuda or pred.ids.device != gt.ids.device:
        raise RuntimeError("coco_match: both Instances must live on the same GPU (the HIP path has no CPU fallback)")
    thr, rng, ladder = _thresholds(iou_thresholds), _area_ranges(area_ranges), _max_dets(max_dets)
    B, H, W = pred.ids.shape
    Mp, Mg = pred.table.shape[1], gt.table.shape[1]
    dev = pred.ids.device
    for name, t in (("crowd", crowd), ("gt_area", gt_area)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, Mg):
            raise RuntimeError(f"coco_match: {name} must be a tensor of shape [B, gt.table.shape[1]] = {(B, Mg)}")
        if t.device != dev:
            raise RuntimeError(f"coco_match: {name} must live on the GPU of the Instances (the HIP path has no CPU fallback)")
    if crowd is not None and (crowd.is_floating_point() or crowd.is_complex()):
        raise TypeError("coco_match: crowd must be bool or integer")
    if gt_area is not None and not gt_area.is_floating_point():
        raise TypeError("coco_match: gt_area must be floating point")
    K = Mp if max_queries is None else min(int(max_queries), Mp)
    num_classes, T, A = int(num_classes), int(thr.size), int(rng.shape[0])
    lib = _lib.load()
    if lib.mu_coco_match_supported(H, W, Mp, Mg, num_classes, K, ladder[-1], T, A) != 0:
        raise RuntimeError("maskunet_amd: coco_match needs H*W <= 65536, 1 <= max_instances <= 4096 on both sides, "
                           "1 <= num_classes <= 1024, max_queries >= 1, 1 to 32 thresholds, 1 to 4 area ranges; got "
                           f"{H}x{W}, {Mp} / {Mg}, {num_classes} classes, max_queries={max_queries}, {T}, {A}")
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    pairs = torch.empty((B, H * W, 3), **i32)
    n_pairs = torch.empty(B, **i32)
    ws = torch.empty(max(lib.mu_instance_pairs_workspace_bytes(B, H, W, Mp, Mg), lib.mu_coco_match_workspace_bytes(B, K)),
                     dtype=torch.uint8, device=dev)
    m = CocoMatches(torch.empty((B, K), **i32), torch.empty((B, K), **i32), torch.empty((B, K), **i32),
                    torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, A, T, K), **i32),
                    torch.empty((B, A, T, K), **f64), torch.empty((B, A, T, K), dtype=torch.uint8, device=dev),
                    torch.empty((B, A, num_classes), **i32), torch.empty((B, num_classes), **i32), torch.empty((B, K), **i32),
                    torch.empty((B, K), **f64), torch.empty((B, K), **i32), torch.empty(B, **i32), pairs, n_pairs)
    tensors = [pred.ids, gt.ids, pred.table, pred.scores, pred.order, pred.count, gt.table, gt.count]
    p_ids, g_ids, p_table, p_score, p_order, p_count, g_table, g_count = [t.contiguous() for t in tensors]
    g_crowd = None if crowd is None else (crowd != 0).to(torch.int32).contiguous()
    g_area = None if gt_area is None else gt_area.to(torch.float64).contiguous()
    call("mu_instance_pairs", ptr(p_ids), ptr(g_ids), B, H, W, Mp, Mg, ptr(pairs), ptr(n_pairs), ptr(ws), ws.numel(), stream())
    call("mu_coco_match", ptr(pairs), ptr(n_pairs), ptr(p_table), ptr(p_score), ptr(p_order), ptr(p_count), ptr(g_table), ptr(g_count),
         None if g_crowd is None else ptr(g_crowd), None if g_area is None else ptr(g_area), B, H, W, Mp, Mg, num_classes, K,
         ladder[-1], thr.ctypes.data_as(ctypes.c_void_p), T, rng.ctypes.data_as(ctypes.c_void_p), A, ptr(m.det_valid),
         ptr(m.det_class), ptr(m.det_rank), ptr(m.det_score), ptr(m.det_gt), ptr(m.det_iou), ptr(m.det_ignore), ptr(m.gt_counted),
         ptr(m.pq_gt_per_class), ptr(m.pq_gt), ptr(m.pq_iou), ptr(m.pq_fp), ptr(m.overflow), ptr(ws), ws.numel(), stream())
    return m


class _Accumulator:
    _fields = ()                    # the last one is the per-class ground-truth count

    def __init__(self, num_classes):
        self.num_classes = int(num_classes)
        if self.num_classes < 1:
            raise ValueError("num_classes must be positive")
        self._seen = []

    def _names(self, matches):
        if isinstance(matches, CocoMatches):
            raise TypeError(f"{type(self).__name__}.update expects the Matches of match_instances; CocoEval takes a CocoMatches")
        return self._fields

    def update(self, matches):
        """Keeps the tensors of `matches` it needs where they are; no copy to the host, no synchronisation."""
        names = self._names(matches)
        made_for = getattr(matches, names[-1]).shape[-1]
        if made_for != self.num_classes:
            raise ValueError(f"matches were made for {made_for} classes, not {self.num_classes}")
        self._check(matches)
        self._seen.append(tuple(getattr(matches, f) for f in ("overflow",) + names))

    def _check(self, matches):
        pass

    def reset(self):
        self._seen = []

    def _host(self):
        """everything seen, on the host: one array per field, images of all updates in update order"""
        if not self._seen:
            raise RuntimeError("compute() before any update()")
        rows = [[t.detach().cpu().numpy() for t in s] for s in self._seen]
        if any(bool(r[0].any()) for r in rows):
            raise RuntimeError("an image has more instances than max_instances (Matches.overflow): its matching is unspecified; "
                               "raise max_instances of the Instances producers")
        return rows


class InstanceAP(_Accumulator):
    """COCOeval.accumulate over everything seen, area range `all`, one maxDets (the `max_dets` the matches were made with):
    `compute()` -> {"precision": float64 [T,101,num_classes] (-1 for classes without ground truth), "ap": the mean of the entries
    > -1 (COCOeval's stats[0]; -1 if there are none)}."""
    _fields = ("det_valid", "det_class", "det_score", "det_gt", "gt_per_class")

    def __init__(self, num_classes, iou_thresholds=None):
        super().__init__(num_classes)
        self.iou_thresholds = _thresholds(iou_thresholds)

    def _check(self, matches):
        if matches.det_gt.shape[1] != self.iou_thresholds.size:
            raise ValueError(f"matches hold {matches.det_gt.shape[1]} thresholds, not {self.iou_thresholds.size}")

    def compute(self):
        rows = self._host()
        T, C = self.iou_thresholds.size, self.num_classes
        valid = np.concatenate([r[1].reshape(-1) for r in rows]) != 0
        cls = np.concatenate([r[2].reshape(-1) for r in rows])[valid]
        score = np.concatenate([r[3].reshape(-1) for r in rows]).astype(np.float64)[valid]
        hit = np.concatenate([r[4].transpose(1, 0, 2).reshape(T, -1) for r in rows], 1)[:, valid] > 0
        npig = np.concatenate([r[5] for r in rows], 0).astype(np.int64).sum(0)
        rec_thr = np.linspace(0.0, 1.0, 101)
        precision = -np.ones((T, 101, C))
        for c in range(C):
            if npig[c] == 0:
                continue
            sel = np.flatnonzero(cls == c)
            sel = sel[np.argsort(-score[sel], kind="mergesort")]
            tp_sum = np.cumsum(hit[:, sel], axis=1).astype(np.float64)
            fp_sum = np.cumsum(~hit[:, sel], axis=1).astype(np.float64)
            for t in range(T):
                tp, fp = tp_sum[t], fp_sum[t]
                rc = tp / npig[c]
                pr = (tp / (fp + tp + np.spacing(1))).tolist()
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                q = np.zeros(101)
                inds = np.searchsorted(rc, rec_thr, side="left")
                for ri, pi in enumerate(inds):
                    if pi < len(pr):
                        q[ri] = pr[pi]
                precision[t, :, c] = q
        kept = precision[precision > -1]
        return {"precision": precision, "ap": float(np.mean(kept)) if kept.size else -1.0}


class PanopticQuality(_Accumulator):
    """panopticapi's PQStat over everything seen.  `compute()` -> {"tp", "fp", "fn" (int64 [num_classes]), "iou_sum", "pq", "sq", "rq"
    (float64 [num_classes]; 0 where undefined), "All": {"pq", "sq", "rq", "n"}} plus "Things" and "Stuff" when `things` (one boolean
    per class) was given.  The means run over the classes with tp + fp + fn > 0.  iou_sum is the exactly rounded sum of the matched IoUs
    (math.fsum), so it does not depend on any order."""
    _fields = ("det_valid", "det_class", "pq_gt", "pq_iou", "pq_fp", "gt_per_class")

    def __init__(self, num_classes, things=None):
        super().__init__(num_classes)
        self.things = None if things is None else np.asarray(things, bool).reshape(-1)
        if self.things is not None and self.things.size != self.num_classes:
            raise ValueError("things: one boolean per class")

    def _names(self, matches):
        """a CocoMatches brings the crowd-aware panoptic matching: its count of ground truths leaves the crowd ones out"""
        if isinstance(matches, CocoMatches):
            return self._fields[:-1] + ("pq_gt_per_class",)
        return super()._names(matches)

    def compute(self):
        rows = self._host()
        C = self.num_classes
        valid = np.concatenate([r[1].reshape(-1) for r in rows]) != 0
        cls = np.concatenate([r[2].reshape(-1) for r in rows])[valid]
        m_gt = np.concatenate([r[3].reshape(-1) for r in rows])[valid]
        m_iou = np.concatenate([r[4].reshape(-1) for r in rows])[valid]
        m_fp = np.concatenate([r[5].reshape(-1) for r in rows])[valid]
        n_gt = np.concatenate([r[6] for r in rows], 0).astype(np.int64).sum(0)
        tp = np.bincount(cls[m_gt > 0], minlength=C).astype(np.int64)
        fp = np.bincount(cls[m_fp != 0], minlength=C).astype(np.int64)
        fn = n_gt - tp
        iou_sum = np.array([math.fsum(m_iou[(cls == c) & (m_gt > 0)].tolist()) for c in range(C)])
        den = tp + 0.5 * fp + 0.5 * fn
        seen = (tp + fp + fn) > 0
        pq = np.where(seen, iou_sum / np.where(seen, den, 1.0), 0.0)
        sq = np.where(tp > 0, iou_sum / np.where(tp > 0, tp, 1), 0.0)
        rq = np.where(seen, tp / np.where(seen, den, 1.0), 0.0)
        out = {"tp": tp, "fp": fp, "fn": fn, "iou_sum": iou_sum, "pq": pq, "sq": sq, "rq": rq}

        def mean(sel):
            n = int(sel.sum())
            return {"pq": float(pq[sel].sum() / n) if n else 0.0, "sq": float(sq[sel].sum() / n) if n else 0.0,
                    "rq": float(rq[sel].sum() / n) if n else 0.0, "n": n}

        out["All"] = mean(seen)
        if self.things is not None:
            out["Things"] = mean(seen & self.things)
            out["Stuff"] = mean(seen & ~self.things)
        return out


class CocoEval(_Accumulator):
    """COCOeval.accumulate and the arithmetic of summarize over everything seen, on the host in fp64.  `compute()` ->
    {"precision": [T,101,C,A,M], "recall": [T,C,A,M] (-1 where a class has no non-ignored ground truth), "stats": float64 [12]} in
    COCOeval's order: AP, AP50, AP75, APs, APm, APl at the largest maxDet, AR at max_dets[0], [1], [2], ARs, ARm, ARl at the largest.
    The area ranges are taken by position (all, small, medium, large); an entry whose range or maxDet is not configured is NaN.  AP50 /
    AP75 pick the threshold that equals 0.5 / 0.75 exactly and are -1 without one, which is what pycocotools prints.  The matches must
    have been made with the same thresholds and ranges and with a `max_dets` whose largest is this one's."""
    _fields = ("det_valid", "det_class", "det_rank", "det_score", "det_gt", "det_ignore", "gt_counted")

    def __init__(self, num_classes, iou_thresholds=None, area_ranges=None, max_dets=(1, 10, 100)):
        super().__init__(num_classes)
        self.iou_thresholds = _thresholds(iou_thresholds)
        self.area_ranges = _area_ranges(area_ranges)
        self.max_dets = _max_dets(max_dets)

    def _names(self, matches):
        if not isinstance(matches, CocoMatches):
            raise TypeError("CocoEval.update expects the CocoMatches of coco_match")
        return self._fields

    def _check(self, matches):
        want = (self.area_ranges.shape[0], self.iou_thresholds.size)
        if tuple(matches.det_gt.shape[1:3]) != want:
            raise ValueError(f"matches hold {tuple(matches.det_gt.shape[1:3])} (area ranges, thresholds), not {want}")

    def compute(self):
        rows = self._host()
        T, C, A, M = self.iou_thresholds.size, self.num_classes, self.area_ranges.shape[0], len(self.max_dets)
        valid = np.concatenate([r[1].reshape(-1) for r in rows]) != 0
        cls = np.concatenate([r[2].reshape(-1) for r in rows])[valid]
        rank = np.concatenate([r[3].reshape(-1) for r in rows])[valid]
        score = np.concatenate([r[4].reshape(-1) for r in rows]).astype(np.float64)[valid]
        hit = np.concatenate([r[5].transpose(1, 2, 0, 3).reshape(A, T, -1) for r in rows], 2)[:, :, valid] > 0
        ign = np.concatenate([r[6].transpose(1, 2, 0, 3).reshape(A, T, -1) for r in rows], 2)[:, :, valid] != 0
        npig = np.concatenate([r[7] for r in rows], 0).astype(np.int64).sum(0)          # [A,C]
        rec_thr = np.linspace(0.0, 1.0, 101)
        precision = -np.ones((T, 101, C, A, M))
        recall = -np.ones((T, C, A, M))
        for c in range(C):
            of_class = np.flatnonzero(cls == c)
            of_class = of_class[np.argsort(-score[of_class], kind="mergesort")]
            for a in range(A):
                if npig[a, c] == 0:
                    continue
                for m, max_det in enumerate(self.max_dets):
                    sel = of_class[rank[of_class] < max_det]
                    if sel.size == 0:
                        precision[:, :, c, a, m] = 0.0
                        recall[:, c, a, m] = 0.0
                        continue
                    tps = hit[a][:, sel] & ~ign[a][:, sel]
                    fps = ~hit[a][:, sel] & ~ign[a][:, sel]
                    tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                    for t in range(T):
                        tp, fp = tp_sum[t], fp_sum[t]
                        rc = tp / npig[a, c]
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, c, a, m] = rc[-1]
                        pr = np.maximum.accumulate(pr[::-1])[::-1]                      # the envelope: pr[i - 1] = max(pr[i - 1], pr[i])
                        inds = np.searchsorted(rc, rec_thr, side="left")
                        precision[t, :, c, a, m] = np.where(inds < pr.size, pr[np.minimum(inds, pr.size - 1)], 0.0)
        out = {"precision": precision, "recall": recall, "stats": np.array([self._stat(precision, recall, *e) for e in self._entries()])}
        return out

    def _entries(self):
        """(is AP, IoU threshold or None, area index, maxDets index or None = not configured) of the twelve stats"""
        A, M = self.area_ranges.shape[0], len(self.max_dets)
        last = M - 1
        area = lambda i: i if i < A else None
        ladder = lambda j: j if j < M else None
        return [(True, None, 0, last), (True, 0.5, 0, last), (True, 0.75, 0, last), (True, None, area(1), last),
                (True, None, area(2), last), (True, None, area(3), last), (False, None, 0, ladder(0)), (False, None, 0, ladder(1)),
                (False, None, 0, ladder(2)), (False, None, area(1), last), (False, None, area(2), last), (False, None, area(3), last)]

    def _stat(self, precision, recall, is_ap, iou, a, m):
        if a is None or m is None:
            return float("nan")
        s = precision[:, :, :, a, m] if is_ap else recall[:, :, a, m]
        if iou is not None:
            s = s[np.flatnonzero(self.iou_thresholds == iou)]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def summarize(self):
        """The lines COCOeval.summarize prints, as a list of strings (the entries that are not configured are left out)."""
        stats = self.compute()["stats"]
        span = f"{self.iou_thresholds[0]:0.2f}:{self.iou_thresholds[-1]:0.2f}"
        lines = []
        for value, (is_ap, iou, a, m) in zip(stats, self._entries()):
            if a is None or m is None:
                continue
            title, kind = ("Average Precision", "(AP)") if is_ap else ("Average Recall", "(AR)")
            iou_str = span if iou is None else f"{iou:0.2f}"
            lines.append(f" {title:<18} {kind} @[ IoU={iou_str:<9} | area={COCO_AREA_LABELS[a]:>6s} | maxDets={self.max_dets[m]:>3d} ] "
                         f"= {value:0.3f}")
        return lines
