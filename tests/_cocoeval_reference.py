"""CPU restatement of the full COCO / panoptic evaluation contract (maskunet_amd.coco_match, CocoEval, PanopticQuality on a
CocoMatches), deliberately naive: dense boolean masks, lists of dicts, Python loops, its own sort of the ground truths.  It has no pair
table and shares nothing with maskunet_amd/matching.py, so that the two can disagree.  Restated from the published algorithms --
COCOeval.evaluateImg / accumulate / summarize and panopticapi's pq_compute_single_core with its crowd handling -- not from the kernel.

A "side" is the dict of numpy arrays of tests/_match_reference.py (ids [B,H,W], count [B], table [B,M,8], score, order); `crowd`
[B,M] (non-zero = iscrowd) and `gt_area` [B,M] (the area of the range test) are indexed by ground-truth id - 1, None = no crowd / the
pixel area.

Besides the results every evaluation returns event counters, so that a test can tell whether its inputs reached a branch at all:
  crowd_rematched   detections matched to a crowd ground truth that another detection had already matched
  break_hid_better  stops under "non-ignored before ignored" where a later ignored ground truth had the larger IoU
  matched_ignored   matched detections that are ignored (their ground truth is)
  unmatched_by_area unmatched detections ignored because their own area is outside the range
  crowd_saved       panoptic: unmatched detections that are no false positive only because of their overlap with the crowd region
"""
import numpy as np

COUNTERS = ("crowd_rematched", "break_hid_better", "matched_ignored", "unmatched_by_area", "crowd_saved")
COCO_THRESHOLDS = np.linspace(0.5, 0.95, 10)
REF_THRESHOLDS = np.linspace(0.30, 0.95, 10)              # the reference scripts' ladder
COCO_AREA_RANGES = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
SMALL_AREA_RANGES = [[0, 1e10], [0, 4], [4, 9], [9, 1e10]]       # the same four, scaled to images of a few hundred pixels


def lists_of_image(pred, gt, b, num_classes, crowd=None, gt_area=None, max_queries=None):
    """dets: one entry per row of order[b, :max_queries] -- None or {"mask", "category_id", "score"}; gts: the ground truths that take
    part, {"id", "mask", "category_id", "iscrowd", "area"}; void: the pixels of no such ground truth."""
    Mp, Mg = pred["table"].shape[1], gt["table"].shape[1]
    K = Mp if max_queries is None else min(max_queries, Mp)
    dets = []
    for p in pred["order"][b, :K].tolist():
        c = int(pred["table"][b, p - 1, 0]) if 1 <= p <= min(int(pred["count"][b]), Mp) else 0
        dets.append({"mask": pred["ids"][b] == p, "category_id": c, "score": np.float32(pred["score"][b, p - 1])}
                    if 1 <= c < num_classes else None)
    gts = []
    void = np.ones(gt["ids"][b].shape, bool)
    for g in range(1, min(int(gt["count"][b]), Mg) + 1):
        c = int(gt["table"][b, g - 1, 0])
        if not 1 <= c < num_classes:
            continue
        mask = gt["ids"][b] == g
        gts.append({"id": g, "mask": mask, "category_id": c, "iscrowd": bool(crowd is not None and crowd[b, g - 1] != 0),
                    "area": float(mask.sum()) if gt_area is None else float(gt_area[b, g - 1])})
        void &= ~mask
    return dets, gts, void


def evaluate_image(dets, gts, void, num_classes, thresholds, area_ranges, max_det):
    """COCOeval.evaluateImg for every class and area range of one image, and the panoptic matching.  Returns (arrays, counters)."""
    K, T, A = len(dets), len(thresholds), len(area_ranges)
    out = {"det_valid": np.zeros(K, np.int32), "det_class": np.zeros(K, np.int32), "det_rank": np.zeros(K, np.int32),
           "det_score": np.zeros(K, np.float32), "det_gt": np.zeros((A, T, K), np.int32), "det_iou": np.zeros((A, T, K), np.float64),
           "det_ignore": np.zeros((A, T, K), np.uint8), "gt_counted": np.zeros((A, num_classes), np.int32),
           "pq_gt_per_class": np.zeros(num_classes, np.int32), "pq_gt": np.zeros(K, np.int32), "pq_iou": np.zeros(K, np.float64),
           "pq_fp": np.zeros(K, np.int32)}
    cnt = dict.fromkeys(COUNTERS, 0)
    for c in range(1, num_classes):
        rows = [k for k, d in enumerate(dets) if d is not None and d["category_id"] == c][:max_det]
        gt_c = [g for g in gts if g["category_id"] == c]
        for r, k in enumerate(rows):
            out["det_valid"][k], out["det_class"][k], out["det_rank"][k], out["det_score"][k] = 1, c, r, dets[k]["score"]
        d_area = [int(dets[k]["mask"].sum()) for k in rows]
        # maskUtils.iou with the iscrowd flags: against a crowd region the union is the detection's own area
        ious = [[0.0] * len(gt_c) for _ in rows]
        for r, k in enumerate(rows):
            for j, g in enumerate(gt_c):
                inter = int((dets[k]["mask"] & g["mask"]).sum())
                union = d_area[r] if g["iscrowd"] else d_area[r] + int(g["mask"].sum()) - inter
                ious[r][j] = float(inter) / float(union)
        for ai, (lo, hi) in enumerate(area_ranges):
            for g in gt_c:
                g["_ignore"] = 1 if (g["iscrowd"] or g["area"] < lo or g["area"] > hi) else 0
            gtind = sorted(range(len(gt_c)), key=lambda j: gt_c[j]["_ignore"])           # stable: non-ignored first
            gs = [gt_c[j] for j in gtind]
            out["gt_counted"][ai, c] = sum(1 for g in gs if not g["_ignore"])
            for ti, t in enumerate(thresholds):
                gtm = [0] * len(gs)
                for r, k in enumerate(rows):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gs):
                        if gtm[gind] > 0 and not g["iscrowd"]:
                            continue
                        if m > -1 and gs[m]["_ignore"] == 0 and g["_ignore"] == 1:
                            rest = [ious[r][gtind[x]] for x in range(gind, len(gs)) if not (gtm[x] > 0 and not gs[x]["iscrowd"])]
                            cnt["break_hid_better"] += bool(rest and max(rest) > iou)
                            break
                        if ious[r][gtind[gind]] < iou:
                            continue
                        iou = ious[r][gtind[gind]]
                        m = gind
                    if m == -1:
                        outside = d_area[r] < lo or d_area[r] > hi
                        out["det_ignore"][ai, ti, k] = outside
                        cnt["unmatched_by_area"] += bool(outside)
                        continue
                    cnt["crowd_rematched"] += bool(gtm[m] > 0)
                    cnt["matched_ignored"] += gs[m]["_ignore"]
                    gtm[m] = 1
                    out["det_gt"][ai, ti, k] = gs[m]["id"]
                    out["det_iou"][ai, ti, k] = iou
                    out["det_ignore"][ai, ti, k] = gs[m]["_ignore"]
        # panopticapi: pq_compute_single_core
        crowd_of_class = None
        for g in gt_c:
            if g["iscrowd"]:
                crowd_of_class = g                       # crowd_labels_dict keeps the last one per category
            else:
                out["pq_gt_per_class"][c] += 1
        for r, k in enumerate(rows):
            v = int((dets[k]["mask"] & void).sum())
            for g in gt_c:
                if g["iscrowd"]:
                    continue
                inter = int((dets[k]["mask"] & g["mask"]).sum())
                if inter == 0:
                    continue
                union = d_area[r] + int(g["mask"].sum()) - inter - v
                iou = inter / union
                if iou > 0.5:
                    assert out["pq_gt"][k] == 0, "at most one match per segment"
                    out["pq_gt"][k] = g["id"]
                    out["pq_iou"][k] = iou
            if out["pq_gt"][k] == 0:
                inter = v
                if crowd_of_class is not None:
                    inter += int((dets[k]["mask"] & crowd_of_class["mask"]).sum())
                if inter / d_area[r] > 0.5:
                    cnt["crowd_saved"] += not v / d_area[r] > 0.5
                else:
                    out["pq_fp"][k] = 1
    return out, cnt


def evaluate(pred, gt, num_classes, crowd=None, gt_area=None, thresholds=None, area_ranges=None, max_queries=None, max_dets=(1, 10, 100)):
    """All images of two sides: arrays with a leading batch axis plus overflow, and the counters summed."""
    thresholds = COCO_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64)
    area_ranges = COCO_AREA_RANGES if area_ranges is None else area_ranges
    per, total = [], dict.fromkeys(COUNTERS, 0)
    for b in range(pred["ids"].shape[0]):
        dets, gts, void = lists_of_image(pred, gt, b, num_classes, crowd, gt_area, max_queries)
        res, cnt = evaluate_image(dets, gts, void, num_classes, thresholds, area_ranges, max(max_dets))
        per.append(res)
        for k in COUNTERS:
            total[k] += int(cnt[k])
    out = {k: np.stack([p[k] for p in per]) for k in per[0]}
    out["overflow"] = ((pred["count"] > pred["table"].shape[1]) | (gt["count"] > gt["table"].shape[1])).astype(np.int32)
    return out, total


def accumulate(results, num_classes, thresholds=None, area_ranges=None, max_dets=(1, 10, 100)):
    """COCOeval.accumulate over a list of evaluate() results: precision [T,101,C,A,M], recall [T,C,A,M]."""
    thresholds = COCO_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64)
    T, A, M = len(thresholds), len(COCO_AREA_RANGES if area_ranges is None else area_ranges), len(max_dets)
    rec_thrs = np.linspace(.0, 1.00, 101)
    precision = -np.ones((T, 101, num_classes, A, M))
    recall = -np.ones((T, num_classes, A, M))
    for c in range(num_classes):
        for a in range(A):
            for mi, max_det in enumerate(max_dets):
                scores, dtm, dt_ig, npig = [], [[] for _ in range(T)], [[] for _ in range(T)], 0
                for r in results:
                    for b in range(r["det_valid"].shape[0]):
                        npig += int(r["gt_counted"][b, a, c])
                        for k in range(r["det_valid"].shape[1]):
                            if r["det_valid"][b, k] and r["det_class"][b, k] == c and r["det_rank"][b, k] < max_det:
                                scores.append(float(r["det_score"][b, k]))
                                for t in range(T):
                                    dtm[t].append(int(r["det_gt"][b, a, t, k]))
                                    dt_ig[t].append(int(r["det_ignore"][b, a, t, k]))
                if npig == 0:
                    continue
                inds = np.argsort(-np.asarray(scores, np.float64), kind="mergesort")
                for t in range(T):
                    m = np.asarray(dtm[t], np.int64)[inds]
                    ig = np.asarray(dt_ig[t], np.int64)[inds] != 0
                    tp = np.cumsum(np.logical_and(m > 0, np.logical_not(ig))).astype(dtype=float)
                    fp = np.cumsum(np.logical_and(m == 0, np.logical_not(ig))).astype(dtype=float)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((101,)).tolist()
                    recall[t, c, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    ri_inds = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(ri_inds):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, c, a, mi] = np.array(q)
    return {"precision": precision, "recall": recall}


def summarize(acc, thresholds=None, max_dets=(1, 10, 100)):
    """COCOeval.summarize's twelve numbers from accumulate()'s arrays (four area ranges, three maxDets)."""
    thresholds = COCO_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64)

    def one(ap, iou_thr=None, area=0, mi=len(max_dets) - 1):
        s = acc["precision"] if ap else acc["recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == thresholds)[0]]
        s = s[:, :, :, area, mi] if ap else s[:, :, area, mi]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    return np.array([one(1), one(1, .5), one(1, .75), one(1, area=1), one(1, area=2), one(1, area=3), one(0, mi=0), one(0, mi=1),
                     one(0, mi=2), one(0, area=1), one(0, area=2), one(0, area=3)])


def accumulate_pq(results, num_classes):
    """panopticapi's PQStat over evaluate() results -> per-class tp / fp / fn / iou and the mean over the classes seen ("All")."""
    tp, fp, fn, iou = [0] * num_classes, [0] * num_classes, [0] * num_classes, [0.0] * num_classes
    for r in results:
        for b in range(r["det_valid"].shape[0]):
            hit = [0] * num_classes
            for k in range(r["det_valid"].shape[1]):
                if not r["det_valid"][b, k]:
                    continue
                c = int(r["det_class"][b, k])
                if r["pq_gt"][b, k] > 0:
                    tp[c] += 1
                    hit[c] += 1
                    iou[c] += float(r["pq_iou"][b, k])
                elif r["pq_fp"][b, k]:
                    fp[c] += 1
            for c in range(num_classes):
                fn[c] += int(r["pq_gt_per_class"][b, c]) - hit[c]
    pq, sq, rq, n = 0.0, 0.0, 0.0, 0
    for c in range(num_classes):
        if tp[c] + fp[c] + fn[c] == 0:
            continue
        n += 1
        pq += iou[c] / (tp[c] + 0.5 * fp[c] + 0.5 * fn[c])
        sq += iou[c] / tp[c] if tp[c] != 0 else 0
        rq += tp[c] / (tp[c] + 0.5 * fp[c] + 0.5 * fn[c])
    return {"tp": np.asarray(tp, np.int64), "fp": np.asarray(fp, np.int64), "fn": np.asarray(fn, np.int64), "iou_sum": np.asarray(iou),
            "All": {"pq": pq / n if n else 0.0, "sq": sq / n if n else 0.0, "rq": rq / n if n else 0.0, "n": n}}
