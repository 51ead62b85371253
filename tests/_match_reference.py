"""CPU restatement of the instance-matching contract (maskunet_amd.matching), deliberately naive and sharing no code with the product:
boolean masks derived from id maps, IoUs by (a & b).sum(), and the three published algorithms as literal loops --
COCOeval.evaluateImg's greedy matching, COCOeval.accumulate, and panopticapi's pq_compute_single_core with VOID = ground-truth id 0 and
no crowd.  Written from the contract, not from the kernels.

A "side" is a dict of numpy arrays as the instance producers return them: ids [B,H,W], count [B], table [B,M,8] (column 0 = class,
1 = area), score [B,M], order [B,M].  An instance takes part iff its id <= min(count, M) and its class is one of 1..num_classes-1.
"""
import numpy as np

from tests._instances_reference import table_from_ids

DEFAULT_THRESHOLDS = np.linspace(0.5, 0.95, 10)


def side_from_ids(ids, classes, max_inst, scores=None):
    """A side from arbitrary id maps: ids [B,H,W] (ids 1..n_b, every one present, regions of any shape), classes[b][k-1] the class of
    id k, scores[b][k-1] its score (1.0 without).  Order: score descending (as fp32), ties by ascending id."""
    ids = np.asarray(ids, np.int32)
    r = table_from_ids(ids, classes, max_inst, scores)
    assert (r["table"][:, :, 1] > 0).sum(1).tolist() == np.minimum(r["count"], max_inst).tolist(), "every id must be present"
    return {"ids": ids, "count": r["count"], "table": r["table"], "score": r["score"].astype(np.float32), "order": r["order"]}


def pair_table(pred_ids, gt_ids, max_pred, max_gt):
    """pairs [B,H*W,3] sorted by (p, g), zero padded, and n_pairs [B]: ids outside 1..max count as 0, p = 0 is dropped."""
    B, H, W = pred_ids.shape
    pairs = np.zeros((B, H * W, 3), np.int32)
    n_pairs = np.zeros(B, np.int32)
    for b in range(B):
        p_map = np.where((pred_ids[b] >= 1) & (pred_ids[b] <= max_pred), pred_ids[b], 0)
        g_map = np.where((gt_ids[b] >= 1) & (gt_ids[b] <= max_gt), gt_ids[b], 0)
        n = 0
        for p in sorted(set(p_map.reshape(-1).tolist()) - {0}):
            under = g_map[p_map == p]
            for g in sorted(set(under.tolist())):
                pairs[b, n] = [p, g, int((under == g).sum())]
                n += 1
        n_pairs[b] = n
    return pairs, n_pairs


def _takes_part(side, b, k, num_classes):
    M = side["table"].shape[1]
    return 1 <= k <= min(int(side["count"][b]), M) and 1 <= int(side["table"][b, k - 1, 0]) < num_classes


def lists_from_sides(pred, gt, b, num_classes, max_queries=None):
    """dets: one entry per row of order[b, :max_queries] -- None, or {"id", "mask", "category_id", "score"}; gts: the ground truths
    that take part, ascending id, {"id", "mask", "category_id"}; void: the pixels of no such ground truth."""
    K = pred["order"].shape[1] if max_queries is None else min(max_queries, pred["order"].shape[1])
    dets = []
    for k in pred["order"][b, :K].tolist():
        if _takes_part(pred, b, k, num_classes):
            dets.append({"id": k, "mask": pred["ids"][b] == k, "category_id": int(pred["table"][b, k - 1, 0]),
                         "score": float(pred["score"][b, k - 1])})
        else:
            dets.append(None)
    gts = [{"id": g, "mask": gt["ids"][b] == g, "category_id": int(gt["table"][b, g - 1, 0])}
           for g in range(1, gt["table"].shape[1] + 1) if _takes_part(gt, b, g, num_classes)]
    void = np.ones(pred["ids"][b].shape, bool)
    for g in gts:
        void &= ~g["mask"]
    return dets, gts, void


def match_image(dets, gts, void, num_classes, thresholds, max_dets):
    """One image.  dets / gts / void as lists_from_sides gives them (dets in score order; None rows are kept as zero rows).
    Returns a dict of per-row arrays [K] / [T,K] and gt_per_class [num_classes]."""
    K, T = len(dets), len(thresholds)
    out = {"det_valid": np.zeros(K, np.int32), "det_class": np.zeros(K, np.int32), "det_score": np.zeros(K, np.float32),
           "det_gt": np.zeros((T, K), np.int32), "det_iou": np.zeros((T, K), np.float64), "gt_per_class": np.zeros(num_classes, np.int32),
           "pq_gt": np.zeros(K, np.int32), "pq_iou": np.zeros(K, np.float64), "pq_fp": np.zeros(K, np.int32)}
    for g in gts:
        out["gt_per_class"][g["category_id"]] += 1
    for c in range(1, num_classes):
        rows = [k for k, d in enumerate(dets) if d is not None and d["category_id"] == c][:max_dets]       # maxDets per (image, class)
        gt_c = [g for g in gts if g["category_id"] == c]
        for k in rows:
            out["det_valid"][k] = 1
            out["det_class"][k] = c
            out["det_score"][k] = np.float32(dets[k]["score"])
        # maskUtils.iou
        ious = np.zeros((len(rows), len(gt_c)))
        for a, k in enumerate(rows):
            for j, g in enumerate(gt_c):
                inter = int((dets[k]["mask"] & g["mask"]).sum())
                union = int(dets[k]["mask"].sum()) + int(g["mask"].sum()) - inter
                ious[a, j] = float(inter) / float(union)
        # COCOeval.evaluateImg, no crowd, no ignore
        for ti, t in enumerate(thresholds):
            gtm = [0] * len(gt_c)
            for a, k in enumerate(rows):
                iou = min([t, 1 - 1e-10])
                m = -1
                for j in range(len(gt_c)):
                    if gtm[j] > 0:
                        continue
                    if ious[a, j] < iou:
                        continue
                    iou = ious[a, j]
                    m = j
                if m == -1:
                    continue
                gtm[m] = 1
                out["det_gt"][ti, k] = gt_c[m]["id"]
                out["det_iou"][ti, k] = iou
        # panopticapi: pq_compute_single_core
        for k in rows:
            area = int(dets[k]["mask"].sum())
            v = int((dets[k]["mask"] & void).sum())
            for g in gt_c:
                inter = int((dets[k]["mask"] & g["mask"]).sum())
                if inter == 0:
                    continue
                union = area + int(g["mask"].sum()) - inter - v
                iou = inter / union
                if iou > 0.5:
                    assert out["pq_gt"][k] == 0, "at most one match per segment"
                    out["pq_gt"][k] = g["id"]
                    out["pq_iou"][k] = iou
            if out["pq_gt"][k] == 0 and not v / area > 0.5:
                out["pq_fp"][k] = 1
    return out


def match(pred, gt, num_classes, thresholds=None, max_queries=None, max_dets=100):
    """All images: arrays with a leading batch axis, plus pairs / n_pairs and overflow."""
    thresholds = DEFAULT_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64)
    B = pred["ids"].shape[0]
    per = []
    for b in range(B):
        dets, gts, void = lists_from_sides(pred, gt, b, num_classes, max_queries)
        per.append(match_image(dets, gts, void, num_classes, thresholds, max_dets))
    out = {k: np.stack([p[k] for p in per]) for k in per[0]}
    out["overflow"] = ((pred["count"] > pred["table"].shape[1]) | (gt["count"] > gt["table"].shape[1])).astype(np.int32)
    out["pairs"], out["n_pairs"] = pair_table(pred["ids"], gt["ids"], pred["table"].shape[1], gt["table"].shape[1])
    return out


def accumulate_ap(results, num_classes, thresholds=None):
    """COCOeval.accumulate over a list of match() results (area range all, one maxDets): precision [T,101,num_classes], ap."""
    thresholds = DEFAULT_THRESHOLDS if thresholds is None else np.asarray(thresholds, np.float64)
    T = len(thresholds)
    rec_thrs = np.linspace(.0, 1.00, 101)
    precision = -np.ones((T, 101, num_classes))
    for c in range(num_classes):
        scores, matched, npig = [], [[] for _ in range(T)], 0
        for r in results:
            for b in range(r["det_valid"].shape[0]):
                npig += int(r["gt_per_class"][b, c])
                for k in range(r["det_valid"].shape[1]):
                    if r["det_valid"][b, k] and r["det_class"][b, k] == c:
                        scores.append(float(r["det_score"][b, k]))
                        for t in range(T):
                            matched[t].append(int(r["det_gt"][b, t, k]))
        if npig == 0:
            continue
        inds = np.argsort(-np.asarray(scores, np.float64), kind="mergesort")
        for t in range(T):
            dtm = np.asarray(matched[t], np.int64)[inds]
            tp = np.cumsum(dtm > 0).astype(dtype=float)
            fp = np.cumsum(dtm == 0).astype(dtype=float)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            q = np.zeros((101,))
            pr = pr.tolist()
            q = q.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            ri_inds = np.searchsorted(rc, rec_thrs, side="left")
            try:
                for ri, pi in enumerate(ri_inds):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[t, :, c] = np.array(q)
    s = precision[precision > -1]
    return {"precision": precision, "ap": -1.0 if len(s) == 0 else float(np.mean(s))}


def accumulate_pq(results, num_classes, things=None):
    """panopticapi's PQStat over a list of match() results: per-class tp / fp / fn / iou_sum / pq / sq / rq and the means."""
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
                fn[c] += int(r["gt_per_class"][b, c]) - hit[c]
    out = {"tp": np.asarray(tp, np.int64), "fp": np.asarray(fp, np.int64), "fn": np.asarray(fn, np.int64), "iou_sum": np.asarray(iou),
           "pq": np.zeros(num_classes), "sq": np.zeros(num_classes), "rq": np.zeros(num_classes)}
    groups = {"All": [True] * num_classes}
    if things is not None:
        groups["Things"] = [bool(x) for x in things]
        groups["Stuff"] = [not bool(x) for x in things]
    for name, member in groups.items():
        pq, sq, rq, n = 0.0, 0.0, 0.0, 0
        for c in range(num_classes):
            if not member[c] or tp[c] + fp[c] + fn[c] == 0:
                continue
            n += 1
            pq_c = iou[c] / (tp[c] + 0.5 * fp[c] + 0.5 * fn[c])
            sq_c = iou[c] / tp[c] if tp[c] != 0 else 0
            rq_c = tp[c] / (tp[c] + 0.5 * fp[c] + 0.5 * fn[c])
            out["pq"][c], out["sq"][c], out["rq"][c] = pq_c, sq_c, rq_c
            pq += pq_c
            sq += sq_c
            rq += rq_c
        out[name] = {"pq": pq / n if n else 0.0, "sq": sq / n if n else 0.0, "rq": rq / n if n else 0.0, "n": n}
    return out


# ------------------------------------------------------------------------------------------------
# cases that the host and the GPU tests share
def hand_case():
    """One 8x8 image, 4 classes, worked out by hand in tests/test_match_host.py.  Flat raster pixel ranges (inclusive):
         gt   1: 0-9     2: 10-17    3: 18-27    4: 28-47   (class 1)   5: 48-49   6: 50-51 (class 2)   7: 52-57 (class 3)   58-63: none
         pred 1: 0-4     2: 10-15    3: 18-26    4: 28-46   (class 1)   5: 48-51 (class 2)   6: 52-54   7: 55-57   8: 58-61 (class 3)
         score   0.9        0.8         0.7         0.6                    0.55                 0.5        0.5        0.4"""
    def fill(ranges):
        m = np.zeros(64, np.int32)
        for k, (a, b) in enumerate(ranges):
            m[a:b + 1] = k + 1
        return m.reshape(1, 8, 8)
    gt = side_from_ids(fill([(0, 9), (10, 17), (18, 27), (28, 47), (48, 49), (50, 51), (52, 57)]), [[1, 1, 1, 1, 2, 2, 3]], 16)
    pred = side_from_ids(fill([(0, 4), (10, 15), (18, 26), (28, 46), (48, 51), (52, 54), (55, 57), (58, 61)]),
                         [[1, 1, 1, 1, 2, 3, 3, 3]], 16, [[0.9, 0.8, 0.7, 0.6, 0.55, 0.5, 0.5, 0.4]])
    return pred, gt


def compact(ids):
    """relabel every image of ids [B,H,W] to 1..n in order of first appearance; 0 stays"""
    out = np.zeros_like(ids, dtype=np.int32)
    for b in range(ids.shape[0]):
        seen = {0: 0}
        flat = ids[b].reshape(-1)
        o = out[b].reshape(-1)
        for i, v in enumerate(flat.tolist()):
            if v not in seen:
                seen[v] = len(seen)
            o[i] = seen[v]
    return out


def random_case(seed, B, H, W, num_classes, block=3, max_inst=64, wild_classes=True):
    """Blocky ground-truth ids; the prediction is the same pattern drawn again with some blocks merged or moved by a pixel and some
    pixels flipped, so IoUs spread over (0, 1].  Regions are not connected in general.  Classes are drawn from 0..num_classes (both ends
    do not take part) when wild_classes, else from 1..num_classes-1; a prediction takes the class of the ground truth it overlaps most
    three times out of four.  Scores have ties (multiples of 1/8)."""
    rng = np.random.default_rng(seed)
    hb, wb = (H + block - 1) // block, (W + block - 1) // block
    g_ids, p_ids = np.zeros((B, H, W), np.int64), np.zeros((B, H, W), np.int64)
    for b in range(B):
        small = rng.integers(0, max(2, hb * wb // 3), (hb, wb))
        g = np.kron(small, np.ones((block, block), np.int64))[:H, :W]
        p = np.roll(g, int(rng.integers(0, 2)), axis=1) + 1000 * (rng.random((H, W)) < 0.08)
        p = np.where(rng.random((H, W)) < 0.1, 0, p)
        g_ids[b], p_ids[b] = g, p
    g_ids, p_ids = compact(g_ids), compact(p_ids)
    lo, hi = (0, num_classes + 1) if wild_classes else (1, num_classes)
    g_cls, p_cls, p_sc = [], [], []
    for b in range(B):
        gc = rng.integers(lo, hi, int(g_ids[b].max()))
        pc = rng.integers(lo, hi, int(p_ids[b].max()))
        for k in range(1, len(pc) + 1):
            under = g_ids[b][p_ids[b] == k]
            under = under[under > 0]
            if len(under) and rng.random() < 0.75:
                pc[k - 1] = gc[np.bincount(under).argmax() - 1]
        g_cls.append(gc)
        p_cls.append(pc)
        p_sc.append(rng.integers(1, 9, len(pc)) / 8.0)
    return side_from_ids(p_ids, p_cls, max_inst, p_sc), side_from_ids(g_ids, g_cls, max_inst)
