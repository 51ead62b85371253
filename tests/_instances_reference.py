"""CPU restatement of the per-instance statistics that every `Instances` producer ends with (inst_stats_kernel): the table, the score and
the score order of an id map.  The four contracts (_cc_reference, _dbscan_reference, _idmap_reference, _match_reference) differ in how
pixels get their id and instances their class; from there on they share this.  Written from the contract, not from the kernel:

  - table row k-1 = class, area, x_min, y_min, x_max, y_max, first_pixel (y*W+x), class_rank (1-based rank among the instances of the
    same class in id order) of id k;
  - order = ids by descending score AS FP32 (the device sorts the score it returns), ties by ascending id;
  - table / score / order hold ids 1..min(count, max_instances), the rest is 0.
"""
import numpy as np


def table_from_ids(ids, classes, max_instances, scores=None):
    """ids [B,H,W] ints (0 = background, ids 1..count as every producer numbers them, also past max_instances), classes[b][k-1] the
    class of id k, scores[b][k-1] its score in float64 (None: 1.0) -> dict of count, table, score (float64), order.  One vectorised
    pass per image, no scan per id."""
    ids = np.asarray(ids)
    B, H, W = ids.shape
    M = max_instances
    count = np.zeros(B, np.int32)
    table = np.zeros((B, M, 8), np.int32)
    score = np.zeros((B, M), np.float64)
    order = np.zeros((B, M), np.int32)
    for b in range(B):
        flat = ids[b].reshape(-1)
        count[b] = flat.max()                              # = the number of distinct ids
        K = min(int(count[b]), M)
        if K == 0:
            continue
        pix = np.flatnonzero((flat >= 1) & (flat <= K))
        k = flat[pix].astype(np.int64) - 1
        area = np.bincount(k, minlength=K)
        lo = np.full((3, K), np.iinfo(np.int64).max)
        hi = np.zeros((2, K), np.int64)
        np.minimum.at(lo[0], k, pix % W)
        np.minimum.at(lo[1], k, pix // W)
        np.minimum.at(lo[2], k, pix)
        np.maximum.at(hi[0], k, pix % W)
        np.maximum.at(hi[1], k, pix // W)
        lo[:, area == 0] = 0                               # an id no pixel holds (a hidden annotation): an empty row
        cls = np.asarray(classes[b], np.int64)[:K]
        seen, rank = {}, np.zeros(K, np.int64)
        for j, c in enumerate(cls.tolist()):
            seen[c] = rank[j] = seen.get(c, 0) + 1
        table[b, :K] = np.stack([cls, area, lo[0], lo[1], hi[0], hi[1], lo[2], rank], 1)
        score[b, :K] = 1.0 if scores is None else np.asarray(scores[b], np.float64)[:K]
        order[b, :K] = 1 + np.argsort(-score[b, :K].astype(np.float32), kind="stable")
    return {"count": count, "table": table, "score": score, "order": order}
