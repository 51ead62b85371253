"""The inputs that tests/test_cocoeval_host.py (CPU) and tests/test_gpu_cocoeval.py share: hand cases worked out in the comments of the
host test, and random cases with crowd flags and an area override.  A case is a dict: pred, gt (sides as in tests/_match_reference.py),
crowd [B,M] int32, gt_area [B,M] float64 or None, num_classes, thresholds, area_ranges."""
import numpy as np

from tests import _cocoeval_reference as CR
from tests import _match_reference as R

MAX_INST = 8


def _fill(shape, ranges):
    """an id map whose id k + 1 covers the flat raster pixels ranges[k] = (first, last), inclusive"""
    m = np.zeros(shape[0] * shape[1], np.int32)
    for k, (a, b) in enumerate(ranges):
        m[a:b + 1] = k + 1
    return m.reshape(1, *shape)


def _case(shape, pred, pred_cls, scores, gt, gt_cls, crowd_ids, num_classes, thresholds, area_ranges, gt_area=None):
    crowd = np.zeros((1, MAX_INST), np.int32)
    crowd[0, [g - 1 for g in crowd_ids]] = 1
    case = {"pred": R.side_from_ids(_fill(shape, pred), [pred_cls], MAX_INST, [scores]),
            "gt": R.side_from_ids(_fill(shape, gt), [gt_cls], MAX_INST), "crowd": crowd, "gt_area": gt_area, "num_classes": num_classes,
            "thresholds": np.asarray(thresholds, np.float64), "area_ranges": area_ranges}
    return freeze(case)


def freeze(case):
    for v in case.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return case


ALL = [[0, 1e10]]


def hand_cases():
    """see tests/test_cocoeval_host.py for the expectations"""
    s = (2, 6)                                            # 12 pixels, flat raster 0..11
    cases = {}
    # detection 0-9; ground truth 1 = 0-2 (plain), 2 = 3-9 (crowd), the same class
    cases["break_rule"] = _case(s, [(0, 9)], [1], [0.9], [(0, 2), (3, 9)], [1, 1], [2], 3, CR.REF_THRESHOLDS, ALL)
    # detections 0-3 and 4-7 inside ground truth 1 = 0-9 (crowd); ground truth 2 = 10-11 keeps the class counted
    cases["shared_crowd"] = _case(s, [(0, 3), (4, 7)], [1, 1], [0.9, 0.8], [(0, 9), (10, 11)], [1, 1], [1], 3, CR.REF_THRESHOLDS, ALL)
    # the same geometry, ground truth 1 plain; the second range [0, 5] leaves its area of 10 out
    cases["shared_plain_out_of_range"] = _case(s, [(0, 3), (4, 7)], [1, 1], [0.9, 0.8], [(0, 9), (10, 11)], [1, 1], [], 3,
                                               CR.REF_THRESHOLDS, [[0, 1e10], [0, 5]])
    # areas 4 (= hi of small = lo of medium), 5 and 3; the detections are the ground truths
    cases["range_edges"] = _case(s, [(0, 3), (4, 8), (9, 11)], [1, 1, 1], [0.9, 0.8, 0.7], [(0, 3), (4, 8), (9, 11)], [1, 1, 1], [], 3,
                                 CR.COCO_THRESHOLDS, CR.SMALL_AREA_RANGES)
    # class 2 has one ground truth and it is crowd; class 1 has a plain one
    cases["crowd_only"] = _case(s, [(0, 3), (6, 9)], [1, 2], [0.9, 0.8], [(0, 3), (6, 11)], [1, 2], [2], 3, CR.COCO_THRESHOLDS, ALL)
    # 4 x 6.  Ground truth 1 = 0-5 crowd of class 1, 2 = 6-9 plain of class 2, 3 = 12-17 crowd of class 2, 4 = 18-21 plain of class 1.
    # Detection 1 = 0-9 class 1 (6 pixels on crowd 1, 4 on ground truth 2), 2 = 12-17 class 2 (= crowd 3), 3 = 18-21 class 1 (= 4)
    cases["pq_same_class"] = _case((4, 6), [(0, 9), (12, 17), (18, 21)], [1, 2, 1], [0.9, 0.8, 0.7],
                                   [(0, 5), (6, 9), (12, 17), (18, 21)], [1, 2, 2, 1], [1, 3], 3, CR.COCO_THRESHOLDS, ALL)
    # the same with detection 1 in class 2 and crowd 3 moved out of its class: its crowd region 1 is of another class
    cases["pq_other_class"] = _case((4, 6), [(0, 9), (12, 17), (18, 21)], [2, 1, 1], [0.9, 0.8, 0.7],
                                    [(0, 5), (6, 9), (12, 17), (18, 21)], [1, 1, 1, 1], [1, 3], 3, CR.COCO_THRESHOLDS, ALL)
    return cases


# (seed, H, W, num_classes, block): searched on the CPU until every counter of the restatement fires (test_cocoeval_host.py asserts it).
# The rare one is the stop at the first ignored ground truth with a larger IoU behind it: about one seed in forty reaches it.
RANDOM = [(3, 13, 9, 3, 2), (20, 20, 24, 5, 3)]


def random_case(seed, H, W, num_classes=5, block=3, B=3, max_inst=64):
    """block-noise ids of _match_reference.random_case; a random third of the ground truths crowd; on image 1 an annotated area that
    differs from the pixel area (multiples of a half, so that range edges are hit); the four ranges scaled to the image; T = 10 from 0.30"""
    pred, gt = R.random_case(seed, B, H, W, num_classes, block=block, max_inst=max_inst)
    rng = np.random.default_rng(1000 + seed)
    crowd = (rng.random((B, max_inst)) < 1 / 3).astype(np.int32)
    gt_area = gt["table"][:, :, 1].astype(np.float64)
    gt_area[1] = rng.integers(1, 25, max_inst) / 2.0
    return freeze({"pred": pred, "gt": gt, "crowd": crowd, "gt_area": gt_area, "num_classes": num_classes,
                   "thresholds": CR.REF_THRESHOLDS, "area_ranges": CR.SMALL_AREA_RANGES})


def reference(case, **kw):
    return CR.evaluate(case["pred"], case["gt"], case["num_classes"], case["crowd"], case["gt_area"], case["thresholds"],
                       case["area_ranges"], **kw)
