"""CPU: the naive restatement of the full COCO / panoptic evaluation (tests/_cocoeval_reference.py) on hand cases, and the host half of
the product -- CocoEval.compute / summarize and PanopticQuality on a CocoMatches -- against it.  The GPU half is
tests/test_gpu_cocoeval.py; the cases are shared through tests/_cocoeval_cases.py."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import _cocoeval_cases as C
from tests import _cocoeval_reference as CR

FIELDS = ("det_valid", "det_class", "det_rank", "det_score", "det_gt", "det_iou", "det_ignore", "gt_counted", "pq_gt_per_class", "pq_gt",
          "pq_iou", "pq_fp", "overflow")


def as_matches(res):
    """a CocoMatches of CPU tensors from the restatement's arrays"""
    from maskunet_amd import CocoMatches
    return CocoMatches(*[torch.from_numpy(np.ascontiguousarray(res[k])) for k in FIELDS])


@functools.lru_cache(maxsize=None)
def hand():
    return {name: (case, *C.reference(case)) for name, case in C.hand_cases().items()}


@functools.lru_cache(maxsize=None)
def random_result(i):
    case = C.random_case(*C.RANDOM[i])
    return (case, *C.reference(case))


# ------------------------------------------------------------------------------------------------
# 1. hand cases.  Rows k = 0, 1, .. are the detections in score order; [A,T,K] arrays are indexed [range, threshold, row].
def test_break_rule_non_ignored_before_ignored():
    """Thresholds linspace(0.30, 0.95, 10) = 0.3, 0.3722, 0.4444, 0.5167, 0.5889, 0.6611, 0.7333, ...  The detection has 10 pixels.
    Ground truth 1 (plain, 3 pixels inside it): 3 / (10 + 3 - 3) = 0.3 exactly, the first threshold itself.  Ground truth 2 (crowd,
    the other 7 pixels): 7 / 10 = 0.7.  The plain one is visited first.
      t = 0.3             1 reaches the threshold; the walk stops at the ignored ground truth 2 although its IoU is larger: a true
                          positive, not ignored.  A matcher that visits both in one pass takes 2 here.
      t = 0.3722..0.6611  1 fails, 2 matches: the detection is ignored.
      t >= 0.7333         0.7 fails as well: unmatched, and its area of 10 is inside [0, 1e10], so it is a false positive.
    (With this geometry the crowd match cannot hold above 0.7; the five thresholds in between are the ones it holds at.)"""
    case, res, cnt = hand()["break_rule"]
    assert case["thresholds"][0] == 0.3 == 3 / 10
    assert res["det_gt"][0, 0, :, 0].tolist() == [1, 2, 2, 2, 2, 2, 0, 0, 0, 0]
    assert res["det_ignore"][0, 0, :, 0].tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert res["det_iou"][0, 0, :, 0].tolist() == [0.3] + [0.7] * 5 + [0.0] * 4
    assert res["gt_counted"][0, 0].tolist() == [0, 1, 0]
    assert cnt["break_hid_better"] == 1 and cnt["matched_ignored"] == 5


def test_two_detections_share_a_crowd_region():
    """Detections of 4 pixels each inside a crowd region of 10: 4 / 4 = 1.0 for both, at every threshold; the second one matches the
    region although the first already did, and both are ignored.  Ground truth 2 (plain, untouched) is the only one counted."""
    _, res, cnt = hand()["shared_crowd"]
    assert (res["det_gt"][0, 0, :, :2] == 1).all() and (res["det_ignore"][0, 0, :, :2] == 1).all()
    assert (res["det_iou"][0, 0, :, :2] == 1.0).all()
    assert res["gt_counted"][0, 0].tolist() == [0, 1, 0]
    assert cnt["crowd_rematched"] == 10 and cnt["matched_ignored"] == 20


def test_a_plain_ground_truth_outside_the_range_is_matched_once():
    """The same geometry with ground truth 1 plain: IoU 4 / 10 = 0.4, above the thresholds 0.3 and 0.3722 only.
      range [0, 1e10]  row 0 matches 1 (counted); row 1 finds it taken, and 0 / .. with ground truth 2: unmatched, a false positive.
      range [0, 5]     1 is ignored (area 10 > 5) and visited after 2.  Row 0 still matches it and is ignored; row 1 finds it taken --
                       it is not crowd -- and stays unmatched; its own area 4 is inside the range, so it is NOT ignored."""
    _, res, cnt = hand()["shared_plain_out_of_range"]
    for a in range(2):
        assert res["det_gt"][0, a, :, 0].tolist() == [1, 1] + [0] * 8 and not res["det_gt"][0, a, :, 1].any()
        assert not res["det_ignore"][0, a, :, 1].any()
    assert not res["det_ignore"][0, 0].any() and res["det_ignore"][0, 1, :, 0].tolist() == [1, 1] + [0] * 8
    assert res["gt_counted"][0].tolist() == [[0, 2, 0], [0, 1, 0]]
    assert cnt["crowd_rematched"] == 0


def test_range_edges_are_inclusive():
    """Ranges [0, 1e10], [0, 4], [4, 9], [9, 1e10]; ground truths of area 4, 5 and 3.  Area 4 = hi of small = lo of medium counts in
    both; every detection is its ground truth (IoU 1) and is ignored exactly where that one is."""
    _, res, _ = hand()["range_edges"]
    assert res["gt_counted"][0, :, 1].tolist() == [3, 2, 2, 0]
    assert (res["det_gt"][0, :, :, :3] == [1, 2, 3]).all()
    assert [res["det_ignore"][0, a, 0, :3].tolist() for a in range(4)] == [[0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]]


def test_a_class_with_only_a_crowd_ground_truth_is_not_evaluated():
    """class 2: one crowd ground truth -> npig = 0, precision and recall stay -1; its detection (4 of 4 pixels inside) is ignored"""
    case, res, _ = hand()["crowd_only"]
    assert res["gt_counted"][0, 0].tolist() == [0, 1, 0] and (res["det_ignore"][0, 0, :, 1] == 1).all()
    acc = CR.accumulate([res], 3, case["thresholds"], case["area_ranges"])
    assert (acc["precision"][:, :, 2] == -1).all() and (acc["recall"][:, 2] == -1).all()
    assert (acc["precision"][:, :, 1] == 1 / (1 + np.spacing(1))).all() and (acc["recall"][:, 1] == 1).all()      # one true positive


def test_panoptic_crowd_rules():
    """pq_same_class: rows = detections 1 (10 pixels: 6 on the crowd region of its class 1, 4 on a plain segment of class 2), 2 (equal to
    the crowd region of class 2), 3 (equal to the plain ground truth 4).  A crowd region is no candidate: row 1 is unmatched although it
    covers it exactly, and neither crowd region is counted -> no true positive and no false negative from them.  Rows 0 and 1 are
    unmatched but 6 / 10 > 0.5 and 6 / 6 > 0.5 lie on the crowd region of their own class: no false positives.
    pq_other_class: row 0 now has class 2, the region under it is a crowd region of class 1: 0 / 10, a false positive."""
    _, res, cnt = hand()["pq_same_class"]
    assert res["pq_gt"][0, :3].tolist() == [0, 0, 4] and res["pq_fp"][0, :3].tolist() == [0, 0, 0]
    assert res["pq_gt_per_class"][0].tolist() == [0, 1, 1] and cnt["crowd_saved"] == 2
    pq = CR.accumulate_pq([res], 3)
    assert pq["tp"].tolist() == [0, 1, 0] and pq["fp"].tolist() == [0, 0, 0] and pq["fn"].tolist() == [0, 0, 1]
    _, res, cnt = hand()["pq_other_class"]
    assert res["pq_gt"][0, :3].tolist() == [0, 0, 4] and res["pq_fp"][0, :3].tolist() == [1, 0, 0] and cnt["crowd_saved"] == 1


# ------------------------------------------------------------------------------------------------
# 3. the random cases of the GPU test reach every branch that has a counter
@pytest.mark.parametrize("i", range(len(C.RANDOM)))
def test_random_cases_reach_every_counted_branch(i):
    case, res, cnt = random_result(i)
    print(cnt)
    assert all(cnt[k] > 0 for k in CR.COUNTERS), cnt
    assert not res["overflow"].any() and case["crowd"].any()
    assert (case["gt_area"][1] != case["gt"]["table"][1, :, 1]).any()
    assert (res["gt_counted"].sum((0, 2)) > 0).all()                 # every range holds ground truths


# ------------------------------------------------------------------------------------------------
# 2. CocoEval against the restatement's accumulate / summarize
def _both(results, num_classes, thresholds, area_ranges, max_dets=(1, 10, 100)):
    import maskunet_amd
    acc = maskunet_amd.CocoEval(num_classes, thresholds, area_ranges, max_dets)
    for r in results:
        acc.update(as_matches(r))
    got = acc.compute()
    want = CR.accumulate(results, num_classes, thresholds, area_ranges, max_dets)
    assert got["precision"].shape == want["precision"].shape and got["recall"].shape == want["recall"].shape
    assert np.array_equal(got["precision"], want["precision"])
    assert np.array_equal(got["recall"], want["recall"])
    return acc, got, want


@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_coco_eval_on_hand_cases(name):
    case, res, _ = hand()[name]
    _both([res], case["num_classes"], case["thresholds"], case["area_ranges"])


@pytest.mark.parametrize("i", range(len(C.RANDOM)))
def test_coco_eval_on_random_cases_two_updates(i):
    """precision / recall exactly; the twelve stats within 1e-12 (means over at most 1e5 values of [0, 1], summed in another order)"""
    case, res, _ = random_result(i)
    other = C.random_case(C.RANDOM[i][0] + 1, *C.RANDOM[i][1:])
    acc, got, want = _both([res, C.reference(other)[0]], case["num_classes"], case["thresholds"], case["area_ranges"])
    stats = CR.summarize(want, case["thresholds"])
    print(got["stats"].tolist())
    assert got["stats"].shape == (12,) and got["stats"].dtype == np.float64
    assert np.abs(got["stats"] - stats).max() <= 1e-12
    assert (stats[[0, 3, 4, 5, 6, 7, 8]] > 0).all() and stats[6] < stats[7] <= stats[8]          # the maxDets ladder cuts
    assert stats[1] == -1 and stats[2] == -1                 # linspace(0.30, 0.95, 10) holds neither 0.5 nor 0.75


def test_stats_select_the_exact_thresholds_and_summarize_wording():
    import maskunet_amd
    case, res, _ = hand()["range_edges"]                     # COCO's ladder: 0.5 and 0.75 are there
    acc, got, want = _both([res], 3, case["thresholds"], case["area_ranges"])
    assert np.abs(got["stats"] - CR.summarize(want, case["thresholds"])).max() <= 1e-12
    assert got["stats"][:5].tolist() == [1.0] * 5 and got["stats"][5] == -1.0 and got["stats"][11] == -1.0      # nothing is large
    lines = acc.summarize()
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000"
    assert lines[5] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.333"
    assert lines[10] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = 1.000"
    # one range and one maxDet: the entries that are not configured are NaN, the arrays are complete
    case, res, _ = hand()["shared_crowd"]
    one = maskunet_amd.CocoEval(3, case["thresholds"], case["area_ranges"], max_dets=(100,))
    one.update(as_matches(res))
    out = one.compute()
    assert out["precision"].shape == (10, 101, 3, 1, 1) and out["recall"].shape == (10, 3, 1, 1)
    assert np.isnan(out["stats"][[3, 4, 5, 7, 8, 9, 10, 11]]).all() and not np.isnan(out["stats"][[0, 1, 2, 6]]).any()
    assert out["stats"][0] == 0.0 and out["stats"][6] == 0.0 and len(one.summarize()) == 4        # both detections are ignored


def test_panoptic_quality_takes_coco_matches():
    import maskunet_amd
    case, res, _ = random_result(1)
    acc = maskunet_amd.PanopticQuality(case["num_classes"])
    acc.update(as_matches(res))
    acc.update(as_matches(hand_as(case["num_classes"])))
    got, want = acc.compute(), CR.accumulate_pq([res, hand_as(case["num_classes"])], case["num_classes"])
    for k in ("tp", "fp", "fn"):
        assert np.array_equal(got[k], want[k]), k
    assert want["tp"].sum() > 0 and want["fp"].sum() > 0 and want["fn"].sum() > 0
    for k in ("pq", "sq", "rq"):
        assert math.isclose(got["All"][k], want["All"][k], rel_tol=1e-12), k
    assert got["All"]["n"] == want["All"]["n"]


def hand_as(num_classes):
    """pq_same_class evaluated for another number of classes, so that it can be accumulated with a random case"""
    case = C.hand_cases()["pq_same_class"]
    return CR.evaluate(case["pred"], case["gt"], num_classes, case["crowd"], None, CR.REF_THRESHOLDS, CR.SMALL_AREA_RANGES)[0]


def test_accumulators_refuse_what_they_cannot_use():
    import maskunet_amd
    case, res, _ = hand()["range_edges"]
    m = as_matches(res)
    with pytest.raises(TypeError):
        maskunet_amd.InstanceAP(3).update(m)
    with pytest.raises(ValueError, match="classes"):
        maskunet_amd.CocoEval(4, case["thresholds"], case["area_ranges"]).update(m)
    with pytest.raises(ValueError, match="area ranges"):
        maskunet_amd.CocoEval(3, case["thresholds"]).update(as_matches(hand()["crowd_only"][1]))
    with pytest.raises(ValueError, match="max_dets"):
        maskunet_amd.CocoEval(3, max_dets=(10, 1))
    with pytest.raises(ValueError, match="area_ranges"):
        maskunet_amd.CocoEval(3, area_ranges=[[5, 4]])
    with pytest.raises(RuntimeError, match="before any update"):
        maskunet_amd.CocoEval(3).compute()
    over = dict(res, overflow=np.ones(1, np.int32))
    acc = maskunet_amd.CocoEval(3, case["thresholds"], case["area_ranges"])
    acc.update(as_matches(over))
    with pytest.raises(RuntimeError, match="max_instances"):
        acc.compute()
    acc.reset()
    acc.update(m)
    assert acc.compute()["stats"][0] == 1.0


def test_c_entry_refuses_before_any_launch():
    """null pointers, limits and values through the C ABI: every refusal returns before a launch, so this needs no GPU"""
    import ctypes
    from maskunet_amd import _lib
    lib = _lib.load()
    ok = (16, 16, 8, 8, 5, 8, 100, 10, 4)
    assert lib.mu_coco_match_supported(*ok) == 0
    assert lib.mu_coco_match_supported(*ok[:8], 5) == -2 and lib.mu_coco_match_supported(*ok[:8], 0) == -2
    assert lib.mu_coco_match_supported(*ok[:7], 33, 4) == -2 and lib.mu_coco_match_supported(257, 256, *ok[2:]) == -2
    assert lib.mu_coco_match_workspace_bytes(3, 8) == 3 * 8 * 4 and lib.mu_coco_match_workspace_bytes(0, 8) == 0
    buf = (ctypes.c_double * 4096)()                          # stands in for every pointer: nothing is read before the refusal
    p = ctypes.cast(buf, ctypes.c_void_p)
    thr = np.linspace(0.5, 0.95, 10)
    rng = np.asarray(CR.COCO_AREA_RANGES, np.float64)

    def run(thr=thr, rng=rng, A=4, T=10, first=p, ws=2 * 8 * 4):
        return lib.mu_coco_match(first, p, p, p, p, p, p, p, None, None, 2, 16, 16, 8, 8, 5, 8, 100, thr.ctypes.data, T, rng.ctypes.data, A,
                                 *[p] * 13, p, ws, None)

    assert run(first=None) == -1
    assert run(A=5) == -2 and run(T=33, thr=np.full(33, 0.5)) == -2
    assert run(thr=np.r_[0.0, thr[1:]]) == -1 and run(thr=np.r_[thr[:9], np.nan]) == -1 and run(thr=np.r_[thr[:9], 1.5]) == -1
    bad = rng.copy()
    bad[2] = [9.0, 4.0]
    assert run(rng=bad) == -1
    bad[2] = [np.nan, 4.0]
    assert run(rng=bad) == -1
    assert run(ws=2 * 8 * 4 - 1) == -4


def test_exports():
    import maskunet_amd
    for n in ("coco_match", "CocoMatches", "CocoEval"):
        assert n in maskunet_amd.__all__ and hasattr(maskunet_amd, n)
    with pytest.raises(TypeError):
        maskunet_amd.coco_match(None, None, 3)
