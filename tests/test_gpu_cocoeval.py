"""GPU: mu_coco_match / maskunet_amd.coco_match / CocoEval / PanopticQuality on a CocoMatches against the naive restatement in
tests/_cocoeval_reference.py.  Every comparison is exact: integers with ==, det_iou / pq_iou bit for bit (each is ONE correctly rounded
fp64 division of the same two integers on both sides), det_score as fp32.  Raw sides go through the C ABI with the memory discipline of
test_gpu_match.py: outputs pre-filled with a sentinel and all written, the workspace exactly the queried size, 4 KiB guard bands around
every buffer, inputs verified untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import _cocoeval_cases as C
from tests import _cocoeval_reference as CR
from tests import _match_reference as R
from tests._device_buffers import Guarded, call, side_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_KEYS = ("det_valid", "det_class", "det_rank", "det_score", "det_gt", "det_iou", "det_ignore", "gt_counted", "pq_gt_per_class",
            "pq_gt", "pq_iou", "pq_fp", "overflow")


def run_coco(pred, gt, num_classes, crowd=None, gt_area=None, thresholds=None, area_ranges=None, max_queries=None, max_det=100):
    """raw mu_instance_pairs + mu_coco_match on two sides -> dict of numpy outputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    thr = np.ascontiguousarray(CR.COCO_THRESHOLDS if thresholds is None else thresholds, np.float64)
    rng = np.ascontiguousarray(CR.COCO_AREA_RANGES if area_ranges is None else area_ranges, np.float64)
    B, H, W = pred["ids"].shape
    Mp, Mg, T, A, N = pred["table"].shape[1], gt["table"].shape[1], len(thr), len(rng), H * W
    K = Mp if max_queries is None else min(max_queries, Mp)
    i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
    sizes = {"ids": (B * N, i32), "table": (B * Mp * 8, i32), "score": (B * Mp, f32), "order": (B * Mp, i32), "count": (B, i32)}
    p_in = {k: Guarded(n, d, pred[k], "pred " + k) for k, (n, d) in sizes.items()}
    g_in = {k: Guarded(n, i32, gt[k], "gt " + k) for k, n in (("ids", B * N), ("table", B * Mg * 8), ("count", B))}
    g_crowd = None if crowd is None else Guarded(B * Mg, i32, crowd, "gt crowd")
    g_area = None if gt_area is None else Guarded(B * Mg, f64, gt_area, "gt area")
    shapes = {"det_valid": ((B, K), i32), "det_class": ((B, K), i32), "det_rank": ((B, K), i32), "det_score": ((B, K), f32),
              "det_gt": ((B, A, T, K), i32), "det_iou": ((B, A, T, K), f64), "det_ignore": ((B, A, T, K), u8),
              "gt_counted": ((B, A, num_classes), i32), "pq_gt_per_class": ((B, num_classes), i32), "pq_gt": ((B, K), i32),
              "pq_iou": ((B, K), f64), "pq_fp": ((B, K), i32), "overflow": ((B,), i32)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    pairs, n_pairs = Guarded(B * N * 3, i32, name="pairs"), Guarded(B, i32, name="n_pairs")
    nws1 = lib.mu_instance_pairs_workspace_bytes(B, H, W, Mp, Mg)
    nws2 = lib.mu_coco_match_workspace_bytes(B, K)
    assert nws1 > 0 and nws1 % 4 == 0 and nws2 == B * K * 4
    ws1, ws2 = Guarded(nws1 // 4, i32, name="pair workspace"), Guarded(nws2 // 4, i32, name="match workspace")
    assert lib.mu_coco_match_supported(H, W, Mp, Mg, num_classes, K, max_det, T, A) == 0
    call("mu_instance_pairs", p_in["ids"], g_in["ids"], B, H, W, Mp, Mg, pairs, n_pairs, ws1, nws1)
    call("mu_coco_match", pairs, n_pairs, p_in["table"], p_in["score"], p_in["order"], p_in["count"], g_in["table"], g_in["count"],
         g_crowd, g_area, B, H, W, Mp, Mg, num_classes, K, max_det, thr.ctypes.data, T, rng.ctypes.data, A,
         *[outs[k] for k in OUT_KEYS], ws2, nws2)
    for g in (*p_in.values(), *g_in.values(), *outs.values(), pairs, n_pairs, ws1, ws2):
        g.check()
    for k in OUT_KEYS:                                        # every output byte is written (det_score 0.0, ids 0: never the sentinel)
        outs[k].all_written()
    return {k: outs[k].host(shapes[k][0]) for k in OUT_KEYS}


def run_case(case, **kw):
    return run_coco(case["pred"], case["gt"], case["num_classes"], case["crowd"], case["gt_area"], case["thresholds"],
                    case["area_ranges"], **kw)


def compare(got, ref):
    print(f"evaluated rows {got['det_valid'].sum(1).tolist()}, coco matches {(ref['det_gt'] > 0).sum()}, ignored "
          f"{int(ref['det_ignore'].sum())}, npig {ref['gt_counted'].sum((0, 2)).tolist()}, panoptic {(ref['pq_gt'] > 0).sum()}, "
          f"fp {ref['pq_fp'].sum()}")
    for k in OUT_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert got[k].tobytes() == ref[k].tobytes(), k        # fp64 IoUs included: one division each


@functools.lru_cache(maxsize=None)
def _hand():
    return C.hand_cases()


@functools.lru_cache(maxsize=None)
def _random(i):
    case = C.random_case(*C.RANDOM[i])
    return case, C.reference(case)[0]


def _with(case, **kw):
    return dict(case, **kw)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_cases(name):
    """the expectations are written out in tests/test_cocoeval_host.py"""
    case = _hand()[name]
    got = run_case(case)
    if name == "break_rule":
        assert got["det_gt"][0, 0, :, 0].tolist() == [1, 2, 2, 2, 2, 2, 0, 0, 0, 0]
        assert got["det_ignore"][0, 0, :, 0].tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0, 0]
        assert got["det_iou"][0, 0, :, 0].tolist() == [0.3] + [0.7] * 5 + [0.0] * 4
    if name == "pq_same_class":
        assert got["pq_fp"][0, :3].tolist() == [0, 0, 0] and got["pq_gt_per_class"][0].tolist() == [0, 1, 1]
    compare(got, C.reference(case)[0])


@pytest.mark.parametrize("i", range(len(C.RANDOM)), ids=[f"{r[1]}x{r[2]}" for r in C.RANDOM])
def test_random_ids_crowd_and_area_override(i):
    """B = 3, a third of the ground truths crowd, an annotated area on image 1, the four ranges scaled to the image, T = 10 from 0.30;
    test_cocoeval_host.py asserts that these seeds reach every counted branch of the restatement"""
    case, ref = _random(i)
    compare(run_case(case), ref)


@functools.lru_cache(maxsize=None)
def _squares(big_extra):
    """128 x 128, the default ranges with 32^2 and 96^2 themselves hit.  Ground truths: a 96 x 96 square (9216; + 1 pixel = 9217 when
    big_extra), and to its right three 32 x 32 squares: whole (1024), less a pixel (1023), plus a pixel (1025).  Both big areas cannot
    share one 16384-pixel id map with the rest, hence the two images, one per call.  Predictions: the same regions, the 1023 one
    grown back to 1024 (IoU 1023 / 1024), and a band of 8 x 128 = 1024 pixels on the background that matches nothing."""
    g = np.zeros((1, 128, 128), np.int32)
    g[0, :96, :96] = 1
    g[0, 0:32, 96:] = 2
    g[0, 32:64, 96:] = 3
    g[0, 32, 96] = 0
    g[0, 64:96, 96:] = 4
    g[0, 96, 96] = 4
    if big_extra:
        g[0, 96, 0] = 1
    p = g.copy()
    p[0, 32, 96] = 3
    p[0, 104:112, :] = 5
    pred = R.side_from_ids(p, [[1, 1, 1, 1, 1]], 8, [[0.9, 0.8, 0.7, 0.6, 0.5]])
    gt = R.side_from_ids(g, [[1, 1, 1, 1]], 8)
    return C.freeze({"pred": pred, "gt": gt, "crowd": None, "gt_area": None, "num_classes": 2, "thresholds": CR.COCO_THRESHOLDS,
                     "area_ranges": CR.COCO_AREA_RANGES})


@pytest.mark.parametrize("big_extra", [0, 1], ids=["9216", "9217"])
def test_default_ranges_at_their_edges(big_extra):
    case = _squares(big_extra)
    assert case["gt"]["table"][0, :4, 1].tolist() == [9216 + big_extra, 1024, 1023, 1025]
    assert case["pred"]["table"][0, :5, 1].tolist() == [9216 + big_extra, 1024, 1024, 1025, 1024]
    got = run_case(case)
    # all; small = 1023, 1024; medium = 1024, 1025 and 9216 but not 9217; large = 9216 / 9217
    assert got["gt_counted"][0, :, 1].tolist() == [4, 2, 3 - big_extra, 1]
    assert got["det_ignore"][0, :, 0, 4].tolist() == [0, 0, 0, 1]          # the unmatched band of 1024 pixels: small and medium
    compare(got, C.reference(case)[0])


# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _single_pixels(H, W, n, num_classes, seed):
    """n single-pixel ground truths on the first n pixels; the predictions are the same pixels numbered in another order, so every
    IoU is 1 or 0 and only the classes, the crowd flags and the order decide"""
    rng = np.random.default_rng(seed)
    g = np.zeros(H * W, np.int32)
    g[:n] = 1 + np.arange(n)
    p = np.zeros(H * W, np.int32)
    p[:n] = 1 + rng.permutation(n)
    gc = rng.integers(1, num_classes, n)
    pc = np.where(rng.random(n) < 0.7, gc[np.argsort(p[:n] - 1)], rng.integers(1, num_classes, n))
    crowd = (rng.random((1, n)) < 1 / 3).astype(np.int32)
    pred = R.side_from_ids(p.reshape(1, H, W), [pc], n, [rng.integers(1, 17, n) / 16.0])
    return C.freeze({"pred": pred, "gt": R.side_from_ids(g.reshape(1, H, W), [gc], n), "crowd": crowd, "gt_area": None,
                     "num_classes": num_classes, "thresholds": np.array([0.5, 1.0]), "area_ranges": [[0, 1e10], [2, 1e10]]})


@pytest.mark.parametrize("shape", [(20, 24, 300, 4), (33, 34, 1100, 21)], ids=["300", "1100"])
def test_more_rows_than_one_pass_of_the_threads(shape):
    """300 single-pixel instances on 20 x 24 (more than 256), and 1100 on 33 x 34 (more than the 1024 threads of the workgroup).  In the
    second range [2, 1e10] every ground truth and every detection is ignored"""
    case = _single_pixels(*shape, seed=shape[2])
    ref = C.reference(case, max_dets=(shape[2],))[0]            # no cut per class: every row is evaluated
    assert ref["det_valid"].sum() == shape[2] and (ref["det_gt"][0, 0] > 0).sum() > shape[2] // 2
    assert ref["det_ignore"][0, 1].all() and not ref["gt_counted"][0, 1].any()
    compare(run_case(case, max_det=shape[2]), ref)


@pytest.mark.parametrize("nc", [64, 65, 130])
def test_class_counts_across_the_scan_turns(nc):
    """as in test_gpu_match.py: 4 x 4 segments, the prediction one column to the right, classes 1, 63, 64 and the last one; every
    third ground truth crowd"""
    yy, xx = np.mgrid[0:16, 0:16]
    g = (1 + (yy // 4) * 4 + xx // 4)[None].astype(np.int32)
    p = np.roll(g, 1, axis=2)
    p[0, :, 0] = 0
    classes = np.array(sorted({c for c in (1, 63, 64, nc - 1) if c < nc}))
    cls = [classes[np.arange(16) % len(classes)]]
    pred, gt = R.side_from_ids(p, cls, 16, [((np.arange(16) * 5) % 8 + 1) / 8.0]), R.side_from_ids(g, cls, 16)
    crowd = (np.arange(16) % 3 == 0).astype(np.int32)[None]
    ref = CR.evaluate(pred, gt, nc, crowd, None, CR.REF_THRESHOLDS, CR.SMALL_AREA_RANGES)[0]
    assert ref["gt_counted"][0, 0, nc - 1] > 0 and ref["det_ignore"].any() and (ref["det_gt"][0, 0, 0] > 0).all()
    compare(run_coco(pred, gt, nc, crowd, None, CR.REF_THRESHOLDS, CR.SMALL_AREA_RANGES), ref)


def test_thirty_two_thresholds():
    """every bit of a matched[] word"""
    case = _with(_random(1)[0], thresholds=np.linspace(1 / 64, 1.0, 32))
    ref = C.reference(case)[0]
    assert (ref["det_gt"][:, 0, 0] > 0).sum() > (ref["det_gt"][:, 0, 31] > 0).sum() > 0
    compare(run_case(case), ref)


@pytest.mark.parametrize("A", [1, 2, 3])
def test_fewer_area_ranges(A):
    """A = 4 is what every other test runs; the first A ranges give the first A slices of the same results"""
    case, full = _random(0)
    got = run_case(_with(case, area_ranges=CR.SMALL_AREA_RANGES[:A]))
    ref = C.reference(_with(case, area_ranges=CR.SMALL_AREA_RANGES[:A]))[0]
    compare(got, ref)
    assert np.array_equal(got["det_gt"], full["det_gt"][:, :A]) and np.array_equal(got["gt_counted"], full["gt_counted"][:, :A])


@functools.lru_cache(maxsize=None)
def _twelve():
    """2 x 24: twelve ground truths of two pixels, class 1; twelve detections of class 1, the even ones cover their ground truth (IoU 1),
    the odd ones half of it (IoU 1/2); scores descend with the id; ground truth 5 is crowd"""
    g = np.repeat(1 + np.arange(12), 2).astype(np.int32)
    p = g.copy()
    p[np.arange(12)[1::2] * 2 + 1] = 0
    crowd = np.zeros((1, 16), np.int32)
    crowd[0, 4] = 1
    pred = R.side_from_ids(p.reshape(1, 2, 12), [[1] * 12], 16, [[(32 - k) / 32.0 for k in range(12)]])
    gt = R.side_from_ids(g.reshape(1, 2, 12), [[1] * 12], 16)
    return C.freeze({"pred": pred, "gt": gt, "crowd": crowd, "gt_area": None, "num_classes": 2, "thresholds": CR.COCO_THRESHOLDS,
                     "area_ranges": CR.SMALL_AREA_RANGES})


def test_twelve_detections_of_one_class_and_the_max_dets_ladder():
    """the ranks 1, 10 and 100 all cut: det_rank from the kernel, the ladder in CocoEval; and the cut of the kernel itself at 10"""
    import maskunet_amd
    case = _twelve()
    ref = C.reference(case)[0]
    got = run_case(case)
    assert got["det_rank"][0, :12].tolist() == list(range(12))
    compare(got, ref)
    acc = maskunet_amd.CocoEval(2, case["thresholds"], case["area_ranges"])
    acc.update(maskunet_amd.CocoMatches(*[torch.from_numpy(got[k]) for k in OUT_KEYS]))
    out, want = acc.compute(), CR.accumulate([ref], 2, case["thresholds"], case["area_ranges"])
    assert np.array_equal(out["precision"], want["precision"]) and np.array_equal(out["recall"], want["recall"])
    ar = out["stats"][6:9]
    print(out["stats"].tolist())
    assert 0 < ar[0] < ar[1] < ar[2] and np.abs(out["stats"] - CR.summarize(want, case["thresholds"])).max() <= 1e-12
    cut = run_case(case, max_det=10)
    assert cut["det_valid"][0].sum() == 10
    compare(cut, C.reference(case, max_dets=(1, 10))[0])
    compare(run_case(case, max_queries=7), C.reference(case, max_queries=7)[0])


# ------------------------------------------------------------------------------------------------
def test_empty_sides_and_all_crowd():
    case, _ = _random(0)
    zero = lambda s: {k: np.zeros_like(v) for k, v in s.items()}
    for kw in (dict(pred=zero(case["pred"])), dict(gt=zero(case["gt"])), dict(pred=zero(case["pred"]), gt=zero(case["gt"])),
               dict(crowd=np.ones_like(case["crowd"]))):
        c = _with(case, **kw)
        ref = C.reference(c)[0]
        got = run_case(c)
        compare(got, ref)
        if "crowd" in kw:
            assert not got["gt_counted"].any() and not got["pq_gt_per_class"].any() and not got["pq_gt"].any()
            assert got["det_valid"].any() and (got["det_gt"] > 0).any() and (got["det_ignore"][got["det_gt"] > 0] == 1).all()
        else:
            assert not got["det_gt"].any() and not got["pq_gt"].any()


def test_more_instances_than_rows_sets_overflow_and_compute_raises():
    import maskunet_amd
    case, ref = _random(1)
    one = {k: v.copy() for k, v in case["pred"].items()}
    one["count"][1] = 65                                     # one image over, the others are untouched
    got = run_case(_with(case, pred=one))
    assert got["overflow"].tolist() == [0, 1, 0]
    for k in OUT_KEYS[:12]:
        assert np.array_equal(got[k][[0, 2]], ref[k][[0, 2]]), k
    acc = maskunet_amd.CocoEval(case["num_classes"], case["thresholds"], case["area_ranges"])
    acc.update(maskunet_amd.CocoMatches(*[torch.from_numpy(got[k]) for k in OUT_KEYS]))
    with pytest.raises(RuntimeError, match="max_instances"):
        acc.compute()


def test_two_runs_are_bit_identical():
    for case in (_random(1)[0], _single_pixels(20, 24, 300, 4, seed=300)):
        a, b = run_case(case, max_det=300), run_case(case, max_det=300)
        for k in OUT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------
def _instances(side):
    from maskunet_amd import Instances
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in side.items()}
    return Instances(classes=torch.zeros_like(t["ids"]), ids=t["ids"], table=t["table"], scores=t["score"], count=t["count"], order=t["order"])


def test_without_crowd_and_ranges_it_is_match_instances():
    """crowd=None, one range [0, 1e10], max_dets=(100,): the parent's match_instances / InstanceAP are the yardstick"""
    import maskunet_amd
    ap_old, ap_new = maskunet_amd.InstanceAP(5, CR.REF_THRESHOLDS), maskunet_amd.CocoEval(5, CR.REF_THRESHOLDS, [[0, 1e10]], (100,))
    for seed, (H, W) in ((27, (20, 24)), (20, (13, 9))):
        pred, gt = R.random_case(seed, 3, H, W, 5)
        pi, gi = _instances(pred), _instances(gt)
        old = maskunet_amd.match_instances(pi, gi, 5, CR.REF_THRESHOLDS, max_queries=40)
        new = maskunet_amd.coco_match(pi, gi, 5, iou_thresholds=CR.REF_THRESHOLDS, area_ranges=[[0, 1e10]], max_queries=40,
                                      max_dets=(100,))
        assert (old.det_gt > 0).any() and (old.pq_gt > 0).any() and bool(old.pq_fp.any())
        for k in ("det_valid", "det_class", "det_score", "pq_gt", "pq_iou", "pq_fp", "overflow", "pairs", "n_pairs"):
            assert torch.equal(getattr(new, k), getattr(old, k)), k
        assert torch.equal(new.det_gt[:, 0], old.det_gt) and torch.equal(new.det_iou[:, 0], old.det_iou)
        assert torch.equal(new.pq_gt_per_class, old.gt_per_class) and torch.equal(new.gt_counted[:, 0], old.gt_per_class)
        assert not bool(new.det_ignore.any())
        ap_old.update(old)
        ap_new.update(new)
    a, b = ap_old.compute(), ap_new.compute()
    print(a["ap"], b["stats"].tolist())
    assert 0 < a["ap"] < 1 and b["stats"][0] == a["ap"]
    assert np.array_equal(b["precision"][:, :, :, 0, 0], a["precision"])


def test_end_to_end_two_updates():
    """predict_instances -> coco_match -> CocoEval, PanopticQuality against the restatement fed with to_reference() lists and masks"""
    import maskunet_amd
    from tests import _cc_reference as CC
    B, C_, H, W, Q = 2, 5, 32, 32, 40
    rng = np.random.default_rng(12)
    thr, ranges = CR.REF_THRESHOLDS, [[0, 1e10], [0, 16], [16, 64], [64, 1e10]]
    acc, acc_pq = maskunet_amd.CocoEval(C_, thr, ranges), maskunet_amd.PanopticQuality(C_)
    refs = []
    for step in range(2):
        labels = np.stack([CC.blocky(rng, H, W, C_, 8) for _ in range(B)])
        logits = 3.0 * np.eye(C_)[np.roll(labels, 1, axis=2)].transpose(0, 3, 1, 2) + rng.standard_normal((B, C_, H, W))
        logits = (logits + np.roll(logits, 1, 2) + np.roll(logits, 1, 3) + np.roll(logits, -1, 2) + np.roll(logits, -1, 3)) / 5
        pred = maskunet_amd.predict_instances(torch.from_numpy(logits.astype(np.float32)).to(DEV), max_instances=256)
        gt = maskunet_amd.instances_from_labels(torch.from_numpy(labels).long().to(DEV), max_instances=256)
        crowd = rng.random((B, 256)) < 0.25
        area = np.round(rng.random((B, 256)) * 100, 1)
        m = maskunet_amd.coco_match(pred, gt, C_, crowd=torch.from_numpy(crowd).to(DEV), gt_area=torch.from_numpy(area).float().to(DEV),
                                    iou_thresholds=thr, area_ranges=ranges, max_queries=Q)
        acc.update(m)
        acc_pq.update(m)
        area32 = area.astype(np.float32).astype(np.float64)          # what the call was given
        per = []
        for b in range(B):                                   # the restatement on the lists that Instances.to_reference() hands out
            dets = [dict(d, score=np.float32(d["score"])) if 1 <= d["category_id"] < C_ else None for d in pred.to_reference(b, Q)]
            dets += [None] * (Q - len(dets))
            gts = [dict(g, id=k + 1, iscrowd=bool(crowd[b, k]), area=float(area32[b, k]))
                   for k, g in enumerate(gt.to_reference(b)) if 1 <= g["category_id"] < C_]
            void = np.ones((H, W), bool)
            for g in gts:
                void &= ~g["mask"]
            per.append(CR.evaluate_image(dets, gts, void, C_, thr, ranges, 100)[0])
        ref = {k: np.stack([p[k] for p in per]) for k in per[0]}
        ref["overflow"] = np.zeros(B, np.int32)
        compare({k: getattr(m, k).cpu().numpy() for k in OUT_KEYS}, ref)
        side, cnt = CR.evaluate(side_of(pred), side_of(gt), C_, crowd, area32, thr, ranges, max_queries=Q)
        compare(ref, side)
        assert cnt["matched_ignored"] > 0 and cnt["unmatched_by_area"] > 0
        refs.append(ref)
    assert sum(int((r["pq_gt"] > 0).sum()) for r in refs) >= 2
    got, want = acc.compute(), CR.accumulate(refs, C_, thr, ranges)
    assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])
    stats = CR.summarize(want, thr)
    print(got["stats"].tolist(), acc.summarize()[0])
    assert (stats[[0, 6, 7, 8]] > 0).all() and np.abs(got["stats"] - stats).max() <= 1e-12
    pq, want = acc_pq.compute(), CR.accumulate_pq(refs, C_)
    for k in ("tp", "fp", "fn"):
        assert np.array_equal(pq[k], want[k]), k
    n = int(want["tp"].sum()) + C_
    for k in ("pq", "sq", "rq"):
        print(f"All {k} {pq['All'][k]!r} reference {want['All'][k]!r}")
        assert 0 < want["All"][k] and abs(pq["All"][k] - want["All"][k]) <= n * 2.0 ** -53 * want["All"][k]


def test_refusals_launch_nothing(monkeypatch):
    import maskunet_amd
    from maskunet_amd import matching
    pred, gt = R.random_case(27, 2, 13, 9, 5)
    pi, gi = _instances(pred), _instances(gt)
    launched = []
    monkeypatch.setattr(matching, "call", lambda name, *a: launched.append(name))
    crowd = torch.zeros((2, 64), dtype=torch.bool, device=DEV)
    for exc, kw in ((ValueError, dict(area_ranges=[[0, 1]] * 5)), (ValueError, dict(iou_thresholds=np.linspace(0.1, 1, 33))),
                    (ValueError, dict(iou_thresholds=[0.0, 0.5])), (ValueError, dict(area_ranges=[[0, 1e10], [9, 4]])),
                    (ValueError, dict(area_ranges=[[0, float("nan")]])), (ValueError, dict(max_dets=(10, 1))),
                    (RuntimeError, dict(crowd=crowd.cpu())), (RuntimeError, dict(crowd=crowd[:, :63])),
                    (RuntimeError, dict(gt_area=torch.zeros((2, 64), dtype=torch.float64))), (TypeError, dict(gt_area=crowd)),
                    (TypeError, dict(crowd=crowd.float())), (RuntimeError, dict(max_queries=0))):
        with pytest.raises(exc):
            maskunet_amd.coco_match(pi, gi, 5, **kw)
    cpu = maskunet_amd.Instances(*[getattr(pi, f).cpu() for f in ("classes", "ids", "table", "scores", "count", "order")])
    with pytest.raises(RuntimeError, match="GPU"):
        maskunet_amd.coco_match(cpu, gi, 5)
    with pytest.raises(RuntimeError, match="1024"):
        maskunet_amd.coco_match(pi, gi, 2000)
    assert launched == []
    maskunet_amd.coco_match(pi, gi, 5, crowd=crowd)
    assert launched == ["mu_instance_pairs", "mu_coco_match"]
