"""GPU: the pair table and the COCO / panoptic matching (mu_instance_pairs, mu_instance_match, maskunet_amd.match_instances) against the
naive restatement of the contract in tests/_match_reference.py.  Every integer output is compared with ==, and so are det_iou / pq_iou:
each is ONE correctly rounded fp64 division of the same two integers on both sides.  Only iou_sum and the means of the accumulators
carry a bound, the summation-order bound n * 2^-53 relative.  Raw id maps and reference-built tables go through the C ABI, so regions are
arbitrary.  Memory discipline as in test_gpu_instances.py: outputs pre-filled with a sentinel, the workspace exactly the queried size,
4 KiB guard bands around every buffer, inputs verified untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import _match_reference as R
from tests._device_buffers import Guarded, call, side_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -53
OUT_KEYS = ("det_valid", "det_class", "det_score", "det_gt", "det_iou", "gt_per_class", "pq_gt", "pq_iou", "pq_fp", "overflow",
            "pairs", "n_pairs")


def run_match(pred, gt, num_classes, thresholds=None, max_queries=None, max_dets=100):
    """raw mu_instance_pairs + mu_instance_match on two sides (dicts of numpy arrays) -> dict of numpy outputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    thr = np.ascontiguousarray(R.DEFAULT_THRESHOLDS if thresholds is None else thresholds, np.float64)
    B, H, W = pred["ids"].shape
    Mp, Mg, T, N = pred["table"].shape[1], gt["table"].shape[1], len(thr), H * W
    K = Mp if max_queries is None else min(max_queries, Mp)
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    sizes = {"ids": (B * N, i32), "table": (B * Mp * 8, i32), "score": (B * Mp, f32), "order": (B * Mp, i32), "count": (B, i32)}
    p_in = {k: Guarded(n, d, pred[k], "pred " + k) for k, (n, d) in sizes.items()}
    g_in = {k: Guarded(n, i32, gt[k], "gt " + k) for k, n in (("ids", B * N), ("table", B * Mg * 8), ("count", B))}
    shapes = {"det_valid": ((B, K), i32), "det_class": ((B, K), i32), "det_score": ((B, K), f32), "det_gt": ((B, T, K), i32),
              "det_iou": ((B, T, K), f64), "gt_per_class": ((B, num_classes), i32), "pq_gt": ((B, K), i32), "pq_iou": ((B, K), f64),
              "pq_fp": ((B, K), i32), "overflow": ((B,), i32), "pairs": ((B, N, 3), i32), "n_pairs": ((B,), i32)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    nws1 = lib.mu_instance_pairs_workspace_bytes(B, H, W, Mp, Mg)
    nws2 = lib.mu_instance_match_workspace_bytes(B, K)
    assert nws1 > 0 and nws1 % 4 == 0 and nws2 == B * K * 4
    ws1, ws2 = Guarded(nws1 // 4, i32, name="pair workspace"), Guarded(nws2 // 4, i32, name="match workspace")
    assert lib.mu_instance_match_supported(H, W, Mp, Mg, num_classes, K, max_dets, T) == 0
    call("mu_instance_pairs", p_in["ids"], g_in["ids"], B, H, W, Mp, Mg, outs["pairs"], outs["n_pairs"], ws1, nws1)
    call("mu_instance_match", outs["pairs"], outs["n_pairs"], p_in["table"], p_in["score"], p_in["order"], p_in["count"], g_in["table"],
         g_in["count"], B, H, W, Mp, Mg, num_classes, K, max_dets, thr.ctypes.data, T, *[outs[k] for k in OUT_KEYS[:10]], ws2, nws2)
    for g in (*p_in.values(), *g_in.values(), *outs.values(), ws1, ws2):       # and every buffer again after the second launch
        g.check()
    return {k: outs[k].host(shapes[k][0]) for k in OUT_KEYS}


def compare(got, ref):
    print(f"pairs {got['n_pairs'].tolist()} (reference {ref['n_pairs'].tolist()}); evaluated rows {got['det_valid'].sum(1).tolist()}, "
          f"coco matches {(ref['det_gt'] > 0).sum()}, panoptic {(ref['pq_gt'] > 0).sum()}, fp {ref['pq_fp'].sum()}")
    for k in OUT_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), k          # fp64 IoUs included: one division each


def same(a, b):
    for k in OUT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def frozen(*sides):
    for s in sides:
        for v in s.values():
            v.setflags(write=False)
    return sides


@functools.lru_cache(maxsize=None)
def _random(seed, B, H, W, C, max_inst=64):
    return frozen(*R.random_case(seed, B, H, W, C, max_inst=max_inst))


@functools.lru_cache(maxsize=None)
def _hand():
    return frozen(*R.hand_case())


# ------------------------------------------------------------------------------------------------
def test_hand_cases_ten_thresholds():
    """the exact IoUs 1/2, 3/4, 9/10, 19/20 at their own thresholds, the equal-IoU tie, the score tie, the void-majority drop:
    expectations written out in tests/test_match_host.py"""
    pred, gt = _hand()
    got = run_match(pred, gt, 4)
    assert (got["det_gt"][0] > 0).sum(0)[:8].tolist() == [1, 6, 9, 10, 1, 1, 0, 0]
    assert got["det_gt"][0, 0, :8].tolist() == [1, 2, 3, 4, 6, 7, 0, 0]
    assert got["det_iou"][0, 0, :6].tolist() == [5 / 10, 6 / 8, 9 / 10, 19 / 20, 2 / 4, 3 / 6]
    assert got["pq_gt"][0, :8].tolist() == [0, 2, 3, 4, 0, 0, 0, 0] and got["pq_fp"][0, :8].tolist() == [1, 0, 0, 0, 1, 1, 1, 0]
    compare(got, R.match(pred, gt, 4))


@pytest.mark.parametrize("shape", [(13, 9), (20, 24)])
def test_random_ids_odd_sizes_three_images(shape):
    pred, gt = _random(7 + shape[0], 3, *shape, 5)
    ref = R.match(pred, gt, 5)
    assert len(set(ref["n_pairs"].tolist())) == 3 and (ref["pq_gt"] > 0).any() and ref["pq_fp"].any()
    compare(run_match(pred, gt, 5), ref)


@functools.lru_cache(maxsize=None)
def _strips(H, W, ph, pw, gh, gw, C):
    """pred segments of ph x pw against gt segments of gh x gw; classes cycle so that every class holds a few of each"""
    yy, xx = np.mgrid[0:H, 0:W]
    p = (1 + (yy // ph) * (W // pw) + xx // pw)[None].astype(np.int32)
    g = (1 + (yy // gh) * (W // gw) + xx // gw)[None].astype(np.int32)
    n_p, n_g = int(p.max()), int(g.max())
    pc = [1 + (np.arange(n_p) * 7) % (C - 1)]
    gc = [1 + (np.arange(n_g) * 5) % (C - 1)]
    sc = [((np.arange(n_p) * 37) % 64 + 1) / 64.0]
    return frozen(R.side_from_ids(p, pc, n_p, sc), R.side_from_ids(g, gc, n_g))


def test_rows_against_columns_every_pixel_its_own_pair():
    pred, gt = _strips(64, 64, 1, 64, 64, 1, 9)
    ref = R.match(pred, gt, 9)
    assert ref["n_pairs"].tolist() == [4096] and (ref["pairs"][0, :, 2] == 1).all()
    compare(run_match(pred, gt, 9), ref)


def test_capacity_65536_pairs():
    """256 x 256: 4096 pred segments of 1 x 16 against 4096 gt segments of 16 x 1 -- 16 pairs of one pixel each per segment, H*W pairs"""
    pred, gt = _strips(256, 256, 1, 16, 16, 1, 1024)
    pairs, n_pairs = R.pair_table(pred["ids"], gt["ids"], 4096, 4096)
    assert n_pairs.tolist() == [65536] and (pairs[0, :, 2] == 1).all()
    got = run_match(pred, gt, 1024, thresholds=[0.05, 0.5], max_queries=4096)
    assert np.array_equal(got["n_pairs"], n_pairs) and np.array_equal(got["pairs"], pairs)
    # every IoU is 1 / 31: written out instead of 4096 x 4 mask intersections.  At 0.05 > 1/31 nothing matches
    assert got["det_valid"].all() and got["overflow"].tolist() == [0] and not got["det_gt"].any() and not got["pq_gt"].any()
    assert got["pq_fp"].all() and got["gt_per_class"][0, 1:].sum() == 4096
    assert np.array_equal(got["det_class"][0], pred["table"][0, pred["order"][0] - 1, 0])
    low = run_match(pred, gt, 1024, thresholds=[1 / 31], max_queries=4096)
    assert np.array_equal(low["pairs"], pairs)
    hit = low["det_gt"][0, 0] > 0
    assert hit.any() and (low["det_iou"][0, 0][hit] == 1 / 31).all()
    p_of = pred["order"][0][hit]
    assert (pred["table"][0, p_of - 1, 0] == gt["table"][0, low["det_gt"][0, 0][hit] - 1, 0]).all()
    assert len(set(low["det_gt"][0, 0][hit].tolist())) == hit.sum()          # a ground truth is matched once


# edges of the shared wave / workgroup helpers (csrc/wave_prims.h), as in test_gpu_instances.py
EDGE_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (7, 73), (16, 32), (19, 27), (31, 33), (32, 32), (25, 41)]


@functools.lru_cache(maxsize=None)
def _edge_sides(H, W, C):
    """runs of three pixels along the raster, the prediction one pixel behind the ground truth.  Image 0: foreground forced on the last
    pixel and on the first pixel of the last wave's segment (16 waves, 64-pixel chunks), on both sides; image 1: an id of their own there"""
    N = H * W
    seg = -(-N // 1024) * 64
    edge = [(N - 1) // seg * seg, N - 1]
    rng = np.random.default_rng(N)
    raw = np.repeat(rng.integers(0, 6, (2, 2, -(-N // 3) + 1)), 3, axis=2)          # [side, image, pixel]
    raw = np.stack([raw[0, :, 1:N + 1], raw[1, :, :N]])
    raw[:, 0, edge] = np.maximum(raw[:, 0, edge], 1)
    raw[:, 1, edge] = 7
    sides = []
    for s in range(2):
        ids = R.compact(raw[s].reshape(2, H, W))
        n = [int(ids[b].max()) for b in range(2)]
        cls = [1 + (np.arange(k) * (3 + 2 * s)) % (C - 1) for k in n]
        sc = [((np.arange(k) * 37) % 64 + 1) / 64.0 for k in n]
        sides.append(R.side_from_ids(ids, cls, 8, sc if s == 0 else None))
    return frozen(*sides)


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixel_counts_at_chunk_and_segment_edges(shape):
    pred, gt = _edge_sides(*shape, 4)
    last = shape[0] * shape[1] - 1
    assert pred["ids"].reshape(2, -1)[:, last].all() and gt["ids"].reshape(2, -1)[:, last].all()
    ref = R.match(pred, gt, 4)
    assert ref["n_pairs"].min() >= 1
    compare(run_match(pred, gt, 4), ref)


@pytest.mark.parametrize("nc", [64, 65, 130])
def test_class_counts_across_the_scan_turns(nc):
    """the per-class starts are scanned 64 classes per turn: evaluated rows in classes 1, 63, 64 (where it exists) and the last one;
    4 x 4 segments, the prediction one column to the right: IoU 12 / 20 with the segment of the same class"""
    yy, xx = np.mgrid[0:16, 0:16]
    g = (1 + (yy // 4) * 4 + xx // 4)[None].astype(np.int32)
    p = np.roll(g, 1, axis=2)
    p[0, :, 0] = 0
    classes = np.array(sorted({c for c in (1, 63, 64, nc - 1) if c < nc}))
    cls = [classes[np.arange(16) % len(classes)]]
    pred, gt = R.side_from_ids(p, cls, 16, [((np.arange(16) * 5) % 8 + 1) / 8.0]), R.side_from_ids(g, cls, 16)
    ref = R.match(pred, gt, nc)
    assert set(ref["det_class"][0].tolist()) == set(classes.tolist()) and (ref["det_gt"][0, 0] > 0).all()
    assert ref["gt_per_class"][0, nc - 1] > 0
    compare(run_match(pred, gt, nc), ref)


def test_disconnected_regions_and_classes_outside_the_range():
    """random_case draws scattered regions and classes from 0..num_classes: class 0 and class num_classes take part on neither side,
    and the pixels of such ground truths are void"""
    pred, gt = _random(3, 2, 16, 16, 4)
    for s in (pred, gt):
        cls = s["table"][:, :, 0]
        assert (cls == 4).any() and ((cls == 0) & (s["table"][:, :, 1] > 0)).any()
    ref = R.match(pred, gt, 4)
    assert (ref["det_valid"] == 0).any() and ref["det_valid"].any()
    got = run_match(pred, gt, 4)
    compare(got, ref)
    drop = {k: v.copy() for k, v in gt.items()}                      # the same with those ground truths erased from the id map
    out = (gt["table"][:, :, 0] < 1) | (gt["table"][:, :, 0] >= 4)
    for b in range(2):
        drop["ids"][b][np.isin(gt["ids"][b], 1 + np.flatnonzero(out[b]))] = 0
    erased = run_match(pred, drop, 4)
    for k in OUT_KEYS[:10]:
        assert np.array_equal(erased[k], got[k]), k


def test_empty_sides():
    pred, gt = _random(5, 2, 13, 9, 5)
    zero = lambda s: {"ids": np.zeros_like(s["ids"]), "count": np.zeros_like(s["count"]), "table": np.zeros_like(s["table"]),
                      "score": np.zeros_like(s["score"]), "order": np.zeros_like(s["order"])}
    for p, g in ((zero(pred), gt), (pred, zero(gt)), (zero(pred), zero(gt))):
        ref = R.match(p, g, 5)
        got = run_match(p, g, 5)
        compare(got, ref)
        assert not got["det_gt"].any() and not got["pq_gt"].any()
    assert R.match(pred, zero(gt), 5)["pq_fp"].sum() == 0            # everything lies on void
    assert R.match(pred, zero(gt), 5)["n_pairs"].sum() > 0


@pytest.mark.parametrize("kw", [dict(max_queries=6), dict(max_dets=2), dict(max_queries=9, max_dets=2), dict(thresholds=[0.5]),
                                dict(thresholds=np.linspace(1 / 64, 1.0, 32)), dict(thresholds=[1.0, 0.25, 0.75])],
                         ids=["max_queries", "max_dets", "both", "T1", "T32", "unsorted_T3"])
def test_truncation_and_threshold_counts(kw):
    pred, gt = _random(27, 3, 20, 24, 5)
    ref = R.match(pred, gt, 5, **kw)
    full = R.match(pred, gt, 5, thresholds=kw.get("thresholds"))
    if "max_dets" in kw or "max_queries" in kw:
        K = ref["det_valid"].shape[1]
        assert not np.array_equal(ref["det_valid"], full["det_valid"][:, :K]) or K < pred["count"].max()
    compare(run_match(pred, gt, 5, **kw), ref)


def test_hand_case_cut_through_a_class():
    pred, gt = _hand()
    compare(run_match(pred, gt, 4, max_queries=6), R.match(pred, gt, 4, max_queries=6))
    compare(run_match(pred, gt, 4, max_dets=1, thresholds=[np.nextafter(0.5, 1)]),
            R.match(pred, gt, 4, max_dets=1, thresholds=[np.nextafter(0.5, 1)]))


def test_more_instances_than_rows_sets_overflow():
    """results of such an image are unspecified; the flag is set and nothing is written out of bounds (run_match checks the guards)"""
    big_p, big_g = R.random_case(9, 3, 20, 24, 5, max_inst=64)
    assert big_p["count"].min() > 4 and big_g["count"].min() > 3
    small_p, small_g = R.random_case(9, 3, 20, 24, 5, max_inst=4)
    small_g3 = {k: (v[:, :3] if k in ("table", "score", "order") else v) for k, v in big_g.items()}
    assert run_match(small_p, big_g, 5)["overflow"].tolist() == [1, 1, 1]
    assert run_match(big_p, small_g3, 5)["overflow"].tolist() == [1, 1, 1]
    got = run_match(small_p, small_g, 5)
    assert got["overflow"].tolist() == [1, 1, 1]
    assert got["pairs"][:, :, 0].max() <= 4 and got["pairs"][:, :, 1].max() <= 4            # ids past the tables are folded to 0
    assert np.array_equal(got["pairs"], R.pair_table(small_p["ids"], small_g["ids"], 4, 4)[0])
    one = {k: v.copy() for k, v in big_p.items()}
    one["count"][1] = 65                                     # one image over, the others are untouched
    got = run_match(one, big_g, 5)
    assert got["overflow"].tolist() == [0, 1, 0]
    ref = R.match(big_p, big_g, 5)
    for k in OUT_KEYS[:9]:
        assert np.array_equal(got[k][[0, 2]], ref[k][[0, 2]]), k


def test_two_runs_are_bit_identical():
    pred, gt = _random(27, 3, 20, 24, 5)
    a = run_match(pred, gt, 5)
    same(a, run_match(pred, gt, 5))
    pred, gt = _strips(64, 64, 1, 64, 64, 1, 9)
    same(run_match(pred, gt, 9), run_match(pred, gt, 9))


# ------------------------------------------------------------------------------------------------
def _match_on_reference_lists(pred, gt, num_classes, max_queries, max_dets):
    """the restatement on the masks, categories and scores that Instances.to_reference() hands out"""
    B = pred.ids.shape[0]
    per = []
    for b in range(B):
        dets = [d if 1 <= d["category_id"] < num_classes else None for d in pred.to_reference(b, max_queries)]
        for d in dets:
            if d is not None:
                d["score"] = np.float32(d["score"])
        dets += [None] * (max_queries - len(dets))
        gts = [dict(g, id=k + 1) for k, g in enumerate(gt.to_reference(b)) if 1 <= g["category_id"] < num_classes]
        void = np.ones(tuple(pred.ids.shape[1:]), bool)
        for g in gts:
            void &= ~g["mask"]
        per.append(R.match_image(dets, gts, void, num_classes, R.DEFAULT_THRESHOLDS, max_dets))
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def test_end_to_end_two_updates():
    import maskunet_amd
    from tests import _cc_reference as CC
    B, C, H, W, Q = 2, 5, 32, 32, 40
    rng = np.random.default_rng(12)
    acc_ap, acc_pq = maskunet_amd.InstanceAP(C), maskunet_amd.PanopticQuality(C, things=[False, True, True, False, False])
    refs = []
    for step in range(2):
        labels = np.stack([CC.blocky(rng, H, W, C, 8) for _ in range(B)])
        # smooth logits around the labels: the arg-max follows them except near the block borders
        logits = 3.0 * np.eye(C)[np.roll(labels, 1, axis=2)].transpose(0, 3, 1, 2) + rng.standard_normal((B, C, H, W))
        logits = (logits + np.roll(logits, 1, 2) + np.roll(logits, 1, 3) + np.roll(logits, -1, 2) + np.roll(logits, -1, 3)) / 5
        pred = maskunet_amd.predict_instances(torch.from_numpy(logits.astype(np.float32)).to(DEV), max_instances=256)
        gt = maskunet_amd.instances_from_labels(torch.from_numpy(labels).long().to(DEV), max_instances=256)
        m = maskunet_amd.match_instances(pred, gt, C, max_queries=Q)
        acc_ap.update(m)
        acc_pq.update(m)
        assert not bool(m.overflow.any())
        ref = R.match(side_of(pred), side_of(gt), C, max_queries=Q)
        got = {k: getattr(m, k).cpu().numpy() for k in OUT_KEYS}
        compare(got, ref)
        lists = _match_on_reference_lists(pred, gt, C, Q, 100)
        for k in lists:
            assert np.array_equal(lists[k], ref[k]), k
        assert (ref["pq_gt"] > 0).sum() >= 4
        refs.append(ref)
    ap, want = acc_ap.compute(), R.accumulate_ap(refs, C)
    assert np.array_equal(ap["precision"], want["precision"])
    n = int((want["precision"] > -1).sum())
    print(f"ap {ap['ap']!r} reference {want['ap']!r}")
    assert 0 < want["ap"] < 1 and abs(ap["ap"] - want["ap"]) <= n * EPS * want["ap"]
    pq, want = acc_pq.compute(), R.accumulate_pq(refs, C, [False, True, True, False, False])
    for k in ("tp", "fp", "fn"):
        assert np.array_equal(pq[k], want[k]), k
    for c in range(C):
        n = max(int(want["tp"][c]), 1)
        for k in ("iou_sum", "pq", "sq", "rq"):
            assert abs(pq[k][c] - want[k][c]) <= n * EPS * abs(want[k][c]), (k, c)
    for name in ("All", "Things", "Stuff"):
        n = want[name]["n"] + int(want["tp"].max())
        for k in ("pq", "sq", "rq"):
            print(f"{name} {k} {pq[name][k]!r} reference {want[name][k]!r}")
            assert abs(pq[name][k] - want[name][k]) <= n * EPS * abs(want[name][k])
    with pytest.raises(RuntimeError, match="4096"):
        maskunet_amd.match_instances(pred, gt, 2000)
