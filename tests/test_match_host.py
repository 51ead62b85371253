"""CPU: the instance-matching contract's numpy restatement (tests/_match_reference.py) against cases worked out by hand below, the
host-side accumulators of maskunet_amd.matching (InstanceAP, PanopticQuality) against the restatement's accumulate on CPU tensors, and
the host-only parts of the C ABI: shape queries and the error codes that must come back before any launch.  No GPU calls."""
import numpy as np
import pytest
import torch

from tests import _match_reference as R

MU_OK, MU_ERR_ARG, MU_ERR_SHAPE, MU_ERR_WORKSPACE = 0, -1, -2, -4
EPS = 2.0 ** -53


def test_hand_case_coco():
    """R.hand_case(): every prediction lies inside its ground truth, so iou = area_pred / area_gt:
         pred 1: 5/10 = 1/2   pred 2: 6/8 = 3/4   pred 3: 9/10   pred 4: 19/20   (class 1)
         pred 5 (4 px) covers gt 5 and gt 6 (2 px each): 2/4 with both -- the equal-IoU tie, the later gt (6) wins
         pred 6, 7 (3 px each, score 0.5 both) lie in gt 7 (6 px): 3/6 each -- the score tie, the lower id (6) goes first and takes it
         pred 8 lies on no ground truth.
       Each of 1/2, 3/4, 9/10, 19/20 passes its own threshold of linspace(0.5, 0.95, 10) (the ninth is 0.8999999999999999)."""
    pred, gt = R.hand_case()
    thr = np.linspace(0.5, 0.95, 10)
    assert thr[8] == 0.8999999999999999 and thr[5] == 0.75 and thr[9] == 0.95
    r = R.match(pred, gt, 4)
    assert pred["order"][0, :8].tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    want = np.zeros((10, 16), np.int32)
    want[:1, 0] = 1                   # 1/2: the first threshold only
    want[:6, 1] = 2                   # 3/4: 0.5 .. 0.75
    want[:9, 2] = 3                   # 9/10: 0.5 .. 0.9
    want[:10, 3] = 4                  # 19/20: all ten
    want[:1, 4] = 6                   # the tie goes to the later gt
    want[:1, 5] = 7                   # the first of two equal scores
    assert np.array_equal(r["det_gt"][0], want)
    assert r["det_iou"][0, 0, :6].tolist() == [5 / 10, 6 / 8, 9 / 10, 19 / 20, 2 / 4, 3 / 6]
    assert r["det_iou"][0, 9].tolist() == [0, 0, 0, 19 / 20] + [0] * 12
    assert r["det_valid"][0].tolist() == [1] * 8 + [0] * 8 and r["det_class"][0, :8].tolist() == [1, 1, 1, 1, 2, 3, 3, 3]
    assert r["det_score"][0, :8].tolist() == [float(np.float32(s)) for s in (0.9, 0.8, 0.7, 0.6, 0.55, 0.5, 0.5, 0.4)]
    assert r["gt_per_class"][0].tolist() == [0, 4, 2, 1] and r["overflow"].tolist() == [0]
    assert r["n_pairs"].tolist() == [9]
    assert r["pairs"][0, :9].tolist() == [[1, 1, 5], [2, 2, 6], [3, 3, 9], [4, 4, 19], [5, 5, 2], [5, 6, 2], [6, 7, 3], [7, 7, 3],
                                          [8, 0, 4]]
    assert not r["pairs"][0, 9:].any()
    # with one threshold just above 1/2 nothing of the 1/2 cases matches, and max_dets = 1 keeps one row per class
    r1 = R.match(pred, gt, 4, thresholds=[np.nextafter(0.5, 1)], max_dets=1)
    assert r1["det_gt"][0, 0, :8].tolist() == [0] * 8 and r1["det_valid"][0, :8].tolist() == [1, 0, 0, 0, 1, 1, 0, 0]
    # max_queries cuts through class 3: rows 6 and 7 are gone
    r2 = R.match(pred, gt, 4, max_queries=6)
    assert r2["det_valid"].shape == (1, 6) and np.array_equal(r2["det_gt"][0], want[:, :6])


def test_hand_case_panoptic_and_accumulate():
    """panoptic: IoU > 0.5 strictly, so the 1/2 cases (pred 1, 5, 6, 7) are unmatched false positives, pred 2, 3, 4 match; pred 8 lies
    wholly on void (4/4 > 0.5) and is dropped.  Class 1: tp 3, fp 1, fn 1, iou_sum 3/4 + 9/10 + 19/20; class 2: fp 1, fn 2; class 3: fp 2, fn 1."""
    pred, gt = R.hand_case()
    r = R.match(pred, gt, 4)
    assert r["pq_gt"][0, :8].tolist() == [0, 2, 3, 4, 0, 0, 0, 0]
    assert r["pq_iou"][0, :8].tolist() == [0, 6 / 8, 9 / 10, 19 / 20, 0, 0, 0, 0]
    assert r["pq_fp"][0, :8].tolist() == [1, 0, 0, 0, 1, 1, 1, 0]
    pq = R.accumulate_pq([r], 4, things=[False, True, False, False])
    assert pq["tp"].tolist() == [0, 3, 0, 0] and pq["fp"].tolist() == [0, 1, 1, 2] and pq["fn"].tolist() == [0, 1, 2, 1]
    s = 6 / 8 + 9 / 10 + 19 / 20
    assert pq["iou_sum"][1] == s and pq["pq"][1] == s / 4 and pq["sq"][1] == s / 3 and pq["rq"][1] == 3 / 4
    assert pq["All"]["n"] == 3 and abs(pq["All"]["pq"] - s / 12) <= 3 * EPS and pq["Things"]["pq"] == s / 4 and pq["Stuff"]["pq"] == 0
    # AP, class 1 (4 gts, scores 0.9 .. 0.6): at 0.5 all four are true positives: precision 1 at every recall;
    # at 0.55 .. 0.75 the first is a false positive: precision envelope 3/4 up to recall 3/4, 0 beyond
    ap = R.accumulate_ap([r], 4)
    assert np.allclose(ap["precision"][0, :, 1], 1.0, rtol=0, atol=1e-12)
    assert np.allclose(ap["precision"][1, :76, 1], 0.75, rtol=0, atol=1e-12) and not ap["precision"][1, 76:, 1].any()
    assert (ap["precision"][:, :, 0] == -1).all()
    # class 3 (1 gt; tp, fp, fp at 0.5): precision 1 everywhere at 0.5, 0 above; class 2 (2 gts, one tp at 0.5): 1 up to recall 1/2
    assert np.allclose(ap["precision"][0, :, 3], 1.0, atol=1e-12) and not ap["precision"][1:, :, 3].any()
    assert np.allclose(ap["precision"][0, :51, 2], 1.0, atol=1e-12) and not ap["precision"][0, 51:, 2].any()
    assert ap["ap"] == float(np.mean(ap["precision"][:, :, 1:]))


def _matches(r):
    from maskunet_amd import Matches
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items()}
    return Matches(t["det_valid"], t["det_class"], t["det_score"], t["det_gt"], t["det_iou"], t["gt_per_class"], t["pq_gt"], t["pq_iou"],
                   t["pq_fp"], t["overflow"], t["pairs"], t["n_pairs"])


@pytest.fixture(scope="module")
def random_results():
    out = []
    for seed, (B, H, W) in enumerate([(3, 20, 24), (2, 13, 9)]):
        pred, gt = R.random_case(100 + seed, B, H, W, 5)
        out.append(R.match(pred, gt, 5, max_dets=4))
    assert sum(int((r["pq_gt"] > 0).sum()) for r in out) >= 5 and sum(int(r["pq_fp"].sum()) for r in out) >= 5
    return out


def test_instance_ap_equals_the_restatement(random_results):
    from maskunet_amd import InstanceAP
    hand = R.match(*R.hand_case(), 4)
    for results, C in ((random_results, 5), ([hand], 4), ([hand, hand], 4)):
        acc = InstanceAP(C)
        for r in results:
            acc.update(_matches(r))
        got, want = acc.compute(), R.accumulate_ap(results, C)
        assert np.array_equal(got["precision"], want["precision"])
        n = int((want["precision"] > -1).sum())
        print(f"ap {got['ap']!r} reference {want['ap']!r} over {n} entries")
        assert n > 0 and abs(got["ap"] - want["ap"]) <= n * EPS * abs(want["ap"])
    assert 0 < R.accumulate_ap(random_results, 5)["ap"] < 1


def test_panoptic_quality_equals_the_restatement(random_results):
    from maskunet_amd import PanopticQuality
    hand = R.match(*R.hand_case(), 4)
    for results, C, things in ((random_results, 5, [False, True, True, False, False]), ([hand, hand], 4, None)):
        acc = PanopticQuality(C, things)
        for r in results:
            acc.update(_matches(r))
        got, want = acc.compute(), R.accumulate_pq(results, C, things)
        for k in ("tp", "fp", "fn"):
            assert np.array_equal(got[k], want[k]), k
        assert want["tp"].sum() > 0
        for c in range(C):
            n = max(int(want["tp"][c]), 1)
            for k in ("iou_sum", "pq", "sq", "rq"):
                assert abs(got[k][c] - want[k][c]) <= n * EPS * abs(want[k][c]), (k, c)
        for name in ("All", "Things", "Stuff") if things else ("All",):
            n = want[name]["n"]
            assert got[name]["n"] == n
            for k in ("pq", "sq", "rq"):
                print(f"{name} {k} {got[name][k]!r} reference {want[name][k]!r} over {n} classes")
                assert abs(got[name][k] - want[name][k]) <= (n + int(want["tp"].max())) * EPS * abs(want[name][k])
    # a second run gives the same bits
    acc2 = PanopticQuality(4)
    acc2.update(_matches(hand))
    acc2.update(_matches(hand))
    assert acc2.compute()["iou_sum"].tobytes() == got["iou_sum"].tobytes()


def test_accumulators_refuse_overflow_and_mismatches(random_results):
    from maskunet_amd import InstanceAP, PanopticQuality
    r = dict(random_results[0])
    r["overflow"] = np.array([0, 1, 0], np.int32)
    for acc in (InstanceAP(5), PanopticQuality(5)):
        with pytest.raises(RuntimeError, match="before any update"):
            acc.compute()
        acc.update(_matches(random_results[1]))
        acc.update(_matches(r))
        with pytest.raises(RuntimeError, match="max_instances"):
            acc.compute()
    with pytest.raises(ValueError):
        InstanceAP(4).update(_matches(random_results[0]))             # made for 5 classes
    with pytest.raises(ValueError):
        InstanceAP(5, [0.5]).update(_matches(random_results[0]))      # made for 10 thresholds
    with pytest.raises(ValueError):
        InstanceAP(5, [0.0, 0.5])
    with pytest.raises(ValueError):
        InstanceAP(5, np.linspace(0.1, 0.9, 33))
    with pytest.raises(ValueError):
        PanopticQuality(5, things=[True])


def test_match_instances_validates_its_arguments():
    import maskunet_amd
    from maskunet_amd import Instances

    def inst(B=1, H=8, W=8, M=4):
        z = torch.zeros
        return Instances(z(B, H, W, dtype=torch.int32), z(B, H, W, dtype=torch.int32), z(B, M, 8, dtype=torch.int32), z(B, M),
                         z(B, dtype=torch.int32), z(B, M, dtype=torch.int32))
    with pytest.raises(TypeError):
        maskunet_amd.match_instances(inst(), None, 4)
    with pytest.raises(RuntimeError, match="differ"):
        maskunet_amd.match_instances(inst(), inst(H=9), 4)
    with pytest.raises(RuntimeError, match="GPU"):
        maskunet_amd.match_instances(inst(), inst(), 4)                # CPU tensors: there is no fallback
    for n in ("match_instances", "Matches", "InstanceAP", "PanopticQuality"):
        assert n in maskunet_amd.__all__


def _lib():
    from maskunet_amd import _lib
    return _lib.load()


def test_entry_points_are_in_the_binding_table_and_exported():
    from maskunet_amd import _lib
    for n in ("mu_instance_pairs", "mu_instance_pairs_supported", "mu_instance_pairs_workspace_bytes", "mu_instance_match",
              "mu_instance_match_supported", "mu_instance_match_workspace_bytes"):
        assert n in _lib.SIGNATURES and hasattr(_lib.load(), n)
    assert len(_lib.SIGNATURES["mu_instance_pairs"][1]) == 12 and len(_lib.SIGNATURES["mu_instance_match"][1]) == 31


def test_supported_and_workspace_are_host_only():
    lib = _lib()
    assert lib.mu_instance_pairs_supported(256, 256, 4096, 4096) == MU_OK and lib.mu_instance_pairs_supported(1, 1, 1, 1) == MU_OK
    assert lib.mu_instance_match_supported(256, 256, 4096, 4096, 1024, 4096, 100, 32) == MU_OK
    assert lib.mu_instance_match_supported(1, 1, 1, 1, 1, 1, 1, 1) == MU_OK
    # bitmap + row numbers: 2 words of 4 bytes per 32 gt ids (0..max) and pred id
    assert lib.mu_instance_pairs_workspace_bytes(2, 16, 16, 64, 31) == 2 * 64 * 1 * 8
    assert lib.mu_instance_pairs_workspace_bytes(2, 16, 16, 64, 32) == 2 * 64 * 2 * 8
    assert lib.mu_instance_pairs_workspace_bytes(64, 128, 128, 1024, 1024) == 64 * 1024 * 33 * 8
    assert lib.mu_instance_pairs_workspace_bytes(0, 16, 16, 64, 64) == 0 and lib.mu_instance_pairs_workspace_bytes(1, 256, 257, 64, 64) == 0
    assert lib.mu_instance_match_workspace_bytes(3, 50) == 3 * 50 * 4 and lib.mu_instance_match_workspace_bytes(0, 50) == 0


@pytest.mark.parametrize("args", [(256, 257, 64, 64), (0, 8, 64, 64), (8, 8, 0, 64), (8, 8, 4097, 64), (8, 8, 64, 0), (8, 8, 64, 4097)])
def test_pair_limits_are_shape_errors(args):
    lib = _lib()
    H, W, mp, mg = args
    assert lib.mu_instance_pairs_supported(*args) == MU_ERR_SHAPE
    if H > 0:
        fake = 4096
        assert lib.mu_instance_pairs(fake, fake, 1, H, W, mp, mg, fake, fake, fake, 1 << 30, None) == MU_ERR_SHAPE


def _match_args(thr):
    fake = 4096
    #        0..7 inputs     B  H  W  mp  mg  nc  K  max_dets  thr  T          18..27 outputs   ws    bytes    stream
    return [fake] * 8 + [1, 8, 8, 16, 16, 4, 16, 100, thr.ctypes.data, len(thr)] + [fake] * 10 + [fake, 1 << 20, None]


@pytest.mark.parametrize("idx,value", [(9, 257), (11, 0), (11, 4097), (12, 0), (12, 4097), (13, 0), (13, 1025), (14, 0), (14, 17),
                                       (15, 0), (17, 0), (17, 33)])
def test_match_limits_are_shape_errors(idx, value):
    thr = np.linspace(0.5, 0.95, 10)
    a = _match_args(thr)
    a[idx] = value
    if idx == 9:
        a[10] = 256                                      # 257 x 256 pixels
    assert _lib().mu_instance_match(*a) == MU_ERR_SHAPE


def test_null_pointers_and_bad_arguments_return_before_any_launch():
    lib = _lib()
    fake = 4096
    args = [fake, fake, 1, 8, 8, 16, 16, fake, fake, fake, 1 << 20, None]
    assert lib.mu_instance_pairs(*args[:10], lib.mu_instance_pairs_workspace_bytes(1, 8, 8, 16, 16) - 1, None) == MU_ERR_WORKSPACE
    for i in (0, 1, 7, 8, 9):
        a = list(args)
        a[i] = None
        assert lib.mu_instance_pairs(*a) == MU_ERR_ARG, i
    for i in (2, 3, 4):
        a = list(args)
        a[i] = 0
        assert lib.mu_instance_pairs(*a) == MU_ERR_ARG, i
    thr = np.linspace(0.5, 0.95, 10)
    args = _match_args(thr)
    for i in list(range(8)) + [16] + list(range(18, 29)):
        a = list(args)
        a[i] = None
        assert lib.mu_instance_match(*a) == MU_ERR_ARG, i
    for i in (8, 9, 10):
        a = list(args)
        a[i] = 0
        assert lib.mu_instance_match(*a) == MU_ERR_ARG, i
    for bad in (0.0, -0.5, 1.5, float("nan")):
        t = np.array([0.5, bad])
        assert lib.mu_instance_match(*_match_args(t)) == MU_ERR_ARG, bad
    a = list(args)
    a[29] = lib.mu_instance_match_workspace_bytes(1, 16) - 1
    assert lib.mu_instance_match(*a) == MU_ERR_WORKSPACE
