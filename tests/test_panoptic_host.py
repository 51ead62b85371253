"""CPU: the numpy restatement of mu_panoptic's contract (tests/_panoptic_reference.py) against expectations written out by hand, and
the parts of maskunet_amd.panoptic that need no device."""
import numpy as np
import pytest

from tests import _panoptic_reference as R


def test_hand_image_stuff_in_two_pieces_and_two_things():
    """hand_4x6: stuff class 1 (category 7) in two pieces of 3 pixels, two things of class 2 (category 9) of 4 pixels each"""
    inputs = R.hand_4x6()
    r = R.segments(**inputs, max_seg=4)
    assert r["count"].tolist() == [3] and r["invalid"].tolist() == [0]
    assert r["seg"][0].tolist() == [[1, 1, 0, 2, 2, 0],
                                    [1, 0, 0, 2, 2, 0],
                                    [0, 0, 3, 3, 0, 1],
                                    [0, 0, 3, 3, 1, 1]]
    assert r["seg_cls"][0].tolist() == [[1, 1, 0, 2, 2, 0],
                                        [1, 0, 0, 2, 2, 0],
                                        [0, 0, 2, 2, 0, 1],
                                        [0, 0, 2, 2, 1, 1]]
    # class, area, x_min, y_min, x_max, y_max, first_pixel, class_rank: the stuff segment's box spans both pieces
    assert r["table"][0].tolist() == [[1, 6, 0, 0, 5, 3, 0, 1],
                                      [2, 4, 3, 0, 4, 1, 3, 1],
                                      [2, 4, 2, 2, 3, 3, 14, 2],
                                      [0, 0, 0, 0, 0, 0, 0, 0]]
    assert r["values"][0].tolist() == [7000, 9001, 9002, 0]
    assert r["source"][0].tolist() == [0, 1, 2, 0]
    assert r["score"][0].tolist() == [1.0, 0.5, 0.75, 0.0]
    assert r["order"][0].tolist() == [1, 3, 2, 0]
    assert r["id_map"][0].tolist() == [[7000, 7000, 0, 9001, 9001, 0],
                                       [7000, 0, 0, 9001, 9001, 0],
                                       [0, 0, 9002, 9002, 0, 7000],
                                       [0, 0, 9002, 9002, 7000, 7000]]
    # 7000 = 0x1b58, 9001 = 0x2329, 9002 = 0x232a: R = low byte, G = the next, B = 0
    colour = {0: [0, 0, 0], 7000: [0x58, 0x1b, 0], 9001: [0x29, 0x23, 0], 9002: [0x2a, 0x23, 0]}
    assert r["rgb"][0].tolist() == [[colour[v] for v in row] for row in r["id_map"][0].tolist()]
    b = R.segments(**inputs, max_seg=4, bgr=1)
    assert b["rgb"][0].tolist() == [[colour[v][::-1] for v in row] for row in r["id_map"][0].tolist()]
    for k in R.OUT_KEYS:
        if k != "rgb":
            assert np.array_equal(b[k], r[k]), k
    assert R.segments_info(r, 0, inputs["category"]) == [
        {"id": 7000, "category_id": 7, "area": 6, "bbox": [0, 0, 6, 4], "iscrowd": 0},
        {"id": 9001, "category_id": 9, "area": 4, "bbox": [3, 0, 2, 2], "iscrowd": 0},
        {"id": 9002, "category_id": 9, "area": 4, "bbox": [2, 2, 2, 2], "iscrowd": 0}]


def small(cls, ids, inst_cls, scores=None, kind=(R.VOID, R.STUFF, R.THING), category=(0, 7, 9), max_inst=4):
    cls, ids = np.asarray(cls, np.int32)[None], np.asarray(ids, np.int32)[None]
    table, score, count = R.instance_rows(ids, [inst_cls], max_inst, None if scores is None else [scores])
    return {"cls": cls, "ids": ids, "table": table, "score": score, "count": count, "kind": np.asarray(kind, np.int32),
            "category": np.asarray(category, np.int32)}


def test_thing_first_when_the_instance_class_differs_from_the_pixel_class():
    """instance 1 has class 2 (a thing: the median of an id map, say) although one of its pixels is of stuff class 1: the pixel goes
    with the thing and takes the thing's class.  Instance 2 has a stuff class, so it is no thing: its pixels go by their own class,
    the one of class 1 to the stuff segment, the two of class 2 (a thing class, but no thing instance) to void."""
    r = R.segments(**small([[1, 2, 2, 1], [1, 1, 2, 2]], [[1, 1, 1, 0], [0, 2, 2, 2]], [2, 1]))
    assert r["seg"][0].tolist() == [[1, 1, 1, 2], [2, 2, 0, 0]]
    assert r["seg_cls"][0].tolist() == [[2, 2, 2, 1], [1, 1, 0, 0]]
    assert r["count"].tolist() == [2] and r["invalid"].tolist() == [0]
    assert r["table"][0, :2, :2].tolist() == [[2, 3], [1, 3]] and r["source"][0, :2].tolist() == [1, 0]
    assert r["values"][0, :2].tolist() == [9001, 7000]


def test_failed_thing_is_void_not_stuff():
    """the thing covers pixels of stuff class 1; when it fails the score threshold all of its pixels are void, and the stuff segment does
    not grow"""
    inputs = small([[1, 1, 1, 1], [1, 1, 1, 1]], [[0, 1, 1, 0], [0, 1, 1, 0]], [2], [0.25])
    kept = R.segments(**inputs, score_threshold=0.25)
    assert kept["seg"][0].tolist() == [[1, 2, 2, 1], [1, 2, 2, 1]] and kept["table"][0, :2, 1].tolist() == [4, 4]
    for kw in ({"score_threshold": 0.5}, {"thing_area_limit": 5}):
        r = R.segments(**inputs, **kw)
        assert r["seg"][0].tolist() == [[1, 0, 0, 1], [1, 0, 0, 1]] and r["count"].tolist() == [1] and r["table"][0, 0, 1] == 4
        assert r["seg_cls"][0].tolist() == [[1, 0, 0, 1], [1, 0, 0, 1]] and not r["id_map"][0, :, 1:3].any()


def test_area_limits_and_the_score_threshold_at_their_edges():
    inputs = R.hand_4x6()                                      # things of 4 pixels (scores 0.5, 0.75), stuff of 6
    n = lambda **kw: R.segments(**inputs, max_seg=4, **kw)["count"].tolist()[0]
    assert [n(thing_area_limit=a) for a in (3, 4, 5)] == [3, 3, 1]
    assert [n(stuff_area_limit=a) for a in (5, 6, 7)] == [3, 3, 2]
    assert n(stuff_area_limit=0) == 3                          # a class with no pixel is no segment whatever the limit
    up = float(np.nextafter(np.float32(0.75), np.float32(1)))
    assert [n(score_threshold=t) for t in (0.5, 0.75, up)] == [3, 2, 1]


def test_every_invalid_bit():
    h = R.hand_4x6()
    r = R.segments(**h, max_seg=4, label_divisor=1)            # bit 0: a thing's rank 1 is not below the divisor
    assert r["invalid"].tolist() == [1] and r["values"][0].tolist() == [7, 0, 0, 0] and r["count"].tolist() == [3]
    assert r["id_map"][0].tolist() == [[7, 7, 0, 0, 0, 0], [7, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 7], [0, 0, 0, 0, 7, 7]]
    assert not r["rgb"][0, 0:2, 3:5].any() and r["seg"][0, 0, 3] == 2                  # black, but still a segment
    for cat, bad in (((1 << 24) - 1, 0), (1 << 24, 1), (0, 1), (-3, 1)):               # bit 0: the id must be in [1, 2^24)
        g = dict(h, category=np.array([0, cat, 9], np.int32), count=np.zeros(1, np.int32))
        r = R.segments(**g, max_seg=4, label_divisor=1)
        assert r["invalid"].tolist() == [bad] and r["values"][0, 0] == (0 if bad else cat)
    r = R.segments(**h, max_seg=2)                             # bit 1: three segments, two rows
    assert r["invalid"].tolist() == [2] and r["count"].tolist() == [3] and r["seg"].max() == 3
    assert r["values"][0].tolist() == [7000, 9001] and r["order"][0].tolist() == [1, 2]
    assert not r["id_map"][0, 2:, 2:4].any() and not r["rgb"][0, 2:, 2:4].any()
    g = dict(h, table=h["table"][:, :1], score=h["score"][:, :1])                      # bit 2: instance 2 is past max_inst = 1
    r = R.segments(**g, max_seg=4)
    assert r["invalid"].tolist() == [4] and r["count"].tolist() == [2] and not r["seg"][0, 2:, 2:4].any()
    r = R.segments(**dict(g, count=np.array([1], np.int32)), max_seg=4)
    assert r["invalid"].tolist() == [0] and not r["seg"][0, 2:, 2:4].any()             # k > count: no instance, and class 2 is no stuff


def test_rgb2id_inverts_the_image_in_both_channel_orders():
    for name in ("33x31", "13x9", "hand_4x6"):
        inputs, params = R.cases()[name]
        for bgr in (0, 1):
            r = R.segments(**inputs, **dict(params, bgr=bgr))
            assert np.array_equal(R.rgb2id(r["rgb"], bgr), r["id_map"]) and r["id_map"].any()
            assert not np.array_equal(R.rgb2id(r["rgb"], 1 - bgr), r["id_map"])


def test_segments_info_box_of_a_single_pixel():
    r = R.segments(**small([[0, 0, 0], [0, 0, 2]], [[0, 0, 0], [0, 0, 1]], [2]))
    assert R.segments_info(r, 0, [0, 7, 9]) == [{"id": 9001, "category_id": 9, "area": 1, "bbox": [2, 1, 1, 1], "iscrowd": 0}]


def test_cases_cover_the_branches_they_are_named_for():
    cases = R.cases()
    ref = {n: R.segments(**i, **p) for n, (i, p) in cases.items() if "256" not in n and "64x64" not in n}
    assert {n: int(r["invalid"].max()) for n, r in ref.items() if r["invalid"].any()} == {
        "33x31_few_rows": 2, "count_past_max_inst": 4, "label_divisor_one": 1, "stuff_value_2_24": 1, "thing_value_2_24_minus_1_and_2_24": 1}
    assert ref["batch_of_three_void_in_the_middle"]["count"][1] == 0
    inputs = cases["33x31"][0]
    classes = inputs["table"][0, :inputs["count"][0], 0]
    first = inputs["table"][0, :inputs["count"][0], 6]
    assert (classes != inputs["cls"][0].reshape(-1)[first]).any()                      # instances whose class is not their pixels'


def test_package_exports_and_refusals_without_a_device():
    import maskunet_amd
    assert callable(maskunet_amd.panoptic_segments) and callable(maskunet_amd.predict_panoptic) and maskunet_amd.Panoptic
    import torch
    z = torch.zeros((1, 4, 4), dtype=torch.int32)
    host = maskunet_amd.Instances(z, z, torch.zeros((1, 2, 8), dtype=torch.int32), torch.zeros((1, 2)), torch.zeros(1, dtype=torch.int32),
                                  torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="on the GPU"):
        maskunet_amd.panoptic_segments(host, (False, True))
    with pytest.raises(TypeError, match="Instances"):
        maskunet_amd.panoptic_segments(z, (False, True))
