"""Plain-numpy restatement of mu_panoptic's contract (include/maskunet_hip.h): loops over pixels and segments, no cleverness.  The rule
restates panopticapi's published format (id2rgb, segments_info, one segment per stuff class) and the usual semantic + instance merge;
panopticapi itself is not needed.  Also the inputs the tests share: instance rows as the producers write them, and the cases() table."""
import numpy as np

VOID, STUFF, THING = 0, 1, 2
OUT_KEYS = ("seg", "seg_cls", "table", "score", "count", "order", "source", "values", "id_map", "rgb", "invalid")


def segments(cls, ids, table, score, count, kind, category, label_divisor=1000, stuff_area_limit=0, thing_area_limit=0,
             score_threshold=0.0, max_seg=16, bgr=0):
    """every output of mu_panoptic as a dict of numpy arrays"""
    B, H, W = cls.shape
    max_inst, C = table.shape[1], len(kind)
    thr = np.float32(score_threshold)
    i32 = np.int32
    out = {"seg": np.zeros((B, H, W), i32), "seg_cls": np.zeros((B, H, W), i32), "table": np.zeros((B, max_seg, 8), i32),
           "score": np.zeros((B, max_seg), np.float32), "count": np.zeros(B, i32), "order": np.zeros((B, max_seg), i32),
           "source": np.zeros((B, max_seg), i32), "values": np.zeros((B, max_seg), i32), "id_map": np.zeros((B, H, W), i32),
           "rgb": np.zeros((B, H, W, 3), np.uint8), "invalid": np.zeros(B, i32)}
    for b in range(B):
        invalid = 0
        cand = []                                              # per pixel: None (void), ("thing", k, class) or ("stuff", c, c)
        stuff_pixels = [0] * C
        for p in range(H * W):
            k, c = int(ids[b].flat[p]), int(cls[b].flat[p])
            key, to_stuff = None, True
            if 1 <= k <= int(count[b]):
                if k > max_inst:
                    invalid |= 4
                    to_stuff = False
                else:
                    tc = int(table[b, k - 1, 0])
                    if 0 <= tc < C and kind[tc] == THING:
                        to_stuff = False                       # a thing candidate: kept, or void
                        if int(table[b, k - 1, 1]) >= thing_area_limit and np.float32(score[b, k - 1]) >= thr:
                            key = ("thing", k, tc)
            if to_stuff and 0 <= c < C and kind[c] == STUFF:
                key = ("stuff", c, c)
                stuff_pixels[c] += 1
            cand.append(key)
        number, rows = {}, []
        for p in range(H * W):
            key = cand[p]
            if key is not None and key[0] == "stuff" and stuff_pixels[key[1]] < max(stuff_area_limit, 1):
                key = None
            if key is None:
                continue
            x, y = p % W, p // W
            if key not in number:
                number[key] = len(rows) + 1
                rows.append({"key": key, "area": 0, "x0": x, "y0": y, "x1": x, "y1": y, "first": p})
            r = rows[number[key] - 1]
            r["area"] += 1
            r["x0"], r["y0"], r["x1"], r["y1"] = min(r["x0"], x), min(r["y0"], y), max(r["x1"], x), max(r["y1"], y)
            out["seg"][b].flat[p] = number[key]
            out["seg_cls"][b].flat[p] = key[2]
        n = len(rows)
        out["count"][b] = n
        if n > max_seg:
            invalid |= 2
        per_class = {}
        pixel_value = [0] * (n + 1)
        for s, r in enumerate(rows[:max_seg]):
            what, k, c = r["key"]
            rank = per_class[c] = per_class.get(c, 0) + 1
            v = int(category[c]) * label_divisor + (rank if what == "thing" else 0)
            if v <= 0 or v >= 1 << 24 or (what == "thing" and rank >= label_divisor):
                invalid |= 1
                v = 0
            out["table"][b, s] = [c, r["area"], r["x0"], r["y0"], r["x1"], r["y1"], r["first"], rank]
            out["score"][b, s] = score[b, k - 1] if what == "thing" else 1.0
            out["source"][b, s] = k if what == "thing" else 0
            out["values"][b, s] = v
            pixel_value[s + 1] = v
        m = min(n, max_seg)
        out["order"][b, :m] = sorted(range(1, m + 1), key=lambda s: (-float(out["score"][b, s - 1]), s))
        for p in range(H * W):
            v = pixel_value[out["seg"][b].flat[p]]
            out["id_map"][b].flat[p] = v
            px = [v & 255, (v >> 8) & 255, v >> 16]
            out["rgb"][b].reshape(-1, 3)[p] = px[::-1] if bgr else px
        out["invalid"][b] = invalid
    return out


def rgb2id(rgb, bgr=0):
    """panopticapi's rgb2id, on either channel order"""
    c = rgb.astype(np.int64)
    return (c[..., 2] + 256 * c[..., 1] + 65536 * c[..., 0]) if bgr else (c[..., 0] + 256 * c[..., 1] + 65536 * c[..., 2])


def segments_info(ref, b, category):
    """panopticapi's segments_info of image b from the restatement's outputs"""
    out = []
    for s in range(min(int(ref["count"][b]), ref["table"].shape[1])):
        c, area, x0, y0, x1, y1, _, _ = (int(v) for v in ref["table"][b, s])
        out.append({"id": int(ref["values"][b, s]), "category_id": int(category[c]), "area": area,
                    "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1], "iscrowd": 0})
    return out


# ------------------------------------------------------------------------------------------------
def instance_rows(ids, inst_cls, max_inst, scores=None):
    """(table, score, count) as mu_instances / mu_id_instances write them for an id map whose ids run 1..count per image: inst_cls[b][k-1]
    = the class of id k, scores[b][k-1] its score (1.0 without)"""
    B, H, W = ids.shape
    table = np.zeros((B, max_inst, 8), np.int32)
    score = np.zeros((B, max_inst), np.float32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        count[b] = ids[b].max() if ids[b].size else 0
        ranks = {}
        for k in range(1, min(int(count[b]), max_inst) + 1):
            p = np.flatnonzero(ids[b].reshape(-1) == k)
            c = int(inst_cls[b][k - 1])
            ranks[c] = ranks.get(c, 0) + 1
            table[b, k - 1] = [c, p.size, (p % W).min(), (p // W).min(), (p % W).max(), (p // W).max(), p.min(), ranks[c]]
            score[b, k - 1] = 1.0 if scores is None else scores[b][k - 1]
    return table, score, count


def raster_ids(cells):
    """cells [H,W] (0 = none) renumbered 1..n by first pixel in raster order"""
    out = np.zeros(cells.shape, np.int32)
    seen = {}
    for p, v in enumerate(cells.reshape(-1)):
        if v != 0:
            out.flat[p] = seen.setdefault(int(v), len(seen) + 1)
    return out


SCORES = np.array([0.25, 0.5, 0.75, 1.0], np.float32)


def blobs(seed, B, H, W, kind, max_inst, cell=4):
    """Random blocky images: every cell of `cell` x `cell` pixels has one class; most cells are an instance of their class (things and
    stuff alike, as predict_instances cuts every class), some instances carry another class than their pixels (as the median of an id
    map can), some cells have no instance.  -> the input dict of segments()"""
    rng = np.random.default_rng(seed)
    C = len(kind)
    gh, gw = -(-H // cell), -(-W // cell)
    up = lambda g: np.kron(g, np.ones((cell, cell), g.dtype))[:H, :W]
    cls = np.zeros((B, H, W), np.int32)
    ids = np.zeros((B, H, W), np.int32)
    inst_cls, scores = [], []
    for b in range(B):
        g = rng.integers(0, C, (gh, gw)).astype(np.int32)
        cls[b] = up(g)
        cell_id = (np.arange(gh * gw, dtype=np.int32).reshape(gh, gw) + 1) * (rng.random((gh, gw)) < 0.8)
        ids[b] = raster_ids(up(cell_id))
        n = int(ids[b].max())
        first = [int(np.flatnonzero(ids[b].reshape(-1) == k)[0]) for k in range(1, n + 1)]
        ic = np.array([cls[b].flat[p] for p in first], np.int32)
        swap = rng.random(n) < 0.15
        ic = np.where(swap, rng.integers(0, C, n), ic).astype(np.int32)
        inst_cls.append(ic)
        scores.append(SCORES[rng.integers(0, 4, n)])
    table, score, count = instance_rows(ids, inst_cls, max_inst, scores)
    return {"cls": cls, "ids": ids, "table": table, "score": score, "count": count, "kind": np.asarray(kind, np.int32),
            "category": (np.arange(C) * 3 + 1).astype(np.int32)}


def kinds(C, seed=0):
    """class 0 void, the rest stuff and things in a fixed random mix (at least one of each when C >= 3)"""
    k = np.random.default_rng(seed).integers(1, 3, C).astype(np.int32)
    k[0] = VOID
    if C >= 3:
        k[1], k[2] = STUFF, THING
    return k


def hand_4x6():
    """One stuff class (1) in two disconnected pieces and two things of class 2; class 0 void.
         cls                ids
         1 1 0 2 2 0        0 0 0 1 1 0
         1 0 0 2 2 0        0 0 0 1 1 0
         0 0 2 2 0 1        0 0 2 2 0 0
         0 0 2 2 1 1        0 0 2 2 0 0        (the stuff pixels carry no instance here)"""
    cls = np.array([[[1, 1, 0, 2, 2, 0], [1, 0, 0, 2, 2, 0], [0, 0, 2, 2, 0, 1], [0, 0, 2, 2, 1, 1]]], np.int32)
    ids = np.array([[[0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0], [0, 0, 2, 2, 0, 0], [0, 0, 2, 2, 0, 0]]], np.int32)
    table, score, count = instance_rows(ids, [[2, 2]], 4, [[0.5, 0.75]])
    return {"cls": cls, "ids": ids, "table": table, "score": score, "count": count, "kind": np.array([VOID, STUFF, THING], np.int32),
            "category": np.array([0, 7, 9], np.int32)}


def distinct_64x64():
    """every pixel its own thing of class 1: 4096 instances, as an id map gives them"""
    ids = (np.arange(4096, dtype=np.int32) + 1).reshape(1, 64, 64)
    cls = np.ones((1, 64, 64), np.int32)
    table, score, count = instance_rows(ids, [np.ones(4096, np.int32)], 4096, [SCORES[np.arange(4096) % 4]])
    return {"cls": cls, "ids": ids, "table": table, "score": score, "count": count, "kind": np.array([VOID, THING], np.int32),
            "category": np.array([0, 1], np.int32)}


def cases():
    """name -> (inputs, parameters) of segments()"""
    out = {}
    one = lambda c, k: {"cls": np.full((1, 1, 1), c, np.int32), "ids": np.full((1, 1, 1), k, np.int32),
                        **dict(zip(("table", "score", "count"), instance_rows(np.full((1, 1, 1), k, np.int32), [[c]], 2))),
                        "kind": np.array([VOID, STUFF, THING], np.int32), "category": np.array([0, 5, 6], np.int32)}
    out["1x1_thing"] = (one(2, 1), {})
    out["1x1_stuff"] = (one(1, 0), {})
    out["1x1_stuff_under_an_instance"] = (one(1, 1), {})
    out["1x1_void"] = (one(0, 0), {})
    out["hand_4x6"] = (hand_4x6(), {"max_seg": 4})
    out["hand_4x6_bgr"] = (hand_4x6(), {"max_seg": 4, "bgr": 1})
    out["5x7"] = (blobs(1, 1, 5, 7, kinds(5, 1), 16, cell=2), {"max_seg": 8})
    out["13x9"] = (blobs(2, 1, 13, 9, kinds(6, 2), 32, cell=3), {"max_seg": 16, "bgr": 1})
    out["33x31"] = (blobs(3, 2, 33, 31, kinds(9, 3), 128), {"max_seg": 64, "score_threshold": 0.5})
    out["33x31_area_limits"] = (blobs(3, 2, 33, 31, kinds(9, 3), 128), {"max_seg": 64, "stuff_area_limit": 40, "thing_area_limit": 13})
    out["33x31_few_rows"] = (blobs(4, 1, 33, 31, kinds(9, 3), 128), {"max_seg": 5})
    d = distinct_64x64()
    for m in (4096, 1, 4095):
        out[f"distinct_64x64_max_seg_{m}"] = (d, {"max_seg": m, "label_divisor": 8192})
    out["256x256"] = (blobs(5, 1, 256, 256, kinds(21, 5), 1024, cell=9), {"max_seg": 256, "bgr": 1})
    out["one_class_stuff"] = (blobs(6, 1, 13, 9, [STUFF], 16, cell=3), {"max_seg": 2})
    out["two_classes"] = (blobs(7, 1, 13, 9, [VOID, THING], 16, cell=3), {"max_seg": 16})
    out["1024_classes"] = (blobs(8, 1, 33, 31, kinds(1024, 8), 512, cell=2), {"max_seg": 512, "label_divisor": 100})
    three = blobs(9, 3, 13, 9, kinds(6, 9), 32, cell=3)
    three["cls"][1] = 0                                        # the image in the middle: nothing but void
    three["ids"][1] = 0
    three["table"][1], three["score"][1], three["count"][1] = 0, 0, 0
    out["batch_of_three_void_in_the_middle"] = (three, {"max_seg": 16})
    over = blobs(10, 1, 13, 9, [VOID, STUFF, THING], 32, cell=3)
    over["table"], over["score"] = over["table"][:, :4].copy(), over["score"][:, :4].copy()      # count stays: ids 5.. are past max_inst
    out["count_past_max_inst"] = (over, {"max_seg": 16})
    none = blobs(11, 1, 13, 9, kinds(6, 11), 32, cell=3)
    none["count"][:] = 0                                       # the ids are there, but no instance is: everything goes by its class
    out["count_zero"] = (none, {"max_seg": 16})
    out["label_divisor_one"] = (hand_4x6(), {"max_seg": 4, "label_divisor": 1})
    for name, cat in (("value_2_24_minus_1", (1 << 24) - 1), ("value_2_24", 1 << 24)):
        h = hand_4x6()
        h["category"] = np.array([0, cat, 9], np.int32)
        h["count"][:] = 0                                      # stuff only: with this divisor every thing would set bit 0
        out[f"stuff_{name}"] = (h, {"max_seg": 4, "label_divisor": 1})
    h = hand_4x6()
    h["category"] = np.array([0, 7, (1 << 23) - 1], np.int32)  # things: 2^24 - 2 + rank; rank 1 fits, rank 2 is 2^24 and >= the divisor
    out["thing_value_2_24_minus_1_and_2_24"] = (h, {"max_seg": 4, "label_divisor": 2})
    for lim in (3, 4, 5):                                      # hand_4x6: both things have 4 pixels, the stuff class has 6
        out[f"thing_area_limit_{lim}"] = (hand_4x6(), {"max_seg": 4, "thing_area_limit": lim})
    for lim in (5, 6, 7):
        out[f"stuff_area_limit_{lim}"] = (hand_4x6(), {"max_seg": 4, "stuff_area_limit": lim})
    out["score_threshold_equal"] = (hand_4x6(), {"max_seg": 4, "score_threshold": 0.75})
    out["score_threshold_one_ulp_above"] = (hand_4x6(), {"max_seg": 4, "score_threshold": float(np.nextafter(np.float32(0.75), np.float32(1)))})
    return out
