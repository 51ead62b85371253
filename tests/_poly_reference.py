"""Naive restatement of COCO's polygon / RLE annotation handling (the published maskApi.c: rleFrPoly, rleMerge, rleDecode, rleArea;
coco.py: annToMask) and of what coco_instance.py:52-83, 331-338 make of it: every annotation's mask, resized with INTER_NEAREST, summed
into the label map.  TEST INFRASTRUCTURE ONLY: mu_coco_masks / maskunet_amd.coco are compared with it bit for bit.  Not pinned to
pycocotools (which is not available where this project is tested); the contract is the text in include/maskunet_hip.h.

Masks are read column-major: position p = x * h + y, N = h * w.  A polygon becomes a list of TOGGLE positions; two forms of the last
step are kept and must agree (tests/test_poly_host.py):
  * counts_from_toggles: maskApi's own -- sort the toggles with N appended, take differences, merge the zero-length runs;
  * mask_from_toggles:   position p < N is set iff an odd number of toggles is <= p (what the kernel's bitmap does).
Every fp64 operation is rounded on its own (numpy never fuses a multiply and an add).
"""
from __future__ import annotations

import numpy as np

MAX_PIXELS = 1 << 19
MAX_OUT_PIXELS = 65536
MAX_POINTS = 1 << 20
COORD_LIMIT = float(1 << 24)


def scaled_vertices(xy):
    """(X, Y) int lists of the k points, or None where a coordinate is non-finite or |5 x + .5| >= 2^24"""
    xy = np.asarray(xy, np.float64).reshape(-1)
    s = 5.0 * xy
    s = s + .5
    if not bool(np.all(np.abs(s) < COORD_LIMIT)):          # NaN compares false
        return None
    t = np.trunc(s).astype(np.int64)                       # (int): toward zero
    return t[0::2].tolist(), t[1::2].tolist()


def edge_count(xs, ys, xe, ye):
    return max(abs(xe - xs), abs(ys - ye)) + 1


def edge_points(xs, ys, xe, ye):
    """the points of one edge from its start to its end: two int64 arrays"""
    dx, dy = abs(xe - xs), abs(ys - ye)
    if dx == 0 and dy == 0:
        return np.array([xs], np.int64), np.array([ys], np.int64)
    flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
    if flip:
        xs, xe, ys, ye = xe, xs, ye, ys
    n = max(dx, dy)
    d = np.arange(n + 1, dtype=np.int64)
    t = (n - d) if flip else d
    tf = t.astype(np.float64)
    if dx >= dy:
        s = np.float64(ye - ys) / np.float64(dx)
        f = s * tf
        f = np.float64(ys) + f
        f = f + .5
        return t + xs, np.trunc(f).astype(np.int64)
    s = np.float64(xe - xs) / np.float64(dy)
    f = s * tf
    f = np.float64(xs) + f
    f = f + .5
    return np.trunc(f).astype(np.int64), t + ys


def polygon_point_count(X, Y):
    k = len(X)
    return sum(edge_count(X[j], Y[j], X[(j + 1) % k], Y[(j + 1) % k]) for j in range(k))


def polygon_toggles(xy, h, w, max_points=MAX_POINTS):
    """the toggle positions of one polygon in emission order (values in 0..h*w), or None for an invalid one"""
    sv = scaled_vertices(xy)
    if sv is None:
        return None
    X, Y = sv
    k = len(X)
    if k == 0:
        return []
    if polygon_point_count(X, Y) > max_points:
        return None
    us, vs = [], []
    for j in range(k):
        u, v = edge_points(X[j], Y[j], X[(j + 1) % k], Y[(j + 1) % k])
        us.append(u)
        vs.append(v)
    u, v = np.concatenate(us), np.concatenate(vs)
    i = np.nonzero(u[1:] != u[:-1])[0] + 1                 # every i >= 1 with u[i] != u[i-1]; no wrap-around
    xd = np.where(u[i] < u[i - 1], u[i], u[i] - 1).astype(np.float64)
    xd = (xd + .5) / 5.0 - .5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = np.where(v[i] < v[i - 1], v[i], v[i - 1]).astype(np.float64)
    yd = (yd + .5) / 5.0 - .5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    return (xd.astype(np.int64) * h + yd.astype(np.int64))[keep].tolist()


def counts_from_toggles(toggles, N):
    """maskApi: a = sorted(toggles + [N]); differences; merge the zero-length runs -> RLE counts"""
    a = sorted(list(toggles) + [N])
    p, diff = 0, []
    for t in a:
        diff.append(t - p)
        p = t
    b = [diff[0]]
    j = 1
    while j < len(diff):
        if diff[j] > 0:
            b.append(diff[j])
            j += 1
        else:
            j += 1
            if j < len(diff):
                b[-1] += diff[j]
                j += 1
    return b


def mask_from_counts(counts, h, w):
    """rleDecode: bool [h, w]"""
    flat = np.zeros(h * w, bool)
    p, v = 0, False
    for c in counts:
        if v:
            flat[p:p + c] = True
        p += c
        v = not v
    assert p == h * w
    return np.ascontiguousarray(flat.reshape(w, h).T)


def mask_from_toggles(toggles, h, w):
    """position p < N is set iff an odd number of toggles is <= p: bool [h, w]"""
    N = h * w
    hist = np.zeros(N + 1, np.int64)
    for t in toggles:
        hist[t] += 1
    flat = (np.cumsum(hist[:N]) & 1).astype(bool)
    return np.ascontiguousarray(flat.reshape(w, h).T)


def rle_toggles(counts, N):
    """the toggles of an RLE = the prefix sums of its counts without the last; None where a count is negative or they do not sum to N"""
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts) or sum(counts) != N:
        return None
    return np.cumsum(np.asarray(counts[:-1], np.int64)).tolist()


def annotation_mask(seg, h, w, max_points=MAX_POINTS):
    """annToMask: (bool [h, w], valid).  seg = a list of polygons (flat coordinate lists), or {"counts": [ints]} at the image's size.
    An invalid annotation (see the module text) gives an empty mask and valid = 0."""
    empty = np.zeros((h, w), bool)
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        return empty, 0
    if isinstance(seg, dict):
        t = rle_toggles(seg["counts"], h * w)
        return (empty, 0) if t is None else (mask_from_toggles(t, h, w), 1)
    m = empty.copy()
    for poly in seg:
        t = polygon_toggles(poly, h, w, max_points)
        if t is None:
            return empty, 0
        m |= mask_from_toggles(t, h, w)
    return m, 1


def nearest_index(dn, sn):
    """source index per destination index of cv2.resize(.., INTER_NEAREST) (oracle/cv2_resize_oracle.resize_nearest)"""
    inv = 1.0 / (float(dn) / float(sn))
    return np.minimum(np.floor(np.arange(dn, dtype=np.float64) * inv).astype(np.int64), sn - 1)


def rasters(annotations, sizes, max_points=MAX_POINTS):
    """[(bool [h, w], valid)] of every annotation, image after image: the costly half of coco_masks, the same for every output size"""
    return [annotation_mask(seg, h, w, max_points) for segs, (h, w) in zip(annotations, sizes) for seg in segs]


def coco_masks(annotations, sizes, out_hw, max_points=MAX_POINTS, rasters_=None):
    """annotations: list (images) of lists of segmentations; sizes: [(h, w)] per image -> dict of
    cover int64 [B,Ho,Wo], ids int32 [B,Ho,Wo], masks uint8 [A,Ho,Wo], area int32 [A], valid int32 [A]"""
    Ho, Wo = out_hw
    B, A = len(annotations), sum(len(a) for a in annotations)
    rasters_ = rasters(annotations, sizes, max_points) if rasters_ is None else rasters_
    cover = np.zeros((B, Ho, Wo), np.int64)
    ids = np.zeros((B, Ho, Wo), np.int32)
    masks = np.zeros((A, Ho, Wo), np.uint8)
    area, valid = np.zeros(A, np.int32), np.zeros(A, np.int32)
    a = 0
    for b, (segs, (h, w)) in enumerate(zip(annotations, sizes)):
        for r in range(len(segs)):
            m, ok = rasters_[a]
            valid[a] = ok
            if ok:
                area[a] = int(m.sum())
                small = m[nearest_index(Ho, h)][:, nearest_index(Wo, w)]
                masks[a] = small
                cover[b] += small
                ids[b] = np.where(small, r + 1, ids[b])         # rows ascend: the largest covering row stays
            a += 1
    return {"cover": cover, "ids": ids, "masks": masks, "area": area, "valid": valid}
