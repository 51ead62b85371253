"""CPU: the restatement of COCO's polygon rasterisation in tests/_poly_reference.py (what mu_coco_masks is compared with on the GPU) and the
host side of maskunet_amd.coco.  Literal vectors worked by hand, the two forms of the last step against each other, two checks that do
not depend on the restatement (point-in-polygon, exact rectangles), a case that a fused multiply-add would change, and the CSR packing."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _poly_reference as R


def counts_of(xy, h, w):
    return R.counts_from_toggles(R.polygon_toggles(xy, h, w), h * w)


def test_rectangle_by_hand():
    """h=5, w=6, [1,1, 4,1, 4,3, 1,3].  Scaled by 5 (+.5, truncated): (5,5) (20,5) (20,15) (5,15).  Edge 0 walks u = 5..20 at v = 5: u rises,
    so xd = (u - 1 + .5) / 5 - .5 is whole for u - 1 = 7, 12, 17: columns 1, 2, 3; yd = (5 + .5) / 5 - .5 = .6 -> ceil 1: toggles 6, 11, 16.
    Edge 2 walks back at v = 15: u falls, xd from u = 17, 12, 7: columns 3, 2, 1; yd = 2.6 -> 3: toggles 18, 13, 8.  The vertical edges
    never change u inside, and at their ends u - 1 = 19 / u = 5 give no whole xd.  Sorted with N = 30: 6 8 11 13 16 18 30 -> differences
    6 2 3 2 3 2 12: rows 1..2 of columns 1..3, area 6."""
    assert counts_of([1, 1, 4, 1, 4, 3, 1, 3], 5, 6) == [6, 2, 3, 2, 3, 2, 12]
    m = R.mask_from_counts([6, 2, 3, 2, 3, 2, 12], 5, 6)
    want = np.zeros((5, 6), bool)
    want[1:3, 1:4] = True
    assert np.array_equal(m, want) and m.sum() == 6


def test_single_point_by_hand():
    """[2,2]: one degenerate edge, one point, no predecessor: no toggle -> [N]"""
    assert counts_of([2, 2], 5, 6) == [30]


def test_covering_polygon_by_hand():
    """[-3,-3, 20,-3, 20,20, -3,20] on 5x6.  Scaled: (int)(-14.5) = -14 and 100.  Edge 0 at v = -14: every column 0..5 is crossed with
    yd < 0 -> 0: toggles 0 5 10 .. 25.  Edge 2 at v = 100: yd > h -> 5: toggles 30 25 .. 5.  Sorted with N: 0 5 5 10 10 .. 25 25 30 30 ->
    differences 0 5 0 5 0 .. 0; merging the zero-length runs leaves [0, 30]: everything set."""
    assert counts_of([-3, -3, 20, -3, 20, 20, -3, 20], 5, 6) == [0, 30]


def test_triangle_by_hand():
    """h=w=8, [0.5,0.5, 6.5,1.0, 3.0,6.2]: scaled (3,3) (33,5) (15,31).  Edge 0 (dx = 30, dy = 2, s = 1/15) rises through u - 1 = 7, 12, ..,
    32, i.e. the columns 1..6, with min(v) = 3, 4, 4, 4, 5, 5: yd = ceil((v + .5) / 5 - .5) = ceil(.2 .. .6) = 1, toggles x * 8 + 1 = 9 17
    25 33 41 49: the upper boundary is row 1.  Edges 1 and 2 fall back through the same columns along the two long sides and give the
    lower boundary 11 21 29 36 42 49 (column 6: both boundaries at 49, a zero-length run that the merge removes).  Sorted with N = 64:
    9 11 17 21 25 29 33 36 41 42 49 49 64 -> differences 9 2 6 4 4 4 4 3 5 1 7 0 15 -> merged [9,2,6,4,4,4,4,3,5,1,22]."""
    xy = [0.5, 0.5, 6.5, 1.0, 3.0, 6.2]
    assert sorted(R.polygon_toggles(xy, 8, 8)) == [9, 11, 17, 21, 25, 29, 33, 36, 41, 42, 49, 49]
    assert counts_of(xy, 8, 8) == [9, 2, 6, 4, 4, 4, 4, 3, 5, 1, 22]


def random_polygon(rng, h, w, kind):
    k = int(rng.integers(1, 10))
    if kind == "float":
        p = rng.uniform(-4, max(h, w) + 4, size=2 * k)
    elif kind == "integer":
        p = rng.integers(-3, max(h, w) + 4, size=2 * k).astype(np.float64)
    elif kind == "outside":
        p = rng.uniform(-3 * max(h, w), 4 * max(h, w), size=2 * k)
    else:                                              # repeated points, closing duplicate
        q = rng.integers(0, max(h, w), size=(k, 2)).astype(np.float64)
        p = np.concatenate([q, q[rng.integers(0, k, size=2)], q[:1]]).reshape(-1)
    return p.tolist()


@pytest.mark.parametrize("kind", ["float", "integer", "outside", "repeated"])
def test_two_forms_agree(kind):
    """sort + difference + merge (maskApi) against toggle parity (the kernel's bitmap), toggles at p = N included"""
    rng = np.random.default_rng({"float": 1, "integer": 2, "outside": 3, "repeated": 4}[kind])
    at_n = 0
    for _ in range(150):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        t = R.polygon_toggles(random_polygon(rng, h, w, kind), h, w)
        at_n += h * w in t
        c = R.counts_from_toggles(t, h * w)
        assert sum(c) == h * w and all(v > 0 for v in c[1:])
        assert np.array_equal(R.mask_from_counts(c, h, w), R.mask_from_toggles(t, h, w))
        assert len(t) % 2 == 0, "a closed outline crosses every column an even number of times"
    assert at_n > 0 or kind == "repeated"


def _inside_even_odd(poly, px, py):
    x, y = np.asarray(poly[0::2]), np.asarray(poly[1::2])
    inside = np.zeros(px.shape, bool)
    for j in range(len(x)):
        x0, y0, x1, y1 = x[j], y[j], x[(j + 1) % len(x)], y[(j + 1) % len(x)]
        if y0 == y1:
            continue
        cross = ((y0 <= py) != (y1 <= py)) & (px < x0 + (py - y0) * (x1 - x0) / (y1 - y0))
        inside ^= cross
    return inside


def _boundary_distance(poly, px, py):
    x, y = np.asarray(poly[0::2]), np.asarray(poly[1::2])
    best = np.full(px.shape, np.inf)
    for j in range(len(x)):
        x0, y0, x1, y1 = x[j], y[j], x[(j + 1) % len(x)], y[(j + 1) % len(x)]
        ex, ey = x1 - x0, y1 - y0
        L = ex * ex + ey * ey
        t = np.clip(((px - x0) * ex + (py - y0) * ey) / L, 0, 1) if L > 0 else np.zeros(px.shape)
        best = np.minimum(best, np.hypot(px - (x0 + t * ex), py - (y0 + t * ey)))
    return best


def test_against_point_in_polygon():
    """Independent of the restatement: even-odd point-in-polygon at the pixel centres (x + .5, y + .5).  Where the two disagree, the
    centre lies within 0.5 px of the polygon's boundary (the rasteriser works on a 5x grid and rounds there)."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(400):
        h, w = int(rng.integers(4, 28)), int(rng.integers(4, 28))
        k = int(rng.integers(3, 9))
        poly = rng.uniform(-4, max(h, w) + 4, size=2 * k).tolist()
        m = R.mask_from_toggles(R.polygon_toggles(poly, h, w), h, w)
        py, px = np.mgrid[0:h, 0:w] + 0.5
        diff = m != _inside_even_odd(poly, px, py)
        if diff.any():
            worst = max(worst, float(_boundary_distance(poly, px, py)[diff].max()))
    print(f"largest distance of a disagreeing pixel centre from the boundary: {worst:.3f} px")
    assert worst <= 0.5


def test_integer_rectangles_are_exact():
    rng = np.random.default_rng(8)
    for _ in range(200):
        h, w = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        x0, x1 = sorted(rng.integers(-3, w + 4, size=2).tolist())
        y0, y1 = sorted(rng.integers(-3, h + 4, size=2).tolist())
        want = np.zeros((h, w), bool)
        want[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
        for corners in ([x0, y0, x1, y0, x1, y1, x0, y1], [x0, y1, x1, y1, x1, y0, x0, y0]):      # both orientations
            m, ok = R.annotation_mask([[float(v) for v in corners]], h, w)
            assert ok == 1 and np.array_equal(m, want), (h, w, corners)


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))       # one rounding


def _edge_points_fused(xs, ys, xe, ye):
    """edge_points with ys + s * t as ONE fused multiply-add: what a compiler that contracts would compute"""
    dx, dy = abs(xe - xs), abs(ys - ye)
    if dx == 0 and dy == 0:
        return np.array([xs], np.int64), np.array([ys], np.int64)
    flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
    if flip:
        xs, xe, ys, ye = xe, xs, ye, ys
    n = max(dx, dy)
    us, vs = [], []
    for d in range(n + 1):
        t = n - d if flip else d
        if dx >= dy:
            us.append(t + xs)
            vs.append(int(_fma(float(ye - ys) / float(dx), float(t), float(ys)) + .5))
        else:
            vs.append(t + ys)
            us.append(int(_fma(float(xe - xs) / float(dy), float(t), float(xs)) + .5))
    return np.array(us, np.int64), np.array(vs, np.int64)


def unscaled(X, Y):
    """fp64 vertices whose scaled coordinates are exactly the given integers"""
    xy = [(float(c) - .5) / 5.0 for pair in zip(X, Y) for c in pair]
    assert R.scaled_vertices(xy) == (list(X), list(Y))
    return xy


TIE_X, TIE_Y = [-3, 5, 8], [-2, 27, 28]


def test_ties_need_per_operation_rounding(monkeypatch):
    """Scaled vertices are integers, so ys + s * t lands on k + .5 all the time: with dx = 2 * dy on odd coordinates every second point
    does, exactly ((1,1)-(7,4): s = .5, v = (int)(1 + .5 t + .5) = 1 2 2 3 3 4 4), and nothing is rounded at all.  With s = dy / dx
    inexact the product is rounded first and then often lands ON the tie where the exact sum lies just below it: the edge
    (-3,-2)-(5,27) of TIE (dy = 29 > dx = 8, s = 8/29) has such points, and a fused multiply-add, which keeps the exact product, moves a
    crossing by one pixel.  Per-operation rounding gives [2, 1, 10, 1, 50] on 8x8; fused arithmetic gives [13, 1, 50]."""
    u, v = R.edge_points(1, 1, 7, 4)
    assert u.tolist() == [1, 2, 3, 4, 5, 6, 7] and v.tolist() == [1, 2, 2, 3, 3, 4, 4]
    xy = unscaled(TIE_X, TIE_Y)
    assert counts_of(xy, 8, 8) == [2, 1, 10, 1, 50]
    monkeypatch.setattr(R, "edge_points", _edge_points_fused)
    assert counts_of(xy, 8, 8) == [13, 1, 50]


def test_invalid_annotations():
    nan, inf = float("nan"), float("inf")
    for poly in ([1, 1, nan, 2, 3, 3], [1, 1, 2, inf, 3, 3], [1, 1, 4e6, 2, 3, 3], [-4e6, 1, 2, 2, 3, 3]):
        assert R.annotation_mask([[0, 0, 3, 0, 3, 3], poly], 6, 6)[1] == 0
    assert R.annotation_mask([[0, 0, 3.3e6, 0, 3, 3]], 6, 6)[1] == 0                       # 16.5 M points
    assert R.annotation_mask([[0, 0, 3, 0, 3, 3]], 6, 6, max_points=48)[1] == 1            # 16 + 16 + 16 points: exactly at the bound
    assert R.annotation_mask([[0, 0, 3, 0, 3, 3]], 6, 6, max_points=48)[0].sum() > 0
    assert R.annotation_mask([[0, 0, 3, 0, 3, 3]], 6, 6, max_points=47)[1] == 0
    assert R.annotation_mask({"counts": [3, 4, 29]}, 6, 6)[1] == 1
    assert R.annotation_mask({"counts": [3, 4, 28]}, 6, 6)[1] == 0
    assert R.annotation_mask({"counts": [3, -1, 34]}, 6, 6)[1] == 0
    assert R.annotation_mask([[0, 0, 3, 0, 3, 3]], 1024, 513)[1] == 0
    m, ok = R.annotation_mask({"counts": [3, 33]}, 6, 6)                                     # an even number of counts: ones to the end
    assert ok == 1 and m.sum() == 33 and np.array_equal(m, R.mask_from_counts([3, 33], 6, 6))


def test_union_cover_and_ids():
    """two polygons of ONE annotation overlap: cover 1; two annotations overlap: cover 2 and the larger row"""
    a, b = [0, 0, 4, 0, 4, 4, 0, 4], [2, 2, 6, 2, 6, 6, 2, 6]
    r = R.coco_masks([[[a, b]], [[a], [b]]], [(6, 6), (6, 6)], (6, 6))
    assert r["cover"][0].max() == 1 and r["area"].tolist() == [28, 16, 16] and r["cover"][0].sum() == 28
    assert r["cover"][1][2:4, 2:4].tolist() == [[2, 2], [2, 2]] and r["ids"][1][2:4, 2:4].tolist() == [[2, 2], [2, 2]]
    assert r["ids"][1][0, 0] == 1 and r["ids"][1][5, 5] == 2 and r["ids"][0].max() == 1
    assert np.array_equal(r["cover"][1], r["masks"][1].astype(np.int64) + r["masks"][2])


def test_pack_annotations():
    from maskunet_amd.coco import pack_annotations
    from maskunet_amd.rle import rle_string_from_counts
    sq = [1, 1, 4, 1, 4, 3, 1, 3]
    p = pack_annotations([[[sq, [0, 0, 1, 1]], {"size": [5, 6], "counts": [6, 2, 22]}], [], [[[2, 2]], {"counts": rle_string_from_counts([0, 16])}]],
                         [(5, 6), (3, 3), (4, 4)])
    assert p["xy"].dtype == np.float64 and p["xy"].tolist() == [float(v) for v in sq + [0, 0, 1, 1, 2, 2]]
    assert p["poly_offsets"].tolist() == [0, 4, 6, 7]
    assert p["ann_poly_offsets"].tolist() == [0, 2, 2, 3, 3]
    assert p["rle_counts"].tolist() == [6, 2, 22, 0, 16] and p["ann_rle_offsets"].tolist() == [0, 0, 3, 3, 5]
    assert p["img_ann_offsets"].tolist() == [0, 2, 2, 4] and p["sizes"].tolist() == [[5, 6], [3, 3], [4, 4]]
    assert all(p[k].dtype == np.int32 for k in p if k != "xy")
    e = pack_annotations([[], []], [(5, 6), (3, 3)])
    assert e["xy"].size == 0 and e["rle_counts"].size == 0 and e["poly_offsets"].tolist() == [0]
    assert e["ann_poly_offsets"].tolist() == [0] and e["ann_rle_offsets"].tolist() == [0] and e["img_ann_offsets"].tolist() == [0, 0, 0]
    big = pack_annotations([[{"counts": [2 ** 40, -7]}]], [(5, 6)])
    assert big["rle_counts"].tolist() == [2 ** 31 - 1, -1]                                   # clamped: still invalid on the device


def test_pack_annotations_errors():
    from maskunet_amd.coco import coco_masks, pack_annotations
    with pytest.raises(ValueError, match="one .height, width. per image"):
        pack_annotations([[]], [(5, 6), (3, 3)])
    with pytest.raises(ValueError, match="at least one"):
        pack_annotations([], [])
    with pytest.raises(ValueError, match="RLE of size .6, 5. in an image of .5, 6."):
        pack_annotations([[{"size": [6, 5], "counts": [30]}]], [(5, 6)])
    with pytest.raises(ValueError, match="polygon with 5 coordinates"):
        pack_annotations([[[[1, 2, 3, 4, 5]]]], [(5, 6)])
    with pytest.raises(ValueError, match="RLE without counts"):
        pack_annotations([[{"counts": []}]], [(5, 6)])
    with pytest.raises(TypeError, match="list of polygons or an RLE dict"):
        pack_annotations([["abc"]], [(5, 6)])
    with pytest.raises(ValueError, match="ends inside a count"):
        pack_annotations([[{"counts": "a"}]], [(5, 6)])
    with pytest.raises(ValueError, match="positive"):
        pack_annotations([[]], [(0, 6)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        coco_masks([[]], [(5, 6)], device="cpu")
