"""GPU: COCO annotations to masks and targets on the device (mu_coco_masks, maskunet_amd.coco) against the naive restatement in
tests/_poly_reference.py.  The feature is integer / fp64 with an exactly stated contract: every output -- cover, ids, masks, area, valid --
is compared with ==, through the C ABI and through coco_masks.  One batch mixes the image sizes and the annotation cases; its full-size
rasters are computed once and shared.  Memory discipline as in test_gpu_rle.py: outputs pre-filled with a sentinel, 4 KiB guard bands
around every buffer, inputs verified untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import _poly_reference as R
from tests._device_buffers import Guarded, call
from tests._instances_reference import table_from_ids
from tests.test_poly_host import TIE_X, TIE_Y, unscaled

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_KEYS = ("cover", "ids", "masks", "area", "valid")
IN_KEYS = ("xy", "poly_offsets", "ann_poly_offsets", "rle_counts", "ann_rle_offsets", "img_ann_offsets", "sizes")
OUT_SIZES = [(128, 128), (3, 5), (96, 80)]             # the reference's; tiny; larger than five of the source sizes (upsampling)
MAX_POINTS = 100000                                    # every legitimate polygon of the batch stays below, one row walks 120 000
OVER_LIMIT = (1024, 513)                               # h * w = 2^19 + 1024


def rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def random_runs(rng, N, n):
    """n counts >= 0 that sum to N, some of them zero"""
    cuts = np.sort(rng.integers(0, N + 1, size=n - 1))
    return np.diff(np.concatenate([[0], cuts, [N]])).astype(int).tolist()


@functools.lru_cache(maxsize=None)
def batch():
    """(annotations, sizes): RLE counts as lists (the reference's form)"""
    rng = np.random.default_rng(5)
    poly = lambda k, lo, hi: rng.uniform(lo, hi, size=2 * k).tolist()
    ang = np.linspace(0, 2 * np.pi, 3000, endpoint=False)
    rad = 150 + 40 * np.sin(7 * ang) + rng.uniform(-.3, .3, size=ang.size)
    star = np.stack([320 + rad * np.cos(ang), 240 + rad * np.sin(ang)], 1).reshape(-1).tolist()       # 3000 vertices: six chunks of edges
    images = [
        ((1, 1), [[rect(0, 0, 1, 1)], [[0.5, 0.5]], [rect(-2, -2, 3, 3)]]),
        ((5, 6), [[[1, 1, 4, 1, 4, 3, 1, 3]], [[2, 2]], [[-3, -3, 20, -3, 20, 20, -3, 20]], {"counts": [6, 2, 22]}]),
        ((7, 64), [[poly(5, -3, 66)], [poly(7, 0, 64), poly(3, 0, 7)], [[-8.25, 3.5, 70.75, 2.25, 30.5, -4.75]], {"counts": [448]},
                   {"counts": [0, 448]}]),
        ((64, 7), [[poly(6, -5, 70)], [[3.5, -10.5, 3.25, 80.75]], [rect(-1.5, 10.25, 4.75, 50.5), rect(2, 30, 9, 60)]]),
        ((33, 31), [[unscaled(TIE_X, TIE_Y)],                                        # a fused multiply-add changes this mask
                    [rect(2, 2, 14, 14), rect(8, 8, 22, 22)],                         # two overlapping polygons in ONE annotation: cover 1
                    [rect(10, 10, 20, 20)], [rect(15, 15, 30, 32)],                   # overlapping annotations: cover 2..3, ids = the larger row
                    [[4, 4]], [[4, 4, 20, 9]],                                        # 1 and 2 points
                    [[5, 20, 12, 20, 12, 28, 5, 28, 5, 20]],                          # closing duplicate vertex
                    [rect(40, 40, 50, 50)], [rect(-90, 5, -10, 25)],                  # wholly outside
                    [rect(-5, -5, 40, 40)],                                           # wholly covering
                    [[1, 1, 9, 1, 5, 8], []],                                         # a polygon without points adds nothing
                    []]),                                                             # no polygon at all: empty and valid
        ((480, 640), [[star],
                      {"counts": random_runs(rng, 480 * 640, 41)}, {"counts": random_runs(rng, 480 * 640, 40)},
                      {"counts": [1000, 2000, 480 * 640 - 2999]},                    # wrong sum
                      {"counts": [1000, -5, 480 * 640 - 995]},                       # negative count
                      [rect(100, 100, 200, 200), [50.0, float("nan"), 60, 60, 70, 50]],   # a non-finite coordinate
                      [[10, 10, float("inf"), 20, 30, 30]], [[10, 10, 3.4e6, 20, 30, 30]],
                      [[-3000, -3000, 5000, -3000, 5000, 5000]],                     # 120 000 points: over max_points
                      [poly(40, 0, 640)]]),
        ((5, 6), []),                                                                # an image without annotations
        ((640, 640), [[rect(-1, -1, 641, 641)], [poly(9, -50, 700)], [rect(639, 639, 640, 640)], [rect(0, 0, 1, 640)]]),
        ((512, 1024), [[poly(12, 0, 1024), rect(1000.5, 500.5, 1030, 520)], {"counts": random_runs(rng, 1 << 19, 300)},
                       {"counts": [(1 << 19) - 1, 1]}, [rect(0, 0, 1024, 512)]]),
        (OVER_LIMIT, [[rect(1, 1, 100, 100)], {"counts": [1024 * 513]}]),            # valid = 0, the other images unaffected
    ]
    return [a for _, a in images], [s for s, _ in images]


@functools.lru_cache(maxsize=None)
def reference(out_hw, with_over_limit=True):
    ann, sizes = batch()
    if not with_over_limit:
        ann, sizes = ann[:-1], sizes[:-1]
    return R.coco_masks(ann, sizes, out_hw, MAX_POINTS, rasters_=_rasters()[:sum(len(a) for a in ann)])


@functools.lru_cache(maxsize=None)
def _rasters():
    ann, sizes = batch()
    return R.rasters(ann, sizes, MAX_POINTS)


def packed(ann, sizes):
    """the CSR arrays without the host wrapper's size check (the C ABI takes any sizes)"""
    from maskunet_amd.coco import pack_annotations
    return pack_annotations(ann, sizes)


def run_raw(p, out_hw, max_points=MAX_POINTS, masks=True):
    """raw mu_coco_masks on packed arrays -> dict of numpy outputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    Ho, Wo = out_hw
    B, A, P = p["sizes"].shape[0], p["ann_poly_offsets"].size - 1, p["poly_offsets"].size - 1
    dt = {"xy": torch.float64}
    ins = [Guarded(p[k].size, dt.get(k, torch.int32), p[k], k) for k in IN_KEYS]
    shapes = {"cover": ((B, Ho, Wo), torch.int64), "ids": ((B, Ho, Wo), torch.int32), "masks": ((A, Ho, Wo), torch.uint8),
              "area": ((A,), torch.int32), "valid": ((A,), torch.int32)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    assert lib.mu_coco_masks_supported(Ho, Wo, max_points) == 0
    nws = lib.mu_coco_masks_workspace_bytes(B, A, Ho, Wo)
    assert nws >= 0
    call("mu_coco_masks", *ins, B, A, P, p["xy"].size // 2, p["rle_counts"].size, Ho, Wo, max_points, outs["cover"], outs["ids"],
         outs["masks"] if masks else None, outs["area"], outs["valid"], Guarded(nws, torch.uint8, name="workspace"), nws)
    if not masks:
        outs["masks"].check()
        assert bool((outs["masks"].t == outs["masks"].sent).all())
    return {k: outs[k].host(shapes[k][0]) for k in OUT_KEYS}


def same(got, ref, keys=OUT_KEYS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        bad = np.argwhere(got[k] != ref[k])
        assert bad.size == 0, f"{k}: {len(bad)} differences, first at {bad[0].tolist()}: {got[k][tuple(bad[0])]} != {ref[k][tuple(bad[0])]}"


def test_reference_batch_has_the_cases():
    """the batch is what the docstring says: invalid rows, covered pixels, cover above 1, the tie polygon differs under fused arithmetic"""
    ann, sizes = batch()
    ref = reference((128, 128))
    first = np.cumsum([0] + [len(a) for a in ann])
    v = [ref["valid"][first[b]:first[b + 1]].tolist() for b in range(len(ann))]
    assert v[5] == [1, 1, 1, 0, 0, 0, 0, 0, 0, 1] and v[9] == [0, 0] and all(all(r) for b, r in enumerate(v) if b not in (5, 9))
    assert ref["cover"][4].max() >= 3 and ref["cover"][6].max() == 0 and ref["cover"][9].max() == 0
    a = ref["area"][first[4]:first[5]].tolist()
    assert a[1] == 12 * 12 + 14 * 14 - 6 * 6 and a[4] == 0 and a[7] == 0 and a[8] == 0 and a[9] == 33 * 31 and a[11] == 0
    assert ref["area"][first[7]] == 640 * 640 and ref["area"][first[8] + 3] == 1 << 19 and ref["area"][first[8] + 2] == 1


@pytest.mark.parametrize("out_hw", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_through_the_c_abi(out_hw):
    ann, sizes = batch()
    got = run_raw(packed(ann, sizes), out_hw)
    print(f"{out_hw}: area {got['area'].tolist()} valid {got['valid'].tolist()}")
    same(got, reference(out_hw))


@pytest.mark.parametrize("out_hw", OUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_through_coco_masks(out_hw):
    """the public interface: RLE counts as compressed strings, sizes checked on the host"""
    from maskunet_amd import CocoMasks, coco_masks
    from maskunet_amd.rle import rle_string_from_counts
    ann, sizes = batch()
    ann, sizes = list(ann[:-1]), list(sizes[:-1])
    as_string = lambda s: {"size": list(sz), "counts": rle_string_from_counts(s["counts"])} if isinstance(s, dict) and min(s["counts"]) >= 0 else s
    for b, sz in enumerate(sizes):
        ann[b] = [as_string(s) for s in ann[b]]
    r = coco_masks(ann, sizes, out_hw, masks=True, max_points=MAX_POINTS)
    assert isinstance(r, CocoMasks) and r.cover.dtype == torch.int64 and r.ids.dtype == torch.int32 and r.masks.dtype == torch.uint8
    got = {k: getattr(r, k).cpu().numpy() for k in OUT_KEYS}
    same(got, reference(out_hw, False))
    r2 = coco_masks(ann, sizes, out_hw, max_points=MAX_POINTS)
    assert r2.masks is None
    same({k: getattr(r2, k).cpu().numpy() for k in OUT_KEYS if k != "masks"}, reference(out_hw, False), [k for k in OUT_KEYS if k != "masks"])


def test_without_masks_and_twice():
    """masks = NULL leaves the other outputs unchanged; two calls are bit-identical"""
    ann, sizes = batch()
    p = packed(ann, sizes)
    a, b, c = run_raw(p, (128, 128)), run_raw(p, (128, 128)), run_raw(p, (128, 128), masks=False)
    same(b, a)
    same(c, a, ("cover", "ids", "area", "valid"))


def test_max_points_is_a_bound_not_a_hint():
    """(0,0) (3,0) (3,3) walks 16 + 16 + 16 points"""
    p = packed([[[[0, 0, 3, 0, 3, 3]], [[0, 0, 3, 0, 3, 3]]]], [(6, 6)])
    for mp, valid in ((48, 1), (47, 0), (1, 0)):
        got = run_raw(p, (6, 6), max_points=mp)
        same(got, R.coco_masks([[[[0, 0, 3, 0, 3, 3]], [[0, 0, 3, 0, 3, 3]]]], [(6, 6)], (6, 6), mp))
        assert got["valid"].tolist() == [valid, valid]


def test_no_annotations_at_all():
    got = run_raw(packed([[], []], [(5, 6), (480, 640)]), (128, 128))
    assert got["cover"].shape == (2, 128, 128) and not got["cover"].any() and not got["ids"].any() and got["area"].size == 0


def test_oversize_raises_in_the_wrapper():
    from maskunet_amd import coco_masks
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        coco_masks([[[rect(1, 1, 5, 5)]]], [OVER_LIMIT])
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        coco_masks([[[rect(1, 1, 5, 5)]]], [(8, 8)], out_hw=(256, 257))
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        coco_masks([[[rect(1, 1, 5, 5)]]], [(8, 8)], max_points=(1 << 21) + 1)


def test_bad_arguments_touch_nothing():
    from maskunet_amd import _lib
    lib = _lib.load()
    bufs = [Guarded(64, torch.int32) for _ in range(8)] + [Guarded(64, torch.float64), Guarded(64, torch.int64)]
    po, apo, rc, aro, iao, sz, area, valid, xy, cover = bufs
    ids = area
    args = lambda **kw: [kw.get("xy", xy.p), po.p, apo.p, rc.p, aro.p, kw.get("iao", iao.p), sz.p, kw.get("B", 1), kw.get("A", 1), 1, 4,
                         kw.get("n_counts", 0), kw.get("Ho", 4), kw.get("Wo", 4), kw.get("max_points", 100), kw.get("cover", cover.p), ids.p,
                         None, area.p, kw.get("valid", valid.p), None, 0, _lib.stream()]
    for kw in (dict(xy=None), dict(iao=None), dict(cover=None), dict(valid=None), dict(B=0), dict(B=-1), dict(A=-1), dict(n_counts=-1),
               dict(Ho=0), dict(Wo=-4), dict(max_points=0), dict(max_points=-1)):
        assert lib.mu_coco_masks(*args(**kw)) == -1, kw
    for kw in (dict(Ho=256, Wo=257), dict(Ho=65537, Wo=1), dict(max_points=(1 << 21) + 1)):
        assert lib.mu_coco_masks(*args(**kw)) == -2, kw
        assert lib.mu_coco_masks_supported(kw.get("Ho", 4), kw.get("Wo", 4), kw.get("max_points", 100)) == -2
    assert lib.mu_coco_masks_supported(256, 256, 1 << 21) == 0 and lib.mu_coco_masks_supported(1, 65536, 1) == 0
    torch.cuda.synchronize()
    for g in bufs:
        g.check("nothing may be written")
        assert bool((g.t == g.sent).all())


def as_instances(ids):
    """an Instances around an id map whose ids are 1..count per image: class 1, the table of the shared restatement"""
    from maskunet_amd import Instances
    r = table_from_ids(ids.cpu().numpy(), [[1] * 16] * ids.shape[0], 16)
    table, score, count, order = (torch.from_numpy(r[k]).to(ids.device) for k in ("table", "score", "count", "order"))
    return Instances((ids > 0).to(torch.int32), ids.contiguous(), table, score.float(), count, order)


def test_ids_feed_match_instances_and_cover_feeds_the_loss():
    from maskunet_amd import CrossEntropyLoss, coco_masks, instances_from_labels, match_instances
    ann, sizes = batch()
    ann, sizes = ann[:-1], sizes[:-1]
    r = coco_masks(ann, sizes, (128, 128), max_points=MAX_POINTS)
    ref = reference((128, 128), False)
    ref_ids = torch.from_numpy(ref["ids"]).to(DEV)
    pred = instances_from_labels((r.cover > 0).to(torch.int32), max_instances=16)
    m_dev, m_ref = match_instances(pred, as_instances(r.ids), 2), match_instances(pred, as_instances(ref_ids), 2)
    for f in ("det_valid", "det_gt", "det_iou", "gt_per_class", "pq_gt", "pq_iou", "pq_fp", "overflow", "pairs", "n_pairs"):
        assert torch.equal(getattr(m_dev, f), getattr(m_ref, f)), f
    assert int(m_dev.det_valid.sum()) > 0 and int((m_dev.det_gt > 0).sum()) > 0 and not bool(m_dev.overflow.any())
    assert r.cover.dtype == torch.int64 and 3 <= int(r.cover.max()) == int(ref["cover"].max()) < 8
    torch.manual_seed(0)
    logits = torch.randn(len(sizes), 8, 128, 128, device=DEV, requires_grad=True)             # cover stays below 8 in this batch
    loss = CrossEntropyLoss()(logits, r.cover)
    want = torch.nn.functional.cross_entropy(logits.detach().double().cpu(), torch.from_numpy(ref["cover"]))
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    loss.backward()
    assert bool(torch.isfinite(logits.grad).all())


def test_on_a_side_stream():
    """stream-ordered: launched on a non-default stream with no synchronisation between the upload, the call and what follows"""
    from maskunet_amd import coco_masks
    ann, sizes = batch()
    ann, sizes = ann[:5], sizes[:5]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = coco_masks(ann, sizes, (96, 80), masks=True, max_points=MAX_POINTS)
        total = r.cover.sum() + r.ids.sum()                                          # consumers on the same stream
    s.synchronize()
    ref = R.coco_masks(ann, sizes, (96, 80), MAX_POINTS, rasters_=_rasters()[:sum(len(a) for a in ann)])
    same({k: getattr(r, k).cpu().numpy() for k in OUT_KEYS}, ref)
    assert int(total) == int(ref["cover"].sum() + ref["ids"].sum())
