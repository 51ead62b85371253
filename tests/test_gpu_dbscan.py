"""GPU: instances from the embedding head (mu_dbscan_instances, maskunet_amd.instances_from_embeddings) against the goldens that the
reference produced with sklearn (tests/golden/dbscan/*.npz) and against the float64 restatement of the contract in
tests/_dbscan_reference.py.  Everything is compared with ==: ids, counts, every table column, scores (exactly 1.0), order (ascending
ids).  There is no tolerance: the neighbour decision is fp64 on both sides, the real-valued inputs keep every same-class pair at
least 1e-6 (relative, in d^2) away from the threshold -- ten orders of magnitude more than fp64 rounding of a 64-term sum -- and the
grid inputs are exact in every format.  Memory discipline as in test_gpu_instances.py: outputs pre-filled with a sentinel, the
workspace exactly the queried size, 4 KiB guard bands around every buffer, inputs verified untouched."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _dbscan_reference as R
from tests._device_buffers import Guarded, call
from tests.conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "dbscan")
pytestmark = pytest.mark.gpu

DEV = "cuda"
T_ROWS, T_COLS = 256, 64             # DB_TR / DB_TC of csrc/instances.hip: points per workgroup, points per LDS chunk
PAD = 100.0                          # value of the padded NHWC channels: reading one would move every distance


def run_dbscan(cls, emb, num_classes, eps=0.5, min_samples=5, max_inst=64, layout="nchw", dtype=None):
    """raw mu_dbscan_instances on cls [B,H,W], emb [B,H,W,D] (numpy) -> dict of numpy outputs; checks guards and untouched inputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, H, W = cls.shape
    D = emb.shape[-1]
    tdt = {np.dtype(np.float16): torch.float16, np.dtype(np.float32): torch.float32}[np.dtype(dtype or emb.dtype)]
    if layout == "nchw":
        data = emb.transpose(0, 3, 1, 2)
        strides = (H * W, D * H * W, H * W, 1)
    else:                                                  # rows padded to 32 channels, as the module's NHWC tensors
        Dp = (D + 31) // 32 * 32
        data = np.full((B, H, W, Dp), PAD, emb.dtype)
        data[..., :D] = emb
        strides = (B * H * W, 0, 1, Dp)
    i32, f32 = torch.int32, torch.float32
    g_cls = Guarded(cls.size, i32, cls, "the class map")
    g_emb = Guarded(data.size, tdt, data, "the embedding tensor")
    shapes = {"ids": ((B, H, W), i32), "table": ((B, max_inst, 8), i32), "score": ((B, max_inst), f32), "count": ((B,), i32),
              "order": ((B, max_inst), i32)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    nws = lib.mu_dbscan_workspace_bytes(B, H, W, num_classes, max_inst)
    assert nws > 0 and nws % 4 == 0
    call("mu_dbscan_instances", g_cls, g_emb, B, H, W, D, *strides, _lib.dt(tdt), num_classes, float(eps), int(min_samples), max_inst,
         *outs.values(), Guarded(nws // 4, i32, name="workspace"), nws)
    return {k: outs[k].host(shapes[k][0]) for k in shapes}


def compare(got, ref, overflow=False):
    print(f"count {got['count'].tolist()} (reference {ref['count'].tolist()})")
    K = ref["table"].shape[1]
    if not overflow:
        assert (ref["count"] <= K).all(), "not meant as an overflow case"
    assert np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["ids"], ref["ids"])
    for j in range(8):
        assert np.array_equal(got["table"][:, :, j], ref["table"][:, :, j]), f"table column {j}"
    for b in range(len(ref["count"])):
        k = min(int(ref["count"][b]), K)
        assert (got["score"][b, :k] == 1.0).all() and (got["score"][b, k:] == 0.0).all()
        assert np.array_equal(got["order"][b, :k], np.arange(1, k + 1)) and (got["order"][b, k:] == 0).all()


def same(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


@functools.lru_cache(maxsize=None)
def _clustered(seed, H, W, D, sizes, min_samples=5, max_inst=64):
    cls, emb = R.clustered_case(seed, H, W, D, list(sizes))
    nc = len(sizes) + 1
    ref = R.instances(cls[None], emb[None], nc, 0.5, min_samples, max_inst)
    for v in (cls, emb, *ref.values()):
        v.setflags(write=False)
    return cls, emb, nc, ref


# ------------------------------------------------------------------------------------------------
# the reference's own results
@pytest.mark.parametrize("name", ["dbscan_16x16_d16", "dbscan_32x32_d16", "dbscan_20x24_d3_fp16"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_goldens(name, layout):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    nc, eps, ms = int(g["num_classes"]), float(g["eps"]), int(g["min_samples"])
    got = run_dbscan(g["cls"][None], g["emb"][None], nc, eps, ms, 64, layout)
    assert np.array_equal(got["ids"][0], g["ids"])                       # sklearn's result
    assert got["count"][0] == len(g["score"])
    for k in range(len(g["score"])):
        row = got["table"][0, k]
        assert row[0] == g["category_id"][k] and got["score"][0, k] == g["score"][k] == 1.0
        assert [row[2], row[3], row[4] - row[2], row[5] - row[3]] == g["bbox"][k].tolist()
    compare(got, R.instances(g["cls"][None], g["emb"][None], nc, eps, ms, 64))


# ------------------------------------------------------------------------------------------------
# tile edges
@pytest.mark.parametrize("sizes", [(T_ROWS - 1, T_ROWS, T_ROWS + 1, 0, 4, 5), (2 * T_ROWS + 1, T_COLS - 1, T_COLS, T_COLS + 1),
                                   (1024,)], ids=["T-1_T_T+1_0_4_5", "2T+1_chunk_edges", "one_class_fills_32x32"])
def test_class_sizes_straddle_the_tiles(sizes):
    """T-1, T, T+1, 2T+1 points per class for the row tile T, the column chunk's edges, a class that fills the image, and classes of
    0, min_samples - 1 and exactly min_samples points (tight blobs: the last is one cluster, the one before all noise)"""
    cls, emb, nc, ref = _clustered(31, 32, 32, 16, sizes)
    if 5 in sizes:
        c4, c5 = sizes.index(4) + 1, sizes.index(5) + 1
        assert (ref["ids"][0][cls == c4] == 0).all() and len(set(ref["ids"][0][cls == c5].tolist())) == 1
        assert (ref["ids"][0][cls == c5] > 0).all() and c5 in ref["table"][0, :, 0]
    assert ref["count"][0] >= 2
    compare(run_dbscan(cls[None], emb[None], nc), ref)


def test_background_only_and_one_pixel_per_class():
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((1, 8, 8, 16)).astype(np.float32)
    bg = np.zeros((1, 8, 8), np.int32)
    got = run_dbscan(bg, emb, 19)
    assert got["count"][0] == 0 and (got["ids"] == 0).all() and (got["table"] == 0).all() and (got["order"] == 0).all()
    one = (1 + rng.permutation(64)).reshape(1, 8, 8).astype(np.int32)
    got = run_dbscan(one, emb, 65)
    assert got["count"][0] == 0 and (got["ids"] == 0).all()                 # every class is below min_samples
    ref = R.instances(one, emb, 65, 0.5, 1, 64)                             # min_samples = 1: every pixel is its own cluster
    assert ref["count"][0] == 64 and np.array_equal(ref["ids"][0], one[0])
    compare(run_dbscan(one, emb, 65, min_samples=1), ref)
    compare(run_dbscan(one, emb, 1024, min_samples=1), ref)                  # the upper end of num_classes


@pytest.mark.parametrize("nc", [64, 65, 130])
def test_class_counts_across_the_scan_turns(nc):
    """segment starts and tile offsets are scanned 64 classes per turn (csrc/wave_prims.h): points in classes 1, 63, 64 (where it exists)
    and the last one, every other class empty"""
    sizes = [0] * (nc - 1)
    for c, n in ((1, 40), (63, 70), (64, 33), (nc - 1, 50)):
        if c < nc:
            sizes[c - 1] = n
    cls, emb, _, ref = _clustered(60 + nc, 16, 16, 4, tuple(sizes))
    assert {c for c in (1, 63, 64, nc - 1) if c < nc} == set(ref["table"][0, :ref["count"][0], 0].tolist())
    compare(run_dbscan(cls[None], emb[None], nc), ref)


def test_sixty_four_classes_in_one_chunk_then_one_class():
    """the counting sort by class: in the first 64-pixel chunk every lane is a class of its own, the second chunk is one class"""
    emb = (8.0 * np.arange(128, dtype=np.float32)).reshape(1, 8, 16, 1)          # far apart: with min_samples = 1 every pixel is a cluster
    cls = np.concatenate([1 + np.random.default_rng(8).permutation(64), np.full(64, 7)]).reshape(1, 8, 16).astype(np.int32)
    ref = R.instances(cls, emb, 65, 0.5, 1, 128)
    assert ref["count"][0] == 128 and ref["table"][0, :, 0].tolist() == sorted(cls.reshape(-1).tolist())
    compare(run_dbscan(cls, emb, 65, min_samples=1, max_inst=128), ref)


# ------------------------------------------------------------------------------------------------
# the rules
@pytest.mark.parametrize("D", [2, 16])
def test_pairs_exactly_at_eps_are_neighbours(D):
    """coordinates on multiples of 1/8, eps = 0.5: d^2 is exact and some pairs sit at d == eps.  Restatement only."""
    cls, emb = R.grid_case(21, 16, 16, D, [100, 80, 5, 4], 28 if D == 2 else 24)
    ties = 0
    for c in range(1, 5):
        ties += int((R.neighbours(emb.reshape(256, D)[cls.reshape(-1) == c], 0.5)[1] == 0.25).sum())
    assert ties >= 40
    ref = R.instances(cls[None], emb[None], 5, 0.5, 5, 64)
    strict = R.instances(cls[None], emb[None], 5, np.nextafter(np.float32(0.5), np.float32(0)), 5, 64)
    assert not np.array_equal(ref["ids"], strict["ids"]), "the ties must matter"
    assert ref["count"][0] >= 2
    a = run_dbscan(cls[None], emb[None], 5)
    compare(a, ref)
    same(a, run_dbscan(cls[None], emb[None].astype(np.float16), 5))
    compare(run_dbscan(cls[None], emb[None], 5, eps=float(np.nextafter(np.float32(0.5), np.float32(0)))), strict)


def test_shared_border_point_and_chain_root():
    """1-D by hand (tests/test_dbscan_host.py): 0.85 is a border point of two clusters and the first pixel of the first; min_samples 4"""
    x = np.array([0.85, 0.0, 0.0, 0.0, 0.4, 1.3, 1.7, 1.7, 1.7], np.float32)
    for flip in (False, True):
        emb = np.full((1, 4, 4, 1), 50.0, np.float32)
        emb.reshape(-1)[:9] = 1.7 - x if flip else x
        cls = np.zeros((1, 4, 4), np.int32)
        cls.reshape(-1)[:9] = 2
        got = run_dbscan(cls, emb, 3, min_samples=4)
        assert got["ids"].reshape(-1)[:9].tolist() == [1, 1, 1, 1, 1, 2, 2, 2, 2] and got["count"][0] == 2
        assert got["table"][0, 0].tolist() == [2, 5, 0, 0, 3, 1, 0, 1] and got["table"][0, 1].tolist() == [2, 4, 0, 1, 3, 2, 5, 2]
        compare(got, R.instances(cls, emb, 3, 0.5, 4, 64))
    cls, emb, nc, ref = _clustered(11, 16, 16, 16, (60, 3, 45, 0, 30))
    cov = R.rule_coverage(cls, emb, nc)
    assert cov["shared_border"] and cov["root_not_first"] and cov["noise"] and cov["two_clusters"]
    compare(run_dbscan(cls[None], emb[None], nc), ref)


@pytest.mark.parametrize("D", [1, 3, 16, 32, 64])
def test_embedding_widths(D):
    cls, emb, nc, ref = _clustered(40 + D, 16, 16, D, (70, 3, 45, 0, 30))
    assert ref["count"][0] >= 2
    a = run_dbscan(cls[None], emb[None], nc)
    compare(a, ref)
    same(a, run_dbscan(cls[None], emb[None], nc, layout="nhwc"))


def test_layouts_and_dtypes_agree():
    cls, emb, nc, _ = _clustered(11, 16, 16, 16, (60, 3, 45, 0, 30))
    h = emb.astype(np.float16)
    ref = R.instances(cls[None], h[None], nc, 0.5, 5, 64)
    assert ref["count"][0] >= 2
    a = run_dbscan(cls[None], h[None], nc, layout="nchw")
    compare(a, ref)
    same(a, run_dbscan(cls[None], h[None], nc, layout="nhwc"))
    same(a, run_dbscan(cls[None], h[None].astype(np.float32), nc, layout="nchw"))
    same(a, run_dbscan(cls[None], h[None].astype(np.float32), nc, layout="nhwc"))


def test_three_images_equal_three_calls():
    cases = [_clustered(s, 16, 16, 16, sz) for s, sz in ((11, (60, 3, 45, 0, 30)), (52, (0, 100, 0, 90, 5)), (53, (30, 30, 30, 30, 30)))]
    cls = np.stack([c[0] for c in cases])
    emb = np.stack([c[1] for c in cases])
    got = run_dbscan(cls, emb, 6)
    assert len(set(got["count"].tolist())) >= 2
    for b, c in enumerate(cases):
        compare({k: v[b:b + 1] for k, v in got.items()}, c[3])
        same({k: v[b:b + 1] for k, v in got.items()}, run_dbscan(cls[b:b + 1], emb[b:b + 1], 6))
    same(got, run_dbscan(cls, emb, 6, layout="nhwc"))


def test_values_outside_the_class_range_are_background():
    cls, emb, nc, _ = _clustered(11, 16, 16, 16, (60, 3, 45, 0, 30))
    wild = cls.copy()
    wild[cls == 0] = np.random.default_rng(5).choice([-1, -7, nc, nc + 1, 1 << 20, -(1 << 31)], int((cls == 0).sum()))
    wild[cls == 5] = 7                                                  # with num_classes = 4 below, classes 4.. are background
    ref = R.instances(wild[None], emb[None], 4, 0.5, 5, 64)
    assert ref["count"][0] >= 2 and (ref["ids"][0][wild >= 4] == 0).all()
    got = run_dbscan(wild[None], emb[None], 4)
    compare(got, ref)
    clean = np.where((wild >= 1) & (wild < 4), wild, 0).astype(np.int32)
    same(got, run_dbscan(clean[None], emb[None], 4))


def test_more_instances_than_rows():
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((1, 8, 8, 16)).astype(np.float32)
    one = (1 + rng.permutation(64)).reshape(1, 8, 8).astype(np.int32)
    for max_inst in (1, 3, 16):
        ref = R.instances(one, emb, 65, 0.5, 1, max_inst)
        got = run_dbscan(one, emb, 65, min_samples=1, max_inst=max_inst)
        assert got["count"][0] == 64 and got["ids"].max() == 64 and got["table"].shape[1] == max_inst
        compare(got, ref, overflow=True)


def test_two_launches_are_bit_identical():
    cls, emb, nc, ref = _clustered(31, 32, 32, 16, (2 * T_ROWS + 1, T_COLS - 1, T_COLS, T_COLS + 1))
    a = run_dbscan(cls[None], emb[None], nc)
    same(a, run_dbscan(cls[None], emb[None], nc))
    compare(a, ref)


# ------------------------------------------------------------------------------------------------
# end to end
def test_instances_from_embeddings_end_to_end():
    import maskunet_amd
    from maskunet_amd.losses import _nhwc_source
    from oracle import maskunet_oracle as O
    hw, c_out, B, seed = 64, 19, 2, 710
    model = maskunet_amd.UNet(3, c_out, 16, hw=hw)
    model.load_state_dict(O.make_params(O.unet_state_shapes(3, c_out, True, hw=hw), seed))
    model.to(DEV).eval()
    model.set_keep_masks(O.make_keeps(seed + 1, B, hw))
    x, _ = O.make_inputs(seed + 2, B, c_out, hw)
    with torch.no_grad():
        sem, _, emb = model(x.to(DEV))
    assert tuple(sem.shape) == (B, c_out, hw, hw) and tuple(emb.shape) == (B, 16, hw, hw)
    assert _nhwc_source(sem) is not None and _nhwc_source(emb) is not None
    res = maskunet_amd.instances_from_embeddings(sem, emb, max_instances=256)
    pred = maskunet_amd.predict_instances(sem)
    assert torch.equal(res.classes, pred.classes) and torch.equal(res.prob.view(torch.int32), pred.prob.view(torch.int32))
    got = {"ids": res.ids.cpu().numpy(), "table": res.table.cpu().numpy(), "score": res.scores.cpu().numpy(),
           "count": res.count.cpu().numpy(), "order": res.order.cpu().numpy()}
    ref = R.instances(res.classes.cpu().numpy(), emb.cpu().numpy().transpose(0, 2, 3, 1), c_out, 0.5, 5, 256)
    compare(got, ref, overflow=bool((ref["count"] > 256).any()))
    res2 = maskunet_amd.instances_from_embeddings(sem.clone(), emb.clone(), max_instances=256)
    assert _nhwc_source(emb.clone()) is None
    for a, b in ((res.classes, res2.classes), (res.ids, res2.ids), (res.table, res2.table), (res.count, res2.count),
                 (res.order, res2.order), (res.scores.view(torch.int32), res2.scores.view(torch.int32)),
                 (res.prob.view(torch.int32), res2.prob.view(torch.int32))):
        assert torch.equal(a, b)
    res3 = maskunet_amd.instances_from_embeddings(res.classes.long(), emb, num_classes=c_out, max_instances=256)
    assert res3.prob is None and torch.equal(res3.ids, res.ids) and torch.equal(res3.table, res.table)
    ids, sc = res.top(50)
    assert ids.shape == (B, 50) and torch.equal(ids, res.order[:, :50])
    dicts = res.to_reference(0, max_queries=50)
    assert len(dicts) == min(int(ref["count"][0]), 50)
    for k, d in enumerate(dicts):
        row = ref["table"][0, k]
        assert d["category_id"] == row[0] and d["score"] == 1.0 and d["mask"].sum() == row[1]
        assert d["bbox"] == [float(row[2]), float(row[3]), float(row[4] - row[2]), float(row[5] - row[3])]
