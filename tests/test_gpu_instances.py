"""GPU: instance extraction (mu_argmax_prob, mu_instances, maskunet_amd.instances) against the numpy restatement of its contract in
tests/_cc_reference.py.  Ids, counts, every table column and the score order are compared with == (one documented exception for the
order of the end-to-end case: check_order).  Memory discipline as in
test_gpu_conv_exact.py: outputs pre-filled with a sentinel, the workspace exactly the queried size, 4 KiB guard bands around every
buffer that must survive.

The one tolerance (probabilities and scores).  Measured on the CPU on the inputs of this file: the reference's own fp32 route (torch
softmax(x / 0.5) in fp32, then a numpy fp32 mean over each region) against float64 is off by at most 1.50e-07 (probabilities of the
arg-max tests; the fp32 region means of the score tests: 6.52e-08).  The gate is four times that; the factor covers the device's
fast exp and the 2^-24 fixed-point step, each of the order of the fp32 route's own rounding.  fp16 logits are exact in fp32, so the
same gate serves both dtypes."""
import functools

import numpy as np
import pytest
import torch

from tests import _cc_reference as R
from tests._device_buffers import Guarded, call

pytestmark = pytest.mark.gpu

FP32_ROUTE_ERROR = 1.50e-07          # measured, see the module docstring (measure_fp32_route_error() below prints it)
GATE = 4 * FP32_ROUTE_ERROR          # 6.0e-07

DEV = "cuda"


def run_instances(cls, prob, max_inst):
    """raw mu_instances on cls [B,H,W] (numpy) -> dict of numpy outputs; checks guards and untouched inputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, H, W = cls.shape
    i32, f32 = torch.int32, torch.float32
    g_cls = Guarded(B * H * W, i32, cls, "the class map")
    g_prob = Guarded(B * H * W, f32, prob, "prob") if prob is not None else None
    shapes = {"ids": ((B, H, W), i32), "table": ((B, max_inst, 8), i32), "score": ((B, max_inst), f32), "count": ((B,), i32),
              "order": ((B, max_inst), i32)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    nws = lib.mu_instances_workspace_bytes(B, H, W, max_inst)
    assert nws > 0 and nws % 4 == 0
    call("mu_instances", g_cls, g_prob, B, H, W, max_inst, *outs.values(), Guarded(nws // 4, i32, name="workspace"), nws)
    return {k: outs[k].host(shapes[k][0]) for k in shapes}


def grid_prob(shape, seed):
    """probabilities on a 2^-10 grid: their fixed-point sums and float64 means are exact, so equal scores are equal on both sides"""
    return (np.random.default_rng(seed).integers(1, 1025, shape) / 1024.0).astype(np.float32)


def check_order(got, ref, near_ties):
    """order == the reference's.  near_ties (the end-to-end case only, whose probabilities are not on a grid): the device sorts the fp32
    scores it returns, the reference its float64 means, and among thousands of instances some scores lie closer together than the two
    sides' rounding.  There the order must still be EXACTLY the stable descending sort of the returned scores, and may differ from the
    reference's only by swaps of instances whose reference scores are within 2 x GATE (each side's scores are within GATE of the
    truth, and sorting moves no value by more than the perturbation)."""
    if not near_ties:
        assert np.array_equal(got["order"], ref["order"])
        return
    for b in range(len(ref["count"])):
        K = min(int(ref["count"][b]), ref["order"].shape[1])
        g, r = got["order"][b], ref["order"][b]
        want = sorted(range(1, K + 1), key=lambda k: (-float(got["score"][b, k - 1]), k))
        assert g[:K].tolist() == want and (g[K:] == 0).all()
        diff = np.nonzero(g[:K] != r[:K])[0]
        gap = np.abs(ref["score"][b, g[diff] - 1] - ref["score"][b, r[diff] - 1])
        print(f"image {b}: {len(diff)} of {K} order positions differ from the float64 order, largest score gap there "
              f"{gap.max() if len(diff) else 0.0:.3e} (allowed {2 * GATE:.2e})")
        assert (gap <= 2 * GATE).all()


def compare(got, ref, overflow=False, near_ties=False):
    for b in range(len(ref["count"])):
        print(f"image {b}: count {got['count'][b]} (reference {ref['count'][b]}), "
              f"max score error {np.abs(got['score'][b] - ref['score'][b]).max():.3e} (gate {GATE:.2e})")
    if not overflow:
        assert (ref["count"] <= ref["table"].shape[1]).all(), "not meant as an overflow case"
    assert np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["ids"], ref["ids"])
    for j in range(8):
        assert np.array_equal(got["table"][:, :, j], ref["table"][:, :, j]), f"table column {j}"
    assert np.abs(got["score"].astype(np.float64) - ref["score"]).max() <= GATE
    check_order(got, ref, near_ties)


@functools.lru_cache(maxsize=None)
def _reference(name, with_prob, max_inst):
    g = R.patterns()[name] if name in R.patterns() else R.random_maps()[name][0]
    p = grid_prob(g.shape, 5) if with_prob else None
    ref = R.instances(g[None], None if p is None else p[None].astype(np.float64), max_inst)
    for v in ref.values():
        v.setflags(write=False)
    return g, p, ref


@pytest.mark.parametrize("name", sorted(R.patterns()))
def test_label_patterns(name):
    max_inst = 256 if name == "isolated" else 512
    g, p, ref = _reference(name, True, max_inst)
    if name in R.EXPECTED_COUNTS:
        assert ref["count"][0] == R.EXPECTED_COUNTS[name]
    if name == "full_256":
        assert ref["table"][0, 0, 1] == 65536
    compare(run_instances(g[None], p[None], max_inst), ref)


def test_isolated_pixels_overflow():
    g, p, ref = _reference("isolated", True, 64)
    got = run_instances(g[None], p[None], 64)
    assert got["count"][0] == 256 and got["ids"].max() == 256           # the id map is complete
    assert got["table"].shape[1] == 64 and (got["table"][0, :, 1] == 1).all()
    compare(got, ref, overflow=True)


@pytest.mark.parametrize("max_inst", [1, 2, 3])
def test_smallest_tables(max_inst):
    """the lower end of max_instances (1: a one-slot LDS layout; 3: not a power of two), with probabilities and more instances than rows"""
    g, p, ref = _reference("rand_16x16_c3", True, max_inst)
    assert ref["count"][0] == 29 and ref["table"].shape[1] == max_inst
    got = run_instances(g[None], p[None], max_inst)
    assert got["ids"].max() == 29
    compare(got, ref, overflow=True)


def test_noise_overflows_without_harm():
    g = np.random.default_rng(0).integers(0, 20, (1, 128, 128)).astype(np.int32)
    p = grid_prob(g.shape, 6)
    ref = R.instances(g, p.astype(np.float64), 1024)
    assert ref["count"][0] > 4096
    compare(run_instances(g, p, 1024), ref, overflow=True)


def test_ground_truth_scores_are_one():
    g, _, ref = _reference("rand_37x29_c5", False, 1024)
    got = run_instances(g[None], None, 1024)
    K = int(ref["count"][0])
    assert (got["score"][0, :K] == 1.0).all() and (got["score"][0, K:] == 0.0).all()
    assert np.array_equal(got["order"][0, :K], np.arange(1, K + 1))
    compare(got, ref)


def test_three_images_do_not_leak():
    P = R.patterns()
    gs = [np.zeros((32, 32), np.int32) for _ in range(3)]
    gs[0][:] = P["serpentine_32"]
    gs[1][:31, :31] = P["spirals"]
    gs[2][:16, :16] = P["isolated"]
    gs[2][16:, 16:] = P["checker_two_classes"]
    g = np.stack(gs)
    p = grid_prob(g.shape, 7)
    ref = R.instances(g, p.astype(np.float64), 512)
    assert len(set(ref["count"].tolist())) == 3
    compare(run_instances(g, p, 512), ref)


@pytest.mark.parametrize("name", sorted(R.random_maps()))
def test_random_maps(name):
    max_inst = R.random_maps()[name][1]
    g, p, ref = _reference(name, True, max_inst)
    assert ref["count"][0] == R.EXPECTED_COUNTS[name]
    compare(run_instances(g[None], p[None], max_inst), ref)


# ------------------------------------------------------------------------------------------------
# edges of the shared wave / workgroup helpers (csrc/wave_prims.h): N = 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025 pixels, i.e. one
# 64-lane chunk and one full turn of the 1024 threads (512 in rle.hip), each one short, exact and one over
EDGE_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (7, 73), (16, 32), (19, 27), (31, 33), (32, 32), (25, 41)]


def last_segment_start(n, waves):
    """first element of the last non-empty wave segment of [0, n): every wave owns ceil(n / (64 waves)) chunks of 64"""
    seg = -(-n // (waves * 64)) * 64
    return (n - 1) // seg * seg


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixel_counts_at_chunk_and_segment_edges(shape):
    """per-pixel noise (many roots in every chunk).  Image 0: foreground forced on the last pixel and on the first pixel of the last
    wave's segment; image 1: those two pixels in a class of their own, so each is the root of its component"""
    H, W = shape
    N = H * W
    edge = [last_segment_start(N, 16), N - 1]
    g = np.random.default_rng(N).integers(0, 3, (2, N)).astype(np.int32)
    g[0, edge] = np.maximum(g[0, edge], 1)
    g[1, edge] = 3
    g = g.reshape(2, H, W)
    p = grid_prob(g.shape, N)
    ref = R.instances(g, p.astype(np.float64), 1024)
    assert (ref["ids"].reshape(2, N)[:, edge] > 0).all() and (ref["table"][1, :, 0] == 3).any()
    compare(run_instances(g, p, 1024), ref)


# ------------------------------------------------------------------------------------------------
# arg-max pass
def argmax_case(C, seed=0, M=1000):
    """logits [M, C] on a grid of 1/8 after a ReLU (exact ties at 0 are the common case), with all-zero rows and repeated maxima"""
    rng = np.random.default_rng(seed + C)
    x = np.maximum(rng.integers(-24, 41, (M, C)) / 8.0, 0.0)
    x[::7] = 0.0                                           # all-zero rows: class 0 wins
    for r in range(3, M, 11):                              # the maximum repeated: the first index wins
        if r % 7 == 0:
            continue
        j = rng.integers(0, C, 2)
        x[r, j] = x[r].max() + 0.125
    return x


def run_argmax(x, dtype, layout, want_prob=True, temperature=0.5):
    from maskunet_amd import _lib
    M, C = x.shape
    tdt = torch.float16 if dtype == "fp16" else torch.float32
    if layout == "nchw":                                   # [B=2, C, M/2]
        B, inner = 2, M // 2
        data = np.ascontiguousarray(x.reshape(B, inner, C).transpose(0, 2, 1))
        n, args = data.size, (inner, C * inner, inner, 1)
    else:                                                  # [M, Cp], padded channels hold a LARGER value that must not be read
        Cp = (C + 31) // 32 * 32
        data = np.full((M, Cp), 100.0)
        data[:, :C] = x
        n, args = data.size, (M, 0, 1, Cp)
    g_x = Guarded(n, tdt, data, "logits")
    g_cls = Guarded(M, torch.int32, name="cls")
    g_prob = Guarded(M, torch.float32, name="prob")
    call("mu_argmax_prob", g_x, M, C, *args, 1.0 / temperature, g_cls, g_prob if want_prob else None, _lib.dt(tdt))
    g_prob.check()
    return g_cls.host(), g_prob.host()


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("C", [2, 19, 150])
def test_argmax_prob(C, dtype, layout):
    x = argmax_case(C)
    ref_cls, ref_prob = R.argmax_prob(x)
    assert (ref_cls[::7] == 0).all()
    cls, prob = run_argmax(x, dtype, layout)
    err = np.abs(prob.astype(np.float64) - ref_prob).max()
    print(f"C={C} {dtype} {layout}: max probability error {err:.3e} (gate {GATE:.2e})")
    assert np.array_equal(cls, ref_cls)
    assert err <= GATE


def test_argmax_layouts_agree_bit_for_bit_and_prob_is_optional():
    x = argmax_case(150, seed=1)
    a = run_argmax(x, "fp16", "nchw")
    b = run_argmax(x, "fp16", "nhwc")
    c = run_argmax(x, "fp32", "nchw")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert np.array_equal(a[1].view(np.int32), c[1].view(np.int32))
    cls, prob = run_argmax(x, "fp32", "nhwc", want_prob=False)
    assert np.array_equal(cls, a[0]) and (prob == -777.0).all()          # still the sentinel


def measure_fp32_route_error():
    """CPU: error of the reference's fp32 route against float64 on the inputs of this file (the source of FP32_ROUTE_ERROR)."""
    e_prob = 0.0
    for C in (2, 19, 150):
        for seed in (0, 1):
            x = argmax_case(C, seed)
            p32 = torch.softmax(torch.from_numpy(x).float() / 0.5, dim=1).max(1).values.numpy()
            e_prob = max(e_prob, float(np.abs(p32.astype(np.float64) - R.argmax_prob(x)[1]).max()))
    e_score = 0.0
    g = R.random_maps()["blocky_128_c19"][0]
    p = np.random.default_rng(3).random(g.shape, dtype=np.float32)
    ids, regions = R.label_image(g)
    for pix in regions:
        v = p.reshape(-1)[pix]
        e_score = max(e_score, abs(float(v.mean(dtype=np.float32)) - float(v.astype(np.float64).mean())))
    print(f"fp32 route vs float64: probabilities {e_prob:.3e}, region means {e_score:.3e}")
    return max(e_prob, e_score)


# ------------------------------------------------------------------------------------------------
# scores
def test_scores_against_float64_means_and_reproducible():
    g = R.random_maps()["blocky_128_c19"][0]
    p = np.random.default_rng(3).random(g.shape, dtype=np.float32)          # not on a grid
    ref = R.instances(g[None], p[None].astype(np.float64), 1024)
    a = run_instances(g[None], p[None], 1024)
    b = run_instances(g[None], p[None], 1024)
    K = int(ref["count"][0])
    err = np.abs(a["score"].astype(np.float64) - ref["score"]).max()
    print(f"max score error {err:.3e} (gate {GATE:.2e})")
    assert err <= GATE
    assert np.array_equal(a["score"].view(np.int32), b["score"].view(np.int32)) and np.array_equal(a["order"], b["order"])
    # the order is the stable descending sort of the scores that came back
    want = sorted(range(1, K + 1), key=lambda k: (-float(a["score"][0, k - 1]), k))
    assert a["order"][0, :K].tolist() == want and (a["order"][0, K:] == 0).all()
    assert np.array_equal(a["ids"], ref["ids"]) and np.array_equal(a["table"], ref["table"])


def test_equal_scores_keep_id_order():
    g = R.random_maps()["rand_37x29_c5"][0]
    p = np.full(g.shape, 0.3, np.float32)
    got = run_instances(g[None], p[None], 1024)
    K = int(got["count"][0])
    assert K > 100 and len(set(got["score"][0, :K].tolist())) == 1
    assert abs(float(got["score"][0, 0]) - float(np.float32(0.3))) <= GATE
    assert np.array_equal(got["order"][0, :K], np.arange(1, K + 1))


# ------------------------------------------------------------------------------------------------
# end to end
E2E_MAX_INSTANCES = 4096


@functools.lru_cache(maxsize=None)
def _model_output():
    from tests import _gpu_checks as G
    rec = G.load_golden("unet1_c150_b2_eval")
    B, c_out, seed = int(rec["B"]), int(rec["c_out"]), int(rec["seed"])
    assert (B, c_out) == (2, 150)
    model, _, _, x, _ = G.build_unet(c_out, False, seed, torch.float16, False, B)
    with torch.no_grad():
        out = model(x.to(DEV))
    assert tuple(out.shape) == (2, 150, 128, 128)
    host = out.detach().cpu().double().numpy().copy()
    cls, prob = R.argmax_prob(host.transpose(0, 2, 3, 1))
    return out, cls, prob, R.instances(cls, prob, E2E_MAX_INSTANCES)


def _compare_result(res, cls, prob, ref):
    got = {"ids": res.ids.cpu().numpy(), "table": res.table.cpu().numpy(), "score": res.scores.cpu().numpy(),
           "count": res.count.cpu().numpy(), "order": res.order.cpu().numpy()}
    assert np.array_equal(res.classes.cpu().numpy(), cls)
    err = np.abs(res.prob.cpu().numpy().astype(np.float64) - prob).max()
    print(f"max probability error {err:.3e} (gate {GATE:.2e})")
    assert err <= GATE
    compare(got, ref, overflow=bool((ref["count"] > E2E_MAX_INSTANCES).any()), near_ties=True)
    return got


def test_predict_instances_end_to_end():
    import maskunet_amd
    from maskunet_amd.losses import _nhwc_source
    out, cls, prob, ref = _model_output()
    assert ref["count"].min() > 0
    assert _nhwc_source(out) is not None, "the module output should still carry its NHWC source"
    res = maskunet_amd.predict_instances(out, max_instances=E2E_MAX_INSTANCES)
    a = _compare_result(res, cls, prob, ref)
    detached = out.clone()
    assert _nhwc_source(detached) is None
    res2 = maskunet_amd.predict_instances(detached, max_instances=E2E_MAX_INSTANCES)
    b = _compare_result(res2, cls, prob, ref)
    assert torch.equal(res.prob.view(torch.int32), res2.prob.view(torch.int32))
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k

    # the reference's sorted(...)[:max_queries]
    ids, sc = res.top(50)
    K = min(int(ref["count"][0]), 50)
    assert ids.shape == (2, 50) and np.array_equal(ids.cpu().numpy(), a["order"][:, :50])
    assert torch.equal(sc[0, :K], res.scores[0][(ids[0, :K] - 1).long()])
    dicts = res.to_reference(0, max_queries=50)
    assert len(dicts) == K and set(dicts[0]) == {"bbox", "category_id", "score", "mask"}
    for d, k in zip(dicts, a["order"][0, :K]):
        row = ref["table"][0, k - 1]
        assert d["category_id"] == row[0] and d["mask"].sum() == row[1] and d["mask"].dtype == np.bool_
        assert d["mask"][row[6] // 128, row[6] % 128]
        assert d["bbox"] == [float(row[2]), float(row[3]), float(row[4] - row[2]), float(row[5] - row[3])]
        assert abs(d["score"] - ref["score"][0, k - 1]) <= GATE
    assert all(dicts[i]["score"] >= dicts[i + 1]["score"] for i in range(K - 1))


def test_generate_instance_mask_feeds_the_contrastive_loss():
    import maskunet_amd
    g = np.stack([R.random_maps()["blocky_128_c19"][0], np.roll(R.random_maps()["blocky_128_c19"][0], 5, 1)])
    labels = torch.from_numpy(g).long().to(DEV)
    mask = maskunet_amd.generate_instance_mask(labels)
    assert mask.dtype == torch.int32 and np.array_equal(mask.cpu().numpy(), R.class_rank_mask(g))
    one = maskunet_amd.generate_instance_mask(labels[0].int())
    assert one.shape == (128, 128) and torch.equal(one, mask[0])
    small = maskunet_amd.generate_instance_mask(labels, max_instances=32)
    assert np.array_equal(small.cpu().numpy(), R.class_rank_mask(g, 32)) and int(small.min()) == -1
    r = maskunet_amd.instances_from_labels(labels)
    assert bool((r.scores[0, :int(r.count[0])] == 1).all())
    feats = torch.randn(2, 16, 128, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(0), requires_grad=True)
    loss = maskunet_amd.InstanceContrastiveLoss()(feats, mask.long())
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(feats.grad).all())
