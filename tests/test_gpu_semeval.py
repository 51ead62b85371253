"""GPU: semantic evaluation in one sweep (mu_sem_eval, maskunet_amd.metrics) against the float64 restatement of its contract in
tests/_semeval_reference.py, which tests/test_semeval_host.py pins to the reference-generated fixtures and to scikit-learn.

Integer outputs (img_counts, confusion, cls, the loss counts) are compared with ==.  The two tolerances are the existing ones:
the per-image loss sums within LOSS_TOL of tests/test_gpu_loss_edges.py (relative to max(1, |ref|), against ce_rows on inputs rounded
to the dtype) and the probabilities within GATE of tests/test_gpu_instances.py (absolute, against float64).  Memory discipline as
everywhere in the post-processing tests: every buffer between guard bands, outputs pre-filled with a sentinel, the workspace exactly
the queried size.  Every test prints its worst error next to its bound."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _semeval_reference as R
from tests._device_buffers import Guarded, call
from tests.test_gpu_instances import GATE, argmax_case
from tests.test_gpu_loss_edges import LOSS_TOL

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TDT = {"fp32": torch.float32, "fp16": torch.float16}
B = 3
# (C, Cp) of the vector path.  MU_SEM_EVAL_LDS_MAX_C = 192 (pinned to the header in test_semeval_host.py): (192, 192) is the last
# class count with the confusion counters in LDS, (193, 200) the first on the global-atomic fallback.  Rows of up to 3 x 16 vectors
# stay in registers (fp16: C <= 384, fp32: C <= 192), so fp32 takes the two-pass rows from 193 on and fp16 at (400, 400).
PAIRS = [(2, 8), (19, 32), (128, 128), (129, 136), (150, 160), (192, 192), (193, 200), (300, 304), (400, 400)]
# pixels per image: the single-pixel image, less than one row batch, two workgroups per image with a tail (1000 > 512), and one past
# a multiple of every row batch of the vector path (64, 128 and 256 rows)
PIXELS = [1, 63, 1000, 257]


@functools.lru_cache(maxsize=None)
def case(C, HW, ignore, seed=0):
    """(x [B,HW,C] float64 on the 1/8 grid of argmax_case (exact in fp16; ties are the common case), labels [B,HW], restatement).
    Labels hold 0 and C - 1, the ignore label, the out-of-range values C and -1, and image 1 is wholly void."""
    M = B * HW
    rng = np.random.default_rng(1000 * C + HW + seed)
    x = argmax_case(C, seed, M).reshape(B, HW, C)
    t = rng.integers(0, C, (B, HW)).astype(np.int64)
    kind = rng.random((B, HW))
    t[kind < 0.10] = ignore
    t[(kind >= 0.10) & (kind < 0.15)] = C
    t[(kind >= 0.15) & (kind < 0.20)] = -1
    t[1] = np.where(kind[1] < 0.5, ignore, np.where(kind[1] < 0.75, C, -1))
    t[0, 0], t[2, -1] = 0, C - 1
    ref = R.sem_eval(x, t, C, ignore)
    assert ref["img_loss"][1].tolist() == [0.0, 0.0] and ref["img_counts"][1, 1].sum() == HW and not ref["img_counts"][1, [0, 2]].any()
    assert ref["confusion"][C].sum() >= HW
    for a in (x, t, *ref.values()):
        a.setflags(write=False)
    return x, t, ref


def run(x, t, C, Cp, dtype, layout="nhwc", ignore=255, want_cls=True, want_prob=True, conf=None, temperature=0.5):
    """raw mu_sem_eval; returns the outputs as numpy arrays (and the Guarded confusion buffer for a second call)"""
    from maskunet_amd import _lib
    lib = _lib.load()
    nb, HW = t.shape
    M, tdt = nb * HW, TDT[dtype]
    if layout == "nchw":
        data = np.ascontiguousarray(x.transpose(0, 2, 1))                      # [B, C, HW]
        args = (HW, C * HW, HW, 1)
    else:                                                                       # [M, Cp]: padded channels hold a LARGER value
        data = np.full((M, Cp), 100.0)
        data[:, :C] = x.reshape(M, C)
        args = (M, 0, 1, Cp)
    g_x = Guarded(data.size, tdt, data, "logits")
    g_t = Guarded(M, torch.int64, np.array(t), "labels")
    g_counts = Guarded(nb * 3 * C, torch.int32, name="img_counts")
    g_loss = Guarded(nb * 2, torch.float64, name="img_loss")
    if conf is None:
        conf = Guarded((C + 1) * C, torch.int64, name="confusion")
        conf.t.zero_()
    g_cls = Guarded(M, torch.int32, name="cls")
    g_prob = Guarded(M, torch.float32, name="prob")
    nws = lib.mu_sem_eval_workspace_bytes(nb, HW, C)
    assert nws > 0 and nws % 8 == 0
    call("mu_sem_eval", g_x, g_t, nb, HW, C, *args, ignore, 1.0 / temperature, g_counts, g_loss, conf, g_cls if want_cls else None,
         g_prob if want_prob else None, Guarded(nws // 8, torch.float64, name="workspace"), nws, _lib.dt(tdt))
    g_cls.check()
    g_prob.check()
    g_counts.all_written()
    g_loss.all_written()
    return {"img_counts": g_counts.host((nb, 3, C)), "img_loss": g_loss.host((nb, 2)), "confusion": conf.host((C + 1, C)),
            "cls": g_cls.host((nb, HW)), "prob": g_prob.host((nb, HW)), "conf_buffer": conf}


def check(what, got, ref, dtype, cls=True, prob=True):
    assert np.array_equal(got["img_counts"], ref["img_counts"]), what + ": img_counts"
    assert np.array_equal(got["confusion"], ref["confusion"]), what + ": confusion"
    assert np.array_equal(got["img_loss"][:, 1], ref["img_loss"][:, 1]), what + ": loss counts"
    if cls:
        assert np.array_equal(got["cls"], ref["cls"]), what + ": cls"
    e_loss = float(np.max(np.abs(got["img_loss"][:, 0] - ref["img_loss"][:, 0]) / np.maximum(1.0, np.abs(ref["img_loss"][:, 0]))))
    e_prob = float(np.abs(got["prob"].astype(np.float64) - ref["prob"]).max()) if prob else 0.0
    print(f"{what}: loss-sum error {e_loss:.3e} (bound {LOSS_TOL[TDT[dtype]]:.0e}), probability error {e_prob:.3e} (gate {GATE:.2e})")
    assert e_loss <= LOSS_TOL[TDT[dtype]] and e_prob <= GATE
    return e_loss, e_prob


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"C{p[0]}_Cp{p[1]}")
def test_vector_path(pair, dtype):
    C, Cp = pair
    for i, HW in enumerate(PIXELS):
        ignore = (255, -100)[i % 2]
        x, t, ref = case(C, HW, ignore)
        check(f"C={C} Cp={Cp} {dtype} HW={HW} ignore={ignore}", run(x, t, C, Cp, dtype, ignore=ignore), ref, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("C", [19, 150])
def test_strided_path_matches_the_vector_path_bit_for_bit_in_the_integers(C, dtype):
    for HW, ignore in ((63, -100), (1000, 255)):
        x, t, ref = case(C, HW, ignore)
        a = run(x, t, C, (C + 7) // 8 * 8, dtype, "nhwc", ignore)
        b = run(x, t, C, None, dtype, "nchw", ignore)
        for k in ("img_counts", "confusion", "cls"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["img_loss"][:, 1].tobytes() == b["img_loss"][:, 1].tobytes()
        check(f"NCHW C={C} {dtype} HW={HW}", b, ref, dtype)


def test_unaligned_rows_take_the_strided_path():
    """c_stride == 1 but rows of 19 elements: not 16-byte aligned, so one thread per pixel; same results"""
    x, t, ref = case(19, 63, 255)
    check("NHWC Cp=19 fp16", run(x, t, 19, 19, "fp16"), ref, "fp16")
    check("NHWC Cp=19 fp32", run(x, t, 19, 19, "fp32"), ref, "fp32")


@pytest.mark.parametrize("C", [19, 300], ids=["lds", "global"])
def test_confusion_is_added_to(C):
    x, t, ref = case(C, 257, 255)
    pre = (np.arange((C + 1) * C, dtype=np.int64).reshape(C + 1, C) % 7 + 1) * ((1 << 33) + 12345)
    assert pre.min() > 1 << 33
    conf = Guarded((C + 1) * C, torch.int64, name="confusion")
    conf.t.copy_(torch.from_numpy(pre.reshape(-1)))
    a = run(x, t, C, (C + 7) // 8 * 8, "fp16", conf=conf)
    assert np.array_equal(a["confusion"], pre + ref["confusion"])
    b = run(x, t, C, (C + 7) // 8 * 8, "fp16", conf=conf)
    assert np.array_equal(b["confusion"], pre + 2 * ref["confusion"])
    assert np.array_equal(b["img_counts"], ref["img_counts"])                   # overwritten, not accumulated
    print(f"C={C}: confusion = pre-load + 2 x batch, exactly (bound 0)")


def test_cls_and_prob_are_optional_and_independent():
    x, t, ref = case(150, 257, 255)
    full = run(x, t, 150, 160, "fp16")
    check("both", full, ref, "fp16")
    for want_cls, want_prob in ((False, False), (True, False), (False, True)):
        got = run(x, t, 150, 160, "fp16", want_cls=want_cls, want_prob=want_prob)
        assert (got["cls"] == -777).all() if not want_cls else np.array_equal(got["cls"], full["cls"])
        assert (got["prob"] == -777.0).all() if not want_prob else got["prob"].tobytes() == full["prob"].tobytes()
        for k in ("img_counts", "confusion", "img_loss"):
            assert got[k].tobytes() == full[k].tobytes(), (k, want_cls, want_prob)
    print("cls / prob null in every combination: sentinel untouched, the other outputs byte-identical (bound 0)")


@pytest.mark.parametrize("C,Cp,layout", [(150, 160, "nhwc"), (300, 304, "nhwc"), (19, None, "nchw")])
def test_two_launches_are_byte_identical(C, Cp, layout):
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((B, 1000, C)) * 2).astype(np.float16).astype(np.float64)      # off the 1/8 grid: the loss sums round
    t = rng.integers(0, C, (B, 1000)).astype(np.int64)
    a, b = run(x, t, C, Cp, "fp16", layout), run(x, t, C, Cp, "fp16", layout)
    for k in ("img_counts", "confusion", "img_loss", "cls", "prob"):
        assert a[k].tobytes() == b[k].tobytes(), k
    check(f"C={C} {layout} random logits", a, R.sem_eval(x, t, C, 255), "fp16")


def test_cross_checks_against_the_three_sweeps_it_replaces():
    """mu_mean_iou, mu_argmax_prob and maskunet_amd.cross_entropy, unchanged, on one NHWC fp16 output-like tensor at C = 150"""
    import maskunet_amd
    from maskunet_amd import _lib
    C, Cp, H, W = 150, 160, 24, 20
    HW, M = H * W, B * H * W
    rng = np.random.default_rng(42)
    x = (rng.standard_normal((B, HW, C)) * 2).astype(np.float16).astype(np.float64)
    t = rng.integers(0, C, (B, HW)).astype(np.int64)
    t[rng.random((B, HW)) < 0.1] = 255                                         # only labels all three sweeps read alike
    got = run(x, t, C, Cp, "fp16")
    data = np.zeros((M, Cp))
    data[:, :C] = x.reshape(M, C)
    g_x, g_t = Guarded(M * Cp, torch.float16, data, "logits"), Guarded(M, torch.int64, t, "labels")
    g_counts, g_out = Guarded(3 * C, torch.int32, name="counts"), Guarded(1, torch.float32, name="miou")
    call("mu_mean_iou", g_x, g_t, M, C, M, 0, 1, Cp, 1e-6, g_counts, g_out, _lib.MU_F16)
    assert np.array_equal(got["img_counts"].sum(axis=0), g_counts.host((3, C)))
    g_cls = Guarded(M, torch.int32, name="cls")
    call("mu_argmax_prob", g_x, M, C, M, 0, 1, Cp, 2.0, g_cls, None, _lib.MU_F16)
    assert np.array_equal(got["cls"].reshape(-1), g_cls.host())
    nchw = torch.from_numpy(x.reshape(B, H, W, C).transpose(0, 3, 1, 2).copy()).to("cuda", torch.float16)
    ce = float(maskunet_amd.cross_entropy(nchw, torch.from_numpy(t.reshape(B, H, W)).cuda(), ignore_index=255).item())
    mine = got["img_loss"][:, 0].sum() / got["img_loss"][:, 1].sum()
    err = abs(mine - ce) / max(1.0, abs(ce))
    print(f"counts == mu_mean_iou, cls == mu_argmax_prob (bound 0); loss {mine:.6f} vs cross_entropy {ce:.6f}: {err:.3e} "
          f"(bound {LOSS_TOL[torch.float16]:.0e})")
    assert err <= LOSS_TOL[torch.float16]


@pytest.mark.parametrize("route", ["module_output", "plain_nchw"])
def test_semantic_metrics_over_three_updates(route):
    from maskunet_amd import SemanticMetrics, ops
    from maskunet_amd.losses import _nhwc_source
    z = np.load(os.path.join(GOLDEN, "semeval", "semeval_updates_19.npz"))
    y, t, C = z["y"], z["t"].astype(np.int64), int(z["num_classes"])
    N, _, H, W = y.shape
    assert (N, C, H, W) == (6, 19, 24, 20) and z["splits"].tolist() == [1, 2, 3]
    ref = R.sem_eval(y.astype(np.float64).transpose(0, 2, 3, 1).reshape(N, H * W, C), t.reshape(N, -1), C, 255)
    acc = SemanticMetrics(C, ignore_index=255)
    edges = np.cumsum([0] + z["splits"].tolist())
    for a, b in zip(edges[:-1], edges[1:]):
        labels = torch.from_numpy(t[a:b]).cuda()
        if route == "module_output":                                            # what a module returns: NCHW carrying its NHWC source
            nhwc = torch.full((b - a, H, W, 32), 100.0, dtype=torch.float16, device="cuda")
            nhwc[..., :C] = torch.from_numpy(y[a:b].transpose(0, 2, 3, 1).copy()).cuda()
            out = ops.to_nchw(nhwc, C)
            assert _nhwc_source(out) is not None
        else:
            out = torch.from_numpy(y[a:b].copy()).cuda()
            assert _nhwc_source(out) is None
        batch = acc.update(out, labels)
        assert batch.classes is None and batch.prob is None and batch.confusion is acc.confusion
    got = acc.compute()
    counts = [ref["img_counts"][a:b] for a, b in zip(edges[:-1], edges[1:])]
    losses = [ref["img_loss"][a:b] for a, b in zip(edges[:-1], edges[1:])]
    dev_losses = [ls.cpu().numpy() for _, ls in acc._seen]
    e_loss = max(float(np.max(np.abs(d[:, 0] - r[:, 0]) / np.maximum(1.0, np.abs(r[:, 0])))) for d, r in zip(dev_losses, losses))
    assert all(np.array_equal(d[:, 1], r[:, 1]) for d, r in zip(dev_losses, losses))
    # every entry against the restatement: integers exactly, floats to 1e-12.  The one input of the restatement that is not an integer,
    # the per-image loss sums, is the device's here (held to LOSS_TOL against ce_rows above and below): 1e-12 then tests the host
    # arithmetic, which is what compute() adds.
    want = R.metrics(ref["confusion"], counts, dev_losses)
    worst = 0.0
    assert set(got) == set(want)
    for k, r in want.items():
        if k == "reference":
            worst = max([worst] + [abs(got[k][n] - r[n]) for n in r])
        elif np.asarray(r).dtype.kind in "ib":
            assert np.array_equal(got[k], r) and np.asarray(got[k]).dtype == np.asarray(r).dtype, k
        else:
            worst = max(worst, float(np.max(np.abs(np.asarray(got[k]) - np.asarray(r)))))
    pure = R.metrics(ref["confusion"], counts, losses)["reference"]["loss"]
    e_ref_loss = abs(got["reference"]["loss"] - pure) / max(1.0, abs(pure))
    e_img = abs(got["reference"]["image_miou"] - float(z["image_miou"]))
    e_batch = abs(got["reference"]["batch_miou"] - float(z["batch_miou"].mean()))
    print(f"{route}: compute() vs restatement {worst:.3e} (bound 1e-12); loss sums {e_loss:.3e}, mean loss {e_ref_loss:.3e} "
          f"(bound {LOSS_TOL[torch.float16]:.0e}); image_miou {e_img:.3e}, batch_miou {e_batch:.3e} vs the reference's (bound 1e-6)")
    assert worst <= 1e-12 and e_loss <= LOSS_TOL[torch.float16] and e_ref_loss <= LOSS_TOL[torch.float16]
    assert e_img <= 1e-6 and e_batch <= 1e-6
    acc.reset()
    with pytest.raises(RuntimeError, match="before any update"):
        acc.compute()


def test_padded_nhwc_input_with_num_classes():
    from maskunet_amd import semantic_eval
    x, t, ref = case(19, 1000, 255)
    H, W = 40, 25
    nhwc = torch.full((B, H, W, 32), 100.0, dtype=torch.float16, device="cuda")
    nhwc[..., :19] = torch.from_numpy(np.array(x.reshape(B, H, W, 19))).cuda()
    batch = semantic_eval(nhwc, torch.from_numpy(np.array(t.reshape(B, H, W))).cuda(), num_classes=19, ignore_index=255, classes=True)
    got = {"img_counts": batch.img_counts.cpu().numpy(), "img_loss": batch.img_loss.cpu().numpy(), "confusion": batch.confusion.cpu().numpy(),
           "cls": batch.classes.cpu().numpy().reshape(B, -1), "prob": batch.prob.cpu().numpy().reshape(B, -1)}
    check("semantic_eval on [B,H,W,32] with num_classes=19", got, ref, "fp16")


def test_batch_instances_equal_predict_instances():
    """validation and instance evaluation share one sweep: the Instances from its class map and probability are predict_instances'"""
    import maskunet_amd
    from maskunet_amd import ops
    C, H, W = 19, 32, 32
    g = torch.Generator().manual_seed(7)
    nhwc = torch.zeros((2, H, W, 32), dtype=torch.float16)
    nhwc[..., :C] = (torch.randn((2, H, W, C), generator=g) * 2).half()
    out = ops.to_nchw(nhwc.cuda(), C)
    labels = torch.randint(0, C, (2, H, W), generator=g).cuda()
    want = maskunet_amd.predict_instances(out, max_instances=1024)
    batch = maskunet_amd.semantic_eval(out, labels, classes=True)
    got = batch.instances(max_instances=1024)
    assert int(want.count.min()) > 10 and int(want.count.max()) <= 1024
    for f in ("classes", "ids", "table", "count", "order"):
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    e_prob = float((got.prob.double() - want.prob.double()).abs().max())
    e_score = float((got.scores.double() - want.scores.double()).abs().max())
    print(f"ids, table, count, order identical (bound 0); probability difference {e_prob:.3e}, score difference {e_score:.3e} (gate {GATE:.2e})")
    assert e_prob <= GATE and e_score <= GATE
    with pytest.raises(RuntimeError, match="classes=True"):
        maskunet_amd.semantic_eval(out, labels).instances()
