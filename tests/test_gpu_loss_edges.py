"""maskunet_amd/csrc/loss.hip against tests/_loss_reference.py (float64) on every dispatch branch, loop tail and grid limit: the two
cross-entropy pairs, mean IoU, the multi-tensor AdamW and the instance triplet loss.  The kernels are reached through the package's
functions; per-row lse, the pixel count and the IoU counts are not visible there and are read through the C entry points with the
argument lists maskunet_amd/losses.py uses.  Every comparison is against the float64 reference computed from the inputs as rounded to
the dtype under test.  Every test prints its worst error next to its bound (pytest -s / -rP)."""
import numpy as np
import pytest
import torch

from tests import _loss_reference as R
from tests._device_buffers import Guarded

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
LOSS_TOL = {F32: 1e-5, F16: 2e-3}          # |loss - ref| <= tol * max(1, |ref|)             (tests/test_gpu_next.py)
GRAD_TOL = {F32: 5e-5, F16: 2e-3}          # |grad * count / grad_scale - ref|, a quantity of magnitude <= 1
LSE_TOL = 1e-5                             # |lse - ref| <= tol * max(1, |ref|): lse is fp32 arithmetic on exact inputs in both dtypes
GRAD_SCALE = {F32: 3.0, F16: 768.0}        # the backward's own factor; 768 keeps fp16 gradients of 70000-row means above the subnormals


def _note(what, err, bound):
    print(f"loss-edges {what}: worst {err:.3e} bound {bound:.3e}")


def _worst(err, bound):
    """largest err / bound (nan if any entry is nan), and the error / bound at that place"""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    ratio = err / bound
    if np.isnan(ratio).any():
        return float("nan"), float("nan"), float("nan")
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), float(err.flat[i]), float(bound.flat[i])


def _check(what, err, bound):
    ratio, e, b = _worst(err, bound)
    _note(what, e, b)
    assert ratio <= 1.0, (what, e, b)


# ================================================================================================
# NHWC cross-entropy: mu_ce_fwd / mu_ce_bwd
# ================================================================================================
CE_PAIRS = {F32: [(5, 8), (64, 64), (65, 72), (128, 128), (129, 136), (150, 160), (192, 192), (193, 200), (300, 304)],
            F16: [(5, 8), (128, 128), (129, 136), (256, 256), (257, 264), (384, 384), (385, 392), (520, 520)]}


def _ce_param(dt, C, Cp):
    return pytest.param(dt, C, Cp, id=f"{'fp32' if dt == F32 else 'fp16'}-{C}-{Cp}")


CE_CASES = [_ce_param(dt, C, Cp) for dt in (F32, F16) for C, Cp in CE_PAIRS[dt]]


def _ignore_for(C):
    return 255 if C <= 255 else -100       # both values the reference scripts use; 255 is a class of the wide cases


def _ce_inputs(seed, M, C, Cp, dtype, ignore, first_label=0, scale=3.0, offset=None, ignore_frac=0.2):
    """logits [M, Cp] (padding 0) rounded to dtype on the host, labels with 0 and C - 1 present and ~20 % ignored rows for M > 1"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((M, Cp), dtype=np.float32) * np.float32(scale)
    if offset is not None:
        x += offset.astype(np.float32)[:, None]
    x[:, C:] = 0.0
    lab = g.integers(0, C, M)
    lab[0] = first_label
    if M > 1:
        lab[1] = C - 1
        drop = g.random(M) < ignore_frac
        drop[:2] = False
        lab[drop] = ignore
    return torch.from_numpy(x).to(dtype), torch.from_numpy(lab)


def _ce_nhwc_device(x, lab, C, ignore, grad_scale):
    """x [M, Cp] on the device.  (lse [M], count, loss, grad [M, Cp]) from the package function and, for lse / count, from mu_ce_fwd."""
    import maskunet_amd
    from maskunet_amd import _lib
    from maskunet_amd._lib import call, dt, ptr, stream, workspace
    M, Cp = x.shape
    xg = x.clone().requires_grad_(True)
    loss = maskunet_amd.pixel_cross_entropy_nhwc(xg, lab, C, ignore, grad_scale=grad_scale)
    loss.backward()
    lse = torch.full((M,), float("nan"), dtype=torch.float32, device=x.device)
    l2 = torch.empty(1, dtype=torch.float32, device=x.device)
    count = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = workspace(_lib.load().mu_ce_workspace_bytes(), x.device)
    call("mu_ce_fwd", ptr(x), ptr(lab), M, Cp, C, ignore, ptr(lse), ptr(l2), ptr(count), ptr(ws), ws.numel(), dt(x), stream())
    assert torch.equal(l2.view(()), loss.detach()) or (torch.isnan(l2).all() and torch.isnan(loss))
    return lse, count, loss.detach(), xg.grad


def _ce_compare(what, dtype, dev, ref, C, grad_scale, lse_extra=0.0, grad_extra=0.0):
    lse, count, loss, grad = dev
    n = float(count.item())
    assert n == ref["count"] and n == int(n), (n, ref["count"])                      # exact
    lse_ref = ref["lse"]
    _check(what + " lse", np.abs(lse.double().cpu().numpy() - lse_ref), LSE_TOL * np.maximum(1.0, np.abs(lse_ref)) + lse_extra)
    _check(what + " loss", abs(float(loss.item()) - ref["loss"]), LOSS_TOL[dtype] * max(1.0, abs(ref["loss"])))
    gn = grad[:, :C].double().cpu().numpy() * (n / grad_scale)
    _check(what + " grad", np.abs(gn - ref["g"]), GRAD_TOL[dtype] + grad_extra)
    assert not grad[:, C:].any()                                                      # padded gradients: exactly 0


def _ce_padding_variants(what, x, lab, C, ignore, grad_scale, base):
    """+1e4 and NaN in the padding channels: everything equals the zero-padding run bit for bit, padded gradients are exactly 0"""
    if x.shape[1] == C:
        return
    for fill in (1e4, float("nan")):
        xv = x.clone()
        xv[:, C:] = fill
        lse, count, loss, grad = _ce_nhwc_device(xv, lab, C, ignore, grad_scale)
        assert torch.equal(lse, base[0]), (what, fill)
        assert torch.equal(count, base[1]) and torch.equal(loss, base[2]), (what, fill)
        assert torch.equal(grad[:, :C], base[3][:, :C]), (what, fill)
        assert not grad[:, C:].any(), (what, fill)


@pytest.mark.parametrize("M", [1, 17, 65, 129])
@pytest.mark.parametrize("dtype,C,Cp", CE_CASES)
def test_ce_nhwc_branch_edges(dtype, C, Cp, M):
    """one (C, Cp) per edge of the forward's dispatch (nv = 1, 2, 3 in registers, the general loop), rows that are no multiple of 16"""
    ignore, gs = _ignore_for(C), GRAD_SCALE[dtype]
    for first in ((0, C - 1) if M == 1 else (0,)):                  # M = 1 holds one label: both ends in turn
        x, lab = _ce_inputs(1000 * M + C, M, C, Cp, dtype, ignore, first_label=first)
        ref = R.ce_rows(x, lab, C, ignore)
        if M > 1:
            assert {0, C - 1} <= set(lab.tolist()) and (M < 17 or (lab == ignore).any())
        xd, ld = x.cuda(), lab.cuda()
        dev = _ce_nhwc_device(xd, ld, C, ignore, gs)
        _ce_compare(f"ce_nhwc {dtype} C={C} Cp={Cp} M={M}", dtype, dev, ref, C, gs)
        _ce_padding_variants(f"ce_nhwc C={C} Cp={Cp} M={M}", xd, ld, C, ignore, gs, dev)


@pytest.mark.parametrize("C,Cp", [(5, 8), (129, 136), (385, 392)])
def test_ce_nhwc_fp16_gradient_without_a_scale(C, Cp):
    """the fp16 backward at grad_scale = 1.  17 rows: gradients of at most 1 / count stay normal fp16 numbers (2^-11 relative, a
    quarter of the bound), and a subnormal quantum of 2^-25 times count <= 17 is 5e-7 of the normalised quantity"""
    ignore = _ignore_for(C)
    x, lab = _ce_inputs(17 + C, 17, C, Cp, F16, ignore)
    ref = R.ce_rows(x, lab, C, ignore)
    dev = _ce_nhwc_device(x.cuda(), lab.cuda(), C, ignore, 1.0)
    _ce_compare(f"ce_nhwc fp16 unscaled C={C} Cp={Cp}", F16, dev, ref, C, 1.0)


@pytest.mark.parametrize("dtype,C,Cp,M", [
    pytest.param(F32, 5, 8, 65536 + 17, id="fp32-5-8-regs4-second-pass"),
    pytest.param(F32, 150, 160, 32768 + 17, id="fp32-150-160-regs2-second-pass"),
    pytest.param(F32, 150, 160, 66000, id="fp32-150-160-backward-cap"),
    pytest.param(F16, 256, 256, 70000, id="fp16-256-256-second-pass")])
def test_ce_nhwc_grid_limits(dtype, C, Cp, M):
    """more rows than one pass of the capped grids covers (forward: 1024 blocks of 64 / 32 rows; backward: 8192 x 256 vectors);
    every row is compared"""
    ignore, gs = _ignore_for(C), GRAD_SCALE[dtype]
    x, lab = _ce_inputs(M + C, M, C, Cp, dtype, ignore)
    ref = R.ce_rows(x, lab, C, ignore)
    xd, ld = x.cuda(), lab.cuda()
    dev = _ce_nhwc_device(xd, ld, C, ignore, gs)
    _ce_compare(f"ce_nhwc grid {dtype} C={C} Cp={Cp} M={M}", dtype, dev, ref, C, gs)
    _ce_padding_variants(f"ce_nhwc grid C={C} Cp={Cp} M={M}", xd, ld, C, ignore, gs, dev)


@pytest.mark.parametrize("dtype,C,Cp", [_ce_param(F32, 150, 160), _ce_param(F32, 300, 304), _ce_param(F16, 257, 264), _ce_param(F16, 520, 520)])
def test_ce_nhwc_every_label_ignored(dtype, C, Cp):
    M, ignore = 65, _ignore_for(C)
    x, _ = _ce_inputs(7, M, C, Cp, dtype, ignore)
    lab = torch.full((M,), ignore, dtype=torch.int64)
    ref = R.ce_rows(x, lab, C, ignore)
    lse, count, loss, grad = _ce_nhwc_device(x.cuda(), lab.cuda(), C, ignore, GRAD_SCALE[dtype])
    assert count.item() == 0.0 and torch.isnan(loss)
    assert not grad.any() and not torch.isnan(grad).any()                            # exactly 0, every element
    _check(f"ce_nhwc all-ignored {dtype} C={C} lse", np.abs(lse.double().cpu().numpy() - ref["lse"]),
           LSE_TOL * np.maximum(1.0, np.abs(ref["lse"])))


@pytest.mark.parametrize("dtype,C,Cp", [_ce_param(F32, 64, 64), _ce_param(F32, 150, 160), _ce_param(F32, 300, 304), _ce_param(F16, 129, 136),
                                      _ce_param(F16, 520, 520)])
def test_ce_nhwc_minus_inf_logit(dtype, C, Cp):
    """a -inf logit in a channel of every row that is not its target: exp -> 0, no NaN anywhere"""
    M, ignore, gs = 65, _ignore_for(C), GRAD_SCALE[dtype]
    x, lab = _ce_inputs(11, M, C, Cp, dtype, ignore)
    ch = (torch.where(lab == ignore, torch.zeros_like(lab), lab) + 1 + torch.arange(M) % (C - 1)) % C
    assert not (ch == lab).any()
    x[torch.arange(M), ch] = float("-inf")
    ref = R.ce_rows(x, lab, C, ignore)
    xd, ld = x.cuda(), lab.cuda()
    dev = _ce_nhwc_device(xd, ld, C, ignore, gs)
    _ce_compare(f"ce_nhwc -inf {dtype} C={C} Cp={Cp}", dtype, dev, ref, C, gs)
    _ce_padding_variants(f"ce_nhwc -inf C={C} Cp={Cp}", xd, ld, C, ignore, gs, dev)


@pytest.mark.parametrize("C,Cp", [(64, 64), (150, 160), (300, 304)])
def test_ce_nhwc_offset_logits(C, Cp):
    """fp32 rows shifted by their own constant in +-300.  The in-register branches compute exp2(fma(x, log2e, -mx * log2e)): rounding
    mx * log2e once puts up to |mx| * 2^-24 into lse, and lse itself (about mx) is stored with up to |lse| * 2^-24 more.  The bound
    adds |mx| * 2^-23 per row to lse and the same amount relative to the softmax p to the gradient (d p = p * d lse); the loss keeps
    its own bound."""
    M, ignore, gs = 129, 255 if C <= 255 else -100, GRAD_SCALE[F32]
    off = np.random.default_rng(C).uniform(-300.0, 300.0, M)
    off[:4] = (300.0, -300.0, 299.5, -299.5)
    x, lab = _ce_inputs(13 + C, M, C, Cp, F32, ignore, offset=off)
    ref = R.ce_rows(x, lab, C, ignore)
    extra = np.abs(ref["mx"]) * 2.0 ** -23
    dev = _ce_nhwc_device(x.cuda(), lab.cuda(), C, ignore, gs)
    _ce_compare(f"ce_nhwc offset C={C} Cp={Cp}", F32, dev, ref, C, gs, lse_extra=extra, grad_extra=extra[:, None] * ref["p"])


# ================================================================================================
# NCHW cross-entropy: mu_ce_nchw_fwd / mu_ce_nchw_bwd
# ================================================================================================
def _ce_nchw_device(x, lab, ignore, grad_scale):
    """x [B, C, HW], lab [B, HW] on the device"""
    import maskunet_amd
    from maskunet_amd import _lib
    from maskunet_amd._lib import call, dt, ptr, stream, workspace
    B, C, HW = x.shape
    xg = x.clone().requires_grad_(True)
    loss = maskunet_amd.cross_entropy(xg, lab, ignore, grad_scale=grad_scale)
    loss.backward()
    lse = torch.full((B * HW,), float("nan"), dtype=torch.float32, device=x.device)
    l2 = torch.empty(1, dtype=torch.float32, device=x.device)
    count = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = workspace(_lib.load().mu_ce_workspace_bytes(), x.device)
    call("mu_ce_nchw_fwd", ptr(x), ptr(lab), B, C, HW, ignore, ptr(lse), ptr(l2), ptr(count), ptr(ws), ws.numel(), dt(x), stream())
    assert torch.equal(l2.view(()), loss.detach()) or (torch.isnan(l2).all() and torch.isnan(loss))
    return lse, count, loss.detach(), xg.grad


def _ce_nchw_case(what, dtype, B, C, HW, seed, variant="plain"):
    ignore, gs = 255, GRAD_SCALE[dtype]
    rows, lab = _ce_inputs(seed, B * HW, C, C, dtype, ignore, ignore_frac=0.2 if B * HW > 4 else 0.0)
    if variant == "minus_inf":                                      # the whole first chunk of 8 channels, the target elsewhere
        rows[:, :8] = float("-inf")
        lab[lab < 8] = 8 + lab[lab < 8] % (C - 8)
    if variant == "all_ignored":
        lab[:] = ignore
    ref = R.ce_rows(rows, lab, C, ignore)
    x = rows.reshape(B, HW, C).permute(0, 2, 1).contiguous()
    lse, count, loss, grad = _ce_nchw_device(x.cuda(), lab.reshape(B, HW).cuda(), ignore, gs)
    grad_rows = grad.permute(0, 2, 1).reshape(B * HW, C)
    if variant == "all_ignored":
        assert count.item() == 0.0 and torch.isnan(loss)
        assert not grad.any() and not torch.isnan(grad).any()
        _check(what + " lse", np.abs(lse.double().cpu().numpy() - ref["lse"]), LSE_TOL * np.maximum(1.0, np.abs(ref["lse"])))
    else:
        _ce_compare(what, dtype, (lse, count, loss, grad_rows), ref, C, gs)


NCHW_SHAPES = [(1, 16), (7, 63), (8, 64), (9, 20), (16, 5), (150, 36)]      # 4 pixels per lane and 1; C below, at and above a chunk of 8


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,HW", NCHW_SHAPES)
def test_ce_nchw_shapes(dtype, C, HW):
    _ce_nchw_case(f"ce_nchw {dtype} C={C} HW={HW}", dtype, 2, C, HW, 100 * C + HW)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,HW", [s for s in NCHW_SHAPES if s[0] > 8])
def test_ce_nchw_first_chunk_minus_inf(dtype, C, HW):
    _ce_nchw_case(f"ce_nchw -inf {dtype} C={C} HW={HW}", dtype, 2, C, HW, 200 * C + HW, variant="minus_inf")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("C,HW", [(7, 63), (150, 36)])
def test_ce_nchw_every_label_ignored(dtype, C, HW):
    _ce_nchw_case(f"ce_nchw all-ignored {dtype} C={C} HW={HW}", dtype, 2, C, HW, 300 * C + HW, variant="all_ignored")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("B,HW", [(1, 1050001), (2, 2100000)], ids=["1px-per-lane", "4px-per-lane"])
def test_ce_nchw_grid_limits(dtype, B, HW):
    """C = 2 and more lane groups than the capped grids hold at once (forward 1024 x 256, backward 4096 x 256)"""
    _ce_nchw_case(f"ce_nchw grid {dtype} B={B} HW={HW}", dtype, B, 2, HW, HW)


# ================================================================================================
# mean IoU: mu_mean_iou
# ================================================================================================
def _iou_device(pred, lab, C, layout):
    """counts [3, C] from mu_mean_iou with the strides losses.mean_iou passes, and the value from losses.mean_iou itself"""
    import maskunet_amd
    from maskunet_amd._lib import call, dt, ptr, stream
    M = lab.numel()
    if layout == "nchw":
        hw = pred.shape[2] * pred.shape[3]
        inner, outer, cs, ps = hw, C * hw, hw, 1
    else:
        inner, outer, cs, ps = M, 0, 1, pred.shape[-1]
    counts = torch.empty(3 * C, dtype=torch.int32, device=pred.device)
    out = torch.empty(1, dtype=torch.float32, device=pred.device)
    call("mu_mean_iou", ptr(pred), ptr(lab), M, C, inner, outer, cs, ps, 1e-6, ptr(counts), ptr(out), dt(pred), stream())
    value = maskunet_amd.mean_iou(pred, lab, C, layout=layout)
    assert torch.equal(value, out.view(()))
    return counts.view(3, C).cpu().numpy().astype(np.int64), float(value.item())


def _iou_layouts(rows, B, H, W, C, dtype):
    """[M, C] rows as the NCHW tensor and as the NHWC tensor padded to a multiple of 8 channels (+1e4 in the padding: never read)"""
    x = rows.reshape(B, H, W, C)
    Cp = (C + 7) // 8 * 8
    nhwc = torch.full((B, H, W, Cp), 1e4, dtype=dtype)
    nhwc[..., :C] = x
    return {"nchw": x.permute(0, 3, 1, 2).contiguous(), "nhwc": nhwc}


IOU_CASES = {                      # C, (B, H, W), logits, labels
    "one-class": (1, (1, 8, 8), "normal", "in-range"),
    "ties": (21, (3, 10, 10), "eight-values", "in-range"),
    "labels-255-and-minus-1": (21, (3, 10, 10), "normal", "outside"),
    "4096-classes": (4096, (3, 10, 10), "normal", "in-range"),
    "second-pass": (2, (2, 2, 131147), "normal", "in-range"),        # 524288 + 300 pixels: past one pass of 2048 x 256 threads
}


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", list(IOU_CASES))
def test_mean_iou_counts(case, dtype, layout):
    C, (B, H, W), kind, labels = IOU_CASES[case]
    M = B * H * W
    g = np.random.default_rng(len(case) + C)
    if kind == "eight-values":
        rows = torch.from_numpy(g.integers(0, 8, (M, C)).astype(np.float32) * 0.25 - 1.0).to(dtype)      # ties everywhere
    else:
        rows = torch.from_numpy(g.standard_normal((M, C), dtype=np.float32)).to(dtype)
    lab = torch.from_numpy(g.integers(0, C, M))
    if labels == "outside":
        lab[::9] = 255
        lab[4::11] = -1
    ref_counts, ref = R.iou_counts(rows, lab, C)
    pred = _iou_layouts(rows, B, H, W, C, dtype)[layout].cuda()
    counts, value = _iou_device(pred, lab.cuda(), C, layout)
    assert np.array_equal(counts, ref_counts)
    _check(f"mean_iou {case} {dtype} {layout}", abs(value - ref), 1e-6)


def test_mean_iou_layout_keyword_on_the_ambiguous_shape():
    """32 classes at 32 x 32: the padded NHWC tensor [2,32,32,32] also has the shape of an NCHW one.  The keyword decides; None keeps
    the guess (NCHW first)."""
    import maskunet_amd
    g = np.random.default_rng(32)
    C, B, H, W = 32, 2, 32, 32
    x = torch.from_numpy(g.standard_normal((B, H, W, C), dtype=np.float32) + np.linspace(0.0, 1.5, C, dtype=np.float32))
    lab = torch.from_numpy(g.integers(0, C, B * H * W))
    as_nhwc = R.iou_counts(x.reshape(-1, C), lab, C)
    as_nchw = R.iou_counts(x.permute(0, 2, 3, 1).reshape(-1, C), lab, C)
    assert not np.array_equal(as_nhwc[0], as_nchw[0]) and abs(as_nhwc[1] - as_nchw[1]) > 1e-4        # the two readings differ
    xd, ld = x.cuda(), lab.cuda().view(B, H, W)
    for layout, (ref_counts, ref) in (("nhwc", as_nhwc), ("nchw", as_nchw)):
        counts, value = _iou_device(xd, ld, C, layout)
        assert np.array_equal(counts, ref_counts), layout
        _check(f"mean_iou ambiguous {layout}", abs(value - ref), 1e-6)
    assert maskunet_amd.mean_iou(xd, ld, C).item() == maskunet_amd.mean_iou(xd, ld, C, layout="nchw").item()
    with pytest.raises(ValueError):
        maskunet_amd.mean_iou(xd, ld, C, layout="hwcn")
    with pytest.raises(RuntimeError):
        maskunet_amd.mean_iou(xd[..., :24].contiguous(), ld, C, layout="nhwc")        # fewer channels than classes


# ================================================================================================
# the dtype gate of the cross-entropy and IoU entry points: MU_F32X and an unknown dtype are MU_ERR_ARG before anything is launched --
# lse, loss, count and the gradient still hold the sentinel; a short workspace is named first (MU_ERR_WORKSPACE)
# ================================================================================================
BAD_DTYPES = [pytest.param(2, id="MU_F32X"), pytest.param(99, id="99")]


def _refused(code, name, *args, outs):
    from maskunet_amd import _lib
    with pytest.raises(RuntimeError, match=code):
        _lib.call(name, *[a.p if isinstance(a, Guarded) else a for a in args], _lib.stream())
    torch.cuda.synchronize()
    for a in list(args) + list(outs):
        if isinstance(a, Guarded):
            a.check()
    for o in outs:
        assert bool((o.t == o.sent).all()), (name, code, o.name)


def _ce_operands(n_logits, n_pix):
    """fp32-sized buffers (an fp16 reading of them is shorter): logits, labels, lse, loss, count, grad_out, dlogits, workspace"""
    from maskunet_amd import _lib
    g = {"logits": Guarded(n_logits, F32, np.zeros(n_logits, np.float32), "logits"),
         "labels": Guarded(n_pix, torch.int64, np.zeros(n_pix, np.int64), "labels"),
         "gout": Guarded(1, F32, np.ones(1, np.float32), "grad_out")}
    for name, n in (("lse", n_pix), ("loss", 1), ("count", 1), ("dlogits", n_logits)):
        g[name] = Guarded(n, F32, name=name)
    nws = _lib.load().mu_ce_workspace_bytes()
    g["ws"] = Guarded(nws, torch.uint8, name="workspace")
    return g, nws


@pytest.mark.parametrize("bad", BAD_DTYPES)
def test_ce_nhwc_dtype_gate(bad):
    M, C, Cp = 1, 2, 8
    g, nws = _ce_operands(M * Cp, M)
    fwd_outs = [g["lse"], g["loss"], g["count"], g["ws"]]
    _refused("MU_ERR_ARG", "mu_ce_fwd", g["logits"], g["labels"], M, Cp, C, -100, g["lse"], g["loss"], g["count"], g["ws"], nws, bad, outs=fwd_outs)
    _refused("MU_ERR_WORKSPACE", "mu_ce_fwd", g["logits"], g["labels"], M, Cp, C, -100, g["lse"], g["loss"], g["count"], g["ws"], nws - 1, bad,
             outs=fwd_outs)
    g["lse"].t.zero_()                                         # the backward's inputs
    g["count"].t.fill_(1.0)
    _refused("MU_ERR_ARG", "mu_ce_bwd", g["logits"], g["labels"], g["lse"], g["count"], g["gout"], 1.0, M, Cp, C, -100, g["dlogits"], bad,
             outs=[g["dlogits"]])


@pytest.mark.parametrize("HW", [3, 4], ids=["1px-per-lane", "4px-per-lane"])
@pytest.mark.parametrize("bad", BAD_DTYPES)
def test_ce_nchw_dtype_gate(bad, HW):
    B, C = 1, 2
    g, nws = _ce_operands(B * C * HW, B * HW)
    fwd_outs = [g["lse"], g["loss"], g["count"], g["ws"]]
    _refused("MU_ERR_ARG", "mu_ce_nchw_fwd", g["logits"], g["labels"], B, C, HW, -100, g["lse"], g["loss"], g["count"], g["ws"], nws, bad,
             outs=fwd_outs)
    _refused("MU_ERR_WORKSPACE", "mu_ce_nchw_fwd", g["logits"], g["labels"], B, C, HW, -100, g["lse"], g["loss"], g["count"], g["ws"], nws - 1, bad,
             outs=fwd_outs)
    g["lse"].t.zero_()
    g["count"].t.fill_(1.0)
    _refused("MU_ERR_ARG", "mu_ce_nchw_bwd", g["logits"], g["labels"], g["lse"], g["count"], g["gout"], 1.0, B, C, HW, -100, g["dlogits"], bad,
             outs=[g["dlogits"]])


@pytest.mark.parametrize("bad", BAD_DTYPES)
def test_mean_iou_dtype_gate(bad):
    """`out` stays untouched.  (The counts are cleared before the dtype is looked at, on a refused call too: they are scratch.)"""
    M, C, Cp = 1, 2, 8
    g, _ = _ce_operands(M * Cp, M)
    counts, out = Guarded(3 * C, torch.int32, name="counts"), Guarded(1, F32, name="out")
    _refused("MU_ERR_ARG", "mu_mean_iou", g["logits"], g["labels"], M, C, M, 0, 1, Cp, 1e-6, counts, out, bad, outs=[out])


# ================================================================================================
# AdamW: mu_adamw_multi
# ================================================================================================
ADAM_SIZES = [1, 255, 257, 4095, 4096, 4097, 8192, 12289]          # either side of the 256-thread stride and of the 4096-element chunk
ADAM_WD = [0.0, 0.1, 0.0, 0.1, 0.0, 0.1, 0.0, 0.1]                 # two parameter groups
ADAM_LR, ADAM_BETAS = 5e-3, (0.9, 0.999)


def _adam_setup(seed, eps):
    import maskunet_amd
    g = np.random.default_rng(seed)
    p0 = [g.standard_normal(n, dtype=np.float32) for n in ADAM_SIZES]
    params = [torch.from_numpy(a).cuda().requires_grad_(True) for a in p0]
    groups = [{"params": [p for p, w in zip(params, ADAM_WD) if w == wd], "weight_decay": wd} for wd in (0.0, 0.1)]
    return g, p0, params, maskunet_amd.FusedAdamW(groups, lr=ADAM_LR, betas=ADAM_BETAS, eps=eps)


def _adam_grads(g, it, scale, missing=None):
    """gradients with exact zeros: every 5th element in every step (v stays 0: denom = eps), every 7th in the first step only"""
    out = []
    for i, n in enumerate(ADAM_SIZES):
        a = g.standard_normal(n, dtype=np.float32)
        a[::5] = 0.0
        if it == 0:
            a[::7] = 0.0
        out.append(None if (it, i) == missing else a * np.float32(scale))
    return out


def _adam_compare(what, opt, params, ref, steps):
    """p: rtol 2e-5 / atol 2e-6 (tests/test_gpu_next.py).  m, v: steps * 8 * 2^-24 relative to their own value -- at most 4-5 fp32
    roundings per step with a margin of 2; one fp32 denormal step more for the one-element tensor.
    exp_avg, widened (NOTES_r11.md): m = beta1 * m + (1 - beta1) * g sums terms of both signs, and where they cancel a correct fp32 m is
    further from the float64 one than any multiple of |m| (a rounding is relative to the term rounded, not to the sum).  An element
    beyond the bound above is held to steps * 4 * 2^-24 * m_abs instead, m_abs being the same recursion on |g|.  Worst case by
    derivation 3 per step: half an ulp each for g * ginv, (1 - beta1) * g, beta1 * m and the sum, every term at most m_abs, and the
    error carried over shrinks by beta1 as m_abs does."""
    rel = steps * 8 * 2.0 ** -24
    for i, (q, (p, m, v, m_abs)) in enumerate(zip(params, ref)):
        st = opt.state[q]
        floor = 2.0 ** -149 if ADAM_SIZES[i] == 1 else 0.0
        tag = f"{what} n={ADAM_SIZES[i]}"
        _check(tag + " p", np.abs(q.detach().double().cpu().numpy() - p), 2e-6 + 2e-5 * np.abs(p))
        m_err = np.abs(st["exp_avg"].double().cpu().numpy() - m)
        beyond = m_err > rel * np.abs(m) + floor
        if beyond.any():
            print(f"loss-edges {tag} exp_avg: {int(beyond.sum())} of {m.size} beyond {rel:.2e} * |m|, worst err / |m| "
                  f"{float((m_err[beyond] / np.abs(m[beyond])).max()):.2e}")
        _check(tag + " exp_avg", m_err, np.maximum(rel * np.abs(m), 0.5 * rel * m_abs) + floor + 1e-300)
        _check(tag + " exp_avg_sq", np.abs(st["exp_avg_sq"].double().cpu().numpy() - v), rel * v + floor + 1e-300)


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
@pytest.mark.parametrize("scale", [1.0, 1000.0])
def test_adamw_chunk_edges(scale, eps):
    """three steps; the 4095-element tensor has no gradient in the second one (its own step counter lags)"""
    g, p0, params, opt = _adam_setup(int(scale) + 7, eps)
    grads = [_adam_grads(g, it, scale, missing=(1, 3)) for it in range(3)]
    ref = R.adamw_steps(p0, grads, ADAM_LR, ADAM_BETAS, eps, ADAM_WD, scale)
    for it in range(3):
        for q, a in zip(params, grads[it]):
            q.grad = None if a is None else torch.from_numpy(a).cuda()
        opt.step(grad_scale=scale)
        _adam_compare(f"adamw scale={scale} eps={eps} step {it + 1}", opt, params, ref[it], it + 1)
    assert opt.state[params[3]]["step"] == 2 and opt.state[params[4]]["step"] == 3
    assert not opt.state[params[5]]["exp_avg_sq"][::5].any()       # gradient always 0 there: v is exactly 0


def test_adamw_large_step_count():
    """a resumed run: after one step the 4097-element tensor's host counter is set to 9998; the next step uses t = 9999 for it
    (bias correction 2 = 1 - 0.999^9999, within 5e-5 of 1) and t = 2 for the others"""
    g, p0, params, opt = _adam_setup(99, 1e-8)
    grads = [_adam_grads(g, it, 1.0) for it in range(2)]
    ref = R.adamw_steps(p0, grads, ADAM_LR, ADAM_BETAS, 1e-8, ADAM_WD, 1.0, set_step={(1, 5): 9998})
    for it in range(2):
        for q, a in zip(params, grads[it]):
            q.grad = torch.from_numpy(a).cuda()
        if it == 1:
            opt.state[params[5]]["step"] = 9998
        opt.step()
        _adam_compare(f"adamw resumed step {it + 1}", opt, params, ref[it], it + 1)
    assert opt.state[params[5]]["step"] == 9999


# ================================================================================================
# instance triplet loss: mu_inst_triplet_fwd / mu_inst_triplet_bwd  (fp32 features, C = 3, id_cap = 32768, B <= H <= W)
# ================================================================================================
ID_CAP = 32768


def _inst_run(what, feat, mask, u, max_inst, margin=1.0, ignore=None, min_hinge=1e-4):
    """device loss and gradient (through an upstream factor of 3) against the reference; 1e-5 as tests/test_gpu_next.py"""
    import maskunet_amd
    u = np.asarray(u, dtype=np.float32)
    u = np.concatenate([u, np.zeros(max_inst - len(u), dtype=np.float32)])
    ref_loss, ref_grad, hinge = R.instance_triplet(feat, mask, u, margin, ignore, ID_CAP, max_inst)
    assert len(hinge) == 0 or np.abs(hinge).min() > min_hinge          # no instance sits on the kink of the clamp
    fd = torch.from_numpy(feat).cuda().requires_grad_(True)
    crit = maskunet_amd.InstanceContrastiveLoss(margin=margin, ignore_index=ignore, id_cap=ID_CAP, max_instances=max_inst)
    loss = crit(fd, torch.from_numpy(mask).cuda(), torch.from_numpy(u).cuda())
    (loss * 3.0).backward()
    _check(what + " loss", abs(float(loss.item()) - ref_loss), 1e-5 * max(1.0, abs(ref_loss)))
    _check(what + " dfeat", np.abs(fd.grad.double().cpu().numpy() / 3.0 - ref_grad), 1e-5)
    return ref_loss, ref_grad, hinge


def _inst_mask(shape, ids, sizes, seed):
    """the ids scattered over random pixels, `sizes[i]` pixels each, background 0"""
    g = np.random.default_rng(seed)
    mask = np.zeros(int(np.prod(shape)), dtype=np.int64)
    where = g.permutation(mask.size)[:int(np.sum(sizes))]
    mask[where] = np.repeat(np.asarray(ids, dtype=np.int64), sizes)
    return mask.reshape(shape), g


def _inst_u(mask, g, ignore, max_inst):
    """u[k] = (j + 0.5) / n_neg with a random j: the product is half a pixel away from every integer in fp32 and in fp64"""
    return [(int(g.integers(0, nneg)) + 0.5) / nneg for _, _, nneg in R.instance_ids(mask, ignore, ID_CAP, max_inst)]


def _inst_feat(shape, g, C=3):
    return g.standard_normal((shape[0], C) + tuple(shape[1:]), dtype=np.float32)


def test_inst_200_ids_fill_the_block_table():
    """200 ids of 2-4 pixels in one block's range: the 128-slot table fills up and the rest goes through the global fallback"""
    g0 = np.random.default_rng(200)
    ids = np.sort(g0.choice(np.arange(1, ID_CAP), 200, replace=False))
    mask, g = _inst_mask((2, 16, 24), ids, 2 + np.arange(200) % 3, 201)
    feat = _inst_feat(mask.shape, g)
    assert len(R.instance_ids(mask, None, ID_CAP, 256)) == 200
    _, _, hinge = _inst_run("inst 200 ids", feat, mask, _inst_u(mask, g, None, 256), 256)
    assert (hinge > 0).sum() >= 100


def test_inst_ids_on_one_probe_chain():
    """ids 128 k, k = 1..40, all hash to slot 0: 16 fit the probe chain, 24 take the fallback, in both blocks of a 6144-pixel mask"""
    ids = 128 * np.arange(1, 41)
    mask, g = _inst_mask((2, 48, 64), ids, 3 + np.arange(40) % 4, 128)
    feat = _inst_feat(mask.shape, g)
    assert len(R.instance_ids(mask, None, ID_CAP, 64)) == 40
    _, _, hinge = _inst_run("inst one chain", feat, mask, _inst_u(mask, g, None, 64), 64)
    assert (hinge > 0).sum() >= 20


def test_inst_more_instances_than_the_cap():
    """40 instances, max_instances = 16: the 16 smallest ids, mean over 16; an ignore label among the pixels"""
    g0 = np.random.default_rng(40)
    ids = np.sort(g0.choice(np.arange(256, 3000), 40, replace=False))                 # none is the ignore label
    mask, g = _inst_mask((2, 16, 24), np.concatenate([ids, [255]]), np.concatenate([2 + np.arange(40) % 3, [30]]), 41)
    feat = _inst_feat(mask.shape, g)
    listed = R.instance_ids(mask, 255, ID_CAP, 16)
    assert [i for i, _, _ in listed] == sorted(ids.tolist())[:16]
    assert len(R.instance_ids(mask, 255, ID_CAP, 64)) == 40
    _, _, hinge = _inst_run("inst cap", feat, mask, _inst_u(mask, g, 255, 16), 16, ignore=255)
    assert len(hinge) == 16 and (hinge > 0).sum() >= 8


def test_inst_ids_out_of_range():
    """-5 and 40000 are no instances, their pixels are negatives: the first two instances draw exactly those pixels"""
    mask, g = _inst_mask((2, 16, 24), [-5, 40000, 7, 300, 32767], [6, 6, 3, 4, 2], 5)
    feat = _inst_feat(mask.shape, g)
    flat = mask.reshape(-1)
    listed = [i for i, _, _ in R.instance_ids(mask, None, ID_CAP, 16)]
    assert listed == [7, 300, 32767]
    u = [R.u_for_negative(mask, 7, int(np.flatnonzero(flat == -5)[3])), R.u_for_negative(mask, 300, int(np.flatnonzero(flat == 40000)[-1])),
         R.u_for_negative(mask, 32767, int(np.flatnonzero(flat == 0)[100]))]
    _inst_run("inst out of range", feat, mask, u, 16)


def test_inst_one_id_everywhere():
    """no pixel outside the only instance: nothing reaches the draw, loss 0 and gradient 0"""
    import maskunet_amd
    g = np.random.default_rng(3)
    feat = torch.from_numpy(_inst_feat((2, 16, 24), g)).cuda().requires_grad_(True)
    mask = torch.full((2, 16, 24), 9, dtype=torch.int64, device="cuda")
    crit = maskunet_amd.InstanceContrastiveLoss(margin=1.0, id_cap=ID_CAP, max_instances=16)
    loss = crit(feat, mask, torch.full((16,), 0.5, device="cuda"))
    loss.backward()
    assert loss.item() == 0.0 and not feat.grad.any()


@pytest.mark.parametrize("shape,own", [((2, 72, 80), (3, 4000)), ((3, 64, 64), (70, 4000))], ids=["2x72x80", "3x64x64"])
def test_inst_negative_at_the_sweep_edge(shape, own):
    """one instance in a mask of more than one 8192-pixel sweep; the negative is pixel 8191, 8192, 8193 in turn, then u = 0 (the first
    negative) and the largest u below 1 (the last).  At 2x72x80 the three pixels share an image row, hence a feature column; at
    3x64x64 pixel 8192 starts a row, so an off-by-one at the hand-over between the sweeps changes the loss."""
    MARGIN = 10.0                                                   # above every distance here: the clamp stays open
    g = np.random.default_rng(shape[1])
    mask = np.zeros(shape, dtype=np.int64)
    mask.reshape(-1)[list(own)] = 7
    feat = _inst_feat(shape, g)
    losses = {}
    for pixel in (8191, 8192, 8193):
        losses[pixel], _, hinge = _inst_run(f"inst sweep {shape} negative {pixel}", feat, mask, [R.u_for_negative(mask, 7, pixel)], 4,
                                            margin=MARGIN)
        assert hinge[0] > 0
    if shape[2] == 64:
        assert abs(losses[8191] - losses[8192]) > 1e-3
    first = _inst_run(f"inst sweep {shape} u=0", feat, mask, [0.0], 4, margin=MARGIN)[0]
    last = _inst_run(f"inst sweep {shape} u<1", feat, mask, [np.nextafter(np.float32(1.0), np.float32(0.0))], 4, margin=MARGIN)[0]
    n = mask.size                                                   # the reference itself: u = 0 is pixel 0, u < 1 the last pixel
    assert first == R.instance_triplet(feat, mask, [R.u_for_negative(mask, 7, 0)], MARGIN, None, ID_CAP, 4)[0] > 0
    assert last == R.instance_triplet(feat, mask, [R.u_for_negative(mask, 7, n - 1)], MARGIN, None, ID_CAP, 4)[0] > 0


def test_inst_negative_in_the_anchors_own_row():
    """the negative pixel lies in the anchor's (batch, row): anchor and negative are the same feature column, d(a, n) = |1e-6| and
    the two gradient contributions to that column cancel"""
    g = np.random.default_rng(17)
    shape = (2, 16, 24)
    mask = np.zeros(shape, dtype=np.int64)
    mask[1, 5, 2], mask[0, 9, 7] = 4, 4                             # anchor (0, 9), positive (1, 5)
    mask[1, 12, 3:6] = 11
    feat = _inst_feat(shape, g)
    u = [R.u_for_negative(mask, 4, (0 * 16 + 9) * 24 + 20), R.u_for_negative(mask, 11, (1 * 16 + 12) * 24 + 20)]
    _, _, hinge = _inst_run("inst own row", feat, mask, u, 4)
    assert hinge[0] > 1.0 and abs(hinge[1] - 1.0) < 1e-4           # d(a, n) ~ 0 in both; the second also has a == p
