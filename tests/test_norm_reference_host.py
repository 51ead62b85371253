"""tests/_norm_reference.py pinned against torch in float64 (CPU): nn.BatchNorm2d in train and eval mode with autograd gradients and
running statistics, bn2(bn1(x)) for the pair, F.layer_norm with a full-shape affine, F.gelu / relu backward, and the device-only
rules (M = 1, padded channels, the dx scale rule) by hand.  Also: every input recipe of tests/test_gpu_norm_edges.py meets its own
conditions, checked here where no GPU is needed."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _norm_reference as R
from tests import test_gpu_norm_edges as E

D = torch.float64
NONE, GELU, RELU = R.ACT_NONE, R.ACT_GELU, R.ACT_RELU
EPS32 = float(np.float32(1e-5))


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.all(np.abs(a - b) <= tol * (1.0 + np.abs(b))), float(np.abs(a - b).max())


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _act_torch(p, a):
    return F.gelu(p) if a == GELU else (F.relu(p) if a == RELU else p)


def _nhwc_rows(t):
    """[N, C, H, W] -> the [M, C] rows the kernels see"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).detach().numpy()


# ------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------
def test_gelu_and_relu_match_torch_forward_and_backward():
    x = torch.linspace(-8.0, 8.0, 801, dtype=D)
    x = torch.cat([x, torch.tensor([4.24, -4.24, 4.26, -4.26, 30.0, -30.0, 0.0, -0.0], dtype=D)]).requires_grad_(True)
    for a in (GELU, RELU, NONE):
        y = _act_torch(x, a)
        (g,) = torch.autograd.grad(y.sum(), x)
        _close(R.act(x.detach().numpy(), a), y.detach().numpy(), 1e-14)
        keep = x.detach().numpy() != 0.0 if a == RELU else np.ones(x.numel(), dtype=bool)          # the step at 0: the reference says 0
        _close(R.act_grad(x.detach().numpy(), a)[keep], g.numpy()[keep], 1e-14)
    assert R.act_grad(np.array([0.0, -0.0]), RELU).tolist() == [0.0, 0.0]
    # the constants the bounds lean on: |GELU'| <= 1.13, |GELU''| <= 0.8
    xs = np.linspace(-10, 10, 200001)
    assert np.abs(R.gelu_grad(xs)).max() <= 1.13 and np.abs(np.gradient(R.gelu_grad(xs), xs)).max() <= 0.8


# ------------------------------------------------------------------------------------------------
# BatchNorm2d, training and eval
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,use_res", [(NONE, False), (GELU, False), (GELU, True), (RELU, True)])
@pytest.mark.parametrize("shape", [(2, 8, 3, 5), (1, 5, 4, 4), (3, 19, 1, 2)])
def test_batchnorm_train_matches_torch(shape, a, use_res):
    torch.manual_seed(sum(shape) + a)
    N, C, Hh, W = shape
    bn = torch.nn.BatchNorm2d(C, eps=EPS32, momentum=0.125).to(D)        # values that are float32 numbers: what the ABI carries
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, dtype=D) * 0.5 + 1.0)
        bn.bias.copy_(torch.randn(C, dtype=D) * 0.5)
        bn.running_mean.copy_(torch.randn(C, dtype=D))
        bn.running_var.copy_(torch.rand(C, dtype=D) + 0.5)
    rm0, rv0 = bn.running_mean.clone().numpy(), bn.running_var.clone().numpy()
    x = (torch.randn(shape, dtype=D) * 1.5 + 0.3).requires_grad_(True)
    res = torch.randn(shape, dtype=D).requires_grad_(True) if use_res else None
    go = torch.randn(shape, dtype=D)
    y = _act_torch(bn(x) + (res if use_res else 0.0), a)
    y.backward(go)
    xr, gr = _nhwc_rows(x), _nhwc_rows(go)
    rr = _nhwc_rows(res) if use_res else None
    st = R.bn_stats(xr, 1e-5, 0.125, rm0, rv0)
    _close(st["running_mean"], bn.running_mean.numpy())
    _close(st["running_var"], bn.running_var.numpy())
    assert int(bn.num_batches_tracked) == 1                                                  # the counter the device advances by 1 per call
    gamma, beta = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    y_ref, _ = R.bn_act_fwd(xr, rr, st["mean"], st["rstd"], gamma, beta, a)
    _close(y_ref, _nhwc_rows(y))
    b = R.bn_act_bwd(xr, rr, gr, st["mean"], st["rstd"], gamma, beta, a, 1, None, "f64" if False else "f32")
    # dz is rounded to fp32 storage in the reference: agreement with the float64 autograd to that rounding
    tol = 2e-7
    _close(b["dx"], _nhwc_rows(x.grad), tol)
    _close(b["dgamma"], bn.weight.grad.numpy(), tol * 4)
    _close(b["dbeta"], bn.bias.grad.numpy(), tol * 4)
    if use_res:
        _close(b["dres"], _nhwc_rows(res.grad), tol)
    # from statistics rows: groups of rows summed, the same statistics
    M = xr.shape[0]
    k = 1 if M % 2 else 2
    grp = xr.reshape(M // k, k, C)
    part = np.stack([grp.sum(1), (grp * grp).sum(1)], -1)
    sr = R.bn_stats_from_rows(part, M, 1e-5, 0.125, rm0, rv0)
    for key in ("mean", "rstd", "running_mean", "running_var"):
        _close(sr[key], st[key], 1e-9)


@pytest.mark.parametrize("a", [NONE, GELU, RELU])
def test_batchnorm_eval_matches_torch(a):
    torch.manual_seed(3 + a)
    shape, C = (2, 8, 3, 3), 8
    bn = torch.nn.BatchNorm2d(C, eps=EPS32).to(D)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, dtype=D))
        bn.bias.copy_(torch.randn(C, dtype=D))
        bn.running_mean.copy_(torch.randn(C, dtype=D))
        bn.running_var.copy_(torch.rand(C, dtype=D) + 0.1)
    bn.eval()
    x = torch.randn(shape, dtype=D, requires_grad=True)
    go = torch.randn(shape, dtype=D)
    y = _act_torch(bn(x), a)
    y.backward(go)
    mean, rstd = R.bn_eval_stats(bn.running_mean.numpy(), bn.running_var.numpy(), 1e-5)
    gamma, beta = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    _close(R.bn_act_fwd(_nhwc_rows(x), None, mean, rstd, gamma, beta, a)[0], _nhwc_rows(y))
    b = R.bn_act_bwd(_nhwc_rows(x), None, _nhwc_rows(go), mean, rstd, gamma, beta, a, 0, np.full(C, 7.0), "f32")
    _close(b["dx"], _nhwc_rows(x.grad), 2e-7)                                                # eval: xhat_scale plays no part
    _close(b["dgamma"], bn.weight.grad.numpy(), 1e-6)
    _close(b["dbeta"], bn.bias.grad.numpy(), 1e-6)
    # padded channels: (0, 1)
    m2, r2 = R.bn_eval_stats(bn.running_mean.numpy(), bn.running_var.numpy(), 1e-5, c_valid=6)
    assert m2[6:].tolist() == [0.0, 0.0] and r2[6:].tolist() == [1.0, 1.0] and np.array_equal(m2[:6], mean[:6]) and np.array_equal(r2[:6], rstd[:6])


@pytest.mark.parametrize("two", [False, True])
def test_eval_fold_matches_two_batchnorms_behind_a_bias(two):
    torch.manual_seed(5)
    C = 8
    bns = [torch.nn.BatchNorm2d(C, eps=e).to(D).eval() for e in (EPS32, float(np.float32(0.3)))]
    for bn in bns:
        with torch.no_grad():
            bn.weight.copy_(torch.randn(C, dtype=D)); bn.bias.copy_(torch.randn(C, dtype=D))
            bn.running_mean.copy_(torch.randn(C, dtype=D)); bn.running_var.copy_(torch.rand(C, dtype=D) + 0.1)
    conv, bias = torch.randn(2, C, 3, 3, dtype=D), torch.randn(C, dtype=D)
    y = bns[0](conv + bias.view(1, C, 1, 1))
    if two:
        y = bns[1](y)
    n = lambda t: t.detach().numpy()
    second = (n(bns[1].running_mean), n(bns[1].running_var), n(bns[1].weight), n(bns[1].bias), 0.3) if two else (None, None, None, None, 0.0)
    scale, shift, _ = R.bn_eval_fold(n(bns[0].running_mean), n(bns[0].running_var), n(bns[0].weight), n(bns[0].bias), 1e-5, *second, conv_bias=n(bias), c_valid=6)
    # eps 0.3 is not a float32: the reference takes the float the ABI carries
    _close((_nhwc_rows(conv) * scale + shift)[:, :6], _nhwc_rows(y)[:, :6], 1e-7)
    assert not scale[6:].any() and not shift[6:].any()


# ------------------------------------------------------------------------------------------------
# the pair
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps1,eps2", [(1e-5, 1e-5), (0.25, 0.5)])
def test_pair_matches_bn2_of_bn1(eps1, eps2):
    """eps values that are float32 numbers, so torch's float64 modules and the ABI's floats agree"""
    torch.manual_seed(11)
    shape, C = (2, 8, 4, 3), 8
    eps1, eps2 = float(np.float32(eps1)), float(np.float32(eps2))
    bn1, bn2 = torch.nn.BatchNorm2d(C, eps=eps1).to(D), torch.nn.BatchNorm2d(C, eps=eps2, momentum=0.125).to(D)
    with torch.no_grad():
        for bn in (bn1, bn2):
            bn.weight.copy_(torch.randn(C, dtype=D) * 0.5 + 1.0); bn.bias.copy_(torch.randn(C, dtype=D))
        bn2.running_mean.copy_(torch.randn(C, dtype=D)); bn2.running_var.copy_(torch.rand(C, dtype=D) + 0.5)
    rm0, rv0 = bn2.running_mean.clone().numpy(), bn2.running_var.clone().numpy()
    x = torch.randn(shape, dtype=D, requires_grad=True)
    go = torch.randn(shape, dtype=D)
    y = bn2(bn1(x))
    y.backward(go)
    xr, gr = _nhwc_rows(x), _nhwc_rows(go)
    M = xr.shape[0]
    st = R.bn_stats(xr, eps1)
    g1, b1, g2, b2 = (t.detach().numpy() for t in (bn1.weight, bn1.bias, bn2.weight, bn2.bias))
    comp = R.bn_pair_compose(st["rstd"], g1, b1, g2, M, eps1, eps2, 0.125, rm0, rv0)
    _close(comp["running_mean2"], bn2.running_mean.numpy(), 1e-9)
    _close(comp["running_var2"], bn2.running_var.numpy(), 1e-9)
    _close(R.bn_act_fwd(xr, None, st["mean"], st["rstd"], comp["gamma_eff"], b2, NONE)[0], _nhwc_rows(y), 1e-9)
    b = R.bn_act_bwd(xr, None, gr, st["mean"], st["rstd"], comp["gamma_eff"], b2, NONE, 1, comp["xhat_scale"], "f32")
    _close(b["dx"], _nhwc_rows(x.grad), 1e-6)
    pg = R.pair_grads(comp["dgamma2_coef"], comp["dgamma1_coef"], b["dgamma"])
    _close(pg[0], bn2.weight.grad.numpy(), 1e-6)
    _close(pg[1], bn1.weight.grad.numpy(), 1e-6)                                            # the eps2-proportional dgamma1
    assert not pg[2].any() and np.abs(bn1.bias.grad.numpy()).max() < 1e-12                   # dbeta1 = 0
    _close(b["dbeta"], bn2.bias.grad.numpy(), 1e-6)
    # padded channels keep their running statistics; M = 1 uses the factor 1
    c6 = R.bn_pair_compose(st["rstd"], g1, b1, g2, M, eps1, eps2, 0.1, rm0, rv0, c_valid=6)
    assert np.array_equal(c6["running_mean2"][6:], rm0[6:]) and np.array_equal(c6["running_var2"][6:], rv0[6:])
    c1 = R.bn_pair_compose(st["rstd"], g1, b1, g2, 1, eps1, eps2, 1.0, rm0, rv0)
    _close(c1["running_var2"], g1 * g1 * c1["q"], 1e-14)


# ------------------------------------------------------------------------------------------------
# device-only rules by hand
# ------------------------------------------------------------------------------------------------
def test_device_rules_by_hand():
    x = np.array([[1.0, -2.0, 3.0, 0.5]])
    rm0, rv0 = np.array([1.0, 1.0, 1.0, 1.0]), np.array([2.0, 2.0, 2.0, 2.0])
    st = R.bn_stats(x, 1e-5, 0.5, rm0, rv0, c_valid=3)                                         # M = 1: variance 0, unbiased factor 1
    assert np.array_equal(st["mean"], x[0]) and not st["var"].any()
    _close(st["rstd"], np.full(4, 1.0 / math.sqrt(float(np.float32(1e-5)))))
    assert st["running_mean"].tolist() == [1.0, -0.5, 2.0, 1.0] and st["running_var"].tolist() == [1.0, 1.0, 1.0, 2.0]
    x2 = np.array([[1.0, 0.0], [3.0, 0.0]])
    st2 = R.bn_stats(x2, 0.0, 1.0, np.zeros(2), np.zeros(2))
    assert st2["var"].tolist() == [1.0, 0.0] and st2["running_var"].tolist() == [2.0, 0.0]         # M / (M - 1) = 2
    # the dx scale rule
    assert R.dx_scale(0.0) == 1.0 and R.dx_scale(float("inf")) == 1.0 and R.dx_scale(float("nan")) == 1.0
    assert R.dx_scale(2.0 ** 13) == 1.0
    assert R.dx_scale(np.nextafter(np.float32(2.0 ** 14), np.float32(0))) == 1.0
    assert R.dx_scale(2.0 ** 14) == 0.5 and R.dx_scale(np.nextafter(np.float32(2.0 ** 13), np.float32(0))) == 2.0
    assert R.dx_scale(1e-40) == 1.0                                                             # a subnormal float32
    assert R.dx_scale(2.0 ** -126) == 2.0 ** 100 and R.dx_scale(3e38) == 2.0 ** -100            # the exponent clamped at +-100
    for bnd in (1e-8, 0.37, 1.0, 5e4):
        assert 2.0 ** 13 <= R.dx_scale(bnd) * float(np.float32(bnd)) < 2.0 ** 14
    # dz is rounded to the storage type before it is summed and applied
    b = R.bn_act_bwd(np.array([[0.0], [1.0]]), None, np.array([[1.0 + 2.0 ** -12], [0.0]]), [0.5], [2.0], [1.0], [0.0], NONE, 1, None, "f16")
    assert b["dz"][0, 0] == 1.0 and b["dbeta"][0] == 1.0
    # the reference's padded-channel bound: a degenerate channel bounds itself with 0
    r = R.bn_act_bwd(np.zeros((4, 1)), None, np.zeros((4, 1)), [0.0], [316.0], [1.0], [0.0], GELU, 1, None, "f32")
    assert R.dx_bound_per_channel(r).tolist() == [0.0]
    s, sa = R.colsum(np.array([[1.0, -1.0], [2.0, -3.0]]))
    assert s.tolist() == [3.0, -4.0] and sa.tolist() == [3.0, 4.0]


# ------------------------------------------------------------------------------------------------
# LayerNorm with a full-shape affine
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,shape", [(1, (2, 2, 2)), (3, (4, 3, 2)), (5, (8, 1, 1))])
def test_layernorm_matches_torch(B, shape):
    torch.manual_seed(B)
    L = int(np.prod(shape))
    x = (torch.randn((B,) + shape, dtype=D) * 2 + 0.5).requires_grad_(True)
    w, b = (torch.randn(shape, dtype=D) * 0.5 + 1).requires_grad_(True), torch.randn(shape, dtype=D).requires_grad_(True)
    dy = torch.randn((B,) + shape, dtype=D)
    y = F.layer_norm(x, shape, w, b, EPS32)
    y.backward(dy)
    n = lambda t: t.detach().numpy()
    f = R.ln_sample_fwd(n(x).reshape(B, L), n(w).reshape(L), n(b).reshape(L), 1e-5)
    _close(f["y"], n(y).reshape(B, L), 1e-9)                                                  # (eps as the float the ABI carries)
    g = R.ln_sample_bwd(n(x).reshape(B, L), n(dy).reshape(B, L), n(w).reshape(L), f["mean"], f["rstd"])
    _close(g["dx"], n(x.grad).reshape(B, L), 1e-9)
    _close(g["dw"], n(w.grad).reshape(L), 1e-9)
    _close(g["db"], n(b.grad).reshape(L), 1e-12)


# ------------------------------------------------------------------------------------------------
# the GPU file's input recipes meet their own conditions
# ------------------------------------------------------------------------------------------------
def test_gpu_shape_sets_hit_the_edges_they_name():
    stat_blocks = lambda M: min(max(M // 32, 1), 1024)
    assert [stat_blocks(M) for M in E.STAT_BIG_M] == [63, 64, 65, 1023, 1024, 1024, 1024]
    assert [min(stat_blocks(M), 768) for M in E.BWD_BIG_M] == [767, 768, 768, 768, 768]
    assert E.rpi_of(152, "f32") == 6 and E.rpi_of(24, "f16") == 85 and E.rpi_of(1024, "f32") == 1 and E.rpi_of(2048, "f16") == 1
    assert E.stat_M_edges(152, "f32") == [1, 31, 32, 33, 47, 48, 49, 97]
    assert E.bwd_M_edges(152, "f32") == [1, 2, 11, 12, 13]
    for C, nvec in ((8, 4), (24, 8), (152, 4), (1024, 8)):
        cv, Ms = C // nvec, E.fwd_M_set(C, nvec)
        for k in (1024, 2048):
            tot = [M * cv for M in Ms]
            assert max(t for t in tot if t < k) > k - 1 - cv and min(t for t in tot if t >= k) < k + cv and any(t > k for t in tot)
    # ew_grid of the large case rounds above its cap; the large colsum runs 17 iterations; the large LayerNorm has 8193 blocks' worth
    m = 19 // math.gcd(19, 256)
    g = min((442000 * 19 + 1023) // 1024, 8192)
    assert (g + m - 1) // m * m == 8208 > 8192
    assert -(-(-(-66000 // 1024)) // 4) == 17
    assert (8388616 // 4 + 255) // 256 == 8193


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_gpu_relu_recipes_leave_no_pre_activation_inside_its_margin(storage):
    for C, M in ((8, 1), (8, 2), (24, 13), (152, 12), (8, 24544)):
        for use_res in (False, True):
            x, res, go, mean, rstd, gamma, beta = E.bwd_inputs(storage, C, M, RELU, use_res)
            assert E.relu_margin_ok(storage, x, res, mean, rstd, gamma, beta)
            assert x.dtype == E.NP[storage] and gamma[0] == 0.0 and gamma[1] < 0.0
    x, res, go, mean, rstd, gamma, beta, cv = E.h_inputs(24, 300, RELU, True, 1.0)
    assert cv == 19 and not x[:, cv:].any() and not go[:, cv:].any() and E.relu_margin_ok("f32", x[:, :cv], res[:, :cv], mean[:cv], rstd[:cv], gamma[:cv], beta[:cv])


def test_gpu_other_recipes():
    for eps1 in (1e-5, 0.2):
        rstd1, gamma1, beta1, gamma2, rm0, rv0 = E.compose_inputs(19, eps1)
        c = R.bn_pair_compose(rstd1, gamma1, beta1, gamma2, 100, eps1, 0.3)
        assert c["q"][1] == 0.0 and 0.0 <= c["q"][0] < 1e-6 and (c["q"][2:] > 0).all()
        assert 1.0 - float(np.float32(eps1)) * float(rstd1[1]) ** 2 < 0.0                      # the clamp is exercised
        _close(c["r2"][:2], np.full(2, 1.0 / math.sqrt(float(np.float32(0.3)))), 1e-6)
    for storage, rs in (("f32", (0, 30, 300)), ("f16", (0, 30))):
        for r in rs:
            x, _, _ = E.stats_inputs(storage, 8, 4096, r)
            st = R.bn_stats(x, 1e-5)
            assert st["var"][3] == 0.0 and (np.delete(st["var"], 3) > 0.8).all() and abs(st["mean"][0] - r) < 0.1
    x, res, mean, rstd, gamma, beta = E.fwd_inputs("f16", 8, 1025)
    _, pre = R.bn_act_fwd(x, res, mean, rstd, gamma, beta, GELU)
    assert np.array_equal(pre[:8, E.SPECIAL_CH], E.GELU_SPECIALS.astype(np.float16).astype(np.float64)) and gamma[0] == 0.0 and gamma[1] < 0.0
    part, _, _ = E.rows_inputs(65, 19)
    assert part.shape == (65, 19, 2) and part.dtype == np.float32
    # the decoder of the chunk encoding inverts a hand-made chunk: hi = (1, 2, 3, 4) as bf16, lo = 2^-9 each
    hi = (np.array([1, 2, 3, 4], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint32)
    lo = np.uint32(np.float32(2.0 ** -9).view(np.uint32) >> 16)
    words = np.array([[hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), lo | (lo << 16), lo | (lo << 16)]], dtype=np.uint32)
    assert E._decode_bf16x4(words).tolist() == [[1 + 2.0 ** -9, 2 + 2.0 ** -9, 3 + 2.0 ** -9, 4 + 2.0 ** -9]]
