"""Shared GPU parity checks: every function runs HIP ops (through maskunet_amd -> C ABI) and the CPU
oracle / stock torch reference on the same seeded inputs and returns [(name, err, tol)] where err is the
max abs error normalised by max(1, |ref|_max).  Used by the pytest files and by tests/aids/gpu_report.py.

Tolerances: fp32 compute 1e-3 (the north_star gate; observed errors are ~1e-5), fp16 compute 3e-2
(fp16 storage, fp32 accumulate; BASELINE.md expects ~1e-2-class errors for half precision).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import maskunet_oracle as O

import os

TOL = {torch.float32: 1e-3, torch.float16: 3e-2}
# parameter gradients of a module case are compared against max(|ref|max, PARAM_GRAD_FLOOR * the case's largest parameter gradient)
PARAM_GRAD_FLOOR = {torch.float32: 1e-3, torch.float16: 5e-2}
# whole-model parameter gradients against the oracle (check_unet_vs_oracle; the max-norm gate also in check_unet_golden): the floor of
# the case's largest gradient below which a gradient counts as rounding noise, the loose max-norm gate and the tight 1 - cosine gate
UNET_GRAD_FLOOR = {torch.float32: 1e-3, torch.float16: 1e-2}
UNET_GRAD_MAXREL = {torch.float32: 5e-2, torch.float16: 3e-1}
UNET_GRAD_COS = {torch.float32: 1e-4, torch.float16: 2e-2}
# static loss scale used for the fp16 backward in whole-model checks (fp16 activation gradients underflow
# without one: d(loss)/d(logit) ~ 1/(B*H*W)); fp32 needs none
FP16_LOSS_SCALE = float(os.environ.get("MU_LOSS_SCALE", "1024"))
DEV = "cuda"


def _err(got, ref):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    scale = max(1.0, float(ref.abs().max()))
    return float((got - ref).abs().max()) / scale


def _rel_err(got, ref):
    """error relative to the reference's own max (for gradients whose scale is far from 1)."""
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def _rnd(gen, *shape, scale=1.0):
    return torch.from_numpy((gen.standard_normal(shape) * scale).astype(np.float32))


def nhwc(x_nchw, dtype):
    from maskunet_amd import ops
    return ops.to_nhwc(x_nchw.to(DEV), dtype)


# ------------------------------------------------------------------------------------------------
def check_transpose(dtype):
    from maskunet_amd import _lib
    gen = np.random.default_rng(1)
    out = []
    for (B, R, C, sld, dld) in [(3, 70, 45, 45, 70), (2, 64, 150, 160, 64), (1, 130, 33, 40, 136)]:
        src = torch.zeros(B, R, sld)
        src[:, :, :C] = _rnd(gen, B, R, C)
        s = src.to(DEV, dtype)
        d = torch.zeros(B, C, dld, dtype=torch.float32, device=DEV)
        _lib.call("mu_transpose", _lib.ptr(s), _lib.dt(s), sld, _lib.ptr(d), _lib.dt(d), dld, B, R, C, _lib.stream())
        ref = torch.zeros(B, C, dld)
        ref[:, :, :R] = s.float().cpu()[:, :, :C].transpose(1, 2)
        out.append((f"transpose{(B, R, C)}", _err(d, ref), 1e-6))
    # zero padding of destination rows [R, R_pad) over a garbage-filled destination: aligned (vector) and unaligned paths
    for (B, R, C, sld, dld, Rp) in [(2, 3, 200, 200, 32, 32), (2, 150, 96, 96, 160, 160), (1, 19, 45, 45, 35, 33), (2, 70, 130, 132, 96, 90)]:
        src = torch.zeros(B, R, sld)
        src[:, :, :C] = _rnd(gen, B, R, C)
        s = src.to(DEV, dtype)
        for ddt in (torch.float32, dtype):
            d = torch.full((B, C, dld), 7.0, dtype=ddt, device=DEV)
            _lib.call("mu_transpose_pad", _lib.ptr(s), _lib.dt(s), sld, _lib.ptr(d), _lib.dt(d), dld, B, R, C, Rp, _lib.stream())
            ref = torch.full((B, C, dld), 7.0)
            ref[:, :, :Rp] = 0
            ref[:, :, :R] = s.float().cpu()[:, :, :C].transpose(1, 2)
            out.append((f"transpose_pad{(B, R, C, Rp)}->{str(ddt)[6:]}", _err(d.float(), ref), 1e-6))
    return out


def check_prep_weight(dtype):
    """OIHW fp32 -> tap-major compute layouts: forward, flipped/transposed data-gradient, and both from one launch."""
    from maskunet_amd import _lib
    gen = np.random.default_rng(11)
    out = []
    for (O, I, k) in [(19, 3, 3), (64, 32, 3), (150, 64, 1), (96, 160, 3)]:
        taps = k * k
        w = _rnd(gen, O, I, k, k)
        wd = w.to(DEV)
        Op, Ip = (O + 31) // 32 * 32, (I + 31) // 32 * 32
        ref0 = torch.zeros(taps, Op, Ip)
        ref0[:, :O, :I] = w.reshape(O, I, taps).permute(2, 0, 1)
        ref1 = torch.zeros(taps, Ip, Op)
        ref1[:, :I, :O] = w.reshape(O, I, taps).flip(2).permute(2, 1, 0)
        ref0, ref1 = ref0.to(dtype).float(), ref1.to(dtype).float()
        d0 = torch.full((taps, Op, Ip), 7.0, dtype=dtype, device=DEV)
        d1 = torch.full((taps, Ip, Op), 7.0, dtype=dtype, device=DEV)
        d2 = torch.full((2 * taps * Op * Ip,), 7.0, dtype=dtype, device=DEV)
        _lib.call("mu_prep_weight", _lib.ptr(wd), _lib.ptr(d0), _lib.dt(d0), O, I, taps, Op, Ip, 0, _lib.stream())
        _lib.call("mu_prep_weight", _lib.ptr(wd), _lib.ptr(d1), _lib.dt(d1), O, I, taps, Ip, Op, 1, _lib.stream())
        _lib.call("mu_prep_weight", _lib.ptr(wd), _lib.ptr(d2), _lib.dt(d2), O, I, taps, Op, Ip, 2, _lib.stream())
        n = taps * Op * Ip
        out += [(f"prep{(O, I, k)} fwd", _err(d0.float(), ref0), 0.0), (f"prep{(O, I, k)} dgrad", _err(d1.float(), ref1), 0.0),
                (f"prep{(O, I, k)} both/fwd", _err(d2[:n].view(taps, Op, Ip).float(), ref0), 0.0),
                (f"prep{(O, I, k)} both/dgrad", _err(d2[n:].view(taps, Ip, Op).float(), ref1), 0.0)]
    return out


def check_layout_roundtrip(dtype):
    from maskunet_amd import ops
    gen = np.random.default_rng(2)
    x = _rnd(gen, 2, 19, 6, 10).to(DEV).requires_grad_(True)
    y = ops.to_nhwc(x, dtype)
    assert y.shape == (2, 6, 10, 32)
    z = ops.to_nchw(y, 19, torch.float32)
    g = _rnd(gen, 2, 19, 6, 10).to(DEV)
    z.backward(g)
    tol = 1e-6 if dtype == torch.float32 else 2e-3
    return [("layout fwd", _err(z, x), tol), ("layout pad zero", float(y[..., 19:].abs().max()), 0.0),
            ("layout bwd", _err(x.grad, g), tol)]


def check_conv(dtype, cases=None):
    from maskunet_amd import ops
    gen = np.random.default_rng(3)
    out = []
    from tests._conv_cases import CONV_CASES
    cases = cases or CONV_CASES
    for (B, H, W, Cin, Cout, k) in cases:
        x = _rnd(gen, B, Cin, H, W)
        w = _rnd(gen, Cout, Cin, k, k, scale=1.0 / math.sqrt(Cin * k * k))
        b = _rnd(gen, Cout, scale=0.1) if k == 1 else None
        g = _rnd(gen, B, Cout, H, W)
        # reference on CPU (inputs rounded to the storage dtype so only accumulation differs)
        xr = x.to(dtype).float().clone().requires_grad_(True)
        wr = w.clone().requires_grad_(True)
        br = b.clone().requires_grad_(True) if b is not None else None
        yr = F.conv2d(xr, wr, br, padding=k // 2)
        yr.backward(g.to(dtype).float())
        xd = x.to(DEV).requires_grad_(True)
        wd = w.to(DEV).requires_grad_(True)
        bd = b.to(DEV).requires_grad_(True) if b is not None else None
        y = ops.to_nchw(ops.conv(ops.to_nhwc(xd, dtype), wd, bd), Cout, torch.float32)
        y.backward(g.to(DEV))
        tol = TOL[dtype]
        tag = f"conv{(B, H, W, Cin, Cout, k)}"
        out += [(tag + " y", _err(y, yr), tol), (tag + " dx", _rel_err(xd.grad, xr.grad), tol),
                (tag + " dw", _rel_err(wd.grad, wr.grad), tol)]
        if b is not None:
            out.append((tag + " db", _rel_err(bd.grad, br.grad), tol))
    return out


def check_conv_fused(dtype, fp32x=False):
    """mu_conv_fwd_fused through the C ABI on Gaussian inputs against fp64: y = act(conv(x, w) * scale + shift + res) with a random
    positive scale and a random shift, every activation, with and without the residual, over the fused cases of the shape table
    (every branch of the fused dispatch: see tests/test_conv_plan_coverage.py)."""
    from maskunet_amd import _lib
    from tests import _conv_cases as CC
    gen = np.random.default_rng(17)
    out = []
    code = _lib.MU_F32X if fp32x else _lib.dt(dtype)
    st = _lib.stream()
    for c in CC.LAYERS:
        if c["heavy"]:
            continue
        B, H, W, Cin, Cout, taps, cin, cout = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["taps"], c["cin"], c["cout"]
        k = 3 if taps == 9 else 1
        kern = CC.plan_name("fused", _lib.load().mu_conv_fwd_fused_plan(B, H, W, Cin, Cout, taps, code))
        x = _rnd(gen, B, cin, H, W).to(dtype).float()
        w = _rnd(gen, cout, cin, k, k, scale=1.0 / math.sqrt(cin * k * k))
        scale = torch.from_numpy(gen.uniform(0.5, 1.5, Cout).astype(np.float32))
        shift = _rnd(gen, Cout, scale=0.3)
        res = _rnd(gen, B, H, W, Cout).to(dtype).float()
        xd = torch.zeros(B, H, W, Cin)
        xd[..., :cin] = x.permute(0, 2, 3, 1)
        xd = xd.to(DEV, dtype)
        if fp32x:
            xe = torch.empty_like(xd)
            _lib.call("mu_split_encode_h4" if taps == 9 else "mu_split_encode", xd.data_ptr(), xe.data_ptr(), xd.numel(), st)
            xd = xe
        wd = w.to(DEV).contiguous()
        wp = torch.empty(taps * Cout * Cin, dtype=dtype, device=DEV)
        _lib.call("mu_prep_weight", wd.data_ptr(), wp.data_ptr(), code, cout, cin, taps, Cout, Cin, 0, st)
        sd, hd, rd = scale.to(DEV), shift.to(DEV), res.to(DEV, dtype)
        conv = torch.zeros(B, H, W, Cout, dtype=torch.float64)
        conv[..., :cout] = F.conv2d(x.double(), (w.to(dtype).double() if dtype == torch.float16 else w.double()), None, padding=k // 2).permute(0, 2, 3, 1)
        for act in (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_RELU):
            for use_res in (False, True):
                y = torch.full((B, H, W, Cout), float("nan"), dtype=dtype, device=DEV)
                _lib.call("mu_conv_fwd_fused", xd.data_ptr(), wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), rd.data_ptr() if use_res else None, act,
                          y.data_ptr(), B, H, W, Cin, Cout, taps, Cin, Cout, code, st)
                pre = conv * scale.double() + shift.double() + (res.double() if use_res else 0)
                ref = F.gelu(pre) if act == _lib.ACT_GELU else (pre.clamp(min=0) if act == _lib.ACT_RELU else pre)
                out.append((f"conv_fused[{kern}]{(B, H, W, cin, cout, k)} act{act} res{int(use_res)}", _err(y, ref), TOL[dtype]))
    return out


def check_conv_stats(dtype):
    """BatchNorm statistics rows left by the conv epilogue == column sums / sums of squares of the conv output it wrote.  fp16: the
    ping-pong kernel (Cout % 128, H % 16) and the halo-tile kernel (Cout = 64; H % 8 only; Cin >= 128 takes its ring variant).
    fp32: the same shapes in the fp32x mode (exact fp32 has no statistics epilogue: rows == 0)."""
    from maskunet_amd import ops, _lib
    gen = np.random.default_rng(12)
    out = []
    if dtype == torch.bfloat16:
        return [("conv_stats (fp16 / fp32x only)", 0.0, 0.0)]
    shapes = [(2, 16, 32, 64, 128), (3, 32, 32, 128, 256), (8, 64, 64, 64, 128),      # the last runs the persistent kernel
              (2, 16, 32, 64, 64), (2, 24, 16, 128, 64), (3, 8, 48, 64, 128), (1, 40, 16, 256, 256),
              (10, 128, 112, 64, 64), (3, 192, 240, 64, 64)]      # the last two (fp16): weights-resident kernel, 4 rows per tile
    import maskunet_amd
    prev = maskunet_amd.get_float32_matmul_precision()
    if dtype == torch.float32:
        maskunet_amd.set_float32_matmul_precision("high")
    try:
        for (B, H, W, Cin, Cout) in shapes:
            x = ops.to_nhwc(_rnd(gen, B, Cin, H, W).to(DEV), dtype)
            w = _rnd(gen, Cout, Cin, 3, 3, scale=1.0 / math.sqrt(Cin * 9)).to(DEV)
            bias = _rnd(gen, Cout, scale=0.3).to(DEV)
            y, part = ops.conv_stats(x, w, bias)
            rows = _lib.load().mu_conv_stats_rows(B, H, W, Cin, Cout, 9, ops.mdt(x))
            assert rows > 0 and part.numel() > 0 and part.shape[0] == rows, (B, H, W, Cin, Cout, rows, tuple(part.shape))
            yf = y.float().reshape(-1, Cout)
            ssum, ssq = part[:, :, 0].double().sum(0), part[:, :, 1].double().sum(0)
            out += [(f"conv_stats{(B, H, W, Cin, Cout)} sum", float((ssum - yf.double().sum(0)).abs().max() / yf.abs().sum(0).max()), 1e-5),
                    (f"conv_stats{(B, H, W, Cin, Cout)} sumsq", float((ssq - (yf.double() ** 2).sum(0)).abs().max() / (yf.double() ** 2).sum(0).max()), 1e-5)]
    finally:
        maskunet_amd.set_float32_matmul_precision(prev)
    return out


def check_bn_act(dtype):
    from maskunet_amd import ops, _lib
    import torch.nn as nn
    gen = np.random.default_rng(4)
    out = []
    for (B, C, H, W, act, use_res, training) in [(2, 32, 6, 6, _lib.ACT_GELU, False, True), (2, 19, 8, 8, _lib.ACT_RELU, False, True),
                                                 (3, 64, 5, 7, _lib.ACT_GELU, True, True), (2, 150, 4, 4, _lib.ACT_NONE, False, True),
                                                 (2, 64, 6, 6, _lib.ACT_GELU, True, False), (1, 512, 16, 16, _lib.ACT_NONE, False, True),
                                                 # every (activation, residual) instantiation of the BatchNorm passes (compile-time constants since round 5)
                                                 (2, 40, 5, 5, _lib.ACT_RELU, True, True), (2, 24, 6, 5, _lib.ACT_NONE, True, True)]:
        x = _rnd(gen, B, C, H, W) * 1.5 + 0.3
        r = _rnd(gen, B, C, H, W) if use_res else None
        g = _rnd(gen, B, C, H, W)
        bn_ref = nn.BatchNorm2d(C)
        with torch.no_grad():
            bn_ref.weight.copy_(torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32)))
            bn_ref.bias.copy_(torch.from_numpy(gen.uniform(-0.2, 0.2, C).astype(np.float32)))
            bn_ref.running_mean.copy_(_rnd(gen, C, scale=0.1))
            bn_ref.running_var.copy_(torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32)))
        bn_dev = nn.BatchNorm2d(C)
        bn_dev.load_state_dict(bn_ref.state_dict())
        bn_dev.to(DEV)
        bn_ref.train(training)
        bn_dev.train(training)
        xr = x.to(dtype).float().clone().requires_grad_(True)
        rr = r.to(dtype).float().clone().requires_grad_(True) if use_res else None
        pre = bn_ref(xr) + (rr if use_res else 0)
        yr = {_lib.ACT_GELU: F.gelu, _lib.ACT_RELU: torch.relu, _lib.ACT_NONE: lambda t: t}[act](pre)
        yr.backward(g.to(dtype).float())
        xd = x.to(DEV).requires_grad_(True)
        rd = r.to(DEV).requires_grad_(True) if use_res else None
        y = ops.bn_act(ops.to_nhwc(xd, dtype), bn_dev, act, res=ops.to_nhwc(rd, dtype) if use_res else None)
        y = ops.to_nchw(y, C, torch.float32)
        y.backward(g.to(DEV))
        tol = TOL[dtype]
        tag = f"bn{(B, C, H, W)}a{act}r{int(use_res)}t{int(training)}"
        out += [(tag + " y", _err(y, yr), tol), (tag + " dx", _rel_err(xd.grad, xr.grad), tol),
                (tag + " dgamma", _rel_err(bn_dev.weight.grad, bn_ref.weight.grad), tol),
                (tag + " dbeta", _rel_err(bn_dev.bias.grad, bn_ref.bias.grad), tol),
                (tag + " rmean", _err(bn_dev.running_mean, bn_ref.running_mean), tol),
                (tag + " rvar", _err(bn_dev.running_var, bn_ref.running_var), tol),
                (tag + " num_batches_tracked", abs(int(bn_dev.num_batches_tracked) - int(bn_ref.num_batches_tracked)), 0.0)]
        if use_res:
            out.append((tag + " dres", _rel_err(rd.grad, rr.grad), tol))
    return out


def check_bn_pair(dtype):
    """ops.bn_pair == bn2(bn1(x)) of two nn.BatchNorm2d in training mode (fp64 reference): output, input gradient, all four
    parameter gradients, both layers' running statistics and step counters (ade_semantic.py:216-219, 237-240)."""
    from maskunet_amd import ops
    import torch.nn as nn
    gen = np.random.default_rng(41)
    out = []
    # large eps values make the eps-proportional terms (dgamma1, var/(var+eps) < 1) first-order effects
    for (B, C, H, W, eps1, eps2) in [(2, 32, 6, 6, 1e-5, 1e-5), (3, 64, 5, 7, 1e-5, 1e-5), (2, 19, 8, 8, 1e-5, 1e-5),
                                     (1, 256, 16, 16, 1e-5, 1e-5), (2, 32, 6, 6, 0.2, 0.3)]:
        x = _rnd(gen, B, C, H, W) * 1.5 + 0.3
        if C == 64:
            x[:, 3] *= 1e-3                       # a channel whose variance is comparable to eps (var/(var+eps) well below 1)
        g = _rnd(gen, B, C, H, W)
        refs, devs = [], []
        for eps in (eps1, eps2):
            bn = nn.BatchNorm2d(C, eps=eps)
            with torch.no_grad():
                bn.weight.copy_(torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32)))
                bn.bias.copy_(torch.from_numpy(gen.uniform(-0.2, 0.2, C).astype(np.float32)))
                bn.running_mean.copy_(_rnd(gen, C, scale=0.1))
                bn.running_var.copy_(torch.from_numpy(gen.uniform(0.5, 1.5, C).astype(np.float32)))
            d = nn.BatchNorm2d(C, eps=eps)
            d.load_state_dict(bn.state_dict())
            refs.append(bn.double().train())
            devs.append(d.to(DEV).train())
        xr = x.to(dtype).double().clone().requires_grad_(True)
        yr = refs[1](refs[0](xr))
        yr.backward(g.to(dtype).double())
        xd = x.to(DEV).requires_grad_(True)
        y = ops.to_nchw(ops.bn_pair(ops.to_nhwc(xd, dtype), devs[0], devs[1]), C, torch.float32)
        y.backward(g.to(DEV))
        tol = TOL[dtype]
        # the two layers one after the other (MU_BN_PAIR=0) carry fp16 rounding noise in the first layer's near-zero gradients
        ztol = tol * 1e-2 if ops.BN_PAIR else tol
        tag = f"bnpair{(B, C, H, W, eps1, eps2)}"
        gscale = float(refs[1].weight.grad.abs().max())
        out += [(tag + " y", _err(y, yr.float()), tol), (tag + " dx", _rel_err(xd.grad, xr.grad.float()), tol),
                (tag + " dgamma2", _rel_err(devs[1].weight.grad, refs[1].weight.grad.float()), tol),
                (tag + " dbeta2", _rel_err(devs[1].bias.grad, refs[1].bias.grad.float()), tol),
                (tag + " dgamma1", _err(devs[0].weight.grad, refs[0].weight.grad.float()) / gscale, ztol),
                (tag + " dbeta1", _err(devs[0].bias.grad, refs[0].bias.grad.float()) / gscale, ztol)]
        for i in range(2):
            out += [(tag + f" rmean{i}", _err(devs[i].running_mean, refs[i].running_mean.float()), tol),
                    (tag + f" rvar{i}", _err(devs[i].running_var, refs[i].running_var.float()), tol),
                    (tag + f" nbt{i}", abs(int(devs[i].num_batches_tracked) - int(refs[i].num_batches_tracked)), 0.0)]
        # eval mode falls back to the two layers one after the other
        for m in refs + devs:
            m.eval()
        ye = refs[1](refs[0](x.to(dtype).double()))
        yd = ops.to_nchw(ops.bn_pair(ops.to_nhwc(x.to(DEV), dtype), devs[0], devs[1]), C, torch.float32)
        out.append((tag + " eval y", _err(yd, ye.float()), tol))
    return out


def check_pool_up(dtype):
    from maskunet_amd import ops
    gen = np.random.default_rng(5)
    out = []
    tol = TOL[dtype]
    x = _rnd(gen, 2, 64, 12, 8)
    g = _rnd(gen, 2, 64, 6, 4)
    xr = x.to(dtype).float().clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    yr.backward(g.to(dtype).float())
    xd = x.to(DEV).requires_grad_(True)
    y = ops.to_nchw(ops.maxpool2(ops.to_nhwc(xd, dtype)), 64, torch.float32)
    y.backward(g.to(DEV))
    out += [("maxpool y", _err(y, yr), tol), ("maxpool dx", _rel_err(xd.grad, xr.grad), tol)]
    # odd sizes: nn.MaxPool2d(2) floors (ade_semantic.py:216); the uncovered last row / column gets a zero gradient
    for (H, W) in [(13, 8), (12, 9), (7, 5), (3, 2)]:
        x = _rnd(gen, 2, 32, H, W)
        g = _rnd(gen, 2, 32, H // 2, W // 2)
        xr = x.to(dtype).float().clone().requires_grad_(True)
        yr = F.max_pool2d(xr, 2)
        yr.backward(g.to(dtype).float())
        xd = x.to(DEV).requires_grad_(True)
        y = ops.to_nchw(ops.maxpool2(ops.to_nhwc(xd, dtype)), 32, torch.float32)
        y.backward(g.to(DEV))
        out += [(f"maxpool{(H, W)} y", _err(y, yr), tol), (f"maxpool{(H, W)} dx", _rel_err(xd.grad, xr.grad), tol)]
    for (B, Cx, Cs, h, w) in [(2, 32, 64, 5, 7), (1, 256, 256, 16, 16), (2, 64, 32, 1, 3)]:
        x = _rnd(gen, B, Cx, h, w)
        s = _rnd(gen, B, Cs, 2 * h, 2 * w)
        g = _rnd(gen, B, Cs + Cx, 2 * h, 2 * w)
        xr = x.to(dtype).float().clone().requires_grad_(True)
        sr = s.to(dtype).float().clone().requires_grad_(True)
        yr = torch.cat([sr, F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=True)], 1)
        yr.backward(g.to(dtype).float())
        xd, sd = x.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
        y = ops.to_nchw(ops.upcat(ops.to_nhwc(xd, dtype), ops.to_nhwc(sd, dtype)), Cs + Cx, torch.float32)
        y.backward(g.to(DEV))
        tag = f"upcat{(B, Cx, Cs, h, w)}"
        out += [(tag + " y", _err(y, yr), tol), (tag + " dx", _rel_err(xd.grad, xr.grad), tol),
                (tag + " dskip", _rel_err(sd.grad, sr.grad), tol)]
    return out


def check_ln_sample(dtype):
    from maskunet_amd import ops
    gen = np.random.default_rng(6)
    B, C, H, W = 3, 64, 16, 16
    x = _rnd(gen, B, C, H, W) * 2 + 0.5
    w = torch.from_numpy(gen.uniform(0.5, 1.5, (C, H, W)).astype(np.float32))
    b = torch.from_numpy(gen.uniform(-0.2, 0.2, (C, H, W)).astype(np.float32))
    g = _rnd(gen, B, C, H, W)
    xr = x.to(dtype).float().clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (C, H, W), wr, br, 1e-5)
    yr.backward(g.to(dtype).float())
    xd = x.to(DEV).to(dtype).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.ln_sample(xd.view(B, -1), wd, bd, 1e-5).view(B, C, H, W)
    y.backward(g.to(DEV).to(dtype))
    tol = TOL[dtype]
    return [("ln_sample y", _err(y, yr), tol), ("ln_sample dx", _rel_err(xd.grad, xr.grad), tol),
            ("ln_sample dw", _rel_err(wd.grad, wr.grad), tol), ("ln_sample db", _rel_err(bd.grad, br.grad), tol)]


def check_dropout(dtype):
    from maskunet_amd import ops
    x = torch.ones(4, 8, 8, 64, device=DEV, dtype=dtype, requires_grad=True)
    torch.manual_seed(5)
    y = ops.dropout(x, 0.3, True)
    keep = (y != 0)
    frac = float(keep.float().mean())
    y.sum().backward()
    same = bool(((x.grad != 0) == keep).all())
    val = float((y[keep].float() - 1 / 0.7).abs().max())
    m = (torch.rand(4, 8, 8, 64) > 0.5).to(torch.uint8)
    y2 = ops.dropout(x, 0.3, True, m)
    ok_mask = bool(((y2 != 0).cpu() == (m != 0)).all())
    return [("dropout keep frac", abs(frac - 0.7), 0.03), ("dropout scale", val, 2e-3), ("dropout bwd mask", 0.0 if same else 1.0, 0.0),
            ("dropout explicit mask", 0.0 if ok_mask else 1.0, 0.0), ("dropout eval identity", 0.0 if ops.dropout(x, 0.3, False) is x else 1.0, 0.0)]


def _attn_modules(C, gen):
    import maskunet_amd
    m = maskunet_amd.Mask2FormerAttention(C, C)
    sd = {}
    for k, v in m.state_dict().items():
        if k.startswith("norm.weight"):
            kind = "gamma"
        elif k.startswith("norm.bias"):
            kind = "beta"
        elif k.endswith("weight"):
            kind = "w"
        else:
            kind = "b%d" % C
        sd[k] = O.make_tensor(gen, tuple(v.shape), kind)
    m.load_state_dict(sd)
    return m, sd


def check_attention(dtype, cases=None):
    gen = np.random.default_rng(7)
    out = []
    cases = cases or [(2, 8, 8, 32), (2, 16, 16, 64), (1, 24, 8, 128), (1, 16, 16, 256), (2, 40, 40, 64), (1, 12, 12, 128),
                      (1, 32, 32, 256), (2, 64, 64, 64), (1, 36, 20, 128),
                      # batches of 8 / 16 images: every XCD owns whole images (XCD-aware block order)
                      (8, 32, 32, 64), (16, 24, 24, 128), (8, 16, 16, 256), (8, 48, 48, 64)]
    for (B, H, W, C) in cases:
        m, sd = _attn_modules(C, gen)
        m.to(DEV).set_compute_dtype(dtype)
        keep = torch.from_numpy(gen.integers(0, 2, size=(B, H * W)).astype(np.uint8))
        keep[:, 0] = 1
        x = _rnd(gen, B, C, H, W)
        g = _rnd(gen, B, C, H, W)
        p = {"m." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
        xr = x.to(dtype).float().clone().requires_grad_(True)
        yr = O.mask_attention(xr, p, "m", keep)
        yr.backward(g.to(dtype).float())
        m.set_keep_mask(keep)
        xd = x.to(DEV).requires_grad_(True)
        y = m(xd)
        y.backward(g.to(DEV))
        tol = TOL[dtype]
        tag = f"attn{(B, H, W, C)}"
        out += [(tag + " y", _err(y, yr), tol), (tag + " dx", _rel_err(xd.grad, xr.grad), tol)]
        for k, v in m.named_parameters():
            gref = p["m." + k].grad
            if k == "key.bias":        # analytically zero gradient (softmax shift invariance): absolute check
                out.append((tag + " d" + k, float(v.grad.abs().max().cpu()), tol * float(p["m.query.bias"].grad.abs().max()) + 1e-6))
            else:
                out.append((tag + " d" + k, _rel_err(v.grad, gref), tol))
    return out


def check_attention_overflow_redo(dtype, fp32x=False, hot=True, gout_scale=1.0):
    """The forward's optimistic sweep (no per-tile running-max tracking, attn.hip) must detect a late score that overflows fp16
    against the first tile's maximum and redo the block exactly (cdna guide rule 26: force the rare branch, full-tensor fp64
    reference).  A kept key far down the list is aligned with a few queries so that its score exceeds every earlier one by ~35 log2
    units; forward (out, PV/l, lse2) and the backward that consumes lse2 are compared with fp64 torch.
    fp32x=True: the MU_F32X entry points on fp16-pair-encoded qkv (mu_split_encode_h); hot=False: no aligned key (plain C-ABI parity
    run); gout_scale: magnitude of the incoming gradient."""
    from maskunet_amd import _lib
    B, N, C = 2, 1024, 64
    g_ = torch.Generator().manual_seed(77)
    qkv = torch.randn(B, N, 3 * C, generator=g_)
    x = torch.randn(B, N, C, generator=g_)
    keep = torch.randint(0, 2, (B, N), generator=g_, dtype=torch.uint8)
    keep[:, 900] = 1
    hot_q = [3, 200, 777]
    for b in range(B if hot else 0):
        for i in hot_q:
            qkv[b, i, :C] = qkv[b, i, :C] * (8.0 / qkv[b, i, :C].norm())
        qkv[b, 900, C:2 * C] = 3.5 * qkv[b, 3, :C] + 3.5 * qkv[b, 200, :C] + 3.5 * qkv[b, 777, :C]     # key 900: late in the kept list
    qkv = qkv.to(dtype)
    x = x.to(dtype)
    gam = torch.rand(C, generator=g_) + 0.5
    bet = torch.randn(C, generator=g_) * 0.1
    gout = (torch.randn(B, N, C, generator=g_) * gout_scale).to(dtype)
    # fp64 reference
    qr = qkv.double().clone().requires_grad_(True)
    xr = x.double().clone().requires_grad_(True)
    q, k, v = qr[..., :C], qr[..., C:2 * C], qr[..., 2 * C:]
    sc = q @ k.transpose(1, 2) / (C ** 0.5)
    sc = sc + torch.where(keep[:, None, :] > 0, 0.0, -float("inf"))
    pv = torch.softmax(sc, -1) @ v
    ref = F.layer_norm(pv + xr, (C,), gam.double(), bet.double(), 1e-5)
    ref.backward(gout.double())
    lse_ref = torch.logsumexp(sc, -1) * 1.4426950408889634
    d = DEV
    qd, xd, kd = qkv.to(d), x.to(d), keep.to(d)
    kidx = torch.argsort(kd, dim=1, descending=True, stable=True).to(torch.int32).contiguous()
    kcnt = kd.sum(1, dtype=torch.int32).contiguous()
    gd, bd = gam.to(d), bet.to(d)
    out, oattn = torch.empty_like(xd), torch.empty_like(xd)
    lse = torch.empty(B, N, device=d)
    mean, rstd, delta = torch.empty_like(lse), torch.empty_like(lse), torch.empty_like(lse)
    st = _lib.stream()
    cdt = _lib.MU_F32X if fp32x else _lib.dt(xd)
    if fp32x:
        _lib.call("mu_split_encode_h", qd.data_ptr(), qd.data_ptr(), qd.numel(), st)
    _lib.call("mu_attn_fwd", qd.data_ptr(), xd.data_ptr(), kidx.data_ptr(), kcnt.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(),
              oattn.data_ptr(), lse.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, N, C, N, 1e-5, cdt, st)
    dY, dqkv = torch.empty_like(xd), torch.empty_like(qd)
    dg, db = torch.empty(C, device=d), torch.empty(C, device=d)
    ws = _lib.workspace(_lib.load().mu_attn_bwd_workspace_bytes(B, N, C), torch.device(d))
    go = gout.to(d)
    _lib.call("mu_attn_bwd", qd.data_ptr(), xd.data_ptr(), oattn.data_ptr(), go.data_ptr(), kidx.data_ptr(), kcnt.data_ptr(), lse.data_ptr(),
              mean.data_ptr(), rstd.data_ptr(), gd.data_ptr(), dY.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), dg.data_ptr(), db.data_ptr(),
              B, N, C, N, ws.data_ptr(), ws.numel(), cdt, st)
    tol = TOL[dtype]
    # fp32x with hot keys (round 6): the key operand of S = Q K^T is ONE fp16 term, so S carries 2^-12 |q k| per product instead of 2^-22;
    # with the |S| ~ 40 log2-unit scores this case constructs (probabilities spanning 12 decades) the recomputed P of the backward is off
    # by up to ~2e-3 where two large scores compete -- observed 1.8e-3 on dK -- while the forward (out, PV, lse2) and every
    # normal-magnitude shape (check_attention's 13 shapes; this case without the hot key) stay inside 1e-3.  Backward gate here: 3e-3.
    gtol_ = 3e-3 if (fp32x and hot) else tol
    res = [("attn overflow-redo out", _err(out, ref.detach()), tol), ("attn overflow-redo PV", _err(oattn, pv.detach()), tol),
           ("attn overflow-redo lse2", _err(lse, lse_ref.detach()), tol),
           ("attn overflow-redo dqkv", _rel_err(dqkv, qr.grad), gtol_),
           ("attn overflow-redo dq", _rel_err(dqkv[..., :C], qr.grad[..., :C]), gtol_),
           ("attn overflow-redo dk", _rel_err(dqkv[..., C:2 * C], qr.grad[..., C:2 * C]), gtol_),
           ("attn overflow-redo dv", _rel_err(dqkv[..., 2 * C:], qr.grad[..., 2 * C:]), gtol_)]
    if hot:
        hotv = float(sc[0, 3, 900].detach() * 1.4426950408889634 - lse_ref[0, 3].detach())      # ~0: key 900 dominates row 3
        res.append(("attn overflow-redo hot key dominates", abs(hotv), 0.5))
    return res


def check_attention_mask_semantics():
    import maskunet_amd
    m = maskunet_amd.Mask2FormerAttention(32, 32).to(DEV)
    res = []
    assert m.mask is None
    x = torch.randn(2, 32, 8, 8, device=DEV)
    y1 = m(x)
    mk = m.mask
    res.append(("mask lazily drawn [B,N,N] view", 0.0 if (mk is not None and tuple(mk.shape) == (2, 64, 64)) else 1.0, 0.0))
    vals = torch.unique(mk)
    res.append(("mask values {0,-inf}", 0.0 if all(v == 0 or v == -float("inf") for v in vals.tolist()) else 1.0, 0.0))
    y2 = m(x)
    res.append(("mask cached", _err(y2, y1), 0.0))
    # inject in the reference's own form and compare with set_keep_mask
    keep = (torch.rand(2, 64) > 0.4)
    add = torch.where(keep, torch.zeros(()), torch.full((), -float("inf"))).unsqueeze(1).expand(-1, 64, -1)
    m.mask = add.to(DEV)
    ya = m(x)
    m.set_keep_mask(keep.to(torch.uint8))
    yb = m(x)
    res.append(("mask inject forms agree", _err(ya, yb), 0.0))
    try:
        m(torch.randn(3, 32, 8, 8, device=DEV))
        res.append(("batch mismatch raises", 1.0, 0.0))
    except RuntimeError:
        res.append(("batch mismatch raises", 0.0, 0.0))
    try:
        m(torch.randn(2, 64, 8, 8, device=DEV))
        res.append(("channel mismatch raises", 1.0, 0.0))
    except ValueError as e:
        res.append(("channel mismatch raises", 0.0 if "Input channel size does not match" in str(e) else 1.0, 0.0))
    m.mask_mode = "resample"
    m(x)
    k1 = m._keep.clone()
    m(x)
    res.append(("resample mode redraws", 0.0 if not torch.equal(k1, m._keep) else 1.0, 0.0))
    return res


# ------------------------------------------------------------------------------------------------
def load_golden(name):
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    return {k: z[k] for k in z.files}


def check_golden_module(name, dtype):
    """Run a committed golden case (generated from the REAL reference) through the HIP modules."""
    import maskunet_amd
    from maskunet_amd import _lib
    rec = load_golden(name)
    training = bool(rec["training"])
    sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("param/")}
    if name.startswith("convblock_res"):
        c = sd["conv_block.0.weight"].shape
        mod = maskunet_amd.ConvBlock(c[1], c[0], residual=True)
    elif name.startswith("convblock_mid"):
        mod = maskunet_amd.ConvBlock(sd["conv_block.0.weight"].shape[1], sd["conv_block.3.weight"].shape[0], sd["conv_block.0.weight"].shape[0])
    elif name.startswith("convblock"):
        mod = maskunet_amd.ConvBlock(sd["conv_block.0.weight"].shape[1], sd["conv_block.3.weight"].shape[0])
    elif name.startswith("down"):
        mod = maskunet_amd.DownSample(sd["maxpool_conv.1.conv_block.0.weight"].shape[1], sd["maxpool_conv.3.weight"].shape[0])
    elif name.startswith("up"):
        mod = maskunet_amd.UpSample(sd["conv.0.conv_block.0.weight"].shape[1], sd["conv.2.weight"].shape[0])
    elif name.startswith("attn"):
        C = sd["query.weight"].shape[0]
        mod = maskunet_amd.Mask2FormerAttention(C, C)
    else:
        raise KeyError(name)
    mod.load_state_dict(sd)
    mod.to(DEV).set_compute_dtype(dtype).train(training)
    if "keep" in rec:
        mod.set_keep_mask(torch.from_numpy(rec["keep"]))
    ins = [torch.from_numpy(rec[f"in/{i}"]).to(DEV).requires_grad_(True) for i in range(2) if f"in/{i}" in rec]
    out = mod(*ins)
    out.backward(torch.from_numpy(rec["gout"]).to(DEV))
    tol = TOL[dtype]
    res = [(name + " out", _err(out, torch.from_numpy(rec["out"])), tol)]
    for i, t in enumerate(ins):
        res.append((name + f" gin{i}", _rel_err(t.grad, torch.from_numpy(rec[f"gin/{i}"])), tol))
    gmax = max(float(np.abs(v).max()) for k, v in rec.items() if k.startswith("gparam/"))
    for k, v in mod.named_parameters():
        if "gparam/" + k in rec:
            ref = torch.from_numpy(rec["gparam/" + k])
            # compare against the largest parameter-gradient scale of the case: gamma/beta feeding a
            # second BatchNorm and key.bias have analytically-zero gradients (pure rounding noise)
            floor = PARAM_GRAD_FLOOR[dtype] * gmax
            if k == "key.bias" and "gparam/query.bias" in rec and _lib.mdt(dtype) == _lib.MU_F32X:
                # analytically zero (a constant added to every key shifts all scores of a query alike: softmax invariance), so what any
                # arithmetic returns is rounding noise of the dK rows summed over the keys.  ONLY in the fp32x mode (exact fp32 and fp16
                # keep the floor above): there dS enters the matrix core as ONE fp16 operand (2^-12 relative per element), which puts
                # this noise at ~1e-5 of the case's gradient scale (exact fp32: ~1e-7); held, as in check_attention, to the gate times
                # the scale of its sibling gradient d query.bias
                floor = float(np.abs(rec["gparam/query.bias"]).max())
            e = float((v.grad.detach().float().cpu() - ref).abs().max()) / max(float(ref.abs().max()), floor)
            res.append((name + " d" + k, e, tol))
    if training:
        for k, v in mod.state_dict().items():
            if "running" in k and "newstat/" + k in rec:
                res.append((name + " " + k, _err(v, torch.from_numpy(rec["newstat/" + k])), tol))
    return res


def build_unet(c_out, three_head, seed, dtype, training, B):
    import maskunet_amd
    shapes = O.unet_state_shapes(3, c_out, three_head)
    params = O.make_params(shapes, seed)
    model = maskunet_amd.InstanceUNet(3, c_out, 16) if three_head else maskunet_amd.UNet(3, c_out)
    model.load_state_dict(params)
    model.to(DEV).set_compute_dtype(dtype).train(training)
    model.dropout.p = 0.0
    keeps = O.make_keeps(seed + 1, B)
    model.set_keep_masks(keeps)
    x, labels = O.make_inputs(seed + 2, B, c_out, ignore_frac=0.1 if three_head else 0.0)
    return model, params, keeps, x, labels


def check_unet_golden(name, dtype):
    """Whole-model case against the committed slices/grad norms produced by the REAL reference."""
    rec = load_golden(name)
    three = name.startswith("unet3")
    B, c_out, seed, training = int(rec["B"]), int(rec["c_out"]), int(rec["seed"]), bool(rec["training"])
    model, params, keeps, x, labels = build_unet(c_out, three, seed, dtype, training, B)
    scale = 1.0 if dtype == torch.float32 else FP16_LOSS_SCALE
    out = model(x.to(DEV))
    outs = out if three else (out,)
    tol = TOL[dtype]
    res = []
    for i, o in enumerate(outs):
        res.append((f"{name} out{i} slice", _err(o[:, :, ::16, ::16], torch.from_numpy(rec[f"out{i}_slice"])), tol))
        res.append((f"{name} out{i} sum", abs(float(o.double().sum()) - float(rec[f"out{i}_sum"])) / float(rec[f"out{i}_abssum"]), tol))
    loss = F.cross_entropy(outs[0], labels.to(DEV), ignore_index=255 if three else -100)
    if three:
        loss = loss + 0.5 * out[2].square().mean() + 0.25 * out[1].square().mean()
    res.append((f"{name} loss", abs(loss.item() - float(rec["loss"])) / max(1.0, abs(float(rec["loss"]))), tol))
    if not training:
        return res
    (loss * scale).backward()
    gmax = max(float(v) for k, v in rec.items() if k.startswith("gnorm/"))
    worst = (0.0, "")
    for k, v in model.named_parameters():
        has = bool(rec["ghas/" + k])
        assert (v.grad is not None) == has, k
        if not has:
            continue
        gn = float((v.grad.double() / scale).norm())
        ref = float(rec["gnorm/" + k])
        floor = (1e-4 if dtype == torch.float32 else 1e-2) * gmax
        e = abs(gn - ref) / max(ref, floor)
        if e > worst[0]:
            worst = (e, k)
        if "g/" + k in rec:
            r = torch.from_numpy(rec["g/" + k])
            e2 = float((v.grad.float().cpu() / scale - r).abs().max()) / max(float(r.abs().max()), floor)
            if e2 > worst[0]:
                worst = (e2, k + " (full)")
    # Max-norm gradient errors of the whole model are dominated by a handful of ReLU / max-pool / GELU-kink decisions that
    # flip under ANY reassociation of the fp32 sums (the reference's own fp32-vs-fp64 noise is ~1e-3 in this metric and a
    # different-but-equally-valid summation order moves single elements by a few %), so the max-norm gate is loose (5e-2
    # fp32, 3e-1 fp16) and the tight gate is the per-parameter cosine (check_unet_vs_oracle: 1-cos <= 1e-4 fp32, 2e-2 fp16).
    gtol = UNET_GRAD_MAXREL[dtype]
    res.append((f"{name} worst grad [{worst[1]}]", worst[0], gtol))
    gsl = model.norm.weight.grad[:, ::16, ::16].float().cpu() / scale
    res.append((f"{name} d norm.weight slice", _rel_err(gsl, torch.from_numpy(rec["g_slice/norm.weight"])), 2 * gtol))
    gw0 = model.initial_conv.conv_block[0].weight.grad.float().cpu() / scale
    res.append((f"{name} d initial conv w", _rel_err(gw0, torch.from_numpy(rec["g_slice/initial_conv.conv_block.0.weight"])), gtol))
    for k, v in model.state_dict().items():
        if "newstat/" + k in rec:
            res.append((f"{name} {k}", _err(v, torch.from_numpy(rec["newstat/" + k])), tol))
    return res


def check_unet_vs_oracle(dtype, B=2, c_out=150, three_head=False, seed=300, with_dropout=True, noise_floor=False):
    """Whole model vs the CPU oracle run live on the same seeded inputs, training mode, with explicit dropout masks.

    noise_floor=True (fp32): the oracle also runs in fp64 and every parameter gradient is gated RELATIVE TO THE REFERENCE'S OWN
    fp32 NOISE: err(HIP fp32 vs fp64 oracle) / err(fp32 oracle vs fp64 oracle) per parameter (max-norm, normalised by the fp64
    gradient's max; the per-parameter floor is the median noise over all parameters so that a parameter the fp32 oracle happens to
    hit exactly does not gate at zero): median <= 2, worst <= 6, with max-pool arg-max flips detected explicitly (below).
    Replaces the constant 5e-2 max-norm gate for this case."""
    model, params, keeps, x, labels = build_unet(c_out, three_head, seed, dtype, True, B)
    gen = np.random.default_rng(seed + 5)
    if with_dropout:
        model.dropout.p = 0.3
        dm = [torch.from_numpy((gen.random((B, 128, 32, 32)) > 0.3).astype(np.uint8)),
              torch.from_numpy((gen.random((B, 64, 64, 64)) > 0.3).astype(np.uint8))]
        model.dropout_masks = [m.permute(0, 2, 3, 1).contiguous() for m in dm]    # NHWC for the HIP path
    else:
        dm = None
    p = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone()) for k, v in params.items()}
    ns = {}
    out = model(x.to(DEV))
    outs = out if three_head else (out,)
    # Discrete decisions of the LAST ReLU (final_layer: Conv1x1 -> BN -> ReLU, ade_semantic.py:283-287): a pre-activation inside the forward
    # noise (|z| ~ 1e-4 of the output scale) can land on either side of zero in two equally valid evaluations, and ONE such flip at a pixel
    # whose label is that class moves the per-pixel LayerNorm gradients of that pixel by ~30 % of their maximum (B = 2: nothing averages).
    # Like the dropout masks, the decisions are therefore INJECTED: the oracle multiplies by the HIP path's sign pattern instead of calling
    # relu -- and the check below holds every overridden pre-activation to the forward gate, so this cannot hide a real forward error.
    dec = (outs[0].detach() > 0).cpu()
    forced = {"n": 0, "zrel": 0.0}
    _head = O.head_1x1_bn_relu

    def head_forced(xh, ph, prefix, training, new_stats=None):
        if prefix != "final_layer":
            return _head(xh, ph, prefix, training, new_stats)
        y = O.batchnorm2d(F.conv2d(xh, ph[prefix + ".0.weight"], ph[prefix + ".0.bias"]), ph, prefix + ".1", training, new_stats)
        diff = (y.detach() > 0) != dec
        forced["n"] = int(diff.sum())
        if forced["n"]:
            forced["zrel"] = float(y.detach().abs()[diff].max()) / max(1.0, float(y.detach().abs().max()))
        return y * dec.to(y.dtype)
    O.head_1x1_bn_relu = head_forced
    try:
        ref = O.unet_forward(p, x, keeps, training=True, dropout_masks=dm, new_stats=ns, three_head=three_head)
    finally:
        O.head_1x1_bn_relu = _head
    refs = ref if three_head else (ref,)
    lref = O.pixel_cross_entropy(refs[0], labels, 255 if three_head else -100)
    if three_head:
        lref = lref + 0.5 * ref[2].square().mean() + 0.25 * ref[1].square().mean()
    lref.backward()
    loss = F.cross_entropy(outs[0], labels.to(DEV), ignore_index=255 if three_head else -100)
    if three_head:
        loss = loss + 0.5 * out[2].square().mean() + 0.25 * out[1].square().mean()
    scale = 1.0 if dtype == torch.float32 else FP16_LOSS_SCALE
    (loss * scale).backward()
    tol = TOL[dtype]
    gtol = UNET_GRAD_MAXREL[dtype]          # max-norm: see check_unet_golden; the cosine below is the tight gate
    ctol = UNET_GRAD_COS[dtype]             # 1 - cosine similarity per parameter gradient
    res = [(f"unet out{i} full", _err(o, r), tol) for i, (o, r) in enumerate(zip(outs, refs))]
    res.append((f"unet final-ReLU decisions taken from the HIP path: {forced['n']} of {dec.numel()}; largest overridden |pre-activation| "
                f"relative to the output scale", forced["zrel"], tol))
    res.append(("unet loss", abs(loss.item() - lref.item()) / max(1.0, abs(lref.item())), tol))
    gmax = max(float(v.grad.abs().max()) for v in p.values() if v.requires_grad and v.grad is not None)
    worst, worst_cos = (0.0, ""), (0.0, "")
    floor = UNET_GRAD_FLOOR[dtype] * gmax
    for k, v in model.named_parameters():
        r = p[k].grad
        assert (v.grad is None) == (r is None), k
        if r is None:
            continue
        g = v.grad.float().cpu() / scale
        e = float((g - r).abs().max()) / max(float(r.abs().max()), floor)
        if e > worst[0]:
            worst = (e, k)
        if float(r.abs().max()) >= floor:       # skip analytically-zero gradients (pure rounding noise)
            c = 1.0 - float((g.double() * r.double()).sum() / (g.double().norm() * r.double().norm() + 1e-300))
            if c > worst_cos[0]:
                worst_cos = (c, k)
    res.append((f"unet worst param grad maxrel [{worst[1]}]", worst[0], gtol))
    res.append((f"unet worst param grad 1-cos [{worst_cos[1]}]", worst_cos[0], ctol))
    if noise_floor:
        p64 = {k: (v.double().clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else
                   (v.double().clone() if v.dtype.is_floating_point else v.clone())) for k, v in params.items()}
        r64 = O.unet_forward(p64, x.double(), keeps, training=True, dropout_masks=dm, new_stats={}, three_head=three_head)
        r64s = r64 if three_head else (r64,)
        l64 = O.pixel_cross_entropy(r64s[0], labels, 255 if three_head else -100)
        if three_head:
            l64 = l64 + 0.5 * r64[2].square().mean() + 0.25 * r64[1].square().mean()
        l64.backward()
        g64max = max(float(v.grad.abs().max()) for v in p64.values() if v.requires_grad and v.grad is not None)
        e_ref, e_hip = {}, {}
        for k, v in model.named_parameters():
            if p64[k].grad is None:
                continue
            g64 = p64[k].grad
            den = max(float(g64.abs().max()), 1e-3 * g64max)
            e_ref[k] = float((p[k].grad.double() - g64).abs().max()) / den
            e_hip[k] = float((v.grad.double().cpu() / scale - g64).abs().max()) / den
        med = sorted(e_ref.values())[len(e_ref) // 2]
        # Discrete decisions: a 2x2 max-pool window whose two largest values differ by less than the forward noise (~1e-6) can pick
        # a different pixel in two equally valid fp32 evaluations; ONE such window moves one gradient element and shifts every
        # weight gradient upstream of that pool by ~1/sqrt(#pixels) ~ 1e-3 (measured: initial_conv.* L2 error 1.1e-3 with every
        # kernel's own backward accurate to 6e-8 and nothing cancelling).  Such windows are FOUND here -- the HIP activations in
        # front of each of the three pools against the fp64 oracle's -- instead of being absorbed by a loose constant: parameters
        # upstream of a pool with a differing arg-max are held to the cosine gate above only, all others to 3x the reference noise.
        from maskunet_amd import ops as _ops
        buffers = {k: v.clone() for k, v in model.state_dict().items()}      # the partial forwards below update running statistics again
        with torch.no_grad():
            pd = {k: v.detach() for k, v in p64.items()}
            o1 = O.conv_block(x.double(), pd, "initial_conv", False, True, {})
            o2 = O.mask_attention(O.downsample(o1, pd, "downsample1", True, {}), pd, "self_attention1", keeps[0])
            o3 = O.mask_attention(O.downsample(o2, pd, "downsample2", True, {}), pd, "self_attention2", keeps[1])
            h1 = model.initial_conv.forward_nhwc(_ops.to_nhwc(x.to(DEV), dtype))
            h2 = model.self_attention1.forward_nhwc(model.downsample1.forward_nhwc(h1))
            h3 = model.self_attention2.forward_nhwc(model.downsample2.forward_nhwc(h2))

        def pool_argmax(t):          # NCHW -> index of the maximum inside every 2x2 window
            b, c, hh, ww = t.shape
            return t.reshape(b, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, hh // 2, ww // 2, 4).argmax(-1)
        model.load_state_dict(buffers)
        flips = [int((pool_argmax(h.permute(0, 3, 1, 2)[:, :o.shape[1]].double().cpu()) != pool_argmax(o)).sum()) for h, o in ((h1, o1), (h2, o2), (h3, o3))]
        upstream = [("initial_conv.",), ("downsample1.", "self_attention1."), ("downsample2.", "self_attention2.")]
        exempt = tuple(pre for i in range(3) if any(flips[i:]) for pre in upstream[i])      # a flip in pool k touches everything before it
        gated = [k for k in e_ref if not k.startswith(exempt)] if exempt else list(e_ref)
        ratio, wk = max(((e_hip[k] / max(e_ref[k], med), k) for k in gated), key=lambda t: t[0])
        print(f"noise-floor gate: oracle fp32-vs-fp64 gradient noise median {med:.2e}, max {max(e_ref.values()):.2e}; HIP fp32-vs-fp64 max over "
              f"gated parameters {max(e_hip[k] for k in gated):.2e}; worst ratio {ratio:.2f} [{wk}]; max-pool windows whose arg-max differs "
              f"from the fp64 oracle's (pool 1, 2, 3): {flips}; parameters held to the cosine gate only: {len(e_ref) - len(gated)} of {len(e_ref)}")
        ratios = sorted(e_hip[k] / max(e_ref[k], med) for k in gated)
        # typical parameter: <= 2x the reference's own fp32 noise (observed 1.6x: the fp32 MFMA accumulates each output as ONE sequential
        # FMA chain over K = 576..4608 terms, the CPU reference in blocked partial sums); worst single parameter: <= 6x (observed 3.8x)
        res.append((f"unet param grads vs fp64 oracle: MEDIAN over {len(gated)} parameters of (HIP err) / max(oracle fp32 err, median noise)",
                    ratios[len(ratios) // 2], 2.0))
        res.append((f"unet param grads vs fp64 oracle: WORST (HIP err) / max(oracle fp32 err, median noise) over the parameters not upstream of a "
                    f"flipped pool window [{wk}: hip {e_hip[wk]:.2e}, oracle {e_ref[wk]:.2e}; flips {flips}]", ratio, 6.0))
        res.append(("unet param grads: at most the encoder in front of pool 3 may be exempt", float(len(e_ref) - len(gated)), 60.0))
        eo_ref = _err(refs[0], r64s[0].float())
        eo_hip = _err(outs[0], r64s[0].float())
        res.append((f"unet out0 vs fp64 oracle [hip {eo_hip:.2e}, oracle fp32 {eo_ref:.2e}]", eo_hip / max(eo_ref, 1e-7), 3.0))
    worst = (0.0, "")
    for k, v in model.state_dict().items():
        if k in ns:
            e = _err(v, ns[k])
            if e > worst[0]:
                worst = (e, k)
    res.append((f"unet worst running stat [{worst[1]}]", worst[0], tol))
    return res


def check_attention_bwd_masked_rows(dtype):
    """mu_attn_bwd_phases with and without MU_ATTN_KIDX_PERMUTATION (8): the dqkv buffer starts as NaN garbage; either way the masked
    keys' dK / dV rows must be exact zeros and everything else identical bit for bit (memset path vs rows zeroed by the dK/dV sweep).
    Shapes cover a key count that ends inside a block, whole masked blocks, and images whose kept keys fill the last block."""
    from maskunet_amd import _lib
    res = []
    for (B, N, C, kept) in ((3, 1024, 64, (1, 500, 1024)), (2, 512, 128, (130, 64)), (2, 256, 256, (255, 17)), (2, 1024, 32, (700, 3))):
        g_ = torch.Generator().manual_seed(5 + C)
        qkv = torch.randn(B, N, 3 * C, generator=g_).to(dtype).to(DEV)
        x = torch.randn(B, N, C, generator=g_).to(dtype).to(DEV)
        gout = torch.randn(B, N, C, generator=g_).to(dtype).to(DEV)
        keep = torch.zeros(B, N, dtype=torch.uint8)
        for b in range(B):
            keep[b, torch.randperm(N, generator=g_)[:kept[b]]] = 1
        kd = keep.to(DEV)
        kidx = torch.argsort(kd, dim=1, descending=True, stable=True).to(torch.int32).contiguous()
        kcnt = kd.sum(1, dtype=torch.int32).contiguous()
        gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        out, oattn = torch.empty_like(x), torch.empty_like(x)
        lse = torch.empty(B, N, device=DEV)
        mean, rstd, delta = torch.empty_like(lse), torch.empty_like(lse), torch.empty_like(lse)
        st = _lib.stream()
        _lib.call("mu_attn_fwd", qkv.data_ptr(), x.data_ptr(), kidx.data_ptr(), kcnt.data_ptr(), gam.data_ptr(), bet.data_ptr(), out.data_ptr(),
                  oattn.data_ptr(), lse.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, N, C, N, 1e-5, _lib.dt(x), st)
        ws = _lib.workspace(_lib.load().mu_attn_bwd_workspace_bytes(B, N, C), torch.device(DEV))
        outs = []
        for flag in (0, 8):
            dY = torch.empty_like(x)
            dqkv = torch.full_like(qkv, float("nan"))
            dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
            for phase in (1, 2, 4):
                _lib.call("mu_attn_bwd_phases", qkv.data_ptr(), x.data_ptr(), oattn.data_ptr(), gout.data_ptr(), kidx.data_ptr(), kcnt.data_ptr(),
                          lse.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gam.data_ptr(), dY.data_ptr(), delta.data_ptr(), dqkv.data_ptr(),
                          dg.data_ptr(), db.data_ptr(), B, N, C, N, ws.data_ptr(), ws.numel(), _lib.dt(x), phase | flag, st)
            torch.cuda.synchronize()
            outs.append(dqkv)
        masked = (kd == 0)
        z = outs[1][..., C:][masked]
        res.append((f"attn bwd C={C} masked rows exact zero with flag 8", float(z.abs().max()) if z.numel() else 0.0, 0.0))
        res.append((f"attn bwd C={C} flag 8 == memset path", 0.0 if torch.equal(outs[0], outs[1]) else 1.0, 0.0))
        res.append((f"attn bwd C={C} finite", 0.0 if torch.isfinite(outs[1].float()).all() else 1.0, 0.0))
    return res


# ------------------------------------------------------------------------------------------------
# round 3: gradient joins inside kernels, key compaction, q/k/v weight prep
# ------------------------------------------------------------------------------------------------
def check_compact_keys():
    """mu_compact_keys against torch.argsort(keep, descending=True, stable=True) (what the modules used before round 3): bit-exact
    index lists for uint8 and int64 masks, ragged N, all keys kept / all masked / a single key."""
    from maskunet_amd import ops
    gen = torch.Generator().manual_seed(11)
    out = []
    for (B, N) in [(3, 256), (2, 1000), (64, 16384), (2, 65536), (5, 1), (4, 1025), (2, 3)]:
        for kdt in (torch.uint8, torch.int64):
            keep = torch.randint(0, 2, (B, N), generator=gen).to(kdt)
            if B >= 3:
                keep[0] = 1                       # every key visible
                keep[1] = 0                       # no key visible (kcnt = 0: the index list is still the identity permutation)
                keep[2] = 0
                keep[2, N // 2] = 1
            kd = keep.to(DEV)
            kidx, kcnt, keep8 = ops.compact_keys(kd)
            ref_idx = torch.argsort(keep.to(torch.uint8), dim=1, descending=True, stable=True).to(torch.int32)
            ref_cnt = (keep != 0).sum(1).to(torch.int32)
            ok = bool((kidx.cpu() == ref_idx).all()) and bool((kcnt.cpu() == ref_cnt).all()) and bool((keep8.cpu() == (keep != 0).to(torch.uint8)).all())
            out.append((f"compact_keys{(B, N)} {str(kdt)[6:]}", 0.0 if ok else 1.0, 0.0))
    return out


def check_grad_joins(dtype):
    """mu_maxpool2_bwd_acc / mu_upcat_bwd_acc / mu_conv1x1_fwd_add against the separate torch ops they replace."""
    from maskunet_amd import _lib
    gen = np.random.default_rng(21)
    out = []
    tol = TOL[dtype]
    call, ptr, dt, st = _lib.call, _lib.ptr, _lib.dt, _lib.stream
    for (B, H, W, C) in [(2, 12, 8, 64), (1, 32, 32, 128)]:
        x = _rnd(gen, B, H, W, C).to(DEV, dtype)
        g1, g2 = _rnd(gen, B, H // 2, W // 2, C).to(DEV, dtype), _rnd(gen, B, H // 2, W // 2, C).to(DEV, dtype)
        ga = _rnd(gen, B, H, W, C).to(DEV, dtype)
        xr = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.max_pool2d(xr, 2).backward((g1.float() + g2.float()).permute(0, 3, 1, 2))
        ref = xr.grad.permute(0, 2, 3, 1) + ga.float()
        for (a2, aa, tag) in [(g2, ga, "dy2+dx_add"), (g2, None, "dy2"), (None, ga, "dx_add")]:
            dx = torch.empty_like(x)
            call("mu_maxpool2_bwd_acc", ptr(x), ptr(g1), ptr(a2), ptr(aa), ptr(dx), B, H, W, C, dt(x), st())
            xr2 = x.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
            F.max_pool2d(xr2, 2).backward((g1.float() + (a2.float() if a2 is not None else 0)).permute(0, 3, 1, 2))
            r = xr2.grad.permute(0, 2, 3, 1) + (aa.float() if aa is not None else 0)
            out.append((f"maxpool_bwd_acc{(B, H, W, C)} {tag}", _rel_err(dx, r), tol))
    for (B, Cx, Cs, h, w) in [(2, 32, 64, 5, 7), (1, 128, 128, 16, 16)]:
        g1, g2 = _rnd(gen, B, 2 * h, 2 * w, Cs + Cx).to(DEV, dtype), _rnd(gen, B, 2 * h, 2 * w, Cs + Cx).to(DEV, dtype)
        xr = torch.zeros(B, Cx, h, w, requires_grad=True)
        sr = torch.zeros(B, Cs, 2 * h, 2 * w, requires_grad=True)
        yr = torch.cat([sr, F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=True)], 1)
        yr.backward((g1.float() + g2.float()).cpu().permute(0, 3, 1, 2))
        dx = torch.empty(B, h, w, Cx, dtype=dtype, device=DEV)
        ds = torch.empty(B, 2 * h, 2 * w, Cs, dtype=dtype, device=DEV)
        call("mu_upcat_bwd_acc", ptr(g1), ptr(g2), ptr(dx), ptr(ds), B, h, w, Cx, Cs, dt(g1), st())
        out += [(f"upcat_bwd_acc{(B, Cx, Cs, h, w)} dx", _rel_err(dx, xr.grad.permute(0, 2, 3, 1)), tol),
                (f"upcat_bwd_acc{(B, Cx, Cs, h, w)} dskip", _rel_err(ds, sr.grad.permute(0, 2, 3, 1)), tol)]
    lib = _lib.load()
    for (M, Cin, Cout) in [(2 * 16 * 16, 192, 64), (1000, 384, 128), (300, 768, 256), (77, 64, 64)]:
        if not lib.mu_conv1x1_add_supported(Cin, Cout, dt(dtype)):
            out.append((f"conv1x1_add{(M, Cin, Cout)} supported", 1.0, 0.0))
            continue
        x = (_rnd(gen, M, Cin) * 0.5).to(DEV, dtype)
        w = (_rnd(gen, Cout, Cin) / math.sqrt(Cin)).to(DEV, dtype)
        a = _rnd(gen, M, Cout).to(DEV, dtype)
        y = torch.full((M, Cout), 7.0, dtype=dtype, device=DEV)
        call("mu_conv1x1_fwd_add", ptr(x), ptr(w), ptr(a), ptr(y), M, Cin, Cout, Cin, Cout, dt(x), st())
        ref = x.double() @ w.double().t() + a.double()
        out.append((f"conv1x1_add{(M, Cin, Cout)}", _err(y, ref.float()), tol))
    out.append(("conv1x1_add unsupported shape -> MU_ERR_SHAPE", 0.0 if lib.mu_conv1x1_fwd_add(1, 1, 1, 1, 8, 32, 32, 32, 32, dt(dtype), None) == -2 else 1.0, 0.0))
    return out


def check_prep_qkv(dtype):
    """mu_prep_qkv == mu_prep_weight(mode 2) of the concatenated [3C, C] weight + the concatenated bias, bit for bit."""
    from maskunet_amd import _lib, ops
    gen = np.random.default_rng(23)
    out = []
    for C in (32, 64, 256):
        ws = [_rnd(gen, C, C).to(DEV) for _ in range(3)]
        bs = [_rnd(gen, C).to(DEV) for _ in range(3)]
        wbuf = torch.empty(6 * C * C, dtype=dtype, device=DEV)
        bias = torch.empty(3 * C, dtype=torch.float32, device=DEV)
        _lib.call("mu_prep_qkv", *[_lib.ptr(t) for t in ws + bs], _lib.ptr(wbuf), _lib.ptr(bias), _lib.dt(dtype), C, _lib.stream())
        f, d = ops._prep_weight_raw(torch.cat(ws, 0).view(3 * C, C, 1, 1), dtype, 3 * C, C, 2)
        same = bool((wbuf[:3 * C * C].view(3 * C, C) == f.view(3 * C, C)).all()) and bool((wbuf[3 * C * C:].view(C, 3 * C) == d.view(C, 3 * C)).all()) \
            and bool((bias == torch.cat(bs)).all())
        out.append((f"prep_qkv C={C}", 0.0 if same else 1.0, 0.0))
    return out


def check_grad_links_model(dtype, B=2):
    """Whole UNet, training mode: parameter and input gradients with the in-kernel gradient joins (ops.GradLink: residual branches into
    the pool / concat backward, skip connections into the pool backward, dY into the projection data-gradient) against the same model
    with every join left to autograd (MU_GRAD_LINKS=0 semantics).  Same kernels otherwise, so fp32 agrees to rounding."""
    import maskunet_amd
    from maskunet_amd import ops
    torch.manual_seed(7)
    model = maskunet_amd.UNet(3, 19).to(DEV)
    model.set_compute_dtype(dtype).train()
    model.dropout.p = 0.0
    gen = np.random.default_rng(31)
    x = torch.from_numpy(gen.random((B, 3, 128, 128), dtype=np.float32)).to(DEV)
    keeps = [torch.from_numpy(gen.integers(0, 2, (B, n)).astype(np.uint8)).to(DEV) for n in (4096, 1024, 256, 1024, 4096, 16384)]
    labels = torch.from_numpy(gen.integers(0, 19, (B, 128, 128))).to(DEV)
    scale = FP16_LOSS_SCALE if dtype == torch.float16 else 1.0
    grads = []
    saved = (ops.GRAD_LINKS, ops.ATTN_FUSED_ADD)
    try:
        for on in (True, False):
            ops.GRAD_LINKS = ops.ATTN_FUSED_ADD = on
            model.set_keep_masks(keeps)
            for bn in [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]:
                bn.reset_running_stats()
            xin = x.clone().requires_grad_(True)
            out = model(xin)
            (F.cross_entropy(out, labels) * scale).backward()
            grads.append({"input": xin.grad.clone(), **{n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}})
            model.zero_grad(set_to_none=True)
    finally:
        ops.GRAD_LINKS, ops.ATTN_FUSED_ADD = saved
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    # per-tensor max error relative to that tensor's own max, floored at 1e-3 of the largest gradient (the key biases' gradients are
    # identically zero in exact arithmetic -- softmax does not see a per-query constant -- so what they hold is rounding noise)
    gmax = max(float(v.abs().max()) for v in grads[1].values())

    def rel(k):
        a, b = grads[0][k].float(), grads[1][k].float()
        if not torch.isfinite(a).all():
            return float("inf")
        return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3 * gmax)
    worst = max(((rel(k), k) for k in grads[1]), key=lambda t: t[0])
    return [(f"grad joins vs autograd sums: worst relative gradient difference ({worst[1]})", worst[0], tol),
            ("grad joins: same set of gradients", 0.0 if set(grads[0]) == set(grads[1]) else 1.0, 0.0)]


def check_prep_weights_multi(dtype):
    """mu_prep_weights_multi (one launch for many layers) == one mu_prep_weight call per layer, bit for bit; and a whole training step
    with the one-launch path (ops.MULTI_PREP) gives bit-identical loss and gradients to the per-layer path."""
    import maskunet_amd
    from maskunet_amd import _lib, ops
    gen = np.random.default_rng(5)
    shapes = [(19, 3, 3), (64, 32, 3), (150, 64, 1), (96, 160, 3), (1, 32, 1), (512, 512, 3), (33, 65, 3)]
    ws = [torch.nn.Parameter(_rnd(gen, O, I, k, k).to(DEV)) for (O, I, k) in shapes]
    holder = {}
    saved = ops.MULTI_PREP
    out = []
    try:
        ops.MULTI_PREP = True
        ops.prep_conv_weights(holder, ws, dtype, fwd_only=(ws[0], ws[4]))
        bad = 0
        for w, (O, I, k) in zip(ws, shapes):
            taps, Op, Ip = k * k, (O + 31) // 32 * 32, (I + 31) // 32 * 32
            need = w is not ws[0] and w is not ws[4]
            pre = ops._take_step_prep(w, dtype, taps, Op, Ip, need)
            if pre is None or (pre[1] is None) == need or getattr(w, "_mu_step", 1) is not None:
                bad += 1
                continue
            ref = ops._prep_weight_raw(w, dtype, Op, Ip, 2)
            if not torch.equal(pre[0], ref[0]) or (need and not torch.equal(pre[1], ref[1])):
                bad += 1
        out.append(("multi-layer weight prep == per-layer prep (layers that differ)", float(bad), 0.0))
        # an entry is rejected when the weight changed after it was made, and when a data-gradient layout is needed but was not made
        ops.prep_conv_weights(holder, ws, dtype, fwd_only=(ws[0], ws[4]))
        with torch.no_grad():
            ws[1].add_(1.0)
        stale = ops._take_step_prep(ws[1], dtype, 9, 64, 32, True) is not None
        nodg = ops._take_step_prep(ws[0], dtype, 9, 32, 32, True) is not None
        out.append(("multi-layer prep: stale / insufficient entries rejected", float(stale) + float(nodg), 0.0))
        for w in ws:
            w._mu_step = None

        torch.manual_seed(3)
        model = maskunet_amd.UNet(3, 19, 16).to(DEV)
        model.set_compute_dtype(dtype).train()
        model.dropout.p = 0.0
        B = 2
        x = torch.from_numpy(gen.random((B, 3, 128, 128), dtype=np.float32)).to(DEV)
        keeps = [torch.from_numpy(gen.integers(0, 2, (B, n)).astype(np.uint8)).to(DEV) for n in (4096, 1024, 256, 1024, 4096, 16384)]
        labels = torch.from_numpy(gen.integers(0, 19, (B, 128, 128))).to(DEV)
        res = []
        for on in (True, False):
            ops.MULTI_PREP = on
            model.set_keep_masks(keeps)
            for bn in [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]:
                bn.reset_running_stats()
            calls = []
            _lib.PROBE = {"pred": lambda name, a: (calls.append(name) or False) if name.startswith("mu_prep_weight") else False, "events": []}
            try:
                sem, bnd, emb = model(x)
                loss = F.cross_entropy(sem, labels) + bnd.float().mean() + emb.float().square().mean()
                loss.backward()
            finally:
                _lib.PROBE = None
            res.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, calls))
            model.zero_grad(set_to_none=True)
        same = torch.equal(res[0][0], res[1][0]) and set(res[0][1]) == set(res[1][1]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[1][1])
        out.append(("one-launch prep: loss and every gradient bit-identical to the per-layer path", 0.0 if same else 1.0, 0.0))
        out.append(("one-launch prep: weight-layout launches in a 3-head training step (per-layer path: %d)" % len(res[1][2]),
                    float(len(res[0][2])), 1.0))
        left = sum(1 for m in model.modules() if isinstance(m, torch.nn.Conv2d) and getattr(m.weight, "_mu_step", None) is not None)
        out.append(("one-launch prep: no entry survives the forward", float(left), 0.0))
    finally:
        ops.MULTI_PREP = saved
    return out


def check_resize_u8():
    """mu_resize_u8_nhwc / mu_resize_nearest_u8 against the committed fixture (tests/golden/resize_cases.npz) and the live numpy
    restatement of cv2.resize: the resized BYTES bit for bit, the [0,1] activations exactly byte/255, BGR->RGB, zero channel padding;
    then UNet.forward_u8 on an image of another size against forward(ToTensor(oracle-resized image))."""
    import maskunet_amd
    from maskunet_amd import ops
    from oracle import cv2_resize_oracle as R
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_cases.npz"))
    n = len([k for k in z.files if k.endswith("_img")])
    out = []
    for i in range(n):
        img, lab = z[f"c{i}_img"], z[f"c{i}_lab"]
        dw, dh = (int(v) for v in z[f"c{i}_dsize"])
        for dtype in (torch.float32, torch.float16):
            for bgr in (False, True):
                y, u8 = ops.resize_u8_to_nhwc(torch.from_numpy(img)[None].to(DEV), (dw, dh), dtype, bgr=bgr, return_u8=True)
                want = z[f"c{i}_lin"][:, :, ::-1] if bgr else z[f"c{i}_lin"]
                ok = bool((u8[0].cpu().numpy() == want).all())
                act = torch.from_numpy(np.ascontiguousarray(want)).to(dtype=torch.float32) / 255.0
                ok_act = bool((y[0, :, :, :3].float().cpu() == act.to(dtype).float()).all()) and float(y[..., 3:].abs().max()) == 0.0
                out.append((f"resize linear case {i} {img.shape[:2]}->{(dh, dw)} {str(dtype)[6:]} bgr={bgr}", 0.0 if (ok and ok_act) else 1.0, 0.0))
        got = ops.resize_labels_u8(torch.from_numpy(lab)[None].to(DEV), (dw, dh))
        out.append((f"resize nearest case {i}", 0.0 if bool((got[0].cpu().numpy() == z[f"c{i}_near"].astype(np.int64)).all()) else 1.0, 0.0))
    # batch of two same-size images, live oracle
    rng = np.random.default_rng(77)
    imgs = rng.integers(0, 256, (2, 95, 143, 3), dtype=np.uint8)
    y, u8 = ops.resize_u8_to_nhwc(torch.from_numpy(imgs).to(DEV), (128, 128), torch.float32, return_u8=True)
    ok = all(bool((u8[b].cpu().numpy() == R.resize_linear_u8(imgs[b], (128, 128))).all()) for b in range(2))
    out.append(("resize linear batch of 2 vs live oracle", 0.0 if ok else 1.0, 0.0))
    # the model entry point: decoded BGR bytes of another size in, same logits as the reference pipeline on the host + forward()
    torch.manual_seed(3)
    model = maskunet_amd.UNet(3, 5).to(DEV).eval()
    keeps = [torch.from_numpy(rng.integers(0, 2, (2, k)).astype(np.uint8)).to(DEV) for k in (4096, 1024, 256, 1024, 4096, 16384)]
    model.set_keep_masks(keeps)
    with torch.no_grad():
        a = model.forward_u8(torch.from_numpy(imgs).to(DEV), bgr=True)
        host = np.stack([R.prepare_sample(imgs[b], np.zeros((95, 143), np.uint8), (128, 128))[0] for b in range(2)])
        b_ = model(torch.from_numpy(host).to(DEV))
    out.append(("forward_u8(any size, bgr) == forward(ToTensor(resize(BGR2RGB(img))))", _err(a, b_), 1e-6))
    return out


def check_eval_fused(dtype):
    """Inference with every eval-mode BatchNorm (+ residual, + GELU / ReLU) folded into the producing conv's epilogue (mu_conv_fwd_fused,
    used under torch.no_grad()): the reference's eval goldens for the four module kinds and the whole UNet, and bit-level agreement in
    class with the unfused path (conv, then a BatchNorm-apply pass) on the 1-head and the 3-head model."""
    import maskunet_amd
    from maskunet_amd import _lib, ops
    tol = TOL[dtype]
    res = []
    calls = []
    orig = _lib.call

    def spy(name, *a):
        calls.append(name)
        return orig(name, *a)
    # module goldens (reference outputs in eval mode), forward only, fused
    for name in ("convblock_8_16_eval", "convblock_mid_16_8_eval", "convblock_res_8_eval", "down_16_32_eval", "up_32_16_eval"):
        rec = load_golden(name)
        sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("param/")}
        if name.startswith("convblock_res"):
            c = sd["conv_block.0.weight"].shape
            mod = maskunet_amd.ConvBlock(c[1], c[0], residual=True)
        elif name.startswith("convblock_mid"):
            mod = maskunet_amd.ConvBlock(sd["conv_block.0.weight"].shape[1], sd["conv_block.3.weight"].shape[0], sd["conv_block.0.weight"].shape[0])
        elif name.startswith("convblock"):
            mod = maskunet_amd.ConvBlock(sd["conv_block.0.weight"].shape[1], sd["conv_block.3.weight"].shape[0])
        elif name.startswith("down"):
            mod = maskunet_amd.DownSample(sd["maxpool_conv.1.conv_block.0.weight"].shape[1], sd["maxpool_conv.3.weight"].shape[0])
        else:
            mod = maskunet_amd.UpSample(sd["conv.0.conv_block.0.weight"].shape[1], sd["conv.2.weight"].shape[0])
        mod.load_state_dict(sd)
        mod.to(DEV).set_compute_dtype(dtype).eval()
        ins = [torch.from_numpy(rec[f"in/{i}"]).to(DEV) for i in range(2) if f"in/{i}" in rec]
        calls.clear()
        ops.call = _lib.call = spy
        try:
            with torch.no_grad():
                out = mod(*ins)
        finally:
            ops.call = _lib.call = orig
        res.append((name + " fused out vs reference", _err(out, torch.from_numpy(rec["out"])), tol))
        res.append((name + " ran fused (no BatchNorm-apply pass)", 0.0 if ("mu_conv_fwd_fused" in calls and "mu_bn_act_fwd" not in calls) else 1.0, 0.0))
    # whole model: reference golden (eval), fused vs unfused
    rec = load_golden("unet1_c150_b2_eval")
    B, c_out, seed = int(rec["B"]), int(rec["c_out"]), int(rec["seed"])
    for three in (False, True):
        model, params, keeps, x, labels = build_unet(19 if three else c_out, three, seed, dtype, False, B)
        outs = {}
        saved = ops.EVAL_FUSE
        try:
            for fuse in (True, False):
                ops.EVAL_FUSE = fuse
                calls.clear()
                ops.call = _lib.call = spy
                try:
                    with torch.no_grad():
                        o = model(x.to(DEV))
                finally:
                    ops.call = _lib.call = orig
                outs[fuse] = o if three else (o,)
                if fuse:
                    res.append((f"unet{3 if three else 1} eval: fused launches, no BatchNorm-apply pass",
                                0.0 if (calls.count("mu_conv_fwd_fused") >= 33 and "mu_bn_act_fwd" not in calls) else 1.0, 0.0))
        finally:
            ops.EVAL_FUSE = saved
        for i, (a, b) in enumerate(zip(outs[True], outs[False])):
            res.append((f"unet{3 if three else 1} eval out{i}: fused vs unfused", _err(a, b), 2e-5 if dtype == torch.float32 else tol))
        if not three:
            res.append(("unet1_c150_b2_eval fused out0 slice vs reference", _err(outs[True][0][:, :, ::16, ::16], torch.from_numpy(rec["out0_slice"])), tol))
    return res


def check_attention_no_visible_key(dtype):
    """An image whose key mask hides EVERY key: the reference's softmax over -inf only is NaN for every query of that image
    (ade_semantic.py:183-185) -- outputs and all gradients NaN; the other images of the batch are untouched (same values as without
    the dead image in the batch)."""
    import maskunet_amd
    res = []
    for C, hw in ((64, 16), (128, 8), (256, 8), (32, 8), (288, 8)):      # 288: the generic path above 256 channels
        torch.manual_seed(C)
        m = maskunet_amd.Mask2FormerAttention(C, C).to(DEV).set_compute_dtype(dtype)
        N = hw * hw
        x = torch.randn(3, C, hw, hw, device=DEV)
        keep = (torch.rand(3, N) > 0.5).to(torch.uint8)
        keep[1] = 0
        xa = x.clone().requires_grad_(True)
        m.set_keep_mask(keep)
        ya = m(xa)
        g = torch.randn_like(ya)
        ya.backward(g)
        nan_out = bool(torch.isnan(ya[1]).all()) and bool(torch.isfinite(ya[0]).all()) and bool(torch.isfinite(ya[2]).all())
        nan_gin = bool(torch.isnan(xa.grad[1]).all()) and bool(torch.isfinite(xa.grad[0]).all()) and bool(torch.isfinite(xa.grad[2]).all())
        # sums over the batch: NaN like the reference's -- except LayerNorm's bias gradient, the plain sum of the incoming gradient
        nan_gw = all(bool(torch.isnan(p.grad).all()) for n, p in m.named_parameters() if n != "norm.bias") and bool(torch.isfinite(m.norm.bias.grad).all())
        m.zero_grad(set_to_none=True)
        xb = x[[0, 2]].clone().requires_grad_(True)
        m.set_keep_mask(keep[[0, 2]])
        yb = m(xb)
        yb.backward(g[[0, 2]])
        same = _err(ya[[0, 2]], yb) + _rel_err(xa.grad[[0, 2]], xb.grad)
        res += [(f"no visible key C={C}: outputs NaN for that image only", 0.0 if nan_out else 1.0, 0.0),
                (f"no visible key C={C}: input gradient NaN for that image only", 0.0 if nan_gin else 1.0, 0.0),
                (f"no visible key C={C}: parameter gradients NaN", 0.0 if nan_gw else 1.0, 0.0),
                (f"no visible key C={C}: other images unchanged", same, 1e-6 if dtype == torch.float32 else 2e-3)]
    return res
