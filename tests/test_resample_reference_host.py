"""tests/_resample_reference.py against torch in float64 on the CPU: the max-pool's values and gradient routing (ties, NaN, -inf, signed
zeros, odd sizes), the bilinear x2 + concat and its transpose.  The numpy restatement of the interpolation keeps the kernels' fp32 source
index, which is not what torch's own fp32 CPU kernel does, so the float64 result within a bound that grows with the axis is the check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _resample_reference as R


def _nchw64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _same_values(a, b):
    """equal as values, NaN positions included; -0 equals +0"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


POOL_SHAPES = [(1, 2, 2, 8), (2, 3, 2, 8), (2, 2, 3, 8), (2, 7, 5, 32), (1, 13, 8, 16), (2, 12, 9, 40), (1, 7, 9, 8)]


@pytest.mark.parametrize("npdt", [np.float32, np.float16])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_values_and_gradient_routing(shape, npdt):
    B, H, W, C = shape
    gen = np.random.default_rng(H * 100 + W)
    x = gen.integers(-1, 2, shape).astype(npdt)                # ties everywhere
    if shape == (1, 7, 9, 8):
        R.plant_special_windows(x)
    # gradients in multiples of 1/8 below 8: every sum is exact in fp16, so torch's float64 sum is the same number
    g = [(gen.integers(-20, 21, s) / 8.0).astype(npdt) for s in ((B, H // 2, W // 2, C), (B, H // 2, W // 2, C), shape)]
    xt = _nchw64(x).requires_grad_(True)
    yt = F.max_pool2d(xt, 2)
    assert _same_values(R.maxpool2_fwd(x), _nhwc(yt.detach()))
    assert R.maxpool2_fwd(x).dtype == npdt
    for dy2, dx_add in ((None, None), (g[1], None), (None, g[2]), (g[1], g[2])):
        xt.grad = None
        yt.backward(_nchw64(g[0]) + (0 if dy2 is None else _nchw64(dy2)), retain_graph=True)
        want = _nhwc(xt.grad) + (0 if dx_add is None else dx_add.astype(np.float64))
        got = R.maxpool2_bwd(x, g[0], dy2, dx_add)
        assert got.dtype == npdt and _same_values(got, want)


def test_maxpool_nan_rule_by_hand():
    """the two facts the kernels were changed for: a window with a NaN pools to NaN, and its gradient goes to the LAST NaN"""
    nan = np.nan
    x = np.array([[1.0, nan], [nan, 0.0]], dtype=np.float32).reshape(1, 2, 2, 1).repeat(8, axis=3)
    assert np.isnan(R.maxpool2_fwd(x)).all()
    dx = R.maxpool2_bwd(x, np.full((1, 1, 1, 8), 3.0, dtype=np.float32))
    assert np.array_equal(dx[0, :, :, 0], [[0.0, 0.0], [3.0, 0.0]])
    ties = np.array([[0.0, 1.0], [1.0, 1.0]], dtype=np.float32).reshape(1, 2, 2, 1).repeat(8, axis=3)
    assert np.array_equal(R.maxpool2_bwd(ties, np.full((1, 1, 1, 8), 3.0, dtype=np.float32))[0, :, :, 0], [[0.0, 3.0], [0.0, 0.0]])
    distinct = np.arange(4, dtype=np.float32).reshape(1, 2, 2, 1).repeat(8, axis=3)
    assert R.tied_fraction(ties) == 1.0 and R.tied_fraction(distinct) == 0.0


def test_maxpool_rounding_order():
    """float32(dy) + float32(dy2) rounded to fp32, then + float32(dx_add), then ONE rounding to fp16"""
    x = np.zeros((1, 2, 2, 8), dtype=np.float16)
    x[0, 0, 0] = 1
    dy = np.full((1, 1, 1, 8), 1.0, dtype=np.float16)
    dy2 = np.full((1, 1, 1, 8), 2.0 ** -11, dtype=np.float16)   # 1 + 2^-11 is exact in fp32 and a tie in fp16
    add = np.full((1, 2, 2, 8), 2.0 ** -14, dtype=np.float16)
    got = R.maxpool2_bwd(x, dy, dy2, add)
    assert got[0, 0, 0, 0] == np.float16(1 + 2.0 ** -10)        # rounding (dy + dy2) to fp16 first would give 1.0
    assert got[0, 1, 1, 0] == np.float16(2.0 ** -14)


UP_SHAPES = [(1, 1), (1, 3), (2, 2), (5, 7), (16, 16), (9, 33), (127, 3)]


def _up64(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("h,w", UP_SHAPES)
def test_upcat_fwd_against_float64(h, w):
    gen = np.random.default_rng(h * 1000 + w)
    B, Cx, Cs = 2, 8, 8
    x = gen.standard_normal((B, h, w, Cx), dtype=np.float32)
    skip = gen.standard_normal((B, 2 * h, 2 * w, Cs), dtype=np.float32)
    y = R.upcat_fwd(x, skip)
    assert y.dtype == np.float32 and y.shape == (B, 2 * h, 2 * w, Cs + Cx)
    assert np.array_equal(y[..., :Cs], skip)
    ref = _nhwc(_up64(_nchw64(x)))
    err, bound = np.abs(y[..., Cs:] - ref).max(), 4 * max(h, w) * 2.0 ** -23 * np.abs(x).max()
    print(f"resample-host upcat_fwd {(h, w)}: worst {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # the storage rounding is numpy's round-to-nearest-even of the fp32 result
    xh, sh = x.astype(np.float16), skip.astype(np.float16)
    yh = R.upcat_fwd(xh, sh)
    assert yh.dtype == np.float16 and np.array_equal(yh[..., Cs:], R.upsample2(xh).astype(np.float16)) and np.array_equal(yh[..., :Cs], sh)


def test_lerp_axis_as_stated():
    for n in (1, 2, 3, 7, 127, 420):
        i0, i1, f = R.lerp_axis(n)
        assert f.dtype == np.float32 and len(i0) == 2 * n
        assert i0[0] == 0 and f[0] == 0 and (i0 <= n - 1).all() and (i1 <= n - 1).all() and ((i1 - i0) == (i0 < n - 1)).all()
        assert (f >= 0).all() and (f[i0 < n - 1] < 1).all()
        scale = np.float32(n - 1) / np.float32(2 * n - 1) if n > 1 else np.float32(0)
        for d in (1, n, 2 * n - 1):
            s = np.float32(scale * np.float32(d))
            assert i0[d] == min(int(s), n - 1) and f[d] == np.float32(s - np.float32(i0[d]))


def test_upcat_compact_layout():
    gen = np.random.default_rng(3)
    B, h, w, cx_ld, cx, cs_ld, cs, ct_ld = 2, 3, 5, 32, 3, 32, 19, 32
    x = gen.standard_normal((B, h, w, cx_ld), dtype=np.float32)
    skip = gen.standard_normal((B, 2 * h, 2 * w, cs_ld), dtype=np.float32)
    x[..., cx:], skip[..., cs:] = np.nan, np.nan
    y = R.upcat_fwd(x, skip, cx, cs, ct_ld)
    full = R.upcat_fwd(np.ascontiguousarray(x[..., :cx]), np.ascontiguousarray(skip[..., :cs]))
    assert y.shape == (B, 2 * h, 2 * w, ct_ld) and np.array_equal(y[..., :cs + cx], full) and not y[..., cs + cx:].any()
    dy = gen.standard_normal((B, 2 * h, 2 * w, ct_ld), dtype=np.float32)
    dy[..., cs + cx:] = np.nan
    ds, dx, A = R.upcat_bwd(dy, None, h, w, None, None, cx, cs, cx_ld, cs_ld)
    ds0, dx0, A0 = R.upcat_bwd(np.ascontiguousarray(dy[..., :cs + cx]), None, h, w, cx, cs)
    assert ds.shape == (B, 2 * h, 2 * w, cs_ld) and np.array_equal(ds[..., :cs], ds0) and not ds[..., cs:].any()
    assert dx.shape == (B, h, w, cx_ld) and np.array_equal(dx[..., :cx], dx0) and not dx[..., cx:].any()
    assert np.array_equal(A[..., :cx], A0) and not A[..., cx:].any()


@pytest.mark.parametrize("with_dy2", [False, True])
@pytest.mark.parametrize("h,w", UP_SHAPES)
def test_upcat_bwd_against_float64_autograd(h, w, with_dy2):
    gen = np.random.default_rng(h * 1000 + w + 7)
    B, Cx, Cs = 2, 8, 8
    dy = gen.standard_normal((B, 2 * h, 2 * w, Cs + Cx), dtype=np.float32)
    dy2 = gen.standard_normal((B, 2 * h, 2 * w, Cs + Cx), dtype=np.float32) if with_dy2 else None
    dskip, dx, A = R.upcat_bwd(dy, dy2, h, w, Cx, Cs)
    g = dy if dy2 is None else dy + dy2                        # numpy fp32 sum: the kernel's rounding of dskip
    assert dskip.dtype == np.float32 and np.array_equal(dskip, g[..., :Cs])
    g64 = dy.astype(np.float64) + (0 if dy2 is None else dy2.astype(np.float64))
    xt = torch.zeros(B, Cx, h, w, dtype=torch.float64, requires_grad=True)
    _up64(xt).backward(_nchw64(g64[..., Cs:]))
    ref = _nhwc(xt.grad)
    err, bound = np.abs(dx - ref).max(), 4 * max(h, w) * 2.0 ** -23 * np.abs(g64[..., Cs:]).max()
    print(f"resample-host upcat_bwd {(h, w)} dy2={with_dy2}: worst {err:.3e} bound {bound:.3e}")
    assert dx.dtype == np.float64 and err <= bound
    # A: the same transpose of the magnitudes -- at least |dx|, at most (sum of a source's weights: about 2 per axis) max
    assert (A >= np.abs(dx) - 1e-12).all() and A.max() <= 5.0 * (np.abs(dy[..., Cs:]).max() + (0 if dy2 is None else np.abs(dy2[..., Cs:]).max())) + 1e-9
