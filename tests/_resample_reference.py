"""Plain numpy restatements of the pooling / resampling operations of maskunet_amd/csrc/elementwise.hip, from the arithmetic the kernels'
comments state.  Nothing of maskunet_amd and no torch is used.  tests/test_resample_reference_host.py pins every function here against
torch in float64 before the GPU tests rely on them.  All arrays are NHWC; the storage dtype (float16 / float32) is the dtype of the inputs.

  * MaxPool2d(2): aten's rule -- scan (0,0), (0,1), (1,0), (1,1), update on `v > m or isnan(v)`: the first maximum of a tie, NaN for a
    window that holds one, its gradient to the last NaN.  Odd H / W floor, the uncovered pixels get 0 + dx_add.
  * bilinear x2 (align_corners=True) + concat [skip, up]: fp32 source index `scale * d`, rows first, then columns, every product and
    sum rounded to fp32 on its own (no FMA), the result rounded to the storage dtype (round to nearest even).
  * its backward: dskip with the kernel's roundings; dx in float64 from the fp32 weights, together with the magnitude sum that bounds
    the kernel's fp32 accumulation error.
"""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------
# MaxPool2d(2)
# ------------------------------------------------------------------------------------------------
def _windows(a, Ho, Wo):
    """the four cells of every 2x2 window in scan order (0,0), (0,1), (1,0), (1,1): views [B, Ho, Wo, C] of a [B, H, W, C]"""
    return [a[:, kh:2 * Ho:2, kw:2 * Wo:2, :] for kh in (0, 1) for kw in (0, 1)]


def maxpool2_scan(x):
    """(maximum [B,Ho,Wo,C] float32, cell index of it [B,Ho,Wo,C] int8) by aten's rule; what maxpool2_fwd and maxpool2_bwd both start
    from (pass it to them as `scan` to compute it once)"""
    B, H, W, C = x.shape
    v = _windows(x.astype(F32, copy=False), H // 2, W // 2)
    m = v[0].copy()
    best = np.zeros(m.shape, dtype=np.int8)
    for k in (1, 2, 3):
        with np.errstate(invalid="ignore"):
            upd = (v[k] > m) | np.isnan(v[k])
        m = np.where(upd, v[k], m)
        best = np.where(upd, np.int8(k), best)
    return m, best


def maxpool2_fwd(x, scan=None):
    """x [B,H,W,C] -> [B,H//2,W//2,C] in x's dtype"""
    return (maxpool2_scan(x) if scan is None else scan)[0].astype(x.dtype)


def maxpool2_bwd(x, dy, dy2=None, dx_add=None, scan=None):
    """dx [B,H,W,C] = scatter(float32(dy) + float32(dy2)) + float32(dx_add), each sum rounded to fp32, then to x's dtype"""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    best = (maxpool2_scan(x) if scan is None else scan)[1]
    g = dy.astype(F32, copy=False)
    if dy2 is not None:
        g = g + dy2.astype(F32, copy=False)
    dx = np.zeros((B, H, W, C), dtype=F32)
    for k, cell in enumerate(_windows(dx, Ho, Wo)):
        cell[...] = np.where(best == k, g, F32(0))
    if dx_add is not None:
        dx += dx_add.astype(F32, copy=False)
    return dx.astype(x.dtype, copy=False)


def tied_fraction(x):
    """fraction of the windows whose maximum is taken by more than one cell"""
    B, H, W, C = x.shape
    v = _windows(x.astype(F32), H // 2, W // 2)
    m = maxpool2_scan(x)[0]
    return float((sum((c == m).astype(np.int32) for c in v) > 1).mean())


def plant_special_windows(x):
    """overwrite the first windows of x [B,H,W,C] (all channels, image 0) with the special patterns; returns how many were planted.
    Input helper of the host and the GPU test."""
    nan, inf = float("nan"), float("inf")
    pats = [(nan, None, None, None), (None, nan, None, None), (None, None, nan, None), (None, None, None, nan),
            (nan, 1, nan, 0), (0, nan, 1, nan), (nan, -1, 1, nan),
            (-inf, -inf, -inf, -inf), (1, inf, inf, 0), (65504, 1, 65504, 0), (-0.0, 0.0, -1, -1), (0.0, -0.0, -1, -1)]
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    assert Ho * Wo >= len(pats)
    for i, p in enumerate(pats):
        ho, wo = divmod(i, Wo)
        for k, v in enumerate(p):
            if v is not None:
                x[0, 2 * ho + k // 2, 2 * wo + k % 2, :] = v
    return len(pats)


# ------------------------------------------------------------------------------------------------
# bilinear x2, align_corners=True
# ------------------------------------------------------------------------------------------------
def lerp_axis(n_in):
    """(i0, i1 int64 [2 n_in], f float32 [2 n_in]) of the destination indices 0 .. 2 n_in - 1, every step in fp32 as the kernel states it"""
    d = np.arange(2 * n_in)
    scale = F32(n_in - 1) / F32(2 * n_in - 1) if n_in > 1 else F32(0)
    s = (scale * d.astype(F32)).astype(F32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    f = (s - i0.astype(F32)).astype(F32)
    return i0, i1, f


def _lerp2(a00, a01, a10, a11, fh, fw):
    one = F32(1)
    r0 = a00 * (one - fh) + a10 * fh
    r1 = a01 * (one - fh) + a11 * fh
    return r0 * (one - fw) + r1 * fw


def upsample2(x):
    """x [B,h,w,C] (any float dtype) -> float32 [B,2h,2w,C], before the rounding to the storage dtype"""
    B, h, w, C = x.shape
    h0, h1, fh = lerp_axis(h)
    w0, w1, fw = lerp_axis(w)
    xf = x.astype(F32)
    top, bot = xf[:, h0], xf[:, h1]
    fh, fw = fh[None, :, None, None], fw[None, None, :, None]
    out = _lerp2(top[:, :, w0], top[:, :, w1], bot[:, :, w0], bot[:, :, w1], fh, fw)
    assert out.dtype == F32
    return out


def upcat_fwd(x, skip, cx=None, cs=None, ct_ld=None):
    """x [B,h,w,Cx], skip [B,2h,2w,Cs] -> y [B,2h,2w,Cs+Cx] = [skip | up].  With cx, cs, ct_ld the compacting form: only the first
    cx / cs channels of x / skip are valid and y = [skip valid | up valid | zeros] with ct_ld channels."""
    B, h, w, Cx = x.shape
    if cx is None:
        return np.concatenate([skip, upsample2(x).astype(x.dtype)], axis=3)
    assert cs + cx <= ct_ld
    y = np.zeros((B, 2 * h, 2 * w, ct_ld), dtype=x.dtype)
    y[..., :cs] = skip[..., :cs]
    y[..., cs:cs + cx] = upsample2(x[..., :cx]).astype(x.dtype)
    return y


def _adjoint_axis(g, n_in):
    """transpose of the interpolation along axis 0 of g [2 n_in, ...] (float64), weights from the fp32 f of lerp_axis"""
    i0, i1, f = lerp_axis(n_in)
    out = np.zeros((n_in,) + g.shape[1:], dtype=np.float64)
    for d in range(2 * n_in):
        if i0[d] == i1[d]:
            out[i0[d]] += g[d]                                 # both taps on one source: weight 1
        else:
            out[i0[d]] += (1.0 - float(f[d])) * g[d]
            out[i1[d]] += float(f[d]) * g[d]
    return out


def _adjoint2(g):
    """g [B,2h,2w,C] float64 -> [B,h,w,C]"""
    B, Ho, Wo, C = g.shape
    t = _adjoint_axis(np.moveaxis(g, 1, 0), Ho // 2)           # [h, B, Wo, C]
    t = _adjoint_axis(np.moveaxis(t, 2, 0), Wo // 2)           # [w, h, B, C]
    return np.ascontiguousarray(np.transpose(t, (2, 1, 0, 3)))


def upcat_bwd(dy, dy2, h, w, Cx, Cs, cx=None, cs=None, cx_ld=None, cs_ld=None):
    """dy (and dy2 or None) [B,2h,2w,Ct] -> (dskip, dx64, A):
      dskip [B,2h,2w,Cs] in dy's dtype = float32(dy) + float32(dy2) rounded (dy itself without dy2);
      dx64  [B,h,w,Cx] float64 = bilinear^T of the exact sum dy + dy2 over the up channels;
      A     [B,h,w,Cx] float64 = sum_k |w_k| (|g_k| + |g2_k|), the magnitude the kernel's roundings scale with.
    Compacting form (cx, cs, cx_ld, cs_ld given; Cx / Cs are ignored): the valid channels are dy[..., :cs] and dy[..., cs:cs+cx], dskip
    has cs_ld and dx64 / A have cx_ld channels, zero behind the valid ones."""
    B = dy.shape[0]
    assert dy.shape[1:3] == (2 * h, 2 * w)
    if cx is not None:
        Cx, Cs = cx, cs
    gs = dy[..., :Cs]
    if dy2 is not None:
        gs = (gs.astype(F32) + dy2[..., :Cs].astype(F32)).astype(dy.dtype)
    g = dy[..., Cs:Cs + Cx].astype(np.float64)
    a = np.abs(g)
    if dy2 is not None:
        g2 = dy2[..., Cs:Cs + Cx].astype(np.float64)
        g, a = g + g2, a + np.abs(g2)
    dx64, A = _adjoint2(g), _adjoint2(a)                       # every weight is >= 0: |w_k| = w_k
    dskip = np.ascontiguousarray(gs)
    if cx is not None:
        pad = np.zeros((B, 2 * h, 2 * w, cs_ld), dtype=dy.dtype)
        pad[..., :cs] = dskip
        dskip = pad
        full = np.zeros((2, B, h, w, cx_ld), dtype=np.float64)
        full[0, ..., :cx], full[1, ..., :cx] = dx64, A
        dx64, A = full[0], full[1]
    return dskip, dx64, A
