"""The pooling / resampling / dropout / add / cast kernels of maskunet_amd/csrc/elementwise.hip through the C ABI, against
tests/_resample_reference.py and plain numpy: bit-equal wherever the kernel only moves values or rounds as stated, and within a bound
derived from the roundings for the one fp32 accumulation (the upsample gradient).  Every buffer is a guarded one: the bands around it
must be intact, inputs unchanged, outputs written everywhere.  Inputs are rounded to the dtype on the host.  Every test prints its worst
error next to its bound (pytest -s / -rP); for a bit-equal comparison that is the number of differing elements next to 0.

"Bit-equal" is: equal as values with the NaN positions equal.  -0 equals +0 in the pool outputs only (fmax-free scans agree on the
value of a signed-zero tie, and the kernel adds `+ 0.f` where the reference leaves a zero alone)."""
import time

import numpy as np
import pytest
import torch

from tests import _resample_reference as R
from tests._device_buffers import Guarded, call

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(F16, id="fp16")]
NP = {F32: np.float32, F16: np.float16}
VEC = {F32: 4, F16: 8}                      # elements of a 16-byte vector
CODE = {F32: 0, F16: 1}                     # MU_F32 / MU_F16
GRID_CAP = 8192 * 256                       # vectors one pass of the 8192-block grid covers


def _note(what, err, bound):
    print(f"elementwise-exact {what}: worst {err:.3e} bound {bound:.3e}")


def _differing(got, ref, signed_zero=True):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype.kind != "f":
        return int((got != ref).sum())
    both_nan = np.isnan(got) & np.isnan(ref)
    if signed_zero:
        u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        same = got.view(u) == ref.view(u)
    else:
        same = got == ref
    return int((~(same | both_nan)).sum())


def _exact(what, got, ref, signed_zero=True):
    bad = _differing(got, ref, signed_zero)
    _note(what, bad, 0)
    assert bad == 0, (what, bad, got.size)


def _bounded(what, err, bound):
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    assert not np.isnan(err).any(), what
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    i = int(np.argmax(ratio))
    _note(what, float(err.flat[i]), float(bound.flat[i]))
    assert ratio.flat[i] <= 1.0, (what, float(err.flat[i]), float(bound.flat[i]))
    return float(ratio.flat[i])


def _in(a, dt, name=None):
    a = np.ascontiguousarray(a)
    assert a.dtype == NP.get(dt, a.dtype)
    return Guarded(a.size, dt, a, name)


def _out(shape, dt, name):
    return Guarded(int(np.prod(shape)), dt, name=name)


def _result(buf, shape):
    buf.all_written()
    return buf.host(shape)


def _normal(gen, shape, dt, scale=1.0):
    return (gen.standard_normal(shape, dtype=np.float32) * np.float32(scale)).astype(NP[dt])


def _raw_status(name, *args):
    """the entry point's own return value (no Guarded here: the call must refuse before it launches anything)"""
    from maskunet_amd import _lib
    return getattr(_lib.load(), name)(*args, _lib.stream())


MU_ERR_SHAPE = -2
MU_F32X, BAD_DTYPE = 2, 99                  # fp32 storage with encoded matrix operands (only the weight preparations take it); no dtype


def _refused(code, name, *args, outs):
    """the entry point returns `code` before it launches anything: every output still holds the sentinel, every band is intact"""
    from maskunet_amd import _lib
    with pytest.raises(RuntimeError, match=code):
        _lib.call(name, *[a.p if isinstance(a, Guarded) else a for a in args], _lib.stream())
    torch.cuda.synchronize()
    for a in list(args) + list(outs):
        if isinstance(a, Guarded):
            a.check()
    for o in outs:
        assert bool((o.t == o.sent).all()), (name, code, o.name)


def _dtype_gate(name, args_of, outs, code, bad=(MU_F32X, BAD_DTYPE)):
    """args_of(c): the arguments with c as the dtype.  Every code of `bad` is MU_ERR_ARG with `outs` untouched; then the valid call on
    the same buffers (the caller compares the outputs)."""
    for c in bad:
        _refused("MU_ERR_ARG", name, *args_of(c), outs=outs)
    call(name, *args_of(code))


def _small_ints(gen, shape, dt):
    return gen.integers(-3, 4, shape).astype(NP[dt])


# ================================================================================================
# max-pool: mu_maxpool2_fwd / mu_maxpool2_bwd / mu_maxpool2_bwd_acc -- bit-equal, -0 == +0
# ================================================================================================
POOL_SHAPES = [(1, 2, 2, 8), (2, 3, 2, 8), (2, 2, 3, 8), (2, 7, 5, 32), (1, 13, 8, 16), (2, 12, 9, 40)]


def _pool_forward(what, dt, x):
    B, H, W, C = x.shape
    xg, y = _in(x, dt, "x"), _out((B, H // 2, W // 2, C), dt, "y")
    call("mu_maxpool2_fwd", xg, y, B, H, W, C, CODE[dt])
    scan = R.maxpool2_scan(x)
    _exact(what + " y", _result(y, (B, H // 2, W // 2, C)), R.maxpool2_fwd(x, scan), signed_zero=False)
    return xg, scan


def _pool_backward(what, dt, x, xg, scan, dy, dy2, dx_add):
    B, H, W, C = x.shape
    g = [None if a is None else _in(a, dt, n) for a, n in ((dy, "dy"), (dy2, "dy2"), (dx_add, "dx_add"))]
    dx = _out(x.shape, dt, "dx")
    if dy2 is None and dx_add is None:
        call("mu_maxpool2_bwd", xg, g[0], dx, B, H, W, C, CODE[dt])
    else:
        call("mu_maxpool2_bwd_acc", xg, g[0], g[1], g[2], dx, B, H, W, C, CODE[dt])
    tag = " dx" + ("+dy2" if dy2 is not None else "") + ("+dx_add" if dx_add is not None else "")
    _exact(what + tag, _result(dx, x.shape), R.maxpool2_bwd(x, dy, dy2, dx_add, scan), signed_zero=False)


def _pool_all(what, dt, x, gen):
    B, H, W, C = x.shape
    dy, dy2, dx_add = (_normal(gen, s, dt) for s in ((B, H // 2, W // 2, C), (B, H // 2, W // 2, C), x.shape))
    xg, scan = _pool_forward(what, dt, x)
    for a2, aa in ((None, None), (dy2, None), (None, dx_add), (dy2, dx_add)):
        _pool_backward(what, dt, x, xg, scan, dy, a2, aa)


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_tied_windows(dt, shape):
    """values from {-1, 0, 1}: more than half of the windows tie, so the routing rule -- first maximum in scan order -- decides most
    gradients; odd H / W run the tail kernel with and without dx_add.  All three windows-per-axis parities, one and several blocks."""
    gen = np.random.default_rng(sum(shape))
    x = gen.integers(-1, 2, shape).astype(NP[dt])
    tied = R.tied_fraction(x)
    print(f"elementwise-exact maxpool {shape}: {tied:.0%} of the windows tie")
    assert tied >= 0.40
    _pool_all(f"maxpool {shape}", dt, x, gen)


@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_special_windows(dt):
    """NaN in each of the four cells and in two of them (the window pools to NaN, the gradient goes to the last NaN), all -inf, a tied
    +inf, the largest fp16, -0 against +0; odd H and W"""
    shape = (1, 7, 9, 8)
    gen = np.random.default_rng(79)
    x = gen.integers(-1, 2, shape).astype(NP[dt])
    n = R.plant_special_windows(x)
    y = R.maxpool2_fwd(x)
    assert np.isnan(y[0, :2].reshape(-1, 8)[:7]).all() and n == 12 and np.isnan(y).sum() == 7 * 8
    _pool_all("maxpool special windows", dt, x, gen)


@pytest.mark.parametrize("dt,shape", [pytest.param(F16, (1, 2050, 4100, 8), id="fp16-1x2050x4100x8"),
                                      pytest.param(F32, (1, 2050, 2052, 8), id="fp32-1x2050x2052x8")])
def test_maxpool_grid_stride(dt, shape):
    """2 101 250 (fp16) and 2 103 300 (fp32) vectors against the 2 097 152 one pass of the capped grid covers: the loops of the forward
    and of the backward (with both addends) run a second time for the last few thousand.  134 MB tensors: the longest tests of the file."""
    t0 = time.perf_counter()
    B, H, W, C = shape
    assert B * (H // 2) * (W // 2) * (C // VEC[dt]) == {F16: 2101250, F32: 2103300}[dt] > GRID_CAP
    gen = np.random.default_rng(H + W)
    # values through 256-entry lookup tables of random bytes (drawing and converting 67 M numbers one by one is most of such a test's
    # time): x from {-1, 0, 1}, the gradients multiples of 1/32 below 4, dx_add multiples of 1/128 below 1 -- their sums still round in fp16
    small, byte = (B, H // 2, W // 2, C), np.arange(256)
    x = (byte % 3 - 1).astype(NP[dt])[gen.integers(0, 256, shape, dtype=np.uint8)]
    dy, dy2 = (((byte - 128) / 32.0).astype(NP[dt])[gen.integers(0, 256, small, dtype=np.uint8)] for _ in range(2))
    dx_add = ((byte - 128) / 128.0).astype(NP[dt])[gen.integers(0, 256, shape, dtype=np.uint8)]
    assert R.tied_fraction(x[:, :64]) >= 0.40
    xg, scan = _pool_forward(f"maxpool grid {shape}", dt, x)
    _pool_backward(f"maxpool grid {shape}", dt, x, xg, scan, dy, dy2, dx_add)
    print(f"elementwise-exact maxpool grid {shape}: {time.perf_counter() - t0:.1f} s")


# ================================================================================================
# upsample + concat: mu_upcat_fwd / mu_upcat_bwd / mu_upcat_bwd_acc
# forward and dskip bit-equal; |dx - ref64| <= 24 * 2^-24 * A + r, A = sum_k |w_k| (|g_k| + |g2_k|): at most 16 taps, each with the
# rounding of g + g2, of wh * ww, of the product and of the running sum; r = 2^-11 |ref64| + 2^-25 for fp16 (the output rounding and
# the subnormal step), 0 for fp32.
# ================================================================================================
def _dx_bound(dt, ref64, A):
    return 24 * 2.0 ** -24 * A + (2.0 ** -11 * np.abs(ref64) + 2.0 ** -25 if dt == F16 else 0.0)


def _fwd_by_rows(Cx, Cs):
    cv = (Cx + Cs) // 8
    return cv <= 256 and 256 % cv == 0


def _bwd_by_rows(Cx, Cs):
    cvs, cvx = Cs // 8, Cx // 8
    return cvs <= 256 and 256 % cvs == 0 and cvx <= 256 and 256 % cvx == 0


def _upcat_forward(what, dt, gen, B, h, w, Cx, Cs):
    x, skip = _normal(gen, (B, h, w, Cx), dt), _normal(gen, (B, 2 * h, 2 * w, Cs), dt)
    y = _out((B, 2 * h, 2 * w, Cs + Cx), dt, "y")
    call("mu_upcat_fwd", _in(x, dt, "x"), _in(skip, dt, "skip"), y, B, h, w, Cx, Cs, CODE[dt])
    _exact(what + " y", _result(y, (B, 2 * h, 2 * w, Cs + Cx)), R.upcat_fwd(x, skip))


def _upcat_backward(what, dt, gen, B, h, w, Cx, Cs, plain=True):
    shape = (B, 2 * h, 2 * w, Cs + Cx)
    dy, dy2 = _normal(gen, shape, dt), _normal(gen, shape, dt)
    g1, g2 = _in(dy, dt, "dy"), _in(dy2, dt, "dy2")
    worst = 0.0
    for second in ((None, dy2) if plain else (dy2,)):
        dx, dskip = _out((B, h, w, Cx), dt, "dx"), _out((B, 2 * h, 2 * w, Cs), dt, "dskip")
        if second is None:
            call("mu_upcat_bwd", g1, dx, dskip, B, h, w, Cx, Cs, CODE[dt])
        else:
            call("mu_upcat_bwd_acc", g1, g2, dx, dskip, B, h, w, Cx, Cs, CODE[dt])
        rskip, ref64, A = R.upcat_bwd(dy, second, h, w, Cx, Cs)
        tag = what + (" +dy2" if second is not None else "")
        _exact(tag + " dskip", _result(dskip, rskip.shape), rskip)
        got = _result(dx, ref64.shape).astype(np.float64)
        worst = max(worst, _bounded(tag + " dx", np.abs(got - ref64), _dx_bound(dt, ref64, A)))
    return worst


# (B, h, w, Cx, Cs), forward by rows?, backward by rows? (None: no backward) -- asserted against the dispatch conditions
UPCAT_F16 = [
    ((2, 1, 1, 8, 8), True, True),              # h = w = 1
    ((1, 3, 1, 8, 8), True, True),              # w = 1
    ((2, 5, 9, 256, 256), True, True),          # Wo = 18: 16 pixels per forward iteration, 8 input pixels per dx iteration -> partial second ones
    ((1, 2, 70, 32, 32), True, True),           # Wo = 140 against 128 pixels per iteration
    ((1, 4, 3, 1024, 1024), True, True),        # one pixel per iteration
    ((1, 2, 2, 2040, 8), True, False),          # 255 vectors of x: forward by rows, backward by elements
    ((1, 8200, 1, 8, 8), True, None),           # 16400 output rows over the 16384-block clamp of the forward
    ((2, 5, 7, 32, 64), False, True),           # 12 vectors per pixel: forward by elements (its backward's 4 and 8 go by rows)
    ((1, 3, 4, 8, 16), False, True),
]


@pytest.mark.parametrize("case,fwd_rows,bwd_rows", UPCAT_F16, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_upcat_fp16(case, fwd_rows, bwd_rows):
    B, h, w, Cx, Cs = case
    assert _fwd_by_rows(Cx, Cs) == fwd_rows and (bwd_rows is None or _bwd_by_rows(Cx, Cs) == bwd_rows)
    gen = np.random.default_rng(sum(case))
    _upcat_forward(f"upcat fp16 {case}", F16, gen, B, h, w, Cx, Cs)
    if bwd_rows is not None:
        _upcat_backward(f"upcat fp16 {case}", F16, gen, B, h, w, Cx, Cs)


@pytest.mark.parametrize("case", [(2, 1, 1, 8, 8), (2, 5, 7, 32, 64), (1, 9, 33, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_upcat_fp32(case):
    B, h, w, Cx, Cs = case
    gen = np.random.default_rng(sum(case) + 1)
    _upcat_forward(f"upcat fp32 {case}", F32, gen, B, h, w, Cx, Cs)
    _upcat_backward(f"upcat fp32 {case}", F32, gen, B, h, w, Cx, Cs)


def _upcat_vectors(dt, B, h, w, Cx, Cs):
    N = VEC[dt]
    return B * 4 * h * w * ((Cx + Cs) // N), B * 4 * h * w * (Cs // N) + B * h * w * (Cx // N)


def test_upcat_grid_stride_fp16():
    """(1,420,418,8,16): the element forward loops a second time; its backward goes by rows (2 and 1 vectors per pixel), a block per
    row and no loop over the grid.  (1,420,418,8,24) sends the BACKWARD through the element kernel, past the cap as well."""
    case = (1, 420, 418, 8, 16)
    assert _upcat_vectors(F16, *case)[0] > GRID_CAP and not _fwd_by_rows(8, 16) and _bwd_by_rows(8, 16)
    gen = np.random.default_rng(420)
    _upcat_forward(f"upcat fp16 grid {case}", F16, gen, *case)
    _upcat_backward(f"upcat fp16 grid {case}", F16, gen, *case, plain=False)


def test_upcat_grid_stride_fp16_backward_by_elements():
    case = (1, 420, 418, 8, 24)
    assert _upcat_vectors(F16, *case)[1] > GRID_CAP and not _bwd_by_rows(8, 24)
    _upcat_backward(f"upcat fp16 grid {case}", F16, np.random.default_rng(421), *case, plain=False)


def test_upcat_grid_stride_fp32():
    """(1,363,365,8,8): 2 119 920 forward vectors; its backward has 1 324 950, under the cap, so (1,363,365,8,16) runs the backward
    with 2 384 910"""
    case = (1, 363, 365, 8, 8)
    assert _upcat_vectors(F32, *case)[0] > GRID_CAP
    gen = np.random.default_rng(363)
    _upcat_forward(f"upcat fp32 grid {case}", F32, gen, *case)
    _upcat_backward(f"upcat fp32 grid {case}", F32, gen, *case, plain=False)
    case = (1, 363, 365, 8, 16)
    assert _upcat_vectors(F32, *case)[1] > GRID_CAP
    _upcat_backward(f"upcat fp32 grid {case}", F32, gen, *case, plain=False)


# ================================================================================================
# compacting form: mu_upcat_compact_fwd / mu_upcat_compact_bwd -- NaN in every pad channel of the inputs
# ================================================================================================
COMPACT = [(2, 3, 5, 32, 3, 32, 19, 32), (1, 1, 1, 32, 16, 32, 16, 32), (1, 4, 2, 64, 45, 64, 50, 96), (1, 2, 3, 32, 32, 32, 7, 64)]


@pytest.mark.parametrize("case", COMPACT, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", DTYPES)
def test_upcat_compact(dt, case):
    B, h, w, cx_ld, cx, cs_ld, cs, ct_ld = case
    gen = np.random.default_rng(sum(case))
    what = f"upcat compact {case}"
    x, skip = _normal(gen, (B, h, w, cx_ld), dt), _normal(gen, (B, 2 * h, 2 * w, cs_ld), dt)
    x[..., cx:], skip[..., cs:] = np.nan, np.nan
    y = _out((B, 2 * h, 2 * w, ct_ld), dt, "y")
    call("mu_upcat_compact_fwd", _in(x, dt, "x"), _in(skip, dt, "skip"), y, B, h, w, cx_ld, cx, cs_ld, cs, ct_ld, CODE[dt])
    got = _result(y, (B, 2 * h, 2 * w, ct_ld))
    assert np.isfinite(got).all() and not got[..., cs + cx:].any()
    _exact(what + " y", got, R.upcat_fwd(x, skip, cx, cs, ct_ld))

    dy = _normal(gen, (B, 2 * h, 2 * w, ct_ld), dt)
    dy[..., cs + cx:] = np.nan
    dx, dskip = _out((B, h, w, cx_ld), dt, "dx"), _out((B, 2 * h, 2 * w, cs_ld), dt, "dskip")
    call("mu_upcat_compact_bwd", _in(dy, dt, "dy"), dx, dskip, B, h, w, cx_ld, cx, cs_ld, cs, ct_ld, CODE[dt])
    rskip, ref64, A = R.upcat_bwd(dy, None, h, w, None, None, cx, cs, cx_ld, cs_ld)
    gskip, gx = _result(dskip, rskip.shape), _result(dx, ref64.shape)
    assert np.isfinite(gskip).all() and np.isfinite(gx).all() and not gskip[..., cs:].any() and not gx[..., cx:].any()
    _exact(what + " dskip", gskip, rskip)
    _bounded(what + " dx", np.abs(gx.astype(np.float64) - ref64)[..., :cx], _dx_bound(dt, ref64, A)[..., :cx])


# ================================================================================================
# dropout: mu_dropout / mu_dropout_step
# ================================================================================================
N_DROP = 1 << 20
SEEDS = [12345, (1 << 61) + 7]


def _scale(p):
    """the entry point's own fp32 arithmetic: 1.0f / (1.0f - p)"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def _dropout(dt, x, p, seed, step=None, mask=None, entry=None):
    """(y, mask_out) of one call; step: None (mu_dropout) or the value of the device counter (mu_dropout_step)"""
    n = x.size
    xg, y, mo = _in(x, dt, "x"), _out((n,), dt, "y"), _out((n,), torch.uint8, "mask_out")
    mg = None if mask is None else _in(mask, torch.uint8, "mask")
    if step is None and entry != "step":
        call("mu_dropout", xg, y, n, float(p), seed, mg, mo, CODE[dt])
    else:
        sg = None if step is None else _in(np.array([step], dtype=np.int64), torch.int64, "seed_step")
        call("mu_dropout_step", xg, y, n, float(p), seed, sg, mg, mo, CODE[dt])
    return _result(y, (n,)), _result(mo, (n,))


def _consistent(what, dt, x, p, y, keep):
    assert set(np.unique(keep).tolist()) <= {0, 1}
    ref = np.where(keep != 0, x.astype(np.float32) * _scale(p), np.float32(0)).astype(NP[dt])
    _exact(what + " y", y, ref)


@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_explicit_mask(dt):
    gen = np.random.default_rng(30)
    x = _normal(gen, (N_DROP,), dt, 3.0)
    mask = (gen.random(N_DROP) < 0.6).astype(np.uint8)
    for p in (0.3, 0.5):
        assert _scale(p) == np.float32(1.0 / (1.0 - float(np.float32(p))))     # both readings of "float32(1 / (1 - p))" are one number here
        for entry in ("plain", "step"):
            y, mo = _dropout(dt, x, p, SEEDS[0], mask=mask, entry=entry)
            _exact(f"dropout mask p={p} {entry} mask_out", mo, mask)
            _consistent(f"dropout mask p={p} {entry}", dt, x, p, y, mask)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_generator_p0_is_identity(dt, seed):
    x = _normal(np.random.default_rng(31), (N_DROP,), dt, 3.0)
    for step in (None, 1):
        y, mo = _dropout(dt, x, 0.0, seed, step)
        assert mo.all()
        _exact(f"dropout p=0 step={step} y", y, x)


def _sigmas(what, frac, expect, count, var=None):
    sigma = np.sqrt((expect * (1 - expect) if var is None else var) / count)
    dev = np.abs(np.asarray(frac, dtype=np.float64) - expect)
    _note(what, float(dev.max()), 5 * sigma)
    assert dev.max() <= 5 * sigma, (what, frac, expect, sigma)
    return float(dev.max() / sigma)


@pytest.mark.parametrize("seed", SEEDS, ids=["seed12345", "seed2p61p7"])
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_generator(dt, p, seed):
    """the backward's promise (same seed and step on another tensor: the same keeps), the element index as the only position input
    (a longer tensor past the grid cap starts with the same keeps), independent masks for another seed or step, and the keep
    probability q = 1 - floor(p 65536) / 65536 overall and for every 16-bit slice of the two generator words: all within 5 sigma,
    sigma = sqrt(q (1 - q) / count).  (An agreement fraction has the variance e (1 - e) / count with e = q^2 + (1 - q)^2, which is the
    larger of the two for q != 1/2: the smaller one is asserted.)  The seeds are fixed, so the figures are too: over all cases the worst
    keep fraction sits at 2.8 sigma, the worst lane at 2.7 and the worst agreement at 3.8."""
    N = VEC[dt]
    gen = np.random.default_rng(32)
    x = _normal(gen, (N_DROP,), dt, 3.0)
    x2 = _normal(gen, (N_DROP,), dt, 3.0)
    q = 1.0 - np.floor(float(np.float32(p) * np.float32(65536))) / 65536.0
    what = f"dropout p={p} seed={seed}"
    masks = {}
    for step in (None, 0, 1, 1 << 40):
        y, keep = _dropout(dt, x, p, seed, step)
        _consistent(f"{what} step={step}", dt, x, p, y, keep)
        masks[step] = keep
        _sigmas(f"{what} step={step} keep", keep.mean(), q, N_DROP)
        _sigmas(f"{what} step={step} keep per lane", keep.reshape(-1, N).mean(axis=0), q, N_DROP // N)
    for step in (None, 1):
        y2, keep2 = _dropout(dt, x2, p, seed, step)
        _consistent(f"{what} step={step} second tensor", dt, x2, p, y2, keep2)
        _exact(f"{what} step={step} second tensor mask_out", keep2, masks[step])
    n_long = (1 << 21) * 8 + 8 * 261
    assert n_long // N > GRID_CAP
    ones = np.ones(n_long, dtype=NP[dt])
    ylong, klong = _dropout(dt, ones, p, seed)
    _exact(f"{what} long tensor first keeps", klong[:N_DROP], masks[None])
    _consistent(f"{what} long tensor", dt, ones, p, ylong, klong)
    _sigmas(f"{what} long tensor tail keep", klong[GRID_CAP * N:].mean(), q, n_long - GRID_CAP * N)
    agree = q * q + (1 - q) * (1 - q)
    other = _dropout(dt, x, p, seed ^ 0x5DEECE66D)[1]
    _sigmas(f"{what} agreement with another seed", (other == masks[None]).mean(), agree, N_DROP, var=min(q * (1 - q), agree * (1 - agree)))
    for step in (0, 1, 1 << 40):
        _sigmas(f"{what} agreement step None / {step}", (masks[step] == masks[None]).mean(), agree, N_DROP, var=min(q * (1 - q), agree * (1 - agree)))
    _sigmas(f"{what} agreement step 0 / 1", (masks[0] == masks[1]).mean(), agree, N_DROP, var=min(q * (1 - q), agree * (1 - agree)))


@pytest.mark.parametrize("dt", DTYPES)
def test_dropout_refuses_a_partial_vector(dt):
    N = VEC[dt]
    buf = torch.zeros(64, dtype=dt, device="cuda")
    for n in (N + N // 2, N - 1, 1):
        for name, extra in (("mu_dropout", ()), ("mu_dropout_step", (None,))):
            rc = _raw_status(name, buf.data_ptr(), buf.data_ptr(), n, 0.3, 1, *extra, None, None, CODE[dt])
            assert rc == MU_ERR_SHAPE, (name, n, rc)
    torch.cuda.synchronize()
    assert not buf.any()


# ================================================================================================
# mu_add: bit-equal to the fp32 sum rounded to the dtype; in place on either operand
# ================================================================================================
def _add_ref(a, b):
    with np.errstate(over="ignore"):                           # 60000 + 60000 is inf in fp16, as in the kernel
        return (a.astype(np.float32) + b.astype(np.float32)).astype(a.dtype)


@pytest.mark.parametrize("n_vec", [1, 37, 256 * 3 + 5, GRID_CAP + 5], ids=lambda v: f"{v}vec")
@pytest.mark.parametrize("dt", DTYPES)
def test_add(dt, n_vec):
    n = n_vec * VEC[dt]
    gen = np.random.default_rng(n_vec)
    a, b = _normal(gen, (n,), dt, 4.0), _normal(gen, (n,), dt, 4.0)
    if dt == F16:
        a[:4], b[:4] = [1.0, 1.0, 60000.0, -0.0], [2.0 ** -11, 3 * 2.0 ** -11, 60000.0, -0.0]   # ties to even both ways, overflow, -0
    ref = _add_ref(a, b)
    ag, bg, out = _in(a, dt, "a"), _in(b, dt, "b"), _out((n,), dt, "out")
    call("mu_add", ag, bg, out, n, CODE[dt])
    _exact(f"add n={n} out of place", _result(out, (n,)), ref)
    for alias in ("a", "b"):                                   # ops.py accumulates in place: out == a
        io = _out((n,), dt, "out = " + alias)
        io.t.copy_(torch.from_numpy(a if alias == "a" else b))
        if alias == "a":
            call("mu_add", io, bg, io, n, CODE[dt])
        else:
            call("mu_add", ag, io, io, n, CODE[dt])
        _exact(f"add n={n} out == {alias}", _result(io, (n,)), ref)


@pytest.mark.parametrize("dt", DTYPES)
def test_add_refuses_a_partial_vector(dt):
    N = VEC[dt]
    buf = torch.zeros(64, dtype=dt, device="cuda")
    for n in (N + N // 2, N - 1, 1):
        assert _raw_status("mu_add", buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), n, CODE[dt]) == MU_ERR_SHAPE
    torch.cuda.synchronize()
    assert not buf.any()


# ================================================================================================
# mu_cast: all four dtype pairs, bit-equal to numpy's astype (round to nearest even, overflow to inf, gradual underflow)
# ================================================================================================
def _cast_specials():
    t = 2.0 ** -11                             # half an fp16 ulp at 1
    v = [1 + t, 1 + 3 * t, 1 + t * (1 + 2.0 ** -12), 1 + t * (1 - 2.0 ** -12), -(1 + t), 2048 + 1, 2048 + 3,      # ties, and next to them
         65504, 65519.99, 65520, 65536, -65519.99, -65520, 1e30, -1e30,                 # the largest finite value against inf
         2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25,      # subnormals and their ties
         2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, -(2.0 ** -25), 1e-30, 2.0 ** -149,    # below the smallest subnormal
         np.inf, -np.inf, np.nan, -0.0, 0.0]
    return np.array(v, dtype=np.float32)


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 77])
@pytest.mark.parametrize("src,dst", [(F32, F16), (F16, F32), (F32, F32), (F16, F16)], ids=["f32-f16", "f16-f32", "f32-f32", "f16-f16"])
def test_cast(src, dst, n):
    """n = 1, one under and one over a block, and 77 past one pass of the 4096-block grid; no alignment requirement"""
    gen = np.random.default_rng(n)
    sp = _cast_specials()
    x = gen.standard_normal(n, dtype=np.float32) * np.float32(8)
    x[-min(n, len(sp)):] = sp[:min(n, len(sp))]                # the specials sit at the END: in the loop's second pass for the long one
    if n == 1:
        x[0] = 65520.0
    with np.errstate(over="ignore"):
        x = x.astype(NP[src])
        ref = x.astype(NP[dst])
    if src == F32 and dst == F16 and n >= len(sp):
        tail = ref[-len(sp):]
        assert tail[0] == 1 and tail[1] == np.float16(1 + 2.0 ** -9) and tail[7] == 65504 and tail[8] == 65504 and np.isinf(tail[9])
        assert tail[17] == np.float16(2.0 ** -24) and tail[18] == np.float16(2.0 ** -23) and tail[20] == 0 and tail[21] == np.float16(2.0 ** -24)
    out = _out((n,), dst, "dst")
    call("mu_cast", _in(x, src, "src"), CODE[src], out, CODE[dst], n)
    _exact(f"cast {NP[src].__name__} -> {NP[dst].__name__} n={n}", _result(out, (n,)), ref)


# ================================================================================================
# the host layer of every dtype-taking entry point, at its smallest shape: MU_F32X (where the entry point takes no encoded operand) and
# an unknown dtype are MU_ERR_ARG before anything is launched -- the outputs still hold the sentinel -- and the valid call on the same
# buffers gives the reference bit for bit.  Small-integer inputs where the kernel accumulates, so that "bit for bit" holds there too.
# ================================================================================================
@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_maxpool(dt):
    shape, small = (1, 2, 2, 8), (1, 1, 1, 8)
    gen = np.random.default_rng(501)
    x, dy, dy2, dx_add = _small_ints(gen, shape, dt), _small_ints(gen, small, dt), _small_ints(gen, small, dt), _small_ints(gen, shape, dt)
    xg, g1, g2, ga = _in(x, dt, "x"), _in(dy, dt, "dy"), _in(dy2, dt, "dy2"), _in(dx_add, dt, "dx_add")
    y, dx, dx2 = _out(small, dt, "y"), _out(shape, dt, "dx"), _out(shape, dt, "dx (plain)")
    _refused("MU_ERR_ARG", "mu_maxpool2_fwd", None, y, 1, 2, 2, 8, BAD_DTYPE, outs=[y])
    _dtype_gate("mu_maxpool2_fwd", lambda c: (xg, y, 1, 2, 2, 8, c), [y], CODE[dt])
    _exact("gate maxpool y", _result(y, small), R.maxpool2_fwd(x), signed_zero=False)
    _dtype_gate("mu_maxpool2_bwd_acc", lambda c: (xg, g1, g2, ga, dx, 1, 2, 2, 8, c), [dx], CODE[dt])
    _exact("gate maxpool dx+dy2+dx_add", _result(dx, shape), R.maxpool2_bwd(x, dy, dy2, dx_add), signed_zero=False)
    _dtype_gate("mu_maxpool2_bwd", lambda c: (xg, g1, dx2, 1, 2, 2, 8, c), [dx2], CODE[dt])
    _exact("gate maxpool dx", _result(dx2, shape), R.maxpool2_bwd(x, dy), signed_zero=False)


@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_upcat(dt):
    """B = 1, h = w = 1, Cx = Cs = 8: the fp16 calls go by rows, the fp32 ones by elements; every weight is 1, so dx is an exact sum"""
    gen = np.random.default_rng(502)
    x, skip = _small_ints(gen, (1, 1, 1, 8), dt), _small_ints(gen, (1, 2, 2, 8), dt)
    dy, dy2 = _small_ints(gen, (1, 2, 2, 16), dt), _small_ints(gen, (1, 2, 2, 16), dt)
    xg, sg, g1, g2 = _in(x, dt, "x"), _in(skip, dt, "skip"), _in(dy, dt, "dy"), _in(dy2, dt, "dy2")
    y = _out((1, 2, 2, 16), dt, "y")
    _dtype_gate("mu_upcat_fwd", lambda c: (xg, sg, y, 1, 1, 1, 8, 8, c), [y], CODE[dt])
    _exact("gate upcat y", _result(y, (1, 2, 2, 16)), R.upcat_fwd(x, skip))
    for name, second in (("mu_upcat_bwd_acc", dy2), ("mu_upcat_bwd", None)):
        dx, dskip = _out((1, 1, 1, 8), dt, "dx"), _out((1, 2, 2, 8), dt, "dskip")
        grads = (g1, g2) if second is not None else (g1,)
        _dtype_gate(name, lambda c: (*grads, dx, dskip, 1, 1, 1, 8, 8, c), [dx, dskip], CODE[dt])
        rskip, ref64, _ = R.upcat_bwd(dy, second, 1, 1, 8, 8)
        assert (ref64 == ref64.astype(NP[dt])).all()
        _exact(f"gate {name} dskip", _result(dskip, rskip.shape), rskip)
        _exact(f"gate {name} dx", _result(dx, ref64.shape), ref64.astype(NP[dt]))


@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_upcat_compact(dt):
    """3 of 8 channels of x and 5 of 8 of skip into 8; NaN in every pad channel of the inputs"""
    gen = np.random.default_rng(503)
    x, skip, dy = _small_ints(gen, (1, 1, 1, 8), dt), _small_ints(gen, (1, 2, 2, 8), dt), _small_ints(gen, (1, 2, 2, 8), dt)
    x[..., 3:], skip[..., 5:] = np.nan, np.nan
    y, dx, dskip = _out((1, 2, 2, 8), dt, "y"), _out((1, 1, 1, 8), dt, "dx"), _out((1, 2, 2, 8), dt, "dskip")
    dims = (1, 1, 1, 8, 3, 8, 5, 8)
    xg, sg, gg = _in(x, dt, "x"), _in(skip, dt, "skip"), _in(dy, dt, "dy")
    _dtype_gate("mu_upcat_compact_fwd", lambda c: (xg, sg, y, *dims, c), [y], CODE[dt])
    _exact("gate compact y", _result(y, (1, 2, 2, 8)), R.upcat_fwd(x, skip, 3, 5, 8))
    _dtype_gate("mu_upcat_compact_bwd", lambda c: (gg, dx, dskip, *dims, c), [dx, dskip], CODE[dt])
    rskip, ref64, _ = R.upcat_bwd(dy, None, 1, 1, None, None, 3, 5, 8, 8)
    assert (ref64 == ref64.astype(NP[dt])).all()
    _exact("gate compact dskip", _result(dskip, rskip.shape), rskip)
    _exact("gate compact dx", _result(dx, ref64.shape), ref64.astype(NP[dt]))


@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_dropout_and_add(dt):
    """one vector each.  An unknown dtype with a partial vector (n = 3) or with a null pointer is MU_ERR_ARG; the partial vector alone
    is MU_ERR_SHAPE."""
    n = VEC[dt]
    gen = np.random.default_rng(504)
    x, b = _normal(gen, (n,), dt, 3.0), _normal(gen, (n,), dt, 3.0)
    mask = np.array([1, 0, 1, 1, 0, 1, 0, 0][:n], dtype=np.uint8)
    xg, bg, mg = _in(x, dt, "x"), _in(b, dt, "b"), _in(mask, torch.uint8, "mask")
    ref = np.where(mask != 0, x.astype(np.float32) * _scale(0.3), np.float32(0)).astype(NP[dt])
    for name, extra in (("mu_dropout_step", (None,)), ("mu_dropout", ())):
        y, mo = _out((n,), dt, "y"), _out((n,), torch.uint8, "mask_out")
        for c in (MU_F32X, BAD_DTYPE):
            _refused("MU_ERR_ARG", name, xg, y, 3, 0.3, 1, *extra, mg, mo, c, outs=[y, mo])
        _refused("MU_ERR_ARG", name, None, y, n, 0.3, 1, *extra, mg, mo, BAD_DTYPE, outs=[y, mo])
        _refused("MU_ERR_SHAPE", name, xg, y, 3, 0.3, 1, *extra, mg, mo, CODE[dt], outs=[y, mo])
        _dtype_gate(name, lambda c: (xg, y, n, 0.3, 1, *extra, mg, mo, c), [y, mo], CODE[dt])
        _exact(f"gate {name} y", _result(y, (n,)), ref)
        _exact(f"gate {name} mask_out", _result(mo, (n,)), mask)
    out = _out((n,), dt, "out")
    for c in (MU_F32X, BAD_DTYPE):
        _refused("MU_ERR_ARG", "mu_add", xg, bg, out, 3, c, outs=[out])
    _refused("MU_ERR_ARG", "mu_add", None, bg, out, n, BAD_DTYPE, outs=[out])
    _refused("MU_ERR_SHAPE", "mu_add", xg, bg, out, 3, CODE[dt], outs=[out])
    _dtype_gate("mu_add", lambda c: (xg, bg, out, n, c), [out], CODE[dt])
    _exact("gate add", _result(out, (n,)), _add_ref(x, b))


def _unit(u8, dt):
    """ToTensor of image bytes: byte / 255 by fp32 division, rounded to the dtype"""
    return (u8.astype(np.float32) / np.float32(255)).astype(NP[dt])


@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_image_inputs(dt):
    """mu_u8_to_nhwc on one pixel (3 of 8 channels), mu_resize_u8_nhwc 2 x 2 -> 1 x 1 (cv::resize's INTER_AREA shortcut)"""
    from oracle import cv2_resize_oracle
    px = np.array([0, 37, 255], dtype=np.uint8)
    src, dst = _in(px, torch.uint8, "src"), _out((8,), dt, "dst")
    _dtype_gate("mu_u8_to_nhwc", lambda c: (src, dst, 1, 3, 8, c), [dst], CODE[dt])
    _exact("gate u8_to_nhwc", _result(dst, (8,)), np.concatenate([_unit(px, dt), np.zeros(5, NP[dt])]))
    img = np.array([[[10, 20, 30], [40, 50, 60]], [[70, 80, 90], [100, 110, 121]]], dtype=np.uint8)
    src, dst, u8 = _in(img, torch.uint8, "src"), _out((8,), dt, "dst"), _out((3,), torch.uint8, "u8_out")
    _dtype_gate("mu_resize_u8_nhwc", lambda c: (src, 1, 2, 2, 3, 0, dst, u8, 1, 1, 8, c), [dst, u8], CODE[dt])
    want = cv2_resize_oracle.resize_linear_u8(img, (1, 1)).reshape(3)
    assert want.tolist() == [55, 65, 75]                      # (a + b + c + d + 2) >> 2
    _exact("gate resize u8_out", _result(u8, (3,)), want)
    _exact("gate resize dst", _result(dst, (8,)), np.concatenate([_unit(want, dt), np.zeros(5, NP[dt])]))


@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_prep_qkv(dt):
    C = 32
    gen = np.random.default_rng(506)
    ws = [gen.standard_normal((C, C), dtype=np.float32) for _ in range(3)]
    bs = [gen.standard_normal(C, dtype=np.float32) for _ in range(3)]
    ins = [_in(a, F32, n) for a, n in zip(ws + bs, ("wq", "wk", "wv", "bq", "bk", "bv"))]
    dst, bias = _out((6 * C * C,), dt, "dst"), _out((3 * C,), F32, "bias")
    _dtype_gate("mu_prep_qkv", lambda c: (*ins, dst, bias, c, C), [dst, bias], CODE[dt])
    w = np.concatenate(ws).astype(NP[dt])                      # [3C, C]: the forward block; its transpose is the data-gradient block
    _exact("gate prep_qkv dst", _result(dst, (6 * C * C,)), np.concatenate([w.reshape(-1), w.T.reshape(-1)]))
    _exact("gate prep_qkv bias", _result(bias, (3 * C,)), np.concatenate(bs))


PAIRS = [(F32, F32), (F32, F16), (F16, F32), (F16, F16)]


@pytest.mark.parametrize("R_,C_", [(1, 4), (3, 5)], ids=["1x4-vector", "3x5-scalar"])
def test_dtype_gate_transpose_and_cast(R_, C_):
    """1 x 4 with every pointer and leading dimension a multiple of four elements: the vector kernel; 3 x 5 with src_ld = 5: the scalar
    one.  All four (source, destination) pairs, and a bad member on either side of a pair."""
    Rp = (R_ + 3) // 4 * 4 if C_ % 4 == 0 else R_
    gen = np.random.default_rng(507 + R_)
    for sdt, ddt in PAIRS:
        x = _normal(gen, (R_, C_), sdt, 4.0)
        src = _in(x, sdt, "src")
        dst = _out((C_, Rp), ddt, "dst")
        bad = [(b, CODE[ddt]) for b in (MU_F32X, BAD_DTYPE)] + [(CODE[sdt], b) for b in (MU_F32X, BAD_DTYPE)]
        for s, d in bad:
            _refused("MU_ERR_ARG", "mu_transpose_pad", src, s, C_, dst, d, Rp, 1, R_, C_, Rp, outs=[dst])
        call("mu_transpose_pad", src, CODE[sdt], C_, dst, CODE[ddt], Rp, 1, R_, C_, Rp)
        ref = np.zeros((C_, Rp), dtype=NP[ddt])
        ref[:, :R_] = x.T.astype(np.float32).astype(NP[ddt])
        _exact(f"gate transpose_pad {R_}x{C_} {sdt}->{ddt}", _result(dst, (C_, Rp)), ref)
        if Rp == R_:
            dst = _out((C_, R_), ddt, "dst")
            for s, d in bad:
                _refused("MU_ERR_ARG", "mu_transpose", src, s, C_, dst, d, R_, 1, R_, C_, outs=[dst])
            call("mu_transpose", src, CODE[sdt], C_, dst, CODE[ddt], R_, 1, R_, C_)
            _exact(f"gate transpose {R_}x{C_} {sdt}->{ddt}", _result(dst, (C_, R_)), ref)
        n = R_ * C_
        out = _out((n,), ddt, "dst")
        for s, d in bad:
            _refused("MU_ERR_ARG", "mu_cast", src, s, out, d, n, outs=[out])
        _refused("MU_ERR_ARG", "mu_cast", None, BAD_DTYPE, out, CODE[ddt], n, outs=[out])
        call("mu_cast", src, CODE[sdt], out, CODE[ddt], n)
        _exact(f"gate cast n={n} {sdt}->{ddt}", _result(out, (n,)), x.reshape(-1).astype(np.float32).astype(NP[ddt]))


# ================================================================================================
# mu_prep_weight / mu_prep_weights_multi: OIHW fp32 -> [tap][rows_pad][cols_pad]; these two take MU_F32X (operands encoded in place)
#   forward        dst[t][o][i]     = w[o][i][t]
#   data gradient  dst[T-1-t][i][o] = w[o][i][t]
# MU_F32X, 9 taps: the forward block as 16-byte chunks [4 fp16 hi | 4 fp16 lo] of 64 w, the data-gradient block as rows
# [rows_pad fp16 lo | rows_pad fp16 hi] of 64 w; hi = fp16(64 w), lo = fp16(64 w - hi).
# ================================================================================================
def _prep_ref(w, mode):
    O, I, T = w.shape
    return np.ascontiguousarray(w.transpose(2, 0, 1) if mode == 0 else w[:, :, ::-1].transpose(2, 1, 0))


def _hi_lo(v):
    s = v.astype(np.float32) * np.float32(64)
    hi = s.astype(np.float16)
    return hi, (s - hi.astype(np.float32)).astype(np.float16)


def _weights_4x4(seed):
    """multiples of 1/8 plus, in half of the places, 2^-12: 64 w then needs a lo half (2^-6, a normal fp16)"""
    gen = np.random.default_rng(seed)
    w = gen.integers(-16, 17, (4, 4, 9)).astype(np.float32) / np.float32(8)
    return w + gen.integers(0, 2, w.shape).astype(np.float32) * np.float32(2.0 ** -12)


@pytest.mark.parametrize("dt", DTYPES)
def test_dtype_gate_prep_weight(dt):
    w = _weights_4x4(508)
    wg = _in(w, F32, "w")
    for mode in (0, 1, 2):
        dst = _out((9 * 16 * (2 if mode == 2 else 1),), dt, "dst")
        _dtype_gate("mu_prep_weight", lambda c: (wg, dst, c, 4, 4, 9, 4, 4, mode), [dst], CODE[dt], bad=(BAD_DTYPE,))
        ref = np.concatenate([_prep_ref(w, m).reshape(-1) for m in ((0, 1) if mode == 2 else (mode,))]).astype(NP[dt])
        _exact(f"gate prep_weight mode {mode}", _result(dst, ref.shape), ref)
    # the many-layers form: one job, one 32 x 32 tile
    jobs = np.array([wg.p, 0, 0, 4, 4, 9, 32, 32, 0, 0], dtype=np.int64)
    jg, dst = _in(jobs, torch.int64, "jobs"), _out((9 * 32 * 32,), dt, "dst")
    _dtype_gate("mu_prep_weights_multi", lambda c: (jg, 1, 1, dst, c), [dst], CODE[dt], bad=(BAD_DTYPE,))
    ref = np.zeros((9, 32, 32), dtype=NP[dt])
    ref[:, :4, :4] = _prep_ref(w, 0)
    _exact("gate prep_weights_multi", _result(dst, ref.shape), ref)


def test_prep_weight_fp32x_encodes_in_place():
    w = _weights_4x4(509)
    wg = _in(w, F32, "w")
    hi0, lo0 = _hi_lo(_prep_ref(w, 0).reshape(-1, 4))          # chunks of four along the input channels
    hi1, lo1 = _hi_lo(_prep_ref(w, 1).reshape(-1, 4))          # rows of rows_pad = 4 output channels
    assert (lo0 != 0).any() and (lo1 != 0).any()
    fwd, dgrad = np.concatenate([hi0, lo0], axis=1).reshape(-1), np.concatenate([lo1, hi1], axis=1).reshape(-1)
    for mode, ref in ((0, fwd), (2, np.concatenate([fwd, dgrad]))):
        dst = _out((ref.size // 2,), F32, "dst")
        call("mu_prep_weight", wg, dst, MU_F32X, 4, 4, 9, 4, 4, mode)
        got = dst.host().view(np.float16)
        _exact(f"prep_weight fp32x mode {mode}", got, ref)


def test_prep_weight_fp32x_refuses_before_it_launches():
    """rows_pad or cols_pad no multiple of four, and a data-gradient row longer than 8192: MU_ERR_SHAPE with dst untouched"""
    wg = _in(_weights_4x4(510), F32, "w")
    for rp, cp in ((6, 4), (4, 6)):
        dst = _out((9 * rp * cp,), F32, "dst")
        _refused("MU_ERR_SHAPE", "mu_prep_weight", wg, dst, MU_F32X, 4, 4, 9, rp, cp, 0, outs=[dst])
    w1 = _in(np.ones((1, 1, 9), dtype=np.float32), F32, "w")
    dst = _out((9 * 4 * 8196,), F32, "dst")
    _refused("MU_ERR_SHAPE", "mu_prep_weight", w1, dst, MU_F32X, 1, 1, 9, 4, 8196, 1, outs=[dst])
