"""maskunet_amd/csrc/norm.hip against tests/_norm_reference.py (float64) through the C ABI at every reduction and grid edge: BatchNorm
statistics (from the tensor, from statistics rows, eval), apply, backward (plain, scaled, pair, the fp16-scaled dx forms), the pair
composition, column sums and the per-sample LayerNorm.  Every tensor operand sits in a tests/_device_buffers.Guarded buffer: after each
call the guard bands are intact, the inputs unchanged, outputs wholly written, and with ld > C the columns C..ld still hold the
sentinel.  Every bound is derived in the docstrings of tests/_norm_reference.py; every test prints its worst error next to its bound
(pytest -s / -rP).  The input recipes are plain numpy functions; tests/test_norm_reference_host.py checks on the CPU that they meet
their own conditions."""
import math

import numpy as np
import pytest
import torch

from tests import _norm_reference as R
from tests._device_buffers import Guarded

pytestmark = pytest.mark.gpu

MU_F32, MU_F16, MU_F32X = 0, 1, 2
NONE, GELU, RELU = R.ACT_NONE, R.ACT_GELU, R.ACT_RELU
ACT_NAME = {NONE: "none", GELU: "gelu", RELU: "relu"}
TORCH = {"f32": torch.float32, "f16": torch.float16}
NP = {"f32": np.float32, "f16": np.float16}
CODE = {"f32": MU_F32, "f16": MU_F16}
NVEC = {"f32": 4, "f16": 8}                 # elements per 16-byte vector
EPS = 1e-5
NAN = float("nan")
U = R.U


# ================================================================================================
# plumbing
# ================================================================================================
def _note(what, err, bound):
    print(f"norm-edges {what}: worst {err:.3e} bound {bound:.3e} ratio {err / bound if bound else float('nan'):.3f}")


def _check(what, err, bound):
    """every element within its bound (a NaN anywhere fails); prints the worst err / bound and the values there"""
    err, bound = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    assert err.size, what
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    assert not np.isnan(ratio).any(), (what, "nan")
    i = int(np.argmax(ratio))
    _note(what, float(err.flat[i]), float(bound.flat[i]))
    assert ratio.flat[i] <= 1.0, (what, float(err.flat[i]), float(bound.flat[i]), np.unravel_index(i, err.shape))


def _in(a, dtype, name):
    a = np.ascontiguousarray(a)
    return Guarded(a.size, dtype, data=a, name=name)


def _out(n, dtype, name):
    return Guarded(int(n), dtype, name=name)


def _inout(a, dtype, name):
    """an operand the kernel updates: starts as `a`, no 'unchanged' check"""
    a = np.ascontiguousarray(a)
    g = Guarded(a.size, dtype, name=name)
    g.t.copy_(torch.as_tensor(a).reshape(-1).to(g.t.device))
    return g


def _counter(v):
    """a long on the device: 8 bytes of a uint8 buffer (the guard bands keep it 4 KiB aligned)"""
    return _inout(np.array([v], dtype=np.int64).view(np.uint8), torch.uint8, "num_batches_tracked")


def _counter_value(g):
    return int(g.host().view(np.int64)[0])


def _ptr(a, offset_bytes=0):
    return (a.p + offset_bytes) if isinstance(a, Guarded) else a


def _call(name, *args):
    from maskunet_amd import _lib
    _lib.call(name, *[_ptr(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Guarded):
            a.check()


def _untouched(g):
    return bool((g.t == g.sent).all())


def _refused(code, name, *args, outs=()):
    """the entry point returns `code` before it launches anything: every output still holds the sentinel"""
    from maskunet_amd import _lib
    with pytest.raises(RuntimeError, match=code):
        _lib.call(name, *[_ptr(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    for a in list(args) + list(outs):
        if isinstance(a, Guarded):
            a.check()
    for o in outs:
        assert _untouched(o), (name, code, o.name)


def _bn_ws(C):
    from maskunet_amd import _lib
    n = _lib.load().mu_bn_workspace_bytes(C)
    return _out(n, torch.uint8, "workspace"), n


def _pad(a, ld, fill=NAN):
    """[M, C] -> [M, ld]; the columns C..ld of an INPUT are NaN: a kernel that reads them poisons its result"""
    M, C = a.shape
    if ld == C:
        return a
    o = np.full((M, ld), fill, dtype=a.dtype)
    o[:, :C] = a
    return o


def _rows(g, M, C, ld, what):
    """an output of M rows of C elements at row stride ld: wholly written, and the columns C..ld still the sentinel"""
    t = g.host((M, ld))
    assert not (t[:, :C] == g.sent).any(), f"{what}: not every element was written"
    assert (t[:, C:] == g.sent).all(), f"{what}: columns C..ld were written"
    return t[:, :C].astype(np.float64)


def _vec(g, what=None):
    g.all_written(what)
    return g.host().astype(np.float64)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def _st(storage, a):
    """float32 draw -> the storage type (numpy array of that type)"""
    return np.asarray(a, dtype=np.float32).astype(NP[storage])


# ================================================================================================
# shapes
# ================================================================================================
def rpi_of(C, storage):
    return 256 // (C // NVEC[storage])


def wide_C(storage):
    return 1024 if storage == "f32" else 2048          # cv = 256, rpi = 1


def stat_M_edges(C, storage, Uf=8):
    r = rpi_of(C, storage)
    return sorted({1, 31, 32, 33, Uf * r - 1, Uf * r, Uf * r + 1, 2 * Uf * r + 1} - {0})


def bwd_M_edges(C, storage):
    r = rpi_of(C, storage)
    return sorted({1, 2, 2 * r - 1, 2 * r, 2 * r + 1} - {0})


STAT_BIG_M = [2016, 2048, 2080, 32767, 32768, 32769, 40000]       # C = 8: nblk = 63, 64, 65, 1023, 1024, 1024, capped
BWD_BIG_M = [24544, 24576, 24608, 32768, 40000]                  # C = 8: nblk = 767, 768, capped


def _id(storage, *k):
    return "-".join([storage] + [str(v) for v in k])


STAT_CASES = [pytest.param(s, C, M, id=_id(s, C, M)) for s in ("f32", "f16") for C in (8, 24, 40, 152, wide_C(s))
              for M in stat_M_edges(C, s) + (STAT_BIG_M if C == 8 else [])]


# ================================================================================================
# statistics: mu_bn_train_stats
# ================================================================================================
def stats_inputs(storage, C, M, r=None):
    """x [M, C] in the storage type.  r = None: randn * 1.5 + 0.3; otherwise randn + r with channel 3 constant (variance 0)."""
    g = _rng(1, C, M, 0 if r is None else r + 1)
    if r is None:
        x = g.standard_normal((M, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    else:
        x = g.standard_normal((M, C), dtype=np.float32) + np.float32(r)
        x[:, 3] = np.float32(r + 0.7)
    return _st(storage, x), g.standard_normal(C).astype(np.float32), (g.random(C) + 0.5).astype(np.float32)


def _train_stats(storage, x, ld, c_valid, momentum, rm0, rv0, nbt0):
    """one call; rm0 / nbt0 None = NULL operands.  Returns (mean, rstd, running_mean, running_var, counter) as float64 / int."""
    M, C = x.shape
    X = _in(_pad(x, ld), TORCH[storage], "x")
    mean, rstd = _out(C, torch.float32, "mean"), _out(C, torch.float32, "rstd")
    rm = None if rm0 is None else _inout(rm0, torch.float32, "running_mean")
    rv = None if rm0 is None else _inout(rv0, torch.float32, "running_var")
    nbt = None if nbt0 is None else _counter(nbt0)
    ws, n = _bn_ws(C)
    _call("mu_bn_train_stats", X, M, C, ld, mean, rstd, rm, rv, nbt, c_valid, momentum, EPS, ws, n, CODE[storage])
    return (_vec(mean), _vec(rstd), None if rm is None else rm.host().copy(), None if rv is None else rv.host().copy(),
            None if nbt is None else _counter_value(nbt))


def _compare_stats(what, got, ref, bounds, rm0, rv0, c_valid, nbt0):
    mean, rstd, rm, rv, nbt = got
    _check(what + " mean", np.abs(mean - ref["mean"]), bounds["mean"])
    _check(what + " rstd", np.abs(rstd - ref["rstd"]), bounds["rstd"])
    if rm is not None:
        _check(what + " running_mean", np.abs(rm[:c_valid] - ref["running_mean"][:c_valid]), bounds["running_mean"][:c_valid])
        _check(what + " running_var", np.abs(rv[:c_valid] - ref["running_var"][:c_valid]), bounds["running_var"][:c_valid])
        assert rm[c_valid:].tobytes() == rm0[c_valid:].tobytes() and rv[c_valid:].tobytes() == rv0[c_valid:].tobytes(), \
            what + ": running statistics at and beyond c_valid moved"
    if nbt0 is not None:
        assert nbt == nbt0 + 1, (what, nbt, nbt0)


@pytest.mark.parametrize("storage,C,M", STAT_CASES)
def test_bn_train_stats(storage, C, M):
    """row lanes that do not fill the block, the widest rows, the chunk tails of U * rpi rows, the block count and its cap; ld = C and
    C + 8; c_valid = C and C - 2 (150 of 152); NULL running operands and a NULL counter"""
    x, rm0, rv0 = stats_inputs(storage, C, M)
    for ld, c_valid, running, nbt0 in ((C, C, True, 5), (C + 8, C - 2, True, None), (C, C - 2, False, (1 << 40) + 7)):
        ref = R.bn_stats(x, EPS, 0.1, rm0 if running else None, rv0 if running else None, c_valid)
        got = _train_stats(storage, x, ld, c_valid, 0.1, rm0 if running else None, rv0, nbt0)
        _compare_stats(f"train_stats {storage} C={C} M={M} ld={ld}", got, ref, R.bn_stats_bounds(ref, EPS, 0.1), rm0, rv0, c_valid, nbt0)


RATIO_CASES = [pytest.param(s, C, r, id=_id(s, C, f"r{r}")) for s, rs in (("f32", (0, 30, 300)), ("f16", (0, 30))) for C in (8, 152) for r in rs]


@pytest.mark.parametrize("storage,C,r", RATIO_CASES)
def test_bn_train_stats_mean_to_std_ratio(storage, C, r):
    """x = randn + r, one channel constant.  The fp32 short sums round relative to E[x^2]: the biased variance is held to 24 u E[x^2]
    (tests/_norm_reference.py bn_stats_bounds), read back through running_var at momentum 1 (= var M / (M - 1), one store)."""
    M = 4096
    x, rm0, rv0 = stats_inputs(storage, C, M, r)
    ref = R.bn_stats(x, EPS, 1.0, rm0, rv0, C)
    b = R.bn_stats_bounds(ref, EPS, 1.0)
    got = _train_stats(storage, x, C, C, 1.0, rm0, rv0, 0)
    what = f"train_stats ratio {storage} C={C} r={r}"
    _compare_stats(what, got, ref, b, rm0, rv0, C, 0)
    var_dev = got[3].astype(np.float64) * ((M - 1.0) / M)
    err = np.abs(var_dev - ref["var"])
    _check(what + " var", err, b["var"] + U * ref["var"])
    live = ref["var"] > 0.5
    print(f"norm-edges variance-by-ratio {storage} C={C} r={r}: worst relative error of the variance {float((err[live] / ref['var'][live]).max()):.3e}"
          f" (constant channel: var {float(var_dev[3]):.3e}, rstd {float(got[1][3]):.6g} of {float(ref['rstd'][3]):.6g})")
    assert ref["var"][3] == 0.0 and abs(ref["rstd"][3] - 1.0 / math.sqrt(float(np.float32(EPS)))) < 1e-9


def test_bn_train_stats_refusals():
    from maskunet_amd import _lib
    x, _, _ = stats_inputs("f32", 8, 4)
    X = _in(x, torch.float32, "x")
    mean, rstd = _out(8, torch.float32, "mean"), _out(8, torch.float32, "rstd")
    ws, n = _bn_ws(16)
    outs = (mean, rstd)
    tail = (None, None, None, 8, 0.1, EPS)
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 4, 12, 12, mean, rstd, *tail, ws, n, MU_F32, outs=outs)          # C % 8
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 4, 8, 7, mean, rstd, *tail, ws, n, MU_F32, outs=outs)            # ld < C
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 0, 8, 8, mean, rstd, *tail, ws, n, MU_F32, outs=outs)            # M = 0
    _refused("MU_ERR_ARG", "mu_bn_train_stats", None, 4, 8, 8, mean, rstd, *tail, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 4, 8, 8, None, rstd, *tail, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 4, 8, 8, mean, None, *tail, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 4, 8, 8, mean, rstd, *tail, None, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats", X, 4, 8, 8, mean, rstd, *tail, ws, n, MU_F32X, outs=outs)           # no such dtype here
    _refused("MU_ERR_WORKSPACE", "mu_bn_train_stats", X, 4, 8, 8, mean, rstd, *tail, ws, _lib.load().mu_bn_workspace_bytes(8) - 1, MU_F32, outs=outs)
    for storage, C in (("f32", 1032), ("f16", 2056)):                                                               # cv = 257
        xw = _in(np.zeros((2, C), dtype=NP[storage]), TORCH[storage], "x")
        mw, rw = _out(C, torch.float32, "mean"), _out(C, torch.float32, "rstd")
        wsw, nw = _bn_ws(C)
        _refused("MU_ERR_SHAPE", "mu_bn_train_stats", xw, 2, C, C, mw, rw, None, None, None, C, 0.1, EPS, wsw, nw, CODE[storage], outs=(mw, rw))


@pytest.mark.parametrize("C,c_valid", [(8, 8), (19, 17), (152, 150), (1, 1)])
def test_bn_eval_stats(C, c_valid):
    g = _rng(2, C)
    rm0, rv0 = g.standard_normal(C).astype(np.float32), (g.random(C) * 2).astype(np.float32)
    rv0[0] = 0.0
    rm, rv = _in(rm0, torch.float32, "running_mean"), _in(rv0, torch.float32, "running_var")
    mean, rstd = _out(C, torch.float32, "mean"), _out(C, torch.float32, "rstd")
    _call("mu_bn_eval_stats", rm, rv, EPS, mean, rstd, C, c_valid)
    m_ref, r_ref = R.bn_eval_stats(rm0, rv0, EPS, c_valid)
    assert np.array_equal(_vec(mean), m_ref)                                   # a copy, and exact zeros in the padding
    _check(f"eval_stats C={C} rstd", np.abs(_vec(rstd) - r_ref), 8 * U * r_ref)
    assert np.all(_vec(rstd)[c_valid:] == 1.0)
    o1, o2 = _out(C, torch.float32, "mean"), _out(C, torch.float32, "rstd")
    _refused("MU_ERR_ARG", "mu_bn_eval_stats", None, rv, EPS, o1, o2, C, c_valid, outs=(o1, o2))
    _refused("MU_ERR_ARG", "mu_bn_eval_stats", rm, rv, EPS, o1, o2, 0, 0, outs=(o1, o2))


@pytest.mark.parametrize("C,c_valid,two", [(8, 8, False), (19, 17, True), (152, 150, True)])
def test_bn_eval_fold(C, c_valid, two):
    g = _rng(3, C)
    f = lambda s=1.0: (g.standard_normal(C) * s).astype(np.float32)
    rm1, rv1, g1, b1, cb = f(), (g.random(C) + 0.1).astype(np.float32), f(), f(), f()
    rm2, rv2, g2, b2 = f(), (g.random(C) + 0.1).astype(np.float32), f(), f()
    for nulls in (False, True):
        ops1 = [None if nulls else a for a in (g1, b1)]
        ops2 = [a if two else None for a in (rm2, rv2)] + [a if (two and not nulls) else None for a in (g2, b2)]
        bias = None if nulls else cb
        G = lambda a, n: None if a is None else _in(a, torch.float32, n)
        scale, shift = _out(C, torch.float32, "scale"), _out(C, torch.float32, "shift")
        _call("mu_bn_eval_fold", G(rm1, "rm1"), G(rv1, "rv1"), G(ops1[0], "g1"), G(ops1[1], "b1"), 1e-5, G(ops2[0], "rm2"), G(ops2[1], "rv2"),
              G(ops2[2], "g2"), G(ops2[3], "b2"), 0.3, G(bias, "bias"), scale, shift, C, c_valid)
        a_ref, s_ref, mag = R.bn_eval_fold(rm1, rv1, ops1[0], ops1[1], 1e-5, ops2[0], ops2[1], ops2[2], ops2[3], 0.3, bias, c_valid)
        _check(f"eval_fold C={C} scale", np.abs(_vec(scale) - a_ref), 16 * U * np.abs(a_ref))
        _check(f"eval_fold C={C} shift", np.abs(_vec(shift) - s_ref), 16 * U * mag)
        assert not _vec(scale)[c_valid:].any() and not _vec(shift)[c_valid:].any()


# ================================================================================================
# statistics from rows: mu_bn_train_stats_rows
# ================================================================================================
def rows_inputs(rows, C):
    """a float32 [rows * 3, C] matrix and its per-row-group (sum, sum of squares), summed in float64 and rounded to float32"""
    g = _rng(4, rows, C)
    x = g.standard_normal((rows * 3, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    xd = x.astype(np.float64).reshape(rows, 3, C)
    part = np.stack([xd.sum(1), (xd * xd).sum(1)], axis=-1).astype(np.float32)          # [rows, C, 2]
    return part, g.standard_normal(C).astype(np.float32), (g.random(C) + 0.5).astype(np.float32)


@pytest.mark.parametrize("C", [8, 19, 152])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1024, 1025, 16384, 16385, 20000])
def test_bn_train_stats_rows(rows, C):
    """the three paths: rows <= 1024 read as floats by the finalize kernel, 16 rows per fold block up to 16384 rows, a wider rpb beyond"""
    part, rm0, rv0 = rows_inputs(rows, C)
    M, c_valid = rows * 3, max(C - 2, 1)
    ref = R.bn_stats_from_rows(part, M, EPS, 0.1, rm0, rv0, c_valid)
    P = _in(part, torch.float32, "stat_part")
    mean, rstd = _out(C, torch.float32, "mean"), _out(C, torch.float32, "rstd")
    rm, rv, nbt = _inout(rm0, torch.float32, "running_mean"), _inout(rv0, torch.float32, "running_var"), _counter(41)
    ws, n = _bn_ws(C)
    _call("mu_bn_train_stats_rows", P, rows, M, C, mean, rstd, rm, rv, nbt, c_valid, 0.1, EPS, ws, n)
    got = (_vec(mean), _vec(rstd), rm.host().copy(), rv.host().copy(), _counter_value(nbt))
    _compare_stats(f"stats_rows rows={rows} C={C}", got, ref, R.tight_stats_bounds(ref, 0.1), rm0, rv0, c_valid, 41)


def test_bn_train_stats_rows_refusals():
    from maskunet_amd import _lib
    part, _, _ = rows_inputs(4, 8)
    P = _in(part, torch.float32, "stat_part")
    mean, rstd = _out(8, torch.float32, "mean"), _out(8, torch.float32, "rstd")
    ws, n = _bn_ws(8)
    outs = (mean, rstd)
    _refused("MU_ERR_ARG", "mu_bn_train_stats_rows", None, 4, 12, 8, mean, rstd, None, None, None, 8, 0.1, EPS, ws, n, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats_rows", P, 0, 12, 8, mean, rstd, None, None, None, 8, 0.1, EPS, ws, n, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats_rows", P, 4, 0, 8, mean, rstd, None, None, None, 8, 0.1, EPS, ws, n, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_train_stats_rows", P, 4, 12, 8, mean, rstd, None, None, None, 8, 0.1, EPS, None, n, outs=outs)
    _refused("MU_ERR_WORKSPACE", "mu_bn_train_stats_rows", P, 4, 12, 8, mean, rstd, None, None, None, 8, 0.1, EPS, ws, n - 1, outs=outs)


# ================================================================================================
# apply: mu_bn_act_fwd, mu_bn_act_fwd_enc
# ================================================================================================
GELU_SPECIALS = np.array([4.24, -4.24, 4.26, -4.26, 30.0, -30.0, 0.0, -0.0], dtype=np.float32)
SPECIAL_CH = 2                                  # mean 0, rstd 1, gamma 1, beta 0, residual 0: pre = x exactly


def channel_operands(g, C):
    """mean, rstd, gamma, beta drawn directly; gamma[0] = 0, gamma[1] < 0, channel 2 the identity"""
    mean = (g.standard_normal(C) * 0.5).astype(np.float32)
    rstd = (g.random(C) * 1.7 + 0.3).astype(np.float32)
    gamma = (g.standard_normal(C) * 0.5 + 1.0).astype(np.float32)
    beta = (g.standard_normal(C) * 0.5).astype(np.float32)
    gamma[0], gamma[1] = 0.0, -1.3
    mean[SPECIAL_CH], rstd[SPECIAL_CH], gamma[SPECIAL_CH], beta[SPECIAL_CH] = 0.0, 1.0, 1.0, 0.0
    return mean, rstd, gamma, beta


def fwd_inputs(storage, C, M):
    g = _rng(5, C, M, NVEC[storage])
    x = g.standard_normal((M, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3)
    res = g.standard_normal((M, C), dtype=np.float32)
    k = min(M, len(GELU_SPECIALS))
    x[:k, SPECIAL_CH] = GELU_SPECIALS[:k]
    res[:k, SPECIAL_CH] = 0.0
    return (_st(storage, x), _st(storage, res)) + channel_operands(g, C)


def fwd_M_set(C, nvec):
    cv = C // nvec
    s = {1, 7, 1025}
    for k in (1024, 2048):                      # M * cv below, at / just above, and above 1024 g: the U-loop tail idx + u * stride < total
        s |= {(k - 1) // cv, -(-k // cv), k // cv + 1}
    return sorted(s - {0})


FWD_CASES = [pytest.param(mode, C, M, id=_id(mode, C, M)) for mode in ("f32", "f16", "f32x") for C in (8, 24, 152, 1024)
             for M in fwd_M_set(C, 8 if mode == "f16" else 4)]


def _encode_h4(y_rows):
    """mu_split_encode_h4 of a float32 [M, ld] matrix on the device -> int32 bits [M, ld]"""
    from maskunet_amd import _lib
    src = torch.from_numpy(np.ascontiguousarray(y_rows, dtype=np.float32)).cuda()
    dst = torch.empty_like(src)
    _lib.call("mu_split_encode_h4", src.data_ptr(), dst.data_ptr(), src.numel(), _lib.stream())
    torch.cuda.synchronize()
    return dst.view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("mode,C,M", FWD_CASES)
def test_bn_act_fwd(mode, C, M):
    """all three activations with and without a residual, ld = C and C + 8.  f32x: the encoded output equals mu_split_encode_h4 of the
    plain fp32 output bit for bit (and mu_bn_act_fwd_enc's y16 its .half())"""
    storage = "f16" if mode == "f16" else "f32"
    x, res, mean, rstd, gamma, beta = fwd_inputs(storage, C, M)
    ops = [_in(a, torch.float32, n) for a, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"))]
    T = TORCH[storage]
    refs = {}
    for ld in (C, C + 8):
        X, RES = _in(_pad(x, ld), T, "x"), _in(_pad(res, ld), T, "res")
        for a in (NONE, GELU, RELU):
            for use_res in (False, True):
                what = f"bn_act_fwd {mode} C={C} M={M} ld={ld} {ACT_NAME[a]}{'+res' if use_res else ''}"
                if (a, use_res) not in refs:
                    y_ref, pre = R.bn_act_fwd(x, res if use_res else None, mean, rstd, gamma, beta, a)
                    refs[a, use_res] = (y_ref, R.bn_act_fwd_bound(x, res if use_res else None, mean, rstd, gamma, beta, a, y_ref, pre, storage))
                y_ref, bound = refs[a, use_res]
                y = _out(M * ld, T, "y")
                _call("mu_bn_act_fwd", X, RES if use_res else None, y, M, C, ld, *ops, a, CODE[storage])
                got = _rows(y, M, C, ld, what)
                _check(what, np.abs(got - y_ref), bound)
                if mode != "f32x":
                    continue
                want = _encode_h4(y.host((M, ld)))[:, :C]
                ye = _out(M * ld, T, "y_enc")
                _call("mu_bn_act_fwd", X, RES if use_res else None, ye, M, C, ld, *ops, a, MU_F32X)
                _rows(ye, M, C, ld, what + " enc")
                assert np.array_equal(ye.host((M, ld)).view(np.int32)[:, :C], want), what + ": encoded output"
                if ld == C:
                    y2, y16 = _out(M * C, T, "y_enc"), _out(M * C, torch.float16, "y16")
                    _call("mu_bn_act_fwd_enc", X, RES if use_res else None, y2, y16, M, C, *ops, a)
                    y16.all_written()
                    assert np.array_equal(y2.host().view(np.int32), want.reshape(-1)), what + ": mu_bn_act_fwd_enc"
                    assert y16.host().tobytes() == y.host().astype(np.float16).tobytes(), what + ": y16"


def test_bn_act_fwd_refusals():
    x, res, mean, rstd, gamma, beta = fwd_inputs("f32", 8, 4)
    X = _in(x, torch.float32, "x")
    ops = [_in(a, torch.float32, n) for a, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"))]
    y, y16 = _out(32, torch.float32, "y"), _out(32, torch.float16, "y16")
    _refused("MU_ERR_ARG", "mu_bn_act_fwd", X, None, y, 4, 12, 12, *ops, NONE, MU_F32, outs=(y,))
    _refused("MU_ERR_ARG", "mu_bn_act_fwd", X, None, y, 4, 8, 7, *ops, NONE, MU_F32, outs=(y,))
    _refused("MU_ERR_ARG", "mu_bn_act_fwd", X, None, y, 0, 8, 8, *ops, NONE, MU_F32, outs=(y,))
    _refused("MU_ERR_ARG", "mu_bn_act_fwd", X, None, y, 4, 8, 8, *ops, 3, MU_F32, outs=(y,))                      # no such activation
    _refused("MU_ERR_ARG", "mu_bn_act_fwd", X, None, y, 4, 8, 8, *ops, NONE, 7, outs=(y,))                        # no such dtype
    _refused("MU_ERR_ARG", "mu_bn_act_fwd", X, None, y, 4, 8, 8, ops[0], None, ops[2], ops[3], NONE, MU_F32, outs=(y,))
    _refused("MU_ERR_ARG", "mu_bn_act_fwd_enc", X, None, y, None, 4, 8, *ops, NONE, outs=(y, y16))
    _refused("MU_ERR_ARG", "mu_bn_act_fwd_enc", X, None, y, y16, 4, 12, *ops, NONE, outs=(y, y16))


# ================================================================================================
# backward: mu_bn_act_bwd, mu_bn_act_bwd_scaled
# ================================================================================================
def bwd_inputs(storage, C, M, a, use_res, gmag=1.0, seed=0):
    """x, res, g in the storage type; mean / rstd the float32-rounded batch statistics of the drawn x; gamma[0] = 0, gamma[1] < 0.
    ReLU: x is moved wherever the pre-activation lies within its rounding margin of 0 (R.relu_margin), until none does (where
    gamma = 0 the residual is moved instead)."""
    g = _rng(6, C, M, a, int(use_res), NVEC[storage], seed)
    x = _st(storage, g.standard_normal((M, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3))
    res = _st(storage, g.standard_normal((M, C), dtype=np.float32)) if use_res else None
    go = _st(storage, g.standard_normal((M, C), dtype=np.float32) * np.float32(gmag))
    st = R.bn_stats(x, EPS)
    mean, rstd = st["mean"].astype(np.float32), st["rstd"].astype(np.float32)
    gamma = (g.standard_normal(C) * 0.5 + 1.0).astype(np.float32)
    beta = (g.standard_normal(C) * 0.5).astype(np.float32)
    gamma[0], gamma[1] = 0.0, -1.3
    if a == RELU:
        for _ in range(40):
            p, m = R.relu_margin(x, res, mean, rstd, gamma, beta, storage)
            bad = p < m
            if not bad.any():
                break
            # 0.4375 of a standard deviation, and at least a few ulps of the storage type (M = 1 or 2: rstd is up to 1 / sqrt(eps))
            xf = x.astype(np.float32)
            step = np.maximum(np.float32(0.4375) / rstd, np.float32(2.0 ** -8) * np.maximum(np.abs(xf), np.float32(1.0)))
            x = _st(storage, np.where(bad, xf + step, xf))
            if res is not None:                          # where gamma = 0 the pre-activation does not depend on x: the residual moves
                res = _st(storage, np.where(bad & (gamma == 0), res.astype(np.float32) + np.float32(0.4375), res.astype(np.float32)))
    return x, res, go, mean, rstd, gamma, beta


def relu_margin_ok(storage, x, res, mean, rstd, gamma, beta):
    p, m = R.relu_margin(x, res, mean, rstd, gamma, beta, storage)
    return not bool((p < m).any())


def _bwd_call(storage, x, res, go, mean, rstd, gamma, beta, a, training, xs, ld):
    """mu_bn_act_bwd (xs None) or mu_bn_act_bwd_scaled; returns dx, dres (or None), dgamma, dbeta as float64"""
    M, C = x.shape
    T = TORCH[storage]
    X, G = _in(_pad(x, ld), T, "x"), _in(_pad(go, ld), T, "grad_out")
    RES = None if res is None else _in(_pad(res, ld), T, "res")
    ops = [_in(v, torch.float32, n) for v, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"))]
    dx = _out(M * ld, T, "dx")
    dres = None if res is None else _out(M * ld, T, "dres")
    dg, db = _out(C, torch.float32, "dgamma"), _out(C, torch.float32, "dbeta")
    ws, n = _bn_ws(C)
    if xs is None:
        _call("mu_bn_act_bwd", X, RES, G, dx, dres, M, C, ld, *ops, a, training, dg, db, ws, n, CODE[storage])
    else:
        _call("mu_bn_act_bwd_scaled", X, RES, G, dx, dres, M, C, ld, *ops, a, training, dg, db, _in(xs, torch.float32, "xhat_scale"), ws, n, CODE[storage])
    return _rows(dx, M, C, ld, "dx"), None if res is None else _rows(dres, M, C, ld, "dres"), _vec(dg), _vec(db)


def _compare_bwd(what, got, ref, b):
    dx, dres, dg, db = got
    _check(what + " dbeta", np.abs(db - ref["dbeta"]), b["dbeta"])
    _check(what + " dgamma", np.abs(dg - ref["dgamma"]), b["dgamma"])
    _check(what + " dx", np.abs(dx - ref["dx"]), b["dx"])
    if dres is not None:
        _check(what + " dres", np.abs(dres - ref["dres"]), b["dres"])


BWD_CASES = [pytest.param(s, C, M, a, rs, id=_id(s, C, M, ACT_NAME[a], "res" if rs else "nores"))
             for s in ("f32", "f16") for C in (8, 24, 152, 1024) + ((2048,) if s == "f16" else ())
             for M in bwd_M_edges(C, s) + (BWD_BIG_M if C == 8 else []) for a in (NONE, GELU, RELU) for rs in (False, True)]


@pytest.mark.parametrize("storage,C,M,a,use_res", BWD_CASES)
def test_bn_act_bwd(storage, C, M, a, use_res):
    """every (activation, residual) pair at the chunk tails of 2 * rpi rows and the block cap of 768; training and eval, xhat_scale NULL
    and given, ld = C and C + 8.  Every element is compared: dx, dres, and dgamma / dbeta against the float64 sums."""
    x, res, go, mean, rstd, gamma, beta = bwd_inputs(storage, C, M, a, use_res)
    assert a != RELU or relu_margin_ok(storage, x, res, mean, rstd, gamma, beta)
    xs = (_rng(7, C).random(C) * 1.5 + 0.25).astype(np.float32)
    big = M > 4096
    combos = ((1, None, C), (0, xs, C + 8)) if big else ((1, None, C), (1, xs, C + 8), (0, None, C + 8), (0, xs, C))
    for training, s, ld in combos:
        ref = R.bn_act_bwd(x, res, go, mean, rstd, gamma, beta, a, training, s, storage)
        if not training:                                     # eval: dx = gamma rstd dz, whatever xhat_scale holds
            assert np.array_equal(ref["dx"], ref["gamma"] * ref["rstd"] * ref["dz"])
        got = _bwd_call(storage, x, res, go, mean, rstd, gamma, beta, a, training, s, ld)
        _compare_bwd(f"bn_act_bwd {storage} C={C} M={M} {ACT_NAME[a]}{'+res' if use_res else ''} train={training} xs={s is not None} ld={ld}",
                     got, ref, R.bn_act_bwd_bounds(ref, a, storage))


def test_bn_act_bwd_refusals():
    from maskunet_amd import _lib
    x, res, go, mean, rstd, gamma, beta = bwd_inputs("f32", 8, 4, NONE, True)
    X, G, RES = _in(x, torch.float32, "x"), _in(go, torch.float32, "grad_out"), _in(res, torch.float32, "res")
    ops = [_in(v, torch.float32, n) for v, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"))]
    dx, dres = _out(32, torch.float32, "dx"), _out(32, torch.float32, "dres")
    dg, db = _out(8, torch.float32, "dgamma"), _out(8, torch.float32, "dbeta")
    ws, n = _bn_ws(16)
    outs = (dx, dres, dg, db)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, G, dx, None, 4, 8, 8, *ops, NONE, 1, dg, db, ws, n, MU_F32, outs=outs)      # res without dres
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, None, G, dx, dres, 4, 8, 8, *ops, NONE, 1, dg, db, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, G, dx, dres, 4, 12, 12, *ops, NONE, 1, dg, db, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, G, dx, dres, 4, 8, 7, *ops, NONE, 1, dg, db, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, G, dx, dres, 0, 8, 8, *ops, NONE, 1, dg, db, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, None, dx, dres, 4, 8, 8, *ops, NONE, 1, dg, db, ws, n, MU_F32, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, G, dx, dres, 4, 8, 8, *ops, NONE, 1, dg, db, ws, n, MU_F32X, outs=outs)
    _refused("MU_ERR_WORKSPACE", "mu_bn_act_bwd", X, RES, G, dx, dres, 4, 8, 8, *ops, NONE, 1, dg, db, ws, _lib.load().mu_bn_workspace_bytes(8) - 1, MU_F32, outs=outs)
    sc = _out(2, torch.float32, "dy_scale")
    outs = outs + (sc,)
    _refused("MU_ERR_WORKSPACE", "mu_bn_act_bwd_h", X, RES, G, dx, dres, 4, 8, *ops, NONE, 1, dg, db, sc, ws, 16, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_act_bwd_h", X, RES, G, dx, dres, 4, 8, *ops, NONE, 1, dg, db, None, ws, n, outs=outs)         # no dy_scale
    xw = _in(np.zeros((1, 1032), dtype=np.float32), torch.float32, "x")
    ow = [_in(np.ones(1032, dtype=np.float32), torch.float32, "op") for _ in range(4)]
    dxw, dgw, dbw = _out(1032, torch.float32, "dx"), _out(1032, torch.float32, "dgamma"), _out(1032, torch.float32, "dbeta")
    wsw, nw = _bn_ws(1032)
    _refused("MU_ERR_SHAPE", "mu_bn_act_bwd", xw, None, xw, dxw, None, 1, 1032, 1032, *ow, NONE, 1, dgw, dbw, wsw, nw, MU_F32, outs=(dxw, dgw, dbw))


def test_bn_act_bwd_refusal_precedence():
    """an unknown activation at every backward entry point that takes one, and two faults at once: a short workspace is reported before
    the activation, too many channel vectors before the activation, an unknown dtype and a short workspace at the pair entry points.
    Every output still holds the sentinel; the same buffers with nothing wrong then give the reference's results."""
    M, C, BAD_ACT = 4, 8, 3
    assert BAD_ACT not in (NONE, GELU, RELU)
    ws, n = _bn_ws(C)
    dg, db, sc = _out(C, torch.float32, "dgamma"), _out(C, torch.float32, "dbeta"), _out(2, torch.float32, "dy_scale")
    pg, db2 = _out(3 * C, torch.float32, "pair_grads"), _out(C, torch.float32, "dbeta2")
    for storage in ("f32", "f16"):
        T = TORCH[storage]
        x, res, go, mean, rstd, gamma, beta = bwd_inputs(storage, C, M, NONE, True)
        X, G, RES = _in(x, T, "x"), _in(go, T, "grad_out"), _in(res, T, "res")
        ops = [_in(v, torch.float32, k) for v, k in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"))]
        dx, dres = _out(M * C, T, "dx"), _out(M * C, T, "dres")
        outs = (dx, dres, dg, db, pg, sc)
        _refused("MU_ERR_ARG", "mu_bn_act_bwd", X, RES, G, dx, dres, M, C, C, *ops, BAD_ACT, 1, dg, db, ws, n, CODE[storage], outs=outs)
        if storage == "f32":
            xs = _in(np.ones(C, dtype=np.float32), torch.float32, "xhat_scale")
            _refused("MU_ERR_ARG", "mu_bn_act_bwd_scaled", X, RES, G, dx, dres, M, C, C, *ops, BAD_ACT, 1, dg, db, xs, ws, n, MU_F32, outs=outs)
            _refused("MU_ERR_ARG", "mu_bn_act_bwd_h", X, RES, G, dx, dres, M, C, *ops, BAD_ACT, 1, dg, db, sc, ws, n, outs=outs)
            _refused("MU_ERR_WORKSPACE", "mu_bn_act_bwd", X, RES, G, dx, dres, M, C, C, *ops, BAD_ACT, 1, dg, db, ws, n - 1, MU_F32, outs=outs)   # size first
        ref = R.bn_act_bwd(x, res, go, mean, rstd, gamma, beta, NONE, 1, None, storage)
        _compare_bwd(f"refusal precedence, valid {storage}", _bwd_call(storage, x, res, go, mean, rstd, gamma, beta, NONE, 1, None, C), ref,
                     R.bn_act_bwd_bounds(ref, NONE, storage))
    # cv = 258 vectors per row: the width is reported before the activation
    CW = 1032
    xw = _in(np.zeros((1, CW), dtype=np.float32), torch.float32, "x")
    ow = [_in(np.ones(CW, dtype=np.float32), torch.float32, "op") for _ in range(4)]
    dxw, dgw, dbw = _out(CW, torch.float32, "dx"), _out(CW, torch.float32, "dgamma"), _out(CW, torch.float32, "dbeta")
    wsw, nw = _bn_ws(CW)
    _refused("MU_ERR_SHAPE", "mu_bn_act_bwd", xw, None, xw, dxw, None, 1, CW, CW, *ow, BAD_ACT, 1, dgw, dbw, wsw, nw, MU_F32, outs=(dxw, dgw, dbw))
    # the pair entry points
    x, go, mean, rstd, geff, beta2, xs, c2, c1 = pair_inputs("f32", C, M)
    X, G = _in(x, torch.float32, "x"), _in(go, torch.float32, "grad_out")
    ops = [_in(v, torch.float32, k) for v, k in ((mean, "mean"), (rstd, "rstd"), (geff, "gamma_eff"), (beta2, "beta2"), (xs, "xhat_scale"),
                                                 (c2, "dgamma2_coef"), (c1, "dgamma1_coef"))]
    dx = _out(M * C, torch.float32, "dx")
    outs = (dx, dg, db, pg, db2, sc)
    _refused("MU_ERR_ARG", "mu_bn_pair_bwd", X, G, dx, M, C, C, *ops, pg, db2, ws, n, MU_F32X, outs=outs)
    _refused("MU_ERR_WORKSPACE", "mu_bn_pair_bwd", X, G, dx, M, C, C, *ops, pg, db2, ws, n - 1, MU_F32, outs=outs)
    _refused("MU_ERR_WORKSPACE", "mu_bn_pair_bwd_h", X, G, dx, M, C, *ops, pg, db2, sc, ws, n - 1, outs=outs)
    _call("mu_bn_pair_bwd", X, G, dx, M, C, C, *ops, pg, db2, ws, n, MU_F32)
    ref = R.bn_act_bwd(x, None, go, mean, rstd, geff, beta2, NONE, 1, xs, "f32")
    b = R.bn_act_bwd_bounds(ref, NONE, "f32")
    _check("refusal precedence, valid pair dx", np.abs(_rows(dx, M, C, C, "dx") - ref["dx"]), b["dx"])
    _compare_pair_grads("refusal precedence, valid pair", _vec(pg).reshape(3, C), _vec(db2), ref, b, c2, c1, C)


# ================================================================================================
# pair: mu_bn_pair_compose, mu_bn_pair_bwd
# ================================================================================================
def compose_inputs(C, eps1):
    g = _rng(8, C, int(eps1 * 1e6))
    top = np.float32(1.0 / math.sqrt(float(np.float32(eps1))))
    rstd1 = (g.random(C) * float(top) * 0.5 + 0.05).astype(np.float32)
    rstd1[0] = top                                              # a constant channel: q = 0 (to rounding), r2 = 1 / sqrt(eps2)
    rstd1[1] = np.nextafter(top, np.float32(np.inf))            # one ulp above: q < 0 before the clamp
    f = lambda: (g.standard_normal(C) * 0.5 + 1.0).astype(np.float32)
    return rstd1, f(), g.standard_normal(C).astype(np.float32), f(), g.standard_normal(C).astype(np.float32), (g.random(C) + 0.5).astype(np.float32)


@pytest.mark.parametrize("M", [1, 100])
@pytest.mark.parametrize("eps1,eps2", [(1e-5, 1e-5), (0.2, 0.3)])
@pytest.mark.parametrize("C", [8, 19, 152])
def test_bn_pair_compose(C, eps1, eps2, M):
    rstd1, gamma1, beta1, gamma2, rm0, rv0 = compose_inputs(C, eps1)
    ins = [_in(a, torch.float32, n) for a, n in ((rstd1, "rstd1"), (gamma1, "gamma1"), (beta1, "beta1"), (gamma2, "gamma2"))]
    for c_valid, running, nbt0 in ((C, True, 3), (C - 2, True, None), (C, False, 9)):
        ref = R.bn_pair_compose(rstd1, gamma1, beta1, gamma2, M, eps1, eps2, 0.1, rm0 if running else None, rv0 if running else None, c_valid)
        rm = _inout(rm0, torch.float32, "running_mean2") if running else None
        rv = _inout(rv0, torch.float32, "running_var2") if running else None
        nbt = None if nbt0 is None else _counter(nbt0)
        outs = [_out(C, torch.float32, n) for n in ("gamma_eff", "xhat_scale", "dgamma2_coef", "dgamma1_coef")]
        _call("mu_bn_pair_compose", *ins, C, c_valid, M, eps1, eps2, 0.1, rm, rv, nbt, *outs)
        what = f"pair_compose C={C} eps=({eps1},{eps2}) M={M} c_valid={c_valid}"
        for o in outs:
            _check(f"{what} {o.name}", np.abs(_vec(o) - ref[o.name]), 2 * U * np.abs(ref[o.name]))
        assert ref["q"][1] == 0.0 and ref["q"][0] < 1e-6
        if running:
            h_rm, h_rv = rm.host(), rv.host()
            _check(what + " running_mean2", np.abs(h_rm[:c_valid] - ref["running_mean2"][:c_valid]), 2 * U * np.abs(ref["running_mean2"][:c_valid]))
            _check(what + " running_var2", np.abs(h_rv[:c_valid] - ref["running_var2"][:c_valid]), 2 * U * np.abs(ref["running_var2"][:c_valid]))
            assert h_rm[c_valid:].tobytes() == rm0[c_valid:].tobytes() and h_rv[c_valid:].tobytes() == rv0[c_valid:].tobytes()
        if nbt0 is not None:
            assert _counter_value(nbt) == nbt0 + 1
    outs = [_out(C, torch.float32, n) for n in ("gamma_eff", "xhat_scale", "dgamma2_coef", "dgamma1_coef")]
    _refused("MU_ERR_ARG", "mu_bn_pair_compose", *ins, C, C, 0, eps1, eps2, 0.1, None, None, None, *outs, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_pair_compose", *ins, C, C, M, eps1, eps2, 0.1, _in(rm0, torch.float32, "rm"), None, None, *outs, outs=outs)
    _refused("MU_ERR_ARG", "mu_bn_pair_compose", ins[0], None, ins[2], ins[3], C, C, M, eps1, eps2, 0.1, None, None, None, *outs, outs=outs)


def pair_inputs(storage, C, M, gmag=1.0):
    """operands of mu_bn_pair_bwd: the backward inputs without activation or residual, and the float32-rounded composition of a first
    layer (gamma1, eps 1e-5) with a second (gamma2, eps 1e-5) as the reference states it"""
    x, _, go, mean, rstd, gamma1, beta = bwd_inputs(storage, C, M, NONE, False, gmag, seed=1)
    gamma2 = (_rng(9, C).standard_normal(C) * 0.5 + 1.0).astype(np.float32)
    comp = R.bn_pair_compose(rstd, gamma1, beta, gamma2, M, EPS, EPS)
    f = lambda k: comp[k].astype(np.float32)
    return x, go, mean, rstd, f("gamma_eff"), beta, f("xhat_scale"), f("dgamma2_coef"), f("dgamma1_coef")


def _compare_pair_grads(what, pg, dbeta2, ref, b, c2, c1, C):
    """rows 0 and 1: coef * float(A) to one fp32 rounding of the product on top of A's own bound; row 2: exactly 0.0"""
    want = R.pair_grads(c2, c1, ref["dgamma"])
    for k, coef in ((0, c2), (1, c1)):
        _check(f"{what} pair_grads[{k}]", np.abs(pg[k] - want[k]), U * np.abs(want[k]) + np.abs(coef.astype(np.float64)) * b["dgamma"])
    assert pg[2].tobytes() == np.zeros(C, dtype=np.float64).tobytes(), what + ": dbeta1 is not +0.0"
    _check(what + " dbeta2", np.abs(dbeta2 - ref["dbeta"]), b["dbeta"])


PAIR_CASES = [pytest.param(s, C, M, id=_id(s, C, M)) for s in ("f32", "f16") for C in (8, 152, 1024) for M in (1, 2 * rpi_of(C, s) + 1, 777)]


@pytest.mark.parametrize("storage,C,M", PAIR_CASES)
def test_bn_pair_bwd(storage, C, M):
    x, go, mean, rstd, geff, beta2, xs, c2, c1 = pair_inputs(storage, C, M)
    ref = R.bn_act_bwd(x, None, go, mean, rstd, geff, beta2, NONE, 1, xs, storage)
    b = R.bn_act_bwd_bounds(ref, NONE, storage)
    T = TORCH[storage]
    for ld in (C, C + 8):
        X, G = _in(_pad(x, ld), T, "x"), _in(_pad(go, ld), T, "grad_out")
        ops = [_in(v, torch.float32, n) for v, n in ((mean, "mean"), (rstd, "rstd"), (geff, "gamma_eff"), (beta2, "beta2"), (xs, "xhat_scale"),
                                                     (c2, "dgamma2_coef"), (c1, "dgamma1_coef"))]
        dx, pg, db2 = _out(M * ld, T, "dx"), _out(3 * C, torch.float32, "pair_grads"), _out(C, torch.float32, "dbeta2")
        ws, n = _bn_ws(C)
        _call("mu_bn_pair_bwd", X, G, dx, M, C, ld, *ops, pg, db2, ws, n, CODE[storage])
        what = f"bn_pair_bwd {storage} C={C} M={M} ld={ld}"
        _check(what + " dx", np.abs(_rows(dx, M, C, ld, what) - ref["dx"]), b["dx"])
        _compare_pair_grads(what, _vec(pg).reshape(3, C), _vec(db2), ref, b, c2, c1, C)


# ================================================================================================
# the fp16-scaled dx forms: mu_bn_act_bwd_h, mu_bn_pair_bwd_h
# ================================================================================================
def h_inputs(C, M, a, use_res, gmag, seed=0):
    """fp32 operands with the zero-padded channels of the model (19 of 24, 150 of 152): x = g = res = 0, gamma = 1, beta = 0, and the
    statistics such data has: mean 0, rstd = 1 / sqrt(eps)"""
    x, res, go, mean, rstd, gamma, beta = bwd_inputs("f32", C, M, a, use_res, gmag, seed)
    cv = {24: 19, 152: 150}.get(C, C)
    x[:, cv:], go[:, cv:] = 0.0, 0.0
    if res is not None:
        res[:, cv:] = 0.0
    mean[cv:], rstd[cv:], gamma[cv:], beta[cv:] = 0.0, np.float32(1.0 / math.sqrt(float(np.float32(EPS)))), 1.0, 0.0
    return x, res, go, mean, rstd, gamma, beta, cv


def _bwd_h_call(x, res, go, mean, rstd, gamma, beta, a, training=1):
    M, C = x.shape
    X, G = _in(x, torch.float32, "x"), _in(go, torch.float32, "grad_out")
    RES = None if res is None else _in(res, torch.float32, "res")
    ops = [_in(v, torch.float32, n) for v, n in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta"))]
    dx = _out(M * C, torch.float32, "dx_h")                   # sized like x: the halves fill its first half
    dres = None if res is None else _out(M * C, torch.float32, "dres")
    dg, db, sc = _out(C, torch.float32, "dgamma"), _out(C, torch.float32, "dbeta"), _out(2, torch.float32, "dy_scale")
    ws, n = _bn_ws(C)
    _call("mu_bn_act_bwd_h", X, RES, G, dx, dres, M, C, *ops, a, training, dg, db, sc, ws, n)
    return _split_dx_h(dx, M, C), None if res is None else _vec(dres).reshape(M, C), _vec(dg), _vec(db), _vec(sc)


def _split_dx_h(dx, M, C):
    """the fp16 rows at the start of the buffer; its second half must still hold the sentinel"""
    raw = dx.host()
    assert (raw[M * C // 2:] == dx.sent).all(), "the second half of the dx buffer was written"
    return raw[:M * C // 2].view(np.float16).astype(np.float64).reshape(M, C)


def _check_scale(what, sc, dx_ref_max, bound_ref):
    """bound_ref: R.dx_bound_per_channel of the reference, its maximum over the channels that count.  The device forms the same bound in
    fp32 from its own dz, s1, s2 (each within ~1e-6 relative of the reference's): S is R.dx_scale of a value within 2^-18 of it"""
    S = float(sc[0])
    assert S in {R.dx_scale(bound_ref * (1 - 2.0 ** -18)), R.dx_scale(bound_ref * (1 + 2.0 ** -18))}, (what, S, bound_ref)
    assert S > 0 and math.frexp(S)[0] == 0.5, (what, S)                       # a power of two
    assert float(sc[1]) == 1.0 / S, (what, sc)
    top = S * dx_ref_max
    print(f"norm-edges {what}: S = 2^{int(math.log2(S))}, S max|dx| = {top:.1f}")
    assert 2.0 ** 11 <= top < 2.0 ** 14, (what, S, top)
    return S


H_CASES = [pytest.param(C, M, a, rs, gm, id=_id("f32", C, M, ACT_NAME[a], "res" if rs else "nores", gm))
           for C in (8, 24, 152) for M in (300, 1025) for a, rs in ((GELU, False), (NONE, False), (GELU, True), (RELU, True)) for gm in (1e-8, 1.0, 3e4)]


@pytest.mark.parametrize("C,M,a,use_res,gmag", H_CASES)
def test_bn_act_bwd_h(C, M, a, use_res, gmag):
    """against the float64 reference, not the plain kernel: S a power of two, dy_scale = {S, 1 / S}, S max|dx| in [2^11, 2^14) whatever the
    gradient's magnitude and with zero-padded channels present, dx_h / S within 2^-11 |dx| of the reference plus the fp32 bound"""
    x, res, go, mean, rstd, gamma, beta, cv = h_inputs(C, M, a, use_res, gmag)
    assert a != RELU or relu_margin_ok("f32", x[:, :cv], None if res is None else res[:, :cv], mean[:cv], rstd[:cv], gamma[:cv], beta[:cv])
    ref = R.bn_act_bwd(x, res, go, mean, rstd, gamma, beta, a, 1, None, "f32")
    b = R.bn_act_bwd_bounds(ref, a, "f32")
    dxh, dres, dg, db, sc = _bwd_h_call(x, res, go, mean, rstd, gamma, beta, a)
    what = f"bn_act_bwd_h C={C} M={M} {ACT_NAME[a]}{'+res' if use_res else ''} g={gmag}"
    S = _check_scale(what, sc, float(np.abs(ref["dx"]).max()), float(R.dx_bound_per_channel(ref).max()))
    _check(what + " dx_h / S", np.abs(dxh / S - ref["dx"]), R.H * np.abs(ref["dx"]) + b["dx"] + 2.0 ** -24 / S)
    _check(what + " dgamma", np.abs(dg - ref["dgamma"]), b["dgamma"])
    _check(what + " dbeta", np.abs(db - ref["dbeta"]), b["dbeta"])
    if use_res:
        _check(what + " dres", np.abs(dres - ref["dres"]), b["dres"])
    assert not dxh[:, cv:].any() and not dg[cv:].any() and not db[cv:].any()           # padded channels: exact zeros


def test_bn_act_bwd_h_special_gradients():
    """an all-zero gradient: S = 1 and exact zeros; an inf: S = 1; one NaN: NaN in that channel only, every other channel within its
    bound and S following the finite values"""
    C, M = 24, 300
    x, res, go, mean, rstd, gamma, beta, cv = h_inputs(C, M, GELU, False, 1.0, seed=2)
    dxh, _, dg, db, sc = _bwd_h_call(x, res, np.zeros_like(go), mean, rstd, gamma, beta, GELU)
    assert sc.tolist() == [1.0, 1.0] and not dxh.any() and not dg.any() and not db.any()
    gi = go.copy()
    gi[7, 4] = np.inf
    assert _bwd_h_call(x, res, gi, mean, rstd, gamma, beta, GELU)[4].tolist() == [1.0, 1.0]
    gn, ch = go.copy(), 5
    gn[7, ch] = np.nan
    gz = go.copy()
    gz[7, ch] = 0.0
    ref = R.bn_act_bwd(x, res, gz, mean, rstd, gamma, beta, GELU, 1, None, "f32")
    b = R.bn_act_bwd_bounds(ref, GELU, "f32")
    dxh, _, dg, db, sc = _bwd_h_call(x, res, gn, mean, rstd, gamma, beta, GELU)
    keep = np.arange(C) != ch
    assert np.isnan(dxh[:, ch]).all() and np.isnan(dg[ch]) and np.isnan(db[ch])
    S = _check_scale("bn_act_bwd_h one NaN", sc, float(np.abs(ref["dx"][:, keep]).max()), float(R.dx_bound_per_channel(ref)[keep].max()))
    _check("bn_act_bwd_h one NaN dx_h / S", np.abs(dxh / S - ref["dx"])[:, keep], (R.H * np.abs(ref["dx"]) + b["dx"] + 2.0 ** -24 / S)[:, keep])
    _check("bn_act_bwd_h one NaN dgamma", np.abs(dg - ref["dgamma"])[keep], b["dgamma"][keep])
    _check("bn_act_bwd_h one NaN dbeta", np.abs(db - ref["dbeta"])[keep], b["dbeta"][keep])


@pytest.mark.parametrize("C,M,gmag", [(8, 300, 1.0), (152, 1025, 1e-8), (152, 300, 3e4)])
def test_bn_pair_bwd_h(C, M, gmag):
    x, go, mean, rstd, geff, beta2, xs, c2, c1 = pair_inputs("f32", C, M, gmag)
    ref = R.bn_act_bwd(x, None, go, mean, rstd, geff, beta2, NONE, 1, xs, "f32")
    b = R.bn_act_bwd_bounds(ref, NONE, "f32")
    X, G = _in(x, torch.float32, "x"), _in(go, torch.float32, "grad_out")
    ops = [_in(v, torch.float32, n) for v, n in ((mean, "mean"), (rstd, "rstd"), (geff, "gamma_eff"), (beta2, "beta2"), (xs, "xhat_scale"),
                                                 (c2, "dgamma2_coef"), (c1, "dgamma1_coef"))]
    dx, pg, db2, sc = _out(M * C, torch.float32, "dx_h"), _out(3 * C, torch.float32, "pair_grads"), _out(C, torch.float32, "dbeta2"), _out(2, torch.float32, "dy_scale")
    ws, n = _bn_ws(C)
    _call("mu_bn_pair_bwd_h", X, G, dx, M, C, *ops, pg, db2, sc, ws, n)
    what = f"bn_pair_bwd_h C={C} M={M} g={gmag}"
    S = _check_scale(what, _vec(sc), float(np.abs(ref["dx"]).max()), float(R.dx_bound_per_channel(ref).max()))
    _check(what + " dx_h / S", np.abs(_split_dx_h(dx, M, C) / S - ref["dx"]), R.H * np.abs(ref["dx"]) + b["dx"] + 2.0 ** -24 / S)
    _compare_pair_grads(what, _vec(pg).reshape(3, C), _vec(db2), ref, b, c2, c1, C)


# ================================================================================================
# the large BatchNorm case: ew_grid rounds above its cap
# ================================================================================================
def _t_gelu(p):
    return 0.5 * p * (1.0 + torch.special.erf(p / math.sqrt(2.0)))


def _t_gelu_grad(p):
    return 0.5 * (1.0 + torch.special.erf(p / math.sqrt(2.0))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi)


def _t_check(what, err, bound):
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound)
    assert not bool(torch.isnan(ratio).any()), (what, "nan")
    i = int(torch.argmax(ratio))
    _note(what, float(err.reshape(-1)[i]), float(bound.expand_as(err).reshape(-1)[i]))
    assert float(ratio.reshape(-1)[i]) <= 1.0, (what, i)


def test_bn_act_large_grid_above_the_cap():
    """fp16, C = 152 (19 vectors per row), M = 442000: 8.4 M vectors, so ew_grid's 8192-block cap is rounded up to 8208 = 19 * 432.
    GELU with a residual, forward and backward on the same buffers; every element is compared with the formulas of
    tests/_norm_reference.py (bn_act_fwd / bn_act_bwd and their bounds) evaluated by torch in float64 on the device."""
    M, C = 442000, 152
    n = M * C
    T, H, D = torch.float16, R.H, torch.float64
    gen = torch.Generator(device="cuda").manual_seed(12)
    bufs = {k: Guarded(n, T, name=k) for k in ("x", "res", "g", "y", "dx", "dres")}
    for k, (s, o) in (("x", (1.5, 0.3)), ("res", (1.0, 0.0)), ("g", (1.0, 0.0))):
        bufs[k].t.copy_((torch.randn(n, device="cuda", generator=gen) * s + o).to(T))
    keep = {k: bufs[k].t.clone() for k in ("x", "res", "g")}
    x = keep["x"].view(M, C).to(D)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    rng = _rng(10)
    mean32, rstd32 = mean.float(), torch.rsqrt(var + float(np.float32(EPS))).float()
    gamma32 = torch.from_numpy((rng.standard_normal(C) * 0.5 + 1.0).astype(np.float32)).cuda()
    beta32 = torch.from_numpy((rng.standard_normal(C) * 0.5).astype(np.float32)).cuda()
    ops = [Guarded(C, torch.float32, name=k) for k in ("mean", "rstd", "gamma", "beta")]
    for o, v in zip(ops, (mean32, rstd32, gamma32, beta32)):
        o.t.copy_(v)
    dg, db = _out(C, torch.float32, "dgamma"), _out(C, torch.float32, "dbeta")
    ws, nws = _bn_ws(C)
    _call("mu_bn_act_fwd", bufs["x"], bufs["res"], bufs["y"], M, C, C, *ops, GELU, MU_F16)
    _call("mu_bn_act_bwd", bufs["x"], bufs["res"], bufs["g"], bufs["dx"], bufs["dres"], M, C, C, *ops, GELU, 1, dg, db, ws, nws, MU_F16)
    for k in keep:
        assert torch.equal(bufs[k].t, keep[k]), k + " is an input"
    for o, v in zip(ops, (mean32, rstd32, gamma32, beta32)):
        assert torch.equal(o.t, v)
    mu, rs, ga, be = (v.to(D) for v in (mean32, rstd32, gamma32, beta32))
    res, g = keep["res"].view(M, C).to(D), keep["g"].view(M, C).to(D)
    # forward (R.bn_act_fwd, R.bn_act_fwd_bound)
    xhat = (x - mu) * rs
    pre = xhat * ga + be + res
    y_ref = _t_gelu(pre)
    A = (rs * ga).abs()
    pre_b = U * (4 * x.abs() * A + 5 * mu.abs() * A + 3 * be.abs() + res.abs())
    y_b = 1.13 * pre_b + R.PHI_POLY_ERR + H * y_ref.abs() + 2.0 ** -24
    _t_check("large bn_act_fwd y", (bufs["y"].t.view(M, C).to(D) - y_ref).abs(), y_b)
    del y_ref, y_b, pre_b
    # backward (R.bn_act_bwd, R.bn_act_bwd_bounds)
    dz = (g * _t_gelu_grad(pre)).to(T).to(D)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    s1, s2 = dbeta / M, dgamma / M
    dx_ref = ga * rs * (dz - s1 - xhat * s2)
    ax, adz = xhat.abs(), dz.abs()
    pre_b = U * (4 * ax * ga.abs() + 2 * be.abs() + 2 * res.abs())
    dz_b = g.abs() * (0.8 * pre_b + R.GRAD_POLY_ERR) + U * adz + 2 * H * adz + 2.0 ** -24
    dbeta_b = dz_b.sum(0) + U * adz.sum(0) + U * dbeta.abs()
    dgamma_b = (dz_b * ax + 2 * U * adz * ax).sum(0) + 2 * U * (adz * ax).sum(0) + U * dgamma.abs()
    s1_b, s2_b = dbeta_b / M + U * s1.abs(), dgamma_b / M + 2 * U * s2.abs()
    gr = (ga * rs).abs()
    dx_b = gr * (dz_b + s1_b + ax * s2_b) + 8 * U * (gr * (adz + s1.abs()) + gr * (rs * s2).abs() * (x.abs() + mu.abs())) + H * dx_ref.abs() + 2.0 ** -24
    _t_check("large bn_act_bwd dres", (bufs["dres"].t.view(M, C).to(D) - dz).abs(), dz_b)
    _t_check("large bn_act_bwd dx", (bufs["dx"].t.view(M, C).to(D) - dx_ref).abs(), dx_b)
    _t_check("large bn_act_bwd dbeta", (db.t.to(D) - dbeta).abs(), dbeta_b)
    _t_check("large bn_act_bwd dgamma", (dg.t.to(D) - dgamma).abs(), dgamma_b)
    del bufs, keep, x, res, g, xhat, pre, dz, dx_ref, dz_b, dx_b, ax, adz, pre_b
    torch.cuda.empty_cache()


# ================================================================================================
# column sums: mu_colsum
# ================================================================================================
def _decode_bf16x4(bits):
    """uint32 words [.., 4] of one 16-byte chunk [4 bf16 hi | 4 bf16 lo] -> the four values hi + lo as float64"""
    f = lambda w: w.astype(np.uint32).view(np.float32).astype(np.float64)
    ex, ey, ez, ew = (bits[..., k] for k in range(4))
    lo16, hi16 = (lambda w: (w << np.uint32(16))), (lambda w: (w & np.uint32(0xffff0000)))
    return np.stack([f(lo16(ex)) + f(lo16(ez)), f(hi16(ex)) + f(hi16(ez)), f(lo16(ey)) + f(lo16(ew)), f(hi16(ey)) + f(hi16(ew))], axis=-1)


def _encode_bf16(a):
    """mu_split_encode of a float32 matrix on the device -> the encoded words as float32 bit patterns (numpy), same shape"""
    from maskunet_amd import _lib
    src = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    dst = torch.empty_like(src)
    _lib.call("mu_split_encode", src.data_ptr(), dst.data_ptr(), src.numel(), _lib.stream())
    torch.cuda.synchronize()
    return dst.cpu().numpy()


COLSUM_CASES = [pytest.param(mode, C, M, id=_id(mode, C, M)) for mode in ("f32", "f16", "f32x")
                for C in (8, 24, 152, 1024) + ((2048,) if mode == "f16" else ())
                for M in stat_M_edges(C, "f16" if mode == "f16" else "f32") + (STAT_BIG_M if C == 8 else [])]


@pytest.mark.parametrize("mode,C,M", COLSUM_CASES)
def test_colsum(mode, C, M):
    """ld = C, and a column block of a wider matrix (ld = 3 C, the pointer at column C; its neighbours are NaN)"""
    storage = "f16" if mode == "f16" else "f32"
    T, code = TORCH[storage], (MU_F32X if mode == "f32x" else CODE[storage])
    g = _rng(11, C, M, {"f32": 4, "f16": 8, "f32x": 5}[mode])
    x = _st(storage, g.standard_normal((M, C), dtype=np.float32) * np.float32(1.5) + np.float32(0.3))
    from maskunet_amd import _lib
    nws = _lib.load().mu_colsum_workspace_bytes(C)
    for ld, col in ((C, 0), (3 * C, C)):
        full = np.full((M, ld), NAN, dtype=x.dtype)
        full[:, col:col + C] = x
        if mode == "f32x":
            full = _encode_bf16(full)
            vals = _decode_bf16x4(full[:, col:col + C].view(np.uint32).reshape(M, C // 4, 4)).reshape(M, C)
        else:
            vals = full[:, col:col + C]
        s, sabs = R.colsum(vals)
        X, out, ws = _in(full, T, "x"), _out(C, torch.float32, "out"), _out(nws, torch.uint8, "workspace")
        _lib.call("mu_colsum", X.p + col * X.t.element_size(), M, C, ld, out.p, ws.p, nws, code, _lib.stream())
        torch.cuda.synchronize()
        for b in (X, out, ws):
            b.check()
        _check(f"colsum {mode} C={C} M={M} ld={ld}", np.abs(_vec(out) - s), R.colsum_bound(s, sabs))


def test_colsum_refusals():
    from maskunet_amd import _lib
    lib = _lib.load()
    X, out = _in(np.zeros((4, 16), dtype=np.float32), torch.float32, "x"), _out(8, torch.float32, "out")
    n = lib.mu_colsum_workspace_bytes(8)
    ws = _out(n, torch.uint8, "workspace")
    _refused("MU_ERR_SHAPE", "mu_colsum", X, 4, 8, 10, out, ws, n, MU_F32X, outs=(out,))                 # ld % 4
    _refused("MU_ERR_ARG", "mu_colsum", X, 4, 12, 12, out, ws, n, MU_F32, outs=(out,))
    _refused("MU_ERR_ARG", "mu_colsum", X, 4, 8, 7, out, ws, n, MU_F32, outs=(out,))
    _refused("MU_ERR_ARG", "mu_colsum", X, 0, 8, 8, out, ws, n, MU_F32, outs=(out,))
    _refused("MU_ERR_ARG", "mu_colsum", X, 4, 8, 8, None, ws, n, MU_F32, outs=(out,))
    _refused("MU_ERR_ARG", "mu_colsum", X, 4, 8, 8, out, ws, n, 9, outs=(out,))
    _refused("MU_ERR_WORKSPACE", "mu_colsum", X, 4, 8, 8, out, ws, n - 1, MU_F32, outs=(out,))
    for code, C, T in ((MU_F32, 1032, torch.float32), (MU_F32X, 1032, torch.float32), (MU_F16, 2056, torch.float16)):      # cv = 257
        xw, ow = _in(np.zeros((1, C), dtype=np.float32), T, "x"), _out(C, torch.float32, "out")
        nw = lib.mu_colsum_workspace_bytes(C)
        _refused("MU_ERR_SHAPE", "mu_colsum", xw, 1, C, C, ow, _out(nw, torch.uint8, "workspace"), nw, code, outs=(ow,))


def test_colsum_encoded_large_runs_the_sixteenth_iteration_fold():
    """MU_F32X, M = 66000, C = 1024: 1024 blocks of 65 rows, one row lane, four rows per iteration -> 17 iterations, so the fold of the
    fp32 short sum into the doubles inside the loop (every 16th iteration) runs.  Encoded and decoded on the device."""
    from maskunet_amd import _lib
    M, C = 66000, 1024
    gen = torch.Generator(device="cuda").manual_seed(13)
    X = Guarded(M * C, torch.float32, name="x")
    src = torch.randn(M * C, device="cuda", generator=gen) * 1.5 + 0.3
    _lib.call("mu_split_encode", src.data_ptr(), X.p, M * C, _lib.stream())
    del src
    keep = X.t.clone()
    n = _lib.load().mu_colsum_workspace_bytes(C)
    out, ws = _out(C, torch.float32, "out"), _out(n, torch.uint8, "workspace")
    _call("mu_colsum", X, M, C, C, out, ws, n, MU_F32X)
    assert torch.equal(X.t.view(torch.int32), keep.view(torch.int32))
    w = keep.view(torch.int32).view(-1, 4)
    halves = lambda d: torch.stack([(d << 16).view(torch.float32), (d & -65536).view(torch.float32)], -1).double()
    dec = (torch.cat([halves(w[:, 0]), halves(w[:, 1])], -1) + torch.cat([halves(w[:, 2]), halves(w[:, 3])], -1)).reshape(M, C)
    s, sabs = dec.sum(0).cpu().numpy(), dec.abs().sum(0).cpu().numpy()
    _check("colsum f32x large", np.abs(_vec(out) - s), R.colsum_bound(s, sabs))
    del X, keep, dec, w
    torch.cuda.empty_cache()


# ================================================================================================
# per-sample LayerNorm: mu_ln_sample_fwd, mu_ln_sample_bwd
# ================================================================================================
def ln_inputs(storage, B, L, r):
    g = _rng(14, B, L, int(r * 2), NVEC[storage])
    x = _st(storage, g.standard_normal((B, L), dtype=np.float32) * np.float32(2.0) + np.float32(r))
    dy = _st(storage, g.standard_normal((B, L), dtype=np.float32))
    return x, dy, (g.standard_normal(L) * 0.5 + 1.0).astype(np.float32), (g.standard_normal(L) * 0.5).astype(np.float32)


def _ln_ws(B):
    from maskunet_amd import _lib
    n = _lib.load().mu_ln_sample_workspace_bytes(B)
    return _out(n, torch.uint8, "workspace"), n


LN_CASES = [pytest.param(s, B, L, r, id=_id(s, B, L, f"r{r}")) for s, rs in (("f32", (0.5, 300)), ("f16", (0.5,)))
            for L in (8, 264, 1016, 1024, 1032, 131072, 131080) for B in (1, 3, 4, 5) for r in rs]


def _count_beyond(what, err, first, wide):
    """the issue's rule for a bound the operation order cannot meet: every element is held to `first`, those beyond it are counted,
    printed and held to `wide`"""
    beyond = err > first
    print(f"norm-edges {what}: {int(beyond.sum())} of {err.size} beyond the first bound, worst err / first bound "
          f"{float(np.max(np.where(first > 0, err / np.where(first > 0, first, 1.0), 0.0))):.3f}")
    _check(what, err, np.where(beyond, wide, first))


@pytest.mark.parametrize("storage,B,L,r", LN_CASES)
def test_ln_sample(storage, B, L, r):
    """empty blocks (L / N < 128), `per` tails, 1 to 5 samples over lns_final_kernel's 4 per block; at r = 300 (fp32) the tight bound
    still holds: this sweep accumulates in fp64 element by element"""
    x, dy, w, b = ln_inputs(storage, B, L, r)
    T = TORCH[storage]
    X, W, Bv = _in(x, T, "x"), _in(w, torch.float32, "w"), _in(b, torch.float32, "b")
    y, mean, rstd = _out(B * L, T, "y"), _out(B, torch.float32, "mean"), _out(B, torch.float32, "rstd")
    ws, n = _ln_ws(B)
    _call("mu_ln_sample_fwd", X, W, Bv, y, mean, rstd, B, L, EPS, ws, n, CODE[storage])
    ref = R.ln_sample_fwd(x, w, b, EPS)
    fb = R.ln_sample_fwd_bounds(ref, storage)
    what = f"ln_sample {storage} B={B} L={L} r={r}"
    _check(what + " mean", np.abs(_vec(mean) - ref["mean"]), fb["mean"])
    _check(what + " rstd", np.abs(_vec(rstd) - ref["rstd"]), fb["rstd"])
    _check(what + " y", np.abs(_vec(y).reshape(B, L) - ref["y"]), fb["y"])
    # backward on the stored statistics
    m32, r32 = mean.host().copy(), rstd.host().copy()
    DY, MEAN, RSTD = _in(dy, T, "dy"), _in(m32, torch.float32, "mean"), _in(r32, torch.float32, "rstd")
    dx, dw, db = _out(B * L, T, "dx"), _out(L, torch.float32, "dw"), _out(L, torch.float32, "db")
    ws, n = _ln_ws(B)
    _call("mu_ln_sample_bwd", X, DY, W, MEAN, RSTD, dx, dw, db, B, L, ws, n, CODE[storage])
    bref = R.ln_sample_bwd(x, dy, w, m32, r32)
    bb = R.ln_sample_bwd_bounds(bref, storage)
    _check(what + " dx", np.abs(_vec(dx).reshape(B, L) - bref["dx"]), bb["dx"])
    _check(what + " db", np.abs(_vec(db) - bref["db"]), bb["db"])
    _count_beyond(what + " dw", np.abs(_vec(dw) - bref["dw"]), bb["dw"], bb["dw_wide"])


def test_ln_sample_large_apply_grid_capped():
    """L = 8388616, B = 2, fp32: 2097154 vectors = 8193 blocks of 256, one more than the apply grids' cap of 8192.  Inputs drawn on the
    device; the reference is the formulas of R.ln_sample_fwd / R.ln_sample_bwd and their bounds in torch float64 on the device."""
    B, L, D = 2, 8388616, torch.float64
    gen = torch.Generator(device="cuda").manual_seed(15)
    X, DY = Guarded(B * L, torch.float32, name="x"), Guarded(B * L, torch.float32, name="dy")
    W, Bv = Guarded(L, torch.float32, name="w"), Guarded(L, torch.float32, name="b")
    X.t.copy_(torch.randn(B * L, device="cuda", generator=gen) * 2.0 + 0.5)
    DY.t.copy_(torch.randn(B * L, device="cuda", generator=gen))
    W.t.copy_(torch.randn(L, device="cuda", generator=gen) * 0.5 + 1.0)
    Bv.t.copy_(torch.randn(L, device="cuda", generator=gen) * 0.5)
    keep = [t.t.clone() for t in (X, DY, W, Bv)]
    y, dx = _out(B * L, torch.float32, "y"), _out(B * L, torch.float32, "dx")
    dw, db = _out(L, torch.float32, "dw"), _out(L, torch.float32, "db")
    mean, rstd = _out(B, torch.float32, "mean"), _out(B, torch.float32, "rstd")
    ws, n = _ln_ws(B)
    _call("mu_ln_sample_fwd", X, W, Bv, y, mean, rstd, B, L, EPS, ws, n, MU_F32)
    _call("mu_ln_sample_bwd", X, DY, W, mean, rstd, dx, dw, db, B, L, ws, n, MU_F32)
    for t, k in zip((X, DY, W, Bv), keep):
        assert torch.equal(t.t, k), t.name + " is an input"
    for o in (y, dx, dw, db, mean, rstd):
        o.all_written()
    x, dy, w, b = keep[0].view(B, L).to(D), keep[1].view(B, L).to(D), keep[2].to(D), keep[3].to(D)
    m = x.mean(1, keepdim=True)
    rs = torch.rsqrt(((x - m) ** 2).mean(1, keepdim=True) + float(np.float32(EPS)))
    mean_b = 2 * U * m.abs() + U * x.abs().mean(1, keepdim=True)
    _t_check("ln large mean", (mean.t.to(D).view(B, 1) - m).abs(), mean_b)
    _t_check("ln large rstd", (rstd.t.to(D).view(B, 1) - rs).abs(), 2 * U * rs)
    xhat = (x - m) * rs
    aw = (xhat * w).abs()
    _t_check("ln large y", (y.t.view(B, L).to(D) - (xhat * w + b)).abs(), rs * mean_b * w.abs() + aw * 2 * U + 4 * U * (aw + b.abs()))
    m32, r32 = mean.t.to(D).view(B, 1), rstd.t.to(D).view(B, 1)
    xhat = (x - m32) * r32
    gw = dy * w
    m1, m2 = gw.mean(1, keepdim=True), (gw * xhat).mean(1, keepdim=True)
    agw, ax = gw.abs(), xhat.abs()
    m1_b = U * (agw.mean(1, keepdim=True) + m1.abs())
    m2_b = U * (3 * (agw * ax).mean(1, keepdim=True) + m2.abs())
    axm2 = ax * m2.abs()
    dx_ref = r32 * (gw - m1 - xhat * m2)
    dx_b = r32 * (U * agw + m1_b + ax * m2_b + 2 * U * axm2) + 4 * U * r32 * (agw + m1.abs() + axm2) + U * dx_ref.abs()
    _t_check("ln large dx", (dx.t.view(B, L).to(D) - dx_ref).abs(), dx_b)
    _t_check("ln large db", (db.t.to(D) - dy.sum(0)).abs() , B * U * dy.abs().sum(0))
    _t_check("ln large dw", (dw.t.to(D) - (dy * xhat).sum(0)).abs(), (B + 3) * U * (dy * xhat).abs().sum(0))
    del X, DY, W, Bv, keep, y, dx, dw, db, x, dy, w, b, xhat, gw, agw, ax, dx_ref, dx_b, aw, axm2
    torch.cuda.empty_cache()


def test_ln_sample_refusals():
    x, dy, w, b = ln_inputs("f32", 2, 16, 0.5)
    X, DY, W, Bv = _in(x, torch.float32, "x"), _in(dy, torch.float32, "dy"), _in(w, torch.float32, "w"), _in(b, torch.float32, "b")
    y, mean, rstd = _out(32, torch.float32, "y"), _out(2, torch.float32, "mean"), _out(2, torch.float32, "rstd")
    dx, dw, db = _out(32, torch.float32, "dx"), _out(16, torch.float32, "dw"), _out(16, torch.float32, "db")
    ws, n = _ln_ws(2)
    M_, R_ = _in(np.zeros(2, np.float32), torch.float32, "mean"), _in(np.ones(2, np.float32), torch.float32, "rstd")
    fo, bo = (y, mean, rstd), (dx, dw, db)
    _refused("MU_ERR_ARG", "mu_ln_sample_fwd", X, W, Bv, y, mean, rstd, 2, 12, EPS, ws, n, MU_F32, outs=fo)          # L % 8
    _refused("MU_ERR_ARG", "mu_ln_sample_fwd", X, W, Bv, y, mean, rstd, 0, 16, EPS, ws, n, MU_F32, outs=fo)          # B = 0
    _refused("MU_ERR_ARG", "mu_ln_sample_fwd", X, None, Bv, y, mean, rstd, 2, 16, EPS, ws, n, MU_F32, outs=fo)
    _refused("MU_ERR_ARG", "mu_ln_sample_fwd", X, W, Bv, y, mean, rstd, 2, 16, EPS, ws, n, MU_F32X, outs=fo)
    _refused("MU_ERR_WORKSPACE", "mu_ln_sample_fwd", X, W, Bv, y, mean, rstd, 2, 16, EPS, ws, n - 1, MU_F32, outs=fo)
    _refused("MU_ERR_ARG", "mu_ln_sample_bwd", X, DY, W, M_, R_, dx, dw, db, 2, 12, ws, n, MU_F32, outs=bo)
    _refused("MU_ERR_ARG", "mu_ln_sample_bwd", X, DY, W, M_, R_, dx, dw, db, 0, 16, ws, n, MU_F32, outs=bo)
    _refused("MU_ERR_ARG", "mu_ln_sample_bwd", X, DY, W, M_, R_, dx, None, db, 2, 16, ws, n, MU_F32, outs=bo)
    _refused("MU_ERR_WORKSPACE", "mu_ln_sample_bwd", X, DY, W, M_, R_, dx, dw, db, 2, 16, ws, n - 1, MU_F32, outs=bo)
