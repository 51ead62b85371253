"""The generic attention path (C > 256): the six row kernels of maskunet_amd/csrc/attn_wide.hip -- mu_gather_rows, mu_scatter_rows,
mu_softmax_rows, mu_attn_wide_ds, mu_ln_rows_fwd, mu_ln_rows_bwd -- through the C ABI against tests/_attn_wide_reference.py (float64)
at every row, stride and mask edge, and ops.mask_attention above 256 channels against the float64 closed form of the whole block.

Every tensor operand sits in a tests/_device_buffers.Guarded buffer: after each call the guard bands are intact, the inputs are
byte-identical, the outputs wholly written except where the contract says "left alone", and with a row stride above the width the
columns between still hold the sentinel.  Every bound is derived in the docstrings of tests/_attn_wide_reference.py (gather, scatter,
tails, pad channels and the NaN rules are bit-exact: bound 0); every test prints its worst err / bound (pytest -s / -rP).
tests/test_attn_wide_reference_host.py checks on the CPU that the reference is right, that the input recipes meet their conditions
and that the bounds catch a list of deliberately wrong kernels.  fp16 and fp32 throughout; MU_F32X must give the bytes of MU_F32.

The caller's obligations are NOT probed: cnt above the row count or ld, indices outside the tensor and infinities break the kernels'
contract (they would read or write out of bounds, or turn into NaN by design) -- handing them in would be provoking a fault."""
import numpy as np
import pytest
import torch

from tests import _attn_wide_reference as R
from tests._device_buffers import Guarded

pytestmark = pytest.mark.gpu

MU_F32, MU_F16, MU_F32X = 0, 1, 2
BAD_DTYPE = 7
STORAGES = ("f32", "f16")
TORCH = {"f32": torch.float32, "f16": torch.float16}
CODES = {"f32": (MU_F32, MU_F32X), "f16": (MU_F16,)}           # the first is the reference run, the others must repeat its bytes
I32 = torch.int32
F32 = torch.float32


# ================================================================================================
# plumbing
# ================================================================================================
class At:
    """a Guarded buffer entered `off` elements in (a block of columns inside wider rows, as ops hands qkv and dqkv over)"""

    def __init__(self, g, off):
        self.g, self.p = g, g.p + off * g.t.element_size()


def _in(a, dtype, name):
    a = np.ascontiguousarray(a)
    return Guarded(a.size, dtype, data=a, name=name)


def _out(n, dtype, name):
    return Guarded(int(n), dtype, name=name)


def _inout(a, dtype, name):
    """an operand the kernel updates in place: starts as `a`, no 'unchanged' check"""
    a = np.ascontiguousarray(a)
    g = Guarded(a.size, dtype, name=name)
    g.t.copy_(torch.as_tensor(a).reshape(-1).to(g.t.device))
    return g


def _cnt(n):
    return _in(np.array([n], dtype=np.int32), I32, "cnt")


def _raw(a):
    return a.p if isinstance(a, (Guarded, At)) else a


def _guards(args):
    for a in args:
        if isinstance(a, (Guarded, At)):
            (a.g if isinstance(a, At) else a).check()


def _call(name, *args):
    from maskunet_amd import _lib
    _lib.call(name, *[_raw(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    _guards(args)


def _refused(name, *args, outs):
    """MU_ERR_ARG before anything is launched: every output still holds the sentinel"""
    from maskunet_amd import _lib
    with pytest.raises(RuntimeError, match="MU_ERR_ARG"):
        _lib.call(name, *[_raw(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    _guards(list(args) + list(outs))
    for o in outs:
        assert bool((o.t == o.sent).all()), (name, o.name)


class Worst:
    """the worst err / bound of one test; every element within its bound, a NaN anywhere fails"""

    def __init__(self, what):
        self.what, self.ratio, self.at = what, 0.0, None

    def check(self, what, got, ref, bound):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
        assert np.isfinite(bound).all(), (what, "the bound itself is not finite")
        assert not np.isnan(got).any(), (what, "nan")
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        i = int(np.argmax(ratio))
        if ratio.flat[i] > self.ratio:
            self.ratio, self.at = float(ratio.flat[i]), (what, float(err.flat[i]), float(bound.flat[i]))
        assert ratio.flat[i] <= 1.0, (what, float(err.flat[i]), float(bound.flat[i]), np.unravel_index(i, err.shape))

    def note(self):
        print(f"attn-wide-edges {self.what}: worst err / bound {self.ratio:.3f} at {self.at}")


def _same(got, want, what):
    """bit-exact, except that any NaN stands for any NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), what + ": NaN pattern"
    assert got[~ng].tobytes() == want[~nw].tobytes(), what


def _repeat(first, got, what):
    """MU_F32X after MU_F32: the same bytes"""
    if first is not None:
        assert got.tobytes() == first.tobytes(), what + ": MU_F32X differs from MU_F32"
    return got if first is None else first


# ================================================================================================
# mu_gather_rows / mu_scatter_rows: bit-exact
# ================================================================================================
@pytest.mark.parametrize("C", sorted(set(R.C_SET) | {8}))
@pytest.mark.parametrize("storage", STORAGES)
def test_gather_rows(storage, C):
    """every channel count around the 256-strided channel loop, src_ld = C and 3C (entered one C in, NaN around the block), 1 / 32 /
    4100 rows (the block cap of 4096), cnt 0 / 1 / rows - 1 / rows, idx a random permutation: rows >= cnt are exactly zero"""
    T, n = TORCH[storage], 0
    for C_, ld, rows, cnt in R.gather_cases():
        if C_ != C:
            continue
        src, off, idx = R.gather_inputs(storage, C, ld, rows, cnt)
        want = R.gather_rows(src[:, off:off + C], idx, cnt, rows)
        SRC, IDX, CNT = _in(src, T, "src"), _in(idx, I32, "idx"), _cnt(cnt)
        first = None
        for code in CODES[storage]:
            dst = _out(rows * C, T, "dst")
            _call("mu_gather_rows", At(SRC, off), ld, IDX, CNT, dst, rows, C, code)
            got = dst.host((rows, C))
            what = f"gather {storage} C={C} ld={ld} rows={rows} cnt={cnt} code={code}"
            assert got.tobytes() == want.tobytes(), what
            assert not got[cnt:].any(), what + ": rows behind cnt"
            first = _repeat(first, got, what)
            n += 1
    assert n
    print(f"attn-wide-edges gather {storage} C={C}: {n} calls bit-exact (bound 0), worst err / bound 0.000")


@pytest.mark.parametrize("C", sorted(set(R.C_SET) | {8}))
@pytest.mark.parametrize("storage", STORAGES)
def test_scatter_rows(storage, C):
    """the same channel counts and strides, 1 / 40 / 4100 rows, cnt 0 / 1 / rows: cnt == 0 writes NaN to the first C columns of every
    row and nothing else; cnt > 0 leaves the unlisted rows and the columns around the block as they were; fp32 -> fp16 rounds to
    nearest even (ties, a subnormal and the largest finite fp16 in the first row)"""
    T, n = TORCH[storage], 0
    for C_, ld, rows, cnt in R.scatter_cases():
        if C_ != C:
            continue
        src, idx = R.scatter_inputs(C, rows, cnt)
        off = C if ld > C else 0
        val, written = R.scatter_rows(src, idx, cnt, rows, storage)
        SRC, IDX, CNT = _in(src, F32, "src"), _in(idx, I32, "idx"), _cnt(cnt)
        first = None
        for code in CODES[storage]:
            dst = _out(rows * ld, T, "dst")
            want = np.full((rows, ld), dst.sent, dtype=R.NP[storage])
            want[written, off:off + C] = val[written]
            _call("mu_scatter_rows", SRC, IDX, CNT, At(dst, off), ld, rows, C, code)
            got = dst.host((rows, ld))
            what = f"scatter {storage} C={C} ld={ld} rows={rows} cnt={cnt} code={code}"
            _same(got, want, what)
            if cnt == 0:
                assert np.isnan(got[:, off:off + C]).all(), what
            first = _repeat(first, np.nan_to_num(got, nan=12345.0), what)
            n += 1
    assert n
    print(f"attn-wide-edges scatter {storage} C={C}: {n} calls bit-exact (bound 0), worst err / bound 0.000")


# ================================================================================================
# mu_softmax_rows / mu_attn_wide_ds
# ================================================================================================
def _score_cases(ld):
    return [c for c in R.softmax_cases() if c[1] == ld]


@pytest.mark.parametrize("ld", R.LD_SET)
@pytest.mark.parametrize("storage", STORAGES)
def test_softmax_rows(storage, ld):
    """ld and cnt around the 256-strided column loops, 1 / 5 / 4100 rows, both scales, every value recipe (ordinary, constant, one
    dominant score with all other probabilities underflowing, scale * (s - m) down to -80): in place; columns behind cnt exactly 0;
    cnt == 0: NaN over the whole ld; fp32: every row sums to 1 within the sum of its elements' bounds"""
    T, w, ws = TORCH[storage], Worst(f"softmax {storage} ld={ld}"), Worst(f"softmax row sums {storage} ld={ld}")
    for N, _, cnt, scale in _score_cases(ld):
        s, _names = R.score_rows(storage, N, ld, cnt, scale)
        ref, bound = R.softmax_rows(s, cnt, scale, storage)
        CNT, first = _cnt(cnt), None
        for code in CODES[storage]:
            S = _inout(s, T, "S")
            _call("mu_softmax_rows", S, N, ld, CNT, float(scale), code)
            got = S.host((N, ld))
            what = f"softmax {storage} N={N} ld={ld} cnt={cnt} scale={scale:.4f} code={code}"
            if cnt == 0:
                assert np.isnan(got).all(), what + ": no visible key must give NaN over the whole ld"
            else:
                w.check(what, got, ref, bound)
                assert not got[:, cnt:].any(), what + ": columns behind cnt"
                if storage == "f32":
                    ws.check(what + " row sum", got.astype(np.float64).sum(1), np.ones(N), bound.sum(1))
            first = _repeat(first, np.nan_to_num(got, nan=12345.0), what)
    w.note()
    if storage == "f32":
        ws.note()


@pytest.mark.parametrize("ld", R.LD_SET)
@pytest.mark.parametrize("storage", STORAGES)
def test_attn_wide_ds(storage, ld):
    """the same shapes and scales; P is the stored softmax of the score recipes with garbage behind cnt, dP ordinary rows and a
    constant row (d - a cancels): dS in place on dP, P unchanged, columns behind cnt exactly 0, cnt == 0: NaN rows"""
    T, w = TORCH[storage], Worst(f"dS {storage} ld={ld}")
    for N, _, cnt, scale in _score_cases(ld):
        p, d, _names = R.ds_inputs(storage, N, ld, cnt, scale)
        ref, bound = R.attn_wide_ds(p, d, cnt, scale, storage)
        P, CNT, first = _in(p, T, "P"), _cnt(cnt), None
        for code in CODES[storage]:
            D = _inout(d, T, "dP")
            _call("mu_attn_wide_ds", P, D, N, ld, CNT, float(scale), code)            # (_call: P is byte-identical afterwards)
            got = D.host((N, ld))
            what = f"dS {storage} N={N} ld={ld} cnt={cnt} scale={scale:.4f} code={code}"
            if cnt == 0:
                assert np.isnan(got).all(), what + ": no visible key must give NaN rows"
            else:
                w.check(what, got, ref, bound)
                assert not got[:, cnt:].any(), what + ": columns behind cnt"
            first = _repeat(first, np.nan_to_num(got, nan=12345.0), what)
    w.note()


# ================================================================================================
# mu_ln_rows_fwd / mu_ln_rows_bwd
# ================================================================================================
@pytest.mark.parametrize("C,cv", R.LN_SHAPES)
@pytest.mark.parametrize("storage", STORAGES)
def test_ln_rows(storage, C, cv):
    """one channel, fewer channels than a wave, one and several 64-strided passes with and without a tail, c_valid below C (the pad
    channels of the inputs hold garbage, those of the outputs are exactly 0), C > 512; 1 / 3 / 4 / 5 rows (4 rows per block) and 16390
    rows (beyond the cap of 4096 blocks); ordinary, constant and mean-100 / spread-0.01 rows.  The backward is fed the reference's
    stored statistics rounded to fp32."""
    T = TORCH[storage]
    w = {k: Worst(f"ln {k} {storage} C={C} cv={cv}") for k in ("out", "mean", "rstd", "dY", "gxh")}
    for C_, cv_, rows in R.ln_cases():
        if (C_, cv_) != (C, cv):
            continue
        o, x, g, gamma, beta, _names = R.ln_inputs(storage, C, cv, rows)
        ref = R.ln_rows_fwd(o, x, gamma, beta, cv, R.EPS, storage)
        mean32, rstd32 = ref["mean"].astype(np.float32), ref["rstd"].astype(np.float32)
        refb = R.ln_rows_bwd(g, o, x, mean32, rstd32, gamma, cv, storage)
        O, X, G = _in(o, T, "o"), _in(x, T, "x"), _in(g, T, "grad_out")
        GAMMA, BETA = _in(gamma, F32, "gamma"), _in(beta, F32, "beta")
        MEAN, RSTD = _in(mean32, F32, "mean"), _in(rstd32, F32, "rstd")
        first = [None] * 5
        for code in CODES[storage]:
            what = f"ln {storage} C={C} cv={cv} rows={rows} code={code}"
            out, mean, rstd = _out(rows * C, T, "out"), _out(rows, F32, "mean"), _out(rows, F32, "rstd")
            _call("mu_ln_rows_fwd", O, X, GAMMA, BETA, out, mean, rstd, rows, C, cv, R.EPS, code)
            dY, gxh = _out(rows * C, T, "dY"), _out(rows * C, T, "g_xhat")
            _call("mu_ln_rows_bwd", G, O, X, MEAN, RSTD, GAMMA, dY, gxh, rows, C, cv, code)
            # (wholly written: an element left as the sentinel, -777, fails its bound below; the sentinel itself is a possible value
            #  of dY in fp16, so it is not searched for)
            got = [out.host((rows, C)), mean.host(), rstd.host(), dY.host((rows, C)), gxh.host((rows, C))]
            w["out"].check(what + " out", got[0], ref["out"], ref["out_b"])
            w["mean"].check(what + " mean", got[1], ref["mean"], ref["mean_b"])
            w["rstd"].check(what + " rstd", got[2], ref["rstd"], ref["rstd_b"])
            w["dY"].check(what + " dY", got[3], refb["dY"], refb["dY_b"])
            w["gxh"].check(what + " gxh", got[4], refb["gxh"], refb["gxh_b"])
            for k in (0, 3, 4):
                assert not got[k][:, cv:].any(), what + ": pad channels"
            first = [_repeat(f, a, what) for f, a in zip(first, got)]
    for v in w.values():
        v.note()


# ================================================================================================
# refusals: every condition of each entry point's first line, and a dtype code no storage type has
# ================================================================================================
def test_gather_scatter_refusals():
    src, _, idx = R.gather_inputs("f32", 8, 8, 4, 2)
    SRC, IDX, CNT = _in(src, F32, "src"), _in(idx, I32, "idx"), _cnt(2)
    dst = _out(4 * 8, F32, "dst")
    ok = dict(src=SRC, src_ld=8, idx=IDX, cnt=CNT, dst=dst, rows_out=4, C=8, dtype=MU_F32)
    for bad in (dict(src=None), dict(idx=None), dict(cnt=None), dict(dst=None), dict(rows_out=0), dict(rows_out=-1), dict(C=0), dict(C=-8),
                dict(src_ld=7), dict(dtype=BAD_DTYPE)):                          # null pointers, rows_out <= 0, C <= 0, src_ld < C
        _refused("mu_gather_rows", *{**ok, **bad}.values(), outs=(dst,))
    ok = dict(src=SRC, idx=IDX, cnt=CNT, dst=dst, dst_ld=8, dst_rows=4, C=8, dtype=MU_F32)
    for bad in (dict(src=None), dict(idx=None), dict(cnt=None), dict(dst=None), dict(dst_rows=0), dict(dst_rows=-1), dict(C=0), dict(C=-8),
                dict(dst_ld=7), dict(dtype=BAD_DTYPE)):                          # null pointers, dst_rows <= 0, C <= 0, dst_ld < C
        _refused("mu_scatter_rows", *{**ok, **bad}.values(), outs=(dst,))


def test_softmax_ds_refusals():
    S, D, CNT = _out(4 * 32, F32, "S"), _out(4 * 32, F32, "dP"), _cnt(3)
    P = _in(np.full((4, 32), 0.25, dtype=np.float32), F32, "P")
    ok = dict(S=S, N=4, ld=32, cnt=CNT, scale=1.0, dtype=MU_F32)
    for bad in (dict(S=None), dict(cnt=None), dict(N=0), dict(N=-1), dict(ld=0), dict(ld=-32), dict(dtype=BAD_DTYPE)):
        _refused("mu_softmax_rows", *{**ok, **bad}.values(), outs=(S,))          # null pointers, N <= 0, ld <= 0
    ok = dict(P=P, dP=D, N=4, ld=32, cnt=CNT, scale=1.0, dtype=MU_F32)
    for bad in (dict(P=None), dict(dP=None), dict(cnt=None), dict(N=0), dict(N=-1), dict(ld=0), dict(ld=-32), dict(dtype=BAD_DTYPE)):
        _refused("mu_attn_wide_ds", *{**ok, **bad}.values(), outs=(D,))


def test_ln_rows_refusals():
    o, x, g, gamma, beta, _ = R.ln_inputs("f32", 32, 24, 3)
    O, X, G = _in(o, F32, "o"), _in(x, F32, "x"), _in(g, F32, "grad_out")
    GAMMA, BETA = _in(gamma, F32, "gamma"), _in(beta, F32, "beta")
    MEAN, RSTD = _in(np.zeros(3, dtype=np.float32), F32, "mean"), _in(np.ones(3, dtype=np.float32), F32, "rstd")
    out, mean, rstd = _out(3 * 32, F32, "out"), _out(3, F32, "mean"), _out(3, F32, "rstd")
    dY, gxh = _out(3 * 32, F32, "dY"), _out(3 * 32, F32, "g_xhat")
    outs = (out, mean, rstd, dY, gxh)
    shape = (dict(rows=0), dict(rows=-1), dict(C=0), dict(C=-32), dict(c_valid=0), dict(c_valid=-1), dict(c_valid=33), dict(dtype=BAD_DTYPE))
    ok = dict(o=O, x=X, gamma=GAMMA, beta=BETA, out=out, mean=mean, rstd=rstd, rows=3, C=32, c_valid=24, eps=R.EPS, dtype=MU_F32)
    for bad in tuple({k: None} for k in ("o", "x", "gamma", "beta", "out", "mean", "rstd")) + shape:      # rows, C, c_valid <= 0, c_valid > C
        _refused("mu_ln_rows_fwd", *{**ok, **bad}.values(), outs=outs)
    ok = dict(grad_out=G, o=O, x=X, mean=MEAN, rstd=RSTD, gamma=GAMMA, dY=dY, g_xhat=gxh, rows=3, C=32, c_valid=24, dtype=MU_F32)
    for bad in tuple({k: None} for k in ("grad_out", "o", "x", "mean", "rstd", "gamma", "dY", "g_xhat")) + shape:
        _refused("mu_ln_rows_bwd", *{**ok, **bad}.values(), outs=outs)


# ================================================================================================
# block level: ops.mask_attention above 256 channels against the float64 closed form, at the project's own gate
# ================================================================================================
DT = {"f32": torch.float32, "f16": torch.float16}
PARAMS = (("query.weight", "wq"), ("query.bias", "bq"), ("key.weight", "wk"), ("key.bias", "bk"), ("value.weight", "wv"),
          ("value.bias", "bv"), ("norm.weight", "gamma"), ("norm.bias", "beta"))
_REF = {}


def _block_ref(name, storage):
    """the case and its float64 reference, computed once and shared"""
    if (name, storage) not in _REF:
        case = R.block_case(name, storage)
        _REF[name, storage] = (case, R.block_ref(case))
    return _REF[name, storage]


def _run_block(case, storage, monkeypatch, kidx=None):
    """ops.mask_attention with Linear / LayerNorm containers, scramble=False, kidx / kcnt as the case builds them; forward and backward.
    Returns torch tensors on the host: out, dx [B, N, C], the eight parameter gradients, and dqkv [B, N, 3C] (the tensor the
    projection bias gradients are summed from, picked up on its way into ops._colsum_wide)."""
    from maskunet_amd import ops
    dev, dtype = "cuda", DT[storage]
    B, H, W, N, cv = case["B"], case["H"], case["W"], case["N"], case["cv"]
    C = ops.attn_width(cv)
    assert C > 256 and C % 32 == 0 and C >= cv
    lin = {n: torch.nn.Linear(cv, cv) for n in ("query", "key", "value")}
    norm = torch.nn.LayerNorm(cv, eps=R.EPS)
    mods = dict(lin, norm=norm)
    with torch.no_grad():
        for pname, key in PARAMS:
            m, attr = pname.split(".")
            getattr(mods[m], attr).copy_(torch.from_numpy(case[key]))
    for m in mods.values():
        m.to(dev)
    x = torch.zeros((B, H, W, C), dtype=dtype)
    x[..., :cv] = torch.from_numpy(case["x"]).view(B, H, W, cv)
    x = x.to(dev).requires_grad_(True)
    gout = torch.zeros((B, N, C), dtype=dtype)
    gout[..., :cv] = torch.from_numpy(case["gout"])
    seen = []
    inner = ops._colsum_wide
    monkeypatch.setattr(ops, "_colsum_wide", lambda t: (seen.append(t.detach().clone()) if t.shape[1] == 3 * C else None, inner(t))[1])
    kidx = torch.from_numpy(case["kidx"] if kidx is None else kidx).to(dev)
    out = ops.mask_attention(x, lin["query"], lin["key"], lin["value"], norm, kidx, torch.from_numpy(case["kcnt"]).to(dev), scramble=False)
    assert out.shape == (B, N, C) and out.dtype == dtype
    out.backward(gout.to(dev))
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "_colsum_wide", inner)
    assert len(seen) == 1
    res = {"out": out.detach().cpu(), "dx": x.grad.view(B, N, C).cpu(), "dqkv": seen[0].view(B, N, 3 * C).cpu()}
    for pname, key in PARAMS:
        m, attr = pname.split(".")
        res[pname] = getattr(mods[m], attr).grad.cpu()
    return res


def _gate(tag, res, ref, case, storage):
    """per tensor as tests/_gpu_checks.check_attention gates it: _err for the output, _rel_err for every gradient, the absolute rule
    for key.bias (analytically zero); also the per-token dQ / dK / dV.  Prints every figure, then asserts."""
    from tests._gpu_checks import TOL, _err, _rel_err
    tol, cv, C = TOL[DT[storage]], case["cv"], res["out"].shape[-1]
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))          # noqa: E731
    rows = [("y", _err(res["out"][..., :cv], t(ref["out"])), tol), ("dx", _rel_err(res["dx"][..., :cv], t(ref["dx"])), tol)]
    for pname, key in PARAMS:
        if pname == "key.bias":
            rows.append(("d" + pname, float(res[pname].abs().max()), tol * float(np.abs(ref["dbq"]).max()) + 1e-6))
        else:
            rows.append(("d" + pname, _rel_err(res[pname], t(ref["d" + key])), tol))
    for i, k in enumerate(("dq", "dk", "dv")):
        rows.append((k, _rel_err(res["dqkv"][..., i * C:i * C + cv], t(ref[k])), tol))
    for n, e, tl in rows:
        print(f"attn-wide-edges block {tag} {storage} {n}: err {e:.3e} (tol {tl:.1e})")
    bad = [(n, e, tl) for n, e, tl in rows if not e <= tl]
    assert not bad, (tag, bad)


def _exact_zeros(tag, res, case):
    """masked keys' dK / dV rows are exactly zero; pad channels of out, dx and of dQ / dK / dV (the operands the padded parameter
    gradients are products and sums of) are exactly zero where cv < C"""
    B, N, cv = case["B"], case["N"], case["cv"]
    C = res["out"].shape[-1]
    for b in range(B):
        masked = torch.from_numpy(np.setdiff1d(np.arange(N), case["kidx"][b, :case["kcnt"][b]]))
        assert not res["dqkv"][b, masked, C:].any(), f"{tag}: dK / dV rows of masked keys, image {b}"
    if cv < C:
        assert not res["out"][..., cv:].any() and not res["dx"][..., cv:].any(), f"{tag}: pad channels of out / dx"
        for i in range(3):
            assert not res["dqkv"][..., i * C + cv:(i + 1) * C].any(), f"{tag}: pad channels of dqkv block {i}"
    for pname, key in PARAMS:
        assert tuple(res[pname].shape) == case[key].shape, (tag, pname)


def _sorted_keys(case):
    kidx = case["kidx"].copy()
    for b in range(case["B"]):
        kidx[b, :case["kcnt"][b]] = np.sort(kidx[b, :case["kcnt"][b]])
    return kidx


@pytest.mark.parametrize("storage", STORAGES)
def test_block_short_key_list_any_order(storage, monkeypatch):
    """C = 288, N = 64, kidx [B, 20] (nkmax < N, no multiple of 32: nk pads to 32), kept keys in random order and no promise of a
    permutation; the same call with the keys sorted agrees within the gate; a second run repeats every byte (no atomics)"""
    from tests._gpu_checks import TOL, _err, _rel_err
    case, ref = _block_ref("short_list", storage)
    res = _run_block(case, storage, monkeypatch)
    _gate("short_list", res, ref, case, storage)
    _exact_zeros("short_list", res, case)
    again = _run_block(case, storage, monkeypatch)
    for k in res:
        assert again[k].numpy().tobytes() == res[k].numpy().tobytes(), f"short_list {storage}: {k} differs between two runs"
    srt = _run_block(case, storage, monkeypatch, kidx=_sorted_keys(case))
    _gate("short_list, sorted keys", srt, ref, case, storage)
    tol = TOL[DT[storage]]
    for k in res:
        e = _err(srt[k], res[k]) if k == "out" else _rel_err(srt[k], res[k])
        if k == "key.bias":                                  # rounding noise around zero: compared at the size of query.bias' gradient
            e = float((srt[k] - res[k]).abs().max()) / float(res["query.bias"].abs().max())
        print(f"attn-wide-edges block short_list {storage} sorted vs random order {k}: {e:.3e} (tol {tol:.1e})")
        assert e <= tol, (k, e)


@pytest.mark.parametrize("name", ["n272", "cv520", "dominant"])
@pytest.mark.parametrize("storage", STORAGES)
def test_block_edges(storage, name, monkeypatch):
    """n272: N = 16 x 17 with 265 and 140 kept keys, every 256-strided loop takes a second pass inside the real composition.
    cv520: 520 channels stored at 544 -- the second 512-column block of ops._colsum_wide, K > 512 in the products, sliced parameter
    gradients.  dominant: one key with a raw score near 200 against every query (|q.k| <= 256, so that fp16 storage of the raw
    score stays inside the fp16 gate: half an ulp at 256, times 1 / sqrt(288), is under 4e-3)."""
    case, ref = _block_ref(name, storage)
    res = _run_block(case, storage, monkeypatch)
    _gate(name, res, ref, case, storage)
    _exact_zeros(name, res, case)


@pytest.mark.parametrize("storage", STORAGES)
def test_block_stale_score_columns(storage, monkeypatch):
    """a batch ordered kcnt = N, then 1, then 29: the reused S / dP buffers hold the columns of the image before.  The image with one
    visible key: P = 1, so dQ and dK are exactly zero and dV is nonzero in the kept row only."""
    case, ref = _block_ref("stale", storage)
    res = _run_block(case, storage, monkeypatch)
    _gate("stale", res, ref, case, storage)
    _exact_zeros("stale", res, case)
    C, N = res["out"].shape[-1], case["N"]
    assert case["kcnt"].tolist()[:2] == [N, 1]
    one = res["dqkv"][1]
    kept = int(case["kidx"][1, 0])
    assert not one[:, :2 * C].any(), "one visible key: dQ and dK must be exactly zero"
    others = torch.arange(N) != kept
    assert one[kept, 2 * C:].any() and not one[others, 2 * C:].any(), "one visible key: dV lives in the kept row only"
