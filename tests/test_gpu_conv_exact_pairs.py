"""Bit-exact convolution tests with LIVE lo halves: the split-operand arithmetic of fp32x and the full mantissa of exact fp32.

tests/test_gpu_conv_exact.py proves indexing, tiling, borders and workspaces on small integers, whose lo halves are zero.  Here the
operands are "pair values" a + b 2^-14 (tests/_conv_pair_cases.py: the recipe, its preconditions and the float64 reference), so that
  * fp32x must return conv(x, w) - conv(x_lo, w_lo): all three kept products lo hi + hi lo + hi hi and not the fourth (1x1: bf16 pairs;
    3x3: fp16 pairs, weights under the 2^6 shift), both terms of the data gradient on the HL weight rows (sum dy w), both column halves
    of the pair-summed weight gradient (sum dy x), and the one-term weight gradient the fp16 rounding of x and nothing else (sum dy a);
  * exact fp32 must return the full product when either operand carries 16 significant bits (each entry runs twice: pair activations
    against integer weights, and the reverse)
BIT FOR BIT: every kept partial sum is a multiple of 2^-14 below 2^10.  No tolerance is involved, except
  * ACT_GELU of the fused epilogue (float64 GELU of the exact pre-activation, at the integer file's tolerance) and
  * the statistics rows of mu_conv_fwd_stats, whose y^2 is not exact here: |sum of rows - sum y| <= (n + 2) 2^-24 sum |y| and
    |sum of rows - sum y^2| <= (n + 3) 2^-24 sum y^2 per channel, n = pixels per channel, both right-hand sides from the exact y.

Rows: the non-heavy rows of tests/_conv_cases.LAYERS (plus the cheapest heavy row of a kernel only heavy rows reach), one pytest id per
(entry, dtype, kernel, row).  Comparator, guarded buffers (NaN-filled outputs, sentinel row padding, 4 KiB guard bands, workspaces of
exactly the queried size), the ld padding rule and every entry the integer file already drives are imported from it.

The subnormal group: x = a + b 2^-20 -- fp16-subnormal lo halves, which the 3x3 fp32x forward and the pair-summed weight gradient must
keep ("22 mantissa bits down to an absolute floor of 2^-25") -- on one row per 3x3 forward kernel family and one mu_conv_wgrad_h row."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_cases as C
from tests import _conv_pair_cases as P
from tests.test_gpu_conv_exact import (Case, Guarded, TOL, _pad_c, assert_exact, run_dgrad_fp16, run_dgrad_h, run_fwd, run_wgrad,
                                       run_wgrad_h)

gpu = pytest.mark.gpu


def _f(t):
    assert P.exact32(t)
    return t.float()


def _case(r, dn, **ref):
    """A Case of the integer file on operands of the pair reference r (ref: the names its entries read -- x, w, b, dy, y0, dx, dw)."""
    return Case(r["c"], dn, {k: _f(v) for k, v in ref.items()})


def variants(r, dn, taps):
    """[(tag, streamed operand, partner, expected key)] an entry runs on the reference r of its scheme."""
    if dn == "fp32x":
        if r["scheme"].endswith("fwd") or (r["scheme"] == "wgrad" and taps == 1):
            return [("pairs", r["s"], r["p"], "three")]
        return [("dy one term", r["sa"], r["p"], "s_int")]                        # 3x3 backward: dy integers under a power-of-two scale
    return [("pairs x integers", r["s"], r["pa"], "p_int"), ("integers x pairs", r["sa"], r["p"], "s_int")]


# ------------------------------------------------------------------------------------------------
# the entries the integer file does not have in this form
# ------------------------------------------------------------------------------------------------
def run_fwd_stats(k, kernel):
    L, lib = k.L, k.lib
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, k.x_enc())
    w = k.weights(0)
    bias = k.bias()
    y = Guarded(k.M, k.Cout, k.y_ld, k.td)
    rows = lib.mu_conv_stats_rows(k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.code)
    part = Guarded(rows, k.Cout * 2, k.Cout * 2, torch.float32)
    L.call("mu_conv_fwd_stats", x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.ptr(), k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.x_ld, k.y_ld, k.code,
           part.ptr(), k.st)
    torch.cuda.synchronize()
    yr = k.y_ref(True)
    y.check("y")
    assert_exact(y.valid().float().view(k.B, k.H, k.W, k.Cout), yr, "bhwc", kernel)
    part.check("statistics rows")
    p = part.valid().view(rows, k.Cout, 2).cpu().double().sum(0)
    y64 = yr.reshape(-1, k.Cout).double()
    n, u = k.M, 2.0 ** -24
    e1, b1 = (p[:, 0] - y64.sum(0)).abs(), (n + 2) * u * y64.abs().sum(0)
    e2, b2 = (p[:, 1] - (y64 * y64).sum(0)).abs(), (n + 3) * u * (y64 * y64).sum(0)
    assert bool((e1 <= b1).all()), f"[{kernel}] sum: worst {float((e1 - b1).max()):.3e} beyond its bound"
    assert bool((e2 <= b2).all()), f"[{kernel}] sum of squares: worst {float((e2 - b2).max()):.3e} beyond its bound"


def _pair_rows(g, M, Cc, ld):
    """[M, ld] pair values a + b 2^-14 (|a| in {1, 2}) in the first Cc columns, zeros behind."""
    a = torch.randint(1, 3, (M, Cc), generator=g) * (2 * torch.randint(0, 2, (M, Cc), generator=g) - 1)
    out = torch.zeros(M, ld, dtype=torch.float64)
    out[:, :Cc] = a.double() + torch.randint(-3, 4, (M, Cc), generator=g).double() * P.E
    return out


def run_fused(k, kernel, tagv):
    L = k.L
    g = torch.Generator().manual_seed(k.M + k.Cout + 5)
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, k.x_enc())
    w = k.weights(0)
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0], dtype=torch.float64)[torch.randint(0, 4, (k.Cout,), generator=g)]
    shift = torch.randint(-3, 4, (k.Cout,), generator=g).double()
    rfull = _pair_rows(g, k.M, k.Cout, k.y_ld)
    res = rfull[:, :k.Cout]
    y0 = _pad_c(k.ref["y0"], k.Cout).reshape(k.M, k.Cout).double()

    def steps(sc):
        return y0 * sc, y0 * sc + shift, y0 * sc + shift + res
    # the epilogue's values must be fp32 values at every step (0.5 y: multiples of 2^-15, exact below 2^9 only): thin the scale
    bad = torch.zeros(k.Cout, dtype=torch.bool)
    for t in steps(scale):
        bad |= (t.float().double() != t).any(0)
    scale = torch.where(bad, torch.ones((), dtype=torch.float64), scale)
    sd, hd, rd = scale.float().cuda(), shift.float().cuda(), rfull.float().cuda()
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU):
        for use_res in (False, True):
            pre = steps(scale)[2 if use_res else 1]
            assert all(P.exact32(t) for t in steps(scale)), "precondition: the pre-activation is exact in fp32 at every step"
            y = Guarded(k.M, k.Cout, k.y_ld, k.td)
            L.call("mu_conv_fwd_fused", x.data_ptr(), w.data_ptr(), sd.data_ptr(), hd.data_ptr(), rd.data_ptr() if use_res else None, act, y.ptr(),
                   k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.x_ld, k.y_ld, k.code, k.st)
            torch.cuda.synchronize()
            y.check(f"y (act {act}, res {use_res})")
            got = y.valid().float().view(k.B, k.H, k.W, k.Cout)
            tag = f"{kernel} {tagv} act={act} res={use_res}"
            if act == L.ACT_GELU:
                ref = F.gelu(pre).view(k.B, k.H, k.W, k.Cout)
                assert bool(torch.isfinite(got).all()), tag
                err = float((got.cpu().double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
                assert err <= TOL[k.dn], f"[{tag}] GELU epilogue: {err:.3e} > {TOL[k.dn]:.1e}"
            else:
                ref = (pre.clamp(min=0) if act == L.ACT_RELU else pre).view(k.B, k.H, k.W, k.Cout)
                assert_exact(got, ref, "bhwc", tag)


def run_fwd_add(k, kernel):
    g = torch.Generator().manual_seed(k.M + k.Cout + 6)
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, "mu_split_encode")
    w = k.weights(0)
    afull = _pair_rows(g, k.M, k.Cout, k.y_ld)
    ref = _pad_c(k.ref["y0"], k.Cout).reshape(k.M, k.Cout).double() + afull[:, :k.Cout]
    assert P.exact32(ref), "precondition: conv + addend is an fp32 value"
    ad = afull.float().cuda()
    y = Guarded(k.M, k.Cout, k.y_ld, k.td)
    k.L.call("mu_conv1x1_fwd_add", x.data_ptr(), w.data_ptr(), ad.data_ptr(), y.ptr(), k.M, k.Cin, k.Cout, k.x_ld, k.y_ld, k.code, k.st)
    torch.cuda.synchronize()
    y.check("y")
    assert_exact(y.valid().view(k.B, k.H, k.W, k.Cout), ref.view(k.B, k.H, k.W, k.Cout), "bhwc", kernel)


def run_fwd_enc_h(k, kernel):
    """y written in the attention operand encoding: the mu_split_encode_h words of the exact y, compared as int32."""
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, "mu_split_encode")
    w = k.weights(0)
    bias = k.bias()
    for with_bias in (False, True):
        y = Guarded(k.M, k.Cout, k.y_ld, torch.float32)
        k.L.call("mu_conv1x1_fwd_enc_h", x.data_ptr(), w.data_ptr(), bias.data_ptr() if with_bias else None, y.ptr(), k.M, k.Cin, k.Cout, k.x_ld, k.y_ld, k.st)
        torch.cuda.synchronize()
        y.check("y")
        want = P.encode_h8(k.y_ref(with_bias).reshape(k.M, k.Cout))
        got = y.valid().contiguous().view(torch.int32).cpu()
        assert_exact(got.view(k.B, k.H, k.W, k.Cout), want.view(k.B, k.H, k.W, k.Cout), "bhwc", f"{kernel} bias={with_bias} (int32 words)")


# ------------------------------------------------------------------------------------------------
# one test per (entry, dtype, kernel, row)
# ------------------------------------------------------------------------------------------------
def run_entry(entry, dn, kernel, r):
    c = r["c"]
    for tagv, s, p, key in variants(r, dn, c["taps"]):
        want, kn = P.expected(r, key), f"{kernel} [{tagv}]"
        if entry in ("fwd", "fwd_stats", "fused", "fwd_add", "fwd_enc_h"):
            k = _case(r, dn, x=s, w=p, b=r["b"], y0=want)
            if entry == "fwd":
                run_fwd(k, kn, False)                      # without and with the integer bias
            elif entry == "fwd_stats":
                run_fwd_stats(k, kn)
            elif entry == "fused":
                run_fused(k, kernel, tagv)
            elif entry == "fwd_add":
                run_fwd_add(k, kn)
            else:
                run_fwd_enc_h(k, kn)
        elif entry == "dgrad":                             # exact fp32: mu_conv_fwd on mode-1 weights
            run_dgrad_fp16(_case(r, dn, dy=s, w=p, dx=want), kn)
        elif entry == "dgrad_h":
            run_dgrad_h(_case(r, dn, dy=s, w=p, dx=want), kn)
        elif entry == "wgrad":
            run_wgrad(_case(r, dn, dy=s, x=p, dw=want), kn, False)
        elif entry == "wgrad_h":
            run_wgrad_h(_case(r, dn, dy=s, x=p, dw=want), kn, False)
        elif entry == "wgrad_h1":                          # handed the fp16 rounding of the pair x: sum dy a
            run_wgrad_h(_case(r, dn, dy=s, x=p, dw=P.expected(r, "int")), kn, True)
        else:
            raise AssertionError(entry)


@functools.lru_cache(maxsize=1)
def _params():
    out = []
    for c, es in P.pair_rows():
        for entry, dn, op, kn in sorted(es, key=lambda e: P.SCHEME_OF[e[0]]):          # (one reference at a time stays cached)
            out.append(pytest.param(entry, dn, C.name_of(c), kn, id=f"{entry}-{dn}-{kn}-{C.name_of(c)}"))
    return out


def _sub_params():
    return [pytest.param(entry, name, kn, id=f"{entry}-fp32x-{kn}-{name}") for entry, kn, name in P.sub_rows()]


@gpu
@pytest.mark.parametrize("entry,dn,name,kernel", _params())
def test_exact_pairs(entry, dn, name, kernel):
    run_entry(entry, dn, kernel, P.pair_reference(name, P.SCHEME_OF[entry]))


@gpu
@pytest.mark.parametrize("entry,name,kernel", _sub_params())
def test_exact_subnormal_lo_halves(entry, name, kernel):
    run_entry(entry, "fp32x", kernel, P.pair_reference(name, "sub_" + P.SCHEME_OF[entry]))
