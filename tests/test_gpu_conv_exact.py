"""Bit-exact convolution tests on small integers, through the C ABI.

x in {-2..2}, w in {-1, 0, 1}, dy in {-2..2}, integer bias: every product and every partial sum, in any summation order, is an
integer below 2^24 (exact in fp32), every output an integer of at most 2048 (exact in fp16), the lo halves of every bf16 / fp16
pair are zero and the dy scale of the fp32x backward is a power of two.  A correct kernel of any tiling, split or pipeline depth
returns the CPU reference BIT FOR BIT; one wrong index is off by at least 1.  Each case checks these preconditions on the reference
alone before any GPU call (and thins x by a seeded fraction where a shape breaks one).

What zero lo halves cannot show -- the three split products of fp32x, the two-term gradients on HL rows and pair columns, the low
mantissa bits of exact fp32 -- is held bit for bit by tests/test_gpu_conv_exact_pairs.py, on operands a + b 2^-14 whose lo halves are
alive; it imports the comparator, the guarded buffers and the entries below.

Cases: tests/_conv_cases.LAYERS, one pytest id per (entry, dtype, kernel, shape); the kernel name comes from the mu_conv_*_plan
queries.  Memory discipline in every case: outputs pre-filled with NaN, row padding (ld - C columns) and 4 KiB guard bands before and
after every output and the workspace hold a sentinel that must survive, workspaces have exactly the queried size and start as NaN.

Behind the cases: the refusals of every mu_conv_* entry point (the documented status for each fault, one at a time, with every output
and guard band bit-unchanged) and the workspace boundary of every weight-gradient family (the smallest ws_bytes each accepts, found
by bisection inside a real buffer of the queried size and pinned in WS_FAMILIES, with the exact dW at exactly that size).

The module mark is per test (not `pytestmark`): the comparator self-tests at the end are CPU tests."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_cases as C

gpu = pytest.mark.gpu
SENT = 1234.0                    # exact in fp16 and fp32, outside every value the cases produce next to it
GUARD_BYTES = 4096
TORCH_DT = {"fp16": torch.float16, "fp32": torch.float32, "fp32x": torch.float32}
TOL = {"fp16": 3e-2, "fp32": 1e-3, "fp32x": 1e-3}        # tests/_gpu_checks.TOL (the GELU epilogue only)


# ------------------------------------------------------------------------------------------------
# comparator
# ------------------------------------------------------------------------------------------------
def mismatch_report(got, ref, layout, kernel):
    """None when got == ref bit for bit (as values; NaN never equals), else a report that locates the first difference.
    layout "bhwc": [B, H, W, C] activations; "oit": [O, I, taps] weight gradients; "c": per-channel vectors."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = ~(got.double() == ref.double())
    n = int(bad.sum())
    if n == 0:
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    where = ""
    if layout == "bhwc":
        b, h, w, c = idx
        where = f"(b, h, w, c) = {idx}: 16x16 tile (row {h // 16}, col {w // 16}), 8-row band {h // 8}, 64-channel block {c // 64}"
    elif layout == "oit":
        o, i, t = idx
        where = f"(o, i, tap) = {idx}: 64-channel blocks (out {o // 64}, in {i // 64})"
    else:
        where = f"index {idx}"
    return (f"[{kernel}] {n} of {bad.numel()} elements differ; first at {where}: expected {float(ref[idx])!r}, got {float(got[idx])!r}; "
            f"max |diff| {float((got.double() - ref.double())[bad].abs().nan_to_num(nan=float('inf')).max())}")


def assert_exact(got, ref, layout, kernel):
    r = mismatch_report(got, ref, layout, kernel)
    assert r is None, r


# ------------------------------------------------------------------------------------------------
# reference (CPU, fp32: exact on these integers) and its preconditions
# ------------------------------------------------------------------------------------------------
def make_ints(c, thin=0.0):
    g = torch.Generator().manual_seed(1000 * c["B"] + 31 * c["H"] + 7 * c["W"] + c["Cin"] + 3 * c["Cout"] + c["taps"])
    B, H, W, cin, cout, k = c["B"], c["H"], c["W"], c["cin"], c["cout"], 3 if c["taps"] == 9 else 1
    x = torch.randint(-2, 3, (B, cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, k, k), generator=g).float()
    b = torch.randint(-3, 4, (cout,), generator=g).float()
    dy = torch.randint(-2, 3, (B, cout, H, W), generator=g).float()
    if thin > 0:
        x = x * (torch.rand(x.shape, generator=g) >= thin)
    return x, w, b, dy


def _pad_c(t, C_):          # [B, c, H, W] -> [B, H, W, C_] with zero channels
    B, c, H, W = t.shape
    out = torch.zeros(B, H, W, C_)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


@functools.lru_cache(maxsize=2)
def reference(name, want_bwd):
    """Integer operands and exact results of the row `name`; asserts the exactness preconditions on them."""
    c = next(c for c in C.LAYERS if C.name_of(c) == name)
    k = 3 if c["taps"] == 9 else 1
    thin = 0.0
    while True:
        x, w, b, dy = make_ints(c, thin)
        y0 = F.conv2d(x, w, None, padding=k // 2)
        mass = F.conv2d(x.abs(), w.abs(), None, padding=k // 2)
        ok = float((y0.abs() + 3).max()) <= 2048 and float(mass.max()) < 2 ** 24
        if ok and c["taps"] == 9:        # statistics rows: sum of y^2 over any aligned 16 x 16 tile (bias included)
            yb = (y0 + b.view(1, -1, 1, 1)) ** 2
            tile = F.avg_pool2d(yb, 16, ceil_mode=True, divisor_override=1) if min(c["H"], c["W"]) >= 16 else yb.sum((2, 3))
            ok = float(tile.max()) < 2 ** 24
        r = dict(c=c, x=x, w=w, b=b, dy=dy, y0=y0, thin=thin)
        if ok and want_bwd:
            xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            F.conv2d(xr, wr, None, padding=k // 2).backward(dy)
            r["dx"], r["dw"], r["db"] = xr.grad, wr.grad, dy.sum((0, 2, 3))
            ok = float(r["dx"].abs().max()) <= 2048 and float(r["dw"].abs().max()) < 2 ** 24 and \
                float(F.conv2d(x.abs().transpose(0, 1), dy.abs().transpose(0, 1), padding=k // 2).max()) < 2 ** 24
        if ok:
            return r
        thin = 0.5 if thin == 0.0 else thin + (1 - thin) / 2          # zero a (larger) seeded fraction of x; the case is never dropped
        assert thin < 0.999, name


# ------------------------------------------------------------------------------------------------
# device buffers with guard bands
# ------------------------------------------------------------------------------------------------
class Guarded:
    """rows x ld elements of `dtype`: columns [0, cols) NaN, [cols, ld) sentinel, 4 KiB of sentinel before and after."""

    def __init__(self, rows, cols, ld, dtype):
        self.g = GUARD_BYTES // torch.empty(0, dtype=dtype).element_size()
        self.rows, self.cols, self.ld = rows, cols, ld
        self.buf = torch.full((2 * self.g + rows * ld,), SENT, dtype=dtype, device="cuda")
        self.body = self.buf[self.g:self.g + rows * ld].view(rows, ld)
        self.body[:, :cols] = float("nan")

    def ptr(self):
        return self.body.data_ptr()

    def valid(self):
        return self.body[:, :self.cols]

    def check(self, what):
        g = self.g
        assert bool((self.buf[:g] == SENT).all()), f"{what}: guard band BEFORE the buffer was written"
        assert bool((self.buf[g + self.rows * self.ld:] == SENT).all()), f"{what}: guard band AFTER the buffer was written"
        assert bool((self.body[:, self.cols:] == SENT).all()), f"{what}: row padding (columns >= {self.cols} of ld {self.ld}) was written"


class Case:
    """Device operands of one row in one dtype."""

    def __init__(self, c, dn, ref):
        from maskunet_amd import _lib
        self.L, self.lib, self.c, self.dn, self.ref = _lib, _lib.load(), c, dn, ref
        self.code, self.td = C.DTYPES[dn], TORCH_DT[dn]
        self.B, self.H, self.W, self.Cin, self.Cout, self.taps = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["taps"]
        self.M = self.B * self.H * self.W
        pad = 8 if (c["B"] + c["H"]) % 2 else 0         # every other row of the table runs with row strides larger than the channel counts
        self.x_ld, self.y_ld = self.Cin + pad, self.Cout + pad
        self.st = _lib.stream()

    def rows(self, t_nchw, C_, ld, encode=None, dtype=None):
        """[B, c, H, W] integers -> device rows [M, ld] (zero channel padding, zero row padding), optionally operand-encoded."""
        dtype = dtype or self.td
        host = torch.zeros(self.M, ld)
        host[:, :C_] = _pad_c(t_nchw, C_).reshape(self.M, C_)
        d = host.to("cuda", dtype)
        if encode:
            e = torch.empty_like(d)
            self.L.call(encode, d.data_ptr(), e.data_ptr(), d.numel(), self.st)
            return e
        return d

    def x_enc(self):
        return None if self.dn != "fp32x" else ("mu_split_encode_h4" if self.taps == 9 else "mu_split_encode")

    def weights(self, mode, code=None):
        c, code = self.c, self.code if code is None else code
        wd = self.ref["w"].contiguous().cuda()
        rp, cp = (self.Cout, self.Cin) if mode == 0 else (self.Cin, self.Cout)          # mode 1: rows = input channels
        dst = torch.empty(self.taps * rp * cp, dtype=self.td, device="cuda")
        self.L.call("mu_prep_weight", wd.data_ptr(), dst.data_ptr(), code, c["cout"], c["cin"], self.taps, rp, cp, mode, self.st)
        return dst

    def bias(self):
        b = torch.zeros(self.Cout)
        b[:self.c["cout"]] = self.ref["b"]
        return b.cuda()

    def y_ref(self, with_bias):
        y = _pad_c(self.ref["y0"] + (self.ref["b"].view(1, -1, 1, 1) if with_bias else 0), self.Cout)
        return y


def _case(name, dn, want_bwd):
    ref = reference(name, want_bwd)
    return Case(ref["c"], dn, ref)


def _params():
    out = []
    for c in C.LAYERS:
        for entry, dn, op, pid in C.entries(c):
            out.append(pytest.param(entry, dn, C.name_of(c), C.plan_name(op, pid), id=f"{entry}-{dn}-{C.plan_name(op, pid)}-{C.name_of(c)}"))
    return out


# ------------------------------------------------------------------------------------------------
# the entries
# ------------------------------------------------------------------------------------------------
def run_fwd(k, kernel, stats):
    L, lib = k.L, k.lib
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, k.x_enc())
    w = k.weights(0)
    bias = k.bias()
    for with_bias in ((True,) if stats else (False, True)):
        y = Guarded(k.M, k.Cout, k.y_ld, k.td)
        bp = bias.data_ptr() if with_bias else None
        if stats:
            rows = lib.mu_conv_stats_rows(k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.code)
            part = Guarded(rows, k.Cout * 2, k.Cout * 2, torch.float32)
            L.call("mu_conv_fwd_stats", x.data_ptr(), w.data_ptr(), bp, y.ptr(), k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.x_ld, k.y_ld, k.code,
                   part.ptr(), k.st)
        else:
            L.call("mu_conv_fwd", x.data_ptr(), w.data_ptr(), bp, y.ptr(), k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.x_ld, k.y_ld, k.code, k.st)
        torch.cuda.synchronize()
        yr = k.y_ref(with_bias)
        y.check("y")
        assert_exact(y.valid().float().view(k.B, k.H, k.W, k.Cout), yr, "bhwc", kernel)
        if stats:
            part.check("statistics rows")
            p = part.valid().view(rows, k.Cout, 2).cpu()
            assert bool((p == p.round()).all()), f"[{kernel}] a statistics row is not an integer"
            y64 = yr.reshape(-1, k.Cout).to(torch.int64)
            assert_exact(p[:, :, 0].to(torch.int64).sum(0), y64.sum(0), "c", kernel + " sum")
            assert_exact(p[:, :, 1].to(torch.int64).sum(0), (y64 * y64).sum(0), "c", kernel + " sum of squares")


def run_dgrad_fp16(k, kernel):
    """mu_conv_fwd on mode-1 weights, no statistics: dx[M, Cin] from dy[M, Cout]."""
    dy = k.rows(k.ref["dy"], k.Cout, k.y_ld)
    w = k.weights(1)
    dx = Guarded(k.M, k.Cin, k.x_ld, k.td)
    k.L.call("mu_conv_fwd", dy.data_ptr(), w.data_ptr(), None, dx.ptr(), k.B, k.H, k.W, k.Cout, k.Cin, k.taps, k.y_ld, k.x_ld, k.code, k.st)
    torch.cuda.synchronize()
    dx.check("dx")
    assert_exact(dx.valid().float().view(k.B, k.H, k.W, k.Cin), _pad_c(k.ref["dx"], k.Cin), "bhwc", kernel)


def run_fused(k, kernel):
    L = k.L
    g = torch.Generator().manual_seed(k.M + k.Cout)
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, k.x_enc())
    w = k.weights(0)
    scale = torch.tensor([0.5, 1.0, 2.0, -1.0])[torch.randint(0, 4, (k.Cout,), generator=g)]
    shift = torch.randint(-3, 4, (k.Cout,), generator=g).float()
    res = torch.randint(-2, 3, (k.M, k.Cout), generator=g).float()
    y0 = _pad_c(k.ref["y0"], k.Cout).reshape(k.M, k.Cout)
    # the epilogue's values must be exact in the storage type too (0.5 y: half-integers -- fp16 holds them below 1024): thin the scale
    if k.td == torch.float16:
        scale = torch.where((y0.abs().max(0).values >= 1000) & (scale == 0.5), torch.ones(()), scale)
        scale = torch.where((y0.abs().max(0).values >= 1000) & (scale == 2.0), torch.ones(()), scale)
    sd, hd = scale.cuda(), shift.cuda()
    rfull = torch.zeros(k.M, k.y_ld)
    rfull[:, :k.Cout] = res
    rd = rfull.to("cuda", k.td)
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU):
        for use_res in (False, True):
            pre = y0 * scale + shift + (res if use_res else 0)
            assert torch.equal(pre.to(k.td).float(), pre), "precondition: the pre-activation is exact in the storage type"
            y = Guarded(k.M, k.Cout, k.y_ld, k.td)
            L.call("mu_conv_fwd_fused", x.data_ptr(), w.data_ptr(), sd.data_ptr(), hd.data_ptr(), rd.data_ptr() if use_res else None, act, y.ptr(),
                   k.B, k.H, k.W, k.Cin, k.Cout, k.taps, k.x_ld, k.y_ld, k.code, k.st)
            torch.cuda.synchronize()
            y.check(f"y (act {act}, res {use_res})")
            got = y.valid().float().view(k.B, k.H, k.W, k.Cout)
            tag = f"{kernel} act={act} res={use_res}"
            if act == L.ACT_GELU:
                ref = F.gelu(pre.double()).view(k.B, k.H, k.W, k.Cout)
                assert bool(torch.isfinite(got).all()), tag
                err = float((got.cpu().double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
                assert err <= TOL[k.dn], f"[{tag}] GELU epilogue: {err:.3e} > {TOL[k.dn]:.1e}"
            else:
                ref = (pre.clamp(min=0) if act == L.ACT_RELU else pre).view(k.B, k.H, k.W, k.Cout)
                assert_exact(got, ref, "bhwc", tag)


def _workspace(nbytes):
    ws = Guarded(1, nbytes // 4, nbytes // 4, torch.float32)
    assert nbytes % 4 == 0 and nbytes > 0
    return ws


def _dw_ref(k):
    return k.ref["dw"].reshape(k.c["cout"], k.c["cin"], k.taps)


def run_wgrad(k, kernel, with_bias):
    L, lib, c = k.L, k.lib, k.c
    enc = "mu_split_encode" if k.dn == "fp32x" else None          # (fp32x reaches mu_conv_wgrad with 1x1 layers only)
    x = k.rows(k.ref["x"], k.Cin, k.x_ld, enc)
    dy = k.rows(k.ref["dy"], k.Cout, k.y_ld, enc)
    nws = lib.mu_conv_wgrad_workspace_bytes(k.B, k.H, k.W, k.Cin, k.Cout, k.taps)
    ws = _workspace(nws)
    dw = Guarded(1, c["cout"] * c["cin"] * k.taps, c["cout"] * c["cin"] * k.taps, torch.float32)
    if with_bias:
        db = Guarded(1, c["cout"], c["cout"], torch.float32)
        L.call("mu_conv_wgrad_bias", x.data_ptr(), dy.data_ptr(), dw.ptr(), db.ptr(), k.B, k.H, k.W, k.Cin, k.Cout, k.taps, c["cin"], c["cout"],
               k.x_ld, k.y_ld, ws.ptr(), nws, k.code, k.st)
    else:
        L.call("mu_conv_wgrad", x.data_ptr(), dy.data_ptr(), dw.ptr(), k.B, k.H, k.W, k.Cin, k.Cout, k.taps, c["cin"], c["cout"], k.x_ld, k.y_ld,
               ws.ptr(), nws, k.code, k.st)
    torch.cuda.synchronize()
    ws.check("workspace")
    dw.check("dW")
    assert_exact(dw.valid().view(c["cout"], c["cin"], k.taps), _dw_ref(k), "oit", kernel)
    if with_bias:
        db.check("db")
        assert_exact(db.valid().view(-1), k.ref["db"], "c", kernel + " db")


def _dy_h(k):
    """mu_dy_encode_h on the plain fp32 dy rows: (halves [M, Cout], scale pair); the scale a power of two, the halves exact."""
    L, lib = k.L, k.lib
    dy = k.rows(k.ref["dy"], k.Cout, k.Cout, dtype=torch.float32)
    out = torch.empty(dy.numel(), dtype=torch.float16, device="cuda")
    sc = torch.empty(2, device="cuda")
    ws0 = torch.empty(lib.mu_dy_encode_h_workspace_bytes(), dtype=torch.uint8, device="cuda")
    L.call("mu_dy_encode_h", dy.data_ptr(), out.data_ptr(), sc.data_ptr(), dy.numel(), ws0.data_ptr(), ws0.numel(), k.st)
    S, inv = float(sc[0]), float(sc[1])
    assert S > 0 and S * inv == 1.0 and math.log2(S) == int(math.log2(S)), S
    assert torch.equal(out.float() * inv, dy.view(-1)), "dy_h / S must reproduce the integer dy exactly"
    return out, sc


def run_dgrad_h(k, kernel):
    dyh, sc = _dy_h(k)
    whl = k.weights(1, C.DTYPES["fp32x"])
    dx = Guarded(k.M, k.Cin, k.Cin + (k.x_ld - k.Cin) // 2, torch.float32)
    k.L.call("mu_conv_dgrad_h", dyh.data_ptr(), whl.data_ptr(), sc.data_ptr(), dx.ptr(), k.B, k.H, k.W, k.Cout, k.Cin, k.Cout, dx.ld, k.st)
    torch.cuda.synchronize()
    dx.check("dx")
    assert_exact(dx.valid().view(k.B, k.H, k.W, k.Cin), _pad_c(k.ref["dx"], k.Cin), "bhwc", kernel)


def run_wgrad_h(k, kernel, one_term):
    L, lib, c = k.L, k.lib, k.c
    dyh, sc = _dy_h(k)
    xd = k.rows(k.ref["x"], k.Cin, k.Cin, dtype=torch.float32)
    xe, x16 = torch.empty_like(xd), torch.empty(xd.shape, dtype=torch.float16, device="cuda")
    L.call("mu_split_encode_h4x", xd.data_ptr(), xe.data_ptr(), x16.data_ptr(), xd.numel(), k.st)
    nws = lib.mu_conv_wgrad_workspace_bytes(k.B, k.H, k.W, k.Cin, k.Cout, 9) if one_term else lib.mu_conv_wgrad_h_workspace_bytes(k.B, k.H, k.W, k.Cin, k.Cout)
    ws = _workspace(nws)
    dw = Guarded(1, c["cout"] * c["cin"] * 9, c["cout"] * c["cin"] * 9, torch.float32)
    L.call("mu_conv_wgrad_h1" if one_term else "mu_conv_wgrad_h", (x16 if one_term else xe).data_ptr(), dyh.data_ptr(), sc.data_ptr(), dw.ptr(),
           k.B, k.H, k.W, k.Cin, k.Cout, c["cin"], c["cout"], k.Cin, k.Cout, ws.ptr(), nws, k.st)
    torch.cuda.synchronize()
    ws.check("workspace")
    dw.check("dW")
    assert_exact(dw.valid().view(c["cout"], c["cin"], 9), _dw_ref(k), "oit", kernel)


@gpu
@pytest.mark.parametrize("entry,dn,name,kernel", _params())
def test_exact(entry, dn, name, kernel):
    k = _case(name, dn, entry not in ("fwd", "fwd_stats", "fused"))
    if entry == "fwd":
        run_fwd(k, kernel, False)
    elif entry == "fwd_stats":
        run_fwd(k, kernel, True)
    elif entry == "dgrad":
        run_dgrad_fp16(k, kernel)
    elif entry == "fused":
        run_fused(k, kernel)
    elif entry in ("wgrad", "wgrad_bias"):
        run_wgrad(k, kernel, entry == "wgrad_bias")
    elif entry == "dgrad_h":
        run_dgrad_h(k, kernel)
    elif entry in ("wgrad_h", "wgrad_h1"):
        run_wgrad_h(k, kernel, entry == "wgrad_h1")
    else:
        raise AssertionError(entry)


# ------------------------------------------------------------------------------------------------
# refusals: the documented status, and nothing written.  Every buffer is real and sized for the valid call.
# ------------------------------------------------------------------------------------------------
ARG, SHAPE, WORKSPACE = -1, -2, -4
ENTRY_ARGS = {
    "mu_conv_fwd": "x w bias y B H W Cin Cout taps x_ld y_ld dtype st",
    "mu_conv_fwd_stats": "x w bias y B H W Cin Cout taps x_ld y_ld dtype stat st",
    "mu_conv_fwd_fused": "x w scale bias res act y B H W Cin Cout taps x_ld y_ld dtype st",
    "mu_conv_dgrad_h": "x w dys y B H W Cin Cout x_ld y_ld st",
    "mu_conv1x1_fwd_add": "x w res y M Cin Cout x_ld y_ld dtype st",
    "mu_conv1x1_fwd_enc_h": "x w bias y M Cin Cout x_ld y_ld st",
    "mu_conv_wgrad": "x dy dw B H W Cin Cout taps cin_valid cout_valid x_ld y_ld ws ws_bytes dtype st",
    "mu_conv_wgrad_bias": "x dy dw db B H W Cin Cout taps cin_valid cout_valid x_ld y_ld ws ws_bytes dtype st",
    "mu_conv_wgrad_h": "x dy dys dw B H W Cin Cout cin_valid cout_valid x_ld y_ld ws ws_bytes st",
    "mu_conv_wgrad_h1": "x dy dys dw B H W Cin Cout cin_valid cout_valid x_ld y_ld ws ws_bytes st",
}


class EntryCall:
    """An entry point on one row: .a = its valid arguments by name, .outs = its Guarded outputs, .status(**changes) = the code it
    returns with those arguments replaced.  Inputs are zeros (fp32-sized, so large enough in every dtype)."""

    def __init__(self, fn, name, dn, out_dtype, ws_bytes=0, stat_rows=0):
        k = self.k = _case(name, dn, False)
        c = k.c
        self.fn, M = fn, k.M
        zeros = lambda n: torch.zeros(n, device="cuda")
        self.outs = {"y": Guarded(M, k.Cout, k.y_ld, out_dtype), "dw": Guarded(1, c["cout"] * c["cin"] * k.taps, c["cout"] * c["cin"] * k.taps, torch.float32),
                     "db": Guarded(1, c["cout"], c["cout"], torch.float32), "ws": _workspace(max(ws_bytes, 4)),
                     "stat": Guarded(max(stat_rows, 1), 2 * k.Cout, 2 * k.Cout, torch.float32)}
        self.keep = [zeros(M * k.x_ld), zeros(2 * k.taps * k.Cin * k.Cout), zeros(k.Cout), zeros(k.Cout), zeros(M * k.y_ld), zeros(M * k.y_ld),
                     torch.ones(2, device="cuda")]
        x, w, bias, scale, res, dy, dys = (t.data_ptr() for t in self.keep)
        self.a = dict(x=x, w=w, bias=bias, scale=scale, res=res, dy=dy, dys=dys, act=k.L.ACT_RELU, B=k.B, H=k.H, W=k.W, M=M, Cin=k.Cin, Cout=k.Cout,
                      taps=k.taps, cin_valid=c["cin"], cout_valid=c["cout"], x_ld=k.x_ld, y_ld=k.y_ld, dtype=k.code, st=k.st, ws_bytes=ws_bytes,
                      **{n: g.ptr() for n, g in self.outs.items()})

    def status(self, **changes):
        a = dict(self.a, **changes)
        return getattr(self.k.lib, self.fn)(*[a[n] for n in ENTRY_ARGS[self.fn].split()])

    def refuses(self, expected, **changes):
        """The call with `changes` returns `expected` and leaves every output, its row padding and its guard bands bit-unchanged."""
        for g in self.outs.values():
            g.body[:] = SENT
        before = {n: g.buf.clone() for n, g in self.outs.items()}
        rc = self.status(**changes)
        torch.cuda.synchronize()
        assert rc == expected, f"{self.fn} with {changes}: status {rc}, documented {expected}"
        for n, g in self.outs.items():
            assert torch.equal(g.buf.view(torch.uint8), before[n].view(torch.uint8)), f"{self.fn} with {changes}: refused, but wrote `{n}`"


def _common_faults(e, nulls, sizes, taps_code=ARG, dtype_code=ARG, cin0_code=SHAPE, yld_step=4):
    """The faults every entry shares, one at a time: null pointers and non-positive sizes (MU_ERR_ARG), then channel counts and row
    strides (MU_ERR_SHAPE)."""
    a = e.a
    for n in nulls:
        e.refuses(ARG, **{n: None})
    for n, bad in sizes:
        e.refuses(ARG, **{n: bad})
    e.refuses(cin0_code, Cin=0)
    e.refuses(SHAPE, Cin=a["Cin"] + 16)
    e.refuses(SHAPE, Cout=a["Cout"] + 16)
    e.refuses(SHAPE, x_ld=a["Cin"] - 8)
    e.refuses(SHAPE, x_ld=a["x_ld"] + (2 if e.fn == "mu_conv_wgrad_h" else 4))      # (that entry doubles x_ld: the 16-bit view)
    e.refuses(SHAPE, y_ld=a["Cout"] - 8)
    e.refuses(SHAPE, y_ld=a["y_ld"] + yld_step)
    if "taps" in ENTRY_ARGS[e.fn].split():
        e.refuses(taps_code, taps=3)
    if "dtype" in ENTRY_ARGS[e.fn].split():
        e.refuses(dtype_code, dtype=7)


BHW = [("B", 0), ("H", -1), ("W", 0)]
ROWS_M = [("M", 0), ("M", 2 ** 31)]


@gpu
def test_forward_entries_refuse_with_the_documented_status_and_write_nothing():
    from maskunet_amd import _lib
    lib = _lib.load()
    row, f16 = "2x8x16_64to64_k3", torch.float16
    e = EntryCall("mu_conv_fwd", row, "fp16", f16)
    assert e.status() == 0
    _common_faults(e, ["x", "w", "y"], BHW)
    rows = lib.mu_conv_stats_rows(2, 8, 16, 64, 64, 9, 1)
    assert rows > 0
    e = EntryCall("mu_conv_fwd_stats", row, "fp16", f16, stat_rows=rows)
    assert e.status() == 0
    # (a tap count or a dtype without statistics rows is "no statistics rows for this shape": MU_ERR_SHAPE, before taps is looked at)
    _common_faults(e, ["x", "w", "y"], BHW, taps_code=SHAPE, dtype_code=SHAPE)
    e.refuses(SHAPE, dtype=0)
    e.refuses(ARG, stat=None, taps=3)
    e = EntryCall("mu_conv_fwd_stats", "2x9x7_64to64_k3", "fp16", f16)          # a shape without statistics rows
    assert lib.mu_conv_stats_rows(2, 9, 7, 64, 64, 9, 1) == 0 and e.status(stat=None) == 0
    e.refuses(SHAPE)
    e.refuses(SHAPE, taps=3)
    e.refuses(ARG, taps=3, x=None)
    e = EntryCall("mu_conv_fwd_fused", row, "fp16", f16)
    assert e.status() == 0
    _common_faults(e, ["x", "w", "y"], BHW)
    e.refuses(ARG, act=e.k.L.ACT_RELU + 1)
    e.refuses(ARG, act=e.k.L.ACT_NONE - 1)
    e.refuses(SHAPE, act=99, Cout=80)                       # the shape is looked at before the activation
    e = EntryCall("mu_conv_dgrad_h", row, "fp32x", torch.float32)
    assert e.status() == 0
    _common_faults(e, ["x", "w", "dys", "y"], BHW, yld_step=2)
    row1 = "1x16x16_64to64_k1"
    e = EntryCall("mu_conv1x1_fwd_add", row1, "fp16", f16)
    assert e.status() == 0
    _common_faults(e, ["x", "w", "res", "y"], ROWS_M, dtype_code=SHAPE)
    e.refuses(SHAPE, Cout=96, y_ld=96)                      # a multiple of 32, not of 64
    e = EntryCall("mu_conv1x1_fwd_enc_h", row1, "fp32x", torch.float32)
    assert e.status() == 0
    _common_faults(e, ["x", "w", "y"], ROWS_M)
    e.refuses(SHAPE, Cout=96, y_ld=96)


@gpu
def test_weight_gradient_entries_refuse_with_the_documented_status_and_write_nothing():
    from maskunet_amd import _lib
    lib = _lib.load()
    # (Cin = 0 passes the multiple-of-32 check and fails 0 < cin_valid <= Cin: MU_ERR_ARG)
    row = "1x16x16_64to64_k1"
    nws = lib.mu_conv_wgrad_workspace_bytes(1, 16, 16, 64, 64, 1)
    e = EntryCall("mu_conv_wgrad", row, "fp16", torch.float32, ws_bytes=nws)
    assert e.status() == 0
    valid = [("cin_valid", 0), ("cin_valid", 65), ("cout_valid", 0), ("cout_valid", 65)]
    _common_faults(e, ["x", "dy", "dw", "ws"], BHW + valid, cin0_code=ARG)
    e.refuses(WORKSPACE, ws_bytes=0)
    e.refuses(WORKSPACE, ws_bytes=WS_SMALLEST[("wgrad", row)] - 1)
    e.refuses(SHAPE, Cin=80, taps=3)                        # the shape is looked at before taps
    # db on a shape without bias partials: MU_ERR_SHAPE, even when taps is bad
    e = EntryCall("mu_conv_wgrad_bias", row, "fp16", torch.float32, ws_bytes=nws)
    assert lib.mu_conv_wgrad_bias_supported(64, 64, 1, 1) == 0
    e.refuses(SHAPE)
    e.refuses(SHAPE, taps=3)
    e.refuses(ARG, db=None)
    e.refuses(ARG, taps=3, x=None)
    rowb = "2x9x7_64to192_k1"
    nws = lib.mu_conv_wgrad_workspace_bytes(2, 9, 7, 64, 192, 1)
    e = EntryCall("mu_conv_wgrad_bias", rowb, "fp16", torch.float32, ws_bytes=nws)
    assert e.status() == 0
    valid = [("cin_valid", 0), ("cin_valid", 65), ("cout_valid", 0), ("cout_valid", 193)]
    _common_faults(e, ["x", "dy", "dw", "db", "ws"], BHW + valid, taps_code=SHAPE, dtype_code=SHAPE, cin0_code=ARG)
    e.refuses(SHAPE, dtype=0)
    e.refuses(WORKSPACE, ws_bytes=0)
    e.refuses(WORKSPACE, ws_bytes=WS_SMALLEST[("wgrad", rowb)])               # the slabs fit, the bias partials do not
    e.refuses(WORKSPACE, ws_bytes=WS_SMALLEST[("wgrad_bias", rowb)] - 1)
    rowh = "1x10x6_19to32_k3"
    for fn, entry, q in (("mu_conv_wgrad_h", "wgrad_h", lib.mu_conv_wgrad_h_workspace_bytes(1, 10, 6, 32, 32)),
                         ("mu_conv_wgrad_h1", "wgrad_h1", lib.mu_conv_wgrad_workspace_bytes(1, 10, 6, 32, 32, 9))):
        e = EntryCall(fn, rowh, "fp32x", torch.float32, ws_bytes=q)
        assert e.status() == 0
        two_term = entry == "wgrad_h"
        valid = [("cin_valid", 0), ("cin_valid", 3), ("cout_valid", 0), ("cout_valid", 33), ("dys", None)]
        _common_faults(e, ["x", "dy", "dw", "ws"], BHW + valid, cin0_code=SHAPE if two_term else ARG)
        e.refuses(SHAPE if two_term else ARG, cin_valid=33)
        e.refuses(ARG, dys=None, Cin=48)                    # the scale pair and the first-layer bound come first
        e.refuses(WORKSPACE, ws_bytes=0)
        e.refuses(WORKSPACE, ws_bytes=WS_SMALLEST[(entry, rowh)] - 1)


# ------------------------------------------------------------------------------------------------
# the workspace boundary of every weight-gradient family
# ------------------------------------------------------------------------------------------------
# (plan, entry, row, smallest ws_bytes the entry accepts): the sizes written down from the library of the commit before the host-layer
# refactor of conv.hip, the way MODEL_PLANS was.  The first-layer kernels run from one [9][Cout][4] slab on; the others need every slab
# of their plan (and the wide tiles with db their bias partials behind them), which may be less than the one size the query reserves.
WS_FAMILIES = [
    ("rgb_fma", "wgrad", "1x8x8_1to64_k3", 9216),
    ("rgb2_npt5", "wgrad", "1x3x160_3to64_k3", 9216),
    ("wgrad9_npt4", "wgrad", "1x6x128_64to64_k3", 884736),
    ("wgrad9_w16", "wgrad", "1x8x16_128to64_k3", 1179648),
    ("wgrad3_128", "wgrad", "1x5x96_128to128_k3", 589824),
    ("wgrad3_64", "wgrad", "1x6x160_64to64_k3", 294912),
    ("wide192_ci64", "wgrad", "2x9x7_64to192_k1", 49152),
    ("wide192_ci64_bias", "wgrad_bias", "2x9x7_64to192_k1", 49920),
    ("gen64", "wgrad", "1x16x16_64to64_k1", 16384),
    ("gen32", "wgrad_h", "1x10x6_19to32_k3", 73728),
    ("gen32", "wgrad_h1", "1x10x6_19to32_k3", 36864),
]
WS_SMALLEST = {(entry, row): n for _, entry, row, n in WS_FAMILIES}


def _wgrad_entry(k, entry):
    """(queried workspace bytes, call(dw, db, ws, ws_bytes) -> status) of a weight-gradient entry on the integer operands of the case k."""
    L, lib, c = k.L, k.lib, k.c
    if entry in ("wgrad", "wgrad_bias"):
        x, dy = k.rows(k.ref["x"], k.Cin, k.x_ld), k.rows(k.ref["dy"], k.Cout, k.y_ld)
        nws = lib.mu_conv_wgrad_workspace_bytes(k.B, k.H, k.W, k.Cin, k.Cout, k.taps)
        tail = (k.B, k.H, k.W, k.Cin, k.Cout, k.taps, c["cin"], c["cout"], k.x_ld, k.y_ld)
        if entry == "wgrad":
            return nws, lambda dw, db, ws, n: lib.mu_conv_wgrad(x.data_ptr(), dy.data_ptr(), dw.ptr(), *tail, ws.ptr(), n, k.code, k.st)
        return nws, lambda dw, db, ws, n: lib.mu_conv_wgrad_bias(x.data_ptr(), dy.data_ptr(), dw.ptr(), db.ptr(), *tail, ws.ptr(), n, k.code, k.st)
    dyh, sc = _dy_h(k)
    xd = k.rows(k.ref["x"], k.Cin, k.Cin, dtype=torch.float32)
    xe, x16 = torch.empty_like(xd), torch.empty(xd.shape, dtype=torch.float16, device="cuda")
    L.call("mu_split_encode_h4x", xd.data_ptr(), xe.data_ptr(), x16.data_ptr(), xd.numel(), k.st)
    tail = (k.B, k.H, k.W, k.Cin, k.Cout, c["cin"], c["cout"], k.Cin, k.Cout)
    if entry == "wgrad_h":
        return (lib.mu_conv_wgrad_h_workspace_bytes(k.B, k.H, k.W, k.Cin, k.Cout),
                lambda dw, db, ws, n: lib.mu_conv_wgrad_h(xe.data_ptr(), dyh.data_ptr(), sc.data_ptr(), dw.ptr(), *tail, ws.ptr(), n, k.st))
    return (lib.mu_conv_wgrad_workspace_bytes(k.B, k.H, k.W, k.Cin, k.Cout, 9),
            lambda dw, db, ws, n: lib.mu_conv_wgrad_h1(x16.data_ptr(), dyh.data_ptr(), sc.data_ptr(), dw.ptr(), *tail, ws.ptr(), n, k.st))


@gpu
@pytest.mark.parametrize("plan,entry,name,smallest", WS_FAMILIES, ids=[f"{e}-{p}-{r}" for p, e, r, _ in WS_FAMILIES])
def test_workspace_boundary(plan, entry, name, smallest):
    k = _case(name, "fp32x" if entry in ("wgrad_h", "wgrad_h1") else "fp16", True)
    c = k.c
    pid = {"wgrad": lambda: k.lib.mu_conv_wgrad_plan(k.B, k.H, k.W, k.Cin, k.Cout, k.taps, c["cin"], 1, 0),
           "wgrad_bias": lambda: k.lib.mu_conv_wgrad_bias_plan(k.B, k.H, k.W, k.Cin, k.Cout, k.taps, c["cin"], 1),
           "wgrad_h": lambda: k.lib.mu_conv_wgrad_plan(k.B, k.H, k.W, k.Cin, k.Cout, 9, c["cin"], 1, 1),
           "wgrad_h1": lambda: k.lib.mu_conv_wgrad_plan(k.B, k.H, k.W, k.Cin, k.Cout, 9, c["cin"], 1, 0)}[entry]()
    assert C.plan_name("wgrad", pid) == plan
    query, call = _wgrad_entry(k, entry)
    n_dw = c["cout"] * c["cin"] * k.taps
    fresh = lambda: (Guarded(1, n_dw, n_dw, torch.float32), Guarded(1, c["cout"], c["cout"], torch.float32), _workspace(query))
    # bisection between 0 (refused) and the query (accepted): every probe is a refusal or a complete valid call inside the real buffer
    dw, db, ws = fresh()
    probes = {0: call(dw, db, ws, 0), query: call(dw, db, ws, query)}
    assert probes[0] == WORKSPACE and probes[query] == 0, probes
    lo, hi = 0, query
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        probes[mid] = call(dw, db, ws, mid)
        assert probes[mid] in (0, WORKSPACE), (mid, probes[mid])
        lo, hi = (lo, mid) if probes[mid] == 0 else (mid, hi)
    for n in (min(hi + 4, query), (hi + query) // 2):      # accepted sizes the bisection may not have visited
        probes[n] = call(dw, db, ws, n)
    torch.cuda.synchronize()
    print(f"{entry} {plan} {name}: smallest accepted workspace {hi} of {query} queried, {len(probes)} probes")
    refused, accepted = [n for n, rc in probes.items() if rc], [n for n, rc in probes.items() if rc == 0]
    assert max(refused) < min(accepted), f"refusal is not monotone in ws_bytes: refused {sorted(refused)}, accepted {sorted(accepted)}"
    assert hi <= query and hi == smallest, (hi, smallest, query)
    for g, what in ((ws, "workspace"), (dw, "dW"), (db, "db")):
        g.check(what)
    # the call at exactly that size: exact results, intact guards, and nothing written behind the bytes it was given
    dw, db, ws = fresh()
    assert call(dw, db, ws, hi) == 0
    torch.cuda.synchronize()
    for g, what in ((ws, "workspace"), (dw, "dW"), (db, "db")):
        g.check(what)
    assert bool(torch.isnan(ws.body[0, hi // 4:]).all()), f"[{plan}] wrote behind the {hi} bytes of workspace it was given"
    assert_exact(dw.valid().view(c["cout"], c["cin"], k.taps), _dw_ref(k), "oit", plan)
    if entry == "wgrad_bias":
        assert_exact(db.valid().view(-1), k.ref["db"], "c", plan + " db")


# ------------------------------------------------------------------------------------------------
# comparator self-test (CPU): the method has no blind scale
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x16x16_512to512_k3", "2x8x16_64to133_k3", "2x33x17_64to150_k1"])
def test_one_wrong_weight_or_one_dropped_channel_is_reported(name):
    r = reference(name, False)
    c, x, w = r["c"], r["x"], r["w"]
    k = 3 if c["taps"] == 9 else 1
    y = _pad_c(r["y0"], c["Cout"])
    assert mismatch_report(y, y.clone(), "bhwc", "self") is None
    w1 = w.clone()
    w1[c["cout"] - 1, c["cin"] - 1, k - 1, k - 1] += 1                    # one weight off by one
    y1 = _pad_c(F.conv2d(x, w1, None, padding=k // 2), c["Cout"])
    rep = mismatch_report(y1, y, "bhwc", "one weight + 1")
    assert rep is not None and "elements differ" in rep and "[one weight + 1]" in rep and float((y1 - y).abs().max()) >= 1
    w2 = w.clone()
    w2[:, c["cin"] - 1, 0, 0] = 0                                        # the last input channel of one tap dropped
    y2 = _pad_c(F.conv2d(x, w2, None, padding=k // 2), c["Cout"])
    rep = mismatch_report(y2, y, "bhwc", "dropped k-step")
    assert rep is not None and float((y2 - y).abs().max()) >= 1
    assert "16x16 tile" in rep and "64-channel block" in rep and "expected" in rep and "got" in rep
    # a NaN (an output never written) is a difference, not a match
    y3 = y.clone()
    y3[0, 0, 0, 0] = float("nan")
    assert mismatch_report(y3, y, "bhwc", "nan") is not None


def test_every_plan_of_every_query_is_an_executed_test_id():
    ids = {p.id for p in _params()}
    for op in C.OPS:
        for n in C.all_plan_names(op):
            assert any(f"-{n}-" in i for i in ids), (op, n)
