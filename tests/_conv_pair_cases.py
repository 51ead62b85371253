"""Operands with LIVE lo halves for the bit-exact convolution tests of the fp32 and fp32x paths (tests/test_gpu_conv_exact_pairs.py).

The recipe.  A "pair value" is v = a + b e with e = 2^-14, b in {-3..3} and a a nonzero integer (|a| <= 2 for x and dy, |a| = 1 for w);
thinning may set a whole value to exactly 0.  |b| e < 2^-12 = half an fp16 (and far below half a bf16) ulp just below 1, so
fp16(v) = bf16(v) = a and the lo half of v is exactly b e in all three operand encodings:
  * bf16 chunk pairs (mu_split_encode, both mu_prep_weight(MU_F32X, taps = 1) blocks);
  * fp16 chunk pairs (mu_split_encode_h4; the forward block of mu_prep_weight(MU_F32X, taps = 9) holds the pair of 2^6 w: 64 a, b 2^-8);
  * HL rows of 2^6 w (the data-gradient block of mu_prep_weight(MU_F32X, taps = 9)).
a != 0 wherever v != 0: with a = 0 the value would land entirely in the hi half and lo * lo would become a kept term.

With both operands pair values the three kept products hi hi + hi lo + lo hi are integers and multiples of e; the dropped lo lo is a multiple
of e^2.  Where sum |x| |w| < 2^10 for an output element, every partial sum of kept terms -- in ANY order and grouping -- is a multiple of
2^-14 below 2^10: exact in fp32 (24 bits).  The same holds under the 2^6 weight shift (multiples of 2^-8 below 2^16) and under the
power-of-two dy scale of the fp32x backward.  A correct kernel of any tiling returns
        conv(x, w) - conv(x_lo, w_lo)                      (fp32x, three terms)
        sum dy w,  sum dy x                                (fp32x 3x3 backward, dy one term: nothing is dropped)
        sum dy a                                           (mu_conv_wgrad_h1: the fp16 rounding of x and nothing else)
        conv(x, w) with one operand integer                (exact fp32: the full product)
computed here in float64 (exact there), BIT FOR BIT.  No tolerance is involved.

pair_reference(name, scheme) builds one row's operands and the four float64 component tensors HH, HL, LH, LL (first letter: half of the
streamed operand -- x or dy --, second: half of the partner) of the product the scheme forms; the expected tensors of every entry are sums
of them (expected()).  It asserts its preconditions on the CPU tensors alone and thins the operand that sets the sum length (x for the
forward, dy for the gradients, then both) by the 0.5, 0.75, ... ladder of the integer file until the mass condition holds; a case is never
dropped.  density() states how much a thinned case still holds; tests/test_conv_pair_reference_host.py asserts it on every row.

The subnormal group (schemes "sub_fwd", "sub_wgrad"): x = a + b 2^-20, whose fp16 lo half b 2^-20 is SUBNORMAL (w stays a 2^-14 pair value:
its shifted lo half is normal).  The kept terms are then multiples of 2^-14 (2^-20 2^6), so the mass bound is sum |x| |w| < 8."""
import functools

import torch
import torch.nn.functional as F

from tests import _conv_cases as C

E = 2.0 ** -14
E_SUB = 2.0 ** -20
MASS = 2.0 ** 10 - 8            # sum |.||.| plus a bias / shift (<= 3) and an addend / residual (< 3) stays below 2^10
MASS_SUB = 8.0
SCHEMES = ("fwd", "dgrad", "wgrad")
SUB_SCHEMES = ("sub_fwd", "sub_wgrad")
WSHIFT = 6                      # MU_XH_WSHIFT (maskunet_amd/csrc/common.h)


# ------------------------------------------------------------------------------------------------
# the three encodings, restated in float64
# ------------------------------------------------------------------------------------------------
def _round_to(v, p, emin):
    """Round-to-nearest-even of float64 v to p significant bits with the smallest normal exponent emin (gradual underflow below)."""
    v = v.double()
    _, ex = torch.frexp(v)                                  # v = m 2^ex, 0.5 <= |m| < 1
    e = torch.clamp(ex - 1, min=emin)
    q = torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - (p - 1)).double())
    return torch.where(v == 0, v, torch.round(v / q) * q)   # torch.round: half to even


def split_bf16(v):
    """(hi, lo) of the bf16 chunk pair: hi = bf16(v), lo = bf16(v - hi)."""
    hi = _round_to(v, 8, -126)
    return hi, _round_to(v.double() - hi, 8, -126)


def split_fp16(v):
    """(hi, lo) of the fp16 chunk pair: hi = fp16(v), lo = fp16(v - hi); lo may be subnormal (multiples of 2^-24)."""
    hi = _round_to(v, 11, -14)
    return hi, _round_to(v.double() - hi, 11, -14)


def split_hl(w):
    """(hi, lo) halves of an HL row / of the 3x3 forward block: the fp16 pair of 2^6 w."""
    return split_fp16(w.double() * 2.0 ** WSHIFT)


def encode_h8(y):
    """mu_split_encode_h of fp32 rows [M, C] (C % 8 == 0): int32 words [M, C], every group of eight floats -> [8 fp16 hi | 8 fp16 lo]."""
    y = y.float() + 0.0
    M, Cc = y.shape
    hi = y.half()
    lo = (y - hi.float()).half()
    g = torch.cat([hi.view(M, Cc // 8, 8), lo.view(M, Cc // 8, 8)], dim=2).contiguous()          # 16 halves per group
    return g.view(torch.int16).view(M, Cc * 2).view(torch.int32).view(M, Cc)


# ------------------------------------------------------------------------------------------------
# the value recipe
# ------------------------------------------------------------------------------------------------
def _layer(name):
    return next(c for c in C.LAYERS if C.name_of(c) == name)


def make_pairs(c, sub=False):
    """Integer parts, lo counts b and thinning uniforms of the row c (float64; seeded per row)."""
    g = torch.Generator().manual_seed(77 + 1000 * c["B"] + 31 * c["H"] + 7 * c["W"] + c["Cin"] + 3 * c["Cout"] + c["taps"] + (500000 if sub else 0))
    B, H, W, cin, cout, k = c["B"], c["H"], c["W"], c["cin"], c["cout"], 3 if c["taps"] == 9 else 1

    def ints(shape, amax):
        a = torch.randint(1, amax + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
        return a.double(), torch.randint(-3, 4, shape, generator=g).double()

    xa, xb = ints((B, cin, H, W), 2)
    wa, wb = ints((cout, cin, k, k), 1)
    dya, dyb = ints((B, cout, H, W), 2)
    bias = torch.randint(-3, 4, (cout,), generator=g).double()
    ux, udy = torch.rand(xa.shape, generator=g), torch.rand(dya.shape, generator=g)
    return dict(xa=xa, xb=xb, wa=wa, wb=wb, dya=dya, dyb=dyb, b=bias, ux=ux, udy=udy)


def _ladder(k):
    """Thinned fraction after k steps of the integer file's ladder: 0, 0.5, 0.75, ..."""
    return 0.0 if k == 0 else 1.0 - 0.5 ** k


def _product(scheme, k):
    """(f, mass_f): the product the scheme forms on float64 (streamed operand, partner), and the same on float32 magnitudes."""
    if scheme.endswith("fwd"):
        return (lambda s, p: F.conv2d(s, p, None, padding=k // 2)), (lambda s, p: F.conv2d(s, p, None, padding=k // 2))
    if scheme == "dgrad":
        return (lambda s, p: F.conv_transpose2d(s, p, None, padding=k // 2)), (lambda s, p: F.conv_transpose2d(s, p, None, padding=k // 2))
    # wgrad: streamed operand dy [B, cout, H, W], partner x [B, cin, H, W] -> [cout, cin, k, k]
    # (one matrix product per tap: the same sums as conv2d(x^T, dy^T), without an image-sized filter)
    def wg(s, p):
        H, W = s.shape[2:]
        s2, pp = s.transpose(0, 1).flatten(1), F.pad(p, (k // 2,) * 4)
        taps = [s2 @ pp[:, :, u:u + H, v:v + W].transpose(0, 1).flatten(1).t() for u in range(k) for v in range(k)]
        return torch.stack(taps, dim=2).view(s.shape[1], p.shape[1], k, k)
    return wg, wg


def _sub_keep(v, kind):
    """The subnormal group's thinning, by construction instead of by the ladder (a random thinning down to sum |x| |w| < 8 at the DENSEST
    output leaves a fraction of a product at the others).  Forward: x lives on the pixel lattice (h % 3 == 1, w % 3 == 1) -- every 3 x 3
    window holds exactly one such pixel -- in three seeded channels per pixel: three products of at most 2.00001 * 1.0002 at every
    output element.  Weight gradient: every dy channel lives at ONE seeded pixel of the batch and x stays dense: each of the
    9 * cin * cout sums is one product of at most 2 * 2.00001."""
    ux, udy = v["ux"], v["udy"]
    if kind == "fwd":
        H, W = ux.shape[2:]
        lattice = (torch.arange(H).view(H, 1) % 3 == 1) & (torch.arange(W).view(1, W) % 3 == 1)
        rank = ux.argsort(dim=1).argsort(dim=1)
        return (rank < 3) & lattice, torch.ones_like(udy, dtype=torch.bool)
    flat = udy.transpose(0, 1).flatten(1)                          # [cout, B * H * W]
    one = torch.zeros_like(flat, dtype=torch.bool)
    one[torch.arange(flat.shape[0]), flat.argmin(dim=1)] = True
    return torch.ones_like(ux, dtype=torch.bool), one.view(udy.shape[1], udy.shape[0], *udy.shape[2:]).transpose(0, 1)


@functools.lru_cache(maxsize=2)
def pair_reference(name, scheme):
    """Operands and float64 component tensors of the row `name` for one product.

    scheme "fwd" (x streamed against w), "dgrad" (dy against w), "wgrad" (dy against x), "sub_fwd" / "sub_wgrad" (the subnormal group).
    Returns a dict: c; s / sa / slo and p / pa / plo = the streamed operand and its partner with their integer and lo parts (thinned);
    x, w, dy, b by name; HH, HL, LH, LL; thin = (thinned fraction of the streamed operand, of the partner); live, full = mean number of
    nonzero products per output element after / before thinning."""
    assert scheme in SCHEMES + SUB_SCHEMES, scheme
    c = _layer(name)
    sub = scheme in SUB_SCHEMES
    kind = scheme[4:] if sub else scheme
    k = 3 if c["taps"] == 9 else 1
    v = make_pairs(c, sub)
    ex = E_SUB if sub else E
    f, fm = _product(kind, k)
    limit = MASS_SUB if sub else MASS
    step = 0
    while True:
        if sub:
            keep_x, keep_dy = _sub_keep(v, kind)
            t_s, t_p = 1.0 - float((keep_x if kind == "fwd" else keep_dy).double().mean()), 0.0
        else:
            # the streamed operand first; once the ladder has run nine steps (1 - 2^-9), the partner activations of the weight gradient as well
            t_s, t_p = _ladder(min(step, 9)), _ladder(max(step - 9, 0))
            keep_x = v["ux"] >= (t_s if kind == "fwd" else t_p if kind == "wgrad" else 0.0)
            keep_dy = v["udy"] >= (t_s if kind != "fwd" else 0.0)
        xa, xlo = v["xa"] * keep_x, v["xb"] * ex * keep_x
        dya, dylo = v["dya"] * keep_dy, v["dyb"] * E * keep_dy
        wa, wlo = v["wa"], v["wb"] * E
        sa, slo = (xa, xlo) if kind == "fwd" else (dya, dylo)
        pa, plo = (xa, xlo) if kind == "wgrad" else (wa, wlo)
        mass = fm((sa.abs() + slo.abs()).float(), (pa.abs() + plo.abs()).float())
        if float(mass.max()) * (1 + 1e-4) < limit:
            break
        step += 1
        assert step <= 13 and not sub, (name, scheme)          # the case is never dropped
    live = float(fm((sa != 0).float(), (pa != 0).float()).mean())
    full = float(fm(torch.ones_like(sa, dtype=torch.float32), torch.ones_like(pa, dtype=torch.float32)).mean())
    r = dict(c=c, scheme=scheme, sa=sa, slo=slo, s=sa + slo, pa=pa, plo=plo, p=pa + plo, b=v["b"], thin=(t_s, t_p), live=live, full=full,
             x=xa + xlo, xa=xa, xlo=xlo, w=wa + wlo, wa=wa, wlo=wlo, dy=dya + dylo, dya=dya, dylo=dylo, mass=float(mass.max()),
             HH=f(sa, pa), HL=f(sa, plo), LH=f(slo, pa), LL=f(slo, plo))
    check_preconditions(r)
    return r


def exact32(t):
    return bool(torch.equal(t.float().double(), t.double()))


def check_preconditions(r):
    """On the CPU tensors alone: every operand is hi + lo of its encoding with hi = a; the mass bound; every expected tensor is an fp32 value."""
    sub = r["scheme"] in SUB_SCHEMES
    for nm, a_, lo_ in (("x", r["xa"], r["xlo"]), ("dy", r["dya"], r["dylo"]), ("w", r["wa"], r["wlo"])):
        val = a_ + lo_
        assert exact32(val), nm
        assert bool(((a_ != 0) | (val == 0)).all()), f"{nm}: a value with a = 0 would sit entirely in the hi half"
        for split in ((split_hl,) if nm == "w" else ()) + (split_bf16, split_fp16):
            if sub and nm == "x" and split is split_bf16:
                continue                                   # (b 2^-20 is a bf16 value too, but the subnormal group runs 3x3 layers only)
            hi, lo = split(val)
            sc = 2.0 ** WSHIFT if split is split_hl else 1.0
            assert torch.equal(hi, a_ * sc) and torch.equal(lo, lo_ * sc), f"{nm}: {split.__name__} is not (a, b e)"
    assert r["mass"] < (MASS_SUB if sub else MASS)
    for key in ("three", "s_int", "p_int", "int"):
        assert exact32(expected(r, key)), key


# expected tensors as sums of the components (first letter: streamed operand's half, second: the partner's)
EXPECTED = {
    "three": ("HH", "HL", "LH"),      # fp32x, both operands pairs: everything but lo lo
    "s_int": ("HH", "HL"),            # the streamed operand an integer (one fp16 term dy; exact fp32 against pair partners)
    "p_int": ("HH", "LH"),            # the partner an integer (exact fp32: pair activations against integer weights)
    "int": ("HH",),                   # both integers (mu_conv_wgrad_h1: dy against the fp16 rounding of x)
    "full": ("HH", "HL", "LH", "LL"),
}


def expected(r, key):
    return sum(r[t] for t in EXPECTED[key]) + 0.0


def density(r):
    """(ok, what): a thinned case still exercises every piece of the sum.  Every 32-channel block of each pair operand (every (tap, block)
    of the weights) holds elements with a live lo half, and the mean number of nonzero products per output element is at least 64 -- or,
    where the unthinned row has fewer than 64 (its full K, less the taps that fall into the zero border), all of them.  The subnormal
    group's mass bound (8) allows about five products per output: there only the block condition is asked."""
    for nm in ("x", "dy", "w"):
        lo = r[nm + "lo"]
        if nm == "w":
            blocks = lo.split(32, dim=1)
            if not all(bool((blk != 0).flatten(2).any(0).any(0).all()) for blk in blocks):          # every tap of every 32-input-channel block
                return False, "a (tap, 32-input-channel block) of w holds no live lo half"
        elif not all(bool((blk != 0).any()) for blk in lo.split(32, dim=1)):
            return False, f"a 32-channel block of {nm} holds no live lo half"
    if r["scheme"] in SUB_SCHEMES:
        return True, ""
    need = min(64.0, r["full"])
    return (r["live"] >= need - 1e-9, f"mean live products per output {r['live']:.1f} < {need:.1f}")


# ------------------------------------------------------------------------------------------------
# which (entry, dtype, kernel, row) the GPU file runs
# ------------------------------------------------------------------------------------------------
SCHEME_OF = {"fwd": "fwd", "fwd_stats": "fwd", "fused": "fwd", "fwd_add": "fwd", "fwd_enc_h": "fwd", "dgrad": "dgrad", "dgrad_h": "dgrad",
             "wgrad": "wgrad", "wgrad_h": "wgrad", "wgrad_h1": "wgrad"}


def _cost(c):
    return c["B"] * c["H"] * c["W"] * c["Cin"] * c["Cout"] * c["taps"]


def pair_entries(c):
    """[(entry, dtype name, op, kernel name)] of the fp32 / fp32x columns for the row c: those of _conv_cases.entries, the exact-fp32 data
    gradient (mu_conv_fwd on mode-1 weights) and the two 1x1 entry points that have no plan query (named after their tile width)."""
    from maskunet_amd import _lib
    lib = _lib.load()
    out = [(e, dn, op, C.plan_name(op, pid)) for e, dn, op, pid in C.entries(c) if dn != "fp16"]
    if c["heavy"]:
        return out
    out.append(("dgrad", "fp32", "fwd", C.plan_name("fwd", lib.mu_conv_fwd_plan(c["B"], c["H"], c["W"], c["Cout"], c["Cin"], c["taps"], C.DTYPES["fp32"], 0))))
    if c["taps"] == 1:
        tile = 128 if c["Cout"] % 128 == 0 else 64
        if lib.mu_conv1x1_add_supported(c["Cin"], c["Cout"], C.DTYPES["fp32x"]):
            out.append(("fwd_add", "fp32x", None, f"dma{tile}_add"))
        if c["Cin"] % 32 == 0 and c["Cout"] % 64 == 0:
            out.append(("fwd_enc_h", "fp32x", None, f"dma{tile}_enc_h"))
    return out


def pair_rows():
    """The non-heavy rows of LAYERS; a plan name of the fp32 / fp32x columns that only heavy rows reach (the fp32x ping-pong kernel needs
    192 tiles of 16 x 16) runs on the cheapest of them, forward entries only as in the integer file."""
    rows = [(c, pair_entries(c)) for c in C.LAYERS if not c["heavy"]]
    have = {(op, n) for _, es in rows for _, _, op, n in es}
    for c in sorted((c for c in C.LAYERS if c["heavy"]), key=_cost):
        es = [e for e in pair_entries(c) if (e[2], e[3]) not in have]
        if es:
            have |= {(e[2], e[3]) for e in es}
            rows.append((c, es))
    return rows


SUB_FAMILIES = {"generic": ("gen32", "gen64", "gen128"), "lds_dma": ("dma64", "dma128"), "halo_tile": ("nt3_64", "nt3_64_ring", "nt3_128"),
                "ping_pong": ("nt4x",)}


def sub_rows():
    """[(entry, kernel name, row name)] of the subnormal group: the cheapest row of each 3x3 fp32x forward kernel family, one mu_conv_wgrad_h row."""
    out = []
    cand = sorted((c for c in C.LAYERS if c["taps"] == 9 and c["cin"] > 3), key=_cost)
    for fam, names in SUB_FAMILIES.items():
        for c in cand:
            kn = next((n for e, dn, op, n in pair_entries(c) if e == "fwd" and dn == "fp32x"), None)
            if kn in names:
                out.append(("fwd", kn, C.name_of(c)))
                break
        else:
            raise AssertionError(fam)
    c = next(c for c in cand if not c["heavy"] and c["Cin"] >= 64)
    out.append(("wgrad_h", next(n for e, dn, op, n in pair_entries(c) if e == "wgrad_h"), C.name_of(c)))
    return out
