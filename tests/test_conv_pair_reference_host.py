"""CPU checks of the pair-value recipe behind tests/test_gpu_conv_exact_pairs.py: its preconditions and densities on every row, the
float64 split helpers against torch's own roundings, the comparator against each deleted or added term, and the plan coverage."""
import pytest
import torch

from tests import _conv_cases as C
from tests import _conv_pair_cases as P
from tests.test_gpu_conv_exact import _pad_c, mismatch_report


def _row_schemes():
    out = []
    for c, es in P.pair_rows():
        out += [(C.name_of(c), s) for s in sorted({P.SCHEME_OF[e[0]] for e in es})]
    return out + [(name, "sub_" + P.SCHEME_OF[entry]) for entry, _, name in P.sub_rows()]


@pytest.mark.parametrize("name,scheme", _row_schemes())
def test_preconditions_and_density(name, scheme):
    r = P.pair_reference(name, scheme)          # (asserts the preconditions itself; again here so that a cached dict is checked too)
    P.check_preconditions(r)
    ok, what = P.density(r)
    assert ok, (name, scheme, what, r["thin"])
    sub = scheme in P.SUB_SCHEMES
    assert r["mass"] < (8 if sub else 2 ** 10)
    if sub:                                     # the lo half of x is an fp16 subnormal that survives the encoding, and only there
        live = r["xlo"][r["xlo"] != 0].abs()
        assert live.numel() > 0 and float(live.max()) < 2.0 ** -14 and torch.equal(P.split_fp16(r["x"])[1], r["xlo"])


def test_split_helpers_agree_with_torch_roundings():
    g = torch.Generator().manual_seed(3)
    a = (torch.randint(1, 3, (4096,), generator=g) * (2 * torch.randint(0, 2, (4096,), generator=g) - 1)).double()
    b = torch.randint(-3, 4, (4096,), generator=g).double()
    for e in (P.E, P.E_SUB):
        v = a + b * e
        v32 = v.float()
        assert torch.equal(v32.double(), v)
        hi, lo = P.split_fp16(v)
        assert torch.equal(hi, v32.half().double()) and torch.equal(lo, (v32 - v32.half().float()).half().double())
        assert torch.equal(hi, a) and torch.equal(lo, b * e)
        hi, lo = P.split_bf16(v)
        assert torch.equal(hi, v32.bfloat16().double()) and torch.equal(lo, (v32 - v32.bfloat16().float()).bfloat16().double())
        assert torch.equal(hi, a) and torch.equal(lo, b * e)
    w = a.sign() + b * P.E
    hi, lo = P.split_hl(w)
    w64 = (w * 64).float()
    assert torch.equal(hi, w64.half().double()) and torch.equal(lo, (w64 - w64.half().float()).half().double())
    assert torch.equal(hi, 64 * a.sign()) and torch.equal(lo, b * 2.0 ** -8)
    # and on values that are NOT of the recipe: ties, subnormals, both signs
    v = torch.cat([torch.randn(4096, generator=g).double() * s for s in (1.0, 1e-3, 1e-6, 300.0)] + [torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 0.0])])
    v = v.float().double()
    for split, cast in ((P.split_fp16, torch.Tensor.half), (P.split_bf16, torch.Tensor.bfloat16)):
        hi, lo = split(v)
        h32 = cast(v.float())
        assert torch.equal(hi, h32.double()) and torch.equal(lo, cast(v.float() - h32.float()).double())
    # the attention operand encoding: eight hi halves, then eight lo halves
    y = torch.arange(1.0, 17.0).view(1, 16) + 2.0 ** -13
    words = P.encode_h8(y).view(torch.int16).view(1, 2, 16)
    assert torch.equal(words[0, 0, :8].view(torch.float16).float(), torch.arange(1.0, 9.0))
    assert torch.equal(words[0, 0, 8:].view(torch.float16).float(), torch.full((8,), 2.0 ** -13))
    assert torch.equal(words[0, 1, :8].view(torch.float16).float(), torch.arange(9.0, 17.0))


@pytest.mark.parametrize("name", ["1x16x16_512to512_k3", "2x12x12_32to32_k3", "2x5x5_256to768_k1"])
def test_each_missing_or_extra_term_is_reported(name):
    r = P.pair_reference(name, "fwd")
    Cout = r["c"]["Cout"]
    y = _pad_c(P.expected(r, "three"), Cout)
    assert mismatch_report(y, y.clone(), "bhwc", "self") is None
    for what, t in (("x_lo w_hi removed", r["HH"] + r["HL"]), ("x_hi w_lo removed", r["HH"] + r["LH"]),
                    ("lo lo added and rounded", (r["HH"] + r["HL"] + r["LH"] + r["LL"]).float())):
        rep = mismatch_report(_pad_c(t, Cout), y, "bhwc", what)
        assert rep is not None and f"[{what}]" in rep and "elements differ" in rep, what
    # the exact-fp32 expectations differ from one another and from a 16-bit operand
    for key in ("p_int", "s_int"):
        assert mismatch_report(_pad_c(P.expected(r, key), Cout), _pad_c(r["HH"], Cout), "bhwc", key) is not None
    if r["c"]["taps"] == 9:
        g = P.pair_reference(name, "wgrad")
        dw = P.expected(g, "s_int").flatten(2)
        assert mismatch_report(dw.float(), dw, "oit", "self") is None
        rep = mismatch_report(g["HH"].flatten(2), dw, "oit", "lo columns removed")          # = what mu_conv_wgrad_h1 must return, and mu_conv_wgrad_h must not
        assert rep is not None and "[lo columns removed]" in rep
        d = P.pair_reference(name, "dgrad")
        assert mismatch_report(_pad_c(d["HH"] * 2, r["c"]["Cin"]), _pad_c(P.expected(d, "s_int"), r["c"]["Cin"]), "bhwc", "hi rows twice") is not None


def test_every_fp32_and_fp32x_plan_is_an_executed_test_id():
    from tests.test_gpu_conv_exact_pairs import _params, _sub_params
    ids = {p.id for p in _params()}
    names = set()
    for c in C.LAYERS:
        for entry, dn, op, pid in C.entries(c):
            if dn != "fp16":
                names.add((op, C.plan_name(op, pid)))
                assert c["heavy"] or f"{entry}-{dn}-{C.plan_name(op, pid)}-{C.name_of(c)}" in ids
    assert len(names) > 30
    for op, n in names:
        assert any(f"-{n}-" in i for i in ids), (op, n)
    # the entry points without a plan query, and the subnormal group's five rows
    for n in ("dma128_add", "dma64_add", "dma128_enc_h", "dma64_enc_h"):
        assert any(f"-{n}-" in i for i in ids), n
    sub = [p.id for p in _sub_params()]
    fams = {f for f, ns in P.SUB_FAMILIES.items() for i in sub if i.startswith("fwd-") and i.split("-")[2] in ns}
    assert fams == set(P.SUB_FAMILIES) and sum(i.startswith("wgrad_h-") for i in sub) == 1 and len(sub) == 5
