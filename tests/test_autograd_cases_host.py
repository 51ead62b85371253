"""Host checks of tests/_autograd_cases.py (no GPU): every fp64 reference, and the oracle with a per-layer `training` callable, against
the torch.nn modules in fp64 with the same train() / eval() flags and requires_grad pattern (gate: 1e-12 relative); the coverage the
tables must have; the ReLU and max-pool margins of the inputs."""
import pytest
import torch
import torch.nn as nn

from oracle import maskunet_oracle as O
from tests import _autograd_cases as AC

GATE = 1e-12


def _close(got, ref, what, scale=None):
    """Relative to the reference tensor's own largest entry, or to `scale` where given."""
    if ref is None or got is None:
        assert got is None and ref is None, what
        return
    assert got.shape == ref.shape, what
    err = float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()) if scale is None else scale, 1e-300)
    assert err <= GATE, (what, err)


# ---- torch.nn restatement of the module surface (state_dict keys of maskunet_amd.modules) -------------------------------------------
class TConvBlock(nn.Module):
    def __init__(self, cin, cout, mid=None, residual=False):
        super().__init__()
        mid = mid or cout
        self.residual = residual
        self.conv_block = nn.Sequential(nn.Conv2d(cin, mid, 3, padding=1, bias=False), nn.BatchNorm2d(mid), nn.GELU(),
                                        nn.Conv2d(mid, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        return nn.functional.gelu(x + self.conv_block(x)) if self.residual else self.conv_block(x)


class TDown(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool2d(2), TConvBlock(cin, cin, residual=True), TConvBlock(cin, cout), nn.BatchNorm2d(cout))
        self.emb_layer = nn.Sequential(nn.SiLU(), nn.Linear(256, cout))

    def forward(self, x):
        return self.maxpool_conv(x)


class TUp(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.upsample = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = nn.Sequential(TConvBlock(cin, cin, residual=True), TConvBlock(cin, cout, cin // 2), nn.BatchNorm2d(cout))
        self.emb_layer = nn.Sequential(nn.SiLU(), nn.Linear(256, cout))

    def forward(self, x, skip):
        return self.conv(torch.cat([skip, self.upsample(x)], dim=1))


class TChain(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return x


def torch_form(form):
    f = AC.FORMS[form]
    if form == "down":
        return TDown(64, 128)
    if form == "up":
        return TUp(128, 64)
    blocks = [TConvBlock(ci, co, mid, res) for (_p, ci, co, mid, res) in f["blocks"]]
    return blocks[0] if len(blocks) == 1 else TChain(blocks)


# ---- references ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.CONV_CASES, ids=lambda c: c["id"])
def test_conv_reference_is_nn_conv2d(case):
    L = AC.CONV_LAYERS[case["layer"]]
    x, w, b, gy = AC.conv_inputs(case["layer"], "fp16")
    ref = AC.conv_ref(x, w, b, gy, case["needs"])
    m = nn.Conv2d(L["cin"], L["cout"], L["k"], padding=L["k"] // 2).double()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    m.weight.requires_grad_(case["needs"][1])
    m.bias.requires_grad_(case["needs"][2])
    xt = x.double().requires_grad_(case["needs"][0])
    y = m(xt)
    y.backward(gy.double())
    for k, t in (("y", y.detach()), ("dx", xt.grad), ("dw", m.weight.grad), ("db", m.bias.grad)):
        _close(ref[k], t, (case["id"], k))
        assert (ref[k] is not None) == (k == "y" or case["needs"][("dx", "dw", "db").index(k)])


def _nn_bn(st, case_like):
    C = st["weight"].numel()
    m = nn.BatchNorm2d(C, momentum=case_like["momentum"], track_running_stats="running_mean" in st)
    m.load_state_dict(st)
    return m.double().train(case_like["training"])


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("case", AC.BN_CASES, ids=lambda c: c["id"])
def test_bn_act_reference_is_nn_batchnorm(case, mode):
    x, res, gy, st = AC.bn_inputs(case, mode)
    ref = AC.bn_act_ref(x, res, gy, st, case)
    m = _nn_bn(st, case)
    for p in m.parameters():
        p.requires_grad_(case["affine"])
    xt = x.double().requires_grad_(case["x_grad"])
    rt = None if res is None else res.double().requires_grad_(case["res"] == "grad")
    pre = m(xt) if rt is None else m(xt) + rt
    y = {AC.ACT_NONE: nn.Identity(), AC.ACT_GELU: nn.GELU(), AC.ACT_RELU: nn.ReLU()}[case["act"]](pre)
    if y.requires_grad:
        y.backward(gy.double())
    got = dict(y=y.detach(), dx=xt.grad, dres=None if rt is None else rt.grad, dgamma=m.weight.grad, dbeta=m.bias.grad,
               running_mean=m.running_mean, running_var=m.running_var)
    for k, t in got.items():
        _close(ref[k], t, (case["id"], k))
    if case["track"]:
        assert int(ref["num_batches_tracked"]) == int(m.num_batches_tracked) == (1 if case["training"] else 0)
    # the margin the table states holds on these very inputs: no element is left out of any comparison
    if case["act"] == AC.ACT_RELU:
        assert case["relu_margin"] == AC.RELU_MARGIN and float(ref["pre"].abs().min()) >= AC.RELU_MARGIN, float(ref["pre"].abs().min())


@pytest.mark.parametrize("case", AC.PAIR_CASES, ids=lambda c: c["id"])
def test_bn_pair_reference_is_two_nn_batchnorms(case):
    x, gy, s1, s2 = AC.pair_inputs(case, "fp16")
    ref = AC.bn_pair_ref(x, gy, s1, s2, case)
    ms = [_nn_bn(st, dict(momentum=0.1, training=tr)) for st, tr in zip((s1, s2), case["training"])]
    for i, m in enumerate(ms, 1):
        m.weight.requires_grad_(f"g{i}" not in case["frozen"])
        m.bias.requires_grad_(f"b{i}" not in case["frozen"])
    xt = x.double().requires_grad_(case["x_grad"])
    y = ms[1](ms[0](xt))
    y.backward(gy.double())
    _close(ref["y"], y.detach(), "y")
    _close(ref["dx"], xt.grad, "dx")
    for i, m in enumerate(ms, 1):
        for k, t in ((f"g{i}", m.weight.grad), (f"b{i}", m.bias.grad), (f"running_mean{i}", m.running_mean), (f"running_var{i}", m.running_var)):
            _close(ref[k], t, (case["id"], k))
        assert int(ref[f"num_batches_tracked{i}"]) == int(m.num_batches_tracked)
        assert (ref[f"g{i}"] is None) == (f"g{i}" in case["frozen"])


@pytest.mark.parametrize("case", AC.BLOCK_CASES, ids=lambda c: c["id"])
def test_oracle_with_per_layer_training_is_the_nn_modules(case):
    """The extended oracle (training = callable(prefix)) under a freeze pattern and per-layer eval() flags == the torch.nn modules."""
    params, ins, gout = AC.block_inputs(case["form"], "fp16")
    ref = AC.block_ref(case, params, ins, gout)
    m = torch_form(case["form"])
    m.load_state_dict({k[2:]: v for k, v in params.items()})
    m.double().train()
    mods = dict(m.named_modules())
    for bn in case["bn_eval"]:
        mods[bn[2:]].eval()
    for k, p in m.named_parameters():
        p.requires_grad_("m." + k not in case["frozen"])
    xs = [t.double().requires_grad_(g) for t, g in zip(ins, case["in_grads"])]
    y = m(*xs)
    if y.requires_grad:
        y.backward(gout.double())
    _close(ref["out"], y.detach(), "out")
    for i, t in enumerate(xs):
        _close(ref["gin"][i], t.grad, f"gin{i}")
    named = dict(m.named_parameters())
    # gamma / beta of a BatchNorm whose only reader is a training-mode BatchNorm: the gradient is zero up to O(eps)
    # terms, i.e. what is left when sums of the size of the case's other gradients cancel -- two fp64 evaluations agree on it to 1e-16 of
    # THOSE sums, not of the remainder (measured: 2e-11 of the remainder).  Held to the gate relative to the case's largest parameter
    # gradient; every other tensor relative to its own largest entry.
    f = AC.FORMS[case["form"]]
    last_bn = f["blocks"][-1][0] + ".conv_block.4"
    cancels = f["tail"] is not None and f["tail"] not in case["bn_eval"]          # (in either mode of the layer in front: a per-channel affine)
    gmax = max([float(g.abs().max()) for g in ref["gparam"].values() if g is not None] or [1.0])
    for k, g in ref["gparam"].items():
        _close(g, named[k[2:]].grad, k, scale=gmax if cancels and k.startswith(last_bn + ".") else None)
        assert (g is None) == (k in case["frozen"]), k
    sd = m.state_dict()
    for k, v in ref["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(sd[k[2:]]), k
        else:
            _close(v, sd[k[2:]], k)
    if case["form"] == "down":
        assert case["pool_margin"] == AC.POOL_MARGIN
        for mode in AC.MODES:
            assert AC.pool_gap(AC.block_inputs("down", mode)[1][0]) >= AC.POOL_MARGIN


def test_oracle_training_flag_bool_and_callable_agree_on_the_whole_model():
    """A plain bool keeps the oracle's behaviour exactly; a callable that answers alike gives the same bits; dropout under a callable is
    off unless masks are given and training("dropout") is true."""
    hw, B = 32, 1
    p = O.make_params(O.unet_state_shapes(3, 5, True, hw=hw), 3)
    keeps = O.make_keeps(4, B, hw)
    x, _ = O.make_inputs(5, B, 5, hw)
    g = torch.Generator().manual_seed(6)
    dm = [(torch.rand(B, 128, hw // 4, hw // 4, generator=g) > 0.3).float(), (torch.rand(B, 64, hw // 2, hw // 2, generator=g) > 0.3).float()]
    with torch.no_grad():
        for flag in (True, False):
            for masks in (None, dm):
                s1, s2 = {}, {}
                a = O.unet_forward(p, x, keeps, training=flag, dropout_masks=masks, new_stats=s1, three_head=True)
                b = O.unet_forward(p, x, keeps, training=lambda prefix, f=flag: f, dropout_masks=masks, new_stats=s2, three_head=True)
                assert all(torch.equal(u, v) for u, v in zip(a, b)) and s1.keys() == s2.keys() and all(torch.equal(s1[k], s2[k]) for k in s1)
        # BatchNorm layers in eval(), dropout on: == training=False everywhere but the dropout
        on = O.unet_forward(p, x, keeps, training=lambda prefix: prefix == "dropout", dropout_masks=dm, three_head=True)
        off = O.unet_forward(p, x, keeps, training=lambda prefix: False, dropout_masks=dm, three_head=True)
        ev = O.unet_forward(p, x, keeps, training=False, dropout_masks=dm, three_head=True)
        assert all(torch.equal(u, v) for u, v in zip(off, ev)) and not torch.equal(on[0], ev[0])
        # one layer alone in eval(): its running statistics are not advanced, every other layer's are
        ns = {}
        O.unet_forward(p, x, keeps, training=lambda prefix: prefix != "bottom2.conv_block.1", new_stats=ns, three_head=True)
        assert "bottom2.conv_block.1.running_mean" not in ns and "bottom2.conv_block.4.running_mean" in ns


def test_unet_reference_with_a_kept_trunk_is_the_plain_oracle_run():
    """UnetRef (trunk once, heads and backward per set of final-ReLU decisions) == one oracle.unet_forward + backward with the same
    frozen leaves and per-layer flags, bit for bit when the decisions are the oracle's own; a second finish() gives the same bits."""
    recipe = "three-head-heads-only"
    r = AC.UnetRef(recipe)
    params, keeps, x, labels = AC.unet_inputs(True)
    assert r.frozen == {k for k, v in params.items() if v.dtype.is_floating_point and "running" not in k
                        and not k.startswith(("boundary_head.", "embedding_head."))}
    p = AC.oracle_leaves(params, r.frozen)
    ns = {}
    outs = O.unet_forward(p, x.double(), keeps, training=r.training, new_stats=ns, three_head=True)
    AC.unet_loss(outs, labels, True, O.pixel_cross_entropy).backward()
    for _ in range(2):
        f = r.finish(outs[0].detach() > 0)
        assert f["forced"]["n"] == 0 and all(torch.equal(u, v.detach()) for u, v in zip(f["outs"], outs))
        assert f["stats"].keys() == ns.keys() and all(torch.equal(f["stats"][k], ns[k]) for k in ns)
        for k, g in f["grads"].items():
            assert (g is None) == (k in r.frozen) == (p[k].grad is None), k
            assert g is None or torch.equal(g, p[k].grad), k
    # the recipes: what each freezes and which BatchNorm layers it puts into eval()
    p1, bns = AC.unet_inputs(False)[0], AC.bn_prefixes(AC.unet_inputs(False)[0])
    fr = {k: AC.unet_frozen(k, p1) for k in ("encoder-frozen-bn-eval", "encoder-frozen-bn-train", "only-final-layer", "bn-frozen-and-eval")}
    assert fr["encoder-frozen-bn-eval"] == fr["encoder-frozen-bn-train"] == {k for k in fr["only-final-layer"] if k.startswith(AC.ENCODER)}
    assert all(k.startswith(AC.ENCODER) for k in fr["encoder-frozen-bn-eval"]) and "bottom1.conv_block.0.weight" not in fr["encoder-frozen-bn-eval"]
    assert fr["bn-frozen-and-eval"] == {b + s for b in bns for s in (".weight", ".bias")} and len(bns) == 39
    R = AC.UNET_RECIPES
    assert R["encoder-frozen-bn-eval"]["bn_eval"]("downsample2.maxpool_conv.3") and not R["encoder-frozen-bn-eval"]["bn_eval"]("bottom1.conv_block.1")
    assert [k for k, v in R.items() if v["twin"]] == ["encoder-frozen-bn-train", "only-final-layer", "three-head-heads-only"]


# ---- coverage: a condition on the tables, not a measurement --------------------------------------------------------------------------
def test_tables_cover_what_the_suite_promises():
    for kind in ("stem3x3", "mc3x3", "1x1"):
        seen = {c["needs"] for c in AC.CONV_CASES if AC.CONV_LAYERS[c["layer"]]["kind"] == kind}
        assert seen == set(AC.PATTERNS) and len(AC.PATTERNS) == 7, kind
    head = {c["needs"] for c in AC.CONV_CASES if c["layer"] == "head3x3"}
    assert (True, True, False) in head and (True, False, True) in head
    for length in (1, 2, 3):
        cases = [c for c in AC.BLOCK_CASES if c["run_length"] == length]
        want = {(i, e) for i in range(length) for e in (1, 2)}
        assert want <= {c["break_pos"] for c in cases}, (length, want - {c["break_pos"] for c in cases})
    forms = {c["form"] for c in AC.BLOCK_CASES}
    assert forms == set(AC.FORMS)
    ids = set()
    for table, cases in AC.ALL_TABLES.items():
        for c in cases:
            assert c["id"] not in ids or table != "blocks"
            ids.add(c["id"])
            missing = set(AC.MODES) - set(c["modes"])
            assert missing == set(c.get("left_out", {})), (table, c["id"])
            for mode in missing:
                assert c["block"] == "c288-wide" and mode == "fp32x" and c["left_out"][mode] == AC.WIDE_FP32X_REASON
            for mode, tensors in c["exceptions"].items():
                assert mode in c["modes"] and tensors
                for name, cause in tensors.items():
                    assert isinstance(cause, str) and "ops.py" in cause and len(cause) > 40, (table, c["id"], name)
    # group B: both modes x both affine states x the three activations; every residual form; no buffers; the refused setting
    bn = AC.BN_CASES
    for act in (AC.ACT_NONE, AC.ACT_GELU, AC.ACT_RELU):
        assert {(c["training"], c["affine"]) for c in bn if c["act"] == act} == {(t, a) for t in (True, False) for a in (True, False)}
        assert {c["res"] for c in bn if c["act"] == act} == {None, "grad", "nograd"}
    assert any(not c["track"] for c in bn) and any(not c["x_grad"] for c in bn)
    assert AC.BN_CUMULATIVE_CASE["momentum"] is None and AC.BN_CUMULATIVE_CASE["training"] and AC.BN_CUMULATIVE_CASE["track"]
    # group C: folded, either layer alone in eval(), the first affine frozen while folded
    pc = {c["id"]: c for c in AC.PAIR_CASES}
    assert {c["training"] for c in AC.PAIR_CASES} == {(True, True), (True, False), (False, True), (False, False)}
    assert pc["fold-first-affine-frozen"]["frozen"] == ("g1", "b1") and pc["fold-first-affine-frozen"]["training"] == (True, True)
    # group D: the residual first block with (down, up) and without (res1) a taker, every BatchNorm in eval(), UpSample's two inputs
    bid = {c["id"] for c in AC.BLOCK_CASES}
    assert {"res1-all-trainable", "down-all-bn-eval", "up-skip-nograd", "up-x-nograd", "down-only-tail-bn", "chain3-only-last-conv"} <= bid
    # group E
    assert {(c["block"], tuple(sorted(c["frozen"])), c["x_grad"]) for c in AC.ATTN_CASES} == {
        (b, tuple(sorted(p["frozen"])), p["x_grad"]) for b in AC.ATTN_BLOCKS for p in AC.ATTN_PATTERNS.values()}


def test_break_position_restates_the_rule_of_conv_blocks():
    names = AC.run_params("down")
    assert AC.break_position("down", (), (True,)) is None
    assert AC.break_position("down", (), (False,)) == (0, 2)
    assert AC.break_position("down", tuple(names[:3]), (False,)) == (0, 1)
    assert AC.break_position("down", tuple(names[:6]), (False,)) == (1, 2)
    assert AC.break_position("down", tuple(names[:12]), (False,)) == (1, 1)          # only the tail BatchNorm trainable


def test_activation_codes_match_the_library():
    from maskunet_amd import _lib
    assert (AC.ACT_NONE, AC.ACT_GELU, AC.ACT_RELU) == (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_RELU)
