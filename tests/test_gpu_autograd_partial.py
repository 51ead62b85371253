"""Partial training through maskunet_amd.ops / modules: frozen parameters, inputs without grad, single BatchNorm layers in eval().

Every test builds one module (or one ops call) twice from the same seeded state (tests/_autograd_cases.py):
run A with everything trainable and the inputs requiring grad, run B with one freeze pattern.
  1. Bit identity: freezing must not change any other result -- every tensor both runs compute (output, gradients of the parameters
     still trainable, input gradients still wanted, running statistics) is torch.equal.  The kernels are deterministic and the
     operands reaching the remaining kernels are the same, so there is no tolerance.  Exceptions are declared in the case tables with
     their cause and held to instrument 2.
  2. fp64 parity of run B with the plain-torch / oracle reference under the same freeze pattern and per-layer training flags, at the
     project's gates: _gpu_checks.TOL for outputs, input gradients and running statistics; check_golden_module's floor rule
     (PARAM_GRAD_FLOOR) for parameter gradients.
Both runs: p.grad is None for frozen parameters, x.grad is None for inputs without grad, the buffers of a BatchNorm in eval() are
bit-unchanged, those of one in train() advanced (num_batches_tracked by exactly 1).

Mutations of ops.py this file was run against (each must fail it): an exit of _ConvBlocks.backward inverted -- 159 of the
test_conv_blocks_partial_training cases (wrong-shaped or missing gradients, input gradients off by 0.85 relative); `needs[1]` replaced by
True in `keep16` -- no value changes (the data gradient reads only the kept tensor's shape), caught by
test_fp32x_conv_keeps_the_operand_its_backward_reads; `and ctx.needs_input_grad[1]` dropped in _UpCat.forward -- no value changes inside
the UNet (link, pool and concat see one tensor), caught by test_upcat_leaves_no_fill_for_a_skip_without_grad; the momentum=None refusal
removed -- test_bn_cumulative_average_is_refused_before_any_launch.
"""
import contextlib

import pytest
import torch
import torch.nn as nn

from tests import _autograd_cases as AC
from tests._gpu_checks import PARAM_GRAD_FLOOR, TOL, _err, _rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


@contextlib.contextmanager
def precision(mode):
    import maskunet_amd
    maskunet_amd.set_float32_matmul_precision("high" if mode == "fp32x" else "highest")
    try:
        yield AC.mode_dtype(mode)
    finally:
        maskunet_amd.set_float32_matmul_precision("highest")


def _pairs(cases):
    return [pytest.param(c, m, id=f"{c['id']}-{m}") for c in cases for m in c["modes"]]


def _same(a, b, what):
    assert a is not None and b is not None, what
    assert torch.equal(a, b), f"{what}: run B differs from the all-trainable run A (max |diff| {float((a.float() - b.float()).abs().max()):.3e})"


def _gate(name, e, tol):
    print(f"  {name}: {e:.3e} (gate {tol:.0e})")
    assert e <= tol, (name, e, tol)


def _param_err(got, ref, gmax, dtype, floor=None):
    """check_golden_module's rule: relative to max(|ref|max, floor * the case's largest parameter gradient)."""
    floor = PARAM_GRAD_FLOOR[dtype] * gmax if floor is None else floor
    return float((got.detach().float().cpu() - ref.float()).abs().max()) / max(float(ref.abs().max()), floor)


def _gmax(grads):
    return max([float(g.abs().max()) for g in grads if g is not None] or [1.0])


# ------------------------------------------------------------------------------------------------
# A. ops.conv alone
# ------------------------------------------------------------------------------------------------
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _run_conv(layer, needs, mode):
    from maskunet_amd import ops
    L = AC.CONV_LAYERS[layer]
    x, w, b, gy = AC.conv_inputs(layer, mode)
    with precision(mode) as dtype:
        leaves = [t.to(DEV).requires_grad_(bool(n)) for t, n in zip((x, w, b), needs)]
        y = ops.to_nchw(ops.conv(ops.to_nhwc(leaves[0], dtype), leaves[1], leaves[2]), L["cout"], torch.float32)
        y.backward(gy.to(DEV))
    return dict(y=y.detach(), dx=leaves[0].grad, dw=leaves[1].grad, db=leaves[2].grad)


@pytest.mark.parametrize("case,mode", _pairs(AC.CONV_CASES))
def test_conv_frozen_operands(case, mode):
    from maskunet_amd import _lib, ops
    layer, needs, L = case["layer"], case["needs"], AC.CONV_LAYERS[case["layer"]]
    dtype = AC.mode_dtype(mode)
    a = _memo(("conv", layer, mode), lambda: _run_conv(layer, (True, True, True), mode))
    b = _run_conv(layer, needs, mode)
    exempt = dict(case["exceptions"].get(mode, {}))
    if exempt and not _lib.load().mu_conv_wgrad_bias_supported(ops.pad32(L["cin"]), ops.pad32(L["cout"]), L["k"] ** 2, _lib.dt(dtype)):
        exempt = {}                          # this shape is on the other side of the plan: one kernel either way, no exception
    _same(a["y"], b["y"], "y")
    for k, n in zip(("dx", "dw", "db"), needs):
        if not n:
            assert b[k] is None, f"{k} delivered although not wanted"
        elif k not in exempt:
            _same(a[k], b[k], k)
    ref = AC.conv_ref(*AC.conv_inputs(layer, mode), needs)
    tol = TOL[dtype]
    _gate("y", _err(b["y"], ref["y"]), tol)
    if needs[0]:
        _gate("dx", _rel_err(b["dx"], ref["dx"]), tol)
    gmax = _gmax([ref["dw"], ref["db"]])
    for k in ("dw", "db"):
        if ref[k] is not None:
            _gate(k, _param_err(b[k], ref[k], gmax, dtype), tol)


# ------------------------------------------------------------------------------------------------
# B. ops.bn_act
# ------------------------------------------------------------------------------------------------
def _make_bn(st, training, momentum=0.1):
    bn = nn.BatchNorm2d(st["weight"].numel(), momentum=momentum, track_running_stats="running_mean" in st)
    bn.load_state_dict(st)
    return bn.to(DEV).train(training)


def _check_buffers(bn, st, training, what):
    """eval(): bit-unchanged; train(): advanced, the step counter by exactly one."""
    if "running_mean" not in st:
        assert bn.running_mean is None and bn.num_batches_tracked is None
        return
    if training:
        assert int(bn.num_batches_tracked) == int(st["num_batches_tracked"]) + 1, what
        assert not torch.equal(bn.running_mean.cpu(), st["running_mean"]) and not torch.equal(bn.running_var.cpu(), st["running_var"]), what
    else:
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            assert torch.equal(getattr(bn, k).cpu(), st[k]), f"{what}: {k} of a BatchNorm in eval() changed"


def _run_bn(case, mode, all_trainable):
    from maskunet_amd import ops
    x, res, gy, st = AC.bn_inputs(case, mode)
    C = case["C"]
    bn = _make_bn(st, case["training"], case["momentum"])
    affine = True if all_trainable else case["affine"]
    for p in bn.parameters():
        p.requires_grad_(affine)
    with precision(mode) as dtype:
        xd = x.to(DEV).requires_grad_(True if all_trainable else case["x_grad"])
        rd = None if res is None else res.to(DEV).requires_grad_(True if all_trainable else case["res"] == "grad")
        y = ops.to_nchw(ops.bn_act(ops.to_nhwc(xd, dtype), bn, case["act"], res=None if rd is None else ops.to_nhwc(rd, dtype)), C, torch.float32)
        if y.requires_grad:
            y.backward(gy.to(DEV))
    _check_buffers(bn, st, case["training"], case["id"])
    return dict(y=y.detach(), dx=xd.grad, dres=None if rd is None else rd.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad,
                running_mean=bn.running_mean, running_var=bn.running_var)


@pytest.mark.parametrize("case,mode", _pairs(AC.BN_CASES))
def test_bn_act_frozen_affine_and_eval_mode(case, mode):
    dtype = AC.mode_dtype(mode)
    a = _run_bn(case, mode, True)                       # same mode of the layer, everything trainable
    b = _run_bn(case, mode, False)
    want = dict(dx=case["x_grad"], dres=case["res"] == "grad", dgamma=case["affine"], dbeta=case["affine"])
    _same(a["y"], b["y"], "y")
    for k, n in want.items():
        if n:
            _same(a[k], b[k], k)
        else:
            assert b[k] is None, f"{k} delivered although not wanted"
    if case["track"]:
        _same(a["running_mean"], b["running_mean"], "running_mean")
        _same(a["running_var"], b["running_var"], "running_var")
    x, res, gy, st = AC.bn_inputs(case, mode)
    ref = AC.bn_act_ref(x, res, gy, st, case)
    tol = TOL[dtype]
    _gate("y", _err(b["y"], ref["y"]), tol)
    for k in ("dx", "dres", "dgamma", "dbeta"):          # as check_bn_act gates them
        if want[k]:
            _gate(k, _rel_err(b[k], ref[k]), tol)
    if case["track"]:
        _gate("running_mean", _err(b["running_mean"], ref["running_mean"]), tol)
        _gate("running_var", _err(b["running_var"], ref["running_var"]), tol)


@pytest.mark.parametrize("mode", AC.MODES)
def test_bn_cumulative_average_is_refused_before_any_launch(mode):
    """nn.BatchNorm2d(momentum=None) in train mode means a cumulative average with the factor 1 / num_batches_tracked, not momentum 0.1:
    refused by name, and the running buffers and the step counter stay untouched -- alone and at the head of a run of ConvBlocks."""
    import maskunet_amd
    from maskunet_amd import ops
    case = AC.BN_CUMULATIVE_CASE
    x, _res, _gy, st = AC.bn_inputs(case, mode)
    bn = _make_bn(st, True, None)
    with precision(mode) as dtype:
        with pytest.raises(RuntimeError, match="momentum=None"):
            ops.bn_act(ops.to_nhwc(x.to(DEV).requires_grad_(True), dtype), bn, case["act"])
        torch.cuda.synchronize()
        _check_buffers(bn, st, False, "refused layer")
        blk = maskunet_amd.ConvBlock(8, 19).to(DEV).set_compute_dtype(dtype).train()
        blk.conv_block[4].momentum = None
        before = {k: v.clone() for k, v in blk.state_dict().items()}
        with pytest.raises(RuntimeError, match="momentum=None"):
            blk(torch.randn(2, 8, 8, 8, device=DEV))
        torch.cuda.synchronize()
        assert all(torch.equal(v, before[k]) for k, v in blk.state_dict().items()), "a layer in front of the refused one advanced"


# ------------------------------------------------------------------------------------------------
# C. ops.bn_pair / the tail BatchNorm
# ------------------------------------------------------------------------------------------------
def _run_pair(case, mode, all_trainable):
    from maskunet_amd import ops
    x, gy, s1, s2 = AC.pair_inputs(case, mode)
    bns = [_make_bn(st, tr) for st, tr in zip((s1, s2), case["training"])]
    frozen = () if all_trainable else case["frozen"]
    for i, bn in enumerate(bns, 1):
        bn.weight.requires_grad_(f"g{i}" not in frozen)
        bn.bias.requires_grad_(f"b{i}" not in frozen)
    with precision(mode) as dtype:
        xd = x.to(DEV).requires_grad_(True if all_trainable else case["x_grad"])
        y = ops.to_nchw(ops.bn_pair(ops.to_nhwc(xd, dtype), bns[0], bns[1]), case["C"], torch.float32)
        y.backward(gy.to(DEV))
    out = dict(y=y.detach(), dx=xd.grad)
    for i, (bn, st, tr) in enumerate(zip(bns, (s1, s2), case["training"]), 1):
        _check_buffers(bn, st, tr, f"{case['id']} layer {i}")
        out.update({f"g{i}": bn.weight.grad, f"b{i}": bn.bias.grad, f"running_mean{i}": bn.running_mean, f"running_var{i}": bn.running_var})
    return out


@pytest.mark.parametrize("case,mode", _pairs(AC.PAIR_CASES))
def test_bn_pair_frozen_layers_and_mixed_modes(case, mode):
    dtype = AC.mode_dtype(mode)
    a = _run_pair(case, mode, True)
    b = _run_pair(case, mode, False)
    _same(a["y"], b["y"], "y")
    want = {k: k not in case["frozen"] for k in ("g1", "b1", "g2", "b2")}
    want["dx"] = case["x_grad"]
    for k, n in want.items():
        if n:
            _same(a[k], b[k], k)
        else:
            assert b[k] is None, f"{k} delivered although not wanted"
    for i in (1, 2):
        _same(a[f"running_mean{i}"], b[f"running_mean{i}"], f"running_mean{i}")
        _same(a[f"running_var{i}"], b[f"running_var{i}"], f"running_var{i}")
    ref = AC.bn_pair_ref(*AC.pair_inputs(case, mode), case)
    tol = TOL[dtype]
    _gate("y", _err(b["y"], ref["y"]), tol)
    if case["x_grad"]:
        _gate("dx", _rel_err(b["dx"], ref["dx"]), tol)
    # the case's gradient scale is that of its all-trainable form: in front of a training-mode BatchNorm gamma1 / beta1 have
    # analytically (near-)zero gradients -- rounding noise of sums of the second layer's scale, as check_bn_pair gates them -- and a
    # pattern that freezes the second layer would otherwise leave the floor to that noise itself
    full = AC.bn_pair_ref(*AC.pair_inputs(case, mode), dict(case, frozen=(), x_grad=True))
    gmax = _gmax([full[k] for k in ("g1", "b1", "g2", "b2")])
    for k in ("g1", "b1", "g2", "b2"):
        if want[k]:
            _gate(k, _param_err(b[k], ref[k], gmax, dtype), tol)
    for i in (1, 2):
        _gate(f"running_mean{i}", _err(b[f"running_mean{i}"], ref[f"running_mean{i}"]), tol)
        _gate(f"running_var{i}", _err(b[f"running_var{i}"], ref[f"running_var{i}"]), tol)


# ------------------------------------------------------------------------------------------------
# module cases (D, E): one runner
# ------------------------------------------------------------------------------------------------
def _build(kind):
    import maskunet_amd
    from maskunet_amd import modules, ops

    class Chain(modules._HipModule):
        """Three ConvBlocks as one run, the bottom chain's form (UNet._forward_nhwc)."""

        def __init__(self):
            super().__init__()
            self.blocks = nn.ModuleList([maskunet_amd.ConvBlock(ci, co) for (_p, ci, co, _m, _r) in AC.FORMS["chain3"]["blocks"]])

        def forward(self, x):
            y = modules._conv_blocks(ops.to_nhwc(x, self.compute_dtype), list(self.blocks))
            return ops.to_nchw(y, AC.FORMS["chain3"]["out"][0], x.dtype)

    if kind in AC.ATTN_BLOCKS:
        C = AC.ATTN_BLOCKS[kind]["C"]
        return maskunet_amd.Mask2FormerAttention(C, C)
    return {"stem": lambda: maskunet_amd.ConvBlock(3, 64), "res1": lambda: maskunet_amd.ConvBlock(64, 64, residual=True),
            "down": lambda: maskunet_amd.DownSample(64, 128), "up": lambda: maskunet_amd.UpSample(128, 64), "chain3": Chain}[kind]()


def _run_module(kind, params, ins, gout, mode, frozen, in_grads, bn_eval, keep=None, twice=False):
    """-> out, input gradients, parameter gradients and buffers by their "m."-prefixed names; asserts what both runs must hold."""
    with precision(mode) as dtype:
        m = _build(kind)
        m.load_state_dict({k[2:]: v for k, v in params.items()})
        m.to(DEV).set_compute_dtype(dtype).train()
        mods = dict(m.named_modules())
        for bn in bn_eval:
            mods[bn[2:]].eval()
        for k, p in m.named_parameters():
            p.requires_grad_("m." + k not in frozen)
        if keep is not None:
            m.set_keep_mask(keep)
        xs = [t.to(DEV).requires_grad_(bool(g)) for t, g in zip(ins, in_grads)]
        out = m(*xs)
        first = None
        if twice:                   # a second backward over the retained graph must give the same bits
            out.backward(gout.to(DEV), retain_graph=True)
            first = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
            for p in m.parameters():
                p.grad = None
        out.backward(gout.to(DEV))
        torch.cuda.synchronize()
    gparam = {"m." + k: p.grad for k, p in m.named_parameters()}
    if first is not None:
        assert first.keys() == {k[2:] for k, g in gparam.items() if g is not None}
        for k, g in first.items():
            _same(g, gparam["m." + k], f"second backward over the retained graph, {k}")
    for k in frozen:
        assert gparam[k] is None, f"{k} is frozen and got a gradient"
    for t, g in zip(xs, in_grads):
        assert (t.grad is not None) == bool(g)
    sd = {"m." + k: v for k, v in m.state_dict().items()}
    for name, mod in mods.items():
        if isinstance(mod, nn.BatchNorm2d):
            st = {k: params[f"m.{name}.{k}"] for k in ("running_mean", "running_var", "num_batches_tracked")}
            _check_buffers(mod, st, mod.training, name)
    return dict(out=out.detach(), gin=[t.grad for t in xs], gparam=gparam, sd=sd)


def _compare_module_runs(a, b, names, frozen, in_grads, stat_keys, exempt=()):
    _same(a["out"], b["out"], "out")
    for i, g in enumerate(in_grads):
        if g:
            _same(a["gin"][i], b["gin"][i], f"gin{i}")
    for k in names:
        if k not in frozen and k not in exempt:
            _same(a["gparam"][k], b["gparam"][k], k)
    for k in stat_keys:
        _same(a["sd"][k], b["sd"][k], k)


def _gate_module(b, ref, names, frozen, in_grads, dtype, stats=None, floors=None):
    tol = TOL[dtype]
    _gate("out", _err(b["out"], ref["out"]), tol)
    for i, g in enumerate(in_grads):
        if g:
            _gate(f"gin{i}", _rel_err(b["gin"][i], ref["gin"][i]), tol)
    gmax = _gmax([ref["gparam"][k] for k in names])
    for k in names:
        if k in frozen:
            assert ref["gparam"][k] is None
            continue
        _gate("d " + k, _param_err(b["gparam"][k], ref["gparam"][k], gmax, dtype, (floors or {}).get(k)), tol)
    for k, v in (stats or {}).items():
        if k.endswith("num_batches_tracked"):
            assert int(b["sd"][k]) == int(v), k
        else:
            _gate(k, _err(b["sd"][k], v), tol)


# ------------------------------------------------------------------------------------------------
# D. ops.conv_blocks through ConvBlock / DownSample / UpSample / a chain of three
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _pairs(AC.BLOCK_CASES))
def test_conv_blocks_partial_training(case, mode):
    form, frozen, in_grads, bn_eval = case["form"], set(case["frozen"]), case["in_grads"], case["bn_eval"]
    dtype = AC.mode_dtype(mode)
    params, ins, gout = AC.block_inputs(form, mode)
    names = AC.run_params(form)
    all_grads = (True,) * len(ins)
    b = _run_module(form, params, ins, gout, mode, frozen, in_grads, bn_eval)
    if frozen or in_grads != all_grads:
        # the twin: everything trainable under the SAME per-layer modes (a BatchNorm in eval() changes values by design)
        a = _memo(("blocks", form, mode, bn_eval), lambda: _run_module(form, params, ins, gout, mode, (), all_grads, bn_eval))
        stat_keys = [f"{bn}.{k}" for bn in AC.run_bns(form) for k in ("running_mean", "running_var", "num_batches_tracked")]
        _compare_module_runs(a, b, names, frozen, in_grads, stat_keys, case["exceptions"].get(mode, {}))
    ref = _memo(("blocks-ref", case["id"], mode == "fp16"), lambda: AC.block_ref(case, params, ins, gout))
    _gate_module(b, ref, names, frozen, in_grads, dtype, ref["stats"])


# ------------------------------------------------------------------------------------------------
# E. Mask2FormerAttention
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _pairs(AC.ATTN_CASES))
def test_attention_partial_training(case, mode):
    block, frozen, in_grads = case["block"], set(case["frozen"]), (case["x_grad"],)
    dtype = AC.mode_dtype(mode)
    params, x, gout, keep = AC.attn_inputs(block, mode)
    names = list(params)
    # the input-without-grad cases also run the backward a second time over the retained graph
    b = _run_module(block, params, [x], gout, mode, frozen, in_grads, (), keep=keep, twice=not case["x_grad"])
    a = _memo(("attn", block, mode), lambda: _run_module(block, params, [x], gout, mode, (), (True,), (), keep=keep))
    _compare_module_runs(a, b, names, frozen, in_grads, (), case["exceptions"].get(mode, {}))
    ref = _memo(("attn-ref", case["id"], mode == "fp16"), lambda: AC.attn_ref(case, params, x, gout, keep))
    floors = {}
    if mode == "fp32x" and "m.key.bias" not in frozen and ref["gparam"]["m.query.bias"] is not None:
        # check_golden_module's key.bias treatment (analytically zero; fp32x carries dS as one fp16 operand): the sibling's scale
        floors["m.key.bias"] = float(ref["gparam"]["m.query.bias"].abs().max())
    _gate_module(b, ref, names, frozen, in_grads, dtype, floors=floors)


# ------------------------------------------------------------------------------------------------
# what the forward keeps, and what a link is left with
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dw", [True, False])
def test_fp32x_conv_keeps_the_operand_its_backward_reads(dw):
    """ops._conv_fwd, `keep16 = x_enc and taps == 9 and needs[1]`: an fp32x matrix-core 3x3 layer keeps the fp16 rounding of its input
    for the one-term weight gradient -- and only then; with the weight frozen no rounding is made (the encoded operand of the forward
    stays, whose shape is all the data gradient reads)."""
    from maskunet_amd import ops
    x, w, _b, gy = AC.conv_inputs("mc3x3", "fp32x")
    with precision("fp32x") as dtype:
        xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(dw)
        y = ops.conv(ops.to_nhwc(xd, dtype), wd)
        kept = y.grad_fn.saved_tensors[0]
        assert kept.dtype == (torch.float16 if dw else torch.float32) and kept.shape == y.shape
        y.backward(ops.to_nhwc(gy.to(DEV), dtype))
    assert (wd.grad is not None) == dw and xd.grad is not None


def test_upcat_leaves_no_fill_for_a_skip_without_grad():
    """ops._UpCat.forward keeps skip_link only if the skip tensor requires grad: an armed link whose taker exists for another reason
    must not be filled with a gradient nobody asked for."""
    from maskunet_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 8, 64, generator=g).to(DEV).requires_grad_(True)
    skip = torch.randn(2, 16, 16, 64, generator=g).to(DEV)
    link = ops.GradLink()
    link.armed = True
    y = ops.upcat(x, skip, skip_link=link)
    y.backward(torch.randn(y.shape, generator=g).to(DEV))
    assert link.t is None and x.grad is not None and skip.grad is None
    # ... and with the skip requiring grad the armed link carries d(skip) instead of autograd
    skip.requires_grad_(True)
    y = ops.upcat(x, skip, skip_link=link)
    y.backward(torch.randn(y.shape, generator=g).to(DEV))
    assert link.t is not None and link.t.shape == skip.shape and skip.grad is None


# ------------------------------------------------------------------------------------------------
# F. whole UNet (hw = 64, B = 2, c_out = 19, dropout off, fixed keep masks), G. optimiser and accumulation
# ------------------------------------------------------------------------------------------------
def _unet_model(three_head, dtype, params, keeps):
    import maskunet_amd
    U = AC.UNET
    model = maskunet_amd.InstanceUNet(3, U["c_out"], 16, hw=U["hw"]) if three_head else maskunet_amd.UNet(3, U["c_out"], hw=U["hw"])
    model.load_state_dict(params)
    model.to(DEV).set_compute_dtype(dtype).train()
    model.dropout.p = 0.0
    model.set_keep_masks(keeps)
    return model


def _unet_step(model, x, labels, three_head, dtype, x_grad):
    """One forward and backward -> (outputs, input gradient); the parameter gradients carry the fp16 loss scale."""
    import torch.nn.functional as F
    from tests._gpu_checks import FP16_LOSS_SCALE
    xd = x.to(DEV).requires_grad_(x_grad)
    out = model(xd)
    outs = out if three_head else (out,)
    loss = AC.unet_loss(outs, labels.to(DEV), three_head, lambda o, t, ig: F.cross_entropy(o, t, ignore_index=ig))
    scale = 1.0 if dtype == torch.float32 else FP16_LOSS_SCALE
    (loss * scale).backward()
    return [o.detach() for o in outs], float(loss.detach()), xd.grad, scale


def _run_unet(recipe, mode, twin=False):
    """Run B of a recipe, or (twin) run A: everything trainable, the input requiring grad, every BatchNorm in train()."""
    R = AC.UNET_RECIPES[recipe]
    three = R["three_head"]
    params, keeps, x, labels = AC.unet_inputs(three)
    frozen = set() if twin else AC.unet_frozen(recipe, params)
    with precision(mode) as dtype:
        model = _unet_model(three, dtype, params, keeps)
        evals = []
        if not twin:
            for name, mod in model.named_modules():
                if isinstance(mod, nn.BatchNorm2d) and R["bn_eval"](name):
                    mod.eval()
                    evals.append(name)
            for k, p in model.named_parameters():
                p.requires_grad_(k not in frozen)
        outs, loss, gx, scale = _unet_step(model, x, labels, three, dtype, twin)
        torch.cuda.synchronize()
    assert (gx is not None) == twin
    for k, p in model.named_parameters():
        if k in frozen:
            assert p.grad is None, f"{k} is frozen and got a gradient"
    for name, mod in model.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            _check_buffers(mod, {k: params[f"{name}.{k}"] for k in ("running_mean", "running_var", "num_batches_tracked")}, mod.training, name)
    return dict(model=model, outs=outs, loss=loss, scale=scale, frozen=frozen, grads={k: p.grad for k, p in model.named_parameters()},
                sd={k: v for k, v in model.state_dict().items()})


_unet_ref = {}


def _unet_reference(recipe):
    if recipe not in _unet_ref:
        _unet_ref.clear()            # one retained fp64 graph at a time
        _unet_ref[recipe] = AC.UnetRef(recipe)
    return _unet_ref[recipe]


@pytest.mark.parametrize("case,mode", _pairs(AC.UNET_CASES))
def test_unet_partial_training(case, mode):
    from tests._gpu_checks import UNET_GRAD_COS, UNET_GRAD_FLOOR, UNET_GRAD_MAXREL
    recipe, R = case["recipe"], AC.UNET_RECIPES[case["recipe"]]
    dtype = AC.mode_dtype(mode)
    b = _run_unet(recipe, mode)
    if R["twin"]:
        a = _memo(("unet", R["three_head"], mode), lambda: {k: v for k, v in _run_unet(recipe, mode, twin=True).items() if k != "model"})
        for i, (u, v) in enumerate(zip(a["outs"], b["outs"])):
            _same(u, v, f"out{i}")
        for k, g in b["grads"].items():
            if k not in b["frozen"] and (g is not None or a["grads"][k] is not None):
                _same(a["grads"][k], g, k)
        for k, v in b["sd"].items():
            if "running" in k or "num_batches" in k:
                _same(a["sd"][k], v, k)
    ref = _unet_reference(recipe).finish((b["outs"][0] > 0).cpu())
    tol = TOL[dtype]
    for i, (o, r) in enumerate(zip(b["outs"], ref["outs"])):
        _gate(f"out{i}", _err(o, r), tol)
    _gate(f"final-ReLU decisions taken from the HIP path ({ref['forced']['n']}): largest overridden |pre-activation| / output scale",
          ref["forced"]["zrel"], tol)
    _gate("loss", abs(b["loss"] - ref["loss"]) / max(1.0, abs(ref["loss"])), tol)
    # check_unet_vs_oracle's gates: max-norm relative to max(|ref|max, floor) and, above the floor, 1 - cosine
    gmax = _gmax(ref["grads"].values())
    floor = UNET_GRAD_FLOOR[dtype] * gmax
    worst, worst_cos = (0.0, ""), (0.0, "")
    for k, g in b["grads"].items():
        r = ref["grads"][k]
        assert (g is None) == (r is None), k
        if r is None:
            continue
        g = g.double().cpu() / b["scale"]
        worst = max(worst, (float((g - r).abs().max()) / max(float(r.abs().max()), floor), k))
        if float(r.abs().max()) >= floor:
            worst_cos = max(worst_cos, (1.0 - float((g * r).sum() / (g.norm() * r.norm() + 1e-300)), k))
    _gate(f"worst param grad maxrel [{worst[1]}]", worst[0], UNET_GRAD_MAXREL[dtype])
    _gate(f"worst param grad 1-cos [{worst_cos[1]}]", worst_cos[0], UNET_GRAD_COS[dtype])
    stat = max([(_err(b["sd"][k], v), k) for k, v in ref["stats"].items()] or [(0.0, "")])
    _gate(f"worst running stat [{stat[1]}]", stat[0], tol)


def test_fused_adamw_after_a_frozen_encoder_step():
    """G (a): one FusedAdamW step after the frozen-encoder recipe leaves every frozen parameter bit-unchanged, and moves the trainable
    ones exactly as the same step from run A's (bit-identical) gradients does."""
    import maskunet_amd
    recipe = "encoder-frozen-bn-train"
    b = _run_unet(recipe, "fp32")
    a = _run_unet(recipe, "fp32", twin=True)
    pa = dict(a["model"].named_parameters())
    for k in b["frozen"]:                    # run A's model takes the same step: its encoder is frozen AFTER the backward
        pa[k].requires_grad_(False)
        pa[k].grad = None
    params0, _keeps, _x, _labels = AC.unet_inputs(False)
    for run in (a, b):
        maskunet_amd.FusedAdamW(run["model"].parameters(), lr=1e-3, weight_decay=1e-2).step()
    torch.cuda.synchronize()
    moved = 0
    for k, p in b["model"].named_parameters():
        if k in b["frozen"]:
            assert torch.equal(p.detach().cpu(), params0[k]), f"{k} is frozen and was changed by the optimiser"
        else:
            _same(pa[k].detach(), p.detach(), k)
            moved += int(not torch.equal(p.detach().cpu(), params0[k]))
    assert moved >= 60          # bottleneck, decoder, attention 4-6, LayerNorm and head: every parameter that has a gradient
    # the recipe proper (the encoder's BatchNorms in eval(): no twin): the step leaves the frozen encoder and its buffers as they were
    c = _run_unet("encoder-frozen-bn-eval", "fp32")
    maskunet_amd.FusedAdamW(c["model"].parameters(), lr=1e-3, weight_decay=1e-2).step()
    torch.cuda.synchronize()
    moved = 0
    for k, v in c["model"].state_dict().items():
        if k.startswith(AC.ENCODER):
            assert torch.equal(v.cpu(), params0[k]), f"{k} belongs to the frozen encoder and changed"
        elif k in c["grads"] and c["grads"][k] is not None:
            moved += int(not torch.equal(v.cpu(), params0[k]))
    assert moved >= 60


def test_gradient_accumulation_over_two_micro_batches_is_exact():
    """G (b): two micro-batches backpropagated without zero_grad leave p.grad == g1 + g2 (fp32, bit for bit), g1 / g2 from single
    backwards of fresh forwards -- in training mode no gradient depends on the running statistics the first forward advanced."""
    params, keeps, x, labels = AC.unet_inputs(False)
    g = torch.Generator().manual_seed(9)
    x2 = torch.rand(x.shape, generator=g)
    labels2 = torch.randint(0, AC.UNET["c_out"], labels.shape, generator=g)
    with precision("fp32") as dtype:
        singles = []
        for xi, li in ((x, labels), (x2, labels2)):
            m = _unet_model(False, dtype, params, keeps)
            _unet_step(m, xi, li, False, dtype, False)
            singles.append({k: p.grad for k, p in m.named_parameters()})
        m = _unet_model(False, dtype, params, keeps)
        _unet_step(m, x, labels, False, dtype, False)
        _unet_step(m, x2, labels2, False, dtype, False)
        torch.cuda.synchronize()
    n = 0
    for k, p in m.named_parameters():
        g1, g2 = singles[0][k], singles[1][k]
        assert (p.grad is None) == (g1 is None) == (g2 is None), k
        if g1 is not None:
            _same(g1 + g2, p.grad, k)
            n += 1
    assert n >= 150             # every parameter the forward uses (the dead emb_layer weights have no gradient)
