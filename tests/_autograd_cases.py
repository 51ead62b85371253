"""Partial training (frozen parameters, inputs without grad, single BatchNorm layers in eval()): the case tables and the fp64 CPU
references of tests/test_gpu_autograd_partial.py.  Importable without a GPU; tests/test_autograd_cases_host.py checks the references
against torch.nn modules in fp64 and the tables' coverage.

Two instruments (see the GPU test file): (1) bit identity of every tensor a frozen run B still computes with the all-trainable run A of
the same seeded state, (2) fp64 parity of run B with the references below under the project's own gates (_gpu_checks.TOL and the
floor rule of check_golden_module).  A case may name tensors that are EXEMPT from instrument 1 in some mode -- `exceptions`:
{mode: {tensor name: cause}} with the ops.py code that makes a different kernel produce the tensor; those are held to instrument 2.
"""
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import maskunet_oracle as O

MODES = ("fp32", "fp16", "fp32x")
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2          # == maskunet_amd._lib.ACT_* (checked by the host test where the library is built)

# |pre-activation| of every ReLU input and the gap between the two largest values of every 2x2 max-pool window, in the fp64 reference,
# on the inputs as the kernels see them (rounded to fp16 in the fp16 mode).  ReLU: the output gate is TOL * max(1, |ref|max) <= 3e-2 * 5
# for these inputs, so a pre-activation 0.2 away from zero cannot change sign inside the gate; max-pool: the pool compares its INPUT
# values, which are exact in every mode, so any gap above zero decides the window -- 0.05 is far above one fp16 ulp at |x| <= 8.
RELU_MARGIN = 0.2
POOL_MARGIN = 0.05


def mode_dtype(mode):
    return torch.float16 if mode == "fp16" else torch.float32


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def _round(t, mode):
    """The values the kernels see: fp16 storage rounds the inputs."""
    return t.half().float() if mode == "fp16" else t


# ------------------------------------------------------------------------------------------------
# A. ops.conv alone
# ------------------------------------------------------------------------------------------------
PATTERNS = [p for p in itertools.product((True, False), repeat=3) if any(p)]        # (dx, dw, db): all seven non-empty ones
CONV_LAYERS = {
    # name: kind (the three layer kinds the coverage condition counts), Cin, Cout, kernel, pixels
    "stem3x3": dict(kind="stem3x3", cin=3, cout=64, k=3, hw=8),            # plain-FMA stem
    "mc3x3": dict(kind="mc3x3", cin=64, cout=64, k=3, hw=16),              # matrix cores; fp32x: the _DyH / keep16 paths
    "1x1_64_19": dict(kind="1x1", cin=64, cout=19, k=1, hw=8),
    "1x1_64_64": dict(kind="1x1", cin=64, cout=64, k=1, hw=8),
    "1x1_64_192": dict(kind="1x1", cin=64, cout=192, k=1, hw=8),           # fp16: mu_conv_wgrad_bias_supported (the other side of that plan)
    "head3x3": dict(kind="head3x3", cin=19, cout=32, k=3, hw=8),           # boundary_head[0]'s form
}
WGRAD_BIAS_CAUSE = ("ops.py _conv_bwd: `both = _wgrad_bias_raw(...) if (m.has_bias and needs[2]) else None` -- with the bias frozen the weight "
                    "gradient comes from mu_conv_wgrad instead of mu_conv_wgrad_bias (fp16 1x1 layers on the wide tiles, where "
                    "mu_conv_wgrad_bias_supported); another summation order")

# (found by the first GPU run of this suite: 1x1_64_192, fp16, db differed from run A in the last bit, 4.8e-7)
COLSUM_CAUSE = ("ops.py _conv_bwd: `_wgrad_bias_raw` is asked only inside `if needs[1]:` -- with the WEIGHT frozen the bias gradient comes from "
                "mu_colsum (`if m.has_bias and needs[2] and gb is None`) instead of the ones column of mu_conv_wgrad_bias (fp16 1x1 layers "
                "on the wide tiles, where mu_conv_wgrad_bias_supported); another summation order")


def _conv_cases():
    out = []
    for name, L in CONV_LAYERS.items():
        pats = PATTERNS if name != "head3x3" else [(True, True, False), (True, False, True)]       # bias frozen / weight frozen
        for needs in pats:
            exc = {}
            if L["kind"] == "1x1" and needs[1] and not needs[2]:
                exc = {"fp16": {"dw": WGRAD_BIAS_CAUSE}}
            if L["kind"] == "1x1" and needs[2] and not needs[1]:
                exc = {"fp16": {"db": COLSUM_CAUSE}}
            out.append(dict(id=f"{name}-dx{int(needs[0])}dw{int(needs[1])}db{int(needs[2])}", layer=name, needs=needs, modes=MODES,
                            exceptions=exc))
    return out


CONV_CASES = _conv_cases()


def conv_inputs(layer, mode):
    L = CONV_LAYERS[layer]
    g = _rng("conv/" + layer)
    bound = 1.0 / np.sqrt(L["cin"] * L["k"] ** 2)
    x = _round(_t(g.standard_normal((2, L["cin"], L["hw"], L["hw"]))), mode)
    w = _t(g.uniform(-bound, bound, (L["cout"], L["cin"], L["k"], L["k"])))
    b = _t(g.uniform(-bound, bound, (L["cout"],)))
    gy = _round(_t(g.standard_normal((2, L["cout"], L["hw"], L["hw"]))), mode)
    return x, w, b, gy


def conv_ref(x, w, b, gy, needs):
    """fp64 F.conv2d with the (dx, dw, db) pattern as requires_grad -> {y, dx, dw, db} (None where not wanted)."""
    x, w, b = (t.double().clone().requires_grad_(bool(n)) for t, n in zip((x, w, b), needs))
    y = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
    y.backward(gy.double())
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad)


# ------------------------------------------------------------------------------------------------
# B. ops.bn_act
# ------------------------------------------------------------------------------------------------
def _bn_cases():
    out = []
    res_cycle = itertools.cycle((None, "grad", "nograd"))
    for act, training, affine in itertools.product((ACT_NONE, ACT_GELU, ACT_RELU), (True, False), (True, False)):
        res = next(res_cycle)
        C = 19 if act == ACT_RELU else 64
        out.append(dict(id=f"act{act}-{'train' if training else 'eval'}-affine{int(affine)}-res{res}", C=C, hw=8, act=act, training=training,
                        affine=affine, res=res, x_grad=True, track=True, momentum=0.1))
    # every residual form with every activation at least once more, the input without grad, and no running statistics at all
    extra = [dict(act=ACT_RELU, training=True, affine=True, res="grad"), dict(act=ACT_RELU, training=False, affine=False, res="nograd"),
             dict(act=ACT_GELU, training=True, affine=False, res="nograd"), dict(act=ACT_NONE, training=False, affine=True, res="grad"),
             dict(act=ACT_GELU, training=True, affine=True, res=None, x_grad=False),
             dict(act=ACT_RELU, training=False, affine=True, res="grad", x_grad=False),
             dict(act=ACT_GELU, training=True, affine=True, res=None, track=False),
             dict(act=ACT_RELU, training=False, affine=False, res="grad", track=False),          # eval() without buffers: batch statistics
             dict(act=ACT_NONE, training=False, affine=True, res=None, momentum=None),            # eval: the momentum is never read
             dict(act=ACT_NONE, training=True, affine=True, res=None, momentum=None, track=False)]
    for i, e in enumerate(extra):
        c = dict(C=19 if i % 2 else 64, hw=8, x_grad=True, track=True, momentum=0.1)
        c.update(e)
        c["id"] = (f"x{i}-act{c['act']}-{'train' if c['training'] else 'eval'}-affine{int(c['affine'])}-res{c['res']}-xg{int(c['x_grad'])}"
                   f"-track{int(c['track'])}-mom{c['momentum']}")
        out.append(c)
    for c in out:
        c["modes"] = MODES
        c["exceptions"] = {}
        c["relu_margin"] = RELU_MARGIN if c["act"] == ACT_RELU else None
    return out


BN_CASES = _bn_cases()
# the refused setting (ops._refuse_cumulative): train mode, running statistics, momentum=None
BN_CUMULATIVE_CASE = dict(id="momentum-none-train", C=19, hw=8, act=ACT_NONE, training=True, affine=True, res=None, x_grad=True, track=True,
                          momentum=None, modes=MODES, exceptions={}, relu_margin=None)


def bn_state(C, g, track=True):
    s = dict(weight=_t(g.uniform(0.5, 1.5, C)), bias=_t(g.uniform(-0.2, 0.2, C)))
    if track:
        s.update(running_mean=_t(g.normal(0.0, 0.1, C)), running_var=_t(g.uniform(0.5, 1.5, C)), num_batches_tracked=torch.zeros((), dtype=torch.int64))
    return s


def _act64(z, act):
    return {ACT_NONE: lambda t: t, ACT_GELU: F.gelu, ACT_RELU: torch.relu}[act](z)


def _bn_pre(x, res, st, training, eps=1e-5):
    """fp64 pre-activation res + BatchNorm2d(x), running buffers untouched."""
    use_batch = training or "running_mean" not in st
    y = F.batch_norm(x.double(), None if use_batch else st["running_mean"].double(), None if use_batch else st["running_var"].double(),
                     st["weight"].double(), st["bias"].double(), use_batch, 0.0, eps)
    return y if res is None else y + res.double()


def bn_inputs(case, mode):
    """x, res, gy, state.  ReLU cases: elements whose fp64 pre-activation is nearer to zero than the margin are pushed away from it (in x,
    a few rounds: the batch statistics move with x), so that no element has to be left out of the comparison."""
    g = _rng("bn/" + case["id"])
    C, hw = case["C"], case["hw"]
    st = bn_state(C, g, case["track"])
    x = _t(g.standard_normal((2, C, hw, hw))) * 1.5 + 0.3
    res = _t(g.standard_normal((2, C, hw, hw))) if case["res"] else None
    gy = _round(_t(g.standard_normal((2, C, hw, hw))), mode)
    x, res = _round(x, mode), (None if res is None else _round(res, mode))
    if case["act"] == ACT_RELU:
        sg = torch.sign(st["weight"])[None, :, None, None]
        for _ in range(50):
            pre = _bn_pre(x, res, st, case["training"])
            bad = pre.abs() < RELU_MARGIN + 0.05
            if not bad.any():
                break
            x = _round(torch.where(bad, x + 0.4 * torch.sign(pre).float() * sg, x), mode)
    return x, res, gy, st


def bn_act_ref(x, res, gy, st, case, eps=1e-5):
    """fp64 act(res + F.batch_norm(x)) with the case's flags -> outputs, gradients (None where not wanted) and the buffers afterwards."""
    x = x.double().clone().requires_grad_(case["x_grad"])
    r = None if res is None else res.double().clone().requires_grad_(case["res"] == "grad")
    w, b = (st[k].double().clone().requires_grad_(case["affine"]) for k in ("weight", "bias"))
    track = "running_mean" in st
    rm, rv = (st["running_mean"].double().clone(), st["running_var"].double().clone()) if track else (None, None)
    use_batch = case["training"] or not track
    mom = 0.0 if case["momentum"] is None else case["momentum"]
    pre = F.batch_norm(x, rm, rv, w, b, use_batch, mom, eps)
    if r is not None:
        pre = pre + r
    y = _act64(pre, case["act"])
    if y.requires_grad:
        y.backward(gy.double())
    nbt = None
    if track:
        nbt = st["num_batches_tracked"] + (1 if case["training"] else 0)
    return dict(y=y.detach(), pre=pre.detach(), dx=x.grad, dres=None if r is None else r.grad, dgamma=w.grad, dbeta=b.grad,
                running_mean=rm, running_var=rv, num_batches_tracked=nbt)


# ------------------------------------------------------------------------------------------------
# C. ops.bn_pair / the tail BatchNorm
# ------------------------------------------------------------------------------------------------
def _pair_cases():
    rows = [  # id, (bn1 training, tail training), frozen parameters, x requires grad
        ("fold-all-trainable", (True, True), (), True),
        ("fold-first-affine-frozen", (True, True), ("g1", "b1"), True),
        ("fold-second-affine-frozen", (True, True), ("g2", "b2"), True),
        ("fold-x-nograd", (True, True), (), False),
        ("fold-only-beta2", (True, True), ("g1", "b1", "g2"), False),
        ("train-then-eval", (True, False), (), True),
        ("eval-then-train", (False, True), (), True),
        ("eval-then-eval", (False, False), (), True),
        ("train-then-eval-first-frozen", (True, False), ("g1", "b1"), True),
        ("eval-then-train-second-frozen-x-nograd", (False, True), ("g2", "b2"), False),
    ]
    return [dict(id=i, C=C, hw=8, training=t, frozen=f, x_grad=xg, modes=MODES, exceptions={})
            for (i, t, f, xg), C in zip(rows, itertools.cycle((64, 19)))]


PAIR_CASES = _pair_cases()


def pair_inputs(case, mode):
    g = _rng("pair/" + case["id"])
    C, hw = case["C"], case["hw"]
    s1, s2 = bn_state(C, g), bn_state(C, g)
    x = _round(_t(g.standard_normal((2, C, hw, hw))) * 1.5 + 0.3, mode)
    gy = _round(_t(g.standard_normal((2, C, hw, hw))), mode)
    return x, gy, s1, s2


def bn_pair_ref(x, gy, s1, s2, case, eps=1e-5):
    """fp64 bn2(bn1(x)), each layer with its own training flag."""
    x = x.double().clone().requires_grad_(case["x_grad"])
    out = dict()
    y = x
    leaves = {}
    for i, (st, tr) in enumerate(zip((s1, s2), case["training"]), 1):
        w = st["weight"].double().clone().requires_grad_(f"g{i}" not in case["frozen"])
        b = st["bias"].double().clone().requires_grad_(f"b{i}" not in case["frozen"])
        rm, rv = st["running_mean"].double().clone(), st["running_var"].double().clone()
        y = F.batch_norm(y, rm, rv, w, b, tr, 0.1, eps)
        leaves[i] = (w, b)
        out.update({f"running_mean{i}": rm, f"running_var{i}": rv, f"num_batches_tracked{i}": st["num_batches_tracked"] + (1 if tr else 0)})
    if y.requires_grad:
        y.backward(gy.double())
    out.update(y=y.detach(), dx=x.grad)
    for i, (w, b) in leaves.items():
        out.update({f"g{i}": w.grad, f"b{i}": b.grad})
    return out


# ------------------------------------------------------------------------------------------------
# D. ops.conv_blocks through ConvBlock / DownSample / UpSample / a chain of three
# ------------------------------------------------------------------------------------------------
# form: blocks of the run as (prefix, Cin, Cout, mid, residual), tail BatchNorm prefix, inputs [(channels, pixels)], output (channels, pixels)
FORMS = {
    "stem": dict(blocks=[("m", 3, 64, None, False)], tail=None, ins=[(3, 16)], out=(64, 16)),                 # initial_conv's form, run of one
    "res1": dict(blocks=[("m", 64, 64, None, True)], tail=None, ins=[(64, 8)], out=(64, 8)),                  # residual block alone: no taker for its link
    "down": dict(blocks=[("m.maxpool_conv.1", 64, 64, None, True), ("m.maxpool_conv.2", 64, 128, None, False)], tail="m.maxpool_conv.3",
                 ins=[(64, 16)], out=(128, 8)),                                                                # link taken by the pool
    "up": dict(blocks=[("m.conv.0", 128, 128, None, True), ("m.conv.1", 128, 64, 64, False)], tail="m.conv.2", ins=[(64, 8), (64, 16)],
               out=(64, 16)),                                                                                  # link taken by the concat
    "chain3": dict(blocks=[("m.blocks.0", 64, 128, None, False), ("m.blocks.1", 128, 128, None, False), ("m.blocks.2", 128, 64, None, False)],
                   tail=None, ins=[(64, 8)], out=(64, 8)),                                                     # the bottom chain's form
}


def form_shapes(form):
    f = FORMS[form]
    if form == "down":
        return O._down_shapes("m", 64, 128)
    if form == "up":
        return O._up_shapes("m", 128, 64)
    return [s for (p, ci, co, mid, _) in f["blocks"] for s in O._conv_block_shapes(p, ci, co, mid)]


def run_params(form):
    """Parameter names of the run in the order ops.conv_blocks lists them: per block (w1, gamma1, beta1, w2, gamma2, beta2), then the tail's."""
    f = FORMS[form]
    names = [f"{p}.conv_block.{k}" for (p, *_r) in f["blocks"] for k in ("0.weight", "1.weight", "1.bias", "3.weight", "4.weight", "4.bias")]
    if f["tail"]:
        names += [f["tail"] + ".weight", f["tail"] + ".bias"]
    return names


def run_bns(form):
    f = FORMS[form]
    return [f"{p}.conv_block.{k}" for (p, *_r) in f["blocks"] for k in (1, 4)] + ([f["tail"]] if f["tail"] else [])


def break_position(form, frozen, in_grads):
    """Which exit _ConvBlocks.backward takes: (block index, 1 = behind the second conv's backward, 2 = behind the first conv's), or None
    when the walk reaches the input -- the rule of ops._ConvBlocks.forward.req restated: the activation in front of parameter k requires
    grad when the input or any parameter before k does."""
    names = run_params(form)
    need = [n not in frozen for n in names]
    if any(in_grads):
        return None
    first = need.index(True) if any(need) else len(need)
    nblk = len(FORMS[form]["blocks"])
    for i in reversed(range(nblk)):
        if first >= 6 * i + 3:
            return (i, 1)
        if first >= 6 * i:
            return (i, 2)
    return None


def _block_cases():
    out = []
    for form, f in FORMS.items():
        names, nblk, nin = run_params(form), len(f["blocks"]), len(f["ins"])
        bns = run_bns(form)
        no_grad = (False,) * nin
        rows = [("all-trainable", (), (True,) * nin, ())]
        # the walk back stops at every position: the input without grad and every parameter in front of position j frozen
        for i in range(nblk):
            rows.append((f"first-trainable-b{i}-conv1", tuple(names[:6 * i]), no_grad, ()))
            rows.append((f"first-trainable-b{i}-bn1", tuple(names[:6 * i + 1]), no_grad, ()))             # i = 0: "first conv frozen"
            rows.append((f"first-trainable-b{i}-conv2", tuple(names[:6 * i + 3]), no_grad, ()))
        last_conv = names[6 * (nblk - 1) + 3]
        rows.append(("only-last-conv", tuple(n for n in names if n != last_conv), no_grad, ()))
        rows.append(("only-last-conv-x-grad", tuple(n for n in names if n != last_conv), (True,) * nin, ()))
        if f["tail"]:
            rows.append(("only-tail-bn", tuple(n for n in names if not n.startswith(f["tail"])), no_grad, ()))
        rows.append(("bn-affine-frozen", tuple(n for n in names if ".conv_block.0." not in n and ".conv_block.3." not in n), (True,) * nin, ()))
        rows.append(("convs-frozen", tuple(n for n in names if ".conv_block.0." in n or ".conv_block.3." in n), (True,) * nin, ()))
        rows.append(("all-bn-eval", (), (True,) * nin, tuple(bns)))
        rows.append(("all-bn-eval-affine-frozen-x-nograd", tuple(n for n in names if ".conv_block.0." not in n and ".conv_block.3." not in n),
                     no_grad, tuple(bns)))
        if f["tail"]:
            rows.append(("tail-eval", (), (True,) * nin, (f["tail"],)))                                   # must not fold
            rows.append(("last-bn-eval-tail-train", (), (True,) * nin, (bns[-2],)))                       # must not fold either
        if form == "up":
            rows.append(("skip-nograd", (), (True, False), ()))
            rows.append(("x-nograd", (), (False, True), ()))
            rows.append(("skip-nograd-first-conv-frozen", (names[0],), (True, False), ()))
        for rid, frozen, in_grads, bn_eval in rows:
            out.append(dict(id=f"{form}-{rid}", form=form, frozen=frozen, in_grads=in_grads, bn_eval=bn_eval, run_length=nblk,
                            break_pos=break_position(form, frozen, in_grads), pool_margin=POOL_MARGIN if form == "down" else None,
                            modes=MODES, exceptions={}))
    return out


BLOCK_CASES = _block_cases()


def block_inputs(form, mode):
    """(state_dict with the prefix "m.", inputs NCHW, gout).  DownSample: the largest value of every 2x2 window of the input is raised
    so that the window's arg-max holds by POOL_MARGIN."""
    f = FORMS[form]
    params = O.make_params(form_shapes(form), zlib.crc32(("blocks/" + form).encode()) % 10000)
    g = _rng("blocks-in/" + form)
    ins = [_t(g.standard_normal((2, c, hw, hw))) for c, hw in f["ins"]]
    if form == "down":
        x = ins[0]
        B, C, H, W = x.shape
        win = x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4).clone()
        win.scatter_add_(-1, win.argmax(-1, keepdim=True), torch.full(win.shape[:-1] + (1,), 2 * POOL_MARGIN))
        ins[0] = win.reshape(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W).contiguous()
    ins = [_round(t, mode) for t in ins]
    gout = _round(_t(g.standard_normal((2, f["out"][0], f["out"][1], f["out"][1]))), mode)
    return params, ins, gout


def pool_gap(x):
    """Smallest gap between the two largest values of a 2x2 window."""
    B, C, H, W = x.shape
    win = x.double().reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    top = win.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def oracle_leaves(params, frozen):
    """fp64 copies of a state dict for the oracle: floating parameters as leaves that require grad unless frozen, buffers plain."""
    p = {}
    for k, v in params.items():
        if v.dtype.is_floating_point:
            v = v.double().clone()
            if "running" not in k:
                v.requires_grad_(k not in frozen)
        else:
            v = v.clone()
        p[k] = v
    return p


def form_forward(form, p, ins, training, new_stats):
    """The oracle's forward of a form; `training`: bool or callable(prefix)."""
    f = FORMS[form]
    if form == "down":
        return O.downsample(ins[0], p, "m", training, new_stats)
    if form == "up":
        return O.upsample(ins[0], ins[1], p, "m", training, new_stats)
    y = ins[0]
    for (pre, _ci, _co, _mid, residual) in f["blocks"]:
        y = O.conv_block(y, p, pre, residual, training, new_stats)
    return y


def block_ref(case, params, ins, gout):
    """fp64 oracle run of a D case -> out, input gradients, parameter gradients {name: grad or None}, running statistics afterwards."""
    p = oracle_leaves(params, set(case["frozen"]))
    xs = [t.double().clone().requires_grad_(g) for t, g in zip(ins, case["in_grads"])]
    ns = {}
    ev = set(case["bn_eval"])
    y = form_forward(case["form"], p, xs, lambda prefix: prefix not in ev, ns)
    if y.requires_grad:
        y.backward(gout.double())
    stats = {}
    for bn in run_bns(case["form"]):
        for k in ("running_mean", "running_var"):
            stats[f"{bn}.{k}"] = ns.get(f"{bn}.{k}", p[f"{bn}.{k}"])
        stats[bn + ".num_batches_tracked"] = params[bn + ".num_batches_tracked"] + (0 if bn in ev else 1)
    return dict(out=y.detach(), gin=[t.grad for t in xs], gparam={k: p[k].grad for k in run_params(case["form"])}, stats=stats)


# ------------------------------------------------------------------------------------------------
# E. Mask2FormerAttention
# ------------------------------------------------------------------------------------------------
ATTN_BLOCKS = {"c64": dict(C=64, hw=8), "c48-padded": dict(C=48, hw=8), "c288-wide": dict(C=288, hw=8)}
_QKV = tuple(f"m.{n}.{k}" for n in ("query", "key", "value") for k in ("weight", "bias"))
_LN = ("m.norm.weight", "m.norm.bias")
ATTN_PATTERNS = {
    "x-nograd": dict(frozen=(), x_grad=False),                     # gx is None, ctx.wd is None
    "qkv-frozen": dict(frozen=_QKV, x_grad=True),
    "ln-frozen": dict(frozen=_LN, x_grad=True),
    "only-value": dict(frozen=tuple(n for n in _QKV + _LN if ".value." not in n), x_grad=False),
}
WIDE_FP32X_REASON = "fp32x runs the wide (C > 256) block in exact fp32: the same kernels as the fp32 case"
ATTN_CASES = [dict(id=f"{b}-{pn}", block=b, frozen=pt["frozen"], x_grad=pt["x_grad"], exceptions={},
                   modes=MODES if b != "c288-wide" else ("fp32", "fp16"), left_out={} if b != "c288-wide" else {"fp32x": WIDE_FP32X_REASON})
              for b in ATTN_BLOCKS for pn, pt in ATTN_PATTERNS.items()]


def attn_inputs(block, mode):
    A = ATTN_BLOCKS[block]
    C, hw = A["C"], A["hw"]
    params = O.make_params(O._attn_shapes("m", C), zlib.crc32(("attn/" + block).encode()) % 10000)
    g = _rng("attn-in/" + block)
    x = _round(_t(g.standard_normal((2, C, hw, hw))), mode)
    gout = _round(_t(g.standard_normal((2, C, hw, hw))), mode)
    keep = torch.from_numpy(g.integers(0, 2, size=(2, hw * hw)).astype(np.uint8))
    keep[:, 0] = 1                                                   # never an image without a visible key
    return params, x, gout, keep


def attn_ref(case, params, x, gout, keep):
    p = oracle_leaves(params, set(case["frozen"]))
    xr = x.double().clone().requires_grad_(case["x_grad"])
    y = O.mask_attention(xr, p, "m", keep)
    y.backward(gout.double())
    return dict(out=y.detach(), gin=[xr.grad], gparam={k: p[k].grad for k in params})


# ------------------------------------------------------------------------------------------------
# F. whole UNet, G. optimiser and accumulation
# ------------------------------------------------------------------------------------------------
UNET = dict(hw=64, B=2, c_out=19, seed=4100)
ENCODER = ("initial_conv.", "downsample1.", "downsample2.", "downsample3.", "self_attention1.", "self_attention2.", "self_attention3.")
_HEADS = ("boundary_head.", "embedding_head.")


def _is_bn_affine(k, bn_prefixes):
    return k.rsplit(".", 1)[0] in bn_prefixes


# frozen(k, bn_prefixes): parameter k is frozen; bn_eval(prefix): that BatchNorm runs in eval(); twin: no BatchNorm mode changes, so the
# all-trainable run A computes the same values (instrument 1 applies)
UNET_RECIPES = {
    "encoder-frozen-bn-eval": dict(three_head=False, frozen=lambda k, bns: k.startswith(ENCODER), bn_eval=lambda pre: pre.startswith(ENCODER),
                                   twin=False),
    "encoder-frozen-bn-train": dict(three_head=False, frozen=lambda k, bns: k.startswith(ENCODER), bn_eval=lambda pre: False, twin=True),
    "only-final-layer": dict(three_head=False, frozen=lambda k, bns: not k.startswith("final_layer."), bn_eval=lambda pre: False, twin=True),
    "bn-frozen-and-eval": dict(three_head=False, frozen=_is_bn_affine, bn_eval=lambda pre: True, twin=False),
    "three-head-heads-only": dict(three_head=True, frozen=lambda k, bns: not k.startswith(_HEADS), bn_eval=lambda pre: False, twin=True),
}
UNET_CASES = [dict(id=k, recipe=k, modes=MODES, exceptions={}) for k in UNET_RECIPES]


def unet_inputs(three_head):
    U = UNET
    params = O.make_params(O.unet_state_shapes(3, U["c_out"], three_head, hw=U["hw"]), U["seed"])
    keeps = O.make_keeps(U["seed"] + 1, U["B"], U["hw"])
    x, labels = O.make_inputs(U["seed"] + 2, U["B"], U["c_out"], U["hw"], ignore_frac=0.1 if three_head else 0.0)
    return params, keeps, x, labels


def bn_prefixes(params):
    return {k[:-len(".running_mean")] for k in params if k.endswith(".running_mean")}


def unet_frozen(recipe, params):
    R, bns = UNET_RECIPES[recipe], bn_prefixes(params)
    return {k for k, v in params.items() if v.dtype.is_floating_point and "running" not in k and R["frozen"](k, bns)}


def unet_loss(outs, labels, three_head, xent):
    loss = xent(outs[0], labels, 255 if three_head else -100)
    if three_head:
        loss = loss + 0.5 * outs[2].square().mean() + 0.25 * outs[1].square().mean()
    return loss


class _Trunk(Exception):
    pass


class UnetRef:
    """fp64 oracle run of a recipe.  The trunk (everything in front of the heads) runs once and keeps its graph; finish(dec) runs the
    heads and the backward for one set of final-ReLU decisions `dec` (taken from the HIP run, as check_unet_vs_oracle injects them: a
    pre-activation inside the forward noise may land on either side of zero, and the overridden ones are held to the output gate)."""

    def __init__(self, recipe):
        R = UNET_RECIPES[recipe]
        self.three = R["three_head"]
        self.params, keeps, x, self.labels = unet_inputs(self.three)
        self.frozen = unet_frozen(recipe, self.params)
        self.p = oracle_leaves(self.params, self.frozen)
        self.training = lambda prefix: prefix != "dropout" and not R["bn_eval"](prefix)
        self.ns = {}
        kept = {}
        head = O.head_1x1_bn_relu

        def stop(xh, ph, prefix, training, new_stats=None):
            kept["xh"] = xh
            raise _Trunk

        O.head_1x1_bn_relu = stop
        try:
            O.unet_forward(self.p, x.double(), keeps, training=self.training, new_stats=self.ns, three_head=self.three)
        except _Trunk:
            pass
        finally:
            O.head_1x1_bn_relu = head
        self.xh = kept["xh"]

    def finish(self, dec):
        p, ns = self.p, dict(self.ns)
        for v in p.values():
            v.grad = None
        y = O.batchnorm2d(F.conv2d(self.xh, p["final_layer.0.weight"], p["final_layer.0.bias"]), p, "final_layer.1", self.training, ns)
        diff = (y.detach() > 0) != dec
        forced = dict(n=int(diff.sum()), zrel=0.0)
        if forced["n"]:
            forced["zrel"] = float(y.detach().abs()[diff].max()) / max(1.0, float(y.detach().abs().max()))
        sem = y * dec.to(y.dtype)
        outs = (sem,)
        if self.three:        # the order of oracle.unet_forward: embedding head, semantic head, boundary head on the semantic output
            emb = O.head_1x1_bn_relu(self.xh, p, "embedding_head", self.training, ns)
            outs = (sem, O.boundary_head(sem, p, "boundary_head", self.training, ns), emb)
        loss = unet_loss(outs, self.labels, self.three, O.pixel_cross_entropy)
        loss.backward(retain_graph=True)
        grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in p.items() if v.dtype.is_floating_point and "running" not in k}
        return dict(outs=[o.detach() for o in outs], loss=float(loss.detach()), grads=grads, stats=ns, forced=forced)


ALL_TABLES = dict(conv=CONV_CASES, bn_act=BN_CASES + [BN_CUMULATIVE_CASE], bn_pair=PAIR_CASES, blocks=BLOCK_CASES, attention=ATTN_CASES, unet=UNET_CASES)
