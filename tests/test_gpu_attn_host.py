"""The host layer of the flash-style attention entry points (maskunet_amd/csrc/attn.hip): what mu_attn_fwd_padded and
mu_attn_bwd_phases_padded refuse, in which order, and that a refused call enqueues nothing; the workspace boundary; and that the
forwarding entry points (mu_attn_fwd, mu_attn_bwd, mu_attn_bwd_phases) and a backward split into its phases give the bytes of the
one-call forms.  The numerics of the sweeps are tests/_gpu_checks.check_attention*'s business, not this file's.

Every tensor operand sits in a tests/_device_buffers.Guarded buffer, as in tests/test_gpu_attn_wide_edges.py: after each call the
guard bands are intact and the inputs byte-identical; after a refused call every output still holds its sentinel.

Refusal order (include/maskunet_hip.h): a null pointer, a non-positive B / N / nkmax or c_valid outside 1..C is MU_ERR_ARG; then
(backward) a workspace below the query is MU_ERR_WORKSPACE; then an unknown dtype is MU_ERR_ARG; then (backward) N % 4 != 0, or a C
the sweeps have no width for, is MU_ERR_SHAPE."""
import numpy as np
import pytest
import torch

from tests._device_buffers import Guarded

pytestmark = pytest.mark.gpu

MU_F32, MU_F16, MU_F32X = 0, 1, 2
BAD_DTYPE = 7
DTYPES = {"f32": (MU_F32, torch.float32), "f16": (MU_F16, torch.float16), "f32x": (MU_F32X, torch.float32)}
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
EPS = 1e-5
C_MAX = 512                                      # the widest (refused) C a call is made with: dqkv and the workspace are sized for it
FWD_ARGS = ("qkv", "x", "kidx", "kcnt", "gamma", "beta", "out", "oattn", "lse2", "mean", "rstd", "B", "N", "C", "c_valid", "nkmax", "eps", "dtype")
BWD_ARGS = ("qkv", "x", "oattn", "gout", "kidx", "kcnt", "lse2", "mean", "rstd", "gamma", "dY", "delta", "dqkv", "dgamma", "dbeta", "B", "N", "C",
            "c_valid", "nkmax", "ws", "ws_bytes", "dtype", "phases")
FWD_PTRS, BWD_PTRS = FWD_ARGS[:11], BWD_ARGS[:15] + ("ws",)
FWD_OUTS = ("out", "oattn", "lse2", "mean", "rstd")


# ================================================================================================
# plumbing
# ================================================================================================
def _raw(a):
    return a.p if isinstance(a, Guarded) else a


def _guards(args):
    for a in args:
        if isinstance(a, Guarded):
            a.check()


def _call(name, *args):
    from maskunet_amd import _lib
    _lib.call(name, *[_raw(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    _guards(args)


def _refused(code, name, *args, outs):
    """`code` before anything is enqueued: after a synchronise every output still holds the sentinel"""
    from maskunet_amd import _lib
    with pytest.raises(RuntimeError, match=code):
        _lib.call(name, *[_raw(a) for a in args], _lib.stream())
    torch.cuda.synchronize()
    _guards(list(args) + list(outs))
    for o in outs:
        assert bool((o.t == o.sent).all()), (name, code, o.name, "written by a refused call")


def _query(B, N, C):
    from maskunet_amd import _lib
    return int(_lib.load().mu_attn_bwd_workspace_bytes(B, N, C))


def _inputs(name, B, N, C, seed=0):
    """qkv (fp32x: in the fp16-pair encoding the sweeps read), x, grad_out, a key list of whole permutations with the kept keys first
    (at least one kept key per image), gamma / beta"""
    from maskunet_amd import _lib
    T = DTYPES[name][1]
    rng = np.random.default_rng(seed)
    qkv = torch.from_numpy(rng.standard_normal((B, N, 3 * C)).astype(np.float32) * 0.5).to(T)
    if name == "f32x":
        q = qkv.cuda()
        _lib.call("mu_split_encode_h", q.data_ptr(), q.data_ptr(), q.numel(), _lib.stream())
        torch.cuda.synchronize()
        qkv = q.cpu()
    keep = rng.integers(0, 2, size=(B, N)).astype(np.uint8)
    keep[:, N // 2] = 1
    kidx = np.argsort(-keep.astype(np.int64), axis=1, kind="stable").astype(np.int32)
    d = {"qkv": Guarded(qkv.numel(), T, data=qkv.numpy(), name="qkv"),
         "x": Guarded(B * N * C, T, data=rng.standard_normal(B * N * C).astype(np.float32), name="x"),
         "gout": Guarded(B * N * C, T, data=rng.standard_normal(B * N * C).astype(np.float32), name="gout"),
         "kidx": Guarded(B * N, I32, data=kidx, name="kidx"),
         "kcnt": Guarded(B, I32, data=keep.sum(1).astype(np.int32), name="kcnt"),
         "gamma": Guarded(C, F32, data=(1.0 + 0.1 * rng.standard_normal(C)).astype(np.float32), name="gamma"),
         "beta": Guarded(C, F32, data=(0.1 * rng.standard_normal(C)).astype(np.float32), name="beta")}
    return d


def _fwd_outs(name, B, N, C):
    T = DTYPES[name][1]
    return {"out": Guarded(B * N * C, T, name="out"), "oattn": Guarded(B * N * C, T, name="oattn"), "lse2": Guarded(B * N, F32, name="lse2"),
            "mean": Guarded(B * N, F32, name="mean"), "rstd": Guarded(B * N, F32, name="rstd")}


def _bwd_outs(name, B, N, C, ws_bytes, c_alloc=None):
    T = DTYPES[name][1]
    return {"dY": Guarded(B * N * C, T, name="dY"), "delta": Guarded(B * N, F32, name="delta"),
            "dqkv": Guarded(B * N * 3 * (c_alloc or C), T, name="dqkv"), "dgamma": Guarded(C, F32, name="dgamma"),
            "dbeta": Guarded(C, F32, name="dbeta"), "ws": Guarded(ws_bytes, U8, name="ws")}


def _forward(name, ins, B, N, C, entry="mu_attn_fwd"):
    """one forward through `entry`; returns its outputs"""
    o = _fwd_outs(name, B, N, C)
    a = dict(ins, **o, B=B, N=N, C=C, c_valid=C, nkmax=N, eps=EPS, dtype=DTYPES[name][0])
    _call(entry, *[a[k] for k in FWD_ARGS if entry.endswith("_padded") or k != "c_valid"])
    return o


def _saved(name, fwd, B, N, C):
    """the forward's outputs as INPUTS of the backward (checked unchanged after every call)"""
    T = DTYPES[name][1]
    return {"oattn": Guarded(B * N * C, T, data=fwd["oattn"].host(), name="oattn"),
            **{k: Guarded(B * N, F32, data=fwd[k].host(), name=k) for k in ("lse2", "mean", "rstd")}}


def _bytes(outs, keys):
    return {k: outs[k].host().tobytes() for k in keys}


# ================================================================================================
# refusals
# ================================================================================================
_REFUSAL_CASE = {}


def _refusal_case(name):
    """B = 2, N = 64, C = 32: the inputs, and output buffers that start as the sentinel and -- nothing being enqueued -- stay so, shared
    by the refusal tests of one dtype.  dqkv and the workspace are sized for C = 512, the widest refused call."""
    if name not in _REFUSAL_CASE:
        B, N, C = 2, 64, 32
        ins = _inputs(name, B, N, C)
        T = DTYPES[name][1]
        # (the backward's saved inputs are never read by a refused call: constants do)
        ins.update(oattn_in=Guarded(B * N * C, T, data=np.zeros(B * N * C, dtype=np.float32), name="oattn"),
                   **{k + "_in": Guarded(B * N, F32, data=np.ones(B * N, dtype=np.float32), name=k) for k in ("lse2", "mean", "rstd")})
        _REFUSAL_CASE[name] = (ins, _fwd_outs(name, B, N, C), _bwd_outs(name, B, N, C, _query(B, N, C_MAX), c_alloc=C_MAX))
    return _REFUSAL_CASE[name]


def _fwd_ok(name):
    ins, fo, _ = _refusal_case(name)
    return dict({k: ins[k] for k in ("qkv", "x", "kidx", "kcnt", "gamma", "beta")}, **fo, B=2, N=64, C=32, c_valid=32, nkmax=64, eps=EPS,
                dtype=DTYPES[name][0])


def _bwd_ok(name):
    ins, _, bo = _refusal_case(name)
    return dict({k: ins[k] for k in ("qkv", "x", "gout", "kidx", "kcnt", "gamma")}, oattn=ins["oattn_in"], lse2=ins["lse2_in"], mean=ins["mean_in"],
                rstd=ins["rstd_in"], **bo, B=2, N=64, C=32, c_valid=32, nkmax=64, ws_bytes=_query(2, 64, 32), dtype=DTYPES[name][0], phases=7)


def _refuse_fwd(name, code, **bad):
    a = {**_fwd_ok(name), **bad}
    _refused(code, "mu_attn_fwd_padded", *[a[k] for k in FWD_ARGS], outs=list(_refusal_case(name)[1].values()))


def _refuse_bwd(name, code, **bad):
    """a short workspace is short of the query of the tuple as it stands; every other call has the query's size"""
    a = {**_bwd_ok(name), **bad}
    short = a.pop("short", False)
    if a["B"] > 0 and a["N"] > 0:
        a["ws_bytes"] = _query(a["B"], a["N"], a["C"]) - int(short)
    _refused(code, "mu_attn_bwd_phases_padded", *[a[k] for k in BWD_ARGS], outs=list(_refusal_case(name)[2].values()))


ARG_FAULTS = (dict(B=0), dict(B=-1), dict(N=0), dict(N=-4), dict(nkmax=0), dict(nkmax=-1), dict(c_valid=0), dict(c_valid=-1), dict(c_valid=33),
              dict(dtype=BAD_DTYPE), dict(dtype=-1))
SHAPE_FAULTS = (dict(N=6), dict(C=96), dict(C=512))


@pytest.mark.parametrize("name", DTYPES)
def test_fwd_refusals(name):
    """every null pointer, B / N / nkmax / c_valid out of range and a dtype code no type has: MU_ERR_ARG; C = 96 and C = 512:
    MU_ERR_SHAPE; a bad dtype comes before the width.  (No N % 4 rule in the forward: N = 6 is a valid call.)"""
    for p in FWD_PTRS:
        _refuse_fwd(name, "MU_ERR_ARG", **{p: None})
    for bad in ARG_FAULTS:
        _refuse_fwd(name, "MU_ERR_ARG", **bad)
    for C in (96, 512):
        _refuse_fwd(name, "MU_ERR_SHAPE", C=C)
        _refuse_fwd(name, "MU_ERR_ARG", C=C, dtype=BAD_DTYPE)
        _refuse_fwd(name, "MU_ERR_ARG", C=C, x=None)


@pytest.mark.parametrize("name", DTYPES)
def test_bwd_refusals(name):
    """every null pointer (the workspace included), B / N / nkmax / c_valid out of range, a dtype code no type has: MU_ERR_ARG; a
    workspace one byte below the query: MU_ERR_WORKSPACE; N = 6, C = 96, C = 512 (with their own query's workspace): MU_ERR_SHAPE.
    Pairs: null + short workspace -> ARG, short workspace + bad dtype -> WORKSPACE, short workspace + N = 6 / C = 96 -> WORKSPACE, bad
    dtype + C = 96 / N = 6 -> ARG.  Every output still holds its sentinel.  The MU_ERR_SHAPE calls here ask for phases 2 | 4 only: with
    phase 1 they are test_bwd_shape_refusals_leave_dqkv's."""
    for p in BWD_PTRS:
        _refuse_bwd(name, "MU_ERR_ARG", **{p: None})
        _refuse_bwd(name, "MU_ERR_ARG", short=True, **{p: None})
    for bad in ARG_FAULTS:
        _refuse_bwd(name, "MU_ERR_ARG", **bad)
    _refuse_bwd(name, "MU_ERR_ARG", short=True, c_valid=33)
    _refuse_bwd(name, "MU_ERR_WORKSPACE", short=True)
    _refuse_bwd(name, "MU_ERR_WORKSPACE", short=True, dtype=BAD_DTYPE)
    for bad in SHAPE_FAULTS:
        _refuse_bwd(name, "MU_ERR_SHAPE", phases=6, **bad)
        _refuse_bwd(name, "MU_ERR_WORKSPACE", short=True, **bad)
        _refuse_bwd(name, "MU_ERR_ARG", dtype=BAD_DTYPE, **bad)
    _refuse_bwd(name, "MU_ERR_SHAPE", phases=6, N=6, C=96)


@pytest.mark.parametrize("name", DTYPES)
def test_bwd_shape_refusals_leave_dqkv(name):
    """MU_ERR_SHAPE with phases & 1 and no permutation promise (N = 6; C = 96; C = 512): dqkv still holds its sentinel -- the memset of
    dqkv is enqueued only after the last check has passed.  This is the ONE assertion of this file that a library built before the
    refusal came first fails (it zeroed dqkv, then returned MU_ERR_SHAPE); every other test of the file passes against such a build."""
    for bad in SHAPE_FAULTS:
        for phases in (1, 7):
            _refuse_bwd(name, "MU_ERR_SHAPE", phases=phases, **bad)


# ================================================================================================
# the workspace boundary
# ================================================================================================
@pytest.mark.parametrize("B,N,C", [(2, 64, 32), (1, 36, 128)])
@pytest.mark.parametrize("name", ["f16", "f32x"])
def test_workspace_exactly_the_query(name, B, N, C):
    """ws_bytes exactly mu_attn_bwd_workspace_bytes succeeds and a full backward leaves the guard bytes behind the workspace intact
    (fp32x is the dtype that uses its last region, the encoded dY; N = 36: a partial 32-row tile of row constants); one byte less is
    MU_ERR_WORKSPACE and writes nothing."""
    ins = _inputs(name, B, N, C, seed=1)
    saved = _saved(name, _forward(name, ins, B, N, C), B, N, C)
    q = _query(B, N, C)
    bo = _bwd_outs(name, B, N, C, q)
    a = dict({k: ins[k] for k in ("qkv", "x", "gout", "kidx", "kcnt", "gamma")}, **saved, **bo, B=B, N=N, C=C, c_valid=C, nkmax=N, ws_bytes=q - 1,
             dtype=DTYPES[name][0], phases=7)
    _refused("MU_ERR_WORKSPACE", "mu_attn_bwd_phases_padded", *[a[k] for k in BWD_ARGS], outs=list(bo.values()))
    a["ws_bytes"] = q
    _call("mu_attn_bwd_phases_padded", *[a[k] for k in BWD_ARGS])          # (_call: guard bands of every buffer, the workspace's included)
    for k in ("dY", "delta", "dqkv", "dgamma", "dbeta"):
        assert np.isfinite(bo[k].host().astype(np.float64)).all(), (k, "not finite")


# ================================================================================================
# the forwarding entry points and the phases
# ================================================================================================
@pytest.mark.parametrize("flags", [0, 8])
@pytest.mark.parametrize("name", ["f16", "f32x"])
def test_backward_forms_agree_bitwise(name, flags):
    """mu_attn_bwd (no flags), mu_attn_bwd_phases with 7 and three calls with 1, 2, 4 (with and without the permutation promise, which
    moves the masked keys' zero rows from the memset into the dK/dV sweep): the same bytes in dY, delta, dqkv, dgamma, dbeta"""
    B, N, C = 2, 64, 32
    ins = _inputs(name, B, N, C, seed=2)
    saved = _saved(name, _forward(name, ins, B, N, C), B, N, C)
    q, keys = _query(B, N, C), ("dY", "delta", "dqkv", "dgamma", "dbeta")

    def run(entry, phase_list):
        bo = _bwd_outs(name, B, N, C, q)
        a = dict({k: ins[k] for k in ("qkv", "x", "gout", "kidx", "kcnt", "gamma")}, **saved, **bo, B=B, N=N, C=C, nkmax=N, ws_bytes=q,
                 dtype=DTYPES[name][0])
        for ph in phase_list:
            a["phases"] = None if ph is None else ph | flags
            _call(entry, *[a[k] for k in BWD_ARGS if k != "c_valid" and not (k == "phases" and ph is None)])
        return _bytes(bo, keys)

    want = run("mu_attn_bwd_phases", [7])
    forms = [("three phase calls", run("mu_attn_bwd_phases", [1, 2, 4]))]
    if flags == 0:
        forms.append(("mu_attn_bwd", run("mu_attn_bwd", [None])))
    for what, got in forms:
        for k in keys:
            assert got[k] == want[k], f"{name} flags {flags}: {k} of {what} differs from mu_attn_bwd_phases(7)"


@pytest.mark.parametrize("name", DTYPES)
def test_fwd_padded_with_full_width_is_fwd(name):
    """mu_attn_fwd_padded with c_valid == C: the bytes of mu_attn_fwd in out, oattn, lse2, mean, rstd"""
    B, N, C = 2, 64, 32
    ins = _inputs(name, B, N, C, seed=3)
    a = _bytes(_forward(name, ins, B, N, C), FWD_OUTS)
    b = _bytes(_forward(name, ins, B, N, C, entry="mu_attn_fwd_padded"), FWD_OUTS)
    for k in FWD_OUTS:
        assert a[k] == b[k], f"{name}: {k} of mu_attn_fwd_padded(c_valid = C) differs from mu_attn_fwd"
