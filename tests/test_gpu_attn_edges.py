"""The flash-style attention sweeps of maskunet_amd/csrc/attn.hip (C in {32, 64, 128, 256}; MU_F16, MU_F32, MU_F32X) through the C ABI
-- mu_attn_fwd_padded and mu_attn_bwd_phases_padded -- against the float64 reference of tests/_attn_reference.py, element by element,
each element against its own first-order bound and, on the Gaussian cases, each tensor against today's gate as well (derived there; tests/test_attn_reference_host.py checks on the CPU that the bounds hold
a model of the kernels' roundings with a factor 2 to spare, that they stay within today's per-tensor gate on ordinary inputs, and that
they report a list of deliberately wrong kernels).  One test id per (dtype, width, sweep); every id prints its worst err / bound per
tensor and its case count (pytest -s / -rP).

The shapes are the smallest that reach each edge (R.cases): kcnt around the key tiles of the forward and of the dQ sweep, around the
keys of a dK/dV block and with kcnt % 16 in {1, 15}; N in {4, 12, 20, 36, 128, 132, 260} (the forward also 5 and 17) against the
128-query block and the 16-query wave tile; 1 to 10 query tiles of 32 against the dK/dV ring of 4 or 2; the compact key list (nkmax <
N) and the whole permutation with MU_ATTN_KIDX_PERMUTATION (blocks with every key masked, a masked key inside the last kept block),
MU_ATTN_DQKV_ENCODED for fp32x; ragged batches of three; c_valid < C; the row blocks of the LayerNorm passes with B x N = 4 x 16388
at the 1024-block cap; and the value regimes of R.make_inputs (overflow redo with the hot key in buffer 1, in a later full tile and in
the partial last tile; a score just below the redo threshold; fp16-subnormal probabilities; rising maxima; one kept key; large x).

The backward is handed the REFERENCE's forward results rounded to their storage types, so its bounds hold no forward error.  Every
operand and the workspace sit in tests/_device_buffers.Guarded buffers: after each call the guard bands are intact and the inputs
byte-identical; outputs and the workspace start as the sentinel and the outputs are wholly written.  Exact, with no tolerance (a zero
bound): dK / dV rows of masked keys and the pad channels of every output are zeros; replacing the K and V parts of masked rows by other
finite values changes no output byte; an image run alone gives the bytes it gives inside its ragged batch (out, oattn, lse2, mean,
rstd, dY, delta, and dqkv for fp16 / fp32 -- the fp32x dqkv is computed under the batch-wide scale of dY, as documented).

Outside the contract and NOT probed: kcnt = 0 (tests/_gpu_checks.check_attention_no_visible_key), N % 4 != 0 in the backward, indices
out of range, infinities or NaNs in the inputs."""
import time

import numpy as np
import pytest
import torch

from tests import _attn_reference as R
from tests._device_buffers import Guarded

pytestmark = pytest.mark.gpu

CODE = {"f32": 0, "f16": 1, "f32x": 2}
TORCH = {"f16": torch.float16, "f32": torch.float32, "f32x": torch.float32}
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
COMBOS = [(dt, C) for dt in R.DTYPES for C in R.WIDTHS]
FWD_ARGS = ("qkv", "x", "kidx", "kcnt", "gamma", "beta", "out", "oattn", "lse2", "mean", "rstd", "B", "N", "C", "c_valid", "nkmax", "eps", "dtype")
BWD_ARGS = ("qkv", "x", "oattn_in", "gout", "kidx", "kcnt", "lse2_in", "mean_in", "rstd_in", "gamma", "dY", "delta", "dqkv", "dgamma", "dbeta",
            "B", "N", "C", "c_valid", "nkmax", "ws", "ws_bytes", "dtype", "phases")
ALONE_KEYS = ("out", "oattn", "lse2", "mean", "rstd", "dY", "delta", "dqkv")


def _call(name, *args):
    from maskunet_amd import _lib
    try:
        _lib.call(name, *[a.p if isinstance(a, Guarded) else a for a in args], _lib.stream())
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" not in str(e):                        # a refusal, a missing symbol, ...: an ordinary test failure
            raise
        pytest.exit(f"{name}: the device reported {e}; nothing more is started on it", returncode=3)
    for a in args:
        if isinstance(a, Guarded):
            a.check()                                        # guard bands intact; an input is byte-identical


def _in(a, dtype, name):
    a = np.ascontiguousarray(a)
    return Guarded(a.size, dtype, data=a, name=name)


def _run(inp, bufs, saved_bufs, backward, flags, images=None):
    """one forward and (backward) one backward call on `images` of the case (all of them by default); every output as a host array"""
    from maskunet_amd import _lib
    dt, N, C, cv, nkmax = inp["dt"], inp["N"], inp["C"], inp["cv"], inp["nkmax"]
    T = TORCH[dt]
    sel = slice(None) if images is None else images
    B = len(inp["kcnt"][sel])
    a = {"qkv": _in(bufs["qkv"][sel], T, "qkv"), "x": _in(bufs["x"][sel], T, "x"), "kidx": _in(inp["kidx"][sel], I32, "kidx"),
         "kcnt": _in(inp["kcnt"][sel], I32, "kcnt"), "gamma": _in(bufs["gamma"], F32, "gamma"), "beta": _in(bufs["beta"], F32, "beta"),
         "out": Guarded(B * N * C, T, name="out"), "oattn": Guarded(B * N * C, T, name="oattn"),
         **{k: Guarded(B * N, F32, name=k) for k in ("lse2", "mean", "rstd")},
         "B": B, "N": N, "C": C, "c_valid": cv, "nkmax": nkmax, "eps": R.EPS, "dtype": CODE[dt]}
    _call("mu_attn_fwd_padded", *[a[k] for k in FWD_ARGS])
    res = {}
    for k in R.FWD_KEYS:
        a[k].all_written()
        res[k] = a[k].host((B, N, C) if k in ("out", "oattn") else (B, N))
    if not backward:
        return res
    ws_bytes = int(_lib.load().mu_attn_bwd_workspace_bytes(B, N, C))
    a.update({"gout": _in(bufs["gout"][sel], T, "gout"), "oattn_in": _in(saved_bufs["oattn"][sel], T, "oattn"),
              **{k + "_in": _in(saved_bufs[k][sel], F32, k) for k in ("lse2", "mean", "rstd")},
              "dY": Guarded(B * N * C, T, name="dY"), "delta": Guarded(B * N, F32, name="delta"), "dqkv": Guarded(B * N * 3 * C, T, name="dqkv"),
              "dgamma": Guarded(C, F32, name="dgamma"), "dbeta": Guarded(C, F32, name="dbeta"), "ws": Guarded(ws_bytes, U8, name="ws"),
              "ws_bytes": ws_bytes, "phases": 7 | (8 if inp["form"] == "perm" else 0) | flags})
    assert bool((a["ws"].t == a["ws"].sent).all())
    _call("mu_attn_bwd_phases_padded", *[a[k] for k in BWD_ARGS])
    for k, shape in (("dY", (B, N, C)), ("delta", (B, N)), ("dqkv", (B, N, 3 * C)), ("dgamma", (C,)), ("dbeta", (C,))):
        a[k].all_written()
        res[k] = a[k].host(shape)
    return res


def _other_masked_kv(case, p):
    """the buffers of the case with the K and V parts of every MASKED row replaced by other ordinary values (the Q parts and the kept
    rows keep their bytes; fp32x: the K | V columns of a row are whole 32-byte groups of the encoding)"""
    inp, C = p["inp"], p["inp"]["C"]
    gen = R.rng(99, case["seed"])
    buf = np.array(p["bufs"]["qkv"])
    for b in range(inp["B"]):
        masked = np.setdiff1d(np.arange(inp["N"]), inp["kidx"][b, :inp["kcnt"][b]])
        new = gen.standard_normal((len(masked), 2, C)) * 3.0
        new[:, :, inp["cv"]:] = 0
        old = buf[b, masked, C:].copy()
        buf[b, masked, C:] = R.stored_qkv(new.reshape(len(masked), 2 * C), inp["dt"])[1]
        assert len(masked) == 0 or not np.array_equal(old, buf[b, masked, C:])
    return dict(p["bufs"], qkv=buf)


@pytest.mark.parametrize("sweep", R.SWEEPS)
@pytest.mark.parametrize("dt,C", COMBOS)
def test_attn_edges(dt, C, sweep):
    t0 = time.time()
    assert R.tiles_from_source(dt, C) == R.TILE_TABLE[dt, C]
    worst, gate, ncase, ncall = {}, {}, 0, 0
    for case in R.cases(dt, C, sweep):
        p = R.prepare(case)
        inp, bwd, flags = p["inp"], not case["fwd_only"], case["flags"]
        got = _run(inp, p["bufs"], p["saved_bufs"], bwd, flags)
        ncase, ncall = ncase + 1, ncall + 1 + bwd
        for k in R.FWD_KEYS + (R.BWD_KEYS if bwd else ()):
            ref = p["ref"][k] if k in R.FWD_KEYS else p["refb"][k]
            val = R.decode_bf(got[k]) if (k == "dqkv" and flags & 16) else got[k]
            r, i = R.worst(val, ref, p["bd"][k])
            if r > worst.get(k, (-1.0,))[0]:
                worst[k] = (r, case["name"])
            print(f"attn-edges {case['name']} {k}: err / bound {r:.3f}")
            assert r <= 1.0, (case["name"], k, r, np.unravel_index(i, ref.shape), float(np.asarray(val, np.float64).flat[i]), float(ref.flat[i]),
                              float(p["bd"][k].flat[i]))
            # today's per-tensor gate as well, on every Gaussian case: the worst-case bound of fp32x stands above its 1e-3 (one fp16
            # term per score), so the new suite asks no less of any dtype than tests/_gpu_checks.check_attention does
            if case["normal"] and R.gate_factor(case, k) is not None:
                e = R.gate_err(val, ref)
                gate[k] = max(gate.get(k, 0.0), e / R.TOL[dt])
                assert e <= R.TOL[dt], (case["name"], k, "error over tensor max", e, R.TOL[dt])
        # exact zeros, asserted on the bytes as well (the bound of these elements is 0 above): pad channels, masked keys' dK / dV rows
        cv = inp["cv"]
        for k in ("out", "oattn") + (("dY",) if bwd else ()):
            assert not got[k][..., cv:].any(), (case["name"], k, "pad channels")
        if bwd:
            dq = R.decode_bf(got["dqkv"]) if flags & 16 else got["dqkv"]
            for i in range(3):
                assert not dq[..., i * C + cv:(i + 1) * C].any(), (case["name"], "dqkv pad channels")
            assert not got["dgamma"][cv:].any() and not got["dbeta"][cv:].any(), (case["name"], "dgamma / dbeta pad channels")
            for b in range(inp["B"]):
                masked = np.setdiff1d(np.arange(inp["N"]), inp["kidx"][b, :inp["kcnt"][b]])
                assert not dq[b, masked, C:].any(), (case["name"], b, "dK / dV rows of masked keys")
        if inp["B"] == 3 and inp["N"] <= 300:
            # masked rows' K / V are never read into a result
            alt = _run(inp, _other_masked_kv(case, p), p["saved_bufs"], bwd, flags)
            for k in got:
                assert alt[k].tobytes() == got[k].tobytes(), (case["name"], k, "changed with the K / V values of masked rows")
            # every image alone gives its bytes of the batch
            for b in range(3):
                one = _run(inp, p["bufs"], p["saved_bufs"], bwd, flags, images=slice(b, b + 1))
                for k in ALONE_KEYS:
                    if k in one and not (k == "dqkv" and dt == "f32x"):
                        assert one[k][0].tobytes() == got[k][b].tobytes(), (case["name"], k, f"image {b} alone differs from the batch")
            ncall += 4 * (1 + bwd)
    dtm = time.time() - t0
    print(f"attn-edges {dt} C={C} {sweep}: {ncase} cases, {ncall} calls, {dtm:.1f} s; worst err / bound " +
          " ".join(f"{k}:{v[0]:.3f}" for k, v in worst.items()))
    print(f"attn-edges {dt} C={C} {sweep}: worst err / (TOL x tensor max) " + " ".join(f"{k}:{v:.3f}" for k, v in gate.items()))
    print(f"attn-edges {dt} C={C} {sweep}: worst at " + "; ".join(f"{k}: {v[1]}" for k, v in worst.items() if v[0] > 0.25))
