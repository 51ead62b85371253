"""tests/_attn_reference.py on the CPU, before tests/test_gpu_attn_edges.py relies on it: the float64 reference against float64 torch
autograd on the dense masked form; the rounding model within HALF of every bound on every case (so no bound is unreachably tight) and,
on the normal-magnitude cases, no bound above today's per-tensor gate (so none is loose); the case tables against the tile constants
in attn.hip and the regimes against the reference; and the comparator against a list of deliberately wrong results."""
import math

import numpy as np
import pytest
import torch

from tests import _attn_reference as R

COMBOS = [(dt, C) for dt in R.DTYPES for C in R.WIDTHS]


@pytest.mark.parametrize("dt,C", COMBOS)
def test_tile_table_matches_source(dt, C):
    assert R.tiles_from_source(dt, C) == R.TILE_TABLE[dt, C]


@pytest.mark.parametrize("dt,C", COMBOS)
def test_case_tables_reach_their_edges(dt, C):
    fkt, dqkt, blk, ring = R.TILE_TABLE[dt, C]
    seen = {sw: R.cases(dt, C, sw) for sw in R.SWEEPS}
    for sw, kt in (("fwd", fkt), ("dq", dqkt)):
        kc = {n for c in seen[sw] for n in c["kcnt"]}
        assert set(R.edge_counts(kt)) <= kc, (sw, sorted(set(R.edge_counts(kt)) - kc))
        ns = {c["N"] for c in seen[sw]}
        assert {4, 12, 20, 36, 128, 132, 260} <= ns
    assert {5, 17} <= {c["N"] for c in seen["fwd"] if c["fwd_only"]}
    kc = {n for c in seen["dkv"] for n in c["kcnt"]}
    assert {blk - 1, blk, blk + 1, 2 * blk + 1} <= kc and {1, 15} <= {n % 16 for n in kc}
    assert {32, 36, 64, 96, 128, 160, 164, 288, 292} <= {c["N"] for c in seen["dkv"]}
    tiles = {-(-c["N"] // 32) for c in seen["dkv"]}
    assert set(range(1, 11)) - {7, 8} <= tiles and any(t > ring and t % ring for t in tiles)
    forms = {(c["form"], bool(c["flags"] & 16)) for sw in R.SWEEPS for c in seen[sw]}
    assert ("compact", False) in forms and ("perm", False) in forms and ((("perm", True) in forms) == (dt == "f32x"))
    for sw in R.SWEEPS:
        for c in seen[sw]:
            assert c["fwd_only"] or c["N"] % 4 == 0, c["name"]
            assert min(c["kcnt"]) >= 1 and max(c["kcnt"]) <= c["N"], c["name"]
        if sw != "ln":
            assert any(c["form"] == "compact" and max(c["kcnt"]) < c["N"] for c in seen[sw]), (sw, "no compact list with nkmax < N")
    assert {c["cv"] for c in seen["ln"]} >= {cv for cv, Cc in ((1, 32), (31, 32), (33, 64), (200, 256)) if Cc == C}
    assert {4, 63, 64, 65, 127, 197} <= {c["N"] for c in seen["ln"] if c["cv"] < C}
    if C == 32:
        big = [c for c in seen["ln"] if c["N"] == 16388]
        assert len(big) == 1 and len(big[0]["kcnt"]) == 4 and max(big[0]["kcnt"]) <= 8
        rows = 4 * 16388                                     # the block count sits at its cap and a block takes 65 rows, not 64
        assert R.ln_row_blocks(rows) == R.LN_MAXBLK and rows > 64 * R.LN_MAXBLK and -(-rows // R.LN_MAXBLK) == 65
        assert R.pshift_of(16388) == 12 and R.pshift_of(4) == 0
    regs = {c["regime"].split(":")[0] for c in seen["fwd"]} | {c["regime"] for c in seen["ln"]}
    assert {"normal", "flat", "rising", "ln"} <= regs and (dt == "f32" or {"hot", "near"} <= regs)


@pytest.mark.parametrize("sweep", R.SWEEPS)
@pytest.mark.parametrize("dt,C", COMBOS)
def test_bounds_hold_the_model_and_meet_the_gate(dt, C, sweep):
    """Condition 1: on every case the rounding model's error is at most HALF of every element's bound.  Condition 2: on every Gaussian
    case no element's bound exceeds TOL[dtype] x the tensor's maximum x R.gate_factor (1 but for the derived exceptions there).
    fp32x cannot meet its own 1e-3 with a worst-case bound: every score carries one fp16 operand rounding (attn.hip 231-251), h A_ij
    with A the ABSOLUTE sum of the products, where the gate is met only because those D roundings are random-signed.  Its bound is
    asserted against the fp16-class gate, TOL['f16'], and its own gate is kept as a SECOND assertion on the error itself: the model
    here, the kernel in tests/test_gpu_attn_edges.py, within TOL[dtype] x tensor max on every Gaussian case, for every dtype."""
    w1, w2, w3, n = 0.0, 0.0, 0.0, 0
    for case in R.cases(dt, C, sweep):
        p = R.prepare(case)
        assert R.regime_reached(p["inp"], p["ref"])
        with np.errstate(invalid="ignore", over="ignore"):
            m = R.model(p["inp"], p["saved"])
        for k in R.FWD_KEYS + (() if case["fwd_only"] else R.BWD_KEYS):
            ref = p["ref"][k] if k in R.FWD_KEYS else p["refb"][k]
            got = R.decode_bf(R.encode_bf(m[k])) if (k == "dqkv" and case["flags"] & 16) else m[k]
            r, i = R.worst(got, ref, p["bd"][k])
            w1 = max(w1, r)
            assert r <= 0.5, (case["name"], k, r, i)
            assert np.isfinite(p["bd"][k]).all(), (case["name"], k)
            if case["normal"]:
                f = R.gate_factor(case, k)
                if f is None:                                # c_valid = 1: the constant beta forward; backward, the rounding of the saved
                    # oattn / mean times rstd (xhat) and rstd again (dY): the bound against 1 / eps x the gate, relative to the inputs
                    if k == "out":
                        assert np.abs(ref[..., 0] - p["inp"]["beta"][0]).max() <= 1e-3, (case["name"], "out is not beta")
                    top = max(float(np.abs(ref).max()), float(np.abs(p["inp"]["gout"]).max()))
                    assert p["bd"][k].max() / top <= R.TOL["f16" if dt == "f32x" else dt] / R.EPS, (case["name"], k)
                    continue
                g = float(p["bd"][k].max() / max(np.abs(ref).max(), 1e-300)) / f
                w2 = max(w2, g / R.TOL[dt])
                assert g <= R.TOL["f16" if dt == "f32x" else dt], (case["name"], k, g)
                e = R.gate_err(got, ref)
                w3 = max(w3, e / R.TOL[dt])
                assert e <= R.TOL[dt], (case["name"], k, e)
        n += 1
    print(f"attn-edges host {dt} C={C} {sweep}: {n} cases, model worst err / bound {w1:.3f}, worst bound / gate {w2:.3f}, model err / gate {w3:.3f}")


def _torch_block(inp, b):
    C, cv, N = inp["C"], inp["cv"], inp["N"]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)          # noqa: E731
    qkv, gamma, beta = t(inp["qkv"][b]).requires_grad_(True), t(inp["gamma"]).requires_grad_(True), t(inp["beta"]).requires_grad_(True)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    mask = torch.full((N,), -math.inf, dtype=torch.float64)
    mask[torch.as_tensor(inp["kidx"][b, :inp["kcnt"][b]].astype(np.int64))] = 0.0
    o = torch.softmax(q @ k.T / math.sqrt(cv) + mask[None, :], dim=1) @ v
    y = torch.nn.functional.layer_norm((o + t(inp["x"][b]))[:, :cv], (cv,), gamma[:cv], beta[:cv], R.EPS)
    (y * t(inp["gout"][b])[:, :cv]).sum().backward()
    return o.detach().numpy(), y.detach().numpy(), qkv.grad.numpy(), gamma.grad.numpy(), beta.grad.numpy()


@pytest.mark.parametrize("case", [R._case("f32", 32, 36, (1, 19, 36), form="perm", seed=1), R._case("f16", 64, 68, (33, 68), cv=33, seed=2),
                                  R._case("f32x", 128, 20, (7,), seed=3), R._case("f32", 256, 12, (12, 5), cv=200, form="perm", seed=4)],
                         ids=lambda c: c["name"])
def test_reference_is_float64_autograd(case):
    """dense {0, -inf} key mask, softmax, P V, LayerNorm over the first cv channels; the backward from the reference's OWN unrounded
    forward results"""
    inp, _ = R.make_inputs(case)
    ref = R.reference_fwd(inp)
    refb = R.reference_bwd(inp, {k: ref[k] for k in ("oattn", "lse2", "mean", "rstd")})
    dga, dbe = 0.0, 0.0
    for b in range(inp["B"]):
        o, y, dqkv, g1, g2 = _torch_block(inp, b)
        dga, dbe = dga + g1, dbe + g2
        np.testing.assert_allclose(ref["oattn"][b], o, rtol=0, atol=1e-12)
        np.testing.assert_allclose(ref["out"][b][:, :inp["cv"]], y, rtol=0, atol=1e-11)
        assert not ref["out"][b][:, inp["cv"]:].any()
        np.testing.assert_allclose(refb["dqkv"][b], dqkv, rtol=0, atol=1e-11)
    np.testing.assert_allclose(refb["dgamma"], dga, rtol=0, atol=1e-10)
    np.testing.assert_allclose(refb["dbeta"], dbe, rtol=0, atol=1e-10)


WRONG_CASES = {
    "mask_left": dict(N=68, kcnt=(65,)), "no_rescale": dict(N=260, kcnt=(193,), regime="rising"), "last_tile": dict(N=68, kcnt=(65,)),
    "dk_neighbour": dict(N=36, kcnt=(19,)), "no_delta": dict(N=36, kcnt=(19,)), "pad_queries": dict(N=36, kcnt=(19,)),
    "scale_C": dict(N=36, kcnt=(19,), cv=33, C=64), "icv_D": dict(N=36, kcnt=(19,), cv=33, C=64),
}


# (no_rescale: fp32 tracks the maximum on every tile -- rising maxima; the fp16-operand types rescale only in the redo -- a hot key in the
#  second key tile, whose redo has to rescale what the first tile accumulated)
@pytest.mark.parametrize("wrong,dt", [(w, dt) for w in R.WRONG for dt in R.DTYPES])
def test_comparator_reports_wrong_results(wrong, dt):
    """each deliberately wrong kernel (model() with one line changed) is outside a bound, and the unchanged model is inside all"""
    kw = dict(WRONG_CASES[wrong])
    if wrong == "no_rescale" and dt != "f32":
        kw["regime"] = f"hot:{R.TILE_TABLE[dt, 32][0] + 1}"
    case = R._case(dt, kw.pop("C", 32), kw.pop("N"), kw.pop("kcnt"), seed=7, **kw)
    p = R.prepare(case)
    with np.errstate(invalid="ignore", over="ignore"):
        good, bad = R.model(p["inp"], p["saved"]), R.model(p["inp"], p["saved"], wrong=wrong)
    ratios = {}
    for k in R.FWD_KEYS + R.BWD_KEYS:
        ref = p["ref"][k] if k in R.FWD_KEYS else p["refb"][k]
        assert R.worst(good[k], ref, p["bd"][k])[0] <= 0.5, k
        ratios[k] = R.worst(bad[k], ref, p["bd"][k])[0]
    print(f"attn-edges host wrong={wrong} {dt}: " + " ".join(f"{k}:{v:.3g}" for k, v in ratios.items()))
    assert max(ratios.values()) > 1.0, ratios


def test_encodings_round_trip():
    a = R.rng(5).standard_normal((6, 16)).astype(np.float32)
    hi, lo = R.pair(a)
    e = R.encode_h(a).view(np.float16).reshape(-1, 16)
    assert np.array_equal(e[:, :8].astype(np.float32).reshape(a.shape), hi) and np.array_equal(e[:, 8:].astype(np.float32).reshape(a.shape), lo)
    d = R.decode_bf(R.encode_bf(a))
    assert np.abs(d - a).max() <= R.BF_PAIR * np.abs(a).max()
