"""The flash-style masked attention block of maskunet_amd/csrc/attn.hip (C in {32, 64, 128, 256}: forward sweep, LayerNorm passes, dQ
sweep, dK/dV sweep) restated in float64 from the contract in include/maskunet_hip.h, a numpy model of the roundings the kernels make,
a per-element first-order error bound, and the case tables of tests/test_gpu_attn_edges.py.  numpy only: no torch, no GPU, nothing of
maskunet_amd.  tests/test_attn_reference_host.py pins the reference against float64 autograd, checks the bounds against the rounding
model and against today's per-tensor gate, and checks that the comparator reports a list of deliberately wrong results.

reference(inp)                the block in float64 on the kept key list, from the operand values AS STORED (fp16 values for MU_F16,
                              the decoded fp16-pair value hi + lo for the qkv of MU_F32X).  The backward half takes the saved forward
                              results (oattn, lse2, mean, rstd) as INPUTS, exactly like the entry point: the tests hand the kernel the
                              reference's forward results rounded to their storage types, and the reference backward is computed from
                              those rounded values, so the backward bounds hold no forward error.
model(inp)                    the same in float32 numpy with the kernels' roundings (see its docstring for the lines).
bounds(inp, ref)              one bound per compared element (see its docstring for the derivation).

No constant here was chosen by looking at GPU output.
"""
import math
import os
import re

import numpy as np

U = 2.0 ** -24            # half an ulp of fp32, relative
H = 2.0 ** -11            # half an ulp of fp16, relative
F = 2.0 ** -25            # half the fp16 subnormal quantum: the absolute rounding error of an fp16 value below 2^-14
PAIR = 2.0 ** -22         # hi + lo of an fp16 pair: |x - hi| <= 2^-11 |x|, |(x - hi) - lo| <= 2^-11 |x - hi| (+ F where lo is subnormal)
BF_PAIR = 2.0 ** -16      # the same for the bf16 pair of MU_ATTN_DQKV_ENCODED (8 significant bits each)
EXP2 = 2.0 * U            # v_exp_f32: ASSUMED within 1 ulp (the CDNA ISA manual's figure for the transcendental unit)
RSQRT = 4.0 * U           # rsqrtf: ASSUMED within 2 ulp (OpenCL's bound, which OCML implements)
LOG2 = 4.0 * U            # log2f: ASSUMED within 2 ulp
F32_FLUSH = 2.0 ** -126
EPS = 1e-5
LOG2E = 1.4426950408889634
DTYPES = ("f16", "f32", "f32x")
WIDTHS = (32, 64, 128, 256)
TOL = {"f16": 3e-2, "f32": 1e-3, "f32x": 1e-3}          # tests/_gpu_checks.TOL: today's per-tensor gate (error over tensor max)
FWD_KEYS = ("out", "oattn", "lse2", "mean", "rstd")
BWD_KEYS = ("dY", "delta", "dqkv", "dgamma", "dbeta")
QBLOCK, DKV_QT = 128, 32                                 # queries per forward / dQ block; query tile of the dK/dV ring
LN_MAXBLK = 1024                                          # ATT_LN_MAXBLK


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def r16(a):
    """fp32 -> fp16 -> back (round to nearest even, as a device conversion)"""
    return f32(a).astype(np.float16).astype(np.float32)


def pair(a):
    """mu_hsplit8 (common.h): hi = fp16(x), lo = fp16(x - hi), both as float32"""
    a = f32(a)
    hi = r16(a)
    return hi, r16(a - hi)


def encode_h(a):
    """mu_split_encode_h on the host: [.., 8k] float32 -> the same shape, every aligned group of eight holding [8 fp16 hi | 8 fp16 lo]"""
    a = f32(a)
    hi, lo = pair(a)
    g = np.concatenate([hi.reshape(-1, 8).astype(np.float16), lo.reshape(-1, 8).astype(np.float16)], axis=1)
    return np.ascontiguousarray(g).view(np.float32).reshape(a.shape)


def decode_bf(a):
    """the chunk encoding of MU_ATTN_DQKV_ENCODED (common.h mu_enc4: [4 bf16 hi | 4 bf16 lo] per 16 bytes) -> float64 values"""
    w = np.ascontiguousarray(f32(a)).view(np.uint16).reshape(-1, 8).astype(np.uint32) << 16
    v = w.view(np.float32).astype(np.float64)
    return (v[:, :4] + v[:, 4:]).reshape(np.shape(a))


def encode_bf(a):
    """mu_enc4 on the host (the test of decode_bf, and the model of MU_ATTN_DQKV_ENCODED): bf16 hi = round(x), lo = round(x - hi)"""
    def bf(x):
        w = np.ascontiguousarray(f32(x)).view(np.uint32)
        w = (w + 0x7FFF + ((w >> 16) & 1)) >> 16
        return w.astype(np.uint16)
    a = f32(a)
    hi = bf(a)
    lo = bf(a - (hi.astype(np.uint32) << 16).view(np.float32))
    g = np.concatenate([hi.reshape(-1, 4), lo.reshape(-1, 4)], axis=1)
    return np.ascontiguousarray(g).view(np.float32).reshape(a.shape)


def stored(a, dt):
    """values -> (what the reference reads, float64; what the device buffer holds)"""
    if dt == "f16":
        s = f32(a).astype(np.float16)
        return f64(s), s
    return f64(f32(a)), f32(a)


def stored_qkv(a, dt):
    if dt != "f32x":
        return stored(a, dt)
    hi, lo = pair(a)
    return f64(hi) + f64(lo), encode_h(a)


# ================================================================================================
# tile constants: read from AttnTiles<T, D> in attn.hip, asserted against this copy (a retuned tile fails loudly)
# ================================================================================================
TILE_LINES = {   # name: (the right-hand side in AttnTiles, asserted verbatim; the same in Python, xf = fp32x, esz = sizeof(T))
    "FWD_KT": ("(D >= 128 || (XF && D == 64)) ? 32 : 64", lambda D, xf, esz: 32 if (D >= 128 or (xf and D == 64)) else 64),
    "DQ_KT": ("D == 32 ? 64 : 32", lambda D, xf, esz: 64 if D == 32 else 32),
    "NKT": ("D <= 64 ? 2 : 1", lambda D, xf, esz: 2 if D <= 64 else 1),
    "NWK": ("D != 128 ? 4 : (sizeof(T) == 2 ? 12 : (XF ? 8 : 4))", lambda D, xf, esz: 4 if D != 128 else (12 if esz == 2 else (8 if xf else 4))),
}
TILE_TABLE = {   # (dtype, D): FWD_KT, DQ_KT, keys per dK/dV block (16 * NWK * NKT), ring depth
    ("f16", 32): (64, 64, 128, 4), ("f16", 64): (64, 32, 128, 4), ("f16", 128): (32, 32, 192, 4), ("f16", 256): (32, 32, 64, 4),
    ("f32", 32): (64, 64, 128, 4), ("f32", 64): (64, 32, 128, 4), ("f32", 128): (32, 32, 64, 4), ("f32", 256): (32, 32, 64, 2),
    ("f32x", 32): (64, 64, 128, 4), ("f32x", 64): (32, 32, 128, 4), ("f32x", 128): (32, 32, 128, 4), ("f32x", 256): (32, 32, 64, 2),
}
ATTN_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "maskunet_amd", "csrc", "attn.hip")


def tiles_from_source(dt, D, text=None):
    """FWD_KT, DQ_KT, keys per dK/dV block and ring depth of (dt, D) from the text of attn.hip"""
    text = open(ATTN_HIP).read() if text is None else text
    v = {}
    for name, (want, fn) in TILE_LINES.items():
        m = re.search(r"static constexpr int " + name + r" = ([^;]*);", text)
        assert m and m.group(1).strip() == want, (name, m and m.group(1))
        v[name] = fn(D, dt == "f32x", 2 if dt == "f16" else 4)
    for line in ("DKV_RING = (STG * (int)sizeof(T) <= 36864) ? 4 : 2", "constexpr int STG = 2 * TEQ", "constexpr int TEQ = Z::TE(QT);",
                 "NDT = D / 16, QT = 32;", "static constexpr int RPW = 1024 / ROWB;", "TE(int rows) { return rows * D; }",
                 "static constexpr int ROWB = D * 4, CPR = ROWB / 16, RPW = 1024 / ROWB;", "static constexpr int S = 2 * RPW;",
                 "static constexpr int BLK = (1024 + 16 * (S % 16)) / 4;", "TE(int rows) { return (rows / RPW) * BLK; }"):
        assert line in text, ("the ring slot's size formula changed", line)      # every line the slot size below restates
    esz = 2 if dt == "f16" else 4
    slot = 2 * 32 * D * esz if dt != "f32x" else 2 * (32 // (1024 // (D * 4))) * (1024 + 16 * ((2 * (1024 // (D * 4))) % 16))
    return v["FWD_KT"], v["DQ_KT"], 16 * v["NWK"] * v["NKT"], 4 if slot <= 36864 else 2


def mfma_adds(n, dt, per_step=1):
    """Additions a term of an n-term sum passes through when the sum runs on the matrix core (see bounds): K inside its own
    instruction (K = 32: v_mfma_f32_16x16x32_f16, fp16 and fp32x; K = 4: v_mfma_f32_16x16x4_f32, plus the rounding of the fp32 product
    itself), then one per later instruction of the chain, per_step instructions for every K terms"""
    K = 4 if dt == "f32" else 32
    return K + (1 if dt == "f32" else 0) + per_step * -(-int(n) // K)


def pshift_of(N):
    """attn_pshift (attn.hip:1532): floor(log2 N) - 2 clamped to 0..12"""
    return float(min(12, max(0, int(math.floor(math.log2(N))) - 2)))


def ln_row_blocks(rows, cap=LN_MAXBLK):
    """attn_row_blocks (attn.hip:1460)"""
    return int(min(cap, max(1, rows // 64)))


# ================================================================================================
# float64 reference
# ================================================================================================
def _ln_fwd(o, x, gamma, beta, cv):
    y = (o + x)[:, :cv]
    mean = y.mean(1)
    d = y - mean[:, None]
    rstd = 1.0 / np.sqrt((d * d).mean(1) + EPS)
    out = np.zeros_like(o)
    out[:, :cv] = d * rstd[:, None] * gamma[:cv] + beta[:cv]
    return out, mean, rstd


def reference_fwd(inp):
    """out, oattn [B, N, C], lse2, mean, rstd [B, N] in float64, and per image the kept scores (log2 units) and probabilities"""
    B, N, C, cv = inp["B"], inp["N"], inp["C"], inp["cv"]
    sl2 = LOG2E / math.sqrt(cv)
    r = {k: np.zeros((B, N, C)) for k in ("out", "oattn")}
    r.update({k: np.zeros((B, N)) for k in ("lse2", "mean", "rstd")})
    r["S2"], r["P"] = [], []
    for b in range(B):
        kk = inp["kidx"][b, :inp["kcnt"][b]].astype(np.int64)
        q, k, v = (inp["qkv"][b][:, i * C:(i + 1) * C] for i in range(3))
        s2 = (q @ k[kk].T) * sl2
        m = s2.max(1, keepdims=True)
        e = np.exp2(s2 - m)
        l = e.sum(1, keepdims=True)
        p = e / l
        r["S2"].append(s2)
        r["P"].append(p)
        r["oattn"][b] = p @ v[kk]
        r["lse2"][b] = (m + np.log2(l))[:, 0]
        r["out"][b], r["mean"][b], r["rstd"][b] = _ln_fwd(r["oattn"][b], inp["x"][b], inp["gamma"], inp["beta"], cv)
    return r


def reference_bwd(inp, saved):
    """dY [B, N, C], delta [B, N], dqkv [B, N, 3C], dgamma, dbeta [C] in float64 from gout and the SAVED oattn / lse2 / mean / rstd (the
    values the entry point is handed, float64 copies of what the buffers hold); per image Pb = 2^(s2 - lse2) and dpp = dP - delta"""
    B, N, C, cv = inp["B"], inp["N"], inp["C"], inp["cv"]
    scale, sl2 = 1.0 / math.sqrt(cv), LOG2E / math.sqrt(cv)
    r = {"dY": np.zeros((B, N, C)), "delta": np.zeros((B, N)), "dqkv": np.zeros((B, N, 3 * C)), "dgamma": np.zeros(C), "dbeta": np.zeros(C),
         "Pb": [], "dpp": [], "xh": np.zeros((B, N, C)), "gg": np.zeros((B, N, C))}
    g = inp["gamma"]
    for b in range(B):
        o, x, go = saved["oattn"][b], inp["x"][b], inp["gout"][b]
        mu, rs = saved["mean"][b][:, None], saved["rstd"][b][:, None]
        xh = np.zeros((N, C))
        xh[:, :cv] = ((o + x)[:, :cv] - mu) * rs
        gg = go * g
        gg[:, cv:] = 0
        a, bs = gg[:, :cv].mean(1, keepdims=True), (gg * xh)[:, :cv].mean(1, keepdims=True)
        dY = rs * (gg - a - xh * bs)
        dY[:, cv:] = 0
        r["xh"][b], r["gg"][b] = xh, gg
        r["dY"][b] = dY
        r["delta"][b] = (dY * o).sum(1)
        r["dgamma"][:cv] += (go * xh)[:, :cv].sum(0)
        r["dbeta"][:cv] += go[:, :cv].sum(0)
        kk = inp["kidx"][b, :inp["kcnt"][b]].astype(np.int64)
        q, k, v = (inp["qkv"][b][:, i * C:(i + 1) * C] for i in range(3))
        pb = np.exp2((q @ k[kk].T) * sl2 - saved["lse2"][b][:, None])
        dpp = dY @ v[kk].T - r["delta"][b][:, None]
        ds = pb * dpp * scale
        r["Pb"].append(pb)
        r["dpp"].append(dpp)
        r["dqkv"][b][:, :C] = ds @ k[kk]
        r["dqkv"][b][kk, C:2 * C] = ds.T @ q
        r["dqkv"][b][kk, 2 * C:] = pb.T @ dY
    return r


def saved_of(ref, dt):
    """the reference's forward results as the backward's saved inputs: rounded to their storage types; (float64 values, buffers)"""
    vals, bufs = {}, {}
    vals["oattn"], bufs["oattn"] = stored(ref["oattn"], "f16" if dt == "f16" else "f32")
    for k in ("lse2", "mean", "rstd"):
        vals[k], bufs[k] = stored(ref[k], "f32")
    return vals, bufs


# ================================================================================================
# the rounding model
# ================================================================================================
def model(inp, saved, wrong=None):
    """The block in float32 numpy with the roundings of attn.hip; sums are float32 matrix products (a fixed order, not the kernels').
    `wrong` names one deliberate defect (see WRONG) -- the comparator tests' wrong kernels are this function with one line changed.

    Rounding points (attn.hip line numbers):
      * ld_scaled (79-84 fp16, 141 fp32, 205-214 fp32x): the RESIDENT operand of every sweep is scaled in fp32 and rounded to its
        operand form -- fp16 for MU_F16, an fp16 pair for MU_F32X.  Forward 565 and dQ 1030: Q * log2(e)/sqrt(cv); dQ 1031:
        dY / sqrt(cv); dK/dV 1254-1255: K * log2(e)/sqrt(cv) and V / sqrt(cv).  The streamed operand is read as stored.
      * fp32x keys / values as ONE fp16 term (231-251, 272-287): S = K_hi (Q_hi + Q_lo) in the forward and dQ (mma_row_*_sa), S = (Q_hi +
        Q_lo) K'_hi in dK/dV (_sb); dP = V_hi dY'_hi only (_bp_); dQ = dS K_hi, dK = dS^T Q_hi, dV = P^T dY'_hi (mma_accb*, 288-291).
        The forward's P V keeps both halves of V (255-258).
      * P rounded to fp16 as an MFMA operand (117-119, 252-259): forward 654-659 (fp16, fp32x), dK/dV 1335.  fp32 keeps fp32.
      * the forward's reference maximum (619-645): fp16 / fp32x first sweep with the maximum of the FIRST key tile only (668-674); a
        non-finite row sum anywhere in the 128-query block repeats the sweep with the running maximum (675-698); fp32 tracks it always.
      * dS = P * dP' (1088 dQ: fp32 product, rounded once to fp16 by mma_accb 131 / 291; 1335-1336 dK/dV: P and dP' rounded to fp16,
        then one packed fp16 multiply).
      * dY (fp32x): encoded as the fp16 pair of gs * dY with ONE power-of-two gs = 2^(-3 - floor(log2 max|dY|)) (887-895, 926-943).
      * 2^pshift (fp32x, 1531-1537): the row constant is pshift - lse2 (816, 1033); accumulators un-scaled by 1 / (gs 2^pshift) (1002,
        1123, 1268, 1400) -- exact, powers of two.
      * the LayerNorm passes (703-749, 757-849, 855-885) are fp32 throughout; outputs are rounded to the storage type on store."""
    dt, B, N, C, cv = inp["dt"], inp["B"], inp["N"], inp["C"], inp["cv"]
    wrong = wrong or ""
    PK = dt != "f32"
    fkt, dqkt, dkvb, _ = TILE_TABLE[dt, C]
    cs = C if wrong == "scale_C" else cv
    scale, sl2 = np.float32(1.0 / math.sqrt(cs)), np.float32(LOG2E / math.sqrt(cs))
    st = (lambda a: r16(a)) if dt == "f16" else f32
    gamma, beta = f32(inp["gamma"]), f32(inp["beta"])
    o = {k: np.zeros((B, N, C), np.float32) for k in ("out", "oattn", "dY")}
    o.update({k: np.zeros((B, N), np.float32) for k in ("lse2", "mean", "rstd", "delta")})
    o["dqkv"] = np.zeros((B, N, 3 * C), np.float32)
    dga, dbe = np.zeros(C), np.zeros(C)

    def operand(a, sc=None):
        """an operand of a row product as the terms the matrix core sees: (hi, lo) with lo = 0 unless fp32x"""
        a = f32(a) if sc is None else f32(a) * sc
        if dt == "f16":
            return r16(a), np.float32(0) * a
        if dt == "f32":
            return a, np.float32(0) * a
        return pair(a)                                     # (unscaled: the stored pair itself, the value IS hi + lo)

    # ---- forward ----
    for b in range(B):
        nk = int(inp["kcnt"][b])
        kk = inp["kidx"][b, :nk].astype(np.int64)
        q, k, v = (f32(inp["qkv"][b][:, i * C:(i + 1) * C]) for i in range(3))
        qh, ql = operand(q, sl2)
        kh, _ = operand(k[kk])
        vh, vl = operand(v[kk])
        if wrong == "xf_qlo":                               # (not in WRONG: the bounds cannot see it, see NOTES_r14.md "Left out")
            ql = 0 * ql
        s = qh @ kh.T + ql @ kh.T                          # (fp16 / fp32: ql = 0)
        if wrong == "mask_left":                            # the partial last tile's masked scores left in: keys re-read from the last kept row
            pad = (-nk) % fkt
            if pad:
                s = np.concatenate([s, np.repeat(s[:, -1:], pad, 1)], 1)
                vh, vl = (np.concatenate([a, np.repeat(a[-1:], pad, 0)], 0) for a in (vh, vl))
        if wrong == "last_tile" and nk > fkt:
            drop = (nk - 1) % fkt + 1
            s, vh, vl = s[:, :-drop], vh[:-drop], vl[:-drop]
        nks = s.shape[1]
        acc = np.zeros((N, C), np.float32)
        l = np.zeros((N, 1), np.float32)
        m = np.zeros((N, 1), np.float32)
        for q0 in range(0, N, QBLOCK):
            rows = slice(q0, min(N, q0 + QBLOCK))
            for exact in ((False, True) if PK else (True,)):
                a_, l_, m_ = 0, 0, None
                for j0 in range(0, nks, fkt):
                    sj = s[rows, j0:j0 + fkt]
                    if m_ is None:
                        m_ = sj.max(1, keepdims=True)
                    elif exact:
                        mn = np.maximum(m_, sj.max(1, keepdims=True))
                        if wrong != "no_rescale":
                            alpha = np.exp2(m_ - mn)
                            a_, l_ = a_ * alpha, l_ * alpha
                        m_ = mn
                    with np.errstate(over="ignore"):
                        p = np.exp2(sj - m_).astype(np.float32)
                        if PK:
                            p = r16(p)
                        l_ = l_ + p.sum(1, keepdims=True, dtype=np.float32)
                        a_ = a_ + p @ vh[j0:j0 + fkt] + p @ vl[j0:j0 + fkt]
                if exact or bool((l_ < 3.0e38).all()):
                    break
            acc[rows], l[rows], m[rows] = a_, l_, m_
        oa = acc * (np.float32(1) / l)
        o["oattn"][b] = st(oa)
        o["lse2"][b] = (m + np.log2(l))[:, 0]
        src = o["oattn"][b] if cv != C else oa               # cv < C: attn_ln_fwd_kernel re-reads the stored oattn (1476-1480)
        y = (src + f32(inp["x"][b]))[:, :cv]
        mean = y.sum(1, dtype=np.float32) / np.float32(cv)
        d = y - mean[:, None]
        rstd = np.float32(1) / np.sqrt((d * d).sum(1, dtype=np.float32) / np.float32(cv) + np.float32(EPS))
        o["out"][b][:, :cv] = st(d * rstd[:, None] * gamma[:cv] + beta[:cv])
        o["mean"][b], o["rstd"][b] = mean, rstd
    # ---- backward prepass ----
    xhs, amax = [], np.float32(0)
    for b in range(B):
        oa, x, go = f32(saved["oattn"][b]), f32(inp["x"][b]), f32(inp["gout"][b])
        mu, rs = f32(saved["mean"][b])[:, None], f32(saved["rstd"][b])[:, None]
        icv = np.float32(1.0 / (C if wrong == "icv_D" else cv))
        xh = (oa + x - mu) * rs
        gg = go * gamma
        a, bs = gg.sum(1, keepdims=True, dtype=np.float32) * icv, (gg * xh).sum(1, keepdims=True, dtype=np.float32) * icv
        dY = rs * (gg - a - xh * bs)
        dY[:, cv:] = 0
        amax = max(amax, np.abs(dY).max())
        o["dY"][b] = st(dY)
        o["delta"][b] = (o["dY"][b] * oa).sum(1, dtype=np.float32)
        dga[:cv] += f64(go * xh)[:, :cv].sum(0)
        dbe[:cv] += f64(go)[:, :cv].sum(0)
    o["dgamma"], o["dbeta"] = f32(dga), f32(dbe)
    gs = np.float32(2.0 ** (-3 - math.floor(math.log2(float(amax))))) if dt == "f32x" and amax > 0 else np.float32(1)
    psh = np.float32(pshift_of(N) if dt == "f32x" else 0)
    un = np.float32(1) / (gs * np.exp2(psh))
    # ---- the sweeps ----
    for b in range(B):
        nk = int(inp["kcnt"][b])
        kk = inp["kidx"][b, :nk].astype(np.int64)
        q, k, v = (f32(inp["qkv"][b][:, i * C:(i + 1) * C]) for i in range(3))
        dYs = o["dY"][b] * gs
        nlse = psh - f32(saved["lse2"][b])[:, None]
        dl = np.zeros_like(o["delta"][b]) if wrong == "no_delta" else o["delta"][b]
        ndel = (-dl * scale * gs)[:, None]
        # dQ (985-1128)
        qh, ql = operand(q, sl2)
        kh, _ = operand(k[kk])
        vh, _ = operand(v[kk])
        if dt == "f32x":
            dh, _ = pair(f32(sum(pair(dYs))) * scale)        # ld_scaled of the encoded dY: decode, scale, split again
        else:
            dh, _ = operand(dYs, scale)
        if wrong == "xf_qlo":
            ql = 0 * ql
        s = qh @ kh.T + ql @ kh.T + nlse
        dp = dh @ vh.T + ndel
        ds = np.exp2(s).astype(np.float32) * dp
        if PK:
            ds = r16(ds)
        o["dqkv"][b][:, :C] = st((ds @ kh) * un)
        # dK/dV (1148-1410)
        qsh, qsl = operand(q)
        kfh, _ = operand(k[kk], sl2)
        vfh, _ = operand(v[kk], scale)
        yh, _ = pair(dYs) if dt == "f32x" else operand(dYs)
        s = qsh @ kfh.T + qsl @ kfh.T + nlse
        dp = yh @ vfh.T + ndel
        p = np.exp2(s).astype(np.float32)
        if PK:
            p = r16(p)
            ds = r16(p * r16(dp))
        else:
            ds = p * dp
        if wrong == "pad_queries" and N % DKV_QT:            # padded queries of the last 32-query tile counted: row N - 1 again
            rep = DKV_QT - N % DKV_QT
            p, ds, yh, qsh = (np.concatenate([a, np.repeat(a[-1:], rep, 0)], 0) for a in (p, ds, yh, qsh))
        dk, dv = st((ds.T @ qsh) * un), st((p.T @ yh) * un)
        rows_k = np.roll(kk, 1) if wrong == "dk_neighbour" and nk > 1 else kk
        o["dqkv"][b][rows_k, C:2 * C] = dk
        o["dqkv"][b][kk, 2 * C:] = dv
    return o


WRONG = ("mask_left", "no_rescale", "last_tile", "dk_neighbour", "no_delta", "pad_queries", "scale_C", "icv_D")


# ================================================================================================
# bounds
# ================================================================================================
def bounds(inp, ref, refb, saved, encoded=False):
    """One first-order bound per element of out, oattn, lse2, mean, rstd (against reference_fwd) and of dY, delta, dqkv, dgamma, dbeta
    (against reference_bwd on the saved values): (unit roundoffs of the rounding points model() names) x (the sum of absolute terms
    of that element).  Notation: u = 2^-24, h = 2^-11, F = 2^-25 (absolute error of an fp16 value below 2^-14), pair = 2^-22.

    Scores (log2 units), s_ij = sum_c q'_ic k_jc + c_i with c_i = -m_i (forward) or pshift - lse2_i (backward).  One operand of each
    product is rounded when it is scaled (fp16: h; fp32: u; fp32x: pair), and fp32x reads the other as one fp16 term (h):
        e_s = h (fp16), 2u (fp32), h + pair + u (fp32x).
    Sums on the matrix core: one MFMA computes c + sum_{k<K} a_k b_k (K = 32 for the fp16 instruction of MU_F16 / MU_F32X, whose
    products are exact in fp32; K = 4 for the fp32 instruction, whose products are rounded: one more u).  The order inside an
    instruction is not documented, so a term is charged K additions there, and one more for every later instruction of the chain
    that carries the accumulator on: mfma_adds(n, per_step) = K [+ 1] + per_step ceil(n / K), per_step = instructions per K terms
    (fp32x: 3 in the forward's Q K^T at most, 2 in P V, 1 in the backward products; otherwise 1).
    Scores: D products, the row constant as the first C operand (+ 1), and the running-maximum updates of the forward (two subtractions
    per 32-key step at most): n_s = mfma_adds(D, 3 | 1) + 1 + 2 ceil(kcnt / 32), so
        es_ij = e_s A_ij + n_s u (A_ij + cmag_i) [+ F sum_c |k_jc| + F sum_c |q_ic| for fp32x: a subnormal lo half of the scaled operand]
    with A_ij = log2(e)/sqrt(cv) sum_c |q_ic k_jc| and cmag_i = max(max_j |S2_ij|, |lse2_i|) + pshift.
    Probabilities: p = exp2(s) is off by expm1(ln2 es) + EXP2 relatively; as an fp16 operand by another h, and below 2^-14 by F
    ABSOLUTELY in the sweep's own units.  Forward: the sweep computes 2^(s - m') with m' <= the row maximum (the first tile's maximum in
    the optimistic sweep, the running maximum in the redo), so its row sum l' >= l = sum_j 2^(S2_ij - max_j S2_ij) >= 1 and the dropped
    mass of a normalised P_ij is at most F / l_i per key -- kcnt F / l_i over a row of subnormal probabilities.  Backward: P = 2^(s -
    lse2) is in natural units (fp32x: times 2^pshift, so F 2^-pshift).
        dP_ij = P_ij (expm1(ln2 es_ij) + EXP2 + [h]) + [F / l_i  or  F 2^-pshift]            ([..]: fp16 and fp32x only)
    oattn_ic = sum_j p_j v_jc / sum_j p_j: numerator and denominator each accumulate kcnt terms (fp32x: two MFMAs per step), are
    rescaled at most once per tile (a product and an exp2 each), then 1 / l and the product: n_a = mfma_adds(kcnt, 2 | 1) + 2 ceil(kcnt / 32) + 3:
        b(oattn_ic) = sum_j dP_ij (|v_jc| + |oattn_ic|) + n_a u (sum_j P_ij |v_jc| + |oattn_ic|) + 3u |oattn_ic| + store
    With ONE kept key the first tile's exact maximum is the score itself: p = 2^0 = 1, l = 1, and oattn is the key's V row to the
    accumulation terms alone (the dP terms drop out of b(oattn); lse2 is the score and keeps them).
    store = 2h |value| + 2F for fp16 storage (ONE ulp: a correctly rounded store is off by up to half of it, and the rounding model has
    to stay within half of every bound; what a later stage inherits from a stored dY is the half ulp), 0 otherwise.  lse2 = m + log2(l): b = (sum_j dP_ij + n_a u) / ln2 + (LOG2 + 4u)(cmag_i + 1).
    LayerNorm forward (a row's sums pass through n_l = D / 4 + 4 additions; rsqrtf RSQRT): with dy_c = b(oattn_ic) + u |y_c|,
        b(mean) = mean_c dy_c + (n_l + 1) u mean_c |y_c|;  dd_c = dy_c + b(mean) + u |d_c|  (d = y - mean)
        b(rstd) = rstd^3 mean_c(|d_c| dd_c) + ((n_l + 3) u / 2 + RSQRT + 2u) rstd
        b(out_c) = |gamma_c| (rstd dd_c + |d_c| b(rstd)) + 4u (|d_c rstd gamma_c| + |beta_c|) + store.
    LayerNorm backward (inputs exact; n_r = 14 additions per row sum): with xh = (o + x - mean) rstd, gg = g gamma, a = mean gg,
    bs = mean gg xh,
        dxh = u (|o + x| + 2 |o + x - mean|) rstd,  da = (n_r + 1) u mean|gg|,  dbs = mean(|gg| dxh) + (n_r + 2) u mean|gg xh|
        b(dY_c) = rstd (u |gg| + da + dxh |bs| + |xh| dbs + 4u (|gg| + |a| + |xh bs|)) + u |dY_c| + store
        b(delta) = sum_c b(dY_c) |o_c| + n_r u sum_c |dY_c o_c|   (fp16 storage: twice that as the compared bound, see store)
        b(dgamma_c) = sum_r |g| dxh + 40u sum_r |g xh|, b(dbeta_c) = 40u sum_r |g|  (a block adds at most 33 rows per lane in fp32; fp64 after).
    dP'_ij = (sum_c dY_ic v_jc - delta_i) / sqrt(cv): operand roundings e_d = h (fp16: the scaled operand), 3u (fp32), 2h + pair (fp32x:
    both operands as one fp16 term), on B_ij = sum_c |dY_ic v_jc| / sqrt(cv); the error of dY and delta themselves; subnormal scaled
    operands F sum_c |v_jc| + F sum_c |dY_ic| (fp32x: the first over gs >= 1 / (8 max|dY|)):
        ddp_ij = e_d B_ij + (sum_c b(dY_ic) |v_jc| + b(delta_i)) / sqrt(cv) + n_s u (B_ij + |delta_i| / sqrt(cv)) + floors
    dS_ij = P_ij dP'_ij: b = dP_ij |dP'_ij| (without P's own h: it is one of the 3h) + P_ij ddp_ij + 3h |dS_ij| + F g (1 + P_ij)  (fp16 / fp32x, g = 1 or 8 max|dY| 2^-pshift ... );
    2u |dS_ij| for fp32.  Then
        b(dQ_ic) = sum_j b(dS_ij) |k_jc| + (e_k + n_a u) sum_j |dS_ij k_jc| + store         e_k = h for fp32x (K_hi only), else 0
        b(dK_jc) = sum_i b(dS_ij) |q_ic| + (e_k + n_q u) sum_i |dS_ij q_ic| + store         n_q = mfma_adds(N) + 1
        b(dV_jc) = sum_i (dP_ij |dY_ic| + P_ij b(dY_ic)) + (e_k + n_q u) sum_i P_ij |dY_ic| + store
    MU_ATTN_DQKV_ENCODED adds the bf16 pair's own rounding, 2^-16 (|value| + bound).  Rows of masked keys and pad channels: bound 0."""
    dt, B, N, C, cv = inp["dt"], inp["B"], inp["N"], inp["C"], inp["cv"]
    PK = dt != "f32"
    scale, sl2 = 1.0 / math.sqrt(cv), LOG2E / math.sqrt(cv)
    e_s = {"f16": H, "f32": 2 * U, "f32x": H + PAIR + U}[dt]
    e_d = {"f16": H, "f32": 3 * U, "f32x": 2 * H + PAIR}[dt]
    e_k = H if dt == "f32x" else 0.0
    psh = pshift_of(N) if dt == "f32x" else 0.0
    store = (lambda a: 2 * H * np.abs(a) + 2 * F) if dt == "f16" else (lambda a: F32_FLUSH + 0 * np.abs(a))
    g = np.abs(inp["gamma"])
    bd = {k: np.zeros((B, N, C)) for k in ("out", "oattn", "dY")}
    bd.update({k: np.zeros((B, N)) for k in ("lse2", "mean", "rstd", "delta")})
    bd["dqkv"] = np.zeros((B, N, 3 * C))
    bd["dgamma"], bd["dbeta"] = np.zeros(C), np.zeros(C)
    n_l, n_r = C / 4 + 4, 14
    amax = max(float(np.abs(refb["dY"]).max()), 1e-300)
    gfl = 16 * amax if dt == "f32x" else 1.0                  # 1 / gs <= 8 max|dY|; max|dY| itself known to a factor < 2 here
    for b in range(B):
        nk = int(inp["kcnt"][b])
        kk = inp["kidx"][b, :nk].astype(np.int64)
        q, k, v = (np.abs(inp["qkv"][b][:, i * C:(i + 1) * C]) for i in range(3))
        k, v = k[kk], v[kk]
        nt = -(-nk // 32)
        n_s = mfma_adds(C, dt, 3 if dt == "f32x" else 1) + 1 + 2 * nt
        n_a = mfma_adds(nk, dt, 2 if dt == "f32x" else 1) + 2 * nt + 3
        n_q = mfma_adds(N, dt) + 1
        A = (q @ k.T) * sl2
        cmag = np.maximum(np.abs(ref["S2"][b]).max(1), np.abs(saved["lse2"][b])) + psh
        es = e_s * A + n_s * U * (A + cmag[:, None])
        if dt == "f32x":
            es = es + F * k.sum(1)[None, :] + F * q.sum(1)[:, None]
        relp0 = np.expm1(math.log(2) * es) + EXP2             # p = exp2(s) in fp32
        relp = relp0 + (H if PK else 0.0)                     # ... as an fp16 operand
        # forward
        P, oa = ref["P"][b], np.abs(ref["oattn"][b])
        s2 = ref["S2"][b]
        l = np.exp2(s2 - s2.max(1, keepdims=True)).sum(1)
        dP = P * relp + ((F / l)[:, None] if PK else 0.0)
        dPo = dP * (nk > 1)                                   # one kept key: p = 2^(s - s) = 1 and l = 1 exactly, oattn is the key's V row
        b_o = dPo @ v + dPo.sum(1)[:, None] * oa + n_a * U * (P @ v + oa) + 3 * U * oa
        bd["oattn"][b] = b_o + store(oa)
        bd["lse2"][b] = (dP.sum(1) + n_a * U) / math.log(2) + (LOG2 + 4 * U) * (cmag + 1)
        y = (ref["oattn"][b] + inp["x"][b])[:, :cv]
        mean, rstd = ref["mean"][b], ref["rstd"][b]
        d = np.abs(y - mean[:, None])
        dy = bd["oattn"][b][:, :cv] + U * np.abs(y)
        b_mean = dy.mean(1) + (n_l + 1) * U * np.abs(y).mean(1)
        dd = dy + b_mean[:, None] + U * d
        b_rstd = rstd ** 3 * (d * dd).mean(1) + ((n_l + 3) * U / 2 + RSQRT + 2 * U) * rstd
        t = d * rstd[:, None] * g[:cv]
        bd["out"][b][:, :cv] = g[:cv] * (rstd[:, None] * dd + d * b_rstd[:, None]) + 4 * U * (t + np.abs(inp["beta"][:cv])) + store(ref["out"][b][:, :cv])
        bd["mean"][b], bd["rstd"][b] = b_mean, b_rstd
        # LayerNorm backward
        o_in, x = saved["oattn"][b], inp["x"][b]
        mu, rs = saved["mean"][b][:, None], saved["rstd"][b][:, None]
        xh, gg, go = np.abs(refb["xh"][b]), np.abs(refb["gg"][b]), np.abs(inp["gout"][b])
        dxh = np.zeros((N, C))
        dxh[:, :cv] = U * (np.abs(o_in + x) + 2 * np.abs(o_in + x - mu))[:, :cv] * rs
        a_, bs_ = np.abs(refb["gg"][b][:, :cv].mean(1, keepdims=True)), np.abs((refb["gg"][b] * refb["xh"][b])[:, :cv].mean(1, keepdims=True))
        da = (n_r + 1) * U * gg[:, :cv].mean(1, keepdims=True)
        dbs = (gg * dxh)[:, :cv].mean(1, keepdims=True) + (n_r + 2) * U * (gg * xh)[:, :cv].mean(1, keepdims=True)
        dYa = np.abs(refb["dY"][b])
        b_dY = rs * (U * gg + da + dxh * bs_ + xh * dbs + 4 * U * (gg + a_ + xh * bs_)) + U * dYa
        b_dY[:, cv:] = 0
        bd["dY"][b] = b_dY + store(dYa) * (b_dY > 0)
        b_dY = b_dY + store(dYa) / 2 * (b_dY > 0)             # what the sweeps inherit: the store's own half ulp
        b_delta = (b_dY * np.abs(o_in)).sum(1) + n_r * U * (dYa * np.abs(o_in)).sum(1)
        bd["delta"][b] = b_delta * (2 if dt == "f16" else 1)   # compared: the stored dY's ulp in full, like dY itself
        bd["dgamma"] += (go * dxh).sum(0) + 40 * U * (go * xh).sum(0)
        bd["dbeta"][:cv] += 40 * U * go[:, :cv].sum(0)
        # the sweeps
        Pb, dpp = refb["Pb"][b], np.abs(refb["dpp"][b]) * scale
        dPb = Pb * relp + (F * 2.0 ** -psh if PK else 0.0)
        Bm = (dYa @ v.T) * scale
        dl = np.abs(refb["delta"][b])[:, None] * scale
        ddp = e_d * Bm + ((b_dY @ v.T) + b_delta[:, None]) * scale + n_s * U * (Bm + dl)
        if PK:
            ddp = ddp + F * gfl * v.sum(1)[None, :] + F * dYa.sum(1)[:, None]
        dS = Pb * dpp
        # (the 3h of dS are the fp16 roundings of P, dP' and their product in dK/dV, of the one product in dQ: P's is not counted twice)
        b_dS = (Pb * relp0 + (F * 2.0 ** -psh if PK else 0.0)) * dpp + Pb * ddp + ((3 * H * dS + F * gfl * 2.0 ** -psh * (1 + Pb)) if PK else 2 * U * dS)
        ref_q = np.abs(refb["dqkv"][b])
        bd["dqkv"][b][:, :C] = b_dS @ k + (e_k + n_a * U) * (dS @ k) + store(ref_q[:, :C])
        bd["dqkv"][b][kk, C:2 * C] = b_dS.T @ q + (e_k + n_q * U) * (dS.T @ q) + store(ref_q[kk, C:2 * C])
        bd["dqkv"][b][kk, 2 * C:] = dPb.T @ dYa + Pb.T @ b_dY + (e_k + n_q * U) * (Pb.T @ dYa) + store(ref_q[kk, 2 * C:])
        if cv < C:
            for i in range(3):
                bd["dqkv"][b][:, i * C + cv:(i + 1) * C] = 0
            bd["oattn"][b][:, cv:] = 0
    bd["dgamma"][cv:] = 0
    if encoded:
        bd["dqkv"] = bd["dqkv"] + BF_PAIR * (np.abs(refb["dqkv"]) + bd["dqkv"])
    return bd


CV1_ZERO = ("dY", "delta", "dqkv", "dgamma")             # c_valid = 1: xhat = 0 and g gamma - mean(g gamma) = 0, these are zero but for rounding


def gate_factor(case, name):
    """How far a derived worst-case bound of a Gaussian case may stand above TOL x tensor max (the tensors are the entry points':
    dqkv is one), with the reason; None: the tensor has no maximum to be relative to.
      * dqkv, dgamma, dbeta hold sums of one rounded term per query (the dK / dV rows, the channel sums): a worst-case bound grows as
        N times a term, the tensor's maximum as sqrt(N) times a term.  The plain gate is asked of sums up to one 32-query tile of the
        dK/dV sweep; above, sqrt(N / 32).
      * c_valid = 1: a LayerNorm over one channel.  y - mean is exactly 0 in the kernel, which a first-order bound cannot know, and
        rstd = 1 / sqrt(eps) multiplies it: out is the constant beta, and dY, delta, dqkv and dgamma are analytically zero (CV1_ZERO).
        None for these and for rstd; the host file asserts that the reference holds beta and rounding noise only."""
    if case["cv"] == 1 and name in CV1_ZERO + ("out", "rstd"):
        return None
    if name in ("dqkv", "dgamma", "dbeta") and case["N"] > DKV_QT:
        return math.sqrt(case["N"] / float(DKV_QT))
    return 1.0


def gate_err(got, ref):
    """today's per-tensor figure (tests/_gpu_checks._rel_err): max error over the tensor's max"""
    return float(np.abs(f64(got) - f64(ref)).max() / max(float(np.abs(ref).max()), 1e-300))


def worst(got, ref, bound):
    """(the worst err / bound, its flat index); a NaN or an error against a zero bound is inf"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isnan(got) | np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i


# ================================================================================================
# inputs and case tables
# ================================================================================================
def rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def key_lists(N, kcnts, form, gen):
    """kidx [B, nkmax], kcnt [B]: form 'compact' -- the kept keys in ascending order, nkmax = max kcnt, padded with an in-range index;
    'perm' -- whole permutations, kept keys first, then the masked keys, both ascending (MU_ATTN_KIDX_PERMUTATION)"""
    B = len(kcnts)
    nkmax = N if form == "perm" else max(kcnts)
    kidx = np.zeros((B, nkmax), np.int32)
    for b, n in enumerate(kcnts):
        kept = np.sort(gen.permutation(N)[:n])
        if form == "perm":
            kidx[b] = np.concatenate([kept, np.setdiff1d(np.arange(N), kept)])
        else:
            kidx[b, :n] = kept
            kidx[b, n:] = kept[-1]
    return kidx, np.asarray(kcnts, np.int32)


def make_inputs(case):
    """A case -> the stored operand values (float64) and the device buffers.  Pad channels (c >= cv) of qkv, x, gout are zero.
    Regimes (`regime`; each asserted by regime_reached):
      normal    Gaussian q, k (0.5, the magnitudes of tests/_gpu_checks.check_attention), v, x, gout (1.0)
      hot:J     key position J of every image's kept list scores >= 17 log2 units above the first tile's maximum for the first query
                block's rows (the optimistic sweep overflows fp16 and the block redoes it)
      near:J    the same with 14 .. 15.9: no redo, P near the top of fp16
      flat      one dominant key in the first tile, every other probability below 2^-14 of it (fp16 subnormal P)
      rising    every score of the first tile negative and the tile maxima rising from tile to tile
      ln        |x| ~ 300 with attention outputs ~ 1e-2: the LayerNorm terms"""
    dt, B, N, C, cv = case["dt"], len(case["kcnt"]), case["N"], case["C"], case["cv"]
    gen = rng(case["seed"], N, C, cv)
    regime = case.get("regime", "normal")
    fkt = TILE_TABLE[dt, C][0]
    kidx, kcnt = key_lists(N, case["kcnt"], case["form"], gen)
    q, k, v = (gen.standard_normal((B, N, C)) * s for s in (0.5, 0.5, 1.0))
    x, gout = gen.standard_normal((B, N, C)), gen.standard_normal((B, N, C))
    root = math.sqrt(cv)
    if regime != "normal":
        u = np.zeros(C)
        u[:cv] = gen.choice([-1.0, 1.0], cv)                 # a +-1 direction: q = a u + noise, k_j = t_j u / cv + noise gives s2 ~ a t_j log2e / sqrt(cv)
        q = 0.05 * q + u * 2.0
        k = 0.05 * k
        for b in range(B):
            n = int(kcnt[b])
            t = np.zeros(n)                                  # target score (log2 units) of each kept key
            if regime.startswith(("hot", "near")):
                j = min(int(regime.split(":")[1]), n - 1)
                t[j] = 18.5 if regime.startswith("hot") else 15.0
            elif regime == "flat":
                t[:] = -17.0
                t[0] = 0.0
            elif regime == "rising":
                t[:] = -6.0 + 3.0 * (np.arange(n) // fkt) + 0.01 * (np.arange(n) % fkt)
            k[b, kidx[b, :n]] += (t * root / (LOG2E * 2.0 * cv))[:, None] * u
    if regime == "ln":
        x, v = 300.0 * x, 0.01 * v
    for a in (q, k, v, x, gout):
        a[..., cv:] = 0
    qkv, qkv_buf = stored_qkv(np.concatenate([q, k, v], axis=2), dt)
    inp = dict(dt=dt, B=B, N=N, C=C, cv=cv, kidx=kidx, kcnt=kcnt, nkmax=kidx.shape[1], form=case["form"], regime=regime, qkv=qkv)
    bufs = {"qkv": qkv_buf}
    sdt = "f16" if dt == "f16" else "f32"
    for name, a in (("x", x), ("gout", gout)):
        inp[name], bufs[name] = stored(a, sdt)
    gamma = 1.0 + 0.1 * gen.standard_normal(C)
    beta = 0.1 * gen.standard_normal(C)
    for name, a in (("gamma", gamma), ("beta", beta)):
        inp[name], bufs[name] = stored(a, "f32")
    return inp, bufs


def regime_reached(inp, ref):
    """the float64 reference shows that the case is in the regime its name claims"""
    regime, dt, C = inp["regime"], inp["dt"], inp["C"]
    fkt = TILE_TABLE[dt, C][0]
    for b in range(inp["B"]):
        s2, n = ref["S2"][b], int(inp["kcnt"][b])
        m1 = s2[:, :fkt].max(1)
        over = s2.max(1) - m1
        if regime.startswith("hot") and n > fkt and int(regime.split(":")[1]) >= fkt:
            assert over.min() > 16.5, (regime, b, over.min())
        elif regime.startswith("near") and n > fkt and int(regime.split(":")[1]) >= fkt:
            assert 14.0 < over.min() and over.max() < 15.9, (regime, b, over.min(), over.max())
        elif regime == "flat" and n > 1:
            rest = np.sort(s2 - s2.max(1, keepdims=True), axis=1)[:, -2]
            assert rest.max() < -14.5 and rest.min() > -24.0, (regime, b, rest.max(), rest.min())
        elif regime == "rising":
            assert s2[:, :fkt].max() < 0, (regime, b)
            tm = np.stack([s2[:, j:j + fkt].max(1) for j in range(0, n, fkt)], 1)
            assert (np.diff(tm, axis=1) > 0).all(), (regime, b)
        elif regime == "ln":
            assert np.abs(inp["x"]).max() > 500 and np.abs(ref["oattn"]).max() < 0.1
        if n == 1:                                           # (f) one kept key: oattn is that key's V row
            kk = int(inp["kidx"][b, 0])
            assert np.array_equal(ref["oattn"][b], np.broadcast_to(inp["qkv"][b][kk, 2 * C:], ref["oattn"][b].shape))
    return True


def edge_counts(kt):
    return [1, kt - 1, kt, kt + 1, 2 * kt - 1, 2 * kt, 2 * kt + 1, 3 * kt + 1, 4 * kt]


def _case(dt, C, N, kcnt, form="compact", cv=None, regime="normal", seed=0, fwd_only=False, flags=0):
    kcnt = tuple(min(int(n), N) for n in kcnt)
    # `normal`: the Gaussian cases, the ones today's per-tensor gate is compared with (see gate_factor for the two derived exceptions)
    normal = regime == "normal"
    return dict(dt=dt, C=C, cv=cv or C, N=N, kcnt=kcnt, form=form, regime=regime, seed=seed, fwd_only=fwd_only, flags=flags, normal=normal,
                name=f"{dt} C={C} cv={cv or C} N={N} kcnt={kcnt} {form} {regime}" + (" enc" if flags & 16 else ""))


def cases(dt, C, sweep):
    """The cases of one (dtype, width, sweep); sweep in 'fwd', 'dq', 'dkv', 'ln'.  Every backward N is a multiple of 4, every kcnt >= 1.
    Ragged batches of three images carry three edge values at once (the smallest shapes that reach each edge: see the module text of
    tests/test_gpu_attn_edges.py)."""
    fkt, dqkt, blk, ring = TILE_TABLE[dt, C]
    out = []
    if sweep in ("fwd", "dq"):
        kt = fkt if sweep == "fwd" else dqkt
        ec = edge_counts(kt)
        N = 4 * kt + 4
        for i in range(0, 9, 3):                             # key-tile edges, ragged B = 3, compact list
            out.append(_case(dt, C, N, ec[i:i + 3], seed=i))
        out.append(_case(dt, C, N, (1, 2 * kt + 1, N), form="perm", seed=11))
        for n in (4, 12, 20, 36, 128, 132, 260):             # query tails
            out.append(_case(dt, C, n, (1, max(1, n // 2 + 1), n), form="perm" if n % 8 == 4 else "compact", seed=n))
        if sweep == "fwd":
            for n in (5, 17):
                out.append(_case(dt, C, n, (1, n - 1, n), seed=n, fwd_only=True))
            for reg in ("hot", "near"):                      # (b), (c): buffer 1, a later full tile, the partial last tile (fp32 has no
                out.append(_case(dt, C, 4 * kt + 4, (kt + 3, 3 * kt, 3 * kt + 5), regime=f"{reg}:{kt + 1}", seed=21))      # optimistic sweep:
                out.append(_case(dt, C, 4 * kt + 4, (2 * kt + 9, 3 * kt, 4 * kt + 4), regime=f"{reg}:{2 * kt + 2}", seed=22))  # there the same
                out.append(_case(dt, C, 4 * kt + 4, (3 * kt + 5,), regime=f"{reg}:{3 * kt + 2}", seed=23))                 # scores move the running maximum)
            out.append(_case(dt, C, 4 * kt + 4, (1, 2 * kt + 1, 4 * kt + 4), regime="flat", seed=24))
            out.append(_case(dt, C, 4 * kt + 4, (kt + 1, 3 * kt + 1, 4 * kt + 4), regime="rising", seed=25))
    elif sweep == "dkv":
        for i, n in enumerate((32, 36, 64, 96, 128, 160, 164, 288, 292)):      # 1 .. 10 query tiles against the ring
            form = "perm" if i % 2 else "compact"
            out.append(_case(dt, C, n, (1, max(1, min(n, 17 if i % 2 else 31)), n), form=form, seed=n))
        N = 2 * blk + 4
        out.append(_case(dt, C, N, (blk - 1, blk, blk + 1), seed=31))
        out.append(_case(dt, C, N, (1, 2 * blk + 1, blk + 15), form="perm", seed=32))
        if dt == "f32x":
            out.append(_case(dt, C, 164, (1, 81, 164), form="perm", seed=33, flags=16))
    elif sweep == "ln":
        for cv, Cc in ((1, 32), (31, 32), (33, 64), (200, 256)):
            if Cc == C:
                out.append(_case(dt, C, 36, (1, 19, 36), form="perm", cv=cv, seed=cv))
        for rows in (4, 63, 64, 65, 127, 64 * 3 + 5):       # attn_ln_fwd_kernel (cv < C only): one image of `rows` tokens; N % 4 != 0 is forward only
            out.append(_case(dt, C, rows, (min(rows, 9),), seed=rows, fwd_only=bool(rows % 4), cv=C - 1))
        for rows in (60, 68, 124, 128, 196):                 # the backward prepass: the multiples of 4 next to the same edges
            out.append(_case(dt, C, rows, (min(rows, 9),), seed=rows))
        out.append(_case(dt, C, 36, (1, 19, 36), regime="ln", seed=41))
        if C == 32:
            out.append(_case(dt, C, 16388, (1, 5, 8, 8), seed=42))
    return out


SWEEPS = ("fwd", "dq", "dkv", "ln")


def prepare(case):
    """inputs, buffers, the float64 reference of both halves and the bounds of one case"""
    inp, bufs = make_inputs(case)
    ref = reference_fwd(inp)
    saved, saved_bufs = saved_of(ref, inp["dt"])
    refb = reference_bwd(inp, saved)
    bd = bounds(inp, ref, refb, saved, encoded=bool(case["flags"] & 16))
    return dict(case=case, inp=inp, bufs=bufs, ref=ref, saved=saved, saved_bufs=saved_bufs, refb=refb, bd=bd)
