"""Plain float64 restatements of the six row kernels of maskunet_amd/csrc/attn_wide.hip (gather, scatter, masked row softmax, dS,
LayerNorm over rows forward / backward) exactly as that file's header comments define them, and of the whole generic attention block
(ops._WideMaskAttention) with every gradient in closed form.  numpy only: no torch, no GPU, nothing of maskunet_amd.
tests/test_attn_wide_reference_host.py pins every function against float64 torch autograd and checks that the bounds have teeth
before tests/test_gpu_attn_wide_edges.py relies on them.

Every value function takes the operand values as stored (already rounded to the storage type under test) and returns its result
together with a per-element error bound.  A bound is the sum of the roundings the kernel's own operation order incurs, each times the
magnitude it rounds; the docstrings walk through the kernel so the sum can be redone with attn_wide.hip beside it.

  u = 2^-24   half an ulp of fp32, relative: one rounding of +, -, *, fmaf
  h = 2^-11   the same for fp16: the output rounding of fp16 storage, plus the fp16 subnormal quantum 2^-24 below the normal range
  2^-126      absolute floor wherever an fp32 intermediate below the normal range may be flushed to zero (v_exp_f32, v_rcp_f32)

A reduction over n terms by a 256-thread block: a thread adds ceil(n / 256) terms in turn, wave_sum adds 6 shuffle levels, blk_sum
2 more -- any term passes through at most k = ceil(n / 256) + 8 additions, so |sum^ - sum| <= k u sum|term| whatever the order.  A
wave per row (the LayerNorm kernels): k = ceil(cv / 64) + 6.

Library functions (no accuracy figure stands in the HIP headers, so these are the stated assumptions, in ulps = 2 u relative):
  __expf(x)   the compiler's __clang_hip_math.h defines it as __builtin_amdgcn_exp2f(0x1.715476p+0f * x), that is v_exp_f32 of a
              rounded product.  ASSUMED: v_exp_f32 within EXP2_ULPS = 1 ulp (the figure the CDNA ISA manuals give for the
              transcendental unit); results below 2^-126 may come out as 0.  The argument carries the rounding of the constant
              (<= u), of the product (u) and of x itself, so the result is off by another |x| times that, relatively.
  1.0f / s    ASSUMED within DIV_ULPS = 1 ulp (hipcc rounds fp32 division correctly by default: 0.5 ulp).
  rsqrtf      ASSUMED within RSQRT_ULPS = 2 ulp (OpenCL's bound for rsqrt, which OCML implements).
No constant here was chosen by looking at GPU output.
"""
import math

import numpy as np

U = 2.0 ** -24
H = 2.0 ** -11
F16_TINY = 2.0 ** -24
F32_FLUSH = 2.0 ** -126
EXP2_ULPS = 1.0
DIV_ULPS = 1.0
RSQRT_ULPS = 2.0
NP = {"f32": np.float32, "f16": np.float16}
EPS = 1e-5


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _f32(v):
    """a scalar argument as the float the ABI carries"""
    return float(np.float32(v))


def st(a, storage):
    """values -> the storage type (a numpy array of that type), through float32 like a device conversion"""
    return np.asarray(a, dtype=np.float32).astype(NP[storage])


def representable(a, storage):
    a = np.asarray(a)
    return bool(np.isfinite(f64(a)).all()) and bool((f64(a.astype(NP[storage])) == f64(a)).all())


def out_round(mag, storage):
    """the store of an fp32 result of magnitude <= mag: exact for fp32 storage (its last operation is already counted; 2^-126 where a
    subnormal result may be flushed), round-to-nearest for fp16 (h relative, the subnormal quantum below the normal range)"""
    mag = f64(mag)
    return np.full_like(mag, F32_FLUSH) if storage == "f32" else H * mag + F16_TINY


def rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


def block_k(n):
    return -(-max(int(n), 1) // 256) + 8


def wave_k(n):
    return -(-max(int(n), 1) // 64) + 6


# ================================================================================================
# gather / scatter: bit-exact, bound 0
# ================================================================================================
def gather_rows(src, idx, cnt, rows_out):
    """dst[j] = j < cnt ? src[idx[j]] : 0 -- src [rows, C] in the storage type; copies and zeros only: bound 0, compared as bytes.
    idx[j] for j >= cnt may hold anything (the kernel does not read the source through it)."""
    src = np.asarray(src)
    dst = np.zeros((rows_out, src.shape[1]), dtype=src.dtype)
    dst[:cnt] = src[np.asarray(idx[:cnt], dtype=np.int64)]
    return dst


def scatter_rows(src, idx, cnt, dst_rows, storage):
    """src float32 [>= cnt, C].  Returns (values [dst_rows, C] in the storage type, written [dst_rows] bool): for cnt > 0 only the rows
    idx[j], j < cnt, change, to src[j] converted round-to-nearest-even; for cnt == 0 every row is NaN in its first C columns.
    Bound 0 (one conversion, which numpy's astype restates exactly)."""
    src = np.asarray(src, dtype=np.float32)
    C = src.shape[1]
    if cnt == 0:
        return np.full((dst_rows, C), np.nan, dtype=NP[storage]), np.ones(dst_rows, dtype=bool)
    val = np.zeros((dst_rows, C), dtype=NP[storage])
    written = np.zeros(dst_rows, dtype=bool)
    rows = np.asarray(idx[:cnt], dtype=np.int64)
    val[rows] = src[:cnt].astype(NP[storage])
    written[rows] = True
    return val, written


# ================================================================================================
# masked row softmax
# ================================================================================================
def softmax_rows(s, cnt, scale, storage):
    """s [N, ld] stored scores.  Columns j < cnt: softmax_j(scale * s), columns cnt <= j < ld: 0, cnt == 0: NaN over the whole ld.
    Returns (p, bound), both [N, ld].

    softmax_rows_kernel, per row: m = max_j s_j (exact).  x_j = scale * (s_j - m) <= 0 in two roundings: x^ = x (1 + 2u).
    e^_j = __expf(x^_j): the constant and the product in front of v_exp_f32 add 2u to the argument's relative error, so the argument
    is off by 4u |x_j| absolutely (natural-log units) and e^_j = e_j (1 + d_j), d_j <= 4u |x_j| + 2 EXP2_ULPS u, or 0 where e_j is
    below 2^-126 (absolute 2^-126).  Z^ = sum e^_j over cnt terms: k = ceil(cnt / 256) + 8 additions of positive terms ->
    Z^ = Z (1 + z), |z| <= k u + sum_j p_j d_j + cnt 2^-126 (Z >= 1: the largest term is exp2(0)).  inv = 1 / Z^: DIV_ULPS ulps.
    p^_j = e^_j * inv (one rounding; e^_j is recomputed from the same operands):
      |p^_j - p_j| <= p_j (exp(d_j + (2 DIV_ULPS + 1) u) / (1 - z) - 1) + 2^-125,
    then the store: out_round().  Tails and the NaN rule are exact: bound 0."""
    s = f64(s)
    N, ld = s.shape
    p, b = np.zeros((N, ld)), np.zeros((N, ld))
    if cnt == 0:
        return np.full((N, ld), np.nan), b
    sc = _f32(scale)
    x = sc * (s[:, :cnt] - s[:, :cnt].max(1, keepdims=True))
    e = np.exp(x)
    Z = e.sum(1, keepdims=True)
    pk = e / Z
    d = 4 * U * np.abs(x) + 2 * EXP2_ULPS * U
    z = block_k(cnt) * U + (pk * d).sum(1, keepdims=True) + cnt * F32_FLUSH
    arith = pk * (np.exp(d + (2 * DIV_ULPS + 1) * U) / (1.0 - z) - 1.0) + 2 * F32_FLUSH
    p[:, :cnt] = pk
    b[:, :cnt] = arith + out_round(pk + arith, storage)
    return p, b


# ================================================================================================
# dS
# ================================================================================================
def attn_wide_ds(p, d, cnt, scale, storage):
    """p, d [N, ld] stored.  Columns j < cnt: p_j (d_j - a) scale with a = sum_{k < cnt} p_k d_k / sum_{k < cnt} p_k (the row's own sum
    in the denominator: 1 for an exact softmax row, and what keeps dS right for a STORED one whose largest entry was rounded); 0 behind;
    NaN rows when cnt == 0.  Returns (ds, bound).

    attn_wide_ds_kernel, per row, k = ceil(cnt / 256) + 8: the numerator by fmaf chains (one rounding per term) and the block
    reduction, |n^ - n| <= k u sum|p_k d_k|; the denominator z by plain additions, |z^ - z| <= k u sum|p_k|; one division
    (DIV_ULPS ulps):  A = |a^ - a| <= (k u sum|p_k d_k| + |a| k u sum|p_k|) / (|z| - k u sum|p_k|) + 2 DIV_ULPS u |a|.
    t = d_j - a^ (one rounding): |t - (d_j - a)| <= A + u (|d_j - a| + A) -- the cancellation: where d_j is close to a the error
    stays A, it does not shrink with the result.  Two products, p_j * t and * scale: 2u relative.
      |ds^_j - ds_j| <= |p_j| scale (A + u (|d_j - a| + A)) (1 + 2u) + 2u |ds_j|,  then out_round()."""
    p, d = f64(p), f64(d)
    N, ld = p.shape
    out, b = np.zeros((N, ld)), np.zeros((N, ld))
    if cnt == 0:
        return np.full((N, ld), np.nan), b
    sc = _f32(scale)
    pk, dk = p[:, :cnt], d[:, :cnt]
    z = pk.sum(1, keepdims=True)
    a = (pk * dk).sum(1, keepdims=True) / z
    ku = block_k(cnt) * U
    sp = np.abs(pk).sum(1, keepdims=True)
    A = (ku * np.abs(pk * dk).sum(1, keepdims=True) + np.abs(a) * ku * sp) / (np.abs(z) - ku * sp) + 2 * DIV_ULPS * U * np.abs(a)
    ds = pk * (dk - a) * sc
    arith = np.abs(pk) * sc * (A + U * (np.abs(dk - a) + A)) * (1 + 2 * U) + 2 * U * np.abs(ds)
    out[:, :cnt] = ds
    b[:, :cnt] = arith + out_round(np.abs(ds) + arith, storage)
    return out, b


# ================================================================================================
# LayerNorm over rows
# ================================================================================================
def ln_rows_fwd(o, x, gamma, beta, cv, eps, storage):
    """o, x [rows, C] stored, gamma / beta float32 [C].  out = LN_{first cv channels}(o + x) * gamma + beta, pad channels 0; also mean
    and rstd [rows].  Returns a dict: out, mean, rstd and their bounds out_b, mean_b, rstd_b.

    ln_rows_fwd_kernel, one wave per row, k = ceil(cv / 64) + 6.  v_c = o_c + x_c is rounded once (u |v_c|) wherever it is used.
      mean: sum of the rounded v_c, k additions, one division (DIV_ULPS ulps):
        M = |mean^ - mean| <= (k + 1) u mean_c|v_c| + 2 DIV_ULPS u |mean|.
      d_c = v_c - mean: d^_c = (v^_c - mean^) rounded once -> e_c = |d^_c - d_c| <= u |v_c| + M + u (|d_c| + u |v_c| + M).
      w = var + eps: sum of d^_c^2 by fmaf and k additions, a division, one addition:
        W = |w^ - w| <= mean_c(e_c (2 |d_c| + e_c)) + (k + 2 DIV_ULPS + 1) u (w + mean_c(e_c (2 |d_c| + e_c))).
      rstd = rsqrtf(w^): |r^ - r| <= r R, R = 1 / sqrt(1 - W / w) - 1 + 2 RSQRT_ULPS u  (not linearised: for a nearly constant row at
        a large mean W / w is not small -- the bound then says so instead of hiding it).
      out_c = d^_c r^ gamma_c + beta_c, three roundings (fewer if the compiler contracts):
        |out^_c - out_c| <= |gamma_c| r (e_c (1 + R) + |d_c| R) + 3u (|d_c r gamma_c| (1 + R) + |gamma_c| r e_c + |beta_c|), out_round().
    Pad channels: exactly 0."""
    o, x, gamma, beta = f64(o), f64(x), f64(gamma), f64(beta)
    rows, C = o.shape
    ep = _f32(eps)
    k = wave_k(cv)
    v = (o + x)[:, :cv]
    g, bt = gamma[:cv], beta[:cv]
    mean = v.sum(1, keepdims=True) / cv
    d = v - mean
    w = (d * d).sum(1, keepdims=True) / cv + ep
    r = 1.0 / np.sqrt(w)
    av = np.abs(v)
    M = (k + 1) * U * av.sum(1, keepdims=True) / cv + 2 * DIV_ULPS * U * np.abs(mean)
    e = U * av + M + U * (np.abs(d) + U * av + M)
    q = (e * (2 * np.abs(d) + e)).sum(1, keepdims=True) / cv
    W = q + (k + 2 * DIV_ULPS + 1) * U * (w + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where(W < w, 1.0 / np.sqrt(np.maximum(1.0 - W / w, 1e-300)) - 1.0, np.inf) + 2 * RSQRT_ULPS * U
    y = d * r * g + bt
    arith = np.abs(g) * r * (e * (1 + R) + np.abs(d) * R) + 3 * U * (np.abs(d * r * g) * (1 + R) + np.abs(g) * r * e + np.abs(bt))
    out, out_b = np.zeros((rows, C)), np.zeros((rows, C))
    out[:, :cv] = y
    out_b[:, :cv] = arith + out_round(np.abs(y) + arith, storage)
    return dict(out=out, mean=mean[:, 0], rstd=r[:, 0], out_b=out_b, mean_b=M[:, 0] + F32_FLUSH, rstd_b=(r * R)[:, 0])


def ln_rows_bwd(g, o, x, mean, rstd, gamma, cv, storage):
    """g, o, x [rows, C] stored; mean, rstd float32 [rows] AS GIVEN (the stored statistics, not recomputed); gamma float32 [C].
    xhat = (o + x - mean) rstd, gg = g gamma, a = mean_c(gg), b = mean_c(gg xhat) over the first cv channels:
      dY = rstd (gg - a - xhat b),  gxh = g xhat,  pad channels 0.  Returns a dict: dY, gxh, dY_b, gxh_b.

    ln_rows_bwd_kernel, one wave per row, k = ceil(cv / 64) + 6, v_c = o_c + x_c rounded once.
      xhat^: (v^ - mean) rounded, * rstd rounded: X_c = |xhat^_c - xhat_c| <= rstd u (|v_c| + |v_c - mean| + u |v_c|) (1 + u) + u |xhat_c|.
      gg^ = g gamma, one rounding.  a^: k additions and a division: Aa = (k + 1 + 2 DIV_ULPS) u mean_c|gg_c|.
      b^: fmaf chain and a division: Ab = mean_c(|gg_c| X_c) + (k + 1 + 2 DIV_ULPS) u mean_c(|gg_c| (|xhat_c| + X_c)).
      T = gg - a - xhat b: gg^ (u |gg|), - a^ (Aa, one rounding), xhat^ b^ (X |b| + (|xhat| + X) Ab, one rounding), the difference
        (one rounding), * rstd (one rounding):
        |dY^ - dY| <= rstd (u |gg| + Aa + u |gg - a| + X |b| + (|xhat| + X) Ab + u |xhat b| + u |T|) (1 + 4u) + u |dY|, out_round().
      gxh = g * xhat^: |g| X + u |g xhat|, out_round()."""
    g, o, x, mean, rstd, gamma = f64(g), f64(o), f64(x), f64(mean), f64(rstd), f64(gamma)
    rows, C = g.shape
    k = wave_k(cv)
    mu, rs = mean[:, None], rstd[:, None]
    v = (o + x)[:, :cv]
    gv, gm = g[:, :cv], gamma[:cv]
    xh = (v - mu) * rs
    gg = gv * gm
    a = gg.sum(1, keepdims=True) / cv
    b = (gg * xh).sum(1, keepdims=True) / cv
    T = gg - a - xh * b
    dY = rs * T
    gxh = gv * xh
    av = np.abs(v)
    X = np.abs(rs) * U * (av + np.abs(v - mu) + U * av) * (1 + U) + U * np.abs(xh)
    kk = (k + 1 + 2 * DIV_ULPS) * U
    Aa = kk * np.abs(gg).sum(1, keepdims=True) / cv
    Ab = (np.abs(gg) * X).sum(1, keepdims=True) / cv + kk * (np.abs(gg) * (np.abs(xh) + X)).sum(1, keepdims=True) / cv
    dY_a = np.abs(rs) * (U * np.abs(gg) + Aa + U * np.abs(gg - a) + X * np.abs(b) + (np.abs(xh) + X) * Ab + U * np.abs(xh * b)
                         + U * np.abs(T)) * (1 + 4 * U) + U * np.abs(dY)
    gxh_a = np.abs(gv) * X + U * np.abs(gxh)
    res = {}
    for name, val, ar in (("dY", dY, dY_a), ("gxh", gxh, gxh_a)):
        full, fb = np.zeros((rows, C)), np.zeros((rows, C))
        full[:, :cv] = val
        fb[:, :cv] = ar + out_round(np.abs(val) + ar, storage)
        res[name], res[name + "_b"] = full, fb
    return res


# ================================================================================================
# the whole block, one batch, float64 closed form
# ================================================================================================
def block(x, wq, bq, wk, bk, wv, bv, gamma, beta, kidx, kcnt, gout, eps=EPS):
    """x, gout [B, N, cv]; the projections' weights [cv, cv] and biases [cv]; gamma, beta [cv]; kidx [B, nkmax] with the visible keys of
    image b in kidx[b, :kcnt[b]] (any order, no repeats); the loss is sum(out * gout).  Returns a dict of float64 arrays: out, dx, dwq,
    dbq, dwk, dbk, dwv, dbv, dgamma, dbeta and the per-token dq, dk, dv [B, N, cv] (rows of masked keys 0)."""
    x, gout = f64(x), f64(gout)
    wq, bq, wk, bk, wv, bv, gamma, beta = (f64(t) for t in (wq, bq, wk, bk, wv, bv, gamma, beta))
    B, N, cv = x.shape
    scale = 1.0 / math.sqrt(cv)
    Q, K, V = x @ wq.T + bq, x @ wk.T + bk, x @ wv.T + bv
    out, dv_ = np.zeros_like(x), np.zeros_like(x)
    dq, dk, dv = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    dgamma, dbeta = np.zeros(cv), np.zeros(cv)
    ep = _f32(eps)
    for b in range(B):
        keys = np.asarray(kidx[b, :int(kcnt[b])], dtype=np.int64)
        Kg, Vg = K[b][keys], V[b][keys]
        S = (Q[b] @ Kg.T) * scale
        E = np.exp(S - S.max(1, keepdims=True))
        P = E / E.sum(1, keepdims=True)
        v = P @ Vg + x[b]
        mean = v.mean(1, keepdims=True)
        var = ((v - mean) ** 2).mean(1, keepdims=True)
        r = 1.0 / np.sqrt(var + ep)
        xh = (v - mean) * r
        out[b] = xh * gamma + beta
        g = gout[b]
        gg = g * gamma
        dY = r * (gg - gg.mean(1, keepdims=True) - xh * (gg * xh).mean(1, keepdims=True))
        dgamma += (g * xh).sum(0)
        dbeta += g.sum(0)
        dP = dY @ Vg.T
        dS = P * (dP - (P * dP).sum(1, keepdims=True)) * scale
        dq[b] = dS @ Kg
        np.add.at(dk[b], keys, dS.T @ Q[b])
        np.add.at(dv[b], keys, P.T @ dY)
        dv_[b] = dY
    dx = dv_ + dq @ wq + dk @ wk + dv @ wv
    flat = lambda t: t.reshape(B * N, cv)              # noqa: E731
    return dict(out=out, dx=dx, dwq=flat(dq).T @ flat(x), dbq=flat(dq).sum(0), dwk=flat(dk).T @ flat(x), dbk=flat(dk).sum(0),
                dwv=flat(dv).T @ flat(x), dbv=flat(dv).sum(0), dgamma=dgamma, dbeta=dbeta, dq=dq, dk=dk, dv=dv)


# ================================================================================================
# input recipes: plain numpy, fixed seeds, every value finite and exactly representable in the storage type
# ================================================================================================
C_SET = (1, 63, 64, 255, 256, 257, 300)
SCALES = (1.0 / math.sqrt(288.0), 1.0)
LD_SET = (1, 32, 33, 255, 256, 257, 513)
SCORE_RECIPES = ("random", "constant", "dominant", "span80")
LN_SHAPES = ((1, 1), (32, 24), (64, 64), (96, 65), (288, 288), (320, 300), (544, 520))
LN_RECIPES = ("random", "constant", "mean100")
DOMINANT_GAP = 120.0                 # scale * (dominant - others): exp(-120 + a few) is below every fp32 subnormal
SPAN = 80.0


def cnt_set(ld):
    return sorted({0, 1, ld - 1, ld} | {c for c in (255, 256, 257) if c <= ld})


def gather_cases():
    """(C, src_ld, rows_out, cnt): every channel count and stride at 1 and 32 rows; 4100 rows (beyond the grid cap of 4096 blocks) at C = 8"""
    out = []
    for C in C_SET:
        for ld in (C, 3 * C):
            for rows in (1, 32):
                out += [(C, ld, rows, c) for c in sorted({0, 1, rows - 1, rows})]
    for ld in (8, 24):
        out += [(8, ld, 4100, c) for c in (0, 1, 4099, 4100)]
    return out


def gather_inputs(storage, C, src_ld, rows_out, cnt):
    """src [rows_out, src_ld] with the C columns the kernel may read at column offset C of a 3C-wide row (0 when src_ld == C), NaN
    around them; idx a random permutation of the rows (behind cnt: garbage within range by construction)."""
    g = rng(11, C, src_ld, rows_out, cnt)
    off = C if src_ld > C else 0
    src = np.full((rows_out, src_ld), np.nan, dtype=NP[storage])
    src[:, off:off + C] = st(g.standard_normal((rows_out, C)) * 3, storage)
    return src, off, g.permutation(rows_out).astype(np.int32)


def scatter_cases():
    out = []
    for C in C_SET:
        for ld in (C, 3 * C):
            for rows in (1, 40):
                out += [(C, ld, rows, c) for c in sorted({0, 1, rows})]
    for ld in (8, 24):
        out += [(8, ld, 4100, c) for c in (0, 1, 4100)]
    return out


def scatter_inputs(C, dst_rows, cnt):
    """src float32 [dst_rows, C]: random values that fp16 cannot hold exactly, and in the first row exact ties between two fp16
    neighbours (round-to-nearest-even decides), an fp16 subnormal and the largest finite fp16; idx a random permutation"""
    g = rng(12, C, dst_rows, cnt)
    src = (g.standard_normal((dst_rows, C)) * 3).astype(np.float32)
    special = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 3 * 2.0 ** -26, 65504.0, 2.0 ** -25, -0.0], dtype=np.float32)
    n = min(C, len(special))
    src[0, :n] = special[:n]
    return src, g.permutation(dst_rows).astype(np.int32)


def softmax_cases():
    """(N, ld, cnt, scale): every ld and cnt edge at 1 and 5 rows, both scales; 4100 rows (beyond the 4096-block cap) at ld = 32"""
    out = [(N, ld, c, s) for ld in LD_SET for c in cnt_set(ld) for s in SCALES for N in (1, 5)]
    return out + [(4100, 32, c, SCALES[0]) for c in cnt_set(32)]


def score_row(recipe, g, ld, cnt, scale, storage):
    """one row of ld stored scores; the recipe shapes the first cnt columns, the tail is ordinary random (finite: a kernel that reads
    one column too many moves its result)"""
    row = g.standard_normal(ld) * 4
    n = max(cnt, 1)
    if recipe == "constant":
        row[:n] = 3.25
    elif recipe == "dominant":
        row[:n] = g.standard_normal(n)
        row[n // 2] = round((DOMINANT_GAP + 4.0) / scale)
    elif recipe == "span80":
        row[:n] = -(SPAN / scale) * g.permutation(n) / max(n - 1, 1)
    return st(row, storage)


def row_recipe(recipes, N, r, salt):
    """rows cycle through the recipes (a single row takes the one `salt` picks; rows beyond the list are ordinary random)"""
    if N == 1:
        return recipes[salt % len(recipes)]
    return recipes[r] if r < len(recipes) else "random"


def score_rows(storage, N, ld, cnt, scale):
    """[N, ld] stored scores and the recipe of every row"""
    g = rng(13, N, ld, cnt, int(scale * 1000), len(storage) + ord(storage[1]))
    names = [row_recipe(SCORE_RECIPES, N, r % 5, ld + cnt) for r in range(N)]
    return np.stack([score_row(nm, g, ld, cnt, scale, storage) for nm in names]), names


def ds_inputs(storage, N, ld, cnt, scale):
    """P: the stored softmax of score_rows() with garbage in (0, 1) behind cnt (in the product those columns are 0: the kernel has to
    ignore them by cnt, not by value); dP: ordinary random rows, a constant row (d - a cancels to rounding noise) in row 1"""
    s, names = score_rows(storage, N, ld, cnt, scale)
    g = rng(14, N, ld, cnt, int(scale * 1000))
    p = softmax_rows(s, max(cnt, 1), scale, storage)[0]
    p[:, cnt:] = g.random((N, ld - cnt)) * 0.9 + 0.05
    d = g.standard_normal((N, ld)) * 2
    if N > 1:
        d[1, :max(cnt, 1)] = 0.75
    return st(p, storage), st(d, storage), names


def ln_cases():
    out = [(C, cv, rows) for C, cv in LN_SHAPES for rows in (1, 3, 4, 5)]
    return out + [(32, 24, 16390)]           # (rows + 3) / 4 = 4098 blocks: beyond the cap, the grid-stride loop's second pass


def ln_row(recipe, g, C, cv, storage):
    """o, x, g rows of C stored values; the pad channels (cv..C) hold large garbage: the kernel must not read them"""
    o, x = g.standard_normal(C) * 1.5 + 0.3, g.standard_normal(C)
    if recipe == "constant":
        o[:cv], x[:cv] = 2.5, -0.75
    elif recipe == "mean100":
        o[:cv], x[:cv] = 100.0, 0.01 * g.standard_normal(cv)
    o[cv:], x[cv:] = 50.0 + g.standard_normal(C - cv), -20.0
    gr = g.standard_normal(C)
    gr[cv:] = 30.0
    return st(o, storage), st(x, storage), st(gr, storage)


def ln_inputs(storage, C, cv, rows):
    """o, x, g [rows, C] stored, gamma / beta float32 [C] (pad entries garbage: never read), and the recipe of every row"""
    g = rng(15, C, cv, rows, ord(storage[1]))
    names = [row_recipe(LN_RECIPES, rows, r % 4, C) for r in range(rows)]
    trip = [ln_row(nm, g, C, cv, storage) for nm in names]
    o, x, gr = (np.stack([t[i] for t in trip]) for i in range(3))
    gamma = (g.standard_normal(C) * 0.5 + 1.0).astype(np.float32)
    beta = (g.standard_normal(C) * 0.5).astype(np.float32)
    gamma[cv:], beta[cv:] = 7.0, -7.0
    return o, x, gr, gamma, beta, names


# ------------------------------------------------------------------------------------------------
# block-level cases
# ------------------------------------------------------------------------------------------------
BLOCK_CASES = ("short_list", "n272", "cv520", "stale", "dominant")
QK_CAP = 256.0


def _key_rows(g, B, N, nkmax, kcnt):
    """kept keys in random order without repeats in the first kcnt[b] entries, arbitrary in-range indices behind"""
    kidx = np.empty((B, nkmax), dtype=np.int32)
    for b in range(B):
        kidx[b, :kcnt[b]] = g.permutation(N)[:kcnt[b]]
        kidx[b, kcnt[b]:] = g.integers(0, N, nkmax - kcnt[b])
    return kidx


def block_case(name, storage):
    """dict: H, W, cv, x [B, N, cv] and gout stored, float32 wq bq wk bk wv bv gamma beta, int32 kidx [B, nkmax] and kcnt [B].
      short_list  cv 288, N 64, a key list of 20 columns (nkmax < N, padded to 32 inside), kept keys in random order
      n272        cv 288, N 272 = 16 x 17 with 265 and 140 kept keys: every 256-strided loop takes a second pass
      cv520       cv 520 stored at 544: column sums beyond 512, K > 512 in the products, sliced parameter gradients
      stale       kcnt = N, then 1, then 29: the score buffers of an image hold the columns of the one before
      dominant    one key with a raw score near 200 against every query, |q.k| <= 256"""
    B, H, W, cv, nkmax, kcnt = {"short_list": (2, 8, 8, 288, 20, [20, 13]), "n272": (2, 16, 17, 288, 272, [265, 140]),
                                "cv520": (2, 4, 6, 520, 24, [24, 9]), "stale": (3, 8, 8, 288, 64, [64, 1, 29]),
                                "dominant": (1, 8, 8, 288, 64, [40])}[name]
    N = H * W
    g = rng(16, BLOCK_CASES.index(name))
    wscale = (0.3 if name == "dominant" else 1.0) / math.sqrt(cv)
    w = lambda: (g.standard_normal((cv, cv)) * wscale).astype(np.float32)        # noqa: E731
    bvec = lambda: (g.standard_normal(cv) * 0.1).astype(np.float32)             # noqa: E731
    wq, wk, wv, bq, bk, bv = w(), w(), w(), bvec(), bvec(), bvec()
    gamma = (g.standard_normal(cv) * 0.5 + 1.0).astype(np.float32)
    beta = (g.standard_normal(cv) * 0.5).astype(np.float32)
    x = g.standard_normal((B, N, cv))
    kcnt = np.asarray(kcnt, dtype=np.int32)
    kidx = _key_rows(g, B, N, nkmax, kcnt)
    if name == "dominant":
        # every query carries 14 in channel 0 (its bias), one kept key gets 14 there through x: q.k ~ 196 against that key
        t = int(kidx[0, 7])
        bq[:], bk[:] = 0.0, 0.0
        bq[0] = 14.0
        r = f64(wk[0])
        x[0, t] += (14.0 / float(r @ r)) * r
    return dict(name=name, B=B, H=H, W=W, N=N, cv=cv, x=st(x, storage), gout=st(g.standard_normal((B, N, cv)), storage), wq=wq, bq=bq,
                wk=wk, bk=bk, wv=wv, bv=bv, gamma=gamma, beta=beta, kidx=kidx, kcnt=kcnt)


def block_ref(case):
    return block(case["x"], case["wq"], case["bq"], case["wk"], case["bk"], case["wv"], case["bv"], case["gamma"], case["beta"],
                 case["kidx"], case["kcnt"], case["gout"])


def raw_scores(case):
    """q.k of every query against every kept key, unscaled, float64: [B] list of [N, kcnt[b]]"""
    x = f64(case["x"])
    Q, K = x @ f64(case["wq"]).T + f64(case["bq"]), x @ f64(case["wk"]).T + f64(case["bk"])
    return [Q[b] @ K[b][np.asarray(case["kidx"][b, :case["kcnt"][b]], dtype=np.int64)].T for b in range(case["B"])]
