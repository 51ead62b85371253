"""Plain float64 restatements of what every entry point of maskunet_amd/csrc/norm.hip computes, from the operands the C ABI takes
(numpy only; no torch, no autograd, nothing of maskunet_amd).  tests/test_norm_reference_host.py pins every function against torch
in float64 before tests/test_gpu_norm_edges.py relies on it.

Every value function is followed by the error bound its GPU test uses.  A bound is the sum of the half-ulp roundings the kernel's own
operation order incurs, each times the magnitude it rounds; the docstrings walk through the kernel so the sum can be redone with
norm.hip beside it.  u = 2^-24 is half an fp32 ulp (relative); h = 2^-11 the same for fp16.  Inputs are always the values as rounded
to the storage type under test, so the bounds hold the arithmetic only.
"""
import math

import numpy as np

U = 2.0 ** -24                  # half an ulp of fp32, relative
H = 2.0 ** -11                  # half an ulp of fp16, relative
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
PHI_POLY_ERR = 5.9e-5           # common.h: |x Phi~(x) - gelu(x)|, the fp16-storage GELU
GRAD_POLY_ERR = 2.05e-4         # common.h: |GELU'~(x) - GELU'(x)|, the fp16-storage GELU derivative

_erf = np.vectorize(math.erf, otypes=[np.float64])


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _f32(v):
    """a scalar argument as the float the ABI carries"""
    return float(np.float32(v))


def storage_round(a, storage):
    """float64 values rounded to the storage type ('f32' / 'f16'), back as float64"""
    return f64(f64(a).astype(np.float32 if storage == "f32" else np.float16))


def storage_half_ulp(storage):
    return U if storage == "f32" else H


def storage_tiny(storage):
    """the quantum below the normal range that a relative bound does not cover (fp16 subnormals: 2^-24)"""
    return 0.0 if storage == "f32" else 2.0 ** -24


# ------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------
def gelu(x):
    x = f64(x)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    x = f64(x)
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act(pre, a):
    pre = f64(pre)
    return gelu(pre) if a == ACT_GELU else (np.maximum(pre, 0.0) if a == ACT_RELU else pre)


def act_grad(pre, a):
    pre = f64(pre)
    return gelu_grad(pre) if a == ACT_GELU else ((pre > 0.0).astype(np.float64) if a == ACT_RELU else np.ones_like(pre))


def act_bound(pre, y, pre_b, a, storage):
    """|act_device(pre_device) - act(pre)| given |pre_device - pre| <= pre_b, before the output rounding.
    none / ReLU: 1-Lipschitz -> pre_b.  GELU: |GELU'| <= 1.13 -> 1.13 pre_b, plus
      fp32 storage: 8 u max(|y|, |pre|) for erff (a few ulp of a value near 1, times |pre| / 2), the rounding of x / sqrt 2 and the two products;
      fp16 storage: the polynomial's documented 5.9e-5 (fp32 Horner included)."""
    if a != ACT_GELU:
        return f64(pre_b)
    if storage == "f32":
        return 1.13 * f64(pre_b) + 8 * U * np.maximum(np.abs(y), np.abs(pre))
    return 1.13 * f64(pre_b) + PHI_POLY_ERR


def act_grad_bound(pre_b, a, storage):
    """|act'_device(pre_device) - act'(pre)|.  none: 0.  ReLU: 0 -- the step is compared only where |pre| exceeds its own rounding
    (relu_margin).  GELU: |GELU''| = |phi(x) (2 - x^2)| <= 0.8 -> 0.8 pre_b, plus 8 u (fp32: erff near 1, __expf's argument rounding
    x^3 phi(x) / 2 u <= 0.23 u, three products) or the polynomial's 2.05e-4 (fp16)."""
    if a == ACT_NONE or a == ACT_RELU:
        return 0.0 * f64(pre_b)
    return 0.8 * f64(pre_b) + (8 * U if storage == "f32" else GRAD_POLY_ERR)


# ------------------------------------------------------------------------------------------------
# BatchNorm statistics
# ------------------------------------------------------------------------------------------------
def _running(mean, var, M, momentum, running_mean, running_var, c_valid):
    if running_mean is None:
        return None, None
    mom = _f32(momentum)
    unb = var * (M / (M - 1.0)) if M > 1 else var            # the device's rule: the factor is 1 at M = 1
    rm, rv = f64(running_mean).copy(), f64(running_var).copy()
    rm[:c_valid] = (1.0 - mom) * rm[:c_valid] + mom * mean[:c_valid]
    rv[:c_valid] = (1.0 - mom) * rv[:c_valid] + mom * unb[:c_valid]
    return rm, rv


def bn_stats(x, eps, momentum=0.1, running_mean=None, running_var=None, c_valid=None):
    """x [M, C].  mean and BIASED variance per channel over the M rows, rstd = 1 / sqrt(var + eps); the running statistics of the
    channels below c_valid move by `momentum` towards the batch mean and the UNBIASED variance (factor M / (M - 1); 1 at M = 1),
    the others keep their values.  Returns a dict: mean, var, rstd, running_mean, running_var (None without running operands),
    absmean = mean |x|, ex2 = mean x^2 (what the bounds scale with)."""
    x = f64(x)
    M, C = x.shape
    c_valid = C if c_valid is None else c_valid
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    rstd = 1.0 / np.sqrt(var + _f32(eps))
    rm, rv = _running(mean, var, M, momentum, running_mean, running_var, c_valid)
    return dict(mean=mean, var=var, rstd=rstd, running_mean=rm, running_var=rv, absmean=np.abs(x).sum(0) / M, ex2=(x * x).sum(0) / M, M=M)


def bn_stats_bounds(ref, eps, momentum=0.1):
    """bn_partial_kernel<MODE 0> + bn_fwd_final_kernel.  A thread sums U = 8 rows of x and of x^2 in fp32 (7 adds / 8 fmaf) and folds
    the two short sums into fp64; everything after the fold (LDS reduce, partial blocks, finalize) is fp64 and contributes ~2^-53.
      mean: every add of a short sum rounds by at most u times that short sum's sum|x| -> 7 u mean|x| over the tensor; the store of
            mean rounds u |m|.  Bound: u |m| + 8 u mean|x|.
      var (biased, absolute): var = q / M - m^2.  q: 8 fmaf roundings per short sum, each at most u times the short sum of squares ->
            8 u E[x^2].  m^2: 2 |m| dm with dm <= 7 u mean|x| and |m| mean|x| <= E[x^2] -> 14 u E[x^2].  Together 22 u E[x^2]; the
            bound is 24 u E[x^2].  It is relative to E[x^2], NOT to the variance: at mean / std = r it is 24 u (1 + r^2) of the variance.
      rstd: d rstd = -0.5 rstd dvar / (var + eps) to first order, plus the store and the 1 / sqrt in fp64 -> rstd (2 u + 0.5 var_b / (var + eps)).
            (Where var_b exceeds var + eps the first-order term is above rstd itself, which no non-negative value below
            1 / sqrt(eps) can miss by more.)
      running statistics: momentum times the batch errors (times M / (M - 1) for the variance), plus u of the stored value."""
    mean_b = U * np.abs(ref["mean"]) + 8 * U * ref["absmean"]
    var_b = 24 * U * ref["ex2"]
    rstd_b = ref["rstd"] * (2 * U + 0.5 * var_b / (ref["var"] + _f32(eps)))
    out = dict(mean=mean_b, var=var_b, rstd=rstd_b)
    if ref["running_mean"] is not None:
        M, mom = ref["M"], _f32(momentum)
        out["running_mean"] = mom * mean_b + U * np.abs(ref["running_mean"])
        out["running_var"] = mom * var_b * (M / (M - 1.0) if M > 1 else 1.0) + U * np.abs(ref["running_var"])
    return out


def bn_stats_from_rows(part, M, eps, momentum=0.1, running_mean=None, running_var=None, c_valid=None):
    """part [rows, C, 2] float32: per row (sum x, sum x^2) of a group of the M data rows (the conv epilogue's statistics rows).
    The float32 rows summed in float64; var = max(q / M - m^2, 0).  Same dict as bn_stats (absmean = sum |part sums| / M)."""
    part = f64(part)
    C = part.shape[1]
    c_valid = C if c_valid is None else c_valid
    s, q = part[:, :, 0].sum(0), part[:, :, 1].sum(0)
    mean = s / M
    var = np.maximum(q / M - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + _f32(eps))
    rm, rv = _running(mean, var, M, momentum, running_mean, running_var, c_valid)
    return dict(mean=mean, var=var, rstd=rstd, running_mean=rm, running_var=rv, absmean=np.abs(part[:, :, 0]).sum(0) / M, ex2=q / M, M=M)


def tight_stats_bounds(ref, momentum=0.1):
    """Statistics accumulated in fp64 from exact fp32 / fp16 terms (mu_bn_train_stats_rows: bn_fwd_final_kernel<FROWS> or
    bn_fold_rows_kernel; the LayerNorm sweep lns_partial_kernel<MODE 0>): the sums carry ~n 2^-53, the only fp32 roundings are the
    stores.  mean: 2 u |m| + u mean|x| (the second term holds a mean that cancels to near 0); rstd: 2 u relative, at any mean / std;
    running statistics: 2 u of the stored value plus momentum times the batch bound."""
    mean_b = 2 * U * np.abs(ref["mean"]) + U * ref["absmean"]
    out = dict(mean=mean_b, rstd=2 * U * ref["rstd"])
    if ref.get("running_mean") is not None:
        mom = _f32(momentum)
        out["running_mean"] = mom * mean_b + 2 * U * np.abs(ref["running_mean"])
        out["running_var"] = 2 * U * np.abs(ref["running_var"]) + mom * 2.0 ** -40 * ref["ex2"]      # fp64 sums: <= 2^13 adds per accumulator
    return out


def bn_eval_stats(running_mean, running_var, eps, c_valid=None):
    """eval mode: (mean, rstd) = (running_mean, 1 / sqrt(running_var + eps)); channels at and beyond c_valid get (0, 1).
    Device (bn_eval_stats_kernel, all fp32): the add rounds u (-> u / 2 on rstd), sqrtf <= 1 ulp = 2 u, the division <= 2.5 ulp = 5 u:
    bound 8 u rstd; mean is a copy (exact)."""
    rm, rv = f64(running_mean), f64(running_var)
    C = rm.shape[0]
    c_valid = C if c_valid is None else c_valid
    mean, rstd = np.zeros(C), np.ones(C)
    mean[:c_valid] = rm[:c_valid]
    rstd[:c_valid] = 1.0 / np.sqrt(rv[:c_valid] + _f32(eps))
    return mean, rstd


def bn_eval_fold(rm1, rv1, g1, b1, eps1, rm2=None, rv2=None, g2=None, b2=None, eps2=0.0, conv_bias=None, c_valid=None):
    """One or two eval-mode BatchNorms behind a convolution as (scale, shift): a1 = g1 / sqrt(rv1 + eps1),
    s1 = b1 + (bias - rm1) a1; with a second layer a2 likewise, scale = a1 a2, shift = (s1 - rm2) a2 + b2.  NULL gamma = 1,
    NULL beta / bias = 0; channels at and beyond c_valid get (0, 0).  Device: fp32 throughout, so every intermediate rounds by u of
    itself; the test's bound is 16 u (|scale|, and for shift the sum of the magnitudes of its terms), returned as `mag`."""
    C = f64(rm1).shape[0]
    c_valid = C if c_valid is None else c_valid
    one, zero = np.ones(C), np.zeros(C)
    g1 = one if g1 is None else f64(g1)
    b1 = zero if b1 is None else f64(b1)
    cb = zero if conv_bias is None else f64(conv_bias)
    a = g1 / np.sqrt(f64(rv1) + _f32(eps1))
    sh = b1 + (cb - f64(rm1)) * a
    mag = np.abs(b1) + (np.abs(cb) + np.abs(f64(rm1))) * np.abs(a)
    if rm2 is not None:
        g2 = one if g2 is None else f64(g2)
        b2 = zero if b2 is None else f64(b2)
        a2 = g2 / np.sqrt(f64(rv2) + _f32(eps2))
        sh = (sh - f64(rm2)) * a2 + b2
        mag = (mag + np.abs(f64(rm2))) * np.abs(a2) + np.abs(b2)
        a = a * a2
    a[c_valid:], sh[c_valid:], mag[c_valid:] = 0.0, 0.0, 0.0
    return a, sh, mag


# ------------------------------------------------------------------------------------------------
# BatchNorm apply, forward
# ------------------------------------------------------------------------------------------------
def bn_act_fwd(x, res, mean, rstd, gamma, beta, a):
    """y = act((x - mean) rstd gamma + beta + res) per channel; res may be None.  Returns (y, pre)."""
    x = f64(x)
    pre = (x - f64(mean)) * f64(rstd) * f64(gamma) + f64(beta)
    if res is not None:
        pre = pre + f64(res)
    return act(pre, a), pre


def bn_act_fwd_bound(x, res, mean, rstd, gamma, beta, a, y, pre, storage):
    """bn_act_fwd_kernel: a = rstd gamma (u |a|), b = beta - mean a (u |mean a| for the product's a, u |mean a| for the product, u |b|
    for the difference), pre = fma(x, a, b) (u |x a| from a, u |x a + b|), pre += res (u |pre|).  With A = |rstd gamma|,
    |b| <= |beta| + |mean| A and |x a + b| <= |x| A + |b|:
        pre_b = u (4 |x| A + 5 |mean| A + 3 |beta| + |res|)
    (the |mean| A term is what cancellation costs when the mean is large against the spread).  Then the activation (act_bound)
    and, for fp16 storage, the output rounding h |y| + 2^-24."""
    A = np.abs(f64(rstd) * f64(gamma))
    pre_b = U * (4 * np.abs(f64(x)) * A + 5 * np.abs(f64(mean)) * A + 3 * np.abs(f64(beta)) + (0.0 if res is None else np.abs(f64(res))))
    b = act_bound(pre, y, pre_b, a, storage)
    if storage == "f16":
        b = b + H * np.abs(y) + storage_tiny(storage)
    return b


# ------------------------------------------------------------------------------------------------
# BatchNorm backward
# ------------------------------------------------------------------------------------------------
def relu_margin(x, res, mean, rstd, gamma, beta, storage):
    """(|pre|, margin): a ReLU pre-activation within margin = 2^-10 (|xhat gamma| + |beta| + |res|) of 0 (2^-6 times that for fp16
    storage) may legitimately take the other side of the step on the device.  The GPU tests move such x before they compare."""
    xhat = (f64(x) - f64(mean)) * f64(rstd)
    t = xhat * f64(gamma)
    pre = t + f64(beta) + (0.0 if res is None else f64(res))
    mag = np.abs(t) + np.abs(f64(beta)) + (0.0 if res is None else np.abs(f64(res)))
    return np.abs(pre), (2.0 ** -10 if storage == "f32" else 2.0 ** -6) * mag


def bn_act_bwd(x, res, g, mean, rstd, gamma, beta, a, training, xhat_scale=None, storage="f32"):
    """xhat = (x - mean) rstd, pre = xhat gamma + beta + res, dz = g act'(pre) ROUNDED TO THE STORAGE TYPE (the kernel sums and applies
    the values it stores), dbeta = sum dz, dgamma = sum dz xhat, and
        training: dx = gamma rstd (dz - dbeta / M - xhat xhat_scale dgamma / M)        (xhat_scale NULL = 1)
        eval:     dx = gamma rstd dz
    dres = dz.  Returns a dict with dx, dres, dgamma, dbeta and the intermediates the bounds need."""
    x, g = f64(x), f64(g)
    M = x.shape[0]
    mean, rstd, gamma, beta = f64(mean), f64(rstd), f64(gamma), f64(beta)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta + (0.0 if res is None else f64(res))
    dz = storage_round(g * act_grad(pre, a), storage)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    xs = np.ones_like(gamma) if xhat_scale is None else f64(xhat_scale)
    s1 = dbeta / M if training else np.zeros_like(dbeta)
    s2 = xs * dgamma / M if training else np.zeros_like(dgamma)
    dx = gamma * rstd * (dz - s1 - xhat * s2)
    return dict(dx=dx, dres=dz, dgamma=dgamma, dbeta=dbeta, dz=dz, xhat=xhat, pre=pre, s1=s1, s2=s2, xs=xs, g=g, x=x, M=M,
                mean=mean, rstd=rstd, gamma=gamma, beta=beta, res=None if res is None else f64(res))


def bn_act_bwd_bounds(r, a, storage):
    """bn_partial_kernel<MODE 1>, bn_bwd_final_kernel, bn_bwd_apply_kernel on the dict of bn_act_bwd.
      xh = (x - mu) rs: the difference and the product round -> 2 u |xhat|.
      pre = fma(xh, gamma, beta) + res: |gamma| 2 u |xhat| + u |xhat gamma + beta| + u |pre| <= pre_b = u (4 |xhat gamma| + 2 |beta| + 2 |res|).
      dz = T(g act'(pre)): |g| act_grad_bound(pre_b) + u |dz| for the product, and two half-ulps of T (the device rounds its fp32
           value, the reference its fp64 one: the two roundings can fall on either side) -> dz_b.  This is also the bound of dres.
      dbeta: the device sums ITS dz: sum dz_b, one fp32 add per pair of rows (U = 2) u sum|dz|, the store u |dbeta|.
      dgamma: sum (dz_b |xhat| + |dz| 2 u |xhat|), the fmaf and the pair's add 2 u sum|dz xhat|, the store u |dgamma|.
      s1 = dbeta / M, s2 = xs dgamma / M: the sums' bounds over M (times |xs|) plus the stores u |s1|, 2 u |s2|.
      dx = fma(gr, dz, fma(k1, x, k0)), gr = gamma rs, k1 = -gr rs s2, k0 = -gr s1 - k1 mu: value errors
           |gr| (dz_b + s1_b + |xhat| s2_b); roundings: gr u, k1 3 u, k0 and the two fma one u each of their results -> at most
           8 u (|gr| (|dz| + |s1|) + |gr rs s2| (|x| + |mu|)) -- the last term is the cancellation of k1 x against k1 mu; then the
           output rounding of T."""
    hT, tiny = storage_half_ulp(storage), storage_tiny(storage)
    ax, agam = np.abs(r["xhat"]), np.abs(r["gamma"])
    ares = 0.0 if r["res"] is None else np.abs(r["res"])
    pre_b = U * (4 * ax * agam + 2 * np.abs(r["beta"]) + 2 * ares)
    adz = np.abs(r["dz"])
    dz_b = np.abs(r["g"]) * act_grad_bound(pre_b, a, storage) + U * adz + 2 * hT * adz + tiny
    M = r["M"]
    dbeta_b = dz_b.sum(0) + U * adz.sum(0) + U * np.abs(r["dbeta"])
    dgamma_b = (dz_b * ax + 2 * U * adz * ax).sum(0) + 2 * U * (adz * ax).sum(0) + U * np.abs(r["dgamma"])
    s1_b = dbeta_b / M + U * np.abs(r["s1"])
    s2_b = np.abs(r["xs"]) * dgamma_b / M + 2 * U * np.abs(r["s2"])
    training = bool(np.any(r["s1"] != 0) or np.any(r["s2"] != 0))
    gr = np.abs(r["gamma"] * r["rstd"])
    if not training:
        s1_b, s2_b = 0.0 * s1_b, 0.0 * s2_b
    dx_b = gr * (dz_b + s1_b + ax * s2_b) \
        + 8 * U * (gr * (adz + np.abs(r["s1"])) + gr * np.abs(r["rstd"] * r["s2"]) * (np.abs(r["x"]) + np.abs(r["mean"]))) \
        + hT * np.abs(r["dx"]) + tiny
    return dict(dx=dx_b, dres=dz_b, dbeta=dbeta_b, dgamma=dgamma_b)


def dx_scale(bound):
    """The power of two S under which mu_bn_act_bwd_h writes fp16(S dx): it puts `bound` (a float32 > 0) into [2^13, 2^14), i.e.
    S = 2^(13 - floor(log2 bound)) with the exponent clamped to +-100; a zero, subnormal, infinite or NaN bound gives S = 1."""
    b = np.float32(bound)
    e = int((b.view(np.uint32) >> 23) & 0xff) - 127
    if not (b > 0) or e <= -127 or e >= 128:
        return 1.0
    return 2.0 ** min(max(13 - e, -100), 100)


def dx_bound_per_channel(r):
    """what bn_bwd_final_kernel bounds |dx| with in a channel: |gamma rstd| (max|dz| + |s1| + max|xhat| |s2|)"""
    return np.abs(r["gamma"] * r["rstd"]) * (np.abs(r["dz"]).max(0) + np.abs(r["s1"]) + np.abs(r["xhat"]).max(0) * np.abs(r["s2"]))


# ------------------------------------------------------------------------------------------------
# BatchNorm pair
# ------------------------------------------------------------------------------------------------
def bn_pair_compose(rstd1, gamma1, beta1, gamma2, M, eps1, eps2, momentum2=0.1, running_mean2=None, running_var2=None, c_valid=None):
    """Second BatchNorm directly behind a first (training): y1 = gamma1 u + beta1 with mean u = 0, mean u^2 = q = 1 - eps1 rstd1^2
    (clamped at 0), so mean(y1) = beta1, var(y1) = gamma1^2 q, r2 = 1 / sqrt(var(y1) + eps2) and
        gamma_eff = gamma1 gamma2 r2,  xhat_scale = r2^2 (gamma1^2 + eps2),  dgamma2_coef = gamma1 r2,  dgamma1_coef = gamma2 r2^3 eps2;
    the second layer's running statistics move towards (beta1, var(y1) M / (M - 1)) below c_valid.
    Device: the same expressions in fp64 on the fp32 operands, one store each: 2 u relative (the test's 2^-23)."""
    r1, g1, g2 = f64(rstd1), f64(gamma1), f64(gamma2)
    e1, e2 = _f32(eps1), _f32(eps2)
    C = r1.shape[0]
    c_valid = C if c_valid is None else c_valid
    q = np.maximum(1.0 - e1 * r1 * r1, 0.0)
    var2 = g1 * g1 * q
    r2 = 1.0 / np.sqrt(var2 + e2)
    rm, rv = _running(f64(beta1), var2, M, momentum2, running_mean2, running_var2, c_valid)
    return dict(gamma_eff=g1 * g2 * r2, xhat_scale=r2 * r2 * (g1 * g1 + e2), dgamma2_coef=g1 * r2, dgamma1_coef=g2 * r2 ** 3 * e2,
                running_mean2=rm, running_var2=rv, q=q, r2=r2)


def pair_grads(dgamma2_coef, dgamma1_coef, A):
    """the three rows mu_bn_pair_bwd writes: dgamma2 = dgamma2_coef A, dgamma1 = dgamma1_coef A (A = sum dz xhat, the single-layer
    dgamma), dbeta1 = 0.  Each product is one fp32 rounding of coef * float(A): bound u |product| + |coef| (A's own bound)."""
    A = f64(A)
    return np.stack([f64(dgamma2_coef) * A, f64(dgamma1_coef) * A, np.zeros_like(A)])


# ------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------
def colsum(x):
    """out[c] = sum_r x[r][c].  Returns (sum, sum |x|).  Device: short fp32 sums (8 rows; the encoded form up to 64) folded into fp64,
    one store: bound u |sum| + 8 u sum|x|."""
    x = f64(x)
    return x.sum(0), np.abs(x).sum(0)


def colsum_bound(s, sabs):
    return U * np.abs(s) + 8 * U * sabs


# ------------------------------------------------------------------------------------------------
# per-sample LayerNorm with a full-shape affine
# ------------------------------------------------------------------------------------------------
def ln_sample_fwd(x, w, b, eps):
    """x [B, L], w, b [L]: per sample mean and biased variance over L, y = (x - mean) rstd w + b.  Returns a dict with y, mean, rstd,
    absmean, xhat."""
    x = f64(x)
    L = x.shape[1]
    mean = x.sum(1) / L
    var = ((x - mean[:, None]) ** 2).sum(1) / L
    rstd = 1.0 / np.sqrt(var + _f32(eps))
    xhat = (x - mean[:, None]) * rstd[:, None]
    return dict(y=xhat * f64(w) + f64(b), mean=mean, rstd=rstd, xhat=xhat, absmean=np.abs(x).sum(1) / L, w=f64(w), b=f64(b))


def ln_sample_fwd_bounds(r, storage):
    """lns_partial_kernel<MODE 0> accumulates x and x^2 in fp64 element by element: tight_stats_bounds for mean and rstd.
    lns_fwd_apply_kernel reads the STORED mean and rstd: y = ((x - mu) rs) w + b moves by rs |w| dmean + |xhat w| (drstd / rstd), and
    its four fp32 operations round by at most 4 u (|xhat w| + |b|); fp16 storage adds h |y| + 2^-24."""
    st = tight_stats_bounds(r)
    aw = np.abs(r["xhat"] * r["w"])
    y_b = (r["rstd"] * st["mean"])[:, None] * np.abs(r["w"]) + aw * 2 * U + 4 * U * (aw + np.abs(r["b"]))
    if storage == "f16":
        y_b = y_b + H * np.abs(r["y"]) + storage_tiny(storage)
    return dict(mean=st["mean"], rstd=st["rstd"], y=y_b)


def ln_sample_bwd(x, dy, w, mean, rstd):
    """mean, rstd [B] are operands (the forward's stored values).  xhat = (x - mean) rstd, gw = dy w, m1 = mean_L gw, m2 = mean_L gw xhat,
    dx = rstd (gw - m1 - xhat m2), dw = sum_b dy xhat, db = sum_b dy."""
    x, dy, w = f64(x), f64(dy), f64(w)
    mean, rstd = f64(mean)[:, None], f64(rstd)[:, None]
    xhat = (x - mean) * rstd
    gw = dy * w
    m1, m2 = gw.mean(1, keepdims=True), (gw * xhat).mean(1, keepdims=True)
    return dict(dx=rstd * (gw - m1 - xhat * m2), dw=(dy * xhat).sum(0), db=dy.sum(0), xhat=xhat, gw=gw, m1=m1, m2=m2, rstd=rstd, dy=dy,
                dw_abs=np.abs(dy * xhat).sum(0), db_abs=np.abs(dy).sum(0), B=x.shape[0])


def ln_sample_bwd_bounds(r, storage):
    """lns_partial_kernel<MODE 1>: gw = dy w in fp32 (u |gw|), xh = (x - mu) rs (2 u |xhat|), both summed in fp64; the stores of m1, m2
    round u: m1_b = u (mean|gw| + |m1|), m2_b = u (3 mean|gw xhat| + |m2|).
    lns_bwd_apply_kernel: dx = rs (g w - m1 - xh m2): value errors rs (u |gw| + m1_b + |xhat| m2_b + 2 u |xhat m2|), four roundings
    4 u rs (|gw| + |m1| + |xhat m2|), then the output rounding of T.
    dw, db: the issue's bound B u sum_b |term| (`dw`, `db`); a term dy xh carries the two roundings of xh besides those of the
    product and the add, so `dw_wide` = (B + 3) u sum_b |dy xhat| is what the operation order gives (see NOTES_r12.md)."""
    hT, tiny = storage_half_ulp(storage), storage_tiny(storage)
    agw, ax, rs = np.abs(r["gw"]), np.abs(r["xhat"]), r["rstd"]
    m1_b = U * (agw.mean(1, keepdims=True) + np.abs(r["m1"]))
    m2_b = U * (3 * (agw * ax).mean(1, keepdims=True) + np.abs(r["m2"]))
    axm2 = ax * np.abs(r["m2"])
    dx_b = rs * (U * agw + m1_b + ax * m2_b + 2 * U * axm2) + 4 * U * rs * (agw + np.abs(r["m1"]) + axm2) + hT * np.abs(r["dx"]) + tiny
    B = r["B"]
    return dict(dx=dx_b, dw=B * U * r["dw_abs"], db=B * U * r["db_abs"], dw_wide=(B + 3) * U * r["dw_abs"])
