"""Plain float64 restatements of the operations of maskunet_amd/csrc/loss.hip, loop by loop from their definitions (numpy; torch's
CPU autograd only for the gradient of the instance loss).  Nothing of maskunet_amd is used.  tests/test_loss_reference_host.py pins
every function here against torch / the oracle / the committed fixtures before the GPU tests rely on them.

  * cross-entropy (nn.CrossEntropyLoss(ignore_index), mean reduction): per row lse = log sum_c exp(x_c) over the first C channels,
    loss = mean over the rows whose label is not `ignore` of lse - x[label], d loss / d x = (softmax - onehot) / count on those rows;
  * mean IoU (ade_semantic.py:128-146): arg-max (first maximum), per class I = #(pred == c and label == c), P = #(pred == c),
    L = #(label == c), U = P + L - I, mean over the classes with U > 0 of (I + smooth) / (U + smooth);
  * AdamW (torch.optim.AdamW: decoupled decay, bias-corrected moments), one step counter per tensor;
  * InstanceContrastiveLoss (oracle.instance_contrastive_loss) plus the two rules of the device version (include/maskunet_hip.h):
    ids outside [0, id_cap) are not instances but their pixels are negatives, and only the first max_inst qualifying ids count.
"""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------------
def ce_rows(logits, labels, C, ignore):
    """logits: [M, >= C] array or tensor, ALREADY rounded to the dtype under test (only the first C channels are read);
    labels: [M] integers.  Returns a dict of float64 values:
      lse [M], mx [M] (row maximum), count (int), loss (nan when count == 0), p [M, C] softmax,
      g [M, C] = softmax - onehot on the counted rows and 0 on the ignored ones (= d loss / d logits * count)."""
    x = _f64(logits)[:, :C]
    lab = np.asarray(_np(labels), dtype=np.int64).reshape(-1)
    M = x.shape[0]
    assert lab.shape[0] == M
    mx = x.max(axis=1)
    p = np.exp(x - mx[:, None])                 # exp(-inf) = 0: a -inf logit takes no part
    se = p.sum(axis=1)
    lse = mx + np.log(se)
    p /= se[:, None]
    counted = lab != ignore
    count = int(counted.sum())
    rows = np.flatnonzero(counted)
    assert np.all((lab[rows] >= 0) & (lab[rows] < C)), "a counted label outside [0, C)"
    tgt = x[rows, lab[rows]]
    loss = float(np.sum(lse[rows] - tgt) / count) if count else float("nan")
    g = p.copy()
    g[rows, lab[rows]] -= 1.0
    g[~counted] = 0.0
    return {"lse": lse, "mx": mx, "count": count, "loss": loss, "p": p, "g": g}


# ------------------------------------------------------------------------------------------------
# mean IoU
# ------------------------------------------------------------------------------------------------
def iou_counts(pred_logits, labels, C, smooth=1e-6):
    """pred_logits: [M, >= C] (first C channels read), labels [M] (values outside [0, C) belong to no class).
    Returns (counts int64 [3, C] = (I, P, L), mean IoU as a float)."""
    x = _f64(pred_logits)[:, :C]
    lab = np.asarray(_np(labels), dtype=np.int64).reshape(-1)
    pred = np.argmax(x, axis=1)                  # numpy: the first maximum
    I = np.zeros(C, dtype=np.int64)
    P = np.bincount(pred, minlength=C).astype(np.int64)
    inr = (lab >= 0) & (lab < C)
    L = np.bincount(lab[inr], minlength=C).astype(np.int64)
    hit = inr & (pred == lab)
    I += np.bincount(lab[hit], minlength=C)
    U = P + L - I
    seen = U > 0
    miou = float(np.mean((I[seen] + smooth) / (U[seen] + smooth))) if seen.any() else float("nan")
    return np.stack([I, P, L]), miou


# ------------------------------------------------------------------------------------------------
# AdamW
# ------------------------------------------------------------------------------------------------
def adamw_steps(params, grads, lr, betas, eps, weight_decay, grad_scale=1.0, set_step=None):
    """AdamW in float64 on the hyper-parameters as the kernel receives them: lr, beta1, beta2, eps, weight_decay and 1 / grad_scale are
    rounded to fp32 first, then everything is float64.

    params: list of fp32 arrays.  grads: one list per step with, per tensor, the (loss-scaled) gradient array or None (no gradient:
    the tensor and its step counter stay as they are).  weight_decay: a float or one per tensor.  set_step: {(step index, tensor
    index): value} -- the tensor's counter is set to `value` before that step (a resumed run).
    Returns one entry per step: a list over the tensors of (p, m, v, m_abs) float64 arrays.  m_abs is the same recursion as m on
    |g| (beta1 * m_abs + (1 - beta1) * |g|): the magnitude of the terms that m sums, which is what fp32 rounding of m is relative to
    (m itself may cancel to nothing; v sums non-negative terms, so its own value is that magnitude)."""
    f = lambda a: float(np.float32(a))
    lr, b1, b2, eps, ginv = f(lr), f(betas[0]), f(betas[1]), f(eps), f(1.0 / float(grad_scale))
    n = len(params)
    wd = [f(w) for w in (weight_decay if isinstance(weight_decay, (list, tuple)) else [weight_decay] * n)]
    p = [np.asarray(a, dtype=np.float64).copy() for a in params]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    ma = [np.zeros_like(a) for a in p]
    t = [0] * n
    out = []
    for it, gs in enumerate(grads):
        for i in range(n):
            if set_step and (it, i) in set_step:
                t[i] = int(set_step[(it, i)])
            if gs[i] is None:
                continue
            t[i] += 1
            g = np.asarray(gs[i], dtype=np.float64) * ginv
            p[i] = p[i] * (1.0 - lr * wd[i])
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            ma[i] = b1 * ma[i] + (1.0 - b1) * np.abs(g)
            bc1 = 1.0 - b1 ** t[i]
            bc2 = 1.0 - b2 ** t[i]
            p[i] = p[i] - (lr / bc1) * (m[i] / (np.sqrt(v[i]) / np.sqrt(bc2) + eps))
        out.append([(p[i].copy(), m[i].copy(), v[i].copy(), ma[i].copy()) for i in range(n)])
    return out


# ------------------------------------------------------------------------------------------------
# instance triplet loss
# ------------------------------------------------------------------------------------------------
def instance_ids(mask, ignore, id_cap, max_inst):
    """The instances that reach the draw, in the order the k-th entry of `u` is used: [(id, n_pixels, n_negatives)] for the ids in
    [0, id_cap) other than 0 and `ignore` (None: no ignore label) with at least two pixels and at least one pixel outside them, in
    increasing order, the first max_inst of them."""
    flat = np.asarray(_np(mask), dtype=np.int64).reshape(-1)
    out = []
    for inst in np.unique(flat).tolist():
        if inst <= 0 or inst >= id_cap or (ignore is not None and inst == ignore):
            continue
        c = int((flat == inst).sum())
        if c < 2 or flat.size - c == 0:
            continue
        out.append((inst, c, flat.size - c))
    return out[:max_inst]


def u_for_negative(mask, inst, pixel):
    """u = (j + 0.5) / n_neg such that the j-th pixel (row-major) outside instance `inst` is `pixel`."""
    flat = np.asarray(_np(mask), dtype=np.int64).reshape(-1)
    assert flat[pixel] != inst
    neg = flat != inst
    return (int(neg[:pixel].sum()) + 0.5) / int(neg.sum())


def instance_triplet(feat, mask, u, margin, ignore, id_cap, max_inst):
    """feat [B,C,H,W], mask int [B,H,W], u: one number per instance that reaches the draw.  Pixel (b, h, w) addresses the feature column
    feat[:, :, b, h] (the reference's own indexing, needs B <= H <= W).  Per instance: anchor / positive = its first two pixels in
    row-major order, negative = the floor(u[k] * n_neg)-th pixel whose label is not the instance's (at most the last one),
    l_k = max(|a - p + 1e-6| - |a - n + 1e-6| + margin, 0); loss = mean of l_k (0 without instances).
    Returns (loss, dfeat [B,C,H,W], hinge [K]) in float64; hinge[k] = d_ap - d_an + margin before the clamp."""
    f = torch.as_tensor(_f64(feat)).clone().requires_grad_(True)
    m = np.asarray(_np(mask), dtype=np.int64)
    B, H, W = m.shape
    assert B <= H <= W and tuple(f.shape[0:1] + f.shape[2:]) == (B, H, W)
    flat = m.reshape(-1)
    uu = np.asarray(_np(u), dtype=np.float64).reshape(-1)

    def column(pix):
        b, h = pix // (H * W), (pix // W) % H
        return f[:, :, b, h].reshape(-1)

    terms, hinge = [], []
    for k, (inst, c, n_neg) in enumerate(instance_ids(m, ignore, id_cap, max_inst)):
        own = np.flatnonzero(flat == inst)
        others = np.flatnonzero(flat != inst)
        j = min(int(np.floor(uu[k] * n_neg)), n_neg - 1)
        a, p, n = column(int(own[0])), column(int(own[1])), column(int(others[j]))
        d_ap = torch.sqrt(torch.sum((a - p + 1e-6) ** 2))
        d_an = torch.sqrt(torch.sum((a - n + 1e-6) ** 2))
        h = d_ap - d_an + margin
        hinge.append(h.item())
        terms.append(torch.clamp(h, min=0.0))
    if not terms:
        return 0.0, np.zeros(tuple(f.shape)), np.zeros(0)
    loss = torch.stack(terms).sum() / len(terms)
    if loss.requires_grad:
        loss.backward()
    grad = f.grad.numpy() if f.grad is not None else np.zeros(tuple(f.shape))
    return loss.item(), grad, np.asarray(hinge)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _f64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double().numpy()
    return np.asarray(a, dtype=np.float64)
