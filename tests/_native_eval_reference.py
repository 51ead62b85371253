"""Numpy restatement of the native-resolution semantic evaluation (mu_sem_eval_native in include/maskunet_hip.h): the bilinear rule in
fp32, operation by operation and in the contract's order, then the first arg-max and the counts.  Plain numpy, imported by the host test
(which pins it to torch's F.interpolate) and by the GPU test (which holds the kernel to it with ==)."""
import numpy as np

F32 = np.float32


def taps(n_in, n_out, dtype=F32):
    """(i0, i1, l0, l1) of every output index of one axis; dtype=np.float64 gives the same formula in double"""
    s = dtype(n_in) / dtype(n_out)
    f = np.maximum(s * (np.arange(n_out).astype(dtype) + dtype(0.5)) - dtype(0.5), dtype(0.0))
    i0 = np.minimum(f.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = f - i0.astype(dtype)
    l0 = dtype(1.0) - l1
    assert f.dtype == dtype and l0.dtype == dtype
    return i0, i1, l0, l1


def upsample(x, H, W, dtype=F32):
    """x [C,h,w] -> v [C,H,W]: v = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11), every operation rounded to dtype"""
    x = np.asarray(x).astype(dtype)
    y0, y1, ly0, ly1 = taps(x.shape[1], H, dtype)
    x0, x1, lx0, lx1 = taps(x.shape[2], W, dtype)
    top, bot = x[:, y0], x[:, y1]
    v = ly0[None, :, None] * (lx0 * top[:, :, x0] + lx1 * top[:, :, x1]) + ly1[None, :, None] * (lx0 * bot[:, :, x0] + lx1 * bot[:, :, x1])
    assert v.dtype == dtype
    return v


def first_argmax(v):
    """[C,H,W] -> uint8 [H,W]: the first channel with the largest value (np.argmax returns the first maximum)"""
    return np.argmax(v, axis=0).astype(np.uint8)


def image_ok(offsets, sizes, b, max_h, max_w):
    H, W = int(sizes[b][0]), int(sizes[b][1])
    return 1 <= H <= max_h and 1 <= W <= max_w and int(offsets[b]) >= 0 and int(offsets[b + 1]) - int(offsets[b]) >= H * W


def native_eval(x, data, offsets, sizes, max_h, max_w, ignore, fill=0xA5):
    """x [B,C,h,w] (values exact in fp32); data: the label bytes, offsets int64 [B+1], sizes [B][2] as the ABI takes them.  Returns
    pred (a list of uint8 [H_b,W_b], None for a refused image), classes (uint8 like data: pred in every accepted image's span, `fill`
    everywhere else), img_counts int32 [B,3,C], confusion int64 [C+1,C] of this call alone, valid uint8 [B]."""
    x = np.asarray(x)
    B, C = x.shape[:2]
    data = np.asarray(data, np.uint8)
    img_counts = np.zeros((B, 3, C), np.int32)
    confusion = np.zeros((C + 1, C), np.int64)
    valid = np.zeros(B, np.uint8)
    classes = np.full(data.shape, fill, np.uint8)
    preds = []
    for b in range(B):
        if not image_ok(offsets, sizes, b, max_h, max_w):
            preds.append(None)
            continue
        valid[b] = 1
        H, W, off = int(sizes[b][0]), int(sizes[b][1]), int(offsets[b])
        pred = first_argmax(upsample(x[b], H, W))
        lab = data[off:off + H * W].reshape(H, W).astype(np.int64)
        counted = (lab != ignore) & (lab < C)
        row = np.where(counted, lab, C)
        np.add.at(confusion, (row.reshape(-1), pred.reshape(-1).astype(np.int64)), 1)
        img_counts[b, 1] = np.bincount(pred.reshape(-1), minlength=C)
        img_counts[b, 2] = np.bincount(lab[counted], minlength=C)
        img_counts[b, 0] = np.bincount(lab[counted & (lab == pred)], minlength=C)
        classes[off:off + H * W] = pred.reshape(-1)
        preds.append(pred)
    return {"pred": preds, "classes": classes, "img_counts": img_counts, "confusion": confusion, "valid": valid}


def grid_logits(B, C, h, w, seed=0):
    """logits on a grid of 1/4 after a ReLU, exact in fp16: interpolated at power-of-two scale factors every operation of the rule is
    exact, and exact ties at the top are common (whole zero pixels, repeated maxima)"""
    rng = np.random.default_rng(seed + 1000 * C + h * w)
    x = np.maximum(rng.integers(-6, 9, (B, C, h, w)) / 4.0, 0.0)
    x[:, :, ::3, ::2] = 0.0                                    # all-zero pixels: class 0 wins
    return x.astype(F32)


def top_ties(v):
    """number of pixels of v [C,H,W] whose largest value is held by more than one channel"""
    return int(((v == v.max(axis=0, keepdims=True)).sum(axis=0) > 1).sum())
