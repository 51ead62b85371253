"""CPU reference of the instance-extraction contract (maskunet_amd.instances), in plain numpy, plus the label patterns that the
host and the GPU tests share.  Written from the contract, not from the kernels:

  - class 0 and negative values are background; an instance is a maximal 8-connected set of pixels of one non-zero class;
  - ids run 1..count per image in raster order of each instance's first pixel;
  - table row k-1 = class, area, x_min, y_min, x_max, y_max, first_pixel (y*W+x), class_rank (1-based rank among the instances of the
    same class in id order); score = mean of prob over the instance's pixels (1.0 without prob);
  - order = ids by descending score, ties by ascending id; table / score / order hold ids 1..min(count, max_instances), the rest is 0.
"""
import numpy as np

from tests._instances_reference import table_from_ids

NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def label_image(cls):
    """ids [H,W] int32 and the list of per-instance pixel index arrays (raster order of the first pixel)."""
    H, W = cls.shape
    ids = np.zeros((H, W), np.int32)
    regions = []
    for y0 in range(H):
        for x0 in range(W):
            c = cls[y0, x0]
            if c <= 0 or ids[y0, x0]:
                continue
            k = len(regions) + 1
            ids[y0, x0] = k
            stack, pix = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                pix.append(y * W + x)
                for dy, dx in NEIGHBOURS:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and cls[yy, xx] == c and not ids[yy, xx]:
                        ids[yy, xx] = k
                        stack.append((yy, xx))
            regions.append(np.sort(np.asarray(pix, np.int64)))
    return ids, regions


def instances(cls, prob=None, max_instances=1024):
    """cls [B,H,W] ints, prob [B,H,W] float64 or None -> dict of ids, count, table, score (float64), order."""
    cls = np.asarray(cls)
    ids = np.zeros(cls.shape, np.int32)
    classes, scores = [], None if prob is None else []
    for b in range(cls.shape[0]):
        ids[b], regions = label_image(cls[b])
        classes.append([int(cls[b].reshape(-1)[pix[0]]) for pix in regions])
        if prob is not None:
            p = np.asarray(prob[b], np.float64).reshape(-1)
            scores.append([float(p[pix].mean()) for pix in regions[:max_instances]])
    return {"ids": ids, **table_from_ids(ids, classes, max_instances, scores)}


def class_rank_mask(cls, max_instances=1024):
    """generate_instance_mask of the contract: per pixel the class_rank of its instance, 0 background, -1 past max_instances."""
    r = instances(cls, None, max_instances)
    out = np.zeros_like(r["ids"])
    for b in range(cls.shape[0]):
        lut = np.concatenate([[0], r["table"][b, :, 7], np.full(max(int(r["count"][b]) - max_instances, 0), -1)]).astype(np.int32)
        out[b] = lut[r["ids"][b]]
    return out


def argmax_prob(logits, temperature=0.5):
    """logits [..., C] -> (first arg-max over the last axis, float64 soft-max probability of that class)."""
    x = np.asarray(logits, np.float64) / temperature
    m = x.max(-1, keepdims=True)
    return x.argmax(-1).astype(np.int32), 1.0 / np.exp(x - m).sum(-1)


# ------------------------------------------------------------------------------------------------
# label patterns: the smallest shapes at which a labeller goes wrong
def _serpentine(n):
    g = np.zeros((n, n), np.int32)
    g[0::2] = 1
    g[1::4, n - 1] = 1
    g[3::4, 0] = 1
    return g


def _spirals(n):
    g = np.full((n, n), 2, np.int32)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and g[ny, nx] == 2 and not (0 <= ny2 < n and 0 <= nx2 < n and g[ny2, nx2] == 1):
                y, x = ny, nx
                g[y, x] = 1
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return g


def patterns():
    """name -> int32 [H,W]"""
    rng = np.random.default_rng(1)
    p = {}
    for h, w in [(1, 1), (1, 7), (7, 1), (5, 3), (37, 29), (63, 65)]:
        p[f"odd_{h}x{w}"] = rng.integers(0, 3, (h, w)).astype(np.int32)
    p["odd_1x1_set"] = np.ones((1, 1), np.int32)
    p["background"] = np.zeros((16, 16), np.int32)
    p["negative_is_background"] = np.where(np.arange(64).reshape(8, 8) % 3 == 0, -1, 0).astype(np.int32)
    p["full_256"] = np.full((256, 256), 7, np.int32)
    d = np.zeros((32, 32), np.int32)
    d[np.arange(32), np.arange(32)] = 1
    d[np.arange(32), 31 - np.arange(32)] = 2
    p["diagonals"] = d
    yy, xx = np.mgrid[0:16, 0:16]
    p["checker_two_classes"] = (1 + (xx + yy) % 2).astype(np.int32)
    p["checker_vs_background"] = ((xx + yy) % 2).astype(np.int32)
    comb = np.zeros((32, 32), np.int32)
    comb[:, 0::2] = 1
    comb[31, :] = 1
    p["comb"] = comb
    yy, xx = np.mgrid[0:33, 0:33]
    p["rings"] = (1 + np.maximum(abs(yy - 16), abs(xx - 16)) % 2).astype(np.int32)
    p["serpentine_32"] = _serpentine(32)
    p["serpentine_128"] = _serpentine(128)
    p["spirals"] = _spirals(31)
    yy, xx = np.mgrid[0:16, 0:16]
    p["isolated"] = (1 + xx % 2 + 2 * (yy % 2)).astype(np.int32)
    return p


EXPECTED_COUNTS = {"background": 0, "negative_is_background": 0, "full_256": 1, "diagonals": 2, "checker_two_classes": 2,
                   "checker_vs_background": 1, "comb": 1, "serpentine_32": 1, "serpentine_128": 1, "isolated": 256, "odd_1x1_set": 1,
                   # random_maps(), counted with scipy.ndimage.label: a changed generator shows here
                   "rand_16x16_c3": 29, "rand_37x29_c5": 340, "blocky_128_c19": 195, "blocky_256_c133": 998}


def blocky(rng, h, w, n_classes, block=8):
    """random classes 0..n_classes-1 in block x block squares"""
    small = rng.integers(0, n_classes, ((h + block - 1) // block, (w + block - 1) // block))
    return np.kron(small, np.ones((block, block), np.int64))[:h, :w].astype(np.int32)


def random_maps():
    """name -> (int32 [H,W], max_instances); generator default_rng(0), drawn in this order"""
    rng = np.random.default_rng(0)
    m = {}
    m["rand_16x16_c3"] = (rng.integers(0, 3, (16, 16)).astype(np.int32), 1024)
    m["rand_37x29_c5"] = (rng.integers(0, 5, (37, 29)).astype(np.int32), 1024)
    m["blocky_128_c19"] = (blocky(rng, 128, 128, 19), 1024)
    m["blocky_256_c133"] = (blocky(rng, 256, 256, 133), 2048)
    return m
