"""CPU restatement of the id-map instance contract (maskunet_amd.instances_from_id_map, mu_id_instances), in vectorised numpy, plus
the case generators that the host and the GPU tests share.  Written from the contract, not from the kernels:

  - per image: an id map v (any integers, or a uint8 [H,W,3] RGB image with v = R + 256 G + 65536 B) and a semantic map c;
  - a pixel with v != 0 is dropped (counts as v = 0) when c is outside [0, class_cap) (bit 0 of invalid) or v does not fit int32 (bit 1);
  - the distinct non-zero values in ascending signed order are v_1 < ... < v_count; id k = the pixels that hold v_k;
  - table row k-1 = class, area, x_min, y_min, x_max, y_max, first_pixel, class_rank for k <= K = min(count, max_instances), where
    class = (c_((n-1)//2) + c_(n//2)) // 2 over the instance's sorted semantic values (int(np.median(..)) for non-negative classes);
  - values row k-1 = v_k; score 1.0 and order 1..K over the first K rows; everything past K is 0; ids and count are complete.
"""
import numpy as np

from tests._instances_reference import table_from_ids

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def rgb2id(color):
    """panopticapi's published rgb2id on a uint8 [...,3] array"""
    c = np.asarray(color).astype(np.int64)
    return c[..., 0] + 256 * c[..., 1] + 65536 * c[..., 2]


def instances(id_map, sem, max_instances=1024, class_cap=256):
    """id_map [B,H,W] ints or uint8 [B,H,W,3], sem [B,H,W] ints -> dict of ids, count, table, score, order, values, invalid."""
    id_map, sem = np.asarray(id_map), np.asarray(sem)
    v_all = rgb2id(id_map) if id_map.ndim == 4 else id_map.astype(np.int64)
    B, H, W = sem.shape
    assert v_all.shape == (B, H, W)
    M = max_instances
    ids = np.zeros((B, H * W), np.int32)
    values = np.zeros((B, M), np.int32)
    invalid = np.zeros(B, np.int32)
    classes = []
    for b in range(B):
        v, c = v_all[b].reshape(-1), sem[b].reshape(-1).astype(np.int64)
        bad_c = (v != 0) & ((c < 0) | (c >= class_cap))
        bad_v = (v != 0) & ((v < I32_MIN) | (v > I32_MAX))
        invalid[b] = int(bad_c.any()) | (int(bad_v.any()) << 1)
        eff = np.where(bad_c | bad_v, 0, v)
        uniq, inverse = np.unique(eff, return_inverse=True)
        number = np.cumsum(uniq != 0)                      # ascending signed order, 0 left out
        number[uniq == 0] = 0
        ids[b] = number[inverse.reshape(-1)]
        distinct = uniq[uniq != 0]
        K = min(len(distinct), M)
        values[b, :K] = distinct[:K]
        pix = np.flatnonzero((ids[b] >= 1) & (ids[b] <= K))
        k = ids[b][pix].astype(np.int64) - 1
        area = np.bincount(k, minlength=K)
        cs = c[pix][np.lexsort((c[pix], k))]                # by instance, then by class
        start = np.cumsum(area) - area
        classes.append((cs[start + (area - 1) // 2] + cs[start + area // 2]) // 2)
    ids = ids.reshape(B, H, W)
    r = table_from_ids(ids, classes, M)
    return {"ids": ids, "count": r["count"], "table": r["table"], "score": r["score"].astype(np.float32), "order": r["order"],
            "values": values, "invalid": invalid}


# ------------------------------------------------------------------------------------------------
# cases: name -> (id_map, sem, max_instances, class_cap); id_map int64 [B,H,W] unless stated
def blocky(seed, B, H, W, bs=4, n_vals=10, class_cap=19, negative=True, noise=0.3):
    """piecewise-constant id maps: blocks of bs x bs draw from a pool of values (0 among them); the semantic map follows the value with
    `noise` of the pixels random, so medians are decided by counts"""
    rng = np.random.default_rng(seed)
    pool = [0, 0] + [int(c) * 1000 + int(k) for c, k in zip(rng.integers(0, class_cap, n_vals), rng.integers(0, 40, n_vals))]
    if negative:
        pool += [-1, -70000, I32_MIN, I32_MAX, 5]
    pool = np.asarray(pool, np.int64)
    gh, gw = -(-H // bs), -(-W // bs)
    v = np.stack([np.kron(pool[rng.integers(0, len(pool), (gh, gw))], np.ones((bs, bs), np.int64))[:H, :W] for _ in range(B)])
    base = (np.abs(v) // 1000) % class_cap
    sem = np.where(rng.random(v.shape) < noise, rng.integers(0, class_cap, v.shape), base).astype(np.int32)
    return v, sem


def distinct(seed, H, W):
    """every pixel its own id: distinct int32 values over the whole range, no zero (all four key bytes live)"""
    rng = np.random.default_rng(seed)
    v = np.unique(rng.integers(I32_MIN, I32_MAX, 2 * H * W, dtype=np.int64))
    v = rng.permutation(v[v != 0])[:H * W].reshape(1, H, W)
    return v, rng.integers(0, 19, v.shape).astype(np.int32)


def cityscapes_like():
    """32x32: instanceIds as the dataset writes them (class * 1000 + k for things, the bare class below 1000 for stuff), the ignore label
    255 inside instances, one instance in two pieces, two touching instances of one class"""
    v = np.zeros((32, 32), np.int64)
    sem = np.zeros((32, 32), np.int32)
    v[20:, :], sem[20:, :] = 7, 7                            # road (stuff)
    v[:6, :], sem[:6, :] = 23, 23                            # sky (stuff)
    v[6:20, :4], sem[6:20, :4] = 11, 11                      # building (stuff)
    v[10:18, 6:14], sem[10:18, 6:14] = 26001, 26             # two touching cars
    v[10:18, 14:20], sem[10:18, 14:20] = 26002, 26
    v[12:19, 22:25], sem[12:19, 22:25] = 26000, 26           # one car behind a pole: two pieces
    v[12:19, 26:30], sem[12:19, 26:30] = 26000, 26
    v[12:19, 25], sem[12:19, 25] = 17, 17
    v[7:10, 8:10], sem[7:10, 8:10] = 24000, 24               # a person
    sem[16:18, 6:14] = 255                                   # ignore inside 26001 (a minority: the median stays 26)
    sem[7:9, 8:10] = 255                                     # and the majority of 24000: the median is 255
    return v[None], sem[None]


def negative_even():
    """20x24: negative ids, even areas, two middle classes that differ"""
    rng = np.random.default_rng(3)
    v = np.zeros((20, 24), np.int64)
    sem = rng.integers(0, 19, (20, 24)).astype(np.int32)
    v[0:4, 0:6] = -5                                         # area 24: half class 2, half class 9 -> 5
    sem[0:4, 0:3], sem[0:4, 3:6] = 2, 9
    v[5:9, 2:10] = -70000                                    # area 32, random classes
    v[10:13, 0:5] = -1                                       # area 15 (odd)
    v[10:12, 8:9] = 3                                        # area 2: classes 3 and 18 -> 10
    sem[10, 8], sem[11, 8] = 18, 3
    v[14:20, 12:24] = 2000000000                             # area 72, random classes
    v[19, 0] = -2000000000                                   # area 1
    return v[None], sem[None]


def colour():
    """16x16 RGB image, ids above 65535 (blue channel in use)"""
    img = np.zeros((16, 16, 3), np.uint8)
    sem = np.zeros((16, 16), np.int32)
    img[1:6, 1:9], sem[1:6, 1:9] = (7, 1, 1), 4              # 65536 + 256 + 7
    img[1:6, 9:15], sem[1:6, 9:15] = (7, 1, 0), 4            # 263: the same low bytes, below 65536
    img[8:15, 2:7], sem[8:15, 2:7] = (0, 0, 255), 9          # 16711680
    img[8:15, 7:12], sem[8:15, 7:12] = (255, 255, 255), 11   # 16777215
    img[15, 15], sem[15, 15] = (0, 0, 1), 2                  # 65536 exactly
    sem[8:10, 2:7] = 13
    return img[None], sem[None]


GOLDEN = {"idmap_cityscapes_32x32": cityscapes_like, "idmap_negative_20x24": negative_even, "idmap_colour_16x16": colour}


def touching_and_split():
    """two touching cars (ids 26001, 26002) and one car in two pieces (26000), class 1, on 16x16; the rest is background"""
    v = np.zeros((1, 16, 16), np.int64)
    v[0, 2:8, 1:6] = 26001
    v[0, 2:8, 6:11] = 26002
    v[0, 10:14, 1:5] = 26000
    v[0, 10:14, 7:12] = 26000
    return v, (v != 0).astype(np.int32)


def things_case(seed, B, H, W, C, bs=6):
    """every bs x bs block its own instance, value class * 1000 + block number, classes 1..C-1; the semantic map is the class with a
    tenth of the pixels random.  Returns (id map, semantic map, the clean class map)."""
    rng = np.random.default_rng(seed)
    gh, gw = -(-H // bs), -(-W // bs)
    cls = rng.integers(1, C, (B, gh, gw))
    big = lambda a: np.kron(a, np.ones((bs, bs), np.int64))[:, :H, :W]
    labels = big(cls)
    v = labels * 1000 + big(np.arange(gh * gw).reshape(1, gh, gw).repeat(B, 0))
    sem = np.where(rng.random(v.shape) < 0.1, rng.integers(0, C, v.shape), labels)
    return v, sem.astype(np.int32), labels.astype(np.int32)


def rgb_of(v):
    v = np.asarray(v, np.int64)
    assert ((v >= 0) & (v < 1 << 24)).all()
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8)


def cases():
    out = {}
    one = lambda val, cls: (np.full((1, 1, 1), val, np.int64), np.full((1, 1, 1), cls, np.int32))
    out["1x1_zero"] = one(0, 3) + (4, 19)
    out["1x1_value"] = one(-9, 3) + (4, 19)
    for i, (H, W) in enumerate([(1, 7), (7, 1), (5, 3), (37, 29), (63, 65)]):
        out[f"blocky_{H}x{W}"] = blocky(10 + i, 1, H, W, bs=1 if H * W < 16 else 4) + (64, 19)
    out["one_id_256x256"] = (np.full((1, 256, 256), 26001, np.int64), np.full((1, 256, 256), 26, np.int32), 8, 256)
    out["batch_of_three"] = blocky(21, 3, 37, 29) + (64, 19)
    v = np.array([[I32_MIN, I32_MAX, -1, 1, 0, 1, -1, I32_MAX, I32_MIN]], np.int64)[None]
    out["extreme_keys"] = (v, np.arange(9, dtype=np.int32).reshape(1, 1, 9), 8, 19)
    rng = np.random.default_rng(31)
    top = (rng.integers(-128, 128, (1, 9, 11)).astype(np.int64)) << 24                  # only the top byte differs (0 among them)
    out["top_byte_only"] = (top, rng.integers(0, 19, top.shape).astype(np.int32), 256, 19)
    out["low_byte_only"] = (rng.integers(0, 256, (1, 9, 11)).astype(np.int64), rng.integers(0, 19, (1, 9, 11)).astype(np.int32), 256, 19)
    out["three_bytes_shared"] = (0x12345600 + rng.integers(0, 256, (1, 9, 11)).astype(np.int64),
                                 rng.integers(0, 19, (1, 9, 11)).astype(np.int32), 256, 19)
    out["zero_among_negatives"] = (np.array([[[-3, 0, 5, -1], [2, 2, 0, -3]]], np.int64), np.ones((1, 2, 4), np.int32), 8, 19)
    out["distinct_64x64"] = distinct(41, 64, 64) + (4096, 19)
    out["distinct_65x64"] = distinct(42, 65, 64) + (4096, 19)
    out["distinct_256x256_one_row"] = distinct(43, 256, 256) + (1, 19)
    out["split_and_touching"] = touching_and_split() + (8, 2)
    cols = np.tile(np.array([7, -7], np.int64), (1, 12, 8))                            # every pixel a run head
    out["alternating_columns"] = (cols, rng.integers(0, 19, cols.shape).astype(np.int32), 4, 19)
    yy, xx = np.mgrid[0:13, 0:15]
    board = np.where((yy + xx) % 2 == 0, 300, 70000).astype(np.int64)[None]
    out["checkerboard"] = (board, rng.integers(0, 19, board.shape).astype(np.int32), 4, 19)
    v = np.zeros((1, 4, 8), np.int64)
    sem = np.zeros((1, 4, 8), np.int32)
    v[0, 0, :4], sem[0, 0, :4] = 1, [13, 255, 14, 13]                                    # {13,13,14,255} -> 13
    v[0, 1, :2], sem[0, 1, :2] = 2, [255, 3]                                             # {3,255} -> 129
    v[0, 2, :4], sem[0, 2, :4] = 3, [0, 255, 255, 0]                                     # classes 0 and class_cap - 1 -> 127
    v[0, 3, 0], sem[0, 3, 0] = 4, 255                                                    # area 1
    v[0, 3, 2:5], sem[0, 3, 2:5] = 5, [9, 0, 4]                                          # odd area -> 4
    out["median_by_hand"] = (v, sem, 8, 256)
    out["median_1024_classes"] = (np.full((1, 256, 256), -12, np.int64), rng.integers(0, 1024, (1, 256, 256)).astype(np.int32), 2, 1024)
    v, _ = blocky(51, 1, 20, 24)
    out["class_cap_one"] = (v, np.zeros(v.shape, np.int32), 64, 1)
    return out


MEDIAN_BY_HAND = [13, 129, 127, 255, 4]


def invalid_case():
    """int64 ids, B = 3: image 0 has classes -1 and class_cap inside instances, image 1 is clean, image 2 holds ids outside int32"""
    v, sem = blocky(61, 3, 12, 16, class_cap=19, negative=False)
    v[0, 0:2, 0:4], v[0, 6:8, 0:4] = 4001, 4002
    sem[0, 0, 0:2], sem[0, 6, 0:4], sem[0, 7, 0:2] = -1, 19, 19                         # 4002 keeps two pixels
    v[2, 0, 0:3], v[2, 1, 0:3], v[2, 2, 0:2] = 2 ** 31, -2 ** 31 - 1, 2 ** 32            # the low word of 2^32 is 0
    v[2, 3, 0:3], v[2, 4, 0:3] = I32_MAX, I32_MIN
    return v, sem, 64, 19
