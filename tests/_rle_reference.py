"""Naive restatement of the COCO run-length format (include/maskunet_hip.h, "COCO run-length masks"; the published maskApi.c: rleEncode,
rleDecode, rleToString, rleFrString, rleArea), loop by loop from the rules.  It uses nothing of maskunet_amd.

  * a mask [H,W] is read column-major: position j = x * H + y, N = H * W;
  * counts: lengths of alternating runs, the first a run of zeros (possibly 0 long); an empty mask is [N];
  * string: count i gives x = counts[i] (i > 2: counts[i] - counts[i-2]); repeat c = x & 0x1f, x >>= 5 (arithmetic),
    more = (x != -1 if c & 0x10 else x != 0), emit chr(48 + (c | 0x20 if more else c)) until more is false;
  * area: the sum of the odd-indexed counts.
"""
import numpy as np


def encode(mask):
    """counts of a boolean mask [H,W]: one walk over the positions"""
    H, W = mask.shape
    counts, run, value = [], 0, False
    for x in range(W):
        for y in range(H):
            v = bool(mask[y, x])
            if v != value:
                counts.append(run)
                run, value = 0, v
            run += 1
    counts.append(run)
    return counts


def encode_fast(mask):
    """the same counts, vectorised: the host path that encoding on the device replaces (used for timing and checked against encode)"""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    bounds = np.flatnonzero(flat[1:] != flat[:-1]) + 1          # the value changes between positions j - 1 and j
    first = [0, 0] if flat[0] else [0]                          # a mask that starts with a one: a boundary at 0, a leading count of 0
    return np.diff(np.concatenate((first, bounds, [flat.size]))).tolist()


def string(counts):
    out = []
    for i in range(len(counts)):
        x = int(counts[i])
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def parse(s):
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = (c & 0x20) != 0
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def is_valid(counts, H, W):
    return all(c >= 0 for c in counts) and sum(counts) == H * W


def decode(counts, H, W):
    """boolean mask [H,W], or None for counts that are negative or do not sum to H*W"""
    if not is_valid(counts, H, W):
        return None
    flat = np.zeros(H * W, bool)
    j, value = 0, False
    for c in counts:
        for _ in range(c):
            flat[j] = value
            j += 1
        value = not value
    return flat.reshape(W, H).T.copy()


def area(counts):
    return sum(counts[1::2])


def encode_batch(ids, sel, max_id):
    """mu_rle_encode on the host: ids [B,H,W], sel [B,K] -> dict of the five outputs in the layout of the C ABI (L = 2*H*W + K)"""
    B, H, W = ids.shape
    K = sel.shape[1]
    L = 2 * H * W + K
    out = {"offsets": np.zeros((B, K + 1), np.int32), "counts": np.zeros((B, L), np.int32), "area": np.zeros((B, K), np.int32),
           "str_offsets": np.zeros((B, K + 1), np.int32), "str_bytes": np.zeros((B, 4 * L), np.uint8)}
    for b in range(B):
        o = so = 0
        for k in range(K):
            s = int(sel[b, k])
            if 1 <= s <= max_id:
                first = [int(v) for v in sel[b, :k]]
                c = encode((ids[b] == s) if s not in first else np.zeros((H, W), bool))
                t = string(c).encode("ascii")
                out["counts"][b, o:o + len(c)] = c
                out["str_bytes"][b, so:so + len(t)] = np.frombuffer(t, np.uint8)
                out["area"][b, k] = area(c)
                o += len(c)
                so += len(t)
            out["offsets"][b, k + 1] = o
            out["str_offsets"][b, k + 1] = so
    return out


def decode_batch(offsets, counts, H, W):
    """mu_rle_decode on the host -> (ids int32 [B,H,W], valid int32 [B,K])"""
    B, K = offsets.shape[0], offsets.shape[1] - 1
    ids = np.zeros((B, H, W), np.int32)
    valid = np.zeros((B, K), np.int32)
    for b in range(B):
        for k in range(K):
            o0, o1 = int(offsets[b, k]), int(offsets[b, k + 1])
            if not 0 <= o0 <= o1 <= counts.shape[1]:
                continue
            m = decode([int(v) for v in counts[b, o0:o1]], H, W)
            if m is None:
                continue
            valid[b, k] = 1
            ids[b][m] = np.maximum(ids[b][m], k + 1)
    return ids, valid
