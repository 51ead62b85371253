"""COCO run-length masks, encoded and decoded on the device.

Every prediction leaves the reference's evaluation scripts as a pycocotools RLE (mask_to_rle / maskUtils.encode: city_instance.py:399-403,
city_panoptic.py:176-181, coco_instance.py:351,397), and COCO ground truth arrives as one (annToMask, coco_instance.py:63).  Here an id
map stays on the device: mu_rle_encode turns the selected instances of every image into counts, areas and the compressed strings in one
pass, and mu_rle_decode paints a list of RLEs back into an id map -- the input of match_instances / mu_instance_pairs.

The format is restated from the published maskApi.c (rleEncode, rleDecode, rleToString, rleFrString, rleArea), NOT pinned to pycocotools
(which is not available where this project is tested):
  * a mask [H,W] is read column-major: position j = x * H + y, N = H * W;
  * counts are the lengths of alternating runs, starting with a run of zeros that may be 0 long; an empty mask is [N];
  * the string holds, count by count, x = counts[i] (for i > 2: counts[i] - counts[i-2]) in groups of 5 bits, lowest first:
    c = x & 0x1f, x >>= 5, more = (x != -1 if c & 0x10 else x != 0), chr(48 + (c | 0x20 if more else c));
  * area is the sum of the odd-indexed counts.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._lib import call, ptr, stream


def rle_string_from_counts(counts) -> str:
    """rleToString on the host: the compressed `counts` string of a COCO RLE."""
    out = []
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        while True:
            c5 = x & 0x1f
            x >>= 5
            more = (x != -1) if (c5 & 0x10) else (x != 0)
            if more:
                c5 |= 0x20
            out.append(chr(c5 + 48))
            if not more:
                break
    return "".join(out)


def rle_counts_from_string(s) -> list:
    """rleFrString on the host: the integer counts of a compressed `counts` string (str or bytes)."""
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts, p = [], 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            if p >= len(data):
                raise ValueError("RLE string ends inside a count")
            c = data[p] - 48
            if not 0 <= c < 64:
                raise ValueError(f"character {chr(data[p])!r} is not part of an RLE string")
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


@dataclass
class RLEs:
    """Device tensors of one encode_rle call; L = 2 * H * W + K.  Row k of image b holds counts[b, offsets[b,k]:offsets[b,k+1]] and the
    string str_bytes[b, str_offsets[b,k]:str_offsets[b,k+1]]; a row whose `sel` was 0 (or outside 1..max_id) is empty, and everything
    past the used part is zero."""
    offsets: torch.Tensor        # int32 [B,K+1]
    counts: torch.Tensor         # int32 [B,L]
    area: torch.Tensor           # int32 [B,K]
    str_offsets: torch.Tensor    # int32 [B,K+1]
    str_bytes: torch.Tensor      # uint8 [B,4*L]
    height: int
    width: int

    def to_coco(self, image, keep_empty=False):
        """[{"size": [H, W], "counts": str}] of the non-empty rows of one image, in row order (keep_empty: None in the place of an empty
        row).  Copies the row offsets and the used bytes to the host: the only synchronisation."""
        so = self.str_offsets[image].cpu().tolist()
        data = bytes(self.str_bytes[image, :so[-1]].cpu().numpy())
        out = []
        for k in range(len(so) - 1):
            if so[k + 1] > so[k]:
                out.append({"size": [self.height, self.width], "counts": data[so[k]:so[k + 1]].decode("ascii")})
            elif keep_empty:
                out.append(None)
        return out

    def counts_list(self, image, keep_empty=False):
        """the integer counts of the non-empty rows of one image, in row order (keep_empty: [] in the place of an empty row)"""
        o = self.offsets[image].cpu().tolist()
        c = self.counts[image, :o[-1]].cpu().tolist()
        return [c[o[k]:o[k + 1]] for k in range(len(o) - 1) if keep_empty or o[k + 1] > o[k]]


def encode_rle(ids, sel, max_id=None) -> RLEs:
    """Row k of image b is the RLE of the mask ids[b] == sel[b, k].  ids: int32 [B,H,W] on the GPU (Instances.ids or any id map); sel:
    int32 [B,K], its non-zero ids distinct within an image; 0 or an id outside 1..max_id (default H*W, which no connected-component id
    exceeds) gives an empty row, an id that does not occur the empty mask [H*W].  Never synchronises."""
    if ids.dim() != 3 or sel.dim() != 2 or ids.dtype != torch.int32 or sel.dtype != torch.int32 or ids.shape[0] != sel.shape[0]:
        raise RuntimeError("encode_rle expects ids int32 [B,H,W] and sel int32 [B,K]")
    B, H, W = ids.shape
    K = sel.shape[1]
    max_id = H * W if max_id is None else int(max_id)
    lib = _lib.load()
    ids, sel = ids.contiguous(), sel.contiguous()
    p_ids, p_sel = ptr(ids), ptr(sel)                  # CPU tensors raise here
    if B < 1 or lib.mu_rle_encode_supported(H, W, K, max_id) != 0:
        raise RuntimeError(f"maskunet_amd: mu_rle_encode failed with MU_ERR_SHAPE: RLE encoding needs H*W <= 65536, 1 <= K <= 4096 and "
                           f"1 <= max_id <= 65536, got {H}x{W}, K={K}, max_id={max_id}")
    dev, i32 = ids.device, torch.int32
    L = 2 * H * W + K
    r = RLEs(torch.empty((B, K + 1), dtype=i32, device=dev), torch.empty((B, L), dtype=i32, device=dev),
             torch.empty((B, K), dtype=i32, device=dev), torch.empty((B, K + 1), dtype=i32, device=dev),
             torch.empty((B, 4 * L), dtype=torch.uint8, device=dev), H, W)
    ws = torch.empty(lib.mu_rle_encode_workspace_bytes(B, H, W, K, max_id), dtype=torch.uint8, device=dev)
    call("mu_rle_encode", p_ids, p_sel, B, H, W, K, max_id, ptr(r.offsets), ptr(r.counts), ptr(r.area), ptr(r.str_offsets),
         ptr(r.str_bytes), ptr(ws), ws.numel(), stream())
    return r


def _host_rows(images, H, W):
    """list (images) of lists (rows) of COCO RLE dicts -> offsets [B,K+1], counts [B,Lc] on the host"""
    K = max(max((len(rows) for rows in images), default=0), 1)
    parsed = []
    for rows in images:
        per = []
        for d in rows:
            if list(d["size"]) != [H, W]:
                raise ValueError(f"RLE of size {list(d['size'])} in an image of {[H, W]}")
            c = d["counts"]
            per.append(rle_counts_from_string(c) if isinstance(c, (str, bytes)) else [int(v) for v in c])
        parsed.append(per)
    Lc = max(max((sum(len(c) for c in per) for per in parsed), default=0), 1)
    offsets = torch.zeros((len(parsed), K + 1), dtype=torch.int32)
    counts = torch.zeros((len(parsed), Lc), dtype=torch.int32)
    for b, per in enumerate(parsed):
        o = 0
        for k in range(K):
            if k < len(per):
                counts[b, o:o + len(per[k])] = torch.tensor(per[k], dtype=torch.int64).clamp_(-1, 2 ** 31 - 1).to(torch.int32)
                o += len(per[k])
            offsets[b, k + 1] = o
    return offsets, counts


def decode_rle(rles, H, W, device=None):
    """(ids int32 [B,H,W], valid int32 [B,K]) of `rles`: an RLEs, a list of COCO RLE dicts (one image; `counts` a string or a list of
    integers) or a list of such lists (a batch).  ids holds the largest row number + 1 among the rows that cover a pixel, else 0 --
    the id map match_instances takes; valid is 1 for the rows whose counts are non-negative and sum to H*W, the others paint nothing."""
    H, W = int(H), int(W)
    if isinstance(rles, RLEs):
        if (rles.height, rles.width) != (H, W):
            raise ValueError(f"RLEs of size {[rles.height, rles.width]} decoded as {[H, W]}")
        offsets, counts = rles.offsets, rles.counts
    else:
        images = [rles] if (len(rles) == 0 or isinstance(rles[0], dict)) else list(rles)
        offsets, counts = _host_rows(images, H, W)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("maskunet_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")
        offsets, counts = offsets.to(dev), counts.to(dev)
    B, K = offsets.shape[0], offsets.shape[1] - 1
    lib = _lib.load()
    p_off, p_cnt = ptr(offsets), ptr(counts)
    if B < 1 or lib.mu_rle_decode_supported(H, W, K) != 0:
        raise RuntimeError(f"maskunet_amd: mu_rle_decode failed with MU_ERR_SHAPE: RLE decoding needs H*W <= 65536 and 1 <= K <= 4096, "
                           f"got {H}x{W}, K={K}")
    ids = torch.empty((B, H, W), dtype=torch.int32, device=offsets.device)
    valid = torch.empty((B, K), dtype=torch.int32, device=offsets.device)
    call("mu_rle_decode", p_off, p_cnt, B, H, W, K, counts.shape[1], ptr(ids), ptr(valid), stream())
    return ids, valid
