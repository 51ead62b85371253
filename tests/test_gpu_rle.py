"""GPU: COCO run-length masks on the device (mu_rle_encode, mu_rle_decode, maskunet_amd.rle) against the naive restatement of the format in
tests/_rle_reference.py.  The feature is integer-exact: every output -- offsets, counts, their zero tail, area, string offsets, string bytes
and their zero tail, decoded ids, valid -- is compared with ==.  Raw id maps go through the C ABI.  Memory discipline as in
test_gpu_match.py: outputs pre-filled with a sentinel, the workspace exactly the queried size, 4 KiB guard bands around every buffer,
inputs verified untouched."""
import functools

import numpy as np
import pytest
import torch

from tests import _rle_reference as R
from tests._device_buffers import Guarded, call

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENC_KEYS = ("offsets", "counts", "area", "str_offsets", "str_bytes")
MU_ERR_SHAPE = -2


def run_encode(ids, sel, max_id):
    """raw mu_rle_encode -> dict of numpy outputs"""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, H, W = ids.shape
    K, L = sel.shape[1], 2 * H * W + sel.shape[1]
    i32, u8 = torch.int32, torch.uint8
    g_ids, g_sel = Guarded(B * H * W, i32, ids, "ids"), Guarded(B * K, i32, sel, "sel")
    shapes = {"offsets": ((B, K + 1), i32), "counts": ((B, L), i32), "area": ((B, K), i32), "str_offsets": ((B, K + 1), i32),
              "str_bytes": ((B, 4 * L), u8)}
    outs = {k: Guarded(int(np.prod(s)), d, name=k) for k, (s, d) in shapes.items()}
    assert lib.mu_rle_encode_supported(H, W, K, max_id) == 0
    nws = lib.mu_rle_encode_workspace_bytes(B, H, W, K, max_id)
    assert nws > 0 and nws % 4 == 0
    call("mu_rle_encode", g_ids, g_sel, B, H, W, K, max_id, *[outs[k] for k in ENC_KEYS], Guarded(nws // 4, i32, name="workspace"), nws)
    return {k: outs[k].host(shapes[k][0]) for k in ENC_KEYS}


def run_decode(offsets, counts, H, W):
    """raw mu_rle_decode -> (ids, valid)"""
    from maskunet_amd import _lib
    lib = _lib.load()
    B, K, Lc = offsets.shape[0], offsets.shape[1] - 1, counts.shape[1]
    i32 = torch.int32
    g_off, g_cnt = Guarded(B * (K + 1), i32, offsets, "offsets"), Guarded(B * Lc, i32, counts, "counts")
    g_ids, g_valid = Guarded(B * H * W, i32, name="ids"), Guarded(B * K, i32, name="valid")
    assert lib.mu_rle_decode_supported(H, W, K) == 0
    call("mu_rle_decode", g_off, g_cnt, B, H, W, K, Lc, g_ids, g_valid)
    return g_ids.host((B, H, W)), g_valid.host((B, K))


def restricted(ids, sel, max_id):
    """ids restricted to sel and renumbered by row: what decode(encode(ids, sel)) must give"""
    out = np.zeros_like(ids)
    for b in range(ids.shape[0]):
        seen = set()
        for k, s in enumerate(sel[b].tolist()):
            if 1 <= s <= max_id and s not in seen:
                out[b][ids[b] == s] = k + 1
                seen.add(s)
    return out


def check(ids, sel, max_id=None):
    """encode against the reference, key by key; decode of the result against the reference decoder and against the id map itself"""
    ids, sel = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(sel, np.int32)
    B, H, W = ids.shape
    max_id = H * W if max_id is None else max_id
    ref = R.encode_batch(ids, sel, max_id)
    got = run_encode(ids, sel, max_id)
    print(f"{H}x{W} K={sel.shape[1]}: counts per image {got['offsets'][:, -1].tolist()} (reference {ref['offsets'][:, -1].tolist()}), "
          f"characters {got['str_offsets'][:, -1].tolist()} (reference {ref['str_offsets'][:, -1].tolist()})")
    for k in ENC_KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), k
    dec_ids, dec_valid = run_decode(got["offsets"], got["counts"], H, W)
    ref_ids, ref_valid = R.decode_batch(ref["offsets"], ref["counts"], H, W)
    assert np.array_equal(dec_valid, ref_valid) and np.array_equal(dec_ids, ref_ids)
    in_range = (sel >= 1) & (sel <= max_id)
    assert np.array_equal(dec_valid, in_range.astype(np.int32))
    assert np.array_equal(dec_ids, restricted(ids, sel, max_id))
    return got


def blocky(seed, B, H, W, n_ids, bs):
    """random id maps of bs x bs blocks with ids 0..n_ids (0 = background); regions need not be connected"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, n_ids + 1, size=(B, -(-H // bs), -(-W // bs)))
    return np.kron(small, np.ones((bs, bs), np.int64))[:, :H, :W].astype(np.int32)


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 7), (7, 5), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_ids_k_below_equal_above(shape):
    """5x7 against 7x5: a transposed walk passes every square case"""
    H, W = shape
    ids = blocky(11 * H + W, 2, H, W, 4, 1)
    present = max(len(np.unique(ids[ids > 0])), 1)
    for K in sorted({max(present - 2, 1), present, present + 3}):
        sel = np.stack([np.arange(1, K + 1), np.arange(K, 0, -1)]).astype(np.int32)
        check(ids, sel)


# edges of the shared wave / workgroup helpers (csrc/wave_prims.h), as in test_gpu_instances.py
EDGE_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (7, 73), (16, 32), (19, 27), (31, 33), (32, 32), (25, 41)]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixel_counts_at_chunk_and_segment_edges(shape):
    """per-pixel noise.  The 8 waves share the boundaries 0..N of the column-major walk in 64-boundary chunks: foreground is forced on the
    last position and on the first position of the last wave's segment (image 0: whatever row is there; image 1: a row of their own)"""
    H, W = shape
    N = H * W
    seg = -(-(N + 1) // 512) * 64
    ids = blocky(N, 2, H, W, 3, 1)
    for j in (min(N // seg * seg, N - 1), N - 1):          # position j of the walk = column j // H, line j % H
        ids[0, j % H, j // H] = max(ids[0, j % H, j // H], 1)
        ids[1, j % H, j // H] = 4
    check(ids, np.array([[1, 2, 3, 4], [4, 3, 2, 1]], np.int32))


@pytest.mark.parametrize("K", [63, 64, 65, 129])
def test_row_counts_across_the_scan_turns(K):
    """offsets and string offsets are scanned 64 rows per turn: a few real rows at the turn's edges, the others empty (image 0: pad
    rows, no counts at all; image 1: absent ids, one count each)"""
    ids = blocky(K, 2, 16, 16, 5, 4)
    sel = np.stack([np.zeros(K, np.int32), 100 + np.arange(K, dtype=np.int32)])
    for n, k in enumerate(k for k in (0, 62, 63, 64, 128) if k < K):
        sel[:, k] = 1 + n
    got = check(ids, sel, max_id=256)
    assert got["offsets"][1, -1] >= K


def test_sixty_four_rows_in_one_chunk():
    """the counting sort by row: 64 single-pixel rows on an 8 x 8 image, so the one chunk of boundaries holds every row twice"""
    ids = (1 + np.random.default_rng(6).permutation(64)).reshape(1, 8, 8).astype(np.int32)
    got = check(ids, np.arange(64, 0, -1, dtype=np.int32)[None])
    assert got["area"].tolist() == [[1] * 64]


def test_one_pixel_image_both_values():
    got = check(np.array([[[3]], [[0]]], np.int32), np.array([[3], [3]], np.int32), max_id=5)
    assert got["counts"][:, :2].tolist() == [[0, 1], [1, 0]] and got["offsets"].tolist() == [[0, 2], [0, 1]]
    assert bytes(got["str_bytes"][0, :2]) == b"01" and bytes(got["str_bytes"][1, :1]) == b"1"


def test_hand_vectors_centre_pixel_and_empty_images():
    """the literal vectors of the contract: [4,1,4] = "414"; an empty 128 x 128 mask is [16384] = "PP`0", an empty 256 x 256 one
    [65536] = "PPP2"; a full 256 x 256 one [0, 65536] = "0PPP2" """
    ids = np.zeros((1, 3, 3), np.int32)
    ids[0, 1, 1] = 2
    got = check(ids, np.array([[2]], np.int32))
    assert got["counts"][0, :3].tolist() == [4, 1, 4] and bytes(got["str_bytes"][0, :3]) == b"414" and got["area"].tolist() == [[1]]
    got = check(np.zeros((1, 128, 128), np.int32), np.array([[7]], np.int32))
    assert got["counts"][0, :1].tolist() == [16384] and bytes(got["str_bytes"][0, :4]) == b"PP`0"
    ids = np.zeros((2, 256, 256), np.int32)
    ids[1] = 9
    got = check(ids, np.array([[9, 0], [9, 4]], np.int32), max_id=65536)
    assert got["offsets"].tolist() == [[0, 1, 1], [0, 2, 3]]
    assert got["counts"][0, :1].tolist() == [65536] and bytes(got["str_bytes"][0, :4]) == b"PPP2"
    assert got["counts"][1, :3].tolist() == [0, 65536, 65536] and bytes(got["str_bytes"][1, :9]) == b"0PPP2PPP2"
    assert got["area"].tolist() == [[0, 0], [65536, 0]]


def test_edges_of_the_walk_pads_and_orders():
    """an instance on position 0 (leading count 0), one on position N - 1 (no closing count), an absent id ([N]), pad rows between real
    rows, sel descending and shuffled, an id past max_id, an all-background image"""
    H, W = 16, 16
    ids = blocky(5, 3, H, W, 6, 4)
    ids[0, 0, 0] = 1                                     # position 0
    ids[0, H - 1, W - 1] = 2                             # position N - 1
    ids[0][ids[0] == 5] = 0                              # 5 is absent from image 0
    ids[2] = 0                                           # all background
    sel = np.array([[1, 0, 2, 0, 0, 5, 40, 3], [6, 5, 4, 3, 2, 1, 0, 0], [3, 1, 0, 2, 6, 0, 4, 5]], np.int32)
    got = check(ids, sel, max_id=30)
    o = got["offsets"][0]
    assert got["counts"][0, o[0]] == 0                               # row 0 starts on position 0
    assert (o[3] - o[2]) % 2 == 0                                    # row 2 ends on position N - 1: an even number of counts
    assert got["counts"][0, o[5]:o[6]].tolist() == [H * W]           # the absent id
    assert o[7] == o[6] and o[2] == o[1] and o[4] == o[3]            # 40 > max_id and the pads: empty rows
    assert got["offsets"][2].tolist() == [0, 1, 2, 2, 3, 4, 4, 5, 6] and set(got["counts"][2, :6].tolist()) == {H * W}
    shuffled = np.random.default_rng(1).permuted(sel, axis=1)
    assert not np.array_equal(shuffled, sel)
    check(ids, shuffled, max_id=30)


def test_full_image_instance():
    ids = np.full((1, 7, 5), 3, np.int32)
    got = check(ids, np.array([[1, 3]], np.int32))
    assert got["counts"][0, :3].tolist() == [35, 0, 35] and got["area"].tolist() == [[0, 35]]


@pytest.mark.parametrize("size", [16, 128])
def test_checkerboard_reaches_the_output_bound(size):
    """one id on a checkerboard: runs of one pixel inside every column (with an even side two neighbouring columns meet in a run of
    two, so the number of counts comes from the reference); below, the alternation along the whole walk: N counts of 1, and every
    value of the string is 0 from the fourth count on"""
    yy, xx = np.mgrid[0:size, 0:size]
    ids = (((yy + xx) % 2) * 4).astype(np.int32)[None]
    got = check(ids, np.array([[4]], np.int32))
    n = int(got["offsets"][0, 1])
    assert n > size * size // 2 and got["area"].tolist() == [[size * size // 2]]
    s = bytes(got["str_bytes"][0, :got["str_offsets"][0, 1]]).decode()
    assert R.parse(s) == got["counts"][0, :n].tolist()
    odd = ((np.arange(15 * 15).reshape(15, 15).T % 2) * 4).astype(np.int32)[None]          # value = parity of the position x * H + y
    got = check(odd, np.array([[4]], np.int32))
    assert got["offsets"][0, 1] == 15 * 15 and got["counts"][0, :225].tolist() == [1] * 225
    assert bytes(got["str_bytes"][0, :225]) == b"111" + b"0" * 222


@pytest.mark.parametrize("size", [16, 128])
def test_two_interleaved_ids(size):
    yy, xx = np.mgrid[0:size, 0:size]
    cols = (1 + xx % 2).astype(np.int32)[None]           # alternating columns: runs of H
    rows = (1 + yy % 2).astype(np.int32)[None]           # alternating rows: runs of one pixel, two events at every boundary
    got = check(np.concatenate([cols, rows]), np.array([[2, 1], [1, 2]], np.int32))
    assert got["offsets"][0].tolist() == [0, size, 2 * size + 1]
    assert got["offsets"][1, -1] == 2 * size * size + 1          # N + 1 and N counts: one below the 2 * N + K bound


def test_three_images_with_different_numbers_of_runs():
    """offsets must not leak across images: a fine map, a coarse map, an empty one"""
    H, W = 20, 24
    ids = np.concatenate([blocky(1, 1, H, W, 9, 1), blocky(2, 1, H, W, 9, 12), np.zeros((1, H, W), np.int32)])
    sel = np.tile(np.arange(1, 11, dtype=np.int32), (3, 1))
    got = check(ids, sel, max_id=9)
    totals = got["offsets"][:, -1].tolist()
    assert totals[0] > 4 * totals[1] > 0 and totals[2] == 9
    assert got["area"].sum(1).tolist() == [int((ids[b] > 0).sum()) for b in range(3)]


@pytest.mark.parametrize("size", [128, 256])
def test_limit_sizes_random_blocks(size):
    ids = blocky(size, 2, size, size, 5, 8 if size == 128 else 32)
    ids[1, -3:, -5:] = 2
    ids[1, :2, :1] = 4
    check(ids, np.array([[4, 0, 2, 6], [2, 4, 5, 1]], np.int32), max_id=65536 if size == 256 else None)


def test_many_rows_few_pixels_each():
    """K = 4096 rows (the LDS limit of the encoder) over a 64 x 64 map of 4096 single-pixel ids"""
    ids = (1 + np.random.default_rng(4).permutation(4096)).reshape(1, 64, 64).astype(np.int32)
    sel = np.arange(4096, 0, -1, dtype=np.int32)[None]
    got = run_encode(ids, sel, 4096)
    assert got["offsets"][0, -1] == 3 * 4096 - 1          # [j, 1, N - 1 - j]; the pixel on the last position has no closing count
    assert got["area"].tolist() == [[1] * 4096]
    dec_ids, dec_valid = run_decode(got["offsets"], got["counts"], 64, 64)
    assert dec_valid.all() and np.array_equal(dec_ids, 4097 - ids)
    o = got["offsets"][0]
    pos = ids[0].T.reshape(-1)                            # id at every position of the walk
    for k in (0, 1, 2047, 4095):
        j = int(np.flatnonzero(pos == sel[0, k])[0])
        want = [j, 1, 4095 - j] if j < 4095 else [j, 1]
        assert got["counts"][0, o[k]:o[k + 1]].tolist() == want


def test_decode_overlapping_invalid_and_foreign_rows():
    """annotation files may hold overlapping masks (the larger row wins), rows that do not cover the image, negative counts, zero-length
    runs in the middle, and more counts than an encoder would write"""
    H, W = 5, 7
    a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    a[1:4, 1:5] = True
    b[2:5, 3:7] = True
    rows = [R.encode(a), R.encode(b), [4, 1, 3], [36, -1], [3, 0, 0, 2, 30], [], [35], [0, 35]]
    rows[7] = [0, 20, 0, 0, 0, 15]                       # a full mask written with zero-length runs
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)[None]
    cnt = np.array([sum(rows, []) + [5, 5]], np.int32)
    ids, valid = run_decode(off, cnt, H, W)
    ref_ids, ref_valid = R.decode_batch(off, cnt, H, W)
    assert ref_valid.tolist() == [[1, 1, 0, 0, 1, 0, 1, 1]]
    assert np.array_equal(valid, ref_valid) and np.array_equal(ids, ref_ids) and (ids == 8).all()
    ids, valid = run_decode(off[:, :6], cnt, H, W)       # without the full row
    ref_ids, _ = R.decode_batch(off[:, :6], cnt, H, W)
    assert np.array_equal(ids, ref_ids) and ids[0, 3, 3] == 2 and ids[0, 1, 1] == 1 and ids[0, 3, 0] == 5 and ids[0, 0, 6] == 0
    bad = np.array([[0, 3, 2, 400, 401]], np.int32)      # offsets out of order and past the buffer: invalid, nothing is read there
    ids, valid = run_decode(bad, cnt, H, W)
    assert valid.tolist() == [[0, 0, 0, 0]] and not ids.any()


def test_two_runs_are_bit_identical():
    ids = blocky(8, 3, 20, 24, 9, 2)
    sel = np.tile(np.arange(9, 0, -1, dtype=np.int32), (3, 1))
    a, b = run_encode(ids, sel, 9), run_encode(ids, sel, 9)
    for k in ENC_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_unsupported_shapes_return_err_shape_without_a_launch():
    from maskunet_amd import _lib
    lib = _lib.load()
    i32 = torch.int32
    bufs = [Guarded(64, i32) for _ in range(7)] + [Guarded(64, torch.uint8)]
    ids, sel, off, cnt, area, soff, ws, sb = bufs
    for H, W, K, max_id in [(256, 257, 1, 1), (65537, 1, 1, 1), (4, 4, 0, 1), (4, 4, 4097, 1), (4, 4, 1, 0), (4, 4, 1, 65537)]:
        assert lib.mu_rle_encode_supported(H, W, K, max_id) == MU_ERR_SHAPE
        assert lib.mu_rle_encode_workspace_bytes(1, H, W, K, max_id) == 0
        rc = lib.mu_rle_encode(ids.p, sel.p, 1, H, W, K, max_id, off.p, cnt.p, area.p, soff.p, sb.p, ws.p, 1 << 40, _lib.stream())
        assert rc == MU_ERR_SHAPE, (H, W, K, max_id)
    for H, W, K in [(256, 257, 1), (4, 4, 0), (4, 4, 4097)]:
        assert lib.mu_rle_decode_supported(H, W, K) == MU_ERR_SHAPE
        assert lib.mu_rle_decode(off.p, cnt.p, 1, H, W, K, 64, ids.p, area.p, _lib.stream()) == MU_ERR_SHAPE
    assert lib.mu_rle_encode(ids.p, sel.p, 1, 4, 4, 1, 16, off.p, cnt.p, area.p, soff.p, sb.p, ws.p, 8, _lib.stream()) == -4
    torch.cuda.synchronize()
    for g in bufs:
        g.check("nothing may be written")
        assert bool((g.t == g.sent).all())
    assert lib.mu_rle_encode_supported(256, 256, 4096, 65536) == 0 and lib.mu_rle_decode_supported(256, 256, 4096) == 0


# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _logits(seed, B=2, C=5, H=32, W=32):
    from tests import _cc_reference as CC
    rng = np.random.default_rng(seed)
    labels = np.stack([CC.blocky(rng, H, W, C, 8) for _ in range(B)])
    x = 3.0 * np.eye(C)[labels].transpose(0, 3, 1, 2) + rng.standard_normal((B, C, H, W))
    x = (x + np.roll(x, 1, 2) + np.roll(x, 1, 3) + np.roll(x, -1, 2) + np.roll(x, -1, 3)) / 5
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def test_predictions_to_coco_against_the_reference_encoder():
    import maskunet_amd
    Q = 12
    pred = maskunet_amd.predict_instances(torch.from_numpy(_logits(12)).to(DEV), max_instances=256)
    rles = pred.rle(Q)
    assert rles.offsets.shape == (2, Q + 1) and rles.counts.shape == (2, 2 * 32 * 32 + Q)
    for b in range(2):
        ref = pred.to_reference(b, Q)
        assert 3 <= len(ref) <= Q
        coco = rles.to_coco(b)
        want = [{"size": [32, 32], "counts": R.string(R.encode(d["mask"]))} for d in ref]
        assert coco == want
        assert rles.counts_list(b) == [R.encode(d["mask"]) for d in ref]
        assert rles.area[b, :len(ref)].tolist() == [int(d["mask"].sum()) for d in ref]
        assert [maskunet_amd.rle_counts_from_string(c["counts"]) for c in coco] == rles.counts_list(b)
        assert len(rles.to_coco(b, keep_empty=True)) == Q
    full = pred.rle()                                     # every row of the table
    assert full.offsets.shape == (2, 257) and full.to_coco(0)[:len(rles.to_coco(0))] == rles.to_coco(0)
    # back: the id map of the kept instances, renumbered by rank, from the RLEs object and from the dictionaries
    ids, valid = maskunet_amd.decode_rle(rles, 32, 32)
    want = restricted(pred.ids.cpu().numpy(), pred.order[:, :Q].cpu().numpy(), 256)
    assert np.array_equal(ids.cpu().numpy(), want)
    assert np.array_equal(valid.cpu().numpy(), (pred.order[:, :Q] > 0).int().cpu().numpy())
    ids2, valid2 = maskunet_amd.decode_rle([rles.to_coco(0), rles.to_coco(1)], 32, 32)
    assert np.array_equal(ids2.cpu().numpy(), want) and bool(valid2[:, :3].all())
    one, _ = maskunet_amd.decode_rle([{"size": [32, 32], "counts": c} for c in rles.counts_list(1)], 32, 32)
    assert np.array_equal(one.cpu().numpy()[0], want[1])


def test_python_api_errors():
    import maskunet_amd
    ids = torch.zeros((1, 4, 4), dtype=torch.int32)
    sel = torch.ones((1, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        maskunet_amd.encode_rle(ids, sel)
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        maskunet_amd.encode_rle(torch.zeros((1, 256, 257), dtype=torch.int32, device=DEV), sel.to(DEV))
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        maskunet_amd.encode_rle(ids.to(DEV), torch.ones((1, 4097), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        maskunet_amd.encode_rle(ids.to(DEV), sel.to(DEV), max_id=65537)
    with pytest.raises(RuntimeError, match="int32"):
        maskunet_amd.encode_rle(ids.long().to(DEV), sel.to(DEV))
    with pytest.raises(ValueError, match="size"):
        maskunet_amd.decode_rle([{"size": [4, 5], "counts": "0"}], 4, 4)
    with pytest.raises(RuntimeError, match="MU_ERR_SHAPE"):
        maskunet_amd.decode_rle([{"size": [256, 257], "counts": [256 * 257]}], 256, 257)


def test_graph_capture_replayed_on_changed_inputs():
    import maskunet_amd
    H, W, K = 20, 24, 6
    maps = blocky(21, 3, H, W, 6, 3).reshape(3, 1, H, W)
    sels = np.array([[[1, 2, 3, 4, 5, 6]], [[6, 0, 4, 0, 2, 9]], [[3, 3, 1, 0, 0, 5]]], np.int32)
    ids = torch.from_numpy(maps[0]).to(DEV)
    sel = torch.from_numpy(sels[0]).to(DEV)
    eager = maskunet_amd.encode_rle(ids, sel, max_id=8)     # also the one-time set-up, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = maskunet_amd.encode_rle(ids, sel, max_id=8)
    for step in (1, 2, 0):
        ids.copy_(torch.from_numpy(maps[step]).to(DEV))
        sel.copy_(torch.from_numpy(sels[step]).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = maskunet_amd.encode_rle(ids, sel, max_id=8)
        ref = R.encode_batch(maps[step], sels[step], 8)
        for k in ENC_KEYS:
            assert torch.equal(getattr(captured, k), getattr(want, k)), (step, k)
            assert np.array_equal(getattr(captured, k).cpu().numpy(), ref[k]), (step, k)
    for k in ENC_KEYS:
        assert torch.equal(getattr(captured, k), getattr(eager, k)), k
