"""CPU: the numpy restatement of the cv2 loaders' target construction (tests/_targets_reference.py) against hand-computed cases, and the
host halves of maskunet_amd.targets: pack_maps' offsets and alignment for every kind, pack_segments' sorted, de-duplicated tables."""
import numpy as np
import pytest
import torch

from tests import _targets_reference as R


# ---- the restatement, by hand -----------------------------------------------------------------------------------------------------
def png_2x3():
    # ids:  7      7    300
    #       70000  0    300            300 = (44, 1, 0), 70000 = (112, 17, 1)
    rgb = np.zeros((2, 3, 3), np.uint8)
    rgb[0, 0] = rgb[0, 1] = (7, 0, 0)
    rgb[0, 2] = rgb[1, 2] = (44, 1, 0)
    rgb[1, 0] = (112, 17, 1)
    return rgb


def test_rgb2id_and_back():
    rgb = png_2x3()
    assert R.rgb2id(rgb).tolist() == [[7, 7, 300], [70000, 0, 300]]
    assert np.array_equal(R.id2rgb(R.rgb2id(rgb)), rgb)
    assert R.rgb2id(np.full((1, 1, 3), 255, np.uint8)).tolist() == [[16777215]]


def test_panoptic_targets_by_hand():
    # 300 is listed twice: the later entry (category 9) stays; 70000 is not listed: 0 / 0; 55 is listed but not in the PNG
    segs = [{"id": 300, "category_id": 4}, {"id": 7, "category_id": 2}, {"id": 55, "category_id": 3}, {"id": 300, "category_id": 9}]
    sem, inst = R.coco_panoptic_targets(png_2x3(), segs, (3, 2))
    assert sem.dtype == np.int64 and inst.dtype == np.int64
    assert sem.tolist() == [[2, 2, 9], [0, 0, 9]]
    assert inst.tolist() == [[7, 7, 300], [0, 0, 300]]
    # cat2label, and an upscale to 6 x 4: every source pixel becomes a 2 x 2 block (index floor(d * 0.5))
    sem, inst = R.coco_panoptic_targets(png_2x3(), segs, (6, 4), cat2label={4: 40, 2: 20, 3: 30, 9: 90})
    assert sem.tolist() == [[20, 20, 20, 20, 90, 90]] * 2 + [[0, 0, 0, 0, 90, 90]] * 2
    assert inst.tolist() == [[7, 7, 7, 7, 300, 300]] * 2 + [[0, 0, 0, 0, 300, 300]] * 2
    # id 0 is a segment like any other once it is listed
    sem, inst = R.coco_panoptic_targets(png_2x3(), [{"id": 0, "category_id": 5}], (3, 2))
    assert sem.tolist() == [[0, 0, 0], [0, 5, 0]] and not inst.any()
    with pytest.raises(KeyError):
        R.coco_panoptic_targets(png_2x3(), segs, (3, 2), cat2label={4: 1})


def test_labels_by_hand():
    m = np.array([[-1, -1000, -1001], [999, 1000, 26001]], np.int32)
    assert R.labels(m, (3, 2), divisor=1000).tolist() == [[-1, -1, -2], [0, 1, 26]]
    c = np.array([[0, 18, 19, 255]], np.uint8)
    assert R.labels(c, (4, 1), num_classes=19).tolist() == [[0, 18, 255, 255]]
    assert R.labels(m, (3, 2), divisor=1000, num_classes=19, fill=-100).tolist() == [[-100, -100, -100], [0, 1, -100]]
    # downscale 4 -> 2 columns takes columns 0 and 2; a uint16 map keeps values above 255
    u = np.array([[26001, 5, 33000, 6]], np.uint16)
    assert R.labels(u, (2, 1)).tolist() == [[26001, 33000]]
    # the script's own order (divide, resize, one-sided clean-up) is the same function on a 16-bit map
    ids = (R.noise(9, 13, 1)[:, :, 0] % 34000).astype(np.uint16)
    assert np.array_equal(R.city_instance_semantic(ids, (5, 4)), R.labels(ids, (5, 4), divisor=1000, num_classes=19))
    assert R.city_instance_semantic(u, (4, 1)).tolist() == [[255, 0, 255, 0]]


def test_image_bytes_by_hand():
    img = np.arange(16 * 3, dtype=np.uint8).reshape(4, 4, 3) * 5
    same = R.image_bytes(img, (4, 4))
    assert np.array_equal(same, img)                                    # the same size is the identity
    assert np.array_equal(R.image_bytes(img, (4, 4), bgr=True), img[:, :, ::-1])
    half = R.image_bytes(img, (2, 2)).astype(int)                       # exactly 2x: (a + b + c + d + 2) >> 2
    a = img.astype(int)
    assert half[0, 0].tolist() == ((a[0, 0] + a[0, 1] + a[1, 0] + a[1, 1] + 2) >> 2).tolist()
    assert R.image_bytes(img[:, :, 0], (2, 2)).shape == (2, 2, 1)
    assert R.to_unit(np.array([0, 255, 51], np.uint8)).tolist() == [0.0, 1.0, np.float32(51) / np.float32(255)]


# ---- pack_maps --------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 5), (7, 2), (1, 9)]
KINDS = [(np.uint8, False, 0, 1, 1), (np.uint16, False, 1, 2, 2), (np.int32, False, 2, 4, 4), (np.uint8, True, 3, 3, 1)]


@pytest.mark.parametrize("np_dtype,rgb,kind,bpp,align", KINDS, ids=["u8", "u16", "i32", "rgb8"])
def test_pack_maps_offsets_and_alignment(np_dtype, rgb, kind, bpp, align):
    from maskunet_amd import PackedMaps, pack_maps
    maps = [(R.noise(h, w, 3 if rgb else 1, salt=i) >> 3).astype(np_dtype) for i, (h, w) in enumerate(SHAPES)]
    maps = [m if rgb else m[:, :, 0] for m in maps]
    for given in (maps, [torch.from_numpy(m) for m in maps]):
        p = pack_maps(given)
        assert isinstance(p, PackedMaps) and p.kind == kind and (p.max_h, p.max_w) == (7, 9)
        assert p.data.dtype == torch.uint8 and p.offsets.dtype == torch.int64 and p.sizes.dtype == torch.int32
        assert p.sizes.tolist() == [list(s) for s in SHAPES]
        assert p.offsets.tolist() == np.concatenate([[0], np.cumsum([h * w * bpp for h, w in SHAPES])]).tolist()
        assert p.data.numel() == p.offsets[-1]
        for m, o in zip(maps, p.offsets.tolist()):
            assert (p.data.data_ptr() + o) % align == 0                 # every map starts element-aligned
            assert p.data[o:o + m.nbytes].numpy().tobytes() == m.tobytes()
        # one buffer: the metadata leads, the bytes follow
        assert p.offsets.data_ptr() + 8 * (len(SHAPES) + 1) == p.sizes.data_ptr() and p.sizes.data_ptr() + 8 * len(SHAPES) == p.data.data_ptr()


@pytest.mark.parametrize("np_dtype,rgb,kind,bpp,align", KINDS, ids=["u8", "u16", "i32", "rgb8"])
def test_pack_maps_uniform_tensor(np_dtype, rgb, kind, bpp, align):
    from maskunet_amd import pack_maps
    t = (R.noise(3 * 4, 6, 3 if rgb else 1) >> 5).astype(np_dtype).reshape((3, 4, 6, 3) if rgb else (3, 4, 6))
    for given in (t, torch.from_numpy(t)):
        p = pack_maps(given)
        assert p.kind == kind and p.sizes.tolist() == [[4, 6]] * 3 and p.offsets.tolist() == [0, 24 * bpp, 48 * bpp, 72 * bpp]
        assert p.data.numpy().tobytes() == t.tobytes() and p.data.data_ptr() % align == 0 and (p.max_h, p.max_w) == (4, 6)


def test_pack_maps_refuses():
    from maskunet_amd import pack_maps
    with pytest.raises(ValueError, match="at least one"):
        pack_maps([])
    with pytest.raises(ValueError, match="uint8, uint16 or int32"):
        pack_maps([np.zeros((2, 2), np.int64)])
    with pytest.raises(ValueError, match="share"):
        pack_maps([np.zeros((2, 2), np.uint8), np.zeros((2, 2), np.uint16)])
    with pytest.raises(ValueError, match="share"):
        pack_maps([np.zeros((2, 2), np.uint8), np.zeros((2, 2, 3), np.uint8)])
    with pytest.raises(ValueError, match="must be uint8"):
        pack_maps([np.zeros((2, 2, 3), np.int32)])
    with pytest.raises(ValueError, match=r"\[h, w\] or \[h, w, 3\]"):
        pack_maps([np.zeros((2, 2, 4), np.uint8)])
    with pytest.raises(ValueError, match="sides"):
        pack_maps([np.zeros((0, 2), np.uint8)])


def test_host_data_is_refused_without_a_device():
    import maskunet_amd as M
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        M.resize_labels_cv2([np.zeros((2, 2), np.uint8)], (2, 2))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        M.resize_cv2_to_nhwc([np.zeros((2, 2, 3), np.uint8)], (2, 2))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        M.panoptic_targets([np.zeros((2, 2, 3), np.uint8)], [[]], (2, 2))
    for n in ("pack_maps", "pack_segments", "resize_cv2_to_nhwc", "resize_labels_cv2", "panoptic_targets", "PackedMaps", "PanopticTargets"):
        assert n in M.__all__ and hasattr(M, n)


# ---- pack_segments ----------------------------------------------------------------------------------------------------------------
def test_pack_segments_sorted_and_deduplicated():
    from maskunet_amd import pack_segments
    infos = [[{"id": 300, "category_id": 4}, {"id": 7, "category_id": 2}, {"id": 55, "category_id": 3}, {"id": 300, "category_id": 9}],
             [],
             [{"id": 16777215, "category_id": 1, "iscrowd": 0}, {"id": 0, "category_id": 200}]]
    ids, labels, off = pack_segments(infos)
    assert ids.dtype == labels.dtype == off.dtype == np.int32
    assert off.tolist() == [0, 3, 3, 5]
    assert ids.tolist() == [7, 55, 300, 0, 16777215] and labels.tolist() == [2, 3, 9, 200, 1]          # the LATER 300 stays
    ids, labels, off = pack_segments(infos, cat2label={4: 40, 2: 20, 3: 30, 9: 90, 1: 10, 200: 0})
    assert labels.tolist() == [20, 30, 90, 0, 10]
    with pytest.raises(KeyError):
        pack_segments(infos, cat2label={4: 40, 2: 20, 3: 30, 9: 90, 1: 10})
    ids, labels, off = pack_segments([[], []])
    assert ids.size == 0 and labels.size == 0 and off.tolist() == [0, 0, 0]


def test_pack_segments_matches_the_loop_of_the_restatement():
    """the table is the loop's outcome: looking ids up in it gives what the loop over segments_info paints"""
    from maskunet_amd import pack_segments
    png = R.id2rgb(R.noise(6, 7, 1)[:, :, 0] % 9)
    segs = [{"id": int(i), "category_id": int(c)} for i, c in [(3, 30), (8, 80), (1, 10), (3, 31), (0, 5), (8, 81), (6, 60)]]
    ids, labels, off = pack_segments([segs])
    assert np.all(np.diff(ids) > 0)
    table = dict(zip(ids.tolist(), labels.tolist()))
    pix = R.rgb2id(png)
    sem, inst = R.coco_panoptic_targets(png, segs, (7, 6))
    assert np.array_equal(sem, np.vectorize(lambda i: table.get(i, 0))(pix))
    assert np.array_equal(inst, np.vectorize(lambda i: i if i in table else 0)(pix))


def test_pack_segments_cap():
    from maskunet_amd import pack_segments
    from maskunet_amd.targets import SEG_MAX
    assert SEG_MAX >= 1024
    full = [{"id": i + 1, "category_id": 1} for i in range(SEG_MAX)]
    assert pack_segments([full])[2].tolist() == [0, SEG_MAX]
    with pytest.raises(ValueError, match="segments"):
        pack_segments([full + [{"id": SEG_MAX + 1, "category_id": 1}]])


# ---- the C entry points refuse on the host ----------------------------------------------------------------------------------------
def test_entry_points_refuse_without_touching_the_gpu():
    from maskunet_amd import _lib
    lib = _lib.load()
    assert lib.mu_cv2_ragged_supported(64, 2048, 2048, 128, 128) == 0 and lib.mu_cv2_ragged_supported(1, 16384, 16384, 16384, 16384) == 0
    for bad in [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 16385, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 16385), (2 ** 12, 1, 1, 16384, 16384)]:
        assert lib.mu_cv2_ragged_supported(*bad) == -2, bad
    assert lib.mu_cv2_resize_ragged_u8_nhwc(None, None, None, 1, 3, 8, 8, 0, None, None, None, 8, 8, 8, 0, None) == -1
    assert lib.mu_cv2_nearest_ragged(None, None, None, 0, 1, 8, 8, 1, 0, 255, None, None, 8, 8, None) == -1
    assert lib.mu_panoptic_targets(None, None, None, None, None, None, 1, 0, 8, 8, 0, 255, None, None, None, 8, 8, None) == -1
    assert _lib.MU_PANOPTIC_SEG_MAX >= 1024 and (_lib.MU_MAP_U8, _lib.MU_MAP_U16, _lib.MU_MAP_I32, _lib.MU_MAP_RGB8, _lib.MU_MAP_BGR8) == (0, 1, 2, 3, 4)
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "maskunet_hip.h")).read()
    for name, value in [("MU_MAP_U8", 0), ("MU_MAP_U16", 1), ("MU_MAP_I32", 2), ("MU_MAP_RGB8", 3), ("MU_MAP_BGR8", 4),
                        ("MU_PANOPTIC_SEG_MAX", _lib.MU_PANOPTIC_SEG_MAX)]:
        assert f"#define {name} {value}\n" in hdr, name
