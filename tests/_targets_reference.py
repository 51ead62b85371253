"""The target construction of the loaders that read with OpenCV, restated in numpy.  TEST INFRASTRUCTURE ONLY: no torch, nothing of
maskunet_amd.  The resizes are oracle.cv2_resize_oracle's (one restatement of cv2 remains); everything else is what the scripts spell out:

  coco_panoptic.py:70-95   seg_id_map = rgb2id(seg_rgb); two zero int32 maps; for every entry of segments_info, IN LIST ORDER, the pixels
                           with its id take its label (semantic) and its id (instance) -- so of two entries with one id the later one
                           stays, and a pixel whose id is not listed keeps 0 / 0; then INTER_NEAREST of both; .long()
  coco_semantic.py:70-86   the semantic half of the same
  city_semantic.py:84-88   np.where((m >= 0) & (m < 19), m, 255), then INTER_NEAREST
  city_panoptic.py:97-115  the same clean-up; the 16-bit instanceIds map resized as it is
  city_instance.py:81-106  without a labelTrainIds file: semantic = instanceIds.astype(int32) // 1000; INTER_NEAREST; after the resize
                           semantic[semantic >= 19] = 255
  ade_semantic.py:65-76    BGR2RGB, INTER_LINEAR, ToTensor (the same three lines in every one of these loaders)
"""
import numpy as np

from oracle.cv2_resize_oracle import resize_linear_u8, resize_nearest


def rgb2id(rgb):
    """panopticapi.utils.rgb2id for a uint8 [h, w, 3] array: R + 256 G + 65536 B"""
    c = rgb.astype(np.int64)
    return c[:, :, 0] + 256 * c[:, :, 1] + 65536 * c[:, :, 2]


def id2rgb(ids):
    """its inverse, for building test PNGs: int [h, w] in [0, 2^24) -> uint8 [h, w, 3]"""
    ids = np.asarray(ids, np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536], axis=-1).astype(np.uint8)


def coco_panoptic_targets(png_rgb, segments_info, size, cat2label=None):
    """(semantic, instance) int64 [Hd, Wd] of one sample; size = (width, height); cat2label None = identity, else a dict (KeyError for a
    category that is not in it, as self.cat2label[cat_id] raises)"""
    ids = rgb2id(png_rgb)
    semantic = np.zeros(ids.shape, np.int32)
    instance = np.zeros(ids.shape, np.int32)
    for seg in segments_info:                                # list order: a later entry overwrites an earlier one with the same id
        label = seg["category_id"] if cat2label is None else cat2label[seg["category_id"]]
        hit = ids == seg["id"]
        semantic[hit] = label
        instance[hit] = seg["id"]
    return resize_nearest(semantic, size).astype(np.int64), resize_nearest(instance, size).astype(np.int64)


def labels(m, size, divisor=1, num_classes=None, fill=255):
    """an id map of any integer type -> int64 [Hd, Wd]: floor division (Python's //, which numpy's // is too), the two-sided class
    clean-up, INTER_NEAREST.  Both steps act per element, so they commute with the nearest resize: the scripts run them on either side."""
    v = np.asarray(m).astype(np.int64)
    if divisor > 1:
        v = v // divisor
    if num_classes is not None:
        v = np.where((v >= 0) & (v < num_classes), v, fill)
    return resize_nearest(v, size)


def city_instance_semantic(instance_ids_u16, size, num_classes=19):
    """city_instance.py's fallback in the script's own order: // 1000, resize, then the one-sided clean-up (no value is negative here)"""
    semantic = resize_nearest(instance_ids_u16.astype(np.int32) // 1000, size).astype(np.int64)
    semantic[semantic >= num_classes] = 255
    return semantic


def image_bytes(img, size, bgr=False):
    """the resized bytes uint8 [Hd, Wd, C] of one decoded image ([h, w] or [h, w, C]); bgr=True: cv2.imread bytes, COLOR_BGR2RGB first"""
    img = np.ascontiguousarray(img[:, :, ::-1] if (bgr and img.ndim == 3) else img)
    out = resize_linear_u8(img, size)
    return out.reshape(size[1], size[0], -1)


def to_unit(u8, dtype=np.float32):
    """ToTensor: float32(byte) / float32(255) by IEEE division, rounded to nearest even for fp16 storage"""
    return (u8.astype(np.float32) / np.float32(255.0)).astype(dtype)


def noise(h, w, c, salt=0):
    """uint32 [h, w, c] from integer arithmetic alone (a multiplicative hash of the position): content for images and id maps"""
    y, x, ch = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(c, dtype=np.uint64), indexing="ij")
    m = np.uint64(0xFFFFFFFF)
    v = (y * np.uint64(73856093) + x * np.uint64(19349663) + ch * np.uint64(83492791) + np.uint64(h * 131 + w * 31 + 7 + salt * 977)) & m
    v = ((v ^ (v >> np.uint64(15))) * np.uint64(0x2C1B3C6D)) & m
    v = ((v ^ (v >> np.uint64(12))) * np.uint64(0x297A2D39)) & m
    return (v ^ (v >> np.uint64(15))).astype(np.uint32)
