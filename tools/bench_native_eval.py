"""Times the native-resolution semantic evaluation (mu_sem_eval_native: bilinear upsampling, arg-max and counting in one kernel that never
writes the upsampled logits) against the torch composition it replaces, in one process on the same tensors, for two shapes:

  Cityscapes  19 classes, 128x128 logits -> 1024x2048 labels, B = 8;
  ADE-like    150 classes, 128x128 logits -> ragged labels around 512x683, B = 8.

The logits are an fp16 module output (NCHW carrying its channel-padded NHWC source).  The torch composition runs per image, because the
images of a batch differ in size: F.interpolate(logits[b], size=(H_b, W_b), mode="bilinear") -> argmax -> bincount of label * C + pred.
The kernel is timed with the class map written and without (every buffer allocated beforehand; what is timed is the two launches).
Bytes per second from algorithmic bytes: the logits once, one label byte per pixel, one class-map byte per pixel when written; the
composition's own traffic is the upsampled tensor written and read once (2 x B x C x H x W x 2 bytes) on top.

Prints one line per figure: median of `--reps` measurements (HIP events) after `--warmup` unmeasured ones, with minimum and maximum.

    python tools/bench_native_eval.py [--reps 10] [--warmup 2]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from maskunet_amd import _lib, ops, pack_images  # noqa: E402
from maskunet_amd.instances import _strided_source  # noqa: E402
from tools.bench_instances import HBM_PEAK, show, timed  # noqa: E402

SHAPES = {
    "Cityscapes": (19, 32, [(1024, 2048)] * 8),
    "ADE-like": (150, 160, [(512, 683), (683, 512), (512, 512), (480, 640), (512, 768), (600, 512), (512, 683), (384, 512)]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda")
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    h = w = 128
    for name, (C, Cp, sizes) in SHAPES.items():
        B = len(sizes)
        # post-ReLU noise plus a 6.0 on a blocky class map: a trained model's output; labels = random classes with a tenth void
        cls_map = torch.randint(0, C, (B, h // 8, w // 8), device=dev, generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        nhwc = torch.zeros(B, h, w, Cp, dtype=torch.float16, device=dev)
        nhwc[..., :C] = torch.relu(torch.randn(B, h, w, C, device=dev, generator=g)).half()
        nhwc.scatter_add_(3, cls_map[..., None], torch.full((B, h, w, 1), 6.0, dtype=torch.float16, device=dev))
        out = ops.to_nchw(nhwc, C)
        rng = np.random.default_rng(0)
        maps = []
        for H, W in sizes:
            m = rng.integers(0, C, (H, W)).astype(np.uint8)
            m[rng.random((H, W)) < 0.1] = 255
            maps.append(m)
        labels = pack_images(maps, device=dev)
        label_t = [torch.from_numpy(m).to(dev) for m in maps]
        npix = sum(H * W for H, W in sizes)
        x, inner, outer, cs, ps = _strided_source(out)
        img_counts = torch.empty((B, 3, C), dtype=torch.int32, device=dev)
        conf = torch.zeros((C + 1, C), dtype=torch.int64, device=dev)
        valid = torch.empty(B, dtype=torch.uint8, device=dev)
        cls = torch.zeros_like(labels.data)
        nws = lib.mu_sem_eval_native_workspace_bytes(B, C, h, w, labels.max_h, labels.max_w)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)

        def native(with_classes):
            c = cls.data_ptr() if with_classes else None
            return lambda: _lib.call("mu_sem_eval_native", x.data_ptr(), B, C, h, w, inner, outer, cs, ps, labels.data.data_ptr(),
                                     labels.offsets.data_ptr(), labels.sizes.data_ptr(), labels.max_h, labels.max_w, 255,
                                     img_counts.data_ptr(), conf.data_ptr(), valid.data_ptr(), c, ws.data_ptr(), nws, _lib.dt(x), _lib.stream())

        conf_t = torch.zeros((C + 1) * C, dtype=torch.int64, device=dev)

        def composition():
            for b, (H, W) in enumerate(sizes):
                up = F.interpolate(out[b:b + 1], size=(H, W), mode="bilinear", align_corners=False)
                pred = up.argmax(1).view(-1)
                lab = label_t[b].view(-1).long()
                row = torch.where((lab != 255) & (lab < C), lab, torch.full_like(lab, C))
                conf_t.add_(torch.bincount(row * C + pred, minlength=(C + 1) * C))

        print(f"--- {name}: B={B} C={C} Cp={Cp} fp16, {h}x{w} -> {sizes[0][0]}x{sizes[0][1]}{' (ragged)' if len(set(sizes)) > 1 else ''}, "
              f"{npix / 1e6:.2f} M label pixels ---")
        med = {}
        for label, fn, nbytes in [("mu_sem_eval_native", native(False), B * h * w * Cp * 2 + npix),
                                  ("mu_sem_eval_native + class map", native(True), B * h * w * Cp * 2 + 2 * npix)]:
            ms = timed(fn, a.reps, a.warmup)
            m = statistics.median(ms)
            med[label] = show(label, ms, f"  {nbytes / m / 1e6:.1f} GB/s = {100 * nbytes / (m * 1e-3) / HBM_PEAK:.2f} % of 8 TB/s; "
                                         f"{npix * C / m / 1e6:.1f} G pixel-classes/s")
        t = show("torch: interpolate + argmax + bincount, per image", timed(composition, a.reps, a.warmup),
                 f"  {2 * npix * C * 2 / 1e6:.0f} MB of upsampled logits written and read")
        for label in med:
            print(f"{label}: {med[label]:.3f} ms against {t:.3f} ms for the torch composition ({t / med[label]:.1f} x)", flush=True)
        assert int(valid.sum()) == B and int(img_counts[:, 1].sum()) == npix       # the kernel did count (read back after the timing)


if __name__ == "__main__":
    main()
