"""Times the ragged cv2 sample preparation (maskunet_amd.targets) at a loader's shape: B images of COCO / ADE20K sizes -> 128x128 fp16, and
beside it what the uniform kernels need for the same batch: B launches of resize_u8_to_nhwc / resize_labels_u8 and one torch.cat each.

    python tools/bench_cv2_ragged.py [--batch 64] [--reps 20] [--inner 10] [--out FILE]

HIP events on the current stream around `--inner` back-to-back rounds through the Python API on batches that are already on the device
(packed once for the ragged calls, a list of tensors for the uniform ones), 3 warm-up rounds, the two ways alternating; median / min / max
per round.  The two results are compared bit for bit first.  Information, not a threshold."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _targets_reference as R  # noqa: E402

SIZES = [(480, 640), (427, 640), (640, 480), (375, 500), (500, 333), (256, 256), (683, 512), (512, 683)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import maskunet_amd as mu
    from maskunet_amd import ops
    dev, B, out = torch.device("cuda"), a.batch, (128, 128)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shapes = [SIZES[i % len(SIZES)] for i in range(B)]
    imgs = [torch.from_numpy((R.noise(h, w, 3, i) >> 9).astype(np.uint8)).to(dev) for i, (h, w) in enumerate(shapes)]
    maps = [torch.from_numpy((R.noise(h, w, 1, i)[:, :, 0] % 150).astype(np.uint8)).to(dev) for i, (h, w) in enumerate(shapes)]
    pngs = [torch.from_numpy(R.id2rgb(R.noise(h // 16 + 1, w // 16 + 1, 1, i)[:, :, 0].repeat(16, 0).repeat(16, 1)[:h, :w] % 40 * 1000)).to(dev)
            for i, (h, w) in enumerate(shapes)]
    infos = [[{"id": k * 1000, "category_id": k % 133 + 1} for k in range(1, 40)] for _ in range(B)]
    p_img, p_map, p_png = mu.pack_images(imgs), mu.pack_maps(maps), mu.pack_images(pngs)

    def ragged():
        x, _ = mu.resize_cv2_to_nhwc(p_img, out, torch.float16, bgr=True)
        lab, _ = mu.resize_labels_cv2(p_map, out)
        return x, lab

    def uniform():
        x = torch.cat([ops.resize_u8_to_nhwc(im[None], out, torch.float16, bgr=True) for im in imgs])
        lab = torch.cat([ops.resize_labels_u8(m[None], out) for m in maps])
        return x, lab

    def panoptic():
        return mu.panoptic_targets(p_png, infos, out)

    (xr, lr), (xu, lu) = ragged(), uniform()
    assert torch.equal(xr.view(torch.int16), xu.view(torch.int16)) and torch.equal(lr, lu)
    runs = {"ragged: 2 launches": ragged, f"uniform: {2 * B} launches + 2 cat": uniform, "panoptic_targets (tables copied per call)": panoptic}
    ms = {k: [] for k in runs}
    for f in runs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in runs.items():                            # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    say(f"B = {B} images of {len(SIZES)} COCO / ADE20K sizes -> 128x128 fp16 + int64 labels; {a.reps} x {a.inner} rounds, ms per round, host-paced")
    for k, v in ms.items():
        say(f"  {k:45s} median {statistics.median(v):8.4f}  min {min(v):8.4f}  max {max(v):8.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
