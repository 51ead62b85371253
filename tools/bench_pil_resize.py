"""Times mu_pil_resize_u8_nhwc at the shape of a COCO batch: B = 64 images of 480x640x3 to 128x128 (fp16, Cp = 32, with the resized bytes),
next to Pillow's own Image.resize(.., BILINEAR) on the same input where Pillow is importable -- FOR SCALE ONLY: one host thread against
a whole GPU, and no time is a pass criterion.

  device   HIP events on the launch stream around the raw entry point (both launches; buffers uploaded and allocated beforehand),
           3 warm-up and 20 timed calls, median / min / max;
  host     Pillow, image after image, by a host clock, once.

    python tools/bench_pil_resize.py [--batch 64] [--reps 20] [--out profiles/pil_resize_bench.txt]

Bytes per batch: 64 * 480 * 640 * 3 = 59.0 MB read, 64 * 128 * 128 * (32 * 2 + 3) = 70.3 MB written (the activations with their zero
padding channels; the three real channels alone are 6.3 MB).  The
device bytes are compared with the numpy restatement (one image) and with Pillow (all of them, where importable) before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _pil_reference as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from maskunet_amd import _lib, pack_images
    lib = _lib.load()
    dev = torch.device("cuda")
    B, h, w, C, Hd, Wd, Cp = a.batch, 480, 640, 3, 128, 128, 32
    base = R.pattern(h, w + B, C, "noise")
    imgs = [np.ascontiguousarray(base[:, i:i + w]) for i in range(B)]           # B different images from one formula
    p = pack_images(imgs, device=dev)
    y = torch.empty((B, Hd, Wd, Cp), dtype=torch.float16, device=dev)
    u8 = torch.empty((B, Hd, Wd, C), dtype=torch.uint8, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    nbytes = lib.mu_pil_resize_workspace_bytes(B, p.max_h, p.max_w, Hd, Wd)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def run():
        _lib.call("mu_pil_resize_u8_nhwc", p.data.data_ptr(), p.offsets.data_ptr(), p.sizes.data_ptr(), B, C, p.max_h, p.max_w, 0, y.data_ptr(),
                  u8.data_ptr(), valid.data_ptr(), Hd, Wd, Cp, _lib.MU_F16, ws.data_ptr(), nbytes, _lib.stream())

    run()
    torch.cuda.synchronize()
    got = u8.cpu().numpy()
    assert bool(valid.all()) and np.array_equal(got[0], R.resize(imgs[0], (Hd, Wd))), "device and restatement differ"
    pillow = None
    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = None
    if PIL is not None:
        t0 = time.perf_counter()
        outs = [np.asarray(Image.fromarray(im).resize((Wd, Hd), Image.BILINEAR)) for im in imgs]
        pillow = {"once": (time.perf_counter() - t0) * 1e3, "clock": "host, one thread, resize only", "version": PIL.__version__}
        assert all(np.array_equal(got[i], outs[i]) for i in range(B)), "device and Pillow differ"

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))

    bytes_in, bytes_out = B * h * w * C, y.numel() * 2 + u8.numel()
    med = statistics.median(ms)
    res = {"what": "Pillow-exact antialiased bilinear resize of a ragged batch, mu_pil_resize_u8_nhwc (coefficient + resample launches); "
                   "the Pillow figure is for scale only",
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "h": h, "w": w, "C": C, "Hd": Hd, "Wd": Wd, "Cp": Cp, "dtype": "fp16"},
           "bytes_in": bytes_in, "bytes_out": bytes_out, "workspace_bytes": int(nbytes),
           "mu_pil_resize_ms": {"median": med, "min": min(ms), "max": max(ms), "n": len(ms), "clock": "HIP events"},
           "effective_GBps_at_median": (bytes_in + bytes_out) / med / 1e6,
           "pillow_ms": pillow}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
