"""Times the RLE export of a predict_instances result at the evaluation shape of the instance scripts (B = 64, 128x128, K = 100
queries, 19 classes) against the host path it replaces, on the same box:

  device   maskunet_amd.encode_rle(pred.ids, pred.order[:, :K]) -- HIP events on the launch stream around the raw mu_rle_encode call
           (buffers allocated beforehand), warm-up calls first, median / min / max;  plus the copy of the used string bytes to the host
           (RLEs.to_coco for every image), by a host clock that ends after the last copy;
  host     Instances.to_reference(b, K) for every image (the dense masks copied to the host) and the vectorised numpy encoder of
           tests/_rle_reference.py (encode_fast + string) on each mask, by a host clock.  pycocotools is not available, so its C
           encoder is NOT what is timed here: the host figure is the path a user of this package has without it.

    python tools/bench_rle.py [--batch 64] [--reps 20] [--host-reps 3] [--out profiles/rle_encode_b64.json]

The logits are smoothed noise around a blocky label map (as tests/test_gpu_match.py builds them), so the instances have ragged borders.
The two paths are compared string by string before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _cc_reference as CC  # noqa: E402
from tests import _rle_reference as R  # noqa: E402


def make_logits(B, C, H, W, block=16, seed=0):
    rng = np.random.default_rng(seed)
    labels = np.stack([CC.blocky(rng, H, W, C, block) for _ in range(B)])
    x = 3.0 * np.eye(C, dtype=np.float32)[labels].transpose(0, 3, 1, 2) + rng.standard_normal((B, C, H, W), dtype=np.float32)
    return ((x + np.roll(x, 1, 2) + np.roll(x, 1, 3) + np.roll(x, -1, 2) + np.roll(x, -1, 3)) / 5).astype(np.float32)


def host_path(pred, B, K, H, W):
    out = []
    for b in range(B):
        out.append([{"size": [H, W], "counts": R.string(R.encode_fast(d["mask"]))} for d in pred.to_reference(b, K)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--max-queries", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import maskunet_amd
    from maskunet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    B, C, H, W, K, M = a.batch, 19, 128, 128, a.max_queries, 1024
    pred = maskunet_amd.predict_instances(torch.from_numpy(make_logits(B, C, H, W)).to(dev), max_instances=M)
    sel = pred.order[:, :K].contiguous()
    L = 2 * H * W + K
    i32 = dict(dtype=torch.int32, device=dev)
    offsets, counts, area, soff = torch.empty((B, K + 1), **i32), torch.empty((B, L), **i32), torch.empty((B, K), **i32), torch.empty((B, K + 1), **i32)
    sbytes = torch.empty((B, 4 * L), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.mu_rle_encode_workspace_bytes(B, H, W, K, M), dtype=torch.uint8, device=dev)

    def run():
        _lib.call("mu_rle_encode", pred.ids.data_ptr(), sel.data_ptr(), B, H, W, K, M, offsets.data_ptr(), counts.data_ptr(), area.data_ptr(),
                  soff.data_ptr(), sbytes.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream())

    rles = maskunet_amd.rle.RLEs(offsets, counts, area, soff, sbytes, H, W)
    run()
    torch.cuda.synchronize()
    want = host_path(pred, B, K, H, W)
    got = [rles.to_coco(b) for b in range(B)]
    assert got == want, "device and host strings differ"

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
    export = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        for b in range(B):
            rles.to_coco(b)
        export.append((time.perf_counter() - t0) * 1e3)
    host = []
    for _ in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path(pred, B, K, H, W)
        host.append((time.perf_counter() - t0) * 1e3)

    n_rows = sum(len(g) for g in got)
    res = {"what": "RLE export of a predict_instances result: device encode against to_reference + numpy encode on the host, same box",
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "H": H, "W": W, "classes": C, "max_queries": K, "max_instances": M},
           "rows_encoded": n_rows, "instances_per_image_mean": float(pred.count.float().mean()),
           "counts_per_image_mean": float(offsets[:, -1].float().mean()), "characters_per_image_mean": float(soff[:, -1].float().mean()),
           "mu_rle_encode_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms), "clock": "HIP events"},
           "encode_plus_to_coco_all_images_ms": {"median": statistics.median(export), "min": min(export), "max": max(export),
                                                 "n": len(export), "clock": "host, ends after the last copy"},
           "host_to_reference_plus_numpy_encode_ms": {"median": statistics.median(host), "min": min(host), "max": max(host),
                                                      "n": len(host), "clock": "host"},
           "dense_masks_bytes_copied_by_host_path": n_rows * H * W,
           "string_bytes_copied_by_device_path": int(soff[:, -1].sum())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
