"""Times mu_coco_masks at the shape of a COCO training batch: B = 64 images of 640x480 (h = 480, w = 640) with 8 annotations of about 40
vertices each, to 128x128 -- next to tests/_poly_reference.py (numpy, one annotation after the other) on the same input, FOR SCALE ONLY:
pycocotools is not available, so its C rasteriser is not what is timed, and no speed-up is claimed.

  device   HIP events on the launch stream around the raw mu_coco_masks call (arrays uploaded and outputs allocated beforehand),
           3 warm-up and 20 timed calls, median / min / max;
  host     tests/_poly_reference.coco_masks by a host clock, once.

    python tools/bench_poly.py [--batch 64] [--reps 20] [--out profiles/coco_masks_b64.json]

Every polygon is a wobbly ring of 30..50 vertices around a random centre (radius 20..120 px, partly outside the image).  The two paths
are compared output by output before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _poly_reference as R  # noqa: E402


def make_annotations(B, per_image, h, w, seed=0):
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(B):
        segs = []
        for _ in range(per_image):
            k = int(rng.integers(30, 51))
            ang = np.sort(rng.uniform(0, 2 * np.pi, size=k))
            rad = rng.uniform(20, 120) * rng.uniform(0.7, 1.3, size=k)
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            segs.append([np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1), 2).reshape(-1).tolist()])
        images.append(segs)
    return images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from maskunet_amd import _lib
    from maskunet_amd.coco import pack_annotations
    lib = _lib.load()
    dev = torch.device("cuda")
    B, per_image, h, w, Ho, Wo, max_points = a.batch, 8, 480, 640, 128, 128, 1 << 20
    ann, sizes = make_annotations(B, per_image, h, w), [(h, w)] * B
    p = pack_annotations(ann, sizes)
    t = {k: torch.from_numpy(v).to(dev) for k, v in p.items()}
    A, P = p["ann_poly_offsets"].size - 1, p["poly_offsets"].size - 1
    cover = torch.empty((B, Ho, Wo), dtype=torch.int64, device=dev)
    ids = torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev)
    masks = torch.empty((A, Ho, Wo), dtype=torch.uint8, device=dev)
    area, valid = torch.empty(A, dtype=torch.int32, device=dev), torch.empty(A, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mu_coco_masks_workspace_bytes(B, A, Ho, Wo), dtype=torch.uint8, device=dev)
    ptr = lambda x: x.data_ptr() if x.numel() else None

    def run():
        _lib.call("mu_coco_masks", ptr(t["xy"]), ptr(t["poly_offsets"]), ptr(t["ann_poly_offsets"]), ptr(t["rle_counts"]),
                  ptr(t["ann_rle_offsets"]), ptr(t["img_ann_offsets"]), ptr(t["sizes"]), B, A, P, p["xy"].size // 2, p["rle_counts"].size,
                  Ho, Wo, max_points, ptr(cover), ptr(ids), ptr(masks), ptr(area), ptr(valid), ptr(ws), ws.numel(), _lib.stream())

    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = R.coco_masks(ann, sizes, (Ho, Wo), max_points)
    host_ms = (time.perf_counter() - t0) * 1e3
    for name, got in (("cover", cover), ("ids", ids), ("masks", masks), ("area", area), ("valid", valid)):
        assert np.array_equal(got.cpu().numpy(), ref[name]), f"device and host differ in {name}"

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

    points = sum(R.polygon_point_count(*R.scaled_vertices(poly)) for segs in ann for seg in segs for poly in seg)
    res = {"what": "COCO polygons to 128x128 masks, cover and ids: mu_coco_masks against tests/_poly_reference.py (numpy) on the same "
                   "input, same box; the host figure is for scale only",
           "date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "annotations_per_image": per_image, "h": h, "w": w, "Ho": Ho, "Wo": Wo},
           "vertices_total": int(p["xy"].size // 2), "upsampled_points_total": int(points), "input_bytes": int(sum(v.nbytes for v in p.values())),
           "dense_full_size_masks_bytes_not_built": A * h * w, "area_mean": float(ref["area"].mean()),
           "mu_coco_masks_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms), "clock": "HIP events"},
           "poly_reference_ms": {"once": host_ms, "clock": "host"}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
