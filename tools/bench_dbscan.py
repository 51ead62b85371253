"""Times the embedding-instance post-processing (mu_dbscan_instances) at the evaluation shape of the instance scripts:
B = 64, 128x128, 19 classes, 16-D embeddings.  The class map is blocky (16x16 blocks, like a trained model's regions); every
connected region gets its own embedding centre, pixels scatter around it with sigma = 0.075 (in-cluster distances around eps).

    python tools/bench_dbscan.py [--batch 64] [--reps 10] [--dtype fp32|fp16] [--layout nchw|nhwc]
    python tools/bench_dbscan.py --host-reference PATH/city_instance.py [--images 2]     # CPU only: the reference's own functions

GPU: HIP events on the launch stream around the raw call (buffers allocated beforehand), 2 warm-up calls, median / min / max.  The
split over the kernels comes from `rocprofv3 --kernel-trace --stats -- python tools/bench_dbscan.py --reps 3`.
--host-reference: get_instances_from_embeddings + get_instance_annotations are extracted from the given file (needs sklearn) and timed
per image on the same input (wall clock, the host this runs on)."""
import argparse
import ast
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _cc_reference as CC  # noqa: E402


def make_input(B, H=128, W=128, C=19, D=16, block=16, sigma=0.075, seed=0):
    rng = np.random.default_rng(seed)
    cls = np.stack([CC.blocky(rng, H, W, C, block) for _ in range(B)])
    emb = np.empty((B, H, W, D), np.float32)
    for b in range(B):
        ids, regions = CC.label_image(cls[b])
        centres = 2.0 * rng.standard_normal((len(regions) + 1, D))
        emb[b] = centres[ids] + sigma * rng.standard_normal((H, W, D))
    return cls, emb


def host_reference(path, cls, emb, images):
    from sklearn.cluster import DBSCAN
    names = ["get_instances_from_embeddings", "get_instance_annotations"]
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"np": np, "DBSCAN": DBSCAN, "mask_to_rle": lambda m: m}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    t = []
    for b in range(images):
        t0 = time.perf_counter()
        ids = ns[names[0]](cls[b].astype(np.int64), emb[b], eps=0.5, min_samples=5)
        ann = ns[names[1]](ids, cls[b].astype(np.int64))
        t.append((time.perf_counter() - t0) * 1e3)
        print(f"image {b}: {len(ann)} instances, {t[-1]:.1f} ms", flush=True)
    print(f"host reference (sklearn DBSCAN + annotations), per image: median {statistics.median(t):.1f} ms over {images} images; "
          f"x{len(cls)} images = {statistics.median(t) * len(cls) / 1e3:.2f} s per batch (wall, this host's CPU)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--layout", default="nchw", choices=["nchw", "nhwc"])
    ap.add_argument("--max-instances", type=int, default=1024)
    ap.add_argument("--host-reference", default=None)
    ap.add_argument("--images", type=int, default=2)
    a = ap.parse_args()
    B, H, W, C, D = a.batch, 128, 128, 19, 16
    cls, emb = make_input(B)
    if a.host_reference:
        return host_reference(a.host_reference, cls, emb, min(a.images, B))

    import torch
    from maskunet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    tdt = torch.float16 if a.dtype == "fp16" else torch.float32
    if a.layout == "nchw":
        e = torch.from_numpy(emb).permute(0, 3, 1, 2).contiguous().to(dev, tdt)
        strides = (H * W, D * H * W, H * W, 1)
    else:
        e = torch.zeros((B, H, W, 32), dtype=tdt, device=dev)
        e[..., :D] = torch.from_numpy(emb).to(dev, tdt)
        strides = (B * H * W, 0, 1, 32)
    c = torch.from_numpy(cls).to(dev)
    K = a.max_instances
    ids = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    table = torch.empty((B, K, 8), dtype=torch.int32, device=dev)
    score = torch.empty((B, K), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    order = torch.empty((B, K), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mu_dbscan_workspace_bytes(B, H, W, C, K), dtype=torch.uint8, device=dev)

    def run():
        _lib.call("mu_dbscan_instances", c.data_ptr(), e.data_ptr(), B, H, W, D, *strides, _lib.dt(tdt), C, 0.5, 5, K, ids.data_ptr(),
                  table.data_ptr(), score.data_ptr(), count.data_ptr(), order.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream())

    for _ in range(2):
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
    sizes = np.bincount(cls[0].reshape(-1), minlength=C)[1:]
    pairs = sum(float((np.bincount(cls[b].reshape(-1), minlength=C)[1:].astype(np.float64) ** 2).sum()) for b in range(B))
    med = statistics.median(ms)
    print(f"shape B={B} {H}x{W} C={C} D={D} {a.dtype} {a.layout}; image 0: class sizes {sizes.min()}..{sizes.max()}, "
          f"{int(count[0])} instances; {pairs:.3e} same-class pairs per batch")
    print(f"mu_dbscan_instances: median {med:.3f} ms   min {min(ms):.3f}   max {max(ms):.3f}   n={len(ms)}   "
          f"({pairs * D * 2 / med / 1e9:.2f} T fp64 instr-lanes/s counted over ONE full sweep)")


if __name__ == "__main__":
    main()
