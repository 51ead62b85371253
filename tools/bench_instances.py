"""Times instance extraction (maskunet_amd.instances) at the evaluation shape of the instance / panoptic scripts:
B = 64, c_out = 150, 128x128, fp32 NCHW and fp16 NHWC outputs.

  (a) predict_instances, HIP events, warm;
  (b) the part of the reference's route that runs here, a LOWER bound on that route: torch softmax(outputs / 0.5) plus .cpu();
  (c) the numpy reference per image (tests/_cc_reference.py), for scale;
  the arg-max pass alone and its share of HBM bandwidth (algorithmic bytes: logits read once, 8 bytes per pixel written);
  the raw mu_instances call (label + statistics launches, every buffer allocated beforehand) on the 128x128 blocky map and on the
  128x128 serpentine, at B = 64 and B = 1.

Prints one line per figure: median of `--reps` measurements, with minimum and maximum.

    python tools/bench_instances.py [--batch 64] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maskunet_amd  # noqa: E402
from maskunet_amd import _lib, ops  # noqa: E402
from tests import _cc_reference as R  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s, MI355X


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def raw_instances(c, prob, max_inst):
    """the bare mu_instances call on buffers allocated here, once: what is timed is the two launches"""
    lib = _lib.load()
    B, H, W = c.shape
    dev = c.device
    ids = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    table = torch.empty((B, max_inst, 8), dtype=torch.int32, device=dev)
    score = torch.empty((B, max_inst), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    order = torch.empty((B, max_inst), dtype=torch.int32, device=dev)
    ws = torch.empty(lib.mu_instances_workspace_bytes(B, H, W, max_inst), dtype=torch.uint8, device=dev)
    args = (c.data_ptr(), prob.data_ptr(), B, H, W, max_inst, ids.data_ptr(), table.data_ptr(), score.data_ptr(), count.data_ptr(),
            order.data_ptr(), ws.data_ptr(), ws.numel())
    keep = (c, prob, ids, table, score, count, order, ws)
    return lambda: (_lib.call("mu_instances", *args, _lib.stream()), keep)[0]


def show(name, ms, extra=""):
    print(f"{name:58s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}   n={len(ms)} {extra}", flush=True)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    B, C, H, W = a.batch, 150, 128, 128
    dev = torch.device("cuda")
    M = B * H * W
    rng = np.random.default_rng(0)
    # logits whose arg-max is a blocky class map (8x8 blocks, 150 classes) under post-ReLU noise: the shape of a trained model's output
    cls = np.stack([R.blocky(rng, H, W, C) for _ in range(B)])
    g = torch.Generator(device=dev).manual_seed(0)
    x32 = torch.relu(torch.randn(B, C, H, W, device=dev, generator=g))
    x32.scatter_add_(1, torch.from_numpy(cls).long().to(dev)[:, None], torch.full((B, 1, H, W), 6.0, device=dev))
    Cp = 160
    x16 = torch.zeros(B, H, W, Cp, dtype=torch.float16, device=dev)
    x16[..., :C] = x32.permute(0, 2, 3, 1).half()
    out16 = ops.to_nchw(x16, C)                       # what a maskunet_amd module returns in fp16: NCHW fp32 + its NHWC source
    print(f"shape B={B} C={C} {H}x{W}; instances per image (reference, image 0): {int(R.instances(cls[:1], None, 4096)['count'][0])}")

    for name, x in [("fp32 NCHW", x32), ("fp16 NHWC source", out16)]:
        show(f"(a) predict_instances, {name}", timed(lambda: maskunet_amd.predict_instances(x), a.reps))
    for name, x in [("fp32 NCHW", x32), ("fp32 NCHW of the fp16 model", out16)]:
        def ref_route():
            return torch.softmax(x / 0.5, dim=1).cpu()
        t = []
        for i in range(max(3, a.reps // 4) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref_route()
            t.append((time.perf_counter() - t0) * 1e3)
        show(f"(b) torch softmax(x/0.5) + .cpu(), {name} (wall)", t[1:])
    prob = R.argmax_prob(x32[:2].permute(0, 2, 3, 1).cpu().double().numpy())[1]
    t = []
    for i in range(2):
        t0 = time.perf_counter()
        R.instances(cls[i:i + 1], prob[i:i + 1], 1024)
        t.append((time.perf_counter() - t0) * 1e3)
    show("(c) numpy reference, one image (wall)", t)

    cls_d = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    prob_d = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    for name, x, args, nbytes in [("fp32 NCHW", x32, (H * W, C * H * W, H * W, 1), M * C * 4 + M * 8),
                                  ("fp16 NHWC", x16, (M, 0, 1, Cp), M * Cp * 2 + M * 8)]:
        ms = timed(lambda: _lib.call("mu_argmax_prob", x.data_ptr(), M, C, *args, 2.0, cls_d.data_ptr(), prob_d.data_ptr(), _lib.dt(x),
                                     _lib.stream()), a.reps)
        med = statistics.median(ms)
        show(f"arg-max pass, {name}", ms, f"  {nbytes / med / 1e9:.2f} TB/s = {100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")

    for name, m in [("blocky 128x128 (19 classes)", R.random_maps()["blocky_128_c19"][0]), ("serpentine 128x128", R.patterns()["serpentine_128"]),
                    ("blocky 128x128 (150 classes, the map above)", None)]:
        c = torch.from_numpy(cls if m is None else np.repeat(m[None], B, 0)).int().to(dev).contiguous()
        for nb in (B, 1):
            show(f"mu_instances (label + statistics launches), B={nb}, {name}", timed(raw_instances(c[:nb].contiguous(), prob_d[:nb], 1024), a.reps))


if __name__ == "__main__":
    main()
