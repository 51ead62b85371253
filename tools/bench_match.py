"""Times the instance matching (mu_instance_pairs + mu_instance_match) at the evaluation shape of the instance / panoptic scripts:
B = 64, 128x128, 19 and 150 classes.  The ground truth is a blocky class map (16x16 blocks); the prediction is the same map moved by
two pixels with 5 % of the blocks redrawn, so most instances have a partner at an IoU between 0.5 and 1.  Both sides are labelled on
the device (mu_instances) before the clock starts.

    python tools/bench_match.py [--batch 64] [--reps 10] [--max-instances 1024]

HIP events on the launch stream around the two raw calls (buffers allocated beforehand), 2 warm-up calls, median / min / max.  The split
over the two kernels comes from `rocprofv3 --kernel-trace --stats -- python tools/bench_match.py --reps 3`.  The host path this replaces
(RLE + JSON + pycocotools + panopticapi) is not timed: neither package is available, so no speed-up is claimed."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _cc_reference as CC  # noqa: E402


def make_input(B, C, H=128, W=128, block=16, seed=0):
    rng = np.random.default_rng(seed)
    gt = np.stack([CC.blocky(rng, H, W, C, block) for _ in range(B)])
    pred = np.roll(gt, (2, 2), axis=(1, 2))
    redraw = np.stack([CC.blocky(rng, H, W, C, block) for _ in range(B)])
    pick = np.kron(rng.random((B, H // block, W // block)) < 0.05, np.ones((block, block), bool))
    return np.where(pick, redraw, pred).astype(np.int32), gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-instances", type=int, default=1024)
    ap.add_argument("--max-queries", type=int, default=100)
    a = ap.parse_args()

    import torch
    import maskunet_amd
    from maskunet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    B, H, W, M, K = a.batch, 128, 128, a.max_instances, a.max_queries
    thr = np.linspace(0.5, 0.95, 10)
    T = len(thr)
    for C in (19, 150):
        p_cls, g_cls = make_input(B, C)
        pred = maskunet_amd.instances_from_labels(torch.from_numpy(p_cls).to(dev), M)
        gt = maskunet_amd.instances_from_labels(torch.from_numpy(g_cls).to(dev), M)
        i32 = dict(dtype=torch.int32, device=dev)
        pairs, n_pairs = torch.empty((B, H * W, 3), **i32), torch.empty(B, **i32)
        o_i = [torch.empty((B, K), **i32) for _ in range(4)]                   # det_valid, det_class, pq_gt, pq_fp
        det_score = torch.empty((B, K), dtype=torch.float32, device=dev)
        det_gt, det_iou = torch.empty((B, T, K), **i32), torch.empty((B, T, K), dtype=torch.float64, device=dev)
        gt_per_class, pq_iou, overflow = torch.empty((B, C), **i32), torch.empty((B, K), dtype=torch.float64, device=dev), torch.empty(B, **i32)
        ws1 = torch.empty(lib.mu_instance_pairs_workspace_bytes(B, H, W, M, M), dtype=torch.uint8, device=dev)
        ws2 = torch.empty(lib.mu_instance_match_workspace_bytes(B, K), dtype=torch.uint8, device=dev)

        def run():
            _lib.call("mu_instance_pairs", pred.ids.data_ptr(), gt.ids.data_ptr(), B, H, W, M, M, pairs.data_ptr(), n_pairs.data_ptr(),
                      ws1.data_ptr(), ws1.numel(), _lib.stream())
            _lib.call("mu_instance_match", pairs.data_ptr(), n_pairs.data_ptr(), pred.table.data_ptr(), pred.scores.data_ptr(),
                      pred.order.data_ptr(), pred.count.data_ptr(), gt.table.data_ptr(), gt.count.data_ptr(), B, H, W, M, M, C, K, 100,
                      thr.ctypes.data, T, o_i[0].data_ptr(), o_i[1].data_ptr(), det_score.data_ptr(), det_gt.data_ptr(),
                      det_iou.data_ptr(), gt_per_class.data_ptr(), o_i[2].data_ptr(), pq_iou.data_ptr(), o_i[3].data_ptr(),
                      overflow.data_ptr(), ws2.data_ptr(), ws2.numel(), _lib.stream())

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
        print(f"shape B={B} {H}x{W} C={C} max_instances={M} max_queries={K} T={T}; instances per image: pred "
              f"{float(pred.count.float().mean()):.0f}, gt {float(gt.count.float().mean()):.0f}; pairs per image "
              f"{float(n_pairs.float().mean()):.0f}; coco matches at 0.5: {int((det_gt[:, 0] > 0).sum())}, panoptic: {int((o_i[2] > 0).sum())}, "
              f"overflow: {int(overflow.sum())}")
        print(f"mu_instance_pairs + mu_instance_match: median {statistics.median(ms):.3f} ms   min {min(ms):.3f}   max {max(ms):.3f}   "
              f"n={len(ms)}")


if __name__ == "__main__":
    main()
