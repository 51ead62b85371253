"""Times the fused semantic-evaluation sweep (mu_sem_eval) against the three sweeps it replaces, in one process on the same tensors:
B = 64, 128x128, fp16 NHWC channel-padded logits, at c_out = 150 (Cp = 160) and c_out = 19 (Cp = 32).

  mu_sem_eval with and without cls / prob (every buffer allocated beforehand; what is timed is the memset and the two launches);
  mu_ce_fwd, mu_mean_iou and mu_argmax_prob on the same logits and labels, and the sum of their medians;
  the share of HBM bandwidth from algorithmic bytes: the logits once, 8 bytes of labels per pixel, 8 bytes out per pixel when cls
  and prob are written.

Prints one line per figure: median of `--reps` measurements (HIP events, warm), with minimum and maximum, and per class count
whether the fused median is no larger than the sum of the three.

    python tools/bench_sem_eval.py [--batch 64] [--reps 20]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from maskunet_amd import _lib  # noqa: E402
from tools.bench_instances import HBM_PEAK, show, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    B, H, W = a.batch, 128, 128
    HW, M = H * W, a.batch * H * W
    dev = torch.device("cuda")
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    for C, Cp in ((150, 160), (19, 32)):
        # post-ReLU noise plus a 6.0 on a blocky class map, labels = that map with a tenth of the pixels void: a trained model's output
        cls_map = torch.randint(0, C, (B, H // 8, W // 8), device=dev, generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        x = torch.zeros(B, H, W, Cp, dtype=torch.float16, device=dev)
        x[..., :C] = torch.relu(torch.randn(B, H, W, C, device=dev, generator=g)).half()
        x.scatter_add_(3, cls_map[..., None], torch.full((B, H, W, 1), 6.0, dtype=torch.float16, device=dev))
        labels = torch.where(torch.rand(B, H, W, device=dev, generator=g) < 0.1, torch.full_like(cls_map, 255), cls_map).contiguous()
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        img_counts, img_loss = torch.empty((B, 3, C), **i32), torch.empty((B, 2), dtype=torch.float64, device=dev)
        conf = torch.zeros((C + 1, C), dtype=torch.int64, device=dev)
        cls_d, prob_d = torch.empty(M, **i32), torch.empty(M, **f32)
        nws = lib.mu_sem_eval_workspace_bytes(B, HW, C)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        lse, loss, count = torch.empty(M, **f32), torch.empty(1, **f32), torch.empty(1, **f32)
        ce_ws = torch.empty(lib.mu_ce_workspace_bytes(), dtype=torch.uint8, device=dev)
        counts, miou = torch.empty(3 * C, **i32), torch.empty(1, **f32)
        dt = _lib.dt(x)

        def fused(with_out):
            c, p = (cls_d.data_ptr(), prob_d.data_ptr()) if with_out else (None, None)
            return lambda: _lib.call("mu_sem_eval", x.data_ptr(), labels.data_ptr(), B, HW, C, M, 0, 1, Cp, 255, 2.0, img_counts.data_ptr(),
                                     img_loss.data_ptr(), conf.data_ptr(), c, p, ws.data_ptr(), nws, dt, _lib.stream())

        print(f"--- B={B} {H}x{W} C={C} Cp={Cp} fp16 NHWC ---")
        med = {}
        for name, fn, nbytes in [("mu_sem_eval", fused(False), M * Cp * 2 + M * 8), ("mu_sem_eval + cls + prob", fused(True), M * Cp * 2 + M * 16)]:
            ms = timed(fn, a.reps)
            m = statistics.median(ms)
            med[name] = show(name, ms, f"  {nbytes / m / 1e9:.2f} TB/s = {100 * nbytes / (m * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
        three = [
            ("mu_ce_fwd", lambda: _lib.call("mu_ce_fwd", x.data_ptr(), labels.data_ptr(), M, Cp, C, 255, lse.data_ptr(), loss.data_ptr(),
                                            count.data_ptr(), ce_ws.data_ptr(), ce_ws.numel(), dt, _lib.stream())),
            ("mu_mean_iou", lambda: _lib.call("mu_mean_iou", x.data_ptr(), labels.data_ptr(), M, C, M, 0, 1, Cp, 1e-6, counts.data_ptr(),
                                              miou.data_ptr(), dt, _lib.stream())),
            ("mu_argmax_prob", lambda: _lib.call("mu_argmax_prob", x.data_ptr(), M, C, M, 0, 1, Cp, 2.0, cls_d.data_ptr(), prob_d.data_ptr(),
                                                 dt, _lib.stream())),
        ]
        total = sum(show(name, timed(fn, a.reps)) for name, fn in three)
        for name in med:
            verdict = "no larger" if med[name] <= total else "LARGER"
            print(f"{name}: {med[name]:.3f} ms against {total:.3f} ms for the three sweeps: {verdict} ({med[name] / total:.2f} x)", flush=True)
        assert int(conf.sum()) > 0 and int(img_counts[:, 1].sum()) == M       # the sweep did count (read back after the timing)


if __name__ == "__main__":
    main()
