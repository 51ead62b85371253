"""Times panoptic_segments (mu_panoptic) beside the predict_instances call it follows, at the evaluation shape: B = 64, 128x128, 150
classes (ADE20K's count; the first 100 stuff, the rest things, class 0 void), fp16 logits whose arg-max is blocky (16x16 cells).

    python tools/bench_panoptic.py [--batch 64] [--reps 20] [--out profiles/panoptic_bench.txt]

HIP events on the current stream around `--inner` back-to-back calls through the Python API (output tensors come from torch's caching
allocator, as a user's call does), 3 warm-up rounds, median / min / max per call.  A second line times the raw entry point alone on
preallocated buffers.  The first images are compared with tests/_panoptic_reference.py.  Information, not a threshold."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _panoptic_reference as R  # noqa: E402


def events(torch, run, warm, reps, inner):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import maskunet_amd
    from maskunet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    B, C, H, W, M, S, cell = a.batch, a.classes, a.size, a.size, 1024, 1024, 16
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cpu").manual_seed(0)
    cls = torch.randint(0, C, (B, H // cell, W // cell), generator=g).repeat_interleave(cell, 1).repeat_interleave(cell, 2)
    logits = (torch.randn((B, C, H, W), generator=g) * 0.3).scatter_add_(1, cls[:, None], torch.full((B, 1, H, W), 2.0)).half().to(dev)
    things = tuple(c >= 100 for c in range(C))
    fmt = lambda ms: f"median {statistics.median(ms) * 1e3:.1f} us   min {min(ms) * 1e3:.1f}   max {max(ms) * 1e3:.1f}   n={len(ms)} x {a.inner} calls"

    say(f"device: {torch.cuda.get_device_name(0)}; B={B} {H}x{W}, {C} classes, fp16 logits, max_instances={M}, max_segments={S}")
    inst = maskunet_amd.predict_instances(logits, max_instances=M)
    pan = maskunet_amd.panoptic_segments(inst, things, max_segments=S)
    say(f"instances per image {float(inst.count.float().mean()):.0f}, segments per image {float(pan.count.float().mean()):.0f}, "
        f"invalid {sorted(set(pan.invalid.tolist()))}")
    kind = np.array([0] + [2 if t else 1 for t in things[1:]], np.int32)
    n = min(B, 2)
    ref = R.segments(inst.classes[:n].cpu().numpy(), inst.ids[:n].cpu().numpy(), inst.table[:n].cpu().numpy(), inst.scores[:n].cpu().numpy(),
                     inst.count[:n].cpu().numpy(), kind, np.arange(C, dtype=np.int32), max_seg=S)
    got = {"seg": pan.seg, "table": pan.table, "values": pan.values, "order": pan.order, "rgb": pan.rgb, "count": pan.count}
    say(f"equal to the numpy restatement on the first {n} images: {all(np.array_equal(ref[k], t[:n].cpu().numpy()) for k, t in got.items())}")

    say("predict_instances(logits):       " + fmt(events(torch, lambda: maskunet_amd.predict_instances(logits, max_instances=M), 3, a.reps, a.inner)))
    say("panoptic_segments(inst, things): " + fmt(events(torch, lambda: maskunet_amd.panoptic_segments(inst, things, max_segments=S), 3, a.reps, a.inner)))
    ws = torch.empty(lib.mu_panoptic_workspace_bytes(B, H, W, M, C, S), dtype=torch.uint8, device=dev)
    kind_t, cat_t = torch.from_numpy(kind).to(dev), pan.category
    outs = (pan.seg, pan.seg_cls, pan.table, pan.scores, pan.count, pan.order, pan.source, pan.values, pan.id_map, pan.rgb, pan.invalid)

    def raw():
        _lib.call("mu_panoptic", inst.classes.data_ptr(), inst.ids.data_ptr(), inst.table.data_ptr(), inst.scores.data_ptr(),
                  inst.count.data_ptr(), kind_t.data_ptr(), cat_t.data_ptr(), B, H, W, M, C, 1000, 0, 0, 0.0, S, 0,
                  *(t.data_ptr() for t in outs), ws.data_ptr(), ws.numel(), _lib.stream())

    say("mu_panoptic alone (raw call):    " + fmt(events(torch, raw, 3, a.reps, a.inner)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
