"""Times the ground-truth instances from dataset id maps (mu_id_instances) on two inputs:
  (a) B = 64, 128x128, blocky 16x16 regions with Cityscapes values class * 1000 + k, 19 classes: the evaluation shape;
  (b) B = 64, 256x256, every pixel a distinct id: the worst case of the sort (65536 keys, four live bytes) and of the bisection.

    python tools/bench_idmap.py [--batch 64] [--reps 20] [--out profiles/idmap_bench.txt]

HIP events on the launch stream around the raw call (buffers allocated beforehand), 3 warm-up calls, median / min / max.  For scale
only, by a host clock on the same machine: tests/_idmap_reference.py (numpy) on the same input, and mu_instances on the class map of
(a) -- a different partition, but the neighbouring producer.  No speed-up against the host is claimed from numpy figures."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import _cc_reference as CC  # noqa: E402
from tests import _idmap_reference as R  # noqa: E402


def blocky_input(B, C=19, H=128, W=128, block=16, seed=0):
    rng = np.random.default_rng(seed)
    sem = np.stack([CC.blocky(rng, H, W, C, block) for _ in range(B)]).astype(np.int32)
    k = np.kron(rng.integers(0, 30, (B, H // block, W // block)), np.ones((block, block), np.int64))
    return np.where(sem > 0, sem.astype(np.int64) * 1000 + k, 0).astype(np.int32), sem


def distinct_input(B, H=256, W=256, seed=1):
    rng = np.random.default_rng(seed)
    v = np.stack([rng.permutation(H * W).reshape(H, W) for _ in range(B)]).astype(np.int64)
    v = (v * 65521 + 12345) % (2 ** 32) - 2 ** 31                      # distinct (an odd multiplier modulo 2^32), all four bytes in use
    v[v == 0] = 2 ** 31 - 1 - 65536 * 3                                # (not produced by the map above for these inputs: checked below)
    assert all(len(np.unique(v[b])) == H * W for b in range(B))
    return v.astype(np.int32), rng.integers(0, 19, v.shape).astype(np.int32)


def events(torch, run, warm, reps):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-instances", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from maskunet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    B, M = a.batch, a.max_instances
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device: {torch.cuda.get_device_name(0)}; HIP events, 3 warm-up + {a.reps} timed calls")
    for name, (v, sem), cap in (("(a) blocky 128x128", blocky_input(B), 256), ("(b) distinct 256x256", distinct_input(B), 256)):
        _, H, W = sem.shape
        i32 = dict(dtype=torch.int32, device=dev)
        tv, ts = torch.from_numpy(v).to(dev), torch.from_numpy(sem).to(dev)
        ids, table, count, order = torch.empty((B, H, W), **i32), torch.empty((B, M, 8), **i32), torch.empty(B, **i32), torch.empty((B, M), **i32)
        score, values, invalid = torch.empty((B, M), dtype=torch.float32, device=dev), torch.empty((B, M), **i32), torch.empty(B, **i32)
        ws = torch.empty(lib.mu_id_instances_workspace_bytes(B, H, W, M, cap), dtype=torch.uint8, device=dev)

        def run():
            _lib.call("mu_id_instances", tv.data_ptr(), _lib.MU_IDMAP_I32, ts.data_ptr(), B, H, W, M, cap, ids.data_ptr(), table.data_ptr(),
                      score.data_ptr(), count.data_ptr(), order.data_ptr(), values.data_ptr(), invalid.data_ptr(), ws.data_ptr(),
                      ws.numel(), _lib.stream())

        ms = events(torch, run, 3, a.reps)
        t0 = time.perf_counter()
        ref = R.instances(v, sem, M, cap)
        host = (time.perf_counter() - t0) * 1e3
        ok = all(np.array_equal(ref[k], t.cpu().numpy()) for k, t in (("ids", ids), ("table", table), ("count", count), ("values", values)))
        say(f"{name}: B={B} max_instances={M} class_cap={cap}; instances per image {float(count.float().mean()):.0f}; workspace "
            f"{ws.numel() / 2 ** 20:.1f} MiB; equal to the numpy restatement: {ok}")
        say(f"  mu_id_instances: median {statistics.median(ms):.3f} ms   min {min(ms):.3f}   max {max(ms):.3f}   n={len(ms)}")
        say(f"  tests/_idmap_reference.py on the same input, host clock, for scale only: {host:.1f} ms")
        if name.startswith("(a)"):
            ws2 = torch.empty(lib.mu_instances_workspace_bytes(B, H, W, M), dtype=torch.uint8, device=dev)

            def run_cc():
                _lib.call("mu_instances", ts.data_ptr(), None, B, H, W, M, ids.data_ptr(), table.data_ptr(), score.data_ptr(),
                          count.data_ptr(), order.data_ptr(), ws2.data_ptr(), ws2.numel(), _lib.stream())

            ms = events(torch, run_cc, 3, a.reps)
            say(f"  mu_instances on the class map of (a), for scale only: median {statistics.median(ms):.3f} ms   min {min(ms):.3f}   "
                f"max {max(ms):.3f}   ({float(count.float().mean()):.0f} components per image)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
