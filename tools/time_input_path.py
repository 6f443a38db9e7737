#!/usr/bin/env python3
"""Time the three ways a training batch's voxels can reach the device, at the bench's shape (B = 4 clips x T = 16 frames x N = 20 000
float32 points), at 64^3 and 96^3:

  device   NeuralMarionette.voxelize_batch on sequences that are already in device memory (descriptor upload, grid clear, box,
           normalise + scatter): device events around the call
  host     the reference's per-clip numpy path (crop -> episodic_normalization -> voxelize, tests/input_path_ref.py) on this host, one
           process, numpy's own threading (the thread count of the run is printed): host clock
  copy     the pinned host -> device copy of the finished (B,T,1,G,G,G) fp32 batch ALONE: device events.  That copy is the least the
           host route can cost per step, whatever the host does to build the voxels.

Each figure is the median of --reps runs after --warmup runs; device and copy alternate in one process.  Expectation from byte counts
(not a measurement): the device call clears the B T G^3 x 4-byte grid and reads the 12 B T N bytes of points twice - 67 MB + 2 x 15 MB
at 64^3 - where the copy moves the whole grid over the host link.  The bar: device <= copy, measured in the same run.

  python tools/time_input_path.py [--out profiles/input_path_times.txt] [--grids 64 96] [--reps 20]
  rocprofv3 --kernel-trace --stats -d rocprof_out -- python tools/time_input_path.py --grids 64 --reps 3 --no-host     # kernel times
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import input_path_ref as IR  # noqa: E402
from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth  # noqa: E402
from neural_marionette_amd.data import ClipBank  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[64, 96])
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy path (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_input_path.py measures on the GPU: no device found")
    B, T, N = a.clips, a.frames, a.points
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    threads = os.environ.get("OMP_NUM_THREADS", "unset")
    say(f"input path, B = {B} clips x T = {T} frames x N = {N} float32 points; median of {a.reps} after {a.warmup} warm-up runs "
        f"(host: median of {a.host_reps}), ms;  {torch.cuda.get_device_name(0)};  host threads: OMP_NUM_THREADS = {threads}, "
        f"torch.get_num_threads() = {torch.get_num_threads()}, numpy element-wise arithmetic runs on one of them")
    seqs = [IR.sequence(901, b, T + 4, N, np.float32) for b in range(B)]
    starts = [b % 4 for b in range(B)]
    for G in a.grids:
        o = HotPathOptions(grid_size=G)
        net = NeuralMarionette(o)
        net.load_state_dict(synth.make_state_dict(o, seed=1))
        net = net.cuda().eval()
        bank = ClipBank("cuda")
        for p in seqs:
            bank.add(p)
        ids = list(range(B))
        host_ms, host_vox = [], None
        if not a.no_host:
            for rep in range(a.host_reps + 1):
                t0 = time.perf_counter()
                host_vox = np.stack([IR.clip(seqs[b], starts[b], T, 1, False, G)["vox"] for b in range(B)])
                if rep:
                    host_ms.append(1e3 * (time.perf_counter() - t0))
        staged = torch.empty(B, T, 1, G, G, G).pin_memory()
        if host_vox is not None:
            staged.copy_(torch.from_numpy(host_vox))
        dev_buf = torch.empty(B, T, 1, G, G, G, device="cuda")
        dev_ms, copy_ms = [], []
        for rep in range(a.reps + a.warmup):
            ms_d, out = event_ms(lambda: net.voxelize_batch(bank, ids, starts, T))
            ms_c, _ = event_ms(lambda: dev_buf.copy_(staged, non_blocking=True))
            if rep == 0 and host_vox is not None:
                assert torch.equal(out["vox"], dev_buf), "the device batch differs from the host-built one"
                assert int(out["bad_rows"].sum()) == 0
            del out
            if rep >= a.warmup:
                dev_ms.append(ms_d)
                copy_ms.append(ms_c)
        d, c = statistics.median(dev_ms), statistics.median(copy_ms)
        grid_mb, pts_mb = B * T * G ** 3 * 4 / 1e6, B * T * N * 12 / 1e6
        host = f"{statistics.median(host_ms):9.2f} (min {min(host_ms):.2f}, max {max(host_ms):.2f})" if host_ms else "not measured"
        say(f"{G}^3: device call {d:8.3f} (min {min(dev_ms):.3f}, max {max(dev_ms):.3f})   pinned copy of the {grid_mb:.0f} MB batch {c:8.3f} "
            f"(min {min(copy_ms):.3f}, max {max(copy_ms):.3f}) = {grid_mb / c:.1f} GB/s   numpy host path {host}   "
            f"points read {pts_mb:.0f} MB x 2;  device <= copy: {'yes' if d <= c else 'NO'} (x{c / d:.1f})")
        del net, bank, dev_buf, staged
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
