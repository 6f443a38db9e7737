#!/usr/bin/env python3
"""Time the ways a batch of decoded voxels can become the ordered point sets its consumers want (vis_generation.py:137-170,
vis_interpolation.py:141-177, vis/visualize.py:130-137), at three shapes: S = 3 samples x T = 30 frames at 64^3 (the generation
demo), B = 4 x T = 16 at 64^3 and B = 2 x T = 8 at 96^3, on synth clips pushed through the detector's decoder ('recon') or on their
input occupancy ('input'):

  a  exact     NeuralMarionette.occupied_points, exact-sized (one read of offsets[-1]: the call's one synchronisation), float64 with
               depth: device events around the call
  b  capacity  the same with capacity = the number of points rounded up to 4096 (no synchronisation): device events
  c  where     the per-frame loop of vis_recon on the device: binarise, then torch.stack(torch.where(x[b, t, 0]), -1) / ((G - 1) / 2)
               - 1 per frame (one synchronisation per frame inside torch.where): device events
  d  copy      the pinned device -> host copy of the dense (B,T,1,G,G,G) fp32 tensor ALONE: device events.  The least the host
               route can cost, whatever the host then does
  e  numpy     that copy plus the scripts' numpy lines on the host (binarise, np.where per frame in two passes, min_z / max_z, the
               per-point depth as one array expression per frame): host clock

Each figure is the median of --reps runs after --warmup runs; a, b, c and d alternate in one process.  The bar: a <= d in the same run.

  python tools/time_output_path.py [--out profiles/output_path_times.txt] [--reps 20] [--sources recon input]
  rocprofv3 --kernel-trace --stats -d rocprof_out -- python tools/time_output_path.py --reps 3 --no-host --sources input     # kernel times
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

from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth  # noqa: E402

SHAPES = ((3, 30, 64), (4, 16, 64), (2, 8, 96))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def where_loop(x, scratch):
    """vis_recon's lines (visualize.py:130-137) on the device"""
    scratch.copy_(x)
    scratch[scratch < 0.5] = 0
    scratch[scratch >= 0.5] = 1
    B, T, G = x.shape[0], x.shape[1], x.shape[3]
    return [torch.stack(torch.where(scratch[b, t, 0]), dim=-1) / ((G - 1) / 2) - 1 for b in range(B) for t in range(T)]


def numpy_lines(host):
    """vis_generation.py:138-170 without the drawing, on the host copy"""
    x = host.clone()
    x[x < 0.5] = 0
    x[x >= 0.5] = 1
    B, T, G = x.shape[0], x.shape[1], x.shape[3]
    n = 0
    for b in range(B):
        min_z, max_z = 1e4, -1
        for t in range(T):
            coords = np.stack(np.where(x[b, t, 0].numpy()), axis=-1) / ((G - 1) / 2) - 1
            if len(coords):
                min_z, max_z = min(min_z, coords[:, -1].min()), max(max_z, coords[:, -1].max())
        z_len = max_z - min_z
        for t in range(T):
            coords = np.stack(np.where(x[b, t, 0].numpy()), axis=-1) / ((G - 1) / 2) - 1
            with np.errstate(invalid="ignore", divide="ignore"):
                depth = (coords[:, -1] - min_z) / z_len
            n += len(depth)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sources", nargs="+", default=["recon", "input"], choices=["recon", "input"])
    ap.add_argument("--no-host", action="store_true", help="skip the numpy lines (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_output_path.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"output path; median of {a.reps} after {a.warmup} warm-up runs (numpy: median of {a.host_reps}), ms;  {torch.cuda.get_device_name(0)};  "
        f"host threads: OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}, torch.get_num_threads() = {torch.get_num_threads()}")
    nets = {}
    for B, T, G in SHAPES:
        if G not in nets:
            o = HotPathOptions(grid_size=G)
            net = NeuralMarionette(o)
            net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
            nets[G] = net.cuda().eval()
            nets[G].anneal(1)
        net = nets[G]
        occ = synth.figure_clip(B, T, G, seed=3).cuda()
        for source in a.sources:
            if source == "recon":
                with torch.no_grad():
                    x = torch.cat([net.kypt_detector(occ[b:b + 1])["recon"] for b in range(B)]).contiguous()
            else:
                x = occ
            scratch = torch.empty_like(x)
            staged = torch.empty(x.shape).pin_memory()
            total = int((~(x < 0.5)).sum())
            cap = (total + 4095) // 4096 * 4096
            kw = dict(return_depth=True)
            ms = {k: [] for k in "abcd"}
            for rep in range(a.reps + a.warmup):
                t_a, out = event_ms(lambda: net.occupied_points(x, 0.5, **kw))
                t_b, outb = event_ms(lambda: net.occupied_points(x, 0.5, capacity=cap, **kw))
                t_c, pts = event_ms(lambda: where_loop(x, scratch))
                t_d, _ = event_ms(lambda: staged.copy_(x, non_blocking=True))
                if rep == 0:
                    assert len(out["coords"]) == total == sum(len(p) for p in pts)
                    assert torch.equal(out["coords"], outb["coords"][:total]) and torch.equal(out["offsets"], outb["offsets"])
                del out, outb, pts
                if rep >= a.warmup:
                    for k, v in zip("abcd", (t_a, t_b, t_c, t_d)):
                        ms[k].append(v)
            host = []
            if not a.no_host:
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    assert numpy_lines(staged) == total
                    host.append(1e3 * (time.perf_counter() - t0))
            med = {k: statistics.median(v) for k, v in ms.items()}
            mb = x.numel() * 4 / 1e6
            e = f"{med['d'] + statistics.median(host):9.1f}" if host else "not measured"
            say(f"{B} x {T} at {G}^3, {source:5s}: {total:8d} points = {100.0 * total / x.numel():.2f} % of {mb:.0f} MB   "
                f"a exact {med['a']:7.3f} (min {min(ms['a']):.3f}, max {max(ms['a']):.3f})   b capacity {med['b']:7.3f} (min {min(ms['b']):.3f})   "
                f"c where-loop {med['c']:8.3f}   d pinned copy {med['d']:7.3f} (min {min(ms['d']):.3f}, max {max(ms['d']):.3f}) = {mb / med['d']:.1f} GB/s   "
                f"e copy + numpy {e}   a <= d: {'yes' if med['a'] <= med['d'] else 'NO'} (x{med['d'] / med['a']:.1f})")
            del x, scratch, staged
        del occ
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
