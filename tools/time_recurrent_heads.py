#!/usr/bin/env python3
"""Time options.const_intensity 2 (recurrent heat-maps: heat_scan_kernel + heat_marginals_kernel / heat_bwd_recurrent_kernel) against 3 at the headline
shape - 64^3, B = 4, T = 16, conv mode 'split16': the full inference forward and one detector training step, the two options alternating
in one process after warm-up, device events around each call, median and spread (min .. max) over --reps repeats each.  The convolution
work of the two options is identical, so the difference is the heads stage.

  python tools/time_recurrent_heads.py [--reps 20] [--out profiles/recurrent_heads_times.txt]
  NM355_LIB_PATH=<another build of libnm355.so> python tools/time_recurrent_heads.py --values 3      # the default path on that library
  rocprofv3 --kernel-trace --stats -d rocprof_out -- python tools/time_recurrent_heads.py --reps 3    # kernel times of their own

The heads stage itself (heat-map + keypoints launches; in the backward heat_bwd_prep + the heat kernel + its reductions) sits between two
launches of one library call, where no event can be placed from outside: its time is the sum of those kernels' durations in the
rocprofv3 kernel trace, a run of its own (--reps 3 keeps the trace small)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth, _lib  # noqa: E402
from neural_marionette_amd.train import DetectorTrainer  # noqa: E402

ACTS = {"detector": True, "learner": True}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return "%8.3f ms (min %8.3f, max %8.3f, n = %d)" % (float(np.median(v)), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--values", type=int, nargs="+", default=[3, 2], help="const_intensity values to alternate (a library without the switch: 3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G, B, T = a.grid, a.batch, a.frames
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = synth.make_state_dict(HotPathOptions(grid_size=G), seed=430, variant="peaky")
    vox = synth.figure_clip(B, T, G, seed=432).cuda()
    eps = synth.make_eps((T, 10, B, 128), seed=433).cuda()
    say(f"const_intensity {' / '.join(map(str, a.values))}: {G}^3, B = {B}, T = {T}, conv mode split16, library {os.path.basename(_lib.LIB_PATH)}; "
        f"device events around each call, alternating, {a.warmup} warm-up rounds")
    nets, trainers = {}, {}
    for v in a.values:
        o = HotPathOptions(grid_size=G, const_intensity=v)
        n = NeuralMarionette(o); n.load_state_dict(sd); n = n.cuda().eval(); n.set_conv_mode("split16"); n.anneal(1)
        nets[v] = n
        m = NeuralMarionette(o); m.load_state_dict(sd); m = m.cuda().train(); m.set_conv_mode("split16"); m.anneal(1)
        trainers[v] = DetectorTrainer(m, lr=4e-4)
    fwd = {v: [] for v in a.values}
    step = {v: [] for v in a.values}
    with torch.no_grad():
        for v in a.values:
            nets[v](vox, ACTS, eps=eps)                      # builds the tree: later calls are the fused forward
        for rep in range(a.reps + a.warmup):
            for v in a.values:
                ms = timed(lambda: nets[v](vox, ACTS, eps=eps))
                if rep >= a.warmup:
                    fwd[v].append(ms)
    for rep in range(a.reps + a.warmup):
        for v in a.values:
            ms = timed(lambda: trainers[v].step(vox))
            if rep >= a.warmup:
                step[v].append(ms)
    for v in a.values:
        say(f"const_intensity {v}: forward {stats(fwd[v])}   training step {stats(step[v])}")
    if len(a.values) == 2:
        p, q = a.values
        df, ds = float(np.median(fwd[q]) - np.median(fwd[p])), float(np.median(step[q]) - np.median(step[p]))
        say(f"const_intensity {q} - {p}: forward {df * 1e3:+.0f} us ({100 * df / float(np.median(fwd[p])):+.2f} % of the forward), "
            f"training step {ds * 1e3:+.0f} us ({100 * ds / float(np.median(step[p])):+.2f} % of the step)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
