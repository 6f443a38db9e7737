#!/usr/bin/env python3
"""Time mesh sampling - the reference's offline preparation (dataset/dfaust/write_sequence_to_obj.py:107-115,
dataset/aistpp/prepare_aistpp.py:75-83: trimesh.sample.sample_surface(mesh, 20000) per frame) - at the size of the SMPL / D-FAUST
topology: T = 64 frames of V = 6890 vertices and F = 13776 faces (a closed synthetic mesh: a sphere of 84 rings x 82 segments and two
poles, pushed about per frame), count = 20000 samples a frame:

  a  sample    NeuralMarionette.sample_surface, float32 vertices, int32 triangles, seeded: device events
  b  tables    the same with return_tables=True (areas, cum and uniforms copied out): device events
  c  float64   a with float64 vertices and int64 triangles: device events
  d  pinned    what the step replaces on the device's side: the finished (T, count, 3) float32 points copied from pinned host memory: device events
  e  numpy     the float64 restatement tests/sample_ref.py on this host, all T frames, fed the device's areas: host clock, once, compared
               with the device's face indices and points

a .. d alternate in one process; each figure is the median of --reps runs after --warmup runs.  The kernels separately are kernel
times: run the tool under rocprofv3 in a run of its own and pass the statistics to the timed run, which appends them:

  rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -- python tools/time_sample_surface.py --reps 2 --warmup 1 --no-host
  python tools/time_sample_surface.py --kernel-stats rocprof_out/<host>/<pid>_kernel_stats.csv [--out profiles/sample_surface_times.txt]

No target is fixed and no ratio is asserted."""
from __future__ import annotations

import argparse
import csv
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth  # noqa: E402
import sample_ref as S  # noqa: E402

T, RINGS, SEGS, COUNT = 64, 84, 82, 20000
V, F = 2 + RINGS * SEGS, 2 * RINGS * SEGS
assert (V, F) == (6890, 13776)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def kernel_table(path):
    """the sample_* rows of rocprofv3's kernel statistics: name, calls, average ns"""
    rows = []
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            m = re.search(r"sample_[a-z_]+_kernel(?:<[\w ,]+>|I\w+E)?", rec.get("Name") or "")
            if m:
                rows.append((m.group(0), int(rec.get("Calls") or 0), float(rec.get("AverageNs") or 0.0)))
    return sorted(rows)


def scene():
    """a closed sphere mesh of V vertices and F faces in T poses: vertices (T,V,3) float64, triangles (F,3) int64"""
    lat = (np.arange(RINGS) + 1) * (np.pi / (RINGS + 1))
    lon = np.arange(SEGS) * (2 * np.pi / SEGS)
    ring = np.stack([np.sin(lat)[:, None] * np.cos(lon)[None], np.sin(lat)[:, None] * np.sin(lon)[None], np.cos(lat)[:, None] + 0 * lon[None]], -1)
    base = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    idx = 1 + np.arange(RINGS * SEGS).reshape(RINGS, SEGS)
    nxt = np.roll(idx, -1, axis=1)
    tri = [np.stack([np.zeros(SEGS, np.int64), idx[0], nxt[0]], 1), np.stack([np.full(SEGS, V - 1), nxt[-1], idx[-1]], 1)]
    for r in range(RINGS - 1):
        tri.append(np.stack([idx[r], idx[r + 1], nxt[r + 1]], 1))
        tri.append(np.stack([idx[r], nxt[r + 1], nxt[r]], 1))
    tri = np.concatenate(tri).astype(np.int64)
    assert base.shape == (V, 3) and tri.shape == (F, 3)
    frames = []
    for t in range(T):
        s = np.array([1.0 + 0.3 * np.sin(0.2 * t), 1.0 + 0.2 * np.cos(0.15 * t), 1.6])
        frames.append(base * s * (1.0 + 0.1 * np.sin(3.0 * base[:, :1] + 0.1 * t)) + np.array([0.02 * t, 0.0, 0.0]))
    return np.stack(frames), tri


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (profiler runs)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats kernel statistics CSV of an earlier run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sample_surface.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"mesh sampling, {T} frames of {V} vertices and {F} faces, {COUNT} samples a frame; median of {a.reps} after {a.warmup} warm-up runs, ms;  "
        f"{torch.cuda.get_device_name(0)};  host threads: OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}")
    o = HotPathOptions(grid_size=32)
    net = NeuralMarionette(o)
    net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
    net = net.cuda().eval()
    dev = net._engine.ready().device
    v64, tri64 = scene()
    v32 = v64.astype(np.float32)
    dv32, dt32 = torch.from_numpy(v32).to(dev), torch.from_numpy(tri64.astype(np.int32)).to(dev)
    dv64, dt64 = torch.from_numpy(v64).to(dev), torch.from_numpy(tri64).to(dev)
    first = net.sample_surface(dv32, dt32, count=COUNT, seed=1, return_tables=True, check=True)
    pinned = first["points"].cpu().pin_memory()
    landing = torch.empty_like(first["points"])
    ms = {k: [] for k in "abcd"}
    for rep in range(a.reps + a.warmup):
        t_a, out = event_ms(lambda: net.sample_surface(dv32, dt32, count=COUNT, seed=1))
        t_b, outb = event_ms(lambda: net.sample_surface(dv32, dt32, count=COUNT, seed=1, return_tables=True))
        t_c, outc = event_ms(lambda: net.sample_surface(dv64, dt64, count=COUNT, seed=1))
        t_d, _ = event_ms(lambda: landing.copy_(pinned, non_blocking=True))
        if rep == 0:
            assert torch.equal(out["points"], first["points"]) and torch.equal(outb["cum"], first["cum"]) and torch.equal(landing, first["points"])
        del out, outb, outc
        if rep >= a.warmup:
            for k, x in zip("abcd", (t_a, t_b, t_c, t_d)):
                ms[k].append(x)
    med = {k: statistics.median(x) for k, x in ms.items()}
    mb = T * COUNT * 12 / 1e6
    say(f"a sample {med['a']:8.3f} (min {min(ms['a']):.3f}, max {max(ms['a']):.3f}) = {1e3 * med['a'] / T:.1f} us a frame, {T * COUNT / med['a'] / 1e6:.2f} million samples a ms   "
        f"b tables {med['b']:8.3f} (min {min(ms['b']):.3f})   c float64 / int64 {med['c']:8.3f} (min {min(ms['c']):.3f})   "
        f"d pinned copy of the finished points ({mb:.1f} MB) {med['d']:8.3f} (min {min(ms['d']):.3f}) = {mb / med['d']:.1f} GB/s   a / d {med['a'] / med['d']:.2f}")
    say("occupancy: sample_faces_kernel is compiled to 27 - 29 VGPRs, sample_scan_kernel to 44, sample_draw_kernel to 37 - 44 VGPRs and 16 384 B of LDS a "
        "workgroup (hipcc -Rpass-analysis=kernel-resource-usage: 8 waves a SIMD for all, no scratch), so registers and LDS admit the eight workgroups a "
        "CU's 32 wavefront slots hold; the occupancy ACHIEVED on the device (a counter run) was not looked at")
    if not a.no_host:
        areas, used = first["areas"].cpu().numpy(), first["uniforms"].cpu().numpy()
        t0 = time.perf_counter()
        ref = S.sample(v32, tri64, used, areas=areas)
        t_e = 1e3 * (time.perf_counter() - t0)
        same = np.array_equal(ref["face_index"], first["face_index"].cpu().numpy()) and np.array_equal(ref["points"], first["points"].cpu().numpy())
        t0 = time.perf_counter()
        S.uniforms(1, T, COUNT)
        t_u = 1e3 * (time.perf_counter() - t0)
        say(f"e numpy {t_e:9.1f} for all {T} frames with the uniforms given (+ {t_u:.1f} for Philox in numpy); face indices and points equal to the device's: {same};  "
            f"e / a {t_e / med['a']:.0f}")
    else:
        say("e numpy not measured")
    if a.kernel_stats:
        say(f"kernel times of an earlier run under rocprofv3 --kernel-trace --stats ({os.path.basename(a.kernel_stats)}; all calls of that run together), "
            f"average per launch, ms:")
        for name, calls, avg in kernel_table(a.kernel_stats):
            say(f"  {name:44s} {calls:6d} launches   {avg / 1e6:8.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
