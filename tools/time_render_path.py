#!/usr/bin/env python3
"""Time the render path - the plates of the surface path drawn as flat discs through a pinhole camera (vis_generation.py:171-190,
vis_interpolation.py:177-185: a cylinder per plate into open3d's off-screen visualiser) - at B = 4 clips x T = 16 frames of 64^3
through the golden camera (tests/golden/camera_source.json, 1025 x 958 pixels, radius 0.03), on synth clips pushed through the
detector's decoder ('recon') or on their input occupancy ('input'):

  a  frames    NeuralMarionette.render_frames, exact-sized (two reads: the number of points and the number of list entries): device
               events around the call
  b  surface   NeuralMarionette.surface_points alone, with colours - what a contains before the renderer: device events
  c  plates    NeuralMarionette.render_plates on b's points, exact-sized (one read): device events
  d  capacity  the same with bin_capacity = the number of list entries rounded up to 4096 (no synchronisation): device events
  e  bin       nm_render_bin alone through the C ABI (transform, count, scan): device events
  f  draw      nm_render_draw alone through the C ABI (fill, draw), all three outputs: device events
  g  numpy     the float64 restatement tests/render_ref.py on this host, on frame 0 of clip 0 CROPPED to a window of --crop x --crop
               pixels about the middle of what the frame covers (a whole 1025 x 958 frame against some thousand plates takes minutes):
               host clock, once, compared with the device's index map on the window

a .. f alternate in one process; each figure is the median of --reps runs after --warmup runs.  transform / count / scan / fill / draw
separately are kernel times: run the tool under rocprofv3 in a run of its own and pass the statistics to the timed run, which appends them:

  rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -- python tools/time_render_path.py --reps 3 --no-host --sources input
  python tools/time_render_path.py --kernel-stats rocprof_out/<host>/<pid>_kernel_stats.csv [--out profiles/render_path_times.txt]

No target is fixed."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
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

from neural_marionette_amd import NeuralMarionette, HotPathOptions, PinholeCamera, synth  # noqa: E402
import render_ref as RR  # noqa: E402

B, T, G = 4, 16, 64
BASE, SHADE, RADIUS = (0.6, 1.0, 0.6), (0.8, 0.2), 0.03


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def kernel_table(path):
    """the render_* rows of rocprofv3's kernel statistics: name, calls, average ns"""
    rows = []
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            m = re.search(r"render_[a-z_]+(?:<\w+>|ILb[01]E)?", rec.get("Name") or "")
            if m:
                rows.append((m.group(0).replace("ILb0E", "<false>").replace("ILb1E", "<true>"), int(rec.get("Calls") or 0), float(rec.get("AverageNs") or 0.0)))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--crop", type=int, default=96)
    ap.add_argument("--sources", nargs="+", default=["recon", "input"], choices=["recon", "input"])
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (profiler runs)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats kernel statistics CSV of an earlier run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_render_path.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cam = PinholeCamera.from_open3d(os.path.join(ROOT, "tests", "golden", "camera_source.json"))
    H, W = cam.height, cam.width
    say(f"render path, {B} x {T} frames at {G}^3 through the golden camera, {W} x {H} pixels, radius {RADIUS}, radius2 = 6; median of {a.reps} after "
        f"{a.warmup} warm-up runs, ms;  {torch.cuda.get_device_name(0)};  host threads: OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}")
    o = HotPathOptions(grid_size=G)
    net = NeuralMarionette(o)
    net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
    net = net.cuda().eval()
    net.anneal(1)
    eng = net._engine
    occ = synth.figure_clip(B, T, G, seed=3).cuda()
    base_dev = torch.from_numpy(np.tile(BASE, (B * T, 1))).cuda()              # on the device already: the calls copy nothing from the host
    F = B * T
    nt = F * ((W + 15) // 16) * ((H + 15) // 16)
    cs = cam.c_struct()
    for source in a.sources:
        if source == "recon":
            with torch.no_grad():
                x = torch.cat([net.kypt_detector(occ[b:b + 1])["recon"] for b in range(B)]).contiguous()
        else:
            x = occ
        kw = dict(base_colors=base_dev, shade=SHADE)
        pts = net.surface_points(x, 0.5, **kw)
        N = int(pts["plates"].shape[0])
        first = net.render_plates(pts, cam, radius=RADIUS, return_index=True, return_depth=True)
        total = int(first["bin_total"])
        cap = (total + 4095) // 4096 * 4096
        xf = torch.empty(N, 8, device="cuda", dtype=torch.float64)
        rect = torch.empty(N, 4, device="cuda", dtype=torch.int32)
        toff = torch.empty(nt + 1, device="cuda", dtype=torch.int64)
        lst = torch.empty(cap, device="cuda", dtype=torch.int32)
        index = torch.empty(F, H, W, device="cuda", dtype=torch.int32)
        depth = torch.empty(F, H, W, device="cuda", dtype=torch.float64)
        image = torch.empty(F, H, W, 3, device="cuda", dtype=torch.uint8)

        def run_bin():
            eng.call("nm_render_bin", pts["plates"].data_ptr(), pts["offsets"].data_ptr(), F, N, C.byref(cs), RADIUS, xf.data_ptr(), rect.data_ptr(),
                     toff.data_ptr())

        def run_draw():
            eng.call("nm_render_draw", xf.data_ptr(), rect.data_ptr(), pts["offsets"].data_ptr(), toff.data_ptr(), pts["colors"].data_ptr(), F, N,
                     C.byref(cs), RADIUS, 1.0, 0.0, None, cap, lst.data_ptr(), index.data_ptr(), depth.data_ptr(), image.data_ptr())

        ms = {k: [] for k in "abcdef"}
        for rep in range(a.reps + a.warmup):
            t_a, out = event_ms(lambda: net.render_frames(x, cam, 0.5, radius=RADIUS, **kw))
            t_b, _ = event_ms(lambda: net.surface_points(x, 0.5, **kw))
            t_c, outc = event_ms(lambda: net.render_plates(pts, cam, radius=RADIUS))
            t_d, outd = event_ms(lambda: net.render_plates(pts, cam, radius=RADIUS, bin_capacity=cap))
            t_e, _ = event_ms(run_bin)
            t_f, _ = event_ms(run_draw)
            if rep == 0:
                assert torch.equal(out["image"], first["image"]) and torch.equal(outc["image"], first["image"]) and torch.equal(outd["image"], first["image"])
                assert torch.equal(image.view_as(first["image"]), first["image"]) and torch.equal(index.view_as(first["index"]), first["index"])
                assert int(toff[-1]) == total
            del out, outc, outd
            if rep >= a.warmup:
                for k, v in zip("abcdef", (t_a, t_b, t_c, t_d, t_e, t_f)):
                    ms[k].append(v)
        med = {k: statistics.median(v) for k, v in ms.items()}
        covered = float((first["index"] >= 0).float().mean())
        host = "g numpy not measured"
        if not a.no_host:
            idx0 = first["index"][0, 0].cpu().numpy()
            ys, xs = np.nonzero(idx0 >= 0)
            my, mx = ((int(ys.min()) + int(ys.max())) // 2, (int(xs.min()) + int(xs.max())) // 2) if len(ys) else (H // 2, W // 2)
            y0, x0 = max(0, min(H - a.crop, my - a.crop // 2)), max(0, min(W - a.crop, mx - a.crop // 2))
            crop = (x0, x0 + a.crop, y0, y0 + a.crop)
            n0 = int(pts["offsets"][1])
            plates0, colors0 = pts["plates"][:n0].cpu().numpy(), pts["colors"][:n0].cpu().numpy()
            t0 = time.perf_counter()
            ref = RR.render(plates0, [0, n0], colors0, cam, radius=RADIUS, crop=crop)
            t_g = 1e3 * (time.perf_counter() - t0)
            win = (slice(y0, y0 + a.crop), slice(x0, x0 + a.crop))
            same = np.array_equal(ref["index"][0], idx0[win]) and np.array_equal(ref["image"][0], first["image"][0, 0].cpu().numpy()[win])
            share = a.crop * a.crop / (H * W)
            host = (f"g numpy {t_g:9.1f} for frame 0 ({n0} plates) CROPPED to {a.crop} x {a.crop} pixels at ({x0}, {y0}) = {100 * share:.2f} % of one frame "
                    f"({100 * float((ref['index'] >= 0).mean()):.1f} % of the window covered; index and image equal to the device's there: {same}); "
                    f"a whole frame was not timed")
        say(f"{source:5s}: {N:8d} plates, {total:8d} list entries = {total / max(N, 1):.2f} tiles a plate, {100 * covered:.2f} % of the pixels covered   "
            f"a frames {med['a']:7.3f} (min {min(ms['a']):.3f}, max {max(ms['a']):.3f})   b surface {med['b']:7.3f}   c plates {med['c']:7.3f} (min {min(ms['c']):.3f})   "
            f"d capacity {med['d']:7.3f} (min {min(ms['d']):.3f})   e bin {med['e']:7.3f} (min {min(ms['e']):.3f})   f draw {med['f']:7.3f} (min {min(ms['f']):.3f}, "
            f"max {max(ms['f']):.3f})   f / b {med['f'] / med['b']:.1f}   outputs {F * H * W * (4 + 8 + 3) / 1e6:.0f} MB   {host}")
        del x, pts, first
    if a.kernel_stats:
        say(f"kernel times of an earlier run under rocprofv3 --kernel-trace --stats ({os.path.basename(a.kernel_stats)}; all sources and calls of that run "
            f"together), average per launch, ms:")
        for name, calls, avg in kernel_table(a.kernel_stats):
            say(f"  {name:28s} {calls:6d} launches   {avg / 1e6:8.4f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
