#!/usr/bin/env python3
"""Time the surface path - normals, plate frames and shading of the decoder's occupied voxels (vis_generation.py:157-171,
vis_interpolation.py:160-177) - at B = 4 clips x T = 16 frames of 64^3, on synth clips pushed through the detector's decoder
('recon') or on their input occupancy ('input'):

  a  surface   NeuralMarionette.surface_points, exact-sized (one read of offsets[-1]: the call's one synchronisation), radius2 = 6,
               outward, with colours (a device tensor): device events around the call
  b  capacity  the same with capacity = the number of points rounded up to 4096 (no synchronisation): device events
  c  points    NeuralMarionette.occupied_points(return_depth=True) alone - what a and b contain before nm_occupied_surface: device events
  d  numpy     the float64 restatement tests/surface_ref.py on this host, on the voxels already copied and thresholded into points:
               moments offset by offset, numpy.linalg.eigh, the orientation rule, drawPlate as array expressions, the colour line:
               host clock, every frame once
  e  scipy     the neighbourhoods from scipy.spatial.cKDTree.query_ball_point instead (the formulation of tests/test_surface_path_cpu.py;
               a Python loop over the points): host clock, --tree-frames frames, per frame
  f  open3d    estimate_normals() + orient_normals_consistent_tangent_plane(5) per frame, where open3d is installed (NOT the same
               normals: its 30 nearest neighbours on a lattice are a matter of tie-breaking): host clock, per frame

a, b and c alternate in one process; each figure is the median of --reps runs after --warmup runs.  No target is fixed.

  python tools/time_surface_path.py [--out profiles/surface_path_times.txt] [--reps 20] [--sources recon input]
  rocprofv3 --kernel-trace --stats -d rocprof_out -- python tools/time_surface_path.py --reps 3 --no-host --sources input     # kernel times
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

from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth  # noqa: E402
import surface_ref as SR  # noqa: E402

B, T, G = 4, 16, 64
BASE, SHADE = (0.6, 1.0, 0.6), (0.8, 0.2)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def open3d_frame(coords):
    import open3d as o3d
    pcd = o3d.geometry.PointCloud()
    pcd.points = o3d.utility.Vector3dVector(coords)
    pcd.estimate_normals()
    pcd.orient_normals_consistent_tangent_plane(5)
    return np.asarray(pcd.normals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tree-frames", type=int, default=2)
    ap.add_argument("--sources", nargs="+", default=["recon", "input"], choices=["recon", "input"])
    ap.add_argument("--no-host", action="store_true", help="skip the host restatements (profiler runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_surface_path.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"surface path, {B} x {T} frames at {G}^3, radius2 = 6; median of {a.reps} after {a.warmup} warm-up runs, ms;  {torch.cuda.get_device_name(0)};  "
        f"host threads: OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}, torch.get_num_threads() = {torch.get_num_threads()}")
    o = HotPathOptions(grid_size=G)
    net = NeuralMarionette(o)
    net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
    net = net.cuda().eval()
    net.anneal(1)
    occ = synth.figure_clip(B, T, G, seed=3).cuda()
    base = np.tile(BASE, (B * T, 1))
    base_dev = torch.from_numpy(base).cuda()                    # on the device already: the call copies nothing from the host
    for source in a.sources:
        if source == "recon":
            with torch.no_grad():
                x = torch.cat([net.kypt_detector(occ[b:b + 1])["recon"] for b in range(B)]).contiguous()
        else:
            x = occ
        total = int((~(x < 0.5)).sum())
        cap = (total + 4095) // 4096 * 4096
        kw = dict(base_colors=base_dev, shade=SHADE)
        ms = {k: [] for k in "abc"}
        for rep in range(a.reps + a.warmup):
            t_a, out = event_ms(lambda: net.surface_points(x, 0.5, **kw))
            t_b, outb = event_ms(lambda: net.surface_points(x, 0.5, capacity=cap, **kw))
            t_c, pts = event_ms(lambda: net.occupied_points(x, 0.5, return_depth=True))
            if rep == 0:
                assert len(out["normals"]) == total == len(pts["coords"])
                assert torch.equal(out["normals"], outb["normals"][:total]) and torch.equal(out["plates"], outb["plates"][:total])
                first = out
            del out, outb, pts
            if rep >= a.warmup:
                for k, v in zip("abc", (t_a, t_b, t_c)):
                    ms[k].append(v)
        med = {k: statistics.median(v) for k, v in ms.items()}
        host = "d numpy not measured   e scipy not measured   f open3d not measured"
        if not a.no_host:
            v = x.cpu().numpy()
            t0 = time.perf_counter()
            ref = SR.surface_points(v, 0.5, 6, base=base, shade_ab=SHADE)
            t_d = 1e3 * (time.perf_counter() - t0)
            assert np.array_equal(ref["colors"], first["colors"].cpu().numpy(), equal_nan=True)
            cross = np.linalg.norm(np.cross(ref["normals"], first["normals"].cpu().numpy()), axis=1)
            gap, _ = SR.exempt_rows(ref)
            keep = (ref["moments"][:, 0] >= 3) & ~gap
            tree = []
            for f in range(min(a.tree_frames, B * T)):
                idx = ref["indices"][ref["offsets"][f]:ref["offsets"][f + 1]]
                t0 = time.perf_counter()
                m = SR.moments_kdtree(idx, 6)
                lam, vec = np.linalg.eigh(SR.covariance(m))
                SR.plate_rows(ref["coords"][ref["offsets"][f]:ref["offsets"][f + 1]], vec[:, :, 0])
                tree.append(1e3 * (time.perf_counter() - t0))
                assert np.array_equal(m, ref["moments"][ref["offsets"][f]:ref["offsets"][f + 1]])
            try:
                import open3d  # noqa: F401
                o3 = []
                for f in range(min(a.tree_frames, B * T)):
                    t0 = time.perf_counter()
                    open3d_frame(ref["coords"][ref["offsets"][f]:ref["offsets"][f + 1]])
                    o3.append(1e3 * (time.perf_counter() - t0))
                f_txt = f"f open3d {statistics.median(o3):8.1f} per frame"
            except ImportError:
                f_txt = "f open3d not installed"
            host = (f"d numpy {t_d:9.1f} for {B * T} frames = {t_d / (B * T):7.1f} per frame (x{t_d / med['a']:.0f} of a; max |n x n_ref| above the gap "
                    f"{cross[keep].max(initial=0):.1e}, {100 * gap.mean():.2f} % of the rows below it)   e scipy {statistics.median(tree):8.1f} per frame   {f_txt}")
        say(f"{source:5s}: {total:8d} points = {100.0 * total / x.numel():.2f} % of the voxels   a surface {med['a']:7.3f} (min {min(ms['a']):.3f}, max {max(ms['a']):.3f})   "
            f"b capacity {med['b']:7.3f} (min {min(ms['b']):.3f})   c points alone {med['c']:7.3f} (min {min(ms['c']):.3f})   a - c {med['a'] - med['c']:7.3f}   {host}")
        del x
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
