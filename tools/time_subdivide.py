#!/usr/bin/env python3
"""Time Loop subdivision, smooth vertex normals and smooth shading on the device - vis_retarget.py's per-frame
``temp_mesh.subdivide_loop(arg.subdivide_iter)`` and ``compute_vertex_normals()`` (:416-423, :497-512) - at the script's size: a synthetic
mesh of the size of the reference's target.obj (12 465 vertices, 24 780 triangles: a closed 118 x 105 torus grid and 75 vertices no
triangle uses), T = 40 posed frames, 3 levels (793 035 vertices, 1 585 920 triangles a frame), its 1025 x 1023 window:

  a  plan       LoopPlan.build on the host (numpy) with the upload of its tables: host clock
  b  levels     nm_subdiv_apply through the C ABI, each level alone, all 40 frames: device events; achieved bytes per second against the
                compulsory traffic (every input and output row and every table entry once)
  c  subdivide  NeuralMarionette.subdivide, the three levels: device events
  d  normals    NeuralMarionette.vertex_normals of the fine mesh, 40 frames: device events, and its bytes per second
  e  shade      nm_mesh_shade alone through the C ABI on one group of frames: device events
  f  flat       NeuralMarionette.render_mesh alone on the fine mesh of all frames (what tools/time_mesh_path.py times on its torus)
  g  retarget   NeuralMarionette.render_retarget(subdivide=3, smooth=True, plan=plan) as a whole: subdivision, normals, draw, shade, two
                skeleton launches, overlay
  h  numpy      the same plan applied by vectorised numpy on this host (rings summed position by position, in order), and the two copies
                that path needs (coarse points to the host, fine points back): host clock, once

b .. g alternate in one process; each figure is the median of --reps runs after --warmup runs.  A device-event time of a call holds its
launches' gaps too; the kernels were not timed separately (that takes a profiler run of its own).  No target is fixed."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neural_marionette_amd import NeuralMarionette, HotPathOptions, PinholeCamera, LoopPlan, synth  # noqa: E402
from neural_marionette_amd.modules import MESH_RECORD_BYTES  # noqa: E402
import mesh_ref as MR  # noqa: E402
import render_ref as RR  # noqa: E402

NU, NV, LOOSE = 118, 105, 75                                                  # 2 NU NV = 24 780 triangles, NU NV + LOOSE = 12 465 vertices
T, W, H, K, LEVELS = 40, 1025, 1023, 24, 3
FOCAL = 880.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def scene(dev):
    verts, tri = MR.torus(NU, NV, 1.0, 0.42)
    verts = np.concatenate([verts, np.zeros((LOOSE, 3))])
    base = torch.from_numpy(verts).to(dev)
    frames = []
    for t in range(T):
        R = torch.from_numpy(RR.rigid((1.0 + 0.02 * t, 0.3 + 0.03 * t, 0.01 * t), (0, 0, 0))[:3, :3]).to(dev)
        frames.append(base @ R.T + torch.tensor([0.0, 0.0, 3.2], device=dev, dtype=torch.float64))
    ring = np.arange(K) * (2 * np.pi / K)
    joints = np.stack([np.cos(ring), np.sin(ring), 0.0 * ring], 1)
    kp = np.zeros((T, K, 4), np.float32)
    for t in range(T):
        R = RR.rigid((1.0 + 0.02 * t, 0.3 + 0.03 * t, 0.01 * t), (0, 0, 0))[:3, :3]
        kp[t, :, :3] = joints @ R.T + np.array([0.0, 0.0, 3.2])
        kp[t, :, 3] = 0.9
    return torch.stack(frames).contiguous(), tri, torch.from_numpy(kp).to(dev), np.maximum(np.arange(K) - 1, 0).astype(np.int32)


def numpy_level(x, tab):
    """one level by vectorised numpy: the rings position by position, so every sum keeps the contract's order"""
    edge, off, ring, w = tab["edge"], tab["ring_offsets"], tab["ring"], tab["w"]
    Tn, V = x.shape[:2]
    out = np.empty((Tn, V + len(edge), 3))
    n = np.diff(off)
    s = np.zeros((Tn, V, 3))
    for k in range(int(n.max()) if len(n) else 0):
        has = np.nonzero(n > k)[0]
        s[:, has] = s[:, has] + x[:, ring[off[has] + k]]
    out[:, :V] = w[:, 0][None, :, None] * x + w[:, 1][None, :, None] * s
    a, b, c, d = edge.T
    inner = d >= 0
    out[:, V:][:, ~inner] = 0.5 * (x[:, a[~inner]] + x[:, b[~inner]])
    out[:, V:][:, inner] = 0.375 * (x[:, a[inner]] + x[:, b[inner]]) + 0.125 * (x[:, c[inner]] + x[:, d[inner]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy application")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_subdivide.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cam = PinholeCamera(np.eye(4).tolist(), FOCAL, FOCAL, W / 2 - 0.5, H / 2 - 0.5, W, H)
    o = HotPathOptions(grid_size=32)
    net = NeuralMarionette(o)
    net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
    net = net.cuda().eval()
    eng = net._engine
    dev = eng.ready().device
    points, tri, kp, parents = scene(dev)
    V0 = int(points.shape[1])
    tri_dev = torch.from_numpy(tri).to(dev)
    t_plan = []
    for _ in range(3):
        t0 = time.perf_counter()
        plan = LoopPlan.build(tri, V0, LEVELS, device=dev)
        torch.cuda.synchronize()
        t_plan.append(1e3 * (time.perf_counter() - t0))
    counts, tcounts = plan.vertex_counts, plan.triangle_counts
    say(f"subdivision path, {T} frames of {V0} vertices / {len(tri)} triangles, {LEVELS} levels -> {counts[-1]} vertices / {tcounts[-1]} triangles a frame, "
        f"{W} x {H} pixels; median of {a.reps} after {a.warmup} warm-up runs, ms;  {torch.cuda.get_device_name(0)};  host threads: OMP_NUM_THREADS = "
        f"{os.environ.get('OMP_NUM_THREADS', 'unset')}")
    say(f"a plan   {statistics.median(t_plan):9.1f} on the host (min {min(t_plan):.1f} of 3), tables of {sum(t[k].numel() * t[k].element_size() for t in plan.levels_tables for k in t) / 1e6:.1f} MB "
        f"and {(plan.triangles.numel() + plan.face_offsets.numel() + plan.faces.numel()) * 4 / 1e6:.1f} MB for the finest level, uploaded; once per mesh")
    fine = net.subdivide(points, plan)
    normals = net.vertex_normals(fine, plan)
    first = net.render_mesh(fine, plan.triangles, cam, vertex_normals=normals, return_index=True)
    flat0 = net.render_mesh(fine, plan.triangles, cam)
    VL, ML = counts[-1], tcounts[-1]
    # the level inputs, for timing each level alone
    level_in = [points]
    for l in range(LEVELS - 1):
        p1 = LoopPlan(plan.V, l + 1, plan.levels_tables[:l + 1], None, None, None, counts[:l + 2], tcounts[:l + 2], plan.device)
        level_in.append(net.subdivide(points, p1))
    level_out = [torch.empty(T, counts[l + 1], 3, device=dev, dtype=torch.float64) for l in range(LEVELS)]
    bad = torch.empty(1, device=dev, dtype=torch.int32)

    def run_level(l):
        tab = plan.levels_tables[l]
        eng.call("nm_subdiv_apply", level_in[l].data_ptr(), T, counts[l], int(tab["edge"].shape[0]), tab["edge"].data_ptr(), tab["ring_offsets"].data_ptr(),
                 tab["ring"].data_ptr(), int(tab["ring"].numel()), tab["w"].data_ptr(), level_out[l].data_ptr(), bad.data_ptr())

    group = max(1, min(T, MESH_RECORD_BYTES // (144 * ML)))
    cs = cam.c_struct()
    TX, TY = (W + 15) // 16, (H + 15) // 16
    rec = torch.empty(group * ML, 16, device=dev, dtype=torch.float64)
    rect = torch.empty(group * ML, 4, device=dev, dtype=torch.int32)
    toff = torch.empty(group * TX * TY + 1, device=dev, dtype=torch.int64)
    eng.call("nm_mesh_bin", fine.data_ptr(), plan.triangles.data_ptr(), group, VL, ML, C.byref(cs), rec.data_ptr(), rect.data_ptr(), toff.data_ptr())
    index = first["index"][:group].contiguous()
    image = torch.empty(group, H, W, 3, device=dev, dtype=torch.uint8)

    def run_shade():
        eng.call("nm_mesh_shade", rec.data_ptr(), index.data_ptr(), plan.triangles.data_ptr(), normals.data_ptr(), None, None, group, VL, ML, C.byref(cs), 0.3, 0.7,
                 None, image.data_ptr())

    result = dict(points=points, keypoints=kp[None], source_keypoints=kp[None], skin_weights=torch.zeros(V0, K, device=dev))
    keys = [f"b{l}" for l in range(LEVELS)] + list("cdefg")
    ms = {k: [] for k in keys}
    for rep in range(a.reps + a.warmup):
        t = {}
        for l in range(LEVELS):
            t[f"b{l}"], _ = event_ms(lambda: run_level(l))
        t["c"], outc = event_ms(lambda: net.subdivide(points, plan))
        t["d"], outd = event_ms(lambda: net.vertex_normals(fine, plan))
        t["e"], _ = event_ms(run_shade)
        t["f"], outf = event_ms(lambda: net.render_mesh(fine, plan.triangles, cam))
        t["g"], outg = event_ms(lambda: net.render_retarget(result, tri_dev, cam, parents=parents, subdivide=LEVELS, smooth=True, plan=plan))
        if rep == 0:
            assert int(bad) == 0 and torch.equal(level_out[-1], fine) and torch.equal(outc, fine) and torch.equal(outd, normals)
            assert torch.equal(image, first["image"][:group]) and torch.equal(outf["image"], flat0["image"]) and torch.equal(outg["mesh"], first["image"])
        del outc, outd, outf, outg
        if rep >= a.warmup:
            for k in keys:
                ms[k].append(t[k])
    med = {k: statistics.median(v) for k, v in ms.items()}
    for l in range(LEVELS):
        tab = plan.levels_tables[l]
        traffic = 24 * T * (counts[l] + counts[l + 1]) + sum(tab[k].numel() * tab[k].element_size() for k in tab)
        say(f"b level {l + 1}: {counts[l]:7d} -> {counts[l + 1]:7d} vertices, {T} frames   {med[f'b{l}']:8.3f} (min {min(ms[f'b{l}']):.3f}, max {max(ms[f'b{l}']):.3f})   "
            f"compulsory traffic {traffic / 1e6:7.1f} MB -> {traffic / med[f'b{l}'] / 1e6:7.1f} GB/s")
    traffic = 48 * T * VL + (plan.triangles.numel() + plan.face_offsets.numel() + plan.faces.numel()) * 4
    say(f"c subdivide {med['c']:8.3f} (min {min(ms['c']):.3f}) = {med['c'] / T:.3f} a frame, {med['c'] / sum(med[f'b{l}'] for l in range(LEVELS)):.2f} of the three levels alone   "
        f"d normals {med['d']:8.3f} (min {min(ms['d']):.3f}, max {max(ms['d']):.3f}) = {med['d'] / T:.3f} a frame, compulsory traffic {traffic / 1e6:.1f} MB -> "
        f"{traffic / med['d'] / 1e6:.1f} GB/s (its gathers read each vertex row 18 times: six triangles, each recomputed by its three corners)")
    covered = float((first["index"] >= 0).float().mean())
    say(f"e shade {med['e']:8.3f} (min {min(ms['e']):.3f}, max {max(ms['e']):.3f}) for {group} frames, {100 * covered:.2f} % of the pixels covered   "
        f"f flat render_mesh of the fine mesh {med['f']:8.3f} (min {min(ms['f']):.3f}) = {med['f'] / T:.3f} a frame   "
        f"g retarget, subdivided and smooth {med['g']:8.3f} (min {min(ms['g']):.3f}, max {max(ms['g']):.3f}) = {med['g'] / T:.3f} a frame = {med['g'] / med['f']:.2f} of f: "
        f"subdivision, normals and shading add {med['g'] - med['f']:.1f} to the draw")
    if not a.no_host:
        host_tabs = [{k: v.cpu().numpy() for k, v in tab.items()} for tab in plan.levels_tables]
        t0 = time.perf_counter()
        x = points.cpu().numpy()
        t_down = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        for tab in host_tabs:
            x = numpy_level(x, tab)
        t_host = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        back = torch.from_numpy(x).to(dev)
        torch.cuda.synchronize()
        t_up = 1e3 * (time.perf_counter() - t0)
        say(f"h numpy {t_host:9.1f} for the three levels of all {T} frames on this host (vectorised, once), copies {t_down:.1f} down ({points.numel() * 8 / 1e6:.0f} MB) + "
            f"{t_up:.1f} up ({back.numel() * 8 / 1e6:.0f} MB); equal to the device's bits: {bool(torch.equal(back.view(torch.int64), fine.view(torch.int64)))}; "
            f"{(t_host + t_down + t_up) / med['c']:.0f} times c")
    else:
        say("h numpy not measured")
    say("not looked at: achieved occupancy, cache hit rates and the kernels' own times apart from their launches (no counter or trace run was made); "
        "whether NM_SUBDIV_FRAMES = 4 frames a lane is the best number; storing face vectors first instead of recomputing the cross products per corner")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
