#!/usr/bin/env python3
"""Time the mesh and skeleton render path - vis_retarget.py's images (:400-557: the posed TriangleMesh, drawSphere / drawCone per joint and
bone, the skeleton pasted over the mesh, all through open3d's off-screen visualiser) - at the script's size: T = 40 posed frames into
its 1025 x 1023 window, a closed procedural mesh (a torus grid) with the triangle count of the reference's target.obj after the script's
three Loop subdivisions, and a K = 24 skeleton:

  a  mesh      NeuralMarionette.render_mesh, exact-sized (one read per group of frames): device events
  b  capacity  the same with bin_capacity = the largest group's list entries rounded up to 4096 (no synchronisation): device events
  c  bin       nm_mesh_bin alone through the C ABI on the first group of frames (transform, count, scan): device events
  d  draw      nm_mesh_draw alone through the C ABI on that group (fill, draw), all three outputs: device events
  e  skeleton  NeuralMarionette.render_skeleton, all T frames in its one launch: device events
  f  retarget  NeuralMarionette.render_retarget (mesh, two skeleton launches, overlay): device events
  g  numpy     the float64 restatement tests/mesh_ref.py on this host, on frame 0 CROPPED to a window of --crop x --crop pixels about the
               middle of what the frame covers (a whole frame was not timed), all triangles (every --host-stride-th with a stride):
               host clock, once, compared with the device's index map and image on the window

a .. f alternate in one process; each figure is the median of --reps runs after --warmup runs.  transform / tiles / scan / draw
separately are kernel times: run the tool under rocprofv3 in a run of its own and pass the statistics to the timed run, which appends them:

  rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -- python tools/time_mesh_path.py --reps 2 --warmup 1 --no-host
  python tools/time_mesh_path.py --kernel-stats rocprof_out/<host>/<pid>_kernel_stats.csv [--out profiles/mesh_path_times.txt]

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
from neural_marionette_amd.modules import MESH_RECORD_BYTES  # noqa: E402
import mesh_ref as MR  # noqa: E402
import render_ref as RR  # noqa: E402

# data/demo/target/ninja/target.obj of the reference has 24 780 faces, all triangles ('f' lines counted on the CPU); a Loop subdivision
# splits every triangle in four, and vis_retarget.py subdivides three times (arg.subdivide_iter)
TARGET_OBJ_FACES = 24780
TRIANGLES = TARGET_OBJ_FACES * 4 ** 3                                          # 1 585 920
NU, NV = 1120, 708                                                            # the torus grid: 2 NU NV = TRIANGLES
assert 2 * NU * NV == TRIANGLES
T, W, H, K = 40, 1025, 1023, 24
FOCAL = 880.0


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def kernel_table(path):
    """the mesh_*, skeleton_* and render_scan_* rows of rocprofv3's kernel statistics: name, calls, average ns"""
    rows = []
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            m = re.search(r"(?:mesh|skeleton|render_scan)_[a-z_]+(?:<\w+>|ILb[01]E)?", rec.get("Name") or "")
            if m:
                rows.append((m.group(0).replace("ILb0E", "<false>").replace("ILb1E", "<true>"), int(rec.get("Calls") or 0), float(rec.get("AverageNs") or 0.0)))
    return sorted(rows)


def scene(dev):
    """the torus posed in T frames (a slow tumble in front of the camera), its triangles, and a skeleton of K joints along its ring"""
    verts, tri = MR.torus(NU, NV, 1.0, 0.42)
    base = torch.from_numpy(verts).to(dev)
    frames = []
    for t in range(T):
        R = torch.from_numpy(RR.rigid((1.0 + 0.02 * t, 0.3 + 0.03 * t, 0.01 * t), (0, 0, 0))[:3, :3]).to(dev)
        frames.append(base @ R.T + torch.tensor([0.0, 0.0, 3.2], device=dev, dtype=torch.float64))
    vertices = torch.stack(frames).contiguous()
    ring = np.arange(K) * (2 * np.pi / K)
    joints = np.stack([np.cos(ring), np.sin(ring), 0.0 * ring], 1)
    kp = np.zeros((T, K, 4), np.float32)
    for t in range(T):
        R = RR.rigid((1.0 + 0.02 * t, 0.3 + 0.03 * t, 0.01 * t), (0, 0, 0))[:3, :3]
        kp[t, :, :3] = joints @ R.T + np.array([0.0, 0.0, 3.2])
        kp[t, :, 3] = 0.9
    parents = np.maximum(np.arange(K) - 1, 0).astype(np.int32)
    return vertices, torch.from_numpy(tri).to(dev), torch.from_numpy(kp).to(dev), parents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crop", type=int, default=96)
    ap.add_argument("--host-stride", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (profiler runs)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats kernel statistics CSV of an earlier run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_path.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cam = PinholeCamera(np.eye(4).tolist(), FOCAL, FOCAL, W / 2 - 0.5, H / 2 - 0.5, W, H)
    say(f"mesh path, {T} frames of {TRIANGLES} triangles ({TARGET_OBJ_FACES} faces x 4^3) and a {K}-joint skeleton into {W} x {H} pixels; median of {a.reps} after "
        f"{a.warmup} warm-up runs, ms;  {torch.cuda.get_device_name(0)};  host threads: OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}")
    o = HotPathOptions(grid_size=32)
    net = NeuralMarionette(o)
    net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
    net = net.cuda().eval()
    eng = net._engine
    dev = eng.ready().device
    vertices, tri, kp, parents = scene(dev)
    V, M = int(vertices.shape[1]), int(tri.shape[0])
    group = max(1, min(T, MESH_RECORD_BYTES // (144 * M)))
    first = net.render_mesh(vertices, tri, cam, return_index=True, return_depth=True)
    total = int(first["bin_total"])
    TX, TY = (W + 15) // 16, (H + 15) // 16
    nt = group * TX * TY
    cs = cam.c_struct()
    rec = torch.empty(group * M, 16, device=dev, dtype=torch.float64)
    rect = torch.empty(group * M, 4, device=dev, dtype=torch.int32)
    toff = torch.empty(nt + 1, device=dev, dtype=torch.int64)
    eng.call("nm_mesh_bin", vertices.data_ptr(), tri.data_ptr(), group, V, M, C.byref(cs), rec.data_ptr(), rect.data_ptr(), toff.data_ptr())
    entries = int(toff[-1])
    groups = (T + group - 1) // group
    cap = (max(entries, total // groups) * 3 // 2 + 4095) // 4096 * 4096         # half again over a group's share: the tumble is slow, the groups alike
    lst = torch.empty(cap, device=dev, dtype=torch.int32)
    index = torch.empty(group, H, W, device=dev, dtype=torch.int32)
    depth = torch.empty(group, H, W, device=dev, dtype=torch.float64)
    image = torch.empty(group, H, W, 3, device=dev, dtype=torch.uint8)
    result = dict(points=vertices, keypoints=kp[None], source_keypoints=kp[None], skin_weights=torch.zeros(V, K, device=dev))

    def run_bin():
        eng.call("nm_mesh_bin", vertices.data_ptr(), tri.data_ptr(), group, V, M, C.byref(cs), rec.data_ptr(), rect.data_ptr(), toff.data_ptr())

    def run_draw():
        eng.call("nm_mesh_draw", rec.data_ptr(), rect.data_ptr(), toff.data_ptr(), tri.data_ptr(), None, None, group, V, M, C.byref(cs), 0.3, 0.7, None, cap,
                 lst.data_ptr(), index.data_ptr(), depth.data_ptr(), image.data_ptr())

    ms = {k: [] for k in "abcdef"}
    for rep in range(a.reps + a.warmup):
        t_a, out = event_ms(lambda: net.render_mesh(vertices, tri, cam))
        t_b, outb = event_ms(lambda: net.render_mesh(vertices, tri, cam, bin_capacity=cap))
        t_c, _ = event_ms(run_bin)
        t_d, _ = event_ms(run_draw)
        t_e, oute = event_ms(lambda: net.render_skeleton(kp, parents, cam))
        t_f, outf = event_ms(lambda: net.render_retarget(result, tri, cam, parents=parents))
        if rep == 0:
            assert torch.equal(out["image"], first["image"]) and torch.equal(outb["image"], first["image"]) and int(outb["bin_total"]) == total
            assert torch.equal(image, first["image"][:group]) and torch.equal(index, first["index"][:group]) and int(toff[-1]) == entries
            assert torch.equal(outf["mesh"], first["image"]) and torch.equal(outf["skeleton"], oute["image"])
            skel_cover = float((oute["image"] != 255).any(-1).float().mean())
        del out, outb, oute, outf
        if rep >= a.warmup:
            for k, v in zip("abcdef", (t_a, t_b, t_c, t_d, t_e, t_f)):
                ms[k].append(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    covered = float((first["index"] >= 0).float().mean())
    mtri = group * M / 1e6
    say(f"mesh: {M} triangles a frame, {group} frames a group ({MESH_RECORD_BYTES >> 20} MiB of records), {total} list entries = {total / (T * M):.2f} tiles a triangle, "
        f"{100 * covered:.2f} % of the pixels covered   a mesh {med['a']:8.3f} (min {min(ms['a']):.3f}, max {max(ms['a']):.3f}) = {med['a'] / T:.3f} a frame   "
        f"b capacity {med['b']:8.3f} (min {min(ms['b']):.3f})   c bin {med['c']:7.3f} (min {min(ms['c']):.3f}) for {group} frames   "
        f"d draw {med['d']:7.3f} (min {min(ms['d']):.3f}, max {max(ms['d']):.3f}) for {group} frames = {med['d'] / mtri:.3f} per million triangles "
        f"(the plate draw's committed figures: 0.83 - 2.74 for 0.3 - 1.3 million plates in 64 frames of 1025 x 958)   "
        f"d / c {med['d'] / med['c']:.2f} (the draw CALL fills the lists before it draws: the kernel times below split it)   "
        f"outputs of a group {group * H * W * (4 + 8 + 3) / 1e6:.0f} MB")
    say(f"skeleton: {K} joints, {100 * skel_cover:.2f} % of the pixels covered   e skeleton {med['e']:8.3f} (min {min(ms['e']):.3f}, max {max(ms['e']):.3f}) = "
        f"{med['e'] / T:.3f} a frame   f retarget {med['f']:8.3f} (min {min(ms['f']):.3f}) = {med['f'] / T:.3f} a frame, {med['f'] / (med['a'] + 2 * med['e']):.2f} of a + 2 e")
    say("occupancy: mesh_draw_kernel is compiled to 56 VGPRs and 11 264 B of LDS a workgroup (hipcc -Rpass-analysis=kernel-resource-usage: 8 waves a SIMD), "
        "so registers and LDS admit the eight workgroups a CU's 32 wavefront slots hold, which is what NM_MESH_CHUNK = 128 was chosen for; the occupancy "
        "ACHIEVED on the device (a counter run) was not measured")
    if not a.no_host:
        idx0 = first["index"][0].cpu().numpy()
        ys, xs = np.nonzero(idx0 >= 0)
        my, mx = ((int(ys.min()) + int(ys.max())) // 2, (int(xs.min()) + int(xs.max())) // 2) if len(ys) else (H // 2, W // 2)
        y0, x0 = max(0, min(H - a.crop, my - a.crop // 2)), max(0, min(W - a.crop, mx - a.crop // 2))
        crop = (x0, x0 + a.crop, y0, y0 + a.crop)
        sub = tri[::a.host_stride].contiguous()
        dev_sub = net.render_mesh(vertices[:1], sub, cam, return_index=True)
        v0, s0 = vertices[0].cpu().numpy(), sub.cpu().numpy()
        t0 = time.perf_counter()
        ref = MR.render_mesh(v0[None], s0, cam, crop=crop)
        t_g = 1e3 * (time.perf_counter() - t0)
        win = (slice(y0, y0 + a.crop), slice(x0, x0 + a.crop))
        same = np.array_equal(ref["index"][0], dev_sub["index"][0].cpu().numpy()[win]) and np.array_equal(ref["image"][0], dev_sub["image"][0].cpu().numpy()[win])
        say(f"g numpy {t_g:9.1f} for frame 0, {len(s0)} of {M} triangles (stride {a.host_stride}), CROPPED to {a.crop} x {a.crop} pixels at ({x0}, {y0}) = "
            f"{100 * a.crop * a.crop / (H * W):.2f} % of one frame ({100 * float((ref['index'] >= 0).mean()):.1f} % of the window covered; index and image equal to the "
            f"device's for those triangles there: {same}); a whole frame was not timed")
    else:
        say("g numpy not measured")
    if a.kernel_stats:
        say(f"kernel times of an earlier run under rocprofv3 --kernel-trace --stats ({os.path.basename(a.kernel_stats)}; all calls of that run together), "
            f"average per launch, ms:")
        table = kernel_table(a.kernel_stats)
        for name, calls, avg in table:
            say(f"  {name:28s} {calls:6d} launches   {avg / 1e6:8.4f}")
        binning = sum(avg for name, _, avg in table if name.startswith(("mesh_transform", "mesh_tiles", "render_scan"))) / 1e6
        drawing = sum(avg for name, _, avg in table if name.startswith("mesh_draw")) / 1e6
        if binning and drawing:
            say(f"  per group of frames: binning (transform, count, scan, fill) {binning:.3f} against the draw kernel's {drawing:.3f}: "
                f"{'binning' if binning > drawing else 'drawing'} dominates")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
