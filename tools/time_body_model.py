#!/usr/bin/env python3
"""Time the body-model step - the reference's AIST++ preparation (dataset/aistpp/prepare_aistpp.py:54-62, :75-89: smplx's SMPL forward,
the joint regressor, then the surface sampling) - on the synthetic model of SMPL's size, V = 6890 vertices, J = 24 joints, S = 10 shape
coefficients (BodyModel.synthetic with SMPL_PARENTS), for every frame count of --frames (64 and 1024):

  a  pose      NeuralMarionette.pose_bodies, float64 poses, betas, transl: device events around the whole call (allocation of the outputs,
               the rotation, chain, vertex and regression launches; v_shaped / J_rest come from the model's cache)
  b  core      nm_body_pose alone on the device's rotations into buffers allocated before: two launches, the chain kernel (a lane per
               frame) and the vertex kernel: device events - an UPPER bound of the vertex kernel's time
  c  bank      ClipBank.add_body: a, then 20 000 surface points per frame (sample_surface) and the float32 joints: device events
  d  numpy     the vectorised numpy form of the same contract (matrix products; NOT the loop-by-loop restatement of tests/body_ref.py)
               on this host: host clock, once, its vertices compared with the device's

a .. c alternate in one process; each figure is the median of --reps runs after --warmup runs.  The vertex kernel's compulsory bytes are
posedirs once per group of NM_BODY_FRAMES = 8 frames and the vertices once; the tool prints them over b's time as a LOWER bound of the
achieved share of the HBM peak (8.0 TB/s; posedirs, 34 MB, may well be served by the caches after its first read, which this count ignores).
The kernels separately are kernel times: run the tool under rocprofv3 in a run of its own and pass the statistics to the timed run:

  rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -- python tools/time_body_model.py --frames 1024 --reps 2 --warmup 1 --no-host --no-bank
  python tools/time_body_model.py --kernel-stats rocprof_out/<host>/<pid>_kernel_stats.csv --stats-frames 1024 [--out profiles/body_model_times.txt]

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

from neural_marionette_amd import NeuralMarionette, HotPathOptions, BodyModel, synth, _lib  # noqa: E402
from neural_marionette_amd.data import ClipBank  # noqa: E402

V, J, S, COUNT, NF = 6890, 24, 10, 20000, 8
HBM_PEAK = 8.0e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def kernel_table(path):
    """the body_* rows of rocprofv3's kernel statistics: name, calls, average ns"""
    rows = []
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            m = re.search(r"body_[a-z_]+_kernel(?:<[\w ,]+>|I\w+E)?", rec.get("Name") or "")
            if m:
                rows.append((m.group(0), int(rec.get("Calls") or 0), float(rec.get("AverageNs") or 0.0)))
    return sorted(rows)


def vertex_bytes(T):
    """compulsory bytes of the vertex kernel: posedirs once per group of NF frames, the vertices once"""
    groups = (T + NF - 1) // NF
    return groups * 9 * (J - 1) * 3 * V * 8 + T * V * 3 * 8


def numpy_forward(m, poses, betas, transl):
    """the contract in matrix products, float64"""
    T = poses.shape[0]
    e = poses + 1e-8
    angle = np.sqrt((e * e).sum(-1))
    u = poses / angle[..., None]
    K = np.zeros((T, J, 3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -u[..., 2], u[..., 1], u[..., 2], -u[..., 0], -u[..., 1], u[..., 0]
    R = np.eye(3) + np.sin(angle)[..., None, None] * K + (1.0 - np.cos(angle))[..., None, None] * (K @ K)
    v_shaped = m["v_template"] + m["shapedirs"] @ betas
    reg = np.zeros((J, V))
    for j in range(J):
        lo, hi = m["reg_offsets"][j], m["reg_offsets"][j + 1]
        reg[j, m["reg_cols"][lo:hi]] = m["reg_vals"][lo:hi]
    J_rest = reg @ v_shaped
    vp = v_shaped[None] + ((R[:, 1:] - np.eye(3)).reshape(T, -1) @ m["posedirs"]).reshape(T, V, 3)
    Gr, Gt = np.empty((T, J, 3, 3)), np.empty((T, J, 3))
    Gr[:, 0], Gt[:, 0] = R[:, 0], J_rest[0]
    for j in range(1, J):
        p = int(m["parents"][j])
        Gr[:, j] = Gr[:, p] @ R[:, j]
        Gt[:, j] = Gr[:, p] @ (J_rest[j] - J_rest[p]) + Gt[:, p]
    A = np.concatenate([Gr, (Gt - np.einsum("tjab,jb->tja", Gr, J_rest))[..., None]], axis=-1).reshape(T, J, 12)
    M = np.einsum("vj,tjk->tvk", m["lbs_weights"], A).reshape(T, V, 3, 4)
    x = np.einsum("tvab,tvb->tva", M[..., :3], vp) + M[..., 3]
    vertices = x + transl[:, None, :]
    return vertices, np.einsum("jv,tvc->tjc", reg, vertices)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,1024")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy form (profiler runs)")
    ap.add_argument("--no-bank", action="store_true", help="skip add_body (profiler runs)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 --kernel-trace --stats kernel statistics CSV of an earlier run")
    ap.add_argument("--stats-frames", type=int, default=1024, help="the frame count of that earlier run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_body_model.py measures on the GPU: no device found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"body model, synthetic, V = {V} vertices, J = {J} joints, S = {S} shape coefficients, {COUNT} samples a frame in add_body; median of {a.reps} after "
        f"{a.warmup} warm-up runs, ms;  {torch.cuda.get_device_name(0)};  host threads: OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}")
    o = HotPathOptions(grid_size=32)
    net = NeuralMarionette(o)
    net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
    net = net.cuda().eval()
    ctx = net._engine.ready()
    dev = ctx.device
    model = BodyModel.synthetic(V, J, S, seed=1, parents=BodyModel.SMPL_PARENTS, device=dev)
    m = model.numpy()
    rng = np.random.default_rng(2)
    betas_h = rng.standard_normal(S)
    betas = torch.from_numpy(betas_h).to(dev)
    parents = np.ascontiguousarray(model.parents, dtype=np.int32)
    for T in [int(x) for x in a.frames.split(",")]:
        poses_h, transl_h = 0.5 * rng.standard_normal((T, J, 3)), rng.standard_normal((T, 3))
        poses, transl = torch.from_numpy(poses_h).to(dev), torch.from_numpy(transl_h).to(dev)
        first = net.pose_bodies(model, poses=poses, betas=betas, transl=transl)
        rot = first["rotations"]
        tr, posed, vert = (torch.empty(T, J, 12, device=dev, dtype=torch.float64), torch.empty(T, J, 3, device=dev, dtype=torch.float64),
                           torch.empty(T, V, 3, device=dev, dtype=torch.float64))

        def core():
            net._engine.call("nm_body_pose", None, 0, rot.data_ptr(), T, V, J, parents.ctypes.data_as(_lib.c_int32_p), first["v_shaped"].data_ptr(),
                             first["J_rest"].data_ptr(), model.posedirs.data_ptr(), model.lbs_weights.data_ptr(), transl.data_ptr(), 1.0, None,
                             tr.data_ptr(), posed.data_ptr(), vert.data_ptr())

        ms = {k: [] for k in "abc"}
        for rep in range(a.reps + a.warmup):
            t_a, out = event_ms(lambda: net.pose_bodies(model, poses=poses, betas=betas, transl=transl))
            t_b, _ = event_ms(core)
            t_c = 0.0
            if not a.no_bank:
                bank = ClipBank(dev)
                t_c, _ = event_ms(lambda: bank.add_body(net, model, poses, betas=betas, transl=transl, count=COUNT, seed=1))
                del bank
            if rep == 0:
                assert torch.equal(out["vertices"], first["vertices"]) and torch.equal(vert, first["vertices"])
            del out
            if rep >= a.warmup:
                for k, x in zip("abc", (t_a, t_b, t_c)):
                    ms[k].append(x)
        med = {k: statistics.median(x) for k, x in ms.items()}
        nbytes = vertex_bytes(T)
        say(f"T = {T:5d}   a pose_bodies {med['a']:8.3f} (min {min(ms['a']):.3f}, max {max(ms['a']):.3f}) = {1e3 * med['a'] / T:.2f} us a frame   "
            f"b nm_body_pose on given rotations {med['b']:8.3f} (min {min(ms['b']):.3f}, max {max(ms['b']):.3f})   "
            + ("c add_body not measured" if a.no_bank else f"c add_body {med['c']:8.3f} (min {min(ms['c']):.3f}, max {max(ms['c']):.3f}) = {1e3 * med['c'] / T:.2f} us a frame"))
        say(f"            vertex kernel, compulsory bytes (posedirs once per {NF} frames, vertices once): {nbytes / 1e6:.1f} MB; over b that is at least "
            f"{nbytes / (1e-3 * med['b']) / 1e12:.3f} TB/s = {100 * nbytes / (1e-3 * med['b']) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak "
            f"(b also holds the chain kernel and two enqueues)")
        if not a.no_host:
            t0 = time.perf_counter()
            ref_v, ref_j = numpy_forward(m, poses_h, betas_h, transl_h)
            t_d = 1e3 * (time.perf_counter() - t0)
            dv = float(np.abs(ref_v - first["vertices"].cpu().numpy()).max())
            dj = float(np.abs(ref_j - first["joints"].cpu().numpy()).max())
            say(f"            d numpy, vectorised {t_d:9.1f}; largest |difference| to the device's vertices {dv:.2e}, joints {dj:.2e};  d / a {t_d / med['a']:.0f}")
        else:
            say("            d numpy not measured")
        del first, rot, tr, posed, vert
    say("occupancy: body_vertices_kernel is compiled to 128 VGPRs, no scratch, and takes 18 432 B of LDS a workgroup of two wavefronts at J = 24 (hipcc "
        "--save-temps), so registers admit 4 waves a SIMD and LDS 8 workgroups a CU; the occupancy ACHIEVED on the device and the cache hit rates of the "
        "posedirs reads (counter runs) were not looked at")
    if a.kernel_stats:
        say(f"kernel times of an earlier run under rocprofv3 --kernel-trace --stats ({os.path.basename(a.kernel_stats)}; T = {a.stats_frames}, all calls of that run "
            f"together), average per launch, ms:")
        for name, calls, avg in kernel_table(a.kernel_stats):
            extra = ""
            if name.startswith("body_vertices_kernel") and avg > 0:
                nbytes = vertex_bytes(a.stats_frames)
                extra = f"   {nbytes / 1e6:.1f} MB compulsory = {nbytes / (avg * 1e-9) / 1e12:.3f} TB/s = {100 * nbytes / (avg * 1e-9) / HBM_PEAK:.1f} % of the HBM peak"
            say(f"  {name:44s} {calls:6d} launches   {avg / 1e6:8.4f}{extra}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
