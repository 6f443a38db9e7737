#!/usr/bin/env python3
"""Time the retargeting kernels (nm_retarget_bind, nm_retarget_pose) against the same computation written in torch device operations
(vectorised bind with the (N,K) distance matrix, dense einsum blend per frame - the form the reference uses, without its per-point
Python loop): N = 20 000 / 250 000 / 2 000 000 points, T = 40 frames, device events after warm-up, the two implementations alternating
in one process.  The times are those of the CALLS (event pairs around the shells: allocations and launch included - at N = 20 000 that is mostly host
overhead); for the pose kernel the bytes moved (24 T N written + the 64-byte bind record read once per chunk of 8 frames) over the call
time are printed, and the same bytes over the KERNEL time are to be taken from the rocprofv3 run below, next to the 6.3 TB/s a streaming
kernel achieves on this device.

  python tools/time_retarget.py [--out profiles/retarget_times.txt] [--n 20000 250000 2000000] [--frames 40]
  rocprofv3 --kernel-trace --stats -d rocprof_out -- python tools/time_retarget.py --n 2000000 --reps 3     # kernel times of their own
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import retarget_ref as RR  # noqa: E402
from neural_marionette_amd import HotPathOptions  # noqa: E402
from neural_marionette_amd.modules import HSVRNNBVH  # noqa: E402

STREAM_TBS = 6.3


def torch_bind(points, kp, R_bind, bones, masked, parents, hardness):
    """extract_skin_weights + local coordinates in device operations: dense (N,K) fp32, local (N,K,3) float64"""
    N, K = points.shape[0], kp.shape[0]
    dist = (points[:, None] - bones[None].double()).pow(2).sum(-1).sqrt()
    dist[:, masked] = 1e4
    child = dist.argmin(-1)
    parent = parents[child]
    pos = kp[:, :3].double()
    c = ((points - pos[child]).pow(2).sum(-1).sqrt() * hardness).exp()
    q = ((points - pos[parent]).pow(2).sum(-1).sqrt() * hardness).exp()
    dense = torch.zeros(N, K, device=points.device)
    n = torch.arange(N, device=points.device)
    dense[n, parent] = (c / (c + q)).float()
    dense[n, child] = (q / (c + q)).float()
    local = torch.einsum("kji,nkj->nki", R_bind.double(), points[:, None] - pos[None])
    return dense, local


def torch_pose(dense, local, R, pos):
    out = torch.empty(R.shape[0], dense.shape[0], 3, device=dense.device, dtype=torch.float64)
    w = dense.double()
    for t in range(R.shape[0]):
        kin = torch.einsum("kab,nkb->nka", R[t].double(), local) + pos[t].double()[None]
        out[t] = torch.einsum("nk,nka->na", w, kin)
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 250000, 2000000])
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, K = a.frames, 24
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    d = HSVRNNBVH(HotPathOptions(grid_size=32, nkeypoints=K)).cuda().eval()
    say(f"retargeting kernels, T = {T}, K = {K}, median of {a.reps} after 2 warm-up rounds, ms (device events)")
    for N in a.n:
        s = RR.standin(1, N=N, K=K, T=T)
        d.set_tree(s["parents"], s["order"])
        dev = torch.device("cuda")
        pts = torch.from_numpy(s["points"]).to(dev)
        kp, Rb, R = (torch.from_numpy(s[k]).to(dev) for k in ("keypoints", "R_bind", "R"))
        pos = torch.from_numpy(RR.fk(s["R"], s["root_pos"], s["offset"], s["order"], s["parents"], np.float32)).to(dev)
        bones, invalid = RR.bone_points(s["parents"], s["keypoints"])
        masked = invalid.copy()
        masked[s["root"]] = True
        bones_d, masked_d, par_d = torch.from_numpy(bones).to(dev), torch.from_numpy(masked).to(dev), torch.from_numpy(s["parents"].astype(np.int64)).to(dev)
        t = {k: [] for k in ("bind", "bind_torch", "pose", "pose_torch")}
        with torch.no_grad():
            for rep in range(a.reps + 2):
                ms_b, rec = timed(lambda: d.skin_weights(pts, kp, Rb))
                ms_bt, (dense, local) = timed(lambda: torch_bind(pts, kp, Rb, bones_d, masked_d, par_d, 8.0))
                ms_p, out = timed(lambda: d.retarget_pose(rec, R, pos))
                ms_pt, out_t = timed(lambda: torch_pose(dense, local, R, pos))
                if rep == 0:
                    err = float((out - out_t).abs().max())
                del out, out_t
                if rep >= 2:
                    for k, v in zip(("bind", "bind_torch", "pose", "pose_torch"), (ms_b, ms_bt, ms_p, ms_pt)):
                        t[k].append(v)
                del dense, local, rec
        m = {k: float(np.median(v)) for k, v in t.items()}
        chunks = (T + 7) // 8
        moved = 24.0 * T * N + 64.0 * N * chunks
        say(f"N = {N:8d}: bind {m['bind']:9.3f} (torch ops {m['bind_torch']:9.3f}, x{m['bind_torch'] / m['bind']:.1f})   "
            f"pose {m['pose']:9.3f} (torch ops {m['pose_torch']:9.3f}, x{m['pose_torch'] / m['pose']:.1f})   "
            f"pose traffic {moved / 1e9:.3f} GB = {moved / m['pose'] / 1e9:.3f} TB/s over the CALL (event pair around the shell: output allocation and "
            f"launch included; bytes over KERNEL time come from the rocprofv3 run; achievable {STREAM_TBS});  library vs torch ops, largest difference {err:.2e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
