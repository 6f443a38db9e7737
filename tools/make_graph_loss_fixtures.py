#!/usr/bin/env python3
"""Generate tests/golden/g15_graph_loss_options.npz: what the REFERENCE computes for the graph-loss options, recorded so that
tests/graph_loss_ref.py and the module shells are pinned to it without the reference tree.

  python tools/make_graph_loss_fixtures.py --reference DIR      # DIR: a checkout of the reference implementation (CPU only)

Recorded (numeric arrays only; names as UTF-8 bytes, SHA-256 digests as 32 bytes each):
1. get_graph_consistency_loss / get_graph_traj_loss (utils/kypt_detector_utils.py:172-265) in fp64 on seeded moving keypoints
   (B=2, T=6, K=24, intensities in (0, 1]) and the version-3 affinity of seeded parameters, for every graph_loss_ver in {0, 1, 2} and
   every (local, time, sparsity) switch combination: the four consistency outputs, the trajectory loss, and the gradients of
   S = sum_i W[i] * mean(output_i) with respect to the keypoints (all four components) and the affinity.
2. keypoints_graph 'none': the state_dict key list, shapes and per-tensor digests of KyptDetector(opt) after torch.manual_seed(3).
3. graph_random_init = 1: the per-tensor digests of KyptDetector(opt) after torch.manual_seed(4), for affinity_ver 3 and 0.
The detectors use the pretrained AIST options (tests/golden/aist_opt.json) at grid_size 32.
"""
from __future__ import annotations

import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g15_graph_loss_options.npz")
B, T, K, N = 2, 6, 24, 2
W = (1.0, 1.3, 0.7, 0.5, 0.9)        # weights of (local, time, sparsity, intensity, traj) in the scalar whose gradient is recorded
SWITCHES = list(itertools.product((1, 0), repeat=3))     # (local, time, sparsity)
VERSIONS = (0, 1, 2)


def inputs():
    """seeded moving keypoints (B,T,K,4) fp64 and version-3 affinity parameters (N,K,K-1) fp64"""
    g = torch.Generator().manual_seed(15)
    start = torch.rand(B, 1, K, 3, generator=g, dtype=torch.float64) * 1.6 - 0.8
    steps = torch.randn(B, T - 1, K, 3, generator=g, dtype=torch.float64) * 0.05
    pos = torch.cat([start, start + steps.cumsum(dim=1)], dim=1)
    inten = 1.0 - torch.rand(B, T, K, 1, generator=g, dtype=torch.float64)          # (0, 1]
    params = torch.randn(N, K, K - 1, generator=g, dtype=torch.float64)
    return torch.cat([pos, inten], dim=-1), params


def sha(t) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).digest(), dtype=np.uint8)


def names_bytes(names) -> np.ndarray:
    return np.frombuffer("\n".join(names).encode(), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation (holds model/, utils/)")
    REF = os.path.abspath(ap.parse_args().reference)
    sys.path.insert(0, REF)
    from model.kypt_detector import KyptDetector as RefDetector
    from utils.kypt_detector_utils import get_graph_consistency_loss, get_graph_traj_loss

    torch.set_num_threads(1)
    rec = {}
    kp0, params = inputs()
    # the reference's get_affinity, version 3 (kypt_detector.py:191-199), on the seeded parameters
    base = json.load(open(os.path.join(ROOT, "tests", "golden", "aist_opt.json")))

    def opt(**kw):
        o = argparse.Namespace(**base)
        o.grid_size = 32
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    det = RefDetector(opt()).double()
    with torch.no_grad():
        det.affinity_params.copy_(params)
    aff0 = det.get_affinity().detach()
    rec["keypoints"] = kp0.numpy()
    rec["affinity_params"] = params.numpy()
    rec["affinity"] = aff0.numpy()
    rec["weights"] = np.array(W)
    rec["switches"] = np.array(SWITCHES, dtype=np.int64)
    for ver in VERSIONS:
        for lo, ti, sp in SWITCHES:
            kp = kp0.clone().requires_grad_(True)
            aff = aff0.clone().requires_grad_(True)
            outs = list(get_graph_consistency_loss(kp, aff, local_const=bool(lo), time_const=bool(ti), sparsity_const=bool(sp),
                                                   intensity_const=True, ver=ver))
            outs.append(get_graph_traj_loss(kp, aff, ver=ver))
            s = sum(w * o.mean() for w, o in zip(W, outs))
            gk, ga = torch.autograd.grad(s, [kp, aff], allow_unused=True)
            tag = f"v{ver}_l{lo}t{ti}s{sp}"
            for name, o in zip(("local", "time", "sparsity", "intensity", "traj"), outs):
                rec[f"{tag}__{name}"] = o.detach().numpy()
            rec[f"{tag}__dkp"] = (gk if gk is not None else torch.zeros_like(kp)).numpy()
            rec[f"{tag}__daff"] = (ga if ga is not None else torch.zeros_like(aff)).numpy()
    # keypoints_graph 'none' (kypt_detector.py:54-68 skipped)
    torch.manual_seed(3)
    sd = RefDetector(opt(keypoints_graph="none")).state_dict()
    rec["none__names"] = names_bytes(list(sd))
    rec["none__shapes"] = np.array([list(v.shape) + [-1] * (5 - v.dim()) for v in sd.values()], dtype=np.int64)
    rec["none__sha256"] = np.stack([sha(v) for v in sd.values()])
    # graph_random_init = 1 (kypt_detector.py:56-61)
    for ver in (3, 0):
        torch.manual_seed(4)
        sd = RefDetector(opt(graph_random_init=1, affinity_ver=ver)).state_dict()
        rec[f"random_init_v{ver}__names"] = names_bytes(list(sd))
        rec[f"random_init_v{ver}__sha256"] = np.stack([sha(v) for v in sd.values()])
    for path in golden_npz.save(OUT, **rec):
        print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
