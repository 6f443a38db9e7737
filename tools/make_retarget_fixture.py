#!/usr/bin/env python3
"""Generate tests/golden/g16_retarget32[.partN].npz: what the REFERENCE computes for motion retargeting on the seeded inputs of
tests/retarget_ref.g16_inputs, recorded so that the library and the restatement are pinned to it without the reference tree.

  python tools/make_retarget_fixture.py --reference DIR      # DIR: a checkout of the reference implementation

The reference's own extract_skin_weights is imported from its vis_retarget.py (whose renderer imports are replaced by empty stand-in
modules; it reads pretrained/aist/opt.pickle relative to the working directory on import, so the tool runs inside DIR), and the
reference's NeuralMarionette sub-modules are driven in the order of that script's lines 236-322; the VRNN noise is injected by
replacing ``torch.distributions.normal._standard_normal``.  The script's re-posing loop and blend are inline code that cannot be
imported: the tool evaluates them on the reference's outputs (fp32 torch operations for the kinematic chain, the dense float64 blend of
tests/retarget_ref.pose_dense with the reference's own weight matrix).  Only arrays are written.

With synthetic weights many frame-0 intensities lie below the script's default threshold 0.2, the root's among them, and with an
invalid root the reference's function does not return; the fixture is therefore written with threshold 0.1 (a parameter of that
function) and the tool checks the root BEFORE it calls the function.
"""
from __future__ import annotations

import argparse
import collections
import os
import pickle
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_npz  # noqa: E402
import retarget_ref as RR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
THREADS = 4
THRESHOLD, HARDNESS = 0.1, 8.0
MARGIN_FREE, MARGIN_CAP = 4e-4, 0.02          # selections with a smaller margin are left out of the free-run comparison; at most 2 %
SENS_DRAWS, SENS_STEP = 8, 1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation (holds vis_retarget.py, model/, pretrained/)")
    REF = os.path.abspath(ap.parse_args().reference)
    for m in ("open3d", "cv2", "imageio"):
        sys.modules.setdefault(m, types.ModuleType(m))
    os.chdir(REF)
    sys.path.insert(0, REF)
    torch.set_num_threads(THREADS)
    import torch.distributions.normal as tdn
    import vis_retarget as VR
    from model.neural_marionette import NeuralMarionette

    seeds = RR.G16_SEEDS
    o, sd, source, target, points, eps_s, eps_t = RR.g16_inputs(seeds)
    opt = argparse.Namespace(**vars(pickle.load(open(os.path.join(REF, "pretrained/aist/opt.pickle"), "rb"))))
    opt.grid_size = seeds["G"]
    net = NeuralMarionette(opt).eval()
    net.load_state_dict(sd)
    net.anneal(1)
    dm = net.dyna_module
    T = seeds["T"]

    draws = iter(list(eps_s) + list(eps_t))
    old = tdn._standard_normal
    tdn._standard_normal = lambda shape, dtype, device: next(draws).clone()
    try:
        with torch.no_grad():
            src = net.kypt_detector(source[None])
            skp = src["keypoints"]
            skp[..., 3] = skp[:, :1, :, 3].clone()                  # every frame carries frame 0's intensities
            aff = src["affinity"]
            R = dm.encode(skp, aff)["R"][0]
            tkp = net.kypt_detector(target[None, None])["keypoints"]
            tkp = tkp.clone()
            tkp[..., 3] = skp[:, :1, :, 3]                          # the target's joints take the source's frame-0 intensities
            R_bind = dm.encode(tkp, aff)["R"][0, 0]
            offset = dm.get_offset(tkp)
            root = int(dm.priority.indices[0])
            ninv = int((tkp[0, 0, :, 3] < THRESHOLD).sum())
            K = tkp.shape[2]
            print(f"threshold {THRESHOLD}: {ninv} of {K} joints invalid; root = joint {root}, intensity {float(tkp[0, 0, root, 3]):.3f}")
            if float(tkp[0, 0, root, 3]) < THRESHOLD:
                raise SystemExit("the root is invalid: the reference's extract_skin_weights would not return; pick other seeds")
            if not 1 <= ninv <= K - 3:
                print("NOTE: these seeds give no usable count of invalid joints; the op-level cases cover the ancestor walk")
            dense = VR.extract_skin_weights(dm.A, dm.priority, dm.parents, points, tkp[0, 0], HARDNESS, THRESHOLD)
            # The re-posing loop and the blend are inline code of the script, not functions that could be imported: they are evaluated
            # here on the reference's outputs with the same torch operations in fp32 (all frames at once) and, for the blend, by the
            # restatement's dense form with the reference's own weight matrix.
            par, ordr = dm.parents.tolist(), dm.priority.indices.tolist()
            chain = torch.zeros(T, K, 3)
            chain[:, root] = skp[0, :, root, :3]
            for j in ordr[1:]:
                chain[:, j] = torch.bmm(R[:, j], offset[0, j][None].expand(T, -1, -1)).squeeze(-1) + chain[:, par[j]]
            new_kp = torch.cat([chain.clip(-1, 1)[None], skp[..., 3:]], dim=-1)
            out = RR.pose_dense(dense, points, tkp[0, 0].numpy(), R_bind.numpy(), R.numpy(), new_kp[0, :, :, :3].numpy())
    finally:
        tdn._standard_normal = old

    parents = dm.parents.numpy().astype(np.int32)
    order = dm.priority.indices.numpy().astype(np.int32)
    a = dict(source_keypoints=skp.numpy(), target_keypoints=tkp.numpy(), R=R.numpy(), R_bind=R_bind.numpy(), offset=offset.numpy(),
             keypoints=new_kp.numpy())
    # the margins of the reference's selections (its function does not return them): from the restatement, after checking that the
    # restatement reproduces the function's result bit for bit
    b, _, pts0 = RR.retarget(parents, order, a["source_keypoints"][0], a["target_keypoints"][0, 0], a["R"], a["R_bind"], a["offset"],
                             points, HARDNESS, THRESHOLD)
    assert np.array_equal(b["dense"].view(np.uint32), dense.view(np.uint32)), "the restatement differs from the reference's skin weights"
    nearest = b["nearest"].astype(np.int32)
    share = float((b["margin"] < MARGIN_FREE).mean())
    print(f"margins: smallest {b['margin'].min():.3e}, {100 * share:.2f} % below {MARGIN_FREE}; restatement vs reference points {np.abs(pts0 - out).max():.2e}")
    assert share <= MARGIN_CAP, f"{100 * share:.2f} % of the selections have a margin below {MARGIN_FREE}"
    # points_sens: how far the 1e-4 contract on keypoints, R, R_bind and offset moves the points, selections held fixed
    sens = 0.0
    for draw in range(SENS_DRAWS):
        rng = np.random.default_rng(1000 + draw)
        q = {k: (a[k] + rng.uniform(-SENS_STEP, SENS_STEP, a[k].shape)).astype(np.float32) for k in ("source_keypoints", "target_keypoints", "R", "R_bind", "offset")}
        _, _, p = RR.retarget(parents, order, q["source_keypoints"][0], q["target_keypoints"][0, 0], q["R"], q["R_bind"], q["offset"], points,
                              HARDNESS, THRESHOLD, force_child=nearest)
        sens = max(sens, float(np.abs(p - pts0).max()))
    print(f"points_sens {sens:.3e}")
    meta = np.array([seeds[k] for k in ("G", "T", "N", "weights", "source", "target", "pick", "eps_source", "eps_target")], dtype=np.int64)
    for path in golden_npz.save(os.path.join(OUT, "g16_retarget32.npz"), meta=meta, threshold=np.float64(THRESHOLD), hardness=np.float64(HARDNESS),
                                parents=parents, order=order, nearest=nearest, margin=b["margin"], dense=dense, points=out,
                                points_sens=np.float64(sens), invalid=np.int64(ninv), **a):
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
