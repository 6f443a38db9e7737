#!/usr/bin/env python3
"""Generate tests/golden/g17_recurrent32.npz: what the REFERENCE computes with options.const_intensity = 2 (heat-maps propagated from frame
to frame, model/kypt_detector.py:308-347) on seeded inputs, so that tests/recurrent_heatmap_ref.py is pinned to it without the reference tree.

  python tools/make_recurrent_fixture.py --reference DIR      # DIR: a checkout of the reference implementation

The reference runs on the CPU with one intra-op thread, the AIST options (tests/golden/aist_opt.json) at grid_size 32 and
synth.make_state_dict(..., variant="peaky") weights.  Recorded:
  fwd__*    B = 2, T = 16 on a synth.figure_clip: keypoints (whole), heat-maps (every 4th voxel per axis + per-map sums), the 13 losses,
            first_feature sums, and - with the recorded eps - kypt_recon, z_kypts, h_kypts, R, best_idx, the tree; also the keypoints the
            reference gives for const_intensity = 3 on the same weights and clip (how far the two options are apart)
  init__*   the seeded construction: digests of the state_dict for const_intensity 2 and 3
  grad{s}__* B = 1, T = 4, seeds 431 and 432, float64: the AIST-weighted training loss and its gradient w.r.t. propagate_heatmaps,
            both head convs and one early conv of each feature net
While it runs, the tool asserts that the restatement agrees with the reference bit for bit in float32 on this machine (best_idx, which the
reference does not return, is the restatement's: the sample whose z / h the reference returned, bit for bit).
The fixture holds numbers and seeds only."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from neural_marionette_amd import synth  # noqa: E402
from neural_marionette_amd.spec import HotPathOptions, DETECTOR_LOSS_KEYS  # noqa: E402
from neural_marionette_amd.train import DETECTOR_LOSS_WEIGHTS as AIST  # noqa: E402
import golden_npz  # noqa: E402
import recurrent_heatmap_ref as RR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LOSS_KEYS = DETECTOR_LOSS_KEYS + ("kl_kypt", "kypt_recon_loss")
G, B, T, SEED = 32, 2, 16, 430
GRAD_SEEDS = (431, 432)
V2K = "kypt_detector.vox_to_kypt"
GRAD_KEYS = (V2K + ".propagate_heatmaps.0.weight", V2K + ".propagate_heatmaps.0.bias",
             V2K + ".extract_heatmaps_from_features.0.weight", V2K + ".extract_heatmaps_from_features.0.bias",
             V2K + ".extract_spatio_temporal_heatmaps_from_features.0.weight", V2K + ".extract_spatio_temporal_heatmaps_from_features.0.bias",
             V2K + ".extract_features.1.stride_conv.0.weight", V2K + ".extract_spatio_temporal_features.1.stride_conv.0.weight")


def digest(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation (holds model/, utils/)")
    REF = os.path.abspath(ap.parse_args().reference)
    sys.path.insert(0, REF)
    torch.set_num_threads(1)
    import torch.distributions.normal as tdn
    from model.neural_marionette import NeuralMarionette

    with open(os.path.join(OUT, "aist_opt.json")) as f:
        base = json.load(f)

    def _opt(ci):
        opt = argparse.Namespace(**base)
        opt.grid_size = G
        opt.const_intensity = ci
        return opt

    d = {}
    # seeded construction: the two options build the same modules and draw the same numbers
    for ci in (2, 3):
        torch.manual_seed(9)
        sd0 = NeuralMarionette(_opt(ci)).state_dict()
        d[f"init__names{ci}"] = np.array(list(sd0))
        d[f"init__sha256_{ci}"] = np.array([digest(v) for v in sd0.values()])

    o2 = HotPathOptions.from_any(_opt(2))
    sd = synth.make_state_dict(o2, seed=SEED, variant="peaky")
    vox = synth.figure_clip(B, T, G, seed=SEED + 2)
    eps = synth.make_eps((T, 10, B, o2.nlatent_kypt), seed=SEED + 3)

    def reference_forward(ci):
        net = NeuralMarionette(_opt(ci)).eval()
        net.load_state_dict(sd)
        net.anneal(1)
        it = iter(eps)
        old = tdn._standard_normal
        tdn._standard_normal = lambda shape, dtype, device: next(it).clone()
        try:
            with torch.no_grad():
                out = net(vox, {"detector": True, "learner": True})
        finally:
            tdn._standard_normal = old
        return out, net

    ref, net = reference_forward(2)
    ref3, _ = reference_forward(3)
    with torch.no_grad():
        mine = RR.nm_forward(sd, o2, vox, eps)
    for k in ("keypoints", "heatmaps", "first_feature", "recon", "kypt_recon", "z_kypts", "h_kypts", "R"):
        assert torch.equal(mine[k], ref[k]), "restatement != reference: " + k
    assert np.array_equal(mine["parents"], net.dyna_module.parents.numpy())
    hm = ref["heatmaps"]
    d.update(fwd__keypoints=ref["keypoints"].numpy(), fwd__keypoints_ci3=ref3["keypoints"].numpy(),
             fwd__heatmaps_strided=hm[..., 1::4, 1::4, 1::4].contiguous().numpy(),
             fwd__heatmaps_sums=hm.double().sum(dim=(3, 4, 5)).numpy(),
             fwd__first_feature_sum=np.float64(ref["first_feature"].double().sum()),
             fwd__first_feature_abssum=np.float64(ref["first_feature"].double().abs().sum()),
             fwd__losses=np.array([float(ref[k]) for k in LOSS_KEYS], dtype=np.float64),
             fwd__affinity=ref["affinity"].numpy(), fwd__kypt_recon=ref["kypt_recon"].numpy(), fwd__z_kypts=ref["z_kypts"].numpy(),
             fwd__h_kypts=ref["h_kypts"].numpy(), fwd__R=ref["R"].numpy(), fwd__best_idx=mine["best_idx"].numpy().astype(np.int32),
             fwd__parents=net.dyna_module.parents.numpy(), fwd__order=net.dyna_module.priority.indices.numpy(),
             fwd__seed=np.int64(SEED), fwd__shape=np.array([B, T, G], dtype=np.int64))
    # gradients of the detector-mode training loss, float64
    for s in GRAD_SEEDS:
        sds = synth.make_state_dict(o2, seed=s, variant="peaky")
        voxs = synth.figure_clip(1, 4, G, seed=s + 2)
        net = NeuralMarionette(_opt(2)).double().train()
        net.load_state_dict({k: v.double() for k, v in sds.items()})
        net.anneal(1)
        out = net.kypt_detector(voxs.double())
        loss = sum(w * out[k] for k, w in AIST.items())
        params = dict(("kypt_detector." + n, p) for n, p in net.kypt_detector.named_parameters())
        grads = torch.autograd.grad(loss, [params[k] for k in GRAD_KEYS])
        d[f"grad{s}__loss"] = np.float64(loss.item())
        for k, gr in zip(GRAD_KEYS, grads):
            d[f"grad{s}__{k}"] = gr.numpy()
    d["grad__seeds"] = np.array(GRAD_SEEDS, dtype=np.int64)
    d["grad__keys"] = np.array(GRAD_KEYS)
    d["threads"] = np.int64(1)
    for path in golden_npz.save(os.path.join(OUT, "g17_recurrent32.npz"), **d):
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
