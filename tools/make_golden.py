#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE (imported from /root/reference)
on the build's seeded synthetic weights and inputs.

Runs only in the build container (the reference tree does not travel to the GPU
box).  Fixtures hold seeds + expected outputs of the reference itself; inputs and
weights are re-created from the seeds by ``neural_marionette_amd.synth``.

  python tools/make_golden.py            # writes every case
  python tools/make_golden.py g2 g3      # subset

The VRNN noise is injected by replacing ``torch.distributions.normal._standard_normal``
(the name ``Normal.rsample`` resolves at call time).
"""
from __future__ import annotations

import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from neural_marionette_amd.spec import HotPathOptions, DETECTOR_LOSS_KEYS  # noqa: E402
from neural_marionette_amd import synth  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
S = 10


def _ref_opt(G):
    opt = pickle.load(open(os.path.join(REF, "pretrained/aist/opt.pickle"), "rb"))
    opt.grid_size = G
    return opt


def _ref_net(opt, sd):
    from model.neural_marionette import NeuralMarionette
    net = NeuralMarionette(opt).eval()
    net.load_state_dict(sd)
    net.anneal(1)           # switches the affinity graph on (kypt_detector.py:71-78)
    return net


class EpsFeed:
    """Feeds pre-drawn eps tensors to Normal.rsample in call order."""

    def __init__(self, chunks):
        self.chunks = list(chunks)
        self.i = 0

    def __call__(self, shape, dtype, device):
        e = self.chunks[self.i]
        self.i += 1
        assert tuple(shape) == tuple(e.shape), (tuple(shape), tuple(e.shape))
        return e.clone()

    def __enter__(self):
        import torch.distributions.normal as tdn
        self._tdn, self._old = tdn, tdn._standard_normal
        tdn._standard_normal = self
        return self

    def __exit__(self, *a):
        self._tdn._standard_normal = self._old


def _np(x):
    return x.detach().cpu().numpy()


def _sub(x, step):
    """strided spatial sub-sample of the last three dims"""
    return _np(x[..., ::step, ::step, ::step])


def case_g1():
    """Config 1 of BASELINE.json: 64^3, B=1, T=4, detector forward only."""
    G, B, T, wseed, iseed = 64, 1, 4, 11, 21
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant="peaky")
    net = _ref_net(opt, sd)
    vox = synth.figure_clip(B, T, G, seed=iseed)
    with torch.no_grad():
        r = net.kypt_detector(vox)
    np.savez_compressed(
        os.path.join(OUT, "g1_detector64.npz"),
        meta=np.array([G, B, T, wseed, iseed]), variant="peaky", clip="figure",
        keypoints=_np(r["keypoints"]),
        losses=np.array([float(r[k]) for k in DETECTOR_LOSS_KEYS], dtype=np.float64),
        heatmaps_sub=_sub(r["heatmaps"], 2), heatmaps_sum=_np(r["heatmaps"].sum(dim=(3, 4, 5))),
        first_feature_sub=_sub(r["first_feature"], 2),
        first_feature_sum=_np(r["first_feature"].double().sum(dim=(2, 3, 4))),
        recon_sub=_sub(r["recon"], 4), recon_sum=_np(r["recon"].double().sum(dim=(2, 3, 4, 5))),
        recon_occ=_np((r["recon"] >= 0.5).sum(dim=(2, 3, 4, 5))),
        recon_margin=np.array(float((r["recon"] - 0.5).abs().min())),
        affinity=_np(r["affinity"]),
    )
    print("g1 ok", float(r["recon_loss"]))


def case_g2():
    """32^3 B=2 T=4 full forward (detector + VRNN.encode) with recorded eps."""
    G, B, T, wseed, iseed, eseed = 32, 2, 4, 3, 5, 9
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant="peaky")
    net = _ref_net(opt, sd)
    vox = synth.figure_clip(B, T, G, seed=iseed)
    eps = synth.make_eps((T, S, B, o.nlatent_kypt), seed=eseed)
    with torch.no_grad(), EpsFeed(eps):
        r = net(vox, {"detector": True, "learner": True})
    d = net.dyna_module
    np.savez_compressed(
        os.path.join(OUT, "g2_forward32.npz"),
        meta=np.array([G, B, T, wseed, iseed, eseed]), variant="peaky", clip="figure",
        keypoints=_np(r["keypoints"]), heatmaps=_np(r["heatmaps"]),
        first_feature=_np(r["first_feature"]),
        recon_sub=_sub(r["recon"], 2), recon_sum=_np(r["recon"].double().sum(dim=(2, 3, 4, 5))),
        recon_occ=_np((r["recon"] >= 0.5).sum(dim=(2, 3, 4, 5))),
        losses=np.array([float(r[k]) for k in DETECTOR_LOSS_KEYS], dtype=np.float64),
        affinity=_np(r["affinity"]),
        kypt_recon=_np(r["kypt_recon"]), R=_np(r["R"]), z_kypts=_np(r["z_kypts"]),
        h_kypts=_np(r["h_kypts"]), kl_kypt=np.array(float(r["kl_kypt"])),
        kypt_recon_loss=np.array(float(r["kypt_recon_loss"])),
        parents=_np(d.parents), order=_np(d.priority.indices), order_values=_np(d.priority.values),
        A=_np(d.A),
    )
    print("g2 ok", float(r["kl_kypt"]))


def case_g3():
    """Skeleton trees: affinity (N,K,K,1) -> (A, parents, priority) for several seeds."""
    from utils.dyna_utils import process_affinity_glob
    K, N = 24, 2

    def affinity_input(params):           # an (N,K,K,1) row-stochastic affinity with a zero diagonal (the fixture stores it)
        P = torch.softmax(params, dim=-1)
        W = torch.zeros(N, K, K, dtype=params.dtype)
        for k in range(K):
            W[:, k, :k] = P[:, k, :k]
            W[:, k, k + 1:] = P[:, k, k:]
        return W[..., None]

    affs, As, pars, ords, vals = [], [], [], [], []
    for seed in range(12):
        rng = np.random.default_rng([seed, 0x73EE])
        if seed == 0:
            params = torch.ones(N, K, K - 1)            # the all-ties init of the reference
        elif seed < 4:
            params = torch.from_numpy(np.round(rng.standard_normal((N, K, K - 1)) * 2) / 2).float()  # many ties
        else:
            params = torch.from_numpy(rng.standard_normal((N, K, K - 1)) * (1 + seed % 3)).float()
        aff = affinity_input(params)
        A, pri, par = process_affinity_glob(aff)
        affs.append(_np(aff)); As.append(_np(A)); pars.append(_np(par))
        ords.append(_np(pri.indices)); vals.append(_np(pri.values))
    np.savez_compressed(os.path.join(OUT, "g3_trees.npz"), affinity=np.stack(affs), A=np.stack(As),
                        parents=np.stack(pars), order=np.stack(ords), order_values=np.stack(vals))
    print("g3 ok")


def case_g4():
    """generate(): 32^3, B=2, Tcond=3, Ttot=8 with recorded eps."""
    G, B, T, Tc, wseed, iseed, eseed = 32, 2, 8, 3, 4, 6, 10
    opt = _ref_opt(G)
    opt.Tcond = Tc
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant="peaky")
    net = _ref_net(opt, sd)
    vox = synth.figure_clip(B, T, G, seed=iseed)
    Z = o.nlatent_kypt
    e_enc = synth.make_eps((Tc, S, B, Z), seed=eseed)
    e_post = synth.make_eps((Tc, S, B, Z), seed=eseed + 1)
    e_prior = synth.make_eps((T - Tc, B, Z), seed=eseed + 2)
    acts = {"detector": True, "learner": True}
    with torch.no_grad():
        with EpsFeed(e_enc):        # a first encode builds the tree (generate needs .parents)
            net(vox[:, :Tc].contiguous(), acts)
        with EpsFeed(list(e_post) + list(e_prior)):
            r = net.generate(vox, acts)
    d = net.dyna_module
    np.savez_compressed(
        os.path.join(OUT, "g4_generate32.npz"),
        meta=np.array([G, B, T, Tc, wseed, iseed, eseed]), variant="peaky", clip="figure",
        keypoints=_np(r["keypoints"]), gen_sub=_sub(r["gen"], 2),
        gen_sum=_np(r["gen"].double().sum(dim=(2, 3, 4, 5))),
        gen_occ=_np((r["gen"] >= 0.5).sum(dim=(2, 3, 4, 5))),
        parents=_np(d.parents), order=_np(d.priority.indices),
    )
    print("g4 ok")


def case_g5():
    """Odd-size plumbing (output_padding path of the hourglass): 40^3, B=1, T=3 detector."""
    G, B, T, wseed, iseed = 40, 1, 3, 7, 8
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant="peaky")
    net = _ref_net(opt, sd)
    vox = synth.figure_clip(B, T, G, seed=iseed)
    with torch.no_grad():
        r = net.kypt_detector(vox)
    np.savez_compressed(
        os.path.join(OUT, "g5_detector40.npz"),
        meta=np.array([G, B, T, wseed, iseed]), variant="peaky", clip="figure",
        keypoints=_np(r["keypoints"]), heatmaps=_np(r["heatmaps"]),
        losses=np.array([float(r[k]) for k in DETECTOR_LOSS_KEYS], dtype=np.float64),
        recon_sub=_sub(r["recon"], 2), recon_sum=_np(r["recon"].double().sum(dim=(2, 3, 4, 5))),
    )
    print("g5 ok")


def case_g6():
    """Learner-mode training gradients (pretrained_mode=1: detector frozen, train.py:146,177-181):
    d(1.0 * kypt_recon_loss + 0.003 * kl_kypt) / d(dyna_module parameters) by the reference's autograd,
    B=3, T=5, recorded eps.  Every gradient is stored as (sum, abs-sum, every 97th element)."""
    B, T, wseed, kseed, eseed = 3, 5, 13, 14, 15
    opt = _ref_opt(32)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant="default")
    net = _ref_net(opt, sd)
    g = torch.Generator().manual_seed(kseed)
    kp = torch.rand(B, T, o.nkeypoints, 4, generator=g) * torch.tensor([1.6, 1.6, 1.6, 1.0]) - torch.tensor([0.8, 0.8, 0.8, 0.0])
    eps = synth.make_eps((T, S, B, o.nlatent_kypt), seed=eseed)
    aff = net.kypt_detector.get_affinity().detach()
    for p in net.parameters():
        p.grad = None
    with EpsFeed(eps):
        r = net.dyna_module.encode(kp, aff)
    loss = 1.0 * r["kypt_recon_loss"] + 0.003 * r["kl_kypt"]
    loss.backward()
    out = dict(meta=np.array([B, T, wseed, kseed, eseed]), loss=np.array(float(loss)),
               kypt_recon_loss=np.array(float(r["kypt_recon_loss"])), kl_kypt=np.array(float(r["kl_kypt"])),
               parents=_np(net.dyna_module.parents), order=_np(net.dyna_module.priority.indices))
    for name, p in net.dyna_module.named_parameters():
        if p.grad is None:
            continue
        gflat = p.grad.reshape(-1).double()
        out["g:" + name] = np.concatenate([[gflat.sum().item(), gflat.abs().sum().item()], gflat[::97].numpy()])
    np.savez_compressed(os.path.join(OUT, "g6_learner_grads.npz"), **out)
    print("g6 ok", float(loss), sorted(k for k in out if k.startswith("g:"))[:3])


def case_g7():
    """utils/eval_utils.py on seeded inputs: voxel_chamfer_distance and semantic_scores of the reference."""
    from utils import eval_utils as ref_eval
    vox, recon, kp, gt = synth.eval_inputs()
    ch = ref_eval.voxel_chamfer_distance(None, dict(voxel=vox.clone(), recon=recon.clone()))
    se = ref_eval.semantic_scores(None, dict(keypoints=kp.clone(), gt_keypoints=gt.clone()))
    np.savez_compressed(os.path.join(OUT, "g7_eval_metrics.npz"), seed=7, B=2, T=3, G=32, K=24, Kg=17,
                        recon_checksum=np.float64(recon.double().sum().item()),
                        chamfer_scores=np.array(ch["scores"], dtype=np.float64), chamfer_log=np.float64(ch["scores_log"]),
                        semantic_scores=np.array(se["scores"], dtype=np.int64), semantic_log=np.float32(se["scores_log"]))
    print("g7 ok", ch["scores_log"], se["scores_log"])


def case_g8():
    """Detector-mode training gradients (pretrained_mode=0, train.py:270-276,388-404): d(sum_k w_k * loss_k) / d(kypt_detector
    parameters) by the reference's autograd with the AIST loss weights (train.py:177-181), 32^3, B=2, T=4, 'peaky' weights and
    random affinity logits.  Every gradient is stored as (sum, abs-sum, max-abs, every 997th element)."""
    G, B, T, seed = 32, 2, 4, 11
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=seed, variant="peaky")
    gen = torch.Generator().manual_seed(seed + 1)
    sd["kypt_detector.affinity_params"] = torch.randn(sd["kypt_detector.affinity_params"].shape, generator=gen)
    vox = synth.figure_clip(B, T, G, seed=seed + 2)
    net = _ref_net(opt, sd).train()
    acts = {"detector": True, "learner": False}
    net.control_active(acts)
    for p in net.parameters():
        p.grad = None
    log = net(vox, acts)
    w = dict(recon_loss=opt.recon_weight, sparsity_loss=opt.sparse_weight, separation_loss=opt.sep_weight, vol_fit_reg=opt.vol_reg_weight,
             kypt_const_loss=opt.kypt_const_weight, local_const_loss=opt.local_const_weight, time_const_loss=opt.time_const_weight,
             sparsity_const_loss=opt.sparsity_const_weight, intensity_const_loss=opt.intensity_const_weight,
             graph_traj_loss=opt.graph_traj_weight, graph_vol_loss=opt.graph_vol_weight)
    loss = sum(float(w[k]) * log[k] for k in DETECTOR_LOSS_KEYS)
    loss.backward()
    out = dict(meta=np.array([G, B, T, seed]), loss=np.array(float(loss)), weights=np.array([float(w[k]) for k in DETECTOR_LOSS_KEYS]),
               losses=np.array([float(log[k]) for k in DETECTOR_LOSS_KEYS]))
    n = 0
    for name, p in net.kypt_detector.named_parameters():
        assert p.grad is not None, name
        gflat = p.grad.reshape(-1).double()
        out["g:" + name] = np.concatenate([[gflat.sum().item(), gflat.abs().sum().item(), gflat.abs().max().item()], gflat[::997].numpy()])
        n += 1
    np.savez_compressed(os.path.join(OUT, "g8_detector_grads.npz"), **out)
    print("g8 ok", float(loss), n, "tensors")


def _pack_recon(x, margin=3e-5):
    """A decoded occupancy field (B,T,1,G,G,G) in the compact form the full-size fixtures carry: the thresholded set and the set of
    voxels within `margin` of the threshold as packed bits (every voxel), the values themselves on a stride-4 sub-lattice."""
    x = x.detach()
    return dict(recon_occ_bits=np.packbits(_np(x >= 0.5).reshape(-1)), recon_near_bits=np.packbits(_np((x - 0.5).abs() <= margin).reshape(-1)),
                recon_sub4=_sub(x, 4), recon_sum=_np(x.double().sum(dim=(2, 3, 4, 5))), recon_margin=np.float64(margin))


def _full_forward_case(fname, G, B, T, wseed, iseed, eseed, variant="peaky"):
    """The reference's full forward (detector + VRNN.encode, recorded eps) at a BASELINE configuration's size; best-of-S indices and
    their margins come from the oracle run on the same inputs, which must equal the reference bit for bit (asserted here)."""
    from oracle import nm_oracle as O
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant=variant)
    net = _ref_net(opt, sd)
    vox = synth.figure_clip(B, T, G, seed=iseed)
    eps = synth.make_eps((T, S, B, o.nlatent_kypt), seed=eseed)
    with torch.no_grad(), EpsFeed(eps):
        r = net(vox, {"detector": True, "learner": True})
    with torch.no_grad():
        ro = O.nm_forward(sd, o, vox, eps)
    for k in ("keypoints", "heatmaps", "recon", "z_kypts", "h_kypts", "kypt_recon", "R"):
        assert torch.equal(r[k], ro[k]), k                       # the oracle IS the reference on these inputs
    d = net.dyna_module
    kp = r["keypoints"][..., :3]
    vel = (kp[:, 1:] - kp[:, :-1]).norm(dim=-1)
    golden_npz.save(                                # (parts of <= 768 KB: the 64^3 / 96^3 cases exceed a committed file's 1 MiB)
        os.path.join(OUT, fname),
        meta=np.array([G, B, T, wseed, iseed, eseed]), variant=variant, clip="figure",
        keypoints=_np(r["keypoints"]), heatmaps_sub=_sub(r["heatmaps"], 2), heatmaps_sum=_np(r["heatmaps"].double().sum(dim=(3, 4, 5))),
        heatmaps_absmax=np.float64(r["heatmaps"].abs().max()),
        first_feature_sub=_sub(r["first_feature"], 2), first_feature_absmax=np.float64(r["first_feature"].abs().max()),
        losses=np.array([float(r[k]) for k in DETECTOR_LOSS_KEYS], dtype=np.float64),
        affinity=_np(r["affinity"]),
        kypt_recon=_np(r["kypt_recon"]), R=_np(r["R"]), z_kypts=_np(r["z_kypts"]), h_kypts=_np(r["h_kypts"]),
        kl_kypt=np.float64(r["kl_kypt"]), kypt_recon_loss=np.float64(r["kypt_recon_loss"]),
        best_idx=_np(ro["best_idx"]).astype(np.int32), keypoint_speed_median=np.float64(vel.median()),
        parents=_np(d.parents), order=_np(d.priority.indices),
        **_pack_recon(r["recon"]),
    )
    print(fname, "ok: recon_loss", float(r["recon_loss"]), "kl", float(r["kl_kypt"]), "median keypoint speed %.2e" % float(vel.median()))


def case_g9():
    """BASELINE config 2 as the bench and tests/test_network_gpu.py::test_config2_* run it: 64^3, B=4, T=16, weights seed 42, clip seed 77."""
    _full_forward_case("g9_config2_forward64.npz", 64, 4, 16, 42, 77, 78)


def case_g10():
    """BASELINE config 4: 96^3, B=2, T=8 (hourglass 24 -> 12 -> 6 -> 3), weights seed 9, clip seed 31."""
    _full_forward_case("g10_config4_forward96.npz", 96, 2, 8, 9, 31, 32)


def case_g12():
    """A clip whose keypoints MOVE (variant 'tracking': median frame-to-frame keypoint speed ~3e-2): the trajectory term of the graph
    loss (kypt_detector_utils.py:228-265) is well conditioned there and is held to the plain 2e-5 like the other ten."""
    _full_forward_case("g12_tracking32.npz", 32, 2, 6, 3, 5, 9, variant="tracking")


def _ref_interpolation(net, vox, rate, Sn, ea, eb):
    """The loop of vis_interpolation.py:80-143 on the reference's own sub-modules (the script imports open3d / cv2 and cannot be
    imported): returns the selected keypoints (1, T, K, 4) and the (posterior, prior) picks of every key frame."""
    import torch.distributions.normal as tdn
    from torch.distributions.normal import Normal
    import torch.nn.functional as F
    dm = net.dyna_module
    T = vox.shape[0]
    draws = []
    for t in range(T):
        draws += [ea[t], eb[t]] if (t % rate == 0 or t == T - 1) else [ea[t]]
    with torch.no_grad():
        det = net.kypt_detector(vox[None])
        kp = det["keypoints"]
        Tn = kp.shape[1]
        with EpsFeed([torch.zeros(S, 1, 128) for _ in range(Tn)]):
            dm.encode(kp, det["affinity"])                   # builds the tree (its own draws are irrelevant)
        K = kp.shape[2]
        with EpsFeed(draws):
            h = dm.init_kypt_rnn_state.expand(Sn, -1)
            off = dm.get_offset(kp).expand(Sn, -1, -1, -1)
            sel, pend, picks = [], [], []
            for t in range(T):
                flat = kp[:, t].clone().view(1, -1).expand(Sn, -1)
                if t % rate == 0 or t == T - 1:
                    mu, sg = torch.chunk(dm.extract_post_dist(torch.cat([h, flat], -1)), 2, -1)
                    pm, ps = torch.chunk(dm.extract_prior_dist(h), 2, -1)
                    z = Normal(mu, F.softplus(sg) + 1e-4).rsample()
                    zc = Normal(pm, F.softplus(ps) + 1e-4).rsample()
                    f, _ = dm.extract_kypt_from_latent_and_state(torch.cat([h, z], -1), off)
                    fc, _ = dm.extract_kypt_from_latent_and_state(torch.cat([h, zc], -1), off)
                    i = (f - flat).pow(2).sum(-1).argmin()
                    f, z, h = f[i][None].expand(Sn, -1), z[i][None].expand(Sn, -1), h[i][None].expand(Sn, -1)
                    j = (fc - f).pow(2).sum(-1).argmin()
                    pend.append(flat)
                    sel += [s_[j].view(K, 4) for s_ in pend]
                    pend = []
                    picks.append((int(i), int(j)))
                else:
                    pm, ps = torch.chunk(dm.extract_prior_dist(h), 2, -1)
                    z = Normal(pm, F.softplus(ps) + 1e-4).rsample()
                    f, _ = dm.extract_kypt_from_latent_and_state(torch.cat([h, z], -1), off)
                    pend.append(f)
                h = dm.kypt_rnn_cell(torch.cat([f, z], -1), h)
            sel = torch.stack(sel, 0)[None].clone()
            sel[0, :, :, -1] = sel[0, 0, :, -1]
        dec = net.kypt_detector.decode_from_dyna(sel, det["first_feature"], vox[None, 0])["gen"][0]
    return sel, picks, dec


def case_g11():
    """The interpolation driver (vis_interpolation.py:80-143) at S = 256 (T = 11, key frames every 5) and at the demo's S = 10 000
    (T = 5, every 2) - the shape where the VRNN MLPs are real GEMMs: selected keypoints, the picks of every key frame with the relative
    gap between the best and second-best candidate (from the oracle, which must reproduce the reference's picks and keypoints
    exactly), thresholded voxels as packed bits."""
    from oracle import nm_oracle as O
    G, wseed, iseed = 32, 29, 8
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=wseed, variant="peaky")
    net = _ref_net(opt, sd)
    out = dict(meta=np.array([G, wseed, iseed]))
    full = synth.figure_clip(1, 11, G, seed=iseed)[0]
    for tag, T, Sn, rate, sa, sb in (("a", 11, 256, 5, 9, 10), ("b", 5, 10000, 2, 11, 12)):
        vox = full[:T]
        ea, eb = synth.make_eps((T, Sn, 128), sa), synth.make_eps((T, Sn, 128), sb)
        sel, picks, dec = _ref_interpolation(net, vox, rate, Sn, ea, eb)
        with torch.no_grad():
            mine = O.sample_interpolation(sd, o, vox, rate, Sn, ea, eb)
        assert torch.equal(mine["keypoints"], sel) and [tuple(p) for p in mine["picks"]] == picks, tag
        assert torch.equal(mine["voxels_raw"], dec), tag
        out.update({tag + "_meta": np.array([T, Sn, rate, sa, sb]), tag + "_keypoints": _np(sel), tag + "_picks": np.array(picks, dtype=np.int64),
                    tag + "_margins": np.array(mine["margins"], dtype=np.float64),
                    tag + "_vox_bits": np.packbits(_np(dec >= 0.5).reshape(-1)), tag + "_vox_near_bits": np.packbits(_np((dec - 0.5).abs() <= 1e-3).reshape(-1))})
        print("g11", tag, "picks", picks, "margins", ["%.1e/%.1e" % tuple(m) for m in mine["margins"]])
    np.savez_compressed(os.path.join(OUT, "g11_interpolation32.npz"), **out)
    print("g11 ok")



def case_g13():
    """Detector-mode TRAINING by the reference itself (train.py:270-276, 376-412: pretrained_mode = 0, the 11 losses with the AIST
    weights of train.py:177-181, torch.optim.Adam(lr 4e-4), no effective clipping): the loss of each of 20 consecutive steps at 32^3,
    B=2, T=4 ('peaky' weights seed 41, random affinity logits, clip seed 43 - tests/test_train_detector_gpu.py::_setup(seed=41)), and
    every detector tensor after step 3 as (sum, abs-sum, every 997th element).  The GPU tests compare DetectorTrainer's trajectory
    with this instead of training the CPU oracle on the box (25 s + 160 s of the round-5 suite)."""
    G, B, T, seed, steps = 32, 2, 4, 41, 20
    opt = _ref_opt(G)
    o = HotPathOptions.from_any(opt)
    sd = synth.make_state_dict(o, seed=seed, variant="peaky")
    gen = torch.Generator().manual_seed(seed + 1)
    sd["kypt_detector.affinity_params"] = torch.randn(sd["kypt_detector.affinity_params"].shape, generator=gen)
    vox = synth.figure_clip(B, T, G, seed=seed + 2)
    net = _ref_net(opt, sd).train()
    acts = {"detector": True, "learner": False}
    net.control_active(acts)
    w = dict(recon_loss=opt.recon_weight, sparsity_loss=opt.sparse_weight, separation_loss=opt.sep_weight, vol_fit_reg=opt.vol_reg_weight,
             kypt_const_loss=opt.kypt_const_weight, local_const_loss=opt.local_const_weight, time_const_loss=opt.time_const_weight,
             sparsity_const_loss=opt.sparsity_const_weight, intensity_const_loss=opt.intensity_const_weight,
             graph_traj_loss=opt.graph_traj_weight, graph_vol_loss=opt.graph_vol_weight)
    params = [p for p in net.kypt_detector.parameters() if p.requires_grad]
    optim = torch.optim.Adam(params, lr=4e-4)
    losses, per = [], []
    out = dict(meta=np.array([G, B, T, seed, steps]), weights=np.array([float(w[k]) for k in DETECTOR_LOSS_KEYS]))
    for it in range(steps):
        optim.zero_grad()
        log = net(vox, acts)
        loss = sum(float(w[k]) * log[k] for k in DETECTOR_LOSS_KEYS)
        loss.backward()
        optim.step()
        losses.append(float(loss))
        per.append([float(log[k]) for k in DETECTOR_LOSS_KEYS])
        if it == 2:
            for name, p in net.kypt_detector.named_parameters():
                f = p.detach().reshape(-1).double()
                out["w3:" + name] = np.concatenate([[f.sum().item(), f.abs().sum().item()], f[::997].numpy()])
        print("g13 step", it, losses[-1], flush=True)
    out["losses"] = np.array(losses, dtype=np.float64)
    out["per_loss"] = np.array(per, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "g13_detector_training20.npz"), **out)
    print("g13 ok", losses[0], "->", losses[-1])


CASES = dict(g1=case_g1, g2=case_g2, g3=case_g3, g4=case_g4, g5=case_g5, g6=case_g6, g7=case_g7, g8=case_g8, g9=case_g9, g10=case_g10, g11=case_g11, g12=case_g12, g13=case_g13)

if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
