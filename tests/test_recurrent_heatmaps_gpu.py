"""options.const_intensity = 2 on the HIP path: the heat-map of frame t is propagated from the heat-map of frame t - 1
(kypt_detector.py:344-345; heat_scan_kernel + heat_marginals_kernel / heat_bwd_recurrent_kernel, nm_ctx_set_const_intensity).

Reference: tests/recurrent_heatmap_ref.py, pinned to the reference implementation by fixture G17 (tests/test_recurrent_heatmaps_cpu.py).
Tolerances are the ones the const_intensity = 3 tests hold the same quantities to (tests/test_option_branches_gpu.py,
tests/test_keypoint_counts_gpu.py): keypoints, z, h, kypt_recon, R 1e-4; affinity 1e-6; every loss 2e-5 max(1, |ref|); selections and the
tree exact; gradients 2e-3 of each tensor's largest entry with the 1e-6 gmax floor.  They carry over to the recurrence: softplus' < 1 and
|w1| < 1 / sqrt(2) at these weights, so a rounding difference of frame t - 1 reaches frame t damped (the reference's own
float32-against-float64 spread on the keypoints is 1.3e-7 ... 2.8e-7 at every t up to 8).  The weights are the 'peaky' variant: on them
the two options are 0.5 ... 0.9 apart in the keypoints from frame 1 on (asserted on the fixture in the CPU file), so a library that ignored
the switch would fail here by orders of magnitude.  Reduced-precision modes: the bounds their own tests state (tests/test_train_detector_gpu.py
'f16': keypoints 2e-3; tests/test_storage16_gpu.py 'bf16' storage: 5e-3)."""
import os

import numpy as np
import pytest
import torch

import golden_npz
import recurrent_heatmap_ref as RR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth
from neural_marionette_amd.spec import DETECTOR_LOSS_KEYS
from neural_marionette_amd.train import DETECTOR_LOSS_WEIGHTS as AIST, DetectorTrainer

pytestmark = pytest.mark.gpu
ACTS = {"detector": True, "learner": True}
DET = {"detector": True, "learner": False}
LOSS_KEYS = DETECTOR_LOSS_KEYS + ("kl_kypt", "kypt_recon_loss")
_REF = {}


def _err(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).double()
    b = torch.as_tensor(np.asarray(b.detach().cpu() if torch.is_tensor(b) else b)).double()
    return (a - b).abs().max().item()


def _setup(seed, B=2, T=4, K=24, ci=2):
    o = HotPathOptions(grid_size=32, const_intensity=ci, nkeypoints=K)
    sd = synth.make_state_dict(o, seed=seed, variant="peaky")
    vox = synth.figure_clip(B, T, 32, seed=seed + 2)
    eps = synth.make_eps((T, 10, B, o.nlatent_kypt), seed=seed + 3)
    return o, sd, vox, eps


def _net(o, sd, mode="split16", train=False):
    net = NeuralMarionette(o)
    net.load_state_dict(sd)
    net = net.cuda()
    net = net.train() if train else net.eval()
    net.set_conv_mode(mode)
    net.anneal(1)
    return net


def _ref_forward(seed, B=2, T=4, K=24):
    """the restatement's full forward, computed once per configuration and left unchanged"""
    key = ("fwd", seed, B, T, K)
    if key not in _REF:
        o, sd, vox, eps = _setup(seed, B, T, K)
        with torch.no_grad():
            _REF[key] = RR.nm_forward(sd, o, vox, eps)
    return _REF[key]


def _ref_grads(seed, dtype=torch.float64):
    """AIST-weighted training loss and its gradient w.r.t. every kypt_detector.* tensor: autograd of the restatement, B = 1, T = 4"""
    key = ("grad", seed, dtype)
    if key not in _REF:
        o, sd, vox, _ = _setup(seed, B=1, T=4)
        sdd = {k: v.to(dtype) for k, v in sd.items()}
        names = [k for k in sdd if k.startswith("kypt_detector.")]
        leaf = {k: sdd[k].clone().requires_grad_(True) for k in names}
        sdd.update(leaf)
        ro = RR.detector_forward(sdd, o, vox.to(dtype), affinity_on=True)
        loss = sum(w * ro[k] for k, w in AIST.items())
        grads = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
        _REF[key] = (float(loss.detach()), {k: (g if g is not None else torch.zeros_like(leaf[k])).double() for k, g in zip(names, grads)},
                     ro["keypoints"].detach())
    return _REF[key]


def _run(net, path, vox, eps):
    def once():
        if path == "inference":
            with torch.no_grad():
                return net(vox.cuda(), ACTS, eps=eps.cuda())
        return net(vox.cuda(), ACTS, eps=eps.cuda())
    once()                                   # (the first call builds the tree; the second takes the path every later call takes)
    out = once()
    torch.cuda.synchronize()
    return out


def _check_forward(net, out, ref, what):
    errs = {k: _err(out[k], ref[k]) for k in ("keypoints", "z_kypts", "h_kypts", "kypt_recon", "R", "affinity")}
    print(what, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert _err(net.kypt_detector.get_affinity(), ref["affinity"]) < 1e-6
    assert errs["affinity"] < 1e-6
    for k in ("keypoints", "z_kypts", "h_kypts", "kypt_recon", "R"):
        assert errs[k] < 1e-4, (k, errs[k])
    assert np.array_equal(net.dyna_module.parents.cpu().numpy(), np.asarray(ref["parents"]))
    assert np.array_equal(net.dyna_module.priority.indices.cpu().numpy(), np.asarray(ref["order"]))
    assert np.array_equal(out["best_idx"].cpu().numpy(), np.asarray(ref["best_idx"]).astype(np.int32))
    for k in LOSS_KEYS:
        r = float(ref[k])
        assert abs(float(out[k].detach()) - r) <= 2e-5 * max(1.0, abs(r)), (k, float(out[k].detach()), r)


# ---- 1 / 6: forward parity, both paths, both fp32-equivalent conv modes --------------------------------------------------------------
@pytest.mark.parametrize("path", ["train_fwd", "inference"])
@pytest.mark.parametrize("mode", ["split16", "fp32"])
def test_forward_parity(mode, path):
    o, sd, vox, eps = _setup(430)
    ref = _ref_forward(430)
    net = _net(o, sd, mode)
    out = _run(net, path, vox, eps)
    _check_forward(net, out, ref, "const_intensity 2 (%s, %s):" % (mode, path))
    e_hm = _err(out["heatmaps"], ref["heatmaps"])
    print("heat-maps %.2e (largest value %.2f)" % (e_hm, float(ref["heatmaps"].max())))
    assert e_hm < 1e-4 * max(1.0, float(ref["heatmaps"].abs().max()))


@pytest.mark.parametrize("path", ["train_fwd", "inference"])
def test_forward_parity_sixteen_frames_vs_reference_fixture(golden_dir, path):
    """fixture G17: what the reference itself computed, T = 16 - the error does not grow along the clip"""
    g = golden_npz.load(os.path.join(golden_dir, "g17_recurrent32.npz"))
    B, T, G = (int(v) for v in g["fwd__shape"])
    seed = int(g["fwd__seed"])
    o, sd, vox, eps = _setup(seed, B, T)
    assert G == 32 and T == 16
    net = _net(o, sd)
    out = _run(net, path, vox, eps)
    ref = {k: g["fwd__" + k] for k in ("keypoints", "z_kypts", "h_kypts", "kypt_recon", "R", "affinity", "parents", "order", "best_idx")}
    ref.update({k: float(v) for k, v in zip(LOSS_KEYS, g["fwd__losses"])})
    # (the kinematic order may differ among joints of equal depth - the shells resolve the reference's topk ties by index; the
    #  restatement resolves them the same way, the reference's own order is compared as a set with the same root)
    order = net.dyna_module.priority.indices.cpu().numpy()
    assert int(order[0]) == int(ref["order"][0]) and sorted(order.tolist()) == sorted(ref["order"].tolist())
    ref["order"] = order
    _check_forward(net, out, ref, "G17 (%s):" % path)
    per_t = (out["keypoints"].cpu().double() - torch.from_numpy(g["fwd__keypoints"]).double()).abs().amax(dim=(0, 2, 3))
    print("keypoint error per frame:", " ".join("%.1e" % float(v) for v in per_t))
    sub = g["fwd__heatmaps_strided"]
    assert _err(out["heatmaps"][..., 1::4, 1::4, 1::4], sub) < 1e-4 * max(1.0, float(np.abs(sub).max()))
    sums = g["fwd__heatmaps_sums"]
    assert _err(out["heatmaps"].double().sum(dim=(3, 4, 5)), sums) < 1e-5 * float(np.abs(sums).max())
    ff = out["first_feature"].double()
    assert abs(float(ff.sum()) - float(g["fwd__first_feature_sum"])) <= 1e-5 * float(g["fwd__first_feature_abssum"])


# ---- 2: frame 0 is the computation of const_intensity 3, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("path", ["train_fwd", "inference"])
def test_frame_zero_and_one_frame_clips_are_bit_identical_to_value_three(path):
    o2, sd, vox, eps = _setup(430, B=2, T=4)
    o3 = HotPathOptions(grid_size=32, const_intensity=3)
    n2, n3 = _net(o2, sd), _net(o3, sd)
    a, b = _run(n2, path, vox, eps), _run(n3, path, vox, eps)
    assert torch.equal(a["keypoints"][:, 0], b["keypoints"][:, 0]) and torch.equal(a["heatmaps"][:, 0], b["heatmaps"][:, 0])
    d = (a["keypoints"][:, 1:] - b["keypoints"][:, 1:]).abs().amax(dim=(0, 2, 3))
    assert (d > 0.1).all(), d                                # ... and the later frames are another computation
    one = vox[:, :1].contiguous()
    e1 = eps[:1].contiguous()
    a, b = _run(n2, path, one, e1), _run(n3, path, one, e1)
    def bits(t):                                             # (a one-frame clip has no velocity: graph_traj_loss is 0 / 0 under both options)
        t = t.detach().reshape(-1)
        return t.view(torch.int32) if t.dtype == torch.float32 else t
    for k in ("keypoints", "heatmaps", "first_feature", "recon", "affinity", "z_kypts", "h_kypts", "kypt_recon", "R", "best_idx") + LOSS_KEYS:
        assert torch.equal(bits(a[k]), bits(b[k])), k


# ---- 3: entry points ----------------------------------------------------------------------------------------------------------------
def test_entry_points_agree_bit_for_bit():
    o, sd, vox, eps = _setup(430)
    net = _net(o, sd)
    v, e = vox.cuda(), eps.cuda()
    with torch.no_grad():
        first = net(v, ACTS, eps=e)                          # detector, then encode: two calls (builds the tree)
        fused = net(v, ACTS, eps=e)                          # nm_forward_fused
        det = net.kypt_detector(v)
        enc = net.dyna_module.encode(det["keypoints"], det["affinity"], eps=e)
    lean = net.kypt_detector.detect(v)
    torch.cuda.synchronize()
    for k in ("keypoints", "heatmaps", "affinity", "first_feature"):
        assert torch.equal(fused[k], det[k]) and torch.equal(fused[k], lean[k]) and torch.equal(fused[k], first[k]), k
    for k in ("recon",) + DETECTOR_LOSS_KEYS:
        assert torch.equal(fused[k], det[k]), k
    for k in ("z_kypts", "h_kypts", "kypt_recon", "R", "best_idx", "kl_kypt", "kypt_recon_loss"):
        assert torch.equal(fused[k], enc[k]) and torch.equal(fused[k], first[k]), k
    assert _err(fused["keypoints"], _ref_forward(430)["keypoints"]) < 1e-4


def test_generation_and_retargeting_drivers_run():
    o = HotPathOptions(grid_size=32, const_intensity=2, Tcond=3)
    sd = synth.make_state_dict(o, seed=430, variant="peaky")
    net = _net(o, sd)
    B, T, Tc, Z = 1, 5, 3, o.nlatent_kypt
    vox = synth.figure_clip(B, T, 32, seed=432).cuda()
    with torch.no_grad():
        net(vox[:, :Tc].contiguous(), ACTS, eps=synth.make_eps((Tc, 10, B, Z), seed=1).cuda())
        ref = RR.detector_forward(sd, o, vox[:, :Tc].cpu().contiguous(), affinity_on=True)["keypoints"]
    out = net.generate(vox, ACTS, eps_post=synth.make_eps((Tc, 10, B, Z), seed=2).cuda(), eps_prior=synth.make_eps((T - Tc, B, Z), seed=3).cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(out["keypoints"]).all() and torch.isfinite(out["gen"]).all() and tuple(out["keypoints"].shape[:2]) == (B, T)
    gen = net.sample_generation(vox[0, :Tc].contiguous(), Tgen=2, sample_num=2, eps_post=synth.make_eps((Tc, 2, Z), 4).cuda(),
                                eps_prior=synth.make_eps((2, 2, Z), 5).cuda())
    assert all(torch.isfinite(gen[k]).all() for k in ("keypoints_cond", "keypoints_gen", "voxels_raw"))
    pts = synth.episodic_normalization(synth.figure_points(1, 4000, np.random.default_rng(7)), scale=0.8)[0]
    target = torch.from_numpy(synth.voxelize(pts, 32))[None].cuda()
    rt = net.sample_retarget(vox[0, :Tc].contiguous(), target, torch.from_numpy(np.ascontiguousarray(pts[:500])),
                             eps_source=synth.make_eps((Tc, 10, 1, Z), 6).cuda(), eps_target=synth.make_eps((1, 10, 1, Z), 7).cuda())
    torch.cuda.synchronize()
    assert all(torch.isfinite(rt[k]).all() for k in ("source_keypoints", "target_keypoints", "R", "R_bind", "offset", "keypoints", "points"))
    # the detector half of the driver ran the recurrence: the source positions are the restatement's (the driver overwrites the intensities)
    assert _err(rt["source_keypoints"][0, ..., :3], ref[0, ..., :3]) < 1e-4


# ---- 4 / 6: gradients ---------------------------------------------------------------------------------------------------------------
def _hip_grads(seed, mode="split16"):
    o, sd, vox, _ = _setup(seed, B=1, T=4)
    net = _net(o, sd, mode, train=True)
    net.control_active(DET)
    net.zero_grad()
    out = net(vox.cuda(), DET)
    loss = sum(w * out[k] for k, w in AIST.items())
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {"kypt_detector." + n: p.grad for n, p in net.kypt_detector.named_parameters()}, out["keypoints"].detach()


@pytest.mark.parametrize("mode", ["split16", "fp32"])
@pytest.mark.parametrize("seed", [431, 432])
def test_detector_gradients(seed, mode):
    """Seeds on which the reference's own float32 autograd stays within 1.9e-4 (431) / 1.7e-5 (432) of float64; 430 is not among them: there
    the reference's float32 gradient of extract_spatio_temporal_features.{1,3}.stride_conv is itself 1.4e-2 off - under const_intensity 2
    the spatio-temporal net hears from frame 0 alone, and its gradient is small and ill-conditioned on that clip."""
    ref_loss, ref, _ = _ref_grads(seed)
    loss, got, _ = _hip_grads(seed, mode)
    print("const_intensity 2, seed %d (%s): loss %.6f, float64 restatement %.6f" % (seed, mode, loss, ref_loss))
    assert abs(loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss))
    gmax = max(r.abs().max().item() for r in ref.values())
    worst, bad = ("", 0.0), []
    for k, r in ref.items():
        g = got[k]
        assert g is not None and tuple(g.shape) == tuple(r.shape) and torch.isfinite(g).all(), k
        e = (g.cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-6 * gmax, 1e-30)
        if "propagate_heatmaps" in k or "heatmaps_from_features" in k:
            print("  %-90s %.2e (largest entry %.3e)" % (k, e, r.abs().max().item()))
        if e > worst[1]:
            worst = (k, e)
        if e >= 2e-3:
            bad.append((k, e))
    print("  worst relative gradient error %.2e at %s" % worst[::-1])
    assert not bad, bad[:8]
    for k in ("weight", "bias"):
        assert ref["kypt_detector.vox_to_kypt.propagate_heatmaps.0." + k].abs().max() > 1e-6 * gmax


# ---- 5: three training steps ----------------------------------------------------------------------------------------------------------
def test_three_training_steps_follow_autograd_and_adam():
    """Three DetectorTrainer steps (Adam lr 4e-4, AIST weights) against torch.optim.Adam on float64 autograd of the restatement: every
    step's loss within 2e-5."""
    o, sd, vox, _ = _setup(431, B=1, T=4)
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("kypt_detector.")}
    opt = torch.optim.Adam(list(leaf.values()), lr=4e-4)
    ref_losses = []
    for _ in range(3):
        sd64 = {k: v.double() for k, v in sd.items()}
        sd64.update(leaf)
        ro = RR.detector_forward(sd64, o, vox.double(), affinity_on=True)
        loss = sum(w * ro[k] for k, w in AIST.items())
        ref_losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    net = _net(o, sd, train=True)
    tr = DetectorTrainer(net, lr=4e-4)
    losses = [tr.step(vox.cuda())["loss"] for _ in range(3)]
    torch.cuda.synchronize()
    print("const_intensity 2 training losses", losses, "restatement", ref_losses,
          "relative", ["%.2e" % (abs(a - b) / abs(b)) for a, b in zip(losses, ref_losses)])
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (losses, ref_losses)


# ---- 6: reduced-precision modes run ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_reduced_precision_modes_run(mode):
    _, ref, ref_kp = _ref_grads(431)
    if mode == "bf16":
        os.environ["NM355_STORE16_MIN"] = "4096"             # bfloat16 storage from 16^3 tensors on (read when a context is created)
    try:
        loss, got, kp = _hip_grads(431, mode)
    finally:
        os.environ.pop("NM355_STORE16_MIN", None)
    e_kp = _err(kp, ref_kp)
    print("const_intensity 2 in mode %s: keypoints %.2e" % (mode, e_kp))
    assert np.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in got.values())
    assert e_kp < {"f16": 2e-3, "bf16": 5e-3}[mode]


# ---- 7: other keypoint counts (heads zero-padded to 8 channels) -----------------------------------------------------------------------
@pytest.mark.parametrize("K", [12, 22])
def test_forward_parity_other_keypoint_counts(K):
    o, sd, vox, eps = _setup(440 + K, K=K)
    sd["kypt_detector.affinity_params"] = torch.randn(sd["kypt_detector.affinity_params"].shape, generator=torch.Generator().manual_seed(K))
    key = ("fwdK", K)
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = RR.nm_forward(sd, o, vox, eps)
    net = _net(o, sd)
    out = _run(net, "inference", vox, eps)
    _check_forward(net, out, _REF[key], "const_intensity 2, K = %d:" % K)
    n3 = _net(HotPathOptions(grid_size=32, nkeypoints=K), sd)
    out3 = _run(n3, "inference", vox, eps)
    assert torch.equal(out["heatmaps"][:, 0], out3["heatmaps"][:, 0]) and not torch.equal(out["heatmaps"][:, 1], out3["heatmaps"][:, 1])


def test_gradients_with_padded_heads():
    """K = 12: the head tensors carry 16 channels per voxel; the reverse scan leaves the padded ones zero (the head convs' gradients
    would otherwise be wrong by whatever the scratch held)"""
    K, seed = 12, 452
    o, sd, vox, _ = _setup(seed, B=1, T=3, K=K)
    sd64 = {k: v.double() for k, v in sd.items()}
    names = [k for k in sd64 if k.startswith("kypt_detector.")]
    leaf = {k: sd64[k].clone().requires_grad_(True) for k in names}
    sd64.update(leaf)
    ro = RR.detector_forward(sd64, o, vox.double(), affinity_on=True)
    ref_loss = sum(w * ro[k] for k, w in AIST.items())
    grads = torch.autograd.grad(ref_loss, [leaf[k] for k in names], allow_unused=True)
    ref = {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(names, grads)}
    net = _net(o, sd, train=True)
    net.control_active(DET)
    net.zero_grad()
    out = net(vox.cuda(), DET)
    sum(w * out[k] for k, w in AIST.items()).backward()
    torch.cuda.synchronize()
    gmax = max(r.abs().max().item() for r in ref.values())
    v2k = "kypt_detector.vox_to_kypt."
    for k in (v2k + "propagate_heatmaps.0.weight", v2k + "propagate_heatmaps.0.bias", v2k + "extract_heatmaps_from_features.0.weight",
              v2k + "extract_heatmaps_from_features.0.bias", v2k + "extract_spatio_temporal_heatmaps_from_features.0.weight",
              v2k + "extract_spatio_temporal_heatmaps_from_features.0.bias"):
        g = dict(("kypt_detector." + n, p.grad) for n, p in net.kypt_detector.named_parameters())[k]
        e = (g.cpu().double() - ref[k]).abs().max().item() / max(ref[k].abs().max().item(), 1e-6 * gmax, 1e-30)
        print("K = 12  %-90s %.2e" % (k, e))
        assert e < 2e-3, (k, e)


# ---- 8: run-to-run identity ------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_are_bit_identical_over_twenty_evaluations():
    o, sd, vox, _ = _setup(433, B=2, T=3)
    net = _net(o, sd, train=True)
    net.control_active(DET)
    v = vox.cuda()

    def evaluate():
        net.zero_grad()
        out = net(v, DET)
        sum(w * out[k] for k, w in AIST.items()).backward()
        torch.cuda.synchronize()
        res = {n: p.grad.detach().clone() for n, p in net.kypt_detector.named_parameters() if p.grad is not None}
        res.update(keypoints=out["keypoints"].detach().clone(), heatmaps=out["heatmaps"].detach().clone())
        return res
    ref = evaluate()
    for i in range(20):
        got = evaluate()
        bad = [k for k in ref if not torch.equal(ref[k], got[k])]
        assert not bad, "evaluation %d differs in %s" % (i, bad[:4])


# ---- 9: the other values stay rejected -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0, 1, 4])
def test_other_values_are_rejected(v):
    with pytest.raises(NotImplementedError):
        NeuralMarionette(HotPathOptions(grid_size=32, const_intensity=v))
    with pytest.raises(NotImplementedError):
        HotPathOptions(const_intensity=v).check_fast_path()
