"""Pins the oracle directly against the reference implementation through fixture G14 (tests/golden/g14_oracle_vs_reference.*.npz,
written by tools/make_reference_fixtures.py from a checkout of the reference): what the reference computed on these very inputs,
each tensor stored as it is or, above 16 384 elements, as a seeded sample with its sums (floating point) or the SHA-256 of its bytes
(anything else).  The reference's option set (its pretrained/aist/opt.pickle) is tests/golden/aist_opt.json.

Discrete results (layouts, seeded initial weights, trees, occupancy grids, vote counts) are compared exactly.  Floating-point results
are compared to TOL relative to the tensor's scale, as in tests/test_oracle_golden.py: run side by side on one machine the oracle and
the reference agree bit for bit, but the CPU kernels' rounding differs between CPU models (1e-8 .. 2e-6 measured on these fixtures).
The oracle runs with the fixture's intra-op thread count, the count the reference ran with."""
import argparse
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import golden_npz

from neural_marionette_amd import synth
from neural_marionette_amd.spec import HotPathOptions, DETECTOR_LOSS_KEYS, param_spec
from oracle import nm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LOSS_KEYS = DETECTOR_LOSS_KEYS + ("kl_kypt", "kypt_recon_loss")
TOL = 2e-5


@pytest.fixture(scope="module")
def g14():
    g = golden_npz.load(os.path.join(GOLD, "g14_oracle_vs_reference.npz"))
    old = torch.get_num_threads()
    torch.set_num_threads(int(g["threads"]))
    yield g
    torch.set_num_threads(old)


def _opt(G, **kw):
    with open(os.path.join(GOLD, "aist_opt.json")) as f:
        opt = argparse.Namespace(**json.load(f))
    opt.grid_size = G
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def _digest(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _sample_index(n, k):
    return np.sort(np.random.default_rng(0).choice(n, k, replace=False))       # (tools/make_reference_fixtures.py::sample_index)


def _close(a, r, what):
    a = np.asarray(a, dtype=np.float64); r = np.asarray(r, dtype=np.float64)
    err = float(np.abs(a - r).max()) if a.size else 0.0
    assert err <= TOL * max(1.0, float(np.abs(r).max()) if r.size else 0.0), f"{what}: max abs err {err:.3e}"


def _equal(g, key, t):
    """t is the reference's tensor `key`: same shape and dtype; floating point within TOL, anything else exactly"""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    exact = not np.issubdtype(a.dtype, np.floating)
    if key in g:
        r = g[key]
        assert a.shape == r.shape and a.dtype == r.dtype, (key, a.shape, r.shape, a.dtype, r.dtype)
        if exact:
            assert np.array_equal(a, r), key
        else:
            _close(a, r, key)
        return
    assert tuple(a.shape) == tuple(g[key + "__shape"]) and str(a.dtype) == str(g[key + "__dtype"]), (key, a.shape, a.dtype)
    if exact:
        assert _digest(a) == str(g[key + "__sha256"]), key
        return
    smp = g[key + "__sample"]
    _close(a.reshape(-1)[_sample_index(a.size, smp.size)], smp, key + " (sample)")
    a64 = a.astype(np.float64)
    assert abs(float(a64.sum()) - float(g[key + "__sum"])) <= TOL * max(1.0, float(g[key + "__abssum"])), key + " (sum)"
    assert abs(float(np.abs(a64).sum()) - float(g[key + "__abssum"])) <= TOL * max(1.0, float(g[key + "__abssum"])), key + " (abs sum)"


def _layout(g, key):
    return [(str(n), tuple(int(x) for x in str(s).split(",") if x)) for n, s in zip(g[key + "__names"], g[key + "__shapes"])]


def _same_sd(g, key, sd):
    """a state_dict equals the reference's `key` bit for bit: names in order, shapes, every tensor's bytes"""
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == _layout(g, key)
    bad = [k for k, v, d in zip(sd, sd.values(), g[key + "__sha256"]) if _digest(v) != str(d)]
    assert not bad, bad[:5]


def _forward_matches(g, key, mine, keys):
    for k in keys:
        _equal(g, f"{key}__{k}", mine[k])
    for k, r in zip(LOSS_KEYS, g[f"{key}__losses"]):
        assert abs(float(mine[k]) - float(r)) <= TOL * max(1.0, abs(float(r))), (k, float(mine[k]), float(r))


def _weights_init(m):
    """The reference's weights_init (utils/train_utils.py:248, train.py:262,268), restated: every module whose class name holds
    'Conv' (not 'GraphConv') gets N(0, 0.02) weights and zero bias, 'BatchNorm' N(1, 0.02) weights and zero bias, and inside a
    module whose class name holds 'Block' every Conv3d / ConvTranspose3d gets N(0, 0.001) weights and zero bias.  Pinned by G14:
    applied to the reference's network it gave the state_dict recorded there."""
    name = type(m).__name__
    if "Conv" in name and name != "GraphConv":
        m.weight.data.normal_(0.0, 0.02)
        if m.bias is not None:
            m.bias.data.fill_(0)
    elif "BatchNorm" in name:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)
    elif "Block" in name:
        for mm in m.modules():
            if isinstance(mm, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
                mm.weight.data.normal_(0.0, 0.001)
                mm.bias.data.fill_(0)


def test_state_dict_layout(g14):
    assert _layout(g14, "layout") == [(k, tuple(s)) for k, s in param_spec(HotPathOptions())]


def test_trees_many_seeds(g14):
    rng = np.random.default_rng(7)
    for trial in range(80):
        p = rng.standard_normal((2, 24, 23)) * [0.1, 1.0, 4.0][trial % 3]
        if trial % 5 == 0:
            p = np.round(p * 2) / 2
        aff = O.affinity_v3(torch.from_numpy(p).float())
        A2, order, vals, parents = O.build_tree(aff)
        assert np.array_equal(g14["trees__parents"][trial], parents), trial
        assert np.array_equal(g14["trees__A"][trial], A2), trial
        assert np.array_equal(g14["trees__values"][trial], vals), trial
        assert int(g14["trees__root"][trial]) == int(order[0])


@pytest.mark.parametrize("G", [64, 40])
def test_shell_initialisation_matches_reference(g14, G):
    """train.py:233,262-268 of the reference: ``NeuralMarionette(opt)`` then ``network.apply(weights_init)``.  The shells
    are built from torch layer subclasses in the reference's creation order under the reference's class names, so the
    same seed gives a bit-identical state_dict before AND after the reference's own ``weights_init``, consumes the same
    amount of the RNG stream, and leaves the same requires_grad flags.  Also stand-alone KyptDetector / HSVRNNBVH."""
    import neural_marionette_amd as nm
    from neural_marionette_amd.modules import KyptDetector, HSVRNNBVH
    opt = _opt(G)
    k = f"init{G}"
    torch.manual_seed(7); net = nm.NeuralMarionette(opt); tail = torch.rand(4)
    _same_sd(g14, k + "__seed7", net.state_dict())
    assert torch.equal(tail, torch.from_numpy(g14[k + "__seed7_tail"]))
    assert [n for n, _ in net.named_parameters()] == [str(n) for n in g14[k + "__param_names"]]
    assert [p.requires_grad for _, p in net.named_parameters()] == [bool(b) for b in g14[k + "__requires_grad"]]
    assert not any(bool((v == 0).all()) for kk, v in net.state_dict().items() if kk.endswith("weight"))
    torch.manual_seed(8); net.apply(_weights_init); tail = torch.rand(4)
    _same_sd(g14, k + "__seed8_winit", net.state_dict())
    assert torch.equal(tail, torch.from_numpy(g14[k + "__seed8_tail"]))
    w = net.state_dict()
    assert 5e-4 < float(w["kypt_detector.vox_to_kypt.extract_features.2.res_branch.0.weight"].std()) < 2e-3
    assert 1e-2 < float(w["kypt_detector.kypt_to_vox.decode_voxel_from_combined_representation.4.weight"].std()) < 4e-2
    # the module walk weights_init sees: same class names in the same order
    strip = lambda m: [type(x).__name__ for x in m.modules() if any(True for _ in x.parameters(recurse=False))]
    assert strip(net) == [str(s) for s in g14[k + "__module_walk"]]
    torch.manual_seed(3); b = KyptDetector(opt)
    _same_sd(g14, k + "__detector", b.state_dict())
    assert [p.requires_grad for _, p in b.named_parameters()] == [bool(x) for x in g14[k + "__detector_requires_grad"]]
    torch.manual_seed(3); b = HSVRNNBVH(opt)
    _same_sd(g14, k + "__learner", b.state_dict())
    assert [p.requires_grad for _, p in b.named_parameters()] == [bool(x) for x in g14[k + "__learner_requires_grad"]]


@pytest.mark.parametrize("variant,clip", [("peaky", "figure"), ("default", "bernoulli"), ("winit", "figure")])
def test_full_forward_32(g14, variant, clip):
    G, B, T = 32, 2, 5
    o = HotPathOptions.from_any(_opt(G))
    sd = synth.make_state_dict(o, seed=17, variant=variant)
    vox = synth.figure_clip(B, T, G, seed=2) if clip == "figure" else synth.bernoulli_clip(B, T, G, seed=2)
    eps = synth.make_eps((T, 10, B, 128), seed=3)
    with torch.no_grad():
        mine = O.nm_forward(sd, o, vox, eps)
    key = f"fwd_{variant}_{clip}"
    _forward_matches(g14, key, mine, ("recon", "keypoints", "heatmaps", "affinity", "first_feature", "kypt_recon", "R", "z_kypts", "h_kypts"))
    assert np.array_equal(g14[key + "__parents"], mine["parents"])


@pytest.mark.parametrize("ver", [0, 1, 2])
def test_full_forward_32_other_affinity_versions(g14, ver):
    """options.affinity_ver 0 / 1 / 2 (kypt_detector.py:57-68,173-189; no shipped configuration selects them): (N,K,K) affinity
    parameters, the reference's forward against the oracle's to TOL - layout, affinity, every loss, the tree the VRNN is built on."""
    G, B, T = 32, 2, 5
    o = HotPathOptions.from_any(_opt(G, affinity_ver=ver))
    assert o.affinity_ver == ver
    assert _layout(g14, f"aff{ver}__layout") == [(k, tuple(sh)) for k, sh in param_spec(o)]
    sd = synth.make_state_dict(o, seed=23 + ver, variant="peaky")
    assert tuple(sd["kypt_detector.affinity_params"].shape) == (2, 24, 24)
    vox = synth.figure_clip(B, T, G, seed=2)
    eps = synth.make_eps((T, 10, B, 128), seed=3)
    with torch.no_grad():
        mine = O.nm_forward(sd, o, vox, eps)
    _equal(g14, f"aff{ver}__get_affinity", O.affinity(sd["kypt_detector.affinity_params"], ver))
    _forward_matches(g14, f"aff{ver}", mine, ("recon", "keypoints", "affinity", "kypt_recon", "R", "z_kypts", "h_kypts"))
    assert np.array_equal(g14[f"aff{ver}__parents"], mine["parents"])


@pytest.mark.parametrize("cat", ["max", "sum"])
def test_full_forward_32_other_gaussian_cat_types(g14, cat):
    """options.gaussian_cat_type 'max' / 'sum' (kypt_detector.py:396-401; no shipped configuration selects them): the K Gaussian channels
    of the decoder's combined representation all carry the maximum / the clipped sum over the K maps.  Reference forward against the
    oracle's to TOL, incl. decode_from_dyna (fed the forward's keypoints and first feature, equal to the reference's)."""
    G, B, T = 32, 2, 5
    o = HotPathOptions.from_any(_opt(G, gaussian_cat_type=cat))
    assert o.gaussian_cat_type == cat
    assert _layout(g14, f"cat_{cat}__layout") == [(k, tuple(sh)) for k, sh in param_spec(o)]
    sd = synth.make_state_dict(o, seed=31, variant="peaky")
    vox = synth.figure_clip(B, T, G, seed=2)
    eps = synth.make_eps((T, 10, B, 128), seed=3)
    with torch.no_grad():
        mine = O.nm_forward(sd, o, vox, eps)
    _forward_matches(g14, f"cat_{cat}", mine, ("recon", "keypoints", "first_feature", "kypt_recon", "R", "z_kypts", "h_kypts"))
    with torch.no_grad():
        mine_gen = O.decode_from_keypoints(sd, o, mine["keypoints"][:, 1:4], mine["first_feature"], vox[:, 0])
    _equal(g14, f"cat_{cat}__gen", mine_gen)


def test_full_forward_32_vol_fit_gaussian(g14):
    """options.vol_fit_type 'gaussian' (kypt_detector_utils.py:154-169; no shipped configuration selects it).  The reference's form
    reads a keypoint's third coordinate as the Gaussian's intensity and broadcasts the (B,1,G,G) mask across the batch
    (oracle.nm_oracle.loss_volume_gaussian spells it out): restated as it computes (to TOL), for B = 1, 2, 3 on the loss alone and
    through the full forward."""
    gen = torch.Generator().manual_seed(5)
    for B in (1, 2, 3):
        seq = (torch.rand(B, 3, 1, 16, 16, 16, generator=gen) < 0.1).float()
        kp = torch.rand(B, 3, 7, 4, generator=gen) * 2 - 1
        _equal(g14, f"volg__loss_B{B}", O.loss_volume_gaussian(seq, kp, 1.5))
    G, B, T = 32, 2, 5
    o = HotPathOptions.from_any(_opt(G, vol_fit_type="gaussian"))
    sd = synth.make_state_dict(o, seed=37, variant="peaky")
    vox = synth.figure_clip(B, T, G, seed=2)
    eps = synth.make_eps((T, 10, B, 128), seed=3)
    with torch.no_grad():
        mine = O.nm_forward(sd, o, vox, eps)
    _forward_matches(g14, "volg", mine, ())
    assert float(mine["vol_fit_reg"]) > 0


def test_full_forward_32_learnable_sigmas(g14):
    """options.fixed_sigma = 0 (kypt_detector.py:258-260, 303-306; no shipped configuration selects it): a (K,) parameter
    `vox_to_kypt.sigmas`, created before the sub-modules, sigmas = sigmoid(parameter) * 2 gaussian_sigma per keypoint in the detector's
    Gaussian maps (decode_from_dyna keeps the fixed list, :226).  Layout, the seeded construction's RNG stream, forward to TOL."""
    import neural_marionette_amd as nm
    G, B, T = 32, 2, 5
    opt = _opt(G, fixed_sigma=0)
    o = HotPathOptions.from_any(opt)
    assert o.fixed_sigma == 0
    torch.manual_seed(11); mine_net = nm.NeuralMarionette(opt); tail_mine = torch.rand(3)
    ref_layout = _layout(g14, "sig__seed11")
    assert ref_layout == [(k, tuple(sh)) for k, sh in param_spec(o)]
    assert ref_layout[1] == ("kypt_detector.vox_to_kypt.sigmas", (24,))
    _same_sd(g14, "sig__seed11", mine_net.state_dict())
    assert torch.equal(tail_mine, torch.from_numpy(g14["sig__seed11_tail"]))
    sd = synth.make_state_dict(o, seed=41, variant="peaky")
    sd["kypt_detector.vox_to_kypt.sigmas"] = torch.randn(24, generator=torch.Generator().manual_seed(42))
    vox = synth.figure_clip(B, T, G, seed=2)
    eps = synth.make_eps((T, 10, B, 128), seed=3)
    with torch.no_grad():
        mine = O.nm_forward(sd, o, vox, eps)
    _forward_matches(g14, "sig", mine, ("recon", "keypoints", "first_feature", "kypt_recon", "R", "z_kypts", "h_kypts"))
    with torch.no_grad():
        mine_gen = O.decode_from_keypoints(sd, o, mine["keypoints"][:, 1:3], mine["first_feature"], vox[:, 0])
    _equal(g14, "sig__gen", mine_gen)


def test_input_path_restatement_matches_reference(g14):
    """synth.episodic_normalization / voxelize (the restated input path) against
    utils/dataset_utils.py of the reference: identical floats and identical occupancy grids."""
    rng = np.random.default_rng(4)
    for i, (G, scale) in enumerate(((64, 1.0), (64, 0.9), (96, 1.0))):
        pts = synth.figure_points(4, 4000, rng)
        b = synth.episodic_normalization(pts, scale=scale)
        _equal(g14, f"input{i}__normalized", b)
        for t in range(4):
            _equal(g14, f"input{i}__vox{t}", synth.voxelize(b[t], G))


def test_generation_driver_matches_reference_modules(g14):
    """oracle.sample_generation against the rollout of vis_generation.py:81-136 re-run on the REFERENCE's own
    sub-modules (the script itself imports open3d/cv2 and cannot be imported there)."""
    G, Tc, Tg, S = 32, 4, 5, 3
    o = HotPathOptions.from_any(_opt(G))
    sd = synth.make_state_dict(o, seed=23, variant="peaky")
    vox = synth.figure_clip(1, Tc, G, seed=3)[0]
    e_post, e_prior = synth.make_eps((Tc, S, 128), 5), synth.make_eps((Tg, S, 128), 6)
    with torch.no_grad():
        mine = O.sample_generation(sd, o, vox, Tg, S, e_post, e_prior)
    _equal(g14, "gen__keypoints_gen", mine["keypoints_gen"])
    _equal(g14, "gen__keypoints_cond", mine["keypoints_cond"])
    _equal(g14, "gen__voxels0", mine["voxels_raw"][0])


def test_interpolation_driver_matches_reference_modules(g14):
    """oracle.sample_interpolation against the loop of vis_interpolation.py:80-143 on the reference's sub-modules."""
    G, T, S, rate = 32, 7, 24, 3
    o = HotPathOptions.from_any(_opt(G))
    sd = synth.make_state_dict(o, seed=29, variant="peaky")
    vox = synth.figure_clip(1, T, G, seed=8)[0]
    ea, eb = synth.make_eps((T, S, 128), 9), synth.make_eps((T, S, 128), 10)
    with torch.no_grad():
        mine = O.sample_interpolation(sd, o, vox, rate, S, ea, eb)
    _equal(g14, "interp__keypoints", mine["keypoints"])


def test_eval_metrics_restatement_matches_reference(g14):
    """oracle.voxel_chamfer_distance / semantic_votes vs utils/eval_utils.py (the fixture g7 pins the same numbers)."""
    vox, recon, kp, gt = synth.eval_inputs(seed=11, B=1, T=2, G=24, K=24, Kg=9)
    pf = O.voxel_chamfer_distance(vox, recon)
    assert abs(pf.mean().item() - float(g14["eval__chamfer_log"])) <= 1e-15
    closest, counts = O.semantic_votes(kp, gt)
    assert np.array_equal(counts.numpy(), g14["eval__semantic_scores"])
    assert O.semantic_log(counts) == g14["eval__semantic_log"][()]


# ---- keypoint counts of the reference's other dataset configs (dataset/config.py:97 panda K = 12, :124 hanco K = 28 with
# gaussian_sigma = 1.0; train.py:60 default 22): the shells construct, the state_dict layout is the reference's, and the oracle stays
# bit-identical to the reference there - so the GPU parity tests of tests/test_keypoint_counts_gpu.py are pinned for those K too.
def _opt_k(G, K, sigma=None):
    return _opt(G, nkeypoints=K, **({} if sigma is None else dict(gaussian_sigma=sigma)))


@pytest.mark.parametrize("K", [12, 22, 28])
def test_state_dict_layout_other_keypoint_counts(g14, K):
    import neural_marionette_amd as nm
    opt = _opt_k(64, K)
    torch.manual_seed(5); net = nm.NeuralMarionette(opt)
    sb = net.state_dict()
    _same_sd(g14, f"K{K}__seed5", sb)
    assert _layout(g14, f"K{K}__seed5") == [(k, tuple(s)) for k, s in param_spec(HotPathOptions(nkeypoints=K))]
    assert tuple(sb["kypt_detector.affinity_params"].shape) == (2, K, K - 1)
    assert tuple(sb["kypt_detector.kypt_to_vox.adjust_combined_representation.0.weight"].shape) == (128, 128 + 2 * K + 3, 1, 1, 1)
    assert tuple(sb["dyna_module.joint_matrix_decoder.2.weight"].shape) == (6 * K, 128)


@pytest.mark.parametrize("K,sigma", [(12, None), (22, None), (28, 1.0)])
def test_full_forward_32_other_keypoint_counts(g14, K, sigma):
    G, B, T = 32, 2, 4
    o = HotPathOptions.from_any(_opt_k(G, K, sigma))
    assert o.nkeypoints == K
    sd = synth.make_state_dict(o, seed=40 + K, variant="peaky")
    gen = torch.Generator().manual_seed(K)
    sd["kypt_detector.affinity_params"] = torch.randn(sd["kypt_detector.affinity_params"].shape, generator=gen)
    vox = synth.figure_clip(B, T, G, seed=2)
    eps = synth.make_eps((T, 10, B, 128), seed=3)
    with torch.no_grad():
        mine = O.nm_forward(sd, o, vox, eps)
    _forward_matches(g14, f"fwdK{K}", mine, ("recon", "keypoints", "heatmaps", "affinity", "first_feature", "kypt_recon", "R", "z_kypts", "h_kypts"))
    assert np.array_equal(g14[f"fwdK{K}__parents"], mine["parents"])
