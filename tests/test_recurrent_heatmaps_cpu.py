"""options.const_intensity = 2 (heat-maps propagated from frame to frame, kypt_detector.py:308-347) without a GPU.

tests/recurrent_heatmap_ref.py is pinned to the reference through fixture G17 (tests/golden/g17_recurrent32.npz, written by
tools/make_recurrent_fixture.py, which also asserts bit equality side by side): floating-point results to TOL relative to the tensor's
scale - the CPU kernels' rounding differs between CPU models, as in tests/test_oracle_vs_reference.py - discrete results exactly, the
float64 gradients to 1e-6 (see the test).  Then the host side of the switch: the option check, the state_dict (the same 337 tensors and the same seeded
construction as const_intensity = 3), the exported entry point, and how far apart the two options are on the fixture's weights."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import golden_npz
import recurrent_heatmap_ref as RR
from neural_marionette_amd import _lib, NeuralMarionette, HotPathOptions, param_spec, synth
from neural_marionette_amd.spec import DETECTOR_LOSS_KEYS
from neural_marionette_amd.train import DETECTOR_LOSS_WEIGHTS as AIST

LOSS_KEYS = DETECTOR_LOSS_KEYS + ("kl_kypt", "kypt_recon_loss")
TOL = 2e-5


@pytest.fixture(scope="module")
def g17(golden_dir):
    g = golden_npz.load(os.path.join(golden_dir, "g17_recurrent32.npz"))
    old = torch.get_num_threads()
    torch.set_num_threads(int(g["threads"]))
    yield g
    torch.set_num_threads(old)


def _close(a, r, what):
    a = np.asarray(a, dtype=np.float64); r = np.asarray(r, dtype=np.float64)
    assert a.shape == r.shape, (what, a.shape, r.shape)
    err = float(np.abs(a - r).max())
    assert err <= TOL * max(1.0, float(np.abs(r).max())), f"{what}: max abs err {err:.3e}"


def test_restatement_matches_the_reference_forward(g17):
    B, T, G = (int(v) for v in g17["fwd__shape"])
    seed = int(g17["fwd__seed"])
    o = HotPathOptions(grid_size=G, const_intensity=2)
    sd = synth.make_state_dict(o, seed=seed, variant="peaky")
    vox = synth.figure_clip(B, T, G, seed=seed + 2)
    eps = synth.make_eps((T, 10, B, o.nlatent_kypt), seed=seed + 3)
    with torch.no_grad():
        out = RR.nm_forward(sd, o, vox, eps)
    for k in ("keypoints", "affinity", "kypt_recon", "z_kypts", "h_kypts", "R"):
        _close(out[k].numpy(), g17["fwd__" + k], k)
    hm = out["heatmaps"]
    _close(hm[..., 1::4, 1::4, 1::4].numpy(), g17["fwd__heatmaps_strided"], "heatmaps (strided)")
    sums = g17["fwd__heatmaps_sums"]
    assert float(np.abs(hm.double().sum(dim=(3, 4, 5)).numpy() - sums).max()) <= TOL * float(np.abs(sums).max())
    ff = out["first_feature"].double()
    assert abs(float(ff.sum()) - float(g17["fwd__first_feature_sum"])) <= TOL * float(g17["fwd__first_feature_abssum"])
    assert abs(float(ff.abs().sum()) - float(g17["fwd__first_feature_abssum"])) <= TOL * float(g17["fwd__first_feature_abssum"])
    for k, r in zip(LOSS_KEYS, g17["fwd__losses"]):
        assert abs(float(out[k]) - float(r)) <= TOL * max(1.0, abs(float(r))), (k, float(out[k]), float(r))
    assert np.array_equal(out["best_idx"].numpy().astype(np.int32), g17["fwd__best_idx"])
    assert np.array_equal(out["parents"], g17["fwd__parents"])
    assert int(out["order"][0]) == int(g17["fwd__order"][0]) and sorted(out["order"].tolist()) == sorted(g17["fwd__order"].tolist())


@pytest.mark.parametrize("seed", [431, 432])
def test_restatement_matches_the_reference_gradients(g17, seed):
    """float64 autograd of the restatement against float64 autograd of the reference's module.  Both sides carry constants made in float32
    (the coordinate ramps of torch.linspace, the 1e-6 guards) into slightly different float64 expressions, so the two evaluations agree to
    ~1e-10 in the loss and, through the conditioning of the small spatio-temporal gradients, to ~1e-8 ... 1e-7 of a tensor's largest entry
    - not to float64 rounding.  The bound is 1e-6: three orders below the 2e-3 the GPU path is held to against this restatement."""
    assert seed in g17["grad__seeds"].tolist()
    o = HotPathOptions(grid_size=32, const_intensity=2)
    sd = {k: v.double() for k, v in synth.make_state_dict(o, seed=seed, variant="peaky").items()}
    vox = synth.figure_clip(1, 4, 32, seed=seed + 2).double()
    keys = [str(k) for k in g17["grad__keys"]]
    leaf = {k: sd[k].clone().requires_grad_(True) for k in keys}
    sd.update(leaf)
    ro = RR.detector_forward(sd, o, vox, affinity_on=True)
    loss = sum(w * ro[k] for k, w in AIST.items())
    grads = torch.autograd.grad(loss, [leaf[k] for k in keys])
    r = float(g17[f"grad{seed}__loss"])
    assert abs(float(loss.detach()) - r) <= 1e-9 * abs(r)
    for k, gr in zip(keys, grads):
        ref = g17[f"grad{seed}__{k}"]
        assert ref.shape == tuple(gr.shape) and np.abs(ref).max() > 0, k
        e = float(np.abs(gr.numpy() - ref).max()) / float(np.abs(ref).max())
        assert e <= 1e-6, (k, e)


def test_the_two_options_are_far_apart_on_these_weights(g17):
    """Frame 0 is the same computation under both options (difference exactly 0 in the reference); from frame 1 on the keypoints of
    const_intensity 2 and 3 differ by at least 0.1 in every clip - a library that ignored the switch would miss the 1e-4 parity of the GPU
    tests by three orders of magnitude.  (The 'winit' weights would not do: their propagate weights ~N(0, 0.02) leave 1.8e-4.)"""
    d = np.abs(g17["fwd__keypoints"].astype(np.float64) - g17["fwd__keypoints_ci3"]).max(axis=(2, 3))         # (B, T)
    print("const_intensity 2 against 3, largest keypoint difference per frame:", np.round(d, 3).tolist())
    assert (d[:, 0] == 0.0).all()
    assert (d[:, 1:] >= 0.1).all(), d.min(axis=0)


def test_option_check_accepts_two_and_three_only():
    HotPathOptions(const_intensity=2).check_fast_path()
    HotPathOptions(const_intensity=3).check_fast_path()
    for v in (0, 1, 4):
        with pytest.raises(NotImplementedError, match="const_intensity must be 2 or 3"):
            HotPathOptions(const_intensity=v).check_fast_path()
        with pytest.raises(NotImplementedError):
            NeuralMarionette(HotPathOptions(grid_size=32, const_intensity=v))


def test_state_dict_and_seeded_construction_equal_those_of_value_three(g17):
    o2, o3 = HotPathOptions(grid_size=32, const_intensity=2), HotPathOptions(grid_size=32, const_intensity=3)
    assert param_spec(o2) == param_spec(o3) and len(param_spec(o2)) == 337
    torch.manual_seed(9); sd2 = NeuralMarionette(o2).state_dict(); tail2 = torch.rand(3)
    torch.manual_seed(9); sd3 = NeuralMarionette(o3).state_dict(); tail3 = torch.rand(3)
    assert list(sd2) == list(sd3) == [k for k, _ in param_spec(o2)] and torch.equal(tail2, tail3)
    assert all(torch.equal(sd2[k], sd3[k]) for k in sd2)
    # ... and those of the reference's module, for both values
    digests = [hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() for v in sd2.values()]
    for ci in (2, 3):
        assert [str(n) for n in g17[f"init__names{ci}"]] == list(sd2)
        assert [str(s) for s in g17[f"init__sha256_{ci}"]] == digests


def test_entry_point_is_exported_and_judges_the_value_without_a_device():
    lib = _lib.load()
    assert "nm_ctx_set_const_intensity" in _lib.SIGNATURES
    for v in (0, 1, 4, -1, 5):
        assert lib.nm_ctx_set_const_intensity(C.c_void_p(), v) == _lib.NM_ERR_UNSUPPORTED, v
        assert b"const_intensity" in lib.nm_last_error()
    for v in (2, 3):                                           # a supported value then needs a context
        assert lib.nm_ctx_set_const_intensity(C.c_void_p(), v) == _lib.NM_ERR_ARG
        assert b"null context" in lib.nm_last_error()
