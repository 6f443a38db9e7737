"""The graph-loss options of KyptDetector (model/kypt_detector.py:20-30,54-68,112-143) on the CPU side: the fp64 restatement of the two
graph losses (tests/graph_loss_ref.py) against what the reference computed (fixture G15, tools/make_graph_loss_fixtures.py), the option
check, the 'none' layout and the seeded initialisation, and a walk over every HotPathOptions field: each non-default value is rejected at
construction, honoured with a named GPU test, or has no effect in the reference."""
import dataclasses
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import golden_npz
import graph_loss_ref as R
from neural_marionette_amd import HotPathOptions, param_spec
from neural_marionette_amd.modules import KyptDetector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g15(golden_dir):
    return golden_npz.load(os.path.join(golden_dir, "g15_graph_loss_options.npz"))


def _names(a):
    return bytes(np.asarray(a, dtype=np.uint8)).decode().split("\n")


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).digest()


@pytest.mark.parametrize("ver", [0, 1, 2])
def test_helper_equals_reference_values_and_gradients(g15, ver):
    kp0 = torch.from_numpy(g15["keypoints"])
    aff0 = torch.from_numpy(g15["affinity"])
    W = [float(w) for w in g15["weights"]]
    worst = 0.0
    for lo, ti, sp in (tuple(int(x) for x in s) for s in g15["switches"]):
        tag = f"v{ver}_l{lo}t{ti}s{sp}"
        kp = kp0.clone().requires_grad_(True)
        aff = aff0.clone().requires_grad_(True)
        outs = list(R.graph_consistency(kp, aff, ver, bool(lo), bool(ti), bool(sp))) + [R.graph_traj(kp, aff, ver)]
        for name, o in zip(("local", "time", "sparsity", "intensity", "traj"), outs):
            ref = torch.from_numpy(np.asarray(g15[f"{tag}__{name}"]))
            assert tuple(o.shape) == tuple(ref.shape), (tag, name)
            e = (o.detach() - ref).abs().max().item()
            worst = max(worst, e)
            assert e <= 1e-10, (tag, name, e)
        s = sum(w * o.mean() for w, o in zip(W, outs))
        gk, ga = torch.autograd.grad(s, [kp, aff], allow_unused=True)
        gk = gk if gk is not None else torch.zeros_like(kp)
        ga = ga if ga is not None else torch.zeros_like(aff)
        for g, key in ((gk, "dkp"), (ga, "daff")):
            e = (g - torch.from_numpy(g15[f"{tag}__{key}"])).abs().max().item()
            assert e <= 1e-10, (tag, key, e)
        if ver != 1 and (lo or ti):
            assert gk[..., 3].abs().max() > 0, tag            # the intensity receives a gradient under ver 0 / 2
        if ver == 1:
            assert gk[..., 3].abs().max() == 0, tag
        if not sp:
            assert float(outs[2].abs().max()) == 0.0
    print("graph_loss_ver %d: worst value error %.1e" % (ver, worst))


def test_check_fast_path_accepts_graph_options():
    for kw in (dict(graph_loss_ver=0), dict(graph_loss_ver=2), dict(keypoints_graph="none"), dict(keypoints_detach=1),
               dict(using_local_const=0, using_time_const=0, using_sparsity_const=0), dict(graph_loss_ver=2, keypoints_detach=1)):
        HotPathOptions(grid_size=32, **kw).check_fast_path()
    for kw in (dict(graph_loss_ver=3), dict(keypoints_graph="learned")):
        with pytest.raises(NotImplementedError):
            HotPathOptions(grid_size=32, **kw).check_fast_path()


def test_graph_loss_flags():
    assert HotPathOptions().graph_loss_flags() == 0
    o = HotPathOptions(using_local_const=0, using_time_const=0, using_sparsity_const=0, keypoints_detach=1, keypoints_graph="none")
    assert o.graph_loss_flags() == 1 | 2 | 4 | 8 | 16
    hdr = open(os.path.join(ROOT, "include", "nm355.h")).read()
    for name, bit in (("LOCAL_OFF", 1), ("TIME_OFF", 2), ("SPARSITY_OFF", 4), ("DETACH", 8), ("NONE", 16)):
        assert re.search(r"#define NM_GRAPH_%s\s+%d\b" % (name, bit), hdr), name


def test_none_layout_matches_reference(g15):
    """keypoints_graph 'none': no affinity_params, and the seeded construction (which then skips kypt_detector.py:54-68) gives the
    reference's state_dict bit for bit."""
    o = HotPathOptions(grid_size=32, keypoints_graph="none")
    torch.manual_seed(3)
    det = KyptDetector(o)
    sd = det.state_dict()
    names = _names(g15["none__names"])
    assert list(sd) == names
    assert "affinity_params" not in names
    shapes = [tuple(int(x) for x in s if x >= 0) for s in g15["none__shapes"]]
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert [_sha(v) for v in sd.values()] == [bytes(d) for d in g15["none__sha256"]]
    assert ["kypt_detector." + k for k in sd] == [k for k, _ in param_spec(o) if k.startswith("kypt_detector.")]
    det.anneal(5)                                  # nothing to start under 'none'
    assert det.affinity_start is False


@pytest.mark.parametrize("ver", [3, 0])
def test_graph_random_init_matches_reference(g15, ver):
    """graph_random_init = 1 (kypt_detector.py:56-61): affinity_params drawn from randn after the sub-modules, as the reference does."""
    torch.manual_seed(4)
    sd = KyptDetector(HotPathOptions(grid_size=32, graph_random_init=1, affinity_ver=ver)).state_dict()
    assert list(sd) == _names(g15[f"random_init_v{ver}__names"])
    assert [_sha(v) for v in sd.values()] == [bytes(d) for d in g15[f"random_init_v{ver}__sha256"]]


# ---- every HotPathOptions field ---------------------------------------------------------------------------------------------------
NON_DEFAULT = dict(
    grid_size=40, nkeypoints=12, input_dim=2, gaussian_sigma=2.0, fixed_sigma=0, const_intensity=1, affinity_ver=0, nneighbor=3,
    graph_loss_ver=0, gaussian_cat_type="max", vol_fit_type="gaussian", keypoints_graph="none", graph_random_init=1,
    keypoints_detach=1, sep_sigma=0.05, nlatent_kypt=64, nhidden_kypt=256, transition_type="gl", Ttot=30, Tcond=4, is_binarized=0,
    affinity_anneal=5, using_local_const=0, using_time_const=0, using_sparsity_const=0, using_intensity_const=0,
    graph_traj_weight=0.0, graph_vol_weight=1.0, state_mode="cat", action_mode="none",
)
# honoured: the test that holds the library to the reference for that value ("file::test")
HONOURED = dict(
    grid_size="test_network_gpu.py::test_g5_odd_hourglass40",
    nkeypoints="test_keypoint_counts_gpu.py::test_forward_parity_other_keypoint_counts",
    gaussian_sigma="test_keypoint_counts_gpu.py::test_forward_parity_other_keypoint_counts",
    fixed_sigma="test_option_branches_gpu.py::test_forward_parity_learnable_sigmas",
    affinity_ver="test_option_branches_gpu.py::test_forward_parity_affinity_versions",
    nneighbor="test_graph_loss_options_gpu.py::test_other_option_values_forward_parity",
    graph_loss_ver="test_graph_loss_options_gpu.py::test_graph_options_forward_parity",
    gaussian_cat_type="test_option_branches_gpu.py::test_forward_parity_gaussian_cat_types",
    vol_fit_type="test_option_branches_gpu.py::test_forward_parity_vol_fit_gaussian",
    keypoints_graph="test_graph_loss_options_gpu.py::test_none_graph_detector_and_learner",
    graph_random_init="test_graph_loss_options_cpu.py::test_graph_random_init_matches_reference",
    keypoints_detach="test_graph_loss_options_gpu.py::test_detach_changes_keypoint_gradients",
    sep_sigma="test_graph_loss_options_gpu.py::test_other_option_values_forward_parity",
    nlatent_kypt="test_graph_loss_options_gpu.py::test_other_option_values_forward_parity",
    nhidden_kypt="test_graph_loss_options_gpu.py::test_other_option_values_forward_parity",
    Tcond="test_keypoint_counts_gpu.py::test_generate_and_rollout_other_keypoint_counts",
    affinity_anneal="test_train_detector_gpu.py::test_trainer_with_frozen_parameters",
    using_local_const="test_graph_loss_options_gpu.py::test_graph_options_forward_parity",
    using_time_const="test_graph_loss_options_gpu.py::test_graph_options_forward_parity",
    using_sparsity_const="test_graph_loss_options_gpu.py::test_graph_options_gradient_parity",
    graph_traj_weight="test_graph_loss_options_gpu.py::test_other_option_values_forward_parity",
)
# read nowhere on the reference's forward / backward path (reference file:line of the only use)
NO_EFFECT = dict(
    is_binarized="model/kypt_detector.py:34 stores it; nothing reads it",
    Ttot="model/ never reads options.Ttot (generate takes Ttot as an argument, neural_marionette.py:76)",
    state_mode="model/hsvrnn_bvh.py:19 stores it; nothing reads it",
    action_mode="model/hsvrnn_bvh.py:20 stores it; nothing reads it",
    using_intensity_const="utils/kypt_detector_utils.py:223: the intensity loss is zeros(1, 1) whatever the switch",
    graph_vol_weight="model/kypt_detector.py:28 sets using_graph_vol, which nothing reads; graph_vol_loss is zeros (:130, :142)",
)


def _test_exists(ref):
    fn, name = ref.split("::")
    src = open(os.path.join(ROOT, "tests", fn)).read()
    return re.search(r"^def %s\(" % re.escape(name), src, flags=re.M) is not None


def test_every_option_field_is_rejected_honoured_or_inert():
    fields = [f.name for f in dataclasses.fields(HotPathOptions)]
    assert sorted(NON_DEFAULT) == sorted(fields), "a new HotPathOptions field needs an entry here"
    rejected = []
    for name in fields:
        value = NON_DEFAULT[name]
        assert value != getattr(HotPathOptions(), name), name
        try:
            HotPathOptions(**{name: value}).check_fast_path()
            accepted = True
        except NotImplementedError:
            accepted = False
            rejected.append(name)
        n_class = (not accepted) + (name in HONOURED) + (name in NO_EFFECT)
        assert n_class == 1, (name, accepted, name in HONOURED, name in NO_EFFECT)
        if name in HONOURED:
            assert _test_exists(HONOURED[name]), HONOURED[name]
    assert sorted(rejected) == ["const_intensity", "input_dim", "transition_type"]
