"""The graph-loss options of KyptDetector on the HIP path (model/kypt_detector.py:20-30,54-68,112-143, utils/kypt_detector_utils.py:172-265):
keypoints_detach, using_local_const / using_time_const / using_sparsity_const, graph_loss_ver 0 / 2 and keypoints_graph 'none'.

The yardstick is an fp64 composite: oracle.nm_oracle.detector_forward for every term outside the graph losses (it does not vary with these
options) plus tests/graph_loss_ref.py - pinned to the reference's own functions by fixture G15 - on the oracle's keypoints and affinity.
Weights variant 'tracking' (the keypoints follow the figure, fixture G12): the trajectory term is well conditioned.  Tolerances as in
tests/test_option_branches_gpu.py: losses 2e-5, gradients 2e-3 of each tensor's largest entry."""
import pytest
import torch

import graph_loss_ref as R
from neural_marionette_amd import HotPathOptions, NeuralMarionette, _lib, param_spec, synth
from neural_marionette_amd.spec import DETECTOR_LOSS_KEYS
from neural_marionette_amd.train import DETECTOR_LOSS_WEIGHTS as AIST
from oracle import nm_oracle as O

pytestmark = pytest.mark.gpu
DET = {"detector": True, "learner": False}
SEED = 1500

VARIANTS = {
    "detach": dict(keypoints_detach=1),
    "local_off": dict(using_local_const=0),
    "time_off": dict(using_time_const=0),
    "sparsity_off": dict(using_sparsity_const=0),
    "all_off": dict(using_local_const=0, using_time_const=0, using_sparsity_const=0),
    "ver0": dict(graph_loss_ver=0),
    "ver2": dict(graph_loss_ver=2),
    "ver2_detach": dict(graph_loss_ver=2, keypoints_detach=1),
    "none": dict(keypoints_graph="none"),
}
OFF = {"local_off": ("local_const_loss",), "time_off": ("time_const_loss",), "sparsity_off": ("sparsity_const_loss",),
       "all_off": ("local_const_loss", "time_const_loss", "sparsity_const_loss"),
       "none": ("local_const_loss", "time_const_loss", "sparsity_const_loss", "graph_traj_loss")}
_CACHE = {}


def _opts(variant, **extra):
    return HotPathOptions(grid_size=32, **VARIANTS.get(variant, {}), **extra)


def _weights(o):
    """the 'tracking' weights of the default layout, restricted to o's layout ('none': without affinity_params)"""
    sd = synth.make_state_dict(HotPathOptions(grid_size=32), seed=SEED, variant="tracking")
    keep = {k for k, _ in param_spec(o)}
    return {k: v for k, v in sd.items() if k in keep}


def _oracle(B, T):
    """fp64 oracle forward with every kypt_detector tensor a leaf; graph terms left out (composed per variant)"""
    key = (B, T)
    if key not in _CACHE:
        sd = synth.make_state_dict(HotPathOptions(grid_size=32), seed=SEED, variant="tracking")
        vox = synth.figure_clip(B, T, 32, seed=SEED + 2)
        sd64 = {k: v.double() for k, v in sd.items()}
        names = [k for k in sd64 if k.startswith("kypt_detector.")]
        leaf = {k: sd64[k].clone().requires_grad_(True) for k in names}
        sd64.update(leaf)
        ro = O.detector_forward(sd64, HotPathOptions(grid_size=32), vox.double(), affinity_on=False)
        aff = O.affinity(leaf["kypt_detector.affinity_params"], 3)
        _CACHE[key] = (vox, leaf, ro, aff)
    return _CACHE[key]


def _composite(o, ro, aff):
    out = {k: ro[k] for k in DETECTOR_LOSS_KEYS}
    out.update(R.graph_terms(ro["keypoints"], None if o.keypoints_graph == "none" else aff, o))
    return out


def _net(o, train=False):
    net = NeuralMarionette(o)
    net.load_state_dict(_weights(o))
    net = net.cuda()
    net = net.train() if train else net.eval()
    net.anneal(1)
    return net


def _hip_grads(o, vox):
    net = _net(o, train=True)
    net.control_active(DET)
    net.zero_grad()
    out = net(vox.cuda(), DET)
    loss = sum(w * out[k] for k, w in AIST.items())
    loss.backward()
    torch.cuda.synchronize()
    return net, out, float(loss), {"kypt_detector." + n: p.grad for n, p in net.kypt_detector.named_parameters()}


@pytest.mark.parametrize("path", ["train_fwd", "inference"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_graph_options_forward_parity(variant, path):
    o = _opts(variant)
    vox, _, ro, aff = _oracle(2, 4)
    with torch.no_grad():
        ref = {k: float(v.detach()) for k, v in _composite(o, ro, aff).items()}
    net = _net(o, train=path == "train_fwd")
    net.control_active(DET)
    if path == "inference":
        with torch.no_grad():
            out = net(vox.cuda(), DET)
    else:
        out = net(vox.cuda(), DET)
    torch.cuda.synchronize()
    bad = []
    for k in DETECTOR_LOSS_KEYS:
        g = float(out[k].detach())
        if abs(g - ref[k]) > 2e-5 * max(1.0, abs(ref[k])):
            bad.append((k, g, ref[k]))
    assert not bad, bad
    for k in OFF.get(variant, ()):
        assert float(out[k].detach()) == 0.0, k
    if variant in ("ver0", "ver2"):          # the option changes the numbers for real
        plain = {k: float(v.detach()) for k, v in _composite(HotPathOptions(grid_size=32), ro, aff).items()}
        assert abs(ref["local_const_loss"] - plain["local_const_loss"]) > 1e-3 * abs(plain["local_const_loss"])
    if variant == "none":
        assert out["affinity"] is None


def _grad_parity(o):
    vox, leaf, ro, aff = _oracle(1, 4)
    comp = _composite(o, ro, aff)
    ref_loss = sum(w * comp[k] for k, w in AIST.items())
    names = [k for k in leaf if o.keypoints_graph != "none" or not k.endswith("affinity_params")]
    grads = torch.autograd.grad(ref_loss, [leaf[k] for k in names], retain_graph=True, allow_unused=True)
    ref = {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(names, grads)}
    net, out, loss, got = _hip_grads(o, vox)
    assert abs(loss - float(ref_loss)) <= 2e-5 * max(1.0, abs(float(ref_loss))), (loss, float(ref_loss))
    assert sorted(got) == sorted(ref)
    gmax = max(r.abs().max().item() for r in ref.values())
    bad = []
    for k, r in ref.items():
        g = got[k]
        assert g is not None and tuple(g.shape) == tuple(r.shape) and torch.isfinite(g).all(), k
        e = (g.cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-6 * gmax, 1e-30)
        if e >= 2e-3:
            bad.append((k, e))
    assert not bad, bad[:8]
    return got, ref


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_graph_options_gradient_parity(variant):
    o = _opts(variant)
    got, ref = _grad_parity(o)
    if variant == "all_off":                 # the trajectory term alone still reaches the affinity
        ga = got["kypt_detector.affinity_params"].cpu().double()
        ra = ref["kypt_detector.affinity_params"]
        assert (ga - ra).abs().max() <= 2e-3 * ra.abs().max()


def test_detach_changes_keypoint_gradients():
    """keypoints_detach = 1: the graph terms' gradients still reach affinity_params but no longer the keypoint side; the test can tell
    the two cases apart (the keypoint-side gradients differ between them by far more than the tolerance)."""
    g_on, _ = _grad_parity(_opts("default"))
    g_det, _ = _grad_parity(_opts("detach"))
    k = "kypt_detector.vox_to_kypt.extract_heatmaps_from_features.0.weight"
    a, b = g_on[k].cpu().double(), g_det[k].cpu().double()
    rel = (a - b).abs().max().item() / a.abs().max().item()
    print("detach: heat-map head gradient changes by %.2e of its largest entry" % rel)
    assert rel > 5e-3
    ka = "kypt_detector.affinity_params"
    assert (g_on[ka] - g_det[ka]).abs().max().item() <= 1e-6 * g_on[ka].abs().max().item() + 1e-12


def test_none_graph_detector_and_learner():
    """keypoints_graph 'none': no affinity_params anywhere, affinity None, no affinity gradient, the learner paths refuse."""
    o = _opts("none")
    vox, _, _, _ = _oracle(2, 4)
    net = _net(o)
    assert "kypt_detector.affinity_params" not in net.state_dict()
    with torch.no_grad():
        out = net(vox.cuda(), DET)
    assert out["affinity"] is None
    got, _ = _grad_parity(o)
    assert not any(k.endswith("affinity_params") for k in got)
    with pytest.raises(_lib.NmError, match="none"):
        net(vox.cuda(), {"detector": True, "learner": True})
    with pytest.raises(_lib.NmError, match="none"):
        net.kypt_detector.get_affinity()
    kp = torch.rand(1, 4, 24, 4, device="cuda")
    with pytest.raises(_lib.NmError, match="none"):
        net.dyna_module.encode(kp, None)
    with pytest.raises(_lib.NmError, match="none"):
        net.generate(vox[:1].cuda(), {"detector": True, "learner": True})
    with pytest.raises(_lib.NmError, match="none"):
        net.sample_generation(vox[0].cuda(), Tgen=2, sample_num=2)


def test_detector_training_ver0_follows_composite_adam():
    """Three DetectorTrainer steps (Adam lr 4e-4, AIST weights) with graph_loss_ver 0 against torch.optim.Adam on the fp64 composite."""
    from neural_marionette_amd.train import DetectorTrainer
    o = _opts("ver0")
    B, T = 1, 4
    sd = _weights(o)
    vox = synth.figure_clip(B, T, 32, seed=SEED + 2)
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("kypt_detector.")}
    opt = torch.optim.Adam(list(leaf.values()), lr=4e-4)
    ref_losses = []
    for _ in range(3):
        sd64 = {k: v.double() for k, v in sd.items()}
        sd64.update(leaf)
        ro = O.detector_forward(sd64, HotPathOptions(grid_size=32), vox.double(), affinity_on=False)
        comp = _composite(o, ro, O.affinity(leaf["kypt_detector.affinity_params"], 3))
        loss = sum(w * comp[k] for k, w in AIST.items())
        ref_losses.append(float(loss))
        opt.zero_grad()
        loss.backward()
        opt.step()
    net = _net(o, train=True)
    tr = DetectorTrainer(net, lr=4e-4)
    losses = [tr.step(vox.cuda())["loss"] for _ in range(3)]
    torch.cuda.synchronize()
    print("ver 0 training losses", losses, "composite", ref_losses)
    assert abs(losses[0] - ref_losses[0]) <= 2e-5 * abs(ref_losses[0])
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 2e-4 * abs(b), (losses, ref_losses)
    num = den = 0.0
    for n, p in net.kypt_detector.named_parameters():
        f = p.detach().reshape(-1).double().cpu()[::97]
        r = leaf["kypt_detector." + n].detach().reshape(-1)[::97]
        num += float((f - r).abs().sum()); den += r.numel()
    print("mean weight difference after 3 steps %.2e over %d sampled entries" % (num / den, den))
    assert num / den < 2e-5


@pytest.mark.parametrize("field,value", [("nneighbor", 3), ("sep_sigma", 0.05), ("graph_traj_weight", 0.0),
                                         ("nlatent_kypt", 64), ("nhidden_kypt", 256)])
def test_other_option_values_forward_parity(field, value):
    """Option values the library honours that no other test set: the full forward (detector + VRNN encode) against the oracle."""
    o = HotPathOptions(grid_size=32, **{field: value})
    sd = synth.make_state_dict(o, seed=SEED + 7, variant="tracking")
    vox = synth.figure_clip(1, 3, 32, seed=SEED + 8)
    eps = synth.make_eps((3, 10, 1, o.nlatent_kypt), seed=SEED + 9)
    with torch.no_grad():
        ref = O.nm_forward(sd, o, vox, eps)
    net = NeuralMarionette(o)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    net.anneal(1)
    with torch.no_grad():
        out = net(vox.cuda(), {"detector": True, "learner": True}, eps=eps.cuda())
    torch.cuda.synchronize()
    for k in DETECTOR_LOSS_KEYS:
        g, r = float(out[k]), float(ref[k])
        assert abs(g - r) <= 2e-5 * max(1.0, abs(r)), (k, g, r)
    for k in ("keypoints", "z_kypts", "h_kypts"):
        e = (out[k].cpu().double() - ref[k].double()).abs().max().item()
        assert e < 1e-4, (k, e)
