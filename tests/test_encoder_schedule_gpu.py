"""Encoder schedule of the inference forward (nm_net.hip hourglass(), NM355_ENC_SCHED / NM355_ENC_S1 / NM355_ENC_S1_WGS): the per-frame
net's hourglass skip branch s1 runs on the third stream beside the interior's launch chain, its persistent convs on a capped grid.

Stream placement and grid size enter no kernel's arithmetic (GroupNorm partials are per brick and summed in fixed order), so every
output must be BIT-IDENTICAL to the serial schedule (NM355_ENC_SCHED=0, the parent's): a difference is a kernel whose result depends
on its grid, or a scratch race between the branch and the main stream.  The training forward and backward do not take the new path at
all: same launches on the same streams."""
import ctypes as C

import pytest
import torch

from test_network_gpu import ACTS, _net, _switches
from neural_marionette_amd import HotPathOptions, synth, _lib

pytestmark = pytest.mark.gpu

SERIAL = {"NM355_ENC_SCHED": "0"}
NEW = {"NM355_ENC_SCHED": "1", "NM355_ENC_S1": "1"}      # pinned: the arm under test must not depend on what the environment exports
_CASES = {}


def _case(G, B, T):
    """options, weights and inputs of one shape, and the serial schedule's outputs (computed once, shared, never modified)"""
    key = (G, B, T)
    if key not in _CASES:
        o = HotPathOptions(grid_size=G)
        sd = synth.make_state_dict(o, seed=8, variant="peaky")
        vox = synth.figure_clip(B, T, G, seed=10).cuda()
        eps = synth.make_eps((T, 10, B, o.nlatent_kypt), seed=9).cuda()
        with _switches(SERIAL):
            ref = _forward(_net(o, sd), vox, eps)
        _CASES[key] = (o, sd, vox, eps, ref)
    return _CASES[key]


def _forward(net, vox, eps):
    with torch.no_grad():
        out = net(vox, ACTS, eps=eps)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


def _equal(a, b):
    """torch.equal on the bit patterns: as strict on every finite value (stricter on signed zeros), and a NaN equals the same NaN -
    at T = 2 graph_traj_loss is NaN under either schedule, which torch.equal on the values would report as a difference"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _same(a, b, what):
    assert set(a) == set(b), what
    assert len(a) >= 5, sorted(a)
    for k in sorted(a):
        assert _equal(a[k], b[k]), "%s: %s differs (max %.3e)" % (what, k, (a[k].double() - b[k].double()).abs().max().item())


def _launches(net, run, mode):
    """profiled conv-family launches during run(): mode 1 the main stream's, mode 2 every stream's"""
    lib, h = net._engine.ctx.lib, net._engine.ctx.handle
    _lib.check(lib.nm_prof_enable(h, mode), "prof_enable")
    run()
    torch.cuda.synchronize()
    _lib.check(lib.nm_prof_enable(h, 0), "prof_enable")
    total = 0
    for v in range(16):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(lib.nm_prof_read(h, v, C.byref(ms), C.byref(fl), C.byref(n)), "prof_read")
        total += n.value
    return total


# 64^3: x0 is 16^3, s1 runs on conv_f16p2 (two frames: 32 bricks); 32^3 and 48^3: the skip branch on the non-persistent kernels, 48^3
# with extents that are no whole bricks; 66 frames: two encoder chunks, a fork and a join each
@pytest.mark.parametrize("G,B,T", [(64, 1, 2), (32, 2, 3), (48, 1, 2), (32, 2, 33)])
def test_new_schedule_is_bit_identical_to_the_serial_one(G, B, T):
    o, sd, vox, eps, ref = _case(G, B, T)
    with _switches(NEW):                               # (the context is created by the first call: it reads the switches then)
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "G=%d B=%d T=%d" % (G, B, T))


def test_capped_grid_smaller_than_the_work_is_bit_identical():
    """cap 8: eight workgroups walk the 32 bricks of s1's convs, four each"""
    o, sd, vox, eps, ref = _case(64, 1, 2)
    with _switches({**NEW, "NM355_ENC_S1_WGS": "8"}):
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "cap 8")


def test_the_skip_branch_leaves_the_main_stream():
    """the new schedule really is one: at 64^3 s1's two convs are launched on another stream (same launches in all)"""
    o, sd, vox, eps, _ = _case(64, 1, 2)
    counts = {}
    for name, env in (("new", NEW), ("serial", SERIAL)):
        with _switches(env):
            net = _net(o, sd)
            _forward(net, vox, eps)
        counts[name] = [_launches(net, lambda: _forward(net, vox, eps), m) for m in (1, 2)]
    print("profiled conv launches [main stream, all streams]:", counts)
    assert counts["new"][1] == counts["serial"][1]
    assert counts["serial"][0] - counts["new"][0] == 2, counts


def test_five_consecutive_forwards_repeat_the_first():
    """a scratch race between the branch and the main stream shows as a mismatch between calls"""
    o, sd, vox, eps, ref = _case(64, 1, 2)
    with _switches(NEW):
        net = _net(o, sd)
        outs = [_forward(net, vox, eps) for _ in range(5)]
    for i, out in enumerate(outs):
        _same(out, ref, "call %d" % i)


def test_keypoints_only_passes_share_the_schedule():
    """nm_detector_keypoints (KyptDetector.detect) and LearnerTrainer(lean=True) run the same encoder"""
    from neural_marionette_amd.train import LearnerTrainer
    o = HotPathOptions(grid_size=64)
    sd = synth.make_state_dict(o, seed=31, variant="peaky")
    B, T = 1, 3
    vox = synth.figure_clip(B, T, 64, seed=12).cuda()
    eps = synth.make_eps((T, 10, B, o.nlatent_kypt), seed=40).cuda()
    res = {}
    for name, env in (("new", NEW), ("serial", SERIAL)):
        with _switches(env):
            net = _net(o, sd)
            det = net.kypt_detector.detect(vox)
            torch.cuda.synchronize()
            det = {k: v.detach().clone() for k, v in det.items() if torch.is_tensor(v)}
            net.train()
            step = LearnerTrainer(net, lr=4e-4, lean=True).step(vox, eps=eps)
            torch.cuda.synchronize()
        res[name] = (det, step, {k: v.detach().cpu().clone() for k, v in net.dyna_module.state_dict().items()})
    for k in ("keypoints", "heatmaps", "affinity", "first_feature"):
        assert _equal(res["new"][0][k], res["serial"][0][k]), k
    assert sorted(res["new"][1]) == sorted(res["serial"][1]) and "loss" in res["new"][1]
    for k, v in res["serial"][1].items():
        assert _equal(torch.tensor(v, dtype=torch.float64), torch.tensor(res["new"][1][k], dtype=torch.float64)), (k, v, res["new"][1][k])
    for k, v in res["serial"][2].items():
        assert _equal(v, res["new"][2][k]), k


def test_training_forward_and_backward_are_untouched():
    """under the new defaults the training step makes the same launches on the same streams as under the serial schedule (profiled
    conv-family launches, main stream / all streams) and computes the same loss and gradients, bit for bit"""
    from neural_marionette_amd.train import DETECTOR_LOSS_WEIGHTS
    o = HotPathOptions(grid_size=32)
    sd = synth.make_state_dict(o, seed=5, variant="peaky")
    B, T = 1, 3
    vox = synth.figure_clip(B, T, 32, seed=6).cuda()
    eps = synth.make_eps((T, 10, B, o.nlatent_kypt), seed=7).cuda()
    res = {}
    for name, env in (("new", NEW), ("serial", SERIAL)):
        with _switches(env):
            net = _net(o, sd)
        state = {}

        def step():
            net.zero_grad()
            out = net(vox, ACTS, eps=eps)
            loss = sum(w * out[k] for k, w in DETECTOR_LOSS_WEIGHTS.items())
            loss.backward()
            state["loss"] = loss.detach().clone()
        with _switches(env):
            step()
        counts = [_launches(net, step, m) for m in (1, 2)]
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        res[name] = (counts, state["loss"], grads)
    print("training step, profiled conv launches [main stream, all streams]:", res["new"][0], res["serial"][0])
    assert res["new"][0] == res["serial"][0]
    assert res["new"][0][0] > 0
    assert _equal(res["new"][1], res["serial"][1])
    assert set(res["new"][2]) == set(res["serial"][2]) and len(res["new"][2]) > 10
    for k, g in res["serial"][2].items():
        assert _equal(g, res["new"][2][k]), k
