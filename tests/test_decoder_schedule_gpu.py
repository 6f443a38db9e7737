"""Decoder schedule of the inference forward (bits 2 and 4 of the mask NM355_ENC_SCHED; nm_net.hip decode_frames / detector_graph): bit 2
the edge kernel of the two fused-upsample layers on the third stream beside their face kernel, bit 4 clip_loss_kernel on the third
stream beside the voxel decoder.  Every value but 0 runs the encoder schedule (tests/test_encoder_schedule_gpu.py), so the value 1 is the
decoder's serial order and the reference here.  (A third part, an adjust_gauss kernel that keeps its weights over several slabs, was built, measured and
removed - DESIGN 5; the shapes chosen for it stay as cases of the schedule.)

Neither enters any value's arithmetic: the face and edge items own disjoint cells and disjoint GroupNorm partial slots, and a stream
is no operand.  So every output must be BIT-IDENTICAL to NM355_ENC_SCHED=1 (the decoder's serial order): a difference is a store race between
face and edge items, a scratch race between the streams or a missing join.  The training forward and backward do not take the new
path."""
import ctypes as C

import pytest
import torch

from test_network_gpu import ACTS, _net, _switches
from neural_marionette_amd import HotPathOptions, synth, _lib

pytestmark = pytest.mark.gpu

SERIAL = {"NM355_ENC_SCHED": "1", "NM355_ENC_S1": "1"}
NEW = {"NM355_ENC_SCHED": "7", "NM355_ENC_S1": "1"}          # pinned: the arm under test must not depend on what the environment exports
_CASES = {}


def _case(G, B, T, mode="split16", **opts):
    """options, weights and inputs of one configuration, and the serial arm's outputs (computed once, shared, never modified)"""
    key = (G, B, T, mode, tuple(sorted(opts.items())))
    if key not in _CASES:
        o = HotPathOptions(grid_size=G, **opts)
        sd = synth.make_state_dict(o, seed=8, variant="peaky")
        vox = synth.figure_clip(B, T, G, seed=10).cuda()
        eps = synth.make_eps((T, 10, B, o.nlatent_kypt), seed=9).cuda()
        with _switches(SERIAL):
            ref = _forward(_net(o, sd, mode), vox, eps)
        _CASES[key] = (o, sd, vox, eps, ref)
    return _CASES[key]


def _forward(net, vox, eps):
    with torch.no_grad():
        out = net(vox, ACTS, eps=eps)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}


def _equal(a, b):
    """torch.equal on the bit patterns: as strict on every finite value (stricter on signed zeros), and a NaN equals the same NaN -
    at T = 2 graph_traj_loss is NaN under either arm, which torch.equal on the values would report as a difference"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _same(a, b, what):
    assert set(a) == set(b), what
    assert len(a) >= 5, sorted(a)
    for k in sorted(a):
        assert _equal(a[k], b[k]), "%s: %s differs (max %.3e)" % (what, k, (a[k].double() - b[k].double()).abs().max().item())


def _launches(net, run, mode):
    """profiled conv-family launches during run(), per family: mode 1 the main stream's, mode 2 every stream's"""
    lib, h = net._engine.ctx.lib, net._engine.ctx.handle
    _lib.check(lib.nm_prof_enable(h, mode), "prof_enable")
    run()
    torch.cuda.synchronize()
    _lib.check(lib.nm_prof_enable(h, 0), "prof_enable")
    counts = []
    for v in range(16):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(lib.nm_prof_read(h, v, C.byref(ms), C.byref(fl), C.byref(n)), "prof_read")
        counts.append(n.value)
    return counts


# 64^3: both up layers on conv_up2y + face_r + edge; 32^3: coarse 8^3 and 16^3; 48^3: coarse 12, no whole bricks - the first up layer takes
# another kernel and the shell lane must change nothing there; 66 frames: clips_per_pass = 1, two decoder passes, the shell events used four
# times in one call; 40^3: coarse 10 and 20
@pytest.mark.parametrize("G,B,T", [(64, 1, 2), (32, 2, 3), (48, 1, 2), (32, 2, 33), (40, 1, 2)])
def test_new_schedule_is_bit_identical_to_the_serial_one(G, B, T):
    o, sd, vox, eps, ref = _case(G, B, T)
    with _switches(NEW):                               # (the context is created by the first call: it reads the switches then)
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "G=%d B=%d T=%d" % (G, B, T))


@pytest.mark.parametrize("bit", [2, 4])
def test_each_part_alone_is_bit_identical(bit):
    o, sd, vox, eps, ref = _case(64, 1, 2)
    with _switches({**SERIAL, "NM355_ENC_SCHED": str(1 | bit)}):
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "NM355_ENC_SCHED=%d" % (1 | bit))


def test_the_whole_mask_off_is_bit_identical():
    """NM355_ENC_SCHED=0: encoder and decoder serial"""
    o, sd, vox, eps, ref = _case(64, 1, 2)
    with _switches({"NM355_ENC_SCHED": "0"}):
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "NM355_ENC_SCHED=0")


@pytest.mark.parametrize("K", [12, 28])
def test_other_keypoint_counts_are_bit_identical(K):
    """other heat-map channel paddings and clip_loss_kernel sizes"""
    o, sd, vox, eps, ref = _case(32, 1, 2, nkeypoints=K)
    with _switches(NEW):
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "K=%d" % K)


def test_one_product_mode_is_bit_identical():
    """conv mode 'f16': the one-product instantiations of the shell kernels beside each other"""
    o, sd, vox, eps, ref = _case(64, 1, 2, mode="f16")
    with _switches(NEW):
        out = _forward(_net(o, sd, "f16"), vox, eps)
    _same(out, ref, "f16")


def test_repeated_forwards_on_one_context_repeat_the_first():
    """five consecutive forwards, then twenty more: the events are re-recorded every call, and a store race between face and edge
    items or a scratch race between the streams shows as a mismatch between calls"""
    o, sd, vox, eps, ref = _case(64, 1, 2)
    with _switches(NEW):
        net = _net(o, sd)
        outs = [_forward(net, vox, eps) for _ in range(5)]
        outs += [_forward(net, vox, eps) for _ in range(20)]
    for i, out in enumerate(outs):
        _same(out, outs[0], "call %d against the first" % i)
        _same(out, ref, "call %d against the serial arm" % i)


def test_decode_from_dyna_is_bit_identical():
    """nm_decode_from_keypoints runs the same decoder passes (no losses: bit 2 alone)"""
    o, sd, vox, eps, _ = _case(64, 1, 2)
    gen, det = {}, None
    for name, env in (("serial", SERIAL), ("new", NEW)):
        with _switches(env):
            net = _net(o, sd)
            with torch.no_grad():
                if det is None:                  # both arms decode the serial arm's keypoints and feature
                    det = {k: v.detach().clone() for k, v in net.kypt_detector.detect(vox).items() if torch.is_tensor(v)}
                gen[name] = net.kypt_detector.decode_from_dyna(det["keypoints"], det["first_feature"], vox[:, 0])["gen"].detach().clone()
            torch.cuda.synchronize()
    assert gen["serial"].abs().max().item() > 0
    assert _equal(gen["new"], gen["serial"])


def test_materialised_combined_tensor_is_untouched():
    """gaussian_cat_type 'max': the combined tensor is materialised and the decoder starts from another kernel; the schedule is the same"""
    o, sd, vox, eps, ref = _case(32, 1, 2, gaussian_cat_type="max")
    with _switches(NEW):
        out = _forward(_net(o, sd), vox, eps)
    _same(out, ref, "gaussian_cat_type max")


def _side_launches(net, run):
    """launches the decoder schedule sent to the third stream during run() (nm_prof_read variant 16: a count)"""
    lib, h = net._engine.ctx.lib, net._engine.ctx.handle
    _lib.check(lib.nm_prof_enable(h, 1), "prof_enable")
    run()
    torch.cuda.synchronize()
    _lib.check(lib.nm_prof_enable(h, 0), "prof_enable")
    ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
    _lib.check(lib.nm_prof_read(h, 16, C.byref(ms), C.byref(fl), C.byref(n)), "prof_read")
    return n.value


@pytest.mark.parametrize("mask,G,want", [("7", 64, 3), ("3", 64, 2), ("5", 64, 1), ("1", 64, 0), ("0", 64, 0), ("7", 48, 2)])
def test_the_new_path_is_taken(mask, G, want):
    """no silent fall-back to the serial order: at 64^3 one forward sends the two up layers' edge kernels (bit 2) and clip_loss_kernel
    (bit 4) to the third stream; at 48^3 the first up layer (coarse 12: no whole 2 x 8 x 8 bricks) runs another kernel, the second (coarse 24) and clip_loss_kernel go;
    a training step sends none"""
    o, sd, vox, eps, _ = _case(G, 1, 2)
    with _switches({"NM355_ENC_SCHED": mask, "NM355_ENC_S1": "1"}):
        net = _net(o, sd)
        _forward(net, vox, eps)
        assert _side_launches(net, lambda: _forward(net, vox, eps)) == want
        if mask == "7" and G == 64:
            def train_fwd():
                net(vox, ACTS, eps=eps)
            assert _side_launches(net, train_fwd) == 0


def test_launch_placement():
    """the edge kernels have no bracket of their own: per family, the main stream's and all streams' profiled launches of one forward
    are the same under both arms, and family 12 (main + shell launch of a fused-upsample layer, timed together, joined inside the
    launcher) is still one bracket per up layer on the main stream"""
    o, sd, vox, eps, _ = _case(64, 1, 2)
    counts = {}
    for name, env in (("new", NEW), ("serial", SERIAL)):
        with _switches(env):
            net = _net(o, sd)
            _forward(net, vox, eps)
            counts[name] = [_launches(net, lambda: _forward(net, vox, eps), m) for m in (1, 2)]
    print("profiled conv launches per family [main stream, all streams]:", counts)
    assert counts["new"] == counts["serial"]
    assert counts["new"][0][12] == 2 and counts["new"][1][12] == 2, counts["new"]
    assert sum(counts["new"][0]) > 10


def test_training_forward_and_backward_are_untouched():
    """one DetectorTrainer step under the new schedule and under the serial arm: same loss and gradients, bit for bit, and the same
    profiled launches on the same streams (main stream / all streams)"""
    from neural_marionette_amd.train import DetectorTrainer
    o = HotPathOptions(grid_size=32)
    sd = synth.make_state_dict(o, seed=5, variant="peaky")
    vox = synth.figure_clip(1, 3, 32, seed=6).cuda()
    res = {}
    for name, env in (("new", NEW), ("serial", SERIAL)):
        with _switches(env):
            net = _net(o, sd)
            net.train()
            tr = DetectorTrainer(net, lr=4e-4)
            step = tr.step(vox)
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            counts = [sum(_launches(net, lambda: tr.step(vox), m)) for m in (1, 2)]
        res[name] = (counts, step, grads)
    print("training step, profiled conv launches [main stream, all streams]:", res["new"][0], res["serial"][0])
    assert res["new"][0] == res["serial"][0]
    assert res["new"][0][0] > 0
    assert sorted(res["new"][1]) == sorted(res["serial"][1]) and "loss" in res["new"][1]
    for k, v in res["serial"][1].items():
        assert _equal(torch.tensor(v, dtype=torch.float64), torch.tensor(res["new"][1][k], dtype=torch.float64)), (k, v, res["new"][1][k])
    assert set(res["new"][2]) == set(res["serial"][2]) and len(res["new"][2]) > 10
    for k, g in res["serial"][2].items():
        assert _equal(g, res["new"][2][k]), k
