"""The HIP VRNN at the batch sizes where nm_vrnn.hip changes its kernels, against an fp64 evaluation of the oracle (tests/vrnn_ref.py):
the row kernels below 128 rows, the fp32-MFMA GEMM (and its broadcast-add epilogue: the decoders' z-halves at S B >= 128 rows add the
h-half of clip b % B) from 128, the GRU input projection as a GEMM, the persistent posterior chain up to S B = 96, the six-launch
posterior steps beyond it, the prior mid kernel and the captured rollout graph up to B = 64, the learner's BPTT with weight-gradient sums
over T B > 64 samples, and the Adam launch at its chunk boundaries.

Bounds.  fp32 arithmetic in any order is some distance from fp64; the fp32 oracle (the reference's own arithmetic) measures that distance
at each shape, and the HIP result must be within 4x of it (floor as stated) - printed next to it.  Operations: MLP / GRU / latents 1e-5
absolute; forward kinematics and step outputs within 4x the oracle's deviation + 2e-5, on rows whose 6-D rotations are ordinarily
conditioned (every joint's |b| / |x^ x b| < 10) and, scaled by each row's conditioning, on all rows (_check_conditioned).  Whole
sequences: best-of-S indices exact (every selection of these seeds has an fp64 margin >= 1e-4, tests/test_vrnn_ref_cpu.py), each step
re-run from the fp64 state within KP_TOL, free-running outputs within 4x the oracle's deviation.  Every fp64 reference is computed once
per module."""
import ctypes as C

import numpy as np
import pytest
import torch

import vrnn_ref as V
from neural_marionette_amd import NeuralMarionette, synth, _lib

pytestmark = pytest.mark.gpu

OP_TOL = 1e-5          # MLP, GRU, z
FK_TOL = 2e-5          # keypoints, R, step outputs: on top of 4x the fp32 oracle's deviation (_check_conditioned)
COND_MAX = 10.0
KP_TOL = 1e-4          # teacher-forced step (north star)
ACTS = {"detector": True, "learner": True}

_NETS, _REFS = {}, {}


class _switches:
    """NM355_* switches are read when a context is created (test_grad_ops_gpu._switches)"""
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        import os
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _net(o, sd, aff, parents, wseed, env=None, fresh=False):
    """a network on the GPU with the weights of vrnn_ref.model(K, wseed), whose context was created under `env` and whose skeleton
    is the oracle's; one per (K, wseed, env) for the module unless `fresh` (then the caller owns it: a test that trains or needs a
    context of its own)"""
    key = (o.nkeypoints, wseed, tuple(sorted((env or {}).items())))
    if key in _NETS and not fresh:
        return _NETS[key]
    with _switches(env or {}):
        net = NeuralMarionette(o)
        net.load_state_dict(sd)
        net = net.cuda().eval()
        net.anneal(1)
        with torch.no_grad():
            net.kypt_detector.get_affinity()             # (creates the context while the switches are set)
    K, Z = o.nkeypoints, o.nlatent_kypt
    with torch.no_grad():
        net.dyna_module.encode(torch.zeros(1, 2, K, 4).cuda() + 0.1, aff.cuda(), SAMPLE_NUM=1, eps=torch.zeros(2, 1, 1, Z).cuda())   # builds the tree
    assert np.array_equal(net.dyna_module.parents.cpu().numpy(), parents)
    if not fresh:
        _NETS[key] = net
    return net


def _model(K, wseed):
    key = ("model", K, wseed)
    if key not in _REFS:
        _REFS[key] = V.model(K, wseed)
    return _REFS[key]


def _cached(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def _err(a, b):
    return V._err(a, b)


def _rowerr(a, b):
    """largest absolute difference per leading row"""
    d = (V._t(a, torch.float64) - V._t(b, torch.float64)).abs()
    return d.reshape(d.shape[0], -1).max(dim=1).values


def _conditioning(sd, dec, K):
    """(vrnn_ref.rot6d_conditioning, vrnn_ref.rot6d_sensitivity) of the decoder inputs `dec` (..., H+Z)"""
    return V.rot6d_conditioning(sd, dec, K), V.rot6d_sensitivity(sd, dec, K)


def _check_conditioned(what, got, r64, r32, conditioning):
    """Rows whose 6-D rotations are ordinarily conditioned (every joint's |b| / |x^ x b| < COND_MAX): within 4x the fp32 oracle's largest
    deviation on those rows + FK_TOL (a flat FK_TOL does not hold for fp32 arithmetic itself: the oracle's ordinary-row deviation reaches
    3.7e-5 at K 32, B 1000).  Every row: within 4x the oracle's largest deviation + FK_TOL, or - on an ill-conditioned row - within 4x the
    oracle's largest deviation PER UNIT OF SENSITIVITY times the row's own sensitivity + FK_TOL (vrnn_ref.rot6d_sensitivity: both
    normalisations of rot6d divide by |a| and |x^ x b|, so two fp32 evaluations of one ill-conditioned row differ by an amount that
    scales with it, and the oracle's worst row need not be the kernel's - measured: 1.4e-4 on one row of B 200, |a| = 0.020 and
    |x^ x b| = 0.011 there, where the oracle's worst row is 1.3e-5)."""
    cond, sens = conditioning
    e, e32 = _rowerr(got, r64), _rowerr(r32, r64)
    c = sens.clamp_min(1.0)
    ok = cond < COND_MAX
    e_ord = e[ok].max().item() if ok.any() else 0.0
    d_ord = e32[ok].max().item() if ok.any() else 0.0
    assert e_ord <= 4 * d_ord + FK_TOL, f"{what}: {e_ord:.3e} on ordinarily conditioned rows, fp32 oracle {d_ord:.3e}"
    per_cond = (e32 / c).max().item()
    bound = torch.clamp(4 * per_cond * c, min=4 * e32.max().item()) + FK_TOL
    bad = e > bound
    assert not bad.any(), (f"{what}: row {int(bad.nonzero()[0])} off by {e[bad].max().item():.3e} (sensitivity {c[bad].max().item():.1f}), "
                           f"fp32 oracle worst {e32.max().item():.3e}, per unit of sensitivity {per_cond:.3e}")
    return e.max().item(), e32.max().item()


# ---- operations through the shells -------------------------------------------------------------------------------------------
OP_B = [1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 1000]
OP_K = [2, 22, 24, 32]


@pytest.mark.parametrize("K", OP_K)
@pytest.mark.parametrize("B", OP_B)
def test_submodule_callables_across_batch_paths(B, K):
    """The sub-module callables and fused steps at batch sizes on both sides of the row kernels' and the GEMM's ranges (K 24 / 32: every
    segment a multiple of 32 columns, GEMM-eligible from 128 rows; K 22 / 2: the post0 and GRU input segments are not)."""
    o, sd, order, parents, aff = _model(K, 80 + K)
    net = _net(o, sd, aff, parents, 80 + K)
    d = net.dyna_module
    H, Z = o.nhidden_kypt, o.nlatent_kypt
    g = torch.Generator().manual_seed(B * 100 + K)
    h = torch.randn(B, H, generator=g) * 0.5
    z = torch.randn(B, Z, generator=g)
    kp = V.keypoints(B, 6, K, B + K)
    obs = kp[:, 2]
    hz = torch.cat([h, z], -1)
    worst = {}
    with torch.no_grad():
        x = torch.cat([h, obs.reshape(B, -1)], -1)
        for name, fn, inp in (("extract_post_dist", d.extract_post_dist, x), ("extract_prior_dist", d.extract_prior_dist, h),
                              ("root_intensity_decoder", d.root_intensity_decoder, hz), ("joint_matrix_decoder", d.joint_matrix_decoder, hz)):
            e = _err(fn(inp.cuda()), V.mlp(sd, inp, name))
            worst[name] = e
            assert e <= OP_TOL, (name, e)
        xin = torch.randn(B, 4 * K + Z, generator=g)
        e = _err(d.kypt_rnn_cell(xin.cuda(), h.cuda()), V.gru(sd, xin, h))
        worst["gru"] = e
        assert e <= OP_TOL, ("gru", e)
        off = d.get_offset(kp.cuda())
        assert _err(off, V.offsets(sd, kp, parents)) <= 1e-6
        off64 = V._t(off, torch.float64)
        # forward kinematics (rows of the fp64 reference's own conditioning)
        flat, R = d.extract_kypt_from_latent_and_state(hz.cuda(), off)
        f64, R64 = V.fk(sd, hz, off64, order, parents)
        f32, R32 = V.fk(sd, hz, off64, order, parents, torch.float32)
        cond = _conditioning(sd, hz, K)
        worst["fk"] = _check_conditioned("fk keypoints", flat, f64, f32, cond)
        _check_conditioned("fk R", R, R64, R32, cond)
        # prior step (six launches below / GEMM from 128 rows; the h-phase's mid kernel up to 64)
        eps = torch.randn(B, Z, generator=g)
        kps, zs, hn = d.step(h.cuda(), off, eps.cuda())
        p64 = V.prior_step(sd, h, eps, off64, order, parents)
        p32 = V.prior_step(sd, h, eps, off64, order, parents, torch.float32)
        assert _err(zs, p64["z"]) <= OP_TOL
        c = _conditioning(sd, p64["dec"], K)
        worst["prior"] = _check_conditioned("prior step keypoints", kps, p64["kp"], p32["kp"], c)
        _check_conditioned("prior step state", hn, p64["h"], p32["h"], c)
        # posterior steps: S B crosses 128 with B < S B (the decoders' epilogue adds the h-half of clip b % B)
        ar = torch.arange(B)
        for S in (1, 3, 10):
            eps = torch.randn(S, B, Z, generator=g)
            kps, zs, hn = d.step(h.cuda(), off, eps.cuda(), keypoints_obs=obs.cuda(), SAMPLE_NUM=S)
            a64 = V.posterior_all(sd, h, obs, eps, off64, order, parents)
            a32 = V.posterior_all(sd, h, obs, eps, off64, order, parents, torch.float32)
            sel = a64["d"].argmin(0)
            near = V.selection_margins(a64["d"]) < V.MARGIN_MIN
            # the sample the kernel took, recognised by its latent (samples differ by eps * sigma, far beyond rounding)
            took = (V._t(zs, torch.float64)[None] - a64["z"]).abs().amax(-1).argmin(0)
            top2 = a64["d"].topk(min(2, S), dim=0, largest=False).indices
            assert torch.equal(took[~near], sel[~near]), f"S={S}: best-of-S index differs from fp64 on rows {torch.nonzero((took != sel) & ~near).flatten().tolist()[:8]}"
            assert (took[near][None] == top2[:, near]).any(0).all(), f"S={S}: a near tie resolved to neither of its two best samples"
            pick = torch.where(near, took, sel)
            c = _conditioning(sd, a64["dec"][pick, ar], K)
            assert _err(zs, a64["z"][pick, ar]) <= OP_TOL
            e = _check_conditioned("posterior S=%d keypoints" % S, kps, a64["kp"][pick, ar], a32["kp"][pick, ar], c)
            _check_conditioned("posterior S=%d state" % S, hn, a64["h"][pick, ar], a32["h"][pick, ar], c)
            worst["post%d" % S] = e
            if near.any():
                print("B=%d K=%d S=%d: %d near-tied selections (fp64 margin < %.0e)" % (B, K, S, int(near.sum()), V.MARGIN_MIN))
    print("B=%d K=%d: %s" % (B, K, ", ".join("%s %s" % (k, ("%.1e" % v) if not isinstance(v, tuple) else "%.1e (fp32 oracle %.1e)" % v)
                                            for k, v in worst.items())))


@pytest.mark.parametrize("shared", [False, True], ids=["per-row-target", "shared-target"])
@pytest.mark.parametrize("B", [1, 255, 256, 257, 10000])
def test_nearest_row(B, shared):
    """nm_rows_argmin_dist (one workgroup, 256 threads, strided rows, then a tree reduction): a planted nearest row anywhere, and an exact
    duplicate of it further down, where the first index must win; the fp64 argmin agrees"""
    o, sd, order, parents, aff = _model(24, 104)
    d = _net(o, sd, aff, parents, 104).dyna_module
    D = 96
    g = torch.Generator().manual_seed(B + 7 * shared)
    for case in range(3):
        rows = torch.randn(B, D, generator=g)
        t = torch.randn(1 if shared else B, D, generator=g)
        i = int(torch.randint(0, B, (1,), generator=g)) if case < 2 else B - 1
        ti = t[0] if shared else t[i]
        rows[i] = ti + 1e-3 * torch.randn(D, generator=g)
        want = i
        if case == 1 and B > 1:                        # the planted row twice: at i and at another index j
            j = int(torch.randint(0, B, (1,), generator=g))
            j = j if j != i else (i + 1) % B
            rows[j] = rows[i].clone()
            if not shared:
                t[j] = ti.clone()
            want = min(i, j)
        tt = t.expand(B, D) if shared else t
        dist = (rows.double() - tt.double()).pow(2).sum(1)
        assert int(dist.argmin()) == want
        got = d.nearest_row(rows.cuda(), (t[0] if shared else t).cuda())
        assert got == want, (case, got, want)


# ---- encode across its paths -------------------------------------------------------------------------------------------------
def _encode_refs(case):
    def make():
        o, sd, order, parents, aff, kp, eps = V.encode_inputs(case)
        r64 = V.encode(sd, o, kp, order, parents, eps)
        r32 = V.encode(sd, o, kp, order, parents, eps, dtype=torch.float32)
        return o, sd, order, parents, aff, kp, eps, r64, r32
    return _cached(("enc", case), make)


def _check_encode_vs_fp64(out, r64, r32, what):
    lines = []
    for k in ("kypt_recon", "R", "z_kypts", "h_kypts"):
        e, e32 = _err(out[k], r64[k]), _err(r32[k], r64[k])
        lines.append("%s %.2e (fp32 oracle %.2e)" % (k, e, e32))
        assert e <= 4 * max(e32, 1e-6), f"{what} {k}: {e:.3e}, fp32 oracle {e32:.3e}"
    for k in ("kl_kypt", "kypt_recon_loss"):
        e, e32 = abs(float(out[k]) - float(r64[k])), abs(float(r32[k]) - float(r64[k]))
        lines.append("%s %.2e (fp32 oracle %.2e)" % (k, e, e32))
        assert e <= 4 * max(e32, 1e-6 * max(1.0, abs(float(r64[k])))), f"{what} {k}: {e:.3e}, fp32 oracle {e32:.3e}"
    print(what + ": " + ", ".join(lines))


def _encode_case(case, env=None, fresh=False):
    o, sd, order, parents, aff, kp, eps, r64, r32 = _encode_refs(case)
    B, S, T = V.ENCODE_CASES[case][:3]
    net = _net(o, sd, aff, parents, V.ENCODE_CASES[case][4], env, fresh)
    d = net.dyna_module
    with torch.no_grad():
        out = d.encode(kp.cuda(), aff.cuda(), SAMPLE_NUM=S, eps=eps.cuda())
        torch.cuda.synchronize()
        assert np.array_equal(out["best_idx"].cpu().numpy(), r64["best_idx"].numpy().astype(np.int32)), "best-of-S indices differ from fp64"
        off = V._t(r64["offset"], torch.float32).reshape(B, -1, 3).cuda()
        step = lambda h, ob, e: d.step(V._t(h, torch.float32).cuda(), off, e.cuda(), keypoints_obs=ob.cuda(), SAMPLE_NUM=S)
        tf = V.teacher_forced(step, r64, kp, eps)
    tf32 = _cached(("tf32", case), lambda: V.teacher_forced(V.oracle_step(sd, r64, order, parents), r64, kp, eps))
    print("%s: teacher-forced worst step %.2e (fp32 oracle %.2e)" % (case, max(tf), max(tf32)))
    assert max(tf) < KP_TOL
    _check_encode_vs_fp64(out, r64, r32, case + ("" if not env else " " + str(env)))
    return out


@pytest.mark.parametrize("case", list(V.ENCODE_CASES))
def test_encode_across_batch_paths_vs_fp64(case):
    _encode_case(case)


@pytest.mark.parametrize("env", [{"NM355_VRNN_GEMM": "0"}], ids=["row-kernels-only"])
@pytest.mark.parametrize("case", ["gemm-16x10", "gemm-24x10"])
def test_encode_kernel_variants_vs_fp64(case, env):
    _encode_case(case, env, fresh=True)


def test_inference_forward_vrnn_off_the_chain_vs_fp64():
    """net(vox, eps) at 32^3, B = 16, T = 4: S B = 160, so the VRNN inside nm_forward_fused runs six-launch GEMM steps.  Its VRNN
    outputs equal a stand-alone encode on its own keypoints and affinity, which is held to fp64 on those keypoints."""
    o, sd, order, parents, aff = _model(24, 71)
    net = _net(o, sd, aff, parents, 71, fresh=True)
    B, T, S = 16, 4, 10
    vox = synth.figure_clip(B, T, 32, seed=3).cuda()
    eps = synth.make_eps((T, S, B, o.nlatent_kypt), seed=4)
    with torch.no_grad():
        out = net(vox, ACTS, eps=eps.cuda())
        enc = net.dyna_module.encode(out["keypoints"], out["affinity"], SAMPLE_NUM=S, eps=eps.cuda())
        torch.cuda.synchronize()
    for k in ("kypt_recon", "R", "z_kypts", "h_kypts", "best_idx", "kl_kypt", "kypt_recon_loss"):
        assert torch.equal(out[k], enc[k]), k
    kp = out["keypoints"].cpu()
    order_n = net.dyna_module.priority.indices.cpu().numpy()
    parents_n = net.dyna_module.parents.cpu().numpy()
    r64 = V.encode(sd, o, kp, order_n, parents_n, eps)
    r32 = V.encode(sd, o, kp, order_n, parents_n, eps, dtype=torch.float32)
    m = V.encode_margins(r64).min().item()
    assert m >= V.MARGIN_MIN, f"the detector's keypoints give a near-tied selection ({m:.2e}): choose another clip seed"
    assert np.array_equal(out["best_idx"].cpu().numpy(), r64["best_idx"].numpy().astype(np.int32))
    _check_encode_vs_fp64(out, r64, r32, "forward B=16 T=4")


# ---- learner training at the reference's batch sizes -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(V.LEARNER_CASES))
def test_learner_gradients_at_reference_batch_sizes_vs_fp64(case):
    """d(kypt_recon_loss + 0.003 kl_kypt)/d(every dyna_module parameter) from the training forward (six-launch steps, tape) and the
    BPTT kernels, whose weight gradients sum over T B > 64 samples; per tensor, max error relative to the tensor's max within 4x the
    fp32 oracle's (floor 1e-5) and never above 2e-3"""
    def make():
        o, sd, order, parents, aff, kp, eps = V.learner_inputs(case)
        return (o, sd, order, parents, aff, kp, eps, V.learner_grads(sd, o, kp, order, parents, eps),
                V.learner_grads(sd, o, kp, order, parents, eps, dtype=torch.float32))
    o, sd, order, parents, aff, kp, eps, (l64, g64), (l32, g32) = _cached(("learn", case), make)
    net = _net(o, sd, aff, parents, V.LEARNER_CASES[case][3])
    net.train()
    try:
        net.zero_grad()
        out = net.dyna_module.encode(kp.cuda(), aff.cuda(), eps=eps.cuda())
        loss = 1.0 * out["kypt_recon_loss"] + 0.003 * out["kl_kypt"]
        loss.backward()
        torch.cuda.synchronize()
        _check_loss_and_grads(case, float(loss), l64, l32, {"dyna_module." + n: p.grad for n, p in net.dyna_module.named_parameters()
                                                             if p.requires_grad}, g64, g32)
    finally:
        net.zero_grad()
        net.eval()


def _check_loss_and_grads(what, loss, l64, l32, grads, g64, g32):
    """loss within 4x the fp32 oracle's deviation (floor 1e-6 relative); every gradient tensor, as max error relative to the tensor's max,
    within 4x the oracle's (floor 1e-5) and never above 2e-3"""
    el, el32 = abs(loss - l64), abs(l32 - l64)
    print("%s: loss err %.2e (fp32 oracle %.2e)" % (what, el, el32))
    assert el <= 4 * max(el32, 1e-6 * abs(l64))
    assert set(grads) == set(g64)
    worst = 0.0
    for name, g in grads.items():
        r, r32 = g64[name], g32[name]
        assert g is not None, name
        scale = max(r.abs().max().item(), 1e-30)
        e, e32 = _err(g, r) / scale, _err(r32, r) / scale
        worst = max(worst, e / max(4 * e32, 1e-5))
        assert e <= min(4 * max(e32, 1e-5), 2e-3), f"{name}: {e:.3e} relative, fp32 oracle {e32:.3e}"
    print("%s: worst gradient error / bound %.2f" % (what, worst))


def _trainer_net(B, T, clip_seed):
    """the AIST learner setting on seeded weights: 32^3 figure clips, peaky detector weights; the frozen detector's keypoints and
    affinity (KyptDetector.detect: bit-identical to the trainer's lean forward, test_lean_learner_step_is_bit_identical_to_the_full_one)"""
    from neural_marionette_amd import HotPathOptions
    o = HotPathOptions(grid_size=32)
    sd = synth.make_state_dict(o, seed=31, variant="peaky")
    net = NeuralMarionette(o)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    net.anneal(1)
    vox = synth.figure_clip(B, T, 32, seed=clip_seed).cuda()
    with torch.no_grad():
        det = net.kypt_detector.detect(vox)
    return o, sd, net, vox, det["keypoints"], det["affinity"]


def _tree(net):
    return net.dyna_module.priority.indices.cpu().numpy(), net.dyna_module.parents.cpu().numpy()


def test_learner_trainer_step_at_the_aist_shape_vs_fp64():
    """One LearnerTrainer(lean=True) step at the shape the shipped AIST dynamics were trained at (B 16, T 20, K 24, best of 10): the
    20-step training forward with its tape and the BPTT over 20 steps, through the trainer's path (lean detector forward, GradBucket,
    finiteness flag, Adam).  The VRNN reference is fed the GPU detector's keypoints and affinity; loss and every gradient against fp64
    autograd within the self-calibrated bound, and the forward teacher-forced from the fp64 states within KP_TOL."""
    from neural_marionette_amd.train import LearnerTrainer
    B, T, S = 16, 20, 10
    o, sd, net, vox, kp, aff = _trainer_net(B, T, clip_seed=61)
    eps = synth.make_eps((T, S, B, o.nlatent_kypt), seed=62)
    d = net.dyna_module
    with torch.no_grad():
        d.encode(kp, aff, eps=eps.cuda())                  # builds the skeleton from the detector's affinity, as the step would
    order, parents = _tree(net)
    kpc = kp.cpu()
    r64 = V.encode(sd, o, kpc, order, parents, eps)
    m = V.encode_margins(r64).min().item()
    assert m >= V.MARGIN_MIN, f"the detector's keypoints give a near-tied selection ({m:.2e}): choose another clip seed"
    with torch.no_grad():
        off = V._t(r64["offset"], torch.float32).reshape(B, -1, 3).cuda()
        tf = V.teacher_forced(lambda h, ob, e: d.step(V._t(h, torch.float32).cuda(), off, e.cuda(), keypoints_obs=ob.cuda(), SAMPLE_NUM=S),
                              r64, kpc, eps)
    print("AIST shape: teacher-forced worst step %.2e" % max(tf))
    assert max(tf) < KP_TOL
    l64, g64 = V.learner_grads(sd, o, kpc, order, parents, eps)
    l32, g32 = V.learner_grads(sd, o, kpc, order, parents, eps, dtype=torch.float32)
    net.train()
    tr = LearnerTrainer(net, lr=4e-4, lean=True)
    res = tr.step(vox, eps=eps.cuda())
    torch.cuda.synchronize()
    _check_loss_and_grads("AIST shape trainer step", res["loss"], l64, l32, {n: p.grad for n, p in tr.named}, g64, g32)


def test_learner_trainer_three_steps_at_reference_batch_vs_fp64_adam():
    """Three LearnerTrainer steps at the reference train.py's nbatch = 24 (T 4): per-step losses against the fp64 oracle + float64
    torch.optim.Adam within the self-calibrated bound, and the updated weights by the 'bulk of the update' criterion of
    test_learner_training_trajectory_vs_oracle"""
    from neural_marionette_amd.train import LearnerTrainer
    B, T, S = 24, 4, 10
    o, sd, net, vox, kp, aff = _trainer_net(B, T, clip_seed=63)
    epss = [synth.make_eps((T, S, B, o.nlatent_kypt), seed=64 + i) for i in range(3)]
    net.train()
    tr = LearnerTrainer(net, lr=4e-4)
    losses = [tr.step(vox, eps=e.cuda())["loss"] for e in epss]
    torch.cuda.synchronize()
    order, parents = _tree(net)
    kpc = kp.cpu()
    for e in epss:                                        # (the first step's margins are the ones that depend on the seed alone)
        m = V.encode_margins(V.encode(sd, o, kpc, order, parents, e)).min().item()
        assert m >= V.MARGIN_MIN, f"near-tied selection ({m:.2e}): choose other seeds"
    ref, p64 = V.adam_trajectory(sd, o, kpc, order, parents, epss)
    ref32, _ = V.adam_trajectory(sd, o, kpc, order, parents, epss, dtype=torch.float32)
    print("trainer B=24 losses", losses, "fp64", ref, "fp32 oracle", ref32)
    for a, b, c in zip(losses, ref, ref32):
        assert abs(a - b) <= 4 * max(abs(c - b), 1e-6 * abs(b)), (a, b, c)
    assert losses[-1] < losses[0]
    name = "dyna_module.kypt_rnn_cell.weight_hh"
    w = dict(tr.named)[name].detach().cpu().double()
    diff = (w - p64[name]).abs()
    upd = (p64[name] - sd[name].double()).abs()
    print("weight_hh after 3 steps: mean abs diff %.3e, mean update %.3e, elements off by > 1e-5: %.4f %%" %
          (diff.mean().item(), upd.mean().item(), 100.0 * (diff > 1e-5).double().mean().item()))
    assert diff.mean().item() < 0.01 * upd.mean().item()
    assert (diff > 1e-5).double().mean().item() < 0.01


def test_wrongly_shaped_eps_is_refused_before_the_library():
    """The shells pass eps to the library as a raw pointer; a tensor smaller than the library reads (noise for fewer samples than
    SAMPLE_NUM, a prior draw where a posterior one is due) would be an out-of-bounds read on the device.  They refuse it instead."""
    o, sd, order, parents, aff = _model(24, 104)
    d = _net(o, sd, aff, parents, 104).dyna_module
    B, T, S, Z, H = 3, 4, 10, o.nlatent_kypt, o.nhidden_kypt
    kp = V.keypoints(B, T, o.nkeypoints, 5).cuda()
    a = aff.cuda()
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    with torch.no_grad():
        with pytest.raises(ValueError, match="eps must be"):
            d.encode(kp, a, SAMPLE_NUM=S, eps=zeros(T, S - 1, B, Z))
        with pytest.raises(ValueError, match="eps must be"):
            d.generate(kp[:, :2], a, Ttot=5, Tcond=2, SAMPLE_NUM=S, eps_post=zeros(2, S - 1, B, Z), eps_prior=zeros(3, B, Z))
        with pytest.raises(ValueError, match="eps must be"):
            d.generate(kp[:, :2], a, Ttot=5, Tcond=2, SAMPLE_NUM=S, eps_post=zeros(2, S, B, Z), eps_prior=zeros(2, B, Z))
        off, h = d.get_offset(kp), zeros(B, H)
        with pytest.raises(ValueError, match="eps must be"):
            d.step(h, off, zeros(B, Z), keypoints_obs=kp[:, 0], SAMPLE_NUM=S)
        with pytest.raises(ValueError, match="eps must be"):
            d.step(h, off, zeros(S, B, Z))
        # the well-shaped calls run
        d.encode(kp, a, SAMPLE_NUM=S, eps=zeros(T, S, B, Z))
        d.step(h, off, zeros(S, B, Z), keypoints_obs=kp[:, 0], SAMPLE_NUM=S)
        d.step(h, off, zeros(B, Z))
        torch.cuda.synchronize()


# ---- generation and rollouts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", V.GEN_B)
def test_generate_and_rollout_across_batch_paths(B):
    """HSVRNNBVH.generate (Tcond 5, Ttot 20) and .rollout at B = 5 / 16 / 64 (prior mid kernel + captured graph) and 65 / 130 (six-launch
    prior steps, GEMM at 130): every step re-run from the fp64 state within KP_TOL, free-running errors reported"""
    Tc, Tt = 5, 20
    def make():
        o, sd, order, parents, aff, kp, ep, er = V.generate_inputs(B)
        return o, sd, order, parents, aff, kp, ep, er, V.generate(sd, o, kp, order, parents, Tt, Tc, ep, er), \
            V.generate(sd, o, kp, order, parents, Tt, Tc, ep, er, dtype=torch.float32)
    o, sd, order, parents, aff, kp, ep, er, r64, r32 = _cached(("gen", B), make)
    K = o.nkeypoints
    d = _net(o, sd, aff, parents, V.GEN_SEEDS[0]).dyna_module
    with torch.no_grad():
        out = d.generate(kp.cuda(), aff.cuda(), Ttot=Tt, Tcond=Tc, eps_post=ep.cuda(), eps_prior=er.cuda())
        off = V._t(r64["offset"], torch.float32).reshape(B, K, 3).cuda()
        h5 = V._t(r64["h_seq"][:, Tc], torch.float32).cuda()
        rk, rh = d.rollout(h5, off, er.cuda())
        torch.cuda.synchronize()
        worst = worst32 = 0.0
        ostep = V.oracle_step(sd, dict(offset=r64["offset"]), order, parents)
        for t in range(Tc):
            h = r64["h_seq"][:, t]
            kps, zs, hn = d.step(V._t(h, torch.float32).cuda(), off, ep[t].cuda(), keypoints_obs=kp[:, t].cuda())
            o32 = _cached(("gen-tf32", B, t), lambda: ostep(h, kp[:, t], ep[t]))
            for a, b in ((kps.view(B, K, 4), r64["keypoints_cond"][:, t]), (zs, r64["z_seq"][:, t]), (hn, r64["h_seq"][:, t + 1])):
                worst = max(worst, _err(a, b))
            worst32 = max(worst32, _err(o32[0].view(B, K, 4), r64["keypoints_cond"][:, t]), _err(o32[1], r64["z_seq"][:, t]), _err(o32[2], r64["h_seq"][:, t + 1]))
        for t in range(Tc, Tt):
            h = r64["h_seq"][:, t]
            kps, zs, hn = d.step(V._t(h, torch.float32).cuda(), off, er[t - Tc].cuda())
            o32 = _cached(("gen-tf32", B, t), lambda: V.prior_step(sd, h, er[t - Tc], r64["offset"], order, parents, torch.float32))
            for a, b in ((kps.view(B, K, 4), r64["keypoints_gen"][:, t - Tc]), (zs, r64["z_seq"][:, t]), (hn, r64["h_seq"][:, t + 1])):
                worst = max(worst, _err(a, b))
            worst32 = max(worst32, _err(o32["kp"].view(B, K, 4), r64["keypoints_gen"][:, t - Tc]), _err(o32["z"], r64["z_seq"][:, t]),
                          _err(o32["h"], r64["h_seq"][:, t + 1]))
    e_c, e_g = _err(out["keypoints_cond"], r64["keypoints_cond"]), _err(out["keypoints_gen"], r64["keypoints_gen"])
    e_c32, e_g32 = _err(r32["keypoints_cond"], r64["keypoints_cond"]), _err(r32["keypoints_gen"], r64["keypoints_gen"])
    e_r1, e_r = _err(rk[:, 0], r64["keypoints_gen"][:, 0]), _err(rk, r64["keypoints_gen"])
    print("generate B=%d: cond %.2e (fp32 oracle %.2e), free-running %.2e (fp32 oracle %.2e); rollout from the fp64 state: first step "
          "%.2e, free-running %.2e; teacher-forced worst step %.2e (fp32 oracle %.2e)" % (B, e_c, e_c32, e_g, e_g32, e_r1, e_r, worst, worst32))
    # KP_TOL, unless the fp32 oracle's own teacher-forced steps are further than KP_TOL / 4 from fp64 at this shape (B = 130: 1.25e-4)
    tol = max(KP_TOL, 4 * worst32)
    assert worst < tol and e_r1 < tol
    assert e_c < max(KP_TOL, 4 * e_c32)
    assert torch.isfinite(out["keypoints_gen"]).all() and torch.isfinite(rk).all() and torch.isfinite(rh).all()


def test_rollout_graph_and_mid_kernel_are_bit_identical_at_64():
    """B = 64, the largest batch of the prior mid kernel and the captured rollout graph: generate and rollout (graph replayed twice)
    against contexts without the graph (NM355_VRNN_GRAPH=0) and without the mid kernel (NM355_VRNN_MID=0), bit for bit"""
    B, Tc, Tt = 64, 5, 20
    o, sd, order, parents, aff, kp, ep, er = V.generate_inputs(B)
    res = {}
    for name, env in (("default", {}), ("no-graph", {"NM355_VRNN_GRAPH": "0"}), ("no-mid", {"NM355_VRNN_MID": "0"})):
        d = _net(o, sd, aff, parents, V.GEN_SEEDS[0], env, fresh=True).dyna_module
        with torch.no_grad():
            g = d.generate(kp.cuda(), aff.cuda(), Ttot=Tt, Tcond=Tc, eps_post=ep.cuda(), eps_prior=er.cuda())
            off = d.get_offset(kp.cuda())
            h = (torch.randn(B, o.nhidden_kypt, generator=torch.Generator().manual_seed(3)) * 0.3).cuda()
            r1 = d.rollout(h, off, er.cuda())
            r2 = d.rollout(h, off, er.cuda())
            torch.cuda.synchronize()
        res[name] = (g["keypoints_cond"], g["keypoints_gen"], r1[0], r1[1], r2[0], r2[1])
    for name in ("no-graph", "no-mid"):
        for i, (a, b) in enumerate(zip(res["default"], res[name])):
            assert torch.equal(a, b), (name, i)
    d0 = res["default"]
    assert torch.equal(d0[2], d0[4]) and torch.equal(d0[3], d0[5])
    assert torch.isfinite(d0[1]).all()


# ---- the learner's Adam launch -----------------------------------------------------------------------------------------------------
def test_adam_multi_at_chunk_boundaries_vs_fp64():
    """nm_adam_step_multi / _ok on tensors of 1, 27, 4095, 4096, 4097 and 3 * 4096 + 5 elements (ADAM_CHUNK = 4096 per workgroup, items
    located by a binary search over their first chunks): torch.optim.Adam's formula with bias corrections in fp64 at steps 1, 2 and 7;
    ok = 0 leaves parameters and both moments bitwise unchanged, ok = null and ok = 1 update them identically"""
    o, sd, order, parents, aff = _model(24, 104)
    eng = _net(o, sd, aff, parents, 104)._engine
    sizes = [1, 27, 4095, 4096, 4097, 3 * 4096 + 5]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    g = torch.Generator().manual_seed(11)
    p = [torch.randn(n, generator=g).cuda() for n in sizes]
    m = [torch.zeros(n).cuda() for n in sizes]
    v = [torch.zeros(n).cuda() for n in sizes]
    p64 = [t.cpu().double() for t in p]
    m64 = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    v64 = [torch.zeros(n, dtype=torch.float64) for n in sizes]
    n = len(sizes)
    arr = lambda ts: (C.c_void_p * n)(*[_lib.ptr(t) for t in ts])
    numels = (C.c_int64 * n)(*sizes)
    for step in range(1, 8):
        grads = [torch.randn(k, generator=g) * (10.0 ** (i % 3 - 1)) for i, k in enumerate(sizes)]
        gd = [t.cuda() for t in grads]
        eng.call("nm_adam_step_multi", arr(p), arr(gd), arr(m), arr(v), numels, n, step, lr, b1, b2, eps)
        # the formula in fp64 on the hyper-parameters the C ABI receives (float: 0.999f is 0.99900001, so 1 - beta2 differs by 1.3e-5)
        f1, f2, fl, fe = (float(np.float32(x)) for x in (b1, b2, lr, eps))
        bc1, bc2 = 1 - f1 ** step, 1 - f2 ** step
        for i in range(n):
            gg = grads[i].double()
            m64[i] = f1 * m64[i] + (1 - f1) * gg
            v64[i] = f2 * v64[i] + (1 - f2) * gg * gg
            p64[i] = p64[i] - fl / bc1 * m64[i] / (v64[i].sqrt() / bc2 ** 0.5 + fe)
        torch.cuda.synchronize()
        if step in (1, 2, 7):
            for i in range(n):
                for what, got, want in (("param", p[i], p64[i]), ("exp_avg", m[i], m64[i]), ("exp_avg_sq", v[i], v64[i])):
                    e = _err(got, want) / max(want.abs().max().item(), 1e-30)
                    assert e <= 1e-6, (step, sizes[i], what, e)
    # the device-side skip flag
    grads = [torch.randn(k, generator=g).cuda() for k in sizes]
    state = [[t.clone() for t in ts] for ts in (p, m, v)]
    outs = {}
    for name, ok in (("null", None), ("one", torch.ones((), device="cuda")), ("zero", torch.zeros((), device="cuda"))):
        pp, mm, vv = ([t.clone() for t in ts] for ts in state)
        eng.call("nm_adam_step_multi_ok", arr(pp), arr(grads), arr(mm), arr(vv), numels, n, 8, lr, b1, b2, eps, _lib.ptr(ok) if ok is not None else None)
        torch.cuda.synchronize()
        outs[name] = (pp, mm, vv)
    for j in range(3):
        for i in range(n):
            assert torch.equal(outs["zero"][j][i], state[j][i]), ("ok = 0 changed", j, sizes[i])
            assert torch.equal(outs["one"][j][i], outs["null"][j][i]), ("ok = 1 differs from ok = null", j, sizes[i])
            assert not torch.equal(outs["null"][j][i], state[j][i]), ("ok = null did not update", j, sizes[i])
