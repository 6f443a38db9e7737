"""The detector past 64 and 96 frames in one call.

The reference trains on 24 clips of 10 frames (240 frames per step) and its demos run clips of 20 to 40 frames in batches; two limits
in the library sit just above what the rest of the suite runs (64 frames per network call, 8 frames per op-level backward call):

  FRAME_CHUNK = 64 (nm_net.hip): without a tape the per-frame encoder runs in chunks of 64 frames and the decoder in passes of
  64 / T whole clips, every pass with its own offsets into the table, the keypoints, the features, the first frames, the target, the
  reconstruction and the tail partials; the clip block is enqueued behind the second encoder chunk.

  96 frames (nm_wgrad_plan.h, W16_TAB_FRAMES): wgrad16z_kernel keeps a per-frame scale / shift table in LDS; above 96 frames the
  fp32-storage modes run wgrad16_kernel (as a volume one brick deep does at every frame count), and the 16-bit storage mode (conv
  mode 4) runs wgrad16z_kernel once per group of frames.

Op level: every kernel against torch CPU autograd of the same op in float64 (inputs drawn in fp32 and cast), at the project's own bounds
(2e-5 of the gradient's max magnitude in modes 0 and 1, 3e-3 in mode 3; torch's fp32 autograd is 1.2e-6 .. 3.1e-6 from fp64 at these
shapes, 520 frames included).  Network level: the CPU oracle on the whole batch for the inference passes; for the training gradient at
100 frames the multiplicity-weighted mean of two single-clip fp64 gradients (tests/test_many_frames_ref_cpu.py guards that identity).
Every test prints its measured worst error (DESIGN.md "Many frames" holds the table)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import ctx, to_cl, from_cl, relerr, dev  # noqa: F401  (ctx is a fixture)
from test_grad_ops_gpu import REL, F16_REL
from test_train_detector_gpu import AIST, TOL, _setup, _oracle_grads, _hip_grads, _compare
from test_network_gpu import KP_TOL, ACTS, PATHS, _net, _call, _err, _check_losses, _check_occupancy_set
from neural_marionette_amd import HotPathOptions, synth
from neural_marionette_amd.spec import DETECTOR_LOSS_KEYS
from oracle import nm_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
_REFS = {}


def _cached(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


# ---- 1. op-level backward at many frames -----------------------------------------------------------------------------------------
def _conv_bwd_ref(Cin, Cout, ks, stride, pad, dims, N, prologue, bf16_values=False):
    """Seeded fp32 inputs of y = conv3d(lrelu(x * scale + shift), w) + b with a scale / shift row per frame, and the float64 autograd
    gradients of the same values (computed once per shape and shared by the modes)."""
    def make():
        g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + 7 * N + dims[0] + 3 * ks)
        x = torch.randn(N, Cin, *dims, generator=g)
        w = torch.randn(Cout, Cin, ks, ks, ks, generator=g) / (Cin * ks ** 3) ** 0.5
        b = torch.randn(Cout, generator=g) * 0.1
        sc = sh = None
        if prologue:
            sc = torch.rand(N, Cin, generator=g) + 0.5             # distinct per frame: a wrong table row shows
            sh = torch.randn(N, Cin, generator=g) * 0.3
        od = tuple((d + 2 * pad - ks) // stride + 1 for d in dims)
        dy = torch.randn(N, Cout, *od, generator=g)
        if bf16_values:                                            # bfloat16-representable operands (16-bit storage parity)
            x, dy = x.to(BF).float(), (dy * 1e-3).to(BF).float()
        x64 = x.double()
        a = F.leaky_relu(x64 * sc.double()[:, :, None, None, None] + sh.double()[:, :, None, None, None], 0.01) if prologue else x64.clone()
        a.requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        F.conv3d(a, w64, b64, stride=stride, padding=pad).backward(dy.double())
        return dict(x=x, w=w, sc=sc, sh=sh, dy=dy, slope=0.01 if prologue else 1.0, d_w=w64.grad, d_b=b64.grad, d_a=a.grad)
    return _cached(("conv", Cin, Cout, ks, stride, pad, dims, N, prologue, bf16_values), make)


def _conv_bwd(c, shape, N, mode, prologue=True, what=""):
    """nm_op_conv3d_backward on context `c` in conv mode `mode` against the float64 reference: d_weight, d_bias and d_in, each relative to
    the gradient's max magnitude, outputs pre-filled with NaN.  shape = (Cin, Cout, ks, stride, pad, dims)."""
    from neural_marionette_amd import _lib
    Cin, Cout, ks, stride, pad, dims = shape
    r = _conv_bwd_ref(Cin, Cout, ks, stride, pad, dims, N, prologue)
    bound = F16_REL if mode == 3 else REL
    d_in = torch.full((N, *dims, Cin), float("nan")).cuda()
    d_w = torch.full(r["w"].shape, float("nan")).cuda()
    d_b = torch.full((Cout,), float("nan")).cuda()
    xd, wd, scd, shd, dyd = to_cl(r["x"]), dev(r["w"]), dev(r["sc"]), dev(r["sh"]), to_cl(r["dy"], Cout)
    _lib.check(c.lib.nm_set_conv_mode(c.handle, mode), "set_conv_mode")
    try:
        _lib.check(c.lib.nm_op_conv3d_backward(c.handle, _lib.ptr(xd), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), r["slope"],
                                               _lib.ptr(wd), Cout, ks, stride, pad, 0, _lib.ptr(dyd), _lib.ptr(d_in), Cin,
                                               _lib.ptr(d_w), _lib.ptr(d_b)), "op_conv3d_backward")
        torch.cuda.synchronize()
    finally:
        _lib.check(c.lib.nm_set_conv_mode(c.handle, 1), "set_conv_mode")
    got = (("d_weight", d_w.cpu(), r["d_w"]), ("d_bias", d_b.cpu(), r["d_b"]), ("d_in", from_cl(d_in, Cin), r["d_a"]))
    errs = {}
    for name, g, ref in got:
        assert torch.isfinite(g).all(), f"{name}: unwritten / non-finite"
        errs[name] = relerr(g.double(), ref)
    print("conv3d backward %s ci%d co%d k%d s%d %s N=%d mode %d%s: d_weight %.2e d_bias %.2e d_in %.2e (bound %.0e)"
          % (what, Cin, Cout, ks, stride, "x".join(map(str, dims)), N, mode, "" if prologue else " no prologue",
             errs["d_weight"], errs["d_bias"], errs["d_in"], bound))
    for name, e in errs.items():
        assert e < bound, f"{name} rel err {e:.3e}"
    return errs


K3 = (32, 32, 3, 1, 1, (4, 8, 8))
K3_RAGGED = (48, 72, 3, 1, 1, (4, 8, 8))
K3_NBZ1 = (32, 32, 3, 1, 1, (2, 8, 8))
K1 = (64, 128, 1, 1, 0, (4, 4, 4))
K2 = (64, 128, 2, 2, 0, (16, 16, 16))

MANY_FRAMES = (
    # the per-frame table at its last row (wgrad16z_kernel) and one frame later (wgrad16_kernel); mode 0: the generic kernel
    [("a", K3, N, m, True) for N in (96, 97) for m in (0, 1, 3)] +
    # the same with 3 x 2 ragged tile pairs
    [("b", K3_RAGGED, N, m, True) for N in (96, 97) for m in (1, 3)] +
    # nbz = 1 (no column for wgrad16z_kernel to walk): wgrad16_kernel at both counts, in both product forms
    [("c", K3_NBZ1, N, m, True) for N in (96, 97) for m in (1, 3)] +
    # the reference's default frame count (24 clips of 10 frames)
    [("d", K3, 240, m, False) for m in (1, 3)] +
    # generic wgrad_kernel: 520 bricks over its 512 workgroup slots - one workgroup walks several bricks, the last ones ragged
    [("e", K3, 520, 0, True)] +
    # wgrad_k1_kernel: 520 bricks over K1_WGS = 512
    [("f", K1, 520, m, True) for m in (0, 1)] +
    # wgrad16k2_kernel: 33 * 8 = 264 work items over 512 / n_tiles = 256
    [("g", K2, 33, m, True) for m in (1, 3)]
)


@pytest.mark.parametrize("case", MANY_FRAMES, ids=lambda c: "%s_ci%d_co%d_k%d_d%d_N%d_mode%d" % (c[0], c[1][0], c[1][1], c[1][2], c[1][5][0], c[2], c[3]))
def test_conv3d_backward_many_frames(ctx, case):
    tag, shape, N, mode, prologue = case
    _conv_bwd(ctx, shape, N, mode, prologue, what="(%s)" % tag)


@pytest.mark.parametrize("C,groups,size,N,slope", [(32, 2, 4, 100, 0.01), (72, 4, 2, 130, 1.0)])
def test_gn_backward_many_frames(ctx, C, groups, size, N, slope):
    """nm_op_gn_backward at 100 / 130 frames; reference and bounds as test_grad_ops_gpu.test_gn_backward."""
    from neural_marionette_amd import _lib
    g = torch.Generator().manual_seed(C + size)
    y = (torch.randn(N, C, size, size, size, generator=g) * 1.5 + 0.3).requires_grad_(True)
    gam = (torch.rand(C, generator=g) + 0.5).requires_grad_(True)
    bet = (torch.randn(C, generator=g) * 0.2).requires_grad_(True)
    out = F.leaky_relu(F.group_norm(y, groups, gam, bet, 1e-5), slope)
    dA = torch.randn(out.shape, generator=g)
    out.backward(dA)
    V = size ** 3
    dy = torch.full((N, size, size, size, C), float("nan")).cuda()
    dg = torch.zeros(C).cuda(); db = torch.zeros(C).cuda(); dbias = torch.zeros(C).cuda()
    yd, gd, bd, dAd = to_cl(y.detach(), C), dev(gam.detach()), dev(bet.detach()), to_cl(dA, C)
    _lib.check(ctx.lib.nm_op_gn_backward(ctx.handle, _lib.ptr(yd), N, V, C, groups, _lib.ptr(gd), _lib.ptr(bd), slope, _lib.ptr(dAd),
                                         _lib.ptr(dy), _lib.ptr(dg), _lib.ptr(db), _lib.ptr(dbias)), "op_gn_backward")
    torch.cuda.synchronize()
    ref_bias = y.grad.sum(dim=(0, 2, 3, 4))
    e = (relerr(from_cl(dy, C), y.grad), relerr(dg.cpu(), gam.grad), relerr(db.cpu(), bet.grad),
         (dbias.cpu() - ref_bias).abs().max().item() / max(y.grad.abs().sum(dim=(0, 2, 3, 4)).max().item(), 1e-30))
    print("gn backward C=%d groups=%d %d^3 N=%d: dy %.2e dgamma %.2e dbeta %.2e dbias %.2e (bound %.0e)" % (C, groups, size, N, *e, REL))
    assert torch.isfinite(dy).all()
    assert max(e) < REL, e


@pytest.mark.parametrize("sparse", [1, 2, 0], ids=["mfma-bricks", "gather", "dense"])
def test_conv5_occ_backward_many_frames(ctx, sparse):
    """First-layer weight gradient at 70 frames (the sparse workspace scales with N x chunks); reference and bounds as
    test_grad_ops_gpu.test_conv5_occ_backward."""
    from neural_marionette_amd import _lib
    Cout, G, N = 32, 16, 70

    def make():
        g = torch.Generator().manual_seed(Cout * 7 + G + N)
        occ = (torch.rand(N, 1, G, G, G, generator=g) < 0.05).float()
        lin = torch.linspace(-1.0, 1.0, G)
        zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
        coords = torch.stack([zz, yy, xx])[None].expand(N, -1, -1, -1, -1)
        w = (torch.randn(Cout, 4, 5, 5, 5, generator=g) / 500 ** 0.5).requires_grad_(True)
        b = torch.zeros(Cout, requires_grad=True)
        y = F.conv3d(torch.cat([occ, coords], dim=1), w, b, padding=2)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        return occ, dy, w.grad, b.grad
    occ, dy, rw, rb = _cached(("conv5occ",), make)
    d_w = torch.full(rw.shape, float("nan")).cuda(); d_b = torch.full((Cout,), float("nan")).cuda()
    occd, dyd = occ[:, 0].contiguous().cuda(), to_cl(dy, Cout)
    _lib.check(ctx.lib.nm_op_conv5_occ_backward(ctx.handle, _lib.ptr(occd), N, G, Cout, _lib.ptr(dyd), _lib.ptr(d_w), _lib.ptr(d_b), sparse),
               "op_conv5_occ_backward")
    torch.cuda.synchronize()
    ew, eb = relerr(d_w.cpu(), rw), relerr(d_b.cpu(), rb)
    print("conv5 occ backward Cout=%d G=%d N=%d sparse_occ=%d: d_weight %.2e d_bias %.2e (bound %.0e)" % (Cout, G, N, sparse, ew, eb, REL))
    assert torch.isfinite(d_w).all() and torch.isfinite(d_b).all()
    assert ew < REL and eb < REL


# ---- 2. 16-bit storage past 96 frames ----------------------------------------------------------------------------------------------
def _set(c, mode, ih, oh):
    from neural_marionette_amd import _lib
    _lib.check(c.lib.nm_set_conv_mode(c.handle, mode), "set_conv_mode")
    _lib.check(c.lib.nm_op_set_storage16(c.handle, ih, oh), "op_set_storage16")


@pytest.mark.parametrize("Cin,Cout,N", [(32, 32, 96), (32, 32, 97), (32, 32, 240), (64, 64, 97)])
def test_conv3d_weight_gradient_storage16_many_frames(ctx, Cin, Cout, N):
    """Conv mode 4, both operands bfloat16, d_in = NULL (weight and bias gradients only).  96 frames: one wgrad16z launch, bit-identical
    to mode 3 with fp32 storage on the same bfloat16-representable values.  Above: wgrad16z over groups of at most 96 frames, each on
    its own partial-sum slots, one fixed-order reduce - within F16_REL of float64 (mode 3 runs wgrad16_kernel there: another summation
    order, so no bit identity), and two runs bit-identical."""
    from neural_marionette_amd import _lib
    dims = (4, 8, 8)
    r = _conv_bwd_ref(Cin, Cout, 3, 1, 1, dims, N, True, bf16_values=True)
    x32, dy32, wd, scd, shd = to_cl(r["x"]), to_cl(r["dy"]), dev(r["w"]), dev(r["sc"]), dev(r["sh"])

    def run(mode, h):
        _set(ctx, mode, h, h)
        xin, dyin = (x32.to(BF), dy32.to(BF)) if h else (x32, dy32)
        dw = torch.full(r["w"].shape, float("nan")).cuda(); db = torch.full((Cout,), float("nan")).cuda()
        _lib.check(ctx.lib.nm_op_conv3d_backward(ctx.handle, _lib.ptr(xin), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), 0.01, _lib.ptr(wd), Cout,
                                                 3, 1, 1, 0, _lib.ptr(dyin), None, Cin, _lib.ptr(dw), _lib.ptr(db)), "op_conv3d_backward")
        torch.cuda.synchronize()
        return dw, db
    try:
        r_w, r_b = run(3, 0)
        g_w, g_b = run(4, 1)
        g_w2, g_b2 = run(4, 1)
    finally:
        _set(ctx, 1, 0, 0)
    assert torch.isfinite(g_w).all() and torch.isfinite(g_b).all()
    ew, eb = relerr(g_w.cpu().double(), r["d_w"]), relerr(g_b.cpu().double(), r["d_b"])
    print("16-bit storage weight gradient ci%d co%d N=%d: d_weight %.2e d_bias %.2e from float64 (bound %.0e); mode 3 with fp32 storage %.2e; "
          "largest difference to it %.2e" % (Cin, Cout, N, ew, eb, F16_REL, relerr(r_w.cpu().double(), r["d_w"]), (g_w - r_w).abs().max().item()))
    assert torch.equal(g_w, g_w2) and torch.equal(g_b, g_b2), "two runs differ"
    if N <= 96:
        assert torch.equal(g_b, r_b), "bias gradient"
        assert torch.equal(g_w, r_w), "weight gradient: max diff %.3e" % (g_w - r_w).abs().max().item()
    assert ew < F16_REL and eb < F16_REL, (ew, eb)


# ---- 3. network level ----------------------------------------------------------------------------------------------------------------
def _network(B, T):
    """32^3 (the smallest grid the network takes), seeded weights, B DISTINCT clips (with identical clips a pass that read clip 0's data
    instead of clip b0's would pass) and the CPU oracle's detector on the whole batch."""
    def make():
        o = HotPathOptions(grid_size=32)
        sd = synth.make_state_dict(o, seed=40 + B + T, variant="peaky")
        vox = synth.figure_clip(B, T, 32, seed=50 + B + T)
        assert all(not torch.equal(vox[0], vox[b]) for b in range(1, B))
        with torch.no_grad():
            ref = O.detector_forward(sd, o, vox)
        return o, sd, vox, ref
    return _cached(("net", B, T), make)


def _check_detector(out, ref, what):
    e_kp = _err(out["keypoints"], ref["keypoints"])
    e_hm, e_ff = _err(out["heatmaps"], ref["heatmaps"]), _err(out["first_feature"], ref["first_feature"])
    print("%s: keypoints %.3e heatmaps %.3e first_feature %.3e" % (what, e_kp, e_hm, e_ff))
    assert e_kp < KP_TOL
    assert e_hm < 1e-4 * max(1.0, float(ref["heatmaps"].abs().max()))
    assert e_ff < 1e-4 * max(1.0, float(ref["first_feature"].abs().max()))
    _check_occupancy_set(out["recon"], ref["recon"], what=what)
    _check_losses(out, [float(ref[k]) for k in DETECTOR_LOSS_KEYS], ref_kp=ref["keypoints"])


INFERENCE_PASSES = [
    (7, 10, "split16"), (7, 10, "fp32"),      # encoder chunks 64 + 6; decoder passes of 6 + 1 clips
    (13, 10, "split16"),                      # three encoder chunks (the clip block behind the second); decoder passes 6 + 6 + 1
    (2, 33, "split16"),                       # one clip per decoder pass; encoder chunks 64 + 2, cut inside a clip
    (1, 65, "split16"),                       # one clip longer than a pass
]


@pytest.mark.parametrize("B,T,mode", INFERENCE_PASSES)
def test_inference_in_several_passes_vs_oracle(B, T, mode):
    o, sd, vox, ref = _network(B, T)
    net = _net(o, sd, mode)
    with torch.no_grad():
        out = net(vox.cuda(), {"detector": True, "learner": False})
    torch.cuda.synchronize()
    _check_detector(out, ref, "inference B=%d T=%d (%s)" % (B, T, mode))


def test_inference_in_several_passes_starts_the_vrnn():
    """nm_forward_fused at B = 7, T = 10: the VRNN starts from inside a multi-pass call.  The detector's side against the oracle; the
    VRNN outputs equal a stand-alone encode on the call's own keypoints and affinity."""
    B, T, S = 7, 10, 10
    o, sd, vox, ref = _network(B, T)
    net = _net(o, sd)
    eps = synth.make_eps((T, S, B, o.nlatent_kypt), seed=8).cuda()
    with torch.no_grad():
        net(vox[:1, :3].cuda(), ACTS, eps=eps[:3, :, :1].contiguous())          # (the first call builds the tree; later ones take the fused forward)
        out = net(vox.cuda(), ACTS, eps=eps)
        enc = net.dyna_module.encode(out["keypoints"], out["affinity"], SAMPLE_NUM=S, eps=eps)
    torch.cuda.synchronize()
    _check_detector(out, ref, "fused forward B=%d T=%d" % (B, T))
    for k in ("kypt_recon", "R", "z_kypts", "h_kypts", "best_idx", "kl_kypt", "kypt_recon_loss"):
        assert torch.isfinite(out[k].float()).all(), k
        assert torch.equal(out[k], enc[k]), k


def test_training_forward_at_70_frames_vs_oracle():
    """The training forward (tape: one pass over all 70 frames) on the same batch."""
    B, T = 7, 10
    o, sd, vox, ref = _network(B, T)
    net = _net(o, sd)
    out = _call(PATHS[0], net, vox.cuda(), {"detector": True, "learner": False})
    torch.cuda.synchronize()
    assert out["recon_loss"].requires_grad
    _check_detector({k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}, ref, "training forward B=%d T=%d" % (B, T))


def test_decode_from_dyna_in_several_passes_vs_oracle():
    """decode_from_dyna with B = 2, Tg = 65 (one clip per decoder pass, each longer than FRAME_CHUNK), as test_decode_from_dyna_unit_vs_oracle."""
    o = HotPathOptions(grid_size=32)
    sd = synth.make_state_dict(o, seed=37, variant="peaky")
    net = _net(o, sd)
    B, T, Tg = 2, 3, 65
    vox = synth.figure_clip(B, T, 32, seed=12)
    with torch.no_grad():
        det = O.detector_forward(sd, o, vox)
        gen = torch.Generator().manual_seed(5)
        kp = det["keypoints"][:, :1].expand(-1, Tg, -1, -1).clone()
        kp[..., :3] += 0.05 * torch.randn(B, Tg, o.nkeypoints, 3, generator=gen)          # keypoints the detector never produced, distinct per frame
        kp[..., 3] = (kp[..., 3] * (1 + 0.2 * torch.randn(B, Tg, o.nkeypoints, generator=gen))).clamp(0, 1)
        ref = O.decode_from_keypoints(sd, o, kp, det["first_feature"], vox[:, 0])
    got = net.kypt_detector.decode_from_dyna(kp.cuda(), det["first_feature"].cuda(), vox[:, 0].cuda())["gen"]
    torch.cuda.synchronize()
    assert got.shape == (B, Tg, 1, 32, 32, 32)
    e = _err(got, ref)
    margin = (ref - 0.5).abs()
    mism = (((got.cpu() >= 0.5) != (ref >= 0.5)) & (margin > 1e-4)).sum().item()
    print("decode_from_dyna B=%d Tg=%d: recon err %.3e, occupancy mismatches away from threshold %d" % (B, Tg, e, mism))
    assert e < 1e-3 and mism == 0


# 13 x A, 12 x B in an irregular order: 25 clips of 4 frames, 100 frames
ORDER_100 = "A B B A B A A B A B B A A B A B B A A B A B A B A".split()


def _training_reference():
    """(options, weights, the 100-frame batch, fp64 loss, fp64 gradient): every loss is a mean over clips and GroupNorm is per frame, so
    the batch gradient is the multiplicity-weighted mean of the single-clip gradients (checked with the fp64 oracle itself in
    tests/test_many_frames_ref_cpu.py; at 32^3, T = 4 and the batch [A, B, B, A, B] the two agree to 4.7e-16 whole-gradient L2)."""
    def make():
        o, sd, vox = _setup(seed=11)
        nA, nB = ORDER_100.count("A"), ORDER_100.count("B")
        assert (nA, nB) == (13, 12)
        batch = torch.stack([vox[0] if s == "A" else vox[1] for s in ORDER_100]).contiguous()
        l_a, g_a, _ = _oracle_grads(o, sd, vox[0:1].contiguous(), AIST, double=True)
        l_b, g_b, _ = _oracle_grads(o, sd, vox[1:2].contiguous(), AIST, double=True)
        ref = {k: (nA * g_a[k] + nB * g_b[k]) / (nA + nB) for k in g_a}
        return o, sd, batch, (nA * l_a + nB * l_b) / (nA + nB), ref
    return _cached(("train100",), make)


def _l2_and_worst(got, ref, floor):
    """whole-gradient relative L2 distance, and the worst per-tensor relative L2 over the tensors whose largest entry exceeds floor x the
    largest gradient entry"""
    gmax = max(r.abs().max().item() for r in ref.values())
    num = den = 0.0
    worst = ("", 0.0)
    for k, r in ref.items():
        g, r = got[k].double(), r.double()
        assert torch.isfinite(g).all(), k
        num += ((g - r) ** 2).sum().item(); den += (r ** 2).sum().item()
        if r.abs().max().item() > floor * gmax:
            rel = ((g - r).norm() / r.norm()).item()
            if rel > worst[1]:
                worst = (k, rel)
    return (num / den) ** 0.5, worst


@pytest.mark.parametrize("mode", ["split16", "f16", "bf16"])
def test_training_gradient_at_100_frames(mode):
    """B = 25, T = 4 at 32^3 in one training step: every k3 weight gradient of a 32^3 / 16^3 / 8^3 layer sums over 100 frames (wgrad16_kernel
    in the fp32-storage modes; 'bf16' with the default storage threshold keeps the 32^3 layers in bfloat16: wgrad16z_kernel over two
    groups of 50 frames).  Bounds: the modes' stated ones (test_detector_gradients_vs_oracle_autograd, test_detector_gradients_f16_mode,
    test_detector_gradients_bf16_storage_vs_fp64_oracle)."""
    o, sd, batch, ref_loss, ref = _training_reference()
    loss, got, _ = _hip_grads(o, sd, batch, AIST, mode=mode)
    rel_loss = abs(loss - ref_loss) / max(1.0, abs(ref_loss))
    if mode == "split16":
        print("100 frames, split16: loss %.6f (fp64 %.6f, rel %.2e; bound 2e-5)" % (loss, ref_loss, rel_loss))
        assert rel_loss <= 2e-5, (loss, ref_loss)
        _compare(ref, got, TOL)
        return
    b_loss, b_l2, b_tensor, floor = (5e-4, 2e-2, 0.25, 1e-6) if mode == "f16" else (2e-3, 4e-2, 0.30, 1e-4)
    l2, worst = _l2_and_worst(got, ref, floor)
    print("100 frames, %s: loss %.6f (fp64 %.6f, rel %.2e; bound %.0e); whole-gradient L2 %.3e (bound %.0e); worst tensor %.3f at %s (bound %.2f)"
          % (mode, loss, ref_loss, rel_loss, b_loss, l2, b_l2, worst[1], worst[0], b_tensor))
    if mode == "bf16":
        loss2, got2, _ = _hip_grads(o, sd, batch, AIST, mode=mode)
        assert loss == loss2
        for k, v in got.items():
            assert torch.equal(v, got2[k]), f"{k}: two evaluations differ"
    assert rel_loss <= b_loss, (loss, ref_loss)
    assert l2 < b_l2, l2
    assert worst[1] < b_tensor, worst
