"""Op-level parity of the backward kernels (detector-mode training): each HIP kernel family, called
through the C ABI, against torch autograd of the same ATen CPU op the reference trains with (train.py:388-404).
Tolerance 2e-5 relative to the gradient's max magnitude, as for the forward ops."""
import pytest
import torch
import torch.nn.functional as F

from test_ops_gpu import ctx, to_cl, from_cl, relerr, dev  # noqa: F401  (ctx is a fixture)

pytestmark = pytest.mark.gpu

REL = 2e-5

BWD_CASES = [
    # Cin, Cout, ks, stride, pad, size, N, prologue, up2, dgrad_channels
    (32, 32, 3, 1, 1, 16, 2, True, False, 32),
    (64, 32, 3, 1, 1, 12, 3, True, False, 64),
    (128, 64, 3, 1, 1, 8, 2, False, False, 128),
    (48, 72, 3, 1, 1, 4, 3, True, False, 48),
    (72, 72, 3, 1, 1, 2, 3, False, False, 72),
    (72, 48, 3, 1, 1, 5, 2, True, False, 72),
    (64, 128, 1, 1, 0, 8, 2, False, False, 64),
    (128, 24, 1, 1, 0, 8, 2, True, False, 128),
    (179, 128, 1, 1, 0, 6, 2, False, False, 176),
    (32, 32, 2, 2, 0, 16, 2, True, False, 32),
    (48, 48, 2, 2, 0, 5, 2, False, False, 48),
    (64, 64, 2, 2, 0, 8, 3, True, False, 64),
    (128, 64, 3, 1, 1, 6, 2, True, True, 128),
    (64, 32, 3, 1, 1, 8, 2, True, True, 64),
    (16, 32, 3, 1, 1, 5, 2, False, True, 16),
    (128, 128, 3, 1, 1, 8, 8, True, False, 128),
    (64, 128, 3, 1, 1, 8, 8, True, False, 64),
    (64, 128, 1, 1, 0, 8, 8, True, False, 64),
    # split-fp16 weight-gradient kernel (2x8x8 bricks): several bricks per workgroup, 2 / 4 / 8 tile pairs, ragged channel tiles
    (32, 32, 3, 1, 1, 16, 6, True, False, 32),
    (64, 64, 3, 1, 1, 16, 3, False, False, 64),
    (128, 64, 3, 1, 1, 8, 5, True, False, 128),
    (48, 72, 3, 1, 1, 8, 3, True, False, 48),
    (64, 32, 3, 1, 1, 8, 2, True, True, 64),
    # 1x1 convs on the all-tiles-per-workgroup weight-gradient kernel (voxels % 64 == 0): ragged channel counts, pending GroupNorm
    (179, 128, 1, 1, 0, 8, 2, False, False, 176),
    (48, 72, 1, 1, 0, 8, 3, True, False, 48),
    (72, 48, 1, 1, 0, 4, 5, True, False, 72),
    # fused-upsample layers big enough for the LDS-tiled upsample adjoint (coarse extents whole 2x4x8 bricks, borders on every side)
    (64, 32, 3, 1, 1, 16, 2, True, True, 64),
    (32, 32, 3, 1, 1, 16, 3, False, True, 32),
    # pool data gradient on the LDS-weight transposed-conv kernel (>= 65536 coarse voxels)
    (32, 32, 2, 2, 0, 32, 5, True, False, 32),
    (64, 64, 2, 2, 0, 32, 3, False, False, 64),
    # k2 s2 weight gradient on the f16 matrix cores (wgrad16k2_kernel: coarse (y, x) extents whole 8 x 8 bricks): four dY channel tiles,
    # ragged channel tiles on both sides, a non-cubic brick count
    (64, 128, 2, 2, 0, 16, 2, True, False, 64),
    (48, 72, 2, 2, 0, 16, 3, True, False, 48),
    (96, 40, 2, 2, 0, 16, 2, False, False, 96),
    # hourglass floor of a 32^3 grid: 1^3 and 2^3 volumes
    (72, 72, 3, 1, 1, 1, 8, True, False, 72),
    (48, 72, 1, 1, 0, 1, 8, False, False, 48),
    (48, 48, 2, 2, 0, 2, 8, True, False, 48),
    (32, 32, 2, 2, 0, 4, 8, True, False, 32),
    (32, 48, 3, 1, 1, 2, 8, True, False, 32),
]


F16_REL = 3e-3   # conv mode 3: gradients from operands rounded to fp16 (11 significant bits), fp32 accumulation


@pytest.mark.parametrize("mode", [0, 1, 3], ids=["fp32mfma", "split16", "f16"])
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "ci%d_co%d_k%d_s%d_d%d%s" % (c[0], c[1], c[2], c[3], c[5], "_up" if c[8] else ""))
def test_conv3d_backward(ctx, case, mode):
    from neural_marionette_amd import _lib
    _lib.check(ctx.lib.nm_set_conv_mode(ctx.handle, mode), "set_conv_mode")
    Cin, Cout, ks, stride, pad, size, N, prologue, up2, csel = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    dims = (size, size, size)
    x = torch.randn(N, Cin, *dims, generator=g)
    w = (torch.randn(Cout, Cin, ks, ks, ks, generator=g) / (Cin * ks ** 3) ** 0.5).requires_grad_(True)
    b = (torch.randn(Cout, generator=g) * 0.1).requires_grad_(True)
    cp = (Cin + 7) // 8 * 8
    if prologue:
        sc = torch.rand(N, Cin, generator=g) + 0.5
        sh = torch.randn(N, Cin, generator=g) * 0.3
        a = F.leaky_relu(x * sc[:, :, None, None, None] + sh[:, :, None, None, None], 0.01)
        scp = torch.zeros(N, cp); scp[:, :Cin] = sc
        shp = torch.zeros(N, cp); shp[:, :Cin] = sh
        slope = 0.01
    else:
        a, scp, shp, slope = x.clone(), None, None, 1.0
    a = a.detach().requires_grad_(True)
    inp = F.interpolate(a, scale_factor=2, mode="trilinear", align_corners=False) if up2 else a
    y = F.conv3d(inp, w, b, stride=stride, padding=pad)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    d_in = torch.full((N, *dims, csel), float("nan")).cuda()
    d_w = torch.full(w.shape, float("nan")).cuda()
    d_b = torch.full((Cout,), float("nan")).cuda()
    xd, wd, scd, shd, dyd = to_cl(x), dev(w.detach()), dev(scp), dev(shp), to_cl(dy, Cout)
    _lib.check(ctx.lib.nm_op_conv3d_backward(ctx.handle, _lib.ptr(xd), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), slope,
                                             _lib.ptr(wd), Cout, ks, stride, pad, int(up2), _lib.ptr(dyd), _lib.ptr(d_in), csel,
                                             _lib.ptr(d_w), _lib.ptr(d_b)), "op_conv3d_backward")
    torch.cuda.synchronize()
    for name, got, ref in (("d_weight", d_w.cpu(), w.grad), ("d_bias", d_b.cpu(), b.grad),
                           ("d_in", from_cl(d_in, csel), a.grad[:, :csel])):
        assert torch.isfinite(got).all(), f"{name}: unwritten / non-finite"
        e = relerr(got, ref)
        if e >= (F16_REL if mode == 3 else REL): _lib.check(ctx.lib.nm_set_conv_mode(ctx.handle, 1), "set_conv_mode")
        assert e < (F16_REL if mode == 3 else REL), f"{name} rel err {e:.3e}"
    _lib.check(ctx.lib.nm_set_conv_mode(ctx.handle, 1), "set_conv_mode")


# need: the plan's ws_floats = slots x tile pairs x tap groups x 1024 (wgrad16z: 2 (frame, y, x) columns x 1 x 27; wgrad16k2: 16 bricks x 6 x 8)
@pytest.mark.parametrize("case,need", [((32, 32, 3, 1, 1, 8, 2, True, False, 32), 2 * 27 * 1024), ((48, 72, 2, 2, 0, 16, 2, True, False, 48), 16 * 6 * 8 * 1024)],
                         ids=["wgrad16z", "wgrad16k2"])
def test_conv3d_backward_refuses_a_short_workspace(ctx, case, need, monkeypatch):
    """nm_launch_wgrad is told what its caller reserved and refuses, before any launch, a plan that needs more: with the op's figure
    patched to one float less than the plan's need (NM355_TEST_WGRAD_WS, read per call) the call returns NM_ERR_INTERNAL and leaves the
    outputs untouched; told exactly the need, and then unpatched, the same context computes the gradients as test_conv3d_backward holds them."""
    from neural_marionette_amd import _lib
    Cin, Cout, ks, stride, pad, size, N, _, _, csel = case
    O = (size + 2 * pad - ks) // stride + 1
    g = torch.Generator().manual_seed(3)
    xd = torch.randn(N, size, size, size, Cin, generator=g).cuda()
    wd = torch.randn(Cout, Cin, ks, ks, ks, generator=g).cuda()
    dyd = torch.randn(N, O, O, O, Cout, generator=g).cuda()
    d_w = torch.full(wd.shape, float("nan")).cuda(); d_b = torch.full((Cout,), float("nan")).cuda()
    monkeypatch.setenv("NM355_TEST_WGRAD_WS", str(need - 1))
    rc = ctx.lib.nm_op_conv3d_backward(ctx.handle, _lib.ptr(xd), N, size, size, size, Cin, None, None, 1.0, _lib.ptr(wd), Cout, ks, stride, pad, 0,
                                       _lib.ptr(dyd), None, csel, _lib.ptr(d_w), _lib.ptr(d_b))
    torch.cuda.synchronize()
    msg = ctx.lib.nm_last_error().decode()
    print("rc %d: %s" % (rc, msg))
    assert rc == _lib.NM_ERR_INTERNAL and "needs %d floats of workspace, the caller reserved %d" % (need, need - 1) in msg
    assert torch.isnan(d_w).all() and torch.isnan(d_b).all(), "a kernel ran"
    monkeypatch.setenv("NM355_TEST_WGRAD_WS", str(need))
    test_conv3d_backward(ctx, case, 1)
    monkeypatch.delenv("NM355_TEST_WGRAD_WS")
    test_conv3d_backward(ctx, case, 1)


@pytest.mark.parametrize("sparse", [1, 2, 0], ids=["mfma-bricks", "gather", "dense"])
@pytest.mark.parametrize("Cout,G,N,frac", [(32, 16, 2, False), (64, 12, 3, False), (32, 32, 1, False), (64, 24, 5, True), (32, 40, 3, True),
                                             (48, 16, 2, False)])
def test_conv5_occ_backward(ctx, Cout, G, N, frac, sparse):
    from neural_marionette_amd import _lib
    g = torch.Generator().manual_seed(Cout * 7 + G)
    occ = (torch.rand(N, 1, G, G, G, generator=g) < 0.05).float()
    if frac:        # the clip-mean net sees fractional occupancy (kypt_detector.py:312)
        occ = occ * torch.rand(N, 1, G, G, G, generator=g)
    if G >= 24:     # one figure in the grid: most 4x8x8 bricks (and their halos) are empty - the brick-skipping path
        box = torch.zeros_like(occ); box[:, :, G // 3:G // 3 + 9, 5:G // 2, G // 2 - 3:G - 6] = 1.0
        occ = occ * box
    lin = torch.linspace(-1.0, 1.0, G)
    zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
    coords = torch.stack([zz, yy, xx])[None].expand(N, -1, -1, -1, -1)
    inp = torch.cat([occ, coords], dim=1)
    w = (torch.randn(Cout, 4, 5, 5, 5, generator=g) / 500 ** 0.5).requires_grad_(True)
    b = torch.zeros(Cout, requires_grad=True)
    y = F.conv3d(inp, w, b, padding=2)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    d_w = torch.full(w.shape, float("nan")).cuda(); d_b = torch.full((Cout,), float("nan")).cuda()
    occd, dyd = occ[:, 0].contiguous().cuda(), to_cl(dy, Cout)      # (named: the buffers must outlive the call)
    _lib.check(ctx.lib.nm_op_conv5_occ_backward(ctx.handle, _lib.ptr(occd), N, G, Cout, _lib.ptr(dyd),
                                                _lib.ptr(d_w), _lib.ptr(d_b), sparse), "op_conv5_occ_backward")
    torch.cuda.synchronize()
    assert relerr(d_w.cpu(), w.grad) < REL
    assert relerr(d_b.cpu(), b.grad) < REL


@pytest.mark.parametrize("Cin,Cout,size,outpad,prologue,N", [(72, 48, 1, 0, True, 8), (72, 48, 2, 0, True, 3), (48, 32, 4, 0, False, 2), (32, 64, 8, 0, True, 2),
                                                             (72, 48, 2, 1, True, 2), (48, 32, 5, 1, False, 2),
                                                             (128, 64, 8, 0, True, 3), (72, 48, 16, 0, False, 2)])      # (wgrad16k2_kernel, roles swapped)
def test_convT2_backward(ctx, Cin, Cout, size, outpad, prologue, N):
    from neural_marionette_amd import _lib
    g = torch.Generator().manual_seed(Cin * 3 + Cout + size + outpad)
    dims = (size, size, size)
    x = torch.randn(N, Cin, *dims, generator=g)
    w = (torch.randn(Cin, Cout, 2, 2, 2, generator=g) / (Cin * 8) ** 0.5).requires_grad_(True)
    b = (torch.randn(Cout, generator=g) * 0.1).requires_grad_(True)
    if prologue:
        sc = torch.rand(N, Cin, generator=g) + 0.5
        sh = torch.randn(N, Cin, generator=g) * 0.3
        a = F.leaky_relu(x * sc[:, :, None, None, None] + sh[:, :, None, None, None], 0.01)
        slope = 0.01
    else:
        a, sc, sh, slope = x.clone(), None, None, 1.0
    a = a.detach().requires_grad_(True)
    y = F.conv_transpose3d(a, w, b, stride=2, output_padding=outpad)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    d_in = torch.full((N, *dims, Cin), float("nan")).cuda()
    d_w = torch.full(w.shape, float("nan")).cuda(); d_b = torch.full((Cout,), float("nan")).cuda()
    xd, scd, shd, wd, dyd = to_cl(x), dev(sc), dev(sh), dev(w.detach()), to_cl(dy, Cout)
    _lib.check(ctx.lib.nm_op_convT2_backward(ctx.handle, _lib.ptr(xd), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), slope,
                                             _lib.ptr(wd), Cout, outpad, _lib.ptr(dyd), _lib.ptr(d_in),
                                             _lib.ptr(d_w), _lib.ptr(d_b)), "op_convT2_backward")
    torch.cuda.synchronize()
    assert relerr(d_w.cpu(), w.grad) < REL
    assert relerr(d_b.cpu(), b.grad) < REL
    assert relerr(from_cl(d_in, Cin), a.grad) < REL


@pytest.mark.parametrize("C,groups,size,N,slope", [(32, 2, 16, 2, 0.01), (64, 4, 8, 3, 0.01), (128, 8, 6, 2, 1.0), (72, 4, 2, 3, 0.01),
                                                   (48, 3, 5, 2, 1.0), (256, 16, 4, 1, 0.01), (72, 4, 1, 8, 0.01), (48, 3, 2, 8, 1.0)])
def test_gn_backward(ctx, C, groups, size, N, slope):
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
    _lib.check(ctx.lib.nm_op_gn_backward(ctx.handle, _lib.ptr(yd), N, V, C, groups, _lib.ptr(gd),
                                         _lib.ptr(bd), slope, _lib.ptr(dAd), _lib.ptr(dy), _lib.ptr(dg),
                                         _lib.ptr(db), _lib.ptr(dbias)), "op_gn_backward")
    torch.cuda.synchronize()
    assert relerr(from_cl(dy, C), y.grad) < REL
    assert relerr(dg.cpu(), gam.grad) < REL
    assert relerr(db.cpu(), bet.grad) < REL
    ref_bias = y.grad.sum(dim=(0, 2, 3, 4))
    assert (dbias.cpu() - ref_bias).abs().max().item() < REL * max(y.grad.abs().sum(dim=(0, 2, 3, 4)).max().item(), 1e-30)


def _fresh_ctx():
    from neural_marionette_amd import _lib
    cfg = _lib.NmConfig(device=0, grid_size=64, nkeypoints=24, nlatent=128, nhidden=512, nneighbor=2,
                        gaussian_sigma=1.5, sep_sigma=0.02, vol_fit_chamfer=1, use_graph_traj=1)
    c = _lib.Context(cfg)
    c.bind_stream()
    return c


class _switches:
    """NM355_* switches are read when a context is created and belong to it: a variant's parity run sets them around the creation of
    a fresh context, in this process (a child process per variant cost 6-8 s of interpreter + torch start-up each)."""
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


_K3_CASES = [c for c in BWD_CASES if c[2] == 3]


def test_conv3d_backward_valu_transposition_wgrad_variant():
    """The older weight-gradient kernel (wgrad16_kernel, VALU transposition): the path of the fp32-storage modes for more than 96
    frames and for a volume one brick deep, and the A/B partner of the default wgrad16z_kernel - NM355_WGRAD_TR=0 forces it for every
    call.  The k3 cases again on a context created with that switch."""
    with _switches({"NM355_WGRAD_TR": "0"}):
        c = _fresh_ctx()
    try:
        for case in _K3_CASES:
            test_conv3d_backward(c, case, 1)
    finally:
        c.close()


@pytest.mark.parametrize("env", [{"NM355_TAIL_RANK1": "0"}, {"NM355_GNB_APPLY4": "0", "NM355_DEFER_SUMS": "0"}, {"NM355_WGRAD_ASYNC": "0"},
                                 {"NM355_WGRAD_ASYNC": "2"}],
                         ids=["tail-gradient-tensor", "gnb-apply-and-sums-per-layer", "weight-gradients-in-the-main-stream",
                              "weight-gradients-enqueued-before-the-data-gradient"])
def test_conv3d_backward_older_kernel_variants(env, golden_dir):
    """The A/B partners of the round-3 defaults stay under parity, re-running the reference's gradient fixture G8 on a fresh network:
    the decoder tail's backward with its [F][G^3][32] gradient materialised (NM355_TAIL_RANK1=0), the GroupNorm backward with the
    one-voxel-at-a-time apply kernel and its gamma / beta / bias sums launched per layer, and the weight gradients inside the main
    stream's chain / enqueued on their own stream in front of the data gradient.  The switches are read when a context is created."""
    from test_train_detector_gpu import test_detector_gradients_vs_reference_fixture as g8
    with _switches(env):
        g8(golden_dir)
