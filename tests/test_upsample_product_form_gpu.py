"""Upsample(x2, trilinear, align_corners=False) -> Conv3d(k3, s1, p1) in the product-then-interpolate form (nm_up2c.hip,
conv_up2y_kernel).

Trilinear upsampling acts per channel and the conv's channel contraction is linear, so the two commute: the products can be taken
with the coarse tensor, once per COARSE voxel and tap, and interpolated afterwards.  The identity is asserted on the CPU in fp64
(all three axes at once, and along y alone with the other two axes left as they are - the form the kernel uses); the kernel is
checked through nm_op_conv3d(..., up2=1) in the split-fp16 mode against ATen's interpolate -> conv3d -> group_norm at the 2e-5 of
test_ops_gpu.py, separately on the interior, the one-voxel shell and the eight corners.

Which kernel ran is read from the launch profiler: family 12 (conv_up2c_kernel) holds the coarse-grid kernels, family 11 / 10 the
fine-grid conv_f16s<.., up2> that takes the shapes the eligibility function rejects.  Inside family 12 the recorded flops tell the
two forms apart: the product form records the products it performs, 4 x 27 per coarse voxel and channel pair (composite along z and
x, raw taps along y), the composite form the fine conv's 8 x 27.  The eligibility function takes whole 2 x 8 x 8 bricks only, so the
accepted 'ragged' extents are those that are no multiple of the 8-cube (z = 6, y = 24); (8, 12, 8) and (5, 8, 8) are rejected."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

REL = 2e-5


# ---- the identity, CPU, fp64 --------------------------------------------------------------------------------------------------
def _fine_conv(a, w):
    return F.conv3d(F.interpolate(a, scale_factor=2.0, mode="trilinear", align_corners=False), w, padding=1)


def _product_form_all_axes(a, w):
    """out[o, p] = sum_t [p + t inside] up(P_t)[o, p + t],  P_t[o, r] = sum_c W[o, c, t] a[c, r] on the coarse grid"""
    N, _, D, H, W_ = a.shape
    out = torch.zeros(N, w.shape[0], 2 * D, 2 * H, 2 * W_, dtype=a.dtype)
    for tz in range(3):
        for ty in range(3):
            for tx in range(3):
                P = torch.einsum("oc,ncdhw->nodhw", w[:, :, tz, ty, tx], a)
                up = F.pad(F.interpolate(P, scale_factor=2.0, mode="trilinear", align_corners=False), (1, 1, 1, 1, 1, 1))
                out += up[:, :, tz:tz + 2 * D, ty:ty + 2 * H, tx:tx + 2 * W_]
    return out


def _product_form_along_y(a, w):
    """the same along y alone: Q_ty = the (z, x) taps of fine tap row ty applied to the tensor upsampled along z and x only,
    still on the coarse y grid; out = sum_ty [py + ty inside] up_y(Q_ty)[.., py + ty, ..]"""
    N, _, D, H, W_ = a.shape
    azx = F.interpolate(a, scale_factor=(2.0, 1.0, 2.0), mode="trilinear", align_corners=False)
    out = torch.zeros(N, w.shape[0], 2 * D, 2 * H, 2 * W_, dtype=a.dtype)
    for ty in range(3):
        Q = F.conv3d(azx, w[:, :, :, ty:ty + 1, :], padding=(1, 0, 1))
        up = F.pad(F.interpolate(Q, scale_factor=(1.0, 2.0, 1.0), mode="trilinear", align_corners=False), (0, 0, 1, 1, 0, 0))
        out += up[:, :, :, ty:ty + 2 * H, :]
    return out


@pytest.mark.parametrize("dims,Cin,Cout", [((3, 5, 4), 6, 4), ((1, 2, 7), 3, 5), ((4, 4, 4), 8, 8)])
def test_products_commute_with_trilinear_upsampling_fp64(dims, Cin, Cout):
    g = torch.Generator().manual_seed(sum(dims) + Cin)
    a = torch.randn(2, Cin, *dims, generator=g, dtype=torch.float64) * 3.0
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = _fine_conv(a, w)
    scale = ref.abs().max().item()
    # fp64: 53 bits, sums of 27 Cin <= 216 terms of both signs - 1e-12 of the scale is four decimal orders above the rounding noise
    for form in (_product_form_all_axes, _product_form_along_y):
        err = (form(a, w) - ref).abs().max().item() / scale
        assert err < 1e-12, f"{form.__name__}: {err:.3e}"


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _cfg():
    from neural_marionette_amd import _lib
    return _lib.NmConfig(device=0, grid_size=64, nkeypoints=24, nlatent=128, nhidden=512, nneighbor=2,
                         gaussian_sigma=1.5, sep_sigma=0.02, vol_fit_chamfer=1, use_graph_traj=1)


@pytest.fixture(scope="module")
def ctx():
    from neural_marionette_amd import _lib
    c = _lib.Context(_cfg())
    c.bind_stream()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_composite():
    """a context created with the A/B switch's other value: the layers stay on the composite-weight kernels"""
    from neural_marionette_amd import _lib
    old = os.environ.get("NM355_UP2Y")
    os.environ["NM355_UP2Y"] = "0"
    try:
        c = _lib.Context(_cfg())
    finally:
        if old is None:
            os.environ.pop("NM355_UP2Y", None)
        else:
            os.environ["NM355_UP2Y"] = old
    c.bind_stream()
    yield c
    c.close()


def _to_cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous().cuda()


def _dev(t):
    return None if t is None else t.contiguous().cuda()


def _case(Cin, Cout, dims, prologue, N):
    D, H, W_ = dims
    g = torch.Generator().manual_seed(Cin * 7 + D * 100 + H * 10 + W_ + (1 if prologue else 0))
    x = torch.randn(N, Cin, D, H, W_, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    if prologue:
        sc = torch.rand(N, Cin, generator=g) + 0.5
        sh = torch.randn(N, Cin, generator=g) * 0.3
        xin = F.leaky_relu(x * sc[:, :, None, None, None] + sh[:, :, None, None, None], 0.01)
    else:
        sc = sh = None
        xin = F.leaky_relu(x, 0.01)
    gam = torch.rand(Cout, generator=g) + 0.5
    bet = torch.randn(Cout, generator=g) * 0.2
    return x, w, b, sc, sh, xin, gam, bet


def _run(c, x, w, b, sc, sh, gam, bet, groups):
    """one nm_op_conv3d(up2=1) launch in conv mode 1 under the launch profiler -> (out, gn scale, gn shift, {family: (flops, launches)})"""
    from neural_marionette_amd import _lib
    lib, h = c.lib, c.handle
    N, Cin, D, H, W_ = x.shape
    Cout = w.shape[0]
    _lib.check(lib.nm_set_conv_mode(h, 1), "set_conv_mode")
    out = torch.full((N, 2 * D, 2 * H, 2 * W_, Cout), float("nan")).cuda()
    gsc = torch.zeros(N, Cout).cuda(); gsh = torch.zeros(N, Cout).cuda()
    xd, wd, bd, scd, shd, gd, btd = _to_cl(x), _dev(w), _dev(b), _dev(sc), _dev(sh), _dev(gam), _dev(bet)
    _lib.check(lib.nm_prof_enable(h, 1), "prof_enable")
    _lib.check(lib.nm_op_conv3d(h, _lib.ptr(xd), N, D, H, W_, Cin, _lib.ptr(scd), _lib.ptr(shd), 0.01, _lib.ptr(wd), _lib.ptr(bd),
                                Cout, 3, 1, 1, _lib.ptr(out), groups, _lib.ptr(gd), _lib.ptr(btd), _lib.ptr(gsc), _lib.ptr(gsh), 1),
               "op_conv3d(up2)")
    torch.cuda.synchronize()
    _lib.check(lib.nm_prof_enable(h, 0), "prof_enable")
    fam = {}
    for v in range(16):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(lib.nm_prof_read(h, v, C.byref(ms), C.byref(fl), C.byref(n)), "prof_read")
        if n.value:
            fam[lib.nm_prof_kernel_name(v).decode()] = (fl.value, n.value)
    return out, gsc, gsh, fam


def _regions(got, ref):
    """max abs error relative to the reference's max magnitude on the interior, the one-voxel shell and the eight corners"""
    scale = ref.abs().max().item()
    err = (got - ref).abs()
    inner = err[:, :, 1:-1, 1:-1, 1:-1].max().item() / scale
    sh = err.clone(); sh[:, :, 1:-1, 1:-1, 1:-1] = 0
    D2, H2, W2 = ref.shape[2:]
    corners = err[:, :, ::D2 - 1, ::H2 - 1, ::W2 - 1]
    assert corners.shape[2:] == (2, 2, 2)
    return inner, sh.max().item() / scale, corners.max().item() / scale


# (Cin, Cout, coarse dims, N, product form expected): both decoder layers at reduced and full extent, non-cubic extents and extents
# that are no multiple of the 8-cube
ACCEPTED = [
    (64, 32, (16, 16, 16), 2, True), (64, 32, (32, 32, 32), 1, True), (128, 64, (8, 8, 8), 2, True), (128, 64, (16, 16, 16), 1, True),
    (64, 32, (6, 24, 8), 3, True), (64, 32, (2, 8, 16), 2, True), (128, 64, (4, 8, 24), 1, True),
]
REJECTED = [(64, 32, (8, 12, 8), 2), (64, 32, (5, 8, 8), 1), (128, 64, (8, 8, 12), 1)]


def _check_against_aten(c, Cin, Cout, dims, prologue, N):
    x, w, b, sc, sh, xin, gam, bet = _case(Cin, Cout, dims, prologue, N)
    groups = Cout // 16
    ref = F.conv3d(F.interpolate(xin, scale_factor=2.0, mode="trilinear", align_corners=False), w, b, padding=1)
    out, gsc, gsh, fam = _run(c, x, w, b, sc, sh, gam, bet, groups)
    got = out.permute(0, 4, 1, 2, 3).contiguous().cpu()
    assert torch.isfinite(got).all(), "unwritten / non-finite outputs"
    inner, shell, corners = _regions(got, ref)
    print("up2 conv %s ci%d co%d: interior %.2e shell %.2e corners %.2e families %s" % (dims, Cin, Cout, inner, shell, corners, fam))
    assert inner < REL, f"interior rel err {inner:.3e}"
    assert shell < REL, f"shell rel err {shell:.3e}"
    assert corners < REL, f"corner rel err {corners:.3e}"
    refn = F.group_norm(ref, groups, gam, bet, 1e-5)
    gotn = got * gsc.cpu()[:, :, None, None, None] + gsh.cpu()[:, :, None, None, None]
    e = (gotn - refn).abs().max().item() / refn.abs().max().item()
    assert e < REL, f"fused GroupNorm rel err {e:.3e}"
    return (x, w, b, sc, sh, gam, bet, groups), (out, gsc, gsh), fam


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N,product", ACCEPTED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_product_form_against_aten(ctx, Cin, Cout, dims, N, product, prologue):
    args, (out, gsc, gsh), fam = _check_against_aten(ctx, Cin, Cout, dims, prologue, N)
    # the coarse-grid family took it, one record (main + shell launches timed together), with the products the kernel performs
    assert list(fam) == ["conv_up2c_kernel"], fam
    coarse = N * dims[0] * dims[1] * dims[2]
    want = 2.0 * coarse * (4 if product else 8) * 27 * Cin * Cout
    assert fam["conv_up2c_kernel"] == (want, 1), (fam, want)
    # the same launch twice: bit-identical, GroupNorm scale / shift included (fixed-order partial sums, no atomics)
    out2, gsc2, gsh2, _ = _run(ctx, *args)
    assert torch.equal(out, out2) and torch.equal(gsc, gsc2) and torch.equal(gsh, gsh2)


@pytest.mark.gpu
@pytest.mark.parametrize("Cin,Cout,dims,N", REJECTED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rejected_extents_keep_the_fine_grid_kernel(ctx, Cin, Cout, dims, N):
    _, _, fam = _check_against_aten(ctx, Cin, Cout, dims, True, N)
    assert len(fam) == 1 and list(fam)[0].startswith("conv_f16s_kernel<2,") and list(fam)[0].endswith("up2>"), fam


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N", [(64, 32, (16, 16, 16), 2), (64, 32, (6, 24, 8), 3), (128, 64, (8, 8, 8), 2), (64, 32, (32, 32, 32), 1)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_switch_off_gives_the_composite_kernels_output(ctx, ctx_composite, Cin, Cout, dims, N, prologue):
    """NM355_UP2Y=0 (read when the context is created): today's kernels.  Both forms are within REL of the exact result, so within
    2 REL of each other - on the raw output and on the normalised one."""
    x, w, b, sc, sh, xin, gam, bet = _case(Cin, Cout, dims, prologue, N)
    groups = Cout // 16
    out_n, gsc_n, gsh_n, fam_n = _run(ctx, x, w, b, sc, sh, gam, bet, groups)
    out_o, gsc_o, gsh_o, fam_o = _run(ctx_composite, x, w, b, sc, sh, gam, bet, groups)
    coarse = N * dims[0] * dims[1] * dims[2]
    fine_flops = 2.0 * coarse * 8 * 27 * Cin * Cout
    # the old arm: the composite kernel with the fine conv's count (64 -> 32), or conv_f16s<.., up2> (128 -> 64)
    assert len(fam_o) == 1 and list(fam_o.values())[0] == (fine_flops, 1), fam_o
    if Cin == 64:
        assert list(fam_o) == ["conv_up2c_kernel"], fam_o
    assert fam_n != fam_o
    scale = out_o.abs().max().item()
    e = (out_n - out_o).abs().max().item() / scale
    print("product form vs composite kernels %s: %.2e" % (dims, e))
    assert e < 2 * REL
    nn = out_n * gsc_n[:, None, None, None, :] + gsh_n[:, None, None, None, :]
    no = out_o * gsc_o[:, None, None, None, :] + gsh_o[:, None, None, None, :]
    assert (nn - no).abs().max().item() / no.abs().max().item() < 2 * REL
