"""The five persistent producer / consumer conv kernels (conv_f16p, _f16p2, _f16p8, _f16q2, _f16r) in the XCD super-tile order.

The kernels take their bricks from neural_marionette_amd/csrc/nm_brick_walk.h.  The other conv tests reach its super-tile order only
at network size (the comment above MANY_SHAPES in test_conv_f16p8_gpu.py; neither 32^3 case of test_ops_gpu.CONV_CASES meets
choose_super_tile's conditions).  Here every kernel runs one nm_op_conv3d call with an affine prologue, bias and GroupNorm groups at a
frame count for which a 256-workgroup launch is tiled with two bricks per workgroup, against F.conv3d / F.group_norm in double at
test_ops_gpu.py's bounds (REL for the three-product modes, F16_REL for mode 3), and the first three frames must equal, bit for bit,
the same call on those three frames alone: with N = 3 the super-tile count is no multiple of 8, so that launch walks in linear order.

Which kernel a case runs (nm_launch_conv's routing; conv_f16p and conv_f16p8 share profiler family 7, so the family alone does not
tell them apart):
  * conv mode 2 sends 16 -> 32 at 32^3 to conv_f16p8, like mode 1 does: whole 8 x 8 x 8 bricks go there first ("p8-mode2").
  * conv_f16p in the tiled order is reachable only in its one-product (SINGLE) instantiation, where the one-product mode has no
    resident-weight form (Cin = 16): "p-single".  The three-product conv_f16p<false> has NO tiled launch through nm_launch_conv: the
    super-tile needs an even number of 4-deep bricks along z, that is D % 8 == 0, and those calls are conv_f16p8's; conv mode 2 with more
    than 32 output channels launches without the super-tile.
  * "p-d20-linear" runs the three-product conv_f16p (D % 8 == 4, which conv_f16p8 cannot take) on the shared walk in LINEAR order, two
    bricks per workgroup: fp64 parity, and the full call against its first three frames alone (both linear: different runs per workgroup).
"""
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
from test_conv_f16p8_gpu import _family_counts
from test_ops_gpu import F16_REL, REL, ctx, dev, from_cl, relerr, to_cl  # noqa: F401  (ctx is a fixture)

pytestmark = pytest.mark.gpu

SLOPE = 0.01
GROUPS = 2
# kernel, Cin, Cout, conv mode, N, dims, profiler family, brick depth of the kernel that runs, tiled order expected
CASES = [
    ("p8", 16, 32, 1, 8, (32, 32, 32), "conv_f16p_kernel", 8, True),
    ("p8", 32, 32, 1, 8, (32, 32, 32), "conv_f16p_kernel", 8, True),
    ("p8-mode2", 16, 32, 2, 8, (32, 32, 32), "conv_f16p_kernel", 8, True),
    ("p2", 16, 64, 1, 4, (32, 32, 32), "conv_f16p2_kernel", 4, True),
    ("q2", 16, 64, 3, 4, (32, 32, 32), "conv_f16q2_kernel", 4, True),
    ("r", 32, 32, 3, 4, (32, 32, 32), "conv_f16r_kernel", 4, True),
    ("p-d20-linear", 16, 32, 1, 4, (20, 32, 32), "conv_f16p_kernel", 4, False),
    ("p-single", 16, 32, 3, 4, (32, 32, 32), "conv_f16p_kernel", 4, True),
]


def _super_tiled(N, dims, bz, wgs=256):
    """choose_super_tile's conditions (nm_brick_walk.h) for a launch of `wgs` workgroups"""
    nbz, nby, nbx = dims[0] // bz, dims[1] // 8, dims[2] // 8
    sz = {64: 4, 32: 2}.get(wgs // 8, 0)
    if wgs % 8 or not sz or nbz % sz or nby % 4 or nbx % 4:
        return False
    st = N * (nbz // sz) * (nby // 4) * (nbx // 4)
    return st % 8 == 0 and st // 8 * wgs == N * nbz * nby * nbx


def _run(c, mode, xd, N, dims, Cin, Cout, d):
    from neural_marionette_amd import _lib
    out = torch.full((N, *dims, Cout), float("nan")).cuda()
    gsc = torch.full((N, Cout), float("nan")).cuda(); gsh = torch.full((N, Cout), float("nan")).cuda()
    _lib.check(c.lib.nm_set_conv_mode(c.handle, mode), "set_conv_mode")
    try:
        _lib.check(c.lib.nm_prof_enable(c.handle, 1), "prof_enable")
        _lib.check(c.lib.nm_op_conv3d(c.handle, _lib.ptr(xd), N, *dims, Cin, _lib.ptr(d["scd"][:N].contiguous()), _lib.ptr(d["shd"][:N].contiguous()), SLOPE,
                                      _lib.ptr(d["wd"]), _lib.ptr(d["bd"]), Cout, 3, 1, 1, _lib.ptr(out), GROUPS, _lib.ptr(d["gd"]), _lib.ptr(d["btd"]),
                                      _lib.ptr(gsc), _lib.ptr(gsh), 0), "op_conv3d")
        torch.cuda.synchronize()
        _lib.check(c.lib.nm_prof_enable(c.handle, 0), "prof_enable")
    finally:
        _lib.check(c.lib.nm_set_conv_mode(c.handle, 1), "set_conv_mode")
    return out, gsc, gsh, _family_counts(c)


@pytest.mark.parametrize("case", CASES, ids=lambda v: "%s_ci%d_co%d_m%d_N%d" % v[:5])
def test_tiled_order(ctx, case):
    name, Cin, Cout, mode, N, dims, family, bz, tiled = case
    # the brick depth must be the running kernel's: conv_f16p8 takes every three-product Cout = 32 call with D % 8 == 0, conv_f16p the rest
    assert bz == (8 if (mode in (1, 2) and Cout == 32 and dims[0] % 8 == 0) else 4), "brick depth of another kernel than the one that runs"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the super-tile order of these frame counts needs 256 workgroups, one per CU; this device has %d CUs" % cus)
    bricks = N * (dims[0] // bz) * (dims[1] // 8) * (dims[2] // 8)
    assert _super_tiled(N, dims, bz) == tiled and bricks / 256 > 1, "the case does not walk several bricks per workgroup in the order it names"
    assert not _super_tiled(3, dims, bz), "the comparison launch must walk in linear order"
    g = torch.Generator().manual_seed(X._seed("pc-orders", case))
    x = torch.randn(N, Cin, *dims, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    sc = torch.rand(N, Cin, generator=g) + 0.5
    sh = torch.randn(N, Cin, generator=g) * 0.3
    gam, bet = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    d = dict(wd=dev(w), bd=dev(b), scd=dev(sc), shd=dev(sh), gd=dev(gam), btd=dev(bet))
    xd = to_cl(x)
    out, gsc, gsh, fam = _run(ctx, mode, xd, N, dims, Cin, Cout, d)
    out3, gsc3, gsh3, fam3 = _run(ctx, mode, xd[:3].contiguous(), 3, dims, Cin, Cout, d)
    print(name, "families:", fam, fam3)
    assert list(fam) == [family] and fam[family][0] == 1 and list(fam3) == [family] and fam3[family][0] == 1, (fam, fam3)
    # fp64 reference
    xa = F.leaky_relu(x.double() * sc.double()[:, :, None, None, None] + sh.double()[:, :, None, None, None], SLOPE)
    ref = F.conv3d(xa, w.double(), b.double(), padding=1)
    refn = F.group_norm(ref, GROUPS, gam.double(), bet.double(), 1e-5)
    got = from_cl(out, Cout)
    assert torch.isfinite(got).all() and torch.isfinite(gsc).all() and torch.isfinite(gsh).all(), "unwritten / non-finite outputs"
    tol = F16_REL if mode == 3 else REL
    per_frame = (got.double() - ref).abs().amax(dim=(1, 2, 3, 4)) / ref.abs().max()
    gotn = got.double() * gsc.cpu().double()[:, :, None, None, None] + gsh.cpu().double()[:, :, None, None, None]
    per_frame_n = (gotn - refn).abs().amax(dim=(1, 2, 3, 4)) / refn.abs().max()
    print("%s: raw %.3e, normalised %.3e (bound %.0e)" % (name, per_frame.max().item(), per_frame_n.max().item(), tol))
    assert per_frame.max().item() < tol, "worst frame %d: %.3e" % (int(per_frame.argmax()), per_frame.max().item())
    assert per_frame_n.max().item() < tol, "fused GroupNorm, worst frame %d: %.3e" % (int(per_frame_n.argmax()), per_frame_n.max().item())
    # the full launch (tiled, but for the case that says linear) against the linear launch of three frames, bit for bit
    for what, a, bb in (("output", out[:3], out3), ("GroupNorm scale", gsc[:3], gsc3), ("GroupNorm shift", gsh[:3], gsh3)):
        assert torch.equal(a, bb), "%s: %d of %d values differ between the full call and its first three frames alone" % (what, int((a != bb).sum()), a.numel())
