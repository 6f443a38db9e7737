"""conv_up2y_kernel marching along y (the two halo row tiles of a brick carried to its y-successor instead of recomputed) and the
fine conv's zero padding along y applied in its epilogue (the y faces leave the shell kernels) - nm_up2c.hip.

Both parts have a switch that is read when a context is created (NM355_UP2Y_MARCH: 0 no carry, 1 march where there are at least as
many columns as CUs, 2 march always; NM355_UP2Y_YPAD: 0 the y faces stay with the shell kernels), so every arm is a context of its
own, made the way test_upsample_product_form_gpu.py makes its NM355_UP2Y=0 context, and driven through nm_op_conv3d(..., up2=1).

  * the carry is EXACT: a carried tile holds the same operands run through the same MFMA chain as the tile it replaces, so march on
    / off (y padding off in both) must agree bit for bit, GroupNorm scale / shift included;
  * the y padding is CONFINED: with it on / off every fine voxel with 0 < oy < OH - 1 is bit-identical; on the two y planes both
    arms are within REL of the exact result, so within 2 REL of each other;
  * against ATen (interpolate -> conv3d -> group_norm, REL = 2e-5; interior, shell, corners) with both parts on and marching
    forced: 1, 2, 3, 4 and 6 bricks along y, several frames, workgroup ranges of two columns that end inside a frame and across a
    frame change, both layers (the 128 -> 64 one marches a column once per 32-channel output group), with and without the affine
    prologue; and the full-size 64 -> 32 layer at 32^3 with enough frames that marching engages by itself;
  * the same launch twice is bit-identical."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_upsample_product_form_gpu import REL, _case, _cfg, _check_against_aten, _run


def _ctx_with(env):
    from neural_marionette_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = _lib.Context(_cfg())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.bind_stream()
    return c


def _ctx_fixture(**env):
    @pytest.fixture(scope="module")
    def fx():
        c = _ctx_with({k: str(v) for k, v in env.items()})
        yield c
        c.close()
    return fx


ctx_default = _ctx_fixture()                                                  # both parts on, marching where it pays
ctx_forced = _ctx_fixture(NM355_UP2Y_MARCH=2, NM355_UP2Y_YPAD=1)              # both parts on, marching at every shape
ctx_march_nopad = _ctx_fixture(NM355_UP2Y_MARCH=2, NM355_UP2Y_YPAD=0)
ctx_plain_nopad = _ctx_fixture(NM355_UP2Y_MARCH=0, NM355_UP2Y_YPAD=0)         # the parent's order and shell
ctx_plain_pad = _ctx_fixture(NM355_UP2Y_MARCH=0, NM355_UP2Y_YPAD=1)

_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)

# (Cin, Cout, coarse dims, N).  Bricks are 2 x 8 x 8 coarse cells, a column is the nby = y / 8 bricks of one (frame, brick z, brick x).
# Forced marching hands out whole columns, ceil(columns / workgroups) each: one column per workgroup up to 256 columns.  (6, 16, 24)
# has 9 columns per frame, so with 40 (30) frames the 360 (270) columns go out in pairs and the pair (8, 9) is the last column of
# frame 0 and the first of frame 1, while (0, 1) ... (6, 7) end inside a frame.
SHAPES = [
    (64, 32, (4, 8, 8), 2), (64, 32, (4, 16, 8), 2), (64, 32, (2, 24, 16), 2), (64, 32, (4, 32, 8), 1), (64, 32, (2, 48, 8), 2),
    (64, 32, (6, 16, 24), 40),
    (128, 64, (8, 8, 8), 2), (128, 64, (16, 16, 16), 1), (128, 64, (2, 24, 8), 3), (128, 64, (2, 32, 8), 1), (128, 64, (2, 48, 8), 1),
    (128, 64, (6, 16, 24), 30),
]
SMALL = [s for s in SHAPES if s[3] < 10]


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N", SHAPES, ids=_ids)
def test_marching_with_y_padding_against_aten(ctx_forced, Cin, Cout, dims, N, prologue):
    args, (out, gsc, gsh), fam = _check_against_aten(ctx_forced, Cin, Cout, dims, prologue, N)
    assert list(fam) == ["conv_up2c_kernel"], fam
    out2, gsc2, gsh2, _ = _run(ctx_forced, *args)
    assert torch.equal(out, out2) and torch.equal(gsc, gsc2) and torch.equal(gsh, gsh2)


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
def test_full_size_layer_marches_by_default(ctx_default, ctx_plain_nopad, prologue):
    """64 -> 32 at 32^3, 4 frames: 4 x 16 x 4 = 256 columns of 4 bricks, as many as the MI355X has CUs, so the default context marches
    (one column per workgroup: 34 row tiles against 4 bricks x 10) without being forced.  Checked against ATen and for repeatability;
    and away from the two y planes the default arm must be the arithmetic of the arm with both switches off, bit for bit (the carry
    is exact, the y padding confined)."""
    args, (out, gsc, gsh), fam = _check_against_aten(ctx_default, 64, 32, (32, 32, 32), prologue, 4)
    assert list(fam) == ["conv_up2c_kernel"], fam
    out2, gsc2, gsh2, _ = _run(ctx_default, *args)
    assert torch.equal(out, out2) and torch.equal(gsc, gsc2) and torch.equal(gsh, gsh2)
    out_p, _, _, _ = _run(ctx_plain_nopad, *args)
    assert torch.equal(out[:, :, 1:-1], out_p[:, :, 1:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N", SHAPES, ids=_ids)
def test_carry_is_exact(ctx_march_nopad, ctx_plain_nopad, Cin, Cout, dims, N, prologue):
    x, w, b, sc, sh, xin, gam, bet = _case(Cin, Cout, dims, prologue, N)
    out_m, gsc_m, gsh_m, _ = _run(ctx_march_nopad, x, w, b, sc, sh, gam, bet, Cout // 16)
    out_p, gsc_p, gsh_p, _ = _run(ctx_plain_nopad, x, w, b, sc, sh, gam, bet, Cout // 16)
    assert torch.isfinite(out_m).all()
    assert torch.equal(out_m, out_p), "carried tiles differ from recomputed ones: %.3e" % (out_m - out_p).abs().max().item()
    assert torch.equal(gsc_m, gsc_p) and torch.equal(gsh_m, gsh_p)


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N", SMALL, ids=_ids)
def test_y_padding_is_confined(ctx_plain_pad, ctx_plain_nopad, Cin, Cout, dims, N, prologue):
    x, w, b, sc, sh, xin, gam, bet = _case(Cin, Cout, dims, prologue, N)
    out_y, gsc_y, gsh_y, _ = _run(ctx_plain_pad, x, w, b, sc, sh, gam, bet, Cout // 16)
    out_s, gsc_s, gsh_s, _ = _run(ctx_plain_nopad, x, w, b, sc, sh, gam, bet, Cout // 16)
    assert torch.isfinite(out_y).all()
    # outputs are (N, z, y, x, C)
    assert torch.equal(out_y[:, :, 1:-1], out_s[:, :, 1:-1])
    scale = out_s.abs().max().item()
    e = max((out_y[:, :, 0] - out_s[:, :, 0]).abs().max().item(), (out_y[:, :, -1] - out_s[:, :, -1]).abs().max().item()) / scale
    print("y planes, epilogue padding vs shell kernels %s: %.2e" % (dims, e))
    assert e < 2 * REL
    ny = out_y * gsc_y[:, None, None, None, :] + gsh_y[:, None, None, None, :]
    ns = out_s * gsc_s[:, None, None, None, :] + gsh_s[:, None, None, None, :]
    assert (ny - ns).abs().max().item() / ns.abs().max().item() < 2 * REL
