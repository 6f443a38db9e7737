"""The shell kernels of the fused-upsample layers under NM355_UP2C_SHELL (nm_up2c.hip): conv_up2c_face_r_kernel (value 1, the
default: a face workgroup owns R lines, one weight fetch feeds 3 R MFMAs) and conv_up2c_edge_p_kernel (values 2 and 3, not the
default: the loads of the next three tap groups in flight, both output halves from one A fetch; launched where there are two
output halves, Cout = 64).

The new forms keep, per output cell, the parent kernels' operands, MFMA order, store expression and GroupNorm partial slots, so
the comparison with NM355_UP2C_SHELL=0 is torch.equal - on the output and on the GroupNorm scale / shift - and not a tolerance.
The switch is read when a context is created: every arm is a context of its own (made like those of test_upsample_march_gpu.py)
and driven through nm_op_conv3d(..., up2=1).

Settings of the exact comparison (the other switches equal in both arms):
  * NM355_UP2C_SHELL=1 against 0 in the default, with NM355_UP2Y_YPAD=0 (the y faces run through the face kernel) and with
    NM355_UP2Y=0 (the composite main kernel with the same shell on 64 -> 32; the 128 -> 64 layer is conv_f16s's there and has no
    shell, so its two shapes compare that kernel with itself);
  * the edge form: with the face form (2) in the default and with NM355_UP2Y_YPAD=0 (the subset {y} runs through it), and alone (3);
  * R = 2 and R = 4 forced (tens digit of the switch), y faces included.
Against ATen (interior, shell, corners within REL) and twice for repeatability in the default context.

Shapes (Cin, Cout, coarse (D, H, W), frames) - the smallest at which each index path can go wrong:
  (64, 32, (2, 8, 8), 3)     smallest eligible extent; D = 2 puts whole lines on an edge for some class, fewer lines per face side
                             than R, three frames so that line groups meet frame boundaries
  (64, 32, (6, 16, 24), 2)   non-cubic; 6, 16 and 24 lines per side: a remainder for R = 4 (and 6 = 3 groups of 2)
  (64, 32, (4, 40, 8), 2)    two tiles along a line, the second ragged (40 = 32 + 8)
  (128, 64, (6, 8, 40), 2)   two output halves, eight channel chunks, a ragged tile along x
  (128, 64, (16, 16, 16), 1), (64, 32, (32, 32, 32), 1)   the bench layers' own per-frame extents"""
import pytest
import torch

from test_upsample_march_gpu import _ctx_with
from test_upsample_product_form_gpu import REL, _case, _check_against_aten, _run

SHAPES = [
    (64, 32, (2, 8, 8), 3), (64, 32, (6, 16, 24), 2), (64, 32, (4, 40, 8), 2), (128, 64, (6, 8, 40), 2),
    (128, 64, (16, 16, 16), 1), (64, 32, (32, 32, 32), 1),
]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)

# setting -> (switches of the new arm, switches of the parent arm)
SETTINGS = {
    "default": (dict(NM355_UP2C_SHELL=1), dict(NM355_UP2C_SHELL=0)),
    "ypad0": (dict(NM355_UP2C_SHELL=1, NM355_UP2Y_YPAD=0), dict(NM355_UP2C_SHELL=0, NM355_UP2Y_YPAD=0)),
    "up2y0": (dict(NM355_UP2C_SHELL=1, NM355_UP2Y=0), dict(NM355_UP2C_SHELL=0, NM355_UP2Y=0)),
    "face_and_edge": (dict(NM355_UP2C_SHELL=2), dict(NM355_UP2C_SHELL=0)),
    "face_and_edge_ypad0": (dict(NM355_UP2C_SHELL=2, NM355_UP2Y_YPAD=0), dict(NM355_UP2C_SHELL=0, NM355_UP2Y_YPAD=0)),
    "edge_only": (dict(NM355_UP2C_SHELL=3), dict(NM355_UP2C_SHELL=0)),
    "r2_ypad0": (dict(NM355_UP2C_SHELL=21, NM355_UP2Y_YPAD=0), dict(NM355_UP2C_SHELL=0, NM355_UP2Y_YPAD=0)),
    "r4_ypad0": (dict(NM355_UP2C_SHELL=41, NM355_UP2Y_YPAD=0), dict(NM355_UP2C_SHELL=0, NM355_UP2Y_YPAD=0)),
}


@pytest.fixture(scope="module")
def ctxs():
    """contexts by their switches, created on first use and closed with the module"""
    made = {}

    def get(env):
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = _ctx_with({k: str(v) for k, v in env.items()})
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def parent_results():
    """the parent arm's (out, scale, shift) per (parent switches, shape, prologue): computed once, shared, never modified"""
    return {}


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N", SHAPES, ids=_ids)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_new_shell_is_bit_identical_to_the_parent_kernels(ctxs, parent_results, setting, Cin, Cout, dims, N, prologue):
    env_new, env_old = SETTINGS[setting]
    x, w, b, sc, sh, xin, gam, bet = _case(Cin, Cout, dims, prologue, N)
    key = (tuple(sorted(env_old.items())), Cin, Cout, dims, N, prologue)
    if key not in parent_results:
        parent_results[key] = _run(ctxs(env_old), x, w, b, sc, sh, gam, bet, Cout // 16)[:3]
    out_o, gsc_o, gsh_o = parent_results[key]
    out_n, gsc_n, gsh_n, _ = _run(ctxs(env_new), x, w, b, sc, sh, gam, bet, Cout // 16)
    assert torch.isfinite(out_n).all(), "unwritten / non-finite outputs"
    assert torch.equal(out_n, out_o), "outputs differ: %.3e at %d voxels" % ((out_n - out_o).abs().max().item(), (out_n != out_o).sum().item())
    assert torch.equal(gsc_n, gsc_o), "GroupNorm scale differs: %.3e" % (gsc_n - gsc_o).abs().max().item()
    assert torch.equal(gsh_n, gsh_o), "GroupNorm shift differs: %.3e" % (gsh_n - gsh_o).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("prologue", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("Cin,Cout,dims,N", SHAPES, ids=_ids)
def test_default_shell_against_aten_and_repeatable(ctxs, Cin, Cout, dims, N, prologue):
    c = ctxs({})
    args, (out, gsc, gsh), fam = _check_against_aten(c, Cin, Cout, dims, prologue, N)
    assert list(fam) == ["conv_up2c_kernel"], fam
    out2, gsc2, gsh2, _ = _run(c, *args)
    assert torch.equal(out, out2) and torch.equal(gsc, gsc2) and torch.equal(gsh, gsh2)
