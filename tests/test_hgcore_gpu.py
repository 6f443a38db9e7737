"""Op-level parity of the two lowest hourglass levels: hg_core_kernel (csrc/nm_hgcore.hip: 13 split-fp16 convs, 14 GroupNorms, the
k2 s2 transposed conv with its output-padding planes and the residual adds of one frame, in LDS) and the same layers as the separate
launches of the inference forward, both through nm_op_hourglass_core - the helper the network itself calls - against the float64
reference of tests/hgcore_ref.py (pinned to the oracle and shown to be well conditioned by tests/test_hgcore_ref_cpu.py).

Level-2 extents D = 2 .. 6 are all the fused launch accepts and all the accepted grids produce (D = grid_size // 16):
  D  rows  32-row tiles (live rows of the last)  level 3   pool drops a plane / padding plane   conv epilogue
  2     8  1 (8)                                  1^3       no                                   K-split partial tiles in LDS
  3    27  1 (27)                                 1^3       yes                                  K-split
  4    64  2 (32)                                 2^3       no                                   K-split
  5   125  4 (29)                                 2^3       yes                                  through the scratch, one part per tile pair
  6   216  7 (24)                                 3^3       no                                   direct store (no LDS left for scratch)
Bound: 2e-5 of the reference's largest magnitude, the project's op-level bound (tests/test_ops_gpu.py); float32 torch is at 3e-7 ..
8e-7 on these cases.  Outputs are pre-filled with NaN and must come back finite."""
import ctypes as C

import pytest
import torch

import hgcore_ref as R

pytestmark = pytest.mark.gpu

REL = 2e-5
FORMS = {1: "fused", 0: "separate"}


def L():
    from neural_marionette_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx():
    """a context holding the weights of hgcore_ref.state_dict(), conv mode split16"""
    from neural_marionette_amd import NeuralMarionette, HotPathOptions
    net = NeuralMarionette(HotPathOptions(grid_size=32))
    net.load_state_dict(R.state_dict())
    net = net.cuda().eval()
    net.set_conv_mode("split16")
    c = net._engine.ready()
    assert c.lib.nm_get_conv_mode(c.handle) == 1
    yield c
    del net


def op(ctx, inp, which, fused, D=None, N=None, **over):
    """raw status and the output (N,48,D,D,D) on the device; `over` replaces single arguments (refusal cases)"""
    P = L().ptr
    x = R.to_cl(inp["raw"]).cuda()
    sc = None if inp["scale"] is None else inp["scale"].contiguous().cuda()
    sh = None if inp["shift"] is None else inp["shift"].contiguous().cuda()
    N = x.shape[0] if N is None else N
    D = x.shape[1] if D is None else D
    out = torch.full((max(N, 1), D, D, D, R.COUT), float("nan"), dtype=torch.float32, device="cuda")
    a = dict(which=which, p_in=P(x), p_scale=P(sc), p_shift=P(sh), slope=inp["slope"], N=N, D=D, fused=fused, p_out=P(out))
    a.update(over)
    rc = ctx.lib.nm_op_hourglass_core(a.get("handle", ctx.handle), a["which"], a["p_in"], a["p_scale"], a["p_shift"], a["slope"], a["N"], a["D"],
                                      a["fused"], a["p_out"])
    torch.cuda.synchronize()
    return rc, R.from_cl(out)


def run(ctx, inp, which, fused):
    rc, out = op(ctx, inp, which, fused)
    L().check(rc, "nm_op_hourglass_core")
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def check_parity(ctx, case, fused):
    r64 = R.ref_case(case, torch.float64)
    out = run(ctx, R.inputs(*case), case[1], fused).cpu()
    assert out.shape == r64.shape and torch.isfinite(out).all(), "not finite / not fully written"
    e = R.relerr(out, r64)
    print("D=%d net %d %-4s %-8s: %.2e   (float32 torch %.2e, max |ref| %.2f)" % (*case, FORMS[fused], e, R.relerr(R.ref_case(case, torch.float32), r64),
                                                                               r64.abs().max().item()))
    assert e < REL, f"{case} {FORMS[fused]}: {e:.3e} >= {REL:.1e}"


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "separate"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "D%d-net%d-%s" % c)
def test_parity_against_float64(ctx, case, fused):
    check_parity(ctx, case, fused)


def test_frames_are_independent_beyond_256_frames(ctx):
    """300 frames of 2^3 voxels, one workgroup each: more workgroups than the chip has compute units, frame indices on both sides of
    255 / 256, a per-frame scale / shift table of 300 rows.  Frames 0, 255, 256 and 299 carry the same input: their outputs must be
    the same bits, and the bits of a one-frame call (a workgroup sees nothing but its frame)."""
    inp = R.inputs(2, 0, "lazy", N=300)
    same = (0, 255, 256, 299)
    for k in ("raw", "scale", "shift"):
        inp[k][list(same[1:])] = inp[k][0].clone()
    out = run(ctx, inp, 0, 1)
    assert torch.isfinite(out).all()
    for f in same[1:]:
        assert torch.equal(bits(out[f]), bits(out[0])), f
    assert not torch.equal(out[1], out[0])
    one = {k: (v[:1].clone() if torch.is_tensor(v) else v) for k, v in inp.items()}
    assert torch.equal(bits(run(ctx, one, 0, 1)[0]), bits(out[0]))
    # (and frame 0 is right: the one-frame reference)
    assert R.relerr(out[:1].cpu(), R.ref(one, 0, torch.float64)) < REL


def test_last_frame_of_five_at_the_largest_extent(ctx):
    """D = 6 (direct-store epilogue, 160 KB of LDS: one workgroup per compute unit): frame 4 of 5 is the one-frame call's bits"""
    inp = R.inputs(6, 1, "lazy", N=5)
    out = run(ctx, inp, 1, 1)
    one = {k: (v[4:5].clone() if torch.is_tensor(v) else v) for k, v in inp.items()}
    assert torch.equal(bits(run(ctx, one, 1, 1)[0]), bits(out[4]))
    assert R.relerr(out[4:5].cpu(), R.ref(one, 1, torch.float64)) < REL


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "separate"])
def test_a_value_beyond_the_fp16_range_stays_in_its_frame(ctx, fused):
    """1e5 has no split-fp16 representation (hi = inf): the frame that holds it must come back non-finite - a finite answer would be
    a silently wrong one - and its neighbours must not change by a bit.  The op-level call leaves the context's range status alone."""
    case = (4, 0, "none")
    inp = R.inputs(*case)
    clean = run(ctx, inp, 0, fused)
    inp["raw"][1, 5, 1, 2, 1] = 1e5
    bad = run(ctx, inp, 0, fused)
    assert not torch.isfinite(bad[1]).all()
    for f in (0, 2):
        assert torch.equal(bits(bad[f]), bits(clean[f])), f
    assert ctx.lib.nm_ctx_check_nonfinite(ctx.handle) == 0
    check_parity(ctx, case, fused)


def refused(ctx, code, word, inp, which, fused, **over):
    rc, _ = op(ctx, inp, which, fused, **over)
    msg = ctx.lib.nm_last_error().decode()
    assert rc == code, (rc, msg)
    assert word in msg, msg
    check_parity(ctx, (2, 1, "lazy"), 1)          # the context is still good
    check_parity(ctx, (3, 0, "none"), 0)


@pytest.mark.parametrize("D", [1, 7])
def test_fused_form_refuses_extents_outside_2_to_6(ctx, D):
    inp = R.inputs(D, 0, "lazy")
    refused(ctx, L().NM_ERR_UNSUPPORTED, "extent %d" % D, inp, 0, 1)


def test_fused_form_refuses_conv_mode_fp32(ctx):
    """conv mode 0 is exact fp32 MFMA; the fused launch is split-fp16 arithmetic and must not stand in for it"""
    lib = L()
    lib.check(ctx.lib.nm_set_conv_mode(ctx.handle, 0), "set_conv_mode")
    try:
        rc, _ = op(ctx, R.inputs(4, 0, "lazy"), 0, 1)
        msg = ctx.lib.nm_last_error().decode()
    finally:
        lib.check(ctx.lib.nm_set_conv_mode(ctx.handle, 1), "set_conv_mode")
    assert rc == lib.NM_ERR_UNSUPPORTED and "conv mode 0" in msg, (rc, msg)
    check_parity(ctx, (4, 0, "lazy"), 1)


@pytest.mark.parametrize("over,word", [(dict(which=2), "which=2"), (dict(which=-1), "which=-1"), (dict(fused=2), "fused=2"), (dict(N=0), "N=0"),
                                       (dict(p_in=None), "null"), (dict(p_out=None), "null"), (dict(p_scale=None), "null"), (dict(p_shift=None), "null"),
                                       (dict(handle=C.c_void_p()), "null")],
                         ids=["which2", "which-1", "fused2", "N0", "null-in", "null-out", "shift-only", "scale-only", "null-ctx"])
def test_bad_arguments_are_refused(ctx, over, word):
    over = dict(over)
    which, fused = over.pop("which", 0), over.pop("fused", 1)
    refused(ctx, L().NM_ERR_ARG, word, R.inputs(2, 0, "lazy"), which, fused, **over)
