"""conv_f16p8_kernel: the k3 s1 p1 split-fp16 conv of the 32-output-channel layers on 8 x 8 x 8 bricks (conv mode 1, fp32 storage,
Cout == 32, OD % 8 == 0), through nm_op_conv3d.

The kernel must compute what conv_f16p computes, bit for bit (same accumulation order per output element, same GroupNorm partial
rows), with twice the voxels per staged step.  conv_f16p stays in the tree for OD % 8 == 4, so the bit-identity test needs no switch:
the same input with four z-planes appended (activated value exactly 0, which is what the padding is) runs on the old kernel.

Profiler family 7 ("conv_f16p") holds both kernels; the routing test tells launches apart by the shape they were given (the
algorithmic FLOPs of the launch), and by results only the right kernel can produce: conv_f16p8 cannot run D = 20."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import test_exact_arithmetic_gpu as TE
from test_ops_gpu import REL, ctx, to_cl, from_cl, relerr, dev  # noqa: F401  (ctx is a fixture)

pytestmark = pytest.mark.gpu

COUT = 32
FAMILY = "conv_f16p_kernel"           # nm_prof_kernel_name(7): conv_f16p and conv_f16p8
GROUPS = 2
SLOPE = 0.01


def _run(c, xd, N, dims, Cin, scd, shd, slope, wd, bd, groups=GROUPS, gd=None, btd=None, mode=1):
    """one nm_op_conv3d launch (k3 s1 p1, Cout = 32) on device operands: output, GroupNorm scale, GroupNorm shift (NaN without gamma /
    beta: the fused GroupNorm is then not asked for - the finaliser reads both)"""
    from neural_marionette_amd import _lib
    if gd is None or btd is None:
        groups = 0
    out = torch.full((N, *dims, COUT), float("nan")).cuda()
    gsc = torch.full((N, COUT), float("nan")).cuda(); gsh = torch.full((N, COUT), float("nan")).cuda()
    _lib.check(c.lib.nm_set_conv_mode(c.handle, mode), "set_conv_mode")
    try:
        _lib.check(c.lib.nm_op_conv3d(c.handle, _lib.ptr(xd), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), slope, _lib.ptr(wd), _lib.ptr(bd),
                                      COUT, 3, 1, 1, _lib.ptr(out), groups, _lib.ptr(gd), _lib.ptr(btd), _lib.ptr(gsc), _lib.ptr(gsh), 0), "op_conv3d")
        torch.cuda.synchronize()
    finally:
        _lib.check(c.lib.nm_set_conv_mode(c.handle, 1), "set_conv_mode")
    return out, gsc, gsh


def _family_counts(c):
    """profiled launches since nm_prof_enable: {family name: (launches, algorithmic FLOPs)}"""
    from neural_marionette_amd import _lib
    res = {}
    for v in range(16):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(c.lib.nm_prof_read(c.handle, v, C.byref(ms), C.byref(fl), C.byref(n)), "prof_read")
        if n.value:
            res[c.lib.nm_prof_kernel_name(v).decode()] = (n.value, fl.value)
    return res


_RANDOM = {}


def _random_case(N, dims, Cin):
    """operands of one shape, made once and shared by the bias / affine variants (never modified)"""
    key = (N, dims, Cin)
    if key not in _RANDOM:
        g = torch.Generator().manual_seed(X._seed("f16p8", key))
        x = torch.randn(N, Cin, *dims, generator=g)
        w = torch.randn(COUT, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
        b = torch.randn(COUT, generator=g) * 0.1
        sc = torch.rand(N, Cin, generator=g) + 0.5
        sh = torch.randn(N, Cin, generator=g) * 0.3
        gam = torch.rand(COUT, generator=g) + 0.5
        bet = torch.randn(COUT, generator=g) * 0.2
        _RANDOM[key] = dict(x=x, w=w, b=b, sc=sc, sh=sh, gam=gam, bet=bet, xd=to_cl(x), wd=dev(w), bd=dev(b), scd=dev(sc), shd=dev(sh),
                            gd=dev(gam), btd=dev(bet), ref={})
    return _RANDOM[key]


def _activated(d, affine, dtype):
    x = d["x"].to(dtype)
    if not affine:
        return x
    return F.leaky_relu(x * d["sc"].to(dtype)[:, :, None, None, None] + d["sh"].to(dtype)[:, :, None, None, None], SLOPE)


# ---- 1. fp64 parity ----------------------------------------------------------------------------------------------------------------
# two bricks and one chunk; two chunks, bricks along y; three chunks (halo-buffer and weight-buffer parity over an odd number of steps),
# bricks along x, three frames
PARITY_SHAPES = [(1, (16, 8, 8), 16), (2, (16, 16, 8), 32), (3, (24, 8, 16), 48)]


@pytest.mark.parametrize("affine", [False, True], ids=["raw", "affine"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N,dims,Cin", PARITY_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fp64_parity(ctx, N, dims, Cin, bias, affine):
    """stored output and the fused GroupNorm (returned scale / shift applied to the output) against F.conv3d / F.group_norm in double
    on the CPU, at the bound of test_ops_gpu.py::test_conv3d (REL = 2e-5 of the reference's largest magnitude)"""
    d = _random_case(N, dims, Cin)
    if (bias, affine) not in d["ref"]:
        ref = F.conv3d(_activated(d, affine, torch.float64), d["w"].double(), d["b"].double() if bias else None, padding=1)
        d["ref"][(bias, affine)] = (ref, F.group_norm(ref, GROUPS, d["gam"].double(), d["bet"].double(), 1e-5))
    ref, refn = d["ref"][(bias, affine)]
    out, gsc, gsh = _run(ctx, d["xd"], N, dims, Cin, d["scd"] if affine else None, d["shd"] if affine else None, SLOPE if affine else 1.0,
                         d["wd"], d["bd"] if bias else None, gd=d["gd"], btd=d["btd"])
    got = from_cl(out, COUT)
    assert torch.isfinite(got).all(), "unwritten / non-finite outputs"
    e = relerr(got.double(), ref)
    gotn = got.double() * gsc.cpu().double()[:, :, None, None, None] + gsh.cpu().double()[:, :, None, None, None]
    en = relerr(gotn, refn)
    print("N=%d dims=%s Cin=%d bias=%d affine=%d: raw %.3e, normalised %.3e (bound %.0e)" % (N, dims, Cin, bias, affine, e, en, REL))
    assert e < REL, f"conv raw output rel err {e:.3e}"
    assert en < REL, f"fused GroupNorm rel err {en:.3e}"


# ---- 2. several bricks per workgroup, frame changes inside a run -------------------------------------------------------------------
# Neither shape takes the XCD super-tile order (nby = 2 and nbz = 3 are no multiples of the super-tile), so a workgroup walks a
# contiguous run of per = ceil(bricks / 256) = 2 bricks in linear order, stepped by the kernel's next_work.
#   (40, 16^3): 8 bricks per frame, 320 bricks: workgroup b walks bricks 2b, 2b + 1 - always two x-neighbours of one frame (only the
#               x step of next_work); 160 workgroups busy, the trailing 96 idle.
#   (11, 24^3): 27 bricks per frame (3 x 3 x 3), 297 bricks: the runs start at even brick numbers while rows (3), planes (9) and frames
#               (27) are odd, so runs cross x -> y wraps, y -> z wraps (z stepped by 8) and frame changes (bricks 26 | 27 of frames
#               0 | 1, 80 | 81 of frames 2 | 3, ...: the inside mask of the tile being loaded is refreshed across a frame); the last
#               workgroup walks a single brick.
MANY_SHAPES = [(40, (16, 16, 16), 16), (11, (24, 24, 24), 16)]


def _runs_crossing(N, dims):
    """what the runs of two bricks cross in linear order: (x -> y wraps, y -> z wraps, frame changes)"""
    nbz, nby, nbx = (d // 8 for d in dims)
    total = N * nbz * nby * nbx
    assert 256 < total <= 512                                   # per == 2 on a 256-CU device
    cross = [0, 0, 0]
    for first in range(0, total - 1, 2):
        b = first + 1
        if b % (nbz * nby * nbx) == 0:
            cross[2] += 1
        elif b % (nby * nbx) == 0:
            cross[1] += 1
        elif b % nbx == 0:
            cross[0] += 1
    return tuple(cross)


@pytest.mark.parametrize("N,dims,Cin", MANY_SHAPES, ids=["40x16x16x16", "11x24x24x24"])
def test_more_bricks_than_workgroups(ctx, N, dims, Cin):
    """two bricks per workgroup (see MANY_SHAPES).  Reference: ATen fp32 on the CPU at REL, as test_ops_gpu.py::test_conv3d; the error
    is taken per frame so that a frame staged from the wrong place cannot hide behind the others."""
    cross = _runs_crossing(N, dims)
    print("runs of two bricks crossing (row, plane, frame):", cross)
    if dims == (24, 24, 24):
        assert min(cross) >= 2, cross                           # every wrap branch of next_work, and a frame change, inside runs
    else:
        assert cross == (0, 0, 0), cross
    g = torch.Generator().manual_seed(X._seed("f16p8-many", N, dims))
    x = torch.randn(N, Cin, *dims, generator=g)
    w = torch.randn(COUT, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
    b = torch.randn(COUT, generator=g) * 0.1
    sc = torch.rand(N, Cin, generator=g) + 0.5
    sh = torch.randn(N, Cin, generator=g) * 0.3
    gam, bet = torch.rand(COUT, generator=g) + 0.5, torch.randn(COUT, generator=g) * 0.2
    ref = F.conv3d(F.leaky_relu(x * sc[:, :, None, None, None] + sh[:, :, None, None, None], SLOPE), w, b, padding=1)
    refn = F.group_norm(ref, GROUPS, gam, bet, 1e-5)
    out, gsc, gsh = _run(ctx, to_cl(x), N, dims, Cin, dev(sc), dev(sh), SLOPE, dev(w), dev(b), gd=dev(gam), btd=dev(bet))
    got = from_cl(out, COUT)
    assert torch.isfinite(got).all(), "unwritten / non-finite outputs"
    per_frame = (got - ref).abs().amax(dim=(1, 2, 3, 4)) / ref.abs().max()
    print("worst frame %d: %.3e (bound %.0e)" % (int(per_frame.argmax()), per_frame.max().item(), REL))
    assert per_frame.max().item() < REL
    gotn = got * gsc.cpu()[:, :, None, None, None] + gsh.cpu()[:, :, None, None, None]
    per_frame_n = (gotn - refn).abs().amax(dim=(1, 2, 3, 4)) / refn.abs().max()
    assert per_frame_n.max().item() < REL, "fused GroupNorm, worst frame %d: %.3e" % (int(per_frame_n.argmax()), per_frame_n.max().item())


# ---- 3. bit-identity with conv_f16p ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True], ids=["raw", "affine"])
def test_bit_identical_to_conv_f16p(ctx, affine):
    """X at D = 16 (conv_f16p8) against X with four z-planes appended (D = 20: 20 % 8 == 4, conv_f16p).  The appended planes activate
    to exactly 0 - raw 0 without an affine; with one, scale a power of two and the raw value -shift / scale, so that fma(raw, scale,
    shift) == 0 - which is what conv_f16p8 sees as padding behind plane 15.  Planes z < 16 of the two outputs: torch.equal."""
    N, dims, Cin = 2, (16, 16, 16), 32
    g = torch.Generator().manual_seed(X._seed("f16p8-bits", affine))
    x = torch.randn(N, Cin, *dims, generator=g)
    w = torch.randn(COUT, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
    b = torch.randn(COUT, generator=g) * 0.1
    tail = torch.zeros(N, Cin, 4, *dims[1:])
    sc = sh = None
    if affine:
        sc = 2.0 ** torch.randint(-2, 3, (N, Cin), generator=g).float()
        sh = torch.randn(N, Cin, generator=g) * 0.3
        tail = tail + (-sh / sc)[:, :, None, None, None]                  # exact: a division by a power of two
        assert torch.equal(tail[:, :, 0, 0, 0] * sc + sh, torch.zeros(N, Cin))
    x20 = torch.cat([x, tail], dim=2)
    slope = SLOPE if affine else 1.0
    wd, bd, scd, shd = dev(w), dev(b), dev(sc), dev(sh)
    from neural_marionette_amd import _lib
    _lib.check(ctx.lib.nm_prof_enable(ctx.handle, 1), "prof_enable")
    gd, btd = dev(torch.ones(COUT)), dev(torch.zeros(COUT))
    out16, _, _ = _run(ctx, to_cl(x), N, dims, Cin, scd, shd, slope, wd, bd, gd=gd, btd=btd)
    out20, _, _ = _run(ctx, to_cl(x20), N, (20, *dims[1:]), Cin, scd, shd, slope, wd, bd, gd=gd, btd=btd)
    _lib.check(ctx.lib.nm_prof_enable(ctx.handle, 0), "prof_enable")
    fam = _family_counts(ctx)
    assert list(fam) == [FAMILY] and fam[FAMILY][0] == 2, fam
    assert torch.isfinite(out16).all() and torch.isfinite(out20).all()
    a, bb = out16, out20[:, :16]
    assert torch.equal(a, bb), "%d of %d stored values differ, largest difference %.3e" % (int((a != bb).sum()), a.numel(), (a - bb).abs().max().item())


# ---- 4. exact arithmetic -----------------------------------------------------------------------------------------------------------
def _spec(Cin, dims, N, prologue):
    return ("conv", Cin, COUT, 3, 1, 1, dims, N, prologue, False, GROUPS, 0)


EXACT_CASES = [(_spec(32, (16, 8, 16), 2, True), "sa"), (_spec(32, (16, 8, 16), 2, True), "dw"), (_spec(32, (16, 8, 16), 2, True), "r8"),
               (_spec(16, (24, 16, 8), 1, False), "sa"), (_spec(48, (16, 8, 8), 3, True), "r30")]


@pytest.mark.parametrize("spec,data", EXACT_CASES, ids=lambda v: v if isinstance(v, str) else "ci%d_d%s_N%d%s" % (v[1], "x".join(map(str, v[6])), v[7], "_pro" if v[8] else ""))
def test_exact_integer_convolution(ctx, spec, data):
    """small-integer operands (tests/exact_ref.py): the stored output equals the fp64 convolution bit for bit, two launches agree, and
    on the statistics sets scale / shift are within exact_ref's ulp bounds - the body of test_exact_arithmetic_gpu, conv mode 1"""
    TE._forward_body(ctx, (spec, data, 0, 0, (1,)))
    assert TE.KERNELS[(spec, 1, 0, 0)] == [FAMILY], TE.KERNELS[(spec, 1, 0, 0)]


@pytest.mark.parametrize("which", ["activations", "weights"])
def test_exact_with_nonzero_lo_halves(ctx, which):
    """operands that do not fit fp16, so the lo halves of the split carry a part of every product: activations of +-2049 and +-4098
    (hi 2048 / 4096, lo 1 / 2) against weights in {-1, 0, 1}, and weights of +-(1 + 2^-11) (hi 1, lo 2^-11) against integer
    activations.  One side keeps a zero lo half, so the dropped lo x lo term is 0 and every partial sum is a multiple of 2^-11 below
    2^12 (weights) or an integer below 2^24 (activations): the fp64 convolution is the only correct output."""
    N, dims, Cin = 2, (16, 8, 16), 32
    g = torch.Generator().manual_seed(X._seed("f16p8-lo", which))
    if which == "activations":
        x = X.sparse_ints((N, Cin, *dims), 0.1, 2, g) * 2049.0
        w = X.sparse_ints((COUT, Cin, 3, 3, 3), 0.5, 1, g)
        assert not X.fits(x, torch.float16) and X.fits(w, torch.float16)
        limit = 2.0 ** 24
    else:
        x = X.sparse_ints((N, Cin, *dims), 0.1, 2, g)
        w = X.sparse_ints((COUT, Cin, 3, 3, 3), 0.5, 1, g) * (1.0 + 2.0 ** -11)
        assert X.fits(x, torch.float16) and not X.fits(w, torch.float16)
        limit = 2.0 ** 12
    b = torch.randint(-3, 4, (COUT,), generator=g).float()
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    mag = F.conv3d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    assert float(mag.max()) < limit and torch.equal(ref.float().double(), ref)
    out, gsc, gsh = _run(ctx, to_cl(x), N, dims, Cin, None, None, 1.0, dev(w), dev(b), gd=dev(torch.ones(COUT)), btd=dev(torch.zeros(COUT)))
    got = from_cl(out, COUT)
    assert torch.equal(got, ref.float()), "%d stored values differ, largest difference %.3e" % (int((got != ref.float()).sum()), (got - ref.float()).abs().max().item())
    assert torch.isfinite(gsc).all() and torch.isfinite(gsh).all()


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------
def test_twenty_launches_agree(ctx):
    N, dims, Cin = 3, (24, 8, 16), 48
    d = _random_case(N, dims, Cin)
    first = None
    for i in range(20):
        res = _run(ctx, d["xd"], N, dims, Cin, d["scd"], d["shd"], SLOPE, d["wd"], d["bd"], gd=d["gd"], btd=d["btd"])
        if first is None:
            first = res
            continue
        for name, a, b in zip(("output", "GroupNorm scale", "GroupNorm shift"), first, res):
            assert torch.equal(a, b), "launch %d: %s differs from the first launch" % (i, name)


# ---- 6. routing --------------------------------------------------------------------------------------------------------------------
def _conv_flops(N, dims, Cin):
    return 2.0 * N * dims[0] * dims[1] * dims[2] * COUT * Cin * 27.0


def test_routing_of_op_level_calls(ctx):
    """conv mode 1: D = 16 and D = 20 both file under family 7 (one launch each, told apart by their FLOPs; D = 20 can only have run
    on conv_f16p - its parity below covers all 20 planes).  Conv mode 3 ('f16') keeps the one-product kernel of these layers."""
    from neural_marionette_amd import _lib
    N, Cin = 2, 32
    g = torch.Generator().manual_seed(X._seed("f16p8-route"))
    w = torch.randn(COUT, Cin, 3, 3, 3, generator=g) / (Cin * 27) ** 0.5
    wd = dev(w)
    seen = {}
    for D, mode in ((16, 1), (20, 1), (16, 3)):
        dims = (D, 16, 16)
        x = torch.randn(N, Cin, *dims, generator=g)
        _lib.check(ctx.lib.nm_prof_enable(ctx.handle, 1), "prof_enable")
        out, _, _ = _run(ctx, to_cl(x), N, dims, Cin, None, None, 1.0, wd, None, mode=mode)
        _lib.check(ctx.lib.nm_prof_enable(ctx.handle, 0), "prof_enable")
        seen[(D, mode)] = _family_counts(ctx)
        e = relerr(from_cl(out, COUT), F.conv3d(x, w, None, padding=1))
        assert e < (REL if mode == 1 else 3e-3), (D, mode, e)
    print(seen)
    for D in (16, 20):
        fam = seen[(D, 1)]
        assert list(fam) == [FAMILY], fam
        assert fam[FAMILY][0] == 1 and fam[FAMILY][1] == _conv_flops(N, (D, 16, 16), Cin), fam
    # (the resident-weight kernel; with its launch switch off, the one-product instantiation of conv_f16p)
    f16 = seen[(16, 3)]
    assert list(f16) in (["conv_f16r_kernel"], [FAMILY]) and list(f16.values())[0] == (1, _conv_flops(N, (16, 16, 16), Cin)), f16


def test_decoder_layer_of_a_forward_takes_family_7():
    """(B 1, T 2) inference forward at 64^3: the decoder's last 3 x 3 x 3 layer (32 -> 32 at 64^3, two frames) is a family-7 launch with
    whole 8 x 8 x 8 bricks in conv mode 1 with fp32 storage - the shape nm_launch_conv sends to conv_f16p8"""
    from test_network_gpu import ACTS, _net
    from neural_marionette_amd import HotPathOptions, synth, _lib
    o = HotPathOptions(grid_size=64)
    sd = synth.make_state_dict(o, seed=8, variant="peaky")
    vox = synth.figure_clip(1, 2, 64, seed=10).cuda()
    eps = synth.make_eps((2, 10, 1, o.nlatent_kypt), seed=9).cuda()
    net = _net(o, sd)
    with torch.no_grad():
        net(vox, ACTS, eps=eps)
        torch.cuda.synchronize()
        c = net._engine.ctx
        _lib.check(c.lib.nm_prof_enable(c.handle, 2), "prof_enable")
        net(vox, ACTS, eps=eps)
        torch.cuda.synchronize()
        _lib.check(c.lib.nm_prof_enable(c.handle, 0), "prof_enable")
    fam = _family_counts(c)
    print(fam)
    assert FAMILY in fam, fam
    n, fl = fam[FAMILY]
    layer = _conv_flops(2, (64, 64, 64), 32)
    # exactly one family-7 launch of the 64^3 layer's size; any other launch of the family is a coarser level, at most an eighth of it
    assert layer <= fl <= layer + (n - 1) * layer / 8.0, fam
