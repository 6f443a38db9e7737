"""Exact-arithmetic parity of the conv kernel families and their GroupNorm statistics (tests/exact_ref.py).

The operands are small integers (or integers times a stated power of two), so every product and partial sum is exactly representable:
fp32 MFMA, split-fp16, one-product f16 and bf16 storage must return the SAME BITS as the fp64 reference, in any summation order and
brick partition - `torch.equal`, no tolerance.  The (sum, sum of squares) partials are exact integers too, so scale / shift of the fused
GroupNorm are pinned to a few ulp (exact_ref.SCALE_ULPS / SHIFT_EPS, derived from the finaliser's operation order) at a group mean
of 0, 8 and 30 standard deviations.  Every case asserts exact_ref's preconditions before it touches the device; the same cases are
checked on the CPU (ATen fp32 == fp64, mutations outside the bounds) in tests/test_exact_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import test_grad_ops_gpu as TG
import test_many_frames_gpu as TM
import test_ops_gpu as TO
import test_storage16_gpu as TS
from test_ops_gpu import ctx, to_cl, from_cl, relerr, dev  # noqa: F401  (ctx is a fixture)

pytestmark = pytest.mark.gpu

REL = TO.REL
BF = torch.bfloat16


def _params(fn):
    """The argument tuples of a test's parametrize mark whose names start with a shape (the project's own sized lists)."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] not in ("mode", "sparse"):
            return list(m.args[1])
    raise LookupError(fn.__name__)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# spec = (kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, groups, outpad)
def _conv_spec(c):
    Cin, Cout, ks, stride, pad, size, N, prologue, groups = c
    return ("conv", Cin, Cout, ks, stride, pad, (size,) * 3, N, prologue, False, groups, 0)


ADDED_CONV = [
    # ragged 8x8x8 bricks at the sizes where a 2e-5 tolerance is weakest: k3 at 12^3, 20^3, 24^3 with Cout 32 (conv_f16r), 64 (conv_f16p2 / q2), 72
    (32, 32, 3, 1, 1, 12, 2, True, 2), (32, 64, 3, 1, 1, 12, 1, False, 4), (32, 72, 3, 1, 1, 12, 2, True, 4),
    (32, 32, 3, 1, 1, 20, 1, False, 2), (32, 64, 3, 1, 1, 20, 2, True, 4), (16, 72, 3, 1, 1, 20, 1, True, 4),
    (16, 32, 3, 1, 1, 24, 1, True, 2), (32, 64, 3, 1, 1, 24, 1, True, 4), (16, 72, 3, 1, 1, 24, 2, False, 4),
    # Cout not a multiple of 32 nor of 8 x (channels per group): 40 = 5 x 8, 24 = 3 x 8, 48 = 3 x 16; N = 1
    (32, 40, 3, 1, 1, 12, 1, True, 5), (16, 24, 3, 1, 1, 20, 1, False, 3), (64, 48, 3, 1, 1, 16, 1, True, 3),
    (32, 40, 2, 2, 0, 12, 1, True, 5), (64, 24, 1, 1, 0, 9, 1, True, 3),
]
CONV_SPECS = list(dict.fromkeys(_conv_spec(c) for c in TO.CONV_CASES + ADDED_CONV))
UP2_SPECS = list(dict.fromkeys(
    [("conv", Cin, Cout, 3, 1, 1, (size,) * 3, N, prologue, True, Cout // 16, 0) for Cin, Cout, size, prologue, N in _params(TO.test_conv3d_fused_upsample)] +
    [("conv", 64, 32, 3, 1, 1, tuple(dims), N, prologue, True, 2, 0) for dims, prologue, N in _params(TO.test_conv3d_fused_upsample_composite)]))
COMPOSITE_DIMS = [tuple(p[0]) for p in _params(TO.test_conv3d_fused_upsample_composite)]
# 16-bit storage: (spec, in16, out16)
S16_SPECS = [(("conv", c[0], c[1], c[2], c[3], c[4], (c[5],) * 3, c[6], True, bool(c[7]), c[1] // 16, 0), c[8], c[9]) for c in TS.FWD_CASES]
ADDED_CONVT = [
    (32, 16, 32, 0, 1, 2),      # convT2_lds_kernel: Cout % 32 != 0 keeps the matrix-core branches away, 65536 coarse voxels, 256 % (Cout / 4) == 0
    (16, 24, 4, 1, 3, 1),       # output_padding 1, N = 1, Cout = 3 x 8
    (64, 32, 7, 1, 2, 2),       # output_padding 1 with matrix-core-sized channels: the generic kernel must take it
]
CONVT_SPECS = list(dict.fromkeys(("convT", Cin, Cout, 2, 2, 0, (size,) * 3, N, False, False, groups, outpad)
                                 for Cin, Cout, size, outpad, groups, N in _params(TO.test_convT2) + ADDED_CONVT))

STAT_SETS = ("r0", "r8", "r30", "const")


def forward_cases():
    """Every (spec, data set, in16, out16, modes) the forward tests run; tests/test_exact_ref_cpu.py walks the same list on the CPU."""
    out = []
    for s in CONV_SPECS + CONVT_SPECS:
        for data in ("sa", "dw") + (STAT_SETS if s[10] > 0 else ()):
            out.append((s, data, 0, 0, (0, 1, 2, 3)))
    for s in UP2_SPECS:
        for data in ("sa", "dw", "chan"):
            out.append((s, data, 0, 0, (0, 1, 2, 3)))
    for s, ih, oh in S16_SPECS:
        out.append((s, "b16", ih, oh, (3, 4)))
    return out


def _fid(c):
    s, data, ih, oh, _ = c
    return "%s_ci%d_co%d_k%d_s%d_d%s_N%d%s%s%s_%s%s" % (s[0], s[1], s[2], s[3], s[4], "x".join(map(str, s[6])), s[7], "_pro" if s[8] else "", "_up" if s[9] else "",
                                                    "_op" if s[11] else "", data, "_io%d%d" % (ih, oh) if (ih or oh) else "")


# spec = (kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, outpad)
BWD_SPECS = list(dict.fromkeys(("conv", c[0], c[1], c[2], c[3], c[4], (c[5],) * 3, c[6], c[7], c[8], 0) + (c[9],) for c in TG.BWD_CASES))
BWDT_SPECS = [("convT", Cin, Cout, 2, 2, 0, (size,) * 3, N, prologue, False, outpad, Cin) for Cin, Cout, size, outpad, prologue, N in _params(TG.test_convT2_backward)]
BWD16_SPECS = [(("conv", c[0], c[1], c[2], c[3], c[4], (c[5],) * 3, c[6], True, bool(c[7]), 0, c[8]), c[9], c[10]) for c in TS.BWD_CASES]
# past 96 frames, at the smallest volume that still splits into frame groups (test_many_frames_gpu): 97 and 240 frames
MANY_SPECS = [("conv",) + TM.K3[:5] + (TM.K3[5], N, True, False, 0, TM.K3[0]) for N in (97, 240)] + \
             [("conv",) + TM.K3_RAGGED[:5] + (TM.K3_RAGGED[5], 97, True, False, 0, TM.K3_RAGGED[0])]


def backward_cases():
    """(spec + (dgrad channels,), in16, out16, modes, with_d_in)"""
    out = [(s, 0, 0, (0, 1, 3), True) for s in BWD_SPECS + BWDT_SPECS + MANY_SPECS]
    out += [(s, ih, oh, (4,), True) for s, ih, oh in BWD16_SPECS]
    out += [(s, 1, 1, (4,), False) for s in MANY_SPECS]
    return out


def _bid(c):
    s, ih, oh, modes, _ = c
    return "%s_ci%d_co%d_k%d_s%d_d%s_N%d%s%s%s%s" % (s[0], s[1], s[2], s[3], s[4], "x".join(map(str, s[6])), s[7], "_pro" if s[8] else "", "_up" if s[9] else "",
                                                   "_op" if s[10] else "", "_io%d%d" % (ih, oh) if 4 in modes else "")


OCC_CASES = _params(TO.test_conv5_occupancy_first_layer)                     # (G, Cout, N) at G = 16, 24, 32
OCC_BWD_CASES = _params(TG.test_conv5_occ_backward)
GNB_CASES = list(dict.fromkeys(_params(TG.test_gn_backward) + [(32, 2, 16, 2, 0.01), (64, 4, 8, 3, 0.01)]))
GNB_RATIOS = (0, 8, 32)


# ---- device helpers ----------------------------------------------------------------------------------------------------------------
def _set(c, mode, ih=0, oh=0):
    from neural_marionette_amd import _lib
    _lib.check(c.lib.nm_set_conv_mode(c.handle, mode), "set_conv_mode")
    _lib.check(c.lib.nm_op_set_storage16(c.handle, ih, oh), "op_set_storage16")


def _pad_rows(t, cp):
    if t is None:
        return None
    p = torch.zeros(t.shape[0], cp)
    p[:, :t.shape[1]] = t
    return p


KERNELS = {}


def _prof_names(c):
    from neural_marionette_amd import _lib
    names = []
    for v in range(16):
        ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
        _lib.check(c.lib.nm_prof_read(c.handle, v, C.byref(ms), C.byref(fl), C.byref(n)), "prof_read")
        if n.value:
            names.append(c.lib.nm_prof_kernel_name(v).decode())
    return names


class _Forward:
    """One forward case on the device: operands uploaded once, launched per mode."""
    def __init__(self, c, d, gam=None, bet=None):
        s = d["spec"]
        self.c, self.d, self.s = c, d, s
        cp = (s[1] + 7) // 8 * 8
        self.x32 = to_cl(d["x"])
        self.xbf = None
        self.w, self.b = dev(d["w"]), dev(d["b"])
        self.sc, self.sh = dev(_pad_rows(d["sc"], cp)), dev(_pad_rows(d["sh"], cp))
        self.gam, self.bet = dev(d["gam"] if gam is None else gam), dev(d["bet"] if bet is None else bet)

    def run(self, mode, ih=0, oh=0, profile=False):
        from neural_marionette_amd import _lib
        c, d = self.c, self.d
        kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, groups, outpad = self.s
        lib, h = c.lib, c.handle
        x = self.x32
        if ih:
            if self.xbf is None:
                self.xbf = self.x32.to(BF)
            x = self.xbf
        if oh:
            out = torch.full((N, *d["od"], Cout), float("nan"), dtype=BF, device="cuda")
        else:
            out = torch.full((N, *d["od"], Cout), float("nan")).cuda()
        gsc = torch.full((N, Cout), float("nan")).cuda(); gsh = torch.full((N, Cout), float("nan")).cuda()
        _set(c, mode, ih, oh)
        try:
            if profile:
                _lib.check(lib.nm_prof_enable(h, 1), "prof_enable")
            if kind == "convT":
                _lib.check(lib.nm_op_convT2(h, _lib.ptr(x), N, *dims, Cin, _lib.ptr(self.w), _lib.ptr(self.b), Cout, outpad, _lib.ptr(out), groups,
                                            _lib.ptr(self.gam), _lib.ptr(self.bet), _lib.ptr(gsc), _lib.ptr(gsh)), "op_convT2")
            else:
                _lib.check(lib.nm_op_conv3d(h, _lib.ptr(x), N, *dims, Cin, _lib.ptr(self.sc), _lib.ptr(self.sh), d["slope"], _lib.ptr(self.w), _lib.ptr(self.b),
                                            Cout, ks, stride, pad, _lib.ptr(out), groups, _lib.ptr(self.gam), _lib.ptr(self.bet), _lib.ptr(gsc), _lib.ptr(gsh),
                                            int(up2)), "op_conv3d")
            torch.cuda.synchronize()
            if profile:
                _lib.check(lib.nm_prof_enable(h, 0), "prof_enable")
                KERNELS[(self.s, mode, ih, oh)] = _prof_names(c)
        finally:
            _set(c, 1, 0, 0)
        return out, gsc, gsh


def _check_stats(gsc, gsh, ref, what):
    sc, sh = gsc.cpu().double().numpy(), gsh.cpu().double().numpy()
    assert np.isfinite(sc).all() and np.isfinite(sh).all(), what
    es, eh = X.stats_errors(sc, sh, ref)
    print("%s: scale error %.2f of %g ulp, shift error %.2f of its bound" % (what, es * X.SCALE_ULPS, X.SCALE_ULPS, eh))
    assert es <= 1.0, f"{what}: scale off by {es * X.SCALE_ULPS:.2f} ulp (bound {X.SCALE_ULPS})"
    assert eh <= 1.0, f"{what}: shift error {eh:.2f} times the bound 4 * 2^-23 * max(|scale mean|, |beta|)"


# ---- forward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", forward_cases(), ids=_fid)
def test_forward_bits_and_statistics(ctx, case):
    """Stored output: bit-identical to the fp64 reference in conv modes 0-3 (and mode 4 with 16-bit storage for the storage cases), a
    second launch bit-identical to the first.  Statistics: on the sets whose per-(frame, channel) sum of squares is below 2^24
    ("r0" / "r8" / "r30": group mean at about 0 / 8 / 30 standard deviations; "const": variance exactly 0; "chan": fused-upsample layer on a
    per-channel constant) scale within 2 ulp and shift within 4 * 2^-23 * max(|scale mean|, |beta|) of the fp64 values from the exact
    sums, and with gamma = 1, beta = 0 scale within 1 ulp of float(rstd).  The general exact input of a fused-upsample layer ("sa" / "dw"
    with up2) is the weaker case: its outputs are multiples of 1/8 whose squares summed over a frame exceed 2^24, so the fp32 partials
    round - stored output exact, statistics at REL = 2e-5 on the normalised output as in test_ops_gpu."""
    _forward_body(ctx, case)


def _forward_body(ctx, case):
    spec, data, ih, oh, modes = case
    d = X.make_forward(spec, data)
    facts = X.preconditions(d, in16=bool(ih), out16=bool(oh))
    exact_stats = spec[10] > 0 and (data in STAT_SETS or data == "chan")
    X.assert_preconditions(facts, stats=exact_stats)
    want = d["y"].float()
    ref = X.reference_stats(d) if spec[10] > 0 else None
    Cout, groups = spec[2], spec[10]
    fw = _Forward(ctx, d)
    for mode in modes:
        mih, moh = (ih, oh) if mode == 4 else (0, 0)
        what = "%s mode %d" % (_fid(case), mode)
        out, gsc, gsh = fw.run(mode, mih, moh, profile=True)
        print(what, "->", ", ".join(KERNELS[(spec, mode, mih, moh)]) or "(no profiled variant)")
        got = from_cl(out.float(), Cout)
        assert torch.isfinite(got).all(), f"{what}: unwritten / non-finite outputs"
        nbad = int((got != want).sum())
        assert torch.equal(got, want), f"{what}: {nbad} of {want.numel()} stored values differ, largest difference {(got - want).abs().max().item():.3e}"
        out2, gsc2, gsh2 = fw.run(mode, mih, moh)
        assert torch.equal(out, out2) and (not groups or (torch.equal(gsc, gsc2) and torch.equal(gsh, gsh2))), f"{what}: two launches differ"
        if not groups:
            continue
        if exact_stats:
            _check_stats(gsc, gsh, ref, what)
            if data == "const":
                # got * scale + shift == beta within the shift bound; scale = gamma / sqrt(eps) is what the scale bound above pins
                n = got.double() * gsc.cpu().double()[:, :, None, None, None] + gsh.cpu().double()[:, :, None, None, None]
                bound = X.SHIFT_EPS * np.maximum(np.abs(ref["scale"] * ref["meanc"]), np.abs(ref["bet"])[None])
                err = (n - d["bet"].double()[None, :, None, None, None]).abs().amax(dim=(2, 3, 4)).numpy()
                assert (err <= bound).all(), f"{what}: normalised constant off by {err.max():.3e}"
        else:
            refn = F.group_norm(d["y"], groups, d["gam"].double(), d["bet"].double(), X.EPS).float()
            e = relerr(got * gsc.cpu()[:, :, None, None, None] + gsh.cpu()[:, :, None, None, None], refn)
            assert e < REL, f"{what}: fused GroupNorm rel err {e:.3e}"
    if exact_stats and data in ("r8", "r30", "chan"):
        # gamma = 1, beta = 0: scale = (float)rstd * 1.0f is ONE rounding of the fp64 rstd
        one = _Forward(ctx, d, gam=torch.ones(Cout), bet=torch.zeros(Cout))
        _, gsc, gsh = one.run(1)
        r1 = X.stats_from_sums(*X.group_sums(d["y"], groups), np.ones(Cout), np.zeros(Cout))
        es, eh = X.stats_errors(gsc.cpu().double().numpy(), gsh.cpu().double().numpy(), r1, scale_ulps=1.0)
        assert es <= 1.0 and eh <= 1.0, f"{_fid(case)}: gamma = 1, beta = 0: scale {es:.2f} ulp from float(rstd), shift {eh:.2f} of its bound"


@pytest.mark.parametrize("G,Cout,N", OCC_CASES)
def test_first_layer_bits_and_statistics(ctx, G, Cout, N):
    """conv5 on cat[occ, coords] with integer weights on the occupancy channel and zero weights on the coordinate channels (the
    constant field is the bias): 0 / 1 occupancy and a fractional 0.5 / 0.25 frame; stored output and statistics exact in modes 0-3.
    Non-zero coordinate weights stay with the tolerance test of test_ops_gpu."""
    from neural_marionette_amd import _lib
    d = X.make_occ(G, Cout, N)
    facts = X.occ_preconditions(d)
    X.assert_preconditions(facts, stats=True)
    assert facts["coordinate_weights_zero"]
    ref = X.reference_stats(d)
    want = d["y"].float()
    groups = d["groups"]
    od, wd, bd, gd, btd = d["occ"].reshape(N, G, G, G).contiguous().cuda(), dev(d["w"]), dev(d["b"]), dev(d["gam"]), dev(d["bet"])
    for mode in (0, 1, 2, 3):
        res = []
        for _ in range(2):
            out = torch.full((N, G, G, G, Cout), float("nan")).cuda()
            gsc = torch.full((N, Cout), float("nan")).cuda(); gsh = torch.full((N, Cout), float("nan")).cuda()
            _set(ctx, mode)
            try:
                _lib.check(ctx.lib.nm_op_conv5_occ(ctx.handle, _lib.ptr(od), N, G, _lib.ptr(wd), _lib.ptr(bd), Cout, _lib.ptr(out), groups, _lib.ptr(gd),
                                                   _lib.ptr(btd), _lib.ptr(gsc), _lib.ptr(gsh)), "op_conv5_occ")
                torch.cuda.synchronize()
            finally:
                _set(ctx, 1)
            res.append((out, gsc, gsh))
        (out, gsc, gsh), (out2, gsc2, gsh2) = res
        got = from_cl(out, Cout)
        what = "conv5_occ G=%d Cout=%d N=%d mode %d" % (G, Cout, N, mode)
        assert torch.equal(got, want), f"{what}: {int((got != want).sum())} stored values differ, largest {(got - want).abs().max().item():.3e}"
        assert torch.equal(out, out2) and torch.equal(gsc, gsc2) and torch.equal(gsh, gsh2), f"{what}: two launches differ"
        _check_stats(gsc, gsh, ref, what)


# ---- backward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", backward_cases(), ids=_bid)
def test_backward_bits(ctx, case):
    """d_weight, d_bias and d_in of nm_op_conv3d_backward / nm_op_convT2_backward on exact x and sparse integer dy: bit-identical to fp64
    autograd in conv modes 0, 1 and 3, in mode 4 with the 16-bit storage combinations of test_storage16_gpu, and past 96 frames (97 and
    240: the weight gradient runs over groups of frames).  Fused-upsample cases go through the upsample adjoint (coefficients k/64:
    d_in is a multiple of 1/64, which the preconditions check)."""
    from neural_marionette_amd import _lib
    spec, ih, oh, modes, with_d_in = case
    d = X.make_backward(spec[:11], lean=bool(spec[9] and (ih or oh)))
    csel = spec[11]
    X.assert_backward_preconditions(X.backward_preconditions(d, in16=bool(ih), out16=bool(oh)))
    kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, outpad = spec[:11]
    cp = (Cin + 7) // 8 * 8
    x32, dy32, wd = to_cl(d["x"]), to_cl(d["dy"], Cout), dev(d["w"])
    scd, shd = dev(_pad_rows(d["sc"], cp)), dev(_pad_rows(d["sh"], cp))
    for mode in modes:
        mih, moh = (ih, oh) if mode == 4 else (0, 0)
        xin = x32.to(BF) if mih else x32
        dyin = dy32.to(BF) if moh else dy32
        d_in = torch.full((N, *dims, csel), float("nan"), dtype=BF if mih else torch.float32, device="cuda") if with_d_in else None
        d_w = torch.full(d["w"].shape, float("nan")).cuda(); d_b = torch.full((Cout,), float("nan")).cuda()
        _set(ctx, mode, mih, moh)
        try:
            if kind == "convT":
                _lib.check(ctx.lib.nm_op_convT2_backward(ctx.handle, _lib.ptr(xin), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), d["slope"], _lib.ptr(wd), Cout,
                                                         outpad, _lib.ptr(dyin), _lib.ptr(d_in), _lib.ptr(d_w), _lib.ptr(d_b)), "op_convT2_backward")
            else:
                _lib.check(ctx.lib.nm_op_conv3d_backward(ctx.handle, _lib.ptr(xin), N, *dims, Cin, _lib.ptr(scd), _lib.ptr(shd), d["slope"], _lib.ptr(wd), Cout,
                                                         ks, stride, pad, int(up2), _lib.ptr(dyin), _lib.ptr(d_in) if with_d_in else None, csel,
                                                         _lib.ptr(d_w), _lib.ptr(d_b)), "op_conv3d_backward")
            torch.cuda.synchronize()
        finally:
            _set(ctx, 1, 0, 0)
        got = [("d_weight", d_w.cpu(), d["d_w"].float()), ("d_bias", d_b.cpu(), d["d_b"].float())]
        if with_d_in:
            got.append(("d_in", from_cl(d_in.float(), csel), d["d_a"][:, :csel].float()))
        for name, g, want in got:
            what = "%s mode %d %s" % (_bid(case), mode, name)
            assert torch.isfinite(g).all(), f"{what}: unwritten / non-finite"
            assert torch.equal(g, want), f"{what}: {int((g != want).sum())} of {want.numel()} values differ, largest difference {(g - want).abs().max().item():.3e}"


@pytest.mark.parametrize("sparse", [1, 2, 0], ids=["mfma-bricks", "gather", "dense"])
@pytest.mark.parametrize("Cout,G,N,frac", OCC_BWD_CASES)
def test_first_layer_backward_bits(ctx, Cout, G, N, frac, sparse):
    """nm_op_conv5_occ_backward in its three forms: occupancy 0 / 1 (or 0.5 / 0.25 where the existing case is fractional), dy sparse
    integers: the occupancy channel's weight gradient and the bias gradient are exact integers / quarters and must match bit for bit;
    the coordinate channels' gradient (dy against the linspace coordinates, not exact) keeps REL."""
    from neural_marionette_amd import _lib

    def make():
        g = torch.Generator().manual_seed(X._seed("occb", Cout, G, N, frac))
        occ = (torch.rand(N, 1, G, G, G, generator=g) < 0.05).float()
        if frac:
            occ = occ * (0.25 * torch.randint(1, 3, occ.shape, generator=g).float())
        if G >= 24:
            box = torch.zeros_like(occ); box[:, :, G // 3:G // 3 + 9, 5:G // 2, G // 2 - 3:G - 6] = 1.0
            occ = occ * box
        lin = torch.linspace(-1.0, 1.0, G)
        zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
        coords = torch.stack([zz, yy, xx])[None].expand(N, -1, -1, -1, -1)
        w = torch.zeros(Cout, 4, 5, 5, 5, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
        dy = X.sparse_ints((N, Cout, G, G, G), min(0.2, 8.0 / G ** 1.5), 2, g)
        F.conv3d(torch.cat([occ, coords], dim=1).double(), w, b, padding=2).backward(dy.double())
        mag = F.conv3d(occ.transpose(0, 1).double(), dy.transpose(0, 1).double().abs(), padding=2)      # sum |occ| |dy| per weight element
        return occ, dy, w.grad, b.grad, float(mag.max()) * 4, float(dy.abs().sum(dim=(0, 2, 3, 4)).max())
    occ, dy, rw, rb, mw, mb = X.cached(("occb", Cout, G, N, frac), make)
    assert X.fits(occ, torch.float16) and X.fits(dy, torch.float16) and mw < X.LIMIT and mb < X.LIMIT
    d_w = torch.full(rw.shape, float("nan")).cuda(); d_b = torch.full((Cout,), float("nan")).cuda()
    occd, dyd = occ[:, 0].contiguous().cuda(), to_cl(dy, Cout)
    _lib.check(ctx.lib.nm_op_conv5_occ_backward(ctx.handle, _lib.ptr(occd), N, G, Cout, _lib.ptr(dyd), _lib.ptr(d_w), _lib.ptr(d_b), sparse), "op_conv5_occ_backward")
    torch.cuda.synchronize()
    gw = d_w.cpu()
    assert torch.equal(gw[:, 0], rw[:, 0].float()), "occupancy channel: largest difference %.3e" % (gw[:, 0] - rw[:, 0].float()).abs().max().item()
    assert torch.equal(d_b.cpu(), rb.float())
    assert relerr(gw[:, 1:].double(), rw[:, 1:]) < REL


# ---- GroupNorm backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", GNB_RATIOS)
@pytest.mark.parametrize("C,groups,size,N,slope", GNB_CASES)
def test_gn_backward_offset_data(ctx, C, groups, size, N, slope, ratio):
    """nm_op_gn_backward on y = integer offset + integer noise (exact per-(frame, channel) sums) at mean / std of 0, about 8 and about
    32, against fp64 autograd at the file's REL = 2e-5, same four outputs and normalisation as test_gn_backward.  The bound is unchanged
    because the statistics are exact: what remains is the fp32 evaluation of y * scale + shift, whose error relative to the gradient's
    max is about 2^-24 * (r + 4) - an order of magnitude under REL for r <= 32."""
    from neural_marionette_amd import _lib
    d = X.make_gn_backward(C, groups, size, N, slope, ratio)
    assert d["sums_exact"]
    V = size ** 3
    dy = torch.full((N, size, size, size, C), float("nan")).cuda()
    dg = torch.zeros(C).cuda(); db = torch.zeros(C).cuda(); dbias = torch.zeros(C).cuda()
    yd, gd, bd, dAd = to_cl(d["y"], C), dev(d["gam"]), dev(d["bet"]), to_cl(d["dA"], C)
    _lib.check(ctx.lib.nm_op_gn_backward(ctx.handle, _lib.ptr(yd), N, V, C, groups, _lib.ptr(gd), _lib.ptr(bd), slope, _lib.ptr(dAd), _lib.ptr(dy),
                                         _lib.ptr(dg), _lib.ptr(db), _lib.ptr(dbias)), "op_gn_backward")
    torch.cuda.synchronize()
    ref_bias = d["dy"].sum(dim=(0, 2, 3, 4))
    e = (relerr(from_cl(dy, C).double(), d["dy"]), relerr(dg.cpu().double(), d["dgam"]), relerr(db.cpu().double(), d["dbet"]),
         (dbias.cpu().double() - ref_bias).abs().max().item() / max(d["dy"].abs().sum(dim=(0, 2, 3, 4)).max().item(), 1e-30))
    print("gn backward C=%d groups=%d %d^3 N=%d mean/std %d: dy %.2e dgamma %.2e dbeta %.2e dbias %.2e (bound %.0e)" % (C, groups, size, N, ratio, *e, REL))
    assert torch.isfinite(dy).all()
    assert max(e) < REL, e


# ---- elementwise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("V", [1, 125, 4096, 32768])
@pytest.mark.parametrize("Cc", [4, 8, 48, 128])
def test_apply2_bits(ctx, Cc, V, N):
    """lrelu(a * sa + ha, 0.25) + (b * sb + hb) and the one-source form on dyadic operands (integers, scale in {1, 2}, integer shift):
    every step is exact, so fp32 and the bf16 in / out combinations equal the CPU bit for bit."""
    from neural_marionette_amd import _lib
    if N * V * Cc > 3 * 32768 * 128:
        N = 3 * 32768 * 128 // (V * Cc)       # (nothing larger than the largest tensor of the reused lists)
    g = torch.Generator().manual_seed(X._seed("apply2", Cc, V, N))
    a = torch.randint(-12, 13, (N, V, Cc), generator=g).float() * 4; b = torch.randint(-30, 31, (N, V, Cc), generator=g).float()
    sa = torch.randint(1, 3, (N, Cc), generator=g).float(); ha = torch.randint(-2, 3, (N, Cc), generator=g).float() * 4
    sb = torch.randint(1, 3, (N, Cc), generator=g).float(); hb = torch.randint(-5, 6, (N, Cc), generator=g).float()
    ref2 = F.leaky_relu(a * sa[:, None] + ha[:, None], 0.25) + (b * sb[:, None] + hb[:, None])
    ref1 = F.leaky_relu(a * sa[:, None] + ha[:, None], 0.25)
    assert X.fits(a, BF) and X.fits(b, BF) and X.fits(ref2, BF) and X.fits(ref1, BF) and X.is_multiple(ref2, 0)
    sad, had, sbd, hbd = dev(sa), dev(ha), dev(sb), dev(hb)
    try:
        for ih, oh in ((0, 0), (1, 1), (1, 0), (0, 1)):
            _set(ctx, 4 if (ih or oh) else 1, ih, oh)
            ad, bd_ = (a.to(BF).cuda(), b.to(BF).cuda()) if ih else (a.cuda(), b.cuda())
            for two in (True, False):
                out = torch.full((N, V, Cc), float("nan"), dtype=BF if oh else torch.float32, device="cuda")
                if two:
                    _lib.check(ctx.lib.nm_op_apply2(ctx.handle, _lib.ptr(ad), _lib.ptr(sad), _lib.ptr(had), 0.25, _lib.ptr(bd_), _lib.ptr(sbd), _lib.ptr(hbd), 1.0,
                                                    N, V, Cc, _lib.ptr(out)), "apply2")
                else:
                    _lib.check(ctx.lib.nm_op_apply2(ctx.handle, _lib.ptr(ad), _lib.ptr(sad), _lib.ptr(had), 0.25, None, None, None, 1.0, N, V, Cc, _lib.ptr(out)), "apply2")
                torch.cuda.synchronize()
                assert torch.equal(out.float().cpu(), ref2 if two else ref1), "apply2 %s-source form, storage (%d, %d)" % ("two" if two else "one", ih, oh)
    finally:
        _set(ctx, 1, 0, 0)


@pytest.mark.parametrize("dims,Cc,N", [((2, 4, 4), 32, 1), ((4, 8, 12), 64, 2), ((6, 4, 20), 32, 3), ((8, 8, 8), 128, 2),          # LDS-tiled kernel
                                       ((3, 4, 4), 32, 2), ((2, 6, 4), 32, 1), ((4, 4, 5), 64, 2), ((4, 8, 8), 24, 2), ((1, 1, 1), 8, 3), ((5, 3, 7), 4, 1)])
def test_upsample2_bits(ctx, dims, Cc, N):
    """Trilinear x2 (align_corners = False) on multiples of 64: every coefficient product (k/64) and their sums are integers, so both
    kernels (LDS tiles: C % 32 == 0, D % 2 == 0, H % 4 == 0, W % 4 == 0; one cell per thread otherwise) equal F.interpolate bit for bit,
    in fp32 and with bf16 on either side."""
    from neural_marionette_amd import _lib
    D, H, W = dims
    g = torch.Generator().manual_seed(X._seed("up2", dims, Cc, N))
    x = torch.randint(-3, 4, (N, Cc, D, H, W), generator=g).float() * 64
    ref = F.interpolate(x.double(), scale_factor=2.0, mode="trilinear", align_corners=False)
    assert X.is_multiple(ref, 0) and X.fits(ref.float(), BF) and X.fits(x, BF)
    assert torch.equal(F.interpolate(x, scale_factor=2.0, mode="trilinear", align_corners=False).double(), ref)
    x32 = to_cl(x, Cc)
    try:
        for ih, oh in ((0, 0), (0, 1), (1, 1), (1, 0)):
            _set(ctx, 4 if (ih or oh) else 1, ih, oh)
            xin = x32.to(BF) if ih else x32
            out = torch.full((N, 2 * D, 2 * H, 2 * W, Cc), float("nan"), dtype=BF if oh else torch.float32, device="cuda")
            _lib.check(ctx.lib.nm_op_upsample2(ctx.handle, _lib.ptr(xin), N, D, H, W, Cc, _lib.ptr(out)), "upsample2")
            torch.cuda.synchronize()
            assert torch.equal(from_cl(out.float(), Cc), ref.float()), "upsample2 storage (%d, %d)" % (ih, oh)
    finally:
        _set(ctx, 1, 0, 0)
