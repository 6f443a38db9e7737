"""Exact-arithmetic operands and references for the conv kernels and their GroupNorm statistics (CPU only: torch + numpy).

The operands are small integers (or integers times a stated 2^-q).  On such data every product and every partial sum of a
convolution is exactly representable in fp32 (and in the fp16 / bf16 operand formats), so a kernel must return the SAME BITS as an
fp64 reference in any summation order, any brick partition and any of the arithmetic modes; (sum y, sum y^2) per frame and channel are
exact integers too, which pins the GroupNorm scale / shift to a few ulp however large the mean is against the spread.

`preconditions()` returns the facts that make this a theorem rather than a hope; every case asserts them before it touches a device
(tests/test_exact_ref_cpu.py asserts them for every case, on the CPU).

The acceptance bounds of the statistics (SCALE_ULPS, SHIFT_EPS) are derived from the finaliser's operation order, not measured:
scale = (float)rstd * gamma is two float roundings; shift = -scale * (float)mean + beta is one rounding of the mean, one product or
fma and one add, on top of the error inherited from scale."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = float(np.float32(1e-5))          # the kernels' eps: (double)1e-5f
LIMIT = float(2 ** 24)                 # integers below this are exact in fp32, and so is every sum that stays below it
SCALE_ULPS = 2.0                       # |scale - scale_ref| <= SCALE_ULPS * ulp32(scale_ref)
SHIFT_EPS = 4.0 * 2.0 ** -23           # |shift - shift_ref| <= SHIFT_EPS * max(|scale_ref * mean|, |beta|)
BRICK = 8                              # edge of the bricks whose partials the mutation tests drop

_CACHE = {}


def cached(key, fn):
    """References are computed once per case and shared by the modes (and by the tests of a session)."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---- representability -------------------------------------------------------------------------------------------------------------
def fits(t, dtype):
    """Every element of t survives a round trip through dtype."""
    t = t.detach()
    return bool(torch.isfinite(t).all()) and bool(torch.equal(t.to(dtype).to(t.dtype), t))


def is_multiple(t, q):
    """Every element of t is an integer times 2^-q."""
    s = t.detach().double() * 2.0 ** q
    return bool(torch.equal(s, s.round()))


def ulp32(v):
    """Unit in the last place of fp32 at the magnitude of v (fp64 array)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -126)))
    return 2.0 ** (e - 23)


# ---- generators -------------------------------------------------------------------------------------------------------------------
def _signed(shape, hi, g):
    """Non-zero integers in [-hi, hi]."""
    return (torch.randint(1, hi + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def sparse_ints(shape, density, hi, g):
    """Integers in [-hi, hi], non-zero with probability `density`."""
    return (torch.rand(shape, generator=g) < density).float() * _signed(shape, hi, g)


def _seed(*key):
    h = 0
    for k in key:                      # (a stable hash: Python's own is salted for strings)
        for ch in repr(k):
            h = (h * 131 + ord(ch)) % 2147483629
    return h


def out_dims(kind, ks, stride, pad, dims, up2, outpad):
    if kind == "convT":
        return tuple(2 * d + outpad for d in dims)
    us = 2 if up2 else 1
    return tuple((us * d + 2 * pad - ks) // stride + 1 for d in dims)


def activate(x, sc, sh, slope):
    """The kernels' prologue lrelu(x * scale + shift) in fp64; sc / sh are [N, C] or None."""
    a = x.double()
    if sc is not None:
        a = a * sc.double()[:, :, None, None, None] + sh.double()[:, :, None, None, None]
    return F.leaky_relu(a, slope) if slope != 1.0 else a


def _forward64(kind, a, w, b, stride, pad, up2, outpad):
    if kind == "convT":
        return F.conv_transpose3d(a, w, b, stride=2, output_padding=outpad)
    if up2:
        a = F.interpolate(a, scale_factor=2.0, mode="trilinear", align_corners=False)
    return F.conv3d(a, w, b, stride=stride, padding=pad)


def make_forward(spec, data):
    """Operands + fp64 reference of one forward case.

    spec = (kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, groups, outpad), kind in {"conv", "convT"}.
    data = one of
      "sa"     sparse activations x dense {-1, 0, 1} weights, small integer bias
      "dw"     dense small activations x sparse weights, small integer bias
      "r0" / "r8" / "r30"   statistics sets: sparse activations, integer bias that puts the group mean at about 0 / 8 / 30 standard
               deviations of the group, densities chosen so that sum (2^q y)^2 per (frame, channel) stays below 2^24
      "const"  w = 0, the bias one integer per group: the variance is exactly 0
      "chan"   (up2 only) input constant per (frame, channel): every output is a small integer, the whole burden on the shell
      "b16"    as "sa", sparser, activation unit chosen so that every output is an integer of at most 256 (bf16 storage is exact)
    The prologue is scale in {1, 2}, integer shift, slope 0.5 (activations even) or 0.25 (activations multiples of 4): the activated
    input is an integer.  Fused-upsample cases scale the activations by 8 more (by 64 for "b16", which keeps the outputs integers):
    every trilinear product is then a multiple of 1/8 that fits fp16, q = 3."""
    def make():
        kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, groups, outpad = spec
        g = torch.Generator().manual_seed(_seed(spec, data))
        od = out_dims(kind, ks, stride, pad, dims, up2, outpad)
        V = od[0] * od[1] * od[2]
        fan = Cin * (ks ** 3 if kind == "conv" else 1)
        slope = (0.25 if (Cin // 8 + Cout // 8) % 2 else 0.5) if (prologue or up2) else 1.0      # (fused-upsample layers always activate)
        unit = int(round(1.0 / slope))
        if up2 and data != "chan":
            unit *= 64 if data == "b16" else 8
        q = 3 if (up2 and data not in ("b16", "chan")) else 0
        ratio = {"r0": 0.0, "r8": 8.0, "r30": 30.0}.get(data)
        # target variance of the output in units of 2^-q: a quarter of what sum (2^q y)^2 < 2^24 leaves at this ratio
        var_t = 16.0
        if ratio is not None:
            var_t = min(16.0, 0.25 * LIMIT / (V * (ratio * ratio + 1.0)))
        if data == "chan":                       # (every voxel of a channel carries the same value: no averaging over the frame, a wider margin)
            var_t = min(16.0, 0.05 * LIMIT / V)
        if data == "b16":
            var_t = 4.0
        amp = float(unit * 2 ** q) ** 2 * 2.5 * (2.5 * 0.6 if prologue else (0.6 if up2 else 1.0)) * (0.3 if up2 else 1.0)    # E[(2^q a)^2] of a non-zero activation
        wshape = (Cout, Cin, ks, ks, ks) if kind == "conv" else (Cin, Cout, 2, 2, 2)
        xshape = (N, Cin, *dims)
        sc = sh = None
        if prologue:
            sc = torch.randint(1, 3, (N, Cin), generator=g).float()
            sh = torch.zeros(N, Cin)
        if data == "const":
            x = sparse_ints(xshape, 0.05, 2, g) * unit
            w = torch.zeros(wshape)
        elif data == "chan":
            # one value per (frame, channel), on the negative side of the activation (small: -1, -2, -4 after slope and scale): the
            # upsample of a constant is that constant, the interior one integer per output channel, the shell the partial tap sums
            x = (-torch.randint(1, 3, (N, Cin, 1, 1, 1), generator=g).float() * unit).expand(xshape).contiguous()
            w = sparse_ints(wshape, min(0.67, var_t / (fan * 5.0)), 1, g)
        elif data == "dw":
            x = torch.randint(-2, 3, xshape, generator=g).float() * unit
            if prologue:
                sh = torch.randint(-1, 2, (N, Cin), generator=g).float() * unit
            w = sparse_ints(wshape, min(0.67, var_t / (fan * amp * 0.8)), 1, g)
        elif data == "b16" and up2:
            # a handful of -64s per frame (scale 1) against sparse weights: every output an integer of at most 256
            x = -(torch.rand(xshape, generator=g) < 6.0 / (Cin * dims[0] * dims[1] * dims[2])).float() * unit
            sc = torch.ones(N, Cin)
            w = sparse_ints(wshape, 0.1, 1, g)
        else:
            pw = 0.67
            pa = min(0.25, var_t / (fan * pw * amp))
            x = sparse_ints(xshape, pa, 2, g) * unit
            if prologue and data == "sa":        # a shift on one (frame, channel) row in eight: the rest of the tensor stays sparse
                sh = (torch.rand(N, Cin, generator=g) < 0.125).float() * _signed((N, Cin), 1, g) * unit
            w = sparse_ints(wshape, pw, 1, g)
        a = activate(x, sc, sh, slope)
        y0 = _forward64(kind, a, w.double(), None, stride, pad, up2, outpad)
        if data == "const":
            gi = torch.arange(Cout) // max(Cout // max(groups, 1), 1)
            b = (3 + gi % 16).float()
        elif ratio is not None and groups > 0:
            cpg = Cout // groups
            yg = y0.reshape(N, groups, cpg * V)
            std_g = yg.var(dim=2, unbiased=False).sqrt().mean(dim=0)                     # per group, averaged over the frames
            mean_c = y0.mean(dim=(0, 2, 3, 4))
            b = (ratio * std_g.repeat_interleave(cpg) - mean_c).round().float()
        elif data == "chan":
            b = torch.randint(-1, 2, (Cout,), generator=g).float()
        else:
            b = torch.randint(-3, 4, (Cout,), generator=g).float()
        y = y0 + b.double()[None, :, None, None, None]
        gam = torch.rand(Cout, generator=g) + 0.5
        bet = torch.randn(Cout, generator=g) * 0.2
        return dict(spec=spec, data=data, x=x, w=w, b=b, sc=sc, sh=sh, slope=slope, a=a, y=y, q=q, gam=gam, bet=bet, od=od)
    return cached(("fwd", spec, data), make)


# ---- preconditions ----------------------------------------------------------------------------------------------------------------
def preconditions(d, in16=False, out16=False):
    """The facts that make the fp64 reference of case d (make_forward) the only result a correct kernel can return."""
    kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, groups, outpad = d["spec"]
    q = d["q"]
    a32 = d["a"].float()
    facts = {}
    # operands: raw input, activated input (the f16 modes round it to fp16 after the prologue), weights; the upsampled input too
    # (the staging of the fused-upsample kernels interpolates, then converts)
    ops16 = [d["x"], a32, d["w"]]
    if up2:
        ops16.append(F.interpolate(d["a"], scale_factor=2.0, mode="trilinear", align_corners=False).float())
    facts["operands_fit_fp16"] = all(fits(t, torch.float16) for t in ops16) and bool(torch.equal(a32.double(), d["a"]))
    facts["prologue_exact"] = d["sc"] is None or (bool(((d["sc"] == 1) | (d["sc"] == 2)).all()) and is_multiple(d["sh"], 0)
                                                    and d["slope"] in (0.25, 0.5))
    facts["bias_integer"] = is_multiple(d["b"], 0)
    if in16:
        facts["input_fits_bf16"] = fits(d["x"], torch.bfloat16)
    if out16:
        facts["output_fits_bf16"] = fits(d["y"].float(), torch.bfloat16) and bool(d["y"].abs().max() <= 256)
    # every output element: (sum |w| |a| + |b|) 2^q < 2^24, by a conv of the absolute values in fp64
    mag = _forward64(kind, d["a"].abs(), d["w"].double().abs(), d["b"].double().abs(), stride, pad, up2, outpad)
    qp = 6 if (up2 and q == 0) else q                    # (integer outputs of a fused-upsample layer: the partial sums are multiples of 1/64)
    facts["max_abs_sum"] = float(mag.max()) * 2.0 ** qp
    facts["sums_below_2^24"] = facts["max_abs_sum"] < LIMIT
    facts["output_on_grid"] = is_multiple(d["y"], q) and bool(torch.equal(d["y"].float().double(), d["y"]))
    ss = ((d["y"] * 2.0 ** q) ** 2).sum(dim=(2, 3, 4))
    facts["max_frame_channel_sumsq"] = float(ss.max())
    facts["stats_exact"] = facts["max_frame_channel_sumsq"] < LIMIT
    return facts


REQUIRED = ("operands_fit_fp16", "prologue_exact", "bias_integer", "input_fits_bf16", "output_fits_bf16", "sums_below_2^24", "output_on_grid")


def assert_preconditions(facts, stats=False):
    for k in REQUIRED:
        assert facts.get(k, True), (k, facts)
    if stats:
        assert facts["stats_exact"], facts


# ---- GroupNorm statistics ---------------------------------------------------------------------------------------------------------
def stats_from_sums(s, ss, count, gam, bet):
    """scale / shift of the fused GroupNorm from per-(frame, group) sums, in fp64: the definition the finaliser implements.
    s, ss: [N, groups]; gam, bet: [C].  Returns dict of [N, C] fp64 arrays + the per-group mean / var / rstd ([N, groups])."""
    s, ss = np.asarray(s, dtype=np.float64), np.asarray(ss, dtype=np.float64)
    gam, bet = np.asarray(gam, dtype=np.float64), np.asarray(bet, dtype=np.float64)
    cpg = gam.shape[0] // s.shape[1]
    mean = s / count
    var = np.maximum(ss / count - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + EPS)
    scale = np.repeat(rstd, cpg, axis=1) * gam[None]
    meanc = np.repeat(mean, cpg, axis=1)
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=bet[None] - scale * meanc, meanc=meanc, bet=bet)


def group_sums(y, groups):
    """Exact (sum y, sum y^2, count) per (frame, group) of an NCDHW fp64 tensor."""
    N, C = y.shape[:2]
    yg = y.double().reshape(N, groups, -1)
    return yg.sum(dim=2).numpy(), (yg * yg).sum(dim=2).numpy(), float(yg.shape[2])


def reference_stats(d):
    s, ss, count = group_sums(d["y"], d["spec"][10])
    return stats_from_sums(s, ss, count, d["gam"].numpy(), d["bet"].numpy())


def stats_errors(scale, shift, ref, scale_ulps=SCALE_ULPS, shift_eps=SHIFT_EPS):
    """Worst violation ratios (<= 1 passes) of scale / shift ([N, C] arrays) against reference_stats / stats_from_sums."""
    scale, shift = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    es = np.abs(scale - ref["scale"]) / (scale_ulps * ulp32(ref["scale"]))
    bound = shift_eps * np.maximum(np.abs(ref["scale"] * ref["meanc"]), np.abs(ref["bet"])[None])
    eh = np.abs(shift - ref["shift"]) / np.maximum(bound, 2.0 ** -149)
    return float(es.max()), float(eh.max())


def stats_accepted(scale, shift, ref, **kw):
    if not (np.isfinite(scale).all() and np.isfinite(shift).all()):
        return False
    es, eh = stats_errors(scale, shift, ref, **kw)
    return es <= 1.0 and eh <= 1.0


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def make_backward(spec, lean=False):
    """Operands + fp64 autograd gradients of one backward case.  spec = (kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2,
    outpad).  x: sparse integers (dense {-1, 0, 1} weights), dy: sparse integers; fused-upsample cases use activations that are
    multiples of 64 in the forward direction (the upsampled input, an operand of the weight gradient, is then an integer) and the adjoint's
    coefficients k/64 make d_in a multiple of 1/64.  lean (fused-upsample cases with 16-bit storage): activations -64 * scale only and a
    sparser dy, so that the upsampled input, the fine-grid data gradient and d_in keep to the 8 significant bits of bfloat16."""
    def make():
        kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, outpad = spec
        g = torch.Generator().manual_seed(_seed("bwd", spec))
        od = out_dims(kind, ks, stride, pad, dims, up2, outpad)
        V = od[0] * od[1] * od[2]
        slope = (0.25 if (Cin // 8 + Cout // 8) % 2 else 0.5) if (prologue or up2) else 1.0
        unit = int(round(1.0 / slope)) * (64 if up2 else 1)
        # densities: each weight-gradient element sums N V products; keep the expected count of non-zero ones near 40
        pa = min(0.2, (40.0 / (N * V)) ** 0.5 * 1.5)
        pd = min(0.2, (40.0 / (N * V)) ** 0.5 * 1.5)
        x = sparse_ints((N, Cin, *dims), pa, 2, g) * unit
        if lean:
            x, pd = -x.abs().clamp(max=unit), 8.0 / (Cout * V)            # (a handful of non-zero dy per frame)
        wshape = (Cout, Cin, ks, ks, ks) if kind == "conv" else (Cin, Cout, 2, 2, 2)
        w = sparse_ints(wshape, 0.1 if lean else 0.67, 1, g)
        sc = sh = None
        if prologue:
            sc = torch.randint(1, 3, (N, Cin), generator=g).float()
            sh = (torch.rand(N, Cin, generator=g) < (0.0 if lean else 0.125)).float() * _signed((N, Cin), 1, g) * unit
        dy = sparse_ints((N, Cout, *od), pd, 2, g)
        a = activate(x, sc, sh, slope).requires_grad_(True)
        w64 = w.double().requires_grad_(True)
        b64 = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
        up = F.interpolate(a, scale_factor=2.0, mode="trilinear", align_corners=False) if up2 else a
        if up2:
            up.retain_grad()
        _forward64(kind, up, w64, b64, stride, pad, False, outpad).backward(dy.double())
        return dict(spec=spec, x=x, w=w, sc=sc, sh=sh, slope=slope, a=a.detach(), dy=dy, d_w=w64.grad, d_b=b64.grad, d_a=a.grad, od=od,
                    up=up.detach(), d_up=up.grad if up2 else a.grad)
    return cached(("bwd", spec, lean), make)


def backward_preconditions(d, in16=False, out16=False):
    kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, outpad = d["spec"]
    a = d["a"].clone().abs().requires_grad_(True)
    w = d["w"].double().abs().requires_grad_(True)
    b = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    _forward64(kind, a, w, b, stride, pad, up2, outpad).backward(d["dy"].double().abs())
    q = 6 if up2 else 0                                   # the upsample adjoint's coefficients are k/64
    facts = {}
    ops = [d["x"], d["a"].float(), d["w"], d["dy"], d["up"].float()]
    facts["operands_fit_fp16"] = all(fits(t, torch.float16) for t in ops) and bool(torch.equal(d["a"].float().double(), d["a"]))
    if in16 or out16:
        # what a 16-bit-storage kernel stores: the input (in16), dy, the upsampled input and the fine-grid data gradient (out16)
        stored = ([d["x"]] if in16 else []) + ([d["dy"], d["up"].float(), d["d_up"].float()] if out16 else [])
        facts["operands_fit_bf16"] = all(fits(t, torch.bfloat16) for t in stored)
        facts["d_in_fits_bf16"] = (not in16) or fits(d["d_a"].float(), torch.bfloat16)
    facts["max_d_weight_abs_sum"] = float(w.grad.max())
    facts["max_d_in_abs_sum"] = float(a.grad.max()) * 2.0 ** q
    facts["max_d_bias_abs_sum"] = float(b.grad.max())
    facts["sums_below_2^24"] = max(facts["max_d_weight_abs_sum"], facts["max_d_in_abs_sum"], facts["max_d_bias_abs_sum"]) < LIMIT
    facts["gradients_on_grid"] = is_multiple(d["d_w"], 0) and is_multiple(d["d_b"], 0) and is_multiple(d["d_a"], q)
    return facts


def assert_backward_preconditions(facts):
    for k in ("operands_fit_fp16", "operands_fit_bf16", "d_in_fits_bf16", "sums_below_2^24", "gradients_on_grid"):
        assert facts.get(k, True), (k, facts)


# ---- first layer (occupancy + coordinate channels) ---------------------------------------------------------------------------------
def make_occ(G, Cout, N):
    """conv5 on cat[occ, coords]: occupancy 0 / 1 (frame 1 fractional: 0.5 / 0.25), integer weights on the occupancy channel, zero
    weights on the three coordinate channels (the constant field is then the bias alone)."""
    def make():
        g = torch.Generator().manual_seed(_seed("occ", G, Cout, N))
        occ = (torch.rand(N, 1, G, G, G, generator=g) < 0.03).float()
        if N > 1:
            occ[1] = occ[1] * (0.25 * torch.randint(1, 3, (1, G, G, G), generator=g).float())
        w = torch.zeros(Cout, 4, 5, 5, 5)
        w[:, 0] = sparse_ints((Cout, 5, 5, 5), 0.5, 1, g)
        groups = Cout // 16
        y0 = F.conv3d(occ.double(), w[:, :1].double(), None, padding=2)
        std_g = y0.reshape(N, groups, -1).var(dim=2, unbiased=False).sqrt().mean(dim=0)
        b = (8.0 * std_g.repeat_interleave(16)).round().float() + torch.randint(-1, 2, (Cout,), generator=g).float()
        y = y0 + b.double()[None, :, None, None, None]
        gam = torch.rand(Cout, generator=g) + 0.5
        bet = torch.randn(Cout, generator=g) * 0.2
        return dict(occ=occ, w=w, b=b, y=y, q=2 if N > 1 else 0, gam=gam, bet=bet, groups=groups, spec=(None,) * 10 + (groups,))
    return cached(("occ", G, Cout, N), make)


def occ_preconditions(d):
    q = d["q"]
    facts = {"operands_fit_fp16": fits(d["occ"], torch.float16) and fits(d["w"], torch.float16), "bias_integer": is_multiple(d["b"], 0),
             "coordinate_weights_zero": bool((d["w"][:, 1:] == 0).all())}
    mag = F.conv3d(d["occ"].double(), d["w"][:, :1].double().abs(), d["b"].double().abs(), padding=2)
    facts["max_abs_sum"] = float(mag.max()) * 2.0 ** q
    facts["sums_below_2^24"] = facts["max_abs_sum"] < LIMIT
    facts["output_on_grid"] = is_multiple(d["y"], q)
    facts["max_frame_channel_sumsq"] = float(((d["y"] * 2.0 ** q) ** 2).sum(dim=(2, 3, 4)).max())
    facts["stats_exact"] = facts["max_frame_channel_sumsq"] < LIMIT
    return facts


# ---- GroupNorm backward -----------------------------------------------------------------------------------------------------------
def make_gn_backward(C, groups, size, N, slope, ratio):
    """y = integer offset + integer noise in [-2, 2] (exact per-(frame, channel) sums), mean / std = ratio; dA = randn; the four
    outputs of nm_op_gn_backward by fp64 autograd."""
    def make():
        g = torch.Generator().manual_seed(_seed("gnb", C, groups, size, N, ratio))
        noise = torch.randint(-2, 3, (N, C, size, size, size), generator=g).double()
        off = float(round(ratio * 2.0 ** 0.5))                     # std of the uniform integers in [-2, 2] is sqrt(2)
        y = (noise + off).requires_grad_(True)
        gam = (torch.rand(C, generator=g) + 0.5).double().requires_grad_(True)
        bet = (torch.randn(C, generator=g) * 0.2).double().requires_grad_(True)
        out = F.leaky_relu(F.group_norm(y, groups, gam, bet, EPS), slope)
        dA = torch.randn(out.shape, generator=g)
        out.backward(dA.double())
        ss = float((y.detach() ** 2).sum(dim=(2, 3, 4)).max())
        return dict(y=y.detach().float(), gam=gam.detach().float(), bet=bet.detach().float(), dA=dA, dy=y.grad, dgam=gam.grad, dbet=bet.grad,
                    sums_exact=ss < LIMIT, off=off)
    return cached(("gnb", C, groups, size, N, slope, ratio), make)


def mean_over_std(d):
    """Per-(frame, group) |mean| / std of a forward case, [N, groups]."""
    r = reference_stats(d)
    return np.abs(r["mean"]) / np.sqrt(np.maximum(r["var"], 1e-300))
