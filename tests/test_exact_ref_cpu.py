"""The exact-arithmetic reference checked on its own, without a device (tests/exact_ref.py, tests/test_exact_arithmetic_gpu.py).

For every case the device file runs: the preconditions hold, and ATen's fp32 result on the CPU equals the fp64 reference bit for bit - the
reference alone is inside the exact range.  Sharpness by mutation: a duplicated or dropped (voxel, channel) item, a dropped brick
partial, E[y^2] - mean^2 evaluated in fp32 and a whole frame accumulated in one fp32 running sum all land OUTSIDE the acceptance
bounds of exact_ref (and the first of them inside the old 2e-5 bound on the normalised output)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref as X
import test_exact_arithmetic_gpu as E

f32 = np.float32


def kernel_model(st, gam, bet):
    """scale / shift as the finaliser rounds them: (float)rstd * gamma, then -scale * (float)mean + beta in one fma."""
    cpg = gam.shape[0] // st["rstd"].shape[1]
    sc = (np.repeat(st["rstd"], cpg, axis=1).astype(f32) * gam.astype(f32)[None]).astype(f32)
    sh = (-sc.astype(np.float64) * st["meanc"].astype(f32).astype(np.float64) + bet.astype(f32).astype(np.float64)[None]).astype(f32)
    return sc.astype(np.float64), sh.astype(np.float64)


# ---- every device case: preconditions + ATen fp32 == fp64 --------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.forward_cases(), ids=E._fid)
def test_forward_case_is_exact(case):
    spec, data, ih, oh, _ = case
    d = X.make_forward(spec, data)
    facts = X.preconditions(d, in16=bool(ih), out16=bool(oh))
    stats = spec[10] > 0 and (data in E.STAT_SETS or data == "chan")
    X.assert_preconditions(facts, stats=stats)
    kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, groups, outpad = spec
    a32 = d["x"]
    if d["sc"] is not None:
        a32 = a32 * d["sc"][:, :, None, None, None] + d["sh"][:, :, None, None, None]
    if d["slope"] != 1.0:
        a32 = F.leaky_relu(a32, d["slope"])
    y32 = X._forward64(kind, a32, d["w"], d["b"], stride, pad, up2, outpad)
    assert y32.dtype == torch.float32 and torch.equal(y32.double(), d["y"]), "ATen fp32 differs from the fp64 reference"
    if stats:
        ref = X.reference_stats(d)
        sc, sh = kernel_model(ref, d["gam"].numpy(), d["bet"].numpy())
        assert X.stats_accepted(sc, sh, ref), X.stats_errors(sc, sh, ref)
        if data in ("r8", "r30") and d["y"][0, 0].numel() >= 4096:      # the set is what its name says (large volumes: the std of a small one is noisy)
            want = 8.0 if data == "r8" else 30.0
            r = float(np.median(X.mean_over_std(d)))
            assert 0.5 * want <= r <= 2.0 * want, r


@pytest.mark.parametrize("case", E.backward_cases(), ids=E._bid)
def test_backward_case_is_exact(case):
    spec, ih, oh, modes, _ = case
    d = X.make_backward(spec[:11], lean=bool(spec[9] and (ih or oh)))
    X.assert_backward_preconditions(X.backward_preconditions(d, in16=bool(ih), out16=bool(oh)))
    kind, Cin, Cout, ks, stride, pad, dims, N, prologue, up2, outpad = spec[:11]
    a = d["a"].float().requires_grad_(True)
    w = d["w"].clone().requires_grad_(True)
    b = torch.zeros(Cout, requires_grad=True)
    X._forward64(kind, a, w, b, stride, pad, up2, outpad).backward(d["dy"])
    assert torch.equal(w.grad.double(), d["d_w"]) and torch.equal(b.grad.double(), d["d_b"]) and torch.equal(a.grad.double(), d["d_a"])


@pytest.mark.parametrize("G,Cout,N", E.OCC_CASES)
def test_first_layer_case_is_exact(G, Cout, N):
    from oracle import nm_oracle as O
    d = X.make_occ(G, Cout, N)
    facts = X.occ_preconditions(d)
    X.assert_preconditions(facts, stats=True)
    assert facts["coordinate_weights_zero"] and (N == 1 or bool(((d["occ"][1] > 0) & (d["occ"][1] < 1)).any()))
    y32 = F.conv3d(O.add_coords(d["occ"]), d["w"], d["b"], padding=2)
    assert torch.equal(y32.double(), d["y"])


@pytest.mark.parametrize("ratio", E.GNB_RATIOS)
@pytest.mark.parametrize("C,groups,size,N,slope", E.GNB_CASES)
def test_gn_backward_case_has_exact_sums(C, groups, size, N, slope, ratio):
    d = X.make_gn_backward(C, groups, size, N, slope, ratio)
    assert d["sums_exact"] and X.is_multiple(d["y"], 0)
    yg = d["y"].double().reshape(N, groups, -1)
    if size > 1:
        r = (yg.mean(dim=2).abs() / yg.var(dim=2, unbiased=False).sqrt()).median().item()
        assert (r < 0.5) if ratio == 0 else (0.7 * ratio <= r <= 1.5 * ratio), r


# ---- sharpness ---------------------------------------------------------------------------------------------------------------------
CENTRED = [("conv", 32, 64, 3, 1, 1, (16, 16, 16), 2, False, False, 4, 0),      # 65536 items per group: where 2e-5 is most forgiving
           ("conv", 32, 64, 3, 1, 1, (24, 24, 24), 1, True, False, 4, 0),
           ("conv", 32, 32, 2, 2, 0, (20, 20, 20), 2, True, False, 2, 0)]
OFFSET = [("conv", 32, 64, 3, 1, 1, (16, 16, 16), 2, False, False, 4, 0), ("conv", 32, 32, 3, 1, 1, (32, 32, 32), 3, True, False, 2, 0)]


def _mutated(d, ds, dss):
    """Reference statistics against the kernel model of sums off by (ds, dss) in (frame 0, group 0)."""
    groups = d["spec"][10]
    s, ss, count = X.group_sums(d["y"], groups)
    ref = X.stats_from_sums(s, ss, count, d["gam"].numpy(), d["bet"].numpy())
    s2, ss2 = s.copy(), ss.copy()
    s2[0, 0] += ds; ss2[0, 0] += dss
    mut = X.stats_from_sums(s2, ss2, count, d["gam"].numpy(), d["bet"].numpy())
    return ref, kernel_model(mut, d["gam"].numpy(), d["bet"].numpy())


@pytest.mark.parametrize("spec", CENTRED, ids=lambda s: "ci%d_co%d_k%d_d%d" % (s[1], s[2], s[3], s[6][0]))
def test_single_item_and_brick_mutations_are_rejected(spec):
    """One (voxel, channel) item duplicated or dropped - the one furthest from the group mean and the nearest with |y - mean| >= 1 - and
    one 8x8x8 brick's partial of one channel dropped: each lands outside the scale / shift bounds.  The last lines restate the old
    criterion (2e-5 of the normalised output's max) and show that it accepts the duplicated near item in a group of >= 65536."""
    assert spec in E.CONV_SPECS
    d = X.make_forward(spec, "r0")
    groups, Cout = spec[10], spec[2]
    cpg = Cout // groups
    y = d["y"]
    s, ss, count = X.group_sums(y, groups)
    ref = X.stats_from_sums(s, ss, count, d["gam"].numpy(), d["bet"].numpy())
    assert X.stats_accepted(*kernel_model(ref, d["gam"].numpy(), d["bet"].numpy()), ref)      # the unmutated model passes
    dev0 = (y[0, :cpg] - ref["mean"][0, 0]).abs().flatten()
    far = y[0, :cpg].flatten()[dev0.argmax()].item()
    near = y[0, :cpg].flatten()[torch.where(dev0 >= 1.0, dev0, torch.full_like(dev0, 1e9)).argmin()].item()
    assert abs(far - ref["mean"][0, 0]) >= 1.0 and abs(near - ref["mean"][0, 0]) >= 1.0
    for item in (far, near):
        for sign, what in ((1.0, "duplicated"), (-1.0, "dropped")):
            r, (sc, sh) = _mutated(d, sign * item, sign * item * item)
            assert not X.stats_accepted(sc, sh, r), f"an item {item} {what} among {count:.0f} passes the bounds"
    brick = y[0, 0, :X.BRICK, :X.BRICK, :X.BRICK]
    r, (sc, sh) = _mutated(d, -brick.sum().item(), -(brick * brick).sum().item())
    assert not X.stats_accepted(sc, sh, r), "a dropped brick partial passes the bounds"
    # the blind spot these tests close: the old criterion (2e-5 of the normalised output's max) accepts the duplicated item
    r, (sc, sh) = _mutated(d, near, near * near)
    n_ref = y[0, :cpg] * torch.from_numpy(r["scale"][0, :cpg])[:, None, None, None] + torch.from_numpy(r["shift"][0, :cpg])[:, None, None, None]
    n_mut = y[0, :cpg] * torch.from_numpy(sc[0, :cpg])[:, None, None, None] + torch.from_numpy(sh[0, :cpg])[:, None, None, None]
    old = (n_mut - n_ref).abs().max().item() / n_ref.abs().max().item()
    if count >= 65536:
        assert old < 2e-5, old


@pytest.mark.parametrize("spec", OFFSET, ids=lambda s: "ci%d_co%d_k%d_d%d" % (s[1], s[2], s[3], s[6][0]))
def test_fp32_variance_subtraction_is_rejected(spec):
    """var = E[y^2] - mean^2 evaluated in fp32 on the exact sums of the mean / std = 30 set."""
    assert spec in E.CONV_SPECS
    d = X.make_forward(spec, "r30")
    groups = spec[10]
    gam, bet = d["gam"].numpy(), d["bet"].numpy()
    s, ss, count = X.group_sums(d["y"], groups)
    ref = X.stats_from_sums(s, ss, count, gam, bet)
    mean32 = (s.astype(f32) / f32(count)).astype(f32)
    var32 = ((ss.astype(f32) / f32(count)).astype(f32) - (mean32 * mean32).astype(f32)).astype(f32)
    rstd32 = (f32(1.0) / np.sqrt((np.maximum(var32, f32(0)) + f32(X.EPS)).astype(f32))).astype(f32)
    cpg = gam.shape[0] // groups
    sc = (np.repeat(rstd32, cpg, axis=1) * gam.astype(f32)[None]).astype(f32)
    sh = (bet.astype(f32)[None] - sc * np.repeat(mean32, cpg, axis=1)).astype(f32)
    assert not X.stats_accepted(sc.astype(np.float64), sh.astype(np.float64), ref)


@pytest.mark.parametrize("ratio", [30.0, 100.0])
def test_single_fp32_running_sum_is_rejected(ratio):
    """One channel's whole 32^3 frame accumulated in ONE fp32 running sum of real-valued (non-exact) data at mean / std >= 30, group = the
    channel: against the fp64 sums of the same fp32 values."""
    g = torch.Generator().manual_seed(int(ratio))
    y = (torch.randn(32768, generator=g) + ratio).numpy().astype(f32)
    s32 = np.cumsum(y, dtype=f32)[-1]
    ss32 = np.cumsum((y * y).astype(f32), dtype=f32)[-1]
    y64 = y.astype(np.float64)
    gam, bet = np.array([1.25]), np.array([0.1])
    ref = X.stats_from_sums([[y64.sum()]], [[(y64 * y64).sum()]], float(y.size), gam, bet)
    assert X.stats_accepted(*kernel_model(ref, gam, bet), ref)
    mut = X.stats_from_sums([[float(s32)]], [[float(ss32)]], float(y.size), gam, bet)
    assert not X.stats_accepted(*kernel_model(mut, gam, bet), ref)
