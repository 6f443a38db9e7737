"""Op-level parity of the detector heads and losses: the launcher sequences of csrc/nm_heads.hip and csrc/nm_heads_bwd.hip, called
through the nm_op_* entry points of include/nm355.h on inputs chosen for the kernels' own branches and tilings, against the same
operation in float64 (the oracle's functions + the glue of tests/heads_ref.py, torch autograd for the adjoints).  The inputs, the case
tables and what each case deliberately contains are in tests/heads_ref.py; tests/test_heads_ref_cpu.py pins that reference to the
oracle and shows that every discontinuous selection on these inputs is decided by a clear margin - nothing is masked out here.

Kernels reached, by family
  heat      heatmap_kernel | heat_scan_kernel + heat_marginals_kernel (recurrent), heat_plane_marginals in all three lane groupings,
            keypoints_kernel; backward heat_bwd_prep_kernel, heat_bwd_kernel + sum_t_kernel | heat_bwd_recurrent_kernel, sum_rows_kernel.
            g = 32 with K = 24 / 32 asks for 96 / 128 KB of dynamic LDS: the launchers raise the limit once per device.
  combined  gauss_width_kernel, gauss_table_kernel, combined_kernel (cat none / max / sum); backward gauss_bwd_kernel,
            sigma_bwd_finish_kernel, gauss_bwd_finish_kernel, first_feature_bwd_kernel (aligned and K % 4 != 0 forms)
  tail      decoder_tail_kernel (C = 32 cooperative branch, generic branch at C = 16; G = 40 leaves the last block of NM_TAIL_TILES half
            filled), tail_sums_kernel; backward tail_bwd32_kernel (dA and per-voxel forms), tail_bwd_kernel (C = 16), sum_rows_kernel,
            chamfer_bwd_kernel, chamfer_bwd_finish_kernel
  clip      clip_loss_kernel, tail_sums_kernel, loss_finalize_kernel; backward clip_loss_bwd_kernel incl. its clamp_k / clamp_a branches
            (a keypoint at rest over one step, constant velocity over two; 'creep': norms of 2^-22 .. 2^-21.5, under the clamp but not
            zero - the kernel dropped the norm's own gradient there until this file found it), coincident keypoints, intensities 0 and 1
  affinity  affinity_kernel, affinity_bwd_kernel, versions 0-3
  volfit    volfit_proj_kernel, volfit_mask_kernel, volfit_frame_kernel; backward volfit_proj_b_kernel, volfit_wsum_kernel, volfit_bwd_kernel
Not reached: combined_rest_kernel, adjust_gauss_kernel, adjust_wg_kernel (the inference split of the 1x1 conv: parity through
tests/test_network_gpu.py only) and the input path's kernels at the end of nm_heads.hip (tests/test_input_path_gpu.py).  The decoder
tail's generic branch cannot be reached at C = 32 on a grid nm_ctx_create admits (G % 8 == 0 makes G^3 a multiple of 256); it runs at
C = 16.  Trajectory lengths T < 3 are not cases: the mean over T - 2 acceleration terms divides by zero in the reference too.

Bounds: REL = 2e-5 of the tensor's largest magnitude (tests/test_ops_gpu.py), keypoint coordinates 1e-6 absolute, each of the eleven
losses REL of its own value.  Where the float32 run of the reference on the CPU misses REL against float64 itself, the bound is four
times that measured error (BOUNDS below: measured value, bound); no bound comes from a kernel's output.  Outputs are pre-filled with NaN
and must come back finite; every forward runs twice and must repeat bit for bit."""

import pytest
import torch

import heads_ref as R
from test_ops_gpu import ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

REL = 2e-5
KP_ABS = 1e-6

# (family, case) -> {output: bound}; measured = max |float32 reference - float64 reference| / max |float64 reference| on the CPU
BOUNDS = {
    ("heat", (32, 24, 1, 4, 1, "")): {"dprop": 1.9e-4},                                  # measured 4.71e-5
    ("heat", (18, 5, 1, 2, 1, "last")): {"dhead": 3.5e-4, "dclip_head": 5.9e-4},         # measured 8.52e-5, 1.46e-4
    ("heat", (32, 5, 1, 1, 0, "last")): {"dhead": 1.0e-4},                               # measured 2.50e-5
    ("tail", (32, 32, 1, 3, 24, False, False, False, False)): {"dw14": 9.4e-5},          # measured 2.34e-5
    ("tail", (40, 32, 2, 2, 24, True, False, False, True)): {"dw14": 1.9e-4},            # measured 4.71e-5
    ("tail", (32, 32, 1, 3, 2, False, True, False, True)): {"dw14": 9.2e-5},             # measured 2.28e-5
    ("tail", (40, 16, 2, 1, 24, True, True, False, False)): {"dw14": 1.0e-4},            # measured 2.50e-5
    # saturation in the float32-only zone (pre ~ 30 against target 0: float32 has 1 - p == 0, log clamped at -100, adjoint 0; float64 has
    # log(1 - p) = -pre and an adjoint through the 1e-12 floor).  measured: BCE sum 2.87e-1, dA 9.46e-1, dw14 6.98e-2 - at four times that
    # the first two only say "finite, fully written, repeatable"; recon, chamfer sum, count and dkp of this case stay at REL
    ("tail", (32, 32, 1, 3, 5, False, False, True, False)): {"bce": 1.15, "dA": 3.8, "dw14": 2.8e-1},
    ("aff", (1, 2, 1, 1, 1, 0, 0)): {"dparams": 5.6e-3},                                 # measured 1.39e-3 (W = m / (m + 1e-6): a gradient of 1e-6 by cancellation)
}


def lib():
    from neural_marionette_amd import _lib
    return _lib


def P(t):
    return lib().ptr(t)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def call(fn, *args):
    L = lib()
    L.check(getattr(L.load(), fn)(*args), fn)


def close(fam, case, name, got, ref, bound=None, absolute=False):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: not finite / not fully written"
    b = BOUNDS.get((fam, case), {}).get(name, bound if bound is not None else REL)
    e = (got - ref).abs().max().item()
    if not absolute:
        e /= max(ref.abs().max().item(), 1e-300)
    print("%s %s %s: %.3e (bound %.1e)" % (fam, case, name, e, b))
    assert e <= b, f"{fam} {case} {name}: {e:.3e} > {b:.1e}"


def cl(x, cpad=None, fill=0.0):
    """(N,C,d,d,d) cpu -> channels-last (N,d,d,d,cpad) on the device; channels beyond C hold `fill`"""
    N, C = x.shape[:2]
    cp = cpad or C
    y = torch.full((N, *x.shape[2:], cp), fill, dtype=torch.float32)
    y[..., :C] = x.permute(0, 2, 3, 4, 1)
    return y.contiguous().cuda()


def uncl(y, C):
    return y[..., :C].permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("case", R.HEAT_CASES, ids=str)
def test_heatmaps_keypoints(ctx, case):
    g, K, B, T, rec, special = case
    inp = R.heat_inputs(*case)
    ref = R.ref_heat(inp, torch.float64)
    Fr, Kc = B * T, (K + 7) // 8 * 8
    head = cl(inp["head"].reshape(Fr, K, g, g, g), Kc, 777.0)          # (padded channels are read with their quad and must be dropped)
    clip = cl(inp["clip_head"], Kc, -555.0)
    prop, dkp, dloss = inp["prop"].cuda(), inp["dkp"].reshape(Fr, K, 4).contiguous().cuda(), inp["dloss"].cuda()
    runs = []
    for _ in range(2):
        hm, kp, mean = nan(Fr, K, g, g, g), nan(Fr, K, 4), nan(Fr, K)
        call("nm_op_heatmaps", ctx.handle, P(head), P(clip), P(prop), B, T, K, Kc, g, rec, P(hm), P(kp), P(mean))
        torch.cuda.synchronize()
        runs.append((hm, kp, mean))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "forward is not repeatable bit for bit"
    hm, kp, mean = runs[0]
    close("heat", case, "heatmaps", hm.view(B, T, K, g, g, g), ref["heatmaps"])
    close("heat", case, "heat_mean", mean.view(B, T, K), ref["heat_mean"])
    close("heat", case, "keypoints", kp.view(B, T, K, 4)[..., :3], ref["keypoints"][..., :3], KP_ABS, absolute=True)
    close("heat", case, "intensity", kp.view(B, T, K, 4)[..., 3], ref["keypoints"][..., 3])
    dhead, dclip, dprop = nan(Fr, g, g, g, Kc), nan(B, g, g, g, Kc), nan(3)
    call("nm_op_heatmaps_backward", ctx.handle, P(head), P(clip), P(prop), B, T, K, Kc, g, rec, P(dkp), P(dloss), P(dhead), P(dclip), P(dprop))
    torch.cuda.synchronize()
    close("heat", case, "dhead", uncl(dhead, K).reshape(B, T, K, g, g, g), ref["dhead"])
    close("heat", case, "dclip_head", uncl(dclip, K), ref["dclip_head"])
    close("heat", case, "dprop", dprop, ref["dprop"])
    assert (dhead[..., K:] == 0).all() and (dclip[..., K:] == 0).all()


@pytest.mark.parametrize("case", R.COMBINED_CASES, ids=str)
def test_gauss_table_combined(ctx, case):
    g, K, B, T, Fd, cat, learn, sigma = case
    inp = R.combined_inputs(*case)
    ref = R.ref_combined(inp, torch.float64)
    Fr, Cd = B * T, inp["Cd"]
    C = 2 * K + Fd + 3
    kp = inp["kp"].reshape(Fr, K, 4).contiguous().cuda()
    ff = cl(inp["ff"])
    sp = inp["sigma_param"].cuda() if learn else None
    runs = []
    for _ in range(2):
        table, out = nan(Fr, K, 3, g), nan(Fr, g, g, g, Cd)
        call("nm_op_combined", ctx.handle, P(kp), P(ff), P(sp), B, T, K, Fd, g, Cd, sigma, cat, P(table), P(out))
        torch.cuda.synchronize()
        runs.append((table, out))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "forward is not repeatable bit for bit"
    table, out = runs[0]
    sig = torch.full((K,), sigma, dtype=torch.float64) if not learn else torch.sigmoid(inp["sigma_param"].double()) * (2.0 * sigma)
    width = 2.0 * (sig / g) ** 2.0
    lin = torch.linspace(-1.0, 1.0, g).double()
    E = (-(lin.view(1, 1, 1, g) - inp["kp"].double().reshape(Fr, K, 4)[..., :3, None]).pow(2) / width.view(1, K, 1, 1)).exp()
    close("comb", case, "table", table, E)
    close("comb", case, "comb", uncl(out, C).reshape(B, T, C, g, g, g), ref["comb"])
    assert (out[..., C:] == 0).all()
    dcomb = cl(inp["dcomb"].reshape(Fr, Cd, g, g, g))
    dfeat, dkp, dsig = nan(Fr, g, g, g, Fd), nan(Fr, K, 4), nan(K) if learn else None
    call("nm_op_combined_backward", ctx.handle, P(dcomb), Cd, P(kp), P(sp), B, T, K, Fd, g, sigma, cat, P(dfeat), P(dkp), P(dsig))
    torch.cuda.synchronize()
    dfeat = dfeat.view(B, T, g, g, g, Fd)
    close("comb", case, "dff", uncl(dfeat[:, 0], Fd), ref["dff"])
    assert (dfeat[:, 1:] == 0).all()
    close("comb", case, "dkp", dkp.view(B, T, K, 4), ref["dkp"])
    if learn:
        close("comb", case, "dsigma", dsig, ref["dsigma"])


@pytest.mark.parametrize("case", R.TAIL_CASES, ids=str)
def test_decoder_tail(ctx, case):
    G, C, B, T, K, share, one, ill, per_voxel = case
    inp = R.tail_inputs(*case[:8])
    ref = R.ref_tail(inp, torch.float64)
    Fr, G3 = B * T, G * G * G
    x = cl(inp["x"].reshape(Fr, C, G, G, G))
    scale, shift = inp["scale"].reshape(Fr, C).contiguous().cuda(), inp["shift"].reshape(Fr, C).contiguous().cuda()
    w14, dloss = inp["w14"].cuda(), inp["dloss"].cuda()
    target = inp["target"].reshape(Fr, G3).contiguous().cuda()
    kp = inp["kp"].reshape(Fr, K, 4).contiguous().cuda()
    if share:                                    # every clip reads clip 0's first frame: stride 0
        first, stride = inp["first"][:1].reshape(1, G3).contiguous().cuda(), 0
    else:                                        # the network's addressing: clip b's first frame is frame b T of a (B T)-frame tensor
        first, stride = nan(B, T, G3), T
        first[:, 0] = inp["first"].reshape(B, G3).cuda()
    runs = []
    for _ in range(2):
        recon, sums = nan(Fr, G3), nan(Fr, 3)
        call("nm_op_decoder_tail", ctx.handle, P(x), P(scale), P(shift), R.LRELU, B, T, C, G, P(w14), P(first), stride, P(target), P(kp), K,
             P(recon), P(sums))
        torch.cuda.synchronize()
        runs.append((recon, sums))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "forward is not repeatable bit for bit"
    recon, sums = runs[0]
    close("tail", case, "recon", recon.view(B, T, 1, G, G, G), ref["recon"])
    for j, nm in enumerate(("bce", "cham", "cnt")):
        close("tail", case, nm, sums.view(B, T, 3)[..., j], ref["sums"][..., j])
    dA, dv = (None, nan(Fr, G3)) if per_voxel else (nan(Fr, G, G, G, C), None)
    dw, dkp = nan(C + 1), nan(Fr, K, 4)
    call("nm_op_decoder_tail_backward", ctx.handle, P(x), P(scale), P(shift), R.LRELU, Fr, C, G, P(w14), P(target), P(recon), P(sums), P(kp), K,
         P(dloss), P(dA), P(dv), P(dw), P(dkp))
    torch.cuda.synchronize()
    if per_voxel:                                # dA = dv (x) w14[0..C): the factor is the reference's dA at the largest weight, divided by it
        c = int(inp["w14"][:C].abs().argmax())
        close("tail", case, "dA", dv.view(B, T, G, G, G), ref["dA"][:, :, c] / inp["w14"][c].double())
    else:
        close("tail", case, "dA", uncl(dA, C).reshape(B, T, C, G, G, G), ref["dA"])
    close("tail", case, "dw14", dw, ref["dw14"])
    close("tail", case, "dkp", dkp.view(B, T, K, 4), ref["dkp"])


def _loss_close(case, got, ref):
    got = got.double().cpu()
    assert torch.isfinite(got).all()
    floor = 1e-6 * ref.abs().max().item()
    for i in range(11):
        e = abs(got[i].item() - ref[i].item()) / max(abs(ref[i].item()), floor)
        print("clip %s loss %d: %.3e" % (case, i, e))
        assert e <= REL, f"clip {case} loss {i}: {got[i].item()!r} against {ref[i].item()!r} ({e:.3e})"


@pytest.mark.parametrize("case", R.CLIP_CASES, ids=str)
def test_clip_losses(ctx, case):
    K, N, T, B, ver, flags, use_traj, with_aff, dg = case
    G = 32
    inp = R.clip_case_inputs(case)
    ref = R.ref_clip(inp, torch.float64, G, R.SEP_SIGMA, ver, flags, use_traj)
    Fr = B * T
    kp = inp["kp"].reshape(Fr, K, 4).contiguous().cuda()
    aff = inp["aff"].reshape(N, K, K).contiguous().cuda() if with_aff else None
    mean, sums, dloss = inp["heat_mean"].reshape(Fr, K).contiguous().cuda(), inp["sums"].reshape(Fr, 3).contiguous().cuda(), inp["dloss"].cuda()
    runs = []
    for _ in range(2):
        losses = nan(11)
        call("nm_op_clip_losses", ctx.handle, P(kp), P(aff), P(mean), P(sums), None, B, T, K, N, G, R.SEP_SIGMA, ver, flags, use_traj, 1, P(losses))
        torch.cuda.synchronize()
        runs.append(losses)
    assert torch.equal(runs[0], runs[1]), "forward is not repeatable bit for bit"
    _loss_close(case, runs[0], ref["losses"])
    dkp, dinfl = nan(Fr, K, 4), nan(B, K, K) if with_aff else None
    call("nm_op_clip_losses_backward", ctx.handle, P(kp), P(aff), P(dloss), B, T, K, N, R.SEP_SIGMA, ver, flags, use_traj, P(dkp), P(dinfl))
    torch.cuda.synchronize()
    close("clip", case, "dkp", dkp.view(B, T, K, 4), ref["dkp"])
    if with_aff:
        close("clip", case, "dinfl", dinfl, ref["dinfl"])


@pytest.mark.parametrize("case", R.AFF_CASES, ids=str)
def test_affinity(ctx, case):
    ver, K, N, B, gv, flags, seed = case
    inp = R.affinity_inputs(ver, K, N, B, seed)
    ref = R.ref_affinity(inp, torch.float64, gv, flags)
    params, dinfl, dloss = inp["params"].cuda(), inp["dinfl"].cuda(), inp["dloss"].cuda()
    runs = []
    for _ in range(2):
        aff = nan(N, K, K)
        call("nm_op_affinity", ctx.handle, P(params), N, K, ver, P(aff))
        torch.cuda.synchronize()
        runs.append(aff)
    assert torch.equal(runs[0], runs[1]), "forward is not repeatable bit for bit"
    close("aff", case, "aff", runs[0], ref["aff"])
    dp = nan(*params.shape)
    call("nm_op_affinity_backward", ctx.handle, P(params), P(runs[0]), P(dinfl), P(dloss), B, N, K, ver, gv, flags, P(dp))
    torch.cuda.synchronize()
    close("aff", case, "dparams", dp, ref["dparams"])


@pytest.mark.parametrize("case", R.VOLFIT_CASES, ids=str)
def test_volfit_gaussian(ctx, case):
    G, B, T, K = case
    inp = R.volfit_inputs(*case)
    ref = R.ref_volfit(inp, torch.float64, R.VOLFIT_SIGMA)
    Fr = B * T
    vox, kp, dloss = inp["vox"].reshape(Fr, G * G * G).contiguous().cuda(), inp["kp"].reshape(Fr, K, 4).contiguous().cuda(), inp["dloss"].cuda()
    runs = []
    for _ in range(2):
        vol = nan(Fr, 2)
        call("nm_op_volfit_gauss", ctx.handle, P(vox), P(kp), B, T, K, G, R.VOLFIT_SIGMA, P(vol))
        torch.cuda.synchronize()
        runs.append(vol)
    assert torch.equal(runs[0], runs[1]), "forward is not repeatable bit for bit"
    vol = runs[0].view(B, T, 2)
    close("vol", case, "den", vol[..., 1], ref["den"])
    close("vol", case, "vol", vol[..., 0].double().cpu() / vol[..., 1].double().cpu(), ref["vol"])
    dkp = nan(Fr, K, 4)
    call("nm_op_volfit_gauss_backward", ctx.handle, P(vox), P(kp), P(dloss), B, T, K, G, R.VOLFIT_SIGMA, P(dkp))
    torch.cuda.synchronize()
    close("vol", case, "dkp", dkp.view(B, T, K, 4), ref["dkp"])


def test_launchers_refuse_sizes_beyond_their_tiles(ctx):
    """g > 32 (the lane groups of heat_plane_marginals end at 32), K > 32 and a channel pitch below K are refused with a message, by the
    op entry and by the launchers under it."""
    L = lib()
    h = nan(8)
    for B, T, K, Kc, g in ((1, 1, 2, 8, 33), (1, 1, 33, 40, 8), (1, 1, 5, 4, 8), (1, 1, 5, 6, 8)):
        rc = L.load().nm_op_heatmaps(ctx.handle, P(h), P(h), P(h), B, T, K, Kc, g, 0, P(h), P(h), P(h))
        assert rc == L.NM_ERR_ARG and b"unsupported" in L.load().nm_last_error(), (B, T, K, Kc, g)
    rc = L.load().nm_op_clip_losses(ctx.handle, P(h), None, P(h), P(h), None, 1, 3, 1, 1, 32, 0.25, 1, 0, 1, 1, P(h))
    assert rc == L.NM_ERR_ARG
