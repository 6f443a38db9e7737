"""Reference for the op-level tests of the detector heads and losses (tests/test_heads_ops_gpu.py): the functions of oracle.nm_oracle and
tests/graph_loss_ref.py as they stand, run on float32 or float64 tensors, plus the glue the detector has between them and the seeded
inputs of every test family.

Glue only: softplus / propagate in both const_intensity forms (model/kypt_detector.py:336-345), the decoder's tail
sigmoid(10 (tanh(v) + first_frame - 0.5)) with BCELoss (:410, :91-92), the layout of the combined representation (:406-407) and the
eleven reported means (:155-165).  tests/test_heads_ref_cpu.py pins this glue against oracle.nm_oracle.detector_forward, which the
fixtures of tests/golden tie to the reference project.

Every generator draws in float64 from a seeded generator and rounds to float32, so the float32 run, the float64 run and the device see
the same numbers; `ref_*` evaluate one family in the dtype asked for and return values and torch-autograd adjoints."""

import torch
import torch.nn.functional as F

from oracle import nm_oracle as O
import graph_loss_ref as GL

LRELU = O.LRELU


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def f32(x):
    """round a float64 draw to float32 (the numbers every precision then shares)"""
    return x.float()


# ------------------------------------------------------------------------------------------------------------------------------------
# heat-maps -> keypoints
# ------------------------------------------------------------------------------------------------------------------------------------
def heatmaps(head, clip_head, prop, recurrent):
    """head (B,T,K,g,g,g), clip_head (B,K,g,g,g): the 1x1 heads' raw outputs; prop (3) = propagate_heatmaps weight[0], weight[1], bias.
    const_intensity 3 (recurrent False): every frame is propagated from the clip's map; 2: frame t from the heat-map of frame t - 1."""
    B, T, K, g = head.shape[:4]
    pw = prop[:2].reshape(1, 2, 1, 1, 1)
    pb = prop[2:3]
    prev = F.leaky_relu(clip_head, LRELU)
    out = []
    for t in range(T):
        hm = F.leaky_relu(head[:, t], LRELU)
        pair = torch.cat([hm.reshape(B * K, 1, g, g, g), prev.reshape(B * K, 1, g, g, g)], dim=1)
        hm = F.softplus(F.conv3d(pair, pw, pb)).view(B, K, g, g, g)
        if recurrent:
            prev = hm
        out.append(hm)
    return torch.stack(out, 1)


def keypoints_of(hm):
    """(B,T,K,g,g,g) -> (B,T,K,4) with the oracle's heatmap_to_keypoints per frame"""
    return torch.stack([O.heatmap_to_keypoints(hm[:, t]) for t in range(hm.shape[1])], 1)


HEAT_SPECIALS = ("", "corner", "last", "softplus")


def heat_inputs(g, K, B, T, recurrent, special="", seed=0):
    """head (B,T,K,g,g,g), clip_head (B,K,g,g,g), prop (3) [one weight negative], dkp (B,T,K,4), dloss (11) as float32 tensors.
    special: 'corner' - keypoint 0's mass sits in voxel (0,0,0), 'last' - in voxel (g-1,g-1,g-1); 'softplus' - softplus arguments of 19.5,
    20.5 and -40 at chosen voxels of frame 0."""
    gen = _gen(1000 * g + 10 * K + B + 100 * T + (7 if recurrent else 0) + seed)
    head = 1.5 * _randn(gen, B, T, K, g, g, g)
    clip = 1.5 * _randn(gen, B, K, g, g, g)
    # distinct mean levels per keypoint: the arg-max intensity is decided by a clear margin
    level = 0.35 * (torch.randperm(K, generator=gen).double() - (K - 1) / 2)
    head = head + level.view(1, 1, K, 1, 1, 1)
    prop = torch.tensor([0.9, -0.45, 0.15], dtype=torch.float64)
    w0, w1, pb = prop.tolist()

    def solve(c, u):            # head value a with w0 lrelu(a) + w1 lrelu(c) + pb = u
        r = (u - w1 * F.leaky_relu(c, LRELU) - pb) / w0
        return torch.where(r > 0, r, r / LRELU)

    if special in ("corner", "last"):
        i = 0 if special == "corner" else g - 1
        head[:, :, 0] = solve(clip[:, None, 0].expand(B, T, g, g, g), torch.tensor(-30.0, dtype=torch.float64))
        head[:, :, 0, i, i, i] = solve(clip[:, None, 0, i, i, i].expand(B, T), torch.tensor(15.0, dtype=torch.float64))
    if special == "softplus":
        for j, u in enumerate((19.5, 20.5, -40.0, 20.5, 19.5)):
            k, z, y, x = j % K, (3 * j) % g, (5 * j + 1) % g, (7 * j + 2) % g
            head[:, 0, k, z, y, x] = solve(clip[:, k, z, y, x], torch.tensor(u, dtype=torch.float64))
    dkp = _randn(gen, B, T, K, 4)
    dloss = torch.zeros(11, dtype=torch.float64)
    dloss[4] = 0.7
    return dict(head=f32(head), clip_head=f32(clip), prop=f32(prop), dkp=f32(dkp), dloss=f32(dloss), recurrent=bool(recurrent))


def ref_heat(inp, dtype):
    head = inp["head"].to(dtype).requires_grad_(True)
    clip = inp["clip_head"].to(dtype).requires_grad_(True)
    prop = inp["prop"].to(dtype).requires_grad_(True)
    hm = heatmaps(head, clip, prop, inp["recurrent"])
    kp = keypoints_of(hm)
    mean = hm.mean(dim=(3, 4, 5))
    L = (kp * inp["dkp"].to(dtype)).sum() + inp["dloss"][4].to(dtype) * O.loss_sparsity(hm).mean()
    dhead, dclip, dprop = torch.autograd.grad(L, [head, clip, prop])
    return dict(heatmaps=hm.detach(), keypoints=kp.detach(), heat_mean=mean.detach(), dhead=dhead, dclip_head=dclip, dprop=dprop)


# ------------------------------------------------------------------------------------------------------------------------------------
# Gaussian table -> combined representation
# ------------------------------------------------------------------------------------------------------------------------------------
def combined(kp, first_feature, sigma, g, cat):
    """kp (B,T,K,4), first_feature (B,Fd,g,g,g) -> (B,T,2K+Fd+3,g,g,g): [gauss_t | first feature | gauss_0 | x1 x2 x3]
    (kypt_detector.py:396-407); sigma a float or a (K,) tensor; cat 0 none / 1 max / 2 sum"""
    B, T = kp.shape[:2]
    ga = torch.stack([O.gaussian_map(kp[:, t], sigma, g) for t in range(T)], 1)
    if cat == 1:
        ga = ga.max(dim=2, keepdim=True).values.expand_as(ga)
    elif cat == 2:
        ga = ga.sum(dim=2, keepdim=True).clip(0, 1).expand_as(ga)
    return torch.stack([O.add_coords(torch.cat([ga[:, t], first_feature, ga[:, 0]], dim=1)) for t in range(T)], 1), ga


def combined_inputs(g, K, B, T, Fd, cat, learn, sigma, seed=0):
    gen = _gen(31 * g + 7 * K + B + 3 * T + 1000 * cat + (500 if learn else 0) + seed)
    kp = torch.cat([1.6 * _rand(gen, B, T, K, 3) - 0.8, 0.1 + 0.9 * _rand(gen, B, T, K, 1)], dim=-1)
    kp[:, :, 0, :3] = 1.3 * kp[:, :, 0, :3] + 0.2                  # (one keypoint may leave [-1, 1])
    ff = _randn(gen, B, Fd, g, g, g)
    Cd = (2 * K + Fd + 3 + 7) // 8 * 8
    dcomb = _randn(gen, B, T, Cd, g, g, g)
    sp = 0.8 * _randn(gen, K) if learn else None
    return dict(kp=f32(kp), ff=f32(ff), dcomb=f32(dcomb), sigma_param=None if sp is None else f32(sp), sigma=sigma, cat=cat, g=g, Cd=Cd)


def ref_combined(inp, dtype):
    kp = inp["kp"].to(dtype).requires_grad_(True)
    ff = inp["ff"].to(dtype).requires_grad_(True)
    sp = None if inp["sigma_param"] is None else inp["sigma_param"].to(dtype).requires_grad_(True)
    sig = inp["sigma"] if sp is None else torch.sigmoid(sp) * (inp["sigma"] * 2.0)
    comb, ga = combined(kp, ff, sig, inp["g"], inp["cat"])
    C = comb.shape[2]
    L = (comb * inp["dcomb"].to(dtype)[:, :, :C]).sum()
    gr = torch.autograd.grad(L, [kp, ff] + ([sp] if sp is not None else []))
    return dict(comb=comb.detach(), gauss=ga.detach(), dkp=gr[0], dff=gr[1], dsigma=gr[2] if sp is not None else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# decoder tail
# ------------------------------------------------------------------------------------------------------------------------------------
def tail(act, w14, b14, first_frame):
    """act (B,T,C,G,G,G) the decoder's last activated tensor, w14 (C), b14 (1), first_frame (B,1,G,G,G) -> recon (B,T,1,G,G,G)"""
    C = act.shape[2]
    out = []
    for t in range(act.shape[1]):
        v = F.conv3d(act[:, t], w14.view(1, C, 1, 1, 1), b14)
        out.append(torch.sigmoid(10.0 * (torch.tanh(v) + first_frame - 0.5)))
    return torch.stack(out, 1)


def tail_inputs(G, C, B, T, K, share_first, one_voxel=False, ill=False, seed=0):
    """raw x (B,T,C,G,G,G) with per-frame scale / shift (B,T,C), w14 (C+1), target (B,T,1,G,G,G) in {0,1}, first (B,1,G,G,G) [clip b's
    first frame, or clip 0's for every clip with share_first], keypoints (B,T,K,4) partly outside [-1,1].  A few hundred voxels of `first`
    carry values that saturate the sigmoid against the opposite target: pre in [40,60] and [110,130] where the target is 0, [-45,-25],
    [-75,-55] and [-130,-110] where it is 1 - every one of them is clamped (or not) alike in float32 and float64.  ill: also pre in
    [25,35] against target 0, where float32 has 1 - p == 0 (log clamped at -100) and float64 has not."""
    gen = _gen(17 * G + C + 5 * B + 3 * T + K + (100 if share_first else 0) + (200 if one_voxel else 0) + seed)
    x = _randn(gen, B, T, C, G, G, G)
    scale = 0.5 + _rand(gen, B, T, C)
    shift = 0.3 * _randn(gen, B, T, C)
    w14 = torch.cat([0.25 * _randn(gen, C), torch.tensor([0.1], dtype=torch.float64)])
    target = (_rand(gen, B, T, 1, G, G, G) < 0.004).double()
    if one_voxel:
        target.zero_()
        for b in range(B):
            for t in range(T):
                i = torch.randint(0, G, (3,), generator=gen)
                target[b, t, 0, i[0], i[1], i[2]] = 1.0
    nb = 1 if share_first else B
    first = target[:nb, 0].clone()
    flat = first.view(nb, -1)
    tf = target[:, 0].reshape(B, -1)
    n = flat.shape[1]
    for b in range(nb):
        idx = torch.randperm(n, generator=gen)[:600]
        for j, i in enumerate(idx.tolist()):
            if tf[b, i].item() == 0.0:
                flat[b, i] = (5.5, 12.5, 3.5 if ill else 5.5)[j % 3]
            else:
                flat[b, i] = (-3.0, -6.0, -11.5)[j % 3]
        # (occupied voxels are rare: give the target-1 side its share explicitly)
        occ = torch.nonzero(tf[b]).flatten().tolist()
        for j, i in enumerate(occ[:30]):
            flat[b, i] = (-3.0, -6.0, -11.5, 1.0)[j % 4]
    if share_first:
        first = first.expand(B, 1, G, G, G).clone()
    kp = torch.cat([3.0 * _rand(gen, B, T, K, 3) - 1.5, _rand(gen, B, T, K, 1)], dim=-1)
    dloss = torch.zeros(11, dtype=torch.float64)
    dloss[0], dloss[1] = 1.3, 0.6
    return dict(x=f32(x), scale=f32(scale), shift=f32(shift), w14=f32(w14), target=f32(target), first=f32(first), kp=f32(kp),
                dloss=f32(dloss), share_first=share_first)


def ref_tail(inp, dtype):
    x, sc, sh = inp["x"].to(dtype), inp["scale"].to(dtype), inp["shift"].to(dtype)
    act = F.leaky_relu(x * sc[..., None, None, None] + sh[..., None, None, None], LRELU).requires_grad_(True)
    w = inp["w14"].to(dtype).requires_grad_(True)
    kp = inp["kp"].to(dtype).requires_grad_(True)
    target, first = inp["target"].to(dtype), inp["first"].to(dtype)
    C = x.shape[2]
    recon = tail(act, w[:C], w[C:], first)
    bce = F.binary_cross_entropy(recon, target, reduction="none")
    c = O.coord_channels(target.shape[3:])
    B, T = target.shape[:2]
    d = (c[None, None, None] - kp.detach()[..., :3][..., None, None, None]).pow(2).sum(dim=3)  # (B,T,K,G,G,G)
    dmin = d.min(dim=2, keepdim=True)
    cham = (dmin.values * target).sum(dim=(2, 3, 4, 5))
    cnt = target.sum(dim=(2, 3, 4, 5))
    vol = O.loss_volume_chamfer(target, kp)
    L = inp["dloss"][0].to(dtype) * bce.mean(dim=(2, 3, 4, 5)).mean() + inp["dloss"][1].to(dtype) * vol.mean()
    dA, dw, dkp = torch.autograd.grad(L, [act, w, kp])
    return dict(recon=recon.detach(), sums=torch.stack([bce.sum(dim=(2, 3, 4, 5)), cham, cnt], -1).detach(), dA=dA, dw14=dw, dkp=dkp,
                argmin=dmin.indices.detach(), dist=d.detach())


# ------------------------------------------------------------------------------------------------------------------------------------
# the eleven losses from keypoints, affinity, heat-map means and the tail's per-frame sums
# ------------------------------------------------------------------------------------------------------------------------------------
NM_GRAPH_LOCAL_OFF, NM_GRAPH_TIME_OFF, NM_GRAPH_SPARSITY_OFF, NM_GRAPH_DETACH = 1, 2, 4, 8


def losses11(kp, aff, heat_mean, sums, G, sep_sigma, ver=1, flags=0, use_traj=1, vol=None):
    """the eleven means of KyptDetector.forward (kypt_detector.py:155-165) in the order of nm_detector_forward's losses11.
    kp (B,T,K,4), aff (N,K,K,1) or None, heat_mean (B,T,K), sums (B,T,3) = BCE sum, chamfer sum, occupied count per frame;
    vol (B,T) replaces the chamfer ratio (vol_fit_type 'gaussian')"""
    z = torch.zeros((), dtype=kp.dtype)
    rec = (sums[..., 0] / float(G) ** 3).mean()
    volm = (sums[..., 1] / sums[..., 2]).mean() if vol is None else vol.mean()
    sep = O.loss_separation(kp, sep_sigma).mean()
    spars = heat_mean.abs().mean(dim=2).mean()
    if aff is None:
        lo = ti = sp = tr = z
    else:
        kk = kp.detach() if flags & NM_GRAPH_DETACH else kp
        a, b, c, _ = GL.graph_consistency(kk, aff, ver, not flags & NM_GRAPH_LOCAL_OFF, not flags & NM_GRAPH_TIME_OFF,
                                          not flags & NM_GRAPH_SPARSITY_OFF)
        lo, ti, sp = a.mean(), b.mean(), c.mean()
        tr = GL.graph_traj(kk, aff, ver).mean() if use_traj else z
    return torch.stack([rec, volm, z, sep, spars, lo, ti, sp, z, tr, z])


CLIP_DEGENERATE = ("", "still", "steady", "same", "all", "creep")


def clip_inputs(K, N, T, B, degenerate="", with_aff=True, seed=0):
    """keypoints (B,T,K,4) on a 2^-12 lattice (differences of positions are exact in float32), affinity (N,K,K,1), heat_mean (B,T,K),
    sums (B,T,3), dloss (11).  degenerate: 'still' - keypoint 0 does not move from frame 0 to 1 (velocity clamp), 'steady' - keypoint
    K-1 moves with exactly constant velocity over frames 0..2 (acceleration clamp), 'same' - keypoints 0 and 1 coincide in every frame
    (K > 2), 'all' - the three together; 'creep' - keypoint 0 moves by 2^-22 from frame 0 to 1 and keypoint K-1's acceleration over frames
    0..2 is 2^-22: norms below the 1e-6 clamp but not zero, where torch's cosine_similarity divides by the clamp and still differentiates
    the norm; intensities of 0 and 1 are always present."""
    gen = _gen(97 * K + 13 * N + 5 * T + B + seed + 1000 * CLIP_DEGENERATE.index(degenerate))
    q = 4096.0
    p0 = 1.4 * _rand(gen, B, 1, K, 3) - 0.7
    vel = 0.06 * _randn(gen, B, T, K, 3)
    pos = torch.round((p0 + vel.cumsum(dim=1)) * q) / q
    if degenerate in ("still", "all"):
        pos[:, 1, 0] = pos[:, 0, 0]
    if degenerate in ("steady", "all"):
        v = torch.round(0.05 * _randn(gen, B, 3) * q) / q + 8.0 / q
        pos[:, 1, K - 1] = pos[:, 0, K - 1] + v
        pos[:, 2, K - 1] = pos[:, 0, K - 1] + 2 * v
    if degenerate in ("same", "all") and K > 2:
        pos[:, :, 1] = pos[:, :, 0]
    if degenerate == "creep":
        tiny = 2.0 ** -22
        pos[:, 1, 0] = pos[:, 0, 0] + torch.tensor([tiny, 0.0, -tiny], dtype=torch.float64)
        v = torch.round(0.05 * _randn(gen, B, 3) * q) / q + 8.0 / q
        pos[:, 1, K - 1] = pos[:, 0, K - 1] + v
        pos[:, 2, K - 1] = pos[:, 0, K - 1] + 2 * v + torch.tensor([0.0, tiny, 0.0], dtype=torch.float64)
    inten = 0.05 + 0.9 * _rand(gen, B, T, K, 1)
    inten[:, 0, 0] = 0.0
    inten[:, T - 1, K - 1] = 1.0
    kp = torch.cat([pos, inten], dim=-1)
    aff = None
    if with_aff:
        aff = torch.softmax(2.0 * _randn(gen, N, K, K), dim=-1) * (1 - torch.eye(K, dtype=torch.float64))
        aff = aff[..., None]
    heat_mean = 0.4 * _randn(gen, B, T, K)
    sums = torch.stack([2000 + 500 * _rand(gen, B, T), 3 + _rand(gen, B, T), torch.round(200 + 50 * _rand(gen, B, T))], -1)
    dloss = torch.tensor([0, 0, 0, 0.8, 0, 1.1, 0.9, 0, 0, 0.7, 0], dtype=torch.float64)
    return dict(kp=f32(kp), aff=None if aff is None else f32(aff), heat_mean=f32(heat_mean), sums=f32(sums), dloss=f32(dloss))


def ref_clip(inp, dtype, G, sep_sigma, ver, flags, use_traj):
    kp = inp["kp"].to(dtype).requires_grad_(True)
    aff = None if inp["aff"] is None else inp["aff"].to(dtype)
    w = inp["dloss"].to(dtype)
    B, K = kp.shape[0], kp.shape[2]
    losses = losses11(kp, aff, inp["heat_mean"].to(dtype), inp["sums"].to(dtype), G, sep_sigma, ver, flags, use_traj)
    dkp, = torch.autograd.grad((losses * w).sum(), [kp])
    dinfl = None
    if aff is not None:
        # per clip: d (sum_i w_i loss_i) / d influence with the influence a leaf; every term is a mean over clips
        M = GL.influence(aff, ver)
        dinfl = []
        for b in range(B):
            Mb = M.clone().requires_grad_(True)
            lb = losses11(kp[b:b + 1].detach(), Mb[None, :, :, None], inp["heat_mean"][b:b + 1].to(dtype), inp["sums"][b:b + 1].to(dtype), G,
                          sep_sigma, 1 if ver == 1 else 0, flags | NM_GRAPH_SPARSITY_OFF, use_traj)
            gb, = torch.autograd.grad((lb * w).sum(), [Mb], allow_unused=True)
            dinfl.append(torch.zeros_like(M) if gb is None else gb / B)
        dinfl = torch.stack(dinfl)
    return dict(losses=losses.detach(), dkp=dkp, dinfl=dinfl)


def clip_selection_margins(inp, dtype):
    """the discontinuous choices of the clip losses on these inputs: index of the max over neighbours, and the time term's |.| arguments
    relative to the largest distance of their pair (exact zeros of coincident keypoints excepted)"""
    kp = inp["kp"].to(dtype)
    out = {}
    if inp["aff"] is not None:
        out["argmax_n"] = inp["aff"].to(dtype).squeeze(-1).max(dim=0).indices
    pos = kp[..., :3]
    dist = (pos[:, :, :, None] - pos[:, :, None]).pow(2).sum(dim=-1)
    dev = dist - dist.mean(dim=1, keepdim=True)
    out["abs_arg_rel"] = dev / dist.amax(dim=1, keepdim=True).clamp(min=1e-30)
    out["sign"] = torch.sign(dev)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# affinity
# ------------------------------------------------------------------------------------------------------------------------------------
def affinity_inputs(ver, K, N, B, seed=0):
    gen = _gen(11 * ver + 3 * K + N + seed)
    shape = (N, K, K - 1) if ver == 3 else (N, K, K)
    p = 2.5 * _randn(gen, *shape)
    if K > 2:
        # logits up to +-30 (softplus beyond / at its threshold 20, the softmax's range) in distinct (row, column) cells, so that the max
        # over the neighbours is never a tie of two saturated rows; K = 2 stays moderate (a saturated two-entry softmax has no gradient left)
        cols = shape[2]
        cells = torch.randperm(K * cols, generator=gen)[:max(4, K * cols // 14)].tolist()
        for i, c in enumerate(cells):
            big = (30.0 - 3.0 * _rand(gen, 1)).item()
            p[i % N, c // cols, c % cols] = big if (i // N) % 2 == 0 else -big
        if ver in (1, 2):
            p[0, cells[0] // cols, cells[0] % cols] = 20.5
            p[N - 1, cells[1] // cols, cells[1] % cols] = 19.5
    dinfl = _randn(gen, B, K, K)
    dloss = torch.zeros(11, dtype=torch.float64)
    dloss[7] = 0.9
    return dict(params=f32(p), dinfl=f32(dinfl), dloss=f32(dloss), ver=ver)


def ref_affinity(inp, dtype, graph_ver, flags):
    p = inp["params"].to(dtype).requires_grad_(True)
    aff = O.affinity(p, inp["ver"])
    L = (inp["dinfl"].to(dtype).sum(dim=0) * GL.influence(aff, graph_ver)).sum()
    if not flags & NM_GRAPH_SPARSITY_OFF:
        a = aff.squeeze(-1)
        sp = (a[:, None] * a[None]).pow(2).sum(dim=1, keepdim=True) - a[:, None].pow(4)
        L = L + inp["dloss"][7].to(dtype) * sp.sum(dim=(0, 1)).mean()
    dp, = torch.autograd.grad(L, [p])
    return dict(aff=aff.detach().squeeze(-1), dparams=dp, argmax_n=aff.detach().squeeze(-1).max(dim=0).indices)


# ------------------------------------------------------------------------------------------------------------------------------------
# vol_fit_type 'gaussian'
# ------------------------------------------------------------------------------------------------------------------------------------
def volfit_inputs(G, B, T, K, seed=0):
    gen = _gen(5 * G + B + 3 * T + K + seed)
    vox = (_rand(gen, B, T, 1, G, G, G) < 0.01).double()
    kp = torch.cat([1.6 * _rand(gen, B, T, K, 2) - 0.8, 0.3 + 0.7 * _rand(gen, B, T, K, 1), _rand(gen, B, T, K, 1)], dim=-1)
    dloss = torch.zeros(11, dtype=torch.float64)
    dloss[1] = 1.2
    return dict(vox=f32(vox), kp=f32(kp), dloss=f32(dloss))


def ref_volfit(inp, dtype, sigma):
    kp = inp["kp"].to(dtype).requires_grad_(True)
    vox = inp["vox"].to(dtype)
    vol = O.loss_volume_gaussian(vox, kp, sigma)
    dkp, = torch.autograd.grad(inp["dloss"][1].to(dtype) * vol.mean(), [kp])
    # the selection: first maximal map per pixel
    B, T, K = kp.shape[:3]
    G = vox.shape[3]
    width = 2.0 * (sigma * 4.0 / G) ** 2.0
    lin = torch.linspace(-1.0, 1.0, G, dtype=dtype)
    c = kp.detach()
    e0 = (-(lin - c[..., 0, None]).pow(2) / width).exp()
    e1 = (-(lin - c[..., 1, None]).pow(2) / width).exp()
    m = e0[..., :, None] * e1[..., None, :] * c[..., 2, None, None]                   # (B,T,K,G,G)
    return dict(vol=vol.detach(), den=vox.sum(dim=(2, 3, 4, 5)), dkp=dkp, argmax=m.max(dim=2).indices, maps=m)


def top2_gap(values, dim, largest=True):
    """relative gap between the best and the second best along dim (how clearly a max / min selection is decided)"""
    v = values if largest else -values
    t = v.topk(2, dim=dim).values
    a, b = t.select(dim, 0), t.select(dim, 1)
    return (a - b).abs() / torch.maximum(a.abs(), b.abs()).clamp(min=1e-300)


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases (shared by tests/test_heads_ref_cpu.py, which checks the selections' margins on them, and tests/test_heads_ops_gpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------
# g, K, B, T, recurrent, special.  g: both sides of the lane-group boundaries 8 | 16 | 32 of heat_plane_marginals, ragged and full groups;
# K: wave striding (k = wave, wave + 4, ...), Kc padding (2, 5 -> 8), the quad-load tail (5); g = 32 with K = 24 / 32: 96 / 128 KB of LDS
HEAT_CASES = [
    (8, 2, 1, 1, 0, ""), (8, 5, 3, 4, 1, "softplus"), (10, 5, 3, 1, 0, "softplus"), (10, 24, 1, 2, 1, ""), (14, 24, 1, 4, 0, ""),
    (14, 2, 3, 1, 1, ""), (16, 32, 1, 4, 0, ""), (16, 5, 1, 7, 1, ""), (18, 2, 3, 4, 0, ""), (18, 32, 1, 2, 1, ""), (24, 24, 3, 1, 0, ""),
    (24, 5, 1, 4, 1, ""), (30, 5, 1, 4, 0, ""), (30, 24, 1, 1, 1, ""), (32, 32, 1, 2, 0, ""), (32, 32, 1, 2, 1, ""), (32, 24, 3, 1, 0, ""),
    (32, 24, 1, 4, 1, ""), (32, 2, 1, 1, 0, ""), (10, 5, 1, 2, 0, "corner"), (18, 5, 1, 2, 1, "last"), (32, 5, 1, 1, 0, "last"),
    (8, 24, 1, 2, 1, "corner"),
]
# g, K, B, T, Fd, cat, learnable widths, sigma
COMBINED_CASES = [
    (8, 2, 1, 1, 8, 0, False, 1.5), (10, 5, 3, 2, 8, 0, False, 1.5), (8, 24, 1, 3, 128, 0, True, 1.5), (10, 5, 1, 4, 12, 1, False, 3.0),
    (8, 24, 3, 1, 8, 1, True, 3.0), (10, 5, 1, 4, 12, 2, False, 3.0), (8, 12, 3, 2, 8, 2, True, 3.0), (12, 32, 1, 2, 4, 0, False, 1.5),
]
# G, C, B, T, K, clips share clip 0's first frame, one occupied voxel per frame, ill-conditioned saturation, per-voxel form of dA
TAIL_CASES = [
    (32, 32, 1, 3, 24, False, False, False, False), (40, 32, 2, 2, 5, False, False, False, False), (40, 32, 2, 2, 24, True, False, False, True),
    (32, 32, 1, 3, 2, False, True, False, True), (32, 16, 1, 3, 5, False, False, False, False), (40, 16, 2, 1, 24, True, True, False, False),
    (32, 32, 1, 3, 5, False, False, True, False),
]
# K, N, T, B, graph_ver, flags, use_traj, affinity present, degenerate.  (T < 3: the trajectory mean over T - 2 acceleration terms divides
# by zero in the reference too, so those lengths are not cases.)
CLIP_CASES = (
    [(K, N, T, B, 1, 0, 1, True, "") for K, N, T, B in ((2, 1, 3, 1), (12, 2, 4, 3), (32, 3, 9, 1), (12, 3, 3, 3), (32, 1, 4, 1), (2, 2, 9, 3))]
    + [(12, 2, 4, 3, ver, 0, 1, True, "") for ver in (0, 2)] + [(32, 3, 9, 1, ver, 0, 1, True, "") for ver in (0, 2)]
    + [(12, 2, 4, 3, ver, fl, 1, True, "") for ver in (1, 2) for fl in (1, 2, 4, 8)]
    + [(12, 2, 4, 3, 1, 0, 0, True, ""), (12, 2, 4, 3, 0, 0, 0, True, ""), (12, 2, 4, 3, 1, 0, 1, False, ""), (32, 1, 3, 3, 2, 0, 1, False, "")]
    + [(12, 2, 4, 3, ver, 0, 1, True, dg) for ver in (1, 0) for dg in ("still", "steady", "same")]
    + [(12, 2, 4, 3, 1, 0, 1, True, "creep"), (12, 2, 4, 3, 2, 0, 1, True, "creep"), (2, 1, 3, 1, 1, 0, 1, True, "creep")]
    + [(2, 1, 3, 1, 1, 0, 1, True, "still"), (2, 2, 4, 3, 2, 0, 1, True, "steady"), (32, 3, 9, 1, 2, 0, 1, True, "all"), (12, 2, 3, 1, 1, 0, 1, True, "all")]
)
# seeds of clip_inputs at which every |.| argument of the time term is at least 1e-4 of its pair's largest squared distance and the max over
# the neighbours is decided by 1e-4 (tests/test_heads_ref_cpu.py asserts both); key (K, N, T, B, degenerate, affinity present), default 0
CLIP_SEEDS = {(32, 3, 9, 1, "", True): 37, (12, 3, 3, 3, "", True): 2, (32, 1, 4, 1, "", True): 1, (32, 1, 3, 3, "", False): 236,
              (12, 2, 4, 3, "still", True): 6, (12, 2, 4, 3, "steady", True): 3, (12, 2, 4, 3, "same", True): 4, (32, 3, 9, 1, "all", True): 109, (12, 2, 4, 3, "creep", True): 1}


def clip_case_inputs(case):
    K, N, T, B, ver, flags, use_traj, with_aff, dg = case
    return clip_inputs(K, N, T, B, dg, with_aff, seed=CLIP_SEEDS.get((K, N, T, B, dg, with_aff), 0))


# affinity version, K, N, B, graph_ver, flags, seed
AFF_CASES = [(ver, K, N, B, gv, fl, 3 if (ver, K) == (2, 32) else 0) for ver in (0, 1, 2, 3)
             for K, N, B, gv, fl in ((2, 1, 1, 1, 0), (24, 3, 3, 2, 0), (32, 3, 1, 1, 4), (24, 1, 3, 0, 0))]
# G, B, T, K
VOLFIT_CASES = [(32, 1, 2, 5), (32, 3, 2, 24), (40, 1, 3, 2), (40, 3, 1, 5)]
VOLFIT_SIGMA = 4.0
SEP_SIGMA = 0.25        # (the shipped 0.02 makes every off-diagonal separation term exp(-500): nothing left to compare)
