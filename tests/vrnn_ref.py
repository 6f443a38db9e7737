"""fp64 reference for the VRNN (model/hsvrnn_bvh.py): the CPU oracle's own functions (oracle/nm_oracle.py, pinned to the reference
by G14) evaluated in float64, next to the same functions in the oracle's fp32.

The fp32 oracle is the reference's arithmetic; its distance from the fp64 evaluation is the rounding noise that ANY fp32 evaluation of
the model carries at that shape, and it grows with the batch, the sequence length and the conditioning of the 6-D rotations.  The GPU
tests (tests/test_vrnn_batch_paths_gpu.py) hold the HIP kernels to fp64 and size their bounds by the fp32 oracle's own deviation.
The best-of-S selections are discrete: a seed is usable only when every selection has a clear winner in fp64 (selection_margins);
tests/test_vrnn_ref_cpu.py checks that for every seed the GPU tests use."""
import contextlib

import torch

from neural_marionette_amd import HotPathOptions, synth
from oracle import nm_oracle as O

DYN = O.DYN
MARGIN_MIN = 1e-4          # smallest relative gap (second best - best) / best of a best-of-S selection a GPU test may depend on


@contextlib.contextmanager
def float64():
    """the oracle allocates with the default dtype (fk_decode's torch.zeros(B, K, 3)): fp64 inside, restored on exit"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@contextlib.contextmanager
def precision(dtype):
    if dtype == torch.float64:
        with float64():
            yield
    else:
        yield


def cast(sd, dtype=torch.float64):
    """the dyna_module.* entries in `dtype` (the detector's are left alone)"""
    return {k: (v.to(dtype) if k.startswith(DYN + ".") and v.is_floating_point() else v) for k, v in sd.items()}


def _t(x, dtype):
    return torch.as_tensor(x).detach().cpu().to(dtype)


def _err(a, b):
    return (_t(a, torch.float64) - _t(b, torch.float64)).abs().max().item()


# ---- whole-sequence calls ---------------------------------------------------------------------------------------------------
def encode(sd, o, kp, order, parents, eps, dtype=torch.float64):
    """HSVRNNBVH.encode (O.vrnn_encode) in `dtype`"""
    with precision(dtype), torch.no_grad():
        return O.vrnn_encode(cast(sd, dtype), o, _t(kp, dtype), order, parents, _t(eps, dtype))


def generate(sd, o, kp_cond, order, parents, Ttot, Tcond, eps_post, eps_prior, dtype=torch.float64):
    """HSVRNNBVH.generate (O.vrnn_generate) in `dtype`"""
    with precision(dtype), torch.no_grad():
        return O.vrnn_generate(cast(sd, dtype), o, _t(kp_cond, dtype), order, parents, Ttot, Tcond, _t(eps_post, dtype),
                               _t(eps_prior, dtype))


def learner_grads(sd, o, kp, order, parents, eps, w_rec=1.0, w_kl=0.003, dtype=torch.float64):
    """d(w_rec kypt_recon_loss + w_kl kl_kypt) / d(every trainable dyna_module parameter) by autograd in `dtype`
    (test_network_gpu._oracle_learner_grads in either precision) -> (loss, {name: grad})"""
    names = [k for k in sd if k.startswith(DYN + ".") and k != DYN + ".offset_param"]
    with precision(dtype):
        sdd = cast(sd, dtype)
        leaf = {k: sdd[k].clone().requires_grad_(True) for k in names}
        sdd.update(leaf)
        r = O.vrnn_encode(sdd, o, _t(kp, dtype), order, parents, _t(eps, dtype))
        loss = w_rec * r["kypt_recon_loss"] + w_kl * r["kl_kypt"]
        grads = torch.autograd.grad(loss, [leaf[k] for k in names])
    return float(loss.detach()), dict(zip(names, grads))


def adam_trajectory(sd, o, kp, order, parents, epss, lr=4e-4, w_rec=1.0, w_kl=0.003, dtype=torch.float64):
    """learner-mode training steps (detector frozen: fixed keypoints) with torch.optim.Adam in `dtype`, one step per eps in `epss` ->
    (loss of each step, {name: parameter after the last step})"""
    names = [k for k in sd if k.startswith(DYN + ".") and k != DYN + ".offset_param"]
    with precision(dtype):
        sdd = cast(sd, dtype)
        leaf = {k: sdd[k].clone().requires_grad_(True) for k in names}
        opt = torch.optim.Adam([leaf[k] for k in names], lr=lr)
        losses = []
        for e in epss:
            s2 = dict(sdd); s2.update(leaf)
            r = O.vrnn_encode(s2, o, _t(kp, dtype), order, parents, _t(e, dtype))
            loss = w_rec * r["kypt_recon_loss"] + w_kl * r["kl_kypt"]
            opt.zero_grad(); loss.backward(); opt.step()
            losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in leaf.items()}


# ---- single operations ------------------------------------------------------------------------------------------------------
def mlp(sd, x, which, dtype=torch.float64):
    """which: extract_post_dist / extract_prior_dist / root_intensity_decoder (tanh) / joint_matrix_decoder"""
    with precision(dtype), torch.no_grad():
        return O._mlp(_t(x, dtype), cast(sd, dtype), DYN + "." + which, tanh=(which == "root_intensity_decoder"))


def gru(sd, x, h, dtype=torch.float64):
    with precision(dtype), torch.no_grad():
        return O.gru_cell(cast(sd, dtype), _t(x, dtype), _t(h, dtype))


def fk(sd, dec_in, offset, order, parents, dtype=torch.float64):
    """extract_kypt_from_latent_and_state -> (flat (B,4K), R (B,K,3,3)); offset (B,K,3[,1])"""
    with precision(dtype), torch.no_grad():
        off = _t(offset, dtype).reshape(dec_in.shape[0], -1, 3, 1)
        return O.fk_decode(cast(sd, dtype), _t(dec_in, dtype), off, order, parents)


def offsets(sd, kp, parents, dtype=torch.float64):
    with precision(dtype), torch.no_grad():
        return O.bone_offsets(cast(sd, dtype), _t(kp, dtype), parents)


def rot6d_conditioning(sd, dec_in, K):
    """per row, the worst joint's |b| / |x^ x b| of the joint decoder's 6-D rotations (a, b): the Gram-Schmidt step of rot6d divides by
    |x^ x b|, so this ratio is the amplification of a rounding error in b into the rotation.  dec_in (..., H+Z) -> (...)"""
    p = mlp(sd, dec_in, "joint_matrix_decoder").reshape(*dec_in.shape[:-1], K, 6)
    a, b = p[..., :3], p[..., 3:]
    x = a / a.norm(dim=-1, keepdim=True)
    return (b.norm(dim=-1) / torch.cross(x, b, dim=-1).norm(dim=-1)).max(dim=-1).values


def rot6d_sensitivity(sd, dec_in, K):
    """per row, the worst joint's 1 / |a| + 1 / |x^ x b|: how much an ABSOLUTE rounding error of the joint decoder's outputs (of about the
    same size on every row) moves the rotation - both normalisations of rot6d divide by these lengths.  dec_in (..., H+Z) -> (...)"""
    p = mlp(sd, dec_in, "joint_matrix_decoder").reshape(*dec_in.shape[:-1], K, 6)
    a, b = p[..., :3], p[..., 3:]
    x = a / a.norm(dim=-1, keepdim=True)
    return (1.0 / a.norm(dim=-1) + 1.0 / torch.cross(x, b, dim=-1).norm(dim=-1)).max(dim=-1).values


def posterior_all(sd, h, obs, eps, offset, order, parents, dtype=torch.float64):
    """One posterior step (O._posterior_step, hsvrnn_bvh.py:99-128) with every sample kept: z (S,B,Z), keypoints (S,B,4K), R (S,B,K,3,3),
    the state each sample leads to (S,B,H), the distances d (S,B) the selection minimises and the decoder inputs (S,B,H+Z)."""
    with precision(dtype), torch.no_grad():
        sdd = cast(sd, dtype)
        B = h.shape[0]
        h, obs, eps = _t(h, dtype), _t(obs, dtype).reshape(B, -1), _t(eps, dtype)
        off = _t(offset, dtype).reshape(B, -1, 3, 1)
        mu, sig = O._dist_params(O._mlp(torch.cat([h, obs], -1), sdd, DYN + ".extract_post_dist"))
        z = mu[None] + eps * sig[None]
        dec = torch.cat([h.expand(z.shape[0], -1, -1), z], -1)
        flats, Rs, hs = [], [], []
        for i in range(z.shape[0]):
            f, R = O.fk_decode(sdd, dec[i], off, order, parents)
            flats.append(f); Rs.append(R)
            hs.append(O.gru_cell(sdd, torch.cat([f, z[i]], -1), h))
        flats = torch.stack(flats, 0)
        d = (obs[None] - flats).pow(2).sum(-1)
        return dict(z=z, kp=flats, R=torch.stack(Rs, 0), h=torch.stack(hs, 0), d=d, dec=dec)


def prior_step(sd, h, eps, offset, order, parents, dtype=torch.float64):
    """one prior sample per row (hsvrnn_bvh.py:210-218) -> keypoints (B,4K), z (B,Z), next state (B,H), decoder input (B,H+Z)"""
    with precision(dtype), torch.no_grad():
        sdd = cast(sd, dtype)
        h, eps = _t(h, dtype), _t(eps, dtype)
        off = _t(offset, dtype).reshape(h.shape[0], -1, 3, 1)
        pm, ps = O._dist_params(O._mlp(h, sdd, DYN + ".extract_prior_dist"))
        z = pm + eps * ps
        dec = torch.cat([h, z], -1)
        f, _ = O.fk_decode(sdd, dec, off, order, parents)
        return dict(kp=f, z=z, h=O.gru_cell(sdd, torch.cat([f, z], -1), h), dec=dec)


# ---- selections and per-step comparisons ------------------------------------------------------------------------------------
def selection_margins(d):
    """relative gap (second best - best) / best of each best-of-S selection: d (S, ...) -> (...); +inf for S = 1"""
    d = d.double()
    if d.shape[0] < 2:
        return torch.full(d.shape[1:], float("inf"), dtype=torch.float64)
    top = d.topk(2, dim=0, largest=False).values
    return (top[1] - top[0]) / top[0].clamp_min(1e-300)


def encode_margins(ref):
    """(T, B) selection margins of an encode: ref['sample_dist'] is (S, B, T)"""
    return selection_margins(ref["sample_dist"]).transpose(0, 1)


def teacher_forced(step, ref, kp, eps):
    """Re-run every posterior step of an encode from the reference's own state h_{t-1}: step(h (B,H), obs (B,K,4), eps (S,B,Z)) ->
    (keypoints (B,4K), z (B,Z), h_t (B,H)).  Returns the largest absolute deviation from `ref` (an fp64 encode) of each step."""
    B, T = kp.shape[:2]
    errs = []
    for t in range(T):
        kps, zs, hn = step(ref["h_kypts"][:, t], kp[:, t], eps[t])
        errs.append(max(_err(kps, ref["kypt_recon"][:, t].reshape(B, -1)), _err(zs, ref["z_kypts"][:, t]), _err(hn, ref["h_kypts"][:, t + 1])))
    return errs


def oracle_step(sd, ref, order, parents, dtype=torch.float32):
    """the oracle's posterior step in `dtype` as a `teacher_forced` step function (bone offsets of the fp64 encode `ref`)"""
    off = ref["offset"]

    def step(h, obs, eps):
        with precision(dtype), torch.no_grad():
            h2, bz, bf, _, _, _, _ = O._posterior_step(cast(sd, dtype), _t(h, dtype), _t(obs, dtype).reshape(h.shape[0], -1), _t(eps, dtype),
                                                      _t(off, dtype), order, parents)
        return bf, bz, h2
    return step


# ---- the seeded inputs the GPU tests use (shared with tests/test_vrnn_ref_cpu.py, which checks their selection margins) ------------
def model(K, wseed):
    """seeded weights with K keypoints and a random skeleton: (options, state dict, order, parents, affinity)"""
    o = HotPathOptions(grid_size=32, nkeypoints=K, Tcond=5)
    sd = synth.make_state_dict(o, seed=wseed, variant="default")
    gen = torch.Generator().manual_seed(1000 + K)
    sd["kypt_detector.affinity_params"] = torch.randn(sd["kypt_detector.affinity_params"].shape, generator=gen)
    aff = O.affinity_v3(sd["kypt_detector.affinity_params"])
    _, order, _, parents = O.build_tree(aff)
    return o, sd, order, parents, aff


def keypoints(B, T, K, seed):
    """coordinates in [-0.8, 0.8), intensities in [0, 1)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, T, K, 4, generator=g) * torch.tensor([1.6, 1.6, 1.6, 1.0]) - torch.tensor([0.8, 0.8, 0.8, 0.0])


# encode cases (B, S, T, K, weight seed, keypoint seed, eps seed): the posterior chain's limits (S B <= 96, S <= 16, B <= 16), six-launch
# row steps (S B < 128), GEMM steps with ragged 128-row sample tiles (S B = 130 / 160 / 240 / 260) and the AIST shape (B 16, T 20)
ENCODE_CASES = {
    "chain-9x10": (9, 10, 6, 24, 71, 1, 11),
    "chain-6x16": (6, 16, 6, 24, 71, 2, 12),
    "chain-16x6": (16, 6, 6, 24, 71, 3, 13),
    "rows-11x10": (11, 10, 6, 24, 71, 4, 14),
    "gemm-13x10": (13, 10, 6, 24, 71, 5, 15),
    "gemm-16x10": (16, 10, 6, 24, 71, 6, 16),
    "gemm-24x10": (24, 10, 6, 24, 71, 7, 17),
    "gemm-26x10": (26, 10, 6, 24, 71, 8, 18),
    "gemm-16x10-K22": (16, 10, 6, 22, 72, 9, 19),
    "aist-16x10-T20": (16, 10, 20, 24, 71, 10, 20),
}

# learner gradient cases (B, T, K, weight seed, keypoint seed, eps seed): T B > 64 samples in every weight-gradient sum
LEARNER_CASES = {
    "B16-T5-K24": (16, 5, 24, 73, 21, 35),
    "B24-T4-K24": (24, 4, 24, 73, 22, 32),
    "B16-T5-K22": (16, 5, 22, 74, 23, 33),
    "B24-T4-K22": (24, 4, 22, 74, 24, 34),
}

# generate / rollout: Tcond 5, Ttot 20 (the AIST values), best of S = 10 in the conditioning steps
GEN_B = [5, 16, 64, 65, 130]
GEN_SEEDS = (75, 41, 42, 43)           # weights, conditioning keypoints, posterior eps, prior eps (the last three offset by B + GEN_SHIFT)
GEN_SHIFT = {65: 100}                  # (B = 65 with the plain offset has a selection margin of 1.6e-5)


def encode_inputs(case):
    B, S, T, K, ws, ks, es = ENCODE_CASES[case]
    o, sd, order, parents, aff = model(K, ws)
    return o, sd, order, parents, aff, keypoints(B, T, K, ks), synth.make_eps((T, S, B, o.nlatent_kypt), seed=es)


def learner_inputs(case):
    B, T, K, ws, ks, es = LEARNER_CASES[case]
    o, sd, order, parents, aff = model(K, ws)
    return o, sd, order, parents, aff, keypoints(B, T, K, ks), synth.make_eps((T, 10, B, o.nlatent_kypt), seed=es)


def generate_inputs(B, Tcond=5, Ttot=20, K=24):
    ws, ks, ep, er = GEN_SEEDS
    o, sd, order, parents, aff = model(K, ws)
    Z, s = o.nlatent_kypt, B + GEN_SHIFT.get(B, 0)
    return (o, sd, order, parents, aff, keypoints(B, Tcond, K, ks + s), synth.make_eps((Tcond, 10, B, Z), seed=ep + s),
            synth.make_eps((Ttot - Tcond, B, Z), seed=er + s))
