"""The two graph losses of the reference's keypoint detector for every graph_loss_ver and switch, restated in fp64 torch
(utils/kypt_detector_utils.py:172-225 get_graph_consistency_loss, :228-265 get_graph_traj_loss; switches of model/kypt_detector.py:112-143).

tests/golden/g15_graph_loss_options.npz records what the reference's own functions return (values and gradients) on seeded inputs;
tests/test_graph_loss_options_cpu.py pins this restatement to it, and the GPU tests compose it with oracle.nm_oracle.detector_forward
for the terms the oracle does not vary (the oracle itself honours keypoints_detach only)."""
import torch


def influence(aff, ver):
    """max over the neighbours of affinity (N, K, K, 1) -> (K, K); ver 2: M + M^T (:182-184, :230-232)"""
    m = aff.squeeze(-1).max(dim=0).values
    if ver == 2:
        m = m + m.transpose(0, 1)
    return m


def graph_consistency(kp, aff, ver=1, local=True, time=True, sparsity=True):
    """:172-225 -> local (B,T) or zeros(1,1), time (B,T) or zeros(1,1), sparsity (1,1), intensity zeros(1,1)"""
    z = torch.zeros(1, 1, dtype=kp.dtype)
    infl = influence(aff, ver)[None, None, :, :, None]                           # (1,1,K,K,1)
    pos = kp[..., :3]
    inten = kp[..., -1][..., None, None]                                        # (B,T,K,1,1): the weight of the FIRST index (:187)
    dist = (pos[:, :, :, None] - pos[:, :, None]).pow(2).sum(dim=-1, keepdim=True)      # (B,T,K,K,1)  :189
    weighted = ver in (0, 2)
    if local:                                                                   # :192-198
        lo = dist * infl * inten if weighted else dist * infl
        lo = lo.mean(dim=(2, 3, 4))
    else:
        lo = z
    if time:                                                                    # :202-208
        dev = (dist - dist.mean(dim=1, keepdim=True)).abs()
        ti = dev * infl * inten if weighted else dev * infl
        ti = ti.mean(dim=(2, 3, 4))
    else:
        ti = z
    if sparsity:                                                                # :213-220 (every neighbour pair but n = m)
        a = aff.squeeze(-1)
        sp = (a[:, None] * a[None]).pow(2).sum(dim=1, keepdim=True) - a[:, None].pow(4)
        sp = sp.sum(dim=(0, 1)).mean(dim=(0, 1), keepdim=True)
    else:
        sp = z
    return lo, ti, sp, z.clone()                                                # intensity loss: always zeros (:223)


def graph_traj(kp, aff, ver=1):
    """:228-265 -> (1,1)"""
    infl = influence(aff, ver)[None, None]                                      # (1,1,K,K)
    weighted = ver in (0, 2)
    vel = kp[:, 1:, :, :3] - kp[:, :-1, :, :3]
    acc = vel[:, 1:] - vel[:, :-1]
    cos = torch.nn.CosineSimilarity(dim=-1, eps=1e-6)
    vc = (-cos(vel[:, :, :, None], vel[:, :, None]) + 1) / 2                   # (B,T-1,K,K)
    ac = (-cos(acc[:, :, :, None], acc[:, :, None]) + 1) / 2                   # (B,T-2,K,K)
    if weighted:                                                                # :237-243: per row k
        iv = (kp[:, 1:, :, -1:] + kp[:, :-1, :, -1:]) / 2                       # (B,T-1,K,1)
        ia = (iv[:, 1:] + iv[:, :-1]) / 2                                       # (B,T-2,K,1)
        vc = (vc * infl * iv).mean(dim=(0, 1))
        ac = (ac * infl * ia).mean(dim=(0, 1))
    else:
        vc = (vc * infl).mean(dim=(0, 1))
        ac = (ac * infl).mean(dim=(0, 1))
    return (vc + ac).mean(dim=(0, 1), keepdim=True)


GRAPH_KEYS = ("local_const_loss", "time_const_loss", "sparsity_const_loss", "intensity_const_loss", "graph_traj_loss", "graph_vol_loss")


def graph_terms(kp, aff, opts):
    """the six graph entries of KyptDetector.forward's dict (kypt_detector.py:114-143, reported means :155-165) for the options
    ``opts`` (a HotPathOptions) with the affinity started; ``aff`` None = keypoints_graph 'none' (or not started): all zeros"""
    z = torch.zeros((), dtype=kp.dtype)
    if aff is None or opts.keypoints_graph == "none":
        return {k: z for k in GRAPH_KEYS}
    kk = kp.detach() if opts.keypoints_detach else kp
    lo, ti, sp, it = graph_consistency(kk, aff, opts.graph_loss_ver, bool(opts.using_local_const), bool(opts.using_time_const),
                                       bool(opts.using_sparsity_const))
    tr = graph_traj(kk, aff, opts.graph_loss_ver) if opts.graph_traj_weight > 0 else z
    return dict(local_const_loss=lo.mean(), time_const_loss=ti.mean(), sparsity_const_loss=sp.mean(), intensity_const_loss=it.mean(),
                graph_traj_loss=tr.mean(), graph_vol_loss=z)
