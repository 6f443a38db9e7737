"""The detector with options.const_intensity = 2 (recurrent heat-maps), restated in torch on the oracle's own pieces.

The reference's VoxToKyptNet.forward (model/kypt_detector.py:308-347) propagates the heat-map of frame t from `prev_heatmap`; under
const_intensity 3 that is the clip's spatio-temporal heat-map at every frame, under 2 it is the propagated heat-map of frame t - 1
(:344-345, `prev_heatmap = heatmap`) and the spatio-temporal one at frame 0 only.  oracle.nm_oracle.vox_to_kypt is value 3; this file
restates the loop for value 2 with the oracle's feature_net / add_coords / heatmap_to_keypoints / gaussian_map and composes it with
the oracle's voxel decoder, losses, affinity, tree and VRNN, unchanged.  Works in float32 and float64 (the dtype of `sd` and `seq`).

tests/golden/g17_recurrent32.npz records what the reference computes with const_intensity = 2 (tools/make_recurrent_fixture.py);
tests/test_recurrent_heatmaps_cpu.py pins this restatement to it, and tests/test_recurrent_heatmaps_gpu.py holds the HIP path to it."""
import torch
import torch.nn.functional as F

from oracle import nm_oracle as O


def vox_to_kypt(sd, opts, seq):
    """VoxToKyptNet.forward for const_intensity == 2 -> heatmaps (B,T,K,g,g,g), keypoints (B,T,K,4), gaussians, first_feature"""
    B, T = seq.shape[:2]
    K, g = opts.nkeypoints, opts.grid_size // 4
    st = O.feature_net(O.add_coords(seq.mean(dim=1)), sd, O.V2K + ".extract_spatio_temporal_features", g)          # :311-316
    hw = O.V2K + ".extract_spatio_temporal_heatmaps_from_features.0"
    prev = F.leaky_relu(F.conv3d(st, sd[hw + ".weight"], sd[hw + ".bias"]), O.LRELU)
    pw, pb = sd[O.V2K + ".propagate_heatmaps.0.weight"], sd[O.V2K + ".propagate_heatmaps.0.bias"]
    hw = O.V2K + ".extract_heatmaps_from_features.0"
    sig = opts.gaussian_sigma if getattr(opts, "fixed_sigma", 1) else torch.sigmoid(sd[O.V2K + ".sigmas"]) * (opts.gaussian_sigma * 2.0)
    hms, kps, gss = [], [], []
    first = None
    for t in range(T):
        feat = O.feature_net(O.add_coords(seq[:, t]), sd, O.V2K + ".extract_features", g)
        if t == 0:
            first = feat
        hm = F.leaky_relu(F.conv3d(feat, sd[hw + ".weight"], sd[hw + ".bias"]), O.LRELU)
        pair = torch.cat([hm.reshape(B * K, 1, g, g, g), prev.reshape(B * K, 1, g, g, g)], dim=1)
        hm = F.softplus(F.conv3d(pair, pw, pb)).view(B, K, g, g, g)                                               # :339-343
        prev = hm                                                                                                 # :344-345
        kp = O.heatmap_to_keypoints(hm)
        hms.append(hm); kps.append(kp); gss.append(O.gaussian_map(kp, sig, g))
    return torch.stack(hms, 1), torch.stack(kps, 1), torch.stack(gss, 1), first


def detector_forward(sd, opts, seq, affinity_on=True):
    """KyptDetector.forward (kypt_detector.py:81-169) around the recurrent heat-maps: oracle.nm_oracle.detector_forward with the loop above"""
    B, T = seq.shape[:2]
    heatmaps, keypoints, gaussians, first = vox_to_kypt(sd, opts, seq)
    recon = O.kypt_to_vox(sd, opts, gaussians, first, seq[:, 0])
    recon_loss = F.binary_cross_entropy(recon, seq, reduction="none").mean(dim=(2, 3, 4, 5))
    zeros = torch.zeros(B, T)
    if opts.vol_fit_type == "chamfer":
        vol = O.loss_volume_chamfer(seq, keypoints)
    elif opts.vol_fit_type == "gaussian":
        vol = O.loss_volume_gaussian(seq, keypoints, opts.gaussian_sigma)
    else:
        vol = zeros
    if affinity_on:
        aff = O.affinity(sd["kypt_detector.affinity_params"], getattr(opts, "affinity_ver", 3))
        kk = keypoints.detach() if opts.keypoints_detach else keypoints
        local, tim, spars, inten = O.loss_graph_consistency_v1(kk, aff)
        traj = O.loss_graph_traj_v1(kk, aff) if opts.graph_traj_weight > 0 else zeros
    else:
        aff = None
        local = tim = spars = inten = traj = zeros
    return dict(
        recon=recon, keypoints=keypoints, heatmaps=heatmaps, affinity=aff,
        recon_loss=recon_loss.mean(), vol_fit_reg=vol.mean(), kypt_const_loss=zeros.mean(),
        separation_loss=O.loss_separation(keypoints, opts.sep_sigma).mean(),
        sparsity_loss=O.loss_sparsity(heatmaps).mean(),
        local_const_loss=local.mean(), time_const_loss=tim.mean(),
        sparsity_const_loss=spars.mean(), intensity_const_loss=inten.mean(),
        graph_traj_loss=traj.mean(), graph_vol_loss=zeros.mean(),
        first_feature=first, gaussians=gaussians,
    )


def nm_forward(sd, opts, vox, eps, tree=None):
    """NeuralMarionette.forward, detector + learner (neural_marionette.py:34-56), as oracle.nm_oracle.nm_forward"""
    log = detector_forward(sd, opts, vox, affinity_on=True)
    if tree is None:
        _, order, _, parents = O.build_tree(log["affinity"])
    else:
        order, parents = tree
    log.update(O.vrnn_encode(sd, opts, log["keypoints"], order, parents, eps))
    log["order"], log["parents"] = order, parents
    return log
