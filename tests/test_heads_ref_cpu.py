"""The reference of tests/test_heads_ops_gpu.py without a GPU.

1. tests/heads_ref.py is glue around the oracle's functions; here the glue is pinned against oracle.nm_oracle.detector_forward: one small
   seeded run's head outputs, first-frame feature and decoder input are fed through the pieces, which must give that run's heat-maps,
   keypoints, combined representation, reconstruction and eleven losses again, in float64 to 1e-12 (and the recurrent form against
   tests/recurrent_heatmap_ref.py, which fixture G17 ties to the reference).
2. The discontinuous choices (chamfer arg-min, max over the neighbours, arg-max intensity, |.| of the time term, the first maximal map
   of vol_fit 'gaussian') are decided by a clear margin on the inputs the GPU cases use: the float32 and the float64 reference pick
   identically everywhere, so no GPU case needs to mask anything out.  sign(mean) of the sparsity adjoint has one value on these
   inputs: a heat-map is a softplus, its mean is positive."""
import pytest
import torch
import torch.nn.functional as F

import heads_ref as R
import recurrent_heatmap_ref as RR
from oracle import nm_oracle as O
from neural_marionette_amd import HotPathOptions, synth
from neural_marionette_amd.spec import DETECTOR_LOSS_KEYS


def _close(a, r, what, tol=1e-12):
    assert a.shape == r.shape, (what, a.shape, r.shape)
    e = (a - r).abs().max().item()
    assert e <= tol * max(r.abs().max().item(), 1e-300), f"{what}: {e:.3e} of {r.abs().max().item():.3e}"


@pytest.fixture(scope="module")
def run():
    o = HotPathOptions(grid_size=32)
    sd = {k: v.double() for k, v in synth.make_state_dict(o, seed=11, variant="peaky").items()}
    vox = synth.figure_clip(1, 3, 32, seed=13).double()
    taps = {}
    with torch.no_grad():
        out = O.detector_forward(sd, o, vox, affinity_on=True, taps=taps)
        g = o.grid_size // 4
        hw = O.V2K + ".extract_heatmaps_from_features.0"
        head = torch.stack([F.conv3d(O.feature_net(O.add_coords(vox[:, t]), sd, O.V2K + ".extract_features", g), sd[hw + ".weight"], sd[hw + ".bias"])
                            for t in range(vox.shape[1])], 1)
        cw = O.V2K + ".extract_spatio_temporal_heatmaps_from_features.0"
        st = O.feature_net(O.add_coords(vox.mean(dim=1)), sd, O.V2K + ".extract_spatio_temporal_features", g)
        clip = F.conv3d(st, sd[cw + ".weight"], sd[cw + ".bias"])
    prop = torch.cat([sd[O.V2K + ".propagate_heatmaps.0.weight"].flatten(), sd[O.V2K + ".propagate_heatmaps.0.bias"].flatten()])
    return dict(o=o, sd=sd, vox=vox, out=out, taps=taps, head=head, clip=clip, prop=prop)


def test_glue_rederives_the_oracle_run(run):
    o, sd, vox, out, taps = run["o"], run["sd"], run["vox"], run["out"], run["taps"]
    g, G = o.grid_size // 4, o.grid_size
    with torch.no_grad():
        hm = R.heatmaps(run["head"], run["clip"], run["prop"], False)
        _close(hm, out["heatmaps"], "heat-maps")
        kp = R.keypoints_of(hm)
        _close(kp, out["keypoints"], "keypoints")
        comb, ga = R.combined(kp, out["first_feature"], o.gaussian_sigma, g, 0)
        _close(ga, out["gaussians"], "gaussian maps")
        aw = O.K2V + ".adjust_combined_representation.0"
        _close(F.leaky_relu(F.conv3d(comb[:, 0], sd[aw + ".weight"], sd[aw + ".bias"]), O.LRELU), taps["dec_adjust"], "combined representation")
        w14, b14 = sd[O.DEC + ".14.weight"], sd[O.DEC + ".14.bias"]
        _close(R.tail(taps["dec_64"][:, None], w14.flatten(), b14, vox[:, 0]), out["recon"][:, :1], "reconstruction of frame 0")
        bce = F.binary_cross_entropy(out["recon"], vox, reduction="none").sum(dim=(2, 3, 4, 5))
        c = O.coord_channels(vox.shape[3:])
        d = (c[None, None, None] - kp[..., :3][..., None, None, None]).pow(2).sum(dim=3).min(dim=2, keepdim=True).values
        sums = torch.stack([bce, (d * vox).sum(dim=(2, 3, 4, 5)), vox.sum(dim=(2, 3, 4, 5))], -1)
        got = R.losses11(kp, out["affinity"], hm.mean(dim=(3, 4, 5)), sums, G, o.sep_sigma, 1, 0, o.graph_traj_weight > 0)
    assert o.vol_fit_type == "chamfer" and o.graph_traj_weight > 0
    ref = torch.stack([out[k].double().reshape(()) for k in DETECTOR_LOSS_KEYS])
    for i, k in enumerate(DETECTOR_LOSS_KEYS):
        assert abs(got[i].item() - ref[i].item()) <= 1e-12 * max(abs(ref[i].item()), 1e-300), (k, got[i].item(), ref[i].item())
    assert (ref[[0, 1, 3, 4, 5, 6, 7, 9]] != 0).all()


def test_recurrent_glue_matches_the_restated_loop(run):
    o2 = HotPathOptions(grid_size=32, const_intensity=2)
    with torch.no_grad():
        hm2, kp2, _, _ = RR.vox_to_kypt(run["sd"], o2, run["vox"])
        hm = R.heatmaps(run["head"], run["clip"], run["prop"], True)
    _close(hm, hm2, "recurrent heat-maps")
    _close(R.keypoints_of(hm), kp2, "recurrent keypoints")
    assert (hm2[:, 1:] - run["out"]["heatmaps"][:, 1:]).abs().max() > 1e-3          # (the two forms differ from frame 1 on)


@pytest.mark.parametrize("case", R.HEAT_CASES, ids=str)
def test_heat_selection_margins(case):
    inp = R.heat_inputs(*case)
    with torch.no_grad():
        m32 = R.heatmaps(inp["head"], inp["clip_head"], inp["prop"], inp["recurrent"]).mean(dim=(3, 4, 5))
        m64 = R.heatmaps(inp["head"].double(), inp["clip_head"].double(), inp["prop"].double(), inp["recurrent"]).mean(dim=(3, 4, 5))
    assert torch.equal(m32.argmax(-1), m64.argmax(-1))
    assert R.top2_gap(m64, -1).min().item() > 1e-2
    assert (m64 > 0).all() and (m32 > 0).all()                 # sign(mean)


@pytest.mark.parametrize("case", R.TAIL_CASES, ids=str)
def test_chamfer_argmin_margins(case):
    inp = R.tail_inputs(*case[:8])
    c = O.coord_channels(inp["target"].shape[3:])
    occ = inp["target"][:, :, 0] != 0
    picks = []
    for dt in (torch.float32, torch.float64):
        kp = inp["kp"].to(dt)
        d = (c[None, None, None] - kp[..., :3][..., None, None, None]).pow(2).sum(dim=3).permute(0, 1, 3, 4, 5, 2)[occ]      # (occupied, K)
        picks.append(d.argmin(-1))
    assert torch.equal(picks[0], picks[1])
    assert R.top2_gap(d, -1, largest=False).min().item() > 1e-4
    assert (inp["kp"][..., :3].abs() > 1).any()
    assert (occ.sum(dim=(2, 3, 4)) > 0).all() and (not case[6] or (occ.sum(dim=(2, 3, 4)) == 1).all())


@pytest.mark.parametrize("case", R.CLIP_CASES, ids=str)
def test_clip_selection_margins(case):
    inp = R.clip_case_inputs(case)
    s32, s64 = R.clip_selection_margins(inp, torch.float32), R.clip_selection_margins(inp, torch.float64)
    assert torch.equal(s32["sign"], s64["sign"])
    r = s64["abs_arg_rel"].abs()
    assert (r[r > 0] > 1e-4).all()
    assert torch.equal(s32["abs_arg_rel"] == 0, r == 0)          # exact zeros (a keypoint with itself, coincident keypoints) are zeros in both
    K, N = case[0], case[1]
    if inp["aff"] is not None:
        assert torch.equal(s32["argmax_n"], s64["argmax_n"])
        if N > 1:
            offd = ~torch.eye(K, dtype=torch.bool)
            assert R.top2_gap(inp["aff"].double().squeeze(-1).permute(1, 2, 0)[offd], -1).min().item() > 1e-4
    kp = inp["kp"]
    assert (kp[..., 3] == 0).any() and (kp[..., 3] == 1).any()
    dg = case[8]
    if dg in ("still", "all"):
        assert torch.equal(kp[:, 1, 0, :3], kp[:, 0, 0, :3])
    if dg in ("steady", "all"):
        p = kp[:, :3, K - 1, :3]
        assert torch.equal((p[:, 2] - p[:, 1]) - (p[:, 1] - p[:, 0]), torch.zeros_like(p[:, 0])) and ((p[:, 1] - p[:, 0]).abs().sum(-1) > 0).all()
    if dg in ("same", "all") and K > 2:
        assert torch.equal(kp[:, :, 1, :3], kp[:, :, 0, :3])


@pytest.mark.parametrize("case", R.AFF_CASES, ids=str)
def test_affinity_selection_margins(case):
    ver, K, N, B, gv, fl, seed = case
    inp = R.affinity_inputs(ver, K, N, B, seed)
    a32, a64 = O.affinity(inp["params"], ver).squeeze(-1), O.affinity(inp["params"].double(), ver).squeeze(-1)
    assert torch.equal(a32.max(dim=0).indices, a64.max(dim=0).indices)
    if N > 1:
        offd = ~torch.eye(K, dtype=torch.bool)
        assert R.top2_gap(a64.permute(1, 2, 0)[offd], -1).min().item() > 1e-4
    if K > 2:
        assert inp["params"].max() > 27 and inp["params"].min() < -27


@pytest.mark.parametrize("case", R.VOLFIT_CASES, ids=str)
def test_volfit_selection_margins(case):
    inp = R.volfit_inputs(*case)
    a, b = R.ref_volfit(inp, torch.float32, R.VOLFIT_SIGMA), R.ref_volfit(inp, torch.float64, R.VOLFIT_SIGMA)
    assert torch.equal(a["argmax"], b["argmax"])
    assert R.top2_gap(b["maps"], 2).min().item() > 1e-5
