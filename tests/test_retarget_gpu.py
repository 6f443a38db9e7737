"""Motion retargeting on the device (nm_retarget_bind / nm_retarget_fk / nm_retarget_pose, HSVRNNBVH.skin_weights,
NeuralMarionette.sample_retarget) against the float64 restatement of tests/retarget_ref.py and the reference-written fixture G16.

Where the bounds come from
 - selections: compared wherever the RESTATEMENT's margin (second-smallest minus smallest bone distance) exceeds 1e-9 at op level -
   the exclusion is computed from the restatement, never from the library's output, and asserted to be empty; 4e-4 in the free run
   against G16 (two bone distances each move by at most sqrt(3) 1e-4 when the keypoints move by the project's 1e-4 contract, so a
   margin above 2 sqrt(3) 1e-4 = 3.5e-4 cannot flip).
 - weights at op level: one fp32 ulp (the two exp implementations may differ in the last float64 bits, which moves the fp32 rounding by
   at most one step); teacher-forced against G16: 7e-4 (w = 1 / (1 + exp(H (d_c - d_p))) has slope <= H / 4 = 2 in d_c - d_p, which
   moves by at most 2 sqrt(3) 1e-4).
 - local coordinates 1e-12, posed points at op level 1e-6 against the DENSE einsum form (one fp32 ulp of a weight, 6e-8, times
   |kin_child - kin_parent| <= ~8); the measured error is printed.
 - points against G16: the fixture's points_sens (the 1e-4 contract carried through the driver, measured on the reference side by the
   fixture tool), no further margin."""
import os

import numpy as np
import pytest
import torch

import golden_npz
import retarget_ref as RR
import vrnn_ref as V
from neural_marionette_amd import NeuralMarionette, HotPathOptions, _lib, synth
from neural_marionette_amd.modules import HSVRNNBVH

pytestmark = pytest.mark.gpu

KP_TOL = 1e-4
MARGIN_OP, MARGIN_FREE, W_TOL_FORCED = 1e-9, 4e-4, 7e-4
_DYN = {}


def _dyn(K, parents, order):
    """a stand-alone learner with K keypoints on the GPU (one per K for the module), given the tree of the case"""
    if K not in _DYN:
        torch.manual_seed(K)
        _DYN[K] = HSVRNNBVH(HotPathOptions(grid_size=32, nkeypoints=K)).cuda().eval()
    d = _DYN[K]
    d.set_tree(parents, order)
    return d


def _np(t):
    return t.detach().cpu().numpy()


def _bind(d, s, kp=None, **kw):
    kp = s["keypoints"] if kp is None else kp
    with torch.no_grad():
        out = d.skin_weights(torch.from_numpy(s["points"]), torch.from_numpy(kp), torch.from_numpy(s["R_bind"]), **kw)
    torch.cuda.synchronize()
    return out


def _ulp_steps(a, b):
    """distance of two fp32 arrays in units of the larger value's spacing"""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def _check_bind(out, ref, K, every_selection=False):
    child, parent, w, local, margin, dense = (_np(out[k]) for k in ("child", "parent", "w", "local", "margin", "dense"))
    clear = np.ones_like(ref["margin"], bool) if every_selection else ref["margin"] > MARGIN_OP
    assert (~clear).sum() == 0, f"{(~clear).sum()} selections of the restatement have a margin below {MARGIN_OP}"
    assert np.array_equal(child[clear], ref["child"][clear])
    assert np.array_equal(parent[clear], ref["parent"][clear])
    steps = _ulp_steps(w, ref["w"])
    e_local = np.abs(local - ref["local"]).max()
    e_margin = np.abs(margin - ref["margin"]).max()
    print("bind N=%d K=%d: weights differ in %d of %d entries (max %.1f ulp), local %.2e, margin %.2e" % (
        child.shape[0], K, int((steps > 0).sum()), steps.size, steps.max(), e_local, e_margin))
    assert steps.max() <= 1.0
    assert e_local < 1e-12 and e_margin < 1e-12
    # the dense matrix is the record scattered: parent first, child second (what remains when parent == child)
    n = np.arange(child.shape[0])
    want = np.zeros_like(dense)
    want[n, parent] = w[:, 1]
    want[n, child] = w[:, 0]
    assert np.array_equal(want.view(np.uint32), dense.view(np.uint32))
    assert (w[parent == child, 1] == 0).all()
    assert _ulp_steps(dense, ref["dense"]).max() <= 1.0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bind_standin(seed):
    s = RR.standin(seed)
    d = _dyn(24, s["parents"], s["order"])
    ref = RR.bind(s["parents"], s["root"], s["points"], s["keypoints"], s["R_bind"])
    _check_bind(_bind(d, s), ref, 24)


@pytest.mark.parametrize("K,N", [(5, 1), (5, 777), (32, 1), (32, 20001)])
def test_bind_other_shapes(K, N):
    s = RR.standin(10 + K, N=max(N, 2000), K=K)
    s["points"] = np.ascontiguousarray(s["points"][:N])
    d = _dyn(K, s["parents"], s["order"])
    ref = RR.bind(s["parents"], s["root"], s["points"], s["keypoints"], s["R_bind"])
    _check_bind(_bind(d, s), ref, K)
    # without R_bind the local coordinates are plain offsets
    with torch.no_grad():
        out = d.skin_weights(torch.from_numpy(s["points"]), torch.from_numpy(s["keypoints"]))
    ref0 = RR.bind(s["parents"], s["root"], s["points"], s["keypoints"], None)
    assert np.abs(_np(out["local"]) - ref0["local"]).max() < 1e-12


def _deep_joint(parents, order, root):
    """a joint whose parent and grandparent are both not the root"""
    for k in order[::-1]:
        p = int(parents[k]); g = int(parents[p])
        if p != root and g != root and k != root:
            return int(k), p, g
    raise AssertionError("the tree has no chain of depth 3")


def test_bind_ancestor_walks():
    s = RR.standin(2, N=5000)
    root = s["root"]
    d = _dyn(24, s["parents"], s["order"])
    # a chain of two invalid ancestors under a valid joint
    k, p, g = _deep_joint(s["parents"], s["order"], root)
    kp = s["keypoints"].copy()
    kp[:, 3] = 0.9
    kp[[p, g], 3] = 0.05
    bones, _ = RR.bone_points(s["parents"], kp)
    gg = int(s["parents"][g])
    assert np.array_equal(bones[k], (kp[k, :3] + kp[gg, :3]) / np.float32(2))
    ref = RR.bind(s["parents"], root, s["points"], kp, s["R_bind"])
    assert (ref["child"] == k).any(), "the case must select the joint whose bone skips two ancestors"
    _check_bind(_bind(d, s, kp), ref, 24)
    # an INVALID root (no reference behaviour: the walk stops there, by the library's and the restatement's documented choice)
    kp = s["keypoints"].copy()
    kp[root, 3] = 0.05
    ref = RR.bind(s["parents"], root, s["points"], kp, s["R_bind"])
    _check_bind(_bind(d, s, kp), ref, 24)
    # every non-root joint invalid: every distance is the VALUE 1e4 and the first index wins (margins are all 0 by construction, the
    # selection is still determined: compared everywhere)
    kp = s["keypoints"].copy()
    kp[:, 3] = 0.05
    kp[root, 3] = 0.9
    ref = RR.bind(s["parents"], root, s["points"], kp, s["R_bind"])
    assert (ref["child"] == 0).all() and (ref["margin"] == 0).all()
    _check_bind(_bind(d, s, kp), ref, 24, every_selection=True)
    # the same with joint 0 as the root: parent == child, the dense row holds the child's weight alone
    parents = np.array([0, 0, 1, 2, 2], np.int32)
    order = np.arange(5, dtype=np.int32)
    s5 = RR.standin(7, N=1000, K=5)
    d5 = _dyn(5, parents, order)
    kp = s5["keypoints"].copy()
    kp[:, 3] = 0.05
    for root_intensity in (0.9, 0.05):
        kp[0, 3] = root_intensity
        ref = RR.bind(parents, 0, s5["points"], kp, s5["R_bind"])
        assert (ref["child"] == 0).all() and (ref["parent"] == 0).all()
        out = _bind(d5, s5, kp)
        _check_bind(out, ref, 5, every_selection=True)
        dense = _np(out["dense"])
        assert (dense[:, 1:] == 0).all() and (dense[:, 0] == np.float32(0.5)).all()


def test_bind_forced_selection():
    s = RR.standin(3, N=4000)
    d = _dyn(24, s["parents"], s["order"])
    force = np.random.default_rng(0).integers(0, 24, 4000).astype(np.int32)
    ref = RR.bind(s["parents"], s["root"], s["points"], s["keypoints"], s["R_bind"], force_child=force)
    out = _bind(d, s, force_child=torch.from_numpy(force))
    assert np.array_equal(_np(out["child"]), force)
    _check_bind(out, ref, 24)
    with pytest.raises(ValueError):
        _bind(d, s, force_child=torch.from_numpy(force + 24))
    with pytest.raises(ValueError):
        _bind(d, s, force_child=torch.from_numpy(force[:-1]))


def test_fk_with_clip():
    s = RR.standin(1, N=2000, T=40)
    d = _dyn(24, s["parents"], s["order"])
    root_pos = (s["root_pos"] * 3).astype(np.float32)            # the walk leaves [-1, 1]
    ref = RR.fk(s["R"], root_pos, s["offset"], s["order"], s["parents"])
    assert (np.abs(ref) == 1).any() and (np.abs(ref) < 1).any() and np.abs(root_pos).max() > 1
    with torch.no_grad():
        pos = d.retarget_fk(torch.from_numpy(s["R"]).cuda(), torch.from_numpy(root_pos).cuda(), torch.from_numpy(s["offset"]).cuda())
    e = np.abs(_np(pos) - ref).max()
    print("fk T=40: %.2e" % e)
    assert e < 1e-6


@pytest.mark.parametrize("T,N", [(1, 20000), (8, 20000), (40, 20000), (1, 250007), (8, 250007), (40, 250007), (3, 1), (9, 255)])
def test_pose_against_dense_form(T, N):
    s = RR.standin(1 + T % 3, N=max(N, 2000), T=T)
    s["points"] = np.ascontiguousarray(s["points"][:N])
    d = _dyn(24, s["parents"], s["order"])
    ref = RR.bind(s["parents"], s["root"], s["points"], s["keypoints"], s["R_bind"])
    assert (ref["margin"] <= MARGIN_OP).sum() == 0
    pos = RR.fk(s["R"], s["root_pos"], s["offset"], s["order"], s["parents"], np.float32)
    want = RR.pose_dense(ref["dense"], s["points"], s["keypoints"], s["R_bind"], s["R"], pos)
    out = _bind(d, s)
    with torch.no_grad():
        got = d.retarget_pose(out, torch.from_numpy(s["R"]).cuda(), torch.from_numpy(pos).cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (T, N, 3)
    e = np.abs(_np(got) - want).max()
    same = np.array_equal(_np(out["w"]).view(np.uint32), ref["w"].view(np.uint32))
    print("pose T=%d N=%d: %.2e against the dense form (weights bit-equal: %s)" % (T, N, e, same))
    assert e < 1e-6


def test_encode_and_offsets_on_one_frame():
    """the target side of the driver calls encode and get_offset on a ONE-frame clip (best-of-10 at T = 1, median over T = 1)"""
    o, sd, order, parents, aff = V.model(24, 71)
    net = NeuralMarionette(o)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    net.anneal(1)
    for ks, es in ((51, 61), (52, 62)):
        kp = V.keypoints(1, 1, 24, ks)
        eps = synth.make_eps((1, 10, 1, o.nlatent_kypt), es)
        ref = V.encode(sd, o, kp, order, parents, eps)
        assert float(V.encode_margins(ref).min()) > V.MARGIN_MIN
        with torch.no_grad():
            out = net.dyna_module.encode(kp.cuda(), aff.cuda(), eps=eps.cuda())
            off = net.dyna_module.get_offset(kp.cuda())
        assert np.array_equal(_np(net.dyna_module.parents), parents)
        assert torch.equal(out["best_idx"].cpu().long(), ref["best_idx"].long().reshape(1, 1))
        errs = {k: V._err(out[k], ref[k]) for k in ("kypt_recon", "R", "z_kypts", "h_kypts")}
        e_off = V._err(off, V.offsets(sd, kp, parents))
        print("T = 1 encode:", " ".join("%s %.2e" % kv for kv in errs.items()), "offset %.2e" % e_off)
        assert max(errs.values()) < KP_TOL and e_off < 1e-6


def _g16_net(golden_dir):
    g = golden_npz.load(os.path.join(golden_dir, "g16_retarget32.npz"))
    seeds = dict(zip(("G", "T", "N", "weights", "source", "target", "pick", "eps_source", "eps_target"), g["meta"].tolist()))
    o, sd, source, target, points, eps_s, eps_t = RR.g16_inputs(seeds)
    net = NeuralMarionette(o)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    net.anneal(1)
    args = (source.cuda(), target.cuda(), torch.from_numpy(points))
    kw = dict(hardness=float(g["hardness"]), threshold=float(g["threshold"]), eps_source=eps_s.cuda(), eps_target=eps_t.cuda())
    return g, net, args, kw


def test_g16_end_to_end(golden_dir):
    g, net, args, kw = _g16_net(golden_dir)
    out = net.sample_retarget(*args, **kw)
    torch.cuda.synchronize()
    # the same tree: parents and root equal; the kinematic order may differ among joints of equal depth (the shells resolve the
    # reference's topk ties by index), which no result depends on
    assert np.array_equal(_np(net.dyna_module.parents), g["parents"])
    order = _np(net.dyna_module.priority.indices)
    assert int(order[0]) == int(g["order"][0]) and sorted(order.tolist()) == sorted(g["order"].tolist())
    errs = {k: V._err(out[k], g[k]) for k in ("source_keypoints", "target_keypoints", "R", "R_bind", "offset", "keypoints")}
    print("G16 free run:", " ".join("%s %.2e" % kv for kv in errs.items()))
    for k in ("source_keypoints", "target_keypoints", "R", "R_bind", "offset", "keypoints"):
        assert errs[k] < KP_TOL, (k, errs[k])
    clear = g["margin"] > MARGIN_FREE
    assert (~clear).mean() <= 0.02
    nearest = _np(out["nearest"])
    flips = int((nearest != g["nearest"]).sum())
    print("G16 free run: %d of %d selections differ, %d of them with a reference margin above %.0e; points %.2e" % (
        flips, nearest.size, int((nearest != g["nearest"])[clear].sum()), MARGIN_FREE, V._err(out["points"], g["points"])))
    assert np.array_equal(nearest[clear], g["nearest"][clear])
    forced = net.sample_retarget(*args, force_nearest=torch.from_numpy(g["nearest"]), **kw)
    torch.cuda.synchronize()
    assert np.array_equal(_np(forced["nearest"]), g["nearest"])
    e_w = V._err(forced["skin_weights"], g["dense"])
    e_p = V._err(forced["points"], g["points"])
    print("G16 teacher-forced: weights %.2e (bound %.0e), points %.2e (points_sens %.3e), margins %.2e" % (
        e_w, W_TOL_FORCED, e_p, float(g["points_sens"]), V._err(forced["nearest_margin"], g["margin"])))
    assert tuple(forced["points"].shape) == g["points"].shape and forced["points"].dtype == torch.float64
    assert e_w < W_TOL_FORCED
    assert e_p < float(g["points_sens"])


def test_two_calls_are_bit_identical(golden_dir):
    g, net, args, kw = _g16_net(golden_dir)
    a = net.sample_retarget(*args, **kw)
    b = net.sample_retarget(*args, **kw)
    for k in ("source_keypoints", "target_keypoints", "R", "R_bind", "offset", "keypoints", "skin_weights", "nearest", "nearest_margin", "points"):
        assert torch.equal(a[k], b[k]), k
    s = RR.standin(2, N=100003, T=40)
    d = _dyn(24, s["parents"], s["order"])
    pos = torch.from_numpy(RR.fk(s["R"], s["root_pos"], s["offset"], s["order"], s["parents"], np.float32)).cuda()
    R = torch.from_numpy(s["R"]).cuda()
    runs = []
    for _ in range(2):
        rec = _bind(d, s)
        with torch.no_grad():
            runs.append((rec, d.retarget_pose(rec, R, pos)))
    for k in ("child", "parent", "w", "local", "margin", "dense"):
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    assert torch.equal(runs[0][1], runs[1][1])


def test_errors():
    o = HotPathOptions(grid_size=32)
    fresh = HSVRNNBVH(o).cuda().eval()
    pts, kp = torch.zeros(10, 3, dtype=torch.float64), torch.zeros(24, 4)
    with pytest.raises(_lib.NmError, match="skeleton has not been built"):
        fresh.skin_weights(pts, kp)
    with pytest.raises(_lib.NmError, match="nm_vrnn_set_tree has not been called"):      # the library's own check, below the shell's
        fresh._eng().call("nm_retarget_fk", None, None, None, 1, 24, None)
    s = RR.standin(1, N=2000)
    d = _dyn(24, s["parents"], s["order"])
    for bad in ((torch.zeros(10, 2), kp), (torch.zeros(0, 3), kp), (pts, torch.zeros(23, 4))):
        with pytest.raises(ValueError):
            d.skin_weights(*bad)
    with pytest.raises(ValueError):
        d.skin_weights(pts, kp, torch.zeros(24, 3, 2))
    with pytest.raises(ValueError):
        d.retarget_fk(torch.zeros(4, 24, 3, 3), torch.zeros(3, 3), torch.zeros(24, 3))
    eng = d._eng()
    buf = torch.zeros(4096, device="cuda", dtype=torch.float64)
    with pytest.raises(_lib.NmError, match="K = 23"):
        eng.call("nm_retarget_fk", _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 1, 23, _lib.ptr(buf))
    with pytest.raises(_lib.NmError, match="T = 0"):
        eng.call("nm_retarget_fk", _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 0, 24, _lib.ptr(buf))
    with pytest.raises(_lib.NmError, match="N = 0"):
        eng.call("nm_retarget_bind", _lib.ptr(buf), 0, _lib.ptr(buf), None, 24, 8.0, 0.2, None, _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf),
                 _lib.ptr(buf), None, None)
    with pytest.raises(_lib.NmError, match="N = 0"):
        eng.call("nm_retarget_pose", _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 1, 0, 24, _lib.ptr(buf))
    net = NeuralMarionette(o).cuda().eval()
    vox = torch.zeros(2, 1, 32, 32, 32)
    with pytest.raises(ValueError, match="target_voxel"):
        net.sample_retarget(vox, torch.zeros(1, 16, 16, 16), pts)
    with pytest.raises(ValueError, match="eps_target"):
        net.sample_retarget(vox, vox[0], pts, eps_target=torch.zeros(2, 10, 1, 128))
    with pytest.raises(ValueError, match="force_nearest"):
        net.sample_retarget(vox, vox[0], pts, force_nearest=torch.zeros(9, dtype=torch.int32))
