"""Body models on the device (nm_body_shape / nm_body_pose / nm_body_joints through NeuralMarionette.pose_bodies and ClipBank.add_body)
against the float64 numpy restatement tests/body_ref.py, which tests/test_body_model_cpu.py pins to hand-worked numbers, an independent
einsum implementation and its own mutations.

What is compared how.
  rotations    (from poses) against body_ref.rodrigues on the host.  This is the one stage with sin, cos and a square root, whose last
               bits are the math library's.  Largest absolute deviation seen on an MI355X over every case of this file: ROT_SEEN = 2^-52 = 2.220e-16;
               asserted: ROT_BOUND = 2^-50, four times that, rounded up to a power of two (the device's and the host's sin / cos / sqrt may
               differ by an ulp or two each).  Independently of the measurement every deviation must stay below 1e-14: the entries are
               at most 1 in magnitude and a handful of roundings cannot exceed that, a larger deviation is a bug and not libm.  A zero
               vector gives exactly the identity.
  everything   v_shaped, J_rest, vertices, posed_joints and joints bit for bit at every entry, nothing left out: the restatement is fed
  downstream   the DEVICE'S OWN rotations, so nothing there depends on the math library.  The same through the `rotations=` input, with
               float32 poses, with betas=None, with transl=None and with scaling=0.5.

Shapes: the smallest that reach every branch of csrc/nm_body.hip.  (V=1, J=1, S=0, T=1): no pose blend shapes, no shape blend shapes, a
one-entry regressor.  (V=37, J=5 as a pure chain, S=3, T=5): one workgroup, fewer frames than NM_BODY_FRAMES = 8.  (V=129 = a workgroup's
128 vertices plus 1, J=24 with SMPL_PARENTS, S=10) at T = 7, 8, 9 and 19: below, at and above the frames per table read, and a
non-multiple with three groups.  One case at SMPL's size, V=6890, J=24, S=10, T=3.

Without the feature (the parent commit) this module fails at import: there is no tests/body_ref.py, no neural_marionette_amd.body, the
library has no nm_body_pose and NeuralMarionette no pose_bodies."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_ref as B
from neural_marionette_amd import NeuralMarionette, HotPathOptions, BodyModel, synth, _lib
from neural_marionette_amd.data import ClipBank

pytestmark = pytest.mark.gpu

ROT_SEEN = 2.0 ** -52               # 2.220e-16, measured on an MI355X over every case of this file
ROT_BOUND = 2.0 ** -50              # 8.882e-16: four times that (already a power of two)
_NET, _CASES = [], {}
SEEN = dict(rot=0.0)

CHAIN5 = (-1, 0, 1, 2, 3)
SHAPES = {"one": (1, 1, 0, 1, None), "chain": (37, 5, 3, 5, CHAIN5), "wg7": (129, 24, 10, 7, BodyModel.SMPL_PARENTS),
          "wg8": (129, 24, 10, 8, BodyModel.SMPL_PARENTS), "wg9": (129, 24, 10, 9, BodyModel.SMPL_PARENTS),
          "wg19": (129, 24, 10, 19, BodyModel.SMPL_PARENTS), "smpl": (6890, 24, 10, 3, BodyModel.SMPL_PARENTS)}


def _net():
    if not _NET:
        o = HotPathOptions(grid_size=32)
        net = NeuralMarionette(o)
        net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
        _NET.append(net.cuda().eval())
    return _NET[0]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(x, dt=np.float64):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()


def _case(name):
    """model (device), its host arrays, and seeded inputs of one shape - built once, shared, never changed"""
    if name not in _CASES:
        V, J, S, T, parents = SHAPES[name]
        model = BodyModel.synthetic(V, J, S, seed=100 + V + T, parents=parents, device="cuda")
        rng = np.random.default_rng(V * 31 + T)
        poses = rng.standard_normal((T, J, 3)) * 0.7
        poses[0, 0] = 0.0                                           # a zero vector in a posed frame ...
        if T > 1:
            poses[T - 1] = 0.0                                      # ... and a frame at rest
        _CASES[name] = dict(model=model, m=model.numpy(), poses=poses, betas=rng.standard_normal(S) if S else None,
                            transl=rng.standard_normal((T, 3)))
    return _CASES[name]


def _check(what, case, out, rot_from=None, betas=True, transl=True, scaling=1.0):
    """every output of one call against the restatement, fed the device's own rotations; rot_from: the poses the rotations came from"""
    got = {k: _np(v) for k, v in out.items()}
    if rot_from is not None:
        want = B.rodrigues(rot_from)
        dev = float(np.abs(got["rotations"] - want).max())
        SEEN["rot"] = max(SEEN["rot"], dev)
        print(f"{what}: rotations deviate from the host's by at most {dev:.3e} (seen so far {SEEN['rot']:.3e})")
        assert dev < 1e-14, f"{what}: rotations are {dev:.3e} from the restatement's: a bug, not libm"
        assert dev <= ROT_BOUND, f"{what}: rotations are {dev:.3e} from the restatement's, the bound from the measurement is {ROT_BOUND:.3e}"
        zero = (np.asarray(rot_from) == 0).all(axis=-1)
        assert zero.any() and np.array_equal(got["rotations"][zero], np.broadcast_to(np.eye(3), got["rotations"][zero].shape)), \
            f"{what}: a zero vector does not give exactly I"
    ref = B.forward(case["m"], got["rotations"], betas=case["betas"] if betas else None, transl=case["transl"] if transl else None, scaling=scaling)
    for k in ("v_shaped", "J_rest", "vertices", "posed_joints", "joints"):
        assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape, (what, k, got[k].shape, got[k].dtype)
        same = got[k] == ref[k]
        assert same.all(), f"{what}: {k} differs from the restatement at {int((~same).sum())} of {same.size} entries, first {np.argwhere(~same)[0].tolist()}: " \
                           f"{got[k][~same][0]!r} for {ref[k][~same][0]!r}"
    return got


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_output_against_the_restatement(name):
    c = _case(name)
    out = _net().pose_bodies(c["model"], poses=_dev(c["poses"]), betas=None if c["betas"] is None else _dev(c["betas"]), transl=_dev(c["transl"]))
    V, J, S, T, _ = SHAPES[name]
    assert tuple(out["vertices"].shape) == (T, V, 3) and tuple(out["rotations"].shape) == (T, J, 3, 3)
    _check(name, c, out, rot_from=c["poses"])


def test_rotations_input():
    c = _case("wg9")
    rot = B.rodrigues(c["poses"] * 1.3)
    given = _dev(rot)
    out = _net().pose_bodies(c["model"], rotations=given, betas=_dev(c["betas"]), transl=_dev(c["transl"]))
    assert out["rotations"] is given
    _check("rotations=", c, out)


def test_float32_poses_betas_and_transl():
    c = _case("wg9")
    p32 = c["poses"].astype(np.float32)
    c32 = dict(c, betas=c["betas"].astype(np.float32).astype(np.float64), transl=c["transl"].astype(np.float32).astype(np.float64))
    out = _net().pose_bodies(c["model"], poses=_dev(p32, np.float32), betas=_dev(c32["betas"], np.float32), transl=_dev(c32["transl"], np.float32))
    _check("float32 inputs", c32, out, rot_from=p32)


@pytest.mark.parametrize("betas,transl,scaling", [(False, True, 1.0), (True, False, 1.0), (False, False, 1.0), (True, True, 0.5), (True, True, -3.0)])
def test_optional_inputs_and_scaling(betas, transl, scaling):
    c = _case("chain")
    out = _net().pose_bodies(c["model"], poses=_dev(c["poses"]), betas=_dev(c["betas"]) if betas else None, transl=_dev(c["transl"]) if transl else None,
                             scaling=scaling)
    _check(f"betas {betas} transl {transl} scaling {scaling}", c, out, rot_from=c["poses"], betas=betas, transl=transl, scaling=scaling)


def test_float32_results_are_rounded_copies_and_joints_are_optional():
    c = _case("wg7")
    args = dict(poses=_dev(c["poses"]), betas=_dev(c["betas"]), transl=_dev(c["transl"]))
    a, b = _net().pose_bodies(c["model"], **args), _net().pose_bodies(c["model"], dtype=torch.float32, **args)
    for k in ("vertices", "posed_joints", "joints"):
        assert b[k].dtype == torch.float32 and torch.equal(b[k], a[k].to(torch.float32)), k
    assert b["rotations"].dtype == torch.float64 and b["v_shaped"].dtype == torch.float64
    assert "joints" not in _net().pose_bodies(c["model"], return_joints=False, **args)


def test_shape_is_cached_per_betas_tensor():
    c = _case("chain")
    model, net = c["model"], _net()
    betas, poses = _dev(c["betas"]), _dev(c["poses"])
    a, b = net.pose_bodies(model, poses=poses, betas=betas), net.pose_bodies(model, poses=poses, betas=betas)
    assert a["v_shaped"] is b["v_shaped"] and a["J_rest"] is b["J_rest"]
    betas.mul_(2.0)                                                # the same tensor, another version
    d = net.pose_bodies(model, poses=poses, betas=betas)
    assert d["v_shaped"] is not a["v_shaped"]
    assert np.array_equal(_np(d["v_shaped"]), B.shape(c["m"], 2.0 * c["betas"])[0])
    e = net.pose_bodies(model, poses=poses)
    assert np.array_equal(_np(e["v_shaped"]), c["m"]["v_template"])


def test_a_nan_pose_poisons_its_own_frame_only():
    c = _case("wg19")
    net = _net()
    args = dict(betas=_dev(c["betas"]), transl=_dev(c["transl"]))
    clean = net.pose_bodies(c["model"], poses=_dev(c["poses"]), **args)
    poses = c["poses"].copy()
    poses[10, 7, 1] = np.nan                                        # frame 10: the second group of eight
    dirty = net.pose_bodies(c["model"], poses=_dev(poses), **args)
    others = [t for t in range(19) if t != 10]
    for k in ("vertices", "posed_joints", "joints", "rotations"):
        assert torch.equal(clean[k][others], dirty[k][others]), k
    assert bool(torch.isnan(dirty["vertices"][10]).all()) and bool(torch.isfinite(clean["vertices"]).all())
    rot = _np(clean["rotations"]).copy()
    rot[3, 0, 1, 1] = np.inf
    dirty = net.pose_bodies(c["model"], rotations=_dev(rot), **args)
    others = [t for t in range(19) if t != 3]
    assert torch.equal(clean["vertices"][others], dirty["vertices"][others]) and not bool(torch.isfinite(dirty["vertices"][3]).all())


def test_two_runs_are_bit_identical():
    c = _case("smpl")
    args = dict(poses=_dev(c["poses"]), betas=_dev(c["betas"]), transl=_dev(c["transl"]), scaling=1.25)
    a = _net().pose_bodies(c["model"], **args)
    c["model"]._shape_cache.clear()
    b = _net().pose_bodies(c["model"], **args)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_add_body_stores_the_sampled_points_and_float32_joints():
    c = _case("wg9")
    net, model = _net(), c["model"]
    args = dict(betas=_dev(c["betas"]), transl=_dev(c["transl"]), scaling=0.5)
    bank = ClipBank("cuda")
    i = bank.add_body(net, model, _dev(c["poses"]), count=700, seed=5, **args)
    posed = net.pose_bodies(model, poses=_dev(c["poses"]), **args)
    want = net.sample_surface(posed["vertices"], model.faces, count=700, seed=5, check=True)["points"]
    assert i == 0 and len(bank) == 1 and bank.points[0].dtype == torch.float32 and torch.equal(bank.points[0], want)
    assert bank.joints[0].dtype == torch.float32 and torch.equal(bank.joints[0], posed["joints"].to(torch.float32))
    out = net.voxelize_batch(bank, [0, 0], [0, 3], T=4, return_joints=True, check=True)
    assert tuple(out["vox"].shape) == (2, 4, 1, 32, 32, 32) and tuple(out["joints"].shape) == (2, 4, 24, 3) and out["joints"].dtype == torch.float32
    assert float(out["vox"].sum()) > 0 and bool(torch.isfinite(out["joints"]).all())


def test_python_argument_checks():
    c = _case("chain")
    net, model = _net(), c["model"]
    poses = _dev(c["poses"])
    for kw, word in ((dict(), "exactly one"), (dict(poses=poses, rotations=_dev(np.zeros((5, 5, 3, 3)))), "exactly one"),
                     (dict(poses=poses[:, :4].contiguous()), "poses must be"), (dict(poses=poses.cpu()), "network's device"),
                     (dict(poses=poses, betas=_dev(np.zeros(4))), "betas must be"), (dict(poses=poses, transl=_dev(np.zeros((4, 3)))), "transl must be"),
                     (dict(poses=poses, scaling=0.0), "scaling"), (dict(poses=poses, scaling=float("nan")), "scaling"),
                     (dict(poses=poses, dtype=torch.float16), "dtype"), (dict(rotations=_dev(np.zeros((5, 5, 3, 3)), np.float32)), "rotations must be")):
        with pytest.raises(ValueError) as e:
            net.pose_bodies(model, **kw)
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="BodyModel"):
        net.pose_bodies(c["m"], poses=poses)
    with pytest.raises(ValueError, match="network's device"):
        net.pose_bodies(BodyModel.synthetic(37, 5, 3, seed=1, parents=CHAIN5), poses=poses)


def test_abi_refusals_launch_nothing():
    c = _case("chain")
    net, model = _net(), c["model"]
    ctx = net._engine.ready()
    lib, h = ctx.lib, ctx.handle
    V, J, S, T = 37, 5, 3, 5
    buf = {k: torch.full((n,), -7.0, device="cuda", dtype=torch.float64) for k, n in
           (("rot", T * J * 9), ("tr", T * J * 12), ("posed", T * J * 3), ("vert", T * V * 3), ("vs", V * 3), ("jr", J * 3), ("joints", T * J * 3))}
    poses, betas = _dev(c["poses"]), _dev(c["betas"])
    p = lambda t: t.data_ptr()
    par = lambda *a: (C.c_int32 * len(a))(*a)
    good_par = par(*CHAIN5)
    BIG = 2 ** 31 - 1

    def pose(**kw):
        a = dict(poses=p(poses), f64=1, rot=None, T=T, V=V, J=J, par=good_par, vs=p(buf["vs"]), jr=p(buf["jr"]), pd=p(model.posedirs), w=p(model.lbs_weights),
                 tl=None, sc=1.0, rot_out=p(buf["rot"]), tr=p(buf["tr"]), posed=p(buf["posed"]), vert=p(buf["vert"]))
        a.update(kw)
        return lib.nm_body_pose(h, a["poses"], a["f64"], a["rot"], a["T"], a["V"], a["J"], a["par"], a["vs"], a["jr"], a["pd"], a["w"], a["tl"], a["sc"],
                                a["rot_out"], a["tr"], a["posed"], a["vert"])

    def shape(**kw):
        a = dict(vt=p(model.v_template), sd=p(model.shapedirs), b=p(betas), V=V, S=S, J=J, off=p(model.reg_offsets), cols=p(model.reg_cols), vals=p(model.reg_vals),
                 nnz=int(model.reg_cols.numel()), vs=p(buf["vs"]), jr=p(buf["jr"]))
        a.update(kw)
        return lib.nm_body_shape(h, a["vt"], a["sd"], a["b"], a["V"], a["S"], a["J"], a["off"], a["cols"], a["vals"], a["nnz"], a["vs"], a["jr"])

    def joints(**kw):
        a = dict(vert=p(buf["vert"]), T=T, V=V, J=J, off=p(model.reg_offsets), cols=p(model.reg_cols), vals=p(model.reg_vals), nnz=int(model.reg_cols.numel()),
                 out=p(buf["joints"]))
        a.update(kw)
        return lib.nm_body_joints(h, a["vert"], a["T"], a["V"], a["J"], a["off"], a["cols"], a["vals"], a["nnz"], a["out"])

    ARG, UNS = _lib.NM_ERR_ARG, _lib.NM_ERR_UNSUPPORTED
    refusals = [
        (pose, dict(vert=None), ARG), (pose, dict(vs=None), ARG), (pose, dict(par=None), ARG), (pose, dict(rot_out=None), ARG), (pose, dict(pd=None), ARG),
        (pose, dict(T=0), ARG), (pose, dict(V=0), ARG), (pose, dict(J=0), ARG), (pose, dict(J=65), ARG),
        (pose, dict(poses=None), ARG), (pose, dict(rot=p(buf["rot"])), ARG),
        (pose, dict(par=par(0, 0, 1, 2, 3)), ARG), (pose, dict(par=par(-1, 1, 1, 2, 3)), ARG), (pose, dict(par=par(-1, 0, 1, 2, 4)), ARG),
        (pose, dict(par=par(-1, 0, -1, 2, 3)), ARG),
        (pose, dict(sc=0.0), ARG), (pose, dict(sc=float("nan")), ARG), (pose, dict(sc=float("inf")), ARG),
        (pose, dict(T=BIG, V=2), UNS), (pose, dict(T=2 ** 30, V=1), UNS),
        (shape, dict(vt=None), ARG), (shape, dict(vs=None), ARG), (shape, dict(off=None), ARG), (shape, dict(cols=None), ARG), (shape, dict(sd=None), ARG),
        (shape, dict(S=-1), ARG), (shape, dict(V=0), ARG), (shape, dict(J=65), ARG), (shape, dict(nnz=-1), ARG), (shape, dict(V=2 ** 30), UNS),
        (joints, dict(vert=None), ARG), (joints, dict(out=None), ARG), (joints, dict(T=0), ARG), (joints, dict(J=0), ARG), (joints, dict(nnz=-1), ARG),
        (joints, dict(T=BIG, V=2), UNS), (joints, dict(T=2 ** 30, J=1, V=1), UNS),
    ]
    for fn, kw, want in refusals:
        rc = fn(**kw)
        assert rc == want, (fn.__name__, kw, rc, lib.nm_last_error())
        assert b"body_" in lib.nm_last_error()
    assert lib.nm_body_pose(None, p(poses), 1, None, T, V, J, good_par, p(buf["vs"]), p(buf["jr"]), p(model.posedirs), p(model.lbs_weights), None, 1.0,
                            p(buf["rot"]), p(buf["tr"]), p(buf["posed"]), p(buf["vert"])) == ARG
    torch.cuda.synchronize()
    for k, t in buf.items():
        assert bool((t == -7.0).all()), f"a refused call wrote {k}"
    assert shape() == 0 and pose() == 0 and joints() == 0            # the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    assert all(not bool((t == -7.0).any()) for t in buf.values())


def test_the_bound_on_the_rotations_is_the_measured_one():
    """ROT_BOUND is four times ROT_SEEN, rounded up to a power of two (0 for 0), and itself below the 1e-14 that no run may exceed"""
    want = 0.0 if ROT_SEEN == 0.0 else 2.0 ** int(np.ceil(np.log2(4.0 * ROT_SEEN)))
    assert ROT_BOUND == want and ROT_BOUND < 1e-14
