"""The body-model contract without a device: tests/body_ref.py (the loop-by-loop restatement of include/nm355.h that the GPU tests compare
bit for bit) against an independent vectorised implementation, against answers worked by hand, and against its own mutations; and
neural_marionette_amd.body.BodyModel itself - validation, storage layouts, from_npz, affinity()."""
import numpy as np
import pytest
import torch

import body_ref as B
from neural_marionette_amd import BodyModel

RZ = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])           # a quarter turn about z, exact


def _rotations(T, J, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return B.rodrigues(scale * rng.standard_normal((T, J, 3)))


def _dense_reg(m, V):
    J = m["reg_offsets"].shape[0] - 1
    reg = np.zeros((J, V))
    for j in range(J):
        for k in range(m["reg_offsets"][j], m["reg_offsets"][j + 1]):
            reg[j, m["reg_cols"][k]] = m["reg_vals"][k]
    return reg


def _einsum_forward(m, R, betas, transl, scaling):
    """the textbook form: matrix products, 4x4 transforms, no care for the order of any sum"""
    V, J = m["lbs_weights"].shape
    T = R.shape[0]
    reg = _dense_reg(m, V)
    v_shaped = m["v_template"] + (np.einsum("vcs,s->vc", m["shapedirs"], betas) if betas is not None else 0.0)
    J_rest = reg @ v_shaped
    feat = (R[:, 1:] - np.eye(3)).reshape(T, -1)
    vp = v_shaped[None] + (feat @ m["posedirs"]).reshape(T, V, 3)
    G = np.zeros((T, J, 4, 4))
    for j in range(J):
        L = np.zeros((T, 4, 4))
        L[:, :3, :3], L[:, 3, 3] = R[:, j], 1.0
        p = int(m["parents"][j])
        L[:, :3, 3] = J_rest[j] - (J_rest[p] if p >= 0 else 0.0)
        G[:, j] = L if p < 0 else G[:, p] @ L
    posed = G[:, :, :3, 3].copy()
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum("tjab,jb->tja", G[:, :, :3, :3], J_rest)
    Tm = np.einsum("vj,tjab->tvab", m["lbs_weights"], A)
    x = np.einsum("tvab,tvb->tva", Tm[:, :, :3, :3], vp) + Tm[:, :, :3, 3]
    tl = 0.0 if transl is None else transl[:, None, :]
    vertices = scaling * x + tl
    return dict(v_shaped=v_shaped, J_rest=J_rest, vertices=vertices, posed_joints=scaling * posed + tl, joints=np.einsum("jv,tvc->tjc", reg, vertices))


@pytest.mark.parametrize("V,J,S,T,smpl", [(1, 1, 0, 1, False), (37, 5, 3, 5, False), (130, 24, 10, 3, True), (61, 9, 2, 4, False)])
def test_restatement_against_einsum(V, J, S, T, smpl):
    m = BodyModel.synthetic(V, J, S, seed=V + J, parents=BodyModel.SMPL_PARENTS if smpl else None).numpy()
    rng = np.random.default_rng(7 * V)
    R = _rotations(T, J, seed=V)
    betas = rng.standard_normal(S) if S else None
    transl = rng.standard_normal((T, 3))
    got = B.forward(m, R, betas=betas, transl=transl, scaling=0.75)
    want = _einsum_forward(m, R, betas, transl, 0.75)
    for k, w in want.items():
        assert got[k].shape == w.shape, k
        assert np.abs(got[k] - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (k, np.abs(got[k] - w).max())


def test_rodrigues_zero_is_identity_and_quarter_turn():
    R = B.rodrigues(np.zeros((2, 3, 3)))
    assert np.array_equal(R, np.broadcast_to(np.eye(3), R.shape))
    assert np.array_equal(B.rodrigues(np.zeros((1, 1, 3), dtype=np.float32)), np.eye(3)[None, None])
    q = B.rodrigues(np.array([[[0.0, 0.0, np.pi / 2]]]))[0, 0]
    assert np.abs(q - RZ).max() < 1e-7                             # (the 1e-8 added inside the angle tilts the axis by that much)
    r = B.rodrigues(np.random.default_rng(0).standard_normal((4, 6, 3)))
    assert np.abs(np.einsum("tjab,tjcb->tjac", r, r) - np.eye(3)).max() < 1e-7
    assert np.allclose(np.linalg.det(r), 1.0, atol=1e-7)


def _hand_model(weights, parents, vt, select, shapedirs=None):
    """a model whose regressor row j selects vertex select[j], no pose blend shapes"""
    vt = np.asarray(vt, dtype=np.float64)
    V, J = vt.shape[0], len(parents)
    reg = np.zeros((J, V))
    for j, v in enumerate(select):
        reg[j, v] = 1.0
    sd = np.zeros((V, 3, 0)) if shapedirs is None else shapedirs
    faces = [[0, min(1, V - 1), min(2, V - 1)]]
    return BodyModel(vt, sd, np.zeros((V, 3, 9 * (J - 1))), reg, np.asarray(parents), np.asarray(weights, dtype=np.float64), faces)


def test_zero_pose_is_the_scaled_translated_shape_bit_for_bit():
    # dyadic numbers throughout: every sum of the chain and the skinning is exact, so M is exactly [I | 0]
    vt = [[0.5, 0.25, -1.0], [1.5, -0.75, 2.0], [0.125, 3.0, 0.5], [-2.0, 1.0, 0.375]]
    sd = np.zeros((4, 3, 2))
    sd[:, :, 0], sd[:, :, 1] = 0.25, [[0.5, 0.0, -0.5]] * 4
    model = _hand_model([[1, 0], [0.75, 0.25], [0.5, 0.5], [0, 1]], [-1, 0], vt, [0, 3], shapedirs=sd)
    m = model.numpy()
    betas, transl = np.array([2.0, -1.0]), np.array([[0.3, -0.7, 0.11], [5.0, 1e-3, -2.5]])
    out = B.forward(m, np.broadcast_to(np.eye(3), (2, 2, 3, 3)), betas=betas, transl=transl, scaling=0.5)
    hand = np.asarray(vt) + 0.25 * 2.0 + np.array([0.5, 0.0, -0.5]) * -1.0
    assert np.array_equal(out["v_shaped"], hand)
    assert np.array_equal(out["vertices"], 0.5 * out["v_shaped"][None] + transl[:, None, :])
    assert np.array_equal(out["J_rest"], hand[[0, 3]])
    assert np.array_equal(out["posed_joints"], 0.5 * hand[[0, 3]][None] + transl[:, None, :])


def test_one_joint_quarter_turn_about_z():
    model = _hand_model([[1], [1], [1]], [-1], [[1, 0, 0], [2, 0, 0], [1, 3, 5]], [0])
    out = B.forward(model.numpy(), RZ[None, None])
    # about the joint at (1, 0, 0): (2,0,0) -> (1,1,0); (1,3,5) -> (1-3, 0, 5) = (-2,0,5)
    assert np.array_equal(out["vertices"][0], [[1, 0, 0], [1, 1, 0], [-2, 0, 5]])
    assert np.array_equal(out["posed_joints"][0], [[1, 0, 0]]) and np.array_equal(out["joints"][0], [[1, 0, 0]])
    assert np.array_equal(out["transforms"][0, 0], np.concatenate([RZ, [[1.0], [-1.0], [0.0]]], axis=1))


def test_two_joint_bend_moves_the_child_only():
    model = _hand_model([[1, 0], [1, 0], [0, 1], [0.5, 0.5]], [-1, 0], [[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0, 4]], [0, 1])
    R = np.stack([np.eye(3), RZ])[None]
    out = B.forward(model.numpy(), R)
    # the child turns about (1,0,0): (2,0,0) -> (1,1,0); the vertex on the joint's axis, half and half, stays
    assert np.array_equal(out["vertices"][0], [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 0, 4]])
    assert np.array_equal(out["posed_joints"][0], [[0, 0, 0], [1, 0, 0]])


def test_rigid_global_rotation_keeps_pairwise_distances():
    model = BodyModel.synthetic(40, 6, 2, seed=3)
    m = model.numpy()
    R = np.broadcast_to(np.eye(3), (2, 6, 3, 3)).copy()
    R[1, 0] = _rotations(1, 1, seed=5)[0, 0]
    v = B.forward(m, R, betas=np.array([0.5, -1.0]))["vertices"]
    d = lambda x: np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    assert not np.allclose(v[0], v[1]) and np.abs(d(v[0]) - d(v[1])).max() < 1e-7     # (rodrigues is orthogonal to ~1e-8)


def test_joints_of_a_selecting_regressor_are_those_vertices():
    rng = np.random.default_rng(11)
    model = _hand_model(np.eye(3)[rng.integers(0, 3, 9)], [-1, 0, 1], rng.standard_normal((9, 3)), [4, 0, 7])
    out = B.forward(model.numpy(), _rotations(3, 3, seed=2), transl=rng.standard_normal((3, 3)), scaling=1.5)
    assert np.array_equal(out["joints"], out["vertices"][:, [4, 0, 7]])


@pytest.mark.parametrize("switch", ["reverse_blend", "keep_rest", "swap_parent", "translate_first"])
def test_mutations_change_the_result(switch):
    m = BodyModel.synthetic(50, 7, 3, seed=9, parents=[-1, 0, 1, 2, 1, 4, 0]).numpy()
    rng = np.random.default_rng(4)
    args = dict(betas=rng.standard_normal(3), transl=rng.standard_normal((3, 3)), scaling=0.5)
    R = _rotations(3, 7, seed=6)
    good, bad = B.forward(m, R, **args), B.forward(m, R, **args, **{switch: True})
    assert not np.array_equal(good["vertices"], bad["vertices"])
    if switch != "reverse_blend":                                  # a wrong formula, not only another rounding
        assert np.abs(good["vertices"] - bad["vertices"]).max() > 1e-3
    else:
        assert np.abs(good["vertices"] - bad["vertices"]).max() < 1e-12


# ---- BodyModel ------------------------------------------------------------------------------------------------------------------

def _arrays(V=6, J=3, S=2):
    rng = np.random.default_rng(1)
    reg = np.zeros((J, V))
    reg[0, [4, 1]], reg[1, [5, 0, 2]], reg[2, 3] = [0.25, 0.75], [0.5, 0.25, 0.25], 1.0
    w = np.zeros((V, J))
    w[np.arange(V), np.arange(V) % J] = 1.0
    return dict(v_template=rng.standard_normal((V, 3)).astype(np.float32), shapedirs=rng.standard_normal((V, 3, S)),
                posedirs=rng.standard_normal((V, 3, 9 * (J - 1))), J_regressor=reg, parents=np.array([-1, 0, 0]), lbs_weights=w,
                faces=np.array([[0, 1, 2], [3, 4, 5]]))


def test_storage_layouts_and_csr_order():
    a = _arrays()
    model = BodyModel(**a)
    m = model.numpy()
    assert (model.V, model.J, model.S, model.P) == (6, 3, 2, 18)
    assert all(m[k].dtype == np.float64 for k in ("v_template", "shapedirs", "posedirs", "lbs_weights", "reg_vals"))
    assert np.array_equal(m["v_template"], a["v_template"].astype(np.float64))          # widened exactly
    for p in (0, 7, 17):
        for v in (0, 5):
            for c in range(3):
                assert m["posedirs"][p, 3 * v + c] == a["posedirs"][v, c, p]
    assert m["reg_offsets"].tolist() == [0, 2, 5, 6] and m["reg_cols"].tolist() == [1, 4, 0, 2, 5, 3]
    assert m["reg_vals"].tolist() == [0.75, 0.25, 0.25, 0.25, 0.5, 1.0]
    assert m["faces"].dtype == np.int32 and model.parents.tolist() == [-1, 0, 0] and model.faces.dtype == torch.int32

    class Sparse:                                                    # what a scipy sparse matrix offers
        def toarray(self):
            return a["J_regressor"]
    m2 = BodyModel(**dict(a, J_regressor=Sparse())).numpy()
    assert np.array_equal(m2["reg_cols"], m["reg_cols"]) and np.array_equal(m2["reg_vals"], m["reg_vals"])
    one = BodyModel(np.zeros((2, 3)), np.zeros((2, 3, 0)), np.zeros((2, 3, 0)), np.ones((1, 2)), np.array([-1]), np.ones((2, 1)), [[0, 1, 1]])
    assert tuple(one.posedirs.shape) == (0, 6) and one.S == 0


@pytest.mark.parametrize("change,word", [
    (dict(v_template=np.zeros((6, 2))), "v_template"),
    (dict(shapedirs=np.zeros((5, 3, 2))), "shapedirs"),
    (dict(posedirs=np.zeros((6, 3, 9))), "posedirs"),
    (dict(posedirs=np.zeros((18, 18))), "posedirs"),
    (dict(J_regressor=np.zeros((3, 5))), "J_regressor"),
    (dict(lbs_weights=np.zeros((6, 2))), "lbs_weights"),
    (dict(faces=np.zeros((2, 4), dtype=np.int64)), "faces"),
    (dict(parents=np.array([-1, 0])), "posedirs"),
    (dict(parents=np.array([0, 0, 0])), "parents[0]"),
    (dict(parents=np.array([-1, 1, 0])), "parents[1]"),
    (dict(parents=np.array([-1, 0, 2])), "parents[2]"),
    (dict(parents=np.array([-1, 0, -1])), "parents[2]"),
    (dict(faces=np.array([[0, 1, 2], [3, 6, 5]])), "faces row 1"),
    (dict(faces=np.array([[0, -1, 2], [3, 4, 5]])), "faces row 0"),
])
def test_refusals_name_the_row(change, word):
    with pytest.raises(ValueError) as e:
        BodyModel(**dict(_arrays(), **change))
    assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("name,row", [("v_template", 4), ("shapedirs", 2), ("posedirs", 5), ("J_regressor", 1), ("lbs_weights", 3)])
def test_non_finite_entries_are_refused_with_their_row(name, row):
    a = _arrays()
    x = np.array(a[name], dtype=np.float64)
    x[row].flat[-1] = np.inf if row % 2 else np.nan
    with pytest.raises(ValueError) as e:
        BodyModel(**dict(a, **{name: x}))
    assert name in str(e.value) and f"row {row}" in str(e.value)


def test_more_than_64_joints_are_refused():
    with pytest.raises(ValueError, match="at most 64"):
        BodyModel.synthetic(70, 65, 0, seed=0)
    assert BodyModel.synthetic(70, 64, 0, seed=0).J == 64


def test_from_npz_file_layout_and_unsigned_root(tmp_path):
    a = _arrays(S=12)
    kt = np.array([[4294967295, 0, 0], [0, 1, 2]], dtype=np.uint32)
    keys = dict(v_template=a["v_template"], shapedirs=a["shapedirs"], posedirs=a["posedirs"], J_regressor=a["J_regressor"], weights=a["lbs_weights"],
                kintree_table=kt, f=a["faces"].astype(np.uint32))
    path = tmp_path / "model.npz"
    np.savez(path, **keys)
    for src in (str(path), keys):
        model = BodyModel.from_npz(src)
        m = model.numpy()
        assert model.parents.tolist() == [-1, 0, 0] and model.S == 10
        assert np.array_equal(m["shapedirs"], a["shapedirs"][:, :, :10])
        assert np.array_equal(m["posedirs"], a["posedirs"].reshape(18, 18).T)
        assert np.array_equal(m["faces"], a["faces"])
    assert BodyModel.from_npz(keys, num_betas=3).S == 3
    with pytest.raises(ValueError, match="weights"):
        BodyModel.from_npz({k: v for k, v in keys.items() if k != "weights"})
    with pytest.raises(ValueError, match="kintree_table"):
        BodyModel.from_npz(dict(keys, kintree_table=kt[0]))


def test_affinity_is_the_preparation_scripts_loop():
    model = BodyModel.synthetic(48, 24, 0, seed=0, parents=BodyModel.SMPL_PARENTS)
    assert len(BodyModel.SMPL_PARENTS) == 24
    want = torch.zeros(24, 24)
    for k in range(24):
        parent = BodyModel.SMPL_PARENTS[k]
        if parent < 0:
            continue
        want[k, parent] = 1
    want = torch.max(want, want.transpose(0, 1)).numpy()
    got = model.affinity()
    assert got.dtype == np.float32 and got.shape == (24, 24) and np.array_equal(got, want)
    assert np.array_equal(got, got.T) and int(got.sum()) == 46 and set(np.unique(got)) == {0.0, 1.0}


def test_synthetic_model_is_what_it_says():
    model = BodyModel.synthetic(130, 24, 10, seed=5, parents=BodyModel.SMPL_PARENTS)
    m = model.numpy()
    w = m["lbs_weights"]
    assert ((w != 0).sum(axis=1) <= 4).all() and np.abs(w.sum(axis=1) - 1.0).max() < 1e-12 and (w >= 0).all()
    assert np.abs(_dense_reg(m, 130).sum(axis=1) - 1.0).max() < 1e-12
    f = m["faces"]
    assert f.shape == (129, 3) and (f[:, 0] == 0).all() and f[-1].tolist() == [0, 129, 1]          # the fan closes
    again = BodyModel.synthetic(130, 24, 10, seed=5, parents=BodyModel.SMPL_PARENTS).numpy()
    assert all(np.array_equal(m[k], again[k]) for k in m)
    assert not np.array_equal(m["v_template"], BodyModel.synthetic(130, 24, 10, seed=6, parents=BodyModel.SMPL_PARENTS).numpy()["v_template"])
