"""Loop-subdivision plans without a device: LoopPlan.build (neural_marionette_amd/subdivide.py, vectorised numpy) against the restatement
tests/subdiv_ref.py (plain dicts and loops), the restatement against known answers, and the sharpness of the bit-for-bit comparison that
tests/test_subdivide_gpu.py makes: each deliberate order mistake changes bits.

A mutation that swaps c and d shows nothing: in 0.125 * (x[c] + x[d]) that cannot change a bit, IEEE addition being commutative;
test_swapping_c_and_d_is_invisible_in_the_values pins that down (the c, d order is a property of the table, which
test_tables_equal_the_restatement compares exactly), and the mutation used for the edge rows pairs a with c instead, which does."""
import numpy as np
import pytest
import torch

import subdiv_ref as SR
from neural_marionette_amd import LoopPlan, NeuralMarionette, HotPathOptions, _lib

NAMES = sorted(SR.MESHES)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rows_changed(a, b):
    return int((_bits(a) != _bits(b)).any(axis=(0, 2)).sum()) if a.ndim == 3 else int((_bits(a) != _bits(b)).any(axis=1).sum())


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_tables_equal_the_restatement(name, levels):
    verts, tri = SR.MESHES[name]()
    V = len(verts)
    plan, ref = LoopPlan.build(tri, V, levels, device="cpu"), SR.build_plan(tri, V, levels)
    assert plan.levels == levels and plan.vertex_counts == ref["vertex_counts"] and plan.triangle_counts == ref["triangle_counts"]
    for got, want in zip(plan.levels_tables, ref["levels"]):
        for key in ("edge", "ring_offsets", "ring"):
            assert got[key].dtype == torch.int32 and np.array_equal(got[key].numpy(), want[key]), (name, key)
        assert got["w"].dtype == torch.float64 and np.array_equal(_bits(got["w"].numpy()), _bits(want["w"])), name
    for key in ("triangles", "face_offsets", "faces"):
        got = getattr(plan, key)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), ref[key]), (name, key)
    # counts: V' = V + E, M' = 4 M, and V - E + M does not change (E' = 2 E + 3 M)
    for l, lv in enumerate(ref["levels"]):
        E, M = len(lv["edge"]), ref["triangle_counts"][l]
        assert ref["vertex_counts"][l + 1] == ref["vertex_counts"][l] + E and ref["triangle_counts"][l + 1] == 4 * M
    euler = []
    for l in range(levels + 1):
        t = ref["levels"][l - 1]["children"] if l else np.asarray(tri)
        edges = {(min(a, b), max(a, b)) for r in t for a, b in ((r[0], r[1]), (r[1], r[2]), (r[2], r[0]))}
        euler.append(ref["vertex_counts"][l] - len(edges) + len(t))
    assert len(set(euler)) == 1, euler


def test_a_plan_without_levels_is_the_mesh_itself():
    verts, tri = SR.grid()
    plan, ref = LoopPlan.build(torch.from_numpy(tri), len(verts), 0, device="cpu"), SR.build_plan(tri, len(verts), 0)
    assert plan.levels_tables == [] and plan.vertex_counts == [272] and plan.triangle_counts == [480]
    for key in ("triangles", "face_offsets", "faces"):
        assert np.array_equal(getattr(plan, key).numpy(), ref[key])


def test_grid_and_icosahedron_sizes():
    verts, tri = SR.grid()
    lv = SR.build_plan(tri, len(verts), 1)["levels"][0]
    assert len(verts) == 272 and len(lv["edge"]) == 751 and int((lv["edge"][:, 3] < 0).sum()) == 62
    valence = np.bincount(lv["edge"][:, :2].reshape(-1), minlength=272)
    assert sorted(valence[[0, 16, 255, 271]].tolist()) == [2, 2, 3, 3] and set(valence.tolist()) == {2, 3, 4, 6}
    assert 272 + 751 > 256 and (272 + 751) % 256 != 0                  # more than one workgroup of 256 lanes, and a tail
    ico = SR.build_plan(SR.icosahedron()[1], 12, 3)
    assert ico["vertex_counts"] == [12, 42, 162, 642] and ico["triangle_counts"] == [20, 80, 320, 1280]
    fan = SR.build_plan(SR.fan()[1], 13, 1)["levels"][0]
    assert fan["ring_offsets"][1] == 12 and (np.diff(fan["ring_offsets"])[1:] == 2).all()
    bow = SR.build_plan(SR.bow_tie()[1], 9, 1)["levels"][0]
    assert bow["ring_offsets"][1] == 0 and bow["w"][0].tolist() == [1.0, 0.0]
    unref = SR.build_plan(SR.with_unreferenced()[1], 5, 1)["levels"][0]
    assert unref["ring_offsets"][3] == unref["ring_offsets"][2] and unref["w"][2].tolist() == [1.0, 0.0]


def test_children_keep_the_winding_on_the_planar_grid():
    verts, tri = SR.grid()
    plan = SR.build_plan(tri, len(verts), 2)
    x, t = verts, np.asarray(tri)
    for lv in plan["levels"]:
        y = SR.apply_level(x[None], lv)[0]
        nz = lambda p, q: np.cross(p[q[:, 1]] - p[q[:, 0]], p[q[:, 2]] - p[q[:, 0]])[:, 2]
        parent, child = nz(x, t), nz(y, lv["children"])
        assert (parent != 0).all() and (np.sign(child) == np.sign(np.repeat(parent, 4))).all()
        x, t = y, lv["children"]


def test_refusals_name_the_row():
    verts, tri = SR.octahedron()
    for levels in (0, 1):
        bad = tri.copy(); bad[5, 1] = 6
        with pytest.raises(ValueError, match=r"row 5 .*outside \[0, 6\)"):
            LoopPlan.build(bad, 6, levels, device="cpu")
        bad = tri.copy(); bad[3, 0] = -1
        with pytest.raises(ValueError, match=r"row 3 .*outside"):
            LoopPlan.build(bad, 6, levels, device="cpu")
        bad = tri.copy(); bad[2] = (1, 3, 1)
        with pytest.raises(ValueError, match=r"row 2 .*repeats an index"):
            LoopPlan.build(bad, 6, levels, device="cpu")
        fin = np.concatenate([tri, [[0, 2, 1]]]).astype(np.int32)      # a third triangle on the edge (0, 2) - and on (1, 2)
        with pytest.raises(ValueError, match=r"row 8 .*third triangle of the undirected edge \(0, 2\)"):
            LoopPlan.build(fin, 6, levels, device="cpu")
    for V, levels in ((0, 1), (6, -1)):
        with pytest.raises(ValueError):
            LoopPlan.build(tri, V, levels, device="cpu")
    with pytest.raises(ValueError, match="integers"):
        LoopPlan.build(tri.astype(np.float64), 6, 1, device="cpu")


def test_tetrahedron_known_answers():
    verts, tri = SR.tetrahedron()
    lv = SR.build_plan(tri, 4, 1)["levels"][0]
    assert np.abs(lv["w"] - [7.0 / 16.0, 3.0 / 16.0]).max() <= 1e-15
    # rows of tri: (0,1,2) (0,3,1) (0,2,3) (1,3,2)
    assert lv["edge"].tolist() == [[0, 1, 2, 3], [0, 2, 1, 3], [0, 3, 1, 2], [1, 2, 0, 3], [1, 3, 0, 2], [2, 3, 0, 1]]
    assert lv["ring"].tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert lv["children"][:4].tolist() == [[0, 4, 5], [4, 1, 7], [5, 7, 2], [4, 7, 5]]


@pytest.mark.parametrize("name", NAMES)
def test_a_constant_field_is_reproduced_exactly(name):
    """for c a power of two every product is exact but y = w_ring * (n c) = fl(n beta_n) c, and w_self c + y = (fl(1 - fl(n beta_n)) +
    fl(n beta_n)) c: 1 - y is off by at most 2^-54 (y lies in [0.23, 0.61]), so the sum is within 2^-54 of 1 and rounds to 1 exactly"""
    verts, tri = SR.MESHES[name]()
    plan = SR.build_plan(tri, len(verts), 2)
    for value in (1.0, -0.25, 1024.0):
        out = SR.subdivide(np.full((2, len(verts), 3), value), plan)
        assert out.shape == (2, plan["vertex_counts"][-1], 3) and (out == value).all(), (name, value)


def test_regular_interior_vertices_of_the_grid_stay_put():
    verts, tri = SR.grid()
    lv = SR.build_plan(tri, 272, 1)["levels"][0]
    c, sn = np.cos(0.7), np.sin(0.7)
    verts = verts @ np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.3, 0.1, 1.0]]).T / 1.1 + 0.1     # a sheared lattice, coordinates up to 24
    out = SR.apply_level(verts[None], lv)[0]
    n = np.diff(lv["ring_offsets"])
    on_boundary = np.zeros(272, bool)
    on_boundary[lv["edge"][lv["edge"][:, 3] < 0][:, :2].reshape(-1)] = True
    regular = (n == 6) & ~on_boundary
    assert regular.sum() == 15 * 14
    err = np.abs(out[:272][regular] - verts[regular]).max()
    print("regular interior vertices move by", err)
    assert err <= 1e-14


@pytest.mark.parametrize("name", ["icosahedron", "grid", "fan12", "bow_tie"])
def test_an_affine_map_commutes_with_subdivision(name):
    verts, tri = SR.MESHES[name]()
    plan = SR.build_plan(tri, len(verts), 2)
    rng = np.random.default_rng(3)
    A, t = rng.standard_normal((3, 3)), rng.standard_normal(3)
    a, b = SR.subdivide(verts @ A.T + t, plan), SR.subdivide(verts, plan) @ A.T + t
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def test_known_normals():
    verts, tri = SR.grid()
    for levels in (0, 1):
        plan = SR.build_plan(tri, 272, levels)
        fine = SR.subdivide(verts, plan)
        n = SR.vertex_normals(fine[None], plan["triangles"], plan["face_offsets"], plan["faces"])[0]
        assert (n[:, :2] == 0.0).all() and (np.abs(n[:, 2]) == 1.0).all() and len(set(n[:, 2].tolist())) == 1
    verts, tri = SR.icosahedron()
    plan = SR.build_plan(tri, 12, 0)
    n = SR.vertex_normals(verts[None], plan["triangles"], plan["face_offsets"], plan["faces"])[0]
    assert np.abs(n - verts / np.linalg.norm(verts, axis=1, keepdims=True)).max() <= 1e-15
    # a vertex whose triangles are all degenerate, and one without triangles: zeros
    v = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [7, 7, 7]])
    t = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    plan = SR.build_plan(t, 5, 0)
    n = SR.vertex_normals(v[None], plan["triangles"], plan["face_offsets"], plan["faces"])[0]
    assert (n[0] == 0).all() and (n[4] == 0).all() and n[3].tolist() == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("name", ["grid", "icosahedron", "fan12", "octahedron"])
def test_order_mistakes_change_bits(name):
    """sharpness by mutation, on inputs whose sums depend on their order"""
    verts, tri = SR.MESHES[name]()
    V = len(verts)
    plan = SR.build_plan(tri, V, 1)
    x = SR.mixed_magnitudes((3, V, 3), seed=1)
    good = SR.subdivide(x, plan)
    ring = _rows_changed(good[:, :V], SR.subdivide(x, plan, ring_reverse=True)[:, :V])
    pair = _rows_changed(good[:, V:], SR.subdivide(x, plan, pair_ac=True)[:, V:])
    nplan = SR.build_plan(tri, V, 0)
    args = (nplan["triangles"], nplan["face_offsets"], nplan["faces"])
    faces = _rows_changed(SR.vertex_normals(x, *args), SR.vertex_normals(x, *args, faces_reverse=True))
    print(f"{name}: reversed rings change {ring} of {V} old-vertex rows, a-c pairing {pair} of {len(plan['levels'][0]['edge'])} edge rows, "
          f"reversed faces {faces} of {V} normals")
    assert ring >= 1 and pair >= 1 and faces >= 1


def test_swapping_c_and_d_is_invisible_in_the_values():
    verts, tri = SR.grid()
    plan = SR.build_plan(tri, 272, 1)
    x = SR.mixed_magnitudes((2, 272, 3), seed=2)
    swapped = dict(plan["levels"][0])
    e = swapped["edge"].copy()
    inner = e[:, 3] >= 0
    e[inner, 2], e[inner, 3] = plan["levels"][0]["edge"][inner, 3], plan["levels"][0]["edge"][inner, 2]
    swapped["edge"] = e
    assert inner.sum() == 751 - 62 and (e[inner, 2] != plan["levels"][0]["edge"][inner, 2]).all()
    assert np.array_equal(_bits(SR.apply_level(x, plan["levels"][0])), _bits(SR.apply_level(x, swapped)))


def test_arguments_are_judged_before_the_context():
    """the Python entry points refuse what they can before touching the device"""
    net = NeuralMarionette(HotPathOptions(grid_size=32))
    verts, tri = SR.tetrahedron()
    plan = LoopPlan.build(tri, 4, 1, device="cpu")
    x = torch.from_numpy(verts)
    with pytest.raises(ValueError, match="LoopPlan"):
        net.subdivide(x, "plan")
    with pytest.raises(ValueError, match=r"\(T,4,3\) or \(4,3\) float64"):
        net.subdivide(x.float(), plan)
    with pytest.raises(ValueError, match=r"\(T,4,3\)"):
        net.subdivide(torch.zeros(5, 3, dtype=torch.float64), plan)
    with pytest.raises(ValueError, match="device"):
        net.subdivide(x, plan)
    with pytest.raises(ValueError, match=r"\(T,10,3\)"):
        net.vertex_normals(x, plan)
    assert {"nm_subdiv_apply", "nm_vertex_normals", "nm_mesh_shade"} <= set(_lib.SIGNATURES)
