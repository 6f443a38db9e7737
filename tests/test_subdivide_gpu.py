"""Loop subdivision, smooth vertex normals and smooth shading on the device (nm_subdiv_apply, nm_vertex_normals and nm_mesh_shade through
the C ABI; NeuralMarionette.subdivide / vertex_normals / render_mesh(vertex_normals=...) / render_retarget(subdivide=, smooth=)) against
the restatement tests/subdiv_ref.py, which tests/test_subdivide_cpu.py pins to known answers and shows to be sensitive to the order of
every sum.

Everything is compared BIT FOR BIT: the stencils are + and * only; the normals add one square root and a division, the shading two more
square roots - IEEE operations that are correctly rounded in float64 on the host and, the library being built with -ffp-contract=off, are
expected to be on the device.  A value that differs is a finding about the kernel, not a reason for a tolerance.

Shapes: the tiny meshes of subdiv_ref.MESHES - the 17 x 16 grid's first level is 1023 rows, three workgroups of 256 lanes and a tail; T = 1
and 3 frames (one group of NM_SUBDIV_FRAMES = 4 frames with a tail) and T = 9 (three groups); the icosahedron at three levels (642
vertices); a 48 x 40 camera.

Without the feature (this file on the parent commit): every test fails - the library exports none of the three symbols, so
_lib.load() raises, and NeuralMarionette has no subdivide / vertex_normals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_npz
import mesh_ref as MR
import render_ref as RR
import retarget_ref as TR
import subdiv_ref as SR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, PinholeCamera, LoopPlan, synth, _lib, modules

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAMES = sorted(SR.MESHES)
_NET, _PLANS = [], {}


def _net():
    if not _NET:
        o = HotPathOptions(grid_size=32)
        net = NeuralMarionette(o)
        net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
        net = net.cuda().eval()
        net.anneal(1)
        _NET.append(net)
    return _NET[0]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(_np(got) if isinstance(got, torch.Tensor) else got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    diff = got.view(np.uint8 if got.dtype == np.uint8 else np.uint64) != want.view(np.uint8 if want.dtype == np.uint8 else np.uint64)
    print(f"{what}: {int(diff.sum())} of {diff.size} values differ")
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ"


def _plans(name, levels):
    """(mesh vertices, triangles, the restatement's plan, the builder's plan on the device), built once per (mesh, levels)"""
    if (name, levels) not in _PLANS:
        verts, tri = SR.MESHES[name]()
        _PLANS[name, levels] = (verts, tri, SR.build_plan(tri, len(verts), levels), LoopPlan.build(tri, len(verts), levels, device="cuda"))
    return _PLANS[name, levels]


def _apply_abi(net, x, lv, slack=5, V=None):
    """nm_subdiv_apply as a C caller uses it, with the tables of one level given as numpy arrays, into a buffer that holds a sentinel"""
    eng = net._engine
    eng.ready()
    x = np.ascontiguousarray(x, np.float64)
    T, V = x.shape[0], x.shape[1] if V is None else V
    E = len(lv["edge"])
    tabs = dict(edge=_dev(lv["edge"], np.int32), ring_offsets=_dev(lv["ring_offsets"], np.int32), ring=_dev(lv["ring"], np.int32), w=_dev(lv["w"], np.float64))
    out = torch.full((T * (V + E) * 3 + slack,), -77.0, device="cuda", dtype=F64)
    bad = torch.full((2,), -77, device="cuda", dtype=torch.int32)
    null = lambda t: t.data_ptr() if t.numel() else None
    eng.call("nm_subdiv_apply", _dev(x, np.float64).data_ptr(), T, V, E, null(tabs["edge"]), tabs["ring_offsets"].data_ptr(), null(tabs["ring"]),
             len(lv["ring"]), tabs["w"].data_ptr(), out.data_ptr(), bad.data_ptr())
    torch.cuda.synchronize()
    assert (out[T * (V + E) * 3:] == -77.0).all() and int(bad[1]) == -77, "written past the end"
    return _np(out[:T * (V + E) * 3]).reshape(T, V + E, 3), int(bad[0])


def _normals_abi(net, verts, tri, face_offsets, faces, slack=5):
    eng = net._engine
    eng.ready()
    verts = np.ascontiguousarray(verts, np.float64)
    F, V = verts.shape[:2]
    out = torch.full((F * V * 3 + slack,), -77.0, device="cuda", dtype=F64)
    bad = torch.full((2,), -77, device="cuda", dtype=torch.int32)
    t, fo, fa = _dev(tri, np.int32), _dev(face_offsets, np.int32), _dev(faces, np.int32)
    null = lambda a: a.data_ptr() if a.numel() else None
    eng.call("nm_vertex_normals", _dev(verts, np.float64).data_ptr(), F, V, null(t), len(tri), fo.data_ptr(), null(fa), out.data_ptr(), bad.data_ptr())
    torch.cuda.synchronize()
    assert (out[F * V * 3:] == -77.0).all() and int(bad[1]) == -77, "written past the end"
    return _np(out[:F * V * 3]).reshape(F, V, 3), int(bad[0])


@pytest.mark.parametrize("name", NAMES)
def test_apply_agrees_bit_for_bit(name):
    net = _net()
    verts, tri, ref, plan = _plans(name, 1)
    V, lv = len(verts), ref["levels"][0]
    for T in (1, 3):
        x = SR.mixed_magnitudes((T, V, 3), seed=1 + T)
        got, bad = _apply_abi(net, x, lv)
        assert bad == 0
        _same_bits(got, SR.apply_level(x, lv), f"{name}: nm_subdiv_apply, T = {T}")
    colours = np.random.default_rng(5).uniform(0.0, 1.0, (V, 3))
    got = net.subdivide(_dev(colours, np.float64), plan)
    assert tuple(got.shape) == (ref["vertex_counts"][1], 3)
    _same_bits(got, SR.subdivide(colours, ref), f"{name}: subdivide, (V,3) colours")
    again = net.subdivide(_dev(colours, np.float64), plan)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64)), "two runs differ"


@pytest.mark.parametrize("name,levels,T", [("icosahedron", 3, 3), ("grid", 2, 9), ("bow_tie", 2, 2), ("icosahedron", 0, 2)])
def test_subdivide_levels_and_frame_groups(name, levels, T):
    net = _net()
    verts, tri, ref, plan = _plans(name, levels)
    x = SR.mixed_magnitudes((T, len(verts), 3), seed=11)
    x[0] = verts
    want = SR.subdivide(x, ref)
    xd = _dev(x, np.float64)
    got = net.subdivide(xd, plan)
    assert tuple(got.shape) == (T, ref["vertex_counts"][-1], 3)
    _same_bits(got, want, f"{name}: subdivide, {levels} levels, T = {T}")
    if levels:
        assert np.array_equal(_np(plan.triangles), ref["triangles"])
    for bound in (1, 24 * sum(ref["vertex_counts"][1:-1]) * 2 + 1):             # a frame at a time; two
        assert torch.equal(net.subdivide(xd, plan, bytes_bound=bound).view(torch.int64), got.view(torch.int64)), f"bytes_bound = {bound}"
    with pytest.raises(ValueError, match="bytes_bound"):
        net.subdivide(xd, plan, bytes_bound=0)


def test_guarded_tables():
    """tables that no plan validated: a row with a bad entry is NaN in every frame and counts once; every other row is unchanged"""
    net = _net()
    verts, tri, ref, _ = _plans("grid", 1)
    V, lv = len(verts), ref["levels"][0]
    E = len(lv["edge"])
    x = SR.mixed_magnitudes((3, V, 3), seed=7)
    want = SR.apply_level(x, lv)

    def check(tables, rows, what):
        got, bad = _apply_abi(net, x, tables)
        rows = sorted(rows)
        assert bad == len(rows), (what, bad, rows)
        assert np.isnan(got[:, rows]).all(), what
        keep = np.ones(V + E, bool)
        keep[rows] = False
        _same_bits(got[:, keep], want[:, keep], what)

    check(lv, [], "the plan's own tables")
    off = lv["ring_offsets"]
    interior = int(np.nonzero((lv["edge"][:, 3] >= 0))[0][300])
    boundary = int(np.nonzero((lv["edge"][:, 3] < 0))[0][7])
    for value in (V, -2):
        for col in range(4):
            t = dict(lv, edge=lv["edge"].copy())
            t["edge"][interior, col] = value
            check(t, [V + interior], f"edge row {interior}, column {col} = {value}")
        t = dict(lv, edge=lv["edge"].copy())
        t["edge"][boundary, 3] = value
        t["edge"][interior, 0] = value
        check(t, [V + interior, V + boundary], f"two edge rows = {value}")
        t = dict(lv, ring=lv["ring"].copy())
        t["ring"][off[100] + 2] = value                                         # vertex 100's third ring entry
        check(t, [100], f"a ring entry = {value}")
    t = dict(lv, ring_offsets=off.copy())
    t["ring_offsets"][41] = off[40] - 1                                         # decreasing: vertex 40 is bad; vertex 41 starts early but in range
    got, bad = _apply_abi(net, x, t)
    assert bad == 1 and np.isnan(got[:, 40]).all() and not np.isnan(np.delete(got, 40, axis=1)).any()
    keep = np.ones(V + E, bool)
    keep[[40, 41]] = False
    _same_bits(got[:, keep], want[:, keep], "a decreasing offset pair")
    t = dict(lv, ring_offsets=off.copy())
    t["ring_offsets"][V] = len(lv["ring"]) + 1                                  # past ring_len: the last vertex
    check(t, [V - 1], "an offset past ring_len")
    t = dict(lv, ring_offsets=off.copy())
    t["ring_offsets"][0] = -1
    check(t, [0], "a negative offset")


@pytest.mark.parametrize("name,levels", [("icosahedron", 0), ("icosahedron", 1), ("grid", 1), ("fan12", 1), ("unreferenced", 1), ("bow_tie", 0)])
def test_vertex_normals_agree_bit_for_bit(name, levels):
    net = _net()
    verts, tri, ref, plan = _plans(name, levels)
    fine = SR.subdivide(verts, ref)
    rng = np.random.default_rng(9)
    frames = np.stack([fine, fine * 3.0 + rng.standard_normal(fine.shape) * 0.05, SR.mixed_magnitudes(fine.shape, seed=4)])
    args = (ref["triangles"], ref["face_offsets"], ref["faces"])
    want = SR.vertex_normals(frames, *args)
    got, bad = _normals_abi(net, frames, *args)
    assert bad == 0
    _same_bits(got, want, f"{name}, level {levels}: nm_vertex_normals")
    length = np.linalg.norm(want, axis=2)
    assert (np.abs(length[length > 0] - 1.0) < 1e-15 * 4).all()
    api = net.vertex_normals(_dev(frames, np.float64), plan)
    _same_bits(api, want, f"{name}, level {levels}: vertex_normals")
    _same_bits(net.vertex_normals(_dev(frames[1], np.float64), plan), want[1], f"{name}: vertex_normals of (V,3)")


def test_vertex_normals_degenerate_and_guarded():
    net = _net()
    v = np.array([[[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [7, 7, 7]]])
    t = np.array([[0, 1, 2], [1, 2, 3]], np.int32)
    ref = SR.build_plan(t, 5, 0)
    got, bad = _normals_abi(net, v, t, ref["face_offsets"], ref["faces"])
    assert bad == 0 and (got[0, 0] == 0).all() and (got[0, 4] == 0).all() and got[0, 3].tolist() == [0.0, 0.0, 1.0]
    _same_bits(got, SR.vertex_normals(v, t, ref["face_offsets"], ref["faces"]), "degenerate triangles")
    none, bad = _normals_abi(net, v, np.zeros((0, 3), np.int32), np.zeros(6, np.int32), np.zeros(0, np.int32))
    assert bad == 0 and (none == 0).all()
    # guarded: a faces entry outside [0, M), a triangle index outside [0, V), offsets
    verts, tri, ref, _ = _plans("grid", 0)
    V, M = len(verts), len(tri)
    x = SR.mixed_magnitudes((3, V, 3), seed=8)
    want = SR.vertex_normals(x, tri, ref["face_offsets"], ref["faces"])

    def check(tri_, fo, fa, rows, what):
        got, bad = _normals_abi(net, x, tri_, fo, fa)
        assert bad == len(rows) and np.isnan(got[:, rows]).all(), (what, bad)
        keep = np.ones(V, bool)
        keep[rows] = False
        _same_bits(got[:, keep], want[:, keep], what)

    fo, fa = ref["face_offsets"], ref["faces"]
    for value in (M, -1):
        f2 = fa.copy()
        f2[fo[30] + 1] = value
        check(tri, fo, f2, [30], f"a faces entry = {value}")
    for value in (V, -2):
        t2 = tri.copy()
        t2[17, 1] = value
        rows = sorted(set(int(i) for i in tri[17]))                              # the row's vertices, the one replaced included
        check(t2, fo, fa, rows, f"a triangle index = {value}")
    o2 = fo.copy()
    o2[V] = 3 * M + 1
    check(tri, o2, fa, [V - 1], "an offset past 3 M")
    o2 = fo.copy()
    o2[51] = fo[50] - 1
    got, bad = _normals_abi(net, x, tri, o2, fa)
    assert bad == 1 and np.isnan(got[:, 50]).all()


def _ico_scene():
    verts, tri, ref, plan = _plans("icosahedron", 1)
    E = RR.rigid((0.2, -0.3, 0.1), (0.0, 0.0, 3.0))
    cam = PinholeCamera(E.tolist(), 42.0, 42.0, 23.5, 19.5, 48, 40)
    fine = SR.subdivide(verts, ref)
    frames = np.stack([MR.posed(fine, E, (0.3, 0.2, 0.1), (0.0, 0.0, 3.0)), MR.posed(fine, E, (1.1, -0.4, 0.6), (0.3, -0.2, 2.6), 0.8)])
    normals = SR.vertex_normals(frames, ref["triangles"], ref["face_offsets"], ref["faces"])
    return ref, plan, cam, frames, normals


def test_render_mesh_with_vertex_normals():
    net = _net()
    ref, plan, cam, frames, normals = _ico_scene()
    V = frames.shape[1]
    colours = RR.palette(V, 3)
    vd, nd, cd = _dev(frames, np.float64), _dev(normals, np.float64), _dev(colours, np.float64)
    kw = dict(light=(0.3, 0.7), background=(0.25, 0.5, 1.0))
    flat = net.render_mesh(vd, plan.triangles, cam, vertex_colors=cd, return_index=True, return_depth=True, **kw)
    for colour_kw, ref_kw in ((dict(vertex_colors=cd), dict(vertex_colors=colours)), (dict(color=(0.9, 0.6, 0.2)), dict(color=(0.9, 0.6, 0.2)))):
        want = SR.render_smooth(frames, ref["triangles"], normals, cam, **ref_kw, **kw)
        assert (want["index"] >= 0).sum() > 400 and (want["image"] != want["flat_image"]).any() and not want["fallback"].any()
        got = net.render_mesh(vd, plan.triangles, cam, vertex_normals=nd, return_index=True, return_depth=True, **colour_kw, **kw)
        _same_bits(got["image"], want["image"], "smooth image")
        assert torch.equal(got["index"], flat["index"]) and torch.equal(got["depth"].view(torch.int64), flat["depth"].view(torch.int64))
        assert np.array_equal(_np(got["index"]), want["index"])
        only = net.render_mesh(vd, plan.triangles, cam, vertex_normals=nd, record_bytes=1, **colour_kw, **kw)       # a frame at a time, no index returned
        assert set(only) == {"image", "bin_total"} and torch.equal(only["image"], got["image"])
        assert torch.equal(net.render_mesh(vd, plan.triangles, cam, vertex_normals=nd, **colour_kw, **kw)["image"], got["image"]), "two runs differ"
    # a zero normal at every vertex of the triangle that wins the most pixels of frame 0: its pixels fall back to the flat shade, and its
    # neighbours mix zero with their other normals
    seen = want["index"][0]
    holes = normals.copy()
    holes[:, ref["triangles"][np.bincount(seen[seen >= 0]).argmax()]] = 0.0
    want = SR.render_smooth(frames, ref["triangles"], holes, cam, vertex_colors=colours, **kw)
    assert want["fallback"].sum() > 5
    got = net.render_mesh(vd, plan.triangles, cam, vertex_colors=cd, vertex_normals=_dev(holes, np.float64), **kw)
    _same_bits(got["image"], want["image"], "smooth image with zero normals")
    fb = torch.from_numpy(want["fallback"]).cuda()
    assert torch.equal(got["image"][fb], flat["image"][fb])
    zero = net.render_mesh(vd, plan.triangles, cam, vertex_colors=cd, vertex_normals=torch.zeros_like(nd), **kw)
    assert torch.equal(zero["image"], flat["image"]), "all-zero normals: the flat image"
    # None is the unmodified call
    assert torch.equal(net.render_mesh(vd, plan.triangles, cam, vertex_colors=cd, vertex_normals=None, **kw)["image"], flat["image"])
    with pytest.raises(ValueError, match="vertex_normals"):
        net.render_mesh(vd, plan.triangles, cam, vertex_normals=nd[:1], **kw)
    with pytest.raises(ValueError, match="vertex_normals"):
        net.render_mesh(vd, plan.triangles, cam, vertex_normals=nd.float(), **kw)


def test_render_retarget_subdivided_and_smooth(golden_dir, monkeypatch):
    g = golden_npz.load(os.path.join(golden_dir, "g16_retarget32.npz"))
    seeds = dict(zip(("G", "T", "N", "weights", "source", "target", "pick", "eps_source", "eps_target"), g["meta"].tolist()))
    o, sd, source, target, _, eps_s, eps_t = TR.g16_inputs(seeds)
    net = NeuralMarionette(o)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    net.anneal(1)
    verts, tri = MR.torus(16, 10, 0.55, 0.22)
    K = o.nkeypoints
    force = torch.arange(len(verts), dtype=torch.int32) % K
    result = net.sample_retarget(source.cuda(), target.cuda(), torch.from_numpy(verts), hardness=float(g["hardness"]), threshold=float(g["threshold"]),
                                 eps_source=eps_s.cuda(), eps_target=eps_t.cuda(), force_nearest=force)
    E = RR.rigid((0.2, -0.3, 0.1), (0.0, 0.0, 3.0))
    cam = PinholeCamera(E.tolist(), 60.0, 60.0, 31.5, 23.5, 64, 48)
    t = _dev(tri, np.int32)
    jc = torch.from_numpy(RR.palette(K, 12)).cuda()
    rk = dict(radius=0.1, bone_radius=0.07)
    today = net.render_retarget(result, t, cam, skin_colors=True, joint_colors=jc, **rk)
    same = net.render_retarget(result, t, cam, skin_colors=True, joint_colors=jc, subdivide=0, smooth=False, plan=None, **rk)
    assert set(same) == set(today) and all(torch.equal(same[k], today[k]) for k in today)
    # by hand
    plan = LoopPlan.build(t, len(verts), 1, device="cuda")
    fine = net.subdivide(result["points"], plan)
    vc = net.subdivide((result["skin_weights"].double() @ jc).contiguous(), plan)
    normals = net.vertex_normals(fine, plan)
    mesh = net.render_mesh(fine, plan.triangles, cam, vertex_colors=vc, vertex_normals=normals)["image"]
    parents = net.dyna_module.parents
    skeleton = net.render_skeleton(result["keypoints"], parents, cam, **rk)["image"]
    overlay = net.render_skeleton(result["keypoints"], parents, cam, over=mesh, **rk)["image"]
    assert not torch.equal(mesh, today["mesh"])
    for kw in (dict(), dict(plan=plan)):
        out = net.render_retarget(result, t, cam, skin_colors=True, joint_colors=jc, subdivide=1, smooth=True, **kw, **rk)
        assert torch.equal(out["mesh"], mesh) and torch.equal(out["skeleton"], skeleton) and torch.equal(out["overlay"], overlay)
        assert torch.equal(out["source_skeleton"], today["source_skeleton"])
    monkeypatch.setattr(modules, "SUBDIV_BYTES", 1)                             # a frame at a time
    out = net.render_retarget(result, t, cam, skin_colors=True, joint_colors=jc, subdivide=1, smooth=True, plan=plan, **rk)
    assert torch.equal(out["mesh"], mesh) and torch.equal(out["overlay"], overlay)
    monkeypatch.undo()
    faceted = net.render_retarget(result, t, cam, subdivide=1, plan=plan, **rk)["mesh"]
    assert torch.equal(faceted, net.render_mesh(fine, plan.triangles, cam)["image"])
    smooth0 = net.render_retarget(result, t, cam, smooth=True, **rk)["mesh"]
    plan0 = LoopPlan.build(t, len(verts), 0, device="cuda")
    assert torch.equal(smooth0, net.render_mesh(result["points"], t, cam, vertex_normals=net.vertex_normals(result["points"], plan0))["image"])
    with pytest.raises(ValueError, match="plan"):
        net.render_retarget(result, t, cam, subdivide=2, plan=plan, **rk)


def test_arguments_are_judged_before_any_launch():
    net = _net()
    eng = net._engine
    eng.ready()
    lib, h = eng.ctx.lib, eng.ctx.handle
    ARG, UNS = _lib.NM_ERR_ARG, _lib.NM_ERR_UNSUPPORTED
    # nm_subdiv_apply(ctx, in, T, V, E, edge, ring_offsets, ring, ring_len, w, out, bad_rows): pointers that are never used
    ok = [1, 2, 5, 4, 1, 1, 1, 6, 1, 1, 1]
    cases = [(0, None, ARG), (1, 0, ARG), (2, 0, ARG), (3, -1, ARG), (4, None, ARG), (5, None, ARG), (6, None, ARG), (7, -1, ARG), (8, None, ARG), (9, None, ARG),
             (10, None, ARG)]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_subdiv_apply(h, *args) == code, ("apply", pos, val)
    assert lib.nm_subdiv_apply(None, *ok) == ARG
    assert b"subdiv_apply" in lib.nm_last_error()
    big = list(ok)
    big[2], big[3] = 2 ** 30, 2 ** 30                                            # V + E = 2^31
    assert lib.nm_subdiv_apply(h, *big) == UNS
    # nm_vertex_normals(ctx, vertices, F, V, triangles, M, face_offsets, faces, normals, bad_rows)
    ok = [1, 2, 5, 1, 4, 1, 1, 1, 1]
    cases = [(0, None, ARG), (1, 0, ARG), (2, 0, ARG), (3, None, ARG), (4, -1, ARG), (4, (2 ** 31 + 2) // 3, UNS), (5, None, ARG), (6, None, ARG), (7, None, ARG),
             (8, None, ARG)]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_vertex_normals(h, *args) == code, ("normals", pos, val)
    assert lib.nm_vertex_normals(None, *ok) == ARG
    assert b"vertex_normals" in lib.nm_last_error()
    # nm_mesh_shade(ctx, rec, index, triangles, normals, vertex_colors, color, F, V, M, camera, light_a, light_b, background, image)
    good = PinholeCamera(np.eye(4).tolist(), 40.0, 40.0, 24.0, 20.0, 48, 40)

    def cam(**kw):
        c = good.c_struct()
        for k, val in kw.items():
            setattr(c, k, val)
        return C.byref(c)

    ok = [1, 1, 1, 1, None, None, 1, 5, 4, cam(), 1.0, 0.0, None, 1]
    cases = [(0, None, ARG), (1, None, ARG), (2, None, ARG), (3, None, ARG), (6, 0, ARG), (7, 0, ARG), (8, -1, ARG), (8, 2 ** 31, UNS), (9, None, ARG), (13, None, ARG),
             (9, cam(width=0), ARG), (9, cam(fx=float("nan")), ARG), (9, cam(near=0.0), ARG), (9, cam(width=65536, height=32768), UNS)]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_mesh_shade(h, *args) == code, ("shade", pos, val)
    assert lib.nm_mesh_shade(None, *ok) == ARG
    assert b"mesh_shade" in lib.nm_last_error()
    torch.cuda.synchronize()
