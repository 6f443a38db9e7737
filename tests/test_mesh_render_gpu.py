"""The mesh and skeleton render path on the device (nm_mesh_bin + nm_mesh_draw and nm_skeleton_draw through the C ABI,
NeuralMarionette.render_mesh / render_skeleton / render_retarget) against the float64 numpy restatement tests/mesh_ref.py, which
tests/test_mesh_render_cpu.py pins to hand-derived results, to a world-space ray caster and to the no-cracks property.

What is compared how:
  mesh index   equal to the restatement on every pixel, no exemptions.
  mesh depth   bit for bit: + - * / only, correctly rounded, built with -ffp-contract=off - the ground the plate tests stand on.
  mesh image   exact with the flat light (1, 0); within one uint8 level with a lit setting, whose square roots are the one operation
               whose last bit on the device nobody has checked (tests/test_render_gpu.py says the same).
  skeleton     coverage (index >= 0) exact: hit or miss needs no square root.  index exact except where the restatement's best and
               second-best depths differ by less than a relative 1e-12 (mesh_ref.near_ties; at most 0.5 % of the covered pixels, which
               the scene's constructor checks of the restatement alone); depth within 4 ulp (one sqrt, one division); image within one
               level where the index agrees.
A pixel that differs is a finding about the kernel's operation order, not a reason for a tolerance.

Shapes: 40 x 33 pixels (3 x 3 tiles of 16 x 16, the right and bottom ones partial), F = 3 frames with the middle one behind the camera,
400 triangles; the icosphere (320) and the torus (320); hand-made degenerates; one 16 x 16 image - a single tile - under
3 * NM_MESH_CHUNK = 384 triangles (csrc/nm_mesh.h: the draw kernel stages a tile's triangles through LDS 128 at a time); the hand-made
skeleton at 40 x 33 and on a single tile; and sample_retarget at G = 32 on a procedural torus end to end.

Without the feature (this file and tests/test_mesh_render_cpu.py on the parent commit, one MI355X): all 11 tests here fail with
AttributeError - "undefined symbol: nm_mesh_bin" / nm_skeleton_draw from the library, or NeuralMarionette has no render_mesh - and of the
CPU file test_arguments_are_judged_before_the_context fails the same way; its tests of the restatement alone pass."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import golden_npz
import mesh_ref as MR
import render_ref as RR
import retarget_ref as TR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, PinholeCamera, synth, _lib

pytestmark = pytest.mark.gpu

F64 = torch.float64
NM_MESH_CHUNK = 128                                                           # csrc/nm_mesh.h
BG = (0.25, 0.5, 1.0)
_NET = []


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


def _compare(got, ref, what, lit=False):
    """index / depth / image of one mesh render (numpy or tensors) against the restatement's"""
    got = {k: (_np(v) if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    shape = ref["index"].shape
    if "index" in got:
        g = got["index"].reshape(shape)
        bad = int((g != ref["index"]).sum())
        print(f"{what}: {int((ref['index'] >= 0).sum())} covered pixels of {g.size}, index differs on {bad}")
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(ref["index"])), f"{what}: index differs on {bad} pixels"
    if "depth" in got:
        g = np.ascontiguousarray(got["depth"].reshape(shape))
        assert g.dtype == np.float64 and np.array_equal(g.view(np.uint8), np.ascontiguousarray(ref["depth"]).view(np.uint8)), f"{what}: depth differs"
    if "image" in got:
        g = got["image"].reshape(shape + (3,))
        err = int(np.abs(g.astype(np.int32) - ref["image"].astype(np.int32)).max(initial=0))
        print(f"{what}: image max |difference| {err} levels")
        assert err <= (1 if lit else 0), f"{what}: image differs by {err} levels"


def _abi(net, vertices, tri, cam, vertex_colors=None, color=None, light=(1.0, 0.0), background=None, capacity=None, want=("index", "depth", "image"), slack=8):
    """nm_mesh_bin + nm_mesh_draw as a C caller uses them, into buffers that hold a sentinel"""
    eng = net._engine
    eng.ready()
    vertices = np.asarray(vertices, np.float64)
    F, V, M = vertices.shape[0], vertices.shape[1], len(tri)
    H, W = cam.height, cam.width
    nt = F * ((W + 15) // 16) * ((H + 15) // 16)
    v, t = _dev(vertices, np.float64), _dev(tri, np.int32)
    c = _dev(vertex_colors, np.float64) if vertex_colors is not None else None
    rec = torch.full((F * M + 1, 16), -77.0, device="cuda", dtype=F64)
    rect = torch.full((F * M + 1, 4), -77, device="cuda", dtype=torch.int32)
    toff = torch.full((nt + 2,), -77, device="cuda", dtype=torch.int64)
    cs = cam.c_struct()
    eng.call("nm_mesh_bin", v.data_ptr(), t.data_ptr(), F, V, M, C.byref(cs), rec.data_ptr(), rect.data_ptr(), toff.data_ptr())
    total = int(toff[nt].item())
    assert int(toff[nt + 1].item()) == -77 and (rec[F * M] == -77).all() and (rect[F * M] == -77).all()
    cap = total if capacity is None else capacity
    lst = torch.full((cap + slack,), -77, device="cuda", dtype=torch.int32)
    shapes = dict(index=((F * H * W + slack,), torch.int32), depth=((F * H * W + slack,), F64), image=((F * H * W * 3 + slack,), torch.uint8))
    buf = {k: torch.full(s, 77 if d == torch.uint8 else -77, device="cuda", dtype=d) for k, (s, d) in shapes.items() if k in want}
    arr = lambda x: None if x is None else (C.c_double * 3)(*x)
    raw = lambda x: None if x is None else x.data_ptr()
    eng.call("nm_mesh_draw", rec.data_ptr(), rect.data_ptr(), toff.data_ptr(), t.data_ptr(), raw(c), arr(color), F, V, M, C.byref(cs), light[0], light[1],
             arr(background), cap, lst.data_ptr(), *[raw(buf.get(k)) for k in ("index", "depth", "image")])
    torch.cuda.synchronize()
    n = dict(index=F * H * W, depth=F * H * W, image=F * H * W * 3)
    for k, b in buf.items():
        assert (b[n[k]:] == (77 if k == "image" else -77)).all(), f"{k} written past its end"
    assert (lst[cap:] == -77).all(), "list written past the capacity"
    assert int(toff[nt].item()) == total
    out = {k: _np(b[:n[k]]) for k, b in buf.items()}
    out.update(total=total, tile_offsets=_np(toff[:nt + 1]), list=_np(lst[:cap]), rect=_np(rect[:F * M]), rec=_np(rec[:F * M]))
    return out


W0, H0, FOC, CX0, CY0 = 40, 33, 45.0, 19.5, 16.0


@functools.lru_cache(maxsize=None)
def _scene():
    """F = 3 frames of 400 triangles, the middle frame wholly behind the camera; vertex colours with NaN rows and rows outside [0, 1]"""
    E = RR.rigid((0.3, -0.4, 0.2), (0.1, -0.2, 0.4))
    cam = PinholeCamera(E.tolist(), FOC, FOC, CX0, CY0, W0, H0)
    v0, tri = MR.soup(400, 3, E, FOC, FOC, CX0, CY0, W0, H0)
    va, ta = MR.soup(400, 103, E, FOC, FOC, CX0, CY0, W0, H0)
    v2 = np.empty_like(v0)
    v2[tri.reshape(-1)] = va[ta.reshape(-1)]                                   # another soup under the same triangle rows
    behind = MR.to_camera(v0, cam) * np.array([1.0, 1.0, -1.0])
    vertices = np.stack([v0, MR.to_world(behind, E), v2])
    colors = RR.palette(len(v0), 5)
    colors[::7] = np.random.default_rng(6).uniform(-0.5, 1.5, colors[::7].shape)
    seen = np.unique(MR.render_mesh(vertices, tri, cam)["index"])[1:]
    assert len(seen) > 100
    colors[tri[seen[3], 0]] = np.nan                                           # two triangles on screen have a NaN colour at a vertex
    colors[tri[seen[-2], 1], 1] = np.nan
    flat = MR.render_mesh(vertices, tri, cam, vertex_colors=colors, light=(1.0, 0.0), background=BG)
    lit = MR.render_mesh(vertices, tri, cam, vertex_colors=colors, light=(0.3, 0.7), background=BG)
    return cam, vertices, tri, colors, flat, lit


def test_soup_over_partial_tiles_and_a_frame_behind_the_camera():
    net = _net()
    cam, vertices, tri, colors, flat, lit = _scene()
    p = MR.to_camera(vertices[0], cam)[tri]                                    # (M, 3, 3)
    u, v = cam.cx + cam.fx * p[..., 0] / p[..., 2], cam.cy + cam.fy * p[..., 1] / p[..., 2]
    for name, lo, hi in (("left", u.min(1) < 0, u.max(1) > 0), ("right", u.min(1) < W0 - 1, u.max(1) > W0 - 1), ("top", v.min(1) < 0, v.max(1) > 0),
                         ("bottom", v.min(1) < H0 - 1, v.max(1) > H0 - 1)):
        assert (lo & hi).sum() >= 5, f"the scene has no triangles across the {name} edge"
    assert ((u.max(1) < -2) | (u.min(1) > W0 + 2)).sum() >= 20, "the scene has no triangles outside the image"
    assert (flat["index"][1] == -1).all() and (flat["index"][0] >= 0).sum() > 300 and (flat["index"][2] >= 0).sum() > 300
    a = _abi(net, vertices, tri, cam, vertex_colors=colors, background=BG)
    _compare(a, flat, "abi, flat light")
    assert (a["image"].reshape(3, H0, W0, 3)[1] == np.array([63, 127, 255], np.uint8)).all()          # the frame behind the camera: background only
    nt, M = 3 * 3, len(tri)
    assert (np.diff(a["tile_offsets"]) >= 0).all() and (np.diff(a["tile_offsets"])[nt:2 * nt] == 0).all() and a["tile_offsets"][-1] == a["total"]
    assert (a["rect"][M:2 * M, 0] > a["rect"][M:2 * M, 1]).all() and (a["rec"][M:2 * M] == 0).all()
    for t in range(3 * nt):                                                    # every list holds records of its own frame only, each once
        rows = a["list"][a["tile_offsets"][t]:a["tile_offsets"][t + 1]]
        f = t // nt
        assert ((rows >= f * M) & (rows < (f + 1) * M)).all() and len(set(rows.tolist())) == len(rows), t
    b = _abi(net, vertices, tri, cam, vertex_colors=colors, light=(0.3, 0.7), background=BG)
    _compare(b, lit, "abi, light (0.3, 0.7)", lit=True)
    # one uniform colour; any subset of the outputs; NULL background is white, NULL colour the grey
    uni = MR.render_mesh(vertices, tri, cam, color=(0.9, 0.4, 0.2), light=(1.0, 0.0))
    _compare(_abi(net, vertices, tri, cam, color=(0.9, 0.4, 0.2)), uni, "abi, uniform colour")
    only = _abi(net, vertices, tri, cam, want=("depth",))
    _compare(only, flat, "abi, depth alone")
    grey = _abi(net, vertices, tri, cam, want=("image",))["image"].reshape(3, H0, W0, 3)
    assert (grey[1] == 255).all() and (grey[0][flat["index"][0] >= 0] == int(0.7 * 255.0)).all()


@pytest.mark.parametrize("which", ["icosphere", "torus"])
def test_closed_meshes_and_run_to_run_identity(which):
    net = _net()
    E = RR.rigid((0.3, -0.4, 0.2), (0.1, -0.2, 0.4))
    cam = PinholeCamera(E.tolist(), FOC, FOC, CX0, CY0, W0, H0)
    verts, tri = MR.icosphere(2) if which == "icosphere" else MR.torus()
    assert len(tri) == 320
    poses = ((0.4, 0.7, -0.2), (1.25, 0.3, 0.2))
    vertices = np.stack([MR.posed(verts, E, ang, (0.05, -0.02, 3.0), 0.9 if which == "icosphere" else 0.75) for ang in poses])
    colors = RR.palette(len(verts), 8)
    flat = MR.render_mesh(vertices, tri, cam, vertex_colors=colors, light=(1.0, 0.0), background=BG, stats=True)
    lit = MR.render_mesh(vertices, tri, cam, vertex_colors=colors, background=BG)
    assert ((flat["cover"] > 0) == (flat["index"] >= 0)).all() and (flat["cover"][~flat["edge0"]] % 2 == 0).all()
    _compare(_abi(net, vertices, tri, cam, vertex_colors=colors, background=BG), flat, f"{which}, abi")
    v, t, c = _dev(vertices, np.float64), _dev(tri, np.int32), _dev(colors, np.float64)
    kw = dict(vertex_colors=c, background=BG, return_index=True, return_depth=True)
    a = net.render_mesh(v, t, cam, light=(1.0, 0.0), **kw)
    assert set(a) == {"image", "bin_total", "index", "depth"} and tuple(a["image"].shape) == (2, H0, W0, 3) and a["image"].dtype == torch.uint8
    assert tuple(a["index"].shape) == (2, H0, W0) and a["index"].dtype == torch.int32 and a["depth"].dtype == F64
    _compare(a, flat, f"{which}, render_mesh")
    l1, l2 = net.render_mesh(v, t, cam, **kw), net.render_mesh(v, t, cam, **kw)      # the default light (0.3, 0.7)
    _compare(l1, lit, f"{which}, render_mesh lit", lit=True)
    for k in l1:
        assert torch.equal(l1[k], l2[k]), f"{k} differs between two runs"
    plain = net.render_mesh(v, t, cam)
    assert set(plain) == {"image", "bin_total"}
    empty = net.render_mesh(v, torch.zeros(0, 3, device="cuda", dtype=torch.int32), cam, return_index=True, return_depth=True)
    assert int(empty["bin_total"]) == 0 and (empty["index"] == -1).all() and torch.isinf(empty["depth"]).all() and (empty["image"] == 255).all()


def _degenerates():
    """identity extrinsic.  rows 0 / 1 one triangle twice (the lower row wins), 2 a farther one partly hidden by them, 3 of zero area
    (collinear: n = 0 exactly), 4 with a NaN vertex, 5 straddling near (one vertex behind the camera: culled whole), 6 edge-on (its plane
    holds the camera: q = 0 and every X_k = 1 / 8 exactly), 7 with an index of -1, 8 with an index of V"""
    v = np.array([[-0.6, -0.5, 2.0], [0.7, -0.4, 2.2], [0.1, 0.6, 1.8],                 # 0 1 2
                  [-0.9, -0.8, 3.0], [0.9, -0.7, 3.0], [0.0, 0.9, 3.0],                 # 3 4 5
                  [0.0, 0.0, 1.5], [0.1, 0.0, 1.5], [0.2, 0.0, 1.5],                    # 6 7 8: collinear
                  [np.nan, 0.0, 2.0],                                                   # 9
                  [0.3, 0.3, -1.0],                                                     # 10: behind
                  [0.125, -0.5, 1.0], [0.25, 0.5, 2.0], [0.375, 0.0, 3.0]])             # 11 12 13: on the plane x = z / 8, exactly
    tri = np.array([[0, 1, 2], [1, 2, 0], [3, 4, 5], [6, 7, 8], [0, 1, 9], [0, 1, 10], [11, 12, 13], [0, -1, 2], [0, 1, len(v)]], np.int32)
    return v[None], tri


def test_degenerate_triangles():
    net = _net()
    cam = PinholeCamera(np.eye(4).tolist(), 40.0, 40.0, 24.0, 20.0, 48, 40)
    vertices, tri = _degenerates()
    colors = RR.palette(vertices.shape[1], 1)
    ref = MR.render_mesh(vertices, tri, cam, vertex_colors=colors, light=(1.0, 0.0))
    assert not MR.triangle_terms(vertices[0], tri, cam)["drawn"][[3, 4, 5, 7, 8]].any()
    a = _abi(net, vertices, tri, cam, vertex_colors=colors)
    _compare(a, ref, "degenerates")
    idx = a["index"].reshape(40, 48)
    assert set(np.unique(idx).tolist()) == {-1, 0, 2}
    assert (a["rect"][[3, 4, 5, 7, 8], 0] > a["rect"][[3, 4, 5, 7, 8], 1]).all(), "triangles that are not drawn have an empty rectangle"
    swapped = _abi(net, vertices, tri[[1, 0, 2, 3, 4, 5, 6, 7, 8]], cam, vertex_colors=colors)
    assert np.array_equal(swapped["index"], a["index"]) and np.array_equal(swapped["depth"], a["depth"])
    lit = MR.render_mesh(vertices, tri, cam, vertex_colors=colors)
    _compare(_abi(net, vertices, tri, cam, vertex_colors=colors, light=(0.3, 0.7)), lit, "degenerates, lit", lit=True)


def test_chunk_loop_on_a_single_tile():
    """one 16 x 16 image = one tile under 3 * NM_MESH_CHUNK = 384 triangles: the tile's list is longer than the 128 records the draw
    kernel stages in LDS at a time, so its chunk loop and barriers run three times (the last chunk partial or full as the culling
    leaves it)"""
    net = _net()
    E = RR.rigid((-0.2, 0.1, 0.5), (0.0, 0.1, 0.2))
    cam = PinholeCamera(E.tolist(), 20.0, 20.0, 7.5, 7.5, 16, 16)
    v, tri = MR.soup(3 * NM_MESH_CHUNK, 21, E, 20.0, 20.0, 7.5, 7.5, 16, 16, spill=1.1, size=0.25)
    colors = RR.palette(len(v), 22)
    ref = MR.render_mesh(v[None], tri, cam, vertex_colors=colors, light=(1.0, 0.0))
    a = _abi(net, v[None], tri, cam, vertex_colors=colors)
    assert a["total"] > 2 * NM_MESH_CHUNK, a["total"]
    assert len(np.unique(ref["index"])) > 40
    _compare(a, ref, "one tile, 384 triangles")


def test_bin_capacity():
    """the list capacity at exactly the true total, generous, and too small.  Too small: nothing is written past the capacity or the
    outputs' ends (the sentinels _abi checks), tile_offsets' last entry is still the true total, and the image is incomplete - each
    pixel shows the nearest of the triangles that made it into the lists, so it is never nearer than the full picture's"""
    net = _net()
    cam, vertices, tri, colors, flat, _ = _scene()
    total = _abi(net, vertices, tri, cam, vertex_colors=colors)["total"]
    for cap in (total, total + 1000):
        a = _abi(net, vertices, tri, cam, vertex_colors=colors, background=BG, capacity=cap)
        assert a["total"] == total
        _compare(a, flat, f"capacity {cap}")
    for cap in (total // 2, 1, 0):
        a = _abi(net, vertices, tri, cam, vertex_colors=colors, capacity=cap)
        assert a["total"] == total and a["tile_offsets"][-1] == total
        d, i = a["depth"].reshape(flat["depth"].shape), a["index"].reshape(flat["index"].shape)
        assert (d >= flat["depth"]).all() and ((i == flat["index"]) | (d > flat["depth"])).all()
        assert (i >= -1).all() and (i < len(tri)).all()
    assert (i == -1).all()                                                       # capacity 0: background only
    v, t, c = _dev(vertices, np.float64), _dev(tri, np.int32), _dev(colors, np.float64)
    kw = dict(vertex_colors=c, light=(1.0, 0.0), background=BG, return_index=True, return_depth=True)
    _compare(net.render_mesh(v, t, cam, bin_capacity=total, **kw), flat, "render_mesh, exact bin_capacity")
    big = net.render_mesh(v, t, cam, bin_capacity=total + 4096, **kw)
    _compare(big, flat, "render_mesh, generous bin_capacity")
    small = net.render_mesh(v, t, cam, bin_capacity=total // 3, **kw)
    assert int(small["bin_total"]) == int(big["bin_total"]) == total
    assert "INCOMPLETE" in NeuralMarionette.render_mesh.__doc__


def test_frame_grouping_does_not_change_the_result():
    net = _net()
    cam, vertices, tri, colors, flat, _ = _scene()
    v, t, c = _dev(vertices, np.float64), _dev(tri, np.int32), _dev(colors, np.float64)
    kw = dict(vertex_colors=c, light=(1.0, 0.0), background=BG, return_index=True, return_depth=True)
    whole = net.render_mesh(v, t, cam, **kw)
    for bound in (144 * len(tri), 2 * 144 * len(tri), 1):                        # one frame a group, two and one, a bound below one frame
        parts = net.render_mesh(v, t, cam, record_bytes=bound, **kw)
        assert set(parts) == set(whole)
        for k in whole:
            assert torch.equal(parts[k], whole[k]), (k, bound)
    _compare(whole, flat, "render_mesh, all frames at once")


def _compare_skeleton(got, ref, what):
    got = {k: (_np(v) if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    shape = ref["index"].shape
    idx, dep, img = got["index"].reshape(shape), got["depth"].reshape(shape), got["image"].reshape(shape + (3,))
    covered, ties = ref["index"] >= 0, MR.near_ties(ref)
    assert ties.sum() <= MR.SKEL_TIE_CAP * covered.sum()
    assert np.array_equal(idx >= 0, covered), f"{what}: coverage differs on {int(((idx >= 0) != covered).sum())} pixels"
    bad = int((idx != ref["index"])[~ties].sum())
    either = (idx == ref["index"]) | ties
    ulp = np.abs(dep[covered] - ref["depth"][covered]) / np.spacing(ref["depth"][covered])
    same = idx == ref["index"]
    err = int(np.abs(img.astype(np.int32) - ref["image"].astype(np.int32))[same].max(initial=0))
    print(f"{what}: {int(covered.sum())} covered pixels, {int(ties.sum())} near ties, index differs on {bad} others, depth within {ulp[~ties[covered]].max(initial=0):.1f} ulp, "
          f"image within {err} levels")
    assert either.all(), f"{what}: index differs on {bad} pixels that are no near ties"
    assert np.isinf(dep[~covered]).all() and (dep[~covered] > 0).all()
    assert (ulp[~ties[covered]] <= 4.0).all() and (ulp <= 4.0 + 1e-12 / np.finfo(np.float64).eps).all()
    assert err <= 1


def _abi_skeleton(net, s, over=None, light=(0.3, 0.7), slack=8):
    eng = net._engine
    eng.ready()
    cam, kp = s["cam"], s["keypoints"]
    F, K = kp.shape[:2]
    H, W = cam.height, cam.width
    n = dict(index=F * H * W, depth=F * H * W, image=F * H * W * 3)
    buf = dict(index=torch.full((n["index"] + slack,), -77, device="cuda", dtype=torch.int32), depth=torch.full((n["depth"] + slack,), -77.0, device="cuda", dtype=F64),
               image=torch.full((n["image"] + slack,), 77, device="cuda", dtype=torch.uint8))
    if over is not None:
        buf["image"][:n["image"]] = _dev(over, np.uint8).reshape(-1)
    k, p, jc = _dev(kp, np.float32), _dev(s["parents"], np.int32), _dev(s["colors"], np.float64)
    kw = s["kw"]
    arr = lambda x: (C.c_double * 3)(*x)
    cs = cam.c_struct()
    eng.call("nm_skeleton_draw", k.data_ptr(), p.data_ptr(), F, K, C.byref(cs), 0.2, kw["radius"], kw["bone_radius"], jc.data_ptr(), None, arr(kw["bone_color"]),
             light[0], light[1], arr(kw["background"]), int(over is not None), buf["index"].data_ptr(), buf["depth"].data_ptr(), buf["image"].data_ptr())
    torch.cuda.synchronize()
    for name, b in buf.items():
        assert (b[n[name]:] == (77 if name == "image" else -77)).all(), f"{name} written past its end"
    return {name: _np(b[:n[name]]) for name, b in buf.items()}


@pytest.mark.parametrize("shape", [(40, 33, 55.0, MR.SKEL_RADIUS, MR.SKEL_BONE), (16, 16, 22.0, 0.3, 0.2)], ids=["40x33", "one tile"])
def test_skeleton(shape):
    net = _net()
    s = MR.skeleton_scene(*shape)
    _compare_skeleton(_abi_skeleton(net, s), s["ref"], "skeleton, abi")
    pasted = _abi_skeleton(net, s, over=s["over"])
    _compare_skeleton(pasted, s["pasted"], "skeleton over an image, abi")
    covered = s["ref"]["index"] >= 0
    assert np.array_equal(pasted["image"].reshape(s["over"].shape)[~covered], s["over"][~covered])
    kp, over = _dev(s["keypoints"], np.float32), _dev(s["over"], np.uint8)
    kw = dict(s["kw"], joint_colors=torch.from_numpy(s["colors"]), return_index=True, return_depth=True)
    a = net.render_skeleton(kp, s["parents"], s["cam"], **kw)
    assert set(a) == {"image", "index", "depth"} and tuple(a["image"].shape) == s["over"].shape and a["image"].dtype == torch.uint8
    _compare_skeleton(a, s["ref"], "render_skeleton")
    keep = over.clone()
    b = net.render_skeleton(kp[None], torch.from_numpy(s["parents"]), s["cam"], over=over, **kw)
    assert torch.equal(over, keep), "the image to paste over was modified"
    _compare_skeleton(b, s["pasted"], "render_skeleton over an image")
    off = torch.from_numpy(~covered).cuda()
    assert torch.equal(b["image"][off], over[off])
    again = net.render_skeleton(kp, s["parents"], s["cam"], **kw)
    for k in a:
        assert torch.equal(a[k], again[k]), f"{k} differs between two runs"
    # one colour for every joint
    uni = MR.render_skeleton(s["keypoints"], s["parents"], s["cam"], radius=shape[3], bone_radius=shape[4])
    one = net.render_skeleton(kp, s["parents"], s["cam"], radius=shape[3], bone_radius=shape[4], return_index=True, return_depth=True)
    _compare_skeleton(one, uni, "render_skeleton, default colours")


def test_render_retarget_end_to_end(golden_dir):
    """sample_retarget at G = 32 with the synthetic weights, noise and teacher forcing of tests/test_retarget_gpu.py, the target points
    being the vertices of a procedural torus, then render_retarget - compared against the restatement fed with the device's own points,
    keypoints and vertex colours: the mesh as in the soup test, the skeletons as in test_skeleton, and the overlay equal to the
    restatement's composition of the two device images"""
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
    T = int(result["points"].shape[0])
    E = RR.rigid((0.2, -0.3, 0.1), (0.0, 0.0, 3.0))
    cam = PinholeCamera(E.tolist(), 60.0, 60.0, 31.5, 23.5, 64, 48)
    t = _dev(tri, np.int32)
    jc = torch.from_numpy(RR.palette(K, 12)).cuda()
    rk = dict(radius=0.1, bone_radius=0.07)                                      # (the script's 0.03 is half a pixel at this size)
    out = net.render_retarget(result, t, cam, skin_colors=True, joint_colors=jc, **rk)
    assert set(out) == {"mesh", "skeleton", "source_skeleton", "overlay"}
    for k in out:
        assert tuple(out[k].shape) == (T, 48, 64, 3) and out[k].dtype == torch.uint8, k
    points = _np(result["points"])
    vc = (result["skin_weights"].double() @ jc).contiguous()
    lit = MR.render_mesh(points, tri, cam, vertex_colors=_np(vc))
    assert (lit["index"] >= 0).sum() > 100 * T
    _compare(dict(image=out["mesh"]), lit, "render_retarget, mesh", lit=True)
    flat = MR.render_mesh(points, tri, cam, vertex_colors=_np(vc), light=(1.0, 0.0))
    _compare(net.render_mesh(result["points"], t, cam, vertex_colors=vc, light=(1.0, 0.0), return_index=True, return_depth=True), flat, "the posed torus, flat")
    parents = _np(net.dyna_module.parents)
    shown = {}
    for key, name in (("keypoints", "skeleton"), ("source_keypoints", "source_skeleton")):
        kp = _np(result[key][0])
        ref = MR.render_skeleton(kp, parents, cam, **rk)
        assert (ref["index"] >= 0).sum() > 20 * T, name
        got = net.render_skeleton(result[key], parents, cam, return_index=True, return_depth=True, **rk)
        _compare_skeleton(got, ref, f"render_retarget, {name}")
        assert torch.equal(got["image"], out[name]), name
        shown[name] = got
    on = shown["skeleton"]["index"] >= 0
    want = torch.where(on[..., None], out["skeleton"], out["mesh"])
    assert torch.equal(out["overlay"], want) and on.any() and not on.all()
    plain = net.render_retarget(result, t, cam, **rk)
    assert torch.equal(plain["skeleton"], out["skeleton"]) and torch.equal(plain["overlay"][on], out["overlay"][on])
    _compare(dict(image=plain["mesh"]), MR.render_mesh(points, tri, cam), "render_retarget, grey mesh", lit=True)


def test_arguments_are_judged_before_any_launch():
    net = _net()
    eng = net._engine
    eng.ready()
    lib, h = eng.ctx.lib, eng.ctx.handle
    good = PinholeCamera(np.eye(4).tolist(), 40.0, 40.0, 24.0, 20.0, 48, 40)

    def cam(**kw):
        c = good.c_struct()
        for k, val in kw.items():
            if k == "e0":
                c.extrinsic[0] = val
            else:
                setattr(c, k, val)
        return C.byref(c)

    nan, inf = float("nan"), float("inf")
    ARG, UNS = _lib.NM_ERR_ARG, _lib.NM_ERR_UNSUPPORTED
    cams = [(dict(width=0), ARG), (dict(height=0), ARG), (dict(fx=nan), ARG), (dict(fy=inf), ARG), (dict(fx=0.0), ARG), (dict(cx=nan), ARG),
            (dict(cy=-inf), ARG), (dict(near=nan), ARG), (dict(near=0.0), ARG), (dict(e0=nan), ARG), (dict(width=65536, height=32768), UNS)]
    # nm_mesh_bin(ctx, vertices, triangles, F, V, M, camera, rec, rect, tile_offsets): pointers that are never used
    ok = [1, 1, 1, 5, 4, cam(), 1, 1, 1]
    cases = [(0, None, ARG), (1, None, ARG), (2, 0, ARG), (3, 0, ARG), (4, -1, ARG), (4, 2 ** 31, UNS), (5, None, ARG), (6, None, ARG), (7, None, ARG),
             (8, None, ARG)] + [(5, cam(**kw), code) for kw, code in cams]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_mesh_bin(h, *args) == code, ("bin", pos, val)
    assert lib.nm_mesh_bin(None, *ok) == ARG
    assert b"mesh_bin" in lib.nm_last_error()
    two = list(ok)
    two[2], two[4] = 2, 2 ** 30                                                  # F M = 2^31
    assert lib.nm_mesh_bin(h, *two) == UNS
    # nm_mesh_draw(ctx, rec, rect, tile_offsets, triangles, vertex_colors, color, F, V, M, camera, light_a, light_b, background, capacity, list, index, depth, image)
    ok = [1, 1, 1, 1, 1, None, 1, 5, 4, cam(), 1.0, 0.0, None, 8, 1, 1, 1, 1]
    cases = [(0, None, ARG), (1, None, ARG), (2, None, ARG), (3, None, ARG), (6, 0, ARG), (7, 0, ARG), (8, -1, ARG), (8, 2 ** 31, UNS), (9, None, ARG),
             (13, -1, ARG), (14, None, ARG)] + [(9, cam(**kw), code) for kw, code in cams]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_mesh_draw(h, *args) == code, ("draw", pos, val)
    assert lib.nm_mesh_draw(None, *ok) == ARG
    nothing = list(ok)
    nothing[15] = nothing[16] = nothing[17] = None                               # every output NULL: nothing to do, nothing launched
    assert lib.nm_mesh_draw(h, *nothing) == 0
    # nm_skeleton_draw(ctx, keypoints, parents, F, K, camera, threshold, radius, bone_radius, joint_colors, joint_color, bone_color, light_a, light_b,
    #                  background, overlay, index, depth, image)
    ok = [1, 1, 1, 6, cam(), 0.2, 0.03, 0.03, None, None, None, 0.3, 0.7, None, 0, 1, 1, 1]
    cases = [(0, None, ARG), (1, None, ARG), (2, 0, ARG), (3, 0, ARG), (3, 33, ARG), (4, None, ARG), (6, 0.0, ARG), (6, nan, ARG), (6, inf, ARG), (7, -1.0, ARG),
             (7, nan, ARG)] + [(4, cam(**kw), code) for kw, code in cams]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_skeleton_draw(h, *args) == code, ("skeleton", pos, val)
    assert lib.nm_skeleton_draw(None, *ok) == ARG
    assert b"skeleton_draw" in lib.nm_last_error()
    nothing = list(ok)
    nothing[15] = nothing[16] = nothing[17] = None
    assert lib.nm_skeleton_draw(h, *nothing) == 0
    # the shells, with tensors on the device
    cam0, vertices, tri, colors, _, _ = _scene()
    v, t = _dev(vertices, np.float64), _dev(tri, np.int32)
    with pytest.raises(ValueError, match="device"):
        net.render_mesh(v, t.cpu(), cam0)
    with pytest.raises(ValueError, match="vertex_colors"):
        net.render_mesh(v, t, cam0, vertex_colors=_dev(colors[:-1], np.float64))
    with pytest.raises(ValueError, match="contiguous"):
        net.render_mesh(v.transpose(0, 1).contiguous().transpose(0, 1), t, cam0)
    with pytest.raises(ValueError, match="device"):
        net.render_skeleton(torch.zeros(1, 6, 4), [0] * 6, cam0)
