"""tests/mesh_ref.py - the float64 restatement of the mesh and skeleton render contract of include/nm355.h - pinned independently of the
library: hand-derived pixels, world-space ray casters written the other way round (Moeller-Trumbore for the triangles, the textbook
sphere and cone quadratics with sqrt for the skeleton), the no-cracks property of closed meshes, the exact
antisymmetry of the edge functions it rests on, and the argument checks of the three methods that precede any device call."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as MR
import render_ref as RR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, PinholeCamera


def _cam(W=11, H=11, focal=10.0, E=None, near=1e-3):
    E = np.eye(4) if E is None else E
    return PinholeCamera(E.tolist(), focal, focal, W / 2 - 0.5, H / 2 - 0.5, W, H, near)


def test_one_triangle_by_hand():
    """identity camera, fx = fy = 10, cx = cy = 5: pixel (px, py) looks along ((px - 5) / 10, (py - 5) / 10, 1).  The triangle
    (-1,-1,2), (1,-1,2), (0,1,2) projects to (-.5,-.5), (.5,-.5), (0,.5); n = (2,0,0) x (1,2,0) = (0,0,4), q = 8, so s = 2 wherever it is
    covered.  At the middle pixel w = (.25, .25, .5), iz = .5 each: l = (.125, .125, .25), L = .5, colour (.25, .25, .5)."""
    cam = _cam()
    v = np.array([[[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0]]])
    tri = np.array([[0, 1, 2]], np.int32)
    vc = np.eye(3)
    out = MR.render_mesh(v, tri, cam, vertex_colors=vc, light=(1.0, 0.0), background=(0.0, 0.0, 0.0))
    idx, dep, img = out["index"][0], out["depth"][0], out["image"][0]
    assert idx[5, 5] == 0 and dep[5, 5] == 2.0 and img[5, 5].tolist() == [63, 63, 127]
    assert idx[0, 0] == 0 and dep[0, 0] == 2.0 and img[0, 0].tolist() == [255, 0, 0]          # exactly on vertex 0: two edge functions are 0
    assert idx[0, 10] == 0 and img[0, 10].tolist() == [0, 255, 0]
    assert idx[10, 5] == 0 and img[10, 5].tolist() == [0, 0, 255]
    assert idx[10, 0] == -1 and np.isinf(dep[10, 0]) and img[10, 0].tolist() == [0, 0, 0]
    # row py: covered for |px - 5| < (10 - py) / 2, not for >; pixels exactly on a slanted edge depend on the rounding of tenths
    for py in range(11):
        got = set(np.nonzero(idx[py] == 0)[0].tolist())
        assert {px for px in range(11) if abs(px - 5) * 2 < 10 - py} <= got <= {px for px in range(11) if abs(px - 5) * 2 <= 10 - py}, py
    # the headlight: the face looks straight at the camera, |den| / (|n| sqrt(A)) = 1 / sqrt(A)
    lit = MR.render_mesh(v, tri, cam, color=(1.0, 0.5, 0.25), light=(0.25, 0.5), background=(0.0, 0.0, 0.0))["image"][0]
    assert lit[5, 5].tolist() == [int(0.75 * 255), int(0.375 * 255), int(0.1875 * 255)]
    a = 0.25 + 0.5 / np.sqrt(1.0 + 0.2 * 0.2)
    assert lit[5, 7].tolist() == [int(a * 255.0), int(0.5 * a * 255.0), int(0.25 * a * 255.0)]
    # the other winding is as visible; a vertex in front of near culls the whole triangle
    assert np.array_equal(MR.render_mesh(v, tri[:, ::-1], cam)["index"], out["index"])
    assert (MR.render_mesh(v, tri, _cam(near=2.5))["index"] == -1).all()
    v2 = v.copy()
    v2[0, 2, 2] = 1e-4
    assert (MR.render_mesh(v2, tri, cam)["index"] == -1).all()


def test_one_sphere_and_one_bone_by_hand():
    """a sphere of radius 1 about (0,0,3): at the middle pixel A = 1, B = 3, C = 8, D = 1, s = 8 / (3 + 1) = 2, the normal (0,0,-1) faces
    the camera; at dx = .5 D = 9 - 1.25 * 8 < 0.  A bone from (0,-1,4) to (0,1,4) of radius .5 seen side-on: its silhouette in the plane
    z = 4 is the kite with corners (0,-1), (+-.5,-.6), (0,1), and on its axis the ray meets it at z = 4 - (the radius there)."""
    cam = _cam()
    kp = np.array([[[0.0, 0.0, 3.0, 1.0]]], np.float32)
    out = MR.render_skeleton(kp, [0], cam, radius=1.0, joint_colors=(1.0, 0.5, 0.0), light=(0.25, 0.5), background=(0.0, 0.0, 0.0))
    assert out["index"][0, 5, 5] == 0 and out["depth"][0, 5, 5] == 2.0 and out["image"][0, 5, 5].tolist() == [int(0.75 * 255), int(0.375 * 255), 0]
    assert out["index"][0, 5, 10] == -1 and out["index"][0, 5, 8] == 0
    inside = (np.hypot(*np.meshgrid(np.arange(11) - 5.0, np.arange(11) - 5.0)) / 10.0) ** 2 * 8.0 <= 1.0      # tan^2 <= 1 / 8
    assert np.array_equal(out["index"][0] == 0, inside)
    assert (MR.render_skeleton(kp, [0], cam, radius=1.0, threshold=1.5)["index"] == -1).all()
    cam = _cam(41, 41, 40.0)
    kp = np.array([[[0.0, -1.0, 4.0, 1.0], [0.0, 1.0, 4.0, 1.0]]], np.float32)
    bone = MR.render_skeleton(kp, [0, 0], cam, radius=1e-3, bone_radius=0.5)
    idx, dep = bone["index"][0], bone["depth"][0]
    assert set(np.unique(idx).tolist()) <= {-1, 0, 1, 3} and (idx == 3).sum() > 100
    for py in range(41):
        y = (py - 20) / 40.0 * 4.0                                              # the axis point the middle ray of this row passes
        r = 0.5 * (y + 1.0) / 0.4 if y <= -0.6 else 0.5 * (1.0 - y) / 1.6
        if -1.0 < y < 1.0 and abs(y + 0.6) > 0.05 and r > 0.05:
            assert idx[py, 20] == 3, py
            # the ray (0, dy, 1) s meets the cone near z = 4 - r(y'), y' = dy s: solve the fixed point in two steps
            s = 4.0 - r
            for _ in range(60):
                yy = (py - 20) / 40.0 * s
                s = 4.0 - (0.5 * (yy + 1.0) / 0.4 if yy <= -0.6 else 0.5 * (1.0 - yy) / 1.6)
            assert abs(dep[py, 20] - s) < 1e-9, (py, dep[py, 20], s)
    # silhouette: in the plane z = 4 the kite, |x| <= r(y) (the cone bulges towards the camera, which only widens it by O(r^2 / z))
    x, y = np.meshgrid((np.arange(41) - 20) / 40.0 * 4.0, (np.arange(41) - 20) / 40.0 * 4.0)
    r = np.where(y <= -0.6, 0.5 * (y + 1.0) / 0.4, 0.5 * (1.0 - y) / 1.6)
    sure_in, sure_out = (np.abs(x) < r - 0.12) & (r > 0), (np.abs(x) > r * 1.2 + 0.12) | (y < -1.2) | (y > 1.2)
    assert (idx[sure_in] == 3).all() and (idx[sure_out] != 3).all()


def _moller_trumbore(vertices, tri, cam):
    """index and depth by a ray caster in WORLD space: origin o = -R^T t, direction R^T d, Moeller-Trumbore per triangle, depth = the
    ray parameter (d_z = 1 in camera space, so it is the camera's z).  No projection, no edge functions."""
    E = RR.extrinsic(cam)
    R, t = E[:3, :3], E[:3, 3]
    o = -R.T @ t
    dx, dy = RR.pixel_rays(cam)
    d = np.stack([dx, dy, np.ones_like(dx)], -1) @ R                           # R^T d per pixel
    index = np.full(dx.shape, -1, np.int32)
    depth = np.full(dx.shape, np.inf)
    margin = np.full(dx.shape, np.inf)
    with np.errstate(all="ignore"):
        for i, (a, b, c) in enumerate(tri):
            p0, e1, e2 = vertices[a], vertices[b] - vertices[a], vertices[c] - vertices[a]
            pv = np.cross(d, e2)
            det = pv @ e1
            tv = o - p0
            u = (pv @ tv) / det
            qv = np.cross(tv, e1)
            v = (d @ qv) / det
            s = (qv @ e2) / det
            # how far the barycentrics are from an edge, in pixels: their gradient across one pixel is about 1 / (the triangle's size in pixels)
            margin = np.minimum(margin, np.where(s > 0, np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1.0 - u - v)), np.inf))
            hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (s >= cam.near) & (s < depth)
            depth[hit] = s[hit]
            index[hit] = i
    return index, depth, margin


@functools.lru_cache(maxsize=None)
def _closed(which):
    E = RR.rigid((0.3, -0.4, 0.2), (0.1, -0.2, 0.4))
    cam = PinholeCamera(E.tolist(), 45.0, 45.0, 19.5, 16.0, 40, 33)
    verts, tri = MR.icosphere(2) if which == "icosphere" else MR.torus()
    v = MR.posed(verts, E, (0.4, 0.7, -0.2) if which == "icosphere" else (1.25, 0.3, 0.2), (0.05, -0.02, 3.0), 0.9 if which == "icosphere" else 0.75)
    return cam, v, tri, MR.render_mesh(v[None], tri, cam, stats=True)


@pytest.mark.parametrize("which", ["icosphere", "torus"])
def test_world_space_ray_caster_agrees_away_from_edges(which):
    cam, v, tri, ref = _closed(which)
    index, depth, margin = _moller_trumbore(v, tri, cam)
    sure = margin > 1e-9
    covered = ref["index"][0] >= 0
    print(f"{which}: {int(covered.sum())} covered pixels, {int((~sure).sum())} within 1e-9 of an edge")
    assert covered.sum() > 300 and sure.mean() > 0.99
    assert np.array_equal(index[sure], ref["index"][0][sure])
    both = sure & covered
    assert np.abs(depth[both] - ref["depth"][0][both]).max() < 1e-12 * 4.0


@pytest.mark.parametrize("which", ["icosphere", "torus"])
def test_closed_meshes_have_no_cracks(which):
    """a closed surface wholly in front of the camera: every ray crosses it an even number of times, so every pixel where no edge
    function is exactly 0 (a pixel ON an edge belongs to both triangles) is covered by an even number of triangles - in particular no
    pixel inside the silhouette is covered by none, which is what a crack along a shared edge would be"""
    cam, v, tri, ref = _closed(which)
    assert len(tri) == 320
    clean = ~ref["edge0"][0]
    cover = ref["cover"][0]
    assert clean.mean() > 0.95 and (cover[clean] % 2 == 0).all()
    assert (cover[clean] > 0).sum() > 300 and ((cover > 0) == (ref["index"][0] >= 0)).all()
    if which == "icosphere":
        assert set(np.unique(cover[clean]).tolist()) == {0, 2}                   # convex: in and out
    else:
        assert 4 in np.unique(cover[clean])                                      # the torus is seen through its own ring somewhere


def test_shared_edge_antisymmetry_on_random_inputs():
    """fl(a * b) = fl(b * a) and fl(x - y) = -fl(y - x): the edge function of (P, Q) is exactly minus that of (Q, P), for any inputs"""
    rng = np.random.default_rng(0)
    for scale in (1.0, 1e-8, 1e8):
        P, Q, d = (rng.standard_normal((2, 100000)) * scale for _ in range(3))
        d = d * rng.choice([1.0, 1e-3], d.shape)
        w_pq = (P[0] - d[0]) * (Q[1] - d[1]) - (P[1] - d[1]) * (Q[0] - d[0])
        w_qp = (Q[0] - d[0]) * (P[1] - d[1]) - (Q[1] - d[1]) * (P[0] - d[0])
        assert np.array_equal(w_pq, -w_qp)
    # and through the restatement: a quad split along its diagonal, either triangle first, covers every pixel inside exactly once or,
    # on the diagonal, twice
    cam = _cam(33, 33, 30.0)
    v = np.array([[[-0.9, -0.8, 2.0], [0.8, -0.9, 2.5], [0.9, 0.8, 2.2], [-0.8, 0.9, 1.9]]])
    tri = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    out = MR.render_mesh(v, tri, cam, stats=True)
    one = MR.render_mesh(v, np.array([[0, 1, 2], [2, 0, 3]], np.int32), cam, stats=True)
    assert np.array_equal(out["cover"], one["cover"]) and np.array_equal(out["index"], one["index"])
    quad = MR.render_mesh(v, np.array([[0, 1, 3], [1, 2, 3]], np.int32), cam, stats=True)      # the other diagonal: the same silhouette
    assert np.array_equal(quad["cover"] > 0, out["cover"] > 0)


def _world_skeleton(keypoints, parents, cam, threshold, radius, bone_radius):
    """index and depth of one frame by a ray caster in WORLD space, written the other way round from mesh_ref: origin o = -R^T t,
    direction R^T d (unnormalised, so the ray parameter is the camera's z), the textbook sphere quadratic, and for a nappe the textbook
    cone (unit axis, cos^2 of the half-angle) whose two roots are computed WITH sqrt and kept if their axis parameter lies inside the
    height; a bone's depth is the first entry into its double cone.  No camera-space primitives, no square-root-free decisions."""
    E = RR.extrinsic(cam)
    R, t = E[:3, :3], E[:3, 3]
    o = -R.T @ t
    dx, dy = RR.pixel_rays(cam)
    D = np.stack([dx, dy, np.ones_like(dx)], -1) @ R
    kp = np.asarray(keypoints, np.float64)
    K = len(kp)
    c, alpha = kp[:, :3], np.clip(kp[:, 3], 0.0, 1.0)
    z = c @ R[2] + t[2]
    visible = alpha >= threshold
    index = np.full(dx.shape, -1, np.int32)
    depth = np.full(dx.shape, np.inf)
    DD = (D * D).sum(-1)

    def take(i, s):
        better = s < depth
        depth[better] = s[better]
        index[better] = i

    with np.errstate(all="ignore"):
        for k in range(K):
            if visible[k] and z[k] - radius >= cam.near:
                w = o - c[k]
                b, cc = D @ w, w @ w - radius ** 2
                disc = b * b - DD * cc
                s = (-b - np.sqrt(disc)) / DD
                take(k, np.where((disc >= 0) & (s > 0), s, np.inf))
        for k in range(K):
            q = int(parents[k])
            if not (visible[k] and visible[q] and q != k) or np.linalg.norm(c[k] - c[q]) == 0 or min(z[k], z[q]) - bone_radius < cam.near:
                continue
            g = c[q] + 0.2 * (c[k] - c[q])
            first = np.full(dx.shape, np.inf)
            for apex in (c[q], c[k]):
                h = np.linalg.norm(g - apex)
                axis = (g - apex) / h
                cos2 = h * h / (h * h + bone_radius ** 2)
                w = o - apex
                Du, wu = D @ axis, w @ axis
                a2, b2, c2 = Du * Du - cos2 * DD, Du * wu - cos2 * (D @ w), wu * wu - cos2 * (w @ w)
                root = np.sqrt(b2 * b2 - a2 * c2)
                for s in ((-b2 - root) / a2, (-b2 + root) / a2):
                    along = wu + s * Du
                    first = np.minimum(first, np.where((along >= 0) & (along <= h) & (s > 0), s, np.inf))
            take(K + k, first)
    return index, depth


def test_world_space_skeleton_caster_agrees_away_from_silhouettes():
    """the hand skeleton at 240 x 198 with spheres thinner than the bones (a bone is some 20 pixels across).  Compared on the pixels whose 3 x 3 neighbourhood has one index in
    the restatement (silhouettes and the seams between primitives move by rounding): index equal, depth to 1e-9.  And the branch the
    header singles out runs: on pixels a bone wins, rays steeper than its cone (c2 > 0) take the quadratic's FAR root."""
    s = MR.skeleton_scene(240, 198, 330.0, 0.04, MR.SKEL_BONE)                     # spheres thinner than the bones: the nappes about the joints show
    ref, cam, K = s["ref"], s["cam"], 6
    steep = 0
    for f in range(2):
        index, depth = _world_skeleton(s["keypoints"][f], s["parents"], cam, 0.2, 0.04, MR.SKEL_BONE)
        want = ref["index"][f]
        pad = np.pad(want, 1, mode="edge")
        sure = np.ones_like(want, bool)
        for oy in range(3):
            for ox in range(3):
                sure &= pad[oy:oy + want.shape[0], ox:ox + want.shape[1]] == want
        covered = want >= 0
        print(f"frame {f}: {int(covered.sum())} covered pixels, {int((covered & sure).sum())} of them compared, primitives {np.unique(want[covered]).tolist()}")
        assert (covered & sure).sum() > 0.5 * covered.sum()
        assert np.array_equal(index[sure], want[sure])
        assert np.abs(depth[sure & covered] - ref["depth"][f][sure & covered]).max() < 1e-9
        assert (np.bincount(want[covered & sure], minlength=2 * K) > 0).sum() >= 6          # most primitives have compared pixels
        dx, dy = RR.pixel_rays(cam)
        A = (dx * dx + dy * dy) + 1.0
        _, _, _, bones = MR.skeleton_primitives(s["keypoints"][f], s["parents"], cam, 0.2, MR.SKEL_RADIUS, MR.SKEL_BONE)
        for k, nappes in bones.items():
            won = sure & (want == K + k)
            for t in nappes:
                dv = (dx * t["v"][0] + dy * t["v"][1]) + t["v"][2]
                with np.errstate(all="ignore"):
                    hit, dep, _ = MR.nappe_hit(t, dx, dy, A)
                mine = won & hit & (dep == ref["depth"][f]) & ((t["kappa"] * dv) * dv - A > 0.0)
                steep += int(mine.sum())
    print(f"{steep} compared pixels are won through a ray steeper than the cone (c2 > 0)")
    assert steep > 50


def test_skeleton_scene_rules():
    s = MR.skeleton_scene(40, 33, 55.0)
    idx = s["ref"]["index"]
    assert set(np.unique(idx[0]).tolist()) == {-1, 0, 1, 2, 3, 5, 6 + 1, 6 + 2, 6 + 3}       # frame 0: no sphere 4, no bones of 4 and 5, none of the root
    assert set(np.unique(idx[1]).tolist()) <= {-1, 0, 1, 3, 4, 5, 6 + 1, 6 + 5} and 6 + 5 in idx[1] and 4 in idx[1]
    p, visible, spheres, bones = MR.skeleton_primitives(s["keypoints"][1], s["parents"], s["cam"], 0.2, MR.SKEL_RADIUS, MR.SKEL_BONE)
    assert visible.all() and not spheres[2] and sorted(bones) == [1, 5] and (p[1] == p[3]).all() and p[2, 2] < 0
    covered = idx >= 0
    assert np.array_equal(s["pasted"]["image"][~covered], s["over"][~covered]) and np.array_equal(s["pasted"]["image"][covered], s["ref"]["image"][covered])
    assert (s["ref"]["image"][~covered] == np.array([63, 127, 255], np.uint8)).all()
    one = MR.skeleton_scene(16, 16, 22.0, 0.3, 0.2)
    assert (one["ref"]["index"] >= 0).mean() > 0.05


def test_arguments_are_judged_before_the_context():
    net = NeuralMarionette(HotPathOptions(grid_size=32))                        # on the CPU: anything that reached the library would raise NmError
    cam = _cam(40, 33)
    v = torch.zeros(2, 5, 3, dtype=torch.float64)
    tri = torch.zeros(4, 3, dtype=torch.int32)
    bad_mesh = [("camera", dict(camera=None)), ("vertices", dict(vertices=v.float())), ("vertices", dict(vertices=v[0])), ("triangles", dict(triangles=tri.long())),
                ("triangles", dict(triangles=tri[:, :2])), ("vertex_colors", dict(vertex_colors=torch.zeros(4, 3, dtype=torch.float64))),
                ("color", dict(color=(1.0, 1.0))), ("light", dict(light=1.0)), ("background", dict(background=(1.0,))), ("bin_capacity", dict(bin_capacity=-1)),
                ("record_bytes", dict(record_bytes=0)), ("device", dict()), ("tensor", dict(vertices=np.zeros((2, 5, 3))))]
    for match, kw in bad_mesh:
        args = dict(vertices=v, triangles=tri, camera=cam)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            net.render_mesh(**args)
    with pytest.raises(ValueError, match="2\\^31"):
        net.render_mesh(v, tri, _cam(65536, 32768))
    kp = torch.zeros(2, 6, 4)
    par = [0, 0, 1, 1, 2, 4]
    bad_skel = [("camera", dict(camera=None)), ("keypoints", dict(keypoints=kp.double())), ("keypoints", dict(keypoints=torch.zeros(2, 33, 4))),
                ("keypoints", dict(keypoints=kp[..., :3])), ("parents", dict(parents=par[:5])), ("parents", dict(parents=[0.5] * 6)),
                ("radius", dict(radius=0.0)), ("bone_radius", dict(bone_radius=float("inf"))), ("radius", dict(radius="r")),
                ("joint_colors", dict(joint_colors=torch.zeros(5, 3))), ("joint_colors", dict(joint_colors=(1.0, 0.0))), ("bone_color", dict(bone_color=(1.0,))),
                ("light", dict(light=(1.0,))), ("over", dict(over=torch.zeros(2, 33, 40, 3))), ("over", dict(over=torch.zeros(1, 33, 40, 3, dtype=torch.uint8))),
                ("device", dict())]
    for match, kw in bad_skel:
        args = dict(keypoints=kp, parents=par, camera=cam)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            net.render_skeleton(**args)
    with pytest.raises(ValueError, match="2\\^31"):
        net.render_skeleton(kp, par, _cam(65536, 32768))
    result = dict(points=v, keypoints=kp[None], source_keypoints=kp[None], skin_weights=torch.zeros(5, 6))
    with pytest.raises(ValueError, match="sample_retarget"):
        net.render_retarget(dict(points=v), tri, cam)
    with pytest.raises(ValueError, match="joint_colors"):
        net.render_retarget(result, tri, cam, skin_colors=True)
    with pytest.raises(ValueError, match="joint_colors"):
        net.render_retarget(result, tri, cam, skin_colors=True, joint_colors=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="parents"):
        net.render_retarget(result, tri, cam)
    with pytest.raises(ValueError, match="device"):
        net.render_retarget(result, tri, cam, parents=par)
