"""float64 numpy restatement of the mesh and skeleton render path (nm_mesh_bin + nm_mesh_draw, nm_skeleton_draw,
NeuralMarionette.render_mesh / render_skeleton / render_retarget): posed triangle meshes, and skeletons of spheres and double cones,
drawn through the plate renderer's pinhole camera.  It is NOT open3d's image - the contract is the library's own, include/nm355.h has it
in full - and this file is that contract by brute force: every pixel against every primitive of its frame, elementwise float64
operations in the header's order, no einsum and no @ that might fuse.

  triangle   p'_k as the plates' c';  n = (p'_1 - p'_0) x (p'_2 - p'_0), q = n . p'_0, X_k = p'_kx / p'_kz, Y_k = p'_ky / p'_kz,
             iz_k = 1 / p'_kz;  not drawn: an index outside [0, V), a non-finite p', n or q, a vertex with p'_z < near, n = 0
  coverage   w0 = (X1 - dx) * (Y2 - dy) - (Y1 - dy) * (X2 - dx), w1, w2 by rotation: all >= 0 or all <= 0, and (w0 + w1) + w2 != 0
             and the pixel inside the triangle's rectangle floor(min_k u_k - 1) .. ceil(max_k u_k + 1), u_k = cx + fx X_k (the same in y)
  depth      den = (n_x dx + n_y dy) + n_z != 0, s = q / den >= near;  the smallest s wins, the lowest row among equal s
  colour     l_k = w_k iz_k, ((l_0 c_0 + l_1 c_1) + l_2 c_2) / ((l_0 + l_1) + l_2), times light_a + light_b |den| / (sqrt(n . n) sqrt(A))
  sphere     A = (dx^2 + dy^2) + 1, B = c . d, C = c . c - r^2, D = B B - A C >= 0 and B > 0:  s = C / (B + sqrt(D))
  nappe      the header's quadratic c2 s^2 - 2 c1 s + c0 = 0 and its square-root-free choice of the root on the nappe

and the small procedural scenes the tests share."""
import numpy as np

import render_ref as RR


# ---- the restatement: mesh -------------------------------------------------------------------------------------------------------
def to_camera(points, cam):
    """p'_r = ((E[r,0] x + E[r,1] y) + E[r,2] z) + E[r,3] for points (..., 3)"""
    E = RR.extrinsic(cam)
    p = np.asarray(points, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([((E[r, 0] * p[..., 0] + E[r, 1] * p[..., 1]) + E[r, 2] * p[..., 2]) + E[r, 3] for r in range(3)], -1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def triangle_terms(vertices, triangles, cam):
    """one frame: X, Y, iz (M,3), n (M,3), q (M) and which triangles are drawn at all"""
    vertices, tri = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(vertices)
    inside = ((tri >= 0) & (tri < V)).all(1)
    p = to_camera(vertices, cam)[np.clip(tri, 0, V - 1)]                        # (M, 3 vertices, 3)
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        q = dot3(n, p[:, 0])
        X, Y, iz = p[:, :, 0] / p[:, :, 2], p[:, :, 1] / p[:, :, 2], 1.0 / p[:, :, 2]
        drawn = inside & np.isfinite(p).all((1, 2)) & ~(p[:, :, 2] < cam.near).any(1) & np.isfinite(n).all(1) & np.isfinite(q) & (n != 0.0).any(1)
    return dict(X=X, Y=Y, iz=iz, n=n, q=q, drawn=drawn)


def edge_functions(X, Y, dx, dy):
    """w0, w1, w2 of one triangle (X, Y: its three projected vertices) at the pixels dx, dy"""
    a, b = [X[k] - dx for k in range(3)], [Y[k] - dy for k in range(3)]
    return a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]


def headlight(light, den, nn, A):
    return light[0] + light[1] * np.abs(den) / (np.sqrt(nn) * np.sqrt(A))


def render_mesh(vertices, triangles, cam, vertex_colors=None, color=(0.7, 0.7, 0.7), light=(0.3, 0.7), background=(1.0, 1.0, 1.0), crop=None,
                stats=False):
    """index (F,h,w) int32, depth (F,h,w) float64, image (F,h,w,3) uint8; with stats=True also cover (F,h,w), the number of drawn
    triangles whose edge functions cover the pixel (whatever their depth), and edge0, whether any drawn triangle has an edge function of
    exactly 0 there"""
    vertices = np.asarray(vertices, np.float64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    F = len(vertices)
    dx, dy = RR.pixel_rays(cam, crop)
    h, w = dx.shape
    cx0, cx1, cy0, cy1 = crop if crop is not None else (0, cam.width, 0, cam.height)
    px, py = np.arange(cx0, cx1, dtype=np.float64)[None, :], np.arange(cy0, cy1, dtype=np.float64)[:, None]
    A = (dx * dx + dy * dy) + 1.0
    index = np.full((F, h, w), -1, np.int32)
    depth = np.full((F, h, w), np.inf)
    den_w = np.zeros((F, h, w))
    w_w = np.zeros((3, F, h, w))
    cover = np.zeros((F, h, w), np.int32)
    edge0 = np.zeros((F, h, w), bool)
    image = np.empty((F, h, w, 3), np.uint8)
    with np.errstate(all="ignore"):
        for f in range(F):
            t = triangle_terms(vertices[f], tri, cam)
            best_i, best_s = index[f], depth[f]
            for i in np.nonzero(t["drawn"])[0]:
                w0, w1, w2 = edge_functions(t["X"][i], t["Y"][i], dx, dy)
                covered = (((w0 >= 0.0) & (w1 >= 0.0) & (w2 >= 0.0)) | ((w0 <= 0.0) & (w1 <= 0.0) & (w2 <= 0.0))) & ((w0 + w1) + w2 != 0.0)
                u, v = cam.cx + cam.fx * t["X"][i], cam.cy + cam.fy * t["Y"][i]
                covered &= (px >= np.floor(u.min() - 1.0)) & (px <= np.ceil(u.max() + 1.0)) & (py >= np.floor(v.min() - 1.0)) & (py <= np.ceil(v.max() + 1.0))
                if stats:
                    cover[f] += covered
                    edge0[f] |= (w0 == 0.0) | (w1 == 0.0) | (w2 == 0.0)
                if not covered.any():
                    continue
                n = t["n"][i]
                den = (n[0] * dx + n[1] * dy) + n[2]
                s = t["q"][i] / den
                better = covered & (den != 0.0) & (s >= cam.near) & (s < best_s)      # strictly: of equal s the earlier, lower row stays
                best_s[better] = s[better]
                best_i[better] = i
                den_w[f][better] = den[better]
                for k, wk in enumerate((w0, w1, w2)):
                    w_w[k, f][better] = wk[better]
            win = np.maximum(best_i, 0)
            n = t["n"][win] if len(tri) else np.zeros((h, w, 3))
            shade = headlight(light, den_w[f], dot3(n, n), A)
            if vertex_colors is not None and len(tri):
                c = np.asarray(vertex_colors, np.float64)[np.clip(tri[win], 0, len(vertex_colors) - 1)]      # (h, w, 3 vertices, 3 channels)
                l = [w_w[k, f] * t["iz"][win, k] for k in range(3)]
                L = (l[0] + l[1]) + l[2]
                col = ((l[0][..., None] * c[:, :, 0] + l[1][..., None] * c[:, :, 1]) + l[2][..., None] * c[:, :, 2]) / L[..., None]
            else:
                col = np.broadcast_to(np.asarray(color, np.float64), (h, w, 3))
            image[f] = RR.byte(col * shade[..., None])
            image[f][best_i < 0] = RR.byte(np.asarray(background, np.float64))
    out = dict(index=index, depth=depth, image=image)
    if stats:
        out.update(cover=cover, edge0=edge0)
    return out


# ---- the restatement: skeleton ---------------------------------------------------------------------------------------------------
def ge0(P, Q, D):
    """P + Q sqrt(D) >= 0 without the square root"""
    return np.where(Q >= 0.0, (P >= 0.0) | ((Q * Q) * D >= P * P), (P >= 0.0) & (P * P >= (Q * Q) * D))


def nappe_terms(a, g, rb):
    v = g - a
    vv = dot3(v, v)
    with np.errstate(all="ignore"):
        kappa = (vv + rb * rb) / (vv * vv)
    return dict(a=a, v=v, vv=vv, kappa=kappa, av=dot3(a, v), aa=dot3(a, a), ok=bool(vv > 0.0 and np.isfinite(kappa)))


def nappe_hit(t, dx, dy, A):
    """hit (h,w) bool, s (h,w), normal (h,w,3) of one nappe"""
    a, v, vv, kappa, av, aa = t["a"], t["v"], t["vv"], t["kappa"], t["av"], t["aa"]
    dv, da = (dx * v[0] + dy * v[1]) + v[2], (dx * a[0] + dy * a[1]) + a[2]
    kd = kappa * dv
    c2, c1, c0 = kd * dv - A, kd * av - da, (kappa * av) * av - aa
    D = c1 * c1 - c2 * c0
    P = c1 * dv - av * c2
    P2 = P - vv * c2
    up = c2 > 0.0
    on = lambda Q: np.where(up, ge0(P, Q, D) & ge0(-P2, -Q, D), ge0(-P, -Q, D) & ge0(P2, Q, D))
    Qn = np.where(up, -dv, dv)
    near_on, far_on = on(Qn), on(-Qn)
    plus = np.where(near_on, ~up, up)
    r = np.sqrt(D)
    qq = c1 + np.where(c1 >= 0.0, r, -r)
    hit = (c2 != 0.0) & (D >= 0.0) & (near_on | far_on) & (qq != 0.0)
    s = np.where(plus == (c1 >= 0.0), qq / c2, c0 / qq)
    km = kappa * (s * dv - av)
    normal = np.stack([(s * dx - a[0]) - km * v[0], (s * dy - a[1]) - km * v[1], (s - a[2]) - km * v[2]], -1)
    return hit, s, normal


def skeleton_primitives(keypoints, parents, cam, threshold, radius, bone_radius):
    """one frame: p' (K,3), visible (K), which spheres and which bones are drawn, and the bones' nappes"""
    kp = np.asarray(keypoints, np.float32).astype(np.float64)
    K = len(kp)
    p = to_camera(kp[:, :3], cam)
    with np.errstate(all="ignore"):
        visible = (np.clip(kp[:, 3], 0.0, 1.0) >= threshold) & np.isfinite(p).all(1)
        spheres = visible & ~(p[:, 2] - radius < cam.near)
    bones = {}
    for k in range(K):
        q = int(parents[k])
        if not (visible[k] and 0 <= q < K and q != k and visible[q]):
            continue
        b = p[k] - p[q]
        bb = dot3(b, b)
        if not (bb > 0.0 and np.isfinite(bb)) or p[k, 2] - bone_radius < cam.near or p[q, 2] - bone_radius < cam.near:
            continue
        g = p[q] + 0.2 * b
        n1, n2 = nappe_terms(p[q], g, bone_radius), nappe_terms(p[k], g, bone_radius)
        if n1["ok"] and n2["ok"]:
            bones[k] = (n1, n2)
    return p, visible, spheres, bones


def render_skeleton(keypoints, parents, cam, threshold=0.2, radius=0.03, bone_radius=0.03, joint_colors=(0.7, 0.1, 0.0), bone_color=(0.0, 0.6, 0.1),
                    light=(0.3, 0.7), background=(1.0, 1.0, 1.0), over=None, crop=None):
    """index (F,h,w) int32 (sphere k: k, bone of joint k: K + k), depth, image (over a copy of `over` where given), and second (F,h,w):
    the second-smallest depth among the primitives at each pixel (+inf with fewer than two)"""
    keypoints = np.asarray(keypoints, np.float32)
    F, K = keypoints.shape[:2]
    dx, dy = RR.pixel_rays(cam, crop)
    h, w = dx.shape
    A = (dx * dx + dy * dy) + 1.0
    jc = np.asarray(joint_colors, np.float64)
    jc = np.broadcast_to(jc, (K, 3)) if jc.ndim == 1 else jc
    palette = np.concatenate([jc, np.broadcast_to(np.asarray(bone_color, np.float64), (K, 3))])
    index = np.full((F, h, w), -1, np.int32)
    depth = np.full((F, h, w), np.inf)
    second = np.full((F, h, w), np.inf)
    image = np.empty((F, h, w, 3), np.uint8)
    with np.errstate(all="ignore"):
        for f in range(F):
            p, visible, spheres, bones = skeleton_primitives(keypoints[f], parents, cam, threshold, radius, bone_radius)
            best_i, best_s, sec = index[f], depth[f], second[f]
            normal = np.zeros((h, w, 3))

            def take(i, hit, s, nrm):
                s = np.where(hit, s, np.inf)
                np.copyto(sec, np.minimum(sec, np.maximum(s, best_s)))
                better = hit & (s < best_s)                                        # strictly: of equal s the lower primitive number stays
                best_s[better] = s[better]
                best_i[better] = i
                normal[better] = nrm[better]

            for k in np.nonzero(spheres)[0]:
                c = p[k]
                Cc = dot3(c, c) - radius * radius
                B = (dx * c[0] + dy * c[1]) + c[2]
                D = B * B - A * Cc
                s = Cc / (B + np.sqrt(D))
                take(k, (D >= 0.0) & (B > 0.0), s, np.stack([s * dx - c[0], s * dy - c[1], s - c[2]], -1))
            for k in sorted(bones):
                h1, s1, m1 = nappe_hit(bones[k][0], dx, dy, A)
                h2, s2, m2 = nappe_hit(bones[k][1], dx, dy, A)
                s1, s2 = np.where(h1, s1, np.inf), np.where(h2, s2, np.inf)
                first = h1 & ~(h2 & (s2 < s1))                                     # the parent's nappe on a tie
                take(K + k, h1 | h2, np.where(first, s1, s2), np.where(first[..., None], m1, m2))
            den = (normal[..., 0] * dx + normal[..., 1] * dy) + normal[..., 2]
            shade = headlight(light, den, dot3(normal, normal), A)
            img = RR.byte(palette[np.maximum(best_i, 0)] * shade[..., None])
            image[f] = np.asarray(over[f]) if over is not None else RR.byte(np.asarray(background, np.float64))
            image[f][best_i >= 0] = img[best_i >= 0]
    return dict(index=index, depth=depth, image=image, second=second)


def near_ties(ref, rel=1e-12):
    """the pixels whose best and second-best depths differ, but by less than a relative `rel`: either primitive may win there.  (Depths
    that are EQUAL - two joints in one place - are no such pixels: the lower primitive number wins them.)"""
    with np.errstate(all="ignore"):
        return np.isfinite(ref["second"]) & (ref["second"] > ref["depth"]) & (ref["second"] - ref["depth"] < rel * ref["depth"])


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def to_world(cam_pts, E):
    return (np.asarray(cam_pts, np.float64) - E[:3, 3]) @ E[:3, :3]                # R^T (p - t) for a rigid E


def soup(n, seed, E, fx, fy, cx, cy, W, H, z_range=(1.5, 4.0), spill=1.6, size=0.35):
    """n independent triangles whose centres project all over the image and `spill` times past its edges (some straddle every edge,
    some lie wholly outside), in world coordinates through the inverse of the rigid E: vertices (3n,3), triangles (n,3) with the
    vertex order shuffled"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(*z_range, n)
    u = (rng.uniform(-spill, spill, n) * 0.5 + 0.5) * W
    v = (rng.uniform(-spill, spill, n) * 0.5 + 0.5) * H
    centre = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    corners = centre[:, None, :] + rng.uniform(-size, size, (n, 3, 3))
    perm = rng.permutation(3 * n)
    vertices = np.empty((3 * n, 3))
    vertices[perm] = to_world(corners.reshape(-1, 3), E)
    return vertices, perm.reshape(n, 3).astype(np.int32)


def icosphere(subdivisions=2, radius=1.0):
    """the icosahedron subdivided `subdivisions` times (2: 162 vertices, 320 triangles), consistently oriented"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
             (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = verts[i] + verts[j]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts) * radius, np.array(faces, np.int32)


def torus(nu=16, nv=10, R=1.0, r=0.4):
    """a torus as an nu x nv grid of quads split in two: nu nv vertices, 2 nu nv triangles, closed"""
    a, b = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    verts = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            faces += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return verts, np.array(faces, np.int32)


def posed(verts, E, angles, shift, scale=1.0):
    """camera-space pose of an object (rotated by `angles`, scaled, centred at `shift` in front of the camera) given in world coordinates"""
    R = RR.rigid(angles, (0, 0, 0))[:3, :3]
    return to_world((verts * scale) @ R.T + np.asarray(shift, np.float64), E)


def hand_skeleton(E):
    """K = 6 joints in F = 2 frames, given through the inverse of the rigid E, in camera space about z = 3: 0 the root (parents[0] = 0),
    1 its child, 2 and 3 the children of 1 (a branch), 4 a child of 2 and 5 a child of 4.  Frame 0: joint 4 is under the threshold, so
    its sphere, its bone and the bone of its child 5 are gone; joint 1's intensity is above 1 (clipped) and joint 3's just above the
    threshold.  Frame 1: every joint is visible, joint 3 coincides with its parent 1 (a bone of length 0) and joint 2 lies behind the
    camera, so its sphere, its bone and the bone of its child 4 to it are gone.  Two bones point along the view, inside their nappes'
    half-angles - 3 towards the camera in frame 0, 5 away from it in frame 1 - so that rays steeper than the cone (c2 > 0, the far root)
    occur.  Returns keypoints (2,6,4) float32, parents (6) int32."""
    parents = np.array([0, 0, 1, 1, 2, 4], np.int32)
    cam0 = np.array([[0.0, -0.5, 3.0], [0.1, -0.1, 2.8], [-0.45, 0.35, 3.3], [0.22, 0.02, 2.3], [-0.6, 0.6, 3.0], [-0.35, 0.77, 3.52]])
    cam1 = cam0 + np.array([0.05, 0.02, 0.1])
    cam1[2] = [-0.2, 0.3, -1.0]
    alpha = np.array([0.9, 1.7, 0.5, 0.21, 0.1, 0.8])
    kp = np.zeros((2, 6, 4), np.float32)
    for f, c in enumerate((cam0, cam1)):
        kp[f, :, :3] = to_world(c, E)
        kp[f, :, 3] = alpha
    kp[1, 3, :3] = kp[1, 1, :3]                                                  # exactly, after the float32 rounding too
    kp[1, 4, 3] = 0.9
    return kp, parents


SKEL_RADIUS, SKEL_BONE, SKEL_TIE_CAP = 0.14, 0.09, 0.005


def skeleton_scene(W, H, focal, radius=SKEL_RADIUS, bone_radius=SKEL_BONE):
    """hand_skeleton through a W x H camera with per-joint colours, and its restatement with and without an image to paste over.  The
    near ties of the restatement (near_ties: either primitive may win) must stay within SKEL_TIE_CAP of the covered pixels."""
    from neural_marionette_amd import PinholeCamera
    E = RR.rigid((0.2, -0.3, 0.1), (0.1, -0.1, 0.3))
    cam = PinholeCamera(E.tolist(), focal, focal, W / 2 - 0.5, H / 2 - 0.5, W, H)
    kp, parents = hand_skeleton(E)
    colors = RR.palette(6, 9)
    over = np.random.default_rng(4).integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    kw = dict(radius=radius, bone_radius=bone_radius, joint_colors=colors, bone_color=(0.0, 0.6, 0.1), background=(0.25, 0.5, 1.0))
    ref = render_skeleton(kp, parents, cam, **kw)
    pasted = render_skeleton(kp, parents, cam, over=over, **kw)
    covered, ties = ref["index"] >= 0, near_ties(ref)
    assert covered.sum() > 100 and ties.sum() <= SKEL_TIE_CAP * covered.sum(), (int(covered.sum()), int(ties.sum()))
    return dict(cam=cam, keypoints=kp, parents=parents, colors=colors, over=over, ref=ref, pasted=pasted, kw=kw)
