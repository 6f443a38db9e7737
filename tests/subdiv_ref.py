"""Restatement of the Loop-subdivision path (neural_marionette_amd/subdivide.py: LoopPlan.build; nm_subdiv_apply, nm_vertex_normals and
nm_mesh_shade; NeuralMarionette.subdivide / vertex_normals / render_mesh(vertex_normals=...)).  It is NOT open3d's subdivide_loop or
compute_vertex_normals - the contract is the library's own, include/nm355.h has it in full - and this file is that contract spelled out
the slow way: the plan with plain Python dicts and loops (nothing of the vectorised builder is used), the stencils, normals and shading as
elementwise float64 numpy in the header's operation order, no einsum and no @ that might fuse.

  edges      the undirected edges {a < b} sorted by (a, b), edge e creates vertex V + e; row (a, b, c, d): c, d the opposite vertices in
             ascending triangle-row order, d = -1 on the boundary
  children   (i,j,k) -> (i,p,r) (p,j,q) (r,q,k) (p,q,r) with p = ev(i,j), q = ev(j,k), r = ev(k,i)
  rings      no boundary edge, n >= 1: the n neighbours ascending, (1 - n beta_n, beta_n); exactly two boundary edges: those two
             neighbours ascending, (0.75, 0.125); anything else: empty, (1, 0)
  apply      old vertex: s = 0.0; s = s + x[ring[j]] in ring order; w_self * x[v] + w_ring * s
             edge vertex: 0.375 * (x[a] + x[b]) + 0.125 * (x[c] + x[d]), or 0.5 * (x[a] + x[b]) on the boundary
  normals    acc = acc + (p1 - p0) x (p2 - p0) over the vertex's triangle rows ascending; acc / sqrt((ax ax + ay ay) + az az), or zero
  shade      h = ((l_0 n'_0 + l_1 n'_1) + l_2 n'_2) / L from the draw's l_k = w_k iz_k; light_a + light_b |h . d| / (sqrt(h . h) sqrt(A))

and the tiny meshes the tests share.  The mutations (ring_reverse, pair_ac, faces_reverse) are deliberate mistakes: the CPU tests show
that each changes bits, so the bit-for-bit GPU comparison can see such a mistake."""
import math

import numpy as np

import mesh_ref as MR
import render_ref as RR


# ---- the plan, by dicts and loops --------------------------------------------------------------------------------------------------
def beta(n):
    return (0.625 - (0.375 + 0.25 * math.cos(2.0 * math.pi / n)) ** 2) / n


def build_level(tri, V):
    """tables of one level as Python lists: edge, ring_offsets, ring, w, children"""
    opposite = {}                                                      # (a, b) -> the opposite vertices, in triangle-row order
    for row in tri:
        i, j, k = (int(x) for x in row)
        for s, t, o in ((i, j, k), (j, k, i), (k, i, j)):
            opposite.setdefault((min(s, t), max(s, t)), []).append(o)
    keys = sorted(opposite)
    number = {key: V + e for e, key in enumerate(keys)}
    edge = [[a, b, opposite[(a, b)][0], opposite[(a, b)][1] if len(opposite[(a, b)]) > 1 else -1] for a, b in keys]
    ev = lambda s, t: number[(min(s, t), max(s, t))]
    children = []
    for row in tri:
        i, j, k = (int(x) for x in row)
        p, q, r = ev(i, j), ev(j, k), ev(k, i)
        children += [[i, p, r], [p, j, q], [r, q, k], [p, q, r]]
    neighbours = [[] for _ in range(V)]
    on_boundary = [[] for _ in range(V)]
    for a, b in keys:
        neighbours[a].append(b)
        neighbours[b].append(a)
        if len(opposite[(a, b)]) == 1:
            on_boundary[a].append(b)
            on_boundary[b].append(a)
    ring_offsets, ring, w = [0], [], []
    for v in range(V):
        n = len(neighbours[v])
        if not on_boundary[v] and n >= 1:
            ring += sorted(neighbours[v])
            w.append([1.0 - n * beta(n), beta(n)])
        elif len(on_boundary[v]) == 2:
            ring += sorted(on_boundary[v])
            w.append([0.75, 0.125])
        else:
            w.append([1.0, 0.0])
        ring_offsets.append(len(ring))
    return dict(edge=edge, ring_offsets=ring_offsets, ring=ring, w=w, children=children)


def build_plan(tri, V, levels):
    """dict: levels (a list of build_level's tables as numpy arrays), triangles, face_offsets, faces, vertex_counts, triangle_counts"""
    tri = [[int(x) for x in row] for row in np.asarray(tri).reshape(-1, 3)]
    out = dict(levels=[], vertex_counts=[V], triangle_counts=[len(tri)])
    for _ in range(levels):
        lv = build_level(tri, V)
        tri, V = lv.pop("children"), V + len(lv["edge"])
        out["levels"].append(dict(edge=np.array(lv["edge"], np.int32).reshape(-1, 4), ring_offsets=np.array(lv["ring_offsets"], np.int32),
                                  ring=np.array(lv["ring"], np.int32), w=np.array(lv["w"], np.float64).reshape(-1, 2), children=np.array(tri, np.int32).reshape(-1, 3)))
        out["vertex_counts"].append(V)
        out["triangle_counts"].append(len(tri))
    incident = [[] for _ in range(V)]
    for m, row in enumerate(tri):
        for v in row:
            incident[v].append(m)
    out["triangles"] = np.array(tri, np.int32).reshape(-1, 3)
    out["face_offsets"] = np.array([0] + list(np.cumsum([len(x) for x in incident])), np.int32)
    out["faces"] = np.array([m for x in incident for m in x], np.int32)
    return out


# ---- the restatement: stencils, normals, shading ----------------------------------------------------------------------------------------
def apply_level(x, lv, ring_reverse=False, pair_ac=False):
    """one level: x (T,V,3) -> (T,V+E,3).  Mutations: ring_reverse sums each ring from its last entry to its first; pair_ac gives the
    edge's weights to the wrong pairs, 0.375 * (x[a] + x[c]) + 0.125 * (x[b] + x[d])."""
    x = np.asarray(x, np.float64)
    T, V = x.shape[:2]
    edge, off, ring, w = lv["edge"], lv["ring_offsets"], lv["ring"], lv["w"]
    out = np.empty((T, V + len(edge), 3))
    for v in range(V):
        s = np.zeros((T, 3))
        js = range(off[v], off[v + 1])
        for j in (reversed(js) if ring_reverse else js):
            s = s + x[:, ring[j]]
        out[:, v] = w[v, 0] * x[:, v] + w[v, 1] * s
    for e, (a, b, c, d) in enumerate(edge):
        if d < 0:
            out[:, V + e] = 0.5 * (x[:, a] + x[:, b])
        elif pair_ac:
            out[:, V + e] = 0.375 * (x[:, a] + x[:, c]) + 0.125 * (x[:, b] + x[:, d])
        else:
            out[:, V + e] = 0.375 * (x[:, a] + x[:, b]) + 0.125 * (x[:, c] + x[:, d])
    return out


def subdivide(x, plan, **mutation):
    """every level of build_plan's dict; x (T,V,3) or (V,3)"""
    x = np.asarray(x, np.float64)
    y = x[None] if x.ndim == 2 else x
    for lv in plan["levels"]:
        y = apply_level(y, lv, **mutation)
    return y[0] if x.ndim == 2 else y


def vertex_normals(vertices, triangles, face_offsets, faces, faces_reverse=False):
    """(F,V,3) -> (F,V,3), area-weighted; faces_reverse (a mutation) sums each vertex's triangles from the last to the first"""
    p = np.asarray(vertices, np.float64)
    F, V = p.shape[:2]
    out = np.zeros((F, V, 3))
    with np.errstate(all="ignore"):
        for v in range(V):
            acc = np.zeros((F, 3))
            js = range(face_offsets[v], face_offsets[v + 1])
            for j in (reversed(js) if faces_reverse else js):
                t = triangles[faces[j]]
                p0, p1, p2 = p[:, t[0]], p[:, t[1]], p[:, t[2]]
                e1, e2 = p1 - p0, p2 - p0
                c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
                acc = acc + c
            r = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
            ok = (r != 0.0) & np.isfinite(r)
            out[:, v] = np.where(ok[:, None], acc / np.where(ok, r, 1.0)[:, None], 0.0)
    return out


def render_smooth(vertices, triangles, normals, cam, vertex_colors=None, color=(0.7, 0.7, 0.7), light=(0.3, 0.7), background=(1.0, 1.0, 1.0)):
    """MR.render_mesh's index and depth, and the image shaded with the interpolated vertex normals (F,V,3): dict index, depth, image, and
    fallback (F,h,w): the covered pixels that kept the flat shade"""
    vertices, normals = np.asarray(vertices, np.float64), np.asarray(normals, np.float64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    flat = MR.render_mesh(vertices, tri, cam, vertex_colors=vertex_colors, color=color, light=light, background=background)
    E = RR.extrinsic(cam)
    dx, dy = RR.pixel_rays(cam)
    A = (dx * dx + dy * dy) + 1.0
    image = np.empty_like(flat["image"])
    fallback = np.zeros(flat["index"].shape, bool)
    with np.errstate(all="ignore"):
        for f in range(len(vertices)):
            t = MR.triangle_terms(vertices[f], tri, cam)
            win = np.maximum(flat["index"][f], 0)
            X, Y, iz, n = t["X"][win], t["Y"][win], t["iz"][win], t["n"][win]
            w = MR.edge_functions([X[..., k] for k in range(3)], [Y[..., k] for k in range(3)], dx, dy)
            l = [w[k] * iz[..., k] for k in range(3)]
            L = (l[0] + l[1]) + l[2]
            nv = [normals[f][tri[win, k]] for k in range(3)]            # (h, w, 3) per corner
            cam_n = [[(E[r, 0] * nv[k][..., 0] + E[r, 1] * nv[k][..., 1]) + E[r, 2] * nv[k][..., 2] for r in range(3)] for k in range(3)]
            h = np.stack([((l[0] * cam_n[0][r] + l[1] * cam_n[1][r]) + l[2] * cam_n[2][r]) / L for r in range(3)], -1)
            hh = MR.dot3(h, h)
            hd = (h[..., 0] * dx + h[..., 1] * dy) + h[..., 2]
            den = (n[..., 0] * dx + n[..., 1] * dy) + n[..., 2]
            use_flat = (hh == 0.0) | ~np.isfinite(hh)
            shade = np.where(use_flat, MR.headlight(light, den, MR.dot3(n, n), A), MR.headlight(light, hd, hh, A))
            if vertex_colors is not None:
                c = np.asarray(vertex_colors, np.float64)[tri[win]]
                col = ((l[0][..., None] * c[:, :, 0] + l[1][..., None] * c[:, :, 1]) + l[2][..., None] * c[:, :, 2]) / L[..., None]
            else:
                col = np.broadcast_to(np.asarray(color, np.float64), dx.shape + (3,))
            image[f] = RR.byte(col * shade[..., None])
            image[f][flat["index"][f] < 0] = RR.byte(np.asarray(background, np.float64))
            fallback[f] = use_flat & (flat["index"][f] >= 0)
    return dict(index=flat["index"], depth=flat["depth"], image=image, fallback=fallback, flat_image=flat["image"])


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def octahedron():
    v = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    return v, np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)


def icosahedron():
    return MR.icosphere(0)                                             # valence 5; its first level has valence 5 and 6


def fan(n=12):
    """a closed fan: the centre (vertex 0, interior, valence n) and n rim vertices, each on two boundary edges"""
    ang = np.arange(n) * (2.0 * np.pi / n)
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0.0 * ang], 1)])
    return v, np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)


def grid(nx=17, ny=16, step=1.5):
    """an open planar nx x ny grid of vertices, every quad split along the same diagonal: V 272, E 751 (62 on the boundary), M 480; two
    corners of valence 2, two of valence 3, the interior regular (valence 6).  Vertex (i, j) is row j * nx + i at (i step, j step, 0)."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    v = np.stack([i.reshape(-1) * step, j.reshape(-1) * step, np.zeros(nx * ny)], 1)
    tri = []
    for b in range(ny - 1):
        for a in range(nx - 1):
            o = b * nx + a
            tri += [[o, o + 1, o + nx + 1], [o, o + nx + 1, o + nx]]
    return v, np.array(tri, np.int32)


def with_unreferenced():
    """the tetrahedron and a fifth vertex that no triangle uses, between the others in the numbering"""
    v, t = tetrahedron()
    v = np.concatenate([v[:2], [[5.0, -3.0, 2.0]], v[2:]])
    return v, np.where(t >= 2, t + 1, t).astype(np.int32)


def bow_tie():
    """two open fans of three triangles that share vertex 0 only: it lies on four boundary edges and stays where it is"""
    v = np.array([[0.0, 0, 0], [1, -1, 0], [1.5, -0.3, 0.2], [1.5, 0.4, 0.1], [1, 1, 0], [-1, 1, 0.3], [-1.5, 0.3, 0], [-1.5, -0.4, 0.2], [-1, -1, 0]])
    return v, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 5, 6], [0, 6, 7], [0, 7, 8]], np.int32)


MESHES = dict(tetrahedron=tetrahedron, octahedron=octahedron, icosahedron=icosahedron, fan12=fan, grid=grid, unreferenced=with_unreferenced, bow_tie=bow_tie)


def mixed_magnitudes(shape, seed=1):
    """standard_normal * 2^integers(-20, 20): sums whose bits depend on their order"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 20, shape)
