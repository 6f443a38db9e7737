"""float64 numpy restatement of the surface path (nm_occupied_surface, NeuralMarionette.surface_points): what the reference's demo
scripts do with every decoded frame after the lines tests/output_path_ref.py restates (vis_generation.py:157-171,
vis_interpolation.py:160-177) - with the library's own definition of the normal in place of open3d's, whose 30-nearest-neighbour set
on a voxel lattice is decided by tie-breaking inside its k-d tree:

  neighbourhood  the occupied voxels q of the point's frame, inside the grid, with |q - p|^2 <= radius2, p included
  moments        d = q - p: n, S = sum d, Q = sum d d^T (xx, xy, xz, yy, yz, zz), by brute force over the offsets
  normal         numpy.linalg.eigh of C = n Q - S S^T: the eigenvector of the smallest eigenvalue; (0, 0, 1) for n < 3
  orientation    "outward": n . o >= 0 for o = -S; S = 0: o = N_f p - sum_f q; that 0 too: (1, 1, 1); or towards a point per clip
  plates         drawPlate's arithmetic (vis_generation.py:30-38), rows [R | centre]
  colours        base[f] * (depth * a + b) (+ add[f])

and a small deterministic generator of voxel shells (surface samples of two ellipsoids and a thin limb, voxelised by the rule of
utils/dataset_utils.py:21-31) for the tests' inputs."""
import numpy as np

import output_path_ref as OR


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _voxelize(points, G):
    """utils/dataset_utils.py:21-31: idx = int32((p + 1) / (2 / G + 1e-5)), occupancy 1.0"""
    step = (np.array([1.0, 1.0, 1.0]) - np.array([-1.0, -1.0, -1.0])) / (G, G, G)
    idx = ((points - np.array([-1.0, -1.0, -1.0])) / (step + 1e-5)).astype(np.int32)
    grid = np.zeros((G, G, G), np.float32)
    grid[idx[:, 0], idx[:, 1], idx[:, 2]] = 1.0
    return grid


def shell_frame(G, seed, phase=0.0):
    """one frame: the surfaces of two ellipsoids (a torso and a head) and of a thin limb (a capsule about a voxel and a half across at
    32^3) that swings with ``phase``"""
    rng = np.random.default_rng(seed)
    n = 6 * G * G

    def sphere(m):
        u = rng.standard_normal((m, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True)

    torso = sphere(n) * np.array([0.30, 0.22, 0.42]) + np.array([0.02, -0.05, -0.12])
    head = sphere(n // 3) * np.array([0.16, 0.15, 0.17]) + np.array([0.05, 0.0, 0.55])
    a = np.array([0.25, 0.10, 0.05])
    b = a + 0.55 * np.array([np.cos(0.4 + phase), 0.35, np.sin(0.4 + phase)])
    t = rng.random((n // 3, 1))
    limb = a + t * (b - a) + 0.045 * sphere(n // 3)
    pts = np.clip(np.concatenate([torso, head, limb]), -0.98, 0.98)
    return _voxelize(pts, G)


def shell_clip(B, T, G, seed=0):
    """(B,T,1,G,G,G) float32 of shell frames, the limb moving from frame to frame"""
    return np.stack([np.stack([shell_frame(G, seed + 31 * b + t, 0.3 * t + 0.7 * b)[None] for t in range(T)]) for b in range(B)])


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def offsets_within(radius2):
    r = int(np.floor(np.sqrt(radius2)))
    d = np.array([(x, y, z) for x in range(-r, r + 1) for y in range(-r, r + 1) for z in range(-r, r + 1)
                  if x * x + y * y + z * z <= radius2], np.int64)
    return r, d


def moments_brute(idx, G, radius2):
    """idx (n,3): one frame's occupied voxels.  (n,10) int64: n, S (3), Q (xx, xy, xz, yy, yz, zz), summed offset by offset"""
    r, offs = offsets_within(radius2)
    occ = np.zeros((G + 2 * r,) * 3, bool)
    idx = idx.astype(np.int64)
    occ[idx[:, 0] + r, idx[:, 1] + r, idx[:, 2] + r] = True
    m = np.zeros((len(idx), 10), np.int64)
    for d in offs:
        q = idx + d + r
        hit = occ[q[:, 0], q[:, 1], q[:, 2]].astype(np.int64)
        m[:, 0] += hit
        m[:, 1:4] += hit[:, None] * d
        m[:, 4:] += hit[:, None] * np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]])
    return m


def moments_kdtree(idx, radius2):
    """the same from scipy's k-d tree: the neighbours of each point within sqrt(radius2) (squared distances are integers, so the
    slack of 1e-9 admits no other lattice point)"""
    from scipy.spatial import cKDTree
    p = idx.astype(np.float64)
    m = np.zeros((len(idx), 10), np.int64)
    if len(idx) == 0:
        return m
    near = cKDTree(p).query_ball_point(p, np.sqrt(radius2) + 1e-9)
    for a, nb in enumerate(near):
        d = idx[nb].astype(np.int64) - idx[a].astype(np.int64)
        m[a, 0] = len(nb)
        m[a, 1:4] = d.sum(0)
        m[a, 4:] = [(d[:, 0] * d[:, 0]).sum(), (d[:, 0] * d[:, 1]).sum(), (d[:, 0] * d[:, 2]).sum(), (d[:, 1] * d[:, 1]).sum(),
                    (d[:, 1] * d[:, 2]).sum(), (d[:, 2] * d[:, 2]).sum()]
    return m


def covariance(m):
    """C = n Q - S S^T (N,3,3), exact in int64, as float64"""
    m = m.astype(np.int64)
    n, S = m[:, 0], m[:, 1:4]
    Q = m[:, [4, 5, 6, 5, 7, 8, 6, 8, 9]].reshape(-1, 3, 3)
    C = n[:, None, None] * Q - S[:, :, None] * S[:, None, :]
    assert np.abs(C).max(initial=0) < 2 ** 31
    return C.astype(np.float64)


def draw_plate_transform(center, orientation):
    """vis_generation.py:30-38 for one plate: the first three rows of the transform"""
    line1 = np.array([0.0, 0.0, 1.0])
    line2 = orientation / (np.linalg.norm(orientation) + 1e-6)
    v = np.cross(line1, line2)
    c = np.dot(line1, line2) + 1e-8
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    R = np.eye(3) + k + np.matmul(k, k) * (1 / (1 + c))
    if np.abs(c + 1.0) < 1e-4:
        R = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]])
    return np.concatenate((R, center[:, np.newaxis]), axis=1)


def plate_rows(centers, normals):
    """draw_plate_transform for (N,3) centres and normals at once, the same operations in the same order: (N,3,4)"""
    centers, normals = np.asarray(centers, np.float64), np.asarray(normals, np.float64)
    N = len(normals)
    line2 = normals / (np.sqrt((normals * normals).sum(1)) + 1e-6)[:, None]
    v = np.stack([0.0 * line2[:, 2] - 1.0 * line2[:, 1], 1.0 * line2[:, 0] - 0.0 * line2[:, 2], 0.0 * line2[:, 1] - 0.0 * line2[:, 0]], 1)
    c = line2[:, 2] + 1e-8
    z = np.zeros(N)
    k = np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)
    R = np.eye(3)[None] + k + np.matmul(k, k) * (1 / (1 + c))[:, None, None]
    R[np.abs(c + 1.0) < 1e-4] = np.array([[-1.0, 0, 0], [0, 1, 0], [0, 0, -1]])
    return np.concatenate([R, centers[:, :, None]], axis=2)


def shade(depth, frame, base, add=None, a=0.8, b=0.2):
    """vis_generation.py:167-169 / vis_interpolation.py:170-175: base[f] * (depth * a + b) (+ add[f]) for every point"""
    base = np.asarray(base, np.float64).reshape(-1, 3)
    col = base[frame] * (depth * a + b)[:, None]
    if add is not None:
        col = col + np.asarray(add, np.float64).reshape(-1, 3)[frame]
    return col


def orient_vectors(m, idx, frame, offsets, coords, orient_point=None, T=1):
    """the vector o each normal must not point away from: (N,3) float64"""
    if orient_point is not None:
        return np.asarray(orient_point, np.float64).reshape(-1, 3)[frame // T] - coords
    o = -m[:, 1:4].astype(np.int64)
    idx = idx.astype(np.int64)
    for f in range(len(offsets) - 1):
        rows = np.arange(offsets[f], offsets[f + 1])
        if len(rows) == 0:
            continue
        flat = rows[(m[rows, 1:4] == 0).all(1)]
        o[flat] = len(rows) * idx[flat] - idx[rows].sum(0)
    o[(o == 0).all(1)] = 1
    return o.astype(np.float64)


def surface_points(vox, threshold=0.5, radius2=6, orient_point=None, base=None, add=None, shade_ab=(0.8, 0.2)):
    """vox (T,1,G,G,G) or (B,T,1,G,G,G) float32.  output_path_ref.occupied_points' float64 dict plus moments (N,10) int32, C (N,3,3),
    normals, spread, o (the orientation vectors), frame (N), plates and - with base (F,3) - colors.  orient_point: None for
    "outward", else (3) or (B,3)"""
    out = OR.occupied_points(vox, threshold, np.float64)
    B, T = out["counts"].shape
    G = np.asarray(vox).shape[-1]
    idx, offs = out["indices"], out["offsets"]
    N = len(idx)
    frame = np.repeat(np.arange(B * T), np.diff(offs))
    m = np.concatenate([moments_brute(idx[offs[f]:offs[f + 1]], G, radius2) for f in range(B * T)] + [np.zeros((0, 10), np.int64)])
    C = covariance(m)
    lam, vec = np.linalg.eigh(C) if N else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    normals = np.ascontiguousarray(vec[:, :, 0])
    normals[m[:, 0] < 3] = (0.0, 0.0, 1.0)
    if orient_point is not None:
        orient_point = np.broadcast_to(np.asarray(orient_point, np.float64), (B, 3))
    o = orient_vectors(m, idx, frame, offs, out["coords"], orient_point, T)
    dot = normals[:, 0] * o[:, 0] + normals[:, 1] * o[:, 1] + normals[:, 2] * o[:, 2]
    normals[dot < 0] *= -1.0
    out.update(moments=m.astype(np.int32), C=C, normals=normals, spread=lam, o=o, frame=frame, plates=plate_rows(out["coords"], normals))
    if base is not None:
        with np.errstate(invalid="ignore"):
            out["colors"] = shade(out["depth"], frame, base, add, *shade_ab)
    return out


# ---- the inputs the device tests use (tests/test_surface_path_cpu.py keeps the restatement inside the tests' caps on them) ---------
def hand_clip():
    """G = 8, one clip of eight frames: a lone voxel, a full plane across each axis, a line, voxels on all six faces and in the
    corners, an empty frame, and a two-voxel pair (n = 2)"""
    G = 8
    v = np.zeros((1, 8, 1, G, G, G), np.float32)
    v[0, 0, 0, 4, 3, 5] = 1                                            # alone: n = 1, S = 0, the frame's centroid itself
    v[0, 1, 0, 3, :, :] = 1                                            # planes: the normal is exactly +-e
    v[0, 2, 0, :, 5, :] = 1
    v[0, 3, 0, :, :, 2] = 1
    v[0, 4, 0, 2, 5, :] = 1                                            # a line along k: two vanishing eigenvalues
    f = v[0, 5, 0]
    for a in (0, G - 1):                                               # faces and corners: every window is clipped
        f[a, 2:6, 2:6] = 1
        f[2:6, a, 2:6] = 1
        f[2:6, 2:6, a] = 1
        for b in (0, G - 1):
            for c in (0, G - 1):
                f[a, b, c] = 1
    v[0, 7, 0, 1, 1, 6] = 1
    v[0, 7, 0, 1, 1, 7] = 1
    return v


def leak_clip(G=20, seed=11):
    """two shell frames with a 3 x 3 patch on the last i-plane of the first and on the first i-plane of the second: adjacent in memory
    (20^3 voxels are whole words, no pad bits lie between the frames), not in space"""
    v = shell_clip(1, 2, G, seed)
    v[0, 0, 0, G - 1, 4:7, 5:8] = 1
    v[0, 1, 0, 0, 4:7, 5:8] = 1
    return v


def nan_clip(G=20, seed=17):
    """shell frames with NaN voxels, which a threshold leaves occupied: one beside the shell, one far from it"""
    v = shell_clip(1, 2, G, seed)
    i, j, k = np.argwhere(v[0, 0, 0] > 0)[40]
    v[0, 0, 0, i, j, max(k - 1, 0)] = np.nan
    v[0, 1, 0, 1, 1, 1] = np.nan
    return v


TOWARDS = (0.3, -2.0, 0.5)
# name -> (builder, radius2, orient_point, held to the caps).  The hand-made frames are degenerate on purpose (a plane's in-plane S, a
# line's two vanishing eigenvalues): their direction and sign are decided by exact statements in the tests, not by the caps.
CASES = {
    "hand_r6": (hand_clip, 6, None, False),
    "hand_r1": (hand_clip, 1, None, False),
    "hand_r16_towards": (hand_clip, 16, TOWARDS, False),
    "G20_leak_r6": (leak_clip, 6, None, True),
    "G20_nan_r4": (nan_clip, 4, None, True),
    "G33_r9": (lambda: shell_clip(1, 2, 33, 5), 9, None, True),
    "G32_r1": (lambda: shell_clip(2, 3, 32, 3), 1, None, True),
    "G32_r3": (lambda: shell_clip(2, 3, 32, 3), 3, None, True),
    "G32_r6": (lambda: shell_clip(2, 3, 32, 3), 6, None, True),
    "G32_r9": (lambda: shell_clip(2, 3, 32, 3), 9, None, True),
    "G32_r16": (lambda: shell_clip(2, 3, 32, 3), 16, None, True),
    "G32_r6_towards": (lambda: shell_clip(2, 3, 32, 3), 6, TOWARDS, True),
    "slab_below_G112_r16": (lambda: shell_clip(1, 1, 112, 7), 16, None, True),
    "slab_above_G124_r16": (lambda: shell_clip(1, 1, 124, 7), 16, None, True),
}
GAP, GAP_CAP, SIGN_TOL, SIGN_CAP = 1e-3, 0.05, 1e-6, 0.12


def exempt_rows(ref):
    """(rows below the eigenvalue gap, rows whose sign the orientation rule does not decide) among the rows the checks look at"""
    lam, o = ref["spread"], ref["o"]
    solved = ref["moments"][:, 0] >= 3
    gap = solved & (lam[:, 1] - lam[:, 0] < GAP * lam[:, 2])
    dot = (ref["normals"] * o).sum(1)
    sign = np.abs(dot) <= SIGN_TOL * np.sqrt((o * o).sum(1))
    return gap, sign
