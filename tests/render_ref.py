"""float64 numpy restatement of the render path (nm_render_bin + nm_render_draw, NeuralMarionette.render_plates): the plates of the
surface path drawn as flat discs through an open3d-style pinhole camera.  It is NOT open3d's image - the contract is the library's
own, include/nm355.h has it in full - and this file is that contract by brute force: every pixel against every plate of its frame,
elementwise float64 operations in the header's order, no einsum and no @ that might fuse.

  per plate   c'_r = ((E[r,0] c_x + E[r,1] c_y) + E[r,2] c_z) + E[r,3],  a'_r = (E[r,0] a_x + E[r,1] a_y) + E[r,2] a_z,
              q = (a'_x c'_x + a'_y c'_y) + a'_z c'_z;  c'_z - radius < near or a non-finite component: not drawn at all
  per pixel   d = ((px - cx) / fx, (py - cy) / fy, 1);  den = (a'_x dx + a'_y dy) + a'_z, 0 is a miss;  s = q / den, a miss unless
              s >= near;  h = s d - c',  m = (h_x^2 + h_y^2) + h_z^2;  hit iff m <= radius * radius
  winner      the smallest s, the lowest row among equal s
  image       uint8(clip(nan_to_0(colors[i] * (light_a + light_b * |den| / sqrt((dx^2 + dy^2) + 1))), 0, 1) * 255.0), truncated

and the small scenes the tests share."""
import numpy as np

import surface_ref as SR


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def extrinsic(cam):
    return np.array(cam.extrinsic, np.float64).reshape(4, 4)


def plate_terms(plates, cam, radius):
    """c' (N,3), a' (N,3), q (N) and which plates are drawn at all"""
    E = extrinsic(cam)
    c, a = plates[:, :, 3], plates[:, :, 2]
    with np.errstate(all="ignore"):
        cp = np.stack([((E[r, 0] * c[:, 0] + E[r, 1] * c[:, 1]) + E[r, 2] * c[:, 2]) + E[r, 3] for r in range(3)], 1)
        ap = np.stack([(E[r, 0] * a[:, 0] + E[r, 1] * a[:, 1]) + E[r, 2] * a[:, 2] for r in range(3)], 1)
        q = (ap[:, 0] * cp[:, 0] + ap[:, 1] * cp[:, 1]) + ap[:, 2] * cp[:, 2]
        drawn = np.isfinite(cp).all(1) & np.isfinite(ap).all(1) & ~(cp[:, 2] - radius < cam.near)
    return cp, ap, q, drawn


def pixel_rays(cam, crop=None):
    """dx, dy (h,w) of the pixels x0 <= px < x1, y0 <= py < y1 (crop = (x0, x1, y0, y1); None: the whole image)"""
    x0, x1, y0, y1 = crop if crop is not None else (0, cam.width, 0, cam.height)
    dx = (np.arange(x0, x1, dtype=np.float64) - cam.cx) / cam.fx
    dy = (np.arange(y0, y1, dtype=np.float64) - cam.cy) / cam.fy
    return np.broadcast_to(dx[None, :], (y1 - y0, x1 - x0)).copy(), np.broadcast_to(dy[:, None], (y1 - y0, x1 - x0)).copy()


def byte(v):
    v = np.where(np.isnan(v), 0.0, v)
    return (np.clip(v, 0.0, 1.0) * 255.0).astype(np.uint8)


def render(plates, offsets, colors, cam, radius=0.03, light=(1.0, 0.0), background=(1.0, 1.0, 1.0), crop=None, margin=False):
    """index (F,h,w) int32, depth (F,h,w) float64, image (F,h,w,3) uint8 [colors given], and with margin=True the smallest
    |m - radius^2| any candidate (den != 0, s >= near) left at each pixel - how far the pixel's verdicts are from changing"""
    plates = np.asarray(plates, np.float64)
    offsets = np.asarray(offsets, np.int64)
    F = len(offsets) - 1
    cp, ap, q, drawn = plate_terms(plates, cam, radius)
    dx, dy = pixel_rays(cam, crop)
    h, w = dx.shape
    r2 = radius * radius
    index = np.full((F, h, w), -1, np.int32)
    depth = np.full((F, h, w), np.inf)
    den_w = np.zeros((F, h, w))
    marg = np.full((F, h, w), np.inf)
    with np.errstate(all="ignore"):
        for f in range(F):
            best_i, best_s, best_den, best_m = index[f], depth[f], den_w[f], marg[f]
            for i in range(int(offsets[f]), min(int(offsets[f + 1]), len(plates))):
                if not drawn[i]:
                    continue
                den = (ap[i, 0] * dx + ap[i, 1] * dy) + ap[i, 2]
                s = q[i] / den
                cand = (den != 0.0) & (s >= cam.near)
                hx, hy, hz = s * dx - cp[i, 0], s * dy - cp[i, 1], s - cp[i, 2]
                m = (hx * hx + hy * hy) + hz * hz
                if margin:
                    np.minimum(best_m, np.where(cand, np.abs(m - r2), np.inf), out=best_m)
                better = cand & (m <= r2) & (s < best_s)                       # strictly: of equal s the earlier, lower row stays
                best_s[better] = s[better]
                best_i[better] = i
                best_den[better] = den[better]
    out = dict(index=index, depth=depth)
    if colors is not None:
        colors = np.asarray(colors, np.float64)
        with np.errstate(all="ignore"):
            shade = light[0] + light[1] * np.abs(den_w) / np.sqrt((dx * dx + dy * dy) + 1.0)[None]
            v = (colors[np.maximum(index, 0)] if len(colors) else np.zeros(index.shape + (3,))) * shade[..., None]
        img = byte(v)
        img[index < 0] = byte(np.array(background, np.float64))
        out["image"] = img
    if margin:
        out["margin"] = marg
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def rigid(angles, t):
    """a 4 x 4 world -> camera matrix: rotations about x, y, z by `angles`, then the translation t"""
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3] = rz @ ry @ rx
    E[:3, 3] = t
    return E


def plates_from(centers, axes):
    """(N,3,4) rows [R | centre] with R's third column = axis exactly; the other two columns are not read by the renderer"""
    p = np.zeros((len(centers), 3, 4))
    p[:, :, 2] = axes
    p[:, :, 3] = centers
    return p


def random_discs(n, seed, E, fx, fy, cx, cy, W, H, z_range=(1.5, 4.0), spill=1.35):
    """n discs whose centres project all over the image and `spill` times past its edges (so some straddle every edge and some lie
    wholly outside), given in world coordinates through the inverse of the rigid E; drawPlate's rows for random unit normals"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(*z_range, n)
    u = (rng.uniform(-spill, spill, n) * 0.5 + 0.5) * W
    v = (rng.uniform(-spill, spill, n) * 0.5 + 0.5) * H
    cam_pts = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    world = (cam_pts - E[:3, 3]) @ E[:3, :3]                                   # R^T (p - t)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return SR.plate_rows(world, nrm)


def frames(*groups):
    """plates of several frames (an empty array for an empty frame) -> plates (N,3,4), offsets (F+1)"""
    groups = [np.asarray(g, np.float64).reshape(-1, 3, 4) for g in groups]
    return np.concatenate(groups), np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)


def palette(n, seed):
    return np.random.default_rng(seed).uniform(0.05, 0.95, (n, 3))


def degenerate_plates():
    """for the identity extrinsic and an integer cx: row 0 / 1 a duplicated plate (the lower row wins everywhere), 2 a disc edge-on to
    the pixel column dx = 0 (a' = (1, 0, 0): den = 0 exactly there), 3 behind the camera, 4 culled by near = 1e-3 at radius 0.25
    (c'_z - radius < near), 5 a plate with a NaN centre, 6 a farther disc partly hidden by rows 0 / 1"""
    centers = np.array([[0.3, 0.2, 2.0], [0.3, 0.2, 2.0], [0.1, -0.4, 1.5], [0.1, 0.0, -2.0], [0.0, 0.0, 0.25], [np.nan, 0.0, 2.0], [0.75, 0.3, 3.0]])
    axes = np.array([[0.0, 0.6, 0.8], [0.0, 0.6, 0.8], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    return plates_from(centers, axes)
