"""The render path's float64 restatement tests/render_ref.py (what tests/test_render_gpu.py holds nm_render_bin / nm_render_draw to)
pinned to results derived by hand and to an independent world-space formulation, and the camera class.  No GPU."""
import json
import os

import numpy as np
import pytest

import render_ref as RR
from neural_marionette_amd import PinholeCamera

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_source.json")
EYE = np.eye(4)


def _cam(W, H, f, cx, cy, E=EYE, near=1e-3):
    return PinholeCamera(E.tolist(), f, f, cx, cy, W, H, near)


def test_disc_facing_the_camera_covers_the_lattice_points_of_a_circle():
    """a disc on the optical axis at depth z, facing the camera: s = z for every pixel, h = z (dx, dy, 0), so the covered pixels are the
    lattice points with (px - cx)^2 + (py - cy)^2 <= (f radius / z)^2.  f = 64, z = 2, radius = 0.25: the bound is 8^2 = 64, with the
    lattice points (8, 0) and (0, 8) exactly on the circle - in float64 too: dx = k / 64 and h = 2 dx are exact, m = (k^2 + l^2) / 1024
    is exact, 0.25 * 0.25 = 64 / 1024 is exact."""
    cam = _cam(33, 31, 64.0, 16.0, 15.0)
    out = RR.render(RR.plates_from([[0.0, 0.0, 2.0]], [[0.0, 0.0, 1.0]]), [0, 1], [[0.2, 0.4, 0.6]], cam, radius=0.25)
    want = np.array([[(px - 16) ** 2 + (py - 15) ** 2 <= 64 for px in range(33)] for py in range(31)])
    assert want.sum() == 197                                                   # the lattice points of the closed disc of radius 8
    assert np.array_equal(out["index"][0] == 0, want) and (out["index"][0][~want] == -1).all()
    assert (out["depth"][0][want] == 2.0).all() and np.isinf(out["depth"][0][~want]).all()
    assert (out["image"][0][want] == np.array([51, 102, 153], np.uint8)).all()      # uint8(c * 255.0), truncated
    assert (out["image"][0][~want] == 255).all()
    # the axis reversed: both faces are visible
    back = RR.render(RR.plates_from([[0.0, 0.0, 2.0]], [[0.0, 0.0, -1.0]]), [0, 1], None, cam, radius=0.25)
    assert np.array_equal(back["index"], out["index"]) and np.array_equal(back["depth"], out["depth"])


def test_occlusion_ties_and_plates_that_are_not_drawn():
    cam = _cam(48, 40, 40.0, 24.0, 20.0)
    plates = RR.degenerate_plates()
    out = RR.render(plates, [0, len(plates)], RR.palette(len(plates), 1), cam, radius=0.25, margin=True)
    idx, dep = out["index"][0], out["depth"][0]
    seen = set(np.unique(idx).tolist())
    assert seen == {-1, 0, 2, 6}, seen            # 1: the duplicate never wins; 3 behind the camera; 4 culled by near; 5 not finite
    near_only = RR.render(plates[4:5], [0, 1], None, cam, radius=0.25)
    assert (near_only["index"] == -1).all()       # c'_z - radius = 0 < near although most of the disc is in front of the near plane
    kept = RR.render(plates[4:5], [0, 1], None, _cam(48, 40, 40.0, 24.0, 20.0, near=1e-9), radius=0.2)
    assert (kept["index"] == 0).any()             # the same plate, not culled: c'_z - radius = 0.05
    # occlusion: row 6 (z = 3) lies behind rows 0 / 1 (z about 2) where they overlap, and shows beside them
    alone = RR.render(plates[6:7], [0, 1], None, cam, radius=0.25)["index"][0] == 0
    both = alone & (RR.render(plates[0:1], [0, 1], None, cam, radius=0.25)["index"][0] == 0)
    assert both.sum() >= 8 and (idx[both] == 0).all() and (idx[alone & ~both] == 6).all() and (alone & ~both).sum() >= 8
    assert (dep[idx == 0] < 2.6).all() and (dep[idx == 6] == 3.0).all()
    # reversing the row order of the duplicate changes nothing but the index that wins: still the lower one
    swapped = RR.render(plates[[1, 0, 2, 3, 4, 5, 6]], [0, len(plates)], None, cam, radius=0.25)
    assert np.array_equal(swapped["index"], out["index"]) and np.array_equal(swapped["depth"], out["depth"])
    # edge-on: a' = (1, 0, 0), cx an integer: den = 0 exactly in the pixel column px = 24, where the disc draws nothing at all; the plane
    # x = 0.1 it lies in is seen as a sliver some columns to the right (s = 0.1 / dx within 0.25 of the centre's depth 1.5)
    edge = RR.render(plates[2:3], [0, 1], None, cam, radius=0.25)["index"][0]
    assert (edge[:, 24] == -1).all() and (idx[:, 24] != 2).all()
    cols = np.unique(np.nonzero(edge == 0)[1])
    assert cols.tolist() == [27], cols             # dx = 3 / 40: s = 1.333; dx = 2 / 40: s = 2 and dx = 4 / 40: s = 1 are both 0.5 away


def test_frames_do_not_share_plates():
    cam = _cam(20, 20, 20.0, 9.5, 9.5)
    a = RR.plates_from([[0.0, 0.0, 2.0]], [[0.0, 0.0, 1.0]])
    plates, offsets = RR.frames(a, np.zeros((0, 3, 4)), a)
    out = RR.render(plates, offsets, [[1, 0, 0], [0, 1, 0]], cam, radius=0.3, background=(0.0, 0.5, 2.0))
    assert (out["index"][1] == -1).all() and (out["image"][1] == np.array([0, 127, 255], np.uint8)).all()
    assert set(np.unique(out["index"][0])) == {-1, 0} and set(np.unique(out["index"][2])) == {-1, 1}
    assert np.array_equal(out["index"][0] >= 0, out["index"][2] >= 0)


def test_image_value_nan_clamp_and_light():
    cam = _cam(9, 9, 8.0, 4.0, 4.0)
    p = RR.plates_from([[0.0, 0.0, 1.0]], [[0.0, 0.0, 1.0]])
    out = RR.render(p, [0, 1], [[np.nan, -0.5, 1.5]], cam, radius=0.2)
    assert (out["image"][0][out["index"][0] == 0] == np.array([0, 0, 255], np.uint8)).all()
    lit = RR.render(p, [0, 1], [[1.0, 1.0, 0.5]], cam, radius=0.2, light=(0.0, 1.0))
    assert lit["image"][0, 4, 4].tolist() == [255, 255, 127]                   # on the axis the ray is the disc's axis: cosine 1
    dx = 1 / 8.0
    assert lit["image"][0, 4, 5, 0] == int(255.0 / np.sqrt(dx * dx + 1.0))     # one pixel off: |den| / |d| = 1 / sqrt(dx^2 + 1)


def test_golden_camera_and_scaling():
    cam = PinholeCamera.from_open3d(GOLDEN)
    E = np.array(cam.extrinsic)
    assert np.array_equal(E[:3, :3], np.diag([1.0, -1.0, -1.0])) and E[3].tolist() == [0, 0, 0, 1]
    assert E[:3, 3].tolist() == [0.5546303168997937, -0.0035468143869429314, 3.3230607082645185]      # the translation is the last COLUMN
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height) == (829.65233682549228, 829.65233682549228, 512.0, 478.5, 1025, 958)
    assert cam.cx == cam.width / 2 - 0.5 and cam.cy == cam.height / 2 - 0.5   # open3d: the principal point is the middle pixel's centre
    with open(GOLDEN) as f:
        assert PinholeCamera.from_open3d(json.load(f)) == cam
    small = cam.scaled(128, 120)
    assert (small.width, small.height, small.cx, small.cy) == (128, 120, 63.5, 59.5) and small.extrinsic == cam.extrinsic
    assert small.fx == cam.fx * 128 / 1025 and small.fy == cam.fy * 120 / 958
    odd = cam.scaled(41, 33)                                                   # an odd size keeps the central ray on the central pixel
    assert (odd.cx, odd.cy) == (20.0, 16.0)
    dxs, dys = RR.pixel_rays(odd)
    assert dxs[16, 20] == 0.0 and dys[16, 20] == 0.0
    with pytest.raises(ValueError):
        PinholeCamera.from_open3d({"extrinsic": [1.0] * 15, "intrinsic": {}})
    with pytest.raises(ValueError):
        PinholeCamera(np.eye(4).tolist(), 0.0, 1.0, 0.0, 0.0, 4, 4)
    with pytest.raises(ValueError):
        PinholeCamera(np.eye(4).tolist(), 1.0, 1.0, float("nan"), 0.0, 4, 4)
    c = cam.c_struct()
    assert list(c.extrinsic) == [v for r in cam.extrinsic for v in r] and (c.width, c.height, c.near) == (1025, 958, 1e-3)


def _world_space_index(plates, offsets, cam, radius):
    """the same picture another way: the untransformed disc against the world-space ray o + s R^T d, o = -R^T t the camera's centre"""
    E = RR.extrinsic(cam)
    R, t = E[:3, :3], E[:3, 3]
    o = -(R.T @ t)
    dx, dy = RR.pixel_rays(cam)
    d = np.stack([dx, dy, np.ones_like(dx)], -1)
    w = d @ R                                                                  # R^T d per pixel
    F = len(offsets) - 1
    index = np.full((F,) + dx.shape, -1, np.int32)
    for f in range(F):
        best = np.full(dx.shape, np.inf)
        for i in range(offsets[f], offsets[f + 1]):
            c, a = plates[i, :, 3], plates[i, :, 2]
            if not np.isfinite(plates[i]).all() or (R[2] @ c + t[2]) - radius < cam.near:
                continue
            with np.errstate(all="ignore"):
                s = np.dot(a, c - o) / (w @ a)
                p = o + s[..., None] * w - c
                hit = np.isfinite(s) & (s >= cam.near) & ((p * p).sum(-1) <= radius * radius)
            better = hit & (s < best)
            best[better] = s[better]
            index[f][better] = i
    return index


@pytest.mark.parametrize("seed", [3, 8])
def test_world_space_formulation_agrees(seed):
    """the restatement's camera-space arithmetic against the world-space one, on every pixel whose verdicts are not within 1e-9 of
    changing (|m - radius^2| > 1e-9 for every candidate plate); those are under 1 % of the covered pixels on these seeds"""
    W, H, f = 40, 33, 45.0
    E = RR.rigid((0.3, -0.4, 0.2), (0.1, -0.2, 0.4))
    cam = _cam(W, H, f, 19.5, 16.0, E)
    a = RR.random_discs(60, seed, E, f, f, 19.5, 16.0, W, H)
    b = RR.random_discs(60, seed + 100, E, f, f, 19.5, 16.0, W, H)
    plates, offsets = RR.frames(a, b)
    ref = RR.render(plates, offsets, None, cam, radius=0.25, margin=True)
    other = _world_space_index(plates, offsets, cam, 0.25)
    covered = ref["index"] >= 0
    sure = ref["margin"] > 1e-9
    assert covered.sum() > 400 and (covered & ~sure).sum() < 0.01 * covered.sum()
    assert np.array_equal(other[sure], ref["index"][sure])
    # two plates at equal depth would make the comparison a matter of rounding too: there are none here apart from exact ties
    assert (other[sure] >= 0).sum() > 400
