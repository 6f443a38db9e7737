"""The surface path without a device: the restatement tests/surface_ref.py (which tests/test_surface_path_gpu.py compares
nm_occupied_surface and NeuralMarionette.surface_points with) against results written out by hand and against an independent
formulation of its neighbourhoods (scipy's k-d tree), the entry point in the header and the ctypes table, the shell's argument errors,
and the restatement ALONE on every input of the device tests: on the generator shells it must stay inside the two caps those tests
put on the rows they exempt - at most 5 % of a case's rows below the eigenvalue gap of 1e-3, at most 12 % with a sign the
orientation rule does not decide.  (An input that exceeds a cap is replaced; the caps stay.)"""
import os
import re

import numpy as np
import pytest
import torch

import surface_ref as SR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_moments_on_a_hand_written_example():
    """5^3: p = (2, 2, 2) with neighbours at (2, 2, 3) and (1, 2, 2) [|d|^2 = 1], (3, 3, 2) [2], (2, 2, 4) [4] and (0, 0, 0) [12]"""
    idx = np.array([[0, 0, 0], [1, 2, 2], [2, 2, 2], [2, 2, 3], [2, 2, 4], [3, 3, 2]], np.int32)
    m1 = SR.moments_brute(idx, 5, 1)[2]
    assert m1.tolist() == [3, -1, 0, 1, 1, 0, 0, 0, 0, 1]                       # d = 0, (0, 0, 1), (-1, 0, 0)
    m2 = SR.moments_brute(idx, 5, 2)[2]
    assert m2.tolist() == [4, 0, 1, 1, 2, 1, 0, 1, 0, 1]                        # and (1, 1, 0)
    m4 = SR.moments_brute(idx, 5, 4)[2]
    assert m4.tolist() == [5, 0, 1, 3, 2, 1, 0, 1, 0, 5]                        # and (0, 0, 2)
    assert SR.moments_brute(idx, 5, 12)[2].tolist() == [6, -2, -1, 1, 6, 5, 4, 5, 4, 9]              # and (-2, -2, -2)
    C = SR.covariance(m2[None])[0]
    assert C.tolist() == [[8.0, 4.0, 0.0], [4.0, 3.0, -1.0], [0.0, -1.0, 3.0]]   # n Q - S S^T
    assert SR.moments_brute(idx, 5, 8)[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]                  # from (0, 0, 0): nothing within 8,
    assert SR.moments_brute(idx, 5, 9)[0].tolist() == [2, 1, 2, 2, 1, 2, 2, 4, 4, 4]                  # (1, 2, 2) at exactly 9


@pytest.mark.parametrize("radius2", [1, 3, 6, 9, 16])
def test_brute_force_moments_equal_the_kd_tree_formulation(radius2):
    frames = [SR.hand_clip()[0, t, 0] for t in range(8)] + [SR.leak_clip()[0, t, 0] for t in range(2)] + [SR.shell_frame(32, 3), SR.shell_frame(33, 5)]
    for v in frames:
        G = v.shape[-1]
        idx = np.argwhere(v > 0).astype(np.int32)
        a, b = SR.moments_brute(idx, G, radius2), SR.moments_kdtree(idx, radius2)
        assert np.array_equal(a, b), (G, radius2, int((a != b).any(1).sum()))
        assert (a[:, 0] >= 1).all()                                            # the point itself


def test_plate_rows_restate_draw_plate():
    """the array form against the scripts' per-plate function, including the branch for a normal along -z"""
    rng = np.random.default_rng(4)
    n = rng.standard_normal((64, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[0], n[1], n[2], n[3] = (0, 0, -1), (0, 0, 1), (1, 0, 0), (1e-6, 0, -1)
    n[3] /= np.linalg.norm(n[3])
    c = rng.random((64, 3)) * 2 - 1
    rows = SR.plate_rows(c, n)
    for a in range(64):
        want = SR.draw_plate_transform(c[a], n[a])
        assert np.abs(rows[a] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), a
    assert rows[0, :, :3].tolist() == [[-1, 0, 0], [0, 1, 0], [0, 0, -1]] and rows[3, :, :3].tolist() == rows[0, :, :3].tolist()
    assert np.abs(rows[1, :, :3] - np.eye(3)).max() < 1e-6
    assert np.abs(np.einsum("nij,nj->ni", rows[4:, :, :3], np.tile([0.0, 0.0, 1.0], (60, 1))) - n[4:]).max() < 1e-3      # R e_z = n, up to the 1e-6 and 1e-8 of the script


def test_restatement_on_the_hand_made_frames():
    v = SR.hand_clip()
    r = SR.surface_points(v, 0.5, 6, base=np.tile([0.6, 0.6, 1.0], (8, 1)))
    o = r["offsets"]
    assert r["counts"].tolist() == [[1, 64, 64, 64, 8, 104, 0, 2]]
    assert r["moments"][0].tolist() == [1] + [0] * 9 and r["normals"][0].tolist() == [0, 0, 1] and r["o"][0].tolist() == [1, 1, 1]
    for t, axis in ((1, 0), (2, 1), (3, 2)):                                   # planes: no neighbour leaves the plane
        rows = slice(o[t], o[t + 1])
        assert (r["moments"][rows][:, 1 + axis] == 0).all() and (r["spread"][rows][:, 0] == 0).all()
        assert np.abs(np.abs(r["normals"][rows][:, axis]) - 1).max() < 1e-12
    line = slice(o[4], o[5])
    assert np.abs(r["spread"][line][:, :2]).max() < 1e-9 and (r["moments"][line][:, 0] >= 3).all()
    pair = r["normals"][o[7]:o[8]]
    assert pair.tolist() == [[0, 0, -1], [0, 0, 1]]                              # n = 2: (0, 0, 1), turned away from the other voxel
    assert not np.isnan(r["colors"]).any() and r["colors"].shape == (307, 3)
    d = r["depth"][5]
    assert r["colors"][5].tolist() == [0.6 * (d * 0.8 + 0.2), 0.6 * (d * 0.8 + 0.2), 1.0 * (d * 0.8 + 0.2)]


@pytest.mark.parametrize("name", list(SR.CASES))
def test_reference_stays_inside_the_caps(name):
    build, radius2, point, capped = SR.CASES[name]
    ref = SR.surface_points(build(), 0.5, radius2, point)
    gap, sign = SR.exempt_rows(ref)
    N = len(gap)
    assert N > 0
    print(f"{name}: {N} rows, {int((ref['moments'][:, 0] < 3).sum())} with n < 3, {100 * gap.mean():.2f} % below the gap, {100 * sign.mean():.2f} % sign-ambiguous")
    if capped:
        assert gap.mean() <= SR.GAP_CAP, f"{name}: {100 * gap.mean():.2f} % of the rows lie below the eigenvalue gap: choose another input"
        assert sign.mean() <= SR.SIGN_CAP, f"{name}: {100 * sign.mean():.2f} % of the rows have an undecided sign: choose another input"
    else:                                                                        # the hand-made frames: degenerate on purpose
        assert name.startswith("hand_")
    fro = np.sqrt((ref["C"] ** 2).sum((1, 2)))
    res = np.linalg.norm(np.einsum("nij,nj->ni", ref["C"], ref["normals"]) - ref["spread"][:, :1] * ref["normals"], axis=1)
    solved = ref["moments"][:, 0] >= 3
    assert (res[solved] <= 1e-12 * fro[solved]).all()                            # eigh itself, two orders inside the device test's bound


def test_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "nm355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+nm_occupied_surface\s*\(([^)]*)\)\s*;", hdr)
    assert m, "nm_occupied_surface is not declared in include/nm355.h"
    assert len(m.group(1).split(",")) == 20
    res, args = _lib.SIGNATURES["nm_occupied_surface"]
    assert len(args) == 20 and res is _lib.C.c_int
    assert args[12] is _lib.C.c_double and args[13] is _lib.C.c_double and args[14] is _lib.C.c_int64      # shade_a, shade_b, capacity
    src = open(os.path.join(ROOT, "neural_marionette_amd", "csrc", "nm_surface.hip")).read()
    assert re.search(r"^int\s+nm_occupied_surface\s*\([^{;]*?\)\s*try\s*\{", src, flags=re.M | re.S)           # a function-try-block
    assert "atomic" not in src.split("#include")[1:][-1]                           # (the header comment says "No atomics")
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        tail = (None, None, None, 0.8, 0.2, 0, None, None, None, None, None)
        assert lib.nm_occupied_surface(None, None, None, None, 1, 1, 8, 6, 0, *tail) == _lib.NM_ERR_ARG
        assert b"null ctx" in lib.nm_last_error()
        for radius2 in (0, 17):                                                  # judged before the context: the message names radius2
            assert lib.nm_occupied_surface(None, 1, 1, 1, 1, 1, 8, radius2, 0, *tail) == _lib.NM_ERR_ARG
            assert b"radius2 = %d" % radius2 in lib.nm_last_error(), lib.nm_last_error()
        for radius2 in (1, 16):
            assert lib.nm_occupied_surface(None, 1, 1, 1, 1, 1, 8, radius2, 0, *tail) == _lib.NM_ERR_ARG
            assert b"null ctx" in lib.nm_last_error()


def test_shell_argument_errors_need_no_device():
    net = NeuralMarionette(HotPathOptions(grid_size=32))
    ok = torch.zeros(2, 1, 8, 8, 8)
    for bad in (0, 17, 2.5, -1, "6", None):
        with pytest.raises(ValueError, match="radius2"):
            net.surface_points(ok, radius2=bad)
    with pytest.raises(ValueError, match="orient"):
        net.surface_points(ok, orient="inward")
    with pytest.raises(ValueError, match="add_colors"):
        net.surface_points(ok, add_colors=[0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match="shade"):
        net.surface_points(ok, shade=0.8)
    with pytest.raises(ValueError, match="surface_points: vox must be on the network's device"):
        net.surface_points(ok)                                                     # a CPU tensor: occupied_points' checks, under this name
    with pytest.raises(ValueError, match=r"surface_points: vox must be \(T,1,G,G,G\)"):
        net.surface_points(torch.zeros(2, 1, 8, 8, 9))
    with pytest.raises(ValueError, match="capacity"):
        net.surface_points(ok, capacity=-1)
    with pytest.raises(ValueError, match="return_points"):
        net._points("generate", ok, "normals")
    assert net._engine.ctx is None                                                 # the library was never asked
