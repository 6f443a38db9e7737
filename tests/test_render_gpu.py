"""The render path on the device (nm_render_bin + nm_render_draw through the C ABI, NeuralMarionette.render_plates / render_frames)
against the float64 numpy restatement tests/render_ref.py, which tests/test_render_cpu.py pins to hand-derived results and to a
world-space formulation.

What is compared how:
  index   torch.equal to the restatement on every pixel, no exemptions.
  depth   bit for bit (the library is built with -ffp-contract=off, float64 division is correctly rounded: the ground the output
          path's bit-for-bit float64 coordinates stand on).
  image   exact with the flat light (1, 0); within one uint8 level with light (0.4, 0.6), whose square root is the one operation here
          whose last bit on the device nobody has checked.
A pixel that differs is a finding about the kernel's operation order, not a reason for a tolerance.

Shapes: 40 x 33 pixels (3 x 3 tiles of 16 x 16, the right and bottom ones partial) with F = 3 frames of which the middle one is empty,
about 300 discs per non-empty frame, some across every image edge and some wholly outside; the hand-made degenerate plates of
render_ref.degenerate_plates (a tie, an edge-on disc, one behind the camera, one culled by near, a NaN centre); one 16 x 16 image - a
single tile - under 3 * NM_RENDER_CHUNK = 768 discs (csrc/nm_render.h: the draw kernel stages a tile's plates through LDS 256 at a
time), so the chunk loop and its barriers run three times; and the surface path's G = 32 shells end to end through the golden camera."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import render_ref as RR
import surface_ref as SR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, PinholeCamera, synth, _lib

pytestmark = pytest.mark.gpu

F64 = torch.float64
NM_RENDER_CHUNK = 256                                                         # csrc/nm_render.h
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


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{what} differs"


def _compare(got, ref, what, lit=False):
    """index / depth / image of one render (numpy or tensors, any leading shape) against the restatement's"""
    got = {k: (_np(v) if isinstance(v, torch.Tensor) else v) for k, v in got.items()}
    shape = ref["index"].shape
    if "index" in got:
        g = got["index"].reshape(shape)
        bad = int((g != ref["index"]).sum())
        print(f"{what}: {int((ref['index'] >= 0).sum())} covered pixels of {g.size}, index differs on {bad}")
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(ref["index"])), f"{what}: index differs on {bad} pixels"
    if "depth" in got:
        _bits_equal(got["depth"].reshape(shape), ref["depth"], f"{what}: depth")
    if "image" in got and "image" in ref:
        g = got["image"].reshape(shape + (3,))
        err = int(np.abs(g.astype(np.int32) - ref["image"].astype(np.int32)).max(initial=0))
        print(f"{what}: image max |difference| {err} levels")
        assert err <= (1 if lit else 0), f"{what}: image differs by {err} levels"


def _abi(net, plates, offsets, colors, cam, radius, light=(1.0, 0.0), background=None, capacity=None, want=("index", "depth", "image"), slack=8):
    """nm_render_bin + nm_render_draw as a C caller uses them, into buffers that hold a sentinel"""
    eng = net._engine
    eng.ready()
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    N, F = len(plates), len(offsets) - 1
    H, W = cam.height, cam.width
    nt = F * ((W + 15) // 16) * ((H + 15) // 16)
    p, o = dev(plates, np.float64), dev(offsets, np.int64)
    c = dev(colors, np.float64) if colors is not None else None
    xf = torch.full((N + 1, 8), -77.0, device="cuda", dtype=F64)
    rect = torch.full((N + 1, 4), -77, device="cuda", dtype=torch.int32)
    toff = torch.full((nt + 2,), -77, device="cuda", dtype=torch.int64)
    cs = cam.c_struct()
    eng.call("nm_render_bin", p.data_ptr(), o.data_ptr(), F, N, C.byref(cs), radius, xf.data_ptr(), rect.data_ptr(), toff.data_ptr())
    total = int(toff[nt].item())
    assert int(toff[nt + 1].item()) == -77 and (xf[N] == -77).all() and (rect[N] == -77).all()
    cap = total if capacity is None else capacity
    lst = torch.full((cap + slack,), -77, device="cuda", dtype=torch.int32)
    shapes = dict(index=((F * H * W + slack,), torch.int32), depth=((F * H * W + slack,), F64), image=((F * H * W * 3 + slack,), torch.uint8))
    buf = {k: torch.full(s, 77 if d == torch.uint8 else -77, device="cuda", dtype=d) for k, (s, d) in shapes.items() if k in want}
    bg = None if background is None else (C.c_double * 3)(*background)
    raw = lambda t: None if t is None else t.data_ptr()
    eng.call("nm_render_draw", xf.data_ptr(), rect.data_ptr(), o.data_ptr(), toff.data_ptr(), raw(c), F, N, C.byref(cs), radius, light[0], light[1], bg,
             cap, lst.data_ptr(), *[raw(buf.get(k)) for k in ("index", "depth", "image")])
    torch.cuda.synchronize()
    n = dict(index=F * H * W, depth=F * H * W, image=F * H * W * 3)
    for k, t in buf.items():
        assert (t[n[k]:] == (77 if k == "image" else -77)).all(), f"{k} written past its end"
    assert (lst[cap:] == -77).all(), "list written past the capacity"
    assert int(toff[nt].item()) == total
    out = {k: _np(t[:n[k]]) for k, t in buf.items()}
    out.update(total=total, tile_offsets=_np(toff[:nt + 1]), list=_np(lst[:cap]), rect=_np(rect[:N]))
    return out


W0, H0, FOC, CX0, CY0, RAD = 40, 33, 45.0, 19.5, 16.0, 0.25


@functools.lru_cache(maxsize=None)
def _scene():
    """F = 3, the middle frame empty; colours with a NaN row, rows below 0 and above 1"""
    E = RR.rigid((0.3, -0.4, 0.2), (0.1, -0.2, 0.4))
    cam = PinholeCamera(E.tolist(), FOC, FOC, CX0, CY0, W0, H0)
    a = RR.random_discs(300, 3, E, FOC, FOC, CX0, CY0, W0, H0, spill=1.8)
    b = RR.random_discs(310, 103, E, FOC, FOC, CX0, CY0, W0, H0, spill=1.8)
    plates, offsets = RR.frames(a, np.zeros((0, 3, 4)), b)
    colors = RR.palette(len(plates), 5)
    colors[::7] = np.random.default_rng(6).uniform(-0.5, 1.5, colors[::7].shape)
    seen = np.unique(RR.render(plates, offsets, None, cam, radius=RAD)["index"])[1:]
    assert len(seen) > 100 and (seen % 7 == 0).sum() >= 5                      # rows with colours outside [0, 1] are on screen
    colors[seen[3]] = np.nan                                                   # and so are two rows with a NaN
    colors[seen[-2], 1] = np.nan
    flat = RR.render(plates, offsets, colors, cam, radius=RAD, background=(0.25, 0.5, 1.0))
    lit = RR.render(plates, offsets, colors, cam, radius=RAD, light=(0.4, 0.6), background=(0.25, 0.5, 1.0))
    return cam, plates, offsets, colors, flat, lit


def test_random_discs_over_partial_tiles_and_an_empty_frame():
    net = _net()
    cam, plates, offsets, colors, flat, lit = _scene()
    cp, _, _, drawn = RR.plate_terms(plates, cam, RAD)
    u, v = cam.cx + cam.fx * cp[:, 0] / cp[:, 2], cam.cy + cam.fy * cp[:, 1] / cp[:, 2]
    rpx = cam.fx * RAD / cp[:, 2]
    for name, lo, hi in (("left", u - rpx < 0, u + rpx > 0), ("right", u - rpx < W0 - 1, u + rpx > W0 - 1), ("top", v - rpx < 0, v + rpx > 0),
                         ("bottom", v - rpx < H0 - 1, v + rpx > H0 - 1)):
        assert (lo & hi & drawn).sum() >= 5, f"the scene has no discs across the {name} edge"
    assert ((u + 2 * rpx < 0) | (u - 2 * rpx > W0)).sum() >= 20, "the scene has no discs outside the image"
    assert (flat["index"][1] == -1).all() and np.isnan(colors[np.unique(flat["index"])[1:]]).any(1).sum() == 2
    a = _abi(net, plates, offsets, colors, cam, RAD, background=(0.25, 0.5, 1.0))
    _compare(a, flat, "abi, flat light")
    assert (a["image"].reshape(3, H0, W0, 3)[1] == np.array([63, 127, 255], np.uint8)).all()          # the empty frame: background only
    nt = 3 * 3
    assert (np.diff(a["tile_offsets"]) >= 0).all() and (np.diff(a["tile_offsets"])[nt:2 * nt] == 0).all() and a["tile_offsets"][-1] == a["total"]
    # every list holds rows of its own frame only
    for t in range(3 * nt):
        rows = a["list"][a["tile_offsets"][t]:a["tile_offsets"][t + 1]]
        f = t // nt
        assert ((rows >= offsets[f]) & (rows < offsets[f + 1])).all() and len(set(rows.tolist())) == len(rows), t
    b = _abi(net, plates, offsets, colors, cam, RAD, light=(0.4, 0.6), background=(0.25, 0.5, 1.0))
    _compare(b, lit, "abi, light (0.4, 0.6)", lit=True)
    # any subset of the outputs; NULL background is white
    only = _abi(net, plates, offsets, None, cam, RAD, want=("depth",))
    _compare(only, flat, "abi, depth alone")
    white = _abi(net, plates, offsets, colors, cam, RAD, want=("image",))
    assert (white["image"].reshape(3, H0, W0, 3)[1] == 255).all()


def test_shell_and_run_to_run_identity():
    net = _net()
    cam, plates, offsets, colors, flat, lit = _scene()
    pts = dict(plates=torch.from_numpy(plates).cuda(), offsets=torch.from_numpy(offsets).cuda(), colors=torch.from_numpy(colors).cuda())
    kw = dict(radius=RAD, background=(0.25, 0.5, 1.0), return_index=True, return_depth=True)
    a = net.render_plates(pts, cam, **kw)
    assert set(a) == {"image", "bin_total", "index", "depth"} and tuple(a["image"].shape) == (1, 3, H0, W0, 3) and a["image"].dtype == torch.uint8
    assert tuple(a["index"].shape) == (1, 3, H0, W0) and a["index"].dtype == torch.int32 and a["depth"].dtype == F64
    _compare(a, flat, "render_plates")
    b = net.render_plates(pts, cam, **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between two runs"
    l1 = net.render_plates(pts, cam, light=(0.4, 0.6), **kw)
    l2 = net.render_plates(pts, cam, light=(0.4, 0.6), **kw)
    _compare(l1, lit, "render_plates, light (0.4, 0.6)", lit=True)
    for k in l1:
        assert torch.equal(l1[k], l2[k]), f"{k} differs between two runs"
    plain = net.render_plates(dict(pts, counts=torch.zeros(3, 1)), cam, radius=RAD)
    assert set(plain) == {"image", "bin_total"} and tuple(plain["image"].shape) == (3, 1, H0, W0, 3)
    # no plates at all
    empty = dict(plates=torch.zeros(0, 3, 4, device="cuda", dtype=F64), offsets=torch.zeros(3, device="cuda", dtype=torch.int64),
                 colors=torch.zeros(0, 3, device="cuda", dtype=F64))
    e = net.render_plates(empty, cam, return_index=True, return_depth=True)
    assert int(e["bin_total"]) == 0 and (e["index"] == -1).all() and torch.isinf(e["depth"]).all() and (e["image"] == 255).all()


def test_degenerate_plates():
    """the hand-made cases of tests/test_render_cpu.py: a duplicated plate (the lower row wins), an edge-on disc whose den is exactly 0
    in the pixel column dx = 0, a plate behind the camera, one culled by near, one with a NaN centre, an occluded one"""
    net = _net()
    cam = PinholeCamera(np.eye(4).tolist(), 40.0, 40.0, 24.0, 20.0, 48, 40)
    plates = RR.degenerate_plates()
    colors = RR.palette(len(plates), 1)
    ref = RR.render(plates, [0, len(plates)], colors, cam, radius=0.25)
    a = _abi(net, plates, np.array([0, len(plates)]), colors, cam, 0.25)
    _compare(a, ref, "degenerate")
    idx = a["index"].reshape(40, 48)
    assert set(np.unique(idx).tolist()) == {-1, 0, 2, 6} and (idx[:, 24] != 2).all()
    assert (a["rect"][[3, 4, 5], 0] > a["rect"][[3, 4, 5], 1]).all(), "plates that are not drawn have an empty rectangle"
    swapped = _abi(net, plates[[1, 0, 2, 3, 4, 5, 6]], np.array([0, len(plates)]), colors[[1, 0, 2, 3, 4, 5, 6]], cam, 0.25)
    assert np.array_equal(swapped["index"], a["index"]) and np.array_equal(swapped["depth"], a["depth"])


def test_chunk_loop_on_a_single_tile():
    """one 16 x 16 image = one tile, 3 * NM_RENDER_CHUNK = 768 discs all over it: the draw kernel's list is longer than the
    NM_RENDER_CHUNK = 256 plates (csrc/nm_render.h) it stages in LDS at a time, so its chunk loop and barriers run three times (the
    last chunk partial or full as the culling leaves it)"""
    net = _net()
    E = RR.rigid((-0.2, 0.1, 0.5), (0.0, 0.1, 0.2))
    cam = PinholeCamera(E.tolist(), 20.0, 20.0, 7.5, 7.5, 16, 16)
    plates = RR.random_discs(3 * NM_RENDER_CHUNK, 21, E, 20.0, 20.0, 7.5, 7.5, 16, 16, spill=1.1)
    offsets = np.array([0, len(plates)])
    colors = RR.palette(len(plates), 22)
    ref = RR.render(plates, offsets, colors, cam, radius=0.12)
    a = _abi(net, plates, offsets, colors, cam, 0.12)
    assert a["total"] > 2 * NM_RENDER_CHUNK, a["total"]
    assert len(np.unique(ref["index"])) > 60
    _compare(a, ref, "one tile, 768 discs")


def test_bin_capacity():
    """the list capacity at exactly the true total, generous, and too small.  Too small: nothing is written past the capacity (the
    sentinels _abi checks), tile_offsets' last entry is still the true total, and the image is incomplete - each pixel shows the nearest
    of the plates that made it into the lists, so it is never nearer than the full picture's"""
    net = _net()
    cam, plates, offsets, colors, flat, _ = _scene()
    total = _abi(net, plates, offsets, colors, cam, RAD)["total"]
    for cap in (total, total + 1000):
        a = _abi(net, plates, offsets, colors, cam, RAD, background=(0.25, 0.5, 1.0), capacity=cap)
        assert a["total"] == total
        _compare(a, flat, f"capacity {cap}")
    for cap in (total // 2, 1, 0):
        a = _abi(net, plates, offsets, colors, cam, RAD, capacity=cap)
        assert a["total"] == total and a["tile_offsets"][-1] == total
        d, i = a["depth"].reshape(flat["depth"].shape), a["index"].reshape(flat["index"].shape)
        assert (d >= flat["depth"]).all() and ((i == flat["index"]) | (d > flat["depth"])).all()
        assert (i >= -1).all() and (i < len(plates)).all()
    assert (i == -1).all()                                                       # capacity 0: background only
    pts = dict(plates=torch.from_numpy(plates).cuda(), offsets=torch.from_numpy(offsets).cuda(), colors=torch.from_numpy(colors).cuda())
    kw = dict(radius=RAD, background=(0.25, 0.5, 1.0), return_index=True, return_depth=True)
    _compare(net.render_plates(pts, cam, bin_capacity=total, **kw), flat, "render_plates, exact bin_capacity")
    big = net.render_plates(pts, cam, bin_capacity=total + 4096, **kw)
    _compare(big, flat, "render_plates, generous bin_capacity")
    small = net.render_plates(pts, cam, bin_capacity=total // 3, **kw)
    assert int(small["bin_total"]) == int(big["bin_total"]) == total
    assert "INCOMPLETE" in NeuralMarionette.render_plates.__doc__


@functools.lru_cache(maxsize=None)
def _shells():
    v = SR.shell_clip(2, 3, 32, 3)
    base = np.tile([0.6, 1.0, 0.6], (6, 1))
    ref = SR.surface_points(v, 0.5, 6, None, base=base, shade_ab=(0.8, 0.2))
    cam = PinholeCamera.from_open3d(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_source.json")).scaled(128, 120)
    pic = RR.render(ref["plates"], ref["offsets"], ref["colors"], cam, radius=0.06, margin=True)
    return v, ref, cam, pic


def test_render_frames_end_to_end():
    """render_frames on the surface path's G = 32 shells (2 x 3 frames) through the golden camera scaled to 128 x 120, radius 0.06 so
    that neighbouring plates (grid pitch 2 / 31) overlap and occlude.  Two comparisons:
      - against the restatement on the DEVICE's own points: index, depth and image exact, no exemptions (the renderer's contract);
      - against surface_ref.surface_points followed by the restatement.  The device's normals are its Jacobi solver's, the reference's
        numpy.linalg.eigh's; they agree to about 1e-13 (tests/test_surface_path_gpu.py: |n x n_ref| <= 1e-9 above the eigenvalue gap,
        and this input has no row below it, which the test asserts), so a disc's edge moves by that much and a verdict can change only
        where |m - radius^2| is that small: index is compared on every pixel whose margin exceeds 1e-9 - as test_render_cpu.py
        compares the two formulations - and depth within 1e-9 there.  The sign-ambiguous rows of the surface path (n . o within 1e-6
        of 0; 2 of 3593 rows here) may come out flipped, and drawPlate's axis of -n is not minus its axis of n: the 1e-6 and 1e-8 in
        its lines move it by up to 4e-6.  The pixels such a row's disc hits, or misses by |m - radius^2| <= 1e-6, are not compared.
        Compared pixels must be over 99 % of the covered ones."""
    net = _net()
    v, ref, cam, pic = _shells()
    gap, _ = SR.exempt_rows(ref)
    assert not gap.any()
    vox = torch.from_numpy(v).cuda()
    out = net.render_frames(vox, cam, 0.5, radius2=6, base_colors=(0.6, 1.0, 0.6), shade=(0.8, 0.2), radius=0.06, return_index=True,
                            return_depth=True, return_points=True)
    assert tuple(out["image"].shape) == (2, 3, 120, 128, 3) and tuple(out["index"].shape) == (2, 3, 120, 128)
    pts = out["points"]
    assert torch.equal(pts["colors"].cpu(), torch.from_numpy(ref["colors"])) and torch.equal(pts["offsets"].cpu(), torch.from_numpy(ref["offsets"]))
    own = RR.render(_np(pts["plates"]), _np(pts["offsets"]), _np(pts["colors"]), cam, radius=0.06)
    _compare(out, own, "render_frames against the restatement on the device's points")
    again = net.render_plates(pts, cam, radius=0.06, return_index=True, return_depth=True)
    for k in ("image", "index", "depth"):
        assert torch.equal(out[k], again[k]), k
    idx, dep = _np(out["index"]).reshape(pic["index"].shape), _np(out["depth"]).reshape(pic["depth"].shape)
    covered, sure = pic["index"] >= 0, pic["margin"] > 1e-9
    _, sign = SR.exempt_rows(ref)
    for r in np.nonzero(sign)[0]:
        f = int(np.searchsorted(ref["offsets"], r, side="right")) - 1
        one = RR.render(ref["plates"][r:r + 1], [0, 1], None, cam, radius=0.06, margin=True)
        sure[f] &= (one["index"][0] < 0) & (one["margin"][0] > 1e-6)
    print(f"end to end: {int(covered.sum())} covered pixels, {int((covered & ~sure).sum())} not compared ({int(sign.sum())} sign-ambiguous rows), "
          f"{int((idx != pic['index']).sum())} differ from the reference pipeline")
    assert covered.sum() > 2000 and (covered & ~sure).sum() < 0.01 * covered.sum()
    assert np.array_equal(idx[sure], pic["index"][sure])
    both = sure & covered
    assert (np.abs(dep[both] - pic["depth"][both]) <= 1e-9).all() and np.isinf(dep[sure & ~covered]).all()
    img = _np(out["image"]).reshape(pic["image"].shape)
    assert np.array_equal(img[sure], pic["image"][sure])                         # the same rows, the same colours, the flat light


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
    # nm_render_bin(ctx, plates, offsets, F, rows, camera, radius, xf, rect, tile_offsets): pointers that are never used
    ok = [1, 1, 1, 4, cam(), 0.03, 1, 1, 1]
    cases = [(0, None, ARG), (1, None, ARG), (2, 0, ARG), (3, -1, ARG), (3, 2 ** 31, UNS), (4, None, ARG), (5, 0.0, ARG), (5, -1.0, ARG), (5, nan, ARG),
             (5, inf, ARG), (6, None, ARG), (7, None, ARG), (8, None, ARG)] + [(4, cam(**kw), code) for kw, code in cams]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_render_bin(h, *args) == code, ("bin", pos, val)
    assert lib.nm_render_bin(None, *ok) == ARG
    assert b"render_bin" in lib.nm_last_error()
    # nm_render_draw(ctx, xf, rect, offsets, tile_offsets, colors, F, rows, camera, radius, light_a, light_b, background, capacity, list, index, depth, image)
    ok = [1, 1, 1, 1, 1, 1, 4, cam(), 0.03, 1.0, 0.0, None, 8, 1, 1, 1, 1]
    cases = [(0, None, ARG), (1, None, ARG), (2, None, ARG), (3, None, ARG), (4, None, ARG), (5, 0, ARG), (6, -1, ARG), (6, 2 ** 31, UNS), (7, None, ARG),
             (8, 0.0, ARG), (8, nan, ARG), (12, -1, ARG), (13, None, ARG)] + [(7, cam(**kw), code) for kw, code in cams]
    for pos, val, code in cases:
        args = list(ok)
        args[pos] = val
        assert lib.nm_render_draw(h, *args) == code, ("draw", pos, val)
    assert lib.nm_render_draw(None, *ok) == ARG
    nothing = list(ok)
    nothing[14] = nothing[15] = nothing[16] = None                               # every output NULL: nothing to do, nothing launched
    assert lib.nm_render_draw(h, *nothing) == 0
    # the shells
    cam0, plates, offsets, colors, _, _ = _scene()
    pts = dict(plates=torch.from_numpy(plates).cuda(), offsets=torch.from_numpy(offsets).cuda(), colors=torch.from_numpy(colors).cuda())
    with pytest.raises(ValueError, match="colors"):
        net.render_plates({k: pts[k] for k in ("plates", "offsets")}, cam0)
    with pytest.raises(ValueError, match="camera"):
        net.render_plates(pts, dict(fx=1.0))
    with pytest.raises(ValueError, match="radius"):
        net.render_plates(pts, cam0, radius=0.0)
    with pytest.raises(ValueError, match="light"):
        net.render_plates(pts, cam0, light=1.0)
    with pytest.raises(ValueError, match="background"):
        net.render_plates(pts, cam0, background=(1.0, 1.0))
    with pytest.raises(ValueError, match="bin_capacity"):
        net.render_plates(pts, cam0, bin_capacity=-1)
    with pytest.raises(ValueError, match="plates"):
        net.render_plates(dict(pts, plates=pts["plates"].float()), cam0)
    with pytest.raises(ValueError, match="device"):
        net.render_plates(dict(pts, colors=pts["colors"].cpu()), cam0)
    with pytest.raises(ValueError, match="2\\^31"):
        net.render_plates(pts, PinholeCamera(np.eye(4).tolist(), 1.0, 1.0, 0.0, 0.0, 32768, 32768))
    with pytest.raises(ValueError, match="base_colors"):
        net.render_frames(torch.zeros(1, 1, 8, 8, 8, device="cuda"), cam0, base_colors=None)
