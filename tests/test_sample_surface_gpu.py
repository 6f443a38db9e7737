"""Mesh sampling on the device (nm_sample_surface through NeuralMarionette.sample_surface and ClipBank.add_mesh) against the float64
numpy restatement tests/sample_ref.py, which tests/test_sample_surface_cpu.py pins to hand-worked numbers.

What is compared how.  The restatement is fed the DEVICE'S OWN areas for steps 2-4 of the contract, so nothing here depends on the
device's float64 square root being correctly rounded:
  areas        against numpy within 1 float64 ulp: the cross product and the sum are the same roundings, the square root is the only
               operation that may differ.  Largest difference seen on an MI355X over every case of this file: 0 ulp.
  normals      within 1 float32 ulp of float32(c / sqrt(n2)) (one float64 square root or division that flips the float32 rounding);
               exact zeros for degenerate faces.  Largest difference seen: 0 ulp.
  cum          bit for bit (int64) against the restatement's integer weights of the device's areas.
  uniforms     bit for bit against the restatement's Philox4x32-10 in the seeded mode.
  face_index   equal at every sample; points bit for bit at every sample.  No sample is left out: the integer table has no
               near-boundary ambiguity.

Path switches of the implementation (csrc/nm_sample.h), each tested on both sides:
  NM_SAMPLE_SCAN_ONE = 16384     one workgroup scans a frame of up to 16384 faces; 16385 faces are scanned in chunks of 4096 (chunk sums,
                                 their scan, the chunks) - with T = 3, so that the chunk offsets of later frames are used.
  NM_SAMPLE_LDS_COARSE = 2048    the draw kernel stages the coarse table (every 64th entry of cum) in LDS up to 2048 entries = 131072 faces;
                                 131073 faces are searched in global memory.
and count = 2500 crosses the 1024 samples a workgroup of the draw kernel takes.

Without the feature (the parent commit) this module fails at import: there is no tests/sample_ref.py, the library has no
nm_sample_surface and NeuralMarionette no sample_surface."""
import numpy as np
import pytest
import torch

import sample_ref as S
from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth, _lib
from neural_marionette_amd.data import ClipBank

pytestmark = pytest.mark.gpu

TOP = 1.0 - 2.0 ** -53
_NET = []
SEEN = dict(area_ulp=0, normal_ulp=0)


def _net():
    if not _NET:
        o = HotPathOptions(grid_size=32)
        net = NeuralMarionette(o)
        net.load_state_dict(synth.make_state_dict(o, seed=23, variant="peaky"))
        _NET.append(net.cuda().eval())
    return _NET[0]


def _np(t):
    return t.detach().cpu().numpy()


def _dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()


def _mesh(T, F, seed, degenerate=True):
    """random triangles over random vertices, frame t scaled by 2^(3 t): another exponent of amax in every frame"""
    rng = np.random.default_rng(seed)
    V = max(3, F // 2 + 7)
    v = rng.standard_normal((T, V, 3)) * (2.0 ** (3 * np.arange(T)))[:, None, None]
    tri = rng.integers(0, V, (F, 3))
    if degenerate and F >= 5:
        tri[0] = [4, 4, 2]                                          # zero-area faces: face 0 and one in the middle
        tri[F // 2] = [1, 1, 1]
    else:
        tri[-1] = [0, 1, 2]                                         # (a small mesh keeps one face with area for certain)
    return v, tri


def _check(what, v, tri, out, u=None, seed=None, bad_faces=0, empty_frames=0):
    """every output of one call against the restatement; v, tri: the numpy arrays the device was given"""
    got = {k: _np(x) for k, x in out.items()}
    T, F, count = v.shape[0], tri.shape[0], got["points"].shape[1]
    assert got["points"].shape == (T, count, 3) and got["points"].dtype == np.float32
    assert got["normals"].shape == (T, count, 3) and got["face_index"].shape == (T, count) and got["face_index"].dtype == np.int32
    assert got["areas"].shape == (T, F) and got["areas"].dtype == np.float64 and got["cum"].dtype == np.int64
    # the uniforms
    if u is None:
        assert np.array_equal(got["uniforms"], S.uniforms(seed, T, count)), f"{what}: the device's uniforms are not the restatement's"
    else:
        assert np.array_equal(got["uniforms"], u)
    # step 1 by itself
    area, _, _ = S.face_records(v, tri)
    fin = np.isfinite(area)
    assert np.array_equal(np.isfinite(got["areas"]), fin) and np.array_equal(np.isnan(got["areas"]), np.isnan(area)), f"{what}: non-finite areas differ"
    a_ulp = int(S.ulp_distance(np.where(fin, got["areas"], 0.0), np.where(fin, area, 0.0)).max())
    # steps 2 - 4 on the device's areas
    ref = S.sample(v, tri, got["uniforms"], areas=got["areas"])
    assert np.array_equal(got["cum"].view(np.uint64), ref["cum"]), f"{what}: cum differs"
    nbad = int((got["face_index"] != ref["face_index"]).sum())
    assert nbad == 0, f"{what}: face_index differs at {nbad} of {T * count} samples"
    n_ulp = int(S.ulp_distance(got["normals"], ref["normals"]).max())
    pbad = int((got["points"].view(np.uint32) != ref["points"].view(np.uint32)).any(axis=-1).sum())
    print(f"{what}: T = {T}, F = {F}, count = {count}: areas differ by at most {a_ulp} ulp, normals by {n_ulp} ulp, {pbad} points differ")
    SEEN["area_ulp"], SEEN["normal_ulp"] = max(SEEN["area_ulp"], a_ulp), max(SEEN["normal_ulp"], n_ulp)
    assert a_ulp <= 1, f"{what}: areas differ from numpy's by {a_ulp} float64 ulp"
    assert n_ulp <= 1, f"{what}: normals differ by {n_ulp} float32 ulp"
    assert pbad == 0, f"{what}: {pbad} points differ in their bits"
    assert int(got["bad_faces"]) == ref["bad_faces"] == bad_faces and int(got["empty_frames"]) == ref["empty_frames"] == empty_frames
    return got, ref


def _run(what, T, F, count, vdt, tdt, seed, u=None):
    v, tri = _mesh(T, F, seed=1000 + F)
    v = v.astype(vdt)
    out = _net().sample_surface(_dev(v, vdt), _dev(tri, tdt), count=count, seed=seed, u=None if u is None else _dev(u, np.float64),
                                return_tables=True)
    return _check(what, v, tri, out, u=u, seed=seed)


@pytest.mark.parametrize("F,count,T,vdt,tdt", [
    (1, 1, 1, np.float64, np.int32), (2, 255, 3, np.float32, np.int64), (63, 256, 1, np.float64, np.int64),
    (64, 257, 3, np.float32, np.int32), (65, 1000, 1, np.float64, np.int32), (257, 255, 3, np.float32, np.int32),
    (1000, 1000, 3, np.float64, np.int64), (1000, 2500, 3, np.float32, np.int64)])
def test_shapes_and_dtypes(F, count, T, vdt, tdt):
    got, _ = _run(f"F={F}", T, F, count, vdt, tdt, seed=(F << 33) + count)                 # (seeds with a high word: the key's second half)
    if T == 3 and F >= 5:
        e = np.frexp(got["areas"].max(axis=1))[1]
        assert len(set(e.tolist())) == 3, "the frames were meant to have three different exponents of amax"


@pytest.mark.parametrize("F,T", [(16384, 1), (16385, 3), (131072, 1), (131073, 1)])
def test_both_sides_of_every_path_switch(F, T):
    got, _ = _run(f"F={F}", T, F, 1000, np.float32, np.int32, seed=F)
    assert len(np.unique(got["face_index"] // 4096)) >= min(4, F // 4096), "the picks were meant to spread over the chunks"


def test_crafted_uniforms():
    """u0 that lands on p = Cum[i] - 1 and p = Cum[i], u0 = 0 and 1 - 2^-53, u1 + u2 exactly 1 and just above"""
    T, F = 3, 257
    v, tri = _mesh(T, F, seed=77)
    dv, dt = _dev(v, np.float64), _dev(tri, np.int32)
    cum = _np(_net().sample_surface(dv, dt, count=1, return_tables=True)["cum"])
    picks = [0, 1, F // 2 - 1, F // 2, 63, 64, 127, 128, F - 2]
    rows = []
    for t in range(T):
        W = int(cum[t, -1])
        r = [(0.0, 0.0, 0.0), (TOP, 0.0, 0.0), (TOP, TOP, TOP), (0.0, 0.25, 0.75), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5 + 2.0 ** -53),
             (0.5, 0.5 + 2.0 ** -52, 0.5), (0.25, 0.75, 0.75), (0.75, TOP, 2.0 ** -53)]
        for i in picks:
            c = int(cum[t, i])
            for p in (c - 1, c):
                if 0 <= p < W:
                    r.append((S.u0_for(p, W), 0.125, 0.5))
        rows.append(r)
    u = np.array(rows, dtype=np.float64)
    out = _net().sample_surface(dv, dt, count=u.shape[1], u=_dev(u, np.float64), return_tables=True)
    got, ref = _check("crafted", v, tri, out, u=u)
    for t in range(T):                                                 # the crafted u0 do what they were made for
        p = S.pick_index(u[t, 9:, 0], int(cum[t, -1]))
        assert np.isin(p, np.concatenate([cum[t, picks] - 1, cum[t, picks]]).astype(np.uint64)).all()
        assert (cum[t, got["face_index"][t]].astype(np.uint64) > S.pick_index(u[t, :, 0], int(cum[t, -1]))).all()
    assert (got["face_index"][:, 1] == np.array([np.flatnonzero(np.diff(np.concatenate([[0], c])))[-1] for c in cum])).all()   # u0 = TOP: the last face with weight


def test_edge_cases():
    net = _net()
    t = 2.0 ** -17
    base = np.array([[0, 0, 0], [1, 1, 0], [2, 2, 0], [0, 0, 0], [2, 0, 0], [0, 2, 0], [3, 3, 3], [3, 3, 3], [4, 4, 4],
                     [5, 0, 0], [5 + t, 0, 0], [5, t, 0], [6, 0, 0], [7, 0, 0], [6, 1, 0], [np.inf, 0, 0]], np.float64)
    # frame 0 as the CPU test's (face 0 collinear, face 2 with two equal vertices, face 3 below amax 2^-32) plus a face with an
    # infinite vertex; frame 1 is one point: no surface
    v = np.stack([base, np.full_like(base, 2.5)])
    tri = np.concatenate([np.arange(15).reshape(5, 3), [[12, 13, 15]]])
    for vdt, tdt in ((np.float64, np.int32), (np.float32, np.int64)):
        vv = v.astype(vdt)
        out = net.sample_surface(_dev(vv, vdt), _dev(tri, tdt), count=300, seed=5, return_tables=True)
        got, _ = _check("degenerate", vv, tri, out, seed=5, empty_frames=1)
        assert set(got["face_index"][0].tolist()) == {1, 4} and not got["face_index"][1].any()
        assert (got["points"][1] == 2.5).all() and not got["normals"][1].any()
        assert got["cum"][0].tolist() == [0, 2 ** 31, 2 ** 31, 2 ** 31, 5 * 2 ** 29, 5 * 2 ** 29] and not got["cum"][1].any()
        with pytest.raises(ValueError, match="1 frames without surface"):
            net.sample_surface(_dev(vv, vdt), _dev(tri, tdt), count=300, seed=5, check=True)
    # indices outside the vertices: the vertices are the inside of a larger buffer whose first and last rows are NaN, so a read
    # through index -1 or V would show; the faces have no area, are counted once (not once a frame) and are never picked
    rng = np.random.default_rng(8)
    V, F = 40, 130
    buf = torch.full((1, V + 2, 3), float("nan"), dtype=torch.float64, device="cuda")
    vin = rng.standard_normal((1, V, 3))
    buf[:, 1:-1] = _dev(vin, np.float64)
    tri = rng.integers(0, V, (F, 3))
    tri[0], tri[64], tri[129] = [-1, 2, 3], [2, V, 3], [1, 2, 2 ** 31 - 1]
    dv = buf[:, 1:-1]
    assert dv.is_contiguous()
    for tdt in (np.int32, np.int64):
        out = net.sample_surface(dv, _dev(tri, tdt), count=500, seed=6, return_tables=True)
        got, _ = _check("bad indices", vin, tri, out, seed=6, bad_faces=3)
        assert got["areas"][0, [0, 64, 129]].tolist() == [0, 0, 0] and not np.isin(got["face_index"], [0, 64, 129]).any()
        assert np.isfinite(got["points"]).all()
        with pytest.raises(ValueError, match="3 faces with a vertex index outside"):
            net.sample_surface(dv, _dev(tri, tdt), count=500, seed=6, check=True)
    net.sample_surface(dv, _dev(tri[1:64], np.int32), count=5, check=True)              # a clean mesh passes the check


def test_seeds_and_frames():
    net = _net()
    v, tri = _mesh(3, 257, seed=3)
    dv, dt = _dev(v, np.float32), _dev(tri, np.int32)
    a = net.sample_surface(dv, dt, count=1000, seed=9, return_tables=True)
    b = net.sample_surface(dv, dt, count=1000, seed=9, return_tables=True)
    c = net.sample_surface(dv, dt, count=1000, seed=10, return_tables=True)
    for k in ("points", "normals", "face_index", "areas", "cum", "uniforms"):
        assert torch.equal(a[k], b[k]), f"{k} differs between two calls with one seed"
    assert not torch.equal(a["uniforms"], c["uniforms"]) and not torch.equal(a["points"], c["points"])
    assert not torch.equal(a["uniforms"][0], a["uniforms"][1]) and not torch.equal(a["uniforms"][1], a["uniforms"][2])
    assert torch.equal(a["areas"], c["areas"]) and torch.equal(a["cum"], c["cum"])
    d = net.sample_surface(dv, dt, count=1000, seed=9)                                    # the default call returns no tables
    assert sorted(d) == ["bad_faces", "empty_frames", "face_index", "normals", "points"] and torch.equal(d["points"], a["points"])


def test_add_mesh_feeds_the_input_path():
    """ClipBank.add_mesh then voxelize_batch = voxelize_batch on bank.add of the same samples, bit for bit, at G = 32"""
    net = _net()
    T = 4
    v, tri = _mesh(1, 500, seed=12, degenerate=False)
    v = np.concatenate([v * (1.0 + 0.1 * k) + 0.05 * k for k in range(T)]).astype(np.float32)
    dv, dt = _dev(v, np.float32), _dev(tri, np.int64)
    bank = ClipBank("cuda:0")
    i = bank.add_mesh(net, dv, dt, count=3000, seed=4)
    pts = net.sample_surface(dv, dt, count=3000, seed=4)["points"]
    j = bank.add(_np(pts))
    assert (i, j) == (0, 1) and bank.points[0].dtype == torch.float32 and tuple(bank.points[0].shape) == (T, 3000, 3)
    assert torch.equal(bank.points[0], bank.points[1])
    a = net.voxelize_batch(bank, [i], [0], T, check=True)
    b = net.voxelize_batch(bank, [j], [0], T, check=True)
    assert tuple(a["vox"].shape) == (1, T, 1, 32, 32, 32) and torch.equal(a["vox"], b["vox"]) and torch.equal(a["bbox"], b["bbox"])
    assert 100 < int(a["vox"][0, 0].sum()) <= 3000
    k = bank.add_mesh(net, dv, dt, count=64, joints=np.zeros((T, 5, 3), np.float32))
    assert bank.joints[k] is not None and tuple(bank.points[k].shape) == (T, 64, 3)


def test_argument_errors_on_the_device():
    net = _net()
    v, tri = _mesh(2, 10, seed=1)
    dv, dt = _dev(v, np.float64), _dev(tri, np.int32)
    with pytest.raises(ValueError):
        net.sample_surface(dv, dt.cpu())
    with pytest.raises(ValueError):
        net.sample_surface(dv, dt, count=8, u=torch.zeros(2, 9, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        net.sample_surface(dv.transpose(0, 1), dt)
    # the C ABI judges its arguments itself
    eng = net._engine
    ctx = eng.ready()
    lib = ctx.lib
    need = lib.nm_sample_surface_workspace(2, 10)
    assert need > 0 and need % 256 == 0 and lib.nm_sample_surface_workspace(2, 0) == 0 and lib.nm_sample_surface_workspace(0, 10) == 0
    assert lib.nm_sample_surface_workspace(1, 2 ** 21) > 0 and lib.nm_sample_surface_workspace(1, 2 ** 21 + 1) == 0
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    pts, nrm = torch.zeros(2, 8, 3, device="cuda"), torch.zeros(2, 8, 3, device="cuda")
    idx, cnt = torch.zeros(2, 8, dtype=torch.int32, device="cuda"), torch.full((2,), -7, dtype=torch.int32, device="cuda")

    def call(T=2, V=v.shape[1], F=10, count=8, sc=scratch.data_ptr(), nbytes=need, points=pts.data_ptr()):
        return lib.nm_sample_surface(ctx.handle, dv.data_ptr(), 1, dt.data_ptr(), 0, T, V, F, count, 0, None, sc, nbytes, points, nrm.data_ptr(),
                                     idx.data_ptr(), None, cnt.data_ptr())
    for kw, word in ((dict(T=0), b"T = 0"), (dict(V=0), b"V = 0"), (dict(F=0), b"F = 0"), (dict(count=0), b"count = 0"),
                     (dict(F=2 ** 21 + 1), b"2^21"), (dict(nbytes=need - 1), b"scratch"), (dict(sc=scratch.data_ptr() + 8), b"aligned"),
                     (dict(points=None), b"null")):
        assert call(**kw) == _lib.NM_ERR_ARG, kw
        assert word in lib.nm_last_error(), (kw, lib.nm_last_error())
    assert call(count=2 ** 31) == _lib.NM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert cnt.tolist() == [-7, -7] and not pts.any(), "a refused call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0] and pts.any()
    with pytest.raises(_lib.NmError):
        eng.call("nm_sample_tables", None, 2, 10, None, None)


def test_largest_differences_seen():
    """the docstring's figures: 0 ulp expected for the areas (a correctly rounded float64 square root) and for the normals"""
    print(f"largest difference over this module: areas {SEEN['area_ulp']} float64 ulp, normals {SEEN['normal_ulp']} float32 ulp")
    assert SEEN["area_ulp"] <= 1 and SEEN["normal_ulp"] <= 1
