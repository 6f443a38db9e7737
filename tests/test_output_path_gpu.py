"""The output path on the device (nm_occupied_count / nm_occupied_write through the C ABI and through
NeuralMarionette.occupied_points, and the drivers' return_points) against the numpy / torch-CPU restatement
tests/output_path_ref.py, which tests/test_output_path_cpu.py pins to a hand-written result.

Every comparison is bit for bit: the outputs are integers, bit masks, and coordinates that are one correctly rounded division and
one subtraction of small integers, in float64 as numpy computes them or in float32 as torch does, so there is no tolerance to
derive.  Floats are compared as bit patterns; the one exception is WHICH NaN a 0 / 0 gives (the depth of a clip whose points share
one z): IEEE 754 leaves an invalid operation's sign and payload to the implementation, so NaNs must sit at the same places and
everything else must have the same bits.

Shapes: G = 5 (125 voxels: no multiple of 4 or 64, so odd frames start 4 bytes off a 16-byte boundary and take the 4-byte loads),
8, 13 (2197 voxels: 35 words, one chunk, a partial last word), 16 and 32 (512 words: eight chunks of 64 words per frame)."""
import functools

import numpy as np
import pytest
import torch

import output_path_ref as OR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth, _lib

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
HALF_BELOW = np.nextafter(np.float32(0.5), np.float32(0))
SPECIAL = np.array([0.0, -0.0, HALF_BELOW, 0.5, 1.0, -1.0, np.inf, np.nan], np.float32)
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


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs at other places"
        a, b = _bits(got)[~nan], _bits(want)[~nan]
    else:
        a, b = got, want
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} entries differ"


def _check(out, ref, what, rows=None):
    """every key of the restatement's dict that the call returned; `rows`: only the first rows of the per-point arrays"""
    for k, want in ref.items():
        if k not in out:
            continue
        got = _np(out[k]) if isinstance(out[k], torch.Tensor) else out[k]
        if rows is not None and k in ("coords", "indices", "depth"):
            got, want = got[:rows], want[:rows]
        _same(got, want, f"{what}: {k}")


def _fill(kind, B, T, G, seed=0):
    """the test patterns, (B,T,1,G,G,G) float32"""
    rng = np.random.default_rng(seed)
    V = G ** 3
    v = np.zeros((B * T, V), np.float32)
    if kind == "empty":
        pass
    elif kind == "ones":
        v[:] = 1
    elif kind == "empty_frame":                 # one empty frame between full ones
        v[:] = 1
        v[1 % (B * T)] = 0
    elif kind == "empty_clip":                  # one empty clip among non-empty ones
        v[:] = rng.random(v.shape) < 0.3
        v.reshape(B, T, V)[B // 2] = 0
    elif kind == "first":
        v[0, 0] = 1
    elif kind == "last":
        v[-1, -1] = 1
    elif kind == "word_edges":
        p = np.arange(V)
        v[:, (p % 64 == 0) | (p % 64 == 63)] = 1
    elif kind == "random2":
        v[:] = rng.random(v.shape) < 0.02
    elif kind == "random50":
        v[:] = rng.random(v.shape)              # values in [0, 1): half of them reach 0.5, none is zero
        v[rng.random(v.shape) < 0.5] = 0
    elif kind == "one_voxel_clip":              # a clip with a single point: its depth is 0 / 0
        v[:] = rng.random(v.shape) < 0.1
        v.reshape(B, T, V)[0] = 0
        v.reshape(B, T, V)[0, T - 1, V // 3] = 1
    else:
        raise KeyError(kind)
    return v.reshape(B, T, 1, G, G, G)


@functools.lru_cache(maxsize=None)
def _case(kind, B, T, G, threshold, dtype):
    v = _fill(kind, B, T, G)
    return v, OR.occupied_points(v, threshold, NP[dtype])


def _abi(net, vox, threshold, dtype, capacity=None, sentinel=None, want=("idx", "coords", "depth")):
    """the two entry points as a C caller uses them: returns the restatement's dict (numpy), rows = capacity or the total"""
    eng = net._engine
    eng.ready()
    B, T, G = vox.shape[0], vox.shape[1], vox.shape[3]
    F, W, f64 = B * T, (G ** 3 + 63) // 64, int(dtype == F64)
    bits = torch.full((F, W), -1, device="cuda", dtype=torch.int64)
    offsets = torch.full((F + 1,), -1, device="cuda", dtype=torch.int64)
    zi = torch.full((B, 2), -5, device="cuda", dtype=torch.int32)
    zr = torch.full((B, 2), 7.0, device="cuda", dtype=dtype)
    eng.call("nm_occupied_count", _lib.ptr(vox), B, T, G, 1 if threshold is None else 0, 0.0 if threshold is None else float(threshold), f64,
             bits.data_ptr(), offsets.data_ptr(), _lib.ptr(zi), _lib.ptr(zr))
    total = int(offsets[-1].item())
    rows = total if capacity is None else capacity
    alloc = max(rows, total) + 8
    fill = 0 if sentinel is None else sentinel
    idx = torch.full((alloc, 3), int(fill), device="cuda", dtype=torch.int32) if "idx" in want else None
    coords = torch.full((alloc, 3), float(fill), device="cuda", dtype=dtype) if "coords" in want else None
    depth = torch.full((alloc,), float(fill), device="cuda", dtype=F64) if f64 and "depth" in want else None
    eng.call("nm_occupied_write", bits.data_ptr(), offsets.data_ptr(), _lib.ptr(zi), B, T, G, f64, rows, _lib.ptr(idx), _lib.ptr(coords),
             _lib.ptr(depth))
    torch.cuda.synchronize()
    out = dict(offsets=_np(offsets), counts=_np(offsets[1:] - offsets[:-1]).reshape(B, T), z_range=_np(zr), z_idx_range=_np(zi),
               bits=_np(bits.view(torch.uint8).view(F, W * 8)), total=total)
    for k, t in (("indices", idx), ("coords", coords), ("depth", depth)):
        if t is not None:
            out[k] = _np(t)
    return out


SIZES = [(G, B, T) for G in (5, 8, 13, 32) for B, T in ((1, 1), (2, 3), (3, 5))]


@pytest.mark.parametrize("G,B,T", SIZES, ids=[f"G{g}_B{b}_T{t}" for g, b, t in SIZES])
def test_grid_sizes_modes_and_arithmetics(G, B, T):
    """both modes and both arithmetics with every optional output, through the ABI and through the shell"""
    net = _net()
    for threshold in (0.5, None):
        for dtype in (F64, F32):
            v, ref = _case("random50", B, T, G, threshold, dtype)
            vox = torch.from_numpy(v).cuda()
            total = int(ref["offsets"][-1])
            assert 0 < total < B * T * G ** 3
            a = _abi(net, vox, threshold, dtype)
            assert a["total"] == total
            _check(a, ref, f"ABI {threshold} {dtype}", rows=total)
            out = net.occupied_points(vox, threshold, dtype, return_indices=True, return_depth=dtype == F64, return_bits=True)
            assert set(out) == {"coords", "offsets", "counts", "z_range", "indices", "bits"} | ({"depth"} if dtype == F64 else set())
            assert tuple(out["coords"].shape) == (total, 3) and out["coords"].dtype == dtype and out["bits"].dtype == torch.uint8
            _check(out, ref, f"shell {threshold} {dtype}")
            if B == 1:                                                  # one clip without the batch axis
                _check(net.occupied_points(vox[0], threshold, dtype), ref, "shell, (T,1,G,G,G)")
            plain = net.occupied_points(vox, threshold, dtype)
            assert set(plain) == {"coords", "offsets", "counts", "z_range"}
            assert torch.equal(vox.cpu(), torch.from_numpy(v))           # the input is not binarised in place


PATTERNS = [(k, G) for G in (13, 32) for k in ("empty", "empty_frame", "empty_clip", "ones", "first", "last", "word_edges", "random2",
                                               "random50", "one_voxel_clip")]


@pytest.mark.parametrize("kind,G", PATTERNS, ids=[f"{k}_G{g}" for k, g in PATTERNS])
def test_patterns(kind, G):
    """B = 2 clips of T = 3 frames.  'ones' at G = 32 is the 196 608-row case: every word and chunk boundary is a rank boundary"""
    net = _net()
    B, T = 2, 3
    v, ref = _case(kind, B, T, G, 0.5, F64)
    vox = torch.from_numpy(v).cuda()
    out = net.occupied_points(vox, 0.5, F64, return_indices=True, return_depth=True, return_bits=True)
    _check(out, ref, kind)
    total = int(ref["offsets"][-1])
    _check(_abi(net, vox, None, F32), _case(kind, B, T, G, None, F32)[1], kind + " (ABI, nonzero, float32)", rows=total)
    zr = _np(out["z_range"])
    if kind == "empty":
        assert total == 0 and zr.tolist() == [[1e4, -1.0]] * B
    if kind == "empty_clip":
        assert zr[B // 2].tolist() == [1e4, -1.0] and total > 0
    if kind == "ones":
        assert total == B * T * G ** 3
        p = np.arange(G ** 3)
        want = np.tile(np.stack([p // (G * G), p // G % G, p % G], -1), (B * T, 1)).astype(np.int32)
        assert np.array_equal(_np(out["indices"]), want)
    if kind in ("first", "last"):
        assert total == 1 and _np(out["indices"]).tolist() == ([[0, 0, 0]] if kind == "first" else [[G - 1] * 3])
        assert _np(out["offsets"]).tolist() == ([0] + [1] * (B * T) if kind == "first" else [0] * (B * T) + [1])
    if kind in ("first", "last", "one_voxel_clip"):
        d = _np(out["depth"])
        n0 = int(ref["offsets"][T])                                    # clip 0's rows
        one = slice(0, n0) if kind != "last" else slice(total - 1, total)
        assert np.isnan(d[one]).all() and d[one].size == 1 and not np.isnan(np.delete(d, np.arange(total)[one])).any()


def test_special_values_beside_word_boundaries():
    """0.0, -0.0, nextafter(0.5, 0), 0.5, 1.0, -1.0, +inf and NaN on both sides of the boundaries between 64-voxel words (G = 16: 64
    words), in an aligned and - by a one-element shift of the buffer - an unaligned frame; the modes differ exactly where the
    restatement says: at nextafter(0.5, 0) and -1.0"""
    net = _net()
    G, V = 16, 16 ** 3
    v = np.zeros((2, V), np.float32)
    for m in range(1, V // 64):
        v[:, 64 * m - 1] = SPECIAL[m % 8]
        v[:, 64 * m] = SPECIAL[(m + m // 8) % 8]
    for side in (63, 0):
        got = v[0, np.arange(V) % 64 == side]
        assert all(np.any(_bits(got) == _bits(SPECIAL[i:i + 1])[0]) for i in range(8))
    v = v.reshape(1, 2, 1, G, G, G)
    shifted = torch.zeros(v.size + 1, device="cuda")[1:].view(v.shape)          # 4 bytes off the allocation's alignment
    shifted.copy_(torch.from_numpy(v))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for vox in (torch.from_numpy(v).cuda(), shifted):
        res = {}
        for threshold in (0.5, None):
            for dtype in (F64, F32):
                ref = OR.occupied_points(v, threshold, NP[dtype])
                _check(net.occupied_points(vox, threshold, dtype, return_indices=True, return_depth=dtype == F64, return_bits=True), ref,
                       f"{threshold} {dtype}")
                res[threshold] = _abi(net, vox, threshold, dtype)
                _check(res[threshold], ref, f"ABI {threshold} {dtype}", rows=int(ref["offsets"][-1]))
        differ = np.unpackbits(res[0.5]["bits"] ^ res[None]["bits"], axis=1, bitorder="little")[:, :V].astype(bool)
        flat = v.reshape(2, V)
        assert np.array_equal(differ, (flat == HALF_BELOW) | (flat == -1.0)) and differ.any()
    t = net.occupied_points(torch.from_numpy(v).cuda(), float(HALF_BELOW), return_bits=True)
    _check(t, OR.occupied_points(v, float(HALF_BELOW)), "threshold nextafter(0.5, 0)")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_capacity(dtype):
    """rows at or past the capacity are not written (the buffers keep their sentinel), offsets holds the true counts"""
    net = _net()
    v, ref = _case("random2", 2, 3, 32, 0.5, dtype)
    vox = torch.from_numpy(v).cuda()
    total = int(ref["offsets"][-1])
    assert total > 64
    for capacity in (0, total - 1, total + 5):
        a = _abi(net, vox, 0.5, dtype, capacity=capacity, sentinel=-77)
        n = min(capacity, total)
        _check(a, ref, f"capacity {capacity}", rows=n)
        assert a["total"] == total
        for k in ("indices", "coords", "depth"):
            if k in a:
                assert len(a[k]) >= total + 8 and (a[k][n:] == -77).all(), f"capacity {capacity}: {k} written past row {n}"
        out = net.occupied_points(vox, 0.5, dtype, capacity=capacity, return_indices=True, return_depth=dtype == F64)
        assert len(out["coords"]) == len(out["indices"]) == capacity
        _check(out, ref, f"shell, capacity {capacity}", rows=n)
    only = _abi(net, vox, 0.5, dtype, sentinel=-77, want=("idx",))                    # coords and depth NULL
    _check(only, ref, "indices alone", rows=total)
    assert "coords" not in only


def test_repeatability_and_workspace_reuse():
    net = _net()
    kw = dict(return_indices=True, return_depth=True, return_bits=True)
    v, ref = _case("random50", 2, 3, 32, 0.5, F64)
    vox = torch.from_numpy(v).cuda()
    a = net.occupied_points(vox, **kw)
    b = net.occupied_points(vox, **kw)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    v2, ref2 = _case("random50", 3, 5, 13, 0.5, F64)                                  # another shape on the same context
    _check(net.occupied_points(torch.from_numpy(v2).cuda(), **kw), ref2, "second shape")
    _check(net.occupied_points(vox, **kw), ref, "first shape again")
    eng = net._engine
    for args, code in (((None, 1, 1, 8, 0, 0.5, 1, None, None, None, None), _lib.NM_ERR_ARG),
                       ((_lib.ptr(vox), 0, 1, 32, 0, 0.5, 1, 1, 1, 1, 1), _lib.NM_ERR_ARG),
                       ((_lib.ptr(vox), 1, 1, 1, 0, 0.5, 1, 1, 1, 1, 1), _lib.NM_ERR_ARG),
                       ((_lib.ptr(vox), 1, 1, 8, 2, 0.5, 1, 1, 1, 1, 1), _lib.NM_ERR_ARG),
                       ((_lib.ptr(vox), 4, 8, 512, 0, 0.5, 1, 1, 1, 1, 1), _lib.NM_ERR_UNSUPPORTED)):
        assert eng.ctx.lib.nm_occupied_count(eng.ctx.handle, *args) == code          # (judged before any pointer is used)
    for args, code in (((None, 1, 1, 1, 1, 8, 1, 4, None, None, None), _lib.NM_ERR_ARG),
                       ((1, 1, 1, 1, 1, 8, 0, 4, None, None, 1), _lib.NM_ERR_ARG),       # depth with float32 arithmetic
                       ((1, 1, 1, 1, 1, 8, 1, -1, None, None, None), _lib.NM_ERR_ARG),
                       ((1, 1, 1, 4, 8, 512, 1, 4, None, None, None), _lib.NM_ERR_UNSUPPORTED)):
        assert eng.ctx.lib.nm_occupied_write(eng.ctx.handle, *args) == code


def test_drivers_return_points():
    """sample_generation / sample_interpolation / generate with return_points: `points` is the restatement applied to the returned
    raw voxels (a clip per sample), every other key is bit-identical to the same call without the flag"""
    net = _net()
    G, Tc, Tg, S, Z = 32, 3, 2, 2, 128
    clip = synth.figure_clip(1, net.Tcond + 2, G, seed=3).cuda()
    gen_kw = dict(Tgen=Tg, sample_num=S, eps_post=synth.make_eps((Tc, S, Z), 5).cuda(), eps_prior=synth.make_eps((Tg, S, Z), 6).cuda())
    T = 4
    int_kw = dict(sample_rate=2, sample_num=S, eps_a=synth.make_eps((T, S, Z), 7).cuda(), eps_b=synth.make_eps((T, S, Z), 8).cuda())
    acts = {"detector": True, "learner": True}
    g_kw = dict(eps_post=synth.make_eps((net.Tcond, 10, 1, Z), 9).cuda(), eps_prior=synth.make_eps((2, 1, Z), 10).cuda())
    runs = (("generation", lambda **k: net.sample_generation(clip[0, :Tc].contiguous(), **gen_kw, **k), "voxels_raw"),
            ("interpolation", lambda **k: net.sample_interpolation(clip[0, :T].contiguous(), **int_kw, **k), "voxels_raw"),
            ("generate", lambda **k: net.generate(clip, acts, **g_kw, **k), "gen"))
    for name, run, raw in runs:
        with torch.no_grad():
            plain, pts = run(), run(return_points=True)
        assert set(pts) == set(plain) | {"points"} and "points" not in plain, name
        for k, a in plain.items():
            b = pts[k]
            if isinstance(a, torch.Tensor):
                assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{name}: {k} changed"
            else:
                assert a == b, f"{name}: {k} changed"
        ref = OR.occupied_points(_np(pts[raw]), 0.5)
        assert set(pts["points"]) == {"coords", "offsets", "counts", "z_range", "depth"}
        assert int(ref["offsets"][-1]) > 0, name + ": the decoder gave no voxel at 0.5, the case checks nothing"
        _check(pts["points"], ref, name)
