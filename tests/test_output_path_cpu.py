"""The device output path without a device: the restatement tests/output_path_ref.py (which tests/test_output_path_gpu.py compares
NeuralMarionette.occupied_points with) against a result written out by hand and against the special values the occupancy test has
to honour, the two entry points in the header and the ctypes table, and the shell's argument errors, which are raised before the
library is touched."""
import os
import re

import numpy as np
import pytest
import torch

import output_path_ref as OR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_BELOW = np.nextafter(np.float32(0.5), np.float32(0))


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = (_bits(got), _bits(want)) if got.dtype.kind == "f" else (got, want)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} entries differ"


def _example():
    v = np.zeros((2, 1, 5, 5, 5), np.float32)
    v[0, 0, 4, 4, 4] = 0.5
    v[0, 0, 0, 0, 1] = 0.7
    v[0, 0, 2, 3, 0] = 0.49
    v[0, 0, 1, 2, 3] = 1.0
    v[1, 0, 3, 0, 2] = 0.9
    return v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_on_a_hand_written_example(dtype):
    """5^3, two frames: i / 2 - 1 is exact in both arithmetics; the clip's z indices run from 1 to 4, so z_len = 1.5"""
    r = OR.occupied_points(_example(), 0.5, dtype)
    idx = np.array([[0, 0, 1], [1, 2, 3], [4, 4, 4], [3, 0, 2]], np.int32)
    _same(r["indices"], idx, "indices")
    _same(r["coords"], np.array([[-1, -1, -0.5], [-0.5, 0, 0.5], [1, 1, 1], [0.5, -1, 0]], dtype), "coords")
    _same(r["offsets"], np.array([0, 3, 4], np.int64), "offsets")
    _same(r["counts"], np.array([[3, 1]], np.int64), "counts")
    _same(r["z_range"], np.array([[-0.5, 1.0]], dtype), "z_range")
    bits = np.zeros((2, 16), np.uint8)
    bits[0, 0], bits[0, 4], bits[0, 15], bits[1, 9] = 0x02, 0x40, 0x10, 0x20        # flat positions 1, 38, 124 and 77
    _same(r["bits"], bits, "bits")
    if dtype == np.float64:
        _same(r["depth"], np.array([0.0, 1.0 / 1.5, 1.0, 0.5 / 1.5], np.float64), "depth")
    else:
        assert "depth" not in r
    n = OR.occupied_points(_example(), None, dtype)                                  # nonzero mode also takes the 0.49
    _same(n["indices"], np.array([[0, 0, 1], [1, 2, 3], [2, 3, 0], [4, 4, 4], [3, 0, 2]], np.int32), "indices (nonzero)")
    _same(n["z_range"], np.array([[-1.0, 1.0]], dtype), "z_range (nonzero)")


def test_restatement_special_values():
    """0.0, -0.0, nextafter(0.5, 0), 0.5, 1.0, -1.0, +inf, NaN along the last axis: the two modes differ at nextafter(0.5, 0) and -1.0"""
    vals = np.array([0.0, -0.0, HALF_BELOW, 0.5, 1.0, -1.0, np.inf, np.nan], np.float32)
    v = np.zeros((1, 1, 8, 8, 8), np.float32)
    v[0, 0, 0, 0, :] = vals
    for dtype in (np.float64, np.float32):
        t = OR.occupied_points(v, 0.5, dtype)
        n = OR.occupied_points(v, None, dtype)
        assert t["indices"][:, 2].tolist() == [3, 4, 6, 7] and n["indices"][:, 2].tolist() == [2, 3, 4, 5, 6, 7]
        assert sorted(set(n["indices"][:, 2].tolist()) ^ set(t["indices"][:, 2].tolist())) == [2, 5]
    assert OR.occupied_points(v, float(HALF_BELOW))["indices"][:, 2].tolist() == [2, 3, 4, 6, 7]
    e = OR.occupied_points(np.zeros((2, 3, 1, 5, 5, 5), np.float32))
    _same(e["z_range"], np.array([[1e4, -1.0]] * 2), "z_range of empty clips")
    assert e["coords"].shape == (0, 3) and e["depth"].shape == (0,) and e["offsets"].tolist() == [0] * 7
    one = np.zeros((1, 1, 5, 5, 5), np.float32)
    one[0, 0, 1, 2, 3] = 1
    d = OR.occupied_points(one)["depth"]
    assert d.shape == (1,) and np.isnan(d[0])


def test_the_two_arithmetics():
    """torch's CPU `int64 / float - 1` is float32's correctly rounded division and subtraction (what the kernel's float32 path
    computes), and at the grids in use it is not the rounding of numpy's float64 result: both paths are needed"""
    differ = []
    for G in range(2, 130):
        i = np.arange(G)
        t = (torch.arange(G) / ((G - 1) / 2) - 1).numpy()
        _same(t, i.astype(np.float32) / np.float32((G - 1) / 2) - np.float32(1), f"float32 coordinates at G = {G}")
        if not np.array_equal((i / ((G - 1) / 2) - 1).astype(np.float32), t):
            differ.append(G)
    assert {8, 13, 32, 64, 96} <= set(differ)


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "nm355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym, nargs in (("nm_occupied_count", 12), ("nm_occupied_write", 12)):
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, sym + " is not declared in include/nm355.h"
        assert len(m.group(1).split(",")) == nargs
        res, args = _lib.SIGNATURES[sym]
        assert len(args) == nargs
    assert _lib.SIGNATURES["nm_occupied_count"][1][6] is _lib.C.c_float            # thr
    assert _lib.SIGNATURES["nm_occupied_write"][1][8] is _lib.C.c_int64            # capacity
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.nm_occupied_count(None, None, 1, 1, 8, 0, 0.5, 1, None, None, None, None) == _lib.NM_ERR_ARG
        assert lib.nm_occupied_write(None, None, None, None, 1, 1, 8, 1, 0, None, None, None) == _lib.NM_ERR_ARG


def test_shell_argument_errors_need_no_device():
    net = NeuralMarionette(HotPathOptions(grid_size=32))
    ok = torch.zeros(2, 1, 8, 8, 8)
    with pytest.raises(ValueError, match="device"):
        net.occupied_points(ok)                                                    # a CPU tensor
    with pytest.raises(ValueError, match=r"\(T,1,G,G,G\)"):
        net.occupied_points(torch.zeros(1, 8, 8, 8))                               # wrong rank
    with pytest.raises(ValueError, match=r"\(T,1,G,G,G\)"):
        net.occupied_points(torch.zeros(2, 1, 8, 8, 9))                            # not a cube
    with pytest.raises(ValueError, match=r"\(T,1,G,G,G\)"):
        net.occupied_points(torch.zeros(2, 2, 8, 8, 8))                            # two channels
    with pytest.raises(ValueError, match="float32"):
        net.occupied_points(ok.double())
    with pytest.raises(ValueError, match="return_depth"):
        net.occupied_points(ok, dtype=torch.float32, return_depth=True)
    with pytest.raises(ValueError, match="dtype"):
        net.occupied_points(ok, dtype=torch.float16)
    with pytest.raises(ValueError, match="capacity"):
        net.occupied_points(ok, capacity=-1)
    assert net._engine.ctx is None                                                 # the library was never asked
