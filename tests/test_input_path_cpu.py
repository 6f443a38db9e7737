"""The batch input path without a GPU: the numpy restatement (tests/input_path_ref.py) and data.ClipSampler reproduce every array the
reference returned for fixture G18 (tools/make_input_fixture.py) exactly - the shuffled order and the start indices included -, the
cases in which the reference fails raise ValueError, the fixture satisfies the conditions the GPU tests rely on, and the new entry
point is declared, bound and exported."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import golden_npz
import input_path_ref as IR
from neural_marionette_amd import _lib
from neural_marionette_amd.data import ClipSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G18 = IR.G18


@pytest.fixture(scope="module")
def g18(golden_dir):
    return golden_npz.load(os.path.join(golden_dir, "g18_input_path.npz"))


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_entry_point_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "nm355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bint\s+nm_voxelize_batch\s*\(", hdr), "nm_voxelize_batch is not declared in include/nm355.h"
    assert "nm_voxelize_batch" in _lib.SIGNATURES and hasattr(lib, "nm_voxelize_batch")
    # the ctypes descriptor mirrors the header's struct, field for field
    body = re.search(r"typedef struct nm_clip_desc \{(.*?)\} nm_clip_desc;", hdr, flags=re.S).group(1)
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.NmClipDesc._fields_], names
    assert C.sizeof(_lib.NmClipDesc) == 56


def test_fixture_holds_numbers_only(g18):
    assert all(a.dtype.kind in "fiu" for a in g18.values())
    assert g18["meta"].tolist() == [G18[k] for k in ("seed", "G", "T", "N", "J", "dataset_seed")]


def _dataset_cases():
    for tag in ("aist", "dfaust"):
        for rate in G18["rates"]:
            for mode in [f"e{e}" for e in G18["epochs"]] + ["rand"]:
                yield f"a_{tag}_r{rate}_{mode}", tag == "aist", rate, mode, False
    yield "a_short_r1_rand", False, 1, "rand", True


@pytest.mark.parametrize("key,with_joints,rate,mode,short", list(_dataset_cases()), ids=[c[0] for c in _dataset_cases()])
def test_sampler_and_restatement_reproduce_the_datasets(g18, key, with_joints, rate, mode, short):
    seqs = IR.g18_sequences(short=short)
    T, G = G18["T"], G18["G"]
    s = ClipSampler([p.shape[0] for p, _ in seqs], T, rate, mode == "rand", random.Random(G18["dataset_seed"]), has_joints=with_joints)
    assert s.order == g18[key + "__order"].tolist(), "shuffled order"
    if mode != "rand":
        s.log_epoch(int(mode[1:]))
    padded = 0
    for i in range(len(s)):
        seq, start, pad = s.crop(i)
        assert start == int(g18[key + "__starts"][i]), (i, start)
        padded += int(pad)
        pts, jts = seqs[seq]
        r = IR.clip(pts, start, T, rate, pad, G, joints=jts if with_joints else None)
        assert not r["bad"].any()
        assert np.array_equal(IR.pack(r["vox"]), g18[key + "__vox"][i]), (key, i)
        if with_joints:
            want = g18[key + "__joints"][i]
            assert r["joints"].dtype == want.dtype == np.float32 and np.array_equal(_bits(r["joints"]), _bits(want))
    assert padded == (1 if short else 0)


@pytest.mark.parametrize("name", sorted(IR.G18_CLIPS))
def test_restatement_reproduces_normalisation_and_voxels(g18, name):
    dtype, T, N, G, scale, xt, zt = IR.G18_CLIPS[name]
    x = IR.g18_clip(name)
    assert x.dtype == np.dtype(dtype) and x.shape == (T, N, 3)
    r = IR.clip(x, 0, T, 1, False, G, scale, xt, zt)
    assert np.array_equal(_bits(r["norm"]), _bits(g18[f"b_{name}__norm"])), "normalised coordinates differ from the reference's bits"
    assert np.array_equal(r["idx"], g18[f"b_{name}__idx"])
    assert int(r["bad"].sum()) == int(g18[f"b_{name}__bad"])
    if int(g18[f"b_{name}__raised"]):
        assert r["bad"].any() and f"b_{name}__vox" not in g18          # the reference raised: there are no voxels to compare
    else:
        assert np.array_equal(IR.pack(r["vox"]), g18[f"b_{name}__vox"])


def test_fixture_conditions(g18):
    """what the GPU tests rely on: wrapped negative indices, a clip the reference refuses, both dtypes"""
    for name in ("f32_wrap", "f64_wrap", "f32_wrap40", "f64_wrap40"):
        idx = g18[f"b_{name}__idx"]
        G = IR.G18_CLIPS[name][3]
        neg = int((idx < 0).any(-1).sum())
        print(name, "rows with a wrapped index:", neg)
        assert neg >= 1 and idx.min() >= -G and int(g18[f"b_{name}__bad"]) == 0
    assert int(g18["b_f32_over__raised"]) == 1 and 0 < int(g18["b_f32_over__bad"]) < g18["b_f32_over__idx"].shape[0] * g18["b_f32_over__idx"].shape[1]
    assert g18["b_f32_over__idx"].max() >= IR.G18_CLIPS["f32_over"][3]


@pytest.mark.parametrize("pd", ["float32", "float64"])
@pytest.mark.parametrize("jd", ["float32", "float64"])
def test_joint_dtype_combinations(g18, pd, jd):
    x, j = IR.g18_joint_case(pd, jd)
    got = IR.episodic_normalization(x, 0.9, joints=j)[2]
    want = g18[f"c_{pd}_{jd}__joints"]
    assert want.dtype == (np.float32 if (pd, jd) == ("float32", "float32") else np.float64)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("G", IR.HARD_GRIDS)
def test_hard_clips_tell_float32_from_upcast_arithmetic(g18, G):
    x = g18[f"d_hard{G}__points"]
    assert x.dtype == np.float32 and x.shape == (IR.HARD_T, IR.HARD_N, 3)
    r = IR.clip(x, 0, IR.HARD_T, 1, False, G, 0.9)
    assert np.array_equal(_bits(r["norm"]), _bits(g18[f"d_hard{G}__norm"]))
    assert np.array_equal(r["idx"], g18[f"d_hard{G}__idx"]) and not r["bad"].any()
    assert np.array_equal(IR.pack(r["vox"]), g18[f"d_hard{G}__vox"])
    up = IR.clip(x, 0, IR.HARD_T, 1, False, G, 0.9, upcast=True)
    rows = int((up["idx"] != r["idx"]).any(-1).sum())
    print(f"{G}^3: {rows} rows differ under float64-upcast arithmetic, {int((up['vox'] != r['vox']).sum())} voxels")
    assert rows >= IR.HARD_MIN and rows == int(g18[f"d_hard{G}__hard"])


def test_sampler_raises_where_the_reference_fails():
    mk = lambda frames, T, rate, rc, **kw: ClipSampler([frames], T, rate, rc, random.Random(0), names=["short.npy"], **kw)
    s = mk(5, 6, 1, False)                                  # the reference: ZeroDivisionError (frames // (T * sample_rate) == 0)
    s.log_epoch(0)
    with pytest.raises(ValueError, match="short.npy"):
        s.crop(0)
    with pytest.raises(ZeroDivisionError):
        IR.reference_start(5, 6, 1, False, 0, None)
    with pytest.raises(ValueError, match="short.npy.*3 frames"):       # the reference returns a 3-frame clip
        mk(5, 6, 2, True).crop(0)
    start, padded = IR.reference_start(5, 6, 2, True, None, None)
    assert (start, len(range(start, min(padded, start + 12), 2))) == (0, 3)
    with pytest.raises(ValueError, match="short.npy.*joints"):         # the reference pads the points, not the joints
        mk(4, 6, 1, True, has_joints=True).crop(0)
    assert mk(4, 6, 1, True).crop(0) == (0, 0, True)                   # without joints the padded clip is what the reference builds
    assert mk(11, 6, 2, True).crop(0) == (0, 0, True)                  # 11 frames, stride 2: frames 0..10, nothing repeated, still T frames
    with pytest.raises(ValueError, match="log_epoch"):
        mk(40, 6, 1, False).crop(0)
    with pytest.raises(ValueError):
        IR.crop_frames(12, 8, 6, 1, False)


def test_sampler_start_rules_match_the_restated_reference():
    """every (frames, T, rate, epoch) of a small grid, both crop modes, against reference_start on the same random stream"""
    for frames in (12, 13, 23, 24, 40, 61):
        for T, rate in ((6, 1), (6, 2), (3, 4)):
            if frames < T * rate:
                continue
            for epoch in range(0, 15):
                s = ClipSampler([frames], T, rate, False, random.Random(1))
                s.log_epoch(epoch)
                want, _ = IR.reference_start(frames, T, rate, False, epoch, None)
                assert s.crop(0) == (0, want, False) and want + (T - 1) * rate < frames
            a, b = random.Random(5), random.Random(5)
            b.shuffle([0])
            s = ClipSampler([frames], T, rate, True, a)
            for _ in range(4):
                assert s.crop(0)[1] == IR.reference_start(frames, T, rate, True, None, b.randint)[0]
