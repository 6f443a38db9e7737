"""Motion retargeting without a GPU: the three entry points are declared and bound, the float64 restatement (tests/retarget_ref.py)
reproduces what the reference computed for fixture G16 (tools/make_retarget_fixture.py), and the fixture and the stand-in inputs of the
GPU tests satisfy the conditions those tests rely on."""
import os
import re

import numpy as np

import golden_npz
import retarget_ref as RR
from neural_marionette_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nm_retarget_bind", "nm_retarget_fk", "nm_retarget_pose")
MARGIN_FREE = 4e-4          # 2 sqrt(3) 1e-4 = 3.5e-4: a selection with a larger margin cannot flip when the keypoints move by 1e-4
MARGIN_CAP = 0.02           # share of the fixture's points that may fall below it (left out of the free-run comparison)
MARGIN_OP = 1e-9            # no op-level selection may be closer than this


def _g16(golden_dir):
    return golden_npz.load(os.path.join(golden_dir, "g16_retarget32.npz"))


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "nm355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/nm355.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"libnm355.so does not export {name}"
    assert "#define NM_ABI_VERSION 1" in hdr


def test_restatement_reproduces_the_reference_on_g16(golden_dir):
    g = _g16(golden_dir)
    _, _, _, _, points, _, _ = RR.g16_inputs(dict(zip(("G", "T", "N", "weights", "source", "target", "pick", "eps_source", "eps_target"), g["meta"].tolist())))
    b, pos, out = RR.retarget(g["parents"], g["order"], g["source_keypoints"][0], g["target_keypoints"][0, 0], g["R"], g["R_bind"], g["offset"],
                              points, float(g["hardness"]), float(g["threshold"]))
    assert np.array_equal(b["dense"].view(np.uint32), g["dense"].view(np.uint32)), "skin weights differ from the reference's bit patterns"
    assert np.array_equal(b["nearest"], g["nearest"])
    e_kp = np.abs(pos.astype(np.float64) - g["keypoints"][0, :, :, :3]).max()
    e_pts = np.abs(out - g["points"]).max()
    print("restatement vs G16: retargeted keypoints %.2e, points %.2e" % (e_kp, e_pts))
    assert e_kp < 1e-12 and e_pts < 1e-12
    assert np.array_equal(g["keypoints"][..., 3], g["source_keypoints"][..., 3])
    # the dense form of the blend agrees with the two-term form
    assert np.abs(RR.pose_dense(b["dense"], points, g["target_keypoints"][0, 0], g["R_bind"], g["R"], pos) - out).max() < 1e-12


def test_g16_conditions(golden_dir):
    g = _g16(golden_dir)
    K = g["parents"].shape[0]
    assert set(g.files) >= {"source_keypoints", "target_keypoints", "R", "R_bind", "offset", "parents", "order", "keypoints", "nearest", "margin",
                            "dense", "points", "points_sens"}
    assert all(a.dtype.kind in "fiu" for a in g.values()), "G16 holds arrays of numbers only"
    root = int(g["order"][0])
    invalid = g["target_keypoints"][0, 0, :, 3] < np.float32(g["threshold"])
    assert not invalid[root], "the fixture's root must be valid (the reference's function does not return otherwise)"
    assert 1 <= int(invalid.sum()) <= K - 3 and int(invalid.sum()) == int(g["invalid"])
    share = float((g["margin"] < MARGIN_FREE).mean())
    print("G16: %d invalid joints, %.2f %% of the margins below %.0e (smallest %.2e), points_sens %.3e" % (
        invalid.sum(), 100 * share, MARGIN_FREE, g["margin"].min(), float(g["points_sens"])))
    assert share <= MARGIN_CAP
    assert 0 < float(g["points_sens"]) < 1e-2
    assert (g["nearest"] != root).all() and not invalid[g["nearest"]].any()
    rows = (g["dense"] != 0).sum(-1)
    assert rows.max() <= 2 and rows.min() >= 1


def test_standin_inputs_have_clear_selections():
    """the op-level GPU tests compare selections wherever the restatement's margin exceeds 1e-9 and assert that nothing is excluded"""
    want = {1: 3, 2: 6, 3: 4}
    for seed in (1, 2, 3):
        s = RR.standin(seed)
        b = RR.bind(s["parents"], s["root"], s["points"], s["keypoints"], s["R_bind"])
        assert int((s["keypoints"][:, 3] < np.float32(0.2)).sum()) == want[seed]
        assert b["margin"].min() > MARGIN_OP, (seed, b["margin"].min())
        assert (b["margin"] < MARGIN_FREE).mean() <= MARGIN_CAP


def test_walk_stops_at_an_invalid_root():
    """the one place without a reference behaviour: the restatement's ancestor walk ends at the root even when the root is invalid"""
    s = RR.standin(4, N=500, K=6)
    kp = s["keypoints"].copy()
    kp[:, 3] = 0.05                                     # every joint invalid, the root too
    bones, invalid = RR.bone_points(s["parents"], kp)
    assert invalid.all()
    root = s["root"]
    for k in range(6):
        want = kp[k, :3] if k == root else (kp[k, :3] + kp[root, :3]) / np.float32(2)
        assert np.array_equal(bones[k], want)
    b = RR.bind(s["parents"], root, s["points"], kp)
    assert (b["child"] == 0).all()                      # every distance is the value 1e4: the first index wins
