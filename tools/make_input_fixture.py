#!/usr/bin/env python3
"""Generate tests/golden/g18_input_path[.partN].npz: what the REFERENCE's input path returns on the seeded sequences of
tests/input_path_ref.py, recorded so that the library, the restatement and ClipSampler are pinned to it without the reference tree.

  python tools/make_input_fixture.py --reference DIR      # DIR: a checkout of the reference implementation

The reference's utils.dataset_utils is imported as it is, and dataset.dataset with an empty stand-in for torchvision (it imports
torchvision.transforms and never uses it).  Its AIST and DFAUST classes read .npy files under data/ relative to the working directory,
so the tool writes the seeded sequences into a temporary directory and runs there.  The start index a dataset object picks is not
part of what it returns: the tool records it by wrapping the module's crop_sequence.  Only arrays are written:

  (a) a_<dataset>_r<rate>_<mode>__{order, starts, vox, joints}: AIST(is_eval=1) and DFAUST items 0..2 in order, for sample_rate 1 and
      2, the epoch-selected crop at epochs 0, 1, 7 and the random crop; a_short_r1_rand: DFAUST on a 4-frame file (padded clip).
  (b) b_<clip>__{norm, vox, idx, bad, raised}: episodic_normalization + voxelize on float32 / float64 clips, with translations that
      give wrapped negative indices, and one clip with rows >= G (the reference raises: raised = 1, no vox).
  (c) c_<points dtype>_<joints dtype>__joints: the normalised joints of the four dtype combinations.
  (d) d_hard<G>__{points, norm, vox, idx, hard}: a float32 clip of 1000 columns cut from a large seeded pool so that it holds the
      pool's six box-extreme points and every column with a row whose index differs under float64-upcast arithmetic.
Voxels are bit-packed.  idx and bad come from the restatement, after the tool has checked that the restatement reproduces the
reference's normalised coordinates and voxels bit for bit.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_npz  # noqa: E402
import input_path_ref as IR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
POOL_COLUMNS = 1_000_000


def _options(**kw):
    o = dict(is_binarized=1, is_eval=0, Ttot=IR.G18["T"], sample_rate=1, grid_size=IR.G18["G"], random_crop=0, seed=IR.G18["dataset_seed"],
             debug=0, nbatch=0)
    o.update(kw)
    return argparse.Namespace(**o)


def _write_tree(seqs, names):
    for (p, j), name in zip(seqs, names):
        for d, a in (("data/aist_plusplus_smpl_joints/surface/train", p), ("data/aist_plusplus_smpl_joints/joints/train", j),
                     ("data/D-FAUST/surface/train/s0", p)):
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, name), a)


def _items(DS, cls, names, starts_log, arrays, key, epoch=None, **opt):
    """items 0 .. n-1 of one dataset object, in order; checks the restatement on each."""
    is_aist = cls is DS.AIST
    ds = cls(True, _options(is_eval=int(is_aist), **opt))
    order = [names.index(os.path.basename(p)) for p in ds.seq_path]
    if epoch is not None:
        ds.log_epoch(epoch)
    vox, joints, starts = [], [], []
    for i in range(len(ds)):
        del starts_log[:]
        item = ds[i]
        starts.append(starts_log[0])
        v = (item[0] if is_aist else item).numpy()
        assert v.shape == (opt.get("Ttot", IR.G18["T"]), 1) + (IR.G18["G"],) * 3, v.shape
        vox.append(IR.pack(v))
        if is_aist:
            joints.append(item[1])
    arrays[key + "__order"] = np.array(order, dtype=np.int32)
    arrays[key + "__starts"] = np.array(starts, dtype=np.int32)
    arrays[key + "__vox"] = np.stack(vox)
    if is_aist:
        arrays[key + "__joints"] = np.stack(joints)
    return order, starts


def _hard_clip(G, DU):
    """(d): columns of a seeded float32 pool (HARD_T, M, 3) - the six box extremes, the columns with an upcast-sensitive row, filled up
    to HARD_N with the pool's first columns."""
    M = POOL_COLUMNS
    while True:
        pool = IR.sequence(IR.G18["seed"], 3000 + G, IR.HARD_T, M, np.float32)
        a, _ = IR.episodic_normalization(pool, 0.9)
        b, _ = IR.episodic_normalization(pool, 0.9, upcast=True)
        ia, _ = IR.voxel_indices(a, G)
        ib, _ = IR.voxel_indices(b, G)
        hard_cols = np.nonzero((ia != ib).any(-1).any(0))[0]
        flat = pool.reshape(-1, 3)
        ext = sorted({int(flat[:, k].argmin()) % M for k in range(3)} | {int(flat[:, k].argmax()) % M for k in range(3)})
        cols = list(dict.fromkeys(ext + hard_cols.tolist()))
        if len(hard_cols) >= IR.HARD_MIN and len(cols) <= IR.HARD_N:
            break
        if len(cols) > IR.HARD_N:
            cols = list(dict.fromkeys(ext + hard_cols.tolist()[:IR.HARD_N - len(ext)]))
            break
        M *= 2
    have, fill = set(cols), []
    for c in range(M):
        if len(cols) + len(fill) == IR.HARD_N:
            break
        if c not in have:
            fill.append(c)
    clip = np.ascontiguousarray(pool[:, cols + fill])
    assert clip.shape == (IR.HARD_T, IR.HARD_N, 3) and clip.dtype == np.float32
    print(f"hard clip {G}^3: pool of {M} columns, {len(hard_cols)} columns with an upcast-sensitive row")
    return clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation (holds utils/, dataset/)")
    REF = os.path.abspath(ap.parse_args().reference)
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, REF)
    import utils.dataset_utils as DU
    import dataset.dataset as DS

    starts_log = []
    crop0 = DS.crop_sequence

    def crop_logged(seq, start, T, sample_rate=1):
        starts_log.append(int(start))
        return crop0(seq, start=start, T=T, sample_rate=sample_rate)
    DS.crop_sequence = crop_logged

    g = IR.G18
    arrays = dict(meta=np.array([g["seed"], g["G"], g["T"], g["N"], g["J"], g["dataset_seed"]], dtype=np.int64),
                  numpy_version=np.array([int(x) for x in np.__version__.split(".")[:3]], dtype=np.int64))
    home = os.getcwd()
    # ---- (a) ----
    seqs = IR.g18_sequences()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            _write_tree(seqs, g["names"])
            for tag, cls in (("aist", DS.AIST), ("dfaust", DS.DFAUST)):
                for rate in g["rates"]:
                    for e in g["epochs"]:
                        _items(DS, cls, list(g["names"]), starts_log, arrays, f"a_{tag}_r{rate}_e{e}", epoch=e, sample_rate=rate)
                    _items(DS, cls, list(g["names"]), starts_log, arrays, f"a_{tag}_r{rate}_rand", sample_rate=rate, random_crop=1)
        finally:
            os.chdir(home)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            _write_tree(IR.g18_sequences(short=True), g["short_names"])
            _items(DS, DS.DFAUST, list(g["short_names"]), starts_log, arrays, "a_short_r1_rand", sample_rate=1, random_crop=1)
            # the cases ClipSampler turns into ValueError, observed on the reference itself
            ds = DS.DFAUST(True, _options(sample_rate=1))
            ds.log_epoch(0)
            try:
                ds[ds.seq_path.index("s0/short_a.npy")]
                raise SystemExit("expected the reference to fail on a short file without random_crop")
            except ZeroDivisionError:
                print("reference: ZeroDivisionError for frames < T * sample_rate without random_crop")
            np.save("data/D-FAUST/surface/train/s0/short_a.npy", IR.sequence(g["seed"], 150, 5, g["N"], np.float32))
            ds = DS.DFAUST(True, _options(sample_rate=2, random_crop=1))
            got = ds[ds.seq_path.index("s0/short_a.npy")].shape[0]
            print(f"reference: a clip of {got} frames for frames = 5, T = 6, sample_rate = 2")
            assert got == 3
            ds = DS.AIST(True, _options(is_eval=1, random_crop=1))
            v, j = ds[ds.seq_path.index("short_a.npy")]
            print(f"reference: padded clip of {v.shape[0]} frames with joints of {j.shape[0]} frames")
            assert v.shape[0] == g["T"] and j.shape[0] == 4
        finally:
            os.chdir(home)
    # ---- (b) ----
    for name, (dtype, T, N, G, scale, xt, zt) in IR.G18_CLIPS.items():
        x = IR.g18_clip(name)
        norm = DU.episodic_normalization(x, scale, xt, zt)
        mine, _ = IR.episodic_normalization(x, scale, xt, zt)
        assert norm.dtype == np.float64 and np.array_equal(norm.view(np.uint64), mine.view(np.uint64)), f"{name}: the restatement's coordinates differ"
        vox_r, idx, bad = IR.voxelize(mine, G)
        try:
            vox = np.stack([DU.voxelize(norm[t], (G, G, G)) for t in range(T)])
            raised = 0
            assert np.array_equal(vox, vox_r), f"{name}: the restatement's voxels differ"
            arrays[f"b_{name}__vox"] = IR.pack(vox)
        except IndexError:
            raised = 1
        assert raised == int(bad.any()), name
        print(f"(b) {name}: {int((idx < 0).any(-1).sum())} rows with a negative index, {int(bad.sum())} bad rows, raised = {raised}")
        arrays[f"b_{name}__norm"] = norm
        arrays[f"b_{name}__idx"] = idx
        arrays[f"b_{name}__bad"] = np.int64(bad.sum())
        arrays[f"b_{name}__raised"] = np.int64(raised)
    # ---- (c) ----
    for pd in ("float32", "float64"):
        for jd in ("float32", "float64"):
            x, j = IR.g18_joint_case(pd, jd)
            _, jn = DU.episodic_normalization(x, 0.9, joints=j)
            mine = IR.episodic_normalization(x, 0.9, joints=j)[2]
            assert jn.dtype == mine.dtype and np.array_equal(jn, mine), f"(c) {pd}/{jd}: the restatement's joints differ"
            print(f"(c) points {pd}, joints {jd} -> {jn.dtype}")
            arrays[f"c_{pd}_{jd}__joints"] = jn
    # ---- (d) ----
    for G in IR.HARD_GRIDS:
        x = _hard_clip(G, DU)
        norm = DU.episodic_normalization(x, 0.9)
        mine, _ = IR.episodic_normalization(x, 0.9)
        assert np.array_equal(norm.view(np.uint64), mine.view(np.uint64))
        vox = np.stack([DU.voxelize(norm[t], (G, G, G)) for t in range(IR.HARD_T)])
        vox_r, idx, bad = IR.voxelize(mine, G)
        assert np.array_equal(vox, vox_r) and not bad.any()
        up, _ = IR.voxel_indices(IR.episodic_normalization(x, 0.9, upcast=True)[0], G)
        hard = int((up != idx).any(-1).sum())
        print(f"(d) hard clip {G}^3: {hard} rows differ under float64-upcast arithmetic")
        assert hard >= IR.HARD_MIN
        arrays[f"d_hard{G}__points"] = x
        arrays[f"d_hard{G}__norm"] = norm
        arrays[f"d_hard{G}__vox"] = IR.pack(vox)
        arrays[f"d_hard{G}__idx"] = idx
        arrays[f"d_hard{G}__hard"] = np.int64(hard)
    for path in golden_npz.save(os.path.join(OUT, "g18_input_path.npz"), **arrays):
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
