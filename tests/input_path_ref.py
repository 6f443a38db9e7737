"""numpy restatement of the reference's input path (utils/dataset_utils.py:6-31 as the dataset classes call it,
dataset/dataset.py:47-88 and :123-183) with every rounding written out, so that it does not depend on the promotion rules of the
numpy that runs it.  Fixture G18 (tools/make_input_fixture.py) holds what the reference itself returned under numpy 2.2.6; this file
is pinned to it by tests/test_input_path_cpu.py and is the reference of the GPU tests for the shapes the fixture does not hold.

Dtype rules (numpy 2: a Python float never widens an array):
  float32 points: bmin, bmax, blen float32; den = f32(blen + f32(1e-5)); (seq - bmin) * scale / den * 2 - 1 in float32, every step
                  rounded; float64 from `+ np.array([x_trans, 0, z_trans])` on; voxelize's (p - (-1)) / (2/G + 1e-5) in float64.
  float64 points: float64 throughout.
  joints:         ((j - bmin) * scale / den) * 2 - 1 in result_type(joints, points), bmin and den widened from the points' dtype.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from neural_marionette_amd import synth  # noqa: E402

# ---- the seeded inputs of fixture G18 ------------------------------------------------------------------------------------------------
G18 = dict(seed=1801, G=32, T=6, N=500, J=17, frames=(12, 23, 40), names=("seq_a.npy", "seq_b.npy", "seq_c.npy"), rates=(1, 2),
           epochs=(0, 1, 7), dataset_seed=3, short_frames=(4, 12), short_names=("short_a.npy", "short_b.npy"))
# (b): name -> (dtype, T, N, G, scale, x_trans, z_trans)
G18_CLIPS = {
    "f32_plain": ("float32", 6, 1000, 32, 1.0, 0.0, 0.0),
    "f64_plain": ("float64", 6, 1000, 32, 1.0, 0.0, 0.0),
    "f32_wrap": ("float32", 6, 1000, 32, 0.8, 0.1, -0.1),
    "f64_wrap": ("float64", 6, 1000, 32, 0.8, 0.1, -0.1),
    "f32_wrap40": ("float32", 3, 257, 40, 0.8, 0.1, -0.1),
    "f64_wrap40": ("float64", 3, 257, 40, 0.8, 0.1, -0.1),
    "f32_over": ("float32", 3, 257, 40, 1.0, 0.9, 0.0),          # rows with an index >= G: the reference raises
}
HARD_GRIDS = (32, 40, 64)
HARD_T, HARD_N, HARD_MIN = 3, 1000, 8


def sequence(seed, tag, frames, N, dtype, J=0):
    """A seeded figure sequence (frames, N, 3) and, with J > 0, joints (frames, J, 3) that move with it."""
    rng = np.random.default_rng(np.random.SeedSequence([seed, tag, 0x18]))
    pts = synth.figure_points(frames, N, rng)
    if not J:
        return pts.astype(dtype)
    pick = rng.integers(0, N, J)
    joints = pts[:, pick] + 0.01 * rng.standard_normal((frames, J, 3))
    return pts.astype(dtype), joints


def g18_sequences(short=False):
    """[(points float32, joints float32)] of the files the fixture's dataset objects read, in sorted file order."""
    frames = G18["short_frames"] if short else G18["frames"]
    out = []
    for i, f in enumerate(frames):
        p, j = sequence(G18["seed"], (100 if short else 0) + i, f, G18["N"], np.float32, J=G18["J"])
        out.append((p, j.astype(np.float32)))
    return out


def g18_clip(name):
    dtype, T, N, G, scale, xt, zt = G18_CLIPS[name]
    return sequence(G18["seed"], 1000 + sorted(G18_CLIPS).index(name), T, N, np.dtype(dtype))


def g18_joint_case(pd, jd):
    """(c): points (4,300,3) of dtype pd and joints (4,9,3) of dtype jd."""
    p, j = sequence(G18["seed"], 2000, 4, 300, np.dtype(pd), J=9)
    return p, j.astype(jd)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def crop_frames(frames, start, T, sample_rate, pad):
    """Frame numbers of a crop; with pad the frames past the end repeat the last one (dataset.py:65-68 appends copies of it)."""
    idx = start + np.arange(T) * sample_rate
    if pad:
        return np.minimum(idx, frames - 1)
    if idx[-1] >= frames or start < 0:
        raise ValueError(f"crop start {start} + {T - 1} x {sample_rate} does not fit {frames} frames")
    return idx


def episodic_normalization(seq, scale=1.0, x_trans=0.0, z_trans=0.0, joints=None, upcast=False):
    """utils/dataset_utils.py:9-19.  Returns float64 (T,N,3) [, joints]; also the box as (bmin, bmax).  upcast=True evaluates the
    float64 chain on widened data (what a float64-only implementation computes for float32 files)."""
    if upcast:
        seq = seq.astype(np.float64)
    ft = seq.dtype.type
    assert ft in (np.float32, np.float64)
    bmax = seq.max(axis=(0, 1))
    bmin = seq.min(axis=(0, 1))
    blen = ft((bmax - bmin).max())
    den = ft(blen + ft(1e-5))
    v = seq - bmin[None, None]
    v = v * ft(scale)
    v = v / den
    v = v * ft(2)
    v = v - ft(1)
    assert v.dtype.type is ft
    w = v.astype(np.float64) + np.array([x_trans, 0.0, z_trans], dtype=np.float64)
    out = [w, (bmin, bmax)]
    if joints is not None:
        rt = np.result_type(joints.dtype, seq.dtype).type
        j = joints.astype(rt) - bmin.astype(rt)[None, None]
        j = j * rt(scale)
        j = j / rt(den)
        j = j * rt(2)
        j = j - rt(1)
        assert j.dtype.type is rt
        out.append(j)
    return tuple(out)


def voxel_indices(w, G):
    """utils/dataset_utils.py:24-28 on float64 coordinates: int32 indices (truncation toward zero) and the mask of the rows the
    reference cannot scatter (an index outside [-G, G), or a coordinate that is not finite)."""
    step = 2.0 / float(G) + 1e-5
    q = (w - (-1.0)) / step
    fin = np.isfinite(q) & (np.abs(q) < 2147483648.0)
    idx = np.where(fin, q, 0.0).astype(np.int32)
    bad = ~(fin & (idx >= -G) & (idx < G)).all(-1)
    return idx, bad


def voxelize(w, G):
    """(T,N,3) float64 -> voxels (T,1,G,G,G) float32 with numpy's negative-index wrap, indices (T,N,3), bad-row mask (T,N)."""
    idx, bad = voxel_indices(w, G)
    T = w.shape[0]
    vox = np.zeros((T, 1, G, G, G), dtype=np.float32)
    for t in range(T):
        i = idx[t][~bad[t]]
        vox[t, 0][i[:, 0], i[:, 1], i[:, 2]] = 1.0
    return vox, idx, bad


def clip(points, start, T, sample_rate, pad, G, scale=1.0, x_trans=0.0, z_trans=0.0, joints=None, upcast=False):
    """The whole path for one crop: dict(vox, idx, bad, bbox (6,) float64 [, joints])."""
    fr = crop_frames(points.shape[0], start, T, sample_rate, pad)
    res = episodic_normalization(points[fr], scale, x_trans, z_trans, joints=None if joints is None else joints[fr], upcast=upcast)
    vox, idx, bad = voxelize(res[0], G)
    out = dict(vox=vox, idx=idx, bad=bad, norm=res[0], bbox=np.concatenate([res[1][0], res[1][1]]).astype(np.float64))
    if joints is not None:
        out["joints"] = res[2]
    return out


def pack(vox):
    return np.packbits(vox.reshape(-1) != 0)


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(np.float32)


# ---- the start-index rules of dataset.py:51-68, restated for the ValueError cases --------------------------------------------------
def reference_start(frames, T, sample_rate, random_crop, epoch_id, randint):
    """What the reference's __getitem__ computes (its exceptions included); returns (start, frames after padding)."""
    if random_crop:
        rand_start = frames - 1 - sample_rate * (T - 1)
        start = 0 if rand_start < 0 else randint(0, rand_start)
    else:
        offset = (epoch_id % T) * sample_rate
        start = epoch_id % (frames // (T * sample_rate)) * (T * sample_rate) + offset
        if start + (T - 1) * sample_rate >= frames:
            start = max(start - 2 * offset, 0)
    padded = frames
    if frames < T * sample_rate:
        start = 0
        padded = frames + max(T - frames, 0)
    return start, padded
