"""Device input path for training and evaluation batches.

The reference's dataset classes (dataset/dataset.py) load a sequence, pick a crop, normalise it and voxelise it on the host for every
item.  Here the sequences stay on the device (ClipBank), the host only picks the crops (ClipSampler: the start-index rules of
dataset.py:51-68, on the reference's own random stream) and one library call builds the (B,T,1,G,G,G) batch
(NeuralMarionette.voxelize_batch -> nm_voxelize_batch).  DeviceClipLoader ties the three together for the trainers.
File I/O is the caller's: ``bank.add(np.load(path)[..., :3])`` for a prepared point sequence, or ``bank.add_mesh(net, vertices,
triangles)`` for a mesh sequence, which is sampled on the device (NeuralMarionette.sample_surface -> nm_sample_surface), or
``bank.add_body(net, model, poses)`` for an SMPL-form pose stream, which is posed on the device first (NeuralMarionette.pose_bodies).
"""
from __future__ import annotations

import ctypes as C
import random
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib


class ClipBank:
    """Sequences (frames, N, 3) kept on the device in their own dtype (float32 stays float32: the reference's arithmetic depends on
    it), each optionally with joints (frames, J, 3)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.points: List[torch.Tensor] = []
        self.joints: List[Optional[torch.Tensor]] = []

    @staticmethod
    def _as_tensor(a, what):
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach()
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what} must be float32 or float64, got {t.dtype}")
        if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{what} must be (frames, n, 3) with frames, n >= 1, got {tuple(t.shape)}")
        return t

    def add(self, points, joints=None) -> int:
        p = self._as_tensor(points, "points")
        j = None
        if joints is not None:
            j = self._as_tensor(joints, "joints")
            if j.shape[0] != p.shape[0]:
                raise ValueError(f"joints have {j.shape[0]} frames, points {p.shape[0]}")
            j = j.to(self.device).contiguous()
        self.points.append(p.to(self.device).contiguous())
        self.joints.append(j)
        return len(self.points) - 1

    def add_mesh(self, net, vertices, triangles, count: int = 20000, seed: int = 0, joints=None) -> int:
        """Samples ``count`` surface points per frame of the mesh sequence ``vertices`` (frames,V,3) / ``triangles`` (F,3) on the
        device (NeuralMarionette.sample_surface) and stores the float32 points - what the reference's prepared ``.npy[..., :3]``
        holds - as a new sequence; returns its id."""
        return self.add(net.sample_surface(vertices, triangles, count=count, seed=seed)["points"], joints)

    def add_body(self, net, model, poses, betas=None, transl=None, scaling: float = 1.0, count: int = 20000, seed: int = 0) -> int:
        """The reference's AIST++ preparation for one motion sequence (dataset/aistpp/prepare_aistpp.py:54-62, :75-89) on the device:
        ``model`` (body.BodyModel) posed by ``poses`` (frames,J,3) axis-angle with ``betas`` / ``transl`` / ``scaling``
        (NeuralMarionette.pose_bodies), ``count`` surface points per frame of the posed meshes over ``model.faces`` (add_mesh), and the
        regressed joints stored with the sequence as float32 - what ``voxelize_batch(..., return_joints=True)`` and
        ``eval_utils.semantic_scores`` read for prepared data.  Returns the sequence's id.
        The whole sequence is posed in one call, there is NO frame grouping: the transient is the float64 vertices, 24 V bytes per frame -
        about 480 MB for a 2 900-frame sequence at SMPL's 6 890 vertices.  (Posing in groups would be harmless, but the sampler counts
        its uniforms by the frame's index within a call, so sampling in groups would change the points.)"""
        out = net.pose_bodies(model, poses=poses, betas=betas, transl=transl, scaling=scaling, return_joints=True)
        return self.add_mesh(net, out["vertices"], model.faces, count=count, seed=seed, joints=out["joints"].to(torch.float32))

    def __len__(self) -> int:
        return len(self.points)

    @property
    def lengths(self) -> List[int]:
        return [int(p.shape[0]) for p in self.points]

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.points + [j for j in self.joints if j is not None])


class ClipSampler:
    """Which crop of which sequence is item ``index`` - dataset/dataset.py:34-35 (seeded shuffle of the sequence list) and :51-68
    (start index, last-frame padding).  ``rng`` stands for the reference's module-level ``random``: ``random.Random(options.seed)``
    reproduces its ``random.seed / shuffle / randint`` stream, the shuffle is drawn here in the constructor and one ``randint`` per
    random crop in ``crop``, in call order.

    lengths[i]: frames of sequence i (the reference's sorted file list).  ``order``: the shuffled list, item -> sequence.
    ``crop(index) -> (sequence, start, pad)``; pad: the crop runs past the sequence's end and repeats its last frame.
    Where the reference fails or returns a clip that does not have T frames, ``crop`` raises ValueError naming the sequence:
    frames < T * sample_rate without random_crop (its ZeroDivisionError), a padded crop of fewer than T frames (e.g. frames = 5, T = 6,
    sample_rate = 2 gives 3), and a padded clip of a sequence with joints (the reference pads the points only).
    """

    def __init__(self, lengths: Sequence[int], T: int, sample_rate: int, random_crop: bool, rng: random.Random,
                 has_joints=False, names: Optional[Sequence[str]] = None):
        self.lengths = [int(f) for f in lengths]
        self.T, self.sample_rate, self.random_crop, self.rng = int(T), int(sample_rate), bool(random_crop), rng
        if self.T < 1 or self.sample_rate < 1 or any(f < 1 for f in self.lengths):
            raise ValueError(f"ClipSampler: T = {T}, sample_rate = {sample_rate}, lengths = {list(lengths)}")
        n = len(self.lengths)
        self.has_joints = [bool(has_joints)] * n if isinstance(has_joints, (bool, int)) else [bool(h) for h in has_joints]
        self.names = [f"sequence {i}" for i in range(n)] if names is None else [str(s) for s in names]
        self.order = list(range(n))
        rng.shuffle(self.order)
        self.epoch_id: Optional[int] = None

    def log_epoch(self, epoch_id: int) -> None:
        self.epoch_id = int(epoch_id)

    def __len__(self) -> int:
        return len(self.order)

    def crop(self, index: int):
        seq = self.order[index]
        frames, T, rate, name = self.lengths[seq], self.T, self.sample_rate, self.names[seq]
        if self.random_crop:
            rand_start = frames - 1 - rate * (T - 1)
            start = 0 if rand_start < 0 else self.rng.randint(0, rand_start)
        else:
            if self.epoch_id is None:
                raise ValueError("ClipSampler: log_epoch() has not been called (the epoch selects the crop without random_crop)")
            if frames < T * rate:
                raise ValueError(f"{name}: {frames} frames < T * sample_rate = {T * rate} without random_crop (the reference divides by zero)")
            offset = (self.epoch_id % T) * rate
            start = self.epoch_id % (frames // (T * rate)) * (T * rate) + offset
            if start + (T - 1) * rate >= frames:
                start = max(start - 2 * offset, 0)
        pad = False
        if frames < T * rate:
            start, pad = 0, True
            padded = frames + max(T - frames, 0)
            got = len(range(0, min(padded, T * rate), rate))
            if got != T:
                raise ValueError(f"{name}: {frames} frames padded to {padded} give a clip of {got} frames, not T = {T} (sample_rate {rate})")
            if self.has_joints[seq] and frames < T:
                raise ValueError(f"{name}: the clip is padded from {frames} to {T} frames but its joints are not (the reference pads the points only)")
        return seq, start, pad


class _DescStaging:
    """Pinned host staging of the descriptor table: a ring of buffers, each guarded by the event of its last copy - a buffer is
    rewritten only after the asynchronous copy that read it has completed (the ring grows while every buffer is still in flight)."""
    MAX_SLOTS = 8

    def __init__(self):
        self.slots = []          # [pinned uint8 tensor, event]
        self.next = 0

    def upload(self, table, nbytes: int, device) -> torch.Tensor:
        slot = None
        for k in range(len(self.slots)):
            cand = self.slots[(self.next + k) % len(self.slots)]
            if cand[0].numel() >= nbytes and cand[1].query():
                slot = cand
                self.next = (self.next + k + 1) % len(self.slots)
                break
        if slot is None and len(self.slots) < self.MAX_SLOTS:
            slot = [torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
            self.slots.append(slot)
        if slot is None:                                    # every buffer in flight (or too small): wait for the oldest one
            slot = self.slots[self.next]
            self.next = (self.next + 1) % len(self.slots)
            slot[1].synchronize()
            if slot[0].numel() < nbytes:
                slot[0] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        C.memmove(slot[0].data_ptr(), table, nbytes)
        dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        dev.copy_(slot[0][:nbytes], non_blocking=True)
        slot[1].record(torch.cuda.current_stream(device))
        return dev


def _per_clip(v, B: int, what: str) -> List[float]:
    if isinstance(v, (int, float)):
        return [float(v)] * B
    v = [float(x) for x in v]
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} values for {B} clips")
    return v


def voxelize_batch(net, bank: ClipBank, ids, starts, T: int, sample_rate: int = 1, scale=1.0, x_trans=0.0, z_trans=0.0,
                   return_joints: bool = False, return_indices: bool = False, check: bool = False, pad=None):
    """See NeuralMarionette.voxelize_batch."""
    eng = net._engine
    ctx = eng.ready()
    dev = ctx.device
    ids, starts = [int(i) for i in ids], [int(s) for s in starts]
    B, T, rate = len(ids), int(T), int(sample_rate)
    pads = [False] * B if pad is None else [bool(p) for p in pad]
    if B < 1 or len(starts) != B or len(pads) != B:
        raise ValueError(f"voxelize_batch: {B} ids, {len(starts)} starts, {len(pads)} pad flags")
    if T < 1 or rate < 1:
        raise ValueError(f"voxelize_batch: T = {T}, sample_rate = {rate}")
    sc, xt, zt = _per_clip(scale, B, "scale"), _per_clip(x_trans, B, "x_trans"), _per_clip(z_trans, B, "z_trans")
    for i in ids:
        if not 0 <= i < len(bank):
            raise ValueError(f"voxelize_batch: no sequence {i} in the bank ({len(bank)} sequences)")
    first = bank.points[ids[0]]
    if first.device != dev:
        raise ValueError(f"voxelize_batch: the bank is on {first.device}, the network on {dev}")
    N, pdt = int(first.shape[1]), first.dtype
    J, jdt = 0, torch.float32
    if return_joints:
        j0 = bank.joints[ids[0]]
        if j0 is None:
            raise ValueError(f"voxelize_batch: sequence {ids[0]} has no joints")
        J, jdt = int(j0.shape[1]), j0.dtype
    table = (_lib.NmClipDesc * B)()
    for b, (i, s, p) in enumerate(zip(ids, starts, pads)):
        pts, jts = bank.points[i], bank.joints[i]
        frames = int(pts.shape[0])
        if int(pts.shape[1]) != N or pts.dtype != pdt:
            raise ValueError(f"voxelize_batch: sequence {i} is {tuple(pts.shape)} {pts.dtype}, sequence {ids[0]} has {N} points of {pdt}: one batch, one shape")
        if s < 0 or (not p and s + (T - 1) * rate >= frames):
            raise ValueError(f"voxelize_batch: sequence {i}: start {s} + {T - 1} x {rate} does not fit its {frames} frames")
        if return_joints and (jts is None or int(jts.shape[1]) != J or jts.dtype != jdt):
            raise ValueError(f"voxelize_batch: sequence {i} has no joints of shape (frames,{J},3) {jdt}")
        d = table[b]
        d.points, d.joints = pts.data_ptr(), (jts.data_ptr() if return_joints else None)
        d.frames, d.start, d.sample_rate, d.pad = frames, s, rate, int(p)
        d.scale, d.x_trans, d.z_trans = sc[b], xt[b], zt[b]
    staging = getattr(eng, "_clip_staging", None)
    if staging is None:
        staging = eng._clip_staging = _DescStaging()
    table_dev = staging.upload(table, C.sizeof(table), dev)
    G = eng.opts.grid_size
    vox = torch.empty(B, T, 1, G, G, G, device=dev)
    out_dt = torch.float32 if (pdt == torch.float32 and jdt == torch.float32) else torch.float64
    joints = torch.empty(B, T, J, 3, device=dev, dtype=out_dt) if return_joints else None
    idx = torch.empty(B, T, N, 3, device=dev, dtype=torch.int32) if return_indices else None
    bbox = torch.empty(B, 6, device=dev, dtype=torch.float64)
    bad = torch.empty(B, device=dev, dtype=torch.int32)
    eng.call("nm_voxelize_batch", table_dev.data_ptr(), B, T, N, J, int(pdt == torch.float64), int(jdt == torch.float64),
             _lib.ptr(vox), _lib.ptr(joints), _lib.ptr(idx), _lib.ptr(bbox), _lib.ptr(bad))
    if check and int(bad.sum()) != 0:                       # (the one synchronisation)
        raise ValueError("Dataset voxelizer error")
    return dict(vox=vox, joints=joints, indices=idx, bbox=bbox, bad_rows=bad)


class DeviceClipLoader:
    """Iterable of device batches: ``for vox in loader: trainer.step(vox)``.  Item i of the sampler's shuffled list goes to batch
    i // batch (the last batch may be smaller); a bank with joints yields ``(vox, joints)`` like the reference's evaluation datasets.
    Every iteration draws the sampler's crops anew (call ``sampler.log_epoch`` first where the epoch selects them)."""

    def __init__(self, net, bank: ClipBank, sampler: ClipSampler, batch: int, scale: float = 1.0, with_joints: Optional[bool] = None,
                 check: bool = False):
        if batch < 1:
            raise ValueError(f"DeviceClipLoader: batch = {batch}")
        if len(sampler.lengths) != len(bank) or sampler.lengths != bank.lengths:
            raise ValueError("DeviceClipLoader: the sampler's lengths are not the bank's")
        self.net, self.bank, self.sampler, self.batch, self.scale, self.check = net, bank, sampler, int(batch), float(scale), bool(check)
        self.with_joints = all(j is not None for j in bank.joints) and len(bank) > 0 if with_joints is None else bool(with_joints)

    def __len__(self) -> int:
        return (len(self.sampler) + self.batch - 1) // self.batch

    def __iter__(self):
        s = self.sampler
        for lo in range(0, len(s), self.batch):
            crops = [s.crop(i) for i in range(lo, min(lo + self.batch, len(s)))]
            out = voxelize_batch(self.net, self.bank, [c[0] for c in crops], [c[1] for c in crops], s.T, s.sample_rate, scale=self.scale,
                                 return_joints=self.with_joints, check=self.check, pad=[c[2] for c in crops])
            yield (out["vox"], out["joints"]) if self.with_joints else out["vox"]
