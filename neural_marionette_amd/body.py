"""Body models for the device input path: SMPL-form linear blend skinning with shape and pose blend shapes.

The reference's AIST++ preparation (dataset/aistpp/prepare_aistpp.py:54-62, :86-89) builds an SMPL model with smplx, evaluates it for every
frame of a motion sequence and multiplies the joint regressor into the posed vertices.  Here the model is plain arrays kept on the device
(BodyModel); NeuralMarionette.pose_bodies evaluates it (nm_body_shape / nm_body_pose / nm_body_joints, csrc/nm_body.hip) and
ClipBank.add_body feeds the posed meshes to the surface sampler.  The arithmetic is the contract of include/nm355.h - float64, not smplx's
float32 - and tests/body_ref.py restates it.  Reading the official ``.pkl`` (pickle, chumpy) stays the caller's: ``BodyModel.from_npz``
takes the arrays under the file's own names.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

MAX_JOINTS = 64


def _bad_row(a: np.ndarray) -> int:
    """first row (index along axis 0) of ``a`` with a non-finite entry, -1 if there is none"""
    if a.size == 0:
        return -1
    bad = ~np.isfinite(a.reshape(a.shape[0], -1)).all(axis=1)
    return int(np.argmax(bad)) if bad.any() else -1


def _f64(a, name: str, shape, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype.kind not in "fiu" or a.ndim != len(shape) or any(s is not None and int(d) != s for d, s in zip(a.shape, shape)):
        want = "(" + ",".join("?" if s is None else str(s) for s in shape) + ")"
        raise ValueError(f"BodyModel: {name} must be {what} {want}, got {tuple(a.shape)} {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.float64)                  # (float16 / float32 / integers widen exactly)
    r = _bad_row(a)
    if r >= 0:
        raise ValueError(f"BodyModel: {name} has a non-finite entry in row {r}")
    return a


class BodyModel:
    """An SMPL-form body model on ``device``: V vertices, J <= 64 joints, S shape coefficients, P = 9 (J - 1) pose features.

    v_template (V,3); shapedirs (V,3,S), S may be 0; posedirs in the model file's layout (V,3,P), stored as (P,3V) - row
    p = 9 (j - 1) + 3 a + b, column 3 v + c - and empty for J = 1; J_regressor (J,V), dense or scipy sparse, stored as CSR (reg_offsets,
    reg_cols, reg_vals) with the columns of every row ascending and explicit zeros dropped; parents (J) with parents[0] = -1 and
    0 <= parents[j] < j, kept on the host too; lbs_weights (V,J); faces (F,3) int32.  Everything floating is widened exactly to float64.
    Raises ValueError, naming the row, for wrong shapes, non-finite entries, a parent table that is not topological, face indices outside
    [0, V) and J > 64."""

    SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
    MAX_JOINTS = MAX_JOINTS

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, faces, device="cpu"):
        self.device = torch.device(device)
        vt = _f64(v_template, "v_template", (None, 3), "a float array")
        V = int(vt.shape[0])
        if V < 1:
            raise ValueError("BodyModel: v_template has no vertices")
        par = np.asarray(parents)
        if par.ndim != 1 or par.dtype.kind not in "iu" or par.shape[0] < 1:
            raise ValueError(f"BodyModel: parents must be a (J) integer array with J >= 1, got {tuple(par.shape)} {par.dtype}")
        J = int(par.shape[0])
        if J > MAX_JOINTS:
            raise ValueError(f"BodyModel: {J} joints, at most {MAX_JOINTS}")
        par = par.astype(np.int64)
        for j in range(J):
            if (par[j] != -1) if j == 0 else not 0 <= par[j] < j:
                raise ValueError(f"BodyModel: parents[{j}] = {int(par[j])}: the root's is -1, every other joint's lies in [0, {j})")
        P = 9 * (J - 1)
        sd = _f64(shapedirs, "shapedirs", (V, 3, None), "a float array")
        pd = _f64(posedirs, "posedirs", (V, 3, P), "a float array in the file layout")
        w = _f64(lbs_weights, "lbs_weights", (V, J), "a float array")
        reg = J_regressor.toarray() if hasattr(J_regressor, "toarray") else J_regressor
        reg = _f64(reg, "J_regressor", (J, V), "a dense or scipy sparse array")
        f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu" or f.shape[0] < 1:
            raise ValueError(f"BodyModel: faces must be an (F,3) integer array with F >= 1, got {tuple(f.shape)} {f.dtype}")
        f = f.astype(np.int64)
        out = (f < 0) | (f >= V)
        if out.any():
            r = int(np.argmax(out.any(axis=1)))
            raise ValueError(f"BodyModel: faces row {r} = {f[r].tolist()} has an index outside [0, {V})")
        self.V, self.J, self.S, self.P = V, J, int(sd.shape[2]), P
        self.parents = par.astype(np.int32)                          # host
        rows, cols = np.nonzero(reg)                                 # row-major: rows ascending, columns ascending within a row
        offsets = np.zeros(J + 1, dtype=np.int32)
        np.cumsum(np.bincount(rows, minlength=J), out=offsets[1:])
        dev = self.device
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.v_template, self.shapedirs, self.lbs_weights = t(vt), t(sd), t(w)
        self.posedirs = t(pd.reshape(3 * V, P).T)                    # (P, 3V)
        self.reg_offsets, self.reg_cols, self.reg_vals = t(offsets), t(cols.astype(np.int32)), t(reg[rows, cols])
        self.faces = t(f.astype(np.int32))
        self._shape_cache = {}                                       # NeuralMarionette.pose_bodies: v_shaped, J_rest per betas tensor

    @classmethod
    def from_npz(cls, path_or_mapping, device="cpu", num_betas: int = 10) -> "BodyModel":
        """From an ``.npz`` (or any mapping) with the model file's own keys: v_template, shapedirs, posedirs, J_regressor, weights,
        kintree_table (2,J), f.  parents = kintree_table[0] with entry 0 forced to -1, whatever unsigned wrap-around it carries;
        shapedirs is cut to its first ``num_betas`` columns."""
        m = np.load(path_or_mapping, allow_pickle=False) if isinstance(path_or_mapping, (str, bytes)) or hasattr(path_or_mapping, "__fspath__") else path_or_mapping
        for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kintree_table", "f"):
            if k not in m:
                raise ValueError(f"BodyModel.from_npz: no key '{k}'")
        kt = np.asarray(m["kintree_table"])
        if kt.ndim != 2 or kt.shape[0] != 2 or kt.shape[1] < 1 or kt.dtype.kind not in "iu":
            raise ValueError(f"BodyModel.from_npz: kintree_table must be a (2,J) integer array, got {tuple(kt.shape)} {kt.dtype}")
        parents = [-1] + [int(p) for p in kt[0, 1:]]
        if max(parents) >= 2 ** 31:
            raise ValueError("BodyModel.from_npz: kintree_table[0] has an entry past 2^31 other than the root's")
        sd = np.asarray(m["shapedirs"])
        if sd.ndim == 3:
            sd = sd[:, :, :int(num_betas)]
        return cls(m["v_template"], sd, m["posedirs"], m["J_regressor"], np.asarray(parents, dtype=np.int64), m["weights"], m["f"], device=device)

    @classmethod
    def synthetic(cls, V: int, J: int, S: int, seed: int, parents=None, device="cpu") -> "BodyModel":
        """A seeded stand-in for tests and timing, NOT a body: a blob of vertices around a random joint tree, smooth weights with at most
        four non-zeros per vertex that sum to 1, small random blend shapes, a sparse regressor whose rows sum to 1, and a closed triangle
        fan around vertex 0 so that the surface sampler has area."""
        rng = np.random.default_rng(seed)
        par = np.asarray([-1] + [int(rng.integers(0, j)) for j in range(1, J)] if parents is None else parents, dtype=np.int64)
        if par.shape != (J,):
            raise ValueError(f"BodyModel.synthetic: parents must have {J} entries, got {tuple(par.shape)}")
        joints = np.zeros((J, 3))
        for j in range(1, J):
            d = rng.standard_normal(3)
            joints[j] = joints[par[j]] + 0.25 * d / np.linalg.norm(d)
        home = np.arange(V) % J
        vt = joints[home] + 0.08 * rng.standard_normal((V, 3))
        d2 = ((vt[:, None, :] - joints[None, :, :]) ** 2).sum(axis=2)
        w = np.exp(-d2 / 0.02)
        keep = np.argsort(-w, axis=1)[:, :min(4, J)]
        mask = np.zeros_like(w, dtype=bool)
        np.put_along_axis(mask, keep, True, axis=1)
        w = np.where(mask, w + 1e-3, 0.0)
        w = w / w.sum(axis=1, keepdims=True)
        sd = 0.01 * rng.standard_normal((V, 3, S))
        pd = 0.01 * rng.standard_normal((V, 3, 9 * (J - 1)))
        reg = np.zeros((J, V))
        n = min(8, V)
        for j in range(J):
            near = np.argsort(d2[:, j])[:n]
            r = rng.random(n) + 0.1
            reg[j, near] = r / r.sum()
        if V >= 3:
            i = np.arange(1, V)
            faces = np.stack([np.zeros(V - 1, dtype=np.int64), i, np.where(i + 1 < V, i + 1, 1)], axis=1)
        else:
            faces = np.asarray([[0, V - 1, V - 1]])
        return cls(vt, sd, pd, reg, par, w, faces, device=device)

    def affinity(self) -> np.ndarray:
        """The (J,J) float32 symmetric 0/1 matrix of prepare_aistpp.py:65-73 (``gt_affinity.npy``): joint and parent are connected."""
        a = np.zeros((self.J, self.J), dtype=np.float32)
        for k in range(self.J):
            p = int(self.parents[k])
            if p < 0:
                continue
            a[k, p] = 1.0
        return np.maximum(a, a.T)

    def numpy(self) -> dict:
        """Host copies of the stored arrays under their stored names and layouts (posedirs (P,3V), the regressor as CSR)."""
        g = lambda t: t.detach().cpu().numpy()
        return dict(v_template=g(self.v_template), shapedirs=g(self.shapedirs), posedirs=g(self.posedirs), lbs_weights=g(self.lbs_weights),
                    reg_offsets=g(self.reg_offsets), reg_cols=g(self.reg_cols), reg_vals=g(self.reg_vals), parents=self.parents.copy(),
                    faces=g(self.faces))
