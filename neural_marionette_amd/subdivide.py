"""Loop-subdivision plans: the topology half of vis_retarget.py's ``temp_mesh.subdivide_loop(arg.subdivide_iter)`` and
``compute_vertex_normals()`` (:416-423, :497-512), built ONCE per mesh on the host in numpy - like the skeleton tree of skeleton.py and
the crops of ClipSampler it is one-shot work.  What runs per frame (NeuralMarionette.subdivide / vertex_normals / render_mesh with
vertex_normals) is HIP: csrc/nm_subdiv.hip applies these tables.

This is not open3d's numbering.  The contract is include/nm355.h's ("PLAN"), restated with plain dicts and loops in tests/subdiv_ref.py:
edge e of the (a, b)-sorted undirected edges creates vertex V + e; parent row m = (i, j, k) becomes rows 4m .. 4m+3 = (i,p,r) (p,j,q)
(r,q,k) (p,q,r); interior vertices take their ascending neighbours with Loop's beta_n, vertices with exactly two boundary edges the
(0.75, 0.125) rule over those two neighbours, every other vertex stays where it is."""
from __future__ import annotations

import math
from typing import List

import numpy as np
import torch


def loop_beta(n: int) -> float:
    """Loop's beta_n = (0.625 - (0.375 + 0.25 cos(2 pi / n))^2) / n in float64, math.cos"""
    return (0.625 - (0.375 + 0.25 * math.cos(2.0 * math.pi / n)) ** 2) / n


def _level_tables(tri: np.ndarray, V: int, level: int):
    """one level from triangles (M,3) int64 over V vertices: edge (E,4), ring_offsets (V+1), ring, w (V,2), and the child rows (4M,3)"""
    M = len(tri)
    where = f"level {level}: " if level else ""
    out_of_range = ((tri < 0) | (tri >= V)).any(1)
    if out_of_range.any():
        m = int(np.nonzero(out_of_range)[0][0])
        raise ValueError(f"LoopPlan.build: {where}triangle row {m} = {tri[m].tolist()} has an index outside [0, {V})")
    repeated = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0])
    if repeated.any():
        m = int(np.nonzero(repeated)[0][0])
        raise ValueError(f"LoopPlan.build: {where}triangle row {m} = {tri[m].tolist()} repeats an index")
    # the three directed edges of row m at 3m + s: (i,j) (j,k) (k,i), the opposite vertices k, i, j
    src, dst, opp = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1), tri[:, [2, 0, 1]].reshape(-1)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    key = lo * V + hi
    ukey, first, inverse, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)      # sorted by (a, b)
    E = len(ukey)
    if E and count.max() > 2:
        order = np.argsort(key, kind="stable")                         # equal keys keep their triangle-row order
        rank = np.arange(len(key)) - np.searchsorted(key[order], key[order], side="left")
        at = int(order[rank >= 2].min())
        raise ValueError(f"LoopPlan.build: {where}triangle row {at // 3} = {tri[at // 3].tolist()} is the third triangle of the undirected edge "
                         f"({int(lo[at])}, {int(hi[at])}); an edge may lie in two")
    edge = np.full((E, 4), -1, np.int64)
    edge[:, 0], edge[:, 1] = ukey // V, ukey % V
    edge[:, 2] = opp[first]                                            # np.unique's first occurrence: the lower triangle row
    last = np.full(E, -1, np.int64)
    last[inverse] = np.arange(len(key))                                # ascending assignment: the highest occurrence stays
    two = count == 2
    edge[two, 3] = opp[last[two]]
    ev = (V + inverse).reshape(M, 3)                                   # p = ev(i,j), q = ev(j,k), r = ev(k,i)
    i, j, k, p, q, r = tri[:, 0], tri[:, 1], tri[:, 2], ev[:, 0], ev[:, 1], ev[:, 2]
    children = np.stack([i, p, r, p, j, q, r, q, k, p, q, r], 1).reshape(4 * M, 3)
    # rings: both directions of every undirected edge, sorted by (vertex, neighbour)
    boundary = ~two
    v2, n2, b2 = np.concatenate([edge[:, 0], edge[:, 1]]), np.concatenate([edge[:, 1], edge[:, 0]]), np.concatenate([boundary, boundary])
    order = np.lexsort((n2, v2))
    v2, n2, b2 = v2[order], n2[order], b2[order]
    valence = np.bincount(v2, minlength=V)
    nbound = np.bincount(v2[b2], minlength=V)
    interior = (nbound == 0) & (valence >= 1)
    crease = nbound == 2
    keep = interior[v2] | (crease[v2] & b2)
    ring = n2[keep]
    ring_offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(v2[keep], minlength=V), out=ring_offsets[1:])
    w = np.empty((V, 2), np.float64)
    w[:] = (1.0, 0.0)
    w[crease] = (0.75, 0.125)
    for n in np.unique(valence[interior]):
        beta = loop_beta(int(n))
        w[interior & (valence == n)] = (1.0 - int(n) * beta, beta)
    return edge, ring_offsets, ring, w, children


def _face_tables(tri: np.ndarray, V: int):
    """face_offsets (V+1), faces (3M): each vertex's triangle rows, ascending"""
    corner = tri.reshape(-1)
    order = np.argsort(corner, kind="stable")                          # corners are listed row by row: equal vertices keep ascending rows
    face_offsets = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(corner, minlength=V), out=face_offsets[1:])
    return face_offsets, order // 3


class LoopPlan:
    """The index tables of ``levels`` Loop subdivisions of one mesh, on ``device`` (int32, the weights float64):
      levels_tables   a list of dicts, one per level: edge (E,4), ring_offsets (V+1), ring, w (V,2) - include/nm355.h, "PLAN"
      triangles       (M_L,3) of the finest level; face_offsets (V_L+1), faces (3 M_L): its vertex -> triangle index
      vertex_counts, triangle_counts   per level, ``levels`` + 1 entries each, the input mesh first
    ``levels`` = 0 holds the finest-level tables of the input mesh alone (what vertex_normals needs)."""

    def __init__(self, V, levels, levels_tables, triangles, face_offsets, faces, vertex_counts, triangle_counts, device):
        self.V, self.levels, self.levels_tables = V, levels, levels_tables
        self.triangles, self.face_offsets, self.faces = triangles, face_offsets, faces
        self.vertex_counts, self.triangle_counts, self.device = vertex_counts, triangle_counts, device

    @staticmethod
    def build(triangles, V: int, levels: int, device="cuda") -> "LoopPlan":
        """``triangles`` (M,3): a numpy array or a tensor of integers over ``V`` vertices.  A device tensor is copied to the host here,
        once - a synchronisation; nothing of the plan is built on the device.  Raises ValueError naming the offending triangle row for
        an index outside [0, V), a triangle with a repeated index, and an undirected edge that lies in more than two triangles."""
        V, levels = int(V), int(levels)
        if V < 1 or levels < 0:
            raise ValueError(f"LoopPlan.build: V must be >= 1 and levels >= 0, got V = {V}, levels = {levels}")
        tri = triangles.detach().cpu().numpy() if isinstance(triangles, torch.Tensor) else np.asarray(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
            raise ValueError(f"LoopPlan.build: triangles must be (M,3) integers, got {tuple(tri.shape)} {tri.dtype}")
        tri = tri.astype(np.int64)
        device = torch.device(device)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
        tables: List[dict] = []
        vertex_counts, triangle_counts = [V], [len(tri)]
        for level in range(levels):
            edge, ring_offsets, ring, w, tri = _level_tables(tri, vertex_counts[-1], level)
            if vertex_counts[-1] + len(edge) >= 2 ** 31 or 3 * len(tri) >= 2 ** 31:
                raise ValueError(f"LoopPlan.build: level {level + 1} would have {vertex_counts[-1] + len(edge)} vertices and {len(tri)} triangles; "
                                 "the tables are 32-bit")
            tables.append(dict(edge=i32(edge), ring_offsets=i32(ring_offsets), ring=i32(ring), w=torch.from_numpy(w).to(device)))
            vertex_counts.append(vertex_counts[-1] + len(edge))
            triangle_counts.append(len(tri))
        if not levels:
            _level_tables(tri, V, 0)                                    # the refusals hold for a plan without levels too
        face_offsets, faces = _face_tables(tri, vertex_counts[-1])
        fine = i32(tri)
        return LoopPlan(V, levels, tables, fine, i32(face_offsets), i32(faces), vertex_counts, triangle_counts, fine.device)      # ("cuda" -> "cuda:0")
