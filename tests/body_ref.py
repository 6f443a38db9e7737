"""float64 numpy restatement of the body-model contract of include/nm355.h (nm_body_shape, nm_body_pose, nm_body_joints), operation by
operation: explicit loops over every summation index, elementwise across vertices and frames, no dot / einsum / matmul on the pinned
path.  It is the library's own contract - SMPL-form linear blend skinning in float64 - and claims nobody else's bits.

A model is the dict BodyModel.numpy() returns: v_template (V,3), shapedirs (V,3,S), posedirs (P,3V), lbs_weights (V,J), parents (J),
reg_offsets (J+1), reg_cols, reg_vals.  `pose` takes ROTATIONS, so that the stage whose last bits belong to the math library
(`rodrigues`: sin, cos, sqrt) stays outside what is compared bit for bit.  The keyword switches of `pose` exist so that the tests can break
the restatement on purpose (tests/test_body_model_cpu.py: the mutations).
"""
import numpy as np


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def rodrigues(poses):
    """(T,J,3) axis-angle, float32 (widened exactly) or float64 -> (T,J,3,3) float64"""
    r = np.asarray(poses).astype(np.float64)
    e = r + 1e-8
    angle = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
    ux, uy, uz = r[..., 0] / angle, r[..., 1] / angle, r[..., 2] / angle
    s, c1 = np.sin(angle), 1.0 - np.cos(angle)
    zero = np.zeros_like(ux)
    K = [[zero, -uz, uy], [uz, zero, -ux], [-uy, ux, zero]]
    R = np.empty(r.shape[:-1] + (3, 3))
    for a in range(3):
        for b in range(3):
            kk = dot3(K[a][0], K[a][1], K[a][2], K[0][b], K[1][b], K[2][b])
            R[..., a, b] = ((1.0 if a == b else 0.0) + s * K[a][b]) + c1 * kk
    return R


def regress(m, x):
    """x (..., V, 3) -> (..., J, 3): the running sum over each CSR row, in row order"""
    off, cols, vals = m["reg_offsets"], m["reg_cols"], m["reg_vals"]
    J = off.shape[0] - 1
    out = np.zeros(x.shape[:-2] + (J, 3))
    for j in range(J):
        s = np.zeros(x.shape[:-2] + (3,))
        for k in range(int(off[j]), int(off[j + 1])):
            s = s + vals[k] * x[..., int(cols[k]), :]
        out[..., j, :] = s
    return out


def shape(m, betas=None):
    """-> v_shaped (V,3), J_rest (J,3)"""
    v = m["v_template"].copy()
    if betas is not None:
        b = np.asarray(betas).astype(np.float64)
        for s in range(m["shapedirs"].shape[2]):
            v = v + m["shapedirs"][:, :, s] * b[s]
    return v, regress(m, v)


def pose(m, rotations, v_shaped, J_rest, transl=None, scaling=1.0, reverse_blend=False, keep_rest=False, swap_parent=False,
         translate_first=False):
    """rotations (T,J,3,3) -> dict(vertices (T,V,3), posed_joints (T,J,3), joints (T,J,3), transforms (T,J,3,4))"""
    R = np.asarray(rotations, dtype=np.float64)
    T, J = R.shape[0], R.shape[1]
    V = v_shaped.shape[0]
    par = m["parents"]
    # chain
    Gr, Gt = np.empty((T, J, 3, 3)), np.empty((T, J, 3))
    Gr[:, 0] = R[:, 0]
    Gt[:, 0] = J_rest[0]
    for j in range(1, J):
        p = int(par[j])
        rel = J_rest[j] - J_rest[p]
        A, B = (R[:, j], Gr[:, p]) if swap_parent else (Gr[:, p], R[:, j])
        for a in range(3):
            for b in range(3):
                Gr[:, j, a, b] = dot3(A[:, a, 0], A[:, a, 1], A[:, a, 2], B[:, 0, b], B[:, 1, b], B[:, 2, b])
            Gt[:, j, a] = dot3(Gr[:, p, a, 0], Gr[:, p, a, 1], Gr[:, p, a, 2], rel[0], rel[1], rel[2]) + Gt[:, p, a]
    tr = np.empty((T, J, 3, 4))
    tr[..., :3] = Gr
    for j in range(J):
        for a in range(3):
            tr[:, j, a, 3] = Gt[:, j, a] if keep_rest else Gt[:, j, a] - dot3(Gr[:, j, a, 0], Gr[:, j, a, 1], Gr[:, j, a, 2], J_rest[j, 0], J_rest[j, 1], J_rest[j, 2])
    # vertices
    P = 9 * (J - 1)
    pd = m["posedirs"].reshape(P, V, 3)
    off = np.zeros((T, V, 3))
    eye = np.eye(3)
    for p in (range(P - 1, -1, -1) if reverse_blend else range(P)):
        j, a, b = 1 + p // 9, (p % 9) // 3, p % 3
        feat = R[:, j, a, b] - eye[a, b]
        off = off + feat[:, None, None] * pd[p][None]
    vp = v_shaped[None] + off
    M = np.zeros((T, V, 3, 4))
    w = m["lbs_weights"]
    for j in range(J):
        wj = w[:, j]
        M = np.where((wj != 0.0)[None, :, None, None], M + wj[None, :, None, None] * tr[:, j][:, None], M)
    x = np.empty((T, V, 3))
    for c in range(3):
        x[..., c] = dot3(M[..., c, 0], M[..., c, 1], M[..., c, 2], vp[..., 0], vp[..., 1], vp[..., 2]) + M[..., c, 3]

    def place(q):
        if translate_first:
            return scaling * (q + (0.0 if transl is None else np.asarray(transl, dtype=np.float64)[:, None, :]))
        q = scaling * q
        return q if transl is None else q + np.asarray(transl, dtype=np.float64)[:, None, :]

    vertices = place(x)
    return dict(vertices=vertices, posed_joints=place(Gt), joints=regress(m, vertices), transforms=tr)


def forward(m, rotations, betas=None, transl=None, scaling=1.0, **switches):
    v_shaped, J_rest = shape(m, betas)
    out = pose(m, rotations, v_shaped, J_rest, transl=transl, scaling=scaling, **switches)
    out.update(v_shaped=v_shaped, J_rest=J_rest)
    return out
