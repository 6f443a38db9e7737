"""float64 restatement of the reference's motion retargeting (vis_retarget.py:21-62 and :236-322), vectorised in numpy, in the
project's own words: what nm_retarget_bind / nm_retarget_fk / nm_retarget_pose (neural_marionette_amd/csrc/nm_retarget.hip) are held to.

bind() repeats the reference's extract_skin_weights in its operation order (fp32 where the reference's tensors are fp32, float64 where
its numpy points make them float64); fixture G16 pins it to the reference's own function bit for bit
(tests/test_retarget_cpu.py).  pose_dense() is the reference's form of the blend - a dense (N,K) weight matrix against the K
transformed copies of every point; pose() is the two-term form on the bind record.

One choice is the project's own: the ancestor walk that looks for a joint's nearest valid ancestor stops at the root even when the
root is invalid (the reference's loop does not terminate there); the library makes the same choice.

standin() builds the seeded inputs of the op-level GPU tests."""
import numpy as np

from neural_marionette_amd import synth


def bone_points(parents, kp, threshold=0.2):
    """(K,3) fp32: the joint itself for the root, else the midpoint of the joint and its nearest ancestor that is not invalid (the walk
    stops at the root); and the invalid mask, intensity < threshold compared in fp32"""
    kp = np.asarray(kp, np.float32)
    K = kp.shape[0]
    invalid = kp[:, 3] < np.float32(threshold)
    bones = np.zeros((K, 3), np.float32)
    for k in range(K):
        a = int(parents[k])
        if a == k:
            bones[k] = kp[k, :3]
            continue
        for _ in range(K):
            if not invalid[a] or int(parents[a]) == a:
                break
            a = int(parents[a])
        bones[k] = (kp[k, :3] + kp[a, :3]) / np.float32(2)
    return bones, invalid


def _norm(d):
    d = d * d
    return np.sqrt((d[..., 0] + d[..., 1]) + d[..., 2])


def bind(parents, root, points, kp, R_bind=None, hardness=8.0, threshold=0.2, force_child=None):
    """points (N,3) float64, kp (K,4) fp32, R_bind (K,3,3) fp32 or None -> dict child, parent, w (N,2) fp32 [child, parent], local
    (N,2,3) float64, margin (N) float64, dense (N,K) fp32 [the reference's matrix]"""
    points = np.asarray(points, np.float64)
    kp = np.asarray(kp, np.float32)
    parents = np.asarray(parents, np.int64)
    N, K = points.shape[0], kp.shape[0]
    bones, invalid = bone_points(parents, kp, threshold)
    dist = _norm(points[:, None] - bones[None].astype(np.float64))
    dist[:, invalid] = 1e4
    dist[:, root] = 1e4
    nearest = dist.argmin(-1)
    srt = np.sort(dist, -1)
    margin = srt[:, 1] - srt[:, 0]
    child = nearest if force_child is None else np.asarray(force_child, np.int64)
    parent = parents[child]
    pos = kp[:, :3].astype(np.float64)
    c = np.exp(_norm(points - pos[child]) * hardness)
    q = np.exp(_norm(points - pos[parent]) * hardness)
    w = np.stack([(q / (c + q)).astype(np.float32), (c / (c + q)).astype(np.float32)], -1)
    n = np.arange(N)
    dense = np.zeros((N, K), np.float32)
    dense[n, parent] = w[:, 1]
    dense[n, child] = w[:, 0]                       # second assignment: when parent == child (the root chosen) it is what remains
    w[parent == child, 1] = 0
    Rb = np.broadcast_to(np.eye(3), (K, 3, 3)) if R_bind is None else np.asarray(R_bind, np.float32).astype(np.float64)
    joints = np.stack([child, parent], -1)                                              # (N,2)
    local = np.einsum("njki,njk->nji", Rb[joints], points[:, None] - pos[joints])       # R^T (p - pos_j)
    return dict(child=child.astype(np.int32), parent=parent.astype(np.int32), w=w, local=local, margin=margin, dense=dense, nearest=nearest)


def fk(R, root_pos, offset, order, parents, dtype=np.float64):
    """R (T,K,3,3), root_pos (T,3), offset (K,3) -> (T,K,3): pos[root] = root_pos, pos[j] = R[j] offset[j] + pos[parents[j]] along `order`,
    clipped to [-1,1] at the end"""
    R, root_pos, offset = np.asarray(R, dtype), np.asarray(root_pos, dtype), np.asarray(offset, dtype).reshape(-1, 3)
    pos = np.zeros((R.shape[0], R.shape[1], 3), dtype)
    pos[:, int(order[0])] = root_pos
    for j in order[1:]:
        j = int(j)
        pos[:, j] = np.einsum("tab,b->ta", R[:, j], offset[j]) + pos[:, int(parents[j])]
    return np.clip(pos, -1, 1)


def pose(b, R, pos):
    """the blend on the bind record -> (T,N,3) float64"""
    R, pos = np.asarray(R, np.float64), np.asarray(pos, np.float64)
    out = np.zeros((R.shape[0], b["child"].shape[0], 3))
    for s, key in enumerate(("child", "parent")):
        j = b[key].astype(np.int64)
        out += b["w"][None, :, s, None].astype(np.float64) * (np.einsum("tnab,nb->tna", R[:, j], b["local"][:, s]) + pos[:, j])
    return out


def pose_dense(dense, points, kp_bind, R_bind, R, pos):
    """the reference's form: every point in the local frame of EVERY joint, transformed by every joint's frame matrix, blended with the
    dense (N,K) weights.  (T,N,3) float64, frame by frame."""
    points = np.asarray(points, np.float64)
    pb = np.asarray(kp_bind, np.float32)[:, :3].astype(np.float64)
    Rb = np.asarray(R_bind, np.float32).astype(np.float64)
    local = np.einsum("kji,nkj->nki", Rb, points[:, None] - pb[None])                   # (N,K,3)
    w = np.asarray(dense, np.float32).astype(np.float64)
    R, pos = np.asarray(R, np.float32).astype(np.float64), np.asarray(pos, np.float32).astype(np.float64)
    out = np.empty((R.shape[0], points.shape[0], 3))
    for t in range(R.shape[0]):
        kin = np.einsum("kab,nkb->nka", R[t], local) + pos[t][None]
        out[t] = np.einsum("nk,nka->na", w, kin)
    return out


def rotations(rng, *shape):
    """seeded random rotations: Gram-Schmidt of two Gaussian vectors (the 6-D parametrisation), columns [x|y|z], fp32"""
    a, b = rng.standard_normal((*shape, 3)), rng.standard_normal((*shape, 3))
    x = a / np.linalg.norm(a, axis=-1, keepdims=True)
    z = np.cross(x, b)
    z /= np.linalg.norm(z, axis=-1, keepdims=True)
    y = np.cross(z, x)
    return np.stack([x, y, z], -1).astype(np.float32)


def standin(seed, N=20000, K=24, T=8):
    """the stand-in inputs of the op-level tests: a figure's points normalised at scale 0.8, K keypoints near K of them with random
    intensities (the root's 0.9), a random tree, random bind / frame rotations, a smooth random walk of the root and random offsets.
    The order of the generator calls is part of the definition."""
    rng = np.random.default_rng(seed)
    pts = synth.episodic_normalization(synth.figure_points(1, N, rng), scale=0.8)[0]
    kp = np.zeros((K, 4), np.float32)
    kp[:, :3] = (pts[rng.choice(N, K, replace=False)] + 0.02 * rng.standard_normal((K, 3))).astype(np.float32)
    kp[:, 3] = rng.random(K).astype(np.float32)
    order = rng.permutation(K)
    parents = np.zeros(K, np.int64)
    root = int(order[0])
    parents[root] = root
    kp[root, 3] = 0.9
    for i in range(1, K):
        parents[order[i]] = order[rng.integers(0, i)]
    R_bind = rotations(rng, K)
    R = rotations(rng, T, K)
    walk = (np.cumsum(0.05 * rng.standard_normal((T, 3)), 0) + 0.2 * rng.standard_normal(3)).astype(np.float32)
    offset = (0.15 * rng.standard_normal((K, 3))).astype(np.float32)
    return dict(points=pts, keypoints=kp, order=order.astype(np.int32), parents=parents.astype(np.int32), root=root, R_bind=R_bind, R=R,
                root_pos=walk, offset=offset)


# ---- fixture G16 (tools/make_retarget_fixture.py writes it from the reference; the tests rebuild its inputs from the recorded seeds) ------
G16_SEEDS = dict(G=32, T=8, N=2048, weights=5, source=6, target=21, pick=22, eps_source=23, eps_target=24)


def g16_inputs(seeds=G16_SEEDS):
    """(options, state dict, source clip (T,1,G,G,G), target frame (1,G,G,G), target points (N,3) float64, eps_source (T,10,1,Z),
    eps_target (1,10,1,Z)): 'peaky' weights, a figure clip as the source, one frame of another figure normalised at scale 0.8 as the
    target, N of its points"""
    import torch
    from neural_marionette_amd import HotPathOptions
    s = seeds
    o = HotPathOptions(grid_size=s["G"])
    sd = synth.make_state_dict(o, seed=s["weights"], variant="peaky")
    source = synth.figure_clip(1, s["T"], s["G"], seed=s["source"])[0]
    pts = synth.episodic_normalization(synth.figure_points(1, 20000, np.random.default_rng(s["target"])), scale=0.8)[0]
    target = torch.from_numpy(synth.voxelize(pts, s["G"]))[None]
    points = np.ascontiguousarray(pts[np.random.default_rng(s["pick"]).choice(pts.shape[0], s["N"], replace=False)])
    Z = o.nlatent_kypt
    return o, sd, source, target, points, synth.make_eps((s["T"], 10, 1, Z), s["eps_source"]), synth.make_eps((1, 10, 1, Z), s["eps_target"])


def retarget(parents, order, source_kp, target_kp, R, R_bind, offset, points, hardness=8.0, threshold=0.2, force_child=None):
    """the driver after the two encodes: bind, forward kinematics (fp32, as the reference) with the source's root trajectory, blend"""
    root = int(order[0])
    b = bind(parents, root, points, target_kp, R_bind, hardness, threshold, force_child)
    pos = fk(R, np.asarray(source_kp, np.float32)[:, root, :3], offset, order, parents, np.float32)
    return b, pos, pose(b, R, pos)
