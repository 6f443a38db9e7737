"""numpy / torch-CPU restatement of the host lines every consumer of the decoder's voxels in the reference starts with, run
literally: vis_generation.py:137-170 and vis_interpolation.py:141-177 (float64: the in-place binarisation, the per-frame np.where
loop, the two-pass min_z / max_z, the shading's (z - min_z) / z_len) and vis/visualize.py:130-137 (float32: vis_recon's
binarisation and its per-frame torch.where + stack + divide).  What NeuralMarionette.occupied_points is compared with, bit for bit.

Two places where the scripts themselves would stop are continued here, as the device path continues: a frame without a point is
skipped in the min_z / max_z pass (``coords[:, -1].min()`` of an empty array raises), and a clip whose points share one z divides
0 by 0 (numpy warns and gives NaN)."""
import numpy as np
import torch


def _six(vox):
    x = torch.as_tensor(np.asarray(vox) if not isinstance(vox, torch.Tensor) else vox).detach().cpu()
    assert x.dtype == torch.float32 and x.dim() in (5, 6)
    x = x.clone()
    return x if x.dim() == 6 else x[None]


def _z_pass(frames):
    """vis_generation.py:143-153 over the (N, 3) coordinate arrays of one clip's frames"""
    min_z = 1e4
    max_z = -1
    for coords in frames:
        if len(coords) == 0:
            continue
        if min_z > coords[:, -1].min():
            min_z = coords[:, -1].min()
        if max_z < coords[:, -1].max():
            max_z = coords[:, -1].max()
    return min_z, max_z


def occupied_points(vox, threshold=0.5, dtype=np.float64):
    """vox (T,1,G,G,G) or (B,T,1,G,G,G) float32.  Returns what NeuralMarionette.occupied_points returns with every optional output,
    as numpy arrays: coords (N,3) `dtype`, offsets (F+1) int64, counts (B,T) int64, z_range (B,2) `dtype`, indices (N,3) int32, bits
    (F, 8 ceil(G^3/64)) uint8 and, for float64, depth (N) float64."""
    dtype = np.dtype(dtype)
    assert dtype in (np.dtype(np.float64), np.dtype(np.float32))
    x = _six(vox)
    B, T, _, G = x.shape[:4]
    X = [G, G, G]
    if threshold is not None:
        thr = float(np.float32(threshold))
        x[x < thr] = 0                                            # vis_generation.py:138-139, visualize.py:130-131
        x[x >= thr] = 1
    coords_all, idx_all, depth_all, counts, z_range, bits = [], [], [], np.zeros((B, T), np.int64), np.zeros((B, 2), dtype), []
    for b in range(B):
        frames = []
        for t in range(T):
            if dtype == np.float64:
                where = np.where(x[b, t, 0].clone().detach().cpu().numpy())
                coords = np.stack(where, axis=-1) / ((G - 1) / 2) - 1                            # vis_generation.py:147
            else:
                where = torch.where(x[b, t, 0])
                coords = (torch.stack(where, dim=-1) / ((X[0] - 1) / 2) - 1).numpy()               # visualize.py:136
                where = tuple(w.numpy() for w in where)
            assert coords.dtype == dtype
            frames.append(coords)
            idx_all.append(np.stack(where, axis=-1).astype(np.int32))
            counts[b, t] = len(coords)
            occ = x[b, t, 0].numpy().astype(bool).reshape(-1)
            packed = np.packbits(occ, bitorder="little")
            bits.append(np.concatenate([packed, np.zeros(-len(packed) % 8, np.uint8)]))
        min_z, max_z = _z_pass(frames)
        z_range[b] = (min_z, max_z)
        if dtype == np.float64:
            z_len = (max_z - min_z)                                                              # vis_generation.py:153
            with np.errstate(invalid="ignore", divide="ignore"):
                for coords in frames:
                    depth_all.append((coords[:, -1] - min_z) / z_len)          # :167, the loop over i as one array expression
        coords_all += frames
    out = dict(coords=np.concatenate(coords_all).reshape(-1, 3).astype(dtype, copy=False),
               indices=np.concatenate(idx_all).reshape(-1, 3),
               offsets=np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int64),
               counts=counts, z_range=z_range, bits=np.stack(bits))
    if dtype == np.float64:
        out["depth"] = np.concatenate(depth_all).astype(np.float64)
    return out
