"""Fixtures larger than a committed file may be (1 MiB) are stored as parts: `<stem>.part0.npz`, `<stem>.part1.npz`, ...

save() writes `<stem>.npz` when the arrays fit in one part, else cuts every array larger than PART_BYTES into flat pieces and packs
the pieces into parts of at most PART_BYTES uncompressed each.  load() returns the same mapping either way (arrays bit for bit as
saved; `.files` lists the names like NpzFile's)."""
import glob
import os

import numpy as np

PART_BYTES = 768 * 1024


class Fixture(dict):
    @property
    def files(self):
        return list(self)


def save(path, **arrays):
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    stem = path[:-4] if path.endswith(".npz") else path
    for old in glob.glob(glob.escape(stem) + ".part*.npz"):
        os.remove(old)
    if sum(a.nbytes for a in arrays.values()) <= PART_BYTES:
        np.savez_compressed(stem + ".npz", **arrays)
        return [stem + ".npz"]
    if os.path.exists(stem + ".npz"):
        os.remove(stem + ".npz")
    pieces = []                                     # (key, array) in save order
    for k, a in arrays.items():
        if a.nbytes <= PART_BYTES:
            pieces.append((k, a))
            continue
        flat = np.ascontiguousarray(a).reshape(-1)
        step = max(1, PART_BYTES // a.itemsize)
        pieces.append((f"{k}@shape", np.array(a.shape, dtype=np.int64)))
        for j, lo in enumerate(range(0, flat.size, step)):
            pieces.append((f"{k}@piece{j}", flat[lo:lo + step]))
    parts, cur, size = [], {}, 0
    for k, a in pieces:
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    out = []
    for i, p in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i}.npz", **p)
        out.append(f"{stem}.part{i}.npz")
    return out


def load(path):
    stem = path[:-4] if path.endswith(".npz") else path
    if os.path.exists(stem + ".npz"):
        with np.load(stem + ".npz", allow_pickle=False) as z:
            return Fixture({k: z[k] for k in z.files})
    files = sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda f: int(f[len(stem) + 5:-4]))
    if not files:
        raise FileNotFoundError(stem + ".npz")
    raw = {}
    for f in files:
        with np.load(f, allow_pickle=False) as z:
            raw.update({k: z[k] for k in z.files})
    out = Fixture()
    for k, a in raw.items():
        if "@piece" in k:
            continue
        if k.endswith("@shape"):
            name = k[:-len("@shape")]
            n = sum(1 for q in raw if q.startswith(name + "@piece"))
            out[name] = np.concatenate([raw[f"{name}@piece{j}"] for j in range(n)]).reshape(tuple(a))
        else:
            out[k] = a
    return out
