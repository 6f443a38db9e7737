"""float64 numpy restatement of the mesh sampling contract of include/nm355.h (nm_sample_surface), operation by operation.

It is the library's own contract - trimesh's algorithm (a face by area, a point in it by two uniforms folded into the triangle) with
integer weights instead of a float cumulative sum - and claims nobody else's bits.  `side` and `reflect` exist so that the tests can
break the restatement on purpose (tests/test_sample_surface_cpu.py: the mutations).
"""
import numpy as np

MAX_FACES = 1 << 21
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or numbers) of 32-bit words, key: two -> the four output words as uint64 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in counter)
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                              # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def unit(hi, lo):
    """a pair of 32-bit words -> [0, 1): ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53, every step exact"""
    hi, lo = np.asarray(hi, dtype=np.uint64), np.asarray(lo, dtype=np.uint64)
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


def uniforms(seed, T, count):
    """(T, count, 3) float64: the device's stream for `seed`"""
    seed = int(seed) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    s = np.arange(count, dtype=np.uint64)[None, :]
    t = np.arange(T, dtype=np.uint64)[:, None] + np.zeros_like(s)
    s = s + np.zeros_like(t)
    x = philox4x32_10((s & _MASK, s >> _S32, t, np.zeros_like(s)), key)
    y = philox4x32_10((s & _MASK, s >> _S32, t, np.ones_like(s)), key)
    return np.stack([unit(x[0], x[1]), unit(x[2], x[3]), unit(y[0], y[1])], axis=-1)


def face_records(vertices, triangles):
    """step 1: areas (T,F) float64, normals (T,F,3) float32, bad (F) bool"""
    v = np.asarray(vertices).astype(np.float64)                     # float32 is widened exactly
    tri = np.asarray(triangles).astype(np.int64)
    T, V = v.shape[0], v.shape[1]
    bad = ((tri < 0) | (tri >= V)).any(axis=1)
    safe = np.where(bad[:, None], 0, tri)
    v0, v1, v2 = v[:, safe[:, 0]], v[:, safe[:, 1]], v[:, safe[:, 2]]
    with np.errstate(all="ignore"):
        a, b = v1 - v0, v2 - v0
        cx = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
        cy = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
        cz = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
        n2 = (cx * cx + cy * cy) + cz * cz
        r = np.sqrt(n2)
        area = 0.5 * r
        normal = np.stack([cx / r, cy / r, cz / r], axis=-1)
    ok = (n2 != 0.0) & np.isfinite(n2) & ~bad[None, :]
    normal = np.where(ok[..., None], normal, 0.0).astype(np.float32)
    area = np.where(bad[None, :], 0.0, area)
    return area, normal, bad


def weights(areas):
    """step 2: (T,F) uint64 integer weights of (T,F) float64 areas"""
    areas = np.asarray(areas, dtype=np.float64)
    finite = np.isfinite(areas)
    amax = np.where(finite, areas, 0.0).max(axis=1)
    _, e = np.frexp(amax)
    with np.errstate(all="ignore"):
        scaled = np.floor(np.ldexp(np.where(finite, areas, 0.0), (32 - e.astype(np.int64))[:, None].astype(np.int32)))
    assert (scaled < 2.0 ** 32).all() and (scaled >= 0).all()
    return scaled.astype(np.uint64)


def cumulative(w):
    return np.cumsum(w, axis=-1, dtype=np.uint64)


def pick_index(u0, W):
    """p = min(floor(u0 * W), W - 1) as uint64 (W > 0)"""
    x = np.floor(np.asarray(u0, dtype=np.float64) * float(W))
    return np.minimum(x.astype(np.uint64), np.uint64(int(W) - 1))


def pick_face(cum, p, side="right"):
    """the smallest i with cum[i] > p"""
    return np.searchsorted(cum, p, side=side)


def fold(u1, u2, reflect=True):
    u1, u2 = np.array(u1, dtype=np.float64), np.array(u2, dtype=np.float64)
    if reflect:
        over = u1 + u2 > 1.0
        u1 = np.where(over, np.abs(u1 - 1.0), u1)
        u2 = np.where(over, np.abs(u2 - 1.0), u2)
    return u1, u2


def sample(vertices, triangles, u, areas=None, side="right", reflect=True):
    """The whole contract for uniforms u (T,count,3).  areas: take these (T,F) float64 areas for steps 2-4 instead of step 1's (the
    device's own, so that a comparison does not depend on its square root's last bit).
    Returns areas, face_normals (T,F,3) f32, weights, cum (T,F) uint64, face_index (T,count) int32, points, normals (T,count,3) f32,
    bad_faces, empty_frames."""
    v = np.asarray(vertices).astype(np.float64)
    tri = np.asarray(triangles).astype(np.int64)
    u = np.asarray(u, dtype=np.float64)
    T, V, F, count = v.shape[0], v.shape[1], tri.shape[0], u.shape[1]
    assert 1 <= F <= MAX_FACES and u.shape == (T, count, 3)
    area1, fnormal, bad = face_records(v, tri)
    area = area1 if areas is None else np.asarray(areas, dtype=np.float64)
    w = weights(area)
    cum = cumulative(w)
    face = np.zeros((T, count), np.int32)
    points = np.zeros((T, count, 3), np.float32)
    normals = np.zeros((T, count, 3), np.float32)
    empty = 0
    for t in range(T):
        W = int(cum[t, -1])
        if W == 0:
            empty += 1
            i0 = int(tri[0, 0])
            points[t] = v[t, i0].astype(np.float32) if 0 <= i0 < V else 0.0
            continue
        f = pick_face(cum[t], pick_index(u[t, :, 0], W), side=side)
        f = np.minimum(f, F - 1)                                    # (only a mutated search can run past the end)
        u1, u2 = fold(u[t, :, 1], u[t, :, 2], reflect=reflect)
        ft = np.where(bad[f, None], 0, tri[f])
        v0 = v[t, ft[:, 0]]
        a, b = v[t, ft[:, 1]] - v0, v[t, ft[:, 2]] - v0
        with np.errstate(all="ignore"):
            points[t] = (v0 + (a * u1[:, None] + b * u2[:, None])).astype(np.float32)
        normals[t] = fnormal[t, f]
        face[t] = f
    return dict(areas=area, face_normals=fnormal, weights=w, cum=cum, face_index=face, points=points, normals=normals,
                bad_faces=int(bad.sum()), empty_frames=empty)


def u0_for(p, W):
    """a u0 in [0, 1) with floor(u0 * W) == p, for 0 <= p < W (checked, not assumed)"""
    p, W = int(p), int(W)
    assert 0 <= p < W
    u = min((p + 0.5) / W, 1.0 - 2.0 ** -53)
    for cand in (u, np.nextafter(u, 1.0), np.nextafter(u, 0.0)):
        if cand < 1.0 and int(np.floor(cand * float(W))) == p:
            return float(cand)
    raise AssertionError(f"no float64 u0 reaches p = {p} of W = {W}")


def ulp_distance(a, b):
    """|a - b| in units of the last place, for finite arrays of one float dtype and one sign convention (+0 only)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    it = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    lim = np.int64(np.iinfo(it).min)
    ia = np.where(ia < 0, lim - ia, ia)                              # sign-magnitude -> a monotone integer line
    ib = np.where(ib < 0, lim - ib, ib)
    return np.abs(ia - ib)
