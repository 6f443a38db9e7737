"""The mesh sampling contract (include/nm355.h, nm_sample_surface) as tests/sample_ref.py restates it, pinned without a device: the
generator's known answers, a hand-worked mesh whose every number is dyadic, the edges of the pick, faces that must never be picked, a
frequency check, and two mutations of the restatement that the named cases must catch.  The last tests look at the library's shell:
arguments are judged before any context exists.

Without the feature (the parent commit): this module does not import - there is no tests/sample_ref.py restating a contract that
does not exist - and NeuralMarionette has no sample_surface."""
import numpy as np
import pytest
import torch

import sample_ref as S
from neural_marionette_amd import NeuralMarionette, HotPathOptions
from neural_marionette_amd.data import ClipBank

TOP = 1.0 - 2.0 ** -53                                             # the largest uniform

# three right triangles in the plane z = 0, legs (2, 2), (1, 2), (1, 1): areas 2, 1, 0.5; amax = 2 = 0.5 * 2^2, so e = 2 and the
# weights are area * 2^30 = 2^31, 2^30, 2^29; Cum = 2^31, 3 * 2^30, 7 * 2^29
HAND_V = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0],
                    [4, 0, 0], [5, 0, 0], [4, 2, 0],
                    [8, 0, 0], [9, 0, 0], [8, 1, 0]]], dtype=np.float64)
HAND_T = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32)
HAND_CUM = [2 ** 31, 3 * 2 ** 30, 7 * 2 ** 29]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join(f"{int(x):08x}" for x in S.philox4x32_10(counter, key)) == want
    # vectorised over counters = the scalar calls
    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88])
    got = S.philox4x32_10((c0, c0, c0, c0), (7, 9))
    for i, c in enumerate(c0):
        assert [int(g[i]) for g in got] == [int(x) for x in S.philox4x32_10((c, c, c, c), (7, 9))]


def test_bits_to_double_rule():
    assert float(S.unit(0xFFFFFFFF, 0xFFFFFFFF)) == TOP
    assert float(S.unit(0, 0)) == 0.0 and float(S.unit(0x1F, 0x3F)) == 0.0          # the dropped low bits
    assert float(S.unit(0x20, 0)) == 2.0 ** -27 and float(S.unit(0, 0x40)) == 2.0 ** -53
    assert float(S.unit(0x80000000, 0)) == 0.5
    u = S.uniforms(0x0123456789ABCDEF, 3, 5)
    assert u.shape == (3, 5, 3) and u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    # counter (s, s >> 32, t, call), key (seed & 0xffffffff, seed >> 32); u0, u1 from call 0, u2 from call 1
    x = S.philox4x32_10((4, 0, 2, 0), (0x89ABCDEF, 0x01234567))
    y = S.philox4x32_10((4, 0, 2, 1), (0x89ABCDEF, 0x01234567))
    assert u[2, 4].tolist() == [float(S.unit(x[0], x[1])), float(S.unit(x[2], x[3])), float(S.unit(y[0], y[1]))]
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u, S.uniforms(0x0123456789ABCDEE, 3, 5))


def test_hand_worked_mesh_tables():
    area, normal, bad = S.face_records(HAND_V, HAND_T)
    assert area.tolist() == [[2.0, 1.0, 0.5]] and not bad.any()
    assert normal.dtype == np.float32 and normal.tolist() == [[[0, 0, 1]] * 3]
    w = S.weights(area)
    assert w.dtype == np.uint64 and w.tolist() == [[2 ** 31, 2 ** 30, 2 ** 29]]
    assert S.cumulative(w).tolist() == [HAND_CUM]
    # float32 vertices are widened exactly; int64 triangles are the same triangles
    r32 = S.sample(HAND_V.astype(np.float32), HAND_T.astype(np.int64), np.zeros((1, 1, 3)))
    assert r32["cum"].tolist() == [HAND_CUM] and r32["areas"].dtype == np.float64
    # another exponent: the mesh scaled by 2^-10 has areas scaled by 2^-20 and the SAME integer weights
    assert S.weights(S.face_records(HAND_V * 2.0 ** -10, HAND_T)[0]).tolist() == w.tolist()


def _case_boundary_picks(side="right"):
    """p = Cum[i] - 1 is the last integer of face i, p = Cum[i] the first of face i + 1; u0 = 0 and u0 = 1 - 2^-53 are the two ends"""
    cum = np.array(HAND_CUM, dtype=np.uint64)
    W = HAND_CUM[-1]
    for i in range(3):
        assert int(S.pick_face(cum, np.uint64(HAND_CUM[i] - 1), side=side)) == i, f"p = Cum[{i}] - 1"
        if i < 2:
            assert int(S.pick_face(cum, np.uint64(HAND_CUM[i]), side=side)) == i + 1, f"p = Cum[{i}]"
    u0 = [S.u0_for(HAND_CUM[0] - 1, W), S.u0_for(HAND_CUM[0], W), S.u0_for(HAND_CUM[1] - 1, W), S.u0_for(HAND_CUM[1], W), 0.0, TOP]
    assert S.pick_index(u0, W).tolist() == [HAND_CUM[0] - 1, HAND_CUM[0], HAND_CUM[1] - 1, HAND_CUM[1], 0, W - 1]
    u = np.zeros((1, len(u0), 3))
    u[0, :, 0] = u0
    r = S.sample(HAND_V, HAND_T, u, side=side)
    assert r["face_index"].tolist() == [[0, 1, 1, 2, 0, 2]]
    assert r["points"][0].tolist() == [[0, 0, 0], [4, 0, 0], [4, 0, 0], [8, 0, 0], [0, 0, 0], [8, 0, 0]]       # u1 = u2 = 0: v0 of the face


def _case_reflection(reflect=True):
    """u1 + u2 == 1 exactly lies on the hypotenuse and is NOT reflected; anything above is, through the hypotenuse's midpoint"""
    u = np.array([[[0.0, 0.25, 0.75], [0.0, 0.5, 0.75], [0.0, TOP, TOP], [0.0, 0.5, 0.5 + 2.0 ** -53]]])
    r = S.sample(HAND_V, HAND_T, u, reflect=reflect)
    # face 0: v0 = 0, a = (2, 0, 0), b = (0, 2, 0): point = (2 u1, 2 u2, 0)
    assert r["points"][0, 0].tolist() == [0.5, 1.5, 0.0]                      # on the edge, as drawn
    assert r["points"][0, 1].tolist() == [1.0, 0.5, 0.0]                      # (0.5, 0.75) -> (0.5, 0.25)
    assert r["points"][0, 2].tolist() == [2.0 ** -52, 2.0 ** -52, 0.0]        # the far corner folds onto v0's neighbourhood
    # 0.5 + (0.5 + 2^-53) rounds to 1.0 in float64 (ties to even): not above 1, not reflected
    assert r["points"][0, 3].tolist() == [1.0, float(np.float32(2.0 * (0.5 + 2.0 ** -53))), 0.0]
    pts = r["points"][0].astype(np.float64)
    assert (pts[:, 0] + pts[:, 1] <= 2.0).all(), "a sample left its triangle"


def test_boundary_picks():
    _case_boundary_picks()


def test_reflection():
    _case_reflection()


def test_mutations_are_caught():
    """searchsorted(side='left') returns the first i with Cum[i] >= p: one face early at every p = Cum[i]; without the reflection half
    of the samples leave the triangle.  The named cases must notice both."""
    with pytest.raises(AssertionError):
        _case_boundary_picks(side="left")
    with pytest.raises(AssertionError):
        _case_reflection(reflect=False)


def test_largest_uniform_stays_below_every_total():
    for W in (1, 2, 3, 2 ** 31, 3 * 2 ** 30, 7 * 2 ** 29, 2 ** 52 + 1, 2 ** 53 - 1):
        assert float(W) == W                                          # (double) W is exact below 2^53
        assert np.floor(TOP * float(W)) < W, W
        assert int(S.pick_index(TOP, W)) == W - 1 and int(S.pick_index(0.0, W)) == 0


def test_faces_without_weight_are_never_picked():
    """a zero-area face in the middle, a face below amax * 2^-32 and a degenerate face 0 take no integer of [0, W)"""
    t = 2.0 ** -17                                                  # legs t, t: area 2^-35 < 2 * 2^-32
    v = np.array([[[0, 0, 0], [1, 1, 0], [2, 2, 0],                # face 0: collinear
                   [0, 0, 0], [2, 0, 0], [0, 2, 0],                # face 1: area 2
                   [3, 3, 3], [3, 3, 3], [4, 4, 4],                # face 2: two equal vertices
                   [5, 0, 0], [5 + t, 0, 0], [5, t, 0],            # face 3: tiny
                   [6, 0, 0], [7, 0, 0], [6, 1, 0]]], np.float64)   # face 4: area 0.5
    tri = np.arange(15, dtype=np.int32).reshape(5, 3)
    area, normal, _ = S.face_records(v, tri)
    assert area[0, 0] == 0 and area[0, 2] == 0 and area[0, 3] == 2.0 ** -35
    assert normal[0, 0].tolist() == [0, 0, 0] and normal[0, 2].tolist() == [0, 0, 0] and normal[0, 3].tolist() == [0, 0, 1]
    w = S.weights(area)
    assert w.tolist() == [[0, 2 ** 31, 0, 0, 2 ** 29]]
    cum = S.cumulative(w)[0]
    W = int(cum[-1])
    p = np.concatenate([np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, W - 1], np.uint64),
                        np.random.default_rng(3).integers(0, W, 100000, dtype=np.uint64)])
    assert set(S.pick_face(cum, p).tolist()) == {1, 4}
    u = np.zeros((1, 4, 3))
    u[0, :, 0] = [0.0, S.u0_for(2 ** 31 - 1, W), S.u0_for(2 ** 31, W), TOP]
    assert S.sample(v, tri, u)["face_index"].tolist() == [[1, 1, 4, 4]]
    # all faces degenerate: no surface - v0 of face 0, zero normals, face 0, and the frame is counted
    r = S.sample(v[:, :3] + 1.0, tri[:1], u)
    assert r["empty_frames"] == 1 and r["face_index"].tolist() == [[0] * 4] and r["points"][0].tolist() == [[1, 1, 1]] * 4
    assert not r["normals"].any()
    # a face with an index outside the vertices: no area, counted, never picked
    r = S.sample(v, np.concatenate([tri, [[0, 1, 99]], [[-1, 1, 2]]]).astype(np.int64), S.uniforms(1, 1, 1000))
    assert r["bad_faces"] == 2 and r["areas"][0, 5:].tolist() == [0, 0] and set(r["face_index"][0].tolist()) == {1, 4}


def test_faces_are_sampled_by_area():
    """97 random faces, 400 000 picks with the generator's uniforms: every face's count within 6 sigma of N w_i / W (sigma = the
    square root of that expectation; the largest deviation seen when the contract was written was 153 against 111, under 2 sigma)"""
    rng = np.random.default_rng(11)
    v = rng.standard_normal((1, 3 * 97, 3))
    tri = np.arange(3 * 97, dtype=np.int32).reshape(97, 3)
    N = 400000
    r = S.sample(v, tri, S.uniforms(2024, 1, N))
    w = r["weights"][0].astype(np.float64)
    expect = N * w / w.sum()
    got = np.bincount(r["face_index"][0], minlength=97)
    dev = np.abs(got - expect)
    print(f"largest count deviation {dev.max():.0f}, sqrt(max expected) {np.sqrt(expect.max()):.0f}, worst {np.max(dev / np.sqrt(expect)):.2f} sigma")
    assert (dev <= 6.0 * np.sqrt(expect)).all()
    # and inside a face uniformly: the mean of the barycentric pair of a folded draw is (1/3, 1/3)
    u1, u2 = S.fold(*S.uniforms(5, 1, N)[0, :, 1:].T)
    assert (u1 + u2 <= 1.0).all() and abs(u1.mean() - 1 / 3) < 6 * np.sqrt(1 / 18 / N) and abs(u2.mean() - 1 / 3) < 6 * np.sqrt(1 / 18 / N)


def test_arguments_are_judged_before_the_context():
    """wrong dtypes, ranks, sizes: ValueError from the shell, on CPU tensors, before any library call"""
    net = NeuralMarionette(HotPathOptions(grid_size=32))
    v, t = torch.zeros(2, 9, 3), torch.zeros(4, 3, dtype=torch.int32)
    bad = [dict(vertices=v.half()), dict(vertices=v[0]), dict(vertices=torch.zeros(2, 9, 2)), dict(vertices=torch.zeros(0, 9, 3)),
           dict(vertices=v.numpy()), dict(triangles=t.float()), dict(triangles=t[0]), dict(triangles=torch.zeros(4, 4, dtype=torch.int32)),
           dict(triangles=torch.zeros(0, 3, dtype=torch.int32)), dict(triangles=torch.zeros(2 ** 21 + 1, 3, dtype=torch.int32)),
           dict(count=0), dict(count=-5), dict(count=2.5), dict(u=torch.zeros(2, 20000, 2, dtype=torch.float64)),
           dict(u=torch.zeros(2, 20000, 3)), dict(count=7, u=torch.zeros(2, 8, 3, dtype=torch.float64)), dict()]      # (the last: CPU tensors)
    for kw in bad:
        args = dict(vertices=v, triangles=t)
        args.update(kw)
        with pytest.raises(ValueError):
            net.sample_surface(**args)
    with pytest.raises(ValueError):
        ClipBank("cpu").add_mesh(net, v, t.float())
