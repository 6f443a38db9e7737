"""The batch input path on the device (nm_voxelize_batch through NeuralMarionette.voxelize_batch, data.ClipBank / ClipSampler /
DeviceClipLoader) against fixture G18 - what the reference's dataset classes and utils.dataset_utils returned - and against the numpy
restatement tests/input_path_ref.py, which tests/test_input_path_cpu.py pins to that fixture.

Every comparison is bit for bit: the outputs are {0,1} voxels, integer indices, and normalised joints / box corners that the kernel
computes with the reference's own sequence of roundings, so there is no tolerance to derive.  Shapes: G = 32 and 40 (64 for the third
float32-sensitive clip), N = 257, 500 and 1000 (one partial tile / two / four tiles of 256 points), T = 3 and 6, B = 3 with sequences of
three different lengths."""
import os
import random

import numpy as np
import pytest
import torch

import golden_npz
import input_path_ref as IR
from neural_marionette_amd import NeuralMarionette, HotPathOptions, synth
from neural_marionette_amd.data import ClipBank, ClipSampler, DeviceClipLoader

pytestmark = pytest.mark.gpu

G18 = IR.G18
_NETS = {}


@pytest.fixture(scope="module")
def g18(golden_dir):
    return golden_npz.load(os.path.join(golden_dir, "g18_input_path.npz"))


def _net(G):
    if G not in _NETS:
        o = HotPathOptions(grid_size=G)
        net = NeuralMarionette(o)
        net.load_state_dict(synth.make_state_dict(o, seed=1))
        _NETS[G] = net.cuda().eval()
    return _NETS[G]


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = (_bits(got), _bits(want)) if got.dtype.kind == "f" else (got, want)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} entries differ"


def _bank(seqs, joints=True):
    bank = ClipBank("cuda")
    for p, j in seqs:
        bank.add(p, j if joints else None)
    return bank


def _dataset_cases():
    for tag in ("aist", "dfaust"):
        for rate in G18["rates"]:
            for mode in ("e0", "e1", "e7", "rand"):
                yield f"a_{tag}_r{rate}_{mode}", tag == "aist", rate, mode, False
    yield "a_short_r1_rand", False, 1, "rand", True


@pytest.mark.parametrize("key,with_joints,rate,mode,short", list(_dataset_cases()), ids=[c[0] for c in _dataset_cases()])
def test_batch_reproduces_the_reference_datasets(g18, key, with_joints, rate, mode, short):
    """items 0..2 of an AIST(is_eval=1) / DFAUST object as ONE batch: float32 files of three lengths, sample_rate 1 and 2, the
    epoch-selected and the random crop, and the padded clip of a 4-frame file"""
    seqs = IR.g18_sequences(short=short)
    T, G = G18["T"], G18["G"]
    bank = _bank(seqs, with_joints)
    assert bank.nbytes == sum(p.nbytes + (j.nbytes if with_joints else 0) for p, j in seqs) and bank.points[0].dtype == torch.float32
    s = ClipSampler(bank.lengths, T, rate, mode == "rand", random.Random(G18["dataset_seed"]), has_joints=with_joints)
    if mode != "rand":
        s.log_epoch(int(mode[1:]))
    crops = [s.crop(i) for i in range(len(s))]
    assert [c[1] for c in crops] == g18[key + "__starts"].tolist()
    out = _net(G).voxelize_batch(bank, [c[0] for c in crops], [c[1] for c in crops], T, sample_rate=rate, pad=[c[2] for c in crops],
                                 return_joints=with_joints, return_indices=True, check=True)
    B = len(crops)
    assert tuple(out["vox"].shape) == (B, T, 1, G, G, G) and out["vox"].dtype == torch.float32
    vox = _np(out["vox"])
    for b, (seq, start, pad) in enumerate(crops):
        _same(IR.pack(vox[b]), g18[key + "__vox"][b], f"voxels of item {b}")
        r = IR.clip(seqs[seq][0], start, T, rate, pad, G)
        _same(_np(out["indices"][b]), r["idx"], f"indices of item {b}")
        _same(_np(out["bbox"][b]), r["bbox"], f"box of item {b}")
        if with_joints:
            _same(_np(out["joints"][b]), g18[key + "__joints"][b], f"joints of item {b}")
    assert _np(out["bad_rows"]).tolist() == [0] * B
    assert any(c[2] for c in crops) == short


@pytest.mark.parametrize("name", sorted(IR.G18_CLIPS))
def test_normalisation_translation_and_wrapped_indices(g18, name):
    """episodic_normalization + voxelize of float32 and float64 clips with scale and translation: indices in [-G,-1] wrap like
    numpy's, rows the reference cannot scatter are counted and check=True raises its error"""
    dtype, T, N, G, scale, xt, zt = IR.G18_CLIPS[name]
    x = IR.g18_clip(name)
    bank = ClipBank("cuda")
    bank.add(x)
    net = _net(G)
    kw = dict(scale=scale, x_trans=xt, z_trans=zt)
    out = net.voxelize_batch(bank, [0], [0], T, return_indices=True, **kw)
    r = IR.clip(x, 0, T, 1, False, G, scale, xt, zt)
    _same(_np(out["indices"][0]), g18[f"b_{name}__idx"], "indices")
    _same(_np(out["bbox"][0]), r["bbox"], "box")
    bad = int(g18[f"b_{name}__bad"])
    assert _np(out["bad_rows"]).tolist() == [bad] == [int(r["bad"].sum())]
    if int(g18[f"b_{name}__raised"]):
        _same(_np(out["vox"][0]), r["vox"], "voxels (the rows the reference refuses set nothing)")
        with pytest.raises(ValueError, match="Dataset voxelizer error"):
            net.voxelize_batch(bank, [0], [0], T, check=True, **kw)
    else:
        _same(IR.pack(_np(out["vox"][0])), g18[f"b_{name}__vox"], "voxels")
        net.voxelize_batch(bank, [0], [0], T, check=True, **kw)


@pytest.mark.parametrize("pd", ["float32", "float64"])
@pytest.mark.parametrize("jd", ["float32", "float64"])
def test_joint_dtype_combinations(g18, pd, jd):
    x, j = IR.g18_joint_case(pd, jd)
    bank = ClipBank("cuda")
    bank.add(x, j)
    out = _net(32).voxelize_batch(bank, [0], [0], x.shape[0], scale=0.9, return_joints=True)
    _same(_np(out["joints"][0]), g18[f"c_{pd}_{jd}__joints"], "joints")
    _same(_np(out["vox"][0]), IR.clip(x, 0, x.shape[0], 1, False, 32, 0.9)["vox"], "voxels")


@pytest.mark.parametrize("G", IR.HARD_GRIDS)
def test_float32_clips_that_upcast_arithmetic_gets_wrong(g18, G):
    """f32_hard: at least 8 rows of each clip land in another voxel when float32 data is widened before the normalisation
    (tests/test_input_path_cpu.py asserts the count): an implementation that upcasts fails here"""
    x = g18[f"d_hard{G}__points"]
    bank = ClipBank("cuda")
    bank.add(x)
    out = _net(G).voxelize_batch(bank, [0], [0], IR.HARD_T, scale=0.9, return_indices=True, check=True)
    _same(_np(out["indices"][0]), g18[f"d_hard{G}__idx"], "indices")
    _same(IR.pack(_np(out["vox"][0])), g18[f"d_hard{G}__vox"], "voxels")


def _three_sequences(dtype, N):
    """three sequences of different lengths whose boxes differ by far (a clip that read another clip's box would miss every voxel)"""
    seqs = []
    for i, (frames, mul, shift) in enumerate(((9, 1.0, 0.0), (14, 3.5, -4.0), (5, 0.2, 11.0))):
        p, j = IR.sequence(77, i, frames, N, np.float64, J=5)
        seqs.append(((p * mul + shift).astype(dtype), (j * mul + shift).astype(dtype)))
    return seqs


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_batch_equals_per_clip_calls(dtype):
    """B = 3 clips of different sequences, strides, scales and translations, one of them padded: the batch is the three single-clip
    results (no clip sees another's box) and the restatement's"""
    G, N, T, rate = 40, 257, 3, 2
    seqs = _three_sequences(dtype, N)
    bank = _bank(seqs)
    net = _net(G)
    ids, starts, pads = [1, 0, 2], [7, 4, 0], [False, False, True]              # sequence 2: 5 frames, frames 0, 2, 4 - and 1 below
    scale, xt, zt = [1.0, 0.8, 0.9], [0.0, 0.1, 0.0], [0.0, -0.1, 0.05]
    kw = dict(sample_rate=rate, return_joints=True, return_indices=True)
    both = net.voxelize_batch(bank, ids, starts, T, scale=scale, x_trans=xt, z_trans=zt, pad=pads, **kw)
    for b in range(3):
        one = net.voxelize_batch(bank, [ids[b]], [starts[b]], T, scale=scale[b], x_trans=xt[b], z_trans=zt[b], pad=[pads[b]], **kw)
        r = IR.clip(seqs[ids[b]][0], starts[b], T, rate, pads[b], G, scale[b], xt[b], zt[b], joints=seqs[ids[b]][1])
        for k, ref in (("vox", r["vox"]), ("indices", r["idx"]), ("bbox", r["bbox"]), ("joints", r["joints"])):
            assert torch.equal(both[k][b], one[k][0]), (k, b)
            _same(_np(both[k][b]), ref, f"{k} of clip {b}")
        assert int(both["bad_rows"][b]) == int(one["bad_rows"][0]) == int(r["bad"].sum())
    # a padded crop that really repeats the last frame: T = 6 frames of the 5-frame sequence at stride 1
    out = net.voxelize_batch(bank, [2], [0], 6, pad=[True], return_indices=True)
    _same(_np(out["indices"][0]), IR.clip(seqs[2][0], 0, 6, 1, True, G)["idx"], "padded indices")
    assert torch.equal(out["vox"][0, 4], out["vox"][0, 5])
    with pytest.raises(ValueError, match="does not fit"):                       # without pad the same crop is refused before any launch
        net.voxelize_batch(bank, [2], [0], 6)
    with pytest.raises(ValueError, match="does not fit"):
        net.voxelize_batch(bank, [0], [5], T, sample_rate=rate)


def test_back_to_back_calls_keep_their_descriptors():
    """more calls than the staging ring has buffers, none waited for: every call's descriptor table must reach the device intact"""
    G, N, T = 32, 257, 3
    seqs = _three_sequences("float32", N)
    bank = _bank(seqs, joints=False)
    net = _net(G)
    torch.cuda.synchronize()
    calls = [([i % 3, (i + 1) % 3], [i % 3, (i * 2) % 3], 0.7 + 0.01 * i) for i in range(24)]
    outs = [net.voxelize_batch(bank, ids, starts, T, scale=sc, return_indices=True)["indices"] for ids, starts, sc in calls]
    torch.cuda.synchronize()
    for (ids, starts, sc), idx in zip(calls, outs):
        for b in range(2):
            _same(_np(idx[b]), IR.clip(seqs[ids[b]][0], starts[b], T, 1, False, G, sc)["idx"], "indices")


def test_non_finite_coordinates_are_counted_like_numpy():
    """one NaN makes the clip's box NaN (np.amax), so every row of that clip is refused - and only that clip's; an infinite coordinate
    goes through the same arithmetic as numpy's"""
    G, N, T = 32, 257, 3
    seqs = [p for p, _ in _three_sequences("float32", N)]
    nan = seqs[0].copy(); nan[1, 100, 2] = np.nan
    inf = seqs[1].copy(); inf[2, 7, 0] = np.inf
    bank = ClipBank("cuda")
    for p in (nan, inf, seqs[2]):
        bank.add(p)
    net = _net(G)
    out = net.voxelize_batch(bank, [0, 1, 2], [0, 0, 0], T, return_indices=True)
    with np.errstate(all="ignore"):
        want = [IR.clip(p, 0, T, 1, False, G) for p in (nan, inf, seqs[2])]
    counts = [int(w["bad"].sum()) for w in want]
    assert counts[0] == T * N and counts[1] > 0 and counts[2] == 0
    assert _np(out["bad_rows"]).tolist() == counts
    for b in range(3):
        _same(_np(out["vox"][b]), want[b]["vox"], f"voxels of clip {b}")
        _same(_np(out["indices"][b]), want[b]["idx"], f"indices of clip {b} (0 where the quotient is not finite)")
    with pytest.raises(ValueError, match="Dataset voxelizer error"):
        net.voxelize_batch(bank, [2, 1], [0, 0], T, check=True)


def test_float64_zero_translation_equals_voxelize():
    """the single-clip call this one generalises: float64 input, no translation"""
    G, N, T = 40, 1000, 6
    x = IR.sequence(78, 0, T + 2, N, np.float64)
    bank = ClipBank("cuda")
    bank.add(x)
    net = _net(G)
    out = net.voxelize_batch(bank, [0], [1], T, scale=0.9, return_indices=True)
    vox, idx = net.voxelize(torch.from_numpy(x[1:1 + T]), scale=0.9, return_indices=True)
    assert torch.equal(out["vox"][0], vox) and torch.equal(out["indices"][0], idx)
    assert int(out["vox"].sum()) > 0


def test_trainer_step_on_a_loader_batch_equals_host_built_voxels():
    """DeviceClipLoader's batch goes into DetectorTrainer.step as it is, and the step returns the losses of the same step on voxels
    built on the host by the restatement, bit for bit"""
    from neural_marionette_amd.train import DetectorTrainer
    G, T = G18["G"], 3
    seqs = IR.g18_sequences()
    o = HotPathOptions(grid_size=G)
    sd = synth.make_state_dict(o, seed=5, variant="peaky")
    results = []
    for device_path in (True, False):
        net = NeuralMarionette(o)
        net.load_state_dict(sd)
        net = net.cuda().train()
        net.anneal(1)
        tr = DetectorTrainer(net, lr=4e-4)
        bank = _bank(seqs, joints=False)
        sampler = ClipSampler(bank.lengths, T, 2, True, random.Random(11))
        if device_path:
            loader = DeviceClipLoader(net, bank, sampler, batch=3)
            assert len(loader) == 1
            vox = next(iter(loader))
            assert vox.is_cuda and tuple(vox.shape) == (3, T, 1, G, G, G)
        else:
            crops = [sampler.crop(i) for i in range(3)]
            vox = torch.from_numpy(np.stack([IR.clip(seqs[s][0], st, T, 2, pad, G)["vox"] for s, st, pad in crops]))
        results.append((vox.cpu(), tr.step(vox)))
    assert torch.equal(results[0][0], results[1][0])
    assert results[0][1] == results[1][1], (results[0][1], results[1][1])
    assert np.isfinite(results[0][1]["loss"])
