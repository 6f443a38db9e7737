"""The fp64 VRNN reference (tests/vrnn_ref.py) on the CPU: it really computes in float64, agrees with the fp32 oracle at small
shapes, leaves the default dtype alone, and every seeded input the GPU tests (tests/test_vrnn_batch_paths_gpu.py) depend on has
best-of-S selections with a clear winner - so that a discrete disagreement there is a kernel fault, not rounding."""
import numpy as np
import pytest
import torch

import vrnn_ref as V
from neural_marionette_amd import synth
from oracle import nm_oracle as O


def _small(K=24, B=3, T=4, S=5):
    o, sd, order, parents, aff = V.model(K, 77)
    return o, sd, order, parents, V.keypoints(B, T, K, 5), synth.make_eps((T, S, B, o.nlatent_kypt), seed=6)


def test_reference_outputs_are_float64():
    o, sd, order, parents, kp, eps = _small()
    r = V.encode(sd, o, kp, order, parents, eps)
    for k in ("kypt_recon", "R", "z_kypts", "h_kypts", "kl_kypt", "kypt_recon_loss", "sample_dist", "offset"):
        assert r[k].dtype == torch.float64, k
    B, K, H, Z = kp.shape[0], kp.shape[2], o.nhidden_kypt, o.nlatent_kypt
    x = torch.randn(B, H + Z)
    assert V.mlp(sd, x, "joint_matrix_decoder").dtype == torch.float64
    assert V.gru(sd, torch.randn(B, 4 * K + Z), torch.randn(B, H)).dtype == torch.float64
    f, R = V.fk(sd, x, r["offset"], order, parents)
    assert f.dtype == torch.float64 and R.dtype == torch.float64
    a = V.posterior_all(sd, torch.randn(B, H), kp[:, 0], eps[0], r["offset"], order, parents)
    assert all(v.dtype == torch.float64 for v in a.values())
    _, g = V.learner_grads(sd, o, kp, order, parents, eps)
    assert all(v.dtype == torch.float64 for v in g.values())


def test_reference_agrees_with_the_fp32_oracle_on_small_shapes():
    o, sd, order, parents, kp, eps = _small()
    r64 = V.encode(sd, o, kp, order, parents, eps)
    with torch.no_grad():
        r32 = O.vrnn_encode(sd, o, kp, order, parents, eps)          # the oracle itself, untouched
    assert r32["kypt_recon"].dtype == torch.float32
    assert V.encode_margins(r64).min().item() >= V.MARGIN_MIN
    assert torch.equal(r64["best_idx"], r32["best_idx"])
    for k in ("kypt_recon", "R", "z_kypts", "h_kypts"):
        e = V._err(r64[k], r32[k])
        assert e < 1e-5, (k, e)
    for k in ("kl_kypt", "kypt_recon_loss"):
        assert abs(float(r64[k]) - float(r32[k])) <= 1e-5 * max(1.0, abs(float(r64[k]))), k
    # the fp32 path of the helpers is the oracle's own arithmetic
    r32b = V.encode(sd, o, kp, order, parents, eps, dtype=torch.float32)
    for k in ("kypt_recon", "h_kypts"):
        assert torch.equal(r32b[k], r32[k]), k
    # teacher-forced steps: the fp32 oracle from the fp64 states, and the fp64 step reproduces its own encode exactly
    errs32 = V.teacher_forced(V.oracle_step(sd, r64, order, parents), r64, kp, eps)
    errs64 = V.teacher_forced(V.oracle_step(sd, r64, order, parents, torch.float64), r64, kp, eps)
    assert len(errs32) == kp.shape[1] and max(errs32) < 1e-5 and max(errs64) == 0.0
    # posterior_all at the selected samples is the oracle's step
    t = 1
    a = V.posterior_all(sd, r64["h_kypts"][:, t], kp[:, t], eps[t], r64["offset"], order, parents)
    ar = torch.arange(kp.shape[0])
    sel = a["d"].argmin(0)
    assert torch.equal(sel, r64["best_idx"][:, t])
    assert V._err(a["kp"][sel, ar], r64["kypt_recon"][:, t].reshape(kp.shape[0], -1)) == 0.0
    assert V._err(a["h"][sel, ar], r64["h_kypts"][:, t + 1]) == 0.0
    # gradients
    l64, g64 = V.learner_grads(sd, o, kp, order, parents, eps)
    l32, g32 = V.learner_grads(sd, o, kp, order, parents, eps, dtype=torch.float32)
    assert abs(l64 - l32) <= 1e-5 * abs(l64)
    for k, g in g64.items():
        assert V._err(g, g32[k]) <= 1e-3 * g.abs().max().item(), k


def test_default_dtype_is_restored():
    assert torch.get_default_dtype() == torch.float32
    o, sd, order, parents, kp, eps = _small(B=2, T=2, S=2)
    V.encode(sd, o, kp, order, parents, eps)
    assert torch.get_default_dtype() == torch.float32
    with pytest.raises(ZeroDivisionError):
        with V.float64():
            assert torch.get_default_dtype() == torch.float64
            1 / 0
    assert torch.get_default_dtype() == torch.float32


def test_selection_margins():
    d = torch.tensor([[4.0, 1.0], [2.0, 1.0], [3.0, 5.0]])
    m = V.selection_margins(d)
    assert torch.allclose(m, torch.tensor([0.5, 0.0], dtype=torch.float64))
    assert torch.isinf(V.selection_margins(d[:1])).all()


@pytest.mark.parametrize("case", list(V.ENCODE_CASES))
def test_encode_seeds_of_the_gpu_tests_have_clear_selections(case):
    o, sd, order, parents, aff, kp, eps = V.encode_inputs(case)
    m = V.encode_margins(V.encode(sd, o, kp, order, parents, eps)).min().item()
    print("%s: smallest selection margin %.2e" % (case, m))
    assert m >= V.MARGIN_MIN


@pytest.mark.parametrize("case", list(V.LEARNER_CASES))
def test_learner_seeds_of_the_gpu_tests_have_clear_selections(case):
    o, sd, order, parents, aff, kp, eps = V.learner_inputs(case)
    m = V.encode_margins(V.encode(sd, o, kp, order, parents, eps)).min().item()
    print("%s: smallest selection margin %.2e" % (case, m))
    assert m >= V.MARGIN_MIN


@pytest.mark.parametrize("B", V.GEN_B)
def test_generate_seeds_of_the_gpu_tests_have_clear_selections(B):
    """the conditioning steps of generate are encode's posterior steps on the conditioning frames"""
    o, sd, order, parents, aff, kp, e_post, e_prior = V.generate_inputs(B)
    m = V.encode_margins(V.encode(sd, o, kp, order, parents, e_post)).min().item()
    print("B=%d: smallest selection margin %.2e" % (B, m))
    assert m >= V.MARGIN_MIN
    g = V.generate(sd, o, kp, order, parents, 20, 5, e_post, e_prior)
    assert g["keypoints_gen"].dtype == torch.float64 and np.isfinite(g["keypoints_gen"].numpy()).all()
