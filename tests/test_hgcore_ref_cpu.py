"""The reference of tests/test_hgcore_gpu.py without a GPU.

1. tests/hgcore_ref.py's `core` is the middle of the oracle's hourglass: spliced between the level-1 blocks and decoder_upsample2 it
   gives oracle.nm_oracle.hourglass again, bit for bit in float64, at hourglass inputs of 8, 10, 12, 16, 20 and 24 voxels per edge
   (level-2 extents 2, 2, 3, 4, 5, 6 - both parities of the transposed conv's output padding), for both feature nets.
2. Conditioning: on every case of the GPU test the float32 evaluation of the reference is within 2e-6 of the float64 one (relative to
   the largest |reference|; measured 3e-7 .. 8e-7) - even at D = 2 and 3, where the level-3 tensors are single voxels and a GroupNorm
   group sees 16 values.  The GPU bound of 2e-5 is therefore an order of magnitude above what fp32 arithmetic itself costs here."""
import pytest
import torch

import hgcore_ref as R
from oracle import nm_oracle as O


def _spliced_hourglass(x, sd, p, Ng):
    op2, op1 = (Ng // 2) % 2, Ng % 2
    s1 = O.res_block(x, sd, p + ".skip_res1")
    x = O.res_block(O.pool_block(x, sd, p + ".encoder_pool1"), sd, p + ".encoder_res1")
    s2 = O.res_block(x, sd, p + ".skip_res2")
    x = R.core(O.pool_block(x, sd, p + ".encoder_pool2"), sd, p)
    x = O.up_block(x, sd, p + ".decoder_upsample2", op2) + s2
    x = O.res_block(x, sd, p + ".decoder_res1")
    return O.up_block(x, sd, p + ".decoder_upsample1", op1) + s1


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("Ng", [8, 10, 12, 16, 20, 24])
def test_core_spliced_into_the_hourglass_is_the_oracle_bit_for_bit(Ng, which):
    sd, p = R.weights(torch.float64), R.NETS[which]
    ci = sd[p + ".skip_res1.res_branch.0.weight"].shape[1]
    x = torch.randn(1, ci, Ng, Ng, Ng, dtype=torch.float64, generator=torch.Generator().manual_seed(Ng + which))
    with torch.no_grad():
        want = O.hourglass(x, sd, p, Ng)
        got = _spliced_hourglass(x, sd, p, Ng)
    assert got.shape == want.shape == (1, ci, Ng, Ng, Ng)
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "D%d-net%d-%s" % c)
def test_float32_reference_is_within_2e6_of_float64(case):
    D = case[0]
    r64, r32 = R.ref_case(case, torch.float64), R.ref_case(case, torch.float32)
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and r64.shape == (R.N_PARITY, R.COUT, D, D, D)
    assert torch.isfinite(r64).all()
    e = R.relerr(r32, r64)
    print("D=%d net %d %s: fp32 vs fp64 %.2e, max |ref| %.2f" % (*case, e, r64.abs().max().item()))
    assert e < 2e-6, e


def test_inputs_are_what_the_cases_say():
    """unit-scale activated inputs, both LeakyReLU branches and both scale signs under the lazy prologue, layout helpers invert"""
    for case in R.CASES:
        inp = R.inputs(*case)
        a = R.activated(inp, torch.float64)
        assert 0.5 < a.std().item() < 1.5, (case, a.std().item())
        if case[2] == "lazy":
            pre = inp["raw"].double() * inp["scale"].double()[:, :, None, None, None] + inp["shift"].double()[:, :, None, None, None]
            assert (pre < 0).any() and (pre > 0).any() and (inp["scale"] < 0).any() and (inp["scale"] > 0).any()
            assert torch.equal(a[pre < 0], pre[pre < 0] * O.LRELU)
        else:
            assert inp["scale"] is None and inp["shift"] is None and inp["slope"] == 1.0 and torch.equal(a.float(), inp["raw"])
        assert torch.equal(R.from_cl(R.to_cl(inp["raw"])), inp["raw"]) and R.to_cl(inp["raw"]).shape[-1] == R.CIN
