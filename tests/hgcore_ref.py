"""Reference, cases and inputs of tests/test_hgcore_gpu.py: the two lowest hourglass levels (vox_modules.py:78-120, the part between
encoder_pool2 and decoder_upsample2) in plain torch, in any dtype, from the oracle's blocks.

    a2 -> encoder_res2 -> e2;  s3 = skip_res3(e2);  encoder_pool3 -> encoder_res3 -> decoder_res3
       -> decoder_upsample3(output_padding = D % 2) + s3 -> decoder_res2 -> out            32 -> 48 channels, D^3 voxels

tests/test_hgcore_ref_cpu.py splices `core` into a whole hourglass and gets oracle.nm_oracle.hourglass back bit for bit, and shows
that the float32 evaluation stays within 2e-6 of the float64 one on every case below: the sub-graph is well conditioned, so the 2e-5
bound of the GPU test is a statement about the kernels.

Weights: synth.make_state_dict(HotPathOptions(grid_size=32), seed=8) - float32 values; the float64 reference uses exactly those values.
Inputs (seeded per case): the pool conv's raw output `raw` (N,32,D,D,D) of scale ~3 around 1, and for the 'lazy' prologue its pending
GroupNorm as per-frame scale / shift (N,32) (scales of both signs around 1/3, so that LeakyReLU's two branches both occur) with slope
0.01; the activated tensor has unit scale.  Prologue 'none': `raw` is the activated tensor itself (unit normal), slope 1."""
import functools

import torch
import torch.nn.functional as F

from neural_marionette_amd import HotPathOptions, synth
from oracle import nm_oracle as O

CIN, COUT = 32, 48
NETS = (O.V2K + ".extract_features.4", O.V2K + ".extract_spatio_temporal_features.4")      # which = 0 / 1
SIZES = (2, 3, 4, 5, 6)              # D2 = grid_size // 16 of every grid the library accepts (32 .. 104)
PROLOGUES = ("lazy", "none")
CASES = [(D, which, pro) for D in SIZES for which in (0, 1) for pro in PROLOGUES]
N_PARITY = 3


@functools.lru_cache(maxsize=None)
def state_dict():
    """the full float32 state_dict the GPU context loads"""
    return synth.make_state_dict(HotPathOptions(grid_size=32), seed=8)


@functools.lru_cache(maxsize=None)
def weights(dtype):
    return {k: v.to(dtype) for k, v in state_dict().items() if k.startswith(NETS[0]) or k.startswith(NETS[1])}


def core(a2, sd, p):
    """encoder_res2 ... decoder_res2 on the ACTIVATED pool-2 output a2 (N,32,D,D,D); sd in a2's dtype, p = the hourglass's key prefix"""
    D = a2.shape[-1]
    e2 = O.res_block(a2, sd, p + ".encoder_res2")
    s3 = O.res_block(e2, sd, p + ".skip_res3")
    x = O.res_block(O.pool_block(e2, sd, p + ".encoder_pool3"), sd, p + ".encoder_res3")
    x = O.res_block(x, sd, p + ".decoder_res3")
    x = O.up_block(x, sd, p + ".decoder_upsample3", D % 2) + s3
    return O.res_block(x, sd, p + ".decoder_res2")


def inputs(D, which, pro, N=N_PARITY):
    """float32 cpu tensors: raw (N,32,D,D,D), scale / shift (N,32) or None, slope"""
    g = torch.Generator().manual_seed(7000 + 100 * D + 10 * which + PROLOGUES.index(pro))
    if pro == "none":
        return dict(raw=torch.randn(N, CIN, D, D, D, generator=g), scale=None, shift=None, slope=1.0)
    raw = 1.0 + 3.0 * torch.randn(N, CIN, D, D, D, generator=g)
    sign = torch.where(torch.rand(N, CIN, generator=g) < 0.25, -1.0, 1.0)
    scale = sign * (1.0 + 0.2 * torch.randn(N, CIN, generator=g)) / 3.0
    shift = 0.3 * torch.randn(N, CIN, generator=g)
    return dict(raw=raw, scale=scale, shift=shift, slope=O.LRELU)


def activated(inp, dtype):
    x = inp["raw"].to(dtype)
    if inp["scale"] is not None:
        x = x * inp["scale"].to(dtype)[:, :, None, None, None] + inp["shift"].to(dtype)[:, :, None, None, None]
    return x if inp["slope"] == 1.0 else F.leaky_relu(x, inp["slope"])


def ref(inp, which, dtype):
    with torch.no_grad():
        return core(activated(inp, dtype), weights(dtype), NETS[which])


@functools.lru_cache(maxsize=None)
def ref_case(case, dtype):
    """the reference of a case of CASES, computed once per process (callers must not modify it)"""
    return ref(inputs(*case), case[1], dtype)


def relerr(a, r):
    return (a.double() - r.double()).abs().max().item() / max(r.abs().max().item(), 1e-300)


def to_cl(x):
    """(N,C,D,D,D) -> channels-last (N,D,D,D,C), contiguous"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def from_cl(y):
    """(N,D,D,D,C) -> (N,C,D,D,D)"""
    return y.permute(0, 4, 1, 2, 3).contiguous()
