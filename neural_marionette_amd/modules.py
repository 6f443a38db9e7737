"""Drop-in nn.Module shells over the nm355 C ABI.

The reference exposes no FFI; its boundary for this path is the nn.Module surface of
``NeuralMarionette`` / ``KyptDetector`` / ``HSVRNNBVH`` (model/neural_marionette.py:6-103,
model/kypt_detector.py:10-241, model/hsvrnn_bvh.py:10-286): attribute names, call
signatures, returned dict keys and ``state_dict`` keys.  These shells keep that surface
and route every computation to libnm355.so (HIP, gfx950).  There is no PyTorch or CPU
fallback: parameters must live on a HIP device, and a missing library raises.

Parameters are ordinary ``nn.Parameter`` objects stored under the reference's key names
(checkpoints load unchanged); the engine re-uploads / re-packs them into the library's
MFMA layouts whenever their version counters change (load_state_dict, optimizer step).

The module tree itself (holders.py) is built from subclasses of the torch layer types in the reference's
construction order, so a freshly constructed network carries torch's default initialisation and
``network.apply(weights_init)`` (train.py:262,268) acts on it exactly as on the reference; a seeded
construction gives a bit-identical ``state_dict``.

Under ``torch.enable_grad()`` with trainable parameters the 11 detector losses and the two VRNN losses are
differentiable w.r.t. the parameters (autograd bridges over nm_detector_backward / nm_vrnn_encode_backward);
every other returned tensor is detached, which is all the reference's training loss consumes.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from . import _lib, holders
from .skeleton import build_skeleton
from .subdivide import LoopPlan
from .spec import DETECTOR_LOSS_KEYS, FEAT_DIM, HotPathOptions, param_spec

Priority = namedtuple("Priority", ["values", "indices"])   # what torch.topk returns in the reference


CONV_MODES = {"fp32": 0, "0": 0, "exact": 0, "split16": 1, "1": 1, "f16": 3, "3": 3, "bf16": 4, "4": 4, "auto": 1}
NM_ERR_RANGE = -5
CONV_MODE_NAMES = ("split16", "fp32", "f16", "bf16", "auto")
MESH_RECORD_BYTES = 512 << 20   # render_mesh draws its frames in groups whose triangle records (144 bytes per frame and triangle) stay under this
SUBDIV_BYTES = 512 << 20        # subdivide and render_retarget work on groups of frames whose intermediate levels / fine meshes stay under this


class Engine:
    """One nm_ctx + weight synchronisation for a NeuralMarionette instance."""

    def __init__(self, opts: HotPathOptions, owner: nn.Module, prefix: str = ""):
        self.opts = opts
        self.owner = owner          # module whose state_dict (under ``prefix``) has the reference's keys
        # a stand-alone KyptDetector / HSVRNNBVH owns only its half of the 337 tensors ('kypt_detector.' /
        # 'dyna_module.'); the library context wants all of them, so the other half is uploaded as zeros and is
        # never reached (the stand-alone object has no method that calls the other half's entry points)
        self.prefix = prefix
        self.ctx: Optional[_lib.Context] = None
        self._stamp = None
        self._named = None
        # conv arithmetic: 1 = split-fp16 MFMA with fp32-equivalent accuracy (default), 0 = exact fp32 MFMA, 3 = fp16 products
        # with fp32 accumulation (reduced precision, for training)
        env_mode = os.environ.get("NM355_CONV_MODE")
        self.conv_mode = CONV_MODES.get((env_mode or "split16").lower(), 1)
        # 'auto': split16 with a synchronous range probe on the first conv-running call after every weight change; a call that
        # overflows the fp16 range is re-run on the exact fp32 path, which then stays selected until the weights change.  This is the
        # DEFAULT (round 5): a script that makes one plain call and reads its outputs must never see NaN where the reference's fp32
        # arithmetic stays finite; the cost is one device synchronisation per weight change, none in steady-state inference.
        # set_conv_mode('split16' | 'fp32' | 'f16' | 'bf16') (or NM355_CONV_MODE) selects a mode explicitly and switches the probe
        # off - bench.py and the trainers' steps run that way, covered by the deferred guard of include/nm355.h.
        self.auto = env_mode is None or env_mode.lower() == "auto"
        self.auto_explicit = env_mode is not None and env_mode.lower() == "auto"
        self._probe = True
        self._auto_fp32 = False
        self._wstamp = None          # identity + version of every weight tensor at the last upload (survives set_training / a new context)
        self.suppress_probe = False  # the trainers' steps (weights change every step): no synchronous probe unless 'auto' was asked for
        self.training_packs = False     # detector-mode training: set_weights also packs the data-gradient weights

    # -- plumbing ---------------------------------------------------------------------------
    def _device(self) -> torch.device:
        p = next(self.owner.parameters())
        if not p.is_cuda:
            raise _lib.NmError("NeuralMarionette parameters are on the CPU: call .cuda() first — the HIP library "
                               "is the only implementation of this path (no CPU fallback)")
        return p.device

    def ready(self) -> _lib.Context:
        dev = self._device()
        if self.ctx is None or self.ctx.device != dev:
            o = self.opts
            cfg = _lib.NmConfig(device=dev.index or 0, grid_size=o.grid_size, nkeypoints=o.nkeypoints,
                                nlatent=o.nlatent_kypt, nhidden=o.nhidden_kypt, nneighbor=o.nneighbor,
                                gaussian_sigma=o.gaussian_sigma, sep_sigma=o.sep_sigma,
                                vol_fit_chamfer={"none": 0, "chamfer": 1, "gaussian": 2}[o.vol_fit_type],
                                use_graph_traj=int(o.graph_traj_weight > 0))
            self.ctx = _lib.Context(cfg)
            if not o.fixed_sigma:                          # kypt_detector.py:258-260: one more state_dict entry, before the first nm_ctx_set_weights
                _lib.check(self.ctx.lib.nm_ctx_set_learnable_sigma(self.ctx.handle, 1), "set_learnable_sigma")
            if o.gaussian_cat_type != "none":              # kypt_detector.py:396-401
                _lib.check(self.ctx.lib.nm_ctx_set_gaussian_cat(self.ctx.handle, {"max": 1, "sum": 2}[o.gaussian_cat_type]), "set_gaussian_cat")
            if o.affinity_ver != 3:                        # (N, K, K) affinity parameters: before the first nm_ctx_set_weights
                _lib.check(self.ctx.lib.nm_ctx_set_affinity_ver(self.ctx.handle, int(o.affinity_ver)), "set_affinity_ver")
            if o.const_intensity == 2:                     # kypt_detector.py:344-345: heat-maps propagated frame to frame (same weights as 3)
                _lib.check(self.ctx.lib.nm_ctx_set_const_intensity(self.ctx.handle, 2), "set_const_intensity")
            flags = o.graph_loss_flags()
            if o.graph_loss_ver != 1 or flags:             # kypt_detector.py:112-143 ('none': before the first nm_ctx_set_weights)
                _lib.check(self.ctx.lib.nm_ctx_set_graph_loss(self.ctx.handle, int(o.graph_loss_ver), flags), "set_graph_loss")
            self._stamp = None
            self._named = None
        _lib.check(self.ctx.lib.nm_ctx_set_training(self.ctx.handle, int(self.training_packs)), "set_training")
        self.ctx.bind_stream()
        mode = 0 if (self.auto and self._auto_fp32) else self.conv_mode
        _lib.check(self.ctx.lib.nm_set_conv_mode(self.ctx.handle, mode), "set_conv_mode")
        self._sync_weights()
        return self.ctx

    def set_training(self, on: bool) -> None:
        """Detector-mode training needs the flipped / transposed weight packs: toggling forces a re-upload."""
        if on != self.training_packs:
            self.training_packs = on
            self._stamp = None
        if self.ctx is not None:
            _lib.check(self.ctx.lib.nm_ctx_set_training(self.ctx.handle, int(on)), "set_training")

    def _sync_weights(self) -> None:
        if self._named is None:
            own = [(self.prefix + k, t) for k, t in self.owner.state_dict(keep_vars=True).items()]   # Parameter objects persist
            have = {k for k, _ in own}
            dev = self.ctx.device
            self._named = own + [(k, torch.zeros(*shape, device=dev)) for k, shape in param_spec(self.opts) if k not in have]
        sd = self._named
        # (the conv mode and the training switch decide which derived tables set_weights builds: part of the stamp)
        wstamp = tuple((t.data_ptr(), t._version) for _, t in sd)
        if wstamp != self._wstamp:
            # (compared against its own record, not against _stamp: set_training() and a re-created context clear _stamp, and a weight
            #  change that coincided with such a toggle must still re-arm the probe and drop a stale fp32 fallback - ADVICE r4)
            self._wstamp = wstamp
            if self.auto:
                self._probe = True                      # new weights: the next conv-running call is range-probed again ...
                if self._auto_fp32:                     # ... starting over on the split path
                    self._auto_fp32 = False
                    _lib.check(self.ctx.lib.nm_set_conv_mode(self.ctx.handle, self.conv_mode), "set_conv_mode")
        stamp = (0 if (self.auto and self._auto_fp32) else self.conv_mode, self.training_packs) + wstamp
        if stamp == self._stamp:
            return
        names, keep = [], []
        arr = (_lib.NmNamedTensor * len(sd))()
        for i, (k, t) in enumerate(sd):
            d = t.detach()
            if d.dtype != torch.float32 or not d.is_contiguous():
                d = d.float().contiguous()
            keep.append(d)
            names.append(k.encode())
            arr[i].name = names[-1]
            arr[i].data = d.data_ptr()
            arr[i].numel = d.numel()
        _lib.check(self.ctx.lib.nm_ctx_set_weights(self.ctx.handle, arr, len(sd)), "set_weights")
        self._stamp = stamp

    def call(self, fn: str, *args) -> None:
        _lib.check(getattr(self.ctx.lib, fn)(self.ctx.handle, *args), fn)

    def call_conv(self, fn: str, *args) -> None:
        """A call that runs the conv stacks.  Every such call is covered by the library's deferred range guard (a call whose
        split-fp16 arithmetic overflowed makes a LATER call raise NmError, no host synchronisation).  In conv mode 'auto' the first
        one after a weight change is also probed synchronously: if it overflowed it is re-run here on the exact fp32 path (all of a
        call's outputs are rewritten), and fp32 stays selected until the weights change."""
        self.call(fn, *args)
        # training forwards (the autograd path with ANY torch optimizer, not only the trainers' steps) change the weights every step: a
        # synchronous probe per weight change would be one device synchronisation per step and, on overflow, a whole second forward -
        # they rely on the deferred guard like the trainers unless 'auto' was asked for explicitly (advisor finding, round 5)
        training_call = self.training_packs or fn.endswith("_train")
        if not (self.auto and self._probe) or ((self.suppress_probe or training_call) and not self.auto_explicit):
            return
        self._probe = False
        rc = self.ctx.lib.nm_ctx_check_nonfinite(self.ctx.handle)
        if rc == 0:
            return
        if rc != NM_ERR_RANGE or self._auto_fp32:
            _lib.check(rc, "check_nonfinite")
        self._auto_fp32 = True
        self.ready()                                # exact fp32 MFMA + the weight tables of that mode
        self.call(fn, *args)
        _lib.check(self.ctx.lib.nm_ctx_check_nonfinite(self.ctx.handle), fn + " (re-run in fp32)")


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


# ==========================================================================================
# detector
# ==========================================================================================
class _DetectorTrain(torch.autograd.Function):
    """KyptDetector.forward with a backward pass (detector mode, train.py:388-404): forward = nm_detector_forward_train
    (activations retained in the library), backward = nm_detector_backward (HIP kernels of nm_grad.hip /
    nm_heads_bwd.hip).  Only the 11 loss scalars carry gradients — exactly what the reference's training loss
    consumes; keypoints reach the learner detached (neural_marionette.py:53)."""

    @staticmethod
    def forward(ctx, module, vox, names, *params):
        eng = module._eng()
        eng.set_training(True)
        c = eng.ready()
        dev = c.device
        B, T = int(vox.shape[0]), int(vox.shape[1])
        G, K, g = module.grid_size, module.nkeypoints, module.grid_size // 4
        kp = torch.empty(B, T, K, 4, device=dev)
        hm = torch.empty(B, T, K, g, g, g, device=dev)
        ff = torch.empty(B, FEAT_DIM, g, g, g, device=dev)
        recon = torch.empty(B, T, 1, G, G, G, device=dev)
        aff = torch.empty(module.nneighbor, K, K, 1, device=dev) if module.affinity_start else torch.empty(0, device=dev)
        losses = torch.empty(len(DETECTOR_LOSS_KEYS), device=dev)
        eng.call_conv("nm_detector_forward_train", _lib.ptr(vox), B, T, int(module.affinity_start), _lib.ptr(kp), _lib.ptr(hm),
                 _lib.ptr(ff), _lib.ptr(recon), _lib.ptr(aff) if module.affinity_start else None, _lib.ptr(losses))
        ctx.module, ctx.names = module, names
        ctx.shapes = [p.shape for p in params]
        ctx.keep = (vox, kp, recon, aff)      # the library reads them again in the backward pass (the tape holds raw pointers)
        ctx.mark_non_differentiable(kp, hm, ff, recon, aff)
        return losses, kp, hm, ff, recon, aff

    @staticmethod
    def backward(ctx, dlosses, *unused):
        eng = ctx.module._eng()
        c = eng.ready()
        dev = c.device
        dl = (dlosses if dlosses is not None else torch.zeros(len(DETECTOR_LOSS_KEYS), device=dev)).float().contiguous()
        grads = [torch.empty(shp, device=dev) for shp in ctx.shapes]
        arr = (_lib.NmNamedTensor * len(grads))()
        keep = []
        for i, (n, g) in enumerate(zip(ctx.names, grads)):
            keep.append(n.encode())
            arr[i].name, arr[i].data, arr[i].numel = keep[-1], g.data_ptr(), g.numel()
        eng.call("nm_detector_backward", _lib.ptr(dl), arr, len(grads))
        ctx.keep = None
        return (None, None, None, *grads)


class KyptDetector(nn.Module):
    """model/kypt_detector.py:10-241.  Stand-alone construction (``KyptDetector(opt)``) gets its own library context."""

    def __init__(self, options, _engine: Optional[Engine] = None):
        super().__init__()
        o = HotPathOptions.from_any(options)
        o.check_fast_path()
        self._o = o
        self.vol_fit_type = o.vol_fit_type
        self.fixed_sigma = bool(o.fixed_sigma)
        self.keypoints_graph = o.keypoints_graph
        self.keypoints_detach = bool(o.keypoints_detach)
        self.affinity_ver = o.affinity_ver
        self.graph_loss_ver = o.graph_loss_ver
        self.gaussian_sigma = o.gaussian_sigma
        self.input_dim = o.input_dim
        self.grid_size = o.grid_size
        self.nkeypoints = o.nkeypoints
        self.nneighbor = o.nneighbor
        self.sigmas = [o.gaussian_sigma] * o.nkeypoints
        self.sep_sigma = o.sep_sigma
        self.affinity_anneal = o.affinity_anneal
        self.affinity_start = False
        # same creation order as kypt_detector.py:44-68 (the RNG stream of a seeded construction matches)
        self.vox_to_kypt = holders.VoxToKyptNet(grid_size=o.grid_size, nkeypoints=o.nkeypoints, input_dim=o.input_dim,
                                                sigmas=self.sigmas, fixed_sigma=bool(o.fixed_sigma),
                                                const_intensity=o.const_intensity)
        self.kypt_to_vox = holders.KyptToVoxNet(grid_size=o.grid_size, nkeypoints=o.nkeypoints, input_dim=o.input_dim,
                                                gaussian_cat_type=o.gaussian_cat_type)
        K, N = o.nkeypoints, o.nneighbor
        if o.keypoints_graph == "none":                        # kypt_detector.py:54: no affinity parameters, no draws from the RNG
            pass
        elif o.affinity_ver < 3:                               # kypt_detector.py:57-58,65-66
            self.affinity_params = nn.Parameter(torch.randn(N, K, K) if o.graph_random_init else torch.zeros(N, K, K))
        else:
            self.affinity_params = nn.Parameter(torch.randn(N, K, K - 1) if o.graph_random_init else torch.ones(N, K, K - 1))
        object.__setattr__(self, "_engine", _engine if _engine is not None else Engine(o, self, prefix="kypt_detector."))

    def _eng(self) -> Engine:
        return self._engine

    def anneal(self, nepoch):
        """kypt_detector.py:71-78 (nothing under keypoints_graph 'none')."""
        if self.keypoints_graph == "none":
            return
        if self.affinity_anneal > nepoch:
            self.affinity_params.requires_grad = False
        elif not self.affinity_start:
            self.affinity_start = True
            self.affinity_params.requires_grad = True

    def forward(self, seq, Tcond=None):
        """KyptDetector.forward (kypt_detector.py:81-169) -> the same dict of 16 entries."""
        eng = self._eng()
        ctx = eng.ready()
        dev = ctx.device
        B, T = int(seq.shape[0]), int(seq.shape[1])
        G, K, g = self.grid_size, self.nkeypoints, self.grid_size // 4
        if tuple(seq.shape[2:]) != (1, G, G, G):
            raise ValueError(f"expected seq of shape (B,T,1,{G},{G},{G}), got {tuple(seq.shape)}")
        vox = _f32(seq, dev)
        named = [(k, p) for k, p in self.named_parameters()]
        if torch.is_grad_enabled() and any(p.requires_grad for _, p in named):
            # detector-mode training (train.py:388): the 11 losses are differentiable w.r.t. every kypt_detector parameter
            names = ["kypt_detector." + k for k, _ in named]
            losses, kp, hm, ff, recon, aff = _DetectorTrain.apply(self, vox, names, *[p for _, p in named])
            aff = aff if self.affinity_start else None
        else:
            kp = torch.empty(B, T, K, 4, device=dev)
            hm = torch.empty(B, T, K, g, g, g, device=dev)
            ff = torch.empty(B, FEAT_DIM, g, g, g, device=dev)
            recon = torch.empty(B, T, 1, G, G, G, device=dev)
            aff = torch.empty(self.nneighbor, K, K, 1, device=dev) if self.affinity_start else None
            losses = torch.empty(len(DETECTOR_LOSS_KEYS), device=dev)
            eng.call_conv("nm_detector_forward", _lib.ptr(vox), B, T, int(self.affinity_start), _lib.ptr(kp), _lib.ptr(hm),
                     _lib.ptr(ff), _lib.ptr(recon), _lib.ptr(aff), _lib.ptr(losses))
        out = dict(recon=recon, keypoints=kp, heatmaps=hm, affinity=aff)
        for i, name in enumerate(DETECTOR_LOSS_KEYS):
            out[name] = losses[i]
        out["first_feature"] = ff
        return out

    def detect(self, seq):
        """Keypoints only: VoxToKyptNet + the affinity (kypt_detector.py:299-364, :171-211) without the voxel decoder and the losses -
        what the learner regime reads from the frozen detector (neural_marionette.py:45-47).  No gradients.  The tensors returned are
        bit-identical to the same entries of forward()."""
        eng = self._eng()
        ctx = eng.ready()
        dev = ctx.device
        B, T = int(seq.shape[0]), int(seq.shape[1])
        G, K, g = self.grid_size, self.nkeypoints, self.grid_size // 4
        if tuple(seq.shape[2:]) != (1, G, G, G):
            raise ValueError(f"expected seq of shape (B,T,1,{G},{G},{G}), got {tuple(seq.shape)}")
        vox = _f32(seq, dev)
        kp = torch.empty(B, T, K, 4, device=dev)
        hm = torch.empty(B, T, K, g, g, g, device=dev)
        ff = torch.empty(B, FEAT_DIM, g, g, g, device=dev)
        aff = torch.empty(self.nneighbor, K, K, 1, device=dev) if self.affinity_start else None
        eng.call_conv("nm_detector_keypoints", _lib.ptr(vox), B, T, int(self.affinity_start), _lib.ptr(kp), _lib.ptr(hm), _lib.ptr(ff), _lib.ptr(aff))
        return dict(keypoints=kp, heatmaps=hm, affinity=aff, first_feature=ff)

    def get_affinity(self):
        """kypt_detector.py:171-211 (ver 3) -> (N,K,K,1)."""
        if self.keypoints_graph == "none":
            raise _lib.NmError("KyptDetector.get_affinity: keypoints_graph 'none' has no affinity")
        eng = self._eng()
        ctx = eng.ready()
        aff = torch.empty(self.nneighbor, self.nkeypoints, self.nkeypoints, 1, device=ctx.device)
        eng.call("nm_get_affinity", _lib.ptr(aff))
        return aff

    def decode_from_dyna(self, keypoints, first_feature, first_frame):
        """kypt_detector.py:213-241 -> {'gen': (B,Tgen,1,G,G,G)}."""
        eng = self._eng()
        ctx = eng.ready()
        dev = ctx.device
        B, Tg = int(keypoints.shape[0]), int(keypoints.shape[1])
        G = self.grid_size
        gen = torch.empty(B, Tg, 1, G, G, G, device=dev)
        kp, ff, fr = _f32(keypoints, dev), _f32(first_feature, dev), _f32(first_frame, dev)
        eng.call_conv("nm_decode_from_keypoints", _lib.ptr(kp), _lib.ptr(ff), _lib.ptr(fr), B, Tg, _lib.ptr(gen))
        return dict(gen=gen)


def _need_graph(o: HotPathOptions, what: str) -> None:
    """The learner builds its skeleton from the detector's affinity (neural_marionette.py:53 calls affinity.detach()): under
    keypoints_graph 'none' there is none, and the reference cannot run this path either."""
    if o.keypoints_graph == "none":
        raise _lib.NmError(f"{what}: keypoints_graph 'none' has no affinity, and the learner needs one to build its skeleton "
                           "(the reference fails here as well, neural_marionette.py:53); only the detector runs under 'none'")


# ==========================================================================================
# VRNN
# ==========================================================================================
class _Mlp(nn.Sequential):
    """nn.Sequential(Linear, LeakyReLU, Linear[, Tanh]) of hsvrnn_bvh.py:29-54: parameters under '0' / '2', callable
    like the reference's (vis_generation.py:97-127 calls the four MLPs directly) — through nm_vrnn_mlp."""

    def __init__(self, which: int, nin: int, nout: int, owner: "HSVRNNBVH"):
        super().__init__(*holders.vrnn_mlp_layers(nin, nout, tanh=(which == 2)))
        self._which, self._nout = which, nout
        object.__setattr__(self, "_owner", owner)

    def forward(self, x):
        eng = self._owner._eng()
        ctx = eng.ready()
        xx = _f32(x, ctx.device)
        lead = xx.shape[:-1]
        xx = xx.reshape(-1, xx.shape[-1])
        y = torch.empty(xx.shape[0], self._nout, device=ctx.device)
        eng.call("nm_vrnn_mlp", self._which, _lib.ptr(xx), int(xx.shape[0]), _lib.ptr(y))
        return y.reshape(*lead, self._nout)


class GRUCell(nn.GRUCell):
    """nn.GRUCell of hsvrnn_bvh.py:57 (torch's parameters and default init), computed by nm_vrnn_gru."""

    def __init__(self, input_size: int, hidden_size: int, owner: "HSVRNNBVH"):
        super().__init__(input_size, hidden_size)
        object.__setattr__(self, "_owner", owner)

    def forward(self, x, h):
        eng = self._owner._eng()
        ctx = eng.ready()
        xx, hh = _f32(x, ctx.device), _f32(h, ctx.device)
        out = torch.empty_like(hh)
        eng.call("nm_vrnn_gru", _lib.ptr(xx), _lib.ptr(hh), int(xx.shape[0]), _lib.ptr(out))
        return out


class _EncodeTrain(torch.autograd.Function):
    """HSVRNNBVH.encode with a backward pass (learner mode): forward = nm_vrnn_encode_train, backward =
    nm_vrnn_encode_backward (BPTT kernels in nm_vrnn.hip).  Only the two scalar losses carry gradients, exactly
    what the reference's training loss consumes (train.py:389-398)."""

    @staticmethod
    def forward(ctx, module, kp, eps, S, names, *params):
        eng = module._eng()
        c = eng.ready()
        dev = c.device
        B, T, K, _ = kp.shape
        Z, H = module.nlatent_kypt, module.nhidden_kypt
        rec = torch.empty(B, T, K, 4, device=dev); R = torch.empty(B, T, K, 3, 3, device=dev)
        z = torch.empty(B, T, Z, device=dev); h = torch.empty(B, T + 1, H, device=dev)
        sc = torch.empty(2, device=dev); best = torch.empty(B, T, device=dev, dtype=torch.int32)
        eng.call("nm_vrnn_encode_train", _lib.ptr(kp), _lib.ptr(eps), B, T, S, _lib.ptr(rec), _lib.ptr(R), _lib.ptr(z),
                 _lib.ptr(h), _lib.ptr(sc), _lib.ptr(best))
        ctx.module, ctx.names = module, names
        ctx.shapes = [p.shape for p in params]
        ctx.mark_non_differentiable(rec, R, z, h, best)
        return sc[0].clone(), sc[1].clone(), rec, R, z, h, best

    @staticmethod
    def backward(ctx, dkl, drec, *unused):
        eng = ctx.module._eng()
        c = eng.ready()
        dev = c.device
        zero = torch.zeros((), device=dev)
        dscal = torch.stack([(dkl if dkl is not None else zero).float().reshape(()),
                             (drec if drec is not None else zero).float().reshape(())]).contiguous()
        grads = [torch.empty(shp, device=dev) for shp in ctx.shapes]
        arr = (_lib.NmNamedTensor * len(grads))()
        keep = []
        for i, (n, g) in enumerate(zip(ctx.names, grads)):
            keep.append(n.encode())
            arr[i].name, arr[i].data, arr[i].numel = keep[-1], g.data_ptr(), g.numel()
        eng.call("nm_vrnn_encode_backward", _lib.ptr(dscal), arr, len(grads))
        return (None, None, None, None, None, *grads)


class HSVRNNBVH(nn.Module):
    """model/hsvrnn_bvh.py:10-286.  Stand-alone construction (``HSVRNNBVH(opt)``) gets its own library context."""

    def __init__(self, options, _engine: Optional[Engine] = None):
        super().__init__()
        o = HotPathOptions.from_any(options)
        o.check_fast_path()
        self._o = o
        self.nkeypoints = o.nkeypoints
        self.nlatent_kypt = o.nlatent_kypt
        self.nhidden_kypt = o.nhidden_kypt
        self.input_dim = o.input_dim
        self.transition_type = o.transition_type
        self.state_mode = o.state_mode
        self.action_mode = o.action_mode
        K, Z, H = o.nkeypoints, o.nlatent_kypt, o.nhidden_kypt
        state_dim = K * (o.input_dim + 1)
        # same creation order as hsvrnn_bvh.py:29-65 (the RNG stream of a seeded construction matches)
        self.extract_post_dist = _Mlp(0, H + state_dim, 2 * Z, self)
        self.extract_prior_dist = _Mlp(1, H, 2 * Z, self)
        self.root_intensity_decoder = _Mlp(2, H + Z, 3 + K, self)
        self.joint_matrix_decoder = _Mlp(3, H + Z, 6 * K, self)
        self.kypt_rnn_cell = GRUCell(state_dim + Z, H, self)
        self.init_kypt_rnn_state = nn.Parameter(torch.randn(1, H))
        self.A, self.priority, self.parents = None, None, None
        self.offset_param = nn.Parameter(torch.randn(K, 3))
        self.offset_param.requires_grad = False
        object.__setattr__(self, "_engine", _engine if _engine is not None else Engine(o, self, prefix="dyna_module."))
        object.__setattr__(self, "_tree_key", None)

    def _eng(self) -> Engine:
        return self._engine

    # -- skeleton ---------------------------------------------------------------------------
    def _ensure_tree(self, affinity, ctx) -> None:
        """First encode() builds and caches the tree (hsvrnn_bvh.py:75-79); later calls reuse it."""
        if self.A is None:
            if affinity is None:
                raise _lib.NmError("the skeleton has not been built yet: call encode() (or pass an affinity) first")
            sk = build_skeleton(affinity.detach().float().cpu().numpy())
            dev = ctx.device
            self.A = torch.from_numpy(sk.A).float().to(dev)
            self.priority = Priority(values=torch.from_numpy(sk.dist).to(dev), indices=torch.from_numpy(sk.order).to(dev))
            self.parents = torch.from_numpy(sk.parents).to(dev)
        key = (self.parents.data_ptr(), self.priority.indices.data_ptr(), id(ctx))
        if key != self._tree_key:
            par = self.parents.detach().cpu().numpy().astype(np.int32)
            order = self.priority.indices.detach().cpu().numpy().astype(np.int32)
            self._eng().call("nm_vrnn_set_tree", par.ctypes.data_as(_lib.c_int32_p), order.ctypes.data_as(_lib.c_int32_p))
            object.__setattr__(self, "_tree_key", key)

    def set_tree(self, parents, order, A=None) -> None:
        """Install a skeleton directly instead of deriving it from an affinity in the first encode(): parents (K) with
        parents[root] == root, order (K) = the joints in kinematic order, root first (what ``priority.indices`` holds); A (K,K) is kept
        as given (default: the tree's adjacency).  The library checks that every joint's parent precedes it.  ``priority.values`` is
        then only a placeholder (0 .. K-1 in kinematic order): the distances the reference's topk returns exist only for a tree derived
        from an affinity, and nothing in the library reads them."""
        ctx = self._eng().ready()
        dev, K = ctx.device, self.nkeypoints
        par = torch.as_tensor(np.asarray(parents).astype(np.int64))
        ordr = torch.as_tensor(np.asarray(order).astype(np.int64))
        if tuple(par.shape) != (K,) or tuple(ordr.shape) != (K,):
            raise ValueError(f"parents and order must be ({K},), got {tuple(par.shape)} and {tuple(ordr.shape)}")
        if A is None:
            A = torch.zeros(K, K)
            k = torch.arange(K)
            A[k, par] = 1
            A[par, k] = 1
            A[k, k] = 0
        self.A = torch.as_tensor(A).float().to(dev)
        self.priority = Priority(values=torch.arange(K, dtype=torch.float64, device=dev), indices=ordr.to(dev))
        self.parents = par.to(dev)
        object.__setattr__(self, "_tree_key", None)
        self._ensure_tree(None, ctx)

    def _eps(self, n, shape, dev, eps):
        if eps is not None:
            # the library reads n * prod(shape) floats: a smaller tensor (e.g. S samples of noise for SAMPLE_NUM > S) is an
            # out-of-bounds read on the device, so the shape is checked here
            if tuple(eps.shape) != (n, *shape):
                raise ValueError(f"eps must be {(n, *shape)}, got {tuple(eps.shape)}")
            return _f32(eps, dev)
        # the reference draws one rsample per step from the device generator (hsvrnn_bvh.py:107,216)
        return torch.stack([torch.randn(*shape, device=dev) for _ in range(n)], dim=0) if n else torch.empty(0, *shape, device=dev)

    # -- public surface -----------------------------------------------------------------------
    def encode(self, keypoints, affinity, SAMPLE_NUM=10, eps=None):
        """hsvrnn_bvh.py:67-156.  ``eps`` (T,S,B,Z) injects the standard-normal draws."""
        _need_graph(self._o, "HSVRNNBVH.encode")
        eng = self._eng()
        ctx = eng.ready()
        dev = ctx.device
        self._ensure_tree(affinity, ctx)
        B, T, K, _ = keypoints.shape
        Z, H, S = self.nlatent_kypt, self.nhidden_kypt, int(SAMPLE_NUM)
        kp = _f32(keypoints, dev)
        e = self._eps(T, (S, B, Z), dev, eps)
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        if torch.is_grad_enabled() and named:
            names = ["dyna_module." + n for n, _ in named]
            kl, rl, rec, R, z, h, best = _EncodeTrain.apply(self, kp, e, S, names, *[p for _, p in named])
            return dict(kypt_recon=rec, R=R, z_kypts=z, h_kypts=h, kl_kypt=kl, kypt_recon_loss=rl,
                        gae_recon_loss=torch.zeros((), dtype=torch.int64, device=dev), topo_recon_loss=torch.zeros((), dtype=torch.int64, device=dev), best_idx=best)
        rec = torch.empty(B, T, K, 4, device=dev)
        R = torch.empty(B, T, K, 3, 3, device=dev)
        z = torch.empty(B, T, Z, device=dev)
        h = torch.empty(B, T + 1, H, device=dev)
        sc = torch.empty(2, device=dev)
        best = torch.empty(B, T, device=dev, dtype=torch.int32)
        eng.call("nm_vrnn_encode", _lib.ptr(kp), _lib.ptr(e), B, T, S, _lib.ptr(rec), _lib.ptr(R), _lib.ptr(z),
                 _lib.ptr(h), _lib.ptr(sc), _lib.ptr(best))
        return dict(kypt_recon=rec, R=R, z_kypts=z, h_kypts=h, kl_kypt=sc[0], kypt_recon_loss=sc[1],
                    gae_recon_loss=torch.zeros((), dtype=torch.int64, device=dev), topo_recon_loss=torch.zeros((), dtype=torch.int64, device=dev),
                    best_idx=best)

    def generate(self, keypoints_cond, affinity=None, Ttot=10, Tcond=3, SAMPLE_NUM=10, eps_post=None, eps_prior=None):
        """hsvrnn_bvh.py:158-234."""
        _need_graph(self._o, "HSVRNNBVH.generate")
        eng = self._eng()
        ctx = eng.ready()
        dev = ctx.device
        self._ensure_tree(affinity, ctx)
        B, Tc_in, K, _ = keypoints_cond.shape
        Z, S = self.nlatent_kypt, int(SAMPLE_NUM)
        if Tc_in != Tcond:
            raise ValueError("keypoints_cond must hold exactly Tcond frames ('dl' transition)")
        kp = _f32(keypoints_cond, dev)
        e_post = self._eps(Tcond, (S, B, Z), dev, eps_post)
        e_prior = self._eps(Ttot - Tcond, (B, Z), dev, eps_prior)
        cond = torch.empty(B, Tcond, K, 4, device=dev)
        gen = torch.empty(B, Ttot - Tcond, K, 4, device=dev)
        eng.call("nm_vrnn_generate", _lib.ptr(kp), _lib.ptr(e_post), _lib.ptr(e_prior) if Ttot > Tcond else None,
                 B, Tcond, Ttot, S, _lib.ptr(cond), _lib.ptr(gen) if Ttot > Tcond else None, None)
        return dict(keypoints_cond=cond, keypoints_gen=gen)

    def get_offset(self, keypoints):
        """hsvrnn_bvh.py:236-253 -> (B,K,3,1), detached."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        B, T, K, _ = keypoints.shape
        kp = _f32(keypoints, ctx.device)
        off = torch.empty(B, K, 3, device=ctx.device)
        eng.call("nm_vrnn_offsets", _lib.ptr(kp), B, T, _lib.ptr(off))
        return off[..., None]

    def extract_kypt_from_latent_and_state(self, decoder_input, offset):
        """hsvrnn_bvh.py:255-286: (B,H+Z), (B,K,3,1) -> (B,K*4), (B,K,3,3)."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        x = _f32(decoder_input, ctx.device)
        off = _f32(offset.reshape(offset.shape[0], self.nkeypoints, 3), ctx.device)
        B = int(x.shape[0])
        kp = torch.empty(B, self.nkeypoints * 4, device=ctx.device)
        R = torch.empty(B, self.nkeypoints, 3, 3, device=ctx.device)
        eng.call("nm_vrnn_fk", _lib.ptr(x), _lib.ptr(off), B, _lib.ptr(kp), _lib.ptr(R))
        return kp, R

    def step(self, h, offset, eps, keypoints_obs=None, SAMPLE_NUM=10, update_state=True):
        """One fused VRNN step for hand-rolled rollouts (vis_generation.py:97-127 of the reference does the
        same with five sub-module calls): posterior best-of-S when ``keypoints_obs`` is given, else prior.
        Returns (keypoints_flat (B,K*4), z (B,Z), h_next (B,H) or None when ``update_state`` is False)."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        dev = ctx.device
        hh = _f32(h, dev)
        B = int(hh.shape[0])
        off = _f32(offset.reshape(B, self.nkeypoints, 3), dev)
        want = (B, self.nlatent_kypt) if keypoints_obs is None else (int(SAMPLE_NUM), B, self.nlatent_kypt)
        if tuple(eps.shape) != want:
            raise ValueError(f"eps must be {want}, got {tuple(eps.shape)}")
        e = _f32(eps, dev)
        obs = None if keypoints_obs is None else _f32(keypoints_obs.reshape(B, -1), dev)
        kp = torch.empty(B, self.nkeypoints * 4, device=dev)
        z = torch.empty(B, self.nlatent_kypt, device=dev)
        hn = torch.empty_like(hh) if update_state else None
        eng.call("nm_vrnn_step", int(obs is not None), _lib.ptr(hh), _lib.ptr(obs), _lib.ptr(off), _lib.ptr(e), B,
                 int(SAMPLE_NUM), _lib.ptr(kp), _lib.ptr(z), _lib.ptr(hn))
        return kp, z, hn

    def rollout(self, h, offset, eps):
        """The prior loop of vis_generation.py:117-127 in one library call (nm_vrnn_rollout: a captured HIP graph of three
        launches per step for small batches): h (B,H), offset (B,K,3,1), eps (T,B,Z) -> keypoints (B,T,K,4), h_T (B,H)."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        dev = ctx.device
        hh = _f32(h, dev)
        B, K = int(hh.shape[0]), self.nkeypoints
        off = _f32(offset.reshape(B, K, 3), dev)
        e = _f32(eps, dev)
        T = int(e.shape[0])
        if tuple(e.shape) != (T, B, self.nlatent_kypt):
            raise ValueError(f"eps must be (T,{B},{self.nlatent_kypt}), got {tuple(e.shape)}")
        kp = torch.empty(B, T, K, 4, device=dev)
        hn = torch.empty_like(hh)
        eng.call("nm_vrnn_rollout", _lib.ptr(hh), _lib.ptr(off), _lib.ptr(e), B, T, _lib.ptr(kp), _lib.ptr(hn))
        return kp, hn

    def nearest_row(self, rows, target):
        """Index (python int) of the row of ``rows`` (B,D) nearest to ``target`` ((D,) or (B,D)) in squared L2 —
        the sample selection of the reference's demo loops (vis_generation.py:109-110)."""
        eng = self._eng()
        ctx = eng.ready()
        r = _f32(rows.reshape(rows.shape[0], -1), ctx.device)
        t = _f32(target.reshape(-1, r.shape[1]), ctx.device)
        idx = torch.empty(1, device=ctx.device, dtype=torch.int32)
        eng.call("nm_rows_argmin_dist", _lib.ptr(r), _lib.ptr(t), 0 if t.shape[0] == 1 else int(r.shape[1]),
                 int(r.shape[0]), int(r.shape[1]), _lib.ptr(idx), None)
        return int(idx.item())

    # -- motion retargeting (vis_retarget.py of the reference; nm_retarget.hip) ---------------------------------------------
    def skin_weights(self, points, keypoints, R_bind=None, hardness=8.0, threshold=0.2, force_child=None):
        """extract_skin_weights (vis_retarget.py:21-62) and the local coordinates of :268-270, one pass over the points on the device.
        points (N,3) [float64 arithmetic, as the reference's numpy points], keypoints (K,4), R_bind (K,3,3) or None (identity: the local
        coordinates are plain offsets).  ``force_child`` (N) imposes the nearest-bone selection (``margin`` stays the free one).
        Returns child (N) int32, parent (N) int32, w (N,2) [child joint, parent joint], local (N,2,3) float64, margin (N) float64
        [second-smallest minus smallest bone distance] and dense (N,K) = what the reference's function returns.  Needs the tree."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        dev, K = ctx.device, self.nkeypoints
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
            raise ValueError(f"points must be (N,3) with N >= 1, got {tuple(points.shape)}")
        if tuple(keypoints.shape) != (K, 4):
            raise ValueError(f"keypoints must be ({K},4), got {tuple(keypoints.shape)}")
        if R_bind is not None and tuple(R_bind.shape) != (K, 3, 3):
            raise ValueError(f"R_bind must be ({K},3,3), got {tuple(R_bind.shape)}")
        N = int(points.shape[0])
        force = None
        if force_child is not None:
            if tuple(force_child.shape) != (N,):
                raise ValueError(f"force_child must be ({N},), got {tuple(force_child.shape)}")
            force = force_child.detach().to(device=dev, dtype=torch.int32).contiguous()
            if int(force.min()) < 0 or int(force.max()) >= K:
                raise ValueError(f"force_child must hold joint indices in [0,{K})")
        pts = points.detach().to(device=dev, dtype=torch.float64).contiguous()
        kp = _f32(keypoints, dev)
        rb = None if R_bind is None else _f32(R_bind, dev)
        child = torch.empty(N, device=dev, dtype=torch.int32)
        parent = torch.empty(N, device=dev, dtype=torch.int32)
        w = torch.empty(N, 2, device=dev)
        local = torch.empty(N, 2, 3, device=dev, dtype=torch.float64)
        margin = torch.empty(N, device=dev, dtype=torch.float64)
        dense = torch.empty(N, K, device=dev)
        eng.call("nm_retarget_bind", _lib.ptr(pts), N, _lib.ptr(kp), _lib.ptr(rb), K, float(hardness), float(threshold), _lib.ptr(force),
                 _lib.ptr(child), _lib.ptr(parent), _lib.ptr(w), _lib.ptr(local), _lib.ptr(margin), _lib.ptr(dense))
        return dict(child=child, parent=parent, w=w, local=local, margin=margin, dense=dense)

    def retarget_fk(self, R, root_pos, offset):
        """The re-posing loop of vis_retarget.py:275-300: R (T,K,3,3), root_pos (T,3), offset (K,3[,1]) -> joint positions (T,K,3), forward
        kinematics along the tree in fp32, clipped to [-1,1]."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        dev, K = ctx.device, self.nkeypoints
        T = int(R.shape[0]) if R.dim() == 4 else -1
        if T < 1 or tuple(R.shape) != (T, K, 3, 3):
            raise ValueError(f"R must be (T,{K},3,3) with T >= 1, got {tuple(R.shape)}")
        if tuple(root_pos.shape) != (T, 3):
            raise ValueError(f"root_pos must be ({T},3), got {tuple(root_pos.shape)}")
        if offset.numel() != K * 3 or offset.shape[0] != K:
            raise ValueError(f"offset must be ({K},3) or ({K},3,1), got {tuple(offset.shape)}")
        pos = torch.empty(T, K, 3, device=dev)
        eng.call("nm_retarget_fk", _lib.ptr(_f32(R, dev)), _lib.ptr(_f32(root_pos, dev)), _lib.ptr(_f32(offset.reshape(K, 3), dev)), T, K, _lib.ptr(pos))
        return pos

    def retarget_pose(self, bind, R, pos):
        """The blend of vis_retarget.py:303-322 on a bind record (the dict of skin_weights): R (T,K,3,3), pos (T,K,3) -> points (T,N,3)
        float64, out[t,n] = w_child (R[t,child] local_child + pos[t,child]) + w_parent (R[t,parent] local_parent + pos[t,parent])."""
        eng = self._eng()
        ctx = eng.ready()
        self._ensure_tree(None, ctx)
        dev, K = ctx.device, self.nkeypoints
        T = int(R.shape[0]) if R.dim() == 4 else -1
        if T < 1 or tuple(R.shape) != (T, K, 3, 3) or tuple(pos.shape) != (T, K, 3):
            raise ValueError(f"R must be (T,{K},3,3) and pos (T,{K},3) with T >= 1, got {tuple(R.shape)} and {tuple(pos.shape)}")
        N = int(bind["child"].shape[0])
        want = dict(child=((N,), torch.int32), parent=((N,), torch.int32), w=((N, 2), torch.float32), local=((N, 2, 3), torch.float64))
        for k, (shape, dtype) in want.items():
            if N < 1 or tuple(bind[k].shape) != shape or bind[k].dtype != dtype:
                raise ValueError(f"bind['{k}'] must be {shape} {dtype}, got {tuple(bind[k].shape)} {bind[k].dtype}")
        rec = {k: bind[k].detach().to(dev).contiguous() for k in want}
        out = torch.empty(T, N, 3, device=dev, dtype=torch.float64)
        eng.call("nm_retarget_pose", _lib.ptr(rec["child"]), _lib.ptr(rec["parent"]), _lib.ptr(rec["w"]), _lib.ptr(rec["local"]),
                 _lib.ptr(_f32(R, dev)), _lib.ptr(_f32(pos, dev)), T, N, K, _lib.ptr(out))
        return out


# ==========================================================================================
# top level
# ==========================================================================================
class NeuralMarionette(nn.Module):
    """model/neural_marionette.py:6-103."""

    def __init__(self, options=None):
        super().__init__()
        self.options = options
        o = HotPathOptions.from_any(options)
        o.check_fast_path()
        engine = Engine(o, self)
        object.__setattr__(self, "_engine", engine)
        self.kypt_detector = KyptDetector(o, _engine=engine)
        self.Tcond = o.Tcond
        self.dyna_module = HSVRNNBVH(o, _engine=engine)
        self.current_actives = {"detector": True, "learner": True}
        self.transition_type = o.transition_type

    def anneal(self, nepoch, nbatch=None):
        if nbatch is None:
            self.kypt_detector.anneal(nepoch)

    def set_conv_mode(self, mode: str) -> None:
        """Without a call of this method (and without NM355_CONV_MODE) the mode is 'auto' (below).
        'split16': convs with Cin % 16 == 0 on the fp16 matrix cores, operands split hi/lo, fp32
        accumulate (fp32-equivalent accuracy); 'fp32': exact fp32 MFMA everywhere; 'f16': the split16 kernels with the
        hi x hi product only - operands rounded to fp16, fp32 accumulation and storage (autocast-class accuracy, the
        reduced-precision training mode; outside the 1e-4 parity contract); 'bf16': 'f16' arithmetic with bfloat16 STORAGE of the
        training path's activations and activation gradients (BASELINE config 3 as named: every tensor of >= 32^3 voxels per frame
        the training forward keeps, fp32 master weights / GroupNorm statistics / accumulators / Adam; the inference forward is
        'f16'); 'auto': split16, but the first conv-running call after
        every weight change is range-checked synchronously and re-run on the exact fp32 path if an activation left the fp16 range
        (fp32 then stays selected until the weights change).  In every mode the library's deferred range guard makes a LATER call
        raise NmError when an earlier one produced non-finite values (no per-call host synchronisation)."""
        if mode not in CONV_MODE_NAMES:
            raise ValueError("conv mode must be one of " + ", ".join(repr(m) for m in CONV_MODE_NAMES))
        eng = self._engine
        eng.conv_mode = CONV_MODES[mode]
        eng.auto, eng._probe, eng._auto_fp32 = mode == "auto", True, False
        eng.auto_explicit = mode == "auto"

    def check_finite(self) -> None:
        """Synchronises and raises NmError if a convolution has produced non-finite values since the last check - in the default
        'split16' conv mode that is what an activation beyond the fp16 range (|x| >= 65520) turns into, where the reference's
        fp32 arithmetic stays finite; ``set_conv_mode('fp32')`` has no such limit (nm_ctx_check_nonfinite)."""
        eng = self._engine
        eng.ready()
        eng.call("nm_ctx_check_nonfinite")

    def voxelize(self, points, scale: float = 1.0, return_indices: bool = False):
        """Device version of the reference's input path (utils/dataset_utils.py:9-31 as used by
        dataset/dataset.py:70-86 and vis_generation.py:14-25): per-episode bbox normalisation + occupancy
        voxelisation.  points (T,N,3) -> (T,1,G,G,G) fp32; voxel indices are bit-exact (fp64 arithmetic)."""
        eng = self._engine
        ctx = eng.ready()
        pts = points.detach().to(device=ctx.device, dtype=torch.float64).contiguous()
        T, N = int(pts.shape[0]), int(pts.shape[1])
        G = eng.opts.grid_size
        vox = torch.empty(T, 1, G, G, G, device=ctx.device)
        idx = torch.empty(T, N, 3, device=ctx.device, dtype=torch.int32) if return_indices else None
        eng.call("nm_voxelize_clip", _lib.ptr(pts), T, N, float(scale), _lib.ptr(vox), _lib.ptr(idx))
        return (vox, idx) if return_indices else vox

    def voxelize_batch(self, bank, ids, starts, T, sample_rate: int = 1, scale=1.0, x_trans=0.0, z_trans=0.0, return_joints: bool = False,
                       return_indices: bool = False, check: bool = False, pad=None):
        """The reference's per-item input path (dataset/dataset.py:47-88, :123-183: crop_sequence -> episodic_normalization ->
        voxelize) for a batch of crops of device-resident sequences, in one stream-ordered library call (nm_voxelize_batch), in the
        reference's arithmetic for the dtype the data has: float32 sequences are normalised in float32 and become float64 at the
        translation add, as numpy does it.  bank: data.ClipBank; clip b is frames starts[b] + t * sample_rate, t < T, of sequence
        ids[b]; pad[b]: frames past the end repeat the last one (data.ClipSampler says when the reference does that), otherwise the
        crop must fit.  scale / x_trans / z_trans: one value or one per clip.
        Returns a dict: vox (B,T,1,G,G,G) fp32; joints (B,T,J,3) [return_joints: normalised with the clip's box, no translation,
        float32 only when points and joints both are]; indices (B,T,N,3) int32 [return_indices: before numpy's negative-index wrap];
        bbox (B,6) float64 (bmin, bmax); bad_rows (B) int32: rows with an index outside [-G,G) or a non-finite coordinate - they set
        no voxel.  The reference raises for such a clip: check=True reads bad_rows (the call's one synchronisation) and raises
        ValueError("Dataset voxelizer error") like it.  The descriptors travel through pinned staging; nothing else is copied."""
        from . import data
        return data.voxelize_batch(self, bank, ids, starts, T, sample_rate=sample_rate, scale=scale, x_trans=x_trans, z_trans=z_trans,
                                   return_joints=return_joints, return_indices=return_indices, check=check, pad=pad)

    @torch.no_grad()
    def sample_surface(self, vertices, triangles, count: int = 20000, seed: int = 0, u=None, check: bool = False, return_tables: bool = False):
        """Device version of the reference's offline preparation (dataset/dfaust/write_sequence_to_obj.py:20-23, :107-115,
        dataset/aistpp/prepare_aistpp.py:13-16, :75-83: trimesh.sample.sample_surface(mesh, 20000) and mesh.face_normals per frame):
        ``count`` points on the surface of every frame of a mesh sequence, a face picked in proportion to its area and a point
        uniformly inside it, in one stream-ordered call (nm_sample_surface, csrc/nm_sample.hip).  **Not trimesh's random stream and
        not its bits**: the result is defined by the contract of include/nm355.h alone (tests/sample_ref.py restates it).  It is
        trimesh's algorithm with integer face weights - the areas scaled by the power of two above the frame's largest and floored, so
        the cumulative table does not depend on the order of a parallel sum - and uniforms from Philox4x32-10 keyed by ``seed`` and
        counted by (sample, frame).  A face below 2^-32 of the frame's largest area is never picked.
        vertices: (T,V,3) float32 or float64, triangles: (F,3) int32 or int64 shared by all frames, F <= 2^21, both contiguous on the
        network's device.  u: (T,count,3) float64 uniforms in [0, 1) of the caller's instead of the generator's (face, then the two
        barycentric draws).
        Returns a dict: points (T,count,3) float32 - what ClipBank.add takes; normals (T,count,3) float32, the picked faces' unit
        normals (zero for a degenerate face); face_index (T,count) int32; bad_faces, empty_frames: 0-d int32 device tensors - rows of
        ``triangles`` with an index outside the vertices (they have no area and are never read through), and frames whose faces all
        have weight 0 (their points are vertex 0 of face 0, their normals zero).  check=True reads the two (the call's one
        synchronisation) and raises ValueError if either is not 0.  return_tables=True adds areas (T,F) float64, cum (T,F) int64 -
        the inclusive sums of the integer weights - and uniforms (T,count,3) float64 as used."""
        who = "sample_surface"
        for name, t in (("vertices", vertices), ("triangles", triangles)) + ((("u", u),) if u is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if vertices.dtype not in (torch.float32, torch.float64) or vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1:
            raise ValueError(f"{who}: vertices must be (T,V,3) float32 or float64 with T, V >= 1, got {tuple(vertices.shape)} {vertices.dtype}")
        if triangles.dtype not in (torch.int32, torch.int64) or triangles.dim() != 2 or triangles.shape[1] != 3:
            raise ValueError(f"{who}: triangles must be (F,3) int32 or int64, got {tuple(triangles.shape)} {triangles.dtype}")
        T, V, F = int(vertices.shape[0]), int(vertices.shape[1]), int(triangles.shape[0])
        if not 1 <= F <= 2 ** 21:
            raise ValueError(f"{who}: {F} faces, a call takes 1 .. 2^21 (a frame's integer weights sum below 2^53)")
        if isinstance(count, bool) or not isinstance(count, int) or count < 1:
            raise ValueError(f"{who}: count must be an integer >= 1, got {count!r}")
        if count >= 2 ** 31 - 1024 or T * ((count + 1023) // 1024) >= 2 ** 31 or T >= 2 ** 31 or V >= 2 ** 31:
            raise ValueError(f"{who}: {T} frames of {count} samples, one call launches fewer than 2^31 workgroups")
        if u is not None and (u.dtype != torch.float64 or tuple(u.shape) != (T, count, 3)):
            raise ValueError(f"{who}: u must be ({T},{count},3) float64, got {tuple(u.shape)} {u.dtype}")
        tensors = [("vertices", vertices), ("triangles", triangles)] + ([("u", u)] if u is not None else [])
        for name, t in tensors:
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous on the network's device, got {t.device}")
        eng = self._engine
        dev = eng._device()
        for name, t in tensors:
            if t.device != dev:
                raise ValueError(f"{who}: {name} must be on the network's device ({dev}), got {t.device}")
        ctx = eng.ready()
        nbytes = int(ctx.lib.nm_sample_surface_workspace(T, F))
        if nbytes == 0:
            raise _lib.NmError(f"{who}: no workspace size for {T} frames of {F} faces")
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        out = dict(points=torch.empty(T, count, 3, device=dev), normals=torch.empty(T, count, 3, device=dev),
                   face_index=torch.empty(T, count, device=dev, dtype=torch.int32))
        counters = torch.empty(2, device=dev, dtype=torch.int32)
        used = torch.empty(T, count, 3, device=dev, dtype=torch.float64) if return_tables and u is None else None
        eng.call("nm_sample_surface", vertices.data_ptr(), int(vertices.dtype == torch.float64), triangles.data_ptr(),
                 int(triangles.dtype == torch.int64), T, V, F, count, int(seed) & (2 ** 64 - 1), _lib.ptr(u), scratch.data_ptr(), nbytes,
                 _lib.ptr(out["points"]), _lib.ptr(out["normals"]), _lib.ptr(out["face_index"]), _lib.ptr(used), _lib.ptr(counters))
        out["bad_faces"], out["empty_frames"] = counters[0], counters[1]
        if return_tables:
            out["areas"] = torch.empty(T, F, device=dev, dtype=torch.float64)
            out["cum"] = torch.empty(T, F, device=dev, dtype=torch.int64)
            eng.call("nm_sample_tables", scratch.data_ptr(), T, F, _lib.ptr(out["areas"]), out["cum"].data_ptr())
            out["uniforms"] = used if u is None else u
        if check:
            bad, empty = (int(x) for x in counters.tolist())          # (the one synchronisation)
            if bad or empty:
                raise ValueError(f"{who}: {bad} faces with a vertex index outside [0, {V}), {empty} frames without surface")
        return out

    @torch.no_grad()
    def pose_bodies(self, model, poses=None, rotations=None, betas=None, transl=None, scaling: float = 1.0, return_joints: bool = True,
                    dtype=torch.float64):
        """Device version of the body-model step of the reference's AIST++ preparation (dataset/aistpp/prepare_aistpp.py:54-62: smplx's
        ``SMPL(...).forward(global_orient, body_pose, transl, scaling).vertices``; :86-89: the joint regressor times the posed vertices):
        ``model`` (body.BodyModel, on the network's device) posed for T frames - linear blend skinning with shape and pose blend shapes
        (nm_body_shape / nm_body_pose / nm_body_joints, csrc/nm_body.hip).  **Not smplx's float32 arithmetic**: the result is defined by
        the contract of include/nm355.h alone, in float64 (tests/body_ref.py restates it), and the order "scale, then translate" is this
        library's choice.
        Exactly one of poses (T,J,3) axis-angle, float32 or float64, and rotations (T,J,3,3) float64 is given; betas (S) float32 or float64
        (None: the template), transl (T,3) float32 or float64 (None: no translation), all contiguous on the network's device; scaling a
        finite number other than 0.
        Returns a dict: vertices (T,V,3); rotations (T,J,3,3) float64 - computed from poses (the one stage with sin, cos and a square
        root), or the tensor given; posed_joints (T,J,3), the kinematic chain's; joints (T,J,3), the regressor over the posed, scaled,
        translated vertices [return_joints]; v_shaped (V,3) and J_rest (J,3) float64, cached on the model per betas tensor (the tensor
        object and its version).  dtype=torch.float32 returns rounded copies of vertices, posed_joints and joints.  Never synchronises,
        no atomics: results are bit-identical from run to run."""
        from .body import BodyModel
        who = "pose_bodies"
        if not isinstance(model, BodyModel):
            raise ValueError(f"{who}: model must be a neural_marionette_amd.BodyModel, got {type(model).__name__}")
        if (poses is None) == (rotations is None):
            raise ValueError(f"{who}: exactly one of poses and rotations is given")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{who}: dtype must be torch.float32 or torch.float64, got {dtype}")
        given = [(n, t) for n, t in (("poses", poses), ("rotations", rotations), ("betas", betas), ("transl", transl)) if t is not None]
        for name, t in given:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        V, J, S = model.V, model.J, model.S
        if poses is not None and (poses.dtype not in (torch.float32, torch.float64) or poses.dim() != 3 or tuple(poses.shape[1:]) != (J, 3) or poses.shape[0] < 1):
            raise ValueError(f"{who}: poses must be (T,{J},3) float32 or float64 with T >= 1, got {tuple(poses.shape)} {poses.dtype}")
        if rotations is not None and (rotations.dtype != torch.float64 or rotations.dim() != 4 or tuple(rotations.shape[1:]) != (J, 3, 3) or rotations.shape[0] < 1):
            raise ValueError(f"{who}: rotations must be (T,{J},3,3) float64 with T >= 1, got {tuple(rotations.shape)} {rotations.dtype}")
        T = int((poses if poses is not None else rotations).shape[0])
        if betas is not None and (betas.dtype not in (torch.float32, torch.float64) or tuple(betas.shape) != (S,)):
            raise ValueError(f"{who}: betas must be ({S}) float32 or float64, got {tuple(betas.shape)} {betas.dtype}")
        if transl is not None and (transl.dtype not in (torch.float32, torch.float64) or tuple(transl.shape) != (T, 3)):
            raise ValueError(f"{who}: transl must be ({T},3) float32 or float64, got {tuple(transl.shape)} {transl.dtype}")
        if isinstance(scaling, bool) or not isinstance(scaling, (int, float)) or not np.isfinite(scaling) or scaling == 0:
            raise ValueError(f"{who}: scaling must be a finite number other than 0, got {scaling!r}")
        if T * V >= 2 ** 31 or T * J * 3 >= 2 ** 31:
            raise ValueError(f"{who}: {T} frames of {V} vertices and {J} joints, one call indexes fewer than 2^31 rows")
        for name, t in given:
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous on the network's device, got {t.device}")
        eng = self._engine
        dev = eng._device()
        for name, t in given + [("model", model.v_template)]:
            if t.device != dev:
                raise ValueError(f"{who}: {name} must be on the network's device ({dev}), got {t.device}")
        eng.ready()
        null = lambda t: t.data_ptr() if t is not None and t.numel() else None
        f64 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float64)
        # shape: once per (model, betas tensor)
        key = None if betas is None or S == 0 else id(betas)
        hit = model._shape_cache.get(key)
        if hit is None or (key is not None and (hit[0] is not betas or hit[1] != betas._version)):
            b64 = None if key is None else betas.to(torch.float64)
            v_shaped, J_rest = f64(V, 3), f64(J, 3)
            eng.call("nm_body_shape", model.v_template.data_ptr(), null(model.shapedirs), null(b64), V, S, J, model.reg_offsets.data_ptr(),
                     null(model.reg_cols), null(model.reg_vals), int(model.reg_cols.numel()), v_shaped.data_ptr(), J_rest.data_ptr())
            if key is not None:
                model._shape_cache = {k: h for k, h in model._shape_cache.items() if k is None}     # one betas tensor at a time
            hit = model._shape_cache[key] = (betas, None if key is None else betas._version, v_shaped, J_rest)
        v_shaped, J_rest = hit[2], hit[3]
        t64 = None if transl is None else transl.to(torch.float64)
        rot_out = f64(T, J, 3, 3) if poses is not None else None
        transforms, posed, vertices = f64(T, J, 3, 4), f64(T, J, 3), f64(T, V, 3)
        parents = np.ascontiguousarray(model.parents, dtype=np.int32)
        eng.call("nm_body_pose", null(poses), int(poses is not None and poses.dtype == torch.float64), null(rotations), T, V, J,
                 parents.ctypes.data_as(_lib.c_int32_p), v_shaped.data_ptr(), J_rest.data_ptr(), null(model.posedirs), model.lbs_weights.data_ptr(),
                 null(t64), float(scaling), null(rot_out), transforms.data_ptr(), posed.data_ptr(), vertices.data_ptr())
        out = dict(vertices=vertices, rotations=rotations if rot_out is None else rot_out, posed_joints=posed, v_shaped=v_shaped, J_rest=J_rest)
        if return_joints:
            out["joints"] = f64(T, J, 3)
            eng.call("nm_body_joints", vertices.data_ptr(), T, V, J, model.reg_offsets.data_ptr(), null(model.reg_cols), null(model.reg_vals),
                     int(model.reg_cols.numel()), out["joints"].data_ptr())
        if dtype == torch.float32:
            for k in ("vertices", "posed_joints", "joints"):
                if k in out:
                    out[k] = out[k].to(torch.float32)
        return out

    @torch.no_grad()
    def occupied_points(self, vox, threshold=0.5, dtype=torch.float64, capacity=None, return_indices: bool = False,
                        return_depth: bool = False, return_bits: bool = False):
        """Device version of the host lines every consumer of the decoder's voxels starts with (vis_generation.py:137-170,
        vis_interpolation.py:141-177, vis/visualize.py:58-59, :130-137): binarise at ``threshold``, np.where / torch.where per frame,
        ``/ ((G - 1) / 2) - 1``, and the clip-wide min_z / max_z of the last coordinate with the shading's (z - min_z) / z_len.
        vox: (T,1,G,G,G) - one clip - or (B,T,1,G,G,G), float32 and contiguous on the network's device; G is the tensor's and need not be
        the network's grid.  It is not modified.  threshold: occupied iff NOT (v < threshold), what the scripts' two in-place assignments
        leave non-zero (a NaN is occupied), the threshold rounded to float32 as torch rounds a Python number it compares a float32 tensor
        with; None: occupied iff v != 0 (torch.where on an un-thresholded tensor).  dtype: torch.float64 - numpy's arithmetic, what the
        vis_* scripts compute - or torch.float32 - torch's, what vis_recon computes; the two are not roundings of each other.
        Returns a dict: coords (N,3) in np.where's order, frame after frame; offsets (F+1) int64, the first row of each of the F = B T
        frames and the total; counts (B,T) int64; z_range (B,2), min_z / max_z per clip, (1e4, -1) for a clip without a point; indices
        (N,3) int32 [return_indices]; depth (N) float64 [return_depth, float64 only]: (z - min_z) / (max_z - min_z) with the point's own
        clip's range, NaN where that is zero; bits (F, 8 ceil(G^3 / 64)) uint8 [return_bits]: np.packbits(occ, bitorder='little') per
        frame, zero-padded to whole 64-bit words.
        capacity=None reads offsets[-1] - the call's one synchronisation - and allocates exactly N rows.  With a capacity the call
        never synchronises and returns ``capacity`` rows, of which the first min(capacity, offsets[-1]) are written."""
        return self._occupied("occupied_points", vox, threshold, dtype, capacity, return_indices, return_depth, return_bits)[0]

    def _occupied(self, who, vox, threshold, dtype, capacity, return_indices, return_depth, return_bits):
        """occupied_points for the shell ``who``: its dict, and (B, T, G, bits, z_idx_range) for a second library call on the same masks"""
        if not isinstance(vox, torch.Tensor) or vox.dim() not in (5, 6):
            raise ValueError(f"{who}: vox must be a (T,1,G,G,G) or (B,T,1,G,G,G) tensor" +
                             (f", got {tuple(vox.shape)}" if isinstance(vox, torch.Tensor) else ""))
        shape = tuple(vox.shape) if vox.dim() == 6 else (1,) + tuple(vox.shape)
        B, T, G = shape[0], shape[1], shape[3]
        if shape[2:] != (1, G, G, G) or G < 2 or B < 1 or T < 1:
            raise ValueError(f"{who}: vox must be (T,1,G,G,G) or (B,T,1,G,G,G) with G >= 2 and at least one frame, got {tuple(vox.shape)}")
        if vox.dtype != torch.float32:
            raise ValueError(f"{who}: vox must be float32, got {vox.dtype}")
        if dtype not in (torch.float64, torch.float32):
            raise ValueError(f"{who}: dtype must be torch.float64 (numpy's arithmetic) or torch.float32 (torch's), got {dtype}")
        if return_depth and dtype != torch.float64:
            raise ValueError(f"{who}: depth is float64 arithmetic (the vis_* scripts' shading): return_depth needs dtype=torch.float64")
        if capacity is not None and int(capacity) < 0:
            raise ValueError(f"{who}: capacity must be >= 0, got {capacity}")
        if B * T * G ** 3 >= 2 ** 31:
            raise ValueError(f"{who}: {B * T} frames of {G}^3 voxels, one call indexes fewer than 2^31")
        pdev = next(self.parameters()).device
        if not vox.is_cuda or vox.device != pdev:
            raise ValueError(f"{who}: vox must be on the network's device (a HIP device; the network is on {pdev}), got {vox.device}")
        if not vox.is_contiguous():
            raise ValueError(f"{who}: vox must be contiguous")
        eng = self._engine
        ctx = eng.ready()
        dev, F, W, f64 = ctx.device, B * T, (G ** 3 + 63) // 64, int(dtype == torch.float64)
        bits = torch.empty(F * W, device=dev, dtype=torch.int64)
        offsets = torch.empty(F + 1, device=dev, dtype=torch.int64)
        zi = torch.empty(B, 2, device=dev, dtype=torch.int32)
        zr = torch.empty(B, 2, device=dev, dtype=dtype)
        eng.call("nm_occupied_count", _lib.ptr(vox), B, T, G, 1 if threshold is None else 0, 0.0 if threshold is None else float(threshold),
                 f64, bits.data_ptr(), offsets.data_ptr(), _lib.ptr(zi), _lib.ptr(zr))
        N = int(offsets[-1].item()) if capacity is None else int(capacity)
        coords = torch.empty(N, 3, device=dev, dtype=dtype)
        idx = torch.empty(N, 3, device=dev, dtype=torch.int32) if return_indices else None
        depth = torch.empty(N, device=dev, dtype=torch.float64) if return_depth else None
        if N:
            eng.call("nm_occupied_write", bits.data_ptr(), offsets.data_ptr(), _lib.ptr(zi), B, T, G, f64, N, _lib.ptr(idx), _lib.ptr(coords),
                     _lib.ptr(depth))
        out = dict(coords=coords, offsets=offsets, counts=(offsets[1:] - offsets[:-1]).view(B, T), z_range=zr)
        if return_indices:
            out["indices"] = idx
        if return_depth:
            out["depth"] = depth
        if return_bits:
            out["bits"] = bits.view(torch.uint8).view(F, W * 8)
        return out, (B, T, G, bits, zi)

    @torch.no_grad()
    def surface_points(self, vox, threshold=0.5, radius2=6, orient="outward", base_colors=None, add_colors=None, shade=(0.8, 0.2),
                       capacity=None, return_moments: bool = False):
        """Device version of what the demo scripts do with every decoded frame after occupied_points' lines (vis_generation.py:157-171,
        vis_interpolation.py:160-177): a surface normal per point, the [R | centre] rows of drawPlate's transform and the shaded colour
        (nm_occupied_surface, csrc/nm_surface.hip).  The normals are NOT open3d's: on a voxel lattice its 30-nearest-neighbour set is
        decided by tie-breaking inside a shell of equidistant points, so the neighbourhood here is the occupied voxels of the point's
        frame within squared lattice distance ``radius2`` (1 .. 16), the moments are exact integers, and the normal is the unit
        eigenvector of the smallest eigenvalue of n Q - S S^T in float64 - (0, 0, 1) for fewer than three neighbours.
        vox, threshold, capacity: as occupied_points (float64 arithmetic).  orient: "outward" - away from the local mass (n . -S > 0;
        S = 0: away from the frame's centroid; then (1, 1, 1); a dot product of exactly zero keeps the solver's sign) - or a point (3) /
        one per clip (B,3): n is flipped where n . (point - coords) < 0 (open3d's orient_normals_towards_camera_location).
        base_colors / add_colors: (3), (T,3), (B,T,3) or (B T,3), one colour per frame; colors = base * (depth * shade[0] + shade[1])
        (+ add) in numpy's operation order - shade (0.8, 0.2) is vis_generation's, (0.9, 0.1) with an additive term
        vis_interpolation's.  Colours and an orientation point given as lists, numpy arrays or CPU tensors are copied to the device
        by the call, a pageable copy that makes the host wait: with ``capacity`` the call never synchronises only if they are float64
        tensors on the network's device already (they are then used as they are).
        Returns occupied_points' dict with depth - coords (N,3), offsets, counts, z_range, depth (N) - and normals (N,3), spread (N,3)
        [the eigenvalues, ascending], plates (N,3,4), colors (N,3) [base_colors given], moments (N,10) int32 [return_moments: n, S (x, y,
        z), Q (xx, xy, xz, yy, yz, zz) over the offsets q - p].  render_plates draws the result through a pinhole camera."""
        who = "surface_points"
        try:
            r2 = int(radius2)
        except (TypeError, ValueError):
            r2 = 0
        if r2 != radius2 or not 1 <= r2 <= 16:
            raise ValueError(f"{who}: radius2 must be an integer from 1 to 16, got {radius2!r}")
        try:
            shade_a, shade_b = (float(v) for v in shade)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: shade must be two numbers (a, b) of depth * a + b, got {shade!r}") from None
        if add_colors is not None and base_colors is None:
            raise ValueError(f"{who}: add_colors without base_colors")
        if isinstance(orient, str) and orient != "outward":
            raise ValueError(f'{who}: orient must be "outward" or a point (3) / one point per clip (B,3), got {orient!r}')
        out, (B, T, G, bits, zi) = self._occupied(who, vox, threshold, torch.float64, capacity, False, True, False)
        dev, F = bits.device, B * T

        def per_frame(x, name):
            try:
                t = torch.as_tensor(x, dtype=torch.float64)
                t = t.reshape(B, T, 3) if tuple(t.shape) == (F, 3) else torch.broadcast_to(t, (B, T, 3))
            except (RuntimeError, TypeError, ValueError):
                raise ValueError(f"{who}: {name} must be (3), (T,3), (B,T,3) or (B T,3) numbers for {B} x {T} frames") from None
            return t.to(dev).contiguous()

        point = None
        if not isinstance(orient, str):
            try:
                point = torch.broadcast_to(torch.as_tensor(orient, dtype=torch.float64), (B, 3)).to(dev).contiguous()
            except (RuntimeError, TypeError, ValueError):
                raise ValueError(f'{who}: orient must be "outward" or a point (3) / one point per clip (B,3) for {B} clips') from None
        base = per_frame(base_colors, "base_colors") if base_colors is not None else None
        add = per_frame(add_colors, "add_colors") if add_colors is not None else None
        N = int(out["coords"].shape[0])
        out["normals"] = torch.empty(N, 3, device=dev, dtype=torch.float64)
        out["spread"] = torch.empty(N, 3, device=dev, dtype=torch.float64)
        out["plates"] = torch.empty(N, 3, 4, device=dev, dtype=torch.float64)
        if base is not None:
            out["colors"] = torch.empty(N, 3, device=dev, dtype=torch.float64)
        if return_moments:
            out["moments"] = torch.empty(N, 10, device=dev, dtype=torch.int32)
        if N:
            self._engine.call("nm_occupied_surface", bits.data_ptr(), out["offsets"].data_ptr(), _lib.ptr(zi), B, T, G, r2, 0 if point is None else 1,
                              _lib.ptr(point), _lib.ptr(base), _lib.ptr(add), shade_a, shade_b, N, _lib.ptr(out.get("moments")),
                              _lib.ptr(out["normals"]), _lib.ptr(out["spread"]), _lib.ptr(out["plates"]), _lib.ptr(out.get("colors")))
        return out

    @torch.no_grad()
    def render_plates(self, points, camera, radius=0.03, light=(1.0, 0.0), background=(1.0, 1.0, 1.0), bin_capacity=None,
                      return_index: bool = False, return_depth: bool = False):
        """Device version of the demo scripts' last step (vis_generation.py:171-190, vis_interpolation.py:177-185: a cylinder mesh per
        plate into open3d's off-screen visualiser and capture_screen_float_buffer): every plate of ``points`` - surface_points' dict, or
        a driver's ``points`` under return_points="surface" chained with colours - drawn as a flat disc of ``radius`` through
        ``camera`` (render.PinholeCamera), the nearest disc winning each pixel (nm_render_bin + nm_render_draw, csrc/nm_render.hip).
        **This is not open3d's image**: its lighting, MSAA and GL rasterisation rules are not reproducible, so the result is defined by
        the contract of include/nm355.h alone (tests/render_ref.py restates it): plate i is the disc about plates[i,:,3] with axis
        plates[i,:,2] - the cylinder's cap, both faces visible, its 0.01 side wall not drawn; pixel (px, py), row 0 at the top, looks
        along ((px - cx) / fx, (py - cy) / fy, 1); plates that reach in front of ``camera.near`` are not drawn; of equal depths the lower
        row wins.  The pixel is colors[i] * (light[0] + light[1] * |cos(axis, ray)|) clamped to [0, 1] (NaN: 0) and truncated to uint8 as
        the scripts' (img * 255).astype(uint8); light (1, 0) leaves the colours - which carry the scripts' depth shading already - flat.
        points needs ``plates`` (N,3,4), ``offsets`` (F+1) and ``colors`` (N,3) [surface_points(base_colors=...)]; ``counts`` (B,T) gives
        the result its leading shape, (1,F) without it.
        Returns a dict: image (B,T,H,W,3) uint8; bin_total, a 0-d int64 device tensor - the number of (tile, plate) list entries the
        draw needs; index (B,T,H,W) int32 [return_index]: the winner's row, -1 for background; depth (B,T,H,W) float64 [return_depth]:
        its distance along the camera's z, +inf for background.
        bin_capacity=None reads bin_total - the call's one synchronisation - and sizes the lists exactly.  With a bin_capacity the
        call never synchronises; if bin_total turns out larger, nothing faults but the image is INCOMPLETE (the tiles past the capacity
        lose plates): compare ``bin_total`` with it afterwards.  No atomics touch an output: results are bit-identical from run to run."""
        from .render import PinholeCamera
        who = "render_plates"
        if not isinstance(camera, PinholeCamera):
            raise ValueError(f"{who}: camera must be a neural_marionette_amd.PinholeCamera, got {type(camera).__name__}")
        if not isinstance(points, dict) or "plates" not in points or "offsets" not in points:
            raise ValueError(f"{who}: points must be surface_points' dict with 'plates' and 'offsets'")
        if "colors" not in points:
            raise ValueError(f"{who}: points has no 'colors': call surface_points with base_colors (one colour per frame)")
        try:
            radius = float(radius)
            light_a, light_b = (float(v) for v in light)
            bg = [float(v) for v in background]
        except (TypeError, ValueError):
            raise ValueError(f"{who}: radius must be a number, light two numbers (a, b) and background three") from None
        if len(bg) != 3:
            raise ValueError(f"{who}: background must be three numbers, got {background!r}")
        if not (radius > 0.0 and radius < float("inf")):
            raise ValueError(f"{who}: radius must be a finite number > 0, got {radius}")
        if bin_capacity is not None and int(bin_capacity) < 0:
            raise ValueError(f"{who}: bin_capacity must be >= 0, got {bin_capacity}")
        plates, offsets, colors = points["plates"], points["offsets"], points["colors"]
        eng = self._engine
        ctx = eng.ready()
        dev = ctx.device
        N = int(plates.shape[0])
        if plates.dtype != torch.float64 or tuple(plates.shape) != (N, 3, 4) or colors.dtype != torch.float64 or tuple(colors.shape) != (N, 3):
            raise ValueError(f"{who}: plates must be (N,3,4) and colors (N,3) float64, got {tuple(plates.shape)} {plates.dtype} and {tuple(colors.shape)} {colors.dtype}")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
            raise ValueError(f"{who}: offsets must be (F+1) int64, got {tuple(offsets.shape)} {offsets.dtype}")
        for name, t in (("plates", plates), ("offsets", offsets), ("colors", colors)):
            if not t.is_cuda or t.device != dev or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous on the network's device ({dev}), got {t.device}")
        F = int(offsets.numel()) - 1
        lead = tuple(points["counts"].shape) if "counts" in points and points["counts"].numel() == F else (1, F)
        H, W = camera.height, camera.width
        if F * H * W >= 2 ** 31:
            raise ValueError(f"{who}: {F} frames of {W} x {H} pixels, one call indexes fewer than 2^31")
        cam = camera.c_struct()
        TX, TY = (W + 15) // 16, (H + 15) // 16
        xf = torch.empty(N, 8, device=dev, dtype=torch.float64)
        rect = torch.empty(N, 4, device=dev, dtype=torch.int32)
        tile_offsets = torch.empty(F * TX * TY + 1, device=dev, dtype=torch.int64)
        eng.call("nm_render_bin", plates.data_ptr(), offsets.data_ptr(), F, N, C.byref(cam), radius, xf.data_ptr(), rect.data_ptr(), tile_offsets.data_ptr())
        cap = int(tile_offsets[-1].item()) if bin_capacity is None else int(bin_capacity)
        lst = torch.empty(cap, device=dev, dtype=torch.int32)
        out = dict(image=torch.empty(lead + (H, W, 3), device=dev, dtype=torch.uint8), bin_total=tile_offsets[-1])
        if return_index:
            out["index"] = torch.empty(lead + (H, W), device=dev, dtype=torch.int32)
        if return_depth:
            out["depth"] = torch.empty(lead + (H, W), device=dev, dtype=torch.float64)
        null = lambda t: t.data_ptr() if t is not None and t.numel() else None
        eng.call("nm_render_draw", null(xf), null(rect), offsets.data_ptr(), tile_offsets.data_ptr(), null(colors), F, N, C.byref(cam), radius, light_a,
                 light_b, (C.c_double * 3)(*bg), cap, null(lst), null(out.get("index")), null(out.get("depth")), out["image"].data_ptr())
        return out

    @torch.no_grad()
    def render_frames(self, vox, camera, threshold=0.5, radius2=6, base_colors=(0.6, 1.0, 0.6), add_colors=None, shade=(0.8, 0.2), radius=0.03,
                      orient="outward", light=(1.0, 0.0), background=(1.0, 1.0, 1.0), bin_capacity=None, return_index: bool = False,
                      return_depth: bool = False, return_points: bool = False):
        """The demo scripts' whole inner loop from a decoded batch (vis_generation.py:137-190, vis_interpolation.py:141-185):
        surface_points(vox, threshold, radius2, orient, base_colors, add_colors, shade) followed by render_plates(points, camera, radius,
        light, background, bin_capacity, ...).  base_colors' default is vis_generation's green.  Returns render_plates' dict, with
        surface_points' under ``points`` [return_points].  **Not open3d's image**: see render_plates."""
        if base_colors is None:
            raise ValueError("render_frames: base_colors must give one colour per frame (or one for all)")
        pts = self.surface_points(vox, threshold, radius2=radius2, orient=orient, base_colors=base_colors, add_colors=add_colors, shade=shade)
        out = self.render_plates(pts, camera, radius=radius, light=light, background=background, bin_capacity=bin_capacity,
                                 return_index=return_index, return_depth=return_depth)
        if return_points:
            out["points"] = pts
        return out

    def _plan_values(self, who, values, plan, count, name="values"):
        """values (T,count,3) or (count,3) float64 on the network's device and a LoopPlan there -> the 3-d tensor, whether it was 2-d"""
        if not isinstance(plan, LoopPlan):
            raise ValueError(f"{who}: plan must be a neural_marionette_amd.LoopPlan, got {type(plan).__name__}")
        if not isinstance(values, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a tensor, got {type(values).__name__}")
        flat = values.dim() == 2
        v3 = values[None] if flat else values
        n = plan.vertex_counts[count]
        if values.dtype != torch.float64 or v3.dim() != 3 or tuple(v3.shape[1:]) != (n, 3) or v3.shape[0] < 1:
            raise ValueError(f"{who}: {name} must be (T,{n},3) or ({n},3) float64 with T >= 1, got {tuple(values.shape)} {values.dtype}")
        if not values.is_cuda or not values.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous on the network's device, got {values.device}")
        dev = self._engine._device()
        if values.device != dev or plan.device != dev:
            raise ValueError(f"{who}: {name} and the plan must be on the network's device ({dev}), got {values.device} and {plan.device}")
        return v3, flat

    @torch.no_grad()
    def subdivide(self, values, plan, bytes_bound: Optional[int] = None):
        """Device version of vis_retarget.py's ``temp_mesh.subdivide_loop(arg.subdivide_iter)`` (:416-423, :497-512: open3d, on the host,
        every frame): ``plan.levels`` Loop subdivisions of ``values`` (T,V,3) or (V,3) float64 - sample_retarget's posed ``points``, or
        the vertex colours, which the script's mesh carries through the same stencils - by ``plan`` (LoopPlan.build(triangles, V,
        levels), built once per mesh).  nm_subdiv_apply per level (csrc/nm_subdiv.hip).  **Not open3d's vertex order**: the contract is
        include/nm355.h's, tests/subdiv_ref.py restates it.  Returns (T,V_L,3), or (V_L,3) for (V,3) values; the matching triangles are
        ``plan.triangles``.  The frames go in groups whose intermediate levels stay under ``bytes_bound`` (SUBDIV_BYTES = 512 MiB by
        default; a single frame past the bound goes alone); the result does not depend on the grouping.  Never synchronises, no atomics:
        results are bit-identical from run to run."""
        who = "subdivide"
        v3, flat = self._plan_values(who, values, plan, 0)
        bound = SUBDIV_BYTES if bytes_bound is None else int(bytes_bound)
        if bound < 1:
            raise ValueError(f"{who}: bytes_bound must be >= 1, got {bytes_bound}")
        if plan.levels == 0:
            return values.clone()
        eng = self._engine
        dev = eng._device()
        eng.ready()
        T, counts = int(v3.shape[0]), plan.vertex_counts
        out = torch.empty(T, counts[-1], 3, device=dev, dtype=torch.float64)
        bad = torch.empty(1, device=dev, dtype=torch.int32)
        group = max(1, min(T, bound // max(1, 24 * sum(counts[1:-1]))))
        mid = [torch.empty(group, n, 3, device=dev, dtype=torch.float64) for n in counts[1:-1]]
        null = lambda t: t.data_ptr() if t.numel() else None
        for f0 in range(0, T, group):
            n = min(group, T - f0)
            src = v3[f0:]
            for level, tab in enumerate(plan.levels_tables):
                dst = out[f0:] if level == plan.levels - 1 else mid[level]
                eng.call("nm_subdiv_apply", src.data_ptr(), n, counts[level], int(tab["edge"].shape[0]), null(tab["edge"]), tab["ring_offsets"].data_ptr(),
                         null(tab["ring"]), int(tab["ring"].numel()), tab["w"].data_ptr(), dst.data_ptr(), bad.data_ptr())
                src = dst
        return out[0] if flat else out

    @torch.no_grad()
    def vertex_normals(self, vertices, plan):
        """Device version of open3d's ``compute_vertex_normals()`` as vis_retarget.py calls it per frame (:421, :510): smooth unit normals
        (F,V_L,3) float64 of ``vertices`` (F,V_L,3) or (V_L,3) float64 over ``plan.triangles`` - the finest level of ``plan``, or the
        mesh itself for a plan of 0 levels (nm_vertex_normals, csrc/nm_subdiv.hip).  **Not open3d's normals**: each is the sum of its
        triangles' cross products in ascending row order, so AREA-WEIGHTED, divided by its length; a vertex whose sum is zero (no
        triangle, or degenerate ones only) or not finite gets (0, 0, 0).  Contract: include/nm355.h; tests/subdiv_ref.py restates it."""
        who = "vertex_normals"
        v3, flat = self._plan_values(who, vertices, plan, -1, "vertices")
        eng = self._engine
        eng.ready()
        out = torch.empty_like(v3)
        bad = torch.empty(1, device=v3.device, dtype=torch.int32)
        null = lambda t: t.data_ptr() if t.numel() else None
        eng.call("nm_vertex_normals", v3.data_ptr(), int(v3.shape[0]), int(v3.shape[1]), null(plan.triangles), int(plan.triangles.shape[0]),
                 plan.face_offsets.data_ptr(), null(plan.faces), out.data_ptr(), bad.data_ptr())
        return out[0] if flat else out

    @staticmethod
    def _render_numbers(who, camera, light, background, **colors):
        """the arguments render_mesh and render_skeleton share, as floats: (light_a, light_b), background, and each named colour"""
        from .render import PinholeCamera
        if not isinstance(camera, PinholeCamera):
            raise ValueError(f"{who}: camera must be a neural_marionette_amd.PinholeCamera, got {type(camera).__name__}")
        try:
            la, lb = (float(v) for v in light)
            out = {name: [float(v) for v in value] for name, value in dict(colors, background=background).items()}
        except (TypeError, ValueError):
            raise ValueError(f"{who}: light must be two numbers (a, b), background and {', '.join(colors) or 'colours'} three each") from None
        for name, value in out.items():
            if len(value) != 3:
                raise ValueError(f"{who}: {name} must be three numbers, got {len(value)}")
        return (la, lb), out

    @torch.no_grad()
    def render_mesh(self, vertices, triangles, camera, vertex_colors=None, color=(0.7, 0.7, 0.7), light=(0.3, 0.7), background=(1.0, 1.0, 1.0),
                    bin_capacity=None, return_index: bool = False, return_depth: bool = False, record_bytes: Optional[int] = None,
                    vertex_normals=None):
        """Device version of vis_retarget.py's mesh images (:400-430, :497-512: a TriangleMesh per frame into open3d's off-screen
        visualiser): the triangles ``triangles`` (M,3) int32 over the posed ``vertices`` (F,V,3) float64 - sample_retarget's ``points``
        - drawn through ``camera`` (render.PinholeCamera), the nearest triangle winning each pixel (nm_mesh_bin + nm_mesh_draw,
        csrc/nm_mesh.hip).  **This is not open3d's image**: the result is defined by the contract of include/nm355.h alone
        (tests/mesh_ref.py restates it): a pixel is covered where its three edge functions in the projected vertices agree in sign
        (both faces are visible, triangles that share an edge leave no crack), a triangle with a vertex in front of ``camera.near``
        is culled WHOLE (no clipping), as are triangles with an index outside the vertices or a non-finite vertex; of equal depths the
        lower row wins.  The pixel is the perspective-correct mix of the winner's ``vertex_colors`` (V,3) float64 - or ``color`` without
        them - times light[0] + light[1] * |cos(face normal, ray)|, clamped to [0, 1] (NaN: 0) and truncated to uint8; light (1, 0)
        leaves the colours flat.  With ``vertex_normals`` (F,V,3) float64 - NeuralMarionette.vertex_normals' rows - the cosine is taken
        with the perspective-correct mix of the winner's three vertex normals instead (smooth shading, the script's ``smooth_imgs``): each
        group of frames draws index and depth, then nm_mesh_shade writes the image; index and depth are the flat call's, and a pixel
        whose mixed normal is zero or not finite keeps the flat shade.  None is the flat path, bit for bit as before.  Loop subdivision
        is NeuralMarionette.subdivide (render_retarget does both per group of frames); textures are the caller's.
        The records take 144 bytes per frame and triangle, so the frames are drawn in groups whose records stay under
        ``record_bytes`` (MESH_RECORD_BYTES = 512 MiB by default; a single frame past the bound is drawn alone).  The result does not
        depend on the grouping.
        Returns a dict: image (F,H,W,3) uint8; bin_total, a 0-d int64 device tensor - the (tile, triangle) list entries of all groups
        together; index (F,H,W) int32 [return_index]: the winner's row in triangles, -1 for background; depth (F,H,W) float64
        [return_depth]: its distance along the camera's z, +inf for background.
        bin_capacity=None reads each group's number of list entries - one synchronisation per group - and sizes its list exactly.
        With a bin_capacity, the capacity of a group's list, the call never synchronises; if a group needs more, nothing faults but the
        image is INCOMPLETE: bin_total <= bin_capacity afterwards rules that out.  No atomics touch an output: results are
        bit-identical from run to run."""
        who = "render_mesh"
        (light_a, light_b), num = self._render_numbers(who, camera, light, background, color=color)
        if bin_capacity is not None and int(bin_capacity) < 0:
            raise ValueError(f"{who}: bin_capacity must be >= 0, got {bin_capacity}")
        bound = MESH_RECORD_BYTES if record_bytes is None else int(record_bytes)
        if bound < 1:
            raise ValueError(f"{who}: record_bytes must be >= 1, got {record_bytes}")
        for name, t in (("vertices", vertices), ("triangles", triangles)) + ((("vertex_colors", vertex_colors),) if vertex_colors is not None else ()):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
        if vertices.dtype != torch.float64 or vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1:
            raise ValueError(f"{who}: vertices must be (F,V,3) float64 with F, V >= 1, got {tuple(vertices.shape)} {vertices.dtype}")
        F, V = int(vertices.shape[0]), int(vertices.shape[1])
        if triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
            raise ValueError(f"{who}: triangles must be (M,3) int32, got {tuple(triangles.shape)} {triangles.dtype}")
        M = int(triangles.shape[0])
        if vertex_colors is not None and (vertex_colors.dtype != torch.float64 or tuple(vertex_colors.shape) != (V, 3)):
            raise ValueError(f"{who}: vertex_colors must be ({V},3) float64, got {tuple(vertex_colors.shape)} {vertex_colors.dtype}")
        H, W = camera.height, camera.width
        if H * W >= 2 ** 31 or M >= 2 ** 31:
            raise ValueError(f"{who}: {W} x {H} pixels and {M} triangles, one frame indexes fewer than 2^31 of either")
        tensors = [("vertices", vertices), ("triangles", triangles)] + ([("vertex_colors", vertex_colors)] if vertex_colors is not None else [])
        if vertex_normals is not None:
            if not isinstance(vertex_normals, torch.Tensor) or vertex_normals.dtype != torch.float64 or tuple(vertex_normals.shape) != (F, V, 3):
                raise ValueError(f"{who}: vertex_normals must be a ({F},{V},3) float64 tensor, got "
                                 f"{(tuple(vertex_normals.shape), vertex_normals.dtype) if isinstance(vertex_normals, torch.Tensor) else type(vertex_normals).__name__}")
            tensors.append(("vertex_normals", vertex_normals))
        for name, t in tensors:
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be contiguous on the network's device, got {t.device}")
        eng = self._engine
        dev = eng._device()
        for name, t in tensors:
            if t.device != dev:
                raise ValueError(f"{who}: {name} must be on the network's device ({dev}), got {t.device}")
        eng.ready()
        cam = camera.c_struct()
        TX, TY = (W + 15) // 16, (H + 15) // 16
        group = max(1, min(F, bound // max(1, 144 * M), (2 ** 31 - 1) // (H * W), (2 ** 31 - 1) // max(1, M)))
        rec = torch.empty(group * M, 16, device=dev, dtype=torch.float64)
        rect = torch.empty(group * M, 4, device=dev, dtype=torch.int32)
        tile_offsets = torch.empty(group * TX * TY + 1, device=dev, dtype=torch.int64)
        out = dict(image=torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8), bin_total=torch.zeros((), device=dev, dtype=torch.int64))
        if return_index:
            out["index"] = torch.empty(F, H, W, device=dev, dtype=torch.int32)
        if return_depth:
            out["depth"] = torch.empty(F, H, W, device=dev, dtype=torch.float64)
        null = lambda t: t.data_ptr() if t is not None and t.numel() else None
        part = lambda t, f0: t[f0:].data_ptr() if t is not None else None
        lst = torch.empty(int(bin_capacity), device=dev, dtype=torch.int32) if bin_capacity is not None else None
        smooth = vertex_normals is not None
        index = out.get("index")
        if smooth and index is None:
            index = torch.empty(F, H, W, device=dev, dtype=torch.int32)     # the shade pass reads the winners
        for f0 in range(0, F, group):
            n = min(group, F - f0)
            last = tile_offsets[n * TX * TY]
            eng.call("nm_mesh_bin", vertices[f0:].data_ptr(), null(triangles), n, V, M, C.byref(cam), null(rec), null(rect), tile_offsets.data_ptr())
            if bin_capacity is None:
                lst = torch.empty(int(last.item()), device=dev, dtype=torch.int32)
            out["bin_total"] += last
            eng.call("nm_mesh_draw", null(rec), null(rect), tile_offsets.data_ptr(), null(triangles), null(vertex_colors), (C.c_double * 3)(*num["color"]),
                     n, V, M, C.byref(cam), light_a, light_b, (C.c_double * 3)(*num["background"]), int(lst.numel()), null(lst),
                     part(index, f0), part(out.get("depth"), f0), None if smooth else out["image"][f0:].data_ptr())
            if smooth:
                eng.call("nm_mesh_shade", null(rec), index[f0:].data_ptr(), null(triangles), vertex_normals[f0:].data_ptr() if M else None, null(vertex_colors),
                         (C.c_double * 3)(*num["color"]), n, V, M, C.byref(cam), light_a, light_b, (C.c_double * 3)(*num["background"]),
                         out["image"][f0:].data_ptr())
        return out

    @torch.no_grad()
    def render_skeleton(self, keypoints, parents, camera, threshold=0.2, radius=0.03, bone_radius=0.03, joint_colors=(0.7, 0.1, 0.0),
                        bone_color=(0.0, 0.6, 0.1), light=(0.3, 0.7), background=(1.0, 1.0, 1.0), over=None, return_index: bool = False,
                        return_depth: bool = False):
        """Device version of vis_retarget.py's skeleton images (:514-547: drawSphere per visible joint, drawCone1 + drawCone2 per bone
        into open3d's off-screen visualiser): ``keypoints`` (F,K,4) float32 (x, y, z, intensity; sample_retarget's (1,T,K,4) is taken
        as (T,K,4)) with ``parents`` (K), K <= 32, drawn through ``camera`` in one launch (nm_skeleton_draw, csrc/nm_mesh.hip).  **Not
        open3d's image**: the contract is include/nm355.h's (tests/mesh_ref.py restates it).  Joint k gets a sphere of ``radius`` iff
        clip(intensity_k, 0, 1) >= ``threshold``, and a bone to parents[k] iff both are visible, parents[k] != k and the bone is not of
        length 0; a bone is the script's double cone - two nappes sharing a base circle of ``bone_radius`` at a fifth of the bone from
        the parent, apexes at the parent and at the child (drawCone2's 0.195 margin and + 1e-6 are not reproduced).  Spheres and nappes
        are intersected analytically per pixel and shaded by light[0] + light[1] * |cos(surface normal, ray)|; spheres and bones that
        reach in front of ``camera.near`` are not drawn.  ``joint_colors``: one colour or (K,3); ``bone_color``: one colour.
        ``over`` (F,H,W,3) uint8: the skeleton is pasted over a COPY of it (the script's overlay :550, without its accident of treating
        white skeleton pixels as background); the input is not modified.  Without it uncovered pixels take ``background``.
        Returns a dict: image (F,H,W,3) uint8; index (F,H,W) int32 [return_index]: joint k's sphere is k, its bone K + k, -1 for
        background; depth (F,H,W) float64 [return_depth]."""
        who = "render_skeleton"
        flat = not (isinstance(joint_colors, (torch.Tensor, np.ndarray)) and joint_colors.ndim == 2) and not (
            isinstance(joint_colors, (list, tuple)) and len(joint_colors) and isinstance(joint_colors[0], (list, tuple)))
        (light_a, light_b), num = self._render_numbers(who, camera, light, background, bone_color=bone_color, **(dict(joint_colors=joint_colors) if flat else {}))
        try:
            threshold, radius, bone_radius = float(threshold), float(radius), float(bone_radius)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: threshold, radius and bone_radius must be numbers") from None
        for name, r in (("radius", radius), ("bone_radius", bone_radius)):
            if not (r > 0.0 and r < float("inf")):
                raise ValueError(f"{who}: {name} must be a finite number > 0, got {r}")
        if not isinstance(keypoints, torch.Tensor):
            raise ValueError(f"{who}: keypoints must be a tensor, got {type(keypoints).__name__}")
        if keypoints.dim() == 4 and keypoints.shape[0] == 1:
            keypoints = keypoints[0]
        if keypoints.dtype != torch.float32 or keypoints.dim() != 3 or keypoints.shape[2] != 4 or keypoints.shape[0] < 1 or not 1 <= keypoints.shape[1] <= 32:
            raise ValueError(f"{who}: keypoints must be (F,K,4) float32 with F >= 1 and 1 <= K <= 32, got {tuple(keypoints.shape)} {keypoints.dtype}")
        F, K = int(keypoints.shape[0]), int(keypoints.shape[1])
        par = torch.as_tensor(parents)
        if par.dim() != 1 or par.numel() != K or par.is_floating_point():
            raise ValueError(f"{who}: parents must be ({K}) integers, got {tuple(par.shape)} {par.dtype}")
        jc = None
        if not flat:
            jc = torch.as_tensor(joint_colors)
            if tuple(jc.shape) != (K, 3):
                raise ValueError(f"{who}: joint_colors must be one colour or ({K},3), got {tuple(jc.shape)}")
        H, W = camera.height, camera.width
        if F * H * W >= 2 ** 31:
            raise ValueError(f"{who}: {F} frames of {W} x {H} pixels, one call indexes fewer than 2^31")
        if over is not None and (not isinstance(over, torch.Tensor) or over.dtype != torch.uint8 or tuple(over.shape) != (F, H, W, 3)):
            raise ValueError(f"{who}: over must be ({F},{H},{W},3) uint8, got {tuple(over.shape) if isinstance(over, torch.Tensor) else type(over).__name__}")
        if not keypoints.is_cuda or (over is not None and not over.is_cuda):
            raise ValueError(f"{who}: keypoints and over must be on the network's device, got {keypoints.device}")
        eng = self._engine
        dev = eng._device()
        if keypoints.device != dev or (over is not None and over.device != dev):
            raise ValueError(f"{who}: keypoints and over must be on the network's device ({dev}), got {keypoints.device}")
        eng.ready()
        keypoints = keypoints.contiguous()
        par = par.to(device=dev, dtype=torch.int32).contiguous()
        if jc is not None:
            jc = jc.to(device=dev, dtype=torch.float64).contiguous()
        out = dict(image=over.clone(memory_format=torch.contiguous_format) if over is not None else torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8))
        if return_index:
            out["index"] = torch.empty(F, H, W, device=dev, dtype=torch.int32)
        if return_depth:
            out["depth"] = torch.empty(F, H, W, device=dev, dtype=torch.float64)
        cam = camera.c_struct()
        raw = lambda t: t.data_ptr() if t is not None else None
        eng.call("nm_skeleton_draw", keypoints.data_ptr(), par.data_ptr(), F, K, C.byref(cam), threshold, radius, bone_radius, raw(jc),
                 (C.c_double * 3)(*num["joint_colors"]) if flat else None, (C.c_double * 3)(*num["bone_color"]), light_a, light_b,
                 (C.c_double * 3)(*num["background"]), int(over is not None), raw(out.get("index")), raw(out.get("depth")), out["image"].data_ptr())
        return out

    @torch.no_grad()
    def render_retarget(self, result, triangles, camera, skin_colors: bool = False, joint_colors=None, parents=None, threshold=0.2, radius=0.03,
                        bone_radius=0.03, color=(0.7, 0.7, 0.7), joint_color=(0.7, 0.1, 0.0), bone_color=(0.0, 0.6, 0.1), light=(0.3, 0.7),
                        background=(1.0, 1.0, 1.0), record_bytes: Optional[int] = None, subdivide: int = 0, smooth: bool = False, plan=None):
        """vis_retarget.py's loop :497-553 from sample_retarget's dict ``result``: per frame the posed mesh (``triangles`` (M,3) int32 over
        result['points']), the skeleton of the retargeted keypoints, the skeleton of the source keypoints, and the first pasted over
        the mesh - render_mesh and render_skeleton, which see.  ``parents`` defaults to the learner's tree as sample_retarget left it.
        skin_colors=True colours the mesh as :415 does, vertex_colors = skin_weights @ joint_colors with ``joint_colors`` (K,3) - a
        torch matmul on the device; the spheres take ``joint_color`` either way, as in the script's loop.
        ``subdivide`` = n > 0 is the script's ``subdivide_loop(arg.subdivide_iter)`` (:418, :507; 3 there): the points - and the skin
        colours, as :416-423 - go through n Loop subdivisions (NeuralMarionette.subdivide) by ``plan``, or by a LoopPlan built here from
        ``triangles`` (host work and one copy of the triangles to the host: pass a plan to call this more than once per mesh; a plan's
        levels must equal ``subdivide``).  ``smooth`` = True is its ``compute_vertex_normals()`` (:421, :510): the mesh and the overlay are
        shaded with NeuralMarionette.vertex_normals of the (subdivided) mesh, render_mesh's ``vertex_normals``.  Both work on groups of
        frames whose fine points and normals stay under SUBDIV_BYTES, so the fine mesh of all frames never exists at once; the result
        does not depend on the grouping and equals composing the four calls by hand.  The defaults are the unsubdivided, flat-shaded
        images, bit for bit as before.
        Returns a dict of (T,H,W,3) uint8 images: mesh, skeleton, source_skeleton, overlay."""
        who = "render_retarget"
        if not isinstance(result, dict) or any(k not in result for k in ("points", "keypoints", "source_keypoints", "skin_weights")):
            raise ValueError(f"{who}: result must be sample_retarget's dict with 'points', 'keypoints', 'source_keypoints' and 'skin_weights'")
        vc = None
        if skin_colors:
            if joint_colors is None:
                raise ValueError(f"{who}: skin_colors needs joint_colors (K,3)")
            w = result["skin_weights"]
            jc = torch.as_tensor(joint_colors)
            if jc.dim() != 2 or tuple(jc.shape) != (int(w.shape[1]), 3):
                raise ValueError(f"{who}: joint_colors must be ({int(w.shape[1])},3), got {tuple(jc.shape)}")
            vc = (w.double() @ jc.to(device=w.device, dtype=torch.float64)).contiguous()
        if parents is None:
            parents = self.dyna_module.parents
            if parents is None:
                raise ValueError(f"{who}: the learner has no tree yet: pass parents (K)")
        common = dict(light=light, background=background)
        levels = int(subdivide)
        if levels < 0:
            raise ValueError(f"{who}: subdivide must be >= 0, got {subdivide}")
        if levels == 0 and not smooth:
            mesh = self.render_mesh(result["points"], triangles, camera, vertex_colors=vc, color=color, record_bytes=record_bytes, **common)["image"]
        else:
            points = result["points"]
            if not isinstance(points, torch.Tensor) or points.dim() != 3:
                raise ValueError(f"{who}: result['points'] must be a (T,N,3) tensor")
            if plan is None:
                plan = LoopPlan.build(triangles, int(points.shape[1]), levels, device=points.device)
            elif not isinstance(plan, LoopPlan) or plan.levels != levels or plan.V != int(points.shape[1]):
                raise ValueError(f"{who}: plan must be a LoopPlan of {levels} levels over {int(points.shape[1])} vertices")
            if vc is not None:
                vc = self.subdivide(vc, plan)
            T = int(points.shape[0])
            per_frame = 24 * (plan.vertex_counts[-1] * (2 if smooth else 1) + sum(plan.vertex_counts[1:-1]))
            group = max(1, min(T, SUBDIV_BYTES // per_frame))
            parts = []
            for f0 in range(0, T, group):
                fine = self.subdivide(points[f0:f0 + group], plan)
                normals = self.vertex_normals(fine, plan) if smooth else None
                parts.append(self.render_mesh(fine, plan.triangles, camera, vertex_colors=vc, color=color, record_bytes=record_bytes, vertex_normals=normals,
                                              **common)["image"])
            mesh = parts[0] if len(parts) == 1 else torch.cat(parts)
        skel = dict(threshold=threshold, radius=radius, bone_radius=bone_radius, joint_colors=joint_color, bone_color=bone_color, **common)
        drawn = self.render_skeleton(result["keypoints"], parents, camera, return_index=True, **skel)
        skeleton = drawn["image"]
        source = self.render_skeleton(result["source_keypoints"], parents, camera, **skel)["image"]
        overlay = torch.where((drawn["index"] >= 0)[..., None], skeleton, mesh)     # render_skeleton(over=mesh) without a second launch
        return dict(mesh=mesh, skeleton=skeleton, source_skeleton=source, overlay=overlay)

    def _points(self, who, vox, return_points):
        """the drivers' ``return_points``: True - occupied_points(vox, 0.5, return_depth=True); "surface" - surface_points(vox, 0.5)"""
        if not isinstance(return_points, str):
            return self.occupied_points(vox, 0.5, return_depth=True)
        if return_points == "surface":
            return self.surface_points(vox, 0.5)
        raise ValueError(f'{who}: return_points must be False, True or "surface", got {return_points!r}')

    # -- sampling drivers: the rollout loops of the reference's demo scripts as methods ------------
    @torch.no_grad()
    def sample_generation(self, cond_voxel, Tgen=25, sample_num=3, eps_post=None, eps_prior=None, return_points=False):
        """vis_generation.py:81-136: condition on ``cond_voxel`` (Tcond,1,G,G,G) with best-of-``sample_num``
        posterior steps, then roll ``sample_num`` independent prior trajectories for ``Tgen`` steps and decode each.
        eps_post (Tcond,sample_num,Z) / eps_prior (Tgen,sample_num,Z) inject the noise.
        Returns keypoints_cond (1,Tcond,K,4) [the detected keypoints, as the script records], keypoints_gen
        (1,Tgen,sample_num,K,4) and voxels (sample_num,Tcond+Tgen,1,G,G,G) binarised at 0.5.  return_points: also ``points``, the
        script's next lines (:137-170) on the device - occupied_points(voxels_raw, 0.5, return_depth=True), a clip per sample;
        return_points="surface": surface_points(voxels_raw, 0.5) instead, with the normals and plate frames of :157-171."""
        _need_graph(self._engine.opts, "NeuralMarionette.sample_generation")
        d = self.dyna_module
        S, K, Z = int(sample_num), d.nkeypoints, d.nlatent_kypt
        det = self.kypt_detector(cond_voxel[None])
        kp = det["keypoints"]
        Tc = int(kp.shape[1])
        dev = kp.device
        d._ensure_tree(det["affinity"], self._engine.ready())
        e_post = _f32(eps_post, dev) if eps_post is not None else torch.randn(Tc, S, Z, device=dev)
        e_prior = _f32(eps_prior, dev) if eps_prior is not None else torch.randn(Tgen, S, Z, device=dev)
        h = d.init_kypt_rnn_state.detach()
        offset = d.get_offset(kp)
        cond = []
        for t in range(Tc):
            _, _, h = d.step(h, offset, e_post[t][:, None], keypoints_obs=kp[:, t], SAMPLE_NUM=S)
            cond.append(kp[0, t])
        h = h.expand(S, -1).contiguous()
        off = offset.expand(S, -1, -1, -1).contiguous()
        gen_k = d.rollout(h, off, e_prior)[0].transpose(0, 1)[None]          # (1, Tgen, S, K, 4)
        cond_k = torch.stack(cond, 0)[None]
        full = torch.cat([cond_k.expand(S, -1, -1, -1), gen_k[0].transpose(0, 1)], dim=1).contiguous()
        ff = det["first_feature"].expand(S, -1, -1, -1, -1).contiguous()
        fr = cond_voxel[None, 0].to(dev).expand(S, -1, -1, -1, -1).contiguous()
        vox = self.kypt_detector.decode_from_dyna(full, ff, fr)["gen"]
        out = dict(keypoints_cond=cond_k, keypoints_gen=gen_k, voxels=(vox >= 0.5).float(), voxels_raw=vox)
        if return_points:
            out["points"] = self._points("sample_generation", vox, return_points)
        return out

    @torch.no_grad()
    def sample_interpolation(self, target_voxel, sample_rate=10, sample_num=10000, eps_a=None, eps_b=None, force_picks=None,
                             return_points=False):
        """vis_interpolation.py:80-143: key frames every ``sample_rate`` steps (and the last one) are matched with a
        posterior sample, the frames in between come from the prior trajectory (out of ``sample_num``) that lands
        nearest the next key frame.  eps_a (T,sample_num,Z): the step's first draw (posterior at key frames, prior
        otherwise); eps_b (T,sample_num,Z): the second (prior, 'for choosing') draw at key frames.
        ``force_picks`` (list of (i1, i2) per key frame) replaces the two nearest-row selections (teacher forcing in tests).
        Returns keypoints (1,T,K,4), voxels (T,1,G,G,G) binarised at 0.5, and the selected row per key frame.  return_points: also
        ``points``, the script's next lines (:141-177) on the device - occupied_points(voxels_raw, 0.5, return_depth=True);
        return_points="surface": surface_points(voxels_raw, 0.5) instead, with the normals and plate frames of :160-177."""
        _need_graph(self._engine.opts, "NeuralMarionette.sample_interpolation")
        d = self.dyna_module
        S, K, Z = int(sample_num), d.nkeypoints, d.nlatent_kypt
        det = self.kypt_detector(target_voxel[None])
        kp = det["keypoints"]
        T = int(kp.shape[1])
        dev = kp.device
        d._ensure_tree(det["affinity"], self._engine.ready())
        ea = _f32(eps_a, dev) if eps_a is not None else torch.randn(T, S, Z, device=dev)
        eb = _f32(eps_b, dev) if eps_b is not None else torch.randn(T, S, Z, device=dev)
        h = d.init_kypt_rnn_state.detach().expand(S, -1).contiguous()
        off = d.get_offset(kp).expand(S, -1, -1, -1).contiguous()
        selected, pending, picks = [], [], []
        for t in range(T):
            obs = kp[:, t].reshape(1, -1)
            if t % sample_rate == 0 or t == T - 1:
                obs_rows = obs.expand(S, -1).contiguous()
                kp_post, z_post, _ = d.step(h, off, ea[t][None], keypoints_obs=obs_rows, SAMPLE_NUM=1, update_state=False)
                kp_pri, _, _ = d.step(h, off, eb[t], update_state=False)
                if force_picks is None:
                    i1 = d.nearest_row(kp_post, obs)
                    i2 = d.nearest_row(kp_pri, kp_post[i1])
                else:
                    i1, i2 = (int(v) for v in force_picks[len(picks)])
                pending.append(obs_rows)
                selected += [s[i2].view(K, 4) for s in pending]
                pending = []
                picks.append((i1, i2))
                h1 = d.kypt_rnn_cell(torch.cat([kp_post[i1], z_post[i1]])[None], h[i1][None])
                h = h1.expand(S, -1).contiguous()
            else:
                kps, _, h = d.step(h, off, ea[t])
                pending.append(kps)
        sel = torch.stack(selected, 0)[None].clone()
        sel[0, :, :, -1] = sel[0, 0, :, -1]
        vox = self.kypt_detector.decode_from_dyna(sel, det["first_feature"], target_voxel[None, 0].to(dev))["gen"][0]
        out = dict(keypoints=sel, voxels=(vox >= 0.5).float(), voxels_raw=vox, picks=picks)
        if return_points:
            out["points"] = self._points("sample_interpolation", vox.contiguous(), return_points)
        return out

    @torch.no_grad()
    def sample_retarget(self, source_voxel, target_voxel, target_points, hardness=8.0, threshold=0.2, eps_source=None, eps_target=None,
                        force_nearest=None):
        """vis_retarget.py:236-322 (its 'ours' branch, the one the script takes): the motion of ``source_voxel`` (T,1,G,G,G) carried over to
        the shape ``target_voxel`` (1,G,G,G) whose points ``target_points`` (N,3) are skinned to the skeleton.  Detector on the source
        clip, every frame's intensity replaced by frame 0's, encode (best-of-10, noise eps_source (T,10,1,Z)) -> R; detector on the
        target frame, its keypoints take the source's frame-0 intensities, encode (eps_target (1,10,1,Z)) -> R_bind; get_offset of the
        target; bind (skin_weights); forward kinematics with the source's root trajectory; pose.  ``force_nearest`` (N) replaces the
        nearest-bone selection (teacher forcing in tests).  Mesh loading and rendering are the caller's.
        Returns source_keypoints (1,T,K,4), target_keypoints (1,1,K,4), R (T,K,3,3), R_bind (K,3,3), offset (1,K,3,1), keypoints
        (1,T,K,4) [retargeted], skin_weights (N,K), nearest (N), nearest_margin (N) and points (T,N,3) float64."""
        _need_graph(self._engine.opts, "NeuralMarionette.sample_retarget")
        d = self.dyna_module
        G, K, Z, S = self._engine.opts.grid_size, d.nkeypoints, d.nlatent_kypt, 10
        if source_voxel.dim() != 5 or tuple(source_voxel.shape[1:]) != (1, G, G, G) or source_voxel.shape[0] < 1:
            raise ValueError(f"source_voxel must be (T,1,{G},{G},{G}) with T >= 1, got {tuple(source_voxel.shape)}")
        T = int(source_voxel.shape[0])
        if tuple(target_voxel.shape) != (1, G, G, G):
            raise ValueError(f"target_voxel must be (1,{G},{G},{G}), got {tuple(target_voxel.shape)}")
        if target_points.dim() != 2 or target_points.shape[1] != 3 or target_points.shape[0] < 1:
            raise ValueError(f"target_points must be (N,3) with N >= 1, got {tuple(target_points.shape)}")
        N = int(target_points.shape[0])
        for name, e, want in (("eps_source", eps_source, (T, S, 1, Z)), ("eps_target", eps_target, (1, S, 1, Z))):
            if e is not None and tuple(e.shape) != want:
                raise ValueError(f"{name} must be {want}, got {tuple(e.shape)}")
        if force_nearest is not None and tuple(force_nearest.shape) != (N,):
            raise ValueError(f"force_nearest must be ({N},), got {tuple(force_nearest.shape)}")
        det = self.kypt_detector.detect(source_voxel[None])
        if det["affinity"] is None:
            raise _lib.NmError("NeuralMarionette.sample_retarget: the detector returns no affinity yet - call anneal() first (vis_retarget.py:237)")
        src = det["keypoints"].clone()
        src[..., 3] = src[:, :1, :, 3].clone()                        # every frame carries frame 0's intensities (vis_retarget.py:242)
        R = d.encode(src, det["affinity"], SAMPLE_NUM=S, eps=eps_source)["R"][0]
        tgt = self.kypt_detector.detect(target_voxel[None, None])["keypoints"]
        tgt = tgt.clone()
        tgt[..., 3] = src[:, :1, :, 3]                              # the target's joints take the source's frame-0 intensities (:260)
        R_bind = d.encode(tgt, det["affinity"], SAMPLE_NUM=S, eps=eps_target)["R"][0, 0]
        offset = d.get_offset(tgt)
        bind = d.skin_weights(target_points, tgt[0, 0], R_bind, hardness=hardness, threshold=threshold, force_child=force_nearest)
        root = int(d.priority.indices[0])
        pos = d.retarget_fk(R, src[0, :, root, :3], offset[0])
        new_kp = torch.cat([pos[None], src[..., 3:]], dim=-1)
        points = d.retarget_pose(bind, R, pos)
        return dict(source_keypoints=src, target_keypoints=tgt, R=R, R_bind=R_bind, offset=offset, keypoints=new_kp,
                    skin_weights=bind["dense"], nearest=bind["child"], nearest_margin=bind["margin"], points=points)

    def control_active(self, module_actives):
        """neural_marionette.py:22-32."""
        for name in self.current_actives:
            if self.current_actives[name] != module_actives[name]:
                module = self.kypt_detector if name == "detector" else self.dyna_module
                for p in module.parameters():
                    p.requires_grad = module_actives[name]
                self.current_actives[name] = module_actives[name]

    def forward(self, vox_seq, module_actives=None, eps=None, detector_outputs="all"):
        """neural_marionette.py:34-56.  ``eps`` optionally injects the VRNN noise (T,S,B,Z).  detector_outputs="keypoints" (learner
        regime only, detector inactive): the frozen detector runs without its voxel decoder and losses (KyptDetector.detect) - the log
        then lacks 'recon' and the eleven detector losses, which the learner's loss does not read."""
        log: Dict[str, torch.Tensor] = dict()
        keypoints = affinity = None
        d, det_m = self.dyna_module, self.kypt_detector
        if module_actives["learner"]:
            _need_graph(self._engine.opts, "NeuralMarionette.forward (learner)")
        if module_actives["learner"] and d.A is not None and det_m.affinity_start and not \
                (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return self._forward_fused(vox_seq, eps)
        if module_actives["detector"] or module_actives["learner"]:
            if module_actives["detector"]:
                det = self.kypt_detector(vox_seq)
            elif detector_outputs == "keypoints":
                det = self.kypt_detector.detect(vox_seq)
            else:
                with torch.no_grad():           # neural_marionette.py:45-47
                    det = self.kypt_detector(vox_seq)
            keypoints, affinity = det["keypoints"], det.get("affinity")
            log.update(det)
        if module_actives["learner"]:
            log.update(self.dyna_module.encode(keypoints.detach(), affinity.detach(), eps=eps))
        return log

    def _forward_fused(self, vox_seq, eps, SAMPLE_NUM=10):
        """Detector + VRNN encode in one library call (nm_forward_fused): same outputs as the two-call path; the VRNN
        runs on a side stream beside the decoder.  Used once the skeleton tree is cached."""
        eng = self._engine
        ctx = eng.ready()
        dev = ctx.device
        d, dm = self.kypt_detector, self.dyna_module
        dm._ensure_tree(None, ctx)
        B, T = int(vox_seq.shape[0]), int(vox_seq.shape[1])
        G, K, g, Z, H, S = d.grid_size, d.nkeypoints, d.grid_size // 4, dm.nlatent_kypt, dm.nhidden_kypt, int(SAMPLE_NUM)
        if tuple(vox_seq.shape[2:]) != (1, G, G, G):
            raise ValueError(f"expected seq of shape (B,T,1,{G},{G},{G}), got {tuple(vox_seq.shape)}")
        vox = _f32(vox_seq, dev)
        e = dm._eps(T, (S, B, Z), dev, eps)
        kp = torch.empty(B, T, K, 4, device=dev); hm = torch.empty(B, T, K, g, g, g, device=dev)
        ff = torch.empty(B, FEAT_DIM, g, g, g, device=dev); recon = torch.empty(B, T, 1, G, G, G, device=dev)
        aff = torch.empty(d.nneighbor, K, K, 1, device=dev)
        losses = torch.empty(len(DETECTOR_LOSS_KEYS), device=dev)
        rec = torch.empty(B, T, K, 4, device=dev); R = torch.empty(B, T, K, 3, 3, device=dev)
        z = torch.empty(B, T, Z, device=dev); h = torch.empty(B, T + 1, H, device=dev)
        sc = torch.empty(2, device=dev); best = torch.empty(B, T, device=dev, dtype=torch.int32)
        eng.call_conv("nm_forward_fused", _lib.ptr(vox), B, T, 1, _lib.ptr(e), S, _lib.ptr(kp), _lib.ptr(hm), _lib.ptr(ff),
                 _lib.ptr(recon), _lib.ptr(aff), _lib.ptr(losses), _lib.ptr(rec), _lib.ptr(R), _lib.ptr(z), _lib.ptr(h),
                 _lib.ptr(sc), _lib.ptr(best))
        log = dict(recon=recon, keypoints=kp, heatmaps=hm, affinity=aff)
        for i, name in enumerate(DETECTOR_LOSS_KEYS):
            log[name] = losses[i]
        log["first_feature"] = ff
        log.update(kypt_recon=rec, R=R, z_kypts=z, h_kypts=h, kl_kypt=sc[0], kypt_recon_loss=sc[1],
                   gae_recon_loss=torch.zeros((), dtype=torch.int64, device=dev), topo_recon_loss=torch.zeros((), dtype=torch.int64, device=dev), best_idx=best)
        return log

    def generate(self, vox_seq, module_actives=None, eps_post=None, eps_prior=None, return_points=False):
        """neural_marionette.py:58-103 ('dl' transition).  return_points: also ``points`` = occupied_points(gen, 0.5, return_depth=True),
        what the reference's plotting does with ``gen`` on the host; return_points="surface": surface_points(gen, 0.5) instead, with the
        normals and plate frames the demo scripts compute per frame."""
        if module_actives["learner"]:
            _need_graph(self._engine.opts, "NeuralMarionette.generate")
        B, T = vox_seq.shape[:2]
        assert self.Tcond < T
        log = dict()
        if module_actives["learner"]:
            det = self.kypt_detector(vox_seq[:, :self.Tcond].contiguous())
            keypoints = det["keypoints"]
            dyn = self.dyna_module.generate(keypoints, det.get("affinity"), Ttot=T, Tcond=self.Tcond,
                                            eps_post=eps_post, eps_prior=eps_prior)
            gen = self.kypt_detector.decode_from_dyna(dyn["keypoints_gen"], det["first_feature"], vox_seq[:, 0])["gen"]
            log.update(gen=torch.cat([det["recon"][:, :self.Tcond], gen], dim=1),
                       keypoints=torch.cat([keypoints[:, :self.Tcond], dyn["keypoints_gen"]], dim=1),
                       A_hats=None)
            if return_points:
                log["points"] = self._points("generate", log["gen"], return_points)
        return log
