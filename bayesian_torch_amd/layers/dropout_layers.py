"""Monte-Carlo dropout (Gal & Ghahramani 2016) on BTX-RNG v1 — BTX-DROP v1, DESIGN.md §25.

`MCDropout` is `nn.Dropout` whose mask is a pure function of (seed, MC sample index, layer id, element index): sample s is the
same draw on every rank, in an eager forward, as lane l of `mc_forward(lanes=k)` and in a replay of `mc.GraphedMC` /
`autograd.GraphedTrainStep`, whose kernels read the sample index from the device word the graphs rewrite.  CUDA tensors (f32 /
bf16) run csrc/btx_drop.hip; CPU tensors, backend "torch" and other dtypes build the SAME mask from torch integer ops
(functional.dropout_mask_aten).  `Dropout` is the reference's tuple-passing wrapper (`bayesian_torch/layers/dropout.py`).
"""
import torch
import torch.nn as nn

from .. import _lib
from .. import functional as BF
from .. import rng as _rng

__all__ = ["MCDropout", "MCDropout1d", "MCDropout2d", "MCDropout3d", "Dropout"]


class MCDropout(nn.Module):
    """out = x * scale where kept, +0.0 where dropped (by selection: a dropped inf / NaN gives 0, where torch multiplies by zero).
    The keep probability is quantised to T / 65536, T = round((1 - p) * 65536) (`keep_prob`, shown by repr); scale = f32(65536 / T).
    mode "element": one decision per element, indexed by its position in the channels-last order of the logical tensor (rank <= 3:
    plain row-major), so NCHW-contiguous and channels-last memory draw the same mask.  mode "channel" (nn.Dropout1d/2d/3d): one
    decision per (example, channel); the input rank must be >= 3.
    always_on=True (the MC-dropout default): active in eval() mode too, which is where mc.evaluate / mc_forward run; always_on=False
    follows `self.training` like nn.Dropout.  inplace=True is accepted and runs OUT of place (the backward regenerates the mask and
    needs nothing saved, so there is no memory to gain).  No parameters, no buffers: state_dict() is empty; kl_loss() is 0."""

    _btx_dropout = True  # what fuse_model (a leaf, nothing folded across it) and the INT8 conversions (refused) look for
    _mode = "element"

    def __init__(self, p=0.5, mode=None, always_on=True, inplace=False):
        super().__init__()
        self.p = float(p)
        self._btx_T, self._btx_scale = BF.dropout_params(p)
        self.mode = self._mode if mode is None else mode
        if self.mode not in BF.DROP_MODES:
            raise ValueError("mode must be 'element' or 'channel' (got %r)" % (mode,))
        self.always_on, self.inplace = bool(always_on), bool(inplace)
        self._btx_layer_id = _rng.next_layer_id()
        self._btx_sample = 0

    @property
    def keep_prob(self):
        return self._btx_T / 65536.0

    def extra_repr(self):
        return "p={}, keep={:.6f} ({}/65536), mode={}{}".format(self.p, self.keep_prob, self._btx_T, self.mode,
                                                                "" if self.always_on else ", always_on=False")

    def __deepcopy__(self, memo):
        """a copy draws its OWN masks: a fresh BTX-RNG layer id, as for the variational layers"""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        new.__dict__["_btx_layer_id"] = _rng.next_layer_id()
        for k in ("_btx_pre", "_btx_sample_dev", "_btx_lanes", "_btx_lane_batch", "_btx_static_x"):
            new.__dict__.pop(k, None)
        return new

    def kl_loss(self):
        return torch.zeros(())

    def _active(self):
        return self.training or self.always_on

    def _use_hip(self, x):
        from . import base_variational_layer as _base
        if _base._BACKEND == "hip" and not x.is_cuda:
            raise _lib.BtxError("backend 'hip' needs CUDA (ROCm) tensors")
        return x.is_cuda and _base._BACKEND != "torch" and x.dtype in (torch.float32, torch.bfloat16)

    def forward(self, x):
        if not self._active():
            return x
        if not x.is_floating_point():
            raise _lib.BtxError("%s needs a floating-point input (got %s)" % (type(self).__name__, x.dtype))
        d = self.__dict__
        lanes, lane_batch = d.get("_btx_lanes", 1), d.get("_btx_lane_batch")
        sdev = d.get("_btx_sample_dev")
        needs_grad = torch.is_grad_enabled() and x.requires_grad
        if lanes > 1 and needs_grad:
            raise _lib.BtxError("MC sample lanes are an inference feature: clear them before a training step")
        s_idx = self._btx_sample
        d["_btx_sample"] = s_idx + lanes  # the host counter advances like the other layers'; a pinned device word wins in the kernel
        T, scale, seed = self._btx_T, self._btx_scale, _rng.seed()
        if not self._use_hip(x):
            return BF.dropout_aten(x, T, scale, self.mode, seed, s_idx, self._btx_layer_id, sample_dev=sdev, lanes=lanes,
                                   lane_batch=lane_batch)
        if needs_grad:
            from .. import autograd as _ag
            return _ag.DropoutFn.apply(self, s_idx, x)
        return BF.dropout_hip(x, T, scale, self.mode, seed, s_idx, self._btx_layer_id, sample_dev=sdev, lanes=lanes,
                              lane_batch=lane_batch)

    def materialize_mask(self, shape, sample_idx, sample_dev=None, device="cpu"):
        """The bool KEEP mask BTX-DROP v1 defines for MC sample `sample_idx` (or the value of the device word `sample_dev`, read on
        the host) and one lane's logical tensor of `shape`; out = where(mask, x * scale, 0)."""
        if sample_dev is not None:
            sample_idx = int(sample_dev.reshape(-1)[0])
        return BF.dropout_mask_aten(tuple(shape), self._btx_T, self.mode, _rng.seed(), sample_idx, self._btx_layer_id, device)


class MCDropout1d(MCDropout):
    """nn.Dropout1d: whole channels of [N, C, L] inputs"""
    _mode = "channel"

    def __init__(self, p=0.5, always_on=True, inplace=False):
        super().__init__(p, "channel", always_on, inplace)


class MCDropout2d(MCDropout1d):
    """nn.Dropout2d: whole channels of [N, C, H, W] inputs"""


class MCDropout3d(MCDropout1d):
    """nn.Dropout3d: whole channels of [N, C, D, H, W] inputs"""


class Dropout(MCDropout):
    """the reference's wrapper (layers/dropout.py): takes the (x, kl) tuple of a variational layer, returns (dropout(x), 0); active
    in training mode only, like the reference's"""

    def __init__(self, p=0.5, inplace=False):
        super().__init__(p, "element", always_on=False, inplace=inplace)

    def forward(self, input):
        return super().forward(input[0]), 0
