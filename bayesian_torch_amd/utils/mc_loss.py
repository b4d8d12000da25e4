"""utils.mc_loss — the loss head of a training step with num_mc > 1 Monte-Carlo samples (reference
examples/main_bayesian_cifar.py:363-372: `output = mean(stack(output_)); loss = CE(output, y) + kl / bs`).

    stack = autograd.mc_train_forward(model, x, num_mc, step)       # [num_mc, B, C], carries gradient
    loss = mc_elbo_loss(stack, y, kl=get_kl_loss(model))            # or MCCrossEntropy()(stack, y, kl)

Two reductions over the sample axis:
  * reduce="logits" (default): CE(mean_s logits_s, y) — what the reference's scripts compute; every sample gets the same gradient
  * reduce="loss":             mean_s CE(logits_s, y) — the unbiased estimate of the expected log-likelihood; the gradient
                               differs per sample
and  loss = ce + kl / B  when a KL term is given (a 0-d / 1-element tensor, or a number).  label_smoothing as in F.cross_entropy.

CUDA stacks [S, B, C] in f32 / bf16 with int64 labels, 1 <= S <= 32 and C <= mc.MC_MAX_CLASSES run libbtx.so (btx_mc_ce_fwd /
btx_mc_ce_bwd: two launches forward, one backward, f32 arithmetic, bit-reproducible, no host read — capturable inside
autograd.GraphedTrainStep(num_mc=...), whose default loss this is).  CPU tensors, set_backend("torch") and everything else run the
ATen chain `_mc_ce_chain` on the tensor's own device.  An S = 1 stack gives the loss and gradient of the 2-D case.

Regression (BTX-REG v1): `mc_gaussian_nll(stack [S, B, W], target [B, D], kl)` / `MCGaussianNLL` are the same head for a
model that predicts real values.  variance="log": W = 2 D, columns [0, D) the mean m and [D, 2 D) the log-variance s (Kendall & Gal);
variance=None: W = D and s = log(noise_var), a constant without gradient.  (A LEARNABLE homoscedastic log-variance is user code:
`torch.cat([m, lv.expand_as(m)], -1)` with `lv` an nn.Parameter of shape [D], fed to the variance="log" head.)
  * reduce="loss" (default):  the ELBO estimate  sum_{s,b,d} 0.5 (s + (y - m)^2 exp(-s)) / (S B)  (+ 0.5 log(2 pi) D with full=True)
  * reduce="moments":         the NLL of the moment-matched predictive, the analogue of reduce="logits":  mbar = mean_s m_s,
                              vbar = mean_s exp(s_s) + mean_s (m_s - mbar)^2,  sum_{b,d} 0.5 (log vbar + (y - mbar)^2 / vbar) / B
and  loss = nll + kl / B.  CUDA stacks in f32 / bf16 with float32 targets and 1 <= S <= 32 run libbtx.so (btx_mc_gnll_fwd / _bwd: two
launches forward, one backward, f32 per element, float64 sums of a fixed shape, no host read: capturable as
GraphedTrainStep(loss_fn=...)); everything else runs the ATen chain `_mc_gnll_chain`.  Targets are finite; NaN propagates as in torch.
"""
import math

import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib
from . import _calibration as _c

MAX_SAMPLES = 32  # BTX_MCLOSS_MAX_S
_REDUCE = {"logits": 0, "loss": 1}


def _check(stack, target, reduce, label_smoothing):
    if reduce not in _REDUCE:
        raise ValueError("reduce must be 'logits' or 'loss', got %r" % (reduce,))
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError("label_smoothing must lie in [0, 1)")
    if stack.dim() != 3:
        raise ValueError("stack must be Monte-Carlo stacked logits [S, batch, classes] (S = 1 for one sample)")
    if target.numel() != stack.shape[1]:
        raise ValueError("target must hold one class index per batch row of the stack")


def _mc_ce_chain(stack, target, kl=None, reduce="logits", label_smoothing=0.0):
    """the vectorised ATen chain (0-d loss); in float64 it is the oracle of the tests.  Half / bf16 stacks are evaluated in f32."""
    _check(stack, target, reduce, label_smoothing)
    S, B, C = stack.shape
    z = stack if stack.dtype in (torch.float32, torch.float64) else stack.float()
    target = target.reshape(-1)
    if reduce == "logits":
        ce = F.cross_entropy(z.mean(0), target, label_smoothing=float(label_smoothing))
    else:
        ce = F.cross_entropy(z.reshape(S * B, C), target.repeat(S), label_smoothing=float(label_smoothing))
    if kl is None:
        return ce
    if torch.is_tensor(kl):
        kl = kl.reshape(())
    return ce + kl / B


class McCeFn(torch.autograd.Function):
    """0-d f32 loss of a [S, B, C] f32 / bf16 CUDA stack through btx_mc_ce_fwd; `kl`: a 1-element f32 tensor on the stack's device
    or None; its gradient g / B is returned here, so get_kl_loss(model) keeps its own backward (autograd.KlFn)."""

    @staticmethod
    def forward(ctx, stack, target, kl, reduce, label_smoothing):
        lg = stack.contiguous()
        lb = target.reshape(-1).contiguous()
        S, B, C = lg.shape
        L = _lib.lib()
        ws = torch.empty(L.btx_mcloss_workspace_bytes(S, B) // 4, dtype=torch.float32, device=lg.device)
        out = torch.empty(1, dtype=torch.float32, device=lg.device)
        act = _lib.ACT_BF16 if lg.dtype == torch.bfloat16 else _lib.ACT_F32
        klp = kl.detach().reshape(1).contiguous() if kl is not None else None
        _lib.check(L.btx_mc_ce_fwd(lg.data_ptr(), lb.data_ptr(), S, B, C, act, reduce, float(label_smoothing), _c._ptr(klp), 1.0 / B,
                                   out.data_ptr(), ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream(lg.device).cuda_stream))
        ctx.save_for_backward(lg, lb, ws)
        ctx.cfg = (act, reduce, float(label_smoothing), None if kl is None else tuple(kl.shape))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lg, lb, ws = ctx.saved_tensors
        act, reduce, ls, kl_shape = ctx.cfg
        S, B, C = lg.shape
        g = g.float().reshape(1).contiguous()
        dl = None
        if ctx.needs_input_grad[0]:
            dl = torch.empty_like(lg)
            _lib.check(_lib.lib().btx_mc_ce_bwd(lg.data_ptr(), lb.data_ptr(), S, B, C, act, reduce, ls, 1.0 / B, g.data_ptr(),
                                                ws.data_ptr(), ws.numel() * 4, dl.data_ptr(),
                                                torch.cuda.current_stream(lg.device).cuda_stream))
        dkl = (g / B).reshape(kl_shape) if (kl_shape is not None and ctx.needs_input_grad[2]) else None
        return dl, None, dkl, None, None


def hip_usable(stack, target):
    """the [S, B, C] stack and its labels can take the libbtx.so heads (this module's and the AvUC type=1 one)"""
    from ..mc import MC_MAX_CLASSES
    return (stack.is_cuda and _c._backend() != "torch" and stack.dtype in (torch.float32, torch.bfloat16)
            and target.dtype == torch.int64 and target.device == stack.device and 1 <= stack.shape[0] <= MAX_SAMPLES
            and stack.shape[1] >= 1 and 1 <= stack.shape[2] <= MC_MAX_CLASSES)


def mc_elbo_loss(stack, target, kl=None, reduce="logits", label_smoothing=0.0):
    """0-d loss = reduce-form cross-entropy of the MC stack [S, B, C] against target [B], plus kl / B (module docstring)"""
    _check(stack, target, reduce, label_smoothing)
    if not hip_usable(stack, target):
        return _mc_ce_chain(stack, target, kl, reduce, label_smoothing)
    dev_kl = torch.is_tensor(kl) and kl.numel() == 1 and kl.device == stack.device and kl.dtype == torch.float32
    loss = McCeFn.apply(stack, target, kl if dev_kl else None, _REDUCE[reduce], float(label_smoothing))
    if kl is not None and not dev_kl:  # a Python number, or a tensor elsewhere / of another dtype: torch's own add
        loss = loss + (kl.reshape(()).to(loss.device) if torch.is_tensor(kl) else kl) / stack.shape[1]
    return loss


class MCCrossEntropy(nn.Module):
    """nn.Module form of mc_elbo_loss: forward(stack [S, B, C], target [B], kl=None) -> 0-d loss"""

    def __init__(self, reduce="logits", label_smoothing=0.0):
        super().__init__()
        if reduce not in _REDUCE:
            raise ValueError("reduce must be 'logits' or 'loss', got %r" % (reduce,))
        self.reduce, self.label_smoothing = reduce, float(label_smoothing)

    def forward(self, stack, target, kl=None):
        return mc_elbo_loss(stack, target, kl, self.reduce, self.label_smoothing)


# ---- regression: the Gaussian negative log-likelihood of an MC stack (BTX-REG v1) --------------------------------------------
_REDUCE_REG = {"moments": 0, "loss": 1}
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _check_reg(stack, target, reduce, variance, noise_var):
    if reduce not in _REDUCE_REG:
        raise ValueError("reduce must be 'loss' or 'moments', got %r" % (reduce,))
    if variance not in ("log", None):
        raise ValueError("variance must be 'log' or None, got %r" % (variance,))
    if stack.dim() != 3:
        raise ValueError("stack must be Monte-Carlo stacked outputs [S, batch, W] (S = 1 for one sample)")
    S, B, W = stack.shape
    if variance == "log":
        if W % 2 or W < 2:
            raise ValueError("variance='log' needs an even output width (mean | log-variance), got %d" % W)
        D = W // 2
    else:
        if noise_var is None or not float(noise_var) > 0.0:
            raise ValueError("variance=None needs a positive noise_var")
        D = W
    if S < 1 or B < 1 or D < 1:
        raise ValueError("empty stack")
    if target.numel() != B * D:
        raise ValueError("target must hold %d x %d values, got %s" % (B, D, tuple(target.shape)))
    return D


def _mc_gnll_chain(stack, target, kl=None, reduce="loss", variance="log", noise_var=None, full=False):
    """the vectorised ATen chain (0-d loss); in float64 it is the oracle of the tests.  Half / bf16 stacks are evaluated in f32."""
    D = _check_reg(stack, target, reduce, variance, noise_var)
    S, B, W = stack.shape
    z = stack if stack.dtype in (torch.float32, torch.float64) else stack.float()
    y = target.to(device=z.device, dtype=z.dtype).reshape(B, D)
    if variance == "log":
        m, s = z[..., :D], z[..., D:]
    else:
        m, s = z, torch.full((1, 1, 1), math.log(float(noise_var)), dtype=z.dtype, device=z.device)
    if reduce == "loss":
        r = y - m
        nll = (0.5 * (s + r * r * torch.exp(-s))).sum() / (S * B)
    else:
        mb = m.mean(0)
        c = m - mb
        vb = torch.exp(s).mean(0) + (c * c).mean(0)
        r = y - mb
        nll = (0.5 * (torch.log(vb) + r * r / vb)).sum() / B
    if full:
        nll = nll + _HALF_LOG_2PI * D
    if kl is None:
        return nll
    if torch.is_tensor(kl):
        kl = kl.reshape(())
    return nll + kl / B


class McGnllFn(torch.autograd.Function):
    """0-d f32 loss of a [S, B, W] f32 / bf16 CUDA stack through btx_mc_gnll_fwd; `kl`: a 1-element f32 tensor on the stack's device or
    None; its gradient g / B is returned here, as McCeFn does."""

    @staticmethod
    def forward(ctx, stack, target, kl, reduce, has_var, noise_var, full):
        st = stack.contiguous()
        S, B, W = st.shape
        D = W // 2 if has_var else W
        y = target.reshape(B, D).contiguous()
        L = _lib.lib()
        ws = torch.empty(L.btx_mc_gnll_workspace_bytes(B, D) // 8, dtype=torch.float64, device=st.device)
        out = torch.empty(1, dtype=torch.float32, device=st.device)
        act = _lib.ACT_BF16 if st.dtype == torch.bfloat16 else _lib.ACT_F32
        klp = kl.detach().reshape(1).contiguous() if kl is not None else None
        _lib.check(L.btx_mc_gnll_fwd(st.data_ptr(), y.data_ptr(), S, B, D, has_var, act, reduce, noise_var, int(full), _c._ptr(klp),
                                     out.data_ptr(), ws.data_ptr(), ws.numel() * 8, torch.cuda.current_stream(st.device).cuda_stream))
        ctx.save_for_backward(st, y)
        ctx.cfg = (D, act, reduce, has_var, noise_var, None if kl is None else tuple(kl.shape))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        st, y = ctx.saved_tensors
        D, act, reduce, has_var, noise_var, kl_shape = ctx.cfg
        S, B, W = st.shape
        g = g.float().reshape(1).contiguous()
        ds = None
        if ctx.needs_input_grad[0]:
            ds = torch.empty_like(st)
            _lib.check(_lib.lib().btx_mc_gnll_bwd(st.data_ptr(), y.data_ptr(), S, B, D, has_var, act, reduce, noise_var, g.data_ptr(),
                                                  ds.data_ptr(), torch.cuda.current_stream(st.device).cuda_stream))
        dkl = (g / B).reshape(kl_shape) if (kl_shape is not None and ctx.needs_input_grad[2]) else None
        return ds, None, dkl, None, None, None, None


def gnll_hip_usable(stack, target):
    """the [S, B, W] stack and its targets can take btx_mc_gnll_*"""
    return (stack.is_cuda and _c._backend() != "torch" and stack.dtype in (torch.float32, torch.bfloat16)
            and target.dtype == torch.float32 and target.device == stack.device and 1 <= stack.shape[0] <= MAX_SAMPLES
            and stack.numel() < 2 ** 31 - 2)


def mc_gaussian_nll(stack, target, kl=None, reduce="loss", variance="log", noise_var=None, full=False):
    """0-d loss = reduce-form Gaussian negative log-likelihood of the MC stack [S, B, W] against target [B, D], plus kl / B (module
    docstring)"""
    _check_reg(stack, target, reduce, variance, noise_var)
    if not gnll_hip_usable(stack, target):
        return _mc_gnll_chain(stack, target, kl, reduce, variance, noise_var, full)
    dev_kl = torch.is_tensor(kl) and kl.numel() == 1 and kl.device == stack.device and kl.dtype == torch.float32
    loss = McGnllFn.apply(stack, target, kl if dev_kl else None, _REDUCE_REG[reduce], 1 if variance == "log" else 0,
                          1.0 if variance == "log" else float(noise_var), bool(full))
    if kl is not None and not dev_kl:  # a Python number, or a tensor elsewhere / of another dtype: torch's own add
        loss = loss + (kl.reshape(()).to(loss.device) if torch.is_tensor(kl) else kl) / stack.shape[1]
    return loss


class MCGaussianNLL(nn.Module):
    """nn.Module form of mc_gaussian_nll: forward(stack [S, B, W], target [B, D], kl=None) -> 0-d loss"""

    def __init__(self, reduce="loss", variance="log", noise_var=None, full=False):
        super().__init__()
        if reduce not in _REDUCE_REG:
            raise ValueError("reduce must be 'loss' or 'moments', got %r" % (reduce,))
        if variance not in ("log", None):
            raise ValueError("variance must be 'log' or None, got %r" % (variance,))
        if variance is None and (noise_var is None or not float(noise_var) > 0.0):
            raise ValueError("variance=None needs a positive noise_var")
        self.reduce, self.variance, self.noise_var, self.full = reduce, variance, noise_var, bool(full)

    def forward(self, stack, target, kl=None):
        return mc_gaussian_nll(stack, target, kl, self.reduce, self.variance, self.noise_var, self.full)
