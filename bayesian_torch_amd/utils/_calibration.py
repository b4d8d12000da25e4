"""Shared core of utils.avuc_loss and utils.uncertainty_calibration_loss.

All five losses are  loss = -beta * log(r + 1e-10),  r = (n_1 + n_4) / (n_1 + n_2 + n_3 + n_4 + 1e-10),  where n_q sums, over
the examples of one quadrant (good / bad x certain / uncertain), a product of two soft weights.  Gradients flow through the
weights only: never through a membership, a threshold, umin / umax or the arg-max.

Two implementations of the same arithmetic:
  * the vectorised ATen chain below (`avu_chain`, `eau_chain`): CPU tensors, set_backend("torch"), GPU inputs the kernels do not
    take (rows wider than mc.MC_MAX_CLASSES, other dtypes).  In float64 it is the oracle of the tests.
  * libbtx.so K9 (include/btx.h: btx_avu_fwd / btx_avu_bwd / btx_eau_fwd / btx_eau_bwd) behind `AvuFn` / `EauFn`: three launches
    for forward + backward, no host read, workspaces from torch's allocator — capturable under torch.cuda.graph.
`avu_mc_chain` / `AvuMcFn` (btx_avu_mc_fwd / btx_avu_mc_bwd, csrc/btx_mcloss.hip) are the same loss on an MC stack [S, B, C] with the
mutual information as the uncertainty (type=1).
"""
import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib

EPS = 1e-10
N_THRESHOLDS = 21  # np.linspace(0, 1, 21) of the reference's area form
AVU_MC_MAX_CLASSES = 16128  # BTX_AVU_MC_MAX_CLASSES: the type=1 backward keeps a row of C floats in LDS; wider rows run the chain


def _backend():
    from ..layers import base_variational_layer as bvl
    return bvl._BACKEND


def _threshold_like(th, ref):
    """threshold to compare `ref` with: a tensor goes to ref's dtype / device; a Python number stays one (no host-to-device copy,
    so the chain stays capturable) and torch rounds it to ref's dtype in the comparison, as torch.tensor(th) does"""
    if torch.is_tensor(th):
        return th.detach().reshape(()).to(device=ref.device, dtype=ref.dtype)
    return float(th)


def _ratio(wc, wu, good, cert):
    """r from the certain / uncertain weight of every example ([B]) and boolean memberships (cert may be [K, B]: r is [K])"""
    ng = ~good
    zero = torch.zeros((), dtype=wc.dtype, device=wc.device)
    n_gc = torch.where(good & cert, wc, zero).sum(-1)
    n_gu = torch.where(good & ~cert, wu, zero).sum(-1)
    n_bc = torch.where(ng & cert, wc, zero).sum(-1)
    n_bu = torch.where(ng & ~cert, wu, zero).sum(-1)
    return (n_gc + n_bu) / (n_gc + n_gu + n_bc + n_bu + EPS)


def row_stats(logits):
    """confidence, prediction and entropy (epsilon 1e-10) of every row of [B, C] logits"""
    probs = F.softmax(logits, dim=1)
    conf, pred = torch.max(probs, 1)
    ent = -1 * torch.sum(probs * torch.log(probs + EPS), dim=-1)
    return conf, pred, ent


def area_thresholds(ent):
    """the 21 thresholds umin + t_k (umax - umin) in float64 from the entropies' own precision; th_0 = umin and th_20 = umax
    exactly (the reference rounds umax - umin in f32 first, which makes the top membership a last-bit coin flip)"""
    e = ent.detach().double()
    umin, umax = e.min(), e.max()
    t = torch.arange(N_THRESHOLDS, dtype=torch.float64, device=ent.device) * 0.05
    th = umin + t * (umax - umin)
    th[N_THRESHOLDS - 1] = umax
    return th


def avu_chain(logits, labels, th, beta, area):
    """(loss, r): shape [1] each.  area=False: one threshold `th`; area=True: trapezoid of AvU over the 21 thresholds."""
    conf, pred, ent = row_stats(logits)
    good = pred == labels.reshape(-1)
    tu = torch.tanh(ent)
    w = torch.where(good, conf, 1 - conf)
    wc, wu = w * (1 - tu), w * tu
    if area:
        cert = ent.detach().double().unsqueeze(0) <= area_thresholds(ent).unsqueeze(1)  # [K, B]
        rk = _ratio(wc, wu, good, cert)
        r = (0.05 * (rk[:-1] + rk[1:]) * 0.5).sum().reshape(1)
    else:
        cert = ent.detach() <= _threshold_like(th, ent)
        r = _ratio(wc, wu, good, cert).reshape(1)
    return -1 * beta * torch.log(r + EPS), r


def mc_row_stats(stack):
    """confidence, prediction and model uncertainty of every batch row of an MC stack [S, B, C] of logits:
    p_s = softmax(logits_s), pbar = mean_s p_s, conf / pred from pbar (lowest index on ties), and the mutual information
    H(pbar) - mean_s H(p_s) with epsilon 1e-10 inside every log (the reference's model_uncertainty / expected_entropy)"""
    probs = F.softmax(stack, dim=2)
    pbar = probs.mean(0)
    conf, pred = torch.max(pbar, 1)
    h_bar = -1 * torch.sum(pbar * torch.log(pbar + EPS), dim=-1)
    h_exp = (-1 * torch.sum(probs * torch.log(probs + EPS), dim=-1)).mean(0)
    return conf, pred, h_bar - h_exp


def avu_mc_chain(stack, labels, th, beta, area):
    """avu_chain on an MC stack [S, B, C]: the same quadrant arithmetic with (conf, pred, uncertainty) of mc_row_stats"""
    conf, pred, unc = mc_row_stats(stack)
    good = pred == labels.reshape(-1)
    tu = torch.tanh(unc)
    w = torch.where(good, conf, 1 - conf)
    wc, wu = w * (1 - tu), w * tu
    if area:
        cert = unc.detach().double().unsqueeze(0) <= area_thresholds(unc).unsqueeze(1)  # [K, B]
        rk = _ratio(wc, wu, good, cert)
        r = (0.05 * (rk[:-1] + rk[1:]) * 0.5).sum().reshape(1)
    else:
        cert = unc.detach() <= _threshold_like(th, unc)
        r = _ratio(wc, wu, good, cert).reshape(1)
    return -1 * beta * torch.log(r + EPS), r


def eau_chain(error, other, error_th, other_th, beta, conf_form):
    """0-d loss of EaU (conf_form False: other = uncertainty) or EaC (conf_form True: other = confidence)"""
    error, other = error.reshape(-1), other.reshape(-1)
    good = error.detach() <= _threshold_like(error_th, error)
    te = torch.tanh(error)
    w = torch.where(good, 1 - te, te)
    if conf_form:
        cert = other.detach() > _threshold_like(other_th, other)
        wc, wu = w * other, w * (1 - other)
    else:
        cert = other.detach() <= _threshold_like(other_th, other)
        tu = torch.tanh(other)
        wc, wu = w * (1 - tu), w * tu
    return -1 * beta * torch.log(_ratio(wc, wu, good, cert) + EPS)


# ---- HIP path ----------------------------------------------------------------------------------------------------------
def _th_args(th, dev):
    """(float, device tensor or None): a Python number is baked into the launch, a tensor is read by the kernel when it runs"""
    if torch.is_tensor(th):
        if th.numel() != 1:
            raise ValueError("a tensor threshold must hold one element")
        if th.device != dev:
            raise ValueError("a tensor threshold must live on the device of the inputs (%s), got %s" % (dev, th.device))
        return 0.0, th.detach().reshape(1).to(torch.float32)
    return float(th), None


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _workspace(B, dev):
    return torch.empty(_lib.lib().btx_calib_workspace_bytes(B) // 4, dtype=torch.float32, device=dev)


def _avu_forward(ctx, fwd, ws_bytes, logits, labels, th, beta, area):
    """forward of AvuFn ([B, C] logits) and AvuMcFn ([S, B, C]): the entry point `fwd` takes the logits' shape as its leading
    integers and `ws_bytes` all of it but the classes"""
    lg = logits.contiguous()
    lb = labels.reshape(-1).contiguous()
    thf, thd = _th_args(0.0 if area else th, lg.device)
    L = _lib.lib()
    ws = torch.empty(getattr(L, ws_bytes)(*lg.shape[:-1]) // 4, dtype=torch.float32, device=lg.device)
    out = torch.empty(2, dtype=torch.float32, device=lg.device)
    act = _lib.ACT_BF16 if lg.dtype == torch.bfloat16 else _lib.ACT_F32
    _lib.check(getattr(L, fwd)(lg.data_ptr(), lb.data_ptr(), *lg.shape, act, 1 if area else 0, thf, _ptr(thd), float(beta),
                               out.data_ptr(), ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream(lg.device).cuda_stream))
    ctx.save_for_backward(lg, ws)
    ctx.act = act
    ctx.set_materialize_grads(False)
    return out[0:1], out[1:2]


def _avu_backward(ctx, bwd, g_loss, g_r):
    lg, ws = ctx.saved_tensors
    if g_loss is None and g_r is None:
        return None, None, None, None, None
    g_loss = None if g_loss is None else g_loss.float().contiguous()
    g_r = None if g_r is None else g_r.float().contiguous()
    dl = torch.empty_like(lg)
    _lib.check(getattr(_lib.lib(), bwd)(lg.data_ptr(), *lg.shape, ctx.act, _ptr(g_loss), _ptr(g_r), ws.data_ptr(), ws.numel() * 4,
                                        dl.data_ptr(), torch.cuda.current_stream(lg.device).cuda_stream))
    return dl, None, None, None, None


class AvuFn(torch.autograd.Function):
    """(loss [1], r [1]) of [B, C] f32 / bf16 CUDA logits through btx_avu_fwd; both outputs are f32 and carry gradient."""

    @staticmethod
    def forward(ctx, logits, labels, th, beta, area):
        return _avu_forward(ctx, "btx_avu_fwd", "btx_calib_workspace_bytes", logits, labels, th, beta, area)

    @staticmethod
    def backward(ctx, g_loss, g_r):
        return _avu_backward(ctx, "btx_avu_bwd", g_loss, g_r)


class EauFn(torch.autograd.Function):
    """0-d f32 loss of 1-D f32 CUDA error / other through btx_eau_fwd"""

    @staticmethod
    def forward(ctx, error, other, error_th, other_th, beta, conf_form):
        e, o = error.contiguous(), other.contiguous()
        B = e.numel()
        etf, etd = _th_args(error_th, e.device)
        otf, otd = _th_args(other_th, e.device)
        ws = _workspace(B, e.device)
        out = torch.empty(2, dtype=torch.float32, device=e.device)
        _lib.check(_lib.lib().btx_eau_fwd(e.data_ptr(), o.data_ptr(), B, 1 if conf_form else 0, etf, _ptr(etd), otf, _ptr(otd),
                                          float(beta), out.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                          torch.cuda.current_stream(e.device).cuda_stream))
        ctx.save_for_backward(e, o, ws)
        ctx.conf_form = 1 if conf_form else 0
        ctx.set_materialize_grads(False)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        e, o, ws = ctx.saved_tensors
        if g is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None, None
        g = g.float().contiguous()
        de = torch.empty_like(e) if ctx.needs_input_grad[0] else None
        do = torch.empty_like(o) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().btx_eau_bwd(e.data_ptr(), o.data_ptr(), e.numel(), ctx.conf_form, g.data_ptr(), ws.data_ptr(),
                                          ws.numel() * 4, _ptr(de), _ptr(do), torch.cuda.current_stream(e.device).cuda_stream))
        return de, do, None, None, None, None


def avu(logits, labels, th, beta, area):
    """dispatch: (loss [1], r [1])"""
    if logits.dim() != 2:
        raise ValueError("logits must be [batch, classes] for type=0 (predictive entropy); MC-stacked [S, batch, classes] logits "
                         "go with type=1 (model uncertainty)")
    if labels.numel() != logits.shape[0]:
        raise ValueError("labels must hold one class index per row of logits")
    from ..mc import MC_MAX_CLASSES
    if (logits.is_cuda and _backend() != "torch" and logits.dtype in (torch.float32, torch.bfloat16)
            and labels.dtype == torch.int64 and labels.device == logits.device and logits.shape[0] > 0
            and 0 < logits.shape[1] <= MC_MAX_CLASSES):
        return AvuFn.apply(logits, labels, th, beta, bool(area))
    return avu_chain(logits, labels, th, beta, bool(area))


class AvuMcFn(torch.autograd.Function):
    """(loss [1], r [1]) of an MC stack [S, B, C] of f32 / bf16 CUDA logits through btx_avu_mc_fwd (model uncertainty, type=1)"""

    @staticmethod
    def forward(ctx, stack, labels, th, beta, area):
        return _avu_forward(ctx, "btx_avu_mc_fwd", "btx_mcloss_workspace_bytes", stack, labels, th, beta, area)

    @staticmethod
    def backward(ctx, g_loss, g_r):
        return _avu_backward(ctx, "btx_avu_mc_bwd", g_loss, g_r)


def avu_mc(stack, labels, th, beta, area):
    """dispatch for type=1 (model uncertainty): (loss [1], r [1]) of an MC stack [S, B, C]"""
    if stack.dim() != 3:
        raise ValueError("type=1 (model uncertainty) needs Monte-Carlo stacked logits [S, batch, classes]; "
                         "use type=0 (predictive entropy) on [batch, classes] logits")
    if labels.numel() != stack.shape[1]:
        raise ValueError("labels must hold one class index per batch row of the stacked logits")
    from .mc_loss import hip_usable
    if hip_usable(stack, labels) and stack.shape[2] <= AVU_MC_MAX_CLASSES:
        return AvuMcFn.apply(stack, labels, th, beta, bool(area))
    return avu_mc_chain(stack, labels, th, beta, bool(area))


def eau(error, other, error_th, other_th, beta, conf_form):
    """dispatch: 0-d loss.  Column vectors [B, 1] are flattened (the reference returns the degenerate -beta * log(1e-10) for
    them: every torch.dot falls into its `except`)."""
    error, other = error.reshape(-1), other.reshape(-1)
    if error.numel() != other.numel():
        raise ValueError("error and %s must hold the same number of elements" % ("conf" if conf_form else "unc"))
    if (error.is_cuda and other.device == error.device and _backend() != "torch" and error.dtype == torch.float32
            and other.dtype == torch.float32 and error.numel() > 0):
        return EauFn.apply(error, other, error_th, other_th, beta, bool(conf_form))
    return eau_chain(error, other, error_th, other_th, beta, bool(conf_form))


# ---- numpy helpers (reference utils/avuc_loss.py:370-443), vectorised ---------------------------------------------------
def np_entropy(prob):
    return -1 * np.sum(prob * np.log(prob + 1e-15), axis=-1)


def np_quadrant_counts(pred_label, true_label, uncertainty, thresholds):
    """(n_ac, n_au, n_ic, n_iu), each of thresholds' shape"""
    acc = (np.asarray(true_label) == np.asarray(pred_label)).reshape(-1)
    cert = np.asarray(uncertainty).reshape(-1) <= np.asarray(thresholds)[..., None]
    n_ac = np.sum(acc & cert, axis=-1)
    n_au = np.sum(acc & ~cert, axis=-1)
    n_ic = np.sum(~acc & cert, axis=-1)
    n_iu = np.sum(~acc & ~cert, axis=-1)
    return n_ac, n_au, n_ic, n_iu
