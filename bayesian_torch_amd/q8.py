"""INT8 inference plumbing (BTX-Q8 v1): the carrier of quantized GPU activations and the ctypes wrappers of the
btx_q8_* entry points (include/btx.h K10).

torch has no quantized tensors on ROCm devices, so a quantized activation travels between layers as a `QTensor`: a uint8
tensor (channels-last for 4-D), a scale and a zero point, with the handful of methods of a torch.quint8 tensor that model code
calls between layers."""
import ctypes

import numpy as np
import torch

from . import _lib


class QTensor:
    """uint8 values + (scale, zero_point): value = (q - zero_point) * scale.  4-D tensors are kept channels-last (what the i8
    contraction reads and writes); the logical shape is NCHW as everywhere in torch."""

    is_quantized = True
    dtype = torch.quint8

    def __init__(self, q, scale, zero_point):
        if q.dtype != torch.uint8:
            raise _lib.BtxError("QTensor holds uint8 values (got %s)" % q.dtype)
        if q.dim() == 4:
            q = q.contiguous(memory_format=torch.channels_last)
        self.q, self.scale, self.zero_point = q, float(scale), int(zero_point)

    shape = property(lambda self: self.q.shape)
    device = property(lambda self: self.q.device)
    is_cuda = property(lambda self: self.q.is_cuda)

    def dim(self):
        return self.q.dim()

    def size(self, *a):
        return self.q.size(*a)

    def int_repr(self):
        return self.q

    def q_scale(self):
        return self.scale

    def q_zero_point(self):
        return self.zero_point

    def dequantize(self):
        return (self.q.to(torch.float32) - float(self.zero_point)) * np.float32(self.scale).item()

    def relu(self):
        return QTensor(self.q.clamp(min=self.zero_point), self.scale, self.zero_point)

    def flatten(self, start_dim=0, end_dim=-1):
        return QTensor(self.q.flatten(start_dim, end_dim), self.scale, self.zero_point)

    def reshape(self, *shape):
        return QTensor(self.q.reshape(*shape), self.scale, self.zero_point)

    def view(self, *shape):
        """torch's view of the logical NCHW tensor.  A channels-last 4-D carrier is viewable as it is when H = W = 1 (the tensor
        behind the average pool of a ResNet); any other 4-D carrier is put in NCHW order first, like reshape()."""
        q = self.q
        if q.dim() == 4 and not q.is_contiguous():
            q = q.contiguous()
        return QTensor(q.view(*shape), self.scale, self.zero_point)

    def contiguous(self):
        return self

    def to(self, *a, **kw):
        return QTensor(self.q.to(*a, **kw), self.scale, self.zero_point)

    def cpu(self):
        return self.to("cpu")

    def as_torch_quint8(self):
        """a real torch.quint8 tensor (CPU only: torch's quantized backends live there)"""
        return torch._make_per_tensor_quantized_tensor(self.q.cpu().contiguous(), self.scale, self.zero_point)

    def __repr__(self):
        return "QTensor(shape=%s, scale=%g, zero_point=%d, device=%s)" % (tuple(self.q.shape), self.scale, self.zero_point, self.q.device)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def quantize_act(x, scale, zero_point):
    """f32 / bf16 CUDA tensor [B, K] or [B, C, H, W] (any memory format) -> QTensor, one launch (btx_q8_quantize_act)"""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.BtxError("quantized layers take float32 or bfloat16 activations (got %s)" % x.dtype)
    if x.dim() == 2:
        nb, c, h, w = x.shape[0], x.shape[1], 1, 1
        st = (x.stride(0), x.stride(1), 0, 0)
        out = torch.empty((nb, c), dtype=torch.uint8, device=x.device)
    elif x.dim() == 4:
        nb, c, h, w = x.shape
        st = tuple(x.stride())
        out = torch.empty((nb, c, h, w), dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
    else:
        raise _lib.BtxError("quantized layers take [B, K] or [B, C, H, W] activations (got %d-D)" % x.dim())
    strides = (ctypes.c_int64 * 4)(*[int(s) for s in st])
    _lib.check(_lib.lib().btx_q8_quantize_act(x.data_ptr(), _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32, strides,
                                              out.data_ptr(), nb, c, h, w, float(scale), int(zero_point), _stream(x.device)))
    return QTensor(out, scale, zero_point)


def make_chain(s_sigma, s_mu, s_eps, s_d, s_w, s_x):
    """BtxQ8Chain: the f32 scales, their f32 reciprocals (computed here, once, in f32) and the double bias divisor"""
    f = np.float32
    one = f(1.0)
    return _lib.Q8Chain(float(f(s_sigma)), float(f(s_mu)), float(f(s_eps)), float(one / f(s_eps)), float(f(s_d)), float(one / f(s_d)),
                        float(one / f(s_w)), float(s_x) * float(s_w))


def weight_row_bytes(taps, c):
    n = int(_lib.lib().btx_q8_weight_row_bytes(int(taps), int(c)))
    if n == 0:
        raise _lib.BtxError("quantized layer too large for the int8 weight image (taps=%d, C=%d)" % (taps, c))
    return n


def sample_weights(mu_p, sigma_p, mu_b, sigma_b, n, taps, c, eps_c, chain, seed, sample_idx, layer_id, sample_dev=None, eps_w=None,
                   eps_b=None):
    """btx_q8_sample_weights: int8 GEMM-major [n][taps][c] mu_i / sigma_i -> (W [n][Kp] int8, S [n] int32, b_i [n] int32).
    eps_w: f32 GEMM-major [n][taps][c] explicit noise (eps_b: [n]) instead of BTX-RNG v1."""
    dev = mu_p.device
    kp = weight_row_bytes(taps, c)
    W = torch.empty((n, kp), dtype=torch.int8, device=dev)
    S = torch.empty(n, dtype=torch.int32, device=dev)
    b_i = torch.empty(n, dtype=torch.int32, device=dev)
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(_lib.lib().btx_q8_sample_weights(mu_p.data_ptr(), sigma_p.data_ptr(), ptr(mu_b), ptr(sigma_b), int(n), int(taps), int(c),
                                                int(eps_c), ctypes.byref(chain), ctypes.byref(r), ptr(eps_w), ptr(eps_b),
                                                W.data_ptr(), S.data_ptr(), b_i.data_ptr(), _stream(dev)))
    return W, S, b_i


def make_add(s_a, z_a, s_b, z_b, scale, zero_point, relu=False):
    """BtxQ8Add: the three f32 constants of the add (pre_a, pre_b, 1 / s), computed here, once, in f32"""
    f = np.float32
    return _lib.Q8Add(float(f(s_a)), float(f(s_a) * f(-int(z_a))), float(f(s_b)), float(f(s_b) * f(-int(z_b))),
                      float(f(1.0) / f(scale)), int(zero_point), 1 if relu else 0)


def contract(xq, z_x, W, S, b_i, n, kernel, stride, padding, dilation, multiplier, z_o, relu, out_f32, s_o, residual=None, add=None):
    """btx_q8_contract, or with `residual` (uint8, the output's shape and layout) and `add` (make_add) btx_q8_contract_res.
    xq: uint8 [B, K] (Linear, kernel (1, 1)) or channels-last [B, C, H, W]."""
    g = _lib.Geom()
    if xq.dim() == 2:
        g.NB, g.C, g.H, g.W = xq.shape[0], xq.shape[1], 1, 1
    else:
        g.NB, g.C, g.H, g.W = xq.shape
    g.D = g.KD = 1
    g.N = int(n)
    g.KH, g.KW = kernel
    g.sd, g.sh, g.sw = 1, stride[0], stride[1]
    g.pd, g.ph, g.pw = 0, padding[0], padding[1]
    g.dd, g.dh, g.dw = 1, dilation[0], dilation[1]
    g.groups = 1
    oh = (g.H + 2 * g.ph - g.dh * (g.KH - 1) - 1) // g.sh + 1
    ow = (g.W + 2 * g.pw - g.dw * (g.KW - 1) - 1) // g.sw + 1
    if oh <= 0 or ow <= 0:
        raise _lib.BtxError("quantized conv: the kernel does not fit the input")
    dt = torch.float32 if out_f32 else torch.uint8
    if xq.dim() == 2:
        out = torch.empty((g.NB, g.N), dtype=dt, device=xq.device)
    else:
        out = torch.empty((g.NB, g.N, oh, ow), dtype=dt, device=xq.device, memory_format=torch.channels_last)
    if residual is not None:
        if residual.dtype != torch.uint8 or residual.shape != out.shape or residual.device != out.device:
            raise _lib.BtxError("quantized conv: the residual must be uint8 of the output's shape %s on its device (got %s %s)"
                                % (tuple(out.shape), residual.dtype, tuple(residual.shape)))
        if residual.dim() == 4:
            residual = residual.contiguous(memory_format=torch.channels_last)
        _lib.check(_lib.lib().btx_q8_contract_res(ctypes.byref(g), xq.data_ptr(), int(z_x), W.data_ptr(), S.data_ptr(), b_i.data_ptr(),
                                                  float(multiplier), int(z_o), 1 if relu else 0, 1 if out_f32 else 0,
                                                  residual.data_ptr(), ctypes.byref(add), out.data_ptr(), _stream(xq.device)))
        return out
    _lib.check(_lib.lib().btx_q8_contract(ctypes.byref(g), xq.data_ptr(), int(z_x), W.data_ptr(), S.data_ptr(), b_i.data_ptr(),
                                          float(multiplier), int(z_o), 1 if relu else 0, 1 if out_f32 else 0, float(np.float32(s_o)),
                                          out.data_ptr(), _stream(xq.device)))
    return out


# ---- Flipout (DESIGN.md §13 "Flipout") -----------------------------------------------------------------------------------
def mul_multiplier(s_a, s_b, s_o):
    """m of quantized.mul: f32(f32(s_a) * f32(s_b)) * (f32(1) / f32(s_o)), computed here, once, in f32"""
    f = np.float32
    return float(f(f(s_a) * f(s_b)) * (f(1.0) / f(s_o)))


def sign_bytes(scale, zero_point):
    """the bytes of q(+1) and q(-1) at (scale, zero_point): a quantized sign is not exactly +-1"""
    f = np.float32
    inv = f(1.0) / f(scale)
    return tuple(int(np.clip(np.rint(f(v) * inv) + f(zero_point), f(0), f(255))) for v in (1.0, -1.0))


_BIAS = {"none": _lib.Q8_BIAS_NONE, "mu": _lib.Q8_BIAS_MU, "sigma_eps": _lib.Q8_BIAS_SIGMA_EPS}


def sample_delta(sigma_p, mu_b, sigma_b, n, taps, c, eps_c, s_sigma, s_mu, s_x, e, mean_bias, pert_bias, seed, sample_idx, layer_id,
                 sample_dev=None, eps_w=None, eps_b=None):
    """btx_q8_sample_delta: int8 GEMM-major [n][taps][c] sigma_i -> (D [n][Kp] int8, S_d, b_mean_i, b_pert_i [n] int32).
    e: the ten (scale, zero point) entries; mean_bias / pert_bias: 'none' | 'mu' | 'sigma_eps'."""
    dev = sigma_p.device
    kp = weight_row_bytes(taps, c)
    D = torch.empty((n, kp), dtype=torch.int8, device=dev)
    S = torch.empty(n, dtype=torch.int32, device=dev)
    bm = torch.empty(n, dtype=torch.int32, device=dev)
    bp = torch.empty(n, dtype=torch.int32, device=dev)
    f = np.float32
    d = _lib.Q8Delta(float(f(1.0) / f(e[0][0])), mul_multiplier(s_sigma, e[0][0], e[1][0]), _BIAS[mean_bias], _BIAS[pert_bias],
                     float(s_x) * float(s_mu), float(e[6][0]) * float(e[1][0]))
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(_lib.lib().btx_q8_sample_delta(sigma_p.data_ptr(), ptr(mu_b), ptr(sigma_b), int(n), int(taps), int(c), int(eps_c),
                                              ctypes.byref(d), ctypes.byref(r), ptr(eps_w), ptr(eps_b), D.data_ptr(), S.data_ptr(),
                                              bm.data_ptr(), bp.data_ptr(), _stream(dev)))
    return D, S, bm, bp


def make_flipout(s_x, z_x, s_mu, e):
    """BtxQ8Flipout from the input's (scale, zero point), the mean weights' scale and the ten entries"""
    f = np.float32
    ip, ineg = sign_bytes(*e[4])
    op, oneg = sign_bytes(*e[5])
    return _lib.Q8Flipout(int(z_x), int(e[6][1]), int(e[3][1]), int(e[7][1]), int(e[8][1]), ip - e[4][1], ineg - e[4][1], op - e[5][1],
                          oneg - e[5][1], mul_multiplier(s_x, e[4][0], e[6][0]), float(f(f(s_x) * f(s_mu)) / f(e[3][0])),
                          float(f(f(e[6][0]) * f(e[1][0])) / f(e[7][0])), mul_multiplier(e[7][0], e[5][0], e[8][0]), float(f(e[9][0])))


def contract_flipout(xq, W_mu, S_mu, bm_i, D, S_d, bp_i, n, kernel, stride, padding, dilation, flip, add, seed, sample_idx, layer_id,
                     sign_c, sample_dev=None, sign_in=None, sign_out=None, out_f32=False):
    """btx_q8_contract_flipout.  xq: uint8 [B, K] or channels-last [B, C, H, W]; sign_in / sign_out: int8 +1 / -1 in the physical
    (channels-last) order of x / the output, or None -> BTX-RNG v1."""
    g = _lib.Geom()
    if xq.dim() == 2:
        g.NB, g.C, g.H, g.W = xq.shape[0], xq.shape[1], 1, 1
    else:
        g.NB, g.C, g.H, g.W = xq.shape
    g.D = g.KD = 1
    g.N = int(n)
    g.KH, g.KW = kernel
    g.sd, g.sh, g.sw = 1, stride[0], stride[1]
    g.pd, g.ph, g.pw = 0, padding[0], padding[1]
    g.dd, g.dh, g.dw = 1, dilation[0], dilation[1]
    g.groups = 1
    oh = (g.H + 2 * g.ph - g.dh * (g.KH - 1) - 1) // g.sh + 1
    ow = (g.W + 2 * g.pw - g.dw * (g.KW - 1) - 1) // g.sw + 1
    if oh <= 0 or ow <= 0:
        raise _lib.BtxError("quantized conv: the kernel does not fit the input")
    dt = torch.float32 if out_f32 else torch.uint8
    if xq.dim() == 2:
        out = torch.empty((g.NB, g.N), dtype=dt, device=xq.device)
    else:
        out = torch.empty((g.NB, g.N, oh, ow), dtype=dt, device=xq.device, memory_format=torch.channels_last)
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(_lib.lib().btx_q8_contract_flipout(ctypes.byref(g), xq.data_ptr(), W_mu.data_ptr(), S_mu.data_ptr(), bm_i.data_ptr(),
                                                  D.data_ptr(), S_d.data_ptr(), bp_i.data_ptr(), ctypes.byref(flip), ctypes.byref(add),
                                                  ctypes.byref(r), int(sign_c), ptr(sign_in), ptr(sign_out), 1 if out_f32 else 0,
                                                  out.data_ptr(), _stream(xq.device)))
    return out


# ---- between the layers: one `forward` for both devices -------------------------------------------------------------------
def _is_quint8(x):
    return isinstance(x, torch.Tensor) and x.dtype == torch.quint8


def _gpu_q(x, what):
    if isinstance(x, QTensor):
        if not x.is_cuda:
            raise _lib.BtxError("q8.%s: a QTensor runs on the GPU; on the CPU pass a torch.quint8 tensor (QTensor.as_torch_quint8())" % what)
        return x
    raise _lib.BtxError("q8.%s takes a q8.QTensor (GPU) or a torch.quint8 tensor (CPU), got %s" % (what, type(x).__name__))


def add(a, b, scale, zero_point, relu=False):
    """torch.ops.quantized.add / add_relu (CPU, torch.quint8), or btx_q8_add (GPU, QTensor): one launch"""
    if _is_quint8(a) and _is_quint8(b):
        op = torch.ops.quantized.add_relu if relu else torch.ops.quantized.add
        return op(a, b, float(scale), int(zero_point))
    a, b = _gpu_q(a, "add"), _gpu_q(b, "add")
    if a.shape != b.shape or a.device != b.device:
        raise _lib.BtxError("q8.add: operands differ in shape or device (%s, %s)" % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty_like(a.q)
    bq = b.q if b.q.stride() == a.q.stride() else b.q.contiguous(memory_format=torch.channels_last if a.q.dim() == 4 else torch.contiguous_format)
    if not out.is_contiguous() and not (out.dim() == 4 and out.is_contiguous(memory_format=torch.channels_last)):
        raise _lib.BtxError("q8.add: operands must be dense")
    p = make_add(a.scale, a.zero_point, b.scale, b.zero_point, scale, zero_point, relu)
    _lib.check(_lib.lib().btx_q8_add(a.q.data_ptr(), bq.data_ptr(), out.data_ptr(), out.numel(), ctypes.byref(p), _stream(out.device)))
    return QTensor(out, scale, zero_point)


def _pool_args(x, what):
    x = _gpu_q(x, what)
    if x.q.dim() != 4:
        raise _lib.BtxError("q8.%s takes a [B, C, H, W] tensor (got %d-D)" % (what, x.q.dim()))
    return x


def _one(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2 or v[0] != v[1]:
            raise _lib.BtxError("q8 pooling: %s must be square (got %s)" % (what, (v,)))
        v = v[0]
    return int(v)


def max_pool2d(x, k, stride=None, padding=0):
    """F.max_pool2d on quint8 (CPU), btx_q8_maxpool2d_cl (GPU).  Scale and zero point pass through."""
    stride = k if stride is None else stride
    if _is_quint8(x):
        return torch.nn.functional.max_pool2d(x, k, stride, padding)
    x = _pool_args(x, "max_pool2d")
    k, s, p = _one(k, "kernel"), _one(stride, "stride"), _one(padding, "padding")
    nb, c, h, w = x.q.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    if ho <= 0 or wo <= 0:
        raise _lib.BtxError("q8.max_pool2d: the window does not fit the input")
    out = torch.empty((nb, c, ho, wo), dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
    _lib.check(_lib.lib().btx_q8_maxpool2d_cl(x.q.data_ptr(), out.data_ptr(), nb, h, w, c, k, s, p, _stream(x.device)))
    return QTensor(out, x.scale, x.zero_point)


def avg_pool2d(x, k, stride=None, padding=0, ceil_mode=False):
    """F.avg_pool2d on quint8 (CPU), btx_q8_avgpool2d_cl (GPU: no padding, floor mode).  Scale and zero point pass through."""
    stride = k if stride is None else stride
    if _is_quint8(x):
        return torch.nn.functional.avg_pool2d(x, k, stride, padding, ceil_mode)
    x = _pool_args(x, "avg_pool2d")
    k, s, p = _one(k, "kernel"), _one(stride, "stride"), _one(padding, "padding")
    nb, c, h, w = x.q.shape
    ho, wo = (h - k) // s + 1, (w - k) // s + 1
    if ho <= 0 or wo <= 0:
        raise _lib.BtxError("q8.avg_pool2d: the window does not fit the input")
    out = torch.empty((nb, c, ho, wo), dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
    _lib.check(_lib.lib().btx_q8_avgpool2d_cl(x.q.data_ptr(), out.data_ptr(), nb, h, w, c, k, s, p, 1 if ceil_mode else 0,
                                              x.zero_point, _stream(x.device)))
    return QTensor(out, x.scale, x.zero_point)


def relu(x):
    """max(q, z): torch.relu on quint8, QTensor.relu() on the GPU"""
    if _is_quint8(x):
        return torch.relu(x)
    return _gpu_q(x, "relu").relu()
