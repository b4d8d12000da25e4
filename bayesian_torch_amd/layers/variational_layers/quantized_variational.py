"""QuantizedLinearReparameterization / QuantizedConv2dReparameterization — INT8 inference twins of the Reparameterization layers
(reference layers/variational_layers/quantize_linear_variational.py:44-224, quantize_conv_variational.py:303-552).

Arithmetic: BTX-Q8 v1.  On a CUDA tensor a forward is three launches of libbtx.so (activation quantize — skipped
when the input arrives quantized —, the weight sampling pre-pass, the i8 MFMA contraction); on a CPU tensor it is the reference's
own chain of torch quantized ops with eps drawn from the torch generator.  Storage: plain int8 buffers under the reference's names
(`quantized_mu_weight`, `quantized_sigma_weight`) with their float scales, f32 `quantized_mu_bias` / `quantized_sigma_bias` (the
bias is never quantized to 8 bits).  Not differentiable; `kl_loss()` is 0 as in the reference."""
import numpy as np
import torch
from torch.nn import Parameter

from .. import base_variational_layer as _base
from ... import _lib
from ... import q8 as _q8
from ... import rng as _rng

__all__ = ["QuantizedLinearReparameterization", "QuantizedConv2dReparameterization"]

_ENTRY_NAMES = ("eps", "mul", "add", "input", "output")


def _pair(v):
    return (int(v), int(v)) if not isinstance(v, (tuple, list)) else (int(v[0]), int(v[1]))


def _entry(e):
    """one quant_dict entry -> (scale, zero_point): a (scale, zp) pair, or the reference's {'scale': .., 'zero_point': ..}"""
    if isinstance(e, (tuple, list)):
        return float(e[0]), int(e[1])
    return float(e["scale"]), int(e["zero_point"])


class _QuantizedReparameterization(_base.BaseVariationalLayer_):
    _nd = 0
    _btx_q8 = True   # rng / mc: MC sample lanes > 1 are refused on a model that holds one of these

    def _setup(self, in_ch, out_ch, kernel_size, stride, padding, dilation, groups, bias):
        nd = self._nd
        self._wn = "weight" if nd == 0 else "kernel"
        self.bias = bias
        if nd == 0:
            self.in_features, self.out_features = in_ch, out_ch
            wshape = (out_ch, in_ch)
        else:
            self.in_channels, self.out_channels = in_ch, out_ch
            self.kernel_size, self.stride, self.padding, self.dilation, self.groups = kernel_size, stride, padding, dilation, groups
            wshape = (out_ch, in_ch // groups) + _pair(kernel_size)
            # conv + BatchNorm folding (reference quantize_conv_variational.py:338-343): set by models.bnn_to_qbnn(fuse_conv_bn=True)
            self.bn_weight = self.bn_bias = self.bn_running_mean = self.bn_running_var = self.bn_eps = None
            self.relu = False   # fold a ReLU (clamp at the output zero point) into the store
        # the float parameters exist until quantize() (the reference's constructor builds a float layer too)
        setattr(self, "mu_" + self._wn, Parameter(torch.empty(wshape).normal_(0, 0.1)))
        setattr(self, "rho_" + self._wn, Parameter(torch.empty(wshape).normal_(-3.0, 0.1)))
        self.register_buffer("eps_" + self._wn, torch.zeros(wshape), persistent=False)
        if bias:
            self.mu_bias = Parameter(torch.empty(out_ch).normal_(0, 0.1))
            self.rho_bias = Parameter(torch.empty(out_ch).normal_(-3.0, 0.1))
            self.register_buffer("eps_bias", torch.zeros(out_ch), persistent=False)
        else:
            self.register_parameter("mu_bias", None)
            self.register_parameter("rho_bias", None)
            self.register_buffer("eps_bias", None, persistent=False)
        self.is_dequant = False
        self.quant_dict = None
        self.quant_prepare = False
        self._btx_layer_id = _rng.next_layer_id()
        self._btx_sample = 0
        self._q8_scales = None   # (s_mu, s_sigma) after quantize()

    # ---- reference surface --------------------------------------------------------------------------------------
    def get_scale_and_zero_point(self, x, upper_bound=100, target_range=255):
        xmax = torch.clamp(x.abs().max(), 0, upper_bound)
        return xmax * 2 / target_range, torch.zeros(1)

    def get_quantized_tensor(self, x, default_scale=0.1):
        """-> (int8 tensor, scale): the reference's symmetric per-tensor quantization, computed on the host"""
        x = x.detach().float().cpu()
        scale, _ = self.get_scale_and_zero_point(x)
        if scale == 0:
            scale = torch.tensor([default_scale])
        qx = torch.quantize_per_tensor(x, scale, torch.zeros(1), torch.qint8)
        return qx.int_repr().contiguous(), qx.q_scale()

    def quantize(self):
        """float parameters -> int8 buffers + scales (reference quantize_linear_variational.py:115-124,
        quantize_conv_variational.py:405-445), with the conv + BatchNorm folding of the bn_* attributes."""
        wn = self._wn
        mu, rho = getattr(self, "mu_" + wn).detach(), getattr(self, "rho_" + wn).detach()
        dev = mu.device
        mu = mu.float().clone(memory_format=torch.contiguous_format)
        sigma = torch.log1p(torch.exp(rho.float().clone(memory_format=torch.contiguous_format)))
        bn = self._nd > 0 and self.bn_weight is not None
        if bn:
            coef = (self.bn_weight / torch.sqrt(self.bn_running_var + self.bn_eps)).detach().float().to(dev)
            mu = mu * coef.view(-1, 1, 1, 1).expand(mu.shape)
            sigma = sigma * coef.view(-1, 1, 1, 1).expand(sigma.shape)
        qmu, s_mu = self.get_quantized_tensor(mu)
        qsg, s_sg = self.get_quantized_tensor(sigma)
        delattr(self, "mu_" + wn)
        delattr(self, "rho_" + wn)
        self.register_buffer("quantized_mu_weight", qmu.to(dev))
        self.register_buffer("quantized_sigma_weight", qsg.to(dev))
        self._q8_scales = (float(s_mu), float(s_sg))
        mu_b = sigma_b = None
        if self.bias:
            mu_b, sigma_b = self.mu_bias.detach().float(), torch.log1p(torch.exp(self.rho_bias.detach().float()))
            if bn:
                mu_b = (mu_b - self.bn_running_mean.detach().float().to(dev)) * coef + self.bn_bias.detach().float().to(dev)
                sigma_b = sigma_b * coef
        elif bn:  # no bias, but the folded BatchNorm leaves a deterministic one
            self.bias = True
            mu_b = coef * (-self.bn_running_mean.detach().float().to(dev)) + self.bn_bias.detach().float().to(dev)
        delattr(self, "mu_bias")
        delattr(self, "rho_bias")
        self.register_buffer("quantized_mu_bias", mu_b.contiguous() if mu_b is not None else None)
        self.register_buffer("quantized_sigma_bias", sigma_b.contiguous() if sigma_b is not None else None)
        if self.eps_bias is None and self.bias:
            self.register_buffer("eps_bias", torch.zeros(self._out_ch(), device=dev), persistent=False)
        for k in ("bn_weight", "bn_bias", "bn_running_mean", "bn_running_var", "bn_eps", "qint_quant", "quint_quant", "dequant"):
            if hasattr(self, k):
                delattr(self, k)
        self.__dict__.pop("_q8_pack", None)

    def get_extra_state(self):
        return {"q8_scales": self._q8_scales, "quant_dict": self._quant_entries()}

    def set_extra_state(self, state):
        self._q8_scales = tuple(state["q8_scales"]) if state.get("q8_scales") is not None else None
        self.quant_dict = state.get("quant_dict")

    def mu_weight_scale(self):
        return self._q8_scales[0]

    def sigma_weight_scale(self):
        return self._q8_scales[1]

    def kl_loss(self):
        return 0

    def set_prior(self, prior, kl_samples=1):
        from ... import priors as _priors
        if _priors.check_prior(prior) is not None:
            raise _lib.BtxError("non-Gaussian priors are not supported on the quantized layers: they are inference only (kl_loss() is 0); "
                                "set the prior on the float model before bnn_to_qbnn")
        return self

    def _out_ch(self):
        return self.out_features if self._nd == 0 else self.out_channels

    def _quant_entries(self):
        if self.quant_dict is None:
            return None
        return [_entry(e) for e in self.quant_dict]

    def _scales(self, normal_scale, default_scale, default_zero_point):
        """the five (scale, zero point) pairs of a forward: (s_eps, s_d, s_w, (s_x, z_x), (s_o, z_o))"""
        if self._q8_scales is None:
            raise _lib.BtxError("quantized layer used before quantize()")
        s_mu, s_sigma = self._q8_scales
        qd = self._quant_entries()
        if qd is None:
            s_eps = float(normal_scale)
            s_d = s_sigma * s_eps
            s_w = max(s_d, s_mu)
            return s_eps, s_d, s_w, (float(default_scale), int(default_zero_point)), (float(default_scale), int(default_zero_point))
        if len(qd) != 5:
            raise _lib.BtxError("quant_dict needs five (scale, zero point) entries: eps, mul, add, input, output")
        for name, (s, z) in zip(_ENTRY_NAMES[:3], qd[:3]):
            if z != 0:
                raise _lib.BtxError("quant_dict entry '%s' has zero point %d: the qint8 entries (eps, mul, add) must be symmetric" % (name, z))
        for name, (s, z) in zip(_ENTRY_NAMES, qd):
            if not s > 0:
                raise _lib.BtxError("quant_dict entry '%s' has a non-positive scale" % name)
        return qd[0][0], qd[1][0], qd[2][0], qd[3], qd[4]

    def _forward(self, input, enable_int8_compute, normal_scale, default_scale, default_zero_point, return_kl):
        if self.dnn_to_bnn_flag:
            return_kl = False
        if self.quant_dict is None and not enable_int8_compute:
            out = self._forward_dequantized(input)
        else:
            sc = self._scales(normal_scale, default_scale, default_zero_point)
            on_gpu = input.is_cuda and _base._BACKEND != "torch"
            if _base._BACKEND == "hip" and not input.is_cuda:
                raise _lib.BtxError("backend 'hip' needs CUDA (ROCm) tensors")
            out = self._forward_hip(input, sc) if on_gpu else self._forward_cpu(input, sc)
        if return_kl:
            return out, 0
        return out

    # ---- CPU: torch's quantized ops in the reference's order ---------------------------------------------------------
    def _torch_weights(self):
        s_mu, s_sigma = self._q8_scales
        return (torch._make_per_tensor_quantized_tensor(self.quantized_sigma_weight.cpu(), s_sigma, 0),
                torch._make_per_tensor_quantized_tensor(self.quantized_mu_weight.cpu(), s_mu, 0))

    def _draw_bias(self):
        if not self.bias:
            return None
        if self.quantized_sigma_bias is None:
            return self.quantized_mu_bias
        return self.quantized_mu_bias + (self.quantized_sigma_bias * self.eps_bias.data.normal_())

    def _forward_cpu(self, x, sc):
        s_eps, s_d, s_w, (s_x, z_x), (s_o, z_o) = sc
        if x.is_cuda:
            raise _lib.BtxError("backend 'torch' runs the quantized layers on CPU tensors only")
        q_sigma, q_mu = self._torch_weights()
        eps = torch.quantize_per_tensor(getattr(self, "eps_" + self._wn).data.normal_(), s_eps, 0, torch.qint8)
        weight = torch.ops.quantized.mul(q_sigma, eps, s_d, 0)
        weight = torch.ops.quantized.add(weight, q_mu, s_w, 0)
        bias = self._draw_bias()
        if isinstance(x, _q8.QTensor):
            x = x.as_torch_quint8()
        elif x.dtype != torch.quint8:
            x = torch.quantize_per_tensor(x.float(), s_x, z_x, torch.quint8)
        import torch.nn.quantized.functional as QF
        if self._nd == 0:
            return QF.linear(x, weight, bias, scale=s_o, zero_point=z_o).dequantize()
        if self.groups != 1:
            raise _lib.BtxError("quantized Conv2d supports groups = 1 only")
        out = QF.conv2d(x, weight, bias, self.stride, self.padding, self.dilation, self.groups, scale=s_o, zero_point=z_o)
        return torch.relu(out) if self.relu else out

    def _forward_dequantized(self, x):
        """enable_int8_compute=False (deprecated in the reference: 'for reducing model size only'): float compute on the
        dequantized weights, CPU tensors"""
        if x.is_cuda:
            raise _lib.BtxError("enable_int8_compute=False is a CPU-only mode; the GPU path of a quantized layer is its int8 compute")
        s_mu, s_sigma = self._q8_scales
        mu = self.quantized_mu_weight.float() * np.float32(s_mu).item()
        sigma = self.quantized_sigma_weight.float() * np.float32(s_sigma).item()
        weight = mu + (sigma * getattr(self, "eps_" + self._wn).data.normal_())
        bias = self._draw_bias()
        if self._nd == 0:
            return torch.nn.functional.linear(x, weight, bias)
        return torch.nn.functional.conv2d(x, weight, bias, self.stride, self.padding, self.dilation, self.groups)

    # ---- MI355X path ------------------------------------------------------------------------------------------------
    def _packed(self, dev):
        """the int8 weights in the kernels' GEMM-major order [N][taps][C] on `dev` (cached; keyed on the buffers' identity)"""
        qm, qs = self.quantized_mu_weight, self.quantized_sigma_weight
        key = (str(dev), qm.data_ptr(), qm._version, qs.data_ptr(), qs._version)
        st = self.__dict__.get("_q8_pack")
        if st is None or st[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.BtxError("quantized layer: run one forward before capturing a graph (the packed int8 weights are made then)")
            pack = (lambda t: t.to(dev).contiguous()) if self._nd == 0 else (lambda t: t.to(dev).permute(0, 2, 3, 1).contiguous())
            f = lambda t: t.detach().to(dev).float().contiguous() if t is not None else None  # noqa: E731
            st = (key, pack(qm), pack(qs), f(self.quantized_mu_bias) if self.bias else None,
                  f(self.quantized_sigma_bias) if self.bias else None)
            self.__dict__["_q8_pack"] = st
        return st[1:]

    def _eps_channels(self):
        """row length of the source float layer's BTX-RNG index space: its channel count, rounded up to 8 (base_variational_layer
        channel padding)"""
        c = self.in_features if self._nd == 0 else self.in_channels
        return c if c % 8 == 0 else (c + 7) // 8 * 8

    def _forward_hip(self, x, sc, noise=None, sample_idx=None, parts=False, residual=None, add=None):
        """noise: dict(eps_w[, eps_b]) in the logical layouts (what the float layer's materialize_noise returns) instead of BTX-RNG;
        parts=True: also return (W, S, b_i) of the sampling pre-pass; residual (a QTensor of the output's shape) with
        add = (scale or None, zero point, relu): the residual add in the contraction's store (btx_q8_contract_res)."""
        s_eps, s_d, s_w, (s_x, z_x), (s_o, z_o) = sc
        if self.__dict__.get("_btx_lanes", 1) > 1:
            raise _lib.BtxError("MC sample lanes > 1 are not supported by quantized (INT8) layers: use lanes=1")
        if self._nd > 0 and self.groups != 1:
            raise _lib.BtxError("quantized Conv2d supports groups = 1 only (got groups=%d)" % self.groups)
        if isinstance(x, _q8.QTensor):
            xq = x
        else:
            if self._nd == 0 and x.dim() != 2:
                lead = x.shape[:-1]
                out = self._forward_hip(x.reshape(-1, x.shape[-1]), sc, noise, sample_idx, parts)
                if parts:
                    return (out[0].reshape(*lead, -1),) + out[1:]
                return out.reshape(*lead, -1)
            xq = _q8.quantize_act(x, s_x, z_x)
        s_x, z_x = xq.scale, xq.zero_point
        mu_p, sg_p, mu_b, sigma_b = self._packed(xq.device)
        n = self._out_ch()
        kernel = (1, 1) if self._nd == 0 else _pair(self.kernel_size)
        taps = kernel[0] * kernel[1]
        c = mu_p.shape[-1]
        if xq.q.dim() != (2 if self._nd == 0 else 4) or xq.q.shape[1] != c:
            raise _lib.BtxError("quantized layer: input shape %s does not match %d input channels" % (tuple(xq.q.shape), c))
        if sample_idx is None:
            sample_idx = self._btx_sample
            self.__dict__["_btx_sample"] = sample_idx + 1
        chain = _q8.make_chain(self._q8_scales[1], self._q8_scales[0], s_eps, s_d, s_w, s_x)
        eps_w = eps_b = None
        if noise is not None:
            e = noise["eps_w"].to(xq.device, torch.float32)
            eps_w = e.contiguous() if self._nd == 0 else e.permute(0, 2, 3, 1).contiguous()
            if sigma_b is not None:
                eps_b = noise["eps_b"].to(xq.device, torch.float32).contiguous()
        W, S, b_i = _q8.sample_weights(mu_p, sg_p, mu_b, sigma_b, n, taps, c, self._eps_channels() if noise is None else c, chain,
                                       _rng.seed(), sample_idx, self._btx_layer_id, getattr(self, "_btx_sample_dev", None), eps_w, eps_b)
        f = np.float32
        mult = float(f(f(s_x) * f(s_w)) / f(s_o))
        if residual is not None:
            if self._nd == 0:
                raise _lib.BtxError("the residual add is an epilogue of the quantized Conv2d only")
            if not isinstance(residual, _q8.QTensor):
                raise _lib.BtxError("quantized conv: on the GPU the residual is a q8.QTensor (got %s)" % type(residual).__name__)
            s_add, z_add, relu_add = add
            s_add = max(float(s_o), residual.scale) if s_add is None else float(s_add)
            p = _q8.make_add(s_o, z_o, residual.scale, residual.zero_point, s_add, z_add, relu_add)
            o = _q8.contract(xq.q, z_x, W, S, b_i, n, kernel, _pair(self.stride), _pair(self.padding), _pair(self.dilation), mult, z_o,
                             bool(self.relu), False, s_o, residual=residual.q, add=p)
            out = _q8.QTensor(o, s_add, z_add)
        elif self._nd == 0:
            out = _q8.contract(xq.q, z_x, W, S, b_i, n, (1, 1), (1, 1), (0, 0), (1, 1), mult, z_o, False, True, s_o)
        else:
            o = _q8.contract(xq.q, z_x, W, S, b_i, n, kernel, _pair(self.stride), _pair(self.padding), _pair(self.dilation), mult, z_o,
                             bool(self.relu), False, s_o)
            out = _q8.QTensor(o, s_o, z_o)
        if parts:
            return out, W, S, b_i
        return out

    def forward_int8(self, x, noise=None, sample_idx=None, parts=False, normal_scale=6 / 255, default_scale=None, default_zero_point=128,
                     residual=None, add_relu=True, add_scale=None, add_zero_point=0):
        """the GPU forward with explicit noise and / or a pinned sample index (tests, parity runs); with `residual` the fused
        residual add of forward_add"""
        if default_scale is None:
            default_scale = 0.2 if self._nd == 0 else 0.1
        return self._forward_hip(x, self._scales(normal_scale, default_scale, default_zero_point), noise, sample_idx, parts, residual,
                                 (add_scale, int(add_zero_point), bool(add_relu)))


class QuantizedLinearReparameterization(_QuantizedReparameterization):
    """reference layers/variational_layers/quantize_linear_variational.py:44-224"""
    _nd = 0

    def __init__(self, in_features, out_features):
        super().__init__()
        self._setup(in_features, out_features, 1, 1, 0, 1, 1, True)

    def forward(self, input, enable_int8_compute=True, normal_scale=6 / 255, default_scale=0.2, default_zero_point=128, return_kl=True):
        """returns the DEQUANTIZED f32 output (and 0 for the KL), as the reference's quantized Linear does"""
        return self._forward(input, enable_int8_compute, normal_scale, default_scale, default_zero_point, return_kl)


class QuantizedConv2dReparameterization(_QuantizedReparameterization):
    """reference layers/variational_layers/quantize_conv_variational.py:303-552"""
    _nd = 2

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)

    def forward(self, input, enable_int8_compute=True, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128, return_kl=True):
        """returns the quantized output (a q8.QTensor on the GPU, a torch.quint8 tensor on the CPU) and 0 for the KL"""
        return self._forward(input, enable_int8_compute, normal_scale, default_scale, default_zero_point, return_kl)

    def forward_add(self, input, residual, relu=True, scale=None, zero_point=0, normal_scale=6 / 255, default_scale=0.1,
                    default_zero_point=128):
        """conv, then the quantized add of `residual` (and a ReLU): quantized.add[_relu](conv(input), residual, scale, zero_point),
        scale=None -> the reference's max(conv output scale, residual scale).  GPU: ONE btx_q8_contract_res launch behind the
        sampling pre-pass; CPU: the conv, then torch's quantized add.  Returns the quantized sum."""
        sc = self._scales(normal_scale, default_scale, default_zero_point)
        if _base._BACKEND == "hip" and not input.is_cuda:
            raise _lib.BtxError("backend 'hip' needs CUDA (ROCm) tensors")
        if input.is_cuda and _base._BACKEND != "torch":
            return self._forward_hip(input, sc, residual=residual, add=(scale, int(zero_point), bool(relu)))
        out = self._forward_cpu(input, sc)
        if isinstance(residual, _q8.QTensor):
            residual = residual.as_torch_quint8()
        return _q8.add(out, residual, max(out.q_scale(), residual.q_scale()) if scale is None else scale, zero_point, relu)
