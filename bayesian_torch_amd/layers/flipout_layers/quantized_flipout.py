"""QuantizedLinearFlipout / QuantizedConv2dFlipout — INT8 inference twins of the Flipout layers (reference
layers/flipout_layers/quantized_linear_flipout.py:48-261, quantized_conv_flipout.py:257-514).

Arithmetic: BTX-Q8 v1, "Flipout" (DESIGN.md §13).  The reference's forward is six quantized ops (mean conv, quantized.mul of the
input with the quantized signs, quantized.mul of sigma with eps, perturbed conv, quantized.mul with the output signs, quantized.add)
on the ten (scale, zero point) entries of `quant_dict`.  On a CUDA tensor that is the activation quantize (skipped when the input
arrives quantized), one weight pre-pass (btx_q8_sample_delta) and ONE contraction launch (btx_q8_contract_flipout); on a CPU
tensor it is the reference's own chain of torch quantized ops with eps and signs drawn from the torch generator.  Storage, state
dict and the conv + BatchNorm folding are those of the Reparameterization twins (variational_layers/quantized_variational.py)."""
import numpy as np
import torch

from .. import base_variational_layer as _base
from ..variational_layers.quantized_variational import _QuantizedReparameterization, _pair
from ... import _lib
from ... import functional as BF
from ... import q8 as _q8
from ... import rng as _rng

__all__ = ["QuantizedLinearFlipout", "QuantizedConv2dFlipout"]

ENTRY_NAMES = ("eps", "delta", "input", "mean output", "input signs", "output signs", "signed input", "perturbed output",
               "signed perturbed output", "output")


class _QuantizedFlipout(_QuantizedReparameterization):

    # ---- the ten entries and the two bias vectors of a forward ----------------------------------------------------
    def _entries(self, normal_scale, default_scale, default_zero_point):
        """-> (e, calibrated): e = ten (scale, zero point) pairs, the reference's defaults when quant_dict is None"""
        if self._q8_scales is None:
            raise _lib.BtxError("quantized layer used before quantize()")
        qd = self._quant_entries()
        if qd is None:
            d = (float(default_scale), int(default_zero_point))
            return [(float(normal_scale), 0), (self._q8_scales[1] * float(normal_scale), 0)] + [d] * 8, False
        if len(qd) != 10:
            raise _lib.BtxError("quant_dict of a Flipout twin needs ten (scale, zero point) entries: " + ", ".join(ENTRY_NAMES))
        for name, (s, z) in zip(ENTRY_NAMES[:2], qd[:2]):
            if z != 0:
                raise _lib.BtxError("quant_dict entry '%s' has zero point %d: the qint8 entries (eps, delta) must be symmetric" % (name, z))
        for name, (s, z) in zip(ENTRY_NAMES, qd):
            if not s > 0:
                raise _lib.BtxError("quant_dict entry '%s' has a non-positive scale" % name)
            if not 0 <= z <= 255:
                raise _lib.BtxError("quant_dict entry '%s' has zero point %d outside [0, 255]" % (name, z))
        return qd, True

    def _bias_kinds(self, calibrated):
        """which f32 vector each GEMM gets, as the reference literally does (reference deviations): the default
        path gives mu_b to the mean GEMM and sigma_b * eps_b to the perturbed one; the calibrated Conv2d path gives mu_b to both;
        the calibrated Linear path gives sigma_b * eps_b to both"""
        if not self.bias:
            return "none", "none"
        rand = "sigma_eps" if self.quantized_sigma_bias is not None else "none"
        if not calibrated:
            return "mu", rand
        return ("mu", "mu") if self._nd > 0 else (rand, rand)

    def _check(self):
        if self.__dict__.get("_btx_lanes", 1) > 1:
            raise _lib.BtxError("MC sample lanes > 1 are not supported by quantized (INT8) layers: use lanes=1")
        if self._nd > 0 and self.groups != 1:
            raise _lib.BtxError("quantized Conv2d supports groups = 1 only (got groups=%d)" % self.groups)

    def _forward(self, input, normal_scale, default_scale, default_zero_point, return_kl):
        if self.dnn_to_bnn_flag:
            return_kl = False
        e, cal = self._entries(normal_scale, default_scale, default_zero_point)
        on_gpu = input.is_cuda and _base._BACKEND != "torch"
        if _base._BACKEND == "hip" and not input.is_cuda:
            raise _lib.BtxError("backend 'hip' needs CUDA (ROCm) tensors")
        out = self._forward_hip(input, e, cal) if on_gpu else self._forward_cpu(input, e, cal)
        if return_kl:
            return out, 0
        return out

    # ---- CPU: torch's quantized ops in the reference's order ---------------------------------------------------------
    def _forward_cpu(self, x, e, cal, noise=None, parts=False):
        """noise: dict(eps_w[, eps_b], sign_in, sign_out) in the logical layouts instead of the torch generator"""
        import torch.nn.quantized.functional as QF
        if x.is_cuda:
            raise _lib.BtxError("backend 'torch' runs the quantized layers on CPU tensors only")
        self._check()
        q_sigma, q_mu = self._torch_weights()
        if isinstance(x, _q8.QTensor):
            x = x.as_torch_quint8()
        elif x.dtype != torch.quint8:
            x = torch.quantize_per_tensor(x.float(), e[2][0], e[2][1], torch.quint8)
        kinds = self._bias_kinds(cal)
        geom = () if self._nd == 0 else (self.stride, self.padding, self.dilation, 1)
        conv = QF.linear if self._nd == 0 else QF.conv2d
        nz = noise or {}

        def draw_eps():
            if "eps_w" in nz:
                return nz["eps_w"].float().cpu()
            return getattr(self, "eps_" + self._wn).data.normal_().cpu()

        def bias_of(kind, eps_b):
            if kind == "none":
                return None
            return self.quantized_mu_bias.cpu() if kind == "mu" else self.quantized_sigma_bias.cpu() * eps_b

        def draw_eps_b():
            if "sigma_eps" not in kinds:
                return None
            return nz["eps_b"].float().cpu() if "eps_b" in nz else self.eps_bias.data.normal_().cpu()

        def draw_sign(name, shape):
            if name in nz:
                return nz[name].float().cpu().reshape(shape)
            return torch.zeros(shape).uniform_(-1, 1).sign()

        if cal:  # reference order: eps, the bias noise, the mean conv, then the signs
            eps = draw_eps()
            eps_b = draw_eps_b()
            o1 = conv(x, q_mu, bias_of(kinds[0], eps_b), *geom, scale=e[3][0], zero_point=e[3][1])
            sign_in, sign_out = draw_sign("sign_in", x.shape), draw_sign("sign_out", o1.shape)
        else:    # default path: the mean conv, the signs, then eps and the bias noise
            o1 = conv(x, q_mu, bias_of(kinds[0], None), *geom, scale=e[3][0], zero_point=e[3][1])
            sign_in, sign_out = draw_sign("sign_in", x.shape), draw_sign("sign_out", o1.shape)
            eps = draw_eps()
            eps_b = draw_eps_b()
        eps_q = torch.quantize_per_tensor(eps, e[0][0], e[0][1], torch.qint8)
        delta = torch.ops.quantized.mul(q_sigma, eps_q, e[1][0], e[1][1])
        s_in = torch.quantize_per_tensor(sign_in, e[4][0], e[4][1], torch.quint8)
        s_out = torch.quantize_per_tensor(sign_out, e[5][0], e[5][1], torch.quint8)
        xp = torch.ops.quantized.mul(x, s_in, e[6][0], e[6][1])
        p = conv(xp, delta, bias_of(kinds[1], eps_b), *geom, scale=e[7][0], zero_point=e[7][1])
        p2 = torch.ops.quantized.mul(p, s_out, e[8][0], e[8][1])
        relu = self._nd > 0 and self.relu
        out = (torch.ops.quantized.add_relu if relu else torch.ops.quantized.add)(o1, p2, e[9][0], e[9][1])
        if self._nd == 0:
            out = out.dequantize()
        if parts:
            return out, dict(d_i=delta, xp=xp, o1=o1, p=p, p2=p2)
        return out

    # ---- MI355X path ------------------------------------------------------------------------------------------------
    def _mean_image(self, mu_p):
        """(W_mu, S_mu): the mean weights in the contraction's image layout with their row sums.  They do not change between
        forwards: made once through the v1 pre-pass with a zero sigma (W = q(mu_i * s_mu, s_mu) = mu_i) and cached like _q8_pack."""
        key = (str(mu_p.device), mu_p.data_ptr(), mu_p._version)
        st = self.__dict__.get("_q8_mean")
        if st is None or st[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.BtxError("quantized layer: run one forward before capturing a graph (the packed int8 weights are made then)")
            n, taps, c = mu_p.shape[0], mu_p.numel() // (mu_p.shape[0] * mu_p.shape[-1]), mu_p.shape[-1]
            s_mu = self._q8_scales[0]
            chain = _q8.make_chain(1.0, s_mu, 1.0, 1.0, s_mu, 1.0)
            W, S, _ = _q8.sample_weights(mu_p, torch.zeros_like(mu_p), None, None, n, taps, c, self._eps_channels(), chain, 0, 0, 0)
            st = (key, W, S)
            self.__dict__["_q8_mean"] = st
        return st[1], st[2]

    def materialize_noise(self, sample_idx, x_shape, out_shape):
        """the noise BTX-RNG v1 defines for MC sample `sample_idx` of this layer — what the kernels regenerate — in the logical
        layouts: dict(eps_w, eps_b, sign_in, sign_out).  Index spaces of the float source layer: eps rows and input-sign rows of
        its channel count rounded up to 8."""
        dev = self.quantized_mu_weight.device
        seed, lid = _rng.seed(), self._btx_layer_id
        n, c, cp = self._out_ch(), self.quantized_mu_weight.shape[1], self._eps_channels()
        taps = self.quantized_mu_weight[0, 0].numel()
        e = BF.fill_eps_hip(n * taps * cp, dev, seed, sample_idx, lid, _lib.STREAM_EPS_W).reshape(n, taps, cp)[:, :, :c]
        d = {"eps_b": BF.fill_eps_hip(n, dev, seed, sample_idx, lid, _lib.STREAM_EPS_B)}
        pix = int(np.prod(x_shape)) // c
        si = BF.fill_sign_hip(pix * cp, dev, seed, sample_idx, lid, _lib.STREAM_SIGN_IN).reshape(pix, cp)[:, :c]
        so = BF.fill_sign_hip(int(np.prod(out_shape)), dev, seed, sample_idx, lid, _lib.STREAM_SIGN_OUT)
        if self._nd == 0:
            d["eps_w"] = e.reshape(n, c).contiguous()
            d["sign_in"], d["sign_out"] = si.reshape(tuple(x_shape)), so.reshape(tuple(out_shape))
        else:
            kh, kw = _pair(self.kernel_size)
            d["eps_w"] = e.reshape(n, kh, kw, c).permute(0, 3, 1, 2).contiguous()
            d["sign_in"] = si.reshape(x_shape[0], x_shape[2], x_shape[3], c).permute(0, 3, 1, 2)
            d["sign_out"] = so.reshape(out_shape[0], out_shape[2], out_shape[3], n).permute(0, 3, 1, 2)
        return d

    def _forward_hip(self, x, e, cal, noise=None, sample_idx=None, parts=False):
        """noise: dict(eps_w[, eps_b], sign_in, sign_out) in the logical layouts instead of BTX-RNG; parts=True: also return a dict
        of the pre-pass outputs (W_mu, S_mu, D, S_d, bm_i, bp_i) and, without explicit noise, `noise` (materialize_noise)."""
        self._check()
        if isinstance(x, _q8.QTensor):
            xq = x
        else:
            if self._nd == 0 and x.dim() != 2:
                lead = x.shape[:-1]
                out = self._forward_hip(x.reshape(-1, x.shape[-1]), e, cal, noise, sample_idx, parts)
                if parts:
                    return (out[0].reshape(*lead, -1),) + out[1:]
                return out.reshape(*lead, -1)
            xq = _q8.quantize_act(x, e[2][0], e[2][1])
        s_x, z_x = xq.scale, xq.zero_point
        mu_p, sg_p, mu_b, sigma_b = self._packed(xq.device)
        n = self._out_ch()
        kernel = (1, 1) if self._nd == 0 else _pair(self.kernel_size)
        taps = kernel[0] * kernel[1]
        c = mu_p.shape[-1]
        if xq.q.dim() != (2 if self._nd == 0 else 4) or xq.q.shape[1] != c:
            raise _lib.BtxError("quantized layer: input shape %s does not match %d input channels" % (tuple(xq.q.shape), c))
        if xq.q.dim() == 2 and not xq.q.is_contiguous():
            xq = _q8.QTensor(xq.q.contiguous(), s_x, z_x)
        if sample_idx is None:
            sample_idx = self._btx_sample
            self.__dict__["_btx_sample"] = sample_idx + 1
        s_mu, s_sigma = self._q8_scales
        W_mu, S_mu = self._mean_image(mu_p)
        kinds = self._bias_kinds(cal)
        eps_w = eps_b = sign_in = sign_out = None
        cl = (lambda t: t.contiguous()) if self._nd == 0 else (lambda t: t.permute(0, 2, 3, 1).contiguous())
        if noise is not None:
            eps_w = cl(noise["eps_w"].to(xq.device, torch.float32))
            if "sigma_eps" in kinds:
                eps_b = noise["eps_b"].to(xq.device, torch.float32).contiguous()
            sign_in = cl(noise["sign_in"].to(xq.device).to(torch.int8))
            sign_out = cl(noise["sign_out"].to(xq.device).to(torch.int8))
            n_out = xq.q.shape[0] * n
            if self._nd > 0:
                for i in (0, 1):
                    ext = (xq.q.shape[2 + i] + 2 * _pair(self.padding)[i] - _pair(self.dilation)[i] * (kernel[i] - 1) - 1) \
                        // _pair(self.stride)[i] + 1
                    n_out *= max(ext, 0)
            if sign_in.numel() != xq.q.numel() or sign_out.numel() != n_out:   # the kernel reads them unchecked
                raise _lib.BtxError("quantized layer: sign_in / sign_out must have the input's / the output's shape")
        sample_dev = getattr(self, "_btx_sample_dev", None)
        eps_c = self._eps_channels()
        D, S_d, bm_i, bp_i = _q8.sample_delta(sg_p, mu_b, sigma_b, n, taps, c, eps_c if noise is None else c, s_sigma, s_mu, s_x, e,
                                              kinds[0], kinds[1], _rng.seed(), sample_idx, self._btx_layer_id, sample_dev, eps_w, eps_b)
        flip = _q8.make_flipout(s_x, z_x, s_mu, e)
        relu = self._nd > 0 and bool(self.relu)
        add = _q8.make_add(e[3][0], e[3][1], e[8][0], e[8][1], e[9][0], e[9][1], relu)
        geom = ((1, 1), (0, 0), (1, 1)) if self._nd == 0 else (_pair(self.stride), _pair(self.padding), _pair(self.dilation))
        o = _q8.contract_flipout(xq.q, W_mu, S_mu, bm_i, D, S_d, bp_i, n, kernel, geom[0], geom[1], geom[2], flip, add, _rng.seed(),
                                 sample_idx, self._btx_layer_id, eps_c, sample_dev, sign_in, sign_out, out_f32=self._nd == 0)
        out = o if self._nd == 0 else _q8.QTensor(o, e[9][0], e[9][1])
        if parts:
            d = dict(W_mu=W_mu, S_mu=S_mu, D=D, S_d=S_d, bm_i=bm_i, bp_i=bp_i)
            if noise is None:
                d["noise"] = self.materialize_noise(sample_idx, tuple(xq.q.shape), tuple(o.shape))
            return out, d
        return out

    def forward_int8(self, x, noise=None, sample_idx=None, parts=False, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128):
        """the forward with explicit noise (dict(eps_w, eps_b, sign_in, sign_out), logical layouts) and / or a pinned sample
        index (tests, parity runs): the GPU launches on a CUDA tensor, torch's quantized ops on a CPU tensor"""
        e, cal = self._entries(normal_scale, default_scale, default_zero_point)
        if x.is_cuda:
            return self._forward_hip(x, e, cal, noise, sample_idx, parts)
        return self._forward_cpu(x, e, cal, noise, parts)


class QuantizedLinearFlipout(_QuantizedFlipout):
    """reference layers/flipout_layers/quantized_linear_flipout.py:48-261"""
    _nd = 0

    def __init__(self, in_features, out_features):
        super().__init__()
        self._setup(in_features, out_features, 1, 1, 0, 1, 1, True)

    def forward(self, x, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128, return_kl=True):
        """returns the DEQUANTIZED f32 output (and 0 for the KL), as the reference's quantized Linear does"""
        return self._forward(x, normal_scale, default_scale, default_zero_point, return_kl)


class QuantizedConv2dFlipout(_QuantizedFlipout):
    """reference layers/flipout_layers/quantized_conv_flipout.py:257-514"""
    _nd = 2

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False):
        super().__init__()
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)

    def forward(self, x, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128, return_kl=True):
        """returns the quantized output (a q8.QTensor on the GPU, a torch.quint8 tensor on the CPU) and 0 for the KL"""
        return self._forward(x, normal_scale, default_scale, default_zero_point, return_kl)

    def forward_add(self, input, residual, relu=True, scale=None, zero_point=0, normal_scale=6 / 255, default_scale=0.1,
                    default_zero_point=128):
        """conv, then q8.add of `residual` (and a ReLU): two launches behind the pre-pass on the GPU (a residual operand in the
        Flipout store is not built).  scale=None -> the reference's max(conv output scale, residual scale)."""
        out = self._forward(input, normal_scale, default_scale, default_zero_point, False)
        if isinstance(residual, _q8.QTensor) and not isinstance(out, _q8.QTensor):
            residual = residual.as_torch_quint8()
        return _q8.add(out, residual, max(out.q_scale(), residual.q_scale()) if scale is None else scale, zero_point, relu)
