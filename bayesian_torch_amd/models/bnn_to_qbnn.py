"""bnn_to_qbnn() — replace the Bayesian layers of a model by their INT8 twins (reference models/bnn_to_qbnn.py:96-237).

Kept from the reference: the in-place traversal; `Quantized<ClassName>` as the twin's class; a prepared and converted layer
(`layer.prepare()` -> torch.quantization.prepare -> calibration forwards -> torch.quantization.convert) hands its seven stubs'
(scale, zero point) pairs over as `quant_dict` = [eps, mul, add, input, output]; fuse_conv_bn=True folds `bn1` into `conv1`,
`bn2` into `conv2`, `bn3` into `conv3` and `downsample[1]` into `downsample[0]` and leaves nn.Identity() where the BatchNorm was.

Quantized here: LinearReparameterization and Conv2dReparameterization, and with `flipout=True` LinearFlipout and Conv2dFlipout
(reference models/bnn_to_qbnn.py: the Flipout twins; their twelve stubs hand over ten entries, qint_quant[2:] + quint_quant).  The
default flipout=False leaves a Flipout layer as it is.  Every other layer kind (Conv1d / 3d / Transpose, LSTM and the Linear layers
inside one, BatchNorm) is left as it is.  The twin keeps its source layer's BTX-RNG layer id and sample counter: at the same seed
and sample index it draws the eps (and a Flipout twin the signs) its float source would."""
import torch
import torch.nn as nn

from .. import layers as bayesian_layers

_KINDS = {"LinearReparameterization": "reparam", "Conv2dReparameterization": "reparam", "LinearFlipout": "flipout",
          "Conv2dFlipout": "flipout"}


def _convertible(m, flipout=False):
    fam = _KINDS.get(type(m).__name__)
    if fam is None or not hasattr(m, "_btx_layer_id") or getattr(m, "_family", None) != fam:
        return False
    return fam == "reparam" or flipout


def _stub_entries(d):
    """[eps, mul, add, input, output] (Flipout: the ten entries eps, delta and the eight quint8 stubs) from the layer's converted
    stubs, or None when there are none"""
    if not getattr(d, "quant_prepare", False) or not hasattr(d, "qint_quant"):
        return None
    stubs = list(d.qint_quant)[2:] + list(d.quint_quant)
    if not all(hasattr(s, "scale") and hasattr(s, "zero_point") for s in stubs):
        return None  # prepared but never converted: no calibration result to carry
    return [(float(s.scale), int(s.zero_point)) for s in stubs]


def _plain(t):
    return t.detach().clone(memory_format=torch.contiguous_format)


def _twin(d, bn=None):
    cls = getattr(bayesian_layers, "Quantized" + type(d).__name__)
    has_bias = d.mu_bias is not None
    if d._nd == 0:
        q = cls(in_features=d.in_features, out_features=d.out_features)
        if not has_bias:
            q.bias = False
            q.mu_bias = q.rho_bias = None
            q.eps_bias = None
    else:
        q = cls(in_channels=d.in_channels, out_channels=d.out_channels, kernel_size=d.kernel_size, stride=d.stride,
                padding=d.padding, dilation=d.dilation, groups=d.groups, bias=has_bias)
    mu, rho = d._w()
    dev = mu.device
    q.to(dev)
    wn = q._wn
    getattr(q, "mu_" + wn).data = _plain(mu)
    getattr(q, "rho_" + wn).data = _plain(rho)
    if has_bias:
        q.mu_bias.data = _plain(d.mu_bias)
        q.rho_bias.data = _plain(d.rho_bias)
    q._btx_layer_id = d._btx_layer_id
    q._btx_sample = d._btx_sample
    q.quant_dict = _stub_entries(d)
    if bn is not None:
        ones = torch.ones_like(bn.running_var)
        q.bn_weight = _plain(bn.weight) if bn.weight is not None else ones
        q.bn_bias = _plain(bn.bias) if bn.bias is not None else torch.zeros_like(ones)
        q.bn_running_mean, q.bn_running_var, q.bn_eps = _plain(bn.running_mean), _plain(bn.running_var), bn.eps
    q.quantize()
    q.train(d.training)
    if d.dnn_to_bnn_flag:
        q.dnn_to_bnn_flag = True
    return q


def qbnn_linear_layer(d):
    return _twin(d)


def qbnn_conv_layer(d):
    return _twin(d)


def batch_norm_folding(conv, bn):
    return _twin(conv, bn)


def _foldable(conv, bn, flipout=False):
    return _convertible(conv, flipout) and conv._nd == 2 and isinstance(bn, nn.BatchNorm2d) and bn.running_var is not None


def bnn_to_qbnn(m, fuse_conv_bn=False, flipout=False):
    for name, sub in m.named_modules():  # before anything is converted: the model stays as it was
        if getattr(sub, "_btx_dropout", False):
            from .._lib import BtxError
            raise BtxError("bnn_to_qbnn: %r is a %s; Monte-Carlo dropout has no INT8 twin (BTX-DROP v1 defines f32 and bf16)"
                           % (name, type(sub).__name__))
    mods = m._modules
    if fuse_conv_bn:
        for c, b in (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3")):
            if c in mods and b in mods and _foldable(mods[c], mods[b], flipout):
                setattr(m, c, batch_norm_folding(mods[c], mods[b]))
                setattr(m, b, nn.Identity())
        ds = mods.get("downsample")
        if isinstance(ds, nn.Sequential) and len(ds) == 2 and _foldable(ds[0], ds[1], flipout):
            ds[0] = batch_norm_folding(ds[0], ds[1])
            ds[1] = nn.Identity()
    for name, child in list(mods.items()):
        if child is None or getattr(child, "_btx_q8", False):
            continue
        if getattr(child, "_family", None) == "lrt" and hasattr(child, "_btx_layer_id"):
            from .._lib import BtxError
            raise BtxError("bnn_to_qbnn: %r is a %s; local reparameterization layers have no INT8 twin" % (name, type(child).__name__))
        if _convertible(child, flipout):
            setattr(m, name, qbnn_linear_layer(child) if child._nd == 0 else qbnn_conv_layer(child))
        elif hasattr(child, "ih") and hasattr(child, "hh") and hasattr(child, "fused_sequence"):
            continue  # a Bayesian LSTM stays whole: its inner Linear layers are part of its recurrence
        elif child._modules:
            bnn_to_qbnn(child, fuse_conv_bn=fuse_conv_bn, flipout=flipout)
    return
