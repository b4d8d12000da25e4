"""QResNet — an INT8 ResNet whose activations stay quantized from the stem to the head (reference
models/bayesian/quantized_resnet_variational_large.py:90-249: Bottleneck, QResNet, qresnet18 ... qresnet101).

Kept from the reference: the module names (conv1, bn1, relu, maxpool, layer1..4, avgpool, fc; downsample), the op chain
conv -> [bn] -> relu -> maxpool -> blocks -> avgpool -> view -> fc, and the residual add
`quantized.add(out, residual, max(out.q_scale(), residual.q_scale()), 0)` followed by a ReLU.

One `forward` serves both devices through the q8.* functions: CUDA tensors travel as q8.QTensor through the HIP kernels of
btx_q8.hip (the residual add rides in the store of the block's last conv: btx_q8_contract_res), CPU tensors as torch.quint8
through torch's quantized engine.  A QResNet is built from one of this repo's models.resnet ResNets:

    m = resnet18(); dnn_to_bnn(m, {... "type": "Reparameterization" or "Flipout" ...}); q = to_qresnet(m)

A BatchNorm2d that was not folded into its conv (fuse_conv_bn=False) is refused: the reference swaps in torch's quantized
BatchNorm there, which has no GPU form here."""
import torch.nn as nn

from .. import _lib
from .. import q8
from .bnn_to_qbnn import bnn_to_qbnn
from .dnn_to_bnn import dnn_to_bnn
from . import resnet as _resnet

__all__ = ["QBasicBlock", "QBottleneck", "QResNet", "to_qresnet", "qresnet18", "qresnet34", "qresnet50", "qresnet101"]


def _out(o):
    return o[0] if isinstance(o, tuple) else o


def _is_qconv(m):
    return type(m).__name__ in ("QuantizedConv2dReparameterization", "QuantizedConv2dFlipout")


class _QBlock(nn.Module):
    """the modules of a models.resnet block under their own names; `fuse_add`: the residual add (and the block's last ReLU) in
    the store of the last conv — False: conv, then q8.add (the same bytes, one more launch and one more pass over the tensor)"""
    _convs = ()

    def __init__(self, src):
        super().__init__()
        for name, child in src._modules.items():
            setattr(self, name, child)
        if "downsample" not in src._modules:
            self.downsample = None
        self.stride = src.stride
        self.fuse_add = True
        for c in self._convs:
            conv = getattr(self, c)
            if not _is_qconv(conv):
                raise _lib.BtxError("to_qresnet: %s.%s is a %s, not a quantized Conv2d (convert the model with "
                                    "dnn_to_bnn(type='Reparameterization' or 'Flipout') first)" % (type(src).__name__, c, type(conv).__name__))
        for c in self._convs[:-1]:
            getattr(self, c).relu = True   # a ReLU follows directly: clamp in the conv's store

    def forward(self, x):
        out = x
        for c, b in zip(self._convs[:-1], self._bns[:-1]):
            out = getattr(self, b)(_out(getattr(self, c)(out)))
        residual = x
        if self.downsample is not None:
            residual = self.downsample[1](_out(self.downsample[0](x)))
        last, bn = getattr(self, self._convs[-1]), getattr(self, self._bns[-1])
        if self.fuse_add and isinstance(bn, nn.Identity):
            return last.forward_add(out, residual, relu=True, scale=None, zero_point=0)
        out = bn(_out(last(out)))
        return q8.add(out, residual, max(out.q_scale(), residual.q_scale()), 0, relu=True)


class QBasicBlock(_QBlock):
    expansion = 1
    _convs, _bns = ("conv1", "conv2"), ("bn1", "bn2")


class QBottleneck(_QBlock):
    expansion = 4
    _convs, _bns = ("conv1", "conv2", "conv3"), ("bn1", "bn2", "bn3")


_BLOCKS = {"BasicBlock": QBasicBlock, "Bottleneck": QBottleneck}


class QResNet(nn.Module):
    """reference quantized_resnet_variational_large.py:142-228, over the (already quantized) modules of `src`"""

    def __init__(self, src):
        super().__init__()
        self.conv1, self.bn1, self.relu, self.maxpool = src.conv1, src.bn1, src.relu, src.maxpool
        if not _is_qconv(self.conv1):
            raise _lib.BtxError("to_qresnet: conv1 is a %s, not a quantized Conv2d" % type(self.conv1).__name__)
        if isinstance(self.bn1, nn.Identity):
            self.conv1.relu = True
        for name in ("layer1", "layer2", "layer3", "layer4"):
            blocks = []
            for b in getattr(src, name):
                cls = _BLOCKS.get(type(b).__name__)
                if cls is None:
                    raise _lib.BtxError("to_qresnet: %s holds a %s; BasicBlock or Bottleneck expected" % (name, type(b).__name__))
                blocks.append(cls(b))
            setattr(self, name, nn.Sequential(*blocks))
        self.avgpool, self.fc = src.avgpool, src.fc

    def set_fuse_add(self, on):
        for m in self.modules():
            if isinstance(m, _QBlock):
                m.fuse_add = bool(on)
        return self

    def forward(self, x):
        x = self.bn1(_out(self.conv1(x)))
        if not self.conv1.relu:
            x = q8.relu(x)
        mp = self.maxpool
        x = q8.max_pool2d(x, mp.kernel_size, mp.stride, mp.padding)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for block in layer:
                x = block(x)
        ap = self.avgpool
        x = q8.avg_pool2d(x, ap.kernel_size, ap.stride, ap.padding, ap.ceil_mode)
        x = x.view(x.size(0), -1)
        return _out(self.fc(x))


def to_qresnet(model, fuse_conv_bn=True):
    """models.resnet ResNet after dnn_to_bnn(type="Reparameterization" or "Flipout") -> QResNet over the same modules (bnn_to_qbnn
    in place, Flipout layers included; a Flipout block's residual add is conv + q8.add)"""
    bnn_to_qbnn(model, fuse_conv_bn=fuse_conv_bn, flipout=True)
    for name, m in model.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            raise _lib.BtxError("to_qresnet: float BatchNorm2d '%s' is left between quantized layers; fold it with fuse_conv_bn=True "
                                "(a quantized BatchNorm is not implemented)" % name)
    return QResNet(model)


_PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0,
          "type": "Reparameterization", "moped_enable": False, "moped_delta": 0.5}


def _make(name, num_classes, bnn_prior_parameters):
    m = getattr(_resnet, name)(num_classes=num_classes).eval()
    # bnn_prior_parameters={"type": "Flipout"} builds the Flipout QResNet; any other (or no) type the Reparameterization one
    kind = "Flipout" if (bnn_prior_parameters or {}).get("type") == "Flipout" else "Reparameterization"
    dnn_to_bnn(m, dict(dict(_PRIOR, **(bnn_prior_parameters or {})), type=kind))
    return to_qresnet(m)


def qresnet18(num_classes=1000, bnn_prior_parameters=None):
    return _make("resnet18", num_classes, bnn_prior_parameters)


def qresnet34(num_classes=1000, bnn_prior_parameters=None):
    return _make("resnet34", num_classes, bnn_prior_parameters)


def qresnet50(num_classes=1000, bnn_prior_parameters=None):
    return _make("resnet50", num_classes, bnn_prior_parameters)


def qresnet101(num_classes=1000, bnn_prior_parameters=None):
    return _make("resnet101", num_classes, bnn_prior_parameters)
