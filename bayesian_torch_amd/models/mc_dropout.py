"""enable_mc_dropout: turn the nn.Dropout layers of a model into MCDropout layers (BTX-DROP v1), in place."""
import torch.nn as nn

from .._lib import BtxError
from ..layers import dropout_layers as _drop

_TWINS = ((nn.Dropout1d, _drop.MCDropout1d), (nn.Dropout2d, _drop.MCDropout2d), (nn.Dropout3d, _drop.MCDropout3d))
_REFUSED = (nn.AlphaDropout, nn.FeatureAlphaDropout)


def enable_mc_dropout(model, always_on=True):
    """Replace every nn.Dropout / nn.Dropout1d / 2d / 3d of `model` by the matching MCDropout* (same p, same training flag), in
    place, and return how many were replaced.  The masks then follow (seed, MC sample index, layer id): set_sample_index,
    mc_forward(lanes=k), mc.GraphedMC, mc.evaluate and autograd.GraphedTrainStep treat the model like any other stochastic one.
    always_on=True keeps the layers active in eval() mode — the Monte-Carlo dropout of Gal & Ghahramani (2016); False keeps
    nn.Dropout's training-only behaviour with reproducible masks.  nn.AlphaDropout / nn.FeatureAlphaDropout have no twin: a model
    that holds one is refused (BtxError naming the module) before anything is replaced.  dnn_to_bnn does NOT call this: a converted
    model keeps its nn.Dropout layers until the caller asks for `enable_mc_dropout(model)`."""
    for name, m in model.named_modules():
        if isinstance(m, _REFUSED):
            raise BtxError("enable_mc_dropout: %r is a %s, which has no Monte-Carlo twin (BTX-DROP v1 defines Bernoulli dropout only)"
                           % (name, type(m).__name__))
    return _replace(model, bool(always_on))


def _twin(m, always_on):
    if type(m) is nn.Dropout:
        return _drop.MCDropout(m.p, "element", always_on, m.inplace)
    for src, dst in _TWINS:
        if type(m) is src:
            return dst(m.p, always_on, m.inplace)
    return None


def _replace(module, always_on):
    n = 0
    for name, child in list(module._modules.items()):
        if child is None:
            continue
        new = _twin(child, always_on)
        if new is None:
            n += _replace(child, always_on)
            continue
        new.train(child.training)
        module._modules[name] = new
        n += 1
    return n
