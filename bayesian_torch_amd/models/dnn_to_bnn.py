"""dnn_to_bnn() / get_kl_loss() — host-side API surface of the hot path (reference models/dnn_to_bnn.py:52-165).

Behaviour kept from the reference: recursion into any child that has children; a leaf is converted when its CLASS
NAME contains "Conv" or "Linear" (so ConvTranspose* and look-alike user classes match too) and the new class is
looked up as `<ClassName><params["type"]>` in `bayesian_torch_amd.layers`; the required dict keys are
prior_mu, prior_sigma, posterior_mu_init, posterior_rho_init, type, moped_enable (KeyError if absent), moped_delta;
`output_padding` / `padding_mode` are NOT forwarded; converted layers get `dnn_to_bnn_flag = True` (forward returns
only `out`).  nn.LSTM children become LSTM<type> (two Bayesian Linear layers per time step).  Beyond the reference: a one-layer,
unidirectional, batch-first nn.GRU becomes GRU<type>; any other nn.GRU is refused by name.  An nn.MultiheadAttention
(self-attention: one packed in-projection, no attention dropout, no bias_k / add_zero_attn) becomes MultiheadAttention<type>
 as a whole, MOPED included; any other one is refused by name.
Beyond the reference: the optional keys "prior" (a bayesian_torch_amd.priors prior) and "kl_samples" install a non-Gaussian weight
prior on every converted layer (layer.set_prior); without them nothing changes.
"""
import torch

from .. import layers as bayesian_layers
from ..utils.util import get_rho


def _moped(bnn_layer, d, params, wname):
    delta = params["moped_delta"]
    getattr(bnn_layer, "mu_" + wname).data.copy_(d.weight.data)
    getattr(bnn_layer, "rho_" + wname).data.copy_(get_rho(d.weight.data, delta))
    if bnn_layer.mu_bias is not None:
        bnn_layer.mu_bias.data.copy_(d.bias.data)
        bnn_layer.rho_bias.data.copy_(get_rho(d.bias.data, delta))


def _layer_class(params, d):
    """`<ClassName><type>` in bayesian_torch_amd.layers; a type that does not cover the module's class (LocalReparameterization has
    no ConvTranspose* / LSTM form) fails with the module's class in the message"""
    name = d.__class__.__name__ + params["type"]
    fn = getattr(bayesian_layers, name, None)
    if fn is None:
        raise AttributeError("dnn_to_bnn: no Bayesian layer class %r: type=%r does not cover %s modules"
                             % (name, params["type"], d.__class__.__name__))
    return fn


def bnn_linear_layer(params, d):
    layer_fn = _layer_class(params, d)
    bnn_layer = layer_fn(in_features=d.in_features, out_features=d.out_features,
                         prior_mean=params["prior_mu"], prior_variance=params["prior_sigma"],
                         posterior_mu_init=params["posterior_mu_init"],
                         posterior_rho_init=params["posterior_rho_init"], bias=d.bias is not None)
    if params["moped_enable"]:
        _moped(bnn_layer, d, params, "weight")
    bnn_layer.dnn_to_bnn_flag = True
    return bnn_layer


def bnn_conv_layer(params, d):
    layer_fn = _layer_class(params, d)
    bnn_layer = layer_fn(in_channels=d.in_channels, out_channels=d.out_channels, kernel_size=d.kernel_size,
                         stride=d.stride, padding=d.padding, dilation=d.dilation, groups=d.groups,
                         prior_mean=params["prior_mu"], prior_variance=params["prior_sigma"],
                         posterior_mu_init=params["posterior_mu_init"],
                         posterior_rho_init=params["posterior_rho_init"], bias=d.bias is not None)
    if params["moped_enable"]:
        _moped(bnn_layer, d, params, "kernel")
    bnn_layer.dnn_to_bnn_flag = True
    return bnn_layer


def bnn_lstm_layer(params, d):
    """reference models/dnn_to_bnn.py:106-122: nn.LSTM(input_size, hidden_size) -> LSTM<type>(in, out); MOPED is not
    defined for LSTM layers (the reference prints the same warning and converts with the default init)."""
    layer_fn = _layer_class(params, d)
    bnn_layer = layer_fn(in_features=d.input_size, out_features=d.hidden_size, prior_mean=params["prior_mu"],
                         prior_variance=params["prior_sigma"], posterior_mu_init=params["posterior_mu_init"],
                         posterior_rho_init=params["posterior_rho_init"], bias=d.bias is not None)
    if params["moped_enable"]:
        print("WARNING: MOPED method is not supported for LSTM layers!!!")
    bnn_layer.dnn_to_bnn_flag = True
    return bnn_layer


def bnn_gru_layer(params, d, name="GRU"):
    """nn.GRU(input_size, hidden_size, batch_first=True) -> GRU<type>(in, out).  The Bayesian GRU is one unidirectional layer over
    [batch, seq, features]: every other configuration is refused with the module and the option in the message.  MOPED: as for
    LSTM layers, the warning and the default init."""
    for opt, want in (("num_layers", 1), ("bidirectional", False), ("batch_first", True), ("dropout", 0), ("proj_size", 0)):
        got = getattr(d, opt, want)
        if got != want:
            raise ValueError("dnn_to_bnn: cannot convert the GRU %r: %s=%r is not supported (the Bayesian GRU needs %s=%r)"
                             % (name, opt, got, opt, want))
    layer_fn = _layer_class(params, d)
    bnn_layer = layer_fn(in_features=d.input_size, out_features=d.hidden_size, prior_mean=params["prior_mu"],
                         prior_variance=params["prior_sigma"], posterior_mu_init=params["posterior_mu_init"],
                         posterior_rho_init=params["posterior_rho_init"], bias=d.bias)
    if params["moped_enable"]:
        print("WARNING: MOPED method is not supported for LSTM layers!!!")
    bnn_layer.dnn_to_bnn_flag = True
    return bnn_layer


def bnn_mha_layer(params, d, name="MultiheadAttention"):
    """nn.MultiheadAttention(E, heads) -> MultiheadAttention<type>(E, heads): the packed in-projection becomes the Bayesian Linear
    `in_proj` (E -> 3E, rows q | k | v), out_proj the Bayesian Linear `out_proj`.  The Bayesian layer is self-attention without
    attention dropout: every other configuration is refused with the module and the option in the message.  MOPED is well defined
    (both projections are Linear layers): in_proj_weight / in_proj_bias and out_proj.weight / out_proj.bias become mu, get_rho of
    them rho."""
    for opt, got, want in (("kdim", d.kdim, d.embed_dim), ("vdim", d.vdim, d.embed_dim), ("dropout", d.dropout, 0),
                           ("add_bias_kv", d.bias_k is not None, False), ("add_zero_attn", d.add_zero_attn, False)):
        if got != want:
            raise ValueError("dnn_to_bnn: cannot convert the MultiheadAttention %r: %s=%r is not supported (the Bayesian attention "
                             "needs %s=%r)" % (name, opt, got, opt, want))
    layer_fn = _layer_class(params, d)
    bnn_layer = layer_fn(embed_dim=d.embed_dim, num_heads=d.num_heads, bias=d.in_proj_bias is not None, batch_first=d.batch_first,
                         prior_mean=params["prior_mu"], prior_variance=params["prior_sigma"],
                         posterior_mu_init=params["posterior_mu_init"], posterior_rho_init=params["posterior_rho_init"])
    if params["moped_enable"]:
        delta = params["moped_delta"]
        for lin, w, b in ((bnn_layer.in_proj, d.in_proj_weight, d.in_proj_bias), (bnn_layer.out_proj, d.out_proj.weight, d.out_proj.bias)):
            lin.mu_weight.data.copy_(w.data)
            lin.rho_weight.data.copy_(get_rho(w.data, delta))
            if lin.mu_bias is not None:
                lin.mu_bias.data.copy_(b.data)
                lin.rho_bias.data.copy_(get_rho(b.data, delta))
    bnn_layer.dnn_to_bnn_flag = True
    return bnn_layer


def _with_prior(bnn_layer, params):
    if "prior" in params:
        bnn_layer.set_prior(params["prior"], params.get("kl_samples", 1))
    return bnn_layer


def dnn_to_bnn(m, bnn_prior_parameters):
    for name, child in list(m._modules.items()):
        if child is None:
            continue
        cname = child.__class__.__name__
        if "MultiheadAttention" in cname:  # before the recursion: its out_proj is a child, its in-projection a bare parameter
            setattr(m, name, _with_prior(bnn_mha_layer(bnn_prior_parameters, child, name), bnn_prior_parameters)
                    .to(child.out_proj.weight.device))
        elif child._modules:
            dnn_to_bnn(child, bnn_prior_parameters)
        elif "Conv" in cname:
            setattr(m, name, _with_prior(bnn_conv_layer(bnn_prior_parameters, child), bnn_prior_parameters).to(child.weight.device))
        elif "Linear" in cname:
            setattr(m, name, _with_prior(bnn_linear_layer(bnn_prior_parameters, child), bnn_prior_parameters).to(child.weight.device))
        elif "LSTM" in cname:
            setattr(m, name, _with_prior(bnn_lstm_layer(bnn_prior_parameters, child), bnn_prior_parameters)
                    .to(next(child.parameters()).device))
        elif "GRU" in cname:
            setattr(m, name, _with_prior(bnn_gru_layer(bnn_prior_parameters, child, name), bnn_prior_parameters)
                    .to(next(child.parameters()).device))
    return


def set_prior(model, prior, kl_samples=1):
    """layer.set_prior(prior, kl_samples) on every variational layer of `model` (priors.py; None / GaussianPrior: back to the closed-form
    Gaussian KL).  A model that holds a Bayesian LSTM / GRU or a quantized layer is refused for a non-Gaussian prior, before any layer is
    changed.  Returns the model."""
    from ..layers.base_variational_layer import _VariationalGRU, _VariationalLSTM, _VariationalNd
    from ..priors import check_prior
    mods = [mod for mod in model.modules() if hasattr(mod, "set_prior")]
    if check_prior(prior) is not None:
        for mod in mods:  # the refusing classes first: nothing is half-set
            if not isinstance(mod, _VariationalNd):
                mod.set_prior(prior, kl_samples)
    inner = {id(lin) for mod in mods if isinstance(mod, (_VariationalLSTM, _VariationalGRU)) for lin in (mod.ih, mod.hh)}
    for mod in mods:
        if isinstance(mod, _VariationalNd) and id(mod) not in inner:
            mod.set_prior(prior, kl_samples)
    return model


def get_kl_loss(m):
    """Sum of `layer.kl_loss()` over every module that has one (None for a model without Bayesian layers).  CUDA
    models: ONE launch for all tensors of all layers (btx_kl_gauss_model), differentiable (btx_kl_gauss_model_bwd)."""
    # (a Bayesian GRU's kl_loss() is the sum over its children ih / hh, which are in the walk themselves: each counts once)
    layers = [layer for layer in m.modules() if hasattr(layer, "kl_loss") and not getattr(layer, "_btx_kl_composite", False)]
    if not layers:
        return None
    # MCDropout layers (no parameters, kl_loss() == 0) do not take a mixed model off the one-launch path: the sum runs over the
    # layers that have a KL; a model whose only layers with a kl_loss are MCDropout sums its zeros below
    var = [layer for layer in layers if not getattr(layer, "_btx_dropout", False)]
    if var and all(hasattr(layer, "_w") and layer._use_hip(layer._w()[0]) for layer in var):
        from .. import autograd as _ag
        return _ag.kl_of_layers(var)
    terms = [layer.kl_loss() for layer in layers]
    if len(terms) == 1:
        return terms[0]
    kl = terms[0]  # the reference's sequential += chain, bit for bit on CPU
    for t in terms[1:]:
        kl = kl + t
    return kl
