"""CPU: the Bayesian multi-head attention layers — conversion, float64 parity of the eager composite with
nn.MultiheadAttention, KL accounting, MOPED, refusals, and the export table of include/btx_attn.h."""
import os
import re

import pytest
import torch
import torch.nn as nn

import bayesian_torch_amd as bt
from bayesian_torch_amd import _lib, layers as L
from bayesian_torch_amd.models import get_kl_loss

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
KINDS = ["Reparameterization", "Flipout"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("batch_first", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_conversion_of_an_encoder_layer(kind, batch_first):
    torch.manual_seed(0)
    enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(32, 4, 64, dropout=0.0, batch_first=batch_first), 2, enable_nested_tensor=False)
    bt.dnn_to_bnn(enc, dict(PRIOR, type=kind))
    for layer in enc.layers:
        assert type(layer.self_attn) is getattr(L, "MultiheadAttention" + kind) and layer.self_attn.batch_first == batch_first
        assert type(layer.linear1) is type(layer.linear2) is getattr(L, "Linear" + kind)
        assert type(layer.self_attn.in_proj) is type(layer.self_attn.out_proj) is getattr(L, "Linear" + kind)
    x = torch.randn(3, 5, 32)
    with torch.no_grad():
        y = enc.eval()(x)   # torch's fast path would read in_proj_weight: AttributeError
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    enc.train()(x).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in enc.parameters())
    # KL: in_proj and out_proj once each (the module's own kl_loss is their sum and is not counted again)
    terms = [m.kl_loss() for m in enc.modules() if hasattr(m, "kl_loss") and not getattr(m, "_btx_kl_composite", False)]
    assert len(terms) == 2 * 4 and torch.allclose(get_kl_loss(enc), sum(terms))
    attn = enc.layers[0].self_attn
    assert torch.equal(attn.kl_loss(), attn.in_proj.kl_loss() + attn.out_proj.kl_loss())


def _pair(kind, batch_first=True):
    """(nn.MultiheadAttention, its Bayesian twin with the same weights and sigma = 0), float64"""
    torch.manual_seed(1)
    ref = nn.MultiheadAttention(32, 4, batch_first=batch_first).double()
    m = getattr(L, "MultiheadAttention" + kind)(32, 4, batch_first=batch_first).double()
    with torch.no_grad():
        ref.in_proj_bias.normal_()
        ref.out_proj.bias.normal_()
        for lin, w, b in ((m.in_proj, ref.in_proj_weight, ref.in_proj_bias), (m.out_proj, ref.out_proj.weight, ref.out_proj.bias)):
            lin.mu_weight.copy_(w)
            lin.mu_bias.copy_(b)
            lin.rho_weight.fill_(-200.0)
            lin.rho_bias.fill_(-200.0)
    return ref, m


@pytest.mark.parametrize("mask", ["none", "pad", "causal", "pad_float"])
@pytest.mark.parametrize("kind", KINDS)
def test_float64_parity_with_torch(kind, mask):
    ref, m = _pair(kind)
    x = torch.randn(3, 7, 32, dtype=torch.float64)
    pad = torch.zeros(3, 7, dtype=torch.bool)
    pad[1, 4:], pad[2, :] = True, True   # row 2: every key masked
    kw = {}
    if mask == "pad":
        kw = dict(key_padding_mask=pad)
    elif mask == "pad_float":
        kw = dict(key_padding_mask=torch.zeros(3, 7, dtype=torch.float64).masked_fill(pad, float("-inf")))
    elif mask == "causal":
        kw = dict(attn_mask=nn.Transformer.generate_square_subsequent_mask(7).double(), is_causal=True)
    with torch.no_grad():
        want = ref(x, x, x, need_weights=False, **kw)[0]
        got, w, kl = m(x, x, x, **({"is_causal": True} if mask == "causal" else kw))
        _, ww = m(x, x, x, need_weights=True, return_kl=False, **kw)
    assert w is None and torch.equal(kl, m.kl_loss()) and ww.shape == (3, 7, 7)
    dead = pad.all(1) if mask.startswith("pad") else torch.zeros(3, dtype=torch.bool)
    assert float((got[~dead] - want[~dead]).abs().max()) <= 1e-12
    # where every key is masked the attention core gives zeros (torch: NaN), so the output is out_proj's bias
    assert torch.equal(got[dead], m.out_proj.mu_bias.detach().expand(int(dead.sum()), 7, 32))


def test_moped_copies_the_four_tensors():
    torch.manual_seed(2)
    from bayesian_torch_amd.utils.util import get_rho
    box = nn.ModuleDict(dict(a=nn.MultiheadAttention(32, 4)))
    src = box["a"]
    bt.dnn_to_bnn(box, dict(PRIOR, type="Reparameterization", moped_enable=True, moped_delta=0.2))
    a = box["a"]
    for lin, w, b in ((a.in_proj, src.in_proj_weight, src.in_proj_bias), (a.out_proj, src.out_proj.weight, src.out_proj.bias)):
        assert torch.equal(lin.mu_weight, w) and torch.equal(lin.mu_bias, b)
        assert torch.equal(lin.rho_weight, get_rho(w.data, 0.2)) and torch.equal(lin.rho_bias, get_rho(b.data, 0.2))


@pytest.mark.parametrize("kw,word", [(dict(kdim=16), "kdim"), (dict(dropout=0.1), "dropout")])
def test_conversion_refuses_by_name(kw, word):
    box = nn.ModuleDict(dict(attn=nn.MultiheadAttention(32, 4, **kw)))
    with pytest.raises(ValueError, match="'attn'.*%s" % word):
        bt.dnn_to_bnn(box, dict(PRIOR, type="Flipout"))
    with pytest.raises(AttributeError, match="LocalReparameterization"):
        bt.dnn_to_bnn(nn.ModuleDict(dict(attn=nn.MultiheadAttention(32, 4))), dict(PRIOR, type="LocalReparameterization"))


def test_cross_attention_is_refused_by_name():
    m = L.MultiheadAttentionReparameterization(32, 4, batch_first=True)
    x = torch.randn(2, 5, 32)
    with pytest.raises(_lib.BtxError, match="cross-attention"):
        m(x, x.clone(), x)


def test_exports_attn_is_the_header():
    text = open(os.path.join(ROOT, "include", "btx_attn.h")).read()
    declared = set(re.findall(r"\b(btx_[a-z0-9_]+)\s*\(", text.split("extern \"C\"", 1)[1]))
    assert declared == set(_lib.EXPORTS_ATTN)
    others = set(_lib.EXPORTS) | set(_lib.EXPORTS_DROP) | set(_lib.EXPORTS_GRU) | set(_lib.EXPORTS_GRU_TRAIN)
    assert not others & set(_lib.EXPORTS_ATTN)
    assert all(hasattr(_lib.lib(), n) for n in _lib.EXPORTS_ATTN)
