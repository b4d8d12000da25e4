"""The Bayesian GRU layers without a GPU: the eager cell against torch.nn.GRU in float64, and the dnn_to_bnn surface."""
import pytest
import torch
import torch.nn as nn

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
KINDS = ["Reparameterization", "Flipout"]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_eager_cell_equals_nn_gru_in_float64(kind, bias):
    """rho = -200 makes sigma 0 (softplus(-200) ~ 1e-87): with nn.GRU's weights copied in unchanged the layer IS nn.GRU — a wrong
    gate order, or r applied to the input half or outside b_hn, moves the output by O(0.1)"""
    from bayesian_torch_amd import layers as L
    torch.manual_seed(3)
    I, H, B, T = 5, 7, 3, 4
    ref = nn.GRU(I, H, batch_first=True, bias=bias).double()
    layer = getattr(L, "GRU" + kind)(I, H, bias=bias).double()
    with torch.no_grad():
        for lin, sfx in ((layer.ih, "ih"), (layer.hh, "hh")):
            lin.mu_weight.copy_(getattr(ref, "weight_%s_l0" % sfx))
            lin.rho_weight.fill_(-200.0)
            if bias:
                lin.mu_bias.copy_(getattr(ref, "bias_%s_l0" % sfx))
                lin.rho_bias.fill_(-200.0)
        x, h0 = torch.randn(B, T, I, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)
        for state in (None, h0):
            want, want_h = ref(x) if state is None else ref(x, state.unsqueeze(0))
            seq, h_T, kl = layer(x, state)
            assert seq.shape == (B, T, H) and h_T.shape == (B, H) and kl.dim() == 0
            assert float((seq - want).abs().max()) <= 1e-12 and float((h_T - want_h[0]).abs().max()) <= 1e-12
    assert set(k.split(".")[0] for k in layer.state_dict()) == {"ih", "hh"} and layer.hh.mu_weight.shape == (3 * H, H)


class _Net(nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.gru = nn.GRU(6, 8, **kw)
        self.fc = nn.Linear(8, 3)

    def forward(self, x):
        return self.fc(self.gru(x)[0][:, -1])


@pytest.mark.parametrize("kind", KINDS)
def test_dnn_to_bnn_converts_a_batch_first_gru_and_refuses_the_rest(kind, capsys):  # (get_kl_loss: every inner layer counts once)
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L, priors
    params = dict(PRIOR, type=kind)
    m = _Net(batch_first=True)
    bt.dnn_to_bnn(m, params)
    assert type(m.gru) is getattr(L, "GRU" + kind) and m.gru.dnn_to_bnn_flag and type(m.gru.ih) is getattr(L, "Linear" + kind)
    with torch.no_grad():
        assert m(torch.randn(2, 5, 6)).shape == (2, 3)
        kl, inner = float(bt.get_kl_loss(m)), float(m.gru.ih.kl_loss()) + float(m.gru.hh.kl_loss())
        assert kl == pytest.approx(inner + float(m.fc.kl_loss()), rel=1e-6) and float(m.gru.kl_loss()) == pytest.approx(inner, rel=1e-6)
    m2, sd = _Net(batch_first=True), m.state_dict()
    bt.dnn_to_bnn(m2, params)
    assert {k for k in sd if k.startswith("gru.")} == {"gru.%s.%s_%s" % (a, b, c) for a in ("ih", "hh") for b in ("mu", "rho")
                                                       for c in ("weight", "bias")}
    m2.load_state_dict(sd)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    for kw, opt in ((dict(num_layers=2, batch_first=True), "num_layers"), (dict(bidirectional=True, batch_first=True), "bidirectional"),
                    (dict(), "batch_first")):
        with pytest.raises(ValueError, match="'gru'.*%s" % opt):
            bt.dnn_to_bnn(_Net(**kw), params)
    capsys.readouterr()
    bt.dnn_to_bnn(_Net(batch_first=True), dict(params, moped_enable=True))
    assert "MOPED method is not supported" in capsys.readouterr().out
    with pytest.raises(bt._lib.BtxError, match="GRU"):   # non-Gaussian priors: refused as on the LSTM classes
        m.gru.set_prior(priors.LaplacePrior(1.0))
    with pytest.raises(bt._lib.BtxError, match="GRU"):
        m.gru.ih.set_prior(priors.LogUniformPrior("sum"))
