"""Fused Bayesian LSTM training (fused_training: btx_lstm_fwd_train + btx_lstm_bwd) on the GPU: gradients against a float64
autograd chain on the CPU fed with the noise BTX-RNG v1 defines, against the eager per-step loop, determinism, captured training
steps (autograd.GraphedTrainStep) and the eager fallbacks."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make(cls, I, H, bias=True, seed=0):
    from bayesian_torch_amd import layers as L
    torch.manual_seed(seed)
    return getattr(L, cls)(I, H, bias=bias).to(_dev())


def _reference_grads(layer, x, h0, c0, s0, bf16, r_h, r_c):
    """float64 torch autograd on the CPU: per step the Linear forwards of ih / hh with materialize_noise(s0 + t) and the torch
    cell; loss = sum(hidden_seq * r_h) + sum(c_seq * r_c).  Returns the gradients of x, h0, c0 and the layers' parameters."""
    c = lambda t: None if t is None else t.detach().double().cpu()  # noqa: E731
    leaf = lambda t: None if t is None else c(t).requires_grad_()  # noqa: E731
    # bf16 precision: the operands the forward rounds, rounded (values only; the gradient passes straight through)
    rb = (lambda t: t + (t.float().to(torch.bfloat16).double() - t).detach()) if bf16 else (lambda t: t)  # noqa: E731
    B, T, I = x.shape
    H = layer.out_features
    flip = layer._family == "flipout"
    xr, hr, cr = leaf(x), leaf(h0), leaf(c0)
    params = {}
    for name, lin in (("ih", layer.ih), ("hh", layer.hh)):
        params[name] = [leaf(lin.mu_weight), leaf(lin.rho_weight), leaf(lin.mu_bias), leaf(lin.rho_bias)]
    h = hr if hr is not None else torch.zeros(B, H, dtype=torch.float64)
    cc = cr if cr is not None else torch.zeros(B, H, dtype=torch.float64)
    hs, cs = [], []
    for t in range(T):
        g = 0
        for name, lin, inp in (("ih", layer.ih, xr[:, t]), ("hh", layer.hh, h)):
            mu, rho, mu_b, rho_b = params[name]
            nz = lin.materialize_noise(s0 + t, (B, inp.shape[1]), (B, 4 * H), torch.float32)
            d = F.softplus(rho) * c(nz["eps_w"])
            db = None if mu_b is None else F.softplus(rho_b) * c(nz["eps_b"])
            if flip:
                out = rb(inp) @ rb(mu).t()
                if mu_b is not None:
                    out = out + mu_b
                pert = (rb(inp) * c(nz["sign_in"])) @ rb(d).t()
                if db is not None:
                    pert = pert + db
                out = out + pert * c(nz["sign_out"])
            else:
                out = rb(inp) @ rb(mu + d).t()
                if mu_b is not None:
                    out = out + mu_b + db
            g = g + out
        i, f = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H])
        gg, o = torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        cc = f * cc + i * gg
        h = o * torch.tanh(cc)
        hs.append(h)
        cs.append(cc)
    loss = (torch.stack(hs, 1) * c(r_h)).sum() + (torch.stack(cs, 1) * c(r_c)).sum()
    loss.backward()
    out = {"x": xr.grad, "h0": hr.grad if hr is not None else None, "c0": cr.grad if cr is not None else None}
    for name in ("ih", "hh"):
        for k, p in zip(("mu_weight", "rho_weight", "mu_bias", "rho_bias"), params[name]):
            if p is not None:
                out[name + "." + k] = p.grad
    return out


def _fused_grads(layer, x, h0, c0, s0, r_h, r_c):
    import bayesian_torch_amd as bt
    layer.fused_training = True
    bt.set_sample_index(layer, s0)
    for p in layer.parameters():
        p.grad = None
    x = x.clone().requires_grad_()
    st = None
    if h0 is not None:
        h0, c0 = h0.clone().requires_grad_(), c0.clone().requires_grad_()
        st = (h0, c0)
    hs, (_, cs), kl = layer(x, st)
    ((hs * r_h).sum() + (cs * r_c).sum()).backward()
    out = {"x": x.grad, "h0": h0.grad if h0 is not None else None, "c0": c0.grad if c0 is not None else None}
    for name, lin in (("ih", layer.ih), ("hh", layer.hh)):
        for k in ("mu_weight", "rho_weight", "mu_bias", "rho_bias"):
            p = getattr(lin, k)
            if p is not None:
                out[name + "." + k] = p.grad
    return out


CASES = [  # (I, H, B, T)
    (12, 10, 4, 6), (7, 10, 1, 9), (33, 48, 5, 12), (40, 70, 66, 4), (16, 8, 3, 1)]


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
@pytest.mark.parametrize("prec,tol", [("f32", 1e-5), ("bf16", 2e-2)])
def test_gradients_match_the_float64_reference(cls, prec, tol):
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.manual_seed(321)
    try:
        bt.set_precision(prec)
        for n, (I, H, B, T) in enumerate(CASES):
            for bias, state in ((True, True), (False, n % 2 == 0)):
                layer = make(cls, I, H, bias=bias, seed=n)
                torch.manual_seed(10 + n)
                x = torch.randn(B, T, I, device=dev)
                h0 = torch.randn(B, H, device=dev) if state else None
                c0 = torch.randn(B, H, device=dev) if state else None
                r_h, r_c = torch.randn(B, T, H, device=dev), torch.randn(B, T, H, device=dev)
                got = _fused_grads(layer, x, h0, c0, 5, r_h, r_c)
                ref = _reference_grads(layer, x, h0, c0, 5, prec == "bf16", r_h, r_c)
                assert set(k for k, v in got.items() if v is not None) == set(k for k, v in ref.items() if v is not None)
                for k, r in ref.items():
                    if r is None:
                        continue
                    e = rel(got[k], r)
                    assert e <= tol, (cls, prec, (I, H, B, T), bias, state, k, e)
    finally:
        bt.set_precision("f32")


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
@pytest.mark.parametrize("I,H,B,T", [(12, 10, 4, 6), (40, 70, 66, 4), (33, 48, 5, 1)])
def test_against_the_eager_loop_and_the_inference_forward(cls, I, H, B, T):
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.set_precision("f32")
    bt.manual_seed(77)
    torch.manual_seed(1)
    x0 = torch.randn(B, T, I, device=dev)
    st0 = (torch.randn(B, H, device=dev), torch.randn(B, H, device=dev))
    r_h, r_c = torch.randn(B, T, H, device=dev), torch.randn(B, T, H, device=dev)
    res = {}
    for mode in ("eager", "fused", "fused2"):
        layer = make(cls, I, H, seed=4)
        bt.assign_layer_ids(layer, start=700)  # the same noise for every layer
        layer.fused_training = mode != "eager"
        layer.fused_sequence = mode != "eager"
        bt.set_sample_index(layer, 9)
        x = x0.clone().requires_grad_()
        h0, c0 = st0[0].clone().requires_grad_(), st0[1].clone().requires_grad_()
        hs, (_, cs), kl = layer(x, (h0, c0))
        counters = (layer.ih._btx_sample, layer.hh._btx_sample)
        ((hs * r_h).sum() + (cs * r_c).sum() + kl).backward()
        res[mode] = dict(hs=hs.detach(), cs=cs.detach(), kl=kl.detach(), counters=counters,
                         grads=[x.grad, h0.grad, c0.grad] + [p.grad for p in layer.parameters()])
        if mode == "fused":
            bt.set_sample_index(layer, 9)
            with torch.no_grad():
                hi, (_, ci), ki = layer(x0, st0)
            assert torch.equal(hi, hs) and torch.equal(ci, cs) and torch.equal(ki, kl)
            if cls == "LSTMFlipout":
                assert layer.kl is ki
    e, f, f2 = res["eager"], res["fused"], res["fused2"]
    assert f["counters"] == e["counters"] == (9 + T, 9 + T)
    assert rel(f["hs"], e["hs"]) <= 1e-5 and rel(f["cs"], e["cs"]) <= 1e-5
    for k, (gf, ge) in enumerate(zip(f["grads"], e["grads"])):
        assert gf is not None and ge is not None
        assert rel(gf, ge) <= 1e-5, (k, rel(gf, ge))
    for gf, gf2 in zip(f["grads"], f2["grads"]):  # deterministic: no atomics, fixed summation orders
        assert torch.equal(gf, gf2)


class SeqNet(nn.Module):
    # the head has no bias: this file pins the LSTM's captured gradients, and the Linear bias gradients of a GraphedTrainStep
    # replay after the first are a separate matter (they are not bit-identical to an eager step, with or without an LSTM)
    def __init__(self, i=24, h=40, classes=5):
        super().__init__()
        self.lstm = nn.LSTM(i, h)
        self.fc = nn.Linear(h, classes, bias=False)

    def forward(self, x):
        out, _ = self.lstm(x)
        return self.fc(out[:, -1, :])


def _model(kind, training):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    torch.manual_seed(0)
    m = SeqNet()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type=kind,
                          moped_enable=False, moped_delta=0.5))
    m = m.to(_dev())
    assert fuse_model(m, lstm_training=training) == 1
    return m


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_graphed_train_step_equals_eager_fused_steps(kind):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    dev = _dev()
    bt.set_precision("f32")
    m = _model(kind, True)
    torch.manual_seed(6)
    x = torch.randn(4, 6, 24, device=dev)
    y = torch.randint(0, 5, (4,), device=dev)
    step = GraphedTrainStep(m, x, y)
    graphed = {}
    try:
        for s in (3, 17):
            step.run(s)
            torch.cuda.synchronize()
            graphed[s] = [p.grad.clone() for p in m.parameters()]
    finally:
        step.close()
    assert any(not torch.equal(a, b) for a, b in zip(graphed[3], graphed[17]))
    for s in (3, 17):
        for p in m.parameters():
            p.grad = None
        bt.set_sample_index(m, s)
        out = m(x)
        loss = F.cross_entropy(out.float(), y) + get_kl_loss(m) / x.shape[0]
        loss.backward()
        for k, (g, p) in enumerate(zip(graphed[s], m.parameters())):
            assert torch.equal(g, p.grad), (s, k)


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_graphed_train_step_without_the_opt_in_still_raises(kind):
    from bayesian_torch_amd._lib import BtxError
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = _dev()
    m = _model(kind, False)
    x = torch.randn(4, 6, 24, device=dev)
    y = torch.randint(0, 5, (4,), device=dev)
    with pytest.raises(BtxError):
        GraphedTrainStep(m, x, y)


def test_fallbacks_take_the_eager_loop(monkeypatch):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import autograd as ag
    from bayesian_torch_amd._lib import BtxError
    dev = _dev()
    bt.set_precision("f32")
    B, T, I, H = 3, 4, 16, 12
    torch.manual_seed(7)
    x = torch.randn(B, T, I, device=dev)
    calls = []
    real = ag.LstmTrainFn.apply
    monkeypatch.setattr(ag.LstmTrainFn, "apply", lambda *a: calls.append(1) or real(*a))

    def train(layer):
        hs, _, kl = layer(x)
        (hs.sum() + kl).backward()

    layer = make("LSTMFlipout", I, H)
    layer.fused_training = True
    train(layer)
    assert len(calls) == 1  # the fused path
    hooked = []
    hk = layer.hh.register_forward_hook(lambda *a: hooked.append(1))
    train(layer)
    hk.remove()
    assert len(calls) == 1 and len(hooked) == T
    layer.precision = "bf16x3"
    layer.ih.precision = layer.hh.precision = "bf16x3"
    train(layer)
    assert len(calls) == 1
    layer = make("LSTMReparameterization", I, H)
    layer.fused_sequence = True  # inference only
    train(layer)
    assert len(calls) == 1
    layer.fused_training = True
    bt.set_sample_lanes(layer, [1, 2], batch=B)
    with pytest.raises(BtxError):
        layer(x)
    bt.set_sample_lanes(layer, None)
    train(layer)
    assert len(calls) == 2
