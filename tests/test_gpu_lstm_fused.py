"""The fused Bayesian LSTM sequence (fused_sequence, btx_lstm_fwd) on the GPU: against the eager per-step loop, against the
CPU reference chain fed with the noise BTX-RNG v1 defines, MC sample lanes, GraphedMC replays and the eager fallbacks."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make(cls, I, H, bias=True, seed=0):
    from bayesian_torch_amd import layers as L
    torch.manual_seed(seed)
    return getattr(L, cls)(I, H, bias=bias).to(_dev())


def run(layer, x, st, fused, s0=7):
    import bayesian_torch_amd as bt
    bt.set_sample_index(layer, s0)
    layer.fused_sequence = fused
    with torch.no_grad():
        hs, (hs2, cs), kl = layer(x, st)
    assert hs2 is hs
    return hs, cs, kl, (layer.ih._btx_sample, layer.hh._btx_sample)


CASES = [  # (I, H, B, T)
    (12, 10, 4, 6), (16, 8, 3, 5), (24, 48, 1, 1), (7, 10, 1, 9), (33, 48, 5, 12), (256, 512, 64, 3), (20, 48, 4, 300),
    (40, 70, 66, 4)]


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
@pytest.mark.parametrize("I,H,B,T", CASES)
def test_fused_matches_the_eager_gpu_loop(cls, I, H, B, T):
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.set_precision("f32")
    bt.manual_seed(1234)
    for bias in (True, False):
        for with_state in (False, True):
            layer = make(cls, I, H, bias)
            torch.manual_seed(1)
            x = torch.randn(B, T, I, device=dev)
            st = (torch.randn(B, H, device=dev), torch.randn(B, H, device=dev)) if with_state else None
            he, ce, ke, cnt_e = run(layer, x, st, False)
            kle = getattr(layer, "kl", None)
            hf, cf, kf, cnt_f = run(layer, x, st, True)
            assert hf.shape == (B, T, H) and cf.shape == (B, T, H) and hf.dtype == x.dtype
            eh, ec = rel(hf, he), rel(cf, ce)
            assert eh <= 1e-5 and ec <= 1e-5, (bias, with_state, eh, ec)
            assert abs(float(kf) - float(ke)) <= 1e-6 * abs(float(ke)), (float(kf), float(ke))
            if cls == "LSTMFlipout":
                assert layer.kl is kf and kle is not None
            assert cnt_f == cnt_e == (7 + T, 7 + T)
    # the counters a fused forward leaves behind are those of the eager loop: the next unfused forward is the same either way
    layer.fused_sequence = False
    with torch.no_grad():
        nxt_f = layer(x, st)[0]
    bt.set_sample_index(layer, 7 + T)
    with torch.no_grad():
        nxt_e = layer(x, st)[0]
    assert torch.equal(nxt_f, nxt_e)


def _reference_chain(layer, x, s0, bf16):
    """bt_ref Linear forwards + the torch cell on the CPU, fed per step with materialize_noise(s0 + t) of ih and hh"""
    from oracle import bt_ref
    c = lambda t: None if t is None else t.detach().float().cpu()  # noqa: E731
    rb = (lambda t: None if t is None else t.to(torch.bfloat16).float()) if bf16 else (lambda t: t)  # noqa: E731
    B, T, I = x.shape
    H = layer.out_features
    h = torch.zeros(B, H)
    cc = torch.zeros(B, H)
    hs, cs = [], []
    flip = layer._family == "flipout"
    for t in range(T):
        g = 0
        for lin, inp in ((layer.ih, c(x[:, t])), (layer.hh, h)):
            nz = lin.materialize_noise(s0 + t, tuple(inp.shape), (B, 4 * H), torch.float32)
            mu, rho = c(lin.mu_weight), c(lin.rho_weight)
            if flip:
                d = bt_ref.softplus(rho) * c(nz["eps_w"])
                out = inp.new_zeros(B, 4 * H) + bt_ref._contract(rb(inp), rb(mu), c(lin.mu_bias), dict(kind="linear"))
                bias = None if lin.mu_bias is None else bt_ref.softplus(c(lin.rho_bias)) * c(nz["eps_b"])
                out = out + bt_ref._contract(rb(inp) * c(nz["sign_in"]), rb(d), bias, dict(kind="linear")) * c(nz["sign_out"])
            else:
                w = mu + bt_ref.softplus(rho) * c(nz["eps_w"])
                bias = None if lin.mu_bias is None else c(lin.mu_bias) + bt_ref.softplus(c(lin.rho_bias)) * c(nz["eps_b"])
                out = bt_ref._contract(rb(inp), rb(w), bias, dict(kind="linear"))
            g = g + out
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        cc = f * cc + i * gg
        h = o * torch.tanh(cc)
        hs.append(h)
        cs.append(cc)
    return torch.stack(hs, 1), torch.stack(cs, 1)


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
@pytest.mark.parametrize("prec,tol", [("f32", 1e-5), ("bf16", 1e-2)])
def test_fused_matches_the_cpu_reference_chain(cls, prec, tol):
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.manual_seed(99)
    for I, H, B, T in ((12, 10, 4, 6), (64, 48, 5, 16)):
        layer = make(cls, I, H)
        layer.precision = None
        bt.set_precision(prec)
        try:
            torch.manual_seed(2)
            x = torch.randn(B, T, I, device=dev)
            hf, cf, _, _ = run(layer, x, None, True, s0=3)
        finally:
            bt.set_precision("f32")
        hr, cr = _reference_chain(layer, x, 3, prec == "bf16")
        eh, ec = rel(hf.cpu(), hr), rel(cf.cpu(), cr)
        print("%s %s %dx%d B=%d T=%d: rel-L2 h %.2e c %.2e" % (cls, prec, I, H, B, T, eh, ec))
        assert eh <= tol and ec <= tol


def test_bf16_activations():
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.set_precision("f32")
    layer = make("LSTMFlipout", 32, 24)
    torch.manual_seed(3)
    x = torch.randn(4, 8, 32, device=dev)
    hf, cf, _, _ = run(layer, x.bfloat16(), None, True)
    assert hf.dtype == torch.bfloat16 and cf.dtype == torch.bfloat16
    hr, cr, _, _ = run(layer, x.bfloat16().float(), None, True)
    assert rel(hf, hr) < 2e-2 and rel(cf, cr) < 2e-2


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_lanes_are_bit_identical_to_single_sample_fused_forwards(cls):
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.set_precision("f32")
    B, T, I, H = 3, 5, 20, 36
    layer = make(cls, I, H)
    layer.fused_sequence = True
    idx = [4, 11, 90]
    torch.manual_seed(4)
    xs = torch.randn(B, T, I, device=dev)
    xl = torch.randn(3 * B, T, I, device=dev)
    st = (torch.randn(B, H, device=dev), torch.randn(B, H, device=dev))
    with torch.no_grad():
        singles_s = []
        singles_l = []
        for l, s in enumerate(idx):
            bt.set_sample_index(layer, s)
            singles_s.append(layer(xs, st)[0])
            bt.set_sample_index(layer, s)
            singles_l.append(layer(xl[l * B:(l + 1) * B], st)[0])
        bt.set_sample_lanes(layer, idx, batch=B)
        shared = layer(xs, st)[0]
        bt.set_sample_lanes(layer, idx, batch=B)
        per_lane = layer(xl, st)[0]
        bt.set_sample_lanes(layer, None)
    assert shared.shape == (3 * B, T, H)
    for l in range(3):
        assert torch.equal(shared[l * B:(l + 1) * B], singles_s[l])
        assert torch.equal(per_lane[l * B:(l + 1) * B], singles_l[l])


class SeqNet(nn.Module):
    def __init__(self, i=24, h=40, classes=5):
        super().__init__()
        self.lstm = nn.LSTM(i, h)
        self.fc = nn.Linear(h, classes)

    def forward(self, x):
        out, _ = self.lstm(x)
        return self.fc(out[:, -1, :])


def _model(kind):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    torch.manual_seed(0)
    m = SeqNet()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type=kind,
                          moped_enable=False, moped_delta=0.5))
    m = m.to(_dev()).eval()
    assert fuse_model(m) == 1
    return m


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_mc_forward_lanes_on_a_fused_lstm_model(kind):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    dev = _dev()
    bt.set_precision("f32")
    m = _model(kind)
    torch.manual_seed(5)
    x = torch.randn(6, 7, 24, device=dev)
    a = mc.mc_forward(m, x, 8, lanes=1)
    b = mc.mc_forward(m, x, 8, lanes=4)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
@pytest.mark.parametrize("lanes", [1, 4])
def test_graphed_mc_replays_equal_fused_eager_forwards(kind, lanes):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    dev = _dev()
    bt.set_precision("f32")
    m = _model(kind)
    torch.manual_seed(6)
    x = torch.randn(4, 6, 24, device=dev)
    g = mc.GraphedMC(m, x.clone(), lanes=lanes, keep_logits=True, lane_mode="launch")
    try:
        samples = [[3], [17]] if lanes == 1 else [[3, 8, 9, 40], [17, 1, 2, 5]]
        for grp in samples:
            if lanes == 1:
                g.run(grp[0])
            else:
                g.run_many(grp)
            torch.cuda.synchronize()
            got = [g.lane_logits[k].clone() for k in range(lanes)]
            for k, s in enumerate(grp):
                bt.set_sample_index(m, s)
                with torch.no_grad():
                    ref = m(x)
                assert torch.equal(got[k], ref), (grp, k)
    finally:
        g.close()


def test_fallbacks_grad_hooks_and_pinned_unfused():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd._lib import BtxError
    dev = _dev()
    bt.set_precision("f32")
    B, T, I, H = 3, 4, 16, 12
    torch.manual_seed(7)
    x = torch.randn(B, T, I, device=dev)
    grads = []
    for fused in (False, True):
        layer = make("LSTMFlipout", I, H, seed=3)
        bt.assign_layer_ids(layer, start=500)  # the same noise for both layers
        layer.fused_sequence = fused
        bt.set_sample_index(layer, 2)
        hs, _, kl = layer(x)
        (hs.square().sum() + kl).backward()
        grads.append([p.grad.clone() for p in layer.parameters()])
    for ga, gb in zip(*grads):
        assert torch.equal(ga, gb)
    layer = make("LSTMReparameterization", I, H)
    layer.fused_sequence = True
    calls = []
    hk = layer.ih.register_forward_hook(lambda *a: calls.append(1))
    with torch.no_grad():
        layer(x)
    hk.remove()
    assert len(calls) == T
    layer.fused_sequence = False
    with torch.no_grad():
        bt.set_sample_lanes(layer, [1, 2], batch=B)
        with pytest.raises(BtxError):
            layer(x)
        bt.set_sample_lanes(layer, None)
