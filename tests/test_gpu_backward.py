"""GPU: the training path on the HIP backend (reference README.md:114-125).  Gradients of the HIP
forward (bayesian_torch_amd/autograd.py) against torch autograd through the reference op chain (oracle/bt_ref.py) fed
with the same BTX-RNG noise; f32 parity mode, rel-L2 <= 1e-4."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

CASES = [
    ("LinearReparameterization", dict(in_features=96, out_features=80), (16, 96)),
    ("LinearFlipout", dict(in_features=128, out_features=64), (8, 128)),
    ("LinearFlipout", dict(in_features=50, out_features=10, bias=False), (7, 50)),                        # channel-padded
    ("Conv2dReparameterization", dict(in_channels=32, out_channels=64, kernel_size=3, stride=1, padding=1), (2, 32, 10, 10)),
    ("Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=3, stride=1, padding=1, bias=False), (2, 64, 12, 12)),
    ("Conv2dFlipout", dict(in_channels=32, out_channels=48, kernel_size=3, stride=2, padding=1), (2, 32, 11, 11)),
    ("Conv2dFlipout", dict(in_channels=32, out_channels=32, kernel_size=3, padding=2, dilation=2, groups=2), (2, 32, 9, 11)),
    ("Conv2dFlipout", dict(in_channels=64, out_channels=128, kernel_size=1, stride=2, bias=False), (2, 64, 10, 10)),
    ("Conv2dFlipout", dict(in_channels=24, out_channels=40, kernel_size=3, padding=1), (1, 24, 9, 9)),        # channel-padded
    ("Conv1dFlipout", dict(in_channels=16, out_channels=32, kernel_size=5, stride=2, padding=2), (3, 16, 41)),
    ("Conv3dReparameterization", dict(in_channels=8, out_channels=8, kernel_size=3, prior_mean=0, prior_variance=1,
                                      posterior_mu_init=0, posterior_rho_init=-3.0, padding=1), (1, 8, 5, 6, 7)),
    ("ConvTranspose2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=4, stride=2, padding=1), (2, 16, 6, 7)),
    # stride-2 data gradients on enough pixels for the parity-major order of the transposed launch (ContractParams.par_major): tiles
    # that straddle two parity classes, a ragged last tile (3 * 26 * 26 = 2028 pixels), 1x1 and 5x5 filters, a forward ConvTranspose
    ("Conv2dFlipout", dict(in_channels=16, out_channels=32, kernel_size=3, stride=2, padding=1, bias=False), (3, 16, 26, 26)),
    ("Conv2dFlipout", dict(in_channels=16, out_channels=32, kernel_size=1, stride=2, bias=False), (3, 16, 26, 26)),
    ("Conv2dReparameterization", dict(in_channels=16, out_channels=16, kernel_size=5, stride=2, padding=2, bias=False), (2, 16, 36, 28)),
    ("ConvTranspose2dFlipout", dict(in_channels=32, out_channels=16, kernel_size=3, stride=2, padding=1, output_padding=1), (2, 32, 18, 16)),
    # small-C stems: forward and weight gradient on the row-fused geometry
    ("Conv2dFlipout", dict(in_channels=3, out_channels=32, kernel_size=7, stride=2, padding=3, bias=False), (2, 3, 30, 26)),
    ("Conv2dReparameterization", dict(in_channels=3, out_channels=16, kernel_size=3, stride=1, padding=1), (2, 3, 11, 9)),
    ("Conv2dFlipout", dict(in_channels=1, out_channels=80, kernel_size=5, stride=1, padding=2), (3, 1, 12, 12)),
]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _op_of(layer):
    op = layer._op
    if op.nd == 0:
        return dict(kind="linear")
    nd = op.nd
    d = dict(kind="convT" if op.transposed else "conv", nd=nd, stride=op.stride[3 - nd:], padding=op.padding[3 - nd:],
             dilation=op.dilation[3 - nd:], groups=op.groups)
    if op.transposed:
        d["output_padding"] = op.output_padding[3 - nd:]
    return d


@pytest.mark.parametrize("cls,kw,xshape", CASES)
def test_layer_gradients_match_autograd_through_the_reference_chain(cls, kw, xshape):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd import functional as BF
    from oracle import bt_ref
    dev = _dev()
    bt.manual_seed(123)
    bt.set_precision("f32")
    torch.manual_seed(0)
    layer = getattr(L, cls)(**kw).to(dev)
    x = torch.randn(*xshape, device=dev, requires_grad=True)
    s = 5
    bt.set_sample_index(layer, s)
    out, kl = layer(x)                                     # HIP forward under autograd
    assert out.requires_grad and kl.requires_grad
    gy = torch.randn_like(out)
    ((out * gy).sum() + 3.0 * kl).backward()
    mu, rho = layer._w()
    got = dict(x=x.grad.clone(), mu=mu.grad.clone(), rho=rho.grad.clone())
    if layer.mu_bias is not None:
        got.update(mu_b=layer.mu_bias.grad.clone(), rho_b=layer.rho_bias.grad.clone())

    # reference: torch autograd through the reference op chain with the noise BTX-RNG defines for (layer, sample s)
    with torch.no_grad():
        nz = layer.materialize_noise(s, tuple(x.shape), tuple(out.shape), x.dtype)
    xr = x.detach().clone().requires_grad_(True)
    mur = BF.plain_layout(mu.detach()).requires_grad_(True)
    rhor = BF.plain_layout(rho.detach()).requires_grad_(True)
    mbr = layer.mu_bias.detach().clone().requires_grad_(True) if layer.mu_bias is not None else None
    rbr = layer.rho_bias.detach().clone().requires_grad_(True) if layer.mu_bias is not None else None
    op = _op_of(layer)
    if layer._family == "flipout":
        ref = bt_ref.flipout_forward(xr, mur, rhor, mbr, rbr, nz["eps_w"], nz.get("eps_b"), nz["sign_in"].float().reshape(x.shape),
                                     nz["sign_out"].float().reshape(out.shape), op)
    else:
        ref = bt_ref.reparam_forward(xr, mur, rhor, mbr, rbr, nz["eps_w"], nz.get("eps_b"), op)
    klr = bt_ref.kl_loss(mur, rhor, mbr, rbr, layer.prior_mean, layer.prior_variance)
    assert _rel(out.detach(), ref.detach()) < 1e-5
    assert abs(float(kl) - float(klr)) <= 1e-5 * abs(float(klr))
    ((ref * gy).sum() + 3.0 * klr).backward()
    want = dict(x=xr.grad, mu=mur.grad, rho=rhor.grad)
    if mbr is not None:
        want.update(mu_b=mbr.grad, rho_b=rbr.grad)
    for k in want:
        err = _rel(got[k], want[k])
        assert err < 1e-4, (cls, k, err)


def test_model_kl_and_its_gradient_one_launch():
    """get_kl_loss on a CUDA model = btx_kl_gauss_model (+ _bwd): value and d/d(mu, rho) against the ATen expression,
    incl. MOPED-style tensor priors"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models.resnet import resnet18
    from oracle import bt_ref
    dev = _dev()
    torch.manual_seed(0)
    m = resnet18()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=True, moped_delta=0.5))
    m = m.to(dev)
    layers = [l_ for l_ in m.modules() if hasattr(l_, "kl_loss")]
    layers[3].prior_weight_mu.copy_(0.1 * torch.randn_like(layers[3].prior_weight_mu))   # a tensor prior
    kl = bt.get_kl_loss(m)
    kl.backward()
    ref = 0.0
    for l_ in layers:
        mu, rho = l_._w()
        mur, rhor = mu.detach().clone().requires_grad_(True), rho.detach().clone().requires_grad_(True)
        t = bt_ref.kl_div(mur, bt_ref.softplus(rhor), l_.prior_weight_mu, l_.prior_weight_sigma)
        if l_.mu_bias is not None:
            mb, rb = l_.mu_bias.detach().clone().requires_grad_(True), l_.rho_bias.detach().clone().requires_grad_(True)
            t = t + bt_ref.kl_div(mb, bt_ref.softplus(rb), l_.prior_bias_mu, l_.prior_bias_sigma)
        t.backward()
        ref = ref + float(t)
        assert _rel(mu.grad, mur.grad) < 1e-5 and _rel(rho.grad, rhor.grad) < 1e-5, l_
        if l_.mu_bias is not None:
            assert _rel(l_.mu_bias.grad, mb.grad) < 1e-5 and _rel(l_.rho_bias.grad, rb.grad) < 1e-5
    assert abs(float(kl) - ref) <= 1e-5 * abs(ref)


def test_readme_training_snippet_runs_on_the_hip_backend():
    """reference README.md:114-125: output = model(x); kl = get_kl_loss(model); loss = ce + kl / batch; loss.backward();
    optimizer.step() — a few steps on a small converted conv net: loss goes down, every variational parameter moves"""
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.manual_seed(9)
    bt.set_precision("f32")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 32, 3, padding=1), torch.nn.BatchNorm2d(32), torch.nn.ReLU(),
                              torch.nn.Conv2d(32, 64, 3, stride=2, padding=1), torch.nn.ReLU(),
                              torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(64, 10))
    bt.dnn_to_bnn(net, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                            moped_enable=False, moped_delta=0.5))
    net = net.to(dev).train()
    x = torch.randn(32, 3, 16, 16, device=dev)
    y = torch.randint(0, 10, (32,), device=dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    losses = []
    for _ in range(25):
        opt.zero_grad()
        out = net(x)
        kl = bt.get_kl_loss(net)
        loss = torch.nn.functional.cross_entropy(out, y) + kl / 32
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0] - 0.2, losses
    for n, p in net.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n


@pytest.mark.parametrize("kw,xshape", [
    (dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, bias=False), (4, 64, 14, 14)),
    (dict(in_channels=32, out_channels=48, kernel_size=3, stride=2, padding=1), (3, 32, 15, 13)),      # bias sums, ragged tiles
    (dict(in_channels=64, out_channels=96, kernel_size=3, padding=1, groups=2, bias=False), (2, 64, 9, 9)),
    (dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), (2, 3, 32, 32)),  # row-fused stem
])
def test_bf16_activations_train_with_f32_weight_gradients(kw, xshape):
    """throughput mode: bf16 activations + bf16 MFMA forward / data gradient, exact-f32 weight gradient (vectorised staging
    path of btx_wgrad.hip) — against the f32 reference chain on the same bf16-valued tensors (bound 1e-2: 8-bit mantissas
    in the forward / dx operands)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd import functional as BF
    from oracle import bt_ref
    dev = _dev()
    bt.manual_seed(5)
    bt.set_precision("bf16")
    try:
        torch.manual_seed(0)
        layer = L.Conv2dFlipout(**kw).to(dev)
        x = torch.randn(*xshape, device=dev).to(torch.bfloat16).requires_grad_(True)
        bt.set_sample_index(layer, 2)
        out = layer(x, return_kl=False)
        gy = torch.randn_like(out)
        (out.float() * gy.float()).sum().backward()
        mu, rho = layer._w()
        with torch.no_grad():
            nz = layer.materialize_noise(2, tuple(x.shape), tuple(out.shape), x.dtype)
        xr = x.detach().float().requires_grad_(True)
        mur, rhor = BF.plain_layout(mu.detach()).requires_grad_(True), BF.plain_layout(rho.detach()).requires_grad_(True)
        mbr = layer.mu_bias.detach().clone().requires_grad_(True) if layer.mu_bias is not None else None
        rbr = layer.rho_bias.detach().clone().requires_grad_(True) if layer.mu_bias is not None else None
        op = layer._op
        ref = bt_ref.flipout_forward(xr, mur, rhor, mbr, rbr, nz["eps_w"], nz.get("eps_b"), nz["sign_in"].float().reshape(x.shape),
                                     nz["sign_out"].float().reshape(out.shape),
                                     dict(kind="conv", nd=2, stride=op.stride[1:], padding=op.padding[1:], dilation=op.dilation[1:],
                                          groups=op.groups))
        (ref * gy.float()).sum().backward()
        assert _rel(out.float(), ref) < 1e-2
        assert _rel(x.grad.float(), xr.grad) < 1e-2
        assert _rel(mu.grad, mur.grad) < 1e-4 and _rel(rho.grad, rhor.grad) < 1e-4   # f32 MFMA on identical bf16-valued inputs
        if mbr is not None:
            assert _rel(layer.mu_bias.grad, mbr.grad) < 1e-4 and _rel(layer.rho_bias.grad, rbr.grad) < 1e-4
    finally:
        bt.set_precision("f32")


def test_kl_gradient_of_parameters_that_are_not_stored_gemm_major():
    """round-2 advisor finding: KlFn.backward wrote into a packed COPY for parameters without a zero-copy GEMM-major view
    (ConvTranspose with groups > 1; a parameter re-assigned contiguous) and returned uninitialised memory"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from oracle import bt_ref
    dev = _dev()
    torch.manual_seed(0)
    cases = [L.ConvTranspose2dFlipout(8, 12, 3, stride=2, padding=1, groups=2).to(dev),
             L.Conv2dFlipout(16, 24, 3, padding=1).to(dev)]
    w = cases[1].mu_kernel.data.clone(memory_format=torch.contiguous_format)
    cases[1].mu_kernel.data = w  # reference-style MOPED: `layer.mu_kernel.data = w` (plain contiguous storage)
    for layer in cases:
        mu, rho = layer._w()
        kl = layer.kl_loss()
        g = torch.autograd.grad(kl, [mu, rho, layer.mu_bias, layer.rho_bias])
        mu_r, rho_r = mu.detach().clone().requires_grad_(), rho.detach().clone().requires_grad_()
        mb, rb = layer.mu_bias.detach().clone().requires_grad_(), layer.rho_bias.detach().clone().requires_grad_()
        klr = bt_ref.kl_loss(mu_r, rho_r, mb, rb, layer.prior_mean, layer.prior_variance)
        gr = torch.autograd.grad(klr, [mu_r, rho_r, mb, rb])
        assert abs(float(kl) - float(klr)) <= 1e-5 * abs(float(klr))
        for a, b in zip(g, gr):
            assert a.shape == b.shape and _rel(a, b) < 1e-5, (layer.__class__.__name__, _rel(a, b))


def test_fused_resnet_with_grad_enabled_gives_gradients_to_every_conv():
    """round-2 advisor finding: forward_fused() returned a detached tensor under autograd — loss.backward() succeeded and
    silently left every fused conv without a gradient"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models.resnet import resnet18
    from bayesian_torch_amd.models.fuse import fuse_resnet
    dev = _dev()
    bt.set_precision("f32")
    torch.manual_seed(0)
    m = resnet18()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=False, moped_delta=0.5))
    m = m.to(dev).eval()
    bt.assign_layer_ids(m)
    fuse_resnet(m)
    x = torch.randn(1, 3, 224, 224, device=dev, requires_grad=True)
    out = m(x)
    assert out.grad_fn is not None
    out.float().square().mean().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0
    for mod in m.modules():
        if hasattr(mod, "kl_loss"):
            mu, rho = mod._w()
            assert mu.grad is not None and rho.grad is not None, mod.__class__.__name__
            assert float(mu.grad.abs().sum()) > 0


def test_unbatched_inputs_on_the_padded_layouts():
    """round-2 advisor finding: [C,*sp] inputs only worked for plain layers (row-fused stems and channel-padded layers
    indexed a 4-D shape)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    dev = _dev()
    torch.manual_seed(0)
    for layer, shape in ((L.Conv2dFlipout(3, 32, 7, stride=2, padding=3).to(dev), (3, 40, 36)),
                         (L.Conv2dFlipout(20, 24, 3, padding=1).to(dev), (20, 9, 9)),
                         (L.Conv2dReparameterization(16, 16, 3, padding=1).to(dev), (16, 8, 8))):
        x = torch.randn(*shape, device=dev)
        with torch.no_grad():
            a = layer._forward_hip(x, sample_idx=5)
            b = layer._forward_hip(x.unsqueeze(0), sample_idx=5)
        assert a.dim() == 3 and torch.equal(a, b[0])


def test_rho_grad_kernel_matches_the_elementwise_formula():
    """btx_rho_grad: drho = dw * eps * sigmoid(rho) with eps regenerated in the kernel == the same product formed from
    btx_fill_eps values by torch (in place and out of place, a length that is not a multiple of 4)"""
    from bayesian_torch_amd import functional as BF, _lib
    dev = _dev()
    torch.manual_seed(0)
    n = 4099
    dw = torch.randn(n, device=dev)
    rho = torch.randn(n, device=dev) * 3
    eps = BF.fill_eps_hip(n, dev, 1234, 7, 5, _lib.STREAM_EPS_W)
    want = dw * eps * torch.sigmoid(rho)
    got = BF.rho_grad_hip(dw, rho, 1234, 7, 5, _lib.STREAM_EPS_W)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    inplace = dw.clone()
    BF.rho_grad_hip(inplace, rho, 1234, 7, 5, _lib.STREAM_EPS_W, out=inplace)
    assert torch.equal(inplace, got)


# BASELINE cfg4 (ResNet18, batch 64): the distinct variational layer shapes (cin, cout, hw, stride, k)
RN18_SHAPES = [(3, 64, 224, 2, 7), (64, 64, 56, 1, 3), (64, 128, 56, 2, 3), (64, 128, 56, 2, 1), (128, 128, 28, 1, 3),
               (128, 256, 28, 2, 3), (128, 256, 28, 2, 1), (256, 256, 14, 1, 3), (256, 512, 14, 2, 3), (256, 512, 14, 2, 1),
               (512, 512, 7, 1, 3)]


@pytest.mark.parametrize("prec,act,bar", [("f32", torch.float32, 1e-4), ("bf16", torch.bfloat16, 2e-2)])
def test_backward_at_baseline_size_every_resnet18_layer_shape(prec, act, bar):
    """per-layer gradients AT SIZE (cfg4 shapes, batch 64) — dx, dmu, drho of the HIP training path against
    torch autograd through the reference op chain (oracle/bt_ref.py) evaluated by torch on the GPU in f32 with the noise BTX-RNG
    defines.  f32 parity mode: <= 1e-4 (north_star's bar).  bf16 activations: the data gradient runs on the bf16 MFMA (bf16
    operands, f32 accumulation, rounded to bf16 on store: bar 2e-2, measured ~3e-3), the weight gradients on bf16 x bf16
    products with f32 accumulation over 200k..800k pixels against the f32 chain on the same bf16-valued inputs."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd import functional as BF
    from oracle import bt_ref
    dev = _dev()
    bt.manual_seed(77)
    bt.set_precision(prec)
    worst = {}
    try:
        for (cin, cout, hw, stride, k) in RN18_SHAPES:
            torch.manual_seed(cin + cout + hw)
            layer = L.Conv2dFlipout(cin, cout, k, stride=stride, padding=k // 2, bias=False).to(dev)
            x = torch.randn(64, cin, hw, hw, device=dev).to(act).requires_grad_(cin != 3)
            bt.set_sample_index(layer, 4)
            out = layer(x, return_kl=False)
            gy = (torch.randn(out.shape, device=dev) / 64.0).to(act)
            (out.float() * gy.float()).sum().backward()
            mu, rho = layer._w()
            got = dict(mu=mu.grad.float().clone(), rho=rho.grad.float().clone())
            if cin != 3:
                got["x"] = x.grad.float().clone()
            with torch.no_grad():
                nz = layer.materialize_noise(4, tuple(x.shape), tuple(out.shape), x.dtype)
            xr = x.detach().float().clone().requires_grad_(cin != 3)
            mur = BF.plain_layout(mu.detach()).requires_grad_(True)
            rhor = BF.plain_layout(rho.detach()).requires_grad_(True)
            ref = bt_ref.flipout_forward(xr, mur, rhor, None, None, nz["eps_w"], None, nz["sign_in"].float().reshape(x.shape),
                                         nz["sign_out"].float().reshape(out.shape), _op_of(layer))
            (ref * gy.float()).sum().backward()
            want = dict(mu=mur.grad, rho=rhor.grad)
            if cin != 3:
                want["x"] = xr.grad
            for kk in want:
                err = _rel(got[kk], want[kk])
                worst[kk] = max(worst.get(kk, 0.0), err)
                assert err < bar, ((cin, cout, hw, stride, k), prec, kk, err)
            del layer, x, out, gy, xr, ref
        print("backward at size (%s): worst rel-L2 %s" % (prec, {k_: "%.3g" % v for k_, v in worst.items()}))
    finally:
        bt.set_precision("f32")


# ---- training-mode BatchNorm through libbtx (csrc/btx_bn.hip): forward, running estimates, backward vs torch's own BatchNorm ----
BN_CASES = [((8, 64, 56, 56), torch.float32, 2e-5), ((64, 64, 56, 56), torch.bfloat16, 1e-2), ((16, 512, 7, 7), torch.bfloat16, 1e-2),
            ((4, 24, 9, 11), torch.float32, 2e-5), ((3, 2048, 2, 2), torch.bfloat16, 1e-2), ((300, 128), torch.float32, 2e-5)]


@pytest.mark.parametrize("shape,dtype,tol", BN_CASES, ids=["%s-%s" % ("x".join(map(str, c[0])), str(c[1]).split(".")[-1]) for c in BN_CASES])
def test_hip_batchnorm_training_matches_torch(shape, dtype, tol):
    """BatchNorm in training mode on channels-last activations: y, running_mean / running_var / num_batches_tracked, dx, dgamma,
    dbeta against torch.nn.BatchNorm evaluated in FLOAT64 on the same, dtype-rounded, inputs (torch's own f32 kernel loses the
    variance of a channel whose mean dwarfs its spread — 6e-3 on the +300 channels below — the
    shifted sums of btx_bn.hip do not: 1e-7).  bf16: outputs are rounded once to bf16 (bar 1e-2 rel-L2, measured ~2e-3); f32: 2e-5."""
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    from bayesian_torch_amd import autograd as ag
    dev = _dev()
    torch.manual_seed(5)
    C = shape[1]
    cls = torch.nn.BatchNorm2d if len(shape) == 4 else torch.nn.BatchNorm1d
    bn = cls(C, momentum=0.1).to(dev)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C))
        bn.bias.copy_(0.2 * torch.randn(C))
        bn.running_mean.copy_(0.1 * torch.randn(C))
        bn.running_var.copy_(0.5 + torch.rand(C))
    ref = cls(C, momentum=0.1).to(dev).double()
    ref.load_state_dict(bn.state_dict())
    if dtype == torch.bfloat16:
        bn = bn.to(torch.bfloat16)  # parameters and running estimates in bf16, as bench.py's build_model does
        with torch.no_grad():       # the reference starts from the same (bf16-valued) tensors, in f32
            for a, b in zip(ref.state_dict().values(), bn.state_dict().values()):
                a.copy_(b.double())
    x = (torch.randn(*shape, device=dev) * 1.7 + 0.3).to(dtype)
    if dtype == torch.float32 and len(shape) == 4:
        x[:, :4] += 300.0   # channels whose mean dwarfs their spread: the shifted sums must keep their variance
    if len(shape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    dy = torch.randn(*shape, device=dev).to(dtype)
    if len(shape) == 4:
        dy = dy.contiguous(memory_format=torch.channels_last)
    assert hip_batchnorm(bn) == 1
    bn.train(); ref.train()
    x1 = x.clone().requires_grad_(True)
    assert ag.bn_train_usable(bn, x1)
    y = bn(x1)
    y.backward(dy)
    x2 = x.double().clone().requires_grad_(True)
    yr = ref(x2)
    yr.backward(dy.double())
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    errs = dict(y=rel(y, yr), dx=rel(x1.grad, x2.grad), dgamma=rel(bn.weight.grad, ref.weight.grad), dbeta=rel(bn.bias.grad, ref.bias.grad),
                rmean=rel(bn.running_mean, ref.running_mean), rvar=rel(bn.running_var, ref.running_var))
    print("hip batchnorm %s %s: %s" % (shape, dtype, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert y.dtype == dtype and y.shape == x.shape and y.stride() == x.stride()
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    for k, v in errs.items():
        assert v < tol, (k, v)
    # eval mode, CPU tensors and layouts outside the contract keep torch's own path
    bn.eval()
    assert not ag.bn_train_usable(bn, x)
    bn.train()
    if len(shape) == 4:
        assert not ag.bn_train_usable(bn, x.contiguous())  # NCHW storage
        y2 = bn(x.contiguous())
        assert torch.isfinite(y2.float()).all()


@pytest.mark.parametrize("shape,dtype,tol", [((8, 64, 56, 56), torch.float32, 2e-5), ((16, 128, 28, 28), torch.bfloat16, 1e-2),
                                             ((4, 24, 9, 11), torch.float32, 2e-5)])
@pytest.mark.parametrize("variant", ["relu", "res_relu", "res"])
def test_hip_batchnorm_fused_relu_and_residual_match_float64(shape, dtype, tol, variant):
    """autograd.bn_act: y = [relu](bn(x) [+ residual]) inside the normalisation's launches (BtxBnFuse) against the same composition
    of torch ops in float64 — y, dx, d(residual), dgamma, dbeta; the ReLU's backward mask is the bit per element the forward wrote"""
    from bayesian_torch_amd import autograd as ag
    dev = _dev()
    torch.manual_seed(11)
    C = shape[1]
    bn = torch.nn.BatchNorm2d(C, momentum=0.1).to(dev)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C))
        bn.bias.copy_(0.2 * torch.randn(C))
    ref = torch.nn.BatchNorm2d(C, momentum=0.1).to(dev).double()
    ref.load_state_dict(bn.state_dict())
    if dtype == torch.bfloat16:
        bn = bn.to(torch.bfloat16)
        with torch.no_grad():
            for a, b in zip(ref.state_dict().values(), bn.state_dict().values()):
                a.copy_(b.double())
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)  # noqa: E731
    x = cl((torch.randn(*shape, device=dev) * 1.3 + 0.2).to(dtype))
    r = cl(torch.randn(*shape, device=dev).to(dtype)) if "res" in variant else None
    dy = cl(torch.randn(*shape, device=dev).to(dtype))
    relu = "relu" in variant
    bn.train(); ref.train()
    x1 = x.clone().requires_grad_(True)
    r1 = r.clone().requires_grad_(True) if r is not None else None
    assert ag.bn_train_usable(bn, x1)
    y = ag.bn_act(bn, x1, residual=r1, relu=relu)
    y.backward(dy)
    x2 = x.double().clone().requires_grad_(True)
    r2 = r.double().clone().requires_grad_(True) if r is not None else None
    yr = ref(x2)
    if r2 is not None:
        yr = yr + r2
    if relu:
        yr = torch.relu(yr)
    yr.backward(dy.double())
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    errs = dict(y=rel(y, yr), dx=rel(x1.grad, x2.grad), dgamma=rel(bn.weight.grad, ref.weight.grad), dbeta=rel(bn.bias.grad, ref.bias.grad),
                rmean=rel(bn.running_mean, ref.running_mean))
    if r is not None:
        errs["dres"] = rel(r1.grad, r2.grad)
    print("fused batchnorm %s %s %s: %s" % (variant, shape, dtype, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert y.dtype == dtype and y.stride() == x.stride() and int(bn.num_batches_tracked) == 1
    if relu:
        assert float(y.min()) >= 0.0
    for k, v in errs.items():
        assert v < tol, (variant, k, v)
    # a residual of another layout (or eval mode) takes torch's ops and still gives the same function
    if r is not None:
        y2 = ag.bn_act(bn, x, residual=r.contiguous(), relu=relu)
        assert rel(y2, y) < (2e-2 if dtype == torch.bfloat16 else 1e-4)


def test_training_step_with_hip_batchnorm_matches_torch_batchnorm():
    """one training step (README.md:114-125) of a converted ResNet18 at batch 8, f32 parity mode: loss and the gradients of the first
    and the last variational layer with hip_batchnorm(model) against the same model on torch's BatchNorm kernels"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    dev = _dev()
    bt.manual_seed(2024)
    bt.set_precision("f32")
    res = []
    for use_hip in (False, True):
        torch.manual_seed(0)
        m = resnet.resnet18()
        bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                              moped_enable=False, moped_delta=0.5))
        m = m.to(dev).train()
        bt.assign_layer_ids(m)
        if use_hip:
            assert hip_batchnorm(m) == 20
        torch.manual_seed(1)
        x = torch.randn(8, 3, 224, 224, device=dev)
        t = torch.randint(0, 1000, (8,), device=dev)
        bt.set_sample_index(m, 3)
        out = m(x)
        loss = torch.nn.functional.cross_entropy(out, t) + bt.get_kl_loss(m) / 8
        loss.backward()
        res.append((float(loss), m.conv1.mu_kernel.grad.clone(), m.fc.mu_weight.grad.clone(), m.bn1.running_var.clone(),
                    m.layer4[1].bn2.weight.grad.clone()))
    (l0, a0, b0, c0, d0), (l1, a1, b1, c1, d1) = res
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    print("training step, hip vs torch BatchNorm: loss %.6f / %.6f, conv1 dmu %.2e, fc dmu %.2e, bn1 running_var %.2e, bn dgamma %.2e" % (
        l1, l0, rel(a1, a0), rel(b1, b0), rel(c1, c0), rel(d1, d0)))
    assert abs(l1 - l0) < 1e-4 * abs(l0)
    assert rel(a1, a0) < 5e-3 and rel(b1, b0) < 1e-3 and rel(c1, c0) < 1e-5 and rel(d1, d0) < 1e-3


@pytest.mark.parametrize("N,T,C,flip", [(64, 9, 64, True), (128, 9, 64, True), (40, 9, 24, True), (1000, 1, 512, False), (10, 1, 50, False),
                                        (33, 25, 7, True)])
def test_dgrad_weights_one_launch_equals_the_torch_chain(N, T, C, flip):
    """btx_dgrad_weights: (mu, rho, eps) of the data gradient's transposed geometry in one launch == flip / transpose / pack of the
    parameters and of btx_fill_eps's eps by torch ops (bit for bit: a permutation of f32 values and the same Philox draws)"""
    from bayesian_torch_amd import functional as BF
    from bayesian_torch_amd import _lib
    dev = _dev()
    torch.manual_seed(N * 7 + T)
    mu = torch.randn(N, T, C, device=dev)
    rho = torch.randn(N, T, C, device=dev) - 3
    om, orh, oe = BF.dgrad_weights_hip(mu, rho, N, T, C, flip, 77, 5, 13)
    eps = BF.fill_eps_hip(N * T * C, dev, 77, 5, 13, _lib.STREAM_EPS_W).reshape(N, T, C)

    def tr(t):
        t = t.flip(1) if flip else t
        return t.permute(2, 1, 0).contiguous().reshape(-1)
    assert torch.equal(om, tr(mu)) and torch.equal(orh, tr(rho)) and torch.equal(oe, tr(eps))


def test_captured_training_step_equals_the_eager_step():
    """autograd.GraphedTrainStep: forward + CE + KL / B + backward of a converted ResNet18 captured into one hipGraph; a replay with
    the sample word set to s must give the loss and the gradients of the eager step with set_sample_index(model, s) (same kernels,
    same noise; the weight gradient's f32 atomics may reorder sums: 1e-5), and two replays with different words must differ."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = _dev()
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(0)
    m = resnet.resnet18()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=False, moped_delta=0.5))
    m = m.to(dev).train()
    bt.assign_layer_ids(m)
    hip_batchnorm(m)
    for mod in m.modules():  # BatchNorm in eval-like frozen-statistics mode would differ between the two runs: keep momentum 0
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 0.0
    torch.manual_seed(1)
    x = torch.randn(4, 3, 224, 224, device=dev)
    t = torch.randint(0, 1000, (4,), device=dev)

    def eager(s):
        for p_ in m.parameters():
            p_.grad = None
        bt.set_sample_index(m, s)
        out = m(x)
        loss = torch.nn.functional.cross_entropy(out.float(), t) + bt.get_kl_loss(m) / 4
        loss.backward()
        return float(loss), [p_.grad.detach().clone() for p_ in (m.conv1.mu_kernel, m.conv1.rho_kernel, m.layer2[0].conv1.rho_kernel,
                                                                 m.layer4[1].conv2.mu_kernel, m.fc.rho_weight, m.fc.rho_bias, m.bn1.weight)]
    l7, g7 = eager(7)
    gs = GraphedTrainStep(m, x, t)
    la = float(gs.run(7))
    ga = [p_.grad.detach().clone() for p_ in (m.conv1.mu_kernel, m.conv1.rho_kernel, m.layer2[0].conv1.rho_kernel,
                                              m.layer4[1].conv2.mu_kernel, m.fc.rho_weight, m.fc.rho_bias, m.bn1.weight)]
    lb = float(gs.run(8))
    gb = m.layer2[0].conv1.rho_kernel.grad.detach().clone()
    gs.close()
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    errs = [rel(a, b) for a, b in zip(ga, g7)]
    print("captured vs eager training step (sample 7): loss %.6f / %.6f, gradient rel-L2 %s; sample 8 loss %.6f" % (
        la, l7, ", ".join("%.1e" % e for e in errs), lb))
    assert abs(la - l7) < 1e-5 * abs(l7)
    assert max(errs) < 1e-5, errs
    assert abs(lb - la) > 0 and rel(gb, ga[2]) > 1e-3  # another sample index: other noise
    l7b, _ = eager(7)  # the model is back to host-side sample indices
    assert abs(l7b - l7) < 1e-5 * abs(l7)


# gradients at the BASELINE batch against autograd through the reference chain evaluated ON THE CPU (ATen f32 conv backward):
# no GPU library between the HIP gradients and the reference arithmetic (the forward has the same check in test_gpu_at_size.py)
CPU_BWD_CASES = [
    ("taps_56", "Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, bias=False), (64, 64, 56, 56)),
    ("taps2_s2", "Conv2dFlipout", dict(in_channels=128, out_channels=256, kernel_size=3, stride=2, padding=1, bias=False), (64, 128, 28, 28)),
    ("pw_s2", "Conv2dFlipout", dict(in_channels=256, out_channels=512, kernel_size=1, stride=2, bias=False), (64, 256, 14, 14)),
    ("fc", "LinearFlipout", dict(in_features=512, out_features=1000), (64, 512)),
    ("reparam_14", "Conv2dReparameterization", dict(in_channels=256, out_channels=256, kernel_size=3, padding=1, bias=False), (64, 256, 14, 14)),
]


@pytest.mark.parametrize("case", CPU_BWD_CASES, ids=[c[0] for c in CPU_BWD_CASES])
def test_backward_at_baseline_batch_vs_cpu_autograd(case):
    import os
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from oracle import bt_ref
    name, cls, kw, xshape = case
    dev = _dev()
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(3)
    layer = getattr(L, cls)(**kw).to(dev)
    torch.manual_seed(1234)
    x = torch.randn(*xshape, device=dev)
    if len(xshape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    bt.set_sample_index(layer, 9)
    out = layer(x, return_kl=False)
    torch.manual_seed(5)
    dy = torch.randn(out.shape, device=dev)
    out.backward(dy)
    mu, rho = layer._w()
    got = [x.grad, mu.grad, rho.grad] + ([layer.mu_bias.grad, layer.rho_bias.grad] if layer.mu_bias is not None else [])
    # the same function on the CPU: reference op chain + torch autograd, fed with the noise BTX-RNG defines for (layer, sample 9)
    nz = layer.materialize_noise(9, tuple(x.shape), tuple(out.shape), x.dtype)
    c = lambda t: None if t is None else t.detach().float().cpu().contiguous()  # noqa: E731
    xc = c(x).requires_grad_(True)
    muc, rhoc = c(mu).requires_grad_(True), c(rho).requires_grad_(True)
    mbc = c(layer.mu_bias).requires_grad_(True) if layer.mu_bias is not None else None
    rbc = c(layer.rho_bias).requires_grad_(True) if layer.rho_bias is not None else None
    op = dict(kind="linear") if layer._op.nd == 0 else dict(kind="conv", nd=2, stride=layer._op.stride[1:], padding=layer._op.padding[1:],
                                                           dilation=layer._op.dilation[1:], groups=layer._op.groups)
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    if "Flipout" in cls:
        ref = bt_ref.flipout_forward(xc, muc, rhoc, mbc, rbc, c(nz["eps_w"]), c(nz.get("eps_b")), c(nz["sign_in"]), c(nz["sign_out"]), op)
    else:
        ref = bt_ref.reparam_forward(xc, muc, rhoc, mbc, rbc, c(nz["eps_w"]), c(nz.get("eps_b")), op)
    ref.backward(c(dy))
    want = [xc.grad, muc.grad, rhoc.grad] + ([mbc.grad, rbc.grad] if mbc is not None else [])
    errs = [float((g.detach().float().cpu() - w).norm() / w.norm()) for g, w in zip(got, want)]
    print("%s batch %d: dx, dmu, drho%s vs CPU autograd through the reference chain: %s" % (
        name, xshape[0], ", dmu_b, drho_b" if mbc is not None else "", ", ".join("%.2e" % e for e in errs)))
    assert max(errs) < 1e-4, (name, errs)


# ---- the weight gradient's two accumulation paths and its all-taps kernel (csrc/btx_wgrad_taps.h) against the definition ----
WGRAD_TAPS3_CASES = [(3, 64, 128, 7, 9), (2, 128, 64, 5, 63), (4, 64, 64, 14, 14), (16, 256, 256, 14, 14), (5, 64, 64, 2, 2)]


@pytest.mark.parametrize("kind", ["flipout", "reparam"])
def test_wgrad_all_taps_kernel_and_chunk_slabs_equal_the_definition(kind):
    """btx_contract_wgrad_ws on stride-1 3x3 'same' convolutions with bf16 activations (the all-taps kernel: ragged pixel counts,
    the widest supported row, several chunks per tile, a 2x2 image whose every tap touches the border) and btx_contract_wgrad
    (f32 atomics, the tap-per-workgroup kernel) against dW_mu = sum_p dy[p] x[p @ tap], dW_delta = the same on the sign-flipped
    operands, evaluated in float64 on the CPU with the sign tensors btx_fill_sign writes.  bf16 x bf16 products are exact in f32:
    what is left is the f32 accumulation order (<= 2e-6)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as BF
    dev = _dev()
    K = _lib.KIND_FLIPOUT if kind == "flipout" else _lib.KIND_REPARAM
    seed, smp, lid = 991, 3, 11
    try:
        for (nb, cin, cout, h, w) in WGRAD_TAPS3_CASES:
            torch.manual_seed(nb + cin + w)
            op = BF.OpDesc(2, cin, cout, 3, 1, 1)
            x = torch.randn(nb, cin, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            dy = torch.randn(nb, cout, h, w, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            w_shape = (cout, cin, 3, 3)
            xd, dyd = x.double().cpu(), dy.double().cpu()
            want = [torch.nn.grad.conv2d_weight(xd, w_shape, dyd, stride=1, padding=1)]
            if kind == "flipout":
                si = BF.fill_sign_hip(x.numel(), dev, seed, smp, lid, _lib.STREAM_SIGN_IN).reshape(nb, h, w, cin).permute(0, 3, 1, 2)
                so = BF.fill_sign_hip(dy.numel(), dev, seed, smp, lid, _lib.STREAM_SIGN_OUT).reshape(nb, h, w, cout).permute(0, 3, 1, 2)
                want.append(torch.nn.grad.conv2d_weight(xd * si.double().cpu(), w_shape, dyd * so.double().cpu(), stride=1, padding=1))
            for atomics in (False, True):
                BF.WGRAD_ATOMICS = atomics
                got = BF.wgrad_hip(K, x, dy, op, seed, smp, lid, w_shape)
                for g_, w_ in zip(got[:len(want)], want):
                    err = _rel(g_.cpu(), w_)
                    assert err < 2e-6, ((nb, cin, cout, h, w), kind, "atomics" if atomics else "slabs", err)
            # the slab path adds the chunks in a fixed order: two calls agree bit for bit (the atomics path does not promise that)
            BF.WGRAD_ATOMICS = False
            a = BF.wgrad_hip(K, x, dy, op, seed, smp, lid, w_shape)
            b = BF.wgrad_hip(K, x, dy, op, seed, smp, lid, w_shape)
            assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1]))
    finally:
        BF.WGRAD_ATOMICS = False


def test_wgrad_workspace_too_small_is_refused():
    import ctypes
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    dev = _dev()
    g = _lib.Geom()
    g.NB, g.D, g.H, g.W, g.C, g.N = 2, 1, 8, 8, 64, 64
    g.KD, g.KH, g.KW = 1, 3, 3
    g.sd = g.sh = g.sw = 1
    g.pd, g.ph, g.pw = 0, 1, 1
    g.dd = g.dh = g.dw = 1
    g.groups = 1
    need = L.btx_wgrad_workspace_bytes(_lib.KIND_FLIPOUT, ctypes.byref(g), _lib.ACT_BF16, 0)
    assert need == 2 * 2 * 64 * 576 * 4  # 128 pixels = two 64-pixel chunks, mean + delta
    x = torch.zeros(2 * 8 * 8 * 64, dtype=torch.bfloat16, device=dev)
    dw = torch.zeros(2, 64 * 576, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    r = _lib.Rng(1, 0, 0, None)
    st = torch.cuda.current_stream(dev).cuda_stream
    args = (_lib.KIND_FLIPOUT, ctypes.byref(g), x.data_ptr(), x.data_ptr(), dw[0].data_ptr(), dw[1].data_ptr(), None, None,
            ctypes.byref(r), None, _lib.ACT_BF16, 0)
    assert L.btx_contract_wgrad_ws(*args, ws.data_ptr(), need - 4, None, None, st) == -4
    assert L.btx_contract_wgrad_ws(*args, ws.data_ptr() + 4, need, None, None, st) == -6
    assert L.btx_contract_wgrad_ws(*args, ws.data_ptr(), need, dw[0].data_ptr(), None, st) == -1  # rho_w without drho
    dw.fill_(7.0)
    assert L.btx_contract_wgrad_ws(*args, ws.data_ptr(), need, None, None, st) == 0
    torch.cuda.synchronize()
    assert float(dw.abs().max()) == 0.0  # fully overwritten (x = dy = 0), no clearing needed


@pytest.mark.parametrize("shape,dtype,k,s,p", [((64, 64, 112, 112), torch.bfloat16, 3, 2, 1), ((3, 16, 13, 17), torch.float32, 3, 2, 1),
                                               ((2, 8, 9, 9), torch.float32, 2, 2, 0), ((2, 24, 10, 11), torch.bfloat16, 3, 1, 1),
                                               ((2, 8, 12, 12), torch.float32, 5, 3, 2)])
def test_hip_maxpool_under_autograd_equals_torch(shape, dtype, k, s, p):
    """nn.MaxPool2d routed by hip_batchnorm(model) (btx_maxpool2d_cl_train / _bwd): outputs equal torch's exactly; the gradient goes
    to the FIRST maximum of each window in scan order, as torch's does — post-ReLU maps (half the entries tie at 0) included"""
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    from bayesian_torch_amd import autograd as ag
    dev = _dev()
    torch.manual_seed(3)
    x = torch.relu(torch.randn(*shape, device=dev)).to(dtype).contiguous(memory_format=torch.channels_last)
    dy_shape = torch.nn.functional.max_pool2d(x[:1].float(), k, s, p).shape
    dy = torch.randn((shape[0],) + tuple(dy_shape[1:]), device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
    net = torch.nn.Sequential(torch.nn.MaxPool2d(k, s, p))
    hip_batchnorm(net)
    x1 = x.clone().requires_grad_(True)
    assert ag.max_pool_train_usable(net[0], x1)
    y = net(x1)
    y.backward(dy)
    x2 = x.clone().requires_grad_(True)
    yr = torch.nn.functional.max_pool2d(x2, k, s, p)
    yr.backward(dy)
    assert y.shape == yr.shape and y.dtype == dtype and torch.equal(y, yr)
    assert x1.grad.shape == x2.grad.shape and x1.grad.stride() == x.stride()
    if dtype == torch.float32:
        assert torch.allclose(x1.grad, x2.grad, rtol=1e-6, atol=1e-7)
    else:
        assert _rel(x1.grad, x2.grad) < 1e-3  # sums of up to (k/s)^2 bf16 values, rounded once: at most an ulp apart
    assert float((x1.grad != 0).float().mean()) > 0.01
    # no gradient wanted, NCHW storage, return_indices: torch's own op
    assert not ag.max_pool_train_usable(net[0], x) and not ag.max_pool_train_usable(net[0], x.contiguous().requires_grad_(True))
    with torch.no_grad():
        assert torch.equal(net(x), yr.detach())
