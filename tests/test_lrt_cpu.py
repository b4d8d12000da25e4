"""CPU: the local reparameterization layers (LinearLocalReparameterization, Conv{1,2,3}dLocalReparameterization) —
their surface against the Reparameterization twins, the ATen composite against tests/lrt_model.py, the statistics of the output,
and what the host-only C-ABI answers for BTX_KIND_LRT.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import envelope as E
import lrt_model as LM

PAIRS = [
    ("LinearLocalReparameterization", "LinearReparameterization", dict(in_features=12, out_features=7), (5, 12)),
    ("Conv1dLocalReparameterization", "Conv1dReparameterization", dict(in_channels=4, out_channels=6, kernel_size=3, padding=1), (2, 4, 9)),
    ("Conv2dLocalReparameterization", "Conv2dReparameterization", dict(in_channels=4, out_channels=6, kernel_size=3, stride=2, groups=2),
     (2, 4, 7, 7)),
    ("Conv3dLocalReparameterization", "Conv3dReparameterization", dict(in_channels=2, out_channels=4, kernel_size=2, prior_mean=0.0,
                                                                       prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0),
     (2, 2, 3, 4, 4)),
]


def _pair(lrt, twin, kw, seed=0):
    from bayesian_torch_amd import layers as L
    torch.manual_seed(seed)
    a = getattr(L, lrt)(**kw)
    b = getattr(L, twin)(**kw)
    b.load_state_dict(a.state_dict())
    return a, b


def test_classes_exist_and_are_exported():
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.layers import variational_layers as V
    for lrt, twin, _, _ in PAIRS:
        assert hasattr(L, lrt) and lrt in V.local_reparam.__all__
        assert issubclass(getattr(L, lrt), L.BaseVariationalLayer_) and getattr(L, lrt)._family == "lrt"
    assert not hasattr(L, "ConvTranspose2dLocalReparameterization") and not hasattr(L, "LSTMLocalReparameterization")


@pytest.mark.parametrize("lrt,twin,kw,xs", PAIRS, ids=[p[0] for p in PAIRS])
def test_surface_state_dict_and_kl_equal_the_reparameterization_twin(lrt, twin, kw, xs):
    a, b = _pair(lrt, twin, kw)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    torch.manual_seed(1)
    c = type(a)(**kw)
    c.load_state_dict(b.state_dict())          # ... and back
    for k, v in c.state_dict().items():
        assert torch.equal(v, a.state_dict()[k]), k
    assert torch.equal(a.kl_loss(), b.kl_loss())
    x = torch.randn(*xs)
    out, kl = a(x)
    assert torch.equal(kl, b(x)[1]) and out.shape == b(x)[0].shape
    assert torch.is_tensor(a(x, return_kl=False))
    a.dnn_to_bnn_flag = True
    assert torch.is_tensor(a(x))
    assert a.presample_item(0, "bf16") is None


@pytest.mark.parametrize("lrt,twin,kw,xs", PAIRS, ids=[p[0] for p in PAIRS])
def test_cpu_forward_equals_the_model_given_the_same_zeta(lrt, twin, kw, xs):
    """the ATen composite (f32) against lrt_model.forward (float64) at the zeta the layer drew: inside the f32 envelope, plus
    (K + 8) 2^-24 of the magnitudes for the f32 evaluation of the composite itself (envelope.py: "f32 reference").  The same check
    with zeta shifted by one element, with m and v exchanged, and without the bias variance must FAIL: the bound is that sharp."""
    a, _ = _pair(lrt, twin, kw)
    with torch.no_grad():
        a._w()[1].uniform_(-4.0, 0.0)
        a.rho_bias.uniform_(-2.0, 0.0)
    x = torch.randn(*xs, generator=torch.Generator().manual_seed(3)) * 1.5
    torch.manual_seed(21)
    with torch.no_grad():
        out = a(x, return_kl=False)
    torch.manual_seed(21)
    zeta = torch.empty(out.shape).normal_().numpy()
    mu, rho, mb, rb = LM.layer_arrays(a)
    r = LM.forward(x.numpy(), mu, rho, mb, rb, zeta, LM.op_of(a), prec="f32")
    extra = (r["K"] + 8) * E.REF32_UNIT * (r["A_m"] + np.abs(zeta) * np.sqrt(r["v"]))
    rep = E.check(out.numpy(), r["ref"], r["bound"] + extra)
    print(rep.line(lrt, "cpu"))
    assert rep.ok, str(rep)
    bnd = r["bound"] + extra
    wrong_index = r["m"] + np.sqrt(r["v"]) * np.roll(zeta.reshape(-1), 1).reshape(zeta.shape)
    swapped = r["v"] + np.sqrt(np.abs(r["m"])) * zeta
    sb = LM.sigma32(rb).astype(np.float64)
    shp = [1] * zeta.ndim
    shp[1 if zeta.ndim > 2 else -1] = -1
    no_bias_var = r["m"] + np.sqrt(np.maximum(r["v"] - (sb * sb).reshape(shp), 0.0)) * zeta
    for name, bad in (("zeta index", wrong_index), ("swapped accumulators", swapped), ("bias variance", no_bias_var)):
        rb_ = E.check(out.numpy(), bad, bnd)
        assert rb_.violations > 0.5 * rb_.numel and rb_.worst > 100.0, (name, str(rb_))


def test_identical_rows_get_independent_noise_under_lrt_only():
    a, b = _pair(*PAIRS[0][:3])
    x = torch.randn(1, 12).repeat(6, 1)
    with torch.no_grad():
        ya, yb = a(x, return_kl=False), b(x, return_kl=False)
    assert all(torch.equal(yb[0], yb[i]) for i in range(1, 6))
    assert all(not torch.equal(ya[0], ya[i]) for i in range(1, 6))


def test_linear_output_moments_agree_with_m_v_and_with_the_reparameterization_twin():
    """S = 4000 samples of a 3 x 6 output (Linear 10 -> 6).  Per element the sample mean must lie within 6 standard errors
    sqrt(v / S) of m and the sample variance within 6 standard errors v sqrt(2 / (S - 1)) of v — for the LRT layer and for its
    Reparameterization twin alike (a Linear output element has exactly the marginal N(m, v) under both) — and the two layers within
    6 standard errors of the DIFFERENCE of each other (sqrt(2) times the above).  At S = 4000 six standard errors are 9.5 % of
    sqrt(v) for the mean and 13 % of v for the variance: a variance contraction on x instead of x^2, sigma instead of sigma^2 or a
    missing bias variance is several times outside."""
    from bayesian_torch_amd import layers as L
    torch.manual_seed(4)
    a = L.LinearLocalReparameterization(10, 6)
    b = L.LinearReparameterization(10, 6)
    with torch.no_grad():
        a.rho_weight.uniform_(-2.0, 0.0)
        a.rho_bias.uniform_(-2.0, 0.0)
    b.load_state_dict(a.state_dict())
    x = torch.randn(3, 10, generator=torch.Generator().manual_seed(9)) * 1.5
    S = 4000
    mu, rho, mb, rb = LM.layer_arrays(a)
    r = LM.forward(x.numpy(), mu, rho, mb, rb, np.zeros((3, 6)), dict(kind="linear"))
    m, v = r["m"], r["v"]
    se_mean, se_var = np.sqrt(v / S), v * np.sqrt(2.0 / (S - 1))
    torch.manual_seed(100)
    stats = {}
    with torch.no_grad():
        xs = x.repeat(S, 1)   # LRT: S x 3 independent rows in ONE forward; the twin shares one weight draw per forward: S forwards
        ya = a(xs, return_kl=False).reshape(S, 3, 6).double().numpy()
        yb = np.stack([b(x, return_kl=False).double().numpy() for _ in range(S)])
    for name, y in (("lrt", ya), ("reparam", yb)):
        mean, var = y.mean(0), y.var(0, ddof=1)
        stats[name] = (mean, var)
        zm, zv = np.abs(mean - m) / se_mean, np.abs(var - v) / se_var
        print("%s: worst |mean - m| / se %.2f, worst |var - v| / se %.2f" % (name, zm.max(), zv.max()))
        assert (zm <= 6.0).all() and (zv <= 6.0).all(), (name, zm.max(), zv.max())
    dm = np.abs(stats["lrt"][0] - stats["reparam"][0]) / (np.sqrt(2.0) * se_mean)
    dv = np.abs(stats["lrt"][1] - stats["reparam"][1]) / (np.sqrt(2.0) * se_var)
    assert (dm <= 6.0).all() and (dv <= 6.0).all(), (dm.max(), dv.max())
    # the bound is meaningful: sigma in place of sigma^2 in the variance contraction is far outside it
    sg = LM.sigma32(rho).astype(np.float64)
    v_wrong = (x.double().numpy() ** 2) @ sg.T + LM.sigma32(rb).astype(np.float64)
    assert (np.abs(stats["lrt"][1] - v_wrong) / (v_wrong * np.sqrt(2.0 / (S - 1))) > 6.0).all()


def test_sqrt_guard_zero_variance_has_zero_value_and_finite_gradients():
    """all-zero activations and no bias: v == 0 exactly.  The forward gives m (= 0); the composite's gradient of sqrt at 0 is
    DEFINED as 0, so every gradient is finite"""
    from bayesian_torch_amd import layers as L
    torch.manual_seed(0)
    a = L.LinearLocalReparameterization(6, 4, bias=False)
    x = torch.zeros(3, 6, requires_grad=True)
    out = a(x, return_kl=False)
    assert torch.equal(out, torch.zeros(3, 4))
    out.sum().backward()
    for t in (x.grad, a.mu_weight.grad, a.rho_weight.grad):
        assert torch.isfinite(t).all()
    assert torch.equal(a.rho_weight.grad, torch.zeros_like(a.rho_weight))


def test_dnn_to_bnn_converts_a_small_conv_net_and_names_what_it_cannot():
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import dnn_to_bnn
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    params = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="LocalReparameterization",
                  moped_enable=True, moped_delta=0.5)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.BatchNorm2d(8), torch.nn.ReLU(), torch.nn.Flatten(),
                              torch.nn.Linear(8 * 5 * 5, 10))
    w0 = net[0].weight.detach().clone()
    dnn_to_bnn(net, params)
    assert isinstance(net[0], L.Conv2dLocalReparameterization) and isinstance(net[4], L.LinearLocalReparameterization)
    assert torch.equal(net[0].mu_kernel.detach(), w0)          # MOPED works unchanged
    assert net[0].dnn_to_bnn_flag and net[4].dnn_to_bnn_flag
    y = net(torch.randn(2, 3, 5, 5))
    assert y.shape == (2, 10) and torch.isfinite(y).all() and torch.isfinite(get_kl_loss(net))
    for mod, word in ((torch.nn.ConvTranspose2d(3, 4, 2), "ConvTranspose2d"), (torch.nn.LSTM(4, 5), "LSTM")):
        with pytest.raises(AttributeError, match=word):
            dnn_to_bnn(torch.nn.Sequential(mod), dict(params, moped_enable=False))


def test_quantization_entry_points_raise():
    from bayesian_torch_amd import _lib, layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn
    for layer in (L.LinearLocalReparameterization(8, 4), L.Conv2dLocalReparameterization(4, 4, 3)):
        with pytest.raises(_lib.BtxError, match="LocalReparameterization"):
            layer.prepare()
        with pytest.raises(_lib.BtxError, match="LocalReparameterization"):
            bnn_to_qbnn(torch.nn.Sequential(layer))


def test_unsupported_precision_is_named_by_the_python_face():
    """bf16x3 is refused before anything is launched: on a CPU-only machine through the planner's answer"""
    from bayesian_torch_amd import _lib, layers as L
    rc, _ = _plan_info(_lib.KIND_LRT, prec=_lib.PREC_CODE["bf16x3"], act=0)
    assert rc == _lib.E_UNSUPPORTED
    layer = L.LinearLocalReparameterization(8, 4)
    layer.precision = "bf16x3"
    with pytest.raises(_lib.BtxError, match="bf16x3"):
        layer._forward_hip(torch.zeros(2, 8))


def _layer4():
    from bayesian_torch_amd import _lib
    g = _lib.Geom()
    g.NB, g.D, g.H, g.W, g.C, g.N = 64, 1, 7, 7, 512, 512
    g.KD, g.KH, g.KW = 1, 3, 3
    g.sd = g.sh = g.sw = 1
    g.pd, g.ph, g.pw = 0, 1, 1
    g.dd = g.dh = g.dw = 1
    g.groups = 1
    return g


def _plan_info(kind, prec=1, flags=0, g=None, act=1):
    from bayesian_torch_amd import _lib
    g = g or _layer4()
    info = _lib.PlanInfo()
    return _lib.lib().btx_contract_plan_info(kind, ctypes.byref(g), act, prec, flags, None, ctypes.byref(info)), info


def test_host_only_cabi_answers_for_kind_2():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9 and _lib.KIND_LRT == 2 and _lib.STREAM_OUT_NOISE == 4
    hdr = open(_lib.lib_path().replace("bayesian_torch_amd/libbtx.so", "include/btx.h")).read()
    assert "#define BTX_KIND_LRT     2" in hdr and "#define BTX_STREAM_OUT_NOISE 4u" in hdr
    # layer4 of ResNet18 at batch 64 (7x7, 512 -> 512, bf16): kinds 0 and 1 split K, kind 2 never does
    for kind in (0, 1):
        rc, info = _plan_info(kind)
        assert rc == 0 and info.ksplits > 1, (kind, info.ksplits)
    rc, info = _plan_info(_lib.KIND_LRT)
    assert rc == 0 and info.family == 1 and info.ksplits == 1 and info.kper == 9 * 512 and info.ws_bytes == 0
    assert info.nwg == 13 * 8      # ceil(64 * 49 / 256) pixel tiles x 512 / 64 channel tiles
    rc, lanes = _plan_info(_lib.KIND_LRT, flags=20 << _lib.FLAG_LANES_SHIFT)
    assert rc == 0 and lanes.ksplits == 1 and lanes.nwg == info.nwg and lanes.lanes == 20 and lanes.family == 1
    assert L.btx_contract_workspace_bytes(ctypes.byref(_layer4()), 2, 1, 1, 0) == 0
    assert L.btx_contract_workspace_bytes(ctypes.byref(_layer4()), 2, 1, 1, 20 << _lib.FLAG_LANES_SHIFT) == 0
    # ragged channels per group -> the gather kernel
    g = _layer4()
    g.C, g.groups = 516, 1
    rc, info = _plan_info(_lib.KIND_LRT, g=g)
    assert rc == 0 and info.family == 0 and info.ksplits == 1
    # refused before anything is launched
    assert _plan_info(_lib.KIND_LRT, prec=_lib.PREC_CODE["bf16x3"], act=0)[0] == -3
    assert _plan_info(_lib.KIND_LRT, flags=_lib.FLAG_ROWFUSE)[0] == -3
    assert _plan_info(_lib.KIND_LRT, flags=_lib.FLAG_OUT_F32)[0] == -3
    assert _plan_info(_lib.KIND_LRT, flags=_lib.FLAG_OUT_BF16, act=0)[0] == -3
    ep = _lib.Epilogue()
    ep.pool = 1
    info = _lib.PlanInfo()
    assert L.btx_contract_plan_info(2, ctypes.byref(_layer4()), 1, 1, 0, ctypes.byref(ep), ctypes.byref(info)) == -3
    assert _plan_info(3)[0] == -3
    # kinds 0 and 1 keep their plans: the numbers of the parent commit for this shape
    for kind, fam in ((0, 5), (1, 5)):
        rc, info = _plan_info(kind)
        assert (rc, info.family, info.ksplits, info.kper) == (0, fam, 2, 256), (kind, info.family, info.ksplits, info.kper)
