"""BTX-KLMC v1 without a GPU: the float64 model against autograd and against its own perturbations, functional.kl_mc_aten on explicit
noise, unbiasedness against closed forms (through the oracle's BTX-RNG), the Python surface and the refusals of the C entry points."""
import copy
import ctypes
import math
import pickle

import numpy as np
import pytest
import torch

import klmc_model as KM

SEED, LAYER, SAMPLE = 1234, 7, 3
LOCS = ("scalar", "tensor")


def _case(n, S, loc_kind, seed=0):
    r = np.random.RandomState(seed + 17 * n + S)
    mu, rho = 0.1 * r.randn(n), r.uniform(-6.0, 0.5, n)
    eps = r.randn(S, n)
    loc = 0.05 if loc_kind == "scalar" else 0.05 * r.randn(n)
    return mu, rho, eps, loc


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _differs(ref, cand, tol):
    """the comparison every check below uses: value and both gradients, relative to the largest reference magnitude"""
    return any(_rel(c, r) > tol for r, c in zip(ref, cand))


def _model_all(mu, rho, eps, spec, loc, variant=None):
    kl = float(KM.forward(mu, rho, eps, spec, loc, variant=variant))
    dmu, drho = KM.grads(mu, rho, eps, spec, loc, variant=variant)
    return kl, dmu.numpy(), drho.numpy()


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("loc_kind", LOCS)
@pytest.mark.parametrize("prior", sorted(KM.PRIORS))
def test_model_gradients_equal_autograd_of_its_forward(prior, loc_kind, S):
    mu, rho, eps, loc = _case(37, S, loc_kind)
    spec = KM.PRIORS[prior]
    tm = torch.tensor(mu, requires_grad=True)
    tr = torch.tensor(rho, requires_grad=True)
    (1.7 * KM.forward(tm, tr, eps, spec, loc)).backward()
    dmu, drho = KM.grads(mu, rho, eps, spec, loc, g=1.7)
    assert _rel(dmu.numpy(), tm.grad.numpy()) <= 1e-12
    assert _rel(drho.numpy(), tr.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("variant", KM.VARIANTS + ("eps_w_stream",))
def test_perturbed_references_are_caught(variant):
    """the comparison of kl_mc_aten with the model (tolerance 1e-5, what the f32 check below uses) flags every wrong estimator"""
    from bayesian_torch_amd import functional as BF, priors as P
    n, S = 37, 4
    mu, rho = KM.case(n, S)
    spec = KM.PRIORS["mix2"]
    eps = KM.oracle_eps(n, S, SEED, SAMPLE, LAYER, KM.STREAM_KL_W)
    tm = torch.tensor(mu, dtype=torch.float32, requires_grad=True)
    tr = torch.tensor(rho, dtype=torch.float32, requires_grad=True)
    kl = BF.kl_mc_aten(tm, torch.log1p(torch.exp(tr)), torch.tensor(eps, dtype=torch.float32), P.ScaleMixturePrior(*spec[1:]))
    kl.backward()
    got = (float(kl.detach()), tm.grad.numpy(), tr.grad.numpy())
    m32, r32 = tm.detach().double().numpy(), tr.detach().double().numpy()
    assert not _differs(_model_all(m32, r32, eps, spec, 0.0), got, 1e-5)
    if variant == "eps_w_stream":
        wrong = _model_all(m32, r32, KM.oracle_eps(n, S, SEED, SAMPLE, LAYER, KM.STREAM_EPS_W), spec, 0.0)
    else:
        wrong = _model_all(m32, r32, eps, spec, 0.0, variant=variant)
    assert _differs(wrong, got, 1e-5), variant


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("loc_kind", LOCS)
@pytest.mark.parametrize("prior", sorted(KM.PRIORS))
def test_kl_mc_aten_equals_the_model_on_explicit_noise(prior, loc_kind, S):
    from bayesian_torch_amd import functional as BF, priors as P
    mu, rho, eps, loc = _case(1025, S, loc_kind, seed=3)
    spec = KM.PRIORS[prior]
    obj = {"mix2": P.ScaleMixturePrior, "laplace": P.LaplacePrior, "student": P.StudentTPrior}[prior](*spec[1:], mu=0.05)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    tm, tr = f32(mu).requires_grad_(), f32(rho).requires_grad_()
    loc_t = None if loc_kind == "scalar" else f32(loc)
    kl = BF.kl_mc_aten(tm, torch.log1p(torch.exp(tr)), f32(eps), obj, loc_t)
    kl.backward()
    m64, r64, e64 = tm.detach().double().numpy(), tr.detach().double().numpy(), f32(eps).double().numpy()
    l64 = 0.05 if loc_t is None else loc_t.double().numpy()
    ref = _model_all(m64, r64, e64, spec, l64)
    # f32 rounding: ~20 operations per element on values of the size of the result, far below 1e-5 relative to the largest magnitude;
    # Laplace's score flips where f32 and f64 disagree on sign(d) — no such element in these draws (|d| >= 1e-6 checked here)
    if prior == "laplace":
        sig = np.logaddexp(0.0, r64)
        assert np.abs(m64[None] + sig[None] * e64 - l64).min() > 1e-6
    assert not _differs(ref, (float(kl.detach()), tm.grad.numpy(), tr.grad.numpy()), 1e-5)


def test_mixture_with_equal_scales_is_the_gaussian():
    from bayesian_torch_amd import priors as P
    w = torch.linspace(-3.0, 3.0, 1001, dtype=torch.float64)
    for pi in (0.1, 0.5, 0.93):
        mix, gau = P.ScaleMixturePrior(pi, 0.3, 0.3, mu=0.2), P.GaussianPrior(0.2, 0.3)
        assert torch.allclose(mix.log_prob(w), gau.log_prob(w), rtol=0, atol=1e-13)
        assert torch.allclose(mix.score(w), gau.score(w), rtol=1e-13, atol=1e-13)
        assert torch.allclose(KM.log_p(("mix2", pi, 0.3, 0.3), w - 0.2), gau.log_prob(w), rtol=0, atol=1e-13)


def test_prior_classes_log_prob_and_score_agree_with_the_model_and_autograd():
    from bayesian_torch_amd import priors as P
    w = torch.linspace(-2.0, 2.0, 401, dtype=torch.float64).requires_grad_()
    for name, cls in (("mix2", P.ScaleMixturePrior), ("laplace", P.LaplacePrior), ("student", P.StudentTPrior)):
        spec = KM.PRIORS[name]
        obj = cls(*spec[1:], mu=0.1)
        lp = obj.log_prob(w)
        assert torch.allclose(lp, KM.log_p(spec, w.detach() - 0.1), rtol=0, atol=1e-13)
        (g,) = torch.autograd.grad(lp.sum(), w)
        assert torch.allclose(obj.score(w.detach()), g, rtol=1e-12, atol=1e-12)
        assert torch.allclose(obj.score(w.detach()), KM.score(spec, w.detach() - 0.1), rtol=1e-12, atol=1e-12)
    assert abs(float(torch.trapezoid(P.StudentTPrior(3.0, 0.2).log_prob(torch.linspace(-400, 400, 2000001, dtype=torch.float64)).exp(),
                                     dx=800 / 2000000)) - 1.0) < 1e-5


def test_argument_validation():
    from bayesian_torch_amd import priors as P
    for bad in (lambda: P.ScaleMixturePrior(0.0, 1, 1), lambda: P.ScaleMixturePrior(1.0, 1, 1), lambda: P.ScaleMixturePrior(0.5, 0, 1),
                lambda: P.ScaleMixturePrior(0.5, 1, -1), lambda: P.ScaleMixturePrior(0.5, 1, 1, mu=float("nan")),
                lambda: P.LaplacePrior(0), lambda: P.LaplacePrior(float("inf")), lambda: P.StudentTPrior(0, 1),
                lambda: P.StudentTPrior(3, 0), lambda: P.StudentTPrior(float("nan"), 1), lambda: P.GaussianPrior(0, 0)):
        with pytest.raises(ValueError):
            bad()
    from bayesian_torch_amd import layers as L
    lin = L.LinearReparameterization(4, 3)
    with pytest.raises(ValueError):
        lin.set_prior(P.LaplacePrior(1.0), kl_samples=0)
    with pytest.raises(TypeError):
        lin.set_prior("laplace")


def _small_net():
    from bayesian_torch_amd import layers as L
    torch.manual_seed(0)
    return torch.nn.Sequential(L.Conv2dFlipout(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                               L.LinearReparameterization(4 * 5 * 5, 6), L.LinearLocalReparameterization(6, 3))


def test_set_prior_surface_and_state_dict():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import models, priors as P
    net = _small_net()
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    torch.manual_seed(5)
    kl0 = bt.get_kl_loss(net)
    prior = P.ScaleMixturePrior(0.25, 1.0, 0.05)
    assert models.set_prior(net, prior, kl_samples=4) is net
    for m in net:
        if hasattr(m, "set_prior"):
            assert m._btx_prior == prior and m._btx_kl_samples == 4 and "ScaleMixturePrior" in repr(m) and "kl_samples=4" in repr(m)
    sd1 = net.state_dict()
    assert list(sd1) == list(sd0) and all(torch.equal(sd1[k], sd0[k]) for k in sd0)
    torch.manual_seed(5)
    kl_a = bt.get_kl_loss(net)
    torch.manual_seed(5)
    kl_b = bt.get_kl_loss(net)
    assert torch.equal(kl_a, kl_b) and not torch.equal(kl_a, kl0) and kl_a.requires_grad
    kl_a.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    out, kl = net[3](torch.randn(2, 100))
    assert kl.requires_grad and kl.dim() == 0
    # back to the Gaussian prior: the same bits as before, repr as before
    models.set_prior(net, P.GaussianPrior())
    assert torch.equal(bt.get_kl_loss(net), kl0) and "prior=" not in repr(net[0])
    net[0].set_prior(prior)
    net[0].set_prior(None)
    assert torch.equal(bt.get_kl_loss(net), kl0)


def test_gaussian_prior_kl_on_cpu_is_bit_equal_to_the_reference_chain():
    """a model that never saw set_prior: get_kl_loss is the sequential sum of kl_div means, as before"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    net = _small_net()
    want = None
    for m in net:
        if hasattr(m, "kl_loss"):
            mu, rho = m._w()
            t = BF.kl_aten(BF.plain_layout(mu), BF.softplus_naive(BF.plain_layout(rho)), m.prior_weight_mu, m.prior_weight_sigma)
            t = t + BF.kl_aten(m.mu_bias, BF.softplus_naive(m.rho_bias), m.prior_bias_mu, m.prior_bias_sigma)
            want = t if want is None else want + t
    assert torch.equal(bt.get_kl_loss(net), want)


def test_cpu_kl_loss_uses_the_tensor_location_after_moped():
    from bayesian_torch_amd import functional as BF, layers as L, priors as P
    torch.manual_seed(1)
    lin = L.LinearReparameterization(5, 4)
    prior = P.LaplacePrior(0.3)
    lin.set_prior(prior, kl_samples=2)
    assert lin._kl_locations() == (None, None)
    lin.prior_weight_mu.copy_(torch.randn(4, 5))
    lin.refresh_priors()
    loc_w, loc_b = lin._kl_locations()
    assert loc_w is lin.prior_weight_mu and loc_b is None
    torch.manual_seed(9)
    kl = lin.kl_loss()
    torch.manual_seed(9)
    eps_w, eps_b = torch.empty(2, 4, 5).normal_(), torch.empty(2, 4).normal_()
    want = BF.kl_mc_aten(lin.mu_weight, BF.softplus_naive(lin.rho_weight), eps_w, prior, lin.prior_weight_mu) + \
        BF.kl_mc_aten(lin.mu_bias, BF.softplus_naive(lin.rho_bias), eps_b, prior)
    assert torch.equal(kl, want)


def test_dnn_to_bnn_keys():
    from bayesian_torch_amd import models, priors as P
    params = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Reparameterization",
                  moped_enable=False, moped_delta=0.5)
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Flatten(), torch.nn.Linear(36, 2))  # noqa: E731
    plain = mk()
    models.dnn_to_bnn(plain, params)
    assert all(m._btx_prior is None for m in plain if hasattr(m, "set_prior"))
    net = mk()
    models.dnn_to_bnn(net, dict(params, prior=P.StudentTPrior(3.0, 0.2), kl_samples=2))
    assert all(m._btx_prior == P.StudentTPrior(3.0, 0.2) and m._btx_kl_samples == 2 for m in net if hasattr(m, "set_prior"))
    assert list(net.state_dict()) == list(plain.state_dict())
    with pytest.raises(Exception, match="LSTM"):
        models.dnn_to_bnn(torch.nn.Sequential(torch.nn.LSTM(4, 3)), dict(params, prior=P.LaplacePrior(1.0)))


def test_pickle_and_deepcopy_round_trip():
    from bayesian_torch_amd import layers as L, priors as P
    lin = L.LinearFlipout(6, 3).set_prior(P.ScaleMixturePrior(0.25, 1.0, 0.05, mu=0.1), kl_samples=3)
    for prior in (P.ScaleMixturePrior(0.25, 1.0, 0.05), P.LaplacePrior(0.3, 0.1), P.StudentTPrior(3.0, 0.2), P.GaussianPrior()):
        assert pickle.loads(pickle.dumps(prior)) == prior and copy.deepcopy(prior) == prior
    cp = copy.deepcopy(lin)
    assert cp._btx_prior == lin._btx_prior and cp._btx_kl_samples == 3 and cp._btx_layer_id != lin._btx_layer_id
    pk = pickle.loads(pickle.dumps(lin))
    assert pk._btx_prior == lin._btx_prior and pk._btx_kl_samples == 3 and torch.equal(pk.mu_weight, lin.mu_weight)


def test_lstm_and_quantized_layers_refuse():
    from bayesian_torch_amd import _lib, layers as L, models, priors as P
    prior = P.LaplacePrior(0.3)
    lstm = L.LSTMReparameterization(4, 3)
    with pytest.raises(_lib.BtxError, match="LSTM"):
        lstm.set_prior(prior)
    with pytest.raises(_lib.BtxError, match="LSTM"):
        lstm.ih.set_prior(prior)
    net = torch.nn.Sequential(L.LinearReparameterization(4, 4), lstm)
    with pytest.raises(_lib.BtxError, match="LSTM"):
        models.set_prior(net, prior)
    assert net[0]._btx_prior is None  # refused before any layer was changed
    assert models.set_prior(net, None) is net and lstm.set_prior(P.GaussianPrior()) is lstm
    from bayesian_torch_amd.layers.variational_layers.quantized_variational import _QuantizedReparameterization
    q = _QuantizedReparameterization.__new__(_QuantizedReparameterization)
    with pytest.raises(_lib.BtxError, match="quantized"):
        _QuantizedReparameterization.set_prior(q, prior)


def _item(L, **kw):
    from bayesian_torch_amd import _lib
    it = (_lib.KlMcItem * 1)()
    one = 16
    it[0].mu, it[0].rho, it[0].dmu, it[0].drho, it[0].n = one, one, one, one, 10
    it[0].prior.type, it[0].prior.loc, it[0].prior.p0, it[0].prior.p1, it[0].prior.p2 = 1, 0.0, 0.25, 1.0, 0.05
    it[0].layer_id, it[0].rng_stream, it[0].sample_idx = 7, 5, 3
    for k, v in kw.items():
        obj, _, attr = k.rpartition("__")
        setattr(it[0].prior if obj == "prior" else it[0], attr, v)
    return it


def test_c_entry_points_refuse_before_any_launch():
    """argument errors of btx_kl_mc_model / _bwd with fake device pointers: every call returns before a kernel is launched"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    big = 1 << 20
    fwd = lambda it, n=1, draws=1, out=one, ws=one, wsb=big: L.btx_kl_mc_model(it, n, SEED, draws, out, 0, ws, wsb, None)  # noqa: E731
    bwd = lambda it, n=1, draws=1, g=one: L.btx_kl_mc_model_bwd(it, n, SEED, draws, g, None)  # noqa: E731
    assert L.btx_kl_mc_workspace_bytes(0) == 0
    assert L.btx_kl_mc_workspace_bytes(1) == L.btx_kl_mc_workspace_bytes(48) == 48 * 64 * 8
    assert L.btx_kl_mc_workspace_bytes(49) == 2 * 48 * 64 * 8
    ok = _item(L)
    # BTX_E_NULL
    assert fwd(None) == -1 and fwd(ok, out=None) == -1 and fwd(ok, ws=None) == -1 and bwd(None) == -1 and bwd(ok, g=None) == -1
    assert fwd(_item(L, mu=None)) == -1 and fwd(_item(L, rho=None)) == -1
    assert bwd(_item(L, dmu=None)) == -1 and bwd(_item(L, drho=None)) == -1
    assert fwd(_item(L, dmu=None, drho=None), wsb=0) == -4  # the forward does not need them (and got as far as the workspace check)
    # BTX_E_SHAPE
    for call in (fwd, bwd):
        assert call(ok, n=0) == -2 and call(ok, draws=0) == -2 and call(ok, draws=1 << 24) == -2
        assert call(_item(L, n=0)) == -2 and call(_item(L, rng_stream=256)) == -2
        for bad in (dict(prior__p0=0.0), dict(prior__p0=1.0), dict(prior__p1=0.0), dict(prior__p2=-1.0), dict(prior__p0=float("nan")),
                    dict(prior__loc=float("inf")), dict(prior__type=2, prior__p0=0.0), dict(prior__type=3, prior__p0=0.0),
                    dict(prior__type=3, prior__p0=3.0, prior__p1=0.0)):
            assert call(_item(L, **bad)) == -2, bad
    # BTX_E_UNSUPPORTED
    for call in (fwd, bwd):
        assert call(_item(L, prior__type=0)) == -3 and call(_item(L, prior__type=4)) == -3
        assert call(_item(L, n=0xfffffffd)) == -3
    # BTX_E_WORKSPACE, BTX_E_ALIGN (the f64 workspace only: parameter pointers on any 4-byte boundary are accepted)
    assert fwd(ok, wsb=48 * 64 * 8 - 1) == -4
    assert fwd(ok, ws=ctypes.c_void_p(20)) == -6
    assert fwd(_item(L, mu=20, rho=28), wsb=0) == -4  # off the 16-byte grid: not an alignment error


@pytest.mark.parametrize("n,S", [(4096, 1), (4099, 4), (65536, 1), (37, 8)])
def test_estimate_is_unbiased_against_the_gaussian_closed_form(n, S):
    """mixture with sigma1 = sigma2 = 0.3 IS N(0, 0.3^2): the estimate must lie within 5 standard errors of the closed-form KL.
    z recorded with the float64 model: -0.48, +0.72, +0.72, -0.57"""
    mu, rho = KM.case(n, S)
    eps = KM.oracle_eps(n, S, SEED, SAMPLE, LAYER, KM.STREAM_KL_W)
    est = float(KM.forward(mu, rho, eps, ("mix2", 0.25, 0.3, 0.3)))
    z = (est - KM.gauss_kl_mean(mu, rho, 0.0, 0.3)) / KM.gauss_se(mu, rho, 0.0, 0.3, S)
    print("n=%d S=%d z=%+.2f" % (n, S, z))
    assert abs(z) <= 5.0


@pytest.mark.parametrize("n,S", [(4096, 1), (4099, 4), (65536, 1), (37, 8)])
def test_estimate_is_unbiased_against_the_laplace_closed_form(n, S):
    mu, rho = KM.case(n, S)
    eps = KM.oracle_eps(n, S, SEED, SAMPLE, LAYER, KM.STREAM_KL_W)
    est = float(KM.forward(mu, rho, eps, ("laplace", 0.3), 0.02))
    z = (est - KM.laplace_kl_mean(mu, rho, 0.02, 0.3)) / KM.laplace_se(rho, 0.3, S)
    print("n=%d S=%d z=%+.2f (SE is an upper bound)" % (n, S, z))
    assert abs(z) <= 5.0


def test_kl_mc_aten_is_the_estimator_the_unbiasedness_checks_model():
    """the ATen composite on the oracle's draws gives the model's estimate: the two tests above speak about the shipped estimator"""
    from bayesian_torch_amd import functional as BF, priors as P
    n, S = 4099, 4
    mu, rho = KM.case(n, S)
    eps = KM.oracle_eps(n, S, SEED, SAMPLE, LAYER, KM.STREAM_KL_W)
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    got = BF.kl_mc_aten(t(mu), torch.log1p(torch.exp(t(rho))), t(eps), P.ScaleMixturePrior(0.25, 0.3, 0.3))
    assert abs(float(got) - float(KM.forward(mu, rho, eps, ("mix2", 0.25, 0.3, 0.3)))) <= 1e-12 * abs(float(got))
    assert math.isfinite(float(got))
