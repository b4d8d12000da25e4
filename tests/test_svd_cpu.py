"""BTX-SVD v1 without a GPU: the float64 model against the true KL and against autograd, perturbed references, the
ATen path, the Python surface, the C entry points' refusals, and sparsity.stats / prune_ on the CPU against the model."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

import svd_model as M

REDUCTIONS = ("mean", "sum")


def _case(n, seed=0):
    """mu / rho (float64 numpy) with exact zeros, elements that clamp on both sides and ordinary ones"""
    r = np.random.RandomState(seed + 13 * n)
    rho = r.uniform(-12.0, 4.0, n)
    mu = r.randn(n) * np.exp(r.uniform(-8.0, 3.0, n))
    k = max(n // 8, 1)
    mu[:k] = 0.0                               # legal; la_raw = 2 log sigma - log EPS
    mu[k:2 * k], rho[k:2 * k] = 50.0, -11.0    # la_raw < -LA_MAX
    mu[2 * k:3 * k], rho[2 * k:3 * k] = 1e-6, 3.0  # la_raw > LA_MAX
    return mu, rho


def _all(mu, rho, reduction, g=1.0, variant=None):
    return (M.kl(mu, rho, reduction, variant),) + M.grads(mu, rho, g, reduction, variant)


def _outside(ref, cand, bnds):
    """does any entry of cand = (kl, dmu, drho) leave the bound around ref?  NaN / inf in cand counts as outside."""
    for r, c, b in zip(ref, cand, bnds):
        err = np.abs(np.asarray(c, dtype=np.float64) - np.asarray(r, dtype=np.float64))
        if not np.all(np.isfinite(err)) or np.any(err > b):
            return True
    return False


def test_approximation_is_the_true_kl_to_0p012():
    """eq. 14 against the quadrature of the true KL on la in [-8, 8]: measured 0.0094 at la = -3.5"""
    la = np.arange(-8.0, 8.0 + 1e-9, 0.25)
    d = np.abs(M.kl_terms(la) - M.kl_quadrature(la))
    print("largest |approximation - quadrature| = %.5f at la = %.2f" % (d.max(), la[int(d.argmax())]))
    assert d.max() <= 0.012


def _torch_forward(mu, rho, reduction):
    """the model's own forward, written in float64 torch so that autograd can differentiate it"""
    sig = torch.log1p(torch.exp(rho))
    raw = 2.0 * torch.log(sig) - torch.log(mu * mu + M.EPS)
    la = torch.clamp(raw, -M.LA_MAX, M.LA_MAX)
    t = M.K1 - M.K1 * torch.sigmoid(M.K2 + M.K3 * la) + 0.5 * torch.log1p(torch.exp(-la))
    return t.mean() if reduction == "mean" else t.sum()


MU_ON_BOUND = 1e-3


def _rho_on_bound(target):
    """a float64 rho for which la_raw(mu = MU_ON_BOUND, rho) is EXACTLY `target` in numpy's and in torch's arithmetic alike (searched
    among the neighbours of the analytic solution: la_raw moves by about one ulp of 20 every few steps of rho)"""
    sig = np.exp(0.5 * (target + np.log(MU_ON_BOUND * MU_ON_BOUND + M.EPS)))
    rho = sig if sig > 40.0 else np.log(np.expm1(sig))
    lo = hi = rho
    for _ in range(4000):
        for cand in (lo, hi):
            t = torch.tensor([cand], dtype=torch.float64)
            m = torch.full((1,), MU_ON_BOUND, dtype=torch.float64)
            raw_t = float(2.0 * torch.log(torch.log1p(torch.exp(t))) - torch.log(m * m + M.EPS))
            if raw_t == target and float(M.la_raw(np.array([MU_ON_BOUND]), np.array([cand]))[0]) == target:
                return cand
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    raise AssertionError("no rho puts la_raw exactly on %r" % (target,))


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_model_gradients_equal_autograd_of_its_forward(reduction):
    mu, rho = _case(64)
    # la_raw EXACTLY on a bound: the gradient passes
    mu[-2:] = MU_ON_BOUND
    rho[-2], rho[-1] = _rho_on_bound(-M.LA_MAX), _rho_on_bound(M.LA_MAX)
    raw = M.la_raw(mu, rho)
    assert raw[-2] == -M.LA_MAX and raw[-1] == M.LA_MAX
    tm, tr = torch.tensor(mu, requires_grad=True), torch.tensor(rho, requires_grad=True)
    kl = _torch_forward(tm, tr, reduction)
    (1.7 * kl).backward()
    dmu, drho = M.grads(mu, rho, 1.7, reduction)
    assert abs(float(kl.detach()) - M.kl(mu, rho, reduction)) <= 1e-12 * abs(float(kl.detach()))
    scale = max(np.abs(dmu).max(), np.abs(drho).max())
    assert np.abs(dmu - tm.grad.numpy()).max() <= 1e-12 * scale and np.abs(drho - tr.grad.numpy()).max() <= 1e-12 * scale
    k = 8
    assert (dmu[:k] == 0).all() and ((drho[:k] == 0) == (raw[:k] > M.LA_MAX)).all()  # mu == 0: dmu = 0; drho = 0 only where it clamps
    assert (dmu[k:3 * k] == 0).all() and (drho[k:3 * k] == 0).all()   # clamped on either side
    assert dmu[-1] != 0 and drho[-1] != 0 and dmu[-2] != 0 and drho[-2] != 0  # on the bound: passes


def test_mu_zero_inside_the_clamp_and_sigma_underflow():
    """mu == 0 with a small sigma stays inside the clamp: dmu = 0, drho != 0.  sigma that underflows: la = -LA_MAX, gradients 0"""
    mu, rho = np.array([0.0, 0.3]), np.array([-9.0, -800.0])
    assert abs(M.la_raw(mu, rho)[0]) < M.LA_MAX and M.log_alpha(mu, rho)[1] == -M.LA_MAX
    dmu, drho = M.grads(mu, rho, 1.0, "sum")
    assert dmu[0] == 0 and drho[0] != 0 and dmu[1] == 0 and drho[1] == 0 and np.isfinite(M.kl(mu, rho, "sum"))
    from bayesian_torch_amd import functional as BF
    tm, tr = torch.tensor(mu, requires_grad=True), torch.tensor(rho, requires_grad=True)
    kl = BF.kl_logu_aten(tm, BF.softplus_naive(tr), "sum")
    kl.backward()
    assert abs(float(kl) - M.kl(mu, rho, "sum")) <= 1e-12 * abs(float(kl))
    assert torch.isfinite(tm.grad).all() and torch.isfinite(tr.grad).all() and tm.grad[1] == 0 and tr.grad[1] == 0


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_perturbed_references_are_caught(variant):
    """each perturbed model must leave BOTH bounds the comparisons of this feature use: the float64 1e-12 and the f32 envelope"""
    mu, rho = _case(257)
    mu32, rho32 = mu.astype(np.float32).astype(np.float64), rho.astype(np.float32).astype(np.float64)
    for reduction in REDUCTIONS:
        ref = _all(mu32, rho32, reduction, 1.3)
        cand = _all(mu32, rho32, reduction, 1.3, variant)
        scale = max(np.abs(ref[1]).max(), np.abs(ref[2]).max())
        assert _outside(ref, cand, (1e-12 * abs(ref[0]), 1e-12 * scale, 1e-12 * scale)), (variant, reduction)
        b = M.bounds(mu32, rho32, 1.3, reduction)
        _, bv = M.value_bound([b["kl"]], [b["b_kl"]])
        assert not _outside(ref, ref, (bv, b["b_dmu"], b["b_drho"]))
        assert _outside(ref, cand, (bv, b["b_dmu"], b["b_drho"])), (variant, reduction)


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_kl_logu_aten_equals_the_model(reduction):
    from bayesian_torch_amd import functional as BF
    mu, rho = _case(257)
    # float64: 1e-12
    tm, tr = torch.tensor(mu, requires_grad=True), torch.tensor(rho, requires_grad=True)
    kl = BF.kl_logu_aten(tm, BF.softplus_naive(tr), reduction)
    (1.3 * kl).backward()
    ref = _all(mu, rho, reduction, 1.3)
    scale = max(np.abs(ref[1]).max(), np.abs(ref[2]).max())
    assert not _outside(ref, (float(kl), tm.grad.numpy(), tr.grad.numpy()), (1e-12 * abs(ref[0]), 1e-12 * scale, 1e-12 * scale))
    la, inside = BF.log_alpha_aten(tm.detach(), BF.softplus_naive(tr.detach()))
    assert np.array_equal(la.numpy(), M.log_alpha(mu, rho)) or np.abs(la.numpy() - M.log_alpha(mu, rho)).max() <= 1e-12
    # f32: inside the derived envelope (the CPU's libm is no worse than the device's measured constants)
    mu32, rho32 = mu.astype(np.float32), rho.astype(np.float32)
    tm, tr = torch.tensor(mu32, requires_grad=True), torch.tensor(rho32, requires_grad=True)
    kl = BF.kl_logu_aten(tm, BF.softplus_naive(tr), reduction)
    (kl * 1.0).backward()
    b = M.bounds(mu32, rho32, 1.0, reduction)
    ref = (b["kl"], b["dmu"], b["drho"])
    # the f32 torch reduction sums n terms in f32 (pairwise): log2(n) + 1 roundings of the partial sums on top of the kernel's bound
    _, bv = M.value_bound([b["kl"]], [b["b_kl"]])
    bv += (np.log2(mu.size) + 1) * M.U32 * float(np.abs(b["term"]).sum()) * (1.0 / mu.size if reduction == "mean" else 1.0)
    assert not _outside(ref, (float(kl), tm.grad.numpy(), tr.grad.numpy()), (bv, b["b_dmu"], b["b_drho"]))


def _small_net():
    from bayesian_torch_amd import layers as L
    torch.manual_seed(0)
    return torch.nn.Sequential(L.Conv2dFlipout(3, 4, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                               L.LinearReparameterization(4 * 5 * 5, 6), L.LinearLocalReparameterization(6, 3))


def test_set_prior_surface_and_state_dict():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import models, priors as P
    assert bt.sparsity is not None and P.LogUniformPrior.deterministic and not P.LaplacePrior.deterministic
    prior = P.LogUniformPrior("sum")
    assert repr(prior) == "LogUniformPrior(reduction='sum')" and repr(P.LogUniformPrior()) == "LogUniformPrior(reduction='mean')"
    assert prior == P.LogUniformPrior("sum") and prior != P.LogUniformPrior() and hash(prior) == hash(P.LogUniformPrior("sum"))
    assert pickle.loads(pickle.dumps(prior)) == prior and copy.deepcopy(prior) == prior
    with pytest.raises(ValueError):
        P.LogUniformPrior("median")
    w = torch.tensor([-2.0, 0.5])
    assert torch.equal(prior.log_prob(w), -torch.log(w.abs())) and torch.equal(prior.score(w), -1.0 / w)
    net = _small_net()
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    kl0 = bt.get_kl_loss(net)
    assert models.set_prior(net, prior) is net
    for m in net:  # all three families
        if hasattr(m, "set_prior"):
            assert m._btx_prior == prior and m._btx_kl_samples == 1 and "LogUniformPrior(reduction='sum')" in repr(m)
    sd1 = net.state_dict()
    assert list(sd1) == list(sd0) and all(torch.equal(sd1[k], sd0[k]) for k in sd0)
    kl_a, kl_b = bt.get_kl_loss(net), bt.get_kl_loss(net)
    assert torch.equal(kl_a, kl_b) and not torch.equal(kl_a, kl0) and kl_a.requires_grad
    want = sum(M.kl(t.detach().double().numpy().reshape(-1), r.detach().double().numpy().reshape(-1), "sum")
               for m in net if hasattr(m, "set_prior") for t, r in (m._w(), (m.mu_bias, m.rho_bias)))
    assert abs(float(kl_a) - want) <= 1e-5 * want
    kl_a.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    out, kl = net[3](torch.randn(2, 100))
    assert kl.requires_grad and kl.dim() == 0
    with pytest.raises(ValueError, match="kl_samples"):
        net[0].set_prior(prior, kl_samples=2)
    with pytest.raises(ValueError, match="kl_samples"):
        models.set_prior(net, prior, kl_samples=4)
    # the location buffers are ignored
    net[3].prior_weight_mu.fill_(0.7)
    net[3].refresh_priors()
    assert torch.equal(bt.get_kl_loss(net), kl_b)
    net[3].prior_weight_mu.fill_(net[3].prior_mean)
    net[3].refresh_priors()
    # back to the Gaussian prior: bit-equal to a fresh layer's KL
    models.set_prior(net, None)
    assert torch.equal(bt.get_kl_loss(net), kl0) and "prior=" not in repr(net[0])
    assert torch.equal(bt.get_kl_loss(net), bt.get_kl_loss(_small_net()))
    cp = copy.deepcopy(net[0].set_prior(prior))
    assert cp._btx_prior == prior and pickle.loads(pickle.dumps(net[0]))._btx_prior == prior


def test_dnn_to_bnn_key_and_refusals():
    from bayesian_torch_amd import _lib, layers as L, models, priors as P
    params = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="LocalReparameterization",
                  moped_enable=False, moped_delta=0.5)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Flatten(), torch.nn.Linear(36, 2))
    models.dnn_to_bnn(net, dict(params, prior=P.LogUniformPrior("sum")))
    assert all(m._btx_prior == P.LogUniformPrior("sum") for m in net if hasattr(m, "set_prior"))
    with pytest.raises(ValueError, match="kl_samples"):
        models.dnn_to_bnn(torch.nn.Sequential(torch.nn.Linear(3, 2)), dict(params, prior=P.LogUniformPrior(), kl_samples=3))
    with pytest.raises(Exception, match="LSTM"):
        models.dnn_to_bnn(torch.nn.Sequential(torch.nn.LSTM(4, 3)), dict(params, type="Reparameterization", prior=P.LogUniformPrior()))
    lstm = L.LSTMReparameterization(4, 3)
    with pytest.raises(_lib.BtxError, match="LSTM"):
        lstm.set_prior(P.LogUniformPrior())
    with pytest.raises(_lib.BtxError, match="LSTM"):
        lstm.ih.set_prior(P.LogUniformPrior())
    from bayesian_torch_amd.layers.variational_layers.quantized_variational import _QuantizedReparameterization
    with pytest.raises(_lib.BtxError, match="quantized"):
        _QuantizedReparameterization.set_prior(_QuantizedReparameterization.__new__(_QuantizedReparameterization), P.LogUniformPrior())


def test_mixed_model_kl_is_the_sum_of_its_three_groups():
    """(Gaussian + sampled) + log-uniform, the documented order"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import priors as P
    net = _small_net()
    net[0].set_prior(P.LaplacePrior(0.3), kl_samples=2)
    net[4].set_prior(P.LogUniformPrior())
    torch.manual_seed(3)
    kl = bt.get_kl_loss(net)
    torch.manual_seed(3)
    parts = [net[0].kl_loss(), net[3].kl_loss(), net[4].kl_loss()]
    assert abs(float(kl) - float(parts[0] + parts[1] + parts[2])) <= 4 * M.U32 * sum(abs(float(p)) for p in parts)
    kl.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def _kl_item(**kw):
    from bayesian_torch_amd import _lib
    it = (_lib.KlLogUItem * 1)()
    it[0].mu, it[0].rho, it[0].dmu, it[0].drho, it[0].n, it[0].reduction = 16, 16, 16, 16, 10, 0
    for k, v in kw.items():
        setattr(it[0], k, v)
    return it


def _la_item(**kw):
    from bayesian_torch_amd import _lib
    it = (_lib.LogAlphaItem * 1)()
    it[0].mu, it[0].rho, it[0].n = 16, 16, 10
    for k, v in kw.items():
        setattr(it[0], k, v)
    return it


def test_c_entry_points_refuse_before_any_launch():
    """argument errors with fake device pointers: every call returns before anything is launched or cleared"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9
    hdr = open(_lib.lib_path().replace("bayesian_torch_amd/libbtx.so", "include/btx.h")).read()
    for n in ("btx_kl_logu_workspace_bytes", "btx_kl_logu_model", "btx_kl_logu_model_bwd", "btx_logalpha_stats", "btx_logalpha_prune"):
        assert n + "(" in hdr and n in _lib.EXPORTS and hasattr(L, n)
    assert ctypes.sizeof(_lib.KlLogUItem) == 48 and ctypes.sizeof(_lib.LogAlphaItem) == 24
    one, big = ctypes.c_void_p(16), 1 << 22
    W = L.btx_kl_logu_workspace_bytes
    assert W(0) == 0 and W(1) == W(48) == (1 + 48 * 256) * 8 and W(49) == (1 + 2 * 48 * 256) * 8
    fwd = lambda it, n=1, out=one, terms=None, ws=one, wsb=big: L.btx_kl_logu_model(it, n, out, terms, 0, ws, wsb, None)  # noqa: E731
    bwd = lambda it, n=1, g=one: L.btx_kl_logu_model_bwd(it, n, g, None)  # noqa: E731
    ok = _kl_item()
    # BTX_E_NULL
    assert fwd(None) == -1 and fwd(ok, out=None) == -1 and fwd(ok, ws=None) == -1 and bwd(None) == -1 and bwd(ok, g=None) == -1
    assert fwd(_kl_item(mu=None)) == -1 and fwd(_kl_item(rho=None)) == -1
    assert bwd(_kl_item(dmu=None)) == -1 and bwd(_kl_item(drho=None)) == -1
    assert fwd(_kl_item(dmu=None, drho=None), wsb=0) == -4  # the forward does not need them (and got as far as the workspace check)
    # BTX_E_SHAPE: n == 0, n_items < 1, an unknown reduction code
    for call in (fwd, bwd):
        assert call(ok, n=0) == -2 and call(ok, n=-1) == -2 and call(_kl_item(n=0)) == -2
        assert call(_kl_item(reduction=2)) == -2 and call(_kl_item(reduction=-1)) == -2
        assert call(_kl_item(n=0xfffffffd)) == -3
    # BTX_E_WORKSPACE, BTX_E_ALIGN (the f64 workspace and terms only: parameter pointers on any 4-byte boundary are accepted)
    assert fwd(ok, wsb=W(1) - 1) == -4 and fwd(_kl_item(reduction=1), wsb=0) == -4
    assert fwd(ok, ws=ctypes.c_void_p(20)) == -6 and fwd(ok, terms=ctypes.c_void_p(20)) == -6
    assert fwd(_kl_item(mu=20, rho=28), wsb=0) == -4  # off the 16-byte grid: not an alignment error
    # statistics and pruning
    th = (ctypes.c_float * 8)(*([3.0] * 8))
    st = lambda it, n=1, t=th, nt=1, bins=0, out=one, hist=None: L.btx_logalpha_stats(it, n, t, nt, bins, out, hist, None)  # noqa: E731
    pr = lambda it, n=1, t=3.0, out=one: L.btx_logalpha_prune(it, n, t, out, None)  # noqa: E731
    la = _la_item()
    assert st(None) == -1 and st(la, out=None) == -1 and st(la, t=None) == -1 and st(la, bins=4) == -1 and st(_la_item(mu=None)) == -1
    assert pr(None) == -1 and pr(la, out=None) == -1 and pr(_la_item(rho=None)) == -1
    assert st(la, n=0) == -2 and st(_la_item(n=0)) == -2 and st(la, nt=9) == -2 and st(la, nt=-1) == -2
    assert st(la, bins=4097, hist=one) == -2 and st(la, bins=-1) == -2
    assert st(la, t=(ctypes.c_float * 8)(float("nan"))) == -2
    assert pr(la, n=0) == -2 and pr(_la_item(n=0)) == -2 and pr(la, t=float("nan")) == -2
    assert st(_la_item(n=0xfffffffd)) == -3 and pr(_la_item(n=0xfffffffd)) == -3
    assert st(la, out=ctypes.c_void_p(20)) == -6 and st(la, bins=4, hist=ctypes.c_void_p(20)) == -6 and pr(la, out=ctypes.c_void_p(20)) == -6


# ---- sparsity.stats / prune_ on the CPU against the model -----------------------------------------------------------------------
THRESHOLDS = (-2.0, 3.0, 7.5)
BINS = 64


def _exact_layer(seed):
    """a Linear layer whose weight and bias hold quarter-bin inputs -> (layer, (mu_w, rho_w), (mu_b, rho_b)) float32 numpy"""
    from bayesian_torch_amd import layers as L
    lin = L.LinearReparameterization(37, 11)
    w, b = M.quarter_bin_inputs(37 * 11, seed, THRESHOLDS, BINS), M.quarter_bin_inputs(11, seed + 1, THRESHOLDS, BINS)
    with torch.no_grad():
        lin.mu_weight.copy_(torch.from_numpy(w[0]).reshape(11, 37))
        lin.rho_weight.copy_(torch.from_numpy(w[1]).reshape(11, 37))
        lin.mu_bias.copy_(torch.from_numpy(b[0]))
        lin.rho_bias.copy_(torch.from_numpy(b[1]))
    return lin, w, b


def test_stats_on_cpu_are_exact_against_the_model():
    from bayesian_torch_amd import sparsity
    lin, w, b = _exact_layer(3)
    net = torch.nn.Sequential(lin)
    rep = sparsity.stats(net, THRESHOLDS, BINS, include_bias=True)
    assert [t["name"] for t in rep["tensors"]] == ["0.weight", "0.bias"] and rep["thresholds"] == THRESHOLDS and rep["bins"] == BINS
    for t, (mu, rho) in zip(rep["tensors"], (w, b)):
        want = M.stats(mu, rho, THRESHOLDS, BINS)
        assert t["numel"] == mu.size and t["above"] == want["above"] and t["zero_mu"] == want["zero_mu"] and t["hist"] == want["hist"]
        assert sum(t["hist"]) == mu.size
    assert rep["tensors"][0]["zero_mu"] > 0 and rep["tensors"][0]["hist"][0] > 0 and rep["tensors"][0]["hist"][-1] > 0
    tot = rep["total"]
    assert tot["numel"] == 37 * 11 + 11 and tot["above"] == [sum(t["above"][k] for t in rep["tensors"]) for k in range(3)]
    assert tot["hist"] == [x + y for x, y in zip(rep["tensors"][0]["hist"], rep["tensors"][1]["hist"])]
    only_w = sparsity.stats(net)
    assert len(only_w["tensors"]) == 1 and only_w["total"]["above"] == [M.stats(w[0], w[1], (3.0,))["above"][0]] and only_w["total"]["hist"] is None
    la_w, la_b = sparsity.log_alpha(lin)
    assert la_w.shape == (11, 37) and la_b.shape == (11,)
    assert np.abs(la_w.numpy().reshape(-1) - M.log_alpha(w[0], w[1])).max() <= 1e-4
    with pytest.raises(ValueError):
        sparsity.stats(net, thresholds=(0.0,) * 9)
    with pytest.raises(ValueError):
        sparsity.stats(net, bins=4097)


def test_prune_on_cpu_is_exact_idempotent_and_bumps_versions():
    from bayesian_torch_amd import sparsity
    lin, w, b = _exact_layer(5)
    net = torch.nn.Sequential(lin)
    v0 = (lin.mu_weight._version, lin.rho_weight._version, lin.mu_bias._version)
    before = sparsity.stats(net, THRESHOLDS, 0, include_bias=True)
    rep = sparsity.prune_(net, threshold=3.0, include_bias=True)
    for t, (mu, rho), pm, pr in zip(rep["tensors"], (w, b), (lin.mu_weight, lin.mu_bias), (lin.rho_weight, lin.rho_bias)):
        mask = M.prune_mask(mu, rho, 3.0)
        assert t["pruned"] == int(mask.sum()) > 0
        got_mu, got_rho = pm.detach().numpy().reshape(-1), pr.detach().numpy().reshape(-1)
        assert np.array_equal(got_mu == 0, mask | (mu == 0)) and np.array_equal(got_rho == M.RHO_PRUNED, mask)   # the pruned indices
        assert np.array_equal(got_mu[~mask], mu[~mask]) and np.array_equal(got_rho[~mask], rho[~mask])      # nothing else moved
    assert rep["total"]["pruned"] == before["total"]["above"][1] and rep["requested"] is None
    assert lin.mu_weight._version > v0[0] and lin.rho_weight._version > v0[1] and lin.mu_bias._version > v0[2]
    after = sparsity.stats(net, THRESHOLDS, 0, include_bias=True)
    again = sparsity.prune_(net, threshold=3.0, include_bias=True)
    assert again["total"]["pruned"] == 0 and sparsity.stats(net, THRESHOLDS, 0, include_bias=True)["total"]["zero_mu"] == after["total"]["zero_mu"]
    # weights only by default
    lin2, w2, _ = _exact_layer(7)
    rep2 = sparsity.prune_(torch.nn.Sequential(lin2))
    assert len(rep2["tensors"]) == 1 and (lin2.rho_bias != M.RHO_PRUNED).all()


def test_prune_fraction_and_ties():
    from bayesian_torch_amd import layers as L, sparsity
    lin, w, _ = _exact_layer(9)
    net = torch.nn.Sequential(lin)
    la = M.log_alpha(w[0], w[1])
    clamped_high = int((la == M.LA_MAX).sum())
    assert clamped_high > 3
    # fewer than the tie at +LA_MAX: every clamped element goes (ties at la >= the threshold), the report says how many
    rep = sparsity.prune_(net, fraction=3.0 / la.size)
    assert rep["requested"] == 3 and rep["total"]["pruned"] == clamped_high and rep["threshold"] == M.LA_MAX and rep["inclusive"]
    # no ties among the rest: exactly the requested number, and exactly the largest ones
    lin, w, _ = _exact_layer(9)
    k = clamped_high + 40
    rep = sparsity.prune_(torch.nn.Sequential(lin), fraction=k / la.size)
    order = np.argsort(-la, kind="stable")
    assert rep["requested"] == k and rep["total"]["pruned"] == k
    assert set(np.flatnonzero(lin.rho_weight.detach().numpy().reshape(-1) == M.RHO_PRUNED)) == set(order[:k])
    assert sparsity.prune_(torch.nn.Sequential(lin), fraction=0.0)["total"]["pruned"] == 0
    with pytest.raises(ValueError):
        sparsity.prune_(torch.nn.Sequential(lin), fraction=1.5)
    with pytest.raises(ValueError):
        sparsity.prune_(torch.nn.Sequential(torch.nn.Linear(2, 2)))
    assert isinstance(lin, L.LinearReparameterization)


def test_kl_and_gradients_stay_finite_after_pruning_for_all_three_prior_kinds():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import models, priors as P, sparsity
    for prior in (None, P.ScaleMixturePrior(0.25, 1.0, 0.05), P.LogUniformPrior("sum")):
        net = _small_net()
        models.set_prior(net, prior)
        for m in net:
            if hasattr(m, "set_prior"):
                m.dnn_to_bnn_flag = True  # forward returns the output alone, as in a converted model
        rep = sparsity.prune_(net, fraction=0.5, include_bias=True)
        assert rep["total"]["pruned"] >= rep["requested"] > 0
        kl = bt.get_kl_loss(net)
        out = net(torch.randn(2, 3, 5, 5))
        (out.sum() + kl).backward()
        assert torch.isfinite(kl) and torch.isfinite(out).all()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters()), prior


@pytest.mark.parametrize("relaid", ["rho_contiguous", "mu_contiguous", "mu_not_dense"])
def test_gradient_buffers_come_back_in_logical_order_when_mu_and_rho_differ_in_layout(relaid):
    """a `.data` replacement may leave mu and rho of one layer in different element orders (GEMM-major against row-major) or one of them
    a non-dense view: the entries are then row-major copies, and a gradient buffer in the ENTRIES' order must come back as the
    logical tensor — checked with buffers that hold 2 * mu and 3 * rho in that order"""
    from bayesian_torch_amd import autograd as AG, functional as BF, layers as L
    torch.manual_seed(3)
    layer = L.Conv2dReparameterization(5, 6, 3)
    shape = tuple(layer.mu_kernel.shape)
    assert not layer.mu_kernel.is_contiguous() and BF.same_dense_order(layer.mu_kernel, layer.rho_kernel)  # stored GEMM-major
    if relaid == "rho_contiguous":
        layer.rho_kernel.data = torch.randn(shape)
    elif relaid == "mu_contiguous":
        layer.mu_kernel.data = torch.randn(shape)
    else:
        layer.mu_kernel.data = torch.randn(shape + (2,))[..., 0]
        assert BF.dense_flat(layer.mu_kernel) is None and BF.dense_flat(layer.rho_kernel) is not None
    mu, rho = layer._w()
    assert not BF.same_dense_order(mu, rho)
    for params in ((mu, rho), (layer.mu_bias, layer.rho_bias)):  # the bias pair: in place, the identity
        (mu_e, rho_e, _), = AG._logu_entries(("sum",), params)
        in_place = BF.same_dense_order(*params)
        assert torch.equal(AG._logical_like(2.0 * mu_e, params[0], in_place), 2.0 * params[0].detach())
        assert torch.equal(AG._logical_like(3.0 * rho_e, params[1], in_place), 3.0 * params[1].detach())
    # and the untouched GEMM-major pair: in place, a strided view
    fresh = L.Conv2dReparameterization(5, 6, 3)
    (mu_e, rho_e, _), = AG._logu_entries(("sum",), fresh._w())
    assert mu_e.data_ptr() == fresh.mu_kernel.data_ptr() and rho_e.data_ptr() == fresh.rho_kernel.data_ptr()
    assert torch.equal(AG._logical_like(2.0 * mu_e, fresh.mu_kernel, True), 2.0 * fresh.mu_kernel.detach())
