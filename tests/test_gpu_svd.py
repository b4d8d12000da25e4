"""BTX-SVD v1 on the GPU: btx_kl_logu_model / _bwd, btx_logalpha_stats / _prune and their Python face against the
float64 model of tests/svd_model.py — the value and EVERY gradient element inside the envelope derived there operation by operation
(envelope.C0_ULP and envelope.DELTA_W, nothing fitted), exact integer statistics, bit-reproducibility, captured steps.
Worst ratios measured on an MI355X: profiles/svd_envelope.txt."""
import copy
import warnings

import numpy as np
import pytest
import torch

import svd_model as M
from test_gpu_alignment import off_grid

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

SEED, G = 1234, 0.37
# below a 4-element group; the block edge (1024 elements); past 64 blocks (the sibling units' per-item cap) with a ragged tail of 4;
# past this unit's own cap of 256 blocks, where blocks stride, with a ragged tail of 3
SIZES = (1, 3, 1023, 1024, 1025, 65540, 262144 + 1027)
REDUCTIONS = ("mean", "sum")


def _dev():
    return torch.device("cuda:0")


def _host(n, seed):
    """(mu, rho) f32 numpy: rho ~ U(-12, 4), mu over eleven decades with exact zeros and runs that clamp on either side"""
    r = np.random.RandomState(1000 * seed + n % 997)
    rho = r.uniform(-12.0, 4.0, n)
    mu = r.randn(n) * np.exp(r.uniform(-8.0, 3.0, n))
    k = max(n // 8, 1)
    if n >= 3:
        mu[:k] = 0.0
        mu[k:2 * k], rho[k:2 * k] = 50.0, -11.0
        mu[2 * k:3 * k], rho[2 * k:3 * k] = 1e-6, 3.0
    return mu.astype(np.float32), rho.astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run(entries, g=G, grads=None, terms=False):
    """forward + backward through the functional face -> (kl numpy scalar, [(dmu, drho) numpy], terms numpy | None)"""
    from bayesian_torch_amd import functional as BF
    out = BF.kl_logu_model_hip(entries, terms=terms)
    kl, tr = out if terms else (out, None)
    if grads is None:
        grads = [(torch.full_like(e[0], float("nan")), torch.full_like(e[0], float("nan"))) for e in entries]
    BF.kl_logu_model_bwd_hip(entries, grads, torch.tensor(g, device=_dev()))
    torch.cuda.synchronize()
    return kl.cpu().numpy().copy(), [(a.cpu().numpy(), b.cpu().numpy()) for a, b in grads], (None if tr is None else tr.cpu().numpy())


def _check_grads(tag, got, m):
    worst = 0.0
    for name, arr in zip(("dmu", "drho"), got):
        assert np.isfinite(arr).all(), (tag, name)
        err, b = np.abs(arr.astype(np.float64) - m[name]), m["b_" + name]
        bad = np.flatnonzero(err > b)
        assert bad.size == 0, "%s %s[%d]: got %r, model %r, bound %.3e" % (tag, name, bad[0], arr[bad[0]], m[name][bad[0]], b[bad[0]])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / b).max()))
    return worst


_CASES = {}


def _case(n, reduction):
    """the inputs, the float64 model and the GPU's results of one (n, reduction), computed once and shared"""
    key = (n, reduction)
    if key not in _CASES:
        mu, rho = _host(n, 3)
        m = M.bounds(mu, rho, G, reduction)
        kl, grads, terms = _run([(_t(mu), _t(rho), reduction)], terms=True)
        _CASES[key] = (mu, rho, m, kl, grads[0], terms)
    return _CASES[key]


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("n", SIZES)
def test_value_and_every_gradient_element_against_the_float64_model(n, reduction):
    mu, rho, m, kl, grads, terms = _case(n, reduction)
    want, bv = M.value_bound([m["kl"]], [m["b_kl"]])
    worst = _check_grads("n=%d %s" % (n, reduction), grads, m)
    print("n=%d %s: kl %.7g (model %.7g), value err/bound %.3g, gradients worst err/bound %.3g, %d elements near a clamp"
          % (n, reduction, float(kl), want, abs(float(kl) - want) / bv, worst, int(m["near"].sum())))
    assert abs(float(kl) - want) <= bv and abs(float(terms[0]) - m["kl"]) <= m["b_kl"]
    if n >= 3:
        k = max(n // 8, 1)
        assert (grads[0][:k] == 0).all()                                          # mu == 0: dmu = 0
        assert (grads[0][k:3 * k] == 0).all() and (grads[1][k:3 * k] == 0).all()  # clamped on either side: exactly 0


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_the_envelope_tells_the_perturbed_references_apart(variant):
    """on the GPU test's own inputs: every perturbed reference leaves the envelope the GPU's results sit in"""
    for reduction in REDUCTIONS:
        mu, rho, m, kl, grads, _ = _case(1025, reduction)
        _, bv = M.value_bound([m["kl"]], [m["b_kl"]])
        ck = M.kl(mu, rho, reduction, variant)
        cm, cr = M.grads(mu, rho, G, reduction, variant)
        with np.errstate(invalid="ignore"):
            out = (not np.isfinite(ck)) or abs(ck - m["kl"]) > bv
            out = out or not np.all(np.abs(cm - m["dmu"]) <= m["b_dmu"]) or not np.all(np.abs(cr - m["drho"]) <= m["b_drho"])
        assert out, (variant, reduction)
        assert abs(float(kl) - m["kl"]) <= bv and _check_grads(variant, grads, m) <= 1.0


def test_49_items_in_one_call_make_two_launches_and_mix_reductions():
    sizes = [1 + (37 * i) % 300 for i in range(49)]
    host = [_host(n, 40 + i) for i, n in enumerate(sizes)]
    entries = [(_t(mu), _t(rho), REDUCTIONS[i % 2]) for i, (mu, rho) in enumerate(host)]
    models = [M.bounds(mu, rho, G, REDUCTIONS[i % 2]) for i, (mu, rho) in enumerate(host)]
    kl, grads, terms = _run(entries, terms=True)
    want, bv = M.value_bound([m["kl"] for m in models], [m["b_kl"] for m in models])
    worst = max(_check_grads("item %d" % i, g, m) for i, (g, m) in enumerate(zip(grads, models)))
    print("49 items: kl %.7g (model %.7g), value err/bound %.3g, gradients worst err/bound %.3g" % (float(kl), want, abs(float(kl) - want) / bv, worst))
    assert abs(float(kl) - want) <= bv
    assert all(abs(float(t) - m["kl"]) <= m["b_kl"] for t, m in zip(terms, models))
    # BTX_FLAG_KL_ACCUM adds to the scalar
    from bayesian_torch_amd import functional as BF
    out = torch.full((), 2.5, device=_dev())
    BF.kl_logu_model_hip(entries, out=out, accumulate=True)
    assert float(out) == float(np.float32(2.5) + np.float32(kl))


def test_reproducible_bits_off_grid_views_and_independence_of_the_call():
    others = [(_t(mu), _t(rho), "sum") for mu, rho in (_host(1 + (53 * i) % 700, 70 + i) for i in range(48))]
    for n in (3, 1025, 65540):
        for reduction in REDUCTIONS:
            mu, rho, m, kl, grads, terms = _case(n, reduction)
            tm, tr = _t(mu), _t(rho)
            # two calls: the same bits
            kl2, g2, t2 = _run([(tm, tr, reduction)], terms=True)
            assert kl2.tobytes() == kl.tobytes() and t2.tobytes() == terms.tobytes()
            assert all(np.array_equal(a, b) for a, b in zip(g2[0], grads))
            # views 1, 2 and 3 floats off the 16-byte grid, gradients too: the scalar path, the same bits
            for nbytes in (4, 8, 12):
                e = [(off_grid(tm, nbytes), off_grid(tr, nbytes), reduction)]
                assert e[0][0].data_ptr() % 16 == nbytes and e[0][1].data_ptr() % 16 == nbytes
                gbuf = [(off_grid(torch.full_like(tm, float("nan")), nbytes), off_grid(torch.full_like(tm, float("nan")), nbytes))]
                kl3, g3, t3 = _run(e, grads=gbuf, terms=True)
                assert kl3.tobytes() == kl.tobytes() and t3.tobytes() == terms.tobytes(), (n, nbytes)
                assert all(np.array_equal(a, b) for a, b in zip(g3[0], grads)), (n, nbytes)
            # alone, and among 48 others (the 49th item: the second launch): the same per-tensor term and gradients
            _, g4, t4 = _run(others + [(tm, tr, reduction)], terms=True)
            assert t4[-1:].tobytes() == terms.tobytes() and all(np.array_equal(a, b) for a, b in zip(g4[-1], grads))
            _, g5, t5 = _run([(tm, tr, reduction)] + others, terms=True)
            assert t5[:1].tobytes() == terms.tobytes() and all(np.array_equal(a, b) for a, b in zip(g5[0], grads))


# ---- layers ------------------------------------------------------------------------------------------------------------------------
LAYERS = {
    "linear_reparam": lambda L: L.LinearReparameterization(33, 7),
    "linear_flipout": lambda L: L.LinearFlipout(33, 7),
    "linear_lrt": lambda L: L.LinearLocalReparameterization(33, 7),
    "conv2d_reparam": lambda L: L.Conv2dReparameterization(5, 6, 3),
    "conv2d_flipout": lambda L: L.Conv2dFlipout(5, 6, 3),
    "conv2d_lrt": lambda L: L.Conv2dLocalReparameterization(5, 6, 3),
    "convT2d_reparam_g2": lambda L: L.ConvTranspose2dReparameterization(4, 6, 3, groups=2),  # contiguous, not stored GEMM-major
    # a `.data` replacement leaves mu and rho in DIFFERENT element orders (GEMM-major against row-major), or one a non-dense view:
    # the kernels then read row-major copies and the gradients must still come back in the logical layout
    "conv2d_rho_relaid_contiguous": lambda L: L.Conv2dReparameterization(5, 6, 3),
    "conv2d_mu_relaid_contiguous": lambda L: L.Conv2dFlipout(5, 6, 3),
    "conv2d_mu_not_dense": lambda L: L.Conv2dLocalReparameterization(5, 6, 3),
}


def _relay(name, layer):
    from bayesian_torch_amd import functional as BF
    mu, rho = layer._w()
    if "rho_relaid" in name:
        rho.data = rho.detach().clone(memory_format=torch.contiguous_format)
    elif "mu_relaid" in name:
        mu.data = mu.detach().clone(memory_format=torch.contiguous_format)
    elif "mu_not_dense" in name:
        wide = torch.empty(tuple(mu.shape) + (2,), device=mu.device)
        wide[..., 0] = mu.detach()
        mu.data = wide[..., 0]
        assert BF.dense_flat(mu) is None
    else:
        assert BF.same_dense_order(mu, rho)
        return
    assert not BF.same_dense_order(mu, rho) and mu.stride() != rho.stride()


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layer_kl_loss_and_gradients_in_logical_layout_match_the_aten_path(name, reduction):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF, layers as L, priors as P
    bt.manual_seed(SEED)
    torch.manual_seed(4)
    layer = LAYERS[name](L)
    with torch.no_grad():
        layer._w()[1].uniform_(-9.0, 1.0)
        BF.dense_flat(layer._w()[0])[::7] = 0.0
    layer = layer.to(_dev()).set_prior(P.LogUniformPrior(reduction))
    _relay(name, layer)
    kl = layer.kl_loss()
    (G * kl).backward()
    # the CPU ATen path in float64 on the same parameters, logical layout
    want, bv, worst = 0.0, 0.0, 0.0
    kls, bkls = [], []
    for mu, rho in (layer._w(), (layer.mu_bias, layer.rho_bias)):
        assert mu.grad.shape == mu.shape and rho.grad.shape == rho.shape
        cm = mu.detach().cpu().double().contiguous().requires_grad_(True)
        cr = rho.detach().cpu().double().contiguous().requires_grad_(True)
        (G * BF.kl_logu_aten(cm, BF.softplus_naive(cr), reduction)).backward()
        m = M.bounds(cm.detach().numpy().reshape(-1), cr.detach().numpy().reshape(-1), G, reduction)
        assert np.allclose(m["dmu"], cm.grad.numpy().reshape(-1), rtol=1e-10, atol=1e-300)
        m["dmu"], m["drho"] = cm.grad.numpy().reshape(-1), cr.grad.numpy().reshape(-1)
        got = (mu.grad.cpu().contiguous().numpy().reshape(-1), rho.grad.cpu().contiguous().numpy().reshape(-1))
        worst = max(worst, _check_grads(name, got, m))
        kls.append(m["kl"])
        bkls.append(m["b_kl"])
    want, bv = M.value_bound(kls, bkls)
    got_kl = float(kl.detach())
    print("%s %s: kl %.7g (aten f64 %.7g), value err/bound %.3g, gradients %.3g" % (name, reduction, got_kl, want, abs(got_kl - want) / bv, worst))
    assert abs(got_kl - want) <= bv
    x = torch.randn((2, layer._op.in_channels) + ((7, 7) if layer._op.nd == 2 else ()), device=_dev())
    with torch.no_grad():
        _, kl2 = layer(x)
    assert torch.equal(kl2, kl.detach())


def test_gaussian_path_is_unchanged_after_set_prior_and_back():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L, models, priors as P
    torch.manual_seed(6)
    net = torch.nn.Sequential(L.Conv2dFlipout(5, 6, 3), L.LinearReparameterization(33, 7), L.LinearLocalReparameterization(7, 3)).to(_dev())
    twin = copy.deepcopy(net)
    models.set_prior(net, P.LogUniformPrior())
    assert not torch.equal(bt.get_kl_loss(net).detach(), bt.get_kl_loss(twin).detach())
    models.set_prior(net, None)
    a, b = bt.get_kl_loss(net), bt.get_kl_loss(twin)
    a.backward()
    b.backward()
    assert torch.equal(a.detach(), b.detach())
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(net.parameters(), twin.parameters()))


def test_a_mixed_model_adds_its_three_groups_in_the_documented_order():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L, priors as P
    bt.manual_seed(SEED)
    torch.manual_seed(6)
    net = torch.nn.Sequential(L.LinearReparameterization(37, 20), L.LinearFlipout(20, 6), L.LinearLocalReparameterization(6, 4)).to(_dev())
    net[1].set_prior(P.ScaleMixturePrior(0.25, 1.0, 0.05), kl_samples=2)
    net[2].set_prior(P.LogUniformPrior("sum"))
    bt.set_sample_index(net, 3)
    total = bt.get_kl_loss(net)
    parts = (net[0].kl_loss() + net[1].kl_loss()) + net[2].kl_loss()
    assert torch.equal(total.detach(), parts.detach())
    total.backward()
    got = [p.grad.clone() for p in net.parameters()]
    for p in net.parameters():
        p.grad = None
    parts.backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(got, net.parameters()))


# ---- captured steps ----------------------------------------------------------------------------------------------------------------
def _capture_net(kind, reduction="mean"):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L, models, priors as P
    bt.manual_seed(SEED)
    bt.set_precision("f32")
    torch.manual_seed(0)
    if kind == "lrt":
        net = torch.nn.Sequential(L.Conv2dLocalReparameterization(8, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                                  L.LinearLocalReparameterization(8 * 6 * 6, 10))
    elif kind == "flipout":
        net = torch.nn.Sequential(L.Conv2dFlipout(8, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), L.LinearFlipout(8 * 6 * 6, 10))
    else:
        net = torch.nn.Sequential(L.Conv2dReparameterization(8, 8, 3, padding=1), torch.nn.ReLU(), L.Conv2dFlipout(8, 8, 3, padding=1),
                                  torch.nn.ReLU(), torch.nn.Flatten(), L.LinearReparameterization(8 * 6 * 6, 10))
    for m in net:
        if hasattr(m, "dnn_to_bnn_flag"):
            m.dnn_to_bnn_flag = True
            m.fused_training = kind == "lrt"
    net = net.to(_dev()).train()
    bt.assign_layer_ids(net)
    if kind == "mixed":
        net[2].set_prior(P.ScaleMixturePrior(0.25, 1.0, 0.05), kl_samples=2)
        net[5].set_prior(P.LogUniformPrior(reduction))
    else:
        models.set_prior(net, P.LogUniformPrior(reduction))
    torch.manual_seed(1)
    return net, torch.randn(4, 8, 6, 6, device=_dev()), torch.randint(0, 10, (4,), device=_dev())


def _eager(net, x, y, s, num_mc):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import mc_train_forward
    from bayesian_torch_amd.utils.mc_loss import mc_elbo_loss
    for p in net.parameters():
        p.grad = None
    if num_mc == 1:
        bt.set_sample_index(net, s, presample=True)
        loss = torch.nn.functional.cross_entropy(net(x).float(), y) + bt.get_kl_loss(net) / x.shape[0]
    else:
        loss = mc_elbo_loss(mc_train_forward(net, x, num_mc, s), y, kl=bt.get_kl_loss(net), reduce="logits")
    loss.backward()
    return loss.detach().clone(), [p.grad.detach().clone() for p in net.parameters()]


@pytest.mark.parametrize("kind", ["flipout", "lrt", "mixed"])
def test_captured_step_is_bit_equal_to_the_eager_step(kind):
    """GraphedTrainStep.run(s), s = 0, 1, 2: the loss and every p.grad equal the eager step at set_sample_index(model, s) bit for bit"""
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = _capture_net(kind)
    want = {s: _eager(net, x, y, s, 1) for s in (0, 1, 2)}
    assert not torch.equal(want[0][0], want[1][0])
    for p in net.parameters():
        p.grad = None
    gs = GraphedTrainStep(net, x, y)
    try:
        for s in (0, 1, 2):
            loss = gs.run(s)
            torch.cuda.synchronize()
            print("%s replay at %d: loss %.7f (eager %.7f)" % (kind, s, float(loss), float(want[s][0])))
            assert torch.equal(loss, want[s][0])
            assert all(torch.equal(p.grad, w) for p, w in zip(net.parameters(), want[s][1]))
    finally:
        gs.close()


@pytest.mark.parametrize("num_mc", [1, 2])
def test_captured_step_with_adam_inside_the_graph(num_mc):
    """optimizer=optim.Adam, reduction "sum": three replays leave every step's loss and the parameters bit-equal to three eager steps"""
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = _capture_net("flipout", "sum")
    params = list(net.parameters())
    start = [p.detach().clone() for p in params]
    opt_e = optim.Adam(params, lr=1e-3)
    losses = []
    for s in (0, 1, 2):
        losses.append(_eager(net, x, y, s, num_mc)[0])
        opt_e.step()
    eager = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, s0 in zip(params, start):
            p.copy_(s0)
            p.grad = None
    gs = GraphedTrainStep(net, x, y, optimizer=optim.Adam(params, lr=1e-3), num_mc=num_mc)
    try:
        for s in (0, 1, 2):
            loss = gs.run(s).clone()
            torch.cuda.synchronize()
            print("captured Adam step %d (num_mc=%d): loss %.7f (eager %.7f)" % (s, num_mc, float(loss), float(losses[s])))
            assert torch.equal(loss, losses[s])
        assert all(torch.equal(p.detach(), e) for p, e in zip(params, eager))
    finally:
        gs.close()


# ---- statistics and pruning ---------------------------------------------------------------------------------------------------------
THRESHOLDS = (-2.0, 3.0, 7.5)
BINS = 64


def _exact_net(seed):
    """Linear -> Conv2d-shaped parameters filled with quarter-bin inputs in their STORAGE order -> (net, [(mu, rho) f32 numpy per tensor
    in report order])"""
    from bayesian_torch_amd import functional as BF, layers as L
    net = torch.nn.Sequential(L.LinearReparameterization(37, 11), L.Conv2dFlipout(5, 6, 3), L.LinearLocalReparameterization(300, 250)).to(_dev())
    host = []
    for i, layer in enumerate(net):
        for mu, rho in (layer._w(), (layer.mu_bias, layer.rho_bias)):
            a, b = M.quarter_bin_inputs(mu.numel(), seed + 10 * i + len(host), THRESHOLDS, BINS)
            with torch.no_grad():
                BF.dense_flat(mu).copy_(_t(a))
                BF.dense_flat(rho).copy_(_t(b))
            host.append((a, b))
    return net, host


def test_stats_and_prune_are_exact_against_the_model():
    from bayesian_torch_amd import functional as BF, sparsity
    net, host = _exact_net(100)
    rep = sparsity.stats(net, THRESHOLDS, BINS, include_bias=True)
    assert [t["numel"] for t in rep["tensors"]] == [37 * 11, 11, 270, 6, 75000, 250]
    for t, (mu, rho) in zip(rep["tensors"], host):
        want = M.stats(mu, rho, THRESHOLDS, BINS)
        assert t["above"] == want["above"] and t["zero_mu"] == want["zero_mu"] and t["hist"] == want["hist"], t["name"]
    assert rep["total"]["numel"] == sum(a.size for a, _ in host) and sum(rep["total"]["hist"]) == rep["total"]["numel"]
    assert sparsity.stats(net, (3.0,))["total"]["above"] == [sum(M.stats(*host[i], (3.0,))["above"][0] for i in (0, 2, 4))]
    versions = [p._version for p in net.parameters()]
    pr = sparsity.prune_(net, threshold=3.0, include_bias=True)
    assert all(p._version > v for p, v in zip(net.parameters(), versions))  # every tensor written: mu / rho of weights and biases
    k = 0
    for layer in net:
        for mu, rho in (layer._w(), (layer.mu_bias, layer.rho_bias)):
            a, b = host[k]
            mask = M.prune_mask(a, b, 3.0)
            gm, gr = BF.dense_flat(mu).cpu().numpy(), BF.dense_flat(rho).cpu().numpy()
            assert pr["tensors"][k]["pruned"] == int(mask.sum())
            assert np.array_equal(gr == M.RHO_PRUNED, mask) and (gm[mask] == 0).all()
            assert np.array_equal(gm[~mask], a[~mask]) and np.array_equal(gr[~mask], b[~mask])
            k += 1
    assert pr["total"]["pruned"] == rep["total"]["above"][1]
    after = sparsity.stats(net, THRESHOLDS, BINS, include_bias=True)
    assert after["total"]["zero_mu"] == rep["total"]["zero_mu"] + sum(int((M.prune_mask(a, b, 3.0) & (a != 0)).sum()) for a, b in host)
    assert sparsity.prune_(net, threshold=3.0, include_bias=True)["total"]["pruned"] == 0
    assert sparsity.stats(net, THRESHOLDS, BINS, include_bias=True) == after


def test_stats_off_the_grid_and_49_tensors():
    from bayesian_torch_amd import functional as BF
    host = [M.quarter_bin_inputs(1 + (91 * i) % 1500, 300 + i, THRESHOLDS, BINS) for i in range(49)]
    pairs = [(off_grid(_t(a), 4 * (1 + i % 3)), off_grid(_t(b), 4 * (1 + i % 3))) for i, (a, b) in enumerate(host)]
    rows = BF.logalpha_stats_hip(pairs, THRESHOLDS, BINS).cpu().tolist()
    for row, (a, b) in zip(rows, host):
        want = M.stats(a, b, THRESHOLDS, BINS)
        assert row[:3] == want["above"] and row[3:8] == [0] * 5 and row[8] == want["zero_mu"] and row[16:] == want["hist"]
    counts = BF.logalpha_prune_hip(pairs, 7.5).cpu().tolist()
    torch.cuda.synchronize()
    for c, (pm, pr), (a, b) in zip(counts, pairs, host):
        mask = M.prune_mask(a, b, 7.5)
        assert c == int(mask.sum()) and np.array_equal(pr.cpu().numpy() == M.RHO_PRUNED, mask)
        assert np.array_equal(pm.cpu().numpy()[~mask], a[~mask])


def test_frozen_eval_model_sees_the_pruned_weights_and_mc_lanes_agree():
    """prune_ through the kernel, then a forward: equal to the forward of the same model whose weights were zeroed with torch ops at the
    same sample index (bit for bit: inside any forward envelope).  The version counters of the tensors written must have moved —
    what caches keyed on (data_ptr, _version) go by."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF, layers as L, mc, sparsity
    bt.manual_seed(SEED)
    bt.set_precision("f32")
    torch.manual_seed(2)
    net = torch.nn.Sequential(L.Conv2dFlipout(8, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(), L.LinearReparameterization(8 * 6 * 6, 10))
    for m in net:
        if hasattr(m, "dnn_to_bnn_flag"):
            m.dnn_to_bnn_flag = True
    net = net.to(_dev()).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    x = torch.randn(4, 8, 6, 6, device=_dev())
    with torch.no_grad():
        bt.set_sample_index(net, 5)
        before = net(x).clone()
    snap = [p.detach().clone() for p in net.parameters()]
    versions = {n: p._version for n, p in net.named_parameters()}
    rep = sparsity.prune_(net, threshold=-1.0)
    assert 0 < rep["total"]["pruned"] < rep["total"]["numel"] and not rep["inclusive"]
    for n, p in net.named_parameters():
        assert (p._version > versions[n]) == ("bias" not in n), n   # weights were written, biases were not selected
    with torch.no_grad():
        bt.set_sample_index(net, 5)
        pruned_out = net(x).clone()
    masks = [(BF.dense_flat(p) == M.RHO_PRUNED) for n, p in net.named_parameters() if n.startswith(("0.rho_k", "3.rho_w"))]
    assert sum(int(mk.sum()) for mk in masks) == rep["total"]["pruned"]
    with torch.no_grad():
        for p, s0 in zip(net.parameters(), snap):
            p.copy_(s0)
        for layer, mk in zip((net[0], net[3]), masks):
            mu, rho = layer._w()
            BF.dense_flat(mu).masked_fill_(mk, 0.0)
            BF.dense_flat(rho).masked_fill_(mk, M.RHO_PRUNED)
        bt.set_sample_index(net, 5)
        torch_out = net(x)
    assert torch.equal(pruned_out, torch_out) and not torch.equal(pruned_out, before)
    assert torch.isfinite(bt.get_kl_loss(net))
    # MC sample lanes on the pruned model: the numbers of one sample at a time
    packed = mc.mc_forward(net, x, 4, lanes=4)
    ref = torch.zeros_like(packed)
    with torch.no_grad(), BF.concurrent_plan(True):
        for s in range(4):
            bt.set_sample_index(net, s, presample=True)
            mc.accumulate_lanes(ref, net(x), 1, 0.0)
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all() and torch.equal(packed, ref)
