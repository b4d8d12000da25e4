"""GPU: BTX-KLMC v1 (csrc/btx_klmc.hip) — the sampled KL against non-Gaussian priors.  The draws are pinned to
btx_fill_eps bit for bit; the value and every gradient element are compared with the float64 model of tests/klmc_model.py fed with the
materialised draws, inside the envelope its header derives (envelope.C0_ULP and DELTA_W, no constant of its own); then the layers, a
mixed model and captured steps.

Each envelope check prints `name: worst err/bound R`; profiles/klmc_envelope.txt holds the lines of the first run.
"""
import copy
import warnings

import numpy as np
import pytest
import torch

import envelope as E
import klmc_model as KM
from test_gpu_alignment import off_grid

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

SEED, LAYER, SAMPLE, G = 1234, 7, 3, 0.37
SIZES = (1, 3, 37, 1023, 1025, 4099, 65539)   # below a Philox group, across a block (1024 elements), across the item's 64-block cap
LOC = 0.05


def _dev():
    return torch.device("cuda:0")


def _prior(name, spec=None, mu=LOC):
    from bayesian_torch_amd import priors as P
    spec = spec or KM.PRIORS[name]
    return {"mix2": P.ScaleMixturePrior, "laplace": P.LaplacePrior, "student": P.StudentTPrior}[name](*spec[1:], mu=mu)


def _tensors(n, seed, tensor_loc):
    """(mu, rho, loc | None) f32 on the device: mu ~ N(0, 0.1), rho ~ U(-6, 0.5) (sigma from 0.0025 to 1), loc ~ N(0, 0.05)"""
    r = np.random.RandomState(1000 * seed + n % 997)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(_dev())  # noqa: E731
    return t(0.1 * r.randn(n)), t(r.uniform(-6.0, 0.5, n)), (t(0.05 * r.randn(n)) if tensor_loc else None)


def _eps(n, S, layer, stream, sample):
    from bayesian_torch_amd import functional as BF
    return np.stack([BF.fill_eps_hip(n, _dev(), SEED, sample, layer, stream | (j << 8)).cpu().numpy() for j in range(S)]).astype(np.float64)


def _run(entries, S, g=G, grads=None, out=None, accumulate=False):
    """forward + backward through the functional face -> (kl f32 numpy scalar, [(dmu, drho) numpy])"""
    from bayesian_torch_amd import functional as BF
    kl = BF.kl_mc_model_hip(entries, SEED, S, out=out, accumulate=accumulate)
    if grads is None:
        grads = [(torch.full_like(e[0], float("nan")), torch.full_like(e[0], float("nan"))) for e in entries]
    BF.kl_mc_model_bwd_hip(entries, grads, SEED, S, torch.tensor(g, device=_dev()))
    torch.cuda.synchronize()
    return kl.cpu().numpy().copy(), [(a.cpu().numpy(), b.cpu().numpy()) for a, b in grads]


def _model(mu, rho, loc, spec, eps, g=G, scalar_loc=LOC):
    l64 = scalar_loc if loc is None else loc.cpu().numpy().astype(np.float64)
    b = KM.bounds(mu.cpu().numpy(), rho.cpu().numpy(), eps, spec, l64, g, c0=E.C0_ULP, dw=E.DELTA_W)
    b["kl"] = float(b["term"].mean())
    return b


def _check_grads(tag, got, m):
    worst = 0.0
    for name, arr in zip(("dmu", "drho"), got):
        assert np.isfinite(arr).all(), (tag, name)
        ratio = np.abs(arr.astype(np.float64) - m[name]) / m["b_" + name]
        i = int(np.argmax(ratio))
        assert ratio[i] <= 1.0, "%s %s[%d]: got %r, model %r, bound %.3e" % (tag, name, i, arr[i], m[name][i], m["b_" + name][i])
        worst = max(worst, float(ratio[i]))
    return worst


def test_kl_noise_is_fill_eps_at_stream_j():
    """materialize_kl_noise: draw j of the weight is btx_fill_eps at BTX_STREAM_KL_W | j << 8 over the unpadded [n][tap][c] order, of the bias
    at BTX_STREAM_KL_B | j << 8, bit for bit; and the oracle's restatement of BTX-RNG v1 to the tolerance of its own test (2e-5)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF, layers as L
    from oracle import bt_oracle as o
    bt.manual_seed(SEED)
    for layer in (L.Conv2dFlipout(3, 5, 3, padding=1), L.LinearReparameterization(37, 6)):
        layer = layer.to(_dev()).set_prior(_prior("mix2"), kl_samples=3)
        nz = layer.materialize_kl_noise(SAMPLE)
        mu = layer._w()[0]
        assert tuple(nz["eps_w"].shape) == (3,) + tuple(mu.shape) and tuple(nz["eps_b"].shape) == (3, mu.shape[0])
        for j in range(3):
            flat = BF.fill_eps_hip(mu.numel(), _dev(), SEED, SAMPLE, layer._btx_layer_id, 5 | (j << 8))
            if mu.dim() == 4:
                want = flat.reshape(mu.shape[0], mu.shape[2], mu.shape[3], mu.shape[1]).permute(0, 3, 1, 2)
            else:
                want = flat.reshape(mu.shape)
            assert torch.equal(nz["eps_w"][j], want)
            assert np.abs(flat.cpu().numpy() - o.eps(mu.numel(), SEED, SAMPLE, layer._btx_layer_id, 5 | (j << 8))).max() < 2e-5
            fb = BF.fill_eps_hip(mu.shape[0], _dev(), SEED, SAMPLE, layer._btx_layer_id, 6 | (j << 8))
            assert torch.equal(nz["eps_b"][j], fb)
            assert np.abs(fb.cpu().numpy() - o.eps(mu.shape[0], SEED, SAMPLE, layer._btx_layer_id, 6 | (j << 8))).max() < 2e-5
        assert not torch.equal(nz["eps_w"][0], nz["eps_w"][1])


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("tensor_loc", [False, True], ids=["scalar", "tensor"])
@pytest.mark.parametrize("prior", sorted(KM.PRIORS))
def test_value_and_every_gradient_element_against_the_float64_model(prior, tensor_loc, S):
    spec = KM.PRIORS[prior]
    for n in SIZES:
        mu, rho, loc = _tensors(n, S, tensor_loc)
        eps = _eps(n, S, LAYER, 5, SAMPLE)
        kl, grads = _run([(mu, rho, loc, _prior(prior), LAYER, 5, SAMPLE, None)], S)
        m = _model(mu, rho, loc, spec, eps)
        bv = KM.value_bound(m["b_term"], m["kl"])
        rv = abs(float(kl) - m["kl"]) / bv
        rg = _check_grads("%s n=%d" % (prior, n), grads[0], m)
        print("%s %s S=%d n=%d: worst err/bound value %.3g, gradients %.3g" % (prior, "tensor" if tensor_loc else "scalar", S, n, rv, rg))
        assert np.isfinite(kl) and rv <= 1.0, (n, float(kl), m["kl"], bv)


def test_the_envelope_tells_the_perturbed_references_apart():
    """the same comparison against the wrong estimators of tests/klmc_model.py (a dropped 1 / S, sigma1 <-> sigma2, a missing sigmoid(rho),
    sampled entropy, the forward's noise stream): each leaves the envelope in the value or in a gradient element"""
    n, S, spec = 1025, 4, KM.PRIORS["mix2"]
    mu, rho, _ = _tensors(n, 33, False)
    eps = _eps(n, S, LAYER, 5, SAMPLE)
    kl, grads = _run([(mu, rho, None, _prior("mix2"), LAYER, 5, SAMPLE, None)], S)
    m = _model(mu, rho, None, spec, eps)
    m64, r64 = mu.cpu().numpy().astype(np.float64), rho.cpu().numpy().astype(np.float64)

    def outside(e, variant):
        v = float(KM.forward(m64, r64, e, spec, LOC, variant=variant))
        dmu, drho = (t.numpy() for t in KM.grads(m64, r64, e, spec, LOC, g=G, variant=variant))
        return (abs(float(kl) - v) > KM.value_bound(m["b_term"], m["kl"]) or (np.abs(grads[0][0] - dmu) > m["b_dmu"]).any() or
                (np.abs(grads[0][1] - drho) > m["b_drho"]).any())
    assert not outside(eps, None)
    for variant in KM.VARIANTS:
        assert outside(eps, variant), variant
    assert outside(_eps(n, S, LAYER, 0, SAMPLE), None), "BTX_STREAM_EPS_W"


@pytest.mark.parametrize("count", [1, 2, 49])
def test_item_counts_in_one_call(count):
    """1, 2 and 49 tensors (one more than a batch holds) of mixed priors, sizes, locations and streams in ONE call"""
    names = sorted(KM.PRIORS)
    sizes = (37, 1025, 3, 4099, 1, 1023)
    entries, models = [], []
    for i in range(count):
        name, n, stream = names[i % 3], sizes[i % len(sizes)], 5 + (i & 1)
        mu, rho, loc = _tensors(n, 50 + i, tensor_loc=(i % 4 == 1))
        entries.append((mu, rho, loc, _prior(name), LAYER + i, stream, SAMPLE + i, None))
        models.append(_model(mu, rho, loc, KM.PRIORS[name], _eps(n, 2, LAYER + i, stream, SAMPLE + i)))
    kl, grads = _run(entries, 2)
    want = sum(m["kl"] for m in models)
    bv = sum(float(np.mean(m["b_term"])) for m in models) + KM.U32 * abs(want)
    worst = max(_check_grads("item %d" % i, grads[i], m) for i, m in enumerate(models))
    print("%d items: value err/bound %.3g, gradients %.3g" % (count, abs(float(kl) - want) / bv, worst))
    assert abs(float(kl) - want) <= bv


def test_accumulate_flag_and_grouping_of_items_into_calls():
    """BTX_FLAG_KL_ACCUM adds to the scalar in f32; a tensor's value does not depend on the call it sits in: accumulating item by item gives
    the f32 sum of the separate calls bit for bit, and two calls return identical bits"""
    from bayesian_torch_amd import functional as BF
    entries, singles = [], []
    for i, (name, n) in enumerate((("mix2", 4099), ("laplace", 1025), ("student", 65539))):
        mu, rho, loc = _tensors(n, 70 + i, tensor_loc=(i == 1))
        entries.append((mu, rho, loc, _prior(name), LAYER + i, 5, SAMPLE, None))
    for e in entries:
        a = BF.kl_mc_model_hip([e], SEED, 2).cpu().numpy().copy()
        b = BF.kl_mc_model_hip([e], SEED, 2).cpu().numpy().copy()
        assert a.tobytes() == b.tobytes()
        singles.append(np.float32(a))
    out = torch.zeros((), dtype=torch.float32, device=_dev())
    run = np.float32(0.0)
    for e, s in zip(entries, singles):
        BF.kl_mc_model_hip([e], SEED, 2, out=out, accumulate=True)
        run = np.float32(run + s)
    assert out.cpu().numpy().tobytes() == run.tobytes()
    # the accumulated value against the model: the bound of the value plus the f32 additions
    mu, rho, loc = entries[0][:3]
    m = _model(mu, rho, loc, KM.PRIORS["mix2"], _eps(4099, 2, LAYER, 5, SAMPLE))
    out.fill_(2.5)
    BF.kl_mc_model_hip([entries[0]], SEED, 2, out=out, accumulate=True)
    assert abs(float(out) - (2.5 + m["kl"])) <= KM.value_bound(m["b_term"], m["kl"], previous=2.5)
    a = BF.kl_mc_model_hip(entries, SEED, 2).cpu().numpy().copy()
    b = BF.kl_mc_model_hip(entries, SEED, 2).cpu().numpy().copy()
    assert a.tobytes() == b.tobytes()


def test_exact_run_against_the_gaussian_closed_form():
    """sigma1 = sigma2 makes the prior N(loc, sp^2); with rho chosen so that sigma is a power of two (up to the rounding of rho) the value is
    btx_kl_gauss_model's closed form plus the sampled remainder the float64 model gives: (1 / n) sum_i [E - mean_j] (d_j^2) / (2 sp^2).
    Bound: the sampled value's own, plus the closed form's — per element DW + (2 c0 + 2) u |log sig| + 2 c0 u |log sp| +
    (2 DW + 8 u) (sig^2 + dm^2) / (2 sp^2) + 4 u (|log sp| + |log sig| + (sig^2 + dm^2) / (2 sp^2) + 1 / 2), and u |kl| for its store."""
    from bayesian_torch_amd import functional as BF
    n, S, sp = 4099, 4, 0.3
    r = np.random.RandomState(5)
    sig = 2.0 ** r.randint(-8, 1, n)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(_dev())  # noqa: E731
    mu, rho = t(0.1 * r.randn(n)), t(np.log(np.expm1(sig)))
    spec = ("mix2", 0.25, sp, sp)
    e = (mu, rho, None, _prior("mix2", spec), LAYER, 5, SAMPLE, None)
    got = float(BF.kl_mc_model_hip([e], SEED, S))
    gauss = float(BF.kl_model_hip([(mu, rho, LOC, sp, None, None)]))
    eps = _eps(n, S, LAYER, 5, SAMPLE)
    m = _model(mu, rho, None, spec, eps)
    m64, r64 = mu.cpu().numpy().astype(np.float64), rho.cpu().numpy().astype(np.float64)
    closed = KM.gauss_kl_mean(m64, r64, LOC, sp)
    remainder = m["kl"] - closed
    s64, u, c0, dw = np.logaddexp(0.0, r64), KM.U32, E.C0_ULP, E.DELTA_W
    quad = (s64 ** 2 + (m64 - LOC) ** 2) / (2 * sp * sp)
    b_gauss = float(np.mean(dw + (2 * c0 + 2) * u * np.abs(np.log(s64)) + 2 * c0 * u * abs(np.log(sp)) + (2 * dw + 8 * u) * quad +
                            4 * u * (abs(np.log(sp)) + np.abs(np.log(s64)) + quad + 0.5))) + u * abs(closed)
    bound = KM.value_bound(m["b_term"], m["kl"]) + b_gauss
    print("exact run: sampled %.7f = closed form %.7f + remainder %+.7f; err/bound %.3g" % (got, gauss, remainder, abs(got - (gauss + remainder)) / bound))
    assert abs(gauss - closed) <= b_gauss
    assert abs(got - (gauss + remainder)) <= bound
    assert float(BF.kl_mc_model_hip([e], SEED, S)) == got


@pytest.mark.parametrize("nbytes", [4, 12])
def test_pointers_off_the_16_byte_grid(nbytes):
    """mu / rho / loc / dmu / drho as views `nbytes` past a 16-byte boundary: accepted (no BTX_E_ALIGN), the scalar path, the same envelope — and
    the same bits as on the grid"""
    for prior in sorted(KM.PRIORS):
        for n in (37, 1025, 4099):
            mu, rho, loc = _tensors(n, 90, tensor_loc=True)
            on = [(mu, rho, loc, _prior(prior), LAYER, 5, SAMPLE, None)]
            off = [(off_grid(mu, nbytes), off_grid(rho, nbytes), off_grid(loc, nbytes), _prior(prior), LAYER, 5, SAMPLE, None)]
            assert off[0][0].data_ptr() % 16 == nbytes and off[0][1].data_ptr() % 16 == nbytes
            gbuf = [(off_grid(torch.full_like(mu, float("nan")), nbytes), off_grid(torch.full_like(mu, float("nan")), nbytes))]
            kl_on, g_on = _run(on, 2)
            kl_off, g_off = _run(off, 2, grads=gbuf)
            m = _model(mu, rho, loc, KM.PRIORS[prior], _eps(n, 2, LAYER, 5, SAMPLE))
            assert abs(float(kl_off) - m["kl"]) <= KM.value_bound(m["b_term"], m["kl"])
            worst = _check_grads("%s n=%d +%d" % (prior, n, nbytes), g_off[0], m)
            print("%s n=%d at +%d bytes: gradients worst err/bound %.3g" % (prior, n, nbytes, worst))
            assert kl_on.tobytes() == kl_off.tobytes() and all(np.array_equal(a, b) for a, b in zip(g_on[0], g_off[0]))


# ---- layers ------------------------------------------------------------------------------------------------------------------------
def _moped_linear():
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.utils.util import MOPED
    torch.manual_seed(2)
    det = torch.nn.Sequential(torch.nn.Linear(37, 6))
    net = torch.nn.Sequential(L.LinearReparameterization(37, 6))
    MOPED(net, det, None, 0.2)
    return net[0]


LAYERS = {
    "linear_reparam": lambda L: L.LinearReparameterization(37, 6),
    "conv2d_flipout_c3": lambda L: L.Conv2dFlipout(3, 8, 3, padding=1),                                  # channel-padded execution
    "convT2d_reparam_g2": lambda L: L.ConvTranspose2dReparameterization(4, 6, 3, groups=2),             # not stored GEMM-major
    "linear_lrt": lambda L: L.LinearLocalReparameterization(40, 5),
    "moped_linear": lambda L: _moped_linear(),
}


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layer_kl_loss_and_gradients_in_logical_layout(name):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(SEED)
    torch.manual_seed(4)
    layer = LAYERS[name](L).to(_dev())
    with torch.no_grad():
        layer._w()[1].uniform_(-5.0, 0.0)
    prior, S = _prior("mix2"), 2
    layer.set_prior(prior, kl_samples=S)
    bt.set_sample_index(layer, SAMPLE)
    loc_w, loc_b = layer._kl_locations()
    assert (loc_w is not None) == (name == "moped_linear")
    kl = layer.kl_loss()
    (G * kl).backward()
    nz = layer.materialize_kl_noise(SAMPLE)
    mu, rho = layer._w()
    flat = lambda t_: t_.detach().contiguous().reshape(-1)  # noqa: E731
    mw = _model(flat(mu), flat(rho), None if loc_w is None else flat(loc_w), KM.PRIORS["mix2"],
                nz["eps_w"].reshape(S, -1).cpu().numpy().astype(np.float64))
    mb = _model(flat(layer.mu_bias), flat(layer.rho_bias), None if loc_b is None else flat(loc_b), KM.PRIORS["mix2"],
                nz["eps_b"].cpu().numpy().astype(np.float64))
    want = mw["kl"] + mb["kl"]
    bv = float(np.mean(mw["b_term"]) + np.mean(mb["b_term"])) + KM.U32 * abs(want)
    assert mu.grad.shape == mu.shape and layer.mu_bias.grad.shape == layer.mu_bias.shape
    gw = (flat(mu.grad).cpu().numpy(), flat(rho.grad).cpu().numpy())
    gb = (layer.mu_bias.grad.cpu().numpy(), layer.rho_bias.grad.cpu().numpy())
    worst = max(_check_grads(name + " weight", gw, mw), _check_grads(name + " bias", gb, mb))
    print("%s: kl %.6f, value err/bound %.3g, gradients %.3g" % (name, float(kl), abs(float(kl) - want) / bv, worst))
    assert abs(float(kl.detach()) - want) <= bv
    # forward(return_kl=True) returns the same estimate for the sample its forward consumed
    x = torch.randn((2, layer._op.in_channels) + ((5, 5) if layer._op.nd == 2 else ()), device=_dev())
    bt.set_sample_index(layer, SAMPLE)
    with torch.no_grad():
        _, kl2 = layer(x)
    assert torch.equal(kl2, kl.detach())


def test_a_model_mixing_gaussian_and_mixture_priors_adds_the_two_paths():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import autograd as AG, layers as L
    bt.manual_seed(SEED)
    torch.manual_seed(6)
    net = torch.nn.Sequential(L.LinearReparameterization(37, 20), L.LinearFlipout(20, 6)).to(_dev())
    net[1].set_prior(_prior("mix2"), kl_samples=2)
    bt.set_sample_index(net, SAMPLE)
    total = bt.get_kl_loss(net)
    pairs = AG.kl_pairs(net[0])
    gauss = AG.KlFn.apply(tuple(m for _, _, m in pairs), *[t for mu, rho, _ in pairs for t in (mu, rho)])
    mc = net[1].kl_loss()
    assert torch.equal(total.detach(), (gauss + mc).detach())
    total.backward()
    got = [p.grad.clone() for p in net.parameters()]
    for p in net.parameters():
        p.grad = None
    (gauss + mc).backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(got, net.parameters()))


# ---- captured steps ----------------------------------------------------------------------------------------------------------------
def _capture_net(prior=True):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L, models
    bt.manual_seed(SEED)
    bt.set_precision("f32")
    torch.manual_seed(0)
    net = torch.nn.Sequential(L.Conv2dReparameterization(8, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Flatten(),
                              L.LinearReparameterization(8 * 6 * 6, 10))
    for m in net:
        if hasattr(m, "dnn_to_bnn_flag"):
            m.dnn_to_bnn_flag = True
    net = net.to(_dev()).train()
    bt.assign_layer_ids(net)
    if prior:
        models.set_prior(net, _prior("mix2", mu=0.0), kl_samples=2)
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


@pytest.mark.parametrize("num_mc", [1, 2])
def test_captured_step_is_bit_equal_to_the_eager_step(num_mc):
    """GraphedTrainStep.run(s), s = 0, 1, 2: the loss and every p.grad equal the eager step at set_sample_index(model, s) bit for bit — the
    replay's KL follows the device word (num_mc = 2: the word of the last pass, as the eager loop's last forward)"""
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = _capture_net()
    want = {s: _eager(net, x, y, s, num_mc) for s in (0, 1, 2)}
    assert not torch.equal(want[0][0], want[1][0])
    for p in net.parameters():
        p.grad = None
    gs = GraphedTrainStep(net, x, y, num_mc=num_mc)
    try:
        for s in (0, 1, 2, 0):
            loss = gs.run(s)
            torch.cuda.synchronize()
            rel = max(float((p.grad - w).norm() / w.norm().clamp_min(1e-30)) for p, w in zip(net.parameters(), want[s][1]))
            print("num_mc=%d replay at %d: loss %.7f (eager %.7f), gradient rel-L2 max %.1e" % (num_mc, s, float(loss), float(want[s][0]), rel))
            assert torch.equal(loss, want[s][0])
            assert all(torch.equal(p.grad, w) for p, w in zip(net.parameters(), want[s][1]))
    finally:
        gs.close()


def test_captured_step_with_sgd_inside_the_graph():
    """optimizer=optim.SGD: three replays leave the loss of every step and the parameters bit-equal to three eager steps + optim.SGD"""
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = _capture_net()
    params = list(net.parameters())
    start = [p.detach().clone() for p in params]
    opt_e = optim.SGD(params, lr=0.05)
    losses = []
    for s in (0, 1, 2):
        losses.append(_eager(net, x, y, s, 1)[0])
        opt_e.step()
    eager = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, s0 in zip(params, start):
            p.copy_(s0)
            p.grad = None
    gs = GraphedTrainStep(net, x, y, optimizer=optim.SGD(params, lr=0.05))
    try:
        for s in (0, 1, 2):
            loss = gs.run(s).clone()
            torch.cuda.synchronize()
            print("captured SGD step %d: loss %.7f (eager %.7f)" % (s, float(loss), float(losses[s])))
            assert torch.equal(loss, losses[s])
        assert all(torch.equal(p.detach(), e) for p, e in zip(params, eager))
    finally:
        gs.close()


def test_gaussian_prior_copy_keeps_the_klfn_path():
    """a Gaussian-prior copy of the model (set_prior(None)): get_kl_loss and its gradients are the unchanged KlFn path's, bit for bit, and
    its captured step equals its eager step as before"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import autograd as AG, models
    net, x, y = _capture_net()
    plain = models.set_prior(copy.deepcopy(net), None)
    assert all(m._btx_prior is None for m in plain if hasattr(m, "set_prior"))
    layers = [m for m in plain if hasattr(m, "kl_loss")]
    pairs = [pr for layer in layers for pr in AG.kl_pairs(layer)]
    want = AG.KlFn.apply(tuple(m for _, _, m in pairs), *[t for mu, rho, _ in pairs for t in (mu, rho)])
    want.backward()
    ref = [p.grad.clone() for p in plain.parameters()]
    for p in plain.parameters():
        p.grad = None
    got = bt.get_kl_loss(plain)
    got.backward()
    assert torch.equal(got.detach(), want.detach()) and all(torch.equal(p.grad, r) for p, r in zip(plain.parameters(), ref))
    never, _, _ = _capture_net(prior=False)
    with torch.no_grad():
        for a, b in zip(never.parameters(), plain.parameters()):
            a.copy_(b)
    assert torch.equal(bt.get_kl_loss(never).detach(), got.detach())
