"""AvUC / EaU / EaC calibration losses on the GPU: the HIP path (btx_avu_fwd / btx_avu_bwd / btx_eau_fwd / btx_eau_bwd) against
the vectorised ATen chain evaluated on the CPU in float64 on the same inputs (tests/golden/avuc.npz).

Tolerance (loss relative error, gradient rel-L2, gradient max-abs over max): max(8 * e_cpu32, 32 * 2^-24), where e_cpu32 is the
same error of the float32 CPU chain against float64 on that case — 8 for a second, independent f32 implementation with other
transcendental and summation orders; the floor is a handful of ulps of expf / logf / tanhf plus two reduction trees.  Every case
first re-asserts its margins (no example within 1e-3 of a threshold — 1e-4 at B = 1500 —, top-2 probability gap > 1e-3) from the
float64 chain: without them a one-ulp difference in an entropy would move an example across a threshold."""
import numpy as np
import pytest
import torch

from avuc_cases import (AREA_NAMES, AVU_NAMES, EAU_NAMES, assert_avu_margin, assert_eau_margin, avu_truth, eau_truth, load,
                        max_over_max, rel, rel_l2)

pytestmark = pytest.mark.gpu

FLOOR = 32 * 2.0 ** -24
BF16_GRAD_TOL = 2.0 ** -8  # one rounding to bf16 is <= 2^-9 per element


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tol(e):
    return max(8 * e, FLOOR)


def _mods():
    from bayesian_torch_amd.utils import avuc_loss as A
    from bayesian_torch_amd.utils import uncertainty_calibration_loss as U
    return A, U


def _gpu_avu(c, area, dtype=torch.float32, module="A", th=None):
    A, U = _mods()
    lg = torch.from_numpy(c["logits"]).to(_dev()).to(dtype).requires_grad_(True)
    lb = torch.from_numpy(c["labels"]).to(_dev())
    th = float(c["th"]) if th is None else th
    if area:
        loss, r = A.AUAvULoss(beta=float(c["beta"]))(lg, lb)
    elif module == "A":
        loss, r = A.AvULoss(beta=float(c["beta"]))(lg, lb, th), None
    else:
        loss, r = U.AvULoss(beta=float(c["beta"]))(lg, lb, th), None
    loss.sum().backward()
    return loss.detach(), (None if r is None else r.detach()), lg.grad.detach()


def _check(tag, t, loss, grad, bf16=False):
    e_loss, e_l2, e_max = rel(loss.cpu(), t["loss"]), rel_l2(grad.float().cpu().numpy(), t["grad"]), \
        max_over_max(grad.float().cpu().numpy(), t["grad"])
    print("%-28s loss rel %.2e (cpu32 %.2e)  grad rel-L2 %.2e (cpu32 %.2e)  grad max/max %.2e (cpu32 %.2e)" % (
        tag, e_loss, t["e32_loss"], e_l2, t["e32_l2"], e_max, t["e32_max"]))
    assert e_loss <= _tol(t["e32_loss"]), (tag, e_loss)
    if bf16:
        assert e_l2 <= BF16_GRAD_TOL, (tag, e_l2)
    else:
        assert e_l2 <= _tol(t["e32_l2"]), (tag, e_l2)
        assert e_max <= _tol(t["e32_max"]), (tag, e_max)


@pytest.mark.parametrize("name", AVU_NAMES)
def test_avuloss_hip_matches_float64_chain(name):
    c = load()["avu"][name]
    assert_avu_margin(name, False)
    t = avu_truth(name, False)
    loss, _, grad = _gpu_avu(c, False)
    assert loss.shape == (1,) and loss.dtype == torch.float32 and grad.dtype == torch.float32
    if t["loss"] == 0.0 or abs(t["loss"]) < 1e-9:  # B = 1: AvU = 1, the loss is -log(1 + 1e-10) and its gradient vanishes
        assert abs(float(loss)) <= 1e-7 and float(grad.abs().max()) <= 1e-7
        return
    _check("AvULoss " + name, t, loss, grad)


def test_uncertainty_calibration_avuloss_hip_is_the_same_kernel():
    c = load()["avu"]["b37_c257"]
    la, _, ga = _gpu_avu(c, False, module="A")
    lu, _, gu = _gpu_avu(c, False, module="U")
    assert lu.shape == () and torch.equal(lu.reshape(1), la) and torch.equal(ga, gu)


@pytest.mark.parametrize("name", AREA_NAMES)
def test_auavuloss_hip_matches_float64_chain(name):
    c = load()["avu"][name]
    assert_avu_margin(name, True)
    t = avu_truth(name, True)
    loss, auc, grad = _gpu_avu(c, True)
    assert loss.shape == (1,) and auc.shape == (1,)
    _check("AUAvULoss " + name, t, loss, grad)
    assert rel(auc.cpu(), t["r"]) <= _tol(t["e32_loss"])
    print("%-28s auc %.8f, reference auc_avu() %.8f" % ("", float(auc), float(c["ref_auc"])))


def test_auavuloss_second_output_carries_gradient():
    """d auc / d logits through the g_r input of btx_avu_bwd, alone and together with the loss"""
    from bayesian_torch_amd.utils import _calibration as C
    A, _ = _mods()
    c = load()["avu"]["b37_c257"]
    assert_avu_margin("b37_c257", True)
    lb = torch.from_numpy(c["labels"])
    truth = {}
    for dt in (torch.float64, torch.float32):
        lg = torch.from_numpy(c["logits"]).to(dt).requires_grad_(True)
        loss, r = C.avu_chain(lg, lb, None, 2.0, True)
        g_r, = torch.autograd.grad(r.sum(), lg, retain_graph=True)
        g_both, = torch.autograd.grad((loss + 3 * r).sum(), lg)
        truth[dt] = (g_r.numpy(), g_both.numpy())
    lg = torch.from_numpy(c["logits"]).to(_dev()).requires_grad_(True)
    loss, r = A.AUAvULoss(beta=2.0)(lg, lb.to(_dev()))
    g_r, = torch.autograd.grad(r.sum(), lg, retain_graph=True)
    g_both, = torch.autograd.grad((loss + 3 * r).sum(), lg)
    for k, g in enumerate((g_r, g_both)):
        e32 = rel_l2(truth[torch.float32][k], truth[torch.float64][k])
        e = rel_l2(g.cpu().numpy(), truth[torch.float64][k])
        print("auc gradient %d: rel-L2 %.2e (cpu32 %.2e)" % (k, e, e32))
        assert e <= _tol(e32)


@pytest.mark.parametrize("name", EAU_NAMES)
@pytest.mark.parametrize("form", ["eau", "eac"])
def test_eau_eac_hip_match_float64_chain(name, form):
    _, U = _mods()
    c = load()["eau"][name]
    assert_eau_margin(name)
    conf_form = form == "eac"
    t = eau_truth(name, conf_form)
    e = torch.from_numpy(c["error"]).to(_dev()).requires_grad_(True)
    o = torch.from_numpy(c["conf" if conf_form else "unc"]).to(_dev()).requires_grad_(True)
    mod = (U.EaCLoss if conf_form else U.EaULoss)(beta=float(c["beta"]))
    loss = mod(e, o, float(c["error_th"]), float(c["conf_th" if conf_form else "unc_th"]))
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    g = np.concatenate([e.grad.cpu().numpy(), o.grad.cpu().numpy()])
    t = dict(t, grad=np.concatenate([t["derror"], t["dother"]]))
    _check("%s %s" % (form, name), t, loss.detach(), torch.from_numpy(g))
    # column vectors are flattened, and a gradient for one input only is enough
    e2 = torch.from_numpy(c["error"]).to(_dev())[:, None].requires_grad_(True)
    loss2 = mod(e2, o.detach()[:, None], float(c["error_th"]), float(c["conf_th" if conf_form else "unc_th"]))
    loss2.backward()
    assert torch.equal(loss2, loss.detach()) and torch.equal(e2.grad.reshape(-1), e.grad)


@pytest.mark.parametrize("name", ["bf16_b7_c10", "bf16_b37_c257"])
@pytest.mark.parametrize("area", [False, True], ids=["avu", "area"])
def test_bf16_logits(name, area):
    """bf16 logits (exact in the fixture): the loss is computed in f32 from them, dlogits comes back in bf16"""
    c = load()["avu"][name]
    assert np.array_equal(torch.from_numpy(c["logits"]).bfloat16().float().numpy(), c["logits"])
    assert_avu_margin(name, area)
    t = avu_truth(name, area)
    loss, _, grad = _gpu_avu(c, area, dtype=torch.bfloat16)
    assert loss.dtype == torch.float32 and grad.dtype == torch.bfloat16
    _check("bf16 %s %s" % ("AUAvULoss" if area else "AvULoss", name), t, loss, grad, bf16=True)


@pytest.mark.parametrize("name", ["b1500_c10", "b64_c1000"])
def test_two_runs_give_identical_bits(name):
    c = load()["avu"][name]
    for area in (False, True):
        a, b = _gpu_avu(c, area), _gpu_avu(c, area)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        if area:
            assert torch.equal(a[1], b[1])


def _second_threshold(c):
    """another threshold with the margin that moves at least one example to the other side"""
    from bayesian_torch_amd.utils import _calibration as C
    ent = np.sort(C.row_stats(torch.from_numpy(c["logits"]).double())[2].numpy())
    for j in range(len(ent) - 1):
        th2 = float(np.float32(0.5 * (ent[j] + ent[j + 1])))
        if np.abs(ent - th2).min() > 1e-3 and (ent <= th2).sum() != (ent <= float(c["th"])).sum():
            return th2
    raise AssertionError("no second threshold")


def test_device_threshold_and_graph_replay_follow_the_threshold():
    A, _ = _mods()
    c = load()["avu"]["b37_c257"]
    dev = _dev()
    th1, th2 = float(c["th"]), _second_threshold(c)
    l1, _, g1 = _gpu_avu(c, False, th=th1)
    l2, _, g2 = _gpu_avu(c, False, th=th2)
    assert not torch.equal(l1, l2)
    ld, _, gd = _gpu_avu(c, False, th=torch.tensor(th1, device=dev))
    assert torch.equal(ld, l1) and torch.equal(gd, g1)
    # forward + backward captured once; the threshold word is rewritten between replays
    th = torch.tensor(th1, device=dev)
    lg = torch.from_numpy(c["logits"]).to(dev).requires_grad_(True)
    lb = torch.from_numpy(c["labels"]).to(dev)
    mod = A.AvULoss(beta=float(c["beta"]))

    def step():
        lg.grad = None
        loss = mod(lg, lb, th)
        loss.sum().backward()
        return loss.detach()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    lg.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss = step()
    grad = lg.grad
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(loss, l1) and torch.equal(grad, g1)
    th.fill_(th2)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(loss, l2) and torch.equal(grad, g2)


@pytest.mark.parametrize("form", ["avu", "area"])
def test_graphed_train_step_with_the_calibration_term(form):
    """autograd.GraphedTrainStep with loss_fn = ce + kl / bs + AvU term: the replay equals the eager step at the same sample"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.utils import _calibration as C
    A, _ = _mods()
    dev = _dev()
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 10))
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=False, moped_delta=0.5))
    m = m.to(dev).train()
    bt.assign_layer_ids(m)
    bs = 37
    x = torch.randn(bs, 16, device=dev) * 2
    y = torch.randint(0, 10, (bs,), device=dev)
    S = 5
    with torch.no_grad():  # a threshold in the widest gap of this batch's entropies at sample S
        bt.set_sample_index(m, S)
        ent = np.sort(C.row_stats(m(x).double())[2].cpu().numpy())
    j = int(np.argmax(ent[bs // 4 + 1:3 * bs // 4 + 1] - ent[bs // 4:3 * bs // 4])) + bs // 4
    th = float(np.float32(0.5 * (ent[j] + ent[j + 1])))
    assert np.abs(ent - th).min() > 1e-4
    avu, area = A.AvULoss(beta=3.0), A.AUAvULoss(beta=3.0)

    def loss_fn(out, tgt):
        base = torch.nn.functional.cross_entropy(out.float(), tgt) + bt.get_kl_loss(m) / bs
        return base + (avu(out, tgt, th) if form == "avu" else area(out, tgt)[0]).sum()

    def eager(with_term):
        for p_ in m.parameters():
            p_.grad = None
        bt.set_sample_index(m, S)
        out = m(x)
        loss = loss_fn(out, y) if with_term else torch.nn.functional.cross_entropy(out.float(), y) + bt.get_kl_loss(m) / bs
        loss.backward()
        return float(loss), [p_.grad.detach().clone() for p_ in m.parameters()]
    l0, g0 = eager(False)
    le, ge = eager(True)
    assert abs(le - l0) > 1e-3 and rel_l2(ge[0].cpu().numpy(), g0[0].cpu().numpy()) > 1e-3  # the term is in the step
    step = GraphedTrainStep(m, x, y, loss_fn=loss_fn)
    try:
        lr = float(step.run(S))
        torch.cuda.synchronize(dev)
        gr = [p_.grad.detach().clone() for p_ in m.parameters()]
    finally:
        step.close()
    errs = [rel_l2(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(gr, ge)]
    print("GraphedTrainStep %s: loss %.7f eager %.7f, gradient rel-L2 %s" % (form, lr, le, ", ".join("%.1e" % e for e in errs)))
    assert rel(lr, le) <= FLOOR
    assert max(errs) <= FLOOR, errs


def test_wide_rows_take_the_aten_chain_on_the_device(monkeypatch):
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.utils import _calibration as C
    A, _ = _mods()
    B, Cw = 3, mc.MC_MAX_CLASSES + 1
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, Cw, generator=g) * 4
    labels = logits.argmax(1)
    labels[1] = 0
    ent = C.row_stats(logits.double())[2]
    th = float(np.float32(0.5 * (ent.sort().values[0] + ent.sort().values[1])))
    assert float((ent - th).abs().min()) > 1e-3

    def hip_must_not_run(*a, **k):
        raise AssertionError("rows wider than MC_MAX_CLASSES must not reach the HIP path")
    monkeypatch.setattr(C.AvuFn, "apply", hip_must_not_run)
    lc = logits.clone().requires_grad_(True)
    loss_c = A.AvULoss()(lc, labels, th)
    loss_c.backward()
    lgpu = logits.to(_dev()).requires_grad_(True)
    loss_g = A.AvULoss()(lgpu, labels.to(_dev()), th)
    loss_g.backward()
    # the same f32 ATen chain on two devices: only the order of the 24 576-term sums differs (~sqrt(C) * 2^-24 = 1e-5)
    assert loss_g.is_cuda and rel(loss_g.detach().cpu(), loss_c.detach()) <= 1e-5
    assert rel_l2(lgpu.grad.cpu().numpy(), lc.grad.numpy()) <= 1e-5
