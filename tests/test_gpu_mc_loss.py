"""num_mc > 1 training on the GPU: the HIP loss heads of csrc/btx_mcloss.hip (btx_mc_ce_* behind utils.mc_loss, btx_avu_mc_* behind the
type=1 AvUC losses) against the float64 ATen chains evaluated on the CPU on the same inputs (tests/mc_loss_cases.py), and the sample
plumbing: autograd.mc_train_forward and GraphedTrainStep(num_mc=...) against single forwards / eager steps at the documented indices.

Head tolerance — the rule of tests/test_gpu_avuc.py, not a new number: max(8 * e_cpu32, 32 * 2^-24) on the loss relative error, the
gradient rel-L2 and the gradient max-abs over max, e_cpu32 being the same error of the float32 CPU chain on that case; bf16 logits:
gradient rel-L2 <= 2^-8 (one rounding to bf16).  Captured against eager gradients / parameters: rel-L2 < 1e-5 per tensor, the
criterion tests/test_gpu_optim.py and tests/test_gpu_backward.py use for a captured against an eager step.  Eager forwards are compared bit for bit:
the forward kernels have a fixed summation order (the test first asserts that a repeated single forward is bit-equal)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mc_loss_cases as K
from mc_loss_cases import max_over_max, rel, rel_l2

pytestmark = pytest.mark.gpu

FLOOR = 32 * 2.0 ** -24
BF16_GRAD_TOL = 2.0 ** -8  # one rounding to bf16 is <= 2^-9 per element
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tol(e):
    return max(8 * e, FLOOR)


def _mods():
    from bayesian_torch_amd.utils import _calibration as C
    from bayesian_torch_amd.utils import avuc_loss as A
    from bayesian_torch_amd.utils import mc_loss as M
    return A, C, M


def _check(tag, t, loss, grad, bf16=False):
    g = grad.float().cpu().numpy()
    e_loss, e_l2, e_max = rel(loss.cpu(), t["loss"]), rel_l2(g, t["grad"]), max_over_max(g, t["grad"])
    print("%-44s loss rel %.2e (cpu32 %.2e)  grad rel-L2 %.2e (cpu32 %.2e)  grad max/max %.2e (cpu32 %.2e)" % (
        tag, e_loss, t["e32_loss"], e_l2, t["e32_l2"], e_max, t["e32_max"]))
    assert e_loss <= _tol(t["e32_loss"]), (tag, e_loss)
    if bf16:
        assert e_l2 <= BF16_GRAD_TOL, (tag, e_l2)
    else:
        assert e_l2 <= _tol(t["e32_l2"]), (tag, e_l2)
        assert e_max <= _tol(t["e32_max"]), (tag, e_max)


def _gpu_ce(c, name, reduce, ls, kl=K.KL, scale=1.0):
    A, C, M = _mods()
    st, y = K.to_device(c, _dev(), K.torch_dtype(name))
    st = st.requires_grad_(True)
    k = torch.tensor([kl], device=_dev(), requires_grad=True)
    loss = M.mc_elbo_loss(st, y, k, reduce, ls)
    assert loss.shape == () and loss.dtype == torch.float32
    assert isinstance(loss.grad_fn, M.McCeFn._backward_cls)  # the HIP head, not the chain
    (scale * loss).backward()
    return loss.detach(), st.grad.detach(), k.grad.detach()


def _gpu_avu(c, name, area, th=None, scale=1.0):
    A, C, M = _mods()
    st, y = K.to_device(c, _dev(), K.torch_dtype(name))
    st = st.requires_grad_(True)
    if area:
        loss, r = A.AUAvULoss(beta=K.BETA)(st, y, type=1)
    else:
        loss, r = A.AvULoss(beta=K.BETA)(st, y, c["th"] if th is None else th, type=1), None
    assert loss.shape == (1,) and isinstance(loss.grad_fn, C.AvuMcFn._backward_cls)
    (scale * loss.sum()).backward()
    return loss.detach(), (None if r is None else r.detach()), st.grad.detach()


# ---- heads against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", K.SMOOTHING)
@pytest.mark.parametrize("reduce", K.REDUCES)
@pytest.mark.parametrize("name", list(K.CE_CASES))
def test_mc_cross_entropy_matches_float64_chain(name, reduce, ls):
    c = K.ce_case(name)
    t = K.ce_truth(name, reduce, ls)
    loss, grad, gk = _gpu_ce(c, name, reduce, ls)
    assert grad.shape == c["stack"].shape and grad.dtype == K.torch_dtype(name)
    _check("McCe %s %s ls=%.1f" % (name, reduce, ls), t, loss, grad, bf16=name.startswith("bf16_"))
    assert float(gk) == np.float32(1.0) / np.float32(c["stack"].shape[1])  # the KL input's gradient is 1 / B


@pytest.mark.parametrize("name", list(K.AVU_CASES))
def test_avu_on_the_stack_matches_float64_chain(name):
    c = K.avu_case(name)
    K.assert_avu_margin(name, False)
    t = K.avu_truth(name, False)
    bf16 = name.startswith("bf16_")
    loss, _, grad = _gpu_avu(c, name, False)
    _check("AvULoss type=1 %s" % name, t, loss, grad, bf16=bf16)
    # the threshold as a device tensor, read by the kernel when it runs: the same launch arithmetic, the same bits
    loss_t, _, grad_t = _gpu_avu(c, name, False, th=torch.tensor([c["th"]], dtype=torch.float32, device=_dev()))
    _check("AvULoss type=1 %s (tensor th)" % name, t, loss_t, grad_t, bf16=bf16)
    assert float(np.float32(c["th"])) == c["th"]  # (the helper rounds it to f32)
    assert torch.equal(loss_t, loss) and torch.equal(grad_t, grad)


@pytest.mark.parametrize("name", K.AVU_AREA_CASES)
def test_auavu_on_the_stack_matches_float64_chain(name):
    c = K.avu_case(name)
    K.assert_avu_margin(name, True)
    t = K.avu_truth(name, True)
    loss, r, grad = _gpu_avu(c, name, True)
    _check("AUAvULoss type=1 %s" % name, t, loss, grad, bf16=name.startswith("bf16_"))
    assert rel(r.cpu(), t["r"]) <= _tol(t["e32_loss"])


def test_heads_are_bit_reproducible():
    for name in ("s5_b65_c257_x8", "bf16_s5_b3_c1001_x8_wide"):
        c = K.ce_case(name)
        for reduce in K.REDUCES:
            a, b = _gpu_ce(c, name, reduce, 0.1), _gpu_ce(c, name, reduce, 0.1)
            assert all(torch.equal(u, v) for u, v in zip(a, b)), (name, reduce)
    for name in ("s32_b65_c10_x8", "bf16_s5_b3_c1001_x8_wide"):
        c = K.avu_case(name)
        for area in (False, True):
            a, b = _gpu_avu(c, name, area), _gpu_avu(c, name, area)
            assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), (name, area)


def test_upstream_gradient_is_read_on_the_device():
    """(3 * loss).backward() gives 3 x the gradients within one f32 rounding, element by element: g_loss enters the kernels as a device
    scalar and multiplies last, so every element is fl(3 * d) with d the element of the unscaled run — as 3 * g1 is"""
    name = "s5_b65_c257_x8"
    for reduce in K.REDUCES:
        _, g1, k1 = _gpu_ce(K.ce_case(name), name, reduce, 0.1)
        _, g3, k3 = _gpu_ce(K.ce_case(name), name, reduce, 0.1, scale=3.0)
        assert float(g1.abs().max()) > 0
        assert bool(((g3 - 3 * g1).abs() <= 2.0 ** -23 * g3.abs()).all())  # one ulp of each element
        assert abs(float(k3) - 3 * float(k1)) <= 2.0 ** -23 * float(k3)
    name = "s5_b37_c257_x8"
    for area in (False, True):
        _, _, g1 = _gpu_avu(K.avu_case(name), name, area)
        _, _, g3 = _gpu_avu(K.avu_case(name), name, area, scale=3.0)
        assert float(g1.abs().max()) > 0
        assert bool(((g3 - 3 * g1).abs() <= 2.0 ** -23 * g3.abs()).all())


def test_one_sample_stack_equals_the_2d_case():
    A, C, M = _mods()
    c = K.s1_case()
    y = torch.from_numpy(c["labels"])
    B = len(y)
    for reduce in K.REDUCES:
        # float64 truth of the 2-D loss and the float32 CPU error of the same 2-D loss: the tolerance rule on the 2-D case
        def run2d(dt):
            z = torch.from_numpy(c["stack"][0]).to(dt).requires_grad_(True)
            loss = F.cross_entropy(z, y, label_smoothing=0.1) + torch.tensor(K.KL, dtype=dt) / B
            loss.backward()
            return float(loss.detach()), z.grad.numpy()[None]
        t = K._truth(run2d)
        loss, grad, _ = _gpu_ce(c, "s1", reduce, 0.1)
        _check("McCe S=1 %s vs 2-D" % reduce, t, loss, grad)
    # AvUC type=1 on one sample: the mutual information is 0, every example certain for th >= 0
    st = torch.from_numpy(c["stack"]).double()
    conf, pred, unc = C.mc_row_stats(st)
    good = pred == y
    w = torch.where(good, conf, 1 - conf)
    want = float(-K.BETA * torch.log(w[good].sum() / (w.sum() + 1e-10) + 1e-10))
    for th in (0.25, 0.0):
        loss, _, grad = _gpu_avu(c, "s1", False, th=th)
        print("AvULoss type=1, S = 1, th = %.2f: loss rel %.2e" % (th, rel(loss.cpu(), want)))
        assert rel(loss.cpu(), want) <= FLOOR
        assert torch.isfinite(grad).all()


def test_stacks_the_kernels_do_not_take_run_the_chain_on_the_device():
    A, C, M = _mods()
    c = K.ce_case("s2_b37_c10_x1")
    st, y = K.to_device(c, _dev(), torch.float32)
    big = st.repeat(17, 1, 1).requires_grad_(True)  # S = 34
    loss = M.mc_elbo_loss(big, y)
    assert not isinstance(loss.grad_fn, M.McCeFn._backward_cls)
    assert rel(loss.detach().cpu(), F.cross_entropy(big.detach().double().cpu().mean(0), y.cpu())) <= 1e-6
    half = st.half().requires_grad_(True)
    assert not isinstance(M.mc_elbo_loss(half, y).grad_fn, M.McCeFn._backward_cls)
    assert not isinstance(A.AvULoss()(big, y, 0.5, type=1).grad_fn, C.AvuMcFn._backward_cls)
    # one class more than the type=1 kernels keep in LDS: the chain, forward and backward (the cross-entropy head still takes it)
    wide = torch.randn(2, 3, C.AVU_MC_MAX_CLASSES + 1, device=_dev()).requires_grad_(True)
    yw = torch.randint(0, 10, (3,), device=_dev())
    for loss in (A.AvULoss()(wide, yw, 0.5, type=1), A.AUAvULoss()(wide, yw, type=1)[0]):
        assert not isinstance(loss.grad_fn, C.AvuMcFn._backward_cls)
        loss.sum().backward()
    assert torch.isfinite(wide.grad).all()
    assert isinstance(M.mc_elbo_loss(wide, yw).grad_fn, M.McCeFn._backward_cls)


# ---- plumbing --------------------------------------------------------------------------------------------------------
def small_model(prec):
    """Flipout conv -> BN -> ReLU -> Flipout linear, B = 4, 3 x 8 x 8, 10 classes"""
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.manual_seed(9)
    bt.set_precision(prec)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1, bias=False), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
                              torch.nn.Flatten(), torch.nn.Linear(8 * 8 * 8, 10))
    bt.dnn_to_bnn(net, dict(PRIOR, type="Flipout"))
    net = net.to(dev).train()
    bt.assign_layer_ids(net)
    torch.manual_seed(1)
    x = torch.randn(4, 3, 8, 8, device=dev)
    if prec == "bf16":
        x = x.to(torch.bfloat16)
    y = torch.randint(0, 10, (4,), device=dev)
    return net, x, y


def _bn_state(net):
    return {k: v.detach().clone() for k, v in net[1].state_dict().items() if "running" in k or "num_batches" in k}


def _restore(net, params, start, bn):
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
        for k, v in bn.items():
            getattr(net[1], k).copy_(v)


def _zero(params):
    for p in params:
        p.grad = None


@pytest.fixture
def f32_precision():
    import bayesian_torch_amd as bt
    yield
    bt.set_precision("f32")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_eager_loop_uses_the_documented_indices(prec, f32_precision):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import mc_train_forward
    net, x, y = small_model(prec)

    def single(idx):
        bt.set_sample_index(net, idx, presample=True)
        return net(x).detach()
    assert torch.equal(single(12), single(12))  # a repeated single forward is bit-equal at this shape: compare bit for bit below
    nbt = int(net[1].num_batches_tracked)
    stack = mc_train_forward(net, x, 3, step=4)
    assert stack.shape == (3, 4, 10) and stack.requires_grad and stack.dtype == x.dtype
    assert int(net[1].num_batches_tracked) == nbt + 3
    for k in range(3):
        assert torch.equal(stack[k].detach(), single(12 + k)), (prec, k)
    assert not torch.equal(stack[0], stack[1])


def _eager_step(net, x, y, n, step, loss_fn):
    from bayesian_torch_amd.autograd import mc_train_forward
    stack = mc_train_forward(net, x, n, step)
    loss = loss_fn(stack, y)
    loss.backward()
    return loss.detach().clone(), stack.detach().clone()


def test_captured_step_equals_the_eager_loop(f32_precision):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    A, C, M = _mods()
    net, x, y = small_model("f32")
    params = list(net.parameters())
    names = [n for n, _ in net.named_parameters()]
    start, bn0 = [p.detach().clone() for p in params], _bn_state(net)
    loss_fn = lambda out, tgt: M._mc_ce_chain(out, tgt, bt.get_kl_loss(net), "logits", 0.0)  # noqa: E731  (the torch chain)
    want, rm = {}, {}
    for s in (2, 5):
        _restore(net, params, start, bn0)
        _zero(params)
        _eager_step(net, x, y, 3, s, loss_fn)
        want[s] = [p.grad.detach().clone() for p in params]
        rm[s] = net[1].running_mean.detach().clone()
    _zero(params)
    gs = GraphedTrainStep(net, x, y, loss_fn=loss_fn, num_mc=3)
    try:
        for r, s in enumerate((2, 5, 2)):
            _restore(net, params, start, bn0)
            gs.run(s)
            torch.cuda.synchronize()
            errs = [float((p.grad - w).norm() / w.norm().clamp_min(1e-30)) for p, w in zip(params, want[s])]
            print("replay %d (step %d): gradient rel-L2 max %.1e (%s)" % (r, s, max(errs), names[int(np.argmax(errs))]))
            assert all(torch.isfinite(p.grad).all() for p in params)
            assert max(errs) < 1e-5, dict(zip(names, errs))
            e_rm = float((net[1].running_mean - rm[s]).norm() / rm[s].norm())
            print("          running_mean rel-L2 %.1e" % e_rm)
            assert e_rm < 1e-5
            assert int(net[1].num_batches_tracked) == int(bn0["num_batches_tracked"]) + 3
    finally:
        gs.close()


def test_captured_default_loss_and_adam_equal_two_eager_steps(f32_precision):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    A, C, M = _mods()
    net, x, y = small_model("f32")
    params = list(net.parameters())
    start, bn0 = [p.detach().clone() for p in params], _bn_state(net)
    opt_e = optim.Adam(params, lr=1e-2)
    head = lambda out, tgt: M.mc_elbo_loss(out, tgt, kl=bt.get_kl_loss(net))  # noqa: E731
    for s in (0, 1):
        _zero(params)
        loss_e, stack_e = _eager_step(net, x, y, 3, s, head)
        if s == 0:
            first = (loss_e, stack_e, float(bt.get_kl_loss(net).detach()))
        opt_e.step()
    eager = [p.detach().clone() for p in params]
    _restore(net, params, start, bn0)
    _zero(params)
    del loss_e, stack_e
    opt = optim.Adam(params, lr=1e-2)
    gs = GraphedTrainStep(net, x, y, optimizer=opt, num_mc=3)
    try:
        _restore(net, params, start, bn0)
        loss0 = gs.run(0).clone()
        gs.run(1)
        torch.cuda.synchronize()
        errs = [float((p.detach() - e).norm() / e.norm()) for p, e in zip(params, eager)]
        print("captured vs eager, two Adam steps with num_mc=3: parameter rel-L2 max %.1e" % max(errs))
        assert max(errs) < 1e-5, errs
        # the returned loss of the first replay against the float64 chain on the eager logits of that step
        st, yc = first[1].cpu(), y.cpu()
        l64 = float(M._mc_ce_chain(st.double(), yc, first[2], "logits", 0.0))
        l32 = float(M._mc_ce_chain(st, yc, np.float32(first[2]), "logits", 0.0))
        print("captured loss %.6f, chain %.6f: rel %.2e (cpu32 %.2e)" % (float(loss0), l64, rel(loss0.cpu(), l64), rel(l32, l64)))
        assert rel(loss0.cpu(), l64) <= _tol(rel(l32, l64))
        assert rel(first[0].cpu(), l64) <= _tol(rel(l32, l64))
    finally:
        gs.close()


def test_backward_regenerates_the_noise_of_its_own_pass(f32_precision):
    """two captured passes read two device words; the backward of pass 0 must regenerate the noise of word 0, not of the word the
    layer points at when backward runs (word 1).  rho's gradient is the one that carries eps."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    A, C, M = _mods()
    net, x, y = small_model("f32")
    params = list(net.parameters())
    rho = net[0].rho_kernel
    head = lambda out, tgt: M.mc_elbo_loss(out, tgt, kl=bt.get_kl_loss(net))  # noqa: E731
    step = 3
    _zero(params)
    _eager_step(net, x, y, 2, step, head)
    g_two = rho.grad.detach().clone()
    _zero(params)
    outs = []
    for _ in range(2):  # both passes on the second index
        bt.set_sample_index(net, 2 * step + 1, presample=True)
        outs.append(net(x))
    head(torch.stack(outs), y).backward()
    g_same = rho.grad.detach().clone()
    del outs
    _zero(params)
    gs = GraphedTrainStep(net, x, y, num_mc=2)
    try:
        gs.run(step)
        torch.cuda.synchronize()
        g_cap = rho.grad.detach().clone()
    finally:
        gs.close()
    e_two = float((g_cap - g_two).norm() / g_two.norm())
    e_same = float((g_cap - g_same).norm() / g_same.norm())
    print("d rho of the first layer, captured num_mc=2: vs the eager two-index loop %.1e, vs both passes on index 1 %.1e" % (e_two, e_same))
    assert e_two < 1e-5
    assert e_same > 1e-2


def test_avuc_on_mutual_information_inside_the_captured_step(f32_precision):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep, mc_train_forward
    A, C, M = _mods()
    net, x, y = small_model("f32")
    avu = A.AvULoss(beta=3)
    th_t = torch.zeros(1, device=_dev())
    loss_fn = lambda out, tgt: M.mc_elbo_loss(out, tgt, kl=bt.get_kl_loss(net)) + avu(out, tgt, th_t, type=1).sum()  # noqa: E731
    with torch.no_grad():
        stack = mc_train_forward(net, x, 3, 1)
        unc = C.mc_row_stats(stack.double().cpu())[2]
        ths = (float(unc.min()) - 0.05, float(unc.max()) + 0.05)  # every example uncertain / every example certain
        want = []
        for th in ths:
            th_t.fill_(th)
            want.append(float(loss_fn(stack, y)))
    assert abs(want[0] - want[1]) > 1e-3 * abs(want[0])
    gs = GraphedTrainStep(net, x, y, loss_fn=loss_fn, num_mc=3)
    try:
        for th, w in zip(ths, want):
            th_t.fill_(th)
            got = float(gs.run(1))
            print("captured ELBO + AvU(type=1) at th %.4f: %.6f (eager %.6f)" % (th, got, w))
            assert abs(got - w) <= 1e-5 * abs(w)
            assert all(torch.isfinite(p.grad).all() for p in net.parameters())
    finally:
        gs.close()


class SeqNet(torch.nn.Module):
    def __init__(self, i=24, h=40, classes=5):
        super().__init__()
        self.lstm1 = torch.nn.LSTM(i, h)
        self.fc = torch.nn.Linear(h, classes, bias=False)

    def forward(self, x):
        out, _ = self.lstm1(x)
        return self.fc(out[:, -1, :])


def test_lstm_models_are_refused_for_num_mc_above_one(f32_precision):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd._lib import BtxError
    from bayesian_torch_amd.autograd import GraphedTrainStep, mc_train_forward
    from bayesian_torch_amd.models import fuse_model
    dev = _dev()
    bt.manual_seed(9)
    bt.set_precision("f32")
    torch.manual_seed(0)
    net = SeqNet()
    bt.dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    net = net.to(dev).train()
    assert fuse_model(net, lstm_training=True) >= 1
    bt.assign_layer_ids(net)
    torch.manual_seed(1)
    x = torch.randn(4, 6, 24, device=dev)
    y = torch.randint(0, 5, (4,), device=dev)
    with pytest.raises(BtxError, match="lstm1"):
        GraphedTrainStep(net, x, y, num_mc=2)
    with pytest.raises(BtxError, match="lstm1"):
        mc_train_forward(net, x, 2, 0)
    # num_mc = 1 behaves as before: the captured gradients of sample 3 against the eager step
    params = list(net.parameters())
    _zero(params)
    bt.set_sample_index(net, 3)
    loss = F.cross_entropy(net(x).float(), y) + bt.get_kl_loss(net) / x.shape[0]
    loss.backward()
    want = [p.grad.detach().clone() for p in params]
    del loss
    for m in net.modules():
        if hasattr(m, "kl"):
            m.kl = None
    _zero(params)
    gs = GraphedTrainStep(net, x, y)
    try:
        assert gs.num_mc == 1 and gs.sample_dev.numel() == 1
        out = gs.run(3)
        torch.cuda.synchronize()
        assert out.dim() == 0 and math.isfinite(float(out))
        errs = [float((p.grad - w).norm() / w.norm().clamp_min(1e-30)) for p, w in zip(params, want)]
        print("LSTM model, num_mc=1: captured vs eager gradient rel-L2 max %.1e" % max(errs))
        assert max(errs) < 1e-5
    finally:
        gs.close()
