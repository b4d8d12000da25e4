"""num_mc > 1 training on the CPU: the ATen chains of utils/mc_loss.py and the type=1 AvUC losses against torch's own cross-entropy
and the numpy mutual information, the eager multi-sample forward with its documented sample indices, and the host-side argument
checks of the new C-ABI entries.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bayesian_torch_amd as bt
from bayesian_torch_amd import autograd as AG
from bayesian_torch_amd import rng as R
from bayesian_torch_amd._lib import BtxError
from bayesian_torch_amd.utils import _calibration as C
from bayesian_torch_amd.utils import avuc_loss as A
from bayesian_torch_amd.utils import mc_loss as M

import mc_loss_cases as K

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def small_model(kind="Flipout"):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1, bias=False), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
                              torch.nn.Flatten(), torch.nn.Linear(8 * 8 * 8, 10))
    bt.dnn_to_bnn(net, dict(PRIOR, type=kind))
    bt.assign_layer_ids(net)
    return net.train()


@pytest.mark.parametrize("name", list(K.CE_CASES))
@pytest.mark.parametrize("ls", K.SMOOTHING)
def test_chain_equals_the_reference_loop(name, ls):
    """reference examples/main_bayesian_cifar.py:363-372: CE(mean(stack(outputs)), y) + kl / bs; reduce="loss": the mean of the
    per-sample cross-entropies"""
    c = K.ce_case(name)
    st, y = torch.from_numpy(c["stack"]).double(), torch.from_numpy(c["labels"])
    B = st.shape[1]
    kl = torch.tensor(K.KL, dtype=torch.float64)
    want = F.cross_entropy(st.mean(0), y, label_smoothing=ls) + kl / B
    got = M._mc_ce_chain(st, y, kl, "logits", ls)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    want = torch.stack([F.cross_entropy(s, y, label_smoothing=ls) for s in st]).mean() + kl / B
    got = M._mc_ce_chain(st, y, kl, "loss", ls)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    # the public faces route CPU tensors to the chain
    assert torch.equal(M.mc_elbo_loss(st, y, kl, "loss", ls), got)
    assert torch.equal(M.MCCrossEntropy("loss", ls)(st, y, kl), got)
    assert float(M.mc_elbo_loss(st, y, reduce="loss", label_smoothing=ls)) == pytest.approx(float(got) - K.KL / B, abs=1e-9)


@pytest.mark.parametrize("reduce", K.REDUCES)
def test_one_sample_stack_equals_the_2d_loss_and_gradient(reduce):
    c = K.s1_case()
    y = torch.from_numpy(c["labels"])
    z2 = torch.from_numpy(c["stack"][0]).double().requires_grad_(True)
    want = F.cross_entropy(z2, y, label_smoothing=0.1)
    want.backward()
    st = torch.from_numpy(c["stack"]).double().requires_grad_(True)
    got = M.mc_elbo_loss(st, y, reduce=reduce, label_smoothing=0.1)
    got.backward()
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-12
    assert float((st.grad[0] - z2.grad).abs().max()) <= 1e-14


def _np_mi(p, eps):
    ent = lambda q: -1 * np.sum(q * np.log(q + eps), axis=-1)  # noqa: E731
    return ent(np.mean(p, axis=0)) - np.mean(ent(p), axis=0)


@pytest.mark.parametrize("name", list(K.AVU_CASES))
def test_uncertainty_is_the_mutual_information(name):
    c = K.avu_case(name)
    st = torch.from_numpy(c["stack"]).double()
    conf, pred, unc = C.mc_row_stats(st)
    p = torch.softmax(st, 2).numpy()
    # the numpy helper of avuc_loss.py carries epsilon 1e-15, the loss module 1e-10: exact against the helper's formula at 1e-10 ...
    assert np.abs(unc.numpy() - _np_mi(p, 1e-10)).max() <= 1e-12
    # ... and against the helper itself up to the epsilons: |p log(p + 1e-10) - p log(p + 1e-15)| <= 1e-10 per class, two entropies
    assert np.array_equal(A.mutual_information(p), _np_mi(p, 1e-15))
    assert np.abs(unc.numpy() - A.mutual_information(p)).max() <= 2 * st.shape[2] * 1e-10 + 1e-12
    pbar = p.mean(0)
    assert np.array_equal(pred.numpy(), pbar.argmax(1)) and np.abs(conf.numpy() - pbar.max(1)).max() <= 1e-15


@pytest.mark.parametrize("name", list(K.AVU_CASES))
def test_avu_case_margins_hold(name):
    K.assert_avu_margin(name, False)
    if name in K.AVU_AREA_CASES:
        K.assert_avu_margin(name, True)


def test_every_sample_gets_gradient_through_the_soft_weights():
    c = K.avu_case("s5_b37_c257_x8")
    for area in (False, True):
        loss, _, g = K.avu_run(c, c["th"], area, torch.float64)
        assert np.isfinite(loss) and all(np.abs(g[s]).max() > 0 for s in range(g.shape[0]))
    # the modules route 3-D CPU stacks to the chain
    st, y = torch.from_numpy(c["stack"]).double(), torch.from_numpy(c["labels"])
    assert float(A.AvULoss(beta=K.BETA)(st, y, c["th"], type=1)) == K.avu_run(c, c["th"], False, torch.float64)[0]
    la, auc = A.AUAvULoss(beta=K.BETA)(st, y, type=1)
    assert (float(la), float(auc)) == K.avu_run(c, c["th"], True, torch.float64)[:2]
    assert float(A.AvULoss(beta=K.BETA)(st, y, torch.tensor(c["th"]), type=1)) == float(A.AvULoss(beta=K.BETA)(st, y, c["th"], type=1))


def test_identical_samples_have_no_model_uncertainty():
    """a stack of S copies: MI = 0, and type=1 shares only confidence and prediction with type=0 (whose uncertainty is the entropy)"""
    c = K.s1_case()
    z = torch.from_numpy(c["stack"][0]).double()
    st = z.unsqueeze(0).repeat(4, 1, 1)
    conf, pred, unc = C.mc_row_stats(st)
    conf0, pred0, ent0 = C.row_stats(z)
    assert float(unc.abs().max()) <= 1e-15
    assert torch.equal(pred, pred0) and float((conf - conf0).abs().max()) <= 1e-15
    assert float(ent0.min()) > 1e-6  # type=0 would see uncertainty here


def test_one_sample_is_degenerate_every_example_certain():
    c = K.s1_case()
    st, y = torch.from_numpy(c["stack"]).double(), torch.from_numpy(c["labels"])
    conf, pred, unc = C.mc_row_stats(st)
    assert float(unc.abs().max()) == 0.0
    good = pred == y
    w = torch.where(good, conf, 1 - conf)
    want = -K.BETA * torch.log(w[good].sum() / (w.sum() + 1e-10) + 1e-10)  # n_au = n_iu = 0, tanh(0) = 0
    for th in (0.0, 0.5):
        got = A.AvULoss(beta=K.BETA)(st, y, th, type=1)
        assert abs(float(got) - float(want)) <= 1e-12


def test_argument_errors_and_fallbacks():
    c = K.avu_case("s2_b3_c10_x8")
    st, y = torch.from_numpy(c["stack"]), torch.from_numpy(c["labels"])
    with pytest.raises(ValueError, match="type=1"):
        A.AvULoss()(st[0], y, 0.5, type=1)
    with pytest.raises(ValueError, match="type=1"):
        A.AUAvULoss()(st[0], y, type=1)
    with pytest.raises(ValueError, match="batch, classes"):
        A.AvULoss()(st, y, 0.5, type=0)
    with pytest.raises(ValueError, match="batch, classes"):
        A.AUAvULoss()(st, y)
    with pytest.raises(ValueError, match="labels"):
        A.AvULoss()(st, y[:2], 0.5, type=1)
    with pytest.raises(ValueError, match="type"):
        A.AvULoss()(st, y, 0.5, type=2)
    with pytest.raises(ValueError, match="type"):
        A.AUAvULoss()(st, y, type=2)
    with pytest.raises(ValueError, match="target"):
        M.mc_elbo_loss(st, y[:2])
    with pytest.raises(ValueError, match="S, batch, classes"):
        M.mc_elbo_loss(st[0], y)
    with pytest.raises(ValueError, match="reduce"):
        M.mc_elbo_loss(st, y, reduce="mean")
    with pytest.raises(ValueError, match="reduce"):
        M.MCCrossEntropy(reduce="mean")
    with pytest.raises(ValueError, match="label_smoothing"):
        M.mc_elbo_loss(st, y, label_smoothing=1.0)
    # more samples than the kernels take: the chain, still correct
    big = st.double().repeat(17, 1, 1)  # S = 34
    assert big.shape[0] > M.MAX_SAMPLES
    want = F.cross_entropy(big.mean(0), y)
    assert abs(float(M.mc_elbo_loss(big, y)) - float(want)) <= 1e-12
    loss = A.AvULoss(beta=2.0)(big, y, c["th"], type=1)
    assert loss.shape == (1,) and torch.isfinite(loss).all()
    assert float(loss) == float(C.avu_mc_chain(big, y, c["th"], 2.0, False)[0])


def test_public_names():
    from bayesian_torch_amd import utils
    assert utils.MCCrossEntropy is M.MCCrossEntropy and utils.mc_elbo_loss is M.mc_elbo_loss and utils.mc_loss is M


def _manual_pass(net, x, idx):
    R.set_sample_index(net, idx)
    with torch.random.fork_rng(devices=[]):
        torch.default_generator.manual_seed(R.cpu_sample_seed(idx))
        return net(x)


def test_eager_loop_on_cpu_uses_the_documented_indices():
    net = small_model()
    torch.manual_seed(1)
    x = torch.randn(4, 3, 8, 8)
    y = torch.randint(0, 10, (4,))
    nbt0 = int(net[1].num_batches_tracked)
    stack = AG.mc_train_forward(net, x, 3, step=4)
    assert stack.shape == (3, 4, 10) and stack.requires_grad
    assert int(net[1].num_batches_tracked) == nbt0 + 3  # training BatchNorm sees num_mc forwards per step
    for k in range(3):
        assert torch.equal(stack[k].detach(), _manual_pass(net, x, 4 * 3 + k).detach())
    assert not torch.equal(stack[0], stack[1])
    loss = M.mc_elbo_loss(stack, y, kl=bt.get_kl_loss(net))
    loss.backward()
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert float(p.grad.abs().max()) > 0, n
    # the index wraps at 31 bits, as the device words do
    big = AG.mc_train_forward(net, x, 2, step=2 ** 30)
    assert torch.equal(big[0].detach(), _manual_pass(net, x, 0).detach())
    with pytest.raises(ValueError):
        AG.mc_train_forward(net, x, 0, step=0)


def test_eager_loop_refuses_a_live_device_sample_word():
    """a captured step / GraphedMC left on the model keeps the index in one device word: every eager pass would rewrite it and every
    backward would regenerate the last pass's noise"""
    net = small_model()
    word = torch.zeros(1, dtype=torch.int32)
    net[0].__dict__["_btx_sample_dev"] = word
    with pytest.raises(BtxError, match="device word"):
        AG.mc_train_forward(net, torch.randn(4, 3, 8, 8), 2, step=0)
    net[0].__dict__["_btx_sample_dev"] = None
    assert AG.mc_train_forward(net, torch.randn(4, 3, 8, 8), 2, step=0).shape == (2, 4, 10)


def test_eager_loop_refuses_lstm_models():
    class Seq(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = torch.nn.LSTM(6, 8)
            self.fc = torch.nn.Linear(8, 3)

        def forward(self, x):
            out, _ = self.lstm(x)
            return self.fc(out[:, -1, :])
    net = Seq()
    bt.dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    with pytest.raises(BtxError, match="lstm"):
        AG.mc_train_forward(net.train(), torch.randn(2, 5, 6), 2, step=0)


def test_cabi_mcloss_entry_points_without_gpu():
    """host-side argument validation: every call returns before anything is launched"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9  # additive: the ABI number does not move
    for n in ("btx_mcloss_workspace_bytes", "btx_mc_ce_fwd", "btx_mc_ce_bwd", "btx_avu_mc_fwd", "btx_avu_mc_bwd"):
        assert n in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.lib_path()), n)
    sizes = [L.btx_mcloss_workspace_bytes(s, b) for s, b in ((0, 0), (1, 1), (1, 7), (5, 7), (5, 64), (32, 1500))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and all(s % 8 == 0 for s in sizes)
    one, big = ctypes.c_void_p(256), sizes[-1]
    ce = L.btx_mc_ce_fwd
    assert ce(None, one, 2, 4, 10, 0, 0, 0.0, None, 0.25, one, one, big, None) == -1
    assert ce(one, None, 2, 4, 10, 0, 0, 0.0, None, 0.25, one, one, big, None) == -1
    assert ce(one, one, 2, 4, 10, 0, 0, 0.0, None, 0.25, None, one, big, None) == -1
    assert ce(one, one, 2, 4, 10, 0, 0, 0.0, None, 0.25, one, None, big, None) == -1
    assert ce(one, one, 0, 4, 10, 0, 0, 0.0, None, 0.25, one, one, big, None) == -2
    assert ce(one, one, 33, 4, 10, 0, 0, 0.0, None, 0.25, one, one, big, None) == -2
    assert ce(one, one, 2, 0, 10, 0, 0, 0.0, None, 0.25, one, one, big, None) == -2
    assert ce(one, one, 2, 4, 0, 0, 0, 0.0, None, 0.25, one, one, big, None) == -2
    assert ce(one, one, 2, 4, 24576, 0, 0, 0.0, None, 0.25, one, one, big, None) == -3
    assert ce(one, one, 2, 4, 10, 0, 2, 0.0, None, 0.25, one, one, big, None) == -2
    assert ce(one, one, 2, 4, 10, 0, 0, 1.0, None, 0.25, one, one, big, None) == -2
    assert ce(one, one, 2, 4, 10, 7, 0, 0.0, None, 0.25, one, one, big, None) == -5
    assert ce(one, one, 2, 4, 10, 0, 0, 0.0, None, 0.25, one, one, 16, None) == -4
    cb = L.btx_mc_ce_bwd
    assert cb(None, one, 2, 4, 10, 0, 0, 0.0, 0.25, one, one, big, one, None) == -1
    assert cb(one, one, 2, 4, 10, 0, 0, 0.0, 0.25, None, one, big, one, None) == -1
    assert cb(one, one, 2, 4, 10, 0, 0, 0.0, 0.25, one, one, big, None, None) == -1
    assert cb(one, one, 0, 4, 10, 0, 0, 0.0, 0.25, one, one, big, one, None) == -2
    assert cb(one, one, 33, 4, 10, 0, 0, 0.0, 0.25, one, one, big, one, None) == -2
    assert cb(one, one, 2, 4, 10, 0, 0, 0.0, 0.25, one, one, 16, one, None) == -4
    af = L.btx_avu_mc_fwd
    assert af(None, one, 2, 4, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -1
    assert af(one, None, 2, 4, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -1
    assert af(one, one, 2, 4, 10, 0, 0, 0.5, None, 1.0, None, one, big, None) == -1
    assert af(one, one, 2, 4, 10, 0, 0, 0.5, None, 1.0, one, None, big, None) == -1
    assert af(one, one, 0, 4, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -2
    assert af(one, one, 33, 4, 10, 0, 0, 0.5, None, 1.0, one, one, big, None) == -2
    assert af(one, one, 2, 4, 10, 0, 2, 0.5, None, 1.0, one, one, big, None) == -2
    assert af(one, one, 2, 4, 10, 7, 0, 0.5, None, 1.0, one, one, big, None) == -5
    assert af(one, one, 2, 4, 10, 0, 0, 0.5, None, 1.0, one, one, 16, None) == -4
    assert af(one, one, 2, 4, C.AVU_MC_MAX_CLASSES + 1, 0, 0, 0.5, None, 1.0, one, one, big, None) == -3  # the backward's LDS row
    ab = L.btx_avu_mc_bwd
    assert ab(None, 2, 4, 10, 0, one, None, one, big, one, None) == -1
    assert ab(one, 2, 4, 10, 0, None, None, one, big, one, None) == -1
    assert ab(one, 0, 4, 10, 0, one, None, one, big, one, None) == -2
    assert ab(one, 33, 4, 10, 0, one, None, one, big, one, None) == -2
    assert ab(one, 2, 4, 10, 0, one, None, one, 16, one, None) == -4
    assert ab(one, 2, 4, C.AVU_MC_MAX_CLASSES + 1, 0, one, None, one, big, one, None) == -3
