"""Fused Bayesian LSTM training (btx_lstm_fwd_train / btx_lstm_bwd) on the host: the C-ABI entry points and their argument
errors, the fused_training switch, fuse_model(lstm_training=True), and CPU tensors, which keep training through the eager loop."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

import bayesian_torch_amd as bt
from bayesian_torch_amd import _lib
from bayesian_torch_amd import layers as L
from bayesian_torch_amd.models import fuse_model

HERE = os.path.dirname(os.path.abspath(__file__))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4
NEW = ("btx_lstm_train_saved_bytes", "btx_lstm_train_workspace_bytes", "btx_lstm_fwd_train", "btx_lstm_bwd")


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(HERE, "..", "include", "btx.h")).read()
    for n in NEW:
        assert n + "(" in hdr and n in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.lib_path()), n)
    assert "BtxLstmGrads" in hdr
    Lb = _lib.lib()
    assert Lb.btx_abi_version() == 9
    # saved: gates [T][B][4H] f32, then c [T][B][H] f32, each 256-byte aligned; workspace: dgates + the f32 dc carry
    assert Lb.btx_lstm_train_saved_bytes(64, 512, 64) == 64 * 64 * 2048 * 4 + 64 * 64 * 512 * 4
    assert Lb.btx_lstm_train_saved_bytes(3, 10, 5) == 2560 + 768  # 5*3*40*4 = 2400 and 5*3*10*4 = 600, rounded up
    assert Lb.btx_lstm_train_workspace_bytes(3, 10, 5) == Lb.btx_lstm_workspace_bytes(1, 3, 10, 5)
    assert Lb.btx_lstm_train_saved_bytes(0, 10, 5) == 0 and Lb.btx_lstm_train_workspace_bytes(3, 10, 0) == 0


FAKE = ctypes.c_void_p(16)  # never dereferenced: every call below returns before a launch
LAY = _lib.LstmLayer(FAKE.value, FAKE.value, None, None, 1, 0, None)
LAYB = _lib.LstmLayer(FAKE.value, FAKE.value, FAKE.value, FAKE.value, 1, 0, None)
NOMU = _lib.LstmLayer(None, FAKE.value, None, None, 1, 0, None)
HALF = _lib.LstmLayer(FAKE.value, FAKE.value, FAKE.value, None, 1, 0, None)


def fwd(kind=0, ih=LAY, hh=LAY, x=FAKE, h0=None, c0=None, B=2, I=3, H=4, T=5, act=0, prec=0, ws=1 << 20, saved=FAKE,
        saved_bytes=1 << 20, kl=(None, None, None)):
    Lb = _lib.lib()
    return Lb.btx_lstm_fwd_train(kind, ctypes.byref(ih), ctypes.byref(hh), 0, x, h0, c0, FAKE, FAKE, kl[0], kl[1], kl[2], B, I,
                                 H, T, act, prec, FAKE, ws, saved, saved_bytes, None)


def bwd(kind=0, ih=LAY, hh=LAY, x=FAKE, h0=None, c0=None, hs=FAKE, saved=FAKE, B=2, I=3, H=4, T=5, act=0, prec=0, ws=1 << 20,
        gi=None, gh=None):
    Lb = _lib.lib()
    return Lb.btx_lstm_bwd(kind, ctypes.byref(ih), ctypes.byref(hh), 0, x, h0, c0, hs, saved, FAKE, None, FAKE, None, None,
                           ctypes.byref(gi) if gi is not None else None, ctypes.byref(gh) if gh is not None else None,
                           B, I, H, T, act, prec, FAKE, ws, None)


def test_training_forward_refuses_bad_arguments():
    Lb = _lib.lib()
    assert fwd(saved=None) == E_NULL
    assert fwd(x=None) == E_NULL
    assert fwd(ih=NOMU) == E_NULL and fwd(hh=HALF) == E_NULL
    assert fwd(h0=FAKE) == E_NULL
    assert fwd(kl=(None, None, FAKE)) == E_NULL
    assert fwd(kind=2) == _lib.E_UNSUPPORTED
    assert fwd(prec=2) == _lib.E_UNSUPPORTED  # bf16x3
    assert fwd(prec=3) == -5 and fwd(act=2) == -5
    for bad in (dict(B=0), dict(I=0), dict(H=0), dict(T=0), dict(B=-1)):
        assert fwd(**bad) == E_SHAPE, bad
    assert fwd(ws=Lb.btx_lstm_train_workspace_bytes(2, 4, 5) - 1) == E_WORKSPACE
    assert fwd(saved_bytes=Lb.btx_lstm_train_saved_bytes(2, 4, 5) - 1) == E_WORKSPACE


def test_backward_refuses_bad_arguments():
    Lb = _lib.lib()
    g = _lib.LstmGrads(FAKE.value, FAKE.value, None, None)
    gb = _lib.LstmGrads(FAKE.value, FAKE.value, FAKE.value, FAKE.value)
    assert bwd(saved=None) == E_NULL and bwd(hs=None) == E_NULL and bwd(x=None) == E_NULL
    assert bwd(ih=NOMU) == E_NULL and bwd(hh=HALF) == E_NULL
    assert bwd(c0=FAKE) == E_NULL
    assert bwd(gi=_lib.LstmGrads(None, FAKE.value, None, None), ws=0) == E_NULL
    assert bwd(gh=_lib.LstmGrads(FAKE.value, FAKE.value, FAKE.value, None), ws=0) == E_NULL
    assert bwd(gi=gb, ws=0) == E_NULL  # bias gradients of a layer without bias
    assert bwd(ih=LAYB, gi=gb, gh=g, ws=0) == E_WORKSPACE  # valid grads: the next check is the workspace
    assert bwd(kind=2) == _lib.E_UNSUPPORTED
    assert bwd(prec=2) == _lib.E_UNSUPPORTED  # bf16x3
    assert bwd(prec=3) == -5 and bwd(act=2) == -5
    for bad in (dict(B=0), dict(I=0), dict(H=0), dict(T=0)):
        assert bwd(**bad) == E_SHAPE, bad
    assert bwd(ws=Lb.btx_lstm_train_workspace_bytes(2, 4, 5) - 1) == E_WORKSPACE


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_fused_training_implies_fused_sequence(cls):
    layer = getattr(L, cls)(6, 5)
    assert not layer.fused_training and not layer.fused_sequence
    layer.fused_training = True
    assert layer.fused_training and layer.fused_sequence
    layer.fused_training = False
    assert not layer.fused_training and layer.fused_sequence


class SeqNet(nn.Module):
    def __init__(self, i=12, h=10, classes=3):
        super().__init__()
        self.lstm = nn.LSTM(i, h)
        self.fc = nn.Linear(h, classes)

    def forward(self, x):
        out, _ = self.lstm(x)
        return self.fc(out[:, -1, :])


def converted(kind, seed=0):
    torch.manual_seed(seed)
    m = SeqNet()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type=kind,
                          moped_enable=False, moped_delta=0.5))
    return m


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_fuse_model_lstm_training(kind):
    m = converted(kind)
    assert fuse_model(m) == 1
    assert m.lstm.fused_sequence and not m.lstm.fused_training  # the default call: inference only, as before
    m = converted(kind)
    assert fuse_model(m, lstm_training=True) == 1
    assert m.lstm.fused_sequence and m.lstm.fused_training
    m = converted(kind)
    fuse_model(m)
    assert fuse_model(m, lstm_training=True) == 0  # a second call switches training on and counts nothing
    assert m.lstm.fused_training


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_cpu_tensors_train_through_the_eager_loop(cls):
    grads = []
    for fused in (False, True):
        torch.manual_seed(3)
        layer = getattr(L, cls)(7, 6)
        layer.fused_training = fused
        x = torch.randn(3, 4, 7, requires_grad=True)
        torch.manual_seed(11)  # the CPU noise comes from torch's generator
        hs, (_, cs), kl = layer(x)
        (hs.square().sum() + cs.sum() + kl).backward()
        grads.append([x.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    for ga, gb in zip(*grads):
        assert torch.equal(ga, gb)
