"""Fused Bayesian GRU training without a GPU: the fourth export table (_lib.EXPORTS_GRU_TRAIN against include/btx_gru_train.h), the
size queries, the argument errors of btx_gru_fwd_train / btx_gru_bwd (all returned before anything is launched) and the CPU
behaviour of fused_training (the eager loop)."""
import ctypes
import os
import re

import pytest
import torch

from bayesian_torch_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_UNSUP, E_WS, E_DTYPE = -1, -2, -3, -4, -5


def test_export_hygiene_of_the_fourth_table():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "btx_gru_train.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(btx_[a-z0-9_]+)\s*\(", src))
    T = _lib.EXPORTS_GRU_TRAIN
    assert names and names == set(T) and len(set(T)) == len(T)
    assert not set(T) & set(_lib.EXPORTS + _lib.EXPORTS_DROP + _lib.EXPORTS_GRU)
    raw, lib = ctypes.CDLL(_lib.lib_path()), _lib.lib()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes is not None for n in T)
    assert lib.btx_abi_version() == 9 and _lib.ABI_VERSION == 9


def test_size_queries():
    lib = _lib.lib()
    a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    B, H, T = 5, 10, 3
    planes = a256(T * B * 4 * H * 4)   # [T][B][4H] f32
    assert lib.btx_gru_train_saved_bytes(B, H, T) == planes
    assert lib.btx_gru_train_workspace_bytes(B, H, T) == planes + a256(B * H * 4)   # dG, then the f32 carry [B][H]
    assert lib.btx_gru_train_workspace_bytes(B, H, T) >= lib.btx_gru_workspace_bytes(1, B, H, T)   # the forward's Gi fits
    for bad in ((0, H, T), (B, -1, T), (B, H, 0)):
        assert lib.btx_gru_train_saved_bytes(*bad) == 0 and lib.btx_gru_train_workspace_bytes(*bad) == 0


def test_argument_errors_return_before_any_launch():
    lib = _lib.lib()
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is refused on the host
    full, bare = _lib.LstmLayer(64, 64, 64, 64, 1, 0, None), _lib.LstmLayer(64, 64, None, None, 1, 0, None)
    F, Bare = ctypes.byref(full), ctypes.byref(bare)
    B, I, H, T = 5, 7, 10, 3
    ws, sv = lib.btx_gru_train_workspace_bytes(B, H, T), lib.btx_gru_train_saved_bytes(B, H, T)

    def fwd(kind=0, ih=F, hh=F, x=p, hs=p, shape=(B, I, H, T), act=0, prec=0, w=p, nws=ws, s=p, nsv=sv):
        return lib.btx_gru_fwd_train(kind, ih, hh, 1, x, None, hs, None, None, None, *shape, act, prec, w, nws, s, nsv, None)

    def bwd(kind=0, ih=F, hh=F, x=p, hs=p, s=p, gi=None, gh=None, shape=(B, I, H, T), act=0, prec=0, w=p, nws=ws):
        return lib.btx_gru_bwd(kind, ih, hh, 1, x, None, hs, s, None, None, None, gi, gh, *shape, act, prec, w, nws, None)

    half = [ctypes.byref(_lib.LstmLayer(64, 64, 64, None, 1, 0, None)), ctypes.byref(_lib.LstmLayer(64, 64, None, 64, 1, 0, None))]
    for f in (fwd, bwd):
        for kw in (dict(ih=None), dict(hh=None), dict(x=None), dict(hs=None), dict(w=None), dict(s=None),
                   dict(ih=ctypes.byref(_lib.LstmLayer(None, 64, None, None, 1, 0, None))), dict(ih=half[0]), dict(hh=half[1])):
            assert f(**kw) == E_NULL, (f.__name__, kw)
        assert f(prec=2) == E_UNSUP and f(kind=2) == E_UNSUP and f(act=2) == E_DTYPE and f(prec=3) == E_DTYPE
        for bad in ((0, I, H, T), (B, 0, H, T), (B, I, -2, T), (B, I, H, 0)):
            assert f(shape=bad) == E_SHAPE
        assert f(nws=ws - 1) == E_WS
    assert fwd(nsv=sv - 1) == E_WS
    assert lib.btx_gru_fwd_train(0, F, F, 1, p, None, p, None, None, p, B, I, H, T, 0, 0, p, ws, p, sv, None) == E_NULL  # kl_out alone
    g4, g2 = _lib.LstmGrads(64, 64, 64, 64), _lib.LstmGrads(64, 64, None, None)
    assert bwd(ih=Bare, gi=ctypes.byref(g4)) == E_NULL and bwd(hh=Bare, gh=ctypes.byref(g4)) == E_NULL   # bias grads, no bias
    assert bwd(gi=ctypes.byref(_lib.LstmGrads(64, None, None, None))) == E_NULL
    assert bwd(gh=ctypes.byref(_lib.LstmGrads(64, 64, 64, None))) == E_NULL
    assert bwd(ih=Bare, gi=ctypes.byref(g2), prec=2) == E_UNSUP   # a valid bias-less pair passes check_grads


@pytest.mark.parametrize("cls", ["GRUReparameterization", "GRUFlipout"])
def test_fused_training_on_the_cpu_is_the_eager_loop(cls):
    from bayesian_torch_amd import layers as L
    grads = []
    for fused in (False, True):
        torch.manual_seed(0)
        layer = getattr(L, cls)(6, 5)
        layer.fused_training = fused
        assert layer.fused_training is fused and layer.fused_sequence is fused
        torch.manual_seed(1)
        x = torch.randn(3, 4, 6, requires_grad=True)
        hs, h_t, kl = layer(x)
        assert torch.equal(h_t, hs[:, -1])
        (hs.sum() + kl).backward()
        grads.append([x.grad] + [p.grad for p in layer.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
