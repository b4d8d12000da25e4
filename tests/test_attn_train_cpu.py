"""Fused attention training without a GPU: the sixth export table against include/btx_attn_train.h, argument errors
that come back before any launch, and the fused_training switch on the CPU, where it must change nothing."""
import ctypes
import os
import re

import pytest
import torch

from bayesian_torch_amd import _lib, layers as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_attn_train_is_the_header():
    text = open(os.path.join(ROOT, "include", "btx_attn_train.h")).read()
    declared = set(re.findall(r"\b(btx_[a-z0-9_]+)\s*\(", text.split("extern \"C\"", 1)[1]))
    T = _lib.EXPORTS_ATTN_TRAIN
    assert declared == set(T) and len(set(T)) == len(T)
    assert not set(T) & set(_lib.EXPORTS + _lib.EXPORTS_DROP + _lib.EXPORTS_GRU + _lib.EXPORTS_GRU_TRAIN + _lib.EXPORTS_ATTN)
    assert all(hasattr(_lib.lib(), n) for n in T)


E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3   # include/btx.h


@pytest.mark.parametrize("change,want", [(dict(q=None), E_NULL), (dict(lse=None), E_NULL), (dict(D=48), E_UNSUPPORTED),
                                         (dict(prec=_lib.PREC_CODE["bf16x3"]), E_UNSUPPORTED), (dict(causal=2), E_SHAPE)],
                         ids=lambda v: "-".join(v) if isinstance(v, dict) else str(v))
def test_argument_errors_return_before_any_launch(change, want):
    """host memory stands in for the device pointers: a call that got as far as a launch could not return these codes"""
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = dict(q=p, lse=p, D=32, prec=_lib.PREC_CODE["f32"], causal=0)
    a.update(change)
    st8, st16 = (ctypes.c_int64 * 8)(*[32, 32] * 4), (ctypes.c_int64 * 16)(*[32, 32] * 8)
    tail = (None, 1, a["causal"], 1.0, _lib.ACT_F32, a["prec"], None)
    assert lib.btx_attn_fwd_train(a["q"], p, p, p, a["lse"], 1, 1, 1, 1, a["D"], st8, *tail) == want
    assert lib.btx_attn_bwd(a["q"], p, p, p, p, a["lse"], p, p, p, p, 1, 1, 1, 1, a["D"], st16, *tail) == want


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_on_the_cpu_the_switch_changes_nothing(kind):
    res = []
    for fused in (False, True):
        torch.manual_seed(3)
        m = getattr(L, "MultiheadAttention" + kind)(32, 4, batch_first=True)
        m.fused_training = fused
        assert m.fused_training == fused and m.fused_attention == fused
        x = torch.randn(2, 5, 32, generator=torch.Generator().manual_seed(4)).requires_grad_()
        assert not m._fused_train_ok(x, None, False, None, False)
        out, _, kl = m(x, x, x, is_causal=True)
        (out.square().sum() + kl).backward()
        res.append([out.detach(), x.grad] + [p.grad for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*res))
