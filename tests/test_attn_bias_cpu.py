"""Fused attention with a score bias without a GPU: the seventh export table against include/btx_attn_bias.h, argument
errors that come back before any launch, the errors of the `bias` keyword by name, the [B * heads, T, T] mask through the composite
against nn.MultiheadAttention, and the switches on the CPU, where they must change nothing."""
import ctypes
import os
import re

import pytest
import torch

from bayesian_torch_amd import _lib, functional as BF, layers as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -5, -6   # include/btx.h


def test_exports_attn_bias_is_the_header():
    text = open(os.path.join(ROOT, "include", "btx_attn_bias.h")).read()
    declared = set(re.findall(r"\b(btx_[a-z0-9_]+)\s*\(", text.split("extern \"C\"", 1)[1]))
    T = _lib.EXPORTS_ATTN_BIAS
    assert declared == set(T) and len(set(T)) == len(T) == 3
    others = _lib.EXPORTS + _lib.EXPORTS_DROP + _lib.EXPORTS_GRU + _lib.EXPORTS_GRU_TRAIN + _lib.EXPORTS_ATTN + _lib.EXPORTS_ATTN_TRAIN
    assert not set(T) & set(others)
    assert all(hasattr(_lib.lib(), n) for n in T) and _lib.lib().btx_abi_version() == 9


@pytest.mark.parametrize("change,want", [(dict(q=None), E_NULL), (dict(bstrides=None), E_NULL), (dict(brows=0), E_SHAPE),
                                         (dict(bstrides=(0, -4, 4)), E_SHAPE), (dict(bdtype=3), E_DTYPE), (dict(boff=2), E_ALIGN),
                                         (dict(causal=2), E_SHAPE)],
                         ids=lambda v: "-".join(v) if isinstance(v, dict) else str(v))
def test_argument_errors_return_before_any_launch(change, want):
    """host memory stands in for the device pointers: a call that got as far as a launch could not return these codes"""
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = dict(q=p, bstrides=(0, 0, 4), brows=1, bdtype=0, boff=0, causal=0)
    a.update(change)
    st8, st16 = (ctypes.c_int64 * 8)(*[32, 32] * 4), (ctypes.c_int64 * 16)(*[32, 32] * 8)
    bs = (ctypes.c_int64 * 3)(*a["bstrides"]) if a["bstrides"] is not None else None
    tail = (None, 1, a["causal"], 1.0, _lib.ACT_F32, _lib.PREC_CODE["f32"], None, p + a["boff"], a["bdtype"], a["brows"], bs)
    assert lib.btx_attn_bias_fwd(a["q"], p, p, p, 1, 1, 1, 1, 32, st8, *tail) == want
    assert lib.btx_attn_bias_fwd_train(a["q"], p, p, p, p, 1, 1, 1, 1, 32, st8, *tail) == want
    assert lib.btx_attn_bias_bwd(a["q"], p, p, p, p, p, p, p, p, p, 1, 1, 1, 1, 32, st16, *tail) == want


@pytest.mark.parametrize("bias,word", [(torch.zeros(5, 7, dtype=torch.float16), "bool, uint8, float32 or bfloat16"),
                                       (torch.zeros(5, 7, dtype=torch.float64), "bool, uint8, float32 or bfloat16"),
                                       (torch.zeros(5, 7).requires_grad_(), "no gradient"), (torch.zeros(7, 5), "bias must be [Tq, Tk]"),
                                       (torch.zeros(3, 5, 7), "bias must be [Tq, Tk]"), (torch.zeros(4, 2, 5, 7), "B dividing rows"),
                                       (torch.zeros(2, 3, 5, 7), "bias must be [Tq, Tk]")], ids=lambda v: "")
def test_bias_errors_are_raised_by_name(bias, word):
    """rows 6, heads 2, Tq 5, Tk 7: the checks need no device"""
    with pytest.raises(_lib.BtxError, match="attn_hip: .*" + re.escape(word)):
        BF._attn_bias("attn_hip", bias, 6, 2, 5, 7, torch.device("cpu"))


@pytest.mark.parametrize("shape,strides", [((5, 7), (0, 0, 7)), ((2, 5, 7), (0, 35, 7)), ((6, 5, 7), (70, 35, 7)), ((3, 1, 1, 7), (7, 0, 0)),
                                           ((3, 2, 5, 7), (70, 35, 7))], ids=str)
def test_bias_forms_become_strides_without_a_copy(shape, strides):
    b = torch.zeros(shape, dtype=torch.bool)
    kept, (ptr, code, B, s) = BF._attn_bias("attn_hip", b, 6, 2, 5, 7, torch.device("cpu"))
    assert ptr == b.data_ptr() and code == 2 and tuple(s) == strides and B == (3 if len(shape) == 4 or shape[0] == 6 else 1)
    ex = torch.zeros(7)[None, None, None, :].expand(3, 2, 5, 7)   # expanded axes: stride 0, nothing materialised
    kept, (ptr, code, B, s) = BF._attn_bias("attn_hip", ex, 6, 2, 5, 7, torch.device("cpu"))
    assert ptr == ex.data_ptr() and code == 0 and tuple(s) == (0, 0, 0) and B == 3


def test_a_batch_heads_mask_through_the_composite_is_torchs():
    torch.manual_seed(0)
    ref = torch.nn.MultiheadAttention(32, 4, batch_first=True).double()
    x = torch.randn(3, 6, 32, dtype=torch.float64)
    mask = torch.randn(12, 6, 6, dtype=torch.float64)
    want = ref(x, x, x, attn_mask=mask, need_weights=False)[0].detach()
    m = L.MultiheadAttentionReparameterization(32, 4, batch_first=True).double()
    with torch.no_grad():
        for lin, w, b in ((m.in_proj, ref.in_proj_weight, ref.in_proj_bias), (m.out_proj, ref.out_proj.weight, ref.out_proj.bias)):
            lin.mu_weight.copy_(w)
            lin.mu_bias.copy_(b)
            lin.rho_weight.fill_(-200.0)
            lin.rho_bias.fill_(-200.0)
        got = m(x, x, x, attn_mask=mask, return_kl=False)[0]
    assert float((got - want).abs().max()) <= 1e-12
    with pytest.raises(_lib.BtxError, match="attn_mask must be"):
        m(x, x, x, attn_mask=mask[:5], return_kl=False)


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_on_the_cpu_the_switches_change_nothing(kind):
    res = []
    fpad = torch.zeros(2, 5).masked_fill(torch.arange(5)[None, :] >= torch.tensor([5, 3])[:, None], float("-inf"))
    win = torch.zeros(5, 5).masked_fill(torch.ones(5, 5, dtype=torch.bool).triu(2), float("-inf"))
    for fused in (False, True):
        torch.manual_seed(3)
        m = getattr(L, "MultiheadAttention" + kind)(32, 4, batch_first=True)
        m.fused_training = fused
        x = torch.randn(2, 5, 32, generator=torch.Generator().manual_seed(4)).requires_grad_()
        assert not m._fused_ok(x, fpad, False, win, False) and not m._fused_train_ok(x, fpad, False, win, False)
        out, _, kl = m(x, x, x, key_padding_mask=fpad, attn_mask=win)
        (out.square().sum() + kl).backward()
        res.append([out.detach(), x.grad] + [p.grad for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*res))
