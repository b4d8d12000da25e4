"""CPU: the helper of the stride contract (tests/strided.py), the CPU routes under its views, and the completeness of the GPU file's
cover table (DESIGN.md "Stride contract").

The CPU routes are ATen op chains, which know a tensor's strides: a strided view must give `torch.equal` results to the dense call —
for the eager layer forwards, the `*_aten` restatements of functional.py and the CPU models the GPU tests compare against.  The
completeness check needs no GPU: every export of the three tuples of _lib is either in STRIDED_COVER of tests/test_gpu_strided.py
(with the tests that drive it, or a reason why its wrapper has no strided input) or in NO_TENSOR_ARGS.
"""
import numpy as np
import pytest
import torch

import strided as S

CL = torch.channels_last


def _samples():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {
        "nchw": r(4, 16, 5, 5), "cl": r(4, 16, 5, 5).contiguous(memory_format=CL), "cl-bf16": r(2, 8, 3, 3).bfloat16().contiguous(memory_format=CL),
        "seq": r(3, 4, 5), "logits": r(5, 7), "vector": r(9), "rows-equal": r(1, 6).expand(4, 6).contiguous(),
        "labels": torch.full((5,), 3, dtype=torch.int64), "u8-cl": torch.randint(0, 256, (2, 16, 3, 3), generator=g, dtype=torch.uint8).contiguous(memory_format=CL),
        "f64": r(6).double(),
    }


WANT = {"nchw": ["batch_step2", "chan_narrow", "other_format"], "cl": ["batch_step2", "chan_narrow", "other_format"],
        "cl-bf16": ["batch_step2", "chan_narrow", "other_format"], "seq": ["batch_step2", "chan_narrow", "permuted", "last_step2"],
        "logits": ["batch_step2", "last_step2"], "vector": ["last_step2"], "rows-equal": ["batch_step2", "last_step2", "expanded"],
        "labels": ["last_step2", "expanded"], "u8-cl": ["batch_step2", "chan_narrow", "other_format"], "f64": ["last_step2"]}


@pytest.mark.parametrize("name", sorted(WANT))
def test_helper_views(name):
    """every form: the values, shape and dtype of t; not stored as t is; first element on the 16-byte grid; the gaps hold the fill
    pattern, and gaps_intact notices one element written into a gap or into the slack"""
    t = _samples()[name]
    assert S.applicable(t) == WANT[name]
    for form, v, buf in S.views_of(t):
        assert torch.equal(v, t) and v.dtype == t.dtype and v.shape == t.shape, form
        assert not S.is_dense_as(v, t) and v.data_ptr() % 16 == 0, form
        assert buf.dim() == 1 and S.gaps_intact(buf, v), form
        mask = S.addressed(buf, v)
        assert int(mask.sum()) == (t.numel() // t.shape[0] if form == "expanded" else t.numel())
        # a dense misread / miswrite of numel elements from the first element stays inside the buffer, 64 bytes of slack behind it
        first = (v.data_ptr() - buf.data_ptr()) // t.element_size()
        assert first * t.element_size() >= 64 and (buf.numel() - first - t.numel()) * t.element_size() >= 64
        for at in (0, buf.numel() - 1, int((~mask).nonzero()[len((~mask).nonzero()) // 2])):
            assert not mask[at]
            old = buf[at].clone()
            buf[at] = 1
            assert not S.gaps_intact(buf, v), (form, at)
            buf[at] = old
            assert S.gaps_intact(buf, v)
        if form in ("batch_step2", "chan_narrow", "last_step2"):
            assert int((~mask).sum()) > 2 * (64 // t.element_size()), "%s leaves no gap between the elements" % form
    with pytest.raises(ValueError, match="does not apply"):
        list(S.views_of(t, [f for f in S.FORMS if f not in WANT[name]][:1]))


def test_helper_flat_with_gaps():
    g = torch.Generator().manual_seed(1)
    ts = [torch.randn(5, generator=g), torch.randn(4097, generator=g), torch.randn(16, 3, 3, 16, generator=g).permute(0, 3, 1, 2)]
    views, buf = S.flat_with_gaps(ts)
    for v, t in zip(views, ts):
        assert torch.equal(v, t) and v.stride() == t.stride() and v.data_ptr() % 16 == 0
    assert S.gaps_intact_many(buf, views)
    buf[views[1].storage_offset() - 1] = 0.0
    assert not S.gaps_intact_many(buf, views)


# ---- the CPU routes ----------------------------------------------------------------------------------------------------------
def _each_view(t, kinds=None):
    for form, v, buf in S.views_of(t, kinds):
        yield form, v, buf


def _layer_call(layer, x):
    torch.manual_seed(11)   # the CPU route draws its noise from torch's generator
    out = layer(x)
    return [o.detach() for o in (out if isinstance(out, tuple) else (out,)) if isinstance(o, torch.Tensor)]


LAYERS = [("LinearReparameterization", dict(in_features=12, out_features=5), (4, 12)),
          ("LinearFlipout", dict(in_features=12, out_features=5), (4, 12)),
          ("Conv2dReparameterization", dict(in_channels=8, out_channels=6, kernel_size=3, padding=1), (2, 8, 5, 5)),
          ("Conv2dFlipout", dict(in_channels=8, out_channels=6, kernel_size=3, padding=1), (2, 8, 5, 5)),
          ("MCDropout", dict(p=0.25), (3, 8, 5, 5)), ("MCDropout2d", dict(p=0.25), (3, 8, 5, 5))]


@pytest.mark.parametrize("cls,kw,xs", LAYERS, ids=[c[0] for c in LAYERS])
def test_eager_layer_forwards(cls, kw, xs):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(3)
    torch.manual_seed(0)
    layer = getattr(L, cls)(**kw)
    x = torch.randn(*xs)
    bases = [x, x.contiguous(memory_format=CL)] if x.dim() == 4 else [x]
    wants = []
    for base in bases:
        bt.set_sample_index(layer, 4)
        wants.append(_layer_call(layer, base))
    for i, base in enumerate(bases):
        for form, v, buf in _each_view(base):
            bt.set_sample_index(layer, 4)
            got = _layer_call(layer, v)
            # the CPU route of the Flipout layers draws its sign tensors with x.clone().uniform_(), as the reference does: torch
            # fills them in the MEMORY order of x, so the noise of a logical element follows x's storage order.  The dense call
            # to compare with is therefore the one on the dense tensor of the view's own order (channels-last: stride 1 on axis 1)
            j = (1 if v.stride(1) == 1 else 0) if (x.dim() == 4 and "Flipout" in cls) else i
            assert all(torch.equal(a, b) for a, b in zip(got, wants[j])), (cls, form)
            assert S.gaps_intact(buf, v)


@pytest.mark.parametrize("cls", ["GRUReparameterization", "GRUFlipout", "LSTMReparameterization", "LSTMFlipout"])
def test_eager_rnn_loops(cls):
    """the eager GRU / LSTM loops on CPU tensors: x as permuted / batch_step2 / chan_narrow, h0 / c0 as batch_step2 / last_step2 /
    expanded give `torch.equal` results to the dense call.

    The loop is the reference's chain: step t hands the slice X[:, t, :] to F.linear as it is, so the row stride of that GEMM
    operand is T * I for the dense x, I for `permuted`, 2 * T * I for `batch_step2` and T * (I + 16) for `chan_narrow`.  Bit equality
    therefore rests on a property of ATen's CPU GEMM, not of this package: that the product of a [B, I] operand does not depend on
    its leading dimension.  A BLAS that picks another blocking or accumulation order per leading dimension breaks it; if this test
    fails for `x` alone on some host, with h0 / c0 passing, that is the place to look before suspecting the layers."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(3)
    torch.manual_seed(0)
    B, T, I, H = 3, 3, 5, 10
    layer = getattr(L, cls)(I, H)
    x = torch.randn(B, T, I)
    h0 = torch.randn(1, H).expand(B, H).contiguous()
    c0 = torch.randn(1, H).expand(B, H).contiguous()
    lstm = cls.startswith("LSTM")

    def run(x, h0, c0):
        torch.manual_seed(11)
        bt.set_sample_index(layer, 4)
        out = layer(x, (h0, c0)) if lstm else layer(x, h0)
        flat = []
        for o in out:
            flat += list(o) if isinstance(o, tuple) else [o]
        return [o.detach() for o in flat if isinstance(o, torch.Tensor)]
    want = run(x, h0, c0)
    args = dict(x=x, h0=h0, c0=c0)
    for name, kinds in (("x", ["permuted", "batch_step2", "chan_narrow"]), ("h0", ["batch_step2", "last_step2", "expanded"]),
                        ("c0", ["batch_step2", "last_step2", "expanded"])):
        for form, v, buf in _each_view(args[name], kinds):
            got = run(**dict(args, **{name: v}))
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), (cls, name, form)
            assert S.gaps_intact(buf, v)


def test_aten_restatements():
    """the *_aten functions of functional.py under the views"""
    from bayesian_torch_amd import functional as BF, priors
    g = torch.Generator().manual_seed(2)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, w, b = r(2, 8, 5, 5), r(6, 8, 3, 3), r(6)
    op = BF.OpDesc(2, 8, 6, 3, 1, 1)
    want = BF.contract_aten(x, w, b, op)
    for form, v, buf in _each_view(x):
        assert torch.equal(BF.contract_aten(v, w, b, op), want), form
    for form, v, buf in _each_view(b):
        assert torch.equal(BF.contract_aten(x, w, v, op), want), form
    mu, rho = r(4097) * 0.3, r(4097) - 2
    sig = BF.softplus_naive(rho)
    eps = r(2, 4097)
    prior = priors.ScaleMixturePrior(0.25, 1.0, 0.05)
    for fn in (lambda m, s: BF.kl_aten(m, s, torch.tensor(0.0), torch.tensor(1.0)), lambda m, s: BF.kl_logu_aten(m, s, "sum"),
               lambda m, s: BF.log_alpha_aten(m, s)[0], lambda m, s: BF.kl_mc_aten(m, s, eps, prior)):
        want = fn(mu, sig)
        for form, v, buf in _each_view(mu):
            assert torch.equal(fn(v, sig), want), form
        for form, v, buf in _each_view(sig):
            assert torch.equal(fn(mu, v), want), form
    T, scale = BF.dropout_params(0.25)
    for mode in ("element", "channel"):
        for base in (x, x.contiguous(memory_format=CL)):
            want = BF.dropout_aten(base, T, scale, mode, 5, 3, 41)
            for form, v, buf in _each_view(base):
                assert torch.equal(BF.dropout_aten(v, T, scale, mode, 5, 3, 41), want), (mode, form)
    assert torch.equal(BF.apply_act_aten(next(S.views_of(x, ["batch_step2"]))[1], "relu6"), BF.apply_act_aten(x, "relu6"))


def test_cpu_models_the_gpu_tests_compare_against():
    """the numpy / torch models take `.cpu().numpy()` copies of whatever the test hands them: under the views they see the values of
    the dense tensor (the copies are dense), so their results are those of the dense call"""
    import drop_model as DM
    import envelope as E
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 12, 5, 5, generator=g).bfloat16().contiguous(memory_format=CL)
    bits = lambda t: t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)  # noqa: E731
    keep = DM.mask((2, 12, 5, 5), "element", 49152, 5, 3, 7)
    want = DM.apply_bf16(bits(x), keep, 4.0 / 3.0)
    for form, v, buf in _each_view(x):
        assert np.array_equal(DM.apply_bf16(bits(v), keep, 4.0 / 3.0), want), form
    w, b = torch.randn(6, 12, 3, 3, generator=g), torch.randn(6, generator=g)
    op = dict(kind="conv", nd=2, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, transposed=False, output_padding=(0, 0))
    want = E.contract(E.d64(x), E.d64(w), E.d64(b), op)
    for form, v, buf in _each_view(x):
        assert torch.equal(E.d64(v), E.d64(x)), form
        assert torch.equal(E.contract(E.d64(v), E.d64(w), E.d64(b), op), want), form
    mu, rho = torch.randn(4097, generator=g) * 0.3, torch.randn(4097, generator=g) - 2
    want = E.kl_reference(mu.double().numpy(), rho.double().numpy(), 0.0, 1.0, 1.7)
    for form, v, buf in _each_view(mu):
        got = E.kl_reference(v.double().numpy(), rho.double().numpy(), 0.0, 1.0, 1.7)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), form


# ---- completeness ---------------------------------------------------------------------------------------------------------------
def test_every_export_is_covered_or_takes_no_tensor():
    from bayesian_torch_amd import _lib
    import test_gpu_strided as G
    exports = _lib.EXPORTS + _lib.EXPORTS_DROP + _lib.EXPORTS_GRU
    assert len(set(exports)) == len(exports)
    cover, none = set(G.STRIDED_COVER), set(G.NO_TENSOR_ARGS)
    assert not cover & none
    missing = [e for e in exports if e not in cover and e not in none]
    assert not missing, "exports without a strided-input case or a place in NO_TENSOR_ARGS: %s" % missing
    assert not (cover | none) - set(exports), "names that are no export: %s" % sorted((cover | none) - set(exports))
    required = {"btx_abi_version", "btx_strerror", "btx_contract_plan_info", "btx_out_shape", "btx_contract_pool_shape",
                "btx_mc_packed_floats", "btx_mc_eval_state_doubles", "btx_q8_weight_row_bytes"}
    assert required <= none
    assert all(e in required or e.endswith("_bytes") or e.endswith("_bytes_lanes") for e in none), sorted(none)
    for e, tests in G.STRIDED_COVER.items():
        assert tests or e in G.NO_STRIDED_INPUT, "%s: neither a driving test nor a reason" % e
        for t in tests:
            assert callable(getattr(G, t, None)), (e, t)
    assert set(G.NO_STRIDED_INPUT) <= cover
