"""GPU: every kernel entry on strided, NON-DENSE views (DESIGN.md "Stride contract").

Every HIP entry point receives a bare `data_ptr()`; the strides are known to the Python wrappers alone.  The sibling files pin the
neighbouring contracts — tests/test_gpu_alignment.py dense tensors off the 16-byte grid, tests/test_gpu_poison.py stale memory, case
S4 of tests/autograd_cases.py strided OUTPUT gradients (stride-0, NCHW and off-grid `dy` of every autograd Function: not repeated
here).  This file hands the public wrappers strided INPUTS: each case makes the dense call once and repeats it with one tensor
argument at a time replaced by each applicable view of tests/strided.py.

  read-only argument      every result has the BITS of the dense call (poison.bits_equal; the wrappers make one dense copy and launch
                          the same kernel, or the kernel reads the strides / another dense layout as it is: BTX-DROP's mask belongs to
                          the logical element), and the fill pattern around and between the view's elements is intact
  argument written to     the logical values after the call equal the dense call's and the gaps are intact ("through"), or the wrapper
                          raises BtxError / ValueError naming the argument ("refused")

No tolerance anywhere, and no quiet fall-back: every call on a view must enter exactly the kernel entries the dense call entered
(`entered`, checked inside `sweep` per view).  OUTCOMES records (entry group, argument, form) -> "as is" | "copy" | "through" | "refused"; the table of
DESIGN.md is written from it.  STRIDED_COVER maps every export that takes a tensor to the tests here that drive it; each test records
the btx_* entries it entered and asserts that the ones the table promises were among them.  tests/test_strided_cpu.py checks the
table against the three export tuples without a GPU.
"""
import contextlib
import copy
import warnings

import numpy as np
import pytest
import torch

import strided as S
from poison import bits_equal

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8

# exports without a tensor argument (queries answered on the host)
NO_TENSOR_ARGS = [
    "btx_abi_version", "btx_strerror", "btx_kl_workspace_bytes", "btx_kl_model_workspace_bytes", "btx_contract_workspace_bytes",
    "btx_contract_pool_shape", "btx_contract_plan_info", "btx_out_shape", "btx_mc_packed_floats", "btx_sampled_w_bytes",
    "btx_sampled_w_bytes_lanes", "btx_bn_workspace_bytes", "btx_wgrad_workspace_bytes", "btx_lstm_workspace_bytes",
    "btx_lstm_train_saved_bytes", "btx_lstm_train_workspace_bytes", "btx_calib_workspace_bytes", "btx_q8_weight_row_bytes",
    "btx_optim_grad_norm_workspace_bytes", "btx_mcloss_workspace_bytes", "btx_bias_grad_workspace_bytes", "btx_mc_eval_state_doubles",
    "btx_mc_eval_workspace_bytes", "btx_mc_gnll_workspace_bytes", "btx_reg_eval_workspace_bytes", "btx_lrt_bwd_workspace_bytes",
    "btx_kl_mc_workspace_bytes", "btx_kl_logu_workspace_bytes", "btx_gru_workspace_bytes",
]

# entries whose wrapper takes no strided tensor from the caller: the reason, next to the test that still enters them
NO_STRIDED_INPUT = {
    "btx_sample_weights": "superseded by btx_sample_weights_lanes (functional.sample_weights always calls the lanes entry)",
    "btx_sample_weights_lanes": "reads mu / rho as gemm_major_view hands them (dense, on the grid) and writes a buffer of its own",
    "btx_fill_eps": "no input tensor: fills a fresh buffer from (seed, sample, layer, stream)",
    "btx_fill_sign": "no input tensor: fills a fresh buffer from (seed, sample, layer, stream)",
    "btx_contract_fwd": "the wrappers call btx_contract_fwd_ex / _lanes, which btx_contract_fwd forwards to",
}

# export -> the tests of this file that enter it (checked by each test against the calls it recorded)
STRIDED_COVER = {
    "btx_contract_fwd_ex": ["test_contraction_forward"],
    "btx_contract_fwd_lanes": ["test_contraction_forward_lanes"],
    "btx_contract_fwd": [],
    "btx_rowfuse_pack": ["test_contraction_forward"],
    "btx_sample_weights_lanes": [],
    "btx_sample_weights": [],
    "btx_fill_eps": ["test_backward_atomics_path"],
    "btx_fill_sign": [],
    "btx_contract_wgrad_ws": ["test_backward_through_autograd"],
    "btx_bias_grad": ["test_backward_through_autograd"],
    "btx_dgrad_weights": ["test_backward_through_autograd"],
    "btx_contract_wgrad": ["test_backward_atomics_path"],
    "btx_rho_grad": ["test_backward_atomics_path"],
    "btx_lrt_fwd_train": ["test_lrt_training"],
    "btx_lrt_bwd": ["test_lrt_training"],
    "btx_gru_fwd": ["test_gru_sequence"],
    "btx_lstm_fwd": ["test_lstm_sequence_and_training"],
    "btx_lstm_fwd_train": ["test_lstm_sequence_and_training"],
    "btx_lstm_bwd": ["test_lstm_sequence_and_training"],
    "btx_bn_train_fwd": ["test_batchnorm_training"],
    "btx_bn_train_bwd": ["test_batchnorm_training"],
    "btx_maxpool2d_cl": ["test_pools"],
    "btx_maxpool2d_cl_train": ["test_pools"],
    "btx_maxpool2d_cl_bwd": ["test_pools"],
    "btx_avgpool_global_cl": ["test_pools"],
    "btx_dropout_fwd": ["test_dropout"],
    "btx_dropout_bwd": ["test_dropout"],
    "btx_mc_ce_fwd": ["test_classification_heads"],
    "btx_mc_ce_bwd": ["test_classification_heads"],
    "btx_avu_mc_fwd": ["test_classification_heads"],
    "btx_avu_mc_bwd": ["test_classification_heads"],
    "btx_avu_fwd": ["test_classification_heads"],
    "btx_avu_bwd": ["test_classification_heads"],
    "btx_eau_fwd": ["test_classification_heads"],
    "btx_eau_bwd": ["test_classification_heads"],
    "btx_mc_accumulate": ["test_mc_accumulate_and_evaluator"],
    "btx_mc_accumulate_lanes": ["test_mc_accumulate_and_evaluator"],
    "btx_mc_eval": ["test_mc_accumulate_and_evaluator"],
    "btx_mc_gnll_fwd": ["test_regression_heads"],
    "btx_mc_gnll_bwd": ["test_regression_heads"],
    "btx_mc_moments_lanes": ["test_regression_heads"],
    "btx_reg_eval_update": ["test_regression_heads"],
    "btx_kl_gauss": ["test_kl_family"],
    "btx_kl_gauss_model": ["test_kl_family"],
    "btx_kl_gauss_model_bwd": ["test_kl_family"],
    "btx_kl_mc_model": ["test_kl_family"],
    "btx_kl_mc_model_bwd": ["test_kl_family"],
    "btx_kl_logu_model": ["test_kl_family"],
    "btx_kl_logu_model_bwd": ["test_kl_family"],
    "btx_logalpha_stats": ["test_log_alpha_statistics_and_pruning"],
    "btx_logalpha_prune": ["test_log_alpha_statistics_and_pruning"],
    "btx_optim_sgd": ["test_optimizers"],
    "btx_optim_adam": ["test_optimizers"],
    "btx_optim_grad_norm": ["test_optimizers"],
    "btx_bucket_pack": ["test_gradient_bucket"],
    "btx_bucket_unpack": ["test_gradient_bucket"],
    "btx_q8_quantize_act": ["test_int8"],
    "btx_q8_sample_weights": ["test_int8"],
    "btx_q8_contract": ["test_int8"],
    "btx_q8_contract_res": ["test_int8"],
    "btx_q8_add": ["test_int8"],
    "btx_q8_maxpool2d_cl": ["test_int8"],
    "btx_q8_avgpool2d_cl": ["test_int8"],
    "btx_q8_sample_delta": ["test_int8_flipout"],
    "btx_q8_contract_flipout": ["test_int8_flipout"],
}

# (entry group, argument, form) -> "as is" | "copy" | "through" | "refused": filled while the tests run, printed by each test
OUTCOMES = {}


# =============================================================================================================================
# helpers
# =============================================================================================================================
def _dev():
    return torch.device("cuda")


@contextlib.contextmanager
def recording():
    """the set of btx_* entries entered while the block runs (every export of the three tuples)"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    seen, saved = set(), []

    def wrap(name, orig):
        def entry(*a):
            seen.add(name)
            return orig(*a)
        return entry
    try:
        for name in _lib.EXPORTS + _lib.EXPORTS_DROP + _lib.EXPORTS_GRU:
            orig = getattr(L, name)
            saved.append((name, orig))
            setattr(L, name, wrap(name, orig))
        yield seen
    finally:
        for name, orig in saved:
            setattr(L, name, orig)


def entered(fn):
    """(fn(), the kernel entries it entered): the exports that take tensors; the host-side queries of NO_TENSOR_ARGS are answered
    from caches after the first call and are left out"""
    with recording() as seen:
        out = fn()
        torch.cuda.synchronize()
    return out, frozenset(seen) - frozenset(NO_TENSOR_ARGS)


def _covered(seen, test, but=()):
    """every export STRIDED_COVER lists for `test` was entered (`but`: the ones another case of a parametrised test enters)"""
    want = {e for e, tests in STRIDED_COVER.items() if test in tests} - set(but)
    print("%s entered: %s" % (test, " ".join(sorted(seen))))
    assert want and want <= seen, "%s never entered %s" % (test, sorted(want - seen))


def _note(group, arg, form, outcome):
    OUTCOMES[(group, arg, form)] = outcome
    print("outcome %-28s %-14s %-13s %s" % (group, arg, form, outcome))


def sweep(group, call, args, forms, outcome="copy"):
    """call(**args) once on the dense tensors, then once per (argument, form) of `forms` = {argument: [form, ...]} with that
    argument alone replaced by the view: the bits of the dense result, and the gaps of the view intact"""
    want, kernels = entered(lambda: call(**args))
    assert kernels, "%s: the dense call entered no kernel" % group
    for name, kinds in forms.items():
        for form, view, buf in S.views_of(args[name], kinds):
            assert not S.is_dense_as(view, args[name]), (group, name, form)
            got, k = entered(lambda: call(**dict(args, **{name: view})))
            # no quiet fall-back: the call on the view enters the kernels the dense call entered, nothing less
            assert k == kernels, "%s: %s as %s entered %s, the dense call %s" % (group, name, form, sorted(k), sorted(kernels))
            assert bits_equal(got, want), "%s: %s as %s differs from the dense call" % (group, name, form)
            assert S.gaps_intact(buf, view), "%s: %s as %s: a store outside the view" % (group, name, form)
            _note(group, name, form, outcome[name] if isinstance(outcome, dict) else outcome(form) if callable(outcome) else outcome)
    return want


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _randn(*shape, seed=0, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(_dev()).to(dtype)


def _ints(shape, seed, dtype=F32, lim=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).to(_dev()).to(dtype)


# =============================================================================================================================
# 1. contraction forward
# =============================================================================================================================
def _fwd_cases():
    from test_gpu_alignment import FWD_CASES
    from test_depthwise_plan import GEOMS
    C, k, s, p, d, xs = GEOMS[0]
    dw = ("Conv2dReparameterization", dict(in_channels=C, out_channels=C, kernel_size=k, stride=s, padding=p, dilation=d, groups=C), xs, False)
    return list(FWD_CASES) + [dw]


def _fwd_ids():
    from test_gpu_elementwise import _tag
    return [_tag(*c[:3]) for c in _fwd_cases()]


X_FORMS = {4: ["batch_step2", "chan_narrow", "other_format"], 2: ["batch_step2", "last_step2"], 3: ["batch_step2", "chan_narrow", "permuted"]}


@pytest.mark.parametrize("case", range(len(_fwd_cases())), ids=_fwd_ids())
def test_contraction_forward(case):
    """contract_hip through layer._forward_hip, one layer per kernel family (the cases of the alignment file, asserted there to cover
    every fast family, plus the depthwise stencil), bf16 and f32: x as every form; on the first two cases the epilogue's scale /
    shift (last_step2) and residual (batch_step2, chan_narrow, other_format).  _to_channels_last makes the one dense copy; the
    row-fused stem's pack kernel (btx_rowfuse_pack) reads x's strides as they are."""
    from test_gpu_alignment import _x_of
    from test_gpu_elementwise import _make
    from test_gpu_fuse_model import _plan
    cls, kw, xs, _ = _fwd_cases()[case]
    nout = kw.get("out_channels", kw.get("out_features"))
    stem = kw.get("in_channels", 99) <= 4
    seen_all = set()
    for prec, act in (("bf16", BF16), ("f32", F32)):
        layer = _make(cls, kw, prec, seed=7, bt_seed=1234)
        rc, fam, _ = _plan(layer, xs, prec)
        assert rc == 0 and (fam != "gather" or kw.get("groups", 1) > 1), (cls, kw, prec, fam)
        x = _x_of(xs, act)
        args = dict(x=x)
        forms = dict(x=X_FORMS[x.dim()])

        def call(x, **ep):
            with torch.no_grad():
                return layer._forward_hip(x, sample_idx=5, epilogue=dict(ep, relu=1) if ep else None)
        with recording() as seen:
            base = sweep("contract_hip [%s]" % fam, call, args, forms, outcome="as is" if stem else "copy")
            if case < 2:
                g = torch.Generator().manual_seed(18)
                res = (torch.randn(base.shape, generator=g) * 4).to(_dev()).to(act)
                res = _cl(res) if res.dim() == 4 else res
                ep = dict(x=x, scale=(torch.rand(nout, generator=g) * 4 + 2).to(_dev()), shift=torch.randn(nout, generator=g).to(_dev()),
                          residual=res)
                sweep("contract_hip epilogue", call, ep, dict(scale=["last_step2"], shift=["last_step2"], residual=X_FORMS[res.dim()]))
        seen_all |= seen
    print("test_contraction_forward entered: %s" % " ".join(sorted(seen_all)))
    assert "btx_contract_fwd_ex" in seen_all and (not stem or "btx_rowfuse_pack" in seen_all)


def test_contraction_forward_lanes():
    """a 2-lane launch (btx_contract_fwd_lanes) whose per-lane x is batch_step2"""
    import bayesian_torch_amd as bt
    from test_gpu_alignment import FWD_CASES, _x_of
    from test_gpu_elementwise import _make
    cls, kw, xs, _ = next(c for c in FWD_CASES if c[1].get("in_channels", 0) > 4)
    with recording() as seen:
        for prec, act in (("bf16", BF16), ("f32", F32)):
            lay = _make(cls, kw, prec, seed=7, bt_seed=1234)
            xr = _x_of(xs, act)
            xx = _cl(torch.cat([xr, xr], 0))

            def call(x):
                with torch.no_grad():
                    bt.set_sample_index(lay, 8, presample=True)
                    lay._forward_hip(x[:xs[0]])
                    bt.set_sample_lanes(lay, [8, 21], batch=xs[0])
                    try:
                        return lay._forward_hip(x)
                    finally:
                        bt.set_sample_lanes(lay, None)
            both = sweep("contract_hip lanes=2", call, dict(x=xx), dict(x=["batch_step2"]))
            assert both.shape[0] == 2 * xs[0] and not torch.equal(both[:xs[0]], both[xs[0]:])
    _covered(seen, "test_contraction_forward_lanes")


# =============================================================================================================================
# 2. backward through autograd (x; the forms of dy are case S4 of tests/autograd_cases.py)
# =============================================================================================================================
def _bwd_call(layer):
    from test_gpu_alignment import _bwd_run

    def call(x, dy):
        return _bwd_run(layer, x, dy, 5)
    return call


@pytest.mark.parametrize("which", [0, 1, 5], ids=["conv-flipout-bf16", "conv-reparam-bf16", "linear-flipout-f32"])
def test_backward_through_autograd(which):
    """layer(x).backward(dy): wgrad_hip (btx_contract_wgrad_ws with the rho fold), btx_bias_grad, dgrad_weights_hip and the data
    gradient's contraction on views of x — out, dx, dmu, drho and the bias gradients carry the dense call's bits"""
    import bayesian_torch_amd as bt
    from test_gpu_alignment import BWD, _x_of
    from test_gpu_elementwise import _make
    cls, kw, xshape, act, _ = BWD[which]
    prec = "bf16" if act == BF16 else "f32"
    bt.set_precision(prec)
    try:
        layer = _make(cls, kw, None, seed=0, bt_seed=123)
        x = _x_of(xshape, act, seed=1, scale=1.0)
        bt.set_sample_index(layer, 5)
        with torch.no_grad():
            oshape = tuple(layer(x, return_kl=False).shape)
        dy = _randn(*oshape, seed=2, dtype=act)
        dy = _cl(dy) if dy.dim() == 4 else dy
        with recording() as seen:
            sweep("ContractFn.backward", _bwd_call(layer), dict(x=x, dy=dy), dict(x=X_FORMS[x.dim()]))
    finally:
        bt.set_precision("f32")
    if which == 0:
        _covered(seen, "test_backward_through_autograd")


def test_backward_atomics_path(monkeypatch):
    """functional.WGRAD_ATOMICS: btx_contract_wgrad with btx_rho_grad behind it.  Small-integer x / dy: every partial sum is an
    integer below 2^24, so the f32 atomics give one result whatever their order, and the views of x must give its bits."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    from test_gpu_alignment import BWD
    from test_gpu_elementwise import _make
    monkeypatch.setattr(BF, "WGRAD_ATOMICS", True)
    cls, kw, xshape, act, _ = BWD[5]
    layer = _make(cls, kw, None, seed=0, bt_seed=123)
    x = _ints(xshape, 31, act)
    dy = _ints((xshape[0], kw["out_features"]), 32, act)
    with recording() as seen:
        r = sweep("wgrad_hip atomics", _bwd_call(layer), dict(x=x, dy=dy), dict(x=X_FORMS[2]))
        with torch.no_grad():
            layer.materialize_noise(5, tuple(x.shape), tuple(dy.shape), x.dtype)
    assert float(r["dmu"].abs().max()) < 2 ** 24
    _covered(seen, "test_backward_atomics_path")


# =============================================================================================================================
# 3. local reparameterization: fused training
# =============================================================================================================================
@pytest.mark.parametrize("cls,kw,xs", [("Conv2dLocalReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, padding=1), (2, 16, 9, 9)),
                                       ("LinearLocalReparameterization", dict(in_features=72, out_features=50), (8, 72))], ids=["conv", "linear"])
def test_lrt_training(cls, kw, xs):
    """lrt_fwd_train_hip on views of x; lrt_bwd_hip on views of x, dy and the saved root"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import _lib, functional as BF, layers as L, rng
    bt.manual_seed(7)
    torch.manual_seed(0)
    layer = getattr(L, cls)(**kw).to(_dev())
    op = layer._op
    mu, rho = layer._w()
    mu_p, rho_p = BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op)
    mb, rb = layer.mu_bias.detach(), layer.rho_bias.detach()
    with recording() as seen:
        for prec, act in (("f32", F32), ("bf16", BF16)):
            x = _randn(*xs, seed=3, dtype=act)
            x = _cl(x) if x.dim() == 4 else x

            def fwd(x):
                return BF.lrt_fwd_train_hip(x, mu_p, rho_p, mb, rb, op, rng.seed(), 3, layer._btx_layer_id, prec=prec)
            out, root = sweep("lrt_fwd_train_hip", fwd, dict(x=x), dict(x=X_FORMS[x.dim()]))
            dy = _randn(*out.shape, seed=4, dtype=act)
            dy = _cl(dy) if dy.dim() == 4 else dy

            def bwd(x, dy, root):
                return BF.lrt_bwd_hip(x, dy, root, mu_p, rho_p, rb, op, rng.seed(), 3, layer._btx_layer_id, prec=prec)
            sweep("lrt_bwd_hip", bwd, dict(x=x, dy=dy, root=root), dict(x=X_FORMS[x.dim()], dy=X_FORMS[x.dim()], root=["last_step2"]))
            for bad in (root.double(), root[:-1]):
                with pytest.raises(_lib.BtxError, match="root"):
                    bwd(x, dy, bad)
            _note("lrt_bwd_hip", "root", "wrong dtype / size", "refused")
    _covered(seen, "test_lrt_training")


# =============================================================================================================================
# 4. GRU and LSTM sequences
# =============================================================================================================================
RNN_SHAPE = (3, 3, 5, 10)  # B, T, I, H


def _rnn_params(gates, seed):
    B, T, I, H = RNN_SHAPE
    mk = lambda i, *s: _randn(*s, seed=seed + i, scale=0.3)  # noqa: E731
    ih = (mk(0, gates * H, I), mk(1, gates * H, I) - 3.0, mk(2, gates * H), mk(3, gates * H) - 3.0, 701, 9, None)
    hh = (mk(4, gates * H, H), mk(5, gates * H, H) - 3.0, mk(6, gates * H), mk(7, gates * H) - 3.0, 702, 9, None)
    return ih, hh


@pytest.mark.parametrize("kind", ["reparam", "flipout"])
def test_gru_sequence(kind):
    """gru_hip: x as permuted / batch_step2 / chan_narrow, h0 as batch_step2 / last_step2 / expanded; a non-contiguous `out` is
    refused by name"""
    from bayesian_torch_amd import _lib, functional as BF
    B, T, I, H = RNN_SHAPE
    k = _lib.KIND_FLIPOUT if kind == "flipout" else _lib.KIND_REPARAM
    ih, hh = _rnn_params(3, 40)
    x = _randn(B, T, I, seed=1)
    h0 = _randn(1, H, seed=2).expand(B, H).contiguous()

    def call(x, h0):
        return BF.gru_hip(k, x, ih, hh, 77, prec="f32", h0=h0)[0]
    with recording() as seen:
        want = sweep("gru_hip", call, dict(x=x, h0=h0), dict(x=["permuted", "batch_step2", "chan_narrow"],
                                                             h0=["batch_step2", "last_step2", "expanded"]))
        for form, view, buf in S.views_of(want, ["batch_step2", "last_step2"]):
            with pytest.raises(_lib.BtxError, match="out must be a contiguous"):
                BF.gru_hip(k, x, ih, hh, 77, prec="f32", h0=h0, out=view)
            assert S.gaps_intact(buf, view)
            _note("gru_hip", "out", form, "refused")
    _covered(seen, "test_gru_sequence")


@pytest.mark.parametrize("kind", ["reparam", "flipout"])
def test_lstm_sequence_and_training(kind):
    """lstm_hip, lstm_train_fwd_hip and lstm_bwd_hip: x as permuted / batch_step2, h0 / c0 as batch_step2 / last_step2 / expanded,
    d_hidden_seq / d_c_seq as permuted / batch_step2"""
    from bayesian_torch_amd import _lib, functional as BF
    B, T, I, H = RNN_SHAPE
    k = _lib.KIND_FLIPOUT if kind == "flipout" else _lib.KIND_REPARAM
    ih, hh = _rnn_params(4, 60)
    x = _randn(B, T, I, seed=1)
    h0 = _randn(1, H, seed=2).expand(B, H).contiguous()
    c0 = _randn(1, H, seed=3).expand(B, H).contiguous()
    xf, hf = ["permuted", "batch_step2", "chan_narrow"], ["batch_step2", "last_step2", "expanded"]
    with recording() as seen:
        sweep("lstm_hip", lambda x, h0, c0: BF.lstm_hip(k, x, ih, hh, 77, prec="f32", h0=h0, c0=c0)[:2],
              dict(x=x, h0=h0, c0=c0), dict(x=xf, h0=hf, c0=hf))
        # (`saved` is a byte buffer with alignment padding nobody writes: it is handed on, not compared)
        sweep("lstm_train_fwd_hip", lambda x, h0, c0: BF.lstm_train_fwd_hip(k, x, ih, hh, 77, prec="f32", h0=h0, c0=c0)[:2],
              dict(x=x, h0=h0, c0=c0), dict(x=xf, h0=hf, c0=hf))
        hs, cs, _, saved = BF.lstm_train_fwd_hip(k, x, ih, hh, 77, prec="f32", h0=h0, c0=c0)
        d_hs, d_cs = _randn(B, T, H, seed=5), _randn(B, T, H, seed=6)

        def bwd(x, h0, c0, d_hs, d_cs):
            return BF.lstm_bwd_hip(k, x, ih, hh, 77, hs, saved, d_hs, d_cs, prec="f32", h0=h0, c0=c0, want_dh0=True, want_dc0=True)
        sweep("lstm_bwd_hip", bwd, dict(x=x, h0=h0, c0=c0, d_hs=d_hs, d_cs=d_cs),
              dict(x=xf, h0=hf, c0=hf, d_hs=["permuted", "batch_step2"], d_cs=["permuted", "batch_step2"]))
    _covered(seen, "test_lstm_sequence_and_training")


# =============================================================================================================================
# 5. BatchNorm training
# =============================================================================================================================
BN_SHAPE = (4, 16, 5, 5)


def _bn_call(bn, state):
    from bayesian_torch_amd import autograd as ag

    def call(x, dy, res, weight=None, bias=None, rm=None, rv=None):
        bn.load_state_dict(state)
        if weight is not None:
            bn.weight = torch.nn.Parameter(weight)
        if bias is not None:
            bn.bias = torch.nn.Parameter(bias)
        with torch.no_grad():  # the estimates are written in place: every call starts from the stored state
            if rm is not None:
                bn.running_mean = rm.copy_(state["running_mean"])
            if rv is not None:
                bn.running_var = rv.copy_(state["running_var"])
        x1 = x.detach().requires_grad_(True)
        r1 = res.detach().requires_grad_(True)
        assert ag.bn_train_usable(bn, x1)
        y = ag.batch_norm_train(bn, x1, residual=r1, relu=True)
        y.backward(dy)
        torch.cuda.synchronize()
        return dict(y=y.detach(), dx=x1.grad, dres=r1.grad, dgamma=bn.weight.grad.clone(), dbeta=bn.bias.grad.clone(),
                    rm=bn.running_mean.detach().clone(), rv=bn.running_var.detach().clone(), nbt=bn.num_batches_tracked.detach().clone())
    return call


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_batchnorm_training(dtype):
    """batch_norm_train with ReLU and residual: the residual as other_format / batch_step2 / chan_narrow / expanded (the kernel
    addresses it with x's strides: one copy in x's layout), weight / bias as last_step2 (one dense copy), the running estimates as
    last_step2 (written: a dense copy and back, the gaps intact).  x stored NCHW is not taken by the HIP path (bn_train_usable) and
    bn_act equals torch's own ops.  A residual of another shape or dtype is refused by name."""
    from bayesian_torch_amd import _lib, autograd as ag
    bn = torch.nn.BatchNorm2d(BN_SHAPE[1]).to(_dev())
    with torch.no_grad():
        bn.weight.copy_(_randn(16, seed=1) + 2)
        bn.bias.copy_(_randn(16, seed=2))
        bn.running_mean.copy_(_randn(16, seed=3))
        bn.running_var.copy_(_randn(16, seed=4).abs() + 0.5)
    state = copy.deepcopy(bn.state_dict())
    x, dy = _cl(_randn(*BN_SHAPE, seed=5, dtype=dtype)), _cl(_randn(*BN_SHAPE, seed=6, dtype=dtype))
    res = _cl(_randn(1, *BN_SHAPE[1:], seed=7, dtype=dtype).expand(BN_SHAPE).contiguous())
    call = _bn_call(bn, state)
    args = dict(x=x, dy=dy, res=res, weight=state["weight"].clone(), bias=state["bias"].clone(), rm=state["running_mean"].clone(),
                rv=state["running_var"].clone())
    with recording() as seen:
        want = sweep("batch_norm_train", call, args, dict(res=["other_format", "batch_step2", "chan_narrow", "expanded"],
                                                           weight=["last_step2"], bias=["last_step2"], rm=["last_step2"], rv=["last_step2"]),
                     outcome=dict(res="copy", weight="copy", bias="copy", rm="through", rv="through"))
    assert int(want["nbt"]) == 1 and not torch.equal(want["rm"], state["running_mean"]) and float(want["y"].abs().max()) > 0
    # the in-place targets themselves: the view handed in holds the new estimates
    for name in ("rm", "rv"):
        for form, view, buf in S.views_of(args[name], ["last_step2"]):
            call(**dict(args, **{name: view}))
            assert bits_equal(view, want[name]) and S.gaps_intact(buf, view), name
    for bad in (res[:, :8], res.to(BF16 if dtype == F32 else F32)):
        with pytest.raises(_lib.BtxError, match="residual must have x's shape and dtype"):
            call(**dict(args, res=bad))
    _note("batch_norm_train", "res", "wrong shape / dtype", "refused")
    # x in the other format: torch's path
    bn.load_state_dict(state)
    bn.weight, bn.bias = torch.nn.Parameter(state["weight"].clone()), torch.nn.Parameter(state["bias"].clone())
    bn.running_mean, bn.running_var = state["running_mean"].clone(), state["running_var"].clone()
    (_, xv, buf), = S.views_of(x, ["other_format"])
    assert not ag.bn_train_usable(bn, xv)
    with torch.no_grad():
        got = ag.bn_act(bn, xv, residual=res, relu=True)
        bn.load_state_dict(state)
        ref = torch.relu(torch.nn.functional.batch_norm(xv, state["running_mean"].clone(), state["running_var"].clone(), bn.weight, bn.bias,
                                                        True, bn.momentum, bn.eps) + res)
    assert torch.equal(got, ref)
    _note("bn_act", "x", "other_format", "torch's path")
    _covered(seen, "test_batchnorm_training")


# =============================================================================================================================
# 6. pools
# =============================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pools(dtype):
    """maxpool2d_hip, maxpool2d_train_hip, maxpool2d_bwd_hip, avgpool_global_hip at (2, 16, 9, 9), k3 s2 p1: views of x, dy and idx;
    a dy or idx that does not belong to the geometry is refused by name"""
    from bayesian_torch_amd import _lib, functional as BF
    shape, k, s, p = (2, 16, 9, 9), 3, 2, 1
    x = _cl(_ints(shape, 51, dtype, lim=7))
    xf = X_FORMS[4]
    with recording() as seen:
        y = sweep("maxpool2d_hip", lambda x: BF.maxpool2d_hip(x, k, s, p), dict(x=x), dict(x=xf))
        assert torch.equal(y, torch.nn.functional.max_pool2d(x.float(), k, s, p).to(dtype))
        yt, idx = sweep("maxpool2d_train_hip", lambda x: BF.maxpool2d_train_hip(x, k, s, p), dict(x=x), dict(x=xf))
        assert torch.equal(yt, y)
        dy = _cl(_ints(tuple(y.shape), 52, dtype))
        sweep("maxpool2d_bwd_hip", lambda dy, idx: BF.maxpool2d_bwd_hip(dy, idx, shape, k, s, p), dict(dy=dy, idx=idx),
              dict(dy=xf, idx=["last_step2"]))
        sweep("avgpool_global_hip", lambda x: BF.avgpool_global_hip(x), dict(x=x), dict(x=xf))
        for bad_dy, bad_idx in ((dy[:, :, :-1], idx), (dy, idx.to(torch.int32)), (dy, idx[:-1])):
            with pytest.raises(_lib.BtxError, match="dy must be .* and idx the uint8"):
                BF.maxpool2d_bwd_hip(bad_dy, bad_idx, shape, k, s, p)
        _note("maxpool2d_bwd_hip", "dy, idx", "wrong shape / dtype / size", "refused")
    _covered(seen, "test_pools")


# =============================================================================================================================
# 7. Monte-Carlo dropout
# =============================================================================================================================
@pytest.mark.parametrize("mode", ["element", "channel"])
def test_dropout(mode):
    """dropout_hip forward and backward on every form of a channels-last and of an NCHW tensor (bf16 and f32): channels-last and
    NCHW-dense memory run as they are (the mask belongs to the logical element, so the logical values carry the same bits), the rest
    enters as one dense copy.  In place (out = x) on a strided x: written through a dense buffer, the gaps intact."""
    from bayesian_torch_amd import _lib, functional as BF
    T, scale = BF.dropout_params(0.25)
    with recording() as seen:
        for dtype in (F32, BF16):
            for cl in (True, False):
                x = _randn(3, 8, 5, 5, seed=9, dtype=dtype)
                x = _cl(x) if cl else x
                for backward in (False, True):
                    def call(x):
                        return BF.dropout_hip(x, T, scale, mode, 5, 3, 41, backward=backward)
                    want = sweep("dropout_hip", call, dict(x=x), dict(x=X_FORMS[4]),
                                 outcome=lambda form: "as is" if form == "other_format" else "copy")
                assert 0 < int((want == 0).sum()) < want.numel()
                fwd = BF.dropout_hip(x, T, scale, mode, 5, 3, 41)
                for form, view, buf in S.views_of(x, ["batch_step2", "chan_narrow", "other_format"]):
                    r, k = entered(lambda: BF.dropout_hip(view, T, scale, mode, 5, 3, 41, out=view))
                    assert k == {"btx_dropout_fwd"}, k
                    assert r is view and bits_equal(view, fwd) and S.gaps_intact(buf, view), (mode, dtype, cl, form)
                    _note("dropout_hip", "out=x", form, "as is" if form == "other_format" else "through")
                for bad in (torch.empty(3, 8, 5, 4, dtype=dtype, device=_dev()), torch.empty(3, 8, 5, 5, dtype=torch.float64, device=_dev())):
                    with pytest.raises(_lib.BtxError, match="out must be"):
                        BF.dropout_hip(x, T, scale, mode, 5, 3, 41, out=bad)
                _note("dropout_hip", "out", "wrong shape / dtype", "refused")
    _covered(seen, "test_dropout")


# =============================================================================================================================
# 8. loss and evaluation heads
# =============================================================================================================================
HS, HB, HC = 3, 5, 7


def _with_grad(fn, t, *rest):
    """(outputs, gradient of their sum w.r.t. t) with t a leaf that keeps the strides handed in"""
    leaf = t.detach().requires_grad_(True)
    assert leaf.stride() == t.stride()
    out = fn(leaf, *rest)
    outs = [o for o in (out if isinstance(out, (tuple, list)) else [out]) if o is not None]
    sum(o.float().sum() for o in outs if o.requires_grad).backward()
    return [o.detach() for o in outs], leaf.grad


def test_classification_heads():
    """mc_elbo_loss (btx_mc_ce_*), avu_mc, avu, eau: stack / logits as last_step2 and batch_step2, labels as last_step2 and expanded
    — loss and gradient carry the dense call's bits"""
    from bayesian_torch_amd.utils import _calibration as C, mc_loss as M
    stack = _randn(HS, HB, HC, seed=1, scale=2.0)
    labels = torch.full((HB,), 3, dtype=torch.int64, device=_dev())
    kl = torch.tensor([1.5], device=_dev())
    err, unc = _randn(HB * 8, seed=2).abs(), _randn(HB * 8, seed=3).abs()
    lf, sf = ["last_step2", "expanded"], ["last_step2", "batch_step2"]
    with recording() as seen:
        for dtype in (F32, BF16):
            st = stack.to(dtype)
            assert M.hip_usable(st, labels)
            sweep("mc_elbo_loss", lambda stack, labels: _with_grad(lambda s: M.mc_elbo_loss(s, labels, kl=kl), stack),
                  dict(stack=st, labels=labels), dict(stack=sf, labels=lf))
            for area in (False, True):
                sweep("avu_mc", lambda stack, labels: _with_grad(lambda s: C.avu_mc(s, labels, 1.0, 1.0, area), stack),
                      dict(stack=st, labels=labels), dict(stack=sf, labels=lf))
                sweep("avu", lambda logits, labels: _with_grad(lambda s: C.avu(s, labels, 1.0, 1.0, area), logits),
                      dict(logits=st[0].contiguous(), labels=labels), dict(logits=sf, labels=lf))
        for conf in (False, True):
            sweep("eau", lambda error, other: _with_grad(lambda e: C.eau(e, other, 0.5, 0.5, 1.0, conf), error),
                  dict(error=err, other=unc), dict(error=["last_step2"], other=["last_step2"]))
    _covered(seen, "test_classification_heads")


def test_mc_accumulate_and_evaluator():
    """mc.accumulate / accumulate_lanes: logits as last_step2 / batch_step2; the packed vector they add into as last_step2 (written
    through a dense copy, the gaps intact).  mc.Evaluator.update: packed as last_step2, labels as last_step2 and expanded; its state
    is the evaluator's own tensor."""
    from bayesian_torch_amd import mc
    n = mc.packed_numel(HB, HC)
    labels = torch.full((HB,), 2, dtype=torch.int64, device=_dev())
    with recording() as seen:
        for dtype in (F32, BF16):
            lg = _randn(HS * HB, HC, seed=4, scale=2.0, dtype=dtype)

            def one(logits, packed):
                return mc.accumulate(packed.clone() if packed.is_contiguous() else packed, logits, kl=1.5).clone()

            def lanes(logits, packed):
                return mc.accumulate_lanes(packed.clone() if packed.is_contiguous() else packed, logits, HS, kl=1.5).clone()
            start = _randn(n, seed=5).abs()
            sweep("mc.accumulate", one, dict(logits=lg[:HB].contiguous(), packed=start), dict(logits=["last_step2", "batch_step2"],
                                                                                            packed=["last_step2"]),
                  outcome=dict(logits="copy", packed="through"))
            packed = sweep("mc.accumulate_lanes", lanes, dict(logits=lg, packed=torch.zeros(n, device=_dev())),
                           dict(logits=["last_step2", "batch_step2"], packed=["last_step2"]), outcome=dict(logits="copy", packed="through"))

        def ev(packed, labels):
            e = mc.Evaluator(HC, thresholds=[0.5, 1.0], capacity=HB, device=_dev()).update(packed, labels)
            return e.state.clone(), e.records_buffer.clone()
        sweep("Evaluator.update", ev, dict(packed=packed, labels=labels), dict(packed=["last_step2"], labels=["last_step2", "expanded"]))
    _covered(seen, "test_mc_accumulate_and_evaluator")


def test_regression_heads():
    """mc_gaussian_nll, GaussianStats.accumulate_lanes, RegressionEvaluator.update at S = 3, B = 5, D = 2"""
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.utils import mc_loss as M
    D = 2
    stack = _randn(HS, HB, 2 * D, seed=1)
    y = _randn(1, D, seed=2).expand(HB, D).contiguous()
    kl = torch.tensor([0.7], device=_dev())
    st = mc.GaussianStats("log")
    with recording() as seen:
        for dtype in (F32, BF16):
            s = stack.to(dtype)
            assert M.gnll_hip_usable(s, y)
            sweep("mc_gaussian_nll", lambda stack, target: _with_grad(lambda t: M.mc_gaussian_nll(t, target, kl, "moments"), stack),
                  dict(stack=s, target=y), dict(stack=["last_step2", "batch_step2"], target=["last_step2", "expanded"]))

            def acc(out, packed):
                return st.accumulate_lanes(packed.clone() if packed.is_contiguous() else packed, out, HS, kl=1.5).clone()
            packed = sweep("GaussianStats.accumulate_lanes", acc,
                           dict(out=s.reshape(HS * HB, 2 * D), packed=torch.zeros(st.numel(HB, 2 * D), dtype=torch.float64, device=_dev())),
                           dict(out=["last_step2", "batch_step2"], packed=["last_step2"]), outcome=dict(out="copy", packed="through"))

        def ev(packed, target):
            return mc.RegressionEvaluator(D, device=_dev()).update(packed, target).state.clone()
        sweep("RegressionEvaluator.update", ev, dict(packed=packed, target=y), dict(packed=["last_step2"], target=["last_step2", "expanded"]))
    _covered(seen, "test_regression_heads")


# =============================================================================================================================
# 9. KL family
# =============================================================================================================================
def _kl_params():
    """(mu, rho) pairs of 5 and 4097 elements and a [16, 16, 3, 3] parameter stored GEMM-major, with its op"""
    from bayesian_torch_amd import functional as BF
    op = BF.OpDesc(2, 16, 16, 3, 1, 1)
    out = []
    for i, shape in enumerate([(5,), (4097,), (16, 16, 3, 3)]):
        pair = []
        for j in range(2):
            p = (BF.gemm_major_param(shape, op) if len(shape) == 4 else torch.empty(shape)).to(_dev())
            p.copy_(_randn(*shape, seed=10 * i + j, scale=0.3) - (2.0 if j else 0.0))
            pair.append(p)
        out.append(tuple(pair) + (op if len(shape) == 4 else None,))
    return out


def _apply_with_grads(fn, meta, params, *pre):
    leaves = [p.detach().requires_grad_(True) for p in params]
    assert all(l.stride() == p.stride() for l, p in zip(leaves, params))
    kl = fn.apply(meta, *pre, *leaves)
    (1.7 * kl).backward()
    return [kl.detach()] + [l.grad for l in leaves]


def test_kl_family():
    """kl_hip, KlFn / KlMcFn / KlLogUFn (forward and backward) on parameters of 5, 4097 and [16, 16, 3, 3] (GEMM-major) elements:
    once dense, once as views of ONE flat buffer with gaps (the parameters' own strides: read in place, the gaps intact, the same
    bits), once as views that are not dense (one dense copy each, the gradients handed back in the logical shape); tensor priors as
    last_step2"""
    from bayesian_torch_amd import _lib, autograd as ag, functional as BF, priors
    import klmc_model as KM
    pairs = _kl_params()
    dense = [t for mu, rho, _ in pairs for t in (mu, rho)]
    flat, buf = S.flat_with_gaps(dense)
    assert all(v.stride() == t.stride() and v.data_ptr() % 16 == 0 for v, t in zip(flat, dense))
    pmt, pst = _randn(5, seed=90), _randn(5, seed=91).abs() + 0.5
    prior = priors.ScaleMixturePrior(*KM.PRIORS["mix2"][1:])
    with recording() as seen:
        for (mu, rho, _), (fm, fr) in zip(pairs, zip(flat[0::2], flat[1::2])):
            assert bits_equal(BF.kl_hip(fm, fr, 0.0, 1.0), BF.kl_hip(mu, rho, 0.0, 1.0))
        sweep("kl_hip", lambda mu, rho, pm, ps: BF.kl_hip(mu, rho, 0.0, 1.0, pm, ps), dict(mu=pairs[0][0], rho=pairs[0][1], pm=pmt, ps=pst),
              dict(mu=["last_step2"], rho=["last_step2"], pm=["last_step2"], ps=["last_step2"]))
        (_, pmv, b1), = S.views_of(pmt, ["last_step2"])
        (_, psv, b2), = S.views_of(pst, ["last_step2"])
        # not dense at all: every other element of the vectors, every other row of the conv parameter's storage
        sparse = [S.view_of(t, "last_step2" if t.dim() == 1 else "batch_step2") for t in dense]
        runs, kern = {}, {}
        for form, ps_, pm_, ps2 in (("dense", dense, pmt, pst), ("flat", flat, pmv, psv), ("strided", [v for v, _ in sparse], pmt, pst)):
            meta = ((0.0, 1.0, pm_, ps2, None), (0.1, 0.9, None, None, None), (0.0, 1.0, None, None, pairs[2][2]))
            mc_meta = tuple((prior, None, op, 50 + i, _lib.STREAM_KL_W, 3, None) for i, (_, _, op) in enumerate(pairs))
            runs[form], kern[form] = entered(lambda: dict(gauss=_apply_with_grads(ag.KlFn, meta, ps_),
                                                          mc=_apply_with_grads(ag.KlMcFn, mc_meta, ps_, 11, 2),
                                                          logu=_apply_with_grads(ag.KlLogUFn, ("sum", "mean", "sum"), ps_)))
        assert kern["flat"] == kern["dense"] == kern["strided"] and len(kern["dense"]) == 6, kern
        assert bits_equal(runs["flat"], runs["dense"]) and bits_equal(runs["strided"], runs["dense"])
        assert S.gaps_intact_many(buf, flat) and S.gaps_intact(b1, pmv) and S.gaps_intact(b2, psv)
        assert all(S.gaps_intact(b, v) and not S.is_dense_as(v, t) for (v, b), t in zip(sparse, dense))
        for i, n in enumerate(("5", "4097", "16x16x3x3")):
            _note("KlFn / KlMcFn / KlLogUFn", "mu, rho of " + n, "flat, gaps", "as is")
            _note("KlFn / KlMcFn / KlLogUFn", "mu, rho of " + n, "last_step2" if i < 2 else "batch_step2", "copy")
        _note("KlFn", "prior tensors", "last_step2", "copy")
    _covered(seen, "test_kl_family")


def _la_layers(flat):
    """a Linear and a Conv2d LocalReparameterization layer with the log-uniform prior, built alike every time; flat: their parameters
    moved into ONE flat buffer with gaps (their own strides) -> (model, views, buffer)"""
    from bayesian_torch_amd import layers as L, priors
    torch.manual_seed(0)
    net = torch.nn.Sequential(L.LinearLocalReparameterization(37, 6), L.Conv2dLocalReparameterization(16, 16, 3, padding=1)).to(_dev())
    for m in net:
        m.set_prior(priors.LogUniformPrior("sum"))
    views, buf = None, None
    if flat:
        ps = list(net.parameters())
        views, buf = S.flat_with_gaps([p.detach() for p in ps])
        for p, v in zip(ps, views):
            p.data = v
    return net, views, buf


def test_log_alpha_statistics_and_pruning():
    """btx_logalpha_stats / btx_logalpha_prune.  (1) logalpha_stats_hip / logalpha_prune_hip on the (mu, rho) pairs of 5, 4097 and
    [16, 16, 3, 3] (GEMM-major) elements through sparsity._in_place_pair, as sparsity.stats / prune_ hand them over: once dense, once
    as views of ONE flat buffer with gaps — the same counts, the same pruned parameters (written in place, in storage order), the
    gaps intact.  (2) sparsity.stats / prune_ on a Linear + Conv2d model whose parameters are such views.  (3) a (mu, rho) pair
    whose two tensors are stored in DIFFERENT orders has no common element order for the element-wise kernel: stats reads row-major
    copies (the kernel, the same counts), prune_ takes torch's masked_fill through the strides (documented; the same parameters)."""
    from bayesian_torch_amd import functional as BF, sparsity
    pairs = _kl_params()
    dense = [t for mu, rho, _ in pairs for t in (mu, rho)]
    flat, buf = S.flat_with_gaps(dense)
    res = {}
    with recording() as seen:
        for form, ts in (("dense", [t.clone(memory_format=torch.preserve_format) for t in dense]), ("flat", flat)):
            assert all(a.stride() == b.stride() for a, b in zip(ts, dense))
            entries = [sparsity._in_place_pair(mu, rho) for mu, rho in zip(ts[0::2], ts[1::2])]
            assert all(e is not None and e[0].numel() == mu.numel() for e, mu in zip(entries, ts[0::2]))
            (st, pr), k = entered(lambda: (BF.logalpha_stats_hip(entries, (-1.0, 3.0), 8), BF.logalpha_prune_hip(entries, -1.0)))
            assert k == {"btx_logalpha_stats", "btx_logalpha_prune"}
            res[form] = [st, pr] + list(ts)
        assert bits_equal(res["flat"], res["dense"]) and S.gaps_intact_many(buf, flat)
        pruned = res["dense"][1].tolist()
        assert pruned == res["dense"][0][:, 0].tolist(), "prune_ takes what stats counted above the threshold"
        assert 0 < pruned[1] < 4097 and 0 < pruned[2] < 16 * 16 * 9, pruned
        assert not bits_equal(res["dense"][2:], dense), "nothing was pruned"
        for n in ("5", "4097", "16x16x3x3"):
            _note("logalpha_stats_hip / logalpha_prune_hip", "mu, rho of " + n, "flat, gaps", "as is (written in place)")
        # ---- through the public functions, on a model
        (na, _, _), (nb, views, mbuf) = _la_layers(False), _la_layers(True)
        kw = dict(thresholds=(-1.0,), bins=8, include_bias=True)
        sa, ka = entered(lambda: sparsity.stats(na, **kw))
        sb, kb = entered(lambda: sparsity.stats(nb, **kw))
        assert sa == sb and ka == kb == {"btx_logalpha_stats"}
        pa, ka = entered(lambda: sparsity.prune_(na, threshold=-1.0, include_bias=True))
        pb, kb = entered(lambda: sparsity.prune_(nb, threshold=-1.0, include_bias=True))
        assert pa == pb and ka == kb == {"btx_logalpha_prune"} and pa["total"]["pruned"] > 0
        assert bits_equal([p.detach() for p in na.parameters()], [p.detach() for p in nb.parameters()])
        assert S.gaps_intact_many(mbuf, views)
        _note("sparsity.stats / prune_", "mu, rho", "flat, gaps", "as is (written in place)")
        # ---- mu GEMM-major, rho row-major
        (na, _, _), (nc, _, _) = _la_layers(False), _la_layers(False)
        mu, rho = nc[1]._w()
        rho.data = rho.detach().clone(memory_format=torch.contiguous_format)
        assert mu.stride() != rho.stride() and sparsity._in_place_pair(mu, rho) is None
        sc, kc = entered(lambda: sparsity.stats(nc, **kw))
        assert sc == sa and kc == {"btx_logalpha_stats"}
        _note("sparsity.stats", "mu, rho", "different orders", "copy")
        pa = sparsity.prune_(na, threshold=-1.0, include_bias=True)
        pc, kc = entered(lambda: sparsity.prune_(nc, threshold=-1.0, include_bias=True))
        assert pc == pa and kc == {"btx_logalpha_prune"}  # the other three pairs still take the kernel
        assert bits_equal([p.detach() for p in na.parameters()], [p.detach() for p in nc.parameters()])
        _note("sparsity.prune_", "mu, rho", "different orders", "torch's masked_fill through the strides")
    _covered(seen, "test_log_alpha_statistics_and_pruning")


# =============================================================================================================================
# 10. optimizers, gradient bucket
# =============================================================================================================================
def _opt_params(flat):
    from bayesian_torch_amd import functional as BF
    op = BF.OpDesc(2, 16, 16, 3, 1, 1)
    ts = []
    for i, shape in enumerate([(5,), (4097,), (16, 16, 3, 3)]):
        p = (BF.gemm_major_param(shape, op) if len(shape) == 4 else torch.empty(shape)).to(_dev())
        p.copy_(_randn(*shape, seed=20 + i, scale=0.3))
        ts.append(p)
    buf = None
    if flat:
        ts, buf = S.flat_with_gaps(ts)
    return [torch.nn.Parameter(t) for t in ts], buf


def _strided_grads(params, seed):
    """gradients with strides other than their parameter's: last_step2 vectors, a row-major gradient of the GEMM-major parameter"""
    out = []
    for i, p in enumerate(params):
        g = _randn(*p.shape, seed=seed + i)
        if p.dim() == 1:
            (_, v, buf), = S.views_of(g, ["last_step2"])
        else:
            v, buf = g, None
        assert v.stride() != p.stride() and torch.equal(v, g)
        out.append((g, v, buf))
    return out


@pytest.mark.parametrize("name", ["SGD", "Adam"])
def test_optimizers(name):
    """two fused steps with gradient clipping (btx_optim_grad_norm + btx_optim_sgd / _adam).  Parameters as views of one flat buffer
    with gaps (dense, their own strides): updated in place, the gaps intact.  Gradients with other strides than the parameter's
    (optim._plan: staged into the parameter's storage order, one copy): the bits of the step on same-strided gradients, the
    gradient buffers untouched.  A parameter that is not dense is refused by name."""
    from bayesian_torch_amd import optim
    from bayesian_torch_amd._lib import BtxError
    kw = dict(lr=1e-2, max_grad_norm=1.0, **(dict(momentum=0.9) if name == "SGD" else {}))
    res, kern = {}, {}
    with recording() as seen:
        for form in ("dense", "flat", "strided grads"):
            params, buf = _opt_params(form == "flat")
            opt = getattr(optim, name)(params, **kw)
            for step in (1, 2):
                gs = _strided_grads(params, 100 * step)
                for p, (g, v, gb) in zip(params, gs):
                    p.grad = v if form == "strided grads" else torch.empty_like(p).copy_(g)
                _, kern[form] = entered(opt.step)
                assert kern[form] == kern["dense"] and len(kern[form]) == 2, (form, sorted(kern[form]))
                if form == "strided grads":
                    assert all(torch.equal(v, g) and (gb is None or S.gaps_intact(gb, v)) for g, v, gb in gs)
            res[form] = [p.detach().clone() for p in params] + [opt.total_norm.clone()]
            if buf is not None:
                assert S.gaps_intact_many(buf, [p.detach() for p in params])
        assert bits_equal(res["flat"], res["dense"]) and bits_equal(res["strided grads"], res["dense"])
        _note("optim." + name, "parameters", "flat, gaps", "as is (written in place)")
        _note("optim." + name, "gradients", "other strides", "copy")
        (_, pv, pb), = S.views_of(_randn(8, seed=1), ["last_step2"])
        p = torch.nn.Parameter(pv)
        p.grad = torch.ones(8, device=_dev())
        with pytest.raises(BtxError, match="dense GPU parameters"):
            getattr(optim, name)([p], **kw).step()
        assert S.gaps_intact(pb, pv)
        _note("optim." + name, "parameters", "last_step2", "refused")
    _covered(seen, "test_optimizers", but=["btx_optim_adam" if name == "SGD" else "btx_optim_sgd"])


def test_gradient_bucket():
    """parallel.GradReducer.pack / unpack: gradients with other strides than the parameter's are staged (pack) and written back
    through the view (unpack): the bucket and the gradients of the same-strided run, the gaps intact"""
    from bayesian_torch_amd import parallel
    res = {}
    with recording() as seen:
        for form in ("dense", "strided grads"):
            params, _ = _opt_params(False)
            mod = torch.nn.Module()
            mod.ps = torch.nn.ParameterList(params)
            gs = _strided_grads(params, 300)
            for p, (g, v, gb) in zip(params, gs):
                p.grad = v if form == "strided grads" else torch.empty_like(p).copy_(g)
            red = parallel.GradReducer(mod, rank=1, world=3)
            bucket, k1 = entered(lambda: red.pack(torch.tensor(2.5, device=_dev())).clone())
            red.bucket.mul_(3.0)
            _, k2 = entered(red.unpack)
            assert k1 == {"btx_bucket_pack"} and k2 == {"btx_bucket_unpack"}, (form, k1, k2)
            res[form] = [bucket] + [p.grad.detach().clone() for p in params]
            if form == "strided grads":
                assert all(p.grad is v and (gb is None or S.gaps_intact(gb, v)) for p, (g, v, gb) in zip(params, gs))
    assert bits_equal(res["strided grads"], res["dense"])
    _note("GradReducer.pack", "gradients", "other strides", "copy")
    _note("GradReducer.unpack", "gradients", "other strides", "through")
    _covered(seen, "test_gradient_bucket")


# =============================================================================================================================
# 11. INT8
# =============================================================================================================================
def _q(t, s=0.1, z=77):
    from bayesian_torch_amd.q8 import QTensor
    return QTensor(t, s, z)


def test_int8():
    """quantize_act reads x's strides as they are; the uint8 carriers of the contraction (plain and with the fused residual), the
    add and the two pools enter through q8.QTensor, which keeps 4-D carriers channels-last and makes everything else dense: x and
    the residual as batch_step2 / chan_narrow (4-D) and batch_step2 / last_step2 ([B, K]) give the bytes of the dense call"""
    from bayesian_torch_amd import q8
    from test_gpu_alignment import _qt
    from test_gpu_q8_net import CONV_ZO, RES_CONV, res_case
    with recording() as seen:
        for dtype in (F32, BF16):
            xf = _cl(_randn(2, 16, 9, 9, seed=1, dtype=dtype, scale=3.0))
            sweep("q8.quantize_act", lambda x: q8.quantize_act(x, 0.1, 128).int_repr(), dict(x=xf), dict(x=X_FORMS[4]), outcome="as is")
            sweep("q8.quantize_act", lambda x: q8.quantize_act(x, 0.1, 128).int_repr(), dict(x=xf.flatten(1).contiguous()),
                  dict(x=X_FORMS[2]), outcome="as is")
        g = torch.Generator().manual_seed(7)
        xb = _cl(torch.randint(0, 256, (2, 16, 9, 9), generator=g, dtype=U8).to(_dev()))
        yb = _cl(torch.randint(0, 256, (2, 16, 9, 9), generator=g, dtype=U8).to(_dev()))
        u4 = ["batch_step2", "chan_narrow", "other_format"]
        sweep("q8.max_pool2d", lambda x: q8.max_pool2d(_q(x), 3, 2, 1).int_repr(), dict(x=xb), dict(x=u4))
        sweep("q8.avg_pool2d", lambda x: q8.avg_pool2d(_q(x), 3, 1).int_repr(), dict(x=xb), dict(x=u4))
        sweep("q8.add", lambda a, b: q8.add(_q(a), _q(b, 0.2, 90), 0.15, 100, relu=True).int_repr(), dict(a=xb, b=yb), dict(a=u4, b=u4))
        x2, y2 = xb.flatten(1).contiguous(), yb.flatten(1).contiguous()
        sweep("q8.add", lambda a, b: q8.add(_q(a), _q(b, 0.2, 90), 0.15, 100).int_repr(), dict(a=x2, b=y2),
              dict(a=["batch_step2", "last_step2"], b=["batch_step2", "last_step2"]))
        # the contraction, plain and with the fused residual add: the smallest case of tests/test_gpu_q8_net.py
        c = res_case(0, True)
        layer = c["q"].to(_dev())
        s_eps, s_d, s_w = c["chain"]
        noise = dict(eps_w=c["eps"], eps_b=c["eps_b"])
        z_r, z_add = 131, 120
        layer.quant_dict = [(s_eps, 0), (s_d, 0), (s_w, 0), (c["s_x"], c["z_x"]), (c["s_o"], CONV_ZO[z_r])]
        try:
            xq, rq = _qt(c["x_i"], c["s_x"], c["z_x"]).q, _qt(c["res"], c["s_r"], z_r).q

            def plain(x):
                with torch.no_grad():
                    return layer.forward_int8(_q(x, c["s_x"], c["z_x"]), noise=noise).int_repr()

            def fused(x, residual):
                with torch.no_grad():
                    return layer.forward_int8(_q(x, c["s_x"], c["z_x"]), noise=noise, residual=_q(residual, c["s_r"], z_r), add_relu=True,
                                              add_scale=None, add_zero_point=z_add).int_repr()
            sweep("q8 contraction", plain, dict(x=xq), dict(x=["batch_step2", "chan_narrow"]))
            sweep("q8 contraction + residual", fused, dict(x=xq, residual=rq), dict(x=["batch_step2", "chan_narrow"],
                                                                                   residual=["batch_step2", "chan_narrow"]))
            with torch.no_grad():
                layer.forward_int8(_q(xq, c["s_x"], c["z_x"]), sample_idx=3)  # noise from BTX-RNG: btx_q8_sample_weights draws it
        finally:
            layer.quant_dict = None
    _covered(seen, "test_int8")


def test_int8_flipout():
    """btx_q8_sample_delta + btx_q8_contract_flipout on the smallest case of tests/test_gpu_q8_flipout.py, its uint8 input as
    batch_step2 and chan_narrow: every output against the numpy model, as for the dense input"""
    from test_gpu_q8_flipout import _case, _check
    c = _case("conv", "c16n64s2")
    x = _cl(torch.from_numpy(np.ascontiguousarray(c["x_i"])).to(_dev()))
    with recording() as seen:
        _, kernels = entered(lambda: _check(c, float_input=_q(x, *c["e_x"])))
        assert {"btx_q8_sample_delta", "btx_q8_contract_flipout"} <= kernels
        for form, view, buf in S.views_of(x, ["batch_step2", "chan_narrow"]):
            _, k = entered(lambda: _check(c, float_input=_q(view, *c["e_x"])))
            assert k == kernels and S.gaps_intact(buf, view), (form, sorted(k))
            _note("q8 flipout contraction", "x", form, "copy")
    _covered(seen, "test_int8_flipout")


# =============================================================================================================================
# the table itself
# =============================================================================================================================
def test_cover_table_names_tests_of_this_file():
    import sys
    me = sys.modules[__name__]
    for export, tests in STRIDED_COVER.items():
        assert tests or export in NO_STRIDED_INPUT, export
        for t in tests:
            assert callable(getattr(me, t, None)), (export, t)
