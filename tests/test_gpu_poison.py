"""GPU: no kernel result may depend on what a buffer held before the call (DESIGN.md "Memory-content contract").

Every wrapper hands the C entry points memory from `torch.empty`, and about fifteen kernels share the per-(device, stream)
workspace `functional._WS` one after another.  The caching allocator gives a test the block it freed a moment ago, so an output
element nobody wrote, or a workspace word read before it was written, reads back the right value of the previous run.  Here each
call runs three times — plain, with every fresh buffer and workspace filled with 0xFF (NaN / -1), with 0x7F (3.4e38 / 127) —
and everything it returns must have the same bits, whatever is saved for a later call included; the consumer (the backward) then
runs under poison as well.  Values are not verified again: the other files do that.

COVERED / HOST_ONLY / READS_PRIOR_CONTENTS classify every name of `_lib.EXPORTS` (tests/test_poison_cpu.py proves it without a
GPU).  Each test asserts that poison was really applied (bytes > 0) and that every entry point the tables name for it was entered
while poison was active, and prints one line per entry: profiles/poison_coverage.txt holds those of the first full run.
Poison is data only: pool indices are compared with the plain run on the host BEFORE the backward addresses memory with them.
"""
import ctypes
import warnings

import pytest
import torch

import poison as P

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

F32, BF16 = torch.float32, torch.bfloat16
PRECS = [("f32", F32), ("bf16x3", F32), ("bf16", BF16)]

# ---- the classification of _lib.EXPORTS -------------------------------------------------------------------------------------------
# entry point -> the test of this file that runs it under poison
COVERED = {
    "btx_contract_fwd": "test_contraction_plain_entry_and_presampled_tiles",
    "btx_sample_weights": "test_contraction_plain_entry_and_presampled_tiles",
    "btx_sample_weights_lanes": "test_contraction_plain_entry_and_presampled_tiles",
    "btx_contract_fwd_ex": "test_contraction_forward_every_family",
    "btx_rowfuse_pack": "test_contraction_forward_every_family",
    "btx_contract_fwd_lanes": "test_contraction_forward_split_k_lanes_tall_strip_epilogue_and_lrt",
    "btx_lrt_fwd_train": "test_lrt_training_forward_and_backward",
    "btx_lrt_bwd": "test_lrt_training_forward_and_backward",
    "btx_contract_wgrad_ws": "test_backward_of_the_impulse_cases",
    "btx_bias_grad": "test_backward_of_the_impulse_cases",
    "btx_dgrad_weights": "test_backward_of_the_impulse_cases",
    "btx_contract_wgrad": "test_weight_gradient_with_atomics_on_integers",
    "btx_rho_grad": "test_weight_gradient_with_atomics_on_integers",
    "btx_maxpool2d_cl": "test_pools",
    "btx_maxpool2d_cl_train": "test_pools",
    "btx_maxpool2d_cl_bwd": "test_pools",
    "btx_avgpool_global_cl": "test_pools",
    "btx_bn_train_bwd": "test_batchnorm_training",
    "btx_fill_eps": "test_fill_kernels_and_mc_accumulate",
    "btx_fill_sign": "test_fill_kernels_and_mc_accumulate",
    "btx_kl_gauss_model": "test_gaussian_kl",
    "btx_kl_gauss_model_bwd": "test_gaussian_kl",
    "btx_kl_mc_model_bwd": "test_sampled_kl",
    "btx_kl_logu_model_bwd": "test_log_uniform_kl_statistics_and_pruning",
    "btx_logalpha_stats": "test_log_uniform_kl_statistics_and_pruning",
    "btx_logalpha_prune": "test_log_uniform_kl_statistics_and_pruning",
    "btx_avu_fwd": "test_calibration_heads",
    "btx_avu_bwd": "test_calibration_heads",
    "btx_eau_fwd": "test_calibration_heads",
    "btx_eau_bwd": "test_calibration_heads",
    "btx_mc_ce_fwd": "test_mc_loss_heads",
    "btx_mc_ce_bwd": "test_mc_loss_heads",
    "btx_avu_mc_fwd": "test_mc_loss_heads",
    "btx_avu_mc_bwd": "test_mc_loss_heads",
    "btx_mc_gnll_fwd": "test_regression_heads_and_evaluator",
    "btx_mc_gnll_bwd": "test_regression_heads_and_evaluator",
    "btx_lstm_fwd": "test_lstm",
    "btx_lstm_fwd_train": "test_lstm",
    "btx_lstm_bwd": "test_lstm",
    "btx_optim_grad_norm": "test_optimizers_and_gradient_norm",
    "btx_bucket_pack": "test_gradient_bucket",
    "btx_bucket_unpack": "test_gradient_bucket",
    "btx_q8_quantize_act": "test_int8",
    "btx_q8_sample_weights": "test_int8",
    "btx_q8_contract": "test_int8",
    "btx_q8_contract_res": "test_int8",
    "btx_q8_add": "test_int8",
    "btx_q8_maxpool2d_cl": "test_int8",
    "btx_q8_avgpool2d_cl": "test_int8",
    "btx_q8_sample_delta": "test_int8",
    "btx_q8_contract_flipout": "test_int8",
}
# queries answered on the host: no device memory is touched
HOST_ONLY = (
    "btx_abi_version", "btx_strerror", "btx_contract_plan_info", "btx_contract_pool_shape", "btx_out_shape",
    "btx_kl_workspace_bytes", "btx_kl_model_workspace_bytes", "btx_contract_workspace_bytes", "btx_sampled_w_bytes",
    "btx_sampled_w_bytes_lanes", "btx_bn_workspace_bytes", "btx_wgrad_workspace_bytes", "btx_lstm_workspace_bytes",
    "btx_lstm_train_saved_bytes", "btx_lstm_train_workspace_bytes", "btx_calib_workspace_bytes", "btx_q8_weight_row_bytes",
    "btx_optim_grad_norm_workspace_bytes", "btx_mcloss_workspace_bytes", "btx_bias_grad_workspace_bytes",
    "btx_mc_eval_workspace_bytes", "btx_mc_gnll_workspace_bytes", "btx_reg_eval_workspace_bytes", "btx_lrt_bwd_workspace_bytes",
    "btx_kl_mc_workspace_bytes", "btx_kl_logu_workspace_bytes", "btx_mc_packed_floats", "btx_mc_eval_state_doubles",
)
# entry points that by their contract (include/btx.h) read what one of their arguments held before the call: that argument is an
# input here; their workspace and the outputs they do write are covered by the test named.  name -> (reason, test)
READS_PRIOR_CONTENTS = {
    "btx_kl_gauss": ("btx.h K1: kl_out += with BTX_FLAG_KL_ACCUM (overwritten without it)", "test_gaussian_kl"),
    "btx_kl_mc_model": ("btx.h BTX-KLMC v1: kl_out += with BTX_FLAG_KL_ACCUM (overwritten without it)", "test_sampled_kl"),
    "btx_kl_logu_model": ("btx.h BTX-SVD v1: 'kl_out overwritten, or += with BTX_FLAG_KL_ACCUM'",
                          "test_log_uniform_kl_statistics_and_pruning"),
    "btx_mc_accumulate": ("btx.h K6: 'The buffer is accumulated in place (zero it first)'", "test_fill_kernels_and_mc_accumulate"),
    "btx_mc_accumulate_lanes": ("btx.h K6: the packed buffer of btx_mc_accumulate, accumulated in place",
                                "test_fill_kernels_and_mc_accumulate"),
    "btx_mc_moments_lanes": ("btx.h BTX-REG v1: the float64 packed sums are accumulated in place",
                             "test_regression_heads_and_evaluator"),
    "btx_bn_train_fwd": ("btx.h: running_mean / running_var are updated in place from their old values (momentum)",
                         "test_batchnorm_training"),
    "btx_optim_sgd": ("btx.h BTX-OPT v1: parameters and the momentum buffer are optimizer state, updated in place",
                      "test_optimizers_and_gradient_norm"),
    "btx_optim_adam": ("btx.h BTX-OPT v1: parameters, exp_avg and exp_avg_sq are optimizer state, updated in place",
                       "test_optimizers_and_gradient_norm"),
    "btx_mc_eval": ("btx.h BTX-EVAL v1: 'state (float64, accumulated in place: zero it to reset ...)'", "test_mc_evaluator"),
    "btx_reg_eval_update": ("btx.h BTX-REG v1: 'state, accumulated in place (zero it to reset ...)'",
                            "test_regression_heads_and_evaluator"),
}


def entries_of(test_name):
    """the entry points the tables name for one test"""
    return sorted([e for e, t in COVERED.items() if t == test_name] + [e for e, (_, t) in READS_PRIOR_CONTENTS.items() if t == test_name])


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


class Run:
    """the three-way runs of one test: collects what was poisoned and which entry points ran while poison was active"""

    def __init__(self, test_name):
        self.name, self.calls, self.tensors, self.bytes, self.cases = test_name, set(), 0, 0, 0

    def poisoned(self, byte):
        return _Active(self, byte)

    def three(self, tag, fn, finite=True):
        """fn() -> tensors (nested): plain, under 0xFF and under 0x7F; the bits must agree -> the plain result"""
        clean = fn()
        torch.cuda.synchronize()
        for byte in P.PATTERNS:
            with self.poisoned(byte):
                got = fn()
                torch.cuda.synchronize()
            assert P.bits_equal(got, clean), "%s: the result under %#04x poison differs from the plain run: %s" % (
                tag, byte, _first_difference(got, clean))
        if finite:
            assert not P.any_nan(clean), "%s: NaN in a result of finite inputs" % tag
        self.cases += 1
        return clean

    def done(self):
        names = entries_of(self.name)
        assert names, "no entry point names %s" % self.name
        assert self.bytes > 0 and self.tensors > 0, "%s: nothing was poisoned" % self.name
        missing = [e for e in names if e not in self.calls]
        assert not missing, "%s: never entered while poison was active: %s" % (self.name, missing)
        for e in names:
            print("%s: %d buffers, %d bytes poisoned, patterns ff/7f: equal" % (e, self.tensors, self.bytes))


class _Active:
    def __init__(self, run, byte):
        self.run, self.cm = run, P.poisoned(byte)

    def __enter__(self):
        self.rec = self.cm.__enter__()
        return self.rec

    def __exit__(self, *exc):
        out = self.cm.__exit__(*exc)
        self.run.calls.update(self.rec.calls)
        self.run.tensors += self.rec.tensors
        self.run.bytes += self.rec.bytes
        return out


def _first_difference(a, b):
    la, lb = P._leaves(a), P._leaves(b)
    for i, (x, y) in enumerate(zip(la, lb)):
        if not P.bits_equal(x, y):
            if x is None or y is None:
                return "leaf %d: None against a tensor" % i
            if x.shape != y.shape or x.dtype != y.dtype:
                return "leaf %d: %s %s against %s %s" % (i, tuple(x.shape), x.dtype, tuple(y.shape), y.dtype)
            xf, yf = x.detach().contiguous().reshape(-1), y.detach().contiguous().reshape(-1)
            bad = (P._raw(x).reshape(xf.numel(), -1) != P._raw(y).reshape(yf.numel(), -1)).any(1).nonzero().reshape(-1)
            k = int(bad[0])
            return "leaf %d (%s %s): %d of %d elements, the first at flat index %d: %r against %r" % (
                i, tuple(x.shape), x.dtype, bad.numel(), xf.numel(), k, xf[k].item(), yf[k].item())
    return "%d against %d leaves" % (len(la), len(lb))


def _x_of(xs, act, seed=17, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*xs, generator=g) * scale).to(_dev()).to(act)
    return x.contiguous(memory_format=torch.channels_last) if len(xs) == 4 else x


def _geom(op, nb, spatial):
    from bayesian_torch_amd import _lib
    g = _lib.Geom()
    g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.od, g.oh, g.ow = op.output_padding
    g.groups = op.groups
    return g


# ---- 0. the negative control: the helper catches a torch-only function on the device --------------------------------------------------
def test_negative_control_a_skipped_element_is_caught_on_the_device():
    """no library kernel: a function that leaves the last element of a torch.empty device tensor unwritten gives three different
    results; the same function writing everything gives three equal ones"""
    dev = _dev()
    src = torch.arange(1.0, 1025.0, device=dev)

    def leaky(full):
        out = torch.empty(1024, device=dev)
        n = 1024 if full else 1023
        out[:n] = src[:n] * 2.0
        return out
    seen = []
    for byte in P.PATTERNS:
        with P.poisoned(byte) as rec:
            got = leaky(False)
            ok = leaky(True)
        assert rec.bytes >= 2 * 4096 and rec.tensors == 2
        assert P.bits_equal(ok, src * 2.0)
        assert not P.bits_equal(got, src * 2.0), "a skipped element went unnoticed under %#04x" % byte
        seen.append(got[-1:].clone())
    assert bool(torch.isnan(seen[0]).all()) and float(seen[1]) > 3e38
    assert not hasattr(torch.empty, "__wrapped__")  # restored
    print("negative control: 2 buffers, 8192 bytes poisoned, patterns ff/7f: caught")


# ---- 1. contraction forward ------------------------------------------------------------------------------------------------------
def _fwd(layer, x, sample, gather=False, epilogue=None):
    with torch.no_grad():
        return layer._forward_hip(x, sample_idx=sample, gather=gather, epilogue=epilogue)


def test_contraction_forward_every_family():
    """one row per fast family of test_gpu_fuse_model.CASES at f32, bf16x3 and bf16; the stem rows also with the activation type the
    MFMA type does not imply (the OUT_BF16 / OUT_F32 store); the stem + max-pool launch"""
    from bayesian_torch_amd import _lib
    import test_gpu_fuse_model as FM
    run = Run("test_contraction_forward_every_family")
    families = set()
    for cls, kw, xs, gather in FM.CASES:
        stem = kw.get("in_channels", 99) <= 4
        for prec, act in PRECS:
            layer = FM._layer(cls, kw, prec)
            rc, fam, _ = FM._plan(layer, xs, prec, gather=gather)
            assert rc == 0
            families.add(fam)
            acts = [act] + ([BF16 if act is F32 else F32] if stem else [])  # prec f32 + bf16 x: OUT_BF16; prec bf16 + f32 x: OUT_F32
            for a in acts:
                x = _x_of(xs, a)
                run.three("%s %s %s %s" % (cls, xs, prec, a), lambda: _fwd(layer, x, 5, gather=gather))
    # the stem with the max-pool in its store
    cls, kw, xs, _ = FM.CASES[-1]
    layer = FM._layer(cls, kw, "bf16")
    x = _x_of(xs, BF16)
    assert layer.pool_fusable(x)
    ep = _lib.Epilogue()
    ep.pool, ep.relu = 1, 1
    rc, fam, _ = FM._plan(layer, tuple(x.shape), "bf16", ep=ep)
    assert rc == 0
    families.add(fam)
    g = torch.Generator().manual_seed(18)
    scale, shift = (torch.rand(64, generator=g) * 4 + 2).to(_dev()), torch.randn(64, generator=g).to(_dev())
    run.three("stem + max-pool", lambda: _fwd(layer, x, 4, epilogue=dict(scale=scale, shift=shift, relu=1, pool=True)))
    assert {"gather", "regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem", "stem_pool"} <= families, families
    run.done()


def test_contraction_forward_split_k_lanes_tall_strip_epilogue_and_lrt():
    """a K split (partials in the shared workspace + the reduce launch), a 2-lane launch of every family, a tall-strip tile whose rows
    do not divide the map, residual + ReLU in the store, and the local reparameterization kind"""
    import bayesian_torch_amd as bt
    import test_gpu_fuse_model as FM
    import test_gpu_lanes as LN
    import test_gpu_lrt as LR
    run = Run("test_contraction_forward_split_k_lanes_tall_strip_epilogue_and_lrt")
    split = [c for c in FM.CASES if c[1].get("in_features") == 256][0]
    for prec, act in PRECS:
        layer = FM._layer(split[0], split[1], prec)
        rc, _, ks = FM._plan(layer, split[2], prec)
        assert rc == 0 and ks > 1, (prec, ks)  # btx_contract_plan_info: ksplits > 1
        x = _x_of(split[2], act)
        run.three("split-K %s" % prec, lambda: _fwd(layer, x, 5))
    # 2 lanes; residual + ReLU
    for cls, kw, xs, gather in FM.CASES:
        stem = kw.get("in_channels", 99) <= 4
        nout = kw.get("out_channels", kw.get("out_features"))
        for prec, act in PRECS:
            layer = FM._layer(cls, kw, prec)
            x1 = _x_of(xs, act)
            x2 = torch.cat([x1, _x_of(xs, act, seed=19)], 0)
            if x2.dim() == 4:
                x2 = x2.contiguous(memory_format=torch.channels_last)
            g = torch.Generator().manual_seed(18)
            scale, shift = (torch.rand(nout, generator=g) * 4 + 2).to(_dev()), torch.randn(nout, generator=g).to(_dev())
            base = _fwd(layer, x1, 5)
            res = None
            if not stem:
                res = (torch.randn(base.shape, generator=g) * 4).to(_dev()).to(act)
                if base.dim() == 4:
                    res = res.contiguous(memory_format=torch.channels_last)
            ep = dict(scale=scale, shift=shift, residual=res, relu=1)
            run.three("epilogue %s %s %s" % (cls, xs, prec), lambda: _fwd(layer, x1, 5, gather=gather, epilogue=ep))

            def lanes():
                bt.set_sample_lanes(layer, [5, 11], batch=xs[0])
                try:
                    return _fwd(layer, x2, None, gather=gather)
                finally:
                    bt.set_sample_lanes(layer, None)
            run.three("2 lanes %s %s %s" % (cls, xs, prec), lanes)
    # tall strip: the smallest row of test_tall_strip_tiles_vs_oracle_chain
    cin, cout, hw, bs = min(LN.test_tall_strip_tiles_vs_oracle_chain.pytestmark[0].args[1], key=lambda c: c[3] * c[2] * c[2] * c[0])
    for prec, act in PRECS:
        layer = LN._layer("Conv2dFlipout", dict(in_channels=cin, out_channels=cout, kernel_size=3, padding=1, bias=True), prec, seed=5)
        x = _x_of((bs, cin, hw, hw), act)
        run.three("tall strip %dx%d %s" % (hw, hw, prec), lambda: _fwd(layer, x, 9))
    # BTX_KIND_LRT
    for name, cls, kw, xs, _ in (LR.CASES[0], LR.CASES[2], LR.CASES[4]):
        for prec, act in LR.PRECS:
            layer = LR._make(cls, kw, prec)
            x = LR._x(xs, act)
            run.three("lrt %s %s" % (name, prec), lambda: _fwd(layer, x, 3))
    run.done()


def test_contraction_plain_entry_and_presampled_tiles():
    """btx_contract_fwd itself (the wrappers go through _ex / _lanes) on the split-K Linear case, and the pre-sampled weight tiles of
    btx_sample_weights / _lanes: the tile buffers hold padding, so what is compared is the forward that consumes them"""
    from bayesian_torch_amd import _lib, functional as BF, rng
    import test_gpu_backward as BW
    import test_gpu_fuse_model as FM
    run = Run("test_contraction_plain_entry_and_presampled_tiles")
    L = _lib.lib()
    dev = _dev()
    split = [c for c in FM.CASES if c[1].get("in_features") == 256][0]
    for prec, act in PRECS:
        layer = FM._layer(split[0], split[1], prec)
        op = layer._op
        x = _x_of(split[2], act)
        mu, rho = layer._w()
        mu_p, rho_p = BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op)
        g = _geom(op, x.shape[0], (1, 1, 1))
        a, pc = (_lib.ACT_BF16 if act is BF16 else _lib.ACT_F32), _lib.PREC_CODE[prec]

        def plain():
            stream = torch.cuda.current_stream(dev).cuda_stream
            need = L.btx_contract_workspace_bytes(ctypes.byref(g), _lib.KIND_FLIPOUT, a, pc, 0)
            assert need > 0
            ws = BF._workspace(dev, need, stream)
            out = torch.empty((x.shape[0], op.out_channels), dtype=act, device=dev)
            r = _lib.Rng(rng.seed(), 5, layer._btx_layer_id, None)
            _lib.check(L.btx_contract_fwd(_lib.KIND_FLIPOUT, ctypes.byref(g), x.data_ptr(), mu_p.data_ptr(), rho_p.data_ptr(),
                                          layer.mu_bias.data_ptr(), layer.rho_bias.data_ptr(), out.data_ptr(), ctypes.byref(r), None,
                                          a, pc, 0, ws.data_ptr(), ws.numel(), stream))
            return out
        run.three("btx_contract_fwd %s" % prec, plain)
    # pre-sampled tiles: a 3x3 layer of test_gpu_backward.CASES
    cls, kw, xs = BW.CASES[4]
    for prec, act in PRECS:
        layer = FM._layer(cls, kw, prec)
        op, kind = layer._op, _lib.KIND_FLIPOUT
        mu, rho = layer._w()
        mu_p, rho_p = BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op)
        x1 = _x_of(xs, act)
        x2 = torch.cat([x1, _x_of(xs, act, seed=19)], 0).contiguous(memory_format=torch.channels_last)
        pc = _lib.PREC_CODE[prec]

        def single():
            wg = BF._weight_geom(op)
            nbytes = L.btx_sampled_w_bytes(ctypes.byref(wg), kind, pc)
            assert nbytes > 0
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            arr = (_lib.SampleItem * 1)()
            arr[0].geom = ctypes.pointer(wg)
            arr[0].mu_w, arr[0].rho_w, arr[0].out = mu_p.data_ptr(), rho_p.data_ptr(), buf.data_ptr()
            arr[0].kind, arr[0].layer_id = kind, layer._btx_layer_id & 0xFFFFFFFF
            r = _lib.Rng(rng.seed(), 7, 0, None)
            _lib.check(L.btx_sample_weights(arr, 1, ctypes.byref(r), pc, torch.cuda.current_stream(dev).cuda_stream))
            with torch.no_grad():
                return BF.contract_hip(kind, x1, mu_p, rho_p, None, None, op, rng.seed(), 7, layer._btx_layer_id, prec=prec, sampled_w=buf)

        def lanes():
            bufs = BF.sample_weights([(kind, op, mu_p, rho_p, layer._btx_layer_id)], rng.seed(), 7, prec, dev, lanes=2)
            with torch.no_grad():
                return BF.contract_hip(kind, x2, mu_p, rho_p, None, None, op, rng.seed(), 7, layer._btx_layer_id, prec=prec,
                                       sampled_w=bufs[0], lanes=2, lane_batch=xs[0])
        run.three("btx_sample_weights %s" % prec, single)
        run.three("btx_sample_weights_lanes %s" % prec, lanes)
    run.done()


def test_lrt_training_forward_and_backward():
    """btx_lrt_fwd_train returns out and the saved root; btx_lrt_bwd consumes root and draws its scratch from the shared workspace"""
    import bayesian_torch_amd as bt
    import test_gpu_lrt_train as LT
    run = Run("test_lrt_training_forward_and_backward")
    for name, cls, kw, xs in LT.CASES:
        for prec, act in LT.PRECS:
            layer = LT._make(cls, kw, prec)
            x = LT._t(xs, act, seed=11)
            with torch.no_grad():
                oshape = tuple(layer._forward_hip(x, sample_idx=LT.SAMPLE).shape)
            gy = LT._t(oshape, act, seed=12, scale=1.0)

            def step():
                for p in layer.parameters():
                    p.grad = None
                x1 = x.detach().requires_grad_()
                bt.set_sample_index(layer, LT.SAMPLE)
                out = layer(x1)
                root = out.grad_fn.saved_tensors[1]
                assert root.dtype == F32 and root.numel() == out.numel()
                out.backward(gy)
                mu, rho = layer._w()
                return (out.detach(), root.detach().clone(), x1.grad, mu.grad, rho.grad,
                        layer.mu_bias.grad if layer.mu_bias is not None else None, layer.rho_bias.grad if layer.mu_bias is not None else None)
            run.three("lrt train %s %s" % (name, prec), step)
    run.done()


# ---- 2. backward -------------------------------------------------------------------------------------------------------------------
def _bwd(layer, x, dy, sample):
    import bayesian_torch_amd as bt
    for p in layer.parameters():
        p.grad = None
    x1 = x.detach().requires_grad_(True)
    bt.set_sample_index(layer, sample)
    out = layer(x1, return_kl=False)
    out.backward(dy)
    mu, rho = layer._w()
    return (out.detach(), x1.grad, mu.grad, rho.grad, layer.mu_bias.grad if layer.mu_bias is not None else None,
            layer.rho_bias.grad if layer.mu_bias is not None else None)


def test_backward_of_the_impulse_cases():
    """IMPULSE_BWD of test_gpu_elementwise.py (stride-2 parity-major and transposed layers included) through autograd: the data
    gradient (btx_dgrad_weights + the transposed contraction), the weight gradient on the slab path with the rho fold, the bias
    gradients of btx_bias_grad; in bf16 the 64 -> 64 3x3 row takes the all-taps weight-gradient kernel"""
    import bayesian_torch_amd as bt
    import test_gpu_alignment as TA
    import test_gpu_elementwise as EW
    run = Run("test_backward_of_the_impulse_cases")
    routes = set()
    try:
        for cls, kw, xs in EW.IMPULSE_BWD:
            for prec, act in (("f32", F32), ("bf16", BF16)):
                if prec == "bf16" and not cls.startswith("Conv2d"):
                    continue
                bt.set_precision(prec)
                layer = EW._make(cls, kw, None, seed=0, bt_seed=123)
                x = _x_of(xs, act, seed=1, scale=1.0)
                bt.set_sample_index(layer, 5)
                with torch.no_grad():
                    oshape = tuple(layer(x, return_kl=False).shape)
                dy = _x_of(oshape, act, seed=2, scale=1.0)
                if len(xs) == 4 and not layer._op.transposed:
                    routes.add(TA._wgrad_route(layer, xs, oshape, act, layer.mu_bias is not None)[0])
                run.three("backward %s %s" % (EW._tag(cls, kw, xs), prec), lambda: _bwd(layer, x, dy, 5))
    finally:
        bt.set_precision("f32")
    assert {"taps3", "fast", "f32"} <= routes, routes  # the all-taps kernel, the vectorised bf16 kernel and the f32 one all ran
    run.done()


def test_weight_gradient_with_atomics_on_integers():
    """WGRAD_ATOMICS: btx_contract_wgrad adds the pixel chunks with f32 atomics into outputs the call itself clears; small-integer x
    and dy make every order of additions give the same bits.  btx_rho_grad on the finished gradient."""
    from bayesian_torch_amd import _lib, functional as BF, rng
    import envelope as E
    import test_gpu_elementwise as EW
    run = Run("test_weight_gradient_with_atomics_on_integers")
    BF.WGRAD_ATOMICS = True
    try:
        for cls, kw, xs in EW.IMPULSE_BWD:
            if "Transpose" in cls:  # (ContractFn.backward hands those over on the plain geometry with x and dy exchanged)
                continue
            kw = dict(kw, bias=True)
            layer = EW._make(cls, kw, None)
            op = EW._op_of(layer)
            with torch.no_grad():
                oshape = tuple(E.contract(torch.zeros((1,) + tuple(xs[1:])), layer._w()[0].detach().float().cpu(), None, op).shape)
            oshape = (xs[0],) + oshape[1:]
            for act in (F32, BF16):
                x, dy = E.small_ints(xs, 31).to(_dev()).to(act), E.small_ints(oshape, 32).to(_dev()).to(act)
                if len(xs) == 4:
                    x, dy = x.contiguous(memory_format=torch.channels_last), dy.contiguous(memory_format=torch.channels_last)
                run.three("atomics %s %s" % (EW._tag(cls, kw, xs), act), lambda: EW._wgrad_like_autograd(layer, x, dy, 4, bias=True))
        # the rho fold on the atomics path: btx_rho_grad (dW exact, the product element-wise)
        cls, kw, xs = EW.IMPULSE_BWD[2]
        layer = EW._make(cls, dict(kw, bias=True), None, seed=0, bt_seed=123)
        op = layer._op
        mu, rho = layer._w()
        x = E.small_ints(xs, 31).to(_dev()).to(BF16).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            oshape = tuple(layer._forward_hip(x, sample_idx=5).shape)
        dy = E.small_ints(oshape, 32).to(_dev()).to(BF16).contiguous(memory_format=torch.channels_last)
        rho_f = BF.gemm_major_view(rho, op).reshape(-1)
        kind = _lib.KIND_FLIPOUT if layer._family == "flipout" else _lib.KIND_REPARAM
        run.three("atomics with the rho fold", lambda: BF.wgrad_hip(kind, x, dy, op, rng.seed(), 5, layer._btx_layer_id, tuple(mu.shape),
                                                                     bias=True, raw=True, rho_flat=rho_f))
        dw = E.small_ints((rho_f.numel(),), 33).to(_dev())
        run.three("btx_rho_grad", lambda: BF.rho_grad_hip(dw, rho_f, rng.seed(), 5, layer._btx_layer_id, _lib.STREAM_EPS_W))
    finally:
        BF.WGRAD_ATOMICS = False
    run.done()


# ---- 3. reductions and small kernels -----------------------------------------------------------------------------------------------
BN_SHAPES = [((2, 8), F32), ((2, 8), BF16), ((3, 2040), F32), ((3, 2040), BF16), ((5, 40, 3, 7), F32), ((5, 40, 3, 7), BF16),
             ((1, 72, 33, 31), F32), ((1, 72, 33, 31), BF16), ((257, 1024), F32), ((256, 1024), BF16), ((2, 16, 3, 5, 7), F32),
             ((2, 16, 3, 5, 7), BF16)]


def test_batchnorm_training():
    """btx_bn_train_fwd / _bwd on shapes of test_gpu_reductions.BN_SHAPES, plain and with residual + ReLU: y, save_mean, save_invstd,
    the running estimates (an input: a fresh module per run), dx, dgamma, dbeta, dres; the partials live in the shared workspace"""
    import test_gpu_reductions as RD
    table = {(tuple(p.values[0]), p.values[1]) for p in RD.BN_SHAPES}
    run = Run("test_batchnorm_training")
    for shape, dtype in BN_SHAPES:
        assert (shape, dtype) in table
        x, dy, res = RD._bn_gauss(shape, dtype, 101)
        for relu in (False, True):
            def call():
                bn = RD._bn_module(shape, dtype)
                r = RD._bn_call(bn, x, dy, res if relu else None, relu)
                return {k: v for k, v in r.items() if v is not None}
            run.three("bn %s %s relu=%s" % (shape, dtype, relu), call)
    run.done()


def test_pools():
    """the max-pool (inference, training and backward forms) on the small shapes of test_hip_maxpool_under_autograd_equals_torch and
    the global average pool on shapes of test_avgpool_global_is_exact_on_small_integers.  The index buffer is compared with the plain
    run's on the host before the backward addresses memory with it."""
    from bayesian_torch_amd import functional as BF
    import envelope as E
    import test_gpu_backward as BW
    run = Run("test_pools")
    cases = [c for c in BW.test_hip_maxpool_under_autograd_equals_torch.pytestmark[0].args[1] if c[0][0] * c[0][1] * c[0][2] * c[0][3] < 10 ** 5]
    assert len(cases) == 4
    for shape, dtype, k, s, p in cases:
        x = E.small_ints(shape, 51).to(dtype).to(_dev()).contiguous(memory_format=torch.channels_last)  # integers: most windows tie
        run.three("maxpool %s" % (shape,), lambda: BF.maxpool2d_hip(x, k, s, p))
        y0, idx0 = BF.maxpool2d_train_hip(x, k, s, p)
        dy = E.small_ints(tuple(y0.shape), 52).to(dtype).to(_dev()).contiguous(memory_format=torch.channels_last)
        dx0 = BF.maxpool2d_bwd_hip(dy, idx0, tuple(shape), k, s, p)
        torch.cuda.synchronize()
        for byte in P.PATTERNS:
            with run.poisoned(byte):
                y, idx = BF.maxpool2d_train_hip(x, k, s, p)
                torch.cuda.synchronize()
                # on the host first: a buffer that still held poison would be an address in the backward
                assert P.bits_equal(idx.cpu(), idx0.cpu()) and P.bits_equal(y, y0), "maxpool train %s under %#04x" % (shape, byte)
                dx = BF.maxpool2d_bwd_hip(dy, idx, tuple(shape), k, s, p)
                torch.cuda.synchronize()
            assert P.bits_equal(dx, dx0), "maxpool bwd %s under %#04x: %s" % (shape, byte, _first_difference(dx, dx0))
        assert not P.any_nan((y0, dx0))
    for hw in (1, 33, 1000):
        for C in (8, 72, 136):
            x = E.small_ints((3, hw, C), 600 + hw + C + 3)
            for dtype in (F32, BF16):
                xd = x.permute(0, 2, 1).reshape(3, C, hw, 1).to(dtype).to(_dev())
                run.three("avgpool HW=%d C=%d" % (hw, C), lambda: BF.avgpool_global_hip(xd))
    run.done()


def test_fill_kernels_and_mc_accumulate():
    """btx_fill_eps / btx_fill_sign write fresh buffers; btx_mc_accumulate / _lanes add into a packed buffer that the caller zeroes (an
    input here): a row of test_mc_accumulate_every_entry_against_float64_softmax and one of ..._lanes_against_float64"""
    from bayesian_torch_amd import _lib, functional as BF, mc
    import test_gpu_reductions as RD
    run = Run("test_fill_kernels_and_mc_accumulate")
    dev = _dev()
    for n in (1, 4097):
        run.three("fill_eps n=%d" % n, lambda: BF.fill_eps_hip(n, dev, 77, 5, 3, _lib.STREAM_EPS_W))
        run.three("fill_sign n=%d" % n, lambda: BF.fill_sign_hip(n, dev, 77, 5, 3, _lib.STREAM_SIGN_IN))
    for lanes, bs, C, dtype in ((1, 3, 257, F32), (1, 1, 4099, BF16), (2, 3, 1000, F32), (17, 1, 1000, BF16)):
        lg = RD._mc_logits(lanes, bs, C, 300 + lanes + bs, dtype).reshape(lanes * bs, C).to(dev)

        def acc():
            packed = torch.zeros(mc.packed_numel(bs, C), dtype=F32, device=dev)
            if lanes == 1:
                mc.accumulate(packed, lg, kl=1.5)
            else:
                mc.accumulate_lanes(packed, lg, lanes, kl=1.5)
            return packed
        run.three("mc accumulate lanes=%d bs=%d C=%d" % (lanes, bs, C), acc)
    run.done()


def _kl_pair(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g).to(_dev()), (torch.rand(n, generator=g) * 12 - 9).to(_dev()))


def test_gaussian_kl():
    """btx_kl_gauss, btx_kl_gauss_model and its backward on two items of 1 and 4097 elements; the block partials live in the shared
    workspace.  With BTX_FLAG_KL_ACCUM the scalar is an input (READS_PRIOR_CONTENTS): it starts from 2.5 in every run."""
    from bayesian_torch_amd import functional as BF
    run = Run("test_gaussian_kl")
    items = [_kl_pair(1, 501), _kl_pair(4097, 502)]
    entries = [(mu, rho, 0.1, 0.7, None, None) for mu, rho in items]
    gout = torch.tensor(1.7, device=_dev())
    for mu, rho in items:
        run.three("kl_gauss n=%d" % mu.numel(), lambda: BF.kl_hip(mu, rho, 0.1, 0.7))
        run.three("kl_gauss accumulate n=%d" % mu.numel(),
                  lambda: BF.kl_hip(mu, rho, 0.1, 0.7, out=torch.full((), 2.5, device=_dev()), accumulate=True))

    def model():
        kl = BF.kl_model_hip(entries)
        grads = [(torch.empty_like(mu), torch.empty_like(rho)) for mu, rho in items]
        BF.kl_model_bwd_hip(entries, grads, gout)
        return kl, grads
    run.three("kl_gauss_model", model)
    run.done()


def test_sampled_kl():
    """btx_kl_mc_model / _bwd (BTX-KLMC v1), two items of 1 and 4097 elements, one with a tensor location"""
    from bayesian_torch_amd import _lib, functional as BF
    import test_gpu_klmc as KT
    run = Run("test_sampled_kl")
    ts = [KT._tensors(1, 3, False), KT._tensors(4097, 4, True)]
    entries = [(mu, rho, loc, KT._prior("mix2" if i == 0 else "student"), 40 + i, _lib.STREAM_KL_W, 5, None) for i, (mu, rho, loc) in enumerate(ts)]
    gout = torch.tensor(KT.G, device=_dev())

    def call(accumulate):
        out = torch.full((), 2.5, device=_dev()) if accumulate else None
        kl = BF.kl_mc_model_hip(entries, KT.SEED, 2, out=out, accumulate=accumulate)
        grads = [(torch.empty_like(e[0]), torch.empty_like(e[0])) for e in entries]
        BF.kl_mc_model_bwd_hip(entries, grads, KT.SEED, 2, gout)
        return kl, grads
    run.three("kl_mc_model", lambda: call(False))
    run.three("kl_mc_model accumulate", lambda: call(True))
    run.done()


def test_log_uniform_kl_statistics_and_pruning():
    """btx_kl_logu_model / _bwd (BTX-SVD v1) with the per-item terms, btx_logalpha_stats with a histogram (the call clears its own
    counters) and btx_logalpha_prune (mu / rho are rewritten in place: fresh copies per run)"""
    from bayesian_torch_amd import functional as BF
    import test_gpu_svd as SV
    run = Run("test_log_uniform_kl_statistics_and_pruning")
    host = [SV._host(1, 3), SV._host(4097, 4)]
    ts = [(SV._t(mu), SV._t(rho)) for mu, rho in host]
    entries = [(mu, rho, red) for (mu, rho), red in zip(ts, SV.REDUCTIONS)]
    gout = torch.tensor(SV.G, device=_dev())

    def call(accumulate):
        if accumulate:
            kl, terms = BF.kl_logu_model_hip(entries, out=torch.full((), 2.5, device=_dev()), accumulate=True), None
        else:
            kl, terms = BF.kl_logu_model_hip(entries, terms=True)
        grads = [(torch.empty_like(e[0]), torch.empty_like(e[0])) for e in entries]
        BF.kl_logu_model_bwd_hip(entries, grads, gout)
        return kl, terms, grads
    run.three("kl_logu_model", lambda: call(False))
    run.three("kl_logu_model accumulate", lambda: call(True))
    run.three("logalpha_stats", lambda: BF.logalpha_stats_hip(ts, (-1.0, 0.5, 3.0), bins=8))
    run.three("logalpha_stats no histogram", lambda: BF.logalpha_stats_hip(ts, (), bins=0))

    def prune():
        fresh = [(mu.clone(), rho.clone()) for mu, rho in ts]
        n = BF.logalpha_prune_hip(fresh, -1.0)
        return n, fresh
    run.three("logalpha_prune", prune)
    run.done()


# ---- 4. heads and evaluation -----------------------------------------------------------------------------------------------------------
def test_calibration_heads():
    """AvU / AUAvU on logits and EaU / EaC on error and uncertainty vectors (btx_avu_* / btx_eau_*): loss, gradients; the workspace the
    forward writes is what the backward reads"""
    from avuc_cases import load
    from bayesian_torch_amd.utils import avuc_loss as A
    from bayesian_torch_amd.utils import uncertainty_calibration_loss as U
    run = Run("test_calibration_heads")
    cases = load()
    by_size = sorted(cases["avu"], key=lambda k: cases["avu"][k]["logits"].size)
    for name in (by_size[0], [k for k in by_size if cases["avu"][k]["logits"].shape[0] > 1][0]):
        c = cases["avu"][name]
        lb = torch.from_numpy(c["labels"]).to(_dev())
        for dt in (F32, BF16):
            lg0 = torch.from_numpy(c["logits"]).to(_dev()).to(dt)
            for area in ((False, True) if c["logits"].shape[0] > 1 else (False,)):
                def avu():
                    lg = lg0.detach().clone().requires_grad_(True)
                    if area:
                        loss, r = A.AUAvULoss(beta=float(c["beta"]))(lg, lb)
                    else:
                        loss, r = A.AvULoss(beta=float(c["beta"]))(lg, lb, float(c["th"])), None
                    loss.sum().backward()
                    return loss.detach(), (None if r is None else r.detach()), lg.grad
                run.three("avu %s %s area=%s" % (name, dt, area), avu)
    ename = min(cases["eau"], key=lambda k: cases["eau"][k]["error"].size)
    c = cases["eau"][ename]
    for conf_form in (False, True):
        mod = (U.EaCLoss if conf_form else U.EaULoss)(beta=float(c["beta"]))
        e0 = torch.from_numpy(c["error"]).to(_dev())
        u0 = torch.from_numpy(c["conf" if conf_form else "unc"]).to(_dev())

        def eau():
            e, u = e0.clone().requires_grad_(True), u0.clone().requires_grad_(True)
            loss = mod(e, u, float(c["error_th"]), float(c["conf_th" if conf_form else "unc_th"]))
            loss.backward()
            return loss.detach(), e.grad, u.grad
        run.three("eau %s conf=%s" % (ename, conf_form), eau)
    run.done()


def test_mc_loss_heads():
    """MC cross-entropy and AvU on the stack (btx_mc_ce_* / btx_avu_mc_*): the smallest rows of mc_loss_cases.py, and a bf16 one"""
    import mc_loss_cases as K
    from bayesian_torch_amd.utils import avuc_loss as A
    from bayesian_torch_amd.utils import mc_loss as M
    run = Run("test_mc_loss_heads")
    size = lambda spec: spec[0] * spec[1] * spec[2]  # noqa: E731
    ce = sorted(K.CE_CASES, key=lambda n: size(K.CE_CASES[n]))[:3] + ["bf16_s2_b3_c257_x1"]
    for name in ce:
        c = K.ce_case(name)
        st0, y = K.to_device(c, _dev(), K.torch_dtype(name))
        for reduce in K.REDUCES:
            def head():
                st = st0.detach().requires_grad_(True)
                k = torch.tensor([K.KL], device=_dev(), requires_grad=True)
                loss = M.mc_elbo_loss(st, y, k, reduce, 0.1)
                assert isinstance(loss.grad_fn, M.McCeFn._backward_cls)
                loss.backward()
                return loss.detach(), st.grad, k.grad
            run.three("mc ce %s %s" % (name, reduce), head)
    avu = sorted(K.AVU_AREA_CASES, key=lambda n: size(K.AVU_CASES[n]))[:2] + ["s2_b3_c10_x8"]
    for name in avu:
        c = K.avu_case(name)
        st0, y = K.to_device(c, _dev(), K.torch_dtype(name))
        for area in ((False, True) if name in K.AVU_AREA_CASES else (False,)):
            def head():
                st = st0.detach().requires_grad_(True)
                if area:
                    loss, r = A.AUAvULoss(beta=K.BETA)(st, y, type=1)
                else:
                    loss, r = A.AvULoss(beta=K.BETA)(st, y, c["th"], type=1), None
                loss.sum().backward()
                return loss.detach(), (None if r is None else r.detach()), st.grad
            run.three("avu mc %s area=%s" % (name, area), head)
    run.done()


def test_regression_heads_and_evaluator():
    """BTX-REG v1: the moment statistics (packed sums: an input, zeroed per run), the Gaussian NLL head forward and backward, one update
    of the device evaluator (its state is an input; only the workspace is poisoned)"""
    import numpy as np
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.utils import mc_loss as M
    import reg_model as RM
    run = Run("test_regression_heads_and_evaluator")
    dev = _dev()
    for (lanes, bs, D), dtype in (((1, 3, 1), F32), ((4, 5, 3), BF16), ((2, 3, 8), F32)):
        out = torch.from_numpy((np.random.RandomState(lanes * 100 + D).randn(lanes * bs, 2 * D) * 2).astype(np.float32)).to(dtype).to(dev)
        st = mc.GaussianStats("log")
        run.three("moments %s" % ((lanes, bs, D),),
                  lambda: st.accumulate_lanes(torch.zeros(st.numel(bs, 2 * D), dtype=torch.float64, device=dev), out, lanes, kl=0.75))
    for (S, B, D), bf16 in [(s, b) for s in sorted(RM.HEAD_SHAPES, key=lambda s: s[0] * s[1] * s[2])[:3] for b in (False, True)]:
        stack, y = RM.head_case(S, B, D, bf16=bf16)
        t0 = torch.from_numpy(stack).to(dev).to(BF16 if bf16 else F32)
        yd = torch.from_numpy(y).to(dev)
        for reduce in ("loss", "moments"):
            def head():
                t = t0.detach().requires_grad_(True)
                k = torch.tensor([RM.KL], device=dev, requires_grad=True)
                loss = M.mc_gaussian_nll(t, yd, k, reduce, "log", None, False)
                assert isinstance(loss.grad_fn, M.McGnllFn._backward_cls)
                loss.backward()
                return loss.detach(), t.grad, k.grad
            run.three("gnll %s %s bf16=%s" % ((S, B, D), reduce, bf16), head)
    c = RM.eval_case(7, 5, 4, seed=11)
    N = 7 * 5
    packed, yd = torch.from_numpy(c["packed"]).to(dev), torch.from_numpy(c["y"]).to(dev)

    def update():
        ev = mc.RegressionEvaluator(c["D"], levels=c["levels"], noise_var=c["noise_var"], capacity=N, device=dev)
        ev.update(packed, yd)
        return ev.state, ev.records_buffer
    run.three("reg evaluator", update, finite=False)  # (err is NaN on an ignored element: btx.h)
    run.done()


def test_mc_evaluator():
    """BTX-EVAL v1: one update on two shapes of test_gpu_mc_eval.SHAPES; state and records"""
    from bayesian_torch_amd import mc
    import test_gpu_mc_eval as EV
    run = Run("test_mc_evaluator")
    dev = _dev()
    for C, bs in ((5, 64), (257, 130)):
        assert (C, bs) in EV.SHAPES
        c = EV._random_case(C, bs)
        packed, labels = EV._t(c["packed"], dev), EV._t(c["labels"], dev)
        for use_mi in (False, True):
            th = c["th_mi"] if use_mi else c["th"]

            def update():
                ev = mc.Evaluator(C, thresholds=th, uncertainty="mi" if use_mi else "entropy", capacity=bs, device=dev)
                ev.update(packed, labels)
                assert ev.workspace is not None
                return ev.state, ev.records_buffer
            run.three("mc evaluator C=%d bs=%d mi=%s" % (C, bs, use_mi), update)
    run.done()


# ---- 5. LSTM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1, 2])
def test_lstm(case):
    """CASES[0..2] of test_gpu_lstm_elementwise.py, both families, f32 and bf16: hidden and cell sequences of the inference and the
    training kernel, the gates and cell states of `saved` (the words between the two blocks are padding), then the backward that
    consumes `saved` and the workspace"""
    from bayesian_torch_amd import _lib, functional as BF, layers as L, rng
    import bayesian_torch_amd as bt
    import test_gpu_lstm_elementwise as LE
    run = Run("test_lstm")
    I, H, B, T = LE.CASES[case]
    dev = _dev()
    for cls in LE.FAMILIES:
        bt.manual_seed(LE.SEED)
        bt.set_precision("f32")
        g = torch.Generator().manual_seed(1000 * LE.FAMILIES.index(cls) + case)
        layer = getattr(L, cls)(I, H, bias=True).to(dev)
        bt.assign_layer_ids(layer, start=900)
        kind = _lib.KIND_FLIPOUT if cls == "LSTMFlipout" else _lib.KIND_REPARAM
        x32 = (0.25 * torch.randn(B, T, I, generator=g)).to(dev)
        h32, c32 = (0.5 * torch.randn(B, H, generator=g)).to(dev), torch.randn(B, H, generator=g).to(dev)
        rh32, rc32 = torch.randn(B, T, H, generator=g).to(dev), torch.randn(B, T, H, generator=g).to(dev)
        for prec, act, state in (("f32", F32, True), ("bf16", BF16, True), ("f32", F32, False)):
            x, d_hs, d_cs = x32.to(act), rh32.to(act), rc32.to(act)
            h0, c0 = (h32.to(act), c32.to(act)) if state else (None, None)
            ihp, hhp = LE._params(layer.ih, LE.S0, True), LE._params(layer.hh, LE.S0, True)

            def call():
                hs, cs, _, sv = BF.lstm_train_fwd_hip(kind, x, ihp, hhp, rng.seed(), prec=prec, h0=h0, c0=c0)
                hs_i, cs_i, _ = BF.lstm_hip(kind, x, ihp, hhp, rng.seed(), prec=prec, h0=h0, c0=c0)
                gates, cells = LE._saved_views(sv, T, B, H)
                dx, dh0, dc0, gi, gh = BF.lstm_bwd_hip(kind, x, ihp, hhp, rng.seed(), hs, sv, d_hs, d_cs, prec=prec, h0=h0, c0=c0,
                                                       want_dx=True, want_dh0=state, want_dc0=state)
                return hs, cs, hs_i, cs_i, gates, cells, dx, dh0, dc0, tuple(gi), tuple(gh)
            run.three("lstm %s %s %s state=%s" % (cls, LE.CASES[case], prec, state), call)
    run.done()


# ---- 6. optimizer and bucket -------------------------------------------------------------------------------------------------------------
def test_optimizers_and_gradient_norm():
    """fused SGD (momentum) and Adam with gradient clipping on tensors of 1, 4095 and 4097 elements, two steps: parameters, state and
    the norm; parameters and state are inputs (fresh per run), the norm's partials and the staging buffers are not"""
    import numpy as np
    from bayesian_torch_amd import optim
    run = Run("test_optimizers_and_gradient_norm")
    dev = _dev()
    r = np.random.RandomState(5)
    sizes = (1, 4095, 4097)
    p0 = [(0.1 * r.randn(n)).astype(np.float32) for n in sizes]
    gs = [[r.randn(n).astype(np.float32) for n in sizes] for _ in range(2)]
    for name, cfg in (("SGD", dict(lr=0.05, momentum=0.9, weight_decay=1e-3)), ("Adam", dict(lr=1e-2, weight_decay=1e-3))):
        def steps():
            params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in p0]
            opt = getattr(optim, name)(params, max_grad_norm=0.5, **cfg)
            norms = []
            for step in range(2):
                for p, g in zip(params, gs[step]):
                    p.grad = torch.from_numpy(g).to(dev)
                opt.step()
                norms += [opt.total_norm.clone(), opt.clip_coef.clone()]
            state = [[v for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)] for p in params]
            return [p.detach() for p in params], norms, state
        run.three("optimizer %s" % name, steps)
    run.done()


def test_gradient_bucket():
    """btx_bucket_pack then btx_bucket_unpack on three tensors of 1, 4095 and 4097 elements at world 3: the unpacked gradients"""
    from bayesian_torch_amd import parallel
    run = Run("test_gradient_bucket")
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    sizes = (1, 4095, 4097)
    grads = [torch.randn(n, generator=g).to(dev) for n in sizes]

    class Three(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in sizes])

    def round_trip():
        m = Three().to(dev)
        for p, gi in zip(m.parameters(), grads):
            p.grad = gi.clone()
        red = parallel.GradReducer(m, rank=1, world=3)
        red.pack(torch.tensor(2.5, device=dev))
        views = [red.grad_view(p).clone() for p in m.parameters()]
        loss = red.loss.clone()
        for p in m.parameters():   # the unpack must write every element of the gradients
            p.grad = torch.empty_like(p)
        red.unpack()
        return views, loss, [p.grad for p in m.parameters()]
    run.three("bucket", round_trip)
    run.done()


# ---- 7. INT8 -------------------------------------------------------------------------------------------------------------------------
def test_int8():
    """one default case each of q8_helpers / q8_flipout_helpers and the residual case of test_gpu_q8_net: quantize, sample, contract,
    contract_res, add, both pools, sample_delta and contract_flipout; the outputs and the row sums / bias vectors of the pre-passes
    (the weight images hold padding: the contraction that reads them is what is compared)"""
    import numpy as np
    from bayesian_torch_amd import q8
    from bayesian_torch_amd.q8 import QTensor
    import q8_helpers as H
    import q8_flipout_helpers as FH
    import test_gpu_q8_net as QN
    run = Run("test_int8")
    dev = "cuda"
    qt = lambda a, s, z: QTensor(torch.from_numpy(np.ascontiguousarray(a)).to(dev), s, z)  # noqa: E731
    # Reparameterization: float input -> quantize -> sample -> contract
    d = H.fixture("q8_conv_default")
    q = H.quantized_layer(dict(d, kind=np.int64(1)), dev)
    x = torch.from_numpy(d["x"]).to(dev)
    noise = dict(eps_w=torch.from_numpy(d["eps"]), eps_b=torch.from_numpy(d["eps_b"]))

    def conv(nz):
        with torch.no_grad():
            out, W, S, b_i = q.forward_int8(x, noise=nz, parts=True)
        return out.int_repr(), S, b_i
    run.three("q8 conv default, recorded noise", lambda: conv(noise))
    # the fused residual add and q8.add
    c = QN.res_case(0, True)
    qr = c["q"].to(dev)
    s_eps, s_d, s_w = c["chain"]
    z_r = 131
    qr.quant_dict = [(s_eps, 0), (s_d, 0), (s_w, 0), (c["s_x"], c["z_x"]), (c["s_o"], QN.CONV_ZO[z_r])]
    qr.relu = False
    rnoise = dict(eps_w=c["eps"], eps_b=c["eps_b"])
    try:
        def res():
            with torch.no_grad():
                xq, rq = qt(c["x_i"], c["s_x"], c["z_x"]), qt(c["res"], c["s_r"], z_r)
                fused = qr.forward_int8(xq, noise=rnoise, residual=rq, add_relu=True, add_scale=None, add_zero_point=120)
                plain = qr.forward_int8(xq, noise=rnoise)
                added = q8.add(plain, rq, c["s_o"], 120, relu=True)
            return fused.int_repr(), plain.int_repr(), added.int_repr()
        run.three("q8 contract_res and add", res)
    finally:
        qr.quant_dict, qr.relu = None, False
    # pools
    xb, xa = QN._bytes((2, 16, 9, 9), 7), QN._bytes((2, 64, 7, 7), 11)
    run.three("q8 pools", lambda: (q8.max_pool2d(qt(xb, 0.1, 77), 3, 2, 1).int_repr(), q8.avg_pool2d(qt(xa, 0.1, 77), 7, 1).int_repr()))
    # Flipout
    d = FH.fixture("q8f_conv_default")
    qf = FH.quantized_layer(d, dev)

    def flip():
        with torch.no_grad():
            out, parts = qf.forward_int8(qt(d["x_i"], *FH.e_x(d)), noise=FH.noise_of(d), parts=True)
        return out.int_repr(), parts["S_d"], parts["S_mu"], parts["bm_i"], parts["bp_i"]
    run.three("q8 flipout conv default", flip)
    run.done()


# ---- 8. captured graphs ----------------------------------------------------------------------------------------------------------------
def _two_layer_net(train):
    import bayesian_torch_amd as bt
    torch.manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Conv2d(32, 64, 3, padding=1, bias=True), torch.nn.ReLU(),
                              torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(64, 16))
    bt.dnn_to_bnn(net, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                            moped_enable=False, moped_delta=0.5))
    net = net.to(_dev())
    net = net.train() if train else net.eval()
    bt.assign_layer_ids(net)
    return net


def _fill_cached(byte, extra):
    """between replays: every buffer of functional._WS and the graph's own output tensors"""
    from bayesian_torch_amd import functional as BF
    n = 0
    for t in list(BF._WS.values()) + [t for t in extra if t is not None and t.is_cuda]:
        n += P.fill_bytes(t, byte)
    torch.cuda.synchronize()
    return n


def test_graphed_mc_replays_do_not_depend_on_cached_buffers():
    """mc.GraphedMC with 2 lanes on a two-layer model, captured with poison off: every workspace in functional._WS and the graph's
    own logits are overwritten with each pattern between replays; each replay must return the bits of the first"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    dev = _dev()
    bt.manual_seed(8)
    net = _two_layer_net(False)
    x = torch.randn(4, 32, 12, 12, generator=torch.Generator().manual_seed(3)).to(dev)
    g = mc.GraphedMC(net, x, kl=0.0, lanes=2, keep_logits=True)
    try:
        g.run_many([5, 6])
        torch.cuda.synchronize()
        first = [t.clone() for t in g.lane_logits]
        total = 0
        for byte in P.PATTERNS:
            total += _fill_cached(byte, g.lane_logits)
            g.run_many([5, 6])
            torch.cuda.synchronize()
            assert P.bits_equal([t for t in g.lane_logits], first), "replay after %#04x fill differs" % byte
        assert total > 0 and not P.any_nan(first)
        print("GraphedMC replay: %d bytes poisoned between replays, patterns ff/7f: equal" % total)
    finally:
        g.close()


def test_graphed_train_step_replays_do_not_depend_on_cached_buffers():
    """autograd.GraphedTrainStep with the fused SGD inside the graph: parameters are restored, the workspaces, the loss and every
    gradient tensor the graph writes are overwritten with each pattern, and the replay must give the loss, gradients and updated
    parameters of the first"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = _dev()
    bt.manual_seed(9)
    bt.set_precision("f32")
    net = _two_layer_net(True)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(8, 32, 12, 12, generator=gen).to(dev)
    y = torch.randint(0, 16, (8,), generator=gen).to(dev)
    params = list(net.parameters())
    start = [p.detach().clone() for p in params]
    opt = optim.SGD(params, lr=0.05, weight_decay=1e-3)
    gs = GraphedTrainStep(net, x, y, optimizer=opt)
    try:
        def replay():
            with torch.no_grad():
                for p, s in zip(params, start):
                    p.copy_(s)
            loss = gs.run(7)
            torch.cuda.synchronize()
            return loss.clone(), [p.grad.clone() for p in params], [p.detach().clone() for p in params]
        first = replay()
        total = 0
        for byte in P.PATTERNS:
            total += _fill_cached(byte, [gs.loss] + [g_ for _, g_ in gs._grads])
            got = replay()
            assert P.bits_equal(got, first), "replay after %#04x fill differs: %s" % (byte, _first_difference(got, first))
        assert total > 0 and not P.any_nan(first)
        assert not P.bits_equal(first[2], start)
        print("GraphedTrainStep replay: %d bytes poisoned between replays, patterns ff/7f: equal" % total)
    finally:
        gs.close()
