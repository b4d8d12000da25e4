"""GPU: the autograd contract of the HIP Functions (bayesian_torch_amd/autograd.py; DESIGN.md "Autograd contract").

The numerical files pin WHAT every Function computes when everything requires a gradient and one dense backward follows one forward.
This file pins that the same values come out the other ways autograd calls them: subsets of needs_input_grad (frozen parameters), a
second forward before the first backward, a seed change in between, the forms dy arrives in, retained graphs and accumulation, a layer
applied twice, second order (refused), in-place updates (caught), activation checkpointing, and a captured step with frozen parameters.
Cases, float64 references and scenarios live in tests/autograd_cases.py; tests/test_autograd_contract_cpu.py runs the scenarios against
a stand-in with planted faults.

Two comparison rules (autograd_cases.py): the same bits where two HIP calls run the same launches, the envelope of tests/envelope.py
against float64 where they do not.  Each test prints its lines; profiles/autograd_contract.txt holds those of the first run.

A case is left out of a scenario only in the tables below, with the reason; nothing is skipped at run time.
"""
import warnings

import pytest
import torch

import autograd_cases as AC
import drop_model as DM
import envelope as E

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

F32, BF16 = torch.float32, torch.bfloat16
S = AC.SAMPLE
CONTRACT = ["L1", "L2", "L3", "C1", "C2", "C2e", "C3", "C4", "C5", "C6", "C7"]
# (case, precision, activation dtype, fused_training): every case in f32; C1, L1 and R2 in bf16 activations as well
VARIANTS = [(c, "f32", F32, None) for c in CONTRACT] + [("C1", "bf16", BF16, None), ("L1", "bf16", BF16, None)] + \
           [("R1", "f32", F32, True), ("R1", "f32", F32, False), ("R2", "f32", F32, True), ("R2", "f32", F32, False),
            ("R2", "bf16", BF16, True)]


def _vid(v):
    c, prec, act, fused = v
    return "%s-%s%s" % (c, "bf16" if act is BF16 else "f32", "" if fused is None else ("-fused" if fused else "-composite"))


def _builder(v):
    c, prec, act, fused = v
    return lambda: AC.build(AC.BY_ID[c], prec, act, fused)


def _lrt_ref64(prec, act):
    """the float64 model of tests/lrt_bwd_model.py, as tests/test_gpu_lrt_train.py feeds it"""
    import lrt_bwd_model as BM
    import lrt_model as LM

    def ref(layer, x, dy, sample):
        with torch.no_grad():
            zeta = layer.materialize_noise(sample, out_shape=tuple(dy.shape))["zeta"]
        mu, rho, mb, rb = LM.layer_arrays(layer)
        m = BM.backward(x.float().cpu().numpy(), dy.float().cpu().numpy(), zeta.float().cpu().numpy(), mu, rho, mb, rb,
                        LM.op_of(layer), prec=prec, act_bf16=act is BF16)
        return m["ref"], m["bound"]
    return ref


def _ref64(v):
    """the float64 side of a variant's all-gradients call: the reference chain for the contraction layers, the LRT model for the LRT
    layers.  The Linear ATen composite (R1, fused_training off) is torch's own autograd on GEMMs, pinned by tests/test_gpu_lrt.py:
    bits only."""
    c, prec, act, fused = v
    if c in CONTRACT:
        return AC.ref64_single(prec)
    return _lrt_ref64(prec, act) if (fused or c == "R2") else None


def _inexact(v):
    """R2 with fused_training off: dmu / drho of the ATen composite come from torch's convolution weight gradient, which is not
    bit-reproducible from call to call on the device (two backward calls on ONE retained graph differ in the last bit, 656 of 2304
    elements, mismatch / max|ref| 2.9e-9): they are compared with float64 by the envelope rule, under torch's DEFAULT algorithm
    choice — the configuration users run.  Everything else of the composite keeps the bit rule.

    An open observation (profiles/autograd_contract.txt): in ONE run of this file, 64 of 2304 elements of dmu and 48 of drho — whole
    groups of the 16 input channels of one (output channel, tap), other groups on every call — were off by up to 12.5 (|dmu| <= 42).
    It has not happened again: three later runs of the same tests in the same order, and 5 calls in a fresh process under each
    layout of x and dy, were inside the bound (worst err/bound 0.0121 dmu, 0.0156 drho).  What was ruled out: the project's launches
    that precede the composite (the inference forward, btx_fill_eps for zeta) take torch's current stream and allocate nothing of
    their own, and every test ends on a device-to-host copy; torch alone — a process that never loads the library — on allocator
    blocks recycled with 7, 1e30 and NaN in them returned the float64 gradient to 6.6e-6 on every call.  The cause was not found;
    if it comes back, this test fails, which is what it is for."""
    return ("mu", "rho") if (v[0] == "R2" and v[3] is False) else ()


# the scenarios that have the bit rule only leave the R2 composite out: see _inexact
BITS_ONLY = [v for v in VARIANTS if not (v[0] == "R2" and v[3] is False)]


# ---- S1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS, ids=[_vid(v) for v in VARIANTS])
def test_s1_every_subset_of_needs_input_grad_has_the_bits_of_the_all_gradients_call(v):
    AC.s1_subsets(_builder(v), _vid(v), _ref64(v), v[1], inexact=_inexact(v))


def _dropouts():
    import bayesian_torch_amd as bt
    bt.manual_seed(2024)
    out = []
    for cls, shape in ((bt.MCDropout, (4, 40)), (bt.MCDropout2d, (2, 16, 5, 5))):
        layer = cls(0.3).to(AC.dev())
        bt.assign_layer_ids(layer)
        out.append((layer, AC.tensor(shape, F32, 11, AC.dev(), 1.5)))
    return out


def _dropout_builder(i):
    return lambda: _dropouts()[i]


@pytest.mark.parametrize("i", [0, 1], ids=["D1-element", "D1-channel"])
def test_s1_dropout_gradient_is_the_model_bit_for_bit(i):
    """D1: x is the only input; dx = where(keep, dy * scale, +0) with the mask BTX-DROP v1 defines at the forward's sample"""
    layer, x = _dropouts()[i]
    dy = AC.dy_for(layer, x)
    out, g = AC.step(layer, x, ("x",), dy, S)
    assert out.grad_fn is not None
    keep = layer.materialize_mask(tuple(x.shape), S).numpy()
    notes = AC.Notes("D1 %s S1" % layer.mode)
    notes.bits("dx", g["x"], DM.apply_f32(dy.float().cpu().numpy(), keep, layer._btx_scale))
    notes.bits("out", out, DM.apply_f32(x.float().cpu().numpy(), keep, layer._btx_scale))
    notes.done()


def _bn_parts():
    """B1: BatchNorm2d(16), MaxPool2d(3, 2, 1), x and the residual, (2, 16, 7, 7) channels-last — the same every call"""
    dev = AC.dev()
    torch.manual_seed(3)
    bn = torch.nn.BatchNorm2d(16).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(AC.tensor((16,), F32, 21, dev) * 0.5 + 1.0)
        bn.bias.copy_(AC.tensor((16,), F32, 22, dev) * 0.3)
    return bn, torch.nn.MaxPool2d(3, 2, 1), AC.tensor((2, 16, 7, 7), F32, 11, dev, 1.5), AC.tensor((2, 16, 7, 7), F32, 14, dev)


def _bn_pool(subset, with_y=False):
    """B1: [relu](bn(x) + residual) through autograd.bn_act, then MaxPool2d(3, 2, 1) through max_pool_train"""
    from bayesian_torch_amd import autograd as AG
    bn, mp, x, res = _bn_parts()
    x.requires_grad_("x" in subset)
    res.requires_grad_("res" in subset)
    bn.weight.requires_grad_("gamma" in subset)
    bn.bias.requires_grad_("beta" in subset)
    assert AG.bn_train_usable(bn, x)
    y = AG.bn_act(bn, x, residual=res, relu=True)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("BatchNormTrainFn"), y.grad_fn
    assert AG.max_pool_train_usable(mp, y)
    z = AG.max_pool_train(mp, y)
    leaves = {n: t for n, t in (("x", x), ("res", res), ("gamma", bn.weight), ("beta", bn.bias)) if n in subset}
    return (z, leaves, y) if with_y else (z, leaves)


def test_s1_batchnorm_and_maxpool_all_gradients_inside_the_envelope():
    """B1, the all-gradients call against float64.  Max-pool backward: window 3, stride 2 — an input element lies in at most 2 x 2
    windows, so its gradient is a sum of at most 4 of the dz it won: 3 f32 adds, bound 3 * 2^-24 * (the same sum on |dz|), against
    float64 max_pool2d on the y the device stored (first maximum in scan order on either side; most windows tie at 0 behind the ReLU).
    BatchNorm + residual + ReLU: envelope.bn_forward64 / bn_backward64 as tests/test_gpu_reductions.py feeds them (_bn_envelope: y, dx,
    dgamma, dbeta, dres, statistics, running estimates), on a twin module fed with the dy the pool's backward produced; the
    all-gradients call of B1 has the bits of that twin's call."""
    from test_gpu_reductions import _bn_envelope
    names = ("x", "res", "gamma", "beta")
    z, leaves, y = _bn_pool(names, with_y=True)
    dz = AC.tensor(tuple(z.shape), F32, 12, z.device)
    (dy_y,) = torch.autograd.grad(z, y, dz, retain_graph=True)
    g_all = AC.grads(z, leaves, dz)
    notes = AC.Notes("B1 S1")
    y64 = y.detach().double().cpu().contiguous().requires_grad_(True)
    z64 = torch.nn.functional.max_pool2d(y64, 3, 2, 1)
    (ref,) = torch.autograd.grad(z64, y64, dz.double().cpu().contiguous(), retain_graph=True)
    (A,) = torch.autograd.grad(z64, y64, dz.abs().double().cpu().contiguous())
    notes.envelope("all max-pool dy", "f32", dy_y, ref, 3 * E.REF32_UNIT * E._np(A))
    notes.bits("max-pool out", z, z64.detach())
    bn2, _, x2, res2 = _bn_parts()
    log = AC.Log()
    got, _, _ = _bn_envelope(log, "B1 S1 all bn+res+relu", bn2, x2, dy_y.detach(), res2, relu=True)
    notes.bad += log.bad
    for n, k in (("x", "dx"), ("res", "dres"), ("gamma", "dgamma"), ("beta", "dbeta")):
        notes.bits("all d%s = the twin's %s" % (n, k), g_all[n], got[k])
    notes.done("the all-gradients call inside the BN / max-pool envelopes")


def test_s1_batchnorm_residual_relu_and_maxpool_subsets():
    names = ("x", "res", "gamma", "beta")
    z, leaves = _bn_pool(names)
    dz = AC.tensor(tuple(z.shape), F32, 12, z.device)
    g_all = AC.grads(z, leaves, dz)
    notes = AC.Notes("B1 S1")
    for sub in (("x",), ("gamma",), ("res",), ("beta",), ("x", "res"), ("gamma", "beta")):
        zs, lv = _bn_pool(sub)
        notes.bits("{%s} out" % "+".join(sub), zs, z)
        g = AC.grads(zs, lv, dz)
        for n in sub:
            notes.bits("{%s} d%s" % ("+".join(sub), n), g[n], g_all[n])
    notes.done()


LSTM_NAMES = ("x", "h0", "c0") + tuple("%s.%s" % (a, b) for a in ("ih", "hh") for b in ("mu", "rho", "mu_b", "rho_b"))


def _lstm(cls):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(3)
    layer = getattr(L, cls)(12, 8).to(AC.dev())
    bt.assign_layer_ids(layer)
    with torch.no_grad():
        g = torch.Generator().manual_seed(41)
        for lin in (layer.ih, layer.hh):
            lin.rho_weight.copy_((torch.rand(tuple(lin.rho_weight.shape), generator=g) * 4.0 - 5.0).to(AC.dev()))
            lin.mu_bias.copy_((torch.randn(tuple(lin.mu_bias.shape), generator=g) * 0.3).to(AC.dev()))
            lin.rho_bias.copy_((torch.rand(tuple(lin.rho_bias.shape), generator=g) * 3.0 - 4.0).to(AC.dev()))
    layer.fused_training = True
    return layer


def _lstm_forward(layer, subset, sample=S):
    import bayesian_torch_amd as bt
    dev = AC.dev()
    leaves = {"x": AC.tensor((3, 4, 12), F32, 11, dev), "h0": AC.tensor((3, 8), F32, 15, dev, 0.5), "c0": AC.tensor((3, 8), F32, 16, dev, 0.5)}
    for a, lin in (("ih", layer.ih), ("hh", layer.hh)):
        leaves.update({a + ".mu": lin.mu_weight, a + ".rho": lin.rho_weight, a + ".mu_b": lin.mu_bias, a + ".rho_b": lin.rho_bias})
    for n, t in leaves.items():
        t.requires_grad_(n in subset)
        t.grad = None
    bt.set_sample_index(layer, sample)
    assert layer._fused_train_ok(leaves["x"], (leaves["h0"], leaves["c0"])), "T1 is no longer on the fused training path: %s" % (subset,)
    hs, (_, cs), kl = layer(leaves["x"], (leaves["h0"], leaves["c0"]))
    return hs, cs, {n: leaves[n] for n in subset}


def _lstm_grads(hs, cs, leaves, retain=False):
    d_hs, d_cs = AC.tensor(tuple(hs.shape), F32, 12, hs.device), AC.tensor(tuple(cs.shape), F32, 13, cs.device)
    names = list(leaves)
    return dict(zip(names, torch.autograd.grad([hs, cs], [leaves[n] for n in names], [d_hs, d_cs], retain_graph=retain, allow_unused=True)))


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_s1_fused_lstm_selective_gradients_have_the_bits_of_the_all_gradients_call(cls):
    layer = _lstm(cls)
    hs_all, cs_all, leaves = _lstm_forward(layer, LSTM_NAMES)
    g_all = _lstm_grads(hs_all, cs_all, leaves)
    notes = AC.Notes("T1 %s S1" % cls)
    for n in LSTM_NAMES:
        if g_all[n] is None:
            notes.bad.append("T1 all: d%s is None" % n)
    ih, hh = tuple(n for n in LSTM_NAMES if n.startswith("ih.")), tuple(n for n in LSTM_NAMES if n.startswith("hh."))
    for sub in (ih, hh, ("h0", "c0"), ("hh.rho_b",), ("ih.rho_b",), ("x",), ("ih.mu", "hh.rho")):
        hs, cs, lv = _lstm_forward(layer, sub)
        key = "+".join(sub)
        if hs.grad_fn is None:
            notes.bad.append("T1 %s S1 {%s}: the output has no grad_fn" % (cls, key))
            continue
        notes.bits("{%s} hs" % key, hs, hs_all)
        g = _lstm_grads(hs, cs, lv)
        for n in sub:
            notes.bits("{%s} d%s" % (key, n), g[n], g_all[n])
    notes.done()


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_s1_fused_lstm_all_gradients_inside_the_envelope(cls):
    """T1, the all-gradients call THROUGH LstmTrainFn against float64: the per-step references of tests/test_gpu_lstm_elementwise.py
    (envelope.lstm_gates64 / lstm_cell64 / lstm_bptt64, fed with weights probed from the device at this shape) applied to what the
    layer's forward and torch.autograd.grad returned — hidden_seq, c_seq, the saved gates and cells, dx, dh0, dc0 and the eight
    parameter gradients."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import rng
    import test_gpu_lstm_elementwise as LE
    case, cfg = (12, 8, 3, 4), ("f32", "f32", True, True)
    I, H, B, T = case
    old = rng.seed()
    c = LE._ctx(cls, case)
    try:
        bt.manual_seed(c.seed)
        bt.set_precision("f32")
        layer = c.layer
        layer.fused_training = True
        leaves = {"x": c.x.detach().clone().requires_grad_(True), "h0": c.h0.detach().clone().requires_grad_(True),
                  "c0": c.c0.detach().clone().requires_grad_(True)}
        for a, lin in (("ih", layer.ih), ("hh", layer.hh)):
            leaves.update({a + ".dmu_w": lin.mu_weight, a + ".drho_w": lin.rho_weight, a + ".dmu_b": lin.mu_bias, a + ".drho_b": lin.rho_bias})
        bt.set_sample_index(layer, LE.S0)
        assert layer._fused_train_ok(leaves["x"], (leaves["h0"], leaves["c0"]))
        hs, (_, cs), _ = layer(leaves["x"], (leaves["h0"], leaves["c0"]))
        assert type(hs.grad_fn).__name__.startswith("LstmTrainFn")
        names = list(leaves)
        g = dict(zip(names, torch.autograd.grad([hs, cs], [leaves[n] for n in names], [c.r_h, c.r_c])))
    finally:
        bt.manual_seed(old)
    gates, cells = LE._saved_views(hs.grad_fn.saved_buf, T, B, H)
    r = dict(x=leaves["x"], h0=leaves["h0"], c0=leaves["c0"], hs=hs, cs=cs, hs_i=hs, cs_i=cs, gates=gates, cells=cells, d_hs=c.r_h,
             d_cs=c.r_c, dx=g.pop("x"), dh0=g.pop("h0"), dc0=g.pop("c0"), **g)
    LE._RUNS[(id(c), cfg)] = {k: v.detach().cpu().clone() for k, v in r.items()}   # what _reports reads in place of its direct launches
    reps, _ = LE._reports(c, cfg)
    worst = {}
    for k, rep in reps.items():
        worst[k.split(" t=")[0]] = max(worst.get(k.split(" t=")[0], 0.0), rep.worst)
    print("T1 %s S1 all f32: worst err/bound %s" % (cls, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    bad = ["%s: %s" % (k, rep) for k, rep in reps.items() if not rep.ok]
    assert not bad, "\n".join(bad[:8])
    assert any(k.startswith("bwd ih.drho_b") for k in reps) and any(k.startswith("bwd dx") for k in reps)


def _kl_layer(kind):
    import bayesian_torch_amd as bt
    layer, x = AC.build(AC.BY_ID["C1"])
    if kind == "mc":
        layer.set_prior(bt.priors.LaplacePrior(0.7), kl_samples=2)
    elif kind == "logu":
        layer.set_prior(bt.priors.LogUniformPrior())
    return layer, x


def _kl_fn_name(kind):
    return {"gauss": "KlFn", "mc": "KlMcFn", "logu": "KlLogUFn"}[kind]


@pytest.mark.parametrize("kind", ["gauss", "mc", "logu"])
def test_s1_kl_mu_only_and_rho_only_have_the_bits_of_the_both_wanted_call(kind):
    import bayesian_torch_amd as bt
    layer, _ = _kl_layer(kind)
    names = tuple(AC.params_of(layer))

    def kl_grads(sub):
        AC.require(layer, sub)
        bt.set_sample_index(layer, S)
        kl = layer.kl_loss()
        assert kl.grad_fn is not None and type(kl.grad_fn).__name__.startswith(_kl_fn_name(kind)), kl.grad_fn
        p = AC.params_of(layer)
        return kl, dict(zip(sub, torch.autograd.grad(kl, [p[n] for n in sub], allow_unused=True)))
    kl_all, g_all = kl_grads(names)
    notes = AC.Notes("%s S1" % _kl_fn_name(kind))
    for sub in (("mu",), ("rho",), ("mu_b",), ("rho_b",), ("mu", "mu_b"), ("rho", "rho_b")):
        kl, g = kl_grads(sub)
        notes.bits("{%s} kl" % "+".join(sub), kl, kl_all)
        for n in sub:
            notes.bits("{%s} d%s" % ("+".join(sub), n), g[n], g_all[n])
    notes.done()


# ---- S2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", BITS_ONLY, ids=[_vid(v) for v in BITS_ONLY])
def test_s2_backward_regenerates_the_noise_of_its_own_forward(v):
    AC.s2_forward_identity(_builder(v), _vid(v))


# left out of the device-word form: L2, C4, C5 and C6 — Flipout layers whose backward needs the sign TENSORS (padded layouts; the bias
# gradient of a transposed layer), which are keyed on the host: materialize_noise refuses them under a device word, as a captured step does
WORDS = [v for v in BITS_ONLY if v[0] not in ("L2", "C4", "C5", "C6")]


@pytest.mark.parametrize("v", WORDS, ids=[_vid(v) for v in WORDS])
def test_s2_backward_reads_the_device_word_its_own_forward_read(v):
    AC.s2_forward_identity(_builder(v), _vid(v), words=True)


@pytest.mark.parametrize("i", [0, 1], ids=["D1-element", "D1-channel"])
@pytest.mark.parametrize("words", [False, True], ids=["host", "words"])
def test_s2_dropout(i, words):
    AC.s2_forward_identity(_dropout_builder(i), "D1-%d" % i, words=words)


def test_s2_sampled_kl_draws_at_the_index_of_the_forward_that_consumed_it():
    import bayesian_torch_amd as bt
    layer, x = _kl_layer("mc")
    names = tuple(AC.params_of(layer))
    AC.require(layer, names)
    p = AC.params_of(layer)
    order = [p[n] for n in names]

    def lone(s):
        bt.set_sample_index(layer, s)
        layer(x)
        kl = layer.kl_loss()
        return kl.detach().clone(), torch.autograd.grad(kl, order)
    kl_a0, ga0 = lone(S)
    kl_b0, gb0 = lone(S + 1)
    bt.set_sample_index(layer, S)
    layer(x)
    kl_a = layer.kl_loss()
    layer(x)
    kl_b = layer.kl_loss()
    assert layer._btx_sample == S + 2
    bt.set_sample_index(layer, 77)
    gb = torch.autograd.grad(kl_b, order)
    ga = torch.autograd.grad(kl_a, order)
    notes = AC.Notes("KlMcFn S2")
    notes.bits("kl first", kl_a, kl_a0)
    notes.bits("kl second", kl_b, kl_b0)
    assert float(kl_a0) != float(kl_b0), "the two draws are the same"
    for n, a, a0, b, b0 in zip(names, ga, ga0, gb, gb0):
        notes.bits("first d%s" % n, a, a0)
        notes.bits("second d%s" % n, b, b0)
    notes.done()


# ---- S3 ------------------------------------------------------------------------------------------------------------------------
S3 = [v for v in VARIANTS if v[0] in ("L1", "C1", "C3", "C4") or (v[0] == "R1" and v[3])]


@pytest.mark.parametrize("v", S3, ids=[_vid(v) for v in S3])
def test_s3_a_seed_change_between_forward_and_backward_does_not_change_the_noise(v):
    AC.s3_seed_change(_builder(v), _vid(v))


@pytest.mark.parametrize("i", [0, 1], ids=["D1-element", "D1-channel"])
def test_s3_dropout(i):
    AC.s3_seed_change(_dropout_builder(i), "D1-%d" % i)


# ---- S4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS, ids=[_vid(v) for v in VARIANTS])
def test_s4_every_form_of_dy_has_the_bits_of_the_dense_one(v):
    # C6: the bias gradients of a transposed layer are torch's own sums over dy, whose order follows dy's memory layout
    AC.s4_dy_forms(_builder(v), _vid(v), _ref64(v), v[1], nchw=v[3] is not False, inexact=_inexact(v),
                   nchw_inexact=("mu_b", "rho_b") if v[0] == "C6" else ())


@pytest.mark.parametrize("i", [0, 1], ids=["D1-element", "D1-channel"])
def test_s4_dropout(i):
    AC.s4_dy_forms(_dropout_builder(i), "D1-%d" % i, nchw=False)


def test_s4_batchnorm_and_maxpool():
    from test_gpu_alignment import off_grid
    names = ("x", "res", "gamma", "beta")
    z, leaves = _bn_pool(names)
    order = [leaves[n] for n in names]
    notes = AC.Notes("B1 S4")
    dense1 = AC.grads(z, leaves, torch.ones_like(z), retain=True)
    got = dict(zip(names, torch.autograd.grad(z.sum(), order, retain_graph=True)))
    for n in names:
        notes.bits("stride-0 dy d%s" % n, got[n], dense1[n])
    dz = AC.tensor(tuple(z.shape), F32, 12, z.device)
    dense = AC.grads(z, leaves, dz, retain=True)
    got = AC.grads(z, leaves, off_grid(dz, 4), retain=True)
    for n in names:
        notes.bits("off-grid dy d%s" % n, got[n], dense[n])
    got = dict(zip(names, torch.autograd.grad((z * dz.contiguous()).sum(), order)))
    for n in names:
        notes.bits("NCHW-contiguous dy d%s" % n, got[n], dense[n])
    notes.done()


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_s4_fused_lstm(cls):
    from test_gpu_alignment import off_grid
    layer = _lstm(cls)
    hs, cs, leaves = _lstm_forward(layer, LSTM_NAMES)
    order = [leaves[n] for n in LSTM_NAMES]
    notes = AC.Notes("T1 %s S4" % cls)
    dense1 = dict(zip(LSTM_NAMES, torch.autograd.grad([hs, cs], order, [torch.ones_like(hs), torch.ones_like(cs)], retain_graph=True)))
    got = dict(zip(LSTM_NAMES, torch.autograd.grad(hs.sum() + cs.sum(), order, retain_graph=True)))
    for n in LSTM_NAMES:
        notes.bits("stride-0 dy d%s" % n, got[n], dense1[n])
    d_hs, d_cs = AC.tensor(tuple(hs.shape), F32, 12, hs.device), AC.tensor(tuple(cs.shape), F32, 13, cs.device)
    dense = _lstm_grads(hs, cs, leaves, retain=True)
    got = dict(zip(LSTM_NAMES, torch.autograd.grad([hs, cs], order, [off_grid(d_hs, 4), off_grid(d_cs, 4)])))
    for n in LSTM_NAMES:
        notes.bits("off-grid dy d%s" % n, got[n], dense[n])
    notes.done()


# ---- S5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", BITS_ONLY, ids=[_vid(v) for v in BITS_ONLY])
def test_s5_retained_graph_and_accumulation(v):
    AC.s5_retain_and_accumulate(_builder(v), _vid(v))


# ---- S6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [AC.L1SQ, AC.BY_ID["C1"]], ids=["L1sq", "C1"])
def test_s6_a_layer_applied_twice_in_one_graph(case):
    AC.s6_applied_twice(lambda: AC.build(case), case.id, AC.ref64_twice())


# ---- S7 ------------------------------------------------------------------------------------------------------------------------
def _second_order_graphs():
    """(name of the Function, output, an input it depends on)"""
    import bayesian_torch_amd as bt
    for cid, fused in (("L1", None), ("C1", None), ("R1", True), ("R2", True)):
        layer, x = AC.build(AC.BY_ID[cid], fused=fused)
        bt.set_sample_index(layer, S)
        out, leaves = AC.forward(layer, x, AC.present(layer))
        yield ("LrtFn" if fused else "ContractFn"), out, leaves["x"]
    for kind in ("gauss", "mc", "logu"):
        layer, _ = _kl_layer(kind)
        AC.require(layer, tuple(AC.params_of(layer)))
        yield _kl_fn_name(kind), layer.kl_loss(), layer._w()[0]
    hs, cs, leaves = _lstm_forward(_lstm("LSTMFlipout"), LSTM_NAMES)
    yield "LstmTrainFn", hs, leaves["x"]
    layer, x = _dropouts()[1]
    out, leaves = AC.forward(layer, x, ("x",))
    yield "DropoutFn", out, leaves["x"]
    from bayesian_torch_amd import autograd as AG
    dev = AC.dev()
    bn = torch.nn.BatchNorm2d(16).to(dev).train()
    xb = AC.tensor((2, 16, 7, 7), F32, 11, dev).requires_grad_(True)
    yb = AG.bn_act(bn, xb, relu=True)
    yield "BatchNormTrainFn", yb, xb
    xp = AC.tensor((2, 16, 7, 7), F32, 11, dev).requires_grad_(True)
    mp = torch.nn.MaxPool2d(3, 2, 1)
    assert AG.max_pool_train_usable(mp, xp)
    yield "MaxPool2dTrainFn", AG.max_pool_train(mp, xp), xp


def test_s7_second_order_is_refused_by_every_function():
    """the gradient penalty's call — torch.autograd.grad(out.sum(), x, create_graph=True), then a backward through the result — raises;
    it never returns constants"""
    seen = []
    for name, out, inp in _second_order_graphs():
        assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith(name), (name, out.grad_fn)
        with pytest.raises(RuntimeError, match="first-order only"):
            (g,) = torch.autograd.grad(out.sum(), inp, create_graph=True)
            g.square().sum().backward()
        with pytest.raises(RuntimeError, match="first-order only"):
            dy = torch.ones_like(out).requires_grad_(True)   # a dy that itself carries a graph
            (g,) = torch.autograd.grad(out, inp, dy, create_graph=True)
            g.square().sum().backward()
        seen.append(name)
    assert set(seen) == {"ContractFn", "LrtFn", "KlFn", "KlMcFn", "KlLogUFn", "LstmTrainFn", "DropoutFn", "BatchNormTrainFn",
                         "MaxPool2dTrainFn"}, seen
    print("S7: create_graph=True raises for %s" % ", ".join(sorted(set(seen))))


# ---- S8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,fused", [("L1", None), ("C1", None), ("R1", True)], ids=["ContractFn-L1", "ContractFn-C1", "LrtFn-R1"])
def test_s8_in_place_updates_between_forward_and_backward(cid, fused):
    import bayesian_torch_amd as bt
    layer, x = AC.build(AC.BY_ID[cid], fused=fused)
    names = AC.present(layer)
    dy = AC.dy_for(layer, x)
    bt.set_sample_index(layer, S)
    out, leaves = AC.forward(layer, x, names)
    with torch.no_grad():
        layer.mu_bias.add_(1)            # not saved, not needed: no error, and the gradients are those of the untouched step
    got = AC.grads(out, leaves, dy)
    with torch.no_grad():
        layer.mu_bias.sub_(1)
    _, want = AC.step(layer, x, names, dy, S)
    notes = AC.Notes("%s S8" % cid)
    for n in names:
        notes.bits("after mu_bias.add_(1) d%s" % n, got[n], want[n])
    notes.done()
    bt.set_sample_index(layer, S)
    out, leaves = AC.forward(layer, x, names)
    with torch.no_grad():
        layer._w()[0].add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        AC.grads(out, leaves, dy)


def test_s8_in_place_update_of_an_lstm_parameter_is_caught():
    layer = _lstm("LSTMReparameterization")
    hs, cs, leaves = _lstm_forward(layer, LSTM_NAMES)
    with torch.no_grad():
        layer.hh.mu_weight.add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        _lstm_grads(hs, cs, leaves)


# ---- S9 ------------------------------------------------------------------------------------------------------------------------
def _linear_block():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(3)
    net = torch.nn.Sequential(L.LinearFlipout(24, 16), torch.nn.ReLU(), L.LinearFlipout(16, 8)).to(AC.dev()).train()
    for m in net:
        m.dnn_to_bnn_flag = True
    bt.assign_layer_ids(net)
    return net, AC.tensor((5, 24), F32, 11, AC.dev(), 1.5)


def _conv_block():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    c1 = AC.BY_ID["C1"]
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(3)
    net = torch.nn.Sequential(getattr(L, c1.cls)(**c1.kw), torch.nn.ReLU(), bt.MCDropout2d(0.3), getattr(L, c1.cls)(**c1.kw)).to(AC.dev()).train()
    for m in net:
        m.dnn_to_bnn_flag = True
    bt.assign_layer_ids(net)
    return net, AC.tensor(c1.xshape, F32, 11, AC.dev(), 1.5)


def _ckpt(net, x):
    from bayesian_torch_amd.utils import checkpoint
    return checkpoint(net, x)


@pytest.mark.parametrize("block", [_linear_block, _conv_block], ids=["linear", "conv-dropout"])
def test_s9_checkpointed_block_has_the_bits_of_the_plain_step(block):
    AC.s9_checkpoint(block, "block %s" % block.__name__.strip("_"), _ckpt)


def test_s9_plain_torch_checkpoint_redraws_the_noise():
    """what the wrapper is for: under torch.utils.checkpoint alone the recomputation draws another sample (documented in INTEGRATION.md)"""
    import torch.utils.checkpoint as tcp
    with pytest.raises(AssertionError, match="not the same bits|counters"):
        AC.s9_checkpoint(_linear_block, "plain torch checkpoint", lambda net, x: tcp.checkpoint(net, x, use_reentrant=False))


# ---- S10 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_opt", [False, True], ids=["no-optimizer", "adam"])
def test_s10_captured_step_with_frozen_parameters(with_opt):
    """the model of test_captured_training_step_equals_the_eager_step (a converted ResNet18 on its 4 x 3 x 224 x 224 batch) with conv1 fully
    frozen and layer2[0].conv1 trained on rho only: a replay equals the eager step under that test's bars, frozen parameters keep
    grad None and their bits"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = AC.dev()
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(0)
    m = resnet.resnet18()
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=False, moped_delta=0.5))
    m = m.to(dev).train()
    bt.assign_layer_ids(m)
    hip_batchnorm(m)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 0.0
    frozen = [m.conv1.mu_kernel, m.conv1.rho_kernel, m.layer2[0].conv1.mu_kernel]
    for p in frozen:
        p.requires_grad_(False)
    torch.manual_seed(1)
    x = torch.randn(4, 3, 224, 224, device=dev)
    t = torch.randint(0, 1000, (4,), device=dev)
    watched = (m.layer2[0].conv1.rho_kernel, m.layer1[0].conv1.mu_kernel, m.layer4[1].conv2.mu_kernel, m.fc.rho_weight, m.fc.rho_bias,
               m.bn1.weight)

    def eager(s):
        for p_ in m.parameters():
            p_.grad = None
        bt.set_sample_index(m, s)
        out = m(x)
        loss = torch.nn.functional.cross_entropy(out.float(), t) + bt.get_kl_loss(m) / 4
        loss.backward()
        assert all(p_.grad is None for p_ in frozen)
        return float(loss), [p_.grad.detach().clone() for p_ in watched]
    l7, g7 = eager(7)
    before = [p.detach().clone() for p in frozen]
    trained = m.fc.rho_weight.detach().clone()
    opt = bt.optim.Adam(m.parameters(), lr=1e-4) if with_opt else None
    gs = GraphedTrainStep(m, x, t, optimizer=opt)
    try:
        la = float(gs.run(7))
        ga = [p_.grad.detach().clone() for p_ in watched]
        assert all(p_.grad is None for p_ in frozen)
        gs.run(8)
        gs.run(9)
        assert all(p_.grad is None for p_ in frozen)
    finally:
        gs.close()
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    errs = [rel(a, b) for a, b in zip(ga, g7)]
    print("S10 %s: captured vs eager step with frozen parameters: loss %.6f / %.6f, gradient rel-L2 %s" % (
        "adam" if with_opt else "no optimizer", la, l7, ", ".join("%.1e" % e for e in errs)))
    assert abs(la - l7) < 1e-5 * abs(l7)
    assert max(errs) < 1e-5, errs
    for p, b in zip(frozen, before):
        assert E.check_exact(p, b).ok, "a frozen parameter changed"
    assert torch.equal(m.fc.rho_weight.detach(), trained) != with_opt   # the captured Adam moved what is trainable, and only with it
