"""GPU: fused training of the local reparameterization layers — btx_lrt_fwd_train / btx_lrt_bwd behind autograd.LrtFn (DESIGN.md §21
"Backward").  Every gradient element against the float64 model of tests/lrt_bwd_model.py (whose header derives the bounds), fed with
the GPU's own x, g and materialize_noise(...)["zeta"]: the local scheme of tests/test_gpu_lrt.py.

Each envelope check prints `name prec/act: worst err/bound R at index`; profiles/lrt_train_envelope.txt holds the lines of the first run.
"""
import warnings

import numpy as np
import pytest
import torch

import envelope as E
import lrt_bwd_model as BM
import lrt_model as LM
from test_gpu_alignment import off_grid
from test_gpu_lrt import _params_of, _train_net

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

F32, BF16 = torch.float32, torch.bfloat16
PRECS = [("f32", F32), ("bf16", F32), ("bf16", BF16)]   # (contraction precision, activation dtype)
_PID = ["%s-%s" % (p, "bf16" if a is BF16 else "f32") for p, a in PRECS]
SAMPLE = 5

# the smallest shapes that reach every path: ragged N with zeta off the 4-grid; the stride-1 flipped data gradient; the transposed one
# with output padding; the channel-padded stem; no bias
CASES = [
    ("linear_72_50_r37", "LinearLocalReparameterization", dict(in_features=72, out_features=50), (37, 72)),
    ("conv_8_16_p1", "Conv2dLocalReparameterization", dict(in_channels=8, out_channels=16, kernel_size=3, padding=1), (4, 8, 5, 5)),
    ("conv_16_72_s2", "Conv2dLocalReparameterization", dict(in_channels=16, out_channels=72, kernel_size=3, stride=2, padding=1),
     (2, 16, 13, 13)),
    ("conv_3_16_cpad", "Conv2dLocalReparameterization", dict(in_channels=3, out_channels=16, kernel_size=3, padding=1), (2, 3, 7, 7)),
    ("conv_8_16_nobias", "Conv2dLocalReparameterization", dict(in_channels=8, out_channels=16, kernel_size=3, padding=1, bias=False),
     (4, 8, 5, 5)),
]
_CID = [c[0] for c in CASES]
NAMES = ("mu", "rho", "mu_b", "rho_b", "x")


def _dev():
    return torch.device("cuda:0")


def _make(cls, kw, prec, fused=True):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(4321)
    torch.manual_seed(3)
    layer = getattr(L, cls)(**kw)
    with torch.no_grad():   # sigma between 0.007 and 0.7: the noise term is neither negligible nor dominant
        layer._w()[1].uniform_(-5.0, 0.0)
        if layer.rho_bias is not None:
            layer.rho_bias.uniform_(-3.0, 0.0)
            layer.mu_bias.normal_(0.0, 0.5)
    layer = layer.to(_dev()).train()
    layer.precision, layer.fused_training, layer.dnn_to_bnn_flag = prec, fused, True
    return layer


def _t(shape, act, seed, ints=False, scale=1.5):
    if ints:
        t = E.small_ints(shape, seed)
    else:
        t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale
    t = t.to(_dev()).to(act)
    return t.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else t


def _run(layer, x, g):
    """one fused forward + backward at sample SAMPLE -> (out, {name: gradient})"""
    import bayesian_torch_amd as bt
    for p in layer.parameters():
        p.grad = None
    x = x.detach().requires_grad_()
    bt.set_sample_index(layer, SAMPLE)
    out = layer(x)
    out.backward(g)
    torch.cuda.synchronize()
    mu, rho = layer._w()
    got = dict(mu=mu.grad, rho=rho.grad, x=x.grad)
    if layer.mu_bias is not None:
        got.update(mu_b=layer.mu_bias.grad, rho_b=layer.rho_bias.grad)
    return out.detach(), got


def _model(layer, x, g, out_shape, prec, act):
    with torch.no_grad():
        zeta = layer.materialize_noise(SAMPLE, out_shape=tuple(out_shape))["zeta"]
    mu, rho, mb, rb = LM.layer_arrays(layer)
    return BM.backward(x.float().cpu().numpy(), g.float().cpu().numpy(), zeta.float().cpu().numpy(), mu, rho, mb, rb,
                       LM.op_of(layer), prec=prec, act_bf16=act is BF16)


_CACHE = {}


def _case(ci, pi):
    """(layer, x, g, out, gradients, model) of one case and precision: computed once, shared by the tests that only read it"""
    key = (ci, pi)
    if key not in _CACHE:
        name, cls, kw, xs = CASES[ci]
        prec, act = PRECS[pi]
        layer = _make(cls, kw, prec)
        x = _t(xs, act, seed=11)
        with torch.no_grad():
            oshape = layer._forward_hip(x, sample_idx=SAMPLE).shape
        g = _t(tuple(oshape), act, seed=12, scale=1.0)
        out, got = _run(layer, x, g)
        _CACHE[key] = dict(layer=layer, x=x, g=g, out=out, got=got, model=_model(layer, x, g, oshape, prec, act))
    return _CACHE[key]


def _tag(pi):
    return "%s/%s" % (PRECS[pi][0], "bf16" if PRECS[pi][1] is BF16 else "f32")


# 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(3), ids=_PID)
def test_switch_on_never_enters_the_composite_on_covered_shapes(pi, monkeypatch):
    """with fused_training on, forward + backward of every covered shape runs without _lrt_composite (it raises here); a Conv1d layer
    is not covered and still enters it"""
    from bayesian_torch_amd import functional as BF, layers as L
    from bayesian_torch_amd.layers.base_variational_layer import _VariationalNd
    prec, act = PRECS[pi]

    def boom(self, *a, **k):
        raise AssertionError("the ATen composite was entered")
    monkeypatch.setattr(_VariationalNd, "_lrt_composite", boom)
    for name, cls, kw, xs in CASES:
        layer = _make(cls, kw, prec)
        x = _t(xs, act, seed=11).requires_grad_()
        assert BF.lrt_train_ok(layer, x), name
        out = layer(x)
        out.float().square().sum().backward()
        torch.cuda.synchronize()
        for p in layer.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
        assert x.grad is not None and x.grad.shape == x.shape and torch.isfinite(x.grad.float()).all()
    c1 = _make("Conv1dLocalReparameterization", dict(in_channels=8, out_channels=16, kernel_size=5), prec)
    x1 = _t((2, 8, 40), act, seed=2).requires_grad_()
    assert not BF.lrt_train_ok(c1, x1)
    with pytest.raises(AssertionError, match="composite was entered"):
        c1(x1)
    assert isinstance(c1, L.Conv1dLocalReparameterization)


# 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(3), ids=_PID)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=_CID)
def test_training_forward_is_the_inference_launch_bit_for_bit_and_saves_the_root(ci, pi):
    from bayesian_torch_amd import functional as BF, rng
    c = _case(ci, pi)
    layer, x = c["layer"], c["x"]
    prec, act = PRECS[pi]
    with torch.no_grad():
        want = layer._forward_hip(x, sample_idx=SAMPLE)
    assert c["out"].dtype == act and torch.equal(c["out"], want)
    op = layer._op
    mu_p, rho_p = BF.gemm_major_view(layer._w()[0], op), BF.gemm_major_view(layer._w()[1], op)
    xin = x
    if layer._btx_cpad is not None:
        extra = layer._btx_cpad - op.in_channels
        xin, op = BF.pad_channels(x, op, extra), layer._op_pad
        mu_p, rho_p = torch.nn.functional.pad(mu_p, (0, extra)), torch.nn.functional.pad(rho_p, (0, extra))
    mb = layer.mu_bias.detach() if layer.mu_bias is not None else None
    rb = layer.rho_bias.detach() if layer.rho_bias is not None else None
    out2, root = BF.lrt_fwd_train_hip(xin, mu_p, rho_p, mb, rb, op, rng.seed(), SAMPLE, layer._btx_layer_id, prec=prec)
    torch.cuda.synchronize()
    assert torch.equal(out2, want)
    r64 = c["model"]["root"]
    root_l = root.reshape(want.shape) if want.dim() == 2 else root.reshape(want.shape[0], want.shape[2], want.shape[3],
                                                                            want.shape[1]).permute(0, 3, 1, 2)
    rep = E.check(root_l.cpu().numpy(), r64, c["model"]["c_r"] * r64)
    print(rep.line("root_" + CASES[ci][0], _tag(pi)))
    assert rep.ok, str(rep)
    assert r64.max() > 0


# 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(3), ids=_PID)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=_CID)
def test_every_gradient_element_inside_the_model_bound(ci, pi):
    c = _case(ci, pi)
    ref, bnd, got = c["model"]["ref"], c["model"]["bound"], c["got"]
    assert set(got) == set(ref)
    for q in NAMES:
        if q not in ref:
            continue
        assert got[q].dtype == (PRECS[pi][1] if q == "x" else F32) and tuple(got[q].shape) == ref[q].shape
        rep = E.check(got[q].float().cpu().numpy(), ref[q], bnd[q])
        print(rep.line("%s_d%s" % (CASES[ci][0], q), _tag(pi)))
        assert rep.ok, (q, str(rep))
        assert np.abs(ref[q]).max() > 0
    # the bound is sharp enough to see the noise path
    assert not E.check(np.zeros_like(ref["rho"]), ref["rho"], bnd["rho"]).ok


# 4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(3), ids=_PID)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=_CID)
def test_small_integer_inputs_give_dmu_and_dmu_b_bit_for_bit(ci, pi):
    name, cls, kw, xs = CASES[ci]
    prec, act = PRECS[pi]
    layer = _make(cls, kw, prec)
    x = _t(xs, act, seed=21, ints=True)
    with torch.no_grad():
        oshape = layer._forward_hip(x, sample_idx=SAMPLE).shape
    g = _t(tuple(oshape), act, seed=22, ints=True)
    _, got = _run(layer, x, g)
    op = LM.op_of(layer)
    want = E.wgrad64(x.float().cpu(), g.float().cpu(), tuple(layer._w()[0].shape), op)
    rep = E.check_exact(got["mu"].cpu().numpy(), want.numpy())
    assert rep.ok and want.abs().max() > 0, str(rep)
    if layer.mu_bias is not None:
        red = [d for d in range(g.dim()) if d != (1 if g.dim() > 2 else g.dim() - 1)]
        wb = g.double().cpu().sum(red)
        assert E.check_exact(got["mu_b"].cpu().numpy(), wb.numpy()).ok and wb.abs().max() > 0


# 5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(3), ids=_PID)
def test_zero_variance_rows_give_finite_gradients_and_no_noise_path(pi):
    """all-zero input on the no-bias layer: v == 0 everywhere, the root's gradient is DEFINED as 0 there — every gradient is finite,
    drho is exactly 0 and dx is op^T(g, mu) alone (inside the bound of the mean path: the model's B term has a zero bound)"""
    name, cls, kw, xs = CASES[4]
    prec, act = PRECS[pi]
    layer = _make(cls, kw, prec)
    x = torch.zeros(xs, device=_dev(), dtype=act).contiguous(memory_format=torch.channels_last)
    g = _t((xs[0], 16, xs[2], xs[3]), act, seed=31, scale=1.0)
    out, got = _run(layer, x, g)
    assert torch.equal(out, torch.zeros_like(out))
    for q, t in got.items():
        assert torch.isfinite(t.float()).all(), q
    assert torch.equal(got["rho"], torch.zeros_like(got["rho"])) and torch.equal(got["mu"], torch.zeros_like(got["mu"]))
    m = _model(layer, x, g, out.shape, prec, act)
    assert (m["bound"]["rho"] == 0).all()
    mu = LM.layer_arrays(layer)[0]
    mu_d = LM.rbf16(mu) if prec == "bf16" else mu
    g_d = LM.rbf16(g.float().cpu().numpy()) if prec == "bf16" else g.float().cpu().numpy()
    a_only = BM._dgrad64(BM._t(g_d), tuple(xs), BM._t(mu_d), LM.op_of(layer)).numpy()
    assert np.array_equal(m["ref"]["x"], a_only) and np.abs(a_only).max() > 0
    rep = E.check(got["x"].float().cpu().numpy(), a_only, m["bound"]["x"])
    print(rep.line("zero_variance_dx", _tag(pi)))
    assert rep.ok, str(rep)


def _direct(layer, x, g, root, prec, **kw):
    """btx_lrt_bwd through functional.lrt_bwd_hip on the layer's plain geometry"""
    from bayesian_torch_amd import functional as BF, rng
    op = layer._op
    mu_p, rho_p = BF.gemm_major_view(layer._w()[0], op), BF.gemm_major_view(layer._w()[1], op)
    rb = layer.rho_bias.detach() if layer.rho_bias is not None else None
    return BF.lrt_bwd_hip(x, g, root, mu_p, rho_p, rb, op, rng.seed(), SAMPLE, layer._btx_layer_id, prec=prec, **kw)


def _root_of(layer, x, prec):
    from bayesian_torch_amd import functional as BF, rng
    op = layer._op
    mu_p, rho_p = BF.gemm_major_view(layer._w()[0], op), BF.gemm_major_view(layer._w()[1], op)
    mb = layer.mu_bias.detach() if layer.mu_bias is not None else None
    rb = layer.rho_bias.detach() if layer.rho_bias is not None else None
    return BF.lrt_fwd_train_hip(x, mu_p, rho_p, mb, rb, op, rng.seed(), SAMPLE, layer._btx_layer_id, prec=prec)


# 6 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(3), ids=_PID)
@pytest.mark.parametrize("ci", (0, 1, 2), ids=_CID[:3])
def test_two_backward_calls_give_identical_bits(ci, pi):
    c = _case(ci, pi)
    prec = PRECS[pi][0]
    with torch.no_grad():
        _, root = _root_of(c["layer"], c["x"], prec)
        a = _direct(c["layer"], c["x"], c["g"], root, prec)
        b = _direct(c["layer"], c["x"], c["g"], root, prec)
    torch.cuda.synchronize()
    for q, (ta, tb) in enumerate(zip(a, b)):
        assert ta is not None and torch.equal(ta, tb), q
    # ... and they are the gradients autograd returned
    lay = c["layer"]
    from bayesian_torch_amd import functional as BF
    assert torch.equal(BF.gemm_major_logical_view(a[1], tuple(lay._w()[0].shape), lay._op), c["got"]["mu"])
    assert torch.equal(a[0].reshape(c["got"]["x"].shape), c["got"]["x"])


# 7 ----------------------------------------------------------------------------------------------------------------------------
def _slack_untouched(v):
    full = torch.empty(0, dtype=v.dtype, device=v.device).set_(v.untyped_storage())
    off, n = v.storage_offset(), v.numel()   # (dense views: the elements of v are [off, off + n) of the buffer)
    return bool(full[:off].isnan().all()) and bool(full[off + n:].isnan().all())


@pytest.mark.parametrize("pi", range(3), ids=_PID)
@pytest.mark.parametrize("ci", (0, 1, 2), ids=_CID[:3])
def test_off_grid_tensors_take_the_slow_path_and_stay_inside_the_bound(ci, pi):
    """x, dy, root and dx 4 (f32) / 2 (bf16) bytes past a 16-byte boundary: the calls return 0 (never BTX_E_ALIGN), nothing outside the
    outputs is written and every gradient stays inside the model's bound"""
    from bayesian_torch_amd import functional as BF
    c = _case(ci, pi)
    prec, act = PRECS[pi]
    lay = c["layer"]
    nb = 2 if act is BF16 else 4
    xo, go = off_grid(c["x"], nb), off_grid(c["g"], nb)
    with torch.no_grad():
        _, root = _root_of(lay, xo, prec)
        ro = off_grid(root, 4)
        dxo = off_grid(torch.full_like(xo, float("nan")), nb)   # (the view itself holds NaN until the call fills it)
        dx, dmu, drho, dmu_b, drho_b = _direct(lay, xo, go, ro, prec, out_dx=dxo)
    torch.cuda.synchronize()
    assert dx.data_ptr() == dxo.data_ptr() and dx.data_ptr() % 16 == nb
    assert torch.isfinite(dxo.float()).all() and _slack_untouched(dxo) and _slack_untouched(ro) and _slack_untouched(go)
    ref, bnd = c["model"]["ref"], c["model"]["bound"]
    wshape = tuple(lay._w()[0].shape)
    got = dict(x=dx.reshape(c["x"].shape), mu=BF.gemm_major_logical_view(dmu, wshape, lay._op),
               rho=BF.gemm_major_logical_view(drho, wshape, lay._op), mu_b=dmu_b, rho_b=drho_b)
    for q in NAMES:
        rep = E.check(got[q].float().cpu().numpy(), ref[q], bnd[q])
        print(rep.line("offgrid_%s_d%s" % (CASES[ci][0], q), _tag(pi)))
        assert rep.ok, (q, str(rep))


# 8 ----------------------------------------------------------------------------------------------------------------------------
def test_graphed_num_mc_2_step_equals_the_eager_fused_step_bit_for_bit():
    """GraphedTrainStep(num_mc=2, optimizer=SGD) on the _TrainNet shapes with the switch on: one replay leaves every parameter bit-equal
    to the eager fused mc_train_forward step on the same sample indices (each backward regenerates the zeta of the device word ITS
    forward read), and a second replay changes the loss"""
    from bayesian_torch_amd import autograd as AG, optim
    from bayesian_torch_amd.layers.base_variational_layer import _VariationalNd
    net = _train_net()
    net.conv.fused_training = net.fc.fused_training = True
    x = _t((4, 8, 5, 5), F32, seed=3)
    y = torch.tensor([1, 0, 7, 3], device=x.device)
    lr = 0.05
    loss_fn = lambda out, tgt: torch.nn.functional.cross_entropy(out.mean(0), tgt)  # noqa: E731
    layers = (("conv", net.conv), ("fc", net.fc))
    p0 = {n: _params_of(l) for n, l in layers}
    entered = []
    orig = _VariationalNd._lrt_composite
    _VariationalNd._lrt_composite = lambda self, *a, **k: (entered.append(1), orig(self, *a, **k))[1]
    try:
        step = AG.GraphedTrainStep(net, x, y, loss_fn=loss_fn, optimizer=optim.SGD(net.parameters(), lr=lr), num_mc=2)
        try:
            loss1 = float(step.run(3))
            torch.cuda.synchronize()
            graphed = {n: _params_of(l) for n, l in layers}
            loss2 = float(step.run(4))
            torch.cuda.synchronize()
            assert np.isfinite(loss1) and np.isfinite(loss2) and loss2 != loss1
        finally:
            step.close()
        with torch.no_grad():
            for n, l in layers:
                mu, rho = l._w()
                for p, k in ((mu, "mu"), (rho, "rho"), (l.mu_bias, "mu_b"), (l.rho_bias, "rho_b")):
                    p.copy_(p0[n][k])
                    p.grad = None
        opt = optim.SGD(net.parameters(), lr=lr)
        loss = loss_fn(AG.mc_train_forward(net, x, 2, 3), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    finally:
        _VariationalNd._lrt_composite = orig
    assert not entered
    assert float(loss.detach()) == loss1
    for n, l in layers:
        now = _params_of(l)
        for k in ("mu", "rho", "mu_b", "rho_b"):
            assert torch.equal(now[k], graphed[n][k]), (n, k)
            assert not torch.equal(now[k], p0[n][k]), (n, k)


# 9 ----------------------------------------------------------------------------------------------------------------------------
def test_fuse_model_lrt_training_one_eager_step_of_a_small_net():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import fuse_model
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    bt.manual_seed(5)
    torch.manual_seed(1)
    conv, fc = L.Conv2dLocalReparameterization(3, 16, 3, padding=1), L.LinearLocalReparameterization(16 * 6 * 6, 10)
    conv.dnn_to_bnn_flag = fc.dnn_to_bnn_flag = True
    net = torch.nn.Sequential(conv, torch.nn.BatchNorm2d(16), torch.nn.ReLU(), torch.nn.Flatten(), fc).to(_dev())
    fuse_model(net, lrt_training=True)
    net.train()
    assert conv.fused_training and fc.fused_training
    x = _t((4, 3, 6, 6), F32, seed=9)
    y = torch.tensor([1, 0, 7, 3], device=x.device)
    bt.set_sample_index(net, 2)
    loss = torch.nn.functional.cross_entropy(net(x), y) + get_kl_loss(net) / 4
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for n, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
