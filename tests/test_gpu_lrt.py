"""GPU: the local reparameterization layers (BTX_KIND_LRT) — every element against float64, an exact run, MC sample
lanes, the inference drivers, the fused epilogue and training.

The reference of the forward checks is tests/lrt_model.py: m64 + sqrt(v64) * zeta built on the CPU from the layer's parameters with
the operands as BTX-LRT v1 rounds them, zeta fetched through btx_fill_eps(stream 4) at the same seed, layer id and sample.  Its
header derives the bound |got - ref| <= c_m A_m + |zeta| sqrt(v64) c_v + u_out |ref| and says why a wrong zeta index, a swapped
accumulator or a missing bias variance land far outside it (test_lrt_cpu.py pins that with perturbed references).

Each envelope check prints `name prec/act: worst err/bound R at index`; profiles/lrt_envelope.txt holds the lines of the first run.
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import envelope as E
import lrt_model as LM

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

F32, BF16 = torch.float32, torch.bfloat16
PRECS = [("f32", F32), ("bf16", F32), ("bf16", BF16)]   # (contraction precision, activation dtype)
_PID = ["%s-%s" % (p, "bf16" if a is BF16 else "f32") for p, a in PRECS]

# (name, class, kwargs, input shape, family the aligned launch must take per precision)
CASES = [
    ("linear_72_50_r37", "LinearLocalReparameterization", dict(in_features=72, out_features=50), (37, 72), "regstage"),
    ("linear_70_130_r300", "LinearLocalReparameterization", dict(in_features=70, out_features=130), (300, 70), "regstage"),
    ("conv2d_16_72_s2", "Conv2dLocalReparameterization", dict(in_channels=16, out_channels=72, kernel_size=3, stride=2, padding=1),
     (2, 16, 13, 13), "regstage"),
    ("conv2d_16_24_d2_g2", "Conv2dLocalReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, dilation=2, groups=2),
     (2, 16, 9, 9), "regstage"),
    ("conv2d_dw_8", "Conv2dLocalReparameterization", dict(in_channels=8, out_channels=8, kernel_size=3, padding=1, groups=8),
     (2, 8, 7, 7), "gather"),
    ("conv1d_8_16_k5_nobias", "Conv1dLocalReparameterization", dict(in_channels=8, out_channels=16, kernel_size=5, bias=False),
     (2, 8, 40), "regstage"),
    ("conv3d_8_8", "Conv3dLocalReparameterization", dict(in_channels=8, out_channels=8, kernel_size=(2, 3, 3), prior_mean=0.0,
                                                         prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0),
     (2, 8, 4, 6, 6), "regstage"),
]
FAMILY = {0: "gather", 1: "regstage"}


def _dev():
    return torch.device("cuda:0")


def _make(cls, kw, prec, seed=3, bt_seed=1234):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(bt_seed)
    torch.manual_seed(seed)
    layer = getattr(L, cls)(**kw)
    with torch.no_grad():   # sigma between 0.007 and 0.7: the noise term is neither negligible nor dominant
        layer._w()[1].uniform_(-5.0, 0.0)
        if layer.rho_bias is not None:
            layer.rho_bias.uniform_(-3.0, 0.0)
            layer.mu_bias.normal_(0.0, 0.5)
    layer = layer.to(_dev()).eval()
    layer.precision = prec
    return layer


def _x(shape, act, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * 1.5).to(_dev()).to(act)
    if len(shape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    return x


def _plan(layer, xshape, prec, act):
    """(rc, BtxPlanInfo) of the kind-2 launch the layer makes on an input of shape xshape"""
    from bayesian_torch_amd import _lib
    op = layer._op_pad if layer._btx_cpad is not None else layer._op
    g = _lib.Geom()
    sp = (1, 1, 1) if op.nd == 0 else (1,) * (3 - op.nd) + tuple(xshape[2:])
    nb = int(np.prod(xshape[:-1])) if op.nd == 0 else xshape[0]
    g.NB, (g.D, g.H, g.W), g.C, g.N = nb, sp, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.groups = op.groups
    info = _lib.PlanInfo()
    rc = _lib.lib().btx_contract_plan_info(_lib.KIND_LRT, ctypes.byref(g), _lib.ACT_BF16 if act is BF16 else _lib.ACT_F32,
                                           _lib.PREC_CODE[prec], 0, None, ctypes.byref(info))
    return rc, info


def _reference(layer, x, zeta, prec, act):
    mu, rho, mb, rb = LM.layer_arrays(layer)
    return LM.forward(x.float().cpu().numpy(), mu, rho, mb, rb, zeta.float().cpu().numpy(), LM.op_of(layer), prec=prec,
                      store_bf16=act is BF16)


def _check(name, prec, act, got, r, ref=None, bnd=None):
    rep = E.check(got.float().cpu().numpy(), r["ref"] if ref is None else ref, r["bound"] if bnd is None else bnd)
    print(rep.line(name, "%s/%s" % (prec, "bf16" if act is BF16 else "f32")))
    assert rep.ok, (name, prec, str(rep))
    return rep


# =============================================================================================================================
# 1. every element against float64
# =============================================================================================================================
@pytest.mark.parametrize("prec,act", PRECS, ids=_PID)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_every_element_inside_the_float64_envelope(case, prec, act):
    """A wrong zeta index replaces zeta by an independent draw (an error of the order of sqrt(v) |zeta| against a bound of c_v ~ 2^-8
    or less of it), swapped accumulators give v + sqrt(m) zeta, a missing bias variance shrinks the root by sigma_b^2 / 2v relative
    (sigma_b is up to 0.7 here): each is orders of magnitude outside.  The planner must put the launch where the case says."""
    name, cls, kw, xs, fam = case
    layer = _make(cls, kw, prec)
    rc, info = _plan(layer, xs, prec, act)
    assert rc == 0 and FAMILY[info.family] == fam and info.ksplits == 1 and info.ws_bytes == 0, (rc, info.family, info.ksplits)
    x = _x(xs, act)
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=5)
        zeta = layer.materialize_noise(5, out_shape=tuple(out.shape))["zeta"]
    assert out.dtype == act and torch.isfinite(out.float()).all()
    r = _reference(layer, x, zeta, prec, act)
    rep = _check(name, prec, act, out, r)
    # the noise term is really there: without it the output is far outside the same envelope
    assert not E.check(out.float().cpu().numpy(), r["m"], r["bound"]).ok
    assert rep.numel == out.numel()


def _raw_launch(layer, xp, out, sample, prec, nb, spatial):
    """btx_contract_fwd_ex(kind 2) on the physical (channels-last) tensors given, `out` included: no wrapper in between"""
    from bayesian_torch_amd import _lib, functional as BF, rng
    op = layer._op
    mu, rho = layer._w()
    mu_p, rho_p = BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op)
    g = _lib.Geom()
    g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.groups = op.groups
    r = _lib.Rng(int(rng.seed()), int(sample), int(layer._btx_layer_id), None)
    act = _lib.ACT_BF16 if xp.dtype is BF16 else _lib.ACT_F32
    mb, rb = layer.mu_bias, layer.rho_bias
    return _lib.lib().btx_contract_fwd_ex(_lib.KIND_LRT, ctypes.byref(g), xp.data_ptr(), mu_p.data_ptr(), rho_p.data_ptr(),
                                          mb.data_ptr() if mb is not None else None, rb.data_ptr() if rb is not None else None,
                                          out.data_ptr(), ctypes.byref(r), None, act, _lib.PREC_CODE[prec], 0, None, 0,
                                          torch.cuda.current_stream(xp.device).cuda_stream, None)


@pytest.mark.parametrize("prec,act", PRECS, ids=_PID)
def test_forward_with_x_and_out_off_the_16_byte_grid(prec, act):
    """`x` and `out` are dense views 4 (f32) / 2 (bf16) bytes past a 16-byte boundary: the launch returns 0 (never BTX_E_ALIGN), runs
    on the gather kernel, writes nothing outside `out` (the slack around it keeps its NaN) and stays inside the envelope."""
    from test_gpu_alignment import off_grid
    name, cls, kw, xs, _ = CASES[2]
    layer = _make(cls, kw, prec)
    x = _x(xs, act)
    with torch.no_grad():
        aligned = layer._forward_hip(x, sample_idx=9)
        nbytes = 2 if act is BF16 else 4
        xo = off_grid(x, nbytes)
        out_o = off_grid(torch.zeros_like(aligned), nbytes)
        buf = out_o._base if out_o._base is not None else None
        xp = xo.permute(0, 2, 3, 1)
        assert xp.is_contiguous()
        rc = _raw_launch(layer, xp, out_o, 9, prec, xs[0], (1, xs[2], xs[3]))
        torch.cuda.synchronize()
        assert rc == 0, rc
        zeta = layer.materialize_noise(9, out_shape=tuple(aligned.shape))["zeta"]
    r = _reference(layer, x, zeta, prec, act)
    _check(name + "_offgrid", prec, act, out_o, r)
    if buf is not None:
        inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
        first = (out_o.data_ptr() - buf.data_ptr()) // buf.element_size()
        inside[first:first + out_o.numel()] = True
        assert torch.isnan(buf[~inside].float()).all(), "the launch wrote outside its output"


# =============================================================================================================================
# 2. exact run
# =============================================================================================================================
def _rho_for_sigma_pow2(k):
    """a float32 rho whose softplus IN THE KERNEL is exactly 2^-k (k >= 26), or None.  btx_softplus_fast computes e = exp2(f32(rho *
    f32(log2 e))) and returns e itself once 1 + e rounds to 1; the hardware exp2 of the integer -k is 2^-k.  So rho qualifies when
    the f32 product rho * 0x1.715476p+0 is exactly -k: search the floats around -k ln 2."""
    log2e = np.float32(float.fromhex("0x1.715476p+0"))
    c = np.float32(-k * np.log(2.0))
    cand = c
    for _ in range(64):
        cand = np.nextafter(cand, np.float32(-np.inf))
    for _ in range(129):
        if np.float32(cand * log2e) == np.float32(-k):
            return float(cand)
        cand = np.nextafter(cand, np.float32(np.inf))
    return None


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[CASES[0][0], CASES[2][0]])
def test_exact_run_small_integers(case, prec):
    """x small integers, mu = 0, sigma = 2^-32 exactly (weights and bias): v = 2^-64 (sum x^2 + 1) is exact in f32 whatever the
    precision and the order of the sum, and the output must be f32(sqrtf(v) * zeta) bit for bit — sqrtf correctly rounded, one
    rounding for the product (the store's fused multiply-add has m = 0)."""
    rho0 = _rho_for_sigma_pow2(32)   # (-22.1807098...; k = 30 and 31 have no such float32)
    assert rho0 is not None, "no float32 rho maps onto -32 under the kernel's exp2 argument"
    name, cls, kw, xs, _ = case
    layer = _make(cls, kw, prec)
    with torch.no_grad():
        layer._w()[0].zero_()
        layer._w()[1].fill_(rho0)
        layer.mu_bias.zero_()
        layer.rho_bias.fill_(rho0)
    x = E.small_ints(xs, seed=4).to(_dev())
    if len(xs) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=2)
        zeta = layer.materialize_noise(2, out_shape=tuple(out.shape))["zeta"].cpu().numpy()
    x64 = x.double().cpu()
    ones = torch.ones(tuple(layer._w()[0].shape), dtype=torch.float64)
    v = (E.contract(x64 * x64, ones, torch.ones(ones.shape[0], dtype=torch.float64), LM.op_of(layer)).numpy() * 2.0 ** -64)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    want = (np.sqrt(v32).astype(np.float64) * zeta.astype(np.float64)).astype(np.float32)
    rep = E.check_exact(out.cpu().numpy(), want)
    print(rep.line(name + "_exact", prec))
    assert rep.ok, str(rep)


# =============================================================================================================================
# 3. MC sample lanes
# =============================================================================================================================
# (40 rows: the per-lane output is 40 * 50 * 2 = 4000 bytes, a multiple of 16 — btx_contract_fwd_lanes takes it as ONE launch)
LANE_CASES = [("linear_72_50_r40", CASES[0][1], CASES[0][2], (40, 72), "regstage"), CASES[2]]


@pytest.mark.parametrize("case", LANE_CASES, ids=[c[0] for c in LANE_CASES])
def test_three_lanes_equal_three_single_sample_launches(case):
    from bayesian_torch_amd import functional as BF, rng, _lib
    name, cls, kw, xs, _ = case
    layer = _make(cls, kw, "bf16")
    x = _x(xs, BF16)
    with torch.no_grad():
        probe = layer._forward_hip(x, sample_idx=0)
        assert (probe.numel() * 2) % 16 == 0 and not BF._lanes_refused(_lib.KIND_LRT, layer._op, xs[0], (1, 1, 1) if len(xs) == 2 else
                                                                       (1, xs[2], xs[3]), BF16, None, _lib.PREC_CODE["bf16"], 0, 3)
        singles = [layer._forward_hip(x, sample_idx=40 + l).clone() for l in range(3)]
        op = layer._op
        mu, rho = layer._w()
        out = BF.contract_hip(_lib.KIND_LRT, x, BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op), layer.mu_bias, layer.rho_bias,
                              op, rng.seed(), 40, layer._btx_layer_id, prec="bf16", lanes=3, lane_batch=xs[0])
    assert out.shape[0] == 3 * xs[0]
    for l in range(3):
        assert torch.equal(out[l * xs[0]:(l + 1) * xs[0]], singles[l]), (name, l)
    assert not torch.equal(singles[0], singles[1])


# =============================================================================================================================
# 4. drivers
# =============================================================================================================================
class _Net(torch.nn.Module):
    def __init__(self):
        from bayesian_torch_amd import layers as L
        super().__init__()
        self.conv = L.Conv2dLocalReparameterization(8, 16, 3, padding=1)
        self.fc = L.LinearLocalReparameterization(16 * 6 * 6, 10)
        self.conv.dnn_to_bnn_flag = self.fc.dnn_to_bnn_flag = True

    def forward(self, x):
        h = torch.relu(self.conv(x))
        return self.fc(h.flatten(1))


def _net(seed=2):
    import bayesian_torch_amd as bt
    bt.manual_seed(77)
    torch.manual_seed(seed)
    return _Net().to(_dev()).eval()


def test_mc_forward_and_graphed_mc_lanes_equal_the_eager_loop():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    net = _net()
    x = _x((4, 8, 6, 6), F32, seed=5)
    idx = [10, 11, 12, 13]
    with torch.no_grad():
        eager, packed_ref = [], None
        for s in idx:
            bt.set_sample_index(net, s)
            lg = net(x)
            if packed_ref is None:
                packed_ref = torch.zeros(mc.packed_numel(4, 10), device=x.device)
            mc.accumulate(packed_ref, lg, 0.0)
            eager.append(lg.clone())
        packed = mc.mc_forward(net, x, 4, sample_offset=10, lanes=4, reduce=False)
        assert torch.equal(packed, packed_ref)
        assert torch.equal(mc.mc_forward(net, x, 4, sample_offset=10, lanes=1, reduce=False), packed_ref)
        g = mc.GraphedMC(net, x, kl=0.0, lanes=4, keep_logits=True)
        try:
            g.run_many(idx)
            torch.cuda.synchronize()
            first = [t.clone() for t in g.lane_logits]
            for l in range(4):
                assert torch.equal(first[l], eager[l]), l
            g.run_many([s + 4 for s in idx])   # the device words advanced: other noise
            torch.cuda.synchronize()
            assert not torch.equal(g.lane_logits[0], first[0])
            bt.set_sample_index(net, 14)
            g.run_many(idx)
            torch.cuda.synchronize()
            for l in range(4):
                assert torch.equal(g.lane_logits[l], eager[l]), l
        finally:
            g.close()


def test_evaluate_runs_on_an_lrt_model():
    from bayesian_torch_amd import mc
    net = _net()
    x = _x((4, 8, 6, 6), F32, seed=6)
    y = torch.tensor([1, 3, 5, 7], device=x.device)
    with torch.no_grad():
        a = mc.evaluate(net, [(x, y)], 4, lanes=4).compute()
        b = mc.evaluate(net, [(x, y)], 4, lanes=1).compute()
    assert a["top1"] == b["top1"] and np.isfinite(a["nll"]) and abs(a["nll"] - b["nll"]) <= 1e-6 * abs(b["nll"])


# =============================================================================================================================
# 5. fused epilogue
# =============================================================================================================================
class _Block(torch.nn.Module):
    def __init__(self):
        from bayesian_torch_amd import layers as L
        super().__init__()
        self.conv1 = L.Conv2dLocalReparameterization(16, 16, 3, padding=1)
        self.conv1.dnn_to_bnn_flag = True
        self.bn1 = torch.nn.BatchNorm2d(16)
        self.relu = torch.nn.ReLU()

    def forward(self, x):
        out = self.bn1(self.conv1(x))
        out = out + x
        return self.relu(out)


@pytest.mark.parametrize("prec,act", PRECS, ids=_PID)
def test_fuse_model_folds_bn_residual_relu_into_the_kind2_store(prec, act):
    """conv -> eval-BN -> + x -> ReLU after models.fuse_model is ONE kind-2 launch; it equals the float64 value of the unfused chain
    (the kind-2 launch followed by ATen BN / add / ReLU) inside the forward envelope carried through the affine, the residual add
    and the ReLU (lrt_model.through_epilogue)."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    bt.manual_seed(31)
    torch.manual_seed(8)
    blk = _Block()
    with torch.no_grad():
        blk.bn1.running_mean.normal_(0.0, 0.3)
        blk.bn1.running_var.uniform_(0.5, 2.0)
        blk.bn1.weight.normal_(1.0, 0.3)
        blk.bn1.bias.normal_(0.0, 0.3)
    blk = blk.to(_dev()).eval()
    blk.conv1.precision = prec
    x = _x((2, 16, 9, 9), act, seed=12)
    with torch.no_grad():
        assert fuse_model(blk) == 1
        bt.set_sample_index(blk, 3)
        from bayesian_torch_amd import functional as BF
        BF.enable_launch_timing(True)
        try:
            fused = blk(x)
            torch.cuda.synchronize()
            assert len(BF.launch_log()) == 1, "the fused block must be one contraction launch"
        finally:
            BF.enable_launch_timing(False)
        zeta = blk.conv1.materialize_noise(3, out_shape=tuple(fused.shape))["zeta"]
    mu, rho, mb, rb = LM.layer_arrays(blk.conv1)
    r = LM.forward(x.float().cpu().numpy(), mu, rho, mb, rb, zeta.cpu().numpy(), LM.op_of(blk.conv1), prec=prec, store_bf16=False)
    bn = blk.bn1
    scale = (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu().numpy()
    shift = bn.bias.detach().double().cpu().numpy() - bn.running_mean.double().cpu().numpy() * scale
    ref, bnd = LM.through_epilogue(r, scale, shift, residual=x.float().cpu().numpy(), relu=1, store_bf16=act is BF16)
    # the folded scale / shift are f32 roundings of the float64 ones: two more roundings on each
    bnd = bnd + 4 * LM.U32 * (np.abs(r["ref"] * scale.reshape(1, -1, 1, 1)) + np.abs(shift).reshape(1, -1, 1, 1))
    assert fused.dtype == act
    _check("block_fused", prec, act, fused, r, ref, bnd)


# =============================================================================================================================
# 6. training
# =============================================================================================================================
# The composite runs as ATen f32 ops on the device (functional.fill_eps_hip supplies zeta), the reference is the float64 composite
# on the CPU at the same zeta.  Each layer is checked LOCALLY, fed with the GPU's own input and upstream gradient (as the fused-LSTM
# tests feed their per-step references): with g = dL/dy, r = sqrt(v), dv = g zeta / (2 r),
#     dmu = corr(x, g)        drho = corr(x^2, dv) 2 sigma sigmoid(rho)        dx = op^T(g, mu) + 2 x op^T(dv, sigma^2)
#     dmu_b = sum g           drho_b = sum dv 2 sigma_b sigmoid(rho_b)
# Every gradient is a contraction; its bound is c A with A the same contraction on absolute values and
#     c = (K_r + 8) 2^-23                 K_r = its reduction length (batch x output pixels for the weight and bias gradients,
#                                         taps x output channels per group for dx), envelope.ACC_UNIT per step as in the forward
#       + c_dv + 8 * 2^-24                on the terms that carry dv: c_dv = ((K + 8) 2^-23 + 12 * 2^-24) / 2 + 4 * 2^-24 is the relative
#                                         error of dv — half of the variance sum's (K products, f32 softplus within 3 ulp so sigma^2
#                                         within 7, x^2 one rounding), then the root, the product with g zeta and the division;
#                                         8 * 2^-24 for the factor 2 sigma sigmoid(rho) that autograd forms from log1p(exp(rho))
#       + 2^-24 |ref|                     the gradient's own final rounding.
class _TrainNet(torch.nn.Module):
    """Conv2d 8 -> 16 (3x3, pad 1) -> flatten -> Linear 400 -> 10, both LRT.  No activation in between: a ReLU mask that flips on a
    rounding error has no envelope.  Every pass records its intermediate values and, through tensor hooks, the gradients that reach
    them (inside a captured step the records are the graph's own static tensors, rewritten by every replay)."""

    def __init__(self):
        from bayesian_torch_amd import layers as L
        super().__init__()
        self.conv = L.Conv2dLocalReparameterization(8, 16, 3, padding=1)
        self.fc = L.LinearLocalReparameterization(16 * 5 * 5, 10)
        self.conv.dnn_to_bnn_flag = self.fc.dnn_to_bnn_flag = True
        self.taps = []

    def forward(self, x):
        h = self.conv(x)
        f = h.flatten(1)
        z = self.fc(f)
        rec = dict(x=x, h=h, f=f, z=z)
        if z.requires_grad:
            h.register_hook(lambda g: rec.__setitem__("gh", g.clone()))
            f.register_hook(lambda g: rec.__setitem__("gf", g.clone()))
            z.register_hook(lambda g: rec.__setitem__("gz", g.clone()))
        self.taps.append(rec)
        return z


def _train_net():
    import bayesian_torch_amd as bt
    bt.manual_seed(99)
    torch.manual_seed(6)
    net = _TrainNet()
    with torch.no_grad():
        for layer in (net.conv, net.fc):
            layer._w()[1].uniform_(-4.0, -1.0)
            layer.rho_bias.uniform_(-3.0, -1.0)
    return net.to(_dev()).train()


def _params_of(layer):
    mu, rho = layer._w()
    return dict(mu=mu.detach().clone(), rho=rho.detach().clone(), mu_b=layer.mu_bias.detach().clone(),
                rho_b=layer.rho_bias.detach().clone())


def _local64(layer, params, x, g, zeta):
    """float64 gradients of ONE layer's composite at the input x, upstream gradient g and zeta given -> ({name: ref}, {name: bound})"""
    op = LM.op_of(layer)
    P = {k: v.detach().double().cpu().contiguous().requires_grad_() for k, v in params.items()}
    x64 = x.detach().double().cpu().contiguous().requires_grad_()
    g64, z64 = g.detach().double().cpu(), zeta.detach().double().cpu()
    sg, sb = torch.log1p(torch.exp(P["rho"])), torch.log1p(torch.exp(P["rho_b"]))
    m = E.contract(x64, P["mu"], P["mu_b"], op)
    v = E.contract(x64 * x64, sg * sg, sb * sb, op)
    (m + torch.sqrt(v) * z64).backward(g64)
    ref = {k: t.grad.numpy() for k, t in P.items()}
    ref["x"] = x64.grad.numpy()
    with torch.no_grad():
        xd, sgd, sbd = x64.detach(), sg.detach(), sb.detach()
        dv = (g64 * z64 / (2.0 * torch.sqrt(v))).abs()
        Kf = E.reduction_length(tuple(P["mu"].shape), op)
        Kw = E.wgrad_reduction_length(tuple(g64.shape), op)
        Kd = E.dgrad_reduction_length(tuple(P["mu"].shape), op)
        c_dv = 0.5 * ((Kf + 8) * E.ACC_UNIT + 12 * LM.U32) + 4 * LM.U32 + 8 * LM.U32
        cw, cd = (Kw + 8) * E.ACC_UNIT, (Kd + 8) * E.ACC_UNIT
        red = [d for d in range(g64.dim()) if d != (1 if g64.dim() > 2 else g64.dim() - 1)]
    wshape = tuple(P["mu"].shape)
    A_mu = E.wgrad_A(xd, g64, wshape, op)
    A_s2 = E.wgrad_A(xd * xd, dv, wshape, op)
    A_x1 = E.dgrad_A(g64, tuple(xd.shape), P["mu"].detach().abs(), op)
    A_x2 = 2.0 * xd.abs() * E.dgrad_A(dv, tuple(xd.shape), sgd * sgd, op)
    with torch.no_grad():
        bnd = {"mu": cw * A_mu,
               "rho": (cw + c_dv) * A_s2 * 2.0 * sgd * torch.sigmoid(P["rho"].detach()),
               "mu_b": cw * g64.abs().sum(red),
               "rho_b": (cw + c_dv) * dv.sum(red) * 2.0 * sbd * torch.sigmoid(P["rho_b"].detach()),
               "x": cd * A_x1 + (cd + c_dv) * A_x2}
    bnd = {k: b.numpy() + LM.U32 * np.abs(ref[k]) for k, b in bnd.items()}
    return ref, bnd


def _grads_of(layer):
    mu, rho = layer._w()
    return dict(mu=mu.grad, rho=rho.grad, mu_b=layer.mu_bias.grad, rho_b=layer.rho_bias.grad)


def test_eager_training_step_gradients_inside_the_float64_envelope():
    """training draws the zeta inference draws at the same (seed, layer id, sample index): the training forward lies inside the f32
    forward envelope of THAT zeta, and dmu, drho, the bias gradients and dx of both layers inside the local envelopes above"""
    import bayesian_torch_amd as bt
    net = _train_net()
    x = _x((4, 8, 5, 5), F32, seed=3).requires_grad_()
    y = torch.tensor([1, 0, 7, 3], device=x.device)
    bt.set_sample_index(net, 6)
    loss = torch.nn.functional.cross_entropy(net(x), y)
    loss.backward()
    torch.cuda.synchronize()
    rec = net.taps[-1]
    for name, layer, xin, g, dx in (("conv", net.conv, x, rec["gh"], x.grad), ("fc", net.fc, rec["f"], rec["gz"], rec["gf"])):
        out = rec["h"] if name == "conv" else rec["z"]
        with torch.no_grad():
            zeta = layer.materialize_noise(6, out_shape=tuple(out.shape))["zeta"]
        mu, rho, mb, rb = LM.layer_arrays(layer)
        r = LM.forward(xin.detach().cpu().numpy(), mu, rho, mb, rb, zeta.cpu().numpy(), LM.op_of(layer), prec="f32")
        extra = (r["K"] + 8) * E.REF32_UNIT * (r["A_m"] + np.abs(zeta.cpu().numpy()) * np.sqrt(r["v"]))
        _check("train_fwd_" + name, "aten", F32, out.detach(), r, r["ref"], r["bound"] + extra)
        ref, bnd = _local64(layer, _params_of(layer), xin, g, zeta)
        got = dict(_grads_of(layer), x=dx)
        for k in ("mu", "rho", "mu_b", "rho_b", "x"):
            rep = E.check(got[k].detach().cpu().numpy(), ref[k], bnd[k])
            print(rep.line("train_%s_d%s" % (name, k), "aten/f32"))
            assert rep.ok, (name, k, str(rep))
            assert np.abs(ref[k]).max() > 0
        # the bound is sharp enough to see the noise path: without the variance branch drho would be zero
        assert not E.check(np.zeros_like(ref["rho"]), ref["rho"], bnd["rho"]).ok


def test_graphed_train_step_num_mc_2_with_captured_sgd():
    """GraphedTrainStep(num_mc=2, optimizer=SGD) captures and replays a model of LRT layers: the layers read the step's device
    sample words (pass k of step s draws sample 2 s + k).  After one replay the loss and every parameter lie inside the float64
    envelope of the eager step — the per-pass local gradients above summed over the two passes, then p - lr G with three more
    roundings — and a second replay (other sample words) changes the loss."""
    from bayesian_torch_amd import autograd as AG, optim
    net = _train_net()
    x = _x((4, 8, 5, 5), F32, seed=3)
    y = torch.tensor([1, 0, 7, 3], device=x.device)
    lr = 0.05
    opt = optim.SGD(net.parameters(), lr=lr)
    loss_fn = lambda out, tgt: torch.nn.functional.cross_entropy(out.mean(0), tgt)  # noqa: E731
    layers = (("conv", net.conv), ("fc", net.fc))
    p0 = {name: _params_of(layer) for name, layer in layers}
    step = AG.GraphedTrainStep(net, x, y, loss_fn=loss_fn, optimizer=opt, num_mc=2)
    try:
        for name, layer in layers:   # constructing the step changes no parameter
            assert all(torch.equal(v, _params_of(layer)[k]) for k, v in p0[name].items())
        taps = net.taps[-2:]
        loss1 = float(step.run(3))
        torch.cuda.synchronize()
        # loss: CE(mean_k z_k) from the GPU's own logits in float64.  f32 errors: the mean (2 roundings), exp / log within 2 ulp, the
        # row sums over C = 10 terms, the subtractions, the mean over B = 4 rows  ->  (C + B + 16) 2^-24 of the magnitudes
        zbar = (taps[0]["z"].double() + taps[1]["z"].double()).cpu() / 2.0
        loss64 = float(torch.nn.functional.cross_entropy(zbar, y.cpu()))
        b_loss = (10 + 4 + 16) * LM.U32 * (1.0 + float(zbar.abs().max()) + abs(loss64))
        print("graphed_loss: err %.3g bound %.3g" % (abs(loss1 - loss64), b_loss))
        assert abs(loss1 - loss64) <= b_loss
        for name, layer in layers:
            tot, btot, mag = None, None, None
            for k in range(2):
                rec = taps[k]
                xin, g, out = (rec["x"], rec["gh"], rec["h"]) if name == "conv" else (rec["f"], rec["gz"], rec["z"])
                with torch.no_grad():
                    zeta = layer.materialize_noise(2 * 3 + k, out_shape=tuple(out.shape))["zeta"]
                ref, bnd = _local64(layer, p0[name], xin, g, zeta)
                tot = ref if tot is None else {q: tot[q] + ref[q] for q in ref}
                btot = bnd if btot is None else {q: btot[q] + bnd[q] for q in bnd}
                mag = {q: np.abs(ref[q]) for q in ref} if mag is None else {q: mag[q] + np.abs(ref[q]) for q in ref}
            now = _params_of(layer)
            for q in ("mu", "rho", "mu_b", "rho_b"):
                p_old = p0[name][q].double().cpu().numpy()
                want = p_old - lr * tot[q]
                bound = lr * (btot[q] + LM.U32 * mag[q]) + 3 * LM.U32 * (np.abs(p_old) + lr * np.abs(tot[q]))
                rep = E.check(now[q].cpu().numpy(), want, bound)
                print(rep.line("graphed_%s_%s" % (name, q), "aten/f32"))
                assert rep.ok, (name, q, str(rep))
                assert not np.array_equal(now[q].cpu().numpy(), p0[name][q].cpu().numpy())
        loss2 = float(step.run(4))
        torch.cuda.synchronize()
        assert np.isfinite(loss2) and loss2 != loss1
    finally:
        step.close()
