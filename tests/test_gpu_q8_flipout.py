"""The INT8 Flipout kernels (btx_q8_sample_delta, btx_q8_contract_flipout) against their numpy model (tests/q8_flipout_model.py),
bit for bit with explicit noise; BTX-RNG noise fetched through btx_fill_eps / btx_fill_sign and fed to the model; the twin against
its float source; graph replay; a tiny Flipout QResNet against its numpy chain."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import q8_flipout_helpers as F
import q8_flipout_model as QF
import q8_model as Q
import q8_net_model as QN

pytestmark = pytest.mark.gpu

DEV = "cuda"
# name -> make_case arguments.  The smallest shapes at which this kernel can still go wrong:
CONV = {
    # bytewise loads (C % 16 != 0), N < the 4-channel pack, M = 72 (a second pixel tile with a tail), Kp tail, padded taps on both tiles
    "c5n7": dict(B=2, C=5, N=7, hw=(6, 6), k=3, padding=1),
    # the 16-byte path, stride 2, odd extent
    "c16n64s2": dict(B=2, C=16, N=64, hw=(9, 9), k=3, stride=2, padding=1),
    # Cp != C, a 16-element chunk straddles a 32-sign word (rows of 24 signs), an n-tile tail
    "c24n68": dict(B=2, C=24, N=68, hw=(5, 5), k=1),
    # the stem
    "stem": dict(B=1, C=3, N=8, hw=(20, 20), k=7, stride=2, padding=3),
    "dil2": dict(B=1, C=16, N=12, hw=(7, 7), k=3, padding=2, dilation=2),
}
LINEAR = {"small": dict(B=3, C=6, N=4), "big": dict(B=70, C=96, N=130)}


def _np(t):
    return t.detach().cpu().numpy()


def _qt(a, s, z):
    from bayesian_torch_amd.q8 import QTensor
    return QTensor(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), s, z)


@functools.lru_cache(maxsize=None)
def _case(kind, name, z_x=126, calibrated=True, relu=False, bias=True):
    kw = (CONV if kind == "conv" else LINEAR)[name]
    seed = sum(ord(ch) for ch in kind + name) + z_x
    return F.make_case(seed, kind == "conv", z_x=z_x, calibrated=calibrated, relu=relu, bias=bias, **kw)


def _check(case, noise=True, float_input=None):
    """run the twin on the case with explicit noise and compare every output with the model"""
    q = F.twin_of(case, DEV)
    m = case["model"]
    x = _qt(case["x_i"], *case["e_x"]) if float_input is None else float_input
    with torch.no_grad():
        out, parts = q.forward_int8(x, noise=F.case_noise(case), parts=True)
    N, C = case["mu"].shape[:2]
    k = case["k"]
    D, pad_zero = F.unpack_image(parts["D"], N, C, k)
    Wm, pad_zero_m = F.unpack_image(parts["W_mu"], N, C, k)
    assert pad_zero and pad_zero_m
    assert np.array_equal(D.reshape(m["d_i"].shape), m["d_i"])
    assert np.array_equal(Wm.reshape(case["mu_i"].shape), case["mu_i"])
    assert np.array_equal(_np(parts["S_d"]), Q.row_sums(m["d_i"])) and np.array_equal(_np(parts["S_mu"]), Q.row_sums(case["mu_i"]))
    assert np.array_equal(_np(parts["bm_i"]), m["bm_i"]) and np.array_equal(_np(parts["bp_i"]), m["bp_i"])
    e = case["e"]
    if case["conv"]:
        assert (out.q_scale(), out.q_zero_point()) == e[9] and out.int_repr().is_contiguous(memory_format=torch.channels_last)
        got = _np(out.int_repr())
    else:
        assert out.dtype == torch.float32
        got = _np(out)
        want = Q.dequantize(m["out"], *e[9])
        assert np.array_equal(got, want)
        got = np.rint(got / np.float32(e[9][0]) + e[9][1]).astype(np.uint8)
    bad = int((got != m["out"]).sum())
    sat = float(((m["out"] == 0) | (m["out"] == 255)).mean())
    print("saturated %.3f, o1 != z: %.3f, p2 spread %d" % (sat, float((m["o1"] != e[3][1]).mean()), int(m["p2"].max()) - int(m["p2"].min())))
    assert bad == 0, "%d of %d output bytes differ from the model" % (bad, got.size)
    assert sat < 0.5 and int(m["p2"].max()) - int(m["p2"].min()) >= 8   # the case exercises the arithmetic, not the clamps


@pytest.mark.parametrize("name", list(CONV))
def test_conv_bit_equal_to_the_model(name):
    _check(_case("conv", name))


@pytest.mark.parametrize("z_x", [0, 255])
def test_conv_extreme_input_zero_points(z_x):
    _check(_case("conv", "c5n7", z_x=z_x))


@pytest.mark.parametrize("name", list(LINEAR))
def test_linear_bit_equal_to_the_model_f32_output(name):
    _check(_case("linear", name))


@pytest.mark.parametrize("kind,name", [("conv", "c5n7"), ("conv", "c16n64s2"), ("linear", "big")])
def test_default_path_bit_equal_to_the_model(kind, name):
    """quant_dict None: the reference's default entries, mu_b to the mean GEMM and sigma_b * eps_b to the perturbed one"""
    _check(_case(kind, name, z_x=128, calibrated=False))


def test_relu_fold_and_no_bias():
    _check(_case("conv", "c5n7", relu=True))
    c = _case("conv", "c5n7", relu=True)
    assert int(c["model"]["out"].min()) == c["e"][9][1]
    _check(_case("conv", "c16n64s2", bias=False))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_float_input_is_quantized_first(dtype):
    c = _case("conv", "c16n64s2")
    s_x, z_x = c["e_x"]
    x = ((torch.from_numpy(c["x_i"].astype(np.float32)) - z_x) * np.float32(s_x)).to(dtype)
    back = Q.quantize_input(x.float().numpy(), s_x, z_x)
    if dtype == torch.float32:
        assert np.array_equal(back, c["x_i"])
    else:  # bf16 rounding moves some bytes: the model runs on what the quantize launch must produce
        c = dict(c, x_i=back)
        c["model"] = QF.layer_forward(back, c["e_x"], c["mu_i"], c["s_mu"], c["sigma_i"], c["s_sigma"], c["eps"],
                                      *[QF.bias_vec(c["mu_b"], c["sigma_b"], c["eps_b"], kk) for kk in c["kinds"]],
                                      c["sign_in"], c["sign_out"], c["e"], **c["geom"])
    _check(c, float_input=x.to(DEV))


@pytest.mark.parametrize("name", F.CASES)
def test_reference_fixtures(name):
    """the kernels on the reference's own cases: bit-equal to the model, hence as close to the reference as the model is"""
    d = F.fixture(name)
    q = F.quantized_layer(d, DEV)
    m = F.model_record(d)
    with torch.no_grad():
        out, parts = q.forward_int8(_qt(d["x_i"], *F.e_x(d)), noise=F.noise_of(d), parts=True)
    assert np.array_equal(_np(parts["bm_i"]), d["bm_i"]) and np.array_equal(_np(parts["bp_i"]), d["bp_i"])
    e9 = F.entries(d)[9]
    got = _np(out.int_repr()) if int(d["kind"]) == 1 else np.rint(_np(out) / np.float32(e9[0]) + e9[1]).astype(np.uint8)
    assert np.array_equal(got, m["out"])
    diff = np.abs(got.astype(np.int32) - d["ref_out"].astype(np.int32))
    assert diff.max() <= F.MAX_LSB


def _fill(n, seed, s_idx, lid, stream, sign):
    from bayesian_torch_amd import functional as BF
    fn = BF.fill_sign_hip if sign else BF.fill_eps_hip
    return _np(fn(n, DEV, seed, s_idx, lid, stream))


@pytest.mark.parametrize("name", ["c24n68", "c5n7"])
def test_btx_rng_noise_fetched_through_the_fill_kernels(name):
    """no explicit noise: the kernels hash their own.  eps and signs are fetched with btx_fill_eps / btx_fill_sign over the index
    spaces the header documents (rows of the channel count rounded up to 8) and fed to the model."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import _lib, rng
    bt.manual_seed(77)
    c = _case("conv", name)
    q = F.twin_of(c, DEV)
    s_idx, lid, seed = 4, q._btx_layer_id, rng.seed()
    N, C = c["mu"].shape[:2]
    k, cp = c["k"], (C + 7) // 8 * 8
    with torch.no_grad():
        out = q.forward_int8(_qt(c["x_i"], *c["e_x"]), sample_idx=s_idx)
    B, _, H, W = c["x_i"].shape
    eps = _fill(N * k * k * cp, seed, s_idx, lid, _lib.STREAM_EPS_W, False).reshape(N, k, k, cp)[..., :C].transpose(0, 3, 1, 2)
    eps_b = _fill(N, seed, s_idx, lid, _lib.STREAM_EPS_B, False)
    si = _fill(B * H * W * cp, seed, s_idx, lid, _lib.STREAM_SIGN_IN, True).reshape(B, H, W, cp)[..., :C].transpose(0, 3, 1, 2)
    oshape = c["model"]["out"].shape
    so = _fill(int(np.prod(oshape)), seed, s_idx, lid, _lib.STREAM_SIGN_OUT, True).reshape(oshape[0], oshape[2], oshape[3], N).transpose(0, 3, 1, 2)
    assert set(np.unique(si)) == {-1, 1} and set(np.unique(so)) == {-1, 1}
    bm, bp = (QF.bias_vec(c["mu_b"], c["sigma_b"], eps_b, kk) for kk in c["kinds"])
    m = QF.layer_forward(c["x_i"], c["e_x"], c["mu_i"], c["s_mu"], c["sigma_i"], c["s_sigma"], eps, bm, bp, si, so, c["e"], **c["geom"])
    assert np.array_equal(_np(out.int_repr()), m["out"])
    with torch.no_grad():
        again = q.forward_int8(_qt(c["x_i"], *c["e_x"]), sample_idx=s_idx + 1)
    assert not torch.equal(again.int_repr(), out.int_repr())


def test_twin_draws_the_eps_and_signs_of_its_float_source():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn
    bt.manual_seed(2024)
    torch.manual_seed(3)
    f = L.Conv2dFlipout(16, 24, 3, padding=1, bias=True).to(DEV)
    m = nn.Sequential(f)
    x = torch.randn(2, 16, 6, 6, device=DEV)
    with torch.no_grad():
        y = f(x, return_kl=False)
    nz = f.materialize_noise(5, tuple(x.shape), tuple(y.shape), x.dtype)
    bnn_to_qbnn(m, flipout=True)
    q = m[0]
    assert type(q).__name__ == "QuantizedConv2dFlipout" and q._btx_layer_id == f._btx_layer_id
    with torch.no_grad():
        out, parts = q.forward_int8(x, sample_idx=5, parts=True)
        out2 = q.forward_int8(x, noise={k_: v for k_, v in nz.items()}, sample_idx=5)
    tw = parts["noise"]
    for k_ in ("eps_w", "eps_b", "sign_in", "sign_out"):
        assert torch.equal(tw[k_].float().cpu(), nz[k_].float().cpu()), k_
    assert torch.equal(out.int_repr(), out2.int_repr())   # the hashed draw inside the kernels == the float layer's tensors


class Two(nn.Module):
    def __init__(self):
        super().__init__()
        from bayesian_torch_amd import layers as L
        self.conv = L.Conv2dFlipout(8, 16, 3, padding=1, bias=True)
        self.fc = L.LinearFlipout(16 * 5 * 5, 10)

    def forward(self, x):
        x = self.conv(x)
        x = x[0] if isinstance(x, tuple) else x
        x = x.dequantize() if getattr(x, "is_quantized", False) else x
        y = self.fc(torch.relu(x).flatten(1))
        return y[0] if isinstance(y, tuple) else y


def test_graphed_mc_replays_equal_eager_forwards_and_lanes_are_refused():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc, _lib
    from bayesian_torch_amd.models import bnn_to_qbnn, fuse_model
    bt.manual_seed(9)
    torch.manual_seed(10)
    m = Two().to(DEV).eval()
    bnn_to_qbnn(m, flipout=True)
    assert type(m.conv).__name__ == "QuantizedConv2dFlipout" and type(m.fc).__name__ == "QuantizedLinearFlipout"
    fuse_model(m)
    assert type(m.conv).__name__ == "QuantizedConv2dFlipout"
    x = torch.randn(3, 8, 5, 5, device=DEV)
    eager = {}
    with torch.no_grad():
        for s in (5, 0, 1, 2):
            bt.set_sample_index(m, s)
            eager[s] = m(x).clone()
    assert not torch.equal(eager[0], eager[1])
    g = mc.GraphedMC(m, x, lanes=1, keep_logits=True)
    try:
        for s in (5, 0, 2):
            g.run(s)
            torch.cuda.synchronize()
            assert torch.equal(g.lane_logits[0], eager[s]), s
    finally:
        g.close()
    packed = mc.mc_forward(m, x, 3, lanes=1)
    assert torch.isfinite(packed).all()
    with pytest.raises(_lib.BtxError, match="lanes"):
        mc.mc_forward(m, x, 4, lanes=2)
    with pytest.raises(_lib.BtxError, match="lanes"):
        mc.GraphedMC(m, x, lanes=2)


# ---- the tiny Flipout QResNet against its numpy chain ---------------------------------------------------------------------
def _model_twin(q, x_i, e_x, s_idx, conv=True):
    """one twin on the numpy model with the noise BTX-RNG defines for it (fetched through the fill kernels)"""
    pr = lambda v: v if isinstance(v, int) else tuple(v)  # noqa: E731
    gm = dict(stride=pr(q.stride), padding=pr(q.padding), dilation=pr(q.dilation)) if conv else {}
    mu_i = _np(q.quantized_mu_weight).astype(np.int32)
    acc = Q.accumulate(x_i, 0, np.zeros_like(mu_i), **gm)
    nz = {k_: _np(v) for k_, v in q.materialize_noise(s_idx, x_i.shape, acc.shape).items()}
    e, cal = q._entries(6 / 255, 0.1, 128)
    kinds = q._bias_kinds(cal)
    mu_b = _np(q.quantized_mu_bias) if q.bias else None
    sigma_b = _np(q.quantized_sigma_bias) if q.bias and q.quantized_sigma_bias is not None else None
    bm, bp = (QF.bias_vec(mu_b, sigma_b, nz["eps_b"], kk) for kk in kinds)
    r = QF.layer_forward(x_i, e_x, mu_i, q._q8_scales[0], _np(q.quantized_sigma_weight).astype(np.int32), q._q8_scales[1], nz["eps_w"],
                         bm, bp, nz["sign_in"], nz["sign_out"], e, relu=conv and bool(q.relu), **gm)
    return r["out"], e[9]


def test_tiny_flipout_qresnet_equals_its_numpy_chain_and_replays():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.models import resnet as R, to_qresnet
    bt.manual_seed(5)
    torch.manual_seed(6)
    m = R.ResNet(R.BasicBlock, [1, 1, 1, 1], num_classes=10).eval()
    m.avgpool = nn.AvgPool2d(1)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
            mod.running_mean.normal_(0, 0.3)
            mod.running_var.uniform_(0.5, 2.0)
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=True, moped_delta=0.5))
    m.to(DEV)
    q = to_qresnet(m)
    assert type(q.conv1).__name__ == "QuantizedConv2dFlipout" and type(q.fc).__name__ == "QuantizedLinearFlipout"
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(8))
    s_idx = 3
    with torch.no_grad():
        bt.set_sample_index(q, s_idx)
        y = q(x.to(DEV)).clone()
    # the numpy chain
    cur = Q.quantize_input(x.numpy(), 0.1, 128)
    cur, ex = _model_twin(q.conv1, cur, (0.1, 128), s_idx)
    assert q.conv1.relu
    cur = QN.max_pool(cur, 3, 2, 1)
    for layer in (q.layer1, q.layer2, q.layer3, q.layer4):
        for blk in layer:
            o, eo = _model_twin(blk.conv1, cur, ex, s_idx)
            o, eo = _model_twin(blk.conv2, o, eo, s_idx)
            res, er = (cur, ex) if blk.downsample is None else _model_twin(blk.downsample[0], cur, ex, s_idx)
            s_add = max(eo[0], er[0])
            cur, ex = QN.add(o, eo[0], eo[1], res, er[0], er[1], s_add, 0, True), (s_add, 0)
    cur = QN.avg_pool(cur, ex[1], 1, 1).reshape(cur.shape[0], -1)
    out, e9 = _model_twin(q.fc, cur, ex, s_idx, conv=False)
    want = Q.dequantize(out, *e9)
    assert y.shape == (2, 10) and np.array_equal(_np(y), want)
    assert len(np.unique(want)) > 3
    g = mc.GraphedMC(q, x.to(DEV), lanes=1, keep_logits=True)
    try:
        g.run(s_idx)
        torch.cuda.synchronize()
        assert torch.equal(g.lane_logits[0], y)
    finally:
        g.close()
