"""The INT8 network ops on the GPU (btx_q8.hip) against their numpy model (tests/q8_net_model.py), bit for bit: the quantized
add, max- and avg-pool, the residual epilogue of the contraction (== requantize, then add == btx_q8_contract + btx_q8_add), the
reference's Bottleneck fixture stage by stage, residual blocks through BTX-RNG, and a whole QResNet: fused add on == off, graph
replay, MC accumulation."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import q8_helpers as H
import q8_model as Q
import q8_net_model as QN

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE_PAIRS = [(0.1, 0.07), (0.2, 0.1), (0.1, 0.1), (0.1, 0.05), (0.0371, 0.0913)]
# (Cin, Cout, k, stride, padding, dilation, (B, H, W)): whole vector stores; K tail and N < 64; N % 4 != 0 (byte loads and stores,
# M = 35); a ragged second N block over two pixel blocks
RES_CONV = [(32, 16, 3, 1, 1, 1, (2, 9, 9)), (80, 40, 1, 2, 0, 1, (2, 8, 8)), (16, 10, 3, 1, 1, 1, (1, 5, 7)),
            (16, 72, 1, 1, 0, 1, (3, 5, 5))]
CONV_ZO = {0: 7, 128: 128, 131: 120}   # residual zero point -> the conv's own output zero point used with it
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Reparameterization",
             moped_enable=True, moped_delta=0.5)   # MOPED: the means are the He-initialised weights, activations stay O(1)


def _np(t):
    return t.detach().cpu().numpy()


def _qt(a, s, z):
    from bayesian_torch_amd.q8 import QTensor
    return QTensor(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), s, z)


def _sat(o):
    return float(((o == 0) | (o == 255)).mean())


# ---- add ------------------------------------------------------------------------------------------------------------------
def add_case(n):
    g = np.random.RandomState(100 + n)
    return g.randint(0, 256, n).astype(np.uint8), g.randint(0, 256, n).astype(np.uint8), 128, 131


@pytest.mark.parametrize("pair", range(len(SCALE_PAIRS)))
@pytest.mark.parametrize("n", [700, 6272])
def test_add_bit_equal_to_the_model(n, pair):
    """n = 700: 43 vector groups and a 12-byte tail; 6272 = 98 * 64.  Full-range bytes: part of the sums leaves [0, 255]"""
    from bayesian_torch_amd import q8
    a, b, z_a, z_b = add_case(n)
    s_a, s_b = SCALE_PAIRS[pair]
    s = max(s_a, s_b)
    qa, qb = _qt(a, s_a, z_a), _qt(b, s_b, z_b)
    for z in (0, 128, 120):
        for relu in (False, True):
            ref = QN.add(a, s_a, z_a, b, s_b, z_b, s, z, relu)
            sat = _sat(ref)
            print("add n=%d pair=%d z=%d relu=%d: saturated %.3f" % (n, pair, z, relu, sat))
            assert 0 < sat < 0.9, sat
            out = q8.add(qa, qb, s, z, relu)
            assert (out.q_scale(), out.q_zero_point()) == (s, z) and out.int_repr().dtype == torch.uint8
            assert np.array_equal(_np(out.int_repr()), ref), (z, relu)


def test_add_on_unaligned_bases_goes_bytewise():
    from bayesian_torch_amd import q8
    a, b, z_a, z_b = add_case(700)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    out = q8.add(q8.QTensor(ta[1:], 0.1, z_a), q8.QTensor(tb[1:], 0.07, z_b), 0.1, 120, True)
    assert np.array_equal(_np(out.int_repr()), QN.add(a[1:], 0.1, z_a, b[1:], 0.07, z_b, 0.1, 120, True))


# ---- pooling --------------------------------------------------------------------------------------------------------------
def _bytes(shape, seed):
    x = np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)
    x.reshape(-1)[:2] = (0, 255)
    x.reshape(-1)[-2:] = (255, 0)
    return x


@pytest.mark.parametrize("shape,k,s,p", [((2, 16, 9, 9), 3, 2, 1), ((1, 24, 8, 8), 3, 2, 1), ((2, 3, 5, 5), 2, 2, 0)])
def test_max_pool_bit_equal_to_the_model(shape, k, s, p):
    """odd extent with clipped windows (16 channels per thread); C = 24 and C = 3: the bytewise path"""
    from bayesian_torch_amd import q8
    x = _bytes(shape, 7)
    out = q8.max_pool2d(_qt(x, 0.1, 77), k, s, p)
    ref = QN.max_pool(x, k, s, p)
    assert out.shape == ref.shape and (out.q_scale(), out.q_zero_point()) == (0.1, 77)
    assert out.int_repr().is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(_np(out.int_repr()), ref)
    assert ref.max() == 255 and ref.min() < 255


@pytest.mark.parametrize("z", [0, 77, 128])
@pytest.mark.parametrize("shape,k,s", [((2, 64, 7, 7), 7, 1), ((1, 24, 8, 8), 2, 2), ((2, 10, 9, 9), 3, 1)])
def test_avg_pool_bit_equal_to_the_model(shape, k, s, z):
    from bayesian_torch_amd import q8
    from bayesian_torch_amd._lib import BtxError
    x = _bytes(shape, 11)
    out = q8.avg_pool2d(_qt(x, 0.1, z), k, s)
    ref = QN.avg_pool(x, z, k, s)
    assert out.shape == ref.shape and (out.q_scale(), out.q_zero_point()) == (0.1, z)
    assert np.array_equal(_np(out.int_repr()), ref)
    with pytest.raises(BtxError, match="code -3"):
        q8.avg_pool2d(_qt(x, 0.1, z), k, s, 1)


def test_relu_and_view_of_the_carrier():
    from bayesian_torch_amd import q8
    x = _bytes((2, 16, 1, 1), 5)
    t = _qt(x, 0.1, 128)
    assert np.array_equal(_np(q8.relu(t).int_repr()), QN.relu(x, 128))
    v = t.view(t.size(0), -1)
    assert v.shape == (2, 16) and np.array_equal(_np(v.int_repr()), x.reshape(2, 16))


# ---- the residual epilogue ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def res_case(idx, bias):
    """float parameters, noise, input and residual bytes of one shape (CPU, seeded), and everything of the model that does not
    depend on the zero points: shared by every variant"""
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn
    cin, cout, k, s, p, dl, (b, h, w) = RES_CONV[idx]
    g = torch.Generator().manual_seed(4000 + 10 * idx + (1 if bias else 0))
    layer = L.Conv2dReparameterization(cin, cout, k, stride=s, padding=p, dilation=dl, bias=bias)
    x = torch.randn(b, cin, h, w, generator=g) * 2
    mu, rho = layer._w()
    with torch.no_grad():
        mu.copy_(torch.randn(mu.shape, generator=g) * 0.2)
        rho.copy_(torch.randn(rho.shape, generator=g) * 0.5 - 2.0)
        if bias:
            layer.mu_bias.copy_(torch.randn(layer.mu_bias.shape, generator=g))
            layer.rho_bias.copy_(torch.randn(layer.rho_bias.shape, generator=g) * 0.3 - 1.0)
    eps = torch.randn(mu.shape, generator=g)
    eps_b = torch.randn(mu.shape[0], generator=g) if bias else None
    wrap = nn.Module()
    wrap.l = layer
    bnn_to_qbnn(wrap)
    q = wrap.l
    s_mu, s_sigma = q._q8_scales
    mu_i, sigma_i = _np(q.quantized_mu_weight).astype(np.int32), _np(q.quantized_sigma_weight).astype(np.int32)
    # calibrated-style scales from the parameters' ranges, as tests/test_gpu_q8.py builds them
    s_eps = 6 / 255
    s_d = float(np.float32(2 * 3 * float(np.abs(sigma_i).max()) * s_sigma / 255))
    s_w = float(np.float32(2 * (float(np.abs(mu_i).max()) * s_mu + 127 * s_d) / 255))
    s_x, z_x = 4.0 * 2 / 255 * 2, 128
    x_i = Q.quantize_input(x.numpy(), s_x, z_x)
    geom = dict(stride=s, padding=p, dilation=dl)
    W_m = Q.sample_weight(mu_i, s_mu, sigma_i, s_sigma, eps.numpy(), s_eps, s_d, s_w)[0]
    acc = Q.accumulate(x_i, z_x, W_m, **geom)
    b_i = Q.bias_int(_np(q.quantized_mu_bias) if bias else None, _np(q.quantized_sigma_bias) if bias else None,
                     eps_b.numpy() if bias else None, s_x, s_w, cout)
    s_o = float(np.float32(s_x * s_w * float(np.abs(acc).max()) / 200))   # the largest conv outputs saturate on either side
    res = np.random.RandomState(77 + idx).randint(0, 256, acc.shape).astype(np.uint8)
    return dict(q=q, x=x, x_i=x_i, eps=eps, eps_b=eps_b, acc=acc, b_i=b_i, res=res, geom=geom, chain=(s_eps, s_d, s_w), s_x=s_x, z_x=z_x,
                s_o=s_o, s_r=float(np.float32(0.7 * s_o)))


def res_variants():
    for z_r in (0, 128, 131):
        for z_add in (0, 120):
            for add_relu in (False, True):
                for conv_relu in (False, True):
                    yield z_r, z_add, add_relu, conv_relu


def res_model(c, z_r, z_add, add_relu, conv_relu):
    """(the conv's own uint8 output, the sum) of one variant; the add's scale is the reference's max(s_o, s_r)"""
    s_eps, s_d, s_w = c["chain"]
    z_o = CONV_ZO[z_r]
    o = Q.requantize(c["acc"], c["b_i"], c["s_x"], s_w, c["s_o"], z_o, conv_relu)
    s_add = max(c["s_o"], c["s_r"])
    return o, QN.conv_add(c["acc"], c["b_i"], c["s_x"], s_w, c["s_o"], z_o, conv_relu, c["res"], c["s_r"], z_r, s_add, z_add, add_relu)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("idx", range(len(RES_CONV)))
def test_fused_residual_epilogue_equals_the_model_and_the_two_launches(idx, bias):
    from bayesian_torch_amd import q8
    c = res_case(idx, bias)
    q = c["q"].to(DEV)
    s_eps, s_d, s_w = c["chain"]
    x = c["x"].to(DEV)
    noise = dict(eps_w=c["eps"], eps_b=c["eps_b"])
    cout = RES_CONV[idx][1]
    try:
        for z_r, z_add, add_relu, conv_relu in res_variants():
            z_o = CONV_ZO[z_r]
            q.quant_dict = [(s_eps, 0), (s_d, 0), (s_w, 0), (c["s_x"], c["z_x"]), (c["s_o"], z_o)]
            q.relu = conv_relu
            o_ref, ref = res_model(c, z_r, z_add, add_relu, conv_relu)
            sat = _sat(ref)
            assert 0 < sat < 0.9, (sat, z_r, z_add, add_relu, conv_relu)
            res = _qt(c["res"], c["s_r"], z_r)
            fused = q.forward_int8(x, noise=noise, residual=res, add_relu=add_relu, add_scale=None, add_zero_point=z_add)
            s_add = max(c["s_o"], c["s_r"])
            assert (fused.q_scale(), fused.q_zero_point()) == (s_add, z_add)
            assert fused.int_repr().is_contiguous(memory_format=torch.channels_last)
            assert np.array_equal(_np(fused.int_repr()), ref), (z_r, z_add, add_relu, conv_relu)
            plain = q.forward_int8(x, noise=noise)
            assert np.array_equal(_np(plain.int_repr()), o_ref)
            two = q8.add(plain, res, s_add, z_add, add_relu)
            assert torch.equal(two.int_repr(), fused.int_repr())
    finally:
        q.quant_dict = None
        q.relu = False
    assert fused.shape[1] == cout


def test_forward_add_is_the_fused_launch_with_the_reference_scale_rule():
    import bayesian_torch_amd as bt
    c = res_case(0, False)
    q = c["q"].to(DEV)
    x = c["x"].to(DEV)
    res = _qt(c["res"], 0.13, 131)
    wrap = nn.Module()
    wrap.l = q
    bt.set_sample_index(wrap, 4)
    a = q.forward_add(x, res)
    assert (a.q_scale(), a.q_zero_point()) == (0.13, 0) and q._btx_sample == 5   # max(0.1, 0.13); the counter advances
    b = q.forward_int8(x, sample_idx=4, residual=res)
    assert torch.equal(a.int_repr(), b.int_repr())
    from bayesian_torch_amd import q8
    two = q8.add(q.forward_int8(x, sample_idx=4), res, 0.13, 0, True)
    assert torch.equal(a.int_repr(), two.int_repr())


# ---- the reference's Bottleneck -------------------------------------------------------------------------------------------
def test_reference_bottleneck_fixture_stage_by_stage():
    """every stage on the reference's recorded input with its recorded eps: convs are the model's bits (hence the reference's
    within 1 LSB / 0.5 %), ReLU and add exact, and the fused conv3 + add + ReLU is the block output under the same cap"""
    from bayesian_torch_amd import q8
    d = H.fixture("q8net_bottleneck")
    outs = {}
    for k in (1, 2, 3):
        c = dict(H.sub(d, "c%d_" % k), kind=np.int64(1))
        q = H.quantized_layer(c, DEV)
        outs[k] = (q, c)
        o = q.forward_int8(_qt(c["x_i"], float(c["s_x"]), int(c["z_x"])), noise=dict(eps_w=torch.from_numpy(c["eps"]), eps_b=None))
        assert np.array_equal(_np(o.int_repr()), H.model_record(c)["out"])
        H.assert_close_to_reference(_np(o.int_repr()), c, "bottleneck conv%d (GPU)" % k)
        z = 128 if k < 3 else 0
        assert np.array_equal(_np(q8.relu(_qt(d["relu%d_in" % k], 0.1, z)).int_repr()), d["relu%d_out" % k])
    q3, c3 = outs[3]
    s_add = float(d["add_scale"])
    a, r = _qt(c3["ref_out_i"], float(c3["s_o"]), int(c3["z_o"])), _qt(d["x_i"], 0.1, 128)
    assert np.array_equal(_np(q8.add(a, r, s_add, 0).int_repr()), d["add_out"])
    assert np.array_equal(_np(q8.add(a, r, s_add, 0, True).int_repr()), d["out_i"])
    fused = q3.forward_int8(_qt(c3["x_i"], 0.1, 128), noise=dict(eps_w=torch.from_numpy(c3["eps"]), eps_b=None), residual=r)
    assert (fused.q_scale(), fused.q_zero_point()) == (s_add, 0)
    mod = QN.add(H.model_record(c3)["out"], float(c3["s_o"]), int(c3["z_o"]), d["x_i"], 0.1, 128, s_add, 0, True)
    assert np.array_equal(_np(fused.int_repr()), mod)
    H.assert_close_to_reference(_np(fused.int_repr()), dict(ref_out_i=d["out_i"]), "bottleneck conv3 + add + relu (GPU)")


# ---- blocks through BTX-RNG -----------------------------------------------------------------------------------------------
def _block(kind):
    """-> (QBasicBlock | QBottleneck on the GPU, {conv name: its source float layer}, channels in)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet as R, bnn_to_qbnn
    from bayesian_torch_amd.models.qresnet import QBasicBlock, QBottleneck
    torch.manual_seed(31)
    if kind == "basic":
        cin, blk = 16, R.BasicBlock(16, 16)
    elif kind == "basic_down":
        cin, blk = 16, R.BasicBlock(16, 32, 2, nn.Sequential(nn.Conv2d(16, 32, 1, 2, bias=False), nn.BatchNorm2d(32)))
    else:
        cin, blk = 32, R.Bottleneck(32, 8)
    for m in blk.modules():
        if isinstance(m, nn.Conv2d):
            n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
            m.weight.data.normal_(0, (2.0 / n) ** 0.5)
        elif isinstance(m, nn.BatchNorm2d):   # a fold that is not the identity
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.3)
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 2.0)
    blk.eval()
    bt.dnn_to_bnn(blk, PRIOR)
    blk.to(DEV)
    src = {n: m for n, m in blk.named_modules() if hasattr(m, "_btx_layer_id")}
    bnn_to_qbnn(blk, fuse_conv_bn=True)
    return (QBottleneck if kind == "bottleneck" else QBasicBlock)(blk), src, cin


def _model_conv(q, f, x_i, s_x, z_x, s_idx, relu):
    nz = f.materialize_noise(s_idx)
    s_eps, s_d, s_w = Q.default_scales(q._q8_scales[1], q._q8_scales[0])
    pr = lambda v: v if isinstance(v, int) else tuple(v)  # noqa: E731
    r = Q.layer_forward(x_i, z_x, s_x, _np(q.quantized_mu_weight).astype(np.int32), q._q8_scales[0],
                        _np(q.quantized_sigma_weight).astype(np.int32), q._q8_scales[1], _np(nz["eps_w"]),
                        _np(q.quantized_mu_bias) if q.bias else None,
                        _np(q.quantized_sigma_bias) if (q.bias and q.quantized_sigma_bias is not None) else None,
                        _np(nz["eps_b"]) if (q.bias and q.quantized_sigma_bias is not None) else None, s_eps, s_d, s_w, 0.1, 128,
                        relu=relu, stride=pr(q.stride), padding=pr(q.padding), dilation=pr(q.dilation))
    return r["out"]


@pytest.mark.parametrize("kind", ["basic", "basic_down", "bottleneck"])
def test_blocks_through_btx_rng_equal_the_model_fused_and_unfused(kind):
    import bayesian_torch_amd as bt
    bt.manual_seed(123)
    blk, src, cin = _block(kind)
    x_i = np.maximum(_bytes((2, cin, 9, 9), 13), 128 - 20)   # like a post-ReLU map with some room below the zero point
    x = _qt(x_i, 0.1, 128)
    s_idx = 3
    outs = {}
    with torch.no_grad():
        for fuse in (True, False):
            blk.fuse_add = fuse
            bt.set_sample_index(blk, s_idx)
            outs[fuse] = blk(x)
    assert torch.equal(outs[True].int_repr(), outs[False].int_repr())
    assert (outs[True].q_scale(), outs[True].q_zero_point()) == (0.1, 0)
    cur = x_i
    names = blk._convs
    for n in names[:-1]:
        cur = _model_conv(getattr(blk, n), src[n], cur, 0.1, 128, s_idx, True)
    last = _model_conv(getattr(blk, names[-1]), src[names[-1]], cur, 0.1, 128, s_idx, False)
    res = x_i if blk.downsample is None else _model_conv(blk.downsample[0], src["downsample.0"], x_i, 0.1, 128, s_idx, False)
    ref = QN.add(last, 0.1, 128, res, 0.1, 128, 0.1, 0, True)
    assert np.array_equal(_np(outs[True].int_repr()), ref)
    print("block %s: saturated %.3f" % (kind, _sat(ref)))
    with torch.no_grad():
        bt.set_sample_index(blk, s_idx + 1)
        assert not torch.equal(blk(x).int_repr(), outs[True].int_repr())   # another sample index, another draw


# ---- the network ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet as R, to_qresnet
    bt.manual_seed(5)
    torch.manual_seed(6)
    m = R.resnet18().eval()
    m.avgpool = nn.AvgPool2d(2)
    bt.dnn_to_bnn(m, PRIOR)
    m.to(DEV)
    q = to_qresnet(m)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    return q, x


def test_qresnet18_fused_add_on_equals_off():
    import bayesian_torch_amd as bt
    q, x = _net()
    outs = {}
    with torch.no_grad():
        for fuse in (True, False, True):
            q.set_fuse_add(fuse)
            bt.set_sample_index(q, 7)
            y = q(x)
            assert y.dtype == torch.float32 and y.shape == (2, 1000) and torch.isfinite(y).all()
            assert fuse not in outs or torch.equal(outs[fuse], y)
            outs[fuse] = y.clone()
    assert torch.equal(outs[True], outs[False])
    assert len(torch.unique(outs[True])) > 1


def test_qresnet18_graph_replay_and_mc_forward():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    q, x = _net()
    q.set_fuse_add(True)
    eager = {}
    with torch.no_grad():
        for s in (5, 0, 1, 2):
            bt.set_sample_index(q, s)
            eager[s] = q(x).clone()
    g = mc.GraphedMC(q, x, lanes=1, keep_logits=True)
    try:
        for s in (5, 0, 2):
            g.run(s)
            torch.cuda.synchronize()
            assert torch.equal(g.lane_logits[0], eager[s]), s
    finally:
        g.close()
    packed = mc.mc_forward(q, x, 3, lanes=1)
    ref = torch.zeros_like(packed)
    for s in (0, 1, 2):
        mc.accumulate_lanes(ref, eager[s], 1, 0.0)
    assert torch.isfinite(packed).all() and torch.equal(packed, ref)
    with torch.no_grad():
        bt.set_sample_index(q, 5)
        assert torch.equal(q(x), eager[5])
