"""INT8 inference without a GPU: the numpy model of BTX-Q8 v1 (tests/q8_model.py) and the quantized layers' CPU path against
the reference's recorded results (tests/golden/q8_*.npz), the converted models' surface, the calibrated flow, and the argument
validation of the btx_q8_* entry points."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import q8_helpers as H
import q8_model as Q

RECORDS = [(n, "") for n in H.SINGLE] + [("q8_calibrated", "conv_"), ("q8_calibrated", "fc_")]


@pytest.mark.parametrize("name,prefix", RECORDS)
def test_numpy_model_against_the_reference(name, prefix):
    """W exact; the output within 1 LSB in at most 0.5 % of the elements"""
    d = H.sub(H.fixture(name), prefix) if prefix else H.fixture(name)
    r = H.model_record(d)
    assert np.array_equal(r["W"], d["ref_W"].astype(np.int32))
    assert np.array_equal(r["S"], d["ref_W"].reshape(d["ref_W"].shape[0], -1).astype(np.int64).sum(1))
    H.assert_close_to_reference(r["out"], d, name + prefix)
    if d["ref_out"].ndim == 2:  # Linear: the reference returns the dequantized output
        assert np.array_equal(Q.dequantize(d["ref_out_i"], float(d["s_o"]), int(d["z_o"])), d["ref_out"])


def test_stored_int8_weights_and_scales_follow_the_reference():
    for name in H.SINGLE:
        d = H.fixture(name)
        q = H.quantized_layer(d)
        assert q.quantized_mu_weight.dtype == torch.int8 and q.quantized_sigma_weight.dtype == torch.int8
        assert np.array_equal(q.quantized_mu_weight.numpy(), d["mu_i"]), name
        assert np.array_equal(q.quantized_sigma_weight.numpy(), d["sigma_i"]), name
        assert (q.mu_weight_scale(), q.sigma_weight_scale()) == (float(d["s_mu"]), float(d["s_sigma"]))
        assert np.array_equal(q.quantized_mu_bias.numpy(), d["mu_b_q"])
        assert np.array_equal(q.quantized_sigma_bias.numpy(), d["sigma_b_q"])
        # and the numpy model's own host-side quantization agrees
        if "bn_weight" not in d:
            mu_i, s_mu = Q.quantize_weight(d["f_mu"])
            # (sigma through torch's log1p / exp: the two libraries' transcendentals differ in the last bit)
            sg_i, s_sg = Q.quantize_weight(torch.log1p(torch.exp(torch.from_numpy(d["f_rho"]))).numpy())
            assert s_mu == float(d["s_mu"]) and np.array_equal(mu_i, d["mu_i"])
            assert s_sg == float(d["s_sigma"]) and np.array_equal(sg_i, d["sigma_i"])


@pytest.mark.parametrize("name", H.SINGLE)
def test_cpu_layers_with_the_fixture_noise(name):
    """the layers on CPU tensors, seeded exactly as the generator of the fixture was: the reference's draw order"""
    d = H.fixture(name)
    q = H.quantized_layer(d)
    x = torch.from_numpy(d["x"])
    torch.manual_seed(int(d["seed_fwd"]))
    out, kl = q(x)
    assert kl == 0
    assert np.array_equal(getattr(q, "eps_" + q._wn).numpy(), d["eps"])
    assert np.array_equal(q.eps_bias.numpy(), d["eps_b"])
    if int(d["kind"]) == 0:
        assert out.dtype == torch.float32
        out_i = np.rint(out.numpy() / np.float32(d["s_o"])).astype(np.int32) + int(d["z_o"])
        assert np.array_equal(Q.dequantize(out_i.astype(np.uint8), float(d["s_o"]), int(d["z_o"])), out.numpy())
    else:
        assert out.dtype == torch.quint8 and (out.q_scale(), out.q_zero_point()) == (float(d["s_o"]), int(d["z_o"]))
        out_i = out.int_repr().numpy()
    H.assert_close_to_reference(out_i, d, name + " (CPU layer)")
    # a quantized input (torch.quint8, or the carrier) is taken as it is
    from bayesian_torch_amd.q8 import QTensor
    xq = torch.quantize_per_tensor(x, float(d["s_x"]), int(d["z_x"]), torch.quint8)
    for inp in (xq, QTensor(xq.int_repr(), float(d["s_x"]), int(d["z_x"]))):
        torch.manual_seed(int(d["seed_fwd"]))
        o2 = q(inp, return_kl=False)
        assert torch.equal(o2.int_repr() if o2.is_quantized else o2, out.int_repr() if out.is_quantized else out)


class Net(nn.Module):
    """conv -> dequantize -> ReLU -> flatten -> Linear: the model of the calibrated fixture"""

    def __init__(self):
        super().__init__()
        from bayesian_torch_amd import layers as L
        self.conv = L.Conv2dReparameterization(8, 6, 3, stride=1, padding=1, bias=True)
        self.fc = L.LinearReparameterization(6 * 5 * 5, 10)

    def forward(self, x):
        x = self.conv(x)[0]
        if getattr(x, "is_quantized", False):
            x = x.dequantize()
        return self.fc(torch.relu(x).flatten(1))[0]


def _load(net, d):
    with torch.no_grad():
        for lay, pre, wn in ((net.conv, "conv_f_", "kernel"), (net.fc, "fc_f_", "weight")):
            getattr(lay, "mu_" + wn).copy_(torch.from_numpy(d[pre + "mu"]))
            getattr(lay, "rho_" + wn).copy_(torch.from_numpy(d[pre + "rho"]))
            lay.mu_bias.copy_(torch.from_numpy(d[pre + "mu_b"]))
            lay.rho_bias.copy_(torch.from_numpy(d[pre + "rho_b"]))


def test_calibrated_flow_end_to_end():
    """prepare -> torch.quantization.prepare -> 4 calibration batches -> convert -> bnn_to_qbnn on a conv -> Linear model: five
    quant_dict entries per layer, the two affine ones equal to the reference's (min / max observers of deterministic tensors),
    and — with the reference's own quant_dict — its output"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import bnn_to_qbnn
    d = H.fixture("q8_calibrated")
    net = Net().eval()
    _load(net, d)
    net.conv.prepare()
    net.fc.prepare()
    assert len(net.conv.qint_quant) == 5 and len(net.conv.quint_quant) == 2 and net.conv.quant_prepare
    torch.quantization.prepare(net, inplace=True)
    torch.manual_seed(1)
    with torch.no_grad():
        for b in d["calib"]:
            net(torch.from_numpy(b))
    torch.quantization.convert(net, inplace=True)
    bnn_to_qbnn(net)
    assert type(net.conv).__name__ == "QuantizedConv2dReparameterization" and type(net.fc).__name__ == "QuantizedLinearReparameterization"
    for lay, pre in ((net.conv, "conv_"), (net.fc, "fc_")):
        qd = lay._quant_entries()
        assert len(qd) == 5 and all(s > 0 for s, _ in qd) and [z for _, z in qd[:3]] == [0, 0, 0]
        assert not hasattr(lay, "qint_quant") and not hasattr(lay, "quint_quant")
    # the input range of the first layer is noise-free: its calibrated pair is the reference's
    assert net.conv._quant_entries()[3] == (float(d["conv_s_x"]), int(d["conv_z_x"]))
    assert bt.get_kl_loss(net) == 0
    y = net(torch.from_numpy(d["x"]))
    assert y.shape == (4, 10) and torch.isfinite(y).all()
    # with the reference's calibration result and its noise: its numbers
    net.conv.quant_dict = H.quant_dict_of(H.sub(d, "conv_"))
    net.fc.quant_dict = H.quant_dict_of(H.sub(d, "fc_"))
    torch.manual_seed(int(d["seed_fwd"]))
    y = net(torch.from_numpy(d["x"]))
    fc = H.sub(d, "fc_")
    assert np.array_equal(net.fc.eps_weight.numpy(), fc["eps"])
    out_i = np.rint(y.numpy() / np.float32(fc["s_o"])).astype(np.int32) + int(fc["z_o"])
    H.assert_close_to_reference(out_i, fc, "calibrated conv -> Linear")


def test_quant_dict_with_a_zero_point_in_a_qint8_entry_raises():
    from bayesian_torch_amd._lib import BtxError
    d = H.fixture("q8_linear_default")
    q = H.quantized_layer(d)
    qd = H.quant_dict_of(d)
    qd[1] = (qd[1][0], 3)
    q.quant_dict = qd
    with pytest.raises(BtxError, match="mul"):
        q(torch.from_numpy(d["x"]))


def test_converted_model_surface():
    """class and attribute names, (out, 0), kl_loss() == 0, get_kl_loss; Flipout and LSTM layers stay; fuse_model skips a twin"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = L.Conv2dReparameterization(4, 8, 3, padding=1, bias=False)
            self.bn1 = nn.BatchNorm2d(8)
            self.flip = L.Conv2dFlipout(8, 8, 3, padding=1)
            self.lstm = L.LSTMReparameterization(8, 4)
            self.c1d = L.Conv1dReparameterization(4, 4, 3)
            self.fc = L.LinearReparameterization(8, 5, bias=False)

    m = M().eval()
    ids = (m.conv1._btx_layer_id, m.fc._btx_layer_id)
    bnn_to_qbnn(m, fuse_conv_bn=True)
    assert type(m.conv1).__name__ == "QuantizedConv2dReparameterization" and isinstance(m.bn1, nn.Identity)
    assert type(m.fc).__name__ == "QuantizedLinearReparameterization"
    assert type(m.flip).__name__ == "Conv2dFlipout" and type(m.c1d).__name__ == "Conv1dReparameterization"
    assert type(m.lstm).__name__ == "LSTMReparameterization" and type(m.lstm.ih).__name__ == "LinearReparameterization"
    assert (m.conv1._btx_layer_id, m.fc._btx_layer_id) == ids
    for lay in (m.conv1, m.fc):
        names = dict(lay.named_buffers())
        assert {"quantized_mu_weight", "quantized_sigma_weight"} <= set(names)
        assert not hasattr(lay, "mu_kernel") and not hasattr(lay, "mu_weight") and not hasattr(lay, "bn_weight")
        assert lay.kl_loss() == 0 and lay.quant_dict is None
    assert m.conv1.bias is True and m.conv1.quantized_sigma_bias is None and m.conv1.quantized_mu_bias.shape == (8,)
    assert m.fc.bias is False and m.fc.quantized_mu_bias is None
    out = m.conv1(torch.randn(2, 4, 6, 6))
    assert isinstance(out, tuple) and out[1] == 0 and out[0].dtype == torch.quint8
    out = m.fc(torch.randn(3, 8))
    assert isinstance(out, tuple) and out[1] == 0 and out[0].dtype == torch.float32
    assert m.fc(torch.randn(3, 8), return_kl=False).shape == (3, 5)
    only = nn.Sequential(m.conv1, m.fc)
    assert bt.get_kl_loss(only) == 0
    # state_dict round trip keeps the int8 buffers and the scales
    twin = L.QuantizedLinearReparameterization(8, 5)
    twin.bias = False
    twin.mu_bias = twin.rho_bias = None
    twin.quantize()
    twin.load_state_dict(m.fc.state_dict())
    assert twin._q8_scales == m.fc._q8_scales and torch.equal(twin.quantized_mu_weight, m.fc.quantized_mu_weight)
    from bayesian_torch_amd.models import fuse as F
    assert not F._is_var(m.conv1) and F._is_q8(m.conv1)   # fuse_model: a leaf of the trace, never an epilogue site


def test_fuse_model_leaves_a_quantized_layer_alone():
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn, fuse_model

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.q = L.Conv2dReparameterization(4, 8, 3, padding=1)
            self.f = nn.Sequential(L.Conv2dReparameterization(8, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU())

        def forward(self, x):
            x = self.q(x)[0].dequantize()
            return self.f[2](self.f[1](self.f[0](x)[0]))

    m = M().eval()
    wrap = nn.Module()
    wrap.q = m.q
    bnn_to_qbnn(wrap)
    m.q = wrap.q
    q = m.q
    buf = q.quantized_mu_weight.clone()
    fuse_model(m)
    assert m.q is q and torch.equal(q.quantized_mu_weight, buf) and not hasattr(q, "forward_fused")
    torch.manual_seed(0)
    assert m(torch.randn(1, 4, 5, 5)).shape == (1, 8, 5, 5)


def test_q8_entry_points_validate_their_arguments_without_a_gpu():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9
    assert L.btx_q8_weight_row_bytes(1, 96) == 128 and L.btx_q8_weight_row_bytes(9, 32) == 320
    assert L.btx_q8_weight_row_bytes(49, 3) == 832 and L.btx_q8_weight_row_bytes(0, 3) == 0
    one, al = ctypes.c_void_p(16), ctypes.c_void_p(64)
    st = (ctypes.c_int64 * 4)(1, 1, 1, 1)
    assert L.btx_q8_quantize_act(None, 0, st, one, 1, 1, 1, 1, 0.1, 128, None) == -1
    assert L.btx_q8_quantize_act(one, 0, None, one, 1, 1, 1, 1, 0.1, 128, None) == -1
    assert L.btx_q8_quantize_act(one, 0, st, one, 1, 0, 1, 1, 0.1, 128, None) == -2
    assert L.btx_q8_quantize_act(one, 0, st, one, 1, 1, 1, 1, 0.0, 128, None) == -2
    assert L.btx_q8_quantize_act(one, 0, st, one, 1, 1, 1, 1, 0.1, 256, None) == -2
    assert L.btx_q8_quantize_act(one, 7, st, one, 1, 1, 1, 1, 0.1, 128, None) == -5
    assert L.btx_q8_quantize_act(one, 0, st, ctypes.c_void_p(18), 1, 1, 1, 1, 0.1, 128, None) == -6
    ch = _lib.Q8Chain(0.01, 0.01, 0.02, 50.0, 0.0002, 5000.0, 100.0, 0.002)
    r = _lib.Rng(1, 2, 3, None)
    sw = lambda *a: L.btx_q8_sample_weights(*a)  # noqa: E731
    assert sw(None, al, None, None, 4, 1, 8, 8, ctypes.byref(ch), ctypes.byref(r), None, None, al, al, al, None) == -1
    assert sw(al, al, None, None, 4, 1, 8, 8, None, ctypes.byref(r), None, None, al, al, al, None) == -1
    assert sw(al, al, None, None, 4, 1, 8, 8, ctypes.byref(ch), None, None, None, al, al, al, None) == -1      # no noise source
    assert sw(al, al, None, al, 4, 1, 8, 8, ctypes.byref(ch), ctypes.byref(r), None, None, al, al, al, None) == -1  # sigma_b without mu_b
    assert sw(al, al, None, None, 0, 1, 8, 8, ctypes.byref(ch), ctypes.byref(r), None, None, al, al, al, None) == -2
    assert sw(al, al, None, None, 4, 1, 6, 6, ctypes.byref(ch), ctypes.byref(r), None, None, al, al, al, None) == -2  # RNG rows: multiples of 8
    assert sw(al, al, None, None, 4, 1, 8, 8, ctypes.byref(ch), ctypes.byref(r), None, None, ctypes.c_void_p(8), al, al, None) == -6
    bad = _lib.Q8Chain(0.01, 0.01, 0.0, 50.0, 0.0002, 5000.0, 100.0, 0.002)
    assert sw(al, al, None, None, 4, 1, 8, 8, ctypes.byref(bad), ctypes.byref(r), None, None, al, al, al, None) == -2
    g = _lib.Geom()
    g.NB, g.D, g.H, g.W, g.C, g.N = 2, 1, 9, 9, 32, 16
    g.KD, g.KH, g.KW = 1, 3, 3
    g.sd = g.sh = g.sw = 1
    g.ph = g.pw = 1
    g.dd = g.dh = g.dw = 1
    g.groups = 1
    ct = lambda *a: L.btx_q8_contract(*a)  # noqa: E731
    assert ct(None, al, 128, al, al, al, 0.01, 128, 0, 0, 0.1, al, None) == -1
    assert ct(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, 0.1, None, None) == -1
    assert ct(ctypes.byref(g), al, 300, al, al, al, 0.01, 128, 0, 0, 0.1, al, None) == -2
    assert ct(ctypes.byref(g), al, 128, al, al, al, 0.0, 128, 0, 0, 0.1, al, None) == -2
    assert ct(ctypes.byref(g), al, 128, ctypes.c_void_p(8), al, al, 0.01, 128, 0, 0, 0.1, al, None) == -6
    g.groups = 2
    assert ct(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, 0.1, al, None) == -3
    g.groups, g.KD = 1, 3
    assert ct(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, 0.1, al, None) == -3
    g.KD, g.KH = 1, 30
    assert ct(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, 0.1, al, None) == -2


def test_grouped_quantized_conv_raises():
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd._lib import BtxError
    q = L.QuantizedConv2dReparameterization(8, 8, 3, groups=2)
    q.quantize()
    with pytest.raises(BtxError, match="groups"):
        q(torch.randn(1, 8, 5, 5))
