"""INT8 Flipout without a GPU: the numpy model (tests/q8_flipout_model.py) against the reference's fixtures under the conditions
the fixture generator asserted, the twins' surface and state dict, bnn_to_qbnn(flipout=True) / to_qresnet, the CPU forward against
the fixtures' torch op chain, and the host-side argument checks of the two new entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import q8_flipout_helpers as F
import q8_flipout_model as QF
import q8_model as Q

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout", moped_enable=True,
             moped_delta=0.5)


# ---- the model against the reference ------------------------------------------------------------------------------------------
def test_mul_model_equals_torch_exactly():
    g = np.random.default_rng(3)
    for _ in range(40):
        sa, sb, so = (float(v) for v in g.uniform(0.002, 0.2, 3))
        za, zb, zo = (int(v) for v in g.integers(0, 256, 3))
        a, b = g.integers(0, 256, 300).astype(np.uint8), g.integers(0, 256, 300).astype(np.uint8)
        ta = torch._make_per_tensor_quantized_tensor(torch.from_numpy(a), sa, za)
        tb = torch._make_per_tensor_quantized_tensor(torch.from_numpy(b), sb, zb)
        ref = torch.ops.quantized.mul(ta, tb, so, zo).int_repr().numpy()
        assert np.array_equal(ref, QF.qmul(a, za, b, zb, QF.mul_multiplier(sa, sb, so), zo, 0, 255))
    assert QF.sign_bytes((2 / 255, 128)) == (255, 1)   # a quantized sign is not exactly +-1: the bytes are 255 and 1


@pytest.mark.parametrize("name", F.CASES)
def test_model_meets_the_fixture_conditions(name):
    d = F.fixture(name)
    m = F.model_record(d)
    e = F.entries(d)
    meta = json.loads(str(d["meta"]))
    assert meta["source"].startswith("reference forward == op chain")
    assert len(e) == 10 and e[0][1] == 0 and e[1][1] == 0
    assert np.array_equal(m["d_i"], d["ref_d_i"]) and np.array_equal(m["xp"], d["ref_xp"])
    assert np.array_equal(m["bm_i"], d["bm_i"]) and np.array_equal(m["bp_i"], d["bp_i"])
    for k in ("o1", "p"):
        diff = np.abs(m[k].astype(np.int32) - d["ref_" + k].astype(np.int32))
        frac = float((diff != 0).mean())
        print("%s %s: max %d LSB, share %.4f%%" % (name, k, diff.max(), 100 * frac))
        assert diff.max() <= F.MAX_LSB and frac <= F.MAX_FRAC
        assert abs(frac - meta[k + "_share"]) < 1e-12
    p2, out = QF.tail(d["ref_o1"], d["ref_p"], d["sign_out"], e, bool(d["relu"]))
    assert np.array_equal(p2, d["ref_p2"]) and np.array_equal(out, d["ref_out"])
    dd = m["out"].astype(np.int32) != d["ref_out"].astype(np.int32)
    inner = (m["o1"] != d["ref_o1"]) | (m["p"] != d["ref_p"])
    assert not np.any(dd & ~inner)
    print("%s end to end: max %d LSB, share %.4f%%" % (name, np.abs(m["out"].astype(np.int32) - d["ref_out"]).max(), 100 * dd.mean()))


def test_calibrated_fixture_has_real_entries_and_a_symmetric_check():
    d = F.fixture("q8f_conv_calibrated")
    e = F.entries(d)
    assert len({z for _, z in e[2:]}) > 3 and all(s > 0 for s, _ in e)
    bad = [list(v) for v in e]
    bad[1][1] = 3
    with pytest.raises(ValueError):
        QF.layer_forward(d["x_i"], F.e_x(d), d["mu_i"], float(d["s_mu"]), d["sigma_i"], float(d["s_sigma"]), d["eps"], None, None,
                         d["sign_in"], d["sign_out"], bad)


# ---- the twins ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CASES)
def test_twin_holds_the_references_int8_weights_and_its_cpu_forward_is_the_op_chain(name):
    d = F.fixture(name)
    q = F.quantized_layer(d)
    conv = int(d["kind"]) == 1
    assert type(q).__name__ == ("QuantizedConv2dFlipout" if conv else "QuantizedLinearFlipout")
    assert np.array_equal(q.quantized_mu_weight.numpy(), d["mu_i"]) and np.array_equal(q.quantized_sigma_weight.numpy(), d["sigma_i"])
    assert q._q8_scales == (float(d["s_mu"]), float(d["s_sigma"]))
    if "mu_b_q" in d:
        assert np.array_equal(q.quantized_mu_bias.numpy(), d["mu_b_q"])
    if "sigma_b_q" in d:
        assert np.array_equal(q.quantized_sigma_bias.numpy(), d["sigma_b_q"])
    assert [F.KINDS.index(k) for k in q._bias_kinds(bool(d["calibrated"]))] == d["kinds"].tolist()
    xq = torch._make_per_tensor_quantized_tensor(torch.from_numpy(d["x_i"]), *F.e_x(d))
    out, parts = q.forward_int8(xq, noise=F.noise_of(d), parts=True)
    for k in ("d_i", "xp", "o1", "p", "p2"):
        assert np.array_equal(parts[k].int_repr().numpy(), d["ref_" + k]), k
    if conv:
        assert out.dtype == torch.quint8 and np.array_equal(out.int_repr().numpy(), d["ref_out"])
    else:
        e9 = F.entries(d)[9]
        assert out.dtype == torch.float32 and np.array_equal(out.numpy(), Q.dequantize(d["ref_out"], *e9))
    # float input: quantized at entry 2 (the default path: at the defaults); signs and eps from the torch generator
    torch.manual_seed(1)
    y, kl = q(torch.from_numpy(d["x"]))
    assert kl == 0 and (y.dtype == (torch.quint8 if conv else torch.float32))
    torch.manual_seed(2)
    y2 = q(torch.from_numpy(d["x"]), return_kl=False)
    assert not torch.equal(y2.int_repr() if conv else y2, y.int_repr() if conv else y)


def test_class_surface_and_state_dict_round_trip():
    from bayesian_torch_amd import layers as L
    import inspect
    assert list(inspect.signature(L.QuantizedLinearFlipout.__init__).parameters)[1:] == ["in_features", "out_features"]
    assert list(inspect.signature(L.QuantizedConv2dFlipout.__init__).parameters)[1:] == [
        "in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "bias"]
    sig = inspect.signature(L.QuantizedConv2dFlipout.forward).parameters
    assert list(sig)[1:] == ["x", "normal_scale", "default_scale", "default_zero_point", "return_kl"]
    assert (sig["normal_scale"].default, sig["default_scale"].default, sig["default_zero_point"].default) == (6 / 255, 0.1, 128)
    assert inspect.signature(L.QuantizedLinearFlipout.forward).parameters["default_scale"].default == 0.1
    for name in ("q8f_conv_calibrated", "q8f_linear_default"):
        d = F.fixture(name)
        q = F.quantized_layer(d)
        assert q._btx_q8 and q.kl_loss() == 0 and q.quant_prepare is False
        for a in ("quantize", "get_scale_and_zero_point", "get_quantized_tensor", "quantized_mu_weight", "quantized_sigma_weight",
                  "quantized_mu_bias", "quantized_sigma_bias", "quant_dict", "forward_int8"):
            assert hasattr(q, a), a
        if int(d["kind"]) == 1:
            assert q.relu is False and not hasattr(q, "bn_weight")
        assert q.quantized_mu_weight.dtype == torch.int8
        sd = q.state_dict()
        conv = int(d["kind"]) == 1
        q2 = L.QuantizedConv2dFlipout(q.in_channels, q.out_channels, q.kernel_size, q.stride, q.padding, q.dilation, 1, True) if conv \
            else L.QuantizedLinearFlipout(q.in_features, q.out_features)
        q2.quantize()
        q2.load_state_dict(sd)
        assert q2._q8_scales == q._q8_scales and q2._quant_entries() == q._quant_entries()
        xq = torch._make_per_tensor_quantized_tensor(torch.from_numpy(d["x_i"]), *F.e_x(d))
        a, b = (t.forward_int8(xq, noise=F.noise_of(d)) for t in (q, q2))
        assert torch.equal(a.int_repr(), b.int_repr()) if conv else torch.equal(a, b)
    q.quant_dict = [(0.1, 0)] * 5
    with pytest.raises(Exception, match="ten"):
        q(torch.zeros(1, q.in_features))
    q.quant_dict = [(0.1, 0), (0.1, 4)] + [(0.1, 128)] * 8
    with pytest.raises(Exception, match="symmetric"):
        q(torch.zeros(1, q.in_features))


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        from bayesian_torch_amd import layers as L
        self.conv1 = L.Conv2dFlipout(8, 6, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(6)
        self.fc = L.LinearFlipout(6 * 5 * 5, 10)
        self.rep = L.Conv2dReparameterization(8, 8, 3, padding=1)

    def forward(self, x):
        x = self.bn1(self.conv1(x)[0])
        x = x.dequantize() if x.is_quantized else x
        return self.fc(torch.relu(x).flatten(1))[0]


def test_bnn_to_qbnn_flipout_flow_prepare_calibrate_convert():
    from bayesian_torch_amd.models import bnn_to_qbnn
    torch.manual_seed(11)
    m = Net().eval()
    with torch.no_grad():
        m.bn1.running_mean.normal_(0, 0.3)
        m.bn1.running_var.uniform_(0.5, 2.0)
    ids = (m.conv1._btx_layer_id, m.fc._btx_layer_id)
    m.conv1._btx_sample = 7
    m.conv1.prepare()
    m.fc.prepare()
    assert (len(m.conv1.qint_quant), len(m.conv1.quint_quant)) == (4, 8) and m.fc.quant_prepare
    torch.quantization.prepare(m, inplace=True)
    with torch.no_grad():
        for _ in range(3):
            y = m(torch.randn(4, 8, 5, 5) * 2)
    assert y.shape == (4, 10)
    torch.quantization.convert(m, inplace=True)
    import copy
    left = copy.deepcopy(m)
    bnn_to_qbnn(left, fuse_conv_bn=True)   # the default leaves a Flipout layer alone
    assert type(left.conv1).__name__ == "Conv2dFlipout" and type(left.fc).__name__ == "LinearFlipout"
    assert type(left.rep).__name__ == "QuantizedConv2dReparameterization" and isinstance(left.bn1, nn.BatchNorm2d)
    bnn_to_qbnn(m, fuse_conv_bn=True, flipout=True)
    assert type(m.conv1).__name__ == "QuantizedConv2dFlipout" and type(m.fc).__name__ == "QuantizedLinearFlipout"
    assert isinstance(m.bn1, nn.Identity) and m.conv1.bias and m.conv1.quantized_sigma_bias is None   # the folded BatchNorm's bias
    assert (m.conv1._btx_layer_id, m.fc._btx_layer_id) == ids and m.conv1._btx_sample == 7
    for q in (m.conv1, m.fc):
        e = q._quant_entries()
        assert len(e) == 10 and e[0][1] == 0 and e[1][1] == 0 and all(s > 0 for s, _ in e)
        assert not hasattr(q, "qint_quant")
    # the calibrated sign entries: range [-1, 1] -> scale 2 / 255
    assert abs(m.conv1._quant_entries()[4][0] - 2 / 255) < 1e-6
    with torch.no_grad():
        y = m(torch.randn(4, 8, 5, 5) * 2)
    assert y.shape == (4, 10) and torch.isfinite(y).all()


def _tiny_resnet():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet as R
    torch.manual_seed(4)
    m = R.ResNet(R.BasicBlock, [1, 1, 1, 1], num_classes=10).eval()
    m.avgpool = nn.AvgPool2d(1)
    bt.dnn_to_bnn(m, PRIOR)
    return m


def test_to_qresnet_on_a_tiny_flipout_resnet_runs_on_cpu_tensors():
    from bayesian_torch_amd.models import to_qresnet, qresnet18
    q = to_qresnet(_tiny_resnet())
    names = {type(m).__name__ for m in q.modules() if hasattr(m, "_btx_layer_id")}
    assert names == {"QuantizedConv2dFlipout", "QuantizedLinearFlipout"}
    assert q.conv1.relu and q.layer1[0].conv1.relu and not q.layer1[0].conv2.relu
    torch.manual_seed(0)
    with torch.no_grad():
        y = q(torch.randn(2, 3, 16, 16))
    assert y.shape == (2, 10) and y.dtype == torch.float32 and torch.isfinite(y).all()
    big = qresnet18(num_classes=10, bnn_prior_parameters={"type": "Flipout"})
    assert type(big.conv1).__name__ == "QuantizedConv2dFlipout"
    assert type(qresnet18(num_classes=10).conv1).__name__ == "QuantizedConv2dReparameterization"


def test_lanes_and_groups_are_refused():
    from bayesian_torch_amd import _lib, layers as L
    q = F.quantized_layer(F.fixture("q8f_conv_default"))
    xq = torch._make_per_tensor_quantized_tensor(torch.from_numpy(F.fixture("q8f_conv_default")["x_i"]), 0.1, 128)
    q.__dict__["_btx_lanes"] = 2
    with pytest.raises(_lib.BtxError, match="lanes"):
        q(xq)
    q.__dict__["_btx_lanes"] = 1
    g = L.QuantizedConv2dFlipout(8, 8, 3, padding=1, groups=2)
    g.quantize()
    with pytest.raises(_lib.BtxError, match="groups"):
        g(torch.zeros(1, 8, 5, 5))
    import bayesian_torch_amd as bt
    m = nn.Sequential(q)
    with pytest.raises(_lib.BtxError, match="lanes"):
        bt.set_sample_lanes(m, [0, 1], batch=2)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_their_arguments_without_a_gpu():
    from bayesian_torch_amd import _lib, q8
    L = _lib.lib()
    assert L.btx_abi_version() == 9
    hdr = open(os.path.join(F.HERE, "..", "include", "btx.h")).read()
    for n in ("btx_q8_sample_delta", "btx_q8_contract_flipout"):
        assert n in _lib.EXPORTS and n + "(" in hdr
    al, al2 = ctypes.c_void_p(64), ctypes.c_void_p(8)
    e = QF.default_entries(0.004)
    dl = _lib.Q8Delta(42.5, 0.5, 1, 2, 0.001, 0.001)
    r = _lib.Rng(1, 0, 0, None)
    sd = lambda *a: L.btx_q8_sample_delta(*a)  # noqa: E731
    ok = (al, al, al, 16, 9, 32, 32, ctypes.byref(dl), ctypes.byref(r), None, None, al, al, al, al, None)

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return tuple(a)
    for i in (0, 7, 11, 12, 13, 14):
        assert sd(*with_(i, None)) == -1
    assert sd(*with_(8, None)) == -1          # no rng and no explicit eps
    assert sd(*with_(1, None)) == -1 and sd(*with_(2, None)) == -1   # a bias kind without its vector
    assert sd(*with_(3, 0)) == -2 and sd(*with_(4, 0)) == -2 and sd(*with_(5, 0)) == -2
    assert sd(*with_(6, 30)) == -2            # eps rows shorter than C / not a multiple of 8
    for bad in (_lib.Q8Delta(0.0, 0.5, 1, 2, 0.001, 0.001), _lib.Q8Delta(42.5, -1.0, 1, 2, 0.001, 0.001),
                _lib.Q8Delta(42.5, 0.5, 3, 2, 0.001, 0.001), _lib.Q8Delta(42.5, 0.5, 1, 2, 0.0, 0.001)):
        assert sd(*with_(7, ctypes.byref(bad))) == -2
    assert sd(*with_(11, al2)) == -6
    assert sd(*with_(4, 1 << 27)) == -3       # the weight row beyond the 32-bit image

    g = _lib.Geom()
    g.NB, g.D, g.H, g.W, g.C, g.N = 2, 1, 9, 9, 32, 16
    g.KD, g.KH, g.KW = 1, 3, 3
    g.sd = g.sh = g.sw = 1
    g.ph = g.pw = 1
    g.dd = g.dh = g.dw = 1
    g.groups = 1
    fl = q8.make_flipout(0.1, 128, 0.01, e)
    assert (fl.sin_pos, fl.sin_neg) == (10, -10) and fl.z_xp == 128
    add = q8.make_add(0.1, 128, 0.1, 128, 0.1, 128, False)
    cf = lambda *a: L.btx_q8_contract_flipout(*a)  # noqa: E731
    okc = (ctypes.byref(g), al, al, al, al, al, al, al, ctypes.byref(fl), ctypes.byref(add), ctypes.byref(r), 32, None, None, 0, al, None)

    def withc(i, v):
        a = list(okc)
        a[i] = v
        return tuple(a)
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15):
        assert cf(*withc(i, None)) == -1, i
    assert cf(*withc(10, None)) == -1         # no rng and no explicit signs
    assert cf(*withc(11, 16)) == -2           # sign rows shorter than C
    for field, v in (("z_x", 256), ("z_xp", -1), ("mult_xp", 0.0), ("mult_p2", -1.0), ("sin_pos", 300)):
        bad = q8.make_flipout(0.1, 128, 0.01, e)
        setattr(bad, field, v)
        assert cf(*withc(8, ctypes.byref(bad))) == -2, field
    bad_add = _lib.Q8Add(0.1, 0.0, 0.1, 0.0, 10.0, 300, 0)
    assert cf(*withc(9, ctypes.byref(bad_add))) == -2
    bad = q8.make_flipout(0.1, 128, 0.01, e)
    bad.out_scale = 0.0
    assert cf(*withc(8, ctypes.byref(bad))[:14] + (1, al, None)) == -2   # f32 output needs its scale
    assert cf(*withc(2, al2)) == -6 and cf(*withc(5, al2)) == -6
    g.groups = 2
    assert cf(*okc) == -3
    g.groups, g.KD = 1, 3
    assert cf(*okc) == -3
