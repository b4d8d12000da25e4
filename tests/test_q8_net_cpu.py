"""The INT8 network ops without a GPU: the numpy model of the add / pooling arithmetic (tests/q8_net_model.py) against torch's own
quantized ops and the reference's Bottleneck (tests/golden/q8net_*.npz, written by tools/make_golden_q8net.py), the argument
validation of the four new entry points, the structure to_qresnet builds, and a QResNet forward on CPU tensors against the same
torch ops applied by hand."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import q8_helpers as H
import q8_net_model as QN

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Reparameterization",
             moped_enable=True, moped_delta=0.5)   # MOPED: the means are the He-initialised weights, activations stay O(1)


def _quint8(q, s, z):
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(np.ascontiguousarray(q)), s, z)


# ---- the model against the fixtures ---------------------------------------------------------------------------------------
def test_add_model_equals_torch_exactly():
    """every fixture tensor has a multiple of 64 elements (torch's vector body only): 0 differing elements"""
    d = H.fixture("q8net_ops")
    a, b, z_a, z_b = d["add_a"], d["add_b"], int(d["add_z_a"]), int(d["add_z_b"])
    assert a.size % 64 == 0
    naive = 0
    for i, (s_a, s_b) in enumerate(d["add_pairs"]):
        s_a, s_b = float(s_a), float(s_b)
        for z in d["add_zero_points"]:
            for relu in (0, 1):
                ref = d["add_out_%d_%d_%d" % (i, int(z), relu)]
                assert np.array_equal(QN.add(a, s_a, z_a, b, s_b, z_b, max(s_a, s_b), int(z), bool(relu)), ref), (i, int(z), relu)
                naive += int((QN.add_naive(a, s_a, z_a, b, s_b, z_b, max(s_a, s_b), int(z), bool(relu)) != ref).sum())
            assert np.array_equal(d["add_out_%d_%d_1" % (i, int(z))], QN.relu(d["add_out_%d_%d_0" % (i, int(z))], int(z)))
    assert naive > 0   # the (a - z_a) * s_a form is NOT torch's arithmetic


def test_pool_models_equal_torch_exactly():
    d = H.fixture("q8net_ops")
    k, s, p = (int(v) for v in d["maxpool_ksp"])
    assert np.array_equal(QN.max_pool(d["maxpool_x"], k, s, p), d["maxpool_out"])
    j = 0
    while "avgpool_x_%d" % j in d:
        x, k = d["avgpool_x_%d" % j], int(d["avgpool_k_%d" % j])
        for z in d["avgpool_zero_points"]:
            assert np.array_equal(QN.avg_pool(x, int(z), k, k), d["avgpool_out_%d_%d" % (j, int(z))]), (j, int(z))
        j += 1
    assert j == 4


def test_bottleneck_fixture_stage_by_stage():
    """each stage on the reference's own recorded input: convs within 1 LSB / 0.5 %, add and ReLU exact"""
    d = H.fixture("q8net_bottleneck")
    for k in (1, 2, 3):
        c = H.sub(d, "c%d_" % k)
        r = H.model_record(c)
        assert np.array_equal(r["W"], c["ref_W"].astype(np.int32))
        H.assert_close_to_reference(r["out"], c, "bottleneck conv%d" % k)
        assert np.array_equal(QN.relu(d["relu%d_in" % k], 128 if k < 3 else int(d["add_zero_point"])), d["relu%d_out" % k])
    assert np.array_equal(d["relu1_in"], d["c1_ref_out_i"]) and np.array_equal(d["c2_x_i"], d["relu1_out"])
    c3 = H.sub(d, "c3_")
    assert d["add_out"].size == 5184 and d["add_out"].size % 64 == 0
    assert float(d["add_scale"]) == max(float(c3["s_o"]), 0.1) and int(d["add_zero_point"]) == 0
    mod = QN.add(c3["ref_out_i"], float(c3["s_o"]), int(c3["z_o"]), d["x_i"], 0.1, 128, float(d["add_scale"]), 0)
    assert np.array_equal(mod, d["add_out"]) and np.array_equal(d["relu3_in"], d["add_out"])
    assert np.array_equal(d["relu3_out"], d["out_i"])
    # the chained model's end-to-end difference is a recorded figure, not a bound
    print("chained model vs the reference block: %d of %d differ, max %d LSB" % (int(d["chained_ndiff"]), d["out_i"].size,
                                                                                 int(d["chained_maxdiff"])))
    diff = np.abs(d["chained_out_i"].astype(np.int32) - d["out_i"].astype(np.int32))
    assert int((diff != 0).sum()) == int(d["chained_ndiff"]) and int(diff.max()) == int(d["chained_maxdiff"])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_their_arguments_without_a_gpu():
    from bayesian_torch_amd import _lib, q8
    L = _lib.lib()
    assert L.btx_abi_version() == 9
    for n in ("btx_q8_add", "btx_q8_contract_res", "btx_q8_maxpool2d_cl", "btx_q8_avgpool2d_cl"):
        assert n in _lib.EXPORTS
    al = ctypes.c_void_p(64)
    ok = q8.make_add(0.1, 128, 0.07, 131, 0.1, 0, True)
    assert (ok.pre_a, ok.inv_s) == (float(np.float32(0.1) * np.float32(-128)), float(np.float32(1) / np.float32(0.1)))
    add = lambda *a: L.btx_q8_add(*a)  # noqa: E731
    assert add(None, al, al, 64, ctypes.byref(ok), None) == -1
    assert add(al, al, None, 64, ctypes.byref(ok), None) == -1
    assert add(al, al, al, 64, None, None) == -1
    assert add(al, al, al, 0, ctypes.byref(ok), None) == -2
    for bad in (_lib.Q8Add(0.0, 0.0, 0.1, 0.0, 10.0, 0, 0), _lib.Q8Add(0.1, 0.0, -0.1, 0.0, 10.0, 0, 0),
                _lib.Q8Add(0.1, 0.0, 0.1, 0.0, 0.0, 0, 0), _lib.Q8Add(0.1, 0.0, 0.1, 0.0, 10.0, 256, 0),
                _lib.Q8Add(0.1, 0.0, 0.1, 0.0, 10.0, -1, 0)):
        assert add(al, al, al, 64, ctypes.byref(bad), None) == -2
    g = _lib.Geom()
    g.NB, g.D, g.H, g.W, g.C, g.N = 2, 1, 9, 9, 32, 16
    g.KD, g.KH, g.KW = 1, 3, 3
    g.sd = g.sh = g.sw = 1
    g.ph = g.pw = 1
    g.dd = g.dh = g.dw = 1
    g.groups = 1
    cr = lambda *a: L.btx_q8_contract_res(*a)  # noqa: E731
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, None, ctypes.byref(ok), al, None) == -1
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, al, None, al, None) == -1
    assert cr(None, al, 128, al, al, al, 0.01, 128, 0, 0, al, ctypes.byref(ok), al, None) == -1
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, al, ctypes.byref(ok), None, None) == -1
    assert cr(ctypes.byref(g), al, 300, al, al, al, 0.01, 128, 0, 0, al, ctypes.byref(ok), al, None) == -2
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.0, 128, 0, 0, al, ctypes.byref(ok), al, None) == -2
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 1, al, ctypes.byref(ok), al, None) == -3   # residual with out_f32
    bad = _lib.Q8Add(0.1, 0.0, 0.1, 0.0, 10.0, 300, 0)
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, al, ctypes.byref(bad), al, None) == -2
    assert cr(ctypes.byref(g), al, 128, ctypes.c_void_p(8), al, al, 0.01, 128, 0, 0, al, ctypes.byref(ok), al, None) == -6
    g.groups = 2
    assert cr(ctypes.byref(g), al, 128, al, al, al, 0.01, 128, 0, 0, al, ctypes.byref(ok), al, None) == -3
    mp = lambda *a: L.btx_q8_maxpool2d_cl(*a)  # noqa: E731
    assert mp(None, al, 2, 9, 9, 16, 3, 2, 1, None) == -1 and mp(al, None, 2, 9, 9, 16, 3, 2, 1, None) == -1
    assert mp(al, al, 0, 9, 9, 16, 3, 2, 1, None) == -2 and mp(al, al, 2, 9, 9, 0, 3, 2, 1, None) == -2
    assert mp(al, al, 2, 9, 9, 16, 0, 2, 1, None) == -2 and mp(al, al, 2, 9, 9, 16, 3, 0, 1, None) == -2
    assert mp(al, al, 2, 9, 9, 16, 3, 2, 2, None) == -2    # 2 * pad > k: a window could hold no image element
    assert mp(al, al, 2, 2, 2, 16, 5, 1, 0, None) == -2    # the window does not fit
    ap = lambda *a: L.btx_q8_avgpool2d_cl(*a)  # noqa: E731
    assert ap(None, al, 2, 7, 7, 64, 7, 1, 0, 0, 128, None) == -1 and ap(al, None, 2, 7, 7, 64, 7, 1, 0, 0, 128, None) == -1
    assert ap(al, al, 2, 7, 7, 64, 7, 1, 1, 0, 128, None) == -3    # padding
    assert ap(al, al, 2, 7, 7, 64, 7, 1, 0, 1, 128, None) == -3    # ceil mode
    assert ap(al, al, 2, 7, 7, 64, 8, 1, 0, 0, 128, None) == -2 and ap(al, al, 2, 7, 0, 64, 7, 1, 0, 0, 128, None) == -2
    assert ap(al, al, 2, 7, 7, 64, 7, 1, 0, 0, 256, None) == -2 and ap(al, al, 2, 7, 7, 64, 7, 1, -1, 0, 128, None) == -2


# ---- to_qresnet -----------------------------------------------------------------------------------------------------------
def _resnet(name="resnet18", avg=2):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet as R
    torch.manual_seed(4)
    m = getattr(R, name)(num_classes=10).eval()
    m.avgpool = nn.AvgPool2d(avg)
    bt.dnn_to_bnn(m, PRIOR)
    return m


@pytest.mark.parametrize("name,block,convs", [("resnet18", "QBasicBlock", 2), ("resnet50", "QBottleneck", 3)])
def test_to_qresnet_structure(name, block, convs):
    from bayesian_torch_amd.models import to_qresnet, QResNet
    m = _resnet(name)
    ids = {n: l._btx_layer_id for n, l in m.named_modules() if hasattr(l, "_btx_layer_id")}
    q = to_qresnet(m)
    assert isinstance(q, QResNet)
    assert [n for n, _ in q.named_children()] == ["conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool", "fc"]
    assert type(q.conv1).__name__ == "QuantizedConv2dReparameterization" and isinstance(q.bn1, nn.Identity) and q.conv1.relu is True
    assert type(q.fc).__name__ == "QuantizedLinearReparameterization"
    assert {n: l._btx_layer_id for n, l in q.named_modules() if hasattr(l, "_btx_layer_id")} == ids   # same modules, same ids
    for lname in ("layer1", "layer2", "layer3", "layer4"):
        for b in getattr(q, lname):
            assert type(b).__name__ == block and b.fuse_add is True
            names = ["conv%d" % (i + 1) for i in range(convs)]
            for i, cn in enumerate(names):
                c = getattr(b, cn)
                assert type(c).__name__ == "QuantizedConv2dReparameterization" and isinstance(getattr(b, "bn%d" % (i + 1)), nn.Identity)
                assert c.relu is (i < convs - 1), (lname, cn)   # the last conv's ReLU comes after the add
                assert c.bias is True and c.quantized_sigma_bias is None   # the folded BatchNorm's deterministic bias
            if b.downsample is not None:
                assert type(b.downsample[0]).__name__ == "QuantizedConv2dReparameterization" and b.downsample[0].relu is False
                assert isinstance(b.downsample[1], nn.Identity)
    assert q.layer1[0].downsample is None or name == "resnet50"
    assert q.layer2[0].downsample is not None
    assert q.set_fuse_add(False) is q and not any(b.fuse_add for b in q.layer3)


def test_factories_and_the_batchnorm_refusal():
    from bayesian_torch_amd import models as M
    from bayesian_torch_amd._lib import BtxError
    for fn in ("qresnet18", "qresnet34", "qresnet50", "qresnet101"):
        assert callable(getattr(M, fn))
    q = M.qresnet18(num_classes=7)
    assert isinstance(q, M.QResNet) and isinstance(q.layer4[1], M.QBasicBlock) and q.fc.out_features == 7
    with pytest.raises(BtxError, match=r"BatchNorm2d 'bn1'"):
        M.to_qresnet(_resnet(), fuse_conv_bn=False)


# ---- CPU tensors: torch's quantized ops -----------------------------------------------------------------------------------
def test_q8_functions_on_quint8_are_the_torch_ops():
    from bayesian_torch_amd import q8
    from bayesian_torch_amd._lib import BtxError
    g = np.random.RandomState(3)
    a, b = g.randint(0, 256, (2, 16, 8, 8)).astype(np.uint8), g.randint(0, 256, (2, 16, 8, 8)).astype(np.uint8)
    qa, qb = _quint8(a, 0.1, 128), _quint8(b, 0.07, 120)
    for relu, op in ((False, torch.ops.quantized.add), (True, torch.ops.quantized.add_relu)):
        o = q8.add(qa, qb, 0.1, 0, relu)
        assert o.dtype == torch.quint8 and torch.equal(o.int_repr(), op(qa, qb, 0.1, 0).int_repr()) and o.q_scale() == 0.1
        assert np.array_equal(o.int_repr().numpy(), QN.add(a, 0.1, 128, b, 0.07, 120, 0.1, 0, relu))   # 2048 = 32 * 64 elements
    assert torch.equal(q8.max_pool2d(qa, 3, 2, 1).int_repr(), F.max_pool2d(qa, 3, 2, 1).int_repr())
    assert np.array_equal(q8.max_pool2d(qa, 3, 2, 1).int_repr().numpy(), QN.max_pool(a, 3, 2, 1))
    assert torch.equal(q8.avg_pool2d(qa, 2).int_repr(), nn.AvgPool2d(2)(qa).int_repr())
    assert np.array_equal(q8.avg_pool2d(qa, 2, 2).int_repr().numpy(), QN.avg_pool(a, 128, 2, 2))
    assert torch.equal(q8.relu(qa).int_repr(), torch.relu(qa).int_repr())
    assert np.array_equal(q8.relu(qa).int_repr().numpy(), QN.relu(a, 128))
    with pytest.raises(BtxError, match="QTensor"):
        q8.add(torch.zeros(3), torch.zeros(3), 0.1, 0)
    with pytest.raises(BtxError, match="GPU"):
        q8.max_pool2d(q8.QTensor(torch.from_numpy(a), 0.1, 128), 3, 2, 1)   # a CPU carrier has no kernels: pass quint8
    v = q8.QTensor(torch.from_numpy(a[:, :, :1, :1].copy()), 0.1, 128).view(2, -1)
    assert v.shape == (2, 16) and v.q_scale() == 0.1 and np.array_equal(v.int_repr().numpy(), a[:, :, 0, 0])
    v = q8.QTensor(torch.from_numpy(a), 0.1, 128).view(2, -1)   # a 4-D carrier is channels-last inside; view() is NCHW order
    assert np.array_equal(v.int_repr().numpy(), a.reshape(2, -1))


def _by_hand(q, x):
    """the reference's op chain written out with torch's ops, the layers called in the order QResNet.forward calls them"""
    out = torch.relu(q.conv1(x))   # conv1.relu is folded: a second ReLU changes nothing
    out = F.max_pool2d(out, 3, 2, 1)
    for layer in (q.layer1, q.layer2, q.layer3, q.layer4):
        for b in layer:
            y = b.conv1(out)
            assert torch.equal(y.int_repr(), torch.relu(y).int_repr())
            res = out if b.downsample is None else b.downsample[0](out)   # the shortcut is drawn before the last conv
            y = b.conv2(y)
            out = torch.relu(torch.ops.quantized.add(y, res, max(y.q_scale(), res.q_scale()), 0))
    out = nn.AvgPool2d(2)(out)
    return q.fc(out.view(out.size(0), -1))


def test_cpu_qresnet_forward_equals_the_torch_ops_by_hand():
    from bayesian_torch_amd.models import to_qresnet
    q = to_qresnet(_resnet())
    torch.manual_seed(9)
    x = torch.randn(1, 3, 64, 64)
    outs = {}
    for fuse in (True, False):
        q.set_fuse_add(fuse)
        torch.manual_seed(21)
        with torch.no_grad():
            outs[fuse] = q(x)
    torch.manual_seed(21)
    with torch.no_grad():
        ref = _by_hand(q, x)
    assert outs[True].dtype == torch.float32 and outs[True].shape == (1, 10) and torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], ref) and torch.equal(outs[False], ref)
    assert len(torch.unique(ref)) > 1   # the logits (steps of 0.2) are not one constant
    torch.manual_seed(22)
    with torch.no_grad():
        assert not torch.equal(q(x), ref)   # another draw of the weights
