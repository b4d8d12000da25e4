#!/usr/bin/env python3
"""Generate tests/golden/q8net_*.npz: what the ops BETWEEN the INT8 layers compute in the reference's QResNet
(models/bayesian/quantized_resnet_variational_large.py) on the CPU quantized engine.  Runs in the build container only (it
imports the reference, like tools/make_golden_q8.py); the fixtures are committed and hold data only.

  q8net_ops.npz         inputs and outputs of torch's own quantized ops: quantized.add / add_relu, F.max_pool2d and AvgPool2d on
                        quint8.  Element counts are multiples of 64 only: torch's add runs a vector body over blocks of 64 and a
                        scalar remainder loop that breaks ties differently from its own vector body, so this
                        keeps the fixture independent of the CPU that wrote it.
  q8net_bottleneck.npz  one reference Bottleneck (inplanes 32, planes 8, stride 1, no downsample, BatchNorms replaced by
                        Identity, default scales) on a quint8 2x32x9x9 input: the float parameters, each conv's eps and sampled
                        weight, every intermediate quantized tensor and the block output.

Before a fixture is written the numpy models (tests/q8_model.py, tests/q8_net_model.py) are ASSERTED against it: the ops
exactly; the block stage by stage, every stage fed the reference's own recorded input — convs within the cap of
make_golden_q8.py (<= 1 LSB in <= 0.5 % of the elements), add and ReLU exactly.  The end-to-end difference of the chained model
is recorded and printed, not bounded: a 1-LSB difference at conv1 propagates.

usage: python tools/make_golden_q8net.py
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_q8 as G  # noqa: E402  (puts the reference and tests/ on the path)
import q8_model as Q  # noqa: E402
import q8_net_model as QN  # noqa: E402
from bayesian_torch.models.bayesian import quantized_resnet_variational_large as RM  # noqa: E402

SCALE_PAIRS = [(0.1, 0.07), (0.2, 0.1), (0.1, 0.1), (0.1, 0.05), (0.0371, 0.0913)]
OUT_ZERO_POINTS = [0, 128, 120]
_np = G._np


def _quint8(q, s, z):
    return torch._make_per_tensor_quantized_tensor(torch.from_numpy(q), s, z)


def ops_fixture():
    rng = np.random.RandomState(20240)
    rec = {}
    # ---- add / add_relu: (1, 64, 7, 7) = 3136 = 49 * 64 elements, full-range bytes, input zero points 128 / 131
    a = rng.randint(0, 256, size=(1, 64, 7, 7)).astype(np.uint8)
    b = rng.randint(0, 256, size=(1, 64, 7, 7)).astype(np.uint8)
    assert a.size % 64 == 0
    z_a, z_b = 128, 131
    rec.update(add_a=a, add_b=b, add_z_a=np.int64(z_a), add_z_b=np.int64(z_b), add_pairs=np.array(SCALE_PAIRS, dtype=np.float64),
               add_zero_points=np.array(OUT_ZERO_POINTS, dtype=np.int64))
    naive = 0
    for i, (s_a, s_b) in enumerate(SCALE_PAIRS):
        s = max(s_a, s_b)   # the reference's rule
        for z in OUT_ZERO_POINTS:
            qa, qb = _quint8(a, s_a, z_a), _quint8(b, s_b, z_b)
            for relu, op in ((False, torch.ops.quantized.add), (True, torch.ops.quantized.add_relu)):
                ref = _np(op(qa, qb, s, z).int_repr())
                mod = QN.add(a, s_a, z_a, b, s_b, z_b, s, z, relu)
                nd = int((mod != ref).sum())
                assert nd == 0, "add pair %d z %d relu %d: %d elements differ from torch" % (i, z, relu, nd)
                naive += int((QN.add_naive(a, s_a, z_a, b, s_b, z_b, s, z, relu) != ref).sum())
                rec["add_out_%d_%d_%d" % (i, z, int(relu))] = ref
            assert np.array_equal(rec["add_out_%d_%d_1" % (i, z)], np.maximum(rec["add_out_%d_%d_0" % (i, z)], z))
    print("add: 0 of %d elements differ from torch on %d tensors (the naive (a - z) * s model: %d)" % (a.size, 30, naive))
    # ---- max-pool 3 / 2 / 1 on 9 x 9: (2, 32, 9, 9) = 5184 = 81 * 64
    x = rng.randint(0, 256, size=(2, 32, 9, 9)).astype(np.uint8)
    x[0, 0, 0, 0], x[0, 1, 4, 4] = 0, 255
    ref = _np(F.max_pool2d(_quint8(x, 0.1, 77), 3, 2, 1).int_repr())
    assert np.array_equal(QN.max_pool(x, 3, 2, 1), ref), "max-pool"
    rec.update(maxpool_x=x, maxpool_out=ref, maxpool_ksp=np.array([3, 2, 1], dtype=np.int64))
    print("max-pool 3/2/1 on %s: exact" % (x.shape,))
    # ---- avg-pool: AvgPool2d(7) on 7 x 7 and AvgPool2d(2) on 8 x 8
    cases = [(4, 16, 7, 7), (64, 37, 7, 7), (4, 64, 7, 7), (1, 24, 8, 8)]   # C = 37: 64 images make the count a multiple of 64
    rec["avgpool_zero_points"] = np.array([0, 77, 128], dtype=np.int64)
    for j, (bb, c, h, k) in enumerate(cases):
        x = rng.randint(0, 256, size=(bb, c, h, h)).astype(np.uint8)
        assert x.size % 64 == 0
        rec["avgpool_x_%d" % j], rec["avgpool_k_%d" % j] = x, np.int64(k)
        for z in (0, 77, 128):
            ref = _np(nn.AvgPool2d(k)(_quint8(x, 0.1, z)).int_repr())
            assert np.array_equal(QN.avg_pool(x, z, k, k), ref), "avg-pool case %d z %d" % (j, z)
            rec["avgpool_out_%d_%d" % (j, z)] = ref
    print("avg-pool: exact on %d cases x 3 zero points" % len(cases))
    return rec


def bottleneck_fixture(s_init, s_fwd):
    import torch.nn.quantized.functional as QF
    torch.manual_seed(s_init)
    blk = RM.Bottleneck(32, 8, stride=1, downsample=None, bias=False)
    convs = [blk.conv1, blk.conv2, blk.conv3]
    fps = [G._float_params(c, "kernel") for c in convs]
    x = torch.randn(2, 32, 9, 9) * 2
    for c in convs:
        if not hasattr(c, "qint_quant"):   # quantize() deletes the stubs prepare() makes
            c.prepare()
            c.quant_prepare = False
        c.quantize()
        c.quantized_sigma_bias = None
        c.dnn_to_bnn_flag = True
    blk.bn1, blk.bn2, blk.bn3 = nn.Identity(), nn.Identity(), nn.Identity()
    blk.eval()
    xq = torch.quantize_per_tensor(x, 0.1, 128, torch.quint8)
    assert np.array_equal(_np(xq.int_repr()), Q.quantize_input(_np(x), 0.1, 128)), "input quantize"

    weights, conv_io, relu_in, relu_out = [], {}, [], []
    orig = QF.conv2d

    def spy(inp, weight, *a, **kw):
        weights.append(weight.int_repr().clone())
        return orig(inp, weight, *a, **kw)
    hooks = [c.register_forward_hook(lambda mod, i, o, k=k: conv_io.__setitem__(k, (i[0].clone(), o.clone()))) for k, c in enumerate(convs)]
    hooks.append(blk.relu.register_forward_pre_hook(lambda mod, i: relu_in.append(i[0].clone())))   # the ReLU is in place
    hooks.append(blk.relu.register_forward_hook(lambda mod, i, o: relu_out.append(o.clone())))
    QF.conv2d = spy
    try:
        torch.manual_seed(s_fwd)
        with torch.no_grad():
            out = blk(xq)
    finally:
        QF.conv2d = orig
        for h in hooks:
            h.remove()
    assert len(weights) == 3 and len(relu_in) == 3
    geoms = [dict(stride=1, padding=0, dilation=1), dict(stride=1, padding=1, dilation=1), dict(stride=1, padding=0, dilation=1)]
    rec = dict(x=_np(x), x_i=_np(xq.int_repr()), seed_fwd=np.int64(s_fwd))
    chained = _np(xq.int_repr())
    for k, c in enumerate(convs):
        c._golden_W = weights[k]
        r = G._record("bottleneck/conv%d" % (k + 1), c, conv_io[k][0], conv_io[k][1], G._scales(c, 0.1, True), True, geoms[k])
        r.update({"f_" + n: v for n, v in fps[k].items()})
        rec.update({"c%d_%s" % (k + 1, n): v for n, v in r.items()})
        # the chained model: each conv on the MODEL's previous output
        d = dict(r, x_i=chained)
        m = Q.layer_forward(d["x_i"], int(d["z_x"]), float(d["s_x"]), d["mu_i"].astype(np.int32), float(d["s_mu"]),
                            d["sigma_i"].astype(np.int32), float(d["s_sigma"]), d["eps"], None, None, None, float(d["s_eps"]),
                            float(d["s_d"]), float(d["s_w"]), float(d["s_o"]), int(d["z_o"]), **geoms[k])["out"]
        chained = QN.relu(m, 128) if k < 2 else m
    # ReLU stages: exact on the reference's own inputs
    for k in range(3):
        zi = relu_in[k].q_zero_point()
        assert np.array_equal(QN.relu(_np(relu_in[k].int_repr()), zi), _np(relu_out[k].int_repr())), "relu %d" % k
        rec["relu%d_in" % (k + 1)], rec["relu%d_out" % (k + 1)] = _np(relu_in[k].int_repr()), _np(relu_out[k].int_repr())
    assert np.array_equal(_np(relu_in[0].int_repr()), _np(conv_io[0][1].int_repr()))
    assert np.array_equal(_np(conv_io[1][0].int_repr()), _np(relu_out[0].int_repr()))
    assert np.array_equal(_np(conv_io[2][0].int_repr()), _np(relu_out[1].int_repr()))
    # the add: exact on the reference's conv3 output and the block input; 2 * 32 * 81 = 5184 = 81 * 64 elements
    c3 = conv_io[2][1]
    add_ref = relu_in[2]
    s_add, z_add = add_ref.q_scale(), add_ref.q_zero_point()
    assert s_add == max(c3.q_scale(), xq.q_scale()) and z_add == 0 and add_ref.numel() % 64 == 0
    mod = QN.add(_np(c3.int_repr()), c3.q_scale(), c3.q_zero_point(), _np(xq.int_repr()), xq.q_scale(), xq.q_zero_point(), s_add, z_add)
    assert np.array_equal(mod, _np(add_ref.int_repr())), "add: %d differ" % int((mod != _np(add_ref.int_repr())).sum())
    assert np.array_equal(_np(out.int_repr()), _np(relu_out[2].int_repr()))
    rec.update(add_out=_np(add_ref.int_repr()), add_scale=np.float64(s_add), add_zero_point=np.int64(z_add), out_i=_np(out.int_repr()))
    # end to end: the chained model against the reference's block output — recorded, not bounded
    end = QN.add(chained, c3.q_scale(), c3.q_zero_point(), _np(xq.int_repr()), xq.q_scale(), xq.q_zero_point(), s_add, z_add, relu=True)
    diff = np.abs(end.astype(np.int32) - _np(out.int_repr()).astype(np.int32))
    rec.update(chained_out_i=end, chained_ndiff=np.int64((diff != 0).sum()), chained_maxdiff=np.int64(diff.max()))
    print("bottleneck: add and ReLUs exact; chained model vs the block output: %d of %d elements differ, max |diff| %d LSB"
          % (int((diff != 0).sum()), diff.size, int(diff.max())))
    return rec


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    total = 0
    for fname, fn in (("q8net_ops", ops_fixture), ("q8net_bottleneck", lambda: bottleneck_fixture(1111, 1212))):
        rec = fn()
        path = os.path.join(gold, fname + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
        print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")
    print("total", total, "bytes; engine", torch.backends.quantized.engine)


if __name__ == "__main__":
    main()
