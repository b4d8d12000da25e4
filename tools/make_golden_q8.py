#!/usr/bin/env python3
"""Generate tests/golden/q8_*.npz from the REFERENCE's INT8 layers (layers/variational_layers/quantize_linear_variational.py,
quantize_conv_variational.py, models/bnn_to_qbnn.py) on the CPU quantized engine.  Same recipe as tools/make_golden.py:
torch.manual_seed(init) -> reference layer (its own init draws); x ~ randn * 2; torch.manual_seed(fwd) -> the reference forward
(eps from the global generator, read back from the layer's eps buffers).  Runs in the build container only (/root/reference is
absent on the GPU box); the fixtures are committed and hold data only.

Before a fixture is written the numpy model tests/q8_model.py (BTX-Q8 v1) is ASSERTED against the reference:
the sampled int8 weight exactly, the output within 1 LSB in at most 0.5 % of the elements.  That cap is a condition: a case that
exceeds it gets another seed, never a wider cap.

usage: python tools/make_golden_q8.py
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bayesian_torch.layers as RL  # noqa: E402  (the reference)
from bayesian_torch.models.bnn_to_qbnn import bnn_to_qbnn  # noqa: E402
import q8_model as Q  # noqa: E402

MAX_LSB, MAX_FRAC = 1, 0.005


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _float_params(layer, wn):
    d = {"mu": _np(getattr(layer, "mu_" + wn)), "rho": _np(getattr(layer, "rho_" + wn))}
    if layer.mu_bias is not None:
        d["mu_b"], d["rho_b"] = _np(layer.mu_bias), _np(layer.rho_bias)
    return d


def _scales(qlayer, default_scale, conv):
    """the five (scale, zero point) pairs of one reference forward + the stored weight scales"""
    s_mu, s_sigma = qlayer.quantized_mu_weight.q_scale(), qlayer.quantized_sigma_weight.q_scale()
    if qlayer.quant_dict is None:
        s_eps, s_d, s_w = Q.default_scales(s_sigma, s_mu)
        sx, zx, so, zo = default_scale, 128, default_scale, 128
        zs = (0, 0, 0)
    else:
        qd = [(float(e["scale"]), int(e["zero_point"])) for e in qlayer.quant_dict]
        (s_eps, z0), (s_d, z1), (s_w, z2), (sx, zx), (so, zo) = qd
        zs = (z0, z1, z2)
    return dict(s_mu=s_mu, s_sigma=s_sigma, s_eps=s_eps, s_d=s_d, s_w=s_w, s_x=sx, z_x=zx, s_o=so, z_o=zo,
                z_eps=zs[0], z_d=zs[1], z_w=zs[2], calibrated=int(qlayer.quant_dict is not None))


def _record(name, qlayer, x, ref_out, sc, conv, geom):
    """one layer's record, checked against the numpy model"""
    rec = {k: np.float64(v) if isinstance(v, float) else np.int64(v) for k, v in sc.items()}
    mu_i, sigma_i = _np(qlayer.quantized_mu_weight.int_repr()), _np(qlayer.quantized_sigma_weight.int_repr())
    eps = _np(qlayer.eps_kernel if conv else qlayer.eps_weight)
    mu_b = _np(qlayer.quantized_mu_bias) if qlayer.bias else None
    sigma_b = _np(qlayer.quantized_sigma_bias) if (qlayer.bias and qlayer.quantized_sigma_bias is not None) else None
    eps_b = _np(qlayer.eps_bias) if sigma_b is not None else None
    assert (sc["z_eps"], sc["z_d"], sc["z_w"]) == (0, 0, 0), "the reference's qint8 observers are symmetric"
    if x.is_quantized:
        x_i, x_f = _np(x.int_repr()), _np(x.dequantize())
        s_x, z_x = x.q_scale(), x.q_zero_point()
        rec["s_x"], rec["z_x"], rec["x_is_q"] = np.float64(s_x), np.int64(z_x), np.int64(1)
    else:
        x_f = _np(x)
        s_x, z_x = sc["s_x"], sc["z_x"]
        x_i = Q.quantize_input(x_f, s_x, z_x)
        rec["x_is_q"] = np.int64(0)
        assert np.array_equal(x_i, _np(torch.quantize_per_tensor(x, s_x, z_x, torch.quint8).int_repr())), name + ": input quantize"
    r = Q.layer_forward(x_i, z_x, s_x, mu_i.astype(np.int32), sc["s_mu"], sigma_i.astype(np.int32), sc["s_sigma"], eps, mu_b, sigma_b,
                        eps_b, sc["s_eps"], sc["s_d"], sc["s_w"], sc["s_o"], sc["z_o"], **geom)
    ref_W = _np(qlayer._golden_W)
    assert np.array_equal(r["W"], ref_W.astype(np.int32)), name + ": the numpy model does not reproduce the reference's sampled weight"
    ref_o = _np(ref_out.int_repr()).astype(np.int32)
    diff = np.abs(r["out"].astype(np.int32) - ref_o)
    frac = float((diff != 0).mean())
    assert diff.max() <= MAX_LSB and frac <= MAX_FRAC, "%s: |diff| max %d, fraction %.4f%% > cap" % (name, diff.max(), 100 * frac)
    print("%-22s W exact (%d elements, %.1f%% of d_i saturated); output: %d of %d differ by 1 LSB (%.3f%%)" % (
        name, ref_W.size, 100 * float((np.abs(Q.sample_weight(mu_i.astype(np.int32), sc["s_mu"], sigma_i.astype(np.int32), sc["s_sigma"],
                                                                   eps, sc["s_eps"], sc["s_d"], sc["s_w"])[1]) >= 127).mean()),
        int((diff != 0).sum()), diff.size, 100 * frac))
    rec.update(x=x_f, x_i=x_i, mu_i=mu_i, sigma_i=sigma_i, eps=eps, ref_W=ref_W, ref_out_i=_np(ref_out.int_repr()),
               ref_out=_np(ref_out.dequantize()))
    for k, v in (("mu_b_q", mu_b), ("sigma_b_q", sigma_b), ("eps_b", eps_b)):
        if v is not None:
            rec[k] = v
    for k, v in geom.items():
        rec[k] = np.int64(v)
    return rec


def _spy_weight(qlayer):
    """record the int8 weight the reference hands to its quantized linear / conv2d"""
    import torch.nn.quantized.functional as QF
    name = "conv2d" if hasattr(qlayer, "kernel_size") else "linear"
    orig = getattr(QF, name)

    def spy(inp, weight, *a, **kw):
        qlayer._golden_W = weight.int_repr().clone()
        return orig(inp, weight, *a, **kw)
    return name, orig, spy


def _run(qlayer, x, seed):
    import torch.nn.quantized.functional as QF
    name, orig, spy = _spy_weight(qlayer)
    setattr(QF, name, spy)
    try:
        torch.manual_seed(seed)
        with torch.no_grad():
            out = qlayer(x)
    finally:
        setattr(QF, name, orig)
    return out[0] if isinstance(out, tuple) else out


def _requant(out_f, s, z):
    """the reference's Linear dequantizes its output: the uint8 values are recovered exactly from it"""
    return torch.quantize_per_tensor(out_f, s, z, torch.quint8)


class _Wrap(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.body = conv


def linear_default(name, fin, fout, batch, s_init, s_fwd):
    torch.manual_seed(s_init)
    ql = RL.QuantizedLinearReparameterization(fin, fout)
    fp = _float_params(ql, "weight")
    x = torch.randn(batch, fin) * 2
    ql.quantize()
    out = _run(ql, x, s_fwd)
    sc = _scales(ql, 0.2, False)
    rec = _record(name, ql, x, _requant(out, sc["s_o"], sc["z_o"]), sc, False, {})
    rec.update({"f_" + k: v for k, v in fp.items()}, seed_fwd=np.int64(s_fwd), kind=np.int64(0))
    return rec


def conv_default(name, cin, cout, k, hw, batch, s_init, s_fwd, stride=1, padding=1, dilation=1, fuse_bn=False):
    torch.manual_seed(s_init)
    conv = RL.Conv2dReparameterization(cin, cout, k, stride=stride, padding=padding, dilation=dilation, bias=True)
    fp = _float_params(conv, "kernel")
    x = torch.randn(batch, cin, hw, hw) * 2
    conv.prepare()
    conv.quant_prepare = False
    geom = dict(stride=stride, padding=padding, dilation=dilation)
    bn_rec = {}
    if fuse_bn:
        class Block(nn.Module):
            def __init__(self):
                super().__init__()
                self.conv1 = conv
                self.bn1 = nn.BatchNorm2d(cout)
        m = Block()
        with torch.no_grad():
            m.bn1.weight.uniform_(0.5, 1.5)
            m.bn1.bias.normal_(0, 0.3)
            m.bn1.running_mean.normal_(0, 0.3)
            m.bn1.running_var.uniform_(0.5, 2.0)
        m.eval()
        bn_rec = dict(bn_weight=_np(m.bn1.weight), bn_bias=_np(m.bn1.bias), bn_mean=_np(m.bn1.running_mean),
                      bn_var=_np(m.bn1.running_var), bn_eps=np.float64(m.bn1.eps))
        # the reference's traversal folds only a conv1 that has no child modules: park the stubs prepare() made outside _modules
        for key in ("qint_quant", "quint_quant", "dequant"):
            conv.__dict__[key] = conv._modules.pop(key)
        bnn_to_qbnn(m, fuse_conv_bn=True)
        ql = m.conv1
        assert isinstance(m.bn1, nn.Identity)
    else:
        m = _Wrap(conv)
        bnn_to_qbnn(m)
        ql = m.body
    assert type(ql).__name__ == "QuantizedConv2dReparameterization"
    out = _run(ql, x, s_fwd)
    sc = _scales(ql, 0.1, True)
    rec = _record(name, ql, x, out, sc, True, geom)
    rec.update({"f_" + k: v for k, v in fp.items()}, seed_fwd=np.int64(s_fwd), kind=np.int64(1), **bn_rec)
    return rec


class _Net(nn.Module):
    """conv -> dequantize -> flatten -> Linear: the calibrated flow's model"""

    def __init__(self):
        super().__init__()
        self.conv = RL.Conv2dReparameterization(8, 6, 3, stride=1, padding=1, bias=True)
        self.fc = RL.LinearReparameterization(6 * 5 * 5, 10)

    def forward(self, x):
        x = self.conv(x)[0]
        if x.is_quantized:
            x = x.dequantize()
        return self.fc(torch.relu(x).flatten(1))[0]


def calibrated(name, s_init, s_fwd):
    torch.manual_seed(s_init)
    m = _Net()
    fpc, fpl = _float_params(m.conv, "kernel"), _float_params(m.fc, "weight")
    batches = [torch.randn(4, 8, 5, 5) * 2 for _ in range(4)]
    x = torch.randn(4, 8, 5, 5) * 2
    m.eval()
    m.conv.prepare()
    m.fc.prepare()
    torch.quantization.prepare(m, inplace=True)
    with torch.no_grad():
        for b in batches:
            m(b)
    torch.quantization.convert(m, inplace=True)
    bnn_to_qbnn(m)
    assert len(m.conv.quant_dict) == 5 and len(m.fc.quant_dict) == 5
    import torch.nn.quantized.functional as QF
    spies = [_spy_weight(m.conv), _spy_weight(m.fc)]
    captured = {}
    for nm, orig, spy in spies:
        setattr(QF, nm, spy)
    hooks = [m.conv.register_forward_hook(lambda mod, i, o: captured.__setitem__("conv", (i[0], o[0]))),
             m.fc.register_forward_hook(lambda mod, i, o: captured.__setitem__("fc", (i[0], o[0])))]
    try:
        torch.manual_seed(s_fwd)
        with torch.no_grad():
            y = m(x)
    finally:
        for nm, orig, spy in spies:
            setattr(QF, nm, orig)
        for h in hooks:
            h.remove()
    out = {}
    scc, scl = _scales(m.conv, 0.1, True), _scales(m.fc, 0.2, False)
    rc = _record(name + "/conv", m.conv, captured["conv"][0], captured["conv"][1], scc, True, dict(stride=1, padding=1, dilation=1))
    rl = _record(name + "/fc", m.fc, captured["fc"][0], _requant(captured["fc"][1], scl["s_o"], scl["z_o"]), scl, False, {})
    rc.update({"f_" + k: v for k, v in fpc.items()})
    rl.update({"f_" + k: v for k, v in fpl.items()})
    out.update({"conv_" + k: v for k, v in rc.items()})
    out.update({"fc_" + k: v for k, v in rl.items()})
    out["calib"] = np.stack([_np(b) for b in batches])
    out["x"], out["y"], out["seed_fwd"], out["kind"] = _np(x), _np(y), np.int64(s_fwd), np.int64(2)
    return out


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    cases = {
        "q8_linear_default": lambda: linear_default("linear_default", 96, 24, 8, 101, 202),
        "q8_conv_default": lambda: conv_default("conv_default", 32, 16, 3, 9, 2, 303, 404),
        "q8_conv_stem_default": lambda: conv_default("conv_stem_default", 3, 16, 3, 9, 2, 505, 606),
        "q8_conv_fused_bn": lambda: conv_default("conv_fused_bn", 32, 16, 3, 9, 2, 707, 808, fuse_bn=True),
        "q8_calibrated": lambda: calibrated("calibrated", 909, 1010),
    }
    total = 0
    for fname, fn in cases.items():
        rec = fn()
        path = os.path.join(gold, fname + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
        print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")
    print("total", total, "bytes; engine", torch.backends.quantized.engine)


if __name__ == "__main__":
    main()
