#!/usr/bin/env python3
"""Generate tests/golden/q8f_*.npz from the REFERENCE's INT8 Flipout layers (layers/flipout_layers/quantized_conv_flipout.py,
quantized_linear_flipout.py, models/bnn_to_qbnn.py) on the CPU quantized engine.  Runs in the build container only (the reference
is absent on the GPU box); the fixtures are committed and hold data only.

Per case eps and the signs are explicit.  Two evaluations are made and asserted EQUAL, bit for bit, before anything is written:
  (i)  the reference's own QuantizedConv2dFlipout.forward.  Default path: torch is re-seeded and the forward's draws (sign_input,
       sign_output, eps_kernel, eps_bias, in that order) are replayed here.  Calibrated path: the reference builds its presampled
       sign pools with torch.randint(0, 1, ..) (every sign -1) but only when they are None, so the pools are preset to chosen +-1
       values and `random` is re-seeded to replay the two window offsets.
  (ii) the same torch ops in the reference's order, called from here, recording every intermediate (d_i, x', o1, p, p2, out).
The reference's QuantizedLinearFlipout can raise in dequantize() when the layer has a bias (and its quantize() needs rho_bias, so
no bias-free layer can be built): the Linear cases try (i) and fall back to (ii) alone; each file's `meta` says which was used.

Then the numpy model tests/q8_flipout_model.py is ASSERTED against the reference (the conditions of tests/test_q8_flipout_cpu.py):
d_i, x', the sign bytes and the bias vectors exactly; o1 and p within 1 LSB in at most 0.5 % of their elements (v1's cap, a
condition: a case that exceeds it gets another seed, never a wider cap); p2 and out from the reference's own o1 and p exactly;
end to end every differing element lies where o1 or p differs.

usage: python tools/make_golden_q8_flipout.py
"""
import json
import os
import random
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
import torch.nn.quantized.functional as QF  # noqa: E402
import q8_model as Q  # noqa: E402
import q8_flipout_model as QF8  # noqa: E402

MAX_LSB, MAX_FRAC = 1, 0.005
KINDS = ("none", "mu", "sigma_eps")


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _entries(ql, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128):
    if ql.quant_dict is None:
        return QF8.default_entries(ql.quantized_sigma_weight.q_scale(), normal_scale, default_scale, default_zero_point), False
    return [(float(e["scale"]), int(e["zero_point"])) for e in ql.quant_dict], True


def chain(q_mu, q_sigma, xq, eps, sign_in, sign_out, b_mean, b_pert, e, conv, geom, relu):
    """(ii): the reference's op order on explicit noise -> dict of torch tensors"""
    eps_q = torch.quantize_per_tensor(eps, e[0][0], e[0][1], torch.qint8)
    delta = torch.ops.quantized.mul(q_sigma, eps_q, e[1][0], e[1][1])
    fn = QF.conv2d if conv else QF.linear
    o1 = fn(xq, q_mu, b_mean, *geom, scale=e[3][0], zero_point=e[3][1])
    s_in = torch.quantize_per_tensor(sign_in, e[4][0], e[4][1], torch.quint8)
    s_out = torch.quantize_per_tensor(sign_out, e[5][0], e[5][1], torch.quint8)
    xp = torch.ops.quantized.mul(xq, s_in, e[6][0], e[6][1])
    p = fn(xp, delta, b_pert, *geom, scale=e[7][0], zero_point=e[7][1])
    p2 = torch.ops.quantized.mul(p, s_out, e[8][0], e[8][1])
    out = torch.ops.quantized.add(o1, p2, e[9][0], e[9][1])
    if relu:
        out = torch.relu(out)
    return dict(eps_q=eps_q, d_i=delta, o1=o1, xp=xp, p=p, p2=p2, out=out, s_in=s_in, s_out=s_out)


def run_reference(ql, x, calibrated, s_fwd, sign_in=None, sign_out=None, fn="conv2d"):
    """(i): the reference forward with its conv / linear calls spied -> (out, calls, noise)"""
    calls = []
    orig = getattr(QF, fn)
    wn = "kernel" if fn == "conv2d" else "weight"

    def spy(inp, weight, bias, *a, **kw):
        o = orig(inp, weight, bias, *a, **kw)
        calls.append((inp, weight, bias, o))
        return o
    setattr(QF, fn, spy)
    try:
        if calibrated:
            n_in, n_out = sign_in.numel(), sign_out.numel()
            ql.presampled_input_perturb = torch.cat([sign_in.flatten(), sign_in.flatten()]).float()
            ql.presampled_output_perturb = torch.cat([sign_out.flatten(), sign_out.flatten()]).float()
            random.seed(s_fwd)
        torch.manual_seed(s_fwd)
        with torch.no_grad():
            out = ql(x)[0]
    finally:
        setattr(QF, fn, orig)
    eps_buf = getattr(ql, "eps_" + wn)
    if calibrated:  # replay the two window offsets
        random.seed(s_fwd)
        st_i = random.randint(0, n_in)
        st_o = random.randint(0, n_out)
        sign_in = ql.presampled_input_perturb[st_i:st_i + n_in].reshape(sign_in.shape)
        sign_out = ql.presampled_output_perturb[st_o:st_o + n_out].reshape(sign_out.shape)
        eps_b = ql.eps_bias.clone() if fn == "linear" else None   # the calibrated Linear path draws eps_bias, the Conv2d path does not
    else:           # replay the forward's draws
        torch.manual_seed(s_fwd)
        sign_in = torch.zeros(calls[0][0].shape).uniform_(-1, 1).sign()
        sign_out = torch.zeros(calls[0][3].shape).uniform_(-1, 1).sign()
        eps = torch.zeros(eps_buf.shape).normal_()
        assert torch.equal(eps, eps_buf)
        eps_b = ql.eps_bias.clone() if getattr(ql, "bias", True) and ql.quantized_sigma_bias is not None else None
    return out, calls, dict(eps=eps_buf.clone(), eps_b=eps_b, sign_in=sign_in, sign_out=sign_out)


def check_and_record(name, meta, x, xq, e, cal, q_mu, q_sigma, mu_b, sigma_b, kinds, noise, ii, conv, geomd, relu, extra):
    """assert the numpy model against the reference's tensors `ii`, then build the record"""
    mu_i, sigma_i = _np(q_mu.int_repr()).astype(np.int32), _np(q_sigma.int_repr()).astype(np.int32)
    s_mu, s_sigma = q_mu.q_scale(), q_sigma.q_scale()
    e_x = (xq.q_scale(), xq.q_zero_point())
    eps, eps_b = _np(noise["eps"]), _np(noise["eps_b"])
    sign_in, sign_out = _np(noise["sign_in"]).astype(np.int8), _np(noise["sign_out"]).astype(np.int8)
    bv = [QF8.bias_vec(_np(mu_b), _np(sigma_b), eps_b, k) for k in kinds]
    m = QF8.layer_forward(_np(xq.int_repr()), e_x, mu_i, s_mu, sigma_i, s_sigma, eps, bv[0], bv[1], sign_in, sign_out, e,
                          relu=relu, **geomd)
    ref = {k: _np(ii[k].int_repr()) for k in ("d_i", "xp", "o1", "p", "p2", "out")}
    assert np.array_equal(m["d_i"], ref["d_i"]), name + ": d_i"
    assert np.array_equal(m["xp"], ref["xp"]), name + ": x'"
    for which, ent in (("s_in", e[4]), ("s_out", e[5])):
        got = set(np.unique(_np(ii[which].int_repr())).tolist())
        assert got <= set(QF8.sign_bytes(ent)), (name, which, got, QF8.sign_bytes(ent))
    for b, rb in zip(bv, ii["biases"]):
        assert (b is None and rb is None) or np.array_equal(b, _np(rb)), name + ": bias vector"
    share = {}
    for k in ("o1", "p"):
        d = np.abs(m[k].astype(np.int32) - ref[k].astype(np.int32))
        share[k] = float((d != 0).mean())
        assert d.max() <= MAX_LSB and share[k] <= MAX_FRAC, (name, k, int(d.max()), share[k])
    p2, out = QF8.tail(ref["o1"], ref["p"], sign_out, e, relu)
    assert np.array_equal(p2, ref["p2"]) and np.array_equal(out, ref["out"]), name + ": tail on the reference's o1, p"
    dd = np.abs(m["out"].astype(np.int32) - ref["out"].astype(np.int32))
    inner = (m["o1"] != ref["o1"]) | (m["p"] != ref["p"])
    assert not np.any((dd != 0) & ~inner), name + ": an end-to-end difference away from an o1 / p difference"
    meta = dict(meta, case=name, o1_share=share["o1"], p_share=share["p"], out_max_lsb=int(dd.max()), out_share=float((dd != 0).mean()),
                engine=torch.backends.quantized.engine, torch=torch.__version__)
    print(name, json.dumps(meta))
    rec = dict(x=_np(x), x_i=_np(xq.int_repr()), e_x=np.array(e_x, dtype=np.float64), e=np.array(e, dtype=np.float64),
               calibrated=np.int64(cal), mu_i=mu_i.astype(np.int8), sigma_i=sigma_i.astype(np.int8), s_mu=np.float64(s_mu),
               s_sigma=np.float64(s_sigma), eps=eps, sign_in=sign_in, sign_out=sign_out,
               kinds=np.array([KINDS.index(k) for k in kinds], dtype=np.int64), bm_i=m["bm_i"], bp_i=m["bp_i"],
               relu=np.int64(relu), kind=np.int64(1 if conv else 0), meta=np.array(json.dumps(meta)),
               **{"ref_" + k: v for k, v in ref.items()})
    if eps_b is not None:
        rec["eps_b"] = eps_b
    if mu_b is not None:
        rec["mu_b_q"] = _np(mu_b)
    if sigma_b is not None:
        rec["sigma_b_q"] = _np(sigma_b)
    rec.update({k: np.int64(v) for k, v in geomd.items()})
    rec.update(extra)
    return rec


def _float_params(layer, wn):
    d = {"f_mu": _np(getattr(layer, "mu_" + wn)), "f_rho": _np(getattr(layer, "rho_" + wn))}
    if layer.mu_bias is not None:
        d["f_mu_b"], d["f_rho_b"] = _np(layer.mu_bias), _np(layer.rho_bias)
    return d


class _Net(nn.Module):
    def __init__(self, layer):
        super().__init__()
        self.conv1 = layer

    def forward(self, x):
        return self.conv1(x)[0]


def _calibrate(m, layer, batches):
    m.eval()
    layer.prepare()
    torch.quantization.prepare(m, inplace=True)
    with torch.no_grad():
        for b in batches:
            m(b)
    torch.quantization.convert(m, inplace=True)


def _pm1(shape, gen):
    return (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)


def conv_case(name, cin, cout, k, hw, batch, s_init, s_fwd, stride=1, padding=1, dilation=1, calibrated=False, fuse_bn=False,
              relu=False, x_scale=2.0):
    torch.manual_seed(s_init)
    conv = RL.Conv2dFlipout(cin, cout, k, stride=stride, padding=padding, dilation=dilation, bias=True)
    fp = _float_params(conv, "kernel")
    x = torch.randn(batch, cin, hw, hw) * x_scale
    geomd = dict(stride=stride, padding=padding, dilation=dilation)
    extra = dict(fp)
    m = _Net(conv)
    if fuse_bn:
        m.bn1 = nn.BatchNorm2d(cout)
        with torch.no_grad():
            m.bn1.weight.uniform_(0.5, 1.5)
            m.bn1.bias.normal_(0, 0.3)
            m.bn1.running_mean.normal_(0, 0.3)
            m.bn1.running_var.uniform_(0.5, 2.0)
        extra.update(bn_weight=_np(m.bn1.weight), bn_bias=_np(m.bn1.bias), bn_mean=_np(m.bn1.running_mean),
                     bn_var=_np(m.bn1.running_var), bn_eps=np.float64(m.bn1.eps))
    m.eval()
    if calibrated:
        batches = [torch.randn(batch, cin, hw, hw) * x_scale for _ in range(4)]
        _calibrate(m, conv, batches)
        extra["calib"] = np.stack([_np(b) for b in batches])
    bnn_to_qbnn(m, fuse_conv_bn=fuse_bn)
    ql = m.conv1
    assert type(ql).__name__ == "QuantizedConv2dFlipout", type(ql).__name__
    e, cal = _entries(ql)
    assert cal == calibrated and len(e) == 10
    gen = torch.Generator().manual_seed(s_fwd + 1)
    with torch.no_grad():
        oshape = torch.nn.functional.conv2d(x, torch.zeros(cout, cin, k, k), None, stride, padding, dilation).shape
    si, so = (_pm1(tuple(x.shape), gen), _pm1(tuple(oshape), gen)) if calibrated else (None, None)
    out, calls, noise = run_reference(ql, x, calibrated, s_fwd, si, so)
    assert len(calls) == 2
    xq = calls[0][0]
    q_mu, q_sigma = ql.quantized_mu_weight, ql.quantized_sigma_weight
    mu_b = ql.quantized_mu_bias if ql.bias else None
    sigma_b = ql.quantized_sigma_bias if ql.bias else None
    kinds = ("mu", "mu") if calibrated else ("mu", "sigma_eps")
    if noise["eps_b"] is None and not calibrated:
        kinds = ("mu", "none")
    b_mean, b_pert = calls[0][2], calls[1][2]
    geom = (stride, padding, dilation, 1)
    ii = chain(q_mu, q_sigma, xq, noise["eps"], noise["sign_in"], noise["sign_out"], b_mean, b_pert, e, True, geom, relu)
    if relu:
        out = torch.relu(out)
    for k_, t in (("out", out), ("o1", calls[0][3]), ("p", calls[1][3]), ("xp", calls[1][0]), ("d_i", calls[1][1])):
        assert torch.equal(ii[k_].int_repr(), t.int_repr()), (name, "reference forward != op chain", k_)
    ii["biases"] = (b_mean, b_pert)
    meta = dict(source="reference forward == op chain (bit for bit)")
    return check_and_record(name, meta, x, xq, e, cal, q_mu, q_sigma, mu_b, sigma_b, kinds, noise, ii, True, geomd, relu, extra)


def linear_case(name, fin, fout, batch, s_init, s_fwd, calibrated=False):
    torch.manual_seed(s_init)
    lin = RL.LinearFlipout(fin, fout)
    fp = _float_params(lin, "weight")
    x = torch.randn(batch, fin) * 2
    m = _Net(lin)
    extra = dict(fp)
    if calibrated:
        batches = [torch.randn(batch, fin) * 2 for _ in range(4)]
        _calibrate(m, lin, batches)
        extra["calib"] = np.stack([_np(b) for b in batches])
    bnn_to_qbnn(m)
    ql = m.conv1
    assert type(ql).__name__ == "QuantizedLinearFlipout", type(ql).__name__
    e, cal = _entries(ql)
    assert cal == calibrated and len(e) == 10
    xq = torch.quantize_per_tensor(x, e[2][0], e[2][1], torch.quint8)
    gen = torch.Generator().manual_seed(s_fwd + 1)
    q_mu, q_sigma = ql.quantized_mu_weight, ql.quantized_sigma_weight
    mu_b = ql.quantized_mu_bias.detach().clone()
    sigma_b = ql.quantized_sigma_bias.detach().clone()
    kinds = ("sigma_eps", "sigma_eps") if calibrated else ("mu", "sigma_eps")
    ref = None
    try:  # (i), where the reference's forward runs on this torch (quirk c: it may raise in dequantize())
        si, so = (_pm1((batch, fin), gen), _pm1((batch, fout), gen)) if calibrated else (None, None)
        out, calls, noise = run_reference(ql, xq, calibrated, s_fwd, si, so, fn="linear")
        assert len(calls) == 2
        ref = (torch.quantize_per_tensor(out, e[9][0], e[9][1], torch.quint8), calls)
        attempt = "ran"
    except Exception as ex:
        attempt = "raised " + type(ex).__name__ + ": " + str(ex).splitlines()[0][:80]
        gen = torch.Generator().manual_seed(s_fwd)
        noise = dict(eps=torch.randn(fout, fin, generator=gen), eps_b=torch.randn(fout, generator=gen),
                     sign_in=_pm1((batch, fin), gen), sign_out=_pm1((batch, fout), gen))
    rnd = sigma_b * noise["eps_b"]
    b_mean = rnd if calibrated else mu_b
    ii = chain(q_mu, q_sigma, xq, noise["eps"], noise["sign_in"], noise["sign_out"], b_mean, rnd, e, False, (), False)
    ii["biases"] = (b_mean, rnd)
    if ref is not None:
        out_q, calls = ref
        for k_, t in (("out", out_q), ("o1", calls[0][3]), ("p", calls[1][3]), ("xp", calls[1][0]), ("d_i", calls[1][1])):
            assert torch.equal(ii[k_].int_repr(), t.int_repr()), (name, "reference forward != op chain", k_)
        for b, rb in zip(ii["biases"], (calls[0][2], calls[1][2])):
            assert torch.equal(b, rb), (name, "bias vector handed to the reference's linear")
        meta = dict(source="reference forward == op chain (bit for bit)", reference_attempt=attempt)
        return check_and_record(name, meta, x, xq, e, cal, q_mu, q_sigma, mu_b, sigma_b, kinds, noise, ii, False, {}, False, extra)
    meta = dict(source="op chain alone (the reference's QuantizedLinearFlipout did not run)", reference_attempt=attempt)
    return check_and_record(name, meta, x, xq, e, cal, q_mu, q_sigma, mu_b, sigma_b, kinds, noise, ii, False, {}, False, extra)


def pin_mul():
    """pin the multiplier spelling of quantized.mul against torch: 200 random (scale, zero point) sets, 0 mismatches required"""
    g = np.random.default_rng(7)
    bad = tot = 0
    for _ in range(200):
        sa, sb, so = (float(v) for v in g.uniform(0.002, 0.2, 3))
        za, zb, zo = (int(v) for v in g.integers(0, 256, 3))
        a = g.integers(0, 256, 360).astype(np.uint8)
        b = g.integers(0, 256, 360).astype(np.uint8)
        ta = torch._make_per_tensor_quantized_tensor(torch.from_numpy(a), sa, za)
        tb = torch._make_per_tensor_quantized_tensor(torch.from_numpy(b), sb, zb)
        ref = torch.ops.quantized.mul(ta, tb, so, zo).int_repr().numpy()
        got = QF8.qmul(a, za, b, zb, QF8.mul_multiplier(sa, sb, so), zo, 0, 255)
        bad += int((ref != got).sum())
        tot += a.size
    print("quantized.mul model vs torch: %d mismatches in %d elements" % (bad, tot))
    assert bad == 0


def main():
    pin_mul()
    gold = os.path.join(ROOT, "tests", "golden")
    cases = {
        "q8f_conv_default": lambda: conv_case("conv_default", 32, 16, 3, 9, 2, 1303, 1404),
        "q8f_conv_calibrated": lambda: conv_case("conv_calibrated", 8, 6, 3, 7, 4, 1505, 1606, calibrated=True),
        "q8f_conv_fused_bn_relu": lambda: conv_case("conv_fused_bn_relu", 32, 16, 3, 9, 2, 1707, 1808, fuse_bn=True, relu=True),
        "q8f_conv_stem": lambda: conv_case("conv_stem", 3, 8, 7, 20, 1, 1909, 2010, stride=2, padding=3),
        "q8f_linear_default": lambda: linear_case("linear_default", 96, 24, 8, 2101, 2202),
        "q8f_linear_calibrated": lambda: linear_case("linear_calibrated", 96, 24, 16, 2303, 2404, calibrated=True),
    }
    total = 0
    for fname, fn in cases.items():
        rec = fn()
        path = os.path.join(gold, fname + ".npz")
        np.savez_compressed(path, **rec)
        total += os.path.getsize(path)
        print("wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
