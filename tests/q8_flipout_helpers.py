"""Shared by tests/test_q8_flipout_cpu.py and tests/test_gpu_q8_flipout.py: the INT8 Flipout fixtures (tests/golden/q8f_*.npz,
written by tools/make_golden_q8_flipout.py from the reference), builders of float Flipout layers / their quantized twins from them,
and random cases for the kernels with the numpy model's answer (q8_flipout_model)."""
import os

import numpy as np
import torch

import q8_model as Q
import q8_flipout_model as QF
from q8_helpers import Block, bn_of, geom, MAX_LSB, MAX_FRAC  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ("q8f_conv_default", "q8f_conv_calibrated", "q8f_conv_fused_bn_relu", "q8f_conv_stem", "q8f_linear_default",
         "q8f_linear_calibrated")
KINDS = ("none", "mu", "sigma_eps")
# the zero points of a really calibrated layer (the ten entries the reference's prepare -> calibrate -> convert flow gave)
CAL_ZP = (0, 0, 126, 116, 127, 127, 129, 141, 114, 129)

_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        z = np.load(os.path.join(HERE, "golden", name + ".npz"))
        _CACHE[name] = {k: z[k] for k in z.files}
    return _CACHE[name]


def entries(d):
    return [(float(s), int(z)) for s, z in d["e"]]


def e_x(d):
    return float(d["e_x"][0]), int(d["e_x"][1])


def bias_vectors(d):
    kinds = [KINDS[int(k)] for k in d["kinds"]]
    return [QF.bias_vec(d.get("mu_b_q"), d.get("sigma_b_q"), d.get("eps_b"), k) for k in kinds]


def model_record(d):
    """q8_flipout_model on one fixture record (cached: the tests share it and leave it unchanged)"""
    key = ("model", id(d))
    if key not in _CACHE:
        bm, bp = bias_vectors(d)
        _CACHE[key] = QF.layer_forward(d["x_i"], e_x(d), d["mu_i"].astype(np.int32), float(d["s_mu"]), d["sigma_i"].astype(np.int32),
                                       float(d["s_sigma"]), d["eps"], bm, bp, d["sign_in"], d["sign_out"], entries(d),
                                       relu=bool(d["relu"]), **geom(d))
    return _CACHE[key]


def noise_of(d):
    nz = dict(eps_w=torch.from_numpy(d["eps"]), sign_in=torch.from_numpy(d["sign_in"]), sign_out=torch.from_numpy(d["sign_out"]))
    if "eps_b" in d:
        nz["eps_b"] = torch.from_numpy(d["eps_b"])
    return nz


def float_layer(d, device="cpu"):
    """the float Flipout layer holding a record's parameters"""
    from bayesian_torch_amd import layers as L
    mu = torch.from_numpy(d["f_mu"])
    if int(d["kind"]) == 1:
        layer = L.Conv2dFlipout(mu.shape[1], mu.shape[0], mu.shape[2], bias="f_mu_b" in d, **geom(d))
        wn = "kernel"
    else:
        layer = L.LinearFlipout(mu.shape[1], mu.shape[0], bias="f_mu_b" in d)
        wn = "weight"
    with torch.no_grad():
        getattr(layer, "mu_" + wn).copy_(mu)
        getattr(layer, "rho_" + wn).copy_(torch.from_numpy(d["f_rho"]))
        if "f_mu_b" in d:
            layer.mu_bias.copy_(torch.from_numpy(d["f_mu_b"]))
            layer.rho_bias.copy_(torch.from_numpy(d["f_rho_b"]))
    return layer.to(device)


def quantized_layer(d, device="cpu"):
    """the twin models.bnn_to_qbnn(flipout=True) builds from a fixture record; a calibrated record's ten entries are set on it"""
    from bayesian_torch_amd.models import bnn_to_qbnn
    m = Block(float_layer(d), bn_of(d) if "bn_weight" in d else None).to(device)
    bnn_to_qbnn(m, fuse_conv_bn="bn_weight" in d, flipout=True)
    q = m.conv1
    if int(d["calibrated"]):
        q.quant_dict = entries(d)
    if int(d["relu"]):
        q.relu = True
    return q


# ---- random cases for the kernels ------------------------------------------------------------------------------------------
def _f64conv(x, w, stride, padding, dilation):
    if x.ndim == 2:
        return x @ w.T
    return torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, stride, padding, dilation).numpy()


def make_case(seed, conv, B, C, N, hw=(1, 1), k=1, stride=1, padding=0, dilation=1, z_x=126, calibrated=True, bias=True, relu=False):
    """a random layer, input and noise, the entries that fit them, and the numpy model's answer.
    The scales are derived, not tuned: each entry's scale is max|value| / 100 of the float quantity it carries (computed here in
    float64 from the very inputs), so that with the calibrated zero points (CAL_ZP, 114 .. 141) values span most of the uint8 range
    and the clamps bind on a few elements only; the zero points are the calibrated ones, and z_x is the caller's."""
    g = np.random.default_rng(seed)
    wshape = (N, C, k, k) if conv else (N, C)
    mu = (g.standard_normal(wshape) * 0.1).astype(np.float32)
    sigma = (np.abs(g.standard_normal(wshape)) * 0.05 + 0.01).astype(np.float32)
    mu_i, s_mu = Q.quantize_weight(mu)
    sigma_i, s_sigma = Q.quantize_weight(sigma)
    xshape = (B, C) + tuple(hw) if conv else (B, C)
    x_i = g.integers(0, 256, xshape).astype(np.uint8)
    s_x = 0.0296
    eps = g.standard_normal(wshape).astype(np.float32)
    eps_b = g.standard_normal(N).astype(np.float32)
    mu_b = (g.standard_normal(N) * 0.5).astype(np.float32) if bias else None
    sigma_b = (np.abs(g.standard_normal(N)) * 0.2 + 0.05).astype(np.float32) if bias else None
    gm = dict(stride=stride, padding=padding, dilation=dilation) if conv else {}
    xf = (x_i.astype(np.float64) - z_x) * s_x
    o1f = _f64conv(xf, mu.astype(np.float64), stride, padding, dilation)
    oshape = o1f.shape
    sign_in = (g.integers(0, 2, xshape) * 2 - 1).astype(np.int8)
    sign_out = (g.integers(0, 2, oshape) * 2 - 1).astype(np.int8)
    pf = _f64conv(xf * sign_in, (sigma * eps).astype(np.float64), stride, padding, dilation)
    amax = lambda v: float(np.abs(v).max()) / 100.0  # noqa: E731
    if calibrated:
        sc = (6 / 255, amax(sigma * eps) * 100 / 127, s_x, amax(o1f), 2 / 255, 2 / 255, amax(xf), amax(pf), amax(pf), amax(o1f + pf * sign_out))
        e = [(float(s), int(z)) for s, z in zip(sc, CAL_ZP)]
        e[2] = (s_x, int(z_x))
        kinds = ("none", "none") if not bias else (("mu", "mu") if conv else ("sigma_eps", "sigma_eps"))
    else:
        e = QF.default_entries(s_sigma)
        kinds = ("mu", "sigma_eps") if bias else ("none", "none")
    ex = (s_x, int(z_x))
    bm, bp = (QF.bias_vec(mu_b, sigma_b, eps_b, kk) for kk in kinds)
    model = QF.layer_forward(x_i, ex, mu_i, s_mu, sigma_i, s_sigma, eps, bm, bp, sign_in, sign_out, e, relu=relu, **gm)
    return dict(conv=conv, mu=mu, sigma=sigma, mu_i=mu_i, s_mu=s_mu, sigma_i=sigma_i, s_sigma=s_sigma, x_i=x_i, e_x=ex, e=e,
                calibrated=calibrated, eps=eps, eps_b=eps_b, mu_b=mu_b, sigma_b=sigma_b, sign_in=sign_in, sign_out=sign_out, kinds=kinds,
                geom=gm, relu=relu, model=model, k=k)


def twin_of(case, device):
    """the quantized twin holding a random case's int8 weights (built directly: quantize() of the float values gives them back)"""
    from bayesian_torch_amd import layers as L
    N, C = case["mu"].shape[:2]
    if case["conv"]:
        q = L.QuantizedConv2dFlipout(C, N, case["k"], bias=case["mu_b"] is not None, **case["geom"])
    else:
        q = L.QuantizedLinearFlipout(C, N)
        if case["mu_b"] is None:
            q.bias = False
            q.mu_bias = q.rho_bias = None
    wn = q._wn
    inv_softplus = lambda s: np.log(np.expm1(s.astype(np.float64))).astype(np.float32)  # noqa: E731
    with torch.no_grad():
        getattr(q, "mu_" + wn).copy_(torch.from_numpy(case["mu"]))
        getattr(q, "rho_" + wn).copy_(torch.from_numpy(inv_softplus(case["sigma"])))
        if case["mu_b"] is not None:
            q.mu_bias.copy_(torch.from_numpy(case["mu_b"]))
            q.rho_bias.copy_(torch.from_numpy(inv_softplus(case["sigma_b"])))
    q.quantize()
    # the stored int8 weights and f32 bias vectors are the case's own (softplus(inv_softplus(s)) may differ from s in the last bit)
    q.quantized_mu_weight.copy_(torch.from_numpy(case["mu_i"].astype(np.int8)))
    q.quantized_sigma_weight.copy_(torch.from_numpy(case["sigma_i"].astype(np.int8)))
    q._q8_scales = (case["s_mu"], case["s_sigma"])
    if case["mu_b"] is not None:
        q.quantized_mu_bias.copy_(torch.from_numpy(case["mu_b"]))
        q.quantized_sigma_bias.copy_(torch.from_numpy(case["sigma_b"]))
    if case["calibrated"]:
        q.quant_dict = list(case["e"])
    q.relu = bool(case["relu"])
    return q.to(device).eval()


def case_noise(case):
    return dict(eps_w=torch.from_numpy(case["eps"]), eps_b=torch.from_numpy(case["eps_b"]), sign_in=torch.from_numpy(case["sign_in"]),
                sign_out=torch.from_numpy(case["sign_out"]))


def unpack_image(W, N, C, k):
    """int8 [N][Kp] weight image -> logical [N, C, k, k] (Linear: [N, C]); also returns whether every padding byte is zero"""
    W = W.cpu().numpy()
    cp = (C + 15) // 16 * 16
    body = W[:, :k * k * cp].reshape(N, k * k, cp)
    pad_zero = not body[:, :, C:].any() and not W[:, k * k * cp:].any()
    w = body[:, :, :C].reshape(N, k, k, C).transpose(0, 3, 1, 2)
    return w, pad_zero
