"""BTX-Q8 v1 extended to Flipout ("Flipout") as a numpy model, beside q8_model (the Reparameterization layers) and
q8_net_model (the ops between layers).  One forward is the reference's six quantized ops (two convs, three quantized.mul, one
quantized.add) on the ten (scale, zero point) entries e0 .. e9 of its quant_dict.  Written independently of the HIP kernels and of
torch's quantized engine; every floating step is one f32 numpy operation, rint is half-to-even.
tools/make_golden_q8_flipout.py asserts it against the reference before it writes a fixture; the GPU tests compare the kernels
against it bit for bit."""
import numpy as np

import q8_model as Q
import q8_net_model as QN

f32 = np.float32


def default_entries(s_sigma, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128):
    """quant_dict is None: the reference's defaults as ten entries (Python doubles, as the reference computes them)"""
    d = (float(default_scale), int(default_zero_point))
    return [(float(normal_scale), 0), (float(s_sigma) * float(normal_scale), 0)] + [d] * 8


def mul_multiplier(s_a, s_b, s_o):
    """m of quantized.mul: f32(f32(s_a) * f32(s_b)) * (f32(1) / f32(s_o))"""
    return f32(f32(s_a) * f32(s_b)) * (f32(1.0) / f32(s_o))


def qmul(a, z_a, b, z_b, m, z_o, lo, hi):
    """torch.ops.quantized.mul: c = (a - z_a) * (b - z_b) in int32; clamp(rint(f32(c) * m) + z_o, lo, hi) as int32"""
    c = (np.asarray(a, dtype=np.int32) - np.int32(z_a)) * (np.asarray(b, dtype=np.int32) - np.int32(z_b))
    r = np.rint(c.astype(f32) * f32(m)) + f32(z_o)
    return np.clip(r, f32(lo), f32(hi)).astype(np.int32)


def sign_bytes(e):
    """the two bytes of a quantized sign tensor: (q(+1, e), q(-1, e))"""
    s, z = e
    return int(Q.q(1.0, s, z, 0, 255)), int(Q.q(-1.0, s, z, 0, 255))


def sample_delta(sigma_i, s_sigma, eps, e0, e1):
    """eps -> eps_i -> d_i = quantized.mul(sigma_i, eps_i -> e1), all qint8 with zero point 0.  Returns (d_i, eps_i)."""
    eps_i = Q.q(eps, e0[0], 0, -128, 127)
    d_i = qmul(sigma_i, 0, eps_i, 0, mul_multiplier(s_sigma, e0[0], e1[0]), 0, -128, 127)
    return d_i, eps_i


def sign_mul(x_i, e_x, sign, e_s, e_o):
    """quantized.mul(x, q(sign, e_s) -> e_o): x_i uint8-valued, sign an array of +1 / -1 of x_i's shape.  uint8."""
    pos, neg = sign_bytes(e_s)
    sb = np.where(np.asarray(sign) < 0, neg, pos)
    return qmul(x_i, e_x[1], sb, e_s[1], mul_multiplier(e_x[0], e_s[0], e_o[0]), e_o[1], 0, 255).astype(np.uint8)


def bias_vec(mu_b, sigma_b, eps_b, kind):
    """the f32 bias vector of one GEMM: kind 'none' | 'mu' | 'sigma_eps' (f32(sigma_b * eps_b))"""
    if kind == "none":
        return None
    if kind == "mu":
        return np.asarray(mu_b, dtype=f32)
    return np.asarray(sigma_b, dtype=f32) * np.asarray(eps_b, dtype=f32)


def tail(o1, p, sign_out, e, relu=False):
    """the store of the contraction from the two requantized accumulators: p2 = mul(p, sign byte -> e8), out = add(o1, p2 -> e9).
    Returns (p2, out), uint8."""
    p2 = sign_mul(p, e[7], sign_out, e[5], e[8])
    out = QN.add(o1, e[3][0], e[3][1], p2, e[8][0], e[8][1], e[9][0], e[9][1], relu)
    return p2, out


def layer_forward(x_i, e_x, mu_i, s_mu, sigma_i, s_sigma, eps, b_mean, b_pert, sign_in, sign_out, e, stride=1, padding=0,
                  dilation=1, relu=False):
    """one quantized Flipout layer on an already quantized input x_i at e_x = (s_x, z_x) (e[2] unless x arrived quantized).
    mu_i / sigma_i: int8-valued, the logical weight shape; b_mean / b_pert: f32 vectors or None; sign_in / sign_out: +1 / -1 arrays
    of the input's / output's logical shape.  Returns every intermediate: d_i, xp, bm_i, bp_i, o1, p, p2, out (uint8; a Linear caller
    dequantizes with q8_model.dequantize at e[9])."""
    for name, (s, z) in (("eps", e[0]), ("mul", e[1])):
        if z != 0:
            raise ValueError("entry '%s' must be symmetric" % name)
    n = mu_i.shape[0]
    s_x, z_x = e_x
    d_i, eps_i = sample_delta(sigma_i, s_sigma, eps, e[0], e[1])
    bm_i = Q.bias_int(b_mean, None, None, s_x, s_mu, n)
    o1 = Q.requantize(Q.accumulate(x_i, z_x, mu_i, stride, padding, dilation), bm_i, s_x, s_mu, e[3][0], e[3][1])
    xp = sign_mul(x_i, e_x, sign_in, e[4], e[6])
    bp_i = Q.bias_int(b_pert, None, None, e[6][0], e[1][0], n)
    # a padded tap of the perturbed conv holds the zero point of x' (e6), i.e. contributes 0
    p = Q.requantize(Q.accumulate(xp, e[6][1], d_i, stride, padding, dilation), bp_i, e[6][0], e[1][0], e[7][0], e[7][1])
    p2, out = tail(o1, p, sign_out, e, relu)
    return dict(eps_i=eps_i, d_i=d_i, xp=xp, bm_i=bm_i, bp_i=bp_i, o1=o1, p=p, p2=p2, out=out)
