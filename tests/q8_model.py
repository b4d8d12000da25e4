"""BTX-Q8 v1 as a numpy model: the integer arithmetic of the INT8 layers, written independently of both the HIP
kernels and torch's quantized engines.  Every floating step is one f32 numpy operation (numpy never contracts), rint is
half-to-even.  tools/make_golden_q8.py asserts this model against the reference before it writes a fixture; the GPU tests
compare the kernels against it bit for bit."""
import numpy as np

f32 = np.float32


def q(v, s, z, lo, hi):
    """clamp(rint(f32(v) * (f32(1) / f32(s))) + z, lo, hi) as int32"""
    inv = f32(1.0) / f32(s)
    r = np.rint(np.asarray(v, dtype=f32) * inv) + f32(z)
    return np.clip(r, f32(lo), f32(hi)).astype(np.int32)


def weight_scale(w, upper_bound=100.0, target_range=255.0, default_scale=0.1):
    """the reference's symmetric scale: 2 * min(max|w|, 100) / 255 in f32, 0 -> 0.1"""
    xmax = np.minimum(np.max(np.abs(np.asarray(w, dtype=f32))), f32(upper_bound)).astype(f32)
    s = f32(f32(xmax * f32(2)) / f32(target_range))
    if s == 0:
        s = f32(default_scale)
    return float(s)


def softplus(rho):
    return np.log1p(np.exp(np.asarray(rho, dtype=f32))).astype(f32)


def quantize_weight(w):
    """-> (int8-valued int32 array, scale)"""
    s = weight_scale(w)
    return q(w, s, 0, -128, 127), s


def default_scales(s_sigma, s_mu, normal_scale=6 / 255):
    """quant_dict is None: s_eps, s_d = s_sigma * s_eps, s_w = max(s_d, s_mu) — Python doubles, as the reference computes them"""
    s_eps = float(normal_scale)
    s_d = float(s_sigma) * s_eps
    return s_eps, s_d, max(s_d, float(s_mu))


def sample_weight(mu_i, s_mu, sigma_i, s_sigma, eps, s_eps, s_d, s_w):
    """eps -> eps_i -> d_i -> W_i (same shape as mu_i).  Returns (W_i, d_i, eps_i)."""
    eps_i = q(eps, s_eps, 0, -128, 127)
    t = (sigma_i.astype(f32) * f32(s_sigma)) * (eps_i.astype(f32) * f32(s_eps))
    d_i = q(t, s_d, 0, -128, 127)
    u = (d_i.astype(f32) * f32(s_d)) + (mu_i.astype(f32) * f32(s_mu))
    return q(u, s_w, 0, -128, 127), d_i, eps_i


def bias_int(mu_b, sigma_b, eps_b, s_x, s_w, n):
    """b = mu_b + sigma_b * eps_b in f32 (sigma_b None: mu_b; mu_b None: 0) -> (int32) rint(double(b) / (double s_x * double s_w))"""
    if mu_b is None:
        return np.zeros(n, dtype=np.int32)
    b = np.asarray(mu_b, dtype=f32)
    if sigma_b is not None:
        b = b + (np.asarray(sigma_b, dtype=f32) * np.asarray(eps_b, dtype=f32))
    return np.rint(b.astype(np.float64) / (float(s_x) * float(s_w))).astype(np.int64).astype(np.int32)


def row_sums(W_i):
    return W_i.reshape(W_i.shape[0], -1).astype(np.int64).sum(axis=1).astype(np.int32)


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def accumulate(x_i, z_x, W_i, stride=1, padding=0, dilation=1):
    """acc = sum_k (x_i - z_x) * W_i, exact.  Linear: x_i [B, K], W_i [N, K] -> [B, N].
    Conv2d: x_i [B, C, H, W], W_i [N, C, KH, KW] -> [B, N, OH, OW]; a padded tap contributes 0."""
    x = np.asarray(x_i, dtype=np.int64) - int(z_x)
    W = np.asarray(W_i, dtype=np.int64)
    if x.ndim == 2:
        return x @ W.T
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    B, C, H, Wd = x.shape
    N, _, KH, KW = W.shape
    OH = (H + 2 * ph - dh * (KH - 1) - 1) // sh + 1
    OW = (Wd + 2 * pw - dw * (KW - 1) - 1) // sw + 1
    xp = np.zeros((B, C, H + 2 * ph, Wd + 2 * pw), dtype=np.int64)
    xp[:, :, ph:ph + H, pw:pw + Wd] = x
    acc = np.zeros((B, N, OH, OW), dtype=np.int64)
    for kh in range(KH):
        for kw in range(KW):
            win = xp[:, :, kh * dh: kh * dh + (OH - 1) * sh + 1: sh, kw * dw: kw * dw + (OW - 1) * sw + 1: sw]
            acc += np.einsum("bchw,nc->bnhw", win, W[:, :, kh, kw])
    return acc


def multiplier(s_x, s_w, s_o):
    return f32(f32(s_x) * f32(s_w)) / f32(s_o)


def requantize(acc, b_i, s_x, s_w, s_o, z_o, relu=False):
    """o_i = clamp(rint(f32(acc + b_i) * M) + z_o, relu ? z_o : 0, 255) as uint8; b_i broadcasts over axis 1"""
    shape = (1, -1) + (1,) * (acc.ndim - 2)
    v = (acc + np.asarray(b_i, dtype=np.int64).reshape(shape)).astype(np.int32).astype(f32)
    r = np.rint(v * multiplier(s_x, s_w, s_o)) + f32(z_o)
    return np.clip(r, f32(z_o if relu else 0), f32(255)).astype(np.uint8)


def dequantize(o_i, s_o, z_o):
    return (o_i.astype(f32) - f32(z_o)) * f32(s_o)


def quantize_input(x, s_x, z_x):
    return q(x, s_x, z_x, 0, 255).astype(np.uint8)


def layer_forward(x_i, z_x, s_x, mu_i, s_mu, sigma_i, s_sigma, eps, mu_b, sigma_b, eps_b, s_eps, s_d, s_w, s_o, z_o,
                  stride=1, padding=0, dilation=1, relu=False):
    """one quantized layer on an already quantized input.  Returns dict(W, S, b_i, acc, out): out is uint8 (a Linear caller
    dequantizes with dequantize())."""
    W_i, _, _ = sample_weight(mu_i, s_mu, sigma_i, s_sigma, eps, s_eps, s_d, s_w)
    b_i = bias_int(mu_b, sigma_b, eps_b, s_x, s_w, W_i.shape[0])
    acc = accumulate(x_i, z_x, W_i, stride, padding, dilation)
    return dict(W=W_i, S=row_sums(W_i), b_i=b_i, acc=acc, out=requantize(acc, b_i, s_x, s_w, s_o, z_o, relu))
