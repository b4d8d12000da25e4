"""The ops between the INT8 layers ("between the layers") as a numpy model, beside q8_model (the layers themselves):
the quantized add with its optional ReLU, max-pool, avg-pool, and the residual epilogue (requantize, then add).  Written
independently of the HIP kernels and of torch's quantized engine; every floating step is one f32 operation, rint is half-to-even.
tools/make_golden_q8net.py asserts it against torch's own ops and the reference's Bottleneck before it writes a fixture; the GPU
tests compare the kernels against it bit for bit."""
import numpy as np

import q8_model as Q

f32, f64 = np.float32, np.float64


def add_consts(s_a, z_a, s_b, z_b, s):
    """the three f32 constants the host computes once: pre_a = f32(s_a * f32(-z_a)), pre_b, 1 / s"""
    return f32(s_a) * f32(-int(z_a)), f32(s_b) * f32(-int(z_b)), f32(1.0) / f32(s)


def _fma(s, q, pre):
    """f32 fma(s, q, pre), one rounding: the product of a 24-bit and an 8-bit significand and its sum with an f32 are exact in f64"""
    return (np.asarray(q, dtype=f64) * f64(f32(s)) + f64(pre)).astype(f32)


def add(a, s_a, z_a, b, s_b, z_b, s, z, relu=False):
    """o = clamp(rint((fma(s_a, a, pre_a) + fma(s_b, b, pre_b)) * (1 / s)) + z, relu ? z : 0, 255) as uint8"""
    pre_a, pre_b, inv = add_consts(s_a, z_a, s_b, z_b, s)
    t = (_fma(s_a, a, pre_a) + _fma(s_b, b, pre_b)) * inv
    r = np.rint(t) + f32(z)
    return np.clip(r, f32(z if relu else 0), f32(255)).astype(np.uint8)


def add_naive(a, s_a, z_a, b, s_b, z_b, s, z, relu=False):
    """the (a - z_a) * s_a form one would guess: NOT what torch computes (kept to show the difference)"""
    da = (np.asarray(a, dtype=f32) - f32(z_a)) * f32(s_a)
    db = (np.asarray(b, dtype=f32) - f32(z_b)) * f32(s_b)
    r = np.rint((da + db) * (f32(1.0) / f32(s))) + f32(z)
    return np.clip(r, f32(z if relu else 0), f32(255)).astype(np.uint8)


def relu(q, z):
    return np.maximum(np.asarray(q), np.uint8(z)).astype(np.uint8)


def _windows(H, W, k, s, p):
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    for ho in range(Ho):
        for wo in range(Wo):
            h0, w0 = ho * s - p, wo * s - p
            yield ho, wo, max(h0, 0), min(h0 + k, H), max(w0, 0), min(w0 + k, W)


def max_pool(x, k, s, p):
    """x uint8 [B, C, H, W]: the maximum over the in-image elements of each window (floor mode)"""
    B, C, H, W = x.shape
    out = np.zeros((B, C, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1), dtype=np.uint8)
    for ho, wo, h0, h1, w0, w1 in _windows(H, W, k, s, p):
        out[:, :, ho, wo] = x[:, :, h0:h1, w0:w1].max(axis=(2, 3))
    return out


def avg_pool(x, z, k, s):
    """no padding, floor mode: o = clamp(rint(f32(sum - cnt * z) * f32(1.0 / cnt)) + z, 0, 255), int32 sum, double reciprocal"""
    B, C, H, W = x.shape
    cnt = k * k
    rcp = f32(1.0 / float(cnt))
    out = np.zeros((B, C, (H - k) // s + 1, (W - k) // s + 1), dtype=np.uint8)
    for ho, wo, h0, h1, w0, w1 in _windows(H, W, k, s, 0):
        sm = x[:, :, h0:h1, w0:w1].astype(np.int32).sum(axis=(2, 3), dtype=np.int32) - np.int32(cnt * int(z))
        r = np.rint(sm.astype(f32) * rcp) + f32(z)
        out[:, :, ho, wo] = np.clip(r, f32(0), f32(255)).astype(np.uint8)
    return out


def conv_add(acc, b_i, s_x, s_w, s_o, z_o, conv_relu, res, s_r, z_r, s, z, add_relu):
    """the residual epilogue: requantize the accumulator as the conv alone would, then add the residual"""
    o = Q.requantize(acc, b_i, s_x, s_w, s_o, z_o, conv_relu)
    return add(o, s_o, z_o, res, s_r, z_r, s, z, add_relu)
