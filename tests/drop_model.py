"""BTX-DROP v1 in numpy: the keep bits, the keep rule and the arithmetic of a kept element, written from the
specification alone (no torch in the arithmetic) — what csrc/btx_drop.hip and functional.dropout_mask_aten are compared with, bit
for bit."""
import math

import numpy as np

STREAM_DROP = 7
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (counter c0..c3, key k0, k1) -> the four output words"""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]   # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def params(p):
    """(T, scale): T = clamp(floor((1 - p) * 65536 + 0.5), 0, 65536) in double; scale = f32(65536.0 / T), 0 when T == 0"""
    T = min(65536, max(0, int(math.floor((1.0 - float(p)) * 65536.0 + 0.5))))
    return T, (np.float32(65536.0 / T) if T else np.float32(0.0))


def bits16(i, seed, sample_idx, layer_id):
    """the sixteen random bits of element index i (any integer array)"""
    i = np.asarray(i, dtype=np.uint64)
    g = i >> np.uint64(3)
    assert g.size == 0 or int(g.max()) <= 0xFFFFFFFF
    P = philox4x32_10(g, sample_idx, layer_id, STREAM_DROP, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = (i >> np.uint64(1)) & np.uint64(3)
    word = np.choose(w.astype(np.int64), P)
    return (word >> (np.uint64(16) * (i & np.uint64(1)))) & np.uint64(0xFFFF)


def index(shape, mode):
    """the element index of every LOGICAL element of a tensor of `shape`: channels-last position [n][spatial...][c] (rank <= 3:
    row-major), or n * C + c in channel mode (rank >= 3)"""
    shape = tuple(int(v) for v in shape)
    if mode == "channel":
        assert len(shape) >= 3
        N, C = shape[:2]
        return np.broadcast_to(np.arange(N * C, dtype=np.uint64).reshape((N, C) + (1,) * (len(shape) - 2)), shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if len(shape) < 4:
        return np.arange(n, dtype=np.uint64).reshape(shape)
    nd = len(shape) - 2
    cl = np.arange(n, dtype=np.uint64).reshape((shape[0],) + shape[2:] + (shape[1],))
    return cl.transpose((0, nd + 1) + tuple(range(1, nd + 1)))


def mask(shape, mode, T, seed, sample_idx, layer_id):
    """the bool KEEP mask in the logical shape"""
    return bits16(index(shape, mode), seed, sample_idx, layer_id) < np.uint64(T)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(f):
    """round to nearest even; NaN -> 0x7fc0"""
    u = np.asarray(f, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint16(0x7FC0), r)


def apply_f32(x, keep, scale):
    """kept: one f32 multiply; dropped: +0.0 by selection"""
    with np.errstate(all="ignore"):
        kept = np.asarray(x, dtype=np.float32) * np.float32(scale)
    return np.where(keep, kept, np.float32(0.0)).astype(np.float32)


def apply_bf16(x_bits, keep, scale):
    """x as uint16 bf16 bit patterns -> bf16 bit patterns: f32(x) * scale in f32, rounded once (RNE)"""
    with np.errstate(all="ignore"):
        kept = f32_to_bf16_bits(bf16_bits_to_f32(x_bits) * np.float32(scale))
    return np.where(keep, kept, np.uint16(0)).astype(np.uint16)
