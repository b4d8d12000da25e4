"""BTX-LRT v1 as a float64 model with the operand roundings of the kernel, and its per-element error envelope.
Plain module, like envelope.py; the contractions run as float64 torch ops on the CPU.

DEFINITION     m = x (*) mu_W + mu_b ,  v = x^2 (*) sigma_W^2 + sigma_b^2 ,  y = m + sqrt(v) * zeta     (one zeta per output element)

OPERANDS       sigma = softplus(rho) in f32, sigma^2 = f32(sigma * sigma).
  f32          mean GEMM (x, mu); variance GEMM (f32(x * x), sigma^2).
  bf16         xr = the activation as the mean GEMM sees it (bf16 input unchanged, f32 input rounded to bf16); mean GEMM
               (xr, bf16(mu)); variance GEMM (bf16(f32(xr) * f32(xr)), bf16(sigma^2)): each operand rounded once; f32 accumulation.
The model reproduces every activation operand and bf16(mu) bit for bit (they are functions of the inputs alone).  sigma is the one
operand it cannot: the kernel's softplus runs on the hardware exp / log and is within envelope.DELTA_W (relative) of the float64
value the model takes.

ENVELOPE       |got - ref| <= c_m A_m + |zeta| sqrt(v64) c_v + u_out (|ref| + the two terms before)
  A_m          the mean contraction on absolute values, |xr| (*) |mu_r| + |mu_b|
  c_m          (K + 8) 2^-23: f32 accumulation over K products (envelope.ACC_UNIT per step, "+ 8" for the bias add and the fused
               multiply-add of the store, as in envelope.rel_constant); the operand term is ZERO, the model holds the same operands
  c_vsum       relative error of the variance sum (every term is >= 0: no cancellation, a relative bound on each product is one on the
               sum).  Operand term of sigma^2: f32  2 delta_w + 2^-24 (sigma twice, one rounding of the product);
               bf16  (2u + 2 delta_w + 2^-24)(1 + u): the kernel's and the model's sigma^2 are each within u of their unrounded values,
               which differ by 2 delta_w + 2^-24 — a value next to a rounding boundary may land on the other side.  Accumulation
               (K + 8) 2^-23 as above (the bias variance is one more term of the same kind).
  c_v          c_vsum / 2 (1 + c_vsum) + 2^-23: half of the sum's relative error reaches the root (sqrt(1 + t) <= 1 + t / 2), then
               sqrtf, counted as two roundings.  zeta itself has no error: btx_fill_eps returns the kernel's values bit for bit.
  u_out        2^-24 for the fused multiply-add that forms y, + u = 2^-8 when the store rounds to bf16.
Where the bound is 0 (a padding-only output of a layer without bias) got must be 0 exactly.

A wrong zeta index, a swapped accumulator or a missing bias variance all land far outside: they change y by a quantity of the
ORDER of sqrt(v) |zeta|, of |m - sqrt-term| or of sqrt(v) (1 - sqrt(1 - sigma_b^2 / v)) |zeta|, against a bound that is c_v ~ 2^-8
(bf16) or ~ 1e-5 (f32) of the same magnitudes; the tests pin this with perturbed references (test_lrt_cpu.py).
"""
import numpy as np
import torch

import envelope as E

U = E.U_BF16
U32 = 2.0 ** -24


def rbf16(a):
    """float32 array -> nearest-even bfloat16, returned as float32 (numpy bit arithmetic; NaN-free inputs)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(a.shape)


def sigma32(rho):
    """softplus as the model takes it: the float64 value rounded to f32"""
    return np.log1p(np.exp(np.asarray(rho, dtype=np.float64))).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def operands(x, mu, rho, prec):
    """(xr, x2, mu_r, s2) as float32 arrays holding the operands of the two GEMMs under BTX-LRT v1"""
    x = np.asarray(x, dtype=np.float32)
    mu = np.asarray(mu, dtype=np.float32)
    sg = sigma32(rho)
    s2 = (sg * sg).astype(np.float32)
    if prec == "f32":
        return x, (x * x).astype(np.float32), mu, s2
    if prec != "bf16":
        raise ValueError("BTX-LRT v1 has no %r form" % (prec,))
    xr = rbf16(x)
    return xr, rbf16((xr * xr).astype(np.float32)), rbf16(mu), rbf16(s2)


def constants(prec, K, store_bf16, delta_w=E.DELTA_W):
    c_m = (K + 8) * E.ACC_UNIT
    op_v = 2 * delta_w + U32 if prec == "f32" else (2 * U + 2 * delta_w + U32) * (1 + U)
    c_vsum = op_v + (K + 8) * E.ACC_UNIT
    c_v = 0.5 * c_vsum * (1 + c_vsum) + 2 * U32
    u_out = U32 + (U if store_bf16 else 0.0)
    return c_m, c_v, u_out


def forward(x, mu, rho, mu_b, rho_b, zeta, op, prec="f32", store_bf16=False):
    """float64 reference and bound.  x, mu, rho in the logical (reference) layouts, zeta in the output's logical shape; op as
    envelope.contract takes it.  -> dict(m, v, ref, bound, A_m, K)"""
    xr, x2, mu_r, s2 = operands(x, mu, rho, prec)
    mb = vb = amb = None
    if mu_b is not None:
        sb = sigma32(rho_b)
        mb, vb, amb = _t(mu_b), _t((sb * sb).astype(np.float32)), _t(np.abs(mu_b))
    m = E.contract(_t(xr), _t(mu_r), mb, op).numpy()
    v = E.contract(_t(x2), _t(s2), vb, op).numpy()
    A_m = E.contract(_t(np.abs(xr)), _t(np.abs(mu_r)), amb, op).numpy()
    z = np.asarray(zeta, dtype=np.float64)
    root = np.sqrt(v)
    ref = m + root * z
    K = E.reduction_length(np.shape(mu), op)
    c_m, c_v, u_out = constants(prec, K, store_bf16)
    b = c_m * A_m + np.abs(z) * root * c_v
    b = b + u_out * (np.abs(ref) + b)
    return dict(m=m, v=v, ref=ref, bound=b, A_m=A_m, K=K)


def through_epilogue(r, scale=None, shift=None, residual=None, relu=0, store_bf16=False, channel_axis=1):
    """the fused epilogue on a forward() result computed with store_bf16=False: eval-BN affine, residual, ReLU / ReLU6 in f32 on the
    pre-store value, then the store's rounding -> (ref, bound).  Uses envelope.through_affine / store_rounding."""
    ref, b = r["ref"], r["bound"]
    if scale is not None or shift is not None:
        shp = [1] * ref.ndim
        shp[channel_axis] = -1
        s = np.ones(ref.shape[channel_axis]) if scale is None else np.asarray(scale, dtype=np.float64)
        t = np.zeros(ref.shape[channel_axis]) if shift is None else np.asarray(shift, dtype=np.float64)
        b = E.through_affine(b, ref, s, t, channel_axis)
        ref = ref * s.reshape(shp) + t.reshape(shp)
    if residual is not None:
        res = np.asarray(residual, dtype=np.float64)
        b = b + U32 * (np.abs(ref) + np.abs(res))
        ref = ref + res
    if relu:
        ref = np.clip(ref, 0.0, 6.0 if relu == 2 else None)  # 1-Lipschitz: the bound passes unchanged
    if store_bf16:
        b = E.store_rounding(b, ref)
    return ref, b


def op_of(layer):
    """envelope.contract's op dict of a layer"""
    op = layer._op
    if op.nd == 0:
        return dict(kind="linear")
    nd = op.nd
    return dict(kind="conv", nd=nd, stride=op.stride[3 - nd:], padding=op.padding[3 - nd:], dilation=op.dilation[3 - nd:],
                groups=op.groups)


def layer_arrays(layer):
    """(mu, rho, mu_b, rho_b) of a layer as float32 numpy arrays in the logical layouts"""
    mu, rho = layer._w()
    f = lambda t: None if t is None else t.detach().float().cpu().contiguous().numpy()  # noqa: E731
    return f(mu), f(rho), f(layer.mu_bias), f(layer.rho_bias)
