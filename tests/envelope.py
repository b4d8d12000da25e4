"""Per-element rounding envelopes, exact-integer inputs and impulse probes for the contraction kernels (plain module,
like helpers.py; DESIGN.md §2 states the same formulas).

ENVELOPE.  For out_j = sum_i a_i w_i computed with rounded operands and f32 accumulation, |got_j - ref_j| <= c * A_j with
A_j = sum_i |a_i| |w_i| — the same contraction on absolute values, so float64 torch produces it with one more call:

  forward          A = op(|x|, |mu| + |sigma eps|) + |mu_b| + |sigma_b eps_b|   (|mu + sigma eps| <= |mu| + |sigma eps| covers
                                                                                 Reparameterization; the Flipout signs are +-1)
  data gradient    A = op^T(|dy|, |mu| + |sigma eps|)
  weight gradient  A = corr(|x|, |dy|)                                           (dW_mu and dW_delta alike)

The constant is derived, not fitted.  u = 2^-8, the unit roundoff of bf16 under round-to-nearest-even (8 significant bits: 7
stored + the hidden one, so half an ulp is 2^-8 of the binade's lower end — 1 + 2^-8 rounds to 1), K = length of the reduction.
(2^-9 is NOT a bound: a single rounding reaches 1.99 * 2^-9, which the K = 1 impulse probes and every bf16 store of an
f32-accurate result show on all kernel families alike; test_envelope_cpu.py pins this on the CPU.)

  operand term   f32     delta_w                       the sampled weight is the only rounded operand
                 bf16    2u + u^2 + delta_w            both operands rounded once
                 bf16x3  3u^2 + 2u^3 + delta_w         x = x_h + x_l (+u^2), w likewise, the w_l x_l product is dropped
  accumulation   (K_acc + 8) 2^-23, K_acc = K (3K for bf16x3: three MFMAs per product).  2^-23 rather than 2^-24: the rounding
                 inside one bf16 MFMA K-step is not documented; +8 covers split-K combine, Flipout combine and bias adds
  bf16 store     + u (|ref_j| + bound_j)
  f32 reference  + (K + 8) 2^-24 A_j when the reference itself was evaluated in f32

delta_w is the relative error of the weight the kernel samples for itself (hardware exp / log softplus, eps as
materialised) against float64 log1p(exp rho).  It is MEASURED by the impulse probes of test_gpu_elementwise.py (an impulse
input makes every output a single product, so an f32 launch returns the sampled weights themselves) and DELTA_W below is
twice the measured maximum; profiles/elementwise_envelope.txt holds the measurement.

The bias is added in f32 by the epilogue: its share of the bound uses the f32 constant whatever the MFMA precision.
Eval-BN multiplies a bound by |scale_n| and adds 4 * 2^-24 of the magnitudes involved; a residual adds only its store
rounding; ReLU, ReLU6 and max are 1-Lipschitz in the sup norm, so a bound passes ReLU unchanged and MaxPool2d as the max-pool
of the bound.

check() compares EVERY element; none is excluded, there is no percentile and no mean.  Where the bound is 0 (padding-only
outputs without a bias) the output must equal the reference exactly.

KNOWN LIMIT.  For the weight gradient at the baseline sizes K is the pixel count (200 704): the rigorous accumulation term
reaches 1.2e-2 * A and the envelope says nothing in f32.  Use it for weight gradients on small cases only; the
exact-integer inputs below (small_ints) cover the large ones with zero tolerance: with |v| <= 3 every product and partial
sum is an integer below 2^24, f32 accumulation is exact in any order and bf16 / the hi+lo split hold the operands exactly.

REDUCTIONS (BatchNorm training, MC accumulate, KL gradients, global average pool; second half of this file).  u32 = 2^-24, the unit
roundoff of f32.  Every constant below is a count of roundings, written out where it is used; none is fitted.

  BatchNorm   the kernel sums d = x - pivot and d^2 per channel in f32 along a chain of K = rows per thread + rows per block
              additions (bn_chain), then folds the blocks in f64.  Statistics term, per channel, with S1 = mean|d|, S2 = mean d^2,
              ms = mean d:   |dmean| <= (K + 8) u32 S1      |dvar| <= (K + 8) u32 (S2 + 2 |ms| S1)
              (K additions, the rounding of d, of d^2 and of the fma, slack for second order: the "+ 8").  invstd follows with the
              derivative 1 / (2 (var + eps)).  The apply pass is y = fma(sc, x, shift), sc = fl(g fl(invstd)), shift =
              fl(b - fl(fl(mean) sc)): roundings 3 on |sc x|, 6 on |sc mean|, 2 on |b|  ->  8 u32 (|sc x| + |sc mean| + |b|); the
              statistics enter through (x - mean) dsc and sc dmean, because the SAME sc multiplies x and mean.
              Backward: s = sum g, q = sum g xhat on the same chain: |ds| <= (K + 8) u32 sum|g|, |dq| <= (K + 8) u32 sum|g xhat| +
              sum|g| |dxhat| with dxhat from the saved (f32) mean and invstd.  dx = fma(A, g, fma(B, x, D)) with A, B, D rounded
              to f32 from f64 values: roundings 2 on |A g|, 3 on |B x|, 3 on |D|  ->  4 u32 (|A g| + |B x| + |D|); the reduction
              term is |g - s/M| dA + |A| ds / M + |x - mean| dB + |B| dmean.  bf16 outputs: store_rounding on top.
  MC          p = exp(x - max) / sum: relative bound (|x - max| + ceil(C / 256) + c0) 2^-23 — the argument's rounding scales with
              |x - max|, the row sum is four chains of ceil(C / 256) additions, c0 = C0_ULP is the error of expf / logf in ulps —
              plus (c0 + 1) 2^-149 where the result is subnormal.  Carried through p^2 and p log(p + 1e-15); the entropy adds
              (ceil(C / 256) + 9) u32 sum|t| for its own chains and tree.  Accumulating S samples in f32 adds u32 times every
              running sum (<= S u32 while the running sums stay below 1, which holds in every case of the tests).
  KL          dmu = g (mu - pm) / ps^2: six roundings -> 8 u32 |dmu|.  drho = g (sig / ps^2 - 1 / sig) sig': the two terms
              cancel near sig = ps, so the bound is on magnitudes: (c1 u32 + DELTA_W) g (sig / ps^2 + 1 / sig) sig' with
              c1 = 12 + 2 c0 (ten roundings and the expf inside sig'; DELTA_W is the softplus, as for the sampled weights).
  avg-pool    small integers: f32(sum) * f32(1 / HW), one rounding, then the store's: exact, zero tolerance.

FUSED LSTM (third part of this file, derivations in its header): per-step float64 references fed with the GPU's own sampled
weights, previous state and saved buffers — gates (accumulation only), cell / hidden state (transcendentals only) and a backward
through time whose bound is propagated operation by operation (Err).
"""
import numpy as np
import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8
ACC_UNIT = 2.0 ** -23
REF32_UNIT = 2.0 ** -24
# relative error of the in-kernel sampled weight against float64: 2 x the maximum the impulse probes measured on an MI355X.
# Three runs with different noise draws gave 4.76e-7, 4.77e-7 and 4.68e-7 (run-time-tap patch kernel and the 8-wave GEMM; the
# other families 1.8e-7 .. 4.2e-7; rho uniform in [-9, 2] and MOPED-style rho): profiles/elementwise_envelope.txt
DELTA_W = 9.55e-7

PRECISIONS = ("f32", "bf16", "bf16x3")


def operand_term(prec, delta_w=DELTA_W):
    u = U_BF16
    if prec == "f32":
        return delta_w
    if prec == "bf16":
        return 2 * u + u * u + delta_w
    if prec == "bf16x3":
        return 3 * u * u + 2 * u ** 3 + delta_w
    raise ValueError(prec)


def rel_constant(prec, K, delta_w=DELTA_W, ref_f32=False):
    """c of |got - ref| <= c * A for a reduction of length K"""
    k_acc = 3 * K if prec == "bf16x3" else K
    c = operand_term(prec, delta_w) + (k_acc + 8) * ACC_UNIT
    if ref_f32:
        c += (K + 8) * REF32_UNIT
    return c


def bound(A, prec, K, ref=None, A_bias=None, store_bf16=False, ref_f32=False, delta_w=DELTA_W):
    """per-element bound (float64 numpy).  A: the contraction on absolute values; A_bias: |mu_b| + |sigma_b eps_b| broadcast
    to A's shape (added in f32 by the epilogue); store_bf16 needs ref (the result is rounded once more on store)."""
    A = _np(A)
    b = rel_constant(prec, K, delta_w, ref_f32) * A
    if A_bias is not None:
        b = b + rel_constant("f32", 0, delta_w, ref_f32) * _np(A_bias)
    if store_bf16:
        b = store_rounding(b, ref)
    return b


def store_rounding(b, ref, u=U_BF16):
    """the bound after one more rounding of the result to bf16"""
    return _np(b) + u * (np.abs(_np(ref)) + _np(b))


def through_affine(b, ref_pre, scale, shift, channel_axis=1):
    """eval-BN folded into the store: out = pre * scale[c] + shift[c] in f32"""
    b, ref_pre = _np(b), _np(ref_pre)
    shp = [1] * b.ndim
    shp[channel_axis] = -1
    s = np.abs(_np(scale)).reshape(shp)
    t = np.abs(_np(shift)).reshape(shp) if shift is not None else 0.0
    return b * s + 4 * REF32_UNIT * ((np.abs(ref_pre) + b) * s + t)


def through_maxpool2d(b, kernel, stride, padding):
    """max is 1-Lipschitz in the sup norm: the bound of a pooled output is the max of the bounds in its window"""
    return F.max_pool2d(torch.as_tensor(_np(b)), kernel, stride, padding).numpy()


def _np(t):
    if isinstance(t, torch.Tensor):
        return t.detach().to(torch.float64).cpu().numpy()
    return np.asarray(t, dtype=np.float64)


class Report:
    """worst: max err / bound over all elements (inf where the bound is 0 and the values differ); violations: elements with
    err > bound; index: position of the worst element in the tensor's logical shape — (image, channel, row, col) for 2-D"""

    def __init__(self, worst, violations, index, err, bnd, numel):
        self.worst, self.violations, self.index, self.err, self.bnd, self.numel = worst, violations, index, err, bnd, numel

    @property
    def ok(self):
        return self.violations == 0

    def line(self, name, prec):
        return "%s %s: worst err/bound %.3g at %s (%d of %d outside)" % (name, prec, self.worst, self.index, self.violations,
                                                                       self.numel)

    def __str__(self):
        return "worst err/bound %.4g at %s (err %.4g, bound %.4g); %d of %d elements outside the envelope" % (
            self.worst, self.index, self.err, self.bnd, self.violations, self.numel)


def check(got, ref, bnd):
    """|got - ref| <= bnd for EVERY element -> Report.  NaN / inf in got is a violation."""
    g, r, b = _np(got), _np(ref), _np(bnd)
    assert g.shape == r.shape == b.shape, (g.shape, r.shape, b.shape)
    err = np.abs(g - r)
    err = np.where(np.isfinite(err), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, np.where(b > 0.0, err / b, np.inf))
    flat = int(np.argmax(ratio)) if ratio.size else 0
    idx = tuple(int(v) for v in np.unravel_index(flat, ratio.shape)) if ratio.size else ()
    return Report(float(ratio.max()) if ratio.size else 0.0, int((err > b).sum()), idx,
                  float(err.reshape(-1)[flat]) if ratio.size else 0.0, float(b.reshape(-1)[flat]) if ratio.size else 0.0,
                  int(ratio.size))


def check_exact(got, ref):
    """zero tolerance (exact-integer runs): Report with the bound 0 everywhere"""
    r = _np(ref)
    return check(got, r, np.zeros_like(r))


# ---- A: the contraction on absolute values, float64 on the CPU -----------------------------------------------------------
_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}
_CONVT = {1: F.conv_transpose1d, 2: F.conv_transpose2d, 3: F.conv_transpose3d}


def contract(x, w, b, op):
    """op as in oracle/bt_ref.py: dict(kind='linear') | dict(kind='conv'|'convT', nd, stride, padding, dilation, groups[, output_padding])"""
    if op["kind"] == "linear":
        return F.linear(x, w, b)
    if op["kind"] == "conv":
        return _CONV[op["nd"]](x, w, b, op["stride"], op["padding"], op["dilation"], op["groups"])
    return _CONVT[op["nd"]](x, w, b, op["stride"], op["padding"], op.get("output_padding", 0), op["groups"], op["dilation"])


def reduction_length(w_shape, op):
    """K of the forward: taps x input channels per group"""
    if op["kind"] == "linear":
        return int(w_shape[1])
    taps = int(np.prod(w_shape[2:]))
    if op["kind"] == "conv":
        return int(w_shape[1]) * taps
    return int(w_shape[0]) // int(op["groups"]) * taps  # transposed: the weight is [Cin, Cout/groups, *k]


def dgrad_reduction_length(w_shape, op):
    """K of the data gradient: taps x output channels per group"""
    if op["kind"] == "linear":
        return int(w_shape[0])
    taps = int(np.prod(w_shape[2:]))
    if op["kind"] == "conv":
        return int(w_shape[0]) // int(op["groups"]) * taps
    return int(w_shape[1]) * taps


def d64(t):
    return None if t is None else t.detach().to(torch.float64).cpu().contiguous()


def sigma64(rho):
    return torch.log1p(torch.exp(d64(rho)))


def abs_weight(mu, rho, eps):
    """|mu| + |sigma eps| in float64"""
    return d64(mu).abs() + (sigma64(rho) * d64(eps)).abs()


def reference_forward(x, mu, rho, eps, mu_b, rho_b, eps_b, sign_in, sign_out, op):
    """the layer's value in float64 (Flipout when sign_in is given, else Reparameterization) and the parts of its envelope:
    -> (ref, A, A_bias | None), float64 CPU tensors"""
    x, mu, eps = d64(x), d64(mu), d64(eps)
    delta = sigma64(rho) * eps
    bias = bias_d = None
    if mu_b is not None:
        bias, bias_d = d64(mu_b), sigma64(rho_b) * d64(eps_b)
    if sign_in is not None:
        ref = contract(x, mu, bias, op) + contract(x * d64(sign_in), delta, bias_d, op) * d64(sign_out)
    else:
        ref = contract(x, mu + delta, None if bias is None else bias + bias_d, op)
    A = contract(x.abs(), mu.abs() + delta.abs(), None, op)
    A_bias = None
    if bias is not None:
        shp = [1] * ref.dim()
        shp[-1 if op["kind"] == "linear" else 1] = -1
        A_bias = (bias.abs() + bias_d.abs()).reshape(shp).expand_as(ref)
    return ref, A, A_bias


def dgrad_A(dy, x_shape, w_abs, op):
    """op^T(|dy|, |W|): autograd through the float64 contraction on absolute values"""
    xz = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(contract(xz, d64(w_abs), None, op), xz, d64(dy).abs())
    return g


def wgrad_A(x, dy, w_shape, op):
    """corr(|x|, |dy|) in the weight's logical shape"""
    wz = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(contract(d64(x).abs(), wz, None, op), wz, d64(dy).abs())
    return g


def wgrad64(x, dy, w_shape, op):
    """dW = corr(x, dy) in float64"""
    wz = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(contract(d64(x), wz, None, op), wz, d64(dy))
    return g


def wgrad_reduction_length(dy_shape, op):
    """K of the weight gradient: output pixels x batch"""
    if op["kind"] == "linear":
        return int(np.prod(dy_shape[:-1]))
    return int(dy_shape[0]) * int(np.prod(dy_shape[2:]))


# ---- exact-integer inputs ---------------------------------------------------------------------------------------------------
def small_ints(shape, seed, lim=3, dtype=torch.float32):
    """integers in [-lim, lim]: exact in bf16, products and sums of up to 2^24 / lim^2 of them exact in f32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).to(dtype)


def dyadic(shape, seed, m=128, shift=7, dtype=torch.float32):
    """m' * 2^-shift with |m'| <= m: 8 significant bits, exact in bf16"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-m, m + 1, tuple(shape), generator=g).to(torch.float64) * 2.0 ** -shift).to(dtype)


# ---- impulse probes ---------------------------------------------------------------------------------------------------------
def impulse_batch(channels, spatial, pixels):
    """one image per (channel, pixel): x[i] = e_c at pixel p -> (x [len(pixels) * channels, channels, *spatial], list of (c, p))"""
    n = len(pixels) * channels
    x = torch.zeros((n, channels) + tuple(spatial))
    where = []
    for p in pixels:
        for c in range(channels):
            x[(len(where), c) + tuple(p)] = 1.0
            where.append((c, tuple(p)))
    return x, where


# =============================================================================================================================
# reductions: BatchNorm training, MC accumulate, KL gradients, global average pool (derivations in the docstring)
# =============================================================================================================================
# error of the device's f32 exp and log in ulps: 2 x the maximum of torch.exp on [-104, 0] and torch.log on [1e-38, 1] (the math
# library functions btx_small.hip calls) against float64 on an MI355X, 4 M points each — exp 1.00 ulp (subnormal results
# included), log 1.88 ulp: profiles/reduction_envelope.txt
C0_ULP = 3.77
TINY32 = 2.0 ** -149  # the smallest subnormal of f32


def ulp32(v):
    """the spacing of f32 at |v| (float64 numpy), 2^-149 below the normal range"""
    a = np.abs(_np(v))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.maximum(np.where(a > 0, 2.0 ** (e - 23), TINY32), TINY32)


def ulp_error(got, ref):
    """max |got - ref| / ulp32(ref) -> (worst, index)"""
    r = np.abs(_np(got) - _np(ref)) / ulp32(ref)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i


def bn_chain(M, C):
    """K of btx_bn.hip: the longest f32 addition chain of a channel's sums — rows per thread plus rows per block"""
    cg = C // 8
    rpb = max(256 // cg, 1)
    nblk = min(max(-(-M // (rpb * 8)), 1), 512)
    return -(-M // (nblk * rpb)) + rpb


def bn_pivot(x):
    """the kernel's pivot: per channel the median of rows 0, M/2 and M-1 of x [M, C]"""
    M = x.shape[0]
    return torch.stack([x[0], x[M // 2], x[M - 1]]).median(0).values


def bn_forward64(x, gamma, beta, eps, K, residual=None, relu=False):
    """training-mode BatchNorm of x [M, C] (float64 torch, the dtype-rounded values) and the parts of its envelope -> dict of
    float64 torch tensors: y, b_y (before any bf16 store), mean, var, invstd and their bounds d_mean, d_var, d_invstd (as SAVED
    in f32: statistics + one rounding), dm_stat / dv_stat (statistics alone)"""
    u = REF32_UNIT
    M, C = x.shape
    g = torch.ones(C, dtype=torch.float64) if gamma is None else d64(gamma)
    b = torch.zeros(C, dtype=torch.float64) if beta is None else d64(beta)
    eps = float(np.float32(eps))
    d = x - bn_pivot(x)
    ms, S1, S2 = d.mean(0), d.abs().mean(0), (d * d).mean(0)
    mean = x.mean(0)
    xc = x - mean
    var = (xc * xc).mean(0)
    st = (K + 8) * u
    dm_stat = st * S1
    dv_stat = st * (S2 + 2 * ms.abs() * S1)
    invstd = 1.0 / torch.sqrt(var + eps)
    dis_stat = invstd * dv_stat / (2 * (var + eps))
    sc = g * invstd
    y = xc * sc + b
    b_y = 8 * u * ((sc * x).abs() + (sc * mean).abs() + b.abs()) + xc.abs() * g.abs() * dis_stat + sc.abs() * dm_stat
    if residual is not None:
        b_y = b_y + 2 * u * (y.abs() + residual.abs() + b_y)
        y = y + residual
    if relu:
        y = torch.relu(y)  # 1-Lipschitz: the bound passes unchanged
    return dict(y=y, b_y=b_y, mean=mean, var=var, invstd=invstd, dm_stat=dm_stat, dv_stat=dv_stat, d_mean=dm_stat + u * mean.abs(),
                d_var=dv_stat, d_invstd=dis_stat + u * invstd, g=g, xc=xc, M=M)


def bn_running64(f, old_mean, old_var, momentum):
    """running estimates after one step and their bounds (f32 storage) -> (rm, b_rm, rv, b_rv)"""
    u = REF32_UNIT
    mom = float(np.float32(momentum))
    M = f["M"]
    unb = f["var"] * (M / (M - 1.0)) if M > 1 else f["var"]
    a, c = (1.0 - mom) * d64(old_mean), mom * f["mean"]
    rm, b_rm = a + c, 4 * u * (a.abs() + c.abs()) + mom * f["dm_stat"]
    a, c = (1.0 - mom) * d64(old_var), mom * unb
    rv, b_rv = a + c, 4 * u * (a.abs() + c.abs()) + mom * f["dv_stat"] * (M / (M - 1.0) if M > 1 else 1.0)
    return rm, b_rm, rv, b_rv


def bn_backward64(x, dy, f, K, mask=None):
    """dx, dgamma, dbeta of training-mode BatchNorm in float64 with their bounds; f = bn_forward64(...); mask: where the fused ReLU
    let the gradient pass (the kernel's own y > 0) -> dict(dx, b_dx, dgamma, b_dgamma, dbeta, b_dbeta, g)"""
    u = REF32_UNIT
    M = f["M"]
    st = (K + 8) * u
    gy = dy if mask is None else dy * mask
    mean, invstd, gam, xc = f["mean"], f["invstd"], f["g"], f["xc"]
    xhat = xc * invstd
    s, q = gy.sum(0), (gy * xhat).sum(0)
    Sa, Sq = gy.abs().sum(0), (gy * xhat).abs().sum(0)
    ds = st * Sa
    dq = st * Sq + Sa * invstd * f["d_mean"] + Sq * f["d_invstd"] / invstd
    A = gam * invstd
    B = -A * invstd * q / M
    D = -A * s / M - B * mean
    dA = gam.abs() * f["d_invstd"]
    dB = B.abs() * 2 * f["d_invstd"] / invstd + A.abs() * invstd * dq / M
    dx = A * (gy - s / M) + B * xc
    b_dx = (4 * u * ((A * gy).abs() + (B * x).abs() + D.abs()) + dA * (gy - s / M).abs() + A.abs() * ds / M + dB * xc.abs()
            + B.abs() * f["d_mean"])
    return dict(dx=dx, b_dx=b_dx, dgamma=q, b_dgamma=dq, dbeta=s, b_dbeta=ds, g=gy)


def bn_exact_stats(x, eps):
    """integer x [M, C] (float64 torch): mean, unbiased variance and 1/sqrt(var + eps) from exact integer sums -> float64 numpy"""
    M = x.shape[0]
    xi = x.to(torch.int64)
    sx, sxx = xi.sum(0).numpy().astype(object), (xi * xi).sum(0).numpy().astype(object)
    mean = np.array([float(a) / M for a in sx])
    num = [M * b - a * a for a, b in zip(sx, sxx)]  # python integers: exact
    var = np.array([float(n) / (float(M) * M) for n in num])
    unb = np.array([float(n) / (float(M) * (M - 1)) for n in num])
    return mean, var, unb, 1.0 / np.sqrt(var + float(np.float32(eps)))


def mc_reference(x, c0=C0_ULP):
    """x [S, bs, C]: the dtype-rounded logits of S samples accumulated in order (float64 numpy) -> dict of the packed statistics
    (sum_p, sum_p2 [bs, C], ent [bs]) and their bounds (b_sum_p, b_sum_p2, b_ent)"""
    u = REF32_UNIT
    x = np.asarray(x, dtype=np.float64)
    S, bs, C = x.shape
    chains = -(-C // 256)
    mx = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = mx - x
    fin = np.isfinite(d)
    e = np.where(fin, np.exp(-np.where(fin, d, 0.0)), 0.0)
    p = e / e.sum(-1, keepdims=True)
    rel = (np.where(fin, d, 0.0) + chains + c0) * 2.0 ** -23
    bp = np.where(fin, rel * p + (c0 + 1) * TINY32, 0.0)  # exp(-inf) = 0 exactly
    p2 = p * p
    bp2 = np.where(fin, 2 * p * bp + bp * bp + u * (p + bp) ** 2 + TINY32, 0.0)
    a = p + 1e-15
    L = np.log(a)
    ra = (bp + u * 1e-15) / a + u
    bL = ra / (1 - ra) + c0 * 2.0 ** -23 * np.abs(L)
    t = p * L
    bt = np.where(fin, bp * (np.abs(L) + bL) + p * bL + u * (np.abs(t) + bp * np.abs(L)) + TINY32, 0.0)
    ent = -t.sum(-1)
    b_ent = bt.sum(-1) + (chains + 9) * u * (np.abs(t) + bt).sum(-1)

    def acc(v, b):  # S additions into an f32 word: u32 times every running sum
        return v.sum(0), b.sum(0) + u * np.cumsum(np.abs(v) + b, axis=0).sum(0)
    out = {}
    out["sum_p"], out["b_sum_p"] = acc(p, bp)
    out["sum_p2"], out["b_sum_p2"] = acc(p2, bp2)
    out["ent"], out["b_ent"] = acc(ent, b_ent)
    out["p"], out["bp"] = p, bp
    return out


def kl_reference(mu, rho, pm, ps, g, c0=C0_ULP):
    """one item of btx_kl_gauss_model[_bwd] in float64 numpy: pm / ps scalars or arrays, g the upstream gradient ->
    (mean KL, dmu, b_dmu, drho, b_drho)"""
    u = REF32_UNIT
    mu, rho = np.asarray(mu, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    pm, ps = np.asarray(pm, dtype=np.float64), np.asarray(ps, dtype=np.float64)
    n = mu.size
    sig = np.logaddexp(0.0, rho)
    dsig = 1.0 / (1.0 + np.exp(-rho))
    kl = (np.log(ps) - np.log(sig) + (sig * sig + (mu - pm) ** 2) / (2 * ps * ps) - 0.5).sum() / n
    gn = float(g) / n
    dmu = gn * (mu - pm) / (ps * ps)
    drho = gn * (sig / (ps * ps) - 1.0 / sig) * dsig
    c1 = 12 + 2 * c0
    b_drho = (c1 * u + DELTA_W) * abs(gn) * (sig / (ps * ps) + 1.0 / sig) * dsig
    return kl, dmu, 8 * u * np.abs(dmu), drho, b_drho


def avgpool_exact(x, dtype):
    """global average pool of integer x [NB, HW, C] as the kernel spells it: f32(sum) * f32(1 / HW), then the store's rounding"""
    hw = x.shape[1]
    s = _np(x).sum(1).astype(np.float32)
    inv = np.float32(1.0) / np.float32(hw)
    return torch.from_numpy((s * inv).astype(np.float32)).to(dtype)


# =============================================================================================================================
# fused Bayesian LSTM (btx_lstm.hip, btx_lstm_bwd.hip): every step judged alone
# =============================================================================================================================
# The whole-sequence references of test_gpu_lstm_fused.py / test_gpu_lstm_train_fused.py re-derive the chain, so a bf16 rounding
# of h that flips feeds back and only a loose rel-L2 bar survives.  Here the reference of step t is fed with the GPU's OWN
# operands — the weights it sampled (read back by identity-impulse probes: x = I makes every gate pre-activation one product),
# its own h_{t-1} (hidden_seq[:, t-1]) and its own saved f32 cell state — so no operand term is left, in f32 and bf16 alike:
#
#   sampled weights   |w_gpu - (mu + sigma64 eps)| <= DELTA_W_LSTM (|mu| + |sigma eps|), eps / signs from materialize_noise(s + t)
#   gates             |got - ref| <= (K_i + K_h + 8) 2^-23 A,   A = the same sum on absolute values (accumulation only)
#   cell / hidden     c = f c' + i g,  h = o tanh c  from the saved gates and the saved c': with es = SIGM_ULP 2^-23 (the relative
#                     error of 1 / (1 + expf(-v))), et = TANH_ULP 2^-23 (tanhf), u = 2^-24 and three roundings per line
#                         b_c = (es + 3u) |f c'| + (es + et + 3u) |i g|
#                         b_h = (es + et + 3u) |o tanh c| + |o| b_c              (tanh' <= 1 carries the error of c into h)
#                     bf16 activations: store_rounding on top
#   backward          the same first-order calculus, carried by Err below: every product, sum and contraction adds its own
#                     roundings to the error it inherits; nothing is fitted.  Contractions: (len + 8) 2^-23 A plus the incoming
#                     error through |W|; len = 4H (recurrent term, dx, dh0), B (one step of a weight gradient), T (the sum over
#                     the steps).  drho multiplies by sigmoid(rho): one more sigm.  The eps the weight-gradient kernel
#                     regenerates is the hardware Box-Muller value, the reference's is materialize_noise's: DELTA_W_LSTM on eps_w,
#                     DELTA_B_LSTM on eps_b (the measured error of sigma eps bounds that of its factor eps).
#
# SIGM_ULP / TANH_ULP: twice the maximum error, in ulps of the result, of the device's 1 / (1 + expf(-v)) and tanhf against
# float64 (torch.sigmoid / torch.tanh on the GPU, the same math library; measured over the gate range of the test cases, never
# on the outputs of the kernels under test): profiles/lstm_envelope.txt
SIGM_ULP = 5.09  # measured 2.544 ulp (torch.sigmoid and the spelled-out expression alike), 5 M points on [-40, 40]
TANH_ULP = 2.72  # measured 1.359 ulp
# The LSTM's own sampled-weight constants, twice the maxima its probes measured.  DELTA_W is not widened: the Reparameterization
# probes (fl(mu + sigma eps) relative to |mu| + |sigma eps|) measured 3.73e-7, inside DELTA_W / 2.  The Flipout probes pass a
# zero mu and return Delta = sigma eps ALONE, so nothing dilutes the error of the hardware softplus times the hardware
# Box-Muller against float64 softplus times the materialised eps: 6.55e-7 relative to |sigma eps|, above DELTA_W / 2.  The
# bias (btx_softplus_fast / btx_normal1) measured 3.08e-7 (Reparameterization) and 5.59e-7 (Flipout, sigma_b eps_b alone).
DELTA_W_LSTM = 1.31e-6
DELTA_B_LSTM = 1.12e-6
LSTM_USEFUL = 1e-4  # a backward bound above this fraction of A (before any bf16 store) says nothing about the element


def rbf16(a):
    """float64 numpy of the values rounded to bf16 (the bits the kernels' own rounding gives)"""
    return torch.as_tensor(_np(a), dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def lstm_layer_step(mu, D=None, bm=None, bd=None, s_in=None, s_out=None):
    """one layer at one step as the kernel contracts it.  Reparameterization: mu = the sampled W = fl(mu + sigma eps), bm =
    fl(mu_b + sigma_b eps_b).  Flipout: mu, D = Delta, bm = mu_b, bd = sigma_b eps_b, s_in [B, K], s_out [B, 4H] (+-1)."""
    f = lambda t: None if t is None else _np(t)  # noqa: E731
    return dict(mu=f(mu), D=f(D), bm=f(bm), bd=f(bd), s_in=f(s_in), s_out=f(s_out))


def _lstm_round(L, bf16):
    if not bf16:
        return L
    return dict(L, mu=rbf16(L["mu"]), D=None if L["D"] is None else rbf16(L["D"]))


def lstm_linear64(inp, L, bf16):
    """inp [B, K] (or None: zeros) through one layer step -> (value, A) [B, 4H] float64"""
    L = _lstm_round(L, bf16)
    N = L["mu"].shape[0]
    if inp is None:
        v = a = 0.0
        B = None
    else:
        inp = rbf16(inp) if bf16 else _np(inp)
        B = inp.shape[0]
        v, a = inp @ L["mu"].T, np.abs(inp) @ np.abs(L["mu"]).T
    if L["D"] is not None and inp is not None:
        p, a = (inp * L["s_in"][:B]) @ L["D"].T, a + np.abs(inp) @ np.abs(L["D"]).T
    else:
        p = 0.0
    if L["bm"] is not None:
        v, a = v + L["bm"], a + np.abs(L["bm"])
    if L["bd"] is not None:
        p, a = p + L["bd"], a + np.abs(L["bd"])
    if L["D"] is not None or L["bd"] is not None:
        so = L["s_out"]
        v = v + p * (so if B is None else so[:B])
    return v, a


def lstm_gates64(x_t, h_prev, Li, Lh, bf16):
    """gate pre-activations of one step in float64 and their accumulation bound -> (ref, bound) [B, 4H]"""
    vi, ai = lstm_linear64(x_t, Li, bf16)
    vh, ah = lstm_linear64(h_prev, Lh, bf16)
    K = Li["mu"].shape[1] + Lh["mu"].shape[1]
    B = _np(x_t).shape[0]
    shape = (B, Li["mu"].shape[0])
    return np.broadcast_to(vi + vh, shape), np.broadcast_to((K + 8) * ACC_UNIT * (ai + ah), shape)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_cell64(gates, c_prev):
    """c_t, h_t in float64 from the (saved, f32) gate pre-activations [B, 4H] and c_{t-1} [B, H] -> (c, b_c, h, b_h)"""
    g4 = _np(gates)
    H = g4.shape[1] // 4
    cp = np.zeros((g4.shape[0], H)) if c_prev is None else _np(c_prev)
    with np.errstate(over="ignore"):
        i, f, g, o = _sig(g4[:, :H]), _sig(g4[:, H:2 * H]), np.tanh(g4[:, 2 * H:3 * H]), _sig(g4[:, 3 * H:])
    es, et, u = SIGM_ULP * ACC_UNIT, TANH_ULP * ACC_UNIT, REF32_UNIT
    c = f * cp + i * g
    b_c = (es + 3 * u) * np.abs(f * cp) + (es + et + 3 * u) * np.abs(i * g)
    h = o * np.tanh(c)
    b_h = (es + et + 3 * u) * np.abs(h) + np.abs(o) * b_c
    return c, b_c, h, b_h


class Err:
    """a float64 value with a bound on the error of its f32 counterpart; every operation adds one f32 rounding of its result
    (a fused multiply-add rounds less often: still inside)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = _np(v)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(_np(e), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def __mul__(self, o):
        o = Err.of(o)
        v = self.v * o.v
        e = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        return Err(v, e + REF32_UNIT * (np.abs(v) + e))

    def __add__(self, o):
        o = Err.of(o)
        e = self.e + o.e
        return Err(self.v + o.v, e + REF32_UNIT * (np.abs(self.v) + np.abs(o.v) + e))

    def __sub__(self, o):
        o = Err.of(o)
        return self + Err(-o.v, o.e)

    def abs(self):
        return Err(np.abs(self.v))

    @property
    def T(self):
        return Err(self.v.T, self.e.T)


def _err_sigm(v):
    with np.errstate(over="ignore"):
        s = _sig(_np(v))
    return Err(s, SIGM_ULP * ACC_UNIT * s)


def _err_tanh(v):
    t = np.tanh(_np(v))
    return Err(t, TANH_ULP * ACC_UNIT * np.abs(t))


def _err_matmul(a, b, length):
    """a [m, k] (Err) @ b [k, n] (exact): the incoming error through |b| and (length + 8) 2^-23 of the magnitudes"""
    ab = np.abs(b)
    return Err(a.v @ b, a.e @ ab + (length + 8) * ACC_UNIT * ((np.abs(a.v) + a.e) @ ab))


def _lstm_contract_T(dG, L, length):
    """dgates [B, 4H] . W -> [B, K]; Flipout: dG mu + s_in o ((dG o s_out) Delta)"""
    out = _err_matmul(dG, L["mu"], length)
    if L["D"] is not None:
        B = dG.v.shape[0]
        p = _err_matmul(Err(dG.v * L["s_out"][:B], dG.e), L["D"], length)
        out = out + Err(p.v * L["s_in"][:B], p.e)
    return out


def _chain_sum(terms, length):
    """sum of Err terms along one f32 chain of `length` additions"""
    v = sum(t.v for t in terms)
    e = sum(t.e for t in terms)
    return Err(v, e + (length + 8) * ACC_UNIT * sum(np.abs(t.v) + t.e for t in terms))


def lstm_bptt64(gates, cells, c0, Li, Lh, x, hs, h0, d_hs, d_cs, noise, rho, bf16, want_state=False, absolute=False):
    """backward through time in float64 from what the GPU saved (gates [T, B, 4H], cells [T, B, H]), the layer steps Li[t] /
    Lh[t] it sampled, its own hidden_seq [B, T, H] as the input of the hh weight gradient, and the given d_hs / d_cs [B, T, H]
    (or None).  noise = dict(ih=[(eps_w, eps_b | None)] per step, hh=...), rho = dict(ih=(rho_w, rho_b | None), hh=...).
    -> dict name -> Err: dx [B, T, I], dh0, dc0 (want_state), ih.dmu_w, ih.drho_w, ih.dmu_b, ih.drho_b, hh.* .
    absolute=True: the same chain on absolute values — the magnitudes A of every output (errors meaningless)."""
    gates, cells = _np(gates), _np(cells)
    T, B, N = gates.shape
    H = N // 4
    ab = (lambda a: np.abs(a)) if absolute else (lambda a: a)
    Li = [_lstm_round(L, bf16) for L in Li]
    Lh = [_lstm_round(L, bf16) for L in Lh]
    if absolute:
        def absL(L):
            one = lambda s: None if s is None else np.ones_like(s)  # noqa: E731
            return dict(mu=np.abs(L["mu"]), D=None if L["D"] is None else np.abs(L["D"]), s_in=one(L["s_in"]), s_out=one(L["s_out"]))
        Li, Lh = [absL(L) for L in Li], [absL(L) for L in Lh]
    x, hs = _np(x), _np(hs)
    xin = rbf16(x) if bf16 else x
    hin = rbf16(hs) if bf16 else hs
    h0in = None if h0 is None else (rbf16(h0) if bf16 else _np(h0))
    fx = (lambda e: e.abs()) if absolute else (lambda e: e)
    one = Err(1.0)
    dG, dcc = [None] * T, None
    for t in range(T - 1, -1, -1):
        g4 = gates[t]
        i, f, o = _err_sigm(g4[:, :H]), _err_sigm(g4[:, H:2 * H]), _err_sigm(g4[:, 3 * H:])
        g, th = _err_tanh(g4[:, 2 * H:3 * H]), _err_tanh(cells[t])
        cp = cells[t - 1] if t > 0 else (np.zeros((B, H)) if c0 is None else _np(c0))
        dth, di, df, dg, do = one - th * th, i * (one - i), f * (one - f), one - g * g, o * (one - o)
        g, th, cp = fx(g), fx(th), ab(cp)
        dh = Err(ab(_np(d_hs)[:, t])) if d_hs is not None else Err(np.zeros((B, H)))
        if t + 1 < T:
            dh = dh + _lstm_contract_T(dG[t + 1], Lh[t + 1], N)
        dc = dh * o * dth
        if d_cs is not None:
            dc = dc + Err(ab(_np(d_cs)[:, t]))
        if dcc is not None:
            dc = dc + dcc
        parts = [dc * g * di, dc * Err(cp) * df, dc * i * dg, dh * th * do]
        dG[t] = Err(np.concatenate([p.v for p in parts], 1), np.concatenate([p.e for p in parts], 1))
        dcc = dc * f
    out = {}
    dx = [_lstm_contract_T(dG[t], Li[t], N) for t in range(T)]
    out["dx"] = Err(np.stack([d.v for d in dx], 1), np.stack([d.e for d in dx], 1))
    if want_state:
        out["dh0"], out["dc0"] = _lstm_contract_T(dG[0], Lh[0], N), dcc
    for name, Ls in (("ih", Li), ("hh", Lh)):
        rho_w, rho_b = rho[name]
        dmu, se, bmu, bse = [], [], [], []
        for t in range(T):
            if name == "ih":
                inp = xin[:, t]
            else:
                inp = hin[:, t - 1] if t > 0 else (h0in if h0in is not None else np.zeros((B, H)))
            inp = ab(inp)
            L = Ls[t]
            eps_w, eps_b = noise[name][t]
            dW = _err_matmul(dG[t].T, inp, B)
            dmu.append(dW)
            dD = dW
            sg = dG[t]
            if L["D"] is not None or L["s_out"] is not None:
                sg = Err(dG[t].v * L["s_out"][:B], dG[t].e)
                dD = _err_matmul(sg.T, inp * L["s_in"][:B], B)
            ew = ab(_np(eps_w))
            se.append(dD * Err(ew, DELTA_W_LSTM * np.abs(ew)))
            if rho_b is not None:
                ones = np.ones((B, 1))
                bm, bd = _err_matmul(dG[t].T, ones, B), _err_matmul(sg.T, ones, B)
                eb = ab(_np(eps_b))
                bmu.append(Err(bm.v[:, 0], bm.e[:, 0]))
                bse.append(Err(bd.v[:, 0], bd.e[:, 0]) * Err(eb, DELTA_B_LSTM * np.abs(eb)))
        out[name + ".dmu_w"] = _chain_sum(dmu, T)
        out[name + ".drho_w"] = _chain_sum(se, T) * _err_sigm(rho_w)
        if rho_b is not None:
            out[name + ".dmu_b"] = _chain_sum(bmu, T)
            out[name + ".drho_b"] = _chain_sum(bse, T) * _err_sigm(rho_b)
    return out
