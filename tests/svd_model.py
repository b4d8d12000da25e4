"""BTX-SVD v1 in float64 numpy: the KL of a variational Gaussian against the log-uniform prior in the approximation of
Molchanov, Ashukha & Vetrov (2017, eq. 14), its analytic gradients, the log-alpha statistics and pruning, the true KL by quadrature,
perturbed references, and the f32 error envelope of the HIP kernels (plain module, like klmc_model.py).

    sigma = log1p(exp(rho))     la_raw = 2 log sigma - log(mu^2 + EPS)     la = clip(la_raw, -LA_MAX, LA_MAX)
    kl_i  = k1 - k1 sigmoid(k2 + k3 la) + 0.5 log1p(exp(-la))             kl = c sum_i kl_i, c = 1 / n ("mean") or 1 ("sum")
    d     = d kl_i / d la = -(k1 k3 s (1 - s) + 0.5 sigmoid(-la)), times 0 where la_raw lies STRICTLY outside [-LA_MAX, LA_MAX]
    dmu_i = g c d (-2 mu / (mu^2 + EPS))            drho_i = g c d (2 sigmoid(rho) / sigma)

ENVELOPE (bounds()).  The kernels (csrc/btx_svd.hip, built without FMA contraction) spell every step as one f32 operation, so the
bound is carried operation by operation with envelope.Err — a float64 value with a bound on the error of its f32 counterpart; every
product, sum and difference adds u = 2^-24 of its result to what it inherits.  What Err does not have is written here:

    constants   a decimal literal rounded to f32: u |c|  (k1 k3 is folded by the compiler from two rounded literals: 3 u)
    sigma       log1pf(expf(rho)) against float64: relative DW = envelope.DELTA_W (the measured f32 softplus)
    expf(x)     relative expm1(bound of x) + 2 c0 u          c0 = envelope.C0_ULP, the measured error of expf / logf in ulps
    logf(x)     r / (1 - r) + 2 c0 u |log x|, r = the relative bound of x
    1 / x       relative r / (1 - r) + u
    clamp       1-Lipschitz: the bound passes; 0 where la_raw is further outside than its own bound (the f32 value clamps too)
    gradients   where la_raw is within its bound of +-LA_MAX the f32 side may take the other branch of the select: bound + |value|
    value       the f32 terms are summed in f64 (n 2^-52 of sum |term|) and rounded to f32 once: + u |kl|

No constant is fitted: C0_ULP and DELTA_W are the measured ones of tests/envelope.py.  They are used here OUTSIDE the ranges they were
measured on, which is an extrapolation and not a measurement: C0_ULP comes from exp on [-104, 0] and log on [1e-38, 1], and is applied
to expf of arguments up to +32 (k2 + k3 LA_MAX) and to logf of arguments above 1 (1 + exp(-la) up to 4.9e8, sigma up to 4, mu^2 + EPS);
DELTA_W comes from rho in [-9, 2] and is applied to rho in [-12, 4].  The functions are the same library routines, whose relative error
does not depend on the sign of the result, and the GPU results use at most 0.47 of the bound (profiles/svd_envelope.txt); a
measurement of the three constants on the ranges used here has not been made.
"""
import math

import numpy as np

import envelope as E

EPS, LA_MAX, RHO_PRUNED = 1e-8, 20.0, -40.0
K1, K2, K3 = 0.63576, 1.87320, 1.48695
U32 = 2.0 ** -24
EULER_GAMMA = 0.57721566490153286061

# what a perturbed reference gets wrong; every one must fall outside whatever bound a comparison uses
VARIANTS = ("no_k1", "k2_sign", "no_half", "no_dsig", "no_two", "no_eps", "swap_reduction")


def sigma(rho):
    return np.logaddexp(0.0, np.asarray(rho, dtype=np.float64))


def _sigm(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def la_raw(mu, rho, variant=None):
    mu = np.asarray(mu, dtype=np.float64)
    eps = 0.0 if variant == "no_eps" else EPS
    with np.errstate(divide="ignore"):
        return 2.0 * np.log(sigma(rho)) - np.log(mu * mu + eps)


def clamp(raw):
    return np.clip(np.where(np.isnan(raw), -LA_MAX, raw), -LA_MAX, LA_MAX)


def log_alpha(mu, rho, variant=None):
    return clamp(la_raw(mu, rho, variant))


def kl_terms(la, variant=None):
    k2 = -K2 if variant == "k2_sign" else K2
    half = 1.0 if variant == "no_half" else 0.5
    k1c = 0.0 if variant == "no_k1" else K1
    return k1c - K1 * _sigm(k2 + K3 * la) + half * np.log1p(np.exp(-la))


def _c(n, reduction, variant=None):
    if reduction not in ("mean", "sum"):
        raise ValueError(reduction)
    if variant == "swap_reduction":
        reduction = "sum" if reduction == "mean" else "mean"
    return 1.0 / n if reduction == "mean" else 1.0


def kl(mu, rho, reduction="mean", variant=None):
    """one tensor's term c sum_i kl_i"""
    t = kl_terms(log_alpha(mu, rho, variant), variant)
    return float(t.sum() * _c(t.size, reduction, variant))


def grads(mu, rho, g=1.0, reduction="mean", variant=None):
    """analytic (dmu, drho) of g * kl(mu, rho)"""
    mu, rho = np.asarray(mu, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    raw = la_raw(mu, rho, variant)
    la = clamp(raw)
    k2 = -K2 if variant == "k2_sign" else K2
    half = 1.0 if variant == "no_half" else 0.5
    s = _sigm(k2 + K3 * la)
    d = -(K1 * K3 * s * (1.0 - s) + half * _sigm(-la))
    d = np.where((raw >= -LA_MAX) & (raw <= LA_MAX), d, 0.0)
    eps = 0.0 if variant == "no_eps" else EPS
    two = 1.0 if variant == "no_two" else 2.0
    dsig = 1.0 if variant == "no_dsig" else _sigm(rho)
    gc = float(g) * _c(mu.size, reduction, variant)
    with np.errstate(divide="ignore", invalid="ignore"):
        fmu = np.where(d == 0.0, 0.0, -two * mu / (mu * mu + eps))
        frho = np.where(d == 0.0, 0.0, 2.0 * dsig / sigma(rho))
    return gc * d * fmu, gc * d * frho


# ---- the true KL by quadrature ---------------------------------------------------------------------------------------------
def kl_quadrature(la, points=400001, lim=12.0):
    """KL(N(mu, alpha mu^2) || log-uniform) up to the prior's constant, fixed so that it vanishes as alpha -> inf:
    -KL = 0.5 la - E_eps log|1 + sqrt(alpha) eps| - (gamma + log 2) / 2, the expectation by the trapezoid rule on [-lim, lim]"""
    x = np.linspace(-lim, lim, points)
    phi = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    out = []
    for v in np.atleast_1d(np.asarray(la, dtype=np.float64)):
        with np.errstate(divide="ignore"):
            f = np.log(np.abs(1.0 + math.exp(0.5 * v) * x))
        f = np.where(np.isfinite(f), f, 0.0) * phi  # a grid point on the (integrable) log singularity: measure zero
        ex = float((f[:-1] + f[1:]).sum() * 0.5 * (x[1] - x[0]))
        out.append(-(0.5 * v - ex - 0.5 * (EULER_GAMMA + math.log(2.0))))
    return np.array(out)


# ---- statistics and pruning ---------------------------------------------------------------------------------------------------
def bin_index(la, bins):
    return np.minimum(bins - 1, np.floor((la + LA_MAX) * bins / (2.0 * LA_MAX)).astype(np.int64))


def stats(mu, rho, thresholds, bins=0):
    """-> dict(above=[count(la > t)], zero_mu, hist | None) of one tensor"""
    mu = np.asarray(mu, dtype=np.float64)
    la = log_alpha(mu, rho)
    return dict(above=[int((la > t).sum()) for t in thresholds], zero_mu=int((mu == 0).sum()),
                hist=np.bincount(bin_index(la, bins).reshape(-1), minlength=bins).tolist() if bins else None)


def prune_mask(mu, rho, threshold):
    return log_alpha(mu, rho) > threshold


def quarter_bin_inputs(n, seed, thresholds=(3.0,), bins=64, clamped=0.1, zeros=0.05):
    """(mu, rho) f32 arrays of n elements whose float64 log alpha lies at least a quarter bin (of `bins` equal bins over
    [-LA_MAX, LA_MAX]) from every bin edge, every threshold and both clamps — asserted here in float64 — so that f32 arithmetic, whose
    error in la is below 1e-4, must reproduce every count and every pruned index EXACTLY.  About `clamped` of the elements lie outside
    the clamp on either side, `zeros` of them have mu == 0 (which clamps high with the rho chosen)."""
    rng = np.random.default_rng(seed)
    width = 2.0 * LA_MAX / bins
    q = 0.25 * width
    target = np.empty(n)
    for i in range(n):
        while True:
            if rng.random() < clamped:
                v = (LA_MAX + 1.5 * q + rng.random() * 4.0) * (1.0 if rng.random() < 0.5 else -1.0)
            else:
                v = -LA_MAX + (rng.integers(bins) + 0.26 + 0.48 * rng.random()) * width
            if all(abs(v - t) >= 1.5 * q for t in thresholds):
                break
        target[i] = v
    zero = (rng.random(n) < zeros)
    target[zero] = LA_MAX + 2.0
    # sigma large enough for mu^2 = sigma^2 exp(-la) - EPS to stay positive: log sigma >= (la + log(4 EPS)) / 2
    logsig = np.maximum(rng.uniform(-6.0, 0.0, n), 0.5 * (target + math.log(4.0 * EPS)) + 0.1)
    logsig = np.where(zero, 0.5 * (target - math.log(1.0 / EPS)), logsig)  # mu = 0: la_raw = 2 log sigma - log EPS
    logsig = np.where(target < -LA_MAX, np.minimum(logsig, -4.0), logsig)
    sig = np.exp(logsig)
    rho = np.where(sig > 30.0, sig, np.log(np.expm1(np.minimum(sig, 30.0)))).astype(np.float32)
    sig = sigma(rho)
    mu2 = np.where(zero, 0.0, sig * sig * np.exp(-target) - EPS)
    assert (mu2 >= 0).all()
    mu = (np.sqrt(mu2) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    raw = la_raw(mu, rho)
    edges = -LA_MAX + width * np.arange(bins + 1)
    dist = np.abs(raw[:, None] - np.concatenate([edges, np.asarray(thresholds, dtype=np.float64)])[None, :]).min(1)
    assert np.isfinite(raw).all() and (dist >= q).all(), float(dist.min())
    assert (mu[zero] == 0).all() and (raw[zero] > LA_MAX + q).all()
    return mu, rho


# ---- the f32 envelope -----------------------------------------------------------------------------------------------------------
def _const(c, roundings=1):
    return E.Err(np.float64(c), roundings * U32 * abs(c))


def _neg(a):
    return E.Err(-a.v, a.e)


def _scale2(a, f):
    """times a power of two: exact"""
    return E.Err(f * a.v, abs(f) * a.e)


def _exp(a, c0):
    with np.errstate(over="ignore"):
        v = np.exp(a.v)
    return E.Err(v, v * (np.expm1(a.e) + 2 * c0 * U32))


def _log(a, c0):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(a.v)
        r = np.where(a.v > 0, a.e / a.v, 0.0)
    return E.Err(v, r / (1.0 - r) + 2 * c0 * U32 * np.abs(v))


def _recip(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 1.0 / a.v
        r = a.e / np.abs(a.v)
    return E.Err(v, np.abs(v) * (r / (1.0 - r) + U32))


def _chain_la(mu, rho, c0, dw):
    sig64 = sigma(rho)
    sig = E.Err(sig64, dw * sig64)
    m2 = E.Err(mu) * E.Err(mu) + _const(EPS)
    raw = _scale2(_log(sig, c0), 2.0) - _log(m2, c0)
    out = np.abs(raw.v) - LA_MAX  # > 0: outside the clamp
    la = E.Err(clamp(raw.v), np.where(out > raw.e, 0.0, raw.e))
    return sig, m2, raw, la, np.abs(out) <= raw.e


def bounds(mu, rho, g=1.0, reduction="mean", c0=E.C0_ULP, dw=E.DELTA_W):
    """one tensor (finite la_raw: rho where sigma neither underflows nor overflows) -> dict: term / b_term (per element, before c),
    kl / b_kl (the tensor's contribution and its bound, the final f32 rounding NOT included: value_bound adds it), dmu / b_dmu,
    drho / b_drho, near (elements whose la_raw is within its bound of a clamp)"""
    mu, rho = np.asarray(mu, dtype=np.float64).reshape(-1), np.asarray(rho, dtype=np.float64).reshape(-1)
    n = mu.size
    one = E.Err(np.ones(n))
    sig, m2, raw, la, near = _chain_la(mu, rho, c0, dw)
    s = _recip(one + _exp(_neg(_const(K2) + _const(K3) * la), c0))
    z = _exp(_neg(la), c0)
    term = (_const(K1) - _const(K1) * s) + _scale2(_log(one + z, c0), 0.5)
    ref = kl_terms(la.v)
    assert np.allclose(term.v, ref, rtol=0, atol=1e-12)
    c = _c(n, reduction)
    b_kl = c * float(term.e.sum()) + n * 2.0 ** -52 * c * float(np.abs(term.v).sum())
    # backward
    sn = _recip(one + _exp(la, c0))
    d = _neg(_const(K1 * K3, 3) * s * (one - s) + _scale2(sn, 0.5))
    dsig = _recip(one + _exp(E.Err(-rho), c0))
    gc = E.Err(np.float64(g)) if reduction == "sum" else E.Err(np.float64(g)) * _recip(E.Err(np.float64(n), U32 * n if n >= 2 ** 24 else 0.0))
    gmu = gc * (d * (E.Err(-2.0 * mu) * _recip(m2)))
    grho = gc * (d * (_scale2(dsig, 2.0) * _recip(sig)))
    passes = (raw.v >= -LA_MAX) & (raw.v <= LA_MAX)
    dmu, drho = np.where(passes, gmu.v, 0.0), np.where(passes, grho.v, 0.0)
    am, ar = grads(mu, rho, g, reduction)
    assert np.allclose(dmu, am, rtol=1e-12, atol=1e-300) and np.allclose(drho, ar, rtol=1e-12, atol=1e-300)
    b_dmu = np.where(near, gmu.e + np.abs(gmu.v), np.where(passes, gmu.e, 0.0))
    b_drho = np.where(near, grho.e + np.abs(grho.v), np.where(passes, grho.e, 0.0))
    return dict(term=term.v, b_term=term.e, kl=c * float(term.v.sum()), b_kl=b_kl, dmu=dmu, b_dmu=b_dmu, drho=drho, b_drho=b_drho,
                near=near, la=la.v, b_la=la.e)


def value_bound(kls, b_kls):
    """the bound of the f32 scalar a call returns for tensors with contributions kls and bounds b_kls: the f64 fold, one rounding"""
    total = float(np.sum(kls))
    return total, float(np.sum(b_kls)) + len(kls) * 2.0 ** -52 * float(np.sum(np.abs(kls))) + U32 * abs(total)
