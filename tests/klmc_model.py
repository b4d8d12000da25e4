"""Float64 model of BTX-KLMC v1: the sampled KL of a variational Gaussian against a non-Gaussian weight prior, its
analytic gradients, and the element-wise error envelope of the HIP unit (csrc/btx_klmc.hip).  No GPU, no package import.

    kl      = (1 / n) sum_i [ -log sigma_i - (1 + log 2 pi) / 2 - (1 / S) sum_j log p(mu_i + sigma_i eps_j[i]) ],  sigma = log1p(exp rho)
    dmu_i   = -(g / n) (1 / S) sum_j s(w_j[i])
    drho_i  =  (g / n) [ -1 / sigma_i - (1 / S) sum_j s(w_j[i]) eps_j[i] ] sigmoid(rho_i)

A prior is a tuple: ("mix2", pi, sigma1, sigma2) | ("laplace", b) | ("student", nu, t).  eps is EXPLICIT, [S, n] (the GPU tests feed
the materialised draws, the CPU tests the oracle's restatement of BTX-RNG v1).  `variant` spells the wrong estimators the tests must be
able to tell from the right one.

ENVELOPE (bounds(); u = 2^-24, c0 = envelope.C0_ULP: expf / logf err <= 2 c0 u relative; DW = envelope.DELTA_W: the f32 softplus).
Every constant is a count of roundings, written where it is used.  Where terms cancel the bound is on magnitudes.
  w      fl(mu + sig eps), sig carrying DW: |dw| <= DW |sig eps| + 2 u (|mu| + |sig eps|);  d = fl(w - loc): + u (|w| + |loc|)  =: bd
  log p  moves with d by at most Lip * bd, Lip a bound of |s| over [d - bd, d + bd]:
           mix2 (|d| + bd) max(1/s1^2, 1/s2^2);  laplace 1 / b;  student (nu + 1) / (2 t sqrt nu)
         and is evaluated with
           mix2     a = c0 - d^2 c2 (constants rounded: u each; square, product, difference): ba = u (2 |c0| + 4 d^2 c2), bb alike;
                    e = expf(-|a - b|) <= 1: be = e (ba + bb + u |a - b| + 2 c0 u);  L = logf(1 + e), 1 + e in [1, 2]: be + u + 2 c0 u L;
                    log p = max(a, b) + L:  ba + bb + be + u + 2 c0 u L + u (|max| + L)
           laplace  c - |d| / b: 3 u (|c| + |d| / b)
           student  c - h logf(1 + d^2 / (nu t^2)): the argument's three roundings cost 3 u in the log, logf 2 c0 u: h (3 u + 2 c0 u L) +
                    3 u (|c| + h L)
  term   -logf(sig) - C - (1/S) sum_j log p_j:  DW + (2 c0 + 2) u |log sig| + 2 u C + mean_j (b_logp_j) + (S + 3) u mean_j |log p_j|
         (the f32 chain over the draws: S additions; 1/S and its product; the final difference)
  value  the mean of the term bounds (the sum is f64, fixed order) + u |kl| for the f32 store (+ u (|kl| + |previous|) with KL_ACCUM)
  s      mix2     s = -d (ra / s1^2 + rb / s2^2): responsibilities abs err br = be + 3 u; the bracket moves with d by at most
                  (|d| + bd)^2 (1/s1^2 - 1/s2^2)^2 / 4 per unit d:  b_s = [max(1/s1^2, 1/s2^2) + (|d| + bd)^2 (1/s1^2 - 1/s2^2)^2 / 4] bd
                  + |d| br (1/s1^2 + 1/s2^2) + 6 u |s|
         laplace  -sign(d) / b: u / b, and 2 / b where |d| <= bd (the sign itself is not determined there)
         student  -(nu + 1) d / (nu t^2 + d^2): Lip (nu + 1) / (nu t^2), eight roundings: 8 u |s|
  dmu    -(g / n) (1/S) sum_j s_j:  |g / n| mean_j b_s_j + (S + 5) u |g / n| mean_j |s_j|
  drho   (g / n) [-1 / sig - (1/S) sum_j s_j eps_j] sig':  |g / n| sig' [(DW + 2 u) / sig + mean_j b_s_j |eps_j| + (S + 4) u mean_j |s_j eps_j|]
         + (2 c0 + 8) u |g / n| sig' (1 / sig + mean_j |s_j eps_j|)       (sig' = 1 / (1 + expf(-rho)): expf and three roundings)
"""
import math

import numpy as np
import torch

STREAM_EPS_W, STREAM_KL_W, STREAM_KL_B = 0, 5, 6
U32 = 2.0 ** -24
ENTROPY_C = 0.5 * (1.0 + math.log(2.0 * math.pi))

PRIORS = {
    "mix2": ("mix2", 0.25, 1.0, 0.05),
    "laplace": ("laplace", 0.3),
    "student": ("student", 3.0, 0.2),
}
VARIANTS = ("no_inv_s", "swap_sigmas", "no_sigmoid", "sampled_entropy")


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64))  # (a copy: never a read-only view)


def log_p(spec, d):
    """log p at d = w - loc, torch float64"""
    kind = spec[0]
    if kind == "mix2":
        _, pi, s1, s2 = spec
        a = math.log(pi) - math.log(s1) - d * d / (2.0 * s1 * s1)
        b = math.log1p(-pi) - math.log(s2) - d * d / (2.0 * s2 * s2)
        return torch.logaddexp(a, b) - 0.5 * math.log(2.0 * math.pi)
    if kind == "laplace":
        return -math.log(2.0 * spec[1]) - d.abs() / spec[1]
    if kind == "student":
        _, nu, t = spec
        c = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - math.log(t)
        return c - 0.5 * (nu + 1.0) * torch.log1p(d * d / (nu * t * t))
    if kind == "gauss":
        return -math.log(spec[1]) - 0.5 * math.log(2.0 * math.pi) - d * d / (2.0 * spec[1] ** 2)
    raise ValueError(kind)


def score(spec, d):
    """s = d log p / dw at d, torch float64 (written out, not differentiated)"""
    kind = spec[0]
    if kind == "mix2":
        _, pi, s1, s2 = spec
        a = math.log(pi) - math.log(s1) - d * d / (2.0 * s1 * s1)
        b = math.log1p(-pi) - math.log(s2) - d * d / (2.0 * s2 * s2)
        r1 = torch.sigmoid(a - b)
        return -d * (r1 / (s1 * s1) + (1.0 - r1) / (s2 * s2))
    if kind == "laplace":
        return -torch.sign(d) / spec[1]
    if kind == "student":
        _, nu, t = spec
        return -(nu + 1.0) * d / (nu * t * t + d * d)
    if kind == "gauss":
        return -d / spec[1] ** 2
    raise ValueError(kind)


def _spec(spec, variant):
    if variant == "swap_sigmas" and spec[0] == "mix2":
        return (spec[0], spec[1], spec[3], spec[2])
    return spec


def forward(mu, rho, eps, spec, loc=0.0, variant=None):
    """the estimate as a torch float64 scalar (differentiable w.r.t. mu / rho when they require grad); eps [S, n]"""
    mu, rho, eps, loc = _t(mu), _t(rho), _t(eps), _t(loc)
    spec = _spec(spec, variant)
    sig = torch.log1p(torch.exp(rho))
    w = mu.unsqueeze(0) + sig.unsqueeze(0) * eps
    lp = log_p(spec, w - loc).sum(0)
    if variant != "no_inv_s":
        lp = lp / eps.shape[0]
    if variant == "sampled_entropy":  # log q sampled as well: unbiased too, but another estimator
        ent = (-torch.log(sig).unsqueeze(0) - 0.5 * math.log(2.0 * math.pi) - 0.5 * eps * eps).mean(0)
    else:
        ent = -torch.log(sig) - ENTROPY_C
    return (ent - lp).mean()


def grads(mu, rho, eps, spec, loc=0.0, g=1.0, variant=None):
    """(dmu, drho), analytic, torch float64"""
    mu, rho, eps, loc = _t(mu), _t(rho), _t(eps), _t(loc)
    spec = _spec(spec, variant)
    n, S = mu.numel(), eps.shape[0]
    sig = torch.log1p(torch.exp(rho))
    s = score(spec, mu.unsqueeze(0) + sig.unsqueeze(0) * eps - loc)
    inv = 1.0 if variant == "no_inv_s" else 1.0 / S
    dsig = 1.0 if variant == "no_sigmoid" else torch.sigmoid(rho)
    gn = float(g) / n
    return -gn * inv * s.sum(0), gn * (-1.0 / sig - inv * (s * eps).sum(0)) * dsig


def bounds(mu, rho, eps, spec, loc=0.0, g=1.0, c0=3.77, dw=9.55e-7):
    """element-wise envelope of the HIP unit around the float64 model (derivation: the module docstring) ->
    dict(term, b_term, dmu, b_dmu, drho, b_drho), numpy float64 arrays of n elements"""
    u = U32
    mu, rho, eps = (np.asarray(a, dtype=np.float64) for a in (mu, rho, eps))
    loc = np.broadcast_to(np.asarray(loc, dtype=np.float64), mu.shape)
    n, S = mu.size, eps.shape[0]
    sig = np.logaddexp(0.0, rho)
    se = sig[None] * eps
    w = mu[None] + se
    d = w - loc[None]
    bd = dw * np.abs(se) + 2 * u * (np.abs(mu)[None] + np.abs(se)) + u * (np.abs(w) + np.abs(loc)[None])
    dt = torch.from_numpy(d)
    lp, s = log_p(spec, dt).numpy(), score(spec, dt).numpy()
    kind = spec[0]
    if kind == "mix2":
        _, pi, s1, s2 = spec
        i1, i2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
        ca = math.log(pi) - math.log(s1) - 0.5 * math.log(2 * math.pi)
        cb = math.log1p(-pi) - math.log(s2) - 0.5 * math.log(2 * math.pi)
        a, b = ca - d * d * i1 / 2, cb - d * d * i2 / 2
        ba, bb = u * (2 * abs(ca) + 2 * d * d * i1), u * (2 * abs(cb) + 2 * d * d * i2)
        e = np.exp(-np.abs(a - b))
        be = e * (ba + bb + u * np.abs(a - b) + 2 * c0 * u)
        L = np.log1p(e)
        b_lp = (np.abs(d) + bd) * max(i1, i2) * bd + ba + bb + be + u + 2 * c0 * u * L + u * (np.abs(np.maximum(a, b)) + L)
        br = be + 3 * u
        b_s = (max(i1, i2) + (np.abs(d) + bd) ** 2 * (i1 - i2) ** 2 / 4) * bd + np.abs(d) * br * (i1 + i2) + 6 * u * np.abs(s)
    elif kind == "laplace":
        bb_ = spec[1]
        b_lp = bd / bb_ + 3 * u * (abs(math.log(2 * bb_)) + np.abs(d) / bb_)
        b_s = u / bb_ + np.where(np.abs(d) <= bd, 2.0 / bb_, 0.0)
    else:
        _, nu, t = spec
        h = 0.5 * (nu + 1.0)
        c = math.lgamma(h) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - math.log(t)
        L = np.log1p(d * d / (nu * t * t))
        b_lp = (nu + 1.0) / (2 * t * math.sqrt(nu)) * bd + h * (3 * u + 2 * c0 * u * L) + 3 * u * (abs(c) + h * L)
        b_s = (nu + 1.0) / (nu * t * t) * bd + 8 * u * np.abs(s)
    term = -np.log(sig) - ENTROPY_C - lp.mean(0)
    b_term = dw + (2 * c0 + 2) * u * np.abs(np.log(sig)) + 2 * u * ENTROPY_C + b_lp.mean(0) + (S + 3) * u * np.abs(lp).mean(0)
    gn = abs(float(g)) / n
    dsig = 1.0 / (1.0 + np.exp(-rho))
    dmu, drho = (t_.numpy() for t_ in grads(mu, rho, eps, spec, loc, g))
    b_dmu = gn * b_s.mean(0) + (S + 5) * u * gn * np.abs(s).mean(0)
    sz = np.abs(s * eps).mean(0)
    b_drho = gn * dsig * ((dw + 2 * u) / sig + (b_s * np.abs(eps)).mean(0) + (S + 4) * u * sz) + (2 * c0 + 8) * u * gn * dsig * (1.0 / sig + sz)
    return dict(term=term, b_term=b_term, dmu=dmu, b_dmu=b_dmu, drho=drho, b_drho=b_drho)


def value_bound(b_term, kl, previous=None):
    """bound of the f32 value of one tensor: the mean of the term bounds and the store's rounding (KL_ACCUM: the f32 addition too)"""
    b = float(np.mean(b_term)) + U32 * abs(kl)
    if previous is not None:
        b += U32 * (abs(kl) + abs(previous) + abs(kl + previous))
    return b


# ---- closed forms the unbiasedness checks compare with ------------------------------------------------------------------------
def gauss_kl_mean(mu, rho, pm, ps):
    """the closed-form mean KL(N(mu, sig^2) || N(pm, ps^2)), numpy float64"""
    mu, rho = np.asarray(mu, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    sig = np.logaddexp(0.0, rho)
    return float((math.log(ps) - np.log(sig) + (sig * sig + (mu - pm) ** 2) / (2 * ps * ps) - 0.5).mean())


def gauss_se(mu, rho, pm, ps, S):
    """standard error of the estimate against a Gaussian prior: the cross term is d^2 / (2 ps^2) + const with d ~ N(mu - pm, sig^2),
    Var d^2 = 2 sig^4 + 4 sig^2 (mu - pm)^2;  SE^2 = sum_i (2 sig^4 + 4 sig^2 mu^2) / (4 ps^4) / (n^2 S)"""
    mu, rho = np.asarray(mu, dtype=np.float64) - pm, np.asarray(rho, dtype=np.float64)
    sig = np.logaddexp(0.0, rho)
    return math.sqrt(float(((2 * sig ** 4 + 4 * sig ** 2 * mu ** 2) / (4 * ps ** 4)).sum()) / (mu.size ** 2 * S))


def laplace_kl_mean(mu, rho, m, b):
    """closed form against Laplace(m, b): E|w - m| of a normal is the folded-normal mean
    sig sqrt(2 / pi) exp(-dm^2 / (2 sig^2)) + dm (1 - 2 Phi(-dm / sig))"""
    mu, rho = np.asarray(mu, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    sig = np.logaddexp(0.0, rho)
    dm = mu - m
    phi = 0.5 * (1.0 + np.vectorize(math.erf)(-dm / sig / math.sqrt(2.0)))
    folded = sig * math.sqrt(2.0 / math.pi) * np.exp(-dm * dm / (2 * sig * sig)) + dm * (1.0 - 2.0 * phi)
    return float((-np.log(sig) - ENTROPY_C + math.log(2 * b) + folded / b).mean())


def laplace_se(rho, b, S):
    """upper bound of the standard error: Var|d| <= Var d = sig^2"""
    sig = np.logaddexp(0.0, np.asarray(rho, dtype=np.float64))
    return math.sqrt(float((sig * sig).sum()) / (b * b) / (sig.size ** 2 * S))


def case(n, S, seed=None):
    """the inputs of the unbiasedness checks: mu ~ N(0, 0.1), rho ~ U(-6, 0.5) from RandomState(n + S)"""
    r = np.random.RandomState(n + S if seed is None else seed)
    return 0.1 * r.randn(n), r.uniform(-6.0, 0.5, n)


def oracle_eps(n, S, seed, sample, layer, stream):
    """[S, n] draws through the oracle's CPU restatement of BTX-RNG v1: draw j at stream | j << 8"""
    from oracle import bt_oracle as o
    return np.stack([o.eps(n, seed, sample, layer, stream | (j << 8)) for j in range(S)]).astype(np.float64)
