"""BTX-OPT v1 in numpy: the parameter update of SGD / Adam / AdamW as a fixed sequence of operations, each rounded
once in `dtype`.  With dtype=float32 this is the DEFINITION the HIP kernels (csrc/btx_optim.hip) and the CPU path of
bayesian_torch_amd.optim are compared with bit for bit; with dtype=float64 it is compared with torch.optim (foreach=False) on float64
parameters, which shows that the order written here is torch's formula.  Scalars that the host derives (1 - beta, lr * wd, the bias
corrections) are computed in Python floats (double) and rounded to `dtype` once, as the device block of the kernels holds them."""
import math

import numpy as np

# the option combinations every test runs (momentum 0 / 0.9, Nesterov, dampening, coupled and decoupled decay, maximize)
SGD_CONFIGS = [
    dict(lr=0.05),
    dict(lr=0.05, momentum=0.9),
    dict(lr=0.05, momentum=0.9, nesterov=True),
    dict(lr=0.05, momentum=0.9, dampening=0.1),
    dict(lr=0.05, momentum=0.9, weight_decay=0.01),
    dict(lr=0.05, weight_decay=0.01, maximize=True),
    dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=0.01, maximize=True),
]
ADAM_CONFIGS = [
    ("Adam", dict(lr=0.01)),
    ("Adam", dict(lr=0.01, weight_decay=0.01)),
    ("Adam", dict(lr=0.01, weight_decay=0.01, maximize=True, betas=(0.8, 0.99), eps=1e-6)),
    ("AdamW", dict(lr=0.01)),
    ("AdamW", dict(lr=0.01, weight_decay=0.1, maximize=True)),
]


def clip_coef(total_norm, max_norm):
    """min(1, max_norm / (total_norm + 1e-6)) in float32, as btx_optim_grad_norm writes it"""
    f = np.float32
    c = f(max_norm) / (f(total_norm) + f(1e-6))
    return c if c < f(1.0) else f(1.0)


def _grad(g, p, dt, weight_decay, coupled, maximize, coef):
    if maximize:
        g = -g
    if coef is not None:
        g = g * dt(coef)
    if coupled and weight_decay != 0:
        g = g + dt(weight_decay) * p
    return g


def sgd_step(p, g, buf, dtype=np.float32, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False,
             coef=None):
    """one step on arrays of `dtype`; buf is None on a parameter's first step.  Returns (p, buf) (buf None when momentum == 0)."""
    dt = dtype
    g = _grad(g, p, dt, weight_decay, True, maximize, coef)
    if momentum != 0:
        if buf is None:
            buf = g.copy()
        else:
            buf = dt(momentum) * buf + dt(1.0 - dampening) * g
        g = g + dt(momentum) * buf if nesterov else buf
    p = p + dt(-lr) * g
    return p, (buf if momentum != 0 else None)


def adam_step(p, g, m, v, t, dtype=np.float32, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
              maximize=False, coef=None):
    """step number t (1 on the first step) on arrays of `dtype`; m, v start as zeros.  Returns (p, m, v)."""
    dt = dtype
    b1, b2 = betas
    g = _grad(g, p, dt, weight_decay, not decoupled, maximize, coef)
    if decoupled and weight_decay != 0:
        p = p * dt(1.0 - lr * weight_decay)
    step_size = lr / (1.0 - b1 ** t)
    bc2s = math.sqrt(1.0 - b2 ** t)
    m = m + dt(1.0 - b1) * (g - m)
    v = dt(b2) * v + (dt(1.0 - b2) * g) * g
    den = np.sqrt(v) / dt(bc2s) + dt(eps)
    p = p + (dt(-step_size) * m) / den
    return p, m, v
