"""BTX-REG v1 in numpy: the definition the CPU paths are compared with bit for bit, the input generators shared by
tests/test_reg_cpu.py and tests/test_gpu_reg.py, and the rounding envelope of the Gaussian NLL head (plain module, like envelope.py).

MODEL.  Everything is float64 numpy, IEEE operations one at a time, so the torch float64 CPU paths and the f64 kernels compute the same
bits.  The two f32 transcendentals are DEFINED as the float64 function rounded once to f32 (expf32, logf32): the correctly rounded
value, whatever a host's or a device's f32 library returns; a device result differs from it by the library's error, which the
envelopes below carry as C_EXP_ULP / C_LOG_ULP.

ENVELOPE of the head (gnll_reference).  The kernel evaluates every element in f32, each operation rounded once; the reference is the
same expression in float64.  The bound is propagated operation by operation with envelope.Err (first-order calculus on absolute
values: a product, a sum or a quotient inherits its operands' errors and adds 2^-24 of its own magnitude), plus
  expf   exp(v) expm1(e) for an argument error e, and C_EXP_ULP 2^-23 of the result
  logf   e / (v - e) for an argument error e, and C_LOG_ULP 2^-23 of the result (+ 2^-149)
Terms widen to double and are added in double: N 2^-53 of the sum of magnitudes, then the division and ONE rounding of the loss to f32.
A bf16 gradient is rounded once more on store (envelope.store_rounding).  Nothing is fitted.

C_EXP_ULP / C_LOG_ULP: envelope.C0_ULP was measured on exp over [-104, 0] and log over [1e-38, 1] only; this head evaluates exp on
[-3, 3] (and sums of them) and log on sums of variances.  tools/reg_envelope.py measures torch.exp on [-8, 8] and torch.log on
[2^-12, 2^12] (f32, 4 M points each, the device's math library) against float64 on an MI355X; the constants are 2 x the measured
maxima, the project's rule: profiles/reg_envelope.txt.
"""
import math

import numpy as np
import torch

from envelope import REF32_UNIT, TINY32, Err, rbf16, store_rounding, ulp32

# 2 x the maxima tools/reg_envelope.py measured on an MI355X (profiles/reg_envelope.txt): exp 0.837 ulp at x = -3.2058, log 1.880 ulp
# at x = 977.43
C_EXP_ULP = 1.68
C_LOG_ULP = 3.76
CHUNK = 4096
HEADER, CURSOR, DROPPED, SUMS = 16, 9, 10, 9
TWO_PI = 6.283185307179586
USEFUL = 1e-4  # a bound (before any bf16 store) above this fraction of |ref| + mean|ref| says nothing about the element


def expf32(s):
    """the model's expf: exp in float64 rounded once to f32, as float64"""
    return np.exp(np.asarray(s, dtype=np.float64)).astype(np.float32).astype(np.float64)


def logf32(x):
    return np.log(np.asarray(x, dtype=np.float64)).astype(np.float32).astype(np.float64)


# ---- 1. MC moment statistics ------------------------------------------------------------------------------------------------
def numel(bs, D):
    return 3 * bs * D + 2


def accumulate_lanes(packed, out, lanes, D, has_var, kl=0.0):
    """packed (float64, in place) += `lanes` samples of out [lanes * bs, W] (float32 values), folded in order"""
    out = np.asarray(out, dtype=np.float32)
    bs = out.shape[0] // lanes
    N = bs * D
    for k in range(lanes):
        o = out[k * bs:(k + 1) * bs].astype(np.float64)
        m = o[:, :D].reshape(-1)
        packed[:N] += m
        packed[N:2 * N] += m * m
        if has_var:
            packed[2 * N:3 * N] += expf32(o[:, D:2 * D]).reshape(-1)
        packed[3 * N] += float(kl)
        packed[3 * N + 1] += 1.0
    return packed


def unpack(packed, bs):
    N = (packed.size - 2) // 3
    D = N // bs
    n = packed[3 * N + 1]
    mean = (packed[:N] / n).reshape(bs, D)
    ep = np.maximum((packed[N:2 * N] / n).reshape(bs, D) - mean * mean, 0.0)
    al = (packed[2 * N:3 * N] / n).reshape(bs, D)
    return dict(mean=mean, epistemic_var=ep, aleatoric_var=al, total_var=ep + al, kl=packed[3 * N] / n, samples=n)


# ---- summation order --------------------------------------------------------------------------------------------------------
def _butterfly(a):
    """xor butterfly over the last axis (64 lanes): lane 0's value"""
    for off in (32, 16, 8, 4, 2, 1):
        a = a[..., :off] + a[..., off:2 * off]
    return a[..., 0]


def chunk_fold_sum(v):
    """v [Q, N] float64 -> [Q]: a 256-thread workgroup per chunk of 4096 elements, thread t adding e = t, t + 256, ... in order from
    zero, a butterfly per wave, (w0 + w1) + (w2 + w3); then ONE wave over the chunks: lane l adds l, l + 64, ..., and a butterfly"""
    v = np.asarray(v, dtype=np.float64)
    Q, N = v.shape
    nch = -(-N // CHUNK)
    pad = np.zeros((Q, nch * CHUNK))
    pad[:, :N] = v
    w = pad.reshape(Q, nch, CHUNK // 256, 256)
    acc = np.zeros((Q, nch, 256))
    for j in range(w.shape[2]):
        acc = acc + w[:, :, j]
    wv = _butterfly(acc.reshape(Q, nch, 4, 64))
    part = (wv[..., 0] + wv[..., 1]) + (wv[..., 2] + wv[..., 3])
    k = -(-nch // 64)
    pad = np.zeros((Q, k * 64))
    pad[:, :nch] = part
    w = pad.reshape(Q, k, 64)
    acc = np.zeros((Q, 64))
    for j in range(k):
        acc = acc + w[:, j]
    return _butterfly(acc)


# ---- 3. evaluation ----------------------------------------------------------------------------------------------------------
def z2_of(levels):
    """z_k^2, z_k = sqrt(2) erfinv(level_k), float64"""
    lv = torch.as_tensor(np.asarray(levels, dtype=np.float64))
    z = 2.0 ** 0.5 * torch.erfinv(lv)
    return (z * z).numpy()


def new_state(K):
    return np.zeros(HEADER + K)


def eval_elements(packed, target, noise_var=None, min_var=1e-12):
    """per element: dict of float64 arrays [N] (ok, mean, ep, al, var, err, e2, nll, y)"""
    y32 = np.asarray(target, dtype=np.float32).reshape(-1)
    N = y32.size
    y = y32.astype(np.float64)
    n = packed[3 * N + 1]
    mean = packed[:N] / n
    ep = np.maximum(packed[N:2 * N] / n - mean * mean, 0.0)
    al = packed[2 * N:3 * N] / n + (0.0 if noise_var is None else float(noise_var))
    var = np.maximum(ep + al, float(min_var))
    err = y - mean
    e2 = err * err
    nll = 0.5 * (logf32((TWO_PI * var).astype(np.float32)) + e2 / var)
    return dict(ok=~np.isnan(y), mean=mean, ep=ep, al=al, var=var, err=err, e2=e2, nll=nll, y=y)


def eval_rows(el, z2):
    """the Q = 9 + K rows the state sums, ignored elements at 0"""
    ok = el["ok"]
    z = np.zeros_like(el["y"])
    rows = [ok.astype(np.float64), (~ok).astype(np.float64)]
    with np.errstate(invalid="ignore"):
        rows += [np.where(ok, t, z) for t in (el["e2"], np.abs(el["err"]), el["nll"], el["ep"], el["al"], el["y"], el["y"] * el["y"])]
        rows += [(ok & (el["e2"] <= zk * el["var"])).astype(np.float64) for zk in z2]
    return np.stack(rows)


def eval_update(state, packed, target, z2, noise_var=None, min_var=1e-12, records=None):
    """state (in place) += one batch; records [capacity, 4] float32 (in place) or None -> the element dict"""
    el = eval_elements(packed, target, noise_var, min_var)
    N, K = el["y"].size, len(z2)
    s = chunk_fold_sum(eval_rows(el, z2))
    cur = state[CURSOR]
    cap = 0 if records is None else records.shape[0]
    if cap:
        at = int(cur) + np.arange(N)
        keep = at < cap
        records[at[keep]] = np.stack([el["mean"], el["ep"], el["al"], el["err"]], 1).astype(np.float32)[keep]
    state[:SUMS] += s[:SUMS]
    state[HEADER:HEADER + K] += s[SUMS:]
    state[DROPPED] += min(max(cur + N - cap, 0.0), float(N))
    state[CURSOR] = cur + N
    return el


LEVELS = {1: (0.9,), 4: (0.5, 0.8, 0.9, 0.95), 8: (0.1, 0.25, 0.5, 0.68, 0.8, 0.9, 0.95, 0.99)}
MARGIN = 1e-9


def coverage_margin(el, z2):
    """the smallest relative margin |err^2 - z^2 var| / (z^2 var) of a coverage decision over the valid elements"""
    ok = el["ok"]
    return min(float((np.abs(el["e2"][ok] - zk * el["var"][ok]) / (zk * el["var"][ok])).min()) for zk in z2)


def eval_case(bs, D, K, seed, samples=5, nan_frac=0.1, variance="log"):
    """outputs of `samples` MC samples [samples * bs, W] f32, targets [bs, D] f32 with about nan_frac NaN, the levels, and the model's
    packed vector.  Asserts BEFORE use that every coverage decision has a relative margin of at least MARGIN, so that a last-bit
    difference cannot flip one."""
    r = np.random.RandomState(seed)
    W = 2 * D if variance == "log" else D
    out = r.randn(samples * bs, W).astype(np.float32)
    if variance == "log":
        out[:, D:] = r.uniform(-3, 1, (samples * bs, D)).astype(np.float32)
    out[:, :D] += 3.0 * r.randn(1, D).astype(np.float32)  # un-standardised means
    y = (out[:bs, :D] + 1.5 * r.randn(bs, D)).astype(np.float32)
    y[r.rand(bs, D) < nan_frac] = np.nan
    if not np.isnan(y).any():
        y.reshape(-1)[-1] = np.nan
    y.reshape(-1)[0] = 0.25  # (never all ignored)
    packed = accumulate_lanes(np.zeros(numel(bs, D)), out, samples, D, variance == "log", kl=1.5)
    levels = LEVELS[K]
    noise_var = None if variance == "log" else 0.5
    el = eval_elements(packed, y, noise_var)
    assert coverage_margin(el, z2_of(levels)) >= MARGIN
    return dict(out=out, y=y, levels=levels, packed=packed, samples=samples, noise_var=noise_var, bs=bs, D=D)


def eval_case_ints(bs, D, seed, samples=4):
    """small integers: n a power of two, integer m and y, variance=None with noise_var = 0.5 — every per-element value and every sum
    is exact in float64, so the sums are bit-equal in ANY order"""
    r = np.random.RandomState(seed)
    out = r.randint(-4, 5, (samples * bs, D)).astype(np.float32)
    y = r.randint(-6, 7, (bs, D)).astype(np.float32)
    y[r.rand(bs, D) < 0.1] = np.nan
    y.reshape(-1)[0] = 1.0
    packed = accumulate_lanes(np.zeros(numel(bs, D)), out, samples, D, False)
    return dict(out=out, y=y, levels=LEVELS[4], packed=packed, samples=samples, noise_var=0.5, bs=bs, D=D)


# ---- 2. the Gaussian NLL head: inputs, float64 reference and envelope -------------------------------------------------------
HEAD_SHAPES = [(1, 1, 1), (2, 3, 1), (4, 7, 5), (32, 2, 3), (2, 3, 1366), (1, 65, 4097)]
KL = 3.25
NOISE_VAR = 0.3


def head_case(S, B, D, bf16=False, variance="log", seed=0):
    """m, y ~ N(0, 1), s ~ U[-3, 3]; the stack holds the dtype-rounded values (float32 numpy) -> (stack [S, B, W], y [B, D])"""
    r = np.random.RandomState(1000 * S + 10 * B + D + seed)
    m = r.randn(S, B, D)
    y = r.randn(B, D).astype(np.float32)
    st = np.concatenate([m, r.uniform(-3, 3, (S, B, D))], -1) if variance == "log" else m
    st = st.astype(np.float32)
    if bf16:
        st = rbf16(st).astype(np.float32)
    return st, y


def _err_exp(x):
    v = np.exp(x.v)
    E = v * np.expm1(x.e)
    return Err(v, E + C_EXP_ULP * 2.0 ** -23 * (v + E) + TINY32)


def _err_log(x):
    v = np.log(x.v)
    arg = x.e / np.maximum(x.v - x.e, 1e-300)
    return Err(v, arg + C_LOG_ULP * 2.0 ** -23 * (np.abs(v) + arg) + TINY32)


def _err_div(a, b):
    v = a.v / b.v
    e = (a.e + np.abs(v) * b.e) / np.maximum(np.abs(b.v) - b.e, 1e-300)
    return Err(v, e + REF32_UNIT * (np.abs(v) + e))


def _neg(a):
    return Err(-a.v, a.e)


def _moments(m, lv, S):
    sm, sv = Err(np.zeros_like(m[0].v)), Err(np.zeros_like(m[0].v))
    ex = [_err_exp(lv[s]) for s in range(S)]
    for s in range(S):
        sm, sv = sm + m[s], sv + ex[s]
    fS = Err(float(S))
    mb = _err_div(sm, fS)
    se = Err(np.zeros_like(mb.v))
    c = [m[s] - mb for s in range(S)]
    for s in range(S):
        se = se + c[s] * c[s]
    return mb, _err_div(sv, fS) + _err_div(se, fS), c, ex


def gnll_reference(stack, y, reduce, variance="log", noise_var=None, full=False, kl=None, g=1.0, store_bf16=False):
    """float64 value and bound of the loss and of every gradient element, from the f32 operation sequence of csrc/btx_reg.hip ->
    dict(loss, b_loss, grad [S, B, W], b_grad (with the bf16 store when store_bf16), b_pre (before it))"""
    st = np.asarray(stack, dtype=np.float64)
    S, B, W = st.shape
    has_var = variance == "log"
    D = W // 2 if has_var else W
    N = B * D
    yy = Err(np.asarray(y, dtype=np.float64).reshape(B, D))
    m = [Err(st[s, :, :D]) for s in range(S)]
    if has_var:
        lv = [Err(st[s, :, D:]) for s in range(S)]
    else:
        l0 = math.log(noise_var)  # the kernel's logf(noise_var): the library's error and the rounding of noise_var to f32
        lv = [Err(np.full((B, D), l0), (C_LOG_ULP * 2.0 ** -23 + REF32_UNIT) * abs(l0) + REF32_UNIT + TINY32)] * S
    half, one, gg = Err(0.5), Err(1.0), Err(float(g))
    k = _err_div(one, Err(float(S)) * Err(float(B)))
    dm, ds = [None] * S, [None] * S
    if reduce == "loss":
        term = np.zeros((B, D))
        b_term = np.zeros((B, D))
        for s in range(S):
            r = yy - m[s]
            iv = _err_exp(_neg(lv[s]))
            t = half * (lv[s] + (r * r) * iv)
            term, b_term = term + t.v, b_term + t.e
            dm[s] = gg * (_neg(r * iv) * k)
            ds[s] = gg * ((half * (one - (r * r) * iv)) * k)
        div = float(S * B)
    else:
        mb, vb, c, ex = _moments(m, lv, S)
        r = yy - mb
        t = half * (_err_log(vb) + _err_div(r * r, vb))
        term, b_term = t.v, t.e
        a = _err_div(one, vb) - _err_div(r * r, vb * vb)
        c0 = _neg(_err_div(r, vb))
        for s in range(S):
            dm[s] = gg * ((c0 + c[s] * a) * k)
            ds[s] = gg * (((half * ex[s]) * a) * k)
        div = float(B)
    loss = term.sum() / div
    b_loss = (b_term.sum() + N * 2.0 ** -53 * (np.abs(term).sum() + b_term.sum())) / div
    if full:
        loss += 0.5 * math.log(2 * math.pi) * D
    if kl is not None:
        loss += float(kl) / B
    b_loss += REF32_UNIT * (abs(loss) + b_loss)
    parts = [np.stack([d.v for d in dm])] + ([np.stack([d.v for d in ds])] if has_var else [])
    bnds = [np.stack([d.e for d in dm])] + ([np.stack([d.e for d in ds])] if has_var else [])
    grad, b_pre = np.concatenate(parts, -1), np.concatenate(bnds, -1)
    b_grad = store_rounding(b_pre, grad) if store_bf16 else b_pre
    return dict(loss=loss, b_loss=b_loss, grad=grad, b_grad=b_grad, b_pre=b_pre)


def moments_grad_closed_form(stack, y):
    """the closed form of the reduce="moments" gradients (variance="log"), float64: r = y - mbar, a = 1 / vbar - r^2 / vbar^2,
    d / d m_s = (-r / vbar + (m_s - mbar) a) / (S B),  d / d s_s = 0.5 exp(s_s) a / (S B)"""
    st = np.asarray(stack, dtype=np.float64)
    S, B, W = st.shape
    D = W // 2
    m, s = st[..., :D], st[..., D:]
    mb = m.mean(0)
    vb = np.exp(s).mean(0) + ((m - mb) ** 2).mean(0)
    r = np.asarray(y, dtype=np.float64).reshape(B, D) - mb
    a = 1.0 / vb - r * r / (vb * vb)
    return np.concatenate([(-r / vb + (m - mb) * a) / (S * B), 0.5 * np.exp(s) * a / (S * B)], -1)
