"""Shared cases, float64 references and scenarios of the autograd-contract tests (DESIGN.md "Autograd contract").  No test functions.

The numerical files drive every torch.autograd.Function of bayesian_torch_amd/autograd.py one way: fresh layer, one forward at a pinned
sample, everything requires a gradient, one dense backward.  The scenarios here call the SAME Functions the ways autograd calls them
in real training code — subsets of needs_input_grad, a second forward before the first backward, a seed change in between, retained
graphs, accumulation, a layer applied twice, activation checkpointing — and are written against a duck-typed layer (`_w()`, `mu_bias`,
`rho_bias`, `_btx_layer_id`, `_btx_sample`), so that tests/test_autograd_contract_cpu.py can run them against a stand-in with planted
faults and tests/test_gpu_autograd_contract.py against the HIP layers.

Two comparison rules, and only these two:
  bits      envelope.check_exact: two calls on the same operands that must run the same launches
  envelope  envelope.check against float64 on the CPU with the bounds envelope.py derives (bound, dgrad_A, wgrad_A); the sum of two
            calls' gradients gets the sum of the two bounds plus 2^-24 |sum| for the one f32 add.  No constants of its own.

Moved here from tests/test_gpu_elementwise.py (which imports them back, unchanged): dev, make, Log, grads64, scaled.
"""
import itertools

import numpy as np
import torch

import envelope as E
from test_gpu_backward import CASES as BWD_CASES, _op_of as op_of

SAMPLE = 5
NAMES = ("x", "mu", "rho", "mu_b", "rho_b")
F32, BF16 = torch.float32, torch.bfloat16


# =============================================================================================================================
# helpers shared with tests/test_gpu_elementwise.py
# =============================================================================================================================
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def make(cls, kw, prec, seed=3, bt_seed=2024):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(bt_seed)
    torch.manual_seed(seed)
    layer = getattr(L, cls)(**kw).to(dev())
    layer.precision = prec
    bt.assign_layer_ids(layer)  # the noise is keyed on the layer id: alone or inside the whole suite, a case sees the same noise
    return layer


class Log:
    """collects the failures of a loop over cases so that ONE run names every bad element"""

    def __init__(self):
        self.bad = []

    def check(self, name, prec, got, ref, bnd):
        rep = E.check(got, ref, bnd)
        print(rep.line(name, prec))
        if not rep.ok:
            self.bad.append("%s %s: %s" % (name, prec, rep))
        return rep

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def grads64(layer, x, dy, sample, weights=True):
    """float64 autograd through the reference chain on the CPU: (dx, dmu, A_dx, ddelta, noise)"""
    with torch.no_grad():
        nz = layer.materialize_noise(sample, tuple(x.shape), tuple(dy.shape), x.dtype)
    mu, rho = layer._w()
    op = op_of(layer)
    flip = layer._family == "flipout"
    x64 = E.d64(x).requires_grad_(True)
    mu64 = E.d64(mu).requires_grad_(True)
    delta64 = (E.sigma64(rho) * E.d64(nz["eps_w"])).requires_grad_(True)
    if flip:
        ref = E.contract(x64, mu64, None, op) + E.contract(x64 * E.d64(nz["sign_in"].reshape(x.shape)), delta64, None, op) \
            * E.d64(nz["sign_out"].reshape(dy.shape))
    else:
        ref = E.contract(x64, mu64 + delta64, None, op)
    if weights:
        dx, dmu, ddelta = torch.autograd.grad(ref, (x64, mu64, delta64), E.d64(dy))
    else:
        (dx,), dmu, ddelta = torch.autograd.grad(ref, (x64,), E.d64(dy)), None, None
    A = E.dgrad_A(dy, tuple(x.shape), E.abs_weight(mu, rho, nz["eps_w"]), op)
    return dx, dmu, A, ddelta, nz


def scaled(b_dw, ref_dw, factor):
    """bound of dW * eps * sigmoid(rho) formed in f32 from a dW with bound b_dw: |factor| scales it, the two products and the
    hardware sigmoid add relative roundings to the result"""
    f = E._np(factor)
    return b_dw * abs(f) + (E.DELTA_W + 4 * E.REF32_UNIT) * (abs(E._np(ref_dw)) + b_dw) * abs(f)


# =============================================================================================================================
# the cases: the smallest shapes that keep each one on the branch of ContractFn.backward / _data_grad_hip it is meant to reach
# =============================================================================================================================
class Case:
    def __init__(self, cid, cls, kw, xshape, why, pre):
        self.id, self.cls, self.kw, self.xshape, self.why, self.pre = cid, cls, kw, tuple(xshape), why, pre

    def check_precondition(self, layer, x):
        assert self.pre(layer, x), "%s is no longer on its branch: %s" % (self.id, self.why)


def _ag():
    from bayesian_torch_amd import autograd
    return autograd


def _outpad(layer, x):
    op = layer._op
    return tuple((i + 2 * p - d * (k - 1) - 1) % s for i, p, d, k, s in
                 zip(x.shape[2:], op.padding[1:], op.dilation[1:], op.kernel[1:], op.stride[1:]))


def _lrt_ok(layer, x):
    from bayesian_torch_amd import functional as BF
    return BF.lrt_train_ok(layer, x.detach().requires_grad_(True)) == bool(layer.fused_training)


_C4_CLS, _C4_KW, _ = BWD_CASES[8]
assert _C4_CLS == "Conv2dFlipout" and _C4_KW["kernel_size"] == 3 and _C4_KW["in_channels"] == 24
# The 24-channel convolution test_gpu_backward.CASES labels "channel-padded" is NOT padded under today's rule (in_channels % 8 != 0):
# C4 keeps its geometry at 20 input channels (padded to 24), so that the branch the case is there for is the one that runs.
_C4_KW = dict(_C4_KW, in_channels=20)

CASES = [
    Case("L1", "LinearReparameterization", dict(in_features=24, out_features=16), (5, 24), "fast dgrad, plain layout",
         lambda l, x: _ag().fast_dgrad_ok(l) and l._btx_cpad is None),
    Case("L2", "LinearFlipout", dict(in_features=50, out_features=10, bias=False), (7, 50), "channel-padded: signs as tensors",
         lambda l, x: l._btx_cpad is not None),
    Case("L3", "LinearFlipout", dict(in_features=32, out_features=16), (3, 4, 32), "3-D input: dy.reshape(-1, N)",
         lambda l, x: x.dim() == 3 and l._op.nd == 0 and l._btx_cpad is None),
    Case("C1", "Conv2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, padding=1), (2, 16, 6, 6),
         "plain layout, hashed signs, stride-1 fast dgrad",
         lambda l, x: l._btx_cpad is None and l._rowfuse_plan(x) is None and _ag().fast_dgrad_ok(l) and l._op.stride == (1, 1, 1)),
    Case("C2", "Conv2dReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, stride=2, padding=1), (2, 16, 7, 7),
         "strided fast dgrad, odd extent", lambda l, x: _ag().fast_dgrad_ok(l) and l._op.stride[1:] == (2, 2) and x.shape[2] % 2 == 1),
    # (7 + 2 - 2 - 1) % 2 == 0: the odd extent of C2 needs NO output padding; the even one does.  Both stay.
    Case("C2e", "Conv2dReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, stride=2, padding=1), (2, 16, 8, 6),
         "strided fast dgrad, output_padding != 0", lambda l, x: _ag().fast_dgrad_ok(l) and _outpad(l, x) == (1, 1)),
    Case("C3", "Conv2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, padding=2, dilation=2, groups=2), (2, 16, 7, 9),
         "slow dgrad: nz['eps_w']", lambda l, x: not _ag().fast_dgrad_ok(l) and l._btx_cpad is None),
    Case("C4", _C4_CLS, _C4_KW, (1, 20, 5, 5), "channel-padded conv: signs as tensors", lambda l, x: l._btx_cpad is not None),
    Case("C5", "Conv2dFlipout", dict(in_channels=3, out_channels=16, kernel_size=7, stride=2, padding=3, bias=False), (2, 3, 18, 14),
         "row-fused stem", lambda l, x: l._rowfuse_plan(x) is not None),
    Case("C6", "ConvTranspose2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=4, stride=2, padding=1), (2, 16, 4, 5),
         "transposed: bias gradient by torch", lambda l, x: l._op.transposed and l.mu_bias is not None),
    Case("C7", "Conv1dFlipout", dict(in_channels=16, out_channels=32, kernel_size=5, stride=2, padding=2), (3, 16, 17),
         "nd == 1", lambda l, x: l._op.nd == 1),
    Case("R1", "LinearLocalReparameterization", dict(in_features=24, out_features=16), (5, 24), "lrt_train_ok follows fused_training",
         _lrt_ok),
    Case("R2", "Conv2dLocalReparameterization", dict(in_channels=16, out_channels=16, kernel_size=3, padding=1), (2, 16, 6, 6),
         "lrt_train_ok follows fused_training", _lrt_ok),
]
BY_ID = {c.id: c for c in CASES}
# the square variant of L1 for a layer applied twice (S6)
L1SQ = Case("L1sq", "LinearReparameterization", dict(in_features=16, out_features=16), (5, 16), "fast dgrad, plain layout",
            BY_ID["L1"].pre)


def tensor(shape, dtype, seed, device, scale=1.0):
    t = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(device).to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else t


def build(case, prec="f32", act=F32, fused=None):
    """(layer, x) of a case on the GPU, the same every call: sigma between 0.007 and 0.7 (the noise term is neither negligible nor
    dominant), biases away from their zero initialisation, the branch precondition asserted"""
    layer = make(case.cls, case.kw, prec)
    with torch.no_grad():
        g = torch.Generator().manual_seed(41)
        mu, rho = layer._w()
        rho.copy_((torch.rand(tuple(rho.shape), generator=g) * 5.0 - 5.0).to(rho.device))
        if layer.mu_bias is not None:
            layer.mu_bias.copy_((torch.randn(tuple(layer.mu_bias.shape), generator=g) * 0.5).to(rho.device))
            layer.rho_bias.copy_((torch.rand(tuple(layer.rho_bias.shape), generator=g) * 3.0 - 3.0).to(rho.device))
    layer.train()
    layer.dnn_to_bnn_flag = True
    if fused is not None:
        layer.fused_training = fused
    x = tensor(case.xshape, act, 11, dev(), 1.5)
    case.check_precondition(layer, x)
    return layer, x


# =============================================================================================================================
# running a layer under autograd
# =============================================================================================================================
def params_of(layer):
    if not hasattr(layer, "_w"):   # MCDropout: no parameters, x is the only input
        return {}
    mu, rho = layer._w()
    d = {"mu": mu, "rho": rho}
    if layer.mu_bias is not None:
        d["mu_b"], d["rho_b"] = layer.mu_bias, layer.rho_bias
    return d


def present(layer):
    return ("x",) + tuple(params_of(layer))


def subsets(names):
    for r in range(1, len(names) + 1):
        for sub in itertools.combinations(names, r):
            yield sub


def require(layer, subset):
    for n, p in params_of(layer).items():
        p.requires_grad_(n in subset)
        p.grad = None


def forward(layer, x, subset):
    """one forward with requires_grad on exactly `subset` -> (out, {name: leaf})"""
    require(layer, subset)
    xin = x.detach().requires_grad_("x" in subset)
    out = layer(xin)
    out = out[0] if isinstance(out, tuple) else out
    leaves = dict(params_of(layer), x=xin)
    return out, {n: leaves[n] for n in subset}


def grads(out, leaves, dy, retain=False):
    """torch.autograd.grad on a subset: nothing accumulates; a gradient the Function did not return comes back as None"""
    names = list(leaves)
    got = torch.autograd.grad(out, [leaves[n] for n in names], dy, retain_graph=retain, allow_unused=True)
    return dict(zip(names, got))


def step(layer, x, subset, dy, sample=SAMPLE):
    import bayesian_torch_amd as bt
    bt.set_sample_index(layer, sample)
    out, leaves = forward(layer, x, subset)
    if out.grad_fn is None:   # the forward took a no-grad route: the scenario reports it
        return out, {n: None for n in leaves}
    return out, grads(out, leaves, dy)


def dy_for(layer, x, seed=12):
    """a dense gradient of the output's shape, dtype and (channels-last) layout"""
    with torch.no_grad():
        out = layer(x)
        out = out[0] if isinstance(out, tuple) else out
    return tensor(tuple(out.shape), out.dtype, seed, out.device)


class Notes:
    """one line per comparison, in the format of profiles/elementwise_envelope.txt; `lines` is what the profile file records"""

    def __init__(self, tag):
        self.tag, self.lines, self.bad = tag, [], []

    def bits(self, name, got, ref):
        if got is None:
            self.bad.append("%s %s: no gradient (None)" % (self.tag, name))
            return
        rep = E.check_exact(got, ref)
        if not rep.ok:
            scale = float(np.abs(E._np(ref)).max())
            self.bad.append("%s %s: not the same bits: %s; mismatch / max|ref| = %.3g" % (self.tag, name, rep, rep.err / max(scale, 1e-300)))

    def envelope(self, name, prec, got, ref, bnd):
        if got is None:
            self.bad.append("%s %s: no gradient (None)" % (self.tag, name))
            return None
        rep = E.check(got, ref, bnd)
        self.lines.append(rep.line("%s %s" % (self.tag, name), prec))
        if not rep.ok:
            self.bad.append("%s %s %s: %s" % (self.tag, name, prec, rep))
        return rep

    def done(self, what="bits equal"):
        for ln in self.lines:
            print(ln)
        assert not self.bad, "\n".join(self.bad)
        print("%s: %s" % (self.tag, what))


# =============================================================================================================================
# float64 references of the contraction layers (the construction of test_small_case_gradients_every_element), with the errors of the
# operands carried through for compositions
# =============================================================================================================================
def noise_of(layer, sample, x, dy):
    with torch.no_grad():
        return layer.materialize_noise(sample, tuple(x.shape), tuple(dy.shape), x.dtype)


def contract_grads64(layer, x, dy, nz, prec="f32", x_err=None, dy_err=None):
    """float64 gradients of ONE call of a Reparameterization / Flipout layer and their per-element bounds -> (ref, bnd), dicts over
    NAMES.  x_err / dy_err: per-element bounds on the operands the device call saw instead of (x, dy) (a composition feeds a call the
    rounded result of another): a linear map carries them through on absolute values, and the roundings act on |operand| + its bound.
    bf16: the data gradient is the forward's contraction (both operands rounded, the result rounded on store), the weight gradient the
    exact-f32 MFMA on bf16 values."""
    mu, rho = layer._w()
    op = op_of(layer)
    flip = layer._family == "flipout"
    w_shape = tuple(mu.shape)
    lin3d = op["kind"] == "linear" and x.dim() > 2
    x2, dy2 = (x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])) if lin3d else (x, dy)
    x64 = E.d64(x2).requires_grad_(True)
    mu64 = E.d64(mu).requires_grad_(True)
    eps = E.d64(nz["eps_w"])
    delta64 = (E.sigma64(rho) * eps).requires_grad_(True)
    dy64 = E.d64(dy2)
    if flip:
        si, so = E.d64(nz["sign_in"].reshape(x2.shape)), E.d64(nz["sign_out"].reshape(dy2.shape))
        val = E.contract(x64, mu64, None, op) + E.contract(x64 * si, delta64, None, op) * so
    else:
        val = E.contract(x64, mu64 + delta64, None, op)
    dx, dmu, dd = torch.autograd.grad(val, (x64, mu64, delta64), dy64)
    zero = lambda t: torch.zeros_like(t)  # noqa: E731
    xe = zero(dy64).new_zeros(x64.shape) if x_err is None else torch.as_tensor(E._np(x_err)).reshape(x64.shape)
    dye = zero(dy64) if dy_err is None else torch.as_tensor(E._np(dy_err)).reshape(dy64.shape)
    absw = E.abs_weight(mu, rho, nz["eps_w"])
    xs = tuple(x64.shape)
    Kd, Kw = E.dgrad_reduction_length(w_shape, op), E.wgrad_reduction_length(tuple(dy64.shape), op)
    A_dx = E.dgrad_A(dy64.abs() + dye, xs, absw, op)
    b_dx = E.bound(A_dx, prec, Kd) + E._np(E.dgrad_A(dye, xs, absw, op))
    if x.dtype == BF16:
        b_dx = E.store_rounding(b_dx, dx)
    xa, dya = x64.detach().abs(), dy64.abs()
    A_w = E.wgrad_A(xa + xe, dya + dye, w_shape, op)
    b_w = E.bound(A_w, "f32", Kw, delta_w=0.0) + E._np(E.wgrad_A(xe, dya + dye, w_shape, op)) + E._np(E.wgrad_A(xa, dye, w_shape, op))
    sig = torch.sigmoid(E.d64(rho)) * eps
    ref = {"x": dx.reshape(x.shape), "mu": dmu, "rho": dd * sig}
    bnd = {"x": b_dx.reshape(x.shape), "mu": b_w, "rho": scaled(b_w, dd, sig)}
    if layer.mu_bias is not None:
        red = tuple(i for i in range(dy64.dim()) if i != (dy64.dim() - 1 if op["kind"] == "linear" else 1))
        db, A_b = dy64.sum(red), (dya + dye).sum(red)
        b_b = E.bound(A_b, "f32", Kw, delta_w=0.0) + E._np(dye.sum(red))
        dbd = (dy64 * so).sum(red) if flip else db
        sig_b = torch.sigmoid(E.d64(layer.rho_bias)) * E.d64(nz["eps_b"])
        ref.update(mu_b=db, rho_b=dbd * sig_b)
        bnd.update(mu_b=b_b, rho_b=scaled(b_b, dbd, sig_b))
    return ref, bnd


def forward64(layer, x, nz, out_shape, prec="f32"):
    """float64 value of one call and its bound (envelope.reference_forward / bound) -> (ref, bnd)"""
    mu, rho = layer._w()
    op = op_of(layer)
    flip = layer._family == "flipout"
    si = nz["sign_in"].reshape(x.shape) if flip else None
    so = nz["sign_out"].reshape(out_shape) if flip else None
    with torch.no_grad():
        ref, A, Ab = E.reference_forward(x, mu, rho, nz["eps_w"], layer.mu_bias, layer.rho_bias, nz.get("eps_b"), si, so, op)
    return ref, E.bound(A, prec, E.reduction_length(tuple(mu.shape), op), ref=ref, A_bias=Ab, store_bf16=(x.dtype == BF16))


def ref64_single(prec="f32"):
    """the float64 side of one call, as the scenarios take it"""
    return lambda layer, x, dy, sample: contract_grads64(layer, x, dy, noise_of(layer, sample, x, dy), prec)


def ref64_twice(prec="f32"):
    """the float64 side of S6: the two noise sets materialised at s and s + 1"""
    def ref(layer, x, dy, sample, h_got, y_got):
        return twice64(layer, x, dy, noise_of(layer, sample, x, h_got), noise_of(layer, sample + 1, h_got, dy), h_got, prec)
    return ref


def sum_bound(b1, b2, total):
    """two calls' gradients added into one tensor in f32: the two bounds plus 2^-24 |sum| for the one add"""
    return E._np(b1) + E._np(b2) + E.REF32_UNIT * np.abs(E._np(total))


# =============================================================================================================================
# the scenarios.  `build()` returns a fresh (layer, x), the same every call; every scenario raises AssertionError naming each bad
# quantity.  `ref64(layer, x, dy, sample)` -> (ref, bnd) is the float64 side, where a scenario has one.
# =============================================================================================================================
def s1_subsets(build, tag, ref64=None, prec="f32", sample=SAMPLE, inexact=()):
    """S1: every non-empty subset of needs_input_grad gives the bits of the all-gradients call; no gradient is None; the output has a
    grad_fn; the all-gradients call is inside the envelope.  inexact: gradients that are not bit-reproducible from call to call on the
    device (named by the caller, with the reason): each call's value is compared with float64 by the envelope rule instead"""
    layer, x = build()
    dy = dy_for(layer, x)
    names = present(layer)
    out_all, g_all = step(layer, x, names, dy, sample)
    notes = Notes("%s S1" % tag)
    for n in names:
        if g_all[n] is None:
            notes.bad.append("%s S1 all: d%s is None" % (tag, n))
    if ref64 is not None:
        ref, bnd = ref64(layer, x, dy, sample)
        for n in names:
            notes.envelope("all d%s" % n, prec, g_all[n], ref[n], bnd[n])
    count = 0
    for sub in subsets(names):
        out, g = step(layer, x, sub, dy, sample)
        key = "+".join(sub)
        if out.grad_fn is None:
            notes.bad.append("%s S1 {%s}: the output has no grad_fn" % (tag, key))
            continue
        notes.bits("{%s} out" % key, out, out_all)
        for n in sub:
            if n in inexact:
                rep = E.check(g[n], ref[n], bnd[n]) if g[n] is not None else None
                if rep is None or not rep.ok:
                    notes.bad.append("%s S1 {%s} d%s (envelope rule): %s" % (tag, key, n, rep))
            elif g_all[n] is not None:
                notes.bits("{%s} d%s" % (key, n), g[n], g_all[n])
        count += 1
    notes.done("%d subsets, bits equal to the all-gradients call%s" % (
        count, " (d%s by the envelope rule)" % ", d".join(inexact) if inexact else ""))


def s2_forward_identity(build, tag, words=False, sample=SAMPLE):
    """S2: out_a = layer(xa) at s, out_b = layer(xb) at s + 1, the layer re-pinned to 77, then backward of out_b, then of out_a: each
    gradient has the bits of a lone forward + backward at its own index.  words: the two forwards read two words of a device sample
    tensor instead (as GraphedTrainStep._step points the layers from pass to pass).  The words hold s + 40 and s + 41 — values the
    host counter (s, s + 1, then 77) never takes — and the layer points at NO word when the backward runs: a backward that falls back
    on ctx.sample_idx, on the layer's current counter or on the layer's current word draws other noise than the lone steps at
    s + 40 / s + 41 and fails."""
    import bayesian_torch_amd as bt
    layer, xa = build()
    xb = (xa.float() * 0.5 + 0.25).to(xa.dtype)
    names = present(layer)
    dya, dyb = dy_for(layer, xa, 12), dy_for(layer, xa, 13)
    ia, ib = (sample + 40, sample + 41) if words else (sample, sample + 1)
    _, lone_a = step(layer, xa, names, dya, ia)
    _, lone_b = step(layer, xb, names, dyb, ib)
    require(layer, names)
    bt.set_sample_index(layer, sample)
    try:
        if words:
            w = torch.tensor([ia, ib], dtype=torch.int32, device=xa.device)
            layer.__dict__["_btx_sample_dev"] = w[0:1]
        out_a, leaves_a = forward(layer, xa, names)
        if words:
            layer.__dict__["_btx_sample_dev"] = w[1:2]
        out_b, leaves_b = forward(layer, xb, names)
    finally:
        if words:
            layer.__dict__["_btx_sample_dev"] = None
    assert layer._btx_sample == sample + 2, (layer._btx_sample, sample)
    bt.set_sample_index(layer, 77)
    gb = grads(out_b, leaves_b, dyb)
    ga = grads(out_a, leaves_a, dya)
    notes = Notes("%s S2%s" % (tag, " device words" if words else ""))
    for n in names:
        notes.bits("second forward d%s" % n, gb[n], lone_b[n])
        notes.bits("first forward d%s" % n, ga[n], lone_a[n])
    notes.done()


def s3_seed_change(build, tag, a=1111, b=2222, sample=SAMPLE):
    """S3: manual_seed(a), forward, manual_seed(b), backward: the bits of a step run entirely under a"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import rng
    layer, x = build()
    old = rng.seed()
    try:
        bt.manual_seed(a)
        names = present(layer)
        dy = dy_for(layer, x)
        _, want = step(layer, x, names, dy, sample)
        bt.set_sample_index(layer, sample)
        out, leaves = forward(layer, x, names)
        bt.manual_seed(b)
        got = grads(out, leaves, dy)
    finally:
        bt.manual_seed(old)
    notes = Notes("%s S3" % tag)
    for n in names:
        notes.bits("d%s" % n, got[n], want[n])
    notes.done()


def s4_dy_forms(build, tag, ref64=None, prec="f32", sample=SAMPLE, nchw=True, inexact=(), nchw_inexact=()):
    """S4: one forward, then backward calls whose dy reaches the Function stride-0 expanded (out.sum()), 4 bytes off the 16-byte grid,
    as f32 on bf16 activations and (4-D outputs) NCHW-contiguous: each has the bits of the call with the equivalent dense dy in the
    output's own layout; the stride-0 form is inside the envelope against float64.
    The f32-dy form is no coverage of an f32-dy kernel path: autograd casts the incoming gradient to the output's dtype before a
    Function sees it (in the backward of out.float(), and again when the engine validates a node's inputs), so the Function
    receives the bf16 dy of the dense call.  The form pins exactly that: a mixed-precision loss changes nothing.
    Moved from the bit rule to the envelope rule (profiles/autograd_contract.txt), wherever the case has a float64 side:
      * dx, dmu, drho under an OFF-GRID dy: it selects other kernels — the gather kernel for the data gradient, the generic weight
        gradient instead of the vectorised / all-taps one (tests/test_gpu_alignment.py::test_backward_off_grid pins exactly this)
      * `inexact` (every form) and `nchw_inexact` (the NCHW form): named by the caller with the reason"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    from test_gpu_alignment import off_grid
    layer, x = build()
    names = present(layer)
    dy = dy_for(layer, x)
    bt.set_sample_index(layer, sample)
    out, leaves = forward(layer, x, names)
    order = [leaves[n] for n in names]
    notes = Notes("%s S4" % tag)
    ones = torch.ones_like(out)
    dense1 = grads(out, leaves, ones, retain=True)
    got = dict(zip(names, torch.autograd.grad(out.sum(), order, retain_graph=True, allow_unused=True)))
    for n in names:
        if n not in inexact:
            notes.bits("stride-0 dy d%s" % n, got[n], dense1[n])
    if ref64 is not None:
        ref, bnd = ref64(layer, x, ones, sample)
        for n in names:
            notes.envelope("stride-0 dy d%s" % n, prec, got[n], ref[n], bnd[n])
    dense = grads(out, leaves, dy, retain=True)
    got = grads(out, leaves, off_grid(dy, 4), retain=True)
    ref_d, bnd_d = ref64(layer, x, dy, sample) if ref64 is not None else (None, None)
    for n in names:
        if ref_d is not None and (n in ("x", "mu", "rho") or n in inexact):
            notes.envelope("off-grid dy d%s" % n, prec, got[n], ref_d[n], bnd_d[n])
        else:
            notes.bits("off-grid dy d%s" % n, got[n], dense[n])
    if out.dtype == BF16:
        got = dict(zip(names, torch.autograd.grad(out.float(), order, dy.float(), retain_graph=True, allow_unused=True)))
        for n in names:
            if n in inexact:
                notes.envelope("f32 dy on bf16 activations d%s" % n, prec, got[n], ref_d[n], bnd_d[n])
            else:
                notes.bits("f32 dy on bf16 activations d%s" % n, got[n], dense[n])
    if out.dim() == 4 and nchw:   # (the output layout is a switch of the HIP Functions: not of dropout, not of the ATen composite)
        BF.set_output_layout("contiguous")
        try:
            bt.set_sample_index(layer, sample)
            out_c, leaves_c = forward(layer, x, names)
            assert out_c.is_contiguous(), out_c.stride()
            w = dy.contiguous()
            assert w.is_contiguous() and not w.is_contiguous(memory_format=torch.channels_last)
            got = dict(zip(names, torch.autograd.grad((out_c * w).sum(), [leaves_c[n] for n in names], allow_unused=True)))
        finally:
            BF.set_output_layout("channels_last")
        for n in names:
            if n in inexact or n in nchw_inexact:
                notes.envelope("NCHW-contiguous dy d%s" % n, prec, got[n], ref_d[n], bnd_d[n])
            else:
                notes.bits("NCHW-contiguous dy d%s" % n, got[n], dense[n])
    notes.done()


def s5_retain_and_accumulate(build, tag, sample=SAMPLE):
    """S5: a second backward on a retained graph has the bits of the first; two backward() calls without zero_grad leave g1 + g2 formed
    in f32 (one add); the accumulated gradient has the parameter's strides and survives an unrelated third backward"""
    import bayesian_torch_amd as bt
    layer, x = build()
    names = present(layer)
    dy1, dy2 = dy_for(layer, x, 12), dy_for(layer, x, 13)
    bt.set_sample_index(layer, sample)
    out, leaves = forward(layer, x, names)
    g1 = grads(out, leaves, dy1, retain=True)
    g1b = grads(out, leaves, dy1, retain=True)
    g2 = grads(out, leaves, dy2, retain=True)
    notes = Notes("%s S5" % tag)
    for n in names:
        notes.bits("retained graph, second call d%s" % n, g1b[n], g1[n])
    out.backward(dy1, retain_graph=True)
    out.backward(dy2)
    held = {}
    for n in names:
        acc = leaves[n].grad
        if acc is None or g1[n] is None or g2[n] is None:
            notes.bad.append("%s S5 accumulated d%s: missing" % (tag, n))
            continue
        notes.bits("accumulated d%s = g1 + g2" % n, acc, g1[n].detach().cpu() + g2[n].detach().cpu())
        if n != "x":
            if tuple(acc.stride()) != tuple(leaves[n].stride()):
                notes.bad.append("%s S5 d%s: strides %s, the parameter's are %s" % (tag, n, tuple(acc.stride()), tuple(leaves[n].stride())))
        held[n] = acc.detach().clone()
    other, xo = build()   # an unrelated layer of the same shapes: its launches reuse whatever buffers the first ones released
    step(other, xo * 2, present(other), dy2, sample + 9)
    for n, keep in held.items():
        notes.bits("d%s after an unrelated backward" % n, leaves[n].grad, keep)
    notes.done()


def s6_applied_twice(build, tag, ref64_twice, prec="f32", sample=SAMPLE):
    """S6: y = layer(layer(x)), the two calls drawing s and s + 1; dmu, drho (and the bias gradients) are the SUM of the two calls'
    gradients: inside the summed envelope against the float64 composition with the two materialised noise sets"""
    import bayesian_torch_amd as bt
    layer, x = build()
    names = present(layer)
    require(layer, names)
    bt.set_sample_index(layer, sample)
    xin = x.detach().requires_grad_(True)
    h = layer(xin)
    y = layer(h)
    assert layer._btx_sample == sample + 2
    dy = tensor(tuple(y.shape), y.dtype, 12, y.device)
    leaves = dict(params_of(layer), x=xin)
    got = grads(y, leaves, dy)
    ref, bnd = ref64_twice(layer, x, dy, sample, h.detach(), y.detach())
    notes = Notes("%s S6" % tag)
    for n in names:
        notes.envelope("d%s" % n, prec, got[n], ref[n], bnd[n])
    notes.done("inside the summed envelope")


def twice64(layer, x, dy, nz1, nz2, h_got, prec="f32"):
    """the float64 side of S6 for a contraction layer: h = f_1(x), y = f_2(h).  Call 2 saw h_got = h + e_f (|e_f| <= the forward's
    bound) as its input; call 1 saw dh_got = dh + e_2 (|e_2| <= call 2's data-gradient bound) as its dy.  Both are carried through
    contract_grads64's x_err / dy_err; the parameter gradients are the two calls' added in f32: sum_bound."""
    h64, b_f = forward64(layer, x, nz1, tuple(h_got.shape), prec)
    r2, b2 = contract_grads64(layer, h64.float(), dy, nz2, prec, x_err=b_f + E.REF32_UNIT * np.abs(E._np(h64)))
    r1, b1 = contract_grads64(layer, x, r2["x"].float(), nz1, prec, dy_err=b2["x"] + E.REF32_UNIT * np.abs(E._np(r2["x"])))
    ref, bnd = {"x": r1["x"]}, {"x": b1["x"]}
    for n in r1:
        if n != "x":
            ref[n] = r1[n] + r2[n]
            bnd[n] = sum_bound(b1[n], b2[n], ref[n])
    return ref, bnd


def s9_checkpoint(build_block, tag, ckpt, sample=SAMPLE):
    """S9: the block through `ckpt` has the bits of the plain step at the same indices — loss, every parameter gradient, dx — leaves
    every layer's counters where the plain step leaves them, and two consecutive checkpointed steps draw s, then s + 1"""
    import bayesian_torch_amd as bt

    def two_steps(wrap):
        net, x = build_block()
        bt.set_sample_index(net, sample)
        res = []
        for _ in range(2):
            for p in net.parameters():
                p.grad = None
            xin = x.detach().requires_grad_(True)
            out = ckpt(net, xin) if wrap else net(xin)
            dy = tensor(tuple(out.shape), out.dtype, 12, out.device)
            loss = (out.float() * dy.float()).sum()
            loss.backward()
            g = {name: p.grad.detach().clone() for name, p in net.named_parameters()}
            g["x"], g["loss"] = xin.grad.detach().clone(), loss.detach().clone()
            counters = [(m._btx_sample, m.__dict__.get("_btx_kl_sample")) for m in net.modules() if hasattr(m, "_btx_layer_id")]
            res.append((g, counters))
        return res
    plain, wrapped = two_steps(False), two_steps(True)
    notes = Notes("%s S9" % tag)
    for k, ((gp, cp), (gw, cw)) in enumerate(zip(plain, wrapped)):
        for n in gp:
            notes.bits("step %d %s" % (k, n), gw[n], gp[n])
        if cp != cw:
            notes.bad.append("%s S9 step %d: counters %s after the checkpointed step, %s after the plain one" % (tag, k, cw, cp))
    assert plain[0][1][0][0] == sample + 1 and plain[1][1][0][0] == sample + 2
    notes.done()
