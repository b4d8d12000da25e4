"""CPU: the instruments of tests/envelope.py have teeth.  No GPU is touched.

Each precision of the HIP kernels is emulated with torch on the CPU (operands rounded with .to(bfloat16), hi/lo split for
bf16x3, f32 convolution, f32 Flipout combine, optional bf16 store, BN + ReLU + max-pool), the float64 chain is the reference:

  * the clean emulation must stay below HALF of the envelope in every case (the derivation, not a fitted constant, has to
    leave that room: a case that does not is a wrong derivation for that case);
  * faults of the kind these kernels can have — one sign flipped at one pixel, one halo column dropped for one row tile, one
    output row shifted, one tap reading its neighbour's weights, one pixel chunk dropped / doubled in a weight gradient — are
    injected into the emulation.  Each must be flagged by the instrument, and (the reason this file exists) helpers.rel_l2 must
    stay UNDER the bar the GPU test of that path uses today.  Where a fault is large enough to trip rel-L2 as well, the
    parametrize id says so and only that half is dropped.
"""
import numpy as np
import pytest
import torch

import envelope as E
from helpers import rel_l2

torch.set_num_threads(min(16, torch.get_num_threads()))

BAR_BF16 = 1e-2        # tests/test_gpu_at_size.py: bf16 per-layer rel-L2
BAR_WGRAD_BF16 = 2e-2  # tests/test_gpu_backward.py: test_backward_at_baseline_size_every_resnet18_layer_shape, bf16


# ---- emulation of the three MFMA precisions ---------------------------------------------------------------------------------
def _r(t):
    return t.to(torch.bfloat16).float()


def _split(t):
    hi = _r(t)
    return hi, _r(t - hi)


def emu_contract(x, w, op, prec):
    """f32 in, f32 out: what one launch computes from f32 activations and f32 sampled weights"""
    if prec == "f32":
        return E.contract(x, w, None, op)
    if prec == "bf16":
        return E.contract(_r(x), _r(w), None, op)
    (xh, xl), (wh, wl) = _split(x), _split(w)
    return E.contract(xh, wh, None, op) + E.contract(xl, wh, None, op) + E.contract(xh, wl, None, op)


def emu_forward(x, p, op, prec, store_bf16=False, sign_out=None, w_of=None):
    """p: dict(mu, rho, eps, mu_b, rho_b, eps_b, sign_in, sign_out) f32; Flipout when sign_in is there.  w_of(mu, delta) -> the
    (possibly faulty) weights the launch reads"""
    delta = torch.log1p(torch.exp(p["rho"])) * p["eps"]
    mu = p["mu"]
    if w_of is not None:
        mu, delta = w_of(mu, delta)
    cshape = [1] * (x.dim())
    cshape[-1 if op["kind"] == "linear" else 1] = -1
    if p.get("sign_in") is not None:
        so = p["sign_out"] if sign_out is None else sign_out
        mean = emu_contract(x, mu, op, prec)
        pert = emu_contract(x * p["sign_in"], delta, op, prec)
        if p.get("mu_b") is not None:
            mean = mean + p["mu_b"].reshape(cshape)
            pert = pert + (torch.log1p(torch.exp(p["rho_b"])) * p["eps_b"]).reshape(cshape)
        out = mean + pert * so
    else:
        out = emu_contract(x, mu + delta, op, prec)
        if p.get("mu_b") is not None:
            out = out + (p["mu_b"] + torch.log1p(torch.exp(p["rho_b"])) * p["eps_b"]).reshape(cshape)
    return _r(out) if store_bf16 else out


def emu_dgrad(dy, x_shape, p, op, prec):
    """the data gradient on the same MFMA precisions: op^T(dy, W) with rounded operands, f32 accumulation"""
    delta = torch.log1p(torch.exp(p["rho"])) * p["eps"]

    def t(dyv, w):
        if prec == "bf16x3":
            (dh, dl), (wh, wl) = _split(dyv), _split(w)
            return _t(dh, wh) + _t(dl, wh) + _t(dh, wl)
        return _t(_r(dyv), _r(w)) if prec == "bf16" else _t(dyv, w)

    def _t(dyv, w):
        xz = torch.zeros(x_shape, requires_grad=True)
        return torch.autograd.grad(E.contract(xz, w, None, op), xz, dyv)[0]
    if p.get("sign_in") is not None:
        return t(dy, p["mu"]) + p["sign_in"] * t(dy * p["sign_out"], delta)
    return t(dy, p["mu"] + delta)


def emu_wgrad(x, dy, w_shape, op, bf16_act):
    """corr(x, dy) in f32 on bf16- or f32-valued activations (the weight gradient has no bf16x3 form)"""
    if bf16_act:
        x, dy = _r(x), _r(dy)
    wz = torch.zeros(w_shape, requires_grad=True)
    return torch.autograd.grad(E.contract(x, wz, None, op), wz, dy)[0]


def _conv(nd=2, stride=1, padding=0, dilation=1, groups=1, kind="conv", output_padding=0):
    t = lambda v: (v,) * nd if isinstance(v, int) else tuple(v)  # noqa: E731
    d = dict(kind=kind, nd=nd, stride=t(stride), padding=t(padding), dilation=t(dilation), groups=groups)
    if kind == "convT":
        d["output_padding"] = t(output_padding)
    return d


# (name, op, weight shape, x shape, Flipout?, bias?)
CASES = [
    ("3x3_s1", _conv(padding=1), (64, 64, 3, 3), (4, 64, 28, 28), True, False),
    ("3x3_s2", _conv(stride=2, padding=1), (128, 64, 3, 3), (4, 64, 28, 28), True, True),
    ("1x1", _conv(), (128, 256, 1, 1), (4, 256, 14, 14), True, False),
    ("7x7_stem", _conv(stride=2, padding=3), (64, 3, 7, 7), (2, 3, 64, 64), True, False),
    ("grouped", _conv(padding=1, groups=2), (96, 32, 3, 3), (3, 64, 17, 19), False, True),
    ("dilated", _conv(padding=2, dilation=2), (48, 32, 3, 3), (2, 32, 9, 11), True, True),
    ("linear", dict(kind="linear"), (512, 784), (64, 784), True, True),
    ("convT", _conv(stride=2, padding=1, kind="convT"), (16, 16, 4, 4), (2, 16, 6, 7), True, False),
]


def _params(w_shape, x_shape, op, flip, bias, seed, rho_mean=-3.0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    nout = w_shape[1] * op["groups"] if op["kind"] == "convT" else w_shape[0]
    p = dict(mu=0.1 * rn(*w_shape), rho=rho_mean + 0.1 * rn(*w_shape), eps=rn(*w_shape))
    if bias:
        p.update(mu_b=0.1 * rn(nout), rho_b=rho_mean + 0.1 * rn(nout), eps_b=rn(nout))
    x = rn(*x_shape)
    out_shape = E.contract(x[:1], p["mu"], None, op).shape[1:]
    out_shape = (x_shape[0],) + tuple(out_shape)
    if flip:
        p["sign_in"] = torch.empty(x_shape).uniform_(-1, 1, generator=g).sign()
        p["sign_out"] = torch.empty(out_shape).uniform_(-1, 1, generator=g).sign()
    return p, x, out_shape


def _ref(x, p, op):
    return E.reference_forward(x, p["mu"], p["rho"], p["eps"], p.get("mu_b"), p.get("rho_b"), p.get("eps_b"), p.get("sign_in"),
                               p.get("sign_out"), op)


@pytest.mark.parametrize("prec,store", [("f32", False), ("bf16", False), ("bf16", True), ("bf16x3", False)])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_clean_forward_emulation_stays_below_half_the_envelope(case, prec, store):
    name, op, w_shape, x_shape, flip, bias = case
    p, x, _ = _params(w_shape, x_shape, op, flip, bias, seed=11)
    if prec == "bf16":
        x = _r(x)  # bf16 activations: the reference sees the same bf16-valued input
    ref, A, Ab = _ref(x, p, op)
    got = emu_forward(x, p, op, prec, store_bf16=store)
    K = E.reduction_length(w_shape, op)
    rep = E.check(got, ref, E.bound(A, prec, K, ref=ref, A_bias=Ab, store_bf16=store))
    print(rep.line("emu fwd " + name + (" bf16-store" if store else ""), prec))
    assert rep.ok and rep.worst < 0.5, str(rep)


@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16x3"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_clean_data_gradient_emulation_stays_below_half_the_envelope(case, prec):
    name, op, w_shape, x_shape, flip, bias = case
    p, x, out_shape = _params(w_shape, x_shape, op, flip, False, seed=12)
    dy = torch.randn(out_shape, generator=torch.Generator().manual_seed(5))
    if prec == "bf16":
        dy = _r(dy)
    got = emu_dgrad(dy, x_shape, p, op, prec)
    ref = emu_dgrad64(dy, x_shape, p, op)
    A = E.dgrad_A(dy, x_shape, E.abs_weight(p["mu"], p["rho"], p["eps"]), op)
    rep = E.check(got, ref, E.bound(A, prec, E.dgrad_reduction_length(w_shape, op)))
    print(rep.line("emu dgrad " + name, prec))
    assert rep.ok and rep.worst < 0.5, str(rep)


def emu_dgrad64(dy, x_shape, p, op):
    q = {k: E.d64(v) for k, v in p.items()}
    delta = torch.log1p(torch.exp(q["rho"])) * q["eps"]

    def _t(dyv, w):
        xz = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(E.contract(xz, w, None, op), xz, dyv)[0]
    dy = E.d64(dy)
    if q.get("sign_in") is not None:
        return _t(dy, q["mu"]) + q["sign_in"] * _t(dy * q["sign_out"], delta)
    return _t(dy, q["mu"] + delta)


@pytest.mark.parametrize("bf16_act", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_clean_small_weight_gradient_emulation_stays_below_half_the_envelope(case, bf16_act):
    name, op, w_shape, x_shape, flip, bias = case
    p, x, out_shape = _params(w_shape, x_shape, op, flip, False, seed=13)
    dy = torch.randn(out_shape, generator=torch.Generator().manual_seed(6))
    if bf16_act:
        x, dy = _r(x), _r(dy)
    got = emu_wgrad(x, dy, w_shape, op, bf16_act)
    ref, A = E.wgrad64(x, dy, w_shape, op), E.wgrad_A(x, dy, w_shape, op)
    # bf16-valued activations multiply exactly in f32: the operand term is zero in both forms, what is left is the accumulation
    rep = E.check(got, ref, E.bound(A, "f32", E.wgrad_reduction_length(out_shape, op), delta_w=0.0))
    print(rep.line("emu wgrad " + name, "bf16" if bf16_act else "f32"))
    assert rep.ok and rep.worst < 0.5, str(rep)


def test_clean_stem_bn_relu_bf16_store_maxpool_emulation():
    """the one-launch stem: conv 7x7/2 -> eval-BN -> ReLU -> bf16 store -> MaxPool2d(3, 2, 1); the bound is carried along"""
    name, op, w_shape, x_shape, flip, _ = CASES[3]
    p, x, _ = _params(w_shape, x_shape, op, flip, False, seed=14)
    x = _r(x)
    g = torch.Generator().manual_seed(3)
    scale, shift = 0.5 + torch.rand(64, generator=g), 0.1 * torch.randn(64, generator=g)
    pre64, A, _ = _ref(x, p, op)
    s64, t64 = E.d64(scale).view(1, -1, 1, 1), E.d64(shift).view(1, -1, 1, 1)
    ref = torch.nn.functional.max_pool2d(torch.relu(pre64 * s64 + t64), 3, 2, 1)
    pre = emu_forward(x, p, op, "bf16")
    got = torch.nn.functional.max_pool2d(_r(torch.relu(pre * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))), 3, 2, 1)
    b = E.bound(A, "bf16", E.reduction_length(w_shape, op))
    b = E.through_affine(b, pre64, scale, shift)
    b = E.store_rounding(b, torch.relu(pre64 * s64 + t64))
    rep = E.check(got, ref, E.through_maxpool2d(b, 3, 2, 1))
    print(rep.line("emu stem+bn+relu+store+pool", "bf16"))
    assert rep.ok and rep.worst < 0.5, str(rep)


# ---- fault injection: bf16 Flipout 3x3 layer of the layer1 shape -------------------------------------------------------
_L1 = dict(op=_conv(padding=1), w_shape=(64, 64, 3, 3), x_shape=(8, 64, 56, 56))
_CACHE = {}


def _layer1():
    if "l1" not in _CACHE:
        p, x, _ = _params(_L1["w_shape"], _L1["x_shape"], _L1["op"], True, False, seed=21)
        x = _r(x)
        ref, A, _ = _ref(x, p, _L1["op"])
        clean = emu_forward(x, p, _L1["op"], "bf16")
        _CACHE["l1"] = (p, x, ref, E.bound(A, "bf16", 576), clean)
    return _CACHE["l1"]


def _fault_sign_one_pixel(p, x, clean):
    so = p["sign_out"].clone()
    so[3, :, 20, 31] *= -1  # sign_out of ONE pixel, all channels
    return emu_forward(x, p, _L1["op"], "bf16", sign_out=so)


def _fault_halo_column(p, x, clean):
    """image 5, the row tile 16..19 reads zeros for the halo column to its right of a 32-wide column tile: only the tile's edge
    column (31) of those rows is computed without that column's three taps"""
    xf = x.clone()
    xf[5, :, :, 32] = 0
    bad = emu_forward(xf, p, _L1["op"], "bf16")
    out = clean.clone()
    out[5, :, 16:20, 31] = bad[5, :, 16:20, 31]
    return out


def _fault_row_shifted(p, x, clean):
    out = clean.clone()
    out[2, :, 40, 1:] = clean[2, :, 40, :-1]
    return out


def _fault_neighbour_tap(p, x, clean):
    def w_of(mu, delta):
        mu, delta = mu.clone(), delta.clone()
        mu[0:16, 0:8, 0, 0] = mu[0:16, 0:8, 0, 1]       # 16 output channels x one 8-channel K block: tap (0,0) reads tap (0,1)
        delta[0:16, 0:8, 0, 0] = delta[0:16, 0:8, 0, 1]
        return mu, delta
    return emu_forward(x, p, _L1["op"], "bf16", w_of=w_of)


FAULTS = [
    pytest.param(_fault_sign_one_pixel, True, id="sign_out-flipped-at-one-pixel"),
    pytest.param(_fault_halo_column, True, id="halo-column-dropped-for-one-row-tile"),
    pytest.param(_fault_row_shifted, False, id="one-output-row-shifted-right--trips-rel-l2-too"),
    pytest.param(_fault_neighbour_tap, False, id="tap-reads-neighbour-weights-one-block--trips-rel-l2-too"),
]


@pytest.mark.parametrize("fault,rel_l2_blind", FAULTS)
def test_injected_forward_fault_is_flagged_where_rel_l2_is_blind(fault, rel_l2_blind):
    p, x, ref, bnd, clean = _layer1()
    rep0 = E.check(clean, ref, bnd)
    assert rep0.ok and rep0.worst < 0.5, str(rep0)
    bad = fault(p, x, clean)
    rep = E.check(bad, ref, bnd)
    r = rel_l2(bad.numpy(), ref.numpy())
    print("fault: %s | rel-L2 %.3g (bar %.0e) | clean rel-L2 %.3g" % (rep, r, BAR_BF16, rel_l2(clean.numpy(), ref.numpy())))
    assert not rep.ok and rep.worst > 1.0 and rep.violations > 0, str(rep)
    if rel_l2_blind:
        assert r < BAR_BF16, r  # today's metric lets this fault through
    else:
        assert r >= BAR_BF16, r  # the id says so: this fault is loud enough for rel-L2 as well


def test_sign_fault_is_located_at_its_pixel():
    p, x, ref, bnd, clean = _layer1()
    rep = E.check(_fault_sign_one_pixel(p, x, clean), ref, bnd)
    assert rep.index[0] == 3 and rep.index[2:] == (20, 31), rep.index
    assert 32 <= rep.violations <= 64, rep.violations  # the flip moves every channel of that pixel; nothing else


@pytest.mark.parametrize("what", ["doubled", "dropped"])
@pytest.mark.parametrize("bf16_act", [False, True], ids=["f32", "bf16"])
def test_pixel_chunk_counted_twice_or_never_in_the_integer_weight_gradient(what, bf16_act):
    """200 704 pixels (the layer1 count at batch 64), small-integer x and dy: the clean f32 weight gradient equals the float64
    one bit for bit, one 64-pixel chunk counted twice (or never) does not, and rel-L2 stays under the 2e-2 bar of the bf16
    at-size backward test"""
    op, w_shape = _conv(padding=1), (8, 8, 3, 3)
    x = E.small_ints((64, 8, 56, 56), 1)
    dy = E.small_ints((64, 8, 56, 56), 2)
    got = emu_wgrad(x, dy, w_shape, op, bf16_act)
    ref = E.wgrad64(x, dy, w_shape, op)
    assert E.check_exact(got, ref).ok  # f32 accumulation of integers below 2^24 is exact in any order
    chunk = torch.zeros_like(dy)
    chunk[17, :, 30, 0:56] = dy[17, :, 30, 0:56]   # 64 consecutive pixels of the channels-last raster: one row + 8 of the next
    chunk[17, :, 31, 0:8] = dy[17, :, 31, 0:8]
    part = emu_wgrad(x, chunk, w_shape, op, bf16_act)
    bad = got + part if what == "doubled" else got - part
    rep = E.check_exact(bad, ref)
    r = rel_l2(bad.numpy(), ref.numpy())
    print("wgrad chunk %s: %s | rel-L2 %.3g (bar %.0e)" % (what, rep, r, BAR_WGRAD_BF16))
    assert not rep.ok and rep.worst == float("inf") and rep.violations > 0.9 * ref.numel()
    assert r < BAR_WGRAD_BF16, r


@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16x3"])
def test_exact_forward_emulation_with_sigma_zero_dyadic_weights_and_integer_inputs(prec):
    """rho = -200: exp underflows, sigma = 0 exactly; mu = m 2^-7 (|m| <= 128) and integer x: exact in every precision"""
    op, w_shape = _conv(padding=1), (32, 64, 3, 3)
    p = dict(mu=E.dyadic(w_shape, 3), rho=torch.full(w_shape, -200.0), eps=torch.randn(w_shape),
             sign_in=torch.ones(2, 64, 20, 20), sign_out=-torch.ones(2, 32, 20, 20))
    x = E.small_ints((2, 64, 20, 20), 4)
    ref = E.contract(E.d64(x), E.d64(p["mu"]), None, op)  # float64 keeps sigma = 1.4e-87: the reference is the mean alone
    assert float(torch.log1p(torch.exp(p["rho"])).max()) == 0.0
    assert E.check_exact(emu_forward(x, p, op, prec), ref).ok
    assert float(ref.abs().max()) > 1


# ---- the helper's own contract ----------------------------------------------------------------------------------------------
def test_worst_element_index_is_translated_to_image_channel_row_col():
    ref = torch.zeros(3, 5, 7, 11, dtype=torch.float64)
    bnd = torch.full_like(ref, 1e-3)
    got = ref.clone()
    got[2, 4, 6, 10] = 5e-3
    got[1, 0, 3, 2] = 2e-3
    got[0, 1, 1, 1] = 0.9e-3  # inside
    rep = E.check(got, ref, bnd)
    assert rep.index == (2, 4, 6, 10) and rep.violations == 2 and abs(rep.worst - 5.0) < 1e-9 and rep.numel == 3 * 5 * 7 * 11
    assert "(2, 4, 6, 10)" in rep.line("x", "f32")
    got[0, 0, 0, 0] = float("nan")
    rep = E.check(got, ref, bnd)
    assert rep.index == (0, 0, 0, 0) and rep.worst == float("inf") and rep.violations == 3


def test_where_the_bound_is_zero_the_output_must_equal_the_reference():
    """A_j = 0: an output that only padding reaches is exactly the bias term (or exactly 0 without one)"""
    op = _conv(padding=2)
    x = torch.zeros(1, 8, 6, 6)
    x[0, :, 4:, 4:] = torch.randn(8, 2, 2)  # the upper-left outputs see zeros only
    p = dict(mu=0.1 * torch.randn(4, 8, 3, 3), rho=torch.full((4, 8, 3, 3), -3.0), eps=torch.randn(4, 8, 3, 3))
    ref, A, _ = _ref(x, p, op)
    assert float(A[0, :, 0, 0].max()) == 0.0
    bnd = E.bound(A, "bf16", 72)
    got = emu_forward(x, p, op, "bf16")
    assert E.check(got, ref, bnd).ok
    got[0, 2, 0, 0] = 1e-30  # any value at all where nothing can have been accumulated
    rep = E.check(got, ref, bnd)
    assert not rep.ok and rep.index == (0, 2, 0, 0) and rep.worst == float("inf") and rep.violations == 1
    # with a bias the bound there is the f32 share of the bias alone
    p.update(mu_b=torch.randn(4), rho_b=torch.full((4,), -3.0), eps_b=torch.randn(4))
    ref, A, Ab = _ref(x, p, op)
    bnd = E.bound(A, "bf16", 72, A_bias=Ab)
    got = emu_forward(x, p, op, "bf16")
    assert E.check(got, ref, bnd).ok
    assert bnd[0, 1, 0, 0] == E.rel_constant("f32", 0) * float(Ab[0, 1, 0, 0]) < 1e-5 * abs(float(ref[0, 1, 0, 0]))
    got[0, 1, 0, 0] *= 1.0 + 2.0 ** -12  # a bf16-sized error on the bias term
    assert not E.check(got, ref, bnd).ok


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """the u of the envelope: bf16 keeps 8 significant bits, so one rounding errs by up to 2^-8 / (1 + 2^-8) — almost twice
    2^-9.  A bound built on 2^-9 is passed by long reductions (the roundings average out) and broken by every short one: a
    single product (the impulse probes) and the bf16 store of an accurately accumulated result."""
    one = torch.tensor([1.0 + 2.0 ** -8])
    assert float(_r(one)) == 1.0                                # the tie goes to the even neighbour
    assert float((one - _r(one)) / one) > 1.99 * 2.0 ** -9
    g = torch.Generator().manual_seed(1)
    v = torch.rand(1 << 20, generator=g) + 1.0
    worst = float(((v - _r(v)).abs() / v).max())
    assert 1.9 * 2.0 ** -9 < worst <= 2.0 ** -8 == E.U_BF16


def test_short_reductions_need_the_true_unit_roundoff():
    """an impulse through the bf16 emulation (K = 1) and the bf16 store of an f32-mode result: clean, inside the envelope, and
    close to it (one rounding fills its bound) — with u = 2^-9 both would be reported as kernel faults"""
    name, op, w_shape, x_shape, flip, bias = CASES[0]
    p, _, out_shape = _params(w_shape, x_shape, op, flip, False, seed=15)
    x = torch.zeros(x_shape)
    x[:, :, 5::3, 4::3] = torch.eye(64)[torch.arange(8 * 8) % 64].t().reshape(1, 64, 8, 8)  # one channel per impulse
    ref, A, _ = _ref(x, p, op)
    assert float(E.contract(x, torch.ones(w_shape), None, op).max()) == 1.0  # every output is a single product
    got = emu_forward(x, p, op, "bf16")
    bnd = (E.U_BF16 + E.DELTA_W * (1 + E.U_BF16) + 8 * E.ACC_UNIT) * A.numpy()
    rep = E.check(got, ref, bnd)
    print(rep.line("emu impulse " + name, "bf16"))
    assert rep.ok and rep.worst > 0.5, str(rep)
    assert not E.check(got, ref, bnd / 2).ok  # what 2^-9 would claim
    # bf16 store of an f32-mode result
    p, xr, _ = _params(w_shape, x_shape, op, flip, False, seed=16)
    ref, A, _ = _ref(xr, p, op)
    got = emu_forward(xr, p, op, "f32", store_bf16=True)
    b32 = E.bound(A, "f32", 576)
    rep = E.check(got, ref, E.store_rounding(b32, ref))
    print(rep.line("emu f32 + bf16 store " + name, "f32"))
    assert rep.ok and rep.worst > 0.5, str(rep)
    assert not E.check(got, ref, E.store_rounding(b32, ref, u=2.0 ** -9)).ok


def test_constants_are_the_derived_ones():
    u = 2.0 ** -8
    assert E.rel_constant("bf16", 576, delta_w=0.0) == 2 * u + u * u + 584 * 2.0 ** -23
    assert E.rel_constant("bf16x3", 576, delta_w=0.0) == 3 * u * u + 2 * u ** 3 + (3 * 576 + 8) * 2.0 ** -23
    assert E.rel_constant("f32", 576, delta_w=1e-6, ref_f32=True) == 1e-6 + 584 * 2.0 ** -23 + 584 * 2.0 ** -24
    assert E.rel_constant("f32", 200704) > 1e-2  # the known limit: vacuous for the weight gradient at size
    assert np.isclose(E.rel_constant("f32", 576), 7e-5, rtol=0.01)


# =============================================================================================================================
# the reducing kernels (BatchNorm training, MC accumulate, KL gradients, global average pool): numpy f32 emulations in the
# summation shape their file headers describe, under HALF of the envelopes of envelope.py; planted faults that the per-element
# checks flag and the rel-L2 / atol bars of the older GPU tests let through
# =============================================================================================================================
F32 = np.float32
BAR_BN_BF16 = 1e-2   # tests/test_gpu_backward.py BN_CASES, bf16
BAR_MC_ATOL = 1e-5   # the MC statistics against torch's f32 softmax
BAR_KL_GRAD = 1e-5   # tests/test_gpu_backward.py: rel-L2 of the KL gradients per tensor


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _bn_sums(v0, v1_of, M, C, rows):
    """btx_bn.hip's two sums per channel: thread (block b, row slot r) takes rows b*rpb + r + k*nblk*rpb in order (f32), the block
    folds its rpb slots in order (f32), the blocks are folded in f64.  rows: the rows the sums visit (a fault drops / repeats one)"""
    cg = C // 8
    rpb = max(256 // cg, 1)
    nblk = min(max(-(-M // (rpb * 8)), 1), 512)
    slab = nblk * rpb
    s0 = np.zeros((slab, C), F32)
    s1 = np.zeros((slab, C), F32)
    for k in range(-(-len(rows) // slab)):
        rw = rows[k * slab:(k + 1) * slab]
        a, b = v0(rw), v1_of(rw)
        s0[:len(rw)] = s0[:len(rw)] + a
        s1[:len(rw)] = _fma(b[0], b[1], s1[:len(rw)])
    s0, s1 = s0.reshape(nblk, rpb, C), s1.reshape(nblk, rpb, C)
    a0, a1 = np.zeros((nblk, C), F32), np.zeros((nblk, C), F32)
    for r in range(rpb):
        a0, a1 = a0 + s0[:, r], a1 + s1[:, r]
    return a0.astype(np.float64).sum(0), a1.astype(np.float64).sum(0)


def emu_bn(x, gamma, beta, eps, dy=None, res=None, relu=False, bf16=False, rows=None, skip_last_group=False, mask_ge=False,
           pivot_row0=False):
    """training-mode BatchNorm forward (+ backward when dy is given) of x [M, C] (f32 numpy holding the dtype-rounded values) as
    btx_bn.hip computes it -> dict(y, mean, invstd, var_unb[, dx, dgamma, dbeta, dres])"""
    M, C = x.shape
    rows = np.arange(M) if rows is None else rows
    piv = x[0].copy() if pivot_row0 else np.median(np.stack([x[0], x[M // 2], x[M - 1]]), axis=0).astype(F32)
    s, q = _bn_sums(lambda rw: x[rw] - piv, lambda rw: (x[rw] - piv, x[rw] - piv), M, C, rows)
    ms = s / M
    m = piv.astype(np.float64) + ms
    var = np.maximum(q / M - ms * ms, 0.0)
    invstd = (1.0 / np.sqrt(var + np.float64(F32(eps)))).astype(F32)
    mean = m.astype(F32)
    g = np.ones(C, F32) if gamma is None else gamma.astype(F32)
    b = np.zeros(C, F32) if beta is None else beta.astype(F32)
    sc = g * invstd
    shift = b - mean * sc
    pre = _fma(np.broadcast_to(sc, x.shape), x, np.broadcast_to(shift, x.shape))
    if skip_last_group:
        pre[:, -8:] = x[:, -8:]
    if res is not None:
        pre = pre + res
    y = np.where(pre < 0, F32(0), pre) if relu else pre
    out = dict(y=_bf(y) if bf16 else y, mean=mean, invstd=invstd, var_unb=(var * M / (M - 1)).astype(F32))
    if dy is None:
        return out
    mask = ((pre >= 0) if mask_ge else (y > 0)).astype(F32) if relu else np.ones_like(x)
    gy = dy * mask
    s, q = _bn_sums(lambda rw: gy[rw], lambda rw: (gy[rw], (x[rw] - mean) * invstd), M, C, rows)
    is64, mu64 = invstd.astype(np.float64), mean.astype(np.float64)
    A = g.astype(np.float64) * is64
    B = -A * is64 * q / M
    D = -A * s / M - B * mu64
    A, B, D = (np.broadcast_to(v.astype(F32), x.shape) for v in (A, B, D))
    dx = _fma(A, gy, _fma(B, x, D))
    out.update(dx=_bf(dx) if bf16 else dx, dgamma=q.astype(F32), dbeta=s.astype(F32), dres=gy)
    return out


BN_EMU_SHAPES = [(2, 8), (3, 2040), (105, 40), (1023, 72), (257, 1024), (256, 1024), (4099, 2048)]


def _bn_inputs(M, C, seed, bf16, mean=0.3, std=1.7):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, dy, res = rn(M, C) * std + mean, rn(M, C), rn(M, C)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.2 * rn(C)
    if bf16:
        x, dy, res = _r(x), _r(dy), _r(res)
    return x, dy, res, gamma, beta


def _bn_check_all(got, x, dy, res, gamma, beta, relu, bf16, half=False):
    """every output of emu_bn against bn_forward64 / bn_backward64 -> {name: Report}"""
    M, C = x.shape
    K = E.bn_chain(M, C)
    f = E.bn_forward64(E.d64(x), gamma, beta, 1e-5, K, residual=E.d64(res) if res is not None else None, relu=relu)
    mask = torch.from_numpy((got["y"] > 0).astype(np.float64)) if relu else None
    bw = E.bn_backward64(E.d64(x), E.d64(dy), f, K, mask=mask)
    M1 = M / (M - 1.0)
    h = 0.5 if half else 1.0  # the f32 arithmetic has to leave half of its share; one bf16 store fills its own
    pairs = [("y", got["y"], f["y"], E.store_rounding(h * f["b_y"], f["y"]) if bf16 else h * f["b_y"]),
             ("save_mean", got["mean"], f["mean"], h * f["d_mean"]), ("save_invstd", got["invstd"], f["invstd"], h * f["d_invstd"]),
             ("var_unb", got["var_unb"], f["var"] * M1, h * (f["dv_stat"] * M1 + E.REF32_UNIT * f["var"] * M1)),
             ("dx", got["dx"], bw["dx"], E.store_rounding(h * bw["b_dx"], bw["dx"]) if bf16 else h * bw["b_dx"]),
             ("dgamma", got["dgamma"], bw["dgamma"], h * (bw["b_dgamma"] + E.REF32_UNIT * bw["dgamma"].abs())),
             ("dbeta", got["dbeta"], bw["dbeta"], h * (bw["b_dbeta"] + E.REF32_UNIT * bw["dbeta"].abs()))]
    return {name: E.check(a, r, b) for name, a, r, b in pairs}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", BN_EMU_SHAPES, ids=lambda s: "%dx%d" % s)
def test_clean_batchnorm_emulation_stays_under_half_the_envelope(shape, bf16):
    M, C = shape
    for relu in (False, True):
        x, dy, res, gamma, beta = _bn_inputs(M, C, 21, bf16)
        res = res if relu else None
        got = emu_bn(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, dy.numpy(), res.numpy() if relu else None, relu, bf16)
        reps = _bn_check_all(got, x, dy, res, gamma, beta, relu, bf16, half=True)
        for name, rep in reps.items():
            print(rep.line("emu bn %dx%d %s%s" % (M, C, name, " res_relu" if relu else ""), "bf16" if bf16 else "f32"))
        assert all(r.ok for r in reps.values()), {k: str(v) for k, v in reps.items() if not v.ok}


@pytest.mark.parametrize("what", ["dropped", "doubled"])
def test_a_row_dropped_or_doubled_in_the_batchnorm_sums_is_flagged_where_rel_l2_is_blind(what):
    """M = 25 088 (8 x 56 x 56), bf16 activations: one row missing from (or counted twice in) the sums moves mean and variance by
    ~1/M.  Every quantity the rel-L2 test of BatchNorm bars at 1e-2 — y, dx, dgamma, dbeta and the running estimates at momentum
    0.1 — stays under that bar; the per-channel statistics leave their envelope and, with integer dy, dbeta is not the exact sum
    any more"""
    M, C = 25088, 64
    x, _, _, gamma, beta = _bn_inputs(M, C, 22, True)
    dyi = E.small_ints((M, C), 23)
    rows = np.delete(np.arange(M), 2500) if what == "dropped" else np.insert(np.arange(M), 2500, 2500)
    clean = emu_bn(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, dyi.numpy(), bf16=True)
    bad = emu_bn(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, dyi.numpy(), bf16=True, rows=rows)
    assert all(r.ok for r in _bn_check_all(clean, x, dyi, None, gamma, beta, False, True).values())
    reps = _bn_check_all(bad, x, dyi, None, gamma, beta, False, True)
    print("bn row %s: save_mean %s | var %s" % (what, reps["save_mean"], reps["var_unb"]))
    assert not reps["save_mean"].ok and reps["save_mean"].violations > 0.9 * C
    assert not reps["var_unb"].ok
    ref_dbeta = E.d64(dyi).sum(0)
    assert E.check_exact(clean["dbeta"], ref_dbeta).ok and not E.check_exact(bad["dbeta"], ref_dbeta).ok
    K = E.bn_chain(M, C)
    f = E.bn_forward64(E.d64(x), gamma, beta, 1e-5, K)
    bw = E.bn_backward64(E.d64(x), E.d64(dyi), f, K)
    g = torch.Generator().manual_seed(27)
    rm0, rv0 = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    rm, _, rv, _ = E.bn_running64(f, rm0, rv0, 0.1)
    bad["rm"] = F32(0.9) * rm0.numpy() + F32(0.1) * bad["mean"]
    bad["rv"] = F32(0.9) * rv0.numpy() + F32(0.1) * bad["var_unb"]
    errs = {k: rel_l2(bad[k], ref.numpy()) for k, ref in (("y", f["y"]), ("dx", bw["dx"]), ("dgamma", bw["dgamma"]),
                                                          ("dbeta", bw["dbeta"]), ("rm", rm), ("rv", rv))}
    print("bn row %s: rel-L2 %s (bar %.0e)" % (what, ", ".join("%s %.2e" % kv for kv in errs.items()), BAR_BN_BF16))
    for k, v in errs.items():
        assert v < BAR_BN_BF16, (k, v)


def test_pivot_of_the_shifted_sums_row_zero_alone_against_the_median_of_three():
    """one row-0 value 300 away from a unit-spread channel (eight channels of 64), M = 25 088, f32: with the pivot taken from row
    0 alone the emulated sums lose more than 1e-4 of the variance of those channels; the median of rows 0, M/2, M-1 keeps it to
    f32 rounding.  The figures printed here are the emulated ones quoted in btx_bn.hip, DESIGN.md and the profile file."""
    g = torch.Generator().manual_seed(131)
    x = torch.randn(25088, 64, generator=g) + 0.3
    x[0, :8] += torch.tensor([300.0, -300.0] * 4)
    M = x.shape[0]
    x64 = x.double()
    unb = (((x64 - x64.mean(0)) ** 2).sum(0) / (M - 1)).numpy()
    err = {}
    for row0 in (True, False):
        got = emu_bn(x.numpy(), None, None, 1e-5, pivot_row0=row0)["var_unb"].astype(np.float64)
        err[row0] = np.abs(got - unb) / unb
        print("emulated variance error, pivot = %s: outlier channels %.3g, other channels %.3g"
              % ("row 0" if row0 else "median of rows 0, M/2, M-1", err[row0][:8].max(), err[row0][8:].max()))
    assert err[True][:8].max() > 1e-4 and err[True][8:].max() < 1e-6
    assert err[False].max() < 1e-6


def test_last_channel_group_left_unnormalised_is_flagged_where_rel_l2_is_blind():
    """C = 2048 on activations that are close to normalised already (what a BatchNorm sees behind another one): the last eight
    channels pass through untouched — 3e-3 rel-L2 of y, under the bf16 bar; every one of their elements is outside the envelope"""
    M, C = 96, 2048
    x, dy, _, _, _ = _bn_inputs(M, C, 24, True, mean=0.02, std=1.05)
    gamma, beta = torch.ones(C), torch.zeros(C)
    bad = emu_bn(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, dy.numpy(), bf16=True, skip_last_group=True)
    rep = _bn_check_all(bad, x, dy, None, gamma, beta, False, True)["y"]
    f = E.bn_forward64(E.d64(x), gamma, beta, 1e-5, E.bn_chain(M, C))
    r = rel_l2(bad["y"], f["y"].numpy())
    print("bn last group unnormalised: %s | rel-L2 %.3g (bar %.0e)" % (rep, r, BAR_BN_BF16))
    assert not rep.ok and rep.index[1] >= C - 8 and rep.violations > 0.5 * 8 * M
    assert r < BAR_BN_BF16, r


def test_relu_mask_taken_as_greater_or_equal_is_flagged_by_the_exact_check():
    """torch's threshold_backward passes the gradient where y > 0.  Three pre-activations are made exactly 0 (the residual
    cancels fma(sc, x, shift) in f32): a mask y >= 0 lets dy through there — three elements of 73 656, 4e-3 in rel-L2 and under
    its 1e-2 bar, and exactly what dres == dy * [y > 0] on the stored y catches"""
    M, C = 1023, 72
    x, _, res, gamma, beta = _bn_inputs(M, C, 25, False)
    dy = E.small_ints((M, C), 26)
    dy[dy == 0] = 1.0
    probe = emu_bn(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5)
    resn = res.numpy().copy()
    where = [(3, 5), (17, 63), (1022, 71)]
    for r_, c_ in where:
        resn[r_, c_] = -probe["y"][r_, c_]
        dy[r_, c_] = 1.0
    for ge in (False, True):
        got = emu_bn(x.numpy(), gamma.numpy(), beta.numpy(), 1e-5, dy.numpy(), resn, True, False, mask_ge=ge)
        assert all(got["y"][r_, c_] == 0 for r_, c_ in where)
        want = dy.numpy() * (got["y"] > 0)
        rep = E.check_exact(got["dres"], want)
        assert rep.ok != ge and rep.violations == (3 if ge else 0), str(rep)
        assert E.check_exact(got["dbeta"], want.astype(np.float64).sum(0)).ok != ge
        assert rel_l2(got["dres"], want) < 1e-2


# ---- MC accumulate ------------------------------------------------------------------------------------------------------------
def _tree64(v):
    """the shuffle tree of a 64-lane wave: lane i += lane i + off for off = 32 .. 1; lane 0 holds the sum"""
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _chains(v):
    """column c of a row belongs to virtual wave (c / 64) % 4, lane c % 64; a lane adds its columns in order -> [4]"""
    C = v.shape[0]
    n = -(-C // 256)
    pad = np.zeros(n * 256, F32)
    pad[:C] = v
    pad = pad.reshape(n, 4, 64)
    s = np.zeros((4, 64), F32)
    for k in range(n):
        s = s + pad[k]
    t = _tree64(s)
    return ((t[0] + t[1]) + t[2]) + t[3]


def emu_mc(x, skip_col=None):
    """btx_mc_accumulate_lanes on x [S, bs, C] (f32 numpy, the dtype-rounded logits) -> (sum_p, sum_p2 [bs, C], ent [bs]) in f32"""
    S, bs, C = x.shape
    sp, sp2, ent = np.zeros((bs, C), F32), np.zeros((bs, C), F32), np.zeros(bs, F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(S):
            for r in range(bs):
                lr = x[s, r]
                ev = np.exp(lr - lr.max()).astype(F32)
                es = ev.copy()
                if skip_col is not None:
                    es[skip_col] = 0
                inv = F32(1) / _chains(es)
                pv = ev * inv
                t = pv * np.log(pv + F32(1e-15))
                sp[r] = sp[r] + pv
                sp2[r] = sp2[r] + pv * pv
                ent[r] = ent[r] + _chains(-t)
    return sp, sp2, ent


def _mc_logits(S, bs, C, seed, bf16, spread=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, bs, C, generator=g) * 2.0
    if spread:
        x = (torch.rand(S, bs, C, generator=g) * 2 - 1) * spread
    return _r(x) if bf16 else x


def _mc_check(got, ref, scale=1.0):
    return {k: E.check(g, ref[k], ref["b_" + k] * scale) for k, g in zip(("sum_p", "sum_p2", "ent"), got)}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1025, 4099])
def test_clean_mc_emulation_stays_under_half_the_envelope(C, bf16):
    x = _mc_logits(3, 2, C, 31 + C, bf16)
    reps = _mc_check(emu_mc(x.numpy()), E.mc_reference(x.double().numpy()), 0.5)
    for k, rep in reps.items():
        print(rep.line("emu mc C=%d %s" % (C, k), "bf16" if bf16 else "f32"))
    assert all(r.ok for r in reps.values()), {k: str(v) for k, v in reps.items() if not v.ok}


def test_clean_mc_emulation_with_wide_logits_and_minus_infinity():
    x = _mc_logits(1, 3, 257, 41, False, spread=80.0)
    x[0, 1, 5:40] = float("-inf")
    ref = E.mc_reference(x.double().numpy())
    assert float((ref["p"] < 1e-45).mean()) > 0.3  # a third of the classes underflow f32 altogether, most of the rest are tiny
    reps = _mc_check(emu_mc(x.numpy()), ref, 0.5)
    assert all(r.ok for r in reps.values()), {k: str(v) for k, v in reps.items() if not v.ok}
    assert (emu_mc(x.numpy())[0][1, 5:40] == 0).all() and (ref["b_sum_p"][1, 5:40] == 0).all()


def test_a_class_column_missing_from_the_softmax_sum_is_flagged_where_atol_is_blind():
    """C = 1000: column 777 (past three strides of 256) never reaches the row sum.  Every probability of the row is 1e-3 too
    large in relative terms — 1e-6 in absolute ones, under the atol 1e-5 of the older test; the relative envelope is 1e-6"""
    x = _mc_logits(1, 2, 1000, 42, False)
    ref = E.mc_reference(x.double().numpy())
    got = emu_mc(x.numpy(), skip_col=777)
    reps = _mc_check(got, ref)
    print("mc column missing: %s" % reps["sum_p"])
    assert not reps["sum_p"].ok and reps["sum_p"].violations > 0.9 * 2000 and not reps["ent"].ok
    assert float(np.abs(got[0] - ref["sum_p"]).max()) < BAR_MC_ATOL


# ---- KL gradients -------------------------------------------------------------------------------------------------------------
def emu_kl_bwd(mu, rho, pm, ps, g, n=None):
    """kl_model_bwd_kernel in f32 numpy; n: the count the mean is scaled by (a fault hands in a neighbour's)"""
    mu, rho, pm, ps = (np.asarray(v, dtype=F32) for v in (mu, rho, pm, ps))
    gn = F32(g) / F32(mu.size if n is None else n)
    sig = np.log1p(np.exp(rho)).astype(F32)
    dsig = F32(1) / (F32(1) + np.exp(-rho).astype(F32))
    ips2 = F32(1) / (ps * ps)
    return gn * (mu - pm) * ips2, gn * (sig * ips2 - F32(1) / sig) * dsig


def _kl_inputs(n, seed, tensor_priors):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, generator=g).numpy()
    rho = (torch.rand(n, generator=g) * 40 - 20).numpy()
    if tensor_priors:
        return mu, rho, (0.3 * torch.randn(n, generator=g)).numpy(), (0.2 + torch.rand(n, generator=g)).numpy()
    return mu, rho, F32(0.1), F32(0.7)


@pytest.mark.parametrize("tensor_priors", [False, True], ids=["scalar-priors", "tensor-priors"])
@pytest.mark.parametrize("n", [1, 3, 2049])
def test_clean_kl_gradient_emulation_stays_under_half_the_envelope(n, tensor_priors):
    mu, rho, pm, ps = _kl_inputs(n, 51 + n, tensor_priors)
    dmu, drho = emu_kl_bwd(mu, rho, pm, ps, 1.7)
    _, rmu, bmu, rrho, brho = E.kl_reference(mu, rho, pm, ps, float(F32(1.7)))
    for name, rep in (("dmu", E.check(dmu, rmu, bmu / 2)), ("drho", E.check(drho, rrho, brho / 2))):
        print(rep.line("emu kl n=%d %s" % (n, name), "f32"))
        assert rep.ok, str(rep)


def test_kl_gradient_scaled_by_a_neighbours_count_is_flagged_where_rel_l2_is_blind():
    """two tensors of 150 001 and 150 000 elements: the first one's gradient divided by the second one's n is 6.7e-6 off in
    every element — under the 1e-5 rel-L2 bar; dmu's envelope is 8 roundings"""
    n = 150001
    mu, rho, pm, ps = _kl_inputs(n, 55, False)
    dmu, drho = emu_kl_bwd(mu, rho, pm, ps, 1.0, n=n - 1)
    _, rmu, bmu, rrho, brho = E.kl_reference(mu, rho, pm, ps, 1.0)
    rep = E.check(dmu, rmu, bmu)
    print("kl neighbour's n: %s | rel-L2 %.3g" % (rep, rel_l2(dmu, rmu)))
    assert not rep.ok and rep.violations > 0.9 * n
    assert rel_l2(dmu, rmu) < BAR_KL_GRAD and rel_l2(drho, rrho) < BAR_KL_GRAD
    assert E.check(emu_kl_bwd(mu, rho, pm, ps, 1.0)[0], rmu, bmu / 2).ok


# ---- global average pool ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [1, 31, 32, 33, 1000])
def test_avgpool_emulation_on_integers_is_exact_and_a_dropped_pixel_group_is_not(hw):
    """32 pixel groups (pixel p belongs to group p % 32), f32 sums, a fixed-order fold: integers make every order exact"""
    x = E.small_ints((3, hw, 72), 61 + hw)
    xn = x.numpy()
    parts = np.stack([xn[:, g::32].sum(1, dtype=F32) if g < hw else np.zeros((3, 72), F32) for g in range(32)])
    s = np.zeros((3, 72), F32)
    for g in range(32):
        s = s + parts[g]
    got = s * (F32(1) / F32(hw))
    for dt in (torch.float32, torch.bfloat16):
        assert E.check_exact(torch.from_numpy(got).to(dt), E.avgpool_exact(x, dt)).ok
    bad = (s - parts[min(hw, 32) - 1]) * (F32(1) / F32(hw))
    assert not E.check_exact(bad, E.avgpool_exact(x, torch.float32)).ok or not parts[min(hw, 32) - 1].any()


def test_reduction_constants_are_the_derived_ones():
    assert E.bn_chain(25088, 64) == 8 + 32 and E.bn_chain(4099, 2048) == 9 + 1 and E.bn_chain(8200, 2048) == 17 + 1
    assert E.bn_chain(257, 1024) == 8 + 2 and E.bn_chain(2, 8) == 1 + 256
    assert list(E.ulp32(np.array([1.0, 0.75, 3.0, 0.0, 1e-45]))) == [2.0 ** -23, 2.0 ** -24, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149]


# =============================================================================================================================
# fused Bayesian LSTM: numpy-f32 emulations of the summation shapes of btx_lstm.hip / btx_lstm_bwd.hip against the per-step
# float64 references of envelope.py (the ones test_gpu_lstm_elementwise.py feeds with the GPU's own operands)
# =============================================================================================================================
LSTM_CASES = [(7, 5, 1, 1), (8, 16, 3, 2), (65, 17, 65, 2), (17, 66, 5, 3), (12, 10, 4, 3)]
LSTM_BAR_FWD = {"f32": 1e-5, "bf16": 1e-2}   # tests/test_gpu_lstm_fused.py
LSTM_BAR_BWD = {"f32": 1e-5, "bf16": 2e-2}   # tests/test_gpu_lstm_train_fused.py
F32 = np.float32


def _nrb(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _sg32(v):  # correctly rounded: the emulation is about the summation shapes, the transcendentals' error is measured on the GPU
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(F32)


def _th32(v):
    return np.tanh(v.astype(np.float64)).astype(F32)


def lstm_problem(I, H, B, T, flip, bias, state, seed, rho_range=(-9.0, 2.0)):
    """parameters, one noise draw per step and the weights a launch samples from them in f32 (what the GPU test probes)"""
    g = np.random.default_rng(seed)
    N = 4 * H
    P = dict(I=I, H=H, B=B, T=T, flip=flip, bias=bias, state=state)
    P["x"] = (0.25 * g.standard_normal((B, T, I))).astype(F32)
    P["h0"] = (0.5 * g.standard_normal((B, H))).astype(F32) if state else None
    P["c0"] = g.standard_normal((B, H)).astype(F32) if state else None
    P["d_hs"], P["d_cs"] = g.standard_normal((B, T, H)).astype(F32), g.standard_normal((B, T, H)).astype(F32)
    for name, K in (("ih", I), ("hh", H)):
        L = dict(mu=(0.1 * g.standard_normal((N, K))).astype(F32), rho=g.uniform(*rho_range, (N, K)).astype(F32),
                 eps=[g.standard_normal((N, K)).astype(F32) for _ in range(T)])
        if bias:
            L.update(mu_b=(0.1 * g.standard_normal(N)).astype(F32), rho_b=g.uniform(*rho_range, N).astype(F32),
                     eps_b=[g.standard_normal(N).astype(F32) for _ in range(T)])
        else:
            L.update(mu_b=None, rho_b=None, eps_b=[None] * T)
        if flip:
            L["s_in"] = [g.choice([-1.0, 1.0], (B, K)).astype(F32) for _ in range(T)]
            L["s_out"] = [g.choice([-1.0, 1.0], (B, N)).astype(F32) for _ in range(T)]
        sig = np.log1p(np.exp(L["rho"].astype(np.float64))).astype(F32)
        sig_b = np.log1p(np.exp(L["rho_b"].astype(np.float64))).astype(F32) if bias else None
        steps = []
        for t in range(T):
            d = sig * L["eps"][t]
            db = sig_b * L["eps_b"][t] if bias else None
            if flip:
                steps.append(dict(mu=L["mu"], D=d, bm=L["mu_b"], bd=db, s_in=L["s_in"][t], s_out=L["s_out"][t]))
            else:
                steps.append(dict(mu=L["mu"] + d, D=None, bm=(L["mu_b"] + db) if bias else None, bd=None, s_in=None, s_out=None))
        L["steps"] = steps
        P[name] = L
    return P


def _steps64(P, name):
    return [E.lstm_layer_step(**s) for s in P[name]["steps"]]


def emu_lstm_linear(inp, L, bf16, drop_k=None, s_out=None):
    """one layer of one step: per 64-chunk four wave partials of 16 sequential FMAs, carried across the chunks and folded in
    wave order; then the bias and the Flipout combine"""
    mu, D = L["mu"], L["D"]
    N, K = mu.shape
    so = L["s_out"] if s_out is None else s_out
    if inp is None:
        v = np.zeros((1, N), F32)
        vd = np.zeros((1, N), F32)
    else:
        B = inp.shape[0]
        xi = _nrb(inp) if bf16 else inp
        w = _nrb(mu) if bf16 else mu
        xd = wd = None
        if D is not None:
            xd, wd = xi * L["s_in"][:B], (_nrb(D) if bf16 else D)
        v, vd = np.zeros((B, N), F32), np.zeros((B, N), F32)
        for wave in range(4):
            acc, accd = np.zeros((B, N), F32), np.zeros((B, N), F32)
            for kc in range(0, K, 64):
                for k in range(kc + 16 * wave, min(kc + 16 * wave + 16, K)):
                    wk = w[None, :, k]
                    if k == drop_k:  # planted fault: the last gate row loses this product
                        wk = wk.copy()
                        wk[0, N - 1] = 0.0
                    acc = _fma(xi[:, k, None], wk, acc)
                    if D is not None:
                        accd = _fma(xd[:, k, None], wd[None, :, k], accd)
            v, vd = v + acc, vd + accd
    if L["bm"] is not None:
        v = v + L["bm"]
    if L["bd"] is not None:
        vd = vd + L["bd"]
    if D is not None or L["bd"] is not None:
        v = v + (so if inp is None else so[:inp.shape[0]]) * vd
    return v


def emu_lstm_forward(P, prec, act_bf16, fault=None):
    bf16 = prec == "bf16"
    B, T, H = P["B"], P["T"], P["H"]
    st = _nrb if act_bf16 else (lambda a: a)
    x = st(P["x"])
    h = st(P["h0"]) if P["state"] else None
    c = st(P["c0"]) if P["state"] else np.zeros((B, H), F32)
    gates, cells, hs, cs = [], [], [], []
    for t in range(T):
        Lh = P["hh"]["steps"][t]
        so = None
        if fault == "s_out_H" and P["flip"]:  # gate 1 of the last batch row reads s_out element b * H + j, not b * 4H + n
            so = Lh["s_out"].copy()
            so[B - 1, H:2 * H] = Lh["s_out"].reshape(-1)[(B - 1) * H:B * H]
        G = emu_lstm_linear(x[:, t], P["ih"]["steps"][t], bf16)
        g4 = G + emu_lstm_linear(h, Lh, bf16, drop_k=H - 1 if fault == "drop_k" else None, s_out=so)
        g4 = np.broadcast_to(g4, (B, 4 * H)).astype(F32)
        i, f, g, o = _sg32(g4[:, :H]), _sg32(g4[:, H:2 * H]), _th32(g4[:, 2 * H:3 * H]), _sg32(g4[:, 3 * H:])
        c = f * c + i * g
        hf = o * _th32(c)
        h = st(hf)
        gates.append(g4), cells.append(c), hs.append(h), cs.append(st(c))
    return dict(gates=np.stack(gates), cells=np.stack(cells), hs=np.stack(hs, 1), cs=np.stack(cs, 1))


def _emu_contract_T(dG, L, bf16):
    """one FMA chain over n in order per output"""
    mu = _nrb(L["mu"]) if bf16 else L["mu"]
    B, N = dG.shape
    acc = np.zeros((B, mu.shape[1]), F32)
    for n in range(N):
        acc = _fma(dG[:, n, None], mu[None, n, :], acc)
    if L["D"] is not None:
        D = _nrb(L["D"]) if bf16 else L["D"]
        gd, accd = dG * L["s_out"][:B], np.zeros_like(acc)
        for n in range(N):
            accd = _fma(gd[:, n, None], D[None, n, :], accd)
        acc = acc + L["s_in"][:B] * accd
    return acc


def emu_lstm_backward(P, fw, prec, act_bf16, fault=None):
    bf16 = prec == "bf16"
    B, T, H, I = P["B"], P["T"], P["H"], P["I"]
    st = _nrb if act_bf16 else (lambda a: a)
    d_hs, d_cs = st(P["d_hs"]), st(P["d_cs"])
    dG, dcc = [None] * T, None
    for t in range(T - 1, -1, -1):
        acc = _emu_contract_T(dG[t + 1], P["hh"]["steps"][t + 1], bf16) if t + 1 < T else np.zeros((B, H), F32)
        dh = acc + d_hs[:, t]
        g4, c = fw["gates"][t], fw["cells"][t]
        i, f, g, o = _sg32(g4[:, :H]), _sg32(g4[:, H:2 * H]), _th32(g4[:, 2 * H:3 * H]), _sg32(g4[:, 3 * H:])
        cp = fw["cells"][t - 1] if t > 0 else (st(P["c0"]) if P["state"] else np.zeros((B, H), F32))
        th = _th32(_nrb(c) if fault == "tanh_bf16_c" else c)
        dc = dh * o * (1 - th * th)
        dc = dc + d_cs[:, t]
        if dcc is not None:
            dc = dc + dcc
        dG[t] = np.concatenate([dc * g * (i * (1 - i)), dc * cp * (f * (1 - f)), dc * i * (1 - g * g), dh * th * (o * (1 - o))], 1)
        dcc = dc * f
        if fault == "dcc_no_f":
            dcc[B - 1, H - 1] = dc[B - 1, H - 1]
        if fault == "dcc_no_f_row":
            dcc[B - 1] = dc[B - 1]
    out = {"dx": st(np.stack([_emu_contract_T(dG[t], P["ih"]["steps"][t], bf16) for t in range(T)], 1))}
    if P["state"]:
        out["dh0"], out["dc0"] = st(_emu_contract_T(dG[0], P["hh"]["steps"][0], bf16)), st(dcc)
    x, hs = st(P["x"]), fw["hs"]
    for name in ("ih", "hh"):
        L = P[name]
        K = L["mu"].shape[1]
        dmu, se = np.zeros((4 * H, K), F32), np.zeros((4 * H, K), F32)
        bm, bs = np.zeros(4 * H, F32), np.zeros(4 * H, F32)
        for t in range(T):
            if name == "ih":
                inp = x[:, t]
            else:
                inp = hs[:, t - 1] if t > 0 else (st(P["h0"]) if P["state"] else np.zeros((B, H), F32))
            if bf16:
                inp = _nrb(inp)
            S = L["steps"][t]
            gd, ind = dG[t], inp
            if P["flip"]:
                gd, ind = dG[t] * S["s_out"], inp * S["s_in"]
            aw, ad = np.zeros((4 * H, K), F32), np.zeros((4 * H, K), F32)
            ab_, abd = np.zeros(4 * H, F32), np.zeros(4 * H, F32)
            for b in range(B):  # a chain over b within a step
                aw = _fma(dG[t][b, :, None], inp[b, None, :], aw)
                ad = _fma(gd[b, :, None], ind[b, None, :], ad)
                ab_, abd = ab_ + dG[t][b], abd + gd[b]
            dmu = dmu + aw                      # a plain add over t
            se = _fma(ad, L["eps"][t], se)      # an FMA over t
            if P["bias"]:
                bm = bm + ab_
                bs = _fma(abd, L["eps_b"][t], bs)
        out[name + ".dmu_w"], out[name + ".drho_w"] = dmu, se * _sg32(L["rho"])
        if P["bias"]:
            sgb = _sg32(L["rho_b"])
            if fault == "drho_bias_neighbour" and name == "hh":
                sgb = sgb.copy()
                sgb[2] = sgb[3]
            out[name + ".dmu_b"], out[name + ".drho_b"] = bm, bs * sgb
    return out


def lstm_new_checks(P, fw, bw, prec, act_bf16):
    """every element of the emulated results against the per-step references -> {check name: Report}, {name: useful fraction}"""
    bf16 = prec == "bf16"
    B, T, H = P["B"], P["T"], P["H"]
    st = _nrb if act_bf16 else (lambda a: a)
    Li, Lh = _steps64(P, "ih"), _steps64(P, "hh")
    x = st(P["x"])
    h0 = st(P["h0"]) if P["state"] else None
    c0 = st(P["c0"]) if P["state"] else None
    reps = {}
    for t in range(T):
        hp = fw["hs"][:, t - 1] if t > 0 else h0
        ref, bnd = E.lstm_gates64(x[:, t], hp, Li[t], Lh[t], bf16)
        reps["gates t=%d" % t] = E.check(fw["gates"][t], ref, bnd)
        c, b_c, h, b_h = E.lstm_cell64(fw["gates"][t], fw["cells"][t - 1] if t > 0 else c0)
        reps["cell t=%d" % t] = E.check(fw["cells"][t], c, b_c)
        reps["c_seq t=%d" % t] = E.check(fw["cs"][:, t], c, E.store_rounding(b_c, c) if act_bf16 else b_c)
        reps["hidden_seq t=%d" % t] = E.check(fw["hs"][:, t], h, E.store_rounding(b_h, h) if act_bf16 else b_h)
    useful = {}
    if bw is not None:
        noise = {n: [(P[n]["eps"][t], P[n]["eps_b"][t]) for t in range(T)] for n in ("ih", "hh")}
        rho = {n: (P[n]["rho"], P[n]["rho_b"]) for n in ("ih", "hh")}
        args = (fw["gates"], fw["cells"], c0, Li, Lh, x, fw["hs"], h0, st(P["d_hs"]), st(P["d_cs"]), noise, rho, bf16)
        ref = E.lstm_bptt64(*args, want_state=P["state"])
        mag = E.lstm_bptt64(*args, want_state=P["state"], absolute=True)
        for k, r in ref.items():
            bnd = r.e
            useful[k] = float((bnd <= E.LSTM_USEFUL * mag[k].v).mean())  # <=: where A is 0 (no c_{t-1}: the f gate) the bound is 0 too
            if act_bf16 and k in ("dx", "dh0", "dc0"):
                bnd = E.store_rounding(bnd, r.v)
            reps[k] = E.check(bw[k], r.v, bnd)
    return reps, useful


def _lstm_chain64(P, bf16):
    """the whole chain in float64 torch autograd, as the existing GPU tests derive it (no teacher forcing): the OLD bar's reference"""
    t64 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    leaf = lambda a: None if a is None else t64(a).requires_grad_()  # noqa: E731
    rb = (lambda t: t + (t.float().to(torch.bfloat16).double() - t).detach()) if bf16 else (lambda t: t)  # noqa: E731
    B, T, H = P["B"], P["T"], P["H"]
    x, h0, c0 = leaf(P["x"]), leaf(P["h0"]), leaf(P["c0"])
    par = {n: [leaf(P[n]["mu"]), leaf(P[n]["rho"]), leaf(P[n]["mu_b"]), leaf(P[n]["rho_b"])] for n in ("ih", "hh")}
    h = h0 if h0 is not None else torch.zeros(B, H, dtype=torch.float64)
    c = c0 if c0 is not None else torch.zeros(B, H, dtype=torch.float64)
    hs, cs = [], []
    for t in range(T):
        g = 0
        for n, inp in (("ih", x[:, t]), ("hh", h)):
            mu, rho, mu_b, rho_b = par[n]
            d = torch.nn.functional.softplus(rho) * t64(P[n]["eps"][t])
            db = None if mu_b is None else torch.nn.functional.softplus(rho_b) * t64(P[n]["eps_b"][t])
            if P["flip"]:
                out = rb(inp) @ rb(mu).t()
                pert = (rb(inp) * t64(P[n]["s_in"][t])) @ rb(d).t()
                if mu_b is not None:
                    out, pert = out + mu_b, pert + db
                out = out + pert * t64(P[n]["s_out"][t])
            else:
                out = rb(inp) @ rb(mu + d).t()
                if mu_b is not None:
                    out = out + mu_b + db
            g = g + out
        i, f = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H])
        gg, o = torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h), cs.append(c)
    hs, cs = torch.stack(hs, 1), torch.stack(cs, 1)
    ((hs * t64(P["d_hs"])).sum() + (cs * t64(P["d_cs"])).sum()).backward()
    out = {"hs": hs.detach(), "cs": cs.detach(), "dx": x.grad}
    if h0 is not None:
        out["dh0"], out["dc0"] = h0.grad, c0.grad
    for n in ("ih", "hh"):
        for k, p in zip(("dmu_w", "drho_w", "dmu_b", "drho_b"), par[n]):
            if p is not None:
                out[n + "." + k] = p.grad
    return out


def lstm_old_bar(P, fw, bw, prec):
    """the largest rel-L2 over bar of the existing tests -> (ratio, name)"""
    ref = _lstm_chain64(P, prec == "bf16")
    worst = (0.0, None)
    for k, r in ref.items():
        got, bar = (fw[k], LSTM_BAR_FWD[prec]) if k in ("hs", "cs") else (bw[k], LSTM_BAR_BWD[prec])
        worst = max(worst, (rel_l2(np.asarray(got, dtype=np.float64), r.numpy()) / bar, k))
    return worst


_LSTM_CLEAN = {}


@pytest.mark.parametrize("flip", [False, True], ids=["reparam", "flipout"])
@pytest.mark.parametrize("case", LSTM_CASES, ids=lambda c: "I%d-H%d-B%d-T%d" % c)
def test_lstm_clean_emulation_stays_under_half_of_every_bound(case, flip):
    """forward gates, cell / hidden state and every gradient element, both precisions and activation dtypes; and the backward
    bound is useful: below LSTM_USEFUL * A (before a bf16 store) on at least 99 % of the elements of every output"""
    worst, least = 0.0, 1.0
    for prec in ("f32", "bf16"):
        for act_bf16 in (False, True):
            for bias, state in ((True, True), (False, False)):
                P = lstm_problem(*case, flip, bias, state, seed=11)
                fw = emu_lstm_forward(P, prec, act_bf16)
                bw = emu_lstm_backward(P, fw, prec, act_bf16)
                reps, useful = lstm_new_checks(P, fw, bw, prec, act_bf16)
                for k, r in reps.items():
                    # a bf16 store is ONE rounding, and one rounding reaches its own bound u |ref| (the K = 1 remark of
                    # envelope.py): only the derived part of a bound can be asked to leave half of it unused
                    stored = act_bf16 and k.split(" ")[0] in ("c_seq", "hidden_seq", "dx", "dh0", "dc0")
                    assert r.worst <= (1.0 if stored else 0.5), (prec, act_bf16, bias, state, k, str(r))
                    if not stored:
                        worst = max(worst, r.worst)
                for k, u in useful.items():
                    assert u >= 0.99, (prec, act_bf16, bias, state, k, u)
                    least = min(least, u)
    print("lstm emulation %s %s: worst err/bound %.3g; backward bound < %.0e A on >= %.4f of the elements"
          % (case, "flipout" if flip else "reparam", worst, E.LSTM_USEFUL, least))


LSTM_FAULTS = [  # (fault, family is Flipout, case, precision, with (h0, c0))
    ("drop_k", False, (17, 66, 5, 3), "bf16", True),
    ("tanh_bf16_c", False, (65, 17, 65, 2), "bf16", True),
    ("drho_bias_neighbour", False, (17, 66, 5, 3), "bf16", True),
    ("dcc_no_f", False, (65, 17, 65, 2), "bf16", False),
    ("s_out_H", True, (65, 17, 65, 2), "bf16", True),
]


@pytest.mark.parametrize("fault,flip,case,prec,state", LSTM_FAULTS, ids=[f[0] for f in LSTM_FAULTS])
def test_lstm_planted_fault_passes_the_old_bar_and_fails_the_new_check(fault, flip, case, prec, state):
    """drop_k: the product k = K - 1 missing from the recurrent sum of the last gate row; tanh_bf16_c: the backward takes tanh of
    the bf16-rounded cell state; drho_bias_neighbour: one drho_bias entry scaled by its neighbour's sigmoid(rho); dcc_no_f: the
    dc carry of the last batch row misses f_t at one hidden unit; s_out_H: one gate's s_out indexed with H for 4H at the last
    batch row.  The old bar is both existing files': rel-L2 of hidden_seq / c_seq at 1e-2 and of every gradient at 2e-2 (bf16).
    Planted on ALL gate rows (drop_k), the whole batch row with (h0, c0) (dcc_no_f: dc0) or all batch rows (s_out_H) the same
    faults move rel-L2 to 9, 1.5 and 8 times the old bar: those forms are left out, the old bar catches them."""
    # rho around -3 as the layers initialise it: the setting of the existing tests, whose bar this is about
    P = lstm_problem(*case, flip, True, state, seed=5, rho_range=(-3.3, -2.7))
    fw = emu_lstm_forward(P, prec, False, fault=fault)
    bw = emu_lstm_backward(P, fw, prec, False, fault=fault)
    old, name = lstm_old_bar(P, fw, bw, prec)
    reps, _ = lstm_new_checks(P, fw, bw, prec, False)
    bad = {k: r for k, r in reps.items() if not r.ok}
    print("lstm fault %s: old bar reaches %.3g of its limit (%s); new checks outside: %s"
          % (fault, old, name, ", ".join("%s x%.3g" % (k, r.worst) for k, r in bad.items())))
    assert old <= 1.0, (fault, old, name)
    assert bad, fault
