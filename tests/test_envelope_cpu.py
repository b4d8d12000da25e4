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
