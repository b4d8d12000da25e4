"""GPU: the fused Bayesian GRU sequence (btx_gru.hip) element by element against float64.

The float64 model of step t is built from the materialised noise (ih / hh .materialize_noise at index s + t) and is fed the GPU's
own h_{t-1}, so errors do not compound across steps.  The bound is derived, nothing is fitted:

  per half       gi, gh: the dot-product envelope of envelope.py (E.bound) with K = Kr and the fused kernels' sampled-weight
                 constant DELTA_W_LSTM (the same sampler functions); a half that a path really STORES in bf16 — the eager loop's
                 Linear outputs under bf16 activations — carries that store rounding, the fused path keeps both halves in f32
  r, z           sigmoid is 1/4-Lipschitz: b = (b_gi + b_gh + u |gi + gh|) / 4 + SIGM_ULP 2^-23 r
  n              tanh is 1-Lipschitz: b = b_gi + r b_gh + (|gh_n| + b_gh) b_r + 2u (|gi_n| + |r gh_n|) + TANH_ULP 2^-23 |n|
  h              (1 - z) n + z h_prev: b = |1 - z| b_n + (|n| + |h_prev| + b_n) b_z + 3u (|(1 - z) n| + |z h_prev|)
  store          bf16 activations: E.store_rounding on top                                              (u = 2^-24)

profiles/gru_envelope.txt holds the printed figures of the first run."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import envelope as E
import poison as P

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3, 5, 10),    # Kr padding on the input side; H not a multiple of the 4 units of a workgroup; a ragged batch block
          (65, 2, 8, 12),   # a second batch block with one row
          (2, 3, 70, 72)]   # more than one 64-wide K chunk on both the projection and the step
KINDS = ["Reparameterization", "Flipout"]
CFGS = [("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"), ("f32", "bf16")]   # (precision, activation dtype): every instantiation
S0, SEED = 5, 4711
_ids = dict(ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else v)
_LAYERS = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _adt(act):
    return torch.bfloat16 if act == "bf16" else torch.float32


def _layer(kind, shape):
    """(layer, x, h0) of one (kind, shape): built once and shared, never changed"""
    if (kind, shape) in _LAYERS:
        return _LAYERS[kind, shape]
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    (B, T, I, H), dev = shape, _dev()
    bt.manual_seed(SEED)
    g = torch.Generator().manual_seed(100 * KINDS.index(kind) + SHAPES.index(shape))
    layer = getattr(L, "GRU" + kind)(I, H).to(dev).eval()
    bt.assign_layer_ids(layer, start=950)
    with torch.no_grad():
        for lin in (layer.ih, layer.hh):
            for p in (lin.mu_weight, lin.mu_bias):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            for p in (lin.rho_weight, lin.rho_bias):   # the rho range of profiles/elementwise_envelope.txt
                p.copy_(torch.rand(p.shape, generator=g) * 11.0 - 9.0)
    x, h0 = (0.25 * torch.randn(B, T, I, generator=g)).to(dev), (0.5 * torch.randn(B, H, generator=g)).to(dev)
    _LAYERS[kind, shape] = (layer, x, h0)
    return _LAYERS[kind, shape]


def _half64(lin, s, inp, prec, stored_bf16):
    """one Linear layer at sample index s in float64 -> (value, bound) [B, 3H]"""
    mu, rho = lin._w()
    nz = lin.materialize_noise(s, tuple(inp.shape), (inp.shape[0], mu.shape[0]), torch.float32)
    ref, A, Ab = E.reference_forward(inp, mu, rho, nz["eps_w"], lin.mu_bias, lin.rho_bias, nz.get("eps_b"), nz.get("sign_in"),
                                     nz.get("sign_out"), dict(kind="linear"))
    Kr = (inp.shape[1] + 7) // 8 * 8
    return E._np(ref), E.bound(A, prec, Kr, ref=ref, A_bias=Ab, store_bf16=stored_bf16, delta_w=E.DELTA_W_LSTM)


def _cell64(gi, bi, gh, bh, hp):
    """the gates of the module docstring: (h, bound) float64 from the two halves, their bounds and the exact h_prev"""
    H = gi.shape[1] // 3
    q = lambda a, k: a[:, k * H:(k + 1) * H]  # noqa: E731
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    es, et, u = E.SIGM_ULP * E.ACC_UNIT, E.TANH_ULP * E.ACC_UNIT, E.REF32_UNIT
    gate, b_gate = [], []
    for k in (0, 1):
        a = q(gi, k) + q(gh, k)
        gate.append(sig(a))
        b_gate.append(0.25 * (q(bi, k) + q(bh, k) + u * np.abs(a)) + es * gate[k])
    (r, z), (b_r, b_z) = gate, b_gate
    n = np.tanh(q(gi, 2) + r * q(gh, 2))
    b_n = q(bi, 2) + r * q(bh, 2) + (np.abs(q(gh, 2)) + q(bh, 2)) * b_r + 2 * u * (np.abs(q(gi, 2)) + np.abs(r * q(gh, 2))) + et * np.abs(n)
    h = (1 - z) * n + z * hp
    b_h = np.abs(1 - z) * b_n + (np.abs(n) + np.abs(hp) + b_n) * b_z + 3 * u * (np.abs((1 - z) * n) + np.abs(z * hp))
    return h, b_h


def _check_sequence(layer, x, h0, hs, prec, act, halves_stored=False, exact_halves=False):
    """every element of hidden_seq [B, T, H] against the per-step model -> worst err / bound; asserts inside"""
    worst = 0.0
    for t in range(x.shape[1]):
        hp = hs[:, t - 1] if t > 0 else (h0 if h0 is not None else torch.zeros_like(hs[:, 0]))
        gi, bi = _half64(layer.ih, S0 + t, x[:, t], prec, halves_stored)
        gh, bh = _half64(layer.hh, S0 + t, hp, prec, halves_stored)
        if exact_halves:
            bi, bh = np.zeros_like(bi), np.zeros_like(bh)
        h, b = _cell64(gi, bi, gh, bh, E._np(hp))
        rep = E.check(hs[:, t], h, E.store_rounding(b, h) if act == "bf16" else b)
        assert rep.ok, (t, str(rep))
        worst = max(worst, rep.worst)
    return worst


def _run(layer, x, h0, prec, fused):
    import bayesian_torch_amd as bt
    bt.set_precision(prec)
    layer.fused_sequence = fused
    bt.set_sample_index(layer, S0)
    try:
        with torch.no_grad():
            hs, h_T, kl = layer(x, h0)
    finally:
        bt.set_precision("f32")
        layer.fused_sequence = False
    assert torch.equal(h_T, hs[:, -1]) and hs.dtype == x.dtype and layer.ih._btx_sample == S0 + x.shape[1]
    return hs, kl


@pytest.mark.parametrize("shape", SHAPES, **_ids)
@pytest.mark.parametrize("cfg", CFGS, **_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_fused_and_eager_every_element_inside_the_envelope(kind, cfg, shape):
    """the same seed and index through both routes, with h0 given and h0 = None: every element of each inside the envelope around
    the same float64 model (the summation orders differ, so the bits may).  The eager loop's halves are Linear outputs in the
    activation dtype: under bf16 activations their bound carries that store, which the fused path does not have."""
    (prec, act), (layer, x, h0) = cfg, _layer(kind, shape)
    x, h0 = x.to(_adt(act)), h0.to(_adt(act))
    for state in (h0, None):
        hf, klf = _run(layer, x, state, prec, fused=True)
        he, kle = _run(layer, x, state, prec, fused=False)
        wf = _check_sequence(layer, x, state, hf, prec, act)
        we = _check_sequence(layer, x, state, he, prec, act, halves_stored=act == "bf16")
        assert torch.equal(klf, kle)   # the per-step KL terms in the eager order
        print("GRU%s B%d T%d I%d H%d prec %s act %s h0 %s: worst err/bound fused %.3g, eager %.3g"
              % ((kind,) + shape + (prec, act, state is not None, wf, we)))


@pytest.mark.parametrize("shape", SHAPES, **_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_exact_preactivations(kind, shape):
    """small-integer x, dyadic mu / h0, rho = -200 (sigma = 0): both halves are exact in f32 and bf16, so their bound is ZERO and only
    expf / tanhf and the store are left of the envelope (one step: h_1 is no longer dyadic).  E.check_exact judges the run whose
    gates are exact in any arithmetic — zero x, biases and W_hh: sigm(0) = 1/2, tanh(0) = 0, h = h0 / 2."""
    from bayesian_torch_amd import layers as L
    (B, _, I, H), dev, n = shape, _dev(), 10 * SHAPES.index(shape)
    layer = getattr(L, "GRU" + kind)(I, H).to(dev).eval()
    with torch.no_grad():
        for k, lin in enumerate((layer.ih, layer.hh)):
            lin.mu_weight.copy_(E.dyadic(lin.mu_weight.shape, 800 + n + k, shift=11))
            lin.mu_bias.copy_(E.dyadic(lin.mu_bias.shape, 810 + n + k, shift=9))
            lin.rho_weight.fill_(-200.0), lin.rho_bias.fill_(-200.0)
    x, h0 = E.small_ints((B, 1, I), 820 + n).to(dev), E.dyadic((B, H), 830 + n).to(dev)
    for prec, act in CFGS:
        xa, ha = x.to(_adt(act)), h0.to(_adt(act))
        hs, _ = _run(layer, xa, ha, prec, fused=True)
        _check_sequence(layer, xa, ha, hs, prec, act, exact_halves=True)
    with torch.no_grad():
        for p_ in (layer.ih.mu_bias, layer.hh.mu_bias, layer.hh.mu_weight):
            p_.zero_()
    for prec, act in CFGS:
        ha = h0.to(_adt(act))
        hs, _ = _run(layer, torch.zeros_like(x).to(_adt(act)), ha, prec, fused=True)
        rep = E.check_exact(hs[:, 0], (E.d64(ha) / 2).to(_adt(act)))
        assert rep.ok, (prec, act, str(rep))


@pytest.mark.parametrize("shape", SHAPES, **_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_lanes_are_bit_equal_to_single_calls(kind, shape):
    import bayesian_torch_amd as bt
    (layer, x, h0), B, idx = _layer(kind, shape), shape[0], [5, 11, 12]
    xl = torch.cat([x, x.flip(0), 2 * x])
    layer.fused_sequence = True
    try:
        with torch.no_grad():
            single_s, single_l = [], []
            for l, s in enumerate(idx):
                bt.set_sample_index(layer, s)
                single_s.append(layer(x, h0)[0])
                bt.set_sample_index(layer, s)
                single_l.append(layer(xl[l * B:(l + 1) * B], h0)[0])
            bt.set_sample_lanes(layer, idx, batch=B)
            shared = layer(x, h0)[0]
            bt.set_sample_lanes(layer, idx, batch=B)
            per_lane = layer(xl, h0)[0]
    finally:
        bt.set_sample_lanes(layer, None)
        layer.fused_sequence = False
    assert P.bits_equal(shared, torch.cat(single_s)) and P.bits_equal(per_lane, torch.cat(single_l))


class _Net(nn.Module):
    def __init__(self, i, h):
        super().__init__()
        self.gru = nn.GRU(i, h, batch_first=True)
        self.fc = nn.Linear(h, 4)

    def forward(self, x):
        return self.fc(self.gru(x)[0][:, -1])


PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_mc_replays_equal_mc_forward_lanes(kind):
    """several replays of a captured 3-lane graph against mc.mc_forward(lanes=3) at the same sample indices"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.models import fuse_model
    (B, T, I, H), dev = SHAPES[0], _dev()
    bt.set_precision("f32")
    torch.manual_seed(0)
    m = _Net(I, H)
    bt.dnn_to_bnn(m, dict(PRIOR, type=kind))
    m = m.to(dev).eval()
    assert fuse_model(m) == 1 and m.gru.fused_sequence
    x = torch.randn(B, T, I, device=dev)
    want = {off: mc.mc_forward(m, x, 3, sample_offset=off, lanes=3) for off in (5, 40)}
    g = mc.GraphedMC(m, x.clone(), lanes=3, lane_mode="launch")
    try:
        for off in (5, 40, 5):
            g.packed.zero_()
            g.run_many([off, off + 1, off + 2])
            torch.cuda.synchronize()
            assert P.bits_equal(g.packed, want[off]), off
    finally:
        g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_off_grid_and_poisoned_buffers_give_the_same_bits(kind):
    """X, h0 and hidden_seq as views 4 bytes off a 16-byte boundary (bf16 and f32 activations), and every fresh buffer — hidden_seq
    and the workspace — pre-filled with 0xFF / 0x7F bytes: the bits of the plain call"""
    from bayesian_torch_amd import _lib, functional as BF, rng
    from test_gpu_alignment import off_grid
    (layer, x, h0), (B, T, _, H) = _layer(kind, SHAPES[0]), SHAPES[0]
    k = _lib.KIND_FLIPOUT if kind == "Flipout" else _lib.KIND_REPARAM
    par = lambda lin: tuple(p.detach() for p in lin._w()) + (lin.mu_bias.detach(), lin.rho_bias.detach(), lin._btx_layer_id, S0, None)  # noqa: E731
    for act in ("f32", "bf16"):
        xa, ha = x.to(_adt(act)), h0.to(_adt(act))
        call = lambda xx, hh, out=None: BF.gru_hip(k, xx, par(layer.ih), par(layer.hh), rng.seed(), prec="f32", h0=hh, out=out,  # noqa: E731
                                                   kl_terms=(layer.ih.kl_loss(), layer.hh.kl_loss()))
        plain = call(xa, ha)
        out = off_grid(torch.zeros(B, T, H, dtype=xa.dtype, device=xa.device), 4)
        got = call(off_grid(xa, 4), off_grid(ha, 4), out)
        assert got[0].data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 4 and P.bits_equal(got, plain), act
        for byte in P.PATTERNS:
            with P.poisoned(byte) as rec:
                got = call(xa, ha)
            assert rec.bytes > 0 and P.bits_equal(got, plain), (act, byte)
