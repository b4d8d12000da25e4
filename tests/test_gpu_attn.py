"""GPU: the fused attention core (btx_attn.hip) element by element against float64, and the attention layers on it.

The float64 reference is attention on the GPU's own q, k, v, so nothing compounds.  The bound is derived, nothing is fitted
(u = 2^-8, the bf16 unit; S = the 2^-23 accumulation unit of envelope.py):

  scores   D_j = (c_op + (D + 8) S) scale sum_d |q_d||k_jd|,  c_op = 2u + u^2 where f32 activations are rounded for a bf16 MFMA, else 0
  p_j      relative error rho = expm1(2 max_j D_j) + (C_EXP + Tk + 2 key_tiles + 8) S    (the maximum shifts every exponent alike; the
           running sum has Tk terms and is rescaled once per key tile; C_EXP: the device's exp2 chain, below)
  output   |dO_d| <= (rho + c_pv) sum_j p_j |v_jd|,  c_pv = (2u + u^2 where P and V are bf16 operands, else 0) + (Tk + 8) S
  store    bf16 activations: E.store_rounding on top

C_EXP is twice the error of the kernel's own exponential chain (one f32 multiply by scale * log2 e, v_exp_f32, the sum and the final
division) measured through the kernel against float64: test_exp_error_is_half_of_c_exp prints the measurement, profiles/attn_envelope.txt
holds the first run's figures with the worst got / bound ratio of every configuration."""
import pytest
import torch
import torch.nn as nn

import envelope as E
import poison as P

pytestmark = pytest.mark.gpu

CFGS = [("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"), ("f32", "bf16")]   # (precision, activation dtype): every instantiation
DIMS = [32, 64, 128]
SHAPES = [(2, 3, 1), (2, 3, 7), (3, 2, 65), (2, 2, 130), (2, 3, 197)]   # (rows, heads, T): T straddles the 32 / 64-key and 128-query tiles
MASKS = ["none", "causal", "pad"]
C_EXP = 16.0      # 2 x the measured 7.79 ulp, rounded up (profiles/attn_envelope.txt)
F32_CAP = 1e-4    # the f32 / f32 bound must stay below this fraction of sum_j p_j |v_jd|: a dropped or doubled key moves it by >= 5e-3
_ids = dict(ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
_CASES = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_adt = lambda act: torch.bfloat16 if act == "bf16" else torch.float32  # noqa: E731


def _case(D, shape, act):
    """(packed qkv [rows, T, 3E] in the activation dtype, ragged key-padding mask [rows, T]) of one case: built once, never changed"""
    key = (D, shape, act)
    if key not in _CASES:
        (R, H, T), dev = shape, _dev()
        g = torch.Generator().manual_seed(1000 * D + 10 * T + R)
        # q, k = 0.3 randn keeps sum |q||k| scale <= 1.2 at D = 128, for which the f32 bound is 8.5e-5 of sum p |v|: under F32_CAP
        qkv = torch.cat([0.3 * torch.randn(R, T, 2 * H * D, generator=g), torch.randn(R, T, H * D, generator=g)], dim=-1)
        lens = [max(1, T - (2 * r + 1) * T // 5) for r in range(R)]   # a ragged length per row, never empty
        pad = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
        _CASES[key] = (qkv.to(dev, _adt(act)), pad.to(dev))
    return _CASES[key]


def _heads64(qkv, H):
    R, T, E3 = qkv.shape
    return qkv.double().reshape(R, T, 3, H, E3 // 3 // H).permute(2, 0, 3, 1, 4)   # q, k, v: [rows, heads, T, D]


def _masked(mask, R, T, pad, dev):
    m = torch.zeros(R, 1, T, T, dtype=torch.bool, device=dev)
    if mask == "causal":
        m = m | torch.ones(T, T, dtype=torch.bool, device=dev).triu(1)
    if mask == "pad":
        m = m | pad[:, None, None, :]
    return m


def _ref_bound(q, k, v, masked, prec, act):
    """float64 attention of q, k, v [rows, heads, T, D] -> (ref, bound, sum_j p_j |v_jd|) as [rows, T, heads * D]"""
    D, Tk = q.shape[-1], k.shape[-2]
    scale, u, S = D ** -0.5, E.U_BF16, E.ACC_UNIT
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(masked, float("-inf"))
    dead = s.amax(-1, keepdim=True) == float("-inf")
    p = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    ref, A = p @ v, p @ v.abs()
    c_op = 2 * u + u * u if (prec == "bf16" and act == "f32") else 0.0
    delta = ((c_op + (D + 8) * S) * scale * (q.abs() @ k.abs().transpose(-1, -2))).masked_fill(masked, 0.0)
    tiles = -(-Tk // (64 if prec == "bf16" else 32))
    rho = torch.expm1(2 * delta.amax(-1, keepdim=True)) + (C_EXP + Tk + 2 * tiles + 8) * S
    c_pv = (2 * u + u * u if prec == "bf16" else 0.0) + (Tk + 8) * S
    merge = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)  # noqa: E731
    ref, bound, A = merge(ref), merge((rho + c_pv) * A), merge(A)
    if act == "bf16":
        bound = torch.as_tensor(E.store_rounding(bound, ref), device=ref.device)
    return ref, bound, A


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_every_element_inside_the_envelope(cfg, D, shape, mask):
    from bayesian_torch_amd import functional as BF
    (prec, act), (R, H, T) = cfg, shape
    qkv, pad = _case(D, shape, act)
    got = BF.attn_hip(qkv, H, pad if mask == "pad" else None, causal=mask == "causal", prec=prec)
    q, k, v = _heads64(qkv, H)
    ref, bound, A = _ref_bound(q, k, v, _masked(mask, R, T, pad, qkv.device), prec, act)
    rep = E.check(got, ref, bound)
    print("attn %s/%s D=%d %s %s: %s" % (prec, act, D, shape, mask, rep))
    if cfg == ("f32", "f32"):
        assert bool((bound <= F32_CAP * A).all()), "the f32 bound itself is too wide to see a dropped key"
    assert got.shape == (R, T, H * D) and got.dtype == qkv.dtype and rep.ok, str(rep)


def test_exp_error_is_half_of_c_exp():
    """the kernel's exponential chain through the kernel itself: two keys, s_0 = 0 and s_1 = -x, v_0 = 0 and v_1 = 1, so
    out = e^-x / (1 + e^-x) for 4096 values of x in [0, 16] (D = 64: q = x / 8 at d = 0, k_1 = -64, scale = 1 / 8, every product exact)"""
    from bayesian_torch_amd import functional as BF
    dev, D, n = _dev(), 64, 4096
    x = torch.linspace(0.0, 16.0, n, device=dev).float()
    q, k, v = torch.zeros(1, n, D, device=dev), torch.zeros(1, 2, D, device=dev), torch.zeros(1, 2, D, device=dev)
    q[0, :, 0], k[0, 1, 0], v[0, 1, 0] = x / 8, -64.0, 1.0
    got = BF.attn_hip((q, k, v), 1, prec="f32")[0, :, 0].double()
    want = torch.sigmoid(-(q[0, :, 0].double() * 8.0))
    ulp = float(((got - want).abs() / (want * E.ACC_UNIT)).max())
    print("attn exp chain: max error %.3f ulp (2^-23 relative) over x in [0, 16]; C_EXP = %.1f" % (ulp, C_EXP))
    assert 2 * ulp <= C_EXP


@pytest.mark.parametrize("cfg", CFGS, **_ids)
@pytest.mark.parametrize("D", DIMS)
def test_exact_probes(cfg, D):
    """p is exactly 1 for Tk = 1 and for query 0 under the causal mask: v_0 as the operand dtype holds it, bit for bit; a row whose
    keys are all masked: zeros"""
    from bayesian_torch_amd import functional as BF
    (prec, act), H = cfg, 3
    held = lambda v: (v.bfloat16() if prec == "bf16" else v).to(_adt(act))  # noqa: E731
    one, _ = _case(D, SHAPES[0], act)
    got = BF.attn_hip(one, H, prec=prec)
    assert P.bits_equal(got, held(one[..., 2 * H * D:]))
    qkv, pad = _case(D, SHAPES[1], act)
    got = BF.attn_hip(qkv, H, causal=True, prec=prec)
    assert P.bits_equal(got[:, 0], held(qkv[:, 0, 2 * H * D:]))
    dead = pad.clone()
    dead[0] = True
    got = BF.attn_hip(qkv, H, dead, prec=prec)
    assert not bool(got[0].any()) and bool(got[1].any()) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_masked_memory_and_off_grid_views_give_the_same_bits(cfg):
    """k / v rows of padded keys filled with NaN and with 0x7F bytes; q / k / v as views of one packed buffer 4 bytes off the 16-byte
    grid; [T, rows, E] strides for input and output: the bits of the dense call"""
    from bayesian_torch_amd import functional as BF
    from test_gpu_alignment import off_grid
    (prec, act), D, (R, H, T) = cfg, 64, SHAPES[2]
    qkv, pad = _case(D, SHAPES[2], act)
    E_ = H * D
    zeroed = qkv.clone()
    zeroed[..., E_:][pad] = 0
    want = BF.attn_hip(zeroed, H, pad, prec=prec)
    assert bool(torch.isfinite(want).all())
    for fill in (float("nan"), None):
        dirty = qkv.clone()
        if fill is None:
            dirty.view(torch.uint8).reshape(R, T, -1)[:, :, E_ * qkv.element_size():][pad] = 0x7F
        else:
            dirty[..., E_:][pad] = fill
        assert P.bits_equal(BF.attn_hip(dirty, H, pad, prec=prec), want), fill
    plain = BF.attn_hip(qkv, H, causal=True, prec=prec)
    off = off_grid(qkv, 4)
    out = off_grid(torch.zeros_like(plain), 4)
    assert off.data_ptr() % 16 == 4 and P.bits_equal(BF.attn_hip(off, H, causal=True, prec=prec, out=out), plain)
    tb = qkv.transpose(0, 1).contiguous().transpose(0, 1)   # [rows, T, 3E] logically, [T, rows, 3E] in memory
    out = torch.zeros(T, R, E_, dtype=qkv.dtype, device=qkv.device).transpose(0, 1)
    assert not tb.is_contiguous() and P.bits_equal(BF.attn_hip(tb, H, causal=True, prec=prec, out=out).contiguous(), plain)


# ---- layer level: a Bayesian Linear embedding, a converted TransformerEncoderLayer, a Linear head -------------------------------
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Linear(16, 64)
        self.enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(64, 2, 128, dropout=0.0, batch_first=True), 1)
        self.head = nn.Linear(64, 8)

    def forward(self, x):
        # a per-token head, read at the first token: every Linear sees batch * T > 256 rows, where single-sample and lane launches share
        # one kernel family (a Linear of <= 256 rows samples in registers when it runs alone: another summation order)
        return self.head(self.enc(self.embed(x)))[:, 0]


PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def _net(kind, fused=True):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    bt.set_precision("f32")
    bt.manual_seed(77)
    torch.manual_seed(0)
    m = _Net()
    bt.dnn_to_bnn(m, dict(PRIOR, type=kind))
    m = m.to(_dev()).eval()
    attn = m.enc.layers[0].self_attn
    if fused:
        assert fuse_model(m) >= 1 and attn.fused_attention
    return m, attn, torch.randn(5, 70, 16, generator=torch.Generator().manual_seed(3)).to(_dev())


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_lanes_graphs_and_the_composite(kind):
    """mc_forward's lanes against single forwards and a GraphedMC replay against the eager call, bit for bit; the fused core against
    the composite inside the sum of both bounds; nn.TransformerEncoder in eval mode calls the module (no fast path, no AttributeError)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    m, attn, x = _net(kind)
    idx = [5, 11, 12]
    try:
        with torch.no_grad():
            single = []
            for s in idx:
                bt.set_sample_index(m, s)
                single.append(m(x))
            bt.set_sample_lanes(m, idx, batch=x.shape[0])
            lanes = m(x)
    finally:
        bt.set_sample_lanes(m, None)
    assert P.bits_equal(lanes, torch.cat(single))
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
    # the attention module alone at sigma = 0: both paths see the same qkv, so their outputs differ by the two core errors pushed
    # through out_proj, |W| (b_fused + b_composite), and out_proj's own f32 accumulation
    with torch.no_grad():
        for lin in (attn.in_proj, attn.out_proj):
            lin.rho_weight.fill_(-200.0)
            lin.rho_bias.fill_(-200.0)
        h = torch.randn(3, 70, 64, generator=torch.Generator().manual_seed(4)).to(x.device)
        fused = attn(h, h, h)[0]
        attn.fused_attention = False
        comp = attn(h, h, h)[0]
        q, k, v = _heads64(attn.in_proj(h, return_kl=False), 2)
        _, b, A = _ref_bound(q, k, v, _masked("none", 3, 70, None, h.device), "f32", "f32")
        W = attn.out_proj.mu_weight.double().abs()
        bound = 2 * b @ W.t() + 2 * E.rel_constant("f32", 64) * (A @ W.t()) + 4 * E.REF32_UNIT * comp.double().abs()
    rep = E.check(fused, comp.double(), bound)
    print("attn %s fused vs composite: %s" % (kind, rep))
    assert rep.ok, str(rep)


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_training_takes_the_composite_and_fills_every_gradient(kind):
    m, attn, x = _net(kind)
    m.train()
    m(x.requires_grad_()).square().mean().backward()
    for name, p in m.named_parameters():
        if name.rsplit(".", 1)[-1].startswith(("mu_", "rho_")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
