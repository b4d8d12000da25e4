"""GPU: fused attention training (btx_attn_fwd_train + btx_attn_bwd) — dq, dk, dv against float64, bit contracts,
masked memory, and the attention layers on autograd.AttnFn.

The float64 reference is the six formulas of include/btx_attn_train.h on the GPU's own q, k, v and d_out, without autograd (O is the
reference's own P V, so that dP - delta cancels in it as it does in the kernel, whose `out` comes from its own P and V).
Metric of one gradient tensor [rows, T, E]: err_t = ||got_t - ref_t|| per (row, token) vector over all heads and channels,
scale_t = max(||ref_t||, rms_t ||ref_t||), metric = max_t err_t / scale_t.  The tolerance comes from the reference alone:

    tol = 4 * metric(ref_prec, ref64) + 4 * (C_EXP + Tk + 2 * key_tiles + 8) * 2^-23

ref_prec: the same formulas at the kernel's precision — in float32 for prec f32; in float64 with q, k, v, dO, P and dS rounded to bf16
by value for prec bf16; in both O and the result rounded to the activation dtype the kernels store (bf16 activations: a bf16 gradient cannot
be nearer to float64 than that).  The second term is the forward's exponential chain (C_EXP of tests/test_gpu_attn.py).  Factor 4:
the kernel rounds where ref_prec rounds, but on sums taken in another order and tiling — an independent draw of the same size.
So that the tolerance cannot hide a dropped key it is itself bounded: <= 1e-3 for f32 / f32, <= 5e-2 wherever bf16 enters (as MFMA
operand or as stored dtype); masking one extra key moves each of dq, dk, dv by >= 1e-1 in this metric on these inputs."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import envelope as E
import poison as P
from test_gpu_attn import C_EXP, CFGS, DIMS, MASKS, PRIOR, _adt, _case, _dev, _heads64, _ids, _masked

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 7), (3, 2, 65), (2, 2, 130), (2, 3, 197)]   # T = 1 left out: dq = dk = 0 there and the relative metric is 0 / 0
_DO = {}


def _d_out(D, shape, act):
    """the gradient at `out` of one case, [rows, T, E] randn: built once, never changed"""
    key = (D, shape, act)
    if key not in _DO:
        (R, H, T), g = shape, torch.Generator().manual_seed(7000 + 1000 * D + 10 * shape[2] + shape[0])
        _DO[key] = torch.randn(R, T, H * D, generator=g).to(_dev(), _adt(act))
    return _DO[key]


def _split(t, H):
    R, T, E_ = t.shape
    return t.reshape(R, T, H, E_ // H).transpose(1, 2)   # [rows, heads, T, D]


def _formulas(q, k, v, dO, masked, dt=torch.float64, rnd=lambda t: t, act=None):
    """dq, dk, dv [rows, T, E] in float64 from [rows, heads, T, D] inputs; dt: the arithmetic, rnd: the rounding of an MFMA operand,
    act: the dtype the forward stores O in (None: exact)"""
    scale = q.shape[-1] ** -0.5
    qr, kr, vr, dOr = (rnd(t.to(dt)) for t in (q, k, v, dO))
    s = (qr @ kr.transpose(-1, -2) * scale).masked_fill(masked, float("-inf"))
    dead = s.amax(-1, keepdim=True) == float("-inf")
    p = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)   # = exp2(c s - L); masked entries exactly 0
    O = rnd(p) @ vr
    delta = (dOr * (O if act is None else O.to(act).to(dt))).sum(-1, keepdim=True)
    ds = rnd(p * (dOr @ vr.transpose(-1, -2) - delta))
    dv, dq, dk = rnd(p).transpose(-1, -2) @ dOr, scale * (ds @ kr), scale * (ds.transpose(-1, -2) @ qr)
    return [t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1).double() for t in (dq, dk, dv)]


def _metric(got, ref):
    got, ref = (t.double().reshape(1, -1) if t.dim() == 1 else t.double().reshape(-1, t.shape[-1]) for t in (got, ref))
    n = ref.norm(dim=-1)
    return float(((got - ref).norm(dim=-1) / torch.maximum(n, n.square().mean().sqrt())).max())


def _references(cfg, D, shape, mask):
    """(ref64, per-tensor tolerances) of one case"""
    (prec, act), (R, H, T) = cfg, shape
    qkv, pad = _case(D, shape, act)
    q, k, v = _heads64(qkv, H)
    dO, m = _split(_d_out(D, shape, act), H), _masked(mask, R, T, pad, qkv.device)
    ref = _formulas(q, k, v, dO, m)
    if prec == "bf16":
        at = _formulas(q, k, v, dO, m, rnd=lambda t: t.bfloat16().to(t.dtype), act=_adt(act))
    else:
        at = _formulas(q, k, v, dO, m, dt=torch.float32, act=_adt(act))
    chain = 4 * (C_EXP + T + 2 * -(-T // (64 if prec == "bf16" else 32)) + 8) * E.ACC_UNIT
    tols = [4 * _metric(a.to(_adt(act)), r) + chain for a, r in zip(at, ref)]
    return ref, tols


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, **_ids)
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_gradients_against_float64(cfg, D, shape, mask):
    from bayesian_torch_amd import functional as BF
    (prec, act), (R, H, T) = cfg, shape
    qkv, pad = _case(D, shape, act)
    kw = dict(key_padding_mask=pad if mask == "pad" else None, causal=mask == "causal", prec=prec)
    out, lse = BF.attn_train_fwd_hip(qkv, H, **kw)
    got = BF.attn_bwd_hip(qkv, out, _d_out(D, shape, act), lse, H, **kw)
    assert got.shape == qkv.shape and got.dtype == qkv.dtype
    ref, tols = _references(cfg, D, shape, mask)
    for name, g, r, tol in zip(("dq", "dk", "dv"), got.split(H * D, dim=-1), ref, tols):
        err = _metric(g, r)
        print("attn bwd %s/%s D=%d %s %s %s: metric %.3e tol %.3e ratio %.3f" % (prec, act, D, shape, mask, name, err, tol, err / tol))
        assert tol <= (1e-3 if cfg == ("f32", "f32") else 5e-2), "the tolerance itself is too wide to see a dropped key"
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_bits(cfg):
    """out is attn_hip's; lse is log2 sum_j exp2(c s_ij) within the forward's rho; two backward calls agree; the packed in-place write
    equals three separate outputs; rows beyond the mask's rows reuse it (MC lanes: rows = lanes * pad_rows)"""
    from bayesian_torch_amd import functional as BF
    (prec, act), D, (R, H, T) = cfg, 64, SHAPES[1]
    qkv, pad = _case(D, SHAPES[1], act)
    dO = _d_out(D, SHAPES[1], act)
    out, lse = BF.attn_train_fwd_hip(qkv, H, pad, prec=prec)
    assert P.bits_equal(out, BF.attn_hip(qkv, H, pad, prec=prec))
    q, k, _ = _heads64(qkv, H)
    scale, u, S = D ** -0.5, E.U_BF16, E.ACC_UNIT
    m = _masked("pad", R, T, pad, qkv.device)
    want = torch.logsumexp((q @ k.transpose(-1, -2) * scale).masked_fill(m, float("-inf")), -1) / 0.6931471805599453
    c_op = 2 * u + u * u if (prec == "bf16" and act == "f32") else 0.0
    d = ((c_op + (D + 8) * S) * scale * (q.abs() @ k.abs().transpose(-1, -2))).masked_fill(m, 0.0).amax(-1)
    rho = torch.expm1(2 * d) + (C_EXP + T + 2 * -(-T // (64 if prec == "bf16" else 32)) + 8) * S
    bound = rho * 1.4426950408889634 + 4 * S * want.abs().clamp_min(1.0)   # d log2(l) = dl / (l ln 2); log2f and the sum m + log2 l
    assert lse.shape == (R, H, T) and bool(((lse.double() - want).abs() <= bound).all())
    got = BF.attn_bwd_hip(qkv, out, dO, lse, H, pad, prec=prec)
    assert P.bits_equal(got, BF.attn_bwd_hip(qkv, out, dO, lse, H, pad, prec=prec))
    three = BF.attn_bwd_hip(tuple(qkv.split(H * D, dim=-1)), out, dO, lse, H, pad, prec=prec)
    assert all(t.is_contiguous() for t in three) and P.bits_equal(torch.cat(three, -1), got)
    two = lambda t: torch.cat([t, t])  # noqa: E731
    out2, lse2 = BF.attn_train_fwd_hip(two(qkv), H, pad, prec=prec)
    assert P.bits_equal(out2, two(out)) and P.bits_equal(lse2, two(lse))
    assert P.bits_equal(BF.attn_bwd_hip(two(qkv), out2, two(dO), lse2, H, pad, prec=prec), two(got))


@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_masked_memory(cfg):
    """k / v rows of padded keys hold NaN and every fresh buffer is poisoned: no NaN comes out, dk and dv of padded keys and dq of a row
    whose keys are all masked are exactly zero"""
    from bayesian_torch_amd import functional as BF
    (prec, act), D, (R, H, T) = cfg, 32, SHAPES[2]
    qkv, pad = _case(D, SHAPES[2], act)
    qkv, pad, E_ = qkv.clone(), pad.clone(), H * D
    pad[0] = True
    qkv[..., E_:][pad] = float("nan")
    for byte in P.PATTERNS:
        with P.poisoned(byte) as rec:
            out, lse = BF.attn_train_fwd_hip(qkv, H, pad, prec=prec)
            got = BF.attn_bwd_hip(qkv, out, _d_out(D, SHAPES[2], act), lse, H, pad, prec=prec)
        assert rec.bytes > 0 and not P.any_nan((out, got))
        assert not bool(got[..., E_:][pad].any()) and not bool(got[0, :, :E_].any()) and bool(got[1, :, :E_].any())


# ---- layer level: the _Net of tests/test_gpu_attn.py ------------------------------------------------------------------------------
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = nn.Linear(16, 64)
        self.enc = nn.TransformerEncoder(nn.TransformerEncoderLayer(64, 2, 128, dropout=0.0, batch_first=True), 1)
        self.head = nn.Linear(64, 8)

    def forward(self, x):
        return self.head(self.enc(self.embed(x)))[:, 0]


def _net(kind, **kw):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    bt.set_precision("f32")
    bt.manual_seed(77)
    torch.manual_seed(0)
    m = _Net()
    bt.dnn_to_bnn(m, dict(PRIOR, type=kind))
    bt.assign_layer_ids(m, start=400)   # the noise is keyed per layer id: both models draw the same
    m = m.to(_dev()).train()
    fuse_model(m, **kw)
    g = torch.Generator().manual_seed(3)
    return m, torch.randn(5, 70, 16, generator=g).to(_dev()), torch.randint(0, 8, (5,), generator=g).to(_dev())


def _step(m, x, y, s):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    for p in m.parameters():
        p.grad = None
    bt.set_sample_index(m, s)
    (F.cross_entropy(m(x).float(), y) + get_kl_loss(m) / x.shape[0]).backward()
    return {n: p.grad.clone() for n, p in m.named_parameters()}


def _layer_tol():
    """check 1's tolerance for f32 / f32 at the layer's attention shape (5 rows, 2 heads, T = 70, D = 32), the widest of dq, dk, dv"""
    return max(_references(("f32", "f32"), 32, (5, 2, 70), "none")[1])


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_layer_gradients_and_graphed_step(kind, monkeypatch):
    from bayesian_torch_amd import autograd as ag
    plain, x, y = _net(kind)
    assert not plain.enc.layers[0].self_attn.fused_training   # fuse_model(m) alone leaves the switch off
    want = _step(plain, x, y, 5)
    m, _, _ = _net(kind, attn_training=True)
    assert m.enc.layers[0].self_attn.fused_training and m.enc.layers[0].self_attn.fused_attention
    calls, real = [], ag.AttnFn.apply
    monkeypatch.setattr(ag.AttnFn, "apply", lambda *a: calls.append(1) or real(*a))
    eager = {s: _step(m, x, y, s) for s in (5, 17)}
    assert len(calls) == 2
    tol = _layer_tol()
    for n, g in eager[5].items():
        if n.rsplit(".", 1)[-1].startswith(("mu_", "rho_")):
            err = _metric(g, want[n])
            print("attn layer %s %s: metric %.3e tol %.3e" % (kind, n, err, tol))
            assert err <= tol, (n, err, tol)
    step = ag.GraphedTrainStep(m, x, y)
    try:
        for s in (5, 17, 5):
            step.run(s)
            torch.cuda.synchronize()
            assert all(torch.equal(p.grad, eager[s][n]) for n, p in m.named_parameters()), s
    finally:
        step.close()


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_time_major_layer(kind):
    """batch_first=False (transposed views, no copies) under a key-padding mask: output and every gradient of the fused training path
    against the composite at the same sample index"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.set_precision("f32")
    tol, dev, res = _layer_tol(), _dev(), []
    pad = (torch.arange(70)[None, :] >= torch.tensor([70, 33, 9])[:, None]).to(dev)
    for fused in (False, True):
        bt.manual_seed(5)
        torch.manual_seed(1)
        a = getattr(L, "MultiheadAttention" + kind)(64, 2, batch_first=False).to(dev)
        bt.assign_layer_ids(a, start=700)
        a.fused_training = fused
        bt.set_sample_index(a, 4)
        x = torch.randn(70, 3, 64, generator=torch.Generator().manual_seed(2)).to(dev).requires_grad_()
        assert a._fused_train_ok(x, pad, False, None, False) == fused
        out = a(x, x, x, key_padding_mask=pad, return_kl=False)[0]
        out.square().sum().backward()
        res.append([out.detach(), x.grad] + [p.grad for p in a.parameters()])
    for k, (got, ref) in enumerate(zip(res[1], res[0])):
        got, ref = (got, ref) if got.dim() < 3 else (got.transpose(0, 1), ref.transpose(0, 1))
        err = _metric(got, ref)
        print("attn %s time-major tensor %d: metric %.3e tol %.3e" % (kind, k, err, tol))
        assert err <= tol, (k, err, tol)
