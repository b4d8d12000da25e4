"""GPU: the fused attention core with an additive score bias / general mask (btx_attn_bias_*) — forward and gradients
against float64, bit contracts, masked memory, and the attention layers under the masks nn.TransformerEncoder passes down.

References and bounds are those of tests/test_gpu_attn.py and tests/test_gpu_attn_train.py with the bias in the scores and one more
term in the exponent's error, D_j += 1.25 S |b_j|.  Finite forward bias values are drawn from [-8, 8]."""
import pytest
import torch
import torch.nn as nn

import envelope as E
import poison as P
from test_gpu_attn import C_EXP, F32_CAP, PRIOR, _adt, _dev, _ids
from test_gpu_attn_train import _metric, _split

pytestmark = pytest.mark.gpu

CFGS = [("f32", "f32"), ("bf16", "bf16")]   # (precision, activation dtype)
R, H = 2, 2
DIMS = [32, 128]
SHAPES = [(1, 1), (33, 65), (130, 97), (64, 128)]   # (Tq, Tk): see DESIGN.md §32.5
FORMS = ["tt", "htt", "rhtt", "key"]
BDT = {"bool": torch.bool, "f32": torch.float32, "bf16": torch.bfloat16}
INF = float("inf")
_CASES = {}


def _case(D, shape, act):
    """(q [R, Tq, E], k, v [R, Tk, E], d_out, ragged key-padding mask [R, Tk]) of one case: built once, never changed"""
    key = (D, shape, act)
    if key not in _CASES:
        (Tq, Tk), dev = shape, _dev()
        g = torch.Generator().manual_seed(100 * D + 10 * Tq + Tk)
        rn = lambda T, s: (s * torch.randn(R, T, H * D, generator=g)).to(dev, _adt(act))  # noqa: E731
        lens = [max(1, Tk - (2 * r + 1) * Tk // 5) for r in range(R)]
        pad = torch.arange(Tk)[None, :] >= torch.tensor(lens)[:, None]
        _CASES[key] = (rn(Tq, 0.3), rn(Tk, 0.3), rn(Tk, 1.0), rn(Tq, 1.0), pad.to(dev))
    return _CASES[key]


def _bias(form, bdt, shape, amp=8.0):
    """a bias of one form and dtype: finite values uniform in [-amp, amp] with one pair in eight masked (-inf); bool: one in three masked"""
    (Tq, Tk), dev = shape, _dev()
    g = torch.Generator().manual_seed(7 + 13 * Tq + Tk)
    full = {"tt": (Tq, Tk), "htt": (H, Tq, Tk), "rhtt": (R, H, Tq, Tk), "key": (R, 1, 1, Tk)}[form]
    if bdt == "bool":
        return (torch.rand(full, generator=g) < 1 / 3).to(dev)
    b = (torch.rand(full, generator=g) * 2 - 1) * amp
    return b.masked_fill(torch.rand(full, generator=g) < 1 / 8, -INF).to(dev, BDT[bdt])


def _b64(bias, shape):
    """the bias as float64 [R, H, Tq, Tk]"""
    b = torch.zeros(bias.shape, dtype=torch.float64, device=bias.device).masked_fill(bias, -INF) if bias.dtype == torch.bool else bias.double()
    return b.expand(R, H, *shape) if b.dim() == 4 else b.expand(R, *((H,) + shape))


def _masked(mask, shape, pad):
    Tq, Tk = shape
    m = torch.zeros(R, 1, Tq, Tk, dtype=torch.bool, device=pad.device)
    if mask == "causal":
        m = m | torch.ones(Tq, Tk, dtype=torch.bool, device=pad.device).triu(1)
    if mask == "pad":
        m = m | pad[:, None, None, :]
    return m


def _probs(q, k, b, masked):
    s = (q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5 + b).masked_fill(masked, -INF)
    dead = s.amax(-1, keepdim=True) == -INF
    return torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)


def _ref_bound(q, k, v, b, masked, prec, act):
    """test_gpu_attn._ref_bound with the bias in the scores and 1.25 S |b| in the exponent's error"""
    D, Tk = q.shape[-1], k.shape[-2]
    scale, u, S = D ** -0.5, E.U_BF16, E.ACC_UNIT
    p = _probs(q, k, b, masked)
    ref, A = p @ v, p @ v.abs()
    c_op = 2 * u + u * u if (prec == "bf16" and act == "f32") else 0.0
    delta = (c_op + (D + 8) * S) * scale * (q.abs() @ k.abs().transpose(-1, -2)) + 1.25 * S * b.abs()
    delta = delta.masked_fill(masked | torch.isinf(b) | torch.isnan(b), 0.0)
    rho = torch.expm1(2 * delta.amax(-1, keepdim=True)) + (C_EXP + Tk + 2 * -(-Tk // (64 if prec == "bf16" else 32)) + 8) * S
    c_pv = (2 * u + u * u if prec == "bf16" else 0.0) + (Tk + 8) * S
    merge = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)  # noqa: E731
    ref, bound, A = merge(ref), merge((rho + c_pv) * A), merge(A)
    if act == "bf16":
        bound = torch.as_tensor(E.store_rounding(bound, ref), device=ref.device)
    return ref, bound, A


@pytest.mark.parametrize("mask", ["none", "pad", "causal"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bdt", list(BDT))
@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_forward_inside_the_envelope(cfg, bdt, form, mask):
    from bayesian_torch_amd import functional as BF
    prec, act = cfg
    for D in DIMS:
        for shape in SHAPES:
            q, k, v, _, pad = _case(D, shape, act)
            bias = _bias(form, bdt, shape)
            got = BF.attn_hip((q, k, v), H, pad if mask == "pad" else None, causal=mask == "causal", prec=prec, bias=bias)
            q64, k64, v64 = (_split(t.double(), H) for t in (q, k, v))
            ref, bound, A = _ref_bound(q64, k64, v64, _b64(bias, shape), _masked(mask, shape, pad), prec, act)
            rep = E.check(got, ref, bound)
            print("attn bias %s/%s %s %s %s D=%d %s: %s" % (prec, act, bdt, form, mask, D, shape, rep))
            if cfg == ("f32", "f32"):
                assert bool((bound <= F32_CAP * A).all()), "the f32 bound itself is too wide to see a dropped key"
            assert got.shape == q.shape and got.dtype == q.dtype and rep.ok, (D, shape, str(rep))


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_exact_probes(cfg, D):
    """a zero bias = no bias; bool = the 0 / -inf f32 bias; a key-only -inf bias = key_pad; a lower-triangular bool bias = causal; the
    training forward = the inference forward; a query whose every key has bias -inf: zeros and lse = +inf — all bit for bit"""
    from bayesian_torch_amd import functional as BF
    prec, act = cfg
    for shape in SHAPES:
        (Tq, Tk), dev = shape, _dev()
        q, k, v, _, pad = _case(D, shape, act)
        run = lambda **kw: BF.attn_hip((q, k, v), H, prec=prec, **kw)  # noqa: E731
        assert P.bits_equal(run(bias=torch.zeros(Tq, Tk, device=dev)), run()), shape
        bb = _bias("rhtt", "bool", shape)
        bf = torch.zeros(bb.shape, device=dev).masked_fill(bb, -INF)
        assert P.bits_equal(run(bias=bb), run(bias=bf)), shape
        assert P.bits_equal(run(bias=torch.zeros(R, 1, 1, Tk, device=dev).masked_fill(pad[:, None, None, :], -INF)), run(key_padding_mask=pad)), shape
        assert P.bits_equal(run(bias=torch.ones(Tq, Tk, dtype=torch.bool, device=dev).triu(1)), run(causal=True)), shape
        dead = bf.clone()
        dead[0, :, 0] = -INF
        out, lse = BF.attn_train_fwd_hip((q, k, v), H, prec=prec, bias=dead)
        assert P.bits_equal(out, run(bias=dead)) and not bool(out[0, 0].any()) and bool((lse[0, :, 0] == INF).all()), shape
        assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("bdt", ["f32", "bf16"])
@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_masked_memory(cfg, bdt):
    """NaN in the bias at padded keys, above the causal diagonal and, with a padded allocation, past Tq and Tk: the same bits"""
    from bayesian_torch_amd import functional as BF
    prec, act = cfg
    for D, shape in [(D, shape) for D in DIMS for shape in SHAPES[1:]]:
        (Tq, Tk), dev = shape, _dev()
        q, k, v, _, pad = _case(D, shape, act)
        clean = _bias("rhtt", bdt, shape)
        want = BF.attn_hip((q, k, v), H, pad, causal=True, prec=prec, bias=clean)
        big = torch.full((R, H, Tq + 4, Tk + 8), float("nan"), dtype=clean.dtype, device=dev)
        dirty = big[:, :, :Tq, :Tk]
        dirty.copy_(clean)
        dirty.masked_fill_(pad[:, None, None, :] | torch.ones(Tq, Tk, dtype=torch.bool, device=dev).triu(1), float("nan"))
        assert not dirty.is_contiguous() and bool(torch.isfinite(want).all())
        assert P.bits_equal(BF.attn_hip((q, k, v), H, pad, causal=True, prec=prec, bias=dirty), want), shape


def _formulas(q, k, v, dO, b, masked, dt=torch.float64, rnd=lambda t: t, act=None):
    """test_gpu_attn_train._formulas with the bias in the scores"""
    scale = q.shape[-1] ** -0.5
    qr, kr, vr, dOr = (rnd(t.to(dt)) for t in (q, k, v, dO))
    p = _probs(qr, kr, b.to(dt), masked)
    O = rnd(p) @ vr
    delta = (dOr * (O if act is None else O.to(act).to(dt))).sum(-1, keepdim=True)
    ds = rnd(p * (dOr @ vr.transpose(-1, -2) - delta))
    dv, dq, dk = rnd(p).transpose(-1, -2) @ dOr, scale * (ds @ kr), scale * (ds.transpose(-1, -2) @ qr)
    return [t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1).double() for t in (dq, dk, dv)]


@pytest.mark.parametrize("form", ["htt", "key"])
@pytest.mark.parametrize("bdt", ["bool", "f32"])
@pytest.mark.parametrize("cfg", CFGS, **_ids)
def test_gradients_against_float64(cfg, bdt, form):
    """dq, dk, dv under a key-padding mask and the bias, with test_gpu_attn_train's metric and tolerance; two calls give the same bits;
    padded keys and dead queries (query 0 of the per-head form is one by construction) get zero gradients.  Finite bias values come
    from [-2, 2] here"""
    from bayesian_torch_amd import functional as BF
    prec, act = cfg
    for D in DIMS:
        for shape in SHAPES:
            (Tq, Tk), (q, k, v, dO, pad) = shape, _case(D, shape, act)
            bias = _bias(form, bdt, shape, amp=2.0).clone()
            if form == "htt":
                bias[:, 0] = True if bdt == "bool" else -INF
            out, lse = BF.attn_train_fwd_hip((q, k, v), H, pad, prec=prec, bias=bias)
            got = BF.attn_bwd_hip((q, k, v), out, dO, lse, H, pad, prec=prec, bias=bias)
            again = BF.attn_bwd_hip((q, k, v), out, dO, lse, H, pad, prec=prec, bias=bias)
            assert all(P.bits_equal(a, b) for a, b in zip(got, again)) and not P.any_nan(got)
            b64, m = _b64(bias, shape), _masked("pad", shape, pad)
            args = [_split(t.double(), H) for t in (q, k, v, dO)]
            ref = _formulas(*args, b64, m)
            dead = (lse == INF).transpose(1, 2)   # [R, Tq, H]
            assert form != "htt" or bool(dead[:, 0].all())
            assert not bool(got[1][pad].any()) and not bool(got[2][pad].any())
            assert not bool(got[0].reshape(R, Tq, H, D)[dead].any())
            if shape == (1, 1):
                # one key: dS = P (dP - delta) = 0 in exact arithmetic (the metric would be 0 / 0); dP and delta are two f32 sums of the
                # same D products in another order, so |dS| <= 2 (D + 8) S sum_d |dO_d v_d|, and dq = scale dS k, dk = scale dS q
                lim = 2 * (D + 8) * E.ACC_UNIT * D ** -0.5 * (args[3].abs() * args[2].abs()).sum(-1, keepdim=True) * (1 + 2 * E.U_BF16)
                assert bool((_split(got[0].double(), H).abs() <= lim * args[1].abs()).all())
                assert bool((_split(got[1].double(), H).abs() <= lim * args[0].abs()).all())
                continue
            if prec == "bf16":
                at = _formulas(*args, b64, m, rnd=lambda t: t.bfloat16().to(t.dtype), act=_adt(act))
            else:
                at = _formulas(*args, b64, m, dt=torch.float32, act=_adt(act))
            chain = 4 * (C_EXP + Tk + 2 * -(-Tk // (64 if prec == "bf16" else 32)) + 8) * E.ACC_UNIT
            for name, g, r, a in zip(("dq", "dk", "dv"), got, ref, at):
                tol, err = 4 * _metric(a.to(_adt(act)), r) + chain, _metric(g, r)
                print("attn bias bwd %s/%s %s %s D=%d %s %s: metric %.3e tol %.3e ratio %.3f" % (prec, act, bdt, form, D, shape, name, err, tol, err / tol))
                assert tol <= (1e-3 if cfg == ("f32", "f32") else 5e-2), "the tolerance itself is too wide to see a dropped key"
                assert err <= tol, (D, shape, name, err, tol)


# ---- layer level: a converted two-layer nn.TransformerEncoder under the masks it passes down ---------------------------------------
def _encoder(kind, train=False):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    bt.set_precision("f32")
    bt.manual_seed(77)
    torch.manual_seed(0)
    m = nn.TransformerEncoder(nn.TransformerEncoderLayer(64, 2, 128, dropout=0.0, batch_first=True), 2, enable_nested_tensor=False)
    bt.dnn_to_bnn(m, dict(PRIOR, type=kind))
    bt.assign_layer_ids(m, start=500)
    m = m.to(_dev()).train(train)
    fuse_model(m, attn_training=train)
    # 5 x 70 > 256 rows: single-sample and lane launches of every Linear share one kernel family (see test_gpu_attn._Net)
    x = torch.randn(5, 70, 64, generator=torch.Generator().manual_seed(3)).to(_dev())
    pad = (torch.arange(70)[None, :] >= torch.tensor([70, 33, 9, 70, 50])[:, None]).to(_dev())
    return m, x, pad


def _no_core(*a, **k):
    raise AssertionError("the composite was taken")


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_encoder_with_padding_stays_on_the_fused_core(kind, monkeypatch):
    """eval and training forwards of the converted encoder under src_key_padding_mask (a float mask by the time the layer sees it)
    and under a float [T, T] window mask never reach the composite; one torch.cuda.graph replay equals the eager bits; MC lanes equal
    single forwards; every parameter gets a finite gradient"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    m, x, pad = _encoder(kind)
    monkeypatch.setattr(L.base_variational_layer._VariationalMHA, "_core", _no_core)
    win = torch.zeros(70, 70, device=x.device).masked_fill((torch.arange(70)[:, None] - torch.arange(70)[None, :]).abs().to(x.device) > 8, -INF)
    with torch.no_grad():
        bt.set_sample_index(m, 5)
        eager = m(x, src_key_padding_mask=pad)
        bt.set_sample_index(m, 5)
        both = m(x, mask=win, src_key_padding_mask=pad)
        assert bool(torch.isfinite(eager).all()) and bool(torch.isfinite(both).all()) and not P.bits_equal(both, eager)
        single = []
        for s in (5, 11):
            bt.set_sample_index(m, s)
            single.append(m(x, src_key_padding_mask=pad))
        assert P.bits_equal(single[0], eager)
        try:
            bt.set_sample_lanes(m, [5, 11], batch=x.shape[0])
            lanes = m(torch.cat([x, x]), src_key_padding_mask=pad)
        finally:
            bt.set_sample_lanes(m, None)
        assert P.bits_equal(lanes, torch.cat(single))
        bt.set_sample_index(m, 5)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x, src_key_padding_mask=pad)   # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        bt.set_sample_index(m, 5)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            captured = m(x, src_key_padding_mask=pad)
        captured.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert P.bits_equal(captured, eager)
    m, x, pad = _encoder(kind, train=True)
    m(x, src_key_padding_mask=pad)[~pad].square().mean().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


@pytest.mark.parametrize("kind", ["Reparameterization", "Flipout"])
def test_layer_against_the_composite(kind):
    """the attention module alone at sigma = 0: both paths see the same qkv, so their outputs differ by the two core errors pushed
    through out_proj (as in test_gpu_attn.test_lanes_graphs_and_the_composite) — under a float key-padding mask alone, with a bool and
    with a float [T, T] mask (_fused_masks' where / add), and under a [B * heads, T, T] mask; training: the fused gradients against
    the composite's in test_gpu_attn_train's metric at its layer tolerance"""
    from test_gpu_attn_train import _layer_tol
    m, x, pad = _encoder(kind)
    attn, dev = m.layers[0].self_attn, x.device
    fpad = torch.zeros(pad.shape, device=dev).masked_fill(pad, -INF)
    far = (torch.arange(70)[:, None] - torch.arange(70)[None, :]).abs().to(dev) > 8
    g = torch.Generator().manual_seed(9)
    rel, full = torch.randn(70, 70, generator=g).to(dev), torch.randn(10, 70, 70, generator=g).to(dev)
    none = torch.zeros(5, 1, 70, 70, dtype=torch.bool, device=dev)
    with torch.no_grad():
        for lin in (attn.in_proj, attn.out_proj):
            lin.rho_weight.fill_(-200.0)
            lin.rho_bias.fill_(-200.0)
        q, k, v = (_split(t.double(), 2) for t in attn.in_proj(x, return_kl=False).split(64, dim=-1))
        W = attn.out_proj.mu_weight.double().abs()
        kp64 = fpad.double()[:, None, None, :]
        for name, kw, b64 in (("kp", dict(key_padding_mask=fpad), kp64),
                              ("kp+bool", dict(key_padding_mask=fpad, attn_mask=far), kp64.masked_fill(far, -INF)),
                              ("kp+float", dict(key_padding_mask=fpad, attn_mask=rel), kp64 + rel.double()),
                              ("3-D", dict(attn_mask=full), full.double().unflatten(0, (5, 2)))):
            res = []
            for on in (True, False):
                attn.fused_attention = on
                assert attn._fused_ok(x, kw.get("key_padding_mask"), False, kw.get("attn_mask"), False) == on
                res.append(attn(x, x, x, **kw)[0])
            fused, comp = res
            _, b, A = _ref_bound(q, k, v, b64.expand(5, 2, 70, 70), none, "f32", "f32")
            bound = 2 * b @ W.t() + 2 * E.rel_constant("f32", 64) * (A @ W.t()) + 4 * E.REF32_UNIT * comp.double().abs()
            rep = E.check(fused, comp.double(), bound)
            print("attn bias %s %s fused vs composite: %s" % (kind, name, rep))
            assert rep.ok, (name, str(rep))
    grads = []
    for on in (False, True):
        attn.fused_training = on
        attn.fused_attention = on
        xg = x.clone().requires_grad_()
        assert attn._fused_train_ok(xg, fpad, False, None, False) == on
        attn(xg, xg, xg, key_padding_mask=fpad)[0][~pad].square().sum().backward()
        grads.append([xg.grad] + [p.grad.clone() for p in (attn.in_proj.mu_weight, attn.out_proj.mu_weight)])
        attn.zero_grad()
    tol = _layer_tol()
    for got, ref in zip(grads[1], grads[0]):
        assert _metric(got, ref) <= tol, (_metric(got, ref), tol)
