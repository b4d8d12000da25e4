"""GPU: every kernel entry on tensors OFF the 16-byte grid (DESIGN.md "Alignment contract").

The other files hand the kernels tensors that come straight from torch's allocator: 512-byte aligned, so of every
`(uintptr_t)ptr & 15` branch in csrc/ only one side ever ran.  Here the same calls are made on dense views carved out of a larger
buffer at 2 / 4 / 8 bytes (bf16), 4 / 8 bytes (f32) or 1 / 4 bytes (uint8) past a 16-byte boundary — what `as_strided`, a dlpack /
frombuffer import or parameters kept in ONE flat storage produce — and on models whose parameters are views of one flat buffer at
+4 bytes.  What must hold is the documented behaviour, nothing else:

  same kernel after one aligned copy (functional.on_grid: BatchNorm, the pools, the epilogue residual, every parameter that goes
  through gemm_major_view), element-wise kernels, integer arithmetic          -> torch.equal with the aligned call
  another kernel on random data (the gather kernel behind `unaligned`, the generic weight-gradient kernels, the scalar KL
  path)                                                                      -> every element inside the bound tests/envelope.py
                                                                                already defines, against float64
  small-integer inputs with dyadic mu and rho = -200                         -> the float64 result bit for bit

No new tolerance.  Every case first asserts that the ALIGNED call is on a fast path (btx_contract_plan_info, or the shape conditions
of the source spelled out), so the off-grid call really goes elsewhere.  `off_grid` fills the slack around the view with NaN (0xAB
bytes for uint8): a read past either end of the tensor that reached a result would show.

Each envelope check prints `name prec: worst err/bound R at index`; profiles/alignment_envelope.txt holds the lines of the first
full run.
"""
import warnings

import numpy as np
import pytest
import torch

import envelope as E
from test_gpu_backward import _op_of
from test_gpu_elementwise import _Log, _dev, _grads64, _make, _refs, _scaled, _sigma_zero_dyadic, _tag
from test_gpu_fuse_model import CASES as EPI_CASES, _plan

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
OFFSETS = {F32: (4, 8), BF16: (2, 8), U8: (1, 4)}   # bytes past a 16-byte boundary, per element type
_N = {F32: "f32", BF16: "bf16"}


# =============================================================================================================================
# helpers
# =============================================================================================================================
def _span(t):
    """elements between the first and one past the last element the view addresses"""
    return 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride())) if t.numel() else 1


def off_grid(t, nbytes):
    """a tensor with t's values, shape and strides whose data_ptr() is `nbytes` past a 16-byte boundary: a view (as_strided) into a
    fresh buffer with at least 64 bytes of slack on either side, so every access of whatever width stays inside a live allocation.
    The slack holds NaN (0xAB for integer types)."""
    esz = t.element_size()
    assert 0 < nbytes < 16 and nbytes % esz == 0, (nbytes, esz)
    slack = 64 // esz
    buf = torch.empty(_span(t) + 2 * slack + 16 // esz, dtype=t.dtype, device=t.device)
    if t.dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.fill_(0xAB)
    first = buf.data_ptr() + slack * esz
    off = slack + ((nbytes - first) % 16) // esz
    v = buf.as_strided(tuple(t.shape), tuple(t.stride()), off)
    v.copy_(t.detach())
    assert v.data_ptr() % 16 == nbytes and v.stride() == t.stride() and v.shape == t.shape
    assert v.data_ptr() - buf.data_ptr() >= 64 and (buf.data_ptr() + buf.numel() * esz) - (v.data_ptr() + _span(t) * esz) >= 64
    return v


def flat_params(module, nbytes=4):
    """move every f32 parameter of `module` into ONE flat buffer, each a view with its own strides `nbytes` past a 16-byte
    boundary (the storage a flat-buffer optimizer keeps) -> the buffer"""
    ps = [p for p in module.parameters() if p.dtype == F32]
    step = lambda p: (_span(p) + 3) // 4 * 4 + 4  # noqa: E731  (keeps the residue, leaves a gap between neighbours)
    flat = torch.full((32 + sum(step(p) for p in ps),), float("nan"), device=ps[0].device)
    at = 16 + ((nbytes - flat.data_ptr()) % 16) // 4
    for p in ps:
        v = flat.as_strided(tuple(p.shape), tuple(p.stride()), at)
        v.copy_(p.detach())
        p.data = v
        assert p.data_ptr() % 16 == nbytes and torch.equal(p.detach(), v)
        at += step(p)
    return flat


def _on_grid(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def _x_of(xs, act, seed=17, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*xs, generator=g) * scale).to(_dev()).to(act)
    return x.contiguous(memory_format=torch.channels_last) if len(xs) == 4 else x


# =============================================================================================================================
# 1. contraction forward: one layer per fast family
# =============================================================================================================================
# EPI_CASES without the two that are on the gather kernel already (the explicit gather case and the depthwise one)
FWD_CASES = [c for c in EPI_CASES if not c[3] and c[1].get("groups", 1) == 1]
PRECS = [("f32", F32), ("bf16x3", F32), ("bf16", BF16)]


def test_forward_cases_cover_every_fast_family():
    families = set()
    for cls, kw, xs, _ in FWD_CASES:
        for prec, _ in PRECS:
            rc, fam, _ = _plan(_make(cls, kw, prec), xs, prec)
            assert rc == 0 and fam != "gather", (cls, kw, prec, fam)
            families.add(fam)
    assert {"regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem"} <= families, families


def _direct(layer, x, prec, sample, mu_p, rho_p, mb, rb):
    """btx_contract_fwd on the layer's geometry with the parameter tensors given (no wrapper in between)"""
    from bayesian_torch_amd import _lib, functional as BF, rng
    kind = _lib.KIND_FLIPOUT if layer._family == "flipout" else _lib.KIND_REPARAM
    return BF.contract_hip(kind, x, mu_p, rho_p, mb, rb, layer._op, rng.seed(), sample, layer._btx_layer_id, prec=prec)


@pytest.mark.parametrize("case", FWD_CASES, ids=[_tag(*c[:3]) for c in FWD_CASES])
def test_forward_off_grid_envelope(case):
    """random data.  x alone off the grid: the gather kernel (select_fwd: `unaligned`), inside the envelope — except the row-fused
    stem, whose input is packed element by element into a fresh buffer first: the same launch, equal bits.  Parameters in a flat
    buffer at +4 bytes: gemm_major_view hands the launch aligned copies, equal bits; the same parameters handed to btx_contract_fwd
    directly: the gather kernel, inside the envelope.  Residual / scale / shift off the grid: the residual enters as an aligned
    copy, scale and shift are read element by element: equal bits.  Everything at once: inside the envelope carried through the
    affine, the residual add and the ReLU."""
    from bayesian_torch_amd import functional as BF
    cls, kw, xs, _ = case
    log = _Log()
    refs = {}
    tag = _tag(cls, kw, xs)
    nout = kw.get("out_channels", kw.get("out_features"))
    stem = kw.get("in_channels", 99) <= 4
    for prec, act in PRECS:
        o1, o2 = OFFSETS[act]
        layer = _make(cls, kw, prec, seed=7, bt_seed=1234)
        rc, fam, _ = _plan(layer, xs, prec)
        assert rc == 0 and fam != "gather"
        name = "%s [%s]" % (tag, fam)
        x = _x_of(xs, act)
        g = torch.Generator().manual_seed(18)
        scale = (torch.rand(nout, generator=g) * 4 + 2).to(_dev())
        shift = torch.randn(nout, generator=g).to(_dev())
        with torch.no_grad():
            base = layer._forward_hip(x, sample_idx=5)
        res = None if stem else (torch.randn(base.shape, generator=g) * 4).to(_dev()).to(act).contiguous(
            memory_format=torch.channels_last if base.dim() == 4 else torch.contiguous_format)
        assert _on_grid(x, scale, shift, res, *[p for p in layer.parameters()])
        if act not in refs:
            refs[act] = _refs(layer, x, base.shape, 5)
        pre, A, Ab, K = refs[act]
        bnd = E.bound(A, prec, K, ref=pre, A_bias=Ab, store_bf16=(act == BF16))
        log.check("aligned " + name, prec, base, pre, bnd)

        # ---- x alone
        with torch.no_grad():
            got = layer._forward_hip(off_grid(x, o1), sample_idx=5)
        if stem:
            assert torch.equal(got, base), "row-fused stem: the packed input does not depend on where x lies"
        else:
            log.check("x+%d %s" % (o1, name), prec, got, pre, bnd)

        # ---- all parameters of the layer in one flat buffer at +4 bytes
        twin = _make(cls, kw, prec, seed=7, bt_seed=1234)
        flat_params(twin)
        assert twin._btx_layer_id == layer._btx_layer_id and all(p.data_ptr() % 16 == 4 for p in twin.parameters())
        with torch.no_grad():
            got = twin._forward_hip(x, sample_idx=5)
        assert torch.equal(got, base), "flat-buffer parameters: %s %s differs from the aligned layer" % (name, prec)
        if not stem and layer._btx_cpad is None:
            mu, rho = twin._w()
            mu_p, rho_p = mu.detach(), rho.detach()
            if layer._op.nd:  # the parameter's own storage order IS GEMM-major: the permuted view is the off-grid buffer itself
                perm = (0,) + tuple(range(2, 2 + layer._op.nd)) + (1,)
                mu_p, rho_p = mu_p.permute(perm), rho_p.permute(perm)
            assert mu_p.is_contiguous() and mu_p.data_ptr() % 16 == 4 and rho_p.data_ptr() % 16 == 4
            mb = twin.mu_bias.detach() if twin.mu_bias is not None else None
            rb = twin.rho_bias.detach() if twin.mu_bias is not None else None
            with torch.no_grad():
                got = _direct(twin, x, prec, 5, mu_p, rho_p, mb, rb)
            log.check("mu,rho,bias+4 through btx_contract_fwd %s" % name, prec, got, pre, bnd)

        # ---- the fused epilogue's residual with scale / shift
        ep = dict(scale=scale, shift=shift, residual=res, relu=1)
        ep_off = dict(scale=off_grid(scale, 4), shift=off_grid(shift, 8), residual=off_grid(res, o2) if res is not None else None,
                      relu=1)
        with torch.no_grad():
            e0 = layer._forward_hip(x, sample_idx=5, epilogue=ep)
            e1 = layer._forward_hip(x, sample_idx=5, epilogue=ep_off)
        assert torch.equal(e1, e0), "epilogue operands off the grid: %s %s differs from the aligned call" % (name, prec)

        # ---- everything
        with torch.no_grad():
            e2 = twin._forward_hip(off_grid(x, o2), sample_idx=5, epilogue=ep_off)
        if stem:
            assert torch.equal(e2, e0)
        else:
            shp = (1, -1) + (1,) * (pre.dim() - 2)
            val = pre * E.d64(scale).view(shp) + E.d64(shift).view(shp)
            b = E.through_affine(E.bound(A, prec, K, A_bias=Ab), pre, scale, shift, channel_axis=1)
            val = val + E.d64(res)
            b = b + E.REF32_UNIT * (val.abs().numpy() + b)  # one f32 add
            if act == BF16:
                b = E.store_rounding(b, val)
            log.check("everything %s" % name, prec, e2, val.clamp_min(0), b)
            log.check("aligned epilogue %s" % name, prec, e0, val.clamp_min(0), b)
    log.done()


@pytest.mark.parametrize("case", FWD_CASES, ids=[_tag(*c[:3]) for c in FWD_CASES])
def test_forward_off_grid_exact_and_lanes(case):
    """sigma = 0 exactly, dyadic mu, small-integer x: every partial sum is an integer multiple of 2^-7 below 2^24, so whichever
    kernel the pointers select returns the float64 convolution bit for bit (bf16 activations: rounded once on store) — the same
    bits as the aligned call.  And a 2-lane launch on off-grid x equals the two single launches on it."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    cls, kw, xs, _ = case
    log = _Log()
    tag = _tag(cls, kw, xs)
    stem = kw.get("in_channels", 99) <= 4
    ref64 = None
    for prec, act in PRECS:
        o1, o2 = OFFSETS[act]
        layer = _make(cls, kw, prec)
        rc, fam, _ = _plan(layer, xs, prec)
        assert rc == 0 and fam != "gather"
        _sigma_zero_dyadic(layer)
        x = E.small_ints(xs, 43).to(_dev()).to(act)
        if len(xs) == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        if ref64 is None:
            with torch.no_grad():
                ref64 = E.contract(E.d64(x), E.d64(layer._w()[0]), E.d64(layer.mu_bias), _op_of(layer))
            assert float(ref64.abs().max()) * 128 < 2 ** 24
        ref = ref64.to(BF16) if act == BF16 else ref64
        twin = _make(cls, kw, prec)
        _sigma_zero_dyadic(twin)
        flat_params(twin)
        xo = off_grid(x, o1)
        with torch.no_grad():
            runs = [("aligned", layer._forward_hip(x, sample_idx=9)), ("x+%d" % o1, layer._forward_hip(xo, sample_idx=9)),
                    ("everything", twin._forward_hip(off_grid(x, o2), sample_idx=9))]
        for form, got in runs:
            rep = E.check_exact(got, ref)
            print(rep.line("exact fwd %s [%s] %s" % (tag, fam, form), prec))
            if not rep.ok:
                log.bad.append("%s %s %s: %s" % (tag, prec, form, rep))
            assert got.stride() == runs[0][1].stride()
        # ---- lanes (random weights again: the samples differ)
        lay = _make(cls, kw, prec, seed=7, bt_seed=1234)
        xr = _x_of(xs, act)
        xro = off_grid(xr, o1)
        idx, bs = [8, 21], xs[0]
        with torch.no_grad():
            with BF.concurrent_plan():
                singles = [lay._forward_hip(xro, sample_idx=s) for s in idx]
            bt.set_sample_lanes(lay, idx, batch=bs)
            xx = torch.cat([xr, xr], 0)
            if xx.dim() == 4:
                xx = xx.contiguous(memory_format=torch.channels_last)
            both = lay._forward_hip(xro if stem else off_grid(xx, o1))
            bt.set_sample_lanes(lay, None)
        assert both.shape[0] == 2 * bs
        for l in range(2):
            assert torch.equal(both[l * bs:(l + 1) * bs], singles[l]), "%s %s: lane %d of a launch on off-grid x" % (tag, prec, l)
        assert not torch.equal(singles[0], singles[1])
    log.done()


def _slack_untouched(t, esz_slack=64):
    """the NaN slack around an off_grid view is still NaN: nothing was stored outside the tensor"""
    base = t._base if t._base is not None else t
    flat = base.reshape(-1)
    n = esz_slack // base.element_size()
    return bool(torch.isnan(flat[:n].float()).all()) and bool(torch.isnan(flat[-n:].float()).all())


@pytest.mark.parametrize("case", [c for c in FWD_CASES if c[1].get("in_features") == 256 or c[1].get("kernel_size") == 5],
                         ids=["split-K", "patch"])
def test_contraction_with_out_and_residual_off_grid(case, monkeypatch):
    """the C ABI alone reaches this (the Python layer allocates `out` itself and realigns the residual; both are switched off
    here): `out` and `ep.residual` off the grid select the gather kernel through `al`, whose 4-channel runs and whose split-K
    reduce then go element by element.  Inside the envelope, exact on integers, and nothing stored outside `out`."""
    from bayesian_torch_amd import functional as BF
    cls, kw, xs, _ = case
    nout = kw.get("out_channels", kw.get("out_features"))
    real_alloc, off = BF._alloc_out, [0]
    monkeypatch.setattr(BF, "_alloc_out", lambda *a: off_grid(real_alloc(*a), off[0]) if off[0] else real_alloc(*a))
    monkeypatch.setattr(BF, "on_grid", lambda t: t)
    log = _Log()
    refs, splits = {}, []
    for prec, act in PRECS:
        layer = _make(cls, kw, prec, seed=7, bt_seed=1234)
        assert _plan(layer, xs, prec)[1] != "gather"
        splits.append(_plan(layer, xs, prec, gather=True)[2])
        x = _x_of(xs, act)
        g = torch.Generator().manual_seed(18)
        scale = (torch.rand(nout, generator=g) * 4 + 2).to(_dev())
        shift = torch.randn(nout, generator=g).to(_dev())
        with torch.no_grad():
            base = layer._forward_hip(x, sample_idx=5)
        res = (torch.randn(base.shape, generator=g) * 4).to(_dev()).to(act)
        if base.dim() == 4:
            res = res.contiguous(memory_format=torch.channels_last)
        if act not in refs:
            refs[act] = _refs(layer, x, base.shape, 5)
        pre, A, Ab, K = refs[act]
        shp = (1, -1) + (1,) * (pre.dim() - 2)
        val = pre * E.d64(scale).view(shp) + E.d64(shift).view(shp) + E.d64(res)
        b = E.through_affine(E.bound(A, prec, K, A_bias=Ab), pre, scale, shift, channel_axis=1)
        b = b + E.REF32_UNIT * (val.abs().numpy() + b)
        if act == BF16:
            b = E.store_rounding(b, val)
        for o_out, o_res in zip(OFFSETS[act], reversed(OFFSETS[act])):
            off[0] = o_out
            with torch.no_grad():
                got = layer._forward_hip(x, sample_idx=5, epilogue=dict(scale=scale, shift=shift, residual=off_grid(res, o_res), relu=1))
                plain = layer._forward_hip(x, sample_idx=5)
            off[0] = 0
            torch.cuda.synchronize()
            assert got.data_ptr() % 16 == o_out and plain.data_ptr() % 16 == o_out
            assert _slack_untouched(got) and _slack_untouched(plain), "a store outside `out`"
            name = "out+%d residual+%d %s" % (o_out, o_res, _tag(cls, kw, xs))
            log.check(name, prec, got, val.clamp_min(0), b)
            log.check(name + " no epilogue", prec, plain, pre, E.bound(A, prec, K, ref=pre, A_bias=Ab, store_bf16=(act == BF16)))
        # ---- exact
        lay = _make(cls, kw, prec)
        _sigma_zero_dyadic(lay)
        xi = E.small_ints(xs, 43).to(_dev()).to(act)
        if len(xs) == 4:
            xi = xi.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ref = E.contract(E.d64(xi), E.d64(lay._w()[0]), E.d64(lay.mu_bias), _op_of(lay))
            off[0] = OFFSETS[act][0]
            got = lay._forward_hip(xi, sample_idx=9)
            off[0] = 0
        rep = E.check_exact(got, ref.to(BF16) if act == BF16 else ref)
        print(rep.line("exact fwd out+%d %s" % (OFFSETS[act][0], _tag(cls, kw, xs)), prec))
        assert rep.ok and _slack_untouched(got), str(rep)
    if kw.get("in_features") == 256:
        assert max(splits) > 1, splits  # the reduce kernel's store ran too
    log.done()


# =============================================================================================================================
# 2. backward through autograd
# =============================================================================================================================
# (class, kwargs, x shape, activation dtype, the weight-gradient kernel the ALIGNED call takes)
BWD = [
    ("Conv2dFlipout", dict(in_channels=32, out_channels=48, kernel_size=3, stride=2, padding=1), (2, 32, 11, 11), BF16, "fast"),
    ("Conv2dReparameterization", dict(in_channels=32, out_channels=64, kernel_size=3, padding=1), (2, 32, 10, 10), BF16, "fast"),
    # the all-taps kernel takes no bias (wgrad_taps3_ok); 2 x 8 x 8 = 128 pixels: two chunks
    ("Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, bias=False), (2, 64, 8, 8), BF16, "taps3"),
    ("Conv2dReparameterization", dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, bias=False), (2, 64, 8, 8), BF16,
     "taps3"),
    ("Conv2dReparameterization", dict(in_channels=32, out_channels=64, kernel_size=3, padding=1), (2, 32, 10, 10), F32, "f32"),
    ("LinearFlipout", dict(in_features=128, out_features=64), (200, 128), F32, "f32"),
]


def _wgrad_route(layer, xshape, oshape, act, bias):
    """the shape conditions of wgrad_impl (csrc/btx_wgrad.hip) for the ALIGNED call, and its chunk count"""
    op = layer._op
    C, N, g = op.in_channels, op.out_channels, op.groups
    M = int(np.prod(oshape)) // N
    T = op.kernel[0] * op.kernel[1] * op.kernel[2]
    ntiles, ctiles = (N // g + 63) // 64, (C // g + 63) // 64
    taps3 = (act == BF16 and not bias and op.nd == 2 and g == 1 and op.kernel == (1, 3, 3) and op.stride == (1, 1, 1) and
             op.padding == (0, 1, 1) and op.dilation == (1, 1, 1) and 2 <= xshape[3] <= 63 and xshape[2] >= 2 and C % 64 == 0 and
             N % 64 == 0)
    fast = act == BF16 and C % 4 == 0 and (C // g) % 16 == 0 and N % 16 == 0 and (N // g) % 16 == 0
    base = ntiles * ctiles if taps3 else g * ntiles * ctiles * T
    chunks = max(1, min((256 if taps3 else 512) // base, (M + 63) // 64))
    cpx = ((M + chunks - 1) // chunks + 63) // 64 * 64
    return ("taps3" if taps3 else "fast" if fast else "f32" if act == F32 else "generic"), (M + cpx - 1) // cpx


def _bwd_run(layer, x, dy, sample):
    import bayesian_torch_amd as bt
    for p in layer.parameters():
        p.grad = None
    x1 = x.detach().requires_grad_(True)
    assert x1.data_ptr() == x.data_ptr()
    bt.set_sample_index(layer, sample)
    out = layer(x1, return_kl=False)
    out.backward(dy)
    torch.cuda.synchronize()
    mu, rho = layer._w()
    r = dict(out=out.detach(), dx=x1.grad, dmu=mu.grad, drho=rho.grad)
    if layer.mu_bias is not None:
        r.update(dmu_b=layer.mu_bias.grad, drho_b=layer.rho_bias.grad)
    return r


@pytest.mark.parametrize("cls,kw,xshape,act,route", BWD, ids=["%s-%s-%s" % (_tag(c[0], c[1], c[2]), _N[c[3]], c[4]) for c in BWD])
def test_backward_off_grid(cls, kw, xshape, act, route):
    """layer(x).backward(dy) with off-grid x, off-grid dy, flat-buffer parameters, and everything.  An off-grid x or dy moves the
    weight gradient from the vectorised bf16 kernel / the all-taps kernel to the generic one (wgrad_impl: fast_ok, wgrad_taps3_ok)
    and the data gradient onto the gather kernel: dx, dmu, drho and the bias gradients inside the envelopes of
    test_small_case_gradients_every_element.  Flat-buffer parameters alone change no kernel: equal bits.  The workspace
    btx_wgrad_workspace_bytes sizes without knowing the pointers covers whichever kernel they select (BTX_E_WORKSPACE would
    raise).  Small-integer x / dy: the weight gradient is exact, hence bit-equal to the aligned call's, on every route."""
    import bayesian_torch_amd as bt
    prec = "bf16" if act == BF16 else "f32"
    bf = act == BF16
    o1, o2 = OFFSETS[act]
    bt.set_precision(prec)
    try:
        layer = _make(cls, kw, None, seed=0, bt_seed=123)
        twin = _make(cls, kw, None, seed=0, bt_seed=123)
        flat_params(twin)
        tag = _tag(cls, kw, xshape)
        x = _x_of(xshape, act, seed=1, scale=1.0)
        bt.set_sample_index(layer, 5)
        with torch.no_grad():
            oshape = tuple(layer(x, return_kl=False).shape)
        got_route, chunks = _wgrad_route(layer, xshape, oshape, act, layer.mu_bias is not None)
        assert got_route == route and chunks > 1, (got_route, chunks)  # the slabs are reduced by wgrad_finish_kernel
        g = torch.Generator().manual_seed(2)
        dy = torch.randn(*oshape, generator=g).to(_dev()).to(act)
        if len(oshape) == 4:
            dy = dy.contiguous(memory_format=torch.channels_last)
        assert _on_grid(x, dy)
        runs = {"aligned": _bwd_run(layer, x, dy, 5),
                "x+%d" % o1: _bwd_run(layer, off_grid(x, o1), dy, 5),
                "dy+%d" % o2: _bwd_run(layer, x, off_grid(dy, o2), 5),
                "flat parameters": _bwd_run(twin, x, dy, 5),
                "everything": _bwd_run(twin, off_grid(x, o2), off_grid(dy, o1), 5)}
        for k in runs["aligned"]:
            assert torch.equal(runs["flat parameters"][k], runs["aligned"][k]), "flat-buffer parameters: %s differs" % k

        mu, rho = layer._w()
        op = _op_of(layer)
        flip = layer._family == "flipout"
        dx64, dmu64, A_dx, dd64, nz = _grads64(layer, x, dy, 5)
        w_shape = tuple(mu.shape)
        b_dx = E.bound(A_dx, prec, E.dgrad_reduction_length(w_shape, op), ref=dx64, store_bf16=bf)
        # bf16 x bf16 products are exact in f32 and the accumulation is f32: the f32 bound with no operand term, as for f32 inputs
        b_w = E.bound(E.wgrad_A(x, dy, w_shape, op), "f32", E.wgrad_reduction_length(oshape, op), delta_w=0.0)
        sig = torch.sigmoid(E.d64(rho)) * E.d64(nz["eps_w"])
        dW64 = dd64 if flip else dmu64
        log = _Log()
        for form, r in runs.items():
            nm = "%s %s" % (tag, form)
            log.check("dx " + nm, prec, r["dx"], dx64, b_dx)
            log.check("dmu " + nm, prec, r["dmu"], dmu64, b_w)
            log.check("drho " + nm, prec, r["drho"], dW64 * sig, _scaled(b_w, dW64, sig))
            if layer.mu_bias is not None:
                red = tuple(i for i in range(dy.dim()) if i != (dy.dim() - 1 if op["kind"] == "linear" else 1))
                gy64 = E.d64(dy)
                db64, A_b = gy64.sum(red), gy64.abs().sum(red)
                b_b = E.bound(A_b, "f32", E.wgrad_reduction_length(oshape, op), delta_w=0.0)
                log.check("dmu_b " + nm, prec, r["dmu_b"], db64, b_b)
                dbd64 = (gy64 * E.d64(nz["sign_out"].reshape(dy.shape))).sum(red) if flip else db64
                sig_b = torch.sigmoid(E.d64(layer.rho_bias)) * E.d64(nz["eps_b"])
                log.check("drho_b " + nm, prec, r["drho_b"], dbd64 * sig_b, _scaled(b_b, dbd64, sig_b))

        # ---- the integer weight gradient
        xi = E.small_ints(xshape, 31).to(_dev()).to(act)
        dyi = E.small_ints(oshape, 32).to(_dev()).to(act)
        if len(xshape) == 4:
            xi, dyi = xi.contiguous(memory_format=torch.channels_last), dyi.contiguous(memory_format=torch.channels_last)
        want = E.wgrad64(xi, dyi, w_shape, op)
        assert float(want.abs().max()) < 2 ** 24
        ints = {"aligned": _bwd_run(layer, xi, dyi, 5), "x+%d" % o2: _bwd_run(layer, off_grid(xi, o2), dyi, 5),
                "dy+%d" % o1: _bwd_run(layer, xi, off_grid(dyi, o1), 5),
                "everything": _bwd_run(twin, off_grid(xi, o1), off_grid(dyi, o2), 5)}
        for form, r in ints.items():
            rep = E.check_exact(r["dmu"], want)
            print(rep.line("exact dW_mu %s %s" % (tag, form), prec))
            if not rep.ok:
                log.bad.append("exact dW_mu %s %s: %s" % (tag, form, rep))
            assert torch.equal(r["dmu"], ints["aligned"]["dmu"])
        log.done()
    finally:
        bt.set_precision("f32")


def test_wgrad_finish_kernel_in_both_widths():
    """btx_contract_wgrad_ws with the rho fold on a two-chunk launch: rho and the gradient buffers on the grid take
    wgrad_finish_kernel<4>, rho 4 bytes off it takes <1>.  Both add the same slabs in the same chunk order: small-integer inputs,
    dW bit-equal and exact; drho = dW * eps * sigmoid(rho) inside the bound of test_small_case_gradients_every_element (dW exact:
    only the product's own roundings)."""
    from bayesian_torch_amd import _lib, functional as BF, rng
    cls, kw, xshape, act, _ = BWD[0]
    layer = _make(cls, kw, None, seed=0, bt_seed=123)
    op = layer._op
    mu, rho = layer._w()
    w_shape = tuple(mu.shape)
    x = E.small_ints(xshape, 31).to(_dev()).to(act).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        oshape = tuple(layer._forward_hip(x, sample_idx=5).shape)
    dy = E.small_ints(oshape, 32).to(_dev()).to(act).contiguous(memory_format=torch.channels_last)
    assert _wgrad_route(layer, xshape, oshape, act, True)[1] > 1 and mu.numel() % 4 == 0
    rho_f = BF.gemm_major_view(rho, op).reshape(-1)
    assert rho_f.is_contiguous() and rho_f.data_ptr() % 16 == 0
    res = {}
    for form, rf in (("rho on the grid", rho_f), ("rho+4", off_grid(rho_f, 4))):
        res[form] = BF.wgrad_hip(_lib.KIND_FLIPOUT, x, dy, op, rng.seed(), 5, layer._btx_layer_id, w_shape, bias=True, raw=True,
                                 rho_flat=rf)
    torch.cuda.synchronize()
    a, b = res["rho on the grid"], res["rho+4"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    with torch.no_grad():
        nz = layer.materialize_noise(5, tuple(x.shape), oshape, x.dtype, signs=True)
    si, so = E.d64(nz["sign_in"].reshape(x.shape)), E.d64(nz["sign_out"].reshape(oshape))
    dWd64 = E.wgrad64(E.d64(x) * si, E.d64(dy) * so, w_shape, _op_of(layer))
    sig = torch.sigmoid(E.d64(rho)) * E.d64(nz["eps_w"])
    log = _Log()
    for form, r in res.items():
        rep = E.check_exact(BF.gemm_major_logical_view(r[0], w_shape, op), E.wgrad64(x, dy, w_shape, _op_of(layer)))
        print(rep.line("exact dW_mu, " + form, "bf16"))
        assert rep.ok, str(rep)
        log.check("drho, " + form, "bf16", BF.gemm_major_logical_view(r[4], w_shape, op), dWd64 * sig,
                  _scaled(np.zeros(w_shape), dWd64, sig))
    log.done()


# =============================================================================================================================
# 3. pre-sampling, GraphedMC lanes, a captured training step on flat-buffer parameters
# =============================================================================================================================
def test_presample_and_graphed_lanes_on_flat_buffer_parameters():
    """btx_sample_weights_lanes refuses off-grid mu / rho (16-byte reads); gemm_major_view hands it aligned copies.  The
    criterion of test_gpu_lanes.py: pre-sampled tiles give the bits of per-layer sampling, a replay's lanes the bits of eager
    single samples — and here also the bits of the same model on aligned parameters."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc, functional as BF
    from test_gpu_lanes import _small_net
    dev = _dev()
    bt.manual_seed(8)
    net, twin = _small_net(dev), _small_net(dev)
    flat_params(twin)
    assert all(p.data_ptr() % 16 == 4 for p in twin.parameters()) and _on_grid(*net.parameters())
    x = torch.randn(4, 32, 12, 12, generator=torch.Generator().manual_seed(3)).to(dev)
    idx = [5, 6]
    with torch.no_grad():
        twin(x)  # the layers record the input shapes presample_item needs
        net(x)
        for pre in (False, True):
            outs = []
            for m in (net, twin):
                bt.set_sample_index(m, 9, presample=pre)
                outs.append(m(x).clone())
            assert torch.equal(outs[0], outs[1]), "presample=%s: flat-buffer parameters change the bits" % pre
            if pre:
                assert torch.equal(outs[1], plain)
            plain = outs[1]
        with BF.concurrent_plan():
            eager = []
            for i in idx:
                bt.set_sample_index(twin, i, presample=True)
                eager.append(twin(x).float().clone())
    g = mc.GraphedMC(twin, x, kl=0.0, lanes=2, keep_logits=True)
    try:
        for rep in range(2):
            g.run_many(idx)
            torch.cuda.synchronize()
            for l in range(2):
                assert torch.equal(g.lane_logits[l].float(), eager[l]), (rep, l)
    finally:
        g.close()


def test_captured_training_step_on_flat_buffer_parameters():
    """the realigning copies inside a captured region are ordinary nodes: GraphedTrainStep on a model whose parameters are views
    of one flat buffer at +4 bytes; the first replay against the eager step, the criterion of tests/test_gpu_optim.py
    (test_every_replay_gives_the_eager_gradients_biases_included: gradient rel-L2 1e-5)"""
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from test_gpu_optim import build, eager_backward
    net, x, y = build("conv")
    flat_params(net)
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())
    assert all(p.data_ptr() % 16 == 4 for p in params)
    eager_backward(net, x, y, 3)
    want = [p.grad.detach().clone() for p in params]
    gs = GraphedTrainStep(net, x, y)
    try:
        gs.run(3)
        torch.cuda.synchronize()
        errs = [float((p.grad - w).norm() / w.norm().clamp_min(1e-30)) for p, w in zip(params, want)]
        print("flat-buffer model, first replay: gradient rel-L2 max %.1e (%s)" % (max(errs), names[int(np.argmax(errs))]))
        assert all(torch.isfinite(p.grad).all() for p in params)
        assert max(errs) < 1e-5, dict(zip(names, errs))
    finally:
        gs.close()


# =============================================================================================================================
# 4. KL
# =============================================================================================================================
def test_kl_on_flat_buffer_parameters_against_float64():
    """kl_hip on off-grid mu / rho (kl_block_sum: the scalar path instead of 16-byte loads), get_kl_loss and its gradient on a
    layer whose parameters live in a flat buffer: the value and every gradient element with the bars of
    test_gpu_reductions.py (2e-6 relative on the value, envelope.kl_reference per element)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    layer = _make("Conv2dFlipout", dict(in_channels=32, out_channels=48, kernel_size=3, padding=1), "f32")
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for p in layer.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (2.0 if p is layer.rho_kernel or p is layer.rho_bias else 0.3)).to(p.device))
    flat_params(layer)
    mu, rho = layer._w()
    pm, ps = float(layer.prior_mean), float(layer.prior_variance)
    log = _Log()
    # ---- one tensor through btx_kl_gauss
    mu_f, rho_f = off_grid(mu.detach().reshape(-1)[:4099].contiguous(), 4), off_grid(rho.detach().reshape(-1)[:4099].contiguous(), 8)
    a_mu, a_rho = mu_f.clone(), rho_f.clone()
    assert _on_grid(a_mu, a_rho)
    k_off, k_al = float(BF.kl_hip(mu_f, rho_f, pm, ps)), float(BF.kl_hip(a_mu, a_rho, pm, ps))
    k64 = E.kl_reference(mu_f.cpu().double().numpy(), rho_f.cpu().double().numpy(), float(np.float32(pm)), float(np.float32(ps)), 1.0)[0]
    print("kl_hip n=4099: off-grid %.9g, aligned %.9g, float64 %.9g" % (k_off, k_al, k64))
    assert abs(k_off - k64) <= 2e-6 * abs(k64) and abs(k_al - k64) <= 2e-6 * abs(k64)
    # ---- the model KL and its gradient
    for p in layer.parameters():
        p.grad = None
    kl = bt.get_kl_loss(layer)
    (1.7 * kl).backward()
    torch.cuda.synchronize()
    tot = 0.0
    for name, m_, r_ in (("kernel", mu, rho), ("bias", layer.mu_bias, layer.rho_bias)):
        k, dmu, b_dmu, drho, b_drho = E.kl_reference(m_.detach().cpu().double().numpy(), r_.detach().cpu().double().numpy(),
                                                     float(np.float32(pm)), float(np.float32(ps)), float(np.float32(1.7)))
        tot += k
        assert m_.data_ptr() % 16 == 4 and m_.grad is not None
        log.check("kl flat-buffer %s dmu" % name, "f32", m_.grad, dmu, b_dmu)
        log.check("kl flat-buffer %s drho" % name, "f32", r_.grad, drho, b_drho)
    print("get_kl_loss on flat-buffer parameters: %.9g, float64 %.9g" % (float(kl), tot))
    assert abs(float(kl) - tot) <= 2e-6 * abs(tot)
    log.done()


# =============================================================================================================================
# 5. BatchNorm training, the pools: one aligned copy, the same launches, equal bits
# =============================================================================================================================
def _bn_run(bn, x, dy, res, relu):
    """test_gpu_reductions._bn_call without its clone of x (a clone would land on the grid again)"""
    from bayesian_torch_amd import autograd as ag
    x1 = x.detach().requires_grad_(True)
    r1 = res.detach().requires_grad_(True) if res is not None else None
    assert x1.data_ptr() == x.data_ptr() and ag.bn_train_usable(bn, x1), "this case must take the HIP kernels"
    for p in bn.parameters():
        p.grad = None
    y = ag.batch_norm_train(bn, x1, residual=r1, relu=relu)
    assert y.dtype == x.dtype and y.stride() == x.stride()
    y.backward(dy)
    torch.cuda.synchronize()
    return dict(y=y.detach(), dx=x1.grad, dgamma=bn.weight.grad.clone(), dbeta=bn.bias.grad.clone(),
                dres=r1.grad if r1 is not None else None, rm=bn.running_mean.detach().clone(), rv=bn.running_var.detach().clone(),
                nbt=bn.num_batches_tracked.detach().clone())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 8), (5, 40, 3, 7)], ids=["2x8", "5x40x3x7"])
def test_batchnorm_training_off_grid_equals_the_aligned_call(shape, dtype):
    """btx_bn_train_fwd / _bwd refuse x, y, res, dy, dx, dres off the grid (8 channels per 16-byte access); the wrapper makes one
    aligned copy with the same strides.  Plain, and ReLU + residual; 2-D and channels-last 4-D: y, dx, dres, dgamma, dbeta and the
    running estimates equal the aligned call's bit for bit."""
    from test_gpu_reductions import _bn_gauss, _bn_module
    x, dy, res = _bn_gauss(shape, dtype, 101)
    assert _on_grid(x, dy, res)
    o1, o2 = OFFSETS[dtype]
    for relu in (False, True):
        r = res if relu else None
        bn = _bn_module(shape, dtype)
        state = {k: v.clone() for k, v in bn.state_dict().items()}
        want = _bn_run(bn, x, dy, r, relu)
        forms = {"x+%d" % o1: (off_grid(x, o1), dy, r), "dy+%d" % o2: (x, off_grid(dy, o2), r),
                 "everything": (off_grid(x, o2), off_grid(dy, o1), off_grid(r, o1) if r is not None else None)}
        if r is not None:
            forms["residual+%d" % o1] = (x, dy, off_grid(r, o1))
        for form, (xa, dya, ra) in forms.items():
            bn.load_state_dict(state)
            got = _bn_run(bn, xa, dya, ra, relu)
            for k, w in want.items():
                assert (w is None) == (got[k] is None), (form, k)
                if w is not None:
                    assert torch.equal(got[k], w), "bn %s %s relu=%s %s: %s differs" % (shape, _N[dtype], relu, form, k)
                    assert got[k].stride() == w.stride()
        assert float(want["y"].abs().max()) > 0 and int(want["nbt"]) == 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_pools_off_grid_equal_the_aligned_call(dtype):
    """max-pool training forward / backward (MaxPool2dTrainFn), maxpool2d_hip, avgpool_global_hip: the entry points refuse off-grid
    tensors, the wrappers realign; equal bits, and the max-pool equal to torch's own on the CPU copy"""
    from bayesian_torch_amd import autograd as ag, functional as BF
    shape, k, s, p = (2, 16, 9, 9), 3, 2, 1
    o1, o2 = OFFSETS[dtype]
    x = E.small_ints(shape, 51, lim=7).to(dtype).to(_dev()).contiguous(memory_format=torch.channels_last)
    mp = torch.nn.MaxPool2d(k, s, p)
    xc = x.detach().cpu().double().requires_grad_(True)
    yc = torch.nn.functional.max_pool2d(xc, k, s, p)
    dy = E.small_ints(tuple(yc.shape), 52).to(dtype).to(_dev()).contiguous(memory_format=torch.channels_last)
    yc.backward(dy.cpu().double())
    assert _on_grid(x, dy)

    def run(xa, dya):
        x1 = xa.detach().requires_grad_(True)
        assert ag.max_pool_train_usable(mp, x1)
        y = ag.max_pool_train(mp, x1)
        y.backward(dya)
        return y.detach(), x1.grad
    want = run(x, dy)
    assert E.check_exact(want[0], yc.detach()).ok and E.check_exact(want[1], xc.grad).ok
    for form, (xa, dya) in {"x": (off_grid(x, o1), dy), "dy": (x, off_grid(dy, o2)), "both": (off_grid(x, o2), off_grid(dy, o1))}.items():
        got = run(xa, dya)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), form
        assert got[0].stride() == want[0].stride() and got[1].stride() == want[1].stride()
    for o in (o1, o2):
        xo = off_grid(x, o)
        assert torch.equal(BF.maxpool2d_hip(xo, k, s, p), BF.maxpool2d_hip(x, k, s, p))
        assert torch.equal(BF.maxpool2d_hip(xo, k, s, p), want[0])
        assert torch.equal(BF.avgpool_global_hip(xo), BF.avgpool_global_hip(x))
    ref = E.avgpool_exact(x.permute(0, 2, 3, 1).reshape(shape[0], -1, shape[1]).float().cpu(), dtype)
    assert E.check_exact(BF.avgpool_global_hip(off_grid(x, o1)), ref).ok


# =============================================================================================================================
# 6. MC accumulate
# =============================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_mc_accumulate_off_grid_logits_against_float64(dtype):
    """mc.accumulate / accumulate_lanes read the logits element by element: off-grid logits, every entry against the float64
    softmax with the bounds of test_gpu_reductions._mc_check, and the bits of the aligned call"""
    from bayesian_torch_amd import mc
    from test_gpu_reductions import _mc_logits
    log = _Log()
    bs, C = 3, 1000
    for lanes, o in zip((1, 2), OFFSETS[dtype]):
        x = _mc_logits(lanes, bs, C, 300 + lanes, dtype)
        lg = x.reshape(lanes * bs, C).to(_dev())
        packs = []
        for t in (lg, off_grid(lg, o)):
            packed = torch.zeros(mc.packed_numel(bs, C), dtype=F32, device=_dev())
            if lanes == 1:
                mc.accumulate(packed, t, kl=1.5)
            else:
                mc.accumulate_lanes(packed, t, lanes, kl=1.5)
            packs.append(packed)
        torch.cuda.synchronize()
        assert torch.equal(packs[0], packs[1])
        pk = packs[1].cpu()
        ref = E.mc_reference(x.double().numpy())
        name = "mc logits+%d lanes=%d C=%d bs=%d" % (o, lanes, C, bs)
        log.check(name + " sum p", _N[dtype], pk[:bs * C].reshape(bs, C), ref["sum_p"], ref["b_sum_p"])
        log.check(name + " sum p^2", _N[dtype], pk[bs * C:2 * bs * C].reshape(bs, C), ref["sum_p2"], ref["b_sum_p2"])
        log.check(name + " entropy", _N[dtype], pk[2 * bs * C:2 * bs * C + bs], ref["ent"], ref["b_ent"])
        log.check(name + " kl, count", _N[dtype], pk[2 * bs * C + bs:], np.array([1.5 * lanes, float(lanes)]), np.zeros(2))
    log.done()


# =============================================================================================================================
# 7. INT8
# =============================================================================================================================
def _np(t):
    return t.detach().cpu().numpy()


def _qt(a, s, z, off=0):
    from bayesian_torch_amd.q8 import QTensor
    q = QTensor(torch.from_numpy(np.ascontiguousarray(a)).to(_dev()), s, z)
    if off:
        q = QTensor(off_grid(q.q, off), s, z)
        assert q.q.data_ptr() % 16 == off
    return q


@pytest.mark.parametrize("bias", [True, False])
def test_q8_contraction_off_grid_x_and_residual_equal_the_model(bias):
    """btx_q8_contract / _res with C % 16 == 0 and N % 4 == 0 (the aligned call loads x in 16-byte chunks, the residual in words):
    x at +1 / +4 bytes takes the bytewise loads (x_vec), the residual at +1 / +4 the bytewise / word loads (res_vec).  Integer
    arithmetic: the bytes of tests/q8_model.py / q8_net_model.py, and of the aligned call."""
    from test_gpu_q8_net import CONV_ZO, RES_CONV, res_case, res_model
    import q8_model as Q
    idx = 0
    cin, cout = RES_CONV[idx][:2]
    assert cin % 16 == 0 and cout % 4 == 0
    c = res_case(idx, bias)
    q = c["q"].to(_dev())
    s_eps, s_d, s_w = c["chain"]
    noise = dict(eps_w=c["eps"], eps_b=c["eps_b"])
    z_r, z_add, add_relu, conv_relu = 131, 120, True, False
    z_o = CONV_ZO[z_r]
    q.quant_dict = [(s_eps, 0), (s_d, 0), (s_w, 0), (c["s_x"], c["z_x"]), (c["s_o"], z_o)]
    q.relu = conv_relu
    o_ref, sum_ref = res_model(c, z_r, z_add, add_relu, conv_relu)
    try:
        with torch.no_grad():
            for ox in (0,) + OFFSETS[U8]:
                xq = _qt(c["x_i"], c["s_x"], c["z_x"], ox)
                assert xq.q.is_contiguous(memory_format=torch.channels_last)
                plain = q.forward_int8(xq, noise=noise)
                assert np.array_equal(_np(plain.int_repr()), o_ref), "x+%d: the plain contraction differs from the model" % ox
                for orr in (0,) + OFFSETS[U8]:
                    res = _qt(c["res"], c["s_r"], z_r, orr)
                    fused = q.forward_int8(xq, noise=noise, residual=res, add_relu=add_relu, add_scale=None, add_zero_point=z_add)
                    assert np.array_equal(_np(fused.int_repr()), sum_ref), "x+%d residual+%d differs from the model" % (ox, orr)
    finally:
        q.quant_dict, q.relu = None, False
    assert 0 < float(((sum_ref == 0) | (sum_ref == 255)).mean()) < 0.9


def test_q8_flipout_contraction_off_grid_x_equals_the_model():
    """btx_q8_contract_flipout, C = 16, N = 64: x at +1 / +4 bytes; every output of the pre-pass and the contraction against
    tests/q8_flipout_model.py (test_gpu_q8_flipout._check)"""
    from test_gpu_q8_flipout import _case, _check
    c = _case("conv", "c16n64s2")
    assert c["mu"].shape[1] % 16 == 0 and c["mu"].shape[0] % 4 == 0
    for o in OFFSETS[U8]:
        _check(c, float_input=_qt(c["x_i"], *c["e_x"], off=o))


def test_q8_pools_off_grid_equal_the_model():
    """q8.max_pool2d / avg_pool2d with C % 16 == 0: an off-grid x takes the bytewise kernel (q8_pool_launch: vec)"""
    from bayesian_torch_amd import q8
    import q8_net_model as QN
    from test_gpu_q8_net import _bytes
    x = _bytes((2, 16, 9, 9), 7)
    xa = _bytes((2, 64, 7, 7), 11)
    for o in (0,) + OFFSETS[U8]:
        out = q8.max_pool2d(_qt(x, 0.1, 77, o), 3, 2, 1)
        assert np.array_equal(_np(out.int_repr()), QN.max_pool(x, 3, 2, 1)), o
        assert out.int_repr().is_contiguous(memory_format=torch.channels_last)
        out = q8.avg_pool2d(_qt(xa, 0.1, 77, o), 7, 1)
        assert np.array_equal(_np(out.int_repr()), QN.avg_pool(xa, 77, 7, 1)), o


# =============================================================================================================================
# 8. kernels without a wide global access: fused LSTM, rowfuse_pack, the calibration losses
# =============================================================================================================================
@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_fused_lstm_forward_and_backward_off_grid_equal_the_aligned_call(cls):
    """btx_lstm_fwd_train / btx_lstm_bwd read x, h0, c0 and the parameters element by element: off-grid inputs and flat-buffer
    parameters give the aligned call's bits (the kernels are deterministic: test_gpu_lstm_train_fused.py)"""
    import bayesian_torch_amd as bt
    from test_gpu_lstm_train_fused import make
    I, H, B, T = 12, 10, 4, 6
    dev = _dev()
    bt.set_precision("f32")
    bt.manual_seed(77)
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    x0, h00, c00, r_h, r_c = rn(B, T, I), rn(B, H), rn(B, H), rn(B, T, H), rn(B, T, H)
    res = {}
    for mode in ("aligned", "off"):
        layer = make(cls, I, H, seed=4)
        bt.assign_layer_ids(layer, start=700)
        layer.fused_training = layer.fused_sequence = True
        if mode == "off":
            flat_params(layer)
        bt.set_sample_index(layer, 9)
        mk = (lambda t, o: off_grid(t, o).detach().requires_grad_()) if mode == "off" else (lambda t, o: t.clone().requires_grad_())
        x, h0, c0 = mk(x0, 4), mk(h00, 8), mk(c00, 4)
        assert (x.data_ptr() % 16 == 4) == (mode == "off")
        hs, (_, cs), kl = layer(x, (h0, c0))
        ((hs * r_h).sum() + (cs * r_c).sum() + kl).backward()
        torch.cuda.synchronize()
        res[mode] = [hs.detach(), cs.detach(), kl.detach(), x.grad, h0.grad, c0.grad] + [p.grad for p in layer.parameters()]
        bt.set_sample_index(layer, 9)
        with torch.no_grad():  # the inference sequence (btx_lstm_fwd) on the same tensors
            hi, (_, ci), ki = layer(x.detach(), (h0.detach(), c0.detach()))
        assert torch.equal(hi, hs) and torch.equal(ci, cs) and torch.equal(ki, kl)
    for k, (a, b) in enumerate(zip(res["aligned"], res["off"])):
        assert a is not None and b is not None and torch.equal(a, b), k


def test_rowfuse_pack_off_grid_equals_the_aligned_call():
    from bayesian_torch_amd import functional as BF
    op = BF.OpDesc(2, 3, 64, 7, 2, 3)
    for dt in (F32, BF16):
        x = _x_of((2, 3, 30, 26), dt)
        plan = BF.rowfuse_plan(op, tuple(x.shape))
        assert plan is not None
        for out_dt in (F32, BF16):
            want = BF.rowfuse_input(x, plan, out_dt)
            for o in OFFSETS[dt]:
                assert torch.equal(BF.rowfuse_input(off_grid(x, o), plan, out_dt), want), (dt, out_dt, o)


def test_calibration_losses_off_grid_equal_the_aligned_call():
    """AvUC / AUAvUC on off-grid logits (f32 and bf16), EaU / EaC on off-grid error / uncertainty vectors: the fused kernels read
    element by element: loss and gradients equal the aligned call's bits"""
    from avuc_cases import load
    from bayesian_torch_amd.utils import avuc_loss as A
    from bayesian_torch_amd.utils import uncertainty_calibration_loss as U
    c = load()["avu"]["b37_c257"]
    lb = torch.from_numpy(c["labels"]).to(_dev())
    for dt in (F32, BF16):
        for area in (False, True):
            outs = []
            for o in (0,) + OFFSETS[dt]:
                lg = torch.from_numpy(c["logits"]).to(_dev()).to(dt)
                lg = (off_grid(lg, o) if o else lg).detach().requires_grad_(True)
                assert lg.data_ptr() % 16 == o
                if area:
                    loss, r = A.AUAvULoss(beta=float(c["beta"]))(lg, lb)
                else:
                    loss, r = A.AvULoss(beta=float(c["beta"]))(lg, lb, float(c["th"])), None
                loss.sum().backward()
                outs.append((loss.detach(), r, lg.grad))
            for got in outs[1:]:
                assert torch.equal(got[0], outs[0][0]) and torch.equal(got[2], outs[0][2]), (dt, area)
                assert got[1] is None or torch.equal(got[1].detach(), outs[0][1].detach())
    e_name = sorted(load()["eau"])[0]
    c = load()["eau"][e_name]
    for conf_form in (False, True):
        mod = (U.EaCLoss if conf_form else U.EaULoss)(beta=float(c["beta"]))
        outs = []
        for o in (0,) + OFFSETS[F32]:
            e = torch.from_numpy(c["error"]).to(_dev())
            u = torch.from_numpy(c["conf" if conf_form else "unc"]).to(_dev())
            e = (off_grid(e, o) if o else e).detach().requires_grad_(True)
            u = (off_grid(u, o) if o else u).detach().requires_grad_(True)
            loss = mod(e, u, float(c["error_th"]), float(c["conf_th" if conf_form else "unc_th"]))
            loss.backward()
            outs.append((loss.detach(), e.grad, u.grad))
        for got in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(got, outs[0])), conf_form
