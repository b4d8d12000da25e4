"""GPU: every element of the kernels' results against a float64 reference — rounding envelopes, exact-integer runs and impulse
probes (tests/envelope.py).  The rel-L2 tests of the other files say that a tensor is 0.3 % off on average; these
say WHICH element is wrong: no element is excluded, there is no percentile and no mean.

  1. envelope    |got - ref| <= c * A element by element, A the same contraction on absolute values in float64 on the CPU, c
                 derived per precision (envelope.py): the cases of the other files, imported, not copied.
  2. exact       small-integer x / dy (and dyadic mu with rho = -200, sigma = 0 exactly): every partial sum is an integer below
                 2^24, so f32 accumulation is exact in ANY order and the kernels must return the float64 result bit for bit at
                 full size — weight gradients (each pixel chunk counted exactly once; slab and atomics paths), bias gradients,
                 the deterministic half of forward and data gradient, max-pool forward and backward.
  3. impulse     one-hot inputs make every output a single product: an f32 launch returns the weights the kernel sampled for
                 itself.  Their relative error against float64 IS delta_w (envelope.DELTA_W = 2 x the maximum measured here).

Left on rel-L2, on purpose: the LSTM sequences (test_gpu_lstm_*.py) — the recurrence is nonlinear, no per-element bound follows
from first principles, and btx_lstm_bwd cannot be fed integers end to end (its gates are transcendental).  The reducing kernels
— training BatchNorm, mc_accumulate, the KL gradients, the global average pool — have their own file, test_gpu_reductions.py.
The stem + max-pool launch cannot be read back by an impulse (BN, ReLU and the pool sit between the weights
and the store): its envelope runs through BN + ReLU + store + pool at batch 64 instead.

Each check prints one line `name prec: worst err/bound R at (n, c, h, w)`; profiles/elementwise_envelope.txt holds the lines of
the first full run.  float64 references are built on the CPU with at most 16 threads and reused for value, envelope and both
launch forms.
"""
import itertools
import math
import warnings

import pytest
import torch

import envelope as E
from autograd_cases import dev as _dev, make as _make, Log as _Log, grads64 as _grads64, scaled as _scaled  # moved there, unchanged
from test_gpu_at_size import CPU_CASES
from test_gpu_backward import CASES as BWD_CASES, CPU_BWD_CASES, RN18_SHAPES, _op_of
from test_gpu_backward import test_hip_maxpool_under_autograd_equals_torch as _maxpool_test
from test_gpu_contract import FUSED_CASES, PRECS, _random_conv_cases
from test_gpu_fuse_model import CASES as EPI_CASES, _plan
from test_gpu_lanes import test_tall_strip_tiles_vs_oracle_chain as _tall_strip_test
from test_gpu_lanes import _WIDE_512, _lanes_vs_singles
from test_gpu_lanes import _layer as _lanes_layer

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))


def _params_of(test_fn):
    return [m for m in test_fn.pytestmark if m.name == "parametrize"][0].args[1]


def _refs(layer, x, out_shape, sample):
    """float64 value of the layer for MC sample `sample` on the CPU, with the noise BTX-RNG v1 defines, and its envelope parts:
    (ref, A, A_bias, K)"""
    with torch.no_grad():
        nz = layer.materialize_noise(sample, tuple(x.shape), tuple(out_shape), x.dtype)
    mu, rho = layer._w()
    flip = layer._family == "flipout"
    si = nz["sign_in"].reshape(x.shape) if flip else None
    so = nz["sign_out"].reshape(out_shape) if flip else None
    op = _op_of(layer)
    with torch.no_grad():
        ref, A, Ab = E.reference_forward(x, mu, rho, nz["eps_w"], layer.mu_bias, layer.rho_bias, nz.get("eps_b"), si, so, op)
    return ref, A, Ab, E.reduction_length(tuple(mu.shape), op)


def _tag(cls, kw, xshape):
    k = kw.get("kernel_size", "")
    return "%s(%s->%s%s%s%s%s)x%s" % (cls.replace("Reparameterization", "Rep"), kw.get("in_channels", kw.get("in_features")),
                                      kw.get("out_channels", kw.get("out_features")), ",k%s" % (k,) if k != "" else "",
                                      ",s%s" % (kw["stride"],) if kw.get("stride", 1) != 1 else "",
                                      ",d%s" % (kw["dilation"],) if kw.get("dilation", 1) != 1 else "",
                                      ",g%d" % kw["groups"] if kw.get("groups", 1) != 1 else "", "x".join(map(str, xshape)))


# =============================================================================================================================
# 3. impulse probes (first: they measure delta_w, which the envelopes below use)
# =============================================================================================================================
def _impulse_like(xshape, op, of_output=False, rnd=0, slot=0):
    """one-hot images: impulses so far apart that no two reach the same output (input) element, channel cycling with the slot,
    the grid shifted from image to image and from round to round so that corners, borders, tile seams and every stride parity
    are visited -> (x, next slot)"""
    n, c = xshape[0], xshape[1]
    sp = tuple(xshape[2:])
    x = torch.zeros(xshape)
    if not sp:
        for i in range(n):
            x[i, (slot + i) % c] = 1.0  # Linear: rows cycle through the input features
        return x, slot + n
    nd = len(sp)
    k, s, d = op.kernel[3 - nd:], op.stride[3 - nd:], op.dilation[3 - nd:]
    step = []
    for a in range(nd):
        ext = d[a] * (k[a] - 1) + 1
        # forward of a plain convolution / gradient of a transposed one: impulses `ext` apart, and coprime with the stride so
        # that every parity is visited; the other direction spreads an impulse over ext positions of a grid `stride` times finer
        spread = op.transposed != of_output
        st = -(-ext // s[a]) if spread else ext
        while not spread and math.gcd(st, s[a]) != 1:
            st += 1
        step.append(max(st, 1))
    for i in range(n):
        starts = [((i + rnd) * (a + 1) + rnd // step[a]) % step[a] for a in range(nd)]
        for pos in itertools.product(*[range(starts[a], sp[a], step[a]) for a in range(nd)]):
            x[(i, (slot * 2654435761 >> 11) % c) + pos] = 1.0  # Knuth's multiplicative hash: no pattern shared with the grid
            slot += 1
        slot += 1  # de-correlate the channel cycle from the grid
    return x, slot


def _impulse_rounds(layer, xshape, max_rounds=48):
    """impulse inputs of the layer's own shape (so the launch stays on its kernel family), as many rounds as it takes until every
    (n, tap, c) weight has been the single product of some output -> (list of x, output shape)"""
    op = _op_of(layer)
    w_shape = tuple(layer._w()[0].shape)
    cover = torch.zeros(w_shape, dtype=torch.float64)
    xs, slot, oshape = [], 0, None
    while len(xs) < max_rounds and (not xs or bool((cover == 0).any())):
        x, slot = _impulse_like(xshape, layer._op, rnd=len(xs), slot=slot)
        if oshape is None:
            oshape = tuple(E.contract(x.double(), torch.zeros(w_shape, dtype=torch.float64), None, op).shape)
        cover += E.wgrad64(x, torch.ones(oshape), w_shape, op)
        xs.append(x)
    assert bool((cover > 0).all()), "impulses probe %.1f%% of the weights" % (100 * float((cover > 0).double().mean()))
    return xs, oshape


def _spread_rho(layer):
    """rho over the range the layers use: even output channels uniform in [-9, 2], odd ones MOPED-style log(expm1(0.5 |mu|))"""
    from oracle import bt_ref
    mu, rho = layer._w()
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        wide = (torch.rand(tuple(rho.shape), generator=g) * 11.0 - 9.0).to(rho.device)
        moped = bt_ref.get_rho(mu.detach(), 0.5)
        sel = (torch.arange(rho.shape[0], device=rho.device) % 2 == 0).reshape((-1,) + (1,) * (rho.dim() - 1))
        rho.copy_(torch.where(sel, wide, moped))


IMPULSE_CASES = [(cls, dict(kw, bias=False), xs, gather) for cls, kw, xs, gather in EPI_CASES] + [
    # a transposed layer (every output phase is one tap of one impulse) and a strided pointwise one from FUSED_CASES
    (FUSED_CASES[14][0], dict(FUSED_CASES[14][1], bias=False), (4,) + tuple(FUSED_CASES[14][2][1:]), False),
    (FUSED_CASES[47][0], dict(FUSED_CASES[47][1]), FUSED_CASES[47][2], False),
]
_DELTA = {}


@pytest.mark.parametrize("case", IMPULSE_CASES, ids=[_tag(*c[:3]) for c in IMPULSE_CASES])
def test_impulse_forward_reads_back_the_sampled_weights(case):
    """x one-hot: out[n, p - tap] = mu[n,tap,c] + s_in s_out (sigma eps)[n,tap,c], one product, nothing accumulated.  f32: the
    output IS the weight the kernel sampled -> delta_w = max |got - w64| / (|mu| + |sigma eps|), asserted <= envelope.DELTA_W
    (twice the first measurement).  bf16 / bf16x3: the rounding of one operand on top (x = 1 is exact).  Outputs no impulse
    reaches are exactly 0.  Lane l of a 2-lane launch returns the weights of sample s_l."""
    import bayesian_torch_amd as bt
    cls, kw, xshape, gather = case
    assert FUSED_CASES[14][0].startswith("ConvTranspose2d") and FUSED_CASES[47][1].get("stride") == 2
    log = _Log()
    u = E.U_BF16
    xs_cpu, _ = _impulse_rounds(_make(cls, kw, "f32"), xshape)
    tag = _tag(cls, kw, xshape)
    for prec, act in (("f32", torch.float32), ("bf16x3", torch.float32), ("bf16", torch.bfloat16)):
        layer = _make(cls, kw, prec)
        _spread_rho(layer)
        rc, fam, _ = _plan(layer, xshape, prec, gather=gather)
        worst = 0.0
        for rnd, x0 in enumerate(xs_cpu):
            x = x0.to(_dev()).to(act)
            runs = []
            with torch.no_grad():
                out = layer._forward_hip(x, sample_idx=7 + rnd, gather=gather)
                runs.append((7 + rnd, out, "single"))
                if rnd == 0:  # lane l of one launch returns the weights of sample s_l
                    shared = kw.get("in_channels") == 3
                    bt.set_sample_lanes(layer, [7, 21], batch=xshape[0])
                    out2 = layer._forward_hip(x if shared else torch.cat([x, x], 0), gather=gather)
                    bt.set_sample_lanes(layer, None)
                    n = out.shape[0]
                    runs += [(7, out2[:n], "lane0"), (21, out2[n:], "lane1")]
            torch.cuda.synchronize()
            for sample, got, form in runs:
                ref, A, _, _ = _refs(layer, x, out.shape, sample)
                name = "impulse %s round %d %s [%s]" % (tag, rnd, form, fam)
                if prec == "f32":
                    ratio = torch.where(A > 0, (got.double().cpu() - ref).abs() / A.clamp_min(1e-300), torch.zeros_like(A))
                    worst = max(worst, float(ratio.max()))
                    bnd = E.DELTA_W * A
                elif prec == "bf16x3":  # w = w_h + w_l up to u^2; the Flipout combine is one rounding, adding zeros is exact
                    bnd = (u * u + E.DELTA_W + 8 * E.ACC_UNIT) * A
                else:                   # w rounded once, the result rounded on store
                    bnd = E.store_rounding((u + E.DELTA_W * (1 + u) + 8 * E.ACC_UNIT) * A, ref)
                rep = E.check(got, ref, bnd)
                if rnd == 0 or not rep.ok:
                    print(rep.line(name, prec))
                if not rep.ok:
                    log.bad.append("%s %s: %s" % (name, prec, rep))
        if prec == "f32":
            _DELTA[tag] = worst
            print("impulse %s f32 [%s]: %d rounds cover every (n, tap, c); delta_w measured %.4g" % (tag, fam, len(xs_cpu), worst))
    log.done()


def test_impulse_probes_reach_every_family_and_report_delta_w():
    families = set()
    for cls, kw, xs, gather in IMPULSE_CASES:
        for prec in PRECS:
            rc, fam, _ = _plan(_make(cls, kw, prec), xs, prec, gather=gather)
            assert rc == 0
            families.add(fam)
    assert {"gather", "regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem"} <= families, families
    if _DELTA:
        worst = max(_DELTA.values())
        print("delta_w: measured maximum %.4g over %d probes; envelope.DELTA_W = %.4g" % (worst, len(_DELTA), E.DELTA_W))
        assert worst <= E.DELTA_W


IMPULSE_BWD = [BWD_CASES[i] for i in (1, 3, 4, 5, 6, 11, 12, 13, 14, 15)]


@pytest.mark.parametrize("cls,kw,xshape", IMPULSE_BWD, ids=[_tag(*c) for c in IMPULSE_BWD])
def test_impulse_data_gradient_reads_back_the_sampled_weights(cls, kw, xshape):
    """dy one-hot: dx is one sampled weight per reached input pixel (the parity-major stride-2 launches and transposed layers
    included), every other dx element exactly 0; x small integers, so dW_mu[n,tap,c] = x[p + tap, c] summed over the impulses
    is exact"""
    import bayesian_torch_amd as bt
    bt.set_precision("f32")
    layer = _make(cls, dict(kw, bias=False), None, seed=0, bt_seed=123)
    _spread_rho(layer)
    x = E.small_ints(xshape, 8).to(_dev()).requires_grad_(True)
    bt.set_sample_index(layer, 5)
    out = layer(x, return_kl=False)
    dy = _impulse_like(tuple(out.shape), layer._op, of_output=True)[0].to(_dev())
    out.backward(dy)
    mu, rho = layer._w()
    dx64, dmu64, A = _grads64(layer, x.detach(), dy, 5)[:3]
    log = _Log()
    # one product, one Flipout combine
    log.check("impulse dgrad " + _tag(cls, kw, xshape), "f32", x.grad, dx64, (E.DELTA_W + 2 * E.REF32_UNIT) * A)
    rep = E.check_exact(mu.grad, dmu64)
    print(rep.line("impulse dW_mu exact " + _tag(cls, kw, xshape), "f32"))
    assert float((A > 0).double().mean()) > 0.02
    assert rep.ok, str(rep)
    log.done()


# =============================================================================================================================
# 1. envelopes on the cases of the other files
# =============================================================================================================================
def _fused_envelope(log, idx, cls, kw, xshape, prec, act, sample=3, seed_init=11):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(2024)
    torch.manual_seed(seed_init)          # the construction of test_gpu_contract._run_fused
    layer = getattr(L, cls)(**kw).to(_dev())
    layer.precision = prec
    bt.assign_layer_ids(layer)
    x = torch.randn(*xshape).to(_dev())
    if act == "bf16":
        x = x.to(torch.bfloat16)
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=sample)
    ref, A, Ab, K = _refs(layer, x, out.shape, sample)
    bnd = E.bound(A, prec, K, ref=ref, A_bias=Ab, store_bf16=(act == "bf16"))
    return log.check("%d %s" % (idx, _tag(cls, kw, xshape)), "%s/%s" % (prec, act), out, ref, bnd)


@pytest.mark.parametrize("prec,act", [("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16"), ("f32", "bf16"), ("bf16x3", "f32")])
def test_fused_cases_every_element_inside_the_envelope(prec, act):
    log = _Log()
    for i, (cls, kw, xshape) in enumerate(FUSED_CASES):
        _fused_envelope(log, i, cls, kw, xshape, prec, act)
    log.done()


@pytest.mark.parametrize("prec", PRECS)
def test_random_geometries_every_element_inside_the_envelope(prec):
    log = _Log()
    for i, (cls, kw, xshape) in enumerate(_random_conv_cases(48, 20260925 + PRECS.index(prec))):
        _fused_envelope(log, i, cls, kw, xshape, prec, "bf16" if prec == "bf16" else "f32", sample=i, seed_init=100 + i)
    log.done()


_REF_CACHE = {}


def _cached_refs(key, make):
    """one float64 reference at a time (the largest is 0.8 GB): reused by the precisions that share the input"""
    if _REF_CACHE.get("key") != key:
        _REF_CACHE.clear()
        _REF_CACHE.update(key=key, val=make())
    return _REF_CACHE["val"]


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])  # the upper decorator varies fastest: f32 and bf16x3 share a reference
@pytest.mark.parametrize("case", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_kernel_families_at_baseline_batch_every_element(case, prec):
    """the cases of test_kernel_families_at_baseline_batch_vs_cpu_reference, built the same way: single launch and lane 1 of a
    2-lane launch against ONE float64 CPU reference"""
    import bayesian_torch_amd as bt
    name, cls, kw, xshape = case
    layer = _make(cls, kw, prec)
    act = torch.bfloat16 if prec == "bf16" else torch.float32
    torch.manual_seed(1234)
    x = torch.randn(*xshape).to(_dev()).to(act)
    if len(xshape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=9)
        shared = kw.get("in_channels") == 3
        bt.set_sample_lanes(layer, [8, 9], batch=xshape[0])
        out2 = layer._forward_hip(x if shared else torch.cat([x, x], 0))[xshape[0]:]
        bt.set_sample_lanes(layer, None)
    torch.cuda.synchronize()
    ref, A, Ab, K = _cached_refs((name, act), lambda: _refs(layer, x, out.shape, 9))
    bnd = E.bound(A, prec, K, ref=ref, A_bias=Ab, store_bf16=(prec == "bf16"))
    log = _Log()
    log.check("%s batch %d single" % (name, xshape[0]), prec, out, ref, bnd)
    log.check("%s batch %d lane1of2" % (name, xshape[0]), prec, out2, ref, bnd)
    log.done()


def test_stem_with_fused_bn_relu_maxpool_at_bs64_every_element():
    """the one-launch stem of the bench (conv1 + eval-BN + ReLU + MaxPool2d(3,2,1), bf16, batch 64): the envelope of the
    convolution carried through the affine, the ReLU (1-Lipschitz), the bf16 store and the pool (max of the bounds)"""
    layer = _make("Conv2dFlipout", dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), "bf16")
    torch.manual_seed(1234)
    x = torch.randn(64, 3, 224, 224).to(_dev()).to(torch.bfloat16)
    scale = (0.5 + torch.rand(64)).to(_dev())
    shift = (0.1 * torch.randn(64)).to(_dev())
    assert layer.pool_fusable(x)
    with torch.no_grad():
        got = layer.forward_fused(x, scale, shift, None, True, pool=True)
    torch.cuda.synchronize()
    pre, A, _, K = _refs(layer, x, (64, 64, 112, 112), layer._btx_sample - 1)
    s64, t64 = E.d64(scale).view(1, -1, 1, 1), E.d64(shift).view(1, -1, 1, 1)
    act = torch.relu(pre * s64 + t64)
    ref = torch.nn.functional.max_pool2d(act, 3, 2, 1)
    b = E.store_rounding(E.through_affine(E.bound(A, "bf16", K), pre, scale, shift), act)
    log = _Log()
    log.check("stem+bn+relu+maxpool batch 64", "bf16", got, ref, E.through_maxpool2d(b, 3, 2, 1))
    assert got.shape == (64, 64, 56, 56)
    log.done()


@pytest.mark.parametrize("cin,cout,hw,bs", _params_of(_tall_strip_test))
def test_tall_strip_tiles_every_element(cin, cout, hw, bs):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(5)
    torch.manual_seed(3)
    layer = L.Conv2dFlipout(cin, cout, 3, padding=1, bias=True).to(_dev())
    bt.assign_layer_ids(layer)
    x = torch.randn(bs, cin, hw, hw, device=_dev()).contiguous(memory_format=torch.channels_last)
    log = _Log()
    for prec in ("f32", "bf16"):
        layer.precision = prec
        xin = x if prec == "f32" else x.to(torch.bfloat16)
        with torch.no_grad():
            out = layer._forward_hip(xin, sample_idx=9)
        ref, A, Ab, K = _refs(layer, xin, out.shape, 9)
        log.check("tall strip %dx%dx%dx%d" % (bs, cin, hw, hw), prec, out, ref,
                  E.bound(A, prec, K, ref=ref, A_bias=Ab, store_bf16=(prec == "bf16")))
    log.done()


def test_wide_tile_with_split_k_every_element():
    """the wide Reparameterization tile with a K split: partial sums + reduce launch (its combine is inside the +8)"""
    (cls, kw), xshape, S = _WIDE_512, (16, 512, 7, 7), 20
    import bayesian_torch_amd as bt
    layer = _lanes_layer(cls, dict(kw, bias=True), "bf16", seed=5)
    bt.assign_layer_ids(layer)
    idx = [40 + l for l in range(S)]
    lanes, singles, xs = _lanes_vs_singles(layer, xshape, torch.bfloat16, idx)
    log = _Log()
    for l in (0, 7, S - 1):
        ref, A, Ab, K = _refs(layer, xs[l], lanes[l].shape, idx[l])
        log.check("wide split-K lane %d" % l, "bf16", lanes[l], ref, E.bound(A, "bf16", K, ref=ref, A_bias=Ab, store_bf16=True))
    log.done()


@pytest.mark.parametrize("prec,act", [("f32", torch.float32), ("bf16x3", torch.float32), ("bf16", torch.bfloat16)],
                         ids=["f32", "bf16x3", "bf16"])
def test_epilogue_bn_residual_relu_every_element(prec, act):
    """the store of every kernel family with eval-BN scale / shift, a residual and none / ReLU / ReLU6 folded in: the bound goes
    through the affine, the residual adds nothing but the store's rounding, the activations are 1-Lipschitz"""
    log = _Log()
    for cls, kw, xs, gather in EPI_CASES:
        layer = _make(cls, kw, prec, seed=7, bt_seed=1234)
        nout = kw.get("out_channels", kw.get("out_features"))
        is_stem = kw.get("in_channels", 99) <= 4
        g = torch.Generator().manual_seed(17)
        x = (torch.randn(*xs, generator=g) * 2).to(_dev()).to(act)
        scale = (torch.rand(nout, generator=g) * 4 + 2).to(_dev())
        shift = torch.randn(nout, generator=g).to(_dev())
        with torch.no_grad():
            plain = layer._forward_hip(x, sample_idx=5, gather=gather)
        pre, A, Ab, K = _refs(layer, x, plain.shape, 5)
        shp = (1, -1) + (1,) * (pre.dim() - 2)
        s64, t64 = E.d64(scale).view(shp), E.d64(shift).view(shp)
        res = None if is_stem else (torch.randn(plain.shape, generator=g) * 4).to(_dev()).to(act)
        for code in (0, 1, 2):
            with torch.no_grad():
                got = layer._forward_hip(x, sample_idx=5, gather=gather,
                                         epilogue=dict(scale=scale, shift=shift, residual=res, relu=code))
            val = pre * s64 + t64
            b = E.through_affine(E.bound(A, prec, K, A_bias=Ab), pre, scale, shift, channel_axis=1)
            if res is not None:
                val = val + E.d64(res)
                b = b + E.REF32_UNIT * (val.abs().numpy() + b)  # one f32 add
            ref = val if code == 0 else (val.clamp_min(0) if code == 1 else val.clamp(0, 6))
            if act == torch.bfloat16:
                b = E.store_rounding(b, val)
            log.check("epilogue relu=%d%s %s" % (code, "+res" if res is not None else "", _tag(cls, kw, xs)), prec, got, ref, b)
    log.done()


# ---- backward: dx everywhere, dW / db on the small cases ------------------------------------------------------------------
@pytest.mark.parametrize("cls,kw,xshape", BWD_CASES, ids=[_tag(*c) for c in BWD_CASES])
def test_small_case_gradients_every_element(cls, kw, xshape):
    """CASES of test_gpu_backward.py, f32 parity mode: dx, dmu, drho, dmu_b, drho_b element by element against float64 autograd
    through the reference chain on the CPU.  K of the weight gradients is the pixel count (small here)."""
    import bayesian_torch_amd as bt
    bt.set_precision("f32")
    layer = _make(cls, kw, None, seed=0, bt_seed=123)
    torch.manual_seed(1)
    x = torch.randn(*xshape, device=_dev(), requires_grad=True)
    bt.set_sample_index(layer, 5)
    out = layer(x, return_kl=False)
    gy = torch.randn_like(out)
    out.backward(gy)
    mu, rho = layer._w()
    op = _op_of(layer)
    flip = layer._family == "flipout"
    dx64, dmu64, A_dx, dd64, nz = _grads64(layer, x.detach(), gy, 5)
    w_shape = tuple(mu.shape)
    log = _Log()
    log.check("dx " + _tag(cls, kw, xshape), "f32", x.grad, dx64, E.bound(A_dx, "f32", E.dgrad_reduction_length(w_shape, op)))
    A_w = E.wgrad_A(x.detach(), gy, w_shape, op)
    Kw = E.wgrad_reduction_length(tuple(out.shape), op)
    b_w = E.bound(A_w, "f32", Kw, delta_w=0.0)
    sig = torch.sigmoid(E.d64(rho)) * E.d64(nz["eps_w"])
    if flip:
        log.check("dmu " + _tag(cls, kw, xshape), "f32", mu.grad, dmu64, b_w)
        log.check("drho " + _tag(cls, kw, xshape), "f32", rho.grad, dd64 * sig, _scaled(b_w, dd64, sig))
    else:  # mu and delta enter as one weight: dW = dmu = ddelta
        log.check("dmu " + _tag(cls, kw, xshape), "f32", mu.grad, dmu64, b_w)
        log.check("drho " + _tag(cls, kw, xshape), "f32", rho.grad, dmu64 * sig, _scaled(b_w, dmu64, sig))
    if layer.mu_bias is not None:
        red = tuple(i for i in range(gy.dim()) if i != (gy.dim() - 1 if op["kind"] == "linear" else 1))
        gy64 = E.d64(gy)
        db64, A_b = gy64.sum(red), gy64.abs().sum(red)
        b_b = E.bound(A_b, "f32", Kw, delta_w=0.0)
        log.check("dmu_b " + _tag(cls, kw, xshape), "f32", layer.mu_bias.grad, db64, b_b)
        dbd64 = (gy64 * E.d64(nz["sign_out"].reshape(gy.shape))).sum(red) if flip else db64
        sig_b = torch.sigmoid(E.d64(layer.rho_bias)) * E.d64(nz["eps_b"])
        log.check("drho_b " + _tag(cls, kw, xshape), "f32", layer.rho_bias.grad, dbd64 * sig_b, _scaled(b_b, dbd64, sig_b))
    log.done()


@pytest.mark.parametrize("case", CPU_BWD_CASES, ids=[c[0] for c in CPU_BWD_CASES])
def test_data_gradient_at_baseline_batch_every_element(case):
    """CPU_BWD_CASES: dx at the baseline batch, f32 (the weight gradients there have K = 12 544 .. 200 704 pixels: the envelope is
    vacuous, the exact-integer runs below cover them)"""
    import bayesian_torch_amd as bt
    name, cls, kw, xshape = case
    bt.set_precision("f32")
    layer = _make(cls, kw, None)
    torch.manual_seed(1234)
    x = torch.randn(*xshape, device=_dev())
    if len(xshape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    bt.set_sample_index(layer, 9)
    out = layer(x, return_kl=False)
    torch.manual_seed(5)
    dy = torch.randn(out.shape, device=_dev())
    out.backward(dy)
    dx64, _, A, _, _ = _grads64(layer, x.detach(), dy, 9, weights=False)
    log = _Log()
    log.check("dx %s batch %d" % (name, xshape[0]), "f32", x.grad, dx64,
              E.bound(A, "f32", E.dgrad_reduction_length(tuple(layer._w()[0].shape), _op_of(layer))))
    log.done()


# =============================================================================================================================
# 2. exact-integer runs: zero tolerance
# =============================================================================================================================
def _wgrad_like_autograd(layer, x, dy, sample, bias):
    """BF.wgrad_hip(..., raw=False) without rho_flat, on the geometry ContractFn.backward takes for this layer"""
    from bayesian_torch_amd import _lib, functional as BF
    from bayesian_torch_amd import rng as _rng
    op = layer._op
    kind = _lib.KIND_FLIPOUT if layer._family == "flipout" else _lib.KIND_REPARAM
    w_shape = tuple(layer._w()[0].shape)
    plan = layer._rowfuse_plan(x) if op.nd == 2 else None
    if plan is not None:
        return BF.wgrad_hip(kind, x, dy, op, _rng.seed(), sample, layer._btx_layer_id, w_shape, bias=bias, rowfuse=plan)
    signs = None
    if layer._btx_cpad is not None and kind == _lib.KIND_FLIPOUT:
        nz = layer.materialize_noise(sample, tuple(x.shape), tuple(dy.shape), x.dtype, signs=True)
        signs = (nz["sign_in"], nz["sign_out"])
    return BF.wgrad_hip(kind, x, dy, op, _rng.seed(), sample, layer._btx_layer_id, w_shape, signs=signs, bias=bias)


def _exact_wgrad(log, name, cls, kw, xshape, acts=(torch.float32, torch.bfloat16)):
    from bayesian_torch_amd import functional as BF
    layer = _make(cls, kw, None)
    op = _op_of(layer)
    flip = layer._family == "flipout"
    x0 = E.small_ints(xshape, 31)
    with torch.no_grad():
        oshape = tuple(E.contract(torch.zeros((1,) + tuple(xshape[1:])), layer._w()[0].detach().float().cpu(), None, op).shape)
    oshape = (xshape[0],) + oshape[1:]
    dy0 = E.small_ints(oshape, 32)
    w_shape = tuple(layer._w()[0].shape)
    want = None
    try:
        for act in acts:
            x, dy = x0.to(_dev()).to(act), dy0.to(_dev()).to(act)
            if len(xshape) == 4:
                x, dy = x.contiguous(memory_format=torch.channels_last), dy.contiguous(memory_format=torch.channels_last)
            if want is None:  # one float64 reference for both activation types and both accumulation paths
                nz = layer.materialize_noise(4, tuple(x.shape), oshape, x.dtype, signs=True)
                red = tuple(i for i in range(len(oshape)) if i != (len(oshape) - 1 if op["kind"] == "linear" else 1))
                want = [E.wgrad64(x0, dy0, w_shape, op), None, E.d64(dy0).sum(red), None]
                if flip:
                    si, so = E.d64(nz["sign_in"].reshape(x.shape)), E.d64(nz["sign_out"].reshape(oshape))
                    want[1] = E.wgrad64(E.d64(x0) * si, E.d64(dy0) * so, w_shape, op)
                    want[3] = (E.d64(dy0) * so).sum(red)
                assert float(want[0].abs().max()) < 2 ** 24
            for atomics in (False, True):
                BF.WGRAD_ATOMICS = atomics
                got = _wgrad_like_autograd(layer, x, dy, 4, bias=True)
                for g_, w_, nm in zip(got, want, ("dW_mu", "dW_delta", "db_mu", "db_delta")):
                    assert (g_ is None) == (w_ is None), nm
                    if w_ is not None:
                        rep = E.check_exact(g_, w_)
                        print(rep.line("exact %s %s %s" % (nm, name, "atomics" if atomics else "slabs"),
                                       "bf16" if act == torch.bfloat16 else "f32"))
                        if not rep.ok:
                            log.bad.append("%s %s %s %s: %s" % (nm, name, act, "atomics" if atomics else "slabs", rep))
    finally:
        BF.WGRAD_ATOMICS = False


@pytest.mark.parametrize("case", CPU_BWD_CASES, ids=[c[0] for c in CPU_BWD_CASES])
def test_integer_weight_gradient_is_exact_at_baseline_batch(case):
    name, cls, kw, xshape = case
    log = _Log()
    _exact_wgrad(log, "%s batch %d" % (name, xshape[0]), cls, kw, xshape)
    log.done()


@pytest.mark.parametrize("shape", RN18_SHAPES, ids=["%d-%d-%d-s%d-k%d" % s for s in RN18_SHAPES])
def test_integer_weight_gradient_is_exact_on_every_resnet18_layer_shape(shape):
    """the shapes of test_backward_at_baseline_size_every_resnet18_layer_shape at batch 64 — the all-taps kernel (3x3 / stride 1),
    the row-fused stem form, strided and pointwise layers; chunk slabs and f32 atomics; f32 and bf16 activations: every pixel
    chunk is counted exactly once, and the bias gradients (f32 atomics in either path) have exactly the right value"""
    cin, cout, hw, stride, k = shape
    log = _Log()
    _exact_wgrad(log, "rn18 %d->%d %d^2 s%d k%d" % shape, "Conv2dFlipout",
                 dict(in_channels=cin, out_channels=cout, kernel_size=k, stride=stride, padding=k // 2, bias=True), (64, cin, hw, hw))
    log.done()


SMALL_EXACT = [BWD_CASES[i] for i in (0, 2, 3, 5, 6, 8, 16, 17, 18)]  # linear, padded, grouped + dilated, strided, stems


@pytest.mark.parametrize("cls,kw,xshape", SMALL_EXACT, ids=[_tag(*c) for c in SMALL_EXACT])
def test_integer_weight_gradient_is_exact_on_small_cases(cls, kw, xshape):
    log = _Log()
    _exact_wgrad(log, _tag(cls, kw, xshape), cls, dict(kw, bias=True), xshape)
    log.done()


def _sigma_zero_dyadic(layer):
    """rho = -200: exp underflows and both softplus forms return exactly 0; mu = m 2^-7, |m| <= 128 (exact in bf16)"""
    mu, rho = layer._w()
    with torch.no_grad():
        mu.copy_(E.dyadic(tuple(mu.shape), 41).to(mu.device))
        rho.fill_(-200.0)
        if layer.mu_bias is not None:
            layer.mu_bias.copy_(E.dyadic(tuple(layer.mu_bias.shape), 42).to(mu.device))
            layer.rho_bias.fill_(-200.0)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_deterministic_half_of_the_forward_is_exact(case, prec):
    """sigma = 0 exactly, dyadic mu, integer x: the float64 convolution bit for bit, in all three precisions, single launch and
    lane 1 of a 2-lane launch (bf16 activations: its one rounding on store)"""
    import bayesian_torch_amd as bt
    name, cls, kw, xshape = case
    layer = _make(cls, kw, prec)
    _sigma_zero_dyadic(layer)
    act = torch.bfloat16 if prec == "bf16" else torch.float32
    x = E.small_ints(xshape, 43).to(_dev()).to(act)
    if len(xshape) == 4:
        x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=9)
        shared = kw.get("in_channels") == 3
        bt.set_sample_lanes(layer, [8, 9], batch=xshape[0])
        out2 = layer._forward_hip(x if shared else torch.cat([x, x], 0))[xshape[0]:]
        bt.set_sample_lanes(layer, None)
    torch.cuda.synchronize()

    def make():
        with torch.no_grad():
            return E.contract(E.d64(x), E.d64(layer._w()[0]), E.d64(layer.mu_bias), _op_of(layer))
    ref = _cached_refs(("exact", name), make)
    assert float(ref.abs().max()) * 128 < 2 ** 24
    if prec == "bf16":
        ref = ref.to(torch.bfloat16)
    log = _Log()
    for got, form in ((out, "single"), (out2, "lane1of2")):
        rep = E.check_exact(got, ref)
        print(rep.line("exact fwd %s %s" % (name, form), prec))
        if not rep.ok:
            log.bad.append("%s %s %s: %s" % (name, prec, form, rep))
    log.done()


@pytest.mark.parametrize("case", CPU_BWD_CASES, ids=[c[0] for c in CPU_BWD_CASES])
@pytest.mark.parametrize("prec,act", [("f32", torch.float32), ("bf16", torch.bfloat16)], ids=["f32", "bf16"])
def test_deterministic_half_of_the_data_gradient_is_exact(case, prec, act):
    import bayesian_torch_amd as bt
    name, cls, kw, xshape = case
    bt.set_precision(prec)
    try:
        layer = _make(cls, kw, None)
        _sigma_zero_dyadic(layer)
        x = E.small_ints(xshape, 44).to(_dev()).to(act)
        if len(xshape) == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        bt.set_sample_index(layer, 9)
        out = layer(x, return_kl=False)
        dy = E.small_ints(tuple(out.shape), 45).to(_dev()).to(act)
        out.backward(dy)
        x64 = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
        (ref,) = torch.autograd.grad(E.contract(x64, E.d64(layer._w()[0]), None, _op_of(layer)), x64, E.d64(dy))
        if act == torch.bfloat16:
            ref = ref.to(torch.bfloat16)
        rep = E.check_exact(x.grad, ref)
        print(rep.line("exact dx %s" % name, prec))
        assert rep.ok, str(rep)
    finally:
        bt.set_precision("f32")


@pytest.mark.parametrize("shape,dtype,k,s,p", _params_of(_maxpool_test))
def test_integer_maxpool_forward_and_backward_equal_torch_on_the_cpu(shape, dtype, k, s, p):
    """integers in [-3, 3]: most windows tie, so the gradient's first-maximum rule decides nearly every element; sums of up to
    (k/s)^2 small integers are exact in bf16"""
    from bayesian_torch_amd import functional as BF
    x = E.small_ints(shape, 51).to(dtype).contiguous(memory_format=torch.channels_last)
    xc = x.double().requires_grad_(True)
    yc = torch.nn.functional.max_pool2d(xc, k, s, p)
    dy = E.small_ints(tuple(yc.shape), 52).to(dtype).contiguous(memory_format=torch.channels_last)
    yc.backward(dy.double())
    xg, dyg = x.to(_dev()), dy.to(_dev())
    y, idx = BF.maxpool2d_train_hip(xg, k, s, p)
    dx = BF.maxpool2d_bwd_hip(dyg, idx, tuple(shape), k, s, p)
    torch.cuda.synchronize()
    for nm, got, ref in (("maxpool fwd", y, yc.detach()), ("maxpool bwd", dx, xc.grad)):
        rep = E.check_exact(got, ref)
        print(rep.line("%s %s k%d s%d p%d" % (nm, "x".join(map(str, shape)), k, s, p), str(dtype).split(".")[-1]))
        assert rep.ok, str(rep)
    if shape[1] % 8 == 0:
        assert E.check_exact(BF.maxpool2d_hip(xg, k, s, p), yc.detach()).ok
