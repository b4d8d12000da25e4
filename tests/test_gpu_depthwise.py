"""The depthwise family (BTX-DW v1) against float64 at the materialised noise: every element of the forward and of
the data gradient inside the envelopes of tests/envelope.py with K = taps, lanes bit-equal to single launches, the deterministic
half exact, and no dependence on what the output buffer held."""
import types
import warnings

import pytest
import torch

import envelope as E
import poison
from autograd_cases import dev as _dev, make as _make, Log as _Log, grads64 as _grads64
from test_depthwise_plan import GEOMS
from test_gpu_backward import _op_of
from test_gpu_fuse_model import _plan

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

PRECS = [("f32", torch.float32), ("bf16x3", torch.float32), ("bf16", torch.bfloat16)]
KINDS = ["Conv2dReparameterization", "Conv2dFlipout"]
IDS = ["C%d-k%d-s%d-p%d-d%d" % g[:5] for g in GEOMS]


def _kw(geo, bias=True):
    C, k, s, p, d, _ = geo
    return dict(in_channels=C, out_channels=C, kernel_size=k, stride=s, padding=p, dilation=d, groups=C, bias=bias)


def _x(xshape, act, seed=17, scale=2.0):
    x = (torch.randn(*xshape, generator=torch.Generator().manual_seed(seed)) * scale).to(_dev()).to(act)
    return x.contiguous(memory_format=torch.channels_last)


def _refs(layer, x, out_shape, sample):
    with torch.no_grad():
        nz = layer.materialize_noise(sample, tuple(x.shape), tuple(out_shape), x.dtype)
        mu, rho = layer._w()
        flip = layer._family == "flipout"
        si = nz["sign_in"].reshape(x.shape) if flip else None
        so = nz["sign_out"].reshape(out_shape) if flip else None
        ref, A, Ab = E.reference_forward(x, mu, rho, nz["eps_w"], layer.mu_bias, layer.rho_bias, nz.get("eps_b"), si, so, _op_of(layer))
    return ref, A, Ab


@pytest.mark.parametrize("prec,act", PRECS, ids=[p for p, _ in PRECS])
@pytest.mark.parametrize("cls", KINDS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_forward_every_element_inside_the_envelope(gi, cls, prec, act):
    """all geometries x kinds x precisions; on geometries 0 and 1 also bias + scale / shift + residual + ReLU6"""
    geo = GEOMS[gi]
    layer = _make(cls, _kw(geo), prec, seed=7, bt_seed=1234)
    with torch.no_grad():
        layer.mu_bias.normal_()
    x = _x(geo[5], act)
    T = geo[1] * geo[1]
    assert _plan(layer, geo[5], prec)[:2] == (0, "depthwise")
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=5)
    ref, A, Ab = _refs(layer, x, out.shape, 5)
    log = _Log()
    log.check("dw fwd %s %s" % (IDS[gi], cls), prec, out, ref, E.bound(A, prec, T, ref=ref, A_bias=Ab, store_bf16=(act == torch.bfloat16)))
    if gi < 2:
        g = torch.Generator().manual_seed(19)
        scale, shift = (torch.rand(geo[0], generator=g) * 4 + 2).to(_dev()), torch.randn(geo[0], generator=g).to(_dev())
        res = (torch.randn(out.shape, generator=g) * 4).to(_dev()).to(act).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            got = layer._forward_hip(x, sample_idx=5, epilogue=dict(scale=scale, shift=shift, residual=res, relu=2))
        val = ref * E.d64(scale).view(1, -1, 1, 1) + E.d64(shift).view(1, -1, 1, 1) + E.d64(res)
        b = E.through_affine(E.bound(A, prec, T, A_bias=Ab), ref, scale, shift, channel_axis=1)
        b = b + E.REF32_UNIT * (val.abs().numpy() + b)  # the residual: one f32 add
        if act == torch.bfloat16:
            b = E.store_rounding(b, val)
        log.check("dw fwd+epilogue %s %s" % (IDS[gi], cls), prec, got, val.clamp(0, 6), b)
    log.done()


@pytest.mark.parametrize("shared", [True, False], ids=["shared-x", "per-lane-x"])
@pytest.mark.parametrize("cls", KINDS)
def test_three_lanes_equal_three_single_launches_bit_for_bit(cls, shared):
    import bayesian_torch_amd as bt
    geo, idx = GEOMS[0], [5, 11, 12]
    layer = _make(cls, _kw(geo), "bf16")
    xs = [_x(geo[5], torch.bfloat16, seed=30 + (0 if shared else l)) for l in range(3)]
    assert _plan(layer, geo[5], "bf16", lanes=3)[:2] == (0, "depthwise")
    with torch.no_grad():
        singles = [layer._forward_hip(xs[l], sample_idx=idx[l]) for l in range(3)]
        bt.set_sample_lanes(layer, idx, batch=geo[5][0])
        lanes = layer._forward_hip(xs[0] if shared else torch.cat(xs, 0))
        bt.set_sample_lanes(layer, None)
    assert poison.bits_equal(lanes, torch.cat(singles, 0))


@pytest.mark.parametrize("prec,act", PRECS, ids=[p for p, _ in PRECS])
@pytest.mark.parametrize("gi", [0, 1, 4, 5], ids=[IDS[i] for i in (0, 1, 4, 5)])
def test_deterministic_half_is_exact(gi, prec, act):
    """rho = -200 (sigma == 0 exactly), dyadic mu, small-integer x: the float64 convolution bit for bit"""
    geo = GEOMS[gi]
    log = _Log()
    for cls in KINDS:
        layer = _make(cls, _kw(geo), prec)
        mu, rho = layer._w()
        with torch.no_grad():
            mu.copy_(E.dyadic(tuple(mu.shape), 41).to(mu.device))
            rho.fill_(-200.0)
            layer.mu_bias.copy_(E.dyadic(tuple(layer.mu_bias.shape), 42).to(mu.device))
            layer.rho_bias.fill_(-200.0)
            x = E.small_ints(geo[5], 43).to(_dev()).to(act).contiguous(memory_format=torch.channels_last)
            out = layer._forward_hip(x, sample_idx=9)
            ref = E.contract(E.d64(x), E.d64(mu), E.d64(layer.mu_bias), _op_of(layer))
        rep = E.check_exact(out, ref.to(act))
        print(rep.line("dw exact %s %s" % (IDS[gi], cls), prec))
        if not rep.ok:
            log.bad.append("%s %s %s: %s" % (IDS[gi], cls, prec, rep))
    log.done()


@pytest.mark.parametrize("cls", KINDS)
@pytest.mark.parametrize("gi", [0, 1, 4, 5], ids=[IDS[i] for i in (0, 1, 4, 5)])
def test_data_gradient_every_element_inside_the_envelope(gi, cls):
    """dx of an eager training step (geometries 1 and 4 are stride 2) against float64 autograd of the composite at the same noise;
    the transposed launch that computes it plans on the depthwise family"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    geo = GEOMS[gi]
    bt.set_precision("f32")
    layer = _make(cls, _kw(geo, bias=False), None, seed=0, bt_seed=123)
    x = _x(geo[5], torch.float32, seed=1, scale=1.0).requires_grad_(True)
    bt.set_sample_index(layer, 5)
    out = layer(x, return_kl=False)
    dy = _x(tuple(out.shape), torch.float32, seed=2, scale=1.0)
    out.backward(dy)
    op = layer._op
    outpad = tuple((i + 2 * p - d * (k - 1) - 1) % s for i, p, d, k, s in
                   zip(geo[5][2:], op.padding[1:], op.dilation[1:], op.kernel[1:], op.stride[1:]))
    opT = BF.OpDesc(2, op.out_channels, op.in_channels, op.kernel[1:], op.stride[1:], op.padding[1:], op.dilation[1:], op.groups,
                    transposed=True, output_padding=outpad)
    assert _plan(types.SimpleNamespace(_op=opT, _family=layer._family, _btx_cpad=None), tuple(dy.shape), "f32")[:2] == (0, "depthwise")
    dx64, _, A, _, _ = _grads64(layer, x.detach(), dy, 5, weights=False)
    log = _Log()
    log.check("dw dx %s %s" % (IDS[gi], cls), "f32", x.grad, dx64,
              E.bound(A, "f32", E.dgrad_reduction_length(tuple(layer._w()[0].shape), _op_of(layer))))
    log.done()


@pytest.mark.parametrize("byte", [0xFF, 0x7F])
def test_output_does_not_depend_on_what_the_buffer_held(byte):
    geo = GEOMS[0]
    layer = _make("Conv2dFlipout", _kw(geo), "bf16")
    x = _x(geo[5], torch.bfloat16)
    with torch.no_grad():
        plain = layer._forward_hip(x, sample_idx=3)
        with poison.poisoned(byte):
            got = layer._forward_hip(x, sample_idx=3)
    assert poison.bits_equal(got, plain)
