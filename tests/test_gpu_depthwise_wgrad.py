"""The weight gradient of the depthwise family (BTX-DW v1) against float64 at the materialised signs, with the
envelope tests/test_gpu_elementwise.py uses for the generic kernel (K = pixels); exact integers, repeats, poison, layers eager and captured."""
import pytest
import torch

import envelope as E
import poison
from bayesian_torch_amd import _lib
from autograd_cases import dev as _dev, make as _make, Log as _Log, grads64 as _grads64, scaled as _scaled
from test_depthwise_plan import GEOMS as _G
from test_depthwise_wgrad_plan import MULTI
from test_gpu_backward import _op_of
from test_gpu_depthwise import _kw, _x, KINDS

GEOMS = _G + MULTI  # 8, 9: slabs of several tiles, ragged last slab
IDS = ["C%d-k%d-s%d-p%d-d%d" % g[:5] for g in GEOMS]

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

ACTS, SAMPLE = [("f32", torch.float32), ("bf16", torch.bfloat16)], 5


def _wgrad(layer, x, dy, flags=0, rho=False, swap=False):
    """(dw_mu, dw_delta | None, drho | None) in the logical weight shape, by BF.wgrad_hip as ContractFn.backward calls it"""
    from bayesian_torch_amd import functional as BF, rng as _rng
    op, w_shape = layer._op, tuple(layer._w()[0].shape)
    kind = _lib.KIND_FLIPOUT if layer._family == "flipout" else _lib.KIND_REPARAM
    rho_f = BF.gemm_major_view(layer._w()[1].detach(), op).reshape(-1).contiguous() if rho else None
    res = BF.wgrad_hip(kind, x, dy, op, _rng.seed(), SAMPLE, layer._btx_layer_id, w_shape, raw=True, rho_flat=rho_f, swap=swap, _flags=flags)
    un = lambda t: None if t is None else BF.gemm_major_logical_view(t, w_shape, op)  # noqa: E731
    return un(res[0]), (None if rho else un(res[1])), (un(res[4]) if rho else None)


def _signs(layer, shape, stream):
    """the hashed +/-1 signs of `stream` at the channels-last linear indices of a tensor of logical `shape`, float64 on the CPU"""
    from bayesian_torch_amd import functional as BF, rng as _rng
    s = BF.fill_sign_hip(torch.Size(shape).numel(), _dev(), _rng.seed(), SAMPLE, layer._btx_layer_id, stream)
    return E.d64(s.reshape(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2))


def _case(gi, cls, act, ints=False):
    geo = GEOMS[gi]
    layer = _make(cls, _kw(geo, bias=False), "bf16" if act == torch.bfloat16 else "f32", seed=7, bt_seed=1234)
    with torch.no_grad():
        oshape = tuple(E.contract(torch.zeros(geo[5]), layer._w()[0].detach().float().cpu(), None, _op_of(layer)).shape)
    if ints:
        cl = lambda t: t.to(_dev()).to(act).contiguous(memory_format=torch.channels_last)  # noqa: E731
        return layer, cl(E.small_ints(geo[5], 31)), cl(E.small_ints(oshape, 32))
    return layer, _x(geo[5], act, seed=21), _x(oshape, act, seed=22, scale=1.0)


@pytest.mark.parametrize("prec,act", ACTS, ids=[p for p, _ in ACTS])
@pytest.mark.parametrize("cls", KINDS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=IDS)
def test_weight_gradient_every_element_inside_the_envelope(gi, cls, prec, act):
    """the stencil route and the BTX_FLAG_GATHER route; inputs rounded to the activation dtype, accumulation in f32 on both"""
    layer, x, dy = _case(gi, cls, act)
    op, w_shape, flip = _op_of(layer), tuple(layer._w()[0].shape), layer._family == "flipout"
    nz = layer.materialize_noise(SAMPLE, tuple(x.shape), tuple(dy.shape), x.dtype, signs=True)
    want_m = want_d = E.wgrad64(x, dy, w_shape, op)
    if flip:
        want_d = E.wgrad64(E.d64(x) * E.d64(nz["sign_in"].reshape(x.shape)), E.d64(dy) * E.d64(nz["sign_out"].reshape(dy.shape)), w_shape, op)
    b = E.bound(E.wgrad_A(x, dy, w_shape, op), "f32", E.wgrad_reduction_length(tuple(dy.shape), op), delta_w=0.0)
    sig = torch.sigmoid(E.d64(layer._w()[1])) * E.d64(nz["eps_w"])
    log, seen = _Log(), []
    for route, flags in (("stencil", 0), ("gather", _lib.FLAG_GATHER)):
        tag = "dw wgrad %s %s %s" % (route, IDS[gi], cls)
        dwm, dwd, _ = _wgrad(layer, x, dy, flags)
        seen.append(dwm)
        log.check(tag + " dw_mu", prec, dwm, want_m, b)
        if flip:
            log.check(tag + " dw_delta", prec, dwd, want_d, b)
        log.check(tag + " drho", prec, _wgrad(layer, x, dy, flags, rho=True)[2], want_d * sig, _scaled(b, want_d, sig))
    log.done()
    if gi >= 7:  # thousands of pixels added in another order: equal bits would mean that flags = 0 did not land on the stencil kernel
        assert not poison.bits_equal(seen[0], seen[1])


@pytest.mark.parametrize("swap", [False, True], ids=["plain", "swap-signs"])
@pytest.mark.parametrize("prec,act", ACTS, ids=[p for p, _ in ACTS])
@pytest.mark.parametrize("gi", [0, 1, 4, 7, 8, 9], ids=[IDS[i] for i in (0, 1, 4, 7, 8, 9)])
def test_small_integers_give_the_float64_sums_bit_for_bit(gi, prec, act, swap):
    """a tile or slab counted twice or not at all shows as a whole number; swap: x carries the output stream, dy the input stream"""
    layer, x, dy = _case(gi, "Conv2dFlipout", act, ints=True)
    op, w_shape = _op_of(layer), tuple(layer._w()[0].shape)
    sx = _signs(layer, tuple(x.shape), _lib.STREAM_SIGN_OUT if swap else _lib.STREAM_SIGN_IN)
    sy = _signs(layer, tuple(dy.shape), _lib.STREAM_SIGN_IN if swap else _lib.STREAM_SIGN_OUT)
    want = [E.wgrad64(x, dy, w_shape, op), E.wgrad64(E.d64(x) * sx, E.d64(dy) * sy, w_shape, op)]
    assert float(E.wgrad_A(x, dy, w_shape, op).max()) < 2 ** 24
    got = _wgrad(layer, x, dy, swap=swap)
    for g_, w_, nm in zip(got, want, ("dw_mu", "dw_delta")):
        assert E.check_exact(g_, w_).ok, "%s %s %s: %s" % (nm, IDS[gi], prec, E.check_exact(g_, w_))
    runs = [_wgrad(layer, x, dy, swap=swap, rho=r) for r in (False, True)]
    for byte in poison.PATTERNS:
        with poison.poisoned(byte):
            runs += [_wgrad(layer, x, dy, swap=swap, rho=r) for r in (False, True)]
    assert poison.bits_equal(runs[0][0], got[0]) and poison.bits_equal(runs[0][1], got[1])  # the second call
    for i in range(2, len(runs)):  # poisoned runs against the plain run of the same form (without | with the fused drho)
        assert all(poison.bits_equal(a, b_) for a, b_ in zip(runs[i], runs[i % 2]) if a is not None), i


@pytest.mark.parametrize("cls,kw,xshape", [("Conv2dFlipout", _kw(GEOMS[0], False), GEOMS[0][5]), (
    "ConvTranspose2dReparameterization", dict(in_channels=64, out_channels=64, kernel_size=3, stride=2, padding=1, groups=64), (2, 64, 7, 9))])
def test_layers_train_on_the_kernel_eagerly_and_captured(cls, kw, xshape):
    """eager dmu / drho against float64 autograd; a captured SGD step replayed twice == two eager steps, bit for bit (device sample word)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim, layers as L
    from bayesian_torch_amd.autograd import GraphedTrainStep
    bt.set_precision("f32")
    layer = _make(cls, dict(kw, bias=False), None, seed=0, bt_seed=123)
    x = _x(xshape, torch.float32, seed=1, scale=1.0)
    bt.set_sample_index(layer, SAMPLE)
    out = layer(x, return_kl=False)
    dy = _x(tuple(out.shape), torch.float32, seed=2, scale=1.0)
    out.backward(dy)
    mu, rho = layer._w()
    _, dmu64, _, dd64, nz = _grads64(layer, x, dy, SAMPLE)
    op, w_shape = _op_of(layer), tuple(mu.shape)
    px = tuple(x.shape) if op["kind"] == "convT" else tuple(out.shape)  # the pixels the sum runs over: the smaller map of a transposed layer
    b = E.bound(E.wgrad_A(x, dy, w_shape, op), "f32", E.wgrad_reduction_length(px, op), delta_w=0.0)
    sig = torch.sigmoid(E.d64(rho)) * E.d64(nz["eps_w"])
    dd64 = dd64 if layer._family == "flipout" else dmu64
    log = _Log()
    log.check("dmu " + cls, "f32", mu.grad, dmu64, b)
    log.check("drho " + cls, "f32", rho.grad, dd64 * sig, _scaled(b, dd64, sig))
    log.done()
    feats = out[0].numel()
    del out  # GraphedTrainStep: no live autograd graph of an earlier eager step of the model (its AccumulateGrad nodes pin a stream)
    net = torch.nn.Sequential(layer, torch.nn.Flatten(), L.LinearReparameterization(feats, 10).to(_dev())).train()
    net[0].dnn_to_bnn_flag = net[2].dnn_to_bnn_flag = True
    bt.assign_layer_ids(net)
    y = torch.randint(0, 10, (xshape[0],), device=_dev())
    params = list(net.parameters())
    start = [p.detach().clone() for p in params]
    opt = optim.SGD(params, lr=0.05)
    for s in (3, 4):
        net.zero_grad(set_to_none=True)
        bt.set_sample_index(net, s, presample=True)
        (torch.nn.functional.cross_entropy(net(x).float(), y) + bt.get_kl_loss(net) / x.shape[0]).backward()
        opt.step()
    eager = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, s0 in zip(params, start):
            p.copy_(s0)
    gs = GraphedTrainStep(net, x, y, optimizer=optim.SGD(params, lr=0.05))
    try:
        for s in (3, 4):
            gs.run(s)
        torch.cuda.synchronize()
        assert not torch.equal(params[0].detach(), start[0]) and all(torch.equal(p.detach(), e) for p, e in zip(params, eager))
    finally:
        gs.close()
