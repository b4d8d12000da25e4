"""ReLU6 in the store of every kernel family (BtxEpilogue.relu = 2), and models.fuse.fuse_model on the GPU."""
import ctypes

import pytest
import torch

from test_fuse_model import MODELS, make

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _plan(layer, xshape, prec, lanes=1, gather=False, ep=None):
    """(rc, family) of btx_contract_plan_info for the launch layer._forward_hip makes on a (per-lane) input of shape xshape"""
    from bayesian_torch_amd import _lib, functional as BF
    op, flags = layer._op, 0
    g = _lib.Geom()
    act = _lib.ACT_BF16 if prec == "bf16" else _lib.ACT_F32
    rf = BF.rowfuse_plan(op, xshape) if op.nd == 2 else None
    if rf is not None:
        op, spatial, flags = rf["op"], (1, rf["Hp"], rf["Wp"]), _lib.FLAG_ROWFUSE
    else:
        if layer._btx_cpad is not None:
            op = layer._op_pad
        spatial = (1, 1, 1) if op.nd == 0 else (1,) * (3 - op.nd) + tuple(xshape[2:])
    g.NB, (g.D, g.H, g.W), g.C, g.N = xshape[0], spatial, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.od, g.oh, g.ow = op.output_padding
    g.groups = op.groups
    if gather:
        flags |= _lib.FLAG_GATHER
    if lanes > 1:
        flags |= lanes << _lib.FLAG_LANES_SHIFT
    info = _lib.PlanInfo()
    kind = _lib.KIND_FLIPOUT if layer._family == "flipout" else _lib.KIND_REPARAM
    rc = _lib.lib().btx_contract_plan_info(kind, ctypes.byref(g), act, _lib.PREC_CODE[prec], flags,
                                           ctypes.byref(ep) if ep is not None else None, ctypes.byref(info))
    return rc, (_lib.FAMILIES[info.family] if rc == 0 else None), info.ksplits


# (layer class, kwargs, per-lane input, gather flag): together they reach every store path at lanes 1 (checked below)
CASES = [
    ("Conv2dFlipout", dict(in_channels=6, out_channels=10, kernel_size=3, padding=1), (2, 6, 9, 9), True),           # gather
    ("Conv2dFlipout", dict(in_channels=32, out_channels=32, kernel_size=3, padding=1, groups=32), (2, 32, 16, 16), False),  # depthwise
    ("Conv2dReparameterization", dict(in_channels=24, out_channels=40, kernel_size=3, padding=1), (2, 24, 10, 10), False),  # regstage
    ("LinearFlipout", dict(in_features=64, out_features=64), (16, 64), False),                                             # Linear
    ("LinearFlipout", dict(in_features=256, out_features=96), (16, 256), False),                                           # split-K
    ("Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=1, bias=False), (4, 64, 56, 56), False),           # dma
    ("Conv2dFlipout", dict(in_channels=256, out_channels=256, kernel_size=1, bias=False), (32, 256, 14, 14), False),       # gemm8
    ("Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=5, padding=2), (2, 64, 12, 12), False),            # patch
    ("Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=3, padding=1), (8, 64, 56, 56), False),            # taps
    ("Conv2dFlipout", dict(in_channels=64, out_channels=128, kernel_size=3, stride=2, padding=1), (8, 64, 56, 56), False),  # taps2
    ("Conv2dFlipout", dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), (2, 3, 64, 64), False),  # stem
]
PRECS = [("f32", torch.float32), ("bf16x3", torch.float32), ("bf16", torch.bfloat16)]


def _layer(cls, kw, prec):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(1234)
    torch.manual_seed(7)
    layer = getattr(L, cls)(**kw).to(_dev())
    layer.precision = prec
    return layer


def test_cases_reach_every_family():
    families = set()
    for cls, kw, xs, gather in CASES:
        for prec, _ in PRECS:
            rc, fam, ks = _plan(_layer(cls, kw, prec), xs, prec, gather=gather)
            assert rc == 0
            families.add(fam)
            if kw.get("in_features") == 256:  # the split-K case: its store is the reduce kernel's (splitk_reduce_kernel)
                assert ks > 1, (prec, fam, ks)
    assert {"gather", "regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem"} <= families, families


@pytest.mark.parametrize("prec,act", PRECS, ids=[p for p, _ in PRECS])
@pytest.mark.parametrize("lanes", [1, 3])
def test_relu6_store_is_the_clamp_of_the_plain_store(prec, act, lanes):
    """relu = 2 == clamp(relu = 0, 0, 6) and relu = 1 == clamp_min(relu = 0, 0), bit for bit: both bounds are exact in bf16 and
    f32, so the clamp commutes with the store's rounding — for every family, with and without a residual, with lanes"""
    import bayesian_torch_amd as bt
    dev = _dev()
    idx = [5, 11, 12][:lanes]
    for cls, kw, xs, gather in CASES:
        layer = _layer(cls, kw, prec)
        nout = kw.get("out_channels", kw.get("out_features"))
        is_stem = kw.get("in_channels", 99) <= 4
        x = (torch.randn((xs[0] * lanes,) + tuple(xs[1:]), device=dev) * 2).to(act)
        scale = (torch.rand(nout, device=dev) * 4 + 2).contiguous()
        shift = torch.randn(nout, device=dev).contiguous()
        for with_res in ([False] if is_stem else [False, True]):
            outs = {}
            with torch.no_grad():
                if lanes > 1:
                    bt.set_sample_lanes(layer, idx, batch=xs[0])
                res = None
                for code in (0, 1, 2):
                    ep = dict(scale=scale, shift=shift, residual=None, relu=code)
                    if with_res:
                        if res is None:
                            res = (torch.randn_like(layer._forward_hip(x, sample_idx=idx[0], epilogue=ep).float()) * 4).to(act)
                        ep["residual"] = res
                    outs[code] = layer._forward_hip(x, sample_idx=idx[0], gather=gather, epilogue=ep).float()
                bt.set_sample_lanes(layer, None)
            y0 = outs[0]
            tag = (cls, xs, prec, lanes, with_res)
            assert (y0 > 6).any() and (y0 < 0).any(), tag
            assert torch.equal(outs[2], y0.clamp(0, 6)), tag
            assert torch.equal(outs[1], y0.clamp_min(0)), tag


def test_stem_pool_refuses_relu6_and_the_python_face_clamps():
    """the stem + max-pool kernel has no ReLU6: the C-ABI refuses relu = 2 with pool = 1, forward_fused runs the ReLU launch and
    clamps; max-pool and min(., 6) commute, so the result is clamp(pool(relu = 0 store), 0, 6)"""
    from bayesian_torch_amd import _lib
    dev = _dev()
    layer = _layer("Conv2dFlipout", dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), "bf16")
    x = (torch.randn(2, 3, 224, 224, device=dev) * 2).to(torch.bfloat16)
    assert layer.pool_fusable(x)
    ep = _lib.Epilogue()
    ep.pool, ep.relu = 1, 1
    assert _plan(layer, tuple(x.shape), "bf16", ep=ep)[:2] == (0, "stem_pool")
    ep.relu = 2
    assert _plan(layer, tuple(x.shape), "bf16", ep=ep)[0] == _lib.E_UNSUPPORTED
    scale = (torch.rand(64, device=dev) * 4 + 2).contiguous()
    shift = torch.randn(64, device=dev).contiguous()
    with torch.no_grad():
        y0 = layer._forward_hip(x, sample_idx=4, epilogue=dict(scale=scale, shift=shift, relu=0, pool=True)).float()
        layer._btx_sample = 4
        y6 = layer.forward_fused(x, scale, shift, None, pool=True, act="relu6").float()
    assert (y0 > 6).any()
    assert torch.equal(y6, y0.clamp(0, 6))


def _gpu_model(name, prec, act):
    dev = _dev()
    m = make(name).to(dev)
    if act == torch.bfloat16:
        for b in m.modules():
            if isinstance(b, torch.nn.modules.batchnorm._BatchNorm):
                b.to(torch.bfloat16)
    return m


@pytest.mark.parametrize("prec,act,tol", [("f32", torch.float32, 1e-5), ("bf16x3", torch.float32, 1e-5),
                                          ("bf16", torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_fused_model_matches_unfused_on_the_gpu(name, prec, act, tol):
    import warnings
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    dev = _dev()
    bt.set_precision(prec)
    try:
        m = _gpu_model(name, prec, act)
        x = torch.randn(4, 3, 16, 16, device=dev).to(act)
        with torch.no_grad():
            bt.set_sample_index(m, 3)
            a = m(x).float()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert fuse_model(m) == MODELS[name][1]
            bt.set_sample_index(m, 3)
            b = m(x).float()
        err = float((a - b).norm() / a.norm())
        assert err <= tol, (name, prec, err)
    finally:
        bt.set_precision("f32")


@pytest.mark.parametrize("name", ["mobilenet_v2", "vgg_bn"])
def test_fused_model_lanes_under_graphed_mc(name):
    """GraphedMC(lanes=4) on a fused model: each lane of an eager lane launch and of a run_many replay equals the single-sample
    forward of its sample index bit for bit; the replay's statistics equal the sum over those samples (summed in another order)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd import functional as BF
    from bayesian_torch_amd.models import fuse_model
    dev = _dev()
    bt.set_precision("bf16")
    try:
        m = _gpu_model(name, "bf16", torch.bfloat16).eval()
        bt.assign_layer_ids(m)
        assert fuse_model(m) == MODELS[name][1]
        x = torch.randn(8, 3, 16, 16, device=dev).to(torch.bfloat16)
        idx = [3, 9, 10, 77]
        with torch.no_grad():
            singles = []
            with BF.concurrent_plan():
                for s in idx:
                    bt.set_sample_index(m, s)
                    singles.append(m(x).float().clone())
            bt.set_sample_lanes(m, idx, batch=8)
            y = m(x).float()
            bt.set_sample_lanes(m, None)
        for l in range(4):
            assert torch.equal(y[l * 8:(l + 1) * 8], singles[l]), l
        want = torch.zeros(mc.packed_numel(8, 10), dtype=torch.float32, device=dev)
        for t in singles:
            mc.accumulate(want, t.to(torch.bfloat16), 0.0)
        g = mc.GraphedMC(m, x, kl=0.0, lanes=4, keep_logits=True)
        g.run_many(idx)
        torch.cuda.synchronize()
        for l in range(4):
            assert torch.equal(g.lane_logits[l].float(), singles[l]), l
        assert torch.allclose(g.packed, want, rtol=1e-6, atol=1e-6)
        g.close()
        out = mc.mc_forward(m, x, 4)
        assert out is not None
    finally:
        bt.set_precision("f32")
