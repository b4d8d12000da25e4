"""The planner's side of the depthwise family (BTX-DW v1): btx_contract_plan_info is host-only, no GPU."""
import ctypes

import pytest

from bayesian_torch_amd import _lib

# (C, k, stride, pad, dil, N x C x H x W): the geometries of tests/test_gpu_depthwise.py
GEOMS = [(72, 3, 1, 1, 1, (2, 72, 13, 11)), (24, 3, 2, 1, 1, (3, 24, 15, 9)), (144, 3, 1, 1, 1, (2, 144, 7, 7)),
         (64, 5, 1, 2, 1, (2, 64, 12, 12)), (32, 7, 2, 3, 1, (1, 32, 17, 20)), (64, 3, 1, 2, 2, (2, 64, 10, 14)),
         (40, 3, 1, 0, 1, (2, 40, 9, 9)), (64, 3, 1, 1, 1, (2, 64, 40, 70))]
PRECS = [("f32", _lib.ACT_F32), ("bf16x3", _lib.ACT_F32), ("bf16", _lib.ACT_BF16)]
KINDS = [_lib.KIND_REPARAM, _lib.KIND_FLIPOUT]


def geom(C, k, s, p, d, xshape, N=None, groups=None):
    g = _lib.Geom()
    g.NB, (g.D, g.H, g.W), g.C, g.N = xshape[0], (1, xshape[2], xshape[3]), C, N or C
    g.KD, g.KH, g.KW = 1, k, k
    g.sd, g.sh, g.sw = 1, s, s
    g.pd, g.ph, g.pw = 0, p, p
    g.dd, g.dh, g.dw = 1, d, d
    g.groups = groups or C
    return g


def plan(g, kind, prec, act, flags=0, ep=None):
    info = _lib.PlanInfo()
    rc = _lib.lib().btx_contract_plan_info(kind, ctypes.byref(g), act, _lib.PREC_CODE[prec], flags,
                                           ctypes.byref(ep) if ep is not None else None, ctypes.byref(info))
    return rc, (_lib.FAMILIES[info.family] if rc == 0 else None), info


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("transposed", [False, True], ids=["conv", "transposed"])
@pytest.mark.parametrize("geo", GEOMS, ids=["C%d-k%d-s%d-p%d-d%d" % g[:5] for g in GEOMS])
def test_depthwise_geometries_plan_on_the_depthwise_family(geo, transposed, lanes):
    flags = (_lib.FLAG_TRANSPOSED if transposed else 0) | (lanes << _lib.FLAG_LANES_SHIFT if lanes > 1 else 0)
    for kind in KINDS:
        for prec, act in PRECS:
            rc, fam, info = plan(geom(*geo), kind, prec, act, flags)
            assert (rc, fam, info.ksplits, info.ws_bytes, info.lanes) == (0, "depthwise", 1, 0, lanes), (kind, prec, rc, fam)
            assert info.nwg >= geo[5][0] * -(-geo[0] // 64)  # at least one workgroup per image and 64-channel block


def test_what_the_family_declines_plans_as_before():
    """each condition alone sends the request where the parent sent it: the gather kernel, or a refusal"""
    base = GEOMS[0]
    for kind in KINDS:
        assert plan(geom(*base), kind, "f32", _lib.ACT_F32, _lib.FLAG_GATHER)[1] == "gather"
        assert plan(geom(36, 3, 1, 1, 1, (2, 36, 13, 11)), kind, "bf16", _lib.ACT_BF16)[1] == "gather"  # 36 bf16: no whole granules
        assert plan(geom(72, 3, 1, 1, 1, (2, 72, 13, 11), N=144), kind, "f32", _lib.ACT_F32)[1] == "gather"  # channel multiplier 2
        g3 = geom(*base)
        g3.D, g3.KD, g3.pd = 5, 3, 1  # a Conv3d
        assert plan(g3, kind, "f32", _lib.ACT_F32)[1] == "gather"
        ep = _lib.Epilogue()
        ep.pool = 1
        assert plan(geom(*base), kind, "f32", _lib.ACT_F32, ep=ep)[0] == _lib.E_UNSUPPORTED
    assert plan(geom(*base), _lib.KIND_LRT, "f32", _lib.ACT_F32)[1] == "gather"
