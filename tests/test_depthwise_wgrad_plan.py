"""The planner's side of the depthwise weight gradient (BTX-DW v1): btx_wgrad_workspace_bytes is host-only, no GPU.
The slab count is transcribed from the rule DESIGN.md section 27 states; the BTX_FLAG_GATHER size is the generic kernel's."""
import ctypes

import pytest

from bayesian_torch_amd import _lib
from test_depthwise_plan import GEOMS, geom

KINDS = [_lib.KIND_REPARAM, _lib.KIND_FLIPOUT]
# slabs of several tiles with a ragged last one (GEOMS has one tile per slab): 57 one-tile images in 29 slabs of 2 on the 3x3 form;
# 22 images of 2 (bf16) or 4 (f32) tiles in slabs of 3 or 5 that cross image boundaries, a kernel row per workgroup
MULTI = [(576, 3, 1, 1, 1, (57, 576, 7, 7)), (320, 5, 1, 2, 1, (22, 320, 9, 33))]
ws_bytes = lambda g, kind, act, flags=0: int(_lib.lib().btx_wgrad_workspace_bytes(kind, ctypes.byref(g), act, flags))  # noqa: E731


def slabs(geo, kind, act):
    C, k, s, p, d, (NB, _, H, W) = geo
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    form1 = k == 3 and d == 1
    esz = 2 if act == _lib.ACT_BF16 else 4
    slots, pixb = 256 // (64 * esz // 16), 64 * esz + ((64 * esz // 16) if kind == _lib.KIND_FLIPOUT else 0)
    rows = lambda th: (th - 1) * s + 3 if form1 else th  # noqa: E731
    ct = -(-Wo // 32)
    while True:
        TW = -(-Wo // ct)
        TH = max(1, min(Ho, slots * 8 // TW))
        while TH >= 1 and rows(TH) * ((TW - 1) * s + (k - 1) * d + 1) * pixb > 64 * 1024:
            TH -= 1
        if TH >= 1:
            break
        ct += 1
    tiles = NB * -(-Ho // TH) * ct
    want = min(tiles, max(1, 512 // (-(-C // 64) * (1 if form1 else k))))
    tps = -(-tiles // want)
    return -(-tiles // tps), tps, tiles


@pytest.mark.parametrize("act", [_lib.ACT_F32, _lib.ACT_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS, ids=["reparam", "flipout"])
@pytest.mark.parametrize("geo", GEOMS + MULTI, ids=["C%d-k%d-s%d-p%d-d%d" % g[:5] for g in GEOMS + MULTI])
def test_workspace_covers_the_slabs_of_the_stencil_kernel(geo, kind, act):
    g, nk = geom(*geo), 2 if kind == _lib.KIND_FLIPOUT else 1
    gather, (n, tps, tiles) = ws_bytes(g, kind, act, _lib.FLAG_GATHER), slabs(geo, kind, act)
    assert gather > 0 and ws_bytes(g, kind, act) == max(n * nk * geo[0] * geo[1] ** 2 * 4, gather)
    if geo is GEOMS[7]:  # 64 @ 40x70: C * T = 576 > 512 workgroups is ONE chunk of the generic kernel; one slab of 5600 pixels is no plan
        assert n > 1 and ws_bytes(g, kind, act) > gather
    assert (tps > 1 and tiles % tps != 0) == (geo in MULTI)


@pytest.mark.parametrize("kind", KINDS, ids=["reparam", "flipout"])
def test_what_the_family_declines_sizes_as_the_generic_kernel(kind):
    g3 = geom(*GEOMS[7])
    g3.D, g3.KD, g3.pd = 5, 3, 1  # a Conv3d
    declined = [(geom(64, 3, 1, 1, 1, (2, 64, 40, 70), N=128), _lib.ACT_F32, 0),         # channel multiplier 2
                (geom(36, 3, 1, 1, 1, (2, 36, 40, 70)), _lib.ACT_BF16, 0),               # 36 bf16: no whole granules
                (g3, _lib.ACT_F32, 0)]
    for g, act, flags in declined:
        assert ws_bytes(g, kind, act, flags) == ws_bytes(g, kind, act, flags | _lib.FLAG_GATHER) > 0
    assert ws_bytes(geom(*GEOMS[7]), kind, _lib.ACT_BF16, _lib.FLAG_ROWFUSE) == 0  # row-fused geometries have groups == 1: refused as before
