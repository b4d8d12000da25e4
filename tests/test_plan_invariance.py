"""The f32 summation order of an MC sample does not depend on how many samples share its launch (no GPU needed).

include/btx.h (btx_contract_fwd_lanes): every lane of an n-lane launch computes bit for bit what a single-sample launch with
BTX_FLAG_CONCURRENT computes for its sample.  GraphedMC's tail groups, mc_forward's lane groups and the sample sharding over
ranks all rest on that.  Which kernel runs and how it splits K is decided on the host, by the routine btx_contract_plan_info
shares with the launch; this sweep holds the order signature (family, ksplits, kper, K-groups, par_major) of every lane count
against the one-lane plan over the contractions of the benched networks and around the planner's boundaries.  The tile shape
(wide, tall strips) and the stem-pool band length may differ: they move work between workgroups, not the order of a sum
(tests/test_gpu_lanes.py checks that on hardware).  A lane launch may also be refused (BTX_E_UNSUPPORTED): the caller then
runs the lanes as single-sample launches, which agree by construction."""
import ctypes

import pytest

from bayesian_torch_amd import _lib

LANES = (2, 3, 4, 5, 8, 16, 20, 32, 64, 255)
BATCHES = (1, 2, 4, 8, 16, 32, 64, 128)
PRECS = (("f32", _lib.PREC_F32, _lib.ACT_F32), ("bf16", _lib.PREC_BF16, _lib.ACT_BF16), ("bf16x3", _lib.PREC_BF16X3, _lib.ACT_F32))
KINDS = (("reparam", _lib.KIND_REPARAM), ("flipout", _lib.KIND_FLIPOUT))


def conv(name, cin, cout, hw, k, s=1, p=None, d=1, groups=1, nd=2, transposed=False, outpad=0):
    """(name, geometry kwargs without NB, flags, pool) of one contraction; hw is the input extent of every spatial axis"""
    p = (k // 2) * d if p is None else p
    sp = [1, 1, 1]
    kk, ss, pp, dd, op = [1, 1, 1], [1, 1, 1], [0, 0, 0], [1, 1, 1], [0, 0, 0]
    for a in range(3 - nd, 3):
        sp[a], kk[a], ss[a], pp[a], dd[a], op[a] = hw, k, s, p, d, outpad
    geo = dict(D=sp[0], H=sp[1], W=sp[2], C=cin, N=cout, KD=kk[0], KH=kk[1], KW=kk[2], sd=ss[0], sh=ss[1], sw=ss[2],
               pd=pp[0], ph=pp[1], pw=pp[2], dd=dd[0], dh=dd[1], dw=dd[2], od=op[0], oh=op[1], ow=op[2], groups=groups)
    return (name, geo, _lib.FLAG_TRANSPOSED if transposed else 0, False)


def linear(name, fin, fout):
    return conv(name, fin, fout, 1, 1, p=0, nd=0)


def stem(name, hw, pool):
    """the ResNet stem 7x7 / stride 2 / pad 3 as functional.rowfuse_plan lays it out: padding materialised, C padded to 4,
    the kernel row to 8 taps"""
    Wp = max((hw // 2 - 1) * 2 + 8, hw + 6)
    Wp += Wp % 2
    geo = dict(D=1, H=hw + 6, W=Wp, C=4, N=64, KD=1, KH=7, KW=8, sd=1, sh=2, sw=2, pd=0, ph=0, pw=0, dd=1, dh=1, dw=1,
               od=0, oh=0, ow=0, groups=1)
    return (name, geo, _lib.FLAG_ROWFUSE, pool)


def resnet_layers():
    out = [stem("stem", 224, False), stem("stem+pool", 224, True)]
    # ResNet18 (basic blocks)
    for cin, cout, hw in ((64, 64, 56), (64, 128, 56), (128, 256, 28), (256, 512, 14)):
        s = 1 if cin == cout else 2
        ho = hw // s
        out.append(conv("r18 3x3 %d->%d s%d @%d" % (cin, cout, s, hw), cin, cout, hw, 3, s))
        out.append(conv("r18 3x3 %d->%d @%d" % (cout, cout, ho), cout, cout, ho, 3))
        if s == 2:
            out.append(conv("r18 down 1x1 %d->%d @%d" % (cin, cout, hw), cin, cout, hw, 1, 2, 0))
    out.append(linear("r18 fc", 512, 1000))
    # ResNet50 (bottlenecks, stride on the 3x3)
    cin = 64
    for width, hw, s in ((64, 56, 1), (128, 56, 2), (256, 28, 2), (512, 14, 2)):
        ho = hw // s
        cout = 4 * width
        out.append(conv("r50 1x1 %d->%d @%d" % (cin, width, hw), cin, width, hw, 1, 1, 0))
        out.append(conv("r50 3x3 %d->%d s%d @%d" % (width, width, s, hw), width, width, hw, 3, s))
        out.append(conv("r50 1x1 %d->%d @%d" % (width, cout, ho), width, cout, ho, 1, 1, 0))
        out.append(conv("r50 down 1x1 %d->%d s%d @%d" % (cin, cout, s, hw), cin, cout, hw, 1, s, 0))
        out.append(conv("r50 1x1 %d->%d @%d" % (cout, width, ho), cout, width, ho, 1, 1, 0))
        if s == 2:
            out.append(conv("r50 3x3 %d->%d @%d" % (width, width, ho), width, width, ho, 3))
        cin = cout
    out.append(linear("r50 fc", 2048, 1000))
    return out


def other_layers():
    return [
        conv("vgg 3x3 256->256 @28", 256, 256, 28, 3),
        conv("vgg 3x3 512->512 @14", 512, 512, 14, 3),
        conv("vgg 3x3 512->512 @7", 512, 512, 7, 3),
        conv("odd 3x3 64->128 @13", 64, 128, 13, 3),
        conv("odd 3x3 s2 128->256 @15", 128, 256, 15, 3, 2),
        conv("odd 5x5 32->64 @11", 32, 64, 11, 5),
        conv("groups 3x3 256->256 g4 @14", 256, 256, 14, 3, groups=4),
        conv("depthwise-ish 3x3 128->128 g32 @14", 128, 128, 14, 3, groups=32),
        conv("dilated 3x3 d2 128->128 @28", 128, 128, 28, 3, d=2),
        conv("channel-padded 3x3 20->24 @9", 20, 24, 9, 3),
        conv("conv1d k5 64->128 @256", 64, 128, 256, 5, nd=1),
        conv("conv1d k3 s2 128->128 @100", 128, 128, 100, 3, 2, nd=1),
        conv("conv3d k3 32->64 @12", 32, 64, 12, 3, nd=3),
        conv("convT 3x3 s2 256->128 @14", 256, 128, 14, 3, 2, 1, transposed=True, outpad=1),
        conv("convT 3x3 s2 128->64 @28", 128, 64, 28, 3, 2, 1, transposed=True, outpad=1),
        conv("convT 4x4 s2 256->128 @14", 256, 128, 14, 4, 2, 1, transposed=True),
        conv("convT 4x4 s2 64->32 @28", 64, 32, 28, 4, 2, 1, transposed=True),
        linear("linear 8192->8192", 8192, 8192),  # its pre-sampled tiles of all lanes outgrow 32-bit descriptor offsets
        linear("linear 784->512", 784, 512),
    ]


class _Planner:
    def __init__(self):
        self.L = _lib.lib()
        self.g = _lib.Geom()
        self.info = _lib.PlanInfo()
        self.pool = _lib.Epilogue()
        self.pool.pool = 1

    def set(self, geo, nb):
        for k, v in geo.items():
            setattr(self.g, k, v)
        self.g.NB = nb

    def __call__(self, kind, prec, act, flags, pool, lanes=1):
        if lanes > 1:
            flags |= lanes << _lib.FLAG_LANES_SHIFT
        rc = self.L.btx_contract_plan_info(kind, ctypes.byref(self.g), act, prec, flags,
                                           ctypes.byref(self.pool) if pool else None, ctypes.byref(self.info))
        i = self.info
        return rc, (i.family, i.ksplits, i.kper, i.kgroups, i.par_major), (i.wide, i.tall, i.pool_band)


def _sweep(layers, batches):
    plan = _Planner()
    bad, seen = [], dict(families=set(), wide=set(), split=False, tall=False, par_major=False, bands=set(), refused=0)
    for name, geo, flags, pool in layers:
        for nb in batches:
            plan.set(geo, nb)
            for kname, kind in KINDS:
                for pname, prec, act in PRECS:
                    if flags & _lib.FLAG_ROWFUSE and act != (_lib.ACT_BF16 if prec == _lib.PREC_BF16 else _lib.ACT_F32):
                        continue
                    rc0, lat, _ = plan(kind, prec, act, flags, pool)  # the latency plan of a lone launch: boundary coverage only
                    if rc0 == 0:
                        seen["families"].add(lat[0])
                        seen["par_major"] |= bool(lat[4])
                    rc1, one, shape1 = plan(kind, prec, act, flags | _lib.FLAG_CONCURRENT, pool)
                    for n in LANES:
                        rc, sig, shape = plan(kind, prec, act, flags, pool, n)
                        if rc1 != 0:
                            assert rc == rc1, (name, nb, kname, pname, n, rc, rc1)
                            continue
                        if rc == _lib.E_UNSUPPORTED:
                            seen["refused"] += 1
                            continue
                        assert rc == 0, (name, nb, kname, pname, n, rc)
                        seen["families"].add(sig[0])
                        seen["wide"].add(shape[0])
                        seen["split"] |= sig[1] > 1
                        seen["tall"] |= bool(shape[1])
                        if shape[2]:
                            seen["bands"].add(shape[2])
                        if sig != one:
                            bad.append("%s nb=%d %s %s lanes=%d: %s (wide %d) vs one lane %s (wide %d)" % (
                                name, nb, kname, pname, n, _fmt(sig), shape[0], _fmt(one), shape1[0]))
    return bad, seen


def _fmt(sig):
    return "%s ks=%d kper=%d kg=%d par=%d" % ((_lib.FAMILIES[sig[0]],) + tuple(sig[1:]))


def test_lane_count_does_not_change_the_summation_order():
    bad, seen = _sweep(resnet_layers(), BATCHES)
    bad2, seen2 = _sweep(other_layers(), (1, 2, 8, 32, 128))
    bad += bad2
    assert not bad, "%d lane launches sum in another order than one lane:\n  " % len(bad) + "\n  ".join(bad[:40])
    # the sweep must stand on the boundaries it is meant to watch, not drift off them and pass vacuously
    fams = seen["families"] | seen2["families"]
    want = {_lib.FAMILIES.index(f) for f in ("gather", "regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem", "stem_pool")}
    assert want <= fams, sorted(_lib.FAMILIES[f] for f in want - fams)
    assert seen["wide"] == {0, 1}
    assert seen["split"] and seen["tall"]
    assert seen2["par_major"]
    assert len(seen["bands"]) >= 3, seen["bands"]
    assert seen2["refused"] > 0  # the 8192 x 8192 Linear at many lanes


def test_plan_info_is_the_plan_of_the_launch():
    """plan_info answers like the launch: argument errors, the workspace btx_contract_workspace_bytes reserves, the REVERSE
    flag (tile order only) and the lane bits of a btx_contract_fwd_ex call (cleared by the launch)"""
    plan = _Planner()
    L = plan.L
    name, geo, flags, pool = conv("r18 3x3 512->512 @7", 512, 512, 7, 3)
    plan.set(geo, 32)
    info = _lib.PlanInfo()
    assert L.btx_contract_plan_info(0, ctypes.byref(plan.g), 0, 0, 0, None, None) == -1
    assert L.btx_contract_plan_info(5, ctypes.byref(plan.g), 0, 0, 0, None, ctypes.byref(info)) == _lib.E_UNSUPPORTED
    assert L.btx_contract_plan_info(0, ctypes.byref(plan.g), 0, 7, 0, None, ctypes.byref(info)) == -5
    for kind in (_lib.KIND_REPARAM, _lib.KIND_FLIPOUT):
        for n in (1, 8, 20):
            fl = _lib.FLAG_CONCURRENT | (n << _lib.FLAG_LANES_SHIFT if n > 1 else 0)
            rc, sig, shape = plan(kind, _lib.PREC_BF16, _lib.ACT_BF16, fl, False)
            assert rc == 0 and plan.info.lanes == n
            need = plan.info.ws_bytes
            assert need <= L.btx_contract_workspace_bytes(ctypes.byref(plan.g), kind, _lib.ACT_BF16, _lib.PREC_BF16, fl)
            assert plan(kind, _lib.PREC_BF16, _lib.ACT_BF16, fl | _lib.FLAG_REVERSE, False) == (rc, sig, shape)
    # the stem-pool epilogue is refused where the launch refuses it
    name, geo, flags, pool = stem("stem+pool", 224, True)
    plan.set(geo, 4)
    rc, sig, _ = plan(_lib.KIND_FLIPOUT, _lib.PREC_BF16, _lib.ACT_BF16, flags, True)
    assert rc == 0 and _lib.FAMILIES[sig[0]] == "stem_pool"
    assert plan(_lib.KIND_FLIPOUT, _lib.PREC_F32, _lib.ACT_F32, flags, True)[0] == _lib.E_UNSUPPORTED
