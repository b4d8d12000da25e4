"""GPU time per captured forward of the ResNet18 convolution and head layers (batch 64, 224^2 input, bf16) as LocalReparameterization
(BTX_KIND_LRT) against Reparameterization and Flipout on their current kernels, for 1 and 20 MC sample lanes, with the
kernel family each launch took.  There is no pass mark: LRT runs on the register-staged / gather family by construction, the slowest
one; this table is what moving it onto the LDS-DMA families (taps, gemm8, stem) is priced from.

    python tools/lrt_bench.py [--out profiles/lrt_bench.txt] [--regions 10] [--inner 20] [--lanes 1,20]

One "captured forward" is what mc.GraphedMC replays for one layer: the weight pre-sampling launch of the layer (Reparameterization,
Flipout: rng.presample with the mean tiles cached, as lane_mode "launch" does; LRT has nothing to sample) and the layer's forward,
captured into a hipGraph with the sample words on the device.  With lanes the input holds the lanes back to back (the activations
behind the first layer of a model); the stem reads ONE batch for all lanes, as the first layer of a model does.

Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back replays form one region; `regions` regions run back to back
after a warm-up of the same shape and the figure is the median of the SECOND half of them, with the range of that half beside it."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mc_loss_bench import capture, settled_regions  # noqa: E402

BATCH = 64
# (name, class stem, kwargs, input extent, occurrences in ResNet18)
LAYERS = [
    ("stem 7x7/2 3->64 @224", "Conv2d", dict(in_channels=3, out_channels=64, kernel_size=7, stride=2, padding=3, bias=False), 224, 1),
    ("layer1 3x3 64->64 @56", "Conv2d", dict(in_channels=64, out_channels=64, kernel_size=3, padding=1, bias=False), 56, 4),
    ("layer2 3x3/2 64->128 @56", "Conv2d", dict(in_channels=64, out_channels=128, kernel_size=3, stride=2, padding=1, bias=False), 56, 1),
    ("layer2 1x1/2 64->128 @56", "Conv2d", dict(in_channels=64, out_channels=128, kernel_size=1, stride=2, bias=False), 56, 1),
    ("layer2 3x3 128->128 @28", "Conv2d", dict(in_channels=128, out_channels=128, kernel_size=3, padding=1, bias=False), 28, 3),
    ("layer3 3x3/2 128->256 @28", "Conv2d", dict(in_channels=128, out_channels=256, kernel_size=3, stride=2, padding=1, bias=False), 28, 1),
    ("layer3 1x1/2 128->256 @28", "Conv2d", dict(in_channels=128, out_channels=256, kernel_size=1, stride=2, bias=False), 28, 1),
    ("layer3 3x3 256->256 @14", "Conv2d", dict(in_channels=256, out_channels=256, kernel_size=3, padding=1, bias=False), 14, 3),
    ("layer4 3x3/2 256->512 @14", "Conv2d", dict(in_channels=256, out_channels=512, kernel_size=3, stride=2, padding=1, bias=False), 14, 1),
    ("layer4 1x1/2 256->512 @14", "Conv2d", dict(in_channels=256, out_channels=512, kernel_size=1, stride=2, bias=False), 14, 1),
    ("layer4 3x3 512->512 @7", "Conv2d", dict(in_channels=512, out_channels=512, kernel_size=3, padding=1, bias=False), 7, 3),
    ("fc 512->1000", "Linear", dict(in_features=512, out_features=1000), 0, 1),
]
KINDS = ("Reparameterization", "Flipout", "LocalReparameterization")
FAMILIES = ("gather", "regstage", "dma", "gemm8", "patch", "taps", "taps2", "stem", "stem_pool")


class _FamilyLog:
    """records the kernel family of every contraction launch made while it is active: functional.contract_hip is wrapped, and the
    planner is asked (btx_contract_plan_info) about the launch the call is about to make"""

    def __init__(self):
        self.seen = []

    def __enter__(self):
        from bayesian_torch_amd import _lib, functional as BF
        self._orig = BF.contract_hip
        log = self

        def wrapped(kind, x, mu_p, rho_p, mu_b, rho_b, op, seed, sample_idx, layer_id, prec=None, noise=None, extra_flags=0,
                    out_dtype=None, epilogue=None, sampled_w=None, sample_dev=None, lanes=1, lane_batch=None, **kw):
            xp, nb, spatial, _ = BF._to_channels_last(x, op)
            if lanes > 1 and nb != lane_batch:
                nb = nb // lanes
            flags = (_lib.FLAG_TRANSPOSED if op.transposed else 0) | extra_flags | (_lib.FLAG_CONCURRENT if BF._CONCURRENT else 0)
            if lanes > 1:
                flags |= lanes << _lib.FLAG_LANES_SHIFT
            if out_dtype is not None and out_dtype != x.dtype:
                flags |= _lib.FLAG_OUT_BF16 if out_dtype == torch.bfloat16 else _lib.FLAG_OUT_F32
            g = _lib.Geom()
            g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
            g.KD, g.KH, g.KW = op.kernel
            g.sd, g.sh, g.sw = op.stride
            g.pd, g.ph, g.pw = op.padding
            g.dd, g.dh, g.dw = op.dilation
            g.od, g.oh, g.ow = op.output_padding
            g.groups = op.groups
            info = _lib.PlanInfo()
            rc = _lib.lib().btx_contract_plan_info(kind, ctypes.byref(g), _lib.ACT_BF16 if xp.dtype == torch.bfloat16 else _lib.ACT_F32,
                                                   _lib.PREC_CODE[prec or BF.get_precision()], flags, None, ctypes.byref(info))
            log.seen.append("%s%s" % (FAMILIES[info.family], "/k%d" % info.ksplits if info.ksplits > 1 else "") if rc == 0 else "rc%d" % rc)
            return log._orig(kind, x, mu_p, rho_p, mu_b, rho_b, op, seed, sample_idx, layer_id, prec=prec, noise=noise,
                             extra_flags=extra_flags, out_dtype=out_dtype, epilogue=epilogue, sampled_w=sampled_w, sample_dev=sample_dev,
                             lanes=lanes, lane_batch=lane_batch, **kw)
        BF.contract_hip = wrapped
        return self

    def __exit__(self, *exc):
        from bayesian_torch_amd import functional as BF
        BF.contract_hip = self._orig


def _layer(stem, kind, kw, dev):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(1)
    torch.manual_seed(0)
    layer = getattr(L, stem + kind)(**kw).to(dev).eval()
    layer.dnn_to_bnn_flag = True
    layer.precision = "bf16"
    return layer


def _input(stem, kw, extent, lanes, dev):
    g = torch.Generator().manual_seed(3)
    if stem == "Linear":
        return torch.randn(lanes * BATCH, kw["in_features"], generator=g).to(dev).to(torch.bfloat16)
    shared = kw["in_channels"] <= 4   # the first layer of a model reads one batch for every lane
    x = torch.randn((BATCH if shared else lanes * BATCH), kw["in_channels"], extent, extent, generator=g)
    return x.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def bench_cell(stem, kind, kw, extent, lanes, a, dev):
    """(median, min, max) us per captured forward, the families of its contraction launches"""
    from bayesian_torch_amd import rng
    layer = _layer(stem, kind, kw, dev)
    x = _input(stem, kw, extent, lanes, dev)
    words = torch.zeros(lanes, dtype=torch.int32, device=dev)
    tiles = {}
    if lanes > 1:
        rng.set_sample_lanes(layer, list(range(lanes)), batch=BATCH, sample_dev=words)
    else:
        layer.__dict__["_btx_sample_dev"] = words

    def forward(skip_mu):
        rng.presample(layer, 0, cache=tiles, skip_mu=skip_mu)
        return layer(x)
    with torch.no_grad():
        with _FamilyLog() as log:
            forward(False)
        torch.cuda.synchronize()
        graph = capture(lambda: forward(True), dev)
        res = settled_regions(graph.replay, a.inner, a.regions)
    del graph
    rng.set_sample_lanes(layer, None)
    return res, ",".join(sorted(set(log.seen)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrt_bench.txt"))
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--lanes", default="1,20")
    a = ap.parse_args()
    assert a.regions >= 8, "the settled half needs at least 8 regions"
    assert torch.cuda.is_available(), "lrt_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/lrt_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; us per captured forward (pre-sampling launch + layer forward, one hipGraph replay), batch %d per lane, "
         "bf16: median (min .. max) of the settled half of %d back-to-back regions of %d replays" % (
             torch.cuda.get_device_name(0), torch.__version__, BATCH, a.regions, a.inner))
    cell = lambda r, fam: "%9.1f (%8.1f ..%8.1f) %-12s" % (r + (fam,))  # noqa: E731
    for lanes in [int(v) for v in a.lanes.split(",")]:
        emit("")
        emit("lanes = %d" % lanes)
        emit("%-27s %2s | %-44s | %-44s | %-44s | %6s %6s" % ("layer", "n", "Reparameterization", "Flipout", "LocalReparameterization",
                                                              "/rep", "/flip"))
        total = {k: 0.0 for k in KINDS}
        for name, stem, kw, extent, count in LAYERS:
            res = {}
            for kind in KINDS:
                res[kind] = bench_cell(stem, kind, kw, extent, lanes, a, dev)
                total[kind] += count * res[kind][0][0]
                torch.cuda.empty_cache()
            lrt = res[KINDS[2]][0][0]
            emit("%-27s %2d | %s | %s | %s | %6.2f %6.2f" % (name, count, cell(*res[KINDS[0]]), cell(*res[KINDS[1]]), cell(*res[KINDS[2]]),
                                                           lrt / res[KINDS[0]][0][0], lrt / res[KINDS[1]][0][0]))
        emit("sum over the network's %d layers (n x median): Reparameterization %.0f us, Flipout %.0f us, LocalReparameterization %.0f us"
             % (sum(l[4] for l in LAYERS), total[KINDS[0]], total[KINDS[1]], total[KINDS[2]]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
