"""Timing of the depthwise family (BTX-DW v1, csrc/btx_contract_dw.h) on the GPU.  No bar fixed in advance: the table decides which
shape classes the planner keeps on the family.

Per row, GPU time per captured call (one hipGraph replay) of the layer's forward
  * on the depthwise family,
  * on the route the parent commit takes, in the same build: gather=True (BTX_FLAG_GATHER), the element-wise MFMA kernel,
  * and of a device copy of x bytes + out bytes (the floor of a memory-bound stencil).
Both kernel columns are measured twice, interleaved (new, gather, new, gather); `spread` is the larger of the two differences between
the repeats.  Rows: every depthwise layer of MobileNetV2 at batch 64, bf16, Reparameterization and Flipout, lanes 1 and 8; one f32 row;
a 5x5 and a 7x7 row at C = 192 @ 28.

    python tools/depthwise_bench.py [--out profiles/depthwise_bench.txt] [--regions 10] [--inner 20]
    BTX_LIB=/path/to/libbtx.so python tools/depthwise_bench.py --step Flipout   # ms per captured MobileNetV2 training step (A/B of two builds)
    python tools/depthwise_bench.py --wgrad      # the weight gradient of the same rows at lanes = 1 -> profiles/depthwise_wgrad_bench.txt

Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back replays form one region; `regions` regions run back to back
after a warm-up and the figure is the median of the second, settled half."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mc_loss_bench import capture, settled_regions  # noqa: E402

MBV2 = ((32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2), (384, 14, 1), (576, 14, 1), (576, 14, 2),
        (960, 7, 1))
# (C, map, stride, k, dtype)
ROWS = [(c, m, s, 3, torch.bfloat16) for c, m, s in MBV2] + [(144, 56, 1, 3, torch.float32), (192, 28, 1, 5, torch.bfloat16),
                                                              (192, 28, 1, 7, torch.bfloat16)]


def bench_row(row, cls, lanes, a, dev):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    C, m, s, k, dtype = row
    prec = "bf16" if dtype == torch.bfloat16 else "f32"
    bt.manual_seed(1)
    layer = getattr(L, cls)(in_channels=C, out_channels=C, kernel_size=k, stride=s, padding=k // 2, groups=C, bias=False).to(dev)
    layer.precision = prec
    bt.assign_layer_ids(layer)
    x = torch.randn(64 * lanes, C, m, m, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
    if lanes > 1:
        bt.set_sample_lanes(layer, list(range(lanes)), batch=64)
    with torch.no_grad():
        out = layer._forward_hip(x, sample_idx=None if lanes > 1 else 3)
        fns = [lambda g=g: layer._forward_hip(x, sample_idx=None if lanes > 1 else 3, gather=g) for g in (False, True)]
        graphs = [capture(f, dev) for f in fns]
        t = [settled_regions(graphs[i % 2].replay, a.inner, a.regions)[0] for i in range(4)]
        src = torch.empty(x.numel() * x.element_size() + out.numel() * out.element_size(), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        half = src.numel() // 2  # a copy reads and writes each byte: half the bytes for the same traffic
        cp = settled_regions(capture(lambda: dst[:half].copy_(src[:half]), dev).replay, a.inner, a.regions)[0]
    new, old = min(t[0], t[2]), min(t[1], t[3])
    spread = max(abs(t[0] - t[2]), abs(t[1] - t[3]))
    return "%-4s C=%4d @%3d s%d k%d %-5s lanes=%d: depthwise %8.1f us  gather %8.1f us  (x%5.1f)  spread %5.1f us  copy floor %7.1f us  (%.2fx floor)" % (
        "rep" if "Reparam" in cls else "flip", C, m, s, k, prec, lanes, new, old, old / new, spread, cp, new / cp)


def bench_wgrad_row(row, cls, a, dev):
    """--wgrad: the layer's weight gradient as ContractFn.backward asks for it (BF.wgrad_hip with the fused drho, bias gradients
    elsewhere): the stencil reduction (btx_contract_dw_wgrad.h) | BTX_FLAG_GATHER, the generic kernel | a copy of the bytes of x + dy"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import _lib, functional as BF, layers as L, rng as _rng
    C, m, s, k, dtype = row
    prec = "bf16" if dtype == torch.bfloat16 else "f32"
    bt.manual_seed(1)
    layer = getattr(L, cls)(in_channels=C, out_channels=C, kernel_size=k, stride=s, padding=k // 2, groups=C, bias=False).to(dev)
    bt.assign_layer_ids(layer)
    mo = (m + 2 * (k // 2) - k) // s + 1
    x = torch.randn(64, C, m, m, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(64, C, mo, mo, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
    kind = _lib.KIND_FLIPOUT if "Flipout" in cls else _lib.KIND_REPARAM
    op, w_shape = layer._op, tuple(layer._w()[0].shape)
    rho_f = BF.gemm_major_view(layer._w()[1].detach(), op).reshape(-1).contiguous()
    with torch.no_grad():
        fns = [lambda f=f: BF.wgrad_hip(kind, x, dy, op, _rng.seed(), 3, layer._btx_layer_id, w_shape, raw=True, rho_flat=rho_f, _flags=f)
               for f in (0, _lib.FLAG_GATHER)]
        graphs = [capture(f, dev) for f in fns]
        t = [settled_regions(graphs[i % 2].replay, a.inner, a.regions)[0] for i in range(4)]
        src = torch.empty((x.numel() + dy.numel()) * x.element_size(), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        half = src.numel() // 2  # a copy reads and writes each byte: half the bytes for the same traffic
        cp = settled_regions(capture(lambda: dst[:half].copy_(src[:half]), dev).replay, a.inner, a.regions)[0]
    new, old = min(t[0], t[2]), min(t[1], t[3])
    spread = max(abs(t[0] - t[2]), abs(t[1] - t[3]))
    return "%-4s C=%4d @%3d s%d k%d %-5s wgrad: stencil %8.1f us  gather %8.1f us  (x%5.1f)  spread %5.1f us  copy floor %7.1f us  (%.2fx floor)" % (
        "rep" if "Reparam" in cls else "flip", C, m, s, k, prec, new, old, old / new, spread, cp, new / cp)


def bench_step(typ, replays):
    """--step TYPE: ms per captured training step (GraphedTrainStep: forward + loss + backward; the BatchNorm parameters are bf16, so
    no fused update in the graph) of the dnn_to_bnn MobileNetV2 of tools/fuse_model_bench.py, batch 64, bf16: three regions of
    `replays` replays after two warm replays.  The library is the one BTX_LIB names, so two builds can alternate in one session."""
    import bayesian_torch_amd as bt
    import fuse_model_bench as FB
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = torch.device("cuda:0")
    bt.set_precision("bf16")
    m, _ = FB.build("mobilenet_v2", typ, dev, False)
    x = torch.randn(64, 3, 224, 224, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gs = GraphedTrainStep(m.train(), x, torch.randint(0, 1000, (64,), device=dev))
    try:
        ms = []
        for r in range(-1, 3):  # region -1: the warm replays
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(replays if r >= 0 else 2):
                gs.run(2 + r * replays + s)
            e1.record()
            torch.cuda.synchronize(dev)
            ms.append(round(e0.elapsed_time(e1) / replays, 3))
    finally:
        gs.close()
    print("%s: ms per captured training step %s (library %s)" % (typ, ms[1:], os.environ.get("BTX_LIB", "in tree")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, metavar="TYPE", help="Flipout | Reparameterization: time the captured MobileNetV2 training step")
    ap.add_argument("--wgrad", action="store_true", help="time the weight gradient (default --out: profiles/depthwise_wgrad_bench.txt)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--lanes", type=int, nargs="*", default=[1, 8])
    a = ap.parse_args()
    if a.step:
        return bench_step(a.step, 5)
    a.out = a.out or os.path.join(ROOT, "profiles", "depthwise_wgrad_bench.txt" if a.wgrad else "depthwise_bench.txt")
    dev = torch.device("cuda:0")
    lines = ["# python tools/depthwise_bench.py --regions %d --inner %d (batch 64 per lane; forward only)" % (a.regions, a.inner)]
    if a.wgrad:
        lines = ["# python tools/depthwise_bench.py --wgrad --regions %d --inner %d (batch 64; dw_mu, dw_delta and the fused drho)" % (a.regions, a.inner)]
    for lanes in ([] if a.wgrad else a.lanes):
        for row in ROWS:
            for cls in ("Conv2dReparameterization", "Conv2dFlipout"):
                if lanes > 1 and (row[3] != 3 or row[4] != torch.bfloat16):
                    continue
                lines.append(bench_row(row, cls, lanes, a, dev))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
    for row in (ROWS if a.wgrad else []):
        for cls in ("Conv2dReparameterization", "Conv2dFlipout"):
            lines.append(bench_wgrad_row(row, cls, a, dev))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
