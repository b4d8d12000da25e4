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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthwise_bench.txt"))
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--lanes", type=int, nargs="*", default=[1, 8])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# python tools/depthwise_bench.py --regions %d --inner %d (batch 64 per lane; forward only)" % (a.regions, a.inner)]
    for lanes in a.lanes:
        for row in ROWS:
            for cls in ("Conv2dReparameterization", "Conv2dFlipout"):
                if lanes > 1 and (row[3] != 3 or row[4] != torch.bfloat16):
                    continue
                lines.append(bench_row(row, cls, lanes, a, dev))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
