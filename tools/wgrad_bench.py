"""Weight-gradient launches of ResNet18 (batch 64, bf16 activations, Flipout) one by one: the f32-atomics path of rounds 2-5
(functional.WGRAD_ATOMICS) and the slab path the library plans by default (the all-taps kernel of csrc/btx_wgrad_taps.h on the
3x3 / stride-1 rows, the chunk-slab path of the tap-per-workgroup kernel elsewhere) — time per call (HIP events, whole call:
memsets / kernel / slab reduction) and agreement between the two.

    python tools/wgrad_bench.py [--iters 20] [--batch 64]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayesian_torch_amd import _lib, functional as BF  # noqa: E402

SHAPES = [  # (label, cin, cout, H, k, stride)
    ("3x3 s1   64->64  56", 64, 64, 56, 3, 1), ("3x3 s1 128->128  28", 128, 128, 28, 3, 1),
    ("3x3 s1 256->256  14", 256, 256, 14, 3, 1), ("3x3 s1 512->512   7", 512, 512, 7, 3, 1),
    ("3x3 s2  64->128  56", 64, 128, 56, 3, 2), ("3x3 s2 128->256  28", 128, 256, 28, 3, 2),
    ("3x3 s2 256->512  14", 256, 512, 14, 3, 2), ("1x1 s2  64->128  56", 64, 128, 56, 1, 2),
    ("1x1 s2 128->256  28", 128, 256, 28, 1, 2), ("1x1 s2 256->512  14", 256, 512, 14, 1, 2),
]


def run(op, x, dy, iters, atomics):
    BF.WGRAD_ATOMICS = atomics
    w_shape = (op.out_channels, op.in_channels) + tuple(op.kernel[1:])
    call = lambda: BF.wgrad_hip(_lib.KIND_FLIPOUT, x, dy, op, 1234, 5, 7, w_shape, raw=True)  # noqa: E731
    out = call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(3):
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1) * 1e3 / iters)
    BF.WGRAD_ATOMICS = False
    return best, out[0].clone(), out[1].clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print("# us per btx_contract_wgrad* call, batch %d, bf16, Flipout (min of 3 x %d calls)" % (a.batch, a.iters))
    print("%-22s %10s %10s   %s" % ("layer", "atomics", "slab", "max rel diff vs atomics (mu, delta)"))
    tot = [0.0, 0.0]
    for label, cin, cout, hw, k, s in SHAPES:
        op = BF.OpDesc(2, cin, cout, k, s, k // 2)
        ho = op.out_spatial((1, hw, hw))[1]
        x = torch.randn(a.batch, cin, hw, hw, device=dev).relu_().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = (torch.randn(a.batch, cout, ho, ho, device=dev) * 0.01).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        ta, ma, da = run(op, x, dy, a.iters, True)
        ts, ms, ds = run(op, x, dy, a.iters, False)
        rel = lambda p, q: float((p - q).abs().max() / q.abs().max())  # noqa: E731
        print("%-22s %10.1f %10.1f   %.1e %.1e" % (label, ta, ts, rel(ms, ma), rel(ds, da)))
        tot = [tot[0] + ta, tot[1] + ts]
    print("%-22s %10.1f %10.1f" % ("sum", tot[0], tot[1]))


if __name__ == "__main__":
    main()
