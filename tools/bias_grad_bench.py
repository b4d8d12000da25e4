"""What the fixed-order bias gradient (csrc/btx_biasgrad.hip, btx_bias_grad: one or two launches of its own per layer with a bias) costs
against the weight-gradient kernel's by-product (f32 atomics over its pixel chunks; functional.BIAS_ATOMICS = True):

  1. us per eager forward + backward of single layers with a bias (what a small model's training loop sees, host-bound);
  2. ms per replay of autograd.GraphedTrainStep on the dnn_to_bnn ResNet18 (Flipout, batch 64, 224^2, bf16 contraction, hip_batchnorm;
     its convolutions have no bias, the 512 -> 1000 head has one).

    python tools/bias_grad_bench.py [--out profiles/bias_grad_bench.txt] [--regions 20] [--inner 50]

Method: as tools/mc_loss_bench.py — HIP events around `inner` back-to-back calls form a region, `regions` regions run back to back and
the figure is the median (min .. max) of the second, settled half."""
import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

from mc_loss_bench import PRIOR, settled_regions  # noqa: E402

LAYERS = [("LinearFlipout", dict(in_features=128, out_features=64), (200, 128), "f32"),
          ("LinearFlipout", dict(in_features=512, out_features=1000), (64, 512), "bf16"),
          ("Conv2dReparameterization", dict(in_channels=32, out_channels=64, kernel_size=3), (2, 32, 10, 10), "f32"),
          ("Conv2dFlipout", dict(in_channels=64, out_channels=64, kernel_size=3, padding=1), (64, 64, 56, 56), "bf16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias_grad_bench.txt"))
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    assert a.regions >= 8 and torch.cuda.is_available()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/bias_grad_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; median (min .. max) of the settled half of %d back-to-back regions" % (
        torch.cuda.get_device_name(0), torch.__version__, a.regions))
    emit("eager forward + backward of one layer with a bias, us per call (%d calls per region):" % a.inner)
    cell = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731
    for cls, kw, xshape, prec in LAYERS:
        bt.manual_seed(1)
        bt.set_precision(prec)
        torch.manual_seed(0)
        layer = getattr(L, cls)(**kw).to(dev)
        x = torch.randn(*xshape, device=dev)
        if prec == "bf16":
            x = x.to(torch.bfloat16)
        if x.dim() == 4:
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        with torch.no_grad():
            dy = torch.randn_like(layer(x, return_kl=False))

        def fn():
            for p in layer.parameters():
                p.grad = None
            x.grad = None
            layer(x, return_kl=False).backward(dy)
        res = {}
        for flag in (True, False):
            BF.BIAS_ATOMICS = flag
            res[flag] = settled_regions(fn, a.inner, a.regions)
        BF.BIAS_ATOMICS = False
        emit("  %-26s %-18s %4s | by-product (atomics) %s | btx_bias_grad %s | %.3fx" % (
            cls, "x".join(map(str, xshape)), prec, cell(res[True]), cell(res[False]), res[False][0] / res[True][0]))
    bt.manual_seed(1)
    torch.manual_seed(0)
    rn = resnet.resnet18()
    bt.dnn_to_bnn(rn, dict(PRIOR, type="Flipout"))
    rn = rn.to(dev).train()
    bt.assign_layer_ids(rn)
    bt.set_precision("bf16")
    hip_batchnorm(rn)
    x = torch.randn(64, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (64,), device=dev)
    it = iter(range(1 << 30))
    res = {}
    for flag in (True, False):
        BF.BIAS_ATOMICS = flag  # read when the step is captured
        gc.collect()
        gs = GraphedTrainStep(rn, x, y)
        res[flag] = settled_regions(lambda: gs.run(next(it)), max(2, a.inner // 10), a.regions)
        gs.close()
        del gs
    BF.BIAS_ATOMICS = False
    bt.set_precision("f32")
    emit("GraphedTrainStep, ResNet18 Flipout, batch 64, 224^2, bf16 contraction, hip_batchnorm, ms per replay:")
    emit("  by-product (atomics) %8.3f (%.3f .. %.3f) | btx_bias_grad %8.3f (%.3f .. %.3f) | %.4fx" % (
        tuple(v / 1e3 for v in res[True]) + tuple(v / 1e3 for v in res[False]) + (res[False][0] / res[True][0],)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
