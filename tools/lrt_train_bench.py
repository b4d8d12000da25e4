"""GPU time of a captured training forward + backward of the ResNet18 layers as LocalReparameterization (batch 64, 224^2 input, bf16),
fused (layer.fused_training = True: btx_lrt_fwd_train + btx_lrt_bwd, DESIGN.md §21 "Backward") against the ATen composite (the switch
off: the path every LRT layer trained through before), and of the whole captured training step of a ResNet18-LocalReparameterization
with optim.Adam inside the graph, switch off against on.  There is no pass mark: the table is what the default of the switch is
decided from.

    python tools/lrt_train_bench.py [--out profiles/lrt_train_bench.txt] [--regions 10] [--inner 10] [--skip-step]

One "captured forward + backward" is a hipGraph of: out = layer(x); out.backward(g) with the sample word on the device, x requiring a
gradient (except the stem, the first layer of a model) and fresh gradient tensors.  Method (tools/lrt_bench.py, tools/mc_loss_bench.py):
HIP events around `inner` back-to-back replays form one region; `regions` regions run back to back after a warm-up of the same shape
and the figure is the median of the SECOND half of them, with the range of that half beside it."""
import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

from lrt_bench import BATCH, LAYERS  # noqa: E402
from mc_loss_bench import capture, settled_regions  # noqa: E402

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def bench_layer(stem, kw, extent, fused, a, dev):
    """(median, min, max) us per captured forward + backward, and whether the call took the fused path"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF, layers as L
    bt.manual_seed(1)
    torch.manual_seed(0)
    layer = getattr(L, stem + "LocalReparameterization")(**kw).to(dev).train()
    layer.dnn_to_bnn_flag, layer.precision, layer.fused_training = True, "bf16", fused
    layer.__dict__["_btx_sample_dev"] = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(3)
    if stem == "Linear":
        x = torch.randn(BATCH, kw["in_features"], generator=g).to(dev).to(torch.bfloat16).requires_grad_()
    else:
        x = torch.randn(BATCH, kw["in_channels"], extent, extent, generator=g).to(dev).to(torch.bfloat16)
        x = x.contiguous(memory_format=torch.channels_last).requires_grad_(kw["in_channels"] > 4)
    took = BF.lrt_train_ok(layer, x)
    gy = torch.randn_like(layer(x).detach())

    def step():
        for p in layer.parameters():
            p.grad = None
        x.grad = None
        layer(x).backward(gy)
    graph = capture(step, dev)
    res = settled_regions(graph.replay, a.inner, a.regions)
    del graph
    gc.collect()
    torch.cuda.empty_cache()
    return res, took


def bench_step(fused, a, dev, act=torch.float32):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models import fuse_model, resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    bt.manual_seed(1)
    torch.manual_seed(0)
    rn = resnet.resnet18()
    bt.dnn_to_bnn(rn, dict(PRIOR, type="LocalReparameterization"))
    rn = rn.to(dev).train()
    bt.assign_layer_ids(rn)
    bt.set_precision("bf16")
    hip_batchnorm(rn)
    if fused:
        fuse_model(rn, lrt_training=True)
    if fused == "body":  # every layer but the channel-padded stem
        rn.conv1.fused_training = False
    x = torch.randn(BATCH, 3, 224, 224, device=dev).to(act)
    y = torch.randint(0, 1000, (BATCH,), device=dev)
    gs = GraphedTrainStep(rn, x, y, optimizer=optim.Adam(rn.parameters(), lr=1e-3))
    it = iter(range(1 << 30))
    res = settled_regions(lambda: gs.run(next(it)), max(2, a.inner // 2), a.regions)
    loss = float(gs.loss)
    gs.close()
    bt.set_precision("f32")
    del gs, rn
    gc.collect()
    torch.cuda.empty_cache()
    return res, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrt_train_bench.txt"))
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    assert a.regions >= 8, "the settled half needs at least 8 regions"
    assert torch.cuda.is_available(), "lrt_train_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/lrt_train_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; us per captured training forward + backward (one hipGraph replay), batch %d, bf16 precision and "
         "activations: median (min .. max) of the settled half of %d back-to-back regions of %d replays" % (
             torch.cuda.get_device_name(0), torch.__version__, BATCH, a.regions, a.inner))
    emit("%-27s %2s | %-32s | %-32s | %9s" % ("layer", "n", "composite (switch off)", "fused (switch on)", "off / on"))
    cell = lambda r: "%9.1f (%8.1f ..%8.1f)" % r  # noqa: E731
    tot = [0.0, 0.0]
    for name, stem, kw, extent, count in LAYERS:
        (off, _), (on, took) = bench_layer(stem, kw, extent, False, a, dev), bench_layer(stem, kw, extent, True, a, dev)
        tot[0] += count * off[0]
        tot[1] += count * on[0]
        emit("%-27s %2d | %s | %s | %9.2f%s" % (name, count, cell(off), cell(on), off[0] / on[0], "" if took else "  (not covered: composite)"))
    emit("sum over the network's %d layers (n x median): composite %.0f us, fused %.0f us, %.2fx" % (
        sum(l[4] for l in LAYERS), tot[0], tot[1], tot[0] / tot[1]))
    if not a.skip_step:
        emit("")
        emit("whole captured training step of ResNet18-LocalReparameterization (forward + CE + KL / B + backward + optim.Adam in the graph), "
             "batch %d, 224^2, bf16 contraction, hip_batchnorm; us per GraphedTrainStep.run:" % BATCH)
        for act, what in ((torch.bfloat16, "bf16 activations (every parameter f32: the captured Adam updates f32 tensors)"), (torch.float32, "f32 activations")):
            emit(" " + what)
            (off, l0), (on, l1), (body, l2) = (bench_step(m, a, dev, act) for m in (False, True, "body"))
            emit("  switch off                       %s   last loss %.4f" % (cell(off), l0))
            emit("  switch on                        %s   last loss %.4f   off / on %.2fx" % (cell(on), l1, off[0] / on[0]))
            emit("  switch on, stem (conv1) left off %s   last loss %.4f   off / on %.2fx" % (cell(body), l2, off[0] / body[0]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
