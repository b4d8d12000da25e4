"""Timing of the num_mc > 1 training path on the GPU (no bar; the feature is the capability, not a speed-up):

  1. us per forward + backward of the loss heads on an MC stack [S, B, C] — utils.mc_loss.mc_elbo_loss (both reductions) and
     AvULoss / AUAvULoss with type=1 — through libbtx.so (csrc/btx_mcloss.hip) against the package's own ATen chain
     (set_backend("torch")) on the same GPU tensors, each issued eagerly and replayed from a captured graph;
  2. ms per replay of autograd.GraphedTrainStep on a dnn_to_bnn ResNet18 (Flipout, batch 64, 224^2, bf16 contraction,
     hip_batchnorm — the step tools/optim_bench.py times): ONE num_mc=2 replay against TWO num_mc=1 replays.

    python tools/mc_loss_bench.py [--out profiles/mc_loss_bench.txt] [--regions 20] [--inner 50] [--skip-train-step]

Method: HIP events around `inner` back-to-back calls form one region; `regions` regions run back to back after a warm-up of the same
shape and the figure is the median of the SECOND half of them (the settled clock: the first half carries the ramp of a package that
was idle a moment ago — bench.py's `settled`), with the range of that half beside it."""
import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
SHAPES = ((2, 64, 10), (5, 64, 1000), (5, 128, 1000))


def settled_regions(fn, inner, regions):
    """per-call microseconds: (median, min, max) of the second half of `regions` back-to-back regions of `inner` calls"""
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(regions)]
    for e0, e1 in ev:
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
    torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 / inner for e0, e1 in ev]
    tail = sorted(us[len(us) // 2:])
    return tail[len(tail) // 2], tail[0], tail[-1]


def capture(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g


def bench_heads(a, dev, emit):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.utils.avuc_loss import AUAvULoss, AvULoss
    from bayesian_torch_amd.utils.mc_loss import mc_elbo_loss
    avu, area = AvULoss(beta=3.0), AUAvULoss(beta=3.0)
    heads = (("mc_elbo logits", lambda st, y, kl: mc_elbo_loss(st, y, kl, "logits")),
             ("mc_elbo loss", lambda st, y, kl: mc_elbo_loss(st, y, kl, "loss")),
             ("AvULoss type=1", lambda st, y, kl: avu(st, y, 0.1, type=1).sum()),
             ("AUAvULoss type=1", lambda st, y, kl: area(st, y, type=1)[0].sum()))
    emit("%-17s %3s %4s %5s %5s | %26s %26s | %26s %26s | %7s %7s" % (
        "head", "S", "B", "C", "dtype", "HIP eager", "ATen chain eager", "HIP graph", "ATen chain graph", "x eager", "x graph"))
    cell = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731
    for name, head in heads:
        for S, B, C in SHAPES:
            for dt in (torch.float32, torch.bfloat16):
                g = torch.Generator().manual_seed(S * 1000003 + B * 10007 + C)
                st = (torch.randn(S, B, C, generator=g) * 3).to(dev).to(dt).requires_grad_(True)
                y = torch.randint(0, C, (B,), generator=g).to(dev)
                kl = torch.full((1,), 1000.0, device=dev)

                def fn():
                    st.grad = None
                    head(st, y, kl).backward()
                res = {}
                for backend in ("auto", "torch"):
                    bt.set_backend(backend)
                    res[backend, "eager"] = settled_regions(fn, a.inner, a.regions)
                    graph = capture(fn, dev)
                    res[backend, "graph"] = settled_regions(graph.replay, a.inner, a.regions)
                    del graph
                bt.set_backend("auto")
                emit("%-17s %3d %4d %5d %5s | %s %s | %s %s | %7.2f %7.2f" % (
                    name, S, B, C, "f32" if dt == torch.float32 else "bf16", cell(res["auto", "eager"]), cell(res["torch", "eager"]),
                    cell(res["auto", "graph"]), cell(res["torch", "graph"]),
                    res["torch", "eager"][0] / res["auto", "eager"][0], res["torch", "graph"][0] / res["auto", "graph"][0]))


def bench_step(a, dev, emit):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
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
    inner = max(2, a.inner // 10)
    res = {}
    for n in (1, 2):
        gc.collect()
        gs = GraphedTrainStep(rn, x, y, num_mc=n)
        if n == 1:
            def fn():
                gs.run(next(it))
                gs.run(next(it))
        else:
            fn = lambda: gs.run(next(it))  # noqa: E731
        res[n] = settled_regions(fn, inner, a.regions)
        gs.close()
        del gs, fn
    bt.set_precision("f32")
    emit("GraphedTrainStep, ResNet18 Flipout, batch 64, 224^2, bf16 contraction, hip_batchnorm, forward + loss + backward; ms:")
    emit("  two num_mc=1 replays (CE + KL / B, torch ops)        %8.3f (%.3f .. %.3f)" % tuple(v / 1e3 for v in res[1]))
    emit("  one num_mc=2 replay  (mc_elbo_loss, btx_mc_ce_*)     %8.3f (%.3f .. %.3f)" % tuple(v / 1e3 for v in res[2]))
    emit("  num_mc=2 replay / two single replays: %.3f" % (res[2][0] / res[1][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_loss_bench.txt"))
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--skip-train-step", action="store_true")
    a = ap.parse_args()
    assert a.regions >= 8, "the settled half needs at least 8 regions"
    assert torch.cuda.is_available(), "mc_loss_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/mc_loss_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; us per forward + backward: median (min .. max) of the settled half of %d back-to-back regions of %d "
         "calls" % (torch.cuda.get_device_name(0), torch.__version__, a.regions, a.inner))
    bench_heads(a, dev, emit)
    if not a.skip_train_step:
        bench_step(a, dev, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
