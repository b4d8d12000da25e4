"""GPU time of sparse variational dropout (BTX-SVD v1, csrc/btx_svd.hip) on dnn_to_bnn(ResNet18): 22 tensors, 11.7 M
elements.

    python tools/svd_bench.py [--out profiles/svd_bench.txt] [--regions 10] [--inner 20] [--skip-step] [--gauss-step-only]

  1. btx_kl_logu_model + btx_kl_logu_model_bwd ("mean" and "sum") and btx_kl_gauss_model + _bwd on the same tensors, each a hipGraph of
     one call, so the figure is device time and not the ctypes call.
  2. sparsity.stats (3 thresholds; without and with a 64-bin histogram) and sparsity.prune_(threshold=3) as the user calls them, host
     work and the one host read included, and their launches alone as hipGraphs.  prune_ is timed on a model it has already pruned:
     the pass reads every element and writes nothing.
  3. the captured batch-64 training step (Flipout, bf16 activations, forward + CE + KL / B + backward) with the Gaussian prior, with
     LogUniformPrior("sum"), and with the Gaussian prior again: the first and the last give the spread.
--gauss-step-only: the Gaussian-prior captured step alone, with its loss at sample 7 and the KL printed to 7 digits (what a run of the
parent commit is compared with).
There is no pass mark.  Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back replays form one region; `regions` regions
run back to back after a warm-up of the same shape; the figure is the median of the SECOND half of them with that half's range."""
import argparse
import gc
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

from klmc_bench import build  # noqa: E402
from mc_loss_bench import capture, settled_regions  # noqa: E402


def bench_kernels(model, a, dev, emit):
    from bayesian_torch_amd import autograd as AG, functional as BF, sparsity
    layers = [m for m in model.modules() if hasattr(m, "_btx_layer_id")]
    g = torch.ones((), device=dev)
    cell = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731
    pairs = [pr for layer in layers for pr in AG.kl_pairs(layer)]
    params = [t for mu, rho, _ in pairs for t in (mu, rho)]
    n_el = sum(mu.numel() for mu, _, _ in pairs)
    emit("%d tensors, %d elements; us per call, median (min .. max); GB/s = 8 B/element forward, 16 B/element backward" % (len(pairs), n_el))
    emit("%-34s | %26s %26s | %7s %7s" % ("KL", "forward", "backward", "fwd GB/s", "bwd GB/s"))
    ent = AG._entries(tuple(m for _, _, m in pairs), params)
    grads = [(torch.empty_like(e[0]), torch.empty_like(e[0])) for e in ent]
    fw = settled_regions(capture(lambda: BF.kl_model_hip(ent), dev).replay, a.inner, a.regions)
    bw = settled_regions(capture(lambda: BF.kl_model_bwd_hip(ent, grads, g), dev).replay, a.inner, a.regions)
    emit("%-34s | %s %s | %7.0f %7.0f" % ("Gaussian (btx_kl_gauss_model)", cell(fw), cell(bw), 8e-3 * n_el / fw[0], 16e-3 * n_el / bw[0]))
    for reduction in ("mean", "sum"):
        le = AG._logu_entries([reduction] * len(pairs), params)
        lg = [(torch.empty_like(e[0]), torch.empty_like(e[0])) for e in le]
        fw = settled_regions(capture(lambda: BF.kl_logu_model_hip(le), dev).replay, a.inner, a.regions)
        bw = settled_regions(capture(lambda: BF.kl_logu_model_bwd_hip(le, lg, g), dev).replay, a.inner, a.regions)
        emit("%-34s | %s %s | %7.0f %7.0f" % ("log-uniform %r (btx_kl_logu_model)" % reduction, cell(fw), cell(bw), 8e-3 * n_el / fw[0],
                                              16e-3 * n_el / bw[0]))
    # statistics and pruning: the launches alone, then the calls as the user makes them
    net_pairs = [(BF.dense_flat(mu), BF.dense_flat(rho)) for mu, rho, _ in pairs]
    th = (0.0, 3.0, 6.0)
    emit("%-52s | %26s | %7s" % ("statistics and pruning", "us per call", "GB/s"))
    for tag, fn in (("btx_logalpha_stats, 3 thresholds (graph)", lambda: BF.logalpha_stats_hip(net_pairs, th, 0)),
                    ("btx_logalpha_stats, 3 thresholds + 64 bins (graph)", lambda: BF.logalpha_stats_hip(net_pairs, th, 64)),
                    ("btx_logalpha_prune, nothing left to prune (graph)", lambda: BF.logalpha_prune_hip(net_pairs, 3.0))):
        if "prune" in tag:
            fn()  # the first call prunes; the timed ones read only
        r = settled_regions(capture(fn, dev).replay, a.inner, a.regions)
        emit("%-52s | %s | %7.0f" % (tag, cell(r), 8e-3 * n_el / r[0]))
    for tag, fn in (("sparsity.stats(model, 3 thresholds, bias too)", lambda: sparsity.stats(model, th, 0, include_bias=True)),
                    ("sparsity.stats(model, ..., bins=64)", lambda: sparsity.stats(model, th, 64, include_bias=True)),
                    ("sparsity.prune_(model, 3.0, bias too)", lambda: sparsity.prune_(model, 3.0, include_bias=True))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.regions):
            t0 = time.perf_counter()
            fn()  # ends in its host read
            ts.append((time.perf_counter() - t0) * 1e6)
        tail = sorted(ts[len(ts) // 2:])
        emit("%-52s | %s | %7s" % (tag + " wall", cell((tail[len(tail) // 2], tail[0], tail[-1])), "-"))


def _step(model, x, y, a):
    from bayesian_torch_amd.autograd import GraphedTrainStep
    for p in model.parameters():
        p.grad = None
    gs = GraphedTrainStep(model, x, y)
    it = [0]

    def run():
        it[0] += 1
        gs.run(it[0])
    r = settled_regions(run, a.step_inner, a.regions)
    loss7 = float(gs.run(7))
    gs.close()
    del gs
    gc.collect()
    torch.cuda.empty_cache()
    return r, loss7


def _batch(dev):
    torch.manual_seed(1234)
    return torch.randn(64, 3, 224, 224, device=dev).to(torch.bfloat16), torch.randint(0, 1000, (64,), device=dev)


def bench_step(a, dev, emit):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import models, priors as P
    model = build(dev)  # a fresh model: the kernel section pruned its own
    x, y = _batch(dev)
    emit("captured training step, ResNet18 Flipout batch 64 bf16: ms per replay, median (min .. max)")
    res = {}
    for tag, prior in (("Gaussian prior (first)", None), ("LogUniformPrior('sum')", P.LogUniformPrior("sum")), ("Gaussian prior (again)", None)):
        models.set_prior(model, prior)
        r, loss7 = _step(model, x, y, a)
        res[tag] = r
        emit("%-34s %8.3f (%7.3f ..%7.3f)   loss at sample 7 = %.7f, kl = %.7f" % (tag, r[0] / 1e3, r[1] / 1e3, r[2] / 1e3, loss7,
                                                                                float(bt.get_kl_loss(model).detach())))
    ga, gb, lu = res["Gaussian prior (first)"][0], res["Gaussian prior (again)"][0], res["LogUniformPrior('sum')"][0]
    emit("log-uniform KL against the Gaussian step: %+.2f %% (the two Gaussian runs differ by %.2f %%)" %
         (100 * (lu / (0.5 * (ga + gb)) - 1), 100 * abs(ga - gb) / (0.5 * (ga + gb))))


def gauss_step_only(a, dev, emit):
    import bayesian_torch_amd as bt
    model = build(dev)
    x, y = _batch(dev)
    r, loss7 = _step(model, x, y, a)
    emit("captured step ms/replay: median %.3f (min %.3f .. max %.3f); loss at sample 7 = %.7f, kl = %.7f"
         % (r[0] / 1e3, r[1] / 1e3, r[2] / 1e3, loss7, float(bt.get_kl_loss(model).detach())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_bench.txt"))
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step-inner", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--gauss-step-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svd_bench needs a GPU: there is no CPU figure to report")
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.gauss_step_only:
        gauss_step_only(a, dev, emit)
        return
    emit("tools/svd_bench.py on %s" % torch.cuda.get_device_name(0))
    bench_kernels(build(dev), a, dev, emit)
    if not a.skip_step:
        bench_step(a, dev, emit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
