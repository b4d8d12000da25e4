"""GPU time of the sampled KL (BTX-KLMC v1, csrc/btx_klmc.hip) on dnn_to_bnn(ResNet18): 22 tensors, 11.7 M elements.

    python tools/klmc_bench.py [--out profiles/klmc_bench.txt] [--regions 10] [--inner 20] [--skip-step]

  1. btx_kl_mc_model + btx_kl_mc_model_bwd per prior and S in {1, 4}, and btx_kl_gauss_model + _bwd on the same tensors: a hipGraph of
     one forward and one backward, so the figure is device time and not the ctypes call.
  2. the captured batch-64 training step (Flipout, bf16 activations, forward + CE + KL / B + backward) with the Gaussian prior, with
     ScaleMixturePrior(0.25, 1, 0.05) at kl_samples = 1, and with the Gaussian prior again: the first and the last give the spread.
There is no pass mark.  Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back replays form one region; `regions` regions
run back to back after a warm-up of the same shape; the figure is the median of the SECOND half of them with that half's range."""
import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

from mc_loss_bench import capture, settled_regions  # noqa: E402

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def build(dev):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    bt.manual_seed(2024)
    bt.set_precision("bf16")
    torch.manual_seed(0)
    m = resnet.resnet18()
    bt.dnn_to_bnn(m, dict(PRIOR, type="Flipout"))
    m = m.to(dev).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.to(torch.bfloat16)
    bt.assign_layer_ids(m)
    hip_batchnorm(m)
    return m


def bench_kernels(model, a, dev, emit):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import autograd as AG, functional as BF, models, priors as P, rng
    layers = [m for m in model.modules() if hasattr(m, "_btx_layer_id")]
    g = torch.ones((), device=dev)
    cell = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731
    pairs = [pr for layer in layers for pr in AG.kl_pairs(layer)]
    params = [t for mu, rho, _ in pairs for t in (mu, rho)]
    n_el = sum(mu.numel() for mu, _, _ in pairs)
    emit("%d tensors, %d elements; us per call, median (min .. max)" % (len(pairs), n_el))
    emit("%-34s %2s | %26s %26s | %9s" % ("prior", "S", "forward", "backward", "Gelem*S/s"))
    ent = AG._entries(tuple(m for _, _, m in pairs), params)
    grads = [(torch.empty_like(e[0]), torch.empty_like(e[0])) for e in ent]
    fw = settled_regions(capture(lambda: BF.kl_model_hip(ent), dev).replay, a.inner, a.regions)
    bw = settled_regions(capture(lambda: BF.kl_model_bwd_hip(ent, grads, g), dev).replay, a.inner, a.regions)
    emit("%-34s %2s | %s %s | %9s" % ("Gaussian (btx_kl_gauss_model)", "-", cell(fw), cell(bw), "-"))
    for prior in (P.ScaleMixturePrior(0.25, 1.0, 0.05), P.LaplacePrior(0.3), P.StudentTPrior(3.0, 0.2)):
        for S in (1, 4):
            models.set_prior(model, prior, kl_samples=S)
            mp = [pr for layer in layers for pr in AG.kl_mc_pairs(layer)]
            me = AG._mc_entries(tuple(m for _, _, m in mp), [t for mu, rho, _ in mp for t in (mu, rho)])
            mg = [(torch.empty_like(e[0]), torch.empty_like(e[0])) for e in me]
            fw = settled_regions(capture(lambda: BF.kl_mc_model_hip(me, rng.seed(), S), dev).replay, a.inner, a.regions)
            bw = settled_regions(capture(lambda: BF.kl_mc_model_bwd_hip(me, mg, rng.seed(), S, g), dev).replay, a.inner, a.regions)
            emit("%-34s %2d | %s %s | %9.1f" % (repr(prior)[:34], S, cell(fw), cell(bw), n_el * S / (fw[0] + bw[0]) * 2e-3))
    models.set_prior(model, None)
    bt.set_sample_index(model, 0)


def bench_step(model, a, dev, emit):
    from bayesian_torch_amd import models, priors as P
    from bayesian_torch_amd.autograd import GraphedTrainStep
    torch.manual_seed(1234)
    x = torch.randn(64, 3, 224, 224, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 1000, (64,), device=dev)
    emit("captured training step, ResNet18 Flipout batch 64 bf16: ms per replay, median (min .. max)")
    res = {}
    for tag, prior in (("Gaussian prior (first)", None), ("ScaleMixturePrior, kl_samples=1", P.ScaleMixturePrior(0.25, 1.0, 0.05)),
                       ("Gaussian prior (again)", None)):
        models.set_prior(model, prior)
        for p in model.parameters():
            p.grad = None
        gs = GraphedTrainStep(model, x, y)
        it = [0]

        def run():
            it[0] += 1
            gs.run(it[0])
        r = settled_regions(run, a.step_inner, a.regions)
        gs.close()
        del gs
        gc.collect()
        torch.cuda.empty_cache()
        res[tag] = r
        emit("%-34s %8.3f (%7.3f ..%7.3f)" % (tag, r[0] / 1e3, r[1] / 1e3, r[2] / 1e3))
    ga, gb, mx = res["Gaussian prior (first)"][0], res["Gaussian prior (again)"][0], res["ScaleMixturePrior, kl_samples=1"][0]
    emit("sampled KL against the Gaussian step: %+.2f %% (the two Gaussian runs differ by %.2f %%)" %
         (100 * (mx / (0.5 * (ga + gb)) - 1), 100 * abs(ga - gb) / (0.5 * (ga + gb))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klmc_bench.txt"))
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step-inner", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("klmc_bench needs a GPU: there is no CPU figure to report")
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("tools/klmc_bench.py on %s" % torch.cuda.get_device_name(0))
    model = build(dev)
    bench_kernels(model, a, dev, emit)
    if not a.skip_step:
        bench_step(model, a, dev, emit)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
