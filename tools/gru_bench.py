"""GPU ms per MC sample of a Bayesian GRU + Linear head, converted by dnn_to_bnn: the fused sequence (fuse_model -> fused_sequence,
one btx_gru_fwd call: 1 + T launches) replayed by mc.GraphedMC with 1 and 8 MC samples per replay (lane_mode "launch"), against the
eager per-step loop of the same build — the only other route — issued from Python (its device word cannot be pinned, so it cannot be
captured: its figure includes the gaps between its launches, which is what a user of that route waits for).

    python tools/gru_bench.py [--types Flipout,Reparameterization] [--precs f32,bf16] [--shapes 256x512x64x64,32x64x8x16] [--out FILE]

Every figure is device time between two events around a region of back-to-back calls, divided by the MC samples in the region: the
median over the settled (second) half of `--regions` regions, with that half's spread (max - min) / median.  f32 activations;
`prec` is the contraction precision.  Prints one JSON line per row and writes the table to --out.

    python tools/gru_bench.py --train [--types ...] [--precs ...] [--shapes 256x512x64x64] [--out FILE]

--train times one training step instead (forward + cross-entropy + KL + backward), ms per step: the eager per-step
loop differentiated op by op, the fused training path (fuse_model(gru_training=True): btx_gru_fwd_train + btx_gru_bwd) issued from
Python, and the same fused step replayed by autograd.GraphedTrainStep.  The three alternate inside every region."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


class SeqNet(nn.Module):
    def __init__(self, i, h, classes=10):
        super().__init__()
        self.gru = nn.GRU(i, h, batch_first=True)
        self.fc = nn.Linear(h, classes)

    def forward(self, x):
        out, _ = self.gru(x)
        return self.fc(out[:, -1, :])


def _regions(fn, calls, regions, samples_per_call):
    """(median ms per sample over the settled half, its spread) of `regions` regions of `calls` calls each"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / (calls * samples_per_call))
    half = ms[len(ms) // 2:]
    med = statistics.median(half)
    return med, (max(half) - min(half)) / med


def _train_rows(a, bt, dev):
    """the --train table: ms per training step of the three routes, timed in alternation (one region of each per round)"""
    import torch.nn.functional as F
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models import fuse_model
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    lines = ["%-19s %-5s %-16s %13s %8s %13s %8s %13s %8s %9s %9s" % (
        "type", "prec", "I x H x B x T", "eager ms", "spread", "fused ms", "spread", "graphed ms", "spread", "fused x", "graphed x")]
    for shape in a.shapes.split(","):
        I, H, B, T = (int(v) for v in shape.split("x"))
        for typ in a.types.split(","):
            for prec in a.precs.split(","):
                bt.set_precision(prec)
                x = torch.randn(B, T, I, device=dev)
                y = torch.randint(0, 10, (B,), device=dev)
                models = []
                for fused in (False, True, True):
                    torch.manual_seed(0)
                    m = SeqNet(I, H)
                    bt.dnn_to_bnn(m, dict(PRIOR, type=typ))
                    m = m.to(dev).train()
                    if fused:
                        fuse_model(m, gru_training=True)
                    models.append(m)

                def step(m, count=[0]):
                    count[0] += 1
                    for p in m.parameters():
                        p.grad = None
                    bt.set_sample_index(m, count[0] * T)
                    loss = F.cross_entropy(m(x).float(), y) + get_kl_loss(m) / B
                    loss.backward()
                g = GraphedTrainStep(models[2], x, y)
                fns = dict(eager=lambda: step(models[0]), fused=lambda: step(models[1]), graphed=lambda: g.run(7))
                ms = {k: [] for k in fns}
                for k, fn in fns.items():  # warm-up of every route at this shape
                    fn()
                torch.cuda.synchronize()
                for _ in range(a.regions):
                    for k, fn in fns.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.calls):
                            fn()
                        e1.record()
                        e1.synchronize()
                        ms[k].append(e0.elapsed_time(e1) / a.calls)
                g.close()
                res = dict(mode="train", type=typ, prec=prec, I=I, H=H, B=B, T=T)
                for k, v in ms.items():
                    half = v[len(v) // 2:]
                    res[k + "_ms"] = statistics.median(half)
                    res[k + "_spread"] = (max(half) - min(half)) / res[k + "_ms"]
                res["speedup_fused"] = res["eager_ms"] / res["fused_ms"]
                res["speedup_graphed"] = res["eager_ms"] / res["graphed_ms"]
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
                lines.append("%-19s %-5s %-16s %13.4f %7.1f%% %13.4f %7.1f%% %13.4f %7.1f%% %8.2fx %8.2fx" % (
                    typ, prec, "%d x %d x %d x %d" % (I, H, B, T), res["eager_ms"], 100 * res["eager_spread"], res["fused_ms"],
                    100 * res["fused_spread"], res["graphed_ms"], 100 * res["graphed_spread"], res["speedup_fused"],
                    res["speedup_graphed"]))
    bt.set_precision("f32")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/gru_bench.py --train on an MI355X: device ms per training step (forward + loss + backward; events around regions\n"
                    "of %d back-to-back steps, the three routes alternating; median of the settled half of %d regions, spread = (max - min) /\n"
                    "median of that half).  eager = the per-step loop differentiated op by op; fused = fused_training issued from Python;\n"
                    "graphed = the fused step replayed by autograd.GraphedTrainStep; x = eager / that route.\n\n" % (a.calls, a.regions))
            f.write(table + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time a training step (forward + backward) instead of MC inference")
    ap.add_argument("--calls", type=int, default=8, help="--train: steps per timed region")
    ap.add_argument("--types", default="Flipout,Reparameterization")
    ap.add_argument("--precs", default="f32,bf16")
    ap.add_argument("--shapes", default="256x512x64x64,32x64x8x16", help="IxHxBxT, comma separated")
    ap.add_argument("--regions", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.models import fuse_model
    if not torch.cuda.is_available():
        raise SystemExit("gru_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    if a.train:
        return _train_rows(a, bt, dev)
    lines = ["%-19s %-5s %-16s %14s %8s %14s %8s %14s %8s %9s %9s" % (
        "type", "prec", "I x H x B x T", "eager ms/smp", "spread", "fused L1 ms", "spread", "fused L8 ms", "spread", "L1 x", "L8 x")]
    for shape in a.shapes.split(","):
        I, H, B, T = (int(v) for v in shape.split("x"))
        for typ in a.types.split(","):
            for prec in a.precs.split(","):
                bt.set_precision(prec)
                torch.manual_seed(0)
                m = SeqNet(I, H)
                bt.dnn_to_bnn(m, dict(PRIOR, type=typ))
                m = m.to(dev).eval()
                x = torch.randn(B, T, I, device=dev)

                def eager():
                    with torch.no_grad():
                        m(x)
                res = dict(type=typ, prec=prec, I=I, H=H, B=B, T=T)
                res["eager_ms"], res["eager_spread"] = _regions(eager, 2, a.regions, 1)
                fuse_model(m)
                for lanes in (1, 8):
                    g = mc.GraphedMC(m, x.clone(), lanes=lanes, lane_mode="launch")
                    fn = (lambda: g.run(0)) if lanes == 1 else (lambda: g.run_many(list(range(lanes))))
                    res["fused_l%d_ms" % lanes], res["fused_l%d_spread" % lanes] = _regions(fn, 8 if lanes == 1 else 2, a.regions, lanes)
                    g.close()
                    del g
                res["speedup_l1"] = res["eager_ms"] / res["fused_l1_ms"]
                res["speedup_l8"] = res["eager_ms"] / res["fused_l8_ms"]
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
                lines.append("%-19s %-5s %-16s %14.4f %7.1f%% %14.4f %7.1f%% %14.4f %7.1f%% %8.2fx %8.2fx" % (
                    typ, prec, "%d x %d x %d x %d" % (I, H, B, T), res["eager_ms"], 100 * res["eager_spread"], res["fused_l1_ms"],
                    100 * res["fused_l1_spread"], res["fused_l8_ms"], 100 * res["fused_l8_spread"], res["speedup_l1"], res["speedup_l8"]))
    bt.set_precision("f32")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/gru_bench.py on an MI355X: device ms per MC sample (events around regions of back-to-back calls; median of the\n"
                    "settled half of %d regions, spread = (max - min) / median of that half).  eager = the per-step loop issued from Python;\n"
                    "fused L1 / L8 = the fused sequence replayed by mc.GraphedMC with 1 / 8 lanes; x = eager / fused.\n\n" % a.regions)
            f.write(table + "\n")


if __name__ == "__main__":
    main()
