"""ms per training step (forward, cross-entropy + KL / batch loss, backward) of a Bayesian LSTM + Linear head converted by
dnn_to_bnn: the eager per-step loop, the fused training path (fuse_model(lstm_training=True): btx_lstm_fwd_train +
btx_lstm_bwd) issued eagerly, and the fused path replayed by autograd.GraphedTrainStep.

    python tools/lstm_train_bench.py [--types Flipout,Reparameterization] [--precs f32,bf16] [--I 256] [--H 512] [--B 64] [--T 64]

f32 activations; `prec` is the contraction precision.  Prints one JSON line per (type, precision)."""
import argparse
import gc
import json
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


class SeqNet(nn.Module):
    def __init__(self, i, h, classes=10):
        super().__init__()
        self.lstm = nn.LSTM(i, h)
        self.fc = nn.Linear(h, classes)

    def forward(self, x):
        out, _ = self.lstm(x)
        return self.fc(out[:, -1, :])


def _time(fn, n, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="Flipout,Reparameterization")
    ap.add_argument("--precs", default="f32,bf16")
    ap.add_argument("--I", type=int, default=256)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed region")
    a = ap.parse_args()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models import fuse_model
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    dev = torch.device("cuda:0")
    for typ in a.types.split(","):
        for prec in a.precs.split(","):
            bt.set_precision(prec)
            torch.manual_seed(0)
            m = SeqNet(a.I, a.H)
            bt.dnn_to_bnn(m, dict(PRIOR, type=typ))
            m = m.to(dev).train()
            x = torch.randn(a.B, a.T, a.I, device=dev)
            y = torch.randint(0, 10, (a.B,), device=dev)
            res = dict(type=typ, prec=prec, I=a.I, H=a.H, B=a.B, T=a.T)

            def step():
                for p in m.parameters():
                    p.grad = None
                loss = F.cross_entropy(m(x).float(), y) + get_kl_loss(m) / a.B
                loss.backward()
            res["eager_ms_per_step"] = round(_time(step, a.steps), 3)
            fuse_model(m, lstm_training=True)
            res["fused_eager_ms_per_step"] = round(_time(step, a.steps), 3)
            # GraphedTrainStep needs every autograd graph of the eager steps gone: a Flipout LSTM keeps its last KL (with its graph)
            # in `.kl`, as the reference does
            m.lstm.kl = None
            gc.collect()
            g = GraphedTrainStep(m, x, y)
            it = iter(range(1 << 30))
            res["fused_graphed_ms_per_step"] = round(_time(lambda: g.run(next(it)), a.steps * 2), 3)
            g.close()
            del g
            res["speedup_graphed_vs_eager"] = round(res["eager_ms_per_step"] / res["fused_graphed_ms_per_step"], 2)
            print(json.dumps(res), flush=True)
    bt.set_precision("f32")


if __name__ == "__main__":
    main()
