"""ms per MC sample of a Bayesian LSTM + Linear head, converted by dnn_to_bnn: the eager per-step loop, the fused sequence
(fuse_model -> fused_sequence, one btx_lstm_fwd call: 1 + T launches) issued eagerly, and the fused sequence replayed by
mc.GraphedMC with 1 and 8 MC samples per replay (lane_mode "launch").

    python tools/lstm_bench.py [--types Flipout,Reparameterization] [--precs f32,bf16] [--I 256] [--H 512] [--B 64] [--T 64]

f32 activations; `prec` is the contraction precision (bf16: bf16 operands, f32 accumulation).  Prints one JSON line per
(type, precision)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

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
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="Flipout,Reparameterization")
    ap.add_argument("--precs", default="f32,bf16")
    ap.add_argument("--I", type=int, default=256)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--samples", type=int, default=8, help="MC samples per timed region")
    a = ap.parse_args()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.models import fuse_model
    dev = torch.device("cuda:0")
    for typ in a.types.split(","):
        for prec in a.precs.split(","):
            bt.set_precision(prec)
            torch.manual_seed(0)
            m = SeqNet(a.I, a.H)
            bt.dnn_to_bnn(m, dict(PRIOR, type=typ))
            m = m.to(dev).eval()
            x = torch.randn(a.B, a.T, a.I, device=dev)
            res = dict(type=typ, prec=prec, I=a.I, H=a.H, B=a.B, T=a.T)
            S = a.samples

            def eager():
                with torch.no_grad():
                    m(x)
            res["eager_ms_per_sample"] = round(_time(eager, S) / S, 4)
            fuse_model(m)
            res["fused_eager_ms_per_sample"] = round(_time(eager, S) / S, 4)
            for lanes in (1, 8):
                g = mc.GraphedMC(m, x.clone(), lanes=lanes, lane_mode="launch")
                if lanes == 1:
                    fn = lambda: g.run(0)  # noqa: E731
                else:
                    fn = lambda: g.run_many(list(range(lanes)))  # noqa: E731
                reps = max(1, S // lanes) * (2 if lanes == 1 else 4)
                res["graphed_lanes%d_ms_per_sample" % lanes] = round(_time(fn, reps) / (reps * lanes), 4)
                g.close()
                del g
            res["speedup_graphed_lanes1_vs_eager"] = round(res["eager_ms_per_sample"] / res["graphed_lanes1_ms_per_sample"], 2)
            res["speedup_graphed_lanes8_vs_eager"] = round(res["eager_ms_per_sample"] / res["graphed_lanes8_ms_per_sample"], 2)
            print(json.dumps(res), flush=True)
    bt.set_precision("f32")


if __name__ == "__main__":
    main()
