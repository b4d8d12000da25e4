"""GPU time of the fused attention core (btx_attn_fwd) against the other routes of the same build, and of a whole
converted nn.TransformerEncoderLayer forward with and without it.

    python tools/attn_bench.py [--regions 10] [--calls 20] [--out profiles/attn_bench.txt]

Core: every route is captured into a graph of its own and the routes ALTERNATE inside every round; a figure is device time between two
events around `--calls` back-to-back replays, per replay: the median over the settled (second) half of `--regions` rounds, with that
half's spread (max - min) / median.
  fused      functional.attn_hip on the packed in-projection output [rows, T, 3E]: q, k, v read in place, [rows, T, E] written
  composite  the layer's eager core on the same tensor: head split, QK^T, softmax, PV, merge (transposes included)
  sdpa       F.scaled_dot_product_attention fed pre-transposed contiguous [rows, heads, T, D] heads (no transposes counted)
TFLOP/s = 4 rows heads Tq Tk D (half of it under the causal mask) over the fused time; "of peak" is that rate over the 2500 TFLOP/s
dense bf16 MFMA peak of an MI355X (printed for the bf16 rows only).
Layer: mc.GraphedMC replays (one MC sample each) of embed -> converted TransformerEncoderLayer -> first token -> head, the model fused by
fuse_model against the same model unfused, alternating.

    python tools/attn_bench.py --train [--out profiles/attn_train_bench.txt]

Training: forward plus backward of the core, each route captured with its backward (torch.autograd.grad at a fixed
d_out) — fused = autograd.AttnFn (btx_attn_fwd_train + btx_attn_bwd), composite = the layer's eager core under autograd, sdpa =
F.scaled_dot_product_attention — and one whole training step (autograd.GraphedTrainStep: forward, loss, backward) of the layer model,
fuse_model(m, attn_training=True) against fuse_model(m).  The saved-activation bytes of the core are derived, not measured."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
BF16_PEAK = 2500e12
# (name, rows, T, heads, D, causal)
SHAPES = [("vit-b", 64, 197, 12, 64, False), ("vit-b x8 lanes", 512, 197, 12, 64, False), ("T1024 D64", 8, 1024, 12, 64, False),
          ("T1024 D128", 8, 1024, 8, 128, False), ("T1024 D64 causal", 8, 1024, 12, 64, True)]


def _alternate(fns, calls, regions):
    """{name: (median ms per call over the settled half, spread)} with the routes alternating inside every round"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(regions):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    out = {}
    for k, v in ms.items():
        half = v[len(v) // 2:]
        med = statistics.median(half)
        out[k] = (med, (max(half) - min(half)) / med)
    return out


def _graphed(fn, grad=False):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.set_grad_enabled(grad):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.set_grad_enabled(grad):
        fn()
    return g.replay


class Net(nn.Module):
    def __init__(self, e, heads, ff):
        super().__init__()
        self.embed = nn.Linear(e, e)
        self.enc = nn.TransformerEncoderLayer(e, heads, ff, dropout=0.0, batch_first=True)
        self.head = nn.Linear(e, 10)

    def forward(self, x):
        return self.head(self.enc(self.embed(x))[:, 0])


def train(a):
    """the training mode: forward + backward of the core per route, then one captured training step of the layer model"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import autograd as ag, layers as L
    from bayesian_torch_amd.models import fuse_model
    dev = torch.device("cuda:0")
    lines = ["%-17s %-5s %11s %7s %13s %7s %10s %7s %9s %8s" % (
        "core fwd + bwd", "dtype", "fused ms", "spread", "composite ms", "spread", "sdpa ms", "spread", "comp / f", "sdpa / f")]
    for name, R, T, H, D, causal in SHAPES:
        for dt, prec in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            torch.manual_seed(0)
            layer = L.MultiheadAttentionReparameterization(H * D, H, batch_first=True)
            qkv = (0.5 * torch.randn(R, T, 3 * H * D, device=dev)).to(dt).requires_grad_()
            d_out = torch.randn(R, T, H * D, device=dev).to(dt)
            heads = [t.detach().reshape(R, T, H, D).transpose(1, 2).contiguous().requires_grad_() for t in qkv.chunk(3, dim=-1)]
            d_heads = d_out.reshape(R, T, H, D).transpose(1, 2).contiguous()
            G = torch.autograd.grad
            fns = dict(fused=_graphed(lambda: G(ag.AttnFn.apply((H, None, causal, prec), qkv), qkv, d_out), True),
                       composite=_graphed(lambda: G(layer._core(qkv, None, False, None, True, causal)[0], qkv, d_out), True),
                       sdpa=_graphed(lambda: G(F.scaled_dot_product_attention(*heads, is_causal=causal), heads, d_heads), True))
            r = _alternate(fns, a.calls, a.regions)
            res = dict(core=name, dtype=prec, rows=R, T=T, heads=H, D=D, causal=causal, mode="train")
            for k, (med, spr) in r.items():
                res[k + "_ms"], res[k + "_spread"] = med, spr
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
            lines.append("%-17s %-5s %11.4f %6.1f%% %13.4f %6.1f%% %10.4f %6.1f%% %8.2fx %7.2fx" % (
                name, prec, r["fused"][0], 100 * r["fused"][1], r["composite"][0], 100 * r["composite"][1], r["sdpa"][0],
                100 * r["sdpa"][1], r["composite"][0] / r["fused"][0], r["sdpa"][0] / r["fused"][0]))
            del fns
    lines.append("")
    lines.append("%-34s %-5s %11s %7s %13s %7s %9s" % ("training step (embed, layer, head)", "prec", "fused ms", "spread", "unfused ms", "spread", "unf / f"))
    B, T, E, H, FF = 64, 197, 768, 12, 3072
    for kind in ("Reparameterization", "Flipout"):
        for prec in ("bf16", "f32"):
            bt.set_precision(prec)
            x, y = torch.randn(B, T, E, device=dev), torch.randint(0, 10, (B,), device=dev)
            steps = {}
            for route in ("fused", "unfused"):
                torch.manual_seed(0)
                m = Net(E, H, FF)
                bt.dnn_to_bnn(m, dict(PRIOR, type=kind))
                m = m.to(dev).train()
                fuse_model(m, attn_training=route == "fused")
                steps[route] = ag.GraphedTrainStep(m, x.clone(), y)
            r = _alternate({k: (lambda g=g: g.run(0)) for k, g in steps.items()}, max(2, a.calls // 4), a.regions)
            for g in steps.values():
                g.close()
            print(json.dumps(dict(layer="vit-b", type=kind, prec=prec, mode="train", fused_ms=round(r["fused"][0], 5),
                                  unfused_ms=round(r["unfused"][0], 5))), flush=True)
            lines.append("%-34s %-5s %11.4f %6.1f%% %13.4f %6.1f%% %8.2fx" % (
                "vit-b 64 x 197 x 768 " + kind[:7], prec, r["fused"][0], 100 * r["fused"][1], r["unfused"][0], 100 * r["unfused"][1],
                r["unfused"][0] / r["fused"][0]))
    bt.set_precision("f32")
    # derived: what the core keeps for its backward beside qkv and out — fused: lse [rows, heads, T] f32 (the backward's delta plane of the
    # same size is transient); composite under autograd: the f32 scores and probabilities [rows, heads, T, T] (softmax keeps its output,
    # the two masked_fill nodes a bool mask each) and the head-major f32 copies of q, k, v
    R, T, H, D = SHAPES[0][1:5]
    lines += ["", "saved by the core for vit-b (derived): fused %d bytes (+ %d transient in the backward); composite >= %d bytes" % (
        R * H * T * 4, R * H * T * 4, R * H * T * T * (4 + 4 + 1) + 3 * R * H * T * D * 4)]
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/attn_bench.py --train on an MI355X: device ms per captured replay of forward + backward (events around %d back-to-back\n"
                    "replays, the routes alternating inside every round; median of the settled half of %d rounds, spread = (max - min) /\n"
                    "median of that half).  fused = autograd.AttnFn; composite = the layer's eager core under autograd; sdpa =\n"
                    "F.scaled_dot_product_attention on pre-transposed contiguous heads; x = that route / fused.\n\n" % (a.calls, a.regions))
            f.write(table + "\n")


def bias(a):
    """--bias: the core under an additive mask — fused with the bias, the composite on the same mask (what these inputs
    took before the bias variant existed), and the fused core without a bias at the same shape (the variant's overhead); forward
    (eval) and forward + backward (train) per shape class.  pad_float: a [rows, T] float key-padding mask, a quarter of every row's
    keys padded; tt: a float [T, T] window of +-T/4; htt: a float bias DISTINCT per (row, head), given as [rows * heads, T, T] — the
    variant's worst case, every element streamed once (a shared relative-position bias [heads, T, T] would be read with row stride 0)."""
    from bayesian_torch_amd import autograd as ag, functional as BF, layers as L
    dev = torch.device("cuda:0")
    lines = ["--bias %s" % a.bias, "%-17s %-5s %-5s %11s %7s %13s %7s %11s %7s %9s %9s" % (
        "core", "dtype", "mode", "bias ms", "spread", "composite ms", "spread", "no-bias ms", "spread", "comp / b", "b / no-b")]
    for name, R, T, H, D, causal in SHAPES:
        if causal:
            continue  # the causal flag needs no bias
        for dt, prec in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            torch.manual_seed(0)
            layer = L.MultiheadAttentionReparameterization(H * D, H, batch_first=True)
            qkv = (0.5 * torch.randn(R, T, 3 * H * D, device=dev)).to(dt).requires_grad_()
            d_out = torch.randn(R, T, H * D, device=dev).to(dt)
            kp = am = None
            if a.bias == "pad_float":
                kp = torch.zeros(R, T, device=dev, dtype=dt).masked_fill(torch.arange(T, device=dev)[None, :] >= T - T // 4, float("-inf"))
            elif a.bias == "tt":
                idx = torch.arange(T, device=dev)
                am = torch.zeros(T, T, device=dev, dtype=dt).masked_fill((idx[:, None] - idx[None, :]).abs() > T // 4, float("-inf"))
            else:
                am = torch.randn(R * H, T, T, device=dev).to(dt)   # [rows * heads, T, T], as nn.MultiheadAttention takes it
            kpb, _, b = layer._fused_masks(kp, am, False)
            G = torch.autograd.grad
            for mode in ("eval", "train"):
                if mode == "eval":
                    fns = dict(bias=_graphed(lambda: BF.attn_hip(qkv.detach(), H, kpb, prec=prec, bias=b)),
                               composite=_graphed(lambda: layer._core(qkv.detach(), kp, False, am, True, False)),
                               nobias=_graphed(lambda: BF.attn_hip(qkv.detach(), H, prec=prec)))
                else:
                    fns = dict(bias=_graphed(lambda: G(ag.AttnFn.apply((H, kpb, False, prec, b), qkv), qkv, d_out), True),
                               composite=_graphed(lambda: G(layer._core(qkv, kp, False, am, True, False)[0], qkv, d_out), True),
                               nobias=_graphed(lambda: G(ag.AttnFn.apply((H, None, False, prec), qkv), qkv, d_out), True))
                r = _alternate(fns, a.calls, a.regions)
                print(json.dumps(dict(core=name, dtype=prec, mode=mode, bias=a.bias, **{k + "_ms": round(v[0], 5) for k, v in r.items()})), flush=True)
                lines.append("%-17s %-5s %-5s %11.4f %6.1f%% %13.4f %6.1f%% %11.4f %6.1f%% %8.2fx %8.2fx" % (
                    name, prec, mode, r["bias"][0], 100 * r["bias"][1], r["composite"][0], 100 * r["composite"][1], r["nobias"][0],
                    100 * r["nobias"][1], r["composite"][0] / r["bias"][0], r["bias"][0] / r["nobias"][0]))
                del fns
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(table + "\n\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true", help="time forward + backward (DESIGN.md section 31) instead of the inference forward")
    ap.add_argument("--bias", choices=("none", "pad_float", "tt", "htt"), default="none",
                    help="time the core under an additive mask (DESIGN.md section 32): appended to --out")
    a = ap.parse_args()
    if a.bias != "none":
        if not torch.cuda.is_available():
            raise SystemExit("attn_bench needs a GPU: nothing is measured without one")
        return bias(a)
    if a.train:
        if not torch.cuda.is_available():
            raise SystemExit("attn_bench needs a GPU: nothing is measured without one")
        return train(a)
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF, layers as L, mc
    from bayesian_torch_amd.models import fuse_model
    if not torch.cuda.is_available():
        raise SystemExit("attn_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = ["%-17s %-5s %11s %7s %13s %7s %10s %7s %9s %8s %8s %8s" % (
        "core", "dtype", "fused ms", "spread", "composite ms", "spread", "sdpa ms", "spread", "comp / f", "sdpa / f", "TFLOP/s", "of peak")]
    for name, R, T, H, D, causal in SHAPES:
        for dt, prec in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            torch.manual_seed(0)
            layer = L.MultiheadAttentionReparameterization(H * D, H, batch_first=True)
            qkv = (0.5 * torch.randn(R, T, 3 * H * D, device=dev)).to(dt)
            heads = [t.reshape(R, T, H, D).transpose(1, 2).contiguous() for t in qkv.chunk(3, dim=-1)]
            fns = dict(fused=_graphed(lambda: BF.attn_hip(qkv, H, causal=causal, prec=prec)),
                       composite=_graphed(lambda: layer._core(qkv, None, False, None, True, causal)),
                       sdpa=_graphed(lambda: F.scaled_dot_product_attention(*heads, is_causal=causal)))
            r = _alternate(fns, a.calls, a.regions)
            flops = 4.0 * R * H * T * T * D * (0.5 if causal else 1.0)
            tf = flops / (r["fused"][0] * 1e-3) / 1e12
            res = dict(core=name, dtype=prec, rows=R, T=T, heads=H, D=D, causal=causal, tflops=tf)
            for k, (med, spr) in r.items():
                res[k + "_ms"], res[k + "_spread"] = med, spr
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
            lines.append("%-17s %-5s %11.4f %6.1f%% %13.4f %6.1f%% %10.4f %6.1f%% %8.2fx %7.2fx %8.1f %8s" % (
                name, prec, r["fused"][0], 100 * r["fused"][1], r["composite"][0], 100 * r["composite"][1], r["sdpa"][0],
                100 * r["sdpa"][1], r["composite"][0] / r["fused"][0], r["sdpa"][0] / r["fused"][0], tf,
                "%.1f%%" % (100 * tf * 1e12 / BF16_PEAK) if prec == "bf16" else "-"))
            del fns
    lines.append("")
    lines.append("%-34s %-5s %11s %7s %13s %7s %9s" % ("layer (embed, encoder layer, head)", "prec", "fused ms", "spread", "unfused ms", "spread", "unf / f"))
    for name, B, T, E, H, FF in (("vit-b 64 x 197 x 768", 64, 197, 768, 12, 3072),):
        for kind in ("Reparameterization", "Flipout"):
            for prec in ("bf16", "f32"):
                bt.set_precision(prec)
                x = torch.randn(B, T, E, device=dev)
                graphs = {}
                for route in ("fused", "unfused"):
                    torch.manual_seed(0)
                    m = Net(E, H, FF)
                    bt.dnn_to_bnn(m, dict(PRIOR, type=kind))
                    m = m.to(dev).eval()
                    if route == "fused":
                        fuse_model(m)
                    graphs[route] = mc.GraphedMC(m, x.clone(), lanes=1)
                r = _alternate({k: (lambda g=g: g.run(0)) for k, g in graphs.items()}, max(2, a.calls // 4), a.regions)
                for g in graphs.values():
                    g.close()
                res = dict(layer=name, type=kind, prec=prec)
                for k, (med, spr) in r.items():
                    res[k + "_ms"], res[k + "_spread"] = med, spr
                print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)
                lines.append("%-34s %-5s %11.4f %6.1f%% %13.4f %6.1f%% %8.2fx" % (
                    name + " " + kind[:7], prec, r["fused"][0], 100 * r["fused"][1], r["unfused"][0], 100 * r["unfused"][1],
                    r["unfused"][0] / r["fused"][0]))
    bt.set_precision("f32")
    table = "\n".join(lines)
    print(table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/attn_bench.py on an MI355X: device ms per captured replay (events around %d back-to-back replays, the routes\n"
                    "alternating inside every round; median of the settled half of %d rounds, spread = (max - min) / median of that half).\n"
                    "fused = btx_attn_fwd on the packed projection output; composite = the layer's eager core (transposes included); sdpa =\n"
                    "F.scaled_dot_product_attention on pre-transposed contiguous heads; x = that route / fused.  TFLOP/s = 4 rows heads T^2 D\n"
                    "(half under the causal mask) over the fused time; of peak = over the 2500 TFLOP/s dense bf16 MFMA peak.\n\n" % (a.calls, a.regions))
            f.write(table + "\n")


if __name__ == "__main__":
    main()
