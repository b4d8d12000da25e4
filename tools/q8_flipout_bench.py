"""GPU time of the INT8 Flipout path (btx_q8_sample_delta + btx_q8_contract_flipout: the delta pre-pass and ONE contraction launch
with two accumulator sets) per layer, beside the bf16 Flipout layer and the INT8 Reparameterization twin at the same shapes: the
convolutions of ResNet18 at batch 64, 224 x 224 and its 512 -> 1000 head.  Then the whole network: a Flipout models.QResNet
against the bf16 Flipout ResNet18 after fuse_model.

    python tools/q8_flipout_bench.py [--out profiles/q8_flipout_bench.txt] [--repeats 20] [--inner 10] [--batch 64] [--no-net]

Method of tools/q8_bench.py: every forward is captured into a graph once (GPU time, not the host's launch work), HIP events bracket
`inner` replays after a warm-up, the figure is the median over `repeats` windows with min and max beside it; the bf16 column is
measured before and after the int8 ones and keeps the better run.  The INT8 layers get an already quantized uint8 carrier.  No
threshold: what comes out is recorded, an int8 path slower than the bf16 one included.  (The reference's own form of this layer,
six quantized torch ops, has no GPU form at all.)"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from q8_bench import CONVS, capture, windows  # noqa: E402

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def cell(r):
    return "%8.1f (%7.1f ..%8.1f)" % r


def best(a, b):
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]))


def twin_of(src, flipout):
    from bayesian_torch_amd.models import bnn_to_qbnn
    wrap = torch.nn.Module()
    wrap.l = src
    bnn_to_qbnn(wrap, flipout=flipout)
    return wrap.l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "q8_flipout_bench.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-net", action="store_true")
    a = ap.parse_args()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd import q8
    from bayesian_torch_amd.models import fuse_model, resnet, to_qresnet
    assert torch.cuda.is_available(), "q8_flipout_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    bt.manual_seed(2024)
    bt.set_precision("bf16")
    torch.manual_seed(0)
    B = a.batch
    lines = ["python tools/q8_flipout_bench.py --repeats %d --inner %d --batch %d%s" % (a.repeats, a.inner, a.batch, " --no-net" if a.no_net else ""),
             "device: %s; batch %d; us of GPU time per layer forward (graph replay), median (min .. max) of %d windows of %d" % (
                 torch.cuda.get_device_name(0), B, a.repeats, a.inner)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say("%-13s %-21s %2s | %27s | %27s | %27s | %9s | %9s | %6s" % ("layer", "shape", "x", "bf16 Flipout", "int8 Flipout (pre-pass + 1)",
                                                                 "int8 Reparameterization", "i8F/bf16F", "i8F/i8R", "TOPS"))
    tot = [0.0, 0.0, 0.0]
    cases = [(n, "conv", c) for n, *c in CONVS] + [("head", "linear", (512, 1000))]
    for name, kind, c in cases:
        if kind == "conv":
            cin, cout, k, s, p, hw, times = c
            mk = lambda cls: getattr(L, "Conv2d" + cls)(cin, cout, k, stride=s, padding=p, bias=False).to(dev).eval()  # noqa: E731
            x = torch.randn(B, cin, hw, hw, device=dev)
            xf = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            ho = (hw + 2 * p - k) // s + 1
            macs = B * ho * ho * cout * cin * k * k
            shape = "%d->%d %dx%d/%d @%d" % (cin, cout, k, k, s, hw)
        else:
            cin, cout = c
            times = 1
            mk = lambda cls: getattr(L, "Linear" + cls)(cin, cout).to(dev).eval()  # noqa: E731
            x = torch.randn(B, cin, device=dev)
            xf = x.to(torch.bfloat16)
            macs = B * cin * cout
            shape = "%d->%d" % (cin, cout)
        xq = q8.quantize_act(x, 0.1, 128)
        src = mk("Flipout")
        tf, tr = twin_of(mk("Flipout"), True), twin_of(mk("Reparameterization"), False)
        g_f = capture(lambda: src(xf, return_kl=False), dev)
        g_q = capture(lambda: tf(xq, return_kl=False), dev)
        g_r = capture(lambda: tr(xq, return_kl=False), dev)
        rf = windows(g_f.replay, a.inner, a.repeats)
        rq = windows(g_q.replay, a.inner, a.repeats)
        rr = windows(g_r.replay, a.inner, a.repeats)
        rf = best(rf, windows(g_f.replay, a.inner, a.repeats))
        for i, r in enumerate((rf, rq, rr)):
            tot[i] += r[0] * times
        # two GEMMs: 2 * 2 * MACs integer operations per forward
        say("%-13s %-21s %2d | %s | %s | %s | %9.2f | %9.2f | %6.1f" % (name, shape, times, cell(rf), cell(rq), cell(rr), rq[0] / rf[0],
                                                                     rq[0] / rr[0], 4.0 * macs / (rq[0] * 1e-6) / 1e12))
        del g_f, g_q, g_r, src, tf, tr
    say("sum over the network's layers (x = occurrences): bf16 Flipout %.1f us, int8 Flipout %.1f us, int8 Reparameterization %.1f us; "
        "int8 Flipout / bf16 Flipout = %.2f, int8 Flipout / int8 Reparameterization = %.2f" % (tot[0], tot[1], tot[2], tot[1] / tot[0],
                                                                                              tot[1] / tot[2]))
    say("TOPS = 2 GEMMs * 2 * MACs of the layer / its int8 Flipout time (pre-pass included)")

    if not a.no_net:
        torch.manual_seed(0)
        x = torch.randn(B, 3, 224, 224, device=dev)
        mq = resnet.resnet18().eval()
        bt.dnn_to_bnn(mq, dict(PRIOR, type="Flipout"))
        mq = to_qresnet(mq.to(dev))
        torch.manual_seed(0)
        mf = resnet.resnet18()
        bt.dnn_to_bnn(mf, dict(PRIOR, type="Flipout"))
        mf = mf.to(dev).eval()
        for mod in mf.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.to(torch.bfloat16)
        fuse_model(mf)
        xf = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        g_q = capture(lambda: mq(x), dev)
        g_b = capture(lambda: mf(xf), dev)
        r_b = windows(g_b.replay, a.inner, a.repeats)
        r_q = windows(g_q.replay, a.inner, a.repeats)
        r_b = best(r_b, windows(g_b.replay, a.inner, a.repeats))
        say("ResNet18 forward, one MC sample (weight sampling and the input's quantize included):")
        say("  Flipout QResNet int8   %s   %8.1f images/s   (residual add: conv + btx_q8_add)" % (cell(r_q), B / (r_q[0] * 1e-6)))
        say("  bf16 Flipout           %s   %8.1f images/s   (fuse_model; BatchNorm, add and ReLU in the stores)" % (
            cell(r_b), B / (r_b[0] * 1e-6)))
        say("  int8 / bf16 = %.2f" % (r_q[0] / r_b[0]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
