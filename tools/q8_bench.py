"""GPU time per layer of the INT8 path (weight sampling pre-pass + i8 MFMA contraction, btx_q8.hip) against the bf16
Reparameterization path (one fused sample-and-contract call, unchanged by the INT8 work) at the same shapes: the convolutions of
ResNet18 at batch 64, 224 x 224 (BASELINE cfg3) and its 512 -> 1000 head.

    python tools/q8_bench.py [--out profiles/q8_bench.txt] [--repeats 20] [--inner 20] [--batch 64]

Both layers get their input the way a layer inside a network does: bf16 channels-last for the float layer, an already quantized
uint8 channels-last carrier for the INT8 twin (the activation quantize of a model's first layer is not part of the figure).
Timing: each forward is captured into a graph once (so the figure is GPU time, not the host's launch work) and HIP events bracket
`inner` replays after a warm-up; the figure is the median over `repeats` windows, min and max beside it.  No threshold: the ratio
is recorded as it comes out."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (name, Cin, Cout, k, stride, padding, input H = W, how many times ResNet18 has it)
CONVS = [("stem 7x7/2", 3, 64, 7, 2, 3, 224, 1),
         ("layer1 3x3", 64, 64, 3, 1, 1, 56, 4),
         ("layer2 3x3/2", 64, 128, 3, 2, 1, 56, 1),
         ("layer2 3x3", 128, 128, 3, 1, 1, 28, 3),
         ("layer2 1x1/2", 64, 128, 1, 2, 0, 56, 1),
         ("layer3 3x3/2", 128, 256, 3, 2, 1, 28, 1),
         ("layer3 3x3", 256, 256, 3, 1, 1, 14, 3),
         ("layer3 1x1/2", 128, 256, 1, 2, 0, 28, 1),
         ("layer4 3x3/2", 256, 512, 3, 2, 1, 14, 1),
         ("layer4 3x3", 512, 512, 3, 1, 1, 7, 3),
         ("layer4 1x1/2", 256, 512, 1, 2, 0, 14, 1)]


def windows(fn, inner, repeats):
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def capture(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "q8_bench.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd import q8
    from bayesian_torch_amd.models import bnn_to_qbnn
    assert torch.cuda.is_available(), "q8_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    bt.manual_seed(2024)
    bt.set_precision("bf16")
    torch.manual_seed(0)
    B = a.batch
    lines = ["python tools/q8_bench.py " + " ".join(sys.argv[1:]),
             "device: %s; batch %d; us of GPU time per layer forward (graph replay), median (min .. max) of %d windows of %d" % (
                 torch.cuda.get_device_name(0), B, a.repeats, a.inner),
             "%-14s %-22s %3s | %28s | %28s | %11s | %8s" % ("layer", "shape", "x", "bf16 Reparameterization", "int8 sample + contract",
                                                             "int8 / bf16", "int8 TOPS")]
    tot = [0.0, 0.0]
    cases = [(n, "conv", c) for n, *c in CONVS] + [("head", "linear", (512, 1000))]
    for name, kind, c in cases:
        if kind == "conv":
            cin, cout, k, s, p, hw, times = c
            src = L.Conv2dReparameterization(cin, cout, k, stride=s, padding=p, bias=False).to(dev).eval()
            x = torch.randn(B, cin, hw, hw, device=dev)
            xf = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            ho = (hw + 2 * p - k) // s + 1
            macs = B * ho * ho * cout * cin * k * k
            shape = "%d->%d %dx%d/%d @%d" % (cin, cout, k, k, s, hw)
            xq = q8.quantize_act(x, 0.1, 128)
        else:
            cin, cout = c
            times = 1
            src = L.LinearReparameterization(cin, cout).to(dev).eval()
            x = torch.randn(B, cin, device=dev)
            xf = x.to(torch.bfloat16)
            macs = B * cin * cout
            shape = "%d->%d" % (cin, cout)
            xq = q8.quantize_act(x, 0.2, 128)
        wrap = torch.nn.Module()
        wrap.l = src
        bnn_to_qbnn(wrap)
        twin = wrap.l
        g_f = capture(lambda: src(xf, return_kl=False), dev)
        g_q = capture(lambda: twin(xq, return_kl=False), dev)
        # bf16, int8, bf16 again: the bf16 column keeps the better of its two runs, so drift on a shared machine cannot flatter int8
        rf = windows(g_f.replay, a.inner, a.repeats)
        rq = windows(g_q.replay, a.inner, a.repeats)
        rf2 = windows(g_f.replay, a.inner, a.repeats)
        rf = (min(rf[0], rf2[0]), min(rf[1], rf2[1]), max(rf[2], rf2[2]))
        tot[0] += rf[0] * times
        tot[1] += rq[0] * times
        cell = lambda r: "%9.1f (%7.1f ..%8.1f)" % r  # noqa: E731
        lines.append("%-14s %-22s %3d | %s | %s | %11.2f | %8.1f" % (name, shape, times, cell(rf), cell(rq), rq[0] / rf[0],
                                                                   2.0 * macs / (rq[0] * 1e-6) / 1e12))
        print(lines[-1], flush=True)
        del g_f, g_q, src, twin
    lines.append("sum over the network's layers (x = occurrences): bf16 %.1f us, int8 %.1f us, int8 / bf16 = %.2f" % (
        tot[0], tot[1], tot[1] / tot[0]))
    lines.append("int8 TOPS = 2 * MACs of the layer / its int8 time (sampling pre-pass included)")
    print(lines[-2])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
