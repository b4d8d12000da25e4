"""GPU time of a whole INT8 network: ResNet18 at batch 64, 224 x 224 as a models.QResNet (activations uint8 from the stem to the
head) with the residual add fused into the last conv's store (fuse_add) and as a launch of its own, beside the same network's bf16
Reparameterization form after fuse_model; and the per-launch times of the four kernels the network added (btx_q8_add,
btx_q8_contract_res, btx_q8_maxpool2d_cl, btx_q8_avgpool2d_cl) at the network's shapes.

    python tools/q8_net_bench.py [--out profiles/q8_net_bench.txt] [--repeats 20] [--inner 10] [--batch 64]

Method of tools/q8_bench.py: every forward is captured into a graph once (GPU time, not the host's launch work), HIP events
bracket `inner` replays after a warm-up, the figure is the median over `repeats` windows with min and max beside it.  Variants
that are compared are measured alternately (A, B, A) and A keeps the better of its two runs.  No threshold: what comes out is
recorded, an int8 network slower than the bf16 one included."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from q8_bench import capture, windows  # noqa: E402

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
# the last conv of a ResNet18 block, where the residual add sits: (name, channels, H = W, occurrences)
ADD_SITES = [("layer1 3x3 64 @56", 64, 56, 2), ("layer2 3x3 128 @28", 128, 28, 2), ("layer3 3x3 256 @14", 256, 14, 2),
             ("layer4 3x3 512 @7", 512, 7, 2)]


def cell(r):
    return "%9.1f (%7.1f ..%8.1f)" % r


def best(a, b):
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]))


def aba(ga, gb, inner, repeats):
    ra = windows(ga.replay, inner, repeats)
    rb = windows(gb.replay, inner, repeats)
    return best(ra, windows(ga.replay, inner, repeats)), rb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "q8_net_bench.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd import q8
    from bayesian_torch_amd.models import bnn_to_qbnn, fuse_model, resnet, to_qresnet
    assert torch.cuda.is_available(), "q8_net_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    bt.manual_seed(2024)
    bt.set_precision("bf16")
    B = a.batch
    lines = ["python tools/q8_net_bench.py --repeats %d --inner %d --batch %d" % (a.repeats, a.inner, a.batch),
             "device: %s; batch %d; us of GPU time (graph replay), median (min .. max) of %d windows of %d" % (
                 torch.cuda.get_device_name(0), B, a.repeats, a.inner)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    # ---- the whole network ------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    x = torch.randn(B, 3, 224, 224, device=dev)
    mq = resnet.resnet18().eval()
    bt.dnn_to_bnn(mq, dict(PRIOR, type="Reparameterization"))
    mq = to_qresnet(mq.to(dev))
    torch.manual_seed(0)
    mf = resnet.resnet18()
    bt.dnn_to_bnn(mf, dict(PRIOR, type="Reparameterization"))
    mf = mf.to(dev).eval()
    for mod in mf.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.to(torch.bfloat16)
    fuse_model(mf)
    xf = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        mq.set_fuse_add(True)(x)
        mf(xf)
    g_on = capture(lambda: mq.set_fuse_add(True)(x), dev)
    g_off = capture(lambda: mq.set_fuse_add(False)(x), dev)
    g_bf = capture(lambda: mf(xf), dev)
    say("ResNet18 forward, one MC sample (weight sampling included):")
    r_on, r_off = aba(g_on, g_off, a.inner, a.repeats)
    r_bf = windows(g_bf.replay, a.inner, a.repeats)
    r_on = best(r_on, windows(g_on.replay, a.inner, a.repeats))
    r_bf = best(r_bf, windows(g_bf.replay, a.inner, a.repeats))
    say("  QResNet int8, fuse_add on   %s   %8.1f images/s" % (cell(r_on), B / (r_on[0] * 1e-6)))
    say("  QResNet int8, fuse_add off  %s   %8.1f images/s" % (cell(r_off), B / (r_off[0] * 1e-6)))
    say("  bf16 Reparameterization     %s   %8.1f images/s   (fuse_model; BatchNorm, add and ReLU in the stores)" % (
        cell(r_bf), B / (r_bf[0] * 1e-6)))
    say("  int8 (fuse_add on) / bf16 = %.2f;  fuse_add off / on = %.3f" % (r_on[0] / r_bf[0], r_off[0] / r_on[0]))
    del g_on, g_off, g_bf, mq, mf

    # ---- the residual add: in the store of the conv, or a launch of its own ------------------------------------------------
    say("the block's last conv with its residual add (int8; sampling pre-pass in both columns):")
    say("  %-20s %2s | %28s | %28s | %28s | %s" % ("site", "x", "conv + add fused (1 launch)", "conv, then btx_q8_add", "btx_q8_add alone",
                                                  "unfused / fused"))
    tot = [0.0, 0.0]
    for name, c, hw, times in ADD_SITES:
        src = L.Conv2dReparameterization(c, c, 3, stride=1, padding=1, bias=False).to(dev).eval()
        wrap = torch.nn.Module()
        wrap.l = src
        bnn_to_qbnn(wrap)
        twin = wrap.l
        xq = q8.quantize_act(torch.randn(B, c, hw, hw, device=dev), 0.1, 128)
        res = q8.quantize_act(torch.randn(B, c, hw, hw, device=dev), 0.1, 128)
        g_f = capture(lambda: twin.forward_add(xq, res), dev)
        g_u = capture(lambda: q8.add(twin(xq, return_kl=False), res, 0.1, 0, True), dev)
        g_a = capture(lambda: q8.add(xq, res, 0.1, 0, True), dev)
        r_f, r_u = aba(g_f, g_u, a.inner, a.repeats)
        r_a = windows(g_a.replay, a.inner, a.repeats)
        tot[0] += r_f[0] * times
        tot[1] += r_u[0] * times
        say("  %-20s %2d | %s | %s | %s | %.3f" % (name, times, cell(r_f), cell(r_u), cell(r_a), r_u[0] / r_f[0]))
        del g_f, g_u, g_a
    say("  sum over the network's add sites: fused %.1f us, unfused %.1f us" % (tot[0], tot[1]))

    # ---- the pools ----------------------------------------------------------------------------------------------------------
    say("pooling (uint8 channels-last), bytes moved = input + output:")
    xm = q8.quantize_act(torch.randn(B, 64, 112, 112, device=dev), 0.1, 128)
    g_m = capture(lambda: q8.max_pool2d(xm, 3, 2, 1), dev)
    r = windows(g_m.replay, a.inner, a.repeats)
    nbytes = B * 64 * (112 * 112 + 56 * 56)
    say("  btx_q8_maxpool2d_cl 64 @112 3/2/1   %s   %6.2f TB/s" % (cell(r), nbytes / (r[0] * 1e-6) / 1e12))
    xa = q8.quantize_act(torch.randn(B, 512, 7, 7, device=dev), 0.1, 128)
    g_a = capture(lambda: q8.avg_pool2d(xa, 7, 1), dev)
    r = windows(g_a.replay, a.inner, a.repeats)
    nbytes = B * 512 * (49 + 1)
    say("  btx_q8_avgpool2d_cl 512 @7 7/1      %s   %6.2f TB/s" % (cell(r), nbytes / (r[0] * 1e-6) / 1e12))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
