"""Timing of the Monte-Carlo dropout unit (BTX-DROP v1, csrc/btx_drop.hip) on the GPU.  No bar: the numbers price a stand-alone
dropout launch, which is what a later fold into a contraction's store would save.

Per case, GPU time per captured call (one hipGraph replay) of
  * the forward (functional.dropout_hip) and the forward + backward (MCDropout under autograd: two launches),
  * torch.nn.functional.dropout on the same tensor (for lanes: on the stacked tensor of all lanes), forward and forward + backward,
  * a device copy of the bytes the forward writes (dst.copy_(src): the byte rate a pure stream reaches at this size).

    python tools/dropout_bench.py [--out profiles/dropout_bench.txt] [--regions 10] [--inner 20]

Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back replays form one region; `regions` regions run back to back
after a warm-up and the figure is the median (min .. max) of the second, settled half."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mc_loss_bench import capture, settled_regions  # noqa: E402

# (name, shape, dtype, channels-last, mode, lanes)
CASES = (("[64,64,56,56] bf16 cl", (64, 64, 56, 56), torch.bfloat16, True, "element", 1),
         ("[64,512,7,7] bf16 cl", (64, 512, 7, 7), torch.bfloat16, True, "element", 1),
         ("[64,4096] f32", (64, 4096), torch.float32, False, "element", 1),
         ("[64,64,56,56] bf16 cl x20 lanes", (64, 64, 56, 56), torch.bfloat16, True, "element", 20),
         ("[64,64,56,56] bf16 cl channel", (64, 64, 56, 56), torch.bfloat16, True, "channel", 1))


def bench_case(name, shape, dtype, cl, mode, lanes, a, dev):
    from bayesian_torch_amd import functional as BF, layers as L
    F = torch.nn.functional
    x = torch.randn(*shape, device=dev).to(dtype)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    layer = L.MCDropout(0.5, mode=mode)
    T, scale = layer._btx_T, layer._btx_scale
    words = torch.arange(lanes, dtype=torch.int32, device=dev)
    kw = dict(sample_dev=words, lanes=lanes, lane_batch=shape[0]) if lanes > 1 else dict(sample_dev=words)
    res = {}
    fwd = lambda: BF.dropout_hip(x, T, scale, mode, 1, 0, layer._btx_layer_id, **kw)  # noqa: E731
    out = fwd()
    out_bytes, in_bytes = out.numel() * out.element_size(), x.numel() * x.element_size()
    res["fwd"] = settled_regions(capture(fwd, dev).replay, a.inner, a.regions)
    stacked = out.detach().clone(memory_format=torch.preserve_format)   # what torch's dropout reads for the lanes case
    tdrop = {"element": F.dropout, "channel": F.dropout2d}[mode]
    tfwd = lambda: tdrop(stacked, 0.5, True)  # noqa: E731
    res["torch fwd"] = settled_regions(capture(tfwd, dev).replay, a.inner, a.regions)
    dst = torch.empty_like(stacked)
    res["copy"] = settled_regions(capture(lambda: dst.copy_(stacked), dev).replay, a.inner, a.regions)
    if lanes == 1:  # lanes are an inference feature
        xg = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
        dy = torch.randn_like(xg)
        layer.__dict__["_btx_sample_dev"] = words

        def fb():
            xg.grad = None
            layer(xg).backward(dy)
        res["fwd+bwd"] = settled_regions(capture(fb, dev).replay, a.inner, a.regions)
        layer.__dict__["_btx_sample_dev"] = None

        def tfb():
            xg.grad = None
            tdrop(xg, 0.5, True).backward(dy)
        res["torch fwd+bwd"] = settled_regions(capture(tfb, dev).replay, a.inner, a.regions)
    return res, in_bytes, out_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_bench.txt"))
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    assert a.regions >= 8, "the settled half needs at least 8 regions"
    assert torch.cuda.is_available(), "dropout_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/dropout_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; us per captured call (one hipGraph replay), p = 0.5: median (min .. max) of the settled half of %d "
         "back-to-back regions of %d replays; GB/s = (bytes read + bytes written) / median" % (
             torch.cuda.get_device_name(0), torch.__version__, a.regions, a.inner))
    cell = lambda r: "%8.1f (%8.1f ..%8.1f)" % r  # noqa: E731
    for case in CASES:
        res, in_bytes, out_bytes = bench_case(*case, a, dev)
        emit("")
        emit("%s   (reads %.1f MB, writes %.1f MB)" % (case[0], in_bytes / 1e6, out_bytes / 1e6))
        for k in ("fwd", "torch fwd", "copy", "fwd+bwd", "torch fwd+bwd"):
            if k not in res:
                continue
            moved = {"fwd": in_bytes + out_bytes, "fwd+bwd": 2 * (in_bytes + out_bytes)}.get(k, 2 * out_bytes if k != "torch fwd+bwd"
                                                                                           else 4 * out_bytes)
            emit("  %-14s %s us   %7.0f GB/s%s" % (k, cell(res[k]), moved / res[k][0] / 1e3,
                                                  "   (x%.2f of the copy's time)" % (res[k][0] / res["copy"][0]) if k == "fwd" else ""))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
