"""Timing of the regression heads on the GPU (no bar: the numbers are reported as measured, slower or faster):

  1. us per forward + backward of utils.mc_loss.mc_gaussian_nll (csrc/btx_reg.hip: two launches forward, one backward) against the
     ATen chain a user writes today (set_backend("torch"): _mc_gnll_chain and its autograd backward), eager and replayed from a graph;
  2. us per batch of mc.RegressionEvaluator.update (two launches) against the ATen chain on mc.GaussianStats.unpack: running sums
     of err^2, |err|, the NLL and four coverage counts into a float64 device vector — eager with one .item() per batch, as such loops
     are written, and captured without it.

    python tools/reg_bench.py [--out profiles/reg_bench.txt] [--regions 20] [--inner 50]

Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back calls form one region; `regions` regions run back to back
after a warm-up of the same shape and the figure is the median of the SECOND half of them, with the range of that half beside it."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mc_loss_bench import capture, settled_regions  # noqa: E402

SHAPES = ((1, 256, 1), (8, 64, 1), (4, 64, 4096))  # (S, B, D)
CELL = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731


def bench_head(a, dev, emit):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.utils.mc_loss import mc_gaussian_nll
    emit("%-8s %3s %4s %5s %5s | %26s %26s | %26s %26s | %7s %7s" % (
        "reduce", "S", "B", "D", "dtype", "HIP eager", "ATen chain eager", "HIP graph", "ATen chain graph", "x eager", "x graph"))
    for reduce in ("loss", "moments"):
        for S, B, D in SHAPES:
            for dt in (torch.float32, torch.bfloat16):
                g = torch.Generator().manual_seed(S * 1000003 + B * 10007 + D)
                st = torch.cat([torch.randn(S, B, D, generator=g), torch.rand(S, B, D, generator=g) * 6 - 3], -1)
                st = st.to(dev).to(dt).requires_grad_(True)
                y = torch.randn(B, D, generator=g).to(dev)
                kl = torch.full((1,), 1000.0, device=dev)

                def fn():
                    st.grad = None
                    mc_gaussian_nll(st, y, kl, reduce).backward()
                res = {}
                for backend in ("auto", "torch"):
                    bt.set_backend(backend)
                    res[backend, "eager"] = settled_regions(fn, a.inner, a.regions)
                    graph = capture(fn, dev)
                    res[backend, "graph"] = settled_regions(graph.replay, a.inner, a.regions)
                    del graph
                bt.set_backend("auto")
                emit("%-8s %3d %4d %5d %5s | %s %s | %s %s | %7.2f %7.2f" % (
                    reduce, S, B, D, "f32" if dt == torch.float32 else "bf16", CELL(res["auto", "eager"]), CELL(res["torch", "eager"]),
                    CELL(res["auto", "graph"]), CELL(res["torch", "graph"]),
                    res["torch", "eager"][0] / res["auto", "eager"][0], res["torch", "graph"][0] / res["auto", "graph"][0]))


class AtenChain:
    """what a user writes after GaussianStats.unpack today"""

    def __init__(self, bs, levels, dev):
        from bayesian_torch_amd import mc
        self.bs = bs
        self.z2 = mc.normal_quantiles_squared(levels).to(dev)
        self.acc = torch.zeros(3 + len(levels), dtype=torch.float64, device=dev)

    def step(self, packed, y):
        from bayesian_torch_amd import mc
        u = mc.GaussianStats.unpack(packed, self.bs)
        var = u["total_var"].clamp_min(1e-12)
        err = y.double() - u["mean"]
        e2 = err * err
        self.acc[0] += e2.sum()
        self.acc[1] += err.abs().sum()
        self.acc[2] += (0.5 * (torch.log(2 * math.pi * var) + e2 / var)).sum()
        self.acc[3:] += (e2[None] <= self.z2[:, None, None] * var[None]).sum((1, 2))

    def step_item(self, packed, y):
        self.step(packed, y)
        return self.acc[0].item()


def bench_update(a, dev, emit):
    from bayesian_torch_amd import mc
    emit("%3s %4s %5s | %26s %26s | %26s %26s | %7s %7s" % ("S", "bs", "D", "update eager", "ATen chain + .item() eager",
                                                          "update graph", "ATen chain graph (no .item())", "x eager", "x graph"))
    levels = (0.5, 0.8, 0.9, 0.95)
    for S, bs, D in SHAPES:
        g = torch.Generator().manual_seed(S * 1000003 + bs * 10007 + D)
        stt = mc.GaussianStats("log")
        out = torch.cat([torch.randn(S * bs, D, generator=g), torch.rand(S * bs, D, generator=g) * 4 - 3], -1).to(dev)
        packed = stt.accumulate_lanes(torch.zeros(stt.numel(bs, 2 * D), dtype=torch.float64, device=dev), out, S)
        y = torch.randn(bs, D, generator=g).to(dev)
        ev = mc.RegressionEvaluator(D, levels=levels, device=dev)
        chain = AtenChain(bs, levels, dev)
        res = {"hip_eager": settled_regions(lambda: ev.update(packed, y), a.inner, a.regions),
               "aten_eager": settled_regions(lambda: chain.step_item(packed, y), a.inner, a.regions)}
        graph = capture(lambda: ev.update(packed, y), dev)
        res["hip_graph"] = settled_regions(graph.replay, a.inner, a.regions)
        graph2 = capture(lambda: chain.step(packed, y), dev)
        res["aten_graph"] = settled_regions(graph2.replay, a.inner, a.regions)
        del graph, graph2
        emit("%3d %4d %5d | %s %s | %s %s | %7.2f %7.2f" % (S, bs, D, CELL(res["hip_eager"]), CELL(res["aten_eager"]), CELL(res["hip_graph"]),
                                                           CELL(res["aten_graph"]), res["aten_eager"][0] / res["hip_eager"][0],
                                                           res["aten_graph"][0] / res["hip_graph"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_bench.txt"))
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    assert a.regions >= 8, "the settled half needs at least 8 regions"
    assert torch.cuda.is_available(), "reg_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/reg_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; us per call: median (min .. max) of the settled half of %d back-to-back regions of %d calls" % (
        torch.cuda.get_device_name(0), torch.__version__, a.regions, a.inner))
    emit("mc_gaussian_nll forward + backward (variance='log', kl on the device):")
    bench_head(a, dev, emit)
    emit("RegressionEvaluator.update (4 levels):")
    bench_update(a, dev, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
