"""Timing of the evaluation head on the GPU (no bar: the feature is the capability and the single host read, not a speed-up):

  1. us per batch of mc.Evaluator.update (csrc/btx_mceval.hip, two launches) on a packed vector, issued eagerly and replayed from
     a captured graph, against the ATen chain a user of mc.unpack writes today: unpack, argmax, topk(5), gather / log,
     bucketize + bincount and one .item() per batch (the captured form leaves the .item() out and replaces bincount by a
     scatter_add_: a host read cannot be captured, which is the point);
  2. batches / s of a 16-batch validation loop of a dnn_to_bnn ResNet18 (Flipout, batch 64, 224^2, bf16, 20 samples as 20 lanes)
     with mc.evaluate() against the same GraphedMC loop followed by the ATen chain.

    python tools/mc_eval_bench.py [--out profiles/mc_eval_bench.txt] [--regions 20] [--inner 50] [--skip-loop]

Method (tools/mc_loss_bench.py): HIP events around `inner` back-to-back calls form one region; `regions` regions run back to back
after a warm-up of the same shape and the figure is the median of the SECOND half of them, with the range of that half beside it."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mc_loss_bench import PRIOR, capture, settled_regions  # noqa: E402

SHAPES = ((64, 1000), (256, 10), (128, 1000))


class AtenChain:
    """what a user writes after mc.unpack today: running top-1 / top-5 / NLL / entropy sums and a 15-bin histogram"""

    def __init__(self, bs, C, dev):
        self.bs, self.C = bs, C
        self.acc = torch.zeros(4, dtype=torch.float64, device=dev)
        self.hist = torch.zeros(15, dtype=torch.int64, device=dev)
        self.edges = torch.linspace(0, 1, 16, device=dev)[1:-1].contiguous()

    def step(self, packed, y, capturable=False):
        from bayesian_torch_amd import mc
        u = mc.unpack(packed, self.bs, self.C)
        p = u["mean_prob"]
        conf, pred = p.max(1)
        top5 = p.topk(min(5, self.C), dim=1).indices
        nll = -torch.log(p.gather(1, y[:, None])[:, 0] + 1e-15)
        self.acc[0] += (pred == y).sum()
        self.acc[1] += (top5 == y[:, None]).any(1).sum()
        self.acc[2] += nll.sum()
        self.acc[3] += u["predictive_entropy"].sum()
        b = torch.bucketize(conf, self.edges, right=False)
        if capturable:  # bincount sizes its result on the host: under capture the histogram is a scatter_add_ instead
            self.hist.scatter_add_(0, b, torch.ones_like(b))
        else:
            self.hist += torch.bincount(b, minlength=15)

    def step_item(self, packed, y):
        self.step(packed, y)
        return self.acc[0].item()


def bench_update(a, dev, emit):
    from bayesian_torch_amd import mc
    emit("%5s %5s | %26s %26s | %26s %26s | %7s %7s" % ("bs", "C", "Evaluator.update eager", "ATen chain + .item() eager",
                                                       "Evaluator.update graph", "ATen chain graph (no .item())", "x eager", "x graph"))
    cell = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731
    for bs, C in SHAPES:
        g = torch.Generator().manual_seed(bs * 10007 + C)
        packed = torch.zeros(mc.packed_numel(bs, C), device=dev)
        for _ in range(4):
            mc.accumulate(packed, (torch.randn(bs, C, generator=g) * 3).to(dev))
        y = torch.randint(0, C, (bs,), generator=g).to(dev)
        ev = mc.Evaluator(C, thresholds=[0.5, 1.0, 2.0], device=dev)
        chain = AtenChain(bs, C, dev)
        res = {"hip_eager": settled_regions(lambda: ev.update(packed, y), a.inner, a.regions),
               "aten_eager": settled_regions(lambda: chain.step_item(packed, y), a.inner, a.regions)}
        graph = capture(lambda: ev.update(packed, y), dev)
        res["hip_graph"] = settled_regions(graph.replay, a.inner, a.regions)
        graph2 = capture(lambda: chain.step(packed, y, capturable=True), dev)
        res["aten_graph"] = settled_regions(graph2.replay, a.inner, a.regions)
        del graph, graph2
        emit("%5d %5d | %s %s | %s %s | %7.2f %7.2f" % (bs, C, cell(res["hip_eager"]), cell(res["aten_eager"]), cell(res["hip_graph"]),
                                                       cell(res["aten_graph"]), res["aten_eager"][0] / res["hip_eager"][0],
                                                       res["aten_graph"][0] / res["hip_graph"][0]))


def bench_loop(a, dev, emit):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import fuse_resnet
    bt.manual_seed(1)
    torch.manual_seed(0)
    rn = resnet.resnet18()
    bt.dnn_to_bnn(rn, dict(PRIOR, type="Flipout"))
    rn = rn.to(dev).eval()
    for mod in rn.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.to(torch.bfloat16)
    bt.assign_layer_ids(rn)
    fuse_resnet(rn)
    bt.set_precision("bf16")
    S, nb, bs = 20, 16, 64
    xs = [torch.randn(bs, 3, 224, 224, device=dev).to(torch.bfloat16) for _ in range(2)]
    ys = [torch.randint(0, 1000, (bs,), device=dev) for _ in range(2)]
    batches = lambda n: ((xs[i & 1], ys[i & 1]) for i in range(n))  # noqa: E731
    try:
        def with_evaluate(n):
            ev = mc.evaluate(rn, batches(n), S, lanes=S, graphed=True, evaluator=mc.Evaluator(1000, capacity=n * bs, device=dev))
            return ev.compute()["top1"]

        def with_chain(n):
            g = mc.GraphedMC(rn, xs[0].clone(), lanes=S, static_input=True)
            chain = AtenChain(bs, 1000, dev)
            try:
                for x, y in batches(n):
                    g.packed.zero_()
                    g.set_input(x)
                    g.run_many(list(range(S)))
                    chain.step_item(g.packed, y)
            finally:
                g.close()
            return chain.acc[0].item() / (n * bs)

        def wall(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        res = {}
        for name, fn in (("evaluate", with_evaluate), ("chain", with_chain)):
            fn(2)  # warm-up: kernels loaded, allocator pools filled
            # both forms capture their graph inside the call: a loop of nb and one of 3 * nb batches differ by 2 * nb batches alone
            rates = sorted(2 * nb / (wall(fn, 3 * nb) - wall(fn, nb)) for _ in range(a.loop_repeats))
            res[name] = (rates[len(rates) // 2], rates[0], rates[-1])
    finally:
        bt.set_precision("f32")
    emit("validation loop, ResNet18 Flipout, batches of %d, 224^2, bf16, %d samples as %d lanes; batches / s from the wall time of a "
         "%d-batch loop minus that of a %d-batch loop (the graph capture cancels), median (min .. max) of %d pairs:" % (
             bs, S, S, 3 * nb, nb, a.loop_repeats))
    emit("  mc.evaluate() (Evaluator.update, one host read at the end)   %8.2f (%.2f .. %.2f)" % res["evaluate"])
    emit("  GraphedMC loop + ATen chain with one .item() per batch       %8.2f (%.2f .. %.2f)" % res["chain"])
    emit("  evaluate / chain: %.3f" % (res["evaluate"][0] / res["chain"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_eval_bench.txt"))
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--loop-repeats", type=int, default=5)
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    assert a.regions >= 8, "the settled half needs at least 8 regions"
    assert torch.cuda.is_available(), "mc_eval_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("python tools/mc_eval_bench.py " + " ".join(sys.argv[1:]))
    emit("device: %s, torch %s; us per batch: median (min .. max) of the settled half of %d back-to-back regions of %d calls" % (
        torch.cuda.get_device_name(0), torch.__version__, a.regions, a.inner))
    bench_update(a, dev, emit)
    if not a.skip_loop:
        bench_loop(a, dev, emit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
