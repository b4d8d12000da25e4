"""us per forward + backward of the calibration losses AvULoss / AUAvULoss on the GPU: the fused HIP path (btx_avu_fwd +
btx_avu_bwd, three launches) against the package's own vectorised ATen chain (set_backend("torch"), utils/_calibration.py) on
the same GPU tensors, each issued eagerly and replayed from a captured graph; then ms per autograd.GraphedTrainStep of a small
LinearFlipout MLP with and without the AvU term in its loss.

    python tools/avuc_bench.py [--out profiles/avuc_bench.txt] [--repeats 25] [--inner 50]

Timing: HIP events around `inner` back-to-back calls (eager: the host issues them, so this is what a training loop sees; graph:
`inner` replays), after a warm-up of the same shape; the figure is the median over `repeats` such windows, min and max beside it.
The table goes to --out with the command on its first line."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def windows(fn, inner, repeats):
    """per-call microseconds of `repeats` windows of `inner` calls: (median, min, max)"""
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
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "avuc_bench.txt"))
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    assert a.repeats >= 20
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.utils.avuc_loss import AUAvULoss, AvULoss
    assert torch.cuda.is_available(), "avuc_bench.py measures on the GPU only"
    dev = torch.device("cuda:0")
    lines = ["python tools/avuc_bench.py " + " ".join(sys.argv[1:]),
             "device: %s; us per forward + backward, median (min .. max) of %d windows of %d calls" % (
                 torch.cuda.get_device_name(0), a.repeats, a.inner),
             "%-10s %5s %5s %5s | %26s %26s | %26s %26s | %7s %7s" % (
                 "loss", "B", "C", "dtype", "fused eager", "ATen chain eager", "fused graph", "ATen chain graph", "x eager", "x graph")]
    slower = []
    for loss_name in ("AvULoss", "AUAvULoss"):
        for B in (128, 256):
            for C in (10, 1000):
                for dt in (torch.float32, torch.bfloat16):
                    g = torch.Generator().manual_seed(B * 10007 + C)
                    logits = (torch.randn(B, C, generator=g) * 3).to(dev).to(dt).requires_grad_(True)
                    labels = torch.randint(0, C, (B,), generator=g).to(dev)
                    mod = AvULoss(beta=3.0) if loss_name == "AvULoss" else AUAvULoss(beta=3.0)

                    def fn():
                        logits.grad = None
                        out = mod(logits, labels, 1.0) if loss_name == "AvULoss" else mod(logits, labels)[0]
                        out.sum().backward()
                    res = {}
                    for backend in ("auto", "torch"):
                        bt.set_backend(backend)
                        res[backend, "eager"] = windows(fn, a.inner, a.repeats)
                        graph = capture(fn, dev)
                        res[backend, "graph"] = windows(graph.replay, a.inner, a.repeats)
                        del graph
                    bt.set_backend("auto")
                    cell = lambda r: "%8.1f (%7.1f ..%7.1f)" % r  # noqa: E731
                    xe = res["torch", "eager"][0] / res["auto", "eager"][0]
                    xg = res["torch", "graph"][0] / res["auto", "graph"][0]
                    lines.append("%-10s %5d %5d %5s | %s %s | %s %s | %7.2f %7.2f" % (
                        loss_name, B, C, "f32" if dt == torch.float32 else "bf16", cell(res["auto", "eager"]),
                        cell(res["torch", "eager"]), cell(res["auto", "graph"]), cell(res["torch", "graph"]), xe, xg))
                    print(lines[-1], flush=True)
                    if xe < 1.0 or xg < 1.0:
                        slower.append(lines[-1])
    # a captured training step of a small MLP, with and without the AvU term
    bt.manual_seed(2024)
    bt.set_precision("f32")
    torch.manual_seed(0)
    bs = 128
    m = torch.nn.Sequential(torch.nn.Linear(784, 512), torch.nn.ReLU(), torch.nn.Linear(512, 10))
    bt.dnn_to_bnn(m, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                          moped_enable=False, moped_delta=0.5))
    m = m.to(dev).train()
    bt.assign_layer_ids(m)
    x = torch.randn(bs, 784, device=dev)
    y = torch.randint(0, 10, (bs,), device=dev)
    avu, area = AvULoss(beta=3.0), AUAvULoss(beta=3.0)
    base = lambda out, tgt: torch.nn.functional.cross_entropy(out.float(), tgt) + bt.get_kl_loss(m) / bs  # noqa: E731
    forms = (("ce + kl / bs", base),
             ("ce + kl / bs + AvULoss", lambda out, tgt: base(out, tgt) + avu(out, tgt, 1.0).sum()),
             ("ce + kl / bs + AUAvULoss", lambda out, tgt: base(out, tgt) + area(out, tgt)[0].sum()))
    lines.append("GraphedTrainStep, LinearFlipout MLP 784 -> 512 -> 10, batch %d, f32: us per replay" % bs)
    for name, loss_fn in forms:
        step = GraphedTrainStep(m, x, y, loss_fn=loss_fn)
        it = iter(range(1 << 30))
        r = windows(lambda: step.run(next(it)), a.inner, a.repeats)
        step.close()
        del step
        lines.append("%-28s %8.1f (%7.1f ..%7.1f)" % ((name,) + r))
        print(lines[-1], flush=True)
    lines.append("rows where the fused path is slower than the ATen chain: %d" % len(slower))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
