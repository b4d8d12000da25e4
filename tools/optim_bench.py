"""us per optimizer step on the parameter tensors of a dnn_to_bnn ResNet18 (Flipout) and of the LSTM model of
tools/lstm_train_bench.py: bayesian_torch_amd.optim (csrc/btx_optim.hip) issued eagerly and replayed from a hipGraph, against
torch.optim with foreach=True, with fused=True (where torch offers it on ROCm) and captured (capturable=True for Adam); then the whole
captured training step with the update inside (GraphedTrainStep(optimizer=)) against a replay followed by a torch.optim step.

    python tools/optim_bench.py [--steps 200] [--repeats 5] [--out profiles/optim_bench.txt]

Every figure is a host clock around `steps` steps that end in a device synchronise (so host-bound variants show their host cost),
median of `repeats` windows with the range; "floor" is the bytes one pass has to move (Adam 28 B/element: read p, g, m, v, write p,
m, v; SGD with momentum 20) over the 6.29 TB/s copy rate measured on this GPU."""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

COPY_RATE = 6.29e12
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
OPTS = [("Adam", dict(lr=1e-3), 28), ("SGD", dict(lr=1e-2, momentum=0.9, weight_decay=1e-4), 20)]


def windows(fn, steps, repeats):
    """us per call of fn: median and range over `repeats` windows of `steps` calls, each ended by a synchronise"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / steps)
    return statistics.median(us), min(us), max(us)


def clones(params):
    """fresh parameters with the strides of the model's (GEMM-major conv parameters stay permuted views of dense storage) and
    gradients of the same strides"""
    out = []
    for p in params:
        q = torch.nn.Parameter(torch.empty_like(p).copy_(p.detach()))
        q.grad = torch.randn_like(p) * 1e-3
        assert q.stride() == p.stride() and q.grad.stride() == p.stride()
        out.append(q)
    return out


def captured(step_fn, warm):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm):
            step_fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step_fn()
    return g


def bench_set(label, params, a, emit):
    from bayesian_torch_amd import optim
    n_el = sum(p.numel() for p in params)
    emit("%s: %d tensors, %d elements (%.1f MB f32), %d not contiguous" % (
        label, len(params), n_el, n_el * 4 / 1e6, sum(not p.is_contiguous() for p in params)))
    for name, kw, bpe in OPTS:
        emit("  %s %s   floor %.1f us (%d B/element at 6.29 TB/s)" % (name, kw, n_el * bpe / COPY_RATE * 1e6, bpe))
        rows = []
        o = getattr(optim, name)(clones(params), **kw)
        rows.append(("ours, eager", windows(o.step, a.steps, a.repeats)))
        o = getattr(optim, name)(clones(params), **kw)
        o.step()
        with torch.no_grad():
            plan = o._plan()
            g = captured(lambda: o._launch(plan), 1)

        def ours_graph():
            o._advance(plan)
            g.replay()
            o._finish(plan)
        rows.append(("ours, inside a graph (host: step counts + block rewrite, then replay)", windows(ours_graph, a.steps, a.repeats)))
        rows.append(("ours, graph replay alone", windows(g.replay, a.steps, a.repeats)))
        o = getattr(torch.optim, name)(clones(params), foreach=True, **kw)
        rows.append(("torch.optim foreach=True, eager", windows(o.step, a.steps, a.repeats)))
        try:
            o = getattr(torch.optim, name)(clones(params), fused=True, **kw)
            rows.append(("torch.optim fused=True, eager", windows(o.step, a.steps, a.repeats)))
        except Exception as e:  # noqa: BLE001 — not offered on this build
            emit("    torch.optim fused=True: not offered (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:90]))
        try:
            ckw = dict(capturable=True) if name != "SGD" else {}
            o = getattr(torch.optim, name)(clones(params), foreach=True, **ckw, **kw)
            g2 = captured(o.step, 3)
            rows.append(("torch.optim foreach=True%s, inside a graph" % (", capturable=True" if ckw else ""),
                         windows(g2.replay, a.steps, a.repeats)))
        except Exception as e:  # noqa: BLE001
            emit("    torch.optim inside a graph: failed (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:90]))
        for what, (med, lo, hi) in rows:
            emit("    %-78s %8.1f us  (%.1f - %.1f)" % (what, med, lo, hi))
        del o, g, plan
        gc.collect()


def bench_step(label, model, x, y, a, emit):
    """the whole training step: GraphedTrainStep with the update inside against replay + torch.optim step"""
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    it = iter(range(1 << 30))
    steps = max(20, a.steps // 4)
    for name, kw, _ in OPTS:
        res = []
        for mode in ("torch", "ours"):
            for m in model.modules():  # a Flipout LSTM keeps its last KL, with its autograd graph, in `.kl`
                if hasattr(m, "kl"):
                    m.kl = None
            gc.collect()
            if mode == "ours":
                opt = getattr(optim, name)(model.parameters(), **kw)
                gs = GraphedTrainStep(model, x, y, optimizer=opt)
                fn = lambda: gs.run(next(it))  # noqa: E731
            else:
                opt = getattr(torch.optim, name)(model.parameters(), foreach=True, **kw)
                gs = GraphedTrainStep(model, x, y)

                def fn():
                    gs.run(next(it))
                    opt.step()
            res.append(windows(fn, steps, a.repeats))
            gs.close()
            del gs, opt, fn
        (t, tl, th), (o, ol, oh) = res
        emit("  %s, %s: replay + torch.optim foreach step %8.1f us (%.1f - %.1f);  update inside the graph %8.1f us (%.1f - %.1f);  %.3fx" % (
            label, name, t, tl, th, o, ol, oh, t / o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.txt"))
    ap.add_argument("--skip-train-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs a GPU"
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model, resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    from lstm_train_bench import SeqNet
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("optim_bench: %s, torch %s, %d steps per window, %d windows (median, range); us per step" % (
        torch.cuda.get_device_name(0), torch.__version__, a.steps, a.repeats))
    bt.manual_seed(1)
    torch.manual_seed(0)
    rn = resnet.resnet18()
    bt.dnn_to_bnn(rn, dict(PRIOR, type="Flipout"))
    rn = rn.to(dev).train()
    bt.assign_layer_ids(rn)
    ls = SeqNet(256, 512)
    bt.dnn_to_bnn(ls, dict(PRIOR, type="Flipout"))
    ls = ls.to(dev).train()
    bench_set("ResNet18 Flipout", list(rn.parameters()), a, emit)
    bench_set("LSTM 256 -> 512 + head", list(ls.parameters()), a, emit)
    if not a.skip_train_step:
        emit("whole captured training step (forward + CE + KL / B + backward [+ update]), us per step:")
        bt.set_precision("bf16")
        hip_batchnorm(rn)
        x = torch.randn(64, 3, 224, 224, device=dev)
        y = torch.randint(0, 1000, (64,), device=dev)
        bench_step("ResNet18 Flipout, batch 64, 224^2, bf16 contraction, hip_batchnorm", rn, x, y, a, emit)
        bt.set_precision("f32")
        fuse_model(ls, lstm_training=True)
        x = torch.randn(64, 64, 256, device=dev)
        y = torch.randint(0, 10, (64,), device=dev)
        bench_step("LSTM I 256, H 512, B 64, T 64, f32, fused training", ls, x, y, a, emit)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
