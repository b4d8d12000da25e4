"""Data-parallel training step (autograd.GraphedTrainStep(group=)) at 1, 2, 4 and 8 ranks of one node: ms per step, the
exposed time of the step's one all-reduce, and the scaling against the ungrouped step measured in the same run.

    python tools/ddp_bench.py [--ranks 1,2,4,8] [--steps 30] [--windows 3] [--out profiles/ddp_bench.txt]

The driver starts `python -m torch.distributed.run --nproc-per-node N tools/ddp_bench.py --worker` once per rank count (rank counts
above the GPUs present are reported as skipped).  Every rank arms its own time limit (--rank-limit seconds, SIGALRM) and the driver
bounds each launch as well.  Workload: ResNet18-Flipout, bf16 contraction, HIP BatchNorm, batch 64 per GPU, 224^2, Adam inside the
graph.  Per rank count, in one process per GPU:
  baseline   GraphedTrainStep(model, x, y, optimizer=Adam) — no group, every rank at the same time (the node's power and host are shared
             as they are in the grouped run)
  grouped    GraphedTrainStep(..., group=WORLD): host clock around `steps` steps ended by a synchronise, median of `windows` windows; the
             all-reduce between events recorded on the replay stream around it, median over the steps of the last window.  The event
             pair measures what the collective adds to the stream: its own time plus the wait for the slowest rank's graph A.
Figures are the slowest rank's (a step ends when the last rank's does)."""
import argparse
import os
import signal
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
BATCH = 64


def windows(fn, steps, n):
    """ms per call: median and range over n windows of `steps` calls, each ended by a synchronise"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    return statistics.median(ms), min(ms), max(ms)


def worker(a):
    import torch.distributed as dist
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    from bayesian_torch_amd.models import resnet
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    signal.alarm(a.rank_limit)  # this rank's own time limit: the default action ends the process
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", 0))
    dev = torch.device("cuda:%d" % local)
    torch.cuda.set_device(dev)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", device_id=dev)
    try:
        bt.manual_seed(1)
        bt.set_precision("bf16")
        torch.manual_seed(0)
        net = resnet.resnet18()
        bt.dnn_to_bnn(net, dict(PRIOR, type="Flipout"))
        net = net.to(dev).train()
        bt.assign_layer_ids(net)
        hip_batchnorm(net)
        torch.manual_seed(100 + rank)
        x = torch.randn(BATCH, 3, 224, 224, device=dev)
        y = torch.randint(0, 1000, (BATCH,), device=dev)
        it = iter(range(1 << 30))
        res = {}
        for mode in ("baseline", "grouped"):
            opt = optim.Adam(net.parameters(), lr=1e-4)
            kw = dict(group=dist.group.WORLD) if mode == "grouped" else {}
            gs = GraphedTrainStep(net, x, y, optimizer=opt, **kw)
            dist.barrier()
            res[mode] = windows(lambda: gs.run(next(it)), a.steps, a.windows)
            if mode == "grouped":
                evs = []
                for _ in range(a.steps):
                    s = next(it)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    gs.forward_backward(s)
                    e0.record()
                    gs.reducer.all_reduce()
                    e1.record()
                    gs.apply()
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                ar = [e0.elapsed_time(e1) for e0, e1 in evs]
                res["allreduce"] = (statistics.median(ar), min(ar), max(ar))
                res["bucket_mb"] = gs.reducer.bucket.numel() * 4 / 1e6
                res["loss"] = float(gs.reducer.loss)
            gs.close()
            del gs, opt
        allres = [None] * world
        dist.all_gather_object(allres, res)
        if rank == 0:
            worst = lambda k: max((r[k] for r in allres), key=lambda t: t[0])  # noqa: E731
            b, g, c = worst("baseline"), worst("grouped"), worst("allreduce")
            print("DDP ranks %d: ungrouped step %.2f ms (%.2f - %.2f); grouped step %.2f ms (%.2f - %.2f); all-reduce of %.1f MB "
                  "exposed %.3f ms (%.3f - %.3f) = %.1f %% of the step; %.0f images/s, %.2fx of one ungrouped GPU (ideal %d); "
                  "mean loss %.4f" % (world, b[0], b[1], b[2], g[0], g[1], g[2], res["bucket_mb"], c[0], c[1], c[2], 100 * c[0] / g[0],
                                      world * BATCH / g[0] * 1e3, world * b[0] / g[0], world, res["loss"]), flush=True)
    finally:
        bt.set_precision("f32")
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--ranks", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rank-limit", type=int, default=240, help="seconds a rank may live")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddp_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    assert torch.cuda.is_available(), "ddp_bench needs a GPU"
    gpus = torch.cuda.device_count()
    lines = ["ddp_bench: %s x %d, torch %s; ResNet18-Flipout bf16, batch %d per GPU, 224^2, Adam in the graph; %d steps per window, "
             "%d windows (median, range); slowest rank" % (torch.cuda.get_device_name(0), gpus, torch.__version__, BATCH, a.steps,
                                                           a.windows)]
    print(lines[0], flush=True)
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    for n in [int(v) for v in a.ranks.split(",")]:
        if not 1 <= n <= 8:
            raise SystemExit("--ranks: 1 to 8 ranks")
        if n > gpus:
            lines.append("DDP ranks %d: skipped, %d GPU(s) present: not measured" % (n, gpus))
            print(lines[-1], flush=True)
            continue
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n, "--master-addr", "127.0.0.1",
               "--master-port", str(29500 + n), os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--windows",
               str(a.windows), "--rank-limit", str(a.rank_limit)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=a.rank_limit + 30)
        except subprocess.TimeoutExpired:
            lines.append("DDP ranks %d: the launch ran into its time limit: not measured" % n)
            print(lines[-1], flush=True)
            break  # nothing more is started on GPUs that a rank may have hung
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("DDP ")]
        if r.returncode != 0 or not got:
            lines.append("DDP ranks %d: failed (exit %d): not measured" % (n, r.returncode))
            print(lines[-1], flush=True)
            print(r.stderr[-3000:], flush=True)
            break
        lines += got
        print("\n".join(got), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
