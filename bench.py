#!/usr/bin/env python3
"""bench.py — MC-samples/sec of the variational-layer forward hot path on MI355X.

Headline workload (BASELINE.json metric / configs[3], the per-GPU shard): dnn_to_bnn(ResNet18) Flipout, 224x224, batch 64,
synthetic input, reference init draws (torch.manual_seed(0)), MC sample s keyed (seed=2024, sample_idx=s), bf16
activations + bf16 MFMA.  A "step" = one Monte-Carlo sample: one stochastic forward of the whole converted model (one
weight-sampling launch, 21 contraction launches with eval-BN / residual / ReLU folded into their stores, the pooling ops
between them) + the on-device accumulation of the predictive statistics, replayed from ONE hipGraph (`--lanes` samples in
flight per replay, one stream each).

    python bench.py                              # 1 GPU
    python bench.py --gpus 8 --steps K --warmup W   # launches 8 ranks itself (torch.distributed.run, RCCL) — or run it
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P bench.py --gpus 8 ...
    python bench.py --full                       # + everything below the headline (roofline, extra, cpu_baseline, ...)

N>1: every rank runs its own K samples (weak scaling; sample indices interleaved by rank; `--scaling strong
--total-samples S` shards S samples instead), then ONE RCCL all-reduce of the packed statistics inside the timed
region.  A run whose process group does not have exactly --gpus ranks aborts: it cannot print a line.

A plain run sets up, warms up, times ONE region of exactly K MC samples (`ms_per_step` = that region / K) and prints the
line; `--dump-outputs DIR` then writes the predictive statistics of that region (mc.unpack: what a caller of the MC path
receives) and the logits of its last MC sample as DIR/<name>.npy.  `--full` times the region back to back until it has
settled (`--repeats`, `--settle-seconds`) and adds to the line (rank 0):
  roofline      dominant kernel = the stride-1 3x3 Flipout contraction (btx::contract_taps_kernel): algorithmic FLOPs
                (2*2*M*N*K per launch) / the GPU time of the same launches, each launch of the step
                re-issued `reps` times inside a hipGraph and timed with HIP events on the launch stream (no host gaps);
                `per_launch` lists every contraction of the step with its own bound; `achieved_e2e` ties the figure to
                the timed region (all algorithmic FLOPs of a step / ms_per_step).
  cpu_baseline  the reference's op chain on the host cores (rank 0, N=1 only; bounded sample).
  extra         (N=1) the other BASELINE configs through the same code: cfg3 RN18 Reparameterization, cfg4 in f32
                parity mode, cfg2 MLP, cfg5 RN50 Flipout + MOPED bs 128 — ms_per_step, roofline fraction, parity figure.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# dense, /opt/skills/guides/MI355X_MICROARCH.md.  bf16x3 (split-bf16: three bf16 MFMAs per algorithmic product) is priced at a
# third of the bf16 peak: frac = the share of the bf16 matrix rate its MFMAs sustain
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3, "bf16x3": 2500.0 / 3}
HBM_PEAK_TBS = 8.0
PREWARM_STEPS = 12
KL_KNOWN = {("resnet18", False): 55.67487335205078, ("resnet18", True): 89.87570190429688,
            ("resnet50", False): 139.18641662597656, ("resnet50", True): 207.42037963867188}  # reference get_kl_loss, seed 0 (tests/golden/kat.json)
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_delta=0.5)


# ------------------------------------------------------------------------------------------------------------------
# workloads
# ------------------------------------------------------------------------------------------------------------------
def build_model(typ, device, act_dtype, fuse=True, arch="resnet18", moped=False):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import resnet
    torch.manual_seed(0)
    m = getattr(resnet, arch)()
    bt.dnn_to_bnn(m, dict(PRIOR, type=typ, moped_enable=moped))
    m = m.to(device).eval()
    if act_dtype == torch.bfloat16:
        # activations (and the stock BN layers) in bf16; the variational parameters stay f32 (the kernels read
        # mu/rho as f32 and sample in f32)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.to(torch.bfloat16)
    bt.assign_layer_ids(m)
    if fuse and device.type == "cuda":
        # eval-mode BN (+ residual + ReLU) folded into the store of the contraction kernels
        from bayesian_torch_amd.models.fuse import fuse_resnet
        fuse_resnet(m)
    return m


def build_mlp(device):
    """BASELINE cfg2: LinearFlipout MLP 784-512-512-10 (+ReLU)"""
    import bayesian_torch_amd as bt
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(784, 512), torch.nn.ReLU(), torch.nn.Linear(512, 512), torch.nn.ReLU(),
                              torch.nn.Linear(512, 10))
    bt.dnn_to_bnn(net, dict(PRIOR, type="Flipout", moped_enable=False))
    net = net.to(device).eval()
    bt.assign_layer_ids(net)
    return net


# ------------------------------------------------------------------------------------------------------------------
# CPU baseline
# ------------------------------------------------------------------------------------------------------------------
def _cpu_model_string():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(typ, bs, budget_s=24.0):
    """The reference's CPU path on the host cores: oracle/bt_ref.py — the reference's ATen calls on the same plain-layout
    tensors (bit-exact against the reference, tests/test_oracle.py).  Timed twice: all host threads (at most
    OMP_NUM_THREADS when that is set) and capped at 32 (on the 256-thread GPU-box host the uncapped run is slower: serial
    RNG fills + small convs); `value` = the better one."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models.resnet import resnet18
    from oracle import bt_ref
    torch.manual_seed(0)
    m = resnet18()
    bt.dnn_to_bnn(m, dict(PRIOR, type=typ, moped_enable=False))
    m = bt_ref.convert_for_baseline(m).eval()
    torch.manual_seed(1234)
    x = torch.randn(bs, 3, 224, 224)
    ncpu = os.cpu_count() or 1
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:  # the host threads this process is given (a share of a larger host)
        ncpu = min(ncpu, int(omp))
    runs = []
    for cores in sorted({ncpu, min(ncpu, 32)}, reverse=True):
        torch.set_num_threads(cores)
        with torch.no_grad():
            t0 = time.time()
            m(x)
            warm = time.time() - t0
            n, t0 = 0, time.time()
            while True:
                m(x)
                n += 1
                el = time.time() - t0
                if el + el / n > budget_s / 2 - warm or n >= 4:
                    break
        runs.append({"cores": cores, "value": n / el, "timed_forwards": n})
    best = max(runs, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "MC-samples/s", "cores": best["cores"], "kind": "port",
            "cpu": _cpu_model_string(), "host_threads": ncpu, "runs": runs,
            "sample": "%d timed MC forwards (+1 warm-up) per thread count of ResNet18-%s bs%d 224^2 f32, %s" % (
                best["timed_forwards"], typ, bs, "oracle/bt_ref.py ATen op chain on plain-layout weights")}


# ------------------------------------------------------------------------------------------------------------------
# per-launch roofline: record the contraction launches of one step, re-issue each inside a hipGraph
# ------------------------------------------------------------------------------------------------------------------
def record_launches(model, x, sample_idx, lanes=1):
    """the contraction launches of one forward (`lanes` MC samples per launch, as the timed loop issues them)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    recs = []
    orig = BF.contract_hip

    def rec(*a, **k):
        recs.append((a, dict(k)))
        return orig(*a, **k)
    BF.contract_hip = rec
    try:
        with torch.no_grad():
            if lanes > 1:
                bt.set_sample_lanes(model, list(range(sample_idx, sample_idx + lanes)), batch=x.shape[0], presample=True)
            else:
                bt.set_sample_index(model, sample_idx, presample=True)
            model(x)
        torch.cuda.synchronize()
    finally:
        BF.contract_hip = orig
        if lanes > 1:
            bt.set_sample_lanes(model, None)
    # row-fused stems run on a zero-padded geometry (3 -> 4 channels, 7 -> 8 taps per kernel row): their ALGORITHMIC
    # contraction length is the layer's own KH*KW*Cin, not the padded one
    algo_k = {}
    for m in model.modules():
        for plan in (m.__dict__.get("_btx_plans") or {}).values():
            if plan is not None:
                algo_k[id(plan["op"])] = m._op.kernel[1] * plan["kw"] * plan["cin"]
    return recs, algo_k


def time_launches(recs, prec, reps=10, algo_k=None):
    """-> list of dicts (one per contraction launch of the step), GPU time from `reps` re-issues inside one hipGraph"""
    from bayesian_torch_amd import functional as BF
    from bayesian_torch_amd import _lib
    out = []
    dev = recs[0][0][1].device
    side = torch.cuda.Stream(dev)
    for a, k in recs:
        kind, xin, op = a[0], a[1], a[6]
        k = dict(k)
        k["sample_dev"] = None  # plain sample index: the graph below is not an MC graph
        with torch.no_grad():
            with torch.cuda.stream(side):
                y = BF.contract_hip(*a, **k)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(reps):
                    BF.contract_hip(*a, **k)
            g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / (2 * reps) * 1e3
        m_rows = y.numel() // op.out_channels
        if (k.get("epilogue") or {}).get("pool"):  # the stem's max-pool is folded into the launch: y is the pooled tensor,
            sp = (1,) * (3 - op.nd) + tuple(xin.shape[2:])  # the contraction still produces every conv pixel
            osp = op.out_spatial(sp)
            m_rows = y.shape[0] * osp[0] * osp[1] * osp[2]  # y holds every lane; the stem's input may be shared by them
        k_red = op.kernel[0] * op.kernel[1] * op.kernel[2] * (op.in_channels // op.groups)
        k_red = (algo_k or {}).get(id(op), k_red)
        nmm = 2 if kind == _lib.KIND_FLIPOUT else 1
        flops = 2.0 * m_rows * op.out_channels * k_red * nmm
        ep = k.get("epilogue") or {}
        nbytes = (xin.numel() * xin.element_size() + y.numel() * y.element_size() +
                  (y.numel() * y.element_size() if ep.get("residual") is not None else 0) +
                  8 * op.out_channels * k_red * int(k.get("lanes") or 1))
        t_mfma, t_hbm = flops / (MFMA_PEAK_TFLOPS[prec] * 1e12), nbytes / (HBM_PEAK_TBS * 1e12)
        out.append({"launch": "%s k%dx%d s%d cin%d cout%d M%d" % ("flipout" if nmm == 2 else "reparam", op.kernel[1],
                                                                  op.kernel[2], op.stride[2], op.in_channels,
                                                                  op.out_channels, m_rows),
                    "lanes": int(k.get("lanes") or 1), "weights": op.out_channels * k_red,
                    "us": us, "gflop": flops / 1e9, "mbytes": nbytes / 1e6, "tflops": flops / (us * 1e-6) / 1e12,
                    "tbs": nbytes / (us * 1e-6) / 1e12, "bound": "mfma" if t_mfma >= t_hbm else "hbm",
                    "frac": max(t_mfma, t_hbm) / (us * 1e-6),
                    "dominant": bool(op.nd == 2 and op.kernel[1:] == (3, 3) and op.stride[1:] == (1, 1))})
        del g
    return out


def time_sampling(model, lanes, reps=10):
    """GPU time of the weight-sampling launch of one forward (all layers, `lanes` MC samples; the mean tiles cached as in
    the timed loop: BTX_SAMPLE_SKIP_MU), re-issued `reps` times inside a hipGraph -> us per launch"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import rng as _rng
    dev = next(model.parameters()).device
    cache = {}
    side = torch.cuda.Stream(dev)
    with torch.no_grad():
        if lanes > 1:
            bt.set_sample_lanes(model, list(range(7, 7 + lanes)), batch=1)
        with torch.cuda.stream(side):
            _rng.presample(model, 7, cache=cache, skip_mu=False)
            _rng.presample(model, 7, cache=cache, skip_mu=True)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                _rng.presample(model, 7, cache=cache, skip_mu=True)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        for m_ in model.modules():
            if hasattr(m_, "_btx_pre"):
                m_._btx_pre = None
        if lanes > 1:
            bt.set_sample_lanes(model, None)
    return e0.elapsed_time(e1) / (2 * reps) * 1e3


def measure_traffic(lanes=8, timeout_s=240):
    """HBM bytes per LAUNCH of the stride-1 3x3 convolutions of ResNet18 layer1 / layer3 / layer4 (batch 64) the way the
    timed loop runs them — `lanes` MC samples per contraction launch, their weights sampled by one pre-pass launch with
    the mean tiles cached (tools/gpu_diag.py lanes) — from rocprofv3 PMC counters collected now (two passes per shape:
    FETCH_SIZE, WRITE_SIZE; gfx950 correction FETCH x2, MI355X_MICROARCH.md section HBM).  The headline numbers are those of
    layer4 (weights dominate: the worst ratio).  None when rocprofv3 is missing or fails (profiles/pmc_traffic.json then
    holds the last collected numbers)."""
    import glob
    import shutil
    import sqlite3
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    shapes = [("layer4", 512, 7), ("layer3", 256, 14), ("layer1", 64, 56)]
    out = {}
    tmp = tempfile.mkdtemp(prefix="btx_pmc_")
    try:
        for name, ch, hw in shapes:
            vals = {}
            for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
                d = os.path.join(tmp, name + ctr)
                cmd = ["rocprofv3", "--pmc", ctr, "--kernel-trace", "-d", d, "-o", "pmc", "--", sys.executable,
                       os.path.join(ROOT, "tools", "gpu_diag.py"), "lanes", "--prec", "bf16", "--iters", "3",
                       "--lanes", str(lanes), "--shape", "%d,%d,%d,1,3" % (ch, ch, hw)]
                subprocess.run(cmd, cwd=tmp, env=dict(os.environ, TMPDIR=tmp), stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=timeout_s / 6, check=True)
                dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
                con = sqlite3.connect(dbs[0])
                cur = con.cursor()
                tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
                tab = lambda p: [t for t in tabs if t.startswith(p)][0]  # noqa: E731
                ev, disp, sym = tab("rocpd_pmc_event"), tab("rocpd_kernel_dispatch"), tab("rocpd_info_kernel_symbol")
                cols = [c[1] for c in cur.execute("pragma table_info('%s')" % disp)]
                # per dispatch: counter summed over its instances; per kernel: the MINIMUM over dispatches = the steady
                # state (the first sampling call also writes the mean tiles and the sigma cache)
                rows = cur.execute(
                    "select s.kernel_name, min(q.v) from (select d.kernel_id as kid, sum(e.value) as v from '%s' e join '%s' d "
                    "on e.event_id = d.%s group by d.id) q join '%s' s on s.id = q.kid group by s.kernel_name" % (
                        ev, disp, "event_id" if "event_id" in cols else "id", sym)).fetchall()
                vals[ctr] = {kn: v for kn, v in rows if "btx" in kn or "presample" in kn or "splitk" in kn}
            per = {}
            for kn in set(vals.get("FETCH_SIZE", {})) | set(vals.get("WRITE_SIZE", {})):
                short = "contraction" if "taps" in kn else ("sampling" if "presample" in kn else ("splitk" if "splitk" in kn else kn[:40]))
                per[short] = per.get(short, 0.0) + 2.0 * 1024.0 * vals["FETCH_SIZE"].get(kn, 0.0) + 1024.0 * vals["WRITE_SIZE"].get(kn, 0.0)
            if not per:
                return None
            # algorithmic: every lane's input and output once (bf16) + (mu, rho) once per launch (f32)
            algo = lanes * 64 * hw * hw * ch * 2 * 2 + 8 * ch * ch * 9
            out[name] = {"launch": "flipout 3x3 s1 cin%d cout%d %dx%d, batch 64 x %d lanes" % (ch, ch, hw, hw, lanes),
                         "hbm_bytes": sum(per.values()), "by_kernel": per, "algorithmic_bytes": algo,
                         "ratio": sum(per.values()) / algo}
    except Exception:  # noqa
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    l4 = out["layer4"]
    return {"launch": l4["launch"] + " (ResNet18 layer4) incl. its weight-sampling launch", "hbm_bytes": l4["hbm_bytes"],
            "by_kernel": l4["by_kernel"], "algorithmic_bytes": l4["algorithmic_bytes"], "ratio": l4["ratio"],
            "layers": out, "mc_samples_per_launch": lanes,
            "how": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) of tools/gpu_diag.py lanes, steady-state "
                   "dispatch; bytes = 2*1024*FETCH_SIZE + 1024*WRITE_SIZE"}


# ------------------------------------------------------------------------------------------------------------------
# shader clock / package power while the GPU is busy (every fraction here is clock-limited: the chip is power-bound)
# ------------------------------------------------------------------------------------------------------------------
class ClockPowerSampler:
    """polls the amdgpu hwmon files (power1_average / power1_input [uW], freq1_input [Hz]) of the device every 10 ms in a
    thread; falls back to `rocm-smi --showpower --showclocks` (~0.3 s per poll).  Best effort: fields are None when the
    box exposes neither."""

    def __init__(self, index=0):
        import glob
        import threading
        self._stop, self._thr, self.src = threading.Event(), None, None
        # the box's sysfs may list every GPU of the host while only the leased one is visible to HIP: match the PCI address
        # of device `index`; when that cannot be read, sample every card and report the one drawing the most power
        self.cards = []
        for h in sorted(glob.glob("/sys/class/drm/card[0-9]*/device/hwmon/hwmon*")):
            if not os.path.exists(os.path.join(h, "freq1_input")):
                continue
            pf = next((os.path.join(h, n) for n in ("power1_average", "power1_input") if os.path.exists(os.path.join(h, n))), None)
            bdf = os.path.basename(os.path.realpath(os.path.join(h, "..", "..")))
            self.cards.append({"bdf": bdf.lower(), "pfile": pf, "ffile": os.path.join(h, "freq1_input"), "power": [], "sclk": []})
        try:
            pr = torch.cuda.get_device_properties(index)
            want = "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
            hit = [c for c in self.cards if c["bdf"].startswith(want)]
            if hit:
                self.cards = hit
        except Exception:  # noqa
            pass
        if self.cards:
            self.src = "hwmon"
        else:
            import shutil
            if shutil.which("rocm-smi"):
                self.src = "rocm-smi"
                self.cards = [{"bdf": "rocm-smi GPU[0]", "power": [], "sclk": []}]
        self._threading = threading

    def _poll(self):
        import re
        while not self._stop.is_set():
            try:
                if self.src == "hwmon":
                    for c in self.cards:
                        if c["pfile"]:
                            c["power"].append(float(open(c["pfile"]).read()) * 1e-6)
                        c["sclk"].append(float(open(c["ffile"]).read()) * 1e-9)
                    time.sleep(0.01)
                else:
                    o = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True,
                                       timeout=10).stdout
                    m = re.search(r"GPU\[0\].*?Power \(W\):\s*([0-9.]+)", o)
                    if m:
                        self.cards[0]["power"].append(float(m.group(1)))
                    m = re.search(r"GPU\[0\].*?sclk clock level:.*?\((\d+)Mhz\)", o)
                    if m:
                        self.cards[0]["sclk"].append(float(m.group(1)) * 1e-3)
            except Exception:  # noqa
                time.sleep(0.05)

    def __enter__(self):
        if self.src:
            self._thr = self._threading.Thread(target=self._poll, daemon=True)
            self._thr.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        if self._thr is not None:
            self._thr.join(timeout=15)

    def summary(self, skip=0.25):
        """mean over the samples after the first `skip` share of the window (ramp-up); of several cards the busiest"""
        def mean(v):
            v = v[int(len(v) * skip):]
            return sum(v) / len(v) if v else None
        best = None
        for c in self.cards:
            p = mean(c["power"])
            if best is None or (p or 0.0) > (best[0] or 0.0):
                best = (p, mean(c["sclk"]), c)
        if best is None:
            return {"shader_clock_ghz": None, "package_w": None, "source": None, "samples": 0}
        return {"shader_clock_ghz": best[1], "package_w": best[0], "source": self.src, "card": best[2]["bdf"],
                "cards_sampled": len(self.cards), "samples": len(best[2]["sclk"]) or len(best[2]["power"])}


def sustained_run(runner, lanes, dev, seconds=2.0):
    """the timed region's graph replayed back to back for ~`seconds` with the clock/power sampler on: the rate the chip
    holds at its settled clock (the 10 ms timed region starts from an idle-cool package)"""
    n = max(1, lanes)
    idx = list(range(20_000_000, 20_000_000 + n))
    with torch.no_grad():
        runner.zero()
        torch.cuda.synchronize(dev)
        done = 0
        with ClockPowerSampler(dev.index or 0) as smp:
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                for _ in range(8):
                    runner.run(idx)
                    done += n
                torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
        runner.zero()
    out = {"value": done / el, "seconds": el, "mc_samples": done}
    out.update(smp.summary())
    return out


# ------------------------------------------------------------------------------------------------------------------
# the timed MC loop
# ------------------------------------------------------------------------------------------------------------------
class Runner:
    """`steps` MC samples of `model` on `x`: hipGraph replays (`lanes` samples in flight) or eager launches"""

    def __init__(self, model, x, kl, num_classes, lanes, graph, presample=True, sizes=(), concurrent_hint=None,
                 lane_mode="launch", static_input=True):
        from bayesian_torch_amd import mc
        import bayesian_torch_amd as bt
        self.model, self.x, self.kl, self.graphed, self.rest = model, x, kl, None, {}
        self.presample = presample
        if graph:
            try:
                # ragged last groups (counts that are not a multiple of the lane count): one smaller graph per remainder.
                # static_input: the batch is the same for every MC sample, so the stem's input is packed into its kernel
                # layout once per batch (at capture) instead of once per replay
                # keep_logits: each graph's static logits stay reachable (last_logits(); no work added to the replays)
                rests = sorted({s % max(1, lanes) for s in sizes} - {0})
                self.rest = {r: mc.GraphedMC(model, x, kl=kl, lanes=r, concurrent_hint=concurrent_hint, lane_mode=lane_mode,
                                             static_input=static_input, keep_logits=True) for r in rests}
                self.graphed = mc.GraphedMC(model, x, kl=kl, lanes=max(1, lanes), concurrent_hint=concurrent_hint,
                                            lane_mode=lane_mode, static_input=static_input, keep_logits=True)
            except Exception as e:  # a runtime that cannot capture: measure the eager path rather than nothing
                print("bench: hipGraph capture failed (%s: %s) - falling back to eager launches" % (type(e).__name__, e),
                      file=sys.stderr)
                self.graphed = None
                for m_ in model.modules():
                    if hasattr(m_, "_btx_sample_dev"):
                        m_._btx_sample_dev = None
                torch.cuda.synchronize(x.device)
        if self.graphed is not None:
            self.packed = self.graphed.packed
        else:
            self.packed = torch.zeros(mc.packed_numel(x.shape[0], num_classes), dtype=torch.float32, device=x.device)
        self._bt, self._mc = bt, mc

    def run(self, indices):
        if self.graphed is None:
            for i in indices:
                self._bt.set_sample_index(self.model, i, presample=self.presample and self.x.is_cuda)
                if self.x.is_cuda:
                    logits = self.model(self.x)
                else:  # ATen route (dry run): torch's generator keyed on the sample index, as mc.mc_forward does
                    with torch.random.fork_rng(devices=[]):
                        torch.default_generator.manual_seed(self._bt.rng.cpu_sample_seed(i))
                        logits = self.model(self.x)
                self._mc.accumulate(self.packed, logits, self.kl)
            return
        g = self.graphed
        full = len(indices) // g.lanes * g.lanes
        for i in range(0, full, g.lanes):
            g.run(indices[i]) if g.lanes == 1 else g.run_many(indices[i:i + g.lanes])
        rest = indices[full:]
        if rest:
            gr = self.rest[len(rest)]
            gr.run(rest[0]) if gr.lanes == 1 else gr.run_many(rest)

    def last_logits(self, n):
        """the logits of the last MC sample of a run(indices) with len(indices) == n (None on the eager path)"""
        if self.graphed is None:
            return None
        return self.rest.get(n % self.graphed.lanes, self.graphed).lane_logits[-1]

    def zero(self):
        self.packed.zero_()
        for gr in self.rest.values():
            gr.packed.zero_()

    def fold(self):
        for gr in self.rest.values():
            self.packed.add_(gr.packed)

    def close(self):
        if self.graphed is not None:
            self.graphed.close()
            for gr in self.rest.values():
                gr.close()


def timed_mc(runner, my_indices, warm_indices, world, dev, repeats=1, min_seconds=0.0):
    """The timed region — EXACTLY len(my_indices) MC samples between barrier + synchronize on both sides — run `repeats` times, and
    on until the regions add up to `min_seconds`: a 20-step region is ~10 ms of GPU time, the package's clock / power management
    settles over hundreds of ms.  Every rank runs the same number of regions (the count follows the slowest rank's first region).
    Returns the per-region times (max over ranks)."""
    def barrier():
        if world > 1:
            dist.barrier()
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
    runs = []
    with torch.no_grad():
        grouped = dist.is_available() and dist.is_initialized()  # also a 1-rank group (torchrun --nproc-per-node 1)
        runner.run(warm_indices)
        if grouped:
            dist.all_reduce(runner.packed)  # warm the communicator too

        def region():
            runner.zero()
            barrier()
            t0 = time.perf_counter()
            runner.run(my_indices)
            runner.fold()
            if grouped:
                dist.all_reduce(runner.packed, op=dist.ReduceOp.SUM)
            barrier()
            runs.append(time.perf_counter() - t0)
        region()
        n = max(1, repeats)
        if min_seconds > 0:
            t1 = torch.tensor([runs[0]], dtype=torch.float64, device=dev)
            if world > 1:
                dist.all_reduce(t1, op=dist.ReduceOp.MAX)
            n = max(n, min(2000, int(min_seconds / max(float(t1[0]), 1e-6)) + 1))
        for _ in range(n - 1):
            region()
    t = torch.tensor(runs, dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)  # per region: the slowest rank
    return [float(v) for v in t]


def settled(runs):
    """the figure a list of back-to-back regions reports: the median of its second half (the first half carries the clock ramp of a
    package that was idle a moment ago); fewer than 8 regions: the median of all"""
    tail = sorted(runs[len(runs) // 2:]) if len(runs) >= 8 else sorted(runs)
    return tail[len(tail) // 2]


def logits_parity(model_fn, x, prec, sample=3):
    """rel-L2 of the logits of the benched configuration (prec, fused epilogues, presampled weights) against the
    UNFUSED f32-parity-mode op chain of the same parameters with the same MC sample index (same BTX-RNG noise)"""
    import bayesian_torch_amd as bt
    dev = x.device
    with torch.no_grad():
        bt.set_precision(prec)
        m = model_fn(True, torch.bfloat16 if prec == "bf16" else torch.float32)
        bt.set_sample_index(m, sample, presample=True)
        y = m(x.to(torch.bfloat16 if prec == "bf16" else torch.float32)).float()
        del m
        bt.set_precision("f32")
        r = model_fn(False, torch.float32)
        bt.set_sample_index(r, sample)
        ref = r(x.float()).float()
        del r
        bt.set_precision(prec)
    torch.cuda.synchronize(dev)
    return float((y - ref).norm() / ref.norm())


def run_resnet_config(arch, typ, prec, bs, moped, steps, warmup, lanes, dev, world=1, rank=0, graph=True, fuse=True,
                      presample=True, scaling="weak", total=None, per_launch=True, parity=False, prewarm=PREWARM_STEPS,
                      concurrent_hint=None, lane_mode="launch", repeats=5, sustain=0.0, min_seconds=0.0):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    bt.manual_seed(2024)
    bt.set_precision(prec)
    act_dtype = torch.bfloat16 if prec == "bf16" else torch.float32
    model = build_model(typ, dev, act_dtype, fuse=fuse, arch=arch, moped=moped)
    torch.manual_seed(1234)
    x = torch.randn(bs, 3, 224, 224).to(dev).to(act_dtype)
    with torch.no_grad():
        kl = float(bt.get_kl_loss(model))
    if scaling == "strong":
        mine = list(range(rank, total, world))
        n_global = total
    else:
        mine = [k * world + rank for k in range(steps)]
        n_global = steps * world
    nwarm = prewarm + warmup
    if graph and lanes > 1:  # whole replays (the warm-up is not timed; a ragged one would only capture one more graph)
        nwarm = -(-nwarm // lanes) * lanes
    warm = [10_000_000 + w * world + rank for w in range(nwarm)]
    runner = Runner(model, x, kl, 1000, lanes, graph, presample, sizes=(len(mine), len(warm)), concurrent_hint=concurrent_hint,
                    lane_mode=lane_mode)
    runs = timed_mc(runner, mine, warm, world, dev, repeats=repeats, min_seconds=min_seconds)
    elapsed = settled(runs)  # median of the settled half of the back-to-back regions; the first five are listed, the rest summarised
    stats = runner.packed.clone()
    last = runner.last_logits(len(mine)) if mine else None
    last = None if last is None else last.float().cpu()
    lanes_used = runner.graphed.lanes if runner.graphed is not None else 0
    sustained = None
    if sustain and dev.type == "cuda" and world == 1 and runner.graphed is not None:
        sustained = sustained_run(runner, lanes_used, dev, seconds=sustain)
    runner.close()
    u = mc.unpack(stats, bs, 1000)
    if last is not None:
        u["last_logits"] = last
    assert abs(float(u["samples"]) - n_global) < 0.5, "work was skipped inside the timed region"
    assert torch.isfinite(u["mean_prob"]).all()
    res = {"elapsed": elapsed, "n_global": n_global, "per_rank": len(mine), "kl": kl, "lanes": lanes_used,
           "lane_mode": lane_mode if lanes_used > 1 else "single",
           "ms_per_step": 1e3 * elapsed / max(len(mine), 1), "value": n_global / elapsed,
           "ms_per_step_runs": [1e3 * r / max(len(mine), 1) for r in runs[:5]], "timed_regions": len(runs),
           "timed_seconds": sum(runs),
           "ms_per_step_all_regions": {"min": 1e3 * min(runs) / max(len(mine), 1), "max": 1e3 * max(runs) / max(len(mine), 1),
                                       "mean": 1e3 * sum(runs) / len(runs) / max(len(mine), 1)},
           "outputs": u}  # the statistics of the last timed region (not part of the JSON result)
    if sustained is not None:
        res["sustained"] = sustained
    known = KL_KNOWN.get((arch, moped))
    if known:
        res["kl_rel_err"] = abs(kl - known) / known
    if per_launch and dev.type == "cuda":
        # the launches as the timed loop issues them: `ll` MC samples per launch when the lanes ride inside the launch
        ll = lanes_used if (lanes_used > 1 and lane_mode == "launch") else 1
        recs, algo_k = record_launches(model, x, 7, lanes=ll)
        table = time_launches(recs, prec, algo_k=algo_k)
        # the sampling launch of the same forward (one launch for all layers and lanes), charged to each contraction by
        # its share of the weights: a contraction's roofline figure counts the sampling that feeds it
        samp_us = time_sampling(model, ll) if presample else 0.0
        wsum = float(sum(r["weights"] for r in table)) or 1.0
        for r in table:
            r["sampling_us"] = samp_us * r["weights"] / wsum
            r["frac_incl_sampling"] = r["frac"] * r["us"] / (r["us"] + r["sampling_us"])
        dom = [r for r in table if r["dominant"]] or table
        res["per_launch"] = table
        res["launch_lanes"] = ll
        res["sampling_us_per_launch"] = samp_us
        res["gflop_per_step"] = sum(r["gflop"] for r in table) / ll
        res["kernel_us_per_step"] = (sum(r["us"] for r in table) + samp_us) / ll
        dom_us = sum(r["us"] for r in dom)
        dom_samp = sum(r["sampling_us"] for r in dom)
        res["dominant_tflops_contraction_only"] = sum(r["gflop"] for r in dom) / dom_us * 1e3  # GFLOP/us = 1e15 FLOP/s
        res["dominant_tflops"] = sum(r["gflop"] for r in dom) / (dom_us + dom_samp) * 1e3
        res["dominant_avg_us"] = dom_us / len(dom)
        res["dominant_sampling_us"] = dom_samp / len(dom)
        res["dominant_n"] = len(dom)
        res["achieved_e2e_tflops"] = res["gflop_per_step"] / res["ms_per_step"]
    if parity and dev.type == "cuda":
        del model
        res["logits_rel_l2_vs_unfused_f32"] = logits_parity(
            lambda fz, dt: build_model(typ, dev, dt, fuse=fz, arch=arch, moped=moped), x, prec)
    return res


def run_mlp_config(dev, steps=8):
    """BASELINE cfg2: 3-layer LinearFlipout MLP, batch 256, 8 MC samples (latency-bound: ~0.7 GFLOP per sample)"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    bt.manual_seed(2024)
    bt.set_precision("bf16")
    net = build_mlp(dev)
    torch.manual_seed(1234)
    x = torch.randn(256, 784, device=dev).to(torch.bfloat16)
    kl = float(bt.get_kl_loss(net).detach())
    def timed(lanes):
        g = mc.GraphedMC(net, x, kl=kl, lanes=lanes)
        run = (lambda base: [g.run(base + s) for s in range(steps)]) if lanes == 1 else (
            lambda base: [g.run_many(list(range(base + k, base + k + lanes))) for k in range(0, steps, lanes)])
        with torch.no_grad():
            run(1000)
            els = []
            for _ in range(5):  # the region is < 1 ms: five of them, the median (one host hiccup is 40x the region)
                g.packed.zero_()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(0)
                torch.cuda.synchronize(dev)
                els.append(time.perf_counter() - t0)
            n = float(mc.unpack(g.packed, 256, 10)["samples"])
            assert abs(n - steps) < 0.5, "cfg2: work was skipped inside the timed region"
        g.close()
        return sorted(els)[len(els) // 2]
    # the 8 MC samples of the config as lanes of ONE launch per layer (one replay per region) — and, for reference, one sample per
    # replay (4 launches of ~20 us each per sample: pure launch-to-launch latency)
    el1 = timed(1)
    el = timed(steps)
    with torch.no_grad():
        # parity figure: bf16 logits vs the f32 parity mode, same sample index
        bt.set_sample_index(net, 3)
        y = net(x).float()
        bt.set_precision("f32")
        bt.set_sample_index(net, 3)
        ref = net(x.float()).float()
        bt.set_precision("bf16")
    gflop = 2 * 2 * 256 * (784 * 512 + 512 * 512 + 512 * 10) / 1e9
    return {"workload": "cfg2: LinearFlipout MLP 784-512-512-10, batch 256, %d MC samples as lanes of one hipGraph replay, bf16" % steps,
            "ms_per_step": 1e3 * el / steps, "value": steps / el, "unit": "MC-samples/s",
            "value_one_sample_per_replay": steps / el1,
            "achieved_e2e_tflops": gflop / (1e3 * el / steps), "bound": "latency (5 launches, 0.7 GFLOP, 7 MB per sample)",
            "logits_rel_l2_vs_f32_mode": float((y - ref).norm() / ref.norm())}


def run_train_step(dev, steps=5):
    """reference README.md:114-125 on the HIP backend: forward + cross-entropy + KL/batch + backward of
    dnn_to_bnn(ResNet18) Flipout, batch 64, bf16 activations (eager launches; weight gradients on the exact-f32 MFMA)"""
    import bayesian_torch_amd as bt
    bt.manual_seed(2024)
    bt.set_precision("bf16")
    model = build_model("Flipout", dev, torch.bfloat16, fuse=False).train()
    from bayesian_torch_amd.models.fuse import hip_batchnorm
    hip_batchnorm(model)  # training-mode BatchNorm through libbtx (csrc/btx_bn.hip); the f32 parity reference below keeps torch's
    torch.manual_seed(1234)
    x = torch.randn(64, 3, 224, 224, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 1000, (64,), device=dev)
    step_no = [0]

    def step():
        for p_ in model.parameters():
            p_.grad = None
        # one sampling launch for the forward of all 21 layers instead of one small pre-pass per layer
        bt.set_sample_index(model, step_no[0], presample=True)
        step_no[0] += 1
        out = model(x)
        loss = torch.nn.functional.cross_entropy(out.float(), y) + bt.get_kl_loss(model) / 64
        loss.backward()
        return loss
    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize(dev)
    ms_eager = 1e3 * (time.perf_counter() - t0) / steps
    loss_finite = bool(torch.isfinite(loss))
    del loss  # the eager step's autograd graph must be gone before the capture (its AccumulateGrad nodes live on this stream)
    for p_ in model.parameters():
        p_.grad = None
    # the same step captured once into a hipGraph (autograd.GraphedTrainStep: the MC sample index lives in a device word): an eager
    # step is ~590 launches dispatched by Python / ATen and bound by the host
    ms, graphed = ms_eager, None
    try:
        from bayesian_torch_amd.autograd import GraphedTrainStep
        gs = GraphedTrainStep(model, x, y)
        for i in range(2):
            gs.run(100 + i)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(max(steps, 10)):
            gl = gs.run(200 + i)
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0) / max(steps, 10)
        loss_finite = loss_finite and bool(torch.isfinite(gl))
        graphed = True
        gs.close()
    except Exception as e:  # noqa — a runtime that cannot capture: the eager figure stands
        graphed = "capture failed: %s: %s" % (type(e).__name__, e)
    # parity figure: the same step (same parameters, same MC sample index => same BTX-RNG noise) in f32 parity mode —
    # loss and the weight gradients of the first convolution, a layer3 convolution and the classifier
    def grads(m, xin):
        for p_ in m.parameters():
            p_.grad = None
        bt.set_sample_index(m, 11)
        out = m(xin)
        loss_ = torch.nn.functional.cross_entropy(out.float(), y) + bt.get_kl_loss(m) / 64
        loss_.backward()
        picks = [m.conv1, m.layer3[0].conv1, m.fc]
        return float(loss_), [l_._w()[0].grad.detach().float().clone() for l_ in picks], [l_._w()[1].grad.detach().float().clone() for l_ in picks]
    parity = None
    try:
        l16, gm16, gr16 = grads(model, x)
        bt.set_precision("f32")
        ref = build_model("Flipout", dev, torch.float32, fuse=False).train()
        l32, gm32, gr32 = grads(ref, x.float())
        rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
        cos = lambda a, b: float((a * b).sum() / (a.norm() * b.norm()))  # noqa: E731
        parity = {"reference": "the same step in f32 parity mode (f32 activations, v_mfma_f32_32x32x2_f32), same sample index; "
                               "a whole-model figure: bf16 activations flip ReLU gates of a random-init 18-layer net, so the "
                               "early layers' gradients differ by tens of percent while the directions agree (cosine) — the "
                               "kernels themselves are pinned per layer at 1e-4 by tests/test_gpu_backward.py",
                  "dmu_cosine": {n: cos(a, b) for n, a, b in zip(("conv1", "layer3.0.conv1", "fc"), gm16, gm32)},
                  "loss_rel_err": abs(l16 - l32) / abs(l32),
                  "dmu_rel_l2": {n: rel(a, b) for n, a, b in zip(("conv1", "layer3.0.conv1", "fc"), gm16, gm32)},
                  "drho_rel_l2": {n: rel(a, b) for n, a, b in zip(("conv1", "layer3.0.conv1", "fc"), gr16, gr32)}}
        del ref
    except Exception as e:  # noqa
        parity = {"error": "%s: %s" % (type(e).__name__, e)}
    finally:
        bt.set_precision("bf16")
    # forward 464.4 + data gradient 434.2 (no dx for the stem) + weight gradient 464.4 GFLOP (Flipout: two contractions
    # each; the stem counted with its own 7x7x3 taps, not the padded row-fused geometry)
    gflop = 464.4 + (464.4 - 30.2) + 464.4
    return {"workload": "training step (README.md:114-125): dnn_to_bnn(ResNet18) Flipout bs64, bf16 activations, forward + "
                        "CE + KL/B + backward through libbtx (bf16-MFMA weight gradients through chunk slabs, HIP BatchNorm with the blocks' residual add + ReLU, HIP max-pool), one hipGraph replay per step (ms_per_step_eager: launched from Python)",
            "ms_per_step": ms, "ms_per_step_eager": ms_eager, "hipgraph": graphed, "achieved_tflops": gflop / ms,
            "loss_finite": loss_finite,
            "parity_vs_f32_mode": parity}


def run_train_step_isolated(timeout_s=420):
    cmd = [sys.executable, os.path.abspath(__file__), "--train-step-only"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, cwd=ROOT)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and lines:
            return json.loads(lines[-1])
        return {"error": "train-step subprocess rc %d: %s" % (r.returncode, (r.stderr or "")[-300:])}
    except Exception as e:  # noqa
        return {"error": "%s: %s" % (type(e).__name__, e)}


def summarise_extra(name, r, prec, table=False):
    peak = MFMA_PEAK_TFLOPS[prec]
    out = {"workload": name, "ms_per_step": r["ms_per_step"], "value": r["value"], "unit": "MC-samples/s", "dtype": prec,
           "kl": r["kl"], "lanes": r["lanes"], "lane_mode": r.get("lane_mode"), "ms_per_step_runs": r.get("ms_per_step_runs")}
    for k in ("kl_rel_err", "logits_rel_l2_vs_unfused_f32"):
        if k in r:
            out[k] = r[k]
    if "per_launch" in r:
        out.update({"gflop_per_step": r["gflop_per_step"], "achieved_e2e_tflops": r["achieved_e2e_tflops"],
                    "frac_e2e": r["achieved_e2e_tflops"] / peak, "dominant_kernel_tflops": r["dominant_tflops"],
                    "dominant_kernel_frac": r["dominant_tflops"] / peak, "kernel_us_per_step": r["kernel_us_per_step"]})
        if table:  # launches of a forward grouped by shape: count, time per launch, share of its own bound
            rows = {}
            for pl in r["per_launch"]:
                g = rows.setdefault(pl["launch"], {"launch": pl["launch"], "count": 0, "us": 0.0, "gflop": pl["gflop"],
                                                   "bound": pl["bound"], "frac": 0.0, "lanes": pl.get("lanes")})
                g["count"] += 1
                g["us"] += pl["us"]
                g["frac"] += pl.get("frac_incl_sampling", pl["frac"])
            out["per_launch"] = [dict(g, us=round(g["us"] / g["count"], 2), frac=round(g["frac"] / g["count"], 3),
                                      share_of_kernel_time=round(g["us"] / sum(q["us"] for q in rows.values()), 3))
                                 for g in rows.values()]
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, outputs):
    """mc.unpack statistics (+ last_logits) -> path/<name>.npy (float32).  Per-example arrays larger than DUMP_LIMIT_BYTES
    in all keep a fixed, seeded sample of their rows (the same rows in every array, listed in path/rows.npy)."""
    import numpy as np
    arrs = {k: v.detach().float().cpu().numpy() for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_LIMIT_BYTES:
        bs = arrs["mean_prob"].shape[0]
        keep = max(1, int(bs * DUMP_LIMIT_BYTES * 0.9 / total))
        rows = np.sort(np.random.default_rng(0).choice(bs, keep, replace=False))
        arrs = {k: (a[rows] if a.ndim and a.shape[0] == bs else a) for k, a in arrs.items()}
        arrs["rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(path, k + ".npy"), a)


def auto_lanes(steps, cap=32):
    """MC samples per hipGraph replay: the whole timed region when it fits, else its largest divisor <= cap (>= 8), else 16"""
    if steps <= cap:
        return max(1, steps)
    for d in range(cap, 7, -1):
        if steps % d == 0:
            return d
    return 16


# ------------------------------------------------------------------------------------------------------------------
# the final stdout line: compact (the driver parses ONE line and keeps an 8 KB stdout tail); the tables go to a file
# ------------------------------------------------------------------------------------------------------------------
LINE_LIMIT = 6144
DETAIL_PATH = os.path.join(ROOT, "gpurun_out", "bench_detail.json")


def _sig(v, n=5):
    """floats to n significant digits (keeps the line short), containers recursively"""
    if isinstance(v, str):
        return v if len(v) <= 360 else v[:357] + "..."
    if isinstance(v, bool) or v is None or isinstance(v, int):
        return v
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None
        return float("%.*g" % (n, v))
    if isinstance(v, dict):
        return {k: _sig(x, n) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, n) for x in v]
    return v


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact_line(out):
    """full result dict -> the ONE JSON line rank 0 prints last (<= LINE_LIMIT bytes).  Carries the contract keys, `roofline`
    (incl. traffic ratio, clock/power, the readings inside north_star's 1e-4) and `cpu_baseline`; per-launch tables,
    traffic breakdowns and prose stay in gpurun_out/bench_detail.json (also echoed to stderr)."""
    top = ("metric", "value", "unit", "n_gpus", "rccl_ranks", "steps", "warmup", "ms_per_step", "ms_per_step_runs",
           "timed_regions", "timed_seconds", "ms_per_step_all_regions",
           "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "dry_run", "total_samples", "collective",
           "kl_rel_err", "logits_rel_l2_vs_unfused_f32", "gpu_over_cpu", "sustained")
    line = {k: out[k] for k in top if k in out}
    cfg = out.get("config") or {}
    line["config"] = _pick(cfg, ("workload", "global_batch", "parallelism"))
    rf = out.get("roofline")
    if rf:
        r = _pick(rf, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_name", "achieved_contraction_only",
                       "frac_contraction_only", "avg_launch_us", "avg_sampling_share_us", "mc_samples_per_launch",
                       "launches_per_forward", "achieved_e2e", "frac_e2e", "shader_clock_ghz", "package_w",
                       "frac_min_dominant_row", "rows"))
        r.setdefault("traffic", None)
        td = rf.get("traffic_detail") or {}
        if td:
            r["algorithmic_bytes"] = td.get("algorithmic_bytes")
            r["traffic_ratio"] = td.get("ratio")
            r["traffic_launch"] = "layer4 3x3 s1 512ch 7x7 (worst ratio) incl. sampling"
            lay = td.get("layers") or {}
            r["traffic_ratio_by_layer"] = {k: v.get("ratio") for k, v in lay.items()}
            r["traffic_source"] = "this run" if (rf.get("traffic_source") or "").startswith("measured") else "profiles/pmc_traffic.json"
        modes = rf.get("modes_within_1e-4") or {}
        if modes:
            r["modes_within_1e-4"] = {m: _pick(v, ("value", "logits_rel_l2", "dominant_kernel_frac", "peak", "frac_e2e"))
                                      for m, v in modes.items()}
        line["roofline"] = r
    else:
        line["roofline"] = None
    cb = out.get("cpu_baseline")
    line["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "cpu", "host_threads", "sample")) if cb else None
    ex = out.get("extra")
    if ex:
        e2 = {}
        for k, v in ex.items():
            if not isinstance(v, dict):
                e2[k] = v  # "error": "..."
                continue
            short = {"cfg4_strong_shape_4_per_rank": "strong_shape", "cfg4_f32_parity_mode": "cfg4_f32"}.get(k, k)
            e2[short] = _pick(v, ("value", "ms_per_step", "frac_e2e", "dominant_kernel_frac", "kl_rel_err",
                                  "logits_rel_l2_vs_unfused_f32", "logits_rel_l2_vs_f32_mode", "vs_weak_region",
                                  "achieved_tflops", "hbm_rows_min_frac", "lanes", "ms_per_step_eager", "value_one_sample_per_replay"))
        line["extra"] = e2
    line["detail"] = "gpurun_out/bench_detail.json"
    line = _sig(line)
    s = json.dumps(line, separators=(",", ":"))
    # belt and braces: shed optional blocks until the line fits
    for drop in (("extra",), ("roofline", "rows"), ("roofline", "traffic_ratio_by_layer"), ("ms_per_step_runs",)):
        if len(s) <= LINE_LIMIT:
            break
        tgt = line
        for k in drop[:-1]:
            tgt = tgt.get(k) or {}
        tgt.pop(drop[-1], None)
        s = json.dumps(line, separators=(",", ":"))
    return s


def emit(out):
    """detail -> gpurun_out/bench_detail.json + stderr; the compact line -> stdout, LAST"""
    try:
        os.makedirs(os.path.dirname(DETAIL_PATH), exist_ok=True)
        with open(DETAIL_PATH, "w") as f:
            json.dump(out, f, indent=1)
    except OSError as e:
        print("bench: could not write %s (%s)" % (DETAIL_PATH, e), file=sys.stderr)
    print("bench detail: " + json.dumps(out), file=sys.stderr)
    sys.stderr.flush()
    print(compact_line(out))
    sys.stdout.flush()


# ------------------------------------------------------------------------------------------------------------------
def self_launch(n, argv, dry_run):
    """re-exec under torch.distributed.run with one rank per GPU (rendezvous on 127.0.0.1, a free port)"""
    if not dry_run:
        have = torch.cuda.device_count()
        if have < n:
            print("bench.py --gpus %d: only %d GPU(s) visible - refusing to run (a line with fewer ranks than asked for "
                  "would misreport n_gpus)" % (n, have), file=sys.stderr)
            return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n, "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def dry_run(args, world, rank):
    """CPU / gloo rehearsal of the multi-rank protocol (launch, sharding, the one all-reduce, max-over-ranks timing) on a
    small LinearFlipout model through the ATen route.  NOT a measurement: the line says dry_run = true."""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    bt.manual_seed(2024)
    dev = torch.device("cpu")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.ReLU(), torch.nn.Linear(16, 10))
    bt.dnn_to_bnn(net, dict(PRIOR, type="Flipout", moped_enable=False))
    net.eval()
    bt.assign_layer_ids(net)
    torch.manual_seed(1234)
    x = torch.randn(8, 32)
    runner = Runner(net, x, 0.0, 10, 1, graph=False, presample=False)
    if args.scaling == "strong":  # S samples over the ranks: {s : s mod R == r}, ragged when R does not divide S
        mine = list(range(rank, args.total_samples, world))
        n_global = args.total_samples
        per_rank = len(range(0, args.total_samples, world))  # rank 0 holds the largest share
    else:
        mine = [k * world + rank for k in range(args.steps)]
        n_global, per_rank = args.steps * world, args.steps
    elapsed = timed_mc(runner, mine, [10_000 + rank], world, dev)[0]
    u = mc.unpack(runner.packed, 8, 10)
    if rank == 0:
        assert abs(float(u["samples"]) - n_global) < 0.5
        # the merged statistics must be those of ONE process evaluating the same sample set (rank-count independence)
        ref = Runner(net, x, 0.0, 10, 1, graph=False, presample=False)
        with torch.no_grad():
            ref.run(sorted(set(range(n_global)) if args.scaling == "strong" else
                           {k * world + r for k in range(args.steps) for r in range(world)}))
        merged_ok = bool(torch.allclose(ref.packed, runner.packed, rtol=1e-5, atol=1e-6))
        assert merged_ok, "sharded statistics differ from the single-process ones"
        print(json.dumps({"metric": "MC-samples/sec (DRY RUN: CPU/gloo protocol rehearsal, not a measurement)",
                          "dry_run": True, "value": n_global / elapsed, "unit": "MC-samples/s",
                          "n_gpus": world, "rccl_ranks": dist.get_world_size() if world > 1 else 1, "steps": per_rank,
                          "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / per_rank, "higher_is_better": True,
                          "scaling": args.scaling, "total_samples": n_global, "merged_equals_single_process": merged_ok,
                          "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": "dry run: LinearFlipout 32-16-10 on CPU", "parallelism":
                                     "mc-sample-shard x%d (gloo)" % world}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--type", default="Flipout", choices=["Flipout", "Reparameterization"])
    ap.add_argument("--arch", default="resnet18", choices=["resnet18", "resnet50"])
    ap.add_argument("--moped", action="store_true", help="dnn_to_bnn(..., moped_enable=True, moped_delta=0.5)")
    ap.add_argument("--prec", default="bf16", choices=["bf16", "f32", "bf16x3"], help="bf16: bf16 activations + bf16 MFMA "
                    "(headline); f32: exact f32 MFMA (parity mode); bf16x3: f32 activations, split-bf16 operands, three bf16 "
                    "MFMAs per product (the 1e-4-tolerance throughput mode)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--total-samples", type=int, default=32, help="--scaling strong: MC samples sharded over the ranks "
                    "(BASELINE cfg4: 32 over 8 GPUs)")
    ap.add_argument("--no-fuse", action="store_true", help="keep BatchNorm/ReLU/residual as separate torch ops")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel of every MC sample from Python")
    ap.add_argument("--lanes", type=int, default=0, help="MC samples evaluated by one hipGraph replay (lanes of one launch "
                    "per layer); independent noise, identical results to one at a time.  0 (default): as many as the timed "
                    "region holds, up to 32 — a launch of 20 lanes has 2.5x the tiles of one of 8: its ramp-up and its last, "
                    "partly filled round of workgroups weigh less (measured: 4 / 8 / 16 lanes = 0.377 / 0.382 / 0.406 of the MFMA "
                    "peak on the dominant kernel)")
    ap.add_argument("--lane-mode", default="launch", choices=["launch", "streams"], help="launch: the samples of a replay "
                    "are lanes of ONE launch per layer (btx_contract_fwd_lanes); streams: one launch per (layer, sample), "
                    "each sample on its own stream (the round-2 form)")
    ap.add_argument("--full", action="store_true", help="measure what the headline does not need as well: settled "
                    "back-to-back regions (the defaults of --repeats / --settle-seconds become 5 / 1.0), the per-launch "
                    "roofline and its rocprofv3 traffic, the 2 s sustained replay, the logits parity, the other BASELINE "
                    "configs (extra) and the CPU baseline; the --no-* options below leave parts of it out")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the predictive statistics of the timed "
                    "region (mean_prob, var_prob, predictive_entropy, mutual_information, kl, samples) and the logits of its "
                    "last MC sample (last_logits) as DIR/<name>.npy, float32")
    ap.add_argument("--repeats", type=int, default=None, help="the timed region (the same --steps MC samples) is run at least this "
                    "many times, back to back (default 1; 5 with --full)")
    ap.add_argument("--settle-seconds", type=float, default=None, help="...and on until the regions add up to this long: value / "
                    "ms_per_step are the median of the SECOND half of the regions (settled clock); ms_per_step_runs lists the "
                    "first five, ms_per_step_all_regions min / max / mean of all (default 0; 1.0 with --full)")
    ap.add_argument("--no-presample", action="store_true")
    ap.add_argument("--latency-plan", action="store_true", help="A/B: plan every launch for its own latency (split-K to fill "
                    "idle CUs) although several MC samples are in flight")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-launch-timing", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the cfg2/cfg3/cfg5/f32 sub-results")
    ap.add_argument("--no-traffic", action="store_true", help="skip the rocprofv3 PMC traffic measurement")
    ap.add_argument("--no-sustain", action="store_true", help="skip the ~2 s back-to-back replay with the clock/power sampler")
    ap.add_argument("--no-stem-pool", action="store_true", help="A/B: the stem's max-pool as its own kernel instead of folded "
                    "into the stem launch (BtxEpilogue.pool)")
    ap.add_argument("--dry-run", action="store_true", help="CPU/gloo rehearsal of the multi-rank protocol (no GPU)")
    ap.add_argument("--train-step-only", action="store_true", help="print the extra.train_step result (JSON) and exit")
    args = ap.parse_args()

    if args.train_step_only:
        print(json.dumps(run_train_step(torch.device("cuda", 0))))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:], args.dry_run))

    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if args.settle_seconds is None:
        args.settle_seconds = 1.0 if args.full else 0.0
    if args.lanes <= 0:
        per_rank = args.steps if args.scaling == "weak" else max(1, -(-args.total_samples // max(1, args.gpus)))
        args.lanes = auto_lanes(per_rank)
    if args.no_stem_pool:
        from bayesian_torch_amd.models import fuse as _fuse
        _fuse.STEM_POOL_FUSION = False
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("bench.py: --gpus %d but the process group has %d rank(s): launch with --nproc-per-node == --gpus (or let "
              "bench.py launch the ranks itself: python bench.py --gpus N)" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    if args.dry_run:
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
        dry_run(args, world, rank)
        if world > 1:
            dist.destroy_process_group()
        return

    assert torch.cuda.is_available(), "bench.py needs a GPU (the product path has no CPU fallback); --dry-run rehearses " \
                                      "the multi-rank protocol on CPU"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    rccl_ranks = 1
    grouped = world > 1 or ("WORLD_SIZE" in os.environ and "MASTER_PORT" in os.environ)  # launched by torch.distributed.run
    if grouped:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)  # RCCL on ROCm
        rccl_ranks = dist.get_world_size()
        assert rccl_ranks == args.gpus

    head = run_resnet_config(args.arch, args.type, args.prec, args.batch, args.moped, args.steps, args.warmup, args.lanes,
                             dev, world, rank, graph=not args.no_graph, fuse=not args.no_fuse,
                             presample=not args.no_presample, scaling=args.scaling, total=args.total_samples,
                             per_launch=args.full and not args.no_launch_timing and rank == 0,
                             concurrent_hint=False if args.latency_plan else None,
                             parity=(args.full and rank == 0 and world == 1 and not args.no_extras), lane_mode=args.lane_mode,
                             repeats=args.repeats, sustain=2.0 if args.full and not args.no_sustain else 0.0,
                             min_seconds=args.settle_seconds)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, head["outputs"])
    if rank == 0:
        peak = MFMA_PEAK_TFLOPS[args.prec]
        roofline = None
        if "per_launch" in head:
            traffic = None
            if world == 1 and not args.no_traffic and args.arch == "resnet18" and args.prec == "bf16":
                traffic = measure_traffic(lanes=head["launch_lanes"])
            tsrc = "measured in this run"
            if traffic is None:
                tfile = os.path.join(ROOT, "profiles", "pmc_traffic.json")
                if os.path.exists(tfile):
                    try:
                        traffic = json.load(open(tfile))
                        tsrc = "profiles/pmc_traffic.json (rocprofv3 not run in this invocation)"
                    except Exception:  # noqa
                        traffic = None
            roofline = {
                "bound": "mfma", "achieved": head["dominant_tflops"], "peak": peak, "unit": "TFLOP/s",
                "frac": head["dominant_tflops"] / peak,
                "traffic": (traffic or {}).get("hbm_bytes"), "traffic_detail": traffic, "traffic_source": tsrc,
                "kernel": "btx::contract_taps_kernel<%s,%s,3,3> — the %d stride-1 3x3 launches of a forward, %d MC sample "
                          "lane(s) per launch, plus their share (by weight count) of the weight-sampling launch" % (
                              args.prec, args.type, head["dominant_n"], head["launch_lanes"]),
                "achieved_contraction_only": head["dominant_tflops_contraction_only"],
                "frac_contraction_only": head["dominant_tflops_contraction_only"] / peak,
                "mc_samples_per_launch": head["launch_lanes"], "sampling_us_per_launch": head["sampling_us_per_launch"],
                "avg_launch_us": head["dominant_avg_us"], "avg_sampling_share_us": head["dominant_sampling_us"],
                "launches_per_forward": len(head["per_launch"]),
                "algorithmic_gflop_per_step": head["gflop_per_step"], "kernel_us_per_step": head["kernel_us_per_step"],
                "achieved_all_launches": head["gflop_per_step"] / head["kernel_us_per_step"] * 1e3,
                "achieved_e2e": head["achieved_e2e_tflops"], "frac_e2e": head["achieved_e2e_tflops"] / peak,
                "measured": "every contraction launch of a forward (as the timed loop issues it: mc_samples_per_launch MC "
                            "samples per launch) re-issued 10x inside a hipGraph, HIP events on the launch stream around 2 "
                            "replays (GPU time, no host gaps); the sampling launch timed the same way; achieved = "
                            "algorithmic FLOP / (contraction time + sampling share); achieved_e2e = algorithmic FLOP of a "
                            "step / ms_per_step of the timed region",
                "per_launch": [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items() if k != "dominant"}
                               for r in head["per_launch"]]}
            roofline["kernel_name"] = "contract_taps_kernel<%s,%s,3,3>" % (args.prec, args.type)
            # one figure per launch family (fraction of its own bound, sampling share included): what holds the step back
            fam = {}
            for r in head["per_launch"]:
                lab = r["launch"].split()
                hw = int(round((int(lab[-1][1:]) / args.batch / max(1, r.get("lanes") or 1)) ** 0.5)) if lab[-1].startswith("M") else 0
                key = "%s_%s_%d" % (lab[1], lab[2], hw)
                fam.setdefault(key, []).append((r.get("frac_incl_sampling", r["frac"]), r["us"]))
            roofline["rows"] = {k: round(sum(f * u for f, u in v) / sum(u for _, u in v), 3) for k, v in fam.items()}
            doms = [r.get("frac_incl_sampling", r["frac"]) for r in head["per_launch"] if r["dominant"]]
            if doms:
                roofline["frac_min_dominant_row"] = min(doms)
            if head.get("sustained"):
                roofline["shader_clock_ghz"] = head["sustained"].get("shader_clock_ghz")
                roofline["package_w"] = head["sustained"].get("package_w")
                roofline["clock_power_note"] = "sampled (%s) during the ~2 s back-to-back replay of the timed graph (`sustained`)" % head["sustained"].get("source")
        out = {
            "metric": "MC-samples/sec (Bayesian-%s, 224^2, bs=%d)" % ("ResNet18" if args.arch == "resnet18" else "ResNet50",
                                                                      args.batch),
            "value": head["value"], "unit": "MC-samples/s", "n_gpus": world, "rccl_ranks": rccl_ranks,
            "collective": "rccl all_reduce in the timed region" if grouped else "none (1 process, no group)",
            "steps": head["per_rank"], "warmup": args.warmup, "ms_per_step": head["ms_per_step"],
            "ms_per_step_runs": head["ms_per_step_runs"], "timed_regions": head["timed_regions"],
            "timed_seconds": head["timed_seconds"], "ms_per_step_all_regions": head["ms_per_step_all_regions"],
            "value_is": "len(steps) / median region of the settled (second) half of `timed_regions` back-to-back regions of "
                        "exactly `steps` MC samples each (barrier + synchronize on both sides of every region)",
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": args.prec, "data": "synthetic",
            "config": {"workload": "dnn_to_bnn(%s) %s%s, 224x224, batch %d, %d MC samples per GPU (%d in total), %s init "
                                   "(seed 0), activations %s, eval-BN/ReLU/residual %s, %s" % (
                                       args.arch, args.type, " + MOPED" if args.moped else "", args.batch, head["per_rank"],
                                       head["n_global"], "MOPED(delta 0.5)" if args.moped else "default", args.prec,
                                       "as torch ops" if args.no_fuse else "folded into the kernel epilogue",
                                       "eager launches" if head["lanes"] == 0 else
                                       ("hipGraph replay, %d MC samples per replay as lanes of one launch per layer" if
                                        head["lane_mode"] == "launch" else
                                        "hipGraph replay, %d MC samples in flight (one stream each)") % head["lanes"]),
                       "global_batch": args.batch * world, "parallelism": "mc-sample-shard x%d" % world},
            "image_samples_per_s": args.batch * head["n_global"] / head["elapsed"],
            "kl": head["kl"], "kl_rel_err": head.get("kl_rel_err"), "roofline": roofline,
        }
        if head.get("sustained"):
            out["sustained"] = head["sustained"]
        if "logits_rel_l2_vs_unfused_f32" in head:
            out["logits_rel_l2_vs_unfused_f32"] = head["logits_rel_l2_vs_unfused_f32"]
        if args.full and world == 1 and not args.no_extras:
            extra = {}
            try:
                r = run_resnet_config("resnet18", "Reparameterization", "bf16", 64, False, 16, 3, 16, dev, parity=True,
                                      prewarm=3, min_seconds=0.5)
                extra["cfg3"] = summarise_extra("cfg3: dnn_to_bnn(ResNet18) Reparameterization bs64 bf16", r, "bf16")
                r = run_resnet_config("resnet18", "Flipout", "f32", 64, False, 3, 1, 1, dev, prewarm=1, parity=True)
                extra["cfg4_f32_parity_mode"] = summarise_extra(
                    "cfg4 shard in f32 parity mode (v_mfma_f32_32x32x2_f32, f32 activations)", r, "f32")
                # north_star's 1e-4 tolerance at throughput: f32 activations, split-bf16 operands, three bf16 MFMAs per product
                r = run_resnet_config("resnet18", "Flipout", "bf16x3", 64, False, 20, 0, 20, dev, parity=True, prewarm=3,
                                      min_seconds=0.5)
                extra["cfg4_bf16x3"] = summarise_extra(
                    "cfg4 shard in split-bf16 mode (f32 activations, 3x v_mfma_f32_32x32x16_bf16 per product; fractions "
                    "against a third of the bf16 peak)", r, "bf16x3", table=True)
                extra["cfg2"] = run_mlp_config(dev)
                r = run_resnet_config("resnet50", "Flipout", "bf16", 128, True, 16, 2, 16, dev, parity=True, prewarm=3,
                                      min_seconds=0.5)
                extra["cfg5"] = summarise_extra("cfg5 shard: dnn_to_bnn(ResNet50) Flipout + MOPED(0.5) bs128 bf16", r, "bf16",
                                                table=True)
                r = run_resnet_config("resnet50", "Flipout", "bf16x3", 128, True, 16, 0, 16, dev, parity=True, prewarm=2,
                                      per_launch=False)
                extra["cfg5_bf16x3"] = summarise_extra("cfg5 shard in split-bf16 mode (f32 activations)", r, "bf16x3")
                # the strong-scaling shape of cfg4 (32 samples over 8 GPUs): 4 MC samples on this rank, one replay — the
                # fixed cost per rank (graph launch, packed-vector fold) is visible against the 24-sample region above
                r = run_resnet_config("resnet18", "Flipout", "bf16", 64, False, 4, 3, 4, dev, per_launch=False, prewarm=3,
                                      scaling="strong", total=4)
                extra["cfg4_strong_shape_4_per_rank"] = {
                    "workload": "cfg4 strong-scaling shape: 4 MC samples on this rank (32 over 8 GPUs), one hipGraph replay of 4 lanes",
                    "ms_per_step": r["ms_per_step"], "ms_per_region": r["ms_per_step"] * 4, "value": r["value"],
                    "unit": "MC-samples/s", "ms_per_step_runs": r.get("ms_per_step_runs"),
                    "vs_weak_region": r["value"] / head["value"]}
                # in a process of its own: the step captures autograd into a hipGraph, and nothing that could go wrong there
                # (a runtime that aborts instead of raising) may cost the run its JSON line
                extra["train_step"] = run_train_step_isolated()
            except Exception as e:  # noqa — the headline must survive a failing extra
                extra["error"] = "%s: %s" % (type(e).__name__, e)
            out["extra"] = extra
            if roofline is not None:  # both readings of north_star's ">= 40 % MFMA roofline ... parity to 1e-4" on the parsed line
                modes = {}
                for key, tag in (("cfg4_f32_parity_mode", "f32"), ("cfg4_bf16x3", "bf16x3")):
                    e = extra.get(key) or {}
                    if "dominant_kernel_frac" in e:
                        modes[tag] = {"dominant_kernel_frac": e["dominant_kernel_frac"], "dominant_kernel_tflops":
                                      e["dominant_kernel_tflops"], "peak": MFMA_PEAK_TFLOPS[tag], "value": e["value"],
                                      "frac_e2e": e.get("frac_e2e"), "logits_rel_l2": e.get("logits_rel_l2_vs_unfused_f32")}
                roofline["modes_within_1e-4"] = modes
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.type, args.batch)
            out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
        else:
            out["cpu_baseline"] = None
        emit(out)
    if grouped:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
