"""Monte-Carlo inference driver: independent MC samples sharded over the GPUs of a node, ONE collective.

What the reference does on one device (examples/main_bayesian_imagenet_dnn2bnn.py:480-499: loop `model(x)`
num_monte_carlo times, torch.stack, softmax, mean; utils/util.py:41-60 for entropy / mutual information) becomes:

  rank r of R runs the samples {s : s mod R == r}; sample s always uses Philox key (seed, sample_idx = s), so the
  result does not depend on R.  Each rank accumulates, on its GPU and in f32, the packed vector
        [ bs*C  sum_s p_s | bs*C  sum_s p_s^2 | bs  sum_s H(p_s) | sum_s KL | number of samples ]
  (btx_mc_accumulate, one launch per sample) and ONE `all_reduce(SUM)` over RCCL/xGMI merges the ranks
  (cfg4: 128 066 floats = 0.5 MB — latency-bound, so one call, not one per tensor).

CPU tensors (gloo tests, config 0) accumulate the same packed layout with ATen ops.
"""
import ctypes

import torch
import torch.distributed as dist

from . import _lib
from . import rng as _rng
from .models.dnn_to_bnn import get_kl_loss


def packed_numel(bs, num_classes):
    return 2 * bs * num_classes + bs + 2


MC_MAX_CLASSES = 24575  # btx_mc_accumulate[_lanes] keeps a row of probabilities in LDS (include/btx.h K6)


def _accumulate_torch(packed, logits, kl):
    """the same statistics with torch ops on the tensor's own device: CPU tensors, and GPU rows wider than MC_MAX_CLASSES"""
    bs, C = logits.shape
    p = torch.softmax(logits.float(), dim=1)
    packed[:bs * C] += p.reshape(-1)
    packed[bs * C:2 * bs * C] += (p * p).reshape(-1)
    packed[2 * bs * C:2 * bs * C + bs] += -(p * torch.log(p + 1e-15)).sum(dim=1)
    packed[2 * bs * C + bs] += float(kl)
    packed[2 * bs * C + bs + 1] += 1.0
    return packed


def accumulate(packed, logits, kl=0.0):
    """packed += statistics of one MC sample's logits [bs, C] (in place)."""
    bs, C = logits.shape
    if logits.is_cuda and C <= MC_MAX_CLASSES:
        lg = logits.contiguous()
        if lg.dtype == torch.float32:
            act = _lib.ACT_F32
        elif lg.dtype == torch.bfloat16:
            act = _lib.ACT_BF16
        else:
            lg, act = lg.float(), _lib.ACT_F32
        rc = _lib.lib().btx_mc_accumulate(lg.data_ptr(), bs, C, act, float(kl), packed.data_ptr(),
                                          torch.cuda.current_stream(lg.device).cuda_stream)
        _lib.check(rc)
        return packed
    return _accumulate_torch(packed, logits, kl)


def accumulate_lanes(packed, logits, lanes, kl=0.0):
    """packed += statistics of `lanes` MC samples whose logits sit back to back along the batch axis ([lanes*bs, C]) —
    on the GPU one launch (btx_mc_accumulate_lanes: a workgroup owns a batch row and folds its lanes in order, so the
    result equals `lanes` accumulate() calls bit for bit)."""
    lanes = int(lanes)
    bs = logits.shape[0] // lanes
    if (lanes == 1 or not logits.is_cuda or logits.dtype not in (torch.float32, torch.bfloat16)
            or logits.shape[1] > MC_MAX_CLASSES):
        for k in range(lanes):
            accumulate(packed, logits[k * bs:(k + 1) * bs], kl)
        return packed
    lg = logits.contiguous()
    act = _lib.ACT_F32 if lg.dtype == torch.float32 else _lib.ACT_BF16
    _lib.check(_lib.lib().btx_mc_accumulate_lanes(lg.data_ptr(), lanes, bs, lg.shape[1], act, float(kl), packed.data_ptr(),
                                                  torch.cuda.current_stream(lg.device).cuda_stream))
    return packed


def unpack(packed, bs, num_classes):
    """-> dict(mean_prob [bs,C], var_prob [bs,C], predictive_entropy [bs], mutual_information [bs], kl, samples)."""
    C = num_classes
    n = packed[2 * bs * C + bs + 1]
    mean = (packed[:bs * C] / n).reshape(bs, C)
    ex2 = (packed[bs * C:2 * bs * C] / n).reshape(bs, C)
    mean_h = packed[2 * bs * C:2 * bs * C + bs] / n
    pred_h = -(mean * torch.log(mean + 1e-15)).sum(dim=1)
    return {"mean_prob": mean, "var_prob": (ex2 - mean * mean).clamp_min(0), "predictive_entropy": pred_h,
            "mutual_information": pred_h - mean_h, "kl": packed[2 * bs * C + bs] / n, "samples": n}


class _SoftmaxStats:
    """the classification statistics above behind the interface the drivers use (`stats=None`): the same functions, f32"""
    dtype = torch.float32

    @staticmethod
    def numel(bs, width):
        return packed_numel(bs, width)

    @staticmethod
    def accumulate(packed, out, kl=0.0):
        return accumulate(packed, out, kl)

    @staticmethod
    def accumulate_lanes(packed, out, lanes, kl=0.0):
        return accumulate_lanes(packed, out, lanes, kl)


_SOFTMAX = _SoftmaxStats()


class GaussianStats:
    """MC moment statistics of a model that predicts real values (BTX-REG v1) — pass as `stats=` to mc_forward,
    mc_forward_batched, GraphedMC and evaluate.

    variance="log": the output is [rows, 2 D], columns [0, D) the mean m and [D, 2 D) the log-variance s (Kendall & Gal);
    variance=None: [rows, D], the mean alone.  The packed vector is FLOAT64, 3 N + 2 words with N = bs * D:
        [ N sum_s m | N sum_s m^2 | N sum_s v | sum_s KL | number of samples ],  v = (double)expf(s), m^2 the exact f64 product
    (the third block stays zero with variance=None).  float64 because E[m^2] - E[m]^2 cancels in f32 for un-standardised targets.
    GPU tensors in f32 / bf16: btx_mc_moments_lanes, ONE element-wise launch for all lanes, equal to one call per sample bit for
    bit.  CPU tensors and other dtypes: the same arithmetic with torch ops in float64 (expf: exp in float64 rounded to f32)."""
    dtype = torch.float64

    def __init__(self, variance="log"):
        if variance not in ("log", None):
            raise ValueError("variance must be 'log' or None, got %r" % (variance,))
        self.variance = variance

    def dims(self, width):
        """D of an output of `width` columns"""
        width = int(width)
        if self.variance == "log":
            if width < 2 or width % 2:
                raise ValueError("variance='log' needs an even output width (mean | log-variance), got %d" % width)
            return width // 2
        if width < 1:
            raise ValueError("empty output")
        return width

    def numel(self, bs, width):
        return 3 * int(bs) * self.dims(width) + 2

    def accumulate(self, packed, out, kl=0.0):
        return self.accumulate_lanes(packed, out, 1, kl)

    def accumulate_lanes(self, packed, out, lanes, kl=0.0):
        """packed += the statistics of `lanes` MC samples whose outputs sit back to back along the batch axis ([lanes * bs, W])"""
        lanes = int(lanes)
        if out.dim() != 2 or lanes < 1 or out.shape[0] % lanes:
            raise ValueError("out must be [lanes * bs, W]")
        bs, W = out.shape[0] // lanes, out.shape[1]
        D = self.dims(W)
        N = bs * D
        if packed.dtype != torch.float64 or packed.numel() != 3 * N + 2 or packed.device != out.device:
            raise ValueError("packed must be a float64 vector of %d words on %s" % (3 * N + 2, out.device))
        has_var = self.variance == "log"
        if out.is_cuda and out.dtype in (torch.float32, torch.bfloat16) and packed.is_contiguous() and N <= 2 ** 31 - 3:
            o = out.contiguous()
            act = _lib.ACT_F32 if o.dtype == torch.float32 else _lib.ACT_BF16
            _lib.check(_lib.lib().btx_mc_moments_lanes(o.data_ptr(), lanes, bs, D, int(has_var), act, float(kl), packed.data_ptr(),
                                                       torch.cuda.current_stream(o.device).cuda_stream))
            return packed
        for k in range(lanes):
            o = out[k * bs:(k + 1) * bs]
            o = o if o.dtype == torch.float64 else o.float()  # what the kernel widens: the f32 value
            m = o[:, :D].double().reshape(-1)
            packed[:N] += m
            packed[N:2 * N] += m * m
            if has_var:
                packed[2 * N:3 * N] += torch.exp(o[:, D:].double()).float().double().reshape(-1)
            packed[3 * N] += float(kl)
            packed[3 * N + 1] += 1.0
        return packed

    @staticmethod
    def unpack(packed, bs):
        """-> dict(mean, epistemic_var (clamped at 0), aleatoric_var, total_var [bs, D], kl, samples), float64"""
        N = (packed.numel() - 2) // 3
        D = N // int(bs)
        n = packed[3 * N + 1]
        mean = (packed[:N] / n).reshape(bs, D)
        ep = ((packed[N:2 * N] / n).reshape(bs, D) - mean * mean).clamp_min(0)
        al = (packed[2 * N:3 * N] / n).reshape(bs, D)
        return {"mean": mean, "epistemic_var": ep, "aleatoric_var": al, "total_var": ep + al, "kl": packed[3 * N] / n, "samples": n}


@torch.no_grad()
def mc_forward(model, x, num_samples, sample_offset=0, with_kl=False, group=None, reduce=True, lanes=1, rank=None,
               world=None, stats=None):
    """Run `num_samples` MC forward passes of `model` on `x`, sharded over the ranks of `group` (or the default
    group when torch.distributed is initialised), and return the all-reduced packed statistics tensor.
    lanes > 1 (GPU): this rank evaluates its samples `lanes` at a time, one launch per layer for all of them
    (rng.set_sample_lanes) — the same numbers as one at a time.  rank / world: override the process group's (tests that
    play several ranks in one process, with reduce=False).  stats: None — the softmax statistics above (f32) — or a GaussianStats
    (regression: float64 moment sums; the all-reduce is the same single call)."""
    stats = _SOFTMAX if stats is None else stats
    r0, w0 = 0, 1
    if dist.is_available() and dist.is_initialized():
        r0, w0 = dist.get_rank(group), dist.get_world_size(group)
    rank = r0 if rank is None else int(rank)
    world = w0 if world is None else int(world)
    packed = None
    kl = float(get_kl_loss(model)) if with_kl else 0.0  # RNG-free: identical for every sample
    mine = list(range(rank, num_samples, world))
    lanes = max(1, int(lanes)) if x.is_cuda else 1
    bs = x.shape[0]
    from . import functional as BF
    for g0 in range(0, len(mine), lanes):
        grp = [sample_offset + s for s in mine[g0:g0 + lanes]]
        if len(grp) > 1:
            _rng.set_sample_lanes(model, grp, batch=bs, presample=True)
            logits = model(x)
        elif x.is_cuda:
            if lanes > 1:
                _rng.set_sample_lanes(model, None)
            # a ragged last group of ONE sample is planned like a lane (BTX_FLAG_CONCURRENT: the K split of the throughput
            # plan), so a sample's f32 summation order does not depend on how the samples were grouped over launches / ranks
            with BF.concurrent_plan(lanes > 1 or BF._CONCURRENT):
                _rng.set_sample_index(model, grp[0], presample=True)
                logits = model(x)
        else:
            # CPU tensors take the ATen route, whose noise comes from torch's generator (the reference's draw order): key
            # that generator on (seed, sample index) for the duration of the forward, so that sample s is the same draw on
            # whichever rank evaluates it — the property the GPU path has by construction (BTX-RNG v1); the caller's CPU
            # generator state is restored by fork_rng and no CUDA generator is touched (torch.manual_seed would reseed them)
            _rng.set_sample_index(model, grp[0])
            with torch.random.fork_rng(devices=[]):
                torch.default_generator.manual_seed(_rng.cpu_sample_seed(grp[0]))  # the CPU generator ONLY
                logits = model(x)
        if isinstance(logits, tuple):
            logits = logits[0]
        if packed is None:
            packed = torch.zeros(stats.numel(bs, logits.shape[1]), dtype=stats.dtype, device=logits.device)
        stats.accumulate_lanes(packed, logits, len(grp), kl)
    if lanes > 1:
        _rng.set_sample_lanes(model, None)
    if packed is None:  # this rank got no sample: it still takes part in the collective
        with torch.no_grad():
            _rng.set_sample_index(model, sample_offset)
            shape = model(x).shape
        packed = torch.zeros(stats.numel(*shape), dtype=stats.dtype, device=x.device)
    if reduce and dist.is_available() and dist.is_initialized() and (w0 > 1 or world == w0):
        # also in a 1-rank group: the packed vector takes the same route (RCCL on a GPU) whatever the rank count
        dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    return packed


@torch.no_grad()
def mc_forward_batched(model, x, num_samples, chunk=4, sample_offset=0, with_kl=False, stats=None):
    """Opt-in batched-MC Flipout: the reference's own trick `data = torch.cat([data]*S, 0)` then ONE
    forward (examples/main_bayesian_flipout_imagenet.py:613-618).  `chunk` replicas of the batch go through the model
    together: they share one weight perturbation (one sampling pass, `chunk` x larger pixel tiles) and are decorrelated
    by their per-example Flipout signs only — pseudo-independent samples, NOT the statistics of `mc_forward`, which
    draws fresh weights per sample.  Returns the packed statistics of all `num_samples` replicas (this rank only).  stats: as in
    mc_forward."""
    stats = _SOFTMAX if stats is None else stats
    bs = x.shape[0]
    packed = None
    kl = float(get_kl_loss(model)) if with_kl else 0.0
    done, cid = 0, 0
    while done < num_samples:
        c = min(chunk, num_samples - done)
        xb = torch.cat([x] * c, 0) if c > 1 else x
        _rng.set_sample_index(model, sample_offset + cid, presample=xb.is_cuda)
        logits = model(xb)
        if isinstance(logits, tuple):
            logits = logits[0]
        if packed is None:
            packed = torch.zeros(stats.numel(bs, logits.shape[1]), dtype=stats.dtype, device=logits.device)
        for i in range(c):
            stats.accumulate(packed, logits[i * bs:(i + 1) * bs], kl)
        done += c
        cid += 1
    return packed


class GraphedMC:
    """One Monte-Carlo sample — weight sampling, the model forward, the accumulation of the predictive statistics —
    captured ONCE into a hipGraph (torch.cuda.CUDAGraph) and replayed per sample.

    A converted ResNet18 step is ~50 kernel launches of 20-70 us; issued one by one from Python the host cannot keep
    the GPU busy.  The graph removes the per-launch host work; what changes between samples — the sample index that
    keys BTX-RNG v1 — lives in one device word (BtxRng.sample_idx_dev) that `run()` rewrites before each replay, so
    every replay draws the noise of ITS sample index exactly as an eager forward with set_sample_index() would.

        g = GraphedMC(model, x, kl=float(get_kl_loss(model)))
        for s in my_samples: g.run(s)
        stats = unpack(g.packed, *g.logits_shape)

    The parameters must not be re-allocated while the graph is alive.  In-place parameter updates are seen by the replays
    of a one-sample graph and of lane_mode "streams"; lane_mode "launch" (the default for lanes > 1) caches the Flipout mean
    tiles and sigma between replays: call refresh_weights() after an update.  The input is read from `self.x` on every
    replay unless static_input=True (then call set_input() to change it)."""

    def __init__(self, model, x, kl=0.0, warmup=2, lanes=1, keep_logits=False, concurrent_hint=None, lane_mode="launch",
                 static_input=False, capture_stream=None, stats=None):
        """lanes > 1: one replay evaluates `lanes` MC samples (independent noise: the same results as one at a time); use
        run_many().  lane_mode "launch" (default): the samples are lanes of ONE launch per layer (rng.set_sample_lanes:
        4x the workgroups per launch fill the 256 CUs where one sample of a 7x7 / 14x14 layer cannot, and one
        workgroup's prologue / store overlaps another's MFMA loop); the mean tiles of the Flipout layers are written
        once (refresh_weights() after a parameter update), a replay samples sigma*eps only.  "streams": each sample on
        its own stream inside the graph, one launch per (layer, sample) — the round-2 form, kept for A/B.
        static_input (lane_mode "launch"): the input batch is the same for every replay, so a row-fused stem packs it into
        its kernel layout ONCE, outside the graph, instead of once per replay (set_input() re-packs).
        stats: None — the softmax statistics (f32 packed vector) — or a GaussianStats (regression: float64 moment sums)."""
        self.stats = _SOFTMAX if stats is None else stats
        if not x.is_cuda:
            raise ValueError("GraphedMC needs CUDA (ROCm) tensors")
        if lane_mode not in ("launch", "streams"):
            raise ValueError("lane_mode must be 'launch' or 'streams'")
        if int(lanes) > 1 and any(getattr(m, "_btx_q8", False) for m in model.modules()):
            raise _lib.BtxError("MC sample lanes > 1 are not supported on a model that holds a quantized (INT8) layer: use lanes=1")
        self.model, self.x, self.kl, self.lanes = model, x, float(kl), int(lanes)
        self.lane_mode = lane_mode
        self._capture_stream = capture_stream  # graphs that will be replayed concurrently must not share a capture stream:
        # the contraction workspace (split-K partials) is per stream and its address is baked into the captured launches
        self.static_input = bool(static_input) and self.lanes > 1 and lane_mode == "launch"
        self._static_packs = {}  # this graph's packed stem inputs {id(layer): (key, tensor)}: owned here, freed by close()
        if self.lanes > 1 and lane_mode == "launch":
            self._init_launch_lanes(warmup, keep_logits)
            return
        # keep_logits: lane_logits[k] is the (static) logits tensor of lane k — after a replay it holds the logits of the
        # sample that lane just evaluated (parity tests of the graphed configuration)
        self.keep_logits, self.lane_logits = bool(keep_logits), [None] * int(lanes)
        dev = x.device
        self.sample_devs = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(self.lanes)]
        self.sample_dev = self.sample_devs[0]
        self._layers = [m for m in model.modules() if hasattr(m, "_btx_layer_id")]
        self.packed = None
        self._lane_packed = [None] * self.lanes
        self._streams = [torch.cuda.Stream(dev) for _ in range(self.lanes)] if self.lanes > 1 else []
        from . import functional as BF
        # several samples in flight: plan every launch for device throughput (no split-K through HBM to fill idle CUs)
        with BF.concurrent_plan((self.lanes > 1) if concurrent_hint is None else bool(concurrent_hint)):
            self._capture_streams(dev, warmup)
        for pk in self._lane_packed:
            pk.zero_()
        for m in self._layers:
            m._btx_sample_dev = self.sample_dev

    def _capture_streams(self, dev, warmup):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup) + 1):  # 1st pass records the input shapes presample() needs
                for k in range(self.lanes):
                    self._lane(k)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: other threads (e.g. the RCCL watchdog of torch.distributed) keep making runtime calls while this
        # thread captures
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            if self.lanes == 1:
                self._lane(0)
            else:
                main = torch.cuda.current_stream(dev)
                for k, st in enumerate(self._streams):
                    st.wait_stream(main)
                    with torch.cuda.stream(st):
                        self._lane(k)
                for st in self._streams:
                    main.wait_stream(st)
                for k in range(1, self.lanes):  # fold the lanes' statistics into lane 0's buffer
                    self._lane_packed[0].add_(self._lane_packed[k])
                    self._lane_packed[k].zero_()

    # ---- lane_mode "launch": the MC samples of a replay are lanes of every layer's launch -----------------------------
    def _init_launch_lanes(self, warmup, keep_logits):
        model, x, dev = self.model, self.x, self.x.device
        self.keep_logits, self.lane_logits = bool(keep_logits), [None] * self.lanes
        self._layers = [m for m in model.modules() if hasattr(m, "_btx_layer_id")]
        self.sample_dev = torch.zeros(self.lanes, dtype=torch.int32, device=dev)
        self.sample_devs = [self.sample_dev]
        self._tiles = {}  # tile buffers of this graph (rng._presample cache): the mean tiles live here between replays
        self.packed, self._streams = None, []
        self.bs = x.shape[0]
        self._set_lane_state(True)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for i in range(max(1, warmup) + 1):  # 1st pass records the input shapes presample() needs
                self._launch_lanes(skip_mu=False)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        kw = dict(stream=self._capture_stream) if self._capture_stream is not None else {}
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local", **kw):
            self._launch_lanes(skip_mu=True)
        self.packed.zero_()
        # the replays need nothing from the Python-side lane state: a plain `model(x)` between replays is a plain forward
        self._set_lane_state(False)

    def _set_lane_state(self, on):
        """(re)apply / clear this graph's lane state on the layers WITHOUT touching the sample words: what makes
        rng.presample() address this graph's tile buffers (its cache key holds the lane count and the layers' ids)"""
        for m in self._layers:
            d = m.__dict__
            if on:
                d["_btx_lanes"], d["_btx_lane_batch"], d["_btx_sample_dev"] = self.lanes, self.bs, self.sample_dev
                d["_btx_static_x"] = self._static_packs if self.static_input else None
            else:
                d.pop("_btx_lanes", None)
                d.pop("_btx_lane_batch", None)
                d.pop("_btx_static_x", None)
                d["_btx_sample_dev"] = None
            d["_btx_pre"] = None

    def _launch_lanes(self, skip_mu):
        _rng.presample(self.model, 0, cache=self._tiles, skip_mu=skip_mu)
        logits = self.model(self.x)
        if isinstance(logits, tuple):
            logits = logits[0]
        bs = self.bs
        if self.packed is None:
            self.logits_shape = (bs, logits.shape[1])
            self.packed = torch.zeros(self.stats.numel(bs, logits.shape[1]), dtype=self.stats.dtype, device=logits.device)
        self.stats.accumulate_lanes(self.packed, logits, self.lanes, self.kl)  # one launch for all lanes of the replay
        if self.keep_logits:
            for k in range(self.lanes):
                self.lane_logits[k] = logits[k * bs:(k + 1) * bs]

    def refresh_weights(self):
        """lane_mode "launch": rewrite the cached mean tiles and sigma after an in-place parameter update (the replays
        sample sigma*eps only).  The sample words keep their values.  Works whatever happened to the model since the
        capture (plain forwards, a training step, another GraphedMC): the lane state of THIS graph is re-applied for the
        call, so the sampling pass writes the buffers the captured launches read."""
        if self.lanes > 1 and self.lane_mode == "launch":
            if not self._tiles:
                raise _lib.BtxError("GraphedMC.refresh_weights() after close()")
            with torch.no_grad():
                self._set_lane_state(True)
                try:
                    n_before = len(self._tiles)
                    _rng.presample(self.model, 0, cache=self._tiles, skip_mu=False)
                    if len(self._tiles) != n_before:  # a cache miss would fill NEW buffers the replays never read
                        raise _lib.BtxError("GraphedMC.refresh_weights(): the model's layers no longer match the captured graph")
                finally:
                    self._set_lane_state(False)

    def set_input(self, x):
        """copy a new batch (same shape / dtype) into the captured input; with static_input the row-fused stem's packed
        copy — what the captured launches read — is refilled from it"""
        self.x.copy_(x)
        if self.static_input:
            with torch.no_grad():
                for m in self._layers:
                    if hasattr(m, "_static_repack"):
                        m._static_repack(self.x, self._static_packs)

    def _lane(self, k):
        for m in self._layers:
            m.__dict__["_btx_sample_dev"] = self.sample_devs[k]
        _rng.presample(self.model, 0)
        logits = self.model(self.x)
        if isinstance(logits, tuple):
            logits = logits[0]
        if self._lane_packed[k] is None:
            self.logits_shape = tuple(logits.shape)
            self._lane_packed[k] = torch.zeros(self.stats.numel(*logits.shape), dtype=self.stats.dtype, device=logits.device)
            if k == 0:
                self.packed = self._lane_packed[0]
        self.stats.accumulate(self._lane_packed[k], logits, self.kl)
        if self.keep_logits:
            self.lane_logits[k] = logits

    def run(self, sample_idx):
        if self.lanes != 1:
            raise ValueError("this graph evaluates %d samples per replay: use run_many()" % self.lanes)
        self.sample_dev.fill_(int(sample_idx) & 0x7FFFFFFF)
        self.graph.replay()

    def run_many(self, sample_indices):
        """one replay = len(sample_indices) == lanes MC samples"""
        if len(sample_indices) != self.lanes:
            raise ValueError("expected %d sample indices" % self.lanes)
        if self.lane_mode == "launch" and self.lanes > 1:
            self.sample_dev.copy_(torch.tensor([int(i) & 0x7FFFFFFF for i in sample_indices], dtype=torch.int32))
        else:
            for w, i in zip(self.sample_devs, sample_indices):
                w.fill_(int(i) & 0x7FFFFFFF)
        self.graph.replay()

    def close(self):
        for m in self._layers:
            m._btx_sample_dev = None
            m._btx_pre = None
            m.__dict__.pop("_btx_lanes", None)
            m.__dict__.pop("_btx_lane_batch", None)
            if m.__dict__.get("_btx_static_x") is self._static_packs:
                m.__dict__.pop("_btx_static_x", None)
        self._static_packs.clear()  # only this graph's buffers: sibling graphs keep theirs
        self._tiles = {}


# ---- evaluation head: BTX-EVAL v1 ---------------------------------------------------------------------------
# What the reference's validate() / evaluate() (examples/main_bayesian_imagenet.py:549-642) and utils/avuc_loss.py:392-443 compute
# on the host, kept on the device: update() folds a batch into a float64 state, compute() reads it once.
EVAL_HEADER, EVAL_CURSOR, EVAL_DROPPED = _lib.MC_EVAL_HEADER, _lib.MC_EVAL_CURSOR, _lib.MC_EVAL_DROPPED
EVAL_RECORD = ("pred", "rank", "conf", "p_y", "nll", "brier", "entropy", "mutual_information")
_EVAL_ROW_THREADS = 256


def _logf32(x):
    """the model's logf: log in float64 rounded once to f32 (the correctly rounded value, whatever the host's f32 log is)"""
    return torch.log(x.double()).float()


def _row_sum32(terms):
    """f32 sum over the last axis in the kernel's shape: 256 strided partials, a butterfly per wave, (w0 + w1) + (w2 + w3)"""
    bs, C = terms.shape
    k = -(-C // _EVAL_ROW_THREADS)
    pad = terms.new_zeros(bs, k * _EVAL_ROW_THREADS)
    pad[:, :C] = terms
    w = pad.view(bs, k, _EVAL_ROW_THREADS)
    acc = terms.new_zeros(bs, _EVAL_ROW_THREADS)
    for j in range(k):
        acc = acc + w[:, j]
    acc = acc.view(bs, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:2 * off]
    acc = acc[..., 0]
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


def _fold_sum64(v):
    """float64 sum over the last axis (rows of the batch) in the fold's shape: 64 strided partials and a butterfly"""
    q, n = v.shape
    k = -(-n // 64)
    pad = v.new_zeros(q, k * 64)
    pad[:, :n] = v
    w = pad.view(q, k, 64)
    acc = v.new_zeros(q, 64)
    for j in range(k):
        acc = acc + w[:, j]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :off] + acc[:, off:2 * off]
    return acc[:, 0]


def _eval_rows_torch(packed, labels, bs, C):
    """the records [bs, 8] of BTX-EVAL v1 with torch ops in f32 on the tensor's own device"""
    packed = packed.float()
    eps = torch.tensor(1e-15, dtype=torch.float32, device=packed.device)
    zero = torch.zeros((), dtype=torch.float32, device=packed.device)
    sum_p = packed[:bs * C].view(bs, C)
    n = packed[2 * bs * C + bs + 1]
    y = labels.reshape(bs).long()
    valid = (y >= 0) & (y < C)
    yi = torch.where(valid, y, torch.full_like(y, -1))
    p = sum_p / n
    pred = p.argmax(1)  # the first of equal maxima
    conf = p.gather(1, pred[:, None])[:, 0]
    py = torch.where(valid, p.gather(1, yi.clamp_min(0)[:, None])[:, 0], zero)
    c = torch.arange(C, device=packed.device)[None, :]
    rank = ((p > py[:, None]) | ((p == py[:, None]) & (c < yi[:, None]))).sum(1)
    H = -_row_sum32(p * _logf32(p + eps))
    d = p - (c == yi[:, None]).float()
    brier = _row_sum32(d * d)
    MI = H - packed[2 * bs * C:2 * bs * C + bs] / n
    rec = packed.new_zeros(bs, 8)
    rec[:, 0] = pred.float()
    rec[:, 1] = torch.where(valid, rank, torch.full_like(rank, -1)).float()
    rec[:, 2] = conf
    rec[:, 3] = py
    rec[:, 4] = torch.where(valid, -_logf32(py + eps), zero)
    rec[:, 5] = torch.where(valid, brier, zero)
    rec[:, 6] = H
    rec[:, 7] = MI
    return rec


def _eval_fold_torch(state, rec, topk, nbins, th, use_mi, capacity):
    """state += the batch of records rec [bs, 8], in the fold kernel's order (in place)"""
    bs = rec.shape[0]
    T = 0 if th is None else th.numel()
    rank, conf32 = rec[:, 1], rec[:, 2]
    valid, hit = rank >= 0, rank == 0
    u32 = rec[:, 7] if use_mi else rec[:, 6]
    u = u32.double()
    z = u.new_zeros(bs)
    rows = [valid, ~valid, hit, valid & (rank < float(topk))]
    rows += [torch.where(valid, rec[:, j].double(), z) for j in (4, 5, 6, 7, 2)]
    rows += [torch.where(hit, u, z), torch.where(valid & ~hit, u, z)]
    b = (torch.ceil(conf32 * torch.tensor(float(nbins), dtype=torch.float32, device=rec.device)).long() - 1).clamp(0, nbins - 1)
    for k in range(nbins):
        m = valid & (b == k)
        rows += [m, torch.where(m, conf32.double(), z), m & hit]
    for t in range(T):
        cert = u32 <= th[t]
        rows += [valid & hit & cert, valid & hit & ~cert, valid & ~hit & cert, valid & ~hit & ~cert]
    s = _fold_sum64(torch.stack([r.double() for r in rows]))
    state[:11] += s[:11]
    state[EVAL_HEADER:EVAL_HEADER + 3 * nbins + 4 * T] += s[11:]
    cur = state[EVAL_CURSOR].clone()
    state[EVAL_DROPPED] += (cur + bs - capacity).clamp(0.0, float(bs))
    state[EVAL_CURSOR] = cur + bs
    return state


class _DeviceEvaluator:
    """What Evaluator and RegressionEvaluator share: a float64 state vector on one device with two cursor words (records seen,
    records dropped), a float32 record buffer [capacity, _WIDTH] of which the rows below the cursor are kept, a grow-only kernel
    workspace and a scratch packed vector.  A subclass sets _CURSOR / _DROPPED / _WIDTH and supplies _state_numel(),
    _alloc_settings(dev) (its device-side settings), _settings() (what merge compares), update, compute and records."""
    _CURSOR = _DROPPED = _WIDTH = None

    def _init_buffers(self, capacity, device):
        self.capacity = int(capacity)
        self.device = None
        self.state = self.records_buffer = self.workspace = self._scratch = None
        if device is not None:
            self._alloc(torch.device(device))

    def _alloc(self, dev):
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.state = torch.zeros(self._state_numel(), dtype=torch.float64, device=dev)
        self._alloc_settings(dev)
        if self.capacity:
            self.records_buffer = torch.zeros(self.capacity, self._WIDTH, dtype=torch.float32, device=dev)

    def _reserve(self, n):
        n = int(n)
        if n <= self.capacity:
            return
        new = max(n, 2 * self.capacity)
        if self.device is not None:
            buf = torch.zeros(new, self._WIDTH, dtype=torch.float32, device=self.device)
            if self.records_buffer is not None:
                buf[:self.capacity] = self.records_buffer
            self.records_buffer = buf
        self.capacity = new

    def _workspace_for(self, need, dtype):
        """the workspace, grown to `need` bytes: (pointer, bytes)"""
        ws = self.workspace
        if ws is None or ws.numel() * ws.element_size() < need:
            ws = self.workspace = torch.empty(need // (torch.finfo(dtype).bits // 8), dtype=dtype, device=self.device)
        return ws.data_ptr(), ws.numel() * ws.element_size()

    def _records_args(self):
        """(pointer or None, rows) of the record buffer, as the kernels take them"""
        rec = self.records_buffer
        return (None, 0) if rec is None else (rec.data_ptr(), rec.shape[0])

    def _zeroed_scratch(self, n, dtype, dev):
        if self._scratch is None or self._scratch.numel() != n or self._scratch.device != dev:
            self._scratch = torch.zeros(n, dtype=dtype, device=dev)
        return self._scratch.zero_()

    def reset(self):
        if self.state is not None:
            self.state.zero_()
        return self

    def _with_cursor_kept(self, op):
        """op(state), which sums into the state in place; the cursor words stay this evaluator's own"""
        keep = self.state[self._CURSOR:self._DROPPED + 1].clone()
        op(self.state)
        self.state[self._CURSOR:self._DROPPED + 1] = keep

    def _merge(self, other):
        if other._settings() != self._settings():
            raise ValueError("merge of evaluators with different settings")
        if other.state is None:
            return self
        if self.device is None:
            self._alloc(other.device)
        self._with_cursor_kept(lambda s: s.add_(other.state.to(self.device)))
        return self

    def _reduce(self, group):
        if dist.is_available() and dist.is_initialized():
            self._with_cursor_kept(lambda s: dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group))
        return self

    def _kept_records(self):
        """numpy [kept, _WIDTH]: the rows of the record buffer below the cursor"""
        import numpy as np
        if self.state is None or self.records_buffer is None:
            return np.zeros((0, self._WIDTH), np.float32)
        kept = min(int(self.state[self._CURSOR].item()), self.records_buffer.shape[0])
        return self.records_buffer[:kept].cpu().numpy()


class Evaluator(_DeviceEvaluator):
    """Classification metrics of MC predictions, accumulated on the device (BTX-EVAL v1).

        ev = Evaluator(1000, thresholds=[0.5, 1.0], capacity=50000)
        for x, y in loader:
            ev.update(mc_forward(model, x, 20), y)         # no host read; on the GPU two launches, capturable
        print(ev.compute())                                # the one host read

    update() takes the packed statistics of a batch (mc_forward / GraphedMC.packed) and int64 labels [bs].  A label outside
    [0, num_classes) — ignore_index by default, and every other out-of-range value alike — marks an ignored row, which adds
    nothing: pad a ragged last batch with them.  The state is a float64 vector (layout: include/btx.h K15); the per-example
    records [pred, rank, conf, p_y, nll, brier, H, MI] of the first `capacity` rows are kept in a device buffer, the rest is
    counted in `dropped`.  The thresholds live in a device tensor (`th`) that set_thresholds() rewrites in place, so a captured
    update sees the new values."""

    def __init__(self, num_classes, bins=15, topk=5, thresholds=None, uncertainty="entropy", capacity=0, ignore_index=-100,
                 device=None):
        if uncertainty not in ("entropy", "mi"):
            raise ValueError("uncertainty must be 'entropy' or 'mi'")
        if not 1 <= int(bins) <= _lib.MC_EVAL_MAX_BINS:
            raise ValueError("bins must be in 1..%d" % _lib.MC_EVAL_MAX_BINS)
        self.num_classes, self.bins, self.topk = int(num_classes), int(bins), int(topk)
        if self.num_classes < 1 or self.topk < 1:
            raise ValueError("num_classes and topk must be positive")
        if 0 <= int(ignore_index) < self.num_classes:
            raise ValueError("ignore_index must not be a class index")
        self.use_mi, self.uncertainty, self.ignore_index = uncertainty == "mi", uncertainty, int(ignore_index)
        th = [] if thresholds is None else [float(t) for t in torch.as_tensor(thresholds).reshape(-1).tolist()]
        if len(th) > _lib.MC_EVAL_MAX_THRESHOLDS:
            raise ValueError("at most %d thresholds" % _lib.MC_EVAL_MAX_THRESHOLDS)
        self.T, self._th_init, self.th = len(th), th, None
        self._init_buffers(capacity, device)

    _CURSOR, _DROPPED, _WIDTH = EVAL_CURSOR, EVAL_DROPPED, 8

    def _state_numel(self):
        return EVAL_HEADER + 3 * self.bins + 4 * self.T

    def _alloc_settings(self, dev):
        self.th = torch.tensor(self._th_init, dtype=torch.float32, device=dev)

    def _settings(self):
        return self.num_classes, self.bins, self.T, self.use_mi, self.topk

    def set_thresholds(self, thresholds):
        """rewrite the thresholds in place (same count): a captured update() reads the new values"""
        self.th.copy_(torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1))

    def reserve(self, rows):
        """grow the record buffer to hold at least `rows` records (a new allocation: not for use between replays of a captured
        update)"""
        self._reserve(rows)

    def update(self, packed, labels):
        """fold one batch: packed [2 * bs * C + bs + 2] f32 and labels [bs] int64, on one device.  GPU: btx_mc_eval, two launches
        on the current stream, capturable in torch.cuda.graph.  Rows the kernel does not take (C > _lib.MC_EVAL_MAX_CLASSES, a
        packed vector that is not f32) and CPU tensors run the same arithmetic with torch ops."""
        if self.device is None:
            self._alloc(packed.device)
        bs, C = labels.numel(), self.num_classes
        if packed.device != self.device:
            raise ValueError("packed is on %s, the evaluator's state on %s" % (packed.device, self.device))
        if packed.numel() != packed_numel(bs, C):
            raise ValueError("packed has %d elements, expected %d for bs %d, C %d" % (packed.numel(), packed_numel(bs, C), bs, C))
        if packed.is_cuda and C <= _lib.MC_EVAL_MAX_CLASSES and packed.dtype == torch.float32:
            pk = packed.contiguous()
            lb = labels.reshape(bs).to(device=packed.device, dtype=torch.int64).contiguous()  # the kernel reads device memory
            L = _lib.lib()
            _lib.check(L.btx_mc_eval(pk.data_ptr(), lb.data_ptr(), bs, C, self.topk, self.bins, self.th.data_ptr() if self.T else None,
                                     self.T, int(self.use_mi), self.state.data_ptr(), self.state.numel(), *self._records_args(),
                                     *self._workspace_for(L.btx_mc_eval_workspace_bytes(bs), torch.float32),
                                     torch.cuda.current_stream(self.device).cuda_stream))
            return self
        rec = _eval_rows_torch(packed, labels.to(packed.device), bs, C)
        cap = 0 if self.records_buffer is None else self.records_buffer.shape[0]
        if cap:
            at = self.state[EVAL_CURSOR].long() + torch.arange(bs, device=rec.device)
            keep = at < cap
            self.records_buffer[at[keep]] = rec[keep]
        _eval_fold_torch(self.state, rec, self.topk, self.bins, self.th, self.use_mi, cap)
        return self

    def update_logits(self, logits, labels):
        """one deterministic (or single-sample) forward, the reference's validate() form: the logits are accumulated into a
        zeroed scratch packed vector (accumulate: softmax and entropy of ONE sample), then update()"""
        bs, C = logits.shape
        scratch = self._zeroed_scratch(packed_numel(bs, C), torch.float32, logits.device)
        accumulate(scratch, logits)
        return self.update(scratch, labels)

    def merge(self, other):
        """add another evaluator's state (same classes / bins / thresholds).  The record cursor, the dropped count and the
        records themselves stay this evaluator's own."""
        return self._merge(other)

    def reduce(self, group=None):
        """ONE float64 all_reduce(SUM) of the state over `group`, for a validation set sharded over ranks: afterwards every
        rank's compute() is that of the whole set.  The records stay local — each rank keeps the examples it saw, with its own
        cursor and dropped count; nothing gathers them."""
        return self._reduce(group)

    def compute(self):
        """-> dict of the metrics; the one host read (the state vector)"""
        import numpy as np
        if self.state is None:
            raise ValueError("compute() before the first update()")
        s = self.state.cpu().numpy()
        n = s[0]
        d = n if n > 0 else 1.0
        bins = s[EVAL_HEADER:EVAL_HEADER + 3 * self.bins].reshape(self.bins, 3).copy()
        quad = s[EVAL_HEADER + 3 * self.bins:].reshape(self.T, 4).copy()
        gap = np.abs(bins[:, 2] - bins[:, 1])
        filled = bins[:, 0] > 0
        qs = quad.sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            hits = s[2]
            out = {"n": int(n), "ignored": int(s[1]), "top1": s[2] / d, "topk": s[3] / d, "nll": s[4] / d, "brier": s[5] / d,
                   "ece": float(gap.sum() / d), "mce": float((gap[filled] / bins[filled, 0]).max()) if filled.any() else 0.0,
                   "mean_entropy": s[6] / d, "mean_mi": s[7] / d, "mean_conf": s[8] / d,
                   "mean_u_correct": s[9] / hits if hits > 0 else float("nan"),
                   "mean_u_incorrect": s[10] / (n - hits) if n - hits > 0 else float("nan"),
                   "avu": np.where(qs > 0, (quad[:, 0] + quad[:, 3]) / np.where(qs > 0, qs, 1.0), np.nan),
                   "quadrants": quad.astype(np.int64), "bins": bins, "dropped": int(s[EVAL_DROPPED])}
        return {k: (float(v) if isinstance(v, np.floating) else v) for k, v in out.items()}

    def records(self):
        """-> dict of numpy arrays [N] over the kept rows, ignored rows left out: pred, rank (int64), correct (bool), conf, p_y,
        nll, brier, entropy, mutual_information (float32), and target (int64): pred where the row is correct, -1 elsewhere — the
        label itself is not kept, and utils.avuc_loss.eval_avu(r["pred"], r["target"], r["entropy"]) / accuracy_vs_uncertainty only
        compare it with pred."""
        import numpy as np
        rec = self._kept_records()
        rec = rec[rec[:, 1] >= 0]
        out = {name: rec[:, j].copy() for j, name in enumerate(EVAL_RECORD)}
        out["pred"], out["rank"] = out["pred"].astype(np.int64), out["rank"].astype(np.int64)
        out["correct"] = out["rank"] == 0
        out["target"] = np.where(out["correct"], out["pred"], -1)
        return out


# ---- regression: BTX-REG v1 --------------------------------------------------------------------------------
REG_HEADER, REG_CURSOR, REG_DROPPED = _lib.REG_EVAL_HEADER, _lib.REG_EVAL_CURSOR, _lib.REG_EVAL_DROPPED
REG_RECORD = ("mean", "epistemic_var", "aleatoric_var", "err")
_REG_SUMS = 9
_TWO_PI = 6.283185307179586


def _chunk_fold_sum64(v):
    """float64 sums over the last axis of v [Q, N] in the kernels' shape: per chunk of 4096 elements 256 strided partials added in
    order from zero, a butterfly per wave, (w0 + w1) + (w2 + w3); then the fold over the chunks (_fold_sum64)"""
    q, n = v.shape
    nch = -(-n // _lib.REG_CHUNK)
    pad = v.new_zeros(q, nch * _lib.REG_CHUNK)
    pad[:, :n] = v
    w = pad.view(q, nch, _lib.REG_CHUNK // 256, 256)
    acc = v.new_zeros(q, nch, 256)
    for j in range(w.shape[2]):
        acc = acc + w[:, :, j]
    acc = acc.view(q, nch, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:2 * off]
    acc = acc[..., 0]
    part = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    return _fold_sum64(part)


def normal_quantiles_squared(levels):
    """z_k^2 with z_k = sqrt(2) erfinv(level_k): the half-width, in standard deviations, of the central interval of a normal that
    holds `level_k` of its mass.  float64, on the host."""
    lv = torch.as_tensor(levels, dtype=torch.float64).reshape(-1)
    z = 2.0 ** 0.5 * torch.erfinv(lv)
    return z * z


class RegressionEvaluator(_DeviceEvaluator):
    """Regression metrics of MC predictions, accumulated on the device (BTX-REG v1).

        st = GaussianStats("log")
        ev = RegressionEvaluator(dims=1, capacity=10000)
        for x, y in loader:
            ev.update(mc_forward(model, x, 20, stats=st), y)   # no host read; on the GPU two launches, capturable
        print(ev.compute())                                    # the one host read

    update() takes the packed moments of a batch (GaussianStats layout, float64) and float32 targets [bs, dims].  A NaN target
    marks an ignored element, which adds nothing: pad a ragged last batch with them.  noise_var: a fixed observation-noise variance
    added to the aleatoric part (the variance=None form); min_var: floor of the predictive variance.  levels: the central-interval
    coverage levels (at most 8).  The state is a float64 vector (layout: include/btx.h K16); the records (mean, epistemic,
    aleatoric, err) of the first `capacity` ELEMENTS are kept in a device buffer, the rest is counted in `dropped`."""

    def __init__(self, dims, levels=(0.5, 0.8, 0.9, 0.95), noise_var=None, min_var=1e-12, capacity=0, device=None):
        self.dims = int(dims)
        if self.dims < 1:
            raise ValueError("dims must be positive")
        self.levels = [float(v) for v in torch.as_tensor(levels, dtype=torch.float64).reshape(-1).tolist()]
        if len(self.levels) > _lib.REG_EVAL_MAX_LEVELS or any(not 0.0 < v < 1.0 for v in self.levels):
            raise ValueError("at most %d levels, each inside (0, 1)" % _lib.REG_EVAL_MAX_LEVELS)
        if noise_var is not None and not float(noise_var) >= 0.0:
            raise ValueError("noise_var must not be negative")
        if not float(min_var) > 0.0:
            raise ValueError("min_var must be positive")
        self.K, self.noise_var, self.min_var, self.z2 = len(self.levels), noise_var, float(min_var), None
        self._init_buffers(capacity, device)

    _CURSOR, _DROPPED, _WIDTH = REG_CURSOR, REG_DROPPED, 4

    def _state_numel(self):
        return REG_HEADER + self.K

    def _alloc_settings(self, dev):
        self.z2 = normal_quantiles_squared(self.levels).to(dev)

    def _settings(self):
        return self.dims, self.levels

    def reserve(self, elements):
        """grow the record buffer to hold at least `elements` records (a new allocation: not for use between replays of a captured
        update)"""
        self._reserve(elements)

    def update(self, packed, target):
        """fold one batch: packed [3 * bs * dims + 2] float64 and target [bs, dims] float32, on one device.  GPU:
        btx_reg_eval_update, two launches on the current stream, capturable in torch.cuda.graph.  CPU tensors run the same
        arithmetic with torch ops in float64."""
        if self.device is None:
            self._alloc(packed.device)
        D = self.dims
        N = target.numel()
        if N % D or N < 1:
            raise ValueError("target must be [bs, %d]" % D)
        bs = N // D
        if packed.device != self.device:
            raise ValueError("packed is on %s, the evaluator's state on %s" % (packed.device, self.device))
        if packed.numel() != 3 * N + 2 or packed.dtype != torch.float64:
            raise ValueError("packed must hold %d float64 words for bs %d, dims %d (GaussianStats)" % (3 * N + 2, bs, D))
        y = target.to(device=packed.device, dtype=torch.float32).reshape(N).contiguous()
        nv = 0.0 if self.noise_var is None else float(self.noise_var)
        if packed.is_cuda:
            pk = packed.contiguous()
            L = _lib.lib()
            _lib.check(L.btx_reg_eval_update(pk.data_ptr(), y.data_ptr(), bs, D, nv, self.min_var, self.z2.data_ptr() if self.K else None,
                                             self.K, self.state.data_ptr(), self.state.numel(), *self._records_args(),
                                             *self._workspace_for(L.btx_reg_eval_workspace_bytes(bs, D), torch.float64),
                                             torch.cuda.current_stream(self.device).cuda_stream))
            return self
        n = packed[3 * N + 1]
        yd = y.double()
        ok = ~torch.isnan(yd)
        mean = packed[:N] / n
        ep = (packed[N:2 * N] / n - mean * mean).clamp_min(0.0)
        al = packed[2 * N:3 * N] / n + nv
        var = (ep + al).clamp_min(self.min_var)
        err = yd - mean
        e2 = err * err
        nll = 0.5 * (torch.log((_TWO_PI * var).float().double()).float().double() + e2 / var)
        z = torch.zeros_like(yd)
        rows = [ok.double(), (~ok).double()]
        rows += [torch.where(ok, t, z) for t in (e2, err.abs(), nll, ep, al, yd, yd * yd)]
        rows += [(ok & (e2 <= self.z2[k] * var)).double() for k in range(self.K)]
        s = _chunk_fold_sum64(torch.stack(rows))
        cap = 0 if self.records_buffer is None else self.records_buffer.shape[0]
        cur = self.state[REG_CURSOR].clone()
        if cap:
            at = cur.long() + torch.arange(N)
            keep = at < cap
            self.records_buffer[at[keep]] = torch.stack([mean, ep, al, err], 1).float()[keep]
        self.state[:_REG_SUMS] += s[:_REG_SUMS]
        self.state[REG_HEADER:REG_HEADER + self.K] += s[_REG_SUMS:]
        self.state[REG_DROPPED] += (cur + N - cap).clamp(0.0, float(N))
        self.state[REG_CURSOR] = cur + N
        return self

    def update_outputs(self, out, target):
        """one deterministic (or single-sample) forward: the outputs [bs, 2 * dims] (mean | log-variance) or [bs, dims] (mean) are
        accumulated into a zeroed scratch packed vector as ONE sample, then update()"""
        bs, W = out.shape
        if W not in (self.dims, 2 * self.dims):
            raise ValueError("out must be [bs, %d] or [bs, %d]" % (self.dims, 2 * self.dims))
        st = GaussianStats("log" if W == 2 * self.dims else None)
        scratch = self._zeroed_scratch(st.numel(bs, W), torch.float64, out.device)
        st.accumulate(scratch, out)
        return self.update(scratch, target)

    def merge(self, other):
        """add another evaluator's state (same dims / levels).  The record cursor, the dropped count and the records themselves stay
        this evaluator's own."""
        return self._merge(other)

    def reduce(self, group=None):
        """ONE float64 all_reduce(SUM) of the state over `group`; the cursor words and the records stay local"""
        return self._reduce(group)

    def compute(self):
        """-> dict of the metrics; the one host read (the state vector)"""
        import numpy as np
        if self.state is None:
            raise ValueError("compute() before the first update()")
        s = self.state.cpu().numpy()
        n = s[0]
        d = n if n > 0 else 1.0
        mse = s[2] / d
        sst = s[8] - s[7] * s[7] / d
        cov = s[REG_HEADER:REG_HEADER + self.K] / d
        lv = np.asarray(self.levels, dtype=np.float64)
        out = {"n": int(n), "ignored": int(s[1]), "mse": mse, "rmse": float(np.sqrt(mse)), "mae": s[3] / d, "nll": s[4] / d,
               "r2": float(1.0 - s[2] / sst) if sst > 0 else float("nan"),
               "mean_epistemic_var": s[5] / d, "mean_aleatoric_var": s[6] / d, "mean_total_var": (s[5] + s[6]) / d,
               "coverage": cov, "levels": lv, "calibration_error": float(((cov - lv) ** 2).mean()) if self.K else 0.0,
               "dropped": int(s[REG_DROPPED])}
        return {k: (float(v) if isinstance(v, np.floating) else v) for k, v in out.items()}

    def records(self):
        """-> dict of numpy float32 arrays [M] over the kept elements, ignored ones left out: mean, epistemic_var, aleatoric_var,
        err, and error = |err|, unc = epistemic_var + aleatoric_var — the vectors uncertainty_calibration_loss.EaULoss takes"""
        import numpy as np
        rec = self._kept_records()
        rec = rec[~np.isnan(rec[:, 3])]
        out = {name: rec[:, j].copy() for j, name in enumerate(REG_RECORD)}
        out["error"], out["unc"] = np.abs(out["err"]), out["epistemic_var"] + out["aleatoric_var"]
        return out


@torch.no_grad()
def evaluate(model, batches, num_samples, lanes=1, graphed=None, sample_offset=0, evaluator=None, group=None, stats=None):
    """The reference's evaluate() loop (examples/main_bayesian_imagenet.py:598-642): `num_samples` MC forwards of every batch of
    `batches` (an iterable of (x, y)), mean probabilities, argmax, accuracy — and everything else Evaluator accumulates — with no
    host read inside the loop.  Returns the evaluator; call compute() / records() on it.

    graphed (default: on for GPU batches): ONE GraphedMC is captured on the first batch; per batch its packed vector is zeroed,
    set_input() copies the batch in, the samples run `lanes` per replay (num_samples must be a multiple of lanes) and update()
    folds the result.  A ragged last batch is padded to the captured shape with zeros and ignore_index labels.  Otherwise:
    mc_forward + update per batch.  Every rank runs all samples of ITS batches (the validation set, not the samples, is what is
    sharded here); with `group` the states are summed at the end by Evaluator.reduce(group).
    evaluator=None: one is built on the first batch that keeps per-example records, its buffer grown between the batches.
    stats=GaussianStats(...) with evaluator=RegressionEvaluator(...) (or None: one is built): the same loop for a model that predicts
    real values; targets are float32 [bs, D] and a ragged last batch is padded with zero rows and NaN targets."""
    ev, grow, g, seen = evaluator, evaluator is None, None, 0
    reg = isinstance(stats, GaussianStats)
    if ev is not None and reg != isinstance(ev, RegressionEvaluator):
        raise ValueError("stats=GaussianStats goes with a RegressionEvaluator, stats=None with an Evaluator")
    lanes = max(1, int(lanes))
    try:
        for x, y in batches:
            use_graph = x.is_cuda if graphed is None else bool(graphed)
            if use_graph and not x.is_cuda:
                raise ValueError("graphed evaluation needs CUDA (ROCm) tensors")
            lane_n = lanes if x.is_cuda else 1
            if use_graph:
                if num_samples % lane_n:
                    raise ValueError("num_samples must be a multiple of lanes for graphed evaluation")
                if g is None:
                    g = GraphedMC(model, x.clone(), lanes=lane_n, static_input=True, stats=stats)
                bs = g.x.shape[0]
                if x.shape[0] > bs or x.shape[1:] != g.x.shape[1:]:
                    raise ValueError("a batch larger than the first (captured) batch")
                if x.shape[0] < bs:
                    xp = torch.zeros_like(g.x)
                    xp[:x.shape[0]] = x
                    if reg:
                        yp = torch.full((bs, y.numel() // x.shape[0]), float("nan"), dtype=torch.float32, device=y.device)
                        yp[:x.shape[0]] = y.reshape(x.shape[0], -1)
                    else:
                        yp = torch.full((bs,), ev.ignore_index if ev is not None else -100, dtype=torch.int64, device=y.device)
                        yp[:y.numel()] = y
                    x, y = xp, yp
                g.packed.zero_()
                g.set_input(x)
                for s0 in range(0, num_samples, lane_n):
                    idx = [sample_offset + s for s in range(s0, s0 + lane_n)]
                    if lane_n == 1:
                        g.run(idx[0])
                    else:
                        g.run_many(idx)
                packed = g.packed
            else:
                packed = mc_forward(model, x, num_samples, sample_offset=sample_offset, reduce=False, lanes=lane_n, rank=0, world=1,
                                    stats=stats)
            bs = x.shape[0]
            if ev is None and reg:
                ev = RegressionEvaluator((packed.numel() - 2) // (3 * bs), device=packed.device)
            elif ev is None:
                ev = Evaluator((packed.numel() - 2 - bs) // (2 * bs), device=packed.device)
            if grow:
                seen += bs * ev.dims if reg else bs
                ev.reserve(seen)
            ev.update(packed, y.to(packed.device))
    finally:
        if g is not None:
            g.close()
    if ev is not None and group is not None:
        ev.reduce(group)
    return ev
