"""SGD / Adam / AdamW whose update is ONE pass of hand-written HIP over every parameter of a group (csrc/btx_optim.hip, DESIGN.md §14
"BTX-OPT v1"), with torch's constructor arguments, state keys and state_dict, so that

    optimizer = torch.optim.Adam(model.parameters(), lr)        # the reference's examples
    optimizer = bayesian_torch_amd.optim.Adam(model.parameters(), lr)

are interchangeable.  Parameters, gradients and state are walked flat in STORAGE order (the GEMM-major conv parameters of this
package are permuted views of dense storage: torch's optimizers iterate them through strided paths).  The hyper-parameters live in
a small device block that the host rewrites before every launch, so the launches can be captured into a hipGraph
(autograd.GraphedTrainStep(..., optimizer=opt)) and still follow an LR scheduler and the advancing step count.

`max_grad_norm=` (ours) clips the global L2 norm over all groups inside the same launches: btx_optim_grad_norm leaves total_norm and
coef = min(1, max_norm / (total_norm + 1e-6)) in device words (`opt.total_norm`, `opt.clip_coef`) and the update multiplies every
gradient element by coef as its first operation.  Unlike torch.nn.utils.clip_grad_norm_, `p.grad` itself is NOT rescaled.

CPU parameters take a chain of torch ops in the same order (each operation its own rounded tensor op), so the classes work on CPU
models; a GPU parameter that cannot take the kernel (not f32, not dense) raises BtxError — there is no quiet fallback."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import BtxError

__all__ = ["SGD", "Adam", "AdamW"]


def _refuse(**kw):
    for name, val in kw.items():
        if isinstance(val, torch.Tensor) or val:
            raise ValueError("%s=%r is not supported by bayesian_torch_amd.optim (the update is one fused HIP pass)" % (name, val))


def _dense(t):
    """non-overlapping and dense: numel elements that fill [data_ptr, data_ptr + numel) in some order"""
    dims = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return True


class _Bucket:
    """the parameters of one group that share one device block (Adam: the same step count; SGD: first step or not)"""
    __slots__ = ("group", "key", "entries", "items", "n_items", "row", "t")

    def __init__(self, group, key):
        self.group, self.key, self.entries, self.items, self.n_items, self.row = group, key, [], None, 0, 0
        self.t = key[1] if key[0] == "adam" else 0  # Adam: the steps its parameters have taken


class _Plan:
    __slots__ = ("buckets", "cpu", "dev", "blocks", "host", "norm_items", "n_norm", "updated", "stages", "ws", "out")


class _BtxOptimizer(torch.optim.Optimizer):
    _torch_cls = None

    def __init__(self, params, defaults, max_grad_norm):
        if max_grad_norm is not None and not (float(max_grad_norm) > 0):
            raise ValueError("max_grad_norm must be > 0 or None")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._stage, self._prealloc, self._blocks, self._ws, self._norm_out = {}, {}, {}, {}, {}
        self._cpu_norm = None
        super().__init__(params, defaults)

    # ---- what the user reads back -------------------------------------------------------------------------------------
    def _norm_word(self, i):
        if self.max_grad_norm is None:
            return None
        if self._norm_out:
            return next(iter(self._norm_out.values()))[i]
        return None if self._cpu_norm is None else self._cpu_norm[i]

    @property
    def total_norm(self):
        """the global gradient norm of the last step (a 0-d f32 tensor where the parameters live; None without max_grad_norm)"""
        return self._norm_word(0)

    @property
    def clip_coef(self):
        return self._norm_word(1)

    # ---- planning: which launches a step consists of --------------------------------------------------------------------
    def _check_group(self, group):
        _refuse(amsgrad=group.get("amsgrad"), foreach=group.get("foreach"), fused=group.get("fused"),
                capturable=group.get("capturable"), differentiable=group.get("differentiable"))
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("lr: a tensor-valued lr is not supported (the host writes lr into the device block at every step)")

    def _plan(self, grads=None):
        """state allocation, gradient staging buffers and the item tables of one step (no launch, no state change).  grads: a mapping
        {parameter: gradient tensor} read in place of p.grad (autograd.GraphedTrainStep(group=): the slices of the reduced bucket);
        a parameter it does not hold is skipped"""
        plan = _Plan()
        plan.buckets, plan.cpu, plan.dev, plan.updated, plan.stages = [], [], None, [], []
        for group in self.param_groups:
            self._check_group(group)
            by_key = {}
            for p in group["params"]:
                g = p.grad if grads is None else grads.get(p)
                if g is None or p.numel() == 0:
                    continue
                if g.is_sparse:
                    raise BtxError("sparse gradients are not supported (parameter of shape %s)" % (tuple(p.shape),))
                if not p.is_cuda:
                    if p.dtype not in (torch.float32, torch.float64):
                        raise BtxError("CPU parameters must be float32 or float64 (got %s, shape %s)" % (p.dtype, tuple(p.shape)))
                    plan.cpu.append((group, p))
                    continue
                if p.dtype != torch.float32 or not _dense(p):
                    raise BtxError("the fused update needs float32, non-overlapping and dense GPU parameters: got %s, shape %s, "
                                   "strides %s" % (p.dtype, tuple(p.shape), tuple(p.stride())))
                if g.dtype != torch.float32 or g.device != p.device:
                    raise BtxError("the gradient of a float32 GPU parameter must be float32 on the same device (got %s on %s, "
                                   "shape %s)" % (g.dtype, g.device, tuple(p.shape)))
                if plan.dev is None:
                    plan.dev = p.device
                elif plan.dev != p.device:
                    raise BtxError("parameters on more than one GPU (%s, %s) are not supported" % (plan.dev, p.device))
                if g.stride() != p.stride() and not (p.numel() == 1):
                    st = self._stage.get(p)
                    if st is None:
                        st = self._stage[p] = torch.empty_like(p)
                    plan.stages.append((st, g))
                    g = st
                key, s0, s1 = self._state_of(group, p)
                b = by_key.get(key)
                if b is None:
                    b = by_key[key] = _Bucket(group, key)
                    plan.buckets.append(b)
                b.entries.append((p, g, s0, s1))
                plan.updated.append(p)
        if self.max_grad_norm is not None and plan.cpu and plan.buckets:
            raise BtxError("max_grad_norm needs all parameters on one device (CPU and GPU parameters are mixed)")
        for i, b in enumerate(plan.buckets):
            b.row, b.n_items = i, len(b.entries)
            b.items = (_lib.OptimItem * b.n_items)()
            for it, (p, g, s0, s1) in zip(b.items, b.entries):
                it.p, it.g, it.n = p.data_ptr(), g.data_ptr(), p.numel()
                it.state0 = s0.data_ptr() if s0 is not None else None
                it.state1 = s1.data_ptr() if s1 is not None else None
        if plan.buckets:
            dev, nb = plan.dev, len(plan.buckets)
            blk = self._blocks.get(dev)
            if blk is None or blk.shape[0] < nb:
                blk = self._blocks[dev] = torch.zeros(max(nb, 4), 16, dtype=torch.int32, device=dev)
            plan.blocks = blk
            plan.host = np.zeros((nb, 16), dtype=np.int32)
            if self.max_grad_norm is not None:
                L = _lib.lib()
                ents = [e for b in plan.buckets for e in b.entries]
                plan.n_norm = len(ents)
                plan.norm_items = (_lib.OptimItem * plan.n_norm)()
                for it, (p, g, _, _) in zip(plan.norm_items, ents):
                    it.g, it.n = g.data_ptr(), p.numel()
                need = L.btx_optim_grad_norm_workspace_bytes(plan.n_norm, sum(e[0].numel() for e in ents))
                ws = self._ws.get(dev)
                if ws is None or ws.numel() * 8 < need:
                    self._ws[dev] = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
                if dev not in self._norm_out:
                    self._norm_out[dev] = torch.zeros(2, dtype=torch.float32, device=dev)
                plan.ws, plan.out = self._ws[dev], self._norm_out[dev]  # (a captured plan keeps the buffers its graph points to)
        return plan

    def _restrided(self, p, t):
        """a state tensor in the storage order of p (torch.empty_like(p) semantics); a loaded one with other strides is re-laid"""
        if t.stride() == p.stride() or p.numel() == 1:
            return t
        new = torch.empty_like(p)
        new.copy_(t)
        return new

    # ---- one step ------------------------------------------------------------------------------------------------------
    def _advance(self, plan):
        """host side of a step: step counts, and the device blocks rewritten from the groups' CURRENT hyper-parameters"""
        for b in plan.buckets:
            self._check_group(b.group)
            h = _lib.OptimHyper()
            self._fill(b, h)
            plan.host[b.row] = np.frombuffer(h, dtype=np.int32)
        if plan.buckets:
            plan.blocks[:len(plan.buckets)].copy_(torch.from_numpy(plan.host))

    def _launch(self, plan):
        """the launches of a step on the current stream: gradient staging, norm, updates.  Capturable."""
        if not plan.buckets:
            return
        L = _lib.lib()
        dev = plan.dev
        stream = torch.cuda.current_stream(dev).cuda_stream
        for st, g in plan.stages:
            st.copy_(g)
        coef = None
        if self.max_grad_norm is not None:
            out, ws = plan.out, plan.ws
            _lib.check(L.btx_optim_grad_norm(plan.norm_items, plan.n_norm, self.max_grad_norm, out.data_ptr(), ws.data_ptr(),
                                             ws.numel() * 8, stream))
            coef = out.data_ptr() + 4
        for b in plan.buckets:
            self._launch_bucket(L, b, plan.blocks.data_ptr() + 64 * b.row, coef, stream)

    def _finish(self, plan):
        for b in plan.buckets:
            self._after(b)
        if plan.updated:  # the kernels wrote through raw pointers: caches keyed on (data_ptr, _version) must see the update
            torch.autograd.graph.increment_version(plan.updated)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._plan()
        self._advance(plan)
        self._launch(plan)
        self._finish(plan)
        if plan.cpu:
            self._cpu_step(plan.cpu)
        return loss

    # ---- inside autograd.GraphedTrainStep ------------------------------------------------------------------------------------
    def _warm(self, dev):
        """load and run every kernel of this class once, on scratch tensors (never on the model): a capture must not be the first
        launch of a kernel"""
        cls = type(self)
        for kw in self._warm_configs():
            ps = [torch.nn.Parameter(torch.zeros(n, device=dev)) for n in (5, 4100)]
            for p in ps:
                p.grad = torch.ones_like(p)
            o = cls(ps, max_grad_norm=1.0, **kw)
            o.step()
            o.step()
        torch.cuda.synchronize(dev)

    # ---- CPU parameters: the same operations as torch ops, one rounded op each ------------------------------------------------
    def _cpu_coef(self, cpu):
        if self.max_grad_norm is None:
            return None
        tot = math.sqrt(sum(float(p.grad.detach().double().pow(2).sum()) for _, p in cpu))
        f = np.float32
        total = f(tot)
        c = f(self.max_grad_norm) / (total + f(1e-6))
        c = c if c < f(1.0) else f(1.0)
        self._cpu_norm = torch.tensor([float(total), float(c)], dtype=torch.float32)
        return float(c)


def _dt(p):
    """rounds a host double to the parameter's dtype and returns it as a Python float (exact in that dtype)"""
    return (lambda x: float(np.float32(x))) if p.dtype == torch.float32 else float


class SGD(_BtxOptimizer):
    """torch.optim.SGD's arguments and state ('momentum_buffer'); see the module docstring"""
    _torch_cls = torch.optim.SGD

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None, max_grad_norm=None):
        _refuse(foreach=foreach, fused=fused, differentiable=differentiable)
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr: a tensor-valued lr is not supported")
        if isinstance(weight_decay, torch.Tensor):
            raise ValueError("weight_decay: a tensor-valued weight_decay is not supported")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("lr, momentum and weight_decay must be >= 0")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(torch.optim.SGD([torch.zeros(1)]).defaults)  # torch's keys, so that state_dict()s interchange
        defaults.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
        super().__init__(params, defaults, max_grad_norm)

    def _warm_configs(self):
        return [dict(lr=0.0, momentum=0.9), dict(lr=0.0)]

    def _state_of(self, group, p):
        if group["momentum"] == 0:
            return ("plain",), None, None
        st = self.state[p]
        buf = st.get("momentum_buffer")
        if buf is not None:
            buf = st["momentum_buffer"] = self._restrided(p, buf)
            return ("mom", False), buf, None
        buf = self._prealloc.get(p)
        if buf is None:
            buf = self._prealloc[p] = torch.empty_like(p)  # written, never read, by the first step
        return ("mom", True), buf, None

    def _fill(self, b, h):
        g = b.group
        h.neg_lr, h.wd, h.momentum = -float(g["lr"]), float(g["weight_decay"]), float(g["momentum"])
        h.one_m_damp = 1.0 - float(g["dampening"])
        # read from the state NOW, not from the plan: a captured plan outlives the first step
        first = b.key[0] == "mom" and self.state[b.entries[0][0]].get("momentum_buffer") is None
        h.flags = (_lib.OPT_MAXIMIZE if g["maximize"] else 0) | (_lib.OPT_NESTEROV if g["nesterov"] else 0) | \
            (_lib.OPT_COUPLED_WD if g["weight_decay"] != 0 else 0) | (_lib.OPT_FIRST_STEP if first else 0)

    def _launch_bucket(self, L, b, block, coef, stream):
        _lib.check(L.btx_optim_sgd(b.items, b.n_items, block, 1 if b.key[0] == "mom" else 0, coef, stream))

    def _after(self, b):
        if b.key[0] == "mom" and b.key[1]:
            for p, _, buf, _ in b.entries:
                if self.state[p].get("momentum_buffer") is None:
                    self.state[p]["momentum_buffer"] = buf
                    self._prealloc.pop(p, None)

    def _cpu_step(self, cpu):
        coef = self._cpu_coef(cpu)
        for group, p in cpu:
            dt = _dt(p)
            g = p.grad.detach()
            if group["maximize"]:
                g = g.neg()
            if coef is not None:
                g = g.mul(coef)
            if group["weight_decay"] != 0:
                g = g.add(p.mul(dt(group["weight_decay"])))
            mom = group["momentum"]
            if mom != 0:
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if buf is None:
                    buf = st["momentum_buffer"] = torch.empty_like(p).copy_(g)
                else:
                    buf.copy_(buf.mul(dt(mom)).add(g.mul(dt(1.0 - group["dampening"]))))
                g = g.add(buf.mul(dt(mom))) if group["nesterov"] else buf
            p.copy_(p.add(g.mul(dt(-group["lr"]))))


class Adam(_BtxOptimizer):
    """torch.optim.Adam's arguments and state ('step', 'exp_avg', 'exp_avg_sq'); amsgrad is refused"""
    _torch_cls = torch.optim.Adam
    _decoupled_default = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=None, max_grad_norm=None):
        _refuse(amsgrad=amsgrad, foreach=foreach, fused=fused, capturable=capturable, differentiable=differentiable)
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr: a tensor-valued lr is not supported")
        if any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("betas: tensor-valued betas are not supported")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("lr, eps and weight_decay must be >= 0 and the betas in [0, 1)")
        if decoupled_weight_decay is None:
            decoupled_weight_decay = self._decoupled_default
        defaults = dict(self._torch_cls([torch.zeros(1)]).defaults)  # torch's keys, so that state_dict()s interchange
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize)
        if "decoupled_weight_decay" in defaults or decoupled_weight_decay != self._decoupled_default:
            defaults["decoupled_weight_decay"] = bool(decoupled_weight_decay)
        super().__init__(params, defaults, max_grad_norm)

    def _warm_configs(self):
        return [dict(lr=0.0)]

    def _decoupled(self, group):
        return bool(group.get("decoupled_weight_decay", self._decoupled_default))

    def _state_of(self, group, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        if st["step"].device.type != "cpu":
            st["step"] = st["step"].cpu()
        m = st["exp_avg"] = self._restrided(p, st["exp_avg"])
        v = st["exp_avg_sq"] = self._restrided(p, st["exp_avg_sq"])
        return ("adam", int(st["step"])), m, v

    def _hyper(self, group, t, dt=float):
        b1, b2 = group["betas"]
        lr, wd = group["lr"], group["weight_decay"]
        return dict(one_m_b1=dt(1.0 - b1), b2=dt(b2), one_m_b2=dt(1.0 - b2), eps=dt(group["eps"]), wd=dt(wd),
                    decay_mul=dt(1.0 - lr * wd), neg_step_size=dt(-(lr / (1.0 - b1 ** t))), bc2s=dt(math.sqrt(1.0 - b2 ** t)))

    def _fill(self, b, h):
        g = b.group
        torch._foreach_add_([self.state[p]["step"] for p, _, _, _ in b.entries], 1)
        b.t = int(self.state[b.entries[0][0]]["step"])  # this launch is step number t of the bucket's parameters
        for k, v in self._hyper(g, b.t).items():
            setattr(h, k, v)
        wd = g["weight_decay"] != 0
        h.flags = (_lib.OPT_MAXIMIZE if g["maximize"] else 0) | \
            ((_lib.OPT_DECOUPLED if self._decoupled(g) else _lib.OPT_COUPLED_WD) if wd else 0)

    def _launch_bucket(self, L, b, block, coef, stream):
        _lib.check(L.btx_optim_adam(b.items, b.n_items, block, coef, stream))

    def _after(self, b):
        pass

    def _cpu_step(self, cpu):
        coef = self._cpu_coef(cpu)
        for group, p in cpu:
            self._check_group(group)
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            st["step"] += 1
            h = self._hyper(group, int(st["step"]), _dt(p))
            m, v = st["exp_avg"], st["exp_avg_sq"]
            g = p.grad.detach()
            if group["maximize"]:
                g = g.neg()
            if coef is not None:
                g = g.mul(coef)
            pn = p.detach()
            if group["weight_decay"] != 0:
                if self._decoupled(group):
                    pn = pn.mul(h["decay_mul"])
                else:
                    g = g.add(pn.mul(h["wd"]))
            m.copy_(m.add(g.sub(m).mul(h["one_m_b1"])))
            v.copy_(v.mul(h["b2"]).add(g.mul(h["one_m_b2"]).mul(g)))
            # a 1-d divisor: torch divides by a Python scalar as a multiplication with its reciprocal, which is another rounding
            # and the square root through float64: torch's vectorised f32 sqrt on the CPU is not correctly rounded (about 0.6 % of
            # the values are one ulp off); sqrt in float64 rounded to f32 is (53 >= 2 * 24 + 2 bits)
            root = v.sqrt() if v.dtype == torch.float64 else v.double().sqrt().to(v.dtype)
            den = root.div(torch.tensor([h["bc2s"]], dtype=p.dtype)).add(h["eps"])
            p.copy_(pn.add(m.mul(h["neg_step_size"]).div(den)))


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay, default weight_decay=0.01"""
    _torch_cls = torch.optim.AdamW
    _decoupled_default = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None, max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True, max_grad_norm=max_grad_norm)
