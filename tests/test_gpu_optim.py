"""GPU: bayesian_torch_amd.optim (csrc/btx_optim.hip, BTX-OPT v1) against its numpy model and against float64, and the update captured
inside autograd.GraphedTrainStep.

(a) five steps: parameters and state equal tests/optim_model.py in float32 BIT FOR BIT, for every option combination, with and
    without max_grad_norm (the model is fed the GPU's own coef word: the norm has its own check, (c)).
(b) one step from the same f32 state against the formula evaluated in float64 with the hyper-parameters in double, element by
    element inside a RUNNING ERROR BOUND that is carried through the same operations (class Err below).  u = 2^-24.  Every f32
    operation returns the exact result times (1 + d), |d| <= u (no underflow: the gradients are N(0,1) * 10^U(-6,0) or exactly 0,
    every intermediate is normal or exactly zero), and every host constant is the f32 rounding of a double, |c32 - c| <= u |c|.  With
    e_x the bound of |x32 - x|:
        z = x * y       e_z = |x| e_y + |y| e_x + e_x e_y + u (|z| + that)
        z = x +- y      e_z = e_x + e_y + u (|z| + e_x + e_y)
        z = x / y       e_z = (e_x + |z| e_y) / (|y| - e_y) + u (|z| + that)
        z = sqrt(x)     e_z = sqrt(x) - sqrt(max(x - e_x, 0)) + u (z + that)        (sqrt is concave: the lower side is the larger)
    so the bound is a count of roundings times 2^-24 times the magnitudes involved, accumulated operation by operation.  Nothing is
    fitted and there is no percentile: every element must lie inside.
(c) the norm: with small-integer gradients (|g| <= 3, fewer than 2^20 elements, sum of squares a perfect square) every lane sum
    (<= 16 * 9), every f64 partial and the square root are exact, so total_norm is exact.  With random gradients each lane sums at most
    BTX_OPTIM_CHUNK / 256 = 16 squares in f32: 1 rounding per square and at most 15 per term from the additions, (1 + u)^16 on every
    (positive) term; the f64 fold adds at most 2^20 * 2^-53; the square root halves the relative error and the f32 result is rounded
    once: |total_norm - ref| <= (16 / 2 + 1) u ref to first order, asserted as 10 u ref."""
import math
import os
import sys
import types
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_model as OM  # noqa: E402

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

U = 2.0 ** -24
STEPS = 5
CONFIGS = [("SGD", c) for c in OM.SGD_CONFIGS] + OM.ADAM_CONFIGS
IDS = ["%s-%s" % (n, "-".join("%s=%s" % kv for kv in c.items())) for n, c in CONFIGS]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else t
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the tensor set: every path of the kernel -----------------------------------------------------------------------------------
_SET = {}


def tensor_set():
    """host arrays, made once and left unchanged: (kind, p0, [g of step 0..4]) with kind in plain / view / conv / conv_cg.
    numel 1, 3, 64, 1000 (scalar tail, one float4 sweep, a ragged one), 4097 (one chunk + 1 element), 70 000 (18 chunks), a view at
    a 4-byte offset (no 16-byte access), 50 one-element tensors (two tables of <= 48 items), a GEMM-major conv parameter with a
    gradient of its own strides and the same with a contiguous gradient (staged)"""
    if _SET:
        return _SET["items"]
    r = np.random.RandomState(1234)

    def grads(shape):
        out = []
        for _ in range(STEPS):
            g = r.randn(*shape) * 10.0 ** r.uniform(-6, 0, size=shape)
            g[r.rand(*shape) < 0.1] = 0.0
            out.append(g.astype(np.float32))
        return out
    items = []
    for n in (1, 3, 64, 1000, 4097, 70000):
        items.append(("plain", (0.1 * r.randn(n)).astype(np.float32), grads((n,))))
    items.append(("view", (0.1 * r.randn(1001)).astype(np.float32), grads((1001,))))
    for _ in range(50):
        items.append(("plain", (0.1 * r.randn(1)).astype(np.float32), grads((1,))))
    conv = (0.1 * r.randn(16, 8, 3, 3)).astype(np.float32)
    items.append(("conv", conv, grads(conv.shape)))
    items.append(("conv_cg", conv.copy(), grads(conv.shape)))
    _SET["items"] = items
    return items


def make_params(dev):
    """the tensor set as nn.Parameters on the GPU, and set_grads(step) that attaches the gradients of one step"""
    from bayesian_torch_amd import functional as BF
    op = types.SimpleNamespace(nd=2, transposed=False, groups=1)
    params = []
    for kind, p0, _ in tensor_set():
        if kind == "view":
            base = torch.zeros(p0.size + 8, device=dev)
            p = torch.nn.Parameter(base[1:1 + p0.size])
            assert p.data_ptr() % 16 == 4
        elif kind.startswith("conv"):
            p = torch.nn.Parameter(BF.gemm_major_param(p0.shape, op).to(dev))
            assert p.stride() != torch.empty(p0.shape).stride() and not p.is_contiguous()
        else:
            p = torch.nn.Parameter(torch.empty(p0.shape, device=dev))
        with torch.no_grad():
            p.copy_(torch.from_numpy(p0))
        params.append(p)

    def set_grads(step):
        for (kind, _, gs), p in zip(tensor_set(), params):
            g = torch.from_numpy(gs[step]).to(dev)
            if kind == "conv":
                g2 = torch.empty_like(p)  # the parameter's own (GEMM-major) strides: read in place
                g2.copy_(g)
                g = g2
                assert g.stride() == p.stride()
            elif kind == "conv_cg":
                assert g.is_contiguous() and g.stride() != p.stride()  # the staging path
            p.grad = g
    return params, set_grads


def model_step(name, cfg, p, g, st, t, coef, dtype=np.float32):
    """one step of the numpy model on one tensor; st: dict of the state arrays (updated in place)"""
    if name == "SGD":
        p, st["buf"] = OM.sgd_step(p, g, st.get("buf"), dtype=dtype, coef=coef, **cfg)
        return p
    if name == "AdamW":
        cfg = {"weight_decay": 0.01, **cfg}
    p, st["m"], st["v"] = OM.adam_step(p, g, st.get("m", np.zeros_like(p)), st.get("v", np.zeros_like(p)), t, dtype=dtype,
                                       decoupled=(name == "AdamW"), coef=coef, **cfg)
    return p


def assert_state_equals(opt, name, p, st, where):
    s = opt.state[p]
    if name == "SGD":
        if st.get("buf") is not None:
            assert np.array_equal(_bits(s["momentum_buffer"]), _bits(st["buf"])), ("momentum_buffer",) + where
            assert s["momentum_buffer"].stride() == p.stride() or p.numel() == 1
    else:
        assert np.array_equal(_bits(s["exp_avg"]), _bits(st["m"])), ("exp_avg",) + where
        assert np.array_equal(_bits(s["exp_avg_sq"]), _bits(st["v"])), ("exp_avg_sq",) + where


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 0.3], ids=["noclip", "clip"])
@pytest.mark.parametrize("name,cfg", CONFIGS, ids=IDS)
def test_five_steps_equal_the_numpy_model_bit_for_bit(name, cfg, clip):
    from bayesian_torch_amd import optim
    dev = _dev()
    params, set_grads = make_params(dev)
    opt = getattr(optim, name)(params, max_grad_norm=clip, **cfg)
    want = [p0.copy() for _, p0, _ in tensor_set()]
    states = [dict() for _ in want]
    for step in range(STEPS):
        versions = [p._version for p in params]
        set_grads(step)
        opt.step()
        coef = None
        if clip is not None:
            coef = float(opt.clip_coef)
            assert coef < 1.0  # the clip is active on this set
        assert all(p._version > v for p, v in zip(params, versions))
        for i, (_, _, gs) in enumerate(tensor_set()):
            want[i] = model_step(name, cfg, want[i], gs[step], states[i], step + 1, coef)
    for i, p in enumerate(params):
        assert np.array_equal(_bits(p), _bits(want[i])), (i, tensor_set()[i][0], p.numel())
        assert_state_equals(opt, name, p, states[i], (i,))
        if name != "SGD":
            assert float(opt.state[p]["step"]) == STEPS and not opt.state[p]["step"].is_cuda


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
class Err:
    """a float64 value with a bound of |f32 result - value|, carried through the operations (see the header)"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    @staticmethod
    def const(c):  # a host double rounded to f32 once
        return Err(np.float64(c), abs(c) * U)

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        z = self.v * o.v
        e = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        return Err(z, e + U * (np.abs(z) + e))

    def _addsub(self, o, z):
        e = self.e + o.e
        return Err(z, e + U * (np.abs(z) + e))

    def __add__(self, o):
        return self._addsub(o, self.v + o.v)

    def __sub__(self, o):
        return self._addsub(o, self.v - o.v)

    def __truediv__(self, o):
        z = self.v / o.v
        den = np.abs(o.v) - o.e
        assert (den > 0).all()
        e = (self.e + np.abs(z) * o.e) / den
        return Err(z, e + U * (np.abs(z) + e))

    def sqrt(self):
        z = np.sqrt(self.v)
        e = z - np.sqrt(np.maximum(self.v - self.e, 0.0))
        return Err(z, e + U * (z + e))


def bound_step(name, cfg, p, g, st, t, coef):
    """the step in float64 with its running error bound: returns dict of Err for p and the state"""
    C = Err.const
    P, G = Err(p), Err(g)
    if cfg.get("maximize"):
        G = -G
    if coef is not None:
        G = G * Err(np.float64(coef))  # the f32 word itself: exact
    wd = cfg.get("weight_decay", 0.01 if name == "AdamW" else 0.0)
    lr = cfg["lr"]
    if name == "SGD":
        if wd:
            G = G + C(wd) * P
        out = {}
        mom = cfg.get("momentum", 0.0)
        if mom:
            B = C(mom) * Err(st["buf"]) + C(1.0 - cfg.get("dampening", 0.0)) * G
            out["buf"] = B
            G = G + C(mom) * B if cfg.get("nesterov") else B
        out["p"] = P + C(-lr) * G
        return out
    b1, b2 = cfg.get("betas", (0.9, 0.999))
    if wd and name == "Adam":
        G = G + C(wd) * P
    if wd and name == "AdamW":
        P = P * C(1.0 - lr * wd)
    M, V = Err(st["m"]), Err(st["v"])
    M = M + C(1.0 - b1) * (G - M)
    V = C(b2) * V + (C(1.0 - b2) * G) * G
    den = V.sqrt() / C(math.sqrt(1.0 - b2 ** t)) + C(cfg.get("eps", 1e-8))
    P = P + (C(-(lr / (1.0 - b1 ** t))) * M) / den
    return {"p": P, "m": M, "v": V}


@pytest.mark.parametrize("clip", [None, 0.3], ids=["noclip", "clip"])
@pytest.mark.parametrize("name,cfg", CONFIGS, ids=IDS)
def test_single_step_lies_inside_the_float64_error_bound(name, cfg, clip):
    """two steps to reach a state with history, then ONE step from that f32 state on the GPU against float64"""
    from bayesian_torch_amd import optim
    dev = _dev()
    params, set_grads = make_params(dev)
    opt = getattr(optim, name)(params, max_grad_norm=clip, **cfg)
    for step in range(2):
        set_grads(step)
        opt.step()
    key = {"SGD": {"buf": "momentum_buffer"}}.get(name, {"m": "exp_avg", "v": "exp_avg_sq"})
    before = []
    for p in params:
        s = opt.state[p]
        before.append((p.detach().cpu().numpy().copy(), {k: s[tk].cpu().numpy().copy() for k, tk in key.items() if tk in s}))
    set_grads(2)
    opt.step()
    coef = None if clip is None else float(opt.clip_coef)
    worst = 0.0
    for i, ((_, _, gs), p) in enumerate(zip(tensor_set(), params)):
        p0, st = before[i]
        out = bound_step(name, cfg, p0, gs[2], st, 3, coef)
        got = {"p": p.detach().cpu().numpy()}
        got.update({k: opt.state[p][tk].cpu().numpy() for k, tk in key.items() if k in out})
        for k, e in out.items():
            d = np.abs(got[k].astype(np.float64) - e.v)
            assert (d <= e.e).all(), (i, k, float(d.max()), float(e.e[d > e.e].min()))
            worst = max(worst, float((d / np.maximum(e.e, 1e-300)).max()))
    print("%s %s clip=%s: worst |gpu - f64| / bound = %.3f" % (name, cfg, clip, worst))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def _norm_run(grads, max_norm, dev):
    from bayesian_torch_amd import optim
    params = [torch.nn.Parameter(torch.zeros(g.shape, device=dev)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).to(dev)
    opt = optim.SGD(params, lr=0.0, max_grad_norm=max_norm)
    opt.step()
    a = (opt.total_norm.clone(), opt.clip_coef.clone())
    opt.step()
    b = (opt.total_norm.clone(), opt.clip_coef.clone())
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))  # fixed order, no atomics
    return float(a[0]), float(a[1])


def test_norm_of_small_integer_gradients_is_exact():
    dev = _dev()
    r = np.random.RandomState(7)
    grads = [r.randint(-3, 4, size=p0.shape).astype(np.float32) for _, p0, _ in tensor_set()]
    total = sum(int((g.astype(np.int64) ** 2).sum()) for g in grads)
    assert sum(g.size for g in grads) <= 2 ** 20
    root = math.isqrt(total) + 1
    big = max(grads, key=lambda g: g.size)
    zeros = np.flatnonzero(big == 0)
    need = root * root - total  # that many zeros become +-1
    assert 0 < need <= zeros.size
    big.reshape(-1)[zeros[:need]] = np.where(r.rand(need) < 0.5, -1.0, 1.0)
    assert sum(int((g.astype(np.int64) ** 2).sum()) for g in grads) == root * root and root < 2 ** 24
    norm, coef = _norm_run(grads, 2.0 * root, dev)
    assert norm == float(root)
    assert coef == 1.0  # below max_norm: exactly 1
    norm, coef = _norm_run(grads, 0.5 * root, dev)
    assert norm == float(root) and np.float32(coef) == OM.clip_coef(root, 0.5 * root)


def test_norm_of_random_gradients_lies_inside_the_float64_bound():
    dev = _dev()
    grads = [gs[0] for _, _, gs in tensor_set()]
    ref = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads))
    norm, coef = _norm_run(grads, 0.3, dev)
    print("total_norm %.9g, float64 %.9g, rel %.2e (bound %.2e)" % (norm, ref, abs(norm - ref) / ref, 10 * U))
    assert abs(norm - ref) <= 10 * U * ref
    assert np.float32(coef) == OM.clip_coef(np.float32(norm), 0.3) and coef < 1.0


def test_gpu_parameters_that_cannot_take_the_kernel_raise():
    from bayesian_torch_amd import optim
    from bayesian_torch_amd._lib import BtxError
    dev = _dev()
    p = torch.nn.Parameter(torch.zeros(8, 8, device=dev)[:, ::2])  # not dense
    p.grad = torch.ones_like(p)
    with pytest.raises(BtxError, match="dense"):
        optim.SGD([p]).step()
    h = torch.nn.Parameter(torch.zeros(8, device=dev, dtype=torch.bfloat16))
    h.grad = torch.ones_like(h)
    with pytest.raises(BtxError, match="float32"):
        optim.Adam([h]).step()


# ---- the update inside GraphedTrainStep --------------------------------------------------------------------------------------------
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


class SeqNet2(torch.nn.Module):
    # two LSTM layers and a head without bias (tests/test_gpu_lstm_train_fused.py: the captured Linear bias gradient is a separate matter)
    def __init__(self, i=24, h=40, classes=5):
        super().__init__()
        self.lstm1 = torch.nn.LSTM(i, h)
        self.lstm2 = torch.nn.LSTM(h, h)
        self.fc = torch.nn.Linear(h, classes, bias=False)

    def forward(self, x):
        out, _ = self.lstm1(x)
        out, _ = self.lstm2(out)
        return self.fc(out[:, -1, :])


def build(kind):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import fuse_model
    dev = _dev()
    bt.manual_seed(9)
    bt.set_precision("f32")
    torch.manual_seed(0)
    if kind == "conv":
        # (no bias in front of the BatchNorm, as in the ResNets: its gradient would be nothing but the rounding noise of the sums)
        net = torch.nn.Sequential(torch.nn.Conv2d(3, 32, 3, padding=1, bias=False), torch.nn.BatchNorm2d(32), torch.nn.ReLU(),
                                  torch.nn.Conv2d(32, 64, 3, stride=2, padding=1), torch.nn.ReLU(),
                                  torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(64, 10))
        bt.dnn_to_bnn(net, dict(PRIOR, type="Flipout"))
        net = net.to(dev).train()
        assert fuse_model(net) >= 1
        torch.manual_seed(1)
        x = torch.randn(16, 3, 16, 16, device=dev)
        y = torch.randint(0, 10, (16,), device=dev)
    else:
        net = SeqNet2()
        bt.dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
        net = net.to(dev).train()
        assert fuse_model(net, lstm_training=True) == 2
        torch.manual_seed(1)
        x = torch.randn(4, 6, 24, device=dev)
        y = torch.randint(0, 5, (4,), device=dev)
    bt.assign_layer_ids(net)
    return net, x, y


def eager_backward(net, x, y, s):
    import bayesian_torch_amd as bt
    for p in net.parameters():
        p.grad = None
    bt.set_sample_index(net, s)
    out = net(x)
    loss = torch.nn.functional.cross_entropy(out.float(), y) + bt.get_kl_loss(net) / x.shape[0]
    loss.backward()
    return float(loss)


OPTS = [("Adam", dict(lr=1e-2, weight_decay=1e-3), 0.5), ("SGD", dict(lr=0.05, momentum=0.9, weight_decay=1e-3), None)]


def _state_arrays(opt, name, p):
    s = opt.state.get(p, {})
    if name == "SGD":
        b = s.get("momentum_buffer")
        return {} if b is None else {"buf": b.detach().cpu().numpy().copy()}
    return {"m": s["exp_avg"].cpu().numpy().copy(), "v": s["exp_avg_sq"].cpu().numpy().copy()} if "exp_avg" in s else {}


@pytest.mark.parametrize("name,cfg,clip", OPTS, ids=["Adam-clip", "SGD-momentum"])
@pytest.mark.parametrize("kind", ["conv", "lstm"])
def test_captured_update_equals_the_model_and_the_eager_step(kind, name, cfg, clip):
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = build(kind)
    params = list(net.parameters())
    start = [p.detach().clone() for p in params]
    # the eager step from the same start
    opt_e = getattr(optim, name)(params, max_grad_norm=clip, **cfg)
    eager_backward(net, x, y, 7)
    opt_e.step()
    eager = [p.detach().clone() for p in params]
    with torch.no_grad():
        for p, s in zip(params, start):
            p.copy_(s)
    for m in net.modules():  # (a Flipout LSTM would keep its last KL with its graph; harmless elsewhere)
        if hasattr(m, "kl"):
            m.kl = None
    # construction changes neither the parameters nor the optimizer's state (here: a state with history, loaded from opt_e)
    opt = getattr(optim, name)(params, max_grad_norm=clip, **cfg)
    if name == "SGD":
        opt.load_state_dict(opt_e.state_dict())  # the momentum buffers of the eager step: not a first step any more
    state_before = [{k: v.clone() for k, v in opt.state.get(p, {}).items()} for p in params]
    with pytest.raises(TypeError):
        GraphedTrainStep(net, x, y, optimizer=torch.optim.SGD(params, lr=0.1))
    gs = GraphedTrainStep(net, x, y, optimizer=opt)
    try:
        torch.cuda.synchronize()
        for p, s, sb in zip(params, start, state_before):
            assert torch.equal(p.detach(), s)
            for k, v in sb.items():
                assert torch.equal(opt.state[p][k], v), k
            if name != "SGD" and p in opt.state and "step" in opt.state[p]:
                assert float(opt.state[p]["step"]) == 0.0
                assert not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any()
        for r, s in enumerate((7, 8, 9)):
            if r == 2:
                opt.param_groups[0]["lr"] = cfg["lr"] * 0.25  # an lr changed between replays is honoured
            snap = [(p.detach().cpu().numpy().copy(), _state_arrays(opt, name, p)) for p in params]
            versions = [p._version for p in params]
            loss = gs.run(s)
            torch.cuda.synchronize()
            coef = None if clip is None else float(opt.clip_coef)
            c = dict(cfg, lr=opt.param_groups[0]["lr"])
            gmax = max(float(p.grad.abs().max()) for p in params if p.grad is not None)
            print("%s %s replay %d: loss %.6f, max |grad| %.3e, coef %s" % (kind, name, r, float(loss), gmax, coef))
            assert math.isfinite(float(loss)) and math.isfinite(gmax)
            for i, p in enumerate(params):
                if p.grad is None:
                    assert torch.equal(p.detach().cpu(), torch.from_numpy(snap[i][0]))
                    continue
                p0, st = snap[i]
                want = model_step(name, c, p0, p.grad.detach().cpu().numpy(), st, r + 1, coef)
                assert np.array_equal(_bits(p), _bits(want)), (kind, name, r, i)
                assert_state_equals(opt, name, p, st, (kind, r, i))
                assert p._version > versions[i]
            assert torch.isfinite(loss).all()
            if r == 0 and name != "SGD":
                # the first replay against the eager step from the same start (tests/test_gpu_backward.py: captured against eager,
                # rel-L2 1e-5: the weight gradient's f32 atomics may reorder sums)
                rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
                errs = [rel(p.detach(), e) for p, e in zip(params, eager)]
                print("captured vs eager %s step on %s: parameter rel-L2 max %.1e" % (name, kind, max(errs)))
                assert max(errs) < 1e-5, errs
        if name == "SGD":
            opt.param_groups[0]["lr"] = 0.0   # lr = 0 (and the decay through it): the replay must leave the parameters alone
            opt.param_groups[0]["weight_decay"] = 0.0
            keep = [p.detach().clone() for p in params]
            gs.run(10)
            torch.cuda.synchronize()
            assert all(torch.equal(p.detach(), k) for p, k in zip(params, keep))
    finally:
        gs.close()


def test_captured_sgd_first_replay_equals_the_eager_first_step():
    """SGD is linear in the gradient, so the file's captured-against-eager criterion (rel-L2 1e-5) carries over to the parameters; the
    first replay is also the step that writes the momentum buffers (buf = g)"""
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    for kind in ("conv", "lstm"):
        net, x, y = build(kind)
        params = list(net.parameters())
        start = [p.detach().clone() for p in params]
        cfg = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-3)
        opt_e = optim.SGD(params, **cfg)
        eager_backward(net, x, y, 7)
        opt_e.step()
        eager = [p.detach().clone() for p in params]
        ebuf = [opt_e.state[p]["momentum_buffer"].clone() for p in params if p.grad is not None]
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
        opt = optim.SGD(params, **cfg)
        gs = GraphedTrainStep(net, x, y, optimizer=opt)
        try:
            assert all("momentum_buffer" not in opt.state.get(p, {}) for p in params)  # nothing a state_dict() could mistake for history
            gs.run(7)
            torch.cuda.synchronize()
            rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))  # noqa: E731
            errs = [rel(p.detach(), e) for p, e in zip(params, eager)]
            berr = [rel(opt.state[p]["momentum_buffer"], b) for p, b in zip([p for p in params if p.grad is not None], ebuf)]
            worst = [n for n, p in net.named_parameters() if p.grad is not None][int(np.argmax(berr))]
            print("captured vs eager SGD first step on %s: parameters %.1e, momentum buffers %.1e (worst: %s)" % (
                kind, max(errs), max(berr), worst))
            assert max(errs) < 1e-5 and max(berr) < 1e-5
        finally:
            gs.close()


def test_every_replay_gives_the_eager_gradients_biases_included():
    """the update consumes the gradients of EVERY replay.  The bias sums of the weight-gradient launch are accumulated with atomics
    into vectors that must be zero on entry; zeroed by memset nodes, the 40-byte vectors of a 10-class head kept part of what the
    graph's pool held there on replays after the first (inf / NaN in fc.rho_bias).  Same parameters, same sample index: replays 0..3
    against the eager step, the file's criterion for captured against eager gradients (rel-L2 1e-5)."""
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = build("conv")
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())
    want = {}
    for s in (3, 4):
        eager_backward(net, x, y, s)
        want[s] = [p.grad.detach().clone() for p in params]
    gs = GraphedTrainStep(net, x, y)
    try:
        for r, s in enumerate((3, 4, 3, 4)):
            gs.run(s)
            torch.cuda.synchronize()
            errs = [float((p.grad - w).norm() / w.norm().clamp_min(1e-30)) for p, w in zip(params, want[s])]
            print("replay %d (sample %d): gradient rel-L2 max %.1e (%s)" % (r, s, max(errs), names[int(np.argmax(errs))]))
            assert all(torch.isfinite(p.grad).all() for p in params)
            assert max(errs) < 1e-5, dict(zip(names, errs))
    finally:
        gs.close()


def test_folded_eval_batchnorm_sees_the_captured_update():
    """models.fuse keys its folded (scale, shift) on (data_ptr, _version) of the BatchNorm tensors; a replay writes them through raw
    pointers, so only the version bump of run() makes the next eval forward fold again"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep
    net, x, y = build("conv")
    opt = optim.Adam(net.parameters(), lr=0.05)
    gs = GraphedTrainStep(net, x, y, optimizer=opt)
    try:
        bn = net[1]
        net.eval()
        with torch.no_grad():
            y0 = net(x).clone()       # the folded scale / shift are cached now
        w0 = bn.weight.detach().clone()
        net.train()
        gs.run(1)
        gs.run(2)
        torch.cuda.synchronize()
    finally:
        gs.close()
    assert float((bn.weight.detach() - w0).abs().max()) > 0.05  # the BatchNorm weights moved: a stale fold would be off by percents
    net.eval()
    with torch.no_grad():
        bt.set_sample_index(net, 5)
        y1 = net(x).clone()
        h = bn.register_forward_hook(lambda *a: None)  # a hooked module makes the site run the original ops: the unfolded reference
        bt.set_sample_index(net, 5)
        ref = net(x).clone()
        h.remove()
    rel = float((y1 - ref).norm() / ref.norm())
    print("folded eval forward after two captured updates vs the unfolded ops: rel-L2 %.1e (before the updates: %.1e)" % (
        rel, float((y0 - ref).norm() / ref.norm())))
    assert rel < 1e-4


def test_twenty_eager_adam_steps_reduce_the_loss():
    from bayesian_torch_amd import optim
    net, x, y = build("conv")
    opt = optim.Adam(net.parameters(), lr=1e-2)
    losses = []
    for s in range(20):
        losses.append(eager_backward(net, x, y, s))
        opt.step()
    print("our Adam, 20 eager steps: loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0] - 0.1, losses
