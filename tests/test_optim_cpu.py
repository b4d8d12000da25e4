"""bayesian_torch_amd.optim without a GPU: the numpy model of BTX-OPT v1 (tests/optim_model.py) against torch.optim in float64, the
CPU path of our classes against the model bit for bit, state_dict interchange with torch's classes, refused arguments, LR
schedulers, the version bump, and the host side of the C-ABI entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_model as OM  # noqa: E402

SGD_CONFIGS, ADAM_CONFIGS = OM.SGD_CONFIGS, OM.ADAM_CONFIGS
SHAPES = [(1,), (3,), (7, 5), (4, 3, 3, 3)]
STEPS = 5


def make_problem(dtype, seed=0):
    """parameters of magnitude 0.1 and STEPS gradients each, N(0,1) * 10^U(-6,0) with some exact zeros"""
    r = np.random.RandomState(seed)
    ps = [(0.1 * r.randn(*s)).astype(dtype) for s in SHAPES]
    gs = []
    for _ in range(STEPS):
        step = []
        for s in SHAPES:
            g = r.randn(*s) * 10.0 ** r.uniform(-6, 0, size=s)
            g[r.rand(*s) < 0.1] = 0.0
            step.append(g.astype(dtype))
        gs.append(step)
    return ps, gs


def run_model_sgd(ps, gs, dtype, cfg, coefs=None):
    ps = [p.copy() for p in ps]
    bufs = [None] * len(ps)
    for t, step in enumerate(gs):
        for i, g in enumerate(step):
            ps[i], bufs[i] = OM.sgd_step(ps[i], g, bufs[i], dtype=dtype, coef=None if coefs is None else coefs[t], **cfg)
    return ps, bufs


def run_model_adam(ps, gs, dtype, name, cfg, coefs=None):
    ps = [p.copy() for p in ps]
    ms = [np.zeros_like(p) for p in ps]
    vs = [np.zeros_like(p) for p in ps]
    if name == "AdamW":
        cfg = {"weight_decay": 0.01, **cfg}  # AdamW's default
    for t, step in enumerate(gs):
        for i, g in enumerate(step):
            ps[i], ms[i], vs[i] = OM.adam_step(ps[i], g, ms[i], vs[i], t + 1, dtype=dtype, decoupled=(name == "AdamW"),
                                               coef=None if coefs is None else coefs[t], **cfg)
    return ps, ms, vs


def run_optimizer(make, ps, gs, tdtype):
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(tdtype)) for p in ps]
    opt = make(params)
    for step in gs:
        for p, g in zip(params, step):
            p.grad = torch.from_numpy(g.copy()).to(tdtype)
        opt.step()
    return params, opt


@pytest.mark.parametrize("cfg", SGD_CONFIGS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_model_float64_is_torch_sgd(cfg):
    ps, gs = make_problem(np.float64)
    want, _ = run_optimizer(lambda p: torch.optim.SGD(p, foreach=False, **cfg), ps, gs, torch.float64)
    got, _ = run_model_sgd(ps, gs, np.float64, cfg)
    err = max(float(np.abs(a - b.detach().numpy()).max()) for a, b in zip(got, want))
    print("numpy model vs torch.optim.SGD float64, %s: max abs %.2e" % (cfg, err))
    assert err <= 1e-12


@pytest.mark.parametrize("name,cfg", ADAM_CONFIGS, ids=lambda c: c if isinstance(c, str) else "-".join("%s=%s" % kv for kv in c.items()))
def test_model_float64_is_torch_adam(name, cfg):
    ps, gs = make_problem(np.float64)
    want, _ = run_optimizer(lambda p: getattr(torch.optim, name)(p, foreach=False, **cfg), ps, gs, torch.float64)
    got, _, _ = run_model_adam(ps, gs, np.float64, name, cfg)
    err = max(float(np.abs(a - b.detach().numpy()).max()) for a, b in zip(got, want))
    print("numpy model vs torch.optim.%s float64, %s: max abs %.2e" % (name, cfg, err))
    assert err <= 1e-12


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("cfg", SGD_CONFIGS, ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
@pytest.mark.parametrize("clip", [None, 0.05])
def test_cpu_sgd_equals_the_f32_model_bit_for_bit(cfg, clip):
    from bayesian_torch_amd import optim
    ps, gs = make_problem(np.float32, seed=1)
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = optim.SGD(params, max_grad_norm=clip, **cfg)
    coefs = []
    for step in gs:
        for p, g in zip(params, step):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        coefs.append(None if clip is None else float(opt.clip_coef))
    want, bufs = run_model_sgd(ps, gs, np.float32, cfg, None if clip is None else coefs)
    if clip is not None:
        assert min(coefs) < 1.0  # the clip is active in this problem
    for p, w, b in zip(params, want, bufs):
        assert np.array_equal(_bits(p.detach().numpy()), _bits(w))
        if b is not None:
            assert np.array_equal(_bits(opt.state[p]["momentum_buffer"].numpy()), _bits(b))


@pytest.mark.parametrize("name,cfg", ADAM_CONFIGS, ids=lambda c: c if isinstance(c, str) else "-".join("%s=%s" % kv for kv in c.items()))
@pytest.mark.parametrize("clip", [None, 0.05])
def test_cpu_adam_equals_the_f32_model_bit_for_bit(name, cfg, clip):
    from bayesian_torch_amd import optim
    ps, gs = make_problem(np.float32, seed=2)
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = getattr(optim, name)(params, max_grad_norm=clip, **cfg)
    coefs = []
    for step in gs:
        for p, g in zip(params, step):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        coefs.append(None if clip is None else float(opt.clip_coef))
    want, ms, vs = run_model_adam(ps, gs, np.float32, name, cfg, None if clip is None else coefs)
    for p, w, m, v in zip(params, want, ms, vs):
        st = opt.state[p]
        assert float(st["step"]) == STEPS and st["step"].dtype == torch.float32 and st["step"].dim() == 0
        assert np.array_equal(_bits(p.detach().numpy()), _bits(w))
        assert np.array_equal(_bits(st["exp_avg"].numpy()), _bits(m))
        assert np.array_equal(_bits(st["exp_avg_sq"].numpy()), _bits(v))


def test_cpu_clip_coefficient_is_the_documented_formula():
    from bayesian_torch_amd import optim
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.tensor([3.0, 4.0, 0.0, 0.0])
    opt = optim.SGD([p], lr=1.0, max_grad_norm=1.0)
    opt.step()
    assert float(opt.total_norm) == 5.0
    assert np.float32(float(opt.clip_coef)) == OM.clip_coef(5.0, 1.0)
    assert torch.equal(p.grad, torch.tensor([3.0, 4.0, 0.0, 0.0]))  # p.grad itself is not rescaled (documented deviation)
    opt2 = optim.SGD([p], lr=1.0, max_grad_norm=10.0)
    opt2.step()
    assert float(opt2.clip_coef) == 1.0


@pytest.mark.parametrize("name,cfg", [("SGD", dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=0.01)),
                                      ("Adam", dict(lr=0.01, weight_decay=0.01)), ("AdamW", dict(lr=0.01))])
def test_state_dict_interchanges_with_torch_in_both_directions(name, cfg):
    """three steps with one class, state_dict into the other, two more steps; compared with five steps of torch's class alone.  The
    float64 parameters make the two implementations agree to rounding (see the float64 tests above)."""
    from bayesian_torch_amd import optim
    ps, gs = make_problem(np.float64, seed=3)
    ours = lambda p: getattr(optim, name)(p, **cfg)  # noqa: E731
    theirs = lambda p: getattr(torch.optim, name)(p, foreach=False, **cfg)  # noqa: E731
    want, _ = run_optimizer(theirs, ps, gs, torch.float64)
    for first, second in ((ours, theirs), (theirs, ours)):
        params, opt = run_optimizer(first, ps, gs[:3], torch.float64)
        sd = opt.state_dict()
        opt2 = second(params)
        opt2.load_state_dict(sd)
        assert opt2.state_dict()["param_groups"][0]["lr"] == cfg["lr"]
        for step in gs[3:]:
            for p, g in zip(params, step):
                p.grad = torch.from_numpy(g.copy())
            opt2.step()
        err = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(params, want))
        assert err <= 1e-12, err
        if name != "SGD":
            assert all(float(opt2.state[p]["step"]) == 5 for p in params)
    # the keys and the layout are torch's
    _, a = run_optimizer(ours, ps, gs[:1], torch.float64)
    _, b = run_optimizer(theirs, ps, gs[:1], torch.float64)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"][0].keys() == sb["param_groups"][0].keys()
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        for key, val in sa["state"][k].items():
            assert val.dtype == sb["state"][k][key].dtype and val.shape == sb["state"][k][key].shape


def test_state_shares_the_strides_of_the_parameter():
    from bayesian_torch_amd import optim
    phys = torch.randn(4, 3, 3, 2)
    p = torch.nn.Parameter(phys.permute(0, 3, 1, 2))  # GEMM-major storage, the reference's logical shape
    p.grad = torch.randn(4, 2, 3, 3)
    opt = optim.Adam([p], lr=0.1)
    opt.step()
    assert opt.state[p]["exp_avg"].stride() == p.stride() and opt.state[p]["exp_avg_sq"].stride() == p.stride()


def test_refused_arguments_raise_and_name_the_argument():
    from bayesian_torch_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam(p, amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.AdamW(p, amsgrad=True)
    with pytest.raises(ValueError, match="lr"):
        optim.Adam(p, lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="lr"):
        optim.SGD(p, lr=torch.tensor(1e-3))
    for cls in (optim.SGD, optim.Adam, optim.AdamW):
        for arg in ("foreach", "fused", "differentiable") + (() if cls is optim.SGD else ("capturable",)):
            with pytest.raises(ValueError, match=arg):
                cls(p, **{arg: True})
            cls(p, **{arg: False})
    with pytest.raises(ValueError, match="max_grad_norm"):
        optim.SGD(p, max_grad_norm=0.0)
    # a refused value that arrives through load_state_dict is refused at the step
    o = optim.Adam(p)
    sd = torch.optim.Adam(p, amsgrad=True).state_dict()
    o.load_state_dict(sd)
    p[0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="amsgrad"):
        o.step()
    sp = torch.nn.Parameter(torch.zeros(4, 2))
    sp.grad = torch.zeros(4, 2).to_sparse()
    from bayesian_torch_amd._lib import BtxError
    with pytest.raises(BtxError, match="sparse"):
        optim.SGD([sp]).step()


def test_parameters_without_a_gradient_are_skipped():
    from bayesian_torch_amd import optim
    a, b = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(3))
    a.grad = torch.ones(3)
    opt = optim.Adam([a, b], lr=0.1)
    opt.step()
    assert torch.equal(b.detach(), torch.ones(3)) and len(opt.state[b]) == 0 and not torch.equal(a.detach(), torch.ones(3))


def test_step_lr_changes_the_update():
    from bayesian_torch_amd import optim
    p = torch.nn.Parameter(torch.zeros(2))
    opt = optim.SGD([p], lr=1.0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    deltas = []
    for _ in range(3):
        before = p.detach().clone()
        p.grad = torch.ones(2)
        opt.step()
        sched.step()
        deltas.append(float((before - p.detach())[0]))
    assert deltas == [1.0, 0.5, 0.25]


def test_version_of_every_updated_parameter_grows():
    from bayesian_torch_amd import optim
    for cls in (optim.SGD, optim.Adam, optim.AdamW):
        ps = [torch.nn.Parameter(torch.zeros(n)) for n in (1, 5)]
        opt = cls(ps, lr=0.1)
        for _ in range(2):
            v = [p._version for p in ps]
            for p in ps:
                p.grad = torch.ones_like(p)
            opt.step()
            assert all(p._version > v0 for p, v0 in zip(ps, v))


def test_cabi_optimizer_entry_points_without_gpu():
    """argument errors return before anything is launched, so they can be checked without a device; the ABI number has not moved"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9
    for name in ("btx_optim_sgd", "btx_optim_adam", "btx_optim_grad_norm_workspace_bytes", "btx_optim_grad_norm"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert ctypes.sizeof(_lib.OptimHyper) == 64 and ctypes.sizeof(_lib.OptimItem) == 40
    E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4, -6
    blk, buf = 0x1000, 0x2000  # never dereferenced: every call below fails validation
    item = lambda **kw: _lib.OptimItem(**{**dict(p=buf, g=buf, state0=buf, state1=buf, n=8), **kw})  # noqa: E731
    arr = lambda *its: (_lib.OptimItem * len(its))(*its)  # noqa: E731
    one = arr(item())
    assert L.btx_optim_adam(one, 1, None, None, None) == E_NULL
    assert L.btx_optim_adam(None, 1, blk, None, None) == E_NULL
    assert L.btx_optim_adam(one, -1, blk, None, None) == E_SHAPE
    assert L.btx_optim_adam(one, 1, blk + 4, None, None) == E_ALIGN
    assert L.btx_optim_adam(arr(item(n=-1)), 1, blk, None, None) == E_SHAPE
    assert L.btx_optim_adam(arr(item(state1=None)), 1, blk, None, None) == E_NULL
    assert L.btx_optim_adam(arr(item(p=buf + 2)), 1, blk, None, None) == E_ALIGN
    assert L.btx_optim_adam(arr(item(), item(g=None)), 2, blk, None, None) == E_NULL  # the second item: nothing was launched for the first
    assert L.btx_optim_adam(one, _lib.OPTIM_MAX_ITEMS + 1, blk, None, None) == E_UNSUPPORTED
    assert L.btx_optim_adam(arr(item(n=0, p=None, g=None)), 1, blk, None, None) == 0  # empty items are skipped: nothing to launch
    assert L.btx_optim_adam(None, 0, blk, None, None) == 0
    assert L.btx_optim_sgd(arr(item(state0=None)), 1, blk, 1, None, None) == E_NULL
    assert L.btx_optim_sgd(arr(item(p=None, state0=None)), 1, blk, 0, None, None) == E_NULL
    assert L.btx_optim_sgd(one, 1, None, 0, None, None) == E_NULL
    assert L.btx_optim_sgd(arr(item(n=-5)), 1, blk, 0, None, None) == E_SHAPE
    # the norm: workspace arithmetic (one f64 per chunk, an upper bound from the totals) and validation
    assert L.btx_optim_grad_norm_workspace_bytes(3, 3 * _lib.OPTIM_CHUNK + 2) == (3 + 3) * 8
    assert L.btx_optim_grad_norm_workspace_bytes(0, 0) == 8
    assert L.btx_optim_grad_norm(one, 1, 1.0, None, buf, 64, None) == E_NULL
    assert L.btx_optim_grad_norm(one, 1, 1.0, buf, None, 64, None) == E_NULL
    assert L.btx_optim_grad_norm(one, 1, 0.0, buf, buf, 64, None) == E_SHAPE
    assert L.btx_optim_grad_norm(one, 1, float("nan"), buf, buf, 64, None) == E_SHAPE
    assert L.btx_optim_grad_norm(arr(item(n=2 * _lib.OPTIM_CHUNK + 1)), 1, 1.0, buf, buf, 16, None) == E_WORKSPACE
    assert L.btx_optim_grad_norm(arr(item(g=None)), 1, 1.0, buf, buf, 64, None) == E_NULL
    assert L.btx_optim_grad_norm(one, 1, 1.0, buf, buf + 4, 64, None) == E_ALIGN
