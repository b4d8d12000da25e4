"""BTX-REG v1 without a GPU: the CPU paths of mc.GaussianStats / mc.RegressionEvaluator against the numpy model of tests/reg_model.py
bit for bit, the float64 ATen chain of utils.mc_loss.mc_gaussian_nll against F.gaussian_nll_loss and the closed-form gradients, and the
argument errors of the new entry points through the library (every such call returns before anything is launched).

Tolerances: float64 quantities computed by two different but mathematically equal operation sequences of a few dozen operations are
compared at 1e-12 relative (2^-53 = 1.1e-16 per operation, magnitudes of the terms within 1e3 of the result); everything the model
defines operation by operation is compared exactly."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import reg_model as RM


def _mods():
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.utils import mc_loss as M
    return mc, M


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- 1. moment statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variance", ["log", None])
@pytest.mark.parametrize("shape", [(1, 3, 1), (4, 5, 3), (3, 2, 1025)])
def test_gaussian_stats_equal_the_model_bit_for_bit(shape, variance):
    mc, _ = _mods()
    lanes, bs, D = shape
    W = 2 * D if variance == "log" else D
    out = np.random.RandomState(7).randn(lanes * bs, W).astype(np.float32) * 3
    st = mc.GaussianStats(variance)
    assert st.numel(bs, W) == RM.numel(bs, D) == 3 * bs * D + 2
    packed = torch.zeros(st.numel(bs, W), dtype=torch.float64)
    st.accumulate_lanes(packed, torch.from_numpy(out), lanes, kl=0.75)
    want = RM.accumulate_lanes(np.zeros(RM.numel(bs, D)), out, lanes, D, variance == "log", kl=0.75)
    assert np.array_equal(_bits(packed.numpy()), _bits(want))
    if variance is None:
        assert not packed[2 * bs * D:3 * bs * D].any()
    # lanes in one call == one call per sample; bf16 outputs widen exactly
    seq = torch.zeros_like(packed)
    for k in range(lanes):
        st.accumulate(seq, torch.from_numpy(out[k * bs:(k + 1) * bs]), kl=0.75)
    assert torch.equal(seq, packed)
    ob = torch.from_numpy(out).to(torch.bfloat16)
    pb = st.accumulate_lanes(torch.zeros_like(packed), ob, lanes)
    wb = RM.accumulate_lanes(np.zeros(RM.numel(bs, D)), ob.float().numpy(), lanes, D, variance == "log")
    assert np.array_equal(_bits(pb.numpy()), _bits(wb))


def test_unpack_against_numpy_moments():
    mc, _ = _mods()
    S, bs, D = 6, 4, 3
    r = np.random.RandomState(3)
    out = (r.randn(S, bs, 2 * D) + 50.0).astype(np.float32)  # un-standardised: E[m^2] - E[m]^2 would cancel in f32
    out[..., D:] = r.uniform(-2, 2, (S, bs, D)).astype(np.float32)
    st = mc.GaussianStats("log")
    packed = st.accumulate_lanes(torch.zeros(st.numel(bs, 2 * D), dtype=torch.float64), torch.from_numpy(out.reshape(S * bs, 2 * D)), S,
                                 kl=2.0)
    u = st.unpack(packed, bs)
    m = out[..., :D].astype(np.float64)
    v = RM.expf32(out[..., D:])
    for got, want in ((u["mean"], m.mean(0)), (u["aleatoric_var"], v.mean(0)), (u["total_var"], m.var(0) + v.mean(0))):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the difference of two numbers near 2500: 1e-12 of THEIR magnitude
    assert np.abs(u["epistemic_var"].numpy() - m.var(0)).max() <= 1e-12 * (m * m).mean(0).max()
    assert float(u["kl"]) == 2.0 and float(u["samples"]) == S
    w = RM.unpack(packed.numpy(), bs)
    for k in ("mean", "epistemic_var", "aleatoric_var", "total_var"):
        assert np.array_equal(_bits(u[k].numpy()), _bits(w[k])), k


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from bayesian_torch_amd import layers as L
        self.a = L.LinearReparameterization(8, 16)
        self.b = L.LinearReparameterization(16, 2)

    def forward(self, x):
        h, _ = self.a(x)
        o, _ = self.b(torch.relu(h))
        return o


def test_two_emulated_ranks_add_up_to_one_rank():
    import bayesian_torch_amd as bt
    mc, _ = _mods()
    bt.manual_seed(5)
    torch.manual_seed(0)
    net = _Net().eval()
    bt.assign_layer_ids(net)
    x = torch.randn(8, 8)
    st = mc.GaussianStats("log")
    one = mc.mc_forward(net, x, 6, stats=st, reduce=False)
    assert one.dtype == torch.float64 and one.numel() == 3 * 8 + 2 and float(one[-1]) == 6
    parts = [mc.mc_forward(net, x, 6, stats=st, rank=r, world=2, reduce=False) for r in (0, 1)]
    both = parts[0] + parts[1]
    assert float((both - one).abs().max()) <= 1e-12 * float(one.abs().max())
    assert float(parts[0][-1]) == 3 and not torch.equal(parts[0], parts[1])
    # stats=None is the softmax layout, untouched
    cls = mc.mc_forward(net, x, 2, reduce=False)
    assert cls.dtype == torch.float32 and cls.numel() == mc.packed_numel(8, 2)
    b = mc.mc_forward_batched(net, x, 4, chunk=2, stats=st)
    assert b.dtype == torch.float64 and float(b[-1]) == 4


# ---- 2. the head: float64 chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_chain_loss_form_equals_gaussian_nll_loss(full):
    _, M = _mods()
    S, B, D = 4, 7, 5
    st, y = RM.head_case(S, B, D)
    st, y = torch.from_numpy(st).double(), torch.from_numpy(y).double()
    got = M._mc_gnll_chain(st, y, None, "loss", "log", None, full)
    m, s = st[..., :D], st[..., D:]
    want = F.gaussian_nll_loss(m, y.expand(S, B, D), torch.exp(s), full=full, eps=1e-6, reduction="sum") / (S * B)
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    # with a KL term and through the public face (CPU tensors run the chain)
    withkl = M.mc_gaussian_nll(st, y, torch.tensor(RM.KL, dtype=torch.float64), "loss", full=full)
    assert abs(float(withkl) - (float(want) + RM.KL / B)) <= 1e-12 * abs(float(withkl))
    # variance=None: s = log(noise_var), a constant
    got0 = M.mc_gaussian_nll(m, y, None, "loss", None, RM.NOISE_VAR, full)
    want0 = F.gaussian_nll_loss(m, y.expand(S, B, D), torch.full_like(m, RM.NOISE_VAR), full=full, eps=1e-6, reduction="sum") / (S * B)
    assert abs(float(got0) - float(want0)) <= 1e-12 * abs(float(want0))


def test_chain_moments_gradients_equal_the_closed_form():
    _, M = _mods()
    S, B, D = 4, 7, 5
    st, y = RM.head_case(S, B, D)
    t = torch.from_numpy(st).double().requires_grad_(True)
    M._mc_gnll_chain(t, torch.from_numpy(y).double(), None, "moments").backward()
    want = RM.moments_grad_closed_form(st, y)
    assert np.abs(t.grad.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the envelope module's own float64 values are the chain's
    for reduce in ("loss", "moments"):
        t = torch.from_numpy(st).double().requires_grad_(True)
        loss = M._mc_gnll_chain(t, torch.from_numpy(y).double(), RM.KL, reduce, full=True)
        loss.backward()
        ref = RM.gnll_reference(st, y, reduce, full=True, kl=RM.KL)
        assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert np.abs(ref["grad"] - t.grad.numpy()).max() <= 1e-12 * np.abs(ref["grad"]).max()


def test_one_sample_moments_equal_loss():
    _, M = _mods()
    st, y = RM.head_case(1, 9, 4)
    st, y = torch.from_numpy(st).double(), torch.from_numpy(y).double()
    a, b = M._mc_gnll_chain(st, y, 2.0, "moments"), M._mc_gnll_chain(st, y, 2.0, "loss")
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))


def test_the_f32_cpu_chain_stays_inside_the_envelope():
    """the envelope is derived for singly rounded f32 operations: the gradients of the f32 ATen chain on the CPU are such a sequence; and
    the envelope is useful at every element (at most USEFUL of |ref| + mean|ref|)"""
    _, M = _mods()
    for S, B, D in [(2, 3, 1), (4, 7, 5), (32, 2, 3)]:
        st, y = RM.head_case(S, B, D)
        for reduce in ("loss", "moments"):
            t = torch.from_numpy(st).requires_grad_(True)
            M._mc_gnll_chain(t, torch.from_numpy(y), None, reduce).backward()
            ref = RM.gnll_reference(st, y, reduce)
            # a plausibility check of the envelope itself: torch's backward forms the same products and quotients per element, in
            # another order, with ATen's own exp / log (observed: at most 0.4 of the bound)
            assert (np.abs(t.grad.numpy() - ref["grad"]) <= ref["b_pre"]).all(), (S, B, D, reduce)
            assert (ref["b_pre"] <= RM.USEFUL * (np.abs(ref["grad"]) + np.abs(ref["grad"]).mean())).all(), (S, B, D, reduce)


def test_head_argument_errors():
    _, M = _mods()
    st, y = torch.zeros(2, 3, 4), torch.zeros(3, 2)
    with pytest.raises(ValueError):
        M.mc_gaussian_nll(st, y, reduce="logits")
    with pytest.raises(ValueError):
        M.mc_gaussian_nll(st, y, variance="exp")
    with pytest.raises(ValueError):
        M.mc_gaussian_nll(st[..., :3], y)          # odd width
    with pytest.raises(ValueError):
        M.mc_gaussian_nll(st, y, variance=None)    # no noise_var
    with pytest.raises(ValueError):
        M.mc_gaussian_nll(st, torch.zeros(3, 3))
    with pytest.raises(ValueError):
        M.MCGaussianNLL(variance=None, noise_var=0.0)
    assert float(M.MCGaussianNLL("moments")(st, y)) == 0.0  # log 1 + 0 / 1


# ---- 3. the evaluator -----------------------------------------------------------------------------------------------------------
def _evaluator(mc, c, capacity=0, device=None):
    return mc.RegressionEvaluator(c["D"], levels=c["levels"], noise_var=c["noise_var"], capacity=capacity, device=device)


@pytest.mark.parametrize("case", [(3, 1, 4, "log"), (7, 5, 4, None), (3, 1366, 8, "log"), (9, 500, 1, "log")])
def test_evaluator_equals_the_model_bit_for_bit(case):
    mc, _ = _mods()
    bs, D, K, variance = case
    c = RM.eval_case(bs, D, K, seed=11, variance=variance)
    cap = bs * D + 5
    ev = _evaluator(mc, c, capacity=cap)
    state, rec = RM.new_state(K), np.zeros((cap, 4), np.float32)
    z2 = RM.z2_of(c["levels"])
    for _ in range(2):  # the second batch overflows the record buffer
        ev.update(torch.from_numpy(c["packed"]), torch.from_numpy(c["y"]))
        RM.eval_update(state, c["packed"], c["y"], z2, c["noise_var"], records=rec)
    assert np.array_equal(_bits(ev.state.numpy()), _bits(state))
    assert np.array_equal(ev.records_buffer.numpy().view(np.uint32), rec.view(np.uint32))
    assert state[RM.CURSOR] == 2 * bs * D and state[RM.DROPPED] == max(bs * D - 5, 0) and state[0] + state[1] == 2 * bs * D
    out = ev.compute()
    n = int(np.sum(~np.isnan(c["y"])))
    assert out["n"] == 2 * n and out["ignored"] == 2 * (bs * D - n) and out["dropped"] == max(bs * D - 5, 0)
    el = RM.eval_elements(c["packed"], c["y"], c["noise_var"])
    ok = el["ok"]
    assert abs(out["mse"] - el["e2"][ok].mean()) <= 1e-12 * out["mse"] and abs(out["rmse"] - math.sqrt(out["mse"])) <= 1e-15
    assert abs(out["mae"] - np.abs(el["err"][ok]).mean()) <= 1e-12 * out["mae"]
    assert abs(out["nll"] - el["nll"][ok].mean()) <= 1e-12 * abs(out["nll"])
    yv = el["y"][ok]
    if yv.size > 1 and yv.var() > 0:
        assert abs(out["r2"] - (1 - el["e2"][ok].sum() / ((yv - yv.mean()) ** 2).sum())) <= 1e-9
    assert abs(out["mean_total_var"] - (el["ep"][ok] + el["al"][ok]).mean()) <= 1e-12 * out["mean_total_var"]
    assert abs(out["calibration_error"] - np.mean((out["coverage"] - np.asarray(c["levels"])) ** 2)) <= 1e-15
    r = ev.records()
    kept = min(cap, 2 * bs * D)
    assert r["err"].shape[0] == int(np.sum(~np.isnan(rec[:kept, 3]))) and np.array_equal(r["error"], np.abs(r["err"]))
    assert np.array_equal(r["unc"], r["epistemic_var"] + r["aleatoric_var"])


def test_quantiles_and_update_outputs():
    from statistics import NormalDist
    mc, _ = _mods()
    z2 = mc.normal_quantiles_squared(RM.LEVELS[8]).numpy()
    want = np.array([NormalDist().inv_cdf((1 + lv) / 2) ** 2 for lv in RM.LEVELS[8]])
    assert np.abs(z2 - want).max() <= 1e-12 * want.max() and np.array_equal(z2, RM.z2_of(RM.LEVELS[8]))
    c = RM.eval_case(6, 3, 4, seed=2, samples=1)
    a = _evaluator(mc, c).update(torch.from_numpy(c["packed"]), torch.from_numpy(c["y"]))
    c["packed"][-2] = 0.0  # update_outputs accumulates without a KL term; the evaluation does not read it
    b = _evaluator(mc, c).update_outputs(torch.from_numpy(c["out"]), torch.from_numpy(c["y"]))
    assert torch.equal(a.state, b.state)
    with pytest.raises(ValueError):
        mc.RegressionEvaluator(1, levels=[0.5] * 9)
    with pytest.raises(ValueError):
        mc.RegressionEvaluator(2).update(torch.zeros(8, dtype=torch.float64), torch.zeros(3, 1))


def test_merge_adds_two_states():
    mc, _ = _mods()
    c1, c2 = RM.eval_case(7, 5, 4, seed=1), RM.eval_case(7, 5, 4, seed=2)
    a = _evaluator(mc, c1, capacity=10).update(torch.from_numpy(c1["packed"]), torch.from_numpy(c1["y"]))
    b = _evaluator(mc, c2).update(torch.from_numpy(c2["packed"]), torch.from_numpy(c2["y"]))
    sa, sb = a.state.clone(), b.state.clone()
    a.merge(b)
    want = sa + sb
    want[RM.CURSOR:RM.DROPPED + 1] = sa[RM.CURSOR:RM.DROPPED + 1]  # the cursor words stay local
    assert torch.equal(a.state, want)
    assert a.reduce() is a and torch.equal(a.state, want)  # no process group: a no-op
    with pytest.raises(ValueError):
        a.merge(mc.RegressionEvaluator(5, levels=(0.5,)))


def test_reset_merge_into_fresh_and_reserve():
    """reset zeroes every word (the cursor too, so records start over); merge allocates an evaluator that saw nothing and skips one
    that saw nothing; reserve grows the record buffer and keeps what it holds"""
    mc, _ = _mods()
    c = RM.eval_case(7, 5, 4, seed=1)
    pk, y = torch.from_numpy(c["packed"]), torch.from_numpy(c["y"])
    ev = _evaluator(mc, c, capacity=40).update(pk, y)
    once, rec = ev.state.clone(), ev.records_buffer.clone()
    assert ev.update(pk, y).reset() is ev and not ev.state.any()
    ev.update(pk, y)
    assert np.array_equal(_bits(ev.state), _bits(once)) and np.array_equal(_bits(ev.records_buffer[:35]), _bits(rec[:35]))
    fresh = _evaluator(mc, c)
    assert fresh.reset() is fresh and fresh.merge(_evaluator(mc, c)) is fresh and fresh.state is None
    fresh.merge(ev)
    want = once.clone()
    want[RM.CURSOR:RM.DROPPED + 1] = 0.0  # the cursor words stay local: the fresh evaluator saw no element
    assert fresh.device == ev.device and torch.equal(fresh.state, want) and fresh.compute()["n"] == once[0]
    ev.reserve(30)
    assert ev.capacity == 40  # already large enough
    held = ev.records_buffer.clone()
    ev.reserve(41)
    assert ev.capacity == 80 and np.array_equal(_bits(ev.records_buffer[:40]), _bits(held)) and not ev.records_buffer[40:].any()


def test_coverage_of_a_calibrated_predictive_lands_on_the_levels():
    """y ~ N(mean, var) on 4096 elements: the count at level p is Binomial(4096, p); 4 standard deviations"""
    mc, _ = _mods()
    n, S = 4096, 4
    r = np.random.RandomState(0)
    out = np.concatenate([r.randn(S, n, 1), r.uniform(-1, 1, (S, n, 1))], -1).astype(np.float32).reshape(S * n, 2)
    st = mc.GaussianStats("log")
    packed = st.accumulate_lanes(torch.zeros(st.numel(n, 2), dtype=torch.float64), torch.from_numpy(out), S)
    u = st.unpack(packed, n)
    y = (u["mean"].numpy() + np.sqrt(u["total_var"].numpy()) * r.randn(n, 1)).astype(np.float32)
    levels = RM.LEVELS[8]
    ev = mc.RegressionEvaluator(1, levels=levels).update(packed, torch.from_numpy(y))
    res = ev.compute()
    for lv, cov in zip(levels, res["coverage"]):
        assert abs(cov - lv) * n <= 4 * math.sqrt(n * lv * (1 - lv)), (lv, cov)
    assert res["calibration_error"] < 1e-3 and abs(res["nll"] - 0.5 * (math.log(2 * math.pi) + 1)) < 0.6


def test_evaluate_loop_on_cpu_pads_nothing_and_equals_manual_updates():
    import bayesian_torch_amd as bt
    mc, _ = _mods()
    bt.manual_seed(5)
    torch.manual_seed(0)
    net = _Net().eval()
    bt.assign_layer_ids(net)
    st = mc.GaussianStats("log")
    batches = [(torch.randn(8, 8), torch.randn(8, 1)), (torch.randn(5, 8), torch.randn(5, 1))]
    ev = mc.evaluate(net, batches, 3, stats=st, evaluator=mc.RegressionEvaluator(1))
    man = mc.RegressionEvaluator(1)
    for x, y in batches:
        man.update(mc.mc_forward(net, x, 3, stats=st, reduce=False, rank=0, world=1), y)
    assert torch.equal(ev.state, man.state) and ev.compute()["n"] == 13
    auto = mc.evaluate(net, batches, 3, stats=st)  # builds its own evaluator, which keeps the records
    assert torch.equal(auto.state[:RM.SUMS], man.state[:RM.SUMS]) and auto.records()["err"].shape[0] == 13
    with pytest.raises(ValueError):
        mc.evaluate(net, batches, 3, stats=st, evaluator=mc.Evaluator(2))
    with pytest.raises(ValueError):
        mc.evaluate(net, batches, 3, evaluator=mc.RegressionEvaluator(1))


# ---- the library's argument checks ------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_k16_entry_points_without_gpu():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9
    p = ctypes.c_void_p(64)
    E_NULL, E_SHAPE, E_UNSUP, E_WS, E_DTYPE, E_ALIGN = -1, -2, -3, -4, -5, -6
    for code, word in ((E_NULL, b"NULL"),):
        assert word in L.btx_strerror(code)
    mom = L.btx_mc_moments_lanes
    assert mom(None, 1, 2, 3, 1, 0, 0.0, p, None) == E_NULL and mom(p, 1, 2, 3, 1, 0, 0.0, None, None) == E_NULL
    assert mom(p, 0, 2, 3, 1, 0, 0.0, p, None) == E_SHAPE and mom(p, 1, 0, 3, 1, 0, 0.0, p, None) == E_SHAPE
    assert mom(p, 1, 2, 0, 1, 0, 0.0, p, None) == E_SHAPE and mom(p, 1, 2, 3, 2, 0, 0.0, p, None) == E_SHAPE
    assert mom(p, 1, 1 << 16, 1 << 15, 1, 0, 0.0, p, None) == E_UNSUP       # N = 2^31
    assert mom(p, 1, 2, 3, 1, 7, 0.0, p, None) == E_DTYPE
    assert mom(ctypes.c_void_p(66), 1, 2, 3, 1, 0, 0.0, p, None) == E_ALIGN  # an f32 tensor is never 2 bytes off
    assert mom(p, 1, 2, 3, 1, 1, 0.0, ctypes.c_void_p(68), None) == E_ALIGN
    assert L.btx_mc_gnll_workspace_bytes(3, 1366) == 8 * 2 and L.btx_mc_gnll_workspace_bytes(65, 4097) == 8 * 66
    assert L.btx_mc_gnll_workspace_bytes(0, 4) == 0
    fwd, bwd = L.btx_mc_gnll_fwd, L.btx_mc_gnll_bwd
    ok = dict(stack=p, target=p, S=2, B=3, D=4, has_var=1, act=0, reduce=1, nv=1.0, full=0, kl=None, out=p, ws=p, wsb=8)
    def f(**kw):  # noqa: E306
        a = dict(ok, **kw)
        return fwd(a["stack"], a["target"], a["S"], a["B"], a["D"], a["has_var"], a["act"], a["reduce"], a["nv"], a["full"], a["kl"],
                   a["out"], a["ws"], a["wsb"], None)
    def b(**kw):  # noqa: E306
        a = dict(dict(ok, g=p, ds=p), **kw)
        return bwd(a["stack"], a["target"], a["S"], a["B"], a["D"], a["has_var"], a["act"], a["reduce"], a["nv"], a["g"], a["ds"], None)
    for call in (f, b):
        assert call(stack=None) == E_NULL and call(target=None) == E_NULL
        assert call(S=0) == E_SHAPE and call(S=33) == E_SHAPE and call(B=0) == E_SHAPE and call(D=0) == E_SHAPE
        assert call(reduce=2) == E_SHAPE and call(has_var=0, nv=0.0) == E_SHAPE and call(has_var=0, nv=float("nan")) == E_SHAPE
        assert call(act=2) == E_DTYPE and call(B=1 << 16, D=1 << 15) == E_UNSUP
        assert call(stack=ctypes.c_void_p(66)) == E_ALIGN
    assert f(out=None) == E_NULL and f(ws=None) == E_NULL and f(full=2) == E_SHAPE and f(wsb=7) == E_WS
    assert f(ws=ctypes.c_void_p(68)) == E_ALIGN
    assert b(g=None) == E_NULL and b(ds=None) == E_NULL
    assert L.btx_reg_eval_workspace_bytes(3, 1366) == 2 * 17 * 8 and L.btx_reg_eval_workspace_bytes(0, 1) == 0
    upd = L.btx_reg_eval_update
    base = [p, p, 3, 4, 0.0, 1e-12, p, 4, p, 20, None, 0, p, 17 * 8, None]
    def u(**kw):  # noqa: E306
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return upd(*a)
    assert u(a0=None) == E_NULL and u(a1=None) == E_NULL and u(a6=None) == E_NULL and u(a8=None) == E_NULL and u(a12=None) == E_NULL
    assert u(a11=5) == E_NULL                                              # capacity without records
    assert u(a2=0) == E_SHAPE and u(a3=0) == E_SHAPE and u(a7=9) == E_SHAPE and u(a7=-1) == E_SHAPE and u(a11=-1) == E_SHAPE
    assert u(a4=-1.0) == E_SHAPE and u(a5=0.0) == E_SHAPE
    assert u(a9=19) == E_WS and u(a13=17 * 8 - 1) == E_WS
    assert u(a2=1 << 16, a3=1 << 15) == E_UNSUP
    assert u(a0=ctypes.c_void_p(68)) == E_ALIGN and u(a1=ctypes.c_void_p(66)) == E_ALIGN
