"""BTX-REG v1 on the GPU (csrc/btx_reg.hip): the moment statistics, the Gaussian NLL head and the regression evaluator against the numpy
model and the float64 references of tests/reg_model.py, and the plumbing (GraphedTrainStep with the head as loss_fn, mc.evaluate with
stats= / evaluator=) against the eager loops bit for bit.

Tolerances.  Sums of exactly representable terms in float64 (sum m, sum m^2, integer cases, counts) are compared EXACTLY.  sum v: C_EXP_ULP
ulp32 of every term (the model rounds exp correctly; the device's expf has the measured error).  Head: every element inside the envelope
reg_model.gnll_reference derives (module docstring there), and that envelope is asserted to be useful: at most USEFUL = 1e-4 of
|ref| + mean|ref| before a bf16 store (one rounding to bf16 is 2^-8 of the value, which no useful-bound assertion can include).
Evaluator sums: N 2^-50 sum|terms| (the order of a float64 sum of N terms), sum nll with C_LOG_ULP ulp32 of the logarithm on top."""
import math

import numpy as np
import pytest
import torch

import reg_model as RM
from envelope import check, ulp32

pytestmark = pytest.mark.gpu

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mods():
    from bayesian_torch_amd import mc
    from bayesian_torch_amd.utils import mc_loss as M
    return mc, M


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. accumulate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variance", ["log", None])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 3, 1), (4, 5, 3), (3, 2, 1025), (2, 3, 8), (2, 33, 64)])
def test_moment_statistics(shape, dtype, variance):
    """(2, 3, 8) and (2, 33, 64) take the 16-byte path (D a multiple of 8; the second with more than one workgroup), the issue's three
    shapes the element-wise one"""
    mc, _ = _mods()
    dev = _dev()
    lanes, bs, D = shape
    has_var = variance == "log"
    W = 2 * D if has_var else D
    N = bs * D
    out = torch.from_numpy((np.random.RandomState(lanes * 100 + D).randn(lanes * bs, W) * 2).astype(np.float32)).to(dtype)
    o64 = out.float().double().numpy()
    st = mc.GaussianStats(variance)
    packed = st.accumulate_lanes(torch.zeros(st.numel(bs, W), dtype=torch.float64, device=dev), out.to(dev), lanes, kl=0.75)
    got = packed.cpu().numpy()
    m = o64[:, :D].reshape(lanes, N)
    sm, sq = np.zeros(N), np.zeros(N)
    for k in range(lanes):  # numpy float64, the samples in order
        sm, sq = sm + m[k], sq + m[k] * m[k]
    assert np.array_equal(got[:N], sm) and np.array_equal(got[N:2 * N], sq)
    assert got[3 * N] == lanes * 0.75 and got[3 * N + 1] == lanes
    if has_var:
        v = np.exp(o64[:, D:].reshape(lanes, N))
        err, bnd = np.abs(got[2 * N:3 * N] - v.sum(0)), (RM.C_EXP_ULP * ulp32(v)).sum(0) + 2.0 ** -50 * v.sum(0)
        print("sum v %s %s: worst err / bound %.3g" % (shape, dtype, float((err / bnd).max())))
        assert (err <= bnd).all()
    else:
        assert not got[2 * N:3 * N].any()
    # lanes in one launch == one launch per sample, bit for bit
    seq = torch.zeros_like(packed)
    for k in range(lanes):
        st.accumulate(seq, out[k * bs:(k + 1) * bs].to(dev), kl=0.75)
    assert torch.equal(_bits(seq), _bits(packed))
    # views 4 bytes off the 16-byte grid (output and packed alike): the same bits
    es = out.element_size()
    buf = torch.zeros(out.numel() + 4 // es, dtype=dtype, device=dev)
    off = buf[4 // es:].view(lanes * bs, W)
    off.copy_(out)
    pbuf = torch.zeros(packed.numel() + 1, dtype=torch.float64, device=dev)
    assert off.data_ptr() % 16 == 4 and pbuf[1:].data_ptr() % 16 == 8
    st.accumulate_lanes(pbuf[1:], off, lanes, kl=0.75)
    assert torch.equal(_bits(pbuf[1:]), _bits(packed))
    again = st.accumulate_lanes(torch.zeros_like(packed), off, lanes, kl=0.75)
    assert torch.equal(_bits(again), _bits(packed))


def test_other_dtypes_run_the_torch_ops_on_the_device():
    mc, _ = _mods()
    dev = _dev()
    out = torch.randn(6, 4).half()
    st = mc.GaussianStats("log")
    got = st.accumulate_lanes(torch.zeros(st.numel(3, 4), dtype=torch.float64, device=dev), out.to(dev), 2)
    want = RM.accumulate_lanes(np.zeros(RM.numel(3, 2)), out.float().numpy(), 2, 2, True)
    assert np.array_equal(got.cpu().numpy()[:12], want[:12])
    assert np.abs(got.cpu().numpy()[12:18] - want[12:18]).max() <= 1e-6 * want[12:18].max()


# ---- 2. the head ------------------------------------------------------------------------------------------------------------------
def _gpu_head(M, st, y, reduce, variance="log", noise_var=None, full=False, kl=RM.KL, scale=1.0, dtype=torch.float32):
    dev = _dev()
    t = torch.from_numpy(st).to(dev).to(dtype).requires_grad_(True)
    k = torch.tensor([kl], device=dev, requires_grad=True)
    loss = M.mc_gaussian_nll(t, torch.from_numpy(y).to(dev), k, reduce, variance, noise_var, full)
    assert loss.shape == () and loss.dtype == torch.float32
    assert isinstance(loss.grad_fn, M.McGnllFn._backward_cls)  # the HIP head, not the chain
    (scale * loss).backward()
    return loss.detach(), t.grad.detach(), k.grad.detach()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("reduce", ["loss", "moments"])
@pytest.mark.parametrize("shape", RM.HEAD_SHAPES)
def test_head_inside_the_envelope(shape, reduce, bf16):
    _, M = _mods()
    S, B, D = shape
    st, y = RM.head_case(S, B, D, bf16=bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    ref = RM.gnll_reference(st, y, reduce, kl=RM.KL, store_bf16=bf16)
    # the float64 chain is the reference; reg_model's own values are the same expression (asserted here at 1e-12)
    t = torch.from_numpy(st).double().requires_grad_(True)
    l64 = M._mc_gnll_chain(t, torch.from_numpy(y).double(), RM.KL, reduce)
    l64.backward()
    g64 = t.grad.numpy()
    assert abs(ref["loss"] - float(l64.detach())) <= 1e-12 * abs(ref["loss"]) and np.abs(ref["grad"] - g64).max() <= 1e-12 * np.abs(g64).max()
    loss, grad, gk = _gpu_head(M, st, y, reduce, dtype=dt)
    assert grad.dtype == dt and grad.shape == st.shape
    e_loss = abs(float(loss) - float(l64.detach()))
    rep = check(grad.float().cpu().numpy(), g64, ref["b_grad"] + 1e-14 * np.abs(g64))
    use = float((ref["b_pre"] / (np.abs(g64) + np.abs(g64).mean())).max())
    print("gnll %s %-7s %s: loss err / bound %.3g (bound / |loss| %.2g); gradient %s; bound / (|ref| + mean|ref|) max %.2g" % (
        shape, reduce, "bf16" if bf16 else "f32", e_loss / ref["b_loss"], ref["b_loss"] / abs(ref["loss"]), rep, use))
    assert e_loss <= ref["b_loss"]
    assert rep.ok, str(rep)
    assert use <= RM.USEFUL and ref["b_loss"] <= RM.USEFUL * abs(ref["loss"])
    assert float(gk) == float(np.float32(1.0) / np.float32(B))  # the KL input's gradient is 1 / B
    # two runs are bit-equal
    loss2, grad2, _ = _gpu_head(M, st, y, reduce, dtype=dt)
    assert torch.equal(_bits(loss2.reshape(1)), _bits(loss.reshape(1))) and torch.equal(_bits(grad2), _bits(grad))


@pytest.mark.parametrize("reduce", ["loss", "moments"])
def test_head_with_a_fixed_noise_variance_and_the_full_constant(reduce):
    _, M = _mods()
    S, B, D = 4, 7, 5
    st, y = RM.head_case(S, B, D, variance=None)
    ref = RM.gnll_reference(st, y, reduce, None, RM.NOISE_VAR, True, RM.KL)
    t = torch.from_numpy(st).double().requires_grad_(True)
    l64 = M._mc_gnll_chain(t, torch.from_numpy(y).double(), RM.KL, reduce, None, RM.NOISE_VAR, True)
    l64.backward()
    loss, grad, _ = _gpu_head(M, st, y, reduce, None, RM.NOISE_VAR, True)
    rep = check(grad.cpu().numpy(), t.grad.numpy(), ref["b_grad"] + 1e-14 * np.abs(t.grad.numpy()))
    print("gnll variance=None full %s: loss err / bound %.3g; gradient %s" % (reduce, abs(float(loss) - float(l64.detach())) / ref["b_loss"], rep))
    assert abs(float(loss) - float(l64.detach())) <= ref["b_loss"] and rep.ok, str(rep)


def test_upstream_gradient_is_read_on_the_device():
    """(3 * loss).backward(): g enters the kernel as a device scalar and multiplies last, so every element is fl(3 d) of the unscaled d"""
    _, M = _mods()
    st, y = RM.head_case(4, 7, 5)
    for reduce in ("loss", "moments"):
        _, g1, k1 = _gpu_head(M, st, y, reduce)
        _, g3, k3 = _gpu_head(M, st, y, reduce, scale=3.0)
        assert float(g1.abs().max()) > 0
        assert torch.equal(g3, 3 * g1)
        assert abs(float(k3) - 3 * float(k1)) <= 2.0 ** -23 * float(k3)


def test_stacks_the_kernels_do_not_take_run_the_chain_on_the_device():
    import bayesian_torch_amd as bt
    _, M = _mods()
    dev = _dev()
    st, y = RM.head_case(33, 3, 2)
    y = torch.from_numpy(y).to(dev)
    big = torch.from_numpy(st).to(dev).requires_grad_(True)  # S = 33
    loss = M.mc_gaussian_nll(big, y, None, "moments")
    assert not isinstance(loss.grad_fn, M.McGnllFn._backward_cls) and loss.is_cuda
    want = M._mc_gnll_chain(torch.from_numpy(st).double(), y.cpu().double(), None, "moments")
    assert abs(float(loss.detach()) - float(want)) <= 1e-5 * abs(float(want))
    loss.backward()
    assert torch.isfinite(big.grad).all()
    half = torch.from_numpy(st[:4]).to(dev).half().requires_grad_(True)
    lh = M.mc_gaussian_nll(half, y)
    assert not isinstance(lh.grad_fn, M.McGnllFn._backward_cls) and lh.is_cuda
    bt.set_backend("torch")
    try:
        lt = M.mc_gaussian_nll(torch.from_numpy(st[:4]).to(dev).requires_grad_(True), y)
        assert not isinstance(lt.grad_fn, M.McGnllFn._backward_cls)
    finally:
        bt.set_backend("auto")


# ---- 3. the evaluator -----------------------------------------------------------------------------------------------------------------
def _gpu_eval(mc, c, capacity=0):
    dev = _dev()
    ev = mc.RegressionEvaluator(c["D"], levels=c["levels"], noise_var=c["noise_var"], capacity=capacity, device=dev)
    return ev.update(torch.from_numpy(c["packed"]).to(dev), torch.from_numpy(c["y"]).to(dev))


@pytest.mark.parametrize("case", [(3, 1, 4), (7, 5, 4), (3, 1366, 8), (65, 4097, 1)])
def test_evaluator_against_the_model(case):
    mc, _ = _mods()
    bs, D, K = case
    c = RM.eval_case(bs, D, K, seed=11)  # asserts the coverage margins
    N = bs * D
    ev = _gpu_eval(mc, c, capacity=N)
    state, rec = RM.new_state(K), np.zeros((N, 4), np.float32)
    z2 = RM.z2_of(c["levels"])
    assert np.array_equal(ev.z2.cpu().numpy(), z2)
    el = RM.eval_update(state, c["packed"], c["y"], z2, c["noise_var"], records=rec)
    got = ev.state.cpu().numpy()
    assert np.array_equal(got[:2], state[:2]) and np.array_equal(got[RM.HEADER:], state[RM.HEADER:])  # counts, exactly
    assert np.array_equal(got[RM.CURSOR:RM.HEADER], state[RM.CURSOR:RM.HEADER])
    rows = RM.eval_rows(el, z2)
    mag = np.abs(rows).sum(1)
    worst = 0.0
    for j in (2, 3, 5, 6, 7, 8):
        bnd = N * 2.0 ** -50 * mag[j]
        worst = max(worst, abs(got[j] - state[j]) / bnd)
        assert abs(got[j] - state[j]) <= bnd, (j, got[j], state[j])
    ok = el["ok"]
    b_nll = 0.5 * (RM.C_LOG_ULP * ulp32(np.log(RM.TWO_PI * el["var"][ok]))).sum() + N * 2.0 ** -50 * mag[4]
    print("evaluator %s: sums worst err / bound %.3g, sum nll err / bound %.3g" % (case, worst, abs(got[4] - state[4]) / b_nll))
    assert abs(got[4] - state[4]) <= b_nll
    assert np.array_equal(ev.records_buffer.cpu().numpy().view(np.uint32), rec.view(np.uint32))
    out = ev.compute()
    assert out["n"] == int(ok.sum()) and out["ignored"] == N - int(ok.sum()) and out["ignored"] > 0
    assert len(ev.records()["err"]) == out["n"]


@pytest.mark.parametrize("case", [(7, 5), (3, 1366)])
def test_evaluator_on_small_integers_is_bit_equal(case):
    mc, _ = _mods()
    c = RM.eval_case_ints(*case, seed=4)
    ev = _gpu_eval(mc, c)
    state = RM.new_state(4)
    RM.eval_update(state, c["packed"], c["y"], RM.z2_of(c["levels"]), c["noise_var"])
    got = ev.state.cpu().numpy()
    for j in (0, 1, 2, 3, 5, 6, 7, 8):
        assert got[j] == state[j], (j, got[j], state[j])
    # and in any order: numpy's own sums
    el = RM.eval_elements(c["packed"], c["y"], c["noise_var"])
    ok = el["ok"]
    assert got[2] == el["e2"][ok].sum() and got[3] == np.abs(el["err"][ok]).sum() and got[7] == el["y"][ok].sum()


def test_captured_update_equals_eager():
    """update() captured once and replayed three times with packed and targets rewritten between the replays equals three eager calls
    bit for bit (state and records: the cursor lives on the device)"""
    mc, _ = _mods()
    dev = _dev()
    bs, D, K = 7, 700, 4
    feeds = [RM.eval_case(bs, D, K, seed=20 + i) for i in range(3)]
    cap = 2 * bs * D + 9
    eager = mc.RegressionEvaluator(D, levels=RM.LEVELS[K], capacity=cap, device=dev)
    for c in feeds:
        eager.update(torch.from_numpy(c["packed"]).to(dev), torch.from_numpy(c["y"]).to(dev))
    ev = mc.RegressionEvaluator(D, levels=RM.LEVELS[K], capacity=cap, device=dev)
    pk_s, y_s = torch.from_numpy(feeds[0]["packed"]).to(dev), torch.from_numpy(feeds[0]["y"]).to(dev)
    ev.update(pk_s, y_s)  # allocates the workspace outside the capture
    torch.cuda.synchronize()
    ev.reset()
    ev.records_buffer.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(pk_s, y_s)
    for c in feeds:
        pk_s.copy_(torch.from_numpy(c["packed"]))
        y_s.copy_(torch.from_numpy(c["y"]))
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(ev.state), _bits(eager.state))
    assert torch.equal(_bits(ev.records_buffer), _bits(eager.records_buffer))
    out = ev.compute()
    assert out["n"] + out["ignored"] == 3 * bs * D and out["dropped"] == bs * D - 9


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _mlp(train):
    import bayesian_torch_amd as bt
    dev = _dev()
    bt.manual_seed(9)
    bt.set_precision("f32")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2))
    bt.dnn_to_bnn(net, dict(PRIOR, type="Reparameterization"))
    net = net.to(dev)
    net = net.train() if train else net.eval()
    bt.assign_layer_ids(net)
    return net


def test_captured_training_step_equals_the_eager_loop():
    """GraphedTrainStep(num_mc=2, loss_fn=mc_gaussian_nll, optimizer=Adam), three replays, against eager mc_train_forward + head + the
    same optimizer at the same indices: loss, parameters and optimizer state bit for bit"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import optim
    from bayesian_torch_amd.autograd import GraphedTrainStep, mc_train_forward
    _, M = _mods()
    dev = _dev()
    net = _mlp(True)
    torch.manual_seed(1)
    x, y = torch.randn(8, 8, device=dev), torch.randn(8, 1, device=dev)
    params = list(net.parameters())
    start = [p.detach().clone() for p in params]
    head = lambda out, tgt: M.mc_gaussian_nll(out, tgt, kl=bt.get_kl_loss(net))  # noqa: E731
    opt_e = optim.Adam(params, lr=1e-2)
    losses = []
    for s in (0, 1, 2):
        for p in params:
            p.grad = None
        loss = head(mc_train_forward(net, x, 2, s), y)
        assert isinstance(loss.grad_fn, M.McGnllFn._backward_cls)
        loss.backward()
        losses.append(loss.detach().clone())
        opt_e.step()
    eager = [p.detach().clone() for p in params]
    state_e = [{k: v.detach().clone() for k, v in opt_e.state[p].items() if torch.is_tensor(v)} for p in params]
    del loss
    with torch.no_grad():
        for p, s0 in zip(params, start):
            p.copy_(s0)
            p.grad = None
    opt = optim.Adam(params, lr=1e-2)
    gs = GraphedTrainStep(net, x, y, loss_fn=head, optimizer=opt, num_mc=2)
    try:
        with torch.no_grad():
            for p, s0 in zip(params, start):
                p.copy_(s0)
        for s in (0, 1, 2):
            got = gs.run(s).clone()
            assert torch.equal(_bits(got.reshape(1)), _bits(losses[s].reshape(1))), (s, float(got), float(losses[s]))
        torch.cuda.synchronize()
        for p, e, se in zip(params, eager, state_e):
            assert torch.equal(_bits(p.detach()), _bits(e))
            for k, v in se.items():
                if v.dtype == torch.float32:
                    assert torch.equal(_bits(opt.state[p][k]), _bits(v)), k
    finally:
        gs.close()
    assert math.isfinite(float(losses[-1])) and float(losses[-1]) != float(losses[0])


def test_evaluate_graphed_equals_the_eager_loop():
    """evaluate(stats=, evaluator=, graphed=True, lanes=4), three batches of 8 with 5 real rows in the last: state and records equal the
    loop of mc_forward(lanes=4, stats=) + update on the same padded batches; stats=None is today's path"""
    mc, _ = _mods()
    dev = _dev()
    net = _mlp(False)
    torch.manual_seed(3)
    xs = [torch.randn(n, 8, device=dev) for n in (8, 8, 5)]
    ys = [torch.randn(n, 1, device=dev) for n in (8, 8, 5)]
    st = mc.GaussianStats("log")
    ev = mc.evaluate(net, zip(xs, ys), 4, lanes=4, graphed=True, stats=st, evaluator=mc.RegressionEvaluator(1, capacity=24))
    want = mc.RegressionEvaluator(1, capacity=24, device=dev)
    for x, y in zip(xs, ys):
        xp = torch.zeros(8, 8, device=dev)
        xp[:x.shape[0]] = x
        yp = torch.full((8, 1), float("nan"), device=dev)
        yp[:y.shape[0]] = y
        want.update(mc.mc_forward(net, xp, 4, lanes=4, reduce=False, stats=st), yp)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ev.state), _bits(want.state))
    assert torch.equal(_bits(ev.records_buffer), _bits(want.records_buffer))
    out = ev.compute()
    assert out["n"] == 21 and out["ignored"] == 3 and out["dropped"] == 0 and out["mean_epistemic_var"] > 0
    r = ev.records()
    assert len(r["err"]) == 21 and np.array_equal(r["unc"], r["epistemic_var"] + r["aleatoric_var"])
    # the one-sample graph and the eager single-sample loop give the same packed vector as well
    g = mc.GraphedMC(net, xs[0].clone(), stats=st)
    try:
        for s in range(3):
            g.run(s)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g.packed), _bits(mc.mc_forward(net, xs[0], 3, reduce=False, stats=st)))
    finally:
        g.close()
    # stats=None: the softmax layout through the same drivers
    a = mc.mc_forward(net, xs[0], 4, lanes=4, reduce=False)
    b = mc.mc_forward(net, xs[0], 4, lanes=4, reduce=False, stats=None)
    assert a.dtype == torch.float32 and a.numel() == mc.packed_numel(8, 2) and torch.equal(_bits(a), _bits(b))
