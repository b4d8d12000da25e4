"""BTX-EVAL v1 on the GPU: csrc/btx_mceval.hip behind mc.Evaluator against the numpy model (tests/mc_eval_model.py).

Integers (pred, rank, bin / quadrant counts, top-k hits) and the values no logf touches (conf, p_y: one IEEE f32 division) are
compared exactly.  nll, brier, H, MI and the state sums are compared with a float64 recomputation from the same packed contents
inside the envelope mc_eval_model.reference64 derives (2^-24 per f32 rounding, C0_ULP for logf, one unit per reduction level).
A quadrant count depends on H only through `H <= th`, so the thresholds of the random cases are put into gaps of the H values and
the test asserts, on its own inputs, that every H is further from them than its bound."""
import numpy as np
import pytest
import torch

import mc_eval_model as M

pytestmark = pytest.mark.gpu

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout", moped_enable=False,
             moped_delta=0.5)
# every C once, every bs once; the last one is the widest row the kernel takes
SHAPES = [(1, 3), (2, 1), (5, 64), (10, 130), (63, 3), (64, 1), (65, 64), (257, 130), (1000, 3), (1031, 64), (24575, 2)]
_CASES = {}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dev is None else t.to(dev)


def _thresholds(u, bound, k=3):
    """k thresholds (f32) in the widest gaps of the sorted values u, each further than `bound` from every value"""
    v = np.sort(np.asarray(u, np.float64))
    gaps = v[1:] - v[:-1]
    j = np.argsort(gaps)[::-1][:k]
    j = np.sort(j[gaps[j] > 16 * bound])  # equal values (C = 1: every H is zero) leave no gap to stand in
    th = (0.5 * (v[j] + v[j + 1])).astype(np.float32)
    th = np.concatenate([th, np.float32(v[-1]) + np.float32(0.25) * np.arange(1, k - th.size + 1, dtype=np.float32)])
    assert np.abs(v[None, :] - th[:, None].astype(np.float64)).min() > 4 * bound, "test inputs: a value sits on a threshold"
    return th


def _random_case(C, bs):
    """S = 4 samples of softmax probabilities, packed; labels half correct, some ignored (computed once per shape)"""
    key = (C, bs)
    if key not in _CASES:
        r = np.random.default_rng(1000 * C + bs)
        lg = r.standard_normal((1, bs, C)) * 2.0 + 0.7 * r.standard_normal((4, bs, C))
        e = np.exp(lg - lg.max(-1, keepdims=True))
        probs = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        packed = M.pack_probs(probs)
        y = r.integers(0, C, bs)
        y[::2] = probs.mean(0).argmax(1)[::2]
        if bs >= 3:
            y[1::5] = -100
            y[2::9] = C
        ref = M.reference64(packed, y, bs, C)
        d = dict(packed=packed, labels=y, ref=ref, th=_thresholds(ref["H"][0], ref["H"][1].max()),
                 th_mi=_thresholds(ref["MI"][0], ref["MI"][1].max()))
        _CASES[key] = d
    return _CASES[key]


def _check_against_model(ev, packed, labels, bs, C, th, use_mi, nbins=15, topk=5, ref=None):
    """one update of a fresh evaluator `ev` (capacity bs) against the model and the float64 recomputation"""
    st = M.new_state(nbins, len(th))
    want = M.update(st, packed, labels, bs, C, topk, nbins, th, use_mi, np.zeros((bs, 8), np.float32))
    torch.cuda.synchronize()
    got = ev.records_buffer.cpu().numpy()
    s = ev.state.cpu().numpy()
    for col in (M.REC_PRED, M.REC_RANK):
        assert np.array_equal(got[:, col], want[:, col]), col
    for col in (M.REC_CONF, M.REC_PY):
        assert np.array_equal(got[:, col].view(np.uint32), want[:, col].view(np.uint32)), col
    ref = ref or M.reference64(packed, labels, bs, C)
    worst = {}
    for name, col in (("nll", M.REC_NLL), ("brier", M.REC_BRIER), ("H", M.REC_H), ("MI", M.REC_MI)):
        v, b = ref[name]
        err = np.abs(got[:, col].astype(np.float64) - v)
        worst[name] = float((err / b.clip(min=1e-300)).max())
        assert (err <= b).all(), (name, float(err.max()), float(b[err.argmax()]))
    print("C %5d bs %3d: worst error / bound %s" % (C, bs, {k: "%.3f" % v for k, v in worst.items()}))
    counts = [M.S_VALID, M.S_IGNORED, M.S_TOP1, M.S_TOPK, M.CURSOR, M.DROPPED]
    counts += list(range(M.HEADER, M.HEADER + 3 * nbins, 3)) + list(range(M.HEADER + 2, M.HEADER + 3 * nbins, 3))
    counts += list(range(M.HEADER + 3 * nbins, s.size))
    assert np.array_equal(s[counts], st[counts])
    valid = ref["valid"]
    hit = want[:, M.REC_RANK] == 0
    u = ref["MI" if use_mi else "H"]
    for j, (v, b), m in ((M.S_NLL, ref["nll"], valid), (M.S_BRIER, ref["brier"], valid), (M.S_H, ref["H"], valid),
                         (M.S_MI, ref["MI"], valid), (M.S_CONF, ref["conf"], valid), (M.S_U_CORRECT, u, hit),
                         (M.S_U_INCORRECT, u, valid & ~hit)):
        assert abs(s[j] - v[m].sum()) <= M.state_sum_bound(v[m], b[m]), j
    bins = M.bin_index(want[:, M.REC_CONF], nbins)
    for k in range(nbins):  # the bins' conf sums: exact f32 values widened, only the f64 additions round
        m = valid & (bins == k)
        v = want[m, M.REC_CONF].astype(np.float64)
        assert abs(s[M.HEADER + 3 * k + 1] - v.sum()) <= M.state_sum_bound(v, np.zeros_like(v))
    return got, s


@pytest.mark.parametrize("C,bs", SHAPES)
def test_update_against_model(C, bs):
    from bayesian_torch_amd import mc
    dev = _dev()
    c = _random_case(C, bs)
    for use_mi in (False, True):
        th = c["th_mi"] if use_mi else c["th"]
        ev = mc.Evaluator(C, thresholds=th, uncertainty="mi" if use_mi else "entropy", capacity=bs, device=dev)
        ev.update(_t(c["packed"], dev), _t(c["labels"], dev))
        assert ev.workspace is not None  # the kernel, not the torch chain
        _check_against_model(ev, c["packed"], c["labels"], bs, C, th, use_mi, ref=c["ref"])


@pytest.mark.parametrize("name", M.GOLDEN_CASES)
def test_fixture_integers_equal_the_reference(name):
    """the fixture through the kernel: pred, hits, bin and quadrant counts are those the reference's code gave"""
    from bayesian_torch_amd import mc
    dev = _dev()
    g = M.golden_case(name)
    B, C = g["B"], g["C"]
    ev = mc.Evaluator(C, thresholds=g["th3"], capacity=B, device=dev)
    ev.update(_t(g["packed"], dev), _t(g["labels"], dev))
    got, s = _check_against_model(ev, g["packed"], g["labels"], B, C, g["th3"], False)
    assert np.array_equal(got[:, M.REC_PRED].astype(np.int64), g["pred"])
    assert np.array_equal(got[:, M.REC_RANK] < 5, g["top5"])
    assert np.array_equal(s[M.HEADER + 45:].reshape(3, 4), g["quad3"])
    bins = s[M.HEADER:M.HEADER + 45].reshape(15, 3)
    assert np.array_equal(bins[:, 0], g["bin_count_hits"][:, 0]) and np.array_equal(bins[:, 2], g["bin_count_hits"][:, 1])
    out = ev.compute()
    assert out["top1"] == float(g["accuracy"]) and out["topk"] == g["top5"].mean()
    r = ev.records()
    from bayesian_torch_amd.utils import avuc_loss
    avu, _ = avuc_loss.eval_avu(r["pred"], r["target"], r["entropy"].astype(np.float64))
    assert np.abs(avu - g["eval_avu"]).max() <= 1e-12


@pytest.mark.parametrize("case", M.exact_cases(), ids=lambda c: c[0])
def test_constructed_exact_cases(case):
    from bayesian_torch_amd import mc
    dev = _dev()
    name, packed, labels, bs, C, nbins, want = case
    ev = mc.Evaluator(C, bins=nbins, capacity=bs, device=dev)
    ev.update(_t(packed, dev), _t(labels, dev))
    got, s = _check_against_model(ev, packed, labels, bs, C, (), False, nbins=nbins)
    assert got[:, M.REC_PRED].tolist() == want["pred"] and got[:, M.REC_RANK].tolist() == want["rank"]
    if "bin" in want:
        assert s[M.HEADER:M.HEADER + 3 * nbins:3].tolist() == np.bincount(want["bin"], minlength=nbins).tolist()


def test_off_grid_tensors_match_on_grid():
    """packed, records, workspace and thresholds 4 bytes off the 16-byte grid, labels and state 8 bytes off: same bits"""
    from bayesian_torch_amd import mc
    dev = _dev()
    C, bs = 1031, 64
    c = _random_case(C, bs)
    on = mc.Evaluator(C, thresholds=c["th"], capacity=bs, device=dev)
    on.update(_t(c["packed"], dev), _t(c["labels"], dev))
    off = mc.Evaluator(C, thresholds=c["th"], capacity=bs, device=dev)
    pk = torch.zeros(c["packed"].size + 1, device=dev)[1:].copy_(_t(c["packed"]))
    lb = torch.zeros(bs + 1, dtype=torch.int64, device=dev)[1:].copy_(_t(c["labels"]))
    off.records_buffer = torch.zeros(bs * 8 + 1, device=dev)[1:].view(bs, 8)
    off.workspace = torch.zeros(bs * 8 + 1, device=dev)[1:]
    off.state = torch.zeros(on.state.numel() + 1, dtype=torch.float64, device=dev)[1:]
    off.th = torch.zeros(4, device=dev)[1:].copy_(_t(c["th"]))
    for t, a in ((pk, 4), (off.records_buffer, 4), (off.workspace, 4), (off.th, 4), (lb, 8), (off.state, 8)):
        assert t.data_ptr() % 16 == a
    off.update(pk, lb)
    torch.cuda.synchronize()
    assert torch.equal(off.state.view(torch.int64), on.state.view(torch.int64))
    assert torch.equal(off.records_buffer.view(torch.int32), on.records_buffer.view(torch.int32))


def test_captured_update_equals_eager():
    """update() captured once and replayed three times, with packed, labels and the thresholds rewritten between the replays,
    equals three eager calls bit for bit (state and records: the cursor lives on the device)"""
    from bayesian_torch_amd import mc
    dev = _dev()
    C, bs = 65, 64
    base = _random_case(C, bs)
    r = np.random.default_rng(5)
    feeds = []
    for i in range(3):
        probs = r.dirichlet(np.full(C, 0.3), size=(3, bs)).astype(np.float32)
        y = r.integers(-1, C + 1, bs)
        feeds.append((M.pack_probs(probs), y, (base["th"] + np.float32(0.1 * i)).astype(np.float32)))
    eager = mc.Evaluator(C, thresholds=feeds[0][2], capacity=2 * bs + 7, device=dev)
    for pk, y, th in feeds:
        eager.set_thresholds(th)
        eager.update(_t(pk, dev), _t(y, dev))
    ev = mc.Evaluator(C, thresholds=feeds[0][2], capacity=2 * bs + 7, device=dev)
    pk_s, y_s = _t(feeds[0][0], dev), _t(feeds[0][1], dev)
    ev.update(pk_s, y_s)  # allocates the workspace outside the capture
    torch.cuda.synchronize()
    ev.reset()
    ev.records_buffer.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(pk_s, y_s)
    for pk, y, th in feeds:
        pk_s.copy_(_t(pk))
        y_s.copy_(_t(y))
        ev.set_thresholds(th)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ev.state.view(torch.int64), eager.state.view(torch.int64))
    assert torch.equal(ev.records_buffer.view(torch.int32), eager.records_buffer.view(torch.int32))
    out = ev.compute()
    assert out["n"] + out["ignored"] == 3 * bs and out["dropped"] == bs - 7


def test_evaluate_graphed_equals_the_eager_loop():
    """evaluate(graphed=True, lanes=4) on a tiny converted model, three batches of 8 with 5 real rows in the last: the state and
    the records equal the loop of mc_forward(lanes=4) + update fed the same padded batches"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    dev = _dev()
    bt.manual_seed(11)
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(32, 10))
    bt.dnn_to_bnn(net, dict(PRIOR))
    net = net.to(dev).eval()
    bt.assign_layer_ids(net)
    xs = [torch.randn(n, 32, device=dev) for n in (8, 8, 5)]
    ys = [torch.randint(0, 10, (n,), device=dev) for n in (8, 8, 5)]
    ev = mc.evaluate(net, zip(xs, ys), 4, lanes=4, graphed=True)
    want = mc.Evaluator(10, capacity=24, device=dev)
    for x, y in zip(xs, ys):
        xp = torch.zeros(8, 32, device=dev)
        xp[:x.shape[0]] = x
        yp = torch.full((8,), -100, dtype=torch.int64, device=dev)
        yp[:y.numel()] = y
        want.update(mc.mc_forward(net, xp, 4, lanes=4, reduce=False), yp)
    torch.cuda.synchronize()
    assert torch.equal(ev.state.view(torch.int64), want.state.view(torch.int64))
    assert torch.equal(ev.records_buffer[:24].view(torch.int32), want.records_buffer.view(torch.int32))
    out = ev.compute()
    assert out["n"] == 21 and out["ignored"] == 3 and out["dropped"] == 0
    assert len(ev.records()["pred"]) == 21
    assert out["mean_mi"] > 0  # four different samples


def test_refused_rows_take_the_torch_chain():
    """a row wider than the kernel's limit: the torch chain on the device, same integers and p's as the model"""
    from bayesian_torch_amd import mc, _lib
    dev = _dev()
    C, bs = _lib.MC_EVAL_MAX_CLASSES + 25, 2
    c = _random_case(C, bs)
    rc = _lib.lib().btx_mc_eval(1 << 8, 1 << 8, bs, C, 5, 15, None, 0, 0, 1 << 8, 61, None, 0, 1 << 8, 64, None)
    assert rc == _lib.E_UNSUPPORTED
    ev = mc.Evaluator(C, thresholds=c["th"], capacity=bs, device=dev)
    ev.update(_t(c["packed"], dev), _t(c["labels"], dev))
    assert ev.workspace is None  # no kernel ran
    _check_against_model(ev, c["packed"], c["labels"], bs, C, c["th"], False, ref=c["ref"])
