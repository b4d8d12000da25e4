"""BTX-EVAL v1 without a GPU: the numpy model (mc_eval_model.py) against what the reference's evaluation code makes of the
fixture, mc.Evaluator's CPU path against the model bit for bit, constructed exact cases, ignored rows, state handling, and a
2-rank gloo reduce."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mc_eval_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", M.GOLDEN_CASES)
def test_model_against_reference(name):
    """pred, top-1 / top-5 hits, quadrant and bin counts equal the reference-derived values exactly; H and MI within 2e-6 of the
    reference's float64 values (f32 rounding of at most 1000 terms); eval_avu of the records equals the golden AvU[21]"""
    from bayesian_torch_amd.utils import avuc_loss
    g = M.golden_case(name)
    B, C = g["B"], g["C"]
    st = M.new_state(15, 3)
    rec = M.update(st, g["packed"], g["labels"], B, C, topk=5, nbins=15, th=g["th3"])
    assert np.array_equal(rec[:, M.REC_PRED].astype(np.int64), g["pred"])
    hit = g["pred"] == g["labels"]
    assert np.array_equal(rec[:, M.REC_RANK] == 0, hit)
    assert np.array_equal(rec[:, M.REC_RANK] < 5, g["top5"])
    assert st[M.S_VALID] == B and st[M.S_IGNORED] == 0
    assert st[M.S_TOP1] == hit.sum() and st[M.S_TOP1] / B == float(g["accuracy"])
    assert st[M.S_TOPK] == g["top5"].sum()
    bins = st[M.HEADER:M.HEADER + 45].reshape(15, 3)
    assert np.array_equal(bins[:, 0], g["bin_count_hits"][:, 0]) and np.array_equal(bins[:, 2], g["bin_count_hits"][:, 1])
    assert np.array_equal(st[M.HEADER + 45:].reshape(3, 4), g["quad3"])
    dH, dMI = np.abs(rec[:, M.REC_H] - g["H"]).max(), np.abs(rec[:, M.REC_MI] - g["MI"]).max()
    print("%s: max |H - ref| %.3e, max |MI - ref| %.3e" % (name, dH, dMI))
    assert dH <= 2e-6 and dMI <= 2e-6
    target = np.where(rec[:, M.REC_RANK] == 0, rec[:, M.REC_PRED], -1)
    avu, _ = avuc_loss.eval_avu(rec[:, M.REC_PRED], target, rec[:, M.REC_H].astype(np.float64))
    assert np.abs(avu - g["eval_avu"]).max() <= 1e-12
    # the same through the public face: what compute() / records() report is what the reference's evaluate() printed
    from bayesian_torch_amd import mc
    ev = mc.Evaluator(C, thresholds=g["th3"], capacity=B).update(_t(g["packed"]), _t(g["labels"]))
    out, r = ev.compute(), ev.records()
    assert out["top1"] == float(g["accuracy"]) and out["topk"] == g["top5"].mean() and out["n"] == B
    assert np.array_equal(out["quadrants"], g["quad3"]) and np.array_equal(r["pred"], g["pred"])
    assert np.array_equal(out["avu"], (g["quad3"][:, 0] + g["quad3"][:, 3]) / B)
    avu, _ = avuc_loss.eval_avu(r["pred"], r["target"], r["entropy"].astype(np.float64))
    assert np.abs(avu - g["eval_avu"]).max() <= 1e-12


def _with_ignored(labels, C):
    y = labels.copy()
    y[1::5] = -100
    y[3::7] = C       # out of range above
    y[4::11] = -1     # out of range below
    return y


@pytest.mark.parametrize("use_mi", [False, True])
@pytest.mark.parametrize("name", M.GOLDEN_CASES)
def test_cpu_path_equals_model_bit_for_bit(name, use_mi):
    """two updates (clean labels, then labels with ignored rows) through mc.Evaluator on CPU tensors: the state vector and the
    record buffer equal the model's, bit for bit"""
    from bayesian_torch_amd import mc
    g = M.golden_case(name)
    B, C = g["B"], g["C"]
    th = g["th3"] if not use_mi else np.array([0.05, 0.2], np.float32)
    st = M.new_state(15, th.size)
    recs = np.zeros((2 * B - 3, 8), np.float32)
    ev = mc.Evaluator(C, thresholds=th, uncertainty="mi" if use_mi else "entropy", capacity=2 * B - 3)
    for y in (g["labels"], _with_ignored(g["labels"], C)):
        M.update(st, g["packed"], y, B, C, 5, 15, th, use_mi, recs)
        ev.update(_t(g["packed"]), _t(y))
    assert np.array_equal(ev.state.numpy().view(np.uint64), st.view(np.uint64))
    assert np.array_equal(ev.records_buffer.numpy().view(np.uint32), recs.view(np.uint32))
    out = ev.compute()
    assert out["n"] == st[M.S_VALID] and out["dropped"] == 3 and out["ignored"] == st[M.S_IGNORED]
    bins = st[M.HEADER:M.HEADER + 45].reshape(15, 3)
    assert out["ece"] == np.abs(bins[:, 2] - bins[:, 1]).sum() / st[M.S_VALID]
    assert out["top1"] == st[M.S_TOP1] / st[M.S_VALID] and out["nll"] == st[M.S_NLL] / st[M.S_VALID]
    assert np.array_equal(out["quadrants"], st[M.HEADER + 45:].reshape(-1, 4))
    assert (out["quadrants"].sum(1) == out["n"]).all()


@pytest.mark.parametrize("case", M.exact_cases(), ids=lambda c: c[0])
def test_constructed_exact_cases(case):
    """n = 8 and sums that are multiples of 2^-7: ties and bin edges decided exactly as BTX-EVAL v1 says"""
    from bayesian_torch_amd import mc
    name, packed, labels, bs, C, nbins, want = case
    rec = M.rows(packed, labels, bs, C)
    ev = mc.Evaluator(C, bins=nbins, capacity=bs)
    ev.update(_t(packed), _t(labels))
    got = ev.records_buffer.numpy()
    for r in (rec, got):
        assert r[:, M.REC_PRED].tolist() == want["pred"]
        assert r[:, M.REC_RANK].tolist() == want["rank"]
        if "bin" in want:
            assert M.bin_index(r[:, M.REC_CONF], nbins).tolist() == want["bin"]
    if "bin" in want:
        bins = ev.compute()["bins"]
        assert bins[:, 0].tolist() == np.bincount(want["bin"], minlength=nbins).tolist()


def test_ignored_rows_add_nothing():
    """ignore_index and every out-of-range label: the sums equal those of the valid rows alone, the records are flagged"""
    from bayesian_torch_amd import mc
    g = M.golden_case("s8_b48_c10")
    B, C = g["B"], g["C"]
    y = _with_ignored(g["labels"], C)
    bad = (y < 0) | (y >= C)
    assert 0 < bad.sum() < B
    ev = mc.Evaluator(C, thresholds=g["th3"], capacity=B)
    ev.update(_t(g["packed"]), _t(y))
    rec = ev.records_buffer.numpy()
    assert (rec[bad, M.REC_RANK] == -1).all() and (rec[~bad, M.REC_RANK] >= 0).all()
    assert not rec[bad][:, [M.REC_PY, M.REC_NLL, M.REC_BRIER]].any()
    full = M.rows(g["packed"], g["labels"], B, C)
    assert np.array_equal(rec[:, [M.REC_PRED, M.REC_CONF, M.REC_H, M.REC_MI]], full[:, [M.REC_PRED, M.REC_CONF, M.REC_H, M.REC_MI]])
    assert np.array_equal(rec[~bad], full[~bad])
    out = ev.compute()
    assert out["n"] == B - bad.sum() and out["ignored"] == bad.sum()
    s = ev.state.numpy()
    assert s[M.S_TOP1] == (full[~bad, M.REC_RANK] == 0).sum()
    assert s[M.S_NLL] == pytest.approx(full[~bad, M.REC_NLL].astype(np.float64).sum(), rel=1e-15)
    assert s[M.HEADER:M.HEADER + 45].reshape(15, 3)[:, 0].sum() == B - bad.sum()
    assert (out["quadrants"].sum(1) == B - bad.sum()).all()
    assert len(ev.records()["pred"]) == B - bad.sum()


def test_capacity_overflow_is_counted():
    from bayesian_torch_amd import mc
    g = M.golden_case("s5_b33_c2")
    ev = mc.Evaluator(2, capacity=40)
    for _ in range(3):
        ev.update(_t(g["packed"]), _t(g["labels"]))
    out = ev.compute()
    assert out["n"] == 99 and out["dropped"] == 59
    r = ev.records()
    assert len(r["pred"]) == 40 and np.array_equal(r["pred"][:33], g["pred"]) and np.array_equal(r["pred"][33:], g["pred"][:7])
    none = mc.Evaluator(2).update(_t(g["packed"]), _t(g["labels"]))
    assert none.compute()["dropped"] == 33 and len(none.records()["pred"]) == 0


def _halves(g):
    """the two halves of a case's batch as (packed, labels, bs)"""
    B, C, h = g["B"], g["C"], g["B"] // 2
    return [(M.pack_probs(g["probs"][:, a:b]), g["labels"][a:b], b - a) for a, b in ((0, h), (h, B))]


def _assert_states_agree(got, want):
    """counts exactly, sums to 1 ulp of f64 (cursor / dropped are local and not compared)"""
    sums = [M.S_NLL, M.S_BRIER, M.S_H, M.S_MI, M.S_CONF, M.S_U_CORRECT, M.S_U_INCORRECT] + list(range(M.HEADER + 1, M.HEADER + 45, 3))
    for j in range(got.size):
        if j in (M.CURSOR, M.DROPPED):
            continue
        if j in sums:
            assert abs(got[j] - want[j]) <= np.spacing(abs(want[j])), j
        else:
            assert got[j] == want[j], j


def test_merge_of_two_halves_equals_one_pass():
    from bayesian_torch_amd import mc
    g = M.golden_case("s8_b48_c10")
    one = mc.Evaluator(10, thresholds=g["th3"]).update(_t(g["packed"]), _t(g["labels"]))
    parts = [mc.Evaluator(10, thresholds=g["th3"]).update(_t(p), _t(y)) for p, y, _ in _halves(g)]
    parts[0].merge(parts[1])
    _assert_states_agree(parts[0].state.numpy(), one.state.numpy())
    assert parts[0].compute()["n"] == 48 and parts[0].state[M.CURSOR] == 24
    with pytest.raises(ValueError):
        parts[0].merge(mc.Evaluator(10, bins=10))
    with pytest.raises(ValueError):
        parts[0].update(torch.zeros(5), torch.zeros(3, dtype=torch.int64))  # not the packed vector of 3 rows


def test_update_logits_equals_accumulate_then_update():
    from bayesian_torch_amd import mc
    g = M.golden_case("s4_b7_c1000")
    lg, y = _t(g["logits"][0]), _t(g["labels"])
    a = mc.Evaluator(1000, capacity=7).update_logits(lg, y)
    packed = torch.zeros(mc.packed_numel(7, 1000))
    mc.accumulate(packed, lg)
    b = mc.Evaluator(1000, capacity=7).update(packed, y)
    assert torch.equal(a.state, b.state) and torch.equal(a.records_buffer, b.records_buffer)
    out = a.compute()
    assert out["n"] == 7 and abs(out["mean_mi"]) < 1e-6  # one sample: no mutual information
    assert out["top1"] == int((lg.argmax(1) == y).sum()) / 7


def test_argument_errors_without_gpu():
    """btx_mc_eval validates before it launches: these calls return on the host"""
    import ctypes
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_mc_eval_state_doubles(15, 3) == 16 + 45 + 12 == M.state_doubles(15, 3)
    assert L.btx_mc_eval_state_doubles(65, 0) == 0 and L.btx_mc_eval_state_doubles(15, 33) == 0
    assert L.btx_mc_eval_workspace_bytes(64) == 64 * 32
    p4, p8, p2 = ctypes.c_void_p(64 + 4), ctypes.c_void_p(64 + 8), ctypes.c_void_p(64 + 2)

    def call(packed=p4, labels=p8, bs=4, C=10, topk=5, nbins=15, th=None, T=0, mi=0, state=p8, nst=61, rec=None, cap=0, ws=p4, wsb=128):
        return L.btx_mc_eval(packed, labels, bs, C, topk, nbins, th, T, mi, state, nst, rec, cap, ws, wsb, None)
    assert call(packed=None) == -1 and call(labels=None) == -1 and call(state=None) == -1 and call(ws=None) == -1
    assert call(T=2) == -1 and call(cap=8) == -1
    assert call(bs=0) == -2 and call(C=0) == -2 and call(topk=0) == -2 and call(nbins=65) == -2 and call(T=33, th=p4) == -2
    assert call(mi=2) == -2 and call(cap=-1, rec=p4) == -2
    assert call(C=_lib.MC_EVAL_MAX_CLASSES + 1) == -3
    assert call(wsb=127) == -4 and call(nst=60) == -4
    assert call(packed=p2) == -6 and call(labels=p4) == -6 and call(state=p4) == -6 and call(ws=p2) == -6


def test_evaluate_on_cpu_equals_the_manual_loop():
    """mc.evaluate without a GPU: mc_forward + update per batch, a default evaluator that keeps every record"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    bt.manual_seed(11)
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(32, 10))
    bt.dnn_to_bnn(net, dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
                            moped_enable=False, moped_delta=0.5))
    net.eval()
    bt.assign_layer_ids(net)
    xs = [torch.randn(n, 32) for n in (8, 8, 5)]
    ys = [torch.randint(0, 10, (n,)) for n in (8, 8, 5)]
    ev = mc.evaluate(net, zip(xs, ys), 4)
    want = mc.Evaluator(10, capacity=21)
    for x, y in zip(xs, ys):
        want.update(mc.mc_forward(net, x, 4, reduce=False), y)
    assert torch.equal(ev.state, want.state)
    assert torch.equal(ev.records_buffer[:21], want.records_buffer)
    out = ev.compute()
    assert out["n"] == 21 and out["dropped"] == 0 and len(ev.records()["pred"]) == 21 and out["mean_mi"] > 0


# ---- two ranks over gloo ---------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bayesian_torch_amd import mc
    import mc_eval_model as MM
    g = MM.golden_case("s8_b48_c10")
    packed, y, _ = _halves(g)[rank]
    ev = mc.Evaluator(10, thresholds=g["th3"], capacity=24).update(_t(packed), _t(y))
    ev.reduce()
    import reg_model as RM
    c = RM.eval_case(7, 5, 4, seed=1 + rank)
    reg = mc.RegressionEvaluator(5, levels=c["levels"], capacity=40).update(torch.from_numpy(c["packed"]), torch.from_numpy(c["y"]))
    before = reg.state.clone()
    reg.reduce()
    torch.save({"state": ev.state, "pred": torch.from_numpy(ev.records()["pred"]), "reg_before": before, "reg_state": reg.state,
                "reg_err": torch.from_numpy(reg.records()["err"])}, out_path + str(rank))
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    """what the two gloo ranks of _worker saved: ONE spawn for the tests below"""
    out = str(tmp_path_factory.mktemp("gloo") / "rank")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    return [torch.load(out + str(r)) for r in (0, 1)]


def test_reduce_world2_equals_one_pass(two_ranks):
    """a validation set sharded over two ranks: after ONE all_reduce both ranks hold the state of the whole set, and each keeps
    the records of its own shard"""
    from bayesian_torch_amd import mc
    g = M.golden_case("s8_b48_c10")
    one = mc.Evaluator(10, thresholds=g["th3"]).update(_t(g["packed"]), _t(g["labels"]))
    got = two_ranks
    assert torch.equal(got[0]["state"][:M.CURSOR], got[1]["state"][:M.CURSOR])
    for r in (0, 1):
        _assert_states_agree(got[r]["state"].numpy(), one.state.numpy())
        assert got[r]["state"][M.CURSOR] == 24
        assert np.array_equal(got[r]["pred"].numpy(), g["pred"][24 * r:24 * r + 24])


def test_regression_reduce_world2_sums_the_states(two_ranks):
    """RegressionEvaluator.reduce over the same two ranks: both hold the sum of the two states (exact: a two-term float64 sum),
    each with its own cursor words and the records of its own shard"""
    import reg_model as RM
    before = [two_ranks[r]["reg_before"] for r in (0, 1)]
    for r in (0, 1):
        want = before[0] + before[1]
        want[RM.CURSOR:RM.DROPPED + 1] = before[r][RM.CURSOR:RM.DROPPED + 1]
        assert torch.equal(two_ranks[r]["reg_state"], want)
        assert want[RM.CURSOR] == 35 and want[RM.DROPPED] == 0
        y = RM.eval_case(7, 5, 4, seed=1 + r)["y"]
        assert two_ranks[r]["reg_err"].numel() == int(np.sum(~np.isnan(y)))


def test_reset_merge_into_fresh_and_reduce_without_a_group():
    """the state handling RegressionEvaluator's tests cover, for Evaluator: reset zeroes every word (the cursor too, so records
    start over), merge allocates an evaluator that saw nothing and skips one that saw nothing, reduce without a process group is a
    no-op"""
    from bayesian_torch_amd import mc
    g = M.golden_case("s5_b33_c2")
    pk, y = _t(g["packed"]), _t(g["labels"])
    ev = mc.Evaluator(2, capacity=40).update(pk, y)
    once, rec = ev.state.clone(), ev.records_buffer.clone()
    assert ev.reduce() is ev and torch.equal(ev.state, once)
    assert ev.update(pk, y).reset() is ev and not ev.state.any()
    ev.update(pk, y)
    assert torch.equal(ev.state, once) and torch.equal(ev.records_buffer[:33], rec[:33])
    fresh = mc.Evaluator(2)
    assert fresh.reset() is fresh and fresh.merge(mc.Evaluator(2)) is fresh and fresh.state is None
    fresh.merge(ev)
    want = once.clone()
    want[M.CURSOR:M.DROPPED + 1] = 0.0  # the cursor words stay local: the fresh evaluator saw no row
    assert fresh.device == ev.device and torch.equal(fresh.state, want) and fresh.compute()["n"] == once[0]
    ev.reserve(30)
    assert ev.capacity == 40  # already large enough
    held = ev.records_buffer.clone()
    ev.reserve(41)
    assert ev.capacity == 80 and torch.equal(ev.records_buffer[:40], held) and not ev.records_buffer[40:].any()
