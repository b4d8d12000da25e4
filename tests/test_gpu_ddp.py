"""GPU: the gradient bucket (csrc/btx_bucket.hip, K14) and data-parallel GraphedTrainStep(group=).

(7) btx_bucket_pack / btx_bucket_unpack against numpy float32, bit for bit: one f32 multiply per element, nothing else written.
(8) a 1-rank RCCL group: the scale is 1 and the sum over one rank is the identity, so four replays with `group=` leave parameters,
    buffers and optimizer state bit-equal to four replays without it.  (Both sides are replays of captured graphs of the same launches
    on the same tensors' values; the small model's gradient kernels have a fixed summation order at these shapes, which the test
    asserts first by running the ungrouped side twice.)
(9) two ranks on two GPUs (skipped with fewer): bit-equal parameters on both, equal to one GPU playing both ranks."""
import os
import socket
import subprocess
import sys
import time
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ddp_worker import ADAM, LOCAL_BS, build_small, shard  # noqa: E402

SENTINEL = np.float32(-7.25)
SIZES = (1, 3, 10, 4095, 4096, 4097)
GUARD = 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- (7) the two launches ------------------------------------------------------------------------------------------------------------
def _layout(count):
    """`count` non-empty items of the SIZES in turn and one empty item; (n, source offset, bucket offset) in floats.  Sources sit back
    to back in one flat buffer at offsets rounded up to 4 floats, except item 2 (n = 10) and item 5 (n = 4097), which start one float
    later: 4-byte but not 16-byte aligned.  Bucket offsets are rounded up to 4 floats, except item 7's (+2: the bucket side off the
    16-byte grid)."""
    items, so, bo = [], 0, 0
    for i in range(count):
        n = SIZES[i % len(SIZES)]
        so = (so + 3) & ~3
        bo = (bo + 3) & ~3
        if i in (2, 5):
            so += 1
        if i == 7:
            bo += 2
        items.append((n, so, bo))
        so += n
        bo += n
        if i == 3:
            items.append((0, so, bo))  # the empty item
    return items, so, bo


def _table(items, base_ptr):
    from bayesian_torch_amd import _lib
    t = (_lib.BucketItem * len(items))()
    for it, (n, so, bo) in zip(t, items):
        it.src, it.offset, it.n = base_ptr + 4 * so, bo, n
    return t


@pytest.mark.parametrize("count", [48, 49], ids=["48-items", "49-items"])
@pytest.mark.parametrize("scale", [1.0, 0.5, float(np.float32(1.0 / 3.0))], ids=["1", "0.5", "third"])
def test_pack_and_unpack_equal_numpy_bit_for_bit(count, scale):
    from bayesian_torch_amd import _lib
    L, dev = _lib.lib(), _dev()
    items, src_len, bkt_len = _layout(count)
    assert sum(1 for n, _, _ in items if n) == count and any(n == 0 for n, _, _ in items)
    rs = np.random.RandomState(count)
    src = (rs.randn(src_len) * 10.0 ** rs.uniform(-3, 3, src_len)).astype(np.float32)
    src_d = torch.from_numpy(src).to(dev)
    assert src_d.data_ptr() % 16 == 0
    bkt_d = torch.full((GUARD + bkt_len + GUARD,), float(SENTINEL), dtype=torch.float32, device=dev)
    bucket_ptr = bkt_d.data_ptr() + 4 * GUARD
    assert bucket_ptr % 16 == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.btx_bucket_pack(_table(items, src_d.data_ptr()), len(items), scale, bucket_ptr, stream))
    torch.cuda.synchronize()
    want = np.full(GUARD + bkt_len + GUARD, SENTINEL, dtype=np.float32)
    for n, so, bo in items:
        want[GUARD + bo:GUARD + bo + n] = src[so:so + n] * np.float32(scale)
    got = bkt_d.cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])   # the items, the pad words and the guard words
    # unpack into a fresh flat buffer with the same carving: the items' ranges are the bucket's slices, nothing else is written
    dst_d = torch.full((src_len + GUARD,), float(SENTINEL), dtype=torch.float32, device=dev)
    _lib.check(L.btx_bucket_unpack(_table(items, dst_d.data_ptr()), len(items), bucket_ptr, stream))
    torch.cuda.synchronize()
    want_dst = np.full(src_len + GUARD, SENTINEL, dtype=np.float32)
    for n, so, bo in items:
        want_dst[so:so + n] = want[GUARD + bo:GUARD + bo + n]
    got_dst = dst_d.cpu().numpy()
    bad = np.flatnonzero(got_dst.view(np.uint32) != want_dst.view(np.uint32))
    assert bad.size == 0, (bad[:8], got_dst[bad[:8]], want_dst[bad[:8]])
    assert np.array_equal(bkt_d.cpu().numpy().view(np.uint32), want.view(np.uint32))  # unpack only reads the bucket


# ---- (8) a 1-rank RCCL group ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_group():
    import torch.distributed as dist
    dev = _dev()
    torch.cuda.set_device(dev)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        yield dist.group.WORLD
    finally:
        import bayesian_torch_amd as bt
        bt.set_precision("f32")
        dist.destroy_process_group()


def _optimizer(name, net):
    from bayesian_torch_amd import optim
    if name == "Adam":
        return optim.Adam(net.parameters(), max_grad_norm=1.0, **ADAM)
    return optim.SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-3)


def _snapshot(net, opt):
    out = [p.detach().clone() for p in net.parameters()]
    out += [b.detach().clone() for n, b in net.named_buffers() if "running_" in n or "num_batches_tracked" in n]
    if opt is not None:
        for p in net.parameters():
            for k in sorted(opt.state.get(p, {})):
                v = opt.state[p][k]
                out.append(v.detach().clone().to(p.device) if torch.is_tensor(v) else torch.tensor(float(v), device=p.device))
    return out


def _four_replays(bn, opt_name, num_mc, group):
    """four replays from the same start; returns (parameters + BatchNorm statistics + optimizer state, losses, collectives seen)"""
    import torch.distributed as dist
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = _dev()
    net = build_small(dev, bn=bn)
    x, y = shard(0, 1, dev)
    opt = _optimizer(opt_name, net)
    kw = {} if group is None else dict(group=group)
    calls, orig = [], dist.all_reduce

    def spy(t, *a, **k):
        calls.append((t.device.type, t.dtype, t.numel()))
        return orig(t, *a, **k)
    gs = GraphedTrainStep(net, x, y, optimizer=opt, num_mc=num_mc, **kw)
    dist.all_reduce = spy
    try:
        losses = []
        for s in range(4):
            losses.append(gs.run(s).detach().clone().reshape(()))
            assert len(calls) == (0 if group is None else s + 1)
        torch.cuda.synchronize()
        if group is not None:
            assert calls == [("cuda", torch.float32, gs.reducer.bucket.numel())] * 4, calls
            assert gs.global_batch == LOCAL_BS
    finally:
        dist.all_reduce = orig
        gs.close()
    return _snapshot(net, opt), losses


@pytest.mark.parametrize("bn,opt_name,num_mc", [(False, "Adam", 1), (False, "SGD", 1), (True, "Adam", 1), (True, "SGD", 1),
                                                (False, "Adam", 2), (True, "SGD", 2)],
                         ids=["plain-Adam", "plain-SGD", "bn-Adam", "bn-SGD", "plain-Adam-mc2", "bn-SGD-mc2"])
def test_one_rank_group_equals_the_ungrouped_step_bit_for_bit(one_rank_group, bn, opt_name, num_mc):
    ref, ref_losses = _four_replays(bn, opt_name, num_mc, None)
    again, _ = _four_replays(bn, opt_name, num_mc, None)
    assert all(torch.equal(a, b) for a, b in zip(ref, again))  # the ungrouped step repeats itself bit for bit at this shape
    start = [p.detach() for p in build_small(_dev(), bn=bn).parameters()]
    assert not any(torch.equal(a, b) for a, b in zip(ref, start))  # the four steps moved every parameter
    got, got_losses = _four_replays(bn, opt_name, num_mc, one_rank_group)
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), (i, float((a.double() - b.double()).abs().max()))
    assert all(torch.equal(a, b) for a, b in zip(got_losses, ref_losses))


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn"])
def test_one_rank_group_without_optimizer_unpacks_into_p_grad(one_rank_group, bn):
    """optimizer=None: run() leaves the reduced gradient in p.grad, a torch.optim.SGD step follows; gradients and parameters of four
    such steps equal the ungrouped run's"""
    import torch.distributed as dist
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = _dev()
    runs = []
    for group in (None, one_rank_group):
        net = build_small(dev, bn=bn)
        x, y = shard(0, 1, dev)
        opt = torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9)
        gs = GraphedTrainStep(net, x, y, **({} if group is None else dict(group=group)))
        calls, orig = [], dist.all_reduce

        def spy(t, *a, **k):
            calls.append(t.numel())
            return orig(t, *a, **k)
        dist.all_reduce = spy
        try:
            grads = []
            for s in range(4):
                gs.run(s)
                grads.append([p.grad.detach().clone() for p in net.parameters()])
                opt.step()
            torch.cuda.synchronize()
        finally:
            dist.all_reduce = orig
            gs.close()
        assert calls == ([] if group is None else [gs.reducer.bucket.numel()] * 4)
        runs.append((grads, [p.detach().clone() for p in net.parameters()]))
    (g0, p0), (g1, p1) = runs
    for s in range(4):
        assert all(torch.equal(a, b) for a, b in zip(g0[s], g1[s])), s
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))


# ---- (9) two ranks ---------------------------------------------------------------------------------------------------------------------
def _play_both_ranks(steps, check=None):
    """one GPU plays both ranks of a 2-rank run: graph A of each replica, the two buckets added with torch.add (two addends commute:
    what the RCCL sum gives), graph B of each.  Returns the two models and the mean losses."""
    from bayesian_torch_amd import optim, parallel
    from bayesian_torch_amd.autograd import GraphedTrainStep
    dev = _dev()
    nets = [build_small(dev) for _ in (0, 1)]
    reds = [parallel.GradReducer(n, rank=r, world=2) for r, n in enumerate(nets)]
    gss = []
    for r in (0, 1):
        x, y = shard(r, 2, dev)
        gss.append(GraphedTrainStep(nets[r], x, y, optimizer=optim.Adam(nets[r].parameters(), max_grad_norm=1.0, **ADAM),
                                    group=reds[r]))
        assert gss[r].global_batch == 2 * LOCAL_BS and gss[r].reducer is reds[r]
    try:
        losses = []
        for s in range(steps):
            for gs in gss:
                gs.forward_backward(s)
            total = torch.add(reds[0].bucket, reds[1].bucket)
            for r in (0, 1):
                reds[r].bucket.copy_(total)
            if check is not None:
                check(s, nets, reds, gss)
            for r in (0, 1):
                loss = gss[r].apply()
            losses.append(float(loss))
        torch.cuda.synchronize()
    finally:
        for gs in gss:
            gs.close()
    return nets, losses


def test_one_gpu_playing_two_ranks_reduces_to_the_mean_and_keeps_the_replicas_equal():
    """world = 2 through rank= / world=: the bucket slices hold f32(g0 * 0.5) + f32(g1 * 0.5) of the two replicas' LOCAL gradients
    (which p.grad keeps), the loss word the mean of the two losses, the sample words (step * 2 + rank), and after three captured Adam
    steps the replicas are bit-equal"""
    def check(s, nets, reds, gss):
        half = torch.tensor(0.5, device=_dev())
        for p0, p1 in zip(nets[0].parameters(), nets[1].parameters()):
            want = p0.grad * half + p1.grad * half
            assert not torch.equal(p0.grad, p1.grad)
            assert torch.equal(reds[0].grad_view(p0), want) and torch.equal(reds[1].grad_view(p1), want)
        assert torch.equal(reds[0].loss, gss[0].loss * half + gss[1].loss * half)
        assert [int(g.sample_dev[0]) for g in gss] == [2 * s, 2 * s + 1]
    nets, losses = _play_both_ranks(3, check)
    start = build_small(_dev())
    for a, b, c in zip(nets[0].parameters(), nets[1].parameters(), start.parameters()):
        assert torch.equal(a.detach(), b.detach()) and not torch.equal(a.detach(), c.detach())
    assert all(np.isfinite(losses))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_ranks_on_two_gpus_equal_one_gpu_playing_both(tmp_path):
    steps, port = 3, str(_free_port())
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    outs = [str(tmp_path / ("rank%d.pt" % r)) for r in (0, 1)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ddp_worker.py"), str(r), "2", port, outs[r], str(steps)],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in (0, 1)]
    deadline = time.monotonic() + 240  # ONE limit for both ranks
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=max(1.0, deadline - time.monotonic()))[0])
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        for p in procs:
            p.wait()
        pytest.fail("the two ranks did not finish inside their shared time limit")
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    ranks = [torch.load(o, weights_only=False) for o in outs]
    for a, b in zip(ranks[0]["params"], ranks[1]["params"]):
        assert torch.equal(a, b)
    assert ranks[0]["losses"] == ranks[1]["losses"]  # both hold the mean loss
    nets, losses = _play_both_ranks(steps)
    for i, (a, b) in enumerate(zip(ranks[0]["params"], nets[0].parameters())):
        assert torch.equal(a, b.detach().cpu()), (i, float((a - b.detach().cpu()).abs().max()))
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(nets[0].parameters(), nets[1].parameters()))
    assert losses == ranks[0]["losses"]
