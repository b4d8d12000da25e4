"""Data-parallel training on the CPU: parallel.GradReducer over a world_size-2 gloo group (mp.spawn as in tests/test_mc_gloo.py).

The two ranks run ONCE per layer type (module fixture `world2`) and leave what they computed in files; the tests compare those with
single-process runs, bit for bit.  Everything runs with one intra-op thread, so that a rank and the process that plays it add in
the same order.  The model is conv(3->8, 3x3) - ReLU - conv(8->8, stride 2) - ReLU - Flatten - Linear(72->5) on 8x8 inputs, 4 images
per rank; the ATen route draws its noise from torch's CPU generator, keyed on the sample index as autograd.mc_train_forward does."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, moped_enable=False, moped_delta=0.5)
TYPES = ("Flipout", "Reparameterization")
STEP = 3          # the step number of the single reduce()
LOCAL_BS = 4
SGD = dict(lr=0.1, momentum=0.9)


def _model(typ):
    import bayesian_torch_amd as bt
    bt.manual_seed(2024)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 8, 3, stride=2),
                              torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(8 * 3 * 3, 5))
    bt.dnn_to_bnn(net, dict(PRIOR, type=typ))
    net.train()
    bt.assign_layer_ids(net)
    return net


def _shard(rank):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2 * LOCAL_BS, 3, 8, 8, generator=g)
    y = torch.randint(0, 5, (2 * LOCAL_BS,), generator=g)
    return x[rank * LOCAL_BS:(rank + 1) * LOCAL_BS], y[rank * LOCAL_BS:(rank + 1) * LOCAL_BS]


def _backward(model, x, y, idx, B, kl_only=False):
    """one training forward + backward with sample index idx (CPU generator keyed on it); returns the detached loss"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import rng
    for p in model.parameters():
        p.grad = None
    if kl_only:
        loss = bt.get_kl_loss(model) / B
    else:
        bt.set_sample_index(model, idx)
        with torch.random.fork_rng(devices=[]):
            torch.default_generator.manual_seed(rng.cpu_sample_seed(idx))
            out = model(x)
        out = out[0] if isinstance(out, tuple) else out
        loss = torch.nn.functional.cross_entropy(out, y) + bt.get_kl_loss(model) / B
    loss.backward()
    return loss.detach().clone()


def _grads(model):
    return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]


def _same(a, b):
    """bit-equal (the non-persistent eps_* buffers of the layers may hold anything, NaN included)"""
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.detach().contiguous().view(torch.uint8), b.detach().contiguous().view(torch.uint8))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bayesian_torch_amd import parallel
    res = {}
    for typ in TYPES:
        r = res[typ] = {}
        x, y = _shard(rank)
        # (3) rank 1 starts somewhere else: construction brings rank 0's parameters and buffers
        model = _model(typ)
        tensors = list(model.parameters()) + list(model.buffers())
        if rank == 1:
            with torch.no_grad():
                for t in tensors:
                    t.copy_(torch.randn(t.shape) + 1.0 if t.is_floating_point() else torch.full_like(t, 3))
        versions = [t._version for t in tensors]
        red = parallel.GradReducer(model)
        r["after_broadcast"] = [t.detach().clone() for t in tensors]
        r["version_advanced"] = all(t._version > v for t, v in zip(tensors, versions))
        bufs = list(model.buffers())
        if rank == 1:   # ... and its buffers drift afterwards (as BatchNorm statistics do): sync_buffers() brings rank 0's again
            with torch.no_grad():
                for t in bufs:
                    t.copy_(torch.randn(t.shape) + 2.0 if t.is_floating_point() else torch.full_like(t, 5))
        red.sync_buffers()
        r["after_sync"] = [t.detach().clone() for t in bufs]
        r["rank_world"] = (red.rank, red.world, red.global_batch(LOCAL_BS), red.sample_index(STEP), red.sample_index(STEP, 1, 2))
        # (1) + (5) one reduce(), the collective counted
        calls, orig = [], dist.all_reduce

        def spy(t, *a, **k):
            calls.append((t.dtype, t.numel()))
            return orig(t, *a, **k)
        local = _backward(model, x, y, red.sample_index(STEP), red.global_batch(LOCAL_BS))
        r["local_grads"], r["local_loss"] = _grads(model), local
        dist.all_reduce = spy
        try:
            mean = red.reduce(local)
        finally:
            dist.all_reduce = orig
        r["calls"], r["bucket_numel"] = calls, red.bucket.numel()
        r["grads"], r["loss"] = _grads(model), mean.clone()
        r["views_equal"] = all(torch.equal(red.grad_view(p), p.grad) for p in model.parameters())
        # (2) the KL alone
        _backward(model, x, y, 0, red.global_batch(LOCAL_BS), kl_only=True)
        red.reduce()
        r["kl_grads"] = _grads(model)
        # (4) three SGD steps
        model = _model(typ)
        red = parallel.GradReducer(model)
        opt = torch.optim.SGD(model.parameters(), **SGD)
        for step in range(3):
            loss = _backward(model, x, y, red.sample_index(step), red.global_batch(LOCAL_BS))
            red.reduce(loss)
            opt.step()
        r["trained"] = [p.detach().clone() for p in model.parameters()]
    torch.save(res, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ddp"))
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    return [torch.load(os.path.join(out, "rank%d.pt" % r), weights_only=False) for r in (0, 1)]


@pytest.fixture()
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("typ", TYPES)
def test_one_reduce_gives_the_mean_of_the_two_ranks_gradients(world2, one_thread, typ):
    """(1) every p.grad on both ranks == f32(g0 * 0.5) + f32(g1 * 0.5), g_r computed HERE on shard r with sample index STEP * 2 + r;
    the returned loss is the mean of the two losses"""
    half = torch.tensor(0.5)
    g, losses = [], []
    for r in (0, 1):
        model = _model(typ)
        x, y = _shard(r)
        losses.append(_backward(model, x, y, STEP * 2 + r, 2 * LOCAL_BS))
        g.append(_grads(model))
        assert world2[r][typ]["rank_world"] == (r, 2, 2 * LOCAL_BS, STEP * 2 + r, (STEP * 2 + r) * 2 + 1)
        # the rank computed the same local gradient as this process does
        assert all(torch.equal(a, b) for a, b in zip(world2[r][typ]["local_grads"], g[r]))
    assert not any(torch.equal(a, b) for a, b in zip(g[0], g[1]))  # different shards, different noise
    want = [a * half + b * half for a, b in zip(g[0], g[1])]
    for r in (0, 1):
        got = world2[r][typ]["grads"]
        assert len(got) == len(want) and all(w is not None for w in got)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (typ, r, i, float((a - b).abs().max()))
        assert torch.equal(world2[r][typ]["loss"], losses[0] * half + losses[1] * half)
        assert world2[r][typ]["views_equal"]


@pytest.mark.parametrize("typ", TYPES)
def test_kl_over_the_global_batch_gives_the_single_process_gradient(world2, one_thread, typ):
    """(2) loss = KL / B_global alone (RNG-free): the reduced gradient, rho_* included, is the single-process one on the global batch"""
    model = _model(typ)
    _backward(model, None, None, 0, 2 * LOCAL_BS, kl_only=True)
    names = [n for n, _ in model.named_parameters()]
    want = _grads(model)
    assert any("rho" in n and w is not None and w.abs().max() > 0 for n, w in zip(names, want))
    for r in (0, 1):
        for n, a, b in zip(names, world2[r][typ]["kl_grads"], want):
            assert (a is None and b is None) or torch.equal(a, b), (typ, r, n)


@pytest.mark.parametrize("typ", TYPES)
def test_construction_broadcasts_rank_0_and_bumps_versions(world2, typ):
    """(3) rank 1 started from other parameters and buffers; sync_buffers() repeats the broadcast for the buffers"""
    model = _model(typ)
    fresh = list(model.parameters()) + list(model.buffers())
    a0, a1 = world2[0][typ]["after_broadcast"], world2[1][typ]["after_broadcast"]
    assert len(a0) == len(a1) == len(fresh) and len(list(model.buffers())) > 0
    for f, u, v in zip(fresh, a0, a1):
        assert _same(u, v)
    for p, u in zip(model.parameters(), a0):  # rank 0 kept what it had
        assert _same(p, u)
    assert world2[0][typ]["version_advanced"] and world2[1][typ]["version_advanced"]
    n_par = len(list(model.parameters()))
    for u, v, w in zip(a0[n_par:], world2[0][typ]["after_sync"], world2[1][typ]["after_sync"]):
        assert _same(u, v) and _same(u, w)


@pytest.mark.parametrize("typ", TYPES)
def test_three_sgd_steps_equal_one_process_playing_both_ranks(world2, one_thread, typ):
    """(4) bit-equal parameters on both ranks, equal to pack() on two reducers with rank= / world=, a manual sum of the two buckets
    and unpack()"""
    from bayesian_torch_amd import parallel
    models = [_model(typ), _model(typ)]
    reds = [parallel.GradReducer(m, rank=r, world=2) for r, m in enumerate(models)]
    opts = [torch.optim.SGD(m.parameters(), **SGD) for m in models]
    for step in range(3):
        for r in (0, 1):
            x, y = _shard(r)
            loss = _backward(models[r], x, y, reds[r].sample_index(step), reds[r].global_batch(LOCAL_BS))
            reds[r].pack(loss)
            reds[r].all_reduce()  # world= is not the group's size (there is no group here): no collective
        total = reds[0].bucket + reds[1].bucket
        for r in (0, 1):
            reds[r].bucket.copy_(total)
            reds[r].unpack()
            opts[r].step()
    want = [p.detach() for p in models[0].parameters()]
    start = [p.detach() for p in _model(typ).parameters()]
    assert not any(torch.equal(a, b) for a, b in zip(want, start))
    for r in (0, 1):
        got = world2[r][typ]["trained"]
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (typ, r, i, float((a - b).abs().max()))
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(models[0].parameters(), models[1].parameters()))


@pytest.mark.parametrize("typ", TYPES)
def test_exactly_one_all_reduce_per_reduce(world2, typ):
    """(5) one collective, of the whole bucket: every parameter at an offset rounded up to 4 floats, plus the loss word"""
    model = _model(typ)
    n = 0
    for p in model.parameters():
        n = (n + p.numel() + 3) & ~3
    for r in (0, 1):
        assert world2[r][typ]["bucket_numel"] == n + 1
        assert world2[r][typ]["calls"] == [(torch.float32, n + 1)]


def test_strided_gradients_and_views_of_one_flat_buffer():
    """a gradient whose strides differ from its parameter's is staged; parameters that are views of one flat buffer keep their place;
    a world size that is no power of two scales by f32(1 / world)"""
    from bayesian_torch_amd import parallel
    flat = torch.arange(30, dtype=torch.float32)
    lin = torch.nn.Linear(2, 2)
    del lin.weight, lin.bias
    lin.weight = torch.nn.Parameter(flat[3:27].view(4, 6).t())       # column-major, at a 12-byte offset
    lin.bias = torch.nn.Parameter(flat[27:30])
    red = parallel.GradReducer(lin, rank=2, world=3)
    gw = torch.randn(6, 4)
    lin.weight.grad = gw.clone()                                     # row-major: other strides than the parameter's
    lin.bias.grad = torch.randn(3)
    gb = lin.bias.grad.clone()
    red.pack(torch.tensor(1.5))
    third = np.float32(1.0 / 3.0)
    assert red.bucket.numel() == 24 + 4 + 1 and red.sample_index(5, 1, 2) == (5 * 3 + 2) * 2 + 1
    assert np.array_equal(red.grad_view(lin.weight).numpy(), gw.numpy() * third)
    assert red.grad_view(lin.weight).stride() == lin.weight.stride()
    assert np.array_equal(red.bucket[24:27].numpy(), gb.numpy() * third) and float(red.bucket[27]) == 0.0
    assert np.array_equal(red.loss.numpy(), np.float32(1.5) * third)
    red.bucket.mul_(2.0)
    red.unpack()
    assert np.array_equal(lin.weight.grad.numpy(), gw.numpy() * third * np.float32(2))
    assert lin.weight.grad.stride() == (4, 1)


def test_bucket_argument_errors_without_gpu():
    """(6) the C-ABI argument errors of btx_bucket_pack / btx_bucket_unpack, all returned before anything is launched"""
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    buf, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)

    def item(src, offset, n):
        it = (_lib.BucketItem * 1)()
        it[0].src, it[0].offset, it[0].n = src, offset, n
        return it
    calls = (lambda items, n, bucket: L.btx_bucket_pack(items, n, 1.0, bucket, None),
             lambda items, n, bucket: L.btx_bucket_unpack(items, n, bucket, None))
    for call in calls:
        assert call(item(4096, 0, 4), 1, None) == -1                       # BTX_E_NULL: bucket
        assert call(None, 1, buf) == -1                                    # items
        assert call(item(None, 0, 4), 1, buf) == -1                        # src of a non-empty item
        assert call(item(4096, 0, 4), -1, buf) == -2                       # BTX_E_SHAPE: n_items < 0
        assert call(item(4096, 0, -4), 1, buf) == -2                       # n < 0
        assert call(item(4096, -4, 4), 1, buf) == -2                       # offset < 0
        assert call(item(4096, 0, 4), _lib.OPTIM_MAX_ITEMS + 1, buf) == -3  # BTX_E_UNSUPPORTED
        assert call(item(4098, 0, 4), 1, buf) == -6                        # BTX_E_ALIGN: not 4-byte aligned
        assert call(item(4096, 0, 4), 1, odd) == -6
        assert call(None, 0, buf) == 0                                     # nothing to do: no launch
        assert call(item(None, 0, 0), 1, buf) == 0                         # only an empty item
