"""GPU: Monte-Carlo dropout, BTX-DROP v1 (csrc/btx_drop.hip).  Forward and backward bit-equal to the numpy model
(tests/drop_model.py) on the smallest shapes that reach every path of the two kernels; the device sample word; MC lanes (with the
broadcast of a shared input); captured replays of mc.GraphedMC / mc.evaluate / autograd.GraphedTrainStep against eager runs at the
same sample indices, bit for bit; and the memory-content contract (tests/poison.py) for the entry points of _lib.EXPORTS_DROP.

COVERED / HOST_ONLY classify every name of `_lib.EXPORTS_DROP` (tests/test_dropout_cpu.py proves it without a GPU)."""
import contextlib
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

import drop_model as DM
import poison as P

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

F32, BF16 = torch.float32, torch.bfloat16
SEED = 0x0BADC0DE12345678
CHUNK = 8192   # BTX_DROP_CHUNK (include/btx_drop.h): the elements of a lane one workgroup owns, 4 sweeps of 256 threads x 8

COVERED = {
    "btx_dropout_fwd": "test_poisoned_buffers_do_not_change_a_result",
    "btx_dropout_bwd": "test_poisoned_buffers_do_not_change_a_result",
}
HOST_ONLY = ()   # no size query: the unit needs no workspace

# (tag, logical shape, mode, memory): the paths of btx_drop.hip
CASES = [
    ("partial_group", (3, 5), "element", "plain"),                  # 15 elements: one partial group, element-wise accesses
    ("ragged_c_cl", (2, 3, 5, 7), "element", "cl"),                 # 210 elements channels-last: 26 groups + a tail of 2
    ("pure_16_byte", (4, 16, 8, 8), "element", "cl"),               # 4096 elements: 16-byte accesses only
    ("chunk_plus_3", (1, CHUNK + 3), "element", "plain"),           # a second workgroup that owns 3 elements
    ("chunk_minus_3", (1, CHUNK - 3), "element", "plain"),          # one workgroup, its last group partial
    ("nchw_memory", (2, 3, 5, 7), "element", "nchw"),               # the index derived per element (drop_index_kernel)
    ("channel_ragged_c", (3, 10, 4, 4), "channel", "cl"),           # C % 8 != 0: drop_index_kernel on channels-last memory
    ("channel_nchw", (3, 10, 4, 4), "channel", "nchw"),
    ("channel_groups", (2, 16, 3, 3), "channel", "cl"),             # C % 8 == 0 channels-last: one Philox call per 8 channels
    ("channel_1d", (2, 7, 9), "channel", "plain"),                  # [N, C, L] contiguous
]
IDS = [c[0] for c in CASES]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _seed():
    import bayesian_torch_amd as bt
    bt.manual_seed(SEED)
    yield


def _tensor(shape, dtype, memory, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * 3.0).to(dtype).to(_dev())
    if memory == "cl":
        x = x.contiguous(memory_format=torch.channels_last)
    return x


def _bits(t):
    t = t.detach().contiguous().cpu()   # logical order
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF16 else t.numpy().view(np.uint32)


def _model_bits(x, keep, scale):
    if x.dtype == BF16:
        return DM.apply_bf16(_bits(x), keep, scale)
    return DM.apply_f32(x.detach().contiguous().cpu().numpy(), keep, scale).view(np.uint32)


def _assert_bits(got, x, keep, scale, tag):
    want = _model_bits(x, keep, scale)
    g = _bits(got)
    assert g.shape == want.shape, (tag, g.shape, want.shape)
    bad = int((g != want).sum())
    print("%s: %d elements, %d kept, %d differ from the model" % (tag, g.size, int(keep.sum()), bad))
    assert bad == 0, tag


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_equal_the_model_bit_for_bit(case, dtype):
    from bayesian_torch_amd import functional as BF, layers as L
    tag, shape, mode, memory = case
    layer = L.MCDropout(0.3, mode=mode)
    T, scale = DM.params(0.3)
    assert (T, float(scale)) == (layer._btx_T, layer._btx_scale)
    x = _tensor(shape, dtype, memory, seed=1)
    keep = DM.mask(shape, mode, T, SEED, 5, layer._btx_layer_id)
    out = BF.dropout_hip(x, T, scale, mode, SEED, 5, layer._btx_layer_id)
    assert out.shape == x.shape and out.dtype == dtype and out.stride() == x.stride()
    _assert_bits(out, x, keep, scale, tag + " forward")
    # through the module with autograd: the backward regenerates the mask (btx_dropout_bwd) and applies it to dy
    import bayesian_torch_amd as bt
    xg = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    dy = _tensor(shape, dtype, memory, seed=2)
    bt.set_sample_index(layer, 5)
    y = layer(xg)
    assert layer._btx_sample == 6 and torch.equal(y.detach(), out)
    y.backward(dy)
    _assert_bits(xg.grad, dy, keep, scale, tag + " backward")
    assert np.array_equal(layer.materialize_mask(shape, 5).numpy(), keep)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_views_off_the_16_byte_grid_and_out_aliasing_x(dtype):
    """x one element past a 16-byte boundary (element-wise accesses: never BTX_E_ALIGN), the slack around the view untouched; and
    out = x, on the grid and off it"""
    from bayesian_torch_amd import functional as BF
    T, scale = DM.params(0.5)
    shape = (9, 100)
    n = 900
    keep = DM.mask(shape, "element", T, SEED, 2, 77)
    buf = _tensor((n + 16,), dtype, "plain", seed=3)
    x = buf[1:1 + n].view(shape)
    assert x.data_ptr() % 16 == buf.element_size()
    ref = x.clone()
    out = BF.dropout_hip(x, T, scale, "element", SEED, 2, 77)
    _assert_bits(out, ref, keep, scale, "off-grid x")
    before = buf.clone()
    got = BF.dropout_hip(x, T, scale, "element", SEED, 2, 77, out=x)
    assert got.data_ptr() == x.data_ptr()
    _assert_bits(x, ref, keep, scale, "off-grid in place")
    assert torch.equal(buf[:1], before[:1]) and torch.equal(buf[1 + n:], before[1 + n:])
    a = _tensor((4, 16, 8, 8), dtype, "cl", seed=4)
    ref = a.clone(memory_format=torch.preserve_format)
    BF.dropout_hip(a, T, scale, "element", SEED, 2, 77, out=a)
    _assert_bits(a, ref, DM.mask((4, 16, 8, 8), "element", T, SEED, 2, 77), scale, "on-grid in place")


def test_edge_probabilities_and_dropped_non_finite_values():
    from bayesian_torch_amd import layers as L
    for dtype in (F32, BF16):
        x = _tensor((5, 33), dtype, "plain", seed=5)
        x[0, 0], x[0, 1] = float("inf"), -0.0
        assert np.array_equal(_bits(L.MCDropout(0.0)(x)), _bits(x))            # p = 0: the identity bit for bit
        assert not _bits(L.MCDropout(1.0)(x)).any()                              # p = 1: +0.0 everywhere
        bad = torch.full((4, 64), float("inf"), dtype=dtype, device=_dev())
        bad[:, 1::2] = float("nan")
        half = L.MCDropout(0.5)
        got = half(bad)
        keep = torch.from_numpy(DM.mask((4, 64), "element", 32768, SEED, 0, half._btx_layer_id)).to(_dev())
        assert 0 < int(keep.sum()) < 256 and not _bits(got[~keep]).any()         # dropped inf / NaN: +0.0 by selection
        assert bool((torch.isinf(got) | torch.isnan(got))[keep].all())


def test_device_sample_word_equals_the_host_index():
    from bayesian_torch_amd import functional as BF
    T, scale = DM.params(0.4)
    x = _tensor((6, 50), F32, "plain", seed=6)
    word = torch.tensor([9], dtype=torch.int32, device=_dev())
    a = BF.dropout_hip(x, T, scale, "element", SEED, 9, 3)
    b = BF.dropout_hip(x, T, scale, "element", SEED, 12345, 3, sample_dev=word)   # the host index is ignored
    assert torch.equal(a, b)
    word.fill_(10)
    c = BF.dropout_hip(x, T, scale, "element", SEED, 9, 3, sample_dev=word)
    assert not torch.equal(a, c) and torch.equal(c, BF.dropout_hip(x, T, scale, "element", SEED, 10, 3))
    _assert_bits(c, x, DM.mask((6, 50), "element", T, SEED, 10, 3), scale, "device word 10")


def _mlp(variational):
    """Linear(5 -> 15) -> ReLU -> MCDropout -> Linear(15 -> 4): 45 elements per lane behind the dropout, off the 16-byte grid"""
    from bayesian_torch_amd import layers as L
    torch.manual_seed(0)
    if variational:
        a, b = L.LinearReparameterization(5, 15), L.LinearReparameterization(15, 4)
        a.dnn_to_bnn_flag = b.dnn_to_bnn_flag = True
    else:
        a, b = nn.Linear(5, 15), nn.Linear(15, 4)
    return nn.Sequential(a, nn.ReLU(), L.MCDropout(0.5), b).to(_dev()).eval()


def _singles(net, x, indices, concurrent):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import functional as BF
    outs = []
    with torch.no_grad(), (BF.concurrent_plan() if concurrent else contextlib.nullcontext()):
        for s in indices:
            bt.set_sample_index(net, s)
            outs.append(net(x).clone())
    return outs


@pytest.mark.parametrize("variational", [True, False], ids=["mixed", "dropout_only"])
def test_lanes_equal_single_sample_forwards(variational):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import _lib
    net = _mlp(variational)
    x = _tensor((3, 5), F32, "plain", seed=7)
    idx = [5, 9, 6]
    want = _singles(net, x, idx, concurrent=True)
    assert not torch.equal(want[0], want[1])
    with torch.no_grad():
        bt.set_sample_lanes(net, idx, batch=3)
        try:
            got = net(x)
            assert tuple(got.shape) == (9, 4)
            for k in range(3):
                assert torch.equal(got[3 * k:3 * k + 3], want[k]), "lane %d" % k
            bt.set_sample_lanes(net, idx, batch=3)
            with pytest.raises(_lib.BtxError):
                net[2](torch.zeros(4, 15, device=_dev()))            # neither the shared 3 rows nor 3 lanes of 3
            with pytest.raises(_lib.BtxError), torch.enable_grad():
                net[2](torch.zeros(3, 15, device=_dev(), requires_grad=True))   # lanes are an inference feature
        finally:
            bt.set_sample_lanes(net, None)
    # the dropout layer on its own: the shared input is broadcast, lane l = the single forward at idx[l], bf16 and channels-last too
    from bayesian_torch_amd import functional as BF
    T, scale = DM.params(0.5)
    for dtype, shape, memory in ((BF16, (3, 15), "plain"), (F32, (2, 8, 3, 3), "cl"), (BF16, (2, 3, 5, 7), "nchw")):
        h = _tensor(shape, dtype, memory, seed=8)
        words = torch.tensor(idx, dtype=torch.int32, device=_dev())
        lanes = BF.dropout_hip(h, T, scale, "element", SEED, 0, 4, sample_dev=words, lanes=3, lane_batch=shape[0])
        assert lanes.shape[0] == 3 * shape[0]
        for k, s in enumerate(idx):
            one = BF.dropout_hip(h, T, scale, "element", SEED, s, 4)
            assert torch.equal(lanes[k * shape[0]:(k + 1) * shape[0]], one), (dtype, shape, k)
        again = BF.dropout_hip(lanes, T, scale, "element", SEED, 0, 4, sample_dev=words, lanes=3, lane_batch=shape[0])
        for k, s in enumerate(idx):   # a laned input: every lane reads its own rows
            one = BF.dropout_hip(lanes[k * shape[0]:(k + 1) * shape[0]], T, scale, "element", SEED, s, 4)
            assert torch.equal(again[k * shape[0]:(k + 1) * shape[0]], one), (dtype, shape, k)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("variational", [True, False], ids=["mixed", "dropout_only"])
def test_graphed_mc_replays_equal_eager_forwards(variational, lanes):
    from bayesian_torch_amd import mc
    net = _mlp(variational)
    x = _tensor((3, 5), F32, "plain", seed=9)
    idx = [4, 11, 12]
    want = _singles(net, x, idx, concurrent=lanes > 1)
    g = mc.GraphedMC(net, x, lanes=lanes, keep_logits=True)
    try:
        if lanes == 1:
            for k, s in enumerate(idx):
                g.run(s)
                torch.cuda.synchronize()
                assert torch.equal(g.lane_logits[0], want[k]), "replay at index %d" % s
        else:
            g.run_many(idx)
            torch.cuda.synchronize()
            for k in range(3):
                assert torch.equal(g.lane_logits[k], want[k]), "lane %d" % k
    finally:
        g.close()
    again = _singles(net, x, idx[:1], concurrent=lanes > 1)       # the model is a plain eager model again
    assert torch.equal(again[0], want[0])


def test_graphed_evaluate_of_a_dropout_only_mlp_equals_the_eager_loop():
    from bayesian_torch_amd import mc
    net = _mlp(False)
    batches = [(_tensor((3, 5), F32, "plain", seed=20 + i), torch.tensor([i, 3 - i, 1], device=_dev())) for i in range(2)]
    ev_g = mc.evaluate(net, batches, 4, lanes=2, graphed=True, evaluator=mc.Evaluator(4, capacity=6, device=_dev()))
    ev_e = mc.Evaluator(4, capacity=6, device=_dev())
    for x, y in batches:
        ev_e.update(mc.mc_forward(net, x, 4, lanes=2, reduce=False, rank=0, world=1), y)
    torch.cuda.synchronize()
    assert torch.equal(ev_g.state, ev_e.state) and P.bits_equal(ev_g.records_buffer, ev_e.records_buffer)
    assert ev_g.compute()["top1"] == ev_e.compute()["top1"]
    # and dropout is really on in eval mode: two samples of one batch differ
    a, b = _singles(net, batches[0][0], [0, 1], concurrent=False)
    assert not torch.equal(a, b)


def test_captured_training_step_equals_the_eager_step_bit_for_bit():
    """conv3x3(8 -> 8) -> ReLU -> MCDropout2d -> flatten -> LinearReparameterization on [4, 8, 6, 6]: two replays of
    GraphedTrainStep(num_mc=2, optimizer=SGD) leave every parameter bit-equal to two eager mc_train_forward steps; the two passes of
    a step draw different masks"""
    from bayesian_torch_amd import autograd as AG, layers as L, optim
    torch.manual_seed(1)
    conv, fc = L.Conv2dReparameterization(8, 8, 3, padding=1), L.LinearReparameterization(8 * 6 * 6, 5)
    conv.dnn_to_bnn_flag = fc.dnn_to_bnn_flag = True
    drop = L.MCDropout2d(0.5)
    net = nn.Sequential(conv, nn.ReLU(), drop, nn.Flatten(), fc).to(_dev()).train()
    x = _tensor((4, 8, 6, 6), F32, "cl", seed=11)
    y = torch.tensor([1, 0, 4, 3], device=_dev())
    loss_fn = lambda out, tgt: torch.nn.functional.cross_entropy(out.mean(0), tgt)  # noqa: E731
    params = list(net.parameters())
    p0 = [p.detach().clone() for p in params]
    step = AG.GraphedTrainStep(net, x, y, loss_fn=loss_fn, optimizer=optim.SGD(params, lr=0.05), num_mc=2)
    try:
        losses = [float(step.run(3)), float(step.run(4))]
        torch.cuda.synchronize()
        graphed = [p.detach().clone() for p in params]
        words = step.sample_dev.clone()
        assert words.tolist() == [8, 9]
        m0 = drop.materialize_mask((4, 8, 6, 6), None, sample_dev=words[0:1])
        m1 = drop.materialize_mask((4, 8, 6, 6), None, sample_dev=words[1:2])
        assert not torch.equal(m0, m1) and torch.equal(m0, drop.materialize_mask((4, 8, 6, 6), 8))
    finally:
        step.close()
    with torch.no_grad():
        for p, q in zip(params, p0):
            p.copy_(q)
            p.grad = None
    opt = optim.SGD(params, lr=0.05)
    eager = []
    for s in (3, 4):
        for p in params:
            p.grad = None
        loss = loss_fn(AG.mc_train_forward(net, x, 2, s), y)
        loss.backward()
        opt.step()
        eager.append(float(loss.detach()))
    torch.cuda.synchronize()
    print("captured losses %r, eager losses %r" % (losses, eager))
    assert eager == losses and losses[0] != losses[1]
    for i, (p, gq, q0) in enumerate(zip(params, graphed, p0)):
        assert torch.equal(p.detach(), gq), "parameter %d differs between the captured and the eager run" % i
        assert not torch.equal(p.detach(), q0)


@contextlib.contextmanager
def _recorded(names):
    """record which entry points of EXPORTS_DROP are entered (tests/poison.py records the names of _lib.EXPORTS only)"""
    from bayesian_torch_amd import _lib
    lib, calls, saved = _lib.lib(), [], {}
    try:
        for n in names:
            saved[n] = getattr(lib, n)

            def entry(*a, _n=n, _f=saved[n]):
                calls.append(_n)
                return _f(*a)
            setattr(lib, n, entry)
        yield calls
    finally:
        for n, f in saved.items():
            setattr(lib, n, f)


def test_poisoned_buffers_do_not_change_a_result():
    """every entry of EXPORTS_DROP that touches device memory, plain and with every fresh buffer filled with 0xFF / 0x7F first: equal
    bits, forward (every kernel path, lanes with broadcast) and backward"""
    from bayesian_torch_amd import _lib, functional as BF, layers as L
    import bayesian_torch_amd as bt
    T, scale = DM.params(0.3)
    words = torch.tensor([5, 9, 6], dtype=torch.int32, device=_dev())

    def run():
        outs = []
        for tag, shape, mode, memory in CASES:
            for dtype in (F32, BF16):
                x = _tensor(shape, dtype, memory, seed=1)
                outs.append(BF.dropout_hip(x, T, scale, mode, SEED, 5, 21))
                if mode == "element":
                    outs.append(BF.dropout_hip(x, T, scale, mode, SEED, 0, 21, sample_dev=words, lanes=3, lane_batch=shape[0]))
                layer = L.MCDropout(0.3, mode=mode)
                layer._btx_layer_id = 21
                bt.set_sample_index(layer, 5)
                xg = x.clone(memory_format=torch.preserve_format).requires_grad_()
                layer(xg).backward(_tensor(shape, dtype, memory, seed=2))
                outs.append(xg.grad)
        torch.cuda.synchronize()
        return outs

    clean = run()
    assert not P.any_nan(clean)
    for byte in P.PATTERNS:
        with _recorded(_lib.EXPORTS_DROP) as calls, P.poisoned(byte) as rec:
            got = run()
        assert rec.bytes > 0 and rec.tensors > 0, "nothing was poisoned"
        assert set(calls) == {e for e, t in COVERED.items() if t == "test_poisoned_buffers_do_not_change_a_result"}
        assert P.bits_equal(got, clean), "a result under %#04x poison differs from the plain run" % byte
        for e in sorted(set(calls)):
            print("%s: %d buffers, %d bytes poisoned, pattern %02x: equal" % (e, rec.tensors, rec.bytes, byte))
