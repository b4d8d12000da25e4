"""GPU: every element of what the REDUCING kernels return against float64 — training-mode BatchNorm (csrc/btx_bn.hip), MC
accumulate (btx_small.hip K6), the model KL and its gradients, global average pooling.  tests/test_gpu_elementwise.py did this
for the contraction kernels and max-pool; the rel-L2 / atol tests of the other files stay as they are.  A reduction goes wrong in
ways an averaged metric hides: a row dropped or counted twice at a block or grid cap, a channel group skipped when C/8 does not
divide 256, a class column skipped past a stride boundary (tests/test_envelope_cpu.py plants each of these into a numpy
emulation and shows the older bar passing it).

  1. exact       small-integer x / dy: x - pivot and its square are integers, every f32 partial sum stays below 2^24, the f64
                 fold holds the exact sums.  Batch mean and unbiased variance (read through momentum = 1), save_mean and
                 save_invstd equal the float64 values to 1 ulp of f32 (a dropped row moves them by ~1/M); dbeta == sum dy bit for
                 bit; behind a fused ReLU dres == dy [y > 0] on the stored y and dbeta == sum dres.  Average pool: bit for bit.
  2. envelope    Gaussian inputs, bounds of envelope.py (derived there, not fitted): y, dx per element, dgamma,
                 dbeta, the saved statistics and the running estimates per channel; sum p, sum p^2 and the entropy of MC
                 accumulate per entry; dmu / drho of the KL per element.
  3. bits        two calls on the same inputs return equal bits.

References are float64 on the CPU from the dtype-rounded inputs, at most 16 threads.  Each check prints one line
`name prec: worst err/bound R at index`; profiles/reduction_envelope.txt holds the lines of one full run, the measured
c0 (envelope.C0_ULP) and the two numbers of the pivot case.
"""
import warnings

import numpy as np
import pytest
import torch

import envelope as E
from test_gpu_elementwise import _Log, _dev

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
torch.set_num_threads(min(16, torch.get_num_threads()))

F32, BF16 = torch.float32, torch.bfloat16
_N = {F32: "f32", BF16: "bf16"}


# =============================================================================================================================
# c0: the device's expf / logf in ulps (first: the MC and KL envelopes use it)
# =============================================================================================================================
def test_device_exp_and_log_error_in_ulps_is_covered_by_c0():
    """torch.exp / torch.log on the GPU are the math-library functions btx_small.hip calls; dense grids over [-104, 0] (down to
    where f32 underflows altogether) and [1e-38, 1] against float64.  envelope.C0_ULP is twice the larger maximum."""
    dev = _dev()
    n = 1 << 22
    xe = torch.linspace(-104.0, 0.0, n, dtype=torch.float64).to(F32)
    xl = torch.exp(torch.linspace(float(np.log(1e-38)), 0.0, n, dtype=torch.float64)).to(F32)
    we, ie = E.ulp_error(torch.exp(xe.to(dev)).cpu(), torch.exp(xe.double()))
    wl, il = E.ulp_error(torch.log(xl.to(dev)).cpu(), torch.log(xl.double()))
    sub = xe < -87.4  # subnormal results
    ws, _ = E.ulp_error(torch.exp(xe[sub].to(dev)).cpu(), torch.exp(xe[sub].double()))
    print("c0: exp %.4g ulp at x = %.9g (subnormal results: %.4g); log %.4g ulp at x = %.9g; envelope.C0_ULP = %.4g"
          % (we, float(xe[ie]), ws, wl, float(xl[il]), E.C0_ULP))
    assert max(we, wl) <= E.C0_ULP


# =============================================================================================================================
# 1. BatchNorm training
# =============================================================================================================================
_CL = {4: torch.channels_last, 5: torch.channels_last_3d}
_BN = {2: torch.nn.BatchNorm1d, 4: torch.nn.BatchNorm2d, 5: torch.nn.BatchNorm3d}


def _rows(t):
    """[M, C] float64 on the CPU, rows in the order of the channels-last storage"""
    t = t.detach().cpu().double()
    if t.dim() > 2:
        t = t.movedim(1, -1)
    return t.reshape(-1, t.shape[-1]).contiguous()


def _to_dev(t, dtype):
    t = t.to(dtype).to(_dev())
    return t.contiguous(memory_format=_CL[t.dim()]) if t.dim() in _CL else t.contiguous()


def _bn_module(shape, pdtype, affine=True, track=True, momentum=0.1, seed=7, zero_channel=None):
    C = shape[1]
    g = torch.Generator().manual_seed(seed)
    bn = _BN[len(shape)](C, momentum=momentum, affine=affine, track_running_stats=track)
    with torch.no_grad():
        if affine:
            bn.weight.copy_(0.5 + torch.rand(C, generator=g))
            bn.bias.copy_(0.2 * torch.randn(C, generator=g))
            if zero_channel is not None:
                bn.weight[zero_channel] = 0.0
                bn.bias[zero_channel] = 0.0
        if track:
            bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.to(_dev()).to(pdtype).train()


def _bn_call(bn, x, dy, res=None, relu=False):
    """one forward + backward through btx_bn_train_fwd / _bwd -> dict of what they wrote (the module's running estimates move)"""
    from bayesian_torch_amd import autograd as ag
    x1 = x.clone().requires_grad_(True)
    r1 = res.clone().requires_grad_(True) if res is not None else None
    assert ag.bn_train_usable(bn, x1), "this case must take the HIP kernels"
    for p in bn.parameters():
        p.grad = None
    y = ag.batch_norm_train(bn, x1, residual=r1, relu=relu)
    saved = y.grad_fn.saved_tensors
    assert y.dtype == x.dtype and y.stride() == x.stride()
    y.backward(dy)
    out = dict(y=y.detach(), dx=x1.grad, save_mean=saved[2], save_invstd=saved[3],
               dgamma=bn.weight.grad if bn.affine else None, dbeta=bn.bias.grad if bn.affine else None,
               dres=r1.grad if r1 is not None else None)
    if bn.track_running_stats:
        out.update(rm=bn.running_mean.detach().clone(), rv=bn.running_var.detach().clone())
    return out


def _bn_gauss(shape, dtype, seed, mean=0.3, std=1.7):
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(*shape, generator=g)  # noqa: E731
    return _to_dev(rn() * std + mean, dtype), _to_dev(rn(), dtype), _to_dev(rn(), dtype)


def _bn_envelope(log, name, bn, x, dy, res=None, relu=False, bits=True):
    """forward + backward against bn_forward64 / bn_backward64, every element and every channel; a second call on the same inputs
    must return the same bits"""
    dt, pd = _N[x.dtype], next((p.dtype for p in list(bn.parameters()) + list(bn.buffers()) if p.is_floating_point()), F32)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    got = _bn_call(bn, x, dy, res, relu)
    x64, dy64 = _rows(x), _rows(dy)
    M, C = x64.shape
    K = E.bn_chain(M, C)
    f = E.bn_forward64(x64, bn.weight if bn.affine else None, bn.bias if bn.affine else None, bn.eps, K,
                       residual=_rows(res) if res is not None else None, relu=relu)
    mask = (_rows(got["y"]) > 0).double() if relu else None  # the mask of the y the kernel stored; y itself is checked below
    bw = E.bn_backward64(x64, dy64, f, K, mask=mask)
    st = (lambda b, r: E.store_rounding(b, r)) if x.dtype == BF16 else (lambda b, r: b)
    sp = (lambda b, r: E.store_rounding(b, r)) if pd == BF16 else (lambda b, r: E._np(b) + E.REF32_UNIT * np.abs(E._np(r)))
    log.check(name + " y", dt, _rows(got["y"]), f["y"], st(f["b_y"], f["y"]))
    log.check(name + " dx", dt, _rows(got["dx"]), bw["dx"], st(bw["b_dx"], bw["dx"]))
    log.check(name + " save_mean", dt, got["save_mean"], f["mean"], f["d_mean"])
    log.check(name + " save_invstd", dt, got["save_invstd"], f["invstd"], f["d_invstd"])
    if bn.affine:
        log.check(name + " dgamma", dt, got["dgamma"], bw["dgamma"], sp(bw["b_dgamma"], bw["dgamma"]))
        log.check(name + " dbeta", dt, got["dbeta"], bw["dbeta"], sp(bw["b_dbeta"], bw["dbeta"]))
    if res is not None:
        log.check(name + " dres", dt, _rows(got["dres"]), bw["g"], np.zeros((M, C)))  # dy where y > 0, nothing computed
    if bn.track_running_stats:
        rm, b_rm, rv, b_rv = E.bn_running64(f, state["running_mean"], state["running_var"], bn.momentum)
        log.check(name + " running_mean", dt, got["rm"], rm, sp(b_rm, rm))
        log.check(name + " running_var", dt, got["rv"], rv, sp(b_rv, rv))
        assert int(bn.num_batches_tracked) == int(state["num_batches_tracked"]) + 1
    if bits:
        bn.load_state_dict(state)
        again = _bn_call(bn, x, dy, res, relu)
        for k in ("y", "dx", "dgamma", "dbeta", "dres", "rm", "rv"):
            if got.get(k) is not None and not torch.equal(got[k], again[k]):
                log.bad.append("%s %s: %s differs between two calls on the same inputs" % (name, dt, k))
    return got, f, bw


# the smallest shapes that reach each path (module inputs, channels-last storage, or 2-D)
BN_SHAPES = [
    pytest.param((2, 8), F32, id="2x8-f32-minimum-M"),
    pytest.param((2, 8), BF16, id="2x8-bf16-minimum-M"),
    pytest.param((3, 2040), F32, id="3x2040-f32-last-thread-idle"),
    pytest.param((3, 2040), BF16, id="3x2040-bf16-last-thread-idle"),
    pytest.param((5, 40, 3, 7), F32, id="5x40x3x7-f32-one-block-under-four-rows-in-flight"),
    pytest.param((5, 40, 3, 7), BF16, id="5x40x3x7-bf16-one-block-under-four-rows-in-flight"),
    pytest.param((1, 72, 33, 31), F32, id="1x72x33x31-f32-nine-groups"),
    pytest.param((1, 72, 33, 31), BF16, id="1x72x33x31-bf16-nine-groups"),
    pytest.param((257, 1024), F32, id="257x1024-f32-fold-over-17-blocks"),
    pytest.param((257, 1024), BF16, id="257x1024-bf16-fold-over-17-blocks"),
    pytest.param((256, 1024), F32, id="256x1024-f32-fold-over-16-blocks"),
    pytest.param((256, 1024), BF16, id="256x1024-bf16-fold-over-16-blocks"),
    pytest.param((4099, 2048), BF16, id="4099x2048-bf16-512-block-cap-ragged-last-group"),
    pytest.param((8200, 2048), F32, id="8200x2048-f32-apply-grid-beyond-8192-blocks"),
    pytest.param((2, 16, 3, 5, 7), F32, id="BatchNorm3d-2x16x3x5x7-f32"),
    pytest.param((2, 16, 3, 5, 7), BF16, id="BatchNorm3d-2x16x3x5x7-bf16"),
]


@pytest.mark.parametrize("shape,dtype", BN_SHAPES)
def test_batchnorm_training_every_element_inside_the_envelope(shape, dtype):
    x, dy, _ = _bn_gauss(shape, dtype, 101)
    bn = _bn_module(shape, dtype)  # parameters and running estimates in the activations' dtype, as bench.py's model
    log = _Log()
    _bn_envelope(log, "bn %s" % "x".join(map(str, shape)), bn, x, dy)
    log.done()


@pytest.mark.parametrize("shape,dtype", BN_SHAPES)
def test_batchnorm_training_exact_sums_on_small_integers(shape, dtype):
    """zero tolerance on the sums: see the file's docstring.  f32 parameters (a bf16 running estimate would round the statistic
    away), momentum = 1: running = 0 * old + batch"""
    C = shape[1]
    x, dy, res = (_to_dev(E.small_ints(shape, s, lim=3), dtype) for s in (111, 112, 113))
    x64 = _rows(x)
    M = x64.shape[0]
    assert M <= 466000  # 36 M < 2^24: (x - pivot)^2 <= 36
    mean, var, unb, invstd = E.bn_exact_stats(x64, 1e-5)
    log = _Log()
    name = "bn exact %s" % "x".join(map(str, shape))
    for relu in (False, True):
        bn = _bn_module(shape, F32, momentum=1.0)
        got = _bn_call(bn, x, dy, res if relu else None, relu)
        tag = name + (" res_relu" if relu else "")
        log.check(tag + " batch mean", _N[dtype], got["rm"], mean, E.ulp32(mean))
        log.check(tag + " unbiased var", _N[dtype], got["rv"], unb, E.ulp32(unb))
        log.check(tag + " save_mean", _N[dtype], got["save_mean"], mean, E.ulp32(mean))
        log.check(tag + " save_invstd", _N[dtype], got["save_invstd"], invstd, E.ulp32(invstd))
        gy = _rows(dy)
        if relu:
            gy = gy * (_rows(got["y"]) > 0)
            log.check(tag + " dres", _N[dtype], _rows(got["dres"]), gy, np.zeros((M, C)))
        log.check(tag + " dbeta", _N[dtype], got["dbeta"], gy.sum(0), np.zeros(C))
    log.done()


BN_VARIANTS = ["affine-false", "no-running-stats", "momentum-0", "momentum-1", "f32-params-bf16-activations",
               "zero-gamma-beta-channel-under-relu", "constant-channel", "res-relu-three-groups"]


@pytest.mark.parametrize("variant", BN_VARIANTS)
def test_batchnorm_training_module_variants_inside_the_envelope(variant):
    shape = (4, 24, 9, 11)  # C/8 = 3 does not divide 256: 85 rows per pass, one thread idle
    dtype = BF16 if variant == "f32-params-bf16-activations" else F32
    x, dy, res = _bn_gauss(shape, dtype, 121)
    kw, relu, use_res = {}, False, False
    if variant == "affine-false":
        kw = dict(affine=False)
    elif variant == "no-running-stats":
        kw = dict(track=False)
    elif variant == "momentum-0":
        kw = dict(momentum=0.0)
    elif variant == "momentum-1":
        kw = dict(momentum=1.0)
    elif variant == "zero-gamma-beta-channel-under-relu":
        kw, relu = dict(zero_channel=5), True
    elif variant == "constant-channel":
        x[:, 7] = 0.75
    elif variant == "res-relu-three-groups":
        relu, use_res = True, True
    bn = _bn_module(shape, F32, **kw)
    log = _Log()
    got, f, bw = _bn_envelope(log, "bn " + variant, bn, x, dy, res if use_res else None, relu)
    if variant == "zero-gamma-beta-channel-under-relu":
        # y = relu(0 * xhat + 0) = 0: torch.relu in float64 passes no gradient at 0, so nothing comes back through channel 5
        z64 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
        torch.relu(z64).backward(torch.ones(1, dtype=torch.float64))
        assert float(z64.grad) == 0.0
        for k in ("y", "dx"):
            assert float(got[k][:, 5].abs().max()) == 0.0, k
        assert float(got["dgamma"][5]) == 0.0 and float(got["dbeta"][5]) == 0.0
    if variant == "constant-channel":
        assert float(f["var"][7]) == 0.0 and float(got["save_mean"][7]) == 0.75  # x - pivot = 0: the sums are exact zeros
        assert float(got["save_invstd"][7]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(bn.eps)))))
    log.done()


def test_batchnorm_pivot_survives_an_outlier_in_row_zero():
    """one row-0 value 300 away from a unit-spread channel (32 channels of 64, both signs; three draws of the input), M = 25 088 in
    f32: the relative error of the batch variance (read as the running estimate at momentum 1) against float64, for btx_bn and for
    torch's own f32 BatchNorm on the GPU on the same input.  A pivot taken from row 0 alone loses more than 1e-4 of the variance
    here (emulated: tests/test_envelope_cpu.py); the median of rows 0, M/2, M-1 must keep btx_bn within 2 x of the kernel it
    replaces, over all outlier channels of all draws (the factor allows another draw of roundings)."""
    shape = (8, 64, 56, 56)
    worst_o, worst_t = 0.0, 0.0
    for seed in (131, 132, 133):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(*shape, generator=g) + 0.3
        x[0, :32, 0, 0] += torch.tensor([300.0, -300.0] * 16)
        x = _to_dev(x, F32)
        dy = torch.zeros_like(x)
        x64 = _rows(x)
        M = x64.shape[0]
        unb = ((x64 - x64.mean(0)) ** 2).sum(0) / (M - 1)
        ours = _bn_call(_bn_module(shape, F32, momentum=1.0), x, dy)["rv"].double().cpu()
        ref = torch.nn.BatchNorm2d(64, momentum=1.0).to(_dev()).train()
        with torch.no_grad():
            ref(x)
        theirs = ref.running_var.double().cpu()
        eo, et = ((ours - unb).abs() / unb), ((theirs - unb).abs() / unb)
        print("pivot seed %d: variance rel. error, outlier channels: btx_bn %.3g, torch f32 %.3g; other channels: btx_bn %.3g, "
              "torch f32 %.3g" % (seed, float(eo[:32].max()), float(et[:32].max()), float(eo[32:].max()), float(et[32:].max())))
        worst_o, worst_t = max(worst_o, float(eo[:32].max())), max(worst_t, float(et[:32].max()))
    print("pivot: worst of 96 outlier channels: btx_bn %.3g, torch f32 %.3g" % (worst_o, worst_t))
    assert worst_o <= 2 * worst_t


# =============================================================================================================================
# 2. MC accumulate
# =============================================================================================================================
def _mc_logits(S, bs, C, seed, dtype, spread=None):
    g = torch.Generator().manual_seed(seed)
    if spread:
        x = (torch.rand(S, bs, C, generator=g) * 2 - 1) * spread
    else:
        x = torch.randn(S, bs, C, generator=g) * 2.0
    return x.to(dtype)


def _mc_check(log, name, x, calls):
    """x [S, bs, C] (CPU, dtype-rounded); calls: the lane counts of the launches that accumulate the S samples into ONE buffer"""
    from bayesian_torch_amd import mc
    S, bs, C = x.shape
    assert sum(calls) == S
    packed = torch.zeros(mc.packed_numel(bs, C), dtype=F32, device=_dev())
    at = 0
    for lanes in calls:
        lg = x[at:at + lanes].reshape(lanes * bs, C).to(_dev())
        if lanes == 1:
            mc.accumulate(packed, lg, kl=1.5)
        else:
            mc.accumulate_lanes(packed, lg, lanes, kl=1.5)
        at += lanes
    torch.cuda.synchronize()
    pk = packed.cpu()
    ref = E.mc_reference(x.double().numpy())
    dt = _N[x.dtype]
    log.check(name + " sum p", dt, pk[:bs * C].reshape(bs, C), ref["sum_p"], ref["b_sum_p"])
    log.check(name + " sum p^2", dt, pk[bs * C:2 * bs * C].reshape(bs, C), ref["sum_p2"], ref["b_sum_p2"])
    log.check(name + " entropy", dt, pk[2 * bs * C:2 * bs * C + bs], ref["ent"], ref["b_ent"])
    log.check(name + " kl, count", dt, pk[2 * bs * C + bs:], np.array([1.5 * S, float(S)]), np.zeros(2))
    assert float(np.cumsum(ref["p"], 0).max()) <= 1.0 + 1e-9  # running sums below 1: the accumulation term is within S u32
    return ref


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1023, 1025, 4099])
def test_mc_accumulate_every_entry_against_float64_softmax(C, dtype):
    log = _Log()
    for bs in (1, 3):
        _mc_check(log, "mc C=%d bs=%d" % (C, bs), _mc_logits(1, bs, C, 200 + C + bs, dtype), [1])
    log.done()


@pytest.mark.parametrize("lanes", [1, 2, 15, 16, 17, 33])
def test_mc_accumulate_lanes_against_float64(lanes):
    log = _Log()
    for bs, dtype in ((1, BF16), (3, F32)):
        _mc_check(log, "mc lanes=%d C=1000 bs=%d" % (lanes, bs), _mc_logits(lanes, bs, 1000, 300 + lanes + bs, dtype), [lanes])
    log.done()


def test_mc_accumulate_lds_chunk_loop_and_the_widest_row():
    """C = 6143 with 5 lanes runs in chunks whether the 96 KiB opt-in is granted (4 lanes per chunk) or not (2); C = 24575 =
    mc.MC_MAX_CLASSES needs the opt-in for a single lane and must run"""
    from bayesian_torch_amd import mc
    assert mc.MC_MAX_CLASSES == 24575
    log = _Log()
    _mc_check(log, "mc C=6143 lanes=5 bs=3", _mc_logits(5, 3, 6143, 401, F32), [5])
    _mc_check(log, "mc C=6143 lanes=5 bs=1", _mc_logits(5, 1, 6143, 402, BF16), [5])
    _mc_check(log, "mc C=24575 lanes=3 bs=3", _mc_logits(3, 3, 24575, 403, F32), [3])
    _mc_check(log, "mc C=24575 lanes=3 bs=1", _mc_logits(3, 1, 24575, 404, BF16), [3])
    log.done()


def test_mc_accumulate_wide_logits_minus_infinity_and_a_second_accumulation():
    log = _Log()
    for bs in (1, 3):
        ref = _mc_check(log, "mc +-80 C=1000 bs=%d" % bs, _mc_logits(1, bs, 1000, 410 + bs, F32, spread=80.0), [1])
        assert float((ref["p"] < 1e-45).mean()) > 0.3  # a third of the classes underflow f32 altogether
        x = _mc_logits(1, bs, 257, 420 + bs, F32)
        x[0, bs - 1, 5:40] = float("-inf")
        x[0, 0, 256] = float("-inf")
        ref = _mc_check(log, "mc -inf C=257 bs=%d" % bs, x, [1])
        assert float(ref["b_sum_p"][0, 256]) == 0.0  # exactly 0 there
        _mc_check(log, "mc 3 + 2 lanes into one buffer C=1000 bs=%d" % bs, _mc_logits(5, bs, 1000, 430 + bs, BF16), [3, 2])
        _mc_check(log, "mc 1 + 1 into one buffer C=65 bs=%d" % bs, _mc_logits(2, bs, 65, 440 + bs, F32), [1, 1])
    log.done()


# =============================================================================================================================
# 3. KL of a model and its gradients
# =============================================================================================================================
KL_SIZES = [1, 3, 2049, 600001] + [(7 * i * i + 5) % 3000 + 1 for i in range(46)]  # 50 items: the batch splits at 48


def _kl_items(dev):
    """50 (mu, rho) tensors sliced from flat buffers: every third item starts 4 bytes past a 16-byte boundary, every third 12
    bytes past one (the scalar load path), the others on one; odd items carry tensor priors"""
    g = torch.Generator().manual_seed(501)
    total = sum(-(-n // 4) * 4 + 8 for n in KL_SIZES)
    pool = lambda: torch.empty(total, dtype=F32, device=dev)  # noqa: E731
    bufs = dict(mu=pool(), rho=pool(), pm=pool(), ps=pool(), dmu=pool(), drho=pool())
    assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
    items, at = [], 0
    for i, n in enumerate(KL_SIZES):
        off = at + (0, 1, 3)[i % 3]
        v = {k: b[off:off + n] for k, b in bufs.items()}
        v["mu"].copy_(torch.randn(n, generator=g))
        v["rho"].copy_(torch.rand(n, generator=g) * 40 - 20)
        tens = i % 2 == 1
        if tens:
            v["pm"].copy_(0.3 * torch.randn(n, generator=g))
            v["ps"].copy_(0.2 + torch.rand(n, generator=g))
        items.append(dict(v=v, tens=tens, pm=0.1 + 0.01 * i, ps=0.7 + 0.02 * i, n=n, byte_offset=4 * (off % 4)))
        at += -(-n // 4) * 4 + 8
    return items


def test_kl_model_value_and_every_gradient_element_against_float64():
    from bayesian_torch_amd import functional as BF
    dev = _dev()
    items = _kl_items(dev)
    assert {it["byte_offset"] for it in items} == {0, 4, 12} and len(items) == 50 and max(KL_SIZES) > 256 * 256 * 8
    entries = [(it["v"]["mu"], it["v"]["rho"], it["pm"], it["ps"], it["v"]["pm"] if it["tens"] else None,
                it["v"]["ps"] if it["tens"] else None) for it in items]
    grads = [(it["v"]["dmu"], it["v"]["drho"]) for it in items]
    gout = torch.tensor(1.7, dtype=F32, device=dev)
    kl = float(BF.kl_model_hip(entries))
    BF.kl_model_bwd_hip(entries, grads, gout)
    torch.cuda.synchronize()
    log = _Log()
    kl64, worst = 0.0, {}
    for i, it in enumerate(items):
        c = {k: t.cpu().double().numpy() for k, t in it["v"].items()}
        pm, ps = (c["pm"], c["ps"]) if it["tens"] else (float(np.float32(it["pm"])), float(np.float32(it["ps"])))
        k64, dmu, b_dmu, drho, b_drho = E.kl_reference(c["mu"], c["rho"], pm, ps, float(gout))
        kl64 += k64
        for name, got, ref, bnd in (("dmu", c["dmu"], dmu, b_dmu), ("drho", c["drho"], drho, b_drho)):
            tag = "kl item %d (n = %d, %s priors, +%d bytes) %s" % (i, it["n"], "tensor" if it["tens"] else "scalar", it["byte_offset"], name)
            if i < 4:
                log.check(tag, "f32", got, ref, bnd)  # the sizes 1, 3, 2049, 600 001: one line each
            else:
                rep = E.check(got, ref, bnd)
                if not rep.ok:
                    log.bad.append("%s: %s" % (tag, rep))
                if rep.worst >= worst.get(name, (-1.0,))[0]:
                    worst[name] = (rep.worst, tag, rep)
    for name, (w, tag, rep) in worst.items():
        print(rep.line(tag + " [the worst of items 4..49]", "f32"))
    print("kl of 50 items: %.9g, float64 %.9g, rel. error %.3g" % (kl, kl64, abs(kl - kl64) / abs(kl64)))
    assert abs(kl - kl64) <= 2e-6 * abs(kl64), (kl, kl64)
    log.done()


# =============================================================================================================================
# 4. global average pool
# =============================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_avgpool_global_is_exact_on_small_integers(dtype):
    """got == f32(sum) * f32(1 / HW), rounded to nearest even for bf16: HW around the 32 pixel groups, C around the 64-channel slab"""
    from bayesian_torch_amd import functional as BF
    log = _Log()
    for hw in (1, 31, 32, 33, 1000):
        for C in (8, 72, 136):
            for nb in (1, 3):
                x = E.small_ints((nb, hw, C), 600 + hw + C + nb)  # [NB][HW][C]: the channels-last raster
                xd = x.permute(0, 2, 1).reshape(nb, C, hw, 1).to(dtype).to(_dev())
                got = BF.avgpool_global_hip(xd)
                assert got.shape == (nb, C) and got.dtype == dtype
                log.check("avgpool exact NB=%d HW=%d C=%d" % (nb, hw, C), _N[dtype], got, E.avgpool_exact(x, dtype), np.zeros((nb, C)))
    log.done()
