"""BTX-DROP v1 without a device: the Philox model against the published known answers, functional.dropout_mask_aten
against the numpy model bit for bit, the keep rate, the edge values, the module surface of MCDropout / Dropout /
enable_mc_dropout, the hygiene of the second export table (_lib.EXPORTS_DROP against include/btx_drop.h and the tables of
tests/test_gpu_dropout.py) and the argument errors of the two entry points (all returned before any launch)."""
import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import bayesian_torch_amd as bt
from bayesian_torch_amd import _lib, functional as BF, layers as L
from bayesian_torch_amd.models import enable_mc_dropout, get_kl_loss

import drop_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234ABCD5678EF01

KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))


@pytest.fixture(autouse=True)
def _seed():
    bt.manual_seed(SEED)
    yield


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_models_against_the_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(v) for v in DM.philox4x32_10(*ctr, *key)) == want
    assert " ".join("%08x" % int(v) for v in BF.philox4x32_10_aten(*ctr, *key)) == want


@pytest.mark.parametrize("mode", ["element", "channel"])
@pytest.mark.parametrize("shape", [(3, 5), (2, 3, 4, 5), (2, 7, 3), (8 * 1000 + 3,)])
def test_mask_aten_equals_the_numpy_model(shape, mode):
    if mode == "channel" and len(shape) < 3:
        with pytest.raises(_lib.BtxError):
            BF.dropout_mask_aten(shape, 32768, mode, SEED, 5, 9)
        return
    for T in (32768, 58982, 1, 65536, 0):
        got = BF.dropout_mask_aten(shape, T, mode, SEED, 5, 9)
        want = DM.mask(shape, mode, T, SEED, 5, 9)
        assert got.dtype == torch.bool and tuple(got.shape) == shape
        assert np.array_equal(got.numpy(), want), (shape, mode, T)
    assert not np.array_equal(DM.mask(shape, mode, 32768, SEED, 5, 9), DM.mask(shape, mode, 32768, SEED, 6, 9))
    assert not np.array_equal(DM.mask(shape, mode, 32768, SEED, 5, 9), DM.mask(shape, mode, 32768, SEED, 5, 10))


def test_the_mask_belongs_to_the_logical_element_not_to_the_memory_layout():
    m = L.MCDropout(0.5)
    x = torch.randn(2, 3, 4, 5)
    xcl = x.contiguous(memory_format=torch.channels_last)
    bt.set_sample_index(m, 4)
    a = m(x)
    bt.set_sample_index(m, 4)
    b = m(xcl)
    assert torch.equal(a, b)
    keep = DM.mask((2, 3, 4, 5), "element", 32768, SEED, 4, m._btx_layer_id)
    assert np.array_equal(a.numpy(), DM.apply_f32(x.numpy(), keep, 2.0))
    # the index IS the channels-last position: element (n, c, h, w) draws bit ((n * H + h) * W + w) * C + c
    flat = DM.bits16(np.arange(120), SEED, 4, m._btx_layer_id) < 32768
    assert np.array_equal(keep, flat.reshape(2, 4, 5, 3).transpose(0, 3, 1, 2))


def test_keep_rate_over_2_pow_20_elements():
    n = 1 << 20
    counts = {}
    for p in (0.1, 0.5):
        T, _ = DM.params(p)
        q = T / 65536.0
        kept = int((DM.bits16(np.arange(n), 2024, 0, 1) < T).sum())
        sd = math.sqrt(n * q * (1.0 - q))
        assert abs(kept - n * q) <= 6.0 * sd, (p, kept, n * q, sd)
        counts[p] = kept
    other = int((DM.bits16(np.arange(n), 2024, 1, 1) < 32768).sum())
    assert other != counts[0.5] and abs(other - n * 0.5) <= 6.0 * math.sqrt(n * 0.25)


def test_threshold_and_scale_table():
    table = {0.0: (65536, 1.0), 1e-6: (65536, 1.0), 0.1: (58982, 65536.0 / 58982), 0.5: (32768, 2.0),
             1.0 - 1e-6: (0, 0.0), 1.0: (0, 0.0)}
    for p, (T, scale) in table.items():
        assert BF.dropout_params(p) == (T, float(np.float32(scale))), p
        mT, ms = DM.params(p)
        assert (mT, float(ms)) == (T, float(np.float32(scale)))
    assert BF.dropout_params(1.0 - 1.0 / 65536)[0] == 1 and BF.dropout_params(1.0 - 1.0 / 65536)[1] == 65536.0
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            BF.dropout_params(bad)
        with pytest.raises(ValueError):
            L.MCDropout(bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_edge_values(dtype):
    x = torch.randn(7, 13).to(dtype)
    x[0, 0], x[0, 1], x[0, 2] = float("inf"), -0.0, 1e-40
    ident, zero, half = L.MCDropout(0.0), L.MCDropout(1.0), L.MCDropout(0.5)
    out = ident(x)
    assert out.dtype == dtype and torch.equal(out.view(-1).view(torch.uint8), x.view(-1).view(torch.uint8))  # p = 0: the identity, bit for bit
    z = zero(x)
    assert z.dtype == dtype and not z.view(-1).view(torch.uint8).any()                       # p = 1: +0.0 everywhere
    # a dropped inf and a dropped NaN give +0.0: selection, not a multiplication by zero
    bad = torch.full((64,), float("inf"), dtype=dtype)
    bad[1::2] = float("nan")
    bt.set_sample_index(half, 2)
    got = half(bad)
    keep = torch.from_numpy(DM.mask((64,), "element", 32768, SEED, 2, half._btx_layer_id))
    assert 0 < int(keep.sum()) < 64
    assert not got[~keep].view(torch.uint8).any()
    kept_in, kept_out = bad[keep], got[keep]
    assert torch.isinf(kept_out[torch.isinf(kept_in)]).all() and torch.isnan(kept_out[torch.isnan(kept_in)]).all()


def test_module_surface():
    m = L.MCDropout(0.25)
    assert len(m.state_dict()) == 0 and list(m.parameters()) == [] and list(m.buffers()) == []
    assert not hasattr(m, "dnn_to_bnn_flag") and float(m.kl_loss()) == 0.0 and m.kl_loss().dim() == 0
    assert "p=0.25" in repr(m) and "keep=0.750000" in repr(m) and "mode=element" in repr(m) and m.keep_prob == 0.75
    assert "mode=channel" in repr(L.MCDropout2d(0.5)) and L.MCDropout1d().mode == L.MCDropout3d().mode == "channel"
    assert bt.MCDropout is L.MCDropout and bt.enable_mc_dropout is enable_mc_dropout
    x = torch.randn(16, 32)
    m.eval()
    assert not torch.equal(m(x), x)                               # always_on: eval() does not switch it off
    off = L.MCDropout(0.25, always_on=False)
    assert not torch.equal(off(x), x)
    off.eval()
    assert off(x) is x
    c = copy.deepcopy(m)
    assert c._btx_layer_id != m._btx_layer_id and c.p == m.p and c._btx_T == m._btx_T
    with pytest.raises(_lib.BtxError):
        L.MCDropout2d(0.5)(torch.randn(4, 8))                      # channel mode: rank >= 3
    assert L.MCDropout(0.5, inplace=True)(x) is not x               # accepted, runs out of place
    with pytest.raises(ValueError):
        L.MCDropout(0.5, mode="rows")


def test_reference_wrapper_returns_out_and_zero():
    d = L.Dropout(0.5)
    x = torch.randn(8, 8)
    out, kl = d((x, torch.tensor(3.0)))
    assert kl == 0 and out.shape == x.shape and not torch.equal(out, x)
    keep = torch.from_numpy(DM.mask((8, 8), "element", 32768, SEED, 0, d._btx_layer_id))
    assert torch.equal(out, torch.where(keep, x * 2.0, torch.zeros(())))
    d.eval()                                                        # the reference's wrapper is F.dropout(..., self.training)
    out, kl = d((x, 0))
    assert out is x and kl == 0


def test_enable_mc_dropout_counts_replaces_and_refuses():
    net = nn.Sequential(nn.Linear(4, 4), nn.Dropout(0.2), nn.Sequential(nn.Conv2d(1, 1, 1), nn.Dropout2d(0.3, inplace=True)),
                        nn.Dropout1d(0.4), nn.Dropout3d(0.1))
    net[1].eval()
    assert enable_mc_dropout(net) == 4
    assert type(net[1]) is L.MCDropout and type(net[2][1]) is L.MCDropout2d and type(net[3]) is L.MCDropout1d
    assert type(net[4]) is L.MCDropout3d
    assert (net[1].p, net[2][1].p, net[2][1].inplace, net[1].always_on) == (0.2, 0.3, True, True)
    assert net[1].training is False and net[3].training is True
    assert enable_mc_dropout(net) == 0
    assert len({m._btx_layer_id for m in net.modules() if hasattr(m, "_btx_layer_id")}) == 4
    net2 = nn.Sequential(nn.Dropout(0.5))
    assert enable_mc_dropout(net2, always_on=False) == 1 and net2[0].always_on is False
    bad = nn.Sequential(nn.Dropout(0.5), nn.Sequential(nn.AlphaDropout(0.5)))
    with pytest.raises(_lib.BtxError, match="1.0.*AlphaDropout"):
        enable_mc_dropout(bad)
    assert type(bad[0]) is nn.Dropout                               # refused before anything was replaced


def test_kl_loss_of_models_with_dropout():
    net = nn.Sequential(nn.Linear(6, 6), nn.ReLU(), L.MCDropout(0.5), nn.Linear(6, 2))
    assert float(get_kl_loss(net)) == 0.0
    assert get_kl_loss(nn.Sequential(nn.Linear(2, 2))) is None
    torch.manual_seed(0)
    var = L.LinearReparameterization(6, 3)
    mixed = nn.Sequential(var, L.MCDropout(0.5))
    assert torch.equal(get_kl_loss(mixed), var.kl_loss())


def test_set_sample_index_pins_the_mask():
    net = nn.Sequential(nn.Linear(9, 33), nn.ReLU(), L.MCDropout(0.5), nn.Linear(33, 4)).eval()
    x = torch.randn(5, 9)
    outs = []
    for s in (3, 3, 4):
        bt.set_sample_index(net, s)
        outs.append(net(x))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    bt.set_sample_index(net, 3)
    first, second = net(x), net(x)                                  # the index advances with every forward
    assert torch.equal(first, outs[0]) and torch.equal(second, outs[2])


@pytest.mark.parametrize("mode,shape", [("element", (6, 11)), ("element", (2, 3, 4, 5)), ("channel", (3, 5, 7))])
def test_cpu_autograd_is_the_mask_times_scale_times_dy(mode, shape):
    m = L.MCDropout(0.3, mode=mode)
    x = torch.randn(*shape, requires_grad=True)
    dy = torch.randn(*shape)
    bt.set_sample_index(m, 6)
    m(x).backward(dy)
    keep = m.materialize_mask(shape, 6)
    assert keep.dtype == torch.bool and np.array_equal(keep.numpy(), DM.mask(shape, mode, m._btx_T, SEED, 6, m._btx_layer_id))
    scale = torch.tensor(m._btx_scale, dtype=torch.float32)
    assert torch.equal(x.grad, keep.float() * (scale * dy))


def test_fuse_model_leaves_the_layer_alone_and_the_int8_conversions_refuse_it():
    from bayesian_torch_amd.models import bnn_to_qbnn, fuse_model, to_qresnet
    torch.manual_seed(0)
    net = nn.Sequential(L.LinearReparameterization(8, 8), L.MCDropout(0.5), nn.ReLU(),
                        L.LinearReparameterization(8, 8), nn.ReLU(), L.MCDropout(0.5))
    for m in net:
        if hasattr(m, "dnn_to_bnn_flag"):
            m.dnn_to_bnn_flag = True
    net.eval()
    x = torch.randn(4, 8)
    bt.set_sample_index(net, 2)
    torch.manual_seed(5)
    want = net(x)
    assert fuse_model(net) == 1                                     # layer 3 + its ReLU; nothing across the dropout behind layer 0
    assert type(net[1]) is L.MCDropout and type(net[5]) is L.MCDropout
    bt.set_sample_index(net, 2)
    torch.manual_seed(5)
    assert torch.equal(net(x), want)
    for convert in (bnn_to_qbnn, to_qresnet):
        with pytest.raises(_lib.BtxError, match="'1'.*MCDropout"):
            convert(net)
    assert type(net[0]) is L.LinearReparameterization                # refused before anything was converted


def _declared():
    src = open(os.path.join(ROOT, "include", "btx_drop.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(btx_[a-z0-9_]+)\s*\(", src)))


def test_export_hygiene_of_the_second_table():
    """the rule of tests/test_cabi.py and tests/test_poison_cpu.py for the names include/btx_drop.h adds"""
    names = _declared()
    assert names and set(names) == set(_lib.EXPORTS_DROP) and len(set(_lib.EXPORTS_DROP)) == len(_lib.EXPORTS_DROP)
    assert not set(_lib.EXPORTS_DROP) & set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.lib_path())
    lib = _lib.lib()
    for n in names:
        assert hasattr(raw, n) and getattr(lib, n).argtypes is not None, n
    assert lib.btx_abi_version() == 9 and _lib.ABI_VERSION == 9
    main = open(os.path.join(ROOT, "include", "btx.h")).read()
    assert "BTX_STREAM_DROP 7u" in main and "btx_dropout" not in main and _lib.STREAM_DROP == DM.STREAM_DROP == 7
    import test_gpu_dropout as T
    covered, host = set(T.COVERED), set(T.HOST_ONLY)
    assert not covered & host and covered | host == set(_lib.EXPORTS_DROP)
    assert host == {e for e in _lib.EXPORTS_DROP if e.endswith("_bytes")}
    for name in set(T.COVERED.values()):
        assert name.startswith("test_") and callable(getattr(T, name, None)), name
    assert any(m.name == "gpu" for m in (T.pytestmark if isinstance(T.pytestmark, list) else [T.pytestmark]))
    hdr = open(os.path.join(ROOT, "include", "btx_drop.h")).read()
    assert "BTX_DROP_CHUNK %d" % _lib.DROP_CHUNK in hdr and T.CHUNK == _lib.DROP_CHUNK


def test_argument_errors_return_before_any_launch():
    lib = _lib.lib()
    r = _lib.Rng(1, 2, 3, None)
    R = ctypes.byref(r)
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is refused on the host
    E_NULL, E_SHAPE, E_UNSUP, E_DTYPE, E_ALIGN = -1, -2, -3, -5, -6
    fwd = lib.btx_dropout_fwd
    assert fwd(None, p, 0, 2, 3, 1, 0, 0, 100, 1.0, 1, 2, R, None) == E_NULL
    assert fwd(p, None, 0, 2, 3, 1, 0, 0, 100, 1.0, 1, 2, R, None) == E_NULL
    assert fwd(p, p, 0, 2, 3, 1, 0, 0, 100, 1.0, 1, 2, None, None) == E_NULL
    assert fwd(p, p, 2, 2, 3, 1, 0, 0, 100, 1.0, 1, 2, R, None) == E_DTYPE
    assert fwd(p, p, 0, 2, 3, 1, 2, 0, 100, 1.0, 1, 2, R, None) == E_UNSUP          # unknown mode
    assert fwd(p, p, 0, 2, 3, 1, 0, 2, 100, 1.0, 1, 2, R, None) == E_UNSUP          # unknown layout
    assert fwd(p, p, 0, 2, 3, 1, 0, 0, 65537, 1.0, 1, 2, R, None) == E_SHAPE        # T > 65536
    assert fwd(p, p, 0, 0, 3, 1, 0, 0, 100, 1.0, 1, 0, R, None) == E_SHAPE
    assert fwd(p, p, 0, 2, 3, 1, 0, 0, 100, 1.0, 0, 2, R, None) == E_SHAPE
    assert fwd(p, p, 0, 2, 3, 1, 0, 0, 100, 1.0, 3, 4, R, None) == E_SHAPE          # rows: neither N nor lanes * N
    assert fwd(p, p, 0, 2, 3, 1, 0, 0, 100, 1.0, 70000, 2, R, None) == E_UNSUP
    big = (1 << 35) + 8
    assert fwd(p, p, 1, 1, big, 1, 0, 0, 100, 1.0, 1, 1, R, None) == E_UNSUP        # a lane tensor above 2^35 elements
    assert fwd(p, p, 1, 1 << 12, 1 << 12, 1 << 12, 0, 0, 100, 1.0, 1, 1 << 12, R, None) == E_UNSUP
    assert fwd(p, p, 1, 1 << 40, 1 << 40, 1 << 40, 1, 1, 100, 1.0, 1, 1 << 40, R, None) == E_UNSUP   # (no overflow on the way)
    assert fwd(ctypes.c_void_p(66), p, 0, 2, 3, 1, 0, 0, 100, 1.0, 1, 2, R, None) == E_ALIGN   # off the ELEMENT's alignment only
    bwd = lib.btx_dropout_bwd
    assert bwd(None, p, 0, 2, 3, 1, 0, 0, 100, 1.0, R, None) == E_NULL
    assert bwd(p, p, 7, 2, 3, 1, 0, 0, 100, 1.0, R, None) == E_DTYPE
    assert bwd(p, p, 0, 2, 3, 1, 5, 0, 100, 1.0, R, None) == E_UNSUP
    assert bwd(p, p, 0, 2, 3, 1, 0, 0, 1 << 17, 1.0, R, None) == E_SHAPE
    assert bwd(p, p, 0, big, 1, 1, 0, 0, 100, 1.0, R, None) == E_UNSUP
    # the Python face refuses the same things with BtxError
    with pytest.raises(_lib.BtxError):
        BF._drop_lane_rows(torch.zeros(7, 3), 3, 2)
    assert BF._drop_lane_rows(torch.zeros(6, 3), 3, 2) == (2, False) and BF._drop_lane_rows(torch.zeros(2, 3), 3, 2) == (2, True)
