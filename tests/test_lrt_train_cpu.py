"""Fused training of the local reparameterization layers (DESIGN.md §21 "Backward"), the part that needs no GPU: the C-ABI's exports
and refusals, the opt-in switch, and the float64 model of the backward (tests/lrt_bwd_model.py) against torch's float64 autograd of
the composite, with perturbed references that must fall outside the bounds."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import envelope as E  # noqa: E402
import lrt_bwd_model as BM  # noqa: E402
import lrt_model as LM  # noqa: E402

E_NULL, E_SHAPE, E_UNSUPPORTED, E_WORKSPACE, E_DTYPE = -1, -2, -3, -4, -5
FAKE = 0x10000  # a non-NULL pointer that is never dereferenced: every call below returns before anything is launched


def _geom(NB=4, H=5, W=5, C=8, N=16, k=3, s=1, p=1, d=1, groups=1, D=1, KD=1):
    from bayesian_torch_amd import _lib
    g = _lib.Geom()
    g.NB, g.D, g.H, g.W, g.C, g.N = NB, D, H, W, C, N
    g.KD, g.KH, g.KW = KD, k, k
    g.sd, g.sh, g.sw = 1, s, s
    g.pd, g.ph, g.pw = 0, p, p
    g.dd, g.dh, g.dw = 1, d, d
    g.groups = groups
    return g


def _ws_bytes(g, act=0, prec=0):
    from bayesian_torch_amd import _lib
    need = ctypes.c_size_t(0)
    rc = _lib.lib().btx_lrt_bwd_workspace_bytes(ctypes.byref(g) if g is not None else None, act, prec, ctypes.byref(need))
    return rc, int(need.value)


def _bwd(g, x=FAKE, dy=FAKE, root=FAKE, mu=FAKE, rho=FAKE, rho_b=FAKE, grads=True, rng=True, act=0, prec=0, ws=FAKE, ws_bytes=1 << 40):
    from bayesian_torch_amd import _lib
    gr = _lib.LrtGrads(FAKE, FAKE, FAKE, FAKE, FAKE)
    r = _lib.Rng(1, 2, 3, None)
    return _lib.lib().btx_lrt_bwd(ctypes.byref(g) if g is not None else None, x, dy, root, mu, rho, rho_b,
                                  ctypes.byref(gr) if grads else None, ctypes.byref(r) if rng else None, act, prec, ws, ws_bytes, None)


def test_exports_exist_and_the_abi_stays_9():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9 and _lib.ABI_VERSION == 9
    hdr = open(os.path.join(HERE, "..", "include", "btx.h")).read()
    assert "#define BTX_ABI_VERSION 9" in hdr
    for n in ("btx_lrt_fwd_train", "btx_lrt_bwd_workspace_bytes", "btx_lrt_bwd"):
        assert n + "(" in hdr and n in _lib.EXPORTS and hasattr(L, n)
    assert "BtxLrtGrads" in hdr


def test_argument_errors_return_their_code_without_a_device():
    from bayesian_torch_amd import _lib
    g = _geom()
    rc, need = _ws_bytes(g)
    assert rc == 0 and need > 0
    # NULL
    assert _ws_bytes(None)[0] == E_NULL
    assert _lib.lib().btx_lrt_bwd_workspace_bytes(ctypes.byref(g), 0, 0, None) == E_NULL
    for kw in (dict(x=None), dict(dy=None), dict(root=None), dict(mu=None), dict(rho=None), dict(grads=False), dict(rng=False),
               dict(rho_b=None)):  # (rho_b: drho_b is asked for)
        assert _bwd(g, **kw) == E_NULL, kw
    assert _bwd(None) == E_NULL
    # SHAPE
    for bad in (_geom(NB=0), _geom(C=0), _geom(H=1, W=1, k=3, p=0), _geom(s=0)):
        assert _ws_bytes(bad)[0] == E_SHAPE and _bwd(bad) == E_SHAPE
    # DTYPE
    assert _ws_bytes(g, act=7)[0] == E_DTYPE and _bwd(g, act=7) == E_DTYPE
    assert _ws_bytes(g, prec=9)[0] == E_DTYPE and _bwd(g, prec=9) == E_DTYPE
    # WORKSPACE
    assert _bwd(g, ws=None) == E_WORKSPACE
    assert _bwd(g, ws_bytes=need - 1) == E_WORKSPACE
    # the training forward: the same order of checks
    L = _lib.lib()
    r = _lib.Rng(1, 2, 3, None)
    fwd = lambda **kw: L.btx_lrt_fwd_train(ctypes.byref(kw.get("g", g)), kw.get("x", FAKE), FAKE, FAKE, kw.get("mu_b", None),  # noqa: E731
                                           None, FAKE, kw.get("root", FAKE), ctypes.byref(r), kw.get("act", 0), kw.get("prec", 0),
                                           kw.get("flags", 0), None)
    assert fwd(x=None) == E_NULL and fwd(root=None) == E_NULL and fwd(mu_b=FAKE) == E_NULL  # (mu_b without rho_b)
    assert fwd(act=5) == E_DTYPE and fwd(prec=5) == E_DTYPE
    assert fwd(g=_geom(NB=0)) == E_SHAPE
    assert fwd(prec=2) == E_UNSUPPORTED                              # bf16x3 stays refused
    assert fwd(flags=_lib.FLAG_TRANSPOSED) == E_UNSUPPORTED and fwd(flags=_lib.FLAG_ROWFUSE) == E_UNSUPPORTED


def test_uncovered_geometries_are_unsupported_before_any_launch():
    covered = (_geom(), _geom(H=13, W=13, C=16, N=72, s=2), _geom(NB=37, H=1, W=1, C=72, N=50, k=1, p=0), _geom(p=2, k=3),
               _geom(d=2, p=4), _geom(C=3, N=16, H=7, W=7))
    for g in covered:
        for act, prec in ((0, 0), (0, 1), (1, 1)):
            rc, need = _ws_bytes(g, act, prec)
            assert rc == 0 and need > 0
    uncovered = (_geom(groups=2), _geom(D=3, KD=3), _geom(D=2), _geom(p=3, k=3), _geom(k=1, p=1))
    for g in uncovered:
        assert _ws_bytes(g)[0] == E_UNSUPPORTED and _bwd(g) == E_UNSUPPORTED
    assert _ws_bytes(_geom(), 0, 2)[0] == E_UNSUPPORTED and _bwd(_geom(), prec=2) == E_UNSUPPORTED   # bf16x3


def test_switch_defaults_off_and_fuse_model_sets_it_on_lrt_layers_only():
    from bayesian_torch_amd import layers as L, functional as BF
    from bayesian_torch_amd.models import fuse_model
    torch.manual_seed(0)
    net = torch.nn.Sequential(L.Conv2dLocalReparameterization(8, 8, 3, padding=1), L.Conv2dReparameterization(8, 8, 3, padding=1),
                              torch.nn.Flatten(), L.LinearLocalReparameterization(8 * 4 * 4, 6), L.LinearFlipout(6, 3))
    for m in net:
        if hasattr(m, "_btx_layer_id"):
            m.dnn_to_bnn_flag = True
            assert m.fused_training is False
    fuse_model(net)
    assert not any(getattr(m, "fused_training", False) for m in net)
    fuse_model(net, lrt_training=True)   # a second call still switches
    assert net[0].fused_training is True and net[3].fused_training is True
    assert net[1].fused_training is False and net[4].fused_training is False
    # a CPU call never takes the fused path, whatever the switch says
    x = torch.randn(2, 8, 4, 4, requires_grad=True)
    assert not BF.lrt_train_ok(net[0], x)
    net[1].fused_training = True         # not an LRT layer: the switch means nothing there
    assert not BF.lrt_train_ok(net[1], x)


def test_cpu_forwards_and_gradients_are_unchanged_by_the_switch():
    from bayesian_torch_amd import layers as L
    res = []
    for on in (False, True):
        torch.manual_seed(3)
        layer = L.Conv2dLocalReparameterization(4, 6, 3, padding=1)
        layer.fused_training = on
        x = torch.randn(2, 4, 5, 5, requires_grad=True)
        torch.manual_seed(11)
        out, kl = layer(x)
        (out.square().sum() + kl).backward()
        res.append((out.detach(), x.grad, layer.mu_kernel.grad, layer.rho_kernel.grad, layer.rho_bias.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


CASES = {
    "linear": (dict(kind="linear"), (37, 72), (50, 72), True),
    "conv_s1": (dict(kind="conv", nd=2, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1), (4, 8, 5, 5), (16, 8, 3, 3), True),
    "conv_s2": (dict(kind="conv", nd=2, stride=(2, 2), padding=(1, 1), dilation=(1, 1), groups=1), (2, 16, 13, 13), (72, 16, 3, 3), True),
    "conv_nobias": (dict(kind="conv", nd=2, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1), (2, 8, 5, 5), (16, 8, 3, 3), False),
}


def _case(name, seed=0):
    op, xs, ws, bias = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(xs, generator=g).numpy()
    mu = (0.1 * torch.randn(ws, generator=g)).numpy()
    rho = (torch.rand(ws, generator=g) * 3.0 - 4.0).numpy()
    mb = (0.1 * torch.randn(ws[0], generator=g)).numpy() if bias else None
    # sigma_b in [0.31, 0.69]: sigma_b^2 is then a visible share (several per cent) of every variance sum, also at K = 144
    rb = (torch.rand(ws[0], generator=g) - 1.0).numpy() if bias else None
    out = E.contract(torch.from_numpy(x).double(), torch.from_numpy(mu).double(), None, op)
    gy = torch.randn(out.shape, generator=g).numpy()
    zeta = torch.randn(out.shape, generator=g).numpy()
    return op, x, gy, zeta, mu, rho, mb, rb


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_float64_autograd_of_the_composite(name):
    op, x, gy, zeta, mu, rho, mb, rb = _case(name)
    want = BM.composite_autograd64(x, gy, zeta, mu, rho, mb, rb, op)
    ex = BM.backward(x, gy, zeta, mu, rho, mb, rb, op, exact=True)
    for q, w in want.items():
        assert np.abs(w).max() > 0
        np.testing.assert_allclose(ex["ref"][q], w, rtol=1e-11, atol=1e-13 * np.abs(w).max())
    # the rounded models stay inside their own bounds of the unrounded definition, plus what the operand roundings themselves move
    # (f32: x^2 and sigma one rounding each — inside op_s and e_gv; bf16: u on every operand of the data gradient)
    for prec, abf in (("f32", False),):
        r = BM.backward(x, gy, zeta, mu, rho, mb, rb, op, prec=prec, act_bf16=abf)
        for q, w in want.items():
            rep = E.check(w, r["ref"][q], r["bound"][q])
            assert rep.ok, (name, q, str(rep))


@pytest.mark.parametrize("prec,abf", [("f32", False), ("bf16", False), ("bf16", True)], ids=["f32-f32", "bf16-f32", "bf16-bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_perturbed_references_fall_outside_the_bounds(name, prec, abf):
    op, x, gy, zeta, mu, rho, mb, rb = _case(name, seed=1)
    if abf:
        x, gy = LM.rbf16(x), LM.rbf16(gy)
    r = BM.backward(x, gy, zeta, mu, rho, mb, rb, op, prec=prec, act_bf16=abf)
    ref, bnd = r["ref"], r["bound"]
    for q in ref:
        assert np.isfinite(ref[q]).all() and np.isfinite(bnd[q]).all() and np.abs(ref[q]).max() > 0
        assert E.check(ref[q], ref[q], bnd[q]).ok
    assert not E.check(np.zeros_like(ref["rho"]), ref["rho"], bnd["rho"]).ok          # the bound sees the noise path
    # a missing factor 2 in dx
    half = BM.backward(x, gy, zeta, mu, rho, mb, rb, op, prec=prec, act_bf16=abf, dx_factor=1.0)
    assert not E.check(half["ref"]["x"], ref["x"], bnd["x"]).ok
    # zeta shifted by one index (of the channels-last tensor the kernel indexes)
    zc = np.moveaxis(zeta, 1, -1) if zeta.ndim > 2 else zeta
    zs = np.roll(zc.reshape(-1), 1).reshape(zc.shape)
    zs = np.moveaxis(zs, -1, 1) if zeta.ndim > 2 else zs
    sh = BM.backward(x, gy, zs, mu, rho, mb, rb, op, prec=prec, act_bf16=abf)
    for q in ("rho", "x") + (("rho_b",) if mb is not None else ()):
        assert not E.check(sh["ref"][q], ref[q], bnd[q]).ok, q
    # sigma_b^2 dropped under the root
    if mb is not None:
        dr = BM.backward(x, gy, zeta, mu, rho, mb, rb, op, prec=prec, act_bf16=abf, drop_bias_var=True)
        for q in ("rho", "rho_b", "x"):
            assert not E.check(dr["ref"][q], ref[q], bnd[q]).ok, q


def test_removed_guard_gives_nan_and_the_guarded_model_does_not():
    op, x, gy, zeta, mu, rho, mb, rb = _case("conv_nobias", seed=2)
    x[0] = 0.0                                                      # image 0: v == 0 at every output position
    r = BM.backward(x, gy, zeta, mu, rho, None, None, op)
    assert all(np.isfinite(v).all() for v in r["ref"].values()) and (r["root"][0] == 0).all()
    want = BM.composite_autograd64(x, gy, zeta, mu, rho, None, None, op)
    np.testing.assert_allclose(BM.backward(x, gy, zeta, mu, rho, None, None, op, exact=True)["ref"]["rho"], want["rho"], rtol=1e-11)
    with np.errstate(all="ignore"):
        bad = BM.backward(x, gy, zeta, mu, rho, None, None, op, guard=False)
    assert np.isnan(bad["ref"]["rho"]).any()
    assert not E.check(bad["ref"]["rho"], r["ref"]["rho"], r["bound"]["rho"]).ok
    # all-zero input: drho is exactly 0 with a zero bound, and dx is the mean path alone
    z = BM.backward(np.zeros_like(x), gy, zeta, mu, rho, None, None, op)
    assert (z["ref"]["rho"] == 0).all() and (z["bound"]["rho"] == 0).all()
    a_only = BM._dgrad64(BM._t(gy), x.shape, BM._t(mu), op).numpy()
    assert np.array_equal(z["ref"]["x"], a_only)
