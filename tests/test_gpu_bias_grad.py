"""The bias gradient with a fixed summation order (csrc/btx_biasgrad.hip, btx_bias_grad): db_mu = sum_m dy[m], db_delta = sum_m dy[m] *
s_out[m] with the hashed BTX-RNG signs the weight-gradient kernels apply to dy.

Against float64 sums of the same numbers (signs from btx_fill_sign, an independent kernel): |err[n]| <= M * 2^-24 * sum_m |dy[m][n]|,
the textbook bound of an f32 sum of M terms in any order (Higham, gamma_{M-1} <= M u).  Bit-equality: two runs, the sign tensor against
the hashed signs, the sample index in a device word against the host's.  Through the layers: the bias gradients of two backward runs are
torch.equal — what tests/test_gpu_alignment.py asks of its flat-parameter twin."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N): one part with a ragged row group, N off the 64-channel tile; several parts; more pixels than parts * 1024 would cover singly
SHAPES = [(200, 64), (37, 10), (1025, 130), (8192, 64), (140000, 24)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(kind, dy, seed=77, sample=5, layer=3, sign=None, sample_dev=None):
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    M, N = dy.shape
    act = _lib.ACT_BF16 if dy.dtype == torch.bfloat16 else _lib.ACT_F32
    dbm = torch.full((N,), float("nan"), device=dy.device)
    dbd = torch.full((N,), float("nan"), device=dy.device) if kind == _lib.KIND_FLIPOUT else None
    ws = torch.empty(int(L.btx_bias_grad_workspace_bytes(M, N)) // 4, dtype=torch.float32, device=dy.device)
    r = _lib.Rng(seed, sample, layer, sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_bias_grad(kind, dy.data_ptr(), M, N, act, dbm.data_ptr(), dbd.data_ptr() if dbd is not None else None,
                               ctypes.byref(r), sign.data_ptr() if sign is not None else None, 0, ws.data_ptr(), ws.numel() * 4,
                               torch.cuda.current_stream(dy.device).cuda_stream))
    torch.cuda.synchronize()
    return dbm, dbd


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_bias_grad_against_float64_and_bit_equalities(M, N, dtype):
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as BF
    g = torch.Generator().manual_seed(M * 131 + N)
    dy = torch.randn(M, N, generator=g).to(_dev()).to(dtype)
    sign = BF.fill_sign_hip(M * N, _dev(), 77, 5, 3, _lib.STREAM_SIGN_OUT)
    d64 = dy.double().cpu().numpy()
    s64 = sign.cpu().numpy().reshape(M, N).astype(np.float64)
    assert set(np.unique(s64)) == {-1.0, 1.0}
    bound = M * 2.0 ** -24 * np.abs(d64).sum(0)
    dbm, dbd = _run(_lib.KIND_FLIPOUT, dy)
    e_m = np.abs(dbm.double().cpu().numpy() - d64.sum(0)) / bound
    e_d = np.abs(dbd.double().cpu().numpy() - (d64 * s64).sum(0)) / bound
    print("M %d N %d %s: worst err / bound  db_mu %.3f  db_delta %.3f" % (M, N, dtype, e_m.max(), e_d.max()))
    assert e_m.max() <= 1.0 and e_d.max() <= 1.0
    again = _run(_lib.KIND_FLIPOUT, dy)
    assert torch.equal(again[0], dbm) and torch.equal(again[1], dbd)
    by_tensor = _run(_lib.KIND_FLIPOUT, dy, sign=sign)
    assert torch.equal(by_tensor[0], dbm) and torch.equal(by_tensor[1], dbd)
    word = torch.tensor([5], dtype=torch.int32, device=_dev())
    by_word = _run(_lib.KIND_FLIPOUT, dy, sample=999, sample_dev=word)
    assert torch.equal(by_word[0], dbm) and torch.equal(by_word[1], dbd)
    other = _run(_lib.KIND_FLIPOUT, dy, sample=6)
    assert torch.equal(other[0], dbm) and not torch.equal(other[1], dbd)
    rep, none = _run(_lib.KIND_REPARAM, dy)
    assert none is None and torch.equal(rep, dbm)


# plain layouts (hashed signs), a channel-padded layout (C % 8 != 0: the sign tensors) and a small-C stem (row-fused where the layer
# takes that plan: hashed signs on the padded geometry)
LAYERS = [("LinearFlipout", dict(in_features=128, out_features=64), (200, 128)),
          ("Conv2dReparameterization", dict(in_channels=32, out_channels=64, kernel_size=3), (2, 32, 10, 10)),
          ("Conv2dFlipout", dict(in_channels=16, out_channels=24, kernel_size=3, padding=1), (8, 16, 32, 32)),
          ("Conv2dFlipout", dict(in_channels=12, out_channels=24, kernel_size=3, padding=1), (4, 12, 16, 16)),
          ("Conv2dFlipout", dict(in_channels=3, out_channels=32, kernel_size=7, stride=2, padding=3), (4, 3, 32, 32))]


@pytest.mark.parametrize("cls,kw,xshape", LAYERS, ids=["%s-%s" % (c[0], "x".join(map(str, c[2]))) for c in LAYERS])
def test_layer_bias_gradients_are_bit_reproducible_and_right(cls, kw, xshape):
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    bt.manual_seed(123)
    bt.set_precision("f32")
    torch.manual_seed(0)
    layer = getattr(L, cls)(**kw).to(_dev())
    x = torch.randn(*xshape, generator=torch.Generator().manual_seed(1)).to(_dev())
    runs = []
    for _ in range(3):
        for p in layer.parameters():
            p.grad = None
        bt.set_sample_index(layer, 5)
        out = layer(x, return_kl=False)
        dy = torch.randn(*out.shape, generator=torch.Generator().manual_seed(2)).to(_dev())
        out.backward(dy)
        torch.cuda.synchronize()
        runs.append((layer.mu_bias.grad.clone(), layer.rho_bias.grad.clone()))
    for a, b in runs[1:]:
        assert torch.equal(a, runs[0][0]) and torch.equal(b, runs[0][1])
    red = tuple(i for i in range(dy.dim()) if i != 1)
    want = dy.double().sum(red)
    M = dy.numel() // dy.shape[1]
    bound = M * 2.0 ** -24 * dy.double().abs().sum(red)
    assert float(((runs[0][0].double() - want).abs() / bound).max()) <= 1.0
    # rho_bias.grad = db_delta * eps_b * sigmoid(rho_b) (Reparameterization: db_mu * ...), db_delta = sum dy * s_out with the signs and eps
    # the layer itself materialises for this sample index: the sum's bound times the factor, plus 8 * 2^-24 relative for the two
    # products and the f32 sigmoid behind it
    with torch.no_grad():
        nz = layer.materialize_noise(5, tuple(x.shape), tuple(dy.shape), x.dtype, signs=layer._family == "flipout")
        signed = dy.double() * nz["sign_out"].reshape(dy.shape).double() if layer._family == "flipout" else dy.double()
        factor = nz["eps_b"].double().reshape(-1) * torch.sigmoid(layer.rho_bias.detach().double())
    want_r = signed.sum(red) * factor
    err = (runs[0][1].double() - want_r).abs()
    lim = bound * factor.abs() + 8 * 2.0 ** -24 * want_r.abs()
    print("%s %s: rho_bias.grad worst err / bound %.3f" % (cls, xshape, float((err / lim).max())))
    assert float(want_r.abs().max()) > 0 and float((err / lim).max()) <= 1.0
