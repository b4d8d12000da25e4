"""INT8 inference on the GPU (btx_q8.hip) against the numpy model of BTX-Q8 v1 (tests/q8_model.py), bit for bit: the activation
quantize, the weight sampling pre-pass (W_i, S_n, b_i), the i8 MFMA contraction (every shape class of the kernel: K tail, ragged N
and M, padding, stride, dilation, small C), impulse probes of the operand layout, accumulator extremes, the reference fixtures,
the BTX-RNG path, graph replay and the carrier between two layers."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import q8_helpers as H
import q8_model as Q

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (in, out, batch): a K tail under 64 with ragged N and M; more than one pixel block; whole tiles
LINEAR = [(96, 24, 8), (96, 24, 70), (64, 64, 16)]
# (Cin, Cout, k, stride, padding, dilation, (B, H, W))
CONV = [(32, 16, 3, 1, 1, 1, (2, 9, 9)), (3, 16, 7, 2, 3, 1, (2, 19, 19)), (80, 40, 1, 2, 0, 1, (2, 8, 8)),
        (16, 8, 3, 1, 2, 2, (1, 11, 11))]
ZERO_POINTS = {128: 128, 0: 7, 131: 120}   # input zero point -> output zero point used with it


def _np(t):
    return t.detach().cpu().numpy()


def _unpack_W(W, n, taps, c, kernel):
    """the kernel's weight image [N][Kp] -> logical int32 [N, C, KH, KW] (Linear: [N, C]); asserts the padding is zero"""
    W = _np(W).astype(np.int32)
    cp = (c + 15) // 16 * 16
    assert W.shape == (n, (taps * cp + 63) // 64 * 64)
    body = W[:, :taps * cp].reshape(n, taps, cp)
    assert not W[:, taps * cp:].any() and not body[:, :, c:].any()
    body = body[:, :, :c]
    if kernel is None:
        return body.reshape(n, c)
    return body.reshape(n, kernel[0], kernel[1], c).transpose(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _case(kind, idx, bias):
    """float parameters, noise and input of one shape (CPU, seeded): shared by every zero point / relu variant"""
    from bayesian_torch_amd import layers as L
    g = torch.Generator().manual_seed(1000 + 10 * idx + (1 if bias else 0) + (500 if kind == "conv" else 0))
    if kind == "linear":
        fin, fout, batch = LINEAR[idx]
        layer = L.LinearReparameterization(fin, fout, bias=bias)
        x = torch.randn(batch, fin, generator=g) * 2
        geom = {}
    else:
        cin, cout, k, s, p, dl, (b, h, w) = CONV[idx]
        layer = L.Conv2dReparameterization(cin, cout, k, stride=s, padding=p, dilation=dl, bias=bias)
        x = torch.randn(b, cin, h, w, generator=g) * 2
        geom = dict(stride=s, padding=p, dilation=dl)
    mu, rho = layer._w()
    with torch.no_grad():
        mu.copy_(torch.randn(mu.shape, generator=g) * 0.2)
        rho.copy_(torch.randn(rho.shape, generator=g) * 0.5 - 2.0)
        if bias:
            layer.mu_bias.copy_(torch.randn(layer.mu_bias.shape, generator=g))
            layer.rho_bias.copy_(torch.randn(layer.rho_bias.shape, generator=g) * 0.3 - 1.0)
    eps = torch.randn(mu.shape, generator=g)
    eps_b = torch.randn(mu.shape[0], generator=g) if bias else None
    wrap = nn.Module()
    wrap.l = layer
    from bayesian_torch_amd.models import bnn_to_qbnn
    bnn_to_qbnn(wrap)
    q = wrap.l.to(DEV)
    s_mu, s_sigma = q._q8_scales
    mu_i, sigma_i = _np(q.quantized_mu_weight).astype(np.int32), _np(q.quantized_sigma_weight).astype(np.int32)
    # calibrated-style scales from the parameters' ranges (delta does not saturate, unlike the default path)
    s_eps = 6 / 255
    s_d = float(np.float32(2 * 3 * float(np.abs(sigma_i).max()) * s_sigma / 255))
    s_w = float(np.float32(2 * (float(np.abs(mu_i).max()) * s_mu + 127 * s_d) / 255))
    return dict(q=q, x=x, eps=eps, eps_b=eps_b, geom=geom, mu_i=mu_i, sigma_i=sigma_i, s_mu=s_mu, s_sigma=s_sigma,
                mu_b=_np(q.quantized_mu_bias) if bias else None, sigma_b=_np(q.quantized_sigma_bias) if bias else None,
                chain=(s_eps, s_d, s_w))


def _check_layer(kind, idx, z_x, default):
    for bias in (True, False):
        c = _case(kind, idx, bias)
        q, x = c["q"], c["x"].to(DEV)
        if default:
            s_eps, s_d, s_w = Q.default_scales(c["s_sigma"], c["s_mu"])
            s_x = s_o = 0.2 if kind == "linear" else 0.1
            z_o = 128
            q.quant_dict = None
        else:
            s_eps, s_d, s_w = c["chain"]
            s_x, z_o = 4.0 * 2 / 255 * 2, ZERO_POINTS[z_x]
            x_i = Q.quantize_input(c["x"].numpy(), s_x, z_x)
            W_m = Q.sample_weight(c["mu_i"], c["s_mu"], c["sigma_i"], c["s_sigma"], c["eps"].numpy(), s_eps, s_d, s_w)[0]
            amax = float(np.abs(Q.accumulate(x_i, z_x, W_m, **c["geom"])).max())
            s_o = float(np.float32(s_x * s_w * amax / 200))   # the largest outputs saturate on either side of every zero point
            q.quant_dict = [(s_eps, 0), (s_d, 0), (s_w, 0), (s_x, z_x), (s_o, z_o)]
        x_i = Q.quantize_input(c["x"].numpy(), s_x, z_x)
        for relu in ((False, True) if kind == "conv" else (False,)):
            if kind == "conv":
                q.relu = relu
            ref = Q.layer_forward(x_i, z_x, s_x, c["mu_i"], c["s_mu"], c["sigma_i"], c["s_sigma"], c["eps"].numpy(), c["mu_b"],
                                  c["sigma_b"], None if c["eps_b"] is None else c["eps_b"].numpy(), s_eps, s_d, s_w, s_o, z_o,
                                  relu=relu, **c["geom"])
            out, W, S, b_i = q.forward_int8(x, noise=dict(eps_w=c["eps"], eps_b=c["eps_b"]), parts=True)
            torch.cuda.synchronize()
            n, cin = c["mu_i"].shape[0], c["mu_i"].shape[1]
            kern = None if kind == "linear" else c["mu_i"].shape[2:]
            taps = 1 if kern is None else kern[0] * kern[1]
            assert np.array_equal(_unpack_W(W, n, taps, cin, kern), ref["W"]), "W_i"
            assert np.array_equal(_np(S), ref["S"]), "S_n"
            assert np.array_equal(_np(b_i), ref["b_i"]), "b_i"
            if kind == "linear":
                assert out.dtype == torch.float32
                assert np.array_equal(_np(out), Q.dequantize(ref["out"], s_o, z_o)), (z_x, bias)
            else:
                assert (out.q_scale(), out.q_zero_point()) == (s_o, z_o) and out.int_repr().is_contiguous(memory_format=torch.channels_last)
                assert np.array_equal(_np(out.int_repr()), ref["out"]), (z_x, bias, relu)
                sat = float(((ref["out"] == 0) | (ref["out"] == 255)).mean())
                assert default or relu or 0 < sat < 0.9, sat   # the case exercises the clamps without being all clamp
        q.quant_dict = None
        if kind == "conv":
            q.relu = False


@pytest.mark.parametrize("z_x", [128, 0, 131])
@pytest.mark.parametrize("idx", range(len(LINEAR)))
def test_linear_bit_equal_to_the_model(idx, z_x):
    _check_layer("linear", idx, z_x, default=False)


@pytest.mark.parametrize("z_x", [128, 0, 131])
@pytest.mark.parametrize("idx", range(len(CONV)))
def test_conv_bit_equal_to_the_model(idx, z_x):
    _check_layer("conv", idx, z_x, default=False)


@pytest.mark.parametrize("kind,idx", [("linear", 0), ("conv", 0), ("conv", 1)])
def test_default_scales_bit_equal_to_the_model(kind, idx):
    """quant_dict is None: s_eps = 6/255, s_d = s_sigma * s_eps, s_w = max(s_d, s_mu), (0.2 | 0.1, 128) in and out"""
    _check_layer(kind, idx, 128, default=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 16, 9, 9), (5, 37)])
def test_activation_quantize(shape, dtype):
    """f32 / bf16, NCHW / channels-last (and 2-D) -> uint8 channels-last, one launch; a size that is no multiple of 4"""
    from bayesian_torch_amd import q8
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(*shape, generator=g) * 8).to(dtype)
    x.view(-1)[:4] = torch.tensor([1e9, -1e9, 0.05, -0.05]).to(dtype)   # both clamps, and values that round to the zero point
    ref = Q.quantize_input(x.float().numpy(), 0.1, 131)
    forms = [x.to(DEV)]
    if len(shape) == 4:
        forms.append(x.to(DEV).contiguous(memory_format=torch.channels_last))
    for xf in forms:
        out = q8.quantize_act(xf, 0.1, 131)
        assert out.int_repr().dtype == torch.uint8 and out.shape == tuple(shape)
        if len(shape) == 4:
            assert out.int_repr().is_contiguous(memory_format=torch.channels_last)
        assert np.array_equal(_np(out.int_repr()), ref)
        assert np.array_equal(_np(out.dequantize()), Q.dequantize(ref, 0.1, 131))


def _image(W_logical, kernel):
    """logical int8 weights -> the kernel's [N][Kp] image, S_n, zero b_i (test-side packing, independent of the sampling pre-pass)"""
    W = np.asarray(W_logical, dtype=np.int8)
    n, c = W.shape[0], W.shape[1]
    taps = 1 if kernel is None else kernel[0] * kernel[1]
    cp = (c + 15) // 16 * 16
    img = np.zeros((n, (taps * cp + 63) // 64 * 64), dtype=np.int8)
    body = img[:, :taps * cp].reshape(n, taps, cp)
    body[:, :, :c] = W.reshape(n, c, taps).transpose(0, 2, 1) if kernel is not None else W.reshape(n, 1, c)
    S = W.reshape(n, -1).astype(np.int64).sum(1).astype(np.int32)
    return torch.from_numpy(img).to(DEV), torch.from_numpy(S).to(DEV), torch.zeros(n, dtype=torch.int32, device=DEV)


def test_impulse_probes_linear():
    """K = 160 (Kp = 192): one impulse pair (x[m][k], W[n][k]) for every k in 0..63 and 64, 127, 128, 159, each in its own row m
    and its own (permuted, so not symmetric) column n.  Distinct k never meet, so out = z_o + diag-like pattern, exactly: a wrong
    MFMA operand lane map or k order moves or loses a product."""
    from bayesian_torch_amd import q8
    ks = list(range(64)) + [64, 127, 128, 159]
    J, K, z_x, z_o = len(ks), 160, 131, 100
    x = np.full((J, K), z_x, dtype=np.uint8)
    W = np.zeros((J, K), dtype=np.int8)
    exp = np.full((J, J), z_o, dtype=np.int32)
    for j, k in enumerate(ks):
        dx, w, n = (j % 5) + 1, ((j % 7) + 1) * (1 if j % 2 else -1), (7 * j + 3) % J
        x[j, k] = z_x + dx
        W[n, k] = w
        exp[j, n] = z_o + dx * w
    assert exp.min() >= 0 and (exp != exp.T).any()
    img, S, b0 = _image(W, None)
    out = q8.contract(torch.from_numpy(x).to(DEV), z_x, img, S, b0, J, (1, 1), (1, 1), (0, 0), (1, 1), 1.0, z_o, False, False, 1.0)
    assert np.array_equal(_np(out).astype(np.int32), exp)
    assert np.array_equal(exp.astype(np.uint8), Q.requantize(Q.accumulate(x, z_x, W), np.zeros(J), 1.0, 1.0, 1.0, z_o))


def test_impulse_probes_conv3x3():
    """3x3, pad 1, C = 32: for every tap one input impulse and one weight impulse, tap t on its own channel and output channel;
    the expected output (the model's) has exactly one non-zero product per tap, at the pixel that tap reaches"""
    from bayesian_torch_amd import q8
    C, N, Hh, z_x, z_o = 32, 12, 6, 0, 100
    x = np.full((1, C, Hh, Hh), z_x, dtype=np.uint8)
    W = np.zeros((N, C, 3, 3), dtype=np.int8)
    for t in range(9):
        kh, kw = divmod(t, 3)
        x[0, 3 * t + 1, (2 * t) % Hh, (t + 3) % Hh] = z_x + t + 2
        W[t + 2, 3 * t + 1, kh, kw] = (t + 1) * (-1 if t % 2 else 1)
    acc = Q.accumulate(x, z_x, W, 1, 1, 1)
    assert int((acc != 0).sum()) >= 7   # an impulse next to the border can fall off the image for its tap, the rest must land
    exp = Q.requantize(acc, np.zeros(N), 1.0, 1.0, 1.0, z_o)
    img, S, b0 = _image(W, (3, 3))
    xq = torch.from_numpy(x).to(DEV).contiguous(memory_format=torch.channels_last)
    out = q8.contract(xq, z_x, img, S, b0, N, (3, 3), (1, 1), (1, 1), (1, 1), 1.0, z_o, False, False, 1.0)
    assert np.array_equal(_np(out), exp)


@pytest.mark.parametrize("xv,wv,z_x", [(0, -128, 128), (255, 127, 0), (0, 127, 128), (255, -128, 0)])
def test_extremes_accumulator_and_saturation(xv, wv, z_x):
    """Linear K = 4608: the largest accumulators of either sign are exact (cancelled to a small value by b_i, multiplier 1), and
    without the cancellation they saturate to 255 / 0"""
    from bayesian_torch_amd import q8
    K, N, B, z_o = 4608, 8, 4, 50
    acc = (xv - z_x) * wv * K
    x = torch.full((B, K), xv, dtype=torch.uint8, device=DEV)
    img, S, b0 = _image(np.full((N, K), wv, dtype=np.int8), None)
    assert int(S[0]) == wv * K
    b = torch.arange(N, dtype=torch.int32, device=DEV) - acc        # acc + b_i = n, exactly, only if acc is exact
    out = q8.contract(x, z_x, img, S, b, N, (1, 1), (1, 1), (0, 0), (1, 1), 1.0, z_o, False, False, 1.0)
    assert np.array_equal(_np(out).astype(np.int32), np.tile(z_o + np.arange(N), (B, 1)))
    out = q8.contract(x, z_x, img, S, b0, N, (1, 1), (1, 1), (0, 0), (1, 1), 1.0, z_o, False, False, 1.0)
    assert (_np(out) == (255 if acc > 0 else 0)).all()
    outf = q8.contract(x, z_x, img, S, b0, N, (1, 1), (1, 1), (0, 0), (1, 1), 1.0, z_o, False, True, 0.5)
    assert (_np(outf) == np.float32(((255 if acc > 0 else 0) - z_o) * 0.5)).all()


RECORDS = [(n, "") for n in H.SINGLE] + [("q8_calibrated", "conv_"), ("q8_calibrated", "fc_")]


@pytest.mark.parametrize("name,prefix", RECORDS)
def test_reference_fixtures(name, prefix):
    """the reference's recorded noise through the GPU layers: the model's bits, hence the reference within 1 LSB / 0.5 %"""
    d = H.sub(H.fixture(name), prefix) if prefix else H.fixture(name)
    conv = d["ref_W"].ndim == 4
    dd = dict(d, kind=np.int64(1 if conv else 0))
    q = H.quantized_layer(dd, DEV)
    if int(d["calibrated"]):
        q.quant_dict = H.quant_dict_of(d)
    x = torch.from_numpy(d["x"]).to(DEV)
    noise = dict(eps_w=torch.from_numpy(d["eps"]), eps_b=torch.from_numpy(d["eps_b"]))
    out, W, S, b_i = q.forward_int8(x, noise=noise, parts=True)
    kern = d["ref_W"].shape[2:] if conv else None
    assert np.array_equal(_unpack_W(W, d["ref_W"].shape[0], 9 if conv else 1, d["ref_W"].shape[1], kern), d["ref_W"].astype(np.int32))
    m = H.model_record(d)
    if conv:
        out_i = _np(out.int_repr())
    else:
        assert np.array_equal(_np(out), Q.dequantize(m["out"], float(d["s_o"]), int(d["z_o"])))
        out_i = np.rint(_np(out) / np.float32(d["s_o"])).astype(np.int32) + int(d["z_o"])
    assert np.array_equal(out_i, m["out"])
    H.assert_close_to_reference(out_i, d, name + prefix + " (GPU)")


@pytest.mark.parametrize("kind,idx", [("linear", 0), ("conv", 0), ("conv", 1)])
def test_rng_path_draws_the_float_layers_noise(kind, idx):
    """no injected noise == eps of the SOURCE float layer's materialize_noise at that sample index (the twin keeps the layer id);
    the same index twice gives the same bits, two indices differ"""
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn
    bt.manual_seed(77)
    torch.manual_seed(5)
    if kind == "linear":
        fin, fout, batch = LINEAR[idx]
        src = L.LinearReparameterization(fin, fout)
        x = torch.randn(batch, fin) * 2
    else:
        cin, cout, k, s, p, dl, (b, h, w) = CONV[idx]
        src = L.Conv2dReparameterization(cin, cout, k, stride=s, padding=p, dilation=dl)
        x = torch.randn(b, cin, h, w) * 2
    src = src.to(DEV)
    x = x.to(DEV)
    wrap = nn.Module()
    wrap.l = src
    bnn_to_qbnn(wrap)
    q = wrap.l
    assert q._btx_layer_id == src._btx_layer_id

    def bits(o):
        return _np(o.int_repr() if kind == "conv" else o)
    for s_idx in (0, 3):
        noise = src.materialize_noise(s_idx)
        a = q.forward_int8(x, sample_idx=s_idx, parts=True)
        b = q.forward_int8(x, noise=noise, sample_idx=s_idx, parts=True)
        for u, v in zip(a[1:], b[1:]):
            assert torch.equal(u, v)
        assert np.array_equal(bits(a[0]), bits(b[0]))
    bt.set_sample_index(wrap, 3)
    o3 = bits(q(x)[0])
    bt.set_sample_index(wrap, 3)
    assert np.array_equal(o3, bits(q(x)[0])) and np.array_equal(o3, bits(a[0]))
    bt.set_sample_index(wrap, 4)
    assert not np.array_equal(o3, bits(q(x)[0]))
    assert q._btx_sample == 5   # the counter advances like the float layer's


class Chain(nn.Module):
    """conv (ReLU folded) -> conv -> flatten -> Linear, quantized activations travelling in the carrier"""

    def __init__(self):
        super().__init__()
        from bayesian_torch_amd import layers as L
        self.c1 = L.Conv2dReparameterization(8, 16, 3, padding=1)
        self.c2 = L.Conv2dReparameterization(16, 12, 3, stride=2, padding=1, bias=False)
        self.fc = L.LinearReparameterization(12 * 4 * 4, 10)

    def forward(self, x):
        x = self.c1(x)[0]
        x = self.c2(x)[0]
        return self.fc(x.flatten(1))[0]


def _chain():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd.models import bnn_to_qbnn
    bt.manual_seed(11)
    torch.manual_seed(2)
    m = Chain().to(DEV).eval()
    src = (m.c1, m.c2, m.fc)
    bnn_to_qbnn(m)
    m.c1.relu = True
    x = (torch.randn(3, 8, 8, 8) * 2).to(DEV)
    return m, src, x


def test_two_convs_and_a_linear_through_the_carrier_equal_the_chained_model():
    m, src, x = _chain()
    s_idx = 2
    import bayesian_torch_amd as bt
    bt.set_sample_index(m, s_idx)
    with torch.no_grad():
        y = m(x)
    cur, z, s = Q.quantize_input(_np(x), 0.1, 128), 128, 0.1
    for q, f, relu, (s_o, z_o) in ((m.c1, src[0], True, (0.1, 128)), (m.c2, src[1], False, (0.1, 128)), (m.fc, src[2], False, (0.2, 128))):
        nz = f.materialize_noise(s_idx)
        s_eps, s_d, s_w = Q.default_scales(q._q8_scales[1], q._q8_scales[0])
        conv = q._nd == 2
        if not conv:
            cur = cur.reshape(cur.shape[0], -1)
        r = Q.layer_forward(cur, z, s, _np(q.quantized_mu_weight).astype(np.int32), q._q8_scales[0],
                            _np(q.quantized_sigma_weight).astype(np.int32), q._q8_scales[1], _np(nz["eps_w"]),
                            _np(q.quantized_mu_bias) if q.bias else None, _np(q.quantized_sigma_bias) if q.bias else None,
                            _np(nz["eps_b"]) if q.bias else None, s_eps, s_d, s_w, s_o, z_o, relu=relu,
                            **(dict(stride=_p(q.stride), padding=_p(q.padding), dilation=_p(q.dilation)) if conv else {}))
        cur, z, s = r["out"], z_o, s_o
    assert np.array_equal(_np(y), Q.dequantize(cur, 0.2, 128))


def _p(v):
    return v if isinstance(v, int) else tuple(v)


def test_graphed_mc_replays_equal_eager_forwards_and_lanes_are_refused():
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import mc
    from bayesian_torch_amd._lib import BtxError
    m, _, x = _chain()
    eager = {}
    with torch.no_grad():
        for s in (5, 0, 9):
            bt.set_sample_index(m, s)
            eager[s] = m(x).clone()
    assert not torch.equal(eager[5], eager[9])
    g = mc.GraphedMC(m, x, lanes=1, keep_logits=True)
    try:
        for s in (5, 0, 9):
            g.run(s)
            torch.cuda.synchronize()
            assert torch.equal(g.lane_logits[0], eager[s]), s
    finally:
        g.close()
    packed = mc.mc_forward(m, x, 3, lanes=1)
    assert torch.isfinite(packed).all()
    with pytest.raises(BtxError, match="lanes"):
        mc.mc_forward(m, x, 4, lanes=2)
    with pytest.raises(BtxError, match="lanes"):
        mc.GraphedMC(m, x, lanes=2)
    with torch.no_grad():
        bt.set_sample_index(m, 5)
        assert torch.equal(m(x), eager[5])   # the refusals left no lane state behind
