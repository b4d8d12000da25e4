"""GPU: every element of the fused Bayesian LSTM kernels (btx_lstm.hip, btx_lstm_bwd.hip) against float64, one step at a time.

The references of test_gpu_lstm_fused.py / test_gpu_lstm_train_fused.py re-derive the whole chain and can only hold a rel-L2
bar (1e-2 / 2e-2 in bf16).  Here each step is judged alone (envelope.py, LSTM section): the float64 reference of step t gets the
GPU's own operands — the weights the kernel sampled for itself, read back by identity-impulse probes; its own hidden_seq[:, t-1];
its own saved f32 gates and cell states — so what is left is accumulation order and the device's expf / tanhf, in f32 and bf16
alike, and every element is compared (no percentile, no mean, nothing excluded).

  1. probes     x = I (resp. h0 = I) in f32 makes every gate pre-activation one product: the launch hands back W_ih(s+t) and
                W_hh(s+t); zero inputs hand back the biases.  Against float64 softplus(rho) * eps with eps / signs from
                materialize_noise(s + t): pins eps_w element n*Kr + k, eps_b element n, s_in, s_out and the index s + t.
  2. gates      saved pre-activations, all (t, b, n): |got - ref| <= (K_i + K_h + 8) 2^-23 A.
  3. cell       saved f32 c_t, c_seq, hidden_seq from the saved gates and the saved c_{t-1}; the inference kernel (lstm_hip)
                returns the same bits; `saved` is compared in full (the API allocates it: tests/test_gpu_poison.py::test_lstm
                runs CASES[0..2] with that allocation, and the workspace, pre-filled with 0xFF and 0x7F bytes).
  4. exact      rho = -200 (sigma = 0 exactly), small integers: the gates are integers and equal float64; drho == 0.
  5. backward   dx, dh0, dc0 and the eight parameter gradients against float64 BPTT from the saved buffers; the bound is the
                propagated first-order error (envelope.Err), nothing fitted.
  6. paths that never ran: bf16 activations through the layers (fused_training) and the selective-gradient launches.

Shapes: the smallest that reach every edge of the tilings (forward 4 units x 64 rows x 64-wide K chunks, 16 k per wave, sampler
groups of 4; backward 16 columns x 64 gate rows; weight gradient 16 x 64 tiles, 64-row batch chunks) — see CASES.
profiles/lstm_envelope.txt holds the measured figures.
"""
import itertools

import numpy as np
import pytest
import torch

import envelope as E

pytestmark = pytest.mark.gpu

CASES = [  # (I, H, B, T)
    (7, 5, 1, 1),      # K % 8 != 0 (Kr != K), K % 4 != 0 sampler tail, last hidden block 1 of 4 units, 4H = 20 < a gate chunk, one row
    (8, 16, 3, 2),     # everything aligned; the recurrent term dgates_{t+1} . W_hh(s+t+1) and the dcc carry
    (65, 17, 65, 2),   # 2nd K chunk / batch block / backward column block with one element, 4H = 68: 2nd gate chunk of 4 rows,
                       # 5 weight-gradient row tiles (last: 4 rows), 2 column tiles, 2 batch chunks
    (17, 66, 5, 3),    # recurrent K = 66 crosses the chunk, Hr = 72; 3 steps
    (12, 10, 4, 3),    # the smallest case of the existing tests
]
FAMILIES = ["LSTMReparameterization", "LSTMFlipout"]
S0 = 5          # sample index of step 0: s + t is never trivially 0
SEED = 90210
GATE_RANGE = 40.0  # SIGM_ULP / TANH_ULP are measured on [-GATE_RANGE, GATE_RANGE]; the cases' gates must stay inside
CONFIGS = [(p, a, b, s) for p in ("f32", "bf16") for a in ("f32", "bf16") for b, s in ((True, True), (True, False), (False, True), (False, False))]
_ids = dict(ids=lambda v: v if isinstance(v, str) else "I%d-H%d-B%d-T%d" % v)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _adt(act):
    return torch.bfloat16 if act == "bf16" else torch.float32


def _saved_views(saved, T, B, H):
    """(gates [T, B, 4H], cells [T, B, H]) of btx_lstm_fwd_train's buffer, and the words in between"""
    f = saved.view(torch.float32)
    ng = T * B * 4 * H
    off = (ng * 4 + 255) // 256 * 256 // 4
    return f[:ng].reshape(T, B, 4 * H), f[off:off + T * B * H].reshape(T, B, H)


class Ctx:
    pass


_CTX, _RUNS, _REPORTS = {}, {}, {}


def _params(lin, s, bias, zero_mu=False, zero_mu_b=False):
    mu, rho = (t.detach() for t in lin._w())
    mu_b = rho_b = None
    if bias:
        mu_b, rho_b = lin.mu_bias.detach(), lin.rho_bias.detach()
        if zero_mu_b:
            mu_b = torch.zeros_like(mu_b)
    if zero_mu:
        mu = torch.zeros_like(mu)
    return (mu, rho, mu_b, rho_b, lin._btx_layer_id, s, None)


def _ctx(cls, case):
    """layer, inputs and the probed per-step weights of one (family, case); built once and shared"""
    key = (cls, case)
    if key in _CTX:
        return _CTX[key]
    import bayesian_torch_amd as bt
    from bayesian_torch_amd import _lib, functional as BF, layers as L, rng
    dev = _dev()
    bt.manual_seed(SEED)
    bt.set_precision("f32")
    I, H, B, T = case
    c = Ctx()
    c.case, c.flip = case, cls == "LSTMFlipout"
    c.kind = _lib.KIND_FLIPOUT if c.flip else _lib.KIND_REPARAM
    # (a case of another file — tests/test_gpu_autograd_contract.py brings its own shape — takes the slot behind the last one)
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(cls) + (CASES.index(case) if case in CASES else len(CASES)))
    c.layer = getattr(L, cls)(I, H, bias=True).to(dev)
    bt.assign_layer_ids(c.layer, start=900)
    with torch.no_grad():
        for lin in (c.layer.ih, c.layer.hh):
            for p, lo, hi in ((lin.mu_weight, None, None), (lin.rho_weight, -9.0, 2.0), (lin.mu_bias, None, None), (lin.rho_bias, -9.0, 2.0)):
                if lo is None:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))
                else:  # the rho range of profiles/elementwise_envelope.txt
                    p.copy_(torch.rand(p.shape, generator=g) * (hi - lo) + lo)
    c.seed = rng.seed()
    # small activations keep the gates moderate: a saturated gate's derivative is a cancellation (1 - i) the bound cannot resolve
    c.x = (0.25 * torch.randn(B, T, I, generator=g)).to(dev)
    c.h0, c.c0 = (0.5 * torch.randn(B, H, generator=g)).to(dev), torch.randn(B, H, generator=g).to(dev)
    c.r_h, c.r_c = torch.randn(B, T, H, generator=g).to(dev), torch.randn(B, T, H, generator=g).to(dev)

    # ---- probes: T = 1, f32, sample index s + t
    ih, hh = c.layer.ih, c.layer.hh
    eyeI = torch.eye(I, device=dev).reshape(I, 1, I)
    eyeH = torch.eye(H, device=dev)
    c.steps = {"ih": [], "hh": []}      # per step: dict(W | D, b | db, eps_w, eps_b, s_in, s_out) float64 numpy
    for t in range(T):
        s = S0 + t
        pw = lambda lin, **kw: _params(lin, s, **kw)  # noqa: E731
        # W_ih: B = I rows, x = I, no state, no biases
        _, _, _, sv = BF.lstm_train_fwd_hip(c.kind, eyeI, pw(ih, bias=False, zero_mu=c.flip), pw(hh, bias=False, zero_mu=c.flip),
                                            c.seed, prec="f32")
        gi = _saved_views(sv, 1, I, H)[0][0].double().cpu().numpy()          # [k, n]
        # W_hh: x = 0, h0 = I, c0 = 0
        _, _, _, sv = BF.lstm_train_fwd_hip(c.kind, torch.zeros(H, 1, I, device=dev), pw(ih, bias=False, zero_mu=c.flip),
                                            pw(hh, bias=False, zero_mu=c.flip), c.seed, prec="f32", h0=eyeH, c0=torch.zeros_like(eyeH))
        gh = _saved_views(sv, 1, H, H)[0][0].double().cpu().numpy()
        # biases: zero input, one layer with bias, the other without
        z1 = torch.zeros(1, 1, I, device=dev)
        _, _, _, sv = BF.lstm_train_fwd_hip(c.kind, z1, pw(ih, bias=True, zero_mu_b=c.flip), pw(hh, bias=False), c.seed, prec="f32")
        bi = _saved_views(sv, 1, 1, H)[0][0, 0].double().cpu().numpy()
        _, _, _, sv = BF.lstm_train_fwd_hip(c.kind, z1, pw(ih, bias=False), pw(hh, bias=True, zero_mu_b=c.flip), c.seed, prec="f32")
        bh = _saved_views(sv, 1, 1, H)[0][0, 0].double().cpu().numpy()
        for name, lin, K, gk, bk in (("ih", ih, I, gi, bi), ("hh", hh, H, gh, bh)):
            nz = lin.materialize_noise(s, (B, K), (B, 4 * H), torch.float32)
            st = dict(eps_w=E._np(nz["eps_w"]), eps_b=E._np(nz["eps_b"]), s_in=None, s_out=None)
            if c.flip:
                pz = lin.materialize_noise(s, (K, K), (K, 4 * H), torch.float32)    # the probe's own rows
                si, so = E._np(pz["sign_in"]), E._np(pz["sign_out"])
                st["D"] = (gk * so * np.diagonal(si)[:, None]).T                     # gate[k, n] = s_out[k, n] s_in[k, k] Delta[n, k]
                st["db"] = bk * E._np(lin.materialize_noise(s, (1, K), (1, 4 * H), torch.float32)["sign_out"])[0]
                st["s_in"], st["s_out"] = E._np(nz["sign_in"]), E._np(nz["sign_out"])
            else:
                st["W"], st["b"] = gk.T, bk
            c.steps[name].append(st)
    _CTX[key] = c
    return c


def _layer_steps(c, name, bias):
    lin = getattr(c.layer, name)
    out = []
    for st in c.steps[name]:
        if c.flip:
            out.append(E.lstm_layer_step(mu=lin._w()[0], D=st["D"], bm=lin.mu_bias if bias else None, bd=st["db"] if bias else None,
                                         s_in=st["s_in"], s_out=st["s_out"]))
        else:
            out.append(E.lstm_layer_step(mu=st["W"], bm=st["b"] if bias else None))
    return out


def _run(c, cfg):
    """one direct forward (training and inference kernels) + backward -> dict of CPU tensors; cached"""
    key = (id(c), cfg)
    if key in _RUNS:
        return _RUNS[key]
    from bayesian_torch_amd import functional as BF
    prec, act, bias, state = cfg
    I, H, B, T = c.case
    dt = _adt(act)
    x = c.x.to(dt)
    h0, c0 = (c.h0.to(dt), c.c0.to(dt)) if state else (None, None)
    ihp, hhp = _params(c.layer.ih, S0, bias), _params(c.layer.hh, S0, bias)
    hs, cs, _, sv = BF.lstm_train_fwd_hip(c.kind, x, ihp, hhp, c.seed, prec=prec, h0=h0, c0=c0)
    hs_i, cs_i, _ = BF.lstm_hip(c.kind, x, ihp, hhp, c.seed, prec=prec, h0=h0, c0=c0)
    d_hs, d_cs = c.r_h.to(dt), c.r_c.to(dt)
    dx, dh0, dc0, gi, gh = BF.lstm_bwd_hip(c.kind, x, ihp, hhp, c.seed, hs, sv, d_hs, d_cs, prec=prec, h0=h0, c0=c0, want_dx=True,
                                           want_dh0=state, want_dc0=state)
    torch.cuda.synchronize()
    gates, cells = _saved_views(sv, T, B, H)
    r = dict(x=x, h0=h0, c0=c0, hs=hs, cs=cs, hs_i=hs_i, cs_i=cs_i, gates=gates, cells=cells, d_hs=d_hs, d_cs=d_cs, dx=dx)
    if state:
        r["dh0"], r["dc0"] = dh0, dc0
    for name, g4 in (("ih", gi), ("hh", gh)):
        for k, t in zip(("dmu_w", "drho_w", "dmu_b", "drho_b"), g4):
            if t is not None:
                r[name + "." + k] = t
    r = {k: (None if v is None else v.detach().cpu().clone()) for k, v in r.items()}
    _RUNS[key] = r
    return r


def _reports(c, cfg):
    """every check of steps 2, 3 and 5 on one run -> {name: Report}, useful fractions of the backward bounds; cached"""
    key = (id(c), cfg)
    if key in _REPORTS:
        return _REPORTS[key]
    prec, act, bias, state = cfg
    I, H, B, T = c.case
    r = _run(c, cfg)
    bf16, act_bf16 = prec == "bf16", act == "bf16"
    Li, Lh = _layer_steps(c, "ih", bias), _layer_steps(c, "hh", bias)
    reps = {}
    for t in range(T):
        hp = r["hs"][:, t - 1] if t > 0 else r["h0"]          # teacher forcing: the GPU's own previous state
        ref, bnd = E.lstm_gates64(r["x"][:, t], hp, Li[t], Lh[t], bf16)
        reps["gates t=%d" % t] = E.check(r["gates"][t], ref, bnd)
        cc, b_c, h, b_h = E.lstm_cell64(r["gates"][t], r["cells"][t - 1] if t > 0 else r["c0"])
        reps["cell t=%d" % t] = E.check(r["cells"][t], cc, b_c)
        reps["c_seq t=%d" % t] = E.check(r["cs"][:, t], cc, E.store_rounding(b_c, cc) if act_bf16 else b_c)
        reps["hidden_seq t=%d" % t] = E.check(r["hs"][:, t], h, E.store_rounding(b_h, h) if act_bf16 else b_h)
    noise = {n: [(st["eps_w"], st["eps_b"] if bias else None) for st in c.steps[n]] for n in ("ih", "hh")}
    rho = {n: (getattr(c.layer, n)._w()[1], getattr(c.layer, n).rho_bias if bias else None) for n in ("ih", "hh")}
    args = (r["gates"], r["cells"], r["c0"], Li, Lh, r["x"], r["hs"], r["h0"], r["d_hs"], r["d_cs"], noise, rho, bf16)
    ref = E.lstm_bptt64(*args, want_state=state)
    mag = E.lstm_bptt64(*args, want_state=state, absolute=True)
    useful = {}
    for k, rv in ref.items():
        bnd = rv.e
        useful[k] = float((bnd <= E.LSTM_USEFUL * mag[k].v).mean())
        if act_bf16 and k in ("dx", "dh0", "dc0"):
            bnd = E.store_rounding(bnd, rv.v)
        reps["bwd " + k] = E.check(r[k], rv.v, bnd)
    assert set(k for k in r if k.startswith(("ih.", "hh.", "dx", "dh0", "dc0"))) == set(ref)
    _REPORTS[key] = (reps, useful)
    return _REPORTS[key]


def _assert_reports(c, cls, prefix):
    worst, bad = {}, []
    for cfg in CONFIGS:
        reps, _ = _reports(c, cfg)
        for k, rep in reps.items():
            if not k.startswith(prefix):
                continue
            name = (cfg[1], k.split(" t=")[0])
            worst[name] = max(worst.get(name, 0.0), rep.worst)
            if not rep.ok:
                bad.append((cfg, k, str(rep)))
    for act in ("f32", "bf16"):  # bf16 activations: the stored outputs carry one store rounding, which reaches its own bound
        print("%s %s, %s activations: worst err/bound over %d configurations: %s"
              % (cls, c.case, act, len(CONFIGS) // 2, ", ".join("%s %.3g" % (k[1], v) for k, v in sorted(worst.items()) if k[0] == act)))
    assert not bad, bad[:8]


# =============================================================================================================================
# 0. the device's sigm expression and tanhf: the constants of envelope.py hold
# =============================================================================================================================
def test_device_sigm_and_tanhf_error_stays_inside_the_constants():
    """1 / (1 + expf(-v)) and tanhf on the GPU against float64 over the gate range (dense near 0, where the results' ulps shrink):
    SIGM_ULP / TANH_ULP are twice the first measurement, so the measured maximum must stay below them"""
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    v = torch.cat([(torch.rand(1 << 21, generator=g) * 2 - 1) * GATE_RANGE, (torch.rand(1 << 21, generator=g) * 2 - 1) * 8,
                   torch.randn(1 << 20, generator=g) * torch.exp2(-torch.rand(1 << 20, generator=g) * 24)]).float()
    vd = v.to(dev)
    sg, th = torch.sigmoid(vd).cpu(), torch.tanh(vd).cpu()
    sg2 = (1.0 / (1.0 + torch.exp(-vd))).cpu()
    v64 = v.double().numpy()
    es, _ = E.ulp_error(sg, 1.0 / (1.0 + np.exp(-v64)))
    es2, _ = E.ulp_error(sg2, 1.0 / (1.0 + np.exp(-v64)))
    et, _ = E.ulp_error(th, np.tanh(v64))
    print("device sigm: %.3f ulp (torch.sigmoid), %.3f ulp (1 / (1 + exp(-v))); tanhf: %.3f ulp; constants %.2f / %.2f"
          % (es, es2, et, E.SIGM_ULP, E.TANH_ULP))
    assert max(es, es2) <= E.SIGM_ULP and et <= E.TANH_ULP


# =============================================================================================================================
# 1. sampled weights and biases: the noise indices
# =============================================================================================================================
@pytest.mark.parametrize("case", CASES, **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_probed_weights_and_biases_match_the_noise_indices(cls, case):
    c = _ctx(cls, case)
    worst_w = worst_b = 0.0
    bad = []
    for name in ("ih", "hh"):
        lin = getattr(c.layer, name)
        mu, rho = lin._w()
        mu64, sg = E.d64(mu).numpy(), E.sigma64(rho).numpy()
        mub, sgb = E.d64(lin.mu_bias).numpy(), E.sigma64(lin.rho_bias).numpy()
        for t, st in enumerate(c.steps[name]):
            d, db = sg * st["eps_w"], sgb * st["eps_b"]
            if c.flip:   # the probe returned +-Delta: mu is known exactly
                items = (("Delta", st["D"], d, np.abs(d), E.DELTA_W_LSTM), ("Delta_b", st["db"], db, np.abs(db), E.DELTA_B_LSTM))
            else:
                items = (("W", st["W"], mu64 + d, np.abs(mu64) + np.abs(d), E.DELTA_W_LSTM),
                         ("b", st["b"], mub + db, np.abs(mub) + np.abs(db), E.DELTA_B_LSTM))
            for what, got, ref, A, delta in items:
                rep = E.check(got, ref, delta * A)
                if what.endswith("b"):
                    worst_b = max(worst_b, rep.worst * delta)
                else:
                    worst_w = max(worst_w, rep.worst * delta)
                if not rep.ok:
                    bad.append((name, t, what, str(rep)))
    print("%s %s: sampled-weight error %.4g (DELTA_W_LSTM %.4g), bias %.4g (DELTA_B_LSTM %.4g), relative to |mu| + |sigma eps|"
          % (cls, case, worst_w, E.DELTA_W_LSTM, worst_b, E.DELTA_B_LSTM))
    assert not bad, bad[:8]


# =============================================================================================================================
# 2. / 3. gate pre-activations (accumulation only), cell and hidden state (transcendentals only)
# =============================================================================================================================
@pytest.mark.parametrize("case", CASES, **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_saved_gates_every_element(cls, case):
    c = _ctx(cls, case)
    _assert_reports(c, cls, "gates")
    top = max(float(_run(c, cfg)["gates"].abs().max()) for cfg in CONFIGS)
    assert top <= GATE_RANGE, top  # the range SIGM_ULP / TANH_ULP were measured on


@pytest.mark.parametrize("case", CASES, **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_cell_and_hidden_state_every_element(cls, case):
    c = _ctx(cls, case)
    for cfg in CONFIGS:
        r = _run(c, cfg)
        # the inference kernel (lanes = 1) returns the training forward's bits
        assert torch.equal(r["hs_i"], r["hs"]) and torch.equal(r["cs_i"], r["cs"]), cfg
        # `saved` is written in full: every word is finite and compared below (gates: the test above)
        assert bool(torch.isfinite(r["gates"]).all()) and bool(torch.isfinite(r["cells"]).all()), cfg
        if cfg[1] == "f32":  # c_seq IS the saved f32 cell state
            assert torch.equal(r["cs"].transpose(0, 1), r["cells"]), cfg
    for prefix in ("cell", "c_seq", "hidden_seq"):
        _assert_reports(c, cls, prefix)


# =============================================================================================================================
# 4. exact forward run
# =============================================================================================================================
@pytest.mark.parametrize("case", CASES, **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_integer_forward_is_exact_and_drho_is_zero(cls, case):
    """rho = -200: btx_softplus_hw returns 0 (its d == 0 branch), W = mu exactly; small integers are exact in bf16 and every
    partial sum is an integer below 2^24.  sigmoid(-200) is 0 in f32, so every drho of the backward is exactly 0."""
    from bayesian_torch_amd import _lib, functional as BF
    dev = _dev()
    I, H, B, _ = case
    kind = _lib.KIND_FLIPOUT if cls == "LSTMFlipout" else _lib.KIND_REPARAM
    n = 10 * CASES.index(case)
    mk = lambda shape, k: E.small_ints(shape, 700 + n + k).to(dev)  # noqa: E731
    x, h0, c0 = mk((B, 1, I), 0), mk((B, H), 1), mk((B, H), 2)
    par = {}
    for name, K, k in (("ih", I, 3), ("hh", H, 5)):
        par[name] = (mk((4 * H, K), k), torch.full((4 * H, K), -200.0, device=dev), mk((4 * H,), k + 1),
                     torch.full((4 * H,), -200.0, device=dev), 40 + k, S0, None)
    ref = (E.d64(x[:, 0]) @ E.d64(par["ih"][0]).t() + E.d64(par["ih"][2]) + E.d64(h0) @ E.d64(par["hh"][0]).t() + E.d64(par["hh"][2]))
    assert float(ref.abs().max()) < 2 ** 24
    g = torch.Generator().manual_seed(n)
    d_hs, d_cs = torch.randn(B, 1, H, generator=g).to(dev), torch.randn(B, 1, H, generator=g).to(dev)
    for prec, act in itertools.product(("f32", "bf16"), ("f32", "bf16")):
        dt = _adt(act)
        hs, cs, _, sv = BF.lstm_train_fwd_hip(kind, x.to(dt), par["ih"], par["hh"], SEED, prec=prec, h0=h0.to(dt), c0=c0.to(dt))
        rep = E.check_exact(_saved_views(sv, 1, B, H)[0][0], ref)
        assert rep.ok, (prec, act, str(rep))
        _, _, _, gi, gh = BF.lstm_bwd_hip(kind, x.to(dt), par["ih"], par["hh"], SEED, hs, sv, d_hs, d_cs, prec=prec, h0=h0.to(dt),
                                          c0=c0.to(dt))
        for g4 in (gi, gh):
            assert bool(torch.isfinite(g4[0]).all()) and bool(torch.isfinite(g4[2]).all())
            assert int(torch.count_nonzero(g4[1])) == 0 and int(torch.count_nonzero(g4[3])) == 0, (prec, act)


# =============================================================================================================================
# 5. backward through time
# =============================================================================================================================
@pytest.mark.parametrize("case", CASES, **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_backward_every_element(cls, case):
    c = _ctx(cls, case)
    _assert_reports(c, cls, "bwd")
    least = min(min(_reports(c, cfg)[1].values()) for cfg in CONFIGS)
    print("%s %s: backward bound <= %.0e A (before a bf16 store) on %.4f of the elements at least" % (cls, case, E.LSTM_USEFUL, least))


# =============================================================================================================================
# 6. paths that never ran
# =============================================================================================================================
_GRAD_KEYS = ("mu_weight", "rho_weight", "mu_bias", "rho_bias")


def _layer_grads(c, prec, act, loss="both", leaves=("x", "h0", "c0"), frozen=()):
    """one training step through the layer (fused_training): (hs, cs, grads).  loss: both | c | h | c+0h | h+0c (the last two
    hand the backward a zero gradient tensor instead of None); leaves: which of x, h0, c0 require grad; frozen: 'ih' / 'hh'"""
    import bayesian_torch_amd as bt
    layer = c.layer
    dt = _adt(act)
    layer.fused_training = True
    bt.set_sample_index(layer, S0)
    for p in layer.parameters():
        p.grad = None
    for name in ("ih", "hh"):
        for k in _GRAD_KEYS:
            getattr(getattr(layer, name), k).requires_grad_(name not in frozen)
    t = {k: v.to(dt).clone().requires_grad_(k in leaves) for k, v in (("x", c.x), ("h0", c.h0), ("c0", c.c0))}
    r_h, r_c = c.r_h.to(dt).float(), c.r_c.to(dt).float()
    try:
        bt.set_precision(prec)
        hs, (_, cs), _ = layer(t["x"], (t["h0"], t["c0"]))
        terms = {"both": (1, 1), "c": (None, 1), "h": (1, None), "c+0h": (0, 1), "h+0c": (1, 0)}[loss]
        total = 0
        if terms[0] is not None:
            total = total + (hs.float() * (r_h * terms[0])).sum()
        if terms[1] is not None:
            total = total + (cs.float() * (r_c * terms[1])).sum()
        total.backward()
    finally:
        bt.set_precision("f32")
        for p in layer.parameters():
            p.requires_grad_(True)
    out = {k: v.grad for k, v in t.items()}
    for name in ("ih", "hh"):
        for k in _GRAD_KEYS:
            out[name + "." + k] = getattr(getattr(layer, name), k).grad
    return hs.detach(), cs.detach(), out


_DIRECT = {"x": "dx", "h0": "dh0", "c0": "dc0", "mu_weight": "dmu_w", "rho_weight": "drho_w", "mu_bias": "dmu_b", "rho_bias": "drho_b"}


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("case", [(12, 10, 4, 3), (65, 17, 65, 2)], **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_bf16_activations_through_the_layers(cls, case, prec):
    """lstm_kernel<*, *, __bf16, 2> and launch_bwd<*, *, __bf16>: bf16 x, h0, c0 through the layer return the bits of the direct
    calls, and those pass the element-wise checks of steps 2, 3 and 5"""
    c = _ctx(cls, case)
    cfg = (prec, "bf16", True, True)
    reps, _ = _reports(c, cfg)
    bad = [(k, str(r)) for k, r in reps.items() if not r.ok]
    assert not bad, bad[:8]
    r = _run(c, cfg)
    hs, cs, grads = _layer_grads(c, prec, "bf16")
    assert hs.dtype == torch.bfloat16 and torch.equal(hs.cpu(), r["hs"]) and torch.equal(cs.cpu(), r["cs"])
    for k, g in grads.items():
        name = k.split(".")
        want = r[_DIRECT[k]] if len(name) == 1 else r[name[0] + "." + _DIRECT[name[1]]]
        assert g is not None and g.dtype == want.dtype and torch.equal(g.cpu(), want), k


SELECTIVE = [  # (id, loss, leaves, frozen, the all-gradients call it is compared with)
    ("c_seq-only", "c", ("x", "h0", "c0"), (), "c+0h"),
    ("hidden_seq-only", "h", ("x", "h0", "c0"), (), "h+0c"),
    ("no-dx", "both", ("h0", "c0"), (), "both"),
    ("only-h0", "both", ("x", "h0"), (), "both"),
    ("only-c0", "both", ("x", "c0"), (), "both"),
    ("ih-frozen", "both", ("x", "h0", "c0"), ("ih",), "both"),
    ("hh-frozen", "both", ("x", "h0", "c0"), ("hh",), "both"),
]


@pytest.mark.parametrize("case", [(8, 16, 3, 2), (65, 17, 65, 2)], **_ids)
@pytest.mark.parametrize("cls", FAMILIES)
def test_selective_gradients_equal_the_all_gradients_call(cls, case):
    """the selective paths of btx_lstm_bwd (d_hidden_seq / d_c_seq null, dx / dh0 / dc0 / g_ih / g_hh not wanted): what is
    produced equals the all-gradients call bit for bit (deterministic kernels, independent launches), the rest is None"""
    c = _ctx(cls, case)
    for act in ("f32", "bf16"):
        full = {}
        for sid, loss, leaves, frozen, base in SELECTIVE:
            if base not in full:
                full[base] = _layer_grads(c, "f32", act, loss=base)[2]
                assert all(g is not None for g in full[base].values())
            got = _layer_grads(c, "f32", act, loss=loss, leaves=leaves, frozen=frozen)[2]
            for k, g in got.items():
                wanted = (k in leaves) if "." not in k else (k.split(".")[0] not in frozen)
                if not wanted:
                    assert g is None, (sid, act, k)
                else:
                    assert g is not None and torch.equal(g, full[base][k]), (sid, act, k)
