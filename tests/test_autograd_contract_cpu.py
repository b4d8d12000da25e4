"""The autograd-contract scenarios of tests/autograd_cases.py without a GPU: they pass on a correct stand-in for the HIP Functions and
each fails when the fault it is there for is planted (the rule of tests/test_envelope_cpu.py and tests/test_poison_cpu.py: a new
instrument proves its teeth on the CPU).

The stand-in is a LinearFlipout whose torch.autograd.Function computes the forward with the float32 reference chain (oracle/bt_ref.py)
on the noise BTX-RNG v1 defines (oracle.bt_oracle.eps / sign) and whose backward REGENERATES that noise from what it kept on ctx —
seed, sample index, device word — behind a layer with the real counter logic of _VariationalNd.forward.  profiles/autograd_contract.txt
lists the faults and the factor by which each fails.
"""
import types

import pytest
import torch

import autograd_cases as AC

SAMPLE = AC.SAMPLE


class _StandInFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, sample_idx, x, mu, rho, mu_b, rho_b):
        from bayesian_torch_amd import rng
        from oracle import bt_ref
        ctx.layer, ctx.sample_idx, ctx.seed = layer, sample_idx, rng.seed()
        ctx.sample_dev = layer.__dict__.get("_btx_sample_dev")
        x2 = x.reshape(-1, x.shape[-1])
        nz = layer._noise(ctx.seed, layer._index(sample_idx, ctx.sample_dev), x2.shape[0])
        with torch.no_grad():
            out = bt_ref.flipout_forward(x2, mu, rho, mu_b, rho_b, nz["eps_w"], nz.get("eps_b"), nz["sign_in"], nz["sign_out"],
                                         dict(kind="linear"))
        ctx.save_for_backward(x, mu, rho, rho_b)
        return out.reshape(x.shape[:-1] + (mu.shape[0],))

    @staticmethod
    def backward(ctx, dy):
        from bayesian_torch_amd.autograd import _first_order
        return _first_order(_StandInFn._backward)(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        from bayesian_torch_amd import rng
        from oracle import bt_ref
        layer, need = ctx.layer, ctx.needs_input_grad
        x, mu, rho, rho_b = ctx.saved_tensors
        fault = layer.fault
        s = layer._index(ctx.sample_idx, ctx.sample_dev)
        if fault == "word_host":
            s = int(ctx.sample_idx)                        # the host index of the forward, ignoring the device word it read
        if fault == "word_current":
            s = layer._index(ctx.sample_idx, layer.__dict__.get("_btx_sample_dev"))   # the word the layer points at NOW
        if fault == "counter":
            s = layer._btx_sample - 1                      # the layer's CURRENT counter instead of ctx
        seed = rng.seed() if fault == "seed" else ctx.seed  # the CURRENT seed instead of ctx
        x2, dy2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
        nz = layer._noise(seed, s, x2.shape[0])
        si, so = nz["sign_in"], nz["sign_out"]
        want_w, want_b = need[3] or need[4], rho_b is not None and (need[5] or need[6])
        if fault == "no_signs" and layer.padded and not (want_w or want_b):
            si, so = torch.ones_like(si), torch.ones_like(so)   # the sign tensors not materialised when only x needs a gradient
        dys = dy2 * so
        dx = dmu = drho = dmu_b = drho_b = None
        if need[2]:
            dx = (dy2 @ mu + (dys @ (bt_ref.softplus(rho) * nz["eps_w"])) * si).reshape(x.shape)
        if want_w:
            dmu = dy2.t() @ x2
            drho = (dys.t() @ (x2 * si)) * nz["eps_w"] * torch.sigmoid(rho)
        if want_b:
            dmu_b = dy2.sum(0)
            drho_b = dys.sum(0) * nz["eps_b"] * torch.sigmoid(rho_b)
        if fault == "drop_drho" and not need[3]:
            drho = None                                     # drho dropped when mu is frozen
        return None, None, dx, dmu, drho, dmu_b, drho_b


class StandIn(torch.nn.Module):
    """LinearFlipout on the CPU with the counters, the needs-grad predicate and the ctx of the HIP path"""
    fault = None
    _family = "flipout"
    _op = types.SimpleNamespace(nd=0)

    def __init__(self, cin, cout, bias=True, padded=False, seed=3):
        super().__init__()
        from bayesian_torch_amd import rng
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.mu_weight = torch.nn.Parameter(r(cout, cin) * 0.3)
        self.rho_weight = torch.nn.Parameter(torch.rand(cout, cin, generator=g) * 5.0 - 5.0)
        self.mu_bias = torch.nn.Parameter(r(cout) * 0.5) if bias else None
        self.rho_bias = torch.nn.Parameter(torch.rand(cout, generator=g) * 3.0 - 3.0) if bias else None
        self.padded, self.cpad = padded, (cin + 7) // 8 * 8 if padded else cin
        self._btx_layer_id = rng.next_layer_id()
        self._btx_sample = 0

    def _w(self):
        return self.mu_weight, self.rho_weight

    @staticmethod
    def _index(sample_idx, sdev):
        return int(sdev.reshape(-1)[0]) if sdev is not None else int(sample_idx)

    def _noise(self, seed, s, rows):
        from bayesian_torch_amd import _lib
        from oracle import bt_oracle as O
        n, k, kp, lid = self.mu_weight.shape[0], self.mu_weight.shape[1], self.cpad, self._btx_layer_id
        t = torch.from_numpy
        d = {"eps_w": t(O.eps(n * kp, seed, s, lid, _lib.STREAM_EPS_W)).reshape(n, kp)[:, :k].contiguous(),
             "sign_in": t(O.sign(rows * kp, seed, s, lid, _lib.STREAM_SIGN_IN)).reshape(rows, kp)[:, :k].float(),
             "sign_out": t(O.sign(rows * n, seed, s, lid, _lib.STREAM_SIGN_OUT)).reshape(rows, n).float()}
        if self.mu_bias is not None:
            d["eps_b"] = t(O.eps(n, seed, s, lid, _lib.STREAM_EPS_B))
        return d

    def materialize_noise(self, sample_idx, x_shape=None, out_shape=None, x_dtype=None, signs=True, sample_dev=None):
        from bayesian_torch_amd import rng
        rows = 1
        for v in x_shape[:-1]:
            rows *= int(v)
        return self._noise(rng.seed(), self._index(sample_idx, sample_dev), rows)

    def _needs_grad(self, t):
        rb = self.rho_bias is not None and self.rho_bias.requires_grad and self.fault != "rho_b_pred"
        return torch.is_grad_enabled() and (self.mu_weight.requires_grad or self.rho_weight.requires_grad or rb or
                                            (self.mu_bias is not None and self.mu_bias.requires_grad) or t.requires_grad)

    def forward(self, x):
        s_idx = self._btx_sample
        self.__dict__["_btx_sample"] = s_idx + 1
        self.__dict__["_btx_kl_sample"] = s_idx
        if self.fault == "shared_index":   # a second application in one graph reuses the first application's index
            s_idx = self.__dict__.setdefault("_first_idx", s_idx)
        if self._needs_grad(x):
            return _StandInFn.apply(self, s_idx, x, self.mu_weight, self.rho_weight, self.mu_bias, self.rho_bias)
        with torch.no_grad():
            return _StandInFn.apply(self, s_idx, x, self.mu_weight, self.rho_weight, self.mu_bias, self.rho_bias)


def _build(cin=24, cout=16, rows=(5,), padded=False, bias=True):
    def build():
        import bayesian_torch_amd as bt
        bt.manual_seed(2024)
        layer = StandIn(cin, cout, bias=bias, padded=padded)
        bt.assign_layer_ids(layer)
        return layer, AC.tensor(rows + (cin,), torch.float32, 11, "cpu", 1.5)
    return build


def _block():
    import bayesian_torch_amd as bt
    bt.manual_seed(2024)
    net = torch.nn.Sequential(StandIn(24, 16, seed=3), torch.nn.ReLU(), StandIn(16, 8, seed=4))
    bt.assign_layer_ids(net)
    return net, AC.tensor((5, 24), torch.float32, 11, "cpu", 1.5)


def _wrapper(net, x):
    from bayesian_torch_amd.utils import checkpoint
    return checkpoint(net, x)


def _plain_torch_checkpoint(net, x):
    import torch.utils.checkpoint as tcp
    return tcp.checkpoint(net, x, use_reentrant=False)   # nothing preserves the counters: the recomputation draws s + 1


PLAIN, PADDED, SQUARE, ROWS3D = _build(), _build(20, 10, (7,), padded=True), _build(16, 16), _build(32, 16, (3, 4))

SCENARIOS = {
    "S1": lambda: AC.s1_subsets(PLAIN, "stand-in", AC.ref64_single()),
    "S1-padded": lambda: AC.s1_subsets(PADDED, "stand-in padded", AC.ref64_single()),
    "S1-3d": lambda: AC.s1_subsets(ROWS3D, "stand-in 3-D", AC.ref64_single()),
    "S2": lambda: AC.s2_forward_identity(PLAIN, "stand-in"),
    "S2-words": lambda: AC.s2_forward_identity(PLAIN, "stand-in", words=True),
    "S3": lambda: AC.s3_seed_change(PLAIN, "stand-in"),
    "S5": lambda: AC.s5_retain_and_accumulate(PLAIN, "stand-in"),
    "S6": lambda: AC.s6_applied_twice(SQUARE, "stand-in", AC.ref64_twice()),
    "S9": lambda: AC.s9_checkpoint(_block, "stand-in", _wrapper),
}


@pytest.fixture(autouse=True)
def _no_fault():
    from bayesian_torch_amd import rng
    old = rng.seed()
    StandIn.fault = None
    yield
    StandIn.fault = None
    rng.manual_seed(old)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenarios_pass_on_the_correct_stand_in(name):
    SCENARIOS[name]()


# fault -> (the scenario that must catch it, what the failure says)
FAULTS = [
    ("counter", "S2", "not the same bits"),
    ("counter", "S2-words", "not the same bits"),  # the host counter instead of the device word the forward read
    ("word_host", "S2-words", "not the same bits"),     # ctx.sample_idx instead of the device word the forward read
    ("word_host", "S2", None),                          # no device word: the host index IS the forward's identity
    ("word_current", "S2-words", "not the same bits"),  # the word the layer points at when the backward runs (none, by then)
    ("seed", "S3", "not the same bits"),
    ("rho_b_pred", "S1", r"\{rho_b\}: the output has no grad_fn"),
    ("drop_drho", "S1", r"\{rho\} drho: no gradient"),
    ("no_signs", "S1-padded", r"\{x\} dx: not the same bits"),
    ("no_signs", "S1", None),                      # plain layout: the fault's branch is not reached
    ("shared_index", "S6", "outside the envelope"),
]


@pytest.mark.parametrize("fault,scenario,says", FAULTS, ids=["%s-%s" % (f, s) for f, s, _ in FAULTS])
def test_each_planted_fault_fails_its_scenario(fault, scenario, says):
    StandIn.fault = fault
    if says is None:
        SCENARIOS[scenario]()
        return
    with pytest.raises(AssertionError, match=says) as info:
        SCENARIOS[scenario]()
    print("fault %s fails %s:\n%s" % (fault, scenario, "\n".join(str(info.value).splitlines()[:3])))


def test_plain_torch_checkpoint_redraws_the_noise_and_the_wrapper_does_not():
    """the counter advancing during the recomputation: plain torch.utils.checkpoint fails S9, the wrapper passes it (SCENARIOS["S9"])"""
    with pytest.raises(AssertionError, match="not the same bits|counters") as info:
        AC.s9_checkpoint(_block, "stand-in plain checkpoint", _plain_torch_checkpoint)
    print("plain torch.utils.checkpoint fails S9:\n%s" % "\n".join(str(info.value).splitlines()[:3]))


def test_wrapper_needs_to_know_its_modules():
    from bayesian_torch_amd.utils import checkpoint
    net, x = _block()
    with pytest.raises(ValueError, match="modules="):
        checkpoint(lambda t: net(t), x.requires_grad_())
    y = checkpoint(lambda t: net(t), x, modules=net)
    y.sum().backward()
    with pytest.raises(ValueError, match="use_reentrant"):
        checkpoint(net, x, use_reentrant=True)


def test_second_order_through_the_stand_in_is_refused():
    layer, x = PLAIN()
    out, leaves = AC.forward(layer, x, ("x", "mu"))
    with pytest.raises(RuntimeError, match="first-order only"):   # the gradient penalty's call: dy is a plain tensor
        (gx,) = torch.autograd.grad(out.sum(), leaves["x"], create_graph=True)
        gx.sum().backward()


def test_cases_table_is_well_formed():
    ids = [c.id for c in AC.CASES]
    assert len(set(ids)) == len(ids) and {"L1", "L2", "L3", "C1", "C2", "C3", "C4", "C5", "C6", "C7", "R1", "R2"} <= set(ids)
    assert len(list(AC.subsets(AC.NAMES))) == 31
