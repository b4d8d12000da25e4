"""models.fuse.fuse_model on the CPU: which chains are folded, and that a fused model computes, trains, pickles and copies
exactly like the unfused one.  (The models are defined here; the GPU side is tests/test_gpu_fuse_model.py.)"""
import copy
import io
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

PRIOR = dict(prior_mu=0.0, prior_sigma=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, type="Flipout",
             moped_enable=False, moped_delta=0.5)


# ---- models ------------------------------------------------------------------------------------------------------------------
def vgg_bn(width=8, classes=10, fc=32):
    """VGG-BN shape: conv-BN-ReLU stages with 2x2 max-pools, Linear-BN1d-ReLU head.  Sites: 4 convs + 1 Linear."""
    c = [width, width, 2 * width, 2 * width]
    feats, cin = [], 3
    for i, co in enumerate(c):
        feats += [nn.Conv2d(cin, co, 3, padding=1), nn.BatchNorm2d(co), nn.ReLU(inplace=True)]
        if i % 2 == 1:
            feats.append(nn.MaxPool2d(2, 2))
        cin = co
    return nn.Sequential(nn.Sequential(*feats), nn.Flatten(),
                         nn.Linear(cin * 4 * 4, fc), nn.BatchNorm1d(fc), nn.ReLU(inplace=True), nn.Linear(fc, classes))


class InvertedResidual(nn.Module):
    """MobileNetV2 block: 1x1 expand -> BN -> ReLU6, 3x3 depthwise -> BN -> ReLU6, 1x1 projection -> BN (+ skip)"""

    def __init__(self, cin, cout, stride, expand):
        super().__init__()
        hid = cin * expand
        self.skip = stride == 1 and cin == cout
        self.expand = nn.Conv2d(cin, hid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(hid)
        self.dw = nn.Conv2d(hid, hid, 3, stride, 1, groups=hid, bias=False)
        self.bn2 = nn.BatchNorm2d(hid)
        self.act2 = nn.Hardtanh(0.0, 6.0)
        self.project = nn.Conv2d(hid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)

    def forward(self, x):
        y = F.relu6(self.bn1(self.expand(x)))
        y = self.act2(self.bn2(self.dw(y)))
        y = self.bn3(self.project(y))
        return x + y if self.skip else y


class MobileNetV2ish(nn.Module):
    """stem ConvBNReLU6, two inverted-residual blocks (one with a skip), a 1x1 ConvBNReLU6, pool, classifier.  Sites: 1 + 3 + 3 + 1."""

    def __init__(self, classes=10):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 8, 3, 2, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU6(inplace=True))
        self.blocks = nn.Sequential(InvertedResidual(8, 8, 1, 4), InvertedResidual(8, 16, 2, 4))
        self.head = nn.Sequential(nn.Conv2d(16, 32, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU6(inplace=True))
        self.fc = nn.Linear(32, classes)

    def forward(self, x):
        x = self.head(self.blocks(self.stem(x)))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


class SimpleCNN(nn.Module):
    """conv -> ReLU without BN, in three spellings.  Sites: 3."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 8, 3, padding=1)
        self.c2 = nn.Conv2d(8, 16, 3, padding=1)
        self.f1 = nn.Linear(16 * 4 * 4, 32)
        self.r = nn.ReLU()
        self.f2 = nn.Linear(32, 10)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.c1(x)), 2)
        x = F.max_pool2d(self.c2(x).relu(), 2)
        return self.f2(self.r(self.f1(x.flatten(1))))


class Branchy(nn.Module):
    """an `if` on a tensor value: not traceable.  The nn.Sequential chains (2) are still fused; `side` is not."""

    def __init__(self):
        super().__init__()
        self.a = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU())
        self.b = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1), nn.BatchNorm2d(8))
        self.side = nn.Conv2d(8, 8, 1)
        self.bn = nn.BatchNorm2d(8)

    def forward(self, x):
        y = self.a(x)
        if y.mean() > 0:
            y = self.b(y)
        return torch.relu(self.bn(self.side(y)))


class TwoUsers(nn.Module):
    """the BN's output feeds both the ReLU and the add: nothing may be folded (0 sites)"""

    def __init__(self):
        super().__init__()
        self.c = nn.Conv2d(3, 8, 3, padding=1)
        self.bn = nn.BatchNorm2d(8)

    def forward(self, x):
        y = self.bn(self.c(x))
        return torch.relu(y) + y


MODELS = {"vgg_bn": (vgg_bn, 5), "mobilenet_v2": (MobileNetV2ish, 8), "simple_cnn": (SimpleCNN, 3),
          "branchy": (Branchy, 2), "two_users": (TwoUsers, 0)}


def make(name, seed=0):
    """the converted model with non-trivial BN statistics and affine parameters, in eval mode"""
    from bayesian_torch_amd.models import dnn_to_bnn
    torch.manual_seed(seed)
    m = MODELS[name][0]()
    dnn_to_bnn(m, PRIOR)
    with torch.no_grad():
        for b in m.modules():
            if isinstance(b, nn.modules.batchnorm._BatchNorm):
                b.running_mean.normal_(0, 0.2)
                b.running_var.uniform_(0.5, 1.5)
                b.weight.uniform_(0.5, 1.5)
                b.bias.normal_(0, 0.2)
    return m.eval()


def run(m, x, seed=123):
    torch.manual_seed(seed)  # the CPU path draws its noise from torch's generator: the same seed, the same noise
    with torch.no_grad():
        return m(x)


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def fuse_quietly(m):
    from bayesian_torch_amd.models import fuse_model
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fuse_model(m)


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_site_count_keys_and_eval_outputs(name):
    m = make(name)
    x = torch.randn(4, 3, 16, 16)
    keys = list(m.state_dict().keys())
    params = [id(p) for p in m.parameters()]
    ref = run(m, x)
    assert fuse_quietly(m) == MODELS[name][1]
    assert list(m.state_dict().keys()) == keys
    assert [id(p) for p in m.parameters()] == params
    assert rel(run(m, x), ref) <= 1e-6


def test_sites_replace_the_chains_ops():
    """the fused forward really calls forward_fused with the folded epilogue (not the original modules)"""
    m = make("mobilenet_v2")
    calls = []
    for mod in m.modules():
        if hasattr(mod, "forward_fused"):
            orig = mod.forward_fused

            def spy(*a, _o=orig, **k):
                calls.append(k.get("act"))
                return _o(*a, **k)
            object.__setattr__(mod, "forward_fused", spy)
    fuse_quietly(m)
    run(m, torch.randn(2, 3, 16, 16))
    assert sorted(calls) == sorted(["relu6"] * 6 + ["none"] * 2)


def test_untraceable_model_falls_back_to_sequentials_with_one_warning():
    from bayesian_torch_amd.models import fuse_model
    m = make("branchy")
    x = torch.randn(2, 3, 16, 16)
    ref = run(m, x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert fuse_model(m) == 2
    msgs = [str(i.message) for i in w if "fuse_model" in str(i.message)]
    assert len(msgs) == 1 and "side" in msgs[0], msgs
    assert rel(run(m, x), ref) <= 1e-6


def test_train_mode_is_the_unfused_model():
    """training mode runs the original ops: same outputs, gradients and running statistics after a step"""
    a = make("mobilenet_v2")
    b = copy.deepcopy(a)
    fuse_quietly(b)
    a.train(); b.train()
    x = torch.randn(4, 3, 16, 16)
    outs = []
    for m in (a, b):
        torch.manual_seed(5)
        y = m(x)
        y.square().mean().backward()
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    for (ka, ta), (kb, tb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(ta, tb), ka
    for (ka, pa), (kb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), ka
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), ka
    # then evaluated without re-fusing: the new running statistics are folded
    a.eval(); b.eval()
    assert rel(run(b, x), run(a, x)) <= 1e-6


def test_layer_ids_are_not_drawn_and_nothing_is_copied():
    from bayesian_torch_amd import rng
    m = make("vgg_bn")
    before = rng.next_layer_id()
    fuse_quietly(m)
    assert rng.next_layer_id() == before + 1


def test_pickle_round_trip_second_call_and_bn_edits():
    from bayesian_torch_amd.models import fuse_model
    from bayesian_torch_amd.models.fuse import _FusedForward
    m = make("mobilenet_v2")
    ref_model = copy.deepcopy(m)
    x = torch.randn(2, 3, 16, 16)
    assert fuse_quietly(m) == 8
    assert fuse_model(m) == 0
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    assert isinstance(m2.__dict__.get("forward"), _FusedForward)
    assert fuse_model(m2) == 0
    assert rel(run(m2, x), run(m, x)) <= 1e-6
    m3 = copy.deepcopy(m)
    out3 = run(m3, x)
    assert all(s.v is not t.v for s, t in zip(m3.forward.sites, m.forward.sites))
    assert rel(out3, run(m, x)) <= 1e-6
    # an in-place BN edit after fusing shows up in the fused output
    before = run(m, x)
    for mm in (m, ref_model):
        with torch.no_grad():
            mm.blocks[0].bn3.weight.mul_(3.0)
            mm.head[1].running_mean.add_(0.5)
    after = run(m, x)
    assert rel(after, before) > 1e-3
    assert rel(after, run(ref_model, x)) <= 1e-6


def test_linear_bn1d_folds_only_for_2d_outputs():
    class Seq3d(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(6, 5)
            self.bn = nn.BatchNorm1d(5)

        def forward(self, x):
            return torch.relu(self.bn(self.fc(x)))
    from bayesian_torch_amd.models import dnn_to_bnn
    torch.manual_seed(0)
    m = Seq3d()
    dnn_to_bnn(m, PRIOR)
    m.bn.running_mean.normal_()
    m.eval()
    x2 = torch.randn(4, 6)
    r2 = run(m, x2)
    assert fuse_quietly(m) == 1
    assert rel(run(m, x2), r2) <= 1e-6
    # [N, 5, 6] -> Linear(6, 5) -> [N, 5, 5]: BatchNorm1d normalises axis 1 (not the Linear's features): original ops
    x3 = torch.randn(3, 5, 6)
    m_ref = Seq3d()
    dnn_to_bnn(m_ref, PRIOR)
    m_ref.load_state_dict(m.state_dict())
    m_ref.eval()
    assert torch.equal(run(m, x3), run(m_ref, x3))


def test_forward_fused_relu6_and_act_keyword_on_cpu():
    from bayesian_torch_amd import layers as L
    torch.manual_seed(0)
    layer = L.Conv2dFlipout(4, 6, 3, padding=1)
    layer.dnn_to_bnn_flag = True
    x = torch.randn(2, 4, 5, 5) * 10
    scale = torch.rand(6) + 2
    shift = torch.randn(6)
    outs = {}
    for k, kw in (("none", dict(relu=False)), ("relu", dict(relu=True)), ("relu6", dict(relu="relu6")),
                  ("relu6b", dict(act="relu6"))):
        torch.manual_seed(9)
        with torch.no_grad():
            outs[k] = layer.forward_fused(x, scale, shift, None, **kw)
    assert torch.equal(outs["relu"], outs["none"].clamp_min(0))
    assert torch.equal(outs["relu6"], outs["none"].clamp(0, 6))
    assert torch.equal(outs["relu6b"], outs["relu6"])
    assert float(outs["none"].max()) > 6
    with pytest.raises(ValueError):
        layer.forward_fused(x, scale, shift, None, act="gelu")


class DropoutHead(nn.Module):
    """conv-BN-ReLU, then functional dropout keyed on self.training (a constant to a tracer), then the classifier"""

    def __init__(self):
        super().__init__()
        self.c = nn.Conv2d(3, 8, 3, padding=1)
        self.bn = nn.BatchNorm2d(8)
        self.fc = nn.Linear(8 * 8 * 8, 10)

    def forward(self, x):
        y = torch.relu(self.bn(self.c(x)))
        y = F.dropout(y, 0.5, training=self.training)
        return self.fc(y.flatten(1))


def _dropout_pair():
    from bayesian_torch_amd.models import dnn_to_bnn
    torch.manual_seed(0)
    a = DropoutHead()
    dnn_to_bnn(a, PRIOR)
    with torch.no_grad():
        a.bn.running_mean.normal_(0, 0.2)
        a.bn.running_var.uniform_(0.5, 1.5)
    b = copy.deepcopy(a)
    return a, b


def test_fused_in_eval_then_trained_keeps_the_training_mode_code():
    """the rewrite is traced in eval mode: switched to training, the fused model runs its dropout (and batch statistics)"""
    a, b = _dropout_pair()
    a.eval(); b.eval()
    assert fuse_quietly(b) == 1
    x = torch.randn(4, 3, 8, 8)
    assert rel(run(b, x), run(a, x)) <= 1e-6
    a.train(); b.train()
    ya, yb = run(a, x), run(b, x)
    assert torch.equal(ya, yb)
    assert a.bn.running_mean.equal(b.bn.running_mean)
    a.eval(); b.eval()
    assert rel(run(b, x), run(a, x)) <= 1e-6


def test_loaded_model_first_called_in_training_mode_still_evaluates_without_dropout():
    a, b = _dropout_pair()
    b.eval()
    fuse_quietly(b)
    buf = io.BytesIO()
    torch.save(b, buf)
    buf.seek(0)
    c = torch.load(buf, weights_only=False)
    x = torch.randn(4, 3, 8, 8)
    a.train(); c.train()
    assert torch.equal(run(c, x), run(a, x))
    a.eval(); c.eval()
    assert rel(run(c, x), run(a, x)) <= 1e-6
    assert len(c.forward.sites) == 1  # rebuilt (in eval mode) on the first eval call: still fused


def test_hooks_on_inlined_modules_are_kept():
    """a hook on a traced-through block: fuse_model falls back (one warning) and the hook fires on every call; a hook
    added after fusing makes the model run its own forward"""
    from bayesian_torch_amd.models import fuse_model
    m = make("mobilenet_v2")
    calls = []
    m.blocks[0].register_forward_hook(lambda mod, i, o: calls.append(1))
    x = torch.randn(2, 3, 16, 16)
    ref = run(m, x)
    calls.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        n = fuse_model(m)
    assert n == 2  # the stem and head Sequentials
    assert any("hooks" in str(i.message) for i in w)
    assert calls == []  # nothing ran on proxies
    assert rel(run(m, x), ref) <= 1e-6 and calls == [1]

    m2 = make("mobilenet_v2")
    assert fuse_quietly(m2) == 8
    ref2 = run(m2, x)
    h = m2.blocks[1].register_forward_hook(lambda mod, i, o: calls.append(2))
    assert rel(run(m2, x), ref2) <= 1e-6 and calls[-1] == 2
    h.remove()


def test_residual_computed_after_the_layer():
    """ResNet-style block whose identity branch runs after conv2: the site runs behind the residual; eval output unchanged
    on the GPU-keyed noise, and on the CPU with the means (rho -> -40) regardless of the draw order"""
    from bayesian_torch_amd.models import dnn_to_bnn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.b1 = nn.Conv2d(8, 16, 3, 2, 1, bias=False), nn.BatchNorm2d(16)
            self.c2, self.b2 = nn.Conv2d(16, 16, 3, 1, 1, bias=False), nn.BatchNorm2d(16)
            self.down = nn.Sequential(nn.Conv2d(8, 16, 1, 2, bias=False), nn.BatchNorm2d(16))

        def forward(self, x):
            out = self.b2(self.c2(torch.relu(self.b1(self.c1(x)))))
            idt = self.down(x)
            out += idt
            return torch.relu(out)
    torch.manual_seed(0)
    m = Block()
    dnn_to_bnn(m, PRIOR)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.rsplit(".", 1)[-1].startswith("rho_"):
                p.fill_(-40.0)
    m.eval()
    x = torch.randn(2, 8, 8, 8)
    ref = run(m, x)
    assert fuse_quietly(m) == 3
    assert rel(run(m, x), ref) <= 1e-6
