"""Eval-mode BatchNorm (+ residual, + ReLU) folded into the variational convolutions of a ResNet — SURVEY §8(f)-3,
"the step either side of the path" (reference block structure: models/deterministic/resnet_large.py:46-62, 85-105,
156-171).  `fuse_resnet(model)` rewrites, in place, every block that looks like a torchvision BasicBlock / Bottleneck
(conv1,bn1,conv2,bn2[,conv3,bn3],downsample) whose convs are variational layers, and the stem (conv1,bn1,relu).
The module tree is untouched (state_dict keys of the fused and the unfused model are identical; checkpoints load either
way) and the folded (scale, shift) follow the BatchNorm tensors.  Only for inference (`model.eval()`); the unfused model
is the parity reference (tests/test_gpu_model.py).
"""
import types

import torch
import torch.nn as nn


STEM_POOL_FUSION = True  # conv1 -> bn1 -> relu -> maxpool as one launch when the geometry allows (btx_contract_pool_shape)


def fold_bn(bn):
    """eval-mode BatchNorm as y = x*scale + shift (f32)"""
    with torch.no_grad():
        w = bn.weight.float() if bn.weight is not None else torch.ones_like(bn.running_var, dtype=torch.float32)
        b = bn.bias.float() if bn.bias is not None else torch.zeros_like(bn.running_var, dtype=torch.float32)
        scale = w / torch.sqrt(bn.running_var.float() + bn.eps)
        shift = b - bn.running_mean.float() * scale
    return scale.contiguous(), shift.contiguous()


def _is_var(m):
    return hasattr(m, "forward_fused")


def _is_q8(m):
    """a quantized (INT8) twin: a leaf of the trace and never an epilogue site — its BatchNorm folding happens in
    models.bnn_to_qbnn(fuse_conv_bn=True), its ReLU is the layer's own `relu` attribute"""
    return getattr(m, "_btx_q8", False)


def _is_lstm(m):
    """a Bayesian LSTM: a leaf of the trace (its forward loops over the time steps), never an epilogue site; fuse_model switches
    it to its fused sequence path (fused_sequence)"""
    return hasattr(m, "fused_sequence") and hasattr(m, "ih") and hasattr(m, "hh")


# ---- "is this module's forward the dataflow the fused forms assume?" — decided by RUNNING it, not by its class name -------------
# Attribute names prove nothing about a forward (a pre-activation block has conv1 / bn1 / conv2 / bn2 / downsample too), and a
# class-name list stops at the classes it knows.  A deep copy of the module on the CPU, in eval mode, is run twice on a small random
# input — once through its CLASS's forward, once through the textbook dataflow below — and must agree.  The copy's rho parameters
# are set to -40 first (sigma ~ 4e-18): its variational layers then compute with their means whatever noise they draw, so the two
# runs do not have to call the layers in the same order.  A module that fails the probe is left alone, with a warning.
def _out(o):
    return o[0] if isinstance(o, tuple) else o


def _textbook_block(m, x):
    """reference models/deterministic/resnet_large.py:46-62 (BasicBlock), 85-105 (Bottleneck)"""
    y = torch.relu(m.bn1(_out(m.conv1(x))))
    y = m.bn2(_out(m.conv2(y)))
    if hasattr(m, "conv3") and hasattr(m, "bn3"):
        y = m.bn3(_out(m.conv3(torch.relu(y))))
    idt = x if m.downsample is None else m.downsample(x)
    return torch.relu(y + _out(idt))


def _textbook_resnet(m, x):
    """resnet_large.py:156-171"""
    x = m.maxpool(torch.relu(m.bn1(_out(m.conv1(x)))))
    x = m.layer4(m.layer3(m.layer2(m.layer1(x))))
    return _out(m.fc(m.avgpool(x).flatten(1)))


def _behaves_like(m, ref_fn, shapes):
    import copy
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            probe = copy.deepcopy(m).to("cpu").float().eval()
            with torch.no_grad():
                for name, prm in probe.named_parameters():
                    if name.rsplit(".", 1)[-1].startswith("rho_"):
                        prm.fill_(-40.0)
        except Exception:  # noqa — a module that cannot be copied cannot be probed: not fused
            return False
        for shp in shapes:
            try:
                with torch.no_grad(), torch.random.fork_rng(devices=[]):
                    x = torch.randn(*shp, generator=torch.Generator().manual_seed(7))
                    torch.manual_seed(1234)
                    a = _out(type(probe).forward(probe, x))
                    torch.manual_seed(1234)
                    b = ref_fn(probe, x)
                return bool(a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=1e-6))
            except Exception:  # noqa — e.g. an input too small for the model's pooling: try the next shape
                continue
    return False


def _cin(conv):
    for k in ("in_channels", "in_features"):
        if hasattr(conv, k):
            return int(getattr(conv, k))
    return None


def block_is_textbook(m):
    """conv1 / bn1 / conv2 / bn2 [/ conv3 / bn3] / downsample with the reference's BasicBlock / Bottleneck dataflow (probed, cached)"""
    if "_btx_textbook" in m.__dict__:
        return m.__dict__["_btx_textbook"]
    ok = all(hasattr(m, k) for k in ("conv1", "bn1", "conv2", "bn2", "downsample")) and _cin(m.conv1) is not None
    if ok:
        ok = _behaves_like(m, _textbook_block, [(2, _cin(m.conv1), 8, 8)])
        if not ok:
            import warnings
            warnings.warn("bayesian_torch_amd.models.fuse: %s has conv1/bn1/conv2/bn2/downsample but not the ResNet block dataflow "
                          "(relu(bn(conv)) ... + identity, relu): left unfused" % type(m).__name__)
    object.__setattr__(m, "_btx_textbook", bool(ok))
    return bool(ok)


def resnet_is_textbook(model):
    """conv1 -> bn1 -> relu -> maxpool -> layer1..4 -> avgpool -> flatten -> fc (probed on a 64^2, then a 224^2 input; cached)"""
    if "_btx_textbook" in model.__dict__:
        return model.__dict__["_btx_textbook"]
    ok = all(hasattr(model, k) for k in ("conv1", "bn1", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool", "fc"))
    ok = ok and _cin(model.conv1) is not None
    if ok:
        c = _cin(model.conv1)
        ok = _behaves_like(model, _textbook_resnet, [(1, c, 64, 64), (1, c, 224, 224)])
        if not ok:
            import warnings
            warnings.warn("bayesian_torch_amd.models.fuse: %s has a ResNet's attributes but not its forward: stem / head left unfused"
                          % type(model).__name__)
    object.__setattr__(model, "_btx_textbook", bool(ok))
    return bool(ok)


class _Folded:
    """conv (variational) + eval-mode BN folded into the conv's store.  A plain object, NOT an nn.Module: it is attached
    with object.__setattr__, so the module tree — and with it state_dict() / load_state_dict() keys, .to(), .parameters()
    — is exactly that of the unfused model.  (scale, shift) are recomputed whenever the BN tensors change identity or
    version (load_state_dict, .to(device), in-place edits)."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        self._key, self._ss = None, None

    def _scale_shift(self):
        bn = self.bn
        ts = [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if key != self._key:
            self._ss, self._key = fold_bn(bn), key
        return self._ss

    def __call__(self, x, residual=None, relu=False, pool=False):
        scale, shift = self._scale_shift()
        return self.conv.forward_fused(x, scale, shift, residual, relu, pool=pool)


def _downsample(self, x):
    f = self.__dict__.get("_fds")
    if f is not None:
        return f(x)
    return x if self.downsample is None else self.downsample(x)


def _basic_forward(self, x):
    idt = _downsample(self, x)
    y = self._f1(x, None, True)
    return self._f2(y, idt, True)


def _bottleneck_forward(self, x):
    idt = _downsample(self, x)
    y = self._f1(x, None, True)
    y = self._f2(y, None, True)
    return self._f3(y, idt, True)


def fuse_resnet(model):
    n = 0
    for m in model.modules():
        names = [k for k in ("conv1", "bn1", "conv2", "bn2") if hasattr(m, k)]
        if (len(names) == 4 and hasattr(m, "downsample") and _is_var(m.conv1) and _is_var(m.conv2)
                and ("_f1" in m.__dict__ or block_is_textbook(m))):
            object.__setattr__(m, "_f1", _Folded(m.conv1, m.bn1))
            object.__setattr__(m, "_f2", _Folded(m.conv2, m.bn2))
            if hasattr(m, "conv3") and _is_var(m.conv3):
                object.__setattr__(m, "_f3", _Folded(m.conv3, m.bn3))
                m.forward = types.MethodType(_bottleneck_forward, m)
            else:
                m.forward = types.MethodType(_basic_forward, m)
            ds = m.downsample  # stays the original nn.Sequential(conv, bn): same keys, the folded call goes beside it
            if isinstance(ds, nn.Sequential) and len(ds) == 2 and _is_var(ds[0]) and isinstance(ds[1], nn.BatchNorm2d):
                object.__setattr__(m, "_fds", _Folded(ds[0], ds[1]))
            n += 1
    # stem: conv1 -> bn1 -> relu -> maxpool
    if (hasattr(model, "conv1") and hasattr(model, "bn1") and hasattr(model, "maxpool") and _is_var(model.conv1)
            and ("_stem" in model.__dict__ or resnet_is_textbook(model))):
        object.__setattr__(model, "_stem", _Folded(model.conv1, model.bn1))

        def pool(mp, y):
            """the stem's max-pool on the channels-last activations (own HBM-bound kernel when the geometry allows)"""
            ints = all(isinstance(v, int) for v in (mp.kernel_size, mp.stride, mp.padding, mp.dilation))
            if (y.is_cuda and isinstance(mp, nn.MaxPool2d) and ints and mp.dilation == 1 and not mp.ceil_mode
                    and not mp.return_indices and y.shape[1] % 8 == 0 and 2 * mp.padding <= mp.kernel_size
                    and y.dtype in (torch.float32, torch.bfloat16) and not torch.is_grad_enabled()):
                from .. import functional as BF
                return BF.maxpool2d_hip(y, mp.kernel_size, mp.stride, mp.padding)
            return mp(y)

        def stem_pool_fusable(self, x):
            """conv1 -> bn1 -> relu -> MaxPool2d(3, 2, 1) in ONE launch (btx_contract_stempool.h): the 112x112 conv
            output never reaches HBM.  Decided per input shape; everything else pools with its own kernel."""
            mp = self.maxpool
            if not STEM_POOL_FUSION:  # A/B measurements (bench.py --no-stem-pool)
                return False
            if not (isinstance(mp, nn.MaxPool2d) and mp.kernel_size in (3, (3, 3)) and mp.stride in (2, (2, 2))
                    and mp.padding in (1, (1, 1)) and mp.dilation in (1, (1, 1)) and not mp.ceil_mode
                    and not mp.return_indices and not torch.is_grad_enabled()):
                return False
            from .. import functional as BF
            cache = self.__dict__.setdefault("_stem_pool_ok", {})
            key = (tuple(x.shape), x.dtype, x.device, self.conv1.precision or BF.get_precision())
            if key not in cache:
                cache[key] = bool(self.conv1.pool_fusable(x))
            return cache[key]

        def fwd(self, x):
            if stem_pool_fusable(self, x):
                x = self._stem(x, None, True, pool=True)
            else:
                x = pool(self.maxpool, self._stem(x, None, True))
            x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
            ap = self.avgpool
            # the reference's nn.AvgPool2d(7, stride=1) on a 7x7 map (resnet_large.py:125) and torchvision's
            # AdaptiveAvgPool2d((1,1)) are both a global average
            is_global = (isinstance(ap, nn.AdaptiveAvgPool2d) and ap.output_size in (1, (1, 1))) or (
                isinstance(ap, nn.AvgPool2d) and ap.padding in (0, (0, 0)) and not ap.ceil_mode
                and ap.divisor_override is None
                and (ap.kernel_size if isinstance(ap.kernel_size, tuple) else (ap.kernel_size,) * 2) == tuple(x.shape[2:]))
            if (x.is_cuda and is_global and x.shape[1] % 8 == 0
                    and x.dtype in (torch.float32, torch.bfloat16) and not torch.is_grad_enabled()):
                from .. import functional as BF
                return self.fc(BF.avgpool_global_hip(x))
            return self.fc(ap(x).flatten(1))
        model.forward = types.MethodType(fwd, model)
        n += 1
    return n


def _basic_forward_train(self, x):
    if not (self.training and x.is_cuda):
        return self._btx_fwd_eval(x)
    from .. import autograd as _ag
    idt = x if self.downsample is None else self.downsample(x)
    y = _ag.bn_act(self.bn1, self.conv1(x))
    return _ag.bn_act(self.bn2, self.conv2(y), residual=idt)


def _bottleneck_forward_train(self, x):
    if not (self.training and x.is_cuda):
        return self._btx_fwd_eval(x)
    from .. import autograd as _ag
    idt = x if self.downsample is None else self.downsample(x)
    y = _ag.bn_act(self.bn1, self.conv1(x))
    y = _ag.bn_act(self.bn2, self.conv2(y))
    return _ag.bn_act(self.bn3, self.conv3(y), residual=idt)


_BN_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)


class _Bound:
    """`fn(module, ...)` as the module's instance-level `forward`.  Unlike a closure holding the ORIGINAL module's bound forward,
    copy.deepcopy gives the copy a _Bound on the COPY (an EMA / AveragedModel copy normalising with the original's weights and
    updating the original's running estimates was the bug), and unlike types.MethodType of a module-level function it pickles
    (torch.save(model)): `fn` goes by reference, the module through the pickler's memo."""
    __slots__ = ("fn", "__self__")

    def __init__(self, fn, module):
        self.fn, self.__self__ = fn, module

    def __call__(self, *a, **k):
        return self.fn(self.__self__, *a, **k)

    def __getstate__(self):
        return (self.fn, self.__self__)

    def __setstate__(self, st):
        self.fn, self.__self__ = st


# The fallback of both is the CLASS's forward on this very module.
def _bn_forward(self, x):
    from .. import autograd as _ag
    if _ag.bn_train_usable(self, x):
        return _ag.batch_norm_train(self, x)
    return type(self).forward(self, x)


def _mp_forward(self, x):
    from .. import autograd as _ag
    if _ag.max_pool_train_usable(self, x):
        return _ag.max_pool_train(self, x)
    return type(self).forward(self, x)


def _resnet_forward_train(self, x):
    if not (self.training and x.is_cuda):
        return self._btx_fwd_eval(x)
    from .. import autograd as _ag
    x = self.maxpool(_ag.bn_act(self.bn1, self.conv1(x)))
    x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
    return self.fc(self.avgpool(x).flatten(1))


def _plain_block(m):
    """a block whose forward IS the textbook one — conv / bn pairs, ReLU, `downsample` — decided by running it (block_is_textbook):
    the classes of models/resnet.py and torchvision.models.resnet pass, so does a user's own block with the same dataflow; a block
    that merely has the same attribute names does not"""
    return (isinstance(getattr(m, "relu", None), nn.ReLU)
            and all(isinstance(getattr(m, k, None), nn.modules.batchnorm._BatchNorm) for k in ("bn1", "bn2"))
            and block_is_textbook(m))


def hip_batchnorm(model, fuse_act=True):
    """Route the TRAINING-mode forward (and backward) of every nn.BatchNorm{1,2,3}d of `model` through libbtx
    (csrc/btx_bn.hip) whenever the call qualifies — CUDA, f32 / bf16, channels-last storage, C % 8 == 0
    (autograd.bn_train_usable) — and leave everything else (eval mode, CPU, other layouts) to torch.  The module tree,
    parameters, buffers and state_dict keys are untouched; results match F.batch_norm to rounding.  The reference's training
    loop (README.md:114-125) spends a third of a ResNet18 step in ATen's channels-last BatchNorm kernels.

    fuse_act: the blocks and the stem of models/resnet.py / torchvision.models.resnet (the architecture of the reference's
    models/deterministic/resnet_large.py:46-62, 85-105) also get their `relu(bn(.))` and
    `relu(bn(.) + identity)` inside the normalisation's launches while training on the GPU (one rounding instead of two or three;
    the ReLU's backward mask is a bit per element written by the forward).  Eval mode and CPU tensors keep the forward the block
    had (the eval-mode folding of fuse_resnet included).  nn.MaxPool2d modules are routed the same way where a gradient is
    needed (btx_maxpool2d_cl_train / _bwd).  Returns the number of BatchNorm modules routed."""
    n = 0
    for m in model.modules():
        if type(m) in _BN_TYPES and "_btx_bn_orig" not in m.__dict__:
            # exact nn.BatchNorm{1,2,3}d only: nn.SyncBatchNorm (cross-rank statistics) and the Lazy* variants (parameters
            # that do not exist yet) are _BatchNorm subclasses too and keep torch's own forward
            object.__setattr__(m, "_btx_bn_orig", True)
            m.forward = _Bound(_bn_forward, m)
            n += 1
        elif type(m) is nn.MaxPool2d and "_btx_mp_orig" not in m.__dict__:
            # the pooling layer behind the stem under autograd: btx_maxpool2d_cl_train / _bwd (a byte per output element instead of
            # ATen's int64 indices); everything outside autograd.max_pool_train_usable keeps torch's op
            object.__setattr__(m, "_btx_mp_orig", True)
            m.forward = _Bound(_mp_forward, m)
    if fuse_act:
        for m in model.modules():
            if _plain_block(m) and "_btx_fwd_eval" not in m.__dict__:
                object.__setattr__(m, "_btx_fwd_eval", m.forward)
                three = hasattr(m, "conv3") and hasattr(m, "bn3")
                m.forward = types.MethodType(_bottleneck_forward_train if three else _basic_forward_train, m)
        if (isinstance(getattr(model, "relu", None), nn.ReLU) and "_btx_fwd_eval" not in model.__dict__
                and all(hasattr(model, k) for k in ("conv1", "bn1", "maxpool", "layer1", "layer4", "avgpool", "fc"))
                and resnet_is_textbook(model)):
            object.__setattr__(model, "_btx_fwd_eval", model.forward)
            model.forward = types.MethodType(_resnet_forward_train, model)
    return n


# ---- fuse_model: the same store-side folding for any model, found on its traced dataflow ---------------------------------------
# A "site" is a chain that starts at a variational layer V (anything with forward_fused) and whose every intermediate value has
# exactly one user:  V -> BN [-> + other] [-> ReLU | ReLU6]  or  V -> ReLU | ReLU6.  The chain's ops are replaced by ONE call of
# the site, which runs V.forward_fused (the BN as scale / shift, the add as residual, the activation in the store) in eval mode
# and the original ops otherwise.  The module tree is not touched: the sites and the rewritten forward are plain objects.
import operator as _operator  # noqa: E402

import torch.nn.functional as _F  # noqa: E402

_RELU_FUNCS = (torch.relu, torch.relu_, _F.relu, _F.relu_)
_RELU6_FUNCS = (_F.relu6,)
_ADD_FUNCS = (_operator.add, _operator.iadd, torch.add)


class _SiteFold(_Folded):
    """_Folded whose key also follows num_batches_tracked: a training-mode forward updates the running statistics in place
    without bumping their version counters, the step counter it increments does"""

    def _scale_shift(self):
        bn = self.bn
        ts = [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked) if t is not None]
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if key != self._key:
            self._ss, self._key = fold_bn(bn), key
        return self._ss


class _Site:
    """One fused chain.  `steps`: the chain's original ops behind V, replayed when the site cannot run fused — (kind, target,
    args, kwargs) with _CUR standing for the chain's running value and _RES for the residual."""

    def __init__(self, v, bn, steps, act, has_res):
        self.v, self.bn, self.steps, self.act, self.has_res = v, bn, steps, act, has_res
        self.folded = _SiteFold(v, bn) if bn is not None else None
        # the modules the fused call would bypass: one with hooks runs the original ops, so its hooks fire
        self.mods = [v] + [t for k, t, _, _ in steps if k == "call_module"]
        self.__name__ = "btx_fused_site"  # (torch.fx code generation names the call after it)

    def _fusable(self, x, residual):
        v, bn = self.v, self.bn
        if v.training or (bn is not None and bn.training):
            return False  # training mode: batch statistics, running-stat updates, autograd — the original ops
        if any(_hooked(m) for m in self.mods):
            return False
        op = getattr(v, "_op", None)
        if op is None:
            return False
        if bn is not None:
            if bn.num_features != op.out_channels or bn.running_mean is None:
                return False
            if op.nd == 0 and x.dim() != 2:
                return False  # Linear -> BatchNorm1d normalises the channel axis only for [batch, features] outputs
        if residual is not None:
            if not torch.is_tensor(residual) or residual.dtype != x.dtype or residual.device != x.device:
                return False
            if op.nd == 0:
                shape = tuple(x.shape[:-1]) + (op.out_channels,)
            else:
                if x.dim() != op.nd + 2:
                    return False
                sp = (1,) * (3 - op.nd) + tuple(x.shape[2:])
                shape = (x.shape[0], op.out_channels) + op.out_spatial(sp)[3 - op.nd:]
            if tuple(residual.shape) != shape:
                return False
        return True

    def __call__(self, x, residual=None):
        if self._fusable(x, residual):
            scale, shift = self.folded._scale_shift() if self.folded is not None else (None, None)
            return self.v.forward_fused(x, scale, shift, residual, act=self.act)
        y = self.v(x)
        for kind, target, args, kwargs in self.steps:
            args = tuple(y if a is _CUR else residual if a is _RES else a for a in args)
            if kind == "call_method":
                y = getattr(args[0], target)(*args[1:], **kwargs)
            else:
                y = target(*args, **kwargs)
        return y


def _hooked(m):
    return bool(m._forward_hooks or m._forward_pre_hooks)


class _Marker:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name


_CUR, _RES = _Marker("_CUR"), _Marker("_RES")


def _act_of(node, modules):
    """'relu' / 'relu6' when the fx node applies ReLU / ReLU6 to its first argument (and nothing else), else None"""
    if node.op == "call_module":
        m = modules.get(node.target)
        if len(node.args) != 1 or node.kwargs:
            return None
        if type(m) is nn.ReLU:
            return "relu"
        if type(m) is nn.ReLU6 or (type(m) is nn.Hardtanh and m.min_val == 0.0 and m.max_val == 6.0):
            return "relu6"
        return None
    if node.op == "call_function":
        extra = set(node.kwargs) - {"inplace"}
        if extra or len(node.args) > (2 if node.target in (_F.relu, _F.relu6) else 1):
            return None
        if node.target in _RELU_FUNCS:
            return "relu"
        if node.target in _RELU6_FUNCS:
            return "relu6"
        return None
    if node.op == "call_method" and node.target in ("relu", "relu_") and len(node.args) == 1 and not node.kwargs:
        return "relu"
    return None


def _is_add(node):
    if node.op == "call_function" and node.target in _ADD_FUNCS:
        return len(node.args) == 2 and not node.kwargs
    return node.op == "call_method" and node.target in ("add", "add_") and len(node.args) == 2 and not node.kwargs


def _only_user(node):
    users = list(node.users)
    return users[0] if len(users) == 1 else None


def _bn_ok(m):
    return type(m) in _BN_TYPES and m.track_running_stats


def _match_site(node, modules):
    """(site, chain nodes, residual node) for the chain that starts at the call of V `node`, or None"""
    v = modules[node.target]
    if len(node.args) != 1 or node.kwargs:
        return None
    chain, steps, bn, act, res = [node], [], None, None, None
    cur = node
    u = _only_user(cur)
    if u is not None and u.op == "call_module" and _bn_ok(modules.get(u.target)) and u.args == (cur,) and not u.kwargs:
        bn = modules[u.target]
        chain.append(u); steps.append(("call_module", bn, (_CUR,), {}))
        cur = u
        u = _only_user(cur)
        if u is None:
            return None  # the normalised value has several users (or none): the chain is left alone
        if u is not None and _is_add(u) and isinstance(u.args[0], torch.fx.Node) and isinstance(u.args[1], torch.fx.Node):
            a0, a1 = u.args
            inplace = u.target in (_operator.iadd, "add_")
            other = a1 if a0 is cur else a0 if (a1 is cur and not inplace) else None  # in place: only the chain's value changes
            if other is not None and other is not cur:
                res = other
                chain.append(u)
                steps.append((u.op, u.target, tuple(_CUR if a is cur else _RES for a in u.args), {}))
                cur = u
                u = _only_user(cur)
    if u is not None and u.args and u.args[0] is cur:
        act = _act_of(u, modules)
        if act is not None:
            chain.append(u)
            target = modules[u.target] if u.op == "call_module" else u.target
            steps.append((u.op, target, (_CUR,) + tuple(u.args[1:]), dict(u.kwargs)))
    if bn is None and act is None:
        return None
    return _Site(v, bn, steps, act or "none", res is not None), chain, res


class _Tracer(torch.fx.Tracer):
    """variational layers and torch.nn modules (not containers) are leaves: their calls stay single nodes"""

    def is_leaf_module(self, m, qualname):
        # (an MCDropout is a leaf and no epilogue site: it stays where it is and nothing is folded across it)
        return _is_var(m) or _is_lstm(m) or _is_q8(m) or getattr(m, "_btx_dropout", False) or super().is_leaf_module(m, qualname)


def _inlined(module):
    """the modules whose forward code the trace inlines: `module` and every non-leaf module reached without passing a leaf"""
    tr, out, todo = _Tracer(), [], [module]
    while todo:
        m = todo.pop()
        out.append(m)
        todo.extend(c for c in m.children() if not tr.is_leaf_module(c, ""))
    return out


def _trace(module):
    """the fx graph of `module`'s forward in EVAL mode: a traced forward reads `self.training` as a constant, so the flags of the
    whole tree are False while tracing (and restored after); _FusedForward runs the class's forward whenever an inlined module
    is in training mode"""
    mods = list(module.modules())
    flags = [m.training for m in mods]
    try:
        for m in mods:
            m.training = False
        return _Tracer().trace(module)
    finally:
        for m, t in zip(mods, flags):
            m.training = t


def _rewrite(module, graph):
    """replace every site of the traced `graph` by one call; returns (compiled forward, sites)"""
    modules = dict(module.named_modules())
    sites, covered = [], set()
    for node in list(graph.nodes):
        if node.op != "call_module" or not _is_var(modules.get(node.target)) or node.graph is not graph:
            continue
        if node.target in covered or not node.users:
            continue
        m = _match_site(node, modules)
        if m is None:
            continue
        site, chain, res = m
        # the site runs where V ran, or right behind the residual when that is computed later: the ops between keep their
        # order relative to V as far as the dataflow allows
        anchor = node
        if res is not None:
            order = {n: i for i, n in enumerate(graph.nodes)}  # (earlier sites added nodes)
            if order[res] > order[node]:
                anchor = res
        with graph.inserting_after(anchor):
            new = graph.call_function(site, (node.args[0], res) if res is not None else (node.args[0],))
        chain[-1].replace_all_uses_with(new)
        for n in reversed(chain):
            graph.erase_node(n)
        sites.append(site)
        covered.add(node.target)
    graph.lint()
    code = graph.python_code(root_module="self")
    glb = dict(code.globals)
    exec(compile(code.src, "<fuse_model %s>" % type(module).__name__, "exec"), glb)  # noqa: S102 — fx-generated source
    return glb["forward"], sites


def _seq_sites(seq):
    """peephole over the consecutive children of one nn.Sequential: [(start index, length, site)]"""
    kids = list(seq)
    out, i = [], 0
    while i < len(kids):
        if not _is_var(kids[i]):
            i += 1
            continue
        j, bn, act, steps = i + 1, None, None, []
        if j < len(kids) and _bn_ok(kids[j]):
            bn = kids[j]; steps.append(("call_module", bn, (_CUR,), {})); j += 1
        if j < len(kids):
            k = kids[j]
            if type(k) is nn.ReLU:
                act = "relu"
            elif type(k) is nn.ReLU6 or (type(k) is nn.Hardtanh and k.min_val == 0.0 and k.max_val == 6.0):
                act = "relu6"
            if act is not None:
                steps.append(("call_module", k, (_CUR,), {})); j += 1
        if bn is None and act is None:
            i += 1
            continue
        out.append((i, j - i, _Site(kids[i], bn, steps, act or "none", False)))
        i = j
    return out


class _FusedForward:
    """the rewritten forward, installed as the module's instance-level `forward`.  It pickles (and deep-copies) as the module
    alone: the copy rebuilds its sites from its own modules on its first call — the same deterministic rewrite — so it is
    fused, and no site of the copy points at the original's layers."""

    def __init__(self, module, mode, fn=None, sites=None):
        self.module, self.mode, self.fn, self.sites = module, mode, fn, sites
        self.inlined = _inlined(module) if mode == "fx" else None

    def _build(self):
        if self.mode == "fx":
            self.fn, self.sites = _rewrite(self.module, _trace(self.module))
            self.inlined = _inlined(self.module)
        else:
            self.sites = _seq_sites(self.module)
            self.fn = None

    def __call__(self, *args, **kwargs):
        if self.mode == "fx":
            # the rewrite was traced in eval mode and inlines the forward code (and skips the hooks) of these modules: in
            # training mode, or with hooks on one of them, the class's own forward runs — the model as it was before fusing
            inl = self.inlined if self.inlined is not None else _inlined(self.module)
            if any(m.training for m in inl) or any(_hooked(m) for m in inl[1:]):
                return type(self.module).forward(self.module, *args, **kwargs)
            if self.sites is None:
                self._build()
            return self.fn(self.module, *args, **kwargs)
        if self.sites is None:
            self._build()
        (x,) = args
        kids = list(self.module)
        starts = {i: (n, s) for i, n, s in self.sites}
        i = 0
        while i < len(kids):
            if i in starts:
                n, s = starts[i]
                x = s(x)
                i += n
            else:
                x = kids[i](x)
                i += 1
        return x

    def __getstate__(self):
        return (self.module, self.mode)

    def __setstate__(self, st):
        self.module, self.mode = st
        self.fn, self.sites, self.inlined = None, None, None


def _lstm_training(model, on):
    if on:
        for m in model.modules():
            if _is_lstm(m):
                m.fused_training = True


def _lrt_training(model, on):
    if on:
        for m in model.modules():
            if getattr(m, "_family", None) == "lrt" and hasattr(m, "_btx_layer_id"):
                m.fused_training = True


def fuse_model(model, lstm_training=False, lrt_training=False):
    """Fold eval-mode BatchNorm, residual adds and ReLU / ReLU6 into the store of the variational layers of ANY model converted
    by dnn_to_bnn (its variational layers return a tensor), in place.  The model's forward is traced with torch.fx (variational
    layers and torch.nn modules as leaves) and every chain

        V -> BatchNorm{1,2,3}d [-> + other] [-> ReLU | ReLU6]      V -> ReLU | ReLU6

    whose intermediate values have exactly one user becomes one V.forward_fused call (BtxEpilogue: scale / shift, residual, relu
    1 / 2).  ReLU: nn.ReLU, F.relu, torch.relu, Tensor.relu (and the in-place forms); ReLU6: nn.ReLU6, F.relu6,
    nn.Hardtanh(0, 6); the add: `+`, torch.add, operator.add / iadd without alpha.  A BatchNorm qualifies with
    track_running_stats=True.  The forward is traced in eval mode; whenever a module whose code the trace inlined (the model, its
    containers and blocks) is in training mode or has forward hooks, the model's class forward runs instead — so a fused model
    trains exactly like the unfused one and can be evaluated afterwards without re-fusing.  At call time a site itself runs the
    ORIGINAL ops whenever its BatchNorm or layer is in training mode, one of its modules has hooks, a Linear -> BatchNorm1d
    output is not 2-D, or the residual does not have the output's shape and dtype.  A fused site runs V where V ran, or right
    behind its residual when that is computed later (a ResNet `downsample`): on the CPU, whose noise comes from torch's
    generator, such a model then draws its noise in another order than the unfused one (the GPU's noise is keyed per layer).  The folded (scale, shift) follow the BatchNorm tensors (load_state_dict, .to(),
    in-place edits).  The module tree, state_dict keys and parameters are unchanged; nothing is copied, moved or sampled.
    A model whose forward cannot be traced (control flow on tensor values), or whose inlined modules have forward hooks at
    fusing time, gets the folding inside its nn.Sequential containers only (consecutive children V, BN, activation), with one
    warning.  Every Bayesian LSTM (LSTMReparameterization / LSTMFlipout) is a leaf of the trace and gets fused_sequence = True:
    its inference forwards on the GPU run the whole sequence in one btx_lstm_fwd call.  Returns the number of fused sites plus
    the number of LSTMs switched; a second call returns 0.  lstm_training=True also sets fused_training on every Bayesian LSTM:
    its training forwards on the GPU then run btx_lstm_fwd_train and their backward btx_lstm_bwd (also inside
    autograd.GraphedTrainStep); it changes neither the count nor what the default call does.  lrt_training=True does the same for
    every ...LocalReparameterization layer (and for no other layer): GPU forwards that need gradients run btx_lrt_fwd_train /
    btx_lrt_bwd where functional.lrt_train_ok holds, the ATen composite elsewhere."""
    _lrt_training(model, lrt_training)
    if model.__dict__.get("_btx_fuse_model"):
        _lstm_training(model, lstm_training)
        return 0
    object.__setattr__(model, "_btx_fuse_model", True)
    lstms = [m for m in model.modules() if _is_lstm(m) and not m.fused_sequence]
    for m in lstms:
        m.fused_sequence = True
    _lstm_training(model, lstm_training)
    inl = set(map(id, _inlined(model)))
    hooked = [k for k, m in model.named_modules() if k and id(m) in inl and _hooked(m)]
    if hooked:  # (tracing would run the hooks on fx proxies, and the rewritten forward would skip them)
        return len(lstms) + _fuse_sequentials(model, "forward hooks on %s" % ", ".join(hooked))
    try:
        graph = _trace(model)
    except Exception as e:  # noqa — torch.fx.proxy.TraceError and whatever a forward raises on Proxy inputs
        return len(lstms) + _fuse_sequentials(model, "it could not be traced (%s: %s)"
                                              % (type(e).__name__, str(e).splitlines()[0] if str(e) else ""))
    fn, sites = _rewrite(model, graph)
    if not sites:
        return len(lstms)
    model.forward = _FusedForward(model, "fx", fn, sites)
    return len(lstms) + len(sites)


def _fuse_sequentials(model, why):
    import warnings
    n, covered = 0, set()
    seqs = [m for m in model.modules() if type(m) is nn.Sequential and not isinstance(m.__dict__.get("forward"), _FusedForward)]
    for seq in seqs:
        sites = _seq_sites(seq)
        if sites:
            seq.forward = _FusedForward(seq, "seq", None, sites)
            n += len(sites)
            covered.update(id(s.v) for _, _, s in sites)
    left = [k for k, m in model.named_modules() if _is_var(m) and id(m) not in covered]
    warnings.warn("bayesian_torch_amd.models.fuse.fuse_model: %s: %s; only chains inside nn.Sequential containers were fused "
                  "(%d); left unfused: %s" % (type(model).__name__, why, n, ", ".join(left) if left else "none"))
    return n
