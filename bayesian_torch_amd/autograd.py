"""Training path of the variational layers on the HIP backend (reference README.md:114-125:
`output = model(x); kl = get_kl_loss(model); loss = ce(output, y) + kl / batch_size; loss.backward()`).

BTX-RNG noise is a pure function of (seed, sample_idx, layer_id, element index), so nothing but (x, mu, rho) is saved for
the backward: eps and the Flipout signs are regenerated.

  forward        the fused HIP contraction (btx_contract_fwd), unchanged
  dx             ALSO btx_contract_fwd: the data gradient of  y = conv(x, mu) + s_out * conv(x * s_in, sigma*eps)  is
                 dx = convT(dy, mu) + s_in * convT(dy * s_out, sigma*eps)  — the same Flipout-shaped contraction on the
                 transposed geometry (stride-1 2-D convolutions: on the flipped kernel, which the tap-unrolled kernel
                 takes) with the two sign streams exchanged (BTX_FLAG_SWAP_SIGNS) and the forward's eps passed explicitly
  KL, dKL        btx_kl_gauss_model / btx_kl_gauss_model_bwd (one launch for the whole model)
  dmu, drho      btx_contract_wgrad: dW_mu = corr(x, dy) [and dW_delta = corr(x*s_in, dy*s_out) for Flipout] — a GEMM whose
                 reduction axis is the pixel axis, on the exact-f32 MFMA (csrc/btx_wgrad.hip); dmu = dW_mu and
                 drho = dW_delta * eps * sigmoid(rho) are elementwise follow-ups here.

Steps with num_mc > 1 Monte-Carlo samples (reference examples/main_bayesian_cifar.py:363-372): mc_train_forward is
the eager loop ([num_mc, B, C] logits, pass k on sample index step * num_mc + k), GraphedTrainStep(num_mc=n) the captured one (n
device sample words, one per pass).  A layer's backward regenerates the noise of the word its FORWARD read (kept on ctx), so passes
on different words can share one backward.  The loss head of the stack is utils.mc_loss (csrc/btx_mcloss.hip).
"""
import ctypes
import functools

import torch

from . import _lib
from . import functional as BF
from . import rng as _rng


def _first_order(backward):
    """Every backward here runs its kernels on detached tensors: a second derivative through it would be a constant.
    torch's once_differentiable turns that into an error only when the incoming gradient itself requires one; a gradient penalty
    (`torch.autograd.grad(out.sum(), x, create_graph=True)`) hands in a plain tensor and would get constants back without a word.  So the
    refusal is made here: a backward that autograd runs in grad mode (create_graph=True) raises."""
    inner = torch.autograd.function.once_differentiable(backward)

    @functools.wraps(backward)
    def guarded(ctx, *grads):
        if torch.is_grad_enabled():
            raise RuntimeError("bayesian_torch_amd: %s is first-order only (once_differentiable): its backward runs HIP kernels on "
                               "detached tensors, so create_graph=True would differentiate constants; use create_graph=False, or "
                               "backend 'torch' for second-order terms" % type(ctx).__name__)
        return inner(ctx, *grads)
    return guarded


def fast_dgrad_ok(layer):
    """the data gradient's weight operands in ONE launch (btx_dgrad_weights): Linear layers and 2-D convolutions on plain layouts
    (no channel padding, no row-fused stem, groups == 1); at stride 1 the padding must not exceed the dilated kernel extent"""
    op = layer._op
    if layer._btx_cpad is not None or op.transposed or op.groups != 1:
        return False
    if op.nd == 0:
        return True
    if op.nd == 2 and op.in_channels > 4:
        if op.stride == (1, 1, 1):
            return all(d * (k - 1) - p >= 0 for d, k, p in zip(op.dilation[1:], op.kernel[1:], op.padding[1:]))
        return True  # strided: the transposed geometry on the un-flipped, channel-transposed kernel (the same one launch)
    return False


def _data_grad_hip(layer, dy, x_shape, nz, sample_idx, hashed_signs, mu, rho, sdev=None, seed=None):
    """dx through libbtx: the contraction of dy with the (mu, sigma*eps) the FORWARD used (the tensors autograd saved) on
    the transposed geometry.  sdev: the device sample word the forward read (None: the host index `sample_idx`); seed: the
    BTX-RNG seed the forward ran under (None: the current one)"""
    seed = _rng.seed() if seed is None else seed
    op = layer._op
    kind = _lib.KIND_FLIPOUT if layer._family == "flipout" else _lib.KIND_REPARAM
    nd = op.nd
    if fast_dgrad_ok(layer) and (kind == _lib.KIND_REPARAM or hashed_signs):
        mu_p, rho_p = BF.gemm_major_view(mu.detach(), op), BF.gemm_major_view(rho.detach(), op)
        if nd == 0:
            opT, taps, flip = BF.OpDesc(0, op.out_channels, op.in_channels), 1, False
        elif op.stride == (1, 1, 1):
            pad = tuple(d * (k - 1) - p for d, k, p in zip(op.dilation[1:], op.kernel[1:], op.padding[1:]))
            opT = BF.OpDesc(2, op.out_channels, op.in_channels, op.kernel[1:], 1, pad, op.dilation[1:], 1)
            taps, flip = op.kernel[1] * op.kernel[2], True
        else:
            # strided: dx = convT(dy, W); its GEMM-major operands [C][tap][N] are the channel transpose of the forward's [N][tap][C]
            outpad = tuple((i + 2 * p - d * (k - 1) - 1) % s_ for i, p, d, k, s_ in
                           zip(x_shape[2:], op.padding[1:], op.dilation[1:], op.kernel[1:], op.stride[1:]))
            opT = BF.OpDesc(2, op.out_channels, op.in_channels, op.kernel[1:], op.stride[1:], op.padding[1:], op.dilation[1:], 1,
                            transposed=True, output_padding=outpad)
            taps, flip = op.kernel[1] * op.kernel[2], False
        w_mu, w_rho, w_eps = BF.dgrad_weights_hip(mu_p, rho_p, op.out_channels, taps, op.in_channels, flip, seed,
                                                  sample_idx, layer._btx_layer_id, sample_dev=sdev)
        dx = BF.contract_hip(kind, dy, w_mu, w_rho, None, None, opT, seed, sample_idx, layer._btx_layer_id,
                             prec=layer.precision, noise={"eps_w_packed": w_eps}, sample_dev=sdev,
                             extra_flags=_lib.FLAG_SWAP_SIGNS if kind == _lib.KIND_FLIPOUT else 0)
        return dx.reshape(x_shape) if nd == 0 else dx
    mu, rho, eps = mu.detach(), rho.detach(), nz["eps_w"]
    if nd == 0:
        opT = BF.OpDesc(0, op.out_channels, op.in_channels)
        w_mu, w_rho, w_eps = mu.t(), rho.t(), eps.t()
    elif op.transposed:
        # forward was a transposed convolution: its data gradient is the plain convolution with the same weight tensor
        opT = BF.OpDesc(nd, op.out_channels, op.in_channels, op.kernel[3 - nd:], op.stride[3 - nd:], op.padding[3 - nd:],
                        op.dilation[3 - nd:], op.groups)
        w_mu, w_rho, w_eps = mu, rho, eps
    elif nd == 2 and op.groups == 1 and op.stride == (1, 1, 1):
        # stride 1: convT(dy, W) == conv(dy, flip(W)^T) with padding d*(k-1) - p: a plain 3x3 again (tap-unrolled kernel)
        pad = tuple(d * (k - 1) - p for d, k, p in zip(op.dilation[1:], op.kernel[1:], op.padding[1:]))
        if min(pad) < 0:
            raise _lib.BtxError("data gradient: padding larger than the dilated kernel extent is not supported")
        opT = BF.OpDesc(2, op.out_channels, op.in_channels, op.kernel[1:], 1, pad, op.dilation[1:], 1)
        tr = lambda t: t.transpose(0, 1).flip(2, 3)  # noqa: E731
        w_mu, w_rho, w_eps = tr(mu), tr(rho), tr(eps)
    else:
        outpad = tuple((i + 2 * p - d * (k - 1) - 1) % s for i, p, d, k, s in
                       zip(x_shape[2:], op.padding[3 - nd:], op.dilation[3 - nd:], op.kernel[3 - nd:], op.stride[3 - nd:]))
        opT = BF.OpDesc(nd, op.out_channels, op.in_channels, op.kernel[3 - nd:], op.stride[3 - nd:], op.padding[3 - nd:],
                        op.dilation[3 - nd:], op.groups, transposed=True, output_padding=outpad)
        w_mu, w_rho, w_eps = mu, rho, eps
    noise = {"eps_w": w_eps}
    flags = 0
    if kind == _lib.KIND_FLIPOUT:
        if hashed_signs:
            flags = _lib.FLAG_SWAP_SIGNS
        else:  # padded forward layouts (C % 8 != 0, row-fused stems): the signs as tensors
            noise["sign_in"], noise["sign_out"] = nz["sign_out"], nz["sign_in"]
    dx = BF.contract_hip(kind, dy, BF.pack_gemm_major(w_mu.float(), opT), BF.pack_gemm_major(w_rho.float(), opT), None, None,
                         opT, seed, sample_idx, layer._btx_layer_id, prec=layer.precision, noise=noise,
                         extra_flags=flags, sample_dev=sdev)
    return dx.reshape(x_shape) if nd == 0 else dx


class ContractFn(torch.autograd.Function):
    """y = layer(x) on the HIP backend with gradients w.r.t. x, mu, rho, mu_b, rho_b"""

    @staticmethod
    def forward(ctx, layer, sample_idx, x, mu, rho, mu_b, rho_b):
        with torch.no_grad():
            out = layer._forward_hip(x, sample_idx=sample_idx)
        # the seed THIS forward ran under: bt.manual_seed() between forward and backward must not change the noise the backward regenerates
        ctx.layer, ctx.sample_idx, ctx.seed = layer, sample_idx, _rng.seed()
        # the device sample word THIS forward read: a step with several MC passes (num_mc > 1) points the layer at another word
        # before the next pass, and the backward must regenerate this pass's noise, not the last one's
        ctx.sample_dev = getattr(layer, "_btx_sample_dev", None)
        ctx.save_for_backward(x, mu, rho, rho_b)  # mu: the data gradient contracts with it (autograd's version check applies)
        return out

    @staticmethod
    @_first_order
    def backward(ctx, dy):
        layer, s, seed = ctx.layer, ctx.sample_idx, ctx.seed
        x, mu_s, rho, rho_b = ctx.saved_tensors
        op = layer._op
        flip = layer._family == "flipout"
        dy = dy.contiguous() if op.nd == 0 else dy
        with torch.no_grad():
            plan = layer._rowfuse_plan(x) if op.nd == 2 else None
            padded = layer._btx_cpad is not None or plan is not None   # forward noise indices run over padded layouts
            # sign TENSORS are only needed where the kernels cannot regenerate the hashed signs: channel-padded layouts, and
            # the data gradient / transposed weight gradient of a row-fused stem
            stem_wgrad = plan is not None and not op.transposed
            need_signs = flip and ((padded and (ctx.needs_input_grad[2] or not stem_wgrad)) or
                                   (op.transposed and rho_b is not None))  # transposed layers: db_delta by torch
            w_shape = tuple(rho.shape)
            fused_w = False  # dmu / drho formed by btx_rho_grad on the kernel's own buffers (plain layouts)
            # the noise TENSORS (eps, signs) are only materialised where something still needs them: the data gradient (it
            # contracts with the transposed / flipped sigma*eps), padded / transposed layouts, bias gradients
            plain_w = not op.transposed and not padded
            fast_dx = plain_w and fast_dgrad_ok(layer)  # the data gradient regenerates eps in its own operand pass
            need_nz = ((ctx.needs_input_grad[2] and not fast_dx) or not plain_w or need_signs or
                       (rho_b is not None and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6])))
            sdev = ctx.sample_dev  # captured step: eps / signs follow the device word the forward read, not `s`
            nz = layer.materialize_noise(s, tuple(x.shape), tuple(dy.shape), x.dtype, signs=need_signs, sample_dev=sdev,
                                         seed=seed) if need_nz else {}   # under the forward's seed, not the process-wide one of NOW
            dx = dmu = drho = dmu_b = drho_b = None
            kind = _lib.KIND_FLIPOUT if flip else _lib.KIND_REPARAM
            want_w = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
            want_b = rho_b is not None and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6])
            if want_w or want_b:
                signs = (nz["sign_in"], nz["sign_out"]) if (flip and padded and "sign_in" in nz) else None
                if plan is not None and not op.transposed:
                    # row-fused stem: the gradient on the geometry the forward ran on (7 kernel rows x 32 elements instead of
                    # 49 taps x 3 channels of a 64-wide tile; the forward's hashed signs instead of sign tensors)
                    dW, dWd, db, dbd = BF.wgrad_hip(kind, x, dy, op, seed, s, layer._btx_layer_id, w_shape,
                                                    bias=want_b, rowfuse=plan, sample_dev=sdev)
                elif not op.transposed and not padded:
                    # plain layouts: the kernel's GEMM-major buffers ARE the gradients (strided logical views, as the
                    # parameters themselves are stored), and drho = dW_delta * eps * sigmoid(rho) is one launch with eps
                    # regenerated in the kernel (btx_rho_grad) instead of fill_eps + unpack + sigmoid + two products
                    rho_f = BF.gemm_major_view(rho, op).reshape(-1) if want_w else None
                    if rho_f is not None and not rho_f.is_contiguous():
                        rho_f = rho_f.contiguous()
                    res = BF.wgrad_hip(kind, x, dy, op, seed, s, layer._btx_layer_id, w_shape, bias=want_b, raw=True,
                                       sample_dev=sdev, rho_flat=rho_f)
                    dWf, dWdf, db, dbd = res[:4]
                    if want_w:
                        drho_f = res[4]  # formed by the weight gradient's own reduction launch (btx_contract_wgrad_ws)
                        dmu = BF.gemm_major_logical_view(dWf, w_shape, op)
                        drho = BF.gemm_major_logical_view(drho_f, w_shape, op)
                    fused_w = True
                elif not op.transposed:
                    dW, dWd, db, dbd = BF.wgrad_hip(kind, x, dy, op, seed, s, layer._btx_layer_id, w_shape,
                                                    signs=signs, bias=want_b, sample_dev=sdev)
                else:
                    # y = convT(x, W): W is the weight of the plain convolution that maps y-space to x-space, so its
                    # gradient is corr(dy, x) on that geometry — x and dy (and the two sign streams) exchange roles
                    nd = op.nd
                    opc = BF.OpDesc(nd, op.out_channels, op.in_channels, op.kernel[3 - nd:], op.stride[3 - nd:],
                                    op.padding[3 - nd:], op.dilation[3 - nd:], op.groups)
                    sw = (signs[1], signs[0]) if signs is not None else None
                    dW, dWd, _, _ = BF.wgrad_hip(kind, dy, x, opc, seed, s, layer._btx_layer_id, w_shape, signs=sw,
                                                 swap=True, sample_dev=sdev)
                    db = dbd = None
                    if want_b:
                        red = tuple(i for i in range(dy.dim()) if i != 1)
                        db = dy.float().sum(red)
                        dbd = (dy.float() * nz["sign_out"].reshape(dy.shape).float()).sum(red) if flip else None
                if want_w and not fused_w:
                    dmu = dW
                    drho = (dWd if flip else dW) * nz["eps_w"] * torch.sigmoid(rho.detach())
                if want_b:
                    dmu_b = db
                    drho_b = (dbd if flip else db) * nz["eps_b"] * torch.sigmoid(rho_b.detach())
            if ctx.needs_input_grad[2]:
                hashed = flip and not padded
                dx = _data_grad_hip(layer, dy, tuple(x.shape), nz, s, hashed, mu_s, rho, sdev, seed)
                if dx.dtype != x.dtype:
                    dx = dx.to(x.dtype)
        return None, None, dx, dmu, drho, dmu_b, drho_b


class LrtFn(torch.autograd.Function):
    """y = layer(x) of a LocalReparameterization layer on the HIP backend with gradients w.r.t. x, mu, rho, mu_b, rho_b: the forward is
    btx_lrt_fwd_train (the kind-2 launch of inference, bit for bit, plus the f32 root: 4 bytes of saved state per output element), the
    backward ONE btx_lrt_bwd call (DESIGN.md §21 "Backward").  Channel-padded layers (the C = 3 stem) run both on the padded geometry
    the inference forward runs on; zeta indexes the output only, so padding does not move it."""

    @staticmethod
    def forward(ctx, layer, sample_idx, x, mu, rho, mu_b, rho_b):
        op = layer._op
        with torch.no_grad():
            mu_p, rho_p = BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op)
            xin = x
            if layer._btx_cpad is not None:
                extra = layer._btx_cpad - op.in_channels
                xin = BF.pad_channels(x, op, extra)
                mu_p = torch.nn.functional.pad(mu_p, (0, extra))   # zero weights meet zero activations
                rho_p = torch.nn.functional.pad(rho_p, (0, extra))
                op = layer._op_pad
            layer.__dict__["_btx_last_xshape"] = tuple(x.shape)
            sdev = getattr(layer, "_btx_sample_dev", None)
            seed = _rng.seed()  # kept on ctx: the backward regenerates zeta under the seed THIS forward ran under
            out, root = BF.lrt_fwd_train_hip(xin, mu_p, rho_p, mu_b.detach() if mu_b is not None else None,
                                             rho_b.detach() if rho_b is not None else None, op, seed, sample_idx,
                                             layer._btx_layer_id, prec=layer.precision, sample_dev=sdev)
        ctx.seed = seed
        ctx.layer, ctx.sample_idx, ctx.sample_dev = layer, sample_idx, sdev  # the device word THIS forward read (num_mc > 1)
        ctx.save_for_backward(x, root, mu, rho, rho_b)
        return out

    @staticmethod
    @_first_order
    def backward(ctx, dy):
        layer, s = ctx.layer, ctx.sample_idx
        x, root, mu, rho, rho_b = ctx.saved_tensors
        op0 = layer._op
        need = ctx.needs_input_grad
        with torch.no_grad():
            mu_p, rho_p = BF.gemm_major_view(mu, op0), BF.gemm_major_view(rho, op0)
            op, xin, extra = op0, x, 0
            if layer._btx_cpad is not None:
                extra = layer._btx_cpad - op0.in_channels
                xin = BF.pad_channels(x, op0, extra)
                mu_p = torch.nn.functional.pad(mu_p, (0, extra))
                rho_p = torch.nn.functional.pad(rho_p, (0, extra))
                op = layer._op_pad
            want_w = need[3] or need[4]
            want_b = rho_b is not None and (need[5] or need[6])
            dx, dmu_f, drho_f, dmu_b, drho_b = BF.lrt_bwd_hip(xin, dy, root, mu_p, rho_p,
                                                              rho_b.detach() if rho_b is not None else None, op, ctx.seed, s,
                                                              layer._btx_layer_id, prec=layer.precision, sample_dev=ctx.sample_dev,
                                                              want_x=need[2], want_w=want_w, want_b=want_b)
            dmu = drho = None
            if want_w:
                w_shape = tuple(rho.shape)
                if extra:  # the padded geometry's [N][tap][cpad] buffers: the real channels, as logical views
                    wp = (w_shape[0], layer._btx_cpad) + w_shape[2:]
                    dmu = BF.gemm_major_logical_view(dmu_f, wp, op)[:, :op0.in_channels]
                    drho = BF.gemm_major_logical_view(drho_f, wp, op)[:, :op0.in_channels]
                else:
                    dmu = BF.gemm_major_logical_view(dmu_f, w_shape, op)
                    drho = BF.gemm_major_logical_view(drho_f, w_shape, op)
            if dx is not None and extra:
                dx = dx[..., :op0.in_channels] if op0.nd == 0 else dx[:, :op0.in_channels]
        return (None, None, dx, dmu if need[3] else None, drho if need[4] else None, dmu_b if need[5] else None,
                drho_b if need[6] else None)


class DropoutFn(torch.autograd.Function):
    """y = MCDropout(x) on the HIP backend (BTX-DROP v1, btx_drop.hip).  Nothing is saved: the backward is the same launch on dy, its
    mask regenerated from (seed, layer id) and the sample index — or the device sample word — the forward read."""

    @staticmethod
    def forward(ctx, layer, sample_idx, x):
        # the device word THIS forward read (num_mc > 1 points the layer at another word before the next pass), as ContractFn keeps it
        sdev = layer.__dict__.get("_btx_sample_dev")
        ctx.meta = (layer._btx_T, layer._btx_scale, layer.mode, _rng.seed(), sample_idx, layer._btx_layer_id, sdev)
        return BF.dropout_hip(x, *ctx.meta[:6], sample_dev=sdev)

    @staticmethod
    @_first_order
    def backward(ctx, dy):
        return None, None, BF.dropout_hip(dy, *ctx.meta[:6], sample_dev=ctx.meta[6], backward=True)


class KlFn(torch.autograd.Function):
    """sum of the per-tensor mean KLs of `n` (mu, rho) pairs on the HIP backend, with gradients"""

    @staticmethod
    def forward(ctx, meta, *params):
        # meta: per pair (prior_mu, prior_sigma, prior_mu_t | None, prior_sigma_t | None, op | None)
        ctx.meta = meta
        ctx.save_for_backward(*params)
        return BF.kl_model_hip(_entries(meta, params))

    @staticmethod
    @_first_order
    def backward(ctx, g):
        params = ctx.saved_tensors
        meta = ctx.meta
        entries = _entries(meta, params)
        grads, outs = [], []
        for i, (pm, ps, pmt, pst, op) in enumerate(meta):
            mu, rho = params[2 * i], params[2 * i + 1]
            if pmt is None and op is not None:
                # The kernel reads (mu, rho) in GEMM-major order (_entries) — a zero-copy view of the parameter's storage or,
                # for parameters that are not stored that way (ConvTranspose with groups > 1, a parameter re-assigned
                # contiguous), a packed copy — and writes the gradients in the SAME element order: into GEMM-major buffers,
                # handed back as logical-shape views of those buffers.
                gpm = torch.empty_like(BF.gemm_major_view(mu, op))
                gpr = torch.empty_like(gpm)
                grads.append((gpm, gpr))
                outs.append((gpm, gpr, tuple(mu.shape), op))
            else:
                gm = torch.empty(mu.shape, dtype=torch.float32, device=mu.device)
                gr = torch.empty(rho.shape, dtype=torch.float32, device=rho.device)
                grads.append((gm, gr))
                outs.append((gm, gr, None, None))
        BF.kl_model_bwd_hip(entries, grads, g)
        res = []
        for gm, gr, shape, op in outs:  # (views where the layout has one, unpacked copies — made NOW — where it does not)
            if op is not None:
                gm, gr = BF.gemm_major_logical_view(gm, shape, op), BF.gemm_major_logical_view(gr, shape, op)
            res += [gm, gr]
        return (None,) + tuple(res)


class LstmTrainFn(torch.autograd.Function):
    """(hidden_seq, c_seq, kl) of a Bayesian LSTM on the HIP backend — btx_lstm_fwd_train, then btx_lstm_bwd for the backward
    through time — with gradients w.r.t. x, h0, c0, the (mu, rho) tensors of ih and hh and the two per-step KL terms.
    meta = (kind, seed, prec, (layer_id, sample_idx, sample_dev) of ih, the same of hh).  kl is the per-step sum of kl_ih + kl_hh
    over the T steps (the eager loop's order), so its backward hands T * g to both terms (KlFn outputs)."""

    @staticmethod
    def forward(ctx, meta, x, h0, c0, mu_i, rho_i, mub_i, rhob_i, mu_h, rho_h, mub_h, rhob_h, kl_i, kl_h):
        kind, seed, prec, mi, mh = meta
        d = lambda t: t.detach() if t is not None else None  # noqa: E731
        ih = (d(mu_i), d(rho_i), d(mub_i), d(rhob_i)) + tuple(mi)
        hh = (d(mu_h), d(rho_h), d(mub_h), d(rhob_h)) + tuple(mh)
        hs, cs, kl, saved = BF.lstm_train_fwd_hip(kind, x.detach(), ih, hh, seed, prec=prec, h0=d(h0), c0=d(c0),
                                                  kl_terms=(kl_i, kl_h))
        ctx.meta, ctx.saved_buf, ctx.steps = meta, saved, x.shape[1]
        ctx.set_materialize_grads(False)
        # save_for_backward: an in-place optimizer update of a parameter between forward and backward is caught by autograd
        ctx.save_for_backward(x, h0, c0, mu_i, rho_i, mub_i, rhob_i, mu_h, rho_h, mub_h, rhob_h, hs)
        return hs, cs, kl

    @staticmethod
    @_first_order
    def backward(ctx, d_hs, d_cs, d_kl):
        kind, seed, prec, mi, mh = ctx.meta
        x, h0, c0, mu_i, rho_i, mub_i, rhob_i, mu_h, rho_h, mub_h, rhob_h, hs = ctx.saved_tensors
        need = ctx.needs_input_grad
        d = lambda t: t.detach() if t is not None else None  # noqa: E731
        with torch.no_grad():
            ih = (d(mu_i), d(rho_i), d(mub_i), d(rhob_i)) + tuple(mi)
            hh = (d(mu_h), d(rho_h), d(mub_h), d(rhob_h)) + tuple(mh)
            want_ih, want_hh = any(need[4:8]), any(need[8:12])
            dx, dh0, dc0, gi, gh = BF.lstm_bwd_hip(kind, x.detach(), ih, hh, seed, hs.detach(), ctx.saved_buf, d_hs, d_cs,
                                                   prec=prec, h0=d(h0), c0=d(c0), want_dx=need[1],
                                                   want_dh0=need[2] and h0 is not None, want_dc0=need[3] and c0 is not None,
                                                   want_ih=want_ih, want_hh=want_hh)
            gi = gi if gi is not None else (None,) * 4
            gh = gh if gh is not None else (None,) * 4
            gk = d_kl * ctx.steps if d_kl is not None else None
        mask = lambda i, g: g if need[i] else None  # noqa: E731
        return ((None, dx, dh0, dc0) + tuple(mask(4 + i, g) for i, g in enumerate(gi)) +
                tuple(mask(8 + i, g) for i, g in enumerate(gh)) + (mask(12, gk), mask(13, gk)))


def _entries(meta, params):
    out = []
    for i, (pm, ps, pmt, pst, op) in enumerate(meta):
        mu, rho = params[2 * i].detach(), params[2 * i + 1].detach()
        if pmt is None and op is not None:
            out.append((BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op), pm, ps, None, None))
        else:  # element order must match the logical prior tensors
            out.append((mu.contiguous(), rho.contiguous(), pm, ps,
                        pmt.detach().contiguous() if pmt is not None else None,
                        pst.detach().contiguous() if pst is not None else None))
    return out


def kl_pairs(layer):
    """[(mu, rho, meta)] of one variational layer for KlFn / kl_model_hip"""
    mu, rho = layer._w()
    tens = not layer._priors_are_scalar()
    pairs = [(mu, rho, (layer.prior_mean, layer.prior_variance, layer.prior_weight_mu if tens else None,
                        layer.prior_weight_sigma if tens else None, layer._op))]
    if layer.mu_bias is not None:
        pairs.append((layer.mu_bias, layer.rho_bias, (layer.prior_mean, layer.prior_variance,
                                                      layer.prior_bias_mu if tens else None,
                                                      layer.prior_bias_sigma if tens else None, None)))
    return pairs


class KlMcFn(torch.autograd.Function):
    """sum of the per-tensor sampled mean KLs (BTX-KLMC v1) of `n` (mu, rho) pairs against their non-Gaussian priors on
    the HIP backend, with gradients: btx_kl_mc_model forward, btx_kl_mc_model_bwd backward (eps regenerated, nothing saved but the
    parameters).  meta: per pair (prior, loc_t | None, op | None, layer_id, rng_stream, sample_idx, sample_dev | None)."""

    @staticmethod
    def forward(ctx, meta, seed, draws, *params):
        ctx.meta, ctx.seed, ctx.draws = meta, seed, draws
        ctx.save_for_backward(*params)
        return BF.kl_mc_model_hip(_mc_entries(meta, params), seed, draws)

    @staticmethod
    @_first_order
    def backward(ctx, g):
        params, meta = ctx.saved_tensors, ctx.meta
        entries = _mc_entries(meta, params)
        grads = []
        for mu_e, _rho_e, *_ in entries:  # gradients in the element order the kernel reads: GEMM-major buffers for the weights
            grads.append((torch.empty_like(mu_e), torch.empty_like(mu_e)))
        BF.kl_mc_model_bwd_hip(entries, grads, ctx.seed, ctx.draws, g)
        res = []
        for i, (gm, gr) in enumerate(grads):  # handed back as logical-shape views (unpacked copies where the layout has no view)
            op = meta[i][2]
            if op is not None:
                shape = tuple(params[2 * i].shape)
                gm, gr = BF.gemm_major_logical_view(gm, shape, op), BF.gemm_major_logical_view(gr, shape, op)
            res += [gm, gr]
        return (None, None, None) + tuple(res)


def _mc_entries(meta, params):
    """the kernel's items: every tensor in its unpadded GEMM-major element order (the index space of the KL draws), biases as they are"""
    out = []
    for i, (prior, loc_t, op, layer_id, rng_stream, sample_idx, sample_dev) in enumerate(meta):
        mu, rho = params[2 * i].detach(), params[2 * i + 1].detach()
        if op is not None:
            mu, rho = BF.gemm_major_view(mu, op), BF.gemm_major_view(rho, op)
            loc_t = BF.gemm_major_view(loc_t, op) if loc_t is not None else None
        else:
            mu, rho = mu.contiguous(), rho.contiguous()
            loc_t = loc_t.detach().contiguous() if loc_t is not None else None
        out.append((mu, rho, loc_t, prior, layer_id, rng_stream, sample_idx, sample_dev))
    return out


def kl_mc_pairs(layer):
    """[(mu, rho, meta)] of one variational layer with a non-Gaussian prior for KlMcFn / kl_mc_model_hip"""
    mu, rho = layer._w()
    prior = layer._btx_prior
    loc_w, loc_b = layer._kl_locations()
    s_idx, sdev = layer._kl_sample_index(), getattr(layer, "_btx_sample_dev", None)
    if sdev is not None and sdev.numel() != 1:
        raise _lib.BtxError("the sampled KL reads ONE device sample word; MC sample lanes are an inference feature")
    pairs = [(mu, rho, (prior, loc_w, layer._op, layer._btx_layer_id, _lib.STREAM_KL_W, s_idx, sdev))]
    if layer.mu_bias is not None:
        pairs.append((layer.mu_bias, layer.rho_bias, (prior, loc_b, None, layer._btx_layer_id, _lib.STREAM_KL_B, s_idx, sdev)))
    return pairs


def _kl_mc_of_layers(layers):
    """the sampled KL of the layers with a non-Gaussian prior: one launch per distinct kl_samples (one, unless the model mixes them)"""
    total = None
    for draws in sorted({layer._btx_kl_samples for layer in layers}):
        pairs = [pr for layer in layers if layer._btx_kl_samples == draws for pr in kl_mc_pairs(layer)]
        params = [t for mu, rho, _ in pairs for t in (mu, rho)]
        meta = tuple(m for _, _, m in pairs)
        if torch.is_grad_enabled() and any(t.requires_grad for t in params):
            kl = KlMcFn.apply(meta, _rng.seed(), draws, *params)
        else:
            kl = BF.kl_mc_model_hip(_mc_entries(meta, params), _rng.seed(), draws)
        total = kl if total is None else total + kl
    return total


class KlLogUFn(torch.autograd.Function):
    """sum of the per-tensor KLs against the log-uniform prior (BTX-SVD v1) of `n` (mu, rho) pairs on the HIP backend,
    with gradients: btx_kl_logu_model forward, btx_kl_logu_model_bwd backward (nothing saved but the parameters).  The kernels are
    element-wise, so every (mu, rho) pair that shares one dense element order is read through its storage in place, and the gradients
    are written in that order and handed back as logical (strided) views; a pair whose layouts differ (a `.data` replacement, a
    non-dense view) is read through row-major copies and its gradients come back as plain reshapes.  meta: per pair the reduction,
    "mean" | "sum"."""

    @staticmethod
    def forward(ctx, meta, *params):
        ctx.meta = meta
        ctx.save_for_backward(*params)
        return BF.kl_logu_model_hip(_logu_entries(meta, params))

    @staticmethod
    @_first_order
    def backward(ctx, g):
        params, meta = ctx.saved_tensors, ctx.meta
        entries = _logu_entries(meta, params)
        grads = [(torch.empty_like(mu_e), torch.empty_like(mu_e)) for mu_e, _rho_e, _ in entries]
        BF.kl_logu_model_bwd_hip(entries, grads, g)
        res = []
        for i, (gm, gr) in enumerate(grads):
            mu, rho = params[2 * i], params[2 * i + 1]
            in_place = BF.same_dense_order(mu, rho)
            res += [_logical_like(gm, mu, in_place), _logical_like(gr, rho, in_place)]
        return (None,) + tuple(res)


def _logical_like(flat, p, in_place):
    """the logical-shape tensor over a gradient buffer of parameter `p`: a strided view in p's own element order when the entry was
    p's storage in place, a plain reshape when the entry was a contiguous (row-major) copy"""
    if in_place:
        return flat.as_strided(tuple(p.shape), tuple(p.stride()))
    return flat.reshape(p.shape)


def _logu_entries(meta, params):
    """the kernel's items: (mu, rho) through their dense storage in place where the two share ONE dense element order
    (functional.same_dense_order), else row-major copies of both — a `.data` replacement may leave the two in different layouts"""
    out = []
    for i, reduction in enumerate(meta):
        mu, rho = params[2 * i], params[2 * i + 1]
        if not BF.same_dense_order(mu, rho):
            mu, rho = mu.detach().contiguous(), rho.detach().contiguous()
        out.append((BF.flat_f32(mu), BF.flat_f32(rho), reduction))
    return out


def _kl_logu_of_layers(layers):
    """the KL of the layers with a log-uniform prior: ONE launch group for all their tensors"""
    params, meta = [], []
    for layer in layers:
        mu, rho = layer._w()
        params += [mu, rho]
        meta.append(layer._btx_prior.reduction)
        if layer.mu_bias is not None:
            params += [layer.mu_bias, layer.rho_bias]
            meta.append(layer._btx_prior.reduction)
    if torch.is_grad_enabled() and any(t.requires_grad for t in params):
        return KlLogUFn.apply(tuple(meta), *params)
    return BF.kl_logu_model_hip(_logu_entries(meta, params))


def kl_of_layers(layers):
    """get_kl_loss on the HIP backend: one launch for every tensor of every layer; differentiable when needed.  Layers with a
    non-Gaussian prior (layer.set_prior) go through a launch group of their own — the sampled KL (KlMcFn) or the log-uniform prior's
    (KlLogUFn) — and the scalars are added in a fixed order: (Gaussian + sampled) + log-uniform, each group in module order."""
    logu = [layer for layer in layers if getattr(layer.__dict__.get("_btx_prior"), "deterministic", False)]
    if logu:
        kl_logu = _kl_logu_of_layers(logu)
        layers = [layer for layer in layers if not getattr(layer.__dict__.get("_btx_prior"), "deterministic", False)]
        if not layers:
            return kl_logu
        return kl_of_layers(layers) + kl_logu
    mc = [layer for layer in layers if layer.__dict__.get("_btx_prior") is not None]
    if mc:
        kl_mc = _kl_mc_of_layers(mc)
        layers = [layer for layer in layers if layer.__dict__.get("_btx_prior") is None]
        if not layers:
            return kl_mc
    pairs = [pr for layer in layers for pr in kl_pairs(layer)]
    params = [t for mu, rho, _ in pairs for t in (mu, rho)]
    meta = tuple(m for _, _, m in pairs)
    if torch.is_grad_enabled() and any(t.requires_grad for t in params):
        kl = KlFn.apply(meta, *params)
    else:
        kl = BF.kl_model_hip(_entries(meta, params))
    return kl + kl_mc if mc else kl


# --------------------------------------------------------------------------------------------------------------------
# training-mode BatchNorm on channels-last activations (csrc/btx_bn.hip, btx_bn_train_fwd / _bwd): the step either side of
# the variational convolutions in the reference's training loop (README.md:114-125 on models/deterministic/resnet_large.py)
# --------------------------------------------------------------------------------------------------------------------
def _act_code(dt):
    return _lib.ACT_BF16 if dt == torch.bfloat16 else _lib.ACT_F32


def bn_train_usable(bn, x):
    """True when nn.BatchNorm{1,2,3}d `bn` in training mode on `x` can take the HIP kernels: CUDA tensor, f32 / bf16,
    channels-last storage (or 2-D [M, C]), C % 8 == 0, parameters and running estimates of one dtype (f32 or bf16)."""
    if type(bn) not in (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d):
        return False  # nn.SyncBatchNorm reduces its statistics across ranks, Lazy* variants have no parameters yet: torch's own path
    if not (bn.training and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.dim() in (2, 4, 5)):
        return False
    C = x.shape[1]
    if C % 8 != 0 or C > 2048 or x.numel() == 0 or x.numel() // C < 2:
        return False
    if bn.momentum is None and bn.track_running_stats:
        return False  # cumulative moving average: torch's own path
    ts = [t for t in (bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
                      bn.running_var if bn.track_running_stats else None) if t is not None]
    if ts and (any(t.dtype != ts[0].dtype for t in ts) or ts[0].dtype not in (torch.float32, torch.bfloat16)):
        return False
    if x.dim() == 2 and not x.is_contiguous():
        return False
    if x.dim() == 4 and not x.is_contiguous(memory_format=torch.channels_last):
        return False
    if x.dim() == 5 and not x.is_contiguous(memory_format=torch.channels_last_3d):
        return False
    return True


class BatchNormTrainFn(torch.autograd.Function):
    """y = [relu](batch_norm(x) [+ residual]) with batch statistics; running_mean / running_var / num_batches_tracked updated in
    place (as F.batch_norm / nn.BatchNorm do).  The ReLU and the residual add of the reference's blocks
    (models/deterministic/resnet_large.py:46-62) ride in the normalisation's own launches (csrc/btx_bn.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, batches_tracked=None, residual=None, relu=False):
        L = _lib.lib()
        C = x.shape[1]
        M = x.numel() // C
        dev = x.device
        # the kernels move 8 channels per 16-byte access: a tensor off that grid (a dense view into a flat buffer) enters as one
        # aligned copy with the same strides — the same launches, the same bits
        x, residual = BF.on_grid(x), BF.on_grid(residual)
        y = torch.empty_like(x)  # preserves the channels-last strides
        save_mean = torch.empty(C, dtype=torch.float32, device=dev)
        save_invstd = torch.empty(C, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = BF._workspace(dev, L.btx_bn_workspace_bytes(M, C), stream)
        ref = next((t for t in (weight, bias, running_mean, running_var) if t is not None), None)
        pdt = _act_code(ref.dtype) if ref is not None else _lib.ACT_F32
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        w = weight.detach().contiguous() if weight is not None else None
        b = bias.detach().contiguous() if bias is not None else None
        mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=dev) if relu else None  # one bit per element: y > 0
        fuse = None
        if relu or residual is not None:
            fuse = _lib.BnFuse(ptr(residual), 1 if relu else 0, ptr(mask), None)
        _lib.check(L.btx_bn_train_fwd(x.data_ptr(), y.data_ptr(), _act_code(x.dtype), M, C, ptr(w), ptr(b), ptr(running_mean),
                                      ptr(running_var), pdt, float(momentum if momentum is not None else 0.0), float(eps),
                                      save_mean.data_ptr(), save_invstd.data_ptr(), ptr(batches_tracked),
                                      ctypes.byref(fuse) if fuse is not None else None, ws.data_ptr(), ws.numel(), stream))
        ctx.save_for_backward(x, w, save_mean, save_invstd, mask)
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.relu = bool(relu)
        ctx.pdt = pdt
        return y

    @staticmethod
    @_first_order
    def backward(ctx, dy):
        L = _lib.lib()
        x, w, save_mean, save_invstd, mask = ctx.saved_tensors
        C = x.shape[1]
        M = x.numel() // C
        dev = x.device
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        # the gradient in the layout of x (channels-last storage): a no-op when the consumer produced it that way
        if x.dim() == 4:
            dy = dy.contiguous(memory_format=torch.channels_last)
        elif x.dim() == 5:
            dy = dy.contiguous(memory_format=torch.channels_last_3d)
        else:
            dy = dy.contiguous()
        dy = BF.on_grid(dy)
        dx = torch.empty_like(x)
        pd = w.dtype if w is not None else torch.float32  # the kernel writes the two [C] gradients in the parameters' dtype
        dgamma = torch.empty(C, dtype=pd, device=dev)
        dbeta = torch.empty(C, dtype=pd, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = BF._workspace(dev, L.btx_bn_workspace_bytes(M, C), stream)
        want_res = ctx.has_res and ctx.needs_input_grad[8]
        dres = None
        fuse = None
        if ctx.relu:
            dres = torch.empty_like(x) if want_res else None  # g = dy where y > 0: the gradient of the residual branch
            fuse = _lib.BnFuse(None, 1, mask.data_ptr(), dres.data_ptr() if dres is not None else None)
        elif want_res:
            dres = dy  # no ReLU behind the add: the residual branch receives dy itself
        _lib.check(L.btx_bn_train_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), _act_code(x.dtype), M, C,
                                      w.data_ptr() if w is not None else None, ctx.pdt, save_mean.data_ptr(),
                                      save_invstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                      ctypes.byref(fuse) if fuse is not None else None, ws.data_ptr(), ws.numel(), stream))
        gw = dgamma if (w is not None and ctx.needs_input_grad[1]) else None
        gb = dbeta if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return (dx if ctx.needs_input_grad[0] else None), gw, gb, None, None, None, None, None, dres, None


def batch_norm_train(bn, x, residual=None, relu=False):
    """training-mode forward of the nn.BatchNorm module `bn` through libbtx (bn_train_usable(bn, x) must hold), optionally with the
    block's residual add and ReLU inside the same launches: y = [relu](bn(x) [+ residual])"""
    nbt = bn.num_batches_tracked if bn.track_running_stats else None
    if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64 and nbt.numel() == 1):
        nbt.add_(1)   # not a device int64 word: torch's own increment
        nbt = None
    rm = bn.running_mean if bn.track_running_stats else None
    rv = bn.running_var if bn.track_running_stats else None
    # nbt += 1 happens inside the statistics launch
    return BatchNormTrainFn.apply(x, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps, nbt, residual, relu)


def bn_act(bn, x, residual=None, relu=True):
    """[relu](bn(x) [+ residual]) as the reference's blocks spell it (resnet_large.py:46-62) — through the fused launches when the
    call qualifies (bn_train_usable, residual of x's shape / dtype / storage layout), else with torch's own ops"""
    if bn_train_usable(bn, x) and (residual is None or (residual.shape == x.shape and residual.dtype == x.dtype and
                                                        residual.stride() == x.stride() and residual.is_cuda)):
        return batch_norm_train(bn, x, residual=residual, relu=relu)
    y = bn(x)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def max_pool_train_usable(mp, x):
    """nn.MaxPool2d `mp` on `x` can take btx_maxpool2d_cl_train / _bwd: a CUDA f32 / bf16 tensor in channels-last storage with
    C % 8 == 0 that needs a gradient; square integer window <= 15, dilation 1, floor mode, no indices asked for"""
    if not (isinstance(mp, torch.nn.MaxPool2d) and x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    if not (torch.is_grad_enabled() and x.requires_grad):
        return False
    sq = lambda v: v if isinstance(v, int) else (v[0] if (len(v) == 2 and v[0] == v[1]) else None)  # noqa: E731
    k, s_, p_, d_ = sq(mp.kernel_size), sq(mp.stride if mp.stride is not None else mp.kernel_size), sq(mp.padding), sq(mp.dilation)
    if None in (k, s_, p_, d_) or d_ != 1 or mp.ceil_mode or mp.return_indices or k > 15 or 2 * p_ > k:
        return False
    n, c, h, w = x.shape
    if c % 8 != 0 or x.numel() == 0 or (h + 2 * p_ - k) // s_ + 1 <= 0 or (w + 2 * p_ - k) // s_ + 1 <= 0:
        return False
    return x.is_contiguous(memory_format=torch.channels_last)


class MaxPool2dTrainFn(torch.autograd.Function):
    """F.max_pool2d on the HIP backend under autograd: one byte per output element (the window position of its maximum) instead of
    ATen's int64 index; forward and backward equal torch's bit for bit (tests/test_gpu_backward.py)"""

    @staticmethod
    def forward(ctx, x, k, s_, p_):
        y, idx = BF.maxpool2d_train_hip(x, k, s_, p_)
        ctx.save_for_backward(idx)
        ctx.geom = (tuple(x.shape), k, s_, p_)
        return y

    @staticmethod
    @_first_order
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        shape, k, s_, p_ = ctx.geom
        return BF.maxpool2d_bwd_hip(dy.contiguous(memory_format=torch.channels_last), idx, shape, k, s_, p_), None, None, None


def max_pool_train(mp, x):
    sq = lambda v: v if isinstance(v, int) else v[0]  # noqa: E731
    return MaxPool2dTrainFn.apply(x, sq(mp.kernel_size), sq(mp.stride if mp.stride is not None else mp.kernel_size), sq(mp.padding))


def _refuse_lstm(model, what):
    from .layers.base_variational_layer import _VariationalLSTM
    for name, m in model.named_modules():
        if isinstance(m, _VariationalLSTM):
            raise _lib.BtxError("%s: the model holds the Bayesian LSTM %r (%s); its time steps consume the sample indices s + t, "
                                "which collide with the indices of the Monte-Carlo passes: use num_mc=1" % (what, name, type(m).__name__))


def mc_train_forward(model, x, num_mc, step):
    """[num_mc, B, C] logits of `num_mc` Monte-Carlo training forwards of `model` on `x`, carrying gradient: the eager form of the
    reference's loop (examples/main_bayesian_cifar.py:363-372).  Pass k runs set_sample_index(model, (step * num_mc + k) &
    0x7FFFFFFF, presample=x.is_cuda) and model(x); a tuple output contributes its element 0.  CPU tensors take the ATen route
    with torch's CPU generator keyed on the index for the duration of the pass, as mc.mc_forward does.
    Training BatchNorm sees num_mc forwards (running_* and num_batches_tracked advance num_mc times, as in the reference); num_mc
    sets of saved activations live until the backward.  A model that holds a Bayesian LSTM is refused (BtxError), and so is a model
    whose layers still read a device sample word (close() the GraphedTrainStep / GraphedMC first)."""
    num_mc = int(num_mc)
    if num_mc < 1:
        raise ValueError("num_mc must be >= 1")
    _refuse_lstm(model, "mc_train_forward")
    for name, m in model.named_modules():
        if getattr(m, "_btx_sample_dev", None) is not None:
            # a live GraphedTrainStep / mc.GraphedMC keeps the sample index in ONE device word: every pass here would rewrite it and
            # every backward would then regenerate the LAST pass's noise
            raise _lib.BtxError("mc_train_forward: layer %r reads its sample index from a device word (a live GraphedTrainStep or "
                                "GraphedMC on this model); close() it first" % name)
    outs = []
    for k in range(num_mc):
        idx = (int(step) * num_mc + k) & 0x7FFFFFFF
        _rng.set_sample_index(model, idx, presample=x.is_cuda)
        if x.is_cuda:
            out = model(x)
        else:
            with torch.random.fork_rng(devices=[]):
                torch.default_generator.manual_seed(_rng.cpu_sample_seed(idx))  # the CPU generator ONLY
                out = model(x)
        outs.append(out[0] if isinstance(out, tuple) else out)
    return torch.stack(outs)


class GraphedTrainStep:
    """forward + loss + backward of `model` on a fixed batch, captured ONCE into a hipGraph and replayed per training step
    (reference README.md:114-125: `output = model(x); kl = get_kl_loss(model); loss = ce(output, y) + kl / batch_size;
    loss.backward()`).  An eager step of a converted ResNet18 dispatches ~590 kernel launches through Python / ATen at ~16 us
    each and is bound by the HOST (profiles/r05_experiments.txt E9); a replay has no host work.  What changes between steps — the MC
    sample index that keys BTX-RNG v1 — lives in one device word that run() rewrites, so every replay draws fresh noise exactly as
    an eager step with set_sample_index(model, s) would (forward, data / weight / rho gradients all read the word).

        step = GraphedTrainStep(model, x, target)            # grads live in p.grad (static tensors, rewritten by every replay)
        for it in range(n): loss = step.run(it); optimizer.step()

    With `optimizer=` one of bayesian_torch_amd.optim.{SGD, Adam, AdamW}, the update is INSIDE the graph as well: the gradient norm
    (max_grad_norm) and the update launches are captured after loss.backward(); run() advances the optimizer's step counts on the
    host, rewrites its device blocks from the groups' current lr, replays, and bumps the parameters' versions:

        step = GraphedTrainStep(model, x, target, optimizer=opt)
        for it in range(n): loss = step.run(it); scheduler.step()

    Constructing the step changes no parameter and no optimizer state (the warm-up runs forward + backward only; the update kernels
    are warmed on scratch tensors).  Load an optimizer state_dict BEFORE constructing the step: the graph holds the state's pointers.

    In-place parameter updates between replays are seen (the kernels read mu / rho where they live); x / target are read from the
    tensors given here (copy new batches INTO them).  Layers on padded layouts that need their input gradient (sign tensors keyed
    on the host) cannot be captured and raise.  Drop every reference to the loss / outputs of earlier EAGER steps of this model
    before constructing one (torch: a live autograd graph pins its AccumulateGrad nodes to the stream it ran on).

    num_mc = n > 1: the reference's Monte-Carlo training loop (examples/main_bayesian_cifar.py:363-372) inside ONE graph.  The step
    holds n device sample words; pass k points every layer at word k, pre-samples and runs model(x); the n outputs are stacked to
    [n, B, C] and `loss_fn(stack, target)` is called ONCE, then loss.backward() and the captured optimizer.  run(step) writes the
    words step * n + k with one copy.  The default loss is utils.mc_loss.mc_elbo_loss(stack, target, kl=get_kl_loss(model)):
    CE(mean_k logits_k, y) + kl / B, the KL (RNG-free) evaluated once.  `out` of loss_fn is 3-D then; num_mc = 1 keeps the 2-D
    `out`, the single word and the default loss above.  Consequences: training BatchNorm sees n forwards per step (running_* and
    num_batches_tracked advance n times, as in the reference's loop); n sets of saved activations live until the backward (no
    recomputation).  Models that hold a Bayesian LSTM are refused for n > 1 (its time steps consume the indices s + t, which would
    collide with the passes').

    group = a process group (torch.distributed.group.WORLD for the default one; None, the default, changes nothing even when
    torch.distributed is initialised): data-parallel training, one process per GPU, parallel.GradReducer as `step.reducer`
    (DESIGN.md §17).  Construction broadcasts rank 0's parameters and buffers (broadcast=False: skip it).  The default losses divide
    the KL by `step.global_batch` = batch * world, so each rank's loss is CE(local shard) + KL / B_global; a custom loss_fn does that
    scaling itself.  The step is TWO graphs with the eager collective between them:

        graph A   forward, loss, backward, staging copies, btx_bucket_pack of every gradient and the loss (x f32(1 / world))
        eager     ONE all_reduce(SUM) of the bucket on the replay stream
        graph B   the captured optimizer, every item's gradient pointing at its slice of the bucket (the norm of max_grad_norm too:
                  the REDUCED gradient is clipped)

    run(step) writes the sample words (step * world + rank) * num_mc + k and returns the mean loss over the ranks (a view of the
    bucket's last word).  With an optimizer, p.grad keeps this rank's LOCAL gradient and step.reducer.grad_view(p) is the reduced
    one; with optimizer=None run() unpacks the bucket into p.grad (btx_bucket_unpack) so that a torch.optim step can follow.
    forward_backward(step) and apply() are the two halves of run() on either side of the collective.  `group` may also be a
    ready GradReducer (one built with rank= / world=: several ranks played in one process)."""

    def __init__(self, model, x, target, loss_fn=None, warmup=2, optimizer=None, num_mc=1, group=None, broadcast=True):
        from .models.dnn_to_bnn import get_kl_loss
        from . import optim as _optim
        if not x.is_cuda:
            raise ValueError("GraphedTrainStep needs CUDA (ROCm) tensors")
        self.num_mc = int(num_mc)
        if self.num_mc < 1:
            raise ValueError("num_mc must be >= 1")
        if self.num_mc > 1:
            _refuse_lstm(model, "GraphedTrainStep(num_mc=%d)" % self.num_mc)
        if optimizer is not None and not isinstance(optimizer, _optim._BtxOptimizer):
            raise TypeError("GraphedTrainStep(optimizer=) takes bayesian_torch_amd.optim.SGD / Adam / AdamW (got %s): a torch.optim "
                            "step cannot be captured here; call it after run() instead" % type(optimizer).__name__)
        self.optimizer, self._plan = optimizer, None
        self.model, self.x, self.target = model, x, target
        bs = x.shape[0]
        self.reducer, self.graph_b = None, None
        if group is not None:
            from .parallel import GradReducer
            self.reducer = group if isinstance(group, GradReducer) else GradReducer(model, group=group, broadcast=broadcast)
        world = 1 if self.reducer is None else self.reducer.world
        self.global_batch = bs * world
        if loss_fn is None and world > 1:  # (world == 1 keeps the expressions below: the same graph, bit for bit)
            if self.num_mc > 1:
                from .utils.mc_loss import mc_elbo_loss
                loss_fn = lambda out, tgt: mc_elbo_loss(out, tgt, kl=get_kl_loss(model) / world, reduce="logits")  # noqa: E731
            else:
                B = self.global_batch
                loss_fn = lambda out, tgt: torch.nn.functional.cross_entropy(out.float(), tgt) + get_kl_loss(model) / B  # noqa: E731
        if loss_fn is None and self.num_mc > 1:
            from .utils.mc_loss import mc_elbo_loss
            loss_fn = lambda out, tgt: mc_elbo_loss(out, tgt, kl=get_kl_loss(model), reduce="logits")  # noqa: E731
        self.loss_fn = loss_fn or (lambda out, tgt: torch.nn.functional.cross_entropy(out.float(), tgt) + get_kl_loss(model) / bs)
        dev = x.device
        import gc
        gc.collect()  # autograd graphs of earlier eager steps still referenced from garbage would pin AccumulateGrad nodes to the
        torch.cuda.synchronize(dev)  # caller's stream (torch warns that this "may break CUDA graph capture": it does)
        self._layers = [m for m in model.modules() if hasattr(m, "_btx_layer_id")]
        self.sample_dev = torch.zeros(self.num_mc, dtype=torch.int32, device=dev)  # one word per MC pass
        self._words = [self.sample_dev[k:k + 1] for k in range(self.num_mc)]
        for m in self._layers:
            m.__dict__["_btx_sample_dev"] = self._words[0]
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup) + 1):
                warm_loss = self._step()
            if self.reducer is not None:   # both bucket kernels once, and the reducer's staging tensors allocated
                self.reducer.pack(warm_loss)
                self.reducer.unpack()
            if optimizer is not None:
                optimizer._warm(dev)   # every update kernel once, on scratch tensors: the model is not touched
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        if optimizer is not None:
            with torch.no_grad():
                # state, staging buffers, device blocks and the norm workspace exist before the capture
                optimizer._plan(self._bucket_grads())
        for p_ in model.parameters():
            p_.grad = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.loss = self._step()
            if self.reducer is not None:
                self.reducer.pack(self.loss)
            elif optimizer is not None:
                with torch.no_grad():
                    self._plan = optimizer._plan()   # the item tables of THIS capture's gradient tensors
                    optimizer._launch(self._plan)
        if self.reducer is not None and optimizer is not None:
            self.graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_b, capture_error_mode="thread_local"), torch.no_grad():
                self._plan = optimizer._plan(self._bucket_grads())   # every gradient read from its slice of the reduced bucket
                optimizer._launch(self._plan)
        # the graph writes its gradients into these pool tensors on every replay; `optimizer.zero_grad()` (set_to_none=True by
        # default) between replays detaches them from the parameters, so run() attaches them again
        self._grads = [(p_, p_.grad) for p_ in model.parameters() if p_.grad is not None]

    def _bucket_grads(self):
        """{parameter: its slice of the bucket} for the parameters that have a gradient; None without a group (p.grad is read)"""
        if self.reducer is None:
            return None
        return {p_: self.reducer.grad_view(p_) for p_ in self.reducer.params if p_.grad is not None}

    def _step(self):
        for p_ in self.model.parameters():
            p_.grad = None
        if self.num_mc == 1:
            out = self._pass()
        else:
            outs = []
            for w in self._words:  # pass k reads word k; each ContractFn keeps the word its forward read for its backward
                for m in self._layers:
                    m.__dict__["_btx_sample_dev"] = w
                outs.append(self._pass())
            out = torch.stack(outs)
        loss = self.loss_fn(out, self.target)
        loss.backward()
        return loss.detach()

    def _pass(self):
        _rng.presample(self.model, 0)  # one sampling launch for the forward of every layer (reads the device word)
        out = self.model(self.x)
        return out[0] if isinstance(out, tuple) else out

    def run(self, sample_idx):
        """replay with MC sample index `sample_idx` (num_mc = n > 1: the step number; pass k draws sample step * n + k).  With a group:
        `sample_idx` is the step number, the same on every rank; returns the mean loss over the ranks."""
        if self.reducer is not None:
            self.forward_backward(sample_idx)
            self.reducer.all_reduce()
            return self.apply()
        if self.num_mc == 1:
            self.sample_dev.fill_(int(sample_idx) & 0x7FFFFFFF)
        else:
            n = self.num_mc
            self.sample_dev.copy_(torch.tensor([(int(sample_idx) * n + k) & 0x7FFFFFFF for k in range(n)], dtype=torch.int32))
        if self._plan is not None:
            with torch.no_grad():
                self.optimizer._advance(self._plan)  # step counts, and lr & co. as the groups hold them NOW, into the device blocks
        self.graph.replay()
        for p_, g_ in self._grads:
            if p_.grad is not g_:
                p_.grad = g_
        if self._plan is not None:
            self.optimizer._finish(self._plan)       # the replay wrote the parameters through raw pointers: bump their versions
        return self.loss

    def forward_backward(self, step):
        """group= only, the first half of run(): sample words, the optimizer's host side, graph A (the bucket then holds this rank's
        gradients and loss times f32(1 / world))"""
        r, n = self.reducer, self.num_mc
        if n == 1:
            self.sample_dev.fill_(r.sample_index(step))
        else:
            self.sample_dev.copy_(torch.tensor([r.sample_index(step, k, n) for k in range(n)], dtype=torch.int32))
        if self._plan is not None:
            with torch.no_grad():
                self.optimizer._advance(self._plan)
        self.graph.replay()
        for p_, g_ in self._grads:
            if p_.grad is not g_:
                p_.grad = g_

    def apply(self):
        """group= only, the second half of run(), after the bucket has been summed over the ranks: graph B (the update from the
        bucket), or without an optimizer the bucket unpacked into p.grad; returns the mean loss"""
        if self._plan is not None:
            self.graph_b.replay()
            self.optimizer._finish(self._plan)
        else:
            self.reducer.unpack()
        return self.reducer.loss

    def close(self):
        for m in self._layers:
            m.__dict__["_btx_sample_dev"] = None
            m.__dict__["_btx_pre"] = None
