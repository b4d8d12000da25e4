"""Log-alpha statistics and pruning of variational layers (BTX-SVD v1).

    log alpha = log(sigma^2 / mu^2) = -2 log(|mu| / sigma)

is the quantity sparse variational dropout thresholds (Molchanov, Ashukha & Vetrov 2017: weights with log alpha > 3 are noise) and,
read as a signal-to-noise ratio, the pruning criterion of Blundell et al. (2015) — so everything here works for ANY prior, the
Gaussian one included, not only for priors.LogUniformPrior.

    log_alpha(layer)                                   -> (la_weight, la_bias | None), logical shapes, clamped to [-20, 20]
    stats(model, thresholds=(3.,), bins=0)             -> report: numel, counts above each threshold, zero_mu, histograms
    prune_(model, threshold=3., fraction=None)         -> report of what was pruned; in place, under no_grad

On the GPU (HIP backend) stats is one launch per 48 tensors and ONE host read (btx_logalpha_stats), prune_ one launch per 48 tensors
(btx_logalpha_prune); on the CPU, on backend "torch" and for prune_(fraction=) the same f32 arithmetic runs in torch.  A pruned
weight has mu = 0 and rho = RHO_PRUNED = -40 (sigma = 4.2e-18): its noise is below any rounding of the contraction, and no KL or
gradient of the pruned model is inf or NaN.  NOT done: a pruned model is not faster (zeros go through the dense MFMA kernels), and masks are not
persistent — further training moves pruned weights again.  A live mc.GraphedMC with lanes > 1 in lane_mode "launch" keeps cached
mean tiles and sigma that follow no version counter: call its refresh_weights() after prune_, or its replays evaluate the UNPRUNED
weights (mc.evaluate / mc.mc_forward build their state per call and need nothing).  Bayesian LSTM and quantized layers are skipped.
"""
import torch

from . import _lib, functional as BF
from .layers import base_variational_layer as _base

LA_MAX, RHO_PRUNED = _lib.LOGALPHA_MAX, _lib.RHO_PRUNED


def _layers(model):
    """[(name, layer)]: the variational layers with their own parameters, in module order (the inner layers of a Bayesian LSTM, which
    refuse non-Gaussian priors, are left alone)"""
    return [(name, m) for name, m in model.named_modules()
            if isinstance(m, _base._VariationalNd) and not m.__dict__.get("_btx_no_prior")]


def _tensors(model, include_bias):
    """[(name, mu, rho)] of the selected parameter tensors"""
    out = []
    for name, layer in _layers(model):
        mu, rho = layer._w()
        prefix = name + "." if name else ""
        out.append((prefix + layer._wn, mu, rho))
        if include_bias and layer.mu_bias is not None:
            out.append((prefix + "bias", layer.mu_bias, layer.rho_bias))
    if not out:
        raise ValueError("the model has no variational layers")
    return out


def _la(mu, rho):
    """clamped log alpha in the tensor's own dtype (f32 for parameters), no gradient"""
    with torch.no_grad():
        return BF.log_alpha_aten(mu.detach(), BF.softplus_naive(rho.detach()))[0]


def log_alpha(layer):
    """(log alpha of the weight, of the bias or None) in the parameters' logical shapes, clamped to [-LA_MAX, LA_MAX]; no gradient"""
    mu, rho = layer._w()
    return _la(mu, rho), (None if layer.mu_bias is None else _la(layer.mu_bias, layer.rho_bias))


def _in_place_pair(mu, rho):
    """the storage-order views of (mu, rho) for the kernels, or None when the two are not dense in one common element order"""
    if mu.dtype != torch.float32 or rho.dtype != torch.float32 or not BF.same_dense_order(mu, rho):
        return None
    return BF.dense_flat(mu), BF.dense_flat(rho)


def _on_hip(tensors):
    return _base._BACKEND != "torch" and all(mu.is_cuda and rho.is_cuda for _, mu, rho in tensors)


def _bin_index(la, bins):
    return torch.floor((la + LA_MAX) * float(bins) / (2.0 * LA_MAX)).clamp_(0, bins - 1).to(torch.int64)


def stats(model, thresholds=(3.0,), bins=0, include_bias=False):
    """Per-tensor and total log-alpha statistics -> dict(thresholds, bins, tensors=[dict(name, numel, above=[count(la > t) per
    threshold], zero_mu, hist=[bins counts] | None)], total=dict(numel, above, zero_mu, hist)).  Strict `>`; histogram bin b =
    min(bins - 1, floor((la + 20) * bins / 40)) over [-20, 20]; all counts are exact integers."""
    thresholds = tuple(float(t) for t in thresholds)
    bins = int(bins)
    if len(thresholds) > _lib.LOGALPHA_MAX_THRESHOLDS:
        raise ValueError("at most %d thresholds (got %d)" % (_lib.LOGALPHA_MAX_THRESHOLDS, len(thresholds)))
    if not 0 <= bins <= _lib.LOGALPHA_MAX_BINS:
        raise ValueError("bins must lie in [0, %d] (got %d)" % (_lib.LOGALPHA_MAX_BINS, bins))
    tens = _tensors(model, include_bias)
    T, W = len(thresholds), _lib.LOGALPHA_STATS_WORDS
    rows = None
    if _on_hip(tens):
        pairs = [_in_place_pair(mu, rho) or (mu.detach().contiguous().reshape(-1), rho.detach().contiguous().reshape(-1))
                 for _, mu, rho in tens]
        rows = BF.logalpha_stats_hip(pairs, thresholds, bins).cpu().tolist()  # the one host read
    per = []
    for i, (name, mu, rho) in enumerate(tens):
        if rows is not None:
            above, zero_mu, hist = rows[i][:T], rows[i][_lib.LOGALPHA_ZERO_MU], (rows[i][W:] if bins else None)
        else:
            la = _la(mu, rho).reshape(-1)
            above = [int((la > t).sum()) for t in thresholds]
            zero_mu = int((mu.detach() == 0).sum())
            hist = torch.bincount(_bin_index(la, bins), minlength=bins).tolist() if bins else None
        per.append(dict(name=name, numel=mu.numel(), above=list(above), zero_mu=int(zero_mu), hist=hist))
    total = dict(numel=sum(p["numel"] for p in per), above=[sum(p["above"][k] for p in per) for k in range(T)],
                 zero_mu=sum(p["zero_mu"] for p in per),
                 hist=[sum(p["hist"][b] for p in per) for b in range(bins)] if bins else None)
    return dict(thresholds=thresholds, bins=bins, tensors=per, total=total)


@torch.no_grad()
def prune_(model, threshold=3.0, fraction=None, include_bias=False):
    """Set mu = 0 and rho = RHO_PRUNED wherever log alpha > threshold, in place -> dict(threshold, inclusive, fraction, requested,
    tensors=[dict(name, numel, pruned)], total=dict(numel, pruned)).  Any prior: for Gaussian-prior models this is the signal-to-noise
    criterion.  fraction= (in [0, 1]) prunes the round(fraction * numel) selected weights of largest log alpha instead: the global
    threshold is their smallest log alpha (torch.kthvalue; one-off, so this mode runs in torch on any device), and ties AT it are
    pruned as well (la >= threshold: `inclusive`), so slightly more than `requested` may go — total["pruned"] says how many.  The
    version counter of every tensor written is bumped, so whatever is keyed on (data_ptr, _version) sees the zeros."""
    tens = _tensors(model, include_bias)
    requested, inclusive = None, False
    if fraction is not None:
        fraction = float(fraction)
        if not 0.0 <= fraction <= 1.0:
            raise ValueError("fraction must lie in [0, 1] (got %r)" % (fraction,))
        numel = sum(mu.numel() for _, mu, _ in tens)
        requested, inclusive = int(round(fraction * numel)), True
        if requested == 0:
            threshold = float("inf")
        else:
            la_all = torch.cat([_la(mu, rho).reshape(-1) for _, mu, rho in tens])
            threshold = float(torch.kthvalue(la_all, numel - requested + 1).values)  # the requested-th largest
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold must not be NaN")
    pruned = [None] * len(tens)
    pairs = {}
    if not inclusive and _on_hip(tens):
        pairs = {i: pair for i, (_, mu, rho) in enumerate(tens) for pair in [_in_place_pair(mu, rho)] if pair is not None}
    if pairs:
        counts = BF.logalpha_prune_hip(list(pairs.values()), threshold)
        # the kernel wrote through raw pointers: bump the versions as an in-place torch op would have
        torch.autograd.graph.increment_version([t for i in pairs for t in tens[i][1:]])
        for i, c in zip(pairs, counts.cpu().tolist()):
            pruned[i] = int(c)
    for i, (_, mu, rho) in enumerate(tens):
        if i in pairs:
            continue
        la = _la(mu, rho)
        mask = (la >= threshold) if inclusive else (la > threshold)
        mu.masked_fill_(mask, 0.0)
        rho.masked_fill_(mask, RHO_PRUNED)
        pruned[i] = int(mask.sum())
    per = [dict(name=name, numel=mu.numel(), pruned=pruned[i]) for i, (name, mu, _) in enumerate(tens)]
    return dict(threshold=threshold, inclusive=inclusive, fraction=fraction, requested=requested, tensors=per,
                total=dict(numel=sum(p["numel"] for p in per), pruned=sum(p["pruned"] for p in per)))
