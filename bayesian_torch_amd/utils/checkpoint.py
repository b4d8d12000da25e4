"""Activation checkpointing that keeps the BTX-RNG identity of every layer inside the checkpointed block (DESIGN.md "Autograd contract").

torch.utils.checkpoint runs `fn` a second time inside the backward.  It preserves torch's generator state around that second run, which
is all the reference needs; here the noise of a layer is keyed on (seed, MC sample index, layer id), and every training forward
advances the layer's host counter — so under plain torch.utils.checkpoint the recomputation draws sample s + 1 (or whatever the
counter has reached), and everything rebuilt inside the block belongs to another draw than the loss saw.  `checkpoint` below records
the counters on the first run and puts them back for the duration of the recomputation.
"""
import torch
import torch.utils.checkpoint as _tcp


_KEYS = ("_btx_sample", "_btx_kl_sample", "_btx_sample_dev")
_MISSING = object()


def _layers_of(fn, modules):
    if modules is None:
        if not isinstance(fn, torch.nn.Module):
            raise ValueError("checkpoint: `fn` is not an nn.Module; name the modules it runs with modules=")
        modules = [fn]
    elif isinstance(modules, torch.nn.Module):
        modules = [modules]
    seen, out = set(), []
    for root in modules:
        for m in root.modules():
            if hasattr(m, "_btx_layer_id") and id(m) not in seen:
                seen.add(id(m))
                out.append(m)
    return out


def _snapshot(layers):
    return [tuple(m.__dict__.get(k, _MISSING) for k in _KEYS) for m in layers]


def _restore(layers, snap):
    for m, vals in zip(layers, snap):
        for k, v in zip(_KEYS, vals):
            if v is _MISSING:
                m.__dict__.pop(k, None)
            else:
                m.__dict__[k] = v


def checkpoint(fn, *args, modules=None, **kw):
    """torch.utils.checkpoint.checkpoint(fn, *args, use_reentrant=False, **kw) whose recomputation draws the noise of the FIRST run.

    On the first run the MC sample counter (`_btx_sample`), the index of the sampled KL (`_btx_kl_sample`) and the device sample word
    (`_btx_sample_dev`) of every layer with a BTX-RNG layer id in `fn.modules()` — or in `modules=` (a module or a list of them) when
    `fn` is not an nn.Module — are recorded.  The recomputation inside the backward runs with the recorded values; afterwards the
    layers hold again what they held when it began, so the counters after a checkpointed step equal those after a plain one.  The
    process-wide seed is NOT touched (changing it here would redirect a forward running on another thread): do not call
    manual_seed between the forward and the backward of a checkpointed block.  CPU tensors: torch's preserve_rng_state (on by
    default) covers the CPU generator the ATen route draws from; the counters are handled here all the same."""
    if kw.pop("use_reentrant", False):
        raise ValueError("checkpoint: use_reentrant=True is not supported (the wrapper is built on the non-reentrant form)")
    layers = _layers_of(fn, modules)
    first = []

    def run(*a, **k):
        if not first:
            first.append(_snapshot(layers))
            return fn(*a, **k)
        now = _snapshot(layers)
        _restore(layers, first[0])
        try:
            return fn(*a, **k)
        finally:
            _restore(layers, now)

    return _tcp.checkpoint(run, *args, use_reentrant=False, **kw)
