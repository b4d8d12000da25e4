"""Poisoned memory: every buffer a wrapper takes from `torch.empty` and every workspace handed out by
`functional._workspace` is filled with one byte pattern before the kernels see it, so a result that depends on what a buffer
held BEFORE the call (an output element nobody wrote, a workspace word read before it was written, a reduce pass that reads one slab
too many) no longer reads back the right value the previous run left there.

    with poisoned(0xFF) as p:        # NaN in f32 / bf16 / f64, -1 or 255 in the integer types
        got = call()
    with poisoned(0x7F) as q:        # ~3.4e38 in f32 / bf16, huge and finite in f64, 127 in int8
        got2 = call()
    assert bits_equal(got, clean) and bits_equal(got2, clean)
    assert p.bytes > 0 and "btx_contract_fwd_ex" in p.calls

Poison is data only: a buffer a later kernel addresses memory through (pool indices) is compared on the host with the
unpoisoned run before it is passed on (tests/test_gpu_poison.py).  Nothing is filled while the current stream is capturing:
the fill would become a node of the graph.
"""
import contextlib

import torch

PATTERNS = (0xFF, 0x7F)


class Record:
    """what one `poisoned` block did: `tensors` buffers and `bytes` bytes filled, `calls` = the btx_* entry points entered"""

    def __init__(self, byte):
        self.byte, self.tensors, self.bytes, self.calls = int(byte), 0, 0, []

    def called(self, name):
        return name in self.calls


def _fill(t, rec, devices):
    """fill the WHOLE storage of a fresh tensor through a uint8 alias (so dense non-contiguous layouts are covered too)"""
    if not isinstance(t, torch.Tensor) or t.device.type not in devices or t.device.type == "meta":
        return t
    if t.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return t
    st = t.untyped_storage()
    n = st.nbytes()
    if n == 0:
        return t
    with torch.no_grad():
        torch.tensor([], dtype=torch.uint8, device=t.device).set_(st, 0, (n,), (1,)).fill_(rec.byte)
    rec.tensors += 1
    rec.bytes += n
    return t


def fill_bytes(t, byte):
    """overwrite the whole storage of `t` with `byte` (the captured-graph tests fill cached buffers between replays)"""
    rec = Record(byte)
    _fill(t, rec, (t.device.type,))
    return rec.bytes


@contextlib.contextmanager
def poisoned(byte, devices=("cuda",)):
    """while active: torch.empty / empty_like / empty_strided, Tensor.new_empty and functional._workspace return memory filled with
    `byte` (tensors on `devices` only; a workspace is refilled on EVERY call), and every btx_* attribute of the loaded library
    records its name when called.  Everything is restored on exit, on an exception too."""
    from bayesian_torch_amd import _lib, functional as BF
    byte = int(byte)
    if not 0 <= byte <= 255:
        raise ValueError("byte must be in 0..255")
    devices = tuple(devices)
    rec = Record(byte)
    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    def wrap_factory(orig):
        def factory(*a, **kw):
            return _fill(orig(*a, **kw), rec, devices)
        factory.__wrapped__ = orig
        return factory

    orig_ws = BF._workspace

    def workspace(device, nbytes, stream):
        return _fill(orig_ws(device, nbytes, stream), rec, devices)

    def wrap_entry(name, orig):
        def entry(*a):
            rec.calls.append(name)
            return orig(*a)
        entry.__wrapped__ = orig
        return entry

    try:
        for name in ("empty", "empty_like", "empty_strided"):
            patch(torch, name, wrap_factory(getattr(torch, name)))
        patch(torch.Tensor, "new_empty", wrap_factory(torch.Tensor.new_empty))
        patch(BF, "_workspace", workspace)
        L = _lib._LIB
        if L is None:
            try:
                L = _lib.lib()
            except _lib.BtxError:
                L = None  # no library built: nothing to record (the CPU self-test of the helper needs none)
        if L is not None:
            for name in _lib.EXPORTS:
                patch(L, name, wrap_entry(name, getattr(L, name)))
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


def _leaves(v):
    if v is None or isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, dict):
        return [t for k in sorted(v) for t in _leaves(v[k])]
    if isinstance(v, (tuple, list)):
        return [t for e in v for t in _leaves(e)]
    raise TypeError("bits_equal compares tensors and nested tuples / lists / dicts of tensors, got %r" % type(v))


def _raw(t):
    t = t.detach()
    if t.layout != torch.strided:
        raise TypeError("bits_equal wants strided tensors")
    return t.contiguous().cpu().reshape(-1).view(torch.uint8)


def bits_equal(a, b):
    """True when a and b (tensors, or nested tuples / lists / dicts of tensors and None) hold the same bytes in every logical
    element, with equal shapes and dtypes: NaN == NaN of the same payload, -0.0 != 0.0"""
    la, lb = _leaves(a), _leaves(b)
    if len(la) != len(lb):
        return False
    for x, y in zip(la, lb):
        if x is None or y is None:
            if x is not y:
                return False
            continue
        if x.dtype != y.dtype or tuple(x.shape) != tuple(y.shape):
            return False
        if not torch.equal(_raw(x), _raw(y)):
            return False
    return True


def any_nan(v):
    """True when a floating tensor among the leaves of v holds a NaN"""
    return any(bool(torch.isnan(t).any()) for t in _leaves(v) if t is not None and t.is_floating_point())
