"""Strided, non-dense views of a tensor (DESIGN.md "Stride contract"): what `torch.chunk` of a channels-last tensor, `x[::2]`,
`x.transpose(0, 1)` of a [T, B, I] sequence, `h0.expand(B, H)`, `logits[:, :k]` and parameters carved from a flat buffer with gaps
hand to the wrappers.  A plain helper module (no fixtures): tests/test_strided_cpu.py checks it, tests/test_gpu_strided.py uses it.

    for name, view, buf in views_of(t):       # view has t's values, shape and dtype; buf is the 1-D buffer it lives in
        got = call(view)
        assert gaps_intact(buf, view)         # nothing was stored between (or around) the elements of the view

Every view's first element lies on the 16-byte grid (so only the strides differ from a tensor of the allocator), and every buffer
holds 64 bytes of slack on either side of a block that is large enough for a DENSE tensor of t's size starting at the view's first
element: a wrapper that forgets the strides and hands the kernel the bare pointer reads (or writes) the fill pattern — NaN, or
0xAB bytes for integer types — inside a live allocation, never unmapped memory.

The forms, where the rank allows them:
  batch_step2    rows [::2] of a buffer with 2 N rows (rank >= 2)
  chan_narrow    channels [8 : 8 + C] of a channels-last buffer with C + 16 channels (rank >= 4); for rank 3 the LAST axis
                 [8 : 8 + I] of a row-major [B, T, I + 16] buffer (a sequence's feature axis is its channel axis)
  other_format   NCHW-dense where t is stored channels-last, channels-last where t is NCHW (rank 4 / 5; dense, no gaps)
  permuted       [T, B, I] storage viewed as [B, T, I] (rank 3; dense, no gaps)
  last_step2     every other element of the last axis of a row-major buffer twice as wide (rank 1 to 3: vectors, [B, C]
                 logits, [S, B, C] stacks)
  expanded       stride 0 over axis 0 — offered only when t's rows are all equal (rank 1: when all elements are equal)
"""
import torch

FORMS = ("batch_step2", "chan_narrow", "other_format", "permuted", "last_step2", "expanded")
FILL_BYTE = 0xAB
SLACK_BYTES = 64


def _dense_strides(t):
    """t's strides when t is non-overlapping and dense (contiguous or channels-last / permuted storage), else ValueError"""
    dims = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1)
    run = 1
    for st, sz in dims:
        if st != run:
            raise ValueError("views_of wants a dense tensor (got shape %s strides %s)" % (tuple(t.shape), tuple(t.stride())))
        run *= sz
    return tuple(t.stride())


def _row_major(shape):
    st, run = [], 1
    for n in reversed(shape):
        st.append(run)
        run *= max(int(n), 1)
    return tuple(reversed(st))


def _channels_last(shape):
    """strides of a logical [N, C, *sp] tensor stored [N, *sp, C]"""
    n, c, sp = shape[0], shape[1], tuple(shape[2:])
    phys = _row_major((n,) + sp + (c,))
    return (phys[0], phys[-1]) + tuple(phys[1:-1])


def _is_channels_last(t):
    return t.dim() >= 4 and t.shape[1] > 1 and tuple(t.stride()) == _channels_last(tuple(t.shape)) and not t.is_contiguous()


def _rows_equal(t):
    if t.numel() == 0 or t.shape[0] < 2:
        return False
    return bool(torch.equal(t[0:1].expand_as(t), t))


def applicable(t):
    """the forms views_of(t) yields"""
    d = t.dim()
    out = []
    if d >= 2 and t.shape[0] >= 1:
        out.append("batch_step2")
    if d >= 3:
        out.append("chan_narrow")
    if d in (4, 5) and t.shape[1] > 1 and max(t.shape[2:]) > 1:
        out.append("other_format")
    if d == 3 and t.shape[0] > 1 and t.shape[1] > 1:
        out.append("permuted")
    if d in (1, 2, 3) and t.shape[-1] > 1:
        out.append("last_step2")
    if d >= 1 and _rows_equal(t):
        out.append("expanded")
    return out


def _strides_of(t, form):
    """(strides, extra) of the view: `extra` = elements before the view's first element inside its block"""
    shape, nat = tuple(t.shape), _dense_strides(t)
    d = len(shape)
    if form == "batch_step2":
        if nat[0] != max(nat):
            raise ValueError("batch_step2: axis 0 must be the outermost axis of the storage")
        return (2 * nat[0],) + nat[1:], 0
    if form == "chan_narrow":
        if d >= 4:
            wide = _channels_last((shape[0], shape[1] + 16) + shape[2:])
            return wide, 8
        wide = _row_major(shape[:-1] + (shape[-1] + 16,))
        return wide, 8
    if form == "other_format":
        return (_row_major(shape) if _is_channels_last(t) else _channels_last(shape)), 0
    if form == "permuted":
        b, tt, i = shape
        return (i, b * i, 1), 0
    if form == "last_step2":
        return tuple(2 * s for s in _row_major(shape)), 0
    if form == "expanded":
        return (0,) + nat[1:], 0
    raise ValueError("unknown form %r (one of %s)" % (form, FORMS))


def _span(shape, strides):
    return 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if all(shape) else 1


def _filled(n, dtype, device):
    buf = torch.empty(n, dtype=dtype, device=device)
    if dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.uint8).fill_(FILL_BYTE)
    return buf


def view_of(t, form):
    """(view, buffer) of one form; ValueError when the form does not apply to t"""
    if form not in applicable(t):
        raise ValueError("form %r does not apply to a tensor of shape %s (applicable: %s)" % (form, tuple(t.shape), applicable(t)))
    t = t.detach()
    strides, extra = _strides_of(t, form)
    esz = t.element_size()
    slack = SLACK_BYTES // esz
    block = extra + max(_span(tuple(t.shape), strides), t.numel())   # a dense misread of numel elements stays inside the block
    buf = _filled(block + 2 * slack + 16 // esz, t.dtype, t.device)
    first = buf.data_ptr() + (slack + extra) * esz
    off = slack + extra + ((-first) % 16) // esz
    v = buf.as_strided(tuple(t.shape), strides, off)
    if form == "expanded":
        v[0:1].copy_(t[0:1])
    else:
        v.copy_(t)
    assert v.data_ptr() % 16 == 0 or esz > 16
    assert v.data_ptr() - buf.data_ptr() >= SLACK_BYTES
    assert (buf.data_ptr() + buf.numel() * esz) - (v.data_ptr() + max(_span(tuple(t.shape), strides), t.numel()) * esz) >= SLACK_BYTES
    return v, buf


def views_of(t, kinds=None):
    """yield (name, view, buffer) for every form in `kinds` (None: every applicable one).  A form asked for by name that does not
    apply to t raises ValueError: a case never loses a form without a word."""
    for form in (applicable(t) if kinds is None else kinds):
        v, buf = view_of(t, form)
        yield form, v, buf


def addressed(buffer, view):
    """bool mask over the 1-D buffer: the elements the view addresses"""
    n = buffer.numel()
    idx = torch.arange(n, device=buffer.device).as_strided(tuple(view.shape), tuple(view.stride()),
                                                           view.storage_offset() - buffer.storage_offset())
    mask = torch.zeros(n, dtype=torch.bool, device=buffer.device)
    mask[idx.reshape(-1)] = True
    return mask


def gaps_intact(buffer, view):
    """True when every element of the buffer outside the view still holds its fill pattern"""
    assert buffer.dim() == 1 and view.untyped_storage().data_ptr() == buffer.untyped_storage().data_ptr()
    rest = buffer[~addressed(buffer, view)]
    if buffer.dtype.is_floating_point:
        return bool(torch.isnan(rest).all())
    return bool((rest.contiguous().view(torch.uint8) == FILL_BYTE).all())


def is_dense_as(view, t):
    """True when the view is stored exactly as the dense tensor t is (same strides): the layout the entry takes as it is"""
    return tuple(view.stride()) == tuple(t.stride())


def flat_with_gaps(tensors, gap=5):
    """the tensors as views (their own shapes and strides) of ONE flat NaN-filled buffer, `gap` elements (rounded so that every
    view starts on the 16-byte grid) between neighbours -> (views, buffer): parameters carved from a flat storage"""
    esz = tensors[0].element_size()
    per = 16 // esz
    step = lambda t: (_span(tuple(t.shape), _dense_strides(t)) + gap + per - 1) // per * per  # noqa: E731
    slack = SLACK_BYTES // esz
    buf = _filled(2 * slack + per + sum(step(t) for t in tensors), tensors[0].dtype, tensors[0].device)
    at = slack + ((-(buf.data_ptr() + slack * esz)) % 16) // esz
    views = []
    for t in tensors:
        v = buf.as_strided(tuple(t.shape), tuple(t.stride()), at)
        v.copy_(t.detach())
        views.append(v)
        at += step(t)
    return views, buf


def gaps_intact_many(buffer, views):
    mask = torch.zeros(buffer.numel(), dtype=torch.bool, device=buffer.device)
    for v in views:
        mask |= addressed(buffer, v)
    return bool(torch.isnan(buffer[~mask]).all())
