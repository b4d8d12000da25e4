"""Host-side plumbing between torch tensors and the C-ABI (include/btx.h).

torch is used here for device memory, streams and layout views only; all arithmetic of the hot path on a GPU
tensor happens inside libbtx.so.  CPU tensors take the ATen route (`*_aten` below: the reference's own op chain —
BASELINE.json config 0, "plumbing, no GPU"); a CUDA tensor NEVER does: if the library is missing or a case is
unsupported the call raises.
"""
import ctypes
import math
import os

import torch
import torch.nn.functional as F

from . import _lib
from . import rng as _rng

_PRECISION = os.environ.get("BTX_PRECISION", "f32")  # "f32" (parity mode) | "bf16x3" | "bf16" (throughput mode)
PRECISIONS = ("f32", "bf16", "bf16x3")


def set_precision(prec):
    """Contraction precision of the HIP path: "f32" = v_mfma_f32_32x32x2_f32 (exact f32 fma chain, parity to
    ~1e-6 rel), "bf16" = v_mfma_f32_32x32x16_bf16 with f32 accumulation (rel-L2 ~3e-3, stated in DESIGN.md),
    "bf16x3" = split-bf16: f32 activations, operands as hi + lo bf16, three bf16 MFMAs per product (rel-L2 ~1e-6 per
    layer: inside north_star's 1e-4 at a third of the bf16 matrix rate)."""
    global _PRECISION
    if prec not in PRECISIONS:
        raise ValueError("precision must be one of %s" % (PRECISIONS,))
    _PRECISION = prec


def get_precision():
    return _PRECISION


# Successive contraction launches walk their tiles in alternating directions (BTX_FLAG_REVERSE on every other call): a
# layer then starts on the activations its producer wrote last.  Values do not depend on it.
_ALT_ORDER = True
_ORDER_TOGGLE = [0]
_OUT_LAYOUT = "channels_last"
_CONCURRENT = False  # set by mc.GraphedMC(lanes > 1) while it captures: BTX_FLAG_CONCURRENT on every contraction launch


class concurrent_plan:
    """context manager: plan the contraction launches issued inside for device throughput (BTX_FLAG_CONCURRENT) — what
    mc.GraphedMC(lanes > 1) does while it captures.  The K-split of small-map layers, hence the f32 summation order, can
    differ from the default (latency) plan by rounding."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global _CONCURRENT
        self.prev, _CONCURRENT = _CONCURRENT, self.on
        return self

    def __exit__(self, *exc):
        global _CONCURRENT
        _CONCURRENT = self.prev
        return False


def set_output_layout(layout):
    """Memory format of the HIP path's convolution outputs.  "channels_last" (default): the kernels' native layout —
    logical [N,C,*sp] shape with channels-last strides, zero extra passes, but `out.view(N, -1)` on a map with H,W > 1
    raises like for any channels_last tensor (use `.reshape` / `.flatten`).  "contiguous": one extra HBM pass per layer
    makes the outputs plain contiguous NCHW, for user code written against the reference that calls `.view`."""
    global _OUT_LAYOUT
    if layout not in ("channels_last", "contiguous"):
        raise ValueError("layout must be 'channels_last' or 'contiguous'")
    _OUT_LAYOUT = layout


def _triple(v, nd, fill):
    """int or nd-tuple -> 3-tuple in (D, H, W) order, padded in front with `fill`."""
    if isinstance(v, int):
        v = (v,) * max(nd, 1)
    v = tuple(int(a) for a in v)
    if len(v) != max(nd, 1) and nd > 0:
        raise ValueError("expected %d values, got %r" % (nd, v))
    if nd == 0:
        return (fill, fill, fill)
    return (fill,) * (3 - nd) + v


class OpDesc:
    """Geometry of one variational contraction (Linear: nd=0)."""

    __slots__ = ("nd", "transposed", "kernel", "stride", "padding", "dilation", "output_padding", "groups",
                 "in_channels", "out_channels")

    def __init__(self, nd, in_channels, out_channels, kernel=1, stride=1, padding=0, dilation=1, groups=1,
                 transposed=False, output_padding=0):
        self.nd, self.transposed, self.groups = nd, bool(transposed), int(groups)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel = _triple(kernel, nd, 1)
        self.stride = _triple(stride, nd, 1)
        self.padding = _triple(padding, nd, 0)
        self.dilation = _triple(dilation, nd, 1)
        self.output_padding = _triple(output_padding, nd, 0)

    def out_spatial(self, spatial):
        out = []
        for i, k, s, p, d, op in zip(spatial, self.kernel, self.stride, self.padding, self.dilation,
                                     self.output_padding):
            if self.transposed:
                out.append((i - 1) * s - 2 * p + d * (k - 1) + op + 1)
            else:
                out.append((i + 2 * p - d * (k - 1) - 1) // s + 1)
        return tuple(out)


def pack_gemm_major(w, op):
    """logical parameter tensor -> the kernel's [N][tap][Cg] f32 layout (a pure layout permute).
    Linear [out,in]: unchanged.  Conv [Cout, Cin/g, *k] -> [Cout, *k, Cin/g] (== channels_last storage).
    ConvTranspose [Cin, Cout/g, *k] -> [g, Cout/g, taps, Cin/g]."""
    if op.nd == 0:
        return w.contiguous()
    if not op.transposed:
        perm = (0,) + tuple(range(2, 2 + op.nd)) + (1,)
        return w.permute(perm).contiguous()
    g = op.groups
    cin, ng = w.shape[0], w.shape[1]
    t = w.reshape(g, cin // g, ng, -1)  # [g, Cg, Ng, T]
    return t.permute(0, 2, 3, 1).contiguous()  # [g, Ng, T, Cg]


def gemm_major_param(shape, op):
    """Allocate a parameter whose STORAGE is the kernel's [N][tap][Cg] layout and return the logical view the
    reference exposes ([out,in] / [Cout,Cin/g,*k] / [Cin,Cout/g,*k]).  The HIP path then reads the parameter in
    place — no packed copy that could go stale when user code mutates `param.data` (which does not bump
    `_version`).  ConvTranspose with groups > 1 has no strided logical view and stays contiguous (re-packed on
    every forward)."""
    nd = op.nd
    if nd == 0:
        return torch.empty(shape)
    k = tuple(shape[2:])
    if not op.transposed:
        phys = torch.empty((shape[0],) + k + (shape[1],))
        return phys.permute((0, nd + 1) + tuple(range(1, nd + 1)))
    if op.groups == 1:
        phys = torch.empty((shape[1],) + k + (shape[0],))  # [Cout][*k][Cin]
        return phys.permute((nd + 1, 0) + tuple(range(1, nd + 1)))
    return torch.empty(shape)


def on_grid(t):
    """`t` itself when its first element lies on the 16-byte grid the vector kernels address (every tensor that comes straight from
    torch's allocator does), else ONE copy in fresh storage with the same shape and strides — what the entry points that refuse an
    off-grid pointer with BTX_E_ALIGN are handed instead (DESIGN.md "Alignment contract").  A dense view into a flat buffer
    (`as_strided`, a dlpack / frombuffer import, parameters carved from one storage at 4-byte offsets) is the tensor this is for.
    The copy is an ordinary stream-ordered launch: inside a captured region it is a node of the graph like any other."""
    if t is None or t.data_ptr() % 16 == 0:
        return t
    return torch.empty_like(t, memory_format=torch.preserve_format).copy_(t)


def gemm_major_view(w, op):
    """The [N][tap][Cg]-ordered tensor of a parameter: a zero-copy view when the parameter is stored GEMM-major
    (the default, see gemm_major_param) on the 16-byte grid, else a packed copy made now.  (A parameter off the grid — a view of
    a flat buffer at some 4-byte offset — is copied on every call: never stale, and the contraction, the pre-sampling and the
    data gradient's weight pass keep their granule kernels, hence their bits.)"""
    nd = op.nd
    w = w.detach()
    if w.dtype != torch.float32:
        raise _lib.BtxError("variational parameters must be float32 (got %s)" % w.dtype)
    if nd == 0:
        return on_grid(w) if w.is_contiguous() else w.contiguous()
    if not op.transposed:
        v = w.permute((0,) + tuple(range(2, 2 + nd)) + (1,))
        return on_grid(v) if v.is_contiguous() else v.contiguous()
    if op.groups == 1:
        v = w.permute((1,) + tuple(range(2, 2 + nd)) + (0,))
        return on_grid(v) if v.is_contiguous() else v.contiguous()
    return pack_gemm_major(w, op)


_WS = {}
_GEOM_CACHE = {}  # (id(op), batch, extent, kind, dtypes, flags) -> (BtxGeom, workspace bytes, op)

# optional per-launch HIP-event timing of btx_contract_fwd (bench.py's roofline leg).  Events are recorded on the
# stream the kernel is launched on (torch's current stream == the stream handed to the C-ABI).
_LAUNCH_LOG = None


def enable_launch_timing(on=True):
    global _LAUNCH_LOG
    _LAUNCH_LOG = [] if on else None


def launch_log():
    """[(tag, flops, start_event, end_event)] recorded since enable_launch_timing(True)."""
    return _LAUNCH_LOG


def _workspace(device, nbytes, stream):
    key = (device, stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def _to_channels_last(x, op):
    """-> (physical channels-last contiguous tensor, NB, (D,H,W), restore(out_phys, out_spatial) -> logical)."""
    if op.nd == 0:
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        return x2, x2.shape[0], (1, 1, 1), lambda o, sp: o.reshape(*lead, op.out_channels)
    if x.dim() == op.nd + 1:  # unbatched [C,*sp], as ATen's convolutions accept
        xp, nb, sp, restore = _to_channels_last(x.unsqueeze(0), op)
        return xp, nb, sp, lambda o, s_: restore(o, s_).squeeze(0)
    if x.dim() != op.nd + 2:
        raise ValueError("expected %dD input, got %dD" % (op.nd + 2, x.dim()))
    nb = x.shape[0]
    if op.nd == 1:
        x4 = x.unsqueeze(2).contiguous(memory_format=torch.channels_last)
        return x4, nb, (1, 1, x.shape[2]), lambda o, sp: o.squeeze(2)
    if op.nd == 2:
        return (x.contiguous(memory_format=torch.channels_last), nb, (1, x.shape[2], x.shape[3]),
                lambda o, sp: o)
    return (x.contiguous(memory_format=torch.channels_last_3d), nb, tuple(x.shape[2:]), lambda o, sp: o)


def _alloc_out(op, nb, out_sp, dtype, device):
    if op.nd == 0:
        return torch.empty((nb, op.out_channels), dtype=dtype, device=device)
    if op.nd == 3:
        return torch.empty((nb, op.out_channels) + tuple(out_sp), dtype=dtype, device=device,
                           memory_format=torch.channels_last_3d)
    return torch.empty((nb, op.out_channels, out_sp[1], out_sp[2]), dtype=dtype, device=device,
                       memory_format=torch.channels_last)


def _sign_to_int8_cl(s, op):
    """explicit +/-1 sign tensor in logical layout -> int8 channels-last physical buffer."""
    phys, _, _, _ = _to_channels_last(s.to(torch.int8), op)
    return phys


def _weight_geom(op):
    """BtxGeom carrying what the sampled-weight tile layout depends on (N, K = taps*C/groups, groups)"""
    g = _lib.Geom()
    g.NB, g.D, g.H, g.W = 1, max(op.kernel[0], 1), max(op.kernel[1], 1), max(op.kernel[2], 1)
    g.C, g.N = op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd = g.sh = g.sw = 1
    g.dd = g.dh = g.dw = 1
    g.groups = op.groups
    return g


def sample_weights(items, seed, sample_idx, prec, device, sample_dev=None, lanes=1, bufs=None, skip_mu=False):
    """btx_sample_weights[_lanes]: ONE launch samples the weights of every layer in `items` for MC sample `sample_idx`
    (lanes > 1: for the samples sample_idx .. sample_idx + lanes - 1, or the `lanes` indices in `sample_dev`).
    items = [(kind, op, mu_p, rho_p, layer_id[, src_kw, src_c])] with GEMM-major f32 mu/rho as handed to contract_hip —
    or, with (src_kw, src_c), the UNPADDED weights of the padded geometry `op` (BtxSampleItem.src_KW/src_C); returns
    the list of uint8 tile buffers, to be passed as contract_hip(..., sampled_w=buf).  `bufs`: buffers of an earlier
    call with the same items to fill again; with skip_mu the mean tiles they hold are kept (BTX_SAMPLE_SKIP_MU: the
    caller vouches that mu has not changed since)."""
    L = _lib.lib()
    if not items:
        return []
    prec_c = _lib.PREC_CODE[prec]
    arr = (_lib.SampleItem * len(items))()
    geoms, outs = [], []
    for i, (kind, op, mu_p, rho_p, layer_id, *src) in enumerate(items):
        g = _weight_geom(op)
        geoms.append(g)
        nbytes = L.btx_sampled_w_bytes_lanes(ctypes.byref(g), kind, prec_c, int(lanes))
        if nbytes == 0:
            raise _lib.BtxError("btx_sampled_w_bytes: unsupported geometry")
        buf = bufs[i] if bufs is not None else torch.empty(nbytes, dtype=torch.uint8, device=device)
        if buf.numel() != nbytes:
            raise _lib.BtxError("sample_weights: buffer %d does not match the item (bytes %d != %d)" % (i, buf.numel(), nbytes))
        outs.append(buf)
        arr[i].geom = ctypes.pointer(g)
        arr[i].mu_w, arr[i].rho_w, arr[i].out = mu_p.data_ptr(), rho_p.data_ptr(), buf.data_ptr()
        arr[i].kind, arr[i].layer_id = kind, int(layer_id) & 0xFFFFFFFF
        if src:
            arr[i].src_KW, arr[i].src_C = int(src[0]), int(src[1])
    stream = torch.cuda.current_stream(device).cuda_stream
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, 0, sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_sample_weights_lanes(arr, len(items), ctypes.byref(r), prec_c, stream, int(lanes),
                                          _lib.SAMPLE_SKIP_MU if skip_mu else 0))
    return outs


_REFUSED_CACHE = {}


def _lanes_refused(kind, op, nb, spatial, dtype, out_dtype, prec_c, extra_flags, lanes):
    """True when btx_contract_fwd_lanes would refuse this launch (BTX_E_UNSUPPORTED) for its lane count alone"""
    flags = (_lib.FLAG_TRANSPOSED if op.transposed else 0) | extra_flags | (lanes << _lib.FLAG_LANES_SHIFT)
    if out_dtype is not None and out_dtype != dtype:
        flags |= _lib.FLAG_OUT_BF16 if out_dtype == torch.bfloat16 else _lib.FLAG_OUT_F32
    act = _lib.ACT_BF16 if dtype == torch.bfloat16 else _lib.ACT_F32
    key = (id(op), nb, spatial, kind, act, prec_c, flags)
    hit = _REFUSED_CACHE.get(key)
    if hit is None or hit[1] is not op:
        L = _lib.lib()
        g = _lib.Geom()
        g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
        g.KD, g.KH, g.KW = op.kernel
        g.sd, g.sh, g.sw = op.stride
        g.pd, g.ph, g.pw = op.padding
        g.dd, g.dh, g.dw = op.dilation
        g.od, g.oh, g.ow = op.output_padding
        g.groups = op.groups
        info = _lib.PlanInfo()
        rc = L.btx_contract_plan_info(kind, ctypes.byref(g), act, prec_c, flags, None, ctypes.byref(info))
        if len(_REFUSED_CACHE) > 4096:
            _REFUSED_CACHE.clear()
        hit = _REFUSED_CACHE[key] = (rc == _lib.E_UNSUPPORTED and
                                     L.btx_contract_plan_info(kind, ctypes.byref(g), act, prec_c, flags & ~_lib.FLAG_LANES_MASK,
                                                              None, ctypes.byref(info)) == 0, op)
    return hit[0]


def act_code(act):
    """BtxEpilogue.relu of an activation request: None / False -> 0, True / "relu" -> 1, "relu6" -> 2"""
    if isinstance(act, str):
        codes = {"none": 0, "relu": 1, "relu6": 2}
        if act not in codes:
            raise ValueError("epilogue activation must be one of %s, got %r" % (sorted(codes), act))
        return codes[act]
    if act is None or isinstance(act, bool):
        return int(bool(act))
    if act in (0, 1, 2):
        return int(act)
    raise ValueError("epilogue activation code must be 0, 1 or 2, got %r" % (act,))


def apply_act_aten(out, act):
    """the epilogue activation as ATen ops (CPU, autograd): act_code 1 -> relu, 2 -> clamp to [0, 6]"""
    code = act_code(act)
    if code == 1:
        return torch.relu(out)
    if code == 2:
        return torch.clamp(out, 0.0, 6.0)
    return out


def contract_hip(kind, x, mu_p, rho_p, mu_b, rho_b, op, seed, sample_idx, layer_id, prec=None, noise=None,
                 extra_flags=0, out_dtype=None, epilogue=None, sampled_w=None, sample_dev=None, lanes=1, lane_batch=None,
                 self_sampling_weights=None):
    """One fused sample-and-contract forward on the GPU (btx_contract_fwd).  `mu_p`/`rho_p` are GEMM-major packed.
    `noise` (parity mode) = dict with optional eps_w (logical weight layout), eps_b, sign_in, sign_out.
    lanes > 1 (btx_contract_fwd_lanes): `lanes` MC samples in one launch.  x holds either the lanes' inputs back to
    back along the batch axis (lanes * lane_batch rows / images) or ONE input shared by all lanes (lane_batch rows);
    the output always holds the lanes back to back.  Sample indices: sample_idx + lane, or the `lanes` words of
    sample_dev.  self_sampling_weights: callable -> (mu_p, rho_p) a launch that samples for itself must read, for callers
    that pass `sampled_w` together with parameters the launch cannot sample from (the row-fused stem hands over its
    UNPADDED mu/rho when pre-sampled tiles exist); used by the per-lane fallback below, which drops the lane-batched tiles."""
    L = _lib.lib()
    if not x.is_cuda:
        raise _lib.BtxError("contract_hip needs a CUDA (ROCm) tensor")
    if x.dtype == torch.float32:
        act = _lib.ACT_F32
    elif x.dtype == torch.bfloat16:
        act = _lib.ACT_BF16
    else:
        raise _lib.BtxError("activations must be float32 or bfloat16, got %s" % x.dtype)
    prec = prec or _PRECISION
    prec_c = _lib.PREC_CODE[prec]
    xp, nb, spatial, restore = _to_channels_last(x, op)
    out_sp = op.out_spatial(spatial)
    if min(out_sp) <= 0:
        raise ValueError("output size is too small")
    lanes = int(lanes)
    nb_out, x_shared = nb, False
    if lanes > 1:
        if noise:
            raise _lib.BtxError("explicit noise tensors are single-sample (lanes == 1)")
        if lane_batch is None:
            raise _lib.BtxError("lanes > 1 needs lane_batch")
        rows = int(lane_batch) * (nb // x.shape[0] if (op.nd == 0 and x.dim() > 1 and x.shape[0] > 0) else 1)
        if nb == rows:
            x_shared, nb_out = True, rows * lanes
        elif nb != rows * lanes:
            raise _lib.BtxError("lanes=%d x lane_batch=%d does not match the input batch %d" % (lanes, lane_batch, x.shape[0]))
        nb = rows  # the geometry of ONE lane
        # btx_contract_fwd_lanes wants 16-byte lane strides.  A layer whose per-lane tensors are not (a 10-class head at an
        # odd batch: 10 * bs * 4 bytes) runs its lanes as single-sample launches planned like lanes (BTX_FLAG_CONCURRENT):
        # the same values, one launch per lane instead of one
        esz_o = (out_dtype or x.dtype).itemsize
        out_lane = nb * out_sp[0] * out_sp[1] * out_sp[2] * op.out_channels * esz_o
        x_lane = 0 if x_shared else (xp.numel() // lanes) * xp.element_size()
        pooled = epilogue is not None and epilogue.get("pool")
        # ... and so does a layer whose launch the library refuses for its lane count (btx_contract_plan_info: the pre-sampled
        # tiles of all lanes would outgrow the 32-bit descriptor offsets and move the samples onto another kernel)
        if not pooled and (((x_lane | out_lane) & 15) or _lanes_refused(kind, op, nb, spatial, x.dtype, out_dtype, prec_c,
                                                                         extra_flags, lanes)):
            outs = []
            if sampled_w is not None and self_sampling_weights is not None:
                mu_p, rho_p = self_sampling_weights()  # the single-lane launches sample in registers, from these
            elif sampled_w is not None and (extra_flags & _lib.FLAG_ROWFUSE):
                raise _lib.BtxError("row-fused launch with pre-sampled tiles and unaligned lane strides: the per-lane fallback "
                                    "needs the padded parameters (self_sampling_weights)")
            xl = x.reshape((lanes, -1) + tuple(x.shape[1:])) if not x_shared else None
            res = epilogue.get("residual") if epilogue is not None else None
            for l in range(lanes):
                ep_l = epilogue
                if res is not None:
                    ep_l = dict(epilogue, residual=res.reshape((lanes, -1) + tuple(res.shape[1:]))[l])
                with concurrent_plan():
                    outs.append(contract_hip(kind, x if x_shared else xl[l], mu_p, rho_p, mu_b, rho_b, op, seed,
                                             int(sample_idx) + l, layer_id, prec=prec, extra_flags=extra_flags,
                                             out_dtype=out_dtype, epilogue=ep_l,
                                             sample_dev=sample_dev[l:l + 1] if sample_dev is not None else None))
            return torch.cat(outs, 0)
    flags = (_lib.FLAG_TRANSPOSED if op.transposed else 0) | extra_flags | (_lib.FLAG_CONCURRENT if _CONCURRENT else 0)
    if lanes > 1:
        flags |= lanes << _lib.FLAG_LANES_SHIFT
    rev = 0
    if _ALT_ORDER:
        _ORDER_TOGGLE[0] ^= 1
        rev = _lib.FLAG_REVERSE if _ORDER_TOGGLE[0] else 0
    if out_dtype is not None and out_dtype != x.dtype:
        flags |= _lib.FLAG_OUT_BF16 if out_dtype == torch.bfloat16 else _lib.FLAG_OUT_F32
    # the geometry struct and the workspace size depend on shapes only: built once per (op, batch, extent, modes)
    gkey = (id(op), nb, spatial, kind, act, prec_c, flags)
    cached = _GEOM_CACHE.get(gkey)
    if cached is None or cached[2] is not op:
        g = _lib.Geom()
        g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
        g.KD, g.KH, g.KW = op.kernel
        g.sd, g.sh, g.sw = op.stride
        g.pd, g.ph, g.pw = op.padding
        g.dd, g.dh, g.dw = op.dilation
        g.od, g.oh, g.ow = op.output_padding
        g.groups = op.groups
        if len(_GEOM_CACHE) > 4096:
            _GEOM_CACHE.clear()
        cached = _GEOM_CACHE[gkey] = (g, L.btx_contract_workspace_bytes(ctypes.byref(g), kind, act, prec_c, flags), op)
    g, need = cached[0], cached[1]
    if epilogue is not None and epilogue.get("pool"):  # BtxEpilogue.pool: `out` is the max-pooled tensor
        hq, wq = ctypes.c_int32(0), ctypes.c_int32(0)
        if not L.btx_contract_pool_shape(ctypes.byref(g), act, prec_c, flags, ctypes.byref(hq), ctypes.byref(wq)):
            raise _lib.BtxError("the fused stem max-pool is not available for this geometry (contract_pool_ok)")
        out_sp = (1, hq.value, wq.value)
    out = _alloc_out(op, nb_out, out_sp, out_dtype or x.dtype, x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    ws = _workspace(x.device, need, stream) if need else None
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    keep = []
    nz = None
    if sampled_w is not None:
        nz = _lib.Noise()
        nz.sampled_w = sampled_w.data_ptr()
        keep.append(sampled_w)
    if noise:
        nz = nz or _lib.Noise()
        if noise.get("eps_w_packed") is not None:  # already in the GEMM-major order of `op` (dgrad_weights_hip)
            t = noise["eps_w_packed"]
            keep.append(t); nz.eps_w = t.data_ptr()
        elif noise.get("eps_w") is not None:
            t = pack_gemm_major(noise["eps_w"].to(device=x.device, dtype=torch.float32), op)
            keep.append(t); nz.eps_w = t.data_ptr()
        if noise.get("eps_b") is not None:
            t = noise["eps_b"].to(device=x.device, dtype=torch.float32).contiguous()
            keep.append(t); nz.eps_b = t.data_ptr()
        if noise.get("sign_in") is not None:
            t = _sign_to_int8_cl(noise["sign_in"].to(x.device), op)
            keep.append(t); nz.sign_in = t.data_ptr()
        if noise.get("sign_out") is not None:
            so = noise["sign_out"].to(x.device)
            if op.nd == 0:
                so = so.reshape(-1, op.out_channels)
            t = _sign_to_int8_cl(so, op)
            keep.append(t); nz.sign_out = t.data_ptr()
    ev0 = None
    if _LAUNCH_LOG is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record(torch.cuda.current_stream(x.device))
    ep = None
    if epilogue is not None:  # dict(scale, shift, residual, relu): eval-BN / residual / ReLU folded into the store
        ep = _lib.Epilogue()
        for name in ("scale", "shift"):
            t = epilogue.get(name)
            if t is not None:
                if t.dtype != torch.float32 or t.numel() != op.out_channels or not t.is_contiguous():
                    raise ValueError("epilogue %s must be a contiguous float32 [out_channels] tensor" % name)
                keep.append(t)
                setattr(ep, name, t.data_ptr())
        res = epilogue.get("residual")
        if res is not None:
            if op.nd == 0:
                res = res.reshape(-1, op.out_channels)
            rp, _, _, _ = _to_channels_last(res, OpDesc(op.nd, op.out_channels, op.out_channels))
            rp = on_grid(rp)  # the store side adds it in 16-byte granules: an off-grid residual would cost the launch its kernel
            if rp.dtype != out.dtype or rp.numel() != out.numel():
                raise ValueError("epilogue residual must match the output shape and dtype")
            keep.append(rp)
            ep.residual = rp.data_ptr()
        ep.relu = act_code(epilogue.get("relu"))
        ep.pool = 1 if epilogue.get("pool") else 0
    args = (kind, ctypes.byref(g), xp.data_ptr(), mu_p.data_ptr(), rho_p.data_ptr(),
            mu_b.data_ptr() if mu_b is not None else None, rho_b.data_ptr() if rho_b is not None else None,
            out.data_ptr(), ctypes.byref(r), ctypes.byref(nz) if nz is not None else None,
            act, prec_c, flags | rev, ws.data_ptr() if ws is not None else None,
            ws.numel() if ws is not None else 0, stream, ctypes.byref(ep) if ep is not None else None)
    if lanes > 1:
        ln = _lib.Lanes()
        ln.n = lanes
        ln.x_stride = 0 if x_shared else (xp.numel() // lanes) * xp.element_size()
        ln.out_stride = (out.numel() // lanes) * out.element_size()
        ln.res_stride = ln.out_stride
        rc = L.btx_contract_fwd_lanes(*args, ctypes.byref(ln))
    else:
        rc = L.btx_contract_fwd_ex(*args)
    if rc == _lib.E_UNSUPPORTED and ep is not None and ep.relu == 2:
        # a store side without ReLU6 (the stem + max-pool kernel): the same launch with ReLU, then the upper bound.
        # min(., 6) commutes with the rounding and with a max-pool, so the result is what ReLU6 in the store gives.
        ep.relu = 1
        rc = L.btx_contract_fwd_lanes(*args, ctypes.byref(ln)) if lanes > 1 else L.btx_contract_fwd_ex(*args)
        _lib.check(rc)
        out.clamp_(max=6.0)
    _lib.check(rc)
    if ev0 is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(torch.cuda.current_stream(x.device))
        m_rows = nb_out * out_sp[0] * out_sp[1] * out_sp[2]
        k_red = op.kernel[0] * op.kernel[1] * op.kernel[2] * (op.in_channels // op.groups)
        flops = 2.0 * m_rows * op.out_channels * k_red * (2 if kind == _lib.KIND_FLIPOUT else 1)
        tag = "%s/%s/%s k%dx%dx%d cin%d cout%d M%d" % ("flipout" if kind else "reparam", prec,
                                                     "bf16" if act == _lib.ACT_BF16 else "f32", op.kernel[0],
                                                     op.kernel[1], op.kernel[2], op.in_channels, op.out_channels, m_rows)
        _LAUNCH_LOG.append((tag, flops, ev0, ev1))
    if op.nd == 0 and x_shared:
        # a Linear layer that reads ONE input for all lanes (the first layer of an MLP): the output stacks the lanes along the
        # leading axis — [lanes * d0, *d1.., N] — where `restore` would fold it back into the input's own leading shape
        res = out.reshape((lanes * x.shape[0],) + tuple(x.shape[1:-1]) + (op.out_channels,))
    else:
        res = restore(out, out_sp)
    return res.contiguous() if (_OUT_LAYOUT == "contiguous" and op.nd > 0) else res


WGRAD_ATOMICS = False  # A/B and tests: accumulate the weight gradient with f32 atomics instead of chunk slabs
BIAS_ATOMICS = False   # A/B (tools/bias_grad_bench.py): the bias gradient as the weight-gradient kernel's by-product (f32 atomics over its chunks)


def wgrad_hip(kind, x, dy, op, seed, sample_idx, layer_id, w_shape, signs=None, swap=False, bias=False, rowfuse=None,
              _flags=0, raw=False, sample_dev=None, rho_flat=None):
    """btx_contract_wgrad: (dW_mu, dW_delta | None, db_mu | None, db_delta | None) in the layer's LOGICAL weight layout
    (f32).  `op` is a plain (non-transposed) contraction; `signs` = (sign_in, sign_out) logical +/-1 tensors for layers
    whose forward ran on padded layouts, else the forward's hashed signs are regenerated.  `rowfuse` = the layer's
    rowfuse_plan(): the gradient is taken on the row-fused geometry the forward ran on (hashed signs, a kernel row as the
    channel axis) and un-padded here.  `rho_flat` (with raw=True): the layer's rho in GEMM-major order — a fifth result, drho =
    dW * eps * sigmoid(rho) (dW = dW_delta, whose buffer then HOLDS drho, for Flipout; dW_mu for Reparameterization), formed by the
    slab reduction launch itself (btx_contract_wgrad_ws) or, on the atomics path, by btx_rho_grad."""
    L = _lib.lib()
    if op.transposed:
        raise _lib.BtxError("wgrad_hip wants the plain-convolution geometry (exchange x and dy for transposed layers)")
    if rowfuse is not None:
        plan, fop = rowfuse, rowfuse["op"]
        xin = rowfuse_input(x, plan, dy.dtype)
        fo = fop.out_spatial((1, plan["Hp"], plan["Wp"]))
        if (fo[1], fo[2]) != tuple(dy.shape[2:]):  # the forward computed (and dropped) extra rows / columns: their dy is 0
            dy = F.pad(dy, (0, fo[2] - dy.shape[3], 0, fo[1] - dy.shape[2]))
        kh, kwp, cp, kw, cin = fop.kernel[1], plan["kwp"], plan["cp"], plan["kw"], plan["cin"]
        dwm, dwd, dbm, dbd = wgrad_hip(kind, xin, dy, fop, seed, sample_idx, layer_id, (fop.out_channels, cp, kh, kwp),
                                       bias=bias, _flags=_lib.FLAG_ROWFUSE, sample_dev=sample_dev)
        un = lambda t: t[:, :cin, :, :kw].contiguous() if t is not None else None  # noqa: E731
        return un(dwm), un(dwd), dbm, dbd
    xp, nb, spatial, _ = _to_channels_last(x, op)
    yop = OpDesc(op.nd, op.out_channels, op.out_channels)
    dy2 = dy.reshape(-1, op.out_channels) if op.nd == 0 else dy
    dyp, _, _, _ = _to_channels_last(dy2, yop)
    if xp.dtype != dyp.dtype:
        dyp = dyp.to(xp.dtype)
    act = _lib.ACT_BF16 if xp.dtype == torch.bfloat16 else _lib.ACT_F32
    if xp.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.BtxError("activations must be float32 or bfloat16, got %s" % xp.dtype)
    g = _lib.Geom()
    g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.groups = op.groups
    n, kred = op.out_channels, op.kernel[0] * op.kernel[1] * op.kernel[2] * (op.in_channels // op.groups)
    dev = x.device
    dwm = torch.empty(n * kred, dtype=torch.float32, device=dev)
    flip = kind == _lib.KIND_FLIPOUT
    dwd = torch.empty(n * kred, dtype=torch.float32, device=dev) if flip else None
    dbm = torch.empty(n, dtype=torch.float32, device=dev) if bias else None
    dbd = torch.empty(n, dtype=torch.float32, device=dev) if (bias and flip) else None
    nz, keep = None, []
    if signs is not None and flip:
        nz = _lib.Noise()
        si = _sign_to_int8_cl(signs[0].reshape(x.shape), op)
        so = _sign_to_int8_cl(signs[1].reshape(dy2.shape), yop)
        keep += [si, so]
        nz.sign_in, nz.sign_out = si.data_ptr(), so.data_ptr()
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    flags = (_lib.FLAG_SWAP_SIGNS if swap else 0) | _flags
    # the pixel chunks' partial sums go to slabs that a second launch adds in chunk order (deterministic; f32 atomics from 2048
    # workgroups cost more than the slab round trip — profiles/r05_experiments.txt E13).  WGRAD_ATOMICS: the round 2-5 path.
    wsb = 0 if WGRAD_ATOMICS else int(L.btx_wgrad_workspace_bytes(kind, ctypes.byref(g), act, flags))
    drho = None
    if rho_flat is not None:
        if not raw:
            raise _lib.BtxError("wgrad_hip: rho_flat goes with raw=True (GEMM-major buffers)")
        if rho_flat.dtype != torch.float32 or not rho_flat.is_contiguous() or rho_flat.numel() != n * kred:
            raise _lib.BtxError("wgrad_hip: rho_flat must be the contiguous f32 GEMM-major rho of the layer")
        drho = dwd if flip else torch.empty_like(dwm)
    if wsb > 0:
        # the slab path adds the WEIGHT gradient's chunks in a fixed order, but the kernel's bias sums would still meet in f32 atomics
        # (last bit = arrival order of the chunks): the bias gradients come from btx_bias_grad instead, in a fixed order as well
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        own = bias and not BIAS_ATOMICS
        _lib.check(L.btx_contract_wgrad_ws(kind, ctypes.byref(g), xp.data_ptr(), dyp.data_ptr(), dwm.data_ptr(), ptr(dwd),
                                           None if own else ptr(dbm), None if own else ptr(dbd), ctypes.byref(r),
                                           ctypes.byref(nz) if nz is not None else None,
                                           act, flags, ws.data_ptr(), wsb, ptr(rho_flat), ptr(drho), stream))
        if own:
            m_px = dyp.numel() // n
            bws = torch.empty(int(L.btx_bias_grad_workspace_bytes(m_px, n)) // 4, dtype=torch.float32, device=dev)
            _lib.check(L.btx_bias_grad(kind, dyp.data_ptr(), m_px, n, act, dbm.data_ptr(), ptr(dbd), ctypes.byref(r),
                                       nz.sign_out if nz is not None else None, flags, bws.data_ptr(), bws.numel() * 4, stream))
    else:
        _lib.check(L.btx_contract_wgrad(kind, ctypes.byref(g), xp.data_ptr(), dyp.data_ptr(), dwm.data_ptr(), ptr(dwd),
                                        ptr(dbm), ptr(dbd), ctypes.byref(r), ctypes.byref(nz) if nz is not None else None,
                                        act, flags, torch.cuda.current_stream(dev).cuda_stream))
        if rho_flat is not None:
            rho_grad_hip(dwd if flip else dwm, rho_flat, seed, sample_idx, layer_id, _lib.STREAM_EPS_W, out=drho, sample_dev=sample_dev)
    if raw:  # the flat GEMM-major buffers as the kernel wrote them (autograd: strided logical views, no unpack copies)
        return (dwm, dwd, dbm, dbd) if rho_flat is None else (dwm, dwd, dbm, dbd, drho)
    un = lambda t: unpack_gemm_major(t, w_shape, op) if t is not None else None  # noqa: E731
    return un(dwm), un(dwd), dbm, dbd


def kl_hip(mu, rho, prior_mu, prior_sigma, prior_mu_t=None, prior_sigma_t=None, out=None, accumulate=False):
    """mean Gaussian KL of one parameter tensor on the GPU (btx_kl_gauss) -> 0-d f32 tensor."""
    L = _lib.lib()
    mu_c, rho_c = mu.detach().contiguous(), rho.detach().contiguous()
    if mu_c.dtype != torch.float32 or rho_c.dtype != torch.float32:
        raise _lib.BtxError("KL kernel needs float32 parameters")
    n = mu_c.numel()
    stream = torch.cuda.current_stream(mu.device).cuda_stream
    ws = _workspace(mu.device, L.btx_kl_workspace_bytes(n), stream)
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=mu.device)
    pm = prior_mu_t.detach().contiguous() if prior_mu_t is not None else None
    ps = prior_sigma_t.detach().contiguous() if prior_sigma_t is not None else None
    rc = L.btx_kl_gauss(mu_c.data_ptr(), rho_c.data_ptr(), n, pm.data_ptr() if pm is not None else None,
                        ps.data_ptr() if ps is not None else None, float(prior_mu), float(prior_sigma),
                        out.data_ptr(), _lib.FLAG_KL_ACCUM if accumulate else 0, ws.data_ptr(), ws.numel(), stream)
    _lib.check(rc)
    return out


def _kl_items(entries, grads=None):
    """entries = [(mu, rho, prior_mu, prior_sigma, prior_mu_t|None, prior_sigma_t|None)] of same-order f32 tensors"""
    arr = (_lib.KlItem * len(entries))()
    for i, (mu, rho, pm, ps, pmt, pst) in enumerate(entries):
        arr[i].mu, arr[i].rho, arr[i].n = mu.data_ptr(), rho.data_ptr(), mu.numel()
        arr[i].prior_mu, arr[i].prior_sigma = float(pm), float(ps)
        arr[i].prior_mu_t = pmt.data_ptr() if pmt is not None else None
        arr[i].prior_sigma_t = pst.data_ptr() if pst is not None else None
        if grads is not None:
            arr[i].dmu, arr[i].drho = grads[i][0].data_ptr(), grads[i][1].data_ptr()
    return arr


def kl_model_hip(entries):
    """sum over tensors of the mean Gaussian KL, ONE launch + one final reduce (btx_kl_gauss_model) -> 0-d f32"""
    L = _lib.lib()
    dev = entries[0][0].device
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _workspace(dev, L.btx_kl_model_workspace_bytes(len(entries)), stream)
    out = torch.empty((), dtype=torch.float32, device=dev)
    _lib.check(L.btx_kl_gauss_model(_kl_items(entries), len(entries), out.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return out


def kl_model_bwd_hip(entries, grads, grad_out):
    """d(kl)/d(mu, rho) of every tensor into `grads` [(dmu, drho)] (same element order), scaled by the device scalar
    `grad_out` (btx_kl_gauss_model_bwd)"""
    L = _lib.lib()
    dev = entries[0][0].device
    g = grad_out.detach().reshape(()).to(device=dev, dtype=torch.float32).contiguous()
    _lib.check(L.btx_kl_gauss_model_bwd(_kl_items(entries, grads), len(entries), g.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream))


def _kl_mc_items(entries, grads=None):
    """entries = [(mu, rho, loc_t | None, prior, layer_id, rng_stream, sample_idx, sample_dev | None)]: same-order contiguous f32 tensors,
    a priors.* prior, and the BTX-RNG coordinates of the tensor's draws"""
    arr = (_lib.KlMcItem * len(entries))()
    for i, (mu, rho, loc_t, prior, layer_id, rng_stream, sample_idx, sample_dev) in enumerate(entries):
        it = arr[i]
        it.mu, it.rho, it.n = mu.data_ptr(), rho.data_ptr(), mu.numel()
        it.loc_t = loc_t.data_ptr() if loc_t is not None else None
        pp = tuple(prior.params()) + (0.0, 0.0, 0.0)
        it.prior.type, it.prior.loc = int(prior.code), float(prior.mu)
        it.prior.p0, it.prior.p1, it.prior.p2 = float(pp[0]), float(pp[1]), float(pp[2])
        it.layer_id, it.rng_stream, it.sample_idx = int(layer_id) & 0xFFFFFFFF, int(rng_stream), int(sample_idx) & 0xFFFFFFFF
        it.sample_idx_dev = sample_dev.data_ptr() if sample_dev is not None else None
        if grads is not None:
            it.dmu, it.drho = grads[i][0].data_ptr(), grads[i][1].data_ptr()
    return arr


def kl_mc_model_hip(entries, seed, draws, out=None, accumulate=False):
    """sum over tensors of the sampled mean KL against their non-Gaussian priors (BTX-KLMC v1), ONE launch + one final reduce
    (btx_kl_mc_model) -> 0-d f32.  `out` / accumulate: add to an existing scalar (BTX_FLAG_KL_ACCUM)."""
    L = _lib.lib()
    dev = entries[0][0].device
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _workspace(dev, L.btx_kl_mc_workspace_bytes(len(entries)), stream)
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=dev)
    _lib.check(L.btx_kl_mc_model(_kl_mc_items(entries), len(entries), int(seed), int(draws), out.data_ptr(),
                                 _lib.FLAG_KL_ACCUM if accumulate else 0, ws.data_ptr(), ws.numel(), stream))
    return out


def kl_mc_model_bwd_hip(entries, grads, seed, draws, grad_out):
    """d(kl)/d(mu, rho) of every tensor into `grads` [(dmu, drho)] (same element order, every element written), scaled by the device
    scalar `grad_out`; eps is regenerated (btx_kl_mc_model_bwd)"""
    L = _lib.lib()
    dev = entries[0][0].device
    g = grad_out.detach().reshape(()).to(device=dev, dtype=torch.float32).contiguous()
    _lib.check(L.btx_kl_mc_model_bwd(_kl_mc_items(entries, grads), len(entries), int(seed), int(draws), g.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream))


def kl_mc_aten(mu, sigma, eps, prior, loc=None):
    """BTX-KLMC v1 as differentiable ATen ops on EXPLICIT noise: eps [S, *mu.shape] -> the mean over elements of
    -log sigma - (1 + log 2 pi) / 2 - (1 / S) sum_j log p(mu + sigma eps_j); loc: a tensor location in place of prior.mu.
    The CPU route and backend "torch" (eps from torch's generator), and what the tests model."""
    if eps.dim() != mu.dim() + 1 or tuple(eps.shape[1:]) != tuple(mu.shape):
        raise ValueError("eps must be [S, *mu.shape] (got %s for mu %s)" % (tuple(eps.shape), tuple(mu.shape)))
    w = mu.unsqueeze(0) + sigma.unsqueeze(0) * eps
    cross = prior.log_prob(w, None if loc is None else loc.unsqueeze(0)).mean(0)
    return (-torch.log(sigma) - 0.5 * (1.0 + math.log(2.0 * math.pi)) - cross).mean()


# ---- BTX-SVD v1: the log-uniform prior's KL, log-alpha statistics, pruning -----------------------------------------
SVD_EPS, SVD_K1, SVD_K2, SVD_K3 = 1e-8, 0.63576, 1.87320, 1.48695


def dense_flat(t):
    """the 1-D view of a tensor's storage when its elements fill one dense block in SOME order (contiguous tensors, the permuted views
    of gemm_major_param), else None.  The element-wise kernels of BTX-SVD v1 read and write parameters through it, in place."""
    t = t.detach()
    dims = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1)
    run = 1
    for st, sz in dims:
        if st != run:
            return None
        run *= sz
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


def same_dense_order(a, b):
    """True when a and b (same shape) are both dense and stored in ONE common element order: element k of dense_flat(a) and of
    dense_flat(b) is then the same logical element, which is what the element-wise kernels of BTX-SVD v1 need of (mu, rho)"""
    return tuple(a.stride()) == tuple(b.stride()) and dense_flat(a) is not None and dense_flat(b) is not None


def flat_f32(t):
    """the storage-order view of a parameter for the element-wise kernels; a contiguous copy where the tensor is not dense"""
    if t.dtype != torch.float32:
        raise _lib.BtxError("variational parameters must be float32 (got %s)" % t.dtype)
    v = dense_flat(t)
    return v if v is not None else t.detach().contiguous().reshape(-1)


def _reduce_code(reduction):
    try:
        return {"mean": _lib.REDUCE_MEAN, "sum": _lib.REDUCE_SUM}[reduction]
    except KeyError:
        raise ValueError("reduction must be 'mean' or 'sum' (got %r)" % (reduction,)) from None


def _kl_logu_items(entries, grads=None):
    """entries = [(mu, rho, reduction)]: same-order dense f32 tensors (any 4-byte boundary) and 'mean' | 'sum'"""
    arr = (_lib.KlLogUItem * len(entries))()
    for i, (mu, rho, reduction) in enumerate(entries):
        it = arr[i]
        it.mu, it.rho, it.n, it.reduction = mu.data_ptr(), rho.data_ptr(), mu.numel(), _reduce_code(reduction)
        if grads is not None:
            it.dmu, it.drho = grads[i][0].data_ptr(), grads[i][1].data_ptr()
    return arr


def kl_logu_model_hip(entries, out=None, accumulate=False, terms=False):
    """sum over tensors of the KL against the log-uniform prior (BTX-SVD v1), one launch + one fold per 48 tensors
    (btx_kl_logu_model) -> 0-d f32; terms=True: -> (kl, the per-tensor terms as an f64 device tensor).  `out` / accumulate: add to
    an existing scalar (BTX_FLAG_KL_ACCUM)."""
    L = _lib.lib()
    dev = entries[0][0].device
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _workspace(dev, L.btx_kl_logu_workspace_bytes(len(entries)), stream)
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=dev)
    t = torch.empty(len(entries), dtype=torch.float64, device=dev) if terms else None
    _lib.check(L.btx_kl_logu_model(_kl_logu_items(entries), len(entries), out.data_ptr(), t.data_ptr() if terms else None,
                                   _lib.FLAG_KL_ACCUM if accumulate else 0, ws.data_ptr(), ws.numel(), stream))
    return (out, t) if terms else out


def kl_logu_model_bwd_hip(entries, grads, grad_out):
    """d(kl)/d(mu, rho) of every tensor into `grads` [(dmu, drho)] (same element order, every element written), scaled by the device
    scalar `grad_out` (btx_kl_logu_model_bwd)"""
    L = _lib.lib()
    dev = entries[0][0].device
    g = grad_out.detach().reshape(()).to(device=dev, dtype=torch.float32).contiguous()
    _lib.check(L.btx_kl_logu_model_bwd(_kl_logu_items(entries, grads), len(entries), g.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream))


def log_alpha_aten(mu, sigma):
    """-> (la, inside): la = clamp(2 log sigma - log(mu^2 + EPS), -LA_MAX, LA_MAX) as differentiable ATen ops, with the clamp
    semantics of BTX-SVD v1 — where the raw value lies STRICTLY outside the clamp (sigma that underflowed to 0 included) la is the
    constant bound and both gradients are exactly 0, never 0 * inf; a raw value on a bound passes its gradient."""
    lim = _lib.LOGALPHA_MAX
    with torch.no_grad():
        raw = 2.0 * torch.log(sigma) - torch.log(mu * mu + SVD_EPS)
        inside = (raw >= -lim) & (raw <= lim)
        bound = torch.where(raw > lim, torch.full_like(raw, lim), torch.full_like(raw, -lim))  # NaN: the kernel's fmax / fmin give -LA_MAX
    one = torch.ones_like(mu)
    mu_s, sig_s = torch.where(inside, mu, one), torch.where(inside, sigma, one)
    la = torch.where(inside, 2.0 * torch.log(sig_s) - torch.log(mu_s * mu_s + SVD_EPS), bound)
    return la, inside


def kl_logu_terms_aten(la):
    """kl_i of BTX-SVD v1 from the clamped log alpha (Molchanov et al. 2017, eq. 14)"""
    return SVD_K1 - SVD_K1 * torch.sigmoid(SVD_K2 + SVD_K3 * la) + 0.5 * torch.log1p(torch.exp(-la))


def kl_logu_aten(mu, sigma, reduction="mean"):
    """BTX-SVD v1 as differentiable ATen ops: the mean ("mean") or the sum ("sum") over elements of kl_i.  The CPU route and backend
    "torch", and what the tests model."""
    _reduce_code(reduction)
    t = kl_logu_terms_aten(log_alpha_aten(mu, sigma)[0])
    return t.mean() if reduction == "mean" else t.sum()


def _la_items(entries):
    arr = (_lib.LogAlphaItem * len(entries))()
    for i, (mu, rho) in enumerate(entries):
        arr[i].mu, arr[i].rho, arr[i].n = mu.data_ptr(), rho.data_ptr(), mu.numel()
    return arr


def logalpha_stats_hip(entries, thresholds, bins=0):
    """entries = [(mu, rho)] dense f32 device tensors -> ONE int64 device tensor [n, LOGALPHA_STATS_WORDS + bins]: per tensor the
    counts above each threshold (words 0..7), count(mu == 0) (word 8) and the histogram (btx_logalpha_stats)"""
    L = _lib.lib()
    dev = entries[0][0].device
    n, W = len(entries), _lib.LOGALPHA_STATS_WORDS
    buf = torch.empty(n * (W + bins), dtype=torch.int64, device=dev)
    th = (ctypes.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    _lib.check(L.btx_logalpha_stats(_la_items(entries), n, th, len(thresholds), int(bins), buf.data_ptr(),
                                    buf.data_ptr() + n * W * 8 if bins else None, torch.cuda.current_stream(dev).cuda_stream))
    return torch.cat([buf[:n * W].reshape(n, W), buf[n * W:].reshape(n, bins)], 1) if bins else buf.reshape(n, W)


def logalpha_prune_hip(entries, threshold):
    """mu = 0, rho = RHO_PRUNED wherever la > threshold, IN PLACE through the raw pointers (the caller bumps the versions) -> int64
    device tensor [n]: the pruned count of each tensor (btx_logalpha_prune)"""
    L = _lib.lib()
    dev = entries[0][0].device
    n, W = len(entries), _lib.LOGALPHA_STATS_WORDS
    buf = torch.empty(n * W, dtype=torch.int64, device=dev)
    _lib.check(L.btx_logalpha_prune(_la_items(entries), n, float(threshold), buf.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return buf.reshape(n, W)[:, 0]


def rowfuse_plan(op, x_shape):
    """Geometry of the row-fused execution of a small-C 2-D stem conv (BTX_FLAG_ROWFUSE), or None.  Decided by the
    layer geometry ONLY (never by dtypes), because the BTX-RNG index space of the layer follows this layout.
    The input is zero-padded to [N][Hp][Wp][cp] with the conv padding materialised and the kernel row padded to kwp
    taps; one kernel row = kwp*cp contiguous elements = a whole number of K-stages of the LDS-DMA kernel.
    Even stride_w: cp=4 (8-byte pixels stay 16-byte aligned), else cp=8."""
    if op.nd != 2 or op.transposed or op.groups != 1 or op.in_channels > 4 or op.dilation != (1, 1, 1):
        return None
    kh, kw = op.kernel[1], op.kernel[2]
    sh, sw = op.stride[1], op.stride[2]
    if kw > 8:
        return None
    if sw % 2 == 0:
        cp, kwp = 4, 8
    else:
        cp, kwp = 8, (4 if kw <= 4 else 8)
    ph, pw = op.padding[1], op.padding[2]
    H, W = x_shape[2], x_shape[3]
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    Wp = max((Wo - 1) * sw + kwp, W + 2 * pw)
    Wp += Wp % 2          # row pitch a multiple of 16 bytes for cp=4 bf16
    Hp = H + 2 * ph
    fop = OpDesc(2, cp, op.out_channels, (kh, kwp), (sh, sw), 0, 1, 1)
    return dict(op=fop, Hp=Hp, Wp=Wp, ph=ph, pw=pw, Ho=Ho, Wo=Wo, kw=kw, kwp=kwp, cp=cp, cin=op.in_channels)


def contract_pool_ok(op, nb, spatial, act_dtype, prec, extra_flags=0):
    """True when btx_contract_fwd_ex takes BtxEpilogue.pool = 1 (the ResNet stem's MaxPool2d(3, 2, 1) folded into the
    store of the row-fused stem contraction) for this geometry."""
    L = _lib.lib()
    g = _lib.Geom()
    g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.od, g.oh, g.ow = op.output_padding
    g.groups = op.groups
    act = _lib.ACT_BF16 if act_dtype == torch.bfloat16 else _lib.ACT_F32
    prec_c = _lib.PREC_CODE[prec]
    return bool(L.btx_contract_pool_shape(ctypes.byref(g), act, prec_c, extra_flags, None, None))


def rowfuse_input(x, plan, out_dtype=None):
    """logical [N,C,H,W] -> zero-padded logical [N,cp,Hp,Wp] stored channels-last (in `out_dtype`).  CUDA tensors:
    one pass of btx_rowfuse_pack; CPU tensors: F.pad."""
    n, c, h, w = x.shape
    out_dtype = out_dtype or x.dtype
    if x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and out_dtype in (torch.float32, torch.bfloat16):
        L = _lib.lib()
        out = torch.empty((n, plan["cp"], plan["Hp"], plan["Wp"]), dtype=out_dtype, device=x.device,
                          memory_format=torch.channels_last)
        st = (ctypes.c_int64 * 4)(*x.stride())
        code = lambda dt: _lib.ACT_BF16 if dt == torch.bfloat16 else _lib.ACT_F32
        _lib.check(L.btx_rowfuse_pack(x.data_ptr(), code(x.dtype), st, n, c, h, w, out.data_ptr(), code(out_dtype),
                                      plan["Hp"], plan["Wp"], plan["cp"], plan["ph"], plan["pw"],
                                      torch.cuda.current_stream(x.device).cuda_stream))
        return out
    x = x.to(out_dtype)
    xp = F.pad(x.permute(0, 2, 3, 1), (0, plan["cp"] - c, plan["pw"], plan["Wp"] - w - plan["pw"], plan["ph"],
                                       plan["Hp"] - h - plan["ph"]))
    return xp.permute(0, 3, 1, 2)


def rowfuse_weights(mu_p, rho_p, plan):
    """GEMM-major [Cout,KH,KW,C] -> [Cout,KH,kwp,cp]; the padded taps meet real pixels, so they must contribute
    exactly nothing: mu = 0 and rho = -1e30 (softplus -> 0)."""
    kw, c = plan["kw"], plan["cin"]
    mu_f = F.pad(mu_p, (0, plan["cp"] - c, 0, plan["kwp"] - kw))
    rho_f = F.pad(rho_p, (0, plan["cp"] - c, 0, plan["kwp"] - kw), value=-1e30)
    return mu_f, rho_f


def pad_channels(x, op, extra):
    """zero-pad the channel axis of a logical [N,C,*sp] (or [*,C]) tensor by `extra`, result channels-last"""
    nd = op.nd
    if nd == 0:
        return F.pad(x, (0, extra))
    perm = (0,) + tuple(range(2, 2 + nd)) + (1,)
    xp = F.pad(x.permute(perm), (0, extra))  # contiguous [N,*sp,C+extra]
    return xp.permute((0, nd + 1) + tuple(range(1, nd + 1)))


LSTM_PRECISIONS = ("f32", "bf16")  # btx_lstm_fwd's forms; bf16x3 LSTMs run the eager per-step loop


def _lstm_layer(p, lanes=1):
    """BtxLstmLayer of (mu_w, rho_w, mu_b, rho_b, layer_id, sample_idx, sample_dev)"""
    mu_w, rho_w, mu_b, rho_b, lid, s, sdev = p
    for t in (mu_w, rho_w, mu_b, rho_b):
        if t is not None:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.BtxError("LSTM parameters must be contiguous float32")
    if sdev is not None and (sdev.dtype != torch.int32 or sdev.numel() != lanes):
        raise _lib.BtxError("sample_dev must be an int32 tensor with one word per lane")
    return _lib.LstmLayer(mu_w.data_ptr(), rho_w.data_ptr(), mu_b.data_ptr() if mu_b is not None else None,
                          rho_b.data_ptr() if rho_b is not None else None, int(lid) & 0xFFFFFFFF,
                          int(s) & 0xFFFFFFFF, sdev.data_ptr() if sdev is not None else None)


def _lstm_act(x):
    if x.dtype == torch.float32:
        return _lib.ACT_F32
    if x.dtype == torch.bfloat16:
        return _lib.ACT_BF16
    raise _lib.BtxError("activations must be float32 or bfloat16, got %s" % x.dtype)


def _lstm_train_prec(prec):
    prec = prec or _PRECISION
    if prec not in LSTM_PRECISIONS:
        raise _lib.BtxError("the fused LSTM sequence has no %s form" % prec)
    return prec


def lstm_train_fwd_hip(kind, x, ih, hh, seed, prec=None, h0=None, c0=None, kl_terms=None):
    """The forward of a fused LSTM training step (btx_lstm_fwd_train, one lane): lstm_hip's (hidden_seq, c_seq, kl), bit for
    bit, plus `saved` — the f32 gate pre-activations and cell states lstm_bwd_hip needs.  ih / hh as in lstm_hip (sample_dev:
    one word); h0 / c0 [B, H] or None."""
    L = _lib.lib()
    if not x.is_cuda:
        raise _lib.BtxError("lstm_train_fwd_hip needs a CUDA (ROCm) tensor")
    act, prec = _lstm_act(x), _lstm_train_prec(prec)
    B, T, I = x.shape
    H = ih[0].shape[0] // 4
    x = x.contiguous()
    li, lh = _lstm_layer(ih), _lstm_layer(hh)
    if hh[0].shape[1] != H or ih[0].shape[1] != I:
        raise _lib.BtxError("LSTM parameter shapes do not match the input (I=%d, H=%d)" % (I, H))
    if h0 is not None:
        if h0.shape != (B, H) or c0 is None or c0.shape != (B, H):
            raise _lib.BtxError("h0 / c0 must be [B, H] = [%d, %d]" % (B, H))
        h0, c0 = h0.to(x.dtype).contiguous(), c0.to(x.dtype).contiguous()
    hs = torch.empty(B, T, H, dtype=x.dtype, device=x.device)
    cs = torch.empty_like(hs)
    need = L.btx_lstm_train_workspace_bytes(B, H, T)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    nsv = L.btx_lstm_train_saved_bytes(B, H, T)
    saved = torch.empty(nsv, dtype=torch.uint8, device=x.device)
    kl = ki = kh = None
    if kl_terms is not None:
        ki, kh = (k.detach().to(torch.float32).reshape(1).contiguous() for k in kl_terms)
        kl = torch.empty((), dtype=torch.float32, device=x.device)
    _lib.check(L.btx_lstm_fwd_train(_lib.KIND_FLIPOUT if kind == _lib.KIND_FLIPOUT else _lib.KIND_REPARAM, ctypes.byref(li),
                                    ctypes.byref(lh), int(seed) & 0xFFFFFFFFFFFFFFFF, x.data_ptr(),
                                    h0.data_ptr() if h0 is not None else None, c0.data_ptr() if c0 is not None else None,
                                    hs.data_ptr(), cs.data_ptr(), ki.data_ptr() if ki is not None else None,
                                    kh.data_ptr() if kh is not None else None, kl.data_ptr() if kl is not None else None,
                                    B, I, H, T, act, _lib.PREC_CODE[prec], ws.data_ptr(), need, saved.data_ptr(), nsv,
                                    torch.cuda.current_stream(x.device).cuda_stream))
    return hs, cs, kl, saved


def lstm_bwd_hip(kind, x, ih, hh, seed, hidden_seq, saved, d_hidden_seq=None, d_c_seq=None, prec=None, h0=None, c0=None,
                 want_dx=True, want_dh0=False, want_dc0=False, want_ih=True, want_hh=True):
    """The backward through time of one lstm_train_fwd_hip call with the same arguments (btx_lstm_bwd).  d_hidden_seq / d_c_seq
    [B, T, H] or None.  Returns (dx, dh0, dc0, grads_ih, grads_hh); grads_* = (dmu_w, drho_w, dmu_b, drho_b) f32 (bias entries
    None without bias), None where not wanted."""
    L = _lib.lib()
    act, prec = _lstm_act(x), _lstm_train_prec(prec)
    B, T, I = x.shape
    H = ih[0].shape[0] // 4
    x = x.contiguous()
    li, lh = _lstm_layer(ih), _lstm_layer(hh)
    if h0 is not None:
        h0, c0 = h0.to(x.dtype).contiguous(), c0.to(x.dtype).contiguous()
    dev = x.device
    d_hs = d_hidden_seq.to(x.dtype).contiguous() if d_hidden_seq is not None else None
    d_cs = d_c_seq.to(x.dtype).contiguous() if d_c_seq is not None else None
    dx = torch.empty(B, T, I, dtype=x.dtype, device=dev) if want_dx else None
    dh0 = torch.empty(B, H, dtype=x.dtype, device=dev) if want_dh0 else None
    dc0 = torch.empty(B, H, dtype=x.dtype, device=dev) if want_dc0 else None

    def grads(p, want):
        if not want:
            return None, None
        mu_w, mu_b = p[0], p[2]
        g = (torch.empty_like(mu_w), torch.empty_like(mu_w), torch.empty_like(mu_b) if mu_b is not None else None,
             torch.empty_like(mu_b) if mu_b is not None else None)
        return g, _lib.LstmGrads(*(t.data_ptr() if t is not None else None for t in g))

    gi, si = grads(ih, want_ih)
    gh, sh = grads(hh, want_hh)
    need = L.btx_lstm_train_workspace_bytes(B, H, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    _lib.check(L.btx_lstm_bwd(_lib.KIND_FLIPOUT if kind == _lib.KIND_FLIPOUT else _lib.KIND_REPARAM, ctypes.byref(li),
                              ctypes.byref(lh), int(seed) & 0xFFFFFFFFFFFFFFFF, x.data_ptr(), ptr(h0), ptr(c0),
                              hidden_seq.data_ptr(), saved.data_ptr(), ptr(d_hs), ptr(d_cs), ptr(dx), ptr(dh0), ptr(dc0),
                              ctypes.byref(si) if si is not None else None, ctypes.byref(sh) if sh is not None else None,
                              B, I, H, T, act, _lib.PREC_CODE[prec], ws.data_ptr(), need,
                              torch.cuda.current_stream(dev).cuda_stream))
    return dx, dh0, dc0, gi, gh


def lstm_hip(kind, x, ih, hh, seed, prec=None, lanes=1, batch=None, h0=None, c0=None, kl_terms=None):
    """The whole sequence of a Bayesian LSTM in one call (btx_lstm_fwd: 1 + T launches enqueued on the current stream).
    x [rows, T, I] (f32 / bf16); ih / hh = (mu_w [4H, K], rho_w, mu_b [4H] or None, rho_b, layer_id, sample_idx, sample_dev):
    step t of a layer draws the noise of sample index sample_idx + lane + t, or sample_dev[lane] + t when sample_dev (an
    int32 tensor with one word per lane) is given.  lanes > 1: rows == batch (one input, shared by the lanes) or lanes * batch
    (lane l's rows at l * B); h0 / c0 hold lanes * B rows.  kl_terms = (kl_ih, kl_hh): f32 scalars whose per-step sum
    over the T steps is returned as the third value (else None).  Returns (hidden_seq, c_seq, kl), [lanes * B, T, H]."""
    L = _lib.lib()
    if not x.is_cuda:
        raise _lib.BtxError("lstm_hip needs a CUDA (ROCm) tensor")
    if x.dtype == torch.float32:
        act = _lib.ACT_F32
    elif x.dtype == torch.bfloat16:
        act = _lib.ACT_BF16
    else:
        raise _lib.BtxError("activations must be float32 or bfloat16, got %s" % x.dtype)
    prec = prec or _PRECISION
    if prec not in LSTM_PRECISIONS:
        raise _lib.BtxError("the fused LSTM sequence has no %s form" % prec)
    lanes = int(lanes)
    rows, T, I = x.shape
    H = ih[0].shape[0] // 4
    B, x_shared = rows, 0
    if lanes > 1:
        if batch is None:
            raise _lib.BtxError("lanes > 1 needs batch (rows per lane)")
        B = int(batch)
        if rows == B:
            x_shared = 1
        elif rows != lanes * B:
            raise _lib.BtxError("lanes=%d x batch=%d does not match the input rows %d" % (lanes, B, rows))
    x = x.contiguous()
    keep = [x]
    li, lh = _lstm_layer(ih, lanes), _lstm_layer(hh, lanes)
    if hh[0].shape[1] != H or ih[0].shape[1] != I:
        raise _lib.BtxError("LSTM parameter shapes do not match the input (I=%d, H=%d)" % (I, H))
    if h0 is not None:
        if h0.shape != (lanes * B, H) or c0 is None or c0.shape != (lanes * B, H):
            raise _lib.BtxError("h0 / c0 must be [lanes * B, H] = [%d, %d]" % (lanes * B, H))
        h0, c0 = h0.to(x.dtype).contiguous(), c0.to(x.dtype).contiguous()
        keep += [h0, c0]
    hs = torch.empty(lanes * B, T, H, dtype=x.dtype, device=x.device)
    cs = torch.empty_like(hs)
    need = L.btx_lstm_workspace_bytes(lanes, B, H, T)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    kl = None
    ki = kh = None
    if kl_terms is not None:
        ki, kh = (k.detach().to(torch.float32).reshape(1).contiguous() for k in kl_terms)
        keep += [ki, kh]
        kl = torch.empty((), dtype=torch.float32, device=x.device)
    _lib.check(L.btx_lstm_fwd(_lib.KIND_FLIPOUT if kind == _lib.KIND_FLIPOUT else _lib.KIND_REPARAM, ctypes.byref(li),
                              ctypes.byref(lh), int(seed) & 0xFFFFFFFFFFFFFFFF, x.data_ptr(), x_shared,
                              h0.data_ptr() if h0 is not None else None, c0.data_ptr() if c0 is not None else None,
                              hs.data_ptr(), cs.data_ptr(), ki.data_ptr() if ki is not None else None,
                              kh.data_ptr() if kh is not None else None, kl.data_ptr() if kl is not None else None,
                              lanes, B, I, H, T, act, _lib.PREC_CODE[prec], ws.data_ptr(), need,
                              torch.cuda.current_stream(x.device).cuda_stream))
    return hs, cs, kl


def fill_eps_hip(n, device, seed, sample_idx, layer_id, rng_stream, sample_dev=None):
    """BTX-RNG v1 eps for a flat index space of n elements, as a flat f32 CUDA tensor.  sample_dev: the sample index lives in
    that device word (captured steps) and sample_idx is ignored."""
    L = _lib.lib()
    out = torch.empty(int(n), dtype=torch.float32, device=device)
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_fill_eps(out.data_ptr(), out.numel(), ctypes.byref(r), rng_stream,
                              torch.cuda.current_stream(out.device).cuda_stream))
    return out


def rho_grad_hip(dw_flat, rho_flat, seed, sample_idx, layer_id, rng_stream, out=None, sample_dev=None):
    """btx_rho_grad: drho = dw * eps * sigmoid(rho) over flat f32 tensors in the same (GEMM-major) element order, eps
    regenerated inside the kernel.  `out` may be dw_flat itself."""
    L = _lib.lib()
    if out is None:
        out = torch.empty_like(dw_flat)
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_rho_grad(dw_flat.data_ptr(), rho_flat.data_ptr(), out.data_ptr(), dw_flat.numel(), ctypes.byref(r),
                              rng_stream, torch.cuda.current_stream(dw_flat.device).cuda_stream))
    return out


def dgrad_weights_hip(mu_p, rho_p, n, taps, c, flip, seed, sample_idx, layer_id, sample_dev=None):
    """btx_dgrad_weights: (mu, rho, eps) of the data gradient's transposed geometry, GEMM-major [c][taps][n] f32, from the layer's
    own GEMM-major parameters [n][taps][c] in ONE launch (eps = the forward's draw, regenerated)."""
    L = _lib.lib()
    dev = mu_p.device
    outs = [torch.empty(int(c) * int(taps) * int(n), dtype=torch.float32, device=dev) for _ in range(3)]
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_dgrad_weights(mu_p.data_ptr(), rho_p.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                   int(n), int(taps), int(c), 1 if flip else 0, ctypes.byref(r),
                                   torch.cuda.current_stream(dev).cuda_stream))
    return outs


# --------------------------------------------------------------------------------------------------------------------
# fused training of the local reparameterization layers (csrc/btx_lrt.hip; DESIGN.md §21 "Backward")
# --------------------------------------------------------------------------------------------------------------------
def _lrt_geom(op, nb, spatial):
    g = _lib.Geom()
    g.NB, (g.D, g.H, g.W), g.C, g.N = nb, spatial, op.in_channels, op.out_channels
    g.KD, g.KH, g.KW = op.kernel
    g.sd, g.sh, g.sw = op.stride
    g.pd, g.ph, g.pw = op.padding
    g.dd, g.dh, g.dw = op.dilation
    g.groups = op.groups
    return g


_LRT_OK_CACHE = {}


def lrt_bwd_workspace_bytes(op, nb, spatial, act, prec_c):
    """(return code, bytes) of btx_lrt_bwd_workspace_bytes for the plain geometry `op` on `nb` images of extent `spatial`"""
    need = ctypes.c_size_t(0)
    rc = _lib.lib().btx_lrt_bwd_workspace_bytes(ctypes.byref(_lrt_geom(op, nb, spatial)), act, prec_c, ctypes.byref(need))
    return rc, int(need.value)


def lrt_train_ok(layer, x):
    """True when a forward of the LocalReparameterization `layer` on `x` that needs gradients goes through autograd.LrtFn (the fused
    HIP forward + backward, btx_lrt_fwd_train / btx_lrt_bwd): `layer.fused_training` is on, x is a CUDA f32 / bf16 tensor on the HIP
    backend, the precision is f32 or bf16, and the geometry is covered — Linear, or Conv2d with groups == 1 whose stride-1 padding
    does not exceed the dilated kernel extent (channel-padded small-C stems run on their padded geometry).  False: the ATen
    composite (_forward_lrt_train), as before."""
    if getattr(layer, "_family", None) != "lrt" or not getattr(layer, "fused_training", False):
        return False
    if not (layer._use_hip(x) and layer._needs_grad(x)) or x.dtype not in (torch.float32, torch.bfloat16):
        return False
    prec = layer.precision or _PRECISION
    op = layer._op_pad if layer._btx_cpad is not None else layer._op
    if prec == "bf16x3" or op.nd not in (0, 2) or op.transposed or x.numel() == 0:
        return False
    if op.nd == 0:
        nb, spatial = x.numel() // x.shape[-1], (1, 1, 1)
    else:
        if x.dim() not in (3, 4):
            return False
        nb, spatial = (x.shape[0] if x.dim() == 4 else 1), (1, x.shape[-2], x.shape[-1])
    act = _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32
    key = (id(op), nb, spatial, act, prec)
    hit = _LRT_OK_CACHE.get(key)
    if hit is None or hit[1] is not op:
        if len(_LRT_OK_CACHE) > 4096:
            _LRT_OK_CACHE.clear()
        hit = _LRT_OK_CACHE[key] = (lrt_bwd_workspace_bytes(op, nb, spatial, act, _lib.PREC_CODE[prec])[0] == 0, op)
    return hit[0]


def lrt_fwd_train_hip(x, mu_p, rho_p, mu_b, rho_b, op, seed, sample_idx, layer_id, prec=None, sample_dev=None):
    """btx_lrt_fwd_train: (out, root) — `out` what contract_hip(KIND_LRT, ...) returns for the same arguments, bit for bit, and
    root = sqrtf(v + sigma_b^2) as a flat f32 tensor in the channels-last element order of `out`"""
    L = _lib.lib()
    act = _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32
    prec_c = _lib.PREC_CODE[prec or _PRECISION]
    xp, nb, spatial, restore = _to_channels_last(x, op)
    out_sp = op.out_spatial(spatial)
    if min(out_sp) <= 0:
        raise ValueError("output size is too small")
    out = _alloc_out(op, nb, out_sp, x.dtype, x.device)
    root = torch.empty(out.numel(), dtype=torch.float32, device=x.device)
    flags = _lib.FLAG_CONCURRENT if _CONCURRENT else 0
    if _ALT_ORDER:
        _ORDER_TOGGLE[0] ^= 1
        flags |= _lib.FLAG_REVERSE if _ORDER_TOGGLE[0] else 0
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_lrt_fwd_train(ctypes.byref(_lrt_geom(op, nb, spatial)), xp.data_ptr(), mu_p.data_ptr(), rho_p.data_ptr(),
                                   mu_b.data_ptr() if mu_b is not None else None, rho_b.data_ptr() if rho_b is not None else None,
                                   out.data_ptr(), root.data_ptr(), ctypes.byref(r), act, prec_c, flags,
                                   torch.cuda.current_stream(x.device).cuda_stream))
    res = restore(out, out_sp)
    return (res.contiguous() if (_OUT_LAYOUT == "contiguous" and op.nd > 0) else res), root


def lrt_bwd_hip(x, dy, root, mu_p, rho_p, rho_b, op, seed, sample_idx, layer_id, prec=None, sample_dev=None, want_x=True,
                want_w=True, want_b=True, out_dx=None):
    """btx_lrt_bwd: (dx | None, dmu_flat | None, drho_flat | None, dmu_b | None, drho_b | None) of one LRT layer from the gradient `dy`
    of its output and the forward's `root`.  dmu / drho: flat GEMM-major f32 buffers (gemm_major_logical_view gives the logical views);
    dx in x's dtype, channels-last.  All in one host call; the scratch is the stream's workspace."""
    L = _lib.lib()
    act = _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32
    prec_c = _lib.PREC_CODE[prec or _PRECISION]
    xp, nb, spatial, _ = _to_channels_last(x, op)
    yop = OpDesc(op.nd, op.out_channels, op.out_channels)
    dy2 = dy.reshape(-1, op.out_channels) if op.nd == 0 else dy
    dyp, _, _, _ = _to_channels_last(dy2 if dy2.dtype == x.dtype else dy2.to(x.dtype), yop)
    if dyp.numel() != root.numel():
        raise _lib.BtxError("lrt_bwd_hip: dy does not match the saved root (%d != %d elements)" % (dyp.numel(), root.numel()))
    dev = x.device
    g = _lrt_geom(op, nb, spatial)
    need = ctypes.c_size_t(0)
    _lib.check(L.btx_lrt_bwd_workspace_bytes(ctypes.byref(g), act, prec_c, ctypes.byref(need)))
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _workspace(dev, int(need.value), stream)
    n, kred = op.out_channels, op.kernel[0] * op.kernel[1] * op.kernel[2] * op.in_channels
    dmu = torch.empty(n * kred, dtype=torch.float32, device=dev) if want_w else None
    drho = torch.empty(n * kred, dtype=torch.float32, device=dev) if want_w else None
    has_b = rho_b is not None and want_b
    dmu_b = torch.empty(n, dtype=torch.float32, device=dev) if has_b else None
    drho_b = torch.empty(n, dtype=torch.float32, device=dev) if has_b else None
    dx = None
    if want_x:
        dx = out_dx if out_dx is not None else torch.empty_like(xp)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    grads = _lib.LrtGrads(ptr(dmu), ptr(drho), ptr(dmu_b), ptr(drho_b), ptr(dx))
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    _lib.check(L.btx_lrt_bwd(ctypes.byref(g), xp.data_ptr(), dyp.data_ptr(), root.data_ptr(), mu_p.data_ptr(), rho_p.data_ptr(),
                             ptr(rho_b), ctypes.byref(grads), ctypes.byref(r), act, prec_c, ws.data_ptr(), ws.numel(), stream))
    if dx is not None and op.nd == 0:
        dx = dx.reshape(x.shape)
    return dx, dmu, drho, dmu_b, drho_b


def fill_sign_hip(n, device, seed, sample_idx, layer_id, rng_stream):
    L = _lib.lib()
    out = torch.empty(int(n), dtype=torch.int8, device=device)
    r = _lib.Rng(int(seed), int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF)
    _lib.check(L.btx_fill_sign(out.data_ptr(), out.numel(), ctypes.byref(r), rng_stream,
                               torch.cuda.current_stream(out.device).cuda_stream))
    return out


def gemm_major_logical_view(buf, w_shape, op):
    """The logical-shape tensor (reference layout [out,in] / [Cout,Cin/g,*k] / [Cin,Cout/g,*k]) over a GEMM-major buffer
    `buf` (what gemm_major_view / pack_gemm_major produce): a strided VIEW of `buf` where one exists — the inverse of
    gemm_major_param — else (ConvTranspose with groups > 1) an unpacked copy."""
    nd = op.nd
    if nd == 0:
        return buf.reshape(w_shape)
    k = tuple(w_shape[2:])
    if not op.transposed:
        return buf.reshape((w_shape[0],) + k + (w_shape[1],)).permute((0, nd + 1) + tuple(range(1, nd + 1)))
    if op.groups == 1:
        return buf.reshape((w_shape[1],) + k + (w_shape[0],)).permute((nd + 1, 0) + tuple(range(1, nd + 1)))
    return unpack_gemm_major(buf.reshape(-1), w_shape, op)


def unpack_gemm_major(flat, w_shape, op):
    """inverse of pack_gemm_major for a flat [N*taps*Cg] tensor -> logical parameter layout."""
    if op.nd == 0:
        return flat.reshape(w_shape)
    k = tuple(w_shape[2:])
    if not op.transposed:
        t = flat.reshape((w_shape[0],) + k + (w_shape[1],))
        perm = (0, op.nd + 1) + tuple(range(1, op.nd + 1))
        return t.permute(perm).contiguous()
    g = op.groups
    cin, ng = w_shape[0], w_shape[1]
    t = flat.reshape(g, ng, -1, cin // g).permute(0, 3, 1, 2).contiguous()  # [g, Cg, Ng, T]
    return t.reshape((cin, ng) + k)


# --------------------------------------------------------------------------------------------------------------
# ATen route for CPU tensors (BASELINE.json config 0) and for autograd-on-request (`backend="torch"`).
# Same op chain and the same torch-generator draw order as the reference methods cited in each layer class.
# --------------------------------------------------------------------------------------------------------------
_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}
_CONVT = {1: F.conv_transpose1d, 2: F.conv_transpose2d, 3: F.conv_transpose3d}


def contract_aten(x, w, b, op):
    nd = op.nd
    if nd == 0:
        return F.linear(x, w, b)
    st, pd, dl, opd = op.stride[3 - nd:], op.padding[3 - nd:], op.dilation[3 - nd:], op.output_padding[3 - nd:]
    if op.transposed:
        return _CONVT[nd](x, w, b, st, pd, opd, op.groups, dl)
    return _CONV[nd](x, w, b, st, pd, dl, op.groups)


def plain_layout(t):
    """row-major copy with DEFAULT strides (`.contiguous()` is not enough: a [Cout,Cin,1,1] view with
    channels-last-looking strides already counts as contiguous and would steer ATen's conv to channels_last)."""
    return t.clone(memory_format=torch.contiguous_format)


def softplus_naive(rho):
    return torch.log1p(torch.exp(rho))


def kl_aten(mu_q, sigma_q, mu_p, sigma_p):
    kl = torch.log(sigma_p) - torch.log(sigma_q) + (sigma_q ** 2 + (mu_q - mu_p) ** 2) / (2 * (sigma_p ** 2)) - 0.5
    return kl.mean()


def maxpool2d_hip(x, kernel, stride, padding):
    """torch.nn.functional.max_pool2d for channels-last CUDA tensors through btx_maxpool2d_cl (C % 8 == 0)"""
    L = _lib.lib()
    n, c, h, w = x.shape
    xp = on_grid(x.contiguous(memory_format=torch.channels_last))
    ho, wo = (h + 2 * padding - kernel) // stride + 1, (w + 2 * padding - kernel) // stride + 1
    out = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    _lib.check(L.btx_maxpool2d_cl(xp.data_ptr(), out.data_ptr(), _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32,
                                  n, h, w, c, kernel, stride, padding, torch.cuda.current_stream(x.device).cuda_stream))
    return out


def maxpool2d_train_hip(x, kernel, stride, padding):
    """(y, idx) of btx_maxpool2d_cl_train: max_pool2d of a channels-last CUDA tensor and, per output element, the window position of
    its maximum (uint8 [N][Ho][Wo][C]) for maxpool2d_bwd_hip"""
    L = _lib.lib()
    n, c, h, w = x.shape
    x = on_grid(x)
    ho, wo = (h + 2 * padding - kernel) // stride + 1, (w + 2 * padding - kernel) // stride + 1
    out = torch.empty((n, c, ho, wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    idx = torch.empty(n * ho * wo * c, dtype=torch.uint8, device=x.device)
    _lib.check(L.btx_maxpool2d_cl_train(x.data_ptr(), out.data_ptr(), idx.data_ptr(), _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32,
                                        n, h, w, c, kernel, stride, padding, torch.cuda.current_stream(x.device).cuda_stream))
    return out, idx


def maxpool2d_bwd_hip(dy, idx, x_shape, kernel, stride, padding):
    """btx_maxpool2d_cl_bwd: the gradient of maxpool2d_train_hip's input (channels-last), dy channels-last"""
    L = _lib.lib()
    n, c, h, w = x_shape
    dy = on_grid(dy)
    dx = torch.empty((n, c, h, w), dtype=dy.dtype, device=dy.device, memory_format=torch.channels_last)
    _lib.check(L.btx_maxpool2d_cl_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), _lib.ACT_BF16 if dy.dtype == torch.bfloat16 else _lib.ACT_F32,
                                      n, h, w, c, kernel, stride, padding, torch.cuda.current_stream(dy.device).cuda_stream))
    return dx


def avgpool_global_hip(x):
    """adaptive_avg_pool2d(x, 1).flatten(1) for channels-last CUDA tensors through btx_avgpool_global_cl (C % 8 == 0)"""
    L = _lib.lib()
    n, c, h, w = x.shape
    xp = on_grid(x.contiguous(memory_format=torch.channels_last))
    out = torch.empty((n, c), dtype=x.dtype, device=x.device)
    _lib.check(L.btx_avgpool_global_cl(xp.data_ptr(), out.data_ptr(), _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32,
                                       n, h * w, c, torch.cuda.current_stream(x.device).cuda_stream))
    return out


# --------------------------------------------------------------------------------------------------------------------
# Monte-Carlo dropout — BTX-DROP v1 (csrc/btx_drop.hip, include/btx_drop.h)
# --------------------------------------------------------------------------------------------------------------------
DROP_MODES = {"element": _lib.DROP_ELEMENT, "channel": _lib.DROP_CHANNEL}


def dropout_params(p):
    """(T, scale) of BTX-DROP v1 for the drop probability `p`: T = clamp(floor((1 - p) * 65536 + 0.5), 0, 65536) in double — an
    element is kept iff its sixteen random bits are below T, so the effective keep probability is T / 65536 — and scale =
    f32(65536.0 / T), divided in double and rounded once (0.0 when T = 0)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got {}".format(p))
    T = min(65536, max(0, int(math.floor((1.0 - p) * 65536.0 + 0.5))))
    scale = float(torch.tensor(65536.0 / T, dtype=torch.float64).to(torch.float32)) if T else 0.0
    return T, scale


def _drop_geom(shape, mode):
    """(N, C, S, logical) of a lane-stacked tensor of `shape`: the examples x channels x spatial positions BTX-DROP v1 indexes.
    Element mode reads tensors of rank <= 3 as plain row-major ([B, F], [B, T, F]: S = 1); channel mode needs rank >= 3."""
    shape = tuple(int(v) for v in shape)
    if mode not in DROP_MODES:
        raise ValueError("dropout mode must be 'element' or 'channel' (got %r)" % (mode,))
    if mode == "channel" and len(shape) < 3:
        raise _lib.BtxError("channel dropout (MCDropout1d/2d/3d) needs an input of rank >= 3, got shape %r" % (shape,))
    if len(shape) == 0:
        return 1, 1, 1
    if mode == "channel" or len(shape) >= 4:
        return shape[0], shape[1], math.prod(shape[2:])
    return shape[0], math.prod(shape[1:]), 1


def _mulhilo32(a, m):
    """(high, low) 32-bit words of a * m for an int64 tensor a in [0, 2^32) and a Python constant m < 2^32, in 16-bit halves: no
    intermediate leaves [0, 2^34)"""
    m_lo, m_hi = m & 0xFFFF, m >> 16
    a_lo, a_hi = a & 0xFFFF, a >> 16
    p00 = a_lo * m_lo
    mid = a_lo * m_hi + a_hi * m_lo + (p00 >> 16)
    return a_hi * m_hi + (mid >> 16), ((mid & 0xFFFF) << 16) | (p00 & 0xFFFF)


def philox4x32_10_aten(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/btx_rng.h) on int64 tensors / Python ints holding 32-bit words; returns the four output words"""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0 = torch.as_tensor(c0, dtype=torch.int64)
    c1, c2, c3 = (torch.as_tensor(v, dtype=torch.int64, device=c0.device) for v in (c1, c2, c3))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        h0, l0 = _mulhilo32(c0, M0)
        h1, l1 = _mulhilo32(c2, M1)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def dropout_index_aten(shape, mode, device="cpu"):
    """the BTX-DROP v1 element index of every LOGICAL element of one lane's tensor of `shape` (int64, in the logical shape): the
    position in channels-last order [n][spatial...][c] (rank <= 3: plain row-major), or n * C + c in channel mode"""
    shape = tuple(int(v) for v in shape)
    N, C, S = _drop_geom(shape, mode)
    if mode == "channel":
        return torch.arange(N * C, dtype=torch.int64, device=device).reshape((N, C) + (1,) * (len(shape) - 2)).expand(shape)
    if len(shape) < 4:
        return torch.arange(N * C * S, dtype=torch.int64, device=device).reshape(shape)
    nd = len(shape) - 2
    return torch.arange(N * C * S, dtype=torch.int64, device=device).reshape((N,) + shape[2:] + (C,)).permute(
        (0, nd + 1) + tuple(range(1, nd + 1)))


def dropout_mask_aten(shape, T, mode, seed, sample_idx, layer_id, device="cpu"):
    """The bool KEEP mask of BTX-DROP v1 for one lane's logical tensor of `shape` from torch integer ops: the same bits as
    btx_dropout_fwd draws, on any device (CPU tensors, backend "torch", dtypes other than f32 / bf16 — and the tests)."""
    i = dropout_index_aten(shape, mode, device)
    if i.numel() > _lib.DROP_MAX_ELEMENTS:
        raise _lib.BtxError("dropout: a lane tensor of more than 2^35 elements")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    P = philox4x32_10_aten(i >> 3, int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF, _lib.STREAM_DROP,
                           seed & 0xFFFFFFFF, seed >> 32)
    w = (i >> 1) & 3
    word = torch.where(w == 0, P[0], torch.where(w == 1, P[1], torch.where(w == 2, P[2], P[3])))
    h = (word >> (16 * (i & 1))) & 0xFFFF
    return h < int(T)


def dropout_apply_aten(x, mask, scale):
    """kept: x * scale as ONE f32 multiply rounded once to x's dtype (float64 tensors multiply in float64); dropped: +0.0 by
    selection, so a dropped inf / NaN gives 0.  Differentiable: the gradient is where(mask, dy * scale, 0)."""
    if x.dtype == torch.float64:
        kept = x * float(scale)
    else:
        kept = (x.float() * float(scale)).to(x.dtype)
    return torch.where(mask, kept, torch.zeros((), dtype=x.dtype, device=x.device))


def _drop_lane_rows(x, lanes, lane_batch):
    rows = int(x.shape[0]) if x.dim() else 1
    if lanes <= 1:
        return rows, False
    if lane_batch is None or rows not in (int(lane_batch), lanes * int(lane_batch)):
        raise _lib.BtxError("dropout with %d MC sample lanes of %r rows: the input has %d rows (expected the shared input of %r rows, "
                            "or %d lanes back to back)" % (lanes, lane_batch, rows, lane_batch, lanes))
    return int(lane_batch), rows == int(lane_batch)


def dropout_aten(x, T, scale, mode, seed, sample_idx, layer_id, sample_dev=None, lanes=1, lane_batch=None):
    """BTX-DROP v1 from torch ops (any device, any floating dtype): the masks of dropout_hip, bit for bit.  A device sample word is
    read on the host here (this route is not capturable)."""
    B, shared = _drop_lane_rows(x, lanes, lane_batch)
    if sample_dev is not None:
        idx = [int(v) for v in sample_dev.reshape(-1)[:max(1, lanes)].tolist()]
    else:
        idx = [int(sample_idx) + l for l in range(max(1, lanes))]
    if lanes <= 1:
        return dropout_apply_aten(x, dropout_mask_aten(tuple(x.shape), T, mode, seed, idx[0], layer_id, x.device), scale)
    outs = []
    for l in range(lanes):
        xl = x if shared else x[l * B:(l + 1) * B]
        outs.append(dropout_apply_aten(xl, dropout_mask_aten(tuple(xl.shape), T, mode, seed, idx[l], layer_id, x.device), scale))
    return torch.cat(outs, 0)


def _drop_layout(x, N, C, S):
    """(tensor to read, layout code): channels-last and plain contiguous memory run as they are; anything else is made contiguous"""
    if S == 1 or C == 1 or x.dim() < 3:
        return (x if x.is_contiguous() else x.contiguous()), _lib.DROP_CL
    if x.is_contiguous():
        return x, _lib.DROP_NCS
    nd = x.dim() - 2
    if x.permute((0,) + tuple(range(2, nd + 2)) + (1,)).is_contiguous():
        return x, _lib.DROP_CL
    return x.contiguous(), _lib.DROP_NCS


def dropout_hip(x, T, scale, mode, seed, sample_idx, layer_id, sample_dev=None, lanes=1, lane_batch=None, out=None, backward=False):
    """btx_dropout_fwd on a CUDA tensor (f32 / bf16): out = drop(x) under the mask of BTX-DROP v1 at (seed, sample index, layer id) —
    the backward is the same call on dy.  The mask belongs to the LOGICAL element: NCHW-contiguous and channels-last memory draw
    the same one, and the output keeps the input's memory format.  sample_dev: the device word(s) the kernel reads instead of
    sample_idx (captured steps; one int32 per lane).  lanes = L > 1 with lane_batch = B: x holds L tensors of B rows back to back,
    or the B shared rows every lane reads (broadcast: the output has L * B rows).  out: x itself for an in-place call.  backward=True:
    x is dy and the call is btx_dropout_bwd (one lane: lanes are an inference feature)."""
    L = _lib.lib()
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.BtxError("dropout_hip: f32 and bf16 activations only (got %s)" % x.dtype)
    lanes = max(1, int(lanes))
    B, shared = _drop_lane_rows(x, lanes, lane_batch)
    lane_shape = ((B,) + tuple(x.shape[1:])) if x.dim() else ()
    N, C, S = _drop_geom(lane_shape, mode)
    if N * C * S > _lib.DROP_MAX_ELEMENTS:
        raise _lib.BtxError("dropout: a lane tensor of more than 2^35 elements")
    xr, layout = _drop_layout(x, N, C, S)
    if shared and lanes > 1:
        oshape = (lanes * B,) + tuple(x.shape[1:])
        if layout == _lib.DROP_CL and x.dim() >= 3 and not (S == 1 or C == 1):
            nd = x.dim() - 2
            out = torch.empty((lanes * B,) + tuple(x.shape[2:]) + (x.shape[1],), dtype=x.dtype, device=x.device).permute(
                (0, nd + 1) + tuple(range(1, nd + 1)))
        else:
            out = torch.empty(oshape, dtype=x.dtype, device=x.device)
    elif out is None:
        out = torch.empty_like(xr)  # preserve_format: the memory order of xr (dense)
    if x.numel() == 0:
        return out
    r = _lib.Rng(int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_idx) & 0xFFFFFFFF, int(layer_id) & 0xFFFFFFFF,
                 sample_dev.data_ptr() if sample_dev is not None else None)
    act = _lib.ACT_BF16 if x.dtype == torch.bfloat16 else _lib.ACT_F32
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if backward:
        if lanes > 1:
            raise _lib.BtxError("MC sample lanes are an inference feature: clear them before a training step")
        _lib.check(L.btx_dropout_bwd(xr.data_ptr(), out.data_ptr(), act, N, C, S, DROP_MODES[mode], layout, int(T), float(scale),
                                     ctypes.byref(r), stream))
        return out
    _lib.check(L.btx_dropout_fwd(xr.data_ptr(), out.data_ptr(), act, N, C, S, DROP_MODES[mode], layout, int(T), float(scale),
                                 lanes, B if (shared and lanes > 1) else lanes * B, ctypes.byref(r), stream))
    return out
