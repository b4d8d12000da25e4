"""The host-side alignment guards that refuse (DESIGN.md "Alignment contract"): every call below returns BTX_E_ALIGN before
anything is launched, so no GPU is needed (the pointers are never dereferenced, as in tests/test_cabi.py).  The fallbacks —
entry points that pick another kernel for an off-grid pointer — need a GPU: tests/test_gpu_alignment.py."""
import ctypes

E_ALIGN = -6


def _p(v):
    return ctypes.c_void_p(v)


def test_entry_points_that_refuse_off_grid_pointers():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert b"aligned" in L.btx_strerror(E_ALIGN)
    on, off4, off8 = _p(4096), _p(4096 + 4), _p(4096 + 8)
    # btx_rowfuse_pack stores one padded pixel (8 / 16 / 32 bytes) per thread: `out` on the grid; x is read element by element
    st = (ctypes.c_int64 * 4)(192, 64, 8, 1)
    for out in (off4, off8):
        assert L.btx_rowfuse_pack(on, 1, st, 1, 3, 8, 8, out, 1, 8, 8, 4, 0, 0, None) == E_ALIGN
    # the pools: 8 channels per 16-byte access on both tensors, the window positions in 8-byte words
    assert L.btx_maxpool2d_cl(on, off8, 1, 1, 8, 8, 16, 3, 2, 1, None) == E_ALIGN
    assert L.btx_maxpool2d_cl_train(off4, on, on, 0, 1, 8, 8, 16, 3, 2, 1, None) == E_ALIGN
    assert L.btx_maxpool2d_cl_train(on, on, off4, 0, 1, 8, 8, 16, 3, 2, 1, None) == E_ALIGN
    assert L.btx_maxpool2d_cl_bwd(on, on, off8, 0, 1, 8, 8, 16, 3, 2, 1, None) == E_ALIGN
    assert L.btx_avgpool_global_cl(off4, on, 0, 1, 49, 16, None) == E_ALIGN
    # the calibration losses keep their thresholds as doubles in the workspace header
    need = L.btx_calib_workspace_bytes(8)
    assert L.btx_avu_fwd(on, on, 8, 10, 0, 0, 0.5, None, 1.0, on, off4, need, None) == E_ALIGN
    assert L.btx_avu_bwd(on, 8, 10, 0, on, None, off4, need, on, None) == E_ALIGN
    assert L.btx_eau_fwd(on, on, 8, 0, 0.5, None, 0.5, None, 1.0, on, off4, need, None) == E_ALIGN
    assert L.btx_eau_bwd(on, on, 8, 0, on, off4, need, on, on, None) == E_ALIGN
    # the KL workspace holds double partial sums
    assert L.btx_kl_gauss(on, on, 10, None, None, 0.0, 1.0, on, 0, off4, L.btx_kl_workspace_bytes(10), None) == E_ALIGN


def test_on_grid_is_the_identity_for_aligned_tensors_and_copies_the_others():
    """functional.on_grid on CPU tensors: the tensor itself when it lies on the 16-byte grid, else one copy with the same values,
    shape and strides in fresh storage"""
    import torch
    from bayesian_torch_amd import functional as BF
    assert BF.on_grid(None) is None
    base = torch.arange(4 * 8 * 3 * 5 + 64, dtype=torch.float32)
    start = (-base.data_ptr() % 16) // 4          # first element on the grid
    shape, strides = (4, 8, 3, 5), (120, 1, 40, 8)  # channels-last strides of [4, 8, 3, 5]
    a = base.as_strided(shape, strides, start)
    assert a.data_ptr() % 16 == 0 and BF.on_grid(a) is a
    for k in (1, 2, 3):
        v = base.as_strided(shape, strides, start + k)
        assert v.data_ptr() % 16 == 4 * k
        c = BF.on_grid(v)
        assert c is not v and c.data_ptr() % 16 == 0 and c.stride() == v.stride() and torch.equal(c, v)
        assert c.is_contiguous(memory_format=torch.channels_last)
