"""btx_bias_grad (csrc/btx_biasgrad.hip): the host-side argument checks, which return before anything is launched — no GPU needed."""
import ctypes


def test_cabi_bias_grad_entry_points_without_gpu():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    assert L.btx_abi_version() == 9  # additive: the ABI number does not move
    for n in ("btx_bias_grad_workspace_bytes", "btx_bias_grad"):
        assert n in _lib.EXPORTS and hasattr(ctypes.CDLL(_lib.lib_path()), n)
    W = L.btx_bias_grad_workspace_bytes
    assert W(0, 64) > 0 and W(1024, 64) == W(1, 64) and W(1025, 64) == 2 * 2 * 64 * 4 and W(10 ** 9, 64) == 2 * 128 * 64 * 4
    one, big = ctypes.c_void_p(256), W(10 ** 6, 64)
    r = _lib.Rng(1, 2, 3, None)
    f = L.btx_bias_grad
    rep, flip = _lib.KIND_REPARAM, _lib.KIND_FLIPOUT
    assert f(rep, None, 4096, 64, 0, one, None, None, None, 0, one, big, None) == -1
    assert f(rep, one, 4096, 64, 0, None, None, None, None, 0, one, big, None) == -1
    assert f(flip, one, 4096, 64, 0, one, None, ctypes.byref(r), None, 0, one, big, None) == -1     # Flipout needs db_delta ...
    assert f(flip, one, 4096, 64, 0, one, one, None, None, 0, one, big, None) == -1                  # ... and signs from somewhere
    assert f(rep, one, 4096, 64, 0, one, None, None, None, 0, None, 0, None) == -1                   # several parts need ws
    assert f(7, one, 4096, 64, 0, one, None, None, None, 0, one, big, None) == -3
    assert f(rep, one, 0, 64, 0, one, None, None, None, 0, one, big, None) == -2
    assert f(rep, one, 4096, 0, 0, one, None, None, None, 0, one, big, None) == -2
    assert f(rep, one, 4096, 64, 9, one, None, None, None, 0, one, big, None) == -5
    assert f(rep, one, 4096, 64, 0, one, None, None, None, 0, one, 16, None) == -4
    assert f(rep, one, 4096, 64, 0, one, None, None, None, 0, ctypes.c_void_p(258), big, None) == -6
