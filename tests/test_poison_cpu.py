"""tests/poison.py without a GPU: the helper catches a skipped element and a workspace read before it is written, under both
patterns, restores what it replaced, and the tables of tests/test_gpu_poison.py classify every export of libbtx.so exactly once."""
import pytest
import torch

import poison as P


def _skips_one(n=1000):
    out = torch.empty(n)
    out[:n - 1] = torch.arange(n - 1, dtype=torch.float32)
    return out


def _sums_a_workspace_before_writing_it():
    from bayesian_torch_amd import functional as BF
    ws = BF._workspace(torch.device("cpu"), 4096, 0)
    acc = ws[:4096].view(torch.float32).sum().reshape(1)   # a reduce pass over partials nobody wrote
    ws[:4096].view(torch.float32).fill_(1.0)
    return acc


def _writes_everything(n=1000):
    from bayesian_torch_amd import functional as BF
    out = torch.empty_strided((4, n), (1, 4))
    ws = BF._workspace(torch.device("cpu"), 4 * n, 0)[:4 * n].view(torch.float32)
    ws.copy_(torch.arange(n, dtype=torch.float32))
    out.copy_(ws.expand(4, n) * 2)
    like = torch.empty_like(out)
    like.copy_(out + 1)
    new = out.new_empty((3,))
    new.zero_()
    return out, like, new, ws.sum().reshape(1)


@pytest.fixture
def cpu_workspace():
    from bayesian_torch_amd import functional as BF
    keys = set(BF._WS)
    BF._workspace(torch.device("cpu"), 8192, 0).zero_()   # what an earlier, correct call left there
    yield
    for k in set(BF._WS) - keys:
        del BF._WS[k]


def _three_ways(fn):
    clean = fn()
    got = []
    for byte in P.PATTERNS:
        with P.poisoned(byte, devices=("cpu",)) as rec:
            got.append((fn(), rec))
    return clean, got


def test_helper_catches_a_skipped_element_and_a_stale_workspace_and_passes_full_writes(cpu_workspace):
    # caught: the last element is whatever the buffer held
    clean, got = _three_ways(_skips_one)
    for (out, rec), byte in zip(got, P.PATTERNS):
        assert rec.tensors == 1 and rec.bytes == 4000
        assert P.bits_equal(out[:-1], clean[:-1])
        assert out[-1:].view(torch.int32).item() == int.from_bytes(bytes([byte] * 4), "little", signed=True)
    assert not P.bits_equal(got[0][0], got[1][0])
    assert torch.isnan(got[0][0][-1]) and got[1][0][-1] > 3e38
    # caught: the workspace is refilled on EVERY call, not only when it grows (it exists since the fixture, and held zeros)
    clean, got = _three_ways(_sums_a_workspace_before_writing_it)
    assert float(clean) in (0.0, 1024.0)
    for (acc, rec), byte in zip(got, P.PATTERNS):
        assert rec.tensors == 1 and rec.bytes >= 4096
        assert not P.bits_equal(acc, clean), "a workspace read before it was written went unnoticed under %#04x" % byte
    assert torch.isnan(got[0][0]).all() and (torch.isinf(got[1][0]) | (got[1][0] > 1e38)).all()
    # clean: every factory is replaced (empty_strided, empty_like, new_empty, the workspace) and full writes give equal bits
    clean, got = _three_ways(_writes_everything)
    for (out, rec), byte in zip(got, P.PATTERNS):
        assert P.bits_equal(out, clean), byte
        assert rec.tensors == 4 and rec.bytes > 2 * 16000
        assert not P.any_nan(out)
    assert clean[0].stride() == (1, 4)


def test_dense_non_contiguous_layouts_are_poisoned_through_the_storage():
    with P.poisoned(0xFF, devices=("cpu",)) as rec:
        t = torch.empty((2, 8, 3, 3), memory_format=torch.channels_last)
        i = torch.empty(5, dtype=torch.int64)
        b = torch.empty(6, dtype=torch.bfloat16)
        d = torch.empty(2, dtype=torch.float64)
        u = torch.empty(3, dtype=torch.uint8)
    assert torch.isnan(t).all() and torch.isnan(b).all() and torch.isnan(d).all() and (i == -1).all() and (u == 255).all()
    assert rec.tensors == 5 and rec.bytes == 2 * 8 * 9 * 4 + 40 + 12 + 16 + 3
    with P.poisoned(0x7F, devices=("cpu",)):
        f = torch.empty(4)
        b = torch.empty(4, dtype=torch.bfloat16)
        d = torch.empty(2, dtype=torch.float64)
        s = torch.empty(3, dtype=torch.int8)
    assert (f > 3.3e38).all() and torch.isfinite(f).all() and (b.float() > 3.3e38).all() and torch.isfinite(b).all()
    assert torch.isfinite(d).all() and (d > 1e300).all() and (s == 127).all()
    with P.poisoned(0xFF, devices=("cuda",)) as rec:   # another device type: left alone
        torch.empty(4)
    assert rec.tensors == 0 and rec.bytes == 0


def test_state_is_restored_also_after_an_exception():
    from bayesian_torch_amd import functional as BF
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, BF._workspace)
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned(0xFF, devices=("cpu",)):
            assert torch.empty is not before[0] and BF._workspace is not before[4]
            raise RuntimeError("boom")
    after = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty, BF._workspace)
    assert all(a is b for a, b in zip(after, before))
    with P.poisoned(0x7F, devices=("cpu",)):
        pass
    assert torch.empty is before[0] and BF._workspace is before[4]
    with pytest.raises(ValueError):
        with P.poisoned(256):
            pass
    assert torch.empty is before[0]


def test_entry_points_are_recorded_and_the_library_object_is_restored():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    orig = L.btx_abi_version
    with P.poisoned(0xFF, devices=("cpu",)) as rec:
        assert L.btx_abi_version() == _lib.ABI_VERSION
        assert L.btx_strerror(-4)
        assert L.btx_kl_workspace_bytes(1000) > 0
    assert rec.calls == ["btx_abi_version", "btx_strerror", "btx_kl_workspace_bytes"] and rec.called("btx_strerror")
    assert L.btx_abi_version is orig and L.btx_abi_version() == _lib.ABI_VERSION


def test_bits_equal():
    nan = torch.tensor([float("nan"), 1.0])
    assert P.bits_equal(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not P.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not P.bits_equal(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert not P.bits_equal(torch.zeros(2), torch.zeros(1, 2))
    a = torch.arange(24.0).reshape(2, 3, 4)
    assert P.bits_equal(a.permute(2, 0, 1), a.permute(2, 0, 1).contiguous())
    assert P.bits_equal((a, [a.bfloat16(), None], dict(k=a.long())), (a.clone(), [a.bfloat16(), None], dict(k=a.long())))
    assert not P.bits_equal((a, None), (a,)) and not P.bits_equal((a, a), (a, a + 1))
    assert P.any_nan((a, [nan])) and not P.any_nan((a, a.long()))
    with pytest.raises(TypeError):
        P.bits_equal(1.0, 1.0)


def test_every_export_is_classified_exactly_once():
    """a new export fails here until tests/test_gpu_poison.py names the test that covers it, or the reason it needs none"""
    from bayesian_torch_amd import _lib
    import test_gpu_poison as T
    covered, host, prior = set(T.COVERED), set(T.HOST_ONLY), set(T.READS_PRIOR_CONTENTS)
    assert len(T.HOST_ONLY) == len(host)
    assert not (covered & host) and not (covered & prior) and not (host & prior)
    exports = set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(exports)
    assert exports - (covered | host | prior) == set(), "unclassified exports"
    assert (covered | host | prior) - exports == set(), "classified names that are not exported"
    # the tests the tables name exist, are GPU tests, and each names at least one entry; every reason cites the header
    names = set(T.COVERED.values()) | {t for _, t in T.READS_PRIOR_CONTENTS.values()}
    for name in names:
        assert callable(getattr(T, name, None)) and name.startswith("test_"), name
        assert T.entries_of(name)
    assert any(m.name == "gpu" for m in (T.pytestmark if isinstance(T.pytestmark, list) else [T.pytestmark]))
    for entry, (reason, _) in T.READS_PRIOR_CONTENTS.items():
        assert reason.startswith("btx.h") and len(reason.splitlines()) == 1, entry
    # HOST_ONLY is what the issue lists: the size queries and five more
    sized = {e for e in exports if e.endswith(("_bytes", "_bytes_lanes", "_doubles", "_floats"))}
    assert host == sized | {"btx_contract_plan_info", "btx_contract_pool_shape", "btx_out_shape", "btx_abi_version", "btx_strerror"}
    L = _lib.lib()
    assert all(hasattr(L, e) for e in exports)
