"""The apply's C ABI (include/tqr.h "apply") without a GPU: every argument error is reported
before any device call."""
import ctypes

EINVAL = -1


def test_apply_create_invalid_args_without_gpu(tqr):
    L = tqr.lib()
    h = ctypes.c_void_p()
    assert L.tqr_apply_create(ctypes.byref(h), 100, 64, 32, 1) == EINVAL  # b does not divide m
    assert L.tqr_apply_create(ctypes.byref(h), 64, 100, 32, 1) == EINVAL  # b does not divide n
    assert L.tqr_apply_create(ctypes.byref(h), 96, 96, 24, 1) == EINVAL   # unsupported tile size
    assert L.tqr_apply_create(ctypes.byref(h), 64, 64, 32, 2) == EINVAL   # bad dtype
    assert L.tqr_apply_create(ctypes.byref(h), 0, 64, 32, 1) == EINVAL
    assert L.tqr_apply_create(None, 64, 64, 32, 1) == EINVAL
    assert not h.value  # no handle came back from any of them


def test_apply_create_leading_dimension_bound_without_gpu(tqr):
    """The library's bound 32 * ldm * sizeof(element) < 2^31 holds for the apply as for a plan."""
    L = tqr.lib()
    h = ctypes.c_void_p()
    m = 8388608 + 256  # too tall for fp64
    assert L.tqr_apply_create(ctypes.byref(h), m, 256, 256, 1) == EINVAL
    # a valid request passes validation and only then needs a device (-4 here without one)
    st = L.tqr_apply_create(ctypes.byref(h), 64, 64, 32, 1)
    assert st in (-4, 0)
    if st == 0:
        assert L.tqr_apply_workspace_bytes(h) > 0
        L.tqr_apply_destroy(h)


def test_apply_null_handle_without_gpu(tqr):
    L = tqr.lib()
    z = ctypes.c_void_p(1)
    assert L.tqr_apply_q(None, 1, z, 64, z, 1, 64, None) == EINVAL
    assert L.tqr_apply_prepare(None, z, 64, z, None) == EINVAL
    assert L.tqr_apply_workspace_bytes(None) == 0
    L.tqr_apply_destroy(None)  # a no-op


def test_python_wrappers_reject_without_gpu(tqr):
    """ApplyQ raises TQRError for a bad shape; compact_tau inverts expand_tau (host only)."""
    import numpy as np
    import pytest
    with pytest.raises(tqr.TQRError):
        tqr.ApplyQ(100, 64, 32, np.float64)
    m, n, b = 96, 64, 32
    tc = np.arange(2 * m, dtype=np.float64).reshape(2, m) + 1.0
    for k in range(2):
        tc[k, :k * b] = 0.0
    assert np.array_equal(tqr.compact_tau(tqr.expand_tau(tc, m, n, b), m, n, b), tc)
