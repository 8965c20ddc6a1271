"""The solve's C ABI (include/tqr.h "solve") without a GPU: every argument error is reported before
any device call. Every call here carries at least one invalid argument (the file also runs where a
GPU is present, so no made-up pointer ever travels with otherwise valid arguments)."""
import ctypes

import pytest

EINVAL = -1
F32, F64 = 0, 1
Z = ctypes.c_void_p(1)  # a non-NULL pointer that is never dereferenced: each call fails validation

# (dtype, trans, n, b, dA, ldda, dX, nrhs, lddx)
BAD_TRSM = {
    "bad dtype": (2, 0, 64, 32, Z, 64, Z, 4, 64),
    "trans = 2": (F64, 2, 64, 32, Z, 64, Z, 4, 64),
    "b = 24": (F64, 0, 96, 24, Z, 96, Z, 4, 96),
    "b does not divide n": (F64, 0, 100, 32, Z, 100, Z, 4, 100),
    "n = 0": (F64, 0, 0, 32, Z, 64, Z, 4, 64),
    "nrhs = 0": (F64, 0, 64, 32, Z, 64, Z, 0, 64),
    "ldda < n": (F64, 0, 64, 32, Z, 63, Z, 4, 64),
    "lddx < n": (F64, 0, 64, 32, Z, 64, Z, 4, 63),
    "lddx beyond the bound (fp64)": (F64, 0, 64, 32, Z, 64, Z, 4, 8388608),
    "NULL dA": (F64, 0, 64, 32, None, 64, Z, 4, 64),
    "NULL dX": (F64, 0, 64, 32, Z, 64, None, 4, 64),
}


@pytest.mark.parametrize("why", sorted(BAD_TRSM))
def test_trsm_r_invalid_args_without_gpu(tqr, why):
    assert tqr.lib().tqr_trsm_r(*BAD_TRSM[why], None) == EINVAL, why


def test_trsm_r_both_directions_and_dtypes_validate(tqr):
    """The same checks hold for TRANS and for fp32 (whose bound is twice as far)."""
    L = tqr.lib()
    assert L.tqr_trsm_r(F32, 1, 100, 32, Z, 100, Z, 4, 100, None) == EINVAL
    assert L.tqr_trsm_r(F64, 1, 64, 32, Z, 64, Z, 4, 63, None) == EINVAL
    assert L.tqr_trsm_r(F32, 0, 64, 32, Z, 16777216, Z, 4, 64, None) == EINVAL
    assert L.tqr_trsm_r(F64, 0, 64, 32, Z, 8388608, Z, 4, 64, None) == EINVAL


def test_lstsq_null_handle_without_gpu(tqr):
    L = tqr.lib()
    assert L.tqr_lstsq(None, 0, Z, 64, Z, 1, 64, None, None) == EINVAL
    assert L.tqr_lstsq(None, 1, Z, 64, Z, 1, 64, None, None) == EINVAL


def test_python_wrapper_rejects_without_gpu(tqr):
    """tqr.trsm_r raises TQRError for a tile size that does not divide n (host arrays stand in for
    device tensors: the call fails validation before anything is read)."""
    import numpy as np
    F = np.zeros((100, 100))
    X = np.zeros((4, 100))
    with pytest.raises(tqr.TQRError):
        tqr.trsm_r(F, X, 32)
    with pytest.raises(tqr.TQRError):
        tqr.trsm_r(F, X.astype(np.float32), 25)
