"""The pipelined solve's C ABI (include/tqr.h "pipelined solve") without a GPU: every argument error
is reported before any device call, and the ticket order the kernel's deadlock freedom rests on
(tqr_solve_ticket evaluates the kernel's own mapping function on the host).

Every device-facing call here carries at least one invalid argument (the file also runs where a GPU
is present, so no made-up pointer ever travels with otherwise valid arguments). A handle can be
created without a device: it then holds no device memory, which is all these calls need."""
import ctypes

import pytest

EINVAL = -1
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call fails validation

# (n, b, dtype, nrhs_max)
BAD_CREATE = {
    "bad dtype": (64, 32, 2, 4),
    "b = 24": (96, 24, F64, 4),
    "b = 512": (1024, 512, F64, 4),
    "b does not divide n": (100, 32, F64, 4),
    "n = 0": (0, 32, F64, 4),
    "n < 0": (-64, 32, F64, 4),
    "nrhs_max = 0": (64, 32, F64, 0),
    "nrhs_max < 0": (64, 32, F32, -3),
    "n beyond the leading-dimension bound (fp64)": (8388608, 256, F64, 4),
    "more work items than a grid holds": (4194304, 16, F32, 2 ** 31 - 1),
}


@pytest.fixture(scope="module")
def handle(tqr):
    """A handle for n = 64, b = 32, fp64, nrhs_max = 80 (with or without a device)."""
    h = P()
    assert tqr.lib().tqr_solve_create(ctypes.byref(h), 64, 32, F64, 80) == 0
    assert h.value
    yield h
    tqr.lib().tqr_solve_destroy(h)


@pytest.mark.parametrize("why", sorted(BAD_CREATE))
def test_create_invalid_args_without_gpu(tqr, why):
    h = P(12345)
    assert tqr.lib().tqr_solve_create(ctypes.byref(h), *BAD_CREATE[why]) == EINVAL, why
    assert h.value is None, "no handle is returned with an error"


def test_create_null_out_and_null_handle_calls(tqr):
    L = tqr.lib()
    assert L.tqr_solve_create(None, 64, 32, F64, 4) == EINVAL
    assert L.tqr_solve_workspace_bytes(None) == 0
    assert L.tqr_solve_status(None, None) == EINVAL
    assert L.tqr_solve_trsm_r(None, 0, Z, 64, Z, 4, 64, None) == EINVAL
    L.tqr_solve_destroy(None)  # a no-op


def test_workspace_bytes(tqr, handle):
    """The ticket, the error word (one 128-B line with its padding) and a 4-byte flag per (strip, tile
    row): nrhs_max = 80 is 2 strips, n / b = 2 tile rows."""
    assert tqr.lib().tqr_solve_workspace_bytes(handle) == 128 + 4 * 2 * 2


# (trans, dA, ldda, dX, nrhs, lddx) on the handle above
BAD_TRSM = {
    "trans = 2": (2, Z, 64, Z, 4, 64),
    "trans = -1": (-1, Z, 64, Z, 4, 64),
    "NULL dA": (0, None, 64, Z, 4, 64),
    "NULL dX": (1, Z, 64, None, 4, 64),
    "nrhs = 0": (0, Z, 64, Z, 0, 64),
    "nrhs < 0": (0, Z, 64, Z, -1, 64),
    "nrhs > nrhs_max": (0, Z, 64, Z, 81, 64),
    "ldda < n": (0, Z, 63, Z, 4, 64),
    "lddx < n": (1, Z, 64, Z, 4, 63),
    "ldda beyond the bound (fp64)": (0, Z, 8388608, Z, 4, 64),
    "lddx beyond the bound (fp64)": (0, Z, 64, Z, 4, 8388608),
}


@pytest.mark.parametrize("why", sorted(BAD_TRSM))
def test_trsm_r_invalid_args_without_gpu(tqr, handle, why):
    assert tqr.lib().tqr_solve_trsm_r(handle, *BAD_TRSM[why], None) == EINVAL, why


def test_fp32_handle_has_the_fp32_bound(tqr):
    L = tqr.lib()
    h = P()
    assert L.tqr_solve_create(ctypes.byref(h), 64, 16, F32, 1) == 0
    try:
        assert L.tqr_solve_trsm_r(h, 0, Z, 16777216, Z, 1, 64, None) == EINVAL
        assert L.tqr_solve_trsm_r(h, 1, Z, 64, Z, 1, 16777216, None) == EINVAL
        assert L.tqr_solve_trsm_r(h, 1, Z, 64, Z, 2, 64, None) == EINVAL  # nrhs_max = 1
    finally:
        L.tqr_solve_destroy(h)


def test_lstsq_fused_solve_null_arguments(tqr, handle):
    """A NULL plan, handle or array is refused before anything is read (a plan itself needs a device:
    the mismatch between a plan and a handle is checked in tests/test_gpu_solve_pipe.py)."""
    L = tqr.lib()
    assert L.tqr_lstsq_fused_solve(None, handle, Z, 64, Z, 1, None, None) == EINVAL
    assert L.tqr_lstsq_fused_solve(None, None, Z, 64, Z, 1, None, None) == EINVAL
    assert L.tqr_lstsq_fused_solve(None, handle, None, 64, Z, 1, None, None) == EINVAL


def test_python_wrapper_rejects_without_gpu(tqr):
    """tqr.Solve raises TQRError for a tile size that does not divide n, and tqr.trsm_r refuses a
    handle made for another shape (host arrays stand in for device tensors: nothing is read)."""
    import numpy as np
    with pytest.raises(tqr.TQRError):
        tqr.Solve(100, 32, np.float64, 4)
    sv = tqr.Solve(64, 32, np.float64, 4)
    assert sv.workspace_bytes() == 128 + 4 * 2
    F = np.zeros((96, 96))
    X = np.zeros((4, 96))
    with pytest.raises(tqr.TQRError):
        tqr.trsm_r(F, X, 32, solve=sv)  # n = 96
    with pytest.raises(tqr.TQRError):
        sv.trsm_r(F[:64, :64].astype(np.float32), X[:, :64].astype(np.float32))  # dtype
    with pytest.raises(tqr.TQRError):
        sv.trsm_r(np.zeros((64, 64)), np.zeros((5, 64)))  # nrhs > nrhs_max


# ---- the ticket order ---------------------------------------------------------------------------
def ticket(L, T, ns, trans, t):
    s, r = ctypes.c_int(-7), ctypes.c_int(-7)
    st = L.tqr_solve_ticket(T, ns, trans, t, ctypes.byref(s), ctypes.byref(r))
    return st, s.value, r.value


@pytest.mark.parametrize("trans", [0, 1], ids=["R", "Rt"])
def test_ticket_order(tqr, trans):
    """T in 1..9, nstrips in 1..5: the tickets are a bijection onto (strip, row), every producer of a
    row (NOTRANS: the rows below it, TRANS: the rows above it, same strip) has a smaller ticket, and
    out-of-range tickets are refused and write nothing."""
    L = tqr.lib()
    for T in range(1, 10):
        for ns in range(1, 6):
            of = {}
            for t in range(T * ns):
                st, s, r = ticket(L, T, ns, trans, t)
                assert st == 0 and 0 <= s < ns and 0 <= r < T, (T, ns, t, st, s, r)
                assert (s, r) not in of, (T, ns, t)
                of[(s, r)] = t
            assert len(of) == T * ns
            for (s, r), t in of.items():
                producers = range(r) if trans else range(r + 1, T)
                for k in producers:
                    assert of[(s, k)] < t, (T, ns, s, r, k)
            for t in (-1, T * ns, T * ns + 1, 2 ** 31 - 1):
                assert ticket(L, T, ns, trans, t) == (EINVAL, -7, -7), (T, ns, t)


def test_ticket_invalid_args(tqr):
    L = tqr.lib()
    s, r = ctypes.c_int(), ctypes.c_int()
    assert L.tqr_solve_ticket(0, 1, 0, 0, ctypes.byref(s), ctypes.byref(r)) == EINVAL
    assert L.tqr_solve_ticket(1, 0, 0, 0, ctypes.byref(s), ctypes.byref(r)) == EINVAL
    assert L.tqr_solve_ticket(2, 2, 2, 0, ctypes.byref(s), ctypes.byref(r)) == EINVAL
    assert L.tqr_solve_ticket(2, 2, 0, 0, None, ctypes.byref(r)) == EINVAL
    assert L.tqr_solve_ticket(2, 2, 0, 0, ctypes.byref(s), None) == EINVAL
    # a product that overflows int is still judged in 64 bits
    assert L.tqr_solve_ticket(2 ** 20, 2 ** 20, 0, 2 ** 31 - 1, ctypes.byref(s), ctypes.byref(r)) == 0
    assert (s.value, r.value) == ((2 ** 31 - 1) % 2 ** 20, 2 ** 20 - 1 - (2 ** 31 - 1) // 2 ** 20)


@pytest.mark.parametrize("n, ns, trans, t", [(1, 1, 0, 0), (4, 1, 0, 3), (4, 3, 1, 7), (9, 5, 0, 44), (9, 5, 1, 0),
                                             (2 ** 20, 2 ** 20, 0, 2 ** 31 - 1), (2 ** 20, 2 ** 20, 1, 2 ** 31 - 1)])
def test_ticket_map_shared_with_the_pipelined_apply(tqr, n, ns, trans, t):
    """tqr_solve_ticket and tqr_apply_pipe_ticket evaluate one map: the same (strip, position)."""
    L = tqr.lib()
    s, k = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.tqr_apply_pipe_ticket(n, ns, trans, t, ctypes.byref(s), ctypes.byref(k)) == 0
    assert ticket(L, n, ns, trans, t) == (0, s.value, k.value)
    assert (s.value, k.value) == (t % ns, t // ns if trans else n - 1 - t // ns)
