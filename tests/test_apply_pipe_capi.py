"""The pipelined apply's C ABI (include/tqr.h "pipelined apply") without a GPU: every argument error
is reported before any device call, and the ticket order the kernel's deadlock freedom rests on
(tqr_apply_pipe_ticket evaluates the kernel's own mapping function on the host).

Every device-facing call here carries at least one invalid argument (the file also runs where a GPU
is present, so no made-up pointer ever travels with otherwise valid arguments). A pipelined handle
can be created without a device: it then holds no device memory, which is all these calls need. An
apply handle (tqr_apply) cannot, so what needs one is checked in tests/test_gpu_apply_pipe.py."""
import ctypes

import pytest

EINVAL = -1
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call fails validation

# (m, n, b, dtype, nrhs_max)
BAD_CREATE = {
    "bad dtype": (64, 64, 32, 2, 4),
    "b = 24": (96, 96, 24, F64, 4),
    "b = 512": (1024, 1024, 512, F64, 4),
    "b does not divide m": (100, 64, 32, F64, 4),
    "b does not divide n": (128, 100, 32, F64, 4),
    "m = 0": (0, 64, 32, F64, 4),
    "n < 0": (64, -64, 32, F64, 4),
    "nrhs_max = 0": (64, 64, 32, F64, 0),
    "m beyond the leading-dimension bound (fp64)": (8388608, 256, 256, F64, 4),
    "more work items than a grid holds": (4194304, 4194304, 16, F32, 2 ** 31 - 1),
}


@pytest.fixture(scope="module")
def handle(tqr):
    """A handle for m = 128, n = 64, b = 32, fp64, nrhs_max = 80 (with or without a device)."""
    h = P()
    assert tqr.lib().tqr_apply_pipe_create(ctypes.byref(h), 128, 64, 32, F64, 80) == 0
    assert h.value
    yield h
    tqr.lib().tqr_apply_pipe_destroy(h)


@pytest.fixture(scope="module")
def solve_handle(tqr):
    h = P()
    assert tqr.lib().tqr_solve_create(ctypes.byref(h), 64, 32, F64, 80) == 0
    yield h
    tqr.lib().tqr_solve_destroy(h)


@pytest.mark.parametrize("why", sorted(BAD_CREATE))
def test_create_invalid_args_without_gpu(tqr, why):
    h = P(12345)
    assert tqr.lib().tqr_apply_pipe_create(ctypes.byref(h), *BAD_CREATE[why]) == EINVAL, why
    assert h.value is None, "no handle is returned with an error"


def test_null_out_null_handle_and_null_ap(tqr, handle, solve_handle):
    """NULL out-pointer, NULL handle and NULL ap on every call, tqr_lstsq_pipe with any of its three
    handles NULL (the others are real where they can be made without a device; the apply handle, which
    cannot, is the one left NULL or stands in as a pointer that is never reached)."""
    L = tqr.lib()
    assert L.tqr_apply_pipe_create(None, 64, 64, 32, F64, 4) == EINVAL
    assert L.tqr_apply_pipe_workspace_bytes(None) == 0
    assert L.tqr_apply_pipe_status(None, None) == EINVAL
    assert L.tqr_apply_pipe_q(None, None, 1, Z, 128, Z, 4, 128, None) == EINVAL
    assert L.tqr_apply_pipe_q(None, Z, 1, Z, 128, Z, 4, 128, None) == EINVAL
    for trans in (0, 1):
        assert L.tqr_apply_pipe_q(handle, None, trans, Z, 128, Z, 4, 128, None) == EINVAL
        assert L.tqr_lstsq_pipe(handle, solve_handle, None, trans, Z, 128, Z, 4, 128, None, None) == EINVAL
        assert L.tqr_lstsq_pipe(None, solve_handle, Z, trans, Z, 128, Z, 4, 128, None, None) == EINVAL
        assert L.tqr_lstsq_pipe(handle, None, Z, trans, Z, 128, Z, 4, 128, None, None) == EINVAL
        assert L.tqr_lstsq_pipe(None, None, None, trans, Z, 128, Z, 4, 128, None, None) == EINVAL
    L.tqr_apply_pipe_destroy(None)  # a no-op


def test_workspace_bytes(tqr, handle):
    """(m, n, b, nrhs_max) = (128, 64, 32, 80): p = 4, kmax = 2, the stored tiles (l, k), l >= k, are
    4 + 3 = 7, nrhs_max = 80 is 2 strips: the 128-B header and a 4-byte flag per (strip, tile)."""
    assert tqr.lib().tqr_apply_pipe_workspace_bytes(handle) == 128 + 4 * 2 * 7


def test_status_of_an_unused_handle(tqr):
    """Nothing was ever enqueued: TQR_OK (a fresh handle; with a device it synchronises an idle stream)."""
    L = tqr.lib()
    h = P()
    assert L.tqr_apply_pipe_create(ctypes.byref(h), 64, 128, 64, F32, 1) == 0
    try:
        assert L.tqr_apply_pipe_workspace_bytes(h) == 128 + 4  # p = 1, kmax = 1: one tile, one strip
        assert L.tqr_apply_pipe_status(h, None) == 0
    finally:
        L.tqr_apply_pipe_destroy(h)


def test_python_wrapper_rejects_without_gpu(tqr):
    """tqr.ApplyPipe raises TQRError for a tile size that does not divide m; a good one reports its
    workspace."""
    import numpy as np
    with pytest.raises(tqr.TQRError):
        tqr.ApplyPipe(100, 64, 32, np.float64, 4)
    with pytest.raises(tqr.TQRError):
        tqr.ApplyPipe(128, 64, 32, np.float64, 0)
    pp = tqr.ApplyPipe(128, 64, 32, np.float64, 80)
    assert pp.workspace_bytes() == 128 + 4 * 2 * 7


# ---- the ticket order ---------------------------------------------------------------------------
def ticket(L, kmax, ns, trans, t):
    s, k = ctypes.c_int(-7), ctypes.c_int(-7)
    st = L.tqr_apply_pipe_ticket(kmax, ns, trans, t, ctypes.byref(s), ctypes.byref(k))
    return st, s.value, k.value


@pytest.mark.parametrize("trans", [0, 1], ids=["Q", "Qt"])
def test_ticket_order(tqr, trans):
    """kmax in 1..9, nstrips in 1..5: the tickets are a bijection onto (strip, step), the producer of a
    step (Q^T: step - 1, Q: step + 1, same strip) has a smaller ticket, and out-of-range tickets are
    refused and write nothing."""
    L = tqr.lib()
    for kmax in range(1, 10):
        for ns in range(1, 6):
            of = {}
            for t in range(kmax * ns):
                st, s, k = ticket(L, kmax, ns, trans, t)
                assert st == 0 and 0 <= s < ns and 0 <= k < kmax, (kmax, ns, t, st, s, k)
                assert (s, k) not in of, (kmax, ns, t)
                of[(s, k)] = t
                assert tqr.apply_pipe_ticket(kmax, ns, bool(trans), t) == (s, k)
            assert len(of) == kmax * ns
            for (s, k), t in of.items():
                producer = k - 1 if trans else k + 1
                if 0 <= producer < kmax:
                    assert of[(s, producer)] < t, (kmax, ns, s, k)
                else:
                    assert t < ns, "a step without a producer is among the first tickets"
            for t in (-1, kmax * ns, kmax * ns + 1, 2 ** 31 - 1):
                assert ticket(L, kmax, ns, trans, t) == (EINVAL, -7, -7), (kmax, ns, t)


def test_ticket_invalid_args(tqr):
    L = tqr.lib()
    s, k = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.tqr_apply_pipe_ticket(0, 1, 0, 0, ctypes.byref(s), ctypes.byref(k)) == EINVAL
    assert L.tqr_apply_pipe_ticket(1, 0, 0, 0, ctypes.byref(s), ctypes.byref(k)) == EINVAL
    assert L.tqr_apply_pipe_ticket(2, 2, 2, 0, ctypes.byref(s), ctypes.byref(k)) == EINVAL
    assert L.tqr_apply_pipe_ticket(2, 2, -1, 0, ctypes.byref(s), ctypes.byref(k)) == EINVAL
    assert L.tqr_apply_pipe_ticket(2, 2, 0, 0, None, ctypes.byref(k)) == EINVAL
    assert L.tqr_apply_pipe_ticket(2, 2, 0, 0, ctypes.byref(s), None) == EINVAL
    assert (s.value, k.value) == (-7, -7), "a refused call writes nothing"
    with pytest.raises(tqr.TQRError):
        tqr.apply_pipe_ticket(2, 2, True, 4)
    # a product that overflows int is still judged in 64 bits
    big = 2 ** 31 - 1
    for trans in (0, 1):
        assert L.tqr_apply_pipe_ticket(2 ** 20, 2 ** 20, trans, big, ctypes.byref(s), ctypes.byref(k)) == 0
        pos = big // 2 ** 20
        assert (s.value, k.value) == (big % 2 ** 20, pos if trans else 2 ** 20 - 1 - pos)
