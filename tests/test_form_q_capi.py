"""Form Q through the C ABI (include/tqr.h "pipelined apply": tqr_apply_pipe_form_q and its two host
functions) without a GPU: the work items and the ticket order the kernel's deadlock freedom rests on
(tqr_apply_pipe_form_q_ticket evaluates the kernel's own mapping function on the host), and the
argument errors, each reported before any device call.

As in tests/test_apply_pipe_capi.py every device-facing call carries exactly one invalid argument,
everything else being valid: the file also runs where a GPU is present. The pipelined handle is real
(it can be made without a device). An apply handle (tqr_apply) cannot be made without a device, so
the ap of these calls is a pointer that validation never reaches — ap is looked at last — or NULL,
which is itself the error. What needs a real ap — an ap of another shape, an unprepared ap, and each
refusal once more against a prepared one — is in tests/test_gpu_form_q.py. TQR_ENODEV for a valid
call on a handle without a device would need a prepared ap on a machine without a device, which
cannot exist: that path (pipe_ready, shared with tqr_apply_pipe_q) is read in the code."""
import ctypes

import pytest

EINVAL = -1
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call fails validation before
BS = [16, 32, 64, 128, 256]
KMAXS = [1, 2, 3, 5]


def ncols_of(kmax, b):
    return sorted({c for c in (1, b - 1, b, b + 1, 63, 64, 65, kmax * b, kmax * b + 70) if c > 0})


def items_expected(kmax, b, ncols):
    """{(strip, step)}: step k exists if k b <= ncols - 1 and has the strips floor(k b / 64) .. nstrips - 1."""
    nstrips = -(-ncols // 64)
    return {(s, k) for k in range(kmax) if k * b <= ncols - 1 for s in range(nstrips) if s >= (k * b) // 64}


def kf(kmax, b, ncols, s):
    """The first step of strip s: the row tile of its last column, capped at kmax - 1."""
    return min(min(64 * s + 63, ncols - 1) // b, kmax - 1)


def ticket(L, kmax, b, ncols, t):
    s, k = ctypes.c_int(-7), ctypes.c_int(-7)
    st = L.tqr_apply_pipe_form_q_ticket(kmax, b, ncols, t, ctypes.byref(s), ctypes.byref(k))
    return st, s.value, k.value


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("kmax", KMAXS)
def test_items_and_ticket_order(tqr, kmax, b):
    L = tqr.lib()
    for ncols in ncols_of(kmax, b):
        want = items_expected(kmax, b, ncols)
        nstrips = -(-ncols // 64)
        # the two descriptions of the item set agree: k <= kf(s)
        assert want == {(s, k) for s in range(nstrips) for k in range(kmax) if k <= kf(kmax, b, ncols, s)}
        n = L.tqr_apply_pipe_form_q_items(kmax, b, ncols)
        assert n == len(want) == tqr.apply_pipe_form_q_items(kmax, b, ncols), (kmax, b, ncols)
        of = {}
        for t in range(n):
            st, s, k = ticket(L, kmax, b, ncols, t)
            assert st == 0 and (s, k) in want and (s, k) not in of, (kmax, b, ncols, t, st, s, k)
            of[(s, k)] = t
            assert tqr.apply_pipe_form_q_ticket(kmax, b, ncols, t) == (s, k)
        assert set(of) == want
        for (s, k), t in of.items():
            if k < kf(kmax, b, ncols, s):
                assert of[(s, k + 1)] < t, (kmax, b, ncols, s, k)  # the one producer came first
        # tickets run step-descending
        steps = [k for (_, k), _ in sorted(of.items(), key=lambda it: it[1])]
        assert steps == sorted(steps, reverse=True)
        for t in (-1, n, n + 1, 2 ** 31 - 1):
            assert ticket(L, kmax, b, ncols, t) == (EINVAL, -7, -7), (kmax, b, ncols, t)


def test_items_and_ticket_invalid_args(tqr):
    L = tqr.lib()
    s, k = ctypes.c_int(-7), ctypes.c_int(-7)
    rs, rk = ctypes.byref(s), ctypes.byref(k)
    for kmax, b, ncols in [(0, 64, 64), (-1, 64, 64), (2, 24, 64), (2, 0, 64), (2, 512, 64), (2, 64, 0), (2, 64, -5)]:
        assert L.tqr_apply_pipe_form_q_items(kmax, b, ncols) == EINVAL, (kmax, b, ncols)
        assert L.tqr_apply_pipe_form_q_ticket(kmax, b, ncols, 0, rs, rk) == EINVAL, (kmax, b, ncols)
    assert L.tqr_apply_pipe_form_q_ticket(2, 64, 128, 0, None, rk) == EINVAL
    assert L.tqr_apply_pipe_form_q_ticket(2, 64, 128, 0, rs, None) == EINVAL
    assert (s.value, k.value) == (-7, -7), "a refused call writes nothing"
    assert L.tqr_apply_pipe_form_q_ticket(2, 64, 128, 0, rs, rk) == 0  # (the good call those were one step from)
    assert (s.value, k.value) == (1, 1)
    with pytest.raises(tqr.TQRError):
        tqr.apply_pipe_form_q_ticket(2, 64, 128, 3)
    with pytest.raises(tqr.TQRError):
        tqr.apply_pipe_form_q_items(2, 24, 128)


def test_counts_of_the_design_note(tqr):
    """The tile-operation counts DESIGN.md §17 quotes: step k costs p - k tile operations per strip."""
    L = tqr.lib()
    for m, n, b, ncols, num, den in [(16384, 16384, 256, 16384, 357760, 532480), (4096, 4096, 128, 4096, 22880, 33792),
                                     (65536, 16384, 256, 16384, 1955200, 3678208)]:
        p, kmax = m // b, min(m, n) // b
        nstrips = -(-ncols // 64)
        full = nstrips * sum(p - k for k in range(kmax))
        mine = sum((p - k) * (nstrips - (k * b) // 64) for k in range(kmax) if k * b <= ncols - 1)
        assert (mine, full) == (num, den)
        assert L.tqr_apply_pipe_form_q_items(kmax, b, ncols) == sum(nstrips - (k * b) // 64 for k in range(kmax))


@pytest.fixture(scope="module")
def handle(tqr):
    """A handle for m = 128, n = 64, b = 32, fp64, nrhs_max = 200 > m (with or without a device)."""
    h = P()
    assert tqr.lib().tqr_apply_pipe_create(ctypes.byref(h), 128, 64, 32, F64, 200) == 0
    assert h.value
    yield h
    tqr.lib().tqr_apply_pipe_destroy(h)


# (dA, ldda, dQ, ncols, lddq) with one error each; the valid call is (Z, 128, Z, 1 .. 128, 128)
BAD_FORM_Q = {
    "dA NULL": (None, 128, Z, 64, 128),
    "dQ NULL": (Z, 128, None, 64, 128),
    "ncols = 0": (Z, 128, Z, 0, 128),
    "ncols < 0": (Z, 128, Z, -3, 128),
    "ncols = m + 1 (within nrhs_max)": (Z, 128, Z, 129, 128),
    "ncols > nrhs_max": (Z, 128, Z, 201, 128),
    "ldda < m": (Z, 127, Z, 64, 128),
    "lddq < m": (Z, 128, Z, 64, 127),
    "ldda beyond the leading-dimension bound": (Z, 8388608, Z, 64, 128),
    "lddq beyond the leading-dimension bound": (Z, 128, Z, 64, 8388608),
}


@pytest.mark.parametrize("why", sorted(BAD_FORM_Q))
def test_form_q_invalid_args_without_gpu(tqr, handle, why):
    assert tqr.lib().tqr_apply_pipe_form_q(handle, Z, *BAD_FORM_Q[why], None) == EINVAL, why


def test_form_q_null_handles(tqr, handle):
    L = tqr.lib()
    assert L.tqr_apply_pipe_form_q(None, Z, Z, 128, Z, 64, 128, None) == EINVAL
    assert L.tqr_apply_pipe_form_q(handle, None, Z, 128, Z, 64, 128, None) == EINVAL
    assert L.tqr_apply_pipe_form_q(None, None, None, 0, None, 0, 0, None) == EINVAL
    assert L.tqr_apply_pipe_status(handle, None) == 0  # nothing was enqueued


def test_ncols_beyond_nrhs_max_below_m(tqr):
    """nrhs_max < m: the handle's own limit refuses what m alone would allow."""
    L = tqr.lib()
    h = P()
    assert L.tqr_apply_pipe_create(ctypes.byref(h), 128, 64, 32, F32, 80) == 0
    try:
        assert L.tqr_apply_pipe_form_q(h, Z, Z, 128, Z, 81, 128, None) == EINVAL
    finally:
        L.tqr_apply_pipe_destroy(h)


class _Shape:
    def __init__(self, m, n, b, dtype):
        self.m, self.n, self.b, self.dtype, self.h = m, n, b, dtype, None


def test_python_wrapper_rejects_without_gpu(tqr):
    """ApplyPipe.form_q raises before the C call: a mismatched ApplyQ, ncols beyond nrhs_max or m."""
    import numpy as np
    pp = tqr.ApplyPipe(128, 64, 32, np.float64, 200)
    Q = np.zeros((64, 128))
    with pytest.raises(tqr.TQRError):
        pp.form_q(_Shape(128, 64, 32, F32), Q, Q)
    with pytest.raises(tqr.TQRError):
        pp.form_q(_Shape(128, 96, 32, F64), Q, Q)
    with pytest.raises(tqr.TQRError):
        pp.form_q(_Shape(128, 64, 32, F64), Q, Q, ncols=201)
    with pytest.raises(tqr.TQRError):
        pp.form_q(_Shape(128, 64, 32, F64), Q, Q, ncols=129)
