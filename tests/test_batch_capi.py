"""The batched factorisation's C ABI (include/tqr.h "batched") without a GPU: every argument error is
reported before any device call, the grouping and launch count of tqr_batch_plan against a
re-derivation from the wave plan's levels, and both stride forms at their exact boundaries.

A batch handle can be created without a device: it then holds no device memory, answers group and
workspace_bytes, and every execute with valid arguments returns TQR_ENODEV. The file also runs where
a GPU is present, so a made-up pointer only ever travels with at least one invalid argument; a call
whose arguments are all valid (the accepted side of a stride boundary) gets the no-device answer
here and real buffers there (accepted())."""
import ctypes

import pytest

from conftest import gpu_available

EINVAL, ENODEV = -1, -4
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call that carries it fails validation
GIB = 1 << 30

# (m, n, b, dtype, batch)
BAD_CREATE = {
    "bad dtype": (64, 64, 32, 2, 3),
    "b = 24": (96, 96, 24, F64, 3),
    "b = 512": (1024, 1024, 512, F64, 3),
    "b does not divide m": (100, 64, 32, F64, 3),
    "b does not divide n": (128, 100, 32, F64, 3),
    "m = 0": (0, 64, 32, F64, 3),
    "n < 0": (64, -64, 32, F64, 3),
    "batch = 0": (64, 64, 32, F64, 0),
    "batch < 0": (64, 64, 32, F64, -2),
    "m beyond the leading-dimension bound (fp64)": (8388608, 256, 256, F64, 2),
    "m beyond the leading-dimension bound (fp32)": (16777216, 256, 256, F32, 2),
}


def per_matrix_bytes(m, n, b):
    """The wave engine's T workspace of one matrix: p * kmax * (b / ib) images of ib x (ib + 1) doubles,
    each padded to whole KiB."""
    ib = min(b, 32)
    timg = (ib * (ib + 1) + 127) // 128 * 128
    return (m // b) * (min(m, n) // b) * (b // ib) * timg * 8


def launches_of_one_matrix(tqr, M, N):
    """Non-empty panel launches plus non-empty update launches over the levels of the wave plan."""
    nl = 0
    for wave in tqr.sched_plan(M, N):
        panel = sum(1 for t in wave if t[0] in (tqr.QRS, tqr.QRD))
        nl += (panel > 0) + (len(wave) - panel > 0)
    return nl


def create(tqr, m, n, b, dtype, batch, ws_limit=0):
    h = P()
    assert tqr.lib().tqr_batch_create(ctypes.byref(h), m, n, b, dtype, batch, ws_limit) == 0
    assert h.value
    return h


@pytest.fixture(scope="module")
def handle(tqr):
    """m = 48, n = 32, b = 16, fp64, batch = 4 (kmax = 2), with or without a device."""
    h = create(tqr, 48, 32, 16, F64, 4)
    yield h
    tqr.lib().tqr_batch_destroy(h)


def accepted(tqr, h, shape, ldda, strideA, strideTau):
    """Execute with arguments that are all valid. Without a GPU: TQR_ENODEV, i.e. validation passed and
    no device call was made. With one: the call runs on zero-filled buffers of exactly the extent the
    layout spans, and returns TQR_OK."""
    m, n, b, batch = shape
    kmax = min(m, n) // b
    L = tqr.lib()
    if not gpu_available():
        assert L.tqr_batch_execute(h, Z, ldda, strideA, Z, strideTau, None) == ENODEV
        return
    import torch
    sa = 0 if batch == 1 else strideA
    A = torch.zeros((batch - 1) * sa + (n - 1) * ldda + m, dtype=torch.float64, device="cuda")
    tau = torch.zeros((batch - 1) * strideTau + m * kmax, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.tqr_batch_execute(h, P(A.data_ptr()), ldda, strideA, P(tau.data_ptr()), strideTau, None) == 0
    torch.cuda.synchronize()


# ---- create ------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", sorted(BAD_CREATE))
def test_create_invalid_args_without_gpu(tqr, why):
    h = P(12345)
    assert tqr.lib().tqr_batch_create(ctypes.byref(h), *BAD_CREATE[why], 0) == EINVAL, why
    assert h.value is None, "no handle is returned with an error"
    g, ng, nl = (ctypes.c_int(-7) for _ in range(3))
    assert tqr.lib().tqr_batch_plan(*BAD_CREATE[why], 0, ctypes.byref(g), ctypes.byref(ng), ctypes.byref(nl)) == EINVAL
    assert (g.value, ng.value, nl.value) == (-7, -7, -7), "a refused call writes nothing"


def test_null_out_and_null_handle(tqr):
    L = tqr.lib()
    assert L.tqr_batch_create(None, 64, 64, 32, F64, 3, 0) == EINVAL
    assert L.tqr_batch_workspace_bytes(None) == 0
    assert L.tqr_batch_group(None) == EINVAL
    assert L.tqr_batch_execute(None, Z, 64, 64 * 64, Z, 64 * 2, None) == EINVAL
    L.tqr_batch_destroy(None)  # a no-op


def test_create_without_device(tqr, handle):
    """Good arguments: a handle, whose group and workspace follow from the shape alone (p = 3, kmax = 2,
    one 16 x 17 image of 384 doubles per tile: 18432 bytes per matrix, the whole batch in one group)."""
    L = tqr.lib()
    assert per_matrix_bytes(48, 32, 16) == 3 * 2 * 384 * 8
    assert L.tqr_batch_group(handle) == 4
    assert L.tqr_batch_workspace_bytes(handle) == 4 * 3 * 2 * 384 * 8
    accepted(tqr, handle, (48, 32, 16, 4), 48, 32 * 48, 2 * 48)


def test_python_wrapper_without_gpu(tqr):
    import numpy as np
    with pytest.raises(tqr.TQRError):
        tqr.BatchedQR(100, 64, 32, np.float64, 3)
    with pytest.raises(tqr.TQRError):
        tqr.BatchedQR(128, 64, 32, np.float64, 0)
    with pytest.raises(tqr.TQRError):
        tqr.batch_plan(128, 64, 32, np.float64, 0)
    per = per_matrix_bytes(128, 64, 32)
    bq = tqr.BatchedQR(128, 64, 32, np.float32, 5, ws_limit=2 * per)
    assert (bq.group(), bq.workspace_bytes()) == (2, 2 * per)
    assert tqr.batch_plan(128, 64, 32, np.float32, 5, ws_limit=2 * per)[:2] == (2, 3)


# ---- execute -----------------------------------------------------------------------------------
def test_execute_invalid_args_without_gpu(tqr, handle):
    """m = 48, n = 32, kmax = 2, batch = 4: good values are ldda = 48, strideA = 31 * 48 + 48, strideTau = 96."""
    L = tqr.lib()
    ok = dict(dA=Z, ldda=48, strideA=32 * 48, dtau=Z, strideTau=96)

    def run(**kw):
        a = dict(ok, **kw)
        return L.tqr_batch_execute(handle, a["dA"], a["ldda"], a["strideA"], a["dtau"], a["strideTau"], None)

    assert run(dA=None) == EINVAL
    assert run(dtau=None) == EINVAL
    assert run(ldda=47) == EINVAL
    assert run(ldda=0) == EINVAL
    assert run(ldda=-48) == EINVAL
    assert run(ldda=8388608, strideA=32 * 8388608) == EINVAL, "beyond the leading-dimension bound (fp64)"
    assert run(strideTau=95) == EINVAL
    assert run(strideTau=0) == EINVAL
    assert run(strideTau=-96) == EINVAL
    for bad in (0, -1, -32 * 48, 47, 48, 31 * 48 + 47):
        assert run(strideA=bad) == EINVAL, f"strideA = {bad}: neither stacked nor row-interleaved"
    # a stride between the two forms: rows fit once but not 4 times under ldda = 200
    assert run(ldda=200, strideA=51) == EINVAL
    assert run(ldda=200, strideA=200) == EINVAL


def test_stride_boundaries(tqr, handle):
    """Both forms at their smallest legal values, and one element less.
    Stacked: strideA >= (n-1) * ldda + m — with ldda = 50: 31 * 50 + 48 = 1598.
    Row-interleaved, batch = 4 domains of m = 48 rows: strideA >= m and 3 * strideA + m <= ldda — with
    strideA = 48 the smallest ldda is 192; with ldda = 200, strideA may be 48 .. 50.
    strideTau >= m * kmax = 96."""
    L = tqr.lib()
    shape = (48, 32, 16, 4)
    accepted(tqr, handle, shape, 50, 1598, 96)
    assert L.tqr_batch_execute(handle, Z, 50, 1597, Z, 96, None) == EINVAL
    accepted(tqr, handle, shape, 192, 48, 96)
    assert L.tqr_batch_execute(handle, Z, 191, 48, Z, 96, None) == EINVAL
    assert L.tqr_batch_execute(handle, Z, 192, 47, Z, 96, None) == EINVAL
    accepted(tqr, handle, shape, 200, 50, 96)
    assert L.tqr_batch_execute(handle, Z, 200, 51, Z, 96, None) == EINVAL
    accepted(tqr, handle, shape, 48, 32 * 48, 96)
    assert L.tqr_batch_execute(handle, Z, 48, 32 * 48, Z, 95, None) == EINVAL


def test_batch_one_ignores_stride(tqr):
    L = tqr.lib()
    h = create(tqr, 48, 32, 16, F64, 1)
    try:
        for stride in (0, -5, 7):
            accepted(tqr, h, (48, 32, 16, 1), 48, stride, 96)
        assert L.tqr_batch_execute(h, Z, 47, 0, Z, 96, None) == EINVAL
        assert L.tqr_batch_execute(h, Z, 48, 0, Z, 95, None) == EINVAL, "strideTau is checked with batch 1 too"
    finally:
        L.tqr_batch_destroy(h)


# ---- tqr_batch_plan ----------------------------------------------------------------------------
PLAN_POINTS = [(256, 256, 32, F64, 16), (512, 256, 128, F32, 7), (64, 192, 16, F64, 1)]


@pytest.mark.parametrize("m,n,b,dtype,batch", PLAN_POINTS)
def test_plan_matches_rederivation(tqr, m, n, b, dtype, batch):
    per = per_matrix_bytes(m, n, b)
    one = launches_of_one_matrix(tqr, m // b, n // b)
    assert one >= 1
    for ws_limit in (0, per, 3 * per, 3 * per + per - 1, per - 1, 1):
        fit = max(1, (ws_limit or GIB) // per)
        group = min(batch, 65535, fit)
        ngroups = -(-batch // group)
        assert tqr.batch_plan(m, n, b, dtype, batch, ws_limit) == (group, ngroups, ngroups * one), ws_limit
    # what create chooses is what the plan says
    h = create(tqr, m, n, b, dtype, batch, 3 * per)
    try:
        assert tqr.lib().tqr_batch_group(h) == min(batch, 3)
        assert tqr.lib().tqr_batch_workspace_bytes(h) == min(batch, 3) * per
    finally:
        tqr.lib().tqr_batch_destroy(h)


def test_plan_forced_groups(tqr):
    """Batch 5 with a ws_limit worth two matrices: group 2, 3 groups (2 + 2 + 1)."""
    per = per_matrix_bytes(128, 128, 64)
    one = launches_of_one_matrix(tqr, 2, 2)
    assert tqr.batch_plan(128, 128, 64, F64, 5, 2 * per) == (2, 3, 3 * one)
    assert tqr.batch_plan(128, 128, 64, F64, 5, 0) == (5, 1, one)


def test_plan_group_cap(tqr):
    """A grid's y dimension holds 65535: 70000 matrices of 16 x 16 (3 KiB of workspace each, so 1 GiB
    would hold far more) run in two groups."""
    assert per_matrix_bytes(16, 16, 16) * 70000 < GIB
    one = launches_of_one_matrix(tqr, 1, 1)
    assert tqr.batch_plan(16, 16, 16, F32, 70000, 0) == (65535, 2, 2 * one)
    assert tqr.batch_plan(16, 16, 16, F32, 65535, 0) == (65535, 1, one)
    assert tqr.batch_plan(16, 16, 16, F32, 65536, 0) == (65535, 2, 2 * one)


def test_plan_null_outputs(tqr):
    L = tqr.lib()
    g = ctypes.c_int(-7)
    assert L.tqr_batch_plan(64, 64, 32, F64, 3, 0, ctypes.byref(g), None, None) == 0
    assert g.value == 3
