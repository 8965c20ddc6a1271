"""The batched apply / solve C ABI (include/tqr.h "batched apply and solve") without a GPU: every
argument error is reported before any device call, both stride forms at their exact boundaries for
every operand (A, C, X, B, Q, dres, the taus), and tqr_batch_apply_bytes against a re-derivation.

A handle can be created without a device: it then holds no device memory, answers workspace_bytes, and
every enqueueing call with valid arguments returns TQR_ENODEV — which shows that validation passed.
The file also runs where a GPU is present. There the module's handles are prepared on zero-filled
buffers, a made-up pointer only ever travels with at least one invalid argument, and a call whose
arguments are all valid gets zero-filled buffers of exactly the extent its layout spans (Call.accepted)."""
import ctypes

import pytest

from conftest import gpu_available

EINVAL, ENODEV = -1, -4
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call that carries it fails validation
M, N, B, BATCH, KMAX, NRHS = 48, 32, 16, 4, 2, 5

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


def apply_bytes(m, n, b, batch):
    """batch * ntiles * (b / min(b, 32)) * timg * 8: a T image (ib x (ib + 1) doubles padded to whole
    KiB) per 32-reflector group of every stored tile (l, k), l >= k, k < kmax."""
    ib = min(b, 32)
    timg = (ib * (ib + 1) + 127) // 128 * 128
    p, kmax = m // b, min(m, n) // b
    ntiles = kmax * p - kmax * (kmax - 1) // 2
    return batch * ntiles * (b // ib) * timg * 8


def extent(rows, cols, ld, stride, batch):
    return (batch - 1) * (0 if batch == 1 else stride) + (cols - 1) * ld + rows


def zeros(nelem):
    import torch
    return torch.zeros(max(1, nelem), dtype=torch.float64, device="cuda")


def create(tqr, m, n, b, dtype, batch):
    h = P()
    assert tqr.lib().tqr_batch_apply_create(ctypes.byref(h), m, n, b, dtype, batch) == 0
    assert h.value
    return h


def prepare_on_zeros(tqr, h, m, n, kmax, batch):
    """With a GPU: a first prepare, so that later refusals are the arguments' and not the missing prepare's."""
    if not gpu_available():
        return
    import torch
    A, tau = zeros(extent(m, n, m, n * m, batch)), zeros(batch * m * kmax)
    assert tqr.lib().tqr_batch_apply_prepare(h, P(A.data_ptr()), m, n * m, P(tau.data_ptr()), m * kmax, None) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def handle(tqr):
    """m = 48, n = 32, b = 16, fp64, batch = 4 (kmax = 2), with or without a device."""
    h = create(tqr, M, N, B, F64, BATCH)
    prepare_on_zeros(tqr, h, M, N, KMAX, BATCH)
    yield h
    tqr.lib().tqr_batch_apply_destroy(h)


class Call:
    """One entry point on (m, n, b, batch): its good arguments, how to issue it with some of them
    replaced, and the operands' (rows, cols, ld key, stride key) for real buffers."""

    def __init__(self, tqr, h, name, m=M, n=N, batch=BATCH, kmax=KMAX, ncols=N):
        self.L, self.h, self.name, self.m, self.n, self.batch, self.kmax = tqr.lib(), h, name, m, n, batch, kmax
        a = dict(dA=Z, ldda=m, strideA=n * m, trans=0)
        if name == "prepare":
            a.update(dtau=Z, strideTau=m * kmax)
            self.ops = {"dA": (m, n, "ldda", "strideA")}
        elif name == "apply_q":
            a.update(dC=Z, nrhs=NRHS, lddc=m, strideC=NRHS * m)
            self.ops = {"dA": (m, n, "ldda", "strideA"), "dC": (m, "nrhs", "lddc", "strideC")}
        elif name == "form_q":
            a.update(dQ=Z, ncols=ncols, lddq=m, strideQ=ncols * m)
            self.ops = {"dA": (m, n, "ldda", "strideA"), "dQ": (m, "ncols", "lddq", "strideQ")}
        elif name == "trsm_r":
            a.update(ldda=n, strideA=n * n, dX=Z, nrhs=NRHS, lddx=n, strideX=NRHS * n)
            self.ops = {"dA": (n, n, "ldda", "strideA"), "dX": (n, "nrhs", "lddx", "strideX")}
        elif name == "lstsq":
            a.update(dB=Z, nrhs=NRHS, lddb=m, strideB=NRHS * m, dres=Z, strideRes=NRHS)
            self.ops = {"dA": (m, n, "ldda", "strideA"), "dB": (m, "nrhs", "lddb", "strideB")}
        self.ok = a

    def issue(self, a):
        L, h = self.L, self.h
        if self.name == "prepare":
            return L.tqr_batch_apply_prepare(h, a["dA"], a["ldda"], a["strideA"], a["dtau"], a["strideTau"], None)
        if self.name == "apply_q":
            return L.tqr_batch_apply_q(h, a["trans"], a["dA"], a["ldda"], a["strideA"], a["dC"], a["nrhs"], a["lddc"],
                                       a["strideC"], None)
        if self.name == "form_q":
            return L.tqr_batch_form_q(h, a["dA"], a["ldda"], a["strideA"], a["dQ"], a["ncols"], a["lddq"], a["strideQ"], None)
        if self.name == "trsm_r":
            return L.tqr_batch_trsm_r(F64, a["trans"], self.n, B, self.batch, a["dA"], a["ldda"], a["strideA"], a["dX"],
                                      a["nrhs"], a["lddx"], a["strideX"], None)
        return L.tqr_batch_lstsq(h, a["trans"], a["dA"], a["ldda"], a["strideA"], a["dB"], a["nrhs"], a["lddb"], a["strideB"],
                                 a["dres"], a["strideRes"], None)

    def refused(self, **kw):
        """Made-up pointers and at least one invalid argument: TQR_EINVAL."""
        assert self.issue(dict(self.ok, **kw)) == EINVAL, (self.name, kw)

    def accepted(self, **kw):
        """All arguments valid. Without a GPU: TQR_ENODEV (validation passed, no device call). With one:
        TQR_OK on zero-filled buffers of exactly the extent the layout spans."""
        a = dict(self.ok, **kw)
        if not gpu_available():
            assert self.issue(a) == ENODEV, (self.name, kw)
            return
        import torch
        keep = []
        for key, (rows, cols, ld, stride) in self.ops.items():
            cols = a[cols] if isinstance(cols, str) else cols
            keep.append(zeros(extent(rows, cols, a[ld], a[stride], self.batch)))
            a[key] = P(keep[-1].data_ptr())
        if "dtau" in a:
            keep.append(zeros(extent(self.m * self.kmax, 1, self.m * self.kmax, a["strideTau"], self.batch)))
            a["dtau"] = P(keep[-1].data_ptr())
        if a.get("dres") is not None and "dres" in a:
            keep.append(zeros(extent(a["nrhs"], 1, a["nrhs"], a["strideRes"], self.batch)))
            a["dres"] = P(keep[-1].data_ptr())
        torch.cuda.synchronize()
        assert self.issue(a) == 0, (self.name, kw)
        torch.cuda.synchronize()


CALLS = ["prepare", "apply_q", "form_q", "trsm_r", "lstsq"]


# ---- create, bytes -----------------------------------------------------------------------------
@pytest.mark.parametrize("why", sorted(BAD_CREATE))
def test_create_invalid_args_without_gpu(tqr, why):
    h = P(12345)
    assert tqr.lib().tqr_batch_apply_create(ctypes.byref(h), *BAD_CREATE[why]) == EINVAL, why
    assert h.value is None, "no handle is returned with an error"
    assert tqr.lib().tqr_batch_apply_bytes(*BAD_CREATE[why]) == 0, why


def test_null_out_and_null_handle(tqr):
    L = tqr.lib()
    assert L.tqr_batch_apply_create(None, 64, 64, 32, F64, 3) == EINVAL
    assert L.tqr_batch_apply_workspace_bytes(None) == 0
    assert L.tqr_batch_apply_prepare(None, Z, M, N * M, Z, M * KMAX, None) == EINVAL
    assert L.tqr_batch_apply_q(None, 0, Z, M, N * M, Z, NRHS, M, NRHS * M, None) == EINVAL
    assert L.tqr_batch_form_q(None, Z, M, N * M, Z, N, M, N * M, None) == EINVAL
    assert L.tqr_batch_lstsq(None, 0, Z, M, N * M, Z, NRHS, M, NRHS * M, None, 0, None) == EINVAL
    L.tqr_batch_apply_destroy(None)  # a no-op


@pytest.mark.parametrize("m,n,b,dtype,batch", [(48, 32, 16, F64, 4), (256, 256, 32, F64, 16), (512, 256, 128, F32, 7),
                                               (64, 192, 16, F64, 1), (512, 256, 256, F32, 1024), (16, 16, 16, F64, 65537)])
def test_bytes_match_rederivation(tqr, m, n, b, dtype, batch):
    L = tqr.lib()
    want = apply_bytes(m, n, b, batch)
    assert L.tqr_batch_apply_bytes(m, n, b, dtype, batch) == want
    if want <= 1 << 24:  # (what create allocates where a device is present: the small ones only)
        h = create(tqr, m, n, b, dtype, batch)
        try:
            assert L.tqr_batch_apply_workspace_bytes(h) == want
        finally:
            L.tqr_batch_apply_destroy(h)


def test_create_without_device(tqr, handle):
    """p = 3, kmax = 2: 5 stored tiles, one 16 x 17 image of 384 doubles each, 4 members."""
    assert apply_bytes(M, N, B, BATCH) == 4 * 5 * 384 * 8
    assert tqr.lib().tqr_batch_apply_workspace_bytes(handle) == 4 * 5 * 384 * 8
    for name in CALLS:
        Call(tqr, handle, name).accepted()


# ---- refusals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CALLS)
def test_invalid_args_without_gpu(tqr, handle, name):
    c = Call(tqr, handle, name)
    rows = N if name == "trsm_r" else M
    c.refused(dA=None)
    c.refused(ldda=rows - 1)
    c.refused(ldda=0)
    c.refused(ldda=-rows)
    c.refused(ldda=8388608, strideA=N * 8388608)  # beyond the leading-dimension bound (fp64)
    for bad in (0, -1, -N * rows, rows - 1, rows, (N - 1) * rows + rows - 1):
        c.refused(strideA=bad)  # neither stacked nor row-interleaved
    c.refused(ldda=200, strideA=200 // 3)  # between the forms: the rows fit once but not 4 times
    c.refused(ldda=200, strideA=200)
    if name == "prepare":
        c.refused(dtau=None)
        for bad in (M * KMAX - 1, 0, -M * KMAX):
            c.refused(strideTau=bad)
        return
    op, cnt, ld, st = {"apply_q": ("dC", "nrhs", "lddc", "strideC"), "form_q": ("dQ", "ncols", "lddq", "strideQ"),
                       "trsm_r": ("dX", "nrhs", "lddx", "strideX"), "lstsq": ("dB", "nrhs", "lddb", "strideB")}[name]
    cols = c.ok[cnt]
    c.refused(**{op: None})
    c.refused(**{cnt: 0})
    c.refused(**{cnt: -1})
    c.refused(**{ld: rows - 1})
    c.refused(**{ld: 0})
    c.refused(**{ld: 8388608, st: cols * 8388608})
    for bad in (0, -1, rows - 1, rows, (cols - 1) * rows + rows - 1):
        c.refused(**{st: bad})
    if name == "form_q":
        c.refused(ncols=M + 1, strideQ=(M + 1) * M)
    else:
        c.refused(trans=2)
        c.refused(trans=-1)
    if name == "lstsq":
        c.refused(strideRes=NRHS - 1)
        c.refused(strideRes=0)
        c.refused(strideRes=-NRHS)


def test_trsm_r_own_arguments(tqr):
    L = tqr.lib()

    def run(dtype=F64, trans=0, n=N, b=B, batch=BATCH):
        return L.tqr_batch_trsm_r(dtype, trans, n, b, batch, Z, n if n > 0 else 1, n * n, Z, NRHS, n if n > 0 else 1,
                                  NRHS * n, None)

    assert run(dtype=2) == EINVAL
    assert run(b=24) == EINVAL
    assert run(n=0) == EINVAL
    assert run(n=40) == EINVAL  # b does not divide n
    assert run(batch=0) == EINVAL
    assert run(batch=-3) == EINVAL


def test_lstsq_needs_m_ge_n(tqr):
    L = tqr.lib()
    h = create(tqr, 32, 48, 16, F64, 2)  # wide: apply and form_q work, lstsq does not
    try:
        prepare_on_zeros(tqr, h, 32, 48, 2, 2)
        Call(tqr, h, "apply_q", m=32, n=48, batch=2).accepted()
        for trans in (0, 1):
            assert L.tqr_batch_lstsq(h, trans, Z, 32, 48 * 32, Z, NRHS, 32, NRHS * 32, None, 0, None) == EINVAL
    finally:
        L.tqr_batch_apply_destroy(h)


def test_calls_before_prepare(tqr):
    """Without a device the handle can never be prepared and says TQR_ENODEV; with one, every call but
    prepare is refused before the first prepare."""
    h = create(tqr, M, N, B, F64, BATCH)
    try:
        for name in CALLS:
            if name in ("prepare", "trsm_r"):
                continue
            assert Call(tqr, h, name).issue(Call(tqr, h, name).ok) == (EINVAL if gpu_available() else ENODEV), name
    finally:
        tqr.lib().tqr_batch_apply_destroy(h)


# ---- stride boundaries -------------------------------------------------------------------------
def test_a_and_tau_boundaries(tqr, handle):
    """A is 48 x 32, batch 4. Stacked: strideA >= 31 * ldda + 48 — with ldda = 50: 1598. Row-interleaved:
    strideA >= 48 and 3 * strideA + 48 <= ldda — strideA = 48 needs ldda >= 192; ldda = 200 allows 48 .. 50.
    strideTau >= m * kmax = 96. (tqr_batch_trsm_r's A is the leading 32 x 32: 31 * 50 + 32 = 1582; 32, 128.)"""
    for name in ("prepare", "apply_q", "form_q", "lstsq"):
        c = Call(tqr, handle, name)
        c.accepted(ldda=50, strideA=1598)
        c.refused(ldda=50, strideA=1597)
        c.accepted(ldda=192, strideA=48)
        c.refused(ldda=191, strideA=48)
        c.refused(ldda=192, strideA=47)
        c.accepted(ldda=200, strideA=50)
        c.refused(ldda=200, strideA=51)
    c = Call(tqr, handle, "prepare")
    c.accepted(strideTau=96)
    c.refused(strideTau=95)
    c = Call(tqr, handle, "trsm_r")
    c.accepted(ldda=50, strideA=1582)
    c.refused(ldda=50, strideA=1581)
    c.accepted(ldda=128, strideA=32)
    c.refused(ldda=127, strideA=32)
    c.refused(ldda=128, strideA=31)
    c.accepted(ldda=130, strideA=32)
    c.refused(ldda=130, strideA=33)


@pytest.mark.parametrize("name,ld,st,rows,cols", [("apply_q", "lddc", "strideC", M, NRHS), ("lstsq", "lddb", "strideB", M, NRHS),
                                                  ("trsm_r", "lddx", "strideX", N, NRHS), ("form_q", "lddq", "strideQ", M, N),
                                                  ("form_q", "lddq", "strideQ", M, M)])
def test_c_x_b_q_boundaries(tqr, handle, name, ld, st, rows, cols):
    """rows x cols members, batch 4. Stacked: stride >= (cols-1) * ld + rows, with ld = rows + 2.
    Row-interleaved: stride >= rows and 3 * stride + rows <= ld."""
    c = Call(tqr, handle, name, ncols=cols)
    pad = rows + 2
    c.accepted(**{ld: pad, st: (cols - 1) * pad + rows})
    c.refused(**{ld: pad, st: (cols - 1) * pad + rows - 1})
    c.accepted(**{ld: 4 * rows, st: rows})
    c.refused(**{ld: 4 * rows - 1, st: rows})
    c.refused(**{ld: 4 * rows, st: rows - 1})
    c.accepted(**{ld: 4 * rows + 8, st: rows + 2})
    c.refused(**{ld: 4 * rows + 8, st: rows + 3})


def test_dres_boundaries(tqr, handle):
    c = Call(tqr, handle, "lstsq")
    c.accepted(strideRes=NRHS)
    c.refused(strideRes=NRHS - 1)
    c.accepted(strideRes=NRHS + 3)
    for s in (0, -7, NRHS - 1):
        c.accepted(dres=None, strideRes=s)  # no dres: its stride is not looked at
    c.accepted(trans=1, dres=None, strideRes=0)


def test_batch_one_ignores_strides(tqr):
    h = create(tqr, M, N, B, F64, 1)
    try:
        prepare_on_zeros(tqr, h, M, N, KMAX, 1)
        for s in (0, -5, 7):
            Call(tqr, h, "prepare", batch=1).accepted(strideA=s)
            Call(tqr, h, "apply_q", batch=1).accepted(strideA=s, strideC=s)
            Call(tqr, h, "form_q", batch=1).accepted(strideA=s, strideQ=s)
            Call(tqr, h, "lstsq", batch=1).accepted(strideA=s, strideB=s, strideRes=s)
            Call(tqr, h, "trsm_r", batch=1).accepted(strideA=s, strideX=s)
        Call(tqr, h, "prepare", batch=1).refused(strideTau=M * KMAX - 1)  # checked with batch 1 too
        Call(tqr, h, "apply_q", batch=1).refused(lddc=M - 1)
        Call(tqr, h, "trsm_r", batch=1).refused(lddx=N - 1)
    finally:
        tqr.lib().tqr_batch_apply_destroy(h)


# ---- Python wrapper ----------------------------------------------------------------------------
def test_python_wrapper_without_gpu(tqr):
    import numpy as np
    with pytest.raises(tqr.TQRError):
        tqr.BatchedApply(100, 64, 32, np.float64, 3)
    with pytest.raises(tqr.TQRError):
        tqr.BatchedApply(128, 64, 32, np.float64, 0)
    with pytest.raises(tqr.TQRError):
        tqr.batch_apply_bytes(128, 64, 32, np.float64, 0)
    ba = tqr.BatchedApply(128, 64, 32, np.float32, 5)
    assert (ba.m, ba.n, ba.b, ba.batch, ba.kmax, ba.dtype) == (128, 64, 32, 5, 2, F32)
    assert ba.workspace_bytes() == apply_bytes(128, 64, 32, 5) == tqr.batch_apply_bytes(128, 64, 32, np.float32, 5)
    A = np.zeros((5, 64, 128), np.float32)
    C = np.zeros((5, 3, 128), np.float32)
    flat = np.zeros(5 * 64 * 128, np.float32)
    with pytest.raises(tqr.TQRError):
        ba.apply(A.astype(np.float64), C)  # the handle's dtype
    with pytest.raises(tqr.TQRError):
        ba.prepare(flat, np.zeros((5, 2, 128), np.float32))  # a flat buffer has no ldda to default to
    with pytest.raises(tqr.TQRError):
        ba.apply(A, flat[:5 * 3 * 128], lddc=128)  # nor an nrhs
    with pytest.raises(tqr.TQRError):
        ba.form_q(A, np.zeros((5, 129, 128), np.float32))  # ncols > m (refused by the library)
    with pytest.raises(tqr.TQRError):
        tqr.trsm_r_batched(A, C.astype(np.float64), 32)
    with pytest.raises(tqr.TQRError):
        tqr.trsm_r_batched(flat, C, 32, n=64, ldda=128)  # no batch to default to
    with pytest.raises(tqr.TQRError):
        tqr.trsm_r_batched(A, C, 24)  # b
