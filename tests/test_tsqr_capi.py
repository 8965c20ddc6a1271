"""The tall-skinny QR's C ABI (include/tqr.h "tall-skinny") without a GPU: every argument error is
reported before any device call, and tqr_tsqr_plan against a Python re-derivation of m_dom, fan, the
levels, D_l and the bytes.

A handle can be created without a device: it then holds no device memory, answers workspace_bytes and
tqr_tsqr_level's integers, and every enqueueing call with valid arguments returns TQR_ENODEV. The file
also runs where a GPU is present, so a made-up pointer only ever travels with at least one invalid
argument; a call whose arguments are all valid gets the no-device answer here and real buffers there
(accepted())."""
import ctypes

import numpy as np
import pytest

import tsqr_ref
from conftest import gpu_available

EINVAL, ENODEV = -1, -4
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call that carries it fails validation
GIB = 1 << 30

# (m, n, b, dtype, m_dom, fan, nrhs_max)
BAD_SPEC = {
    "bad dtype": (256, 32, 16, 2, 64, 2, 4),
    "b = 24": (96, 48, 24, F64, 48, 2, 4),
    "b = 512": (2048, 512, 512, F64, 512, 2, 4),
    "b does not divide m": (250, 32, 16, F64, 0, 2, 4),
    "b does not divide n": (256, 40, 16, F64, 64, 2, 4),
    "m = 0": (0, 32, 16, F64, 0, 2, 4),
    "n < 0": (256, -32, 16, F64, 64, 2, 4),
    "m < n": (32, 64, 16, F64, 0, 2, 4),
    "m beyond the leading-dimension bound (fp64)": (8388608, 256, 256, F64, 1024, 2, 4),
    "m_dom not a multiple of b": (256, 32, 16, F64, 40, 2, 4),
    "m_dom < n": (256, 32, 16, F64, 16, 2, 4),
    "m_dom does not divide m": (256, 32, 16, F64, 48, 2, 4),
    "m_dom > m": (256, 32, 16, F64, 512, 2, 4),
    "m_dom < 0": (256, 32, 16, F64, -64, 2, 4),
    "fan = 1": (256, 32, 16, F64, 64, 1, 4),
    "fan < 0": (256, 32, 16, F64, 64, -2, 4),
    "fan * n beyond the leading-dimension bound": (1024, 256, 256, F64, 256, 32768, 4),
    "nrhs_max < 0": (256, 32, 16, F64, 64, 2, -1),
}


def r256(x):
    return (x + 255) // 256 * 256


def timg(b):
    ib = min(b, 32)
    return (ib * (ib + 1) + 127) // 128 * 128


def derive(m, n, b, dtype, m_dom=0, fan=0, nrhs_max=0, ws_limit=0):
    """(m_dom, fan, nlevels, [D_l], bytes) re-derived from include/tqr.h: per level the compact taus, one
    tqr_apply T workspace per domain, W_l and C_l (levels >= 1), each rounded up to 256 bytes, plus the
    level's tqr_batch workspace (group T workspaces of the wave engine)."""
    es = 8 if dtype == F64 else 4
    m_dom, fan = tsqr_ref.resolve(m, n, b, m_dom, fan)
    lv = tsqr_ref.levels_of(m, n, m_dom, fan)
    kmax, ng = n // b, b // min(b, 32)
    total = 0
    for l, (rows, D) in enumerate(lv):
        p = rows // b
        ntiles = kmax * p - kmax * (kmax - 1) // 2
        total += r256(D * rows * kmax * es) + r256(D * ntiles * ng * timg(b) * 8)
        if l:
            total += r256(D * rows * n * es) + r256(D * rows * nrhs_max * es)
        per = p * kmax * ng * timg(b) * 8
        total += min(D, 65535, max(1, (ws_limit or GIB) // per)) * per
    return m_dom, fan, len(lv), [D for _, D in lv], total


def create(tqr, *a):
    h = P()
    sp = tqr.TsqrSpec(*a)
    assert tqr.lib().tqr_tsqr_create(ctypes.byref(h), ctypes.byref(sp)) == 0
    assert h.value
    return h


@pytest.fixture(scope="module")
def handle(tqr):
    """m = 192, n = 32, b = 16, fp64, m_dom = 64, fan = 2, nrhs_max = 8: D = 3, 2, 1."""
    h = create(tqr, 192, 32, 16, F64, 64, 2, 8, 0)
    yield h
    tqr.lib().tqr_tsqr_destroy(h)


@pytest.fixture(scope="module")
def handle0(tqr):
    """The same shape with nrhs_max = 0: factor only."""
    h = create(tqr, 192, 32, 16, F64, 64, 2, 0, 0)
    yield h
    tqr.lib().tqr_tsqr_destroy(h)


# ---- create / plan -----------------------------------------------------------------------------
@pytest.mark.parametrize("why", sorted(BAD_SPEC))
def test_create_invalid_spec(tqr, why):
    L = tqr.lib()
    sp = tqr.TsqrSpec(*BAD_SPEC[why], 0)
    h = P(12345)
    assert L.tqr_tsqr_create(ctypes.byref(h), ctypes.byref(sp)) == EINVAL, why
    assert h.value is None, "no handle is returned with an error"
    md, f, nl = (ctypes.c_int(-7) for _ in range(3))
    ws = ctypes.c_size_t(77)
    dom = (ctypes.c_int * 4)(-7, -7, -7, -7)
    assert L.tqr_tsqr_plan(ctypes.byref(sp), ctypes.byref(md), ctypes.byref(f), ctypes.byref(nl), dom, 4,
                           ctypes.byref(ws)) == EINVAL, why
    assert (md.value, f.value, nl.value, ws.value, list(dom)) == (-7, -7, -7, 77, [-7] * 4), "a refused call writes nothing"


def test_null_arguments(tqr):
    L = tqr.lib()
    sp = tqr.TsqrSpec(192, 32, 16, F64, 64, 2, 8, 0)
    assert L.tqr_tsqr_create(None, ctypes.byref(sp)) == EINVAL
    h = P(12345)
    assert L.tqr_tsqr_create(ctypes.byref(h), None) == EINVAL and h.value is None
    assert L.tqr_tsqr_plan(None, None, None, None, None, 0, None) == EINVAL
    assert L.tqr_tsqr_workspace_bytes(None) == 0
    assert L.tqr_tsqr_level(None, 0, None, None, None, None, None) == EINVAL
    assert L.tqr_tsqr_factor(None, Z, 192, None) == EINVAL
    assert L.tqr_tsqr_apply_q(None, 1, Z, 192, Z, 1, 192, None) == EINVAL
    assert L.tqr_tsqr_form_q(None, Z, 192, Z, 192, None) == EINVAL
    assert L.tqr_tsqr_lstsq(None, 0, Z, 192, Z, 1, 192, None, None) == EINVAL
    L.tqr_tsqr_destroy(None)  # a no-op
    assert L.tqr_tsqr_plan(ctypes.byref(sp), None, None, None, None, 0, None) == 0, "outputs may be NULL"


PLAN_POINTS = {
    "defaults": (65536, 256, 64, F64, 0, 0, 0, 0),
    "defaults fp32, nrhs": (262144, 128, 128, F32, 0, 0, 64, 0),
    "D = 3, f = 2 (one zero block)": (192, 32, 16, F64, 64, 2, 8, 0),
    "D = 5, f = 4 (a group of 1 + 3 zero blocks)": (640, 64, 32, F64, 128, 4, 70, 0),
    "D = 5, f = 2": (320, 32, 32, F32, 64, 2, 3, 0),
    "D = 3, f = 4": (384, 64, 64, F64, 128, 4, 64, 0),
    "D_0 = 1": (64, 32, 16, F64, 64, 2, 5, 0),
    "m_dom = n": (320, 32, 32, F64, 32, 4, 32, 0),
    "m / b prime: one domain by default": (16 * 7, 16, 16, F64, 0, 0, 16, 0),
    "no multiple of b >= max(4 n, 1024) below m": (192, 32, 16, F64, 0, 0, 1, 0),
    "default m_dom with m = 5.5 * 1024": (5632, 64, 64, F64, 0, 0, 1, 0),
    "more domains than a grid's y": (65537 * 16, 16, 16, F64, 16, 16, 3, 0),
    "ws_limit forces batch groups": (1024, 128, 64, F64, 256, 2, 16, 100000),
}


@pytest.mark.parametrize("why", sorted(PLAN_POINTS))
def test_plan_matches_rederivation(tqr, why):
    a = PLAN_POINTS[why]
    want = derive(*a)
    assert tqr.tsqr_plan(*a) == want, why
    assert want[3][-1] == 1 and want[2] == len(want[3])
    for prev, nxt in zip(want[3], want[3][1:]):
        assert nxt == -(-prev // want[1])
    if a[0] <= 1024:  # what create chooses is what the plan says (handles without device memory are cheap)
        h = create(tqr, *a)
        try:
            assert tqr.lib().tqr_tsqr_workspace_bytes(h) == want[4]
        finally:
            tqr.lib().tqr_tsqr_destroy(h)


def test_plan_expected_values(tqr):
    """The re-derivation itself against values worked out by hand."""
    assert derive(65536, 256, 64, F64)[:4] == (1024, 4, 4, [64, 16, 4, 1])
    assert derive(16 * 7, 16, 16, F64)[:4] == (112, 4, 1, [1])
    assert derive(192, 32, 16, F64)[:4] == (192, 4, 1, [1]), "m is below 1024: one domain"
    assert derive(262144, 128, 128, F64)[:4] == (1024, 4, 5, [256, 64, 16, 4, 1]), "4 n = 512 is below 1024 rows"
    assert derive(5 * 1024 + 512, 64, 64, F64)[:2] == (1408, 4), "the first divisor of 5632 from 1024 on, in steps of b"
    assert derive(640, 64, 32, F64, 128, 4)[:4] == (128, 4, 3, [5, 2, 1])
    assert derive(65537 * 16, 16, 16, F64, 16, 16)[3] == [65537, 4097, 257, 17, 2, 1]
    # (64, 32, 16), one domain, nrhs_max 0: taus 64 * 2 * 8, T: 7 tiles of 384 doubles, batch: 4 * 2 images
    assert derive(64, 32, 16, F64, 64, 2)[4] == 1024 + 7 * 384 * 8 + 8 * 384 * 8


def test_plan_cap(tqr):
    L = tqr.lib()
    sp = tqr.TsqrSpec(256, 32, 16, F64, 64, 2, 0, 0)
    dom = (ctypes.c_int * 4)(-7, -7, -7, -7)
    nl = ctypes.c_int()
    assert L.tqr_tsqr_plan(ctypes.byref(sp), None, None, ctypes.byref(nl), dom, 2, None) == 0
    assert nl.value == 3 and list(dom) == [4, 2, -7, -7], "at most cap entries are written"


def test_level_without_device(tqr, handle):
    L = tqr.lib()
    for l, (rows, nd, ld) in enumerate([(64, 3, 0), (64, 2, 128), (64, 1, 64)]):
        w, t = P(5), P(5)
        ldw, r, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert L.tqr_tsqr_level(handle, l, ctypes.byref(w), ctypes.byref(ldw), ctypes.byref(t), ctypes.byref(r),
                                ctypes.byref(d)) == 0
        assert (ldw.value, r.value, d.value) == (ld, rows, nd)
        if l == 0:
            assert w.value is None, "level 0's matrix is the caller's"
        if not gpu_available():
            assert w.value is None and t.value is None
    assert L.tqr_tsqr_level(handle, 3, None, None, None, None, None) == EINVAL
    assert L.tqr_tsqr_level(handle, -1, None, None, None, None, None) == EINVAL
    assert L.tqr_tsqr_level(handle, 1, None, None, None, None, None) == 0, "outputs may be NULL"


def test_python_wrapper_without_gpu(tqr):
    with pytest.raises(tqr.TQRError):
        tqr.TSQR(256, 32, 16, np.float64, m_dom=48)
    with pytest.raises(tqr.TQRError):
        tqr.tsqr_plan(256, 32, 16, np.float64, fan=1)
    t = tqr.TSQR(640, 64, 32, np.float32, m_dom=128, fan=4, nrhs_max=70)
    assert (t.m_dom, t.fan, t.levels, t.domains) == (128, 4, 3, [5, 2, 1])
    assert t.workspace_bytes() == derive(640, 64, 32, F32, 128, 4, 70)[4]
    lv = t.level(1)
    assert (lv[1], lv[3], lv[4]) == (2 * 256, 256, 2)


# ---- the enqueueing calls ----------------------------------------------------------------------
def accepted(tqr, h, call, **kw):
    """A call whose arguments are all valid. Without a GPU: TQR_ENODEV, i.e. validation passed and no
    device call was made. With one: the call runs on real buffers (a zero matrix, factorised first) and
    returns TQR_OK. The handle is for (192, 32, 16, fp64), nrhs_max = 8."""
    L = tqr.lib()
    a = dict(trans=1, ldda=192, nrhs=8, ldc=192, res=False)
    a.update(kw)
    if not gpu_available():
        got = {"factor": lambda: L.tqr_tsqr_factor(h, Z, a["ldda"], None),
               "apply": lambda: L.tqr_tsqr_apply_q(h, a["trans"], Z, a["ldda"], Z, a["nrhs"], a["ldc"], None),
               "lstsq": lambda: L.tqr_tsqr_lstsq(h, a["trans"], Z, a["ldda"], Z, a["nrhs"], a["ldc"], None, None)}[call]()
        assert got == ENODEV, (call, kw)
        return
    import torch
    A = torch.zeros(32 * a["ldda"], dtype=torch.float64, device="cuda")
    A.view(32, a["ldda"])[:, :192] = torch.from_numpy(np.ascontiguousarray(
        np.random.default_rng(1).standard_normal((32, 192)))).cuda()
    C = torch.zeros(a["nrhs"] * a["ldc"], dtype=torch.float64, device="cuda")
    res = torch.zeros(a["nrhs"], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pA, pC = P(A.data_ptr()), P(C.data_ptr())
    assert L.tqr_tsqr_factor(h, pA, a["ldda"], None) == 0
    if call == "apply":
        assert L.tqr_tsqr_apply_q(h, a["trans"], pA, a["ldda"], pC, a["nrhs"], a["ldc"], None) == 0
    if call == "lstsq":
        assert L.tqr_tsqr_lstsq(h, a["trans"], pA, a["ldda"], pC, a["nrhs"], a["ldc"], P(res.data_ptr()), None) == 0
    torch.cuda.synchronize()


def test_factor_arguments(tqr, handle):
    L = tqr.lib()
    assert L.tqr_tsqr_factor(handle, None, 192, None) == EINVAL
    assert L.tqr_tsqr_factor(handle, Z, 191, None) == EINVAL
    assert L.tqr_tsqr_factor(handle, Z, 0, None) == EINVAL
    assert L.tqr_tsqr_factor(handle, Z, -192, None) == EINVAL
    assert L.tqr_tsqr_factor(handle, Z, 8388608, None) == EINVAL, "beyond the leading-dimension bound (fp64)"
    accepted(tqr, handle, "factor")
    accepted(tqr, handle, "factor", ldda=193)


def test_apply_arguments(tqr, handle):
    L = tqr.lib()
    ok = dict(trans=1, dA=Z, ldda=192, dC=Z, nrhs=8, ldc=192)

    def run(**kw):
        a = dict(ok, **kw)
        return L.tqr_tsqr_apply_q(handle, a["trans"], a["dA"], a["ldda"], a["dC"], a["nrhs"], a["ldc"], None)

    for bad in (dict(dA=None), dict(dC=None), dict(trans=2), dict(trans=-1), dict(nrhs=0), dict(nrhs=-1), dict(nrhs=9),
                dict(ldda=191), dict(ldc=191), dict(ldda=0), dict(ldc=-192), dict(ldda=8388608), dict(ldc=8388608)):
        assert run(**bad) == EINVAL, bad
    accepted(tqr, handle, "apply", nrhs=8)
    accepted(tqr, handle, "apply", nrhs=1, trans=0, ldc=193)


def test_lstsq_and_form_q_arguments(tqr, handle):
    L = tqr.lib()
    ok = dict(trans=0, dA=Z, ldda=192, dB=Z, nrhs=8, ldb=192)

    def run(**kw):
        a = dict(ok, **kw)
        return L.tqr_tsqr_lstsq(handle, a["trans"], a["dA"], a["ldda"], a["dB"], a["nrhs"], a["ldb"], None, None)

    for bad in (dict(dA=None), dict(dB=None), dict(trans=2), dict(nrhs=0), dict(nrhs=9), dict(ldda=191), dict(ldb=191),
                dict(ldb=8388608)):
        assert run(**bad) == EINVAL, bad
    accepted(tqr, handle, "lstsq", trans=0)
    accepted(tqr, handle, "lstsq", trans=1, nrhs=3)
    # form_q needs nrhs_max >= n = 32: this handle has 8
    assert L.tqr_tsqr_form_q(handle, Z, 192, Z, 192, None) == EINVAL
    h = create(tqr, 192, 32, 16, F64, 64, 2, 32, 0)
    try:
        assert L.tqr_tsqr_form_q(h, None, 192, Z, 192, None) == EINVAL
        assert L.tqr_tsqr_form_q(h, Z, 192, None, 192, None) == EINVAL
        assert L.tqr_tsqr_form_q(h, Z, 191, Z, 192, None) == EINVAL
        assert L.tqr_tsqr_form_q(h, Z, 192, Z, 191, None) == EINVAL
        if not gpu_available():
            assert L.tqr_tsqr_form_q(h, Z, 192, Z, 192, None) == ENODEV
    finally:
        L.tqr_tsqr_destroy(h)


def test_no_c_workspace_refuses_the_applies(tqr, handle0):
    """nrhs_max = 0: every apply / form_q / lstsq is an argument error (nrhs > nrhs_max), whatever else."""
    L = tqr.lib()
    assert L.tqr_tsqr_apply_q(handle0, 1, Z, 192, Z, 1, 192, None) == EINVAL
    assert L.tqr_tsqr_lstsq(handle0, 0, Z, 192, Z, 1, 192, None, None) == EINVAL
    assert L.tqr_tsqr_form_q(handle0, Z, 192, Z, 192, None) == EINVAL
    accepted(tqr, handle0, "factor")
