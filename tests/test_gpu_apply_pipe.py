"""The pipelined apply (tqr_apply_pipe_q, tqr_lstsq_pipe; include/tqr.h "pipelined apply") on the GPU,
against tqr_apply_q / tqr_lstsq on the same device buffers.

The reference is the one-workgroup-per-strip kernel, which tests/test_gpu_apply.py holds against the
oracle and numpy. The pipelined kernel runs the same tile operations on the same operands in the same
order, so the claim checked here is equality of BYTES over the whole C allocation — padding rows and
columns included. No tolerance appears anywhere.

F and tau come from a GPU factorisation of a RANDZO matrix (computed once per shape, never written
afterwards); both calls read the same F through the same prepared ApplyQ. Every C allocation has
PAD_R extra rows (lddc = m + PAD_R) and PAD_C extra columns holding SENTINEL. Arrays follow the module
convention of tqr.py: row j of an array is column j of the matrix.

No test provokes a timeout: the bounded waits are read in the code (csrc/apply_pipe.hip)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL = -1
PAD_R, PAD_C = 3, 2
SENTINEL = 7.25
DTS = [np.float64, np.float32]
TRANS = [False, True]
TIDS = ["Q", "Qt"]


def dn(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


_cache = {}


def factored(tqr, shape, dt, seed=0):
    """(F, tau, ap): the GPU factorisation of the shape's RANDZO matrix, F (n, m) and tau (kmax, m) on
    the device, and an ApplyQ prepared on them. Computed once per (shape, dtype, seed), read-only."""
    import torch
    key = ("fact", shape, np.dtype(dt).name, seed)
    if key not in _cache:
        m, n, b = shape
        F = torch.empty((n, m), dtype=tdt(dt), device="cuda")
        tqr.fill_randzo(F, m, n, 31 + 5 * b + seed)
        tau = torch.zeros((min(m, n) // b, m), dtype=F.dtype, device="cuda")
        plan = tqr.TiledQR(m, n, b, F.dtype)
        plan.execute(F, tau)
        plan.status()
        ap = tqr.ApplyQ(m, n, b, F.dtype)
        ap.prepare(F, tau)
        torch.cuda.synchronize()
        assert bool(torch.all(torch.isfinite(F))) and bool(torch.all(torch.isfinite(tau)))
        _cache[key] = (F, tau, ap)
    return _cache[key]


def rhs(m, nrhs, dt, seed=0):
    """The whole C allocation (nrhs + PAD_C, m + PAD_R) on the host: right-hand sides in [-1, 1],
    SENTINEL in the padding rows and columns."""
    key = ("C", m, nrhs, np.dtype(dt).name, seed)
    if key not in _cache:
        rng = np.random.default_rng(70 + 3 * m + nrhs + seed)
        C = np.full((nrhs + PAD_C, m + PAD_R), SENTINEL, dtype=dt)
        C[:nrhs, :m] = rng.uniform(-1.0, 1.0, (nrhs, m))
        C.setflags(write=False)
        _cache[key] = C
    return _cache[key]


def raw(t):
    """The bytes of a device tensor's allocation."""
    return t.contiguous().cpu().numpy().view(np.uint8)


def both(tqr, F, ap, C, nrhs, trans, pp=None):
    """tqr_apply_q and the pipelined apply on device copies of the host allocation C; returns the two
    allocations as host arrays, reference first."""
    import torch
    d0 = torch.from_numpy(np.array(C)).cuda()
    d1 = d0.clone()
    pp = pp or tqr.ApplyPipe(ap.m, ap.n, ap.b, F.dtype, nrhs)
    ap.apply(F, d0, trans=trans, nrhs=nrhs)
    ap.apply(F, d1, trans=trans, nrhs=nrhs, pipe=pp)
    pp.status()
    torch.cuda.synchronize()
    return d0.cpu().numpy(), d1.cpu().numpy()


def assert_same_bytes(ref, got, C, m, nrhs):
    assert np.array_equal(ref.view(np.uint8), got.view(np.uint8))
    # (what the reference itself is held to elsewhere, restated so that this file stands alone)
    assert np.all(got[nrhs:] == SENTINEL) and np.all(got[:, m:] == SENTINEL), "padding touched"
    assert not np.array_equal(got[:nrhs, :m], C[:nrhs, :m]), "nothing was applied"
    assert np.all(np.isfinite(got))


# (m, n, b), the smallest at which each wait exists: square with p = kmax >= 3 (a step waits on a
# producer that itself waited), at the smallest and the largest tile; p = 4, kmax = 3; wide, kmax = p = 3
# (the last step is a lone UNMQR); tall, 9 hand-overs per step, kmax = 2; kmax = 1 (no waits at all);
# p = 1 (no TSMQR).
SHAPES = [(64, 64, 16), (768, 768, 256), (128, 96, 32), (512, 384, 128), (192, 320, 64), (1280, 256, 128),
          (192, 64, 64), (64, 128, 64)]


@pytest.mark.parametrize("nrhs", [1, 17, 64, 80])
@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%db%d" % s)
def test_bit_identical(tqr, shape, dt, trans, nrhs):
    """One lane, a ragged wave, one full strip, two strips with a partial one."""
    F, _, ap = factored(tqr, shape, dt)
    C = rhs(shape[0], nrhs, dt)
    ref, got = both(tqr, F, ap, C, nrhs, trans)
    assert_same_bytes(ref, got, C, shape[0], nrhs)


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape", [(128, 96, 32), (192, 320, 64)], ids=lambda s: "%dx%db%d" % s)
def test_nan_where_the_apply_must_not_read(tqr, shape, dt, trans):
    """NaN on and above the diagonal of F (R, and every tile column from kmax on): the bytes of the
    apply on the clean F."""
    import torch
    m, n, b = shape
    F, tau, ap = factored(tqr, shape, dt)
    Fn = F.clone()
    i, j = torch.arange(m, device="cuda")[None, :], torch.arange(n, device="cuda")[:, None]
    Fn[(i <= j).expand(n, m)] = float("nan")  # array (j, i): element (i, j) with i <= j
    apn = tqr.ApplyQ(m, n, b, F.dtype)
    apn.prepare(Fn, tau)
    C = rhs(m, 17, dt)
    ref, got = both(tqr, Fn, apn, C, 17, trans)
    assert_same_bytes(ref, got, C, m, 17)
    clean, _ = both(tqr, F, ap, C, 17, trans)
    assert np.array_equal(got.view(np.uint8), clean.view(np.uint8))


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_padded_lds_offset_base_and_stream(tqr, dt):
    """ldda = m + 5, lddc = m + 9, both arrays at an odd element offset inside their allocations, on a
    non-default stream: the whole buffers are byte-equal to tqr_apply_q's, and F is unwritten."""
    import torch
    shape = (256, 192, 64)
    m, n, b = shape
    nrhs, ldda, lddc, oa, oc = 80, m + 5, m + 9, 3, 5
    F, tau, _ = factored(tqr, shape, dt)
    bufF = torch.full((oa + n * ldda,), 2.5, dtype=F.dtype, device="cuda")
    dF = bufF[oa:].view(n, ldda)
    dF[:, :m] = F
    keepF = bufF.clone()
    C = rhs(m, nrhs, dt)
    bufs = []
    for _ in range(2):
        bc = torch.full((oc + (nrhs + PAD_C) * lddc + 4,), SENTINEL, dtype=F.dtype, device="cuda")
        bc[oc:oc + (nrhs + PAD_C) * lddc].view(nrhs + PAD_C, lddc)[:nrhs, :m] = torch.from_numpy(np.array(C[:nrhs, :m])).cuda()
        bufs.append(bc)
    views = [bc[oc:oc + (nrhs + PAD_C) * lddc].view(nrhs + PAD_C, lddc) for bc in bufs]
    before = raw(bufs[1])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ap = tqr.ApplyQ(m, n, b, F.dtype)
    ap.prepare(dF, tau, ldda=ldda, stream=st)
    pp = tqr.ApplyPipe(m, n, b, F.dtype, nrhs)
    for trans in (True, False, False):  # Q^T, then Q (back to C up to rounding), then Q again
        ap.apply(dF, views[0], trans=trans, nrhs=nrhs, ldda=ldda, lddc=lddc, stream=st)
        pp.apply(ap, dF, views[1], trans=trans, nrhs=nrhs, ldda=ldda, lddc=lddc, stream=st)
    pp.status(st)
    st.synchronize()
    assert np.array_equal(raw(bufs[0]), raw(bufs[1]))
    assert not np.array_equal(raw(bufs[1]), before)
    assert torch.all(views[1][nrhs:] == SENTINEL) and torch.all(views[1][:, m:] == SENTINEL)
    assert np.array_equal(raw(bufF), raw(keepF)), "dA was written"


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_handle_reuse_without_host_sync(tqr, dt):
    """20 calls back to back on one handle, no host synchronisation in between, alternating direction
    and nrhs <= nrhs_max: every result is tqr_apply_q's, and the status is TQR_OK at the end (epochs,
    the ticket re-arm and the serialisation of a handle's calls)."""
    import torch
    shape = (128, 96, 32)
    m, n, b = shape
    F, _, ap = factored(tqr, shape, dt)
    calls = [([80, 1, 17, 64, 33][c % 5], bool(c % 2)) for c in range(20)]
    C0 = [torch.from_numpy(np.array(rhs(m, nrhs, dt, seed=c))).cuda() for c, (nrhs, _) in enumerate(calls)]
    ref = [c.clone() for c in C0]
    for c, (nrhs, trans) in zip(ref, calls):
        ap.apply(F, c, trans=trans, nrhs=nrhs)
    torch.cuda.synchronize()
    pp = tqr.ApplyPipe(m, n, b, F.dtype, 80)
    for c, (nrhs, trans) in zip(C0, calls):
        pp.apply(ap, F, c, trans=trans, nrhs=nrhs)
    assert tqr.lib().tqr_apply_pipe_status(pp.h, None) == 0
    for i, (c, r) in enumerate(zip(C0, ref)):
        assert np.array_equal(raw(c), raw(r)), (i, calls[i])
        assert not np.array_equal(c.cpu().numpy(), rhs(m, calls[i][0], dt, seed=i)), "nothing was applied"


def test_two_handles_on_two_streams(tqr):
    """Two ApplyPipe handles, each on a stream of its own, against one prepared ApplyQ, enqueued
    together: both results are tqr_apply_q's."""
    import torch
    shape = (512, 384, 128)
    m, n, b = shape
    nrhs = 80
    F, _, ap = factored(tqr, shape, np.float64)
    C = [torch.from_numpy(np.array(rhs(m, nrhs, np.float64, seed=s))).cuda() for s in (1, 2)]
    ref = [c.clone() for c in C]
    for c, trans in zip(ref, TRANS):
        ap.apply(F, c, trans=trans, nrhs=nrhs)
    pps = [tqr.ApplyPipe(m, n, b, F.dtype, nrhs) for _ in C]
    streams = [torch.cuda.Stream() for _ in C]
    torch.cuda.synchronize()
    for pp, st, c, trans in zip(pps, streams, C, TRANS):
        pp.apply(ap, F, c, trans=trans, nrhs=nrhs, stream=st)
    for pp, st in zip(pps, streams):
        pp.status(st)
    for c, r in zip(C, ref):
        assert np.array_equal(raw(c), raw(r))


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_prepare_between_two_applies(tqr, dt):
    """A pipelined apply on one stream, a prepare with a second factorisation of the same shape on
    another, a pipelined apply again, nothing synchronised in between: the prepare waits for the first
    apply (it is recorded among the handle's applies) and the second apply waits for the prepare. Both
    results equal those of the same sequence with tqr_apply_q and a full synchronisation between steps."""
    import torch
    shape = (512, 384, 128)
    m, n, b = shape
    nrhs = 64
    F1, tau1, _ = factored(tqr, shape, dt)
    F2, tau2, _ = factored(tqr, shape, dt, seed=9)
    assert not torch.equal(F1, F2)
    Ca = torch.from_numpy(np.array(rhs(m, nrhs, dt, seed=1))).cuda()
    Cb = torch.from_numpy(np.array(rhs(m, nrhs, dt, seed=2))).cuda()
    Ra, Rb = Ca.clone(), Cb.clone()
    ap = tqr.ApplyQ(m, n, b, F1.dtype)
    # the reference sequence, synchronised
    ap.prepare(F1, tau1)
    torch.cuda.synchronize()
    ap.apply(F1, Ra, trans=True, nrhs=nrhs)
    torch.cuda.synchronize()
    ap.prepare(F2, tau2)
    torch.cuda.synchronize()
    ap.apply(F2, Rb, trans=True, nrhs=nrhs)
    torch.cuda.synchronize()
    # the same on two streams, pipelined, enqueued back to back
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pp = tqr.ApplyPipe(m, n, b, F1.dtype, nrhs)
    ap.prepare(F1, tau1, stream=s1)
    pp.apply(ap, F1, Ca, trans=True, nrhs=nrhs, stream=s1)
    ap.prepare(F2, tau2, stream=s2)
    pp.apply(ap, F2, Cb, trans=True, nrhs=nrhs, stream=s1)
    pp.status(s1)
    torch.cuda.synchronize()
    assert np.array_equal(raw(Ca), raw(Ra))
    assert np.array_equal(raw(Cb), raw(Rb))
    assert not np.array_equal(raw(Ra), raw(Rb))


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
def test_more_workgroups_than_resident(tqr, trans):
    """b = 16, m = n = 1024, nrhs = 512: kmax = 64 steps x 8 strips = 512 work items against the 256
    resident at one workgroup per CU (the kernel reserves 96 KiB of a CU's 160 KiB of LDS), so a
    ticket's producer may long have left, or a later-dispatched workgroup runs first. Only the ticket
    order makes that safe. The bytes are tqr_apply_q's."""
    shape, nrhs = (1024, 1024, 16), 512
    F, _, ap = factored(tqr, shape, np.float64)
    C = rhs(shape[0], nrhs, np.float64)
    ref, got = both(tqr, F, ap, C, nrhs, trans)
    assert_same_bytes(ref, got, C, shape[0], nrhs)


# ---- least squares ------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [3, 80])
@pytest.mark.parametrize("trans", TRANS, ids=["lsq", "minnorm"])
@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape", [(384, 256, 128), (192, 128, 64), (128, 128, 32)], ids=lambda s: "%dx%db%d" % s)
def test_lstsq_pipe(tqr, shape, dt, trans, nrhs):
    """tqr_lstsq_pipe against tqr_lstsq on the same buffers, both directions: the whole B allocation
    (X, the rest of Q^T B or the zeroed rows, the padding) and dres are byte-equal, through the C ABI
    and through the Python pipe= / solve= keywords."""
    import torch
    m, n, b = shape
    F, _, ap = factored(tqr, shape, dt)
    B = rhs(m, nrhs, dt, seed=4)
    pp = tqr.ApplyPipe(m, n, b, F.dtype, nrhs)
    sv = tqr.Solve(n, b, F.dtype, nrhs)
    L = tqr.lib()
    out = []
    for how in ("ref", "c", "py"):
        dB = torch.from_numpy(np.array(B)).cuda()
        res = torch.full((nrhs + 1,), -1.0, dtype=F.dtype, device="cuda")
        if how == "ref":
            ap.lstsq(F, dB, trans=trans, nrhs=nrhs, res=res)
        elif how == "py":
            ap.lstsq(F, dB, trans=trans, nrhs=nrhs, res=res, pipe=pp, solve=sv)
        else:
            st = L.tqr_lstsq_pipe(pp.h, sv.h, ap.h, 1 if trans else 0, P(F.data_ptr()), m, P(dB.data_ptr()), nrhs,
                                  m + PAD_R, P(res.data_ptr()), None)
            assert st == 0
        pp.status()
        sv.status()
        torch.cuda.synchronize()
        out.append((dB, res))
    for dB, res in out[1:]:
        assert np.array_equal(raw(dB), raw(out[0][0]))
        assert np.array_equal(raw(res), raw(out[0][1]))
    dB, res = out[1]
    assert not np.array_equal(dB.cpu().numpy()[:nrhs, :m], B[:nrhs, :m])
    assert torch.all(dB[nrhs:] == SENTINEL) and torch.all(dB[:, m:] == SENTINEL), "padding touched"
    assert torch.all(torch.isfinite(dB))
    assert res[nrhs] == -1.0
    if trans:
        assert torch.all(res == -1.0), "dres is not written in the TRANS direction"
    else:
        assert torch.all(torch.isfinite(res[:nrhs])) and torch.all(res[:nrhs] >= 0)
        if m == n:
            assert torch.all(res[:nrhs] == 0)


# ---- refusals -----------------------------------------------------------------------------------
def test_refusals(tqr):
    """TQR_EINVAL with C unchanged: an ApplyPipe made for another m, n, b or dtype; nrhs > nrhs_max; an
    unprepared ApplyQ; a Solve handle that does not match, in tqr_lstsq_pipe. The Python keywords raise
    before the C call."""
    import torch
    shape = (192, 128, 64)
    m, n, b = shape
    nrhs = 17
    F, _, ap = factored(tqr, shape, np.float64)
    C0 = torch.from_numpy(np.array(rhs(m, nrhs, np.float64))).cuda()
    C = C0.clone()
    L = tqr.lib()
    pF, pC, ldc = P(F.data_ptr()), P(C.data_ptr()), m + PAD_R
    good = tqr.ApplyPipe(m, n, b, np.float64, nrhs)
    sv = tqr.Solve(n, b, np.float64, nrhs)
    bad_pipes = [tqr.ApplyPipe(m + b, n, b, np.float64, nrhs), tqr.ApplyPipe(m, n + b, b, np.float64, nrhs),
                 tqr.ApplyPipe(m, n, b // 2, np.float64, nrhs), tqr.ApplyPipe(m, n, b, np.float32, nrhs),
                 tqr.ApplyPipe(m, n, b, np.float64, nrhs - 1)]
    for pp in bad_pipes:
        for trans in (0, 1):
            assert L.tqr_apply_pipe_q(pp.h, ap.h, trans, pF, m, pC, nrhs, ldc, None) == EINVAL
            assert L.tqr_lstsq_pipe(pp.h, sv.h, ap.h, trans, pF, m, pC, nrhs, ldc, None, None) == EINVAL
        with pytest.raises(tqr.TQRError):
            pp.apply(ap, F, C, nrhs=nrhs)
        with pytest.raises(tqr.TQRError):
            ap.lstsq(F, C, nrhs=nrhs, pipe=pp, solve=sv)
    fresh = tqr.ApplyQ(m, n, b, np.float64)  # never prepared
    for trans in (0, 1):
        assert L.tqr_apply_pipe_q(good.h, fresh.h, trans, pF, m, pC, nrhs, ldc, None) == EINVAL
        assert L.tqr_lstsq_pipe(good.h, sv.h, fresh.h, trans, pF, m, pC, nrhs, ldc, None, None) == EINVAL
    bad_solves = [tqr.Solve(n + b, b, np.float64, nrhs), tqr.Solve(n, b // 2, np.float64, nrhs),
                  tqr.Solve(n, b, np.float32, nrhs), tqr.Solve(n, b, np.float64, nrhs - 1)]
    for h in bad_solves:
        for trans in (0, 1):
            assert L.tqr_lstsq_pipe(good.h, h.h, ap.h, trans, pF, m, pC, nrhs, ldc, None, None) == EINVAL
        with pytest.raises(tqr.TQRError):
            ap.lstsq(F, C, nrhs=nrhs, pipe=good, solve=h)
    with pytest.raises(tqr.TQRError):
        ap.lstsq(F, C, nrhs=nrhs, pipe=good)  # pipe= without solve=
    # the other argument errors of tqr_apply_pipe_q on a matching pair
    for args in [(2, pF, m, pC, nrhs, ldc), (1, None, m, pC, nrhs, ldc), (1, pF, m, None, nrhs, ldc),
                 (1, pF, m, pC, 0, ldc), (1, pF, m - 1, pC, nrhs, ldc), (1, pF, m, pC, nrhs, m - 1),
                 (0, pF, m, pC, nrhs, 8388608)]:
        assert L.tqr_apply_pipe_q(good.h, ap.h, *args, None) == EINVAL, args
    # a wide factorisation has no least-squares problem
    wide = factored(tqr, (64, 128, 64), np.float64)
    wpp, wsv = tqr.ApplyPipe(64, 128, 64, np.float64, 4), tqr.Solve(128, 64, np.float64, 4)
    assert L.tqr_lstsq_pipe(wpp.h, wsv.h, wide[2].h, 0, P(wide[0].data_ptr()), 64, pC, 4, ldc, None, None) == EINVAL
    assert good.status() is None
    torch.cuda.synchronize()
    assert torch.equal(C, C0)
