"""Form Q (tqr_apply_pipe_form_q; include/tqr.h "pipelined apply") on the GPU, against the pipelined
apply of Q to an explicit identity — tqr_apply_pipe_q(TQR_NOTRANS) on a device buffer that holds E, the
first ncols columns of I_m — and, for one shape, against tqr_apply_q on the same E. All three read the
same F through the same prepared ApplyQ. tests/test_gpu_apply_pipe.py and tests/test_gpu_apply.py hold
those references to each other, to the oracle and to numpy.

form_q runs the reference's tile operations in the reference's order on the non-zero data and leaves
out those that turn zeros into zeros, so the claim is equality of VALUES (np.array_equal: the sign of a
zero is free in the contract) with no tolerance. Whether the bytes are equal as well is asserted on its
own (test_bytes_equal_too), so that a difference there reads as what it is.

Every dQ allocation has PAD_R extra rows (lddq = m + PAD_R) and PAD_C extra columns holding SENTINEL,
and NaN in the m x ncols block before the call: dQ is output-only, so no NaN may survive, and an
implementation that loads dQ cannot pass. Arrays follow the module convention of tqr.py: row j of an
array is column j of the matrix.

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


def dn(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


_cache = {}


def factored(tqr, shape, dt):
    """(A, F, tau, ap): the shape's RANDZO matrix, its GPU factorisation F (n, m) and tau (kmax, m) on the
    device, and an ApplyQ prepared on them. Computed once per (shape, dtype), read-only."""
    import torch
    key = ("fact", shape, np.dtype(dt).name)
    if key not in _cache:
        m, n, b = shape
        F = torch.empty((n, m), dtype=tdt(dt), device="cuda")
        tqr.fill_randzo(F, m, n, 31 + 5 * b)
        A = F.clone()
        tau = torch.zeros((min(m, n) // b, m), dtype=F.dtype, device="cuda")
        plan = tqr.TiledQR(m, n, b, F.dtype)
        plan.execute(F, tau)
        plan.status()
        ap = tqr.ApplyQ(m, n, b, F.dtype)
        ap.prepare(F, tau)
        torch.cuda.synchronize()
        assert bool(torch.all(torch.isfinite(F))) and bool(torch.all(torch.isfinite(tau)))
        _cache[key] = (A, F, tau, ap)
    return _cache[key]


def alloc(m, ncols, dt, fill):
    """A dQ allocation (ncols + PAD_C, m + PAD_R) on the device: SENTINEL in the padding; the block holds
    NaN (fill = "nan") or E (fill = "eye")."""
    import torch
    d = torch.full((ncols + PAD_C, m + PAD_R), SENTINEL, dtype=tdt(dt), device="cuda")
    if fill == "nan":
        d[:ncols, :m] = float("nan")
    else:
        d[:ncols, :m] = 0.0
        d[:ncols, :m].fill_diagonal_(1.0)
    return d


def form(tqr, F, ap, ncols, dt, pp=None):
    """tqr_apply_pipe_form_q into a NaN-filled allocation; the allocation as a host array."""
    import torch
    d = alloc(ap.m, ncols, dt, "nan")
    pp = pp or tqr.ApplyPipe(ap.m, ap.n, ap.b, F.dtype, ncols)
    pp.form_q(ap, F, d, ncols=ncols)
    pp.status()
    torch.cuda.synchronize()
    return d.cpu().numpy()


def applied(tqr, F, ap, ncols, dt, pipe=True):
    """The reference: Q applied to an allocation that holds E (pipelined, or tqr_apply_q)."""
    import torch
    d = alloc(ap.m, ncols, dt, "eye")
    pp = tqr.ApplyPipe(ap.m, ap.n, ap.b, F.dtype, ncols) if pipe else None
    ap.apply(F, d, trans=False, nrhs=ncols, pipe=pp)
    if pp:
        pp.status()
    torch.cuda.synchronize()
    return d.cpu().numpy()


def pair(tqr, shape, dt, ncols):
    """(reference, form_q) allocations of a case, computed once and shared by the tests below."""
    key = ("pair", shape, np.dtype(dt).name, ncols)
    if key not in _cache:
        _, F, _, ap = factored(tqr, shape, dt)
        ref, got = applied(tqr, F, ap, ncols, dt), form(tqr, F, ap, ncols, dt)
        for x in (ref, got):
            x.setflags(write=False)
        _cache[key] = (ref, got)
    return _cache[key]


def assert_same_values(ref, got, m, ncols):
    assert np.all(np.isfinite(got[:ncols, :m])), "NaN of the pre-fill survived, or was read"
    assert np.array_equal(got[:ncols, :m], ref[:ncols, :m])
    assert np.all(got[ncols:] == SENTINEL) and np.all(got[:, m:] == SENTINEL), "padding touched"
    eye = np.eye(ncols, m, dtype=got.dtype)
    assert not np.array_equal(got[:ncols, :m], eye), "nothing was applied"


# (m, n, b): tests/test_gpu_apply_pipe.py's, for its reasons, and here: a strip spans four tile columns
# (b = 16); four strips per tile column, smin(k) = 0, 4, 8 (b = 256); kmax = p = 3; tall; kmax = 1 (no
# waits, everything synthesised); p = 1 (a lone UNMQR)
SHAPES = [(64, 64, 16), (768, 768, 256), (128, 96, 32), (512, 384, 128), (192, 320, 64), (1280, 256, 128),
          (192, 64, 64), (64, 128, 64)]


def ncols_of(shape):
    """thin; full (columns beyond kmax b) where that is more; one column; a ragged count that is a
    multiple of neither b nor 64."""
    m, n, b = shape
    ragged = b + 37 if b + 37 <= m else 37
    assert ragged % b and ragged % 64
    return sorted({min(m, n), m, 1, ragged})


CASES = [(s, c) for s in SHAPES for c in ncols_of(s)]
CIDS = ["%dx%db%d-c%d" % (s + (c,)) for s, c in CASES]


@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape,ncols", CASES, ids=CIDS)
def test_equals_apply_to_identity(tqr, shape, dt, ncols):
    """Checks 1 and 2: the values of the pipelined apply to E, finite, padding untouched, and no trace
    of the NaN the allocation held."""
    ref, got = pair(tqr, shape, dt, ncols)
    assert_same_values(ref, got, shape[0], ncols)


@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape,ncols", CASES, ids=CIDS)
def test_bytes_equal_too(tqr, shape, dt, ncols):
    """Beyond the contract: the skipped operations would have produced +0.0 from +0.0 (a sum of
    products with +0.0 added to +0.0 rounds to +0.0), and the synthesised zeros are +0.0, so the whole
    allocation is expected to be byte-equal to the reference's."""
    ref, got = pair(tqr, shape, dt, ncols)
    same = np.array_equal(ref.view(np.uint8), got.view(np.uint8))
    print(f"form_q vs apply to E, {shape}, {dn(dt)}, ncols = {ncols}: bytes {'equal' if same else 'DIFFER'}")
    assert same


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_equals_tqr_apply_q(tqr, dt):
    """The one-workgroup-per-strip kernel on the same E: the same values."""
    shape = (512, 384, 128)
    _, F, _, ap = factored(tqr, shape, dt)
    for ncols in (384, 512):
        ref = applied(tqr, F, ap, ncols, dt, pipe=False)
        assert_same_values(ref, pair(tqr, shape, dt, ncols)[1], shape[0], ncols)


@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape", [(128, 96, 32), (192, 320, 64), (768, 768, 256)], ids=lambda s: "%dx%db%d" % s)
def test_nan_where_form_q_must_not_read(tqr, shape, dt):
    """Check 3. NaN in every tile (l, k), l >= k, of the steps k with k b > ncols - 1, and in the strict
    upper triangle of R; the ApplyQ is prepared on that F, so those steps' T images are NaN as well.
    ncols = b (step 0 alone is read) and b + 1 (steps 0 and 1; kmax = 3 leaves step 2 poisoned): the
    result on the clean F. An apply to an identity walks every step and cannot pass."""
    import torch
    m, n, b = shape
    _, F, tau, ap = factored(tqr, shape, dt)
    kmax = min(m, n) // b
    assert kmax >= 3
    i, j = torch.arange(m, device="cuda")[None, :], torch.arange(n, device="cuda")[:, None]
    for ncols in (b, b + 1):
        k0 = (ncols - 1) // b + 1  # the first step that is not read
        assert 1 <= k0 < kmax
        Fn = F.clone()
        Fn[(i < j).expand(n, m)] = float("nan")  # array (j, i): element (i, j) of R's strict upper triangle
        for k in range(k0, kmax):
            Fn[k * b:(k + 1) * b, k * b:] = float("nan")
        apn = tqr.ApplyQ(m, n, b, F.dtype)
        apn.prepare(Fn, tau)
        got = form(tqr, Fn, apn, ncols, dt)
        clean = form(tqr, F, ap, ncols, dt)
        assert_same_values(clean, got, m, ncols)
        assert np.array_equal(got.view(np.uint8), clean.view(np.uint8))
        # (the reference does read them)
        assert not np.all(np.isfinite(applied(tqr, Fn, apn, ncols, dt)[:ncols, :m]))


@pytest.mark.parametrize("shape", [(512, 384, 128), (1280, 256, 128)], ids=lambda s: "%dx%db%d" % s)
def test_meaning(tqr, shape):
    """Check 4, fp64, the full Q (ncols = m): Q^T Q = I and Q[:, :n] R = A for the RANDZO A, computed with
    numpy on the host, to the bound tests/test_gpu_apply.py holds the apply to against numpy:
    max|error| <= 1e-11 * max(1, max|reference|)."""
    m, n, b = shape
    A, F, _, _ = factored(tqr, shape, np.float64)
    Q = pair(tqr, shape, np.float64, m)[1][:m, :m]  # row j = column j of Q
    e_orth = float(np.abs(Q @ Q.T - np.eye(m)).max())
    Fh, Ah = F.cpu().numpy(), A.cpu().numpy()
    R = np.tril(Fh[:, :n])  # array (j, i), i <= j: element (i, j) of R
    e_qr = float(np.abs(R @ Q[:n] - Ah).max())
    print(f"{shape}: max|Q^T Q - I| = {e_orth:.3e}, max|Q R - A| = {e_qr:.3e} (max|A| {np.abs(Ah).max():.3e})")
    assert e_orth <= 1e-11
    assert e_qr <= 1e-11 * max(1.0, float(np.abs(Ah).max()))
    # the thin Q is the leading columns of the full one
    assert np.array_equal(pair(tqr, shape, np.float64, n)[1][:n, :m], Q[:n])


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_handle_reuse_without_host_sync(tqr, dt):
    """20 form_q calls alternating with 20 apply calls on one handle, no host synchronisation in
    between: every Q is the reference's, every C is tqr_apply_q's, and the status is TQR_OK at the end."""
    import torch
    shape = (128, 96, 32)
    m, n, b = shape
    _, F, _, ap = factored(tqr, shape, dt)
    ncs = [[96, 1, 69, 128, 64][c % 5] for c in range(20)]
    rng = np.random.default_rng(5)
    C0 = [torch.from_numpy(rng.uniform(-1.0, 1.0, (17, m)).astype(dt)).cuda() for _ in range(20)]
    ref = [c.clone() for c in C0]
    for c, r in enumerate(ref):
        ap.apply(F, r, trans=bool(c % 2))
    Qs = [alloc(m, nc, dt, "nan") for nc in ncs]
    torch.cuda.synchronize()
    pp = tqr.ApplyPipe(m, n, b, F.dtype, 128)
    for c in range(20):
        pp.form_q(ap, F, Qs[c], ncols=ncs[c])
        pp.apply(ap, F, C0[c], trans=bool(c % 2))
    assert tqr.lib().tqr_apply_pipe_status(pp.h, None) == 0
    for c in range(20):
        assert_same_values(pair(tqr, shape, dt, ncs[c])[0], Qs[c].cpu().numpy(), m, ncs[c])
        assert torch.equal(C0[c], ref[c]), c


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_padded_lds_offset_base_and_stream(tqr, dt):
    """ldda = m + 5, lddq = m + 9, both arrays at an odd element offset inside their allocations, on a
    non-default stream: the whole Q buffer equals the pipelined apply's on E in the same layout, and F
    is unwritten."""
    import torch
    shape = (256, 192, 64)
    m, n, b = shape
    ncols, ldda, lddq, oa, oc = 229, m + 5, m + 9, 3, 5
    _, F, tau, _ = factored(tqr, shape, dt)
    bufF = torch.full((oa + n * ldda,), 2.5, dtype=F.dtype, device="cuda")
    dF = bufF[oa:].view(n, ldda)
    dF[:, :m] = F
    keepF = bufF.clone()
    bufs = [torch.full((oc + (ncols + PAD_C) * lddq + 4,), SENTINEL, dtype=F.dtype, device="cuda") for _ in range(2)]
    views = [bq[oc:oc + (ncols + PAD_C) * lddq].view(ncols + PAD_C, lddq) for bq in bufs]
    views[0][:ncols, :m] = 0.0
    views[0][:ncols, :m].fill_diagonal_(1.0)
    views[1][:ncols, :m] = float("nan")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    ap = tqr.ApplyQ(m, n, b, F.dtype)
    ap.prepare(dF, tau, ldda=ldda, stream=st)
    pp = tqr.ApplyPipe(m, n, b, F.dtype, ncols)
    pp.apply(ap, dF, views[0], trans=False, nrhs=ncols, ldda=ldda, lddc=lddq, stream=st)
    pp.form_q(ap, dF, views[1], ncols=ncols, ldda=ldda, lddq=lddq, stream=st)
    pp.status(st)
    st.synchronize()
    r, g = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    assert np.all(np.isfinite(g)) and np.array_equal(r, g)
    assert torch.all(views[1][ncols:] == SENTINEL) and torch.all(views[1][:, m:] == SENTINEL)
    assert np.array_equal(bufF.cpu().numpy(), keepF.cpu().numpy()), "dA was written"


def test_more_workgroups_than_resident(tqr):
    """b = 16, m = n = ncols = nrhs_max = 2048: 128 steps x up to 32 strips, 2112 work items against the
    256 resident at one workgroup per CU, so a ticket's producer may long have left, or a
    later-dispatched workgroup runs first. Only the ticket order makes that safe."""
    shape, ncols = (2048, 2048, 16), 2048
    assert tqr.apply_pipe_form_q_items(128, 16, ncols) == 2112
    ref, got = pair(tqr, shape, np.float64, ncols)
    assert_same_values(ref, got, shape[0], ncols)
    assert np.array_equal(ref.view(np.uint8), got.view(np.uint8))


@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("shape", [(128, 96, 32), (192, 320, 64)], ids=lambda s: "%dx%db%d" % s)
def test_python_form_q(tqr, shape, dt):
    """Check 6: tqr.form_q(F, tau, b) is the thin Q of the explicit calls, and ncols = m the full one."""
    m, n, b = shape
    _, F, tau, _ = factored(tqr, shape, dt)
    for ncols, arg in ((min(m, n), None), (m, m)):
        Q = tqr.form_q(F, tau, b, ncols=arg) if arg else tqr.form_q(F, tau, b)
        assert tuple(Q.shape) == (ncols, m) and Q.dtype == F.dtype
        assert np.array_equal(Q.cpu().numpy(), pair(tqr, shape, dt, ncols)[1][:ncols, :m])
    for bad in (0, m + 1):
        with pytest.raises(tqr.TQRError):
            tqr.form_q(F, tau, b, ncols=bad)


def test_refusals(tqr):
    """TQR_EINVAL with dQ unchanged, each against an otherwise valid call on a prepared ApplyQ: an
    ApplyPipe made for another m, n, b or dtype; ncols < 1, > m, > nrhs_max; NULL pointers; bad leading
    dimensions; an unprepared ApplyQ. The valid call itself succeeds."""
    import torch
    shape = (192, 128, 64)
    m, n, b = shape
    ncols = 101
    _, F, _, ap = factored(tqr, shape, np.float64)
    Q = alloc(m, ncols, np.float64, "nan")
    Q0 = Q.clone()
    L = tqr.lib()
    pF, pQ, ldq = P(F.data_ptr()), P(Q.data_ptr()), m + PAD_R
    good = tqr.ApplyPipe(m, n, b, np.float64, m + 8)
    small = tqr.ApplyPipe(m, n, b, np.float64, ncols - 1)
    bad_pipes = [tqr.ApplyPipe(m + b, n, b, np.float64, ncols), tqr.ApplyPipe(m, n + b, b, np.float64, ncols),
                 tqr.ApplyPipe(m, n, b // 2, np.float64, ncols), tqr.ApplyPipe(m, n, b, np.float32, ncols), small]
    for pp in bad_pipes:
        assert L.tqr_apply_pipe_form_q(pp.h, ap.h, pF, m, pQ, ncols, ldq, None) == EINVAL
        with pytest.raises(tqr.TQRError):
            pp.form_q(ap, F, Q, ncols=ncols)
    fresh = tqr.ApplyQ(m, n, b, np.float64)  # never prepared
    assert L.tqr_apply_pipe_form_q(good.h, fresh.h, pF, m, pQ, ncols, ldq, None) == EINVAL
    for args in [(None, m, pQ, ncols, ldq), (pF, m, None, ncols, ldq), (pF, m, pQ, 0, ldq), (pF, m, pQ, -1, ldq),
                 (pF, m, pQ, m + 1, ldq), (pF, m, pQ, m + 9, ldq), (pF, m - 1, pQ, ncols, ldq), (pF, m, pQ, ncols, m - 1),
                 (pF, 8388608, pQ, ncols, ldq), (pF, m, pQ, ncols, 8388608)]:
        assert L.tqr_apply_pipe_form_q(good.h, ap.h, *args, None) == EINVAL, args
    assert L.tqr_apply_pipe_form_q(None, ap.h, pF, m, pQ, ncols, ldq, None) == EINVAL
    assert L.tqr_apply_pipe_form_q(good.h, None, pF, m, pQ, ncols, ldq, None) == EINVAL
    assert good.status() is None
    torch.cuda.synchronize()
    assert np.array_equal(Q.cpu().numpy().view(np.uint8), Q0.cpu().numpy().view(np.uint8))
    assert L.tqr_apply_pipe_form_q(good.h, ap.h, pF, m, pQ, ncols, ldq, None) == 0
    assert good.status() is None
    assert_same_values(pair(tqr, shape, np.float64, ncols)[0], Q.cpu().numpy(), m, ncols)
