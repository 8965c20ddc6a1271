"""The pipelined solve (tqr_solve_trsm_r, tqr_lstsq_fused_solve; include/tqr.h "pipelined solve") on the
GPU, against tqr_trsm_r / tqr_lstsq_fused on the same inputs.

The reference is the one-workgroup-per-strip kernel, which tests/test_gpu_solve.py holds against numpy
componentwise. The pipelined kernel runs the same operations in the same order, so the claim checked
here is equality of BYTES over the whole X allocation — padding rows and columns included, so NaN and
inf positions and the untouched padding fall under the one comparison. No tolerance appears anywhere.

R needs no factorisation (the solve reads only the upper triangle): a random upper triangle with a
dominant diagonal (|r_ii| = n / 4 + 1 against off-diagonal entries in [-1, 1]: every solution stays
of the order of the right-hand side), and arbitrary values in [-5, 5] everywhere below the diagonal,
except where a test says otherwise. Arrays follow the module convention of tqr.py: row j of an array is
column j of the matrix.

No test provokes a timeout: the bounded waits are read in the code (csrc/solve_pipe.hip)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
EINVAL = -1
PAD_R, PAD_C = 3, 2  # padding rows (lddx = n + PAD_R) and columns of every X allocation
SENTINEL = 7.25
DTS = [np.float64, np.float32]
TRANS = [False, True]
TIDS = ["R", "Rt"]


def dn(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


_cache = {}


def triangle(n, dt, seed=0):
    """F (n, n): the upper triangle of the matrix (the lower triangle of the array) is R, the rest
    arbitrary. Computed once per (n, dtype, seed), read-only."""
    key = ("F", n, np.dtype(dt).name, seed)
    if key not in _cache:
        rng = np.random.default_rng(1000 + 7 * n + seed)
        R = np.tril(rng.uniform(-1.0, 1.0, (n, n)))  # array (j, i), i <= j
        R[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], n) * (n / 4 + 1 + rng.uniform(0, 1, n))
        F = (R + np.triu(rng.uniform(-5.0, 5.0, (n, n)), 1)).astype(dt)
        F.setflags(write=False)
        _cache[key] = F
    return _cache[key]


def rhs(n, nrhs, dt, seed=0):
    """The whole X allocation (nrhs + PAD_C, n + PAD_R): right-hand sides in [-1, 1], SENTINEL in the
    padding rows and columns."""
    key = ("X", n, nrhs, np.dtype(dt).name, seed)
    if key not in _cache:
        rng = np.random.default_rng(50 + 3 * n + nrhs + seed)
        X = np.full((nrhs + PAD_C, n + PAD_R), SENTINEL, dtype=dt)
        X[:nrhs, :n] = rng.uniform(-1.0, 1.0, (nrhs, n))
        X.setflags(write=False)
        _cache[key] = X
    return _cache[key]


def raw(t):
    """The bytes of a device tensor's allocation."""
    return t.contiguous().cpu().numpy().view(np.uint8)


def both(tqr, F, X, n, b, nrhs, trans, sv=None):
    """tqr_trsm_r and the pipelined solve on device copies of host F and X (whole allocations);
    returns the two X allocations as host arrays, reference first."""
    import torch
    dF = torch.from_numpy(np.array(F)).cuda()
    dX0 = torch.from_numpy(np.array(X)).cuda()
    dX1 = dX0.clone()
    sv = sv or tqr.Solve(n, b, dF.dtype, nrhs)
    tqr.trsm_r(dF, dX0, b, trans=trans, n=n, nrhs=nrhs)
    tqr.trsm_r(dF, dX1, b, trans=trans, n=n, nrhs=nrhs, solve=sv)
    sv.status()
    torch.cuda.synchronize()
    return dX0.cpu().numpy(), dX1.cpu().numpy()


def assert_same_bytes(ref, got, X, n, nrhs, finite=True):
    assert np.array_equal(ref.view(np.uint8), got.view(np.uint8))
    # (what the reference itself is held to elsewhere, restated so that this file stands alone)
    assert np.all(got[nrhs:] == SENTINEL) and np.all(got[:, n:] == SENTINEL), "padding touched"
    assert not np.array_equal(got[:nrhs, :n], X[:nrhs, :n]), "nothing was solved"
    if finite:
        assert np.all(np.isfinite(got))


SHAPES = [(64, 16), (128, 32), (256, 64), (512, 128), (768, 256)]  # T = 4 (b = 256: 3) tile rows


@pytest.mark.parametrize("nrhs", [1, 17, 64, 80])
@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("n,b", SHAPES)
def test_bit_identical(tqr, n, b, dt, trans, nrhs):
    """T >= 3 tile rows (a row waits for two producers at least, whose order matters); a partial wave,
    a ragged wave, a full strip, two strips with a partial one."""
    F, X = triangle(n, dt), rhs(n, nrhs, dt)
    ref, got = both(tqr, F, X, n, b, nrhs, trans)
    assert_same_bytes(ref, got, X, n, nrhs)


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_single_tile(tqr, dt, trans):
    """n = b = 64: one work item per strip, no waits at all."""
    F, X = triangle(64, dt), rhs(64, 80, dt)
    ref, got = both(tqr, F, X, 64, 64, 80, trans)
    assert_same_bytes(ref, got, X, 64, 80)


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("n,b", [(192, 64), (128, 16)])
def test_nan_below_the_diagonal(tqr, n, b, dt, trans):
    """NaN everywhere below the diagonal of every diagonal tile: the bytes of the solve on triu(R)."""
    F = np.array(triangle(n, dt))
    Fn = F.copy()
    for k in range(n // b):
        blk = Fn[k * b:(k + 1) * b, k * b:(k + 1) * b]
        blk[np.triu_indices(b, 1)] = np.nan  # array (j, i) with i > j: below the diagonal
    clean = np.tril(F)  # the upper triangle alone, zeros elsewhere
    X = rhs(n, 17, dt)
    ref, got = both(tqr, Fn, X, n, b, 17, trans)
    assert_same_bytes(ref, got, X, n, 17)
    _, got_clean = both(tqr, clean, X, n, b, 17, trans)
    assert np.array_equal(got.view(np.uint8), got_clean.view(np.uint8))


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_zero_diagonal_in_a_middle_tile(tqr, dt, trans):
    """r_jj = 0 in the middle tile row of three: the inf / NaN pattern is tqr_trsm_r's, byte for byte,
    and it is there (the rows solved before j are finite, row j is not)."""
    n, b, nrhs, j = 192, 64, 17, 64 + 21
    F = np.array(triangle(n, dt))
    F[j, j] = 0.0
    X = rhs(n, nrhs, dt)
    ref, got = both(tqr, F, X, n, b, nrhs, trans)
    assert_same_bytes(ref, got, X, n, nrhs, finite=False)
    before = got[:nrhs, :j] if trans else got[:nrhs, j + 1:n]
    assert np.all(np.isfinite(before)) and not np.any(np.isfinite(got[:nrhs, j]))


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_padded_lds_offset_base_and_stream(tqr, dt):
    """ldda = n + 5, lddx = n + 9, both arrays at an odd element offset inside their allocations, on a
    non-default stream: the bytes of tqr_trsm_r on the same buffers, and of the packed default-stream
    solve in the solved block."""
    import torch
    n, b, nrhs = 256, 64, 80
    ldda, lddx, oa, ox = n + 5, n + 9, 3, 5
    F, X = triangle(n, dt), rhs(n, nrhs, dt)
    bufF = torch.full((oa + n * ldda,), 2.5, dtype=tdt(dt), device="cuda")
    dF = bufF[oa:].view(n, ldda)
    dF[:, :n] = torch.from_numpy(np.array(F)).cuda()
    bufs = []
    for _ in range(2):
        bx = torch.full((ox + (nrhs + PAD_C) * lddx + 4,), SENTINEL, dtype=dF.dtype, device="cuda")
        bx[ox:ox + (nrhs + PAD_C) * lddx].view(nrhs + PAD_C, lddx)[:nrhs, :n] = torch.from_numpy(np.array(X[:nrhs, :n])).cuda()
        bufs.append(bx)
    views = [bx[ox:ox + (nrhs + PAD_C) * lddx].view(nrhs + PAD_C, lddx) for bx in bufs]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sv = tqr.Solve(n, b, dF.dtype, nrhs)
    for trans in TRANS:
        tqr.trsm_r(dF, views[0], b, trans=trans, n=n, nrhs=nrhs, ldda=ldda, lddx=lddx, stream=st)
        tqr.trsm_r(dF, views[1], b, trans=trans, n=n, nrhs=nrhs, ldda=ldda, lddx=lddx, stream=st, solve=sv)
    sv.status(st)
    st.synchronize()
    assert np.array_equal(raw(bufs[0]), raw(bufs[1]))
    assert torch.all(bufF[:oa] == 2.5) and torch.all(dF[:, n:] == 2.5), "dA was written"
    # R^{-T} R^{-1} X on packed arrays, default stream
    dP = torch.from_numpy(np.array(X)).cuda()
    dFp = torch.from_numpy(np.array(F)).cuda()
    for trans in TRANS:
        tqr.trsm_r(dFp, dP, b, trans=trans, n=n, nrhs=nrhs, solve=sv)
    sv.status()
    assert np.array_equal(raw(views[1][:nrhs, :n]), raw(dP[:nrhs, :n]))


@pytest.mark.parametrize("dt", DTS, ids=dn)
def test_handle_reuse_without_host_sync(tqr, dt):
    """20 calls back to back on one handle, no host synchronisation in between, alternating direction
    and nrhs <= nrhs_max: every result is tqr_trsm_r's, and the status is TQR_OK at the end (epochs,
    the ticket re-arm and the serialisation of a handle's calls)."""
    import torch
    n, b, nmax = 128, 32, 80
    F = triangle(n, dt)
    dF = torch.from_numpy(np.array(F)).cuda()
    calls = [([80, 1, 17, 64, 33][c % 5], bool(c % 2)) for c in range(20)]
    X0 = [torch.from_numpy(np.array(rhs(n, nrhs, dt, seed=c))).cuda() for c, (nrhs, _) in enumerate(calls)]
    ref = [x.clone() for x in X0]
    for x, (nrhs, trans) in zip(ref, calls):
        tqr.trsm_r(dF, x, b, trans=trans, n=n, nrhs=nrhs)
    torch.cuda.synchronize()
    sv = tqr.Solve(n, b, dF.dtype, nmax)
    for x, (nrhs, trans) in zip(X0, calls):
        sv.trsm_r(dF, x, trans=trans, nrhs=nrhs)
    assert tqr.lib().tqr_solve_status(sv.h, None) == 0
    for c, (x, r) in enumerate(zip(X0, ref)):
        assert np.array_equal(raw(x), raw(r)), (c, calls[c])


def test_two_handles_on_two_streams(tqr):
    """Two handles, each on a stream of its own, enqueued together: both results are tqr_trsm_r's."""
    import torch
    n, b, nrhs = 512, 64, 80
    dF = torch.from_numpy(np.array(triangle(n, np.float64))).cuda()
    X = [torch.from_numpy(np.array(rhs(n, nrhs, np.float64, seed=s))).cuda() for s in (1, 2)]
    ref = [x.clone() for x in X]
    for x, trans in zip(ref, TRANS):
        tqr.trsm_r(dF, x, b, trans=trans, n=n, nrhs=nrhs)
    svs = [tqr.Solve(n, b, dF.dtype, nrhs) for _ in X]
    streams = [torch.cuda.Stream() for _ in X]
    torch.cuda.synchronize()
    for sv, st, x, trans in zip(svs, streams, X, TRANS):
        sv.trsm_r(dF, x, trans=trans, nrhs=nrhs, stream=st)
    for sv, st in zip(svs, streams):
        sv.status(st)
    for x, r in zip(X, ref):
        assert np.array_equal(raw(x), raw(r))


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
def test_more_workgroups_than_resident(tqr, trans):
    """b = 16, n = 2048, nrhs = 2048: T = 128 tile rows x 32 strips = 4096 workgroups, more than the 2048
    four-wave workgroups 256 CUs hold at 8 waves per SIMD — and far more than are resident here: the
    kernel reserves 96 KiB of a CU's 160 KiB of LDS (the hand-over protocol is measured at one workgroup
    per CU; resource report of the b = 16 fp64 kernels: 60-64 registers, 12 of them AGPRs, 0 B scratch), so 256 are
    resident at a time and a ticket's producers may long have left, or not yet have started when a
    later-dispatched workgroup runs first. Only the ticket order makes that safe; it is exercised only
    here. The bytes are tqr_trsm_r's."""
    n, b, nrhs = 2048, 16, 2048
    F, X = triangle(n, np.float64), rhs(n, nrhs, np.float64)
    ref, got = both(tqr, F, X, n, b, nrhs, trans)
    assert_same_bytes(ref, got, X, n, nrhs)


# ---- fused least squares ------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", [3, 80])
@pytest.mark.parametrize("dt", DTS, ids=dn)
@pytest.mark.parametrize("m,n,b", [(384, 256, 128), (192, 128, 64)])
def test_lstsq_fused_solve(tqr, oracle, m, n, b, dt, nrhs):
    """tqr_lstsq_fused_solve against tqr_lstsq_fused on [A | B | padding]: X, the rest of Q^T B, the
    padding, the factorisation, tau and the residual norms are byte-equal; so are the results of the
    Python solve= keywords. A handle that does not match the plan is refused before any launch."""
    import torch
    A = oracle.randzo(m, n, dt, seed=7)
    B = oracle.randzo(m, nrhs, dt, seed=8)
    r = -(-nrhs // b)
    AB0 = torch.full((n + r * b, m), 3.5, dtype=tdt(dt), device="cuda")
    AB0[:n] = torch.from_numpy(A).cuda()
    AB0[n:n + nrhs] = torch.from_numpy(B).cuda()
    plan = tqr.TiledQR(m, n + r * b, b, AB0.dtype, steps=n // b)
    sv = tqr.Solve(n, b, AB0.dtype, nrhs)
    out = []
    for solve in (None, sv):
        AB = AB0.clone()
        tau = torch.zeros((n // b, m), dtype=AB.dtype, device="cuda")
        res = torch.full((nrhs,), -1.0, dtype=AB.dtype, device="cuda")
        plan.lstsq_fused(AB, tau, nrhs, res=res, solve=solve)
        plan.status()
        sv.status()
        out.append((AB, tau, res))
    for x, y in zip(*out):
        assert np.array_equal(raw(x), raw(y))
    assert not torch.equal(out[1][0][n:n + nrhs, :n], AB0[n:n + nrhs, :n])
    assert torch.all(torch.isfinite(out[1][2])) and torch.all(out[1][2] >= 0)
    # handles that do not match the plan, or too small: TQR_EINVAL, nothing enqueued, nothing written
    L = tqr.lib()
    AB, tau = AB0.clone(), torch.zeros((n // b, m), dtype=AB0.dtype, device="cuda")
    other = torch.float32 if AB0.dtype == torch.float64 else torch.float64
    bad = [tqr.Solve(n + b, b, AB0.dtype, nrhs), tqr.Solve(n, b // 2, AB0.dtype, nrhs), tqr.Solve(n, b, other, nrhs)]
    if nrhs > 1:
        bad.append(tqr.Solve(n, b, AB0.dtype, nrhs - 1))
    for h in bad:
        st = L.tqr_lstsq_fused_solve(plan.h, h.h, P(AB.data_ptr()), m, P(tau.data_ptr()), nrhs, None, None)
        assert st == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(AB, AB0)
    # the Python form
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    p0 = tqr.lstsq_fused(dA, dB, b)
    p1 = tqr.lstsq_fused(dA, dB, b, solve=sv)
    torch.cuda.synchronize()
    for x, y in zip(p0, p1):
        assert np.array_equal(raw(x), raw(y))
    assert np.array_equal(raw(p1[0]), raw(out[1][0][n:n + nrhs, :n]))
