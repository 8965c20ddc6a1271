"""Batched apply, form-Q, solve and least squares (include/tqr.h "batched apply and solve",
csrc/batch_apply.hip) on the device.

The contract is one of bytes: member i of a batch has the bytes of the per-member public call on it
alone (tqr_apply_q on a handle prepared on the member, tqr_trsm_r, tqr_lstsq), and nothing outside the
members is written. So almost every check compares whole allocations — NaN-filled gaps and 7 guard
elements included — with clones of the same allocations after the per-member calls ran on each member
in turn through offset pointers. No tolerance. The factorisations come from tqr.BatchedQR. One
least-squares case goes against numpy.linalg.lstsq with tests/test_gpu_solve.py's bounds (1e-11 cond(A)
and 1e-11 |B|_F), and one form-Q member is checked for meaning with test_gpu_form_q's (1e-11, and 1e-11
max(1, max|A|)), so the feature does not rest on the library alone.

A. prepare + apply_q; B. trsm_r_batched; C. lstsq; D. form_q; E. layouts; F. member independence;
G. more members than a grid's y; H. ordering; I. refusals with live device buffers.
"""
import ctypes
import threading

import numpy as np
import pytest

import inputs
from inputs import dtname
from test_gpu_batch import CASES, Layout, ids, same_bytes, tdt

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TQR_EINVAL = -1
P = ctypes.c_void_p
NRHS = [1, 5, 64, 70]  # one lane, a ragged wave, a full strip, two strips (the second ragged, with an idle wave)
TALL = [(s, dt) for s, dt in CASES if s[0] >= s[1]]
SMALL = (96, 64, 32)
NAN = float("nan")


class Mat:
    """`batch` members of rows x cols inside one flat NaN-filled device buffer: member i at element base +
    i * stride, column-major with leading dimension ld. The buffer ends in 7 guard elements."""

    def __init__(self, rows, cols, dt, batch, ld=None, stride=None, base=0, extent=None):
        import torch
        self.rows, self.cols, self.dt, self.batch, self.base = rows, cols, dt, batch, base
        self.ld = ld or rows
        self.stride = cols * self.ld if stride is None else stride
        size = extent or base + (batch - 1) * self.stride + (cols - 1) * self.ld + rows
        self.buf = torch.full((size + 7,), NAN, dtype=tdt(dt), device="cuda")

    def view(self, buf=None):
        """(batch, cols, rows) strided view of the members (of self.buf, or of a clone of it)."""
        import torch
        return torch.as_strided(self.buf if buf is None else buf, (self.batch, self.cols, self.rows),
                                (self.stride, self.ld, 1), self.base)

    def at(self, i, buf=None):
        return (self.buf if buf is None else buf)[self.base + i * self.stride:]

    def fill(self, seed=0):
        import torch
        v = np.random.default_rng(1000 + seed).standard_normal((self.batch, self.cols, self.rows)).astype(self.dt)
        self.view().copy_(torch.from_numpy(v).cuda())
        torch.cuda.synchronize()
        return self

    def host(self, buf=None):
        import torch
        torch.cuda.synchronize()
        return (self.buf if buf is None else buf).cpu().numpy()


_fac, _apq = {}, {}


def factored(tqr, shape, dt, batch=3, offset0=0, **kw):
    """A Layout (test_gpu_batch) of Gaussian members after BatchedQR ran on it; shared, read-only."""
    import torch
    key = (shape, dtname(dt), batch, offset0, tuple(sorted(kw.items())))
    if key not in _fac:
        m, n, b = shape
        lay = Layout(shape, dt, batch, **kw).fill(offset0)
        lay.execute(tqr.BatchedQR(m, n, b, tdt(dt), batch))
        torch.cuda.synchronize()
        _fac[key] = lay
    return _fac[key]


def apq(tqr, shape, dt):
    """The per-member handle of the references."""
    key = (shape, dtname(dt))
    if key not in _apq:
        m, n, b = shape
        _apq[key] = tqr.ApplyQ(m, n, b, tdt(dt))
    return _apq[key]


def a_args(lay):
    return dict(ldda=lay.ldda, strideA=lay.sA)


def member(lay, i, A=None):
    return (lay.A if A is None else A)[lay.base + i * lay.sA:], lay.tau[lay.tbase + i * lay.sT:]


def prepared(tqr, lay, stream=None):
    m, n, b = lay.shape
    ba = tqr.BatchedApply(m, n, b, tdt(lay.dt), lay.batch)
    ba.prepare(lay.A[lay.base:], lay.tau[lay.tbase:], strideTau=lay.sT, stream=stream, **a_args(lay))
    return ba


def b_apply(ba, lay, C, trans, stream=None):
    ba.apply(lay.A[lay.base:], C.buf[C.base:], trans=trans, nrhs=C.cols, lddc=C.ld, strideC=C.stride, stream=stream,
             **a_args(lay))


def b_lstsq(ba, lay, Bm, trans, res=None, stream=None):
    ba.lstsq(lay.A[lay.base:], Bm.buf[Bm.base:], trans=trans, nrhs=Bm.cols, lddb=Bm.ld, strideB=Bm.stride,
             res=None if res is None else res.buf[res.base:], strideRes=None if res is None else res.stride, stream=stream,
             **a_args(lay))


def ref_apply(tqr, lay, C, trans, buf=None):
    """A clone of C's buffer after tqr_apply_q ran on each member in turn (prepare on the member first)."""
    buf = C.buf.clone() if buf is None else buf
    ap = apq(tqr, lay.shape, lay.dt)
    for i in range(lay.batch):
        Ai, ti = member(lay, i)
        ap.prepare(Ai, ti, ldda=lay.ldda)
        ap.apply(Ai, C.at(i, buf), trans=trans, nrhs=C.cols, ldda=lay.ldda, lddc=C.ld)
    return C.host(buf)


def ref_lstsq(tqr, lay, Bm, trans, res=None):
    buf = Bm.buf.clone()
    rbuf = None if res is None else res.buf.clone()
    ap = apq(tqr, lay.shape, lay.dt)
    for i in range(lay.batch):
        Ai, ti = member(lay, i)
        ap.prepare(Ai, ti, ldda=lay.ldda)
        ap.lstsq(Ai, Bm.at(i, buf), trans=trans, nrhs=Bm.cols, ldda=lay.ldda, lddb=Bm.ld,
                 res=None if res is None else res.at(i, rbuf))
    return Bm.host(buf), None if res is None else res.host(rbuf)


def ref_trsm(tqr, lay, X, trans):
    buf = X.buf.clone()
    n, b = lay.shape[1], lay.shape[2]
    for i in range(lay.batch):
        tqr.trsm_r(member(lay, i)[0], X.at(i, buf), b, trans=trans, n=n, nrhs=X.cols, ldda=lay.ldda, lddx=X.ld)
    return X.host(buf)


def b_trsm(tqr, lay, X, trans, A=None):
    n, b = lay.shape[1], lay.shape[2]
    tqr.trsm_r_batched((lay.A if A is None else A)[lay.base:], X.buf[X.base:], b, trans=trans, n=n, nrhs=X.cols,
                       batch=lay.batch, lddx=X.ld, strideX=X.stride, **a_args(lay))


def assert_bytes(got, ref, what=""):
    assert same_bytes(got, ref), f"{what}: the buffers differ in bytes"


def check_written(M_, host):
    """Every member element is finite and everything else of the buffer is still NaN."""
    import torch
    t = torch.from_numpy(host.copy())
    v = M_.view(t)
    assert torch.isfinite(v).all()
    v.fill_(NAN)
    assert torch.isnan(t).all(), "an element outside the members was written"


# ---- A. prepare + apply_q ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", CASES, ids=ids(CASES))
def test_apply_bytes_equal_per_member(tqr, shape, dt):
    """Batch 3, padded ldda and lddc, gaps between the members, all NaN: for both directions and every
    nrhs the whole C allocation equals that after tqr_apply_q ran on each member in turn."""
    m, n, b = shape
    lay = factored(tqr, shape, dt, ldda=m + 3, strideA=n * (m + 3) + 5, strideTau=(min(m, n) // b) * m + 2)
    ba = prepared(tqr, lay)
    for trans in (True, False):
        for nrhs in NRHS:
            C = Mat(m, nrhs, dt, 3, ld=m + 2, stride=nrhs * (m + 2) + 3).fill(nrhs)
            ref = ref_apply(tqr, lay, C, trans)
            b_apply(ba, lay, C, trans)
            got = C.host()
            assert_bytes(got, ref, f"{shape} {dtname(dt)} trans={trans} nrhs={nrhs}")
            check_written(C, got)


# ---- B. trsm_r_batched ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", TALL, ids=ids(TALL))
def test_trsm_bytes_equal_per_member(tqr, shape, dt):
    """X (n x nrhs) <- R^{-1} X / R^{-T} X on the leading n x n of every member: the bytes of tqr_trsm_r
    per member, and the same bytes again with one member's V below the diagonal turned to NaN."""
    import torch
    m, n, b = shape
    lay = factored(tqr, shape, dt, ldda=m + 3, strideA=n * (m + 3) + 5, strideTau=(n // b) * m + 2)
    poisoned = lay.A.clone()
    low = torch.triu(torch.ones((n, n), dtype=torch.bool, device="cuda"), diagonal=1)  # array (j, i), i > j
    lay.mats(poisoned)[1][:, :n][low] = NAN
    for trans in (False, True):
        for nrhs in NRHS:
            X = Mat(n, nrhs, dt, 3, ld=n + 1, stride=nrhs * (n + 1) + 2).fill(nrhs)
            X2 = Mat(n, nrhs, dt, 3, ld=n + 1, stride=nrhs * (n + 1) + 2).fill(nrhs)
            ref = ref_trsm(tqr, lay, X, trans)
            b_trsm(tqr, lay, X, trans)
            b_trsm(tqr, lay, X2, trans, A=poisoned)
            got = X.host()
            assert_bytes(got, ref, f"{shape} {dtname(dt)} trans={trans} nrhs={nrhs}")
            assert_bytes(X2.host(), got, "V below the diagonal is never read as a value")
            check_written(X, got)


def test_trsm_batched_tensors(tqr):
    """The (batch, columns, ld) form with default strides."""
    import torch
    m, n, b = SMALL
    lay = factored(tqr, SMALL, F64)
    F = lay.mats().contiguous()
    X = Mat(n, 5, F64, 3).fill()
    ref = ref_trsm(tqr, lay, X, False)
    Xt = X.view().contiguous()
    tqr.trsm_r_batched(F, Xt, b, n=n)
    torch.cuda.synchronize()
    assert same_bytes(Xt.cpu().numpy(), X.view(torch.from_numpy(ref)).contiguous().numpy())


# ---- C. lstsq ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", TALL, ids=ids(TALL))
def test_lstsq_bytes_equal_per_member(tqr, shape, dt):
    """Both directions, with dres and without, against tqr_lstsq per member: B (X, the rest of Q^T B, the
    zeroed rows of TQR_TRANS) and dres, whole allocations. m == n: every residual norm is 0."""
    m, n, b = shape
    lay = factored(tqr, shape, dt, ldda=m + 3, strideA=n * (m + 3) + 5, strideTau=(n // b) * m + 2)
    ba = prepared(tqr, lay)
    for trans in (False, True):
        for nrhs in (5, 70):
            Bm = Mat(m, nrhs, dt, 3, ld=m + 2, stride=nrhs * (m + 2) + 3).fill(nrhs)
            Bn = Mat(m, nrhs, dt, 3, ld=m + 2, stride=nrhs * (m + 2) + 3).fill(nrhs)
            res = Mat(nrhs, 1, dt, 3, stride=nrhs + 3)
            refB, refR = ref_lstsq(tqr, lay, Bm, trans, res)
            b_lstsq(ba, lay, Bm, trans, res)
            b_lstsq(ba, lay, Bn, trans)  # dres = NULL
            got = Bm.host()
            what = f"{shape} {dtname(dt)} trans={trans} nrhs={nrhs}"
            assert_bytes(got, refB, what)
            assert_bytes(Bn.host(), got, what + " without dres")
            assert_bytes(res.host(), refR, what + " dres")
            check_written(Bm, got)
            if not trans:
                check_written(res, res.host())
                if m == n:
                    assert float(res.view().abs().max()) == 0.0
            else:
                assert np.isnan(res.host()).all(), "TQR_TRANS writes no dres"


def test_lstsq_vs_numpy(tqr):
    """256 x 128, b = 128, fp64, batch 3, 5 right-hand sides, against numpy.linalg.lstsq per member with
    test_gpu_solve's bounds: |X - X_np|_F / |X_np|_F <= 1e-11 cond(A) and max|res - res_np| <= 1e-11 |B|_F.
    Through the one-shot tqr.lstsq_batched, which must also equal the handle's bytes."""
    import torch
    shape = (256, 128, 128)
    m, n, b = shape
    src = np.stack([inputs.matrix("gauss", shape, F64, i) for i in range(3)])  # (3, n, m)
    Bh = np.random.default_rng(7).standard_normal((3, 5, m))
    X, res, F, tau = tqr.lstsq_batched(torch.from_numpy(src).cuda(), torch.from_numpy(Bh).cuda(), b)
    torch.cuda.synchronize()
    lay = factored(tqr, shape, F64)
    assert same_bytes(F.cpu().numpy(), lay.mats().contiguous().cpu().numpy())
    Xh, rh = X.cpu().numpy(), res.cpu().numpy()
    for i in range(3):
        A64, B64 = src[i].T, Bh[i].T
        cond = float(np.linalg.cond(A64))
        Xn = np.linalg.lstsq(A64, B64, rcond=None)[0]
        rn = np.linalg.norm(A64 @ Xn - B64, axis=0)
        ex = float(np.linalg.norm(Xh[i].T - Xn) / np.linalg.norm(Xn))
        er = float(np.abs(rh[i] - rn).max())
        print(f"member {i}: cond(A) = {cond:.2f}, |X - X_np|_F / |X_np|_F = {ex:.3e}, max|res - res_np| = {er:.3e}")
        assert ex <= 1e-11 * cond
        assert er <= 1e-11 * float(np.linalg.norm(B64))


# ---- D. form_q -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", CASES, ids=ids(CASES))
def test_form_q_bytes_equal_apply_to_identity(tqr, shape, dt):
    """Thin (ncols = min(m, n)) and full (ncols = m) Q into a NaN-filled dQ: the bytes of tqr_apply_q
    (TQR_NOTRANS) per member on a buffer holding the first ncols columns of I_m."""
    import torch
    m, n, b = shape
    lay = factored(tqr, shape, dt, ldda=m + 3, strideA=n * (m + 3) + 5, strideTau=(min(m, n) // b) * m + 2)
    ba = prepared(tqr, lay)
    for ncols in sorted({min(m, n), m}):
        Q = Mat(m, ncols, dt, 3, ld=m + 2, stride=ncols * (m + 2) + 3)
        E = Q.buf.clone()
        Q.view(E).copy_(torch.eye(ncols, m, dtype=tdt(dt), device="cuda").expand(3, ncols, m))
        ref = ref_apply(tqr, lay, Q, False, buf=E)
        ba.form_q(lay.A[lay.base:], Q.buf[Q.base:], ncols=ncols, lddq=Q.ld, strideQ=Q.stride, **a_args(lay))
        got = Q.host()
        assert_bytes(got, ref, f"{shape} {dtname(dt)} ncols={ncols}")
        check_written(Q, got)


def test_form_q_meaning(tqr):
    """Member 1 of 3 (128 x 64, b = 32, fp64), the full Q: |Q^T Q - I| <= 1e-11 and |Q[:, :n] R - A| <=
    1e-11 * max(1, max|A|) (test_gpu_form_q.test_meaning's bounds), on contiguous tensors."""
    import torch
    shape = (128, 64, 32)
    m, n, b = shape
    lay = factored(tqr, shape, F64)
    ba = prepared(tqr, lay)
    F = lay.mats().contiguous()
    Q = torch.full((3, m, m), NAN, dtype=torch.float64, device="cuda")
    ba.form_q(F, Q)
    torch.cuda.synchronize()
    Qh, Fh, Ah = Q[1].cpu().numpy(), F[1].cpu().numpy(), inputs.matrix("gauss", shape, F64, 1)
    e_orth = float(np.abs(Qh @ Qh.T - np.eye(m)).max())
    R = np.tril(Fh[:, :n])  # array (j, i), i <= j: element (i, j) of R
    e_qr = float(np.abs(R @ Qh[:n] - Ah).max())
    print(f"member 1: max|Q^T Q - I| = {e_orth:.3e}, max|Q R - A| = {e_qr:.3e} (max|A| {np.abs(Ah).max():.3e})")
    assert e_orth <= 1e-11
    assert e_qr <= 1e-11 * max(1.0, float(np.abs(Ah).max()))


# ---- E. layouts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_odd_strides_offset_bases(tqr, dt):
    """Padded ldda / lddc, odd stacked strides beyond their minima, every base offset by an odd number of
    elements: apply both ways and lstsq with dres."""
    m, n, b = SMALL
    lay = factored(tqr, SMALL, dt, ldda=m + 5, strideA=n * (m + 5) + 11, strideTau=(n // b) * m + 13, base=3, tbase=5)
    assert lay.sA % 2 == 1 and lay.sT % 2 == 1
    ba = prepared(tqr, lay)
    for trans in (True, False):
        C = Mat(m, 5, dt, 3, ld=m + 4, stride=5 * (m + 4) + 7, base=9).fill()
        assert C.stride % 2 == 1
        ref = ref_apply(tqr, lay, C, trans)
        b_apply(ba, lay, C, trans)
        assert_bytes(C.host(), ref, f"trans={trans}")
    Bm = Mat(m, 5, dt, 3, ld=m + 4, stride=5 * (m + 4) + 7, base=9).fill()
    res = Mat(5, 1, dt, 3, stride=7, base=1)
    refB, refR = ref_lstsq(tqr, lay, Bm, False, res)
    b_lstsq(ba, lay, Bm, False, res)
    assert_bytes(Bm.host(), refB)
    assert_bytes(res.host(), refR)


@pytest.mark.parametrize("a_inter", [True, False], ids=["A-interleaved", "A-stacked"])
@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_row_interleaved(tqr, dt, a_inter):
    """C's members are row blocks of one array (strideC = m + 1 under lddc = 3 (m + 1) + 2), with A in the
    same form or stacked: apply both ways, lstsq, form_q."""
    m, n, b = SMALL
    kw = dict(ldda=3 * (m + 2) + 1, strideA=m + 2) if a_inter else dict(ldda=m + 1)
    lay = factored(tqr, SMALL, dt, **kw)
    ba = prepared(tqr, lay)
    ldc = 3 * (m + 1) + 2

    def inter(cols):
        return Mat(m, cols, dt, 3, ld=ldc, stride=m + 1, base=2)

    for trans in (True, False):
        C = inter(70).fill()
        ref = ref_apply(tqr, lay, C, trans)
        b_apply(ba, lay, C, trans)
        got = C.host()
        assert_bytes(got, ref, f"trans={trans}")
        check_written(C, got)
    for trans in (False, True):
        Bm = inter(5).fill()
        refB, _ = ref_lstsq(tqr, lay, Bm, trans)
        b_lstsq(ba, lay, Bm, trans)
        assert_bytes(Bm.host(), refB, f"lstsq trans={trans}")
    import torch
    Q = inter(n)
    E = Q.buf.clone()
    Q.view(E).copy_(torch.eye(n, m, dtype=tdt(dt), device="cuda").expand(3, n, m))
    ref = ref_apply(tqr, lay, Q, False, buf=E)
    ba.form_q(lay.A[lay.base:], Q.buf[Q.base:], ncols=n, lddq=Q.ld, strideQ=Q.stride, **a_args(lay))
    assert_bytes(Q.host(), ref, "form_q")


def test_batch_one(tqr):
    """Batch 1: the strides are ignored."""
    m, n, b = SMALL
    lay = factored(tqr, SMALL, F64, batch=1)
    ba = tqr.BatchedApply(m, n, b, tdt(F64), 1)
    ba.prepare(lay.A, lay.tau, ldda=m, strideA=-3, strideTau=(n // b) * m)
    C = Mat(m, 5, F64, 1).fill()
    ref = ref_apply(tqr, lay, C, True)
    ba.apply(lay.A, C.buf, nrhs=5, ldda=m, lddc=m, strideA=0, strideC=-7)
    assert_bytes(C.host(), ref)


# ---- F. member independence ----------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_member_independence(tqr, dt):
    """Member 1's C is all NaN: the other members' bytes equal those of the run without it."""
    m, n, b = SMALL
    lay = factored(tqr, SMALL, dt)
    ba = prepared(tqr, lay)
    for trans in (True, False):
        C, D = Mat(m, 70, dt, 3).fill(), Mat(m, 70, dt, 3).fill()
        D.view()[1] = NAN
        b_apply(ba, lay, C, trans)
        b_apply(ba, lay, D, trans)
        c, d = C.view().cpu().numpy(), D.view().cpu().numpy()
        assert same_bytes(c[0], d[0]) and same_bytes(c[2], d[2])
        assert np.isfinite(c).all() and np.isnan(d[1]).all()


# ---- G. more members than a grid's y -------------------------------------------------------------
def test_more_members_than_a_grid_dimension(tqr):
    """65537 members of 16 x 16 (b = 16, fp64, nrhs 1), member i a copy of member i mod 7: two launches
    per kernel. Members 0 .. 6 against the per-member calls, every member against member i mod 7."""
    import torch
    shape, nb = (16, 16, 16), 65537
    seven = factored(tqr, shape, F64, batch=7)
    idx = torch.arange(nb, device="cuda") % 7
    A = seven.mats().contiguous()[idx].contiguous()   # (nb, 16, 16)
    tau = seven.taus().contiguous()[idx].contiguous()  # (nb, 1, 16)
    C7 = Mat(16, 1, F64, 7).fill()
    ba = tqr.BatchedApply(16, 16, 16, torch.float64, nb)
    ba.prepare(A, tau)

    def same_as_first_seven(T):
        v = T.reshape(nb, -1).view(torch.int64)
        return bool(torch.equal(v, v[:7][idx]))

    # apply
    ref = C7.view(torch.from_numpy(ref_apply(tqr, seven, C7, True))).contiguous().numpy()
    C = C7.view().contiguous()[idx].contiguous()  # (nb, 1, 16)
    ba.apply(A, C, trans=True)
    torch.cuda.synchronize()
    assert same_bytes(C[:7].cpu().numpy(), ref)
    assert same_as_first_seven(C)
    # lstsq, both directions
    for trans in (False, True):
        res7 = Mat(1, 1, F64, 7)
        refB, refR = ref_lstsq(tqr, seven, C7, trans, res7)
        refB = C7.view(torch.from_numpy(refB)).contiguous().numpy()
        Bm = C7.view().contiguous()[idx].contiguous()
        res = torch.full((nb, 1), NAN, dtype=torch.float64, device="cuda")
        ba.lstsq(A, Bm, trans=trans, res=res)
        torch.cuda.synchronize()
        assert same_bytes(Bm[:7].cpu().numpy(), refB), f"trans={trans}"
        assert same_as_first_seven(Bm)
        assert same_bytes(res[:7].cpu().numpy().ravel(), refR[:7])
        assert same_as_first_seven(res)
    # the solve alone
    X = C7.view().contiguous()[idx].contiguous()
    tqr.trsm_r_batched(A, X, 16)
    torch.cuda.synchronize()
    assert same_bytes(X[:7].cpu().numpy(), C7.view(torch.from_numpy(ref_trsm(tqr, seven, C7, False))).contiguous().numpy())
    assert same_as_first_seven(X)


# ---- H. ordering ---------------------------------------------------------------------------------
def test_inputs_written_on_side_stream(tqr):
    """The factorisation and C are copied into place on a side stream; prepare and apply follow on that
    stream with no host synchronisation in between."""
    import torch
    m, n, b = SMALL
    src = factored(tqr, SMALL, F64, ldda=m + 1)
    Csrc = Mat(m, 5, F64, 3).fill()
    ref = ref_apply(tqr, src, Csrc, True)
    dst, C = Layout(SMALL, F64, 3, ldda=m + 1), Mat(m, 5, F64, 3)
    ba = tqr.BatchedApply(m, n, b, torch.float64, 3)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dst.A.copy_(src.A, non_blocking=True)
        dst.tau.copy_(src.tau, non_blocking=True)
        C.buf.copy_(Csrc.buf, non_blocking=True)
        ba.prepare(dst.A, dst.tau, stream=s, **a_args(dst))
        b_apply(ba, dst, C, True, stream=s)
    assert_bytes(C.host(), ref)


def test_ten_calls_alternating_streams(tqr):
    """10 applies on one handle, back to back on two alternating streams, each on its own C."""
    import torch
    m = SMALL[0]
    lay = factored(tqr, SMALL, F64)
    ba = prepared(tqr, lay)
    Cs = [Mat(m, 70, F64, 3).fill(x % 4) for x in range(10)]
    refs = [ref_apply(tqr, lay, Cs[x], True) for x in range(4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for x, C in enumerate(Cs):
        b_apply(ba, lay, C, True, stream=streams[x % 2])
    for x, C in enumerate(Cs):
        assert_bytes(C.host(), refs[x % 4], f"apply {x}")


def test_two_threads_share_one_handle(tqr):
    """Two host threads, each with its own stream and buffers, 4 calls each (apply and lstsq) on one handle."""
    import torch
    m = SMALL[0]
    lay = factored(tqr, SMALL, F64)
    ba = prepared(tqr, lay)
    Cs = [[Mat(m, 5, F64, 3).fill(t) for _ in range(4)] for t in range(2)]
    refs = [[ref_apply(tqr, lay, Cs[t][0], True), ref_lstsq(tqr, lay, Cs[t][0], False)[0]] for t in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    errors = []
    torch.cuda.synchronize()

    def work(t):
        try:
            for x, C in enumerate(Cs[t]):
                if x % 2 == 0:
                    b_apply(ba, lay, C, True, stream=streams[t])
                else:
                    b_lstsq(ba, lay, C, False, stream=streams[t])
            streams[t].synchronize()
        except Exception as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for x, C in enumerate(Cs[t]):
            assert_bytes(C.host(), refs[t][x % 2], f"thread {t}, call {x}")


def test_prepare_between_two_applies(tqr):
    """apply on factorisation 1, prepare on factorisation 2, apply on it — three streams, no host
    synchronisation: each apply sees the T images of its own factorisation."""
    import torch
    m, n, b = SMALL
    one, two = factored(tqr, SMALL, F64), factored(tqr, SMALL, F64, offset0=10)
    C1, C2 = Mat(m, 70, F64, 3).fill(1), Mat(m, 70, F64, 3).fill(1)
    ref1, ref2 = ref_apply(tqr, one, C1, True), ref_apply(tqr, two, C2, True)
    assert not same_bytes(ref1, ref2)
    s = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    ba = prepared(tqr, one, stream=s[0])
    b_apply(ba, one, C1, True, stream=s[1])
    ba.prepare(two.A, two.tau, stream=s[2], **a_args(two))
    b_apply(ba, two, C2, True, stream=s[0])
    assert_bytes(C1.host(), ref1, "the apply before the second prepare")
    assert_bytes(C2.host(), ref2, "the apply after it")


# ---- I. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_buffers_untouched(tqr):
    """Every call before the first prepare, then bad strides, leading dimensions, widths and trans with
    live device buffers: TQR_EINVAL, and not a byte of C changes. The handle still works afterwards."""
    import torch
    m, n, b = SMALL
    lay = factored(tqr, SMALL, F64, ldda=m + 2)
    C = Mat(m, 5, F64, 3, ld=m + 2).fill()
    before = C.host()
    res = torch.full((3 * 5,), NAN, dtype=torch.float64, device="cuda")
    L = tqr.lib()
    ba = tqr.BatchedApply(m, n, b, torch.float64, 3)
    pA, pT, pC, pR = P(lay.A.data_ptr()), P(lay.tau.data_ptr()), P(C.buf.data_ptr()), P(res.data_ptr())
    ld, sA, sC, sT = m + 2, n * (m + 2), 5 * (m + 2), (n // b) * m
    # before the first prepare
    assert L.tqr_batch_apply_q(ba.h, 1, pA, ld, sA, pC, 5, ld, sC, None) == TQR_EINVAL
    assert L.tqr_batch_form_q(ba.h, pA, ld, sA, pC, 5, ld, sC, None) == TQR_EINVAL
    assert L.tqr_batch_lstsq(ba.h, 0, pA, ld, sA, pC, 5, ld, sC, pR, 5, None) == TQR_EINVAL
    with pytest.raises(tqr.TQRError):
        b_apply(ba, lay, C, True)
    assert L.tqr_batch_apply_prepare(ba.h, pA, ld, (n - 1) * ld + m - 1, pT, sT, None) == TQR_EINVAL
    assert L.tqr_batch_apply_prepare(ba.h, pA, ld, sA, pT, sT - 1, None) == TQR_EINVAL
    assert L.tqr_batch_apply_q(ba.h, 1, pA, ld, sA, pC, 5, ld, sC, None) == TQR_EINVAL, "a refused prepare prepares nothing"
    assert L.tqr_batch_apply_prepare(ba.h, pA, ld, sA, pT, sT, None) == 0
    bad = [
        dict(ldda=m - 1), dict(ldda=0), dict(ldda=8388608, sA=n * 8388608), dict(sA=(n - 1) * ld + m - 1), dict(sA=m),
        dict(sA=0), dict(sA=-sA), dict(lddc=m - 1), dict(lddc=0), dict(sC=4 * ld + m - 1), dict(sC=m), dict(sC=0),
        dict(nrhs=0), dict(nrhs=-5), dict(trans=2), dict(pA=None), dict(pC=None),
    ]
    ok = dict(trans=1, pA=pA, ldda=ld, sA=sA, pC=pC, nrhs=5, lddc=ld, sC=sC)
    for kw in bad:
        a = dict(ok, **kw)
        assert L.tqr_batch_apply_q(ba.h, a["trans"], a["pA"], a["ldda"], a["sA"], a["pC"], a["nrhs"], a["lddc"], a["sC"],
                                   None) == TQR_EINVAL, kw
        assert L.tqr_batch_lstsq(ba.h, a["trans"], a["pA"], a["ldda"], a["sA"], a["pC"], a["nrhs"], a["lddc"], a["sC"], pR, 5,
                                 None) == TQR_EINVAL, kw
        if "trans" not in kw:
            assert L.tqr_batch_form_q(ba.h, a["pA"], a["ldda"], a["sA"], a["pC"], a["nrhs"], a["lddc"], a["sC"],
                                      None) == TQR_EINVAL, kw
    # the solve's members are the leading n x n of A and n x 5 of C
    for kw in [dict(ldda=n - 1), dict(ldda=0), dict(sA=(n - 1) * ld + n - 1), dict(sA=n), dict(sA=0), dict(lddc=n - 1),
               dict(sC=4 * ld + n - 1), dict(sC=n), dict(sC=0), dict(nrhs=0), dict(trans=2), dict(pA=None), dict(pC=None)]:
        a = dict(ok, **kw)
        assert L.tqr_batch_trsm_r(1, a["trans"], n, b, 3, a["pA"], a["ldda"], a["sA"], a["pC"], a["nrhs"], a["lddc"], a["sC"],
                                  None) == TQR_EINVAL, kw
    assert L.tqr_batch_trsm_r(1, 0, n, b, 0, pA, ld, sA, pC, 5, ld, sC, None) == TQR_EINVAL, "batch < 1"
    assert L.tqr_batch_lstsq(ba.h, 0, pA, ld, sA, pC, 5, ld, sC, pR, 4, None) == TQR_EINVAL, "strideRes < nrhs"
    assert L.tqr_batch_form_q(ba.h, pA, ld, sA, pC, m + 1, ld, (m + 1) * ld, None) == TQR_EINVAL, "ncols > m"
    with pytest.raises(tqr.TQRError):
        b_apply(tqr.BatchedApply(m, n, b, torch.float32, 3), lay, C, True)  # the handle's dtype
    assert_bytes(C.host(), before, "after refused calls")
    assert torch.isnan(res).all()
    ref = ref_apply(tqr, lay, C, True)
    b_apply(ba, lay, C, True)
    assert_bytes(C.host(), ref)
