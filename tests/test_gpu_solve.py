"""tqr_trsm_r (X <- R^{-1} X / R^{-T} X with the R of a finished factorisation) and tqr_lstsq (both
gels directions on an apply handle), include/tqr.h "solve", on the GPU.

References (never the GPU). tqr_trsm_r: F is the oracle's factorisation of a RANDZO matrix, Y the first
n rows of another; the fp64 upper triangle of F is solved by numpy.linalg.solve, and the residual
op(R) x - y is formed in numpy.longdouble. tqr_lstsq: numpy.linalg.lstsq on the original matrix (the
factorisation itself runs on the GPU, TiledQR). All matrices are well conditioned (asserted), so a
wrong answer cannot hide behind conditioning. Conditioned and structured inputs, and leading dimensions
at the library's bound: tests/test_gpu_solve_inputs.py.

Tolerances (derived, not tuned; u = 2^-53 for fp64, 2^-24 for fp32 storage):
  backward, componentwise:  |op(R) x - y| <= n u (|op(R)| |x| + |y|) element by element — the
      substitution bound gamma_n (Higham, Accuracy and Stability, thm 8.5), which holds for any order of
      the sums, so also for this kernel's tile-blocked order; fp32 storage rounds x once per tile
      step, each rounding one more u per term of the same form;
  forward:  max|x - x_ref| <= 1e-11 max(1, max|x_ref|) (fp64), 1e-4 (fp32) — the project's bounds;
  tqr_lstsq:  |X - X_np|_F / |X_np|_F <= tol cond(A) and max|res - res_np| <= tol |B|_F with tol = 1e-11
      (fp64) / 1e-4 (fp32) — the rule of test_gpu_apply.py::test_lstsq_vs_numpy.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
# (m, n, b): one 32-row group per tile (b = 16: one 16-row group), 2, 4 and 8 groups, two tile rows of R
# in each, and a single tile
SHAPES = [(48, 32, 16), (96, 64, 32), (192, 128, 64), (384, 256, 128), (768, 512, 256), (1024, 256, 256)]
SHAPES32 = [(48, 32, 16), (96, 64, 32), (192, 128, 64), (384, 256, 128), (768, 512, 256)]
NRHS = [1, 17, 64, 80]  # one lane, a ragged wave, one full workgroup, two workgroups (the second ragged)
NMAX = max(NRHS)
CASES = [(s, np.float64) for s in SHAPES] + [(s, np.float32) for s in SHAPES32]
IDS = [f"{m}x{n}b{b}-{'f64' if dt == np.float64 else 'f32'}" for (m, n, b), dt in CASES]
TRANS = [False, True]
TIDS = ["R", "Rt"]

_cache = {}


def unit(dt):
    return 2.0 ** -53 if np.dtype(dt) == np.float64 else 2.0 ** -24


def problem(oracle, shape, dt):
    """(F, R, Y): the oracle's factorisation (n, m), its fp64 upper triangle as an n x n matrix, and
    the right-hand sides (NMAX, n). Computed once, read-only."""
    key = ("prob", shape, np.dtype(dt).name)
    if key not in _cache:
        m, n, b = shape
        A = oracle.randzo(m, n, dt, seed=11 + b)
        F, _ = oracle.factor(A, b)
        R = np.triu(F[:, :n].T.astype(np.float64))
        Y = np.ascontiguousarray(oracle.randzo(m, NMAX, dt, seed=23)[:, :n])
        cond = float(np.linalg.cond(R))
        assert cond < 20, cond
        for x in (F, R, Y):
            x.setflags(write=False)
        _cache[key] = (F, R, Y)
    return _cache[key]


def reference(oracle, shape, dt, trans):
    """op(R)^{-1} Y^T in fp64, n x NMAX (columns are independent: nrhs < NMAX takes a slice)."""
    key = ("ref", shape, np.dtype(dt).name, trans)
    if key not in _cache:
        _, R, Y = problem(oracle, shape, dt)
        X = np.linalg.solve(R.T if trans else R, Y.T.astype(np.float64))
        X.setflags(write=False)
        _cache[key] = X
    return _cache[key]


def gpu_solve(tqr, F, Y, b, trans, stream=None):
    """tqr.trsm_r on copies of host F (n, m) and Y (nrhs, n); returns the solved (nrhs, n) array."""
    import torch
    dF = torch.from_numpy(np.array(F)).cuda()  # (copies: the cached inputs are read-only)
    dX = torch.from_numpy(np.array(Y)).cuda()
    tqr.trsm_r(dF, dX, b, trans=trans, stream=stream)
    torch.cuda.synchronize()
    return dX.cpu().numpy()


def check_backward(got, R, Y, trans, dt, what=""):
    """got (nrhs, n): finite, and the componentwise backward rule of the module docstring (it holds at
    any condition number). Returns the largest ratio in units of u."""
    n = R.shape[0]
    u = unit(dt)
    ld = np.longdouble
    op = (R.T if trans else R).astype(ld)
    x, y = got.T.astype(ld), Y.T.astype(ld)
    resid = np.abs(op @ x - y)
    bound = np.abs(op) @ np.abs(x) + np.abs(y)
    nz = bound > 0  # (an all-zero row of the bound has a zero residual: asserted below with the rest)
    ratio = float((resid[nz] / (u * bound[nz])).max())  # in units of u; the rule is <= n
    print(f"{what} backward {ratio:.2f} u (allowed {n} u), max|x| {float(np.abs(got).max()):.3e}")
    assert np.all(np.isfinite(got))
    assert np.all(resid <= n * u * bound)
    return ratio


def check_solution(got, R, Y, Xref, trans, dt, what=""):
    """got (nrhs, n) against the two accuracy rules of the module docstring."""
    check_backward(got, R, Y, trans, dt, what)
    err = float(np.abs(got.T.astype(np.float64) - Xref).max())
    scale = max(1.0, float(np.abs(Xref).max()))
    print(f"{what} forward max|x - x_ref| = {err:.3e} (max|x_ref| {scale:.3e})")
    assert err <= (1e-11 if np.dtype(dt) == np.float64 else 1e-4) * scale


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_trsm_r_accuracy(tqr, oracle, shape, dt, trans, nrhs):
    F, R, Y = problem(oracle, shape, dt)
    Xref = reference(oracle, shape, dt, trans)
    got = gpu_solve(tqr, F, Y[:nrhs], shape[2], trans)
    assert got.shape == (nrhs, shape[1]) and got.dtype == np.dtype(dt)
    check_solution(got, R, Y[:nrhs], Xref[:, :nrhs], trans, dt)


@pytest.mark.parametrize("nrhs", [17, 80])
@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
def test_trsm_r_square_single_tile(tqr, oracle, trans, nrhs):
    """m = n = b = 256: R is the one tile of a factorisation with a single tile row. A square RANDZO
    matrix is not as well conditioned as the tall ones of problem() (cond(R) about 2e3, asserted below
    1e4 as in test_lstsq_square_residual_is_zero), which both rules of check_solution carry as they
    stand: cond u is about 2e-13 of the forward rule's 1e-11."""
    m = n = b = 256
    A = oracle.randzo(m, n, np.float64, seed=11 + b)
    F, _ = oracle.factor(A, b)
    R = np.triu(F.T)
    cond = float(np.linalg.cond(R))
    assert cond < 1e4, cond
    Y = np.ascontiguousarray(oracle.randzo(m, nrhs, np.float64, seed=23))
    Xref = np.linalg.solve(R.T if trans else R, Y.T)
    got = gpu_solve(tqr, F, Y, b, trans)
    check_solution(got, R, Y, Xref, trans, np.float64, f"cond {cond:.0f}:")


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("shape,dt", [((96, 64, 32), np.float64), ((768, 512, 256), np.float64), ((192, 128, 64), np.float32)],
                         ids=["96x64b32-f64", "768x512b256-f64", "192x128b64-f32"])
def test_v_below_the_diagonal_is_ignored(tqr, oracle, shape, dt, trans):
    """F as factorised, its upper triangle alone (zeros below the diagonal), and NaN below the diagonal
    of every diagonal tile give three bit-identical results."""
    m, n, b = shape
    F, _, Y = problem(oracle, shape, dt)
    i, j = np.arange(m)[None, :], np.arange(n)[:, None]  # F[j, i] is element (i, j)
    Fz = np.where(i > j, 0.0, F).astype(dt)
    Fn = F.copy()
    Fn[(i > j) & (i // b == j // b)] = np.nan
    assert np.isnan(Fn).sum() == (n // b) * b * (b - 1) // 2
    nrhs = 17
    ref = gpu_solve(tqr, F, Y[:nrhs], b, trans)
    assert np.all(np.isfinite(ref))
    assert np.array_equal(gpu_solve(tqr, Fz, Y[:nrhs], b, trans), ref)
    assert np.array_equal(gpu_solve(tqr, Fn, Y[:nrhs], b, trans), ref)


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
def test_strip_independence_and_determinism(tqr, oracle, trans):
    """The first 17 columns of an nrhs = 80 solve equal an nrhs = 17 solve, and two identical calls
    are equal, bit for bit."""
    shape = (192, 128, 64)
    F, _, Y = problem(oracle, shape, np.float64)
    o80 = gpu_solve(tqr, F, Y, shape[2], trans)
    o17 = gpu_solve(tqr, F, Y[:17], shape[2], trans)
    again = gpu_solve(tqr, F, Y, shape[2], trans)
    assert np.array_equal(o80[:17], o17)
    assert np.array_equal(o80, again)


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
def test_padding_and_inputs_untouched(tqr, oracle, trans):
    """ldda = m + 8, lddx = n + 3, X allocated with 16 extra columns: rows >= n and columns >= nrhs
    keep their sentinels, dA is bit-identical after the call, and the result is right."""
    import torch
    shape, nrhs = (192, 128, 64), 17
    m, n, b = shape
    F, R, Y = problem(oracle, shape, np.float64)
    Fp = np.full((n, m + 8), -7.5)
    Fp[:, :m] = F
    Xp = np.full((nrhs + 16, n + 3), 1234.5)
    Xp[:nrhs, :n] = Y[:nrhs]
    dF, dX = torch.from_numpy(Fp).cuda(), torch.from_numpy(Xp).cuda()
    F0 = dF.clone()
    tqr.trsm_r(dF, dX, b, trans=trans, n=n, nrhs=nrhs, ldda=m + 8, lddx=n + 3)
    torch.cuda.synchronize()
    out = dX.cpu().numpy()
    assert torch.equal(dF, F0)
    assert np.all(out[nrhs:] == 1234.5) and np.all(out[:, n:] == 1234.5)
    check_solution(out[:nrhs, :n], R, Y[:nrhs], reference(oracle, shape, np.float64, trans)[:, :nrhs], trans, np.float64)
    # the padded call computes what the packed call computes
    assert np.array_equal(out[:nrhs, :n], gpu_solve(tqr, F, Y[:nrhs], b, trans))


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
def test_non_default_stream_same_bits(tqr, oracle, trans):
    import torch
    shape = (384, 256, 128)
    F, _, Y = problem(oracle, shape, np.float64)
    ref = gpu_solve(tqr, F, Y, shape[2], trans)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = gpu_solve(tqr, F, Y, shape[2], trans, stream=s)
    assert np.array_equal(got, ref)


# ---- tqr_lstsq --------------------------------------------------------------------------------
# (the last: a tall chain, 10 tile rows under each panel)
LSQ = [((768, 256, 128), np.float64), ((1024, 256, 256), np.float64), ((768, 512, 256), np.float64),
       ((192, 128, 64), np.float32), ((1280, 256, 128), np.float64)]
LSQ_IDS = [f"{m}x{n}b{b}-{'f64' if dt == np.float64 else 'f32'}" for (m, n, b), dt in LSQ]


def lsq_problem(tqr, oracle, shape, dt, ldda=None):
    """Host A (n, m), B (NMAX, m), cond(A), and the GPU factorisation: a prepared ApplyQ handle with the
    device F (n, ldda) and tau. The host parts are computed once."""
    import torch
    m, n, b = shape
    key = ("lsq", shape, np.dtype(dt).name)
    if key not in _cache:
        A = oracle.randzo(m, n, dt, seed=7)
        B = oracle.randzo(m, NMAX, dt, seed=8)
        cond = float(np.linalg.cond(A.T.astype(np.float64)))
        assert cond < 20, cond
        A.setflags(write=False)
        B.setflags(write=False)
        _cache[key] = (A, B, cond)
    A, B, cond = _cache[key]
    ldda = ldda or m
    Ap = np.full((n, ldda), -7.5, dtype=dt)
    Ap[:, :m] = A
    dF = torch.from_numpy(Ap).cuda()
    tdt = torch.float64 if np.dtype(dt) == np.float64 else torch.float32
    dtau = torch.zeros((n // b, m), dtype=tdt, device="cuda")
    plan = tqr.TiledQR(m, n, b, tdt)
    plan.execute(dF, dtau, ldda=ldda)
    plan.status()
    ap = tqr.ApplyQ(m, n, b, tdt)
    ap.prepare(dF, dtau, ldda=ldda)
    return A, B, cond, ap, dF, dtau


def tol(dt):
    return 1e-11 if np.dtype(dt) == np.float64 else 1e-4


@pytest.mark.parametrize("nrhs", [3, 80])
@pytest.mark.parametrize("shape,dt", LSQ, ids=LSQ_IDS)
def test_lstsq_notrans_vs_numpy(tqr, oracle, shape, dt, nrhs):
    import torch
    m, n, b = shape
    A, B, cond, ap, dF, _ = lsq_problem(tqr, oracle, shape, dt)
    Bh = np.ascontiguousarray(B[:nrhs])
    dB = torch.from_numpy(Bh.copy()).cuda()
    dres = torch.full((nrhs,), -1.0, dtype=dB.dtype, device="cuda")
    ap.lstsq(dF, dB, res=dres)
    dQ = torch.from_numpy(Bh.copy()).cuda()
    ap.apply(dF, dQ, trans=True)  # what the apply alone leaves
    dN = torch.from_numpy(Bh.copy()).cuda()
    ap.lstsq(dF, dN)  # res = None
    torch.cuda.synchronize()
    out, res = dB.cpu().numpy(), dres.cpu().numpy().astype(np.float64)
    assert np.array_equal(out[:, n:], dQ.cpu().numpy()[:, n:])
    assert np.array_equal(dN.cpu().numpy(), out)
    A64, B64 = A.T.astype(np.float64), Bh.T.astype(np.float64)
    Xn = np.linalg.lstsq(A64, B64, rcond=None)[0]  # n x nrhs
    rn = np.linalg.norm(A64 @ Xn - B64, axis=0)
    ex = float(np.linalg.norm(out[:, :n].T.astype(np.float64) - Xn) / np.linalg.norm(Xn))
    er = float(np.abs(res - rn).max())
    print(f"cond(A) = {cond:.2f}, |X - X_np|_F / |X_np|_F = {ex:.3e}, max|res - res_np| = {er:.3e}")
    assert ex <= tol(dt) * cond
    assert er <= tol(dt) * float(np.linalg.norm(B64))


@pytest.mark.parametrize("nrhs", [3, 80])
@pytest.mark.parametrize("shape,dt", LSQ, ids=LSQ_IDS)
def test_lstsq_trans_minimum_norm_vs_numpy(tqr, oracle, shape, dt, nrhs):
    """A^T x = c: the minimum-norm x against numpy's, A^T x against c, and NaN in rows n .. m-1 of the
    array on entry (they are ignored and zeroed) does not reach the result."""
    import torch
    m, n, b = shape
    A, B, cond, ap, dF, _ = lsq_problem(tqr, oracle, shape, dt)
    Ch = np.ascontiguousarray(B[:nrhs, :n])  # c: n x nrhs
    Bh = np.full((nrhs, m), np.nan, dtype=dt)
    Bh[:, :n] = Ch
    dB = torch.from_numpy(Bh).cuda()
    ap.lstsq(dF, dB, trans=True)
    torch.cuda.synchronize()
    x = dB.cpu().numpy().T.astype(np.float64)  # m x nrhs
    assert np.all(np.isfinite(x))
    At64, C64 = A.astype(np.float64), Ch.T.astype(np.float64)  # A^T is (n, m) as stored
    Xn = np.linalg.lstsq(At64, C64, rcond=None)[0]  # minimum norm, m x nrhs
    ex = float(np.linalg.norm(x - Xn) / np.linalg.norm(Xn))
    ec = float(np.abs(At64 @ x - C64).max())
    print(f"cond(A) = {cond:.2f}, |x - x_np|_F / |x_np|_F = {ex:.3e}, max|A^T x - c| = {ec:.3e}")
    assert ex <= tol(dt) * cond
    assert ec <= tol(dt) * float(np.linalg.norm(C64))


def test_lstsq_square_residual_is_zero(tqr, oracle):
    """m == n: no residual rows, res is exactly 0 and X solves A X = B."""
    import torch
    m = n = 256
    b = 128
    A = oracle.randzo(m, n, np.float64, seed=7)
    cond = float(np.linalg.cond(A.T))
    assert cond < 1e4, cond
    dF = torch.from_numpy(A.copy()).cuda()
    dtau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
    tqr.TiledQR(m, n, b, torch.float64).execute(dF, dtau)
    ap = tqr.ApplyQ(m, n, b, torch.float64)
    ap.prepare(dF, dtau)
    B = oracle.randzo(m, 5, np.float64, seed=8)
    dB = torch.from_numpy(B.copy()).cuda()
    dres = torch.full((5,), -1.0, dtype=torch.float64, device="cuda")
    ap.lstsq(dF, dB, res=dres)
    torch.cuda.synchronize()
    assert np.all(dres.cpu().numpy() == 0.0)
    Xn = np.linalg.solve(A.T, B.T)
    ex = float(np.linalg.norm(dB.cpu().numpy().T - Xn) / np.linalg.norm(Xn))
    print(f"cond(A) = {cond:.2f}, |X - X_np|_F / |X_np|_F = {ex:.3e}")
    assert ex <= 1e-11 * cond


@pytest.mark.parametrize("trans", [False, True], ids=["ls", "minnorm"])
def test_lstsq_padded_leading_dimensions(tqr, oracle, trans):
    """ldda = m + 8, lddb = m + 3, B allocated with 4 extra columns: the same bits as the packed call,
    sentinels intact."""
    import torch
    shape, nrhs = (768, 256, 128), 3
    m, n, b = shape
    A, B, _, ap, dF, _ = lsq_problem(tqr, oracle, shape, np.float64)
    dB = torch.from_numpy(np.array(B[:nrhs])).cuda()
    dres = torch.zeros((nrhs,), dtype=torch.float64, device="cuda")
    ap.lstsq(dF, dB, trans=trans, res=dres)
    _, _, _, ap2, dF2, _ = lsq_problem(tqr, oracle, shape, np.float64, ldda=m + 8)
    Bp = np.full((nrhs + 4, m + 3), 1234.5)
    Bp[:nrhs, :m] = B[:nrhs]
    dBp = torch.from_numpy(Bp).cuda()
    dres2 = torch.zeros((nrhs,), dtype=torch.float64, device="cuda")
    ap2.lstsq(dF2, dBp, trans=trans, nrhs=nrhs, ldda=m + 8, lddb=m + 3, res=dres2)
    torch.cuda.synchronize()
    out = dBp.cpu().numpy()
    assert np.all(out[nrhs:] == 1234.5) and np.all(out[:, m:] == 1234.5)
    assert np.array_equal(out[:nrhs, :m], dB.cpu().numpy())
    assert torch.equal(dres, dres2)


def test_lstsq_error_cases(tqr, oracle):
    """TQR_EINVAL: before the first prepare, on a handle with m < n, and for bad arguments on a live
    handle."""
    import torch
    L = tqr.lib()
    m, n, b = 768, 256, 128
    _, _, _, ap, dF, dtau = lsq_problem(tqr, oracle, (m, n, b), np.float64)
    dB = torch.zeros((4, m), dtype=torch.float64, device="cuda")
    a, c = P(dF.data_ptr()), P(dB.data_ptr())
    fresh = tqr.ApplyQ(m, n, b, torch.float64)
    assert L.tqr_lstsq(fresh.h, 0, a, m, c, 4, m, None, None) == -1  # before the first prepare
    with pytest.raises(tqr.TQRError):
        fresh.lstsq(dF, dB)
    wide = tqr.ApplyQ(256, 384, 128, torch.float64)  # m < n
    wF = torch.zeros((384, 256), dtype=torch.float64, device="cuda")
    wtau = torch.zeros((2, 256), dtype=torch.float64, device="cuda")
    tqr.TiledQR(256, 384, 128, torch.float64).execute(wF, wtau)
    wide.prepare(wF, wtau)
    wB = torch.zeros((4, 256), dtype=torch.float64, device="cuda")
    for tr in (0, 1):
        assert L.tqr_lstsq(wide.h, tr, P(wF.data_ptr()), 256, P(wB.data_ptr()), 4, 256, None, None) == -1
    assert L.tqr_lstsq(ap.h, 0, a, m, c, 0, m, None, None) == -1       # nrhs < 1
    assert L.tqr_lstsq(ap.h, 2, a, m, c, 4, m, None, None) == -1       # trans not 0 / 1
    assert L.tqr_lstsq(ap.h, 0, None, m, c, 4, m, None, None) == -1
    assert L.tqr_lstsq(ap.h, 0, a, m, None, 4, m, None, None) == -1
    assert L.tqr_lstsq(ap.h, 0, a, m, c, 4, m - 1, None, None) == -1   # lddb < m
    assert L.tqr_lstsq(ap.h, 1, a, m, c, 4, m - 1, None, None) == -1
    assert L.tqr_lstsq(ap.h, 0, a, m - 1, c, 4, m, None, None) == -1   # ldda < m
    torch.cuda.synchronize()
    assert torch.all(dB == 0)  # none of the rejected calls wrote anything
