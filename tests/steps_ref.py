"""References and bounds shared by test_steps_cpu.py and test_gpu_steps.py (capped plans,
tqr_plan_create_steps): the oracle's partial factorisation and the bounds copied from the tests of the
whole factorisation and of the solve. No GPU, no product code."""
import ctypes

import numpy as np

P = ctypes.c_void_p


def oracle_qt_cols(oracle, F, T, C, b):
    """Q^T C by the oracle's tile kernels (the tile-op loop of tests/test_gpu_apply.py::oracle_qt):
    [F | C] in one array of leading dimension m, the factorisation's order column by column. F, T
    (n, m): a factorisation and its m x n tau matrix; C (c, m) with c a multiple of b."""
    n, m = F.shape
    p, q = m // b, n // b
    kmax = min(p, q)
    nb = C.shape[0] // b
    assert nb * b == C.shape[0]
    W = np.zeros((n + nb * b, m), dtype=F.dtype)
    W[:n] = F
    W[n:] = C
    Tc = np.ascontiguousarray(T)
    es, wb, tb = W.itemsize, W.ctypes.data, Tc.ctypes.data
    sfx = oracle.sfx(F.dtype)
    unmqr, tsmqr = getattr(oracle.L, f"oracle_unmqr_{sfx}"), getattr(oracle.L, f"oracle_tsmqr_{sfx}")

    def tile(r, c):
        return P(wb + (c * b * m + r * b) * es)

    def taus(r, k):
        return P(tb + (k * b * m + r * b) * es)

    for j in range(q, q + nb):
        for k in range(kmax):
            unmqr(tile(k, j), tile(k, k), taus(k, k), b, b, m)
            for l in range(k + 1, p):
                tsmqr(tile(l, k), tile(k, j), tile(l, j), taus(l, k), b, b, m)
    return W[n:].copy()


def partial(oracle, A, b, s):
    """partial(A, s) = [oracle.factor(A[:, :s*b]) | oracle Q^T applied to A[:, s*b:]] as (F, T):
    (n, m) arrays, T the m x n tau matrix (zero in the columns >= s*b)."""
    n, m = A.shape
    F1, T1 = oracle.factor(np.ascontiguousarray(A[:s * b]), b)
    F = np.empty_like(A)
    T = np.zeros_like(A)
    F[:s * b], T[:s * b] = F1, T1
    if s * b < n:
        F[s * b:] = oracle_qt_cols(oracle, F1, T1, np.ascontiguousarray(A[s * b:]), b)
    return F, T


def expand_tau_steps(tau, m, n, b):
    """compact (steps, m) -> the m x n tau matrix as an (n, m) array (tqr.expand_tau for any cap)."""
    T = np.zeros((n, m), dtype=tau.dtype)
    for k in range(tau.shape[0]):
        T[k * b, k * b:] = tau[k, k * b:]
    return T


def assert_close(F, T, F_ref, T_ref):
    """tests/test_gpu_factor.py::assert_close (copied): the whole factorisation's bounds."""
    if F_ref.dtype == np.float64:
        s = max(1.0, float(np.abs(F_ref).max()))
        assert float(np.abs(F - F_ref).max()) <= 1e-11 * s
        assert float(np.abs(T - T_ref).max()) <= 1e-11 * 2
    else:
        assert float(np.abs(F.astype(np.float64) - F_ref).max()) <= 1e-3
        assert float(np.abs(T.astype(np.float64) - T_ref).max()) <= 1e-3


def tol(dt):
    """tests/test_gpu_solve.py::tol (copied)."""
    return 1e-11 if np.dtype(dt) == np.float64 else 1e-4


def check_apply(got, ref, ref64, what=""):
    """tests/test_gpu_apply.py::check (copied): the apply tests' bound on Q^T C."""
    g = got.astype(np.float64)
    err = float(np.abs(g - ref).max())
    scale = max(1.0, float(np.abs(ref).max()))
    if ref.dtype == np.float64:
        print(f"{what} max|GPU - ref| = {err:.3e} (max|ref| {scale:.3e})")
        assert err <= 1e-11 * scale
    else:
        e_gpu = float(np.abs(g - ref64).max())
        e_ref = float(np.abs(ref.astype(np.float64) - ref64).max())
        print(f"{what} max|GPU - ref32| = {err:.3e} (max|ref| {scale:.3e}); vs fp64: GPU {e_gpu:.3e}, ref32 {e_ref:.3e}")
        assert err <= 1e-4 * scale
        assert e_gpu <= 1.5 * e_ref
