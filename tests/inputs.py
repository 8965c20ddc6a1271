"""Inputs beyond RANDZO and an extended-precision reference, shared by test_gpu_inputs.py (GPU)
and test_inputs_cpu.py (the same conditions on the oracle alone), and the references of the apply,
the solve and least squares shared by test_gpu_apply.py, test_gpu_solve_inputs.py (GPU) and
test_solve_inputs_cpu.py. Plain numpy (and, for oracle_qt, the oracle's tile kernels).

Array convention as everywhere here: a column-major m x n matrix is an (n, m) array, row j of the
array = matrix column j. Seeds are fixed: default_rng(1000 + m + n + b) (+ a stated offset where a
second, independent matrix of the same shape is needed).
"""
import ctypes

import numpy as np

P = ctypes.c_void_p
# (m, n, b): the smallest shapes at which each mechanism exists — one reflector group per tile; two;
# four; the production tile (8 groups); wide (kmax = p); a TS chain of 9 under one panel. Under the
# default knobs fp64 storage runs that chain one TSMQR per task (flowplan.cpp default_tail: every step
# of a plan of at most 32 tile rows is a tail step), not as the segments of 8 and 1 it was chosen for:
# those run under TQR_TAIL=0 as case T0-128 of tests/segments.py (test_gpu_segments.py)
SHAPES = [(96, 64, 32), (192, 128, 64), (384, 256, 128), (768, 512, 256), (256, 384, 128), (1280, 256, 128)]
SHAPES32 = [(192, 128, 64), (768, 512, 256)]
ACC_SHAPES = [(192, 128, 64), (768, 512, 256)]
FAMILIES = ["gauss", "rowgraded", "cond1e8"]
# the wave engine's shapes (test_gpu_waves.py), both dtypes at each: 4 x 4, 4 x 4, 4 x 3, 4 x 3 and 3 x 3
# tiles and a wide 2 x 4. Every tile size, so k_update's strip counts 1, 1, 1, 2, 4 and the reflector-group
# counts 1, 1, 2, 4, 8; p, q >= 3 (all but the wide one) puts the panel tasks of step k+1 into one wave
# with update tasks of step k. The smallest shapes with those properties.
WAVE_SHAPES = [(64, 64, 16), (128, 128, 32), (256, 192, 64), (512, 384, 128), (768, 768, 256), (128, 256, 64)]
WAVE_ACC_SHAPES = [(64, 64, 16), (256, 192, 64), (768, 768, 256)]
WAVE_ACC_SHAPES32 = [(256, 192, 64), (768, 768, 256)]
KMAX = {np.dtype(np.float64): 400, np.dtype(np.float32): 30}  # column exponents of scaling()
# shapes of the apply / solve tests on these inputs (test_gpu_solve_inputs.py and its CPU twin)
SOLVE_CASES = [((96, 64, 32), np.float64), ((192, 128, 64), np.float64), ((768, 512, 256), np.float64),
               ((192, 128, 64), np.float32)]
APPLY_FAMILIES = FAMILIES + ["structured"]
ZERO_COL = 5  # the zero column of matrix("structured")
# right-hand-side exponents of the fp32 least-squares calls: 2^+-80 times entries of 0.01 .. 10 are
# normal floats (1e-26 .. 1e25) whose squares (1e-52 .. 1e50) are not
KMAX_RES32 = 80
# e_gpu <= LSQ_MARGIN * max(e_oracle_path, e_numpy) in the conditioned least-squares tests: twice the
# largest spread between the two CPU solvers, rounded up (measured by test_solve_inputs_cpu.py)
LSQ_MARGIN = 6

_cache = {}


def _frozen(key, make):
    """make() once per key; the arrays are shared between tests and therefore read-only."""
    if key not in _cache:
        out = make()
        for x in (out if isinstance(out, tuple) else (out,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def dtname(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


def rng_for(shape, offset=0):
    m, n, b = shape
    return np.random.default_rng(1000 + m + n + b + offset)


def matrix(family, shape, dt=np.float64, offset=0):
    """The input of `family` at `shape`, (n, m) of dtype dt (read-only, cached).
    gauss: standard normal (cond ~ 10). rowgraded: standard normal, matrix row i times
    2^(-40 i / (m - 1)) (cond ~ 1e7 .. 1e9). cond1e8: U diag(logspace(0, -8, n)) V^T with U, V
    from numpy's QR of normal matrices. structured: standard normal with the 32 columns n/2 .. n/2+31
    zero except a 1 in row j of column j, then column ZERO_COL zero and column n/2+6 a copy of
    column 3 (n >= 64): reflectors with tau == 2 and an R with exactly zero diagonal entries."""
    def make():
        m, n, _ = shape
        rng = rng_for(shape, offset)
        if family == "gauss":
            A = rng.standard_normal((n, m))
        elif family == "rowgraded":
            A = rng.standard_normal((n, m)) * np.exp2(-40.0 * np.arange(m) / (m - 1))[None, :]
        elif family == "cond1e8":
            assert m >= n
            U = np.linalg.qr(rng.standard_normal((m, n)))[0]
            V = np.linalg.qr(rng.standard_normal((n, n)))[0]
            A = np.ascontiguousarray(((U * np.logspace(0, -8, n)[None, :]) @ V.T).T)
        elif family == "structured":
            A = rng.standard_normal((n, m))
            c0 = n // 2
            A[c0:c0 + 32] = 0.0
            A[np.arange(c0, c0 + 32), np.arange(c0, c0 + 32)] = 1.0
            A[ZERO_COL] = 0.0
            A[c0 + 6] = A[3]
        else:
            raise ValueError(family)
        return np.ascontiguousarray(A, dtype=dt)
    return _frozen(("A", family, shape, np.dtype(dt).name, offset), make)


def scaling(shape, dt):
    """d_j = s_j 2^(k_j): s_j = +-1, k_j uniform in [-KMAX, KMAX] per column, exact in dt."""
    def make():
        n = shape[1]
        rng = rng_for(shape, 1)
        kmax = KMAX[np.dtype(dt)]
        k = rng.integers(-kmax, kmax + 1, size=n)
        s = rng.choice([-1.0, 1.0], size=n)
        return (s * np.ldexp(1.0, k)).astype(dt)
    return _frozen(("D", shape, np.dtype(dt).name), make)


def scale_columns(A, d):
    """A D for D = diag(d): exact while nothing leaves the normal range."""
    out = A * np.asarray(d, dtype=A.dtype).reshape(-1, 1)
    assert out.dtype == A.dtype
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def covariance_mismatches(F, T, Fs, Ts, d):
    """factor(A D) = (R D, V, tau) bit for bit: the counts of differing (tau, V, R) entries of the
    scaled result (Fs, Ts) against the unscaled (F, T). V: strictly below the global diagonal;
    R: on or above it, column j times d_j."""
    n, m = F.shape
    below = np.arange(m)[None, :] > np.arange(n)[:, None]  # matrix row i > column j
    want = np.where(below, F, scale_columns(F, d))
    diff = bits(want) != bits(Fs)
    return int((bits(T) != bits(Ts)).sum()), int((diff & below).sum()), int((diff & ~below).sum())


def assert_covariant(F, T, Fs, Ts, d):
    assert np.isfinite(Fs).all() and np.isfinite(Ts).all()
    nt, nv, nr = covariance_mismatches(F, T, Fs, Ts, d)
    print(f"scaling covariance: differing entries tau {nt}, V {nv}, R {nr}")
    assert nt == 0, f"{nt} tau entries are not bit-identical under column scaling"
    assert nv == 0, f"{nv} V entries are not bit-identical under column scaling"
    assert nr == 0, f"{nr} R entries differ from R[:, j] * d_j"


def have_longdouble():
    return np.finfo(np.longdouble).eps <= 2.0 ** -63


def qr_longdouble(A):
    """R (n x n, upper) of a plain Householder QR of the m x n matrix (m >= n), column by column in
    numpy.longdouble. R's row signs are this routine's own: compare |R|."""
    W = np.array(A.T, dtype=np.longdouble)
    m, n = W.shape
    assert m >= n
    for j in range(n):
        x = W[j:, j]
        nrm = np.sqrt(x @ x)
        if nrm == 0:
            continue
        alpha = -nrm if x[0] >= 0 else nrm
        v = x.copy()
        v[0] -= alpha
        W[j:, j + 1:] -= np.outer(v, (2 / (v @ v)) * (v @ W[j:, j + 1:]))
        W[j, j] = alpha
        W[j + 1:, j] = 0
    return np.triu(W[:n])


def r_longdouble(family, shape):
    return _frozen(("Rld", family, shape), lambda: qr_longdouble(matrix(family, shape)))


def r_of(F):
    """R (min(m, n) rows) of a factorised (n, m) array as a matrix."""
    n, m = F.shape
    return np.triu(F.T[:min(m, n)])


def col_rel_err(F, R_ld):
    """e = max_j max_i | |R| - |R_ld| |[i, j] / ||R_ld[:, j]||."""
    R = r_of(F).astype(np.longdouble)
    cn = np.sqrt((R_ld * R_ld).sum(axis=0))
    return float((np.abs(np.abs(R) - np.abs(R_ld)) / cn[None, :]).max())


def colnorm_rel_err(A, F):
    """max_j | ||A[:, j]|| - ||R[:, j]|| | / ||A[:, j]||."""
    na = np.linalg.norm(A.astype(np.float64), axis=1)
    nr = np.linalg.norm(r_of(F).astype(np.float64), axis=0)
    return float((np.abs(na - nr) / na).max())


def oracle_factor(oracle, family, shape, dt=np.float64, offset=0):
    """(F, T) of the oracle's factorisation of matrix(family, shape, dt, offset), cached."""
    return _frozen(("F", family, shape, np.dtype(dt).name, offset),
                   lambda: oracle.factor(matrix(family, shape, dt, offset), shape[2]))


# ---- the apply's references (shared by test_gpu_apply.py, test_gpu_solve_inputs.py and its CPU twin) ----
def oracle_qt(oracle, F, T, C, b):
    """Q^T C by the oracle's tile kernels: [F | C] in one array of leading dimension m, C padded to
    whole b-column blocks, the factorisation's order block column by block column."""
    n, m = F.shape
    nrhs = C.shape[0]
    p, q = m // b, n // b
    kmax = min(p, q)
    nb = (nrhs + b - 1) // b
    W = np.zeros((n + nb * b, m), dtype=F.dtype)
    W[:n] = F
    W[n:n + nrhs] = C
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
    return W[n:n + nrhs].copy()


def reflectors(F, T, b):
    """The factorisation's reflectors in application order: (rows, v, tau) with v over `rows`."""
    n, m = F.shape
    p, q = m // b, n // b
    out = []
    for k in range(min(p, q)):
        for c in range(b):
            d = k * b + c
            rows = np.arange(d, (k + 1) * b)
            v = F[d, rows].copy()
            v[0] = 1.0
            out.append((rows, v, T[k * b, d]))
        for l in range(k + 1, p):
            for c in range(b):
                d = k * b + c
                rows = np.concatenate(([d], np.arange(l * b, (l + 1) * b)))
                v = np.concatenate(([1.0], F[d, l * b:(l + 1) * b])).astype(F.dtype)
                out.append((rows, v, T[k * b, l * b + c]))
    return out


def numpy_q(F, T, C, b):
    """Q C: the reflectors I - tau v v^T one by one in reverse, in the arrays' own precision."""
    C = C.copy()
    for rows, v, tau in reversed(reflectors(F, T, b)):
        w = C[:, rows] @ v
        C[:, rows] -= np.outer(tau * w, v)
    return C


def numpy_qt(F, T, C, b):
    """Q^T C: the same reflectors one by one in the factorisation's order."""
    C = C.copy()
    for rows, v, tau in reflectors(F, T, b):
        w = C[:, rows] @ v
        C[:, rows] -= np.outer(tau * w, v)
    return C


# ---- right-hand sides, substitution and the extended-precision least-squares solution ----------
def rhs_scaling(shape, dt, nrhs, kmax=None):
    """e_j = s_j 2^(k_j) per right-hand side: s_j = +-1, k_j uniform in [-kmax, kmax] (default
    KMAX[dt]) with k_0 = kmax and k_1 = -kmax (nrhs >= 2), exact in dt."""
    kmax = kmax or KMAX[np.dtype(dt)]

    def make():
        rng = rng_for(shape, 2)
        k = rng.integers(-kmax, kmax + 1, size=nrhs)
        k[:2] = [kmax, -kmax][:nrhs]
        s = rng.choice([-1.0, 1.0], size=nrhs)
        return (s * np.ldexp(1.0, k)).astype(dt)
    return _frozen(("E", shape, np.dtype(dt).name, nrhs, kmax), make)


def in_normal_range(x):
    """Every entry is finite and either zero or a normal number of its dtype."""
    a = np.abs(x)
    return bool(np.isfinite(x).all() and (a[a > 0] >= np.finfo(x.dtype).tiny).all())


def assert_scaled(out_s, out, e):
    """out_s[j] = e_j out[j] bit for bit, with nothing lost: all normal, no zero created."""
    assert in_normal_range(out_s) and in_normal_range(out)
    assert np.array_equal(out_s == 0, out == 0)
    bad = int((bits(out_s) != bits(scale_columns(out, e))).sum())
    assert bad == 0, f"{bad} entries differ from column j * e_j"


def upper(F, n=None):
    """R = the upper triangle of the leading n x n block of a factorised (>= n, m) array, as a matrix."""
    n = F.shape[0] if n is None else n
    return np.triu(F[:n, :n].T)


def subst(R, Y, trans=False):
    """X (nrhs, n) with op(R) X^T = Y^T by plain substitution in R's own dtype, dividing by the diagonal
    entries (no inverse, no pivoting, no check): the reference of tqr_trsm_r."""
    n = R.shape[0]
    X = np.array(Y, dtype=R.dtype)
    with np.errstate(all="ignore"):
        if trans:
            for j in range(n):
                X[:, j] = (X[:, j] - X[:, :j] @ R[:j, j]) / R[j, j]
        else:
            for j in range(n - 1, -1, -1):
                X[:, j] = (X[:, j] - X[:, j + 1:] @ R[j, j + 1:]) / R[j, j]
    return X


def backward_ratio(R, X, Y, trans, u):
    """max over the entries of |op(R) x - y| / (u (|op(R)| |x| + |y|)), the residual in
    numpy.longdouble: the componentwise substitution bound is `<= n`."""
    ld = np.longdouble
    op = (R.T if trans else R).astype(ld)
    x, y = X.T.astype(ld), Y.T.astype(ld)
    resid = np.abs(op @ x - y)
    bound = np.abs(op) @ np.abs(x) + np.abs(y)
    assert np.all(resid[bound == 0] == 0)
    nz = bound > 0
    return float((resid[nz] / (u * bound[nz])).max())


def lsq_rhs(family, shape, nrhs=5):
    """(nrhs, m) right-hand sides of the conditioned least-squares tests: standard normal (the same
    for every family of a shape), so max|x| is about cond(A) and the residual is of order |b|."""
    return _frozen(("B", shape, nrhs), lambda: rng_for(shape, 3).standard_normal((nrhs, shape[0])))


def lstsq_longdouble(A, B):
    """X (nrhs, n) minimising |A x - b| per right-hand side in numpy.longdouble: qr_longdouble on
    [A | B] gives [R11 R12; 0 R22], then R11 X = R12 by back substitution."""
    n = A.shape[0]
    R = qr_longdouble(np.concatenate([A, B], axis=0))
    return subst(R[:n, :n], np.ascontiguousarray(R[:n, n:].T))


def x_ld(family, shape):
    return _frozen(("Xld", family, shape), lambda: lstsq_longdouble(matrix(family, shape), lsq_rhs(family, shape)))


def rel_err(X, Xld):
    d = X.astype(np.longdouble) - Xld
    return float(np.sqrt((d * d).sum()) / np.sqrt((Xld * Xld).sum()))


def oracle_lstsq(oracle, F, T, B, b):
    """The fp64 reference path: Q^T B by the oracle's tile kernels, R X = rows 0 .. n-1 by subst(), and
    the 2-norm of rows n .. m-1. Returns (X (nrhs, n), res (nrhs,), Q^T B (nrhs, m))."""
    n = F.shape[0]
    QtB = oracle_qt(oracle, F, T, np.ascontiguousarray(B), b)
    return subst(upper(F), QtB[:, :n]), resnorm(QtB, n), QtB


def resnorm(QtB, n):
    """|rows n .. m-1| per column as tqr_lstsq defines it: squares summed in fp64, unscaled, the root
    rounded to the storage dtype."""
    t = QtB[:, n:].astype(np.float64)
    return np.sqrt((t * t).sum(axis=1)).astype(QtB.dtype)


def zero_diag_index(b):
    """The middle row of the middle 32-row group of the second tile row (b >= 32)."""
    return b + 32 * (b // 64) + 16


def poison_r(F):
    """F with NaN in every element on or above the global diagonal (matrix row i <= column j)."""
    n, m = F.shape
    Fn = F.copy()
    Fn[np.arange(m)[None, :] <= np.arange(n)[:, None]] = np.nan
    assert np.isnan(Fn).sum() == sum(min(j + 1, m) for j in range(n))
    return Fn
