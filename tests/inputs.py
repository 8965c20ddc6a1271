"""Inputs beyond RANDZO and an extended-precision reference, shared by test_gpu_inputs.py (GPU)
and test_inputs_cpu.py (the same conditions on the oracle alone). Plain numpy.

Array convention as everywhere here: a column-major m x n matrix is an (n, m) array, row j of the
array = matrix column j. Seeds are fixed: default_rng(1000 + m + n + b) (+ a stated offset where a
second, independent matrix of the same shape is needed).
"""
import numpy as np

# (m, n, b): the smallest shapes at which each mechanism exists — one reflector group per tile; two;
# four; the production tile (8 groups); wide (kmax = p); a TS chain of 9 under one panel (more than
# one default chain segment of 8)
SHAPES = [(96, 64, 32), (192, 128, 64), (384, 256, 128), (768, 512, 256), (256, 384, 128), (1280, 256, 128)]
SHAPES32 = [(192, 128, 64), (768, 512, 256)]
ACC_SHAPES = [(192, 128, 64), (768, 512, 256)]
FAMILIES = ["gauss", "rowgraded", "cond1e8"]
KMAX = {np.dtype(np.float64): 400, np.dtype(np.float32): 30}  # column exponents of scaling()

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
    from numpy's QR of normal matrices."""
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
