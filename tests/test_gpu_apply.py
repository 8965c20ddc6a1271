"""C <- Q^T C / C <- Q C of a finished tiled factorisation (tqr_apply, include/tqr.h "apply") and
tqr.lstsq, on the GPU.

References (never the GPU): F and tau come from the oracle's factorisation of a RANDZO matrix; Q^T C
is the oracle's own UNMQR / TSMQR tile kernels walked over [F | C] in the order of the
factorisation; Q C is a plain numpy loop applying the reflectors I - tau v v^T one by one in reverse.

Tolerances:
  fp64: max|GPU - ref| <= 1e-11 * max(1, max|ref|) — the project's whole-factorisation bound (the
        apply is the same chain of tile updates);
  fp32: max|GPU - ref32| <= 1e-4 * max(1, max|ref32|), and the GPU result is no farther from the fp64
        reference on the same fp32-valued input than 1.5 times the fp32 reference's own distance
        (the rule of test_gpu_factor.py for fp32 storage with fp64 arithmetic).
"""
import ctypes

import numpy as np
import pytest

from inputs import numpy_q, oracle_qt, reflectors  # noqa: F401 (shared with the other apply / solve tests)

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
# the smallest shapes at which each mechanism exists (m, n, b): one group per tile; two groups (the GE
# group's skipped zero k-steps); 4 and 8 groups (the production tile); wide (kmax = p); tall (a TS
# chain of 3 under one panel); a single tile row (p = 1: no TSMQR at all), wide and square; a tall chain
# (9 TSMQR tiles under each UNMQR).
SHAPES = [(48, 32, 16), (96, 64, 32), (192, 128, 64), (384, 256, 128), (768, 512, 256), (256, 384, 128),
          (1024, 256, 256), (64, 128, 64), (256, 256, 256), (1280, 256, 128)]
SHAPES32 = [(48, 32, 16), (96, 64, 32), (192, 128, 64), (384, 256, 128), (768, 512, 256), (256, 384, 128)]
NRHS = [1, 17, 64, 80]  # one lane, a ragged wave, one full workgroup, two workgroups (the second ragged)
NMAX = max(NRHS)
CASES = [(s, np.float64) for s in SHAPES] + [(s, np.float32) for s in SHAPES32]
IDS = [f"{m}x{n}b{b}-{'f64' if dt == np.float64 else 'f32'}" for (m, n, b), dt in CASES]

_cache = {}


def factored(oracle, shape, dt):
    """(A, F, T) of the oracle's factorisation of the shape's RANDZO matrix (computed once)."""
    key = ("fact", shape, np.dtype(dt).name)
    if key not in _cache:
        m, n, b = shape
        A = oracle.randzo(m, n, dt, seed=11 + b)
        F, T = oracle.factor(A, b)
        for x in (A, F, T):
            x.setflags(write=False)
        _cache[key] = (A, F, T)
    return _cache[key]


def rhs(oracle, shape, dt, seed=23):
    key = ("rhs", shape, np.dtype(dt).name, seed)
    if key not in _cache:
        C = oracle.randzo(shape[0], NMAX, dt, seed=seed)
        C.setflags(write=False)
        _cache[key] = C
    return _cache[key]


def reference(oracle, shape, dt, trans):
    """(ref, ref64): the reference for NMAX right-hand sides in dtype dt, and (fp32) the fp64
    reference on the same fp32-valued input. Columns are independent: nrhs < NMAX takes a slice."""
    key = ("ref", shape, np.dtype(dt).name, trans)
    if key not in _cache:
        _, F, T = factored(oracle, shape, dt)
        C = rhs(oracle, shape, dt)
        b = shape[2]
        fn = (lambda f, t, c: oracle_qt(oracle, f, t, c, b)) if trans else (lambda f, t, c: numpy_q(f, t, c, b))
        ref = fn(F, T, C)
        ref64 = ref if dt == np.float64 else fn(F.astype(np.float64), T.astype(np.float64), C.astype(np.float64))
        _cache[key] = (ref, ref64)
    return _cache[key]


def check(got, ref, ref64, what=""):
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


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_apply_qt_vs_oracle(tqr, oracle, shape, dt, nrhs):
    _, F, T = factored(oracle, shape, dt)
    C = rhs(oracle, shape, dt)[:nrhs]
    ref, ref64 = reference(oracle, shape, dt, True)
    got = tqr.apply_q_host(F, T, C, shape[2], trans=True)
    assert got.shape == C.shape and got.dtype == C.dtype
    check(got, ref[:nrhs], ref64[:nrhs], "Q^T C:")


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_apply_q_vs_numpy(tqr, oracle, shape, dt, nrhs):
    _, F, T = factored(oracle, shape, dt)
    C = rhs(oracle, shape, dt)[:nrhs]
    ref, ref64 = reference(oracle, shape, dt, False)
    got = tqr.apply_q_host(F, T, C, shape[2], trans=False)
    check(got, ref[:nrhs], ref64[:nrhs], "Q C:")


def _upper(F):
    """R of a factorised (n, m) array: entries (i, j) with i <= j, zero below."""
    n, m = F.shape
    return np.where(np.arange(m)[None, :] <= np.arange(n)[:, None], F, 0.0)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}b{b}" for m, n, b in SHAPES])
def test_apply_q_of_R_gives_A(tqr, oracle, shape):
    """Q [R; 0] = A: NOTRANS on the upper-triangular part of F recovers the original matrix."""
    A, F, T = factored(oracle, shape, np.float64)
    got = tqr.apply_q_host(F, T, _upper(F), shape[2], trans=False)
    err = float(np.abs(got - A).max())
    print(f"max|Q R - A| = {err:.3e}")
    assert err <= 1e-11 * max(1.0, float(np.abs(A).max()))


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}b{b}" for m, n, b in SHAPES])
def test_apply_qt_of_A_gives_R(tqr, oracle, shape):
    """End to end on the GPU: F, tau from tqr.geqrt_host, then Q^T A (C = A, nrhs = n) is R on and
    above the diagonal and zero below it."""
    m, n, b = shape
    A = oracle.randzo(m, n, np.float64, seed=3)
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    got = tqr.apply_q_host(F, T, A, b, trans=True)
    R = _upper(F)
    up = np.arange(m)[None, :] <= np.arange(n)[:, None]
    e_up = float(np.abs(got - R)[up].max())
    e_lo = float(np.abs(got)[~up].max())
    print(f"max|triu(Q^T A) - R| = {e_up:.3e}, max|below the diagonal| = {e_lo:.3e}")
    assert e_up <= 1e-11 * max(1.0, float(np.abs(R).max()))
    assert e_lo <= 1e-11 * float(np.abs(A).max())


@pytest.mark.parametrize("shape", [(192, 128, 64), (768, 512, 256)], ids=["192x128b64", "768x512b256"])
def test_roundtrip(tqr, oracle, shape):
    """Q (Q^T C) = C."""
    _, F, T = factored(oracle, shape, np.float64)
    C = rhs(oracle, shape, np.float64)
    back = tqr.apply_q_host(F, T, tqr.apply_q_host(F, T, C, shape[2], trans=True), shape[2], trans=False)
    err = float(np.abs(back - C).max())
    print(f"max|Q Q^T C - C| = {err:.3e}")
    assert err <= 1e-11 * max(1.0, float(np.abs(C).max()))


def _device_setup(tqr, oracle, shape, dt, ldda=None, seed_shift=0):
    """Handle plus device F (n, ldda), compact tau of the oracle's factorisation."""
    import torch
    m, n, b = shape
    if seed_shift:
        A = oracle.randzo(m, n, dt, seed=101 + seed_shift)
        F, T = oracle.factor(A, b)
    else:
        _, F, T = factored(oracle, shape, dt)
    ldda = ldda or m
    Fp = np.full((n, ldda), -7.5, dtype=dt)
    Fp[:, :m] = F
    dF = torch.from_numpy(Fp).cuda()
    dtau = torch.from_numpy(tqr.compact_tau(T, m, n, b)).cuda()
    return tqr.ApplyQ(m, n, b, dt), dF, dtau, F, T


@pytest.mark.parametrize("trans", [True, False], ids=["qt", "q"])
def test_padding_and_inputs_untouched(tqr, oracle, trans):
    """ldda = m + 8, lddc = m + 3, C allocated with 16 extra columns: rows >= m and columns >= nrhs
    (sentinels), A and tau are bit-identical after the call, and the result is right."""
    import torch
    shape, nrhs = (192, 128, 64), 17
    m, n, b = shape
    ap, dF, dtau, F, T = _device_setup(tqr, oracle, shape, np.float64, ldda=m + 8)
    C = rhs(oracle, shape, np.float64)[:nrhs]
    Cp = np.full((nrhs + 16, m + 3), 1234.5)
    Cp[:nrhs, :m] = C
    dC = torch.from_numpy(Cp).cuda()
    F0, tau0 = dF.clone(), dtau.clone()
    ap.prepare(dF, dtau, ldda=m + 8)
    ap.apply(dF, dC, trans=trans, nrhs=nrhs, ldda=m + 8, lddc=m + 3)
    torch.cuda.synchronize()
    out = dC.cpu().numpy()
    assert torch.equal(dF, F0) and torch.equal(dtau, tau0)
    assert np.all(out[nrhs:] == 1234.5) and np.all(out[:, m:] == 1234.5)
    ref, ref64 = reference(oracle, shape, np.float64, trans)
    check(out[:nrhs, :m], ref[:nrhs], ref64[:nrhs])


@pytest.mark.parametrize("trans", [True, False], ids=["qt", "q"])
def test_strip_independence_and_determinism(tqr, oracle, trans):
    """The first 17 columns of an nrhs = 80 apply are bit-identical to an nrhs = 17 apply of the same
    columns, and two identical calls give bit-identical output."""
    shape = (192, 128, 64)
    _, F, T = factored(oracle, shape, np.float64)
    C = rhs(oracle, shape, np.float64)
    o80 = tqr.apply_q_host(F, T, C, shape[2], trans=trans)
    o17 = tqr.apply_q_host(F, T, C[:17], shape[2], trans=trans)
    again = tqr.apply_q_host(F, T, C, shape[2], trans=trans)
    assert np.array_equal(o80[:17], o17)
    assert np.array_equal(o80, again)


def test_prepare_once_apply_many_on_stream(tqr, oracle):
    """One prepare, two applies with different C on a non-default torch stream; then a second
    prepare with another factorisation of the same shape and an apply after it."""
    import torch
    shape, nrhs = (384, 256, 128), 80
    b = shape[2]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ap, dF, dtau, F, T = _device_setup(tqr, oracle, shape, np.float64)
        C1 = rhs(oracle, shape, np.float64)
        C2 = rhs(oracle, shape, np.float64, seed=29)
        d1, d2 = torch.from_numpy(C1.copy()).cuda(), torch.from_numpy(C2.copy()).cuda()
        ap.prepare(dF, dtau, stream=s)
        ap.apply(dF, d1, trans=True, stream=s)
        ap.apply(dF, d2, trans=True, stream=s)
        _, dF2, dtau2, F2, T2 = _device_setup(tqr, oracle, shape, np.float64, seed_shift=1)
        d3 = torch.from_numpy(C1.copy()).cuda()
        ap.prepare(dF2, dtau2, stream=s)
        ap.apply(dF2, d3, trans=True, stream=s)
    s.synchronize()
    ref1, _ = reference(oracle, shape, np.float64, True)
    check(d1.cpu().numpy(), ref1, ref1, "first C:")
    ref2 = oracle_qt(oracle, F, T, C2, b)
    check(d2.cpu().numpy(), ref2, ref2, "second C:")
    ref3 = oracle_qt(oracle, F2, T2, C1, b)
    check(d3.cpu().numpy(), ref3, ref3, "after the second prepare:")
    assert nrhs == C1.shape[0] and ap.workspace_bytes() > 0


def test_apply_before_prepare_and_bad_args(tqr, oracle):
    """tqr_apply_q's TQR_EINVAL cases on a live handle."""
    import torch
    shape = (96, 64, 32)
    m = shape[0]
    ap, dF, dtau, _, _ = _device_setup(tqr, oracle, shape, np.float64)
    dC = torch.zeros((4, m), dtype=torch.float64, device="cuda")
    with pytest.raises(tqr.TQRError):
        ap.apply(dF, dC)  # before the first prepare
    ap.prepare(dF, dtau)
    L = tqr.lib()
    a, c = P(dF.data_ptr()), P(dC.data_ptr())
    assert L.tqr_apply_q(ap.h, 1, a, m, c, 0, m, None) == -1       # nrhs < 1
    assert L.tqr_apply_q(ap.h, 2, a, m, c, 4, m, None) == -1       # trans not 0 / 1
    assert L.tqr_apply_q(ap.h, 1, a, m - 1, c, 4, m, None) == -1   # ldda < m
    assert L.tqr_apply_q(ap.h, 1, a, m, c, 4, m - 1, None) == -1   # lddc < m
    assert L.tqr_apply_q(ap.h, 1, a, m, c, 4, 8388608, None) == -1  # lddc beyond the bound
    assert L.tqr_apply_q(ap.h, 1, None, m, c, 4, m, None) == -1
    assert L.tqr_apply_q(ap.h, 1, a, m, None, 4, m, None) == -1
    # workspace: one whole-KiB T image per group of every tile (l, k), l >= k (here 3 * 2 - 1 tiles)
    assert ap.workspace_bytes() == 5 * 1 * 1152 * 8
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(768, 256, 128), (1024, 256, 256)], ids=["768x256b128", "1024x256b256"])
def test_lstsq_vs_numpy(tqr, oracle, shape):
    """tqr.lstsq on a GPU factorisation against numpy.linalg.lstsq. The matrices are well conditioned
    (asserted), so a wrong answer cannot hide behind ill-conditioning."""
    import torch
    m, n, b = shape
    nrhs = 3
    A = oracle.randzo(m, n, np.float64, seed=7)
    B = oracle.randzo(m, nrhs, np.float64, seed=8)
    cond = float(np.linalg.cond(A.T))
    assert cond < 10
    dF = torch.from_numpy(A.copy()).cuda()
    dtau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
    tqr.TiledQR(m, n, b, torch.float64).execute(dF, dtau)
    dB = torch.from_numpy(B.copy()).cuda()
    X, res = tqr.lstsq(dF, dtau, dB, b)
    torch.cuda.synchronize()
    X, res = X.cpu().numpy(), res.cpu().numpy()
    assert X.shape == (nrhs, n) and res.shape == (nrhs,)
    Xn = np.linalg.lstsq(A.T, B.T, rcond=None)[0]  # n x nrhs
    rn = np.linalg.norm(A.T @ Xn - B.T, axis=0)
    ex = float(np.linalg.norm(X.T - Xn) / np.linalg.norm(Xn))
    er = float(np.abs(res - rn).max())
    print(f"cond(A) = {cond:.2f}, |X - X_np|_F / |X_np|_F = {ex:.3e}, max|res - res_np| = {er:.3e}")
    assert ex <= 1e-11 * cond
    assert er <= 1e-11 * float(np.linalg.norm(B))


def test_lstsq_rejects_wide(tqr):
    import torch
    F = torch.zeros((384, 256), dtype=torch.float64, device="cuda")
    tau = torch.zeros((2, 256), dtype=torch.float64, device="cuda")
    B = torch.zeros((3, 256), dtype=torch.float64, device="cuda")
    with pytest.raises(tqr.TQRError):
        tqr.lstsq(F, tau, B, 128)
