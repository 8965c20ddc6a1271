"""The apply (tqr_apply_prepare / tqr_apply_q), the solve (tqr_trsm_r, tqr_lstsq, k_resnorm) and
tqr_lstsq_fused on inputs other than a well-conditioned RANDZO factorisation, and on leading
dimensions at the documented bound. Generators and references: tests/inputs.py; that the references
alone meet every condition used here: tests/test_solve_inputs_cpu.py.

Where a test starts from "the oracle's factorisation", the oracle's F and tau are uploaded
(tqr.compact_tau), so a factorisation bug cannot hide an apply bug or the reverse.

A. Exact relations, compared bit for bit (no tolerance).
   1. A D (D = diag(+-2^k), inputs.scaling) has the same V and tau as A: prepare + apply on the scaled
      factorisation give the bits of the unscaled one, while the R entries the apply loads and
      discards are 2^+-400 instead of about 1.
   2. NaN in every element on or above the global diagonal of F changes nothing: R is never used as
      a value by prepare or apply (include/tqr.h "apply").
   3. Column j of the right-hand side times e_j = +-2^k_j (inputs.rhs_scaling; fp64 +-400, fp32 +-30)
      multiplies column j of the result by e_j: apply_q, trsm_r, ApplyQ.lstsq (both directions each)
      and TiledQR.lstsq_fused, the residual norms included (fp64 sum, the root of an even power of
      two is exact). fp32 least squares uses +-KMAX_RES32 = 80: the entries stay normal floats, their
      squares do not — a float accumulator in k_resnorm fails here.
   4. trsm_r(R D, Y) = D^{-1} trsm_r(R, Y) and trsm_r(R D, D Y, trans) = trsm_r(R, Y, trans).
   5. lstsq_fused on [A D | B] against [A | B]: X' = D^{-1} X, the same rows n .. m-1 of Q^T B, the
      same residual norms — the engine's covariance through the capped plan and the solve.
   6. ApplyQ.lstsq is the documented composition of apply_q and trsm_r, on the conditioned matrices.
B. Accuracy on gauss, rowgraded, cond1e8 and the structured matrix (a zero column: reflectors with
   tau == 2; a duplicated column and an identity band: an exactly zero diagonal entry of R).
   apply:  the bounds of tests/test_gpu_apply.py unchanged (Q is orthogonal whatever cond(A) is).
   trsm_r: the componentwise rule |op(R) x - y| <= n u (|op(R)| |x| + |y|) of tests/test_gpu_solve.py
           on the R of rowgraded and cond1e8 (max|x| about 1e8). The forward rule of check_solution
           is not asserted there: it presumes cond(R) < 20, and at cond 1e8 a correct x differs from
           another correct x by cond u = 1e-8 relative.
   lstsq, lstsq_fused (fp64, 5 right-hand sides): e = |x - x_ld|_F / |x_ld|_F against the
           numpy.longdouble solution (inputs.lstsq_longdouble) must satisfy
               e_gpu <= LSQ_MARGIN * max(e_oracle_path, e_numpy),  LSQ_MARGIN = 6,
           e_oracle_path: oracle factorisation, oracle_qt, plain substitution; e_numpy:
           numpy.linalg.lstsq. The margin is twice the largest spread between those two CPU solvers,
           rounded up, measured by test_solve_inputs_cpu.py::test_lstsq_reference_spread:
               family     shape          e_oracle_path  e_numpy    spread
               rowgraded  96x64 b32      1.41e-14       1.14e-14   1.24
               cond1e8    96x64 b32      3.20e-09       1.67e-09   1.91
               rowgraded  192x128 b64    2.90e-14       2.00e-14   1.45
               cond1e8    192x128 b64    3.92e-09       1.51e-09   2.60
               rowgraded  768x512 b256   6.17e-14       7.18e-14   1.16
               cond1e8    768x512 b256   7.28e-09       4.29e-09   1.69
           (the project's tol * cond(A) rule would be 1e-3 here, five orders looser). fp32 is left
           out of this rule: numpy.linalg.lstsq has no fp32-storage counterpart to measure a spread
           against. The residual norms are compared with the norm of rows n .. m-1 of oracle_qt's
           result at 1e-11 |B|_F. That is conditioning-free for a given factorisation (the apply is
           orthogonal), not between two factorisations: range(A) moves by cond(A) u under the rounding
           of the QR itself, and |(I - P) b| with it (numpy's residual norms differ from the oracle
           path's by 2e-9 on cond1e8). So oracle_qt runs on the factorisation the GPU call applies: the
           oracle's own, uploaded, for ApplyQ.lstsq, and the F, tau that lstsq_fused leaves.
C. tqr_trsm_r with R[d, d] = 0 (a legal argument with documented behaviour): the rows solved before
   row d are bit-identical to the unmodified solve, row d is not finite in any column. Nothing is
   asserted about inf against NaN or about the rows that depend on row d.
D. Leading dimensions at the bound 32 * ld * sizeof(element) < 2^31: ld = 8,388,607 (fp64) and
   16,777,215 (fp32), both odd. The engine, apply_q and trsm_r give the bits of the packed calls and
   leave the rows just below the matrix alone. The 32-bit offset expressions these runs exercise are
   listed in DESIGN.md 5.1.
"""
import numpy as np
import pytest

import inputs
from inputs import APPLY_FAMILIES, SOLVE_CASES, bits, dtname
from test_gpu_apply import check
from test_gpu_solve import check_backward, gpu_solve, problem

pytestmark = pytest.mark.gpu

IDS = [f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in SOLVE_CASES]
NRHS = 17
TRANS = [False, True]
TIDS = ["R", "Rt"]
SENTINEL = -7.25
_cache = {}


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def rhs(oracle, shape, dt, nrhs=NRHS, seed=23):
    return oracle.randzo(shape[0], nrhs, dt, seed=seed)


def scaled_factor(oracle, shape, dt):
    """(F, T, Fs, Ts, d): the oracle on matrix("gauss") and on its columns times scaling()."""
    key = ("scaled", shape, dtname(dt))
    if key not in _cache:
        d = inputs.scaling(shape, dt)
        Fs, Ts = oracle.factor(inputs.scale_columns(inputs.matrix("gauss", shape, dt), d), shape[2])
        Fs.setflags(write=False)
        Ts.setflags(write=False)
        _cache[key] = (Fs, Ts, d)
    F, T = inputs.oracle_factor(oracle, "gauss", shape, dt)
    return (F, T) + _cache[key]


def gpu_lstsq(tqr, F, T, B, shape, trans=False):
    """ApplyQ.lstsq on host factors: (B on exit (nrhs, m), res (nrhs,); res is None with trans)."""
    import torch
    m, n, b = shape
    dF = torch.from_numpy(np.array(F)).cuda()
    dtau = torch.from_numpy(tqr.compact_tau(T, m, n, b)).cuda()
    dB = torch.from_numpy(np.array(B)).cuda()
    res = torch.full((B.shape[0],), -1.0, dtype=dB.dtype, device="cuda")
    ap = tqr.ApplyQ(m, n, b, dB.dtype)
    ap.prepare(dF, dtau)
    ap.lstsq(dF, dB, trans=trans, res=None if trans else res)
    torch.cuda.synchronize()
    return dB.cpu().numpy(), None if trans else res.cpu().numpy()


def gpu_fused(tqr, A, B, b, pad=0.0):
    """TiledQR.lstsq_fused on [A | B | padding]: (B's nrhs columns on exit (nrhs, m), res, and the
    factorisation of A the call leaves: F (n, m), compact tau)."""
    import torch
    n, m = A.shape
    nrhs = B.shape[0]
    r = -(-nrhs // b)
    AB = torch.full((n + r * b, m), pad, dtype=tdt(A.dtype), device="cuda")
    AB[:n] = torch.from_numpy(np.array(A)).cuda()
    AB[n:n + nrhs] = torch.from_numpy(np.array(B)).cuda()
    plan = tqr.TiledQR(m, n + r * b, b, AB.dtype, steps=n // b)
    tau = torch.zeros((n // b, m), dtype=AB.dtype, device="cuda")
    res = torch.full((nrhs,), -1.0, dtype=AB.dtype, device="cuda")
    plan.lstsq_fused(AB, tau, nrhs, res=res)
    plan.status()
    return AB[n:n + nrhs].cpu().numpy(), res.cpu().numpy(), AB[:n].cpu().numpy(), tau.cpu().numpy()


# ---- A. exact relations ----------------------------------------------------------------------
@pytest.mark.parametrize("trans", [True, False], ids=["qt", "q"])
@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_same_q_from_scaled_a(tqr, oracle, shape, dt, trans):
    b = shape[2]
    F, T, Fs, Ts, d = scaled_factor(oracle, shape, dt)
    inputs.assert_covariant(F, T, Fs, Ts, d)
    C = rhs(oracle, shape, dt)
    clean = tqr.apply_q_host(F, T, C, b, trans=trans)
    assert np.isfinite(clean).all()
    assert same_bits(tqr.apply_q_host(Fs, Ts, C, b, trans=trans), clean)


@pytest.mark.parametrize("trans", [True, False], ids=["qt", "q"])
@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_r_is_never_used_as_a_value(tqr, oracle, shape, dt, trans):
    m, n, b = shape
    F, T = inputs.oracle_factor(oracle, "gauss", shape, dt)
    Fn = inputs.poison_r(F)
    assert np.isnan(Fn).sum() == n * (n + 1) // 2
    C = rhs(oracle, shape, dt)
    clean = tqr.apply_q_host(F, T, C, b, trans=trans)
    assert np.isfinite(clean).all()
    assert same_bits(tqr.apply_q_host(Fn, T, C, b, trans=trans), clean)


@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_rhs_scaling_apply_and_trsm(tqr, oracle, shape, dt):
    m, n, b = shape
    F, T = inputs.oracle_factor(oracle, "gauss", shape, dt)
    C = rhs(oracle, shape, dt)
    e = inputs.rhs_scaling(shape, dt, NRHS)
    Cs = inputs.scale_columns(C, e)
    for trans in (True, False):
        inputs.assert_scaled(tqr.apply_q_host(F, T, Cs, b, trans=trans), tqr.apply_q_host(F, T, C, b, trans=trans), e)
    Y, Ys = np.ascontiguousarray(C[:, :n]), np.ascontiguousarray(Cs[:, :n])
    for trans in TRANS:
        inputs.assert_scaled(gpu_solve(tqr, F, Ys, b, trans), gpu_solve(tqr, F, Y, b, trans), e)


@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_rhs_scaling_least_squares(tqr, oracle, shape, dt):
    m, n, b = shape
    F, T = inputs.oracle_factor(oracle, "gauss", shape, dt)
    C = rhs(oracle, shape, dt)
    e = inputs.rhs_scaling(shape, dt, NRHS, inputs.KMAX_RES32 if np.dtype(dt) == np.float32 else None)
    Cs = inputs.scale_columns(C, e)
    out, res = gpu_lstsq(tqr, F, T, C, shape)
    outs, ress = gpu_lstsq(tqr, F, T, Cs, shape)
    inputs.assert_scaled(outs, out, e)
    assert inputs.in_normal_range(ress) and np.all(res > 0)
    assert same_bits(ress, res * np.abs(e))
    inputs.assert_scaled(gpu_lstsq(tqr, F, T, Cs, shape, trans=True)[0], gpu_lstsq(tqr, F, T, C, shape, trans=True)[0], e)
    A = inputs.matrix("gauss", shape, dt)
    out, res = gpu_fused(tqr, A, C, b)[:2]
    outs, ress = gpu_fused(tqr, A, Cs, b)[:2]
    inputs.assert_scaled(outs, out, e)
    assert inputs.in_normal_range(ress) and np.all(res > 0)
    assert same_bits(ress, res * np.abs(e))


@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_column_scaling_through_trsm(tqr, oracle, shape, dt):
    m, n, b = shape
    F, T, Fs, Ts, d = scaled_factor(oracle, shape, dt)
    Y = np.ascontiguousarray(rhs(oracle, shape, dt)[:, :n])
    X = gpu_solve(tqr, F, Y, b, False)
    assert inputs.in_normal_range(X / d[None, :])
    assert same_bits(gpu_solve(tqr, Fs, Y, b, False), X / d[None, :])
    assert same_bits(gpu_solve(tqr, Fs, Y * d[None, :], b, True), gpu_solve(tqr, F, Y, b, True))


@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_column_scaling_through_lstsq_fused(tqr, oracle, shape, dt):
    m, n, b = shape
    A = inputs.matrix("gauss", shape, dt)
    d = inputs.scaling(shape, dt)
    B = rhs(oracle, shape, dt, nrhs=5, seed=8)
    out, res = gpu_fused(tqr, A, B, b)[:2]
    outs, ress = gpu_fused(tqr, inputs.scale_columns(A, d), B, b)[:2]
    assert np.isfinite(out).all() and np.all(res > 0)
    assert same_bits(outs[:, n:], out[:, n:])
    assert same_bits(ress, res)
    assert inputs.in_normal_range(out[:, :n] / d[None, :])
    assert same_bits(outs[:, :n], out[:, :n] / d[None, :])


@pytest.mark.parametrize("family", ["rowgraded", "cond1e8"])
@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_lstsq_is_the_documented_composition(tqr, oracle, shape, dt, family):
    """NOTRANS: apply(trans) then trsm_r on rows 0 .. n-1. TRANS: rows n .. m-1 zeroed, trsm_r(trans)
    on rows 0 .. n-1, then apply(notrans)."""
    m, n, b = shape
    F, T = inputs.oracle_factor(oracle, family, shape, dt)
    B = rhs(oracle, shape, dt, nrhs=5, seed=8)
    out, _ = gpu_lstsq(tqr, F, T, B, shape)
    step = tqr.apply_q_host(F, T, B, b, trans=True)
    step[:, :n] = gpu_solve(tqr, F, np.ascontiguousarray(step[:, :n]), b, False)
    assert np.isfinite(out).all() and same_bits(out, step)
    out, _ = gpu_lstsq(tqr, F, T, B, shape, trans=True)
    step = np.zeros_like(B)
    step[:, :n] = gpu_solve(tqr, F, np.ascontiguousarray(B[:, :n]), b, True)
    assert np.isfinite(out).all() and same_bits(out, tqr.apply_q_host(F, T, step, b, trans=False))


# ---- B. accuracy -------------------------------------------------------------------------------
def apply_reference(oracle, family, shape, dt, trans):
    """(ref, ref64) for 80 right-hand sides, as tests/test_gpu_apply.py::reference builds them."""
    key = ("ref", family, shape, dtname(dt), trans)
    if key not in _cache:
        b = shape[2]
        F, T = inputs.oracle_factor(oracle, family, shape, dt)
        C = rhs(oracle, shape, dt, nrhs=80)
        fn = (lambda f, t, c: inputs.oracle_qt(oracle, f, t, c, b)) if trans else (lambda f, t, c: inputs.numpy_q(f, t, c, b))
        ref = fn(F, T, C)
        ref64 = ref if dt == np.float64 else fn(F.astype(np.float64), T.astype(np.float64), C.astype(np.float64))
        _cache[key] = (ref, ref64)
    return _cache[key]


@pytest.mark.parametrize("nrhs", [17, 80])
@pytest.mark.parametrize("family", APPLY_FAMILIES)
@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_apply_accuracy(tqr, oracle, shape, dt, family, nrhs):
    """Q^T C against the oracle's tile kernels, Q C against the reflector loop, Q (Q^T C) = C."""
    b = shape[2]
    F, T = inputs.oracle_factor(oracle, family, shape, dt)
    if family == "structured":
        assert (T == 2).any() and (np.diag(inputs.upper(F)) == 0).any()
    C = rhs(oracle, shape, dt, nrhs=80)[:nrhs]
    ref, ref64 = apply_reference(oracle, family, shape, dt, True)
    qt = tqr.apply_q_host(F, T, C, b, trans=True)
    check(qt, ref[:nrhs], ref64[:nrhs], f"{family} Q^T C:")
    ref, ref64 = apply_reference(oracle, family, shape, dt, False)
    check(tqr.apply_q_host(F, T, C, b, trans=False), ref[:nrhs], ref64[:nrhs], f"{family} Q C:")
    if dt == np.float64:
        back = tqr.apply_q_host(F, T, qt, b, trans=False)
        err = float(np.abs(back - C).max())
        print(f"{family} max|Q Q^T C - C| = {err:.3e}")
        assert err <= 1e-11 * max(1.0, float(np.abs(C).max()))


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("family", ["rowgraded", "cond1e8"])
@pytest.mark.parametrize("shape,dt", SOLVE_CASES, ids=IDS)
def test_trsm_r_componentwise_on_conditioned_r(tqr, oracle, shape, dt, family, trans):
    """The backward rule only: the forward rule of check_solution presumes cond(R) < 20 (module
    docstring, B)."""
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    n, b = shape[1], shape[2]
    F, _ = inputs.oracle_factor(oracle, family, shape, dt)
    Y = np.ascontiguousarray(rhs(oracle, shape, dt)[:, :n])
    got = gpu_solve(tqr, F, Y, b, trans)
    check_backward(got, inputs.upper(F).astype(np.float64), Y, trans, dt, f"{family}:")


def lsq_reference(oracle, family, shape):
    """(e_oracle_path, e_numpy, res_ref) of the CPU solvers against the extended-precision solution."""
    key = ("lsq", family, shape)
    if key not in _cache:
        A, B = inputs.matrix(family, shape), inputs.lsq_rhs(family, shape)
        F, T = inputs.oracle_factor(oracle, family, shape)
        Xo, res, _ = inputs.oracle_lstsq(oracle, F, T, B, shape[2])
        Xn = np.linalg.lstsq(A.T, B.T, rcond=None)[0].T
        Xld = inputs.x_ld(family, shape)
        _cache[key] = (inputs.rel_err(Xo, Xld), inputs.rel_err(Xn, Xld), res)
    return _cache[key]


@pytest.mark.parametrize("fused", [False, True], ids=["lstsq", "fused"])
@pytest.mark.parametrize("family", ["rowgraded", "cond1e8"])
@pytest.mark.parametrize("shape", [s for s, dt in SOLVE_CASES if dt == np.float64], ids=lambda s: "%dx%db%d" % s)
def test_lstsq_vs_longdouble(tqr, oracle, shape, family, fused):
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    m, n, b = shape
    A, B = inputs.matrix(family, shape), inputs.lsq_rhs(family, shape)
    eo, en, res_ref = lsq_reference(oracle, family, shape)
    if fused:
        # (the call's own factorisation of A: the residual norm is conditioning-free only for a given Q)
        out, res, Fg, taug = gpu_fused(tqr, A, B, b)
        res_ref = inputs.resnorm(inputs.oracle_qt(oracle, Fg, tqr.expand_tau(taug, m, n, b), B, b), n)
    else:
        F, T = inputs.oracle_factor(oracle, family, shape)
        out, res = gpu_lstsq(tqr, F, T, B, shape)
    eg = inputs.rel_err(out[:, :n], inputs.x_ld(family, shape))
    er = float(np.abs(res - res_ref).max())
    print(f"{family} {shape} {'fused' if fused else 'lstsq'}: e_gpu {eg:.3e}, e_oracle_path {eo:.3e}, e_numpy {en:.3e}, "
          f"ratio {eg / max(eo, en):.2f} (allowed {inputs.LSQ_MARGIN}), max|res - res_ref| {er:.2e}")
    assert np.isfinite(out).all()
    assert eg <= inputs.LSQ_MARGIN * max(eo, en)
    assert er <= 1e-11 * float(np.linalg.norm(B))


# ---- C. a zero diagonal entry --------------------------------------------------------------------
ZERO_CASES = [((192, 128, 64), np.float64), ((192, 128, 64), np.float32), ((768, 512, 256), np.float64)]


@pytest.mark.parametrize("trans", TRANS, ids=TIDS)
@pytest.mark.parametrize("shape,dt", ZERO_CASES, ids=[f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in ZERO_CASES])
def test_trsm_r_zero_diagonal(tqr, oracle, shape, dt, trans):
    m, n, b = shape
    F, _, Y = problem(oracle, shape, dt)
    d = inputs.zero_diag_index(b)
    assert b < d < n - 1 and d % 32 == 16
    F0 = F.copy()
    F0[d, d] = 0.0
    X = gpu_solve(tqr, F, Y[:NRHS], b, trans)
    X0 = gpu_solve(tqr, F0, Y[:NRHS], b, trans)
    before = slice(0, d) if trans else slice(d + 1, n)
    assert np.isfinite(X).all()
    assert same_bits(X0[:, before], X[:, before])
    assert not np.isfinite(X0[:, d]).any()


# ---- D. leading dimensions at the bound ---------------------------------------------------------
LD = {np.dtype(np.float64): 8388607, np.dtype(np.float32): 16777215}
SMALL = (64, 64, 32)


def strided(buf, cols, rows, ld, row0=0):
    """rows row0 .. row0 + rows - 1 of the first `cols` columns of a flat buffer of leading dimension ld."""
    return buf.as_strided((cols, rows), (ld, 1), row0)


def big_copy(host, ld):
    """A flat device buffer holding the (cols, rows) host array with leading dimension ld, sentinels in
    the two rows below it; everything else is uninitialised."""
    import torch
    cols, rows = host.shape
    buf = torch.empty(cols * ld, dtype=tdt(host.dtype), device="cuda")
    strided(buf, cols, rows, ld).copy_(torch.from_numpy(np.array(host)).cuda())
    strided(buf, cols, 2, ld, rows).fill_(SENTINEL)
    return buf


def sentinels_intact(buf, cols, rows, ld):
    return bool((strided(buf, cols, 2, ld, rows) == SENTINEL).all())


ENGINE_LD = [(SMALL, np.float64), (SMALL, np.float32), ((256, 256, 128), np.float64)]


@pytest.mark.parametrize("shape,dt", ENGINE_LD, ids=[f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in ENGINE_LD])
def test_engine_at_the_ld_bound(tqr, shape, dt):
    import torch
    m, n, b = shape
    ld = LD[np.dtype(dt)]
    if n * ld * np.dtype(dt).itemsize > 16e9 and torch.cuda.mem_get_info()[0] < 20e9:
        pytest.skip("less than 20 GB of device memory free")
    A = inputs.matrix("gauss", shape, dt)
    plan = tqr.TiledQR(m, n, b, tdt(dt))
    dA = torch.from_numpy(A.copy()).cuda()
    tau0 = torch.zeros((plan.kmax, m), dtype=dA.dtype, device="cuda")
    plan.execute(dA, tau0)
    plan.status()
    buf = big_copy(A, ld)
    tau = torch.zeros_like(tau0)
    plan.execute(buf, tau, ldda=ld)
    plan.status()
    ok = torch.equal(strided(buf, n, m, ld), dA) and torch.equal(tau, tau0) and sentinels_intact(buf, n, m, ld)
    del buf
    torch.cuda.empty_cache()
    assert ok and bool(torch.isfinite(dA).all())


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=dtname)
def test_apply_at_the_ld_bound(tqr, oracle, dt):
    import torch
    m, n, b = SMALL
    ld = LD[np.dtype(dt)]
    F, T = inputs.oracle_factor(oracle, "gauss", SMALL, dt)
    C = rhs(oracle, SMALL, dt)
    want = {tr: tqr.apply_q_host(F, T, C, b, trans=tr) for tr in (True, False)}
    dtau = torch.from_numpy(tqr.compact_tau(T, m, n, b)).cuda()
    ap = tqr.ApplyQ(m, n, b, tdt(dt))
    # ldda = ld
    bufF = big_copy(F, ld)
    ap.prepare(bufF, dtau, ldda=ld)
    ok = True
    for tr in (True, False):
        dC = torch.from_numpy(C.copy()).cuda()
        ap.apply(bufF, dC, trans=tr, ldda=ld)
        ok = ok and same_bits(dC.cpu().numpy(), want[tr])
    ok = ok and sentinels_intact(bufF, n, m, ld) and same_bits(strided(bufF, n, m, ld).cpu().numpy(), F)
    del bufF
    torch.cuda.empty_cache()
    assert ok
    # lddc = ld
    dF = torch.from_numpy(F.copy()).cuda()
    ap.prepare(dF, dtau)
    for tr in (True, False):
        bufC = big_copy(C, ld)
        ap.apply(dF, bufC, trans=tr, nrhs=NRHS, lddc=ld)
        ok = ok and same_bits(strided(bufC, NRHS, m, ld).cpu().numpy(), want[tr]) and sentinels_intact(bufC, NRHS, m, ld)
        del bufC
        torch.cuda.empty_cache()
    assert ok


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=dtname)
def test_trsm_r_at_the_ld_bound(tqr, oracle, dt):
    import torch
    m, n, b = SMALL
    ld = LD[np.dtype(dt)]
    F, _ = inputs.oracle_factor(oracle, "gauss", SMALL, dt)
    Y = np.ascontiguousarray(rhs(oracle, SMALL, dt)[:, :n])
    want = {tr: gpu_solve(tqr, F, Y, b, tr) for tr in TRANS}
    ok = True
    # ldda = ld
    bufF = big_copy(F, ld)
    for tr in TRANS:
        dX = torch.from_numpy(Y.copy()).cuda()
        tqr.trsm_r(bufF, dX, b, trans=tr, n=n, nrhs=NRHS, ldda=ld, lddx=n)
        ok = ok and same_bits(dX.cpu().numpy(), want[tr])
    ok = ok and sentinels_intact(bufF, n, m, ld) and same_bits(strided(bufF, n, m, ld).cpu().numpy(), F)
    del bufF
    torch.cuda.empty_cache()
    assert ok
    # lddx = ld
    dF = torch.from_numpy(F.copy()).cuda()
    for tr in TRANS:
        bufX = big_copy(Y, ld)
        tqr.trsm_r(dF, bufX, b, trans=tr, n=n, nrhs=NRHS, ldda=m, lddx=ld)
        ok = ok and same_bits(strided(bufX, NRHS, n, ld).cpu().numpy(), want[tr]) and sentinels_intact(bufX, NRHS, n, ld)
        del bufX
        torch.cuda.empty_cache()
    assert ok
