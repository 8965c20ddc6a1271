"""The single-GPU engine on inputs other than RANDZO, and on device arrays other than a packed one
on the default stream. Generators and the extended-precision reference: tests/inputs.py; that the
oracle alone meets every condition used here: tests/test_inputs_cpu.py.

1. Column scaling. Householder QR satisfies factor(A D) = (R D, V, tau) bit for bit for
   D = diag(+-2^k_j): every operation on column j is linear in it, powers of two commute with
   rounding while nothing over- or underflows, and sign(x0) flips with the column. The panel's
   hand-written norm (v_rsq_f64 seed + Newton steps on the unscaled n2 = x0^2 + D_c), reciprocal
   (v_rcp_f64 seed) and tau see n2 from 2^-997 to 2^+968 here instead of 1e-4 .. 1e3. The unscaled
   result is compared with the oracle at the project's bounds, so the scaled one is tied to the
   oracle by an exact relation and needs no tolerance.
2. A zero first pivot (+0.0 and -0.0) over a live tail: sign(0) = +1 in the reference.
3. Accuracy against a numpy.longdouble Householder QR on conditioned inputs: residual, column
   norms and the column-relative error of |R|, which must be within 1.5 x the oracle's own (the
   project's rule for fp32 storage). These are sign-free and well posed at any condition number.
   V and tau are compared elementwise for `gauss` only: on `rowgraded` and `cond1e8` the trailing
   columns shrink to about sigma_min, so two correct factorisations differ in V by about
   cond * eps relative, and there is nothing to assert.
4. Device arrays: ldda > m (even and odd padding: columns then start 8 bytes (fp64) / 4 bytes
   (fp32) off the engine's 16- / 8-byte pair accesses), a base one element into an allocation, a
   non-default stream, and one plan run on X, Y, X. The arithmetic does not depend on where the
   matrix lies, so each result is bit-identical to the packed default-stream run.
"""
import numpy as np
import pytest

import inputs
from inputs import ACC_SHAPES, FAMILIES, SHAPES, SHAPES32, dtname
from test_gpu_factor import assert_close

pytestmark = pytest.mark.gpu

SCALE_CASES = [(s, np.float64) for s in SHAPES] + [(s, np.float32) for s in SHAPES32]


def ids(cases):
    return [f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in cases]


def gpu_factor(tqr, A, b):
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    return F, T


_base = {}


def base_factor(tqr, oracle, shape, dt):
    """The GPU's factorisation of the shape's gauss matrix, checked against the oracle (once)."""
    key = (shape, np.dtype(dt).name)
    if key not in _base:
        F, T = gpu_factor(tqr, inputs.matrix("gauss", shape, dt), shape[2])
        F.setflags(write=False)
        T.setflags(write=False)
        _base[key] = (F, T)
    F, T = _base[key]
    F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, dt)
    assert_close(F, T, F_ref, T_ref)
    return F, T


# ---- 1. column scaling ----------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", SCALE_CASES, ids=ids(SCALE_CASES))
def test_column_scaling_bitexact(tqr, oracle, shape, dt):
    A = inputs.matrix("gauss", shape, dt)
    d = inputs.scaling(shape, dt)
    F, T = base_factor(tqr, oracle, shape, dt)
    Fs, Ts = gpu_factor(tqr, inputs.scale_columns(A, d), shape[2])
    inputs.assert_covariant(F, T, Fs, Ts, d)


@pytest.mark.parametrize("e", [480, -480])
def test_global_factor_bitexact(tqr, oracle, e):
    """All columns times 2^e: n2 near both ends of the fp64 range (about 1e+-289), still normal."""
    shape = (192, 128, 64)
    A = inputs.matrix("gauss", shape)
    d = np.full(shape[1], np.ldexp(1.0, e))
    F, T = base_factor(tqr, oracle, shape, np.float64)
    Fs, Ts = gpu_factor(tqr, inputs.scale_columns(A, d), shape[2])
    inputs.assert_covariant(F, T, Fs, Ts, d)


# ---- 2. zero pivots --------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=dtname)
def test_zero_first_pivot(tqr, oracle, dt, zero):
    shape = (192, 128, 64)
    A = inputs.matrix("gauss", shape, dt).copy()
    A[0, 0] = zero
    assert np.signbit(A[0, 0]) == np.signbit(zero) and np.abs(A[0, 1:]).min() > 0
    F_ref, T_ref = oracle.factor(A, shape[2])
    assert F_ref[0, 0] < 0  # sign(0) = +1: R_00 = -norm
    F, T = gpu_factor(tqr, A, shape[2])
    assert_close(F, T, F_ref, T_ref)


# ---- 3. accuracy on conditioned inputs -------------------------------------------------------
@pytest.mark.parametrize("shape", ACC_SHAPES, ids=lambda s: "%dx%db%d" % s)
@pytest.mark.parametrize("family", FAMILIES)
def test_accuracy_vs_longdouble(tqr, oracle, family, shape):
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    b = shape[2]
    A = inputs.matrix(family, shape)
    F_ref, T_ref = inputs.oracle_factor(oracle, family, shape)
    R_ld = inputs.r_longdouble(family, shape)
    F, T = gpu_factor(tqr, A, b)
    res = oracle.residual(A, F, T, b)
    cn = inputs.colnorm_rel_err(A, F)
    e_gpu, e_orc = inputs.col_rel_err(F, R_ld), inputs.col_rel_err(F_ref, R_ld)
    print(f"{family} {shape}: residual {res:.3e}, column norms {cn:.3e}, "
          f"e_gpu {e_gpu:.3e}, e_oracle {e_orc:.3e}, ratio {e_gpu / e_orc:.3f}")
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert res <= 1e-13
    assert cn <= 1e-12
    assert e_gpu <= 1.5 * e_orc
    if family == "gauss":
        assert_close(F, T, F_ref, T_ref)


@pytest.mark.parametrize("shape", SHAPES32, ids=lambda s: "%dx%db%d" % s)
def test_accuracy_fp32(tqr, oracle, shape):
    """fp32 storage: within 1e-4 max(1, max|F|) of the fp32 oracle (tau: 2e-4), and no farther
    from the fp64 oracle on the same fp32-valued input than 1.5 x the fp32 oracle is."""
    b = shape[2]
    A = inputs.matrix("gauss", shape, np.float32)
    F32, T32 = inputs.oracle_factor(oracle, "gauss", shape, np.float32)
    F64, _ = oracle.factor(A.astype(np.float64), b)
    F, T = gpu_factor(tqr, A, b)
    Fg = F.astype(np.float64)
    dF = float(np.abs(Fg - F32).max())
    dT = float(np.abs(T.astype(np.float64) - T32).max())
    e_gpu, e_ref = float(np.abs(Fg - F64).max()), float(np.abs(F32 - F64).max())
    print(f"fp32 gauss {shape}: max|dF| {dF:.3e} (max|F| {np.abs(F32).max():.3e}), max|dtau| {dT:.3e}, "
          f"vs fp64 oracle: GPU {e_gpu:.3e}, fp32 oracle {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}")
    assert dF <= 1e-4 * max(1.0, float(np.abs(F32).max()))
    assert dT <= 2e-4
    assert e_gpu <= 1.5 * e_ref


# ---- 4. device arrays ------------------------------------------------------------------------
DEV_CASES = [((192, 128, 64), np.float64), ((768, 512, 256), np.float64), ((768, 512, 256), np.float32)]
PAD_CASES = [(s, dt, pad) for s, dt in DEV_CASES for pad in ((8, 1) if dt == np.float64 else (4, 3))]
SENTINEL = -7.25

_plans = {}


def device_base(tqr, oracle, shape, dt):
    """(plan, F, tau) of the packed (ldda = m) default-stream run on the gauss matrix, as torch CPU
    tensors, checked against the oracle; the plan is the one every variant reuses."""
    import torch
    key = (shape, np.dtype(dt).name)
    m, n, b = shape
    if key not in _plans:
        tdt = torch.float64 if dt == np.float64 else torch.float32
        plan = tqr.TiledQR(m, n, b, tdt)
        dA = torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda()
        tau = torch.zeros((plan.kmax, m), dtype=tdt, device="cuda")
        plan.execute(dA, tau)
        plan.status()
        _plans[key] = (plan, dA.cpu(), tau.cpu())
    plan, F, tau = _plans[key]
    F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, dt)
    assert_close(F.numpy(), tqr.expand_tau(tau.numpy(), m, n, b), F_ref, T_ref)
    return plan, F, tau


@pytest.mark.parametrize("shape,dt,pad", PAD_CASES, ids=[f"{m}x{n}b{b}-{dtname(dt)}-ld+{p}" for (m, n, b), dt, p in PAD_CASES])
def test_padded_ldda(tqr, oracle, shape, dt, pad):
    import torch
    m, n, b = shape
    plan, F0, tau0 = device_base(tqr, oracle, shape, dt)
    ldda = m + pad
    buf = torch.full((n, ldda), SENTINEL, dtype=F0.dtype, device="cuda")
    buf[:, :m] = torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda()
    tau = torch.zeros_like(tau0, device="cuda")
    plan.execute(buf, tau, ldda=ldda)
    plan.status()
    out = buf.cpu()
    assert torch.all(out[:, m:] == SENTINEL), "the engine wrote into the padding rows m .. ldda-1"
    assert torch.equal(out[:, :m], F0) and torch.equal(tau.cpu(), tau0)


@pytest.mark.parametrize("shape,dt", DEV_CASES, ids=ids(DEV_CASES))
def test_offset_base(tqr, oracle, shape, dt):
    """A starts one element into its allocation: 8-byte (fp64) / 4-byte (fp32) aligned base."""
    import torch
    m, n, b = shape
    plan, F0, tau0 = device_base(tqr, oracle, shape, dt)
    big = torch.full((n * m + 2,), SENTINEL, dtype=F0.dtype, device="cuda")
    view = big[1:1 + n * m].view(n, m)
    view.copy_(torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda())
    assert view.data_ptr() == big.data_ptr() + big.element_size()
    tau = torch.zeros_like(tau0, device="cuda")
    plan.execute(view, tau)
    plan.status()
    out = big.cpu()
    assert out[0] == SENTINEL and out[-1] == SENTINEL
    assert torch.equal(out[1:-1].view(n, m), F0) and torch.equal(tau.cpu(), tau0)


@pytest.mark.parametrize("shape,dt", DEV_CASES, ids=ids(DEV_CASES))
def test_stream_and_plan_reuse(tqr, oracle, shape, dt):
    """One plan on a non-default stream: X, then Y (another seed), then X again. The third result is
    the first bit for bit (and both the default-stream one); the second is the oracle's factorisation
    of Y — nothing of one execute survives into the next."""
    import torch
    m, n, b = shape
    plan, F0, tau0 = device_base(tqr, oracle, shape, dt)
    X = inputs.matrix("gauss", shape, dt)
    Y = inputs.matrix("gauss", shape, dt, offset=7)
    s = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(s):
        for M in (X, Y, X):
            dA = torch.from_numpy(M.copy()).to("cuda", non_blocking=False)
            tau = torch.zeros_like(tau0, device="cuda")
            s.wait_stream(torch.cuda.default_stream())
            plan.execute(dA, tau, stream=s.cuda_stream)
            outs.append((dA, tau))
        plan.status(stream=s.cuda_stream)
    s.synchronize()
    (F1, t1), (F2, t2), (F3, t3) = [(a.cpu(), t.cpu()) for a, t in outs]
    assert torch.equal(F3, F1) and torch.equal(t3, t1)
    assert torch.equal(F1, F0) and torch.equal(t1, tau0)
    FY, TY = inputs.oracle_factor(oracle, "gauss", shape, dt, offset=7)
    assert_close(F2.numpy(), tqr.expand_tau(t2.numpy(), m, n, b), FY, TY)
