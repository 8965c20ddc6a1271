"""The conditions test_gpu_inputs.py relies on, shown for the oracle alone (no GPU): with the same
generators, shapes and seeds (tests/inputs.py) the oracle's factorisation is bit-exactly covariant
under column scaling, meets the residual and column-norm bounds on the conditioned families, and
sits within 1e-13 (column-relative) of the extended-precision QR. It also runs the generators and
the longdouble QR where there is no GPU."""
import numpy as np
import pytest

import inputs
from inputs import ACC_SHAPES, FAMILIES, SHAPES, SHAPES32, WAVE_ACC_SHAPES, WAVE_ACC_SHAPES32, WAVE_SHAPES, dtname

# (the wave engine's shapes, test_gpu_waves.py, run in both dtypes at every shape)
SCALE_CASES = [(s, np.float64) for s in SHAPES] + [(s, np.float32) for s in SHAPES32] + \
              [(s, dt) for s in WAVE_SHAPES for dt in (np.float64, np.float32)]


@pytest.mark.parametrize("shape,dt", SCALE_CASES, ids=[f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in SCALE_CASES])
def test_oracle_column_scaling_bitexact(oracle, shape, dt):
    A = inputs.matrix("gauss", shape, dt)
    d = inputs.scaling(shape, dt)
    assert np.abs(A).min() > 0  # no zero pivot: sign(x0) flips with the column
    assert inputs.in_normal_range(inputs.scale_columns(A, d))  # the scaling itself is exact
    F, T = inputs.oracle_factor(oracle, "gauss", shape, dt)
    Fs, Ts = oracle.factor(inputs.scale_columns(A, d), shape[2])
    inputs.assert_covariant(F, T, Fs, Ts, d)


@pytest.mark.parametrize("e", [480, -480])
def test_oracle_global_factor_bitexact(oracle, e):
    shape = (192, 128, 64)
    A = inputs.matrix("gauss", shape)
    d = np.full(shape[1], np.ldexp(1.0, e))
    F, T = inputs.oracle_factor(oracle, "gauss", shape)
    Fs, Ts = oracle.factor(inputs.scale_columns(A, d), shape[2])
    inputs.assert_covariant(F, T, Fs, Ts, d)


def test_generators():
    m, n, b = shape = (192, 128, 64)
    for fam, lo, hi in [("gauss", 1.0, 1e2), ("rowgraded", 1e6, 1e10), ("cond1e8", 0.9e8, 1.1e8)]:
        A = inputs.matrix(fam, shape)
        assert A.shape == (n, m) and A.dtype == np.float64 and not A.flags.writeable
        assert lo <= np.linalg.cond(A) <= hi, fam
    assert not np.array_equal(inputs.matrix("gauss", shape), inputs.matrix("gauss", shape, offset=7))
    for dt in (np.float64, np.float32):
        d = inputs.scaling(shape, dt)
        mant, ex = np.frexp(d.astype(np.float64))
        assert d.dtype == dt and np.all(np.abs(mant) == 0.5)
        assert (ex - 1).min() >= -inputs.KMAX[np.dtype(dt)] and (ex - 1).max() <= inputs.KMAX[np.dtype(dt)]
        assert (d < 0).any() and (d > 0).any()


def test_qr_longdouble_small():
    """The reference against numpy's QR at a size where both are far inside 1e-14."""
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    A = inputs.matrix("gauss", (96, 64, 32))
    R = inputs.qr_longdouble(A)
    Rn = np.linalg.qr(A.T, mode="r")
    assert np.abs(np.abs(R.astype(np.float64)) - np.abs(Rn)).max() <= 1e-13 * np.abs(Rn).max()
    assert np.all(np.tril(R, -1) == 0)


@pytest.mark.parametrize("shape", ACC_SHAPES + WAVE_ACC_SHAPES, ids=lambda s: "%dx%db%d" % s)
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_accuracy(oracle, family, shape):
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    A = inputs.matrix(family, shape)
    F, T = inputs.oracle_factor(oracle, family, shape)
    res = oracle.residual(A, F, T, shape[2])
    cn = inputs.colnorm_rel_err(A, F)
    e = inputs.col_rel_err(F, inputs.r_longdouble(family, shape))
    print(f"{family} {shape}: oracle residual {res:.2e}, column norms {cn:.2e}, e_oracle {e:.2e}")
    assert res <= 1e-13
    assert cn <= 1e-12
    assert np.isfinite(e) and e < 1e-13


@pytest.mark.parametrize("shape", WAVE_ACC_SHAPES32, ids=lambda s: "%dx%db%d" % s)
def test_oracle_fp32_reference_error(oracle, shape):
    """test_gpu_waves.py bounds the fp32 wave engine by 1.5 x the fp32 oracle's distance from the fp64
    oracle on the same fp32-valued input: that distance is a positive number far inside the 1e-4 scale."""
    A = inputs.matrix("gauss", shape, np.float32)
    F32, _ = inputs.oracle_factor(oracle, "gauss", shape, np.float32)
    F64, _ = oracle.factor(A.astype(np.float64), shape[2])
    e_ref = float(np.abs(F32 - F64).max())
    print(f"fp32 gauss {shape}: fp32 oracle vs fp64 oracle {e_ref:.3e} (max|F| {np.abs(F32).max():.3e})")
    assert 0 < e_ref <= 1e-4 * max(1.0, float(np.abs(F32).max()))
