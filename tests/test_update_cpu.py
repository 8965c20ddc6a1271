"""The row update's model (tests/update_ref.py) on the CPU: the separation identity that states the bit
contract of tqr_update_rows, the Gram relation, the diagonal-sign rule, and both apply identities.

The separation identity: in the flat-tree factorisation of the stacked S = [G; W] the tile operations on
the W rows never feed those on the G rows, and at step k they see G's own final R_kk and R_kj. So the
oracle's factorisation of S equals its factorisation of G followed by update_ref.update with W, byte for
byte — the upper triangle, the W rows (V) and their taus — and G's V is the same in both."""
import numpy as np
import pytest

import inputs
import update_ref

DTYPES = [np.float64, np.float32]
# |R'^T R' - R^T R - W^T W|_F / |R'^T R'|_F: a product of q * wt * b reflectors applied in the dtype, each
# within a few u; the observed errors are far below (5.5e-15 and 3.5e-6 on these shapes).
GRAM_BOUND = {np.float64: 1e-13, np.float32: 5e-5}


def stacked(oracle, b, q, wt, dt, seed=11):
    """S = [G; W] (RANDZO), its oracle factorisation, G's own, and W."""
    n, mw = q * b, wt * b
    S = oracle.randzo(n + mw, n, dt, seed=seed)
    G, W = np.ascontiguousarray(S[:, :n]), np.ascontiguousarray(S[:, n:])
    return S, oracle.factor(S, b), oracle.factor(G, b), G, W


@pytest.fixture(scope="module")
def cases(oracle):
    return {(b, q, wt, np.dtype(dt).name): stacked(oracle, b, q, wt, dt)
            for b, q, wt in update_ref.CPU_SHAPES for dt in DTYPES}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("b,q,wt", update_ref.CPU_SHAPES)
def test_separation_identity(oracle, cases, b, q, wt, dt):
    n = q * b
    S, (Fs, Ts), (Fg, Tg), G, W = cases[(b, q, wt, np.dtype(dt).name)]
    Rn, V, tau_u = update_ref.update(oracle, Fg, W, b)
    upper = np.tril(np.ones((n, n), dtype=bool))
    assert np.array_equal(inputs.bits(Rn[upper]), inputs.bits(Fs[:, :n][upper])), "upper triangle"
    assert np.array_equal(inputs.bits(V), inputs.bits(Fs[:, n:])), "V of the W rows"
    assert np.array_equal(inputs.bits(tau_u), inputs.bits(np.ascontiguousarray(Ts[0::b, n:]))), "taus of the W rows"
    # G's V: the same in the stacked factorisation, and untouched by the update
    assert np.array_equal(inputs.bits(Fg[~upper]), inputs.bits(Fs[:, :n][~upper]))
    assert np.array_equal(inputs.bits(Rn[~upper]), inputs.bits(Fg[~upper]))
    assert np.array_equal(inputs.bits(Tg), inputs.bits(np.ascontiguousarray(Ts[:, :n])))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("b,q,wt", update_ref.CPU_SHAPES)
def test_gram_and_diagonal_sign(oracle, cases, b, q, wt, dt):
    _, _, (Fg, _), _, W = cases[(b, q, wt, np.dtype(dt).name)]
    Rn, _, _ = update_ref.update(oracle, Fg, W, b)
    ld = np.longdouble
    R0, R1, Wm = inputs.upper(Fg).astype(ld), inputs.upper(Rn).astype(ld), W.T.astype(ld)
    lhs = R1.T @ R1
    err = float(np.linalg.norm(lhs - R0.T @ R0 - Wm.T @ Wm) / np.linalg.norm(lhs))
    print(f"b={b} q={q} wt={wt} {np.dtype(dt).name}: gram {err:.2e}")
    assert err <= GRAM_BOUND[dt]
    d0, d1 = np.diag(inputs.upper(Fg)), np.diag(inputs.upper(Rn))
    assert (d0 != 0).all()
    assert np.array_equal(np.sign(d1), np.sign(d0) * (-1) ** wt), "diag(R') = sign(diag(R)) (-1)^wt"


def test_update_ignores_what_lies_below_the_diagonal(oracle, cases):
    b, q, wt = 32, 3, 2
    _, _, (Fg, _), _, W = cases[(b, q, wt, "float64")]
    n = q * b
    Fn = Fg.copy()
    Fn[~np.tril(np.ones((n, n), dtype=bool))] = np.nan
    a, c = update_ref.update(oracle, Fg, W, b), update_ref.update(oracle, Fn, W, b)
    assert np.array_equal(inputs.bits(inputs.upper(a[0])), inputs.bits(inputs.upper(c[0])))
    assert np.array_equal(inputs.bits(a[1]), inputs.bits(c[1])) and np.array_equal(inputs.bits(a[2]), inputs.bits(c[2]))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("b,q,wt", update_ref.CPU_SHAPES)
def test_apply_identities(oracle, cases, b, q, wt, dt):
    """Q^T of the stacked factorisation = G's Q^T on the top rows, then Q_u^T; Q = Q_u, then G's Q. The
    step-k G operations and the step-(k-1) W operations touch disjoint row tiles, so they commute, and
    every reflector sees the same operands on both sides: the bytes agree."""
    n = q * b
    _, (Fs, Ts), (Fg, Tg), _, W = cases[(b, q, wt, np.dtype(dt).name)]
    _, V, tau_u = update_ref.update(oracle, Fg, W, b)
    C = inputs.rng_for((n + wt * b, n, b), 7).standard_normal((5, n + wt * b)).astype(dt)
    Ct, Cn = np.ascontiguousarray(C[:, :n]), np.ascontiguousarray(C[:, n:])
    # Q^T
    want = inputs.numpy_qt(Fs, Ts, C, b)
    t, c = update_ref.apply(V, tau_u, inputs.numpy_qt(Fg, Tg, Ct, b), Cn, b, trans=True)
    assert np.array_equal(inputs.bits(t), inputs.bits(np.ascontiguousarray(want[:, :n])))
    assert np.array_equal(inputs.bits(c), inputs.bits(np.ascontiguousarray(want[:, n:])))
    # Q
    want = inputs.numpy_q(Fs, Ts, C, b)
    t, c = update_ref.apply(V, tau_u, Ct, Cn, b, trans=False)
    t = inputs.numpy_q(Fg, Tg, t, b)
    assert np.array_equal(inputs.bits(t), inputs.bits(np.ascontiguousarray(want[:, :n])))
    assert np.array_equal(inputs.bits(c), inputs.bits(np.ascontiguousarray(want[:, n:])))
    # and Q_u (Q_u^T C) = C
    t, c = update_ref.apply(V, tau_u, *update_ref.apply(V, tau_u, Ct, Cn, b, trans=True), b, trans=False)
    u = np.finfo(dt).eps
    assert np.abs(np.concatenate([t, c], axis=1) - C).max() <= 64 * u * q * wt * b * np.abs(C).max()
