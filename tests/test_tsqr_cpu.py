"""The tall-skinny tree's reference (tests/tsqr_ref.py) on the CPU, composed from the oracle's tile
kernels: the model alone meets the conditions test_gpu_tsqr.py asks of the GPU, at the same shapes.

Bounds are the project's own: residual |Q^T A - [R; 0]|_F / |A|_F <= 1e-13 (oracle.residual's measure
and bound), column norms of R against A's to 1e-12 (test_gpu_inputs.py), and for the explicit thin Q
max|Q^T Q - I| <= 1e-11, max|Q R - A| <= 1e-11 * max(1, max|A|) (test_gpu_form_q.test_meaning)."""
import numpy as np
import pytest

import inputs
import tsqr_ref

# (m, n, b, m_dom, fan): the shapes of test_gpu_tsqr.py
SHAPES = [(256, 32, 16, 64, 2), (192, 32, 16, 64, 2), (640, 64, 32, 128, 4), (320, 32, 32, 32, 4),
          (1024, 128, 64, 256, 2), (1024, 128, 128, 256, 2), (2048, 256, 256, 512, 2), (64, 32, 16, 64, 2)]
LEVELS = {(256, 32, 16, 64, 2): [4, 2, 1], (192, 32, 16, 64, 2): [3, 2, 1], (640, 64, 32, 128, 4): [5, 2, 1],
          (320, 32, 32, 32, 4): [10, 3, 1], (1024, 128, 64, 256, 2): [4, 2, 1], (1024, 128, 128, 256, 2): [4, 2, 1],
          (2048, 256, 256, 512, 2): [4, 2, 1], (64, 32, 16, 64, 2): [1]}


def sid(s):
    return "{}x{}b{}d{}f{}".format(*s)


_fac = {}


def tree(oracle, shape):
    """(A, backend, factorised tree) of the Gaussian input at `shape`, computed once."""
    if shape not in _fac:
        m, n, b, m_dom, fan = shape
        A = inputs.matrix("gauss", (m, n, b))
        be = tsqr_ref.OracleBackend(oracle, b)
        _fac[shape] = (A, be, tsqr_ref.factor(A, b, m_dom, fan, be))
    return _fac[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_levels(shape):
    m, n, b, m_dom, fan = shape
    lv = tsqr_ref.levels_of(m, n, m_dom, fan)
    assert [d for _, d in lv] == LEVELS[shape]
    assert [r for r, _ in lv] == [m_dom] + [fan * n] * (len(lv) - 1)


def test_defaults():
    assert tsqr_ref.resolve(65536, 256, 256) == (1024, 4)
    assert tsqr_ref.resolve(65536, 512, 256) == (2048, 4)
    assert tsqr_ref.resolve(1048576, 64, 64) == (1024, 4), "4 n = 256 is below 1024 rows"
    assert tsqr_ref.resolve(3 * 1024, 64, 64) == (1024, 4)
    assert tsqr_ref.resolve(5 * 1024 + 512, 64, 64) == (1408, 4), "1024 .. 1344 do not divide 5632 = 4 * 1408"
    assert tsqr_ref.resolve(192, 32, 16) == (192, 4), "nothing from 1024 on is below m: one domain"
    assert tsqr_ref.resolve(16 * 7, 16, 16) == (112, 4), "m / b prime"
    assert tsqr_ref.resolve(1024, 32, 16, 64, 2) == (64, 2)


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_r_and_qt(oracle, shape):
    """Q^T A has R in rows 0 .. n-1 and zeros below, to the residual bound; R's column norms are A's."""
    m, n, b, m_dom, fan = shape
    A, be, fac = tree(oracle, shape)
    QtA, _ = tsqr_ref.apply(fac, A, True, be)
    R0 = np.zeros_like(A)
    R0[:, :n] = np.tril(fac["A"][:, :n])
    res = float(np.linalg.norm(QtA - R0) / np.linalg.norm(A))
    cn = inputs.colnorm_rel_err(A, fac["A"])
    print(f"{sid(shape)}: residual {res:.3e}, column norms {cn:.3e}, max|(Q^T A)[n:]| {np.abs(QtA[:, n:]).max():.3e}")
    assert res <= 1e-13
    assert cn <= 1e-12
    # below the diagonal of the leading block the final A still holds level 0's V, not R
    if len(fac["lv"]) > 1:
        low = ~np.tril(np.ones((n, n), dtype=bool))
        assert np.array_equal(fac["A"][:, :n][low], fac["lv"][0]["F"][:, :n][low])


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_thin_q(oracle, shape):
    m, n, b, m_dom, fan = shape
    A, be, fac = tree(oracle, shape)
    Q = tsqr_ref.form_q(fac, be)  # (n, m): row j = column j
    R = np.tril(fac["A"][:, :n])
    e_orth = float(np.abs(Q @ Q.T - np.eye(n)).max())
    e_qr = float(np.abs(R @ Q - A).max())
    print(f"{sid(shape)}: max|Q^T Q - I| = {e_orth:.3e}, max|Q R - A| = {e_qr:.3e} (max|A| {np.abs(A).max():.3e})")
    assert e_orth <= 1e-11
    assert e_qr <= 1e-11 * max(1.0, float(np.abs(A).max()))


@pytest.mark.parametrize("shape", [(192, 32, 16, 64, 2), (640, 64, 32, 128, 4), (320, 32, 32, 32, 4)], ids=sid)
def test_zero_blocks(oracle, shape):
    """Padding: the V_B of a zero block is exactly zero and its taus are finite; padded rows of C stay
    zero through the walk in both directions."""
    m, n, b, m_dom, fan = shape
    A, be, fac = tree(oracle, shape)
    padded = 0
    for l in range(1, len(fac["lv"])):
        L, prev = fac["lv"][l], fac["lv"][l - 1]["ndom"]
        for j in range(prev, L["ndom"] * fan):  # zero blocks of W_l: rows j n .. j n + n - 1
            padded += 1
            assert not fac["lv"][l]["W"][:, j * n:(j + 1) * n].any()
            assert not L["F"][:, j * n:(j + 1) * n].any(), f"level {l}, block {j}: V_B of a zero block"
            dom, off = divmod(j * n, L["rows"])
            T = L["aux"][dom]
            assert np.isfinite(T).all()
    assert padded > 0
    C = np.random.default_rng(3).standard_normal((5, m))
    for trans in (True, False):
        _, Cs = tsqr_ref.apply(fac, C, trans, be)
        for l in range(1, len(fac["lv"])):
            prev = fac["lv"][l - 1]["ndom"]
            assert not Cs[l][:, prev * n:].any(), f"level {l}: padded rows of C_l (trans={trans})"


@pytest.mark.parametrize("shape", [(640, 64, 32, 128, 4), (64, 32, 16, 64, 2)], ids=sid)
def test_q_qt_roundtrip(oracle, shape):
    m, n, b, m_dom, fan = shape
    A, be, fac = tree(oracle, shape)
    C = np.random.default_rng(4).standard_normal((5, m))
    back = tsqr_ref.apply(fac, tsqr_ref.apply(fac, C, True, be)[0], False, be)[0]
    assert np.abs(back - C).max() <= 1e-11 * max(1.0, float(np.abs(C).max()))
