"""What test_gpu_segments.py relies on, shown without a GPU (tests/segments.py).

1. Coverage. Each case's exported task list holds every regime the case is listed for, the cases
   together hold all of them, and the default-knob fp64 lists of the shapes the other test files use
   (inputs.SHAPES, inputs.ACC_SHAPES) hold no task with two TSMQR elements: whoever changes
   default_tail (csrc/flowplan.cpp) learns here which tests changed meaning.
2. regimes() itself, on hand-made lists.
3. The numeric conditions on the oracle alone, as test_inputs_cpu.py shows them at its shapes:
   column scaling bit for bit, residual and column norms on the conditioned families, the
   extended-precision error at the b = 64 shapes.
"""
import ctypes

import numpy as np
import pytest

import inputs
import segments as S
from segments import BY_NAME, CASES


@pytest.fixture(scope="module")
def lists(tqr):
    return {c.name: S.export(tqr, c) for c in CASES}


def reached(tqr, case, items, **kw):
    p, q = case.tiles
    return S.regimes(p, q, case.shape[2], items, grid=case.grid, tqr=tqr, **kw)


# ---- 1. coverage -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_reaches_its_regimes(tqr, lists, case):
    got = reached(tqr, case, lists[case.name])
    print(f"{case.name} {case.shape} {case.env}: {len(lists[case.name])} tasks on {case.grid} workgroups: {sorted(got)}")
    assert set(case.reach) <= got, sorted(set(case.reach) - got)
    p, q = case.tiles
    items = lists[case.name]
    assert tqr.lib().tqr_flow_order_check(p, q, case.shape[2], items.ctypes.data_as(ctypes.c_void_p), len(items)) == 1


def test_every_regime_is_reached(tqr, lists):
    union = set()
    for c in CASES:
        union |= reached(tqr, c, lists[c.name])
    assert union == set(S.REGIMES), sorted(set(S.REGIMES) - union)


def test_default_case_sets_no_knob():
    """D64 and D256 reach their regimes with the environment empty: the default list of p = 34."""
    assert BY_NAME["D64"].env == {} and BY_NAME["D256"].env == {}
    assert BY_NAME["D64"].tiles[0] == 34 and BY_NAME["D256"].tiles[0] == 34


@pytest.mark.parametrize("shape", sorted(set(inputs.SHAPES + inputs.ACC_SHAPES)), ids=lambda s: "%dx%db%d" % s)
def test_old_default_lists_hold_no_multi_element_segment(tqr, shape):
    m, n, b = shape
    with S.knobs():
        items = tqr.flow_list(m // b, n // b, b, tqr.TQR_F64)
    got = S.regimes(m // b, n // b, b, items, tqr=tqr)
    assert not got & set(S.MULTI), sorted(got)


def test_all_tail_lists_hold_no_multi_element_segment(tqr):
    """The plans every case is compared with bit for bit (ALL_TAIL): one TSMQR per task at most."""
    for c in CASES:
        got = reached(tqr, c, S.export(tqr, c, env=S.ALL_TAIL))
        assert not got & set(S.MULTI) and "lines_handover" not in got, (c.name, sorted(got))


def test_task_counts_of_the_planner(tqr, lists):
    """The counts the planner gives for the lists named in DESIGN.md §5.1."""
    with S.knobs():
        assert len(tqr.flow_list(10, 2, 128, tqr.TQR_F64)) == 29
    assert len(lists["T0-128"]) == 21
    with S.knobs():
        assert len(tqr.flow_list(10, 2, 128, tqr.TQR_F32)) == 21
    assert len(lists["D64"]) == 185


def test_capped_lists_keep_the_segments(tqr):
    """The capped plans of test_gpu_segments.py (T0's shape, 2 and 3 steps, TQR_TAIL=0): their lists
    hold the multi-element regimes too, whole-line hand-overs at step 1 included."""
    c = BY_NAME["T0"]
    p, q = c.tiles
    for steps in (2, 3):
        got = S.regimes(p, q, c.shape[2], S.export(tqr, c, steps=steps), steps=steps, tqr=tqr)
        assert {"handover", "full0", "rem1", "lines_handover"} <= got, (steps, sorted(got))


def test_knobs_restores_the_environment(monkeypatch):
    import os
    monkeypatch.setenv("TQR_TAIL", "5")
    monkeypatch.delenv("TQR_SEGLEN", raising=False)
    with S.knobs({"TQR_SEGLEN": "3"}):
        assert "TQR_TAIL" not in os.environ and os.environ["TQR_SEGLEN"] == "3"
    assert os.environ["TQR_TAIL"] == "5" and "TQR_SEGLEN" not in os.environ


def test_transfer_lists_hold_the_device_lists_chains(tqr, lists):
    """The host-pointer path's list (UP / DOWN tasks, the estimator's order) is built from the plan's
    own knobs: under T0's and MIX's knobs its chain and panel tasks are the device list's (as a set;
    the deep-lookahead pass does not run on transfer lists), so xfer.hpp's column-final counts, which
    recompute the segments from those knobs, count the tasks that exist."""
    for name in ("T0", "MIX"):
        c = BY_NAME[name]
        p, q = c.tiles
        x = S.export(tqr, c, nxc=2, tcol=2.5)
        assert tqr.lib().tqr_flow_order_check(p, q, c.shape[2], x.ctypes.data_as(ctypes.c_void_p), len(x)) == 1
        core = [tuple(r) for r in x.tolist() if r[0] & 0xff not in (5, 6)]
        assert len(x) - len(core) == 2 * 2 * q
        assert sorted(core) == sorted(map(tuple, lists[name].tolist()))
        assert S.chains(x) == S.chains(lists[name])


# ---- 2. regimes() on hand-made lists ------------------------------------------------------------
def chain_item(k, j, e, i0, i1, s=0):
    return [S.T_CHAIN | (s << 8), i0 | (i1 << 16), j, k | (e << 16)]


def test_regimes_on_handmade_lists(tqr):
    p, q, b = 12, 3, 64
    one = [chain_item(0, 1, 0, 1, 1)] + [chain_item(0, 1, e, e, e + 1) for e in range(1, 12)]  # UNMQR alone, 11 x 1
    assert S.regimes(p, q, b, np.array(one)) == set()
    assert S.segmentation(p, 0, S.chains(np.array(one))[(0, 1, 0)]) == (True, 1)
    full = [chain_item(0, 2, 0, 1, 9), chain_item(0, 2, 1, 9, 12)]  # UNMQR + 8, then 3
    assert S.regimes(p, q, b, np.array(full)) == {"handover", "full0"}
    rem = [chain_item(0, 2, 0, 1, 6), chain_item(0, 2, 1, 6, 11), chain_item(0, 2, 2, 11, 12)]  # 5 + 5 + 1
    assert S.regimes(p, q, b, np.array(rem)) == {"handover", "rem1"}
    assert S.regimes(p, q, b, np.array(one + rem)) == {"handover", "rem1", "la_own"}
    assert S.regimes(p, q, b, np.array(rem), grid=1) == {"handover", "rem1"}  # 3 tasks on one workgroup
    eight = [chain_item(0, 2, 0, 1, 2)] + [chain_item(0, 2, e, e + 1, e + 2) for e in range(1, 11)]
    assert "queued" in S.regimes(p, q, b, np.array(eight), grid=1) and "queued" not in S.regimes(p, q, b, np.array(eight), grid=2)
    with pytest.raises(AssertionError):  # rows that are not runs of one length
        S.regimes(p, q, b, np.array([chain_item(0, 2, 0, 1, 6), chain_item(0, 2, 1, 6, 8), chain_item(0, 2, 2, 8, 12)]))
    with pytest.raises(AssertionError):  # a missing segment
        S.regimes(p, q, b, np.array([chain_item(0, 2, 0, 1, 6), chain_item(0, 2, 2, 11, 12)]))


def test_lines_handover_follows_the_strip_layout(tqr):
    """b = 256 only, steps k >= 1 only (a step-0 strip is the caller's: standard), and not in a capped
    plan's view of a step it does not have."""
    p, q = 10, 4
    step0 = np.array([chain_item(0, 3, 0, 1, 9), chain_item(0, 3, 1, 9, 10)])
    step1 = np.array([chain_item(1, 3, 0, 2, 10)])
    assert "lines_handover" not in S.regimes(p, q, 256, step0, tqr=tqr)
    assert "lines_handover" in S.regimes(p, q, 256, step1, tqr=tqr)
    assert "lines_handover" not in S.regimes(p, q, 128, step1, tqr=tqr)
    assert "lines_handover" not in S.regimes(p, q, 256, np.array([chain_item(1, 2, 0, 2, 10)]), tqr=tqr)  # lookahead column


# ---- 3. the numeric conditions on the oracle alone ------------------------------------------------
def test_threaded_oracle_gives_the_serial_bits(oracle):
    shape = BY_NAME["T0-3seg"].shape
    A = S.randzo(oracle, shape)
    F, T = S.randzo_ref(oracle, shape)
    F1, T1 = oracle.factor(A, shape[2])
    assert np.array_equal(F, F1) and np.array_equal(T, T1)


@pytest.mark.parametrize("name", S.SCALE_CASES)
def test_oracle_column_scaling_bitexact(oracle, name):
    shape = BY_NAME[name].shape
    A = inputs.matrix("gauss", shape)
    d = inputs.scaling(shape, np.float64)
    assert np.abs(A).min() > 0
    assert inputs.in_normal_range(inputs.scale_columns(A, d))
    F, T = S.family_ref(oracle, "gauss", shape)
    Fs, Ts = oracle.factor(inputs.scale_columns(A, d), shape[2], threads=8)
    inputs.assert_covariant(F, T, Fs, Ts, d)


@pytest.mark.parametrize("name", S.LD_CASES + S.FAMILY_CASES_256)
@pytest.mark.parametrize("family", S.CONDITIONED)
def test_oracle_accuracy(oracle, family, name):
    shape = BY_NAME[name].shape
    A = inputs.matrix(family, shape)
    F, T = S.family_ref(oracle, family, shape)
    res = oracle.residual(A, F, T, shape[2])
    cn = inputs.colnorm_rel_err(A, F)
    print(f"{family} {shape}: oracle residual {res:.2e}, column norms {cn:.2e}")
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert res <= 1e-13
    assert cn <= 1e-12
    if name in S.LD_CASES and inputs.have_longdouble():
        e = inputs.col_rel_err(F, inputs.r_longdouble(family, shape))
        print(f"{family} {shape}: e_oracle {e:.2e}")
        assert np.isfinite(e) and e < 1e-13


def test_oracle_structured_and_zero_pivot(oracle):
    """T0's shape: the structured family has reflectors with tau = 2 and an exactly zero diagonal entry
    of R; a zero first pivot of either sign is taken as +0."""
    shape = BY_NAME["T0"].shape
    F, T = S.family_ref(oracle, "structured", shape)
    n = shape[1]
    assert np.isfinite(F).all() and (T == 2.0).sum() >= 5
    assert (np.diag(F[:, :n]) == 0).sum() >= 1
    # the copy of column 3 is rounding noise below row 3 once column 3 is eliminated: its pivot, which
    # decides the reflector's direction, is some 1e-16 of the column's norm — so the GPU test compares the
    # columns before it with the oracle (and the whole result with the all-tail plan, bit for bit)
    c = n // 2 + 6
    A = inputs.matrix("structured", shape)
    print(f"structured {shape}: |R[c, c]| / |A[:, c]| = {abs(F[c, c]) / np.linalg.norm(A[c]):.2e}")
    assert np.array_equal(A[c], A[3]) and abs(F[c, c]) <= 1e-13 * np.linalg.norm(A[c])
    outs = []
    for zero in (0.0, -0.0):
        F0, T0 = S.zero_pivot_ref(oracle, shape, zero)
        # sign(0) = +1 in GEQRT (R_00 = -norm), and each of the p - 1 TSQRTs below flips the sign again
        assert (F0[0, 0] < 0) == ((shape[0] // shape[2]) % 2 == 1)
        outs.append((F0, T0))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
