"""Capped plans (tqr_plan_create_steps, include/tqr.h) without a GPU: the task lists, the argument
checks, and what the reference arithmetic itself satisfies.

The list sweep is the deadlock-freedom evidence for the capped engine: every exported list is
topological for the engine's in-task waits (tqr_flow_order_check, the condition of flow.hpp's header)
and holds exactly the tasks of the first `steps` steps — panels (i, k) for k < steps, and for every step
the chains of ALL later tile columns, each strip's rows k+1 .. M-1 partitioned by its segments.
"""
import ctypes
import os

import numpy as np
import pytest

from steps_ref import partial

EINVAL = -1
F32, F64 = 0, 1
Z = ctypes.c_void_p(1)  # a non-NULL pointer that is never dereferenced: each call fails validation
T_CHAIN, QRS, QRD = 4, 0, 2
SMALL = [(M, N) for M in range(1, 13) for N in range(1, 13)]
LARGE = [(64, 64), (256, 64), (64, 128)]
LARGE_TASKS = 60000  # default run: the large grids' lists up to this many tasks (about a second each)
KNOBS = ("TQR_SEGLEN", "TQR_SEGLEN_LA", "TQR_LA_TAIL", "TQR_TAIL", "TQR_TAIL_SEGLEN", "TQR_UNMQR_ALONE", "TQR_LAZY",
         "TQR_LA", "TQR_LAC", "TQR_TG", "TQR_DIST_DEFAULTS", "TQR_DIST_PART", "TQR_FLOW_SHAPE")
ENVS = [{"TQR_TAIL": "3", "TQR_TAIL_SEGLEN": "2"}, {"TQR_UNMQR_ALONE": "0"}, {"TQR_LA_TAIL": "4"}, {"TQR_SEGLEN_LA": "2"}]


@pytest.fixture
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def check_list(tqr, items, M, N, b, steps, what):
    """Every property of one capped list (module docstring); vectorised, the large grids hold ~1e6 tasks."""
    n = len(items)
    assert n > 0, what
    arr = items.ctypes.data_as(ctypes.c_void_p)
    assert tqr.lib().tqr_flow_order_check(M, N, b, arr, n) == 1, what
    ns = -(-b // tqr.lib().tqr_flow_strip_width())
    it = items.astype(np.int64)
    ty, strip = it[:, 0] & 0xff, it[:, 0] >> 8
    ch = ty == T_CHAIN
    assert np.all(ch | (ty == QRS) | (ty == QRD)), what
    # panel tasks: exactly (i, k), k < steps, k <= i < M (GEQRT on the diagonal), each once
    pa = it[~ch]
    assert np.all(pa[:, 2] == pa[:, 3]) and np.all((pa[:, 0] == QRS) == (pa[:, 1] == pa[:, 3])), what
    want = np.array([(i, k) for k in range(steps) for i in range(k, M)], dtype=np.int64)
    got = pa[:, [1, 3]]
    got = got[np.lexsort((got[:, 0], got[:, 1]))]
    assert got.shape == want.shape and np.array_equal(got, want), what
    # chain tasks: step k < steps; (k, j, strip) exactly k < steps, k < j < N, strip < ns; the segments
    # e = 0, 1, .. of each partition rows k+1 .. M-1 in order (empty segments allowed: the lone UNMQR)
    c = it[ch]
    k, e, j, s = c[:, 3] & 0xffff, c[:, 3] >> 16, c[:, 2], strip[ch]
    i0, i1 = c[:, 1] & 0xffff, c[:, 1] >> 16
    nchains = sum(N - 1 - kk for kk in range(steps)) * ns
    if nchains == 0:
        assert len(c) == 0, what
    else:
        assert np.all(k < steps) and np.all((j > k) & (j < N)) and np.all((s >= 0) & (s < ns)), what
        o = np.lexsort((e, s, j, k))
        k, e, j, s, i0, i1 = k[o], e[o], j[o], s[o], i0[o], i1[o]
        key = (k * N + j) * ns + s
        first = np.r_[True, key[1:] != key[:-1]]
        last = np.r_[first[1:], True]
        assert int(first.sum()) == nchains and len(np.unique(key)) == nchains, what
        assert np.all(e[first] == 0) and np.all(e[~first] == e[:-1][~first[1:]] + 1), what
        assert np.all(i0 <= i1) and np.all(i0[first] == k[first] + 1) and np.all(i1[last] == M), what
        assert np.all(i0[~first] == i1[:-1][~first[1:]]), what
    assert n == len(want) + len(c), what


def all_steps(M, N):
    return range(1, min(M, N) + 1)


@pytest.mark.parametrize("b", [256, 32])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_small_grid_sweep(tqr, clean_env, dtype, b):
    """Every (M, N) in 1..12 x 1..12, every steps, seglen default / 1 / 2."""
    for (M, N) in SMALL:
        for seglen in (0, 1, 2):
            full = tqr.flow_list(M, N, b, dtype, seglen)
            for steps in all_steps(M, N):
                items = tqr.flow_list(M, N, b, dtype, seglen, steps=steps)
                check_list(tqr, items, M, N, b, steps, (M, N, b, dtype, seglen, steps))
                if steps == min(M, N):
                    assert np.array_equal(items, full), (M, N, b, dtype, seglen)
            assert np.array_equal(tqr.flow_list(M, N, b, dtype, seglen, steps=0), full)


@pytest.mark.parametrize("seglen", [0, 1, 2])
@pytest.mark.parametrize("b", [256, 32])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M,N", LARGE)
def test_large_grid_sweep(tqr, clean_env, M, N, dtype, b, seglen):
    """(64, 64), (256, 64) and (64, 128) tiles. These lists hold up to 10^6 tasks and the planner
    takes seconds for each, so every steps in 1 .. min(M, N) for all 36 cases is 44 minutes of one
    core: that sweep runs with TQR_STEPS_SWEEP=full in the environment (DESIGN.md §14 records its result).
    Without it each case takes the steps where something changes — 1, 2, 33 (M = 64: the first step
    of fp64's default one-element tail, flowplan.cpp default_tail), min - 1, min — as far as the list
    stays under LARGE_TASKS tasks, and always steps = 1."""
    kmax = min(M, N)
    ns = -(-b // tqr.lib().tqr_flow_strip_width())
    if os.environ.get("TQR_STEPS_SWEEP") == "full":
        cand = list(all_steps(M, N))
    else:
        sl = seglen or 8
        size = lambda s: sum(M - k + (N - 1 - k) * ns * (-(-(M - 1 - k) // sl) + 1) for k in range(s))  # noqa: E731
        cand = [s for s in (1, 2, 33, kmax - 1, kmax) if s == 1 or size(s) <= LARGE_TASKS]
    for steps in cand:
        items = tqr.flow_list(M, N, b, dtype, seglen, steps=steps)
        check_list(tqr, items, M, N, b, steps, (M, N, b, dtype, seglen, steps))
        if steps == kmax:  # tqr_flow_list_export's list item for item
            assert np.array_equal(items, tqr.flow_list(M, N, b, dtype, seglen))
            assert np.array_equal(items, tqr.flow_list(M, N, b, dtype, seglen, steps=0))


@pytest.mark.parametrize("env", ENVS, ids=["tail", "ualone", "la_tail", "seglen_la"])
def test_ordering_knobs_from_environment(tqr, clean_env, env):
    """The same with the ordering knobs that count steps back from the last one set through the
    environment: they count back from the capped last step, and every list stays valid."""
    for k, v in env.items():
        clean_env.setenv(k, v)
    for (M, N) in [(M, N) for M in (1, 2, 5, 8, 12) for N in (1, 3, 6, 9, 12)] + [(16, 6), (6, 16)]:
        for dtype in (F64, F32):
            for b in (256, 32):
                full = tqr.flow_list(M, N, b, dtype)
                for steps in all_steps(M, N):
                    items = tqr.flow_list(M, N, b, dtype, steps=steps)
                    check_list(tqr, items, M, N, b, steps, (env, M, N, b, dtype, steps))
                assert np.array_equal(items, full) and np.array_equal(tqr.flow_list(M, N, b, dtype, steps=0), full)


def test_knobs_count_back_from_the_cap(tqr, clean_env):
    """TQR_TAIL=1 with 8-row segments otherwise: at steps = 2 of an 12 x 6 grid the one-element segments
    are step 1's (the capped last step), not step 5's."""
    clean_env.setenv("TQR_TAIL", "1")
    clean_env.setenv("TQR_UNMQR_ALONE", "0")
    it = tqr.flow_list(12, 6, 32, F64, 8, steps=2).astype(np.int64)
    c = it[(it[:, 0] & 0xff) == T_CHAIN]
    k, rows = c[:, 3] & 0xffff, (c[:, 1] >> 16) - (c[:, 1] & 0xffff)
    assert set(rows[k == 0]) == {8, 3} and set(rows[k == 1]) == {1}


def test_export_steps_rejects(tqr):
    L = tqr.lib()
    spec = tqr.FlowListSpec(4, 6, 32, F64, 0, 1, -1, 1, 0, 0.0)
    assert L.tqr_flow_list_export_steps(ctypes.byref(spec), 5, None, 0) == EINVAL  # steps > min(M, N)
    assert L.tqr_flow_list_export_steps(None, 1, None, 0) == EINVAL
    two = tqr.FlowListSpec(4, 6, 32, F64, 0, 2, -1, 1, 0, 0.0)
    assert L.tqr_flow_list_export_steps(ctypes.byref(two), 2, None, 0) == EINVAL   # capped: world must be 1
    assert L.tqr_flow_list_export_steps(ctypes.byref(two), 0, None, 0) > 0
    xfer = tqr.FlowListSpec(4, 6, 32, F64, 0, 1, -1, 1, 2, 1.0)
    assert L.tqr_flow_list_export_steps(ctypes.byref(xfer), 2, None, 0) == EINVAL  # no host-pointer list


# (m, n, b, dtype, steps) — every call carries at least one invalid argument
BAD_CREATE = {
    "steps = 0": (256, 384, 64, F64, 0),
    "steps < 0": (256, 384, 64, F64, -1),
    "steps = min + 1": (256, 384, 64, F64, 5),
    "steps = min + 1 (tall)": (384, 256, 64, F32, 5),
    "b = 24": (96, 96, 24, F64, 1),
    "b = 0": (96, 96, 0, F64, 1),
    "bad dtype": (256, 384, 64, 2, 1),
    "b does not divide m": (100, 64, 32, F64, 1),
    "b does not divide n": (64, 100, 32, F64, 1),
    "m = 0": (0, 64, 32, F64, 1),
}


@pytest.mark.parametrize("why", sorted(BAD_CREATE))
def test_plan_create_steps_invalid_args_without_gpu(tqr, why):
    h = ctypes.c_void_p(7)
    assert tqr.lib().tqr_plan_create_steps(ctypes.byref(h), *BAD_CREATE[why]) == EINVAL, why
    assert h.value is None  # *plan is cleared


def test_null_plan_arguments_without_gpu(tqr):
    L = tqr.lib()
    assert L.tqr_plan_create_steps(None, 256, 384, 64, F64, 0) == EINVAL
    assert L.tqr_plan_create_steps(None, 256, 384, 64, F64, 1) == EINVAL
    assert L.tqr_plan_steps(None) == EINVAL
    assert L.tqr_lstsq_fused(None, Z, 256, Z, 1, None, None) == EINVAL
    assert L.tqr_lstsq_fused(None, Z, 256, Z, 0, Z, None) == EINVAL
    with pytest.raises(tqr.TQRError):
        tqr.TiledQR(256, 384, 64, F64, steps=0)


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("p,q,s", [(4, 6, 2), (6, 4, 3)])
def test_oracle_partial_is_a_prefix_and_resumes(oracle, p, q, s, dt):
    """What the GPU tests ask of a capped plan, the reference arithmetic meets by itself, bit for bit:
    (i) columns < s*b, and rows < s*b of every column, of partial(A, s) are those of oracle.factor(A)
        (with the taus of the steps < s);
    (ii) oracle.factor of the trailing block of partial(A, s) reproduces the rest of oracle.factor(A),
        R, V and tau.
    The tile kernels are position-independent and every tile sees the same operations on the same
    operands in the same order, whichever way the work is cut."""
    b = 32
    m, n = p * b, q * b
    A = oracle.randzo(m, n, dt, seed=5)
    F, T = oracle.factor(A, b)
    Fp, Tp = partial(oracle, A, b, s)
    assert np.array_equal(Fp[:s * b], F[:s * b]) and np.array_equal(Fp[:, :s * b], F[:, :s * b])
    assert np.array_equal(Tp[:s * b], T[:s * b]) and not Tp[s * b:].any()
    F2, T2 = oracle.factor(np.ascontiguousarray(Fp[s * b:, s * b:]), b)
    assert np.array_equal(F2, F[s * b:, s * b:]) and np.array_equal(T2, T[s * b:, s * b:])
