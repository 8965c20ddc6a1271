"""The row update's C ABI (include/tqr.h "row update") without a GPU: the symbols, every argument error
before any device call, a handle without a device, and the schedule of tqr_update_plan /
tqr_update_level_items against a brute-force dependency graph of the update's tile operations.

The file also runs where a GPU is present, so a made-up pointer only ever travels with at least one
invalid argument."""
import ctypes
import itertools

import pytest

import update_ref
from conftest import gpu_available

EINVAL, ENODEV = -1, -4
F32, F64 = 0, 1
P = ctypes.c_void_p
Z = P(1)  # a non-NULL pointer that is never dereferenced: each call that carries it fails validation
BS = [16, 32, 64, 128, 256]

SYMBOLS = ["tqr_update_create", "tqr_update_workspace_bytes", "tqr_update_rows", "tqr_update_prepare",
           "tqr_update_apply_q", "tqr_update_lstsq", "tqr_update_destroy", "tqr_update_plan", "tqr_update_level_items"]

# (n, mw, b, dtype)
BAD_CREATE = {
    "bad dtype": (64, 32, 32, 2),
    "b = 24": (96, 48, 24, F64),
    "b = 512": (1024, 512, 512, F64),
    "b does not divide n": (100, 64, 32, F64),
    "b does not divide mw": (128, 100, 32, F64),
    "n = 0": (0, 64, 32, F64),
    "n < 0": (-64, 64, 32, F64),
    "mw = 0": (64, 0, 32, F64),
    "mw < 0": (64, -32, 32, F64),
    "n beyond the leading-dimension bound (fp64)": (8388608, 256, 256, F64),
    "mw beyond the leading-dimension bound (fp32)": (256, 16777216, 256, F32),
}
LD_MAX = 8388607  # fp64


def test_symbols(tqr):
    for s in SYMBOLS:
        assert hasattr(tqr.lib(), s), s
    for s in ("RowUpdate", "update_plan", "update_level_items"):
        assert hasattr(tqr, s), s


@pytest.mark.parametrize("why", sorted(BAD_CREATE))
def test_create_invalid_args(tqr, why):
    h = P(12345)
    assert tqr.lib().tqr_update_create(ctypes.byref(h), *BAD_CREATE[why]) == EINVAL, why
    assert h.value is None, "no handle is returned with an error"


@pytest.mark.parametrize("why", [w for w in sorted(BAD_CREATE) if "dtype" not in w and "bound" not in w])
def test_plan_invalid_args(tqr, why):
    n, mw, b, _ = BAD_CREATE[why]
    out = [ctypes.c_int(-7) for _ in range(4)]
    assert tqr.lib().tqr_update_plan(n, mw, b, *(ctypes.byref(o) for o in out)) == EINVAL
    assert [o.value for o in out] == [-7] * 4, "a refused call writes nothing"
    buf = (ctypes.c_int * 8)(*([-7] * 8))
    assert tqr.lib().tqr_update_level_items(n, mw, b, 0, buf, 2) == EINVAL
    assert list(buf) == [-7] * 8


def test_level_items_invalid_level(tqr):
    buf = (ctypes.c_int * 8)()
    L = tqr.lib()
    nl = tqr.update_plan(64, 32, 32)[0]
    assert nl == 3
    assert L.tqr_update_level_items(64, 32, 32, -1, buf, 2) == EINVAL
    assert L.tqr_update_level_items(64, 32, 32, nl, buf, 2) == EINVAL
    assert L.tqr_update_level_items(64, 32, 32, 0, buf, -1) == EINVAL
    assert L.tqr_update_level_items(64, 32, 32, 0, None, 2) == EINVAL
    assert L.tqr_update_level_items(64, 32, 32, 0, None, 0) == 1, "cap = 0 counts only"


@pytest.fixture(scope="module")
def handle(tqr):
    """n = 64, mw = 32, b = 16, fp64 (q = 4, wt = 2), with or without a device."""
    h = P()
    assert tqr.lib().tqr_update_create(ctypes.byref(h), 64, 32, 16, F64) == 0
    assert h.value
    yield h
    tqr.lib().tqr_update_destroy(h)


def test_null_out_and_null_handle(tqr):
    L = tqr.lib()
    assert L.tqr_update_create(None, 64, 32, 32, F64) == EINVAL
    assert L.tqr_update_workspace_bytes(None) == 0
    assert L.tqr_update_rows(None, Z, 64, Z, 32, Z, None) == EINVAL
    assert L.tqr_update_prepare(None, Z, 32, Z, None) == EINVAL
    assert L.tqr_update_apply_q(None, 1, Z, 32, Z, 64, Z, 32, 1, None) == EINVAL
    assert L.tqr_update_lstsq(None, Z, 64, Z, 32, Z, Z, 64, Z, 32, 1, Z, 64, None, None) == EINVAL
    L.tqr_update_destroy(None)  # a no-op


def test_create_workspace_destroy(tqr, handle):
    """Two sets of T images: q * wt tiles, one 16 x 17 image padded to 384 doubles per tile (b = 16)."""
    assert tqr.lib().tqr_update_workspace_bytes(handle) == 2 * (4 * 2) * 1 * 384 * 8
    h = P()
    assert tqr.lib().tqr_update_create(ctypes.byref(h), 512, 256, 256, F32) == 0
    assert tqr.lib().tqr_update_workspace_bytes(h) == 2 * (2 * 1) * 8 * 1152 * 8
    tqr.lib().tqr_update_destroy(h)


# the handle is for n = 64, mw = 32: rows(dR, lddr, dW, lddw, dtau)
BAD_ROWS = {
    "NULL dR": (None, 64, Z, 32, Z),
    "NULL dW": (Z, 64, None, 32, Z),
    "NULL dtau_u": (Z, 64, Z, 32, None),
    "lddr < n": (Z, 63, Z, 32, Z),
    "lddw < mw": (Z, 64, Z, 31, Z),
    "lddr beyond the bound": (Z, LD_MAX + 1, Z, 32, Z),
    "lddw beyond the bound": (Z, 64, Z, LD_MAX + 1, Z),
}


@pytest.mark.parametrize("why", sorted(BAD_ROWS))
def test_rows_invalid_args(tqr, handle, why):
    assert tqr.lib().tqr_update_rows(handle, *BAD_ROWS[why], None) == EINVAL, why


@pytest.mark.parametrize("why,args", [
    ("NULL dW", (None, 32, Z)), ("NULL dtau_u", (Z, 32, None)), ("lddw < mw", (Z, 31, Z)),
    ("lddw beyond the bound", (Z, LD_MAX + 1, Z))])
def test_prepare_invalid_args(tqr, handle, why, args):
    assert tqr.lib().tqr_update_prepare(handle, *args, None) == EINVAL, why


# apply_q(trans, dW, lddw, dCtop, lddct, dCnew, lddcn, nrhs)
BAD_APPLY = {
    "bad trans": (2, Z, 32, Z, 64, Z, 32, 3),
    "negative trans": (-1, Z, 32, Z, 64, Z, 32, 3),
    "NULL dW": (1, None, 32, Z, 64, Z, 32, 3),
    "NULL dCtop": (1, Z, 32, None, 64, Z, 32, 3),
    "NULL dCnew": (1, Z, 32, Z, 64, None, 32, 3),
    "nrhs = 0": (1, Z, 32, Z, 64, Z, 32, 0),
    "nrhs < 0": (0, Z, 32, Z, 64, Z, 32, -3),
    "lddw < mw": (1, Z, 31, Z, 64, Z, 32, 3),
    "lddct < n": (1, Z, 32, Z, 63, Z, 32, 3),
    "lddcn < mw": (1, Z, 32, Z, 64, Z, 31, 3),
    "lddw beyond the bound": (1, Z, LD_MAX + 1, Z, 64, Z, 32, 3),
    "lddct beyond the bound": (1, Z, 32, Z, LD_MAX + 1, Z, 32, 3),
    "lddcn beyond the bound": (0, Z, 32, Z, 64, Z, LD_MAX + 1, 3),
}


@pytest.mark.parametrize("why", sorted(BAD_APPLY))
def test_apply_invalid_args(tqr, handle, why):
    assert tqr.lib().tqr_update_apply_q(handle, *BAD_APPLY[why], None) == EINVAL, why


def test_apply_before_prepare(tqr):
    """Valid arguments, but nothing was prepared: TQR_EINVAL and no device call (on a fresh handle)."""
    h = P()
    assert tqr.lib().tqr_update_create(ctypes.byref(h), 64, 32, 16, F64) == 0
    assert tqr.lib().tqr_update_apply_q(h, 1, Z, 32, Z, 64, Z, 32, 3, None) == EINVAL
    tqr.lib().tqr_update_destroy(h)


# lstsq(dR, lddr, dW, lddw, dtau, dD, lddd, dBnew, lddb, nrhs, dX, lddx, dres)
GOOD_LSTSQ = [Z, 64, Z, 32, Z, Z, 64, Z, 32, 3, Z, 64, None]
BAD_LSTSQ = {
    "NULL dR": {0: None}, "NULL dW": {2: None}, "NULL dtau_u": {4: None}, "NULL dD": {5: None},
    "NULL dBnew": {7: None}, "NULL dX": {10: None}, "lddr < n": {1: 63}, "lddw < mw": {3: 31},
    "lddd < n": {6: 63}, "lddb < mw": {8: 31}, "lddx < n": {11: 63}, "nrhs = 0": {9: 0}, "nrhs < 0": {9: -1},
    "lddr beyond the bound": {1: LD_MAX + 1}, "lddw beyond the bound": {3: LD_MAX + 1},
    "lddd beyond the bound": {6: LD_MAX + 1}, "lddb beyond the bound": {8: LD_MAX + 1},
    "lddx beyond the bound": {11: LD_MAX + 1},
}


@pytest.mark.parametrize("why", sorted(BAD_LSTSQ))
def test_lstsq_invalid_args(tqr, handle, why):
    args = list(GOOD_LSTSQ)
    for i, v in BAD_LSTSQ[why].items():
        args[i] = v
    assert tqr.lib().tqr_update_lstsq(handle, *args, None) == EINVAL, why


def test_valid_calls(tqr, handle):
    """Arguments that are all valid. Without a GPU: TQR_ENODEV, i.e. validation passed and no device call
    was made. With one: the calls run on real buffers (R = I, W = 0) and return TQR_OK."""
    L = tqr.lib()
    if not gpu_available():
        assert L.tqr_update_rows(handle, Z, 64, Z, 32, Z, None) == ENODEV
        assert L.tqr_update_prepare(handle, Z, 32, Z, None) == ENODEV
        assert L.tqr_update_lstsq(handle, *GOOD_LSTSQ, None) == ENODEV
        return
    import torch
    R = torch.eye(64, dtype=torch.float64, device="cuda")
    W = torch.zeros((64, 32), dtype=torch.float64, device="cuda")
    tau = torch.zeros((4, 32), dtype=torch.float64, device="cuda")
    D, X = (torch.zeros((3, 64), dtype=torch.float64, device="cuda") for _ in range(2))
    Bn = torch.zeros((3, 32), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: P(t.data_ptr())
    assert L.tqr_update_rows(handle, p(R), 64, p(W), 32, p(tau), None) == 0
    assert L.tqr_update_prepare(handle, p(W), 32, p(tau), None) == 0
    assert L.tqr_update_lstsq(handle, p(R), 64, p(W), 32, p(tau), p(D), 64, p(Bn), 32, 3, p(X), 64, None, None) == 0
    torch.cuda.synchronize()


# ---- the schedule --------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BS)
def test_schedule_against_brute_force_dag(tqr, b):
    """Over all q, wt <= 6: each item of the serial order appears exactly once; every dependency of the
    brute-force graph lies on a strictly earlier level; the items of one level are pairwise disjoint in
    what they write and in what one writes and another reads; the counts and nlaunch are consistent."""
    ns = (b + 63) // 64
    for q, wt in itertools.product(range(1, 7), range(1, 7)):
        n, mw = q * b, wt * b
        nlevels, npanel, nupdate, nlaunch = tqr.update_plan(n, mw, b)
        tasks = update_ref.serial_tasks(q, wt, ns)
        index = {t: i for i, t in enumerate(tasks)}
        level_of = {}
        launches = 1  # the closing T pass
        tot_p = tot_u = 0
        for L in range(nlevels):
            items = tqr.update_level_items(n, mw, b, L)
            assert items, f"level {L} of q={q} wt={wt} is empty"
            types = [it[0] for it in items]
            np_ = types.count(update_ref.QRD)
            assert types == [update_ref.QRD] * np_ + [update_ref.DAPP] * (len(items) - np_), "TSQRT items first"
            launches += (np_ > 0) + (len(items) > np_)
            tot_p += np_
            tot_u += len(items) - np_
            for it in items:
                assert it in index, f"{it} is no task of the update"
                assert it not in level_of, f"{it} appears twice"
                level_of[it] = L
        assert len(level_of) == len(tasks), "every task appears"
        assert (tot_p, tot_u, launches) == (npanel, nupdate, nlaunch)
        assert npanel == q * wt and nupdate == ns * wt * q * (q - 1) // 2
        assert nlevels == 2 * q + wt - 2
        # dependencies on strictly earlier levels
        for a, c in update_ref.brute_force_deps(tasks, ns):
            assert level_of[tasks[a]] < level_of[tasks[c]], f"{tasks[c]} needs {tasks[a]} (q={q} wt={wt})"
        # one level: no resource written by one item and touched by another
        touched = {}
        for t in tasks:
            rd, wr = update_ref.accesses(t, ns)
            for r in rd | wr:
                touched.setdefault((level_of[t], r), []).append(r in wr)
        for (L, r), ws in touched.items():
            assert len(ws) == 1 or not any(ws), f"level {L}: {r} is written by one item and touched by another"


def test_brute_force_dag_finds_the_chains():
    """The checker itself: TSQRT(1,0) needs TSQRT(0,0) (R_00), TSMQR(0,1,0) needs TSQRT(0,0) (V, T), and
    TSQRT(0,1) needs TSMQR(0,1,0) (W_01) — and the two strips of a TSMQR are independent."""
    tasks = update_ref.serial_tasks(2, 2, 2)
    idx = {t: i for i, t in enumerate(tasks)}
    deps = update_ref.brute_force_deps(tasks, 2)
    Q, D = update_ref.QRD, update_ref.DAPP
    assert (idx[(Q, 0, 0, 0, 0)], idx[(Q, 0, 1, 0, 0)]) in deps
    assert (idx[(Q, 0, 0, 0, 0)], idx[(D, 1, 0, 1, 0)]) in deps
    assert (idx[(D, 0, 0, 1, 0)], idx[(Q, 0, 0, 1, 1)]) in deps
    assert (idx[(D, 0, 0, 1, 0)], idx[(D, 0, 1, 1, 0)]) in deps, "the head rows R_01 chain through l"
    assert (idx[(D, 0, 0, 1, 0)], idx[(D, 1, 0, 1, 0)]) not in deps
