"""The task-list planner (csrc/flowplan.cpp) against lists recorded before it was moved out of
engine.hip.

tests/golden/flow_lists.json holds, per case of the grid below, the task count, est_order and the
FNV-1a hash (flow_list_hash, the plan signature's formula) of the list the planner built when the
file was recorded. Two independent runs must reproduce it: tqr_flow_list_export of the built
library, and a stand-alone driver (tests/drivers/flowplan_driver.cpp) compiled with flowplan.cpp
under the host address and undefined-behaviour sanitizers.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "gpu-tiled-qr-decomposition_amd")
sys.path.insert(0, PKG)
import tqr  # noqa: E402

FIELDS = ("M", "N", "b", "dtype", "seglen", "world", "rank", "full", "nxc", "tcol")
GRIDS = [(1, 1), (1, 5), (3, 6), (6, 3), (5, 7), (8, 8), (16, 4), (16, 6), (32, 16), (64, 64)]
TILES = [16, 32, 64, 256]
SEGLENS = [0, 1, 2, 8]
WORLDS = [1, 2, 3, 4, 8]
ENVS = [{"TQR_SEGLEN_LA": "2"}, {"TQR_LA_TAIL": "4"}, {"TQR_TAIL": "3", "TQR_TAIL_SEGLEN": "2"}, {"TQR_UNMQR_ALONE": "0"},
        {"TQR_LAZY": "0"}, {"TQR_LA": "2"}, {"TQR_LAC": "4"}, {"TQR_TG": "2.0"}, {"TQR_DIST_DEFAULTS": "r4"},
        {"TQR_DIST_PART": "cyclic"}, {"TQR_FLOW_SHAPE": "w4"}, {"TQR_FLOW_SHAPE": "r"}]
# every variable that shapes a list: none may leak into a case from the caller's environment
KNOBS = sorted({k for e in ENVS for k in e} | {"TQR_SEGLEN"})


def _case(M, N, b, dtype, seglen=0, world=1, rank=-1, full=1, nxc=0, tcol=0.0, env=None):
    return dict(zip(FIELDS, (M, N, b, dtype, seglen, world, rank, full, nxc, tcol)), env=dict(env or {}))


def grid():
    """The case grid: a thinned product in which every tile grid, tile size, dtype, segment length,
    world (each with a square and a tall grid, every rank, full 0 and 1), transfer setting and
    environment override appears (test_grid_covers checks that)."""
    cases = []
    x = 0
    for (M, N) in GRIDS:  # one-GPU lists: every grid x tile size x dtype, the segment lengths in turn
        for b in ([64, 256] if M * N >= 4096 else TILES):
            for dtype in (tqr.TQR_F64, tqr.TQR_F32):
                cases.append(_case(M, N, b, dtype, SEGLENS[x % 4]))
                x += 1
    for world in WORLDS:  # multi-GPU: the global list and every rank's, square and tall grids
        for (M, N), b in (((8, 8), 64), ((16, 4), 256), ((5, 7), 32), ((16, 6), 128)):
            for full in (0, 1):
                dtype = tqr.TQR_F64 if (M + full) % 2 == 0 else tqr.TQR_F32
                seglen = SEGLENS[(x + full) % 4] if (M, N) == (5, 7) else 0
                for rank in range(-1, world):
                    if world > 1 or rank < 0:
                        cases.append(_case(M, N, b, dtype, seglen, world, rank, full))
        x += 1
    for rank in range(-1, 8):  # the 8-GPU run's shape in tiles / 2
        cases.append(_case(32, 16, 256, tqr.TQR_F64, 0, 8, rank, 1))
    cases.append(_case(64, 64, 256, tqr.TQR_F64, 0, 4, -1, 1))
    for (M, N), b in (((1, 1), 16), ((3, 6), 64), ((6, 3), 32), ((8, 8), 256), ((16, 6), 256)):  # host-pointer lists
        for nxc in (1, 3):
            for tcol in (0.0, 2.5):
                dtype = tqr.TQR_F64 if (nxc + int(tcol)) % 2 else tqr.TQR_F32
                cases.append(_case(M, N, b, dtype, 8 if nxc == 3 else 0, nxc=nxc, tcol=tcol))
    for env in ENVS:  # the environment's knobs, one setting at a time
        cases.append(_case(8, 8, 256, tqr.TQR_F64, env=env))
        cases.append(_case(16, 6, 64, tqr.TQR_F32, env=env))
        cases.append(_case(5, 7, 256, tqr.TQR_F64, nxc=3, tcol=2.5, env=env))
        cases.append(_case(16, 4, 256, tqr.TQR_F64, 0, 4, -1, 1, env=env))
        cases.append(_case(16, 4, 256, tqr.TQR_F64, 0, 4, 2, 1, env=env))
        cases.append(_case(8, 8, 64, tqr.TQR_F64, 0, 8, 7, 1, env=env))
    return cases


def case_id(c):
    return " ".join(str(c[f]) for f in FIELDS) + "".join(f" {k}={v}" for k, v in sorted(c["env"].items()))


CASES = grid()
with open(os.path.join(HERE, "golden", "flow_lists.json")) as f:
    GOLDEN = json.load(f)


def fnv1a(items):
    """flow_list_hash: FNV-1a over the items' ints in order, little-endian bytes."""
    h = 2166136261
    for byte in np.ascontiguousarray(items, dtype="<i4").tobytes():
        h = ((h ^ byte) * 16777619) & 0xffffffff
    return h


@pytest.fixture
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def export(c, mp):
    with mp.context() as m:
        for k, v in c["env"].items():
            m.setenv(k, v)
        return tqr.flow_list(**{f: c[f] for f in FIELDS})


def test_grid_covers():
    assert len(set(map(case_id, CASES))) == len(CASES) and 200 <= len(CASES) <= 500
    assert sorted(GOLDEN) == sorted(map(case_id, CASES))  # the recorded file is of this very grid
    assert {(c["M"], c["N"]) for c in CASES} == set(GRIDS)
    assert {c["b"] for c in CASES} >= set(TILES)
    assert {c["dtype"] for c in CASES} == {tqr.TQR_F32, tqr.TQR_F64}
    assert {c["seglen"] for c in CASES} == set(SEGLENS)
    assert {(c["nxc"], c["tcol"]) for c in CASES} >= {(1, 0.0), (1, 2.5), (3, 0.0), (3, 2.5)}
    for e in ENVS:
        assert any(c["env"] == e for c in CASES)
    for world in WORLDS:
        mine = [c for c in CASES if c["world"] == world]
        assert any(c["M"] == c["N"] for c in mine) and any(c["M"] > c["N"] for c in mine)
        for full in (0, 1):
            assert {c["rank"] for c in mine if c["full"] == full} >= set(range(-1, world if world > 1 else 0))


def test_lists_match_recorded(clean_env):
    """tqr_flow_list_export of the built library, case by case: count and hash as recorded, and
    every list topological for the engine's waits."""
    L = tqr.lib()
    for c in CASES:
        cid = case_id(c)
        with clean_env.context() as m:
            for k, v in c["env"].items():
                m.setenv(k, v)
            items = tqr.flow_list(**{f: c[f] for f in FIELDS})
            n, est, h = GOLDEN[cid]
            assert (len(items), fnv1a(items)) == (n, h), cid
            # (whole lists only: a rank's partition waits on tasks of other ranks; the checker counts
            # the strips per tile of the fp64 shape, which TQR_FLOW_SHAPE changes for fp64 lists alone)
            if c["rank"] < 0 and not (c["dtype"] == tqr.TQR_F32 and "TQR_FLOW_SHAPE" in c["env"]):
                arr = items.ctypes.data_as(ctypes.c_void_p)
                assert L.tqr_flow_order_check(c["M"], c["N"], c["b"], arr, n) == 1, cid
            # est_order of the lists the older entry points can describe
            if c["dtype"] == tqr.TQR_F64 and c["world"] == 1 and c["seglen"] >= 1:
                nt, eo = ctypes.c_int(), ctypes.c_int()
                if c["nxc"]:
                    L.tqr_flow_xfer_plan_check.argtypes = [ctypes.c_int] * 5 + [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
                    st = L.tqr_flow_xfer_plan_check(c["M"], c["N"], c["b"], c["seglen"], c["nxc"], c["tcol"],
                                                    ctypes.byref(nt), ctypes.byref(eo))
                else:
                    st = L.tqr_flow_plan_check(c["M"], c["N"], c["b"], c["seglen"], ctypes.byref(nt), ctypes.byref(eo))
                assert (st, nt.value, eo.value) == (0, n, est), cid


def test_rank_lists_partition_global(clean_env):
    """The ranks' lists of a world are the global list split by owner: every task on exactly one
    rank, and each rank's tasks in the global order."""
    worlds = {}
    for c in CASES:
        if c["world"] > 1:
            key = case_id(dict(c, rank=-1))
            worlds.setdefault(key, {})[c["rank"]] = c
    assert worlds
    checked = 0
    for key, ranks in worlds.items():
        world = next(iter(ranks.values()))["world"]
        if set(ranks) != set(range(-1, world)):
            continue  # (an environment case that holds one rank only)
        glob = [tuple(t) for t in export(ranks[-1], clean_env)]
        pos = {t: x for x, t in enumerate(glob)}
        assert len(pos) == len(glob)
        seen = []
        for r in range(world):
            mine = [tuple(t) for t in export(ranks[r], clean_env)]
            where = [pos[t] for t in mine]
            assert where == sorted(where), (key, r)
            seen += mine
        assert sorted(seen) == sorted(glob), key
        checked += 1
    assert checked >= 2 * 2 * 4  # grids x full x worlds > 1


def test_sanitized_driver(tmp_path):
    """The planner alone (g++, no HIP) under ASan + UBSan walks the grid: exit status 0, no
    sanitizer report, the recorded values, and no missed dependency lookup."""
    exe = str(tmp_path / "flowplan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "drivers", "flowplan_driver.cpp"), os.path.join(PKG, "csrc", "flowplan.cpp"),
                           "-o", exe])
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(case_id(c) + "\n" for c in CASES))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe, str(cases)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert lines[len(CASES)] == "missed 0"
    for c, line in zip(CASES, lines):
        assert [int(v) for v in line.split()] == GOLDEN[case_id(c)], case_id(c)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,b,dt", [(512, 512, 64, "float64"), (512, 256, 128, "float32")])
def test_plan_list_is_the_export(m, n, b, dt):
    """A plan's device list is the host-only export of its spec (tqr_plan_set_tasks accepts only a
    topological permutation of the plan's own tasks), and loading it changes no bit."""
    import torch
    dtype = getattr(torch, dt)
    plan = tqr.TiledQR(m, n, b, dtype)

    def run():
        A = torch.empty((n, m), dtype=dtype, device="cuda")
        tqr.fill_randzo(A, m, n, 11)
        tau = torch.zeros((n // b, m), dtype=dtype, device="cuda")
        plan.execute(A, tau)
        plan.status()
        return A.cpu(), tau.cpu()

    A0, t0 = run()
    items = tqr.flow_list(m // b, n // b, b, tqr.TQR_F64 if dt == "float64" else tqr.TQR_F32)
    assert tqr.lib().tqr_plan_set_tasks(plan.h, items.ctypes.data_as(ctypes.c_void_p), len(items)) == 0
    A1, t1 = run()
    assert torch.equal(A0, A1) and torch.equal(t0, t1)
