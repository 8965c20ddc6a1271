"""The planner's deep-lookahead order (csrc/flowplan.cpp window_order; FlowKnobs::depth, TQR_DEPTH).

Only the order of a plan's task list changes: the list must stay a topological permutation of the
list with the knob at 0, differ from it where the default is on (one rank, fp64 storage, b = 256,
8-element segments, no cap, no transfers, 44 to 80 steps of a grid that is not taller than wide)
and equal it everywhere else. Checked through tqr_flow_list_export of the built library and, case by
case, by a stand-alone driver (tests/drivers/flow_window_driver.cpp) compiled with flowplan.cpp under
the host address and undefined-behaviour sanitizers. On the GPU a forced depth changes no bit of A
and tau.
"""
import ctypes
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

FIELDS = ("M", "N", "b", "dtype", "seglen", "world", "rank", "full", "nxc", "tcol", "steps")
# every variable that shapes a list: none may leak into a case from the caller's environment
KNOBS = ["TQR_DEPTH", "TQR_SEGLEN", "TQR_SEGLEN_LA", "TQR_LA_TAIL", "TQR_TAIL", "TQR_TAIL_SEGLEN", "TQR_UNMQR_ALONE", "TQR_LAZY",
         "TQR_LA", "TQR_LAC", "TQR_TG", "TQR_DIST_DEFAULTS", "TQR_DIST_PART", "TQR_FLOW_SHAPE"]
F64, F32 = tqr.TQR_F64, tqr.TQR_F32


def _case(M, N, b=256, dtype=F64, seglen=0, world=1, rank=-1, full=1, nxc=0, tcol=0.0, steps=0, depth=None):
    return dict(zip(FIELDS, (M, N, b, dtype, seglen, world, rank, full, nxc, tcol, steps)), depth=depth)


# the default is on: a new list
ON = [_case(48, 48), _case(64, 64), _case(64, 96), _case(44, 44), _case(80, 80)]
# the default is off: the list of the knob at 0
OFF = [_case(64, 64, b=64), _case(64, 64, seglen=2), _case(64, 64, dtype=F32), _case(64, 64, world=2), _case(64, 64, steps=48),
       _case(48, 48, nxc=2, tcol=2.5), _case(64, 64, full=0),
       # taller than wide (measured slower with the window: no latency-bound tail), and outside 44..80 steps
       _case(96, 64), _case(40, 40), _case(84, 84)]
# forced on small grids, where both priority classes exist
FORCED = [_case(8, 8, depth=2), _case(8, 8, depth=3), _case(16, 4, depth=2), _case(5, 7, depth=2), _case(5, 7, depth=3),
          _case(8, 8, b=64, depth=2), _case(8, 8, dtype=F32, depth=3), _case(16, 8, steps=4, depth=2), _case(1, 1, depth=2)]
CASES = ON + OFF + FORCED


def case_id(c):
    return " ".join(str(c[f]) for f in FIELDS) + (f" TQR_DEPTH={c['depth']}" if c["depth"] is not None else "")


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


def export(c, mp, depth="case"):
    """The case's list; depth: "case" (its own TQR_DEPTH, if any) or a value to force."""
    d = c["depth"] if depth == "case" else depth
    with mp.context() as m:
        if d is not None:
            m.setenv("TQR_DEPTH", str(d))
        return tqr.flow_list(**{f: c[f] for f in FIELDS})


def topological(c, items):
    return tqr.lib().tqr_flow_order_check(c["M"], c["N"], c["b"], items.ctypes.data_as(ctypes.c_void_p), len(items)) == 1


def is_permutation(a, b):
    return sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))


@pytest.mark.parametrize("c", ON, ids=case_id)
def test_default_on_is_a_new_topological_permutation(c, clean_env):
    new, old = export(c, clean_env), export(c, clean_env, 0)
    assert topological(c, new) and topological(c, old)
    assert is_permutation(new, old)
    assert fnv1a(new) != fnv1a(old)


@pytest.mark.parametrize("c", OFF, ids=case_id)
def test_default_off_keeps_the_list(c, clean_env):
    new, old = export(c, clean_env), export(c, clean_env, 0)
    assert new.shape == old.shape and (new == old).all()


@pytest.mark.parametrize("c", FORCED, ids=case_id)
def test_forced_depth_is_a_topological_permutation(c, clean_env):
    new, old = export(c, clean_env), export(c, clean_env, 0)
    assert topological(c, new)
    assert is_permutation(new, old)
    if min(c["M"], c["N"]) >= 5:  # (both classes exist: the window moves tasks)
        assert fnv1a(new) != fnv1a(old)


def test_forced_depth_leaves_multi_rank_and_transfer_lists(clean_env):
    """TQR_DEPTH reorders one-rank device lists only: the ranks' lists and the host-pointer list keep
    their order."""
    for c in (_case(16, 4, world=4, depth=3), _case(16, 4, world=2, rank=1, depth=2), _case(8, 8, nxc=3, tcol=2.5, depth=2)):
        assert (export(c, clean_env) == export(c, clean_env, 0)).all(), case_id(c)


@pytest.mark.parametrize("M,N,D", [(16, 16, 4), (12, 20, 3), (36, 36, 9)])
def test_planner_list_is_the_models_greedy(M, N, D, clean_env):
    """The planner's pass against the model it was ported from (tools/sched_sim.py greedy_order with
    the window priority and the round-6 costs, on the depth-0 list's own tasks and segments; 36 steps
    have the one-element tail and the lone UNMQR segments): the same list item for item, so it
    simulates no worse."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import sched_sim as S
    base = export(_case(M, N), clean_env, 0)
    cpp = export(_case(M, N), clean_env, D)
    py = S.to_items(S.greedy_order(M, N, prm=S.P6, prio="window", depth=D, items=base))
    assert S.simulate(cpp, M, N, prm=S.P6)[0] <= S.simulate(py, M, N, prm=S.P6)[0]
    assert (py == cpp).all()


def test_sanitized_driver(tmp_path):
    """The planner alone (g++, no HIP) under ASan + UBSan walks the same cases: exit status 0, no
    sanitizer report, and per case what the library's export gives."""
    exe = str(tmp_path / "flow_window_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "drivers", "flow_window_driver.cpp"), os.path.join(PKG, "csrc", "flowplan.cpp"),
                           "-o", exe])
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(case_id(c) + "\n" for c in CASES))
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([exe, str(cases)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")
    assert len(lines) == len(CASES) + 1
    for c, line in zip(CASES, lines):
        n, topo, perm, h, h0 = (int(v) for v in line.split())
        assert topo == 1 and perm == 1, case_id(c)
        if c in ON:
            assert h != h0, case_id(c)
        if c in OFF:
            assert h == h0, case_id(c)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,b", [(2048, 2048, 256), (4096, 1024, 256), (512, 512, 64)])
def test_forced_depth_changes_no_bit(m, n, b, clean_env):
    """Plans with the depth forced to 2 and 3 against the knob-0 plan: A and tau bit-identical, the
    engine's status clean, and each plan's device list is the host export of its spec."""
    import torch

    def run(depth):
        with clean_env.context() as mp:
            mp.setenv("TQR_DEPTH", str(depth))
            plan = tqr.TiledQR(m, n, b, torch.float64)
            want = tqr.flow_list(m // b, n // b, b)
        A = torch.empty((n, m), dtype=torch.float64, device="cuda")
        tqr.fill_randzo(A, m, n, 11)
        tau = torch.zeros((min(m, n) // b, m), dtype=torch.float64, device="cuda")
        plan.execute(A, tau)
        plan.status()
        return A.cpu(), tau.cpu(), tqr.plan_tasks(plan), want

    A0, t0, dev0, exp0 = run(0)
    assert (dev0 == exp0).all()
    for depth in (2, 3):
        A1, t1, dev, exp = run(depth)
        assert dev.shape == exp.shape and (dev == exp).all()
        assert not (dev == dev0).all()  # (the shapes have both priority classes: the order moved)
        assert torch.equal(A0, A1) and torch.equal(t0, t1)
