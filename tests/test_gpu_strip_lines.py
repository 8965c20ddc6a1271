"""Whole-line strips of the fp64 engine on the GPU (TQR_STRIP_LINES, read at plan
creation).

Between two steps the chain strips of a tile whose next reader is a TSMQR element lie in HBM in a
permuted order (flow_list.hpp strip_permuted / strip_lane_off); the arithmetic is untouched. So a plan
with the layout on computes exactly the bits of the same plan with it off (no tolerance applies), and
nothing the caller sees is permuted. Shapes: the smallest that reach each case, fp64, b = 256 —
768 x 768 holds one permuted tile ((2, 2) after step 0); 1280 x 1280 permuted tiles that are re-read
and re-written permuted over several steps; tall and wide; 1280 x 1280 capped at 2 and at 3 steps (the
last step stores standard); 1024 x 1024 under a step-major task order. The oracle comparison uses the
bounds of tests/test_gpu_factor.py (steps_ref.assert_close holds the same ones).
"""
import ctypes
import os

import numpy as np
import pytest

from steps_ref import assert_close, expand_tau_steps, partial

pytestmark = pytest.mark.gpu

B = 256
# (m, n, steps or None, step-major order)
CASES = [(768, 768, None, False), (1280, 1280, None, False), (1024, 768, None, False), (768, 1024, None, False),
         (1280, 1280, 2, False), (1280, 1280, 3, False), (1024, 1024, None, True)]
IDS = [f"{m}x{n}" + (f"s{s}" if s else "") + ("-stepmajor" if o else "") for m, n, s, o in CASES]
_inputs = {}


def host_input(oracle, m, n):
    if (m, n) not in _inputs:
        A = oracle.randzo(m, n, np.float64, seed=5)
        A.setflags(write=False)
        _inputs[(m, n)] = A
    return _inputs[(m, n)]


class lines_env:
    """TQR_STRIP_LINES for the plans created inside the block."""

    def __init__(self, on):
        self.v = "1" if on else "0"

    def __enter__(self):
        self.old = os.environ.get("TQR_STRIP_LINES")
        os.environ["TQR_STRIP_LINES"] = self.v

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("TQR_STRIP_LINES")
        else:
            os.environ["TQR_STRIP_LINES"] = self.old


def run(tqr, A, steps, step_major_order, on):
    import torch
    from test_capi import step_major
    n, m = A.shape
    with lines_env(on):
        plan = tqr.TiledQR(m, n, B, torch.float64, steps=steps)
    if step_major_order:
        L = tqr.lib()
        items = tqr.flow_list(m // B, n // B, B, tqr.TQR_F64)
        order = step_major([tuple(int(v) for v in it) for it in items])
        assert order != [tuple(int(v) for v in it) for it in items]
        arr = (ctypes.c_int * (4 * len(order)))(*[v for it in order for v in it])
        assert L.tqr_plan_set_tasks(plan.h, arr, len(order)) == 0
    dA = torch.from_numpy(A.copy()).cuda()
    tau = torch.full((plan.kmax, m), 7.0, dtype=torch.float64, device="cuda")
    plan.execute(dA, tau)
    plan.status()
    return dA.cpu(), tau.cpu()


@pytest.mark.parametrize("m,n,steps,order", CASES, ids=IDS)
def test_bits_equal_standard_layout(tqr, oracle, m, n, steps, order):
    import torch
    A = host_input(oracle, m, n)
    F0, t0 = run(tqr, A, steps, order, on=False)
    F1, t1 = run(tqr, A, steps, order, on=True)
    d = (F0 != F1).numpy()
    tiles = sorted({(int(i) // B, int(j) // B) for j, i in zip(*np.nonzero(d))})[:20]
    assert torch.equal(F1, F0), f"differing tiles (row, column): {tiles}"
    assert torch.equal(t1, t0)
    if steps:
        F_ref, T_ref = partial(oracle, A, B, steps)
    else:
        F_ref, T_ref = oracle.factor(A, B, threads=8)
    assert_close(F1.numpy(), expand_tau_steps(t1.numpy(), m, n, B), F_ref, T_ref)


def test_padded_leading_dimension(tqr, oracle):
    """ldda = m + 8: columns that are not whole lines apart lose the speed only."""
    import torch
    m = n = 768
    A = host_input(oracle, m, n)
    out = []
    for on in (False, True):
        with lines_env(on):
            plan = tqr.TiledQR(m, n, B, torch.float64)
        dA = torch.full((n, m + 8), -3.0, dtype=torch.float64, device="cuda")
        dA[:, :m] = torch.from_numpy(A.copy()).cuda()
        tau = torch.zeros((plan.kmax, m), dtype=torch.float64, device="cuda")
        plan.execute(dA, tau, ldda=m + 8)
        plan.status()
        out.append((dA.cpu(), tau.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.all(out[1][0][:, m:] == -3.0)


def test_host_pointer_path(tqr, oracle):
    """The host-pointer API's downloads read finished tiles only, which are standard."""
    m = n = 1280
    A = host_input(oracle, m, n)
    out = []
    for on in (False, True):
        tqr.cache_clear()
        with lines_env(on):
            F = A.copy()
            T = tqr.geqrt_host(F, B)
        out.append((F, T))
    tqr.cache_clear()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    F_ref, T_ref = oracle.factor(A, B, threads=8)
    assert_close(out[1][0], out[1][1], F_ref, T_ref)
