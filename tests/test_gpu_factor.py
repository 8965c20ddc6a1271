"""Whole-factorisation parity of the MI355X engine (through the C ABI).

Against the reference's own outputs (tests/golden, from oracle/_ref) and against the oracle
at sizes it finishes in seconds; at BASELINE.json's full sizes through size-independent
properties (column norms preserved by an orthogonal Q, ||R||_F = ||A||_F, |R| against an
independent QR).

Stated tolerances:
  fp64: elementwise max|GPU - oracle| <= 1e-11 * max|A|-scale for R, V and tau;
        residual ||Q^T A - R||_F / ||A||_F <= 1e-13 * max(1, n/4096)
  fp32: elementwise <= 1e-3 absolute (the reference's EPSILON, qrdecomp.c:23); residual <= 5e-5
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu


def assert_close(F, T, F_ref, T_ref):
    if F_ref.dtype == np.float64:
        s = max(1.0, float(np.abs(F_ref).max()))
        assert float(np.abs(F - F_ref).max()) <= 1e-11 * s
        assert float(np.abs(T - T_ref).max()) <= 1e-11 * 2
    else:
        assert float(np.abs(F.astype(np.float64) - F_ref).max()) <= 1e-3
        assert float(np.abs(T.astype(np.float64) - T_ref).max()) <= 1e-3


FACTOR = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "factor_*.npz")))


@pytest.mark.parametrize("name", FACTOR)
def test_factor_vs_reference(tqr, oracle, name):
    g = golden(name)
    A, F_ref, T_ref, b = g["A"], g["F"], g["T"], int(g["b"])
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    assert_close(F, T, F_ref, T_ref)
    res = oracle.residual(A, F, T, b)
    assert res <= (5e-5 if A.dtype == np.float32 else 1e-13)


@pytest.mark.parametrize("m,n,b,dt", [
    (512, 512, 64, np.float64),      # BASELINE configs[0] shape
    (1024, 768, 128, np.float64),
    (768, 1024, 128, np.float64),
    (1024, 1024, 256, np.float64),
    (2048, 512, 256, np.float64),    # tall-skinny: 7 TS rows under the panel, one TSMQR per chain task under the
                                     # default knobs (default_tail); chain tasks of several: test_gpu_segments.py
    (512, 512, 64, np.float32),
    (1024, 1024, 256, np.float32),
    (1024, 768, 128, np.float32),    # fp32 asm chain, 128-tiles
    (4096, 512, 256, np.float32),    # fp32: two chain segments per column (head strip handed on)
])
def test_factor_vs_oracle(tqr, oracle, m, n, b, dt):
    A = oracle.randzo(m, n, dt, seed=5)
    F_ref, T_ref = oracle.factor(A, b, threads=8)
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    assert_close(F, T, F_ref, T_ref)


def test_config_c2_vs_oracle(tqr, oracle):
    """BASELINE configs[1]: 4096 x 4096 fp64, b = 128, full elementwise parity."""
    m = n = 4096
    A = oracle.randzo(m, n, np.float64, seed=5)
    F_ref, T_ref = oracle.factor(A, 128, threads=16)
    F = A.copy()
    T = tqr.geqrt_host(F, 128)
    assert_close(F, T, F_ref, T_ref)


@pytest.mark.parametrize("kind", ["eye", "triu", "zerocol"])
def test_structured_inputs(tqr, oracle, kind):
    m, n, b = 512, 512, 128
    A = oracle.randzo(m, n, np.float64, seed=2)
    if kind == "eye":
        A = np.eye(n, m)
    elif kind == "triu":
        for j in range(n):
            A[j, j + 1:] = 0
    else:
        A[300, :] = 0.0  # matrix column 300 = 0: tau = 2, no scaling (qrdecomp.c:1219,1265)
        A[301, :] = 0.0
    F_ref, T_ref = oracle.factor(A, b)
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    assert_close(F, T, F_ref, T_ref)


def test_zero_row_sign_ambiguous(tqr, oracle):
    """A zero matrix ROW makes a diagonal tile rank-deficient: some pivot x0 is pure rounding
    noise and sign(x0) — hence that reflector's sign — is decided by the noise, in the
    reference as much as here. Elementwise parity is therefore not defined for such inputs;
    the factorisation is checked by its residual and |R| (unique up to row signs) instead."""
    m, n, b = 512, 512, 128
    A = oracle.randzo(m, n, np.float64, seed=2)
    A[:, 77] = 0.0
    F_ref, T_ref = oracle.factor(A, b)
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    assert oracle.residual(A, F, T, b) <= 1e-13
    R, R_ref = np.triu(F.T), np.triu(F_ref.T)
    assert np.abs(np.abs(R) - np.abs(R_ref)).max() <= 1e-11 * np.abs(R_ref).max()


def _device_factor(tqr, m, n, b, dtype, seed=5):
    import torch
    A = torch.empty((n, m), dtype=dtype, device="cuda")
    tqr.fill_randzo(A, m, n, seed)
    A0 = A.clone()
    tau = torch.zeros((min(m, n) // b, m), dtype=dtype, device="cuda")
    plan = tqr.TiledQR(m, n, b, dtype)
    plan.execute(A, tau)
    torch.cuda.synchronize()
    return A0, A, tau


@pytest.mark.parametrize("m,n,b", [(16384, 16384, 256), (65536, 4096, 256), (65536, 16384, 256)])
def test_full_size_properties(tqr, oracle, m, n, b):
    """BASELINE configs[2] and configs[3] (65536 x 16384, here on one GPU), and a tall shape:
    Q orthogonal => every column norm of R equals that of A; every tau lies in [1, 2] (tau =
    2/(1+|v_B|^2) >= 1 for TSQRT reflectors, 2/(v'v) with v0 = 1 for GEQRT); R matches an
    independent QR (torch) up to row signs on the leading 2048 columns."""
    import torch
    A0, F, tau = _device_factor(tqr, m, n, b, torch.float64)
    R = torch.triu(F.T).T  # (n, m) storage: zero below the diagonal
    na = torch.linalg.vector_norm(A0, dim=1)
    nr = torch.linalg.vector_norm(R[:, :m], dim=1)
    rel = ((na - nr).abs() / na).max().item()
    assert rel <= 1e-12 * max(1.0, n / 4096)
    assert torch.all(tau[tau != 0] >= 1.0) and torch.all(tau <= 2.0)
    # leading 2048 columns: |R| vs torch's QR of the same columns (R is unique up to signs)
    c = 2048
    Rt = torch.linalg.qr(A0[:c, :].T.contiguous(), mode="r")[1]
    Rg = R[:c, :c].T
    err = (Rt.abs() - Rg.abs()).abs().max().item() / Rt.abs().max().item()
    assert err <= 1e-11
    # ... and elementwise against the oracle: tile columns 0..c/b-1 of a tiled QR depend only on
    # themselves (panel k and the updates of steps < k), so the full-size output's leading c
    # columns — R, V and tau — are the oracle's factorisation of the m x c slice
    # (reference qrdecomp.c:94-114 compares the whole in-place matrix; SURVEY.md §8d tolerance)
    _leading_columns_vs_oracle(oracle, A0, F, tau, m, b, c, 1e-11)


def _oracle_threads():
    return int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or len(os.sched_getaffinity(0))


def _leading_columns_vs_oracle(oracle, A0, F, tau, m, b, c, tol):
    """Elementwise parity of the leading c columns of a full-size device factorisation with the
    oracle run on that m x c slice: fp64 max|dF| <= tol * max|F|, |dtau| <= tol * 2.
    fp32 (tol None): the reference's EPSILON (qrdecomp.c:23) is 1e-3 absolute at its own sizes,
    where |F| stays below ~10; at 32768 rows |R| reaches ~100 and the fp32 oracle's own rounding
    grows with it, so the bound is 1e-4 relative to max|F| (2e-4 for tau in [1, 2]) — and the GPU's
    fp32 result must be no farther from the fp64 oracle on the same (fp32) input than the fp32
    oracle is (the chains run fp32 MFMA, the panels fp64: DESIGN.md §6)."""
    import time
    As = A0[:c].cpu().numpy()
    t0 = time.perf_counter()
    F_ref, T_ref = oracle.factor(As, b, threads=_oracle_threads())
    print(f"oracle {m}x{c}: {time.perf_counter() - t0:.1f} s")
    Fg = F[:c].cpu().numpy().astype(np.float64)
    Tg = tau[:c // b].cpu().numpy().astype(np.float64)
    dF = float(np.abs(Fg - F_ref).max())
    dT = max(float(np.abs(Tg[k, k * b:] - T_ref[k * b, k * b:]).max()) for k in range(c // b))
    print(f"leading {c} columns vs oracle: max|dF| = {dF:.3e} (max|F| {np.abs(F_ref).max():.3e}), max|dtau| = {dT:.3e}")
    if tol is None:
        assert dF <= 1e-4 * max(1.0, float(np.abs(F_ref).max())) and dT <= 2e-4
        F64, _ = oracle.factor(As.astype(np.float64), b, threads=_oracle_threads())
        e_gpu = float(np.abs(Fg - F64).max())
        e_ref = float(np.abs(F_ref - F64).max())
        print(f"vs the fp64 oracle: GPU fp32 {e_gpu:.3e}, reference-arithmetic fp32 oracle {e_ref:.3e}")
        assert e_gpu <= 1.5 * e_ref
    else:
        assert dF <= tol * max(1.0, float(np.abs(F_ref).max()))
        assert dT <= tol * 2


@pytest.mark.parametrize("m", [4096, 32768])
def test_fp32_device_large(tqr, oracle, m):
    """fp32 storage up to BASELINE configs[4] (32768 x 32768, b = 256) at full size: column norms
    of R equal those of A (fp32 tolerance 5e-5), |R| matches torch's fp64 QR of
    the same (fp32) columns on the leading 1024 columns within the reference's EPSILON-scale
    relative bound, and those 1024 columns (R, V, tau) match the fp32 oracle elementwise."""
    import torch
    n = m
    A0, F, tau = _device_factor(tqr, m, n, 256, torch.float32)
    R = torch.triu(F.T).T
    na = torch.linalg.vector_norm(A0.double(), dim=1)
    nr = torch.linalg.vector_norm(R.double(), dim=1)
    assert ((na - nr).abs() / na).max().item() <= 5e-5
    assert torch.all(tau[tau != 0] >= 1.0 - 1e-6) and torch.all(tau <= 2.0 + 1e-6)
    c = 1024
    Rt = torch.linalg.qr(A0[:c, :].double().T.contiguous(), mode="r")[1]
    Rg = R[:c, :c].T.double()
    assert ((Rt.abs() - Rg.abs()).abs().max() / Rt.abs().max()).item() <= 1e-4
    del R
    _leading_columns_vs_oracle(oracle, A0, F, tau, m, 256, c, None)
    del F, A0


@pytest.mark.timeout(900)
def test_config_c3_elementwise_vs_oracle(tqr, oracle):
    """BASELINE configs[2] (16384 x 16384 fp64, b = 256) elementwise against the oracle (the
    reference host path restated, run with every host thread this process may use): R, V and tau
    at the SURVEY.md §8d tolerance max|dF| <= 1e-11 max|F|, tau <= 1e-11 * 2. The oracle's wall
    time is printed (pytest -s / the log's captured stdout)."""
    import time
    m = n = 16384
    b = 256
    thr = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or len(os.sched_getaffinity(0))
    A = oracle.randzo(m, n, np.float64, seed=5)
    F = A.copy()
    T = tqr.geqrt_host(F, b)
    t0 = time.perf_counter()
    F_ref, T_ref = oracle.factor(A, b, threads=thr)
    print(f"c3 oracle: {time.perf_counter() - t0:.1f} s on {thr} threads")
    del A
    s = max(1.0, float(np.abs(F_ref).max()))
    dF = max(float(np.abs(F[j:j + 1024] - F_ref[j:j + 1024]).max()) for j in range(0, n, 1024))
    dT = max(float(np.abs(T[j * b] - T_ref[j * b]).max()) for j in range(n // b))
    print(f"c3 elementwise: max|dF| = {dF:.3e} (scale {s:.3e}), max|dtau| = {dT:.3e}")
    assert dF <= 1e-11 * s
    assert dT <= 1e-11 * 2


def test_legacy_entry_points(tqr, oracle):
    """cudaQRTask (gpucalc.h) and taskQRP_threads (qrdecomp.h) through the C ABI, checked the
    way the reference checks itself: checkEqual against the CPU result at 1e-3."""
    import ctypes
    L = tqr.lib()
    m = n = 128
    A = oracle.randzo(m, n, np.float32, seed=5)
    F_ref, T_ref = oracle.factor(A, 32)
    G = A.copy()
    L.cudaQRTask(G.ctypes.data_as(ctypes.c_void_p), m, n, m, 128)
    assert L.checkEqual(G.ctypes.data_as(ctypes.c_void_p), F_ref.ctypes.data_as(ctypes.c_void_p), m, n, m) == 1
    R = np.zeros_like(A)
    T = np.zeros_like(A)
    P = ctypes.c_void_p
    L.taskQRP_threads(A.ctypes.data_as(P), R.ctypes.data_as(P), T.ctypes.data_as(P), m, n, 32, m, 1)
    assert np.abs(R - F_ref).max() <= 1e-3 and np.abs(T - T_ref).max() <= 1e-3


def test_task_order_and_lookahead_segments_bitexact(tqr):
    """The persistent engine computes the same bits whatever valid task order it runs: the plan's
    estimated order vs a step-major permutation loaded with tqr_plan_set_tasks, and vs plans whose
    lookahead column or tail steps use other segment lengths (TQR_SEGLEN_LA, TQR_TAIL,
    TQR_TAIL_SEGLEN, read at plan creation)."""
    import ctypes
    import torch
    from test_capi import step_major
    m, n, b = 3072, 2048, 256
    L = tqr.lib()

    def run(plan):
        A = torch.empty((n, m), dtype=torch.float64, device="cuda")
        tqr.fill_randzo(A, m, n, 9)
        tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
        plan.execute(A, tau)
        plan.status()
        return A.cpu(), tau.cpu()

    p0 = tqr.TiledQR(m, n, b, torch.float64)
    A0, t0 = run(p0)
    nt = ctypes.c_int()
    L.tqr_plan_info(p0.h, None, ctypes.byref(nt), None, None)
    buf = (ctypes.c_int * (4 * nt.value))()
    assert L.tqr_flow_plan_export(m // b, n // b, b, 8, buf, nt.value) == nt.value
    items = step_major([tuple(buf[4 * x:4 * x + 4]) for x in range(nt.value)])
    arr = (ctypes.c_int * (4 * len(items)))(*[v for it in items for v in it])
    assert L.tqr_plan_set_tasks(p0.h, arr, len(items)) == 0
    A1, t1 = run(p0)
    assert torch.equal(A0, A1) and torch.equal(t0, t1)
    old = os.environ.get("TQR_SEGLEN_LA")
    os.environ["TQR_SEGLEN_LA"] = "3"
    try:
        p2 = tqr.TiledQR(m, n, b, torch.float64)
    finally:
        if old is None:
            os.environ.pop("TQR_SEGLEN_LA")
        else:
            os.environ["TQR_SEGLEN_LA"] = old
    A2, t2 = run(p2)
    assert torch.equal(A0, A2) and torch.equal(t0, t2)
    # the fp64 list's one-element tail segments (flowplan.cpp default_tail; every step of this size)
    # against none (TQR_TAIL=0) and two-element ones
    for env in ({"TQR_TAIL": "0"}, {"TQR_TAIL_SEGLEN": "2"}):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            p3 = tqr.TiledQR(m, n, b, torch.float64)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k)
                else:
                    os.environ[k] = v
        A3, t3 = run(p3)
        assert torch.equal(A0, A3) and torch.equal(t0, t3), env


@pytest.mark.parametrize("env", [{"TQR_CHAIN_ASM": "1"}, {"TQR_CHAIN_ASM": "0"}, {"TQR_FLOW_SHAPE": "r"}])
@pytest.mark.parametrize("m,n", [(1024, 1024), (2048, 512), (1536, 1280)])
def test_fp64_chain_forms_vs_oracle(tqr, oracle, monkeypatch, env, m, n):
    """The fp64 chain forms other than the default (late strip loads in the 8-wave asm chain):
    the whole strip loaded inside the hand-over (TQR_CHAIN_ASM=1), the compiler-scheduled chain
    (TQR_CHAIN_ASM=0) and the resident one-wave-per-SIMD form (TQR_FLOW_SHAPE=r, chain_res.hpp)
    against the oracle at b = 256 (the knobs are read at plan creation: plans cached before are
    dropped first)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tqr.cache_clear()
    try:
        A = oracle.randzo(m, n, np.float64, seed=7)
        F_ref, T_ref = oracle.factor(A, 256, threads=8)
        F = A.copy()
        T = tqr.geqrt_host(F, 256)
        assert_close(F, T, F_ref, T_ref)
    finally:
        tqr.cache_clear()


@pytest.mark.parametrize("env", [{"TQR_CHAIN_ASM": "1"}, {"TQR_CHAIN32_ASM": "0"}, {"TQR_UNMQR_ALONE": "0"},
                                 {"TQR_TAIL": "64", "TQR_UNMQR_ALONE": "64"}])
@pytest.mark.parametrize("m,n,b,dt", [(4096, 768, 256, np.float32), (1024, 1024, 128, np.float32),
                                      (1536, 1280, 256, np.float64)])
def test_chain_knobs_vs_oracle(tqr, oracle, monkeypatch, env, m, n, b, dt):
    """Non-default chain knobs on both precisions: the fp32 asm chain with the whole next strip
    loaded in the hand-over (TQR_CHAIN_ASM=1) and the compiler-scheduled fp32 chain
    (TQR_CHAIN32_ASM=0); the tail's lookahead UNMQR-alone segments off (TQR_UNMQR_ALONE=0) and on
    for every step with one-element segments (also for fp32, whose default tail is 0)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tqr.cache_clear()
    try:
        A = oracle.randzo(m, n, dt, seed=11)
        F_ref, T_ref = oracle.factor(A, b, threads=8)
        F = A.copy()
        T = tqr.geqrt_host(F, b)
        assert_close(F, T, F_ref, T_ref)
    finally:
        tqr.cache_clear()
