"""Capped plans on the GPU (tqr_plan_create_steps, tqr_lstsq_fused, tqr.lstsq_fused, tqr.form_qt;
include/tqr.h).

A capped plan runs the tile tasks of the first `steps` steps of the ordinary plan, on the same operands
in the same per-tile order, and include/tqr.h promises bit-identical results per tile operation
whatever the task order. So (a) what the capped run finishes is bit-identical to the ordinary run,
(b) an ordinary plan on the trailing block completes it bit for bit — both are properties the
reference arithmetic has by itself (tests/test_steps_cpu.py::test_oracle_partial_is_a_prefix_and_resumes)
— and (c) the whole capped result is the oracle's partial(A, s) under the whole factorisation's
bounds. The least-squares and Q^T forms are checked against numpy and the apply, under the bounds of
tests/test_gpu_solve.py and tests/test_gpu_apply.py (copied into tests/steps_ref.py).

Every execute is followed by status(): the engine bounds its waits and reports a timeout there.
"""
import ctypes

import numpy as np
import pytest

from steps_ref import assert_close, check_apply, expand_tau_steps, oracle_qt_cols, partial, tol

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
# (m, n, b, steps): smallest (one group per tile); wide, two groups per tile, s = 3 < p: the last step
# has TS rows and trailing columns at once; tall; chains of more than one default segment (11 rows > 8);
# the generated b = 256 chain bodies; b = 256 with two segments per chain (head hand-over)
SHAPES = [(64, 96, 32, (1,)), (256, 384, 64, (1, 2, 3)), (384, 256, 64, (1, 3)), (384, 160, 32, (2,)),
          (1024, 768, 256, (2,)), (2560, 512, 256, (1,))]
CASES = [(m, n, b, s, dt) for m, n, b, ss in SHAPES for s in ss for dt in (np.float64, np.float32)]


def dn(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


IDS = [f"{m}x{n}b{b}s{s}-{dn(dt)}" for m, n, b, s, dt in CASES]
_cache = {}


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def host_input(oracle, m, n, dt):
    key = ("A", m, n, dn(dt))
    if key not in _cache:
        A = oracle.randzo(m, n, dt, seed=5)
        A.setflags(write=False)
        _cache[key] = A
    return _cache[key]


def ordinary(tqr, oracle, m, n, b, dt):
    """(F, tau) of the ordinary plan on the shape's input, as CPU tensors (computed once)."""
    import torch
    key = ("full", m, n, b, dn(dt))
    if key not in _cache:
        dA = torch.from_numpy(host_input(oracle, m, n, dt).copy()).cuda()
        tau = torch.zeros((min(m, n) // b, m), dtype=dA.dtype, device="cuda")
        plan = tqr.TiledQR(m, n, b, dA.dtype)
        plan.execute(dA, tau)
        plan.status()
        _cache[key] = (dA.cpu(), tau.cpu())
    return _cache[key]


def capped(tqr, oracle, m, n, b, s, dt):
    """(F, tau) of the capped plan on the same input, and (F, tau) after an ordinary plan of
    (m - s*b) x (n - s*b) resumed in place on the trailing block; CPU tensors, computed once."""
    import torch
    key = ("cap", m, n, b, s, dn(dt))
    if key not in _cache:
        dA = torch.from_numpy(host_input(oracle, m, n, dt).copy()).cuda()
        tau = torch.zeros((s, m), dtype=dA.dtype, device="cuda")
        plan = tqr.TiledQR(m, n, b, dA.dtype, steps=s)
        assert plan.kmax == s and tqr.lib().tqr_plan_steps(plan.h) == s
        plan.execute(dA, tau)
        plan.status()
        F, t = dA.cpu(), tau.cpu()
        m2, n2 = m - s * b, n - s * b
        rest = tqr.TiledQR(m2, n2, b, dA.dtype)
        tau2 = torch.zeros((rest.kmax, m2), dtype=dA.dtype, device="cuda")
        block = dA.view(-1)[s * b * m + s * b:]  # tile (s, s): base pointer offset, same ldda
        rest.execute(block, tau2, ldda=m)
        rest.status()
        tall = torch.zeros((min(m, n) // b, m), dtype=dA.dtype)
        tall[:s] = t
        tall[s:, s * b:] = tau2.cpu()
        _cache[key] = (F, t, dA.cpu(), tall)
    return _cache[key]


def differing_tiles(X, Y, b):
    d = (X != Y).numpy()
    return sorted({(int(i) // b, int(j) // b) for j, i in zip(*np.nonzero(d))})[:20]


@pytest.mark.parametrize("m,n,b,s,dt", CASES, ids=IDS)
def test_prefix_identity(tqr, oracle, m, n, b, s, dt):
    """(a) columns < s*b, rows < s*b of every column, and tau columns < s: bit-identical to the
    ordinary plan's."""
    import torch
    F0, t0 = ordinary(tqr, oracle, m, n, b, dt)
    F, t, _, _ = capped(tqr, oracle, m, n, b, s, dt)
    assert t.shape == (s, m)
    assert torch.equal(F[:s * b], F0[:s * b]), differing_tiles(F[:s * b], F0[:s * b], b)
    assert torch.equal(F[:, :s * b], F0[:, :s * b]), differing_tiles(F[:, :s * b], F0[:, :s * b], b)
    assert torch.equal(t, t0[:s])


@pytest.mark.parametrize("m,n,b,s,dt", CASES, ids=IDS)
def test_resumption(tqr, oracle, m, n, b, s, dt):
    """(b) an ordinary plan executed in place on the trailing block: the whole matrix and the
    re-assembled tau equal the ordinary plan's, bit for bit."""
    import torch
    F0, t0 = ordinary(tqr, oracle, m, n, b, dt)
    _, _, F2, t2 = capped(tqr, oracle, m, n, b, s, dt)
    assert torch.equal(F2, F0), f"differing tiles (row, column): {differing_tiles(F2, F0, b)}"
    assert torch.equal(t2, t0)


@pytest.mark.parametrize("m,n,b,s,dt", CASES, ids=IDS)
def test_vs_oracle_partial(tqr, oracle, m, n, b, s, dt):
    """(c) the capped result against partial(A, s), the whole factorisation's bounds."""
    F, t, _, _ = capped(tqr, oracle, m, n, b, s, dt)
    F_ref, T_ref = partial(oracle, host_input(oracle, m, n, dt), b, s)
    assert_close(F.numpy(), expand_tau_steps(t.numpy(), m, n, b), F_ref, T_ref)


def test_steps_equal_min_is_the_ordinary_plan(tqr, oracle):
    """steps = min(p, q): the ordinary plan's list (item for item) and result (bit for bit)."""
    import torch
    m, n, b = 64, 96, 32
    F0, t0 = ordinary(tqr, oracle, m, n, b, np.float64)
    dA = torch.from_numpy(host_input(oracle, m, n, np.float64).copy()).cuda()
    tau = torch.zeros((2, m), dtype=torch.float64, device="cuda")
    plan = tqr.TiledQR(m, n, b, torch.float64, steps=2)
    nt = ctypes.c_int()
    assert tqr.lib().tqr_plan_info(plan.h, None, ctypes.byref(nt), None, None) == 0
    assert nt.value == len(tqr.flow_list(2, 3, b, tqr.TQR_F64))
    plan.execute(dA, tau)
    plan.status()
    assert torch.equal(dA.cpu(), F0) and torch.equal(tau.cpu(), t0)
    assert tqr.lib().tqr_plan_steps(tqr.TiledQR(m, n, b, torch.float64).h) == 2


def test_other_entry_points_on_a_capped_plan(tqr, oracle):
    """tqr_plan_info, tqr_plan_set_tasks and tqr_plan_debug_workspace work against the capped plan's
    own list; whatever TQR_ENGINE says the plan is a flow plan."""
    import torch
    m, n, b, s = 256, 384, 64, 2
    F, t, _, _ = capped(tqr, oracle, m, n, b, s, np.float64)
    L = tqr.lib()
    plan = tqr.TiledQR(m, n, b, torch.float64, steps=s)
    items = tqr.flow_list(m // b, n // b, b, tqr.TQR_F64, steps=s)
    eng, nt = ctypes.c_int(), ctypes.c_int()
    assert L.tqr_plan_info(plan.h, ctypes.byref(eng), ctypes.byref(nt), None, None) == 0
    assert (eng.value, nt.value) == (1, len(items))
    assert L.tqr_plan_set_tasks(plan.h, items.ctypes.data_as(P), len(items)) == 0
    full = tqr.flow_list(m // b, n // b, b, tqr.TQR_F64)
    assert L.tqr_plan_set_tasks(plan.h, full.ctypes.data_as(P), len(full)) == -1  # not this plan's tasks
    dA = torch.from_numpy(host_input(oracle, m, n, np.float64).copy()).cuda()
    tau = torch.zeros((s, m), dtype=torch.float64, device="cuda")
    plan.execute(dA, tau)
    plan.status()
    assert torch.equal(dA.cpu(), F) and torch.equal(tau.cpu(), t)
    L.tqr_plan_debug_workspace.argtypes = [P, ctypes.c_int, P, ctypes.c_size_t]
    buf = np.zeros(16)
    assert L.tqr_plan_debug_workspace(plan.h, s - 1, buf.ctypes.data_as(P), buf.nbytes) > 0
    assert L.tqr_plan_debug_workspace(plan.h, s, buf.ctypes.data_as(P), buf.nbytes) == -1


def test_padded_ldda_stream_and_reuse(tqr, oracle):
    """(f) one capped plan, ldda = m + 8, a non-default stream, executed twice: both results are the
    packed default-stream one bit for bit, and the padding rows are untouched."""
    import torch
    m, n, b, s = 256, 384, 64, 2
    F, t, _, _ = capped(tqr, oracle, m, n, b, s, np.float64)
    A = torch.from_numpy(host_input(oracle, m, n, np.float64).copy()).cuda()
    plan = tqr.TiledQR(m, n, b, torch.float64, steps=s)
    st = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(st):
        for _ in range(2):
            buf = torch.full((n, m + 8), -7.25, dtype=torch.float64, device="cuda")
            buf[:, :m] = A
            tau = torch.zeros((s, m), dtype=torch.float64, device="cuda")
            st.wait_stream(torch.cuda.default_stream())
            plan.execute(buf, tau, ldda=m + 8, stream=st.cuda_stream)
            plan.status(stream=st.cuda_stream)
            outs.append((buf, tau))
    st.synchronize()
    for buf, tau in outs:
        out = buf.cpu()
        assert torch.all(out[:, m:] == -7.25), "the engine wrote into the padding rows m .. ldda-1"
        assert torch.equal(out[:, :m], F) and torch.equal(tau.cpu(), t)


# ---- (d) fused least squares --------------------------------------------------------------------
LSQ = [(384, 256, 64), (1024, 512, 256)]
LSQ_CASES = [(m, n, b, nrhs, dt) for m, n, b in LSQ for dt in (np.float64, np.float32) for nrhs in (1, 17, 64, b + 1)]
LSQ_IDS = [f"{m}x{n}b{b}-{dn(dt)}-nrhs{nrhs}" for m, n, b, nrhs, dt in LSQ_CASES]


def lsq_problem(oracle, m, n, b, dt):
    key = ("lsq", m, n, b, dn(dt))
    if key not in _cache:
        A = oracle.randzo(m, n, dt, seed=7)
        B = oracle.randzo(m, b + 1, dt, seed=8)
        cond = float(np.linalg.cond(A.T.astype(np.float64)))
        assert cond < 20, cond
        A.setflags(write=False)
        B.setflags(write=False)
        _cache[key] = (A, B, cond)
    return _cache[key]


@pytest.mark.parametrize("m,n,b,nrhs,dt", LSQ_CASES, ids=LSQ_IDS)
def test_lstsq_fused(tqr, oracle, m, n, b, nrhs, dt):
    """tqr_lstsq_fused on [A | B | padding | guard column] and tqr.lstsq_fused: X and the residual
    norms against numpy.linalg.lstsq and against ApplyQ.lstsq on the ordinary factorisation (the
    bounds of tests/test_gpu_solve.py); A's columns are the ordinary factorisation bit for bit; the
    padding's contents reach nothing else; the column after the r*b columns is unchanged."""
    import torch
    A, B, cond = lsq_problem(oracle, m, n, b, dt)
    Bh = np.ascontiguousarray(B[:nrhs])
    r = -(-nrhs // b)
    dA, dB = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(Bh.copy()).cuda()
    AB = torch.full((n + r * b + 1, m), 3.5, dtype=dA.dtype, device="cuda")  # padding and guard: 3.5
    AB[:n] = dA
    AB[n:n + nrhs] = dB
    plan = tqr.TiledQR(m, n + r * b, b, dA.dtype, steps=n // b)
    tau = torch.zeros((n // b, m), dtype=dA.dtype, device="cuda")
    res = torch.full((nrhs,), -1.0, dtype=dA.dtype, device="cuda")
    plan.lstsq_fused(AB, tau, nrhs, res=res)
    plan.status()
    assert torch.all(AB[n + r * b] == 3.5), "the guard column after the r*b columns changed"
    # the ordinary factorisation of A, and tqr_lstsq on it
    F0 = dA.clone()
    t0 = torch.zeros_like(tau)
    full = tqr.TiledQR(m, n, b, dA.dtype)
    full.execute(F0, t0)
    full.status()
    assert torch.equal(AB[:n], F0) and torch.equal(tau, t0)
    ap = tqr.ApplyQ(m, n, b, dA.dtype)
    ap.prepare(F0, t0)
    dB2 = dB.clone()
    res2 = torch.empty_like(res)
    ap.lstsq(F0, dB2, res=res2)
    # the Python form (zero padding): the same X and residuals, bit for bit — columns are independent
    X, rs, F, tf = tqr.lstsq_fused(dA, dB, b)
    torch.cuda.synchronize()
    assert X.shape == (nrhs, n) and rs.shape == (nrhs,)
    assert torch.equal(X, AB[n:n + nrhs, :n]) and torch.equal(rs, res)
    assert torch.equal(F, F0) and torch.equal(tf, t0)
    assert np.array_equal(dA.cpu().numpy(), A) and np.array_equal(dB.cpu().numpy(), Bh)  # inputs untouched
    A64, B64 = A.T.astype(np.float64), Bh.T.astype(np.float64)
    Xn = np.linalg.lstsq(A64, B64, rcond=None)[0]  # n x nrhs
    rn = np.linalg.norm(A64 @ Xn - B64, axis=0)
    Xg = X.cpu().numpy().T.astype(np.float64)
    Xa = dB2.cpu().numpy()[:, :n].T.astype(np.float64)
    ex = float(np.linalg.norm(Xg - Xn) / np.linalg.norm(Xn))
    ea = float(np.linalg.norm(Xg - Xa) / np.linalg.norm(Xa))
    er = float(np.abs(res.cpu().numpy().astype(np.float64) - rn).max())
    era = float(np.abs((res - res2).cpu().numpy().astype(np.float64)).max())
    print(f"cond(A) = {cond:.2f}, |X - X_np|_F / |X_np|_F = {ex:.3e}, |X - X_apply|_F / |X_apply|_F = {ea:.3e}, "
          f"max|res - res_np| = {er:.3e}, max|res - res_apply| = {era:.3e}")
    assert ex <= tol(dt) * cond
    assert ea <= tol(dt) * cond
    assert er <= tol(dt) * float(np.linalg.norm(B64))
    assert era <= tol(dt) * float(np.linalg.norm(B64))


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=dn)
@pytest.mark.parametrize("m,n,b", LSQ)
def test_fused_factors_serve_the_apply(tqr, oracle, m, n, b, dt):
    """An ApplyQ handle for (m, n) prepared on the F, tau that tqr.lstsq_fused returns gives Q^T C of
    a fresh C (the oracle's tile kernels on the oracle's factorisation; the apply tests' bound).
    A is the apply tests' matrix of the shape (RANDZO seed 11 + b), not the least-squares one: on seed
    7 at 1024 x 512, b = 256 the fp32 oracle itself takes the other sign for the reflector of column
    337 than the fp64 oracle on the same input (max|F32 - F64| = 30.8; a pivot decided by rounding, as
    in test_gpu_factor.py::test_zero_row_sign_ambiguous), so elementwise fp32 parity is not defined
    there. That the fp32 oracle is a reference here is asserted (the reference's EPSILON, 1e-3)."""
    import torch
    A = oracle.randzo(m, n, dt, seed=11 + b)
    B = oracle.randzo(m, 3, dt, seed=8)
    _, _, F, tau = tqr.lstsq_fused(torch.from_numpy(A.copy()).cuda(), torch.from_numpy(B.copy()).cuda(), b)
    C = oracle.randzo(m, b, dt, seed=29)
    dC = torch.from_numpy(C.copy()).cuda()
    ap = tqr.ApplyQ(m, n, b, F.dtype)
    ap.prepare(F, tau, ldda=m)
    ap.apply(F, dC, trans=True, ldda=m)
    torch.cuda.synchronize()
    Fo, To = oracle.factor(A, b)
    F64, T64 = (Fo, To) if dt == np.float64 else oracle.factor(A.astype(np.float64), b)
    assert float(np.abs(Fo - F64).max()) <= 1e-3 and float(np.abs(To - T64).max()) <= 1e-3
    ref = oracle_qt_cols(oracle, Fo, To, C, b)
    ref64 = ref if dt == np.float64 else oracle_qt_cols(oracle, F64, T64, C.astype(np.float64), b)
    check_apply(dC.cpu().numpy(), ref, ref64, "Q^T C on the fused call's factors:")


# ---- (e) Q^T from a capped plan over [A | I] -----------------------------------------------------
@pytest.mark.parametrize("m,n,b", [(256, 128, 64), (512, 512, 256)])
def test_form_qt(tqr, oracle, m, n, b):
    """Q^T A = [R; 0], Q^T Q = I, and Q^T equals the apply of Q^T to an identity — each under the
    bound tests/test_gpu_apply.py uses for the same quantity."""
    import torch
    A = host_input(oracle, m, n, np.float64)
    dA = torch.from_numpy(A.copy()).cuda()
    Qt, F, tau = tqr.form_qt(dA, b)
    assert Qt.shape == (m, m) and F.shape == (n, m) and tau.shape == (n // b, m)
    ap = tqr.ApplyQ(m, n, b, torch.float64)
    ap.prepare(F, tau, ldda=m)
    eye = torch.eye(m, dtype=torch.float64, device="cuda")
    ap.apply(F, eye, trans=True)
    torch.cuda.synchronize()
    QT = Qt.cpu().numpy().T  # element (i, j) of Q^T (the tensor's row j is column j)
    Am, Fm = A.T, F.cpu().numpy().T
    got = QT @ Am
    R = np.triu(Fm)
    up = np.arange(m)[:, None] <= np.arange(n)[None, :]
    e_up = float(np.abs(got - R)[up].max())
    e_lo = float(np.abs(got)[~up].max()) if m > 1 else 0.0
    e_orth = float(np.abs(QT @ QT.T - np.eye(m)).max())
    print(f"max|triu(Q^T A) - R| = {e_up:.3e}, below the diagonal {e_lo:.3e}, max|Q^T Q - I| = {e_orth:.3e}")
    assert e_up <= 1e-11 * max(1.0, float(np.abs(R).max()))
    assert e_lo <= 1e-11 * float(np.abs(A).max())
    assert e_orth <= 1e-11
    ref = eye.cpu().numpy()
    check_apply(Qt.cpu().numpy(), ref, ref, "form_qt against the apply to an identity:")


def test_form_qt_rowgraded(tqr):
    """Q^T of a row-graded matrix (cond about 1e8, tests/inputs.py) is as orthogonal as that of a
    well-conditioned one: max|Q^T Q - I| at test_form_qt's bound, and Q^T A = [R; 0] relative to max|A|."""
    import torch
    import inputs
    m, n, b = shape = (256, 128, 64)
    A = inputs.matrix("rowgraded", shape)
    Qt, F, tau = tqr.form_qt(torch.from_numpy(A.copy()).cuda(), b)
    torch.cuda.synchronize()
    QT = Qt.cpu().numpy().T
    got = QT @ A.T
    R = np.triu(F.cpu().numpy().T)
    up = np.arange(m)[:, None] <= np.arange(n)[None, :]
    e_up, e_lo = float(np.abs(got - R)[up].max()), float(np.abs(got)[~up].max())
    e_orth = float(np.abs(QT @ QT.T - np.eye(m)).max())
    print(f"max|triu(Q^T A) - R| = {e_up:.3e}, below the diagonal {e_lo:.3e}, max|Q^T Q - I| = {e_orth:.3e}")
    assert np.isfinite(QT).all()
    assert e_orth <= 1e-11
    assert e_up <= 1e-11 * max(1.0, float(np.abs(R).max()))
    assert e_lo <= 1e-11 * float(np.abs(A).max())


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=dn)
@pytest.mark.parametrize("m,n,b,nrhs", [(384, 256, 64, 17), (1024, 512, 256, 257)])
def test_lstsq_fused_poisoned_padding(tqr, oracle, m, n, b, nrhs, dt):
    """NaN in the padding columns nrhs .. r*b-1 on entry: X, the rows n .. m-1 of Q^T B, the residual
    norms, the factorisation of A and tau are the bits of the run with zero padding (include/tqr.h:
    "what they hold on entry influences nothing else"), and the NaN stays in the padding."""
    import torch
    A, B, _ = lsq_problem(oracle, m, n, b, dt)
    r = -(-nrhs // b)
    assert nrhs < r * b
    outs = []
    for pad in (0.0, float("nan")):
        AB = torch.full((n + r * b, m), pad, dtype=tdt(dt), device="cuda")
        AB[:n] = torch.from_numpy(A.copy()).cuda()
        AB[n:n + nrhs] = torch.from_numpy(B[:nrhs].copy()).cuda()
        plan = tqr.TiledQR(m, n + r * b, b, AB.dtype, steps=n // b)
        tau = torch.zeros((n // b, m), dtype=AB.dtype, device="cuda")
        res = torch.full((nrhs,), -1.0, dtype=AB.dtype, device="cuda")
        plan.lstsq_fused(AB, tau, nrhs, res=res)
        plan.status()
        outs.append((AB.cpu(), tau.cpu(), res.cpu()))
    (AB0, tau0, res0), (AB1, tau1, res1) = outs
    assert bool(torch.isfinite(AB0).all()) and bool(torch.isfinite(res0).all())
    assert torch.equal(AB1[:n + nrhs], AB0[:n + nrhs]) and torch.equal(tau1, tau0) and torch.equal(res1, res0)
    assert bool(torch.isnan(AB1[n + nrhs:]).all())


# ---- (g) argument errors on live objects --------------------------------------------------------
def test_einval_on_live_plans(tqr):
    import torch
    L = tqr.lib()
    m, n, b = 128, 64, 32
    AB = torch.zeros((n + 2 * b, m), dtype=torch.float64, device="cuda")
    tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
    a, t = P(AB.data_ptr()), P(tau.data_ptr())
    uncapped = tqr.TiledQR(m, n + b, b, torch.float64)
    assert L.tqr_lstsq_fused(uncapped.h, a, m, t, 1, None, None) == -1            # not a capped plan
    nob = tqr.TiledQR(m, n, b, torch.float64, steps=n // b)
    assert L.tqr_lstsq_fused(nob.h, a, m, t, 1, None, None) == -1                 # steps*b = the plan's n: no B
    plan = tqr.TiledQR(m, n + b, b, torch.float64, steps=n // b)                   # r = 1
    assert L.tqr_lstsq_fused(plan.h, a, m, t, 0, None, None) == -1                # nrhs < 1
    assert L.tqr_lstsq_fused(plan.h, a, m, t, b + 1, None, None) == -1            # nrhs > r*b
    assert L.tqr_lstsq_fused(plan.h, None, m, t, 1, None, None) == -1
    assert L.tqr_lstsq_fused(plan.h, a, m, None, 1, None, None) == -1
    assert L.tqr_lstsq_fused(plan.h, a, m - 1, t, 1, None, None) == -1            # ldda < m
    # a plan whose steps*b is not the n that nrhs / r imply: 2 right-hand sides after ONE tile column
    # of A would be r = 2 tile columns of B, but the call can only see that as B's columns — so nrhs
    # beyond the columns after steps*b is what is rejected
    short = tqr.TiledQR(m, n + b, b, torch.float64, steps=1)                       # A = 32 columns, r = 2
    assert L.tqr_lstsq_fused(short.h, a, m, t, 2 * b + 1, None, None) == -1
    # multi-GPU calls on a capped plan
    buf = ctypes.create_string_buffer(4096)
    seen = ctypes.c_ulonglong()
    assert L.tqr_dist_export(plan.h, buf, 4096) == -1
    assert L.tqr_dist_import(plan.h, buf, 4096) == -1
    assert L.tqr_dist_probe(plan.h, 0, ctypes.byref(seen)) == -1
    assert L.tqr_dist_reset(plan.h, None) == -1
    assert L.tqr_dist_owner(plan.h, 0) == -1
    assert L.tqr_dist_local_cols(plan.h) == -1
    with pytest.raises(tqr.TQRError):
        tqr.lstsq_fused(torch.zeros((64, 32), dtype=torch.float64, device="cuda"),
                        torch.zeros((1, 32), dtype=torch.float64, device="cuda"), 32)  # m < n
    torch.cuda.synchronize()
