"""The fp64 engine on chain tasks of several elements, at small shapes (cases and regimes:
tests/segments.py; that each case's list holds its regimes, and the numeric conditions on the oracle
alone: tests/test_segments_cpu.py).

Under the default knobs every fp64 plan of at most 32 tile rows runs one TSMQR per chain task
(csrc/flowplan.cpp default_tail), so the small shapes of the other test files never run the
TSMQR-to-TSMQR hand-over: the head strip handed on inside the task, the next element's strip streamed
in during the last reflector group (whole-line layout included), the in-flight counts that go with it,
and the state a workgroup carries from one chain task to the next. The cases here do, in milliseconds.

The reference is the oracle at the project's bounds (steps_ref.assert_close). Where the project states
an exact relation the test compares bits, with no tolerance:
  * any valid task order and any segmentation give the same bits (test_gpu_factor.py::
    test_task_order_and_lookahead_segments_bitexact): every run here equals the run of the same shape
    and chain form with every step in the one-element tail (segments.ALL_TAIL), which is the list the
    other test files check;
  * whole-line strips on and off (test_gpu_strip_lines.py);
  * where the matrix lies, which stream runs it and what the plan ran before (test_gpu_inputs.py);
  * column scaling by powers of two (test_gpu_inputs.py).
Every execute is followed by status(): the engine bounds its waits and reports a timeout there.
"""
import numpy as np
import pytest

import inputs
import segments as S
from segments import BY_NAME, CASES
from steps_ref import assert_close, expand_tau_steps, partial, tol

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
_plans, _runs = {}, {}


def envkey(env):
    return tuple(sorted(env.items()))


def plan_for(tqr, shape, env, steps=None):
    """The plan of `shape` created under the knobs `env` alone (cached: plans are reusable)."""
    import torch
    key = (shape, envkey(env), steps)
    if key not in _plans:
        m, n, b = shape
        with S.knobs(env):
            _plans[key] = tqr.TiledQR(m, n, b, torch.float64, steps=steps)
    return _plans[key]


def execute(plan, A):
    """(F, tau) as CPU tensors of one packed default-stream run on the host array A (n, m)."""
    import torch
    dA = torch.from_numpy(np.array(A)).cuda()
    tau = torch.zeros((plan.kmax, A.shape[1]), dtype=torch.float64, device="cuda")
    plan.execute(dA, tau)
    plan.status()
    return dA.cpu(), tau.cpu()


def run(tqr, shape, env, key, A):
    """execute() of the shape's plan under `env` on the input named `key`, once."""
    k = (shape, envkey(env), key)
    if k not in _runs:
        _runs[k] = execute(plan_for(tqr, shape, env), A)
    return _runs[k]


def differing_tiles(X, Y, b):
    d = (X != Y).numpy()
    return sorted({(int(i) // b, int(j) // b) for j, i in zip(*np.nonzero(d))})[:20]


def assert_same_bits(F, t, F0, t0, b, what=""):
    import torch
    assert torch.equal(F, F0), f"{what}: differing tiles (row, column): {differing_tiles(F, F0, b)}"
    assert torch.equal(t, t0), what


def factor(tqr, case, key, A, form=None):
    """(F, T) as numpy arrays of the case's plan (its knobs, plus the chain form's) on A, after asserting
    that they are the bits of the all-tail plan of the same form on the same input."""
    m, n, b = case.shape
    form = form or {}
    F, t = run(tqr, case.shape, {**case.env, **form}, key, A)
    F0, t0 = run(tqr, case.shape, {**S.ALL_TAIL, **form}, key, A)
    assert_same_bits(F, t, F0, t0, b, f"{case.name} {form} against the all-tail plan")
    return F.numpy(), expand_tau_steps(t.numpy(), m, n, b)


# ---- every case, default chain form, RANDZO -------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_vs_oracle_and_all_tail(tqr, oracle, case):
    """F and tau against the oracle; bit-identical to the all-tail plan; the plan's device list is the
    host export of its spec and holds the regimes the case is listed for; status clean (in execute)."""
    p, q = case.tiles
    b = case.shape[2]
    A = S.randzo(oracle, case.shape)
    F_ref, T_ref = S.randzo_ref(oracle, case.shape)
    F, T = factor(tqr, case, "randzo", A)
    assert_close(F, T, F_ref, T_ref)
    for env in (case.env, S.ALL_TAIL):
        plan = plan_for(tqr, case.shape, env)
        dev, want = tqr.plan_tasks(plan), S.export(tqr, case, env=env)
        assert dev.shape == want.shape and (dev == want).all(), env
    plan = plan_for(tqr, case.shape, case.env)
    info, dev = tqr.plan_info(plan), tqr.plan_tasks(plan)
    assert info["engine"] == 1 and info["ntasks"] == len(dev)
    if "TQR_FLOW_GRID" in case.env:
        assert info["grid"] == case.grid
    got = S.regimes(p, q, b, dev, grid=info["grid"], tqr=tqr)
    assert set(case.reach) <= got, sorted(set(case.reach) - got)


# ---- chain forms on multi-element segments ----------------------------------------------------------
FORMS = {"asm1": {"TQR_CHAIN_ASM": "1"}, "asm0": {"TQR_CHAIN_ASM": "0"}, "r": {"TQR_FLOW_SHAPE": "r"},
         "w4": {"TQR_FLOW_SHAPE": "w4"}, "skip0": {"TQR_UNMQR_SKIP": "0"}, "lines0": {"TQR_STRIP_LINES": "0"}}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["T0", "MIX"])
def test_chain_forms_on_multi_element_segments(tqr, oracle, name, form):
    """The A/B chain forms at b = 256 (the resident form exists for that tile only; the whole-line
    layout too): the whole next strip loaded in the hand-over (asm1), the compiler-scheduled chain
    (asm0, flow.hpp flow_chain), the resident one-wave-per-SIMD form (r, chain_res.hpp), two 4-wave
    workgroups per CU (w4), UNMQR elements on the full bodies (skip0), standard strips only (lines0).
    Each against the oracle, and against the SAME form's all-tail plan bit for bit: in every form the
    segment decides only which loads, stores and waits surround a reflector group's body (has_next /
    xin in chain_asm.hpp, flow.hpp and chain_res.hpp) — the MFMA stream of a group of an element is one
    code path, and the head strip handed on in registers holds the fp64 values a one-element segment
    stores and the next one loads. lines0 must also equal the default form (whole lines on) bit for bit:
    the layout permutes the strip's 16-byte pieces in memory and nothing else."""
    case = BY_NAME[name]
    A = S.randzo(oracle, case.shape)
    F_ref, T_ref = S.randzo_ref(oracle, case.shape)
    F, T = factor(tqr, case, "randzo", A, form=FORMS[form])
    assert_close(F, T, F_ref, T_ref)
    p, q = case.tiles
    plan = plan_for(tqr, case.shape, {**case.env, **FORMS[form]})
    got = S.regimes(p, q, case.shape[2], tqr.plan_tasks(plan), tqr=tqr)
    assert {"handover", "full0", "rem1"} <= got, sorted(got)
    if form == "lines0":
        Fd, Td = factor(tqr, case, "randzo", A)
        assert np.array_equal(F, Fd) and np.array_equal(T, Td)


# ---- inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.SCALE_CASES)
def test_column_scaling_bitexact(tqr, oracle, name):
    case = BY_NAME[name]
    A = inputs.matrix("gauss", case.shape)
    d = inputs.scaling(case.shape, np.float64)
    F, T = factor(tqr, case, "gauss", A)
    assert_close(F, T, *S.family_ref(oracle, "gauss", case.shape))
    Fs, Ts = factor(tqr, case, "gauss-scaled", inputs.scale_columns(A, d))
    inputs.assert_covariant(F, T, Fs, Ts, d)


def test_zero_first_pivot(tqr, oracle):
    """+0.0 and -0.0 over a live tail on T0: each against the oracle, and the two bit-identical
    (sign(0) = +1 whatever the zero's sign bit, as in the reference)."""
    case = BY_NAME["T0"]
    outs = []
    for zero in (0.0, -0.0):
        A = S.zero_pivot_input(case.shape, zero)
        F, T = factor(tqr, case, f"zero{'-' if np.signbit(zero) else '+'}", A)
        assert_close(F, T, *S.zero_pivot_ref(oracle, case.shape, zero))
        outs.append((F, T))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_structured_family(tqr, oracle):
    """matrix("structured") on T0: unit columns, a zero column (tau = 2, a zero on R's diagonal) and
    column n/2 + 6 an exact copy of column 3. Below the diagonal that copy is rounding noise after step
    0, so the direction of its reflector is decided by the noise, in the oracle as much as here: from
    that column on V, tau and the rows of R below it are not unique (test_gpu_waves.py::
    test_wave_structured; measured here: max|F - F_oracle| = 7.6e-13 in the columns before the copy and
    92 in the columns from it on). Against the oracle what is well posed, as that test does: elementwise parity of every column
    before the copy (column j of a Householder QR depends on columns <= j only) and of their taus, the
    residual of the whole factorisation, |R| of the leading columns. The whole result, the columns after
    the copy included, is the all-tail plan's bit for bit (in factor())."""
    case = BY_NAME["T0"]
    m, n, b = case.shape
    A = inputs.matrix("structured", case.shape)
    F, T = factor(tqr, case, "structured", A)
    F_ref, T_ref = S.family_ref(oracle, "structured", case.shape)
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert oracle.residual(A, F, T, b) <= 1e-13
    c = n // 2 + 6  # the copied column
    k, c_in = divmod(c, b)
    print(f"structured {case.shape}: max|F - F_oracle| columns < {c}: {np.abs(F[:c] - F_ref[:c]).max():.3e}, "
          f"columns >= {c}: {np.abs(F[c:] - F_ref[c:]).max():.3e}")
    Tm, Tm_ref = T.copy(), T_ref.copy()
    for X in (Tm, Tm_ref):  # taus of step k live in row k*b, column c_in of every tile row: drop c_in ..
        X[k * b].reshape(m // b, b)[:, c_in:] = 0
        X[(k + 1) * b:] = 0
    assert_close(F[:c], Tm, F_ref[:c], Tm_ref)
    assert (T[inputs.ZERO_COL // b * b].reshape(m // b, b)[:, inputs.ZERO_COL % b] == 2).all()
    R, R_ref = inputs.r_of(F)[:, :c], inputs.r_of(F_ref)[:, :c]
    assert np.abs(np.abs(R) - np.abs(R_ref)).max() <= 1e-11 * np.abs(R_ref).max()


@pytest.mark.parametrize("name", S.LD_CASES)
@pytest.mark.parametrize("family", S.CONDITIONED)
def test_accuracy_vs_longdouble(tqr, oracle, family, name):
    """The conditions of test_gpu_inputs.py::test_accuracy_vs_longdouble at the b = 64 cases."""
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    case = BY_NAME[name]
    b = case.shape[2]
    A = inputs.matrix(family, case.shape)
    F_ref, _ = S.family_ref(oracle, family, case.shape)
    R_ld = inputs.r_longdouble(family, case.shape)
    F, T = factor(tqr, case, family, A)
    res = oracle.residual(A, F, T, b)
    cn = inputs.colnorm_rel_err(A, F)
    e_gpu, e_orc = inputs.col_rel_err(F, R_ld), inputs.col_rel_err(F_ref, R_ld)
    print(f"{family} {case.name} {case.shape}: residual {res:.3e}, column norms {cn:.3e}, "
          f"e_gpu {e_gpu:.3e}, e_oracle {e_orc:.3e}, ratio {e_gpu / e_orc:.3f}")
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert res <= 1e-13
    assert cn <= 1e-12
    assert e_gpu <= 1.5 * e_orc


@pytest.mark.parametrize("name", S.FAMILY_CASES_256)
@pytest.mark.parametrize("family", S.CONDITIONED)
def test_conditioned_families_b256(tqr, oracle, family, name):
    """The same families on the generated b = 256 chain with whole lines: residual, column norms and
    the bits of the all-tail plan (in factor()). The 1.5 x comparison with the extended-precision QR is
    carried by the b = 64 cases above (the numpy.longdouble QR of this shape takes minutes); the
    all-tail plan's arithmetic is what test_gpu_inputs.py holds to that bound at 768 x 512, b = 256."""
    case = BY_NAME[name]
    A = inputs.matrix(family, case.shape)
    F, T = factor(tqr, case, family, A)
    res = oracle.residual(A, F, T, case.shape[2])
    cn = inputs.colnorm_rel_err(A, F)
    print(f"{family} {case.name} {case.shape}: residual {res:.3e}, column norms {cn:.3e}")
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert res <= 1e-13
    assert cn <= 1e-12


# ---- device arrays ---------------------------------------------------------------------------------
DEV_CASES = ["T0", "D64"]


def device_base(tqr, oracle, case):
    """(plan, F, tau) of the packed default-stream run on the gauss matrix, checked against the oracle."""
    m, n, b = case.shape
    A = inputs.matrix("gauss", case.shape)
    F, t = run(tqr, case.shape, case.env, "gauss", A)
    assert_close(F.numpy(), expand_tau_steps(t.numpy(), m, n, b), *S.family_ref(oracle, "gauss", case.shape))
    return plan_for(tqr, case.shape, case.env), F, t


@pytest.mark.parametrize("pad", [8, 1])
@pytest.mark.parametrize("name", DEV_CASES)
def test_padded_ldda(tqr, oracle, name, pad):
    """ldda = m + 8 and m + 1; the odd one puts T0's whole-line strips on columns that are not whole
    lines apart (and 8 bytes off the 16-byte accesses), inside a hand-over."""
    import torch
    case = BY_NAME[name]
    m, n, b = case.shape
    plan, F0, tau0 = device_base(tqr, oracle, case)
    ldda = m + pad
    buf = torch.full((n, ldda), SENTINEL, dtype=torch.float64, device="cuda")
    buf[:, :m] = torch.from_numpy(np.array(inputs.matrix("gauss", case.shape))).cuda()
    tau = torch.zeros_like(tau0, device="cuda")
    plan.execute(buf, tau, ldda=ldda)
    plan.status()
    out = buf.cpu()
    assert torch.all(out[:, m:] == SENTINEL), "the engine wrote into the padding rows m .. ldda-1"
    assert_same_bits(out[:, :m], tau.cpu(), F0, tau0, b, f"ldda = m + {pad}")


@pytest.mark.parametrize("name", DEV_CASES)
def test_offset_base(tqr, oracle, name):
    import torch
    case = BY_NAME[name]
    m, n, b = case.shape
    plan, F0, tau0 = device_base(tqr, oracle, case)
    big = torch.full((n * m + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    view = big[1:1 + n * m].view(n, m)
    view.copy_(torch.from_numpy(np.array(inputs.matrix("gauss", case.shape))).cuda())
    assert view.data_ptr() == big.data_ptr() + big.element_size()
    tau = torch.zeros_like(tau0, device="cuda")
    plan.execute(view, tau)
    plan.status()
    out = big.cpu()
    assert out[0] == SENTINEL and out[-1] == SENTINEL
    assert_same_bits(out[1:-1].view(n, m), tau.cpu(), F0, tau0, b, "base one element into the allocation")


@pytest.mark.parametrize("name", DEV_CASES)
def test_stream_and_plan_reuse(tqr, oracle, name):
    """One plan on a side stream: X, Y, X. The third result is the first bit for bit and both are the
    default-stream one; the Y in between is the oracle's factorisation of Y."""
    import torch
    case = BY_NAME[name]
    m, n, b = case.shape
    plan, F0, tau0 = device_base(tqr, oracle, case)
    X = inputs.matrix("gauss", case.shape)
    Y = inputs.matrix("gauss", case.shape, offset=7)
    s = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(s):
        for M in (X, Y, X):
            dA = torch.from_numpy(np.array(M)).to("cuda", non_blocking=False)
            tau = torch.zeros_like(tau0, device="cuda")
            s.wait_stream(torch.cuda.default_stream())
            plan.execute(dA, tau, stream=s.cuda_stream)
            outs.append((dA, tau))
        plan.status(stream=s.cuda_stream)
    s.synchronize()
    (F1, t1), (F2, t2), (F3, t3) = [(a.cpu(), t.cpu()) for a, t in outs]
    assert_same_bits(F3, t3, F1, t1, b, "X after Y against X")
    assert_same_bits(F1, t1, F0, tau0, b, "side stream against the default stream")
    assert_close(F2.numpy(), expand_tau_steps(t2.numpy(), m, n, b), *S.family_ref(oracle, "gauss", case.shape, offset=7))


# ---- queued workgroups -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [{}, {"TQR_CHAIN_ASM": "0"}], ids=["default", "asm0"])
def test_queued_workgroups(tqr, oracle, form):
    """T0's list on 6 workgroups (8.7 tasks each, chain task after chain task on one workgroup: the
    buffer parity, the LDS tail words and the in-flight counts carried from task to task) gives T0's
    bits. A topological list dequeued in order cannot deadlock on any grid >= 1 (flow.hpp)."""
    q_, t0 = BY_NAME["Q"], BY_NAME["T0"]
    assert q_.shape == t0.shape
    A = S.randzo(oracle, t0.shape)
    Fq, tq = run(tqr, q_.shape, {**q_.env, **form}, "randzo", A)
    F0, tt = run(tqr, t0.shape, {**t0.env, **form}, "randzo", A)
    info = tqr.plan_info(plan_for(tqr, q_.shape, {**q_.env, **form}))
    assert info["grid"] == q_.grid and info["ntasks"] >= 8 * info["grid"]
    assert_same_bits(Fq, tq, F0, tt, q_.shape[2], "6 workgroups against the whole device")
    m, n, b = t0.shape
    assert_close(Fq.numpy(), expand_tau_steps(tq.numpy(), m, n, b), *S.randzo_ref(oracle, t0.shape))


# ---- what is built on the list -----------------------------------------------------------------------
def test_capped_plan_and_resumption(tqr, oracle):
    """steps = 2 on T0's shape under TQR_TAIL=0 (its list holds UNMQR + 8 and a remainder of one, and
    at step 1 whole-line strips handed over; the last step stores standard): against
    steps_ref.partial, and an ordinary plan on the trailing block completes it to the bits of the
    full plan."""
    import torch
    case = BY_NAME["T0"]
    m, n, b = case.shape
    s = 2
    p, q = case.tiles
    A = S.randzo(oracle, case.shape)
    plan = plan_for(tqr, case.shape, case.env, steps=s)
    dev, want = tqr.plan_tasks(plan), S.export(tqr, case, steps=s)
    assert dev.shape == want.shape and (dev == want).all()
    assert {"handover", "full0", "rem1", "lines_handover"} <= S.regimes(p, q, b, dev, steps=s, tqr=tqr)
    dA = torch.from_numpy(np.array(A)).cuda()
    tau = torch.zeros((s, m), dtype=torch.float64, device="cuda")
    plan.execute(dA, tau)
    plan.status()
    F, t = dA.cpu(), tau.cpu()
    F_ref, T_ref = inputs._frozen(("seg-partial", case.shape, s), lambda: partial(oracle, A, b, s))
    assert_close(F.numpy(), expand_tau_steps(t.numpy(), m, n, b), F_ref, T_ref)
    m2, n2 = m - s * b, n - s * b
    rest = plan_for(tqr, (m2, n2, b), case.env)
    tau2 = torch.zeros((rest.kmax, m2), dtype=torch.float64, device="cuda")
    rest.execute(dA.view(-1)[s * b * m + s * b:], tau2, ldda=m)
    rest.status()
    tall = torch.zeros((min(m, n) // b, m), dtype=torch.float64)
    tall[:s] = t
    tall[s:, s * b:] = tau2.cpu()
    Ff, tf = run(tqr, case.shape, case.env, "randzo", A)
    assert_same_bits(dA.cpu(), tall, Ff, tf, b, "capped plan resumed against the full plan")


def test_lstsq_fused(tqr, oracle):
    """tqr_lstsq_fused on [A | B], 5 right-hand sides, A 2560 x 768 (the capped plan is T0's shape with
    3 steps) under TQR_TAIL=0: X and the residual norms against numpy.linalg.lstsq at the bounds of
    test_gpu_steps.py::test_lstsq_fused; A's columns and tau are the ordinary plan's bits; the whole
    call is bit-identical to the all-tail plan's."""
    import torch
    case = BY_NAME["T0"]
    m, nb, b = case.shape
    n, nrhs = nb - b, 5
    A = inputs._frozen(("seg-lsq-A", m, n), lambda: oracle.randzo(m, n, np.float64, seed=7))
    B = inputs._frozen(("seg-lsq-B", m, nrhs), lambda: oracle.randzo(m, nrhs, np.float64, seed=8))
    cond = float(np.linalg.cond(A.T))
    assert cond < 20, cond
    outs = []
    for env in (case.env, S.ALL_TAIL):
        plan = plan_for(tqr, case.shape, env, steps=n // b)
        AB = torch.full((nb + 1, m), 3.5, dtype=torch.float64, device="cuda")  # padding and guard column: 3.5
        AB[:n] = torch.from_numpy(np.array(A)).cuda()
        AB[n:n + nrhs] = torch.from_numpy(np.array(B)).cuda()
        tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
        res = torch.full((nrhs,), -1.0, dtype=torch.float64, device="cuda")
        plan.lstsq_fused(AB, tau, nrhs, res=res)
        plan.status()
        assert torch.all(AB[nb] == 3.5), "the guard column after the r*b columns changed"
        outs.append((AB.cpu(), tau.cpu(), res.cpu()))
    (AB, tau, res), (AB0, tau0, res0) = outs
    assert torch.equal(AB[:n + nrhs], AB0[:n + nrhs]) and torch.equal(tau, tau0) and torch.equal(res, res0)
    p, q = case.tiles
    dev = tqr.plan_tasks(plan_for(tqr, case.shape, case.env, steps=n // b))
    assert {"handover", "full0", "rem1", "lines_handover"} <= S.regimes(p, q, b, dev, steps=n // b, tqr=tqr)
    Ff, tf = execute(plan_for(tqr, (m, n, b), case.env), A)
    assert torch.equal(AB[:n], Ff) and torch.equal(tau, tf)
    A64, B64 = A.T, B.T
    Xn = np.linalg.lstsq(A64, B64, rcond=None)[0]
    rn = np.linalg.norm(A64 @ Xn - B64, axis=0)
    Xg = AB[n:n + nrhs, :n].numpy().T
    ex = float(np.linalg.norm(Xg - Xn) / np.linalg.norm(Xn))
    er = float(np.abs(res.numpy() - rn).max())
    print(f"cond(A) = {cond:.2f}, |X - X_np|_F / |X_np|_F = {ex:.3e}, max|res - res_np| = {er:.3e}")
    assert ex <= tol(np.float64) * cond
    assert er <= tol(np.float64) * float(np.linalg.norm(B64))


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("name", ["T0", "MIX"])
def test_host_pointer_path(tqr, oracle, name, pad):
    """tqr.geqrt_host under the case's knobs: the launch's DOWN tasks wait on counts that xfer.hpp
    recomputes from the plan's knobs (nseg_of_chain per chain) — a count larger than the segments that
    exist times out (an error here), a smaller one downloads a column before it is final (wrong values
    here). Against the oracle, rows beyond m untouched, and the bits of the device-pointer plan."""
    case = BY_NAME[name]
    m, n, b = case.shape
    A = S.randzo(oracle, case.shape)
    F = np.full((n, m + pad), 7.25)
    F[:, :m] = A
    tqr.cache_clear()
    try:
        with S.knobs(case.env):
            T = tqr.geqrt_host(F, b, m=m)
    finally:
        tqr.cache_clear()
    assert np.all(F[:, m:] == 7.25) and np.all(T[:, m:] == 0)
    Fh, Th = np.ascontiguousarray(F[:, :m]), np.ascontiguousarray(T[:, :m])
    assert_close(Fh, Th, *S.randzo_ref(oracle, case.shape))
    Fd, Td = factor(tqr, case, "randzo", A)
    assert np.array_equal(Fh, Fd) and np.array_equal(Th, Td)
