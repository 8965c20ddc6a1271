"""The wave engine (tqr.h TQR_ENGINE_WAVES: BFS waves of the reference DAG, k_panel / k_update launches
on two side streams joined to the caller's stream by events) as a factorisation on device pointers,
and the contracts both engines share: where the matrix lies, stream ordering, one plan shared by
threads and streams, the cached one-shot helpers, the profile counters. Generators, shapes and the
extended-precision reference: tests/inputs.py; that the oracle alone meets every condition used here
at these shapes: tests/test_inputs_cpu.py.

Tolerances are the project's: test_gpu_factor.assert_close (fp64 1e-11 scaled, fp32 1e-3),
test_gpu_inputs.test_accuracy_vs_longdouble's and test_accuracy_fp32's bounds, and equality of bits
wherever the arithmetic cannot depend on what is varied.

A. the wave engine against the oracle, the column-scaling relation and the long-double QR;
B. padded ldda, an offset base, a non-default stream with plan reuse, profile on / off: same bits;
C. input produced and result consumed on the caller's stream with no host synchronisation;
D. one plan shared by two host threads, and by two streams of one thread;
E. the host-pointer API on the wave engine, and cudaQRFull;
F. tqr_dgeqrt_tiled / tqr_sgeqrt_tiled;
G. tqr_plan_stats, and what a wave plan refuses;
H. the wave engine's factors under tqr_apply and least squares;
I. the two engines' bits against each other.
"""
import ctypes
import threading

import numpy as np
import pytest

import inputs
from inputs import FAMILIES, WAVE_ACC_SHAPES, WAVE_ACC_SHAPES32, WAVE_SHAPES, dtname
from test_gpu_factor import assert_close

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
WAVE_CASES = [(s, dt) for s in WAVE_SHAPES for dt in (F64, F32)]
DEV_CASES = [((256, 192, 64), F64), ((768, 768, 256), F64), ((768, 768, 256), F32), ((64, 64, 16), F32)]
SHARE_CASES = [((256, 192, 64), F64), ((768, 768, 256), F64)]
ENGINES = ["waves", "flow"]
SENTINEL = -7.25
SMALL = (256, 192, 64)
TQR_EINVAL = -1


def ids(cases):
    return [f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in cases]


def sid(shape):
    return "%dx%db%d" % shape


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


_plans = {}
_runs = {}


def plan_of(tqr, engine, shape, dt):
    """One plan per (engine, shape, dtype) for the whole module: every variant reuses it."""
    key = (engine, shape, dtname(dt))
    if key not in _plans:
        m, n, b = shape
        _plans[key] = tqr.TiledQR(m, n, b, tdt(dt), engine=engine)
        assert tqr.plan_info(_plans[key])["engine"] == tqr.ENGINES[engine]
    return _plans[key]


def execute(plan, A, tau_fill=0.0):
    """Packed (ldda = m), default stream, host-synchronised: (F, tau) as torch CPU tensors. tau has one
    guard row behind its kmax rows, filled like the rest with tau_fill."""
    import torch
    dA = torch.from_numpy(np.array(A)).cuda()
    tau = torch.full((plan.kmax + 1, plan.m), tau_fill, dtype=dA.dtype, device="cuda")
    torch.cuda.synchronize()
    plan.execute(dA, tau)
    plan.status()
    torch.cuda.synchronize()
    return dA.cpu(), tau.cpu()


def base(tqr, engine, shape, dt, offset=0):
    """(plan, F, tau (kmax, m)) of the plan's packed default-stream run on the shape's gauss matrix
    (offset: another matrix of the same shape), computed once, read-only by convention."""
    key = (engine, shape, dtname(dt), offset)
    plan = plan_of(tqr, engine, shape, dt)
    if key not in _runs:
        F, tau = execute(plan, inputs.matrix("gauss", shape, dt, offset))
        _runs[key] = (F, tau[:plan.kmax].clone())
    return (plan,) + _runs[key]


def as_host(tqr, F, tau, shape):
    """numpy F and the reference's m x n tau matrix from a device-path result."""
    m, n, b = shape
    return F.numpy(), tqr.expand_tau(tau.numpy()[:min(m, n) // b], m, n, b)


def wave_factor(tqr, A, shape):
    F, tau = execute(plan_of(tqr, "waves", shape, A.dtype), A)
    return as_host(tqr, F, tau, shape)


# ---- A. the wave engine against the references -------------------------------------------------
@pytest.mark.parametrize("shape,dt", WAVE_CASES, ids=ids(WAVE_CASES))
def test_wave_vs_oracle(tqr, oracle, shape, dt):
    """tqr_plan_execute on a wave plan against the oracle; of the compact tau only row k, elements
    k*b .. m-1, is written (the guard row behind it and the elements above row k*b keep their fill)."""
    import torch
    m, n, b = shape
    plan = plan_of(tqr, "waves", shape, dt)
    assert tqr.plan_info(plan)["engine"] == 0
    F, tau = execute(plan, inputs.matrix("gauss", shape, dt), tau_fill=SENTINEL)
    assert torch.isfinite(F).all() and torch.isfinite(tau).all()
    assert torch.all(tau[plan.kmax] == SENTINEL), "the engine wrote behind the compact tau"
    for k in range(plan.kmax):
        assert torch.all(tau[k, :k * b] == SENTINEL), f"tau column {k} was written above row {k * b}"
        assert torch.all(tau[k, k * b:] != SENTINEL), f"tau column {k} was not written from row {k * b} on"
    F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, dt)
    assert_close(*as_host(tqr, F, tau, shape), F_ref, T_ref)
    # the module's shared run (tau zero-filled) has the same bits
    _, F0, tau0 = base(tqr, "waves", shape, dt)
    assert torch.equal(F, F0)
    for k in range(plan.kmax):
        assert torch.equal(tau[k, k * b:], tau0[k, k * b:]) and not tau0[k, :k * b].any()


@pytest.mark.parametrize("shape,dt", WAVE_CASES, ids=ids(WAVE_CASES))
def test_wave_column_scaling_bitexact(tqr, oracle, shape, dt):
    """factor(A D) = (R D, V, tau) bit for bit on the wave engine's own results (inputs.assert_covariant;
    the oracle satisfies it at these shapes: test_inputs_cpu.py). No tolerance."""
    A = inputs.matrix("gauss", shape, dt)
    d = inputs.scaling(shape, dt)
    _, F, tau = base(tqr, "waves", shape, dt)
    F, T = as_host(tqr, F, tau, shape)
    F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, dt)
    assert_close(F, T, F_ref, T_ref)
    Fs, Ts = wave_factor(tqr, inputs.scale_columns(A, d), shape)
    inputs.assert_covariant(F, T, Fs, Ts, d)


@pytest.mark.parametrize("shape", WAVE_ACC_SHAPES, ids=sid)
@pytest.mark.parametrize("family", FAMILIES)
def test_wave_accuracy_vs_longdouble(tqr, oracle, family, shape):
    """test_gpu_inputs.test_accuracy_vs_longdouble on the wave engine: the same three sign-free bounds,
    and the elementwise comparison for gauss only, for the reason stated there."""
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    b = shape[2]
    A = inputs.matrix(family, shape)
    F_ref, T_ref = inputs.oracle_factor(oracle, family, shape)
    R_ld = inputs.r_longdouble(family, shape)
    F, T = wave_factor(tqr, A, shape)
    res = oracle.residual(A, F, T, b)
    cn = inputs.colnorm_rel_err(A, F)
    e_gpu, e_orc = inputs.col_rel_err(F, R_ld), inputs.col_rel_err(F_ref, R_ld)
    print(f"waves {family} {shape}: residual {res:.3e}, column norms {cn:.3e}, "
          f"e_gpu {e_gpu:.3e}, e_oracle {e_orc:.3e}, ratio {e_gpu / e_orc:.3f}")
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert res <= 1e-13
    assert cn <= 1e-12
    assert e_gpu <= 1.5 * e_orc
    if family == "gauss":
        assert_close(F, T, F_ref, T_ref)


@pytest.mark.parametrize("shape", WAVE_ACC_SHAPES32, ids=sid)
def test_wave_accuracy_fp32(tqr, oracle, shape):
    """test_gpu_inputs.test_accuracy_fp32's three conditions on the wave engine."""
    b = shape[2]
    A = inputs.matrix("gauss", shape, F32)
    F32o, T32o = inputs.oracle_factor(oracle, "gauss", shape, F32)
    F64o, _ = oracle.factor(A.astype(F64), b)
    F, T = wave_factor(tqr, A, shape)
    Fg = F.astype(F64)
    dF = float(np.abs(Fg - F32o).max())
    dT = float(np.abs(T.astype(F64) - T32o).max())
    e_gpu, e_ref = float(np.abs(Fg - F64o).max()), float(np.abs(F32o - F64o).max())
    print(f"waves fp32 gauss {shape}: max|dF| {dF:.3e} (max|F| {np.abs(F32o).max():.3e}), max|dtau| {dT:.3e}, "
          f"vs fp64 oracle: GPU {e_gpu:.3e}, fp32 oracle {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}")
    assert dF <= 1e-4 * max(1.0, float(np.abs(F32o).max()))
    assert dT <= 2e-4
    assert e_gpu <= 1.5 * e_ref


@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_wave_zero_first_pivot(tqr, oracle, dt, zero):
    """sign(0) = +1 in the reference, for both zeros, over a live tail."""
    A = inputs.matrix("gauss", SMALL, dt).copy()
    A[0, 0] = zero
    assert np.signbit(A[0, 0]) == np.signbit(zero) and np.abs(A[0, 1:]).min() > 0
    F_ref, T_ref = oracle.factor(A, SMALL[2])
    # sign(0) = +1: GEQRT leaves R_00 = -norm, and each of the p - 1 = 3 TSQRTs below flips it again
    assert F_ref[0, 0] > 0
    F, T = wave_factor(tqr, A, SMALL)
    assert_close(F, T, F_ref, T_ref)


def test_wave_zero_tile_column(tqr, oracle):
    """Tile column 1 all zero: every reflector of step 1 has a zero column (tau = 2, v = e1, R = 0), in
    k_panel's GEQRT and in each TSQRT, and k_update applies them to tile column 2. Nothing is decided
    by rounding, so the elementwise comparison is well posed."""
    m, n, b = SMALL
    A = inputs.matrix("gauss", SMALL).copy()
    A[b:2 * b] = 0.0
    F_ref, T_ref = oracle.factor(A, b)
    assert np.all(T_ref[b, b:] == 2) and not F_ref[b:2 * b, b:].any()
    F, T = wave_factor(tqr, A, SMALL)
    assert_close(F, T, F_ref, T_ref)
    assert oracle.residual(A, F, T, b) <= 1e-13


def test_wave_structured(tqr, oracle):
    """matrix("structured"): unit columns, a zero column (tau == 2, a zero on R's diagonal) and column
    n/2 + 6 an exact copy of column 3. Below the diagonal that copy is rounding noise after step 0, so
    the sign and direction of its reflector are decided by the noise, in the oracle as much as here
    (test_gpu_factor.test_zero_row_sign_ambiguous): from that column on, V, tau and the rows of R below
    it are not unique. Well posed and asserted: elementwise parity of every column before the copy
    (column j of a Householder QR depends on columns <= j only), of their taus, and the residual of the
    whole factorisation with |R| of the leading columns."""
    m, n, b = SMALL
    A = inputs.matrix("structured", SMALL)
    F_ref, T_ref = inputs.oracle_factor(oracle, "structured", SMALL)
    F, T = wave_factor(tqr, A, SMALL)
    assert np.isfinite(F).all() and np.isfinite(T).all()
    assert oracle.residual(A, F, T, b) <= 1e-13
    c = n // 2 + 6  # the copied column
    k, c_in = divmod(c, b)
    Tm, Tm_ref = T.copy(), T_ref.copy()
    for X in (Tm, Tm_ref):  # taus of step k live in row k*b, column c_in of every tile row: drop c_in ..
        X[k * b].reshape(m // b, b)[:, c_in:] = 0
        X[(k + 1) * b:] = 0
    assert_close(F[:c], Tm, F_ref[:c], Tm_ref)
    assert (T[inputs.ZERO_COL // b * b].reshape(m // b, b)[:, inputs.ZERO_COL % b] == 2).all()
    R, R_ref = inputs.r_of(F)[:, :c], inputs.r_of(F_ref)[:, :c]
    assert np.abs(np.abs(R) - np.abs(R_ref)).max() <= 1e-11 * np.abs(R_ref).max()


# ---- B. where the matrix lies -------------------------------------------------------------------
PAD_CASES = [(s, dt, pad) for s, dt in DEV_CASES for pad in ((8, 1) if dt == F64 else (4, 3))]


def checked_base(tqr, oracle, shape, dt, engine="waves"):
    plan, F0, tau0 = base(tqr, engine, shape, dt)
    assert_close(*as_host(tqr, F0, tau0, shape), *inputs.oracle_factor(oracle, "gauss", shape, dt))
    return plan, F0, tau0


@pytest.mark.parametrize("shape,dt,pad", PAD_CASES,
                         ids=[f"{m}x{n}b{b}-{dtname(dt)}-ld+{p}" for (m, n, b), dt, p in PAD_CASES])
def test_wave_padded_ldda(tqr, oracle, shape, dt, pad):
    import torch
    m, n, b = shape
    plan, F0, tau0 = checked_base(tqr, oracle, shape, dt)
    ldda = m + pad
    buf = torch.full((n, ldda), SENTINEL, dtype=F0.dtype, device="cuda")
    buf[:, :m] = torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda()
    tau = torch.zeros_like(tau0, device="cuda")
    torch.cuda.synchronize()
    plan.execute(buf, tau, ldda=ldda)
    plan.status()
    out = buf.cpu()
    assert torch.all(out[:, m:] == SENTINEL), "the engine wrote into the padding rows m .. ldda-1"
    assert torch.equal(out[:, :m], F0) and torch.equal(tau.cpu(), tau0)


@pytest.mark.parametrize("shape,dt", DEV_CASES, ids=ids(DEV_CASES))
def test_wave_offset_base(tqr, oracle, shape, dt):
    """A starts one element into its allocation: 8-byte (fp64) / 4-byte (fp32) aligned base."""
    import torch
    m, n, b = shape
    plan, F0, tau0 = checked_base(tqr, oracle, shape, dt)
    big = torch.full((n * m + 2,), SENTINEL, dtype=F0.dtype, device="cuda")
    view = big[1:1 + n * m].view(n, m)
    view.copy_(torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda())
    assert view.data_ptr() == big.data_ptr() + big.element_size()
    tau = torch.zeros_like(tau0, device="cuda")
    torch.cuda.synchronize()
    plan.execute(view, tau)
    plan.status()
    out = big.cpu()
    assert out[0] == SENTINEL and out[-1] == SENTINEL
    assert torch.equal(out[1:-1].view(n, m), F0) and torch.equal(tau.cpu(), tau0)


@pytest.mark.parametrize("shape,dt", DEV_CASES, ids=ids(DEV_CASES))
def test_wave_stream_and_plan_reuse(tqr, oracle, shape, dt):
    """X, Y, X on one wave plan and one non-default stream, with no host synchronisation between the
    executes: the third result is the first bit for bit (and the default-stream one), the second is
    the oracle's factorisation of Y. The inputs are on the device before the first execute; the
    stream was made to wait for them."""
    import torch
    m, n, b = shape
    plan, F0, tau0 = checked_base(tqr, oracle, shape, dt)
    X = inputs.matrix("gauss", shape, dt)
    Y = inputs.matrix("gauss", shape, dt, offset=7)
    s = torch.cuda.Stream()
    bufs = [(torch.from_numpy(M.copy()).cuda(), torch.zeros_like(tau0, device="cuda")) for M in (X, Y, X)]
    s.wait_stream(torch.cuda.default_stream())
    for dA, tau in bufs:
        plan.execute(dA, tau, stream=s.cuda_stream)
    plan.status(stream=s.cuda_stream)
    (F1, t1), (F2, t2), (F3, t3) = [(a.cpu(), t.cpu()) for a, t in bufs]
    assert torch.equal(F3, F1) and torch.equal(t3, t1)
    assert torch.equal(F1, F0) and torch.equal(t1, tau0)
    FY, TY = inputs.oracle_factor(oracle, "gauss", shape, dt, offset=7)
    assert_close(*as_host(tqr, F2, t2, shape), FY, TY)


@pytest.mark.parametrize("shape,dt", DEV_CASES, ids=ids(DEV_CASES))
def test_wave_profile_same_bits(tqr, oracle, shape, dt):
    """tqr_plan_set_profile adds timing events between the launches (and a host synchronisation):
    the bits are those of the unprofiled run, on and off again."""
    import torch
    plan, F0, tau0 = checked_base(tqr, oracle, shape, dt)
    A = inputs.matrix("gauss", shape, dt)
    try:
        plan.set_profile(True)
        F1, t1 = execute(plan, A)
    finally:
        plan.set_profile(False)
    F2, t2 = execute(plan, A)
    assert torch.equal(F1, F0) and torch.equal(t1[:plan.kmax], tau0)
    assert torch.equal(F2, F0) and torch.equal(t2[:plan.kmax], tau0)


# ---- C. stream ordering -------------------------------------------------------------------------
SCRATCH_BYTES = 256 << 20


@pytest.mark.parametrize("null_stream", [False, True], ids=["stream", "null-stream"])
@pytest.mark.parametrize("engine", ENGINES)
def test_stream_ordered_input_and_result(tqr, oracle, engine, null_stream):
    """tqr_plan_execute is stream-ordered on both sides. Queued on one stream with no host
    synchronisation anywhere in between: a 256 MiB device copy that fills a scratch buffer whose last
    elements are the input, a copy of the input out of the scratch into dA (which held NaN), the
    execute, and clones of dA and tau. The clones must hold the host-synchronised run's bits. The wave
    engine works on two non-blocking side streams, which order themselves against nothing implicitly —
    not against the NULL stream either — so its evStart record / wait and its final joins are all that
    orders them against the fill before and the clones behind; a missing one reads the NaN or clones an
    unfinished matrix. (This cannot prove the ordering; it makes a missing join likely to show. It runs
    once.) The flow engine launches on the caller's stream itself: the same contract, trivially."""
    import torch
    shape, dt = (768, 768, 256), F64
    m, n, b = shape
    plan, F0, tau0 = checked_base(tqr, oracle, shape, dt, engine)
    nel = SCRATCH_BYTES // 8
    src = torch.zeros((nel,), dtype=torch.float64, device="cuda")
    src[nel - n * m:] = torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda().reshape(-1)
    scratch = torch.full((nel,), float("nan"), dtype=torch.float64, device="cuda")
    dA = torch.full((n, m), float("nan"), dtype=torch.float64, device="cuda")
    tau = torch.zeros_like(tau0, device="cuda")
    s = torch.cuda.default_stream() if null_stream else torch.cuda.Stream()
    if null_stream:
        assert s.cuda_stream == 0
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        scratch.copy_(src)
        dA.copy_(scratch[nel - n * m:].view(n, m))
        plan.execute(dA, tau, stream=s.cuda_stream)
        F, t = dA.clone(), tau.clone()
    s.synchronize()
    plan.status(stream=s.cuda_stream)
    assert torch.equal(F.cpu(), F0) and torch.equal(t.cpu(), tau0)


# ---- D. one plan shared by threads and streams --------------------------------------------------
@pytest.mark.parametrize("shape,dt", SHARE_CASES, ids=ids(SHARE_CASES))
@pytest.mark.parametrize("engine", ENGINES)
def test_plan_shared_by_two_threads(tqr, oracle, engine, shape, dt):
    """a plan may be shared by threads and streams; tqr.h: executes of one plan are
    mutually excluded while they enqueue and never overlap on the GPU. Two host threads, each with its
    own stream and its own buffers, run X, Y, X and Y, X, Y on one plan with no synchronisation of
    their own between executes. The plan's panel workspace (both engines), counters (flow) and side
    streams and events (waves) are shared, the callers order nothing between the two streams: every
    result equals the single-threaded result of its input bit for bit only if the plan serialises the
    executes as documented. Runs once; the threads are joined with a timeout."""
    import torch
    plan, FX, tX = checked_base(tqr, oracle, shape, dt, engine)
    _, FY, tY = base(tqr, engine, shape, dt, offset=7)
    want = {"X": (FX, tX), "Y": (FY, tY)}
    mats = {"X": inputs.matrix("gauss", shape, dt), "Y": inputs.matrix("gauss", shape, dt, offset=7)}
    seqs = ["XYX", "YXY"]
    streams = [torch.cuda.Stream() for _ in seqs]
    bufs = [[(torch.from_numpy(mats[c].copy()).cuda(), torch.zeros_like(tX, device="cuda")) for c in seq] for seq in seqs]
    torch.cuda.synchronize()
    errors = [None, None]
    start = threading.Barrier(2, timeout=30)

    def work(i):
        try:
            start.wait()
            for dA, tau in bufs[i]:
                plan.execute(dA, tau, stream=streams[i].cuda_stream)
            plan.status(stream=streams[i].cuda_stream)
        except BaseException as e:  # reported by the main thread
            errors[i] = e

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "a thread did not finish its three executes in 60 s"
    assert errors == [None, None], errors
    torch.cuda.synchronize()
    for seq, bb in zip(seqs, bufs):
        for c, (dA, tau) in zip(seq, bb):
            assert torch.equal(dA.cpu(), want[c][0]) and torch.equal(tau.cpu(), want[c][1]), (seq, c)


@pytest.mark.parametrize("shape,dt", SHARE_CASES, ids=ids(SHARE_CASES))
@pytest.mark.parametrize("engine", ENGINES)
def test_plan_on_two_alternating_streams(tqr, oracle, engine, shape, dt):
    """One thread, one dA / tau pair, executes alternating between two streams (a, b, a, b on X, Y, X,
    Y), no host synchronisation. Execute i runs on stream s_i; behind it, on the same s_i, the result
    is cloned and dA and tau are re-filled for execute i+1, which runs on the OTHER stream.
    The caller provides exactly one ordering per hand-over: an event recorded on s_i behind the re-fill,
    which s_(i+1) waits for before its execute — the data dependency any device buffer needs. Clone and
    re-fill are ordered behind execute i by s_i itself, because tqr_plan_execute is stream-ordered
    (the wave engine's final joins).
    The plan provides what tqr.h promises: each execute's stream first waits for the plan's previous
    execute, whatever its stream. With one shared dA the caller's event already implies that order, so
    this test does not observe the promise on its own (test_plan_shared_by_two_threads does: there the
    callers order nothing); it shows that the plan's cross-stream wait, the wave engine's side-stream
    events re-recorded from alternating caller streams, and the caller's events compose: no deadlock,
    and every result has the single-stream bits."""
    import torch
    plan, FX, tX = checked_base(tqr, oracle, shape, dt, engine)
    _, FY, tY = base(tqr, engine, shape, dt, offset=7)
    want = [(FX, tX), (FY, tY)] * 2
    srcs = [torch.from_numpy(inputs.matrix("gauss", shape, dt, offset=o).copy()).cuda() for o in (0, 7)] * 2
    dA = srcs[0].clone()
    tau = torch.zeros_like(tX, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for i in range(4):
        s = streams[i % 2]
        with torch.cuda.stream(s):
            plan.execute(dA, tau, stream=s.cuda_stream)
            outs.append((dA.clone(), tau.clone()))
            if i < 3:
                dA.copy_(srcs[i + 1])
                tau.zero_()
                ev = s.record_event()
        if i < 3:
            streams[(i + 1) % 2].wait_event(ev)
    for s in streams:
        plan.status(stream=s.cuda_stream)
    for i, (F, t) in enumerate(outs):
        assert torch.equal(F.cpu(), want[i][0]) and torch.equal(t.cpu(), want[i][1]), f"execute {i}"


# ---- E. host-pointer API on the wave engine ------------------------------------------------------
HOST_CASES = [((256, 192, 64), F64, 1, True), ((768, 768, 256), F32, 3, True), ((128, 256, 64), F64, 0, True),
              ((64, 64, 16), F32, 4, False)]


@pytest.mark.parametrize("shape,dt,pad,with_tau", HOST_CASES,
                         ids=[f"{sid(s)}-{dtname(dt)}-ld+{p}{'' if wt else '-notau'}" for s, dt, p, wt in HOST_CASES])
def test_wave_host_api(tqr, oracle, shape, dt, pad, with_tau):
    """tqr_geqrt_host_engine(TQR_ENGINE_WAVES): staged copies through the plan's pinned buffers around
    the same launches. Against the oracle; rows m .. ldm-1 of A (sentinel) and of tau (zero) untouched,
    as test_gpu_xfer.test_host_xfer_vs_oracle checks for the flow path; the bits of the device path."""
    m, n, b = shape
    A = inputs.matrix("gauss", shape, dt)
    F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, dt)
    S = np.full((n, m + pad), 7.25, dtype=dt)
    S[:, :m] = A
    T = tqr.geqrt_host(S, b, with_tau=with_tau, m=m, engine="waves")
    assert np.all(S[:, m:] == 7.25)
    _, F0, tau0 = base(tqr, "waves", shape, dt)
    F0, T0 = as_host(tqr, F0, tau0, shape)
    assert np.array_equal(inputs.bits(S[:, :m]), inputs.bits(F0))
    if with_tau:
        assert T.shape == S.shape and np.all(T[:, m:] == 0)
        assert_close(S[:, :m], T[:, :m], F_ref, T_ref)
        assert np.array_equal(inputs.bits(T[:, :m]), inputs.bits(T0))
    else:
        assert T is None
        assert_close(S[:, :m], T_ref, F_ref, T_ref)  # (F alone)


def test_cudaQRFull_is_the_wave_engine_at_b32(tqr, oracle):
    """gpucalc.h's cudaQRFull (fp32, ldm = m, tau discarded) is tqr_geqrt_host_engine on the wave engine
    with 32 x 32 tiles (csrc/legacy.cpp): the same bits."""
    shape = (256, 192, 32)
    m, n, b = shape
    A = inputs.matrix("gauss", shape, F32)
    F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, F32)
    G = A.copy()
    tqr.lib().cudaQRFull(G.ctypes.data_as(ctypes.c_void_p), m, n)
    assert_close(G, T_ref, F_ref, T_ref)
    F = A.copy()
    assert tqr.geqrt_host(F, b, with_tau=False, engine="waves") is None
    assert np.array_equal(inputs.bits(G), inputs.bits(F))


# ---- F. the cached one-shot device helpers ---------------------------------------------------------
TILED_CASES = [((256, 192, 64), F64), ((768, 768, 256), F32)]


@pytest.fixture
def clean_cache(tqr):
    tqr.cache_clear()
    yield
    tqr.cache_clear()


def tiled(tqr, shape, dt, pad=0, stream=None):
    """geqrt_tiled on the gauss matrix: (F, tau) as CPU tensors (rows beyond m checked for the sentinel)."""
    import torch
    m, n, b = shape
    buf = torch.full((n, m + pad), SENTINEL, dtype=tdt(dt), device="cuda")
    buf[:, :m] = torch.from_numpy(inputs.matrix("gauss", shape, dt).copy()).cuda()
    tau = torch.zeros((min(m, n) // b, m), dtype=tdt(dt), device="cuda")
    torch.cuda.synchronize()
    if stream is not None:
        stream.wait_stream(torch.cuda.default_stream())
    tqr.geqrt_tiled(buf, tau, b, m=m, ldda=m + pad, stream=stream)
    (stream or torch.cuda.default_stream()).synchronize()
    torch.cuda.synchronize()
    out = buf.cpu()
    assert torch.all(out[:, m:] == SENTINEL)
    return out[:, :m], tau.cpu()


@pytest.mark.parametrize("shape,dt", TILED_CASES, ids=ids(TILED_CASES))
def test_geqrt_tiled(tqr, oracle, clean_cache, monkeypatch, shape, dt):
    """tqr_dgeqrt_tiled / tqr_sgeqrt_tiled: the bits of a TiledQR run, on the first call (which builds
    the cached plan), on the second (which finds it) and with a padded ldda on a non-default stream."""
    import torch
    monkeypatch.delenv("TQR_ENGINE", raising=False)
    _, F0, tau0 = checked_base(tqr, oracle, shape, dt, "flow")
    for kw in ({}, {}, {"pad": 8 if dt == F64 else 3, "stream": torch.cuda.Stream()}):
        F, tau = tiled(tqr, shape, dt, **kw)
        assert torch.equal(F, F0) and torch.equal(tau, tau0), kw


def test_geqrt_tiled_follows_TQR_ENGINE(tqr, oracle, clean_cache, monkeypatch):
    """The cached plan is made by tqr_plan_create_engine(TQR_ENGINE_DEFAULT), which reads TQR_ENGINE when
    the plan is created: after a cache_clear the helper runs the wave engine under TQR_ENGINE=waves, and
    the flow engine again once the variable is gone and the cache was cleared."""
    import torch
    shape, dt = SMALL, F64
    _, Fw, tw = checked_base(tqr, oracle, shape, dt, "waves")
    _, Ff, tf = checked_base(tqr, oracle, shape, dt, "flow")
    monkeypatch.setenv("TQR_ENGINE", "waves")
    F, tau = tiled(tqr, shape, dt)
    assert torch.equal(F, Fw) and torch.equal(tau, tw)
    monkeypatch.delenv("TQR_ENGINE")
    tqr.cache_clear()
    F, tau = tiled(tqr, shape, dt)
    assert torch.equal(F, Ff) and torch.equal(tau, tf)


def test_geqrt_tiled_argument_errors(tqr, clean_cache):
    import torch
    L = tqr.lib()
    m, n, b = SMALL
    for fn, tt in ((L.tqr_dgeqrt_tiled, torch.float64), (L.tqr_sgeqrt_tiled, torch.float32)):
        dA = torch.full((n, m), SENTINEL, dtype=tt, device="cuda")
        tau = torch.zeros((n // b, m), dtype=tt, device="cuda")
        pa, pt = dA.data_ptr(), tau.data_ptr()
        assert fn(m - 8, n, b, pa, m, pt, None) == TQR_EINVAL      # b does not divide m
        assert fn(m, n - 8, b, pa, m, pt, None) == TQR_EINVAL      # ... nor n
        assert fn(m, n, 48, pa, m, pt, None) == TQR_EINVAL         # not a tile size
        assert fn(m, n, b, pa, m - 1, pt, None) == TQR_EINVAL      # ldda < m
        assert fn(m, n, b, None, m, pt, None) == TQR_EINVAL
        assert fn(m, n, b, pa, m, None, None) == TQR_EINVAL
        torch.cuda.synchronize()
        assert torch.all(dA == SENTINEL) and not tau.any()


# ---- G. profile counters, and what a wave plan refuses -------------------------------------------
def test_wave_profile_stats(tqr):
    """With tqr_plan_set_profile the wave engine reports one panel launch per wave that holds a GEQRT /
    TSQRT task and one update launch per wave that holds an UNMQR / TSMQR task (tqr.sched_plan is the
    plan it replays), with finite positive times; switched off, a further execute leaves them alone."""
    shape = SMALL
    m, n, b = shape
    plan = tqr.TiledQR(m, n, b, tdt(F64), engine="waves")
    waves = tqr.sched_plan(m // b, n // b)
    n_panel = sum(1 for w in waves if np.isin(w[:, 0], (tqr.QRS, tqr.QRD)).any())
    n_update = sum(1 for w in waves if np.isin(w[:, 0], (tqr.SAPP, tqr.DAPP)).any())
    assert 0 < n_panel <= len(waves) and 0 < n_update <= len(waves)
    A = inputs.matrix("gauss", shape)
    assert plan.stats() == {"n_update": 0, "ms_update": 0.0, "n_panel": 0, "ms_panel": 0.0}
    execute(plan, A)
    assert plan.stats()["n_panel"] == 0  # not profiled: nothing recorded
    plan.set_profile(True)
    execute(plan, A)
    st = plan.stats()
    print(f"wave profile {shape}: {st}; waves {len(waves)}")
    assert st["n_panel"] == n_panel and st["n_update"] == n_update
    assert np.isfinite(st["ms_panel"]) and st["ms_panel"] > 0
    assert np.isfinite(st["ms_update"]) and st["ms_update"] > 0
    plan.set_profile(False)
    execute(plan, A)
    assert plan.stats() == st


def test_flow_profile_stats(tqr):
    """The flow engine is one launch, reported as the update kernel's."""
    import torch
    shape = SMALL
    m, n, b = shape
    plan = tqr.TiledQR(m, n, b, tdt(F64), engine="flow")
    A = inputs.matrix("gauss", shape)
    plan.set_profile(True)
    F1, t1 = execute(plan, A)
    st = plan.stats()
    assert st["n_update"] == 1 and st["n_panel"] == 0 and st["ms_panel"] == 0
    assert np.isfinite(st["ms_update"]) and st["ms_update"] > 0
    plan.set_profile(False)
    F2, t2 = execute(plan, A)
    assert plan.stats() == st
    assert torch.equal(F1, F2) and torch.equal(t1, t2)  # the profile switch does not change the bits


def test_wave_plan_refusals(tqr):
    """The flow engine's task-list and workspace calls return TQR_EINVAL on a wave plan, before and after
    an execute; tqr_plan_status has nothing to report on it and returns TQR_OK."""
    m, n, b = SMALL
    L = tqr.lib()
    plan = tqr.TiledQR(m, n, b, tdt(F64), engine="waves")
    info = tqr.plan_info(plan)
    assert info["engine"] == 0 and info["ntasks"] > 0
    items = (ctypes.c_int * (4 * info["ntasks"]))()
    host = (ctypes.c_char * 4096)()
    for _ in range(2):
        assert L.tqr_plan_set_tasks(plan.h, items, info["ntasks"]) == TQR_EINVAL
        assert L.tqr_plan_debug_workspace(plan.h, 0, host, ctypes.c_size_t(4096)) == TQR_EINVAL
        assert L.tqr_plan_status(plan.h, None) == 0
        execute(plan, inputs.matrix("gauss", SMALL))
    with pytest.raises(tqr.TQRError):
        tqr.TiledQR(m, n, b, tdt(F64), steps=2, engine="waves")


# ---- H. the wave factorisation feeds the rest of the library --------------------------------------
def test_wave_factors_under_apply_and_lstsq(tqr, oracle):
    """tqr_apply_prepare / tqr_apply_q read V and tau as a factorisation leaves them: on the wave
    engine's, Q^T A is R on and above the diagonal and zero below (test_gpu_apply's bound), and least
    squares agrees with the one on the flow engine's factors at assert_close's scale."""
    import torch
    shape = SMALL
    m, n, b = shape
    A = inputs.matrix("gauss", shape)
    _, Fw, tw = checked_base(tqr, oracle, shape, F64, "waves")
    _, Ff, tf = checked_base(tqr, oracle, shape, F64, "flow")
    dF, dt_ = Fw.cuda(), tw.cuda()
    ap = tqr.ApplyQ(m, n, b, torch.float64)
    C = torch.from_numpy(A.copy()).cuda()
    cs = torch.cuda.current_stream()
    ap.prepare(dF, dt_, stream=cs)
    ap.apply(dF, C, trans=True, stream=cs)
    torch.cuda.synchronize()
    got, F = C.cpu().numpy(), Fw.numpy()
    up = np.arange(m)[None, :] <= np.arange(n)[:, None]
    R = np.where(up, F, 0.0)
    e_up, e_lo = float(np.abs(got - R)[up].max()), float(np.abs(got)[~up].max())
    print(f"waves: max|triu(Q^T A) - R| = {e_up:.3e}, max|below the diagonal| = {e_lo:.3e}")
    assert e_up <= 1e-11 * max(1.0, float(np.abs(R).max()))
    assert e_lo <= 1e-11 * float(np.abs(A).max())
    B = inputs.lsq_rhs("gauss", shape)
    sols = []
    for F_, t_ in ((Fw, tw), (Ff, tf)):
        X, res = tqr.lstsq(F_.cuda(), t_.cuda(), torch.from_numpy(B.copy()).cuda(), b)
        torch.cuda.synchronize()
        sols.append((X.cpu().numpy(), res.cpu().numpy()))
    (Xw, rw), (Xf, rf) = sols
    assert np.isfinite(Xw).all() and np.isfinite(rw).all()
    assert float(np.abs(Xw - Xf).max()) <= 1e-11 * max(1.0, float(np.abs(Xf).max()))
    assert float(np.abs(rw - rf).max()) <= 1e-11 * max(1.0, float(np.abs(rf).max()))


# ---- I. the engines against each other -----------------------------------------------------------
@pytest.mark.parametrize("shape,dt", WAVE_CASES, ids=ids(WAVE_CASES))
def test_engines_against_each_other(tqr, oracle, shape, dt):
    """The two engines run the same tile operations over the same DAG, but not the same kernels: the
    flow engine's panels and chains use other reflector-group sizes and summation orders than k_panel /
    k_update (and fp32 MFMA chains for fp32 storage). Measured on an MI355X on gauss, the entries of
    (F, tau) whose bits differ between engine="waves" and engine="flow" (of all entries of F; of all
    kmax * m compact tau entries, those above row k*b included):

        shape           fp64: F, tau                      fp32: F, tau
        64x64   b16     3534 / 4096,       96 / 256       2853 / 4096,       56 / 256
        128x128 b32     14814 / 16384,    227 / 512       11584 / 16384,    121 / 512
        256x192 b64     44827 / 49152,    371 / 768       38878 / 49152,    196 / 768
        512x384 b128    183172 / 196608,  765 / 1536      171442 / 196608,  446 / 1536
        768x768 b256    558762 / 589824, 1010 / 2304      545353 / 589824,  730 / 2304
        128x256 b64     29594 / 32768,    117 / 256       27136 / 32768,     74 / 256

    with max|dF| at most 7.3e-14 (fp64) and 6.4e-5 (fp32). So equality of bits across the engines is
    not a property of the library and is not asserted (include/tqr.h says what is: each engine alone is
    bit-reproducible). Both are tied to the oracle by assert_close (here, through checked_base), hence
    to each other within twice that bound; the counts are printed."""
    _, Fw, tw = checked_base(tqr, oracle, shape, dt, "waves")
    _, Ff, tf = checked_base(tqr, oracle, shape, dt, "flow")
    nF = int((inputs.bits(Fw.numpy()) != inputs.bits(Ff.numpy())).sum())
    nt = int((inputs.bits(tw.numpy()) != inputs.bits(tf.numpy())).sum())
    dF = float(np.abs(Fw.numpy().astype(F64) - Ff.numpy().astype(F64)).max())
    dT = float(np.abs(tw.numpy().astype(F64) - tf.numpy().astype(F64)).max())
    print(f"engines {sid(shape)} {dtname(dt)}: differing entries F {nF} of {Fw.numel()}, tau {nt} of {tw.numel()}, "
          f"max|dF| {dF:.3e}, max|dtau| {dT:.3e}")
    F_ref, _ = inputs.oracle_factor(oracle, "gauss", shape, dt)
    if dt == F64:
        assert dF <= 2 * 1e-11 * max(1.0, float(np.abs(F_ref).max())) and dT <= 2 * 1e-11 * 2
    else:
        assert dF <= 2 * 1e-3 and dT <= 2 * 1e-3
