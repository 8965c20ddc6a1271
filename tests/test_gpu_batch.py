"""The strided-batched factorisation (include/tqr.h "batched", csrc/batch.hip) on the device.

The contract is one of bytes: matrix i of a batch has the bytes of a TQR_ENGINE_WAVES plan executed on
that matrix alone, and nothing outside the matrices is written. So almost every check here compares
whole allocations, NaN-filled gaps included, with the same allocations after a wave plan was run on
each member in turn — no tolerance. One case goes against the oracle with the project's fp64 bound
(test_gpu_factor.assert_close: 1e-11 scaled), so the batch does not rest on the wave engine alone, and
one runs tqr.form_q on a member through an offset base pointer with test_gpu_form_q.test_meaning's
bounds (1e-11, and 1e-11 * max(1, max|A|)).

A. byte equality with the wave engine, all tile sizes, both dtypes, gaps and padding NaN;
B. accuracy against the oracle;
C. grouping: a forced group of 2 out of 5, and batch 1;
D. strides: padded ldda, odd strides, offset bases; the row-interleaved form;
E. ordering: input written on a side stream, 10 executes on alternating streams, two host threads;
F. composition with form_q;
G. refusals with live device buffers.
"""
import ctypes
import threading

import numpy as np
import pytest

import inputs
from inputs import dtname
from test_gpu_factor import assert_close

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
TQR_EINVAL = -1
P = ctypes.c_void_p
# (m, n, b): every tile size; one tile, tall, wide, several steps; b = 128 runs two update strips per tile
SHAPES = [(32, 32, 16), (48, 32, 16), (32, 48, 16), (64, 64, 32), (128, 128, 64), (256, 128, 128), (512, 256, 256)]
CASES = [(s, dt) for s in SHAPES for dt in (F64, F32)]
SMALL = (96, 64, 32)


def ids(cases):
    return [f"{m}x{n}b{b}-{dtname(dt)}" for (m, n, b), dt in cases]


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


_wave = {}


def wave_plan(tqr, shape, dt):
    key = (shape, dtname(dt))
    if key not in _wave:
        m, n, b = shape
        _wave[key] = tqr.TiledQR(m, n, b, tdt(dt), engine="waves")
        assert tqr.plan_info(_wave[key])["engine"] == 0
    return _wave[key]


class Layout:
    """`batch` matrices of `shape` inside one flat NaN-filled device buffer, and their compact taus inside
    another: matrix i at element base + i * strideA with leading dimension ldda, tau i at tbase +
    i * strideTau. Both buffers end in 7 guard elements."""

    def __init__(self, shape, dt, batch, ldda=None, strideA=None, strideTau=None, base=0, tbase=0):
        import torch
        m, n, b = shape
        self.shape, self.dt, self.batch = shape, dt, batch
        self.kmax = min(m, n) // b
        self.ldda = ldda or m
        self.sA = self.n_ld() if strideA is None else strideA
        self.sT = self.kmax * m if strideTau is None else strideTau
        self.base, self.tbase = base, tbase
        self.A = torch.full((base + (batch - 1) * self.sA + (n - 1) * self.ldda + m + 7,), float("nan"),
                            dtype=tdt(dt), device="cuda")
        self.tau = torch.full((tbase + (batch - 1) * self.sT + self.kmax * m + 7,), float("nan"), dtype=tdt(dt),
                              device="cuda")

    def n_ld(self):
        return self.shape[1] * self.ldda

    def mats(self, A=None):
        """(batch, n, m) strided view of the matrices (of self.A, or of a clone of it)."""
        import torch
        m, n, _ = self.shape
        return torch.as_strided(self.A if A is None else A, (self.batch, n, m), (self.sA, self.ldda, 1), self.base)

    def taus(self, tau=None):
        import torch
        m = self.shape[0]
        return torch.as_strided(self.tau if tau is None else tau, (self.batch, self.kmax, m), (self.sT, m, 1), self.tbase)

    def fill(self, offset0=0):
        """Distinct Gaussian matrices (inputs.matrix offsets offset0 ..); the taus' written part is left
        NaN: the engine overwrites it."""
        import torch
        v = self.mats()
        for i in range(self.batch):
            v[i] = torch.from_numpy(inputs.matrix("gauss", self.shape, self.dt, offset0 + i).copy()).cuda()
        torch.cuda.synchronize()
        return self

    def wave_reference(self, tqr):
        """Clones of both buffers after the wave plan ran on each member in turn, on the host."""
        import torch
        A, tau = self.A.clone(), self.tau.clone()
        plan = wave_plan(tqr, self.shape, self.dt)
        torch.cuda.synchronize()
        for i in range(self.batch):
            plan.execute(A[self.base + i * self.sA:], tau[self.tbase + i * self.sT:], ldda=self.ldda)
        plan.status()
        torch.cuda.synchronize()
        return A.cpu().numpy(), tau.cpu().numpy()

    def execute(self, bq, stream=None):
        bq.execute(self.A[self.base:], self.tau[self.tbase:], ldda=self.ldda, strideA=self.sA, strideTau=self.sT,
                   stream=stream)

    def host(self):
        import torch
        torch.cuda.synchronize()
        return self.A.cpu().numpy(), self.tau.cpu().numpy()


def same_bytes(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def assert_same(got, ref, what=""):
    assert same_bytes(got[0], ref[0]), f"{what}: the matrix buffers differ in bytes"
    assert same_bytes(got[1], ref[1]), f"{what}: the tau buffers differ in bytes"


def check_written(lay, A, tau):
    """Every matrix element is finite, everything else in the A buffer is still NaN; of the taus, row k
    is finite from element k*b on and NaN before it, and everything outside the taus is NaN."""
    import torch
    m, n, b = lay.shape
    tA, tT = torch.from_numpy(A.copy()), torch.from_numpy(tau.copy())
    vA, vT = lay.mats(tA), lay.taus(tT)
    assert torch.isfinite(vA).all()
    for k in range(lay.kmax):
        assert torch.isfinite(vT[:, k, k * b:]).all() and torch.isnan(vT[:, k, :k * b]).all()
    vA.fill_(float("nan"))
    vT.fill_(float("nan"))
    assert torch.isnan(tA).all(), "an element outside the matrices was written"
    assert torch.isnan(tT).all(), "an element outside the compact taus was written"


# ---- A. byte equality with the wave engine -------------------------------------------------------
@pytest.mark.parametrize("shape,dt", CASES, ids=ids(CASES))
def test_bytes_equal_wave_engine(tqr, shape, dt):
    """Batch 3, padded ldda, gaps between the matrices and between the taus, all NaN: both whole
    allocations equal those after the wave plan ran on each matrix in turn."""
    m, n, b = shape
    kmax = min(m, n) // b
    lay = Layout(shape, dt, 3, ldda=m + 3, strideA=n * (m + 3) + 5, strideTau=kmax * m + 2).fill()
    ref = lay.wave_reference(tqr)
    bq = tqr.BatchedQR(m, n, b, tdt(dt), 3)
    assert bq.group() == 3
    lay.execute(bq)
    got = lay.host()
    assert_same(got, ref, f"{shape} {dtname(dt)}")
    check_written(lay, *got)


# ---- B. accuracy, independent of the wave engine -------------------------------------------------
def test_accuracy_vs_oracle(tqr, oracle):
    """64 x 64, b = 32, fp64, batch 2, contiguous tensors and default strides: each member against the
    oracle's factorisation of it, fp64 bound of test_gpu_factor.assert_close (1e-11 scaled)."""
    import torch
    shape = (64, 64, 32)
    m, n, b = shape
    src = [inputs.matrix("gauss", shape, F64, i) for i in range(2)]
    A = torch.from_numpy(np.stack(src)).cuda()
    tau = torch.zeros((2, n // b, m), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tqr.BatchedQR(m, n, b, torch.float64, 2).execute(A, tau)
    torch.cuda.synchronize()
    for i in range(2):
        F_ref, T_ref = inputs.oracle_factor(oracle, "gauss", shape, F64, i)
        F, T = A[i].cpu().numpy(), tqr.expand_tau(tau[i].cpu().numpy(), m, n, b)
        err = float(np.abs(F - F_ref).max())
        print(f"member {i}: max|F - oracle| = {err:.3e} (max|F| {np.abs(F_ref).max():.3e}), "
              f"max|tau - oracle| = {np.abs(T - T_ref).max():.3e}")
        assert_close(F, T, F_ref, T_ref)
        assert oracle.residual(src[i], F, T, b) <= 1e-13


# ---- C. grouping ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_forced_groups(tqr, dt):
    """Batch 5 with a ws_limit worth two matrices runs as 2 + 2 + 1: the bytes of the one-group run (and of
    the wave engine), from a third of the workspace."""
    m, n, b = SMALL
    one = tqr.BatchedQR(m, n, b, tdt(dt), 5)
    assert one.group() == 5
    per = one.workspace_bytes() // 5
    two = tqr.BatchedQR(m, n, b, tdt(dt), 5, ws_limit=2 * per + per // 2)
    assert (two.group(), two.workspace_bytes()) == (2, 2 * per)
    assert tqr.batch_plan(m, n, b, tdt(dt), 5, 2 * per + per // 2)[:2] == (2, 3)
    a, c = Layout(SMALL, dt, 5, ldda=m + 1).fill(), Layout(SMALL, dt, 5, ldda=m + 1).fill()
    ref = a.wave_reference(tqr)
    a.execute(one)
    c.execute(two)
    got = c.host()
    assert_same(a.host(), ref, "one group")
    assert_same(got, ref, "groups of 2")
    check_written(c, *got)


@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_batch_one(tqr, dt):
    """Batch 1 is the single wave plan; strideA is ignored."""
    m, n, b = SMALL
    lay = Layout(SMALL, dt, 1).fill(7)
    ref = lay.wave_reference(tqr)
    bq = tqr.BatchedQR(m, n, b, tdt(dt), 1)
    bq.execute(lay.A, lay.tau, ldda=m, strideA=-3)
    assert_same(lay.host(), ref)
    with pytest.raises(tqr.TQRError):
        bq.execute(lay.A, lay.tau)  # a flat buffer has no ldda to default to


def test_geqrt_batched(tqr):
    """The one-shot helper on contiguous tensors: the bytes of the handle's execute."""
    import torch
    m, n, b = SMALL
    lay = Layout(SMALL, F64, 4).fill()
    ref = lay.wave_reference(tqr)
    A, tau = lay.mats().contiguous(), lay.taus().contiguous()
    tqr.geqrt_batched(A, tau, b)
    torch.cuda.synchronize()
    rA, rT = torch.from_numpy(ref[0]), torch.from_numpy(ref[1])
    assert same_bytes(A.cpu().numpy(), lay.mats(rA).contiguous().numpy())
    assert same_bytes(tau.cpu().numpy(), lay.taus(rT).contiguous().numpy())
    with pytest.raises(tqr.TQRError):
        tqr.geqrt_batched(A, tau[:, :1], b)


# ---- D. strides ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_odd_strides_offset_base(tqr, dt):
    """Padded ldda, an odd strideA and an odd strideTau beyond their minima, both bases offset by an odd
    number of elements."""
    m, n, b = SMALL
    lay = Layout(SMALL, dt, 3, ldda=m + 5, strideA=n * (m + 5) + 11, strideTau=(n // b) * m + 13, base=3, tbase=5).fill()
    assert lay.sA % 2 == 1 and lay.sT % 2 == 1
    ref = lay.wave_reference(tqr)
    lay.execute(tqr.BatchedQR(m, n, b, tdt(dt), 3))
    got = lay.host()
    assert_same(got, ref)
    check_written(lay, *got)


@pytest.mark.parametrize("dt", [F64, F32], ids=dtname)
def test_row_interleaved(tqr, dt):
    """4 row domains of 32 rows of one 128-row array, n = 32, b = 16, ldda = 128, strideA = 32: each domain
    equals the wave plan run on a packed copy of that domain, and its tau likewise."""
    import torch
    shape = (32, 32, 16)
    m, n, b = shape
    tall = torch.from_numpy(inputs.matrix("gauss", (128, 32, 16), dt).copy()).cuda()  # (n, 128)
    tau = torch.full((4, n // b, m), float("nan"), dtype=tdt(dt), device="cuda")
    plan = wave_plan(tqr, shape, dt)
    refs = []
    torch.cuda.synchronize()
    for i in range(4):
        D = tall[:, i * m:(i + 1) * m].contiguous()
        t = torch.full((n // b, m), float("nan"), dtype=tdt(dt), device="cuda")
        plan.execute(D, t)
        refs.append((D, t))
    plan.status()
    torch.cuda.synchronize()
    tqr.BatchedQR(m, n, b, tdt(dt), 4).execute(tall, tau, ldda=128, strideA=m)
    torch.cuda.synchronize()
    for i, (D, t) in enumerate(refs):
        assert same_bytes(tall[:, i * m:(i + 1) * m].contiguous().cpu().numpy(), D.cpu().numpy()), f"domain {i}"
        assert same_bytes(tau[i].cpu().numpy(), t.cpu().numpy()), f"tau of domain {i}"


# ---- E. ordering ---------------------------------------------------------------------------------
def test_input_written_on_side_stream(tqr):
    """The matrices are copied into place on a side stream and the execute follows on that stream with no
    host synchronisation in between."""
    import torch
    m, n, b = SMALL
    src = Layout(SMALL, F64, 3, ldda=m + 1).fill()
    ref = src.wave_reference(tqr)
    dst = Layout(SMALL, F64, 3, ldda=m + 1)
    bq = tqr.BatchedQR(m, n, b, torch.float64, 3)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dst.A.copy_(src.A, non_blocking=True)
        dst.execute(bq, stream=s)
    assert_same(dst.host(), ref)


def test_ten_executes_alternating_streams(tqr):
    """10 executes on one handle, back to back on two alternating streams, each on its own buffers: the
    handle's one workspace serialises them, so every result is the wave engine's."""
    import torch
    m, n, b = SMALL
    lays = [Layout(SMALL, F64, 3).fill(x % 4) for x in range(10)]
    refs = [lays[x].wave_reference(tqr) for x in range(4)]
    bq = tqr.BatchedQR(m, n, b, torch.float64, 3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for x, lay in enumerate(lays):
        lay.execute(bq, stream=streams[x % 2])
    for x, lay in enumerate(lays):
        assert_same(lay.host(), refs[x % 4], f"execute {x}")


def test_two_threads_share_one_handle(tqr):
    """Two host threads, each with its own stream and buffers, 4 executes each on one handle."""
    import torch
    m, n, b = SMALL
    lays = [[Layout(SMALL, F64, 3).fill(t) for _ in range(4)] for t in range(2)]
    refs = [lays[t][0].wave_reference(tqr) for t in range(2)]
    bq = tqr.BatchedQR(m, n, b, torch.float64, 3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    errors = []
    torch.cuda.synchronize()

    def work(t):
        try:
            for lay in lays[t]:
                lay.execute(bq, stream=streams[t])
            streams[t].synchronize()
        except Exception as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for x, lay in enumerate(lays[t]):
            assert_same(lay.host(), refs[t], f"thread {t}, execute {x}")


# ---- F. composition ------------------------------------------------------------------------------
def test_form_q_on_a_member(tqr):
    """Matrix 1 of a batch of 3 (128 x 64, b = 32, fp64) through an offset base pointer: tqr.form_q gives
    |Q^T Q - I| <= 1e-11 and |Q R - A| <= 1e-11 * max(1, max|A|) (test_gpu_form_q.test_meaning's bounds)."""
    import torch
    shape = (128, 64, 32)
    m, n, b = shape
    src = np.stack([inputs.matrix("gauss", shape, F64, i) for i in range(3)])
    A = torch.from_numpy(src).cuda()
    tau = torch.zeros((3, n // b, m), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tqr.BatchedQR(m, n, b, torch.float64, 3).execute(A, tau)
    torch.cuda.synchronize()
    Q = tqr.form_q(A[1], tau[1], b).cpu().numpy()  # (n, m): row j = column j of the thin Q
    F = A[1].cpu().numpy()
    e_orth = float(np.abs(Q @ Q.T - np.eye(n)).max())
    R = np.tril(F[:, :n])  # array (j, i), i <= j: element (i, j) of R
    e_qr = float(np.abs(R @ Q - src[1]).max())
    print(f"member 1: max|Q^T Q - I| = {e_orth:.3e}, max|Q R - A| = {e_qr:.3e} (max|A| {np.abs(src[1]).max():.3e})")
    assert e_orth <= 1e-11
    assert e_qr <= 1e-11 * max(1.0, float(np.abs(src[1]).max()))


# ---- G. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_buffers_untouched(tqr):
    """Bad strides and ldda with live device buffers: TQR_EINVAL, and not a byte of either buffer changes."""
    import torch
    m, n, b = SMALL
    kmax = n // b
    lay = Layout(SMALL, F64, 3, ldda=m + 2).fill()
    before = lay.host()
    bq = tqr.BatchedQR(m, n, b, torch.float64, 3)
    L = tqr.lib()
    pA, pT = P(lay.A.data_ptr()), P(lay.tau.data_ptr())
    ld = m + 2
    bad = [
        (m - 1, n * ld, kmax * m),          # ldda < m
        (0, n * ld, kmax * m),
        (8388608, n * 8388608, kmax * m),   # ldda beyond the leading-dimension bound
        (ld, (n - 1) * ld + m - 1, kmax * m),  # one short of stacked
        (ld, m, kmax * m),                  # row-interleaved needs 2 * m + m <= ldda
        (ld, 0, kmax * m),
        (ld, -n * ld, kmax * m),
        (ld, n * ld, kmax * m - 1),         # strideTau short
        (ld, n * ld, 0),
    ]
    for ldda, sA, sT in bad:
        assert L.tqr_batch_execute(bq.h, pA, ldda, sA, pT, sT, None) == TQR_EINVAL, (ldda, sA, sT)
    assert L.tqr_batch_execute(bq.h, None, ld, n * ld, pT, kmax * m, None) == TQR_EINVAL
    assert L.tqr_batch_execute(bq.h, pA, ld, n * ld, None, kmax * m, None) == TQR_EINVAL
    with pytest.raises(tqr.TQRError):
        lay.execute(tqr.BatchedQR(m, n, b, torch.float32, 3))  # the handle's dtype
    assert_same(lay.host(), before, "after refused calls")
    # the handle still works
    ref = lay.wave_reference(tqr)
    lay.execute(bq)
    assert_same(lay.host(), ref)
