"""The tall-skinny QR (include/tqr.h "tall-skinny", csrc/tsqr.hip) on the device.

The contract is one of bytes: every domain of every level has the bytes of tqr_batch_execute on that
layout, every apply those of tqr_apply_q on the member, and nothing outside the matrices is written. The
reference is tests/tsqr_ref.py — the tree's gathers, padding and walks in numpy — with the library's
existing public per-member calls plugged in (tqr.BatchedQR, tqr.ApplyQ through offset pointers), so
sections A and B compare whole allocations without a tolerance. Sections C to E check the meaning with
the project's own bounds, independent of those calls.

A. factor: bytes of A, of every level's W_l and taus; gaps still NaN;
B. apply: bytes in both directions, nrhs in {1, 5, 64, 70}, columns >= nrhs and rows >= m untouched;
C. meaning (fp64): thin Q, Q (Q^T C) = C, (Q^T A)[n:] = 0, lstsq in both directions against numpy;
D. conditioned inputs against an extended-precision R; fp32 against the fp32 oracle tree;
E. more domains than a grid's y dimension holds;
F. ordering: side stream, 10 rounds on alternating streams, two host threads, nrhs_max = 0, re-factor;
G. composition with tqr_trsm_r, and refusals with live device buffers.
"""
import ctypes
import threading

import numpy as np
import pytest

import inputs
import tsqr_ref
from inputs import dtname

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
EINVAL = -1
P = ctypes.c_void_p
# (m, n, b, m_dom, fan): the smallest shapes at which each mechanism exists
SHAPES = [(256, 32, 16, 64, 2),      # three levels, no padding
          (192, 32, 16, 64, 2),      # one zero block at level 1
          (640, 64, 32, 128, 4),     # a group of 1 real + 3 zero blocks
          (320, 32, 32, 32, 4),      # m_dom = n, one tile per domain, D = 10, 3, 1
          (1024, 128, 64, 256, 2),
          (1024, 128, 128, 256, 2),  # two update strips per tile, four reflector groups
          (2048, 256, 256, 512, 2),
          (64, 32, 16, 64, 2)]       # D_0 = 1
CASES = [(s, dt) for s in SHAPES for dt in (F64, F32)]
NRHS = [1, 5, 64, 70]  # one lane, a partial wave, a full strip, two strips with a partial one
NMAX = 70
MEANING = [(640, 64, 32, 128, 4), (1024, 128, 128, 256, 2)]
COND_SHAPE = (1024, 128, 64, 256, 2)


def sid(s):
    return "{}x{}b{}d{}f{}".format(*s)


def ids(cases):
    return [f"{sid(s)}-{dtname(dt)}" for s, dt in cases]


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def same_bytes(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


class Pad:
    """A column-major rows x cols matrix inside a flat NaN-filled device buffer: leading dimension ld >
    rows, an odd base offset, `extra` further NaN columns and 7 guard elements."""

    def __init__(self, rows, cols, dt, pad=3, base=3, extra=0):
        import torch
        self.rows, self.cols, self.ld, self.base = rows, cols, rows + pad, base
        self.buf = torch.full((base + (cols + extra) * self.ld + 7,), float("nan"), dtype=tdt(dt), device="cuda")

    def view(self, buf=None):
        import torch
        return torch.as_strided(self.buf if buf is None else buf, (self.cols, self.rows), (self.ld, 1), self.base)

    def put(self, host):
        import torch
        self.view().copy_(torch.from_numpy(np.array(host, order="C")).cuda())
        torch.cuda.synchronize()
        return self

    @property
    def t(self):
        return self.buf[self.base:]

    def host(self):
        """(the matrix, True if everything else in the allocation is still NaN)."""
        import torch
        torch.cuda.synchronize()
        whole = self.buf.clone()
        mat = self.view(whole).cpu().numpy().copy()
        self.view(whole).fill_(float("nan"))
        return mat, bool(torch.isnan(whole).all())


def dev_view(ptr, nelem, dt):
    """A device allocation of the library as a flat torch tensor (no copy)."""
    import torch

    class Raw:
        pass

    r = Raw()
    r.__cuda_array_interface__ = dict(shape=(nelem,), typestr="<f8" if np.dtype(dt) == np.float64 else "<f4",
                                      data=(ptr, False), version=2)
    return torch.as_tensor(r, device="cuda")


def level_arrays(t, l, n, b, dt):
    """(W_l (n, ldw) or None at level 0, taus (ndom, kmax, rows)) of a handle, as torch views."""
    dW, ldw, dtau, rows, nd = t.level(l)
    kmax = n // b
    W = None if l == 0 else dev_view(dW, n * ldw, dt).view(n, ldw)
    return W, dev_view(dtau, nd * rows * kmax, dt).view(nd, kmax, rows)


_ref = {}


def reference(tqr, shape, dt):
    """(A, the tree by the per-member GPU calls) at `shape`, computed once and never modified."""
    key = (shape, dtname(dt))
    if key not in _ref:
        m, n, b, m_dom, fan = shape
        A = inputs.matrix("gauss", (m, n, b), dt)
        be = tsqr_ref.GpuMemberBackend(tqr, b)
        _ref[key] = (A, be, tsqr_ref.factor(A, b, m_dom, fan, be))
    return _ref[key]


def make(tqr, shape, dt, nrhs_max=NMAX):
    m, n, b, m_dom, fan = shape
    return tqr.TSQR(m, n, b, tdt(dt), m_dom=m_dom, fan=fan, nrhs_max=nrhs_max)


def written_taus_equal(tau, ref, b):
    """Row k of a compact tau is written from element k * b on."""
    return all(same_bytes(tau[:, k, k * b:], ref[:, k, k * b:]) for k in range(tau.shape[1]))


# ---- A. factor: bytes ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", CASES, ids=ids(CASES))
def test_factor_bytes(tqr, shape, dt):
    m, n, b, m_dom, fan = shape
    A, _, ref = reference(tqr, shape, dt)
    t = make(tqr, shape, dt)
    assert t.domains == [L["ndom"] for L in ref["lv"]]
    pad = Pad(m, n, dt).put(A)
    t.factor(pad.t, ldda=pad.ld)
    got, clean = pad.host()
    assert same_bytes(got, ref["A"]), "A differs from the tree of per-member calls"
    assert clean, "an element outside the matrix was written"
    for l, L in enumerate(ref["lv"]):
        W, tau = level_arrays(t, l, n, b, dt)
        assert tuple(tau.shape) == L["aux"].shape
        assert written_taus_equal(tau.cpu().numpy(), L["aux"], b), f"level {l}: taus"
        if l:
            assert same_bytes(W.cpu().numpy(), L["F"]), f"level {l}: W_l"
    if len(ref["lv"]) > 1:
        root = level_arrays(t, len(ref["lv"]) - 1, n, b, dt)[0].cpu().numpy()
        assert same_bytes(np.tril(got[:, :n]), np.tril(root[:, :n])), "the triangle of A[0:n, 0:n] is the root's"


# ---- B. apply: bytes -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", CASES, ids=ids(CASES))
def test_apply_bytes(tqr, shape, dt):
    m, n, b, m_dom, fan = shape
    A, be, ref = reference(tqr, shape, dt)
    t = make(tqr, shape, dt)
    pad = Pad(m, n, dt).put(A)
    t.factor(pad.t, ldda=pad.ld)
    rng = np.random.default_rng(11)
    for nrhs in NRHS:
        C = rng.standard_normal((nrhs, m)).astype(dt)
        for trans in (True, False):
            want = tsqr_ref.apply(ref, C, trans, be)[0]
            pc = Pad(m, nrhs, dt, pad=5, base=1, extra=2).put(C)
            t.apply(pad.t, pc.t, trans=trans, nrhs=nrhs, ldda=pad.ld, lddc=pc.ld)
            got, clean = pc.host()
            assert same_bytes(got, want), f"nrhs {nrhs}, trans {trans}"
            assert clean, f"nrhs {nrhs}, trans {trans}: columns >= nrhs or rows >= m were written"
    assert same_bytes(pad.host()[0], ref["A"]), "the apply wrote to A"


# ---- C. meaning ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MEANING, ids=sid)
def test_meaning(tqr, shape):
    """Bounds of test_gpu_form_q.test_meaning: 1e-11, and 1e-11 * max(1, max|A|)."""
    import torch
    m, n, b, m_dom, fan = shape
    A = inputs.matrix("gauss", (m, n, b))
    amax = max(1.0, float(np.abs(A).max()))
    t = make(tqr, shape, F64, nrhs_max=max(n, 5))
    dA = torch.from_numpy(A.copy()).cuda()
    t.factor(dA)
    Q = torch.full((n, m), float("nan"), dtype=torch.float64, device="cuda")  # output-only
    t.form_q(dA, Q)
    QtA = torch.from_numpy(A.copy()).cuda()
    t.apply(dA, QtA, trans=True)
    C = np.random.default_rng(5).standard_normal((5, m))
    dC = torch.from_numpy(C.copy()).cuda()
    t.apply(dA, dC, trans=True)
    t.apply(dA, dC, trans=False)
    torch.cuda.synchronize()
    Q, F, QtA = Q.cpu().numpy(), dA.cpu().numpy(), QtA.cpu().numpy()
    R = np.tril(F[:, :n])
    e_orth = float(np.abs(Q @ Q.T - np.eye(n)).max())
    e_qr = float(np.abs(R @ Q - A).max())
    e_rt = float(np.abs(dC.cpu().numpy() - C).max())
    e_low = float(np.abs(QtA[:, n:]).max())
    e_top = float(np.abs(QtA[:, :n] - R).max())
    print(f"{sid(shape)}: max|Q^T Q - I| {e_orth:.3e}, max|Q R - A| {e_qr:.3e}, max|Q Q^T C - C| {e_rt:.3e}, "
          f"max|(Q^T A)[n:]| {e_low:.3e}, max|(Q^T A)[:n] - R| {e_top:.3e} (max|A| {amax:.3e})")
    assert e_orth <= 1e-11
    assert e_qr <= 1e-11 * amax
    assert e_rt <= 1e-11 * max(1.0, float(np.abs(C).max()))
    assert e_low <= 1e-11 * amax
    assert e_top <= 1e-11 * amax


@pytest.mark.parametrize("shape", MEANING, ids=sid)
def test_lstsq_vs_numpy(tqr, oracle, shape):
    """Both directions against numpy.linalg.lstsq on the unfactorised A, with test_gpu_solve.py's
    criteria: |X - X_np|_F / |X_np|_F <= 1e-11 cond(A), max|res - res_np| <= 1e-11 |B|_F, and for the
    minimum-norm direction max|A^T x - c| <= 1e-11 |c|_F."""
    import torch
    m, n, b, m_dom, fan = shape
    nrhs = 5
    A = oracle.randzo(m, n, F64, seed=7)
    B = oracle.randzo(m, nrhs, F64, seed=8)
    cond = float(np.linalg.cond(A.T))
    assert cond < 20, cond
    t = make(tqr, shape, F64, nrhs_max=nrhs)
    dA = torch.from_numpy(A.copy()).cuda()
    t.factor(dA)
    dB = torch.from_numpy(B.copy()).cuda()
    dres = torch.full((nrhs,), -1.0, dtype=torch.float64, device="cuda")
    t.lstsq(dA, dB, res=dres)
    Ch = np.ascontiguousarray(B[:, :n])
    Bt = np.full((nrhs, m), np.nan)
    Bt[:, :n] = Ch
    dT = torch.from_numpy(Bt).cuda()
    t.lstsq(dA, dT, trans=True)
    torch.cuda.synchronize()
    out, res = dB.cpu().numpy(), dres.cpu().numpy()
    Xn = np.linalg.lstsq(A.T, B.T, rcond=None)[0]
    rn = np.linalg.norm(A.T @ Xn - B.T, axis=0)
    ex = float(np.linalg.norm(out[:, :n].T - Xn) / np.linalg.norm(Xn))
    er = float(np.abs(res - rn).max())
    x = dT.cpu().numpy().T
    assert np.isfinite(x).all()
    Mn = np.linalg.lstsq(A, Ch.T, rcond=None)[0]  # A^T x = c, minimum norm, m x nrhs
    em = float(np.linalg.norm(x - Mn) / np.linalg.norm(Mn))
    ec = float(np.abs(A @ x - Ch.T).max())
    print(f"{sid(shape)}: cond {cond:.2f}, |X - X_np| / |X_np| {ex:.3e}, max|res - res_np| {er:.3e}, "
          f"minimum norm: |x - x_np| / |x_np| {em:.3e}, max|A^T x - c| {ec:.3e}")
    assert ex <= 1e-11 * cond
    assert er <= 1e-11 * float(np.linalg.norm(B))
    assert em <= 1e-11 * cond
    assert ec <= 1e-11 * float(np.linalg.norm(Ch))


# ---- D. conditioned inputs -------------------------------------------------------------------------
def gpu_final(tqr, shape, A, dt):
    import torch
    t = make(tqr, shape, dt, nrhs_max=0)
    dA = torch.from_numpy(np.array(A, order="C")).cuda()
    t.factor(dA)
    torch.cuda.synchronize()
    tau0 = level_arrays(t, 0, shape[1], shape[2], dt)[1].cpu().numpy()
    return dA.cpu().numpy(), tau0


@pytest.mark.parametrize("family", inputs.FAMILIES)
def test_accuracy_vs_longdouble(tqr, oracle, family):
    """e = col_rel_err of |R| against an extended-precision Householder QR: the GPU tree within 1.5 x the
    oracle-composed tree's error on the same matrix (test_gpu_inputs.test_accuracy_vs_longdouble's factor)."""
    if not inputs.have_longdouble():
        pytest.skip("numpy.longdouble is no wider than double here")
    m, n, b, m_dom, fan = COND_SHAPE
    A = inputs.matrix(family, (m, n, b))
    R_ld = inputs.r_longdouble(family, (m, n, b))
    ref = tsqr_ref.factor(A, b, m_dom, fan, tsqr_ref.OracleBackend(oracle, b))
    F, _ = gpu_final(tqr, COND_SHAPE, A, F64)
    e_gpu, e_ref = inputs.col_rel_err(F, R_ld), inputs.col_rel_err(ref["A"], R_ld)
    cn = inputs.colnorm_rel_err(A, F)
    print(f"{family} {sid(COND_SHAPE)}: e_gpu {e_gpu:.3e}, e_ref {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}, column norms {cn:.3e}")
    assert np.isfinite(F).all()
    assert cn <= 1e-12
    assert e_gpu <= 1.5 * e_ref


def test_accuracy_fp32(tqr, oracle):
    """fp32 storage, test_gpu_inputs.test_accuracy_fp32's criteria against the fp32 oracle tree: the final A
    within 1e-4 max(1, max|F|), level 0's taus within 2e-4, and no farther from the fp64 oracle tree on the
    same fp32-valued input than 1.5 x the fp32 oracle tree is."""
    m, n, b, m_dom, fan = COND_SHAPE
    A = inputs.matrix("gauss", (m, n, b), F32)
    r32 = tsqr_ref.factor(A, b, m_dom, fan, tsqr_ref.OracleBackend(oracle, b))
    r64 = tsqr_ref.factor(A.astype(F64), b, m_dom, fan, tsqr_ref.OracleBackend(oracle, b))
    F, tau0 = gpu_final(tqr, COND_SHAPE, A, F32)
    Fg = F.astype(F64)
    dF = float(np.abs(Fg - r32["A"]).max())
    dT = 0.0
    for i, T in enumerate(r32["lv"][0]["aux"]):  # the oracle's tau matrix of domain i: row k*b holds step k's taus
        for k in range(n // b):
            dT = max(dT, float(np.abs(tau0[i, k, k * b:].astype(F64) - T[k * b, k * b:]).max()))
    e_gpu, e_ref = float(np.abs(Fg - r64["A"]).max()), float(np.abs(r32["A"] - r64["A"]).max())
    print(f"fp32 {sid(COND_SHAPE)}: max|dF| {dF:.3e} (max|F| {np.abs(r32['A']).max():.3e}), max|dtau| {dT:.3e}, "
          f"vs fp64 tree: GPU {e_gpu:.3e}, fp32 oracle tree {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}")
    assert dF <= 1e-4 * max(1.0, float(np.abs(r32["A"]).max()))
    assert dT <= 2e-4
    assert e_gpu <= 1.5 * e_ref


# ---- E. more domains than a grid's y ---------------------------------------------------------------
def test_more_domains_than_grid_y(tqr):
    """m = 65537 * 16, n = b = m_dom = 16, fan = 16: D = 65537, 4097, 257, 17, 2, 1 — level 0 and its applies
    run as two launches each. |R| against numpy.linalg.qr's to 1e-11 max|R|; lstsq with 3 right-hand sides
    against numpy with test_gpu_solve.py's criteria."""
    import torch
    m, n, b = 65537 * 16, 16, 16
    t = tqr.TSQR(m, n, b, torch.float64, m_dom=16, fan=16, nrhs_max=3)
    assert t.domains == [65537, 4097, 257, 17, 2, 1]
    g = torch.Generator(device="cuda").manual_seed(17)
    dA = torch.randn((n, m), dtype=torch.float64, device="cuda", generator=g)
    dB = torch.randn((3, m), dtype=torch.float64, device="cuda", generator=g)
    A, B = dA.cpu().numpy(), dB.cpu().numpy()
    dres = torch.empty(3, dtype=torch.float64, device="cuda")
    t.factor(dA)
    t.lstsq(dA, dB, res=dres)
    torch.cuda.synchronize()
    R = np.tril(dA[:, :n].cpu().numpy()).T
    Rn = np.linalg.qr(A.T, mode="r")
    e_r = float(np.abs(np.abs(R) - np.abs(Rn)).max())
    Xn = np.linalg.lstsq(A.T, B.T, rcond=None)[0]
    rn = np.linalg.norm(A.T @ Xn - B.T, axis=0)
    cond = float(np.linalg.cond(Rn))
    ex = float(np.linalg.norm(dB[:, :n].cpu().numpy().T - Xn) / np.linalg.norm(Xn))
    er = float(np.abs(dres.cpu().numpy() - rn).max())
    print(f"max||R| - |R_np|| {e_r:.3e} (max|R| {np.abs(Rn).max():.3e}), cond {cond:.2f}, |X - X_np| / |X_np| {ex:.3e}, "
          f"max|res - res_np| {er:.3e} (|B|_F {np.linalg.norm(B):.3e})")
    assert e_r <= 1e-11 * float(np.abs(Rn).max())
    assert ex <= 1e-11 * cond
    assert er <= 1e-11 * float(np.linalg.norm(B))


# ---- F. ordering -----------------------------------------------------------------------------------
ORD = (192, 32, 16, 64, 2)


def sync_results(tqr, t, A, C, trans=True):
    """(A after factor, C after apply, B and res after lstsq) by synchronous calls on handle t."""
    import torch
    dA, dC, dB = (torch.from_numpy(np.array(x, order="C")).cuda() for x in (A, C, C))
    dres = torch.empty(C.shape[0], dtype=dA.dtype, device="cuda")
    torch.cuda.synchronize()
    t.factor(dA)
    torch.cuda.synchronize()
    t.apply(dA, dC, trans=trans)
    torch.cuda.synchronize()
    t.lstsq(dA, dB, res=dres)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (dA, dC, dB, dres)]


def ord_inputs():
    m, n, b = ORD[:3]
    A = [inputs.matrix("gauss", (m, n, b), F64, off) for off in (0, 1)]
    C = np.random.default_rng(9).standard_normal((5, m))
    return A, C


def test_input_written_on_side_stream(tqr):
    import torch
    (A0, _), C = ord_inputs()
    t = make(tqr, ORD, F64)
    want = sync_results(tqr, t, A0, C)
    src = torch.from_numpy(A0.copy()).cuda()
    dst = torch.full_like(src, float("nan"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dst.copy_(src, non_blocking=True)
        t.factor(dst, stream=s)
    torch.cuda.synchronize()
    assert same_bytes(dst.cpu().numpy(), want[0])


def test_ten_rounds_alternating_streams(tqr):
    """factor -> apply -> factor (other data) -> lstsq, 10 rounds back to back on two alternating streams
    with no host synchronisation: the handle's events order every call behind the one before it."""
    import torch
    (A0, A1), C = ord_inputs()
    t = make(tqr, ORD, F64)
    w0, w1 = sync_results(tqr, t, A0, C), sync_results(tqr, t, A1, C)
    up = lambda x: torch.from_numpy(np.array(x, order="C")).cuda()
    bufs = [dict(a0=up(A0), c=up(C), a1=up(A1), b=up(C), r=torch.empty(5, dtype=torch.float64, device="cuda"))
            for _ in range(10)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for x, u in enumerate(bufs):
        t.factor(u["a0"], stream=streams[x % 2])
        t.apply(u["a0"], u["c"], stream=streams[(x + 1) % 2])
        t.factor(u["a1"], stream=streams[x % 2])
        t.lstsq(u["a1"], u["b"], res=u["r"], stream=streams[(x + 1) % 2])
    torch.cuda.synchronize()
    for x, u in enumerate(bufs):
        assert same_bytes(u["a0"].cpu().numpy(), w0[0]) and same_bytes(u["c"].cpu().numpy(), w0[1]), f"round {x}"
        assert same_bytes(u["a1"].cpu().numpy(), w1[0]) and same_bytes(u["b"].cpu().numpy(), w1[2]), f"round {x}"
        assert same_bytes(u["r"].cpu().numpy(), w1[3]), f"round {x}"


def test_two_threads_share_one_handle(tqr):
    """Two host threads, each with its own stream and buffers, 4 x (factor, apply) on one handle. The
    handle holds the factorisation's T factors, so both threads factorise copies of the same matrix: any
    interleaving of the calls then gives the same bytes."""
    import torch
    (A0, _), C = ord_inputs()
    t = make(tqr, ORD, F64)
    want = sync_results(tqr, t, A0, C)
    up = lambda x: torch.from_numpy(np.array(x, order="C")).cuda()
    bufs = [[(up(A0), up(C)) for _ in range(4)] for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    errors = []
    torch.cuda.synchronize()

    def work(i):
        try:
            for a, c in bufs[i]:
                t.factor(a, stream=streams[i])
                t.apply(a, c, stream=streams[i])
            streams[i].synchronize()
        except Exception as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for i in range(2):
        for x, (a, c) in enumerate(bufs[i]):
            assert same_bytes(a.cpu().numpy(), want[0]) and same_bytes(c.cpu().numpy(), want[1]), f"thread {i}, round {x}"


def test_refactor_forgets_the_first_matrix(tqr):
    """A handle factorised on a second matrix gives a fresh handle's bytes, although every W_l was filled
    with NaN in between: each factor rewrites the whole of every W_l."""
    import torch
    (A0, A1), C = ord_inputs()
    m, n, b = ORD[:3]
    want = sync_results(tqr, make(tqr, ORD, F64), A1, C)
    t = make(tqr, ORD, F64)
    sync_results(tqr, t, A0, C)
    for l in range(1, t.levels):
        level_arrays(t, l, n, b, F64)[0].fill_(float("nan"))
    torch.cuda.synchronize()
    got = sync_results(tqr, t, A1, C)
    for g, w, what in zip(got, want, ("A", "Q^T C", "lstsq B", "res")):
        assert same_bytes(g, w), what
    for l in range(1, t.levels):
        assert torch.isfinite(level_arrays(t, l, n, b, F64)[0]).all()


def test_no_c_workspace_refuses_the_applies(tqr):
    import torch
    (A0, _), C = ord_inputs()
    m, n, b = ORD[:3]
    t = make(tqr, ORD, F64, nrhs_max=0)
    dA, dC = torch.from_numpy(A0.copy()).cuda(), torch.from_numpy(C.copy()).cuda()
    t.factor(dA)
    torch.cuda.synchronize()
    L = tqr.lib()
    pA, pC = P(dA.data_ptr()), P(dC.data_ptr())
    assert L.tqr_tsqr_apply_q(t.h, 1, pA, m, pC, 1, m, None) == EINVAL
    assert L.tqr_tsqr_lstsq(t.h, 0, pA, m, pC, 1, m, None, None) == EINVAL
    assert L.tqr_tsqr_form_q(t.h, pA, m, pC, m, None) == EINVAL
    torch.cuda.synchronize()
    assert same_bytes(dC.cpu().numpy(), C)


# ---- G. composition and refusals -------------------------------------------------------------------
def test_trsm_r_on_the_factorised_matrix(tqr):
    """tqr_trsm_r directly on dA after factor solves with the final R: the bytes of the solve on a matrix
    that holds R alone, and the componentwise substitution bound of include/tqr.h (<= n)."""
    import torch
    shape = (640, 64, 32, 128, 4)
    m, n, b = shape[:3]
    A = inputs.matrix("gauss", (m, n, b))
    t = make(tqr, shape, F64, nrhs_max=0)
    dA = torch.from_numpy(A.copy()).cuda()
    t.factor(dA)
    torch.cuda.synchronize()
    F = dA.cpu().numpy()
    R = inputs.upper(F, n)
    Y = np.random.default_rng(2).standard_normal((5, n))
    for trans in (False, True):
        X = torch.from_numpy(Y.copy()).cuda()
        tqr.trsm_r(dA, X, b, trans=trans, n=n, lddx=n)
        only_r = torch.from_numpy(np.ascontiguousarray(np.tril(F[:, :n]))).cuda()
        X2 = torch.from_numpy(Y.copy()).cuda()
        tqr.trsm_r(only_r, X2, b, trans=trans, n=n, lddx=n)
        torch.cuda.synchronize()
        assert same_bytes(X.cpu().numpy(), X2.cpu().numpy())
        ratio = inputs.backward_ratio(R, X.cpu().numpy(), Y, trans, np.finfo(F64).eps / 2)
        print(f"trans {trans}: componentwise backward ratio {ratio:.2f} (bound {n})")
        assert ratio <= n


def test_refusals_leave_buffers_untouched(tqr):
    import torch
    (A0, _), C = ord_inputs()
    m, n, b = ORD[:3]
    t = make(tqr, ORD, F64, nrhs_max=8)
    pa, pc = Pad(m, n, F64).put(A0), Pad(m, 5, F64).put(C)
    before = (pa.buf.cpu().numpy(), pc.buf.cpu().numpy())
    L = tqr.lib()
    A_, C_ = P(pa.t.data_ptr()), P(pc.t.data_ptr())
    # before the first factor every other call is refused
    assert L.tqr_tsqr_apply_q(t.h, 1, A_, pa.ld, C_, 5, pc.ld, None) == EINVAL
    assert L.tqr_tsqr_lstsq(t.h, 0, A_, pa.ld, C_, 5, pc.ld, None, None) == EINVAL
    assert L.tqr_tsqr_form_q(t.h, A_, pa.ld, C_, pc.ld, None) == EINVAL
    for ldda in (m - 1, 0, -m, 8388608):
        assert L.tqr_tsqr_factor(t.h, A_, ldda, None) == EINVAL, ldda
    assert L.tqr_tsqr_factor(t.h, None, pa.ld, None) == EINVAL
    torch.cuda.synchronize()
    assert same_bytes(pa.buf.cpu().numpy(), before[0]) and same_bytes(pc.buf.cpu().numpy(), before[1])
    t.factor(pa.t, ldda=pa.ld)
    torch.cuda.synchronize()
    fact = pa.buf.cpu().numpy()
    bad = [dict(trans=2), dict(nrhs=0), dict(nrhs=9), dict(ldda=m - 1), dict(ldc=m - 1), dict(ldc=8388608), dict(A=None),
           dict(C=None)]
    for kw in bad:
        a = dict(trans=1, A=A_, ldda=pa.ld, C=C_, nrhs=5, ldc=pc.ld)
        a.update(kw)
        assert L.tqr_tsqr_apply_q(t.h, a["trans"], a["A"], a["ldda"], a["C"], a["nrhs"], a["ldc"], None) == EINVAL, kw
        assert L.tqr_tsqr_lstsq(t.h, a["trans"], a["A"], a["ldda"], a["C"], a["nrhs"], a["ldc"], None, None) == EINVAL, kw
    assert L.tqr_tsqr_form_q(t.h, A_, pa.ld, C_, pc.ld, None) == EINVAL, "form_q needs nrhs_max >= n"
    with pytest.raises(tqr.TQRError):
        t.apply(pa.t.float(), pc.t, nrhs=5, ldda=pa.ld, lddc=pc.ld)  # the handle's dtype
    torch.cuda.synchronize()
    assert same_bytes(pa.buf.cpu().numpy(), fact) and same_bytes(pc.buf.cpu().numpy(), before[1])
    # the handle still works
    t.apply(pa.t, pc.t, nrhs=5, ldda=pa.ld, lddc=pc.ld)
    got, clean = pc.host()
    assert clean and np.isfinite(got).all()
