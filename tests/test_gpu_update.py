"""tqr_update_* (include/tqr.h "row update") on the GPU.

The bit contract is the separation identity (tests/test_update_cpu.py checks it on the oracle): a wave plan
on the stacked S = [G; W] equals a wave plan on G followed by tqr_update_rows with W, byte for byte — the
upper triangle, the W rows (V) and their taus — and the stacked factorisation's apply equals G's apply and
tqr_update_apply_q in sequence. Both sides of every byte comparison come from the GPU; the values are held
against the oracle model (tests/update_ref.py) within the project's bounds (test_gpu_factor.assert_close:
fp64 1e-11 scaled, fp32 1e-3; the apply tests' 1e-11 / 1e-4 scaled).

Every device array is a NaN-filled allocation with an offset base and a padded leading dimension; after
each call everything outside the logical blocks must still be NaN.
"""
import threading

import numpy as np
import pytest

import inputs
import update_ref
from test_gpu_factor import assert_close

pytestmark = pytest.mark.gpu

# (b, q, wt): q >= 2 gives a head-row chain, wt >= 2 the TSQRT chain through R_kk, q >= 3 with wt >= 2 puts
# panel and update items on one level
SHAPES = [(16, 4, 2), (32, 3, 2), (64, 2, 3), (128, 2, 1), (256, 2, 1), (256, 3, 2)]
DTYPES = [np.float64, np.float32]
CASES = [(s, dt) for s in SHAPES for dt in DTYPES]
IDS = [f"b{b}q{q}wt{wt}-{'f64' if dt == np.float64 else 'f32'}" for (b, q, wt), dt in CASES]
APPLY_SHAPES = [(16, 4, 2), (32, 3, 2), (128, 2, 1), (256, 3, 2)]
APPLY_CASES = [(s, dt) for s in APPLY_SHAPES for dt in DTYPES]
APPLY_IDS = [f"b{b}q{q}wt{wt}-{'f64' if dt == np.float64 else 'f32'}" for (b, q, wt), dt in APPLY_CASES]
NRHS = [1, 5, 64, 70]  # one lane, a ragged wave, one full workgroup, two workgroups (the second ragged)

_cache = {}


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


class Pad:
    """A (cols, rows) host array inside a NaN-filled flat device allocation: element (i, j) at
    off + j * ld + i, `tail` NaN elements after the last column."""

    def __init__(self, host, ld, off=0, tail=9):
        import torch
        self.cols, self.rows = host.shape
        self.ld, self.off = ld, off
        flat = np.full(off + self.cols * ld + tail, np.nan, dtype=host.dtype)
        flat[off:off + self.cols * ld].reshape(self.cols, ld)[:, :self.rows] = host
        self.dev = torch.from_numpy(flat).cuda()
        self.t = self.dev[off:]  # what the calls get, with ld given explicitly

    def get(self, check=True):
        """The logical block; asserts that everything around it is still NaN."""
        flat = self.dev.cpu().numpy()
        body = flat[self.off:self.off + self.cols * self.ld].reshape(self.cols, self.ld)
        if check:
            assert np.isnan(flat[:self.off]).all() and np.isnan(flat[self.off + self.cols * self.ld:]).all()
            assert np.isnan(body[:, self.rows:]).all(), "rows beyond the block were written"
        return np.array(body[:, :self.rows])


def same(a, b):
    return np.array_equal(inputs.bits(a), inputs.bits(b))


def problem(oracle, b, q, wt, dt):
    """S = [G; W] (RANDZO), read-only."""
    key = ("S", b, q, wt, np.dtype(dt).name)
    if key not in _cache:
        S = oracle.randzo((q + wt) * b, q * b, dt, seed=11 + b)
        S.setflags(write=False)
        _cache[key] = S
    return _cache[key]


def run_case(tqr, oracle, b, q, wt, dt, engine="waves"):
    """The stacked wave plan, G's plan (`engine`) and the update on a side stream. Returns a dict of the
    host results and the live device objects (computed once per case and engine)."""
    import torch
    key = ("run", b, q, wt, np.dtype(dt).name, engine)
    if key in _cache:
        return _cache[key]
    n, mw = q * b, wt * b
    S = problem(oracle, b, q, wt, dt)
    side = torch.cuda.Stream()
    # the stacked factorisation
    dS = Pad(S, n + mw + 4, off=3)
    tauS = torch.full((q, n + mw), float("nan"), dtype=tdt(dt), device="cuda")
    # G alone, then the update: lddr != lddw, offset bases
    dG = Pad(np.ascontiguousarray(S[:, :n]), n + 8, off=5)
    tauG = torch.full((q, n), float("nan"), dtype=tdt(dt), device="cuda")
    dW = Pad(np.ascontiguousarray(S[:, n:]), mw + 3, off=7)
    tauU = Pad(np.full((q, mw), np.nan, dtype=dt), mw, off=2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        pS = tqr.TiledQR(n + mw, n, b, tdt(dt), engine="waves")
        pS.execute(dS.t, tauS, ldda=dS.ld, stream=side.cuda_stream)
        pG = tqr.TiledQR(n, n, b, tdt(dt), engine=engine)
        pG.execute(dG.t, tauG, ldda=dG.ld, stream=side.cuda_stream)
        pS.status(side.cuda_stream)
        pG.status(side.cuda_stream)
        FG = dG.get()
        up = tqr.RowUpdate(n, mw, b, tdt(dt))
        up.update(dG.t, dW.t, tauU.t, lddr=dG.ld, lddw=dW.ld, stream=side)
    side.synchronize()
    out = dict(S=S, FS=dS.get(), tauS=tauS.cpu().numpy(), FG=FG, tauG=tauG.cpu().numpy(), R=dG.get(), V=dW.get(),
               tauU=tauU.get(), dS=dS, dtauS=tauS, dG=dG, dtauG=tauG, dW=dW, dtauU=tauU, up=up, n=n, mw=mw)
    _cache[key] = out
    return out


def tri(n):
    return np.tril(np.ones((n, n), dtype=bool))  # elements (i, j), i <= j, of an (n, n) array[j, i]


# ---- 1. byte-equality against the stacked wave plan -------------------------------------------------
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_rows_equal_stacked_wave_plan(tqr, oracle, shape, dt):
    b, q, wt = shape
    r = run_case(tqr, oracle, b, q, wt, dt)
    n, up = r["n"], tri(r["n"])
    assert same(r["R"][up], r["FS"][:, :n][up]), "upper triangle"
    assert same(r["V"], r["FS"][:, n:]), "the W rows: V"
    assert same(r["tauU"], r["tauS"][:, n:]), "the W rows' taus"
    assert same(r["R"][~up], r["FG"][~up]), "G's V keeps its bytes"
    assert same(r["FG"][~up], r["FS"][:, :n][~up]) and same(r["tauG"], r["tauS"][:, :n])


# ---- 2. against the oracle model; what lies below the diagonal --------------------------------------
@pytest.mark.parametrize("engine", ["waves", "flow"])
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_rows_vs_oracle_model(tqr, oracle, shape, dt, engine):
    b, q, wt = shape
    r = run_case(tqr, oracle, b, q, wt, dt, engine)
    n, up = r["n"], tri(r["n"])
    assert same(r["R"][~up], r["FG"][~up]), "below the diagonal: bytes unchanged"
    Rm, Vm, tm = update_ref.update(oracle, r["FG"], np.ascontiguousarray(r["S"][:, n:]), b)
    got = np.concatenate([np.where(up, r["R"], 0), r["V"]], axis=1)
    ref = np.concatenate([np.where(up, Rm, 0), Vm], axis=1)
    assert_close(got, r["tauU"], ref, tm)


@pytest.mark.parametrize("shape,dt", [((32, 3, 2), np.float64), ((256, 2, 1), np.float32)], ids=["b32-f64", "b256-f32"])
def test_nan_below_the_diagonal_never_enters(tqr, oracle, shape, dt):
    import torch
    b, q, wt = shape
    r = run_case(tqr, oracle, b, q, wt, dt)
    n, mw, up = r["n"], r["mw"], tri(r["n"])
    Fn = r["FG"].copy()
    Fn[~up] = np.nan
    dR = Pad(Fn, n + 8, off=5)
    dW = Pad(np.ascontiguousarray(r["S"][:, n:]), mw + 3, off=7)
    tau = Pad(np.full((q, mw), np.nan, dtype=dt), mw, off=2)
    torch.cuda.synchronize()
    r["up"].update(dR.t, dW.t, tau.t, lddr=dR.ld, lddw=dW.ld)
    torch.cuda.synchronize()
    R = dR.get()
    assert np.isnan(R[~up]).all() and same(R[~up], Fn[~up])
    assert same(R[up], r["R"][up]) and same(dW.get(), r["V"]) and same(tau.get(), r["tauU"])


# ---- 3. apply -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", APPLY_CASES, ids=APPLY_IDS)
def test_apply_identities_and_prepare(tqr, oracle, shape, dt):
    import torch
    b, q, wt = shape
    r = run_case(tqr, oracle, b, q, wt, dt)
    n, mw, m = r["n"], r["mw"], r["n"] + r["mw"]
    nmax = max(NRHS)
    C = oracle.randzo(m, nmax + 2, dt, seed=23)  # two more columns than any nrhs: they must stay
    apS = tqr.ApplyQ(m, n, b, tdt(dt))
    apS.prepare(r["dS"].t, r["dtauS"], ldda=r["dS"].ld)
    apG = tqr.ApplyQ(n, n, b, tdt(dt))
    apG.prepare(r["dG"].t, r["dtauG"], ldda=r["dG"].ld)  # after the update: V and taus are G's still
    up2 = tqr.RowUpdate(n, mw, b, tdt(dt))
    up2.prepare(r["dW"].t, r["dtauU"].t, lddw=r["dW"].ld)
    for nrhs in NRHS:
        for trans in (True, False):
            cS = Pad(C, m + 6, off=1)
            apS.apply(r["dS"].t, cS.t, trans=trans, nrhs=nrhs, ldda=r["dS"].ld, lddc=cS.ld)
            outs = []
            for h in (r["up"], up2):
                ct = Pad(np.ascontiguousarray(C[:, :n]), n + 5, off=4)
                cn = Pad(np.ascontiguousarray(C[:, n:]), mw + 2, off=6)
                ga = lambda: apG.apply(r["dG"].t, ct.t, trans=trans, nrhs=nrhs, ldda=r["dG"].ld, lddc=ct.ld)
                ua = lambda: h.apply(r["dW"].t, ct.t, cn.t, trans=trans, nrhs=nrhs, lddw=r["dW"].ld, lddct=ct.ld, lddcn=cn.ld)
                if trans:
                    ga(); ua()
                else:
                    ua(); ga()
                outs.append((ct, cn))
            torch.cuda.synchronize()
            want = cS.get()
            for ct, cn in outs:
                t, c = ct.get(), cn.get()
                assert same(t, want[:, :n]) and same(c, want[:, n:]), f"nrhs={nrhs} trans={trans}"
                assert same(t[nrhs:], C[nrhs:, :n]) and same(c[nrhs:], C[nrhs:, n:]), "columns >= nrhs"
    # Q_u (Q_u^T C) = C, and Q_u^T against the model
    ct = Pad(np.ascontiguousarray(C[:, :n]), n + 5, off=4)
    cn = Pad(np.ascontiguousarray(C[:, n:]), mw + 2, off=6)
    kw = dict(nrhs=nmax, lddw=r["dW"].ld, lddct=ct.ld, lddcn=cn.ld)
    r["up"].apply(r["dW"].t, ct.t, cn.t, trans=True, **kw)
    torch.cuda.synchronize()
    mid = np.concatenate([ct.get(), cn.get()], axis=1)[:nmax]
    r["up"].apply(r["dW"].t, ct.t, cn.t, trans=False, **kw)
    torch.cuda.synchronize()
    back = np.concatenate([ct.get(), cn.get()], axis=1)[:nmax]
    tol = 1e-11 if dt == np.float64 else 1e-4
    ref = np.concatenate(update_ref.apply(r["V"], r["tauU"], C[:nmax, :n], C[:nmax, n:], b, trans=True), axis=1)
    em = float(np.abs(mid.astype(np.float64) - ref).max())
    eb = float(np.abs(back.astype(np.float64) - C[:nmax]).max())
    print(f"max|Q_u^T C - model| = {em:.3e}, max|Q_u Q_u^T C - C| = {eb:.3e}")
    assert em <= tol * max(1.0, float(np.abs(ref).max()))
    assert eb <= tol * max(1.0, float(np.abs(C).max()))


def test_apply_before_prepare_is_refused(tqr):
    import torch
    up = tqr.RowUpdate(64, 32, 32, torch.float64)
    W = torch.zeros((64, 32), dtype=torch.float64, device="cuda")
    Ct, Cn = torch.zeros((3, 64), dtype=torch.float64, device="cuda"), torch.zeros((3, 32), dtype=torch.float64, device="cuda")
    with pytest.raises(tqr.TQRError):
        up.apply(W, Ct, Cn)


# ---- 4. tqr_update_lstsq ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dt", [((32, 3, 2), np.float64), ((256, 2, 1), np.float64), ((64, 2, 3), np.float32)],
                         ids=["b32-f64", "b256-f64", "b64-f32"])
def test_lstsq_equals_its_parts(tqr, oracle, shape, dt):
    import torch
    b, q, wt = shape
    r = run_case(tqr, oracle, b, q, wt, dt)
    n, mw, nrhs = r["n"], r["mw"], 5
    Wh = np.ascontiguousarray(r["S"][:, n:])
    Dh = oracle.randzo(n, nrhs, dt, seed=31)
    Bh = oracle.randzo(mw, nrhs, dt, seed=32)
    res0 = np.abs(oracle.randzo(nrhs, 1, dt, seed=33)[0]) + 0.5
    up = r["up"]

    def bufs():
        return (Pad(r["FG"], n + 8, off=5), Pad(Wh, mw + 3, off=7), Pad(np.full((q, mw), np.nan, dtype=dt), mw, off=2),
                Pad(Dh, n + 1, off=3), Pad(Bh, mw + 6, off=1), Pad(np.full((nrhs, n), np.nan, dtype=dt), n + 2, off=8))
    R1, W1, t1, D1, B1, X1 = bufs()
    dres = torch.from_numpy(res0.copy()).cuda()
    torch.cuda.synchronize()
    up.lstsq(R1.t, W1.t, t1.t, D1.t, B1.t, X1.t, res=dres, nrhs=nrhs, lddr=R1.ld, lddw=W1.ld, lddd=D1.ld, lddb=B1.ld,
             lddx=X1.ld)
    R2, W2, t2, D2, B2, X2 = bufs()
    up.update(R2.t, W2.t, t2.t, lddr=R2.ld, lddw=W2.ld)
    up.apply(W2.t, D2.t, B2.t, trans=True, nrhs=nrhs, lddw=W2.ld, lddct=D2.ld, lddcn=B2.ld)
    torch.cuda.synchronize()
    X2 = Pad(D2.get(), n + 2, off=8)
    tqr.trsm_r(R2.t, X2.t, b, n=n, nrhs=nrhs, ldda=R2.ld, lddx=X2.ld)
    torch.cuda.synchronize()
    for a, c in ((R1, R2), (W1, W2), (t1, t2), (D1, D2), (B1, B2), (X1, X2)):
        assert same(a.get(), c.get())
    # the running residual norms: sqrt(res0^2 + |Bnew'|^2), fp64 sums, one rounding to the dtype
    Bn = B1.get().astype(np.float64)
    want = np.sqrt(res0.astype(np.float64) ** 2 + (Bn * Bn).sum(axis=1))
    got = dres.cpu().numpy().astype(np.float64)
    rel = float(np.abs(got - want).max() / want.max())
    print(f"res: rel {rel:.2e}")
    assert rel <= 4 * np.finfo(dt).eps
    # res = None leaves the same bytes elsewhere
    R3, W3, t3, D3, B3, X3 = bufs()
    up.lstsq(R3.t, W3.t, t3.t, D3.t, B3.t, X3.t, nrhs=nrhs, lddr=R3.ld, lddw=W3.ld, lddd=D3.ld, lddb=B3.ld, lddx=X3.ld)
    torch.cuda.synchronize()
    assert same(X3.get(), X1.get()) and same(B3.get(), B1.get())


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_recursive_least_squares(tqr, dt):
    """ApplyQ.lstsq on A0, then three appended blocks: after each, the solution and the residual norms
    against numpy.linalg.lstsq on all rows so far, within test_gpu_solve's bound for tqr_lstsq
    (|X - X_np|_F / |X_np|_F <= tol cond(A), max|res - res_np| <= tol |B|_F; tol 1e-11 / 1e-4)."""
    import torch
    b, n, m0, mw, nrhs = 64, 128, 256, 128, 5
    tol = 1e-11 if dt == np.float64 else 1e-4
    rng = np.random.default_rng(20)
    A = rng.standard_normal((n, m0 + 3 * mw)).astype(dt)  # (n, rows): column-major A
    B = rng.standard_normal((nrhs, m0 + 3 * mw)).astype(dt)
    dF = torch.from_numpy(np.ascontiguousarray(A[:, :m0])).cuda()
    tau = torch.zeros((n // b, m0), dtype=tdt(dt), device="cuda")
    plan = tqr.TiledQR(m0, n, b, tdt(dt))
    plan.execute(dF, tau)
    plan.status()
    ap = tqr.ApplyQ(m0, n, b, tdt(dt))
    ap.prepare(dF, tau)
    dB = torch.from_numpy(np.ascontiguousarray(B[:, :m0])).cuda()
    dQ = dB.clone()
    dres = torch.zeros(nrhs, dtype=tdt(dt), device="cuda")
    ap.lstsq(dF, dB, res=dres)
    ap.apply(dF, dQ, trans=True)
    dD = dQ[:, :n].contiguous()
    dX = torch.full((nrhs, n), float("nan"), dtype=tdt(dt), device="cuda")
    up = tqr.RowUpdate(n, mw, b, tdt(dt))
    torch.cuda.synchronize()

    def check(rows, X, res):
        A64, B64 = A[:, :rows].T.astype(np.float64), B[:, :rows].T.astype(np.float64)
        Xn = np.linalg.lstsq(A64, B64, rcond=None)[0]
        rn = np.linalg.norm(A64 @ Xn - B64, axis=0)
        cond = float(np.linalg.cond(A64))
        ex = float(np.linalg.norm(X.T.astype(np.float64) - Xn) / np.linalg.norm(Xn))
        er = float(np.abs(res.astype(np.float64) - rn).max())
        print(f"rows {rows}: cond {cond:.2f}, |X - X_np|/|X_np| = {ex:.3e}, max|res - res_np| = {er:.3e}")
        assert ex <= tol * cond
        assert er <= tol * float(np.linalg.norm(B64))

    check(m0, dB.cpu().numpy()[:, :n], dres.cpu().numpy())
    for i in range(3):
        r0 = m0 + i * mw
        dW = torch.from_numpy(np.ascontiguousarray(A[:, r0:r0 + mw])).cuda()
        dBn = torch.from_numpy(np.ascontiguousarray(B[:, r0:r0 + mw])).cuda()
        tu = torch.zeros((n // b, mw), dtype=tdt(dt), device="cuda")
        up.lstsq(dF, dW, tu, dD, dBn, dX, res=dres, lddr=m0)
        torch.cuda.synchronize()
        check(r0 + mw, dX.cpu().numpy(), dres.cpu().numpy())


# ---- 5. zero-padded rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_zero_padded_rows(tqr, oracle, dt):
    """W with its last b + 3 rows zero: those rows of V are +-0, the taus of the all-zero tile are the
    convention's 2 (v_B = 0: tau = 2 / (1 + 0); exactly 2 in the model), and R' matches the model of the
    same padded W."""
    import torch
    b, q, wt = 32, 3, 2
    r = run_case(tqr, oracle, b, q, wt, dt)
    n, mw, up = r["n"], r["mw"], tri(r["n"])
    Wh = np.array(r["S"][:, n:])
    Wh[:, mw - b - 3:] = 0
    dR = Pad(r["FG"], n + 8, off=5)
    dW = Pad(Wh, mw + 3, off=7)
    tau = Pad(np.full((q, mw), np.nan, dtype=dt), mw, off=2)
    torch.cuda.synchronize()
    r["up"].update(dR.t, dW.t, tau.t, lddr=dR.ld, lddw=dW.ld)
    torch.cuda.synchronize()
    R, V, tu = dR.get(), dW.get(), tau.get()
    assert (V[:, mw - b - 3:] == 0).all(), "zero rows stay +-0 in V"
    # (the engine forms tau as a product with a reciprocal square root, clamped to [1, 2]: a few ulp)
    assert (tu[:, b:] <= 2).all() and (np.abs(tu[:, b:].astype(np.float64) - 2) <= 8 * np.finfo(dt).eps).all(), "tau = 2"
    Rm, Vm, tm = update_ref.update(oracle, r["FG"], Wh, b)
    assert (tm[:, b:] == 2).all() and (Vm[:, mw - b - 3:] == 0).all()
    assert_close(np.concatenate([np.where(up, R, 0), V], axis=1), tu, np.concatenate([np.where(up, Rm, 0), Vm], axis=1), tm)
    assert same(R[~up], r["FG"][~up])


# ---- 6. handle behaviour ------------------------------------------------------------------------------
def chain_inputs(oracle, b, q, wt, count, seed):
    n, mw = q * b, wt * b
    R0 = np.ascontiguousarray(oracle.factor(oracle.randzo(n, n, np.float64, seed=seed), b)[0])
    Ws = [oracle.randzo(mw, n, np.float64, seed=seed + 1 + i) for i in range(count)]
    return R0, Ws


def run_chain(tqr, up, R0, Ws, q, stream=None, sync=False):
    """R <- update(R, W_i) for every i on `stream`; returns the device tensors."""
    import torch
    dR = torch.from_numpy(R0.copy()).cuda()
    dWs = [torch.from_numpy(w.copy()).cuda() for w in Ws]
    taus = [torch.zeros((q, Ws[0].shape[1]), dtype=torch.float64, device="cuda") for _ in Ws]
    torch.cuda.synchronize()
    for w, t in zip(dWs, taus):
        up.update(dR, w, t, stream=stream)
        if sync:
            torch.cuda.synchronize()
    return dR, dWs, taus


def host(out):
    dR, dWs, taus = out
    return [dR.cpu().numpy()] + [w.cpu().numpy() for w in dWs] + [t.cpu().numpy() for t in taus]


def test_twenty_updates_without_host_sync(tqr, oracle):
    import torch
    b, q, wt = 32, 3, 2
    R0, Ws = chain_inputs(oracle, b, q, wt, 20, seed=40)
    up = tqr.RowUpdate(q * b, wt * b, b, torch.float64)
    serial = host(run_chain(tqr, tqr.RowUpdate(q * b, wt * b, b, torch.float64), R0, Ws, q, sync=True))
    s = torch.cuda.Stream()
    out = run_chain(tqr, up, R0, Ws, q, stream=s)
    torch.cuda.synchronize()
    assert all(same(a, c) for a, c in zip(host(out), serial))
    assert np.isfinite(serial[0]).all()


def test_two_handles_on_two_streams(tqr, oracle):
    import torch
    b, q, wt = 32, 3, 2
    probs = [chain_inputs(oracle, b, q, wt, 4, seed=60 + 10 * i) for i in range(2)]
    serial = [host(run_chain(tqr, tqr.RowUpdate(q * b, wt * b, b, torch.float64), R0, Ws, q, sync=True)) for R0, Ws in probs]
    ups = [tqr.RowUpdate(q * b, wt * b, b, torch.float64) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [run_chain(tqr, ups[i], *probs[i], q, stream=streams[i]) for i in range(2)]
    torch.cuda.synchronize()
    for o, s in zip(outs, serial):
        assert all(same(a, c) for a, c in zip(host(o), s))


def test_two_threads_share_one_handle(tqr, oracle):
    """Each thread runs its own chain of tqr_update_lstsq calls on its own buffers and stream through one
    shared handle: the calls exclude each other while they enqueue and are ordered on the GPU."""
    import torch
    b, q, wt, nrhs, count = 32, 3, 2, 3, 4
    n, mw = q * b, wt * b
    probs = [chain_inputs(oracle, b, q, wt, count, seed=80 + 10 * i) for i in range(2)]
    Dh = oracle.randzo(n, nrhs, np.float64, seed=95)
    Bh = [oracle.randzo(mw, nrhs, np.float64, seed=96 + i) for i in range(count)]

    def run(up, R0, Ws, stream, out, sync):
        dR = torch.from_numpy(R0.copy()).cuda()
        dD = torch.from_numpy(Dh.copy()).cuda()
        dX = torch.zeros((nrhs, n), dtype=torch.float64, device="cuda")
        dres = torch.zeros(nrhs, dtype=torch.float64, device="cuda")
        keep = []
        torch.cuda.synchronize()
        for w, bn in zip(Ws, Bh):
            dW, dB = torch.from_numpy(w.copy()).cuda(), torch.from_numpy(bn.copy()).cuda()
            tu = torch.zeros((q, mw), dtype=torch.float64, device="cuda")
            torch.cuda.current_stream().synchronize()
            up.lstsq(dR, dW, tu, dD, dB, dX, res=dres, stream=stream)
            keep += [dW, dB, tu]
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out.extend(t.cpu().numpy() for t in [dR, dD, dX, dres] + keep)

    serial = [[], []]
    for i in range(2):
        run(tqr.RowUpdate(n, mw, b, torch.float64), *probs[i], None, serial[i], True)
    shared = tqr.RowUpdate(n, mw, b, torch.float64)
    streams = [torch.cuda.Stream() for _ in range(2)]
    got = [[], []]
    errs = []

    def work(i):
        try:
            run(shared, *probs[i], streams[i], got[i], False)
        except Exception as e:  # surfaced below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for g, s in zip(got, serial):
        assert len(g) == len(s) and all(same(a, c) for a, c in zip(g, s))
