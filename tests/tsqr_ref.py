"""A numpy model of the tall-skinny QR tree (include/tqr.h "tall-skinny"): the levels, the triangular
gathers with their zero padding, the final R scatter and the apply walks in both directions. The
per-domain factorisation and apply are plugged in (a backend), so the same tree runs on the oracle's
tile kernels (the CPU twin, OracleBackend) and on the library's existing public per-member GPU calls
(GpuMemberBackend: tqr.BatchedQR on the row-interleaved layout, tqr.ApplyQ through offset pointers).

Arrays follow the module convention of tqr.py: a column-major r x c matrix is an array of shape (c, r),
so array[j, i] is element (i, j) and the upper triangle i <= j of a square block is numpy's tril.

A backend has
    factor(W, rows, ndom)          -> (F, aux): W (n, ndom * rows) holds ndom row domains of `rows` rows;
                                      F the same array factorised per domain, aux whatever apply needs
    apply(F, aux, C, rows, ndom, trans) -> C (nrhs, ndom * rows) with Q^T (trans) or Q of every domain
                                      applied to that domain's rows
"""
import numpy as np


def resolve(m, n, b, m_dom=0, fan=0):
    """The defaults of tqr_tsqr_spec re-derived: fan 0 -> 4; m_dom 0 -> the smallest multiple of b that
    divides m and is >= max(4 n, 1024), or m if there is none."""
    fan = fan or 4
    if m_dom == 0:
        m_dom = m
        d = -(-max(4 * n, 1024) // b) * b
        while d < m:
            if m % d == 0:
                m_dom = d
                break
            d += b
    return m_dom, fan


def levels_of(m, n, m_dom, fan):
    """[(domain rows, domains)] per level: level 0 the row blocks of A, then stacks of fan R factors."""
    out = [(m_dom, m // m_dom)]
    while out[-1][1] > 1:
        out.append((fan * n, -(-out[-1][1] // fan)))
    return out


def gather_tri(Fprev, prev_rows, prev_nd, n, rows, nd):
    """W_l: block j = the upper triangle of the top n x n of domain j of the level below, zeros below the
    diagonal; blocks beyond prev_nd are zero."""
    W = np.zeros((n, nd * rows), dtype=Fprev.dtype)
    for j in range(prev_nd):
        W[:, j * n:(j + 1) * n] = np.tril(Fprev[:, j * prev_rows:j * prev_rows + n])
    return W


def gather_rows(Cprev, prev_rows, prev_nd, n, rows, nd):
    """C_l: block j = the top n rows of domain j of the level below; padding zero."""
    C = np.zeros((Cprev.shape[0], nd * rows), dtype=Cprev.dtype)
    for j in range(prev_nd):
        C[:, j * n:(j + 1) * n] = Cprev[:, j * prev_rows:j * prev_rows + n]
    return C


def scatter_rows(Cl, Cprev, prev_rows, prev_nd, n):
    for j in range(prev_nd):
        Cprev[:, j * prev_rows:j * prev_rows + n] = Cl[:, j * n:(j + 1) * n]


def factor(A, b, m_dom, fan, be):
    """The tree on A (n, m). Returns dict(A=the matrix as tqr_tsqr_factor leaves it, lv=[per level
    dict(W=the level's input (level 0: A), F, aux, rows, ndom)])."""
    n, m = A.shape
    lv = []
    for l, (rows, nd) in enumerate(levels_of(m, n, m_dom, fan)):
        W = A if l == 0 else gather_tri(lv[-1]["F"], lv[-1]["rows"], lv[-1]["ndom"], n, rows, nd)
        F, aux = be.factor(W, rows, nd)
        lv.append(dict(W=W, F=F, aux=aux, rows=rows, ndom=nd))
    out = lv[0]["F"].copy()
    if len(lv) > 1:
        mask = np.tril(np.ones((n, n), dtype=bool))
        out[:, :n][mask] = lv[-1]["F"][:, :n][mask]
    return dict(A=out, lv=lv)


def apply(fac, C, trans, be):
    """C (nrhs, m) -> (Q^T C (trans) or Q C, [C_l of every level as the walk left them])."""
    lv = fac["lv"]
    n = lv[0]["F"].shape[0]
    L = len(lv)

    def level_apply(l, X):
        return be.apply(lv[l]["F"], lv[l]["aux"], X, lv[l]["rows"], lv[l]["ndom"], trans)

    def up(l, X):
        return gather_rows(X, lv[l - 1]["rows"], lv[l - 1]["ndom"], n, lv[l]["rows"], lv[l]["ndom"])

    Cs = [np.array(C)]
    if trans:
        Cs[0] = level_apply(0, Cs[0])
        for l in range(1, L):
            Cs.append(level_apply(l, up(l, Cs[l - 1])))
        for l in range(L - 1, 0, -1):
            scatter_rows(Cs[l], Cs[l - 1], lv[l - 1]["rows"], lv[l - 1]["ndom"], n)
    else:
        for l in range(1, L):
            Cs.append(up(l, Cs[l - 1]))
        for l in range(L - 1, 0, -1):
            Cs[l] = level_apply(l, Cs[l])
            scatter_rows(Cs[l], Cs[l - 1], lv[l - 1]["rows"], lv[l - 1]["ndom"], n)
        Cs[0] = level_apply(0, Cs[0])
    return Cs[0], Cs


def form_q(fac, be):
    """The thin Q as an (n, m) array: Q applied to [I_n; 0]."""
    n, m = fac["A"].shape
    E = np.zeros((n, m), dtype=fac["A"].dtype)
    E[np.arange(n), np.arange(n)] = 1
    return apply(fac, E, False, be)[0]


class OracleBackend:
    """Per domain the oracle's factorisation; Q^T by its tile kernels (inputs.oracle_qt), Q by the stored
    reflectors one by one (inputs.numpy_q)."""

    def __init__(self, oracle, b):
        self.oracle, self.b = oracle, b

    def factor(self, W, rows, ndom):
        F = np.empty_like(W)
        Ts = []
        for i in range(ndom):
            Fi, Ti = self.oracle.factor(np.ascontiguousarray(W[:, i * rows:(i + 1) * rows]), self.b)
            F[:, i * rows:(i + 1) * rows] = Fi
            Ts.append(Ti)
        return F, Ts

    def apply(self, F, Ts, C, rows, ndom, trans):
        import inputs
        out = np.array(C)
        for i in range(ndom):
            s = slice(i * rows, (i + 1) * rows)
            Fi, Ci = np.ascontiguousarray(F[:, s]), np.ascontiguousarray(C[:, s])
            out[:, s] = inputs.oracle_qt(self.oracle, Fi, Ts[i], Ci, self.b) if trans else inputs.numpy_q(Fi, Ts[i], Ci, self.b)
        return out


class GpuMemberBackend:
    """The library's existing public per-member calls: tqr.BatchedQR on the level's row-interleaved
    layout, and per domain a tqr.ApplyQ prepared and applied through offset pointers."""

    def __init__(self, tqr, b):
        self.tqr, self.b = tqr, b

    def factor(self, W, rows, ndom):
        import torch
        n, ld = W.shape
        kmax = n // self.b
        dW = torch.from_numpy(np.array(W, order="C")).cuda()
        tau = torch.full((ndom, kmax, rows), float("nan"), dtype=dW.dtype, device="cuda")
        torch.cuda.synchronize()
        self.tqr.BatchedQR(rows, n, self.b, dW.dtype, ndom).execute(dW, tau, ldda=ld, strideA=rows)
        torch.cuda.synchronize()
        return dW.cpu().numpy(), tau.cpu().numpy()

    def apply(self, F, tau, C, rows, ndom, trans):
        import torch
        n, ld = F.shape
        dF = torch.from_numpy(np.array(F, order="C")).cuda()
        dT = torch.from_numpy(np.array(tau, order="C")).cuda()
        dC = torch.from_numpy(np.array(C, order="C")).cuda()
        ap = self.tqr.ApplyQ(rows, n, self.b, dF.dtype)
        torch.cuda.synchronize()
        for i in range(ndom):
            Fi, Ci = dF.view(-1)[i * rows:], dC.view(-1)[i * rows:]
            ap.prepare(Fi, dT[i], ldda=ld)
            ap.apply(Fi, Ci, trans=trans, nrhs=C.shape[0], ldda=ld, lddc=ld)
        torch.cuda.synchronize()
        return dC.cpu().numpy()
