"""A numpy / oracle model of the row update (include/tqr.h "row update"): the update of R by appended
rows W from the oracle's tile kernels on a stacked array, the apply of its Q_u reflector by reflector,
and a brute-force dependency graph of the update's tile operations for the schedule checks.

Arrays follow the module convention of tqr.py: a column-major r x c matrix is an array of shape (c, r),
so array[j, i] is element (i, j) and the upper triangle i <= j of a square block is numpy's tril.
"""
import ctypes

import numpy as np

QRD, DAPP = 2, 3  # the oracle's task types (oracle.h)

# (b, q, wt) of the CPU checks
CPU_SHAPES = [(16, 4, 2), (32, 3, 1), (32, 3, 2), (64, 2, 3), (128, 2, 1)]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def update(oracle, Rarr, W, b):
    """The update of the R in Rarr (>= n, >= n; only elements (i, j), i <= j < n, are used) by the rows W
    (n, mw): oracle_do_task QRD / DAPP on the W rows of the stacked [R; W], in the order of the header.
    Returns (Rnew, V, tau_u): Rnew a copy of Rarr with the upper triangle of the leading block replaced,
    V (n, mw) the TSQRT V tiles, tau_u (q, mw) with tau_u[k, l*b + c] the tau of column c of TSQRT(., W_lk)."""
    n, mw = W.shape
    q, wt, m = n // b, mw // b, n + mw
    dt = W.dtype
    S = np.zeros((n, m), dtype=dt)
    S[:, :n] = Rarr[:n, :n]
    S[:, n:] = W
    lower = ~np.tril(np.ones((n, n), dtype=bool))  # elements (i, j) with i > j
    S[:, :n][lower] = np.nan                       # whatever lies below the diagonal must not matter
    T = np.zeros((n, m), dtype=dt)
    w = np.zeros(2 * b, dtype=dt)
    fn = getattr(oracle.L, f"oracle_do_task_{oracle.sfx(dt)}")
    for k in range(q):
        for l in range(wt):
            fn(QRD, q + l, k, k, _ptr(S), _ptr(T), b, m, _ptr(w))
            for j in range(k + 1, q):
                fn(DAPP, q + l, j, k, _ptr(S), _ptr(T), b, m, _ptr(w))
    Rnew = np.array(Rarr)
    blk = Rnew[:n, :n]
    blk[~lower] = S[:, :n][~lower]
    tau_u = np.ascontiguousarray(T[0::b, n:])
    return Rnew, np.ascontiguousarray(S[:, n:]), tau_u


def reflectors(V, tau_u, b):
    """[(rows, v, tau)] of Q_u on the stacked [Ctop; Cnew] in the update's order (k ascending, l ascending,
    column c), in the form of inputs.reflectors: rows = the head row and the b rows of W tile l, v = [1; v_B]."""
    n, mw = V.shape
    out = []
    for k in range(n // b):
        for l in range(mw // b):
            for c in range(b):
                d = k * b + c
                rows = np.concatenate(([d], np.arange(n + l * b, n + (l + 1) * b)))
                v = np.concatenate(([1.0], V[d, l * b:(l + 1) * b])).astype(V.dtype)
                out.append((rows, v, tau_u[k, l * b + c]))
    return out


def apply(V, tau_u, Ctop, Cnew, b, trans=True):
    """(Ctop (nrhs, n), Cnew (nrhs, mw)) <- Q_u^T (trans) or Q_u of the pair: the reflectors I - tau v v^T one
    by one in the arrays' own precision, with the arithmetic of inputs.numpy_qt / inputs.numpy_q."""
    n = Ctop.shape[1]
    C = np.concatenate([Ctop, Cnew], axis=1)
    refl = reflectors(V, tau_u, b)
    for rows, v, tau in (refl if trans else reversed(refl)):
        w = C[:, rows] @ v
        C[:, rows] -= np.outer(tau * w, v)
    return np.ascontiguousarray(C[:, :n]), np.ascontiguousarray(C[:, n:])


# ---- the schedule --------------------------------------------------------------------------------
def serial_tasks(q, wt, nstrips):
    """The update's tile operations in the serial order of the header, as (type, strip, l, j, k): a TSQRT
    is one task, a TSMQR one task per 64-column strip."""
    out = []
    for k in range(q):
        for l in range(wt):
            out.append((QRD, 0, l, k, k))
            for j in range(k + 1, q):
                for s in range(nstrips):
                    out.append((DAPP, s, l, j, k))
    return out


def accesses(task, nstrips):
    """(reads, writes) of a task as sets of resources: ("R" | "W", tile row, tile column, strip) for the
    64-column strips of a tile, ("T", l, k) for the taus and the T images of TSQRT(l, k)."""
    ty, s, l, j, k = task
    if ty == QRD:
        wr = {("R", k, k, x) for x in range(nstrips)} | {("W", l, k, x) for x in range(nstrips)} | {("T", l, k)}
        return set(wr), wr  # read-modify-write of both tiles
    rd = {("W", l, k, x) for x in range(nstrips)} | {("T", l, k)}
    wr = {("R", k, j, s), ("W", l, j, s)}
    return rd | wr, wr


def brute_force_deps(tasks, nstrips):
    """Every ordered pair (a, b), a before b in the serial order, that touch a common resource with at
    least one of them writing it: b depends on a. Found per resource over all earlier accesses."""
    hist = {}
    deps = set()
    for b_idx, t in enumerate(tasks):
        rd, wr = accesses(t, nstrips)
        for r in rd | wr:
            for a_idx, a_writes in hist.get(r, ()):
                if a_writes or r in wr:
                    deps.add((a_idx, b_idx))
            hist.setdefault(r, []).append((b_idx, r in wr))
    return deps
