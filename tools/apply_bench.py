"""Apply benchmark: tqr_apply_prepare and tqr_apply_q (both directions) on a GPU
factorisation, device time from events after a warm-up, best of `reps` runs.
Cases: fp64 4096^2 b=128 and 16384^2 b=256, nrhs in {64, n} (or "m:b" arguments for other squares).
One JSON line per case. An apply counts 4 b^2 nrhs flop per TSMQR tile and 2 b^2 nrhs per UNMQR tile.
Two yardsticks from the same process:
  (a) tqr_tile_batch DAPP — the same inner loop in one launch of independent blocks, launch and V
      traffic at their best — with as many b-column blocks as the apply has TSMQR tile updates (capped
      by the batch's 32-bit device matrix), reported per block;
  (b) torch.geqrf + torch.ormqr (Q^T C) on the same shape, "unavailable" if torch cannot run them here.
Pipelined apply: --pipe times, per shape and nrhs (--nrhs a,b,...; default 64),
tqr_apply_q against tqr_apply_pipe_q in both directions and tqr_lstsq against tqr_lstsq_pipe (least
squares with residual norms, and the minimum-norm direction) in the same run, with all `reps` timings of
every call (`*_runs_ms`) so the run-to-run spread can be read next to the difference, and the model
(p + 2 kmax) / (stored tiles) x the tqr_apply_q time of the same run next to the measured time. Nothing
else is timed in that mode. Crossover measured on an MI355X (fp64, 16384^2, b = 256): none up to nrhs = n —
the pipelined call is 26.5 x faster at nrhs = 64 (15.7 against 416.9 ms), 17 x at 1024, 5.4 x at 4096 and
still 1.49 x at 16384 columns (282.8 against 422.7 ms), where tqr_apply_q has exactly one workgroup per CU.
Beyond nrhs = n it was not measured: tqr_apply_q then runs two workgroups per CU, which the pipelined kernel
cannot, so a crossover may lie there.
Form Q: --formq times, per shape with ncols = min(m, n), tqr_apply_pipe_form_q against what it
replaces — the fill of an explicit m x ncols identity, tqr_apply_pipe_q(NOTRANS) on it and tqr_apply_q on it —
alternating the calls run by run, with all timings (`*_runs_ms`), the tile-operation counts of both item sets,
and whether the two results have the same values and the same bytes at this size. A shape "m:b:n" is a tall
m x n factorisation (--formq only). Nothing else is timed in that mode.
Usage: python tools/apply_bench.py [--reps N] [--no-torch] [--pipe [--nrhs a,b,...]] [--formq] [m:b ...]"""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402


PIPE = {"on": False, "nrhs": [64]}  # --pipe / --nrhs (parse is shared with tools/solve_bench.py)
FORMQ = {"on": False, "n": {}}  # --formq; n of the shapes given as m:b:n


def parse(argv):
    reps, use_torch, shapes = 3, True, []
    it = iter(argv)
    for a in it:
        if a == "--reps":
            reps = int(next(it))
        elif a == "--pipe":
            PIPE["on"] = True
        elif a == "--nrhs":
            PIPE["nrhs"] = [int(v) for v in next(it).split(",")]
        elif a == "--formq":
            FORMQ["on"] = True
        elif a == "--no-torch":
            use_torch = False
        else:
            m, b, *n = a.split(":")
            shapes.append((int(m), int(b)))
            if n:
                FORMQ["n"][shapes[-1]] = int(n[0])
    return reps, use_torch, shapes or [(4096, 128), (16384, 256)]


def tile_counts(m, n, b):
    """(TSMQR tiles, UNMQR tiles) one column block of C passes through."""
    p, kmax = m // b, min(m, n) // b
    return sum(p - k - 1 for k in range(kmax)), kmax


def apply_flops(m, n, b, nrhs):
    ts, ge = tile_counts(m, n, b)
    return (4.0 * ts + 2.0 * ge) * b * b * nrhs


def timed(fn, reps, warm=True):
    """best device time (ms) of fn() over `reps` runs after one warm-up run"""
    import torch
    if warm:
        fn()
        torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def timed_all(fn, reps):
    """device times (ms) of `reps` runs of fn() after one warm-up run, in run order"""
    import torch
    fn()
    torch.cuda.synchronize()
    return [round(timed(fn, 1, warm=False), 3) for _ in range(reps)]


def pipe_records(m, b, nrhs_list, reps):
    """tqr_apply_q / tqr_apply_pipe_q and tqr_lstsq / tqr_lstsq_pipe on one fp64 m x m factorisation."""
    import torch
    n = m
    cs = torch.cuda.current_stream()
    A = torch.empty((n, m), dtype=torch.float64, device="cuda")
    tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
    tqr.fill_randzo(A, m, n, 5)
    plan = tqr.TiledQR(m, n, b, torch.float64)
    plan.execute(A, tau)
    plan.status()
    ap = tqr.ApplyQ(m, n, b, torch.float64)
    ap.prepare(A, tau, stream=cs)
    p = kmax = m // b
    tiles = kmax * p - kmax * (kmax - 1) // 2
    for nrhs in nrhs_list:
        pp = tqr.ApplyPipe(m, n, b, torch.float64, nrhs)
        sv = tqr.Solve(n, b, torch.float64, nrhs)
        C = torch.empty((nrhs, m), dtype=torch.float64, device="cuda")
        tqr.fill_randzo(C, m, nrhs, 9)
        # the two calls on the same input, at this size: the same bytes (both directions, one after the other)
        C1 = C.clone()
        for trans in (True, False):
            ap.apply(A, C, trans=trans, stream=cs)
            ap.apply(A, C1, trans=trans, stream=cs, pipe=pp)
        pp.status(cs)
        same = bool(torch.equal(C.view(torch.int64), C1.view(torch.int64)))
        del C1
        runs = {}
        for name, trans, pipe in (("apply_qt", True, None), ("apply_qt_pipe", True, pp),
                                  ("apply_q", False, None), ("apply_q_pipe", False, pp)):
            runs[name] = timed_all(lambda: ap.apply(A, C, trans=trans, stream=cs, pipe=pipe), reps)
        # the solves run in place: every timed least-squares call starts from the same right-hand side
        X0 = C.clone()
        tqr.fill_randzo(X0, m, nrhs, 9)
        res = torch.zeros((nrhs,), dtype=torch.float64, device="cuda")
        t_copy = timed(lambda: C.copy_(X0), reps)

        def ls(trans, piped):
            def run():
                C.copy_(X0)
                if piped:
                    ap.lstsq(A, C, trans=trans, res=res, stream=cs, pipe=pp, solve=sv)
                else:
                    ap.lstsq(A, C, trans=trans, res=res, stream=cs)
            return run

        for name, trans, piped in (("lstsq", False, False), ("lstsq_pipe", False, True),
                                   ("lstsq_t", True, False), ("lstsq_t_pipe", True, True)):
            runs[name] = [round(t - t_copy, 3) for t in timed_all(ls(trans, piped), reps)]
        pp.status(cs)
        sv.status(cs)
        best = {k: min(v) for k, v in runs.items()}
        rec = {"record": "pipe", "dtype": "f64", "m": m, "n": n, "b": b, "nrhs": nrhs, "copy_ms": round(t_copy, 3),
               "stored_tiles": tiles, "path_tiles": p + 2 * kmax, "bytes_equal": same,
               **{k + "_ms": v for k, v in best.items()},
               "model_qt_pipe_ms": round(best["apply_qt"] * (p + 2 * kmax) / tiles, 3),
               "model_q_pipe_ms": round(best["apply_q"] * (p + 2 * kmax) / tiles, 3),
               **{k + "_runs_ms": v for k, v in runs.items()},
               "spread_max_ms": round(max(max(v) - min(v) for v in runs.values()), 3)}
        print(json.dumps(rec), flush=True)
        del pp, sv, C, X0, res
        torch.cuda.empty_cache()


def form_q_records(m, n, b, reps):
    """tqr_apply_pipe_form_q against the fill of an identity + tqr_apply_pipe_q / tqr_apply_q on it, fp64."""
    import torch
    cs = torch.cuda.current_stream()
    A = torch.empty((n, m), dtype=torch.float64, device="cuda")
    tau = torch.zeros((min(m, n) // b, m), dtype=torch.float64, device="cuda")
    tqr.fill_randzo(A, m, n, 5)
    plan = tqr.TiledQR(m, n, b, torch.float64)
    plan.execute(A, tau)
    plan.status()
    ap = tqr.ApplyQ(m, n, b, torch.float64)
    ap.prepare(A, tau, stream=cs)
    del plan
    p, kmax, ncols = m // b, min(m, n) // b, min(m, n)
    nstrips = (ncols + 63) // 64
    ops_full = nstrips * sum(p - k for k in range(kmax))
    ops_form = sum((p - k) * (nstrips - k * b // 64) for k in range(kmax) if k * b <= ncols - 1)
    pp = tqr.ApplyPipe(m, n, b, torch.float64, ncols)
    Q = torch.full((ncols, m), float("nan"), dtype=torch.float64, device="cuda")
    E = torch.empty((ncols, m), dtype=torch.float64, device="cuda")

    def fill():
        E.zero_()
        E.fill_diagonal_(1.0)

    calls = {"form_q": lambda: pp.form_q(ap, A, Q, stream=cs), "fill_identity": fill,
             "apply_q_pipe_on_identity": lambda: ap.apply(A, E, trans=False, stream=cs, pipe=pp),
             "apply_q_on_identity": lambda: ap.apply(A, E, trans=False, stream=cs)}
    # the two results at this size (E holds the identity once more for every timed apply: the time of an
    # apply does not depend on the values, but inf must not build up over the repetitions)
    fill()
    calls["form_q"]()
    calls["apply_q_pipe_on_identity"]()
    pp.status(cs)
    same_values = bool(torch.equal(Q, E))
    same_bytes = bool(torch.equal(Q.view(torch.int64), E.view(torch.int64)))
    runs = {k: [] for k in calls}
    order = ["form_q", "fill_identity", "apply_q_pipe_on_identity", "fill_identity", "apply_q_on_identity", "fill_identity"]
    for name in order[:5]:  # warm-up: every call once
        calls[name]()
    torch.cuda.synchronize()
    for _ in range(reps):  # alternating, so that drift hits every call alike
        for name in order:
            runs[name].append(round(timed(calls[name], 1, warm=False), 3))
    pp.status(cs)
    best = {k: min(v) for k, v in runs.items()}
    rec = {"record": "formq", "dtype": "f64", "m": m, "n": n, "b": b, "ncols": ncols,
           "items_form_q": tqr.apply_pipe_form_q_items(kmax, b, ncols), "items_apply_pipe": nstrips * kmax,
           "tile_ops_form_q": ops_form, "tile_ops_apply": ops_full, "tile_ops_ratio": round(ops_form / ops_full, 4),
           "values_equal": same_values, "bytes_equal": same_bytes,
           **{k + "_ms": v for k, v in best.items()},
           "form_q_over_fill_plus_pipe": round(best["form_q"] / (best["fill_identity"] + best["apply_q_pipe_on_identity"]), 4),
           **{k + "_runs_ms": v for k, v in runs.items()}}
    print(json.dumps(rec), flush=True)
    del pp, ap, Q, E, A, tau
    torch.cuda.empty_cache()


def dapp_yardstick(b, want, reps):
    """(us per block, blocks) of one tqr_tile_batch DAPP launch of min(want, what fits) blocks."""
    L = tqr.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rng = np.random.default_rng(5)
    V = (rng.uniform(-0.5, 0.5, (b, b)) / np.sqrt(b)).astype(np.float64)
    tau = 2.0 / (1.0 + (V * V).sum(axis=1))  # orthogonal reflectors [e_j; V column j] (V[col, row])
    blk = rng.uniform(-1, 1, (b, 2 * b))
    nb = max(1, min(want, (0x7fffffff // (8 * 2 * b * b)) - 1))
    ms, best = ctypes.c_float(), None
    for rep in range(reps + 1):
        rc = L.tqr_tile_batch(tqr.TQR_F64, tqr.DAPP, b, nb, vp(V), b, vp(tau), vp(blk), 2 * b, None, 0, ctypes.byref(ms))
        if rc != 0:
            return None, nb
        if rep > 0:  # (run 0 is the warm-up)
            best = ms.value if best is None else min(best, ms.value)
    return best * 1e3 / nb, nb


def torch_yardstick(m, n, nrhs, reps):
    import torch
    try:
        A = (torch.randint(0, 201, (m, n), device="cuda", dtype=torch.float64) - 100.0) / 100.0
        C = torch.randn((m, nrhs), device="cuda", dtype=torch.float64)
        fac = {}

        def geqrf():
            fac["a"], fac["tau"] = torch.geqrf(A)

        t_f = timed(geqrf, reps)
        t_o = timed(lambda: torch.ormqr(fac["a"], fac["tau"], C, left=True, transpose=True), reps)
        return {"geqrf_ms": round(t_f, 3), "ormqr_qt_ms": round(t_o, 3)}
    except Exception as e:  # no rocSOLVER path for this call on this build
        return f"unavailable ({type(e).__name__})"


def main(argv):
    import torch
    reps, use_torch, shapes = parse(argv)
    assert torch.cuda.is_available(), "apply_bench.py measures on the GPU only"
    cs = torch.cuda.current_stream()
    if FORMQ["on"]:
        for m, b in shapes:
            form_q_records(m, FORMQ["n"].get((m, b), m), b, reps)
        return
    if PIPE["on"]:
        for m, b in shapes:
            pipe_records(m, b, PIPE["nrhs"], reps)
        return
    for m, b in shapes:
        n = m
        A = torch.empty((n, m), dtype=torch.float64, device="cuda")
        tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
        tqr.fill_randzo(A, m, n, 5)
        plan = tqr.TiledQR(m, n, b, torch.float64)
        plan.execute(A, tau)
        plan.status()
        ap = tqr.ApplyQ(m, n, b, torch.float64)
        t_prep = timed(lambda: ap.prepare(A, tau, stream=cs), reps)
        ts, ge = tile_counts(m, n, b)
        for nrhs in (64, n):
            C = torch.empty((nrhs, m), dtype=torch.float64, device="cuda")
            tqr.fill_randzo(C, m, nrhs, 9)
            t_qt = timed(lambda: ap.apply(A, C, trans=True, stream=cs), reps)
            t_q = timed(lambda: ap.apply(A, C, trans=False, stream=cs), reps)
            fl = apply_flops(m, n, b, nrhs)
            nupd = ts * ((nrhs + b - 1) // b)  # TSMQR tile updates in b-column blocks
            y_us, y_nb = dapp_yardstick(b, nupd, reps)
            rec = {"dtype": "f64", "m": m, "n": n, "b": b, "nrhs": nrhs,
                   "workspace_bytes": ap.workspace_bytes(), "prepare_ms": round(t_prep, 3),
                   "apply_qt_ms": round(t_qt, 3), "apply_q_ms": round(t_q, 3),
                   "gflops_qt": round(fl / t_qt / 1e6, 1), "gflops_q": round(fl / t_q / 1e6, 1),
                   "tsmqr_updates": nupd, "us_per_tsmqr_update_qt": round(t_qt * 1e3 / nupd, 3),
                   "us_per_tsmqr_update_q": round(t_q * 1e3 / nupd, 3),
                   "yardstick_dapp_us_per_block": None if y_us is None else round(y_us, 3),
                   "yardstick_dapp_blocks": y_nb,
                   "yardstick_torch": torch_yardstick(m, n, nrhs, max(1, reps - 1)) if use_torch else "skipped"}
            print(json.dumps(rec), flush=True)
            del C
        del ap, plan, A, tau
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
