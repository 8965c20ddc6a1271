"""Solve benchmark: tqr_trsm_r in both directions and tqr_lstsq (NOTRANS, split into
apply / solve / residual) on a GPU factorisation, device time from events after a warm-up, best of
`reps` runs. Cases: fp64 4096^2 b=128 and 16384^2 b=256, nrhs in {64, n} (or "m:b" arguments for other
squares). One JSON line per case. A solve counts n^2 nrhs flop.
Yardsticks on the same data, from the same process:
  (a) torch.tril + torch.linalg.solve_triangular — what tqr.lstsq does for its triangular solve —
      timed separately and together, with the bytes of the n x n temporary tril makes;
  (b) the existing tqr.lstsq (handle creation, prepare, apply, tril and solve per call).
Pipelined solve: every case also times tqr_solve_trsm_r (tqr.Solve) in both directions
in the same run, with all `reps` timings of both kernels (`*_runs_ms`, restore copy subtracted) so the
run-to-run spread can be read next to the difference; and per shape one "fused" record,
tqr_lstsq_fused against tqr_lstsq_fused_solve on [A | B] with 64 right-hand sides (the restore copy of
the whole [A | B] subtracted). Crossover measured on an MI355X (fp64): the pipelined call is 13.6 x
faster at 16384^2, b = 256, nrhs = 64 (9.26 against 125.8 ms) and still 2.7 x faster with 64 strips
(4096^2, nrhs = n), but 13 % slower with 256 strips (16384^2, nrhs = n: 153.8 against 136.2 ms), where
the strips alone put two workgroups on every CU. Use it while the strips are fewer than the CUs (nrhs
below about 64 x 256), tqr_trsm_r beyond; the crossover was not measured more finely.
--solve-only skips the apply / lstsq split and the yardsticks (the two solves and the fused pair only).
Usage: python tools/solve_bench.py [--reps N] [--no-torch] [--solve-only] [m:b ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402

from apply_bench import parse, timed  # noqa: E402


def torch_yardstick(A, X, n, reps):
    """tril, solve_triangular and both, on the factorised A (n, m) and right-hand sides X (nrhs, >= n)."""
    import torch
    try:
        Y = X[:, :n].contiguous()
        t_tril = timed(lambda: torch.tril(A[:, :n]), reps)
        Rt = torch.tril(A[:, :n])
        tmp = Rt.numel() * Rt.element_size()
        t_solve = timed(lambda: torch.linalg.solve_triangular(Rt, Y, upper=False, left=False), reps)
        del Rt
        t_both = timed(lambda: torch.linalg.solve_triangular(torch.tril(A[:, :n]), Y, upper=False, left=False), reps)
        return {"tril_ms": round(t_tril, 3), "solve_triangular_ms": round(t_solve, 3), "tril_and_solve_ms": round(t_both, 3),
                "tril_temporary_bytes": tmp}
    except Exception as e:
        return f"unavailable ({type(e).__name__})"


def timed_runs(fn, reps):
    """device times (ms) of `reps` runs of fn() after one warm-up run, in run order"""
    return [timed(fn, 1) if r == 0 else timed_once(fn) for r in range(reps)]


def timed_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def fused_record(m, b, nrhs, reps):
    """tqr_lstsq_fused and tqr_lstsq_fused_solve on the same [A | B] (n = m, one tile column of B)."""
    import torch
    n = m
    AB0 = torch.empty((n + b, m), dtype=torch.float64, device="cuda")
    tqr.fill_randzo(AB0, m, n + b, 5)
    AB = AB0.clone()
    tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
    res = torch.zeros((nrhs,), dtype=torch.float64, device="cuda")
    plan = tqr.TiledQR(m, n + b, b, torch.float64, steps=n // b)
    sv = tqr.Solve(n, b, torch.float64, nrhs)
    cs = torch.cuda.current_stream()

    def run(solve):
        def go():
            AB.copy_(AB0)
            plan.lstsq_fused(AB, tau, nrhs, res=res, stream=cs, solve=solve)
        return go

    t_copy = timed(lambda: AB.copy_(AB0), reps)
    r0 = [round(t - t_copy, 3) for t in timed_runs(run(None), reps)]
    r1 = [round(t - t_copy, 3) for t in timed_runs(run(sv), reps)]
    plan.status()
    sv.status()
    return {"record": "fused", "dtype": "f64", "m": m, "n": n, "b": b, "nrhs": nrhs, "copy_ms": round(t_copy, 3),
            "lstsq_fused_ms": min(r0), "lstsq_fused_runs_ms": r0,
            "lstsq_fused_solve_ms": min(r1), "lstsq_fused_solve_runs_ms": r1}


def main(argv):
    import torch
    solve_only = "--solve-only" in argv
    reps, use_torch, shapes = parse([a for a in argv if a != "--solve-only"])
    assert torch.cuda.is_available(), "solve_bench.py measures on the GPU only"
    cs = torch.cuda.current_stream()
    for m, b in shapes:
        n = m
        A = torch.empty((n, m), dtype=torch.float64, device="cuda")
        tau = torch.zeros((n // b, m), dtype=torch.float64, device="cuda")
        tqr.fill_randzo(A, m, n, 5)
        plan = tqr.TiledQR(m, n, b, torch.float64)
        plan.execute(A, tau)
        plan.status()
        ap = None
        if not solve_only:
            ap = tqr.ApplyQ(m, n, b, torch.float64)
            ap.prepare(A, tau, stream=cs)
        sv = tqr.Solve(n, b, torch.float64, n)
        for nrhs in (64, n):
            # the solves run in place on their own output again and again: a random X stays bounded
            # only if R is well conditioned, so every timed call starts from the same right-hand side
            X0 = torch.empty((nrhs, m), dtype=torch.float64, device="cuda")
            tqr.fill_randzo(X0, m, nrhs, 9)
            X = X0.clone()
            res = torch.zeros((nrhs,), dtype=torch.float64, device="cuda")

            def fresh(fn):
                def run():
                    X.copy_(X0)
                    fn()
                return run

            t_copy = timed(lambda: X.copy_(X0), reps)
            runs = {}
            for name, trans, solve in (("trsm_r", False, None), ("trsm_rt", True, None),
                                       ("trsm_r_pipe", False, sv), ("trsm_rt_pipe", True, sv)):
                ts = timed_runs(fresh(lambda: tqr.trsm_r(A, X, b, trans=trans, stream=cs, solve=solve)), reps)
                runs[name] = [round(t - t_copy, 3) for t in ts]
            sv.status(cs)
            t_r, t_rt = min(runs["trsm_r"]), min(runs["trsm_rt"])
            fl = float(n) * n * nrhs
            pipe = {"trsm_r_pipe_ms": min(runs["trsm_r_pipe"]), "trsm_rt_pipe_ms": min(runs["trsm_rt_pipe"]),
                    "gflops_r_pipe": round(fl / min(runs["trsm_r_pipe"]) / 1e6, 1),
                    "gflops_rt_pipe": round(fl / min(runs["trsm_rt_pipe"]) / 1e6, 1),
                    **{k + "_runs_ms": v for k, v in runs.items()}}
            if solve_only:
                print(json.dumps({"dtype": "f64", "m": m, "n": n, "b": b, "nrhs": nrhs, "copy_ms": round(t_copy, 3),
                                  "trsm_r_ms": round(t_r, 3), "trsm_rt_ms": round(t_rt, 3), **pipe}), flush=True)
                del X, X0, res
                continue
            t_apply = timed(fresh(lambda: ap.apply(A, X, trans=True, stream=cs)), reps) - t_copy
            t_ls = timed(fresh(lambda: ap.lstsq(A, X, stream=cs)), reps) - t_copy
            t_lsr = timed(fresh(lambda: ap.lstsq(A, X, res=res, stream=cs)), reps) - t_copy
            rec = {"dtype": "f64", "m": m, "n": n, "b": b, "nrhs": nrhs, "copy_ms": round(t_copy, 3),
                   "trsm_r_ms": round(t_r, 3), "trsm_rt_ms": round(t_rt, 3),
                   "gflops_r": round(fl / t_r / 1e6, 1), "gflops_rt": round(fl / t_rt / 1e6, 1),
                   "lstsq_ms": round(t_lsr, 3), "lstsq_apply_ms": round(t_apply, 3),
                   "lstsq_solve_ms": round(t_ls - t_apply, 3), "lstsq_residual_ms": round(t_lsr - t_ls, 3), **pipe}
            if use_torch:
                rec["yardstick_torch"] = torch_yardstick(A, X0, n, max(1, reps - 1))
                try:
                    rec["yardstick_tqr_lstsq_ms"] = round(timed(fresh(lambda: tqr.lstsq(A, tau, X, b)), max(1, reps - 1)) - t_copy, 3)
                except Exception as e:
                    rec["yardstick_tqr_lstsq_ms"] = f"unavailable ({type(e).__name__})"
            else:
                rec["yardstick_torch"] = rec["yardstick_tqr_lstsq_ms"] = "skipped"
            print(json.dumps(rec), flush=True)
            del X, X0, res
        del ap, sv, plan, A, tau
        torch.cuda.empty_cache()
        print(json.dumps(fused_record(m, b, 64, reps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
