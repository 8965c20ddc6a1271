"""Tall-skinny QR benchmark: tqr_tsqr_* against the flat tile tree on the same matrix,
in one process, device time from HIP events around each whole call (enqueue included), after one warm-up
run of every method, the methods alternating run by run, every run from the same Gaussian matrix
(restored outside the timed window). Per shape, three kinds of JSON lines:
  factor  TSQR.factor at the default m_dom / fan and each tile size b <= 256 dividing n (from --tsqr-b),
          against tqr_plan_execute on a flow plan at b in {64, 128, 256} dividing n (the baseline: the
          library's path before TSQR) and torch.geqrf. Before timing, |R| of every TSQR run is compared
          with the first flow plan's |R|: max ||R| - |R_flow|| <= tol * max|R|, tol = 1e-11 (fp64) / 1e-4
          (fp32); a miss aborts the tool.
  sweep   TSQR.factor at the fastest b of `factor`, m_dom in {2, 4, 8, 16} n and {1024, 2048, 4096} rows x fan in
          {2, 4, 8, 16}.
  apply   TSQR.apply (Q^T) and TSQR.lstsq at the defaults for nrhs in {1, 64, n}, against
          tqr_apply_pipe_q / tqr_lstsq_pipe on the fastest flow factorisation.
Each method's line carries all run times (`*_runs_ms`), the minimum (`*_ms`) and the spread (max - min)
/ min of the runs. A torch.geqrf whose warm-up takes over --torch-limit seconds is recorded by that run.
Usage: python tools/tsqr_bench.py [--reps N] [--no-torch] [--torch-limit S] [--no-sweep] [--no-apply]
                                  [--tsqr-b a,b,...] [--out FILE] [m:n:f64|f32 ...]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402

DEFAULT_POINTS = [(65536, 256, "f64"), (262144, 128, "f64"), (1048576, 64, "f64"), (262144, 128, "f32")]
DEFAULT_OUT = os.path.join(REPO, "profiles", "tsqr", "tsqr_bench.jsonl")
FLOW_B = [64, 128, 256]


def parse(argv):
    opt = {"reps": 4, "torch": True, "torch_limit": 15.0, "sweep": True, "apply": True, "tsqr_b": [32, 64, 128, 256],
           "out": DEFAULT_OUT, "points": []}
    it = iter(argv)
    for a in it:
        if a == "--reps":
            opt["reps"] = max(4, int(next(it)))
        elif a == "--no-torch":
            opt["torch"] = False
        elif a == "--torch-limit":
            opt["torch_limit"] = float(next(it))
        elif a == "--no-sweep":
            opt["sweep"] = False
        elif a == "--no-apply":
            opt["apply"] = False
        elif a == "--tsqr-b":
            opt["tsqr_b"] = [int(v) for v in next(it).split(",")]
        elif a == "--out":
            opt["out"] = next(it)
        else:
            m, n, dt = a.split(":")
            if dt not in ("f64", "f32"):
                raise SystemExit(f"tsqr_bench: dtype of {a!r} must be f64 or f32")
            opt["points"].append((int(m), int(n), dt))
    opt["points"] = opt["points"] or DEFAULT_POINTS
    return opt


def event_ms(fn):
    """Device time of fn() between two events on the current stream."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(methods, restore, reps):
    """{name: runs} of methods {name: fn}: one warm-up each, then `reps` rounds alternating the methods,
    restore(name) before every run and outside its timed window."""
    import torch
    for name, fn in methods.items():
        restore(name)
        fn()
        torch.cuda.synchronize()
    runs = {name: [] for name in methods}
    for _ in range(reps):
        for name, fn in methods.items():
            restore(name)
            torch.cuda.synchronize()
            runs[name].append(round(event_ms(fn), 4))
    return runs


def put(rec, name, runs):
    rec[f"{name}_runs_ms"] = runs
    rec[f"{name}_ms"] = min(runs)
    rec[f"{name}_spread"] = round((max(runs) - min(runs)) / min(runs), 4)


def abs_r(A, n):
    """|R| (n x n, on the host) of a factorised device matrix (n, m)."""
    return np.abs(np.tril(A[:, :n].cpu().numpy()))


def run_shape(m, n, dt, opt, emit):
    import torch
    tdt = torch.float64 if dt == "f64" else torch.float32
    tol = 1e-11 if dt == "f64" else 1e-4
    gen = torch.Generator(device="cuda").manual_seed(1000 + m + n)
    A0 = torch.randn((n, m), dtype=tdt, device="cuda", generator=gen)
    A = torch.empty_like(A0)

    def restore(_name=None):
        A.copy_(A0)

    # ---- factor -------------------------------------------------------------------------------
    rec = {"kind": "factor", "m": m, "n": n, "dtype": dt, "reps": opt["reps"]}
    methods, flows, tsqrs = {}, {}, {}
    for b in [b for b in FLOW_B if n % b == 0 and m % b == 0]:
        plan = tqr.TiledQR(m, n, b, tdt, engine="flow")
        tau = torch.zeros((n // b, m), dtype=tdt, device="cuda")
        flows[b] = (plan, tau)
        methods[f"flow_b{b}"] = (lambda p=plan, t=tau: p.execute(A, t))
    for b in [b for b in opt["tsqr_b"] if n % b == 0 and m % b == 0]:
        t = tqr.TSQR(m, n, b, tdt, nrhs_max=n)
        tsqrs[b] = t
        methods[f"tsqr_b{b}"] = (lambda t=t: t.factor(A))
    # |R| against the first flow plan's, at the size timed
    b0 = next(iter(flows))
    restore()
    flows[b0][0].execute(A, flows[b0][1])
    flows[b0][0].status()
    R_flow = abs_r(A, n)
    rmax = float(R_flow.max())
    for b, t in tsqrs.items():
        restore()
        t.factor(A)
        torch.cuda.synchronize()
        err = float(np.abs(abs_r(A, n) - R_flow).max())
        rec[f"tsqr_b{b}_absR_err"] = err
        rec[f"tsqr_b{b}_plan"] = {"m_dom": t.m_dom, "fan": t.fan, "domains": t.domains, "workspace_bytes": t.workspace_bytes()}
        if not err <= tol * rmax:
            raise SystemExit(f"tsqr_bench: {m}x{n} {dt} b={b}: ||R| - |R_flow|| = {err:.3e} exceeds {tol} * max|R| = {tol * rmax:.3e}")
    rec["absR_bound"] = tol * rmax
    At0 = At = None
    if opt["torch"]:
        try:
            At0 = A0.t().contiguous()
            At = torch.empty_like(At0)
            At.copy_(At0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.geqrf(At)
            torch.cuda.synchronize()
            warm_s = time.perf_counter() - t0
            if warm_s > opt["torch_limit"]:
                rec["torch_runs_ms"] = [round(warm_s * 1e3, 3)]
                rec["torch_note"] = "first run only (host clock, includes set-up): over the time limit"
            else:
                methods["torch"] = lambda: torch.geqrf(At)
        except Exception as e:  # torch cannot run it here
            rec["torch_runs_ms"] = "unavailable"
            rec["torch_note"] = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
    else:
        rec["torch_runs_ms"] = "not run"

    def restore_f(name):
        if name == "torch":
            At.copy_(At0)
        else:
            A.copy_(A0)

    for name, runs in timed(methods, restore_f, opt["reps"]).items():
        put(rec, name, runs)
    for p, _ in flows.values():
        p.status()
    best_flow = min(flows, key=lambda b: rec[f"flow_b{b}_ms"])
    best_tsqr = min(tsqrs, key=lambda b: rec[f"tsqr_b{b}_ms"])
    rec["best_flow_b"], rec["best_tsqr_b"] = best_flow, best_tsqr
    rec["flow_over_tsqr"] = round(rec[f"flow_b{best_flow}_ms"] / rec[f"tsqr_b{best_tsqr}_ms"], 3)
    if "torch_ms" in rec:
        rec["torch_over_tsqr"] = round(rec["torch_ms"] / rec[f"tsqr_b{best_tsqr}_ms"], 3)
    emit(rec)
    del At, At0, methods
    t_def = tsqrs[best_tsqr]
    tsqrs = None
    torch.cuda.empty_cache()

    # ---- sweep of m_dom x fan at the fastest b ---------------------------------------------------
    if opt["sweep"]:
        b = best_tsqr
        rec = {"kind": "sweep", "m": m, "n": n, "dtype": dt, "b": b, "reps": opt["reps"], "points": []}
        for md in sorted({2 * n, 4 * n, 8 * n, 16 * n, 1024, 2048, 4096}):
            if m % md or md % b or md < n:
                continue
            handles = {f: tqr.TSQR(m, n, b, tdt, m_dom=md, fan=f) for f in (2, 4, 8, 16)}
            runs = timed({f: (lambda t=t: t.factor(A)) for f, t in handles.items()}, restore, opt["reps"])
            for f, r in runs.items():
                rec["points"].append({"m_dom": md, "fan": f, "levels": handles[f].levels, "runs_ms": r, "ms": min(r),
                                      "spread": round((max(r) - min(r)) / min(r), 4)})
            del handles
            torch.cuda.empty_cache()
        best = min(rec["points"], key=lambda p: p["ms"])
        rec["best"] = {k: best[k] for k in ("m_dom", "fan", "ms")}
        rec["default"] = {"m_dom": t_def.m_dom, "fan": t_def.fan}
        emit(rec)

    # ---- apply / lstsq ---------------------------------------------------------------------------
    if opt["apply"]:
        bf = best_flow
        plan, tau = flows[bf]
        Af = A0.clone()
        plan.execute(Af, tau)
        plan.status()
        ap = tqr.ApplyQ(m, n, bf, tdt)
        ap.prepare(Af, tau)
        At_ = A0.clone()
        t_def.factor(At_)
        torch.cuda.synchronize()
        for nrhs in sorted({1, 64, n}):
            rec = {"kind": "apply", "m": m, "n": n, "dtype": dt, "nrhs": nrhs, "tsqr_b": best_tsqr, "flow_b": bf,
                   "reps": opt["reps"]}
            C0 = torch.randn((nrhs, m), dtype=tdt, device="cuda", generator=gen)
            C = torch.empty_like(C0)
            res = torch.empty(nrhs, dtype=tdt, device="cuda")
            pipe = tqr.ApplyPipe(m, n, bf, tdt, nrhs)
            sv = tqr.Solve(n, bf, tdt, nrhs)
            methods = {
                "tsqr_apply": lambda: t_def.apply(At_, C, trans=True),
                "pipe_apply": lambda: ap.apply(Af, C, trans=True, pipe=pipe),
                "tsqr_lstsq": lambda: t_def.lstsq(At_, C, res=res),
                "pipe_lstsq": lambda: ap.lstsq(Af, C, res=res, pipe=pipe, solve=sv),
            }
            # the two solutions agree (both solve the same least-squares problem)
            C.copy_(C0)
            methods["tsqr_lstsq"]()
            X1 = C[:, :n].clone()
            C.copy_(C0)
            methods["pipe_lstsq"]()
            pipe.status()
            sv.status()
            rec["lstsq_x_rel_diff"] = float((torch.linalg.norm(X1 - C[:, :n]) / torch.linalg.norm(X1)).item())
            for name, runs in timed(methods, lambda _n: C.copy_(C0), opt["reps"]).items():
                put(rec, name, runs)
            pipe.status()
            sv.status()
            rec["pipe_over_tsqr_apply"] = round(rec["pipe_apply_ms"] / rec["tsqr_apply_ms"], 3)
            rec["pipe_over_tsqr_lstsq"] = round(rec["pipe_lstsq_ms"] / rec["tsqr_lstsq_ms"], 3)
            emit(rec)
            del pipe, sv, C, C0
            torch.cuda.empty_cache()


def main(argv):
    import torch
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsqr_bench: needs a GPU (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for m, n, dt in opt["points"]:
            run_shape(m, n, dt, opt, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
