"""Batched-factorisation benchmark: `batch` same-shape matrices factorised four ways in
one process, device time from HIP events around each whole call sequence (enqueue included: that is what
a caller waits for), after one warm-up run of every method, the methods alternating run by run:
  batched    one tqr_batch_execute (BatchedQR);
  wave_loop  a loop of tqr_plan_execute over the members on ONE wave plan (the same workgroups as
             `batched`, in batch times the launches);
  flow_loop  the same loop on one flow plan (the default engine: one persistent launch per matrix);
  torch      torch.geqrf on the same batch as a (batch, m, n) tensor, "unavailable" where torch refuses.
The loops run from Python through ctypes with every pointer prepared beforehand; a plan's executes are
serialised by contract, so a loop over one plan is serial on the device however it is driven.
Every run starts from the same Gaussian matrices (restored before the timed window). Before timing, the
batched result is compared with the wave loop's, byte for byte, at the size timed.
One JSON line per (shape, dtype, batch): all run times of each method (`*_runs_ms`), their minima, the
batch handle's group / groups / launches, and the ratios wave_loop / batched, flow_loop / batched, torch /
batched of the minima. Default points: 256^2 b=32, 512^2 b=64, 1024^2 b=128, 4096x256 b=128 in fp64 and 512^2
b=64 in fp32, batches 1, 16, 64, 256, 1024. A torch.geqrf whose warm-up run takes over --torch-limit seconds
(default 15) is timed by that one run only (host clock, marked in `torch_note`).
Usage: python tools/batch_bench.py [--reps N] [--no-torch] [--torch-limit S] [--batches a,b,...]
                                   [--out FILE] [m:n:b:f64|f32 ...]"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402

DEFAULT_POINTS = [(256, 256, 32, "f64"), (512, 512, 64, "f64"), (1024, 1024, 128, "f64"), (4096, 256, 128, "f64"),
                  (512, 512, 64, "f32")]
DEFAULT_BATCHES = [1, 16, 64, 256, 1024]
DEFAULT_OUT = os.path.join(REPO, "profiles", "batch", "batch_bench.jsonl")


def parse(argv):
    opt = {"reps": 5, "torch": True, "torch_limit": 15.0, "batches": DEFAULT_BATCHES, "out": DEFAULT_OUT, "points": []}
    it = iter(argv)
    for a in it:
        if a == "--reps":
            opt["reps"] = int(next(it))
        elif a == "--no-torch":
            opt["torch"] = False
        elif a == "--torch-limit":
            opt["torch_limit"] = float(next(it))
        elif a == "--batches":
            opt["batches"] = [int(v) for v in next(it).split(",")]
        elif a == "--out":
            opt["out"] = next(it)
        else:
            m, n, b, dt = a.split(":")
            if dt not in ("f64", "f32"):
                raise SystemExit(f"batch_bench: dtype of {a!r} must be f64 or f32")
            opt["points"].append((int(m), int(n), int(b), dt))
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


def plan_loop(plan, A, tau, batch):
    """fn() that runs tqr_plan_execute on each member of contiguous A (batch, n, m), tau (batch, kmax, m)."""
    L, P = tqr.lib(), ctypes.c_void_p
    m, h = plan.m, plan.h
    args = [(P(A[i].data_ptr()), P(tau[i].data_ptr())) for i in range(batch)]
    execute = L.tqr_plan_execute

    def fn():
        for pa, pt in args:
            st = execute(h, pa, m, pt, None)
            if st != 0:
                tqr.check(st, "tqr_plan_execute")
    return fn


def run_point(m, n, b, dt, batch, opt):
    import torch
    tdt = torch.float64 if dt == "f64" else torch.float32
    kmax = min(m, n) // b
    gen = torch.Generator(device="cuda").manual_seed(1000 + m + n + b + batch)
    A0 = torch.randn((batch, n, m), dtype=tdt, device="cuda", generator=gen)
    A = torch.empty_like(A0)
    tau = torch.zeros((batch, kmax, m), dtype=tdt, device="cuda")
    bq = tqr.BatchedQR(m, n, b, tdt, batch)
    group, ngroups, nlaunch = tqr.batch_plan(m, n, b, tdt, batch)
    assert group == bq.group()
    waves = tqr.TiledQR(m, n, b, tdt, engine="waves")
    flow = tqr.TiledQR(m, n, b, tdt, engine="flow")
    methods = {
        "batched": lambda: bq.execute(A, tau),
        "wave_loop": plan_loop(waves, A, tau, batch),
        "flow_loop": plan_loop(flow, A, tau, batch),
    }
    rec = {"m": m, "n": n, "b": b, "dtype": dt, "batch": batch, "group": group, "ngroups": ngroups, "nlaunch": nlaunch,
           "nlaunch_wave_loop": batch * (nlaunch // ngroups), "workspace_bytes": bq.workspace_bytes(), "reps": opt["reps"]}

    # results at the size timed: the batched call against the wave loop, in bytes (also the warm-up runs)
    out = {}
    for name, fn in methods.items():
        A.copy_(A0)
        tau.zero_()
        fn()
        torch.cuda.synchronize()
        if name != "flow_loop":
            out[name] = (A.clone(), tau.clone())
    flow.status()
    rec["batched_equals_wave_loop_bytes"] = bool(
        torch.equal(out["batched"][0].view(torch.uint8), out["wave_loop"][0].view(torch.uint8)) and
        torch.equal(out["batched"][1].view(torch.uint8), out["wave_loop"][1].view(torch.uint8)))
    del out

    # torch.geqrf on the batch as torch lays it out: (batch, m, n), the same matrices
    At0 = At = None
    if opt["torch"]:
        try:
            At0 = A0.transpose(1, 2).contiguous()
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

    runs = {name: [] for name in methods}
    for _ in range(opt["reps"]):
        for name, fn in methods.items():  # alternating: a drift of the machine hits every method alike
            if name == "torch":
                At.copy_(At0)
            else:
                A.copy_(A0)
            runs[name].append(round(event_ms(fn), 4))
    flow.status()
    for name, r in runs.items():
        rec[f"{name}_runs_ms"] = r
    for name in ("batched", "wave_loop", "flow_loop", "torch"):
        r = rec.get(f"{name}_runs_ms")
        if isinstance(r, list):
            rec[f"{name}_ms"] = min(r)
    for name in ("wave_loop", "flow_loop", "torch"):
        if f"{name}_ms" in rec:
            rec[f"{name}_over_batched"] = round(rec[f"{name}_ms"] / rec["batched_ms"], 3)
    return rec


def main(argv):
    import torch
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench: needs a GPU (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        for m, n, b, dt in opt["points"]:
            for batch in opt["batches"]:
                rec = run_point(m, n, b, dt, batch, opt)
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
