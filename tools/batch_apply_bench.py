"""Batched least-squares benchmark: `batch` same-shape factorisations (one BatchedQR
execute, not timed) solved against nrhs right-hand sides each, three ways in one process. Device time
from HIP events around each whole call sequence (enqueue included: that is what a caller waits for),
after one warm-up run of every method, the methods alternating run by run; the minimum of --reps runs
(default 4) is reported with the spread (max - min) / min and every run time:
  batched  one tqr_batch_lstsq (BatchedApply.lstsq, TQR_NOTRANS, with dres); its tqr_batch_apply_prepare
           is timed separately (`batched_prepare_*`);
  loop     a loop of tqr_lstsq over `batch` tqr_apply handles, each prepared on its member (the loop of
           tqr_apply_prepare is timed separately, `loop_prepare_*`) — three launches per member;
  torch    torch.linalg.lstsq on the unfactorised (batch, m, n) and (batch, m, nrhs) tensors: the whole
           factor-plus-solve problem, so it is compared with factor + prepare + batched. Recorded, not
           required: "unavailable" where torch refuses; a warm-up run over --torch-limit seconds (default 3)
           is recorded alone (host clock) and larger batches of that shape are not run.
The loops run from Python through ctypes with every pointer prepared beforehand. Every run starts from
the same right-hand sides (restored before the timed window). Before timing, B and dres of the batched
call are compared with the loop's, byte for byte, at the size timed; a difference ends the run.
One JSON line per (shape, dtype, batch, nrhs). Default points: 256^2 b=32, 512^2 b=64, 1024^2 b=128,
4096x256 b=128 in fp64 and 512^2 b=64 in fp32, batches 1, 16, 64, 256, 1024, nrhs 1 and 64.
Usage: python tools/batch_apply_bench.py [--reps N] [--no-torch] [--torch-limit S] [--batches a,b,...]
                                         [--nrhs a,b,...] [--out FILE] [m:n:b:f64|f32 ...]"""
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402

DEFAULT_POINTS = [(256, 256, 32, "f64"), (512, 512, 64, "f64"), (1024, 1024, 128, "f64"), (4096, 256, 128, "f64"),
                  (512, 512, 64, "f32")]
DEFAULT_BATCHES = [1, 16, 64, 256, 1024]
DEFAULT_NRHS = [1, 64]
DEFAULT_OUT = os.path.join(REPO, "profiles", "batch", "batch_apply_bench.jsonl")


def parse(argv):
    opt = {"reps": 4, "torch": True, "torch_limit": 3.0, "batches": DEFAULT_BATCHES, "nrhs": DEFAULT_NRHS,
           "out": DEFAULT_OUT, "points": []}
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
        elif a == "--nrhs":
            opt["nrhs"] = [int(v) for v in next(it).split(",")]
        elif a == "--out":
            opt["out"] = next(it)
        else:
            m, n, b, dt = a.split(":")
            if dt not in ("f64", "f32"):
                raise SystemExit(f"batch_apply_bench: dtype of {a!r} must be f64 or f32")
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


def member_loops(aps, A, tau, B, res, nrhs):
    """(prepare(), lstsq()): tqr_apply_prepare / tqr_lstsq on each member of contiguous A (batch, n, m), tau
    (batch, kmax, m), B (batch, nrhs, m), res (batch, nrhs), member i on handle aps[i]."""
    L, P = tqr.lib(), ctypes.c_void_p
    m = A.shape[-1]
    args = [(ap.h, P(A[i].data_ptr()), P(tau[i].data_ptr()), P(B[i].data_ptr()), P(res[i].data_ptr()))
            for i, ap in enumerate(aps)]
    f_prepare, f_lstsq = L.tqr_apply_prepare, L.tqr_lstsq

    def prepare():
        for h, pa, pt, _, _ in args:
            st = f_prepare(h, pa, m, pt, None)
            if st != 0:
                tqr.check(st, "tqr_apply_prepare")

    def lstsq():
        for h, pa, _, pb, pr in args:
            st = f_lstsq(h, 0, pa, m, pb, nrhs, m, pr, None)
            if st != 0:
                tqr.check(st, "tqr_lstsq")
    return prepare, lstsq


def stats(rec, name, runs):
    rec[f"{name}_runs_ms"] = runs
    rec[f"{name}_ms"] = min(runs)
    rec[f"{name}_spread"] = round((max(runs) - min(runs)) / min(runs), 3)


def run_point(m, n, b, dt, batch, nrhs, opt, torch_off):
    import torch
    tdt = torch.float64 if dt == "f64" else torch.float32
    kmax = min(m, n) // b
    gen = torch.Generator(device="cuda").manual_seed(1000 + m + n + b + batch + nrhs)
    A0 = torch.randn((batch, n, m), dtype=tdt, device="cuda", generator=gen)
    B0 = torch.randn((batch, nrhs, m), dtype=tdt, device="cuda", generator=gen)
    A, B = A0.clone(), torch.empty_like(B0)
    tau = torch.zeros((batch, kmax, m), dtype=tdt, device="cuda")
    res = torch.empty((batch, nrhs), dtype=tdt, device="cuda")
    bq = tqr.BatchedQR(m, n, b, tdt, batch)
    ba = tqr.BatchedApply(m, n, b, tdt, batch)
    aps = [tqr.ApplyQ(m, n, b, tdt) for _ in range(batch)]
    rec = {"m": m, "n": n, "b": b, "dtype": dt, "batch": batch, "nrhs": nrhs, "reps": opt["reps"],
           "workspace_bytes": ba.workspace_bytes(), "nlaunch_batched": 3 * ((batch + 65534) // 65535), "nlaunch_loop": 3 * batch}
    rec["factor_ms"] = round(event_ms(lambda: bq.execute(A, tau)), 4)  # (one run, for the torch comparison)
    loop_prepare, loop_lstsq = member_loops(aps, A, tau, B, res, nrhs)
    methods = {
        "batched_prepare": lambda: ba.prepare(A, tau),
        "batched": lambda: ba.lstsq(A, B, res=res),
        "loop_prepare": loop_prepare,
        "loop": loop_lstsq,
    }

    # results at the size timed: the batched call against the loop, in bytes (also the warm-up runs)
    out = {}
    for name, fn in methods.items():
        B.copy_(B0)
        res.fill_(-1.0)
        fn()
        torch.cuda.synchronize()
        if name in ("batched", "loop"):
            out[name] = (B.clone(), res.clone())
    same = bool(torch.equal(out["batched"][0].view(torch.uint8), out["loop"][0].view(torch.uint8)) and
                torch.equal(out["batched"][1].view(torch.uint8), out["loop"][1].view(torch.uint8)))
    rec["batched_equals_loop_bytes"] = same
    del out
    if not same:
        raise SystemExit(f"batch_apply_bench: the batched call and the loop differ in bytes at {rec}")

    # torch.linalg.lstsq on the problem as torch lays it out: (batch, m, n) and (batch, m, nrhs)
    At = Bt = None
    key = (m, n, b, dt)
    if not opt["torch"]:
        rec["torch_runs_ms"] = "not run"
    elif key in torch_off:
        rec["torch_runs_ms"] = "not run"
        rec["torch_note"] = f"batch {torch_off[key]} of this shape was over the time limit"
    else:
        try:
            At, Bt = A0.transpose(1, 2).contiguous(), B0.transpose(1, 2).contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.linalg.lstsq(At, Bt)
            torch.cuda.synchronize()
            warm_s = time.perf_counter() - t0
            if warm_s > opt["torch_limit"]:
                rec["torch_runs_ms"] = [round(warm_s * 1e3, 3)]
                rec["torch_note"] = "first run only (host clock, includes set-up): over the time limit"
                torch_off[key] = batch
            else:
                methods["torch"] = lambda: torch.linalg.lstsq(At, Bt)
        except Exception as e:  # torch cannot run it here
            rec["torch_runs_ms"] = "unavailable"
            rec["torch_note"] = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"

    runs = {name: [] for name in methods}
    for _ in range(opt["reps"]):
        for name, fn in methods.items():  # alternating: a drift of the machine hits every method alike
            if name in ("batched", "loop"):
                B.copy_(B0)
            runs[name].append(round(event_ms(fn), 4))
    for name, r in runs.items():
        stats(rec, name, r)
    rec["loop_over_batched"] = round(rec["loop_ms"] / rec["batched_ms"], 3)
    rec["loop_prepare_over_batched_prepare"] = round(rec["loop_prepare_ms"] / rec["batched_prepare_ms"], 3)
    if "torch_ms" in rec:
        rec["torch_over_factor_prepare_batched"] = round(
            rec["torch_ms"] / (rec["factor_ms"] + rec["batched_prepare_ms"] + rec["batched_ms"]), 3)
    return rec


def main(argv):
    import torch
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("batch_apply_bench: needs a GPU (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    torch_off = {}
    with open(opt["out"], "w") as f:
        for m, n, b, dt in opt["points"]:
            for batch in opt["batches"]:
                for nrhs in opt["nrhs"]:
                    rec = run_point(m, n, b, dt, batch, nrhs, opt, torch_off)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    f.write(line + "\n")
                    f.flush()
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
