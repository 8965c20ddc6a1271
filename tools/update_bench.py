"""Row-update benchmark: append mw rows to the R of a finished n-column factorisation,
timed in one process against the two alternatives the library offers without tqr_update_*:
  update      tqr_update_rows (RowUpdate.update) on R and W;
  apply64     tqr_update_apply_q (TQR_TRANS) on 64 columns, after that update;
  lstsq       tqr_update_lstsq with 64 right-hand sides (update + apply + copy + solve + norms);
  flow_full   a flow plan on the stacked (n + mw) x n matrix [G; W] from scratch;
  wave_dense  a wave plan on the dense (n + mw) x n matrix [R; W] (R's triangle, zeros below): what
              tqr_tsqr_* does to its triangle stacks — GEQRT on tiles that are triangular already and
              TSQRT / TSMQR on every zero tile below the block diagonal.
Device time from HIP events around each whole call (enqueue included: that is what a caller waits for),
after one warm-up run of every method, the methods alternating run by run; every run starts from the same
operands, restored before the timed window. G and W are Gaussian; R comes from a flow plan on G.
Before timing, R' of `update` is compared with wave_dense's (up to the sign of each row: wave_dense's
GEQRTs flip signs) and the Gram relation R'^T R' = R^T R + W^T W is checked on 64 random vectors.
One JSON line per point: all run times of each method (`*_runs_ms`), their minima, the schedule
(levels, items, launches), the workspace and the ratios flow_full / update and wave_dense / update.
Default points: fp64 n = 16384, b = 256, mw = 256, 1024, 4096; fp32 the same n, b with mw = 1024.
Usage: python tools/update_bench.py [--reps N] [--no-wave] [--out FILE] [n:mw:b:f64|f32 ...]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402

DEFAULT_POINTS = [(16384, 256, 256, "f64"), (16384, 1024, 256, "f64"), (16384, 4096, 256, "f64"), (16384, 1024, 256, "f32")]
DEFAULT_OUT = os.path.join(REPO, "profiles", "update", "update_bench.jsonl")
NRHS = 64


def parse(argv):
    opt = {"reps": 3, "wave": True, "out": DEFAULT_OUT, "points": []}
    it = iter(argv)
    for a in it:
        if a == "--reps":
            opt["reps"] = int(next(it))
        elif a == "--no-wave":
            opt["wave"] = False
        elif a == "--out":
            opt["out"] = next(it)
        else:
            n, mw, b, dt = a.split(":")
            if dt not in ("f64", "f32"):
                raise SystemExit(f"update_bench: dtype of {a!r} must be f64 or f32")
            opt["points"].append((int(n), int(mw), int(b), dt))
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


def run_point(n, mw, b, dt, opt):
    import torch
    tdt = torch.float64 if dt == "f64" else torch.float32
    q, m = n // b, n + mw
    gen = torch.Generator(device="cuda").manual_seed(1000 + n + mw + b)
    S0 = torch.randn((n, m), dtype=tdt, device="cuda", generator=gen)  # column-major (n + mw) x n: [G; W]
    W0 = S0[:, n:].contiguous()
    # R of G by a flow plan on G alone
    R0 = S0[:, :n].contiguous()
    tauG = torch.zeros((q, n), dtype=tdt, device="cuda")
    pG = tqr.TiledQR(n, n, b, tdt, engine="flow")
    pG.execute(R0, tauG)
    pG.status()
    del pG, tauG
    D0 = torch.randn((NRHS, n), dtype=tdt, device="cuda", generator=gen)
    B0 = torch.randn((NRHS, mw), dtype=tdt, device="cuda", generator=gen)

    R, W = torch.empty_like(R0), torch.empty_like(W0)
    tauU = torch.zeros((q, mw), dtype=tdt, device="cuda")
    D, Bn, X = torch.empty_like(D0), torch.empty_like(B0), torch.empty_like(D0)
    res = torch.zeros(NRHS, dtype=tdt, device="cuda")
    S = torch.empty_like(S0)
    tauS = torch.zeros((q, m), dtype=tdt, device="cuda")
    up = tqr.RowUpdate(n, mw, b, tdt)
    flow = tqr.TiledQR(m, n, b, tdt, engine="flow")
    wave = tqr.TiledQR(m, n, b, tdt, engine="waves") if opt["wave"] else None
    nlevels, npanel, nupdate, nlaunch = tqr.update_plan(n, mw, b)
    rec = {"n": n, "mw": mw, "b": b, "dtype": dt, "nrhs": NRHS, "nlevels": nlevels, "npanel": npanel, "nupdate": nupdate,
           "nlaunch": nlaunch, "workspace_bytes": up.workspace_bytes(), "reps": opt["reps"]}

    def restore_rw():
        R.copy_(R0)
        W.copy_(W0)

    def restore_lstsq():
        restore_rw()
        D.copy_(D0)
        Bn.copy_(B0)
        res.zero_()

    def restore_full():
        S.copy_(S0)

    def restore_dense():
        S[:, :n].copy_(torch.tril(R0))  # array[j, i], i <= j: the upper triangle
        S[:, n:].copy_(W0)

    def restore_apply():
        D.copy_(D0)
        Bn.copy_(B0)

    methods = {
        "update": (restore_rw, lambda: up.update(R, W, tauU)),
        "lstsq": (restore_lstsq, lambda: up.lstsq(R, W, tauU, D, Bn, X, res=res)),
        "flow_full": (restore_full, lambda: flow.execute(S, tauS)),
    }
    if wave is not None:
        methods["wave_dense"] = (restore_dense, lambda: wave.execute(S, tauS))

    # warm-up runs, and the checks at the size timed
    for name, (restore, fn) in methods.items():
        restore()
        fn()
        torch.cuda.synchronize()
        if name == "wave_dense":
            Rw = torch.tril(S[:, :n]).clone()
    flow.status()
    restore_rw()
    up.update(R, W, tauU)
    torch.cuda.synchronize()
    Ru = torch.tril(R)
    if wave is not None:
        wave.status()
        d = (Ru.abs() - Rw.abs()).abs().max().item()
        rec["max_abs_diff_vs_wave_dense_up_to_sign"] = d
        del Rw
    Z = torch.randn((n, NRHS), dtype=torch.float64, device="cuda", generator=gen)
    # array Ru[j, i] = R'(i, j): R' z = Ru^T z; W z = W0^T z
    lhs = (Ru.double().T @ Z).square().sum(0)
    rhs = (torch.tril(R0).double().T @ Z).square().sum(0) + (W0.double().T @ Z).square().sum(0)
    rec["gram_rel_err_on_64_vectors"] = ((lhs - rhs).abs() / rhs).max().item()
    del Z, lhs, rhs, Ru
    # apply64: the handle holds the update just made
    methods["apply64"] = (restore_apply, lambda: up.apply(W, D, Bn, trans=True))
    restore_apply()
    up.apply(W, D, Bn, trans=True)
    torch.cuda.synchronize()

    runs = {name: [] for name in methods}
    order = ["update", "apply64", "lstsq", "flow_full"] + (["wave_dense"] if wave is not None else [])
    for _ in range(opt["reps"]):
        for name in order:  # alternating: a drift of the machine hits every method alike
            restore, fn = methods[name]
            if name == "apply64":  # needs W = the V of an update: redo it outside the timed window
                restore_rw()
                up.update(R, W, tauU)
            restore()
            torch.cuda.synchronize()
            runs[name].append(round(event_ms(fn), 4))
    flow.status()
    if wave is not None:
        wave.status()
    for name in order:
        rec[f"{name}_runs_ms"] = runs[name]
        rec[f"{name}_ms"] = min(runs[name])
    for name in ("flow_full", "wave_dense"):
        if f"{name}_ms" in rec:
            rec[f"{name}_over_update"] = round(rec[f"{name}_ms"] / rec["update_ms"], 3)
    return rec


def main(argv):
    import torch
    opt = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("update_bench: needs a GPU (nothing is measured without one)")
    os.makedirs(os.path.dirname(os.path.abspath(opt["out"])), exist_ok=True)
    with open(opt["out"], "w") as f:
        for n, mw, b, dt in opt["points"]:
            rec = run_point(n, mw, b, dt, opt)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
