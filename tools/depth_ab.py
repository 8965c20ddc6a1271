"""Alternating A/B of task lists on one GPU: per variant one fp64 b = 256 plan of the same P x Q tile
grid, timed round by round like bench.py (one staged input per timed step), after a check that every
variant leaves A and tau bit-identical to the first one's. Writes the ms per factorisation as JSON.
Usage: python tools/depth_ab.py P[xQ] ROUNDS STEPS OUT.json VARIANT ...
VARIANT: default (the plan as created) | LIST.npy (an (n, 4) int32 task list loaded with
tqr_plan_set_tasks, e.g. from tools/sched_sim.py greedy_order) | env:NAME=VALUE (the plan created with
that variable set, e.g. env:TQR_DEPTH=0)"""
import ctypes, json, os, sys, time
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "gpu-tiled-qr-decomposition_amd"))
import tqr

PQ, R, steps, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
MP, MQ = ([int(x) for x in PQ.split('x')] * 2)[:2]
variants = sys.argv[5:]
b = 256
m, n = MP * b, MQ * b
M = min(MP, MQ)
L = tqr.lib()
A0 = torch.empty((n, m), dtype=torch.float64, device="cuda")
tqr.fill_randzo(A0, m, n, 5)
tau = torch.zeros((M, m), dtype=torch.float64, device="cuda")
As = [A0.clone() for _ in range(steps)]
plans = {}
for v in variants:
    if v.startswith("env:"):
        k, val = v[4:].split("=")
        os.environ[k] = val
        plans[v] = tqr.TiledQR(m, n, b, torch.float64)
        del os.environ[k]
    else:
        plans[v] = tqr.TiledQR(m, n, b, torch.float64)
        if v != "default":
            a = np.ascontiguousarray(np.load(v).astype(np.int32))
            st = L.tqr_plan_set_tasks(plans[v].h, a.ctypes.data_as(ctypes.c_void_p), len(a))
            assert st == 0, (v, st)
stream = torch.cuda.current_stream().cuda_stream
res = {v: [] for v in variants}
ref = None
for v in variants:  # warm-up and bit-exactness
    for _ in range(2):
        As[0].copy_(A0)
        plans[v].execute(As[0], tau, stream=stream)
    torch.cuda.synchronize()
    plans[v].status(stream)
    if ref is None:
        ref = (As[0].clone(), tau.clone())
    else:
        assert torch.equal(ref[0], As[0]) and torch.equal(ref[1], tau), v
        print(f"{v}: bit-identical to {variants[0]}", flush=True)
del ref
for r in range(R):
    for v in variants:
        for a in As:
            a.copy_(A0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            plans[v].execute(As[s], tau, stream=stream)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        plans[v].status(stream)
        res[v].append(round(ms, 3))
        print(f"round {r} {v}: {ms:.3f} ms", flush=True)
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump({"tiles": PQ, "steps": steps, "rounds": R, "ms_per_step": res}, open(out, "w"), indent=1)
print(json.dumps(res))
