"""Capped-plan benchmark: what a partial factorisation over [A | B] or [A | I] costs
next to the ordinary factorisation of A and the apply-based calls it replaces. fp64 squares, default
16384^2 b=256 and 4096^2 b=128 ("m:b" arguments for others). Device time from events around the timed
calls only (every run first restores its input, outside the events), best of `reps` after one warm-up
run. One JSON line per shape:
  factor_ms            ordinary plan on A (the yardstick; bench.py's ms_per_step on the same box)
  capped_full_ms       tqr_plan_create_steps with steps = n / b on A: the same list, must time alike
  capped_ab_ms[r]      capped plan on [A | B], B = r tile columns, r = 1 and 4: the whole launch
  lstsq_fused_ms[nrhs] tqr_lstsq_fused, nrhs = 64 and 256 (launch + tqr_trsm_r + residual norms)
  lstsq_apply_ms[nrhs] the existing path on the same data: ordinary execute, tqr_apply_prepare, tqr_lstsq
  qt_capped_ms         capped plan on [A | I] (Q^T explicitly; tqr.form_qt's launch)
  qt_apply_ms          ordinary execute, tqr_apply_prepare, tqr_apply_q(TRANS) on an identity
and the ratios to factor_ms / to the apply-based path, with the model figure (q + r) / q.
Usage: python tools/steps_bench.py [--reps N] [m:b ...]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-tiled-qr-decomposition_amd"))
import tqr  # noqa: E402

from apply_bench import parse  # noqa: E402


def timed(setup, fn, reps):
    """best device time (ms) of fn() over `reps` runs after one warm-up; setup() runs before each,
    outside the timed events"""
    import torch
    setup()
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def main(argv):
    import torch
    reps, _, shapes = parse(argv)
    if not any(":" in a for a in argv):
        shapes = [(16384, 256), (4096, 128)]
    assert torch.cuda.is_available(), "steps_bench.py measures on the GPU only"
    cs = torch.cuda.current_stream()
    f64 = torch.float64
    for m, b in shapes:
        n, q = m, m // b
        rmax = 4
        A0 = torch.empty((n, m), dtype=f64, device="cuda")
        tqr.fill_randzo(A0, m, n, 5)
        B0 = torch.empty((rmax * b, m), dtype=f64, device="cuda")
        tqr.fill_randzo(B0, m, rmax * b, 9)
        W = torch.empty((n + rmax * b, m), dtype=f64, device="cuda")  # [A | B] work array
        tau = torch.zeros((q, m), dtype=f64, device="cuda")
        res = torch.zeros((rmax * b,), dtype=f64, device="cuda")

        def restore():
            W[:n].copy_(A0)
            W[n:].copy_(B0)

        def checked(plan):
            plan.status(cs.cuda_stream)
            return plan

        rec = {"dtype": "f64", "m": m, "n": n, "b": b, "reps": reps}
        plan = tqr.TiledQR(m, n, b, f64)
        rec["factor_ms"] = round(timed(restore, lambda: plan.execute(W, tau, stream=cs.cuda_stream), reps), 3)
        checked(plan)
        full = tqr.TiledQR(m, n, b, f64, steps=q)
        rec["capped_full_ms"] = round(timed(restore, lambda: full.execute(W, tau, stream=cs.cuda_stream), reps), 3)
        checked(full)
        del full
        rec["capped_ab_ms"], rec["capped_ab_ratio"], rec["model_ratio"] = {}, {}, {}
        for r in (1, 4):
            cp = tqr.TiledQR(m, n + r * b, b, f64, steps=q)
            t = timed(restore, lambda: cp.execute(W, tau, stream=cs.cuda_stream), reps)
            checked(cp)
            rec["capped_ab_ms"][r] = round(t, 3)
            rec["capped_ab_ratio"][r] = round(t / rec["factor_ms"], 4)
            rec["model_ratio"][r] = round((q + r) / q, 4)
            del cp
        ap = tqr.ApplyQ(m, n, b, f64)
        rec["lstsq_fused_ms"], rec["lstsq_apply_ms"], rec["lstsq_fused_over_apply"] = {}, {}, {}
        for nrhs in (64, 256):
            r = -(-nrhs // b)
            cp = tqr.TiledQR(m, n + r * b, b, f64, steps=q)
            t_f = timed(restore, lambda: cp.lstsq_fused(W, tau, nrhs, res=res, stream=cs), reps)
            checked(cp)
            del cp

            def apply_path():
                plan.execute(W, tau, stream=cs.cuda_stream)
                ap.prepare(W, tau, ldda=m, stream=cs)
                ap.lstsq(W, W[n:], nrhs=nrhs, ldda=m, lddb=m, res=res, stream=cs)

            t_a = timed(restore, apply_path, reps)
            checked(plan)
            rec["lstsq_fused_ms"][nrhs] = round(t_f, 3)
            rec["lstsq_apply_ms"][nrhs] = round(t_a, 3)
            rec["lstsq_fused_over_apply"][nrhs] = round(t_f / t_a, 4)
        del W, B0, res
        torch.cuda.empty_cache()
        # Q^T: [A | I] in one capped launch against factorise + prepare + apply to an identity
        AI = torch.zeros((n + m, m), dtype=f64, device="cuda")

        def restore_ai():
            AI[:n].copy_(A0)
            AI[n:].zero_()
            AI[n:].fill_diagonal_(1.0)

        cq = tqr.TiledQR(m, n + m, b, f64, steps=q)
        rec["qt_capped_ms"] = round(timed(restore_ai, lambda: cq.execute(AI, tau, stream=cs.cuda_stream), reps), 3)
        checked(cq)
        del cq

        def apply_qt():
            plan.execute(AI, tau, stream=cs.cuda_stream)
            ap.prepare(AI, tau, ldda=m, stream=cs)
            ap.apply(AI, AI[n:], trans=True, ldda=m, lddc=m, stream=cs)

        rec["qt_apply_ms"] = round(timed(restore_ai, apply_qt, reps), 3)
        checked(plan)
        rec["qt_capped_over_apply"] = round(rec["qt_capped_ms"] / rec["qt_apply_ms"], 4)
        rec["qt_capped_over_factor"] = round(rec["qt_capped_ms"] / rec["factor_ms"], 4)
        print(json.dumps(rec), flush=True)
        del AI, A0, tau, ap, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
