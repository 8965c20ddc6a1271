"""Host model of the pipelined apply's schedule: replays the ticket order of
tqr_apply_pipe_q(NOTRANS) and of tqr_apply_pipe_form_q on `ncu` resident workgroups with every tile
operation costing one time unit, a workgroup taking the next ticket when it is free and operation
(k, l) waiting for operation (k + 1, l) of its strip. Prints the makespan of both in tile operations
next to the perfectly balanced one (operations / ncu): what the ticket order and the dependencies
alone cost, before any memory effect. No GPU.
Usage: python tools/form_q_sim.py [m:b[:n] ...]   (default: the shapes of apply_bench.py --formq)"""
import heapq
import sys


def makespan(p, kmax, b, ncols, form, ncu=256):
    nstrips = (ncols + 63) // 64
    items = [(s, k) for k in range(kmax - 1, -1, -1) if not form or k * b <= ncols - 1
             for s in range(k * b // 64 if form else 0, nstrips)]
    done, free, ops = {}, [0.0] * ncu, 0
    for s, k in items:
        t = heapq.heappop(free)
        prod, d = done.get((s, k + 1)), {}
        for l in range(p - 1, k - 1, -1):  # TSMQR(l, k) for l > k, then UNMQR(k)
            if prod is not None:
                t = max(t, prod[max(l, k + 1)])  # (l = k waits for nothing new: flag (k+1, k+1) was seen at l = k+1)
            t += 1.0
            d[l] = t
        ops += p - k
        done[(s, k)] = d
        done.pop((s, k + 2), None)
        heapq.heappush(free, t)
    return max(free), ops


def main(argv):
    shapes = []
    for a in argv or ["4096:128", "16384:256", "65536:256:16384"]:
        m, b, *n = (int(v) for v in a.split(":"))
        shapes.append((m, n[0] if n else m, b))
    for m, n, b in shapes:
        p, kmax, ncols = m // b, min(m, n) // b, min(m, n)
        (ta, oa), (tf, of) = makespan(p, kmax, b, ncols, False), makespan(p, kmax, b, ncols, True)
        print(f"{m} x {n}, b = {b}, ncols = {ncols}: apply {ta:.0f} (balanced {oa / 256:.0f}, {oa} operations), "
              f"form_q {tf:.0f} (balanced {of / 256:.0f}, {of} operations), ratio {tf / ta:.3f} "
              f"(operations {of / oa:.3f})")


if __name__ == "__main__":
    main(sys.argv[1:])
