"""Multi-element chain segments of the fp64 engine at small shapes: the cases and a coverage function,
shared by test_segments_cpu.py (which regimes each case's task list holds; no GPU) and
test_gpu_segments.py (the engine on those lists).

A chain is one tile column's UNMQR followed by its TSMQRs at one step; the planner cuts it into
segments (csrc/flow_list.hpp: rows k+1 .. p-1 in runs of the chain's segment length, after the
UNMQR-only segment where unmqr_alone), one task per segment and strip. Inside a task each element
hands its head strip to the next and the next element's strip streams in during the last reflector
group: the hand-over. fp64 plans put every step with at most 31 tile rows below the diagonal into
one-element segments (csrc/flowplan.cpp default_tail), so with p <= 32 tile rows no TSMQR follows a
TSMQR inside a task under the default knobs. The cases here are the smallest fp64 shapes, with the
knobs they need, whose lists do hold such tasks; regimes() says which kinds, reading the list alone.

Knobs are read at plan creation: `with knobs(env):` around the creation (and around tqr.flow_list).
"""
import os

import numpy as np

T_CHAIN = 4
REGIMES = ("handover", "full0", "full", "rem1", "lines_handover", "mixed", "la_own", "queued")
MULTI = ("handover", "full0", "full", "rem1")  # what no default-knob list of p <= 32 tile rows holds
DEVICE_GRID = 256  # workgroups of a default launch: one per CU of an MI355X
# every variable that shapes a plan's list, its grid or its chain form: none may leak into a case
KNOBS = ["TQR_DEPTH", "TQR_SEGLEN", "TQR_SEGLEN_LA", "TQR_LA_TAIL", "TQR_TAIL", "TQR_TAIL_SEGLEN", "TQR_UNMQR_ALONE",
         "TQR_LAZY", "TQR_LA", "TQR_LAC", "TQR_TG", "TQR_DIST_DEFAULTS", "TQR_DIST_PART", "TQR_FLOW_SHAPE", "TQR_FLOW_GRID",
         "TQR_CHAIN_ASM", "TQR_UNMQR_SKIP", "TQR_STRIP_LINES", "TQR_ENGINE"]
# every step in the tail, every lookahead UNMQR alone: one TSMQR per task at most (the list the small
# shapes of the other test files run under the default knobs)
ALL_TAIL = {"TQR_TAIL": "64", "TQR_UNMQR_ALONE": "64"}


class knobs:
    """The environment of the plans created inside the block: `env` and no other knob."""

    def __init__(self, env=None):
        self.env = dict(env or {})

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in KNOBS}
        assert set(self.env) <= set(KNOBS), sorted(set(self.env) - set(KNOBS))
        os.environ.update(self.env)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Case:
    def __init__(self, name, shape, env, reach):
        self.name, self.shape, self.env, self.reach = name, shape, dict(env), tuple(reach)
        self.grid = int(env.get("TQR_FLOW_GRID", DEVICE_GRID))

    @property
    def tiles(self):
        m, n, b = self.shape
        return m // b, n // b

    def __repr__(self):
        return self.name


# The smallest fp64 shapes that reach each regime (test_segments_cpu.py asserts `reach`, and that the
# union is every regime). 34 tile rows: the smallest p with a step outside the default tail (steps 0 and
# 1; p = 33 has one). 10 tile rows: UNMQR + 8 TSMQR, then a segment of one. 18: 8 + 8 + 1.
CASES = [
    Case("D64", (2176, 256, 64), {}, ("handover", "full0", "full", "rem1", "mixed")),
    Case("D256", (8704, 1024, 256), {}, ("handover", "full0", "full", "rem1", "mixed", "lines_handover")),
    Case("T0", (2560, 1024, 256), {"TQR_TAIL": "0"}, ("handover", "full0", "rem1", "lines_handover")),
    Case("T0-3seg", (1152, 256, 64), {"TQR_TAIL": "0"}, ("handover", "full0", "full", "rem1")),
    Case("T0-128", (1280, 256, 128), {"TQR_TAIL": "0"}, ("handover", "full0", "rem1")),
    Case("MIX", (2560, 1280, 256), {"TQR_TAIL": "2", "TQR_DEPTH": "2"}, ("handover", "full0", "rem1", "mixed", "lines_handover")),
    Case("SL", (2560, 1024, 256), {"TQR_TAIL": "0", "TQR_SEGLEN": "3", "TQR_SEGLEN_LA": "2"},
         ("handover", "la_own", "lines_handover")),
    Case("WIDE", (1024, 2560, 256), {"TQR_TAIL": "0"}, ("handover", "lines_handover")),
    Case("Q", (2560, 1024, 256), {"TQR_TAIL": "0", "TQR_FLOW_GRID": "6"}, ("handover", "full0", "rem1", "lines_handover", "queued")),
]
BY_NAME = {c.name: c for c in CASES}


def export(tqr, case, env=None, **spec):
    """The host export of the case's device list (tqr.flow_list) under its knobs, or under `env`.
    A launch smaller than the device is not a whole-device rank (flow_list's `full`)."""
    p, q = case.tiles
    env = case.env if env is None else env
    full = 0 if int(env.get("TQR_FLOW_GRID", DEVICE_GRID)) < DEVICE_GRID else 1
    with knobs(env):
        return tqr.flow_list(p, q, case.shape[2], tqr.TQR_F64, full=full, **spec)


def chains(items):
    """{(k, j, strip): [(i0, i1), ...] by segment index} of a list's chain tasks: task e of chain
    (k, j) holds the UNMQR if e = 0 and the TSMQR elements of rows i0 .. i1-1."""
    out = {}
    for ts, l, j, ke in np.asarray(items).tolist():
        if ts & 0xff != T_CHAIN:
            continue
        out.setdefault((ke & 0xffff, j, (ts >> 8) & 0xff), {})[ke >> 16] = (l & 0xffff, l >> 16)
    res = {}
    for key, segs in out.items():
        assert sorted(segs) == list(range(len(segs))), (key, sorted(segs))  # segments 0 .. nseg-1, each once
        res[key] = [segs[e] for e in range(len(segs))]
    return res


def segmentation(p, k, segs):
    """(unmqr_alone, segment length or None) of one chain, derived from its number of tasks and checked
    against flow_list.hpp's arithmetic: rows k+1 .. p-1 in runs of the segment length after the
    UNMQR-only segment. The length is None where one run holds every row (any length >= rows gives it)."""
    rows = p - k - 1
    nseg = len(segs)
    if rows <= 0:
        assert nseg == 1 and segs[0][0] == segs[0][1], (k, segs)
        return False, None
    ua = segs[0][0] == segs[0][1]
    nrun = nseg - (1 if ua else 0)
    assert nrun >= 1, (k, segs)
    first = segs[1 if ua else 0]
    sl = first[1] - first[0] if nrun > 1 else None
    run = sl if sl is not None else rows
    assert run >= 1 and (rows + run - 1) // run == nrun, (k, segs)  # nseg_of_chain
    for e, (i0, i1) in enumerate(segs):
        er = e - (1 if ua else 0)
        want = (k + 1, k + 1) if er < 0 else (k + 1 + er * run, min(p, k + 1 + (er + 1) * run))
        assert (i0, i1) == want, (k, e, (i0, i1), want)
    return ua, sl


def regimes(p, q, b, items, grid=DEVICE_GRID, steps=0, tqr=None):
    """Which of REGIMES the task list `items` of a p x q-tile fp64 plan (tile size b, `steps` steps, 0 =
    all) holds when it runs on `grid` workgroups. Everything is read from the list: the segment sizes
    from the chain tasks per (k, j, strip), whatever knobs produced them. tqr: the module, needed for
    lines_handover at b = 256 (tqr.strip_layout).

    handover        a task with at least 2 TSMQR elements
    full0           a segment 0 holding the UNMQR and 8 TSMQR
    full            a segment >= 1 with 8 TSMQR
    rem1            a last segment of exactly one element after one of several
    lines_handover  b = 256: a TSMQR element that is not its task's first TSMQR, at a step k >= 1 in a
                    column j > k+1, whose strip arrives in the whole-line layout (tqr.strip_layout of the
                    tile at step k-1)
    mixed           a step with multi-element segments and a later step whose chains of 2+ rows are all
                    one element per segment, its lookahead column's UNMQR alone in segment 0
    la_own          a step whose lookahead column (j = k+1) has another segment length than another
                    column of the step (both known: more than one run of rows)
    queued          at least 8 tasks per workgroup
    """
    out = set()
    ch = chains(items)
    bulk_steps, tail_steps = set(), {}
    sl_by_step = {}
    for (k, j, s), segs in sorted(ch.items()):
        ua, sl = segmentation(p, k, segs)
        sizes = [i1 - i0 for i0, i1 in segs]
        if max(sizes) >= 2:
            out.add("handover")
            bulk_steps.add(k)
        if sizes[0] == 8:
            out.add("full0")
        if 8 in sizes[1:]:
            out.add("full")
        if len(sizes) >= 2 and sizes[-1] == 1 and sizes[-2] >= 2:
            out.add("rem1")
        if p - k - 1 >= 2:
            t = tail_steps.setdefault(k, {"one": True, "ua": False})
            t["one"] &= max(sizes) == 1
            t["ua"] |= j == k + 1 and ua
        if sl is not None:
            sl_by_step.setdefault(k, {}).setdefault(j == k + 1, set()).add(sl)
        if b == 256 and k >= 1 and j > k + 1:
            for i0, i1 in segs:
                for i in range(i0 + 1, i1):
                    if tqr.strip_layout(p, q, steps, i, j, k - 1) == 1:
                        out.add("lines_handover")
    tails = [k for k, t in tail_steps.items() if t["one"] and t["ua"]]
    if bulk_steps and tails and min(bulk_steps) < max(tails):
        out.add("mixed")
    for k, d in sl_by_step.items():
        if True in d and False in d and d[True] != d[False]:
            out.add("la_own")
    if len(items) >= 8 * grid:
        out.add("queued")
    return out


# ---- inputs and host references, computed once per shape and read-only ---------------------------
SCALE_CASES = ("D64", "T0", "MIX")          # column scaling, bit-exact covariance
LD_CASES = ("D64", "T0-3seg")               # b = 64: the numpy.longdouble QR takes a few seconds here
FAMILY_CASES_256 = ("T0",)                  # b = 256: residual, column norms, bits of the all-tail plan
CONDITIONED = ("rowgraded", "cond1e8")


def randzo(oracle, shape, seed=5):
    import inputs
    m, n, _ = shape
    return inputs._frozen(("seg-randzo", shape, seed), lambda: oracle.randzo(m, n, np.float64, seed=seed))


def factor_ref(oracle, key, A, b):
    """The oracle's (F, T) of A under a cache key (the threaded oracle: the bits of the serial one,
    every tile operation being the same — test_segments_cpu.py asserts it at one shape)."""
    import inputs
    return inputs._frozen(("seg-F",) + tuple(key), lambda: oracle.factor(A, b, threads=8))


def randzo_ref(oracle, shape, seed=5):
    return factor_ref(oracle, ("randzo", shape, seed), randzo(oracle, shape, seed), shape[2])


def family_ref(oracle, family, shape, offset=0):
    import inputs
    return factor_ref(oracle, (family, shape, offset), inputs.matrix(family, shape, offset=offset), shape[2])


def zero_pivot_input(shape, zero):
    """The shape's gauss matrix with element (0, 0) = zero (+0.0 or -0.0) over a live tail."""
    import inputs
    A = inputs.matrix("gauss", shape).copy()
    A[0, 0] = zero
    assert np.signbit(A[0, 0]) == np.signbit(zero) and np.abs(A[0, 1:]).min() > 0
    return A


def zero_pivot_ref(oracle, shape, zero):
    return factor_ref(oracle, ("zero", shape, bool(np.signbit(zero))), zero_pivot_input(shape, zero), shape[2])
