"""Python host mirror of the MI355X tiled QR (libtqr.so) — thin ctypes bindings.

The product is the C ABI in include/{tqr,gridscheduler,gpucalc,qrdecomp}.h; this module only
binds it (for tests, bench.py and __graft_entry__), mirroring the reference's interface
(taskQRP_threads / cudaQRTask / SGEQRF ... / the gridscheduler API, reference qrdecomp.h,
include/gpucalc.h, include/gridscheduler.h). There is no Python or CPU compute path here:
every factorisation call goes to the HIP kernels, and loading fails loudly if libtqr.so is
missing.

Array convention: a column-major m x n matrix is a numpy/torch array of shape (n, m)
(row j = column j), so ldm = m and element (i, j) is A[j, i] — the reference's
CO(i,j,ldm) = j*ldm + i.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# TQR_LIB: a diagnostic build of the same library (e.g. libtqr_fst.so, activity stamps) by file name
LIB_PATH = os.path.join(HERE, os.environ.get("TQR_LIB", "libtqr.so"))

TQR_F32, TQR_F64 = 0, 1
QRS, SAPP, QRD, DAPP = 0, 1, 2, 3
TASK_AVAIL, TASK_NONE, TASK_DONE = 0, 1, 2
READY, DOING, DONE, NONE, NOTASKS = 0, 1, 2, 3, 4

_lib = None
_P = ctypes.c_void_p
_I = ctypes.c_int


class TQRError(RuntimeError):
    pass


class Task(ctypes.Structure):
    """reference include/gridscheduler.h:13-17"""
    _fields_ = [("taskType", _I), ("l", _I), ("m", _I), ("k", _I), ("taskStatus", _I)]


class Plan(ctypes.Structure):
    """tqr_plan_t, include/gridscheduler.h"""
    _fields_ = [("M", _I), ("N", _I), ("nlevels", _I), ("ntasks", ctypes.c_long),
                ("tasks", ctypes.POINTER(_I)), ("level_off", ctypes.POINTER(ctypes.c_long))]


class TsqrSpec(ctypes.Structure):
    """tqr_tsqr_spec, include/tqr.h"""
    _fields_ = [(f, _I) for f in ("m", "n", "b", "dtype", "m_dom", "fan", "nrhs_max")] + [("ws_limit", ctypes.c_size_t)]


def lib():
    """Load libtqr.so (raises if it was not built: no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels dlopen their own bundled libamdhip64.so.7 by path; if libtqr.so were
    # loaded first, the process would hold two HIP runtimes and torch would see no GPU. Loading
    # torch first makes libtqr.so bind (by soname) to the one runtime torch already holds.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise TQRError(f"{LIB_PATH} is missing — build it with __graft_entry__.build() "
                       "(make -C gpu-tiled-qr-decomposition_amd)")
    L = ctypes.CDLL(LIB_PATH)
    L.tqr_strerror.restype = ctypes.c_char_p
    L.tqr_version.restype = ctypes.c_char_p
    L.tqr_total_tasks.restype = ctypes.c_long
    L.tqr_sched_total_tasks.restype = ctypes.c_long
    L.initScheduler.restype = ctypes.POINTER(Task)
    L.tqr_plan_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I]
    L.tqr_plan_create_steps.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I, _I]
    L.tqr_plan_create_steps.restype = _I
    L.tqr_plan_create_engine.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I, _I]
    L.tqr_plan_create_engine.restype = _I
    L.tqr_plan_info.argtypes = [_P, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]
    L.tqr_plan_info.restype = _I
    L.tqr_plan_set_tasks.argtypes = [_P, _P, _I]
    L.tqr_plan_set_tasks.restype = _I
    if hasattr(L, "tqr_plan_get_tasks"):  # (TQR_LIB may name a build from before the call existed)
        L.tqr_plan_get_tasks.argtypes = [_P, _P, _I]
        L.tqr_plan_get_tasks.restype = _I
    if hasattr(L, "tqr_flow_strip_layout"):
        L.tqr_flow_strip_layout.argtypes = [_I] * 6
        L.tqr_flow_strip_layout.restype = _I
        L.tqr_flow_strip_offset.argtypes = [_I, _I, _I, ctypes.c_long]
        L.tqr_flow_strip_offset.restype = ctypes.c_long
    L.tqr_plan_debug_workspace.argtypes = [_P, _I, _P, ctypes.c_size_t]
    L.tqr_plan_debug_workspace.restype = _I
    L.cudaQRFull.argtypes = [_P, _I, _I]
    L.cudaQRFull.restype = None
    L.tqr_plan_steps.argtypes = [_P]
    L.tqr_plan_steps.restype = _I
    L.tqr_plan_execute.argtypes = [_P, _P, _I, _P, _P]
    L.tqr_plan_destroy.argtypes = [_P]
    L.tqr_plan_set_profile.argtypes = [_P, _I]
    L.tqr_plan_stats.argtypes = [_P, ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_double)]
    L.tqr_fill_randzo.argtypes = [_I, _P, _I, _I, _I, ctypes.c_ulonglong, _P]
    L.tqr_fill_randzo_cols.argtypes = [_I, _P, _I, _I, _I, ctypes.c_ulonglong, ctypes.c_long, _P]
    L.tqr_dist_local_cols.argtypes = [_P]
    for nm in ("tqr_tile_geqrt", "tqr_tile_unmqr", "tqr_tile_tsqrt", "tqr_tile_tsmqr"):
        getattr(L, nm).restype = _I
    L.tqr_dist_plan_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I, _I, _I]
    L.tqr_dist_handle_bytes.argtypes = [_P]
    L.tqr_dist_handle_bytes.restype = ctypes.c_size_t
    L.tqr_dist_export.argtypes = [_P, ctypes.c_char_p, ctypes.c_size_t]
    L.tqr_dist_import.argtypes = [_P, ctypes.c_char_p, ctypes.c_size_t]
    L.tqr_dist_reset.argtypes = [_P, _P]
    L.tqr_dist_probe.argtypes = [_P, _I, ctypes.POINTER(ctypes.c_ulonglong)]
    L.tqr_plan_status.argtypes = [_P, _P]
    L.tqr_dist_owner.argtypes = [_P, _I]
    L.tqr_dgeqrt_host.argtypes = [_P, _P, _I, _I, _I, _I]
    L.tqr_sgeqrt_host.argtypes = [_P, _P, _I, _I, _I, _I]
    L.tqr_geqrt_host_engine.argtypes = [_I, _P, _P, _I, _I, _I, _I, _I]
    L.tqr_geqrt_host_engine.restype = _I
    L.tqr_dgeqrt_tiled.argtypes = [_I, _I, _I, _P, _I, _P, _P]
    L.tqr_dgeqrt_tiled.restype = _I
    L.tqr_sgeqrt_tiled.argtypes = [_I, _I, _I, _P, _I, _P, _P]
    L.tqr_sgeqrt_tiled.restype = _I
    L.tqr_flow_list_export.argtypes = [_P, _P, _I]
    L.tqr_flow_list_export_steps.argtypes = [_P, _I, _P, _I]
    L.tqr_flow_list_export_steps.restype = _I
    L.tqr_apply_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I]
    L.tqr_apply_create.restype = _I
    L.tqr_apply_workspace_bytes.argtypes = [_P]
    L.tqr_apply_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_apply_prepare.argtypes = [_P, _P, _I, _P, _P]
    L.tqr_apply_prepare.restype = _I
    L.tqr_apply_q.argtypes = [_P, _I, _P, _I, _P, _I, _I, _P]
    L.tqr_apply_q.restype = _I
    L.tqr_apply_destroy.argtypes = [_P]
    L.tqr_apply_destroy.restype = None
    L.tqr_trsm_r.argtypes = [_I, _I, _I, _I, _P, _I, _P, _I, _I, _P]
    L.tqr_trsm_r.restype = _I
    L.tqr_lstsq.argtypes = [_P, _I, _P, _I, _P, _I, _I, _P, _P]
    L.tqr_lstsq.restype = _I
    L.tqr_lstsq_fused.argtypes = [_P, _P, _I, _P, _I, _P, _P]
    L.tqr_lstsq_fused.restype = _I
    L.tqr_solve_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I]
    L.tqr_solve_create.restype = _I
    L.tqr_solve_workspace_bytes.argtypes = [_P]
    L.tqr_solve_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_solve_trsm_r.argtypes = [_P, _I, _P, _I, _P, _I, _I, _P]
    L.tqr_solve_trsm_r.restype = _I
    L.tqr_solve_status.argtypes = [_P, _P]
    L.tqr_solve_status.restype = _I
    L.tqr_solve_destroy.argtypes = [_P]
    L.tqr_solve_destroy.restype = None
    L.tqr_solve_ticket.argtypes = [_I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]
    L.tqr_solve_ticket.restype = _I
    L.tqr_lstsq_fused_solve.argtypes = [_P, _P, _P, _I, _P, _I, _P, _P]
    L.tqr_lstsq_fused_solve.restype = _I
    L.tqr_apply_pipe_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I, _I]
    L.tqr_apply_pipe_create.restype = _I
    L.tqr_apply_pipe_workspace_bytes.argtypes = [_P]
    L.tqr_apply_pipe_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_apply_pipe_q.argtypes = [_P, _P, _I, _P, _I, _P, _I, _I, _P]
    L.tqr_apply_pipe_q.restype = _I
    L.tqr_apply_pipe_status.argtypes = [_P, _P]
    L.tqr_apply_pipe_status.restype = _I
    L.tqr_apply_pipe_destroy.argtypes = [_P]
    L.tqr_apply_pipe_destroy.restype = None
    L.tqr_apply_pipe_ticket.argtypes = [_I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]
    L.tqr_apply_pipe_ticket.restype = _I
    L.tqr_apply_pipe_form_q.argtypes = [_P, _P, _P, _I, _P, _I, _I, _P]
    L.tqr_apply_pipe_form_q.restype = _I
    L.tqr_apply_pipe_form_q_items.argtypes = [_I, _I, _I]
    L.tqr_apply_pipe_form_q_items.restype = _I
    L.tqr_apply_pipe_form_q_ticket.argtypes = [_I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]
    L.tqr_apply_pipe_form_q_ticket.restype = _I
    L.tqr_lstsq_pipe.argtypes = [_P, _P, _P, _I, _P, _I, _P, _I, _I, _P, _P]
    L.tqr_lstsq_pipe.restype = _I
    _LL = ctypes.c_longlong
    L.tqr_batch_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I, _I, ctypes.c_size_t]
    L.tqr_batch_create.restype = _I
    L.tqr_batch_workspace_bytes.argtypes = [_P]
    L.tqr_batch_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_batch_group.argtypes = [_P]
    L.tqr_batch_group.restype = _I
    L.tqr_batch_execute.argtypes = [_P, _P, _I, _LL, _P, _LL, _P]
    L.tqr_batch_execute.restype = _I
    L.tqr_batch_destroy.argtypes = [_P]
    L.tqr_batch_destroy.restype = None
    L.tqr_batch_plan.argtypes = [_I, _I, _I, _I, _I, ctypes.c_size_t, ctypes.POINTER(_I), ctypes.POINTER(_I),
                                 ctypes.POINTER(_I)]
    L.tqr_batch_plan.restype = _I
    L.tqr_batch_apply_bytes.argtypes = [_I, _I, _I, _I, _I]
    L.tqr_batch_apply_bytes.restype = ctypes.c_size_t
    L.tqr_batch_apply_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I, _I]
    L.tqr_batch_apply_create.restype = _I
    L.tqr_batch_apply_workspace_bytes.argtypes = [_P]
    L.tqr_batch_apply_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_batch_apply_prepare.argtypes = [_P, _P, _I, _LL, _P, _LL, _P]
    L.tqr_batch_apply_prepare.restype = _I
    L.tqr_batch_apply_q.argtypes = [_P, _I, _P, _I, _LL, _P, _I, _I, _LL, _P]
    L.tqr_batch_apply_q.restype = _I
    L.tqr_batch_form_q.argtypes = [_P, _P, _I, _LL, _P, _I, _I, _LL, _P]
    L.tqr_batch_form_q.restype = _I
    L.tqr_batch_trsm_r.argtypes = [_I, _I, _I, _I, _I, _P, _I, _LL, _P, _I, _I, _LL, _P]
    L.tqr_batch_trsm_r.restype = _I
    L.tqr_batch_lstsq.argtypes = [_P, _I, _P, _I, _LL, _P, _I, _I, _LL, _P, _LL, _P]
    L.tqr_batch_lstsq.restype = _I
    L.tqr_batch_apply_destroy.argtypes = [_P]
    L.tqr_batch_apply_destroy.restype = None
    _SP = ctypes.POINTER(TsqrSpec)
    L.tqr_tsqr_plan.argtypes = [_SP, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), _I,
                                ctypes.POINTER(ctypes.c_size_t)]
    L.tqr_tsqr_plan.restype = _I
    L.tqr_tsqr_create.argtypes = [ctypes.POINTER(_P), _SP]
    L.tqr_tsqr_create.restype = _I
    L.tqr_tsqr_workspace_bytes.argtypes = [_P]
    L.tqr_tsqr_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_tsqr_factor.argtypes = [_P, _P, _I, _P]
    L.tqr_tsqr_factor.restype = _I
    L.tqr_tsqr_apply_q.argtypes = [_P, _I, _P, _I, _P, _I, _I, _P]
    L.tqr_tsqr_apply_q.restype = _I
    L.tqr_tsqr_form_q.argtypes = [_P, _P, _I, _P, _I, _P]
    L.tqr_tsqr_form_q.restype = _I
    L.tqr_tsqr_lstsq.argtypes = [_P, _I, _P, _I, _P, _I, _I, _P, _P]
    L.tqr_tsqr_lstsq.restype = _I
    L.tqr_tsqr_level.argtypes = [_P, _I, ctypes.POINTER(_P), ctypes.POINTER(_I), ctypes.POINTER(_P), ctypes.POINTER(_I),
                                 ctypes.POINTER(_I)]
    L.tqr_tsqr_level.restype = _I
    L.tqr_tsqr_destroy.argtypes = [_P]
    L.tqr_tsqr_destroy.restype = None
    L.tqr_update_create.argtypes = [ctypes.POINTER(_P), _I, _I, _I, _I]
    L.tqr_update_create.restype = _I
    L.tqr_update_workspace_bytes.argtypes = [_P]
    L.tqr_update_workspace_bytes.restype = ctypes.c_size_t
    L.tqr_update_rows.argtypes = [_P, _P, _I, _P, _I, _P, _P]
    L.tqr_update_rows.restype = _I
    L.tqr_update_prepare.argtypes = [_P, _P, _I, _P, _P]
    L.tqr_update_prepare.restype = _I
    L.tqr_update_apply_q.argtypes = [_P, _I, _P, _I, _P, _I, _P, _I, _I, _P]
    L.tqr_update_apply_q.restype = _I
    L.tqr_update_lstsq.argtypes = [_P, _P, _I, _P, _I, _P, _P, _I, _P, _I, _I, _P, _I, _P, _P]
    L.tqr_update_lstsq.restype = _I
    L.tqr_update_destroy.argtypes = [_P]
    L.tqr_update_destroy.restype = None
    L.tqr_update_plan.argtypes = [_I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]
    L.tqr_update_plan.restype = _I
    L.tqr_update_level_items.argtypes = [_I, _I, _I, _I, _P, _I]
    L.tqr_update_level_items.restype = _I
    _lib = L
    return L


def check(st, what=""):
    if st != 0:
        raise TQRError(f"{what}: {lib().tqr_strerror(st).decode()} ({st})")


def _ptr(a):
    if hasattr(a, "data_ptr"):
        return _P(a.data_ptr())
    return a.ctypes.data_as(_P)


def _dtype_code(dt):
    dt = np.dtype(dt) if not hasattr(dt, "is_floating_point") else dt
    if str(dt) in ("float64", "torch.float64"):
        return TQR_F64
    if str(dt) in ("float32", "torch.float32"):
        return TQR_F32
    raise TQRError(f"unsupported dtype {dt}")


# ---- scheduler (host C, no GPU needed) ---------------------------------------------------
class Scheduler:
    """The reference gridscheduler API (initScheduler / getNextTask / doneATask)."""

    def __init__(self, M, N):
        self.M, self.N = M, N
        self.grid = lib().initScheduler(M, N)
        if not self.grid:
            raise TQRError("initScheduler failed")

    def next_task(self):
        t = Task()
        r = lib().getNextTask(ctypes.byref(t), self.grid, self.M, self.N)
        return r, t

    def done(self, t):
        lib().doneATask(self.grid, self.M, self.N, t)

    def __del__(self):
        try:
            ctypes.CDLL(None).free(ctypes.cast(self.grid, _P))
        except Exception:
            pass


def sched_plan(M, N):
    """Static wave plan: list of waves, each a list of (type, l, m, k)."""
    p = Plan()
    check(lib().tqr_sched_plan(M, N, ctypes.byref(p)), "tqr_sched_plan")
    tasks = np.ctypeslib.as_array(p.tasks, shape=(p.ntasks * 4,)).reshape(-1, 4).copy()
    offs = np.ctypeslib.as_array(p.level_off, shape=(p.nlevels + 1,)).copy()
    lib().tqr_sched_plan_free(ctypes.byref(p))
    return [tasks[offs[L]:offs[L + 1]] for L in range(len(offs) - 1)]


# ---- device factorisation -------------------------------------------------------------------
ENGINES = {"waves": 0, "flow": 1}  # tqr_engine (include/tqr.h)


class TiledQR:
    """A planned factorisation (tqr_plan): create once, execute on device arrays. steps: a capped
    plan (tqr_plan_create_steps) — only the leading `steps` tile columns are factorised, every other
    column receives Q^T of those steps; tau is then (steps, m). engine: None (tqr_plan_create: the
    flow engine unless TQR_ENGINE=waves), or "flow" / "waves" (tqr_plan_create_engine); a capped plan
    always runs the flow engine, so engine together with steps raises."""

    def __init__(self, m, n, b, dtype, steps=None, engine=None):
        self.m, self.n, self.b = m, n, b
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.h = None
        if engine is not None and engine not in ENGINES:
            raise TQRError(f"TiledQR: engine must be None, 'flow' or 'waves', not {engine!r}")
        if engine is not None and steps is not None:
            raise TQRError("TiledQR: a capped plan (steps) always runs the flow engine; engine= cannot be given with it")
        h = _P()
        if engine is not None:
            self.kmax = min(m, n) // b
            check(lib().tqr_plan_create_engine(ctypes.byref(h), m, n, b, self.dtype, ENGINES[engine]),
                  "tqr_plan_create_engine")
        elif steps is None:
            self.kmax = min(m, n) // b
            check(lib().tqr_plan_create(ctypes.byref(h), m, n, b, self.dtype), "tqr_plan_create")
        else:
            self.kmax = steps
            check(lib().tqr_plan_create_steps(ctypes.byref(h), m, n, b, self.dtype, steps), "tqr_plan_create_steps")
        self.h = h

    def execute(self, A, tau, ldda=None, stream=None):
        """A, tau: device tensors (torch) — A (n, ldda) column-major, tau (kmax, m) compact."""
        ldda = ldda or self.m
        check(lib().tqr_plan_execute(self.h, _ptr(A), ldda, _ptr(tau), _P(stream or 0)), "tqr_plan_execute")

    def status(self, stream=None):
        """Synchronise `stream` and raise if the engine reported an error (tqr_plan_status)."""
        check(lib().tqr_plan_status(self.h, _P(stream or 0)), "tqr_plan_status")

    def lstsq_fused(self, AB, tau, nrhs, res=None, ldda=None, stream=None, solve=None):
        """tqr_lstsq_fused on a capped plan over [A | B] (steps = A's tile columns): AB (n, ldda) in
        place, tau (steps, m); `res` (optional) receives the nrhs residual norms. Stream-ordered.
        solve: a Solve handle for (steps * b, b, dtype) — the triangular solve then runs pipelined over
        workgroups (tqr_lstsq_fused_solve), with the same bits."""
        ldda = ldda or self.m
        pres = None if res is None else _ptr(res)
        if solve is None:
            check(lib().tqr_lstsq_fused(self.h, _ptr(AB), ldda, _ptr(tau), nrhs, pres, _stream_handle(stream)),
                  "tqr_lstsq_fused")
        else:
            check(lib().tqr_lstsq_fused_solve(self.h, solve.h, _ptr(AB), ldda, _ptr(tau), nrhs, pres,
                                              _stream_handle(stream)), "tqr_lstsq_fused_solve")

    def set_profile(self, on=True):
        check(lib().tqr_plan_set_profile(self.h, int(on)))

    def stats(self):
        nu, np_ = _I(), _I()
        mu, mp = ctypes.c_double(), ctypes.c_double()
        check(lib().tqr_plan_stats(self.h, ctypes.byref(nu), ctypes.byref(mu), ctypes.byref(np_), ctypes.byref(mp)))
        return {"n_update": nu.value, "ms_update": mu.value, "n_panel": np_.value, "ms_panel": mp.value}

    def __del__(self):
        try:
            if self.h:
                lib().tqr_plan_destroy(self.h)
        except Exception:
            pass


def tile_owner(j, world):
    """Rank owning tile column j in a multi-GPU factorisation (csrc/flow.hpp tile_owner): snake
    order over the ranks, 0..W-1 then W-1..0, so every rank's columns sum to the same index total.
    TQR_DIST_PART=cyclic restores j % W for A/B runs. Host-only helper (tests, planning): code that
    holds a plan asks the plan (DistTiledQR.owner), which read TQR_DIST_PART once, at creation."""
    blk, r = divmod(j, world)
    if os.environ.get("TQR_DIST_PART") == "cyclic":
        return r
    return world - 1 - r if blk % 2 else r


def peer_probe(L, h, rank, world, barrier):
    """The setup's peer-path probe (include/tqr.h tqr_dist_probe): every rank stores its token into
    each peer's probe word, `barrier()` (all ranks), every rank checks it sees each peer's token
    through the load path the chains poll. Raises TQRError naming the ranks whose stores did not
    arrive, before any factorisation could wait on them. Returns the bit mask of peers seen."""
    st = L.tqr_dist_probe(h, 0, None)
    if st != 0:
        raise TQRError(f"DistTiledQR: rank {rank}: peer probe (put) failed: {L.tqr_strerror(st).decode()} ({st})")
    barrier()
    seen = ctypes.c_ulonglong(0)
    st = L.tqr_dist_probe(h, 1, ctypes.byref(seen))
    missing = [r for r in range(world) if r != rank and not (seen.value >> r) & 1]
    if st != 0 or missing:
        raise TQRError(f"DistTiledQR: rank {rank} does not see the flag stores of rank(s) {missing}: "
                       "no working peer path (xGMI / IPC mapping) for the panel flags; "
                       "the factorisation would wait on them and time out")
    return seen.value


def owned_tile_cols(q, rank, world):
    """The tile columns 0..q-1 that `rank` owns."""
    return [j for j in range(q) if tile_owner(j, world) == rank]


class DistTiledQR(TiledQR):
    """One rank's share of a multi-GPU factorisation (tile-column partition, one process per GPU;
    include/tqr.h "multi-GPU"). Tile column j belongs to rank owner(j) (snake order 0..W-1,
    W-1..0, ...), and a rank stores only its own tile columns, packed: global tile column j is
    local tile column j // W (alloc_local / fill_randzo_local). The handle exchange goes over
    torch.distributed (`group`) once; the panel data moves GPU to GPU inside the persistent
    launch (xGMI stores into IPC-opened peer workspaces), and consecutive executes need no host
    synchronisation or barrier (epoch-valued flags on the device)."""

    def __init__(self, m, n, b, dtype, group=None):
        import torch.distributed as dist
        self.m, self.n, self.b = m, n, b
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.kmax = min(m, n) // b
        self.group = group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        verbose = os.environ.get("TQR_DIST_VERBOSE") == "1"

        def say(msg):
            if verbose:
                import sys
                print(f"[rank {self.rank}] DistTiledQR: {msg}", file=sys.stderr, flush=True)

        say("create")
        h = _P()
        check(lib().tqr_dist_plan_create(ctypes.byref(h), m, n, b, self.dtype, self.rank, self.world),
              "tqr_dist_plan_create")
        self.h = h
        if self.world > 1:
            say("export")
            hb = lib().tqr_dist_handle_bytes(self.h)
            buf = ctypes.create_string_buffer(hb)
            check(lib().tqr_dist_export(self.h, buf, hb), "tqr_dist_export")
            blocks = [None] * self.world
            say("all_gather")
            dist.all_gather_object(blocks, bytes(buf.raw), group=group)
            allb = b"".join(blocks)
            say("import")
            check(lib().tqr_dist_import(self.h, allb, len(allb)), "tqr_dist_import")
            # every rank must deal the tile columns the same way (TQR_DIST_PART is read per process
            # at plan creation): a disagreement would deadlock the launch, so fail here instead
            mine = self.owners()
            every = [None] * self.world
            dist.all_gather_object(every, mine, group=group)
            if any(o != mine for o in every):
                raise TQRError("DistTiledQR: ranks disagree on the tile-column partition (TQR_DIST_PART)")
            say("probe")
            peer_probe(lib(), self.h, self.rank, self.world, lambda: dist.barrier(group=group))
            say("ready")

    def owner(self, tile_col):
        """Rank owning tile column tile_col, as this plan partitions (tqr_dist_owner)."""
        r = lib().tqr_dist_owner(self.h, tile_col)
        if r < 0:
            check(r, "tqr_dist_owner")
        return r

    def owners(self):
        return [self.owner(j) for j in range(self.n // self.b)]

    def owned_cols(self):
        """The tile columns this rank owns (its panels and all their updates)."""
        return [j for j, r in enumerate(self.owners()) if r == self.rank]

    def owns(self, tile_col):
        return self.owner(tile_col) == self.rank

    def local_cols(self):
        """Number of tile columns this rank stores (tqr_dist_local_cols)."""
        c = lib().tqr_dist_local_cols(self.h)
        if c < 0:
            check(c, "tqr_dist_local_cols")
        return c

    def local_index(self, tile_col):
        """Local tile column of an owned global tile column."""
        return tile_col // self.world

    def alloc_local(self, device="cuda"):
        """(A, tau) device arrays of this rank's storage: A (local_cols * b, m) — row c = local
        matrix column c — and the compact tau (local_cols, m)."""
        import torch
        dt = torch.float64 if self.dtype == TQR_F64 else torch.float32
        nl = self.local_cols()
        return (torch.empty((nl * self.b, self.m), dtype=dt, device=device),
                torch.zeros((nl, self.m), dtype=dt, device=device))

    def fill_randzo_local(self, A, seed, stream=None):
        """This rank's tile columns of the global RANDZO matrix (tqr_fill_randzo_cols)."""
        b = self.b
        for j in self.owned_cols():
            lj = self.local_index(j)
            fill_randzo(A[lj * b:(lj + 1) * b], self.m, b, seed, stream=stream, col0=j * b)

    def fwd_bytes(self):
        """Bytes this rank forwards to its peers per factorisation (panel V/T images over xGMI)."""
        lib().tqr_plan_fwd_bytes.restype = ctypes.c_longlong
        return int(lib().tqr_plan_fwd_bytes(self.h))

    def execute(self, A, tau, ldda=None, stream=None):
        """Launch (stream-ordered) on this rank's packed storage (alloc_local). Every rank calls it
        the same number of times; no host synchronisation or barrier is needed between calls."""
        ldda = ldda or self.m
        check(lib().tqr_plan_execute(self.h, _ptr(A), ldda, _ptr(tau), _P(stream or 0)), "tqr_plan_execute")


def dist_plan_check(M, N, b, rank, world, seglen=8):
    """Host-only: (ntasks, n_forwarding_members) of one rank's task list (its panel tasks forward
    their images to the peers when world > 1)."""
    nt, nf = _I(), _I()
    check(lib().tqr_dist_plan_check(M, N, b, seglen, rank, world, ctypes.byref(nt), ctypes.byref(nf)),
          "tqr_dist_plan_check")
    return nt.value, nf.value


class FlowListSpec(ctypes.Structure):
    """tqr_flow_list_spec, include/tqr.h"""
    _fields_ = [(f, _I) for f in ("M", "N", "b", "dtype", "seglen", "world", "rank", "full", "nxc")] + \
               [("tcol", ctypes.c_double)]


def flow_list(M, N, b, dtype=TQR_F64, seglen=0, world=1, rank=-1, full=1, nxc=0, tcol=0.0, steps=0):
    """Host-only: the persistent engine's task list of a plan (tqr_flow_list_export) as an (n, 4)
    int32 array of {type | strip << 8, l, m, k}; rank < 0: the global list. steps > 0: the list of a
    capped plan (tqr_flow_list_export_steps)."""
    spec = FlowListSpec(M, N, b, dtype, seglen, world, rank, full, nxc, tcol)
    if steps:
        def export(items, cap):
            return lib().tqr_flow_list_export_steps(ctypes.byref(spec), steps, items, cap)
    else:
        def export(items, cap):
            return lib().tqr_flow_list_export(ctypes.byref(spec), items, cap)
    n = export(None, 0)
    if n < 0:
        check(n, "tqr_flow_list_export")
    items = np.zeros((n, 4), dtype=np.int32)
    if export(_ptr(items), n) != n:
        raise TQRError("tqr_flow_list_export: the list changed between two calls")
    return items


def strip_layout(p, q, steps, i, j, k):
    """Host-only: the layout (0 standard, 1 whole lines) in which a whole-line plan of p x q tiles with
    `steps` steps (0 = all) stores the chain strips of tile (i, j) at step k (tqr_flow_strip_layout)."""
    r = lib().tqr_flow_strip_layout(p, q, steps, i, j, k)
    if r < 0:
        check(r, "tqr_flow_strip_layout")
    return r


def strip_offset(layout, pair, lane, ld):
    """Host-only: byte offset of lane `lane`'s 16 bytes of row pair `pair` inside a wave's 16-column
    strip block under `layout`, leading dimension ld elements (tqr_flow_strip_offset)."""
    r = lib().tqr_flow_strip_offset(layout, pair, lane, ld)
    if r < 0:
        check(r, "tqr_flow_strip_offset")
    return r


def plan_info(plan):
    """tqr_plan_info of a TiledQR: engine (0 waves, 1 flow), ntasks, est_order, grid."""
    v = [_I() for _ in range(4)]
    check(lib().tqr_plan_info(plan.h, *[ctypes.byref(x) for x in v]), "tqr_plan_info")
    return dict(zip(("engine", "ntasks", "est_order", "grid"), (x.value for x in v)))


def plan_tasks(plan):
    """The task list on the device of a TiledQR's flow plan (tqr_plan_get_tasks), (n, 4) int32."""
    n = lib().tqr_plan_get_tasks(plan.h, None, 0)
    if n < 0:
        check(n, "tqr_plan_get_tasks")
    items = np.zeros((n, 4), dtype=np.int32)
    if lib().tqr_plan_get_tasks(plan.h, _ptr(items), n) != n:
        raise TQRError("tqr_plan_get_tasks: the list changed between two calls")
    return items


def fill_randzo(A, m, n, seed, ldda=None, stream=None, col0=0):
    """RANDZO input on the device (columns col0 .. col0 + n - 1 of the global matrix)."""
    check(lib().tqr_fill_randzo_cols(_dtype_code(A.dtype), _ptr(A), m, n, ldda or m, seed, col0, _P(stream or 0)),
          "tqr_fill_randzo_cols")


def geqrt_host(A, b, with_tau=True, m=None, tau=None, engine=None):
    """Factorise a host column-major array (shape (n, ldm)) in place on the GPU; returns the
    reference's m x n tau matrix (shape (n, ldm), zero except columns k*b; written into `tau` if
    given, else a new zeroed array), or None with with_tau=False (the reference's cudaQRTask
    discards tau). m: rows (default ldm). engine: None (tqr_dgeqrt_host / tqr_sgeqrt_host), or
    "flow" / "waves" (tqr_geqrt_host_engine)."""
    n, ldm = A.shape
    m = m or ldm
    if with_tau and tau is None:
        tau = np.zeros_like(A)
    if with_tau:
        assert tau.shape == A.shape and tau.dtype == A.dtype and tau.flags.c_contiguous
    ptau = _ptr(tau) if with_tau else None
    if engine is not None:
        if engine not in ENGINES:
            raise TQRError(f"geqrt_host: engine must be None, 'flow' or 'waves', not {engine!r}")
        check(lib().tqr_geqrt_host_engine(_dtype_code(A.dtype), _ptr(A), ptau, m, n, ldm, b, ENGINES[engine]),
              "tqr_geqrt_host_engine")
        return tau
    fn = lib().tqr_dgeqrt_host if A.dtype == np.float64 else lib().tqr_sgeqrt_host
    check(fn(_ptr(A), ptau, m, n, ldm, b), "tqr_geqrt_host")
    return tau


def geqrt_tiled(A, tau, b, m=None, ldda=None, stream=None):
    """The cached one-shot device helper (tqr_dgeqrt_tiled / tqr_sgeqrt_tiled by A's dtype): A
    (n, ldda) and tau (kmax, m) are device tensors of one dtype, factorised in place with the plan
    cached for (device, m, n, b, dtype). m defaults to ldda, ldda to A's row length. Stream-ordered."""
    n = A.shape[0]
    ldda = ldda or A.shape[-1]
    m = m or ldda
    if tau.dtype != A.dtype:
        raise TQRError("geqrt_tiled: A and tau must be of one dtype")
    fn = lib().tqr_dgeqrt_tiled if _dtype_code(A.dtype) == TQR_F64 else lib().tqr_sgeqrt_tiled
    check(fn(m, n, b, _ptr(A), ldda, _ptr(tau), _stream_handle(stream)), "tqr_geqrt_tiled")


class BatchedQR:
    """Many same-shape factorisations in one call (tqr_batch, include/tqr.h "batched"): every matrix
    of the batch comes out with the bytes of a TiledQR(engine="waves") executed on it alone, in the
    launch count of one matrix. Create once per (m, n, b, dtype, batch); ws_limit bounds the T
    workspace in bytes (0: 1 GiB) — a batch that needs more runs in groups of group() matrices."""

    def __init__(self, m, n, b, dtype, batch, ws_limit=0):
        self.m, self.n, self.b, self.batch = m, n, b, batch
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.kmax = min(m, n) // b if b > 0 else 0
        self.h = None
        h = _P()
        check(lib().tqr_batch_create(ctypes.byref(h), m, n, b, self.dtype, batch, ws_limit), "tqr_batch_create")
        self.h = h

    def workspace_bytes(self):
        return int(lib().tqr_batch_workspace_bytes(self.h))

    def group(self):
        """Matrices per launch group (tqr_batch_group)."""
        return int(lib().tqr_batch_group(self.h))

    def execute(self, A, tau, ldda=None, strideA=None, strideTau=None, stream=None):
        """A: device tensor (batch, n, ldda), column-major per matrix as for TiledQR.execute; tau
        (batch, kmax, m). ldda and the strides (in elements) default to those of contiguous tensors of
        these shapes; any other layout of include/tqr.h — padded, row-interleaved — is given by ldda,
        strideA, strideTau on a tensor whose first element is matrix 0's. Stream-ordered."""
        if _dtype_code(A.dtype) != self.dtype or _dtype_code(tau.dtype) != self.dtype:
            raise TQRError("BatchedQR.execute: A and tau must be of the handle's dtype")
        if ldda is None:
            if A.ndim != 3:  # (a flat buffer's length taken for ldda would pass the C validation)
                raise TQRError("BatchedQR.execute: ldda defaults to the row length of a (batch, n, ldda) tensor only")
            ldda = A.shape[-1]
        strideA = self.n * ldda if strideA is None else strideA
        strideTau = self.kmax * self.m if strideTau is None else strideTau
        check(lib().tqr_batch_execute(self.h, _ptr(A), ldda, strideA, _ptr(tau), strideTau, _stream_handle(stream)),
              "tqr_batch_execute")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_batch_destroy(self.h)
        except Exception:
            pass


def batch_plan(m, n, b, dtype, batch, ws_limit=0):
    """Host-only: (group, ngroups, nlaunch) a BatchedQR of these arguments would use (tqr_batch_plan)."""
    dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
    g, ng, nl = _I(), _I(), _I()
    check(lib().tqr_batch_plan(m, n, b, dtype, batch, ws_limit, ctypes.byref(g), ctypes.byref(ng), ctypes.byref(nl)),
          "tqr_batch_plan")
    return g.value, ng.value, nl.value


def geqrt_batched(A, tau, b, stream=None):
    """One-shot batched factorisation of contiguous device tensors A (batch, n, m) and tau
    (batch, kmax, m) in place: builds a BatchedQR, executes it and keeps nothing (the handle is
    released once its work has finished)."""
    if A.ndim != 3 or tau.ndim != 3 or tau.shape[0] != A.shape[0]:
        raise TQRError("geqrt_batched: A must be (batch, n, m) and tau (batch, kmax, m)")
    if not (A.is_contiguous() and tau.is_contiguous()):
        raise TQRError("geqrt_batched: A and tau must be contiguous (BatchedQR.execute takes strides)")
    batch, n, m = A.shape
    bq = BatchedQR(m, n, b, A.dtype, batch)
    if tuple(tau.shape[1:]) != (bq.kmax, m):
        raise TQRError(f"geqrt_batched: tau must be (batch, {bq.kmax}, {m})")
    bq.execute(A, tau, stream=stream)


def cache_clear():
    """Release the cached plans and host-API staging buffers (tqr_cache_clear)."""
    check(lib().tqr_cache_clear(), "tqr_cache_clear")


def expand_tau(tau_compact, m, n, b):
    """compact (kmax, m) -> the reference's m x n tau matrix as an (n, m) array."""
    T = np.zeros((n, m), dtype=tau_compact.dtype)
    for k in range(min(m, n) // b):
        T[k * b, k * b:] = tau_compact[k, k * b:]
    return T


def compact_tau(T, m, n, b):
    """The reference's m x n tau matrix ((n, m) array) -> compact (kmax, m): the inverse of
    expand_tau (column k*b, rows k*b.., becomes row k)."""
    kmax = min(m, n) // b
    tc = np.zeros((kmax, m), dtype=T.dtype)
    for k in range(kmax):
        tc[k, k * b:] = T[k * b, k * b:m]
    return tc


# ---- apply Q / Q^T of a finished factorisation; least squares -------------------------------
def _stream_handle(stream):
    """hipStream_t of a torch stream, a raw handle (int), or None (the default stream)."""
    return _P(getattr(stream, "cuda_stream", stream) or 0)


class ApplyQ:
    """C <- Q^T C / C <- Q C with the factors a TiledQR left on the device (tqr_apply, include/tqr.h
    "apply"). Create once per shape, prepare() once per factorisation (rebuilds the T factors into
    the handle's workspace), then apply() to any number of right-hand sides. Single GPU."""

    def __init__(self, m, n, b, dtype):
        self.m, self.n, self.b = m, n, b
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.kmax = min(m, n) // b if b > 0 else 0
        self.h = None
        h = _P()
        check(lib().tqr_apply_create(ctypes.byref(h), m, n, b, self.dtype), "tqr_apply_create")
        self.h = h

    def workspace_bytes(self):
        return int(lib().tqr_apply_workspace_bytes(self.h))

    def prepare(self, A, tau, ldda=None, stream=None):
        """A (n, ldda): the factorised matrix; tau (kmax, m) compact. Stream-ordered."""
        ldda = ldda or A.shape[-1]
        check(lib().tqr_apply_prepare(self.h, _ptr(A), ldda, _ptr(tau), _stream_handle(stream)), "tqr_apply_prepare")

    def apply(self, A, C, trans=True, nrhs=None, ldda=None, lddc=None, stream=None, pipe=None):
        """C (nrhs, lddc) <- Q^T C (trans) or Q C, in place; A as given to prepare(). nrhs, ldda and
        lddc default to the tensors' shapes. Stream-ordered. pipe: an ApplyPipe handle made for this
        (m, n, b, dtype) — the same bits from the pipelined kernel (ApplyPipe.apply), for a narrow C."""
        if pipe is not None:
            return pipe.apply(self, A, C, trans=trans, nrhs=nrhs, ldda=ldda, lddc=lddc, stream=stream)
        ldda = ldda or A.shape[-1]
        lddc = lddc or C.shape[-1]
        nrhs = C.shape[0] if nrhs is None else nrhs
        check(lib().tqr_apply_q(self.h, 1 if trans else 0, _ptr(A), ldda, _ptr(C), nrhs, lddc, _stream_handle(stream)),
              "tqr_apply_q")

    def lstsq(self, A, B, trans=False, nrhs=None, ldda=None, lddb=None, res=None, stream=None, pipe=None, solve=None):
        """tqr_lstsq on a prepared handle with m >= n; A as given to prepare(), B (nrhs, lddb) in place.
        trans=False: least squares — B <- Q^T B, then rows 0 .. n-1 <- X; `res` (optional, nrhs
        elements of B's dtype) receives |A x - b| per column. trans=True: the minimum-norm solution of
        A^T x = c, c in rows 0 .. n-1 of B on entry, x in all m rows on exit. Stream-ordered.
        pipe, solve: an ApplyPipe handle for this (m, n, b, dtype) and a Solve handle for (n, b, dtype),
        given together — the apply and the solve then run pipelined over workgroups (tqr_lstsq_pipe),
        with the same bits."""
        ldda = ldda or A.shape[-1]
        lddb = lddb or B.shape[-1]
        nrhs = B.shape[0] if nrhs is None else nrhs
        pres = None if res is None else _ptr(res)
        if pipe is None and solve is None:
            check(lib().tqr_lstsq(self.h, 1 if trans else 0, _ptr(A), ldda, _ptr(B), nrhs, lddb, pres,
                                  _stream_handle(stream)), "tqr_lstsq")
            return
        if pipe is None or solve is None:
            raise TQRError("ApplyQ.lstsq: pipe= and solve= go together (tqr_lstsq_pipe takes both)")
        pipe._match(self, nrhs, "ApplyQ.lstsq")
        if (solve.n, solve.b, solve.dtype) != (self.n, self.b, self.dtype) or nrhs > solve.nrhs_max:
            raise TQRError(f"ApplyQ.lstsq: the Solve handle is for n = {solve.n}, b = {solve.b}, dtype {solve.dtype}, "
                           f"nrhs <= {solve.nrhs_max}, not {self.n}, {self.b}, {self.dtype}, {nrhs}")
        check(lib().tqr_lstsq_pipe(pipe.h, solve.h, self.h, 1 if trans else 0, _ptr(A), ldda, _ptr(B), nrhs, lddb, pres,
                                   _stream_handle(stream)), "tqr_lstsq_pipe")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_apply_destroy(self.h)
        except Exception:
            pass


class ApplyPipe:
    """The apply of Q / Q^T pipelined over workgroups (tqr_apply_pipe, include/tqr.h "pipelined
    apply"): the bits of ApplyQ.apply, on one CU per step of the factorisation and 64 right-hand sides
    instead of one CU per 64 right-hand sides — the call for a narrow C. Create once per (m, n, b,
    dtype) and largest nrhs, independent of any ApplyQ; apply() takes a prepared ApplyQ of the same
    shape. Calls on one handle are serialised on the GPU and need no host synchronisation in between."""

    def __init__(self, m, n, b, dtype, nrhs_max):
        self.m, self.n, self.b, self.nrhs_max = m, n, b, nrhs_max
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.h = None
        h = _P()
        check(lib().tqr_apply_pipe_create(ctypes.byref(h), m, n, b, self.dtype, nrhs_max), "tqr_apply_pipe_create")
        self.h = h

    def workspace_bytes(self):
        return int(lib().tqr_apply_pipe_workspace_bytes(self.h))

    def _match(self, ap, nrhs, who):
        if (ap.m, ap.n, ap.b, ap.dtype) != (self.m, self.n, self.b, self.dtype):
            raise TQRError(f"{who}: the ApplyPipe handle is for (m, n, b, dtype) = {(self.m, self.n, self.b, self.dtype)}, "
                           f"the ApplyQ for {(ap.m, ap.n, ap.b, ap.dtype)}")
        if nrhs > self.nrhs_max:
            raise TQRError(f"{who}: nrhs = {nrhs} exceeds the ApplyPipe handle's nrhs_max = {self.nrhs_max}")

    def apply(self, ap, A, C, trans=True, nrhs=None, ldda=None, lddc=None, stream=None):
        """C (nrhs, lddc) <- Q^T C (trans) or Q C in place, as ap.apply(A, C, ...): ap a prepared ApplyQ
        of this handle's shape and dtype, A as given to its prepare(). Stream-ordered."""
        ldda = ldda or A.shape[-1]
        lddc = lddc or C.shape[-1]
        nrhs = C.shape[0] if nrhs is None else nrhs
        self._match(ap, nrhs, "ApplyPipe.apply")
        if _dtype_code(C.dtype) != self.dtype or _dtype_code(A.dtype) != self.dtype:
            raise TQRError("ApplyPipe.apply: A and C must be of the handle's dtype")
        check(lib().tqr_apply_pipe_q(self.h, ap.h, 1 if trans else 0, _ptr(A), ldda, _ptr(C), nrhs, lddc,
                                     _stream_handle(stream)), "tqr_apply_pipe_q")

    def form_q(self, ap, A, Q, ncols=None, ldda=None, lddq=None, stream=None):
        """Q (ncols, lddq) <- the first ncols columns of the m x m orthogonal factor (row j = column j of
        Q), 1 <= ncols <= min(m, nrhs_max): ap a prepared ApplyQ of this handle's shape and dtype, A as
        given to its prepare(). Q is output-only — what it holds on entry does not matter — and the
        work on the identity's zero blocks is not done (tqr_apply_pipe_form_q). ncols and lddq default
        to Q's shape. Stream-ordered."""
        ldda = ldda or A.shape[-1]
        lddq = lddq or Q.shape[-1]
        ncols = Q.shape[0] if ncols is None else ncols
        self._match(ap, ncols, "ApplyPipe.form_q")
        if ncols > self.m:
            raise TQRError(f"ApplyPipe.form_q: ncols = {ncols} exceeds m = {self.m}")
        if _dtype_code(Q.dtype) != self.dtype or _dtype_code(A.dtype) != self.dtype:
            raise TQRError("ApplyPipe.form_q: A and Q must be of the handle's dtype")
        check(lib().tqr_apply_pipe_form_q(self.h, ap.h, _ptr(A), ldda, _ptr(Q), ncols, lddq, _stream_handle(stream)),
              "tqr_apply_pipe_form_q")

    def status(self, stream=None):
        """Synchronise `stream` and the handle's last call; raise if a wait timed out (tqr_apply_pipe_status)."""
        check(lib().tqr_apply_pipe_status(self.h, _stream_handle(stream)), "tqr_apply_pipe_status")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_apply_pipe_destroy(self.h)
        except Exception:
            pass


def apply_pipe_ticket(kmax, nstrips, trans, ticket):
    """Host-only: (strip, step) of a ticket of the pipelined apply (tqr_apply_pipe_ticket)."""
    st, step = _I(), _I()
    check(lib().tqr_apply_pipe_ticket(kmax, nstrips, 1 if trans else 0, ticket, ctypes.byref(st), ctypes.byref(step)),
          "tqr_apply_pipe_ticket")
    return st.value, step.value


def apply_pipe_form_q_items(kmax, b, ncols):
    """Host-only: the number of work items (the grid) of ApplyPipe.form_q (tqr_apply_pipe_form_q_items)."""
    n = lib().tqr_apply_pipe_form_q_items(kmax, b, ncols)
    if n < 0:
        check(n, "tqr_apply_pipe_form_q_items")
    return n


def apply_pipe_form_q_ticket(kmax, b, ncols, ticket):
    """Host-only: (strip, step) of a ticket of ApplyPipe.form_q (tqr_apply_pipe_form_q_ticket)."""
    st, step = _I(), _I()
    check(lib().tqr_apply_pipe_form_q_ticket(kmax, b, ncols, ticket, ctypes.byref(st), ctypes.byref(step)),
          "tqr_apply_pipe_form_q_ticket")
    return st.value, step.value


class Solve:
    """The triangular solve with R pipelined over workgroups (tqr_solve, include/tqr.h "pipelined
    solve"): the bits of trsm_r, on n / b CUs per 64 right-hand sides instead of one — the call for a
    narrow X. Create once per (n, b, dtype) and largest nrhs; calls on one handle are serialised on
    the GPU and need no host synchronisation in between."""

    def __init__(self, n, b, dtype, nrhs_max):
        self.n, self.b, self.nrhs_max = n, b, nrhs_max
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.h = None
        h = _P()
        check(lib().tqr_solve_create(ctypes.byref(h), n, b, self.dtype, nrhs_max), "tqr_solve_create")
        self.h = h

    def workspace_bytes(self):
        return int(lib().tqr_solve_workspace_bytes(self.h))

    def trsm_r(self, F, X, trans=False, nrhs=None, ldda=None, lddx=None, stream=None):
        """X (>= nrhs, lddx) <- R^{-1} X (or R^{-T} X with trans) in place, R the upper triangle of the
        leading n x n block of F (>= n, ldda); as tqr.trsm_r. Stream-ordered."""
        if X.dtype != F.dtype or _dtype_code(F.dtype) != self.dtype:
            raise TQRError("Solve.trsm_r: F and X must be of the handle's dtype")
        nrhs = X.shape[0] if nrhs is None else nrhs
        ldda = ldda or F.shape[-1]
        lddx = lddx or X.shape[-1]
        check(lib().tqr_solve_trsm_r(self.h, 1 if trans else 0, _ptr(F), ldda, _ptr(X), nrhs, lddx,
                                     _stream_handle(stream)), "tqr_solve_trsm_r")

    def status(self, stream=None):
        """Synchronise `stream` and the handle's last call; raise if a wait timed out (tqr_solve_status)."""
        check(lib().tqr_solve_status(self.h, _stream_handle(stream)), "tqr_solve_status")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_solve_destroy(self.h)
        except Exception:
            pass


def solve_ticket(T, nstrips, trans, ticket):
    """Host-only: (strip, row) of a ticket of the pipelined solve (tqr_solve_ticket)."""
    st, row = _I(), _I()
    check(lib().tqr_solve_ticket(T, nstrips, 1 if trans else 0, ticket, ctypes.byref(st), ctypes.byref(row)),
          "tqr_solve_ticket")
    return st.value, row.value


def trsm_r(F, X, b, trans=False, n=None, nrhs=None, ldda=None, lddx=None, stream=None, solve=None):
    """X <- R^{-1} X (or R^{-T} X with trans) in place, R the upper triangle of the leading n x n block
    of the factorised F (tqr_trsm_r, include/tqr.h "solve"). F (>= n, ldda) and X (>= nrhs, lddx) are
    device tensors of one dtype; n defaults to F's column count, nrhs, ldda and lddx to the tensors'
    shapes. No handle and no workspace. Stream-ordered. solve: a Solve handle made for (n, b, dtype) —
    the same bits from the pipelined kernel (Solve.trsm_r), the faster call for a narrow X."""
    if X.dtype != F.dtype:
        raise TQRError("trsm_r: F and X must be of one dtype")
    n = F.shape[0] if n is None else n
    nrhs = X.shape[0] if nrhs is None else nrhs
    ldda = ldda or F.shape[-1]
    lddx = lddx or X.shape[-1]
    if solve is not None:
        if solve.n != n or solve.b != b:
            raise TQRError(f"trsm_r: the Solve handle is for n = {solve.n}, b = {solve.b}, not {n}, {b}")
        return solve.trsm_r(F, X, trans=trans, nrhs=nrhs, ldda=ldda, lddx=lddx, stream=stream)
    check(lib().tqr_trsm_r(_dtype_code(F.dtype), 1 if trans else 0, n, b, _ptr(F), ldda, _ptr(X), nrhs, lddx,
                           _stream_handle(stream)), "tqr_trsm_r")


def lstsq(F, tau, B, b):
    """Least squares min |A x - b| for every column of B from a finished factorisation of the
    m x n matrix A, m >= n: F (n, m) and tau (kmax, m) as TiledQR.execute left them, B (nrhs, m), all
    device tensors of one dtype. B is overwritten with Q^T B (the apply kernel); R X = (Q^T B)[:n] is
    then one triangular solve on the upper triangle of F (torch: n^2 nrhs flops of plumbing next to
    the apply's ~4 m n nrhs). Returns X as (nrhs, n) and the residual norms |A x - b| per column,
    taken from rows n .. m-1 of Q^T B."""
    import torch
    n, m = F.shape
    if m < n:
        raise TQRError(f"lstsq needs m >= n, got {m} x {n}")
    if B.shape[-1] != m or B.dtype != F.dtype or tau.dtype != F.dtype:
        raise TQRError("lstsq: B must be (nrhs, m) and F, tau, B of one dtype")
    ap = ApplyQ(m, n, b, F.dtype)
    cs = torch.cuda.current_stream()  # the torch ops below are ordered behind the apply on it
    ap.prepare(F, tau, stream=cs)
    ap.apply(F, B, trans=True, stream=cs)
    # column-major R is the transpose of the torch view: X^T R^T = Y^T with R^T lower triangular
    Rt = torch.tril(F[:, :n])
    X = torch.linalg.solve_triangular(Rt, B[:, :n], upper=False, left=False)
    res = torch.linalg.vector_norm(B[:, n:], dim=1)
    return X, res


def _batch_layout(who, T, cols, ld, stride):
    """(cols, ld, stride) of a batch operand: the defaults of a (batch, cols, ld) tensor, or what the
    caller gives for a flat one (whose length taken for ld would pass the C validation)."""
    if T.ndim == 3:
        cols = T.shape[1] if cols is None else cols
        ld = T.shape[-1] if ld is None else ld
    elif cols is None or ld is None:
        raise TQRError(f"{who}: the column count and the leading dimension default to the shape of a "
                       "(batch, columns, ld) tensor only")
    return cols, ld, cols * ld if stride is None else stride


class BatchedApply:
    """Apply, form-Q and least squares on every member of a BatchedQR's layout in the launches of one
    (tqr_batch_apply, include/tqr.h "batched apply and solve"): member i gets the bytes of ApplyQ's
    calls on it alone. Create once per (m, n, b, dtype, batch) — the handle holds the T images of all
    members, batch_apply_bytes() of them —, prepare() once per factorisation, then any number of calls.
    Operands are (batch, columns, ld) tensors with default strides, or flat tensors whose first element
    is member 0's with ldd*= and stride*= (elements) for any layout of include/tqr.h."""

    def __init__(self, m, n, b, dtype, batch):
        self.m, self.n, self.b, self.batch = m, n, b, batch
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.kmax = min(m, n) // b if b > 0 else 0
        self.h = None
        h = _P()
        check(lib().tqr_batch_apply_create(ctypes.byref(h), m, n, b, self.dtype, batch), "tqr_batch_apply_create")
        self.h = h

    def workspace_bytes(self):
        return int(lib().tqr_batch_apply_workspace_bytes(self.h))

    def _same(self, who, *tensors):
        for t in tensors:
            if t is not None and _dtype_code(t.dtype) != self.dtype:
                raise TQRError(f"BatchedApply.{who}: every tensor must be of the handle's dtype")

    def prepare(self, A, tau, ldda=None, strideA=None, strideTau=None, stream=None):
        """A and tau as BatchedQR.execute left them, with the same ldda / strideA / strideTau. Stream-ordered."""
        self._same("prepare", A, tau)
        _, ldda, strideA = _batch_layout("BatchedApply.prepare", A, self.n, ldda, strideA)
        strideTau = self.kmax * self.m if strideTau is None else strideTau
        check(lib().tqr_batch_apply_prepare(self.h, _ptr(A), ldda, strideA, _ptr(tau), strideTau, _stream_handle(stream)),
              "tqr_batch_apply_prepare")

    def apply(self, A, C, trans=True, nrhs=None, ldda=None, lddc=None, strideA=None, strideC=None, stream=None):
        """C_i (nrhs, lddc) <- Q_i^T C_i (trans) or Q_i C_i in place, for every member. Stream-ordered."""
        self._same("apply", A, C)
        _, ldda, strideA = _batch_layout("BatchedApply.apply", A, self.n, ldda, strideA)
        nrhs, lddc, strideC = _batch_layout("BatchedApply.apply", C, nrhs, lddc, strideC)
        check(lib().tqr_batch_apply_q(self.h, 1 if trans else 0, _ptr(A), ldda, strideA, _ptr(C), nrhs, lddc, strideC,
                                      _stream_handle(stream)), "tqr_batch_apply_q")

    def form_q(self, A, Q, ncols=None, ldda=None, lddq=None, strideA=None, strideQ=None, stream=None):
        """Q_i (ncols, lddq) <- the first ncols columns of member i's Q, 1 <= ncols <= m; Q is output-only."""
        self._same("form_q", A, Q)
        _, ldda, strideA = _batch_layout("BatchedApply.form_q", A, self.n, ldda, strideA)
        ncols, lddq, strideQ = _batch_layout("BatchedApply.form_q", Q, ncols, lddq, strideQ)
        check(lib().tqr_batch_form_q(self.h, _ptr(A), ldda, strideA, _ptr(Q), ncols, lddq, strideQ, _stream_handle(stream)),
              "tqr_batch_form_q")

    def lstsq(self, A, B, trans=False, nrhs=None, ldda=None, lddb=None, strideA=None, strideB=None, res=None,
              strideRes=None, stream=None):
        """ApplyQ.lstsq on every member (m >= n): B_i in place; res (optional): member i's nrhs residual
        norms at element i * strideRes (default nrhs). Stream-ordered."""
        self._same("lstsq", A, B, res)
        _, ldda, strideA = _batch_layout("BatchedApply.lstsq", A, self.n, ldda, strideA)
        nrhs, lddb, strideB = _batch_layout("BatchedApply.lstsq", B, nrhs, lddb, strideB)
        strideRes = nrhs if strideRes is None else strideRes
        pres = None if res is None else _ptr(res)
        check(lib().tqr_batch_lstsq(self.h, 1 if trans else 0, _ptr(A), ldda, strideA, _ptr(B), nrhs, lddb, strideB, pres,
                                    strideRes, _stream_handle(stream)), "tqr_batch_lstsq")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_batch_apply_destroy(self.h)
        except Exception:
            pass


def batch_apply_bytes(m, n, b, dtype, batch):
    """Host-only: the workspace a BatchedApply of these arguments allocates (tqr_batch_apply_bytes);
    bad arguments raise."""
    dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
    nb = int(lib().tqr_batch_apply_bytes(m, n, b, dtype, batch))
    if nb == 0:
        raise TQRError(f"tqr_batch_apply_bytes: invalid arguments {(m, n, b, dtype, batch)}")
    return nb


def trsm_r_batched(F, X, b, trans=False, n=None, nrhs=None, batch=None, ldda=None, lddx=None, strideA=None, strideX=None,
                   stream=None):
    """X_i <- R_i^{-1} X_i (or R_i^{-T} X_i with trans) in place for every member of a batch
    (tqr_batch_trsm_r): trsm_r's bytes per member, no handle, no workspace. F (batch, >= n, ldda) and X
    (batch, nrhs, lddx) with default strides, or flat tensors with n, nrhs, batch, ldd* and stride*."""
    if X.dtype != F.dtype:
        raise TQRError("trsm_r_batched: F and X must be of one dtype")
    if batch is None:
        if F.ndim != 3:
            raise TQRError("trsm_r_batched: batch defaults to the first dimension of a (batch, columns, ld) tensor only")
        batch = F.shape[0]
    fcols, ldda, strideA = _batch_layout("trsm_r_batched", F, None if F.ndim == 3 else n, ldda, strideA)
    n = fcols if n is None else n
    nrhs, lddx, strideX = _batch_layout("trsm_r_batched", X, nrhs, lddx, strideX)
    check(lib().tqr_batch_trsm_r(_dtype_code(F.dtype), 1 if trans else 0, n, b, batch, _ptr(F), ldda, strideA, _ptr(X), nrhs,
                                 lddx, strideX, _stream_handle(stream)), "tqr_batch_trsm_r")


def lstsq_batched(A, B, b):
    """One-shot batched least squares min |A_i x - b| for every column of every B_i: A (batch, n, m)
    and B (batch, nrhs, m) contiguous device tensors of one dtype, m >= n. Factorises a copy of A with
    a BatchedQR and solves with a BatchedApply; A and B are not modified. Returns (X (batch, nrhs, n),
    res (batch, nrhs), F, tau): F and tau as BatchedQR.execute leaves them."""
    import torch
    if A.ndim != 3 or B.ndim != 3 or B.shape[0] != A.shape[0] or B.shape[-1] != A.shape[-1] or B.dtype != A.dtype:
        raise TQRError("lstsq_batched: A must be (batch, n, m) and B (batch, nrhs, m), of one dtype")
    batch, n, m = A.shape
    if m < n:
        raise TQRError(f"lstsq_batched needs m >= n, got {m} x {n}")
    bq = BatchedQR(m, n, b, A.dtype, batch)
    ba = BatchedApply(m, n, b, A.dtype, batch)
    F, Y = A.clone().contiguous(), B.clone().contiguous()
    tau = torch.zeros((batch, bq.kmax, m), dtype=A.dtype, device=A.device)
    res = torch.empty((batch, B.shape[1]), dtype=A.dtype, device=A.device)
    cs = torch.cuda.current_stream()
    bq.execute(F, tau, stream=cs)
    ba.prepare(F, tau, stream=cs)
    ba.lstsq(F, Y, res=res, stream=cs)
    return Y[:, :, :n], res, F, tau


def lstsq_fused(A, B, b, solve=None):
    """Least squares min |A x - b| for every column of B with the factorisation itself, in one
    pipelined launch (tqr_lstsq_fused, include/tqr.h): A (n, m) and B (nrhs, m) are device tensors of
    one dtype, m >= n (row j = column j, as everywhere in this module). Builds [A | B padded with zero
    columns to whole tiles], runs a capped plan over it, and returns (X (nrhs, n), res (nrhs,), F, tau):
    F (n, m) and tau (n / b, m) are an ordinary factorisation of A — ApplyQ(m, n).prepare(F, tau) and
    trsm_r(F, ...) work on them. A and B are not modified. solve: a Solve handle for (n, b, dtype) with
    nrhs_max >= nrhs — the triangular solve then runs pipelined over workgroups, with the same bits."""
    import torch
    n, m = A.shape
    if m < n:
        raise TQRError(f"lstsq_fused needs m >= n, got {m} x {n}")
    if B.ndim != 2 or B.shape[-1] != m or B.dtype != A.dtype or B.shape[0] < 1:
        raise TQRError("lstsq_fused: B must be (nrhs, m) of A's dtype")
    nrhs = B.shape[0]
    r = (nrhs + b - 1) // b
    AB = torch.zeros((n + r * b, m), dtype=A.dtype, device=A.device)
    AB[:n] = A
    AB[n:n + nrhs] = B
    plan = TiledQR(m, n + r * b, b, A.dtype, steps=n // b if b > 0 and n % b == 0 else 0)
    tau = torch.zeros((n // b, m), dtype=A.dtype, device=A.device)
    res = torch.empty((nrhs,), dtype=A.dtype, device=A.device)
    cs = torch.cuda.current_stream()
    plan.lstsq_fused(AB, tau, nrhs, res=res, stream=cs, solve=solve)
    plan.status(cs.cuda_stream)
    if solve is not None:
        solve.status(cs)
    return AB[n:n + nrhs, :n], res, AB[:n], tau


def form_qt(A, b):
    """Q^T (m x m) of the tiled factorisation of A (n, m), m >= n, from a capped plan over [A | I]:
    the identity's columns receive Q^T in the factorisation's own launch. Returns (Qt, F, tau): Qt
    (m, m) with row j = column j of Q^T (so Qt.T, read in this module's convention, is Q), F (n, m)
    and tau (n / b, m) an ordinary factorisation of A."""
    import torch
    n, m = A.shape
    if m < n:
        raise TQRError(f"form_qt needs m >= n, got {m} x {n}")
    AI = torch.zeros((n + m, m), dtype=A.dtype, device=A.device)
    AI[:n] = A
    AI[n:].fill_diagonal_(1.0)
    plan = TiledQR(m, n + m, b, A.dtype, steps=n // b if b > 0 and n % b == 0 else 0)
    tau = torch.zeros((n // b, m), dtype=A.dtype, device=A.device)
    cs = torch.cuda.current_stream()
    plan.execute(AI, tau, stream=cs.cuda_stream)
    plan.status(cs.cuda_stream)
    return AI[n:], AI[:n], tau


def form_q(F, tau, b, ncols=None):
    """The first ncols columns of Q (m x m) from a finished factorisation: F (n, m) and tau (kmax, m)
    as TiledQR.execute left them (any m, n). ncols defaults to min(m, n), the thin Q; up to m gives
    the full Q. Returns a new (ncols, m) tensor, row j = column j of Q. Prepares an ApplyQ and runs
    ApplyPipe.form_q — the pipelined apply to an identity that is never stored and whose zero blocks
    cost nothing (unlike form_qt it needs no unfactorised A and no second factorisation)."""
    import torch
    n, m = F.shape
    ncols = min(m, n) if ncols is None else ncols
    if ncols < 1 or ncols > m:
        raise TQRError(f"form_q: ncols = {ncols} must be in 1 .. m = {m}")
    if tau.dtype != F.dtype:
        raise TQRError("form_q: F and tau must be of one dtype")
    ap = ApplyQ(m, n, b, F.dtype)
    pipe = ApplyPipe(m, n, b, F.dtype, ncols)
    Q = torch.empty((ncols, m), dtype=F.dtype, device=F.device)
    cs = torch.cuda.current_stream()
    ap.prepare(F, tau, stream=cs)
    pipe.form_q(ap, F, Q, stream=cs)
    pipe.status(cs)
    return Q


def apply_q_host(F, T, C, b, trans=True):
    """Convenience for host arrays: F, T (n, m) as geqrt_host produces them (T: the reference's
    m x n tau matrix), C (nrhs, m). Staged through torch to the GPU; returns the new C."""
    import torch
    n, m = F.shape
    if T.shape != F.shape or C.ndim != 2 or C.shape[1] != m or C.dtype != F.dtype or T.dtype != F.dtype:
        raise TQRError("apply_q_host: F, T (n, m) and C (nrhs, m) of one dtype")
    ap = ApplyQ(m, n, b, F.dtype)
    dF = torch.tensor(np.ascontiguousarray(F), device="cuda")  # (copies: read-only inputs are fine)
    dt = torch.tensor(compact_tau(T, m, n, b), device="cuda")
    dC = torch.tensor(np.ascontiguousarray(C), device="cuda")
    cs = torch.cuda.current_stream()
    ap.prepare(dF, dt, stream=cs)
    ap.apply(dF, dC, trans=trans, stream=cs)
    torch.cuda.synchronize()
    return dC.cpu().numpy()


# ---- tall-skinny QR: a tree of batched factorisations ----------------------------------------
class TSQR:
    """QR of a tall-skinny m x n matrix as a tree of batched factorisations (tqr_tsqr, include/tqr.h
    "tall-skinny"): the row domains of m_dom rows are factorised in the launches of one, their R factors
    are stacked `fan` at a time and factorised again, up to one root. factor() leaves R of the whole
    matrix in the upper triangle of A[0:n, 0:n] (trsm_r works on A unchanged); apply / form_q / lstsq
    need nrhs_max >= their width (form_q: >= n). m_dom = 0 and fan = 0 take the library's defaults.
    Calls on one handle are serialised on the GPU and need no host synchronisation in between."""

    def __init__(self, m, n, b, dtype, m_dom=0, fan=0, nrhs_max=0, ws_limit=0):
        self.m, self.n, self.b, self.nrhs_max = m, n, b, nrhs_max
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.h = None
        spec = TsqrSpec(m, n, b, self.dtype, m_dom, fan, nrhs_max, ws_limit)
        h = _P()
        check(lib().tqr_tsqr_create(ctypes.byref(h), ctypes.byref(spec)), "tqr_tsqr_create")
        self.h = h
        self.m_dom, self.fan, self.levels, self.domains, _ = tsqr_plan(m, n, b, self.dtype, m_dom, fan, nrhs_max, ws_limit)

    def workspace_bytes(self):
        return int(lib().tqr_tsqr_workspace_bytes(self.h))

    def level(self, l):
        """(dW, ldw, dtau, dom_rows, ndom) of level l (tqr_tsqr_level): device addresses as ints (dW is
        None at level 0, where the matrix is the caller's; both are None without a device)."""
        w, t = _P(), _P()
        ld, rows, nd = _I(), _I(), _I()
        check(lib().tqr_tsqr_level(self.h, l, ctypes.byref(w), ctypes.byref(ld), ctypes.byref(t), ctypes.byref(rows),
                                   ctypes.byref(nd)), "tqr_tsqr_level")
        return w.value, ld.value, t.value, rows.value, nd.value

    def _same(self, who, *tensors):
        for t in tensors:
            if _dtype_code(t.dtype) != self.dtype:
                raise TQRError(f"{who}: every tensor must be of the handle's dtype")

    def factor(self, A, ldda=None, stream=None):
        """A (n, ldda), column-major as for TiledQR.execute, in place. Stream-ordered."""
        self._same("TSQR.factor", A)
        ldda = ldda or A.shape[-1]
        check(lib().tqr_tsqr_factor(self.h, _ptr(A), ldda, _stream_handle(stream)), "tqr_tsqr_factor")

    def apply(self, A, C, trans=True, nrhs=None, ldda=None, lddc=None, stream=None):
        """C (nrhs, lddc) <- Q^T C (trans) or Q C in place; A as factor() left it. Stream-ordered."""
        self._same("TSQR.apply", A, C)
        ldda = ldda or A.shape[-1]
        lddc = lddc or C.shape[-1]
        nrhs = C.shape[0] if nrhs is None else nrhs
        check(lib().tqr_tsqr_apply_q(self.h, 1 if trans else 0, _ptr(A), ldda, _ptr(C), nrhs, lddc, _stream_handle(stream)),
              "tqr_tsqr_apply_q")

    def form_q(self, A, Q, ldda=None, lddq=None, stream=None):
        """Q (n, lddq) <- the thin Q (row j = column j of Q); output-only. Stream-ordered."""
        self._same("TSQR.form_q", A, Q)
        ldda = ldda or A.shape[-1]
        lddq = lddq or Q.shape[-1]
        check(lib().tqr_tsqr_form_q(self.h, _ptr(A), ldda, _ptr(Q), lddq, _stream_handle(stream)), "tqr_tsqr_form_q")

    def lstsq(self, A, B, trans=False, nrhs=None, ldda=None, lddb=None, res=None, stream=None):
        """tqr_tsqr_lstsq: as ApplyQ.lstsq, on the handle's own factorisation. Stream-ordered."""
        self._same("TSQR.lstsq", A, B)
        ldda = ldda or A.shape[-1]
        lddb = lddb or B.shape[-1]
        nrhs = B.shape[0] if nrhs is None else nrhs
        pres = None if res is None else _ptr(res)
        check(lib().tqr_tsqr_lstsq(self.h, 1 if trans else 0, _ptr(A), ldda, _ptr(B), nrhs, lddb, pres,
                                   _stream_handle(stream)), "tqr_tsqr_lstsq")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_tsqr_destroy(self.h)
        except Exception:
            pass


def tsqr_plan(m, n, b, dtype, m_dom=0, fan=0, nrhs_max=0, ws_limit=0):
    """Host-only: (m_dom, fan, nlevels, [D_0 .. D_{L-1}], workspace bytes) a TSQR of these arguments
    would use (tqr_tsqr_plan)."""
    dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
    spec = TsqrSpec(m, n, b, dtype, m_dom, fan, nrhs_max, ws_limit)
    md, f, nl = _I(), _I(), _I()
    ws = ctypes.c_size_t()
    dom = (_I * 32)()
    check(lib().tqr_tsqr_plan(ctypes.byref(spec), ctypes.byref(md), ctypes.byref(f), ctypes.byref(nl), dom, 32,
                              ctypes.byref(ws)), "tqr_tsqr_plan")
    return md.value, f.value, nl.value, list(dom[:nl.value]), int(ws.value)


# ---- row update: append rows to a finished QR ---------------------------------------------------
class RowUpdate:
    """Append mw rows to the R of a finished n-column factorisation (tqr_update, include/tqr.h "row
    update"): R'^T R' = R^T R + W^T W by the flat-tree TSQRT / TSMQR on the tiles that exist. Create once
    per (n, mw, b, dtype); update() any number of times. Tensors follow the module convention: R
    (n, lddr) with the triangle in R[j, i], i <= j; W (n, lddw) the new rows, column-major; tau (q, mw).
    After an update the Q of the whole is diag(Q_old, I) Q_u: apply() is Q_u alone, on a pair of blocks."""

    def __init__(self, n, mw, b, dtype):
        self.n, self.mw, self.b = n, mw, b
        self.dtype = dtype if isinstance(dtype, int) else _dtype_code(dtype)
        self.q = n // b if b > 0 else 0
        self.h = None
        h = _P()
        check(lib().tqr_update_create(ctypes.byref(h), n, mw, b, self.dtype), "tqr_update_create")
        self.h = h

    def workspace_bytes(self):
        return int(lib().tqr_update_workspace_bytes(self.h))

    def _same(self, who, *tensors):
        for t in tensors:
            if t is not None and _dtype_code(t.dtype) != self.dtype:
                raise TQRError(f"{who}: every tensor must be of the handle's dtype")

    def update(self, R, W, tau, lddr=None, lddw=None, stream=None):
        """R <- R' in place (only its upper triangle is read or written), W <- the TSQRT V tiles, tau
        (q, mw) <- their taus; then the T pass of prepare(). Stream-ordered."""
        self._same("RowUpdate.update", R, W, tau)
        lddr = lddr or R.shape[-1]
        lddw = lddw or W.shape[-1]
        check(lib().tqr_update_rows(self.h, _ptr(R), lddr, _ptr(W), lddw, _ptr(tau), _stream_handle(stream)),
              "tqr_update_rows")

    def prepare(self, W, tau, lddw=None, stream=None):
        """Rebuild the apply's T images from a stored update (W, tau). Stream-ordered."""
        self._same("RowUpdate.prepare", W, tau)
        lddw = lddw or W.shape[-1]
        check(lib().tqr_update_prepare(self.h, _ptr(W), lddw, _ptr(tau), _stream_handle(stream)), "tqr_update_prepare")

    def apply(self, W, Ctop, Cnew, trans=True, nrhs=None, lddw=None, lddct=None, lddcn=None, stream=None):
        """[Ctop (nrhs, lddct); Cnew (nrhs, lddcn)] <- Q_u^T (trans) or Q_u of the pair, in place."""
        self._same("RowUpdate.apply", W, Ctop, Cnew)
        lddw = lddw or W.shape[-1]
        lddct = lddct or Ctop.shape[-1]
        lddcn = lddcn or Cnew.shape[-1]
        nrhs = Ctop.shape[0] if nrhs is None else nrhs
        check(lib().tqr_update_apply_q(self.h, 1 if trans else 0, _ptr(W), lddw, _ptr(Ctop), lddct, _ptr(Cnew), lddcn, nrhs,
                                       _stream_handle(stream)), "tqr_update_apply_q")

    def lstsq(self, R, W, tau, D, Bnew, X, res=None, nrhs=None, lddr=None, lddw=None, lddd=None, lddb=None, lddx=None,
              stream=None):
        """One step of recursive least squares (tqr_update_lstsq): update(R, W, tau); (D, Bnew) <- Q_u^T
        of them; X <- R'^{-1} D; res (optional, nrhs running residual norms) <- sqrt(res^2 + |Bnew'|^2).
        D (nrhs, lddd) holds the top n rows of Q^T b so far, Bnew (nrhs, lddb) the new rows' right-hand
        sides, X (nrhs, lddx) receives the solution over all rows so far. Stream-ordered."""
        self._same("RowUpdate.lstsq", R, W, tau, D, Bnew, X, res)
        lddr = lddr or R.shape[-1]
        lddw = lddw or W.shape[-1]
        lddd = lddd or D.shape[-1]
        lddb = lddb or Bnew.shape[-1]
        lddx = lddx or X.shape[-1]
        nrhs = D.shape[0] if nrhs is None else nrhs
        pres = None if res is None else _ptr(res)
        check(lib().tqr_update_lstsq(self.h, _ptr(R), lddr, _ptr(W), lddw, _ptr(tau), _ptr(D), lddd, _ptr(Bnew), lddb, nrhs,
                                     _ptr(X), lddx, pres, _stream_handle(stream)), "tqr_update_lstsq")

    def __del__(self):
        try:
            if self.h:
                lib().tqr_update_destroy(self.h)
        except Exception:
            pass


def update_plan(n, mw, b):
    """Host-only: (nlevels, npanel, nupdate, nlaunch) of a RowUpdate of these arguments (tqr_update_plan)."""
    nl, np_, nu, nla = _I(), _I(), _I(), _I()
    check(lib().tqr_update_plan(n, mw, b, ctypes.byref(nl), ctypes.byref(np_), ctypes.byref(nu), ctypes.byref(nla)),
          "tqr_update_plan")
    return nl.value, np_.value, nu.value, nla.value


def update_level_items(n, mw, b, level):
    """Host-only: the items of one level of the update's schedule as (type, strip, l, j, k) tuples, the
    TSQRT items (type 2, j = k) first, then the TSMQR strip items (type 3) (tqr_update_level_items)."""
    cnt = lib().tqr_update_level_items(n, mw, b, level, None, 0)
    if cnt < 0:
        check(cnt, "tqr_update_level_items")
    buf = (_I * (4 * max(cnt, 1)))()
    got = lib().tqr_update_level_items(n, mw, b, level, buf, cnt)
    if got < 0:
        check(got, "tqr_update_level_items")
    return [(buf[4 * i] & 0xff, buf[4 * i] >> 8, buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]) for i in range(cnt)]


# ---- single tile ops (host pointers; the reference's SGEQRF/SLARFT/STSQRF/SSSRFT) --------
def _tile_ptr(M, r, c, b):
    """pointer to tile (r,c) of a column-major matrix stored as (n, m) numpy array"""
    ldm = M.shape[1]
    return _P(M.ctypes.data + (c * b * ldm + r * b) * M.itemsize)


def tile_geqrt(M, b, tau):
    check(lib().tqr_tile_geqrt(_dtype_code(M.dtype), _tile_ptr(M, 0, 0, b), _ptr(tau), b, M.shape[1]), "tile_geqrt")


def tile_unmqr(M, b, tau):
    """C = tile (0,1) updated with V, tau of tile (0,0)"""
    check(lib().tqr_tile_unmqr(_dtype_code(M.dtype), _tile_ptr(M, 0, 1, b), _tile_ptr(M, 0, 0, b), _ptr(tau), b,
                               M.shape[1]), "tile_unmqr")


def tile_tsqrt(M, b, tau):
    """[R tile (0,0); tile (1,0)]"""
    check(lib().tqr_tile_tsqrt(_dtype_code(M.dtype), _tile_ptr(M, 0, 0, b), _tile_ptr(M, 1, 0, b), _ptr(tau), b,
                               M.shape[1]), "tile_tsqrt")


def tile_tsmqr(M, b, tau):
    """V = tile (1,0), A = tile (0,1), B = tile (1,1)"""
    check(lib().tqr_tile_tsmqr(_dtype_code(M.dtype), _tile_ptr(M, 1, 0, b), _tile_ptr(M, 0, 1, b),
                               _tile_ptr(M, 1, 1, b), _ptr(tau), b, M.shape[1]), "tile_tsmqr")


def flops(m, n):
    """Algorithmic Householder QR flop count 2mn^2 - 2n^3/3 (m >= n)."""
    if m >= n:
        return 2.0 * m * n * n - 2.0 * n ** 3 / 3.0
    return 2.0 * n * m * m - 2.0 * m ** 3 / 3.0
