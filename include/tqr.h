/*
 * tqr — MI355X-native flat-tree tiled Householder QR (libtqr.so), the native API.
 *
 * Same algorithm and output layout as the reference (s10m/GPU-Tiled-QR-Decomposition):
 *   * A is column-major m x n with leading dimension ldm, factorised in place: the global
 *     upper triangle is R, the strict lower part of each diagonal tile (k,k) holds the
 *     unit-lower GEQRT V, and every tile (i,k), i>k, holds the dense TSQRT V_B
 *     (reference qrdecomp.c:522-523, 683-684);
 *   * Householder conventions of qrdecomp.c:1201-1272 (sign(0)=+1, v0=1, tau=2/v'v, tau=2
 *     for length-1 and zero columns).
 * The tile size b must divide m and n; b in {16, 32, 64, 128, 256}. The leading dimension is
 * bounded by the engine's 32-bit buffer offsets: 32 * ldm * sizeof(element) < 2^31, i.e.
 * ldm <= 8,388,607 (fp64) / 16,777,215 (fp32); larger values return TQR_EINVAL.
 *
 * tau, device API: "compact" m x kmax column-major array (kmax = min(m,n)/b), column k holds
 * the b*(p-k) taus of panel k in rows k*b .. m-1 — exactly column k*b of the reference's
 * m x n tau matrix (qrdecomp.c:392,420,435). The host API returns the reference's m x n
 * tau matrix (other entries untouched).
 *
 * Status codes: 0 = ok, negative = error (see tqr_strerror).
 */
#ifndef TQR_H
#define TQR_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum tqr_status {
    TQR_OK = 0,
    TQR_EINVAL = -1,   /* bad sizes / tile size / pointers */
    TQR_ENOMEM = -2,   /* device or host allocation failed */
    TQR_EHIP = -3,     /* a HIP runtime call failed */
    TQR_ENODEV = -4,   /* no usable gfx950 device */
    TQR_ERCCL = -5     /* an RCCL call failed */
};
enum tqr_dtype { TQR_F32 = 0, TQR_F64 = 1 };

const char* tqr_strerror(int status);
const char* tqr_version(void);

/* ---- plans: allocate once, execute many times (no allocation inside execute) ---------- */
typedef struct tqr_plan tqr_plan;

/* Plan a factorisation of an m x n matrix of `dtype` with tile size b on the current HIP
 * device. */
int tqr_plan_create(tqr_plan** plan, int m, int n, int b, int dtype);
/* Execution engines. Both compute the same factorisation — the same tile operations over the same
 * DAG, each within the project's bound of the reference (fp64 1e-11 scaled, fp32 1e-3) — but with
 * different kernels: reflector-group sizes and summation orders inside a tile operation differ (and
 * fp32 storage runs fp32 MFMA chains in the flow engine only), so their results agree to rounding,
 * NOT in bits. Measured on an MI355X on Gaussian inputs from 64 x 64, b = 16 to 768 x 768, b = 256, in
 * both dtypes: 70 - 95 % of the entries of the factorised matrix and about half of the written taus
 * differ in their last bits (max difference 7e-14 fp64, 6e-5 fp32; DESIGN.md §4.1 has the counts).
 * Each engine on its own is bit-reproducible: the bits do not depend on ldda, the base address, the
 * stream, the profile switch, or on which threads and streams share the plan.
 *   TQR_ENGINE_FLOW  — one persistent dataflow launch: workgroups pull GEQRT/TSQRT panel tasks
 *                      and fused UNMQR/TSMQR column chains from a static topological list and
 *                      synchronise through progress counters (default);
 *   TQR_ENGINE_WAVES — the host scheduler's BFS waves of the reference DAG, two batched launches
 *                      per wave (panel tasks, update strips) on two HIP streams joined by events:
 *                      the level-synchronous multi-stream form of the reference's cudaQRFull
 *                      sketch (src/gpucalc.cu:1801-1877).
 * TQR_ENGINE_DEFAULT = FLOW unless the environment sets TQR_ENGINE=waves. */
enum tqr_engine { TQR_ENGINE_DEFAULT = -1, TQR_ENGINE_WAVES = 0, TQR_ENGINE_FLOW = 1 };
int tqr_plan_create_engine(tqr_plan** plan, int m, int n, int b, int dtype, int engine);
/* Partial factorisation ("capped plan"): factorise only the leading `steps` tile columns of the
 * m x n matrix (1 <= steps <= min(m,n)/b, else TQR_EINVAL) and apply Q^T of those steps to every
 * other column. On exit of tqr_plan_execute, with s = steps:
 *   * columns 0 .. s*b-1 hold R, the GEQRT V and the TSQRT V_B of steps 0 .. s-1, as a whole
 *     factorisation leaves them: they are a complete factorisation of the m x s*b matrix A[:, :s*b],
 *     on which tqr_apply_*, tqr_trsm_r and tqr_lstsq work unchanged;
 *   * rows 0 .. s*b-1 of the columns >= s*b hold R12 (final);
 *   * rows >= s*b of the columns >= s*b hold the updated trailing block — the lower rows of
 *     Q_s^T A[:, s*b:], no reflectors: the block-elimination form [R11 R12; 0 S]. An ordinary plan
 *     of (m - s*b) x (n - s*b) executed in place on S (base pointer offset, same ldda, its own tau
 *     array) completes the factorisation;
 *   * dtau_compact is m x s: columns 0 .. s-1 of the usual compact layout.
 * So a capped plan over [A | B] (steps = A's tile columns) factorises A and leaves Q^T B in B's
 * place, and one over [A | I] leaves Q^T explicitly, both in the one pipelined launch.
 * The plan always runs the persistent dataflow engine, whatever TQR_ENGINE says, and is a
 * single-GPU device-pointer plan: every tqr_dist_* call on it returns TQR_EINVAL. Arguments are
 * validated as by tqr_plan_create, before any device call. With steps == min(m,n)/b the task list
 * is exactly tqr_plan_create's. tqr_plan_set_tasks, tqr_plan_info and tqr_plan_debug_workspace
 * (k < steps) work on the capped plan's own list. */
int tqr_plan_create_steps(tqr_plan** plan, int m, int n, int b, int dtype, int steps);
/* The steps of a plan: the cap of a tqr_plan_create_steps plan, min(m,n)/b for every other plan. */
int tqr_plan_steps(const tqr_plan* plan);
void tqr_plan_destroy(tqr_plan* plan);

/* Factorise device matrix dA (ldda >= m) in place; dtau_compact is device memory of
 * m * kmax elements of the same dtype. `stream` is a hipStream_t (NULL = default stream).
 * Stream-ordered: returns once all work is enqueued.
 * A plan owns one set of progress counters and panel workspaces, so its executions are
 * serialised: calls from several host threads are mutually excluded while they enqueue, and
 * each execute's stream first waits for the plan's previous execute (whatever its stream). Two
 * executes of one plan never overlap on the GPU; use one plan per concurrent factorisation. */
int tqr_plan_execute(tqr_plan* plan, void* dA, int ldda, void* dtau_compact, void* stream);

/* Synchronise `stream` and report whether the last execute completed (the persistent engine
 * bounds every dependency wait and reports a timeout here instead of hanging). */
int tqr_plan_status(tqr_plan* plan, void* stream);
/* engine: 1 = persistent dataflow (default; TQR_ENGINE=waves selects 0 = wave-batched
 * launches), ntasks: task-list length, est_order: 1 if the start-time-estimate order was
 * used (else step-major), grid: workgroups of the persistent launch. */
int tqr_plan_info(const tqr_plan* plan, int* engine, int* ntasks, int* est_order, int* grid);

/* Host-only check of the persistent engine's task list for an M x N tile grid (no GPU):
 * number of tasks and whether the estimated-start-time order is topological. */
int tqr_flow_plan_check(int M, int N, int b, int seglen, int* ntasks, int* est_order);
/* Columns of one chain strip of the persistent engine (a tile column is split into
 * ceil(b / width) strips; one workgroup updates one strip). */
int tqr_flow_strip_width(void);
/* Host-only: the persistent engine's task list for an M x N tile grid, 4 ints per task
 * {type | strip << 8, l, m, k} (chains: type 4, l = i0 | i1 << 16, k = step | segment << 16);
 * returns the number of tasks (writes at most `cap`). */
int tqr_flow_plan_export(int M, int N, int b, int seglen, int* items, int cap);
/* Whole-line strips of the fp64 engine (tiles of 256): the layout, 0 standard or 1 whole lines, in
 * which the chain strips of tile (i, j) — i >= k (i = k: the UNMQR element), j > k — are stored at
 * step k of a p x q tile plan with `steps` steps (0 = all), where the plan has them on
 * (TQR_STRIP_LINES); the function the kernel evaluates. A tile's next reader expects what this gives
 * for its last writer; 1 only for tiles that a TSMQR element of step k + 1 reads next, so the
 * caller, the panel and the transfers see standard tiles only. TQR_EINVAL outside the plan.
 * tqr_flow_strip_offset: the byte offset, inside a wave's 16-column x 256-row block of a matrix with
 * leading dimension ld (elements), of the 16 bytes that lane `lane` of the wave moves in its access
 * of row pair `pair` (0..31) under that layout. */
int tqr_flow_strip_layout(int p, int q, int steps, int i, int j, int k);
long tqr_flow_strip_offset(int layout, int pair, int lane, long ld);
/* Host-only: the task list of any plan, in the same 4-int form — exactly the list
 * tqr_plan_create / tqr_dist_plan_create builds for the spec (nxc = 0), or the host-pointer API's
 * list with nxc upload / download tasks per tile column (nxc 1..255, one-GPU plans only).
 *   M, N    tiles;  dtype: tqr_dtype;  seglen <= 0: the plan's default segment length;
 *   world   ranks, full != 0: each rank's launch covers its whole device (the multi-rank defaults
 *           depend on both);  rank < 0: the global list, else that rank's partition of it;
 *   tcol    with nxc > 0: one tile column's upload time in chain elements.
 * The environment's task-list knobs apply as at plan creation. Returns the number of tasks
 * (writes at most `cap`), or TQR_EINVAL. tqr_flow_plan_export and the *_plan_check functions
 * are this call for fp64, full = 1 and a caller-given seglen >= 1. */
typedef struct tqr_flow_list_spec {
    int M, N, b, dtype, seglen, world, rank, full, nxc;
    double tcol;
} tqr_flow_list_spec;
int tqr_flow_list_export(const tqr_flow_list_spec* spec, int* items, int cap);
/* The same for a capped plan (tqr_plan_create_steps of M*b x N*b with `steps`): exactly the list
 * that plan builds. steps <= 0: uncapped, identical to tqr_flow_list_export. A capped spec must have
 * world == 1, nxc == 0 and steps <= min(M, N), else TQR_EINVAL. */
int tqr_flow_list_export_steps(const tqr_flow_list_spec* spec, int steps, int* items, int cap);
/* Replace the persistent engine's task order (the same tasks as the plan's list, 4 ints each as
 * tqr_flow_plan_export gives them, e.g. from an offline list scheduler): rejected with
 * TQR_EINVAL unless it is a permutation of the plan's tasks that is topological for every
 * in-task wait (the engine's deadlock-freedom condition). Single-GPU flow plans only. */
int tqr_plan_set_tasks(tqr_plan* plan, const int* items, int n);
/* Diagnostics: the task list the persistent engine's workgroups dequeue, read back from the device
 * in order (4 ints per task, at most `cap` tasks written). Returns the number of tasks of the list
 * (this rank's), or TQR_EINVAL (no flow plan). */
int tqr_plan_get_tasks(tqr_plan* plan, int* items, int cap);
/* Host-only: 1 if `items` is topological for the engine's waits on an M x N tile grid, else 0. */
int tqr_flow_order_check(int M, int N, int b, const int* items, int n);
/* Diagnostics: copy the persistent engine's panel workspace of step k (the reflector groups'
 * operand images, DESIGN.md "Data layout") to host memory; returns its size in bytes. */
int tqr_plan_debug_workspace(const tqr_plan* plan, int k, void* host, size_t bytes);

/* Per-launch statistics of the last execute (filled when the plan was created with
 * tqr_plan_set_profile(plan, 1)): number of kernel launches and the summed device time of
 * the trailing-update (TSMQR/UNMQR) and panel (GEQRT/TSQRT) kernels in ms. */
int tqr_plan_set_profile(tqr_plan* plan, int on);
int tqr_plan_stats(const tqr_plan* plan, int* nlaunch_update, double* ms_update, int* nlaunch_panel,
                   double* ms_panel);

/* Number of flat-tree tasks (reference calcTotalTasks, src/gpucalc.cu:1546, for all m,n). */
long tqr_total_tasks(int m, int n, int b);

/* ---- apply: C <- Q^T C or C <- Q C with the factors of a finished factorisation -------------
 * (the ormqr to the plan's geqrf). dA, ldda and dtau_compact are what tqr_plan_execute left on the
 * device: R, the V tiles and the compact tau; the apply only reads them. Of dA, prepare and apply_q
 * use as values only the elements strictly below the diagonal, in tile columns k < kmax (the V of the
 * GEQRT and TSQRT tiles): R on and above the diagonal of a diagonal tile is loaded with its column
 * and replaced by the unit-lower trapezoid's 0 / 1 through a select, and the tiles above the block
 * diagonal are never read — whatever R holds, inf and NaN included, cannot reach C (the mirror image
 * of tqr_trsm_r's rule below). Q is the full m x m orthogonal factor (Q^T A = [R; 0]). C is m x nrhs, column-major, of the handle's dtype, with
 * leading dimension lddc >= m; nrhs >= 1 need not be a multiple of anything. Rows >= m and columns
 * >= nrhs of C's allocation are not touched. ldda and lddc obey the library's leading-dimension
 * bound (above).
 *   TQR_TRANS:   for k = 0 .. kmax-1: C_k <- UNMQR(V_kk) C_k, then for l = k+1 .. p-1:
 *                [C_k; C_l] <- TSMQR(V_lk) [C_k; C_l] — what the factorisation did to a trailing
 *                column (C_i = row tile i of C, p = m/b);
 *   TQR_NOTRANS: the exact reverse (k descending, l descending then the UNMQR tile, each block
 *                reflector untransposed), so Q (Q^T C) = C. Q itself is the apply to an identity.
 * fp32 handles load and store float and compute in fp64, as the tile updates of the single-tile API.
 * One workgroup per 64 columns of C walks the whole reflector sequence serially; workgroups never
 * wait for each other (the kernel has no counters or flags), so a narrow C uses few CUs — the
 * "pipelined apply" below (tqr_apply_pipe_q, tqr_lstsq_pipe) computes the same bits on one CU per step.
 * Single-GPU factorisations only: the packed per-rank storage of a tqr_dist_plan is not supported.
 *
 * create validates as tqr_plan_create (before any device call) and allocates the T workspace:
 * one 32 x 33 fp64 image (b < 32: b x (b+1)), padded to whole KiB, per 32-reflector group of every
 * tile (l,k), l >= k, k < kmax — tqr_apply_workspace_bytes. prepare and apply_q allocate nothing.
 * prepare rebuilds the T factors from V and tau (once per factorisation); apply_q before the first
 * successful prepare returns TQR_EINVAL. Both are stream-ordered and return once enqueued.
 * Ordering on one handle: an apply_q's stream first waits for the last prepare (an event), and a
 * prepare's stream first waits for every apply_q enqueued since the previous prepare — a prepare
 * never overlaps an apply of its handle on the GPU, whatever the streams. Applies only read the
 * workspace: two apply_q calls of one handle on different streams may overlap. The caller keeps
 * dA and dtau unchanged while work that reads them is in flight, as with any device buffer. */
typedef struct tqr_apply tqr_apply;
enum tqr_trans { TQR_NOTRANS = 0, TQR_TRANS = 1 };
int tqr_apply_create(tqr_apply** ap, int m, int n, int b, int dtype);
size_t tqr_apply_workspace_bytes(const tqr_apply* ap);
int tqr_apply_prepare(tqr_apply* ap, const void* dA, int ldda, const void* dtau_compact, void* stream);
int tqr_apply_q(tqr_apply* ap, int trans, const void* dA, int ldda, void* dC, int nrhs, int lddc, void* stream);
void tqr_apply_destroy(tqr_apply* ap);

/* ---- solve: triangular solves with R, and both least-squares directions --------------------
 * tqr_trsm_r: X <- R^{-1} X (TQR_NOTRANS) or X <- R^{-T} X (TQR_TRANS), in place, R = the upper
 * triangle of the leading n x n block of dA as tqr_plan_execute left it. Only elements (i, j) with
 * i <= j < n are read as values: everything below the diagonal of the diagonal tiles (the GEQRT V)
 * is ignored, whatever it holds (it is masked by a select, so an inf or NaN there cannot leak). dA is
 * not written. X is n x nrhs, column-major, of `dtype`, lddx >= n; nrhs >= 1 need not be a multiple
 * of anything. Rows >= n and columns >= nrhs of X's allocation are not touched. b in {16, 32, 64,
 * 128, 256} must divide n; ldda >= n and lddx obey the library's leading-dimension bound (above).
 * No handle, no workspace, no prepare pass: the call is stream-ordered and returns once enqueued.
 * Every argument error returns TQR_EINVAL before any device call; a missing or non-gfx950 device
 * returns TQR_ENODEV after that validation.
 * Method: one workgroup per 64 columns of X walks the tile rows of R serially (k descending for R,
 * ascending for R^T); workgroups never wait for each other (the kernel has no counters or flags),
 * so a narrow X uses few CUs. Inside a tile the 32 x 32 diagonal blocks are solved by substitution,
 * dividing by R's own diagonal entries (no inverse is formed): the computed X satisfies the
 * componentwise substitution bound |op(R) X - Y| <= gamma_n (|op(R)| |X| + |Y|).
 * R is NOT checked for zero diagonal entries, and inf / NaN propagate as in BLAS trsm: a zero
 * diagonal gives inf or NaN in the rows that depend on it. fp32 storage loads and stores float and
 * computes in fp64; X is rounded to float whenever a tile row is stored.
 *
 * tqr_lstsq: LAPACK gels in both directions on a prepared apply handle with m >= n (else, or before
 * the first prepare, TQR_EINVAL). dA / ldda as given to tqr_apply_prepare. Everything is enqueued on
 * `stream`, nothing is allocated.
 *   TQR_NOTRANS: least squares, min |A x - b|_2 for every column. dB (m x nrhs, lddb >= m) is
 *                overwritten by Q^T B (tqr_apply_q), then rows 0 .. n-1 by X (tqr_trsm_r); rows
 *                n .. m-1 stay exactly as the apply left them. dres: NULL, or nrhs elements of the
 *                handle's dtype that receive |A x - b|_2 per column = the 2-norm of rows n .. m-1
 *                (0 when m == n). The norm is accumulated in fp64 in a fixed order (bit-reproducible)
 *                and is not scaled: squares of entries beyond about 1e154 in magnitude overflow to
 *                inf and entries below about 1e-154 are lost (fp32 storage: the whole float range is
 *                safe in the sum; a result beyond FLT_MAX rounds to inf).
 *   TQR_TRANS:   the minimum-norm solution of the underdetermined A^T x = c. On entry rows 0 .. n-1
 *                of dB hold c; rows n .. m-1 are ignored and zeroed by the call. Rows 0 .. n-1 become
 *                R^{-T} c (tqr_trsm_r), then dB <- Q dB (tqr_apply_q): on exit all m rows hold x.
 *                dres is not written. */
int tqr_trsm_r(int dtype, int trans, int n, int b, const void* dA, int ldda, void* dX, int nrhs, int lddx,
               void* stream);
int tqr_lstsq(tqr_apply* ap, int trans, const void* dA, int ldda, void* dB, int nrhs, int lddb, void* dres,
              void* stream);
/* tqr_lstsq_fused: least squares min |A x - b|_2 with the factorisation itself, in one stream-ordered
 * call and no apply handle. plan = tqr_plan_create_steps(m, n + r*b, b, dtype, n/b) with m >= n and
 * r >= 1; dAB (ldda >= m) holds [A | B]: A's n columns, then r tile columns of which the first nrhs
 * (1 <= nrhs <= r*b) are the right-hand sides. The call enqueues tqr_plan_execute (which factorises
 * A and leaves Q^T B in B's place), then tqr_trsm_r(TQR_NOTRANS) on rows 0 .. n-1 of B's nrhs
 * columns, then — dres: NULL, or nrhs elements of the plan's dtype — |A x - b|_2 per column from
 * rows n .. m-1, exactly as tqr_lstsq computes it (the same kernel, the same fixed summation order).
 * On exit: columns 0 .. n-1 and dtau_compact (m x n/b) are an ordinary factorisation of A (an apply
 * handle for (m, n) can be prepared on them); rows 0 .. n-1 of B's first nrhs columns hold X, their
 * rows n .. m-1 the rest of Q^T B. The padding columns nrhs .. r*b-1 are OVERWRITTEN: they are
 * updated like any column (by Q^T, not solved); columns are independent, so what they hold on entry
 * influences nothing else — they need not be initialised to anything in particular, but inf / NaN in
 * them stay in them. Nothing beyond the n + r*b columns is touched.
 * Everything is validated before any device call (TQR_EINVAL): a NULL plan, dAB or dtau_compact; a
 * plan not made by tqr_plan_create_steps; a plan without columns after its steps*b (no B); nrhs < 1
 * or nrhs > r*b; a bad ldda. Status of the launch: tqr_plan_status, as after tqr_plan_execute. */
int tqr_lstsq_fused(tqr_plan* plan, void* dAB, int ldda, void* dtau_compact, int nrhs, void* dres, void* stream);

/* ---- pipelined solve: tqr_trsm_r spread over workgroups, for narrow right-hand sides ----------
 * tqr_solve_trsm_r computes what tqr_trsm_r computes, bit for bit, and its semantics are
 * tqr_trsm_r's word for word: X <- R^{-1} X (TQR_NOTRANS) or X <- R^{-T} X (TQR_TRANS) in place, R
 * the upper triangle of the leading n x n block of dA; only elements (i, j) with i <= j < n are read
 * as values, everything below the diagonal of the diagonal tiles is masked by a select; dA is not
 * written; rows >= n and columns >= nrhs of X's allocation are not touched; a zero diagonal entry,
 * inf and NaN propagate exactly as there (the same operations in the same order); fp32 storage
 * computes in fp64 and rounds a tile row to float whenever it is stored.
 * Method: one workgroup per (64-column strip of X, tile row of R) instead of one per strip. The
 * workgroup of tile row i waits for each solved X_k it depends on (k > i, descending, for R; k < i,
 * ascending, for R^T), subtracts op(R)_ik X_k from its own rows, and finally solves against tile
 * (i,i) and publishes X_i through a flag in the handle's workspace — so a narrow X occupies n / b
 * CUs instead of one, and the serial chain is one tile update plus one diagonal tile per tile row.
 * With many strips (nrhs of the order of n) tqr_trsm_r already fills the device and is the faster
 * call (DESIGN.md §15 has the crossover); nothing here replaces it.
 * Work items are handed out by an atomic ticket in dependency order, so a workgroup only ever waits
 * for workgroups that are already running, however few fit on the device. Every wait is bounded
 * (5 s): on expiry the kernel sets the handle's error word and all its workgroups leave — it
 * cannot hang. tqr_solve_status synchronises `stream` and the handle's last call and returns
 * TQR_OK, or TQR_EHIP once after a wait timed out (X is then undefined; the handle stays usable).
 *
 * tqr_solve_create: a handle for n x n triangles of tile size b (b in {16, 32, 64, 128, 256} dividing
 * n) and `dtype`, for up to nrhs_max >= 1 right-hand sides. It owns tqr_solve_workspace_bytes of
 * device memory: the ticket counter, the error word and one flag per (strip, tile row) — 4 bytes
 * each, ceil(nrhs_max / 64) * (n / b) flags. Calls allocate nothing.
 * A handle's calls are serialised like a plan's executes: concurrent host threads are mutually
 * excluded while they enqueue, and each call's stream first waits for the handle's previous call
 * (whatever its stream), so two calls of one handle never overlap on the GPU; use one handle per
 * concurrent solve. Consecutive calls need no host synchronisation: flags carry a per-call epoch
 * and the ticket counter is re-armed in stream order.
 * Every argument error returns TQR_EINVAL before any device call: create with a bad dtype, a b
 * outside the list or not dividing n, n <= 0, nrhs_max < 1, or a shape whose grid would pass 2^31
 * workgroups; tqr_solve_trsm_r with a NULL handle or pointer, a bad trans, nrhs < 1 or > nrhs_max,
 * ldda or lddx below n or beyond the library's leading-dimension bound. A missing or non-gfx950
 * device is reported after that validation: tqr_solve_create then still returns a handle (without
 * device memory), and every tqr_solve_trsm_r on it returns TQR_ENODEV.
 *
 * tqr_solve_ticket (host only, no GPU): the work item (*strip, *row) of ticket `ticket` on T tile
 * rows and nstrips strips — the function the kernel itself evaluates. Tickets 0 .. T*nstrips-1 map
 * one to one onto the items, and every item a row waits for (rows above it for TQR_TRANS, below it
 * for TQR_NOTRANS, same strip) has a smaller ticket. Anything out of range returns TQR_EINVAL.
 *
 * tqr_lstsq_fused_solve: tqr_lstsq_fused with tqr_solve_trsm_r in place of tqr_trsm_r; same
 * arguments, same results bit for bit. sv must have been created for (steps * b, b, the plan's dtype)
 * with nrhs_max >= nrhs, else TQR_EINVAL (with tqr_lstsq_fused's own argument errors, before any
 * device call). Launch status: tqr_plan_status for the factorisation, tqr_solve_status for the solve.
 * tqr_lstsq's variant is tqr_lstsq_pipe ("pipelined apply" below): its apply strip, not the solve,
 * dominates a narrow call, so it takes the pipelined apply with this solve. */
typedef struct tqr_solve tqr_solve;
int tqr_solve_create(tqr_solve** sv, int n, int b, int dtype, int nrhs_max);
size_t tqr_solve_workspace_bytes(const tqr_solve* sv);
int tqr_solve_trsm_r(tqr_solve* sv, int trans, const void* dA, int ldda, void* dX, int nrhs, int lddx,
                     void* stream);
int tqr_solve_status(tqr_solve* sv, void* stream);
void tqr_solve_destroy(tqr_solve* sv);
int tqr_solve_ticket(int T, int nstrips, int trans, int ticket, int* strip, int* row);
int tqr_lstsq_fused_solve(tqr_plan* plan, tqr_solve* sv, void* dAB, int ldda, void* dtau_compact, int nrhs,
                          void* dres, void* stream);

/* ---- pipelined apply: tqr_apply_q spread over workgroups, for narrow right-hand sides ----------
 * tqr_apply_pipe_q computes what tqr_apply_q computes, bit for bit, and its semantics are
 * tqr_apply_q's word for word: dC <- Q^T dC (TQR_TRANS) or Q dC (TQR_NOTRANS) in place, Q the
 * orthogonal factor of the factorisation `ap` was last prepared on (dA / ldda as given to
 * tqr_apply_prepare; dA is not written); rows >= m and columns >= nrhs of C's allocation are not
 * touched; inf and NaN propagate exactly as there (the same operations on the same operands in the
 * same order); fp32 storage computes in fp64 and rounds a row tile to float whenever it is stored.
 * Method: one workgroup per (64-column strip of C, step k of the factorisation) instead of one per
 * strip. The workgroup of step k runs that step's UNMQR and its TSMQRs down the tile rows (up, for
 * Q), waiting for each row tile C_l until the step before it has released it, and releases it in
 * turn through a flag in the handle's workspace — a wavefront over (step, row tile) whose serial
 * chain is about p + 2 kmax tile operations (p = m / b, kmax = min(m, n) / b) instead of all
 * kmax p - kmax (kmax - 1) / 2 of them, on up to kmax CUs per strip instead of one.
 * Measured on an MI355X, fp64, 64 right-hand sides: 15.7 ms against tqr_apply_q's
 * 416.9 ms at 16384 x 16384, b = 256, and 2.59 against 18.3 ms at 4096 x 4096, b = 128; tqr_lstsq_pipe
 * 25.0 against tqr_lstsq's 542.9 ms, and 4.11 against 27.6 ms. No crossover was found up to nrhs = n:
 * at 16384 x 16384 the pipelined call is also the faster one for 1024, 4096 and 16384 columns (23.0,
 * 73.6 and 282.8 ms against 391.6, 397.5 and 422.7 ms). Beyond nrhs = n nothing was measured;
 * tqr_apply_q runs two workgroups per CU from 2 x 64 x (CU count) columns on, which this kernel
 * cannot, so prefer tqr_apply_q there until measured.
 * Work items are handed out by an atomic ticket in dependency order, so a workgroup only ever waits
 * for workgroups that are already running, however few fit on the device. Every wait is bounded
 * (5 s): on expiry the kernel sets the handle's error word and all its workgroups leave — it
 * cannot hang. tqr_apply_pipe_status synchronises `stream` and the handle's last call and returns
 * TQR_OK, or TQR_EHIP once after a wait timed out (C is then undefined; the handle stays usable).
 *
 * tqr_apply_pipe_create: a handle for m x n factorisations of tile size b and `dtype` (validated as
 * tqr_apply_create validates them), for up to nrhs_max >= 1 right-hand sides. It is independent of
 * any apply handle and owns tqr_apply_pipe_workspace_bytes of device memory: the ticket counter and
 * the error word (128 bytes with their padding) and one 4-byte flag per (strip, stored tile (l, k),
 * l >= k) — ceil(nrhs_max / 64) * (kmax p - kmax (kmax - 1) / 2) flags. Calls allocate nothing.
 * tqr_apply_pipe_q takes the pipelined handle and a prepared apply handle of the same (m, n, b,
 * dtype). Ordering: the call's stream first waits for ap's last prepare, and the call is recorded
 * among ap's applies, so a later tqr_apply_prepare waits for it — exactly as tqr_apply_q. The calls
 * of one tqr_apply_pipe are serialised like a tqr_solve's: concurrent host threads are mutually
 * excluded while they enqueue, and each call's stream first waits for the handle's previous call
 * (whatever its stream); use one handle per concurrent apply (any number may share one prepared
 * ap). Consecutive calls need no host synchronisation: flags carry a per-call epoch and the ticket
 * counter is re-armed in stream order.
 * Every argument error returns TQR_EINVAL before any device call: create with tqr_apply_create's
 * errors, nrhs_max < 1, or a shape whose grid of ceil(nrhs_max / 64) * kmax workgroups would pass
 * 2^31; tqr_apply_pipe_q with a NULL handle, ap or pointer, a bad trans, nrhs < 1 or > nrhs_max,
 * ldda or lddc below m or beyond the library's leading-dimension bound, an ap made for another
 * (m, n, b, dtype), or an ap that was never prepared. A missing or non-gfx950 device is reported
 * after that validation: tqr_apply_pipe_create then still returns a handle (without device
 * memory), and every call on it returns TQR_ENODEV.
 *
 * tqr_apply_pipe_ticket (host only, no GPU): the work item (*strip, *step) of ticket `ticket` on
 * kmax steps and nstrips strips — the function the kernel itself evaluates. Tickets
 * 0 .. kmax*nstrips-1 map one to one onto the items, and the one item a step waits for (step - 1
 * for TQR_TRANS, step + 1 for TQR_NOTRANS, same strip) has a smaller ticket. Anything out of range
 * returns TQR_EINVAL and writes nothing.
 *
 * tqr_apply_pipe_form_q: Q itself. Writes Q[:, 0:ncols], 1 <= ncols <= min(m, nrhs_max), Q the m x m
 * orthogonal factor of the factorisation `ap` was last prepared on, into dQ (m x ncols, column-major,
 * lddq >= m, the handle's dtype): ncols = min(m, n) is the thin Q, ncols = m the full one. Rows >= m
 * and columns >= ncols of the allocation are not touched. dQ is output-only: no byte of it is read
 * before this call has written it, so what it holds on entry does not matter, inf and NaN included —
 * no identity is allocated, filled or loaded. The call is tqr_apply_pipe_q(TQR_NOTRANS) on E = the
 * first ncols columns of I_m without the work on E's zero blocks: the 64-column strip s of E is zero
 * below row tile jhi(s) (the tile of its last column), and step k of Q touches only row tiles >= k, so
 * the steps k > jhi(s) of that strip would turn zeros into zeros and are never issued; a row tile's
 * first operation takes E's 0 / 1 pattern from registers. In tile operations nstrips * sum_k (p - k)
 * becomes sum_k (p - k) * #{strips with jhi(s) >= k}: 0.67 of them for a square thin Q, towards 0.5 for
 * a tall one.
 * Which parts of dA are read (the mirror of tqr_apply_q's rule that R is never read as a value): tile
 * (l, k) of dA and its T images are read only if k * b <= ncols - 1. With all of V and T finite, dQ is
 * equal as values to tqr_apply_pipe_q(TQR_NOTRANS) on a dQ pre-filled with E — the same operations in
 * the same order on the non-zero data; a skipped operation would have produced zeros. The sign of a
 * zero is left free by this contract (on an MI355X the bytes came out equal in every case tested,
 * DESIGN.md §17). With inf or NaN in a tile this call does not read the two differ: the apply to E
 * spreads them, this call never sees them.
 * Everything else is tqr_apply_pipe_q's, word for word: the same handle and no further workspace (the
 * flags of tqr_apply_pipe_create cover every (strip, tile) used), the same ordering against ap's
 * prepare and the handle's previous call, the same epochs, bounded waits and tqr_apply_pipe_status;
 * TQR_EINVAL before any device call for every argument error — tqr_apply_pipe_q's, and ncols < 1,
 * ncols > m or ncols > nrhs_max; TQR_ENODEV after validation without a gfx950.
 * Measured on an MI355X, fp64, thin Q (tools/apply_bench.py --formq), against the fill
 * of an identity plus tqr_apply_pipe_q on it, and against tqr_apply_q on it: 16384 x 16384, b = 256:
 * 196.2 ms against 0.3 + 282.6 ms and 423.6 ms (0.67 of the tile operations); 4096 x 4096, b = 128:
 * 4.71 ms against 0.03 + 6.17 ms and 18.90 ms (0.68); 65536 x 16384, b = 256: 1060.1 ms against
 * 1.3 + 2092.0 ms and 3030.1 ms (0.53). The call also saves the m x ncols identity itself.
 * tqr_apply_pipe_form_q_items (host only): the number of work items, which is the grid —
 * sum over the steps k < kmax with k * b <= ncols - 1 of ceil(ncols / 64) - floor(k * b / 64).
 * tqr_apply_pipe_form_q_ticket (host only): the work item (*strip, *step) of ticket `ticket` — the
 * function the kernel itself evaluates. Tickets run step-descending, over a step's strips s >=
 * floor(step * b / 64) only; they map one to one onto the items, and the one item a step waits for
 * (step + 1 of the same strip, unless the step is the strip's first) has a smaller ticket. For both,
 * anything out of range (kmax < 1, b outside {16, 32, 64, 128, 256}, ncols < 1, a ticket outside
 * 0 .. items-1, a NULL output) returns TQR_EINVAL and writes nothing.
 *
 * tqr_lstsq_pipe: tqr_lstsq with tqr_apply_pipe_q in place of tqr_apply_q and tqr_solve_trsm_r in
 * place of tqr_trsm_r, both directions; same arguments, same results bit for bit (X, the rest of
 * Q^T B, the zeroed rows of TQR_TRANS, dres). pp must match ap as above; sv must have been created
 * for (n, b, dtype) with nrhs_max >= nrhs, else TQR_EINVAL (with tqr_lstsq's own argument errors,
 * before any device call). Launch status: tqr_apply_pipe_status and tqr_solve_status. */
typedef struct tqr_apply_pipe tqr_apply_pipe;
int tqr_apply_pipe_create(tqr_apply_pipe** pp, int m, int n, int b, int dtype, int nrhs_max);
size_t tqr_apply_pipe_workspace_bytes(const tqr_apply_pipe* pp);
int tqr_apply_pipe_q(tqr_apply_pipe* pp, tqr_apply* ap, int trans, const void* dA, int ldda, void* dC, int nrhs,
                     int lddc, void* stream);
int tqr_apply_pipe_status(tqr_apply_pipe* pp, void* stream);
void tqr_apply_pipe_destroy(tqr_apply_pipe* pp);
int tqr_apply_pipe_ticket(int kmax, int nstrips, int trans, int ticket, int* strip, int* step);
int tqr_apply_pipe_form_q(tqr_apply_pipe* pp, tqr_apply* ap, const void* dA, int ldda, void* dQ, int ncols, int lddq,
                          void* stream);
int tqr_apply_pipe_form_q_items(int kmax, int b, int ncols);
int tqr_apply_pipe_form_q_ticket(int kmax, int b, int ncols, int ticket, int* strip, int* step);
int tqr_lstsq_pipe(tqr_apply_pipe* pp, tqr_solve* sv, tqr_apply* ap, int trans, const void* dA, int ldda, void* dB,
                   int nrhs, int lddb, void* dres, void* stream);

/* ---- batched: many same-shape factorisations in one call --------------------------------------
 * tqr_batch_execute factorises `batch` matrices of one shape (m, n, b, dtype) in place, each exactly
 * as tqr_plan_execute leaves one: R, the GEQRT V, the TSQRT V_B and the compact tau.
 * Layout: matrix i lives at dA + i * strideA elements, column-major with leading dimension ldda (one
 * ldda for all); its compact tau (m x kmax) at dtau_compact + i * strideTau elements.
 * Bit contract: matrix i has the bytes of a TQR_ENGINE_WAVES plan of (m, n, b, dtype) executed on
 * that matrix alone. The bytes do not depend on batch, the group size (below), the strides, the base
 * address or the stream. Bytes outside the matrices are not touched: rows >= m, the gaps between
 * matrices, columns >= n; of a compact tau only what a plan's execute writes.
 * Use of the other handles: because of the bit contract every handle of this library works on a
 * batch member unchanged, through an offset base pointer — tqr_apply_* (prepare on dA + i * strideA,
 * ldda, dtau_compact + i * strideTau), tqr_trsm_r, tqr_lstsq*, the pipelined solve and apply, and
 * tqr_apply_pipe_form_q. For all members in one call: tqr_batch_apply_* and tqr_batch_trsm_r below
 * ("batched apply and solve"), with the per-member calls' bytes.
 * Method: the wave engine runs every BFS wave of the reference DAG as two launches (panel tasks,
 * update strips; tqr_engine above) whose workgroups are independent of each other. The batched call
 * issues the same launches with the matrix as a second grid dimension, so the launch count is that
 * of one matrix and each launch holds batch times the workgroups. It uses two side streams joined to
 * the caller's stream by events, as a wave plan does.
 * Measured on an MI355X, fp64 (tools/batch_bench.py), against a loop of
 * tqr_plan_execute on one wave plan and on one flow plan in the same run: 64 matrices of 512 x 512,
 * b = 64: 2.42 ms against 130.9 and 68.1 ms; 1024 of them: 22.3 ms against 2061 and 1092 ms; 256
 * matrices of 1024 x 1024, b = 128: 21.6 ms against 1187 and 533 ms; 256 of 4096 x 256, b = 128: 16.2
 * ms against 1800 and 372 ms. For ONE matrix tqr_plan_execute on the default (flow) engine is the
 * faster call (1.07 against 1.97 ms at 512 x 512, 1.46 against 6.71 ms at 4096 x 256); from 16
 * matrices on the batched call was faster at every point measured. Matrices beyond 1024 x 1024 were
 * not measured; one large enough to fill the device alone gains nothing from a batch.
 * Workspace and groups: every matrix in flight needs the wave engine's T workspace, one 32 x 33 fp64
 * image (b < 32: b x (b+1)) padded to whole KiB per 32-reflector group of every tile (l, k), k < kmax:
 * (m/b) * kmax * (b / min(b, 32)) images. The batch therefore runs in groups of
 *   group = min(batch, 65535, max(1, ws_limit / bytes per matrix))
 * matrices, one group after another on the same streams (the last group may be smaller); ws_limit
 * == 0 means 1 GiB. tqr_batch_workspace_bytes = group * bytes per matrix, allocated by create;
 * execute allocates nothing. tqr_batch_group returns group (a NULL handle: TQR_EINVAL, and 0 bytes).
 * Strides (elements): with batch == 1 strideA is ignored; else one of two forms, anything else is
 * TQR_EINVAL:
 *   stacked          strideA >= (n-1) * ldda + m: one matrix after the other;
 *   row-interleaved  strideA >= m and (batch-1) * strideA + m <= ldda: the matrices are row blocks of
 *                    one array under a common ldda — with strideA == m the row domains of one tall
 *                    (batch * m) x n matrix.
 * strideTau >= m * kmax always.
 * Ordering: as a plan's executes. Concurrent host threads are mutually excluded while they enqueue,
 * and each execute's stream first waits for the handle's previous execute, whatever its stream; two
 * executes of one handle never overlap on the GPU. Stream-ordered: returns once all is enqueued.
 * Errors: TQR_EINVAL before any device call for tqr_plan_create's own argument errors, batch < 1, a
 * NULL handle or pointer, ldda < m or beyond the library's leading-dimension bound, and bad strides.
 * A missing or non-gfx950 device is reported after that validation: tqr_batch_create then still
 * returns a handle (without device memory; group and workspace_bytes answer), and every
 * tqr_batch_execute on it returns TQR_ENODEV.
 * tqr_batch_plan (host only, no GPU): the grouping and launch count create would choose — *group,
 * *ngroups = ceil(batch / group), *nlaunch = ngroups * (the non-empty panel launches plus the
 * non-empty update launches of one wave plan). Outputs may be NULL. Arguments out of range return
 * TQR_EINVAL and write nothing. */
typedef struct tqr_batch tqr_batch;
int tqr_batch_create(tqr_batch** bt, int m, int n, int b, int dtype, int batch, size_t ws_limit);
size_t tqr_batch_workspace_bytes(const tqr_batch* bt);
int tqr_batch_group(const tqr_batch* bt); /* matrices per launch group */
int tqr_batch_execute(tqr_batch* bt, void* dA, int ldda, long long strideA, void* dtau_compact, long long strideTau,
                      void* stream);
void tqr_batch_destroy(tqr_batch* bt);
int tqr_batch_plan(int m, int n, int b, int dtype, int batch, size_t ws_limit, int* group, int* ngroups, int* nlaunch);

/* ---- batched apply and solve: Q, Q^T, form-Q, the solve with R and least squares on a whole batch ---
 * What tqr_apply_* / tqr_trsm_r / tqr_lstsq do on one factorisation, on every member of a batch that
 * tqr_batch_execute factorised, in the launches of one member: a loop over the members issues 3 * batch
 * launches of one or two workgroups each (per 64 right-hand sides), the batched call issues 3 launches
 * with the member as a second grid dimension.
 * Layouts: member i of A and of the compact taus sits where tqr_batch_execute put it — dA + i * strideA
 * under ldda, dtau_compact + i * strideTau, the same two stride forms for strideA, strideTau >= m * kmax
 * always. C (m x nrhs), Q (m x ncols), B (m x nrhs) and X (n x nrhs) take the same two forms with their
 * own row and column counts, under their own leading dimension ld >= rows:
 *   stacked          stride >= (cols-1) * ld + rows;
 *   row-interleaved  stride >= rows and (batch-1) * stride + rows <= ld.
 * With batch == 1 the strides are ignored. tqr_batch_trsm_r's A is the leading n x n of a member: ldda
 * >= n and the forms with rows = cols = n (every layout tqr_batch_execute accepts for m >= n is one).
 * dres member i is nrhs elements at dres + i * strideRes; strideRes >= nrhs when batch > 1; dres may be
 * NULL (strideRes is then not looked at). Stride arithmetic is in 64 bits on the base pointers; inside a
 * member the 32-bit offset rules and the leading-dimension bound of the per-member calls hold.
 * Bit contract: member i has the bytes of the per-member call on it alone, because the same kernel
 * body runs on the same operands behind a per-member pointer offset:
 *   tqr_batch_apply_q   tqr_apply_q on a handle prepared on member i;
 *   tqr_batch_trsm_r    tqr_trsm_r;
 *   tqr_batch_lstsq     tqr_lstsq: X, the rest of Q^T B, the zeroed rows of TQR_TRANS, dres (TQR_NOTRANS
 *                       only, as there);
 *   tqr_batch_form_q    tqr_apply_q(TQR_NOTRANS) on a buffer holding the first ncols columns of I_m,
 *                       1 <= ncols <= m (ncols = min(m, n): the thin Q; ncols = m: the full one).
 * tqr_batch_form_q is output-only: dQ need not be initialised — the call fills the identity's columns
 * itself and then applies Q; the work on the identity's zero blocks is done, as in tqr_tsqr_form_q (not
 * skipped as in tqr_apply_pipe_form_q). The bytes do not depend on batch, the strides, the base address
 * or the stream. Nothing outside the members is written: rows beyond a member, the gaps between
 * members, columns >= nrhs or ncols. What is read as a value is the per-member calls' rule, word for
 * word: R on and above the diagonal of a diagonal tile is never read by the apply, and V (everything
 * below the diagonal) is never read by the solve — either may hold anything, inf and NaN included.
 * Workspace: the handle holds the T images of all members, batch * tqr_apply_workspace_bytes of the
 * shape, so one prepare serves any number of applies. There are no groups: tqr_batch_apply_bytes (host
 * only, no GPU; 0 on bad arguments) tells a caller beforehand when to split a batch through offset
 * pointers. create allocates it (TQR_ENOMEM if that fails); no other call allocates. tqr_batch_trsm_r
 * needs no handle and no workspace.
 * Ordering: a plan's, as tqr_tsqr_*. Concurrent host threads are mutually excluded while they
 * enqueue, and every call's stream first waits for the handle's previous call, whatever its stream (a
 * prepare rewrites the T images the applies read). Calls return once all is enqueued.
 * tqr_batch_trsm_r is ordered by its stream alone. Every kernel of these calls is ordered by its launch
 * alone — no flags, counters or waits between workgroups. More members than a grid's y dimension
 * (65535) run as consecutive launches with advanced base pointers.
 * Errors: TQR_EINVAL before any device call for tqr_apply_create's own argument errors, batch < 1, a
 * shape whose prepare grid (one workgroup per T image of a member) would pass 2^31 or whose workspace a
 * size_t, a NULL handle or pointer, a bad trans, nrhs < 1, ncols outside 1 .. m, a leading dimension
 * below the member's rows or beyond the library's bound, a stride of neither form, strideTau < m * kmax,
 * strideRes < nrhs, tqr_batch_lstsq with m < n. Without a gfx950, create still returns a handle with
 * no device memory, workspace_bytes answers, and every enqueueing call returns TQR_ENODEV after that
 * validation (tqr_batch_trsm_r too). With a device, any call on a handle other than prepare before its
 * first successful prepare returns TQR_EINVAL, before any device call.
 * Measured on an MI355X (tools/batch_apply_bench.py), TQR_NOTRANS least squares with
 * dres, against a loop of tqr_lstsq over per-member prepared tqr_apply handles in the same run, equal
 * bytes: 64 factorisations of 512 x 512, b = 64, fp64, 64 right-hand sides each: 0.81 against 47.3 ms;
 * 1024 of them: 2.75 against 851.7 ms; 1024 of 1024 x 1024, b = 128: 7.50 against 2138 ms; 256 of 4096 x
 * 256, b = 128, one right-hand side: 2.05 against 499.5 ms. tqr_batch_apply_prepare against the loop of
 * tqr_apply_prepare: 0.14 against 0.81, 1.48 against 14.4, 5.80 against 19.2 and 2.22 against 4.68 ms.
 * From 16 members on the batched calls were faster at all 40 points measured (lstsq 13.5 to 745 x,
 * prepare 1.24 to 19.4 x). For ONE factorisation tqr_lstsq on a tqr_apply handle is the faster call
 * (0.164 against 0.195 ms at 256 x 256, 1.64 against 1.65 ms at 4096 x 256): the batched handle adds an
 * event wait and record per call. TQR_TRANS, the apply and form-Q alone were not measured. */
typedef struct tqr_batch_apply tqr_batch_apply;
size_t tqr_batch_apply_bytes(int m, int n, int b, int dtype, int batch);
int tqr_batch_apply_create(tqr_batch_apply** ba, int m, int n, int b, int dtype, int batch);
size_t tqr_batch_apply_workspace_bytes(const tqr_batch_apply* ba);
int tqr_batch_apply_prepare(tqr_batch_apply* ba, const void* dA, int ldda, long long strideA, const void* dtau_compact,
                            long long strideTau, void* stream);
int tqr_batch_apply_q(tqr_batch_apply* ba, int trans, const void* dA, int ldda, long long strideA, void* dC, int nrhs,
                      int lddc, long long strideC, void* stream);
int tqr_batch_form_q(tqr_batch_apply* ba, const void* dA, int ldda, long long strideA, void* dQ, int ncols, int lddq,
                     long long strideQ, void* stream);
int tqr_batch_trsm_r(int dtype, int trans, int n, int b, int batch, const void* dA, int ldda, long long strideA, void* dX,
                     int nrhs, int lddx, long long strideX, void* stream);
int tqr_batch_lstsq(tqr_batch_apply* ba, int trans, const void* dA, int ldda, long long strideA, void* dB, int nrhs,
                    int lddb, long long strideB, void* dres, long long strideRes, void* stream);
void tqr_batch_apply_destroy(tqr_batch_apply* ba);

/* ---- tall-skinny: QR of an m x n matrix, m >> n, as a tree of batched factorisations (TSQR) -------
 * The flat tile tree of tqr_plan_execute is one GEQRT and m/b - 1 TSQRTs in series per panel: on a
 * tall-skinny matrix the device idles behind one CU. tqr_tsqr_factor cuts A into D_0 = m / m_dom row
 * domains, factorises them all in the launches of one (tqr_batch_execute on the row-interleaved
 * layout), stacks the domains' R factors `fan` at a time, factorises the stacks in the same way, and so
 * on up to one root.
 * Shape: m >= n; b in {16, 32, 64, 128, 256} divides m and n; m_dom is a multiple of b, >= n, and
 * divides m; fan >= 2; nrhs_max >= 0 is the widest C / B the handle's calls take (0: no C workspaces,
 * and every apply / form_q / lstsq returns TQR_EINVAL; form_q needs nrhs_max >= n); ws_limit goes to
 * every level's tqr_batch_create (0 = 1 GiB). Defaults: fan == 0 means 4; m_dom == 0 means the smallest
 * multiple of b that divides m and is >= max(4 n, 1024), or m (one domain) if there is none.
 * Levels: level 0's domains are the row blocks of A itself. Level l >= 1 has D_l = ceil(D_{l-1} / fan)
 * domains of fan * n rows: the row blocks of the handle's workspace W_l, a (D_l * fan * n) x n
 * column-major matrix of the handle's dtype with leading dimension D_l * fan * n. Block j of W_l (rows
 * j n .. j n + n - 1) is the upper triangle (i <= j) of the top n x n of domain j of level l-1 with zeros
 * below the diagonal; blocks beyond D_{l-1} (padding) are zero. All of W_l is rewritten by every factor.
 * The last level has one domain; D_0 == 1 gives one level and no merge. Level l's compact taus are D_l
 * blocks of (domain rows) x (n / b) elements, domain i at element i * (domain rows) * (n / b).
 * tqr_tsqr_level returns a level's W_l (level 0: NULL, the matrix is the caller's), its leading
 * dimension (level 0: 0), its taus, the domain height and D_l; outputs may be NULL. So domain i of
 * level l is the member (dW + i * dom_rows, ldw, dtau + i * dom_rows * (n / b)) of shape (dom_rows, n,
 * b), and by the bit contract every per-member handle of this library works on it through these offset
 * pointers.
 * On exit of tqr_tsqr_factor the upper triangle of dA[0:n, 0:n] is R of the whole matrix (only elements
 * i <= j are written there; the V below the diagonal stays), so tqr_trsm_r works on dA unchanged. The
 * rest of dA holds level 0's V and, in the other domains' top triangles, their R_i, which nothing reads.
 * The Q this defines: a domain's top n rows travel up and a stack's leader is its first block, so the
 * root's top rows trace back to rows 0 .. n-1 of A — a genuine m x m orthogonal Q with Q^T A = [R; 0]
 * in natural row order. tqr_tsqr_apply_q: dC (m x nrhs, lddc >= m) <- Q^T dC (TQR_TRANS) or Q dC
 * (TQR_NOTRANS) in place, with tqr_apply_q's semantics: rows >= m and columns >= nrhs are not touched;
 * after Q^T rows 0 .. n-1 hold the "R part". Q^T applies level 0 on C's domains, gathers their top n rows
 * into the handle's C_1 (zero padding), applies level 1 there, and so on to the root, then scatters
 * back down; Q is the exact reverse. tqr_tsqr_form_q: the thin Q (m x n) into dQ, output-only: [I_n; 0]
 * is filled, then Q applied (the work on its zero blocks is done). tqr_tsqr_lstsq: tqr_lstsq's semantics,
 * dres and zeroed rows of TQR_TRANS exactly — TQR_NOTRANS: Q^T, tqr_trsm_r on rows 0 .. n-1, the residual
 * norms of rows n .. m-1; TQR_TRANS: rows n .. zeroed, tqr_trsm_r(TQR_TRANS), Q.
 * Bit contract: after tqr_tsqr_factor every domain of every level has the bytes of tqr_batch_execute on
 * that layout, i.e. of a TQR_ENGINE_WAVES plan on the member alone — except the upper triangle of
 * dA[0:n, 0:n], which holds the final R. tqr_tsqr_apply_q on a domain computes the bytes of tqr_apply_q
 * on that member (the same kernel bodies behind a per-domain pointer offset: the kernels are the ones
 * tqr_batch_apply_prepare / tqr_batch_apply_q launch, shared between the two). Nothing outside the
 * matrices is written: rows >= m, columns >= n or nrhs, the padding of ldda / lddc.
 * Zero padding is harmless by the tile kernels' conventions: a TSQRT on [R_kk; 0] gives V_B = 0 and
 * tau = 2 (no scaling when |x| == 0), and zero rows of a right-hand side stay zero.
 * Workspace: tqr_tsqr_workspace_bytes = the levels' taus, the W_l, per level and domain one tqr_apply T
 * workspace (rebuilt by every factor, so the applies need no prepare), the C_l ((D_l * fan * n) x
 * nrhs_max), each rounded up to 256 bytes, plus the levels' tqr_batch_workspace_bytes. create allocates
 * it; no call allocates.
 * Ordering: a plan's. Concurrent host threads are mutually excluded while they enqueue, and every
 * call's stream first waits for the handle's previous call, whatever its stream (factor rewrites the T
 * and W workspaces the applies read, the applies share the C_l). Calls return once all is enqueued.
 * Every kernel of these calls is ordered by its launch alone — no flags, counters or waits between
 * workgroups. More domains than a grid's y dimension (65535) run as consecutive launches.
 * Errors: TQR_EINVAL before any device call for tqr_plan_create's own argument errors, m < n, a bad
 * m_dom or fan, nrhs_max < 0, a shape whose grids or workspace dimensions would pass 2^31 or the
 * leading-dimension bound, NULL pointers, a bad trans, nrhs < 1 or > nrhs_max, ldda / lddc / lddq / lddb
 * below m or beyond the leading-dimension bound. Without a gfx950, create still returns a handle with no
 * device memory; workspace_bytes and level's integer outputs answer (its pointers are NULL), and every
 * enqueueing call returns TQR_ENODEV after that validation. With a device, any call other than factor
 * before the first successful factor returns TQR_EINVAL, before any device call.
 * Measured on an MI355X (tools/tsqr_bench.py), fp64, defaults, against tqr_plan_execute on
 * a flow plan of the same matrix at its fastest b, and torch.geqrf, in the same run: 65536 x 256: 8.98 ms
 * against 13.51 and 75.4 ms; 262144 x 128: 6.05 against 66.1 and 61.3 ms; 1048576 x 64: 8.42 against 521.1
 * and 140.4 ms. tqr_tsqr_apply_q(TQR_TRANS) on 64 columns: 2.43, 1.08 and 1.42 ms against tqr_apply_pipe_q's
 * 31.4, 120.1 and 423.5 ms on the flow factorisation; tqr_tsqr_lstsq: 2.57, 1.44 and 3.08 against
 * tqr_lstsq_pipe's 31.6, 120.4 and 425.6 ms. The defaults are the fastest point of the sweep of m_dom x fan
 * at all three shapes. No shape was measured at which the flow plan is the faster call; shorter matrices
 * (below 65536 rows) and n > 256 were not measured.
 * tqr_tsqr_plan (host only, no GPU): the resolved m_dom and fan, the level count, domains[l] = D_l (at
 * most `cap` written) and tqr_tsqr_workspace_bytes of such a handle. Outputs may be NULL; arguments out
 * of range return TQR_EINVAL and write nothing. */
typedef struct tqr_tsqr tqr_tsqr;
typedef struct tqr_tsqr_spec {
    int m, n, b, dtype, m_dom, fan, nrhs_max;
    size_t ws_limit;
} tqr_tsqr_spec;
int tqr_tsqr_plan(const tqr_tsqr_spec* spec, int* m_dom, int* fan, int* nlevels, int* domains, int cap, size_t* ws_bytes);
int tqr_tsqr_create(tqr_tsqr** ts, const tqr_tsqr_spec* spec);
size_t tqr_tsqr_workspace_bytes(const tqr_tsqr* ts);
int tqr_tsqr_factor(tqr_tsqr* ts, void* dA, int ldda, void* stream);
int tqr_tsqr_apply_q(tqr_tsqr* ts, int trans, const void* dA, int ldda, void* dC, int nrhs, int lddc, void* stream);
int tqr_tsqr_form_q(tqr_tsqr* ts, const void* dA, int ldda, void* dQ, int lddq, void* stream); /* thin Q, m x n */
int tqr_tsqr_lstsq(tqr_tsqr* ts, int trans, const void* dA, int ldda, void* dB, int nrhs, int lddb, void* dres,
                   void* stream);
int tqr_tsqr_level(const tqr_tsqr* ts, int level, void** dW, int* ldw, void** dtau, int* dom_rows, int* ndom);
void tqr_tsqr_destroy(tqr_tsqr* ts);

/* ---- row update: append rows to a finished QR (qrinsert for rows, recursive least squares) ------
 * R is the upper triangle of the leading n x n block of a device matrix dR (lddr >= n), as any engine
 * of this library left it; W (dW, mw x n, lddw >= mw) holds mw new rows. b in {16, 32, 64, 128, 256}
 * divides n and mw (a caller with fewer rows pads W with zero rows); q = n/b, wt = mw/b.
 * tqr_update_rows replaces R by the R' of the stacked [R; W]:
 *   for k in 0..q-1: for l in 0..wt-1:
 *     TSQRT(R_kk, W_lk) -> R_kk's triangle, V in W_lk, b taus
 *     for j in k+1..q-1: TSMQR(V = W_lk; R_kj, W_lj)
 * the flat-tree update restricted to the tiles that exist. On exit R'^T R' = R^T R + W^T W, W holds the
 * dense TSQRT V tiles, and dtau_u (mw x q column-major, leading dimension mw, of the handle's dtype)
 * holds at (l*b + c, k) the tau of column c of TSQRT(., W_lk). With the Householder convention above
 * diag(R') has the sign of diag(R) times (-1)^wt.
 * Of dR only elements (i, j), i <= j < n, are read or written: the strictly lower part of every
 * diagonal tile keeps its bytes (the old GEQRT V, NaN and inf included, never enters a product), and
 * the tiles below the block diagonal are never touched — the rule of tqr_trsm_r. Rows >= mw of dW's
 * allocation and columns >= n are not touched.
 * After an update the old V of dR no longer belongs to R': the Q of the updated factorisation of
 * [A; W] is diag(Q_old, I) * Q_u, where Q_old is the Q of the factorisation that left R (its V and
 * taus are unchanged and its tqr_apply_* reads nothing else of dR, so that handle still applies
 * Q_old from dR, prepared before or after the update) and Q_u, (n+mw) x (n+mw), is this
 * update's, applied by tqr_update_apply_q to a pair (Ctop: n x nrhs, Cnew: mw x nrhs):
 *   TQR_TRANS:   for k ascending, l ascending: [Ctop_k; Cnew_l] <- TSMQR(V = W_lk) [Ctop_k; Cnew_l];
 *   TQR_NOTRANS: the exact reverse, each block reflector untransposed, so Q_u (Q_u^T C) = C.
 * Q^T [c; c_new] of the whole is Q_old^T on c, then Q_u^T on the pair; Q is the reverse order.
 * Bit contract (the separation identity): in the flat-tree factorisation of the stacked S = [G; W], G
 * n x n, the tile operations on the W rows never feed those on the G rows, and at step k they see G's
 * own final R_kk and R_kj. So a TQR_ENGINE_WAVES plan on S equals a wave plan on G followed by
 * tqr_update_rows with W, bit for bit: the upper triangle, rows >= n (W's V) and rows >= n of the
 * compact tau (= dtau_u). Likewise tqr_apply_q of the stacked factorisation equals G's tqr_apply_q
 * then tqr_update_apply_q (TQR_TRANS; reversed for TQR_NOTRANS), both with T from prepare passes.
 * fp32 handles load and store float and compute in fp64, as the wave engine.
 * Method: level-synchronous, as the wave engine. TSQRT(l,k) sits on level 2k + l, TSMQR(l,j,k) on
 * level 2k + l + 1; every dependency lies on an earlier level and the items of one level touch
 * disjoint data. Each level is at most two launches (the TSQRTs, one workgroup each; the 64-column
 * strips of the TSMQRs) on two side streams of the handle joined by events to the caller's stream.
 * No kernel waits for another workgroup: no flags, no counters, nothing that can hang. The critical
 * path is 2q + wt - 2 levels, each at least one TSQRT long: the update pays when wt is small against
 * q. For mw >> n it is a serial chain of wt TSQRTs per step — factorise such a block first
 * (tqr_tsqr_* or a plan) and append its R.
 * Measured on an MI355X (tools/update_bench.py), n = 16384, b = 256, against a flow plan
 * on the stacked (n + mw) x n matrix from scratch and a wave plan on the dense [R; W], in the same run:
 * fp64, mw = 256: 48.2 ms against 118.6 and 226.2 ms; mw = 1024: 83.6 against 125.6 and 235.1 ms; mw =
 * 4096: 115.5 against 153.9 and 291.5 ms. The update LOSES in fp32 (mw = 1024: 91.1 ms against the flow
 * plan's 70.5 ms, whose fp32 chains run on the fp32 MFMA; 249.1 ms for the dense wave plan).
 * tqr_update_apply_q on 64 columns: 9.7 / 41.7 / 201.5 ms (one workgroup walks q * wt TSMQRs);
 * tqr_update_lstsq with 64 right-hand sides: 182.4 / 250.1 / 441.7 ms, of which tqr_trsm_r on one
 * workgroup is 124 ms. mw > n/4, other n and b were not measured.
 * tqr_update_rows ends with the T pass of tqr_update_prepare, so the handle is ready for applies.
 * tqr_update_prepare rebuilds the apply's T images from stored W and dtau_u alone (how one
 * re-attaches a handle to an update kept from earlier); tqr_update_apply_q before any prepare or rows
 * returns TQR_EINVAL. nrhs >= 1 need not be a multiple of anything; rows and columns outside the two
 * blocks are untouched. One workgroup per 64 columns walks the q * wt TSMQRs serially.
 * tqr_update_lstsq: one step of recursive least squares. dD (n x nrhs, lddd >= n, in/out) holds the
 * top n rows of Q^T b so far; dBnew (mw x nrhs, lddb >= mw) the new right-hand-side rows on entry,
 * their transformed rows on exit. In order: tqr_update_rows; tqr_update_apply_q(TQR_TRANS) on (dD,
 * dBnew); a copy of dD to dX (n x nrhs, lddx >= n; dX must not overlap dD); tqr_trsm_r(TQR_NOTRANS)
 * on dX with R' — dX is the solution over all rows so far. dres: NULL, or nrhs running residual norms
 * of the handle's dtype, dres[j] <- sqrt(dres[j]^2 + |Bnew'[:, j]|^2), the sum accumulated in fp64 in
 * a fixed order and unscaled, as tqr_lstsq's norm (start it from tqr_lstsq's dres, or zeros).
 * Workspace: two sets of T images (the factorisation's and the apply's), one 32 x 33 fp64 image (b <
 * 32: b x (b+1)) padded to whole KiB per 32-reflector group of each of the q * wt W tiles —
 * tqr_update_workspace_bytes, allocated by create; nothing is allocated afterwards.
 * Ordering: as a plan's. Calls of one handle are mutually excluded while they enqueue; each call's
 * stream first waits for the handle's previous rows / prepare, and a rows / prepare for every apply
 * enqueued since; applies may overlap each other. Everything is stream-ordered.
 * Errors: TQR_EINVAL before any device call for a bad dtype, a bad b or one that does not divide n
 * and mw, n <= 0 or mw <= 0, a NULL handle or pointer, a bad trans, nrhs < 1, lddr < n, lddw, lddcn or
 * lddb below mw, lddct, lddd or lddx below n, and any leading dimension (n and mw included) beyond
 * the library's bound. A missing or non-gfx950 device is reported after that validation:
 * tqr_update_create then still returns a handle (without device memory; workspace_bytes answers), and
 * rows, prepare and lstsq on it return TQR_ENODEV.
 * tqr_update_plan, tqr_update_level_items (host only, no GPU): the schedule the host side issues.
 * *nlevels = 2q + wt - 2, *npanel = q * wt TSQRT items, *nupdate = ceil(b/64) * wt * q(q-1)/2 TSMQR
 * strip items, *nlaunch = the non-empty TSQRT launches plus the non-empty TSMQR launches of all levels
 * plus 1 (the closing T pass). Outputs may be NULL. tqr_update_level_items writes the items of one
 * level, 4 ints each {type | strip << 8, l, j, k} (type 2 = TSQRT with j = k, type 3 = TSMQR; the
 * TSQRT items first), at most `cap` of them, and returns the level's item count. Arguments out of
 * range return TQR_EINVAL and write nothing. */
typedef struct tqr_update tqr_update;
int tqr_update_create(tqr_update** up, int n, int mw, int b, int dtype);
size_t tqr_update_workspace_bytes(const tqr_update* up);
int tqr_update_rows(tqr_update* up, void* dR, int lddr, void* dW, int lddw, void* dtau_u, void* stream);
int tqr_update_prepare(tqr_update* up, const void* dW, int lddw, const void* dtau_u, void* stream);
int tqr_update_apply_q(tqr_update* up, int trans, const void* dW, int lddw, void* dCtop, int lddct, void* dCnew,
                       int lddcn, int nrhs, void* stream);
int tqr_update_lstsq(tqr_update* up, void* dR, int lddr, void* dW, int lddw, void* dtau_u, void* dD, int lddd,
                     void* dBnew, int lddb, int nrhs, void* dX, int lddx, void* dres, void* stream);
void tqr_update_destroy(tqr_update* up);
int tqr_update_plan(int n, int mw, int b, int* nlevels, int* npanel, int* nupdate, int* nlaunch);
int tqr_update_level_items(int n, int mw, int b, int level, int* items, int cap);

/* ---- multi-GPU: tile-column partition, one process per GPU ---------------------------------
 * Rank r owns the tile columns j with tqr_dist_owner(j) == r — snake order over the ranks
 * (0..W-1, W-1..0, 0..W-1, ...: every rank's columns sum to the same index total, balancing the
 * chain work that grows with j); the owner of column j factors it entirely (its panel when j <
 * kmax, and all its updates).
 * Storage (round 4): a rank holds ONLY its own tile columns, packed in column order — global tile
 * column j is local tile column j / W of the rank's dA (b * tqr_dist_local_cols(plan) columns,
 * leading dimension ldda >= m), and the taus of panel k are column k / W of its compact tau (m x
 * tqr_dist_local_cols(plan)). A 65536 x 16384 fp64 matrix on 8 ranks is 1 GiB per rank.
 * The owner of panel k forwards each finished reflector group's V/T images to every peer over
 * xGMI inside the persistent launch (peer workspaces opened by IPC), so panels of successive
 * steps overlap across GPUs exactly as on one GPU. Every rank calls tqr_plan_execute the same
 * number of times; consecutive executes need no host synchronisation or barrier between the
 * ranks (the cross-rank flags carry launch epochs, and a rank forwards into a peer only once that
 * peer's previous launch has finished, all on the device).
 * Chain tasks are shorter on 4+ ranks that each launch over a whole device (2 elements instead of
 * 8; TQR_SEGLEN overrides): more parallel slack per rank. Every rank must build the
 * same global task list — tqr_dist_import compares the ranks' list signatures (segment lengths,
 * lookahead tail, tail segments, list length and a hash of the whole list in order, so every
 * ordering knob is covered) and fails with TQR_EINVAL if they differ.
 * Setup once: tqr_dist_export -> exchange all ranks' handle blocks (e.g. an all-gather over
 * torch.distributed / MPI) -> tqr_dist_import(plan, blocks of rank 0..world-1). */
int tqr_dist_plan_create(tqr_plan** plan, int m, int n, int b, int dtype, int rank, int world);
/* bytes of one rank's handle block (its device's PCI bus id, its task-list signature, the IPC
 * handles of its panel counters and per-step panel workspaces — one allocation per step keeps
 * every export under 2 GiB) */
size_t tqr_dist_handle_bytes(const tqr_plan* plan);
int tqr_dist_export(tqr_plan* plan, void* handles, size_t len);
int tqr_dist_import(tqr_plan* plan, const void* all_handles, size_t len);
/* Peer-path probe, once after tqr_dist_import (fails fast instead of a wait timeout or a hang in the
 * first factorisation): phase 0 stores this rank's token into every peer's probe word (system-scope
 * stores through the IPC-mapped peer flags, the path panel flags take); then a host barrier over all
 * ranks; phase 1 loads this rank's probe words (system-scope loads, the path the chains poll) and
 * returns TQR_OK if every peer's token arrived, else TQR_EHIP with each missing rank printed.
 * *seen (may be NULL; phase 1) receives the bit mask of the peers whose token arrived. */
int tqr_dist_probe(tqr_plan* plan, int phase, unsigned long long* seen);
/* no-op since round 4 (executes reset their own counters); kept for source compatibility */
int tqr_dist_reset(tqr_plan* plan, void* stream);
int tqr_dist_owner(const tqr_plan* plan, int tile_col);
/* number of tile columns this rank stores (and of its compact tau columns) */
int tqr_dist_local_cols(const tqr_plan* plan);
/* bytes this rank forwards to its peers per factorisation (every owned panel member's V/T images,
 * all reflector groups, to each of the world - 1 peers); 0 for a single-GPU plan */
long long tqr_plan_fwd_bytes(const tqr_plan* plan);
/* host-only: this rank's task-list length and the number of its panel members that forward
 * their V/T images to the peers (its panel tasks when world > 1, else 0); the list is the one a
 * plan of `world` ranks with a whole device each builds (the multi-rank task-list defaults of
 * tqr_dist_plan_create apply; the segment length is `seglen`) */
int tqr_dist_plan_check(int M, int N, int b, int seglen, int rank, int world, int* ntasks, int* nfwd);

/* ---- one-shot helpers ------------------------------------------------------------------ */
/* Device pointers, stream-ordered; plan cached per (device,m,n,b,dtype) and shared by all
 * callers — concurrent calls with the same shape are serialised on the GPU (see execute). The
 * result has the bits of tqr_plan_execute on a plan of one's own. The cached plan's engine is
 * TQR_ENGINE_DEFAULT's at the time the plan is created (the first call for a shape, or the first
 * after tqr_cache_clear). Argument errors (sizes, tile size, NULL pointers, ldda < m or beyond the
 * leading-dimension bound) return TQR_EINVAL before the cache or a device is touched. */
int tqr_dgeqrt_tiled(int m, int n, int b, double* dA, int ldda, double* dtau_compact, void* stream);
int tqr_sgeqrt_tiled(int m, int n, int b, float* dA, int ldda, float* dtau_compact, void* stream);

/* Host pointers, blocking: A in place; tau = the reference's m x n tau matrix (ldm), or NULL
 * (the reference's cudaQRTask discards tau). Any ldm >= m.
 * With the default (flow) engine the persistent launch moves the matrix itself, overlapping PCIe
 * with the factorisation: it reads each tile column from host memory just before step 0 needs it
 * and writes each tile column back as soon as it is final. Host memory is either a pinned staging
 * buffer that host threads fill and drain while the kernel runs (default), or — environment
 * TQR_HOST_XFER=register — the caller's array itself, page-locked for the call.
 * Retention: the plan of each (device, m, n, b, dtype) keeps an m x n device matrix and an
 * m x kmax tau array, and each device keeps one pinned staging buffer of the largest matrix seen,
 * until tqr_cache_clear(). Calls on one shape are serialised. */
int tqr_dgeqrt_host(double* A, double* tau, int m, int n, int ldm, int b);
int tqr_sgeqrt_host(float* A, float* tau, int m, int n, int ldm, int b);
/* the same with an explicit engine (tqr_engine) and dtype */
int tqr_geqrt_host_engine(int dtype, void* A, void* tau, int m, int n, int ldm, int b, int engine);
/* Release every cached plan of the one-shot helpers (device buffers, pinned buffers) and the
 * host-API staging buffers; synchronises the device first. Plans created by the caller are not
 * affected. */
int tqr_cache_clear(void);
/* Host-only check of the host-API task list (the flow list plus nxc upload / download tasks per
 * tile column, a column's upload estimated at tcol chain elements): number of tasks and whether
 * the estimated-start-time order is topological. */
int tqr_flow_xfer_plan_check(int M, int N, int b, int seglen, int nxc, double tcol, int* ntasks, int* est_order);

/* Host pointers, single tile tasks on the GPU (the reference's per-tile kernels; used by
 * qrdecomp.h's SGEQRF/SLARFT/STSQRF/SSSRFT and by the per-tile parity tests). Tile pointers
 * are tile origins inside one ldm-strided matrix; tau pointers point at the tile's b
 * consecutive taus, as in the reference. */
int tqr_tile_geqrt(int dtype, void* blk, void* tau, int b, int ldm);
int tqr_tile_unmqr(int dtype, void* C, const void* V, const void* tau, int b, int ldm);
int tqr_tile_tsqrt(int dtype, void* A, void* B, void* tau, int b, int ldm);
int tqr_tile_tsmqr(int dtype, const void* V, void* A, void* B, const void* tau, int b, int ldm);

/* Batched independent tile updates in ONE launch of the update kernel (the reference's testDAPP
 * microbenchmark, src/gpucalc.cu:1687-1774, generalised to UNMQR and any b): `nblocks` copies of
 * the host block `blk` are each updated with the same reflectors.
 *   type DAPP (TSMQR): V = b x b dense TSQRT V_B (ldv), tau = its b taus, blk = 2b x b [A; B] (ldb);
 *   type SAPP (UNMQR): V = b x b GEQRT tile (unit-lower V below the diagonal), blk = b x b C.
 * *ms = device time of the update launch (HIP events); out (optional) receives the nblocks
 * results, block j at out + j*b*ldo. The batch is one 2b-row device matrix of (1 + nblocks) b
 * columns addressed with 32-bit offsets: more than 2^31 - 1 bytes returns TQR_EINVAL. */
int tqr_tile_batch(int dtype, int type, int b, int nblocks, const void* V, int ldv, const void* tau,
                   const void* blk, int ldb, void* out, int ldo, float* ms);

/* Device-side synthetic input with the reference's RANDZO distribution
 * ((r mod 201) - 100)/100 (qrdecomp.c:1383), from a counter-based hash of (seed, i, j). */
int tqr_fill_randzo(int dtype, void* dA, int m, int n, int ldda, unsigned long long seed, void* stream);
/* columns col0 .. col0 + ncols - 1 of that matrix only (a multi-GPU rank's own tile columns) */
int tqr_fill_randzo_cols(int dtype, void* dA, int m, int ncols, int ldda, unsigned long long seed, long col0, void* stream);

#ifdef __cplusplus
}
#endif
#endif
