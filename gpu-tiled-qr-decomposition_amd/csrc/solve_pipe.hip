// The triangular solve with R spread over workgroups (include/tqr.h "pipelined solve"): the same
// operations as solve.hip's k_trsm_r, in the same order, hence the same bits — but one workgroup per
// (64-column strip, tile row) instead of one per strip, so a narrow X uses T = n / b CUs, not one.
//
// k_trsm_r is right-looking: once X_k is solved it subtracts R_ik X_k from every tile row i still to
// be solved. Tile row i therefore receives X_i -= R_ik X_k for k = T-1 .. i+1 in that order (TRANS:
// R_ki^T X_k, k = 0 .. i-1) and is then solved against tile (i,i); nothing else touches its rows.
// k_trsm_r_pipe is the left-looking form of exactly that: the workgroup of (strip, i) waits for X_k,
// runs the per-group stage_r / accum_z update of its own rows, and after the last k the diag / step
// sequence of k_trsm_r — the helpers of solve_dev.hpp, unchanged. Its rows pass through memory
// between two updates as they do there (fp32 storage: rounded to float after every tile's update).
//
// Protocol between workgroups (MI355X_MICROARCH.md "Workgroup dispatch ... inter-workgroup
// visibility", "Valid forms", first table row; the engine's form, flow.hpp):
//   * work items come from one atomic ticket counter, never from blockIdx: ticket t is (strip, row)
//     by solve_ticket_map, and every producer of a row has a smaller ticket. A workgroup that waits
//     holds a ticket, so everything it waits for was taken by a workgroup already running: the
//     smallest unfinished ticket never waits on an unfinished one, whatever the dispatch order and
//     however few workgroups are resident;
//   * every load and store of X in this kernel is an sc1 buffer access (L1-bypassing / write-through).
//     After its last store each wave drains (s_waitcnt vmcnt(0)), the workgroup meets at a barrier,
//     and one lane stores the row's flag (sc1). A consumer's thread 0 polls that flag with sc1 loads
//     and s_sleep; the other waves load X_k only behind the barrier thread 0 then joins;
//   * the table row holds at one workgroup per CU: the launch asks for PIPE_LDS bytes of LDS (more
//     than half a CU's 160 KiB), so two of these workgroups never share a CU;
//   * flags hold the epoch of the call that set them (a call waits for its own epoch: nothing is
//     reset between calls); the ticket counter is zeroed by a memset node ahead of each launch, and
//     the calls of one handle are serialised by an event, as tqr_plan_execute's are;
//   * every spin is bounded (PIPE_TIMEOUT): on expiry the error word is set, the workgroup leaves
//     without publishing, and every workgroup that sees the word — in a spin or before it takes a
//     ticket — leaves too. tqr_solve_status reports it.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

#include "pipe_dev.hpp"
#include "solve.hpp"
#include "solve_dev.hpp"
#include "tqr.h"

namespace tqr {

// Work item of ticket t on T tile rows x nstrips strips: tickets go row by row in the order the
// solve needs them (NOTRANS: T-1 first; TRANS: 0 first), all strips of a row side by side — so the
// producers of (strip, row), the rows solved before it in the same strip, have smaller tickets.
__host__ __device__ inline void solve_ticket_map(int T, int nstrips, bool trans, int t, int* strip, int* row) {
  const int pos = t / nstrips;
  *strip = t - pos * nstrips;
  *row = trans ? pos : T - 1 - pos;
}

struct PipeArgs {
  const void* A;  // factorised matrix (S*): R in the upper triangle of the leading n x n block
  void* X;        // n x nrhs (S*)
  long lda, ldx;
  int nt, nrhs;  // nt = n / b tile rows
  int epoch;     // this call's flag value
  int* ws;       // the handle's workspace (one pointer: the kernels are short of SGPRs at b = 256)
};

// workspace (pipe_dev.hpp): the header, then the flags [strip][row] = the epoch of the call whose X_row
// of the strip is final

// ---------------------------------------------------------------------------------------
// One workgroup per ticket = (strip, tile row i): wave w owns columns 64 strip + 16w .. + 15 of X.
// A wave with no column below nrhs does no arithmetic but takes part in the staging and in every
// barrier (as in k_trsm_r).
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT) void k_trsm_r_pipe(PipeArgs a) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG, NRI = G::NRI, NKS = G::NKS;
  constexpr int SC1 = 16;  // aux bits of every X access
  extern __shared__ __align__(16) double lds[];
  double* Vs = lds;
  __shared__ int s_tk, s_ok;

  if (threadIdx.x == 0)
    s_tk = ld_sc1(a.ws + PIPE_ERR) ? -1 : __hip_atomic_fetch_add((pint*)(a.ws + PIPE_TICKET), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const int tk = __builtin_amdgcn_readfirstlane(s_tk), nstrips = (a.nrhs + 63) >> 6;
  if (tk < 0 || tk >= a.nt * nstrips) return;  // (an earlier call of the handle timed out: tqr_solve_status)
  int strip, i;
  solve_ticket_map(a.nt, nstrips, TRANS, tk, &strip, &i);

  const S* A = (const S*)a.A;
  const size_t lda = a.lda, ldx = a.ldx;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = strip * 64 + 16 * w, col = col0 + (lane & 15);
  const bool active = col0 < a.nrhs;  // wave-uniform
  // The kernel is short of SGPRs at b = 256 (stage_r's chunk resources and offsets), so what only
  // the rare paths read sits in VGPRs, which are plentiful at one workgroup per CU: the lane's
  // column mask as an integer instead of a mask pair, and the poll's pointer and epoch.
  int on = col < a.nrhs;
  unsigned long long wsv = (unsigned long long)a.ws;
  int epoch = a.epoch;
  asm volatile("" : "+v"(on), "+v"(wsv), "+v"(epoch));
  int* const ws = (int*)wsv;
  S* Xw = (S*)a.X + (size_t)(active ? col0 : 0) * ldx;
  const unsigned coff = head_off<B, S>(ldx, 0);
  const int fl = PIPE_HDR + strip * a.nt;  // the strip's flags in the workspace
  // one resource over the wave's 16 columns; a tile row is a byte offset in it (below 2^31 by the
  // leading-dimension bound), ioff the workgroup's own
  const __amdgpu_buffer_rsrc_t rx = uniform_rsrc(Xw);
  const unsigned ioff = coff + (unsigned)i * (unsigned)(B * sizeof(S));
  double X[NKS];

  // a whole tile row of the strip into X (a lane whose column is >= nrhs: zeros)
  auto load_rows = [&](unsigned off) {
    if (on) {
      load_strip_buf<B, S, SC1>(X, rx, off, 0);
    } else {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) X[ks] = 0.0;
    }
  };
  // all threads: X_k of this strip is final (false: error or timeout, uniform)
  auto wait = [&](int k) {
    if (threadIdx.x == 0) s_ok = pipe_spin_ge(ws + fl + k, epoch, ws + PIPE_ERR) ? 1 : 0;
    __syncthreads();
    // (thread 0 rewrites s_ok only behind the next barrier, which every thread reaches after this read)
    return s_ok != 0;
  };
  // X_i -= (tile Rt of op(R)) X_k, X_k in X: k_trsm_r's update(), group by group — the 32 target rows
  // loaded ahead of the staging, updated by one pass of accum_z over the whole strip, stored
  auto update = [&](const S* Rt) {
    for (int g = 0; g < NG; ++g) {
      double H[NRI];
      const unsigned hoff = ioff + (unsigned)(g * IB * (int)sizeof(S));
      if (active) {
        if (on) {
          load_head_buf<B, S, SC1>(H, rx, hoff);
        } else {
#pragma unroll
          for (int r = 0; r < NRI; ++r) H[r] = 0.0;
        }
      }
      __syncthreads();
      stage_r<B, S, !TRANS, false>(Vs, Rt, lda, g, 0, NG);
      __syncthreads();
      if (active) {
        accum_z<B>(Vs, X, H, 0, NKS);
        if (on) store_head_buf<B, S, SC1>(H, rx, hoff);
      }
    }
  };
  // tile (i,i) against X_i in X: k_trsm_r's diag()
  auto diag = [&]() {
    const S* Rt = A + (size_t)i * B * lda + (size_t)i * B;
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_r<B, S, !TRANS, true>(Vs, Rt, lda, g, TRANS ? 0 : g, TRANS ? g + 1 : NG);
      __syncthreads();
      if (active) {
        double Z[NRI];
#pragma unroll
        for (int r = 0; r < NRI; ++r) Z[r] = X[r];
#pragma unroll
        for (int gg = 1; gg < NG; ++gg)
#pragma unroll
          for (int r = 0; r < NRI; ++r) Z[r] = gg == g ? X[gg * NRI + r] : Z[r];
        accum_z<B>(Vs, X, Z, TRANS ? 0 : (g + 1) * NRI, TRANS ? g * NRI : NKS);
        subst<B, TRANS>(Vs + g * IB * G::VP, Z);
#pragma unroll
        for (int gg = 0; gg < NG; ++gg)
#pragma unroll
          for (int r = 0; r < NRI; ++r) X[gg * NRI + r] = gg == g ? Z[r] : X[gg * NRI + r];
      }
    }
  };

  // the producers in k_trsm_r's order. No byte of X_k's rows is read before X_k's flag is set: the
  // only loads of rows other than the workgroup's own are the load_rows below, behind wait(k).
  for (int kk = 0; kk < (TRANS ? i : a.nt - 1 - i); ++kk) {
    const int k = TRANS ? kk : a.nt - 1 - kk;
    if (!wait(k)) return;
    if (active) load_rows(coff + (unsigned)k * (unsigned)(B * sizeof(S)));
    update(TRANS ? A + (size_t)i * B * lda + (size_t)k * B    // R_ki
                 : A + (size_t)k * B * lda + (size_t)i * B);  // R_ik
  }
  // k_trsm_r's step(i); the rows were last stored by the lanes that load them now
  if (active) load_rows(ioff);
  diag();
  if (active) {
    // fp32 storage: the consumers use X_i as it is stored
    if constexpr (sizeof(S) == 4) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) X[ks] = (double)(float)X[ks];
    }
    if (on) store_strip_buf<B, S, SC1>(X, rx, ioff, 0);
  }
  // publish X_i: every wave's stores drained, a barrier, one lane's flag store
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store((pint*)(ws + fl + i), epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

typedef void (*pfn)(PipeArgs);
template <int B>
static pfn pipe_kernel(int dtype, int trans) {
  if (dtype == TQR_F64) return trans == TQR_TRANS ? k_trsm_r_pipe<B, double, true> : k_trsm_r_pipe<B, double, false>;
  return trans == TQR_TRANS ? k_trsm_r_pipe<B, float, true> : k_trsm_r_pipe<B, float, false>;
}
static pfn pipe_kernel_b(int b, int dtype, int trans) {
  switch (b) {
    case 16: return pipe_kernel<16>(dtype, trans);
    case 32: return pipe_kernel<32>(dtype, trans);
    case 64: return pipe_kernel<64>(dtype, trans);
    case 128: return pipe_kernel<128>(dtype, trans);
    default: return pipe_kernel<256>(dtype, trans);
  }
}

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "tqr: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return TQR_EHIP;                                                                    \
    }                                                                                     \
  } while (0)

}  // namespace tqr

using namespace tqr;

struct tqr_solve {
  int n, b, dtype, nrhs_max, nt, nstrips_max;
  size_t es, ws_bytes;
  pfn kn = nullptr, kt = nullptr;
  std::mutex mu;       // the enqueue sequence of a call (epoch, event bookkeeping)
  int* d_ws = nullptr; // device workspace (null until a gfx950 was seen)
  hipEvent_t evDone = nullptr;
  int epoch = 0;
};

// The handle's device side, made on first need (tqr_solve_create where a device is present): the
// zeroed workspace, the event and the kernels' LDS attribute. mu held, or the handle not yet shared.
static int solve_pipe_ready(tqr_solve* sv) {
  if (sv->d_ws) return TQR_OK;
  int dev = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) {
    (void)hipGetLastError();
    return TQR_ENODEV;
  }
  if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "tqr: device %d is %s, this build targets gfx950 only\n", dev, pr.gcnArchName);
    return TQR_ENODEV;
  }
  HIPCHK(hipFuncSetAttribute((const void*)sv->kn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS));
  HIPCHK(hipFuncSetAttribute((const void*)sv->kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS));
  if (!sv->evDone) HIPCHK(hipEventCreateWithFlags(&sv->evDone, hipEventDisableTiming));
  int* ws = nullptr;
  if (hipMalloc(&ws, sv->ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return TQR_ENOMEM;
  }
  if (hipMemset(ws, 0, sv->ws_bytes) != hipSuccess) {
    (void)hipFree(ws);
    return TQR_EHIP;
  }
  sv->d_ws = ws;
  return TQR_OK;
}

namespace tqr {
SolveShape solve_shape(const tqr_solve* sv) { return {sv->n, sv->b, sv->dtype, sv->nrhs_max}; }
}  // namespace tqr

extern "C" {

int tqr_solve_ticket(int T, int nstrips, int trans, int ticket, int* strip, int* row) {
  if (T < 1 || nstrips < 1 || (trans != TQR_NOTRANS && trans != TQR_TRANS) || !strip || !row || ticket < 0 ||
      (long long)ticket >= (long long)T * nstrips)
    return TQR_EINVAL;
  solve_ticket_map(T, nstrips, trans == TQR_TRANS, ticket, strip, row);
  return TQR_OK;
}

void tqr_solve_destroy(tqr_solve* sv) {
  if (!sv) return;
  if (sv->evDone) {
    (void)hipEventSynchronize(sv->evDone);  // the last call may still be reading the workspace
    (void)hipEventDestroy(sv->evDone);
  }
  if (sv->d_ws) (void)hipFree(sv->d_ws);
  delete sv;
}

int tqr_solve_create(tqr_solve** out, int n, int b, int dtype, int nrhs_max) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if ((dtype != TQR_F32 && dtype != TQR_F64) || !solve_valid_b(b) || n <= 0 || n % b || nrhs_max < 1 ||
      !solve_valid_ld(n, dtype == TQR_F64 ? 8 : 4))
    return TQR_EINVAL;
  const size_t nstrips = ((size_t)nrhs_max + 63) / 64, items = nstrips * (size_t)(n / b);
  if (items > 0x7fffffffull) return TQR_EINVAL;  // (one workgroup per item: the grid)
  tqr_solve* sv = new (std::nothrow) tqr_solve();
  if (!sv) return TQR_ENOMEM;
  sv->n = n; sv->b = b; sv->dtype = dtype; sv->nrhs_max = nrhs_max; sv->nt = n / b; sv->nstrips_max = (int)nstrips;
  sv->es = dtype == TQR_F64 ? 8 : 4;
  sv->ws_bytes = ((size_t)PIPE_HDR + items) * sizeof(int);
  sv->kn = pipe_kernel_b(b, dtype, TQR_NOTRANS);
  sv->kt = pipe_kernel_b(b, dtype, TQR_TRANS);
  // without a gfx950 the handle exists but holds no device memory: every tqr_solve_trsm_r on it
  // validates its arguments and then returns TQR_ENODEV
  const int st = solve_pipe_ready(sv);
  if (st != TQR_OK && st != TQR_ENODEV) {
    tqr_solve_destroy(sv);
    return st;
  }
  *out = sv;
  return TQR_OK;
}

size_t tqr_solve_workspace_bytes(const tqr_solve* sv) { return sv ? sv->ws_bytes : 0; }

int tqr_solve_trsm_r(tqr_solve* sv, int trans, const void* dA, int ldda, void* dX, int nrhs, int lddx, void* stream) {
  if (!sv || (trans != TQR_NOTRANS && trans != TQR_TRANS) || !dA || !dX || nrhs < 1 || nrhs > sv->nrhs_max ||
      ldda < sv->n || lddx < sv->n || !solve_valid_ld(ldda, sv->es) || !solve_valid_ld(lddx, sv->es))
    return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(sv->mu);
  if (const int st = solve_pipe_ready(sv)) return st;
  HIPCHK(hipStreamWaitEvent(cs, sv->evDone, 0));  // the previous call of this handle (any stream)
  if (sv->epoch == INT_MAX) {  // the epochs start over: behind the previous call, ahead of this one
    HIPCHK(hipMemsetAsync(sv->d_ws + PIPE_HDR, 0, sv->ws_bytes - PIPE_HDR * sizeof(int), cs));
    sv->epoch = 0;
  }
  PipeArgs a;
  a.A = dA; a.X = dX; a.lda = ldda; a.ldx = lddx; a.nt = sv->nt; a.nrhs = nrhs;
  a.epoch = sv->epoch + 1;
  a.ws = sv->d_ws;
  const unsigned grid = (unsigned)((nrhs + 63) / 64) * (unsigned)a.nt;
  HIPCHK(hipMemsetAsync(sv->d_ws + PIPE_TICKET, 0, sizeof(int), cs));  // (the error word stays: tqr_solve_status)
  hipLaunchKernelGGL(trans == TQR_TRANS ? sv->kt : sv->kn, dim3(grid), dim3(NT), PIPE_LDS, cs, a);
  const hipError_t le = hipGetLastError();
  // recorded behind whatever was enqueued, so the next call stays ordered after it
  const hipError_t re = hipEventRecord(sv->evDone, cs);
  HIPCHK(le);
  sv->epoch = a.epoch;  // committed once the launch is enqueued
  HIPCHK(re);
  return TQR_OK;
}

int tqr_solve_status(tqr_solve* sv, void* stream) {
  if (!sv) return TQR_EINVAL;
  std::lock_guard<std::mutex> lk(sv->mu);
  if (!sv->d_ws) return TQR_OK;  // nothing was ever enqueued
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipEventSynchronize(sv->evDone));  // the handle's last call, whatever its stream
  int err = 0;
  HIPCHK(hipMemcpy(&err, sv->d_ws + PIPE_ERR, sizeof(int), hipMemcpyDeviceToHost));
  if (!err) return TQR_OK;
  fprintf(stderr, "tqr: pipelined solve: a wait for another workgroup's tile row timed out (error word %d)\n", err);
  HIPCHK(hipMemset(sv->d_ws + PIPE_ERR, 0, sizeof(int)));  // reported once; the handle is usable again
  return TQR_EHIP;
}

// tqr_lstsq_fused (solve.hip) with the pipelined solve in place of tqr_trsm_r
int tqr_lstsq_fused_solve(tqr_plan* plan, tqr_solve* sv, void* dAB, int ldda, void* dtau, int nrhs, void* dres,
                          void* stream) {
  if (!plan || !sv || !dAB || !dtau) return TQR_EINVAL;
  const PlanShape ps = plan_shape(plan);
  const int n = ps.steps * ps.b;  // A's columns; B's tile columns follow
  if (!ps.capped || n >= ps.n || ps.m < n || nrhs < 1 || nrhs > ps.n - n || ldda < ps.m ||
      !solve_valid_ld(ldda, ps.dtype == TQR_F64 ? 8 : 4) || sv->n != n || sv->b != ps.b || sv->dtype != ps.dtype ||
      nrhs > sv->nrhs_max)
    return TQR_EINVAL;
  void* dB = (char*)dAB + (size_t)n * (size_t)ldda * sv->es;
  int st;
  if ((st = tqr_plan_execute(plan, dAB, ldda, dtau, stream)) != TQR_OK) return st;
  if ((st = tqr_solve_trsm_r(sv, TQR_NOTRANS, dAB, ldda, dB, nrhs, ldda, stream)) != TQR_OK) return st;
  return dres ? resnorm(ps.dtype, dB, ldda, n, ps.m, nrhs, dres, stream) : TQR_OK;
}

}  // extern "C"
