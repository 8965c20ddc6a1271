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
// The protocol between the workgroups — tickets, sc1 hand-over, epoch flags, bounded waits — is
// pipe_dev.hpp's. Here a work item is (strip, tile row) by pipe_ticket_map over the nt tile rows, the
// producers of a row are the rows solved before it in the same strip, every load and store of X is an
// sc1 access, and flag [strip][row] holds the epoch of the call whose X_row of the strip is final.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>

#include "host_common.hpp"
#include "pipe_dev.hpp"
#include "pipe_host.hpp"
#include "solve.hpp"
#include "solve_dev.hpp"
#include "tqr.h"

namespace tqr {

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

  const int tk = pipe_take_ticket(a.ws, &s_tk), nstrips = (a.nrhs + 63) >> 6;
  if (tk < 0 || tk >= a.nt * nstrips) return;  // (an earlier call of the handle timed out: tqr_solve_status)
  int strip, i;
  pipe_ticket_map(a.nt, nstrips, TRANS, tk, &strip, &i);

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
  auto wait = [&](int k) { return pipe_wait(ws + fl + k, epoch, ws + PIPE_ERR, &s_ok); };
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
  pipe_publish(ws + fl + i, epoch);  // X_i
}

typedef void (*pfn)(PipeArgs);
template <int B>
static pfn pipe_kernel(int dtype, int trans) {
  if (dtype == TQR_F64) return trans == TQR_TRANS ? k_trsm_r_pipe<B, double, true> : k_trsm_r_pipe<B, double, false>;
  return trans == TQR_TRANS ? k_trsm_r_pipe<B, float, true> : k_trsm_r_pipe<B, float, false>;
}
static pfn pipe_kernel_b(int b, int dtype, int trans) {
  return dispatch_b(b, [&](auto bb) { return pipe_kernel<decltype(bb)::value>(dtype, trans); });
}

}  // namespace tqr

using namespace tqr;

struct tqr_solve {
  int n, b, dtype, nrhs_max, nt, nstrips_max;
  size_t es;
  pfn kn = nullptr, kt = nullptr;
  PipeCore core;
};

namespace tqr {
SolveShape solve_shape(const tqr_solve* sv) { return {sv->n, sv->b, sv->dtype, sv->nrhs_max}; }
}  // namespace tqr

extern "C" {

int tqr_solve_ticket(int T, int nstrips, int trans, int ticket, int* strip, int* row) {
  if (T < 1 || nstrips < 1 || (trans != TQR_NOTRANS && trans != TQR_TRANS) || !strip || !row || ticket < 0 ||
      (long long)ticket >= (long long)T * nstrips)
    return TQR_EINVAL;
  pipe_ticket_map(T, nstrips, trans == TQR_TRANS, ticket, strip, row);
  return TQR_OK;
}

void tqr_solve_destroy(tqr_solve* sv) {
  if (!sv) return;
  pipe_destroy(sv->core);
  delete sv;
}

int tqr_solve_create(tqr_solve** out, int n, int b, int dtype, int nrhs_max) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if ((dtype != TQR_F32 && dtype != TQR_F64) || !valid_b(b) || n <= 0 || n % b || nrhs_max < 1 ||
      !valid_ld(n, elem_size(dtype)))
    return TQR_EINVAL;
  const size_t nstrips = ((size_t)nrhs_max + 63) / 64, items = nstrips * (size_t)(n / b);
  if (items > 0x7fffffffull) return TQR_EINVAL;  // (one workgroup per item: the grid)
  tqr_solve* sv = new (std::nothrow) tqr_solve();
  if (!sv) return TQR_ENOMEM;
  sv->n = n; sv->b = b; sv->dtype = dtype; sv->nrhs_max = nrhs_max; sv->nt = n / b; sv->nstrips_max = (int)nstrips;
  sv->es = elem_size(dtype);
  sv->core.ws_bytes = ((size_t)PIPE_HDR + items) * sizeof(int);
  sv->core.kern[0] = (const void*)(sv->kn = pipe_kernel_b(b, dtype, TQR_NOTRANS));
  sv->core.kern[1] = (const void*)(sv->kt = pipe_kernel_b(b, dtype, TQR_TRANS));
  // without a gfx950 the handle exists but holds no device memory: every tqr_solve_trsm_r on it
  // validates its arguments and then returns TQR_ENODEV
  const int st = pipe_ready(sv->core);
  if (st != TQR_OK && st != TQR_ENODEV) {
    tqr_solve_destroy(sv);
    return st;
  }
  *out = sv;
  return TQR_OK;
}

size_t tqr_solve_workspace_bytes(const tqr_solve* sv) { return sv ? sv->core.ws_bytes : 0; }

int tqr_solve_trsm_r(tqr_solve* sv, int trans, const void* dA, int ldda, void* dX, int nrhs, int lddx, void* stream) {
  if (!sv || (trans != TQR_NOTRANS && trans != TQR_TRANS) || !dA || !dX || nrhs < 1 || nrhs > sv->nrhs_max ||
      ldda < sv->n || lddx < sv->n || !valid_ld(ldda, sv->es) || !valid_ld(lddx, sv->es))
    return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(sv->core.mu);
  if (const int st = pipe_ready(sv->core)) return st;
  PipeArgs a;
  if (const int st = pipe_call_begin(sv->core, cs, &a.epoch)) return st;
  a.A = dA; a.X = dX; a.lda = ldda; a.ldx = lddx; a.nt = sv->nt; a.nrhs = nrhs;
  a.ws = sv->core.d_ws;
  const unsigned grid = (unsigned)((nrhs + 63) / 64) * (unsigned)a.nt;
  hipLaunchKernelGGL(trans == TQR_TRANS ? sv->kt : sv->kn, dim3(grid), dim3(NT), PIPE_LDS, cs, a);
  return pipe_call_end(sv->core, cs, hipGetLastError(), a.epoch);
}

int tqr_solve_status(tqr_solve* sv, void* stream) {
  return sv ? pipe_status(sv->core, stream, "solve: a wait for another workgroup's tile row") : TQR_EINVAL;
}

// tqr_lstsq_fused (solve.hip) with the pipelined solve in place of tqr_trsm_r
int tqr_lstsq_fused_solve(tqr_plan* plan, tqr_solve* sv, void* dAB, int ldda, void* dtau, int nrhs, void* dres,
                          void* stream) {
  if (!plan || !sv || !dAB || !dtau) return TQR_EINVAL;
  const PlanShape ps = plan_shape(plan);
  const int n = ps.steps * ps.b;  // A's columns; B's tile columns follow
  if (!ps.capped || n >= ps.n || ps.m < n || nrhs < 1 || nrhs > ps.n - n || ldda < ps.m ||
      !valid_ld(ldda, elem_size(ps.dtype)) || sv->n != n || sv->b != ps.b || sv->dtype != ps.dtype ||
      nrhs > sv->nrhs_max)
    return TQR_EINVAL;
  void* dB = (char*)dAB + (size_t)n * (size_t)ldda * sv->es;
  int st;
  if ((st = tqr_plan_execute(plan, dAB, ldda, dtau, stream)) != TQR_OK) return st;
  if ((st = tqr_solve_trsm_r(sv, TQR_NOTRANS, dAB, ldda, dB, nrhs, ldda, stream)) != TQR_OK) return st;
  return dres ? resnorm(ps.dtype, dB, ldda, n, ps.m, nrhs, dres, stream) : TQR_OK;
}

}  // extern "C"
