// Triangular solve with the R of a finished tiled factorisation (include/tqr.h "solve"), and the
// residual norms of tqr_lstsq. Single GPU.
//
//   tqr_trsm_r   k_trsm_r: X <- R^{-1} X or X <- R^{-T} X in place. One 4-wave workgroup per 64
//                columns of X (a wave owns 16, the strip layout of k_apply_q) walks the tile rows of
//                R serially — k descending for R (back substitution), ascending for R^T. Per step
//                it solves the diagonal tile (k,k) against the strip X_k held in registers, stores
//                X_k, then subtracts R_ik X_k (R: i < k) or R_ki^T X_k (R^T: i > k) from every other
//                tile row still to be solved.
//   resnorm      k_resnorm: the 2-norm of rows n .. m-1 of every column of Q^T B.
//   tqr_lstsq_fused  host only: a capped plan's execute over [A | B], then the two above on B.
// R is read where the factorisation left it: the GEQRT V below the diagonal of the diagonal tiles
// is replaced by zeros with a select while the tile is staged, and never enters a product.
// The column strips of X are independent, so workgroups never communicate: the only
// synchronisation is the __syncthreads() around the LDS staging of an operand image.
// Every element of X is loaded and stored by one lane only (its column's lane with x = row mod 4),
// so the rows a step stores and a later step reloads are ordered by program order.
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "solve.hpp"
#include "solve_dev.hpp"
#include "tqr.h"

namespace tqr {

// (SolveArgs and the kernel's body trsm_r_body, which batch_apply.hip's k_trsm_r_batch shares, and the
// operand images stage_r, the substitution subst and the strip loads load_h / load_x, which
// solve_pipe.hip's kernel shares: solve_dev.hpp)

// ---------------------------------------------------------------------------------------
// solve: trsm_r_body on the launch's own arguments, one workgroup per 64 columns of X
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT, 2) void k_trsm_r(SolveArgs a) {
  extern __shared__ __align__(16) double lds[];
  trsm_r_body<B, S, TRANS>(a, blockIdx.x, lds);
}

// ---------------------------------------------------------------------------------------
// res[c] = |rows n .. m-1 of column c|_2 (tqr_lstsq): one workgroup per column, thread t sums the
// squares of rows n + t, n + t + NT, ... in fp64, then the fixed tree of block_sum — the same bits
// on every run. Unscaled: see include/tqr.h for the range.
// ---------------------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(NT) void k_resnorm(const S* __restrict__ Bm, size_t ldb, int n, int m, S* __restrict__ res) {
  __shared__ double red[4];
  const S* c = Bm + (size_t)blockIdx.x * ldb;
  double s = 0.0;
  for (int i = n + (int)threadIdx.x; i < m; i += NT) {
    const double v = (double)c[i];
    s = fma(v, v, s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) res[blockIdx.x] = (S)sqrt(s);
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
typedef void (*sfn)(SolveArgs);
template <int B>
static sfn solve_kernel(int dtype, int trans) {
  if (dtype == TQR_F64) return trans == TQR_TRANS ? k_trsm_r<B, double, true> : k_trsm_r<B, double, false>;
  return trans == TQR_TRANS ? k_trsm_r<B, float, true> : k_trsm_r<B, float, false>;
}
// (lds_solve: solve_dev.hpp)

// the current device is a gfx950, and the kernel may use its dynamic LDS (host-side calls only)
static int solve_ready(sfn fn, size_t ldsz) {
  if (const int st = current_device_is_gfx950()) return st;
  HIPCHK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsz));
  return TQR_OK;
}

int resnorm(int dtype, const void* dB, int lddb, int n, int m, int nrhs, void* dres, void* stream) {
  hipStream_t cs = (hipStream_t)stream;
  if (dtype == TQR_F64)
    hipLaunchKernelGGL(k_resnorm<double>, dim3((unsigned)nrhs), dim3(NT), 0, cs, (const double*)dB, (size_t)lddb, n, m, (double*)dres);
  else
    hipLaunchKernelGGL(k_resnorm<float>, dim3((unsigned)nrhs), dim3(NT), 0, cs, (const float*)dB, (size_t)lddb, n, m, (float*)dres);
  HIPCHK(hipGetLastError());
  return TQR_OK;
}

}  // namespace tqr

using namespace tqr;

extern "C" {

int tqr_trsm_r(int dtype, int trans, int n, int b, const void* dA, int ldda, void* dX, int nrhs, int lddx, void* stream) {
  if ((dtype != TQR_F32 && dtype != TQR_F64) || (trans != TQR_NOTRANS && trans != TQR_TRANS) || !valid_b(b) || n <= 0 ||
      n % b || nrhs < 1 || !dA || !dX || ldda < n || lddx < n)
    return TQR_EINVAL;
  const size_t es = elem_size(dtype);
  if (!valid_ld(ldda, es) || !valid_ld(lddx, es)) return TQR_EINVAL;
  const sfn fn = dispatch_b(b, [&](auto bb) { return solve_kernel<decltype(bb)::value>(dtype, trans); });
  const int st = solve_ready(fn, lds_solve(b));
  if (st != TQR_OK) return st;
  SolveArgs a;
  a.A = dA; a.X = dX; a.lda = ldda; a.ldx = lddx; a.nt = n / b; a.nrhs = nrhs;
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(NT), lds_solve(b), (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return TQR_OK;
}

// Least squares in one factorisation launch (include/tqr.h "solve"): the capped plan over [A | B]
// leaves Q^T B in B's place (the engine's chains, pipelined over the steps), so what remains is the
// solve with R and the residual norms — tqr_lstsq's own last two steps, on B's columns inside dAB.
int tqr_lstsq_fused(tqr_plan* plan, void* dAB, int ldda, void* dtau, int nrhs, void* dres, void* stream) {
  if (!plan || !dAB || !dtau) return TQR_EINVAL;
  const PlanShape ps = plan_shape(plan);
  const int n = ps.steps * ps.b;  // A's columns; B's tile columns follow
  if (!ps.capped || n >= ps.n || ps.m < n || nrhs < 1 || nrhs > ps.n - n || ldda < ps.m ||
      !valid_ld(ldda, elem_size(ps.dtype)))
    return TQR_EINVAL;
  void* dB = (char*)dAB + (size_t)n * (size_t)ldda * elem_size(ps.dtype);
  int st;
  if ((st = tqr_plan_execute(plan, dAB, ldda, dtau, stream)) != TQR_OK) return st;
  if ((st = tqr_trsm_r(ps.dtype, TQR_NOTRANS, n, ps.b, dAB, ldda, dB, nrhs, ldda, stream)) != TQR_OK) return st;
  return dres ? resnorm(ps.dtype, dB, ldda, n, ps.m, nrhs, dres, stream) : TQR_OK;
}

}  // extern "C"
