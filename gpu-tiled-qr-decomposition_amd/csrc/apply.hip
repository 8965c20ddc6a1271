// Apply Q or Q^T of a finished tiled factorisation to a separate matrix C (include/tqr.h
// "apply"): the ormqr to the plan's geqrf. Single GPU.
//
//   tqr_apply_prepare  k_apply_t: one workgroup per (tile, reflector group) rebuilds the group's
//                      T factor from the stored V and tau (tiles.hpp build_t, as the engine's
//                      k_build_t) into the handle's workspace — once per factorisation.
//   tqr_apply_q        k_apply_q: one 4-wave workgroup per 64 columns of C (a wave owns 16, the
//                      strip layout of the engine's k_update) walks the whole reflector sequence
//                      for its columns: per step k the UNMQR of tile (k,k) on C_k, then the TSMQR
//                      of every tile (l,k), l > k, on [C_k; C_l] — Q^T; the exact reverse for Q.
// The column strips of C are independent, so workgroups never communicate: the only
// synchronisation is the __syncthreads() around the LDS staging of a group's V and T.
// Every element of C is loaded and stored by one lane only (its column's lane with x = row mod
// 4), so the head rows a step stores and the next step reloads are ordered by program order.
// The device helpers of k_apply_q live in apply_dev.hpp and the handle in apply.hpp: apply_pipe.hip
// runs the same tile operations with one workgroup per (strip, step) on them.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>

#include "apply.hpp"
#include "apply_dev.hpp"
#include "host_common.hpp"
#include "solve.hpp"
#include "tqr.h"

namespace tqr {

// ---------------------------------------------------------------------------------------
// The kernels: the bodies of apply_dev.hpp (apply_t_body: one workgroup per (tile, reflector group);
// apply_q_body: one per 64 columns of C) on the launch's own arguments
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_apply_t(ApplyArgs a) {
  extern __shared__ __align__(16) double lds[];
  apply_t_body<B, S>(a, blockIdx.x, lds);
}

template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT, 2) void k_apply_q(ApplyArgs a) {
  extern __shared__ __align__(16) double lds[];
  apply_q_body<B, S, TRANS>(a, blockIdx.x, lds);
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
template <int B, typename S>
static void apply_kernels(afn* t, afn* qt, afn* qn) {
  *t = k_apply_t<B, S>;
  *qt = k_apply_q<B, S, true>;
  *qn = k_apply_q<B, S, false>;
}
// (lds_apply_q, lds_apply_t, timg_doubles, apply_ws_bytes: apply.hpp)
static_assert(Geo<256>::TIMG == 1152 && Geo<16>::TIMG == 384, "host timg_doubles mirrors Geo::TIMG");

}  // namespace tqr

using namespace tqr;

extern "C" {

void tqr_apply_destroy(tqr_apply* ap) {
  if (!ap) return;
  if (ap->d_T) (void)hipFree(ap->d_T);
  if (ap->evPrep) (void)hipEventDestroy(ap->evPrep);
  for (hipEvent_t e : ap->evApply)
    if (e) (void)hipEventDestroy(e);
  delete ap;
}

int tqr_apply_create(tqr_apply** out, int m, int n, int b, int dtype) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || (dtype != TQR_F32 && dtype != TQR_F64) ||
      !valid_ld(m, elem_size(dtype)))
    return TQR_EINVAL;
  if (const int st = current_device_is_gfx950()) return st;
  tqr_apply* ap = new (std::nothrow) tqr_apply();
  if (!ap) return TQR_ENOMEM;
  ap->m = m; ap->n = n; ap->b = b; ap->p = m / b; ap->q = n / b;
  ap->kmax = ap->p < ap->q ? ap->p : ap->q;
  ap->dtype = dtype;
  ap->es = elem_size(dtype);
  ap->ws_bytes = apply_ws_bytes(ap->p, ap->kmax, b);
  dispatch_b(b, [&](auto bb) {
    if (dtype == TQR_F64) apply_kernels<decltype(bb)::value, double>(&ap->kt, &ap->kqt, &ap->kqn);
    else apply_kernels<decltype(bb)::value, float>(&ap->kt, &ap->kqt, &ap->kqn);
  });
  if (hipFuncSetAttribute((const void*)ap->kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_t(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)ap->kqt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)ap->kqn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(b)) != hipSuccess) {
    tqr_apply_destroy(ap);
    return TQR_EHIP;
  }
  if (hipMalloc(&ap->d_T, ap->ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    tqr_apply_destroy(ap);
    return TQR_ENOMEM;
  }
  bool ok = hipEventCreateWithFlags(&ap->evPrep, hipEventDisableTiming) == hipSuccess;
  for (int s = 0; ok && s < APPLY_NSLOT; ++s)
    ok = hipEventCreateWithFlags(&ap->evApply[s], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    tqr_apply_destroy(ap);
    return TQR_EHIP;
  }
  *out = ap;
  return TQR_OK;
}

size_t tqr_apply_workspace_bytes(const tqr_apply* ap) { return ap ? ap->ws_bytes : 0; }

int tqr_apply_prepare(tqr_apply* ap, const void* dA, int ldda, const void* dtau, void* stream) {
  if (!ap || !dA || !dtau || ldda < ap->m || !valid_ld(ldda, ap->es)) return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(ap->mu);
  // the workspace is rewritten: wait for every apply enqueued since the last prepare
  for (int s = 0; s < ap->nslot; ++s) HIPCHK(hipStreamWaitEvent(cs, ap->evApply[s], 0));
  ap->nslot = 0;
  ApplyArgs a;
  a.A = dA; a.tau = dtau; a.C = nullptr; a.Tw = ap->d_T; a.lda = ldda; a.ldc = 0;
  a.m = ap->m; a.p = ap->p; a.kmax = ap->kmax; a.nrhs = 0;
  const size_t ng = ap->b / (ap->b < 32 ? ap->b : 32);
  const size_t grid = tile_slot(ap->kmax, ap->kmax, ap->p) * ng;
  if (grid > 0x7fffffffull) return TQR_EINVAL;
  hipLaunchKernelGGL(ap->kt, dim3((unsigned)grid), dim3(NT), lds_apply_t(ap->b), cs, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ap->evPrep, cs));
  ap->prepared = true;
  return TQR_OK;
}

int tqr_apply_q(tqr_apply* ap, int trans, const void* dA, int ldda, void* dC, int nrhs, int lddc, void* stream) {
  if (!ap || !dA || !dC || nrhs < 1 || ldda < ap->m || lddc < ap->m || !valid_ld(ldda, ap->es) ||
      !valid_ld(lddc, ap->es) || (trans != TQR_NOTRANS && trans != TQR_TRANS))
    return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(ap->mu);
  if (!ap->prepared) return TQR_EINVAL;
  int slot = 0;
  HIPCHK(apply_enqueue_begin(ap, cs, &slot));
  ApplyArgs a;
  a.A = dA; a.tau = nullptr; a.C = dC; a.Tw = ap->d_T; a.lda = ldda; a.ldc = lddc;
  a.m = ap->m; a.p = ap->p; a.kmax = ap->kmax; a.nrhs = nrhs;
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  hipLaunchKernelGGL(trans == TQR_TRANS ? ap->kqt : ap->kqn, dim3(grid), dim3(NT), lds_apply_q(ap->b), cs, a);
  HIPCHK(hipGetLastError());
  HIPCHK(apply_enqueue_end(ap, cs, slot));
  return TQR_OK;
}

// Both gels directions on the handle's factorisation (include/tqr.h "solve"): the apply above and
// solve.hip's tqr_trsm_r / resnorm enqueued on `stream`, nothing allocated. The solve reads dA
// only (not the T workspace), so it needs none of the handle's events.
int tqr_lstsq(tqr_apply* ap, int trans, const void* dA, int ldda, void* dB, int nrhs, int lddb, void* dres,
              void* stream) {
  if (!ap || !dA || !dB || nrhs < 1 || ap->m < ap->n || ldda < ap->m || lddb < ap->m || !valid_ld(ldda, ap->es) ||
      !valid_ld(lddb, ap->es) || (trans != TQR_NOTRANS && trans != TQR_TRANS))
    return TQR_EINVAL;
  {
    std::lock_guard<std::mutex> lk(ap->mu);
    if (!ap->prepared) return TQR_EINVAL;
  }
  int st;
  if (trans == TQR_NOTRANS) {
    // B <- Q^T B; rows 0 .. n-1 <- R^{-1} of them; the residual norms from rows n .. m-1
    if ((st = tqr_apply_q(ap, TQR_TRANS, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
    if ((st = tqr_trsm_r(ap->dtype, TQR_NOTRANS, ap->n, ap->b, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
    return dres ? resnorm(ap->dtype, dB, lddb, ap->n, ap->m, nrhs, dres, stream) : TQR_OK;
  }
  // x = Q [R^{-T} c; 0]
  if (ap->m > ap->n)
    HIPCHK(hipMemset2DAsync((char*)dB + (size_t)ap->n * ap->es, (size_t)lddb * ap->es, 0, (size_t)(ap->m - ap->n) * ap->es,
                            (size_t)nrhs, (hipStream_t)stream));
  if ((st = tqr_trsm_r(ap->dtype, TQR_TRANS, ap->n, ap->b, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
  return tqr_apply_q(ap, TQR_NOTRANS, dA, ldda, dB, nrhs, lddb, stream);
}

}  // extern "C"
