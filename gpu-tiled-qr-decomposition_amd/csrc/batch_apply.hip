// Batched apply, form-Q, solve and least squares on a strided batch of factorisations (include/tqr.h
// "batched apply and solve"): what tqr_apply_* / tqr_trsm_r / tqr_lstsq do on one factorisation, on
// every member of a tqr_batch_execute layout in the launches of one.
//
//   tqr_batch_apply_prepare  k_apply_t_batch: the T images of every member into the handle's workspace;
//   tqr_batch_apply_q        k_apply_q_batch: C_i <- Q_i^T C_i or Q_i C_i;
//   tqr_batch_form_q         k_fill_eye_batch (the first ncols columns of I_m), then k_apply_q_batch;
//   tqr_batch_trsm_r         k_trsm_r_batch: X_i <- R_i^{-1} X_i or R_i^{-T} X_i;
//   tqr_batch_lstsq          the three above, k_zero_rows_batch and k_resnorm_batch composed as tqr_lstsq
//                            composes the per-member calls.
// The kernels are the per-member bodies (apply_dev.hpp, solve_dev.hpp) with the member on blockIdx.y:
// its offset is taken in 64 bits on the base pointers, and inside a member the offsets are the
// per-member kernels' own. A member therefore has the bytes of the per-member call on it alone.
// Every launch is ordered by its stream only: no flags, counters or waits between workgroups. More
// members than a grid's y (or z) holds run as consecutive launches with advanced base pointers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>

#include "apply.hpp"
#include "apply_batch_dev.hpp"
#include "apply_dev.hpp"
#include "batch_layout.hpp"
#include "host_common.hpp"
#include "solve_dev.hpp"
#include "tqr.h"

namespace tqr {

// ---------------------------------------------------------------------------------------
// solve: trsm_r_body (solve_dev.hpp) of strip blockIdx.x on member blockIdx.y
// ---------------------------------------------------------------------------------------
struct SolveBatchArgs {
  SolveArgs a;          // member 0 of the launch
  long long sA, sX;     // elements between consecutive members
};

template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT, 2) void k_trsm_r_batch(SolveBatchArgs sa) {
  extern __shared__ __align__(16) double lds[];
  SolveArgs a = sa.a;
  const size_t i = blockIdx.y;
  a.A = (const S*)a.A + i * (size_t)sa.sA;
  a.X = (S*)a.X + i * (size_t)sa.sX;
  trsm_r_body<B, S, TRANS>(a, blockIdx.x, lds);
}

// ---------------------------------------------------------------------------------------
// res_i[c] = |rows n .. m-1 of column c of member i|_2: solve.hip's k_resnorm — its loop, its
// block_sum tree, so the same bits — with the column on blockIdx.x and the member on blockIdx.y
// ---------------------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(NT) void k_resnorm_batch(const S* __restrict__ Bm, size_t ldb, long long sB, int n, int m,
                                                     S* __restrict__ res, long long sRes) {
  __shared__ double red[4];
  const size_t i = blockIdx.y;
  const S* c = Bm + i * (size_t)sB + (size_t)blockIdx.x * ldb;
  double s = 0.0;
  for (int r = n + (int)threadIdx.x; r < m; r += NT) {
    const double v = (double)c[r];
    s = fma(v, v, s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) res[i * (size_t)sRes + blockIdx.x] = (S)sqrt(s);
}

// ---------------------------------------------------------------------------------------
// Fills: one thread per element, consecutive threads on consecutive rows of a column (coalesced),
// columns on blockIdx.y (strided when there are more than a grid's y holds), the member on blockIdx.z.
// ---------------------------------------------------------------------------------------
struct FillArgs {
  void* dst;         // member 0 of the launch, at the first row written
  long ld;
  long long stride;  // elements between consecutive members
  int rows;          // rows written, from dst's on
  int ncols;
};
constexpr int CT = 256;

// the first ncols columns of I_m (dst at row 0, rows == m)
template <typename S>
__global__ __launch_bounds__(CT) void k_fill_eye_batch(FillArgs f) {
  const long r = (long)blockIdx.x * CT + threadIdx.x;
  if (r >= f.rows) return;
  S* dst = (S*)f.dst + (size_t)blockIdx.z * (size_t)f.stride + r;
  for (int j = blockIdx.y; j < f.ncols; j += gridDim.y) dst[(size_t)j * f.ld] = r == j ? S(1) : S(0);
}
// zeros in `rows` rows of ncols columns
template <typename S>
__global__ __launch_bounds__(CT) void k_zero_rows_batch(FillArgs f) {
  const long r = (long)blockIdx.x * CT + threadIdx.x;
  if (r >= f.rows) return;
  S* dst = (S*)f.dst + (size_t)blockIdx.z * (size_t)f.stride + r;
  for (int j = blockIdx.y; j < f.ncols; j += gridDim.y) dst[(size_t)j * f.ld] = S(0);
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
typedef void (*abfn)(ApplyBatchArgs);
typedef void (*sbfn)(SolveBatchArgs);
typedef void (*ffn)(FillArgs);

template <int B, typename S>
static void apply_batch_kernels(abfn* t, abfn* qt, abfn* qn) {
  *t = k_apply_t_batch<B, S>;
  *qt = k_apply_q_batch<B, S, true>;
  *qn = k_apply_q_batch<B, S, false>;
}
template <int B>
static sbfn solve_batch_kernel(int dtype, int trans) {
  if (dtype == TQR_F64) return trans == TQR_TRANS ? k_trsm_r_batch<B, double, true> : k_trsm_r_batch<B, double, false>;
  return trans == TQR_TRANS ? k_trsm_r_batch<B, float, true> : k_trsm_r_batch<B, float, false>;
}
static sbfn solve_batch_kernel_of(int b, int dtype, int trans) {
  return dispatch_b(b, [&](auto bb) { return solve_batch_kernel<decltype(bb)::value>(dtype, trans); });
}

constexpr int kMaxGridYZ = 65535;

// tqr_apply_create's argument errors, batch < 1, a prepare grid beyond 2^31 (one workgroup per T image)
// and a workspace beyond a size_t
static bool batch_apply_shape_ok(int m, int n, int b, int dtype, int batch) {
  if (!valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || (dtype != TQR_F32 && dtype != TQR_F64) ||
      !valid_ld(m, elem_size(dtype)) || batch < 1)
    return false;
  const int p = m / b, q = n / b;
  const size_t per = apply_ws_bytes(p, std::min(p, q), b);
  return per / (timg_doubles(b) * sizeof(double)) <= 0x7fffffffull && batch_total_bytes(batch, per) != 0;
}

// a member layout of rows x cols under (ld, stride): ld, the leading-dimension bound, the stride form
static bool layout_ok(int rows, int cols, int batch, int ld, long long stride, size_t es) {
  return ld >= rows && valid_ld(ld, es) && batch_stride_ok(rows, cols, batch, ld, stride);
}
static bool trans_ok(int trans) { return trans == TQR_NOTRANS || trans == TQR_TRANS; }

// ---- launches (arguments checked; strides already 0 where batch == 1) ---------------------------
// X_i <- op(R_i)^{-1} X_i, fn = solve_batch_kernel_of(b, dtype, trans) with its LDS limit set
static int launch_trsm(sbfn fn, int n, int b, int batch, size_t es, const void* dA, int ldda, long long sA, void* dX,
                       int nrhs, int lddx, long long sX, hipStream_t cs) {
  SolveBatchArgs sa;
  sa.a.lda = ldda; sa.a.ldx = lddx; sa.a.nt = n / b; sa.a.nrhs = nrhs;
  sa.sA = sA; sa.sX = sX;
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  for (int i0 = 0; i0 < batch; i0 += kMaxGridYZ) {
    const unsigned nb = (unsigned)std::min(kMaxGridYZ, batch - i0);
    sa.a.A = (const char*)dA + (size_t)i0 * (size_t)sA * es;
    sa.a.X = (char*)dX + (size_t)i0 * (size_t)sX * es;
    hipLaunchKernelGGL(fn, dim3(grid, nb), dim3(NT), lds_solve(b), cs, sa);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

static int launch_fill(bool eye, int dtype, int batch, size_t es, void* dst, int ld, long long stride, int row0, int rows,
                       int ncols, hipStream_t cs) {
  if (rows <= 0) return TQR_OK;
  FillArgs f;
  f.ld = ld; f.stride = stride; f.rows = rows; f.ncols = ncols;
  const ffn fn = dtype == TQR_F64 ? (eye ? k_fill_eye_batch<double> : k_zero_rows_batch<double>)
                                  : (eye ? k_fill_eye_batch<float> : k_zero_rows_batch<float>);
  const unsigned gx = (unsigned)((rows + CT - 1) / CT), gy = (unsigned)std::min(ncols, kMaxGridYZ);
  for (int i0 = 0; i0 < batch; i0 += kMaxGridYZ) {
    const unsigned nb = (unsigned)std::min(kMaxGridYZ, batch - i0);
    f.dst = (char*)dst + ((size_t)i0 * (size_t)stride + (size_t)row0) * es;
    hipLaunchKernelGGL(fn, dim3(gx, gy, nb), dim3(CT), 0, cs, f);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

static int launch_resnorm(int dtype, int batch, size_t es, const void* dB, int lddb, long long sB, int n, int m, int nrhs,
                          void* dres, long long sRes, hipStream_t cs) {
  for (int i0 = 0; i0 < batch; i0 += kMaxGridYZ) {
    const unsigned nb = (unsigned)std::min(kMaxGridYZ, batch - i0);
    const char* Bm = (const char*)dB + (size_t)i0 * (size_t)sB * es;
    char* res = (char*)dres + (size_t)i0 * (size_t)sRes * es;
    if (dtype == TQR_F64)
      hipLaunchKernelGGL(k_resnorm_batch<double>, dim3((unsigned)nrhs, nb), dim3(NT), 0, cs, (const double*)Bm, (size_t)lddb,
                         sB, n, m, (double*)res, sRes);
    else
      hipLaunchKernelGGL(k_resnorm_batch<float>, dim3((unsigned)nrhs, nb), dim3(NT), 0, cs, (const float*)Bm, (size_t)lddb, sB,
                         n, m, (float*)res, sRes);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

}  // namespace tqr

using namespace tqr;

struct tqr_batch_apply {
  int m, n, b, p, q, kmax, dtype, batch;
  size_t es, per, ws_bytes;  // element size; bytes of one member's T images; of all
  bool ready = false;        // the device side exists (a gfx950 was present at create)
  bool prepared = false;     // a prepare has been enqueued successfully
  double* d_T = nullptr;     // member i's T images at d_T + i * per / 8
  abfn kt = nullptr, kqt = nullptr, kqn = nullptr;
  sbfn ksn = nullptr, kst = nullptr;  // the solve with R, with R^T
  hipEvent_t evDone = nullptr;
  std::mutex mu;  // one enqueue sequence at a time
};

// ---- launches on a handle (mu held, arguments checked, strides 0 where batch == 1) ---------------
static int enqueue_prepare(tqr_batch_apply* h, const void* dA, int ldda, long long sA, const void* dtau, long long sTau,
                           hipStream_t cs) {
  ApplyBatchArgs ba;
  ba.a.C = nullptr; ba.a.lda = ldda; ba.a.ldc = 0;
  ba.a.m = h->m; ba.a.p = h->p; ba.a.kmax = h->kmax; ba.a.nrhs = 0;
  ba.sA = sA; ba.sTau = sTau; ba.sC = 0; ba.sTw = (long long)(h->per / sizeof(double));
  const unsigned grid = (unsigned)(h->per / (timg_doubles(h->b) * sizeof(double)));
  for (int i0 = 0; i0 < h->batch; i0 += kMaxGridYZ) {
    const unsigned nb = (unsigned)std::min(kMaxGridYZ, h->batch - i0);
    ba.a.A = (const char*)dA + (size_t)i0 * (size_t)sA * h->es;
    ba.a.tau = (const char*)dtau + (size_t)i0 * (size_t)sTau * h->es;
    ba.a.Tw = h->d_T + (size_t)i0 * (size_t)ba.sTw;
    hipLaunchKernelGGL(h->kt, dim3(grid, nb), dim3(NT), lds_apply_t(h->b), cs, ba);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

static int enqueue_apply(tqr_batch_apply* h, int trans, const void* dA, int ldda, long long sA, void* dC, int nrhs, int lddc,
                         long long sC, hipStream_t cs) {
  ApplyBatchArgs ba;
  ba.a.tau = nullptr; ba.a.lda = ldda; ba.a.ldc = lddc;
  ba.a.m = h->m; ba.a.p = h->p; ba.a.kmax = h->kmax; ba.a.nrhs = nrhs;
  ba.sA = sA; ba.sTau = 0; ba.sC = sC; ba.sTw = (long long)(h->per / sizeof(double));
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  for (int i0 = 0; i0 < h->batch; i0 += kMaxGridYZ) {
    const unsigned nb = (unsigned)std::min(kMaxGridYZ, h->batch - i0);
    ba.a.A = (const char*)dA + (size_t)i0 * (size_t)sA * h->es;
    ba.a.C = (char*)dC + (size_t)i0 * (size_t)sC * h->es;
    ba.a.Tw = h->d_T + (size_t)i0 * (size_t)ba.sTw;
    hipLaunchKernelGGL(trans == TQR_TRANS ? h->kqt : h->kqn, dim3(grid, nb), dim3(NT), lds_apply_q(h->b), cs, ba);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

// The frame of every enqueueing call (tsqr.hip's tsqr_call): mutual exclusion, the stream waits for
// the handle's previous call, and the call is marked also behind a partly failed enqueue.
// `need_prepare`: TQR_EINVAL before the first prepare.
template <typename F>
static int batch_apply_call(tqr_batch_apply* h, bool need_prepare, void* stream, F enqueue) {
  if (!h->ready) return TQR_ENODEV;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(h->mu);
  if (need_prepare && !h->prepared) return TQR_EINVAL;
  HIPCHK(hipStreamWaitEvent(cs, h->evDone, 0));
  const int st = enqueue(cs);
  const hipError_t e = hipEventRecord(h->evDone, cs);
  if (st != TQR_OK) return st;
  HIPCHK(e);
  return TQR_OK;
}

// argument errors shared by apply_q / form_q / lstsq: pointers, the width, both layouts
static bool batch_apply_args_ok(const tqr_batch_apply* h, const void* dA, int ldda, long long sA, const void* dC, int nrhs,
                                int lddc, long long sC) {
  return h && dA && dC && nrhs >= 1 && layout_ok(h->m, h->n, h->batch, ldda, sA, h->es) &&
         layout_ok(h->m, nrhs, h->batch, lddc, sC, h->es);
}

extern "C" {

size_t tqr_batch_apply_bytes(int m, int n, int b, int dtype, int batch) {
  if (!batch_apply_shape_ok(m, n, b, dtype, batch)) return 0;
  const int p = m / b, q = n / b;
  return batch_total_bytes(batch, apply_ws_bytes(p, std::min(p, q), b));
}

void tqr_batch_apply_destroy(tqr_batch_apply* h) {
  if (!h) return;
  if (h->evDone) {
    (void)hipEventSynchronize(h->evDone);  // the last call may still be using the workspace
    (void)hipEventDestroy(h->evDone);
  }
  if (h->d_T) (void)hipFree(h->d_T);
  delete h;
}

int tqr_batch_apply_create(tqr_batch_apply** out, int m, int n, int b, int dtype, int batch) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!batch_apply_shape_ok(m, n, b, dtype, batch)) return TQR_EINVAL;
  tqr_batch_apply* h = new (std::nothrow) tqr_batch_apply();
  if (!h) return TQR_ENOMEM;
  h->m = m; h->n = n; h->b = b; h->p = m / b; h->q = n / b; h->kmax = std::min(h->p, h->q);
  h->dtype = dtype; h->es = elem_size(dtype); h->batch = batch;
  h->per = apply_ws_bytes(h->p, h->kmax, b);
  h->ws_bytes = batch_total_bytes(batch, h->per);
  // without a gfx950 the handle exists, holds no device memory, and every enqueueing call returns TQR_ENODEV
  if (current_device_is_gfx950() != TQR_OK) { *out = h; return TQR_OK; }
  dispatch_b(b, [&](auto bb) {
    if (dtype == TQR_F64) apply_batch_kernels<decltype(bb)::value, double>(&h->kt, &h->kqt, &h->kqn);
    else apply_batch_kernels<decltype(bb)::value, float>(&h->kt, &h->kqt, &h->kqn);
  });
  h->ksn = solve_batch_kernel_of(b, dtype, TQR_NOTRANS);
  h->kst = solve_batch_kernel_of(b, dtype, TQR_TRANS);
  if (hipFuncSetAttribute((const void*)h->kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_t(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)h->kqt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)h->kqn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)h->ksn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_solve(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)h->kst, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_solve(b)) != hipSuccess ||
      hipEventCreateWithFlags(&h->evDone, hipEventDisableTiming) != hipSuccess) {
    tqr_batch_apply_destroy(h);
    return TQR_EHIP;
  }
  if (hipMalloc(&h->d_T, h->ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    tqr_batch_apply_destroy(h);
    return TQR_ENOMEM;
  }
  h->ready = true;
  *out = h;
  return TQR_OK;
}

size_t tqr_batch_apply_workspace_bytes(const tqr_batch_apply* h) { return h ? h->ws_bytes : 0; }

int tqr_batch_apply_prepare(tqr_batch_apply* h, const void* dA, int ldda, long long strideA, const void* dtau,
                            long long strideTau, void* stream) {
  if (!h || !dA || !dtau || !layout_ok(h->m, h->n, h->batch, ldda, strideA, h->es) ||
      strideTau < (long long)h->m * h->kmax)
    return TQR_EINVAL;
  if (h->batch == 1) strideA = strideTau = 0;  // ignored
  return batch_apply_call(h, false, stream, [&](hipStream_t cs) -> int {
    const int st = enqueue_prepare(h, dA, ldda, strideA, dtau, strideTau, cs);
    if (st == TQR_OK) h->prepared = true;
    return st;
  });
}

int tqr_batch_apply_q(tqr_batch_apply* h, int trans, const void* dA, int ldda, long long strideA, void* dC, int nrhs, int lddc,
                      long long strideC, void* stream) {
  if (!batch_apply_args_ok(h, dA, ldda, strideA, dC, nrhs, lddc, strideC) || !trans_ok(trans)) return TQR_EINVAL;
  if (h->batch == 1) strideA = strideC = 0;
  return batch_apply_call(h, true, stream, [&](hipStream_t cs) -> int {
    return enqueue_apply(h, trans, dA, ldda, strideA, dC, nrhs, lddc, strideC, cs);
  });
}

int tqr_batch_form_q(tqr_batch_apply* h, const void* dA, int ldda, long long strideA, void* dQ, int ncols, int lddq,
                     long long strideQ, void* stream) {
  if (!batch_apply_args_ok(h, dA, ldda, strideA, dQ, ncols, lddq, strideQ) || ncols > h->m) return TQR_EINVAL;
  if (h->batch == 1) strideA = strideQ = 0;
  return batch_apply_call(h, true, stream, [&](hipStream_t cs) -> int {
    const int st = launch_fill(true, h->dtype, h->batch, h->es, dQ, lddq, strideQ, 0, h->m, ncols, cs);
    if (st != TQR_OK) return st;
    return enqueue_apply(h, TQR_NOTRANS, dA, ldda, strideA, dQ, ncols, lddq, strideQ, cs);
  });
}

int tqr_batch_trsm_r(int dtype, int trans, int n, int b, int batch, const void* dA, int ldda, long long strideA, void* dX,
                     int nrhs, int lddx, long long strideX, void* stream) {
  if ((dtype != TQR_F32 && dtype != TQR_F64) || !trans_ok(trans) || !valid_b(b) || n <= 0 || n % b || batch < 1 || nrhs < 1 ||
      !dA || !dX)
    return TQR_EINVAL;
  const size_t es = elem_size(dtype);
  if (!layout_ok(n, n, batch, ldda, strideA, es) || !layout_ok(n, nrhs, batch, lddx, strideX, es)) return TQR_EINVAL;
  if (batch == 1) strideA = strideX = 0;
  if (const int st = current_device_is_gfx950()) return st;
  const sbfn fn = solve_batch_kernel_of(b, dtype, trans);
  HIPCHK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_solve(b)));
  return launch_trsm(fn, n, b, batch, es, dA, ldda, strideA, dX, nrhs, lddx, strideX, (hipStream_t)stream);
}

// Both gels directions on every member: tqr_lstsq's composition (apply.hip) of the batched launches.
int tqr_batch_lstsq(tqr_batch_apply* h, int trans, const void* dA, int ldda, long long strideA, void* dB, int nrhs, int lddb,
                    long long strideB, void* dres, long long strideRes, void* stream) {
  if (!batch_apply_args_ok(h, dA, ldda, strideA, dB, nrhs, lddb, strideB) || !trans_ok(trans) || h->m < h->n ||
      (dres && h->batch > 1 && strideRes < nrhs))
    return TQR_EINVAL;
  if (h->batch == 1) strideA = strideB = strideRes = 0;
  return batch_apply_call(h, true, stream, [&](hipStream_t cs) -> int {
    int st;
    if (trans == TQR_NOTRANS) {
      // B <- Q^T B; rows 0 .. n-1 <- R^{-1} of them; the residual norms from rows n .. m-1
      if ((st = enqueue_apply(h, TQR_TRANS, dA, ldda, strideA, dB, nrhs, lddb, strideB, cs)) != TQR_OK) return st;
      if ((st = launch_trsm(h->ksn, h->n, h->b, h->batch, h->es, dA, ldda, strideA, dB, nrhs, lddb, strideB, cs)) != TQR_OK)
        return st;
      return dres ? launch_resnorm(h->dtype, h->batch, h->es, dB, lddb, strideB, h->n, h->m, nrhs, dres, strideRes, cs)
                  : (int)TQR_OK;
    }
    // x = Q [R^{-T} c; 0]
    if ((st = launch_fill(false, h->dtype, h->batch, h->es, dB, lddb, strideB, h->n, h->m - h->n, nrhs, cs)) != TQR_OK) return st;
    if ((st = launch_trsm(h->kst, h->n, h->b, h->batch, h->es, dA, ldda, strideA, dB, nrhs, lddb, strideB, cs)) != TQR_OK)
      return st;
    return enqueue_apply(h, TQR_NOTRANS, dA, ldda, strideA, dB, nrhs, lddb, strideB, cs);
  });
}

}  // extern "C"
