// Strided-batched factorisation (include/tqr.h "batched"): many same-shape matrices, each factorised
// exactly as a TQR_ENGINE_WAVES plan factorises one, in the launches of one matrix.
//
// The wave engine runs each BFS wave of the reference DAG as two launches — the panel tasks on one
// stream, the update strips on another, joined by events — and every workgroup of a launch is
// independent of the others. A batch is one more grid dimension of those launches: blockIdx.x is the
// item within the wave, blockIdx.y the matrix within the current group. The kernels below are the wave
// engine's bodies (wave_dev.hpp) behind a per-matrix offset of the three base pointers, so matrix i has
// the bytes of a wave plan executed on it alone, whatever the batch, the group size and the strides.
// Each matrix needs the wave engine's T workspace; a batch runs in groups of `group` matrices, one
// group after another on the same two streams, so the workspace is bounded by ws_limit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "batch_layout.hpp"
#include "host_common.hpp"
#include "tqr.h"
#include "wave_dev.hpp"

namespace tqr {

struct BatchArgs {
  void* A;        // matrix 0 of the group (S*)
  void* tau;      // its compact tau (S*), m x kmax
  double* Tw;     // T workspace of the group: matrix i at Tw + i * strideTw
  const Item* items;
  long ldm;
  long long strideA, strideTau;  // elements between consecutive matrices / compact taus
  long long strideTw;            // doubles between consecutive T workspaces
  int m, p;
};

// blockIdx.x: the item within the wave; blockIdx.y: the matrix within the group. The matrix's offset is
// taken in 64 bits on the base pointers; inside a matrix the wave engine's offset rules hold unchanged.
template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_panel_batch(BatchArgs a) {
  extern __shared__ __align__(16) double lds[];
  const size_t i = blockIdx.y;
  wave_panel<B, S>((S*)a.A + i * (size_t)a.strideA, (S*)a.tau + i * (size_t)a.strideTau, a.Tw + i * (size_t)a.strideTw,
                   a.items[blockIdx.x], (size_t)a.ldm, a.m, a.p, lds);
}

template <int B, typename S>
__global__ __launch_bounds__(NT, 2) void k_update_batch(BatchArgs a) {
  extern __shared__ __align__(16) double lds[];
  const size_t i = blockIdx.y;
  wave_update<B, S>((S*)a.A + i * (size_t)a.strideA, a.Tw + i * (size_t)a.strideTw, a.items[blockIdx.x], (size_t)a.ldm,
                    a.p, lds);
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
typedef void (*bfn)(BatchArgs);
template <int B>
static void batch_kernels(int dtype, bfn* kp, bfn* ku) {
  if (dtype == TQR_F64) { *kp = k_panel_batch<B, double>; *ku = k_update_batch<B, double>; }
  else { *kp = k_panel_batch<B, float>; *ku = k_update_batch<B, float>; }
}

constexpr int kMaxGroup = 65535;                    // gridDim.y
constexpr size_t kDefaultWsLimit = (size_t)1 << 30;  // ws_limit == 0

// tqr_plan_create's argument errors, and batch < 1
static bool batch_shape_ok(int m, int n, int b, int dtype, int batch) {
  return valid_b(b) && m > 0 && n > 0 && m % b == 0 && n % b == 0 && (dtype == TQR_F32 || dtype == TQR_F64) &&
         valid_ld(m, elem_size(dtype)) && batch >= 1;
}
// matrices per launch group: as many as ws_limit holds T workspaces for, at least one, at most a grid's y
static int batch_group_of(int batch, size_t per, size_t ws_limit) {
  const size_t lim = ws_limit ? ws_limit : kDefaultWsLimit;
  const size_t fit = std::max<size_t>(1, lim / per);
  return (int)std::min<size_t>({(size_t)batch, (size_t)kMaxGroup, fit});
}

}  // namespace tqr

using namespace tqr;

struct tqr_batch {
  int m, n, b, p, q, kmax, dtype, batch, group;
  size_t es, per;                  // element size; bytes of one matrix's T workspace
  std::vector<long> off_p, off_u;  // per wave offsets into the item arrays
  int nlevels = 0;
  bool ready = false;  // the device side below exists (a gfx950 was present at create)
  Item* d_items_p = nullptr;
  Item* d_items_u = nullptr;
  double* d_T = nullptr;  // group x per bytes
  hipStream_t sP = nullptr, sU = nullptr;
  hipEvent_t evP = nullptr, evU = nullptr, evStart = nullptr, evDone = nullptr;
  bfn kp = nullptr, ku = nullptr;
  size_t ldsP = 0, ldsU = 0;
  std::mutex mu;  // one enqueue sequence at a time (the executes share the workspace and the streams)
};

// The device side of a handle: item lists, the group's T workspace, the two side streams and their
// events, the kernels' LDS limits.
static int batch_device_init(tqr_batch* bt, const std::vector<Item>& ip, const std::vector<Item>& iu) {
  if (hipMalloc(&bt->d_items_p, std::max<size_t>(1, ip.size()) * sizeof(Item)) != hipSuccess ||
      hipMalloc(&bt->d_items_u, std::max<size_t>(1, iu.size()) * sizeof(Item)) != hipSuccess ||
      hipMalloc(&bt->d_T, (size_t)bt->group * bt->per) != hipSuccess) {
    (void)hipGetLastError();
    return TQR_ENOMEM;
  }
  if (!ip.empty()) HIPCHK(hipMemcpy(bt->d_items_p, ip.data(), ip.size() * sizeof(Item), hipMemcpyHostToDevice));
  if (!iu.empty()) HIPCHK(hipMemcpy(bt->d_items_u, iu.data(), iu.size() * sizeof(Item), hipMemcpyHostToDevice));
  HIPCHK(hipStreamCreateWithFlags(&bt->sP, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&bt->sU, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&bt->evP, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&bt->evU, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&bt->evStart, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&bt->evDone, hipEventDisableTiming));
  dispatch_b(bt->b, [&](auto bb) { batch_kernels<decltype(bb)::value>(bt->dtype, &bt->kp, &bt->ku); });
  bt->ldsP = lds_panel(bt->b);
  bt->ldsU = lds_update(bt->b);
  HIPCHK(hipFuncSetAttribute((const void*)bt->kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bt->ldsP));
  HIPCHK(hipFuncSetAttribute((const void*)bt->ku, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bt->ldsU));
  bt->ready = true;
  return TQR_OK;
}

// The waves of every group, enqueued on the two side streams behind evStart; mu held.
static int batch_enqueue(tqr_batch* bt, void* dA, int ldda, long long strideA, void* dtau, long long strideTau,
                         hipStream_t cs) {
  BatchArgs a;
  a.Tw = bt->d_T; a.ldm = ldda; a.strideA = strideA; a.strideTau = strideTau;
  a.strideTw = (long long)(bt->per / sizeof(double)); a.m = bt->m; a.p = bt->p;
  // both work streams start after everything already queued on the caller's stream
  HIPCHK(hipEventRecord(bt->evStart, cs));
  HIPCHK(hipStreamWaitEvent(bt->sP, bt->evStart, 0));
  HIPCHK(hipStreamWaitEvent(bt->sU, bt->evStart, 0));
  HIPCHK(hipEventRecord(bt->evP, bt->sP));
  HIPCHK(hipEventRecord(bt->evU, bt->sU));
  for (int g0 = 0; g0 < bt->batch; g0 += bt->group) {
    const unsigned nb = (unsigned)std::min(bt->group, bt->batch - g0);
    a.A = (char*)dA + (size_t)g0 * (size_t)strideA * bt->es;
    a.tau = (char*)dtau + (size_t)g0 * (size_t)strideTau * bt->es;
    for (int L = 0; L < bt->nlevels; ++L) {
      const long np = bt->off_p[L + 1] - bt->off_p[L];
      const long nu = bt->off_u[L + 1] - bt->off_u[L];
      // each stream waits for the other stream's previous wave (events hold wave L-1; for a group's
      // first wave, the last wave of the group before it, whose T workspace this group reuses)
      HIPCHK(hipStreamWaitEvent(bt->sP, bt->evU, 0));
      HIPCHK(hipStreamWaitEvent(bt->sU, bt->evP, 0));
      if (np) {
        a.items = bt->d_items_p + bt->off_p[L];
        hipLaunchKernelGGL(bt->kp, dim3((unsigned)np, nb), dim3(NT), bt->ldsP, bt->sP, a);
        HIPCHK(hipGetLastError());
      }
      if (nu) {
        a.items = bt->d_items_u + bt->off_u[L];
        hipLaunchKernelGGL(bt->ku, dim3((unsigned)nu, nb), dim3(NT), bt->ldsU, bt->sU, a);
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipEventRecord(bt->evP, bt->sP));
      HIPCHK(hipEventRecord(bt->evU, bt->sU));
    }
  }
  return TQR_OK;
}

extern "C" {

int tqr_batch_plan(int m, int n, int b, int dtype, int batch, size_t ws_limit, int* group, int* ngroups, int* nlaunch) {
  if (!batch_shape_ok(m, n, b, dtype, batch)) return TQR_EINVAL;
  const int p = m / b, q = n / b;
  std::vector<Item> ip, iu;
  std::vector<long> off_p, off_u;
  if (!wave_items(p, q, b, ip, iu, off_p, off_u)) return TQR_ENOMEM;
  int per_matrix = 0;  // non-empty panel launches + non-empty update launches of one wave plan
  for (size_t L = 0; L + 1 < off_p.size(); ++L) per_matrix += (off_p[L + 1] > off_p[L]) + (off_u[L + 1] > off_u[L]);
  const int g = batch_group_of(batch, wave_tw_bytes(p, std::min(p, q), b), ws_limit);
  const int ng = (batch + g - 1) / g;
  if ((long long)ng * per_matrix > 0x7fffffffLL) return TQR_EINVAL;
  if (group) *group = g;
  if (ngroups) *ngroups = ng;
  if (nlaunch) *nlaunch = ng * per_matrix;
  return TQR_OK;
}

int tqr_batch_create(tqr_batch** out, int m, int n, int b, int dtype, int batch, size_t ws_limit) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!batch_shape_ok(m, n, b, dtype, batch)) return TQR_EINVAL;
  tqr_batch* bt = new (std::nothrow) tqr_batch();
  if (!bt) return TQR_ENOMEM;
  bt->m = m; bt->n = n; bt->b = b; bt->p = m / b; bt->q = n / b; bt->kmax = std::min(bt->p, bt->q);
  bt->dtype = dtype; bt->es = elem_size(dtype); bt->batch = batch;
  bt->per = wave_tw_bytes(bt->p, bt->kmax, b);
  bt->group = batch_group_of(batch, bt->per, ws_limit);
  std::vector<Item> ip, iu;
  if (!wave_items(bt->p, bt->q, b, ip, iu, bt->off_p, bt->off_u)) { delete bt; return TQR_ENOMEM; }
  bt->nlevels = (int)bt->off_p.size() - 1;
  // without a gfx950 the handle exists, holds no device memory, and every execute returns TQR_ENODEV
  if (current_device_is_gfx950() == TQR_OK) {
    const int st = batch_device_init(bt, ip, iu);
    if (st != TQR_OK) { tqr_batch_destroy(bt); return st; }
  }
  *out = bt;
  return TQR_OK;
}

size_t tqr_batch_workspace_bytes(const tqr_batch* bt) { return bt ? (size_t)bt->group * bt->per : 0; }

int tqr_batch_group(const tqr_batch* bt) { return bt ? bt->group : TQR_EINVAL; }

int tqr_batch_execute(tqr_batch* bt, void* dA, int ldda, long long strideA, void* dtau, long long strideTau, void* stream) {
  if (!bt || !dA || !dtau || ldda < bt->m || !valid_ld(ldda, bt->es)) return TQR_EINVAL;
  if (strideTau < (long long)bt->m * bt->kmax) return TQR_EINVAL;
  if (!batch_stride_ok(bt->m, bt->n, bt->batch, ldda, strideA)) return TQR_EINVAL;  // batch_layout.hpp
  if (bt->batch == 1) strideA = 0;                                                  // ignored
  if (!bt->ready) return TQR_ENODEV;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(bt->mu);
  HIPCHK(hipStreamWaitEvent(cs, bt->evDone, 0));  // the previous execute of this handle (any stream)
  const int st = batch_enqueue(bt, dA, ldda, strideA, dtau, strideTau, cs);
  // join the side streams and mark this execute, also behind a partly failed enqueue: the next
  // execute stays ordered after whatever was enqueued
  const hipError_t e1 = hipStreamWaitEvent(cs, bt->evP, 0);
  const hipError_t e2 = hipStreamWaitEvent(cs, bt->evU, 0);
  const hipError_t e3 = hipEventRecord(bt->evDone, cs);
  if (st != TQR_OK) return st;
  HIPCHK(e1);
  HIPCHK(e2);
  HIPCHK(e3);
  return TQR_OK;
}

void tqr_batch_destroy(tqr_batch* bt) {
  if (!bt) return;
  if (bt->evDone) {
    (void)hipEventSynchronize(bt->evDone);  // the last execute may still be using the workspace
    (void)hipEventDestroy(bt->evDone);
  }
  if (bt->d_items_p) (void)hipFree(bt->d_items_p);
  if (bt->d_items_u) (void)hipFree(bt->d_items_u);
  if (bt->d_T) (void)hipFree(bt->d_T);
  if (bt->sP) (void)hipStreamDestroy(bt->sP);
  if (bt->sU) (void)hipStreamDestroy(bt->sU);
  if (bt->evP) (void)hipEventDestroy(bt->evP);
  if (bt->evU) (void)hipEventDestroy(bt->evU);
  if (bt->evStart) (void)hipEventDestroy(bt->evStart);
  delete bt;
}

}  // extern "C"
