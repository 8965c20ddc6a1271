// MI355X tiled-QR engine: the device side of libtqr.so and the code that launches it.
//
// Two engines compute the same factorisation (DESIGN.md "Engine"). The default is the persistent
// dataflow engine: one launch of k_flow (flow.hpp) whose workgroups pull panel tasks and chain
// segments from a static list; the list, its order and the deadlock-freedom check are the host
// planner's (flowplan.hpp / flowplan.cpp, built without HIP). TQR_ENGINE=waves selects the
// wave-batched engine: the host scheduler (sched.c) turns the reference DAG (src/gridscheduler.c)
// into BFS waves, two launches per wave on two HIP streams joined by events.
// This file holds what is tied to the device templates, and it is the only unit the diagnostic
// targets (make stamps / flowstamps / diag / variant) rebuild with their -D flags:
//   * the wave engine's kernels (k_panel: one 256-thread workgroup per GEQRT / TSQRT task; k_update:
//     one per 64-column strip of every UNMQR / TSMQR task of the wave; their bodies are wave_dev.hpp's,
//     shared with the batched factorisation of batch.hip), k_build_t, k_randzo;
//   * every k_flow instantiation and its LDS size; resolve / resolve_flow hand the kernels to the
//     other units (plan.hpp), so none is instantiated twice;
//   * the launch code: plan_execute of both engines, the wait limit, tqr_plan_execute, tqr_fill_randzo*;
//   * the diagnostic builds' device symbols and their tqr_debug_* readers.
// The rest of a plan's life is host code in units of its own (plan.hpp lists them): plans.hip
// (creation, destruction, introspection), dist.hip (multi-GPU setup), hostpath.hip (plan cache,
// host-pointer path), tileapi.hip (single-tile and tile-batch API).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "gridscheduler.h"
#include "plan.hpp"
#include "tiles.hpp"
#include "tqr.h"

namespace tqr {

#ifdef TQR_STAMPS
// Diagnostic build only (make stamps): per-phase cycle sums of the panel kernel's TSQRT tasks.
__device__ unsigned long long g_stamps[8];
__device__ unsigned long long g_pstamps[8];
#define STAMP_INIT unsigned long long st_last = __builtin_amdgcn_s_memrealtime();
#define STAMP(i)                                                          \
  do {                                                                    \
    if (threadIdx.x == 0) {                                               \
      unsigned long long now_ = __builtin_amdgcn_s_memrealtime();             \
      atomicAdd(&g_stamps[i], now_ - st_last);                            \
      st_last = now_;                                                     \
    }                                                                     \
  } while (0)
#else
#define STAMP_INIT
#define STAMP(i) do {} while (0)
#endif

#ifdef TQR_FLOW_STAMPS
__device__ unsigned long long g_fst[4096 * 24];  // >= FST_N categories per workgroup
__device__ unsigned long long g_ttl[3 << 18];     // task timeline (first 2^18 tasks)
__device__ unsigned long long g_wst[4096 * 64];   // per-wave activity sums (flow.hpp WSL slots x 8 waves)
__device__ unsigned long long g_gtr[4096 * 8 * 8];  // group trace of workgroup 0 (flow.hpp GTR)
__device__ unsigned long long g_xtr[4096 * 8 * 8];  // its hand-over phase-2 marks (flow.hpp XPipe)
#endif
}  // namespace tqr
#include "flow.hpp"
#include "wave_dev.hpp"  // (after STAMP / STAMP_INIT above: the stamps build times the panel body)
namespace tqr {
static_assert(FST_N <= 24, "g_fst holds 24 categories per workgroup");
static_assert(Geo<256>::TPIMG == 1024 && Geo<16>::TPIMG == 256 && Geo<256, 16>::TPIMG == 256 &&
                  Geo<256, 16>::VIMG == 4608 && Geo<64, 16>::VIMG == 1152,
              "host tpimg_doubles / vimg_doubles mirror Geo::TPIMG / VIMG");
static_assert(Img<256, float>::V == 4096 && Img<256, float>::T == 384 && Img<16, float>::V == 128 && Img<16, float>::T == 128 &&
                  Img<64, float>::V == 1024 && Img<64, float>::T == 384,
              "host wk_bytes mirrors Img<B, float>");
static_assert(Geo<256>::TPK <= Geo<256>::TSZ && Geo<16>::TPK <= Geo<16>::TSZ, "packed T fits the Gram buffer");

template <int B>
__device__ __forceinline__ double* tw_ptr(const Args& a, int i, int k, int g) {
  return wave_tw<B>(a.Tw, a.p, i, k, g);
}

// ---------------------------------------------------------------------------------------
// The wave engine's kernels: thin wrappers around the bodies of wave_dev.hpp (which the batched
// factorisation, batch.hip, launches over many matrices). Panel kernel: GEQRT (QRS) and TSQRT (QRD)
// tasks, one workgroup each. Update kernel: UNMQR (SAPP) and TSMQR (DAPP) on one 64-column strip.
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_panel(Args a) {
  extern __shared__ __align__(16) double lds[];
  wave_panel<B, S>((S*)a.A, (S*)a.tau, a.Tw, a.items[blockIdx.x], (size_t)a.ldm, a.m, a.p, lds);
}

template <int B, typename S>
__global__ __launch_bounds__(NT, 2) void k_update(Args a) {
  extern __shared__ __align__(16) double lds[];
  wave_update<B, S>((S*)a.A, a.Tw, a.items[blockIdx.x], (size_t)a.ldm, a.p, lds);
}

// T factors from a stored V and tau (for the single-tile API, where the caller hands over V
// and tau as the reference's SLARFT/SSSRFT take them). One workgroup per (item, group).
template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_build_t(Args a) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  extern __shared__ __align__(16) double lds[];
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;
  double* Gs = Ts + G::TSZ;
  double* tauv = Gs + G::TSZ;
  double* Gp = tauv + IB + 2;
  const Item it = a.items[blockIdx.x / NG];
  const int g = blockIdx.x % NG, c0 = g * IB, type = it.ts & 0xff, l = it.l, k = it.k;
  const S* A = (const S*)a.A;
  const S* tau = (const S*)a.tau;
  const size_t ldm = a.ldm;
  const int row0 = type == QRS ? k * B : l * B;
  if (type == QRS) stage_v_ge<B>(Vs, A + (size_t)k * B * ldm + (size_t)k * B, ldm, c0);
  else stage_v_ts<B>(Vs, A + (size_t)k * B * ldm + (size_t)l * B, ldm, c0);
  if (threadIdx.x < IB) tauv[threadIdx.x] = ld(tau + (size_t)k * a.m + row0 + c0 + threadIdx.x);
  __syncthreads();
  build_t<B>(Vs, tauv, Gs, Ts, Gp, type == QRS ? c0 / 4 : 0);
  double* tg = tw_ptr<B>(a, type == QRS ? k : l, k, g);
  for (int idx = threadIdx.x; idx < G::TSZ; idx += NT) tg[idx] = Ts[idx];
}

// RANDZO-distributed synthetic input: ((h mod 201) - 100) / 100 from a splitmix64 hash.
// col0: the first column's index in the global matrix (the value of element (i, j) depends only on
// the seed and its global position, so a rank can fill just its own columns)
template <typename S>
__global__ void k_randzo(S* A, int m, int n, long ldm, unsigned long long seed, long col0) {
  long total = (long)m * n;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long jj = e / m, ii = e % m;
    const unsigned long long eg = (unsigned long long)(e + col0 * m);  // global element index
    unsigned long long z = seed * 0x9E3779B97F4A7C15ull + eg + 0x632BE59BD9B4E019ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    A[jj * ldm + ii] = (S)(((double)(long)(z % 201ull) - 100.0) / 100.0);
  }
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
// (lds_panel, lds_update, wave_tw_bytes, wave_items: wave_dev.hpp; kfn, ffn: plan.hpp)

template <int B, typename S>
static void get_kernels(kfn* p, kfn* u, kfn* t) {
  *p = k_panel<B, S>;
  *u = k_update<B, S>;
  *t = k_build_t<B, S>;
}
// the persistent kernel of an engine shape (flowplan.hpp flow_shape: 8 ShapeW8, 4 ShapeW4, 5 ShapeR)
template <int B, typename S, class C>
static ffn get_flow() { return k_flow<B, S, C>; }
template <int B>
static ffn get_flow_res() {
  if constexpr (B == 256) return k_flow<256, double, ShapeR>;
  else return nullptr;
}
template <int B>
static int lds_res() {
  if constexpr (B == 256) return flow_lds_doubles<256, double, ShapeR>();
  else return 0;
}
size_t lds_flow(int b, int dtype, int shape) {
  int d = 0;
#define TQR_L(BB)                                                                                  \
  case BB:                                                                                         \
    d = dtype != TQR_F64 ? flow_lds_doubles<BB, float, ShapeW8>()                                  \
        : shape == 4     ? flow_lds_doubles<BB, double, ShapeW4>()                                 \
        : shape == 5     ? lds_res<BB>()                                                           \
                         : flow_lds_doubles<BB, double, ShapeW8>();                                \
    break;
  switch (b) { TQR_L(16) TQR_L(32) TQR_L(64) TQR_L(128) TQR_L(256) }
#undef TQR_L
  return (size_t)d * sizeof(double) + 1536;  // + task index, sync-point verdicts, Rc view, FST sums, wave sums
}
ffn resolve_flow(int b, int dtype, int shape) {
  ffn f = nullptr;
#define TQR_F(BB)                                                                                  \
  case BB:                                                                                         \
    f = dtype != TQR_F64 ? get_flow<BB, float, ShapeW8>()                                          \
        : shape == 4     ? get_flow<BB, double, ShapeW4>()                                         \
        : shape == 5     ? get_flow_res<BB>()                                                      \
                         : get_flow<BB, double, ShapeW8>();                                        \
    break;
  switch (b) { TQR_F(16) TQR_F(32) TQR_F(64) TQR_F(128) TQR_F(256) }
#undef TQR_F
  if (f && hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_flow(b, dtype, shape)) !=
               hipSuccess)
    return nullptr;
  return f;
}

size_t lds_build_t(int b) {
  int ib = b < 32 ? b : 32;
  return ((size_t)b * (ib + 2) + 6 * (size_t)ib * (ib + 1) + ib + 2) * sizeof(double);
}
// Resolve the kernels of one (b, dtype) and raise their dynamic-LDS limits.
int resolve(int b, int dtype, kfn* kp, kfn* ku, kfn* kt) {
#define TQR_K(BB)                                                   \
  case BB:                                                          \
    if (dtype == TQR_F64) get_kernels<BB, double>(kp, ku, kt);      \
    else get_kernels<BB, float>(kp, ku, kt);                        \
    break;
  switch (b) { TQR_K(16) TQR_K(32) TQR_K(64) TQR_K(128) TQR_K(256) default: return TQR_EINVAL; }
#undef TQR_K
  if (hipFuncSetAttribute((const void*)*kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_panel(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)*ku, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_update(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)*kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_build_t(b)) != hipSuccess)
    return TQR_EHIP;
  return TQR_OK;
}

// The engine's wait limit (flow.hpp g_flow_wait_limit, read only after a wait's first 5 s): 5 s for
// one-GPU plans, TQR_PEER_TIMEOUT_S (default 60, at least 5) for multi-GPU plans, whose peers'
// launches may start seconds apart. It is a per-device symbol, so every launch sets its plan's
// value on its own stream when the device holds another one (a per-device cache skips the copy
// otherwise): a one-GPU launch after a multi-GPU plan reports a real stall after 5 s again, and a
// multi-GPU plan on any device gets its limit there. (Round 5 raised it once per process, on the
// current device only.) Launches of plans with different limits running at once on one device
// share whichever value was set last — only how long a real stall takes to be reported differs.
static unsigned long long plan_wait_limit(int world) {
  if (world <= 1) return FLOW_TIMEOUT;
  double sec = 60.0;
  if (const char* e = getenv("TQR_PEER_TIMEOUT_S")) sec = std::max(5.0, atof(e));
  return (unsigned long long)(sec * 1e8);  // s_memrealtime: 100 MHz
}
static int set_wait_limit(unsigned long long ticks, hipStream_t cs) {
  constexpr int kDev = 64;
  static std::mutex mu;
  static unsigned long long cur[kDev] = {};  // per device: the value last set (0: unknown); also the
                                             // copy's source, alive after the async copy returns
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kDev) {
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_flow_wait_limit), &ticks, sizeof(ticks)));
    return TQR_OK;
  }
  std::lock_guard<std::mutex> lk(mu);
  if (cur[dev] == ticks) return TQR_OK;
  cur[dev] = ticks;
  if (hipMemcpyToSymbolAsync(HIP_SYMBOL(g_flow_wait_limit), &cur[dev], sizeof(ticks), 0, hipMemcpyHostToDevice, cs) !=
      hipSuccess) {
    cur[dev] = 0;
    return TQR_EHIP;
  }
  return TQR_OK;
}
static int plan_execute(tqr_plan* pl, void* dA, int ldda, void* dtau, hipStream_t cs, const XferArgs* xa = nullptr);
// Serialised enqueue of one execute (see tqr.h): the stream first waits for the plan's previous
// execute; evDone marks this one. If enqueuing fails part-way, evDone is still recorded behind
// whatever was enqueued (the wave engine's side streams are joined first), so the next execute
// stays ordered after it.
int plan_execute_serial(tqr_plan* pl, void* dA, int ldda, void* dtau, hipStream_t cs, const XferArgs* xa) {
  std::lock_guard<std::mutex> lk(pl->mu);
  HIPCHK(hipStreamWaitEvent(cs, pl->evDone, 0));  // the previous execute of this plan (any stream)
  int st = plan_execute(pl, dA, ldda, dtau, cs, xa);
  if (st != TQR_OK && pl->engine != TQR_ENGINE_FLOW) {
    (void)hipStreamWaitEvent(cs, pl->evP, 0);
    (void)hipStreamWaitEvent(cs, pl->evU, 0);
  }
  const hipError_t e = hipEventRecord(pl->evDone, cs);
  if (st == TQR_OK && e != hipSuccess) HIPCHK(e);
  return st;
}
static int plan_execute(tqr_plan* pl, void* dA, int ldda, void* dtau, hipStream_t cs, const XferArgs* xa) {
  if (pl->engine == 1) {
    if (!pl->kflow || !pl->d_flow || !pl->d_sync || (xa && !pl->d_flow_x)) return TQR_EINVAL;
    FlowArgs f;
    f.A = dA; f.tau = dtau; f.Wk = pl->d_wk; f.ldm = ldda;
    f.tasks = xa ? pl->d_flow_x : pl->d_flow;
    f.ntasks = xa ? pl->nflow_x : pl->nflow;
    f.m = pl->m; f.p = pl->p; f.q = pl->q; f.kmax = pl->kmax; f.ns = pl->ns;
    f.next = pl->d_sync; f.err = pl->d_sync + 1; f.exitc = pl->d_sync + 3; f.Rc = pl->d_sync + 4;
    f.Tc = f.Rc + (size_t)pl->kmax * pl->ng;
    f.Ac = f.Tc + (size_t)pl->p * pl->q * pl->ns;
    f.Rt = f.Ac + (size_t)pl->kmax * pl->q * pl->ns * pl->ng;
    f.Rr = f.Rt + (size_t)pl->kmax * pl->ng;
    f.dist = pl->world > 1; f.rank = pl->rank; f.world = pl->world; f.cyclic = pl->cyclic; f.peers = pl->d_peers; f.Rf = pl->d_rf;
    f.cdiv = pl->world;  // multi-GPU: the rank's own tile columns only, packed (FlowArgs::cdiv)
    f.rf_done = (long)pl->kmax * pl->p * pl->ng;
    // the launch's epoch: committed to the plan only once the launch is enqueued (a failed
    // enqueue must not leave this rank one epoch ahead of its peers for good)
    f.epoch = pl->world > 1 ? pl->epoch + 1 : 0;
    f.chain_asm = pl->chain_asm;
    f.seglen = pl->knobs.seglen; f.seglen_la = pl->knobs.seglen_la; f.la_tail = pl->knobs.la_tail;
    f.tail = pl->knobs.tail; f.tail_sl = pl->knobs.tail_sl; f.ualone = pl->knobs.ualone;
    if (xa) {
      f.hsrc = xa->hsrc; f.hdst = xa->hdst; f.hld = xa->hld; f.hup = xa->hup; f.hdn = xa->hdn; f.gen = xa->gen;
      f.Uc = f.Rr + (size_t)pl->kmax * pl->ng;
      f.nxc = pl->nxc; f.xrows = pl->xrows;
    } else {
      f.hsrc = nullptr; f.hdst = nullptr; f.hld = 0; f.hup = nullptr; f.hdn = nullptr; f.gen = 0;
      f.Uc = nullptr; f.nxc = 0; f.xrows = 0;
    }
    // local progress counters (multi-GPU: the member flags are epoch-valued and never reset)
    HIPCHK(hipMemsetAsync(pl->d_sync, 0, sizeof(int) * pl->sync_ints, cs));
    if (const int st = set_wait_limit(plan_wait_limit(pl->world), cs)) return st;
    if (pl->profile) HIPCHK(hipEventRecord(pl->ev0, cs));
    hipLaunchKernelGGL(pl->kflow, dim3(pl->grid), dim3(pl->nt), pl->ldsF, cs, f);
    HIPCHK(hipGetLastError());
    if (pl->world > 1) pl->epoch = f.epoch;
    if (pl->profile) {
      HIPCHK(hipEventRecord(pl->ev1, cs));
      HIPCHK(hipEventSynchronize(pl->ev1));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, pl->ev0, pl->ev1));
      pl->nl_u = 1; pl->ms_u = ms; pl->nl_p = 0; pl->ms_p = 0;
    }
    return TQR_OK;
  }
  Args a;
  a.A = dA; a.tau = dtau; a.Tw = pl->d_T; a.ldm = ldda; a.m = pl->m; a.p = pl->p; a.kmax = pl->kmax;
  // both work streams start after everything already queued on the caller's stream
  HIPCHK(hipEventRecord(pl->evStart, cs));
  HIPCHK(hipStreamWaitEvent(pl->sP, pl->evStart, 0));
  HIPCHK(hipStreamWaitEvent(pl->sU, pl->evStart, 0));
  HIPCHK(hipEventRecord(pl->evP, pl->sP));
  HIPCHK(hipEventRecord(pl->evU, pl->sU));
  size_t nev = 0;
  if (pl->profile) {
    size_t need = 2 * (size_t)pl->nlevels * 2;
    while (pl->prof_ev.size() < need) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      pl->prof_ev.push_back(e);
    }
    pl->prof_kind.assign(need / 2, -1);
  }
  for (int L = 0; L < pl->nlevels; ++L) {
    long np = pl->off_p[L + 1] - pl->off_p[L];
    long nu = pl->off_u[L + 1] - pl->off_u[L];
    // each stream waits for the other stream's previous wave (events hold wave L-1)
    HIPCHK(hipStreamWaitEvent(pl->sP, pl->evU, 0));
    HIPCHK(hipStreamWaitEvent(pl->sU, pl->evP, 0));
    if (np) {
      a.items = pl->d_items_p + pl->off_p[L];
      if (pl->profile) { pl->prof_kind[nev / 2] = 1; HIPCHK(hipEventRecord(pl->prof_ev[nev++], pl->sP)); }
      hipLaunchKernelGGL(pl->kp, dim3((unsigned)np), dim3(NT), pl->ldsP, pl->sP, a);
      HIPCHK(hipGetLastError());
      if (pl->profile) HIPCHK(hipEventRecord(pl->prof_ev[nev++], pl->sP));
    }
    if (nu) {
      a.items = pl->d_items_u + pl->off_u[L];
      if (pl->profile) { pl->prof_kind[nev / 2] = 0; HIPCHK(hipEventRecord(pl->prof_ev[nev++], pl->sU)); }
      hipLaunchKernelGGL(pl->ku, dim3((unsigned)nu), dim3(NT), pl->ldsU, pl->sU, a);
      HIPCHK(hipGetLastError());
      if (pl->profile) HIPCHK(hipEventRecord(pl->prof_ev[nev++], pl->sU));
    }
    HIPCHK(hipEventRecord(pl->evP, pl->sP));
    HIPCHK(hipEventRecord(pl->evU, pl->sU));
  }
  HIPCHK(hipStreamWaitEvent(cs, pl->evP, 0));
  HIPCHK(hipStreamWaitEvent(cs, pl->evU, 0));
  if (pl->profile) {
    HIPCHK(hipStreamSynchronize(cs));
    pl->nl_u = pl->nl_p = 0;
    pl->ms_u = pl->ms_p = 0;
    for (size_t x = 0; x + 1 < nev; x += 2) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, pl->prof_ev[x], pl->prof_ev[x + 1]));
      if (pl->prof_kind[x / 2] == 1) { pl->nl_p++; pl->ms_p += ms; }
      else { pl->nl_u++; pl->ms_u += ms; }
    }
  }
  return TQR_OK;
}

}  // namespace tqr

using namespace tqr;

extern "C" {

int tqr_plan_execute(tqr_plan* pl, void* dA, int ldda, void* dtau, void* stream) {
  if (!pl || !dA || !dtau || ldda < pl->m || !valid_ld(ldda, pl->es)) return TQR_EINVAL;
  // a multi-GPU plan whose peers were never imported would dereference unset peer pointers
  if (pl->world > 1 && !pl->imported) return TQR_EINVAL;
  return plan_execute_serial(pl, dA, ldda, dtau, (hipStream_t)stream, nullptr);
}

int tqr_fill_randzo_cols(int dtype, void* dA, int m, int ncols, int ldda, unsigned long long seed, long col0, void* stream) {
  if (!dA || ldda < m || m <= 0 || ncols <= 0 || col0 < 0) return TQR_EINVAL;
  long total = (long)m * ncols;
  int blocks = (int)std::min<long>(65536, (total + 255) / 256);
  if (dtype == TQR_F64)
    hipLaunchKernelGGL(k_randzo<double>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (double*)dA, m, ncols, (long)ldda, seed, col0);
  else
    hipLaunchKernelGGL(k_randzo<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float*)dA, m, ncols, (long)ldda, seed, col0);
  HIPCHK(hipGetLastError());
  return TQR_OK;
}
int tqr_fill_randzo(int dtype, void* dA, int m, int n, int ldda, unsigned long long seed, void* stream) {
  return tqr_fill_randzo_cols(dtype, dA, m, n, ldda, seed, 0, stream);
}

}  // extern "C"

#ifdef TQR_STAMPS
extern "C" int tqr_debug_stamps(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8) != hipSuccess) return TQR_EHIP;
  if (hipMemcpyFromSymbol(out + 8, HIP_SYMBOL(g_pstamps), sizeof(unsigned long long) * 8) != hipSuccess) return TQR_EHIP;
  if (reset) {
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z) != hipSuccess) return TQR_EHIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_pstamps), z, sizeof z) != hipSuccess) return TQR_EHIP;
  }
  return TQR_OK;
}
#endif

#ifdef TQR_FLOW_STAMPS
extern "C" int tqr_debug_flow_stamp_count(void) { return FST_N; }
// per-workgroup activity sums of the last k_flow launch (FST_N categories, flow.hpp FST)
extern "C" int tqr_debug_flow_stamps(unsigned long long* out, int nblocks) {
  if (nblocks > 4096) return TQR_EINVAL;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fst), sizeof(unsigned long long) * FST_N * nblocks) != hipSuccess) return TQR_EHIP;
  return TQR_OK;
}
// per-wave activity sums of the last k_flow launch: [workgroup][wave][WSL slots, flow.hpp]
extern "C" int tqr_debug_flow_wave_stamps(unsigned long long* out, int nblocks) {
  if (nblocks > 4096) return TQR_EINVAL;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wst), sizeof(unsigned long long) * 8 * WSL * nblocks) != hipSuccess) return TQR_EHIP;
  return TQR_OK;
}
// group trace of workgroup 0 in the last k_flow launch: [group][wave][mark] s_memrealtime (flow.hpp GTR),
// then the hand-over phase-2 marks [group][wave][8] (XPipe); `out` holds 2 x 64 x ngroups values
extern "C" int tqr_debug_group_trace(unsigned long long* out, int ngroups) {
  if (ngroups > GTR_GROUPS) return TQR_EINVAL;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gtr), sizeof(unsigned long long) * 64 * ngroups) != hipSuccess) return TQR_EHIP;
  if (hipMemcpyFromSymbol(out + 64 * (size_t)ngroups, HIP_SYMBOL(g_xtr), sizeof(unsigned long long) * 64 * ngroups) != hipSuccess)
    return TQR_EHIP;
  return TQR_OK;
}
// task timeline of the last k_flow launch: (start, end, workgroup) per task index, and the task list
extern "C" int tqr_debug_task_timeline(const tqr_plan* plan, unsigned long long* out, int ntasks, int* items) {
  if (ntasks > (1 << 18)) return TQR_EINVAL;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ttl), sizeof(unsigned long long) * 3 * ntasks) != hipSuccess) return TQR_EHIP;
  if (items && plan->d_flow && hipMemcpy(items, plan->d_flow, sizeof(Item) * ntasks, hipMemcpyDeviceToHost) != hipSuccess)
    return TQR_EHIP;
  return TQR_OK;
}
#endif
