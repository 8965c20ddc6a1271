// The one-shot helpers: the plan cache (cached_plan, tqr_cache_clear), the device-pointer one-shot
// calls on it (tqr_dgeqrt_tiled / tqr_sgeqrt_tiled), and the host-pointer path (tqr_*geqrt_host*) —
// host threads, staging buffers and flag polling around one execute of the cached plan
// (plan_execute_serial, engine.hip). Host code only: no kernel, no device header.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <tuple>
#include <vector>

#include "plan.hpp"
#include "tqr.h"

using namespace tqr;

// ---- plan cache for the one-shot helpers -------------------------------------------------
static std::mutex g_cache_mu;
static std::map<std::tuple<int, int, int, int, int, int>, tqr_plan*> g_cache;

namespace tqr {
// (PlanRef: plan.hpp)
int cached_plan(int m, int n, int b, int dtype, PlanRef& ref, int engine) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return TQR_ENODEV;
  std::lock_guard<std::mutex> lk(g_cache_mu);
  auto key = std::make_tuple(dev, m, n, b, dtype, engine);
  auto itc = g_cache.find(key);
  tqr_plan* pl = nullptr;
  if (itc != g_cache.end()) {
    pl = itc->second;
  } else {
    int st = tqr_plan_create_engine(&pl, m, n, b, dtype, engine);
    if (st) return st;
    g_cache[key] = pl;
  }
  pl->users.fetch_add(1);
  ref.pl = pl;
  return TQR_OK;
}
}  // namespace tqr

extern "C" {

// Argument errors are refused here, before the cache is touched: a call that tqr_plan_execute would
// refuse anyway must not first build (and keep) a plan, nor need a device to be told so.
static int geqrt_tiled(int m, int n, int b, int dtype, void* dA, int ldda, void* dtau, void* stream) {
  if (!dA || !dtau || !valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || ldda < m ||
      !valid_ld(ldda, elem_size(dtype)))
    return TQR_EINVAL;
  PlanRef r;
  int st = cached_plan(m, n, b, dtype, r);
  return st ? st : tqr_plan_execute(r.pl, dA, ldda, dtau, stream);
}
int tqr_dgeqrt_tiled(int m, int n, int b, double* dA, int ldda, double* dtau, void* stream) {
  return geqrt_tiled(m, n, b, TQR_F64, dA, ldda, dtau, stream);
}
int tqr_sgeqrt_tiled(int m, int n, int b, float* dA, int ldda, float* dtau, void* stream) {
  return geqrt_tiled(m, n, b, TQR_F32, dA, ldda, dtau, stream);
}

// Host-pointer factorisation (the reference's calling convention: cudaQRTask copies a host matrix
// in and out, gpucalc.cu:1614-1619, 1665-1670 — one cudaMemcpy per column, before and after the
// kernel). The flow engine moves the matrix INSIDE its persistent launch (xfer.hpp): UP tasks
// read tile columns from host memory ahead of the step-0 tasks that need them, DOWN tasks write
// each tile column back as soon as it is final, so PCIe traffic overlaps the factorisation.
// Host memory, one of:
//   * staging (default): a pinned, fine-grained buffer shared by all host-API calls of the device;
//     host threads copy the caller's columns into it tile column by tile column (flag hup[j] per
//     column, polled by the UP tasks) and copy finished chunks back out as the DOWN tasks flag them
//     (hdn[j][c]) — while the kernel runs;
//   * registered (TQR_HOST_XFER=register): the caller's array itself is page-locked for the call
//     (hipHostRegister) and read / written by the launch directly; no host copies.
// The wave engine (cudaQRFull) keeps pre/post copies through two pinned buffers of the plan.
// The device matrix and compact tau stay with the cached plan; tqr_cache_clear releases them.

// host threads for host-side copies (the GPU box exports OMP_NUM_THREADS = this job's CPU share;
// hardware_concurrency() there is the whole machine)
static int host_threads() {
  const char* e = getenv("OMP_NUM_THREADS");
  int n = e ? atoi(e) : 0;
  if (n <= 0) n = (int)std::max(1u, std::thread::hardware_concurrency());
  return std::min(n, 32);
}

// Run jobs on their own threads; a job whose thread cannot be created runs on the caller, after
// the others were started (jobs are ordered so that no job waits for a later one).
static void run_jobs(std::vector<std::function<void()>>& jobs) {
  std::vector<std::thread> th;
  size_t created = 0;
  try {
    for (; created + 1 < jobs.size(); ++created) th.emplace_back(jobs[created]);
  } catch (...) {
  }
  for (size_t x = created; x < jobs.size(); ++x) jobs[x]();
  for (auto& t : th) t.join();
}

// wave engine: device buffers + two pinned staging buffers. Everything is allocated into locals and
// committed to the plan only when all of it succeeded (a failed call leaves the plan untouched).
static constexpr size_t kPinBytes = 64ull << 20;
static int plan_host_buffers(tqr_plan* pl, size_t es) {
  if (pl->hA) return TQR_OK;
  const size_t abytes = es * (size_t)pl->m * pl->n, tbytes = es * (size_t)pl->m * pl->kmax;
  void *hA = nullptr, *hT = nullptr;
  if (hipMalloc(&hA, abytes) != hipSuccess || hipMalloc(&hT, tbytes) != hipSuccess) {
    if (hA) (void)hipFree(hA);
    return TQR_ENOMEM;
  }
  pl->hA = hA;
  pl->hT = hT;
  return TQR_OK;
}
static int plan_pinned_staging(tqr_plan* pl, size_t es) {
  if (pl->pin[0]) return TQR_OK;
  const size_t bytes = std::min(kPinBytes, std::max(es * (size_t)pl->m * pl->n, es * (size_t)pl->m * pl->kmax));
  void* pin[2] = {nullptr, nullptr};
  hipEvent_t pev[2] = {nullptr, nullptr};
  hipStream_t sC = nullptr;
  int st = TQR_OK;
  for (int x = 0; x < 2 && st == TQR_OK; ++x) {
    if (hipHostMalloc(&pin[x], bytes, hipHostMallocDefault) != hipSuccess) st = TQR_ENOMEM;
    else if (hipEventCreateWithFlags(&pev[x], hipEventDisableTiming) != hipSuccess) st = TQR_EHIP;
  }
  if (st == TQR_OK && hipStreamCreateWithFlags(&sC, hipStreamNonBlocking) != hipSuccess) st = TQR_EHIP;
  if (st != TQR_OK) {
    for (int x = 0; x < 2; ++x) {
      if (pin[x]) (void)hipHostFree(pin[x]);
      if (pev[x]) (void)hipEventDestroy(pev[x]);
    }
    return st;
  }
  for (int x = 0; x < 2; ++x) {
    pl->pin[x] = pin[x];
    pl->pev[x] = pev[x];
  }
  pl->pin_bytes = bytes;
  pl->sC = sC;
  return TQR_OK;
}

// copy `ncols` columns of `rows` elements between strided host memory (ld) and packed device memory
// through the plan's pinned buffers, double-buffered (wave engine)
static int staged_copy(tqr_plan* pl, char* host, size_t ld, char* dev, size_t rows, size_t ncols, size_t es, bool h2d) {
  const size_t col = es * rows, per = std::max<size_t>(1, pl->pin_bytes / col);
  const size_t nchunk = (ncols + per - 1) / per;
  const int nthr = std::min(8, host_threads());
  auto chunk = [&](size_t c, size_t& c0, size_t& nc) { c0 = c * per; nc = std::min(per, ncols - c0); };
  auto par_columns = [&](size_t nc, const std::function<void(size_t)>& f) {
    const size_t nt = std::min<size_t>(nc, (size_t)nthr);
    std::vector<std::function<void()>> jobs;
    for (size_t t = 0; t < nt; ++t)
      jobs.push_back([&, t] {
        for (size_t j = t; j < nc; j += nt) f(j);
      });
    run_jobs(jobs);
  };
  if (h2d) {
    for (size_t c = 0; c < nchunk; ++c) {
      size_t c0, nc;
      chunk(c, c0, nc);
      char* pb = (char*)pl->pin[c & 1];
      HIPCHK(hipEventSynchronize(pl->pev[c & 1]));  // the DMA from this buffer two chunks ago is done
      par_columns(nc, [&](size_t j) { memcpy(pb + j * col, host + (c0 + j) * ld * es, col); });
      HIPCHK(hipMemcpyAsync(dev + c0 * col, pb, nc * col, hipMemcpyHostToDevice, pl->sC));
      HIPCHK(hipEventRecord(pl->pev[c & 1], pl->sC));
    }
    return TQR_OK;
  }
  auto issue = [&](size_t c) -> int {
    size_t c0, nc;
    chunk(c, c0, nc);
    HIPCHK(hipMemcpyAsync(pl->pin[c & 1], dev + c0 * col, nc * col, hipMemcpyDeviceToHost, pl->sC));
    HIPCHK(hipEventRecord(pl->pev[c & 1], pl->sC));
    return TQR_OK;
  };
  for (size_t c = 0; c < std::min<size_t>(2, nchunk); ++c)
    if (int st = issue(c)) return st;
  for (size_t c = 0; c < nchunk; ++c) {
    size_t c0, nc;
    chunk(c, c0, nc);
    HIPCHK(hipEventSynchronize(pl->pev[c & 1]));
    const char* pb = (const char*)pl->pin[c & 1];
    par_columns(nc, [&](size_t j) { memcpy(host + (c0 + j) * ld * es, pb + j * col, col); });
    if (c + 2 < nchunk)
      if (int st = issue(c + 2)) return st;
  }
  return TQR_OK;
}

// The pinned, fine-grained staging buffer and flag words of the flow engine's host path, one per
// device, shared by all plans (grown on demand; tqr_cache_clear frees it). `mu` serialises the
// host-API calls that use it.
struct HostStage {
  std::mutex mu;
  char* buf = nullptr;
  size_t bytes = 0;
  int* flags = nullptr;  // host view: hup[q] then hdn[q * nxc]
  int* dflags = nullptr;  // device view
  size_t nflags = 0;
  int gen = 0;
  void release() {
    if (buf) (void)hipHostFree(buf);
    if (flags) (void)hipHostFree(flags);
    buf = nullptr; flags = nullptr; dflags = nullptr; bytes = 0; nflags = 0;
  }
  int ensure(size_t need, size_t nf) {
    if (bytes < need) {
      if (buf) (void)hipHostFree(buf);
      buf = nullptr; bytes = 0;
      void* p = nullptr;
      if (hipHostMalloc(&p, need, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) return TQR_ENOMEM;
      buf = (char*)p;
      bytes = need;
    }
    if (nflags < nf) {
      if (flags) (void)hipHostFree(flags);
      flags = nullptr; dflags = nullptr; nflags = 0;
      void* p = nullptr;
      if (hipHostMalloc(&p, nf * sizeof(int), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) return TQR_ENOMEM;
      memset(p, 0, nf * sizeof(int));
      flags = (int*)p;
      nflags = nf;
      gen = 0;
      void* d = nullptr;
      if (hipHostGetDevicePointer(&d, flags, 0) != hipSuccess) { release(); return TQR_EHIP; }
      dflags = (int*)d;
    }
    return TQR_OK;
  }
};
static std::map<int, HostStage*> g_stage;  // guarded by g_cache_mu

static int plan_xfer_list(tqr_plan* pl) {
  if (pl->d_flow_x) return TQR_OK;
  // chunk rows: one UP / DOWN task moves ~8 MiB (16-B vectors, 4 columns x 4 vectors per lane in
  // flight), a multiple of 4 rows so 16-B vectors stay whole (fp32), and
  // at most 255 chunks per column (the task word's chunk field)
  int xrows = std::max(4, (int)((8u << 20) / (pl->es * (size_t)pl->b)) & ~3);
  xrows = std::min(pl->m, std::max(xrows, ((pl->m + 254) / 255 + 3) & ~3));
  XferPlan xp;
  xp.nxc = (pl->m + xrows - 1) / xrows;
  // estimator unit = one chain element (4 b^2 SW flop at ~1/256 of the chip, SW the shape's strip
  // width); a tile column over PCIe at TQR_XFER_GBS (default 45 GB/s)
  const char* eg = getenv("TQR_XFER_GBS");
  const double gbs = eg ? std::max(1.0, atof(eg)) : 45.0;
  const double elem_s = 4.0 * pl->b * pl->b * shape_info(pl->shape).sw / (pl->dtype == TQR_F64 ? 0.175e12 : 0.38e12);
  xp.tcol = ((double)pl->m * pl->b * pl->es / (gbs * 1e9)) / elem_s;
  FlowPlan fp;
  build_flow_plan(pl->p, pl->q, pl->ns, pl->ng, pl->knobs, fp, &xp);  // the plan's own knobs (not the environment now)
  Item* d = nullptr;
  if (hipMalloc(&d, sizeof(Item) * fp.items.size()) != hipSuccess) return TQR_ENOMEM;
  if (hipMemcpy(d, fp.items.data(), sizeof(Item) * fp.items.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return TQR_EHIP;
  }
  pl->d_flow_x = d;
  pl->nflow_x = (int)fp.items.size();
  pl->nxc = xp.nxc;
  pl->xrows = xrows;
  return TQR_OK;
}

// tau: compact device array -> the reference's m x n matrix (column k*b of tau = compact column k,
// rows k*b .. m-1; other entries untouched)
static int tau_out(tqr_plan* pl, void* tau, int ldm, size_t es, hipStream_t s) {
  const int m = pl->m, b = pl->b, kmax = pl->kmax;
  std::vector<char> ct(es * (size_t)m * kmax);
  HIPCHK(hipMemcpyAsync(ct.data(), pl->hT, ct.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int k = 0; k < kmax; ++k)
    memcpy((char*)tau + es * ((size_t)k * b * ldm + (size_t)k * b), ct.data() + es * ((size_t)k * m + (size_t)k * b),
           es * (size_t)(m - k * b));
  return TQR_OK;
}

static int geqrt_host_flow(tqr_plan* pl, void* A, void* tau, int ldm, size_t es) {
  const int m = pl->m, n = pl->n, q = pl->q, b = pl->b;
  int st;
  if ((st = plan_host_buffers(pl, es)) || (st = plan_xfer_list(pl))) return st;
  if (!pl->sC && hipStreamCreateWithFlags(&pl->sC, hipStreamNonBlocking) != hipSuccess) return TQR_EHIP;
  hipStream_t s = pl->sC;
  HIPCHK(hipMemsetAsync(pl->hT, 0, es * (size_t)m * pl->kmax, s));
  const char* mode = getenv("TQR_HOST_XFER");
  if (mode && strcmp(mode, "register") == 0) {
    const size_t span = es * ((size_t)(n - 1) * ldm + m);
    if (hipHostRegister(A, span, hipHostRegisterMapped) == hipSuccess) {
      void* dv = nullptr;
      if (hipHostGetDevicePointer(&dv, A, 0) != hipSuccess) {
        (void)hipHostUnregister(A);
        return TQR_EHIP;
      }
      XferArgs xa{dv, dv, ldm, nullptr, nullptr, 0};
      st = plan_execute_serial(pl, pl->hA, m, pl->hT, s, &xa);
      if (st == TQR_OK) st = tqr_plan_status(pl, s);
      else (void)hipStreamSynchronize(s);
      (void)hipHostUnregister(A);
      if (st == TQR_OK && tau) st = tau_out(pl, tau, ldm, es, s);
      return st;
    }
    (void)hipGetLastError();  // not registrable: stage instead
  }
  HostStage* hs;
  {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto& e = g_stage[dev];
    if (!e) e = new (std::nothrow) HostStage();
    if (!e) return TQR_ENOMEM;
    hs = e;
  }
  std::lock_guard<std::mutex> lk(hs->mu);
  const int nxc = pl->nxc;
  if ((st = hs->ensure(es * (size_t)m * n, (size_t)q * (1 + nxc)))) return st;
  void* dbuf = nullptr;
  HIPCHK(hipHostGetDevicePointer(&dbuf, hs->buf, 0));
  const int gen = ++hs->gen;
  int* hup = hs->flags;
  int* hdn = hs->flags + q;
  XferArgs xa{dbuf, dbuf, m, hs->dflags, hs->dflags + q, gen};
  // TQR_HOST_XFER_VERBOSE=1: where the time goes (launch, staging done, kernel, drain done)
  const bool verbose = getenv("TQR_HOST_XFER_VERBOSE") && atoi(getenv("TQR_HOST_XFER_VERBOSE")) == 1;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  std::atomic<long long> t_up{0}, t_dn{0};
  // host side, beside the launch: nu threads stage tile columns in order (the last one to finish a
  // column flags it), nd threads move finished chunks back to the caller's array. They start
  // BEFORE the launch call: the launched kernel waits for the staging flags, so the staging must
  // not depend on this thread returning from HIP calls (another thread's hipFree — e.g. a
  // concurrent tqr_cache_clear — waits for the device to be idle, i.e. for this kernel; a staging
  // started behind a HIP call stalled by it would leave the kernel waiting until its timeout)
  std::atomic<int> launched{0};
  const int nthr = host_threads();
  const int nu = std::max(1, nthr / 2), nd = std::max(1, nthr - nu);
  const size_t col = es * (size_t)m;
  char* user = (char*)A;
  std::vector<std::atomic<int>> staged(q);
  for (auto& x : staged) x.store(0);
  std::atomic<int> failed{0};
  std::vector<std::function<void()>> jobs;
  // TQR_HOST_STAGE_DELAY_MS (tests only): a slow host, each tile column staged that much later
  const char* edl = getenv("TQR_HOST_STAGE_DELAY_MS");
  const int stage_delay_ms = edl ? std::max(0, atoi(edl)) : 0;
  for (int t = 0; t < nu; ++t)
    jobs.push_back([&, t] {
      for (int j = 0; j < q; ++j) {
        if (stage_delay_ms) std::this_thread::sleep_for(std::chrono::milliseconds(stage_delay_ms));
        for (int c = j * b + t; c < (j + 1) * b; c += nu) memcpy(hs->buf + c * col, user + (size_t)c * ldm * es, col);
        if (staged[j].fetch_add(1) + 1 == nu) __atomic_store_n(&hup[j], gen, __ATOMIC_RELEASE);
      }
      if (verbose) t_up.store(std::max<long long>(t_up.load(), (long long)((now() - t0) * 1e3)));
    });
  for (int t = 0; t < nd; ++t)
    jobs.push_back([&, t] {
      for (int j = 0; j < q; ++j) {
        for (int c = 0; c < nxc; ++c) {
          // the chunk's flag, or the launch ended without setting it (an engine error)
          for (long spins = 0; __atomic_load_n(&hdn[(size_t)j * nxc + c], __ATOMIC_ACQUIRE) < gen; ++spins) {
            if (failed.load(std::memory_order_relaxed)) return;
            if ((spins & 255) == 255) {
              if (launched.load(std::memory_order_acquire) && hipStreamQuery(s) != hipErrorNotReady &&
                  __atomic_load_n(&hdn[(size_t)j * nxc + c], __ATOMIC_ACQUIRE) < gen) {
                failed.store(1);
                return;
              }
              std::this_thread::yield();
            } else {
              __builtin_ia32_pause();
            }
          }
        }
        for (int c = j * b + t; c < (j + 1) * b; c += nd) memcpy(user + (size_t)c * ldm * es, hs->buf + c * col, col);
      }
      if (verbose) t_dn.store(std::max<long long>(t_dn.load(), (long long)((now() - t0) * 1e3)));
    });
  std::vector<std::thread> th;
  std::vector<size_t> inline_jobs;  // jobs whose thread could not be created: run after the launch
  for (size_t x = 0; x < jobs.size(); ++x) {
    try {
      th.emplace_back(jobs[x]);
    } catch (...) {
      inline_jobs.push_back(x);
    }
  }
  if (verbose) (void)hipEventRecord(pl->ev0, s);
  st = plan_execute_serial(pl, pl->hA, m, pl->hT, s, &xa);
  if (st == TQR_OK) {
    if (verbose) (void)hipEventRecord(pl->ev1, s);
    launched.store(1, std::memory_order_release);
  } else {
    failed.store(1);  // (the copy-out threads stop waiting)
  }
  for (size_t x : inline_jobs) jobs[x]();
  for (auto& t : th) t.join();
  if (st != TQR_OK) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  st = tqr_plan_status(pl, s);
  if (st == TQR_OK && failed.load()) st = TQR_EHIP;
  if (verbose && st == TQR_OK) {
    float kms = 0;
    HIPCHK(hipEventElapsedTime(&kms, pl->ev0, pl->ev1));
    fprintf(stderr, "tqr host xfer: %d host threads (%d in, %d out); staged all columns at %.2f ms, kernel %.2f ms, "
            "last chunk copied out at %.2f ms, done %.2f ms after the launch call\n", nthr, nu, nd, t_up.load() * 1e-3, kms,
            t_dn.load() * 1e-3, now() - t0);
  }
  if (st == TQR_OK && tau) st = tau_out(pl, tau, ldm, es, s);
  return st;
}

static int geqrt_host(void* A, void* tau, int m, int n, int ldm, int b, int dtype, int engine = TQR_ENGINE_DEFAULT) {
  if (!A || ldm < m || !valid_b(b) || m <= 0 || n <= 0 || m % b || n % b) return TQR_EINVAL;
  PlanRef ref;
  int st = cached_plan(m, n, b, dtype, ref, engine);
  if (st) return st;
  tqr_plan* pl = ref.pl;
  std::lock_guard<std::mutex> lk(pl->hmu);
  const size_t es = elem_size(dtype);
  if (pl->engine == TQR_ENGINE_FLOW) return geqrt_host_flow(pl, A, tau, ldm, es);
  if ((st = plan_host_buffers(pl, es)) || (st = plan_pinned_staging(pl, es))) return st;
  char* dA = (char*)pl->hA;
  if ((st = staged_copy(pl, (char*)A, ldm, dA, m, n, es, true))) return st;
  HIPCHK(hipMemsetAsync(pl->hT, 0, es * (size_t)m * pl->kmax, pl->sC));
  if ((st = plan_execute_serial(pl, dA, m, pl->hT, pl->sC, nullptr))) return st;
  if ((st = tqr_plan_status(pl, pl->sC))) return st;
  if ((st = staged_copy(pl, (char*)A, ldm, dA, m, n, es, false))) return st;
  return tau ? tau_out(pl, tau, ldm, es, pl->sC) : TQR_OK;
}

int tqr_dgeqrt_host(double* A, double* tau, int m, int n, int ldm, int b) { return geqrt_host(A, tau, m, n, ldm, b, TQR_F64); }
int tqr_sgeqrt_host(float* A, float* tau, int m, int n, int ldm, int b) { return geqrt_host(A, tau, m, n, ldm, b, TQR_F32); }
int tqr_geqrt_host_engine(int dtype, void* A, void* tau, int m, int n, int ldm, int b, int engine) {
  if (dtype != TQR_F32 && dtype != TQR_F64) return TQR_EINVAL;
  if (engine != TQR_ENGINE_DEFAULT && engine != TQR_ENGINE_WAVES && engine != TQR_ENGINE_FLOW) return TQR_EINVAL;
  return geqrt_host(A, tau, m, n, ldm, b, dtype, engine);
}

// Release every cached plan (the one-shot helpers' and the host API's device matrices, compact
// tau, pinned buffers) and the host-API staging buffers. Safe against concurrent tqr calls: the
// plans are unlinked from the cache under its lock (later calls build new ones), then each is
// destroyed once no call still uses it (PlanRef count) and its last execute has finished (its
// evDone event, whatever device or stream it ran on). A staging buffer is released under its own
// mutex, which a host-API call holds from before its launch until its last copy out; the
// HostStage objects themselves are kept (a call may hold a pointer to one), so a later call just
// allocates again.
int tqr_cache_clear(void) {
  std::vector<tqr_plan*> plans;
  std::vector<HostStage*> stages;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (auto& kv : g_cache) plans.push_back(kv.second);
    g_cache.clear();
    for (auto& kv : g_stage) stages.push_back(kv.second);
  }
  int st = TQR_OK;
  for (tqr_plan* pl : plans) {
    while (pl->users.load() > 0) std::this_thread::yield();
    {
      std::lock_guard<std::mutex> l1(pl->hmu);
      std::lock_guard<std::mutex> l2(pl->mu);
      if (pl->evDone && hipEventSynchronize(pl->evDone) != hipSuccess) st = TQR_EHIP;
    }
    tqr_plan_destroy(pl);
  }
  for (HostStage* hs : stages) {
    std::lock_guard<std::mutex> l2(hs->mu);
    hs->release();
  }
  return st;
}

}  // extern "C"
