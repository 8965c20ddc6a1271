// What more than one unit of the library needs of a plan: struct tqr_plan itself, the kernels'
// argument blocks and pointer types, the host mirrors of the workspace slot sizes, and the few
// functions that cross units. The units: engine.hip (every kernel but the peer probe's, the launch
// code, the diagnostic builds' device symbols), plans.hip (creation, destruction, introspection),
// dist.hip (multi-GPU setup), hostpath.hip (plan cache, host-pointer path), tileapi.hip (single-tile
// and tile-batch API).
//
// RULE: this header tests no build macro — not TQR_STAMPS, TQR_FLOW_STAMPS, TQR_DIAG_*, nor anything
// the Makefile passes as VDEF or DIAG. The diagnostic targets (stamps, flowstamps, diag, variant)
// link an engine.o built WITH such macros against host objects built WITHOUT them, so everything
// declared here must mean the same in both. For the same reason it includes none of the device
// headers (tiles.hpp, flow.hpp, wave_dev.hpp): only engine.hip may depend on those flags.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "flow_list.hpp"
#include "flowplan.hpp"
#include "host_common.hpp"

namespace tqr {

struct Args {
  void* A;        // matrix (S*)
  void* tau;      // compact tau (S*), m x kmax
  double* Tw;     // T factors: [(k*p + i)*NG + g][IB*IB]
  const Item* items;
  long ldm;
  int m, p, kmax;
};
struct FlowArgs;  // flow.hpp (engine.hip fills it; a plan only holds the kernel's pointer)

typedef void (*kfn)(Args);
typedef void (*ffn)(FlowArgs);

// workspace slot sizes (doubles) of Geo<b, ib>::TIMG / VIMG / TPIMG (ib: reflectors per group);
// engine.hip's static_asserts tie these mirrors to tiles.hpp
static inline size_t timg_doubles(int b, int ib = 32) {
  ib = std::min(b, ib);
  return ((size_t)ib * (ib + 1) + 127) / 128 * 128;
}
static inline size_t vimg_doubles(int b, int ib = 32) {
  ib = std::min(b, ib);
  return ((size_t)b * (ib + 2) + 127) / 128 * 128;
}
static inline size_t tpimg_doubles(int b, int ib = 32) {  // packed T image (Geo<b, ib>::TPIMG)
  const size_t nri = std::min(b, ib) / 4;
  return (16 * nri * nri + 127) / 128 * 128;
}
// fp32 chain image slots (doubles; tiles.hpp Geo32 / Img<B, float>)
static inline size_t vimg32_doubles(int b) { return (size_t)b * (b < 32 ? b : 32) / 2; }  // VR floats / 2
static inline size_t timg32_doubles(int b) {
  const size_t nmi = (b < 32 ? b : 32) / 16, npr = nmi * (nmi + 1) / 2;
  return (npr * 256 / 2 + 127) / 128 * 128;
}
// flow engine workspace of one step with `rows` tile rows (flow.hpp flow_vw_off / flow_tw_off);
// ib: the engine shape's group size (fp32: 32)
static inline size_t wk_bytes(int b, int rows, int dtype, int ib) {
  ib = std::min(b, ib);
  const size_t ng = b / ib;
  const size_t slot = dtype == TQR_F64 ? vimg_doubles(b, ib) + tpimg_doubles(b, ib) : vimg32_doubles(b) + timg32_doubles(b);
  return (size_t)rows * ng * slot * sizeof(double);
}

}  // namespace tqr

struct tqr_plan {
  int m, n, b, p, q, kmax, dtype, nlevels;
  size_t es;
  std::vector<long> off_p, off_u;  // per wave offsets into the item arrays
  tqr::Item* d_items_p = nullptr;
  tqr::Item* d_items_u = nullptr;
  double* d_T = nullptr;   // T factors of the wave-batched engine
  std::vector<double*> wk;  // flow engine: per-step panel workspaces (V and T images)
  double** d_wk = nullptr;  // device table of wk
  hipStream_t sP = nullptr, sU = nullptr;
  hipEvent_t evP = nullptr, evU = nullptr, evStart = nullptr;
  tqr::kfn kp = nullptr, ku = nullptr;
  size_t ldsP = 0, ldsU = 0;
  int profile = 0;
  int chain_asm = 2;  // fp64 chains on the hand-scheduled MFMA stream (TQR_CHAIN_ASM: 0 compiler-scheduled, 1 whole strip loaded in the hand-over, 2 late strip loads)
  // flow engine
  int engine = 1;          // 1 = persistent dataflow (default), 0 = wave-batched launches
  bool capped = false;     // tqr_plan_create_steps: kmax is the caller's cap (flow engine, one GPU, device pointers)
  tqr::Item* d_flow = nullptr;
  int nflow = 0;
  int nflow_global = 0;  // tasks of the global list (before a multi-GPU partition)
  unsigned list_hash = 0;  // FNV-1a of the global list's items in order (plan_signature)
  int* d_sync = nullptr;   // next, err, Rc, Tc, Ac, Rt, Rr
  size_t sync_ints = 0;
  int ns = 1, ng = 1, grid = 256, est_order = 0;
  int shape = 8, nt = 512;  // flow engine shape (flow_shape) and its workgroup size
  tqr::ffn kflow = nullptr;
  size_t ldsF = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> prof_ev;  // pairs per launch when profiling
  std::vector<int> prof_kind;
  int nl_u = 0, nl_p = 0;
  double ms_u = 0, ms_p = 0;
  // multi-GPU (tile-column snake partition; cyclic = TQR_DIST_PART=cyclic): rank / world, uncached
  // panel counters, forward counters, peer workspaces opened by IPC
  int rank = 0, world = 1, cyclic = 0;
  int* d_rf = nullptr;     // multi-GPU member flags (uncached), kmax x p x ng, then Done[world]
  int epoch = 0;           // multi-GPU: launches so far (the member flags' and Done's values)
  tqr::PeerBufs* d_peers = nullptr;
  double** d_peer_wk = nullptr;  // world x kmax opened peer workspace pointers
  std::vector<void*> opened;     // IPC-opened peer pointers
  bool imported = false;         // tqr_dist_import succeeded (world > 1 may execute)
  // executions of one plan share its counters and workspaces: they are serialised — a host
  // mutex around each enqueue sequence, and every execute's stream waits for the previous one
  std::mutex mu;
  hipEvent_t evDone = nullptr;
  tqr::FlowKnobs knobs;  // task-list order knobs, read once at creation (segment lengths: flow.hpp seglen_of_chain)
  // host-pointer path (geqrt_host): device matrix and compact tau, kept with the (cached) plan
  // (tqr_cache_clear releases them); hmu serialises whole host-API calls on one plan. The flow
  // engine's transfers run inside its launch (xfer.hpp): a second task list with UP / DOWN
  // tasks (d_flow_x), nxc chunks of xrows rows per tile column. The wave engine stages through
  // two pinned buffers (pin, pev, sC) before / after its launches.
  std::mutex hmu;
  std::atomic<int> users{0};  // one-shot helpers using this cached plan right now (PlanRef)
  void* hA = nullptr;
  void* hT = nullptr;
  tqr::Item* d_flow_x = nullptr;
  int nflow_x = 0, nxc = 0, xrows = 0;
  void* pin[2] = {nullptr, nullptr};
  size_t pin_bytes = 0;
  hipStream_t sC = nullptr;
  hipEvent_t pev[2] = {nullptr, nullptr};
};

namespace tqr {

// transfer arguments of one host-pointer execute of the flow engine (xfer.hpp)
struct XferArgs {
  const void* hsrc;
  void* hdst;
  long hld;
  int* hup;  // device view of the host flags (or null)
  int* hdn;
  int gen;
};

// A cached plan in use by a one-shot helper: counted in plan->users from the lookup (under
// g_cache_mu) until the call returns, so tqr_cache_clear never frees a plan another thread is
// still using (it unlinks the plans first, then waits for each one's users to drain).
struct PlanRef {
  tqr_plan* pl = nullptr;
  PlanRef() = default;
  PlanRef(const PlanRef&) = delete;
  PlanRef& operator=(const PlanRef&) = delete;
  ~PlanRef() {
    if (pl) pl->users.fetch_sub(1);
  }
};

// engine.hip: the kernels of one (b, dtype) / one engine shape with their dynamic-LDS limits raised
// (resolve: TQR_OK or an error; resolve_flow: null on failure), the LDS bytes of k_flow and k_build_t
int resolve(int b, int dtype, kfn* kp, kfn* ku, kfn* kt);
ffn resolve_flow(int b, int dtype, int shape);
size_t lds_flow(int b, int dtype, int shape);
size_t lds_build_t(int b);
// engine.hip: one execute enqueued behind the plan's previous one (xa: the host-pointer path's transfers, or null)
int plan_execute_serial(tqr_plan* pl, void* dA, int ldda, void* dtau, hipStream_t cs, const XferArgs* xa);
// plans.hip: what every tqr_plan_create* and tqr_dist_plan_create (dist.hip) end in
int plan_create(tqr_plan** out, int m, int n, int b, int dtype, int rank, int world, int engine, int steps = 0);
// dist.hip: close the IPC-opened peer pointers (tqr_plan_destroy)
void close_opened(tqr_plan* pl);
// hostpath.hip: the plan cache of the one-shot helpers
int cached_plan(int m, int n, int b, int dtype, PlanRef& ref, int engine = TQR_ENGINE_DEFAULT);

}  // namespace tqr
