// Plans: creation (both engines' item lists, counters, workspaces, kernels), destruction, status,
// statistics and the introspection calls of include/tqr.h, and plan_shape (solve.hpp). Host code only:
// the kernels a plan launches are engine.hip's, handed over by resolve / resolve_flow (plan.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <tuple>
#include <vector>

#include "gridscheduler.h"
#include "plan.hpp"
#include "solve.hpp"
#include "tqr.h"
#include "wave_dev.hpp"  // (host side only: wave_items, lds_panel, lds_update, wave_tw_bytes)

using namespace tqr;

// what solve.hip's tqr_lstsq_fused reads of a plan (solve.hpp)
tqr::PlanShape tqr::plan_shape(const tqr_plan* pl) { return PlanShape{pl->m, pl->n, pl->b, pl->dtype, pl->kmax, pl->capped}; }

extern "C" {

const char* tqr_strerror(int s) {
  switch (s) {
    case TQR_OK: return "ok";
    case TQR_EINVAL: return "invalid argument";
    case TQR_ENOMEM: return "out of memory";
    case TQR_EHIP: return "HIP runtime error";
    case TQR_ENODEV: return "no usable gfx950 device";
    case TQR_ERCCL: return "RCCL error";
  }
  return "unknown";
}

const char* tqr_version(void) { return "tqr 0.1 (gfx950, flat-tree tiled Householder QR)"; }

long tqr_total_tasks(int m, int n, int b) {
  if (b <= 0 || m % b || n % b) return -1;
  return tqr_sched_total_tasks(m / b, n / b);
}

void tqr_plan_destroy(tqr_plan* pl) {
  if (!pl) return;
  if (pl->d_items_p) (void)hipFree(pl->d_items_p);
  if (pl->d_items_u) (void)hipFree(pl->d_items_u);
  if (pl->d_T) (void)hipFree(pl->d_T);
  for (double* w : pl->wk) (void)hipFree(w);
  if (pl->d_wk) (void)hipFree(pl->d_wk);
  if (pl->sP) (void)hipStreamDestroy(pl->sP);
  if (pl->sU) (void)hipStreamDestroy(pl->sU);
  if (pl->evP) (void)hipEventDestroy(pl->evP);
  if (pl->evU) (void)hipEventDestroy(pl->evU);
  if (pl->evStart) (void)hipEventDestroy(pl->evStart);
  if (pl->d_flow) (void)hipFree(pl->d_flow);
  if (pl->d_sync) (void)hipFree(pl->d_sync);
  if (pl->ev0) (void)hipEventDestroy(pl->ev0);
  if (pl->ev1) (void)hipEventDestroy(pl->ev1);
  if (pl->evDone) (void)hipEventDestroy(pl->evDone);
  if (pl->hA) (void)hipFree(pl->hA);
  if (pl->hT) (void)hipFree(pl->hT);
  if (pl->d_flow_x) (void)hipFree(pl->d_flow_x);
  for (int x = 0; x < 2; ++x) {
    if (pl->pin[x]) (void)hipHostFree(pl->pin[x]);
    if (pl->pev[x]) (void)hipEventDestroy(pl->pev[x]);
  }
  if (pl->sC) (void)hipStreamDestroy(pl->sC);
  for (auto e : pl->prof_ev) (void)hipEventDestroy(e);
  close_opened(pl);
  if (pl->d_peers) (void)hipFree(pl->d_peers);
  if (pl->d_peer_wk) (void)hipFree(pl->d_peer_wk);
  if (pl->d_rf) (void)hipFree(pl->d_rf);
  delete pl;
}

int tqr_plan_create(tqr_plan** out, int m, int n, int b, int dtype) {
  return plan_create(out, m, n, b, dtype, 0, 1, TQR_ENGINE_DEFAULT);
}
int tqr_plan_create_engine(tqr_plan** out, int m, int n, int b, int dtype, int engine) {
  if (engine != TQR_ENGINE_DEFAULT && engine != TQR_ENGINE_WAVES && engine != TQR_ENGINE_FLOW) return TQR_EINVAL;
  return plan_create(out, m, n, b, dtype, 0, 1, engine);
}
// A capped plan (include/tqr.h): panels for the leading `steps` tile columns only. Always the flow
// engine — the wave engine replays sched.c's waves of the whole DAG.
int tqr_plan_create_steps(tqr_plan** out, int m, int n, int b, int dtype, int steps) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!valid_b(b) || m <= 0 || n <= 0 || steps < 1 || steps > std::min(m, n) / b) return TQR_EINVAL;
  return plan_create(out, m, n, b, dtype, 0, 1, TQR_ENGINE_FLOW, steps);
}
int tqr_plan_steps(const tqr_plan* pl) { return pl ? pl->kmax : TQR_EINVAL; }

}  // extern "C"

namespace tqr {
// steps > 0: tqr_plan_create_steps's cap (already checked against min(m, n) / b)
int plan_create(tqr_plan** out, int m, int n, int b, int dtype, int rank, int world, int engine, int steps) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || (dtype != TQR_F32 && dtype != TQR_F64) ||
      !valid_ld(m, elem_size(dtype)))
    return TQR_EINVAL;
  int st = current_device_is_gfx950();
  if (st) return st;
  tqr_plan* pl = new (std::nothrow) tqr_plan();
  if (!pl) return TQR_ENOMEM;
  pl->m = m; pl->n = n; pl->b = b; pl->p = m / b; pl->q = n / b;
  pl->rank = rank; pl->world = world; pl->cyclic = world > 1 && dist_cyclic();
  pl->capped = steps > 0;
  pl->kmax = flow_kmax(pl->p, pl->q, steps);
  pl->dtype = dtype;
  pl->es = elem_size(dtype);

  std::vector<Item> ip, iu;
  if (!wave_items(pl->p, pl->q, b, ip, iu, pl->off_p, pl->off_u)) { delete pl; return TQR_ENOMEM; }
  pl->nlevels = (int)pl->off_p.size() - 1;

  if (engine == TQR_ENGINE_DEFAULT) {
    const char* eng = getenv("TQR_ENGINE");
    engine = (eng && strcmp(eng, "waves") == 0) ? TQR_ENGINE_WAVES : TQR_ENGINE_FLOW;
  }
  pl->engine = world > 1 ? TQR_ENGINE_FLOW : engine;  // the multi-GPU protocol lives in the flow engine
  size_t tw = pl->engine == 0 ? wave_tw_bytes(pl->p, pl->kmax, b) : 8;
  if (hipMalloc(&pl->d_items_p, std::max<size_t>(1, ip.size()) * sizeof(Item)) != hipSuccess ||
      hipMalloc(&pl->d_items_u, std::max<size_t>(1, iu.size()) * sizeof(Item)) != hipSuccess ||
      hipMalloc(&pl->d_T, tw) != hipSuccess) {
    tqr_plan_destroy(pl);
    return TQR_ENOMEM;
  }
  if (!ip.empty() && hipMemcpy(pl->d_items_p, ip.data(), ip.size() * sizeof(Item), hipMemcpyHostToDevice) != hipSuccess) {
    tqr_plan_destroy(pl); return TQR_EHIP;
  }
  if (!iu.empty() && hipMemcpy(pl->d_items_u, iu.data(), iu.size() * sizeof(Item), hipMemcpyHostToDevice) != hipSuccess) {
    tqr_plan_destroy(pl); return TQR_EHIP;
  }
  if (hipStreamCreateWithFlags(&pl->sP, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&pl->sU, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&pl->evP, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&pl->evU, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&pl->evStart, hipEventDisableTiming) != hipSuccess) {
    tqr_plan_destroy(pl); return TQR_EHIP;
  }
  kfn kt;
  if (resolve(b, dtype, &pl->kp, &pl->ku, &kt) != TQR_OK) { tqr_plan_destroy(pl); return TQR_EHIP; }
  pl->ldsP = lds_panel(b);
  pl->ldsU = lds_update(b);
  if (hipEventCreate(&pl->ev0) != hipSuccess || hipEventCreate(&pl->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&pl->evDone, hipEventDisableTiming) != hipSuccess) {
    tqr_plan_destroy(pl); return TQR_EHIP;
  }
  // persistent dataflow engine: task list, progress counters, panel workspaces, kernel
  pl->shape = flow_shape(dtype, b);
  pl->nt = shape_info(pl->shape).nt;
  pl->ns = shape_ns(pl->shape, b);  // chain strips per tile
  pl->ng = b / shape_ib(pl->shape, b);  // reflector groups per tile
  if (pl->engine == TQR_ENGINE_FLOW) {
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) {
      tqr_plan_destroy(pl); return TQR_EHIP;
    }
    const int full_grid = pr.multiProcessorCount * shape_info(pl->shape).wpc;  // (ShapeW4: two workgroups per CU)
    pl->grid = full_grid;
    if (const char* gs = getenv("TQR_FLOW_GRID")) pl->grid = std::max(1, atoi(gs));
    FlowPlan fp;
    pl->knobs = flow_knobs(pl->p, pl->q, dtype, world, pl->grid >= full_grid, 0, steps, b);
    if (const char* eca = getenv("TQR_CHAIN_ASM")) pl->chain_asm = atoi(eca) & 3;  // 0 off, 1 on, 2 late strip loads
    // (bit 2: UNMQR elements on the full TSMQR bodies instead of the zero-row-skipping ones; A/B only)
    if (const char* eu = getenv("TQR_UNMQR_SKIP"); eu && atoi(eu) == 0 && pl->chain_asm) pl->chain_asm |= 4;
    // (bit 3: fp32 storage on the compiler-scheduled flow_chain32; A/B only)
    if (const char* e32 = getenv("TQR_CHAIN32_ASM"); e32 && atoi(e32) == 0) pl->chain_asm |= 8;
    // (bit 4: whole-line strips between steps, flow_list.hpp strip_permuted — only the form that knows
    // the layout: the fp64 generated chain with late strip loads, 8-wave shape, tiles of 256, at any
    // number of ranks; TQR_STRIP_LINES=0 keeps every strip standard, A/B runs)
    if (dtype == TQR_F64 && b == 256 && pl->shape == 8 && (pl->chain_asm & 3) == 2) {
      const char* el = getenv("TQR_STRIP_LINES");
      if (!el || atoi(el) != 0) pl->chain_asm |= 16;
    }
    build_flow_plan(pl->p, pl->q, pl->ns, pl->ng, pl->knobs, fp, nullptr, steps);
    pl->nflow_global = (int)fp.items.size();
    pl->list_hash = flow_list_hash(fp.items);  // of the global list: the ranks must agree on it (tqr_dist_import)
    if (world > 1) partition_flow_plan(fp, rank, world);
    pl->nflow = (int)fp.items.size();
    pl->est_order = fp.est_order;
    // next, err, host-transfer progress (flow.hpp timed_out), exit count, Rc, Tc, Ac, Rt, Rr, then Uc (upload chunks per tile column, host-pointer API)
    pl->sync_ints = 4 + 3 * (size_t)pl->kmax * pl->ng + (size_t)pl->p * pl->q * pl->ns +
                    (size_t)pl->kmax * pl->q * pl->ns * pl->ng + (size_t)pl->q;
    if (pl->nflow <= 0 || hipMalloc(&pl->d_flow, sizeof(Item) * pl->nflow) != hipSuccess ||
        hipMalloc(&pl->d_sync, sizeof(int) * pl->sync_ints) != hipSuccess ||
        hipMalloc(&pl->d_wk, sizeof(double*) * pl->kmax) != hipSuccess) {
      tqr_plan_destroy(pl); return TQR_ENOMEM;
    }
    // one workspace per step k: V then T images of tiles (k..p-1, k), every group.
    // Multi-GPU: peers' panel tasks write images of their panels into these slots over xGMI,
    // and such writes do not pass through this device's L2 — a line of a slot left in L2 by the
    // previous execute's reads would be served stale to this execute's chains. The slots are
    // therefore uncached (like the member flags); TQR_DIST_WK_CACHED=1 keeps them cached (the
    // one-GPU rehearsal's A/B of that cost only).
    const bool wk_uc = world > 1 && !(getenv("TQR_DIST_WK_CACHED") && atoi(getenv("TQR_DIST_WK_CACHED")) == 1);
    for (int k = 0; k < pl->kmax; ++k) {
      double* w = nullptr;
      const size_t wb = wk_bytes(b, pl->p - k, dtype, shape_ib(pl->shape, b));
      if ((wk_uc ? hipExtMallocWithFlags((void**)&w, wb, hipDeviceMallocUncached) : hipMalloc(&w, wb)) != hipSuccess) {
        tqr_plan_destroy(pl); return TQR_ENOMEM;
      }
      pl->wk.push_back(w);
    }
    if (hipMemcpy(pl->d_wk, pl->wk.data(), sizeof(double*) * pl->kmax, hipMemcpyHostToDevice) != hipSuccess) {
      tqr_plan_destroy(pl); return TQR_EHIP;
    }
    if (hipMemcpy(pl->d_flow, fp.items.data(), sizeof(Item) * pl->nflow, hipMemcpyHostToDevice) != hipSuccess) {
      tqr_plan_destroy(pl); return TQR_EHIP;
    }
    if (world > 1) {
      // member flags (+ Done[world] + Probe[world]) in uncached memory (peers' panels set them over
      // xGMI); zeroed once: their values are launch epochs (flow.hpp FlowArgs), Probe[r] rank r's
      // setup token (tqr_dist_probe)
      const size_t nrf = sizeof(int) * ((size_t)pl->kmax * pl->p * pl->ng + 2 * (size_t)world);
      if (hipExtMallocWithFlags((void**)&pl->d_rf, nrf, hipDeviceMallocUncached) != hipSuccess || hipMemset(pl->d_rf, 0, nrf) != hipSuccess ||
          hipMalloc(&pl->d_peers, sizeof(PeerBufs) * world) != hipSuccess ||
          hipMalloc(&pl->d_peer_wk, sizeof(double*) * (size_t)world * pl->kmax) != hipSuccess) {
        tqr_plan_destroy(pl); return TQR_ENOMEM;
      }
    }
    pl->kflow = resolve_flow(b, dtype, pl->shape);
    pl->ldsF = lds_flow(b, dtype, pl->shape);
    if (!pl->kflow) { tqr_plan_destroy(pl); return TQR_EHIP; }
  }
  *out = pl;
  return TQR_OK;
}
}  // namespace tqr

extern "C" {

int tqr_plan_status(tqr_plan* pl, void* stream) {
  if (!pl) return TQR_EINVAL;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (pl->engine != TQR_ENGINE_FLOW) return TQR_OK;  // wave engine: no in-kernel waits to time out
  int err = 0;
  HIPCHK(hipMemcpy(&err, pl->d_sync + 1, sizeof(int), hipMemcpyDeviceToHost));
  if (err) {
    fprintf(stderr, "tqr: dataflow engine aborted (error word %d: a dependency wait timed out)\n", err);
    return TQR_EHIP;
  }
  return TQR_OK;
}

int tqr_plan_set_tasks(tqr_plan* pl, const int* items, int n) {
  if (!pl || !items || pl->engine != TQR_ENGINE_FLOW || pl->world != 1 || n != pl->nflow) return TQR_EINVAL;
  std::vector<Item> L(n), cur(n);
  for (int x = 0; x < n; ++x) L[x] = Item{items[4 * x], items[4 * x + 1], items[4 * x + 2], items[4 * x + 3]};
  std::lock_guard<std::mutex> lk(pl->mu);
  HIPCHK(hipEventSynchronize(pl->evDone));  // no execute may be using the current list
  HIPCHK(hipMemcpy(cur.data(), pl->d_flow, sizeof(Item) * n, hipMemcpyDeviceToHost));
  auto key = [](const Item& a) { return std::make_tuple(a.ts, a.l, a.m, a.k); };
  std::vector<std::tuple<int, int, int, int>> ka, kb;
  for (auto& it : L) ka.push_back(key(it));
  for (auto& it : cur) kb.push_back(key(it));
  std::sort(ka.begin(), ka.end());
  std::sort(kb.begin(), kb.end());
  if (ka != kb || !flow_list_topological(L, pl->p, pl->q, pl->ns)) return TQR_EINVAL;
  HIPCHK(hipMemcpy(pl->d_flow, L.data(), sizeof(Item) * n, hipMemcpyHostToDevice));
  return TQR_OK;
}

int tqr_plan_get_tasks(tqr_plan* pl, int* items, int cap) {
  if (!pl || pl->engine != TQR_ENGINE_FLOW || cap < 0 || (cap > 0 && !items)) return TQR_EINVAL;
  const int n = std::min(cap, pl->nflow);
  if (n > 0) {
    std::vector<Item> cur(n);
    std::lock_guard<std::mutex> lk(pl->mu);
    HIPCHK(hipMemcpy(cur.data(), pl->d_flow, sizeof(Item) * n, hipMemcpyDeviceToHost));
    for (int x = 0; x < n; ++x) {
      items[4 * x] = cur[x].ts; items[4 * x + 1] = cur[x].l;
      items[4 * x + 2] = cur[x].m; items[4 * x + 3] = cur[x].k;
    }
  }
  return pl->nflow;
}

int tqr_plan_debug_workspace(const tqr_plan* pl, int k, void* host, size_t bytes) {
  if (!pl || pl->engine != TQR_ENGINE_FLOW || k < 0 || k >= pl->kmax || !host) return TQR_EINVAL;
  const size_t have = wk_bytes(pl->b, pl->p - k, pl->dtype, shape_ib(pl->shape, pl->b));
  HIPCHK(hipMemcpy(host, pl->wk[k], std::min(bytes, have), hipMemcpyDeviceToHost));
  return (int)std::min<size_t>(have, 0x7fffffff);
}

int tqr_plan_info(const tqr_plan* pl, int* engine, int* ntasks, int* est_order, int* grid) {
  if (!pl) return TQR_EINVAL;
  if (engine) *engine = pl->engine;
  if (ntasks) *ntasks = pl->engine == 1 ? pl->nflow : (int)pl->off_u.back();
  if (est_order) *est_order = pl->est_order;
  if (grid) *grid = pl->grid;
  return TQR_OK;
}

int tqr_plan_set_profile(tqr_plan* pl, int on) {
  if (!pl) return TQR_EINVAL;
  pl->profile = on;
  return TQR_OK;
}

int tqr_plan_stats(const tqr_plan* pl, int* nu, double* msu, int* np, double* msp) {
  if (!pl) return TQR_EINVAL;
  if (nu) *nu = pl->nl_u;
  if (msu) *msu = pl->ms_u;
  if (np) *np = pl->nl_p;
  if (msp) *msp = pl->ms_p;
  return TQR_OK;
}

}  // extern "C"
