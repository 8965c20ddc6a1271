// Multi-GPU setup (include/tqr.h tqr_dist_*): the plan of one rank, the IPC hand-shake that opens
// the peers' panel workspaces and member flags (export / import, with the task-list signature every
// rank must share), the peer-path probe with its two kernels, and the partition queries. The launch
// itself is the flow engine's (engine.hip); nothing here sees the device templates.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "plan.hpp"
#include "tqr.h"

using namespace tqr;

namespace tqr {
void close_opened(tqr_plan* pl) {
  for (void* p : pl->opened) (void)hipIpcCloseMemHandle(p);
  pl->opened.clear();
}
}  // namespace tqr

extern "C" {

int tqr_dist_plan_create(tqr_plan** out, int m, int n, int b, int dtype, int rank, int world) {
  if (world < 1 || rank < 0 || rank >= world) return TQR_EINVAL;
  return plan_create(out, m, n, b, dtype, rank, world, TQR_ENGINE_FLOW);
}

// ---- multi-GPU ------------------------------------------------------------------------------
// handle block: the PCI bus id of the exporting device (64 bytes), then the IPC handles of its
// member flags and of its per-step panel workspaces
static constexpr size_t kBusIdBytes = 64;
// a rank's handle: PCI bus id, the task-list signature (every rank must partition the same global
// list: segment lengths, lookahead tail, list length), the IPC handles of Rf and the workspaces
constexpr size_t kSigInts = 7;
static void plan_signature(const tqr_plan* pl, int* sig) {
  sig[0] = pl->knobs.seglen; sig[1] = pl->knobs.seglen_la; sig[2] = pl->knobs.la_tail; sig[3] = pl->nflow_global;
  sig[4] = pl->knobs.tail; sig[5] = pl->knobs.tail_sl; sig[6] = (int)pl->list_hash;
}
size_t tqr_dist_handle_bytes(const tqr_plan* pl) {
  return pl ? kBusIdBytes + sizeof(int) * kSigInts + sizeof(hipIpcMemHandle_t) * (1 + (size_t)pl->kmax) : 0;
}

int tqr_dist_export(tqr_plan* pl, void* buf, size_t len) {
  if (!pl || pl->world < 2 || !buf || len < tqr_dist_handle_bytes(pl)) return TQR_EINVAL;
  char bus[kBusIdBytes] = {0};
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetPCIBusId(bus, (int)kBusIdBytes - 1, dev));
  std::vector<hipIpcMemHandle_t> h(1 + pl->kmax);
  HIPCHK(hipIpcGetMemHandle(&h[0], pl->d_rf));
  for (int k = 0; k < pl->kmax; ++k) HIPCHK(hipIpcGetMemHandle(&h[1 + k], pl->wk[k]));
  int sig[kSigInts];
  plan_signature(pl, sig);
  memcpy(buf, bus, kBusIdBytes);
  memcpy((char*)buf + kBusIdBytes, sig, sizeof(sig));
  memcpy((char*)buf + kBusIdBytes + sizeof(sig), h.data(), sizeof(hipIpcMemHandle_t) * h.size());
  return TQR_OK;
}

// Peer reachability of the device that exported `bus`: the same device (ranks sharing a GPU)
// needs nothing; another device must be peer-accessible from this one (xGMI), and peer access
// is enabled explicitly before any handle is opened — a missing link fails here, loudly,
// instead of as a fault or a hang inside the persistent launch.
static int enable_peer(int rank, int r, const char* bus) {
  int me = 0, peer = -1;
  HIPCHK(hipGetDevice(&me));
  if (hipDeviceGetByPCIBusId(&peer, bus) != hipSuccess) {
    (void)hipGetLastError();
    // not visible in this process (e.g. HIP_VISIBLE_DEVICES): the IPC open decides
    fprintf(stderr, "tqr: rank %d: rank %d's device %s is not visible here; relying on IPC peer mapping\n", rank, r, bus);
    return TQR_OK;
  }
  if (peer == me) return TQR_OK;
  int can = 0;
  HIPCHK(hipDeviceCanAccessPeer(&can, me, peer));
  if (!can) {
    fprintf(stderr, "tqr: rank %d: device %d cannot access rank %d's device %d (%s): no peer path\n", rank, me, r, peer, bus);
    return TQR_EHIP;
  }
  hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
  if (e == hipErrorPeerAccessAlreadyEnabled) {
    (void)hipGetLastError();
  } else if (e != hipSuccess) {
    fprintf(stderr, "tqr: rank %d: enabling peer access to device %d failed: %s\n", rank, peer, hipGetErrorString(e));
    return TQR_EHIP;
  }
  return TQR_OK;
}

int tqr_dist_import(tqr_plan* pl, const void* all, size_t len) {
  const size_t hb = tqr_dist_handle_bytes(pl);
  if (!pl || pl->world < 2 || !all || len < (size_t)pl->world * hb || pl->imported) return TQR_EINVAL;
  close_opened(pl);  // a previous failed import
  std::vector<PeerBufs> pb(pl->world);
  std::vector<double*> pwk((size_t)pl->world * pl->kmax, nullptr);
  for (int r = 0; r < pl->world; ++r) {
    double** tab = pl->d_peer_wk + (size_t)r * pl->kmax;
    if (r == pl->rank) {
      for (int k = 0; k < pl->kmax; ++k) pwk[(size_t)r * pl->kmax + k] = pl->wk[k];
      pb[r] = PeerBufs{tab, pl->d_rf};
      continue;
    }
    const char* blk = (const char*)all + (size_t)r * hb;
    int sig[kSigInts], mine[kSigInts];
    memcpy(sig, blk + kBusIdBytes, sizeof(sig));
    plan_signature(pl, mine);
    if (memcmp(sig, mine, sizeof(sig)) != 0) {  // a launch over different lists would deadlock
      fprintf(stderr, "tqr: rank %d and rank %d built different task lists (segment lengths %d/%d vs %d/%d, "
              "lookahead tail %d vs %d, tail %d/%d vs %d/%d, %d vs %d tasks, list hash %08x vs %08x): set "
              "TQR_SEGLEN / TQR_TAIL / TQR_LA / TQR_LAC / TQR_TG / TQR_LAZY / TQR_FLOW_GRID alike on every rank\n",
              pl->rank, r, mine[0], mine[1], sig[0], sig[1], mine[2], sig[2], mine[4], mine[5], sig[4], sig[5],
              mine[3], sig[3], (unsigned)mine[6], (unsigned)sig[6]);
      close_opened(pl);
      return TQR_EINVAL;
    }
    char bus[kBusIdBytes];
    memcpy(bus, blk, kBusIdBytes);
    bus[kBusIdBytes - 1] = 0;
    int st = enable_peer(pl->rank, r, bus);
    if (st) { close_opened(pl); return st; }
    std::vector<hipIpcMemHandle_t> h(1 + pl->kmax);
    memcpy(h.data(), blk + kBusIdBytes + sizeof(sig), hb - kBusIdBytes - sizeof(sig));
    for (int x = 0; x <= pl->kmax; ++x) {
      void* p = nullptr;
      if (hipIpcOpenMemHandle(&p, h[x], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        fprintf(stderr, "tqr: rank %d cannot open rank %d's workspace (IPC handle %d)\n", pl->rank, r, x);
        close_opened(pl);
        return TQR_EHIP;
      }
      pl->opened.push_back(p);
      if (x == 0) pb[r].Rf = (int*)p;
      else pwk[(size_t)r * pl->kmax + x - 1] = (double*)p;
    }
    pb[r].Wk = tab;
  }
  if (hipMemcpy(pl->d_peer_wk, pwk.data(), sizeof(double*) * pwk.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pl->d_peers, pb.data(), sizeof(PeerBufs) * pl->world, hipMemcpyHostToDevice) != hipSuccess) {
    close_opened(pl);
    return TQR_EHIP;
  }
  pl->imported = true;
  return TQR_OK;
}

// ---- peer-path probe (setup): the flag path of the persistent launch, exercised once ----------
// A panel's owner sets the member flags in its peers' Rf with system-scope stores through the
// IPC-mapped peer pointers, and the chains poll their own Rf with system-scope loads (flow.hpp).
// A broken path would otherwise show up only as a 60 s wait timeout inside the first factorisation
// (or never, as a hang, if the stores are silently lost), so the setup runs the same two operations
// on a probe word per rank: put (every rank stores its token into each peer's Probe[rank]), a host
// barrier, then check (every rank loads its own Probe[r] of every peer r).
static int probe_token(int rank) { return 0x7e510000 | (rank + 1); }
__global__ void k_probe_put(const PeerBufs* peers, long off, int rank, int world, int token) {
  const int r = threadIdx.x;
  if (r < world && r != rank)
    __hip_atomic_store((__attribute__((address_space(1))) int*)(peers[r].Rf + off + rank), token, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_probe_get(int* rf, long off, int world, int* out) {
  const int r = threadIdx.x;
  // (the system-scope load of flow.hpp's ld_sys)
  if (r < world)
    out[r] = __hip_atomic_load((__attribute__((address_space(1))) int*)(rf + off + r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
int tqr_dist_probe(tqr_plan* pl, int phase, unsigned long long* seen) {
  if (!pl || pl->world < 2 || !pl->imported || pl->world > 64 || (phase != 0 && phase != 1)) return TQR_EINVAL;
  const long off = (long)pl->kmax * pl->p * pl->ng + pl->world;  // Probe[] after Done[]
  if (phase == 0) {
    hipLaunchKernelGGL(k_probe_put, dim3(1), dim3(64), 0, 0, (const PeerBufs*)pl->d_peers, off, pl->rank, pl->world,
                       probe_token(pl->rank));
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return TQR_OK;
  }
  int* d_out = nullptr;
  HIPCHK(hipMalloc(&d_out, sizeof(int) * 64));
  hipLaunchKernelGGL(k_probe_get, dim3(1), dim3(64), 0, 0, pl->d_rf, off, pl->world, d_out);
  int h[64] = {0};
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(h, d_out, sizeof(int) * pl->world, hipMemcpyDeviceToHost);
  (void)hipFree(d_out);
  if (e != hipSuccess) {
    fprintf(stderr, "tqr: rank %d: peer probe failed: %s\n", pl->rank, hipGetErrorString(e));
    return TQR_EHIP;
  }
  unsigned long long got = 0;
  for (int r = 0; r < pl->world; ++r)
    if (r != pl->rank && h[r] == probe_token(r)) got |= 1ull << r;
  if (seen) *seen = got;
  int st = TQR_OK;
  for (int r = 0; r < pl->world; ++r)
    if (r != pl->rank && !((got >> r) & 1)) {
      fprintf(stderr, "tqr: rank %d does not see rank %d's flag stores (probe word 0x%08x, expected 0x%08x): no working "
              "peer path for the panel flags\n", pl->rank, r, (unsigned)h[r], (unsigned)probe_token(r));
      st = TQR_EHIP;
    }
  return st;
}

// Kept for the API: since round 4 every execute resets its own (local) counters, and the
// cross-rank flags carry launch epochs, so consecutive multi-GPU executes need no reset, host
// synchronisation or barrier (flow.hpp FlowArgs Done[]).
int tqr_dist_reset(tqr_plan* pl, void* stream) {
  (void)stream;
  if (!pl || pl->world < 2) return TQR_EINVAL;
  return TQR_OK;
}

int tqr_dist_local_cols(const tqr_plan* pl) {
  if (!pl || pl->capped) return TQR_EINVAL;
  int c = 0;
  for (int j = 0; j < pl->q; ++j) c += tile_owner(j, pl->world, pl->cyclic) == pl->rank;
  return c;
}

long long tqr_plan_fwd_bytes(const tqr_plan* pl) {
  if (!pl) return TQR_EINVAL;
  if (pl->world < 2) return 0;
  long long members = 0;  // panel members of the tile columns this rank owns
  for (int k = 0; k < pl->kmax; ++k)
    if (tile_owner(k, pl->world, pl->cyclic) == pl->rank) members += pl->p - k;
  const long long slot = (long long)(wk_bytes(pl->b, 1, pl->dtype, shape_ib(pl->shape, pl->b)));  // one member's images, all groups
  return members * slot * (pl->world - 1);
}

int tqr_dist_owner(const tqr_plan* pl, int tile_col) {
  if (!pl || pl->capped || tile_col < 0 || tile_col >= pl->q) return TQR_EINVAL;
  return tile_owner(tile_col, pl->world, pl->cyclic);
}

}  // extern "C"
