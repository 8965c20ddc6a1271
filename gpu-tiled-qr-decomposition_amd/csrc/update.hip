// Row update of a finished QR (include/tqr.h "row update"): append mw rows W to the R of an n x n
// triangle, R'^T R' = R^T R + W^T W, with the flat-tree tile operations restricted to the tiles that
// exist — per step k the TSQRT of [R_kk; W_lk] for every appended tile row l, each followed by its
// TSMQRs on [R_kj; W_lj], j > k. Single GPU.
//
//   tqr_update_rows     level-synchronous, as the wave engine: TSQRT(l,k) on level 2k + l, TSMQR(l,j,k)
//                       on level 2k + l + 1; every dependency lies on an earlier level and the items of
//                       one level touch disjoint data. Per level one launch of k_upd_panel (a TSQRT per
//                       workgroup) on one side stream and one of k_upd_update (a 64-column strip of a
//                       TSMQR per workgroup) on another, each stream waiting for the other's previous
//                       level by an event. No workgroup ever waits for another inside a launch: no
//                       flag, no counter, no spin.
//   tqr_update_prepare  k_upd_t: one workgroup per (W tile, reflector group) rebuilds the group's T from
//                       the stored V and taus — the TS branch of apply_dev.hpp's apply_t_body.
//   tqr_update_apply_q  k_upd_apply: one workgroup per 64 columns walks the q * wt TSMQRs on
//                       [Ctop_k; Cnew_l] — the tsmqr lambda of apply_q_body with the head rows and the
//                       body rows in two arrays.
//   tqr_update_lstsq    host only: the three above, a copy and solve.hip's tqr_trsm_r; k_upd_resnorm
//                       folds the new rows into the running residual norms.
// The two factorisation bodies are wave_dev.hpp's QRD branch of wave_panel and DAPP branch of
// wave_update with two base arrays in place of one (R tiles from dR / lddr, W tiles from dW / lddw, taus
// into dtau_u): the same tiles.hpp primitives on the same operands in the same order, so a wave plan on
// the stacked [G; W] equals a wave plan on G followed by this update, bit for bit.
// Of dR only elements (i, j), i <= j < n, are read or written: the TSQRT loads and stores the upper
// triangle of a diagonal tile's 32 x 32 diagonal blocks and whole head rows right of them, the TSMQR
// head rows of tiles right of the diagonal tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "apply.hpp"
#include "apply_dev.hpp"
#include "host_common.hpp"
#include "tqr.h"
#include "wave_dev.hpp"

namespace tqr {

struct UpdArgs {
  void* R;            // S*: the n x n triangle's array
  void* W;            // S*: mw x n appended rows / their TSQRT V
  void* tau;          // S*: mw x q, column k = the taus of step k's wt TSQRTs
  double* Tw;         // T images: [(k * wt + l) * NG + g][TIMG]
  const Item* items;  // the launch's items (factorisation kernels)
  void* Ctop;         // S*: n x nrhs (apply)
  void* Cnew;         // S*: mw x nrhs (apply)
  long ldr, ldw, ldct, ldcn;
  int mw, q, wt, nrhs;
};

template <int B>
__device__ __forceinline__ double* upd_tw(double* Tw, int wt, int l, int k, int g) {
  using G = Geo<B>;
  return Tw + (((size_t)k * wt + l) * G::NG + g) * G::TIMG;
}

// ---------------------------------------------------------------------------------------
// TSQRT of [R_kk; W_lk]: wave_panel's QRD branch, Rt in dR, Bt in dW. lds: lds_panel(B) bytes.
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void upd_panel(const UpdArgs& a, const Item it, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, VP = G::VP, TP = G::TP, NG = G::NG;
  double* Vs = lds;
  double* Hs = Vs + G::VSZ;
  double* Ts = Hs + G::TSZ;
  double* Gs = Ts + G::TSZ;
  double* tauv = Gs + G::TSZ;
  double* scratch = tauv + IB + 2;
  double* Gp = scratch + 2 * 4 * 32 + 4 * 32 + 2 * 32 + G::TSZ;  // 4 partial Grams

  const int l = it.l, k = it.k;
  const int t = threadIdx.x, w = t >> 6;
  const size_t ldr = a.ldr, ldw = a.ldw;
  S* Rt = (S*)a.R + (size_t)k * B * ldr + (size_t)k * B;  // R_kk
  S* Bt = (S*)a.W + (size_t)k * B * ldw + (size_t)l * B;  // W_lk
  S* tau = (S*)a.tau;
  double X[G::NKS];
  double H[G::NRI];

  for (int g = 0; g < NG; ++g) {
    const int c0 = g * IB;
#pragma unroll 8
    for (int idx = t; idx < B * IB; idx += NT) {
      int r = idx % B, c = idx / B;
      Vs[r * VP + G::pc(c)] = ld(Bt + (size_t)(c0 + c) * ldw + r);
    }
    for (int idx = t; idx < IB * IB; idx += NT) {
      int r = idx % IB, c = idx / IB;
      if (r <= c) Hs[r * TP + c] = ld(Rt + (size_t)(c0 + c) * ldr + c0 + r);
    }
    __syncthreads();
    panel_factor<B, true>(Vs, Hs, tauv, scratch, c0);
    for (int idx = t; idx < B * IB; idx += NT) {
      int r = idx % B, c = idx / B;
      st(Bt + (size_t)(c0 + c) * ldw + r, Vs[r * VP + G::pc(c)]);
    }
    for (int idx = t; idx < IB * IB; idx += NT) {
      int r = idx % IB, c = idx / IB;
      if (r <= c) st(Rt + (size_t)(c0 + c) * ldr + c0 + r, Hs[r * TP + c]);
    }
    if (t < IB) st(tau + (size_t)k * a.mw + (size_t)l * B + c0 + t, tauv[t]);
    __syncthreads();
    build_t<B>(Vs, tauv, Gs, Ts, Gp, 0);
    double* tg = upd_tw<B>(a.Tw, a.wt, l, k, g);
    for (int idx = t; idx < G::TSZ; idx += NT) tg[idx] = Ts[idx];
    const int nstr = (B - c0 - IB) / 16;
    for (int s = w; s < nstr; s += NT / 64) {
      asm volatile("" ::: "memory");  // keep the V-image reads inside the loop (no LICM of ~1k LDS loads)
      const int col = c0 + IB + 16 * s;
      load_strip<B>(X, Bt, ldw, col, 0);
      load_head<B>(H, Rt, ldr, c0, col);
      apply_group<B, true>(Vs, Ts, X, H, 0);
      store_strip<B>(X, Bt, ldw, col, 0);
      store_head<B>(H, Rt, ldr, c0, col);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// One 64-column strip of TSMQR(V = W_lk; R_kj, W_lj): wave_update's DAPP branch. lds: lds_update(B).
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void upd_update(const UpdArgs& a, const Item it, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;

  const int strip = it.ts >> 8, l = it.l, j = it.m, k = it.k;
  const int w = threadIdx.x >> 6;
  const int col = strip * 64 + 16 * w;  // strip column inside the tile
  const bool active = col < B;          // wave-uniform
  const size_t ldr = a.ldr, ldw = a.ldw;
  double X[G::NKS];
  double H[G::NRI];

  const S* Vt = (const S*)a.W + (size_t)k * B * ldw + (size_t)l * B;  // W_lk: V
  S* At = (S*)a.R + (size_t)j * B * ldr + (size_t)k * B;              // R_kj: head rows
  S* Bt = (S*)a.W + (size_t)j * B * ldw + (size_t)l * B;              // W_lj
  if (active) load_strip<B>(X, Bt, ldw, col, 0);
  for (int g = 0; g < NG; ++g) {
    __syncthreads();
    stage_v_ts<B>(Vs, Vt, ldw, g * IB);
    stage_t<B>(Ts, upd_tw<B>(a.Tw, a.wt, l, k, g));
    __syncthreads();
    if (active) {
      load_head<B>(H, At, ldr, g * IB, col);
      apply_group<B, true>(Vs, Ts, X, H, 0);
      store_head<B>(H, At, ldr, g * IB, col);
    }
  }
  if (active) store_strip<B>(X, Bt, ldw, col, 0);
}

// ---------------------------------------------------------------------------------------
// prepare: T_g of every W tile (l,k) from the stored V and taus (apply_t_body's TS branch).
// item = (k * wt + l) * NG + g. lds: lds_apply_t(B) bytes.
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void upd_t_body(const UpdArgs& a, const unsigned item, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;
  double* Gs = Ts + G::TSZ;
  double* tauv = Gs + G::TSZ;
  double* Gp = tauv + IB + 2;
  const int tile = item / NG, g = item % NG, c0 = g * IB;
  const int k = tile / a.wt, l = tile % a.wt;
  const S* tau = (const S*)a.tau;
  const size_t ldw = a.ldw;
  const S* Vt = (const S*)a.W + (size_t)k * B * ldw + (size_t)l * B;
  stage_v_ts<B>(Vs, Vt, ldw, c0);
  if (threadIdx.x < IB) tauv[threadIdx.x] = ld(tau + (size_t)k * a.mw + (size_t)l * B + c0 + threadIdx.x);
  __syncthreads();
  build_t<B>(Vs, tauv, Gs, Ts, Gp, 0);
  double* tg = upd_tw<B>(a.Tw, a.wt, l, k, g);
  for (int idx = threadIdx.x; idx < G::TSZ; idx += NT) tg[idx] = Ts[idx];
}

// ---------------------------------------------------------------------------------------
// apply: [Ctop; Cnew] <- Q_u^T [Ctop; Cnew] (TRANS: k ascending, l ascending) or Q_u (the exact
// reverse). apply_q_body's tsmqr with the head rows in Ctop and the body rows in Cnew; a wave with no
// column below nrhs does no MFMA work but takes part in every barrier of the staging.
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__device__ __forceinline__ void upd_apply_body(const UpdArgs& a, const unsigned strip, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;

  const S* Wm = (const S*)a.W;
  const size_t ldw = a.ldw, ldct = a.ldct, ldcn = a.ldcn;
  const int lane = threadIdx.x & 63, x = lane >> 4, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = strip * 64 + 16 * w, col = col0 + (lane & 15);
  const bool active = col0 < a.nrhs;  // wave-uniform
  const bool on = col < a.nrhs;
  S* Ct = (S*)a.Ctop + (size_t)(active ? col0 : 0) * ldct;
  S* Cn = (S*)a.Cnew + (size_t)(active ? col0 : 0) * ldcn;
  const unsigned cofft = head_off<B, S>(ldct, 0);
  const unsigned coffn = head_off<B, S>(ldcn, 0);
  double X[G::NKS];
  double H[G::NRI];

  auto tsmqr = [&](int l, int k) {
    const S* Vt = Wm + (size_t)k * B * ldw + (size_t)l * B;
    const __amdgpu_buffer_rsrc_t rk = uniform_rsrc(Ct + (size_t)k * B);
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(Cn + (size_t)l * B);
    if (active) load_rows<B, S>(X, rl, coffn, on);
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_vq<B, S, false, !TRANS>(Vs, Vt, ldw, g * IB);
      stage_tq<B, !TRANS>(Ts, upd_tw<B>(a.Tw, a.wt, l, k, g));
      __syncthreads();
      if (active) {
        // (Q: the head rows in reverse — this lane takes the rows of lane row 3 - x)
        const unsigned hoff = cofft + (unsigned)((g * IB + (TRANS ? 0 : 3 - 2 * x)) * (int)sizeof(S));
        load_hrows<B, S, !TRANS>(H, rk, hoff, on);
        apply_group<B, true>(Vs, Ts, X, H, 0);
        store_hrows<B, S, !TRANS>(H, rk, hoff, on);
      }
    }
    if (active) store_rows<B, S>(X, rl, coffn, on);
  };

  if constexpr (TRANS) {
    for (int k = 0; k < a.q; ++k)
      for (int l = 0; l < a.wt; ++l) tsmqr(l, k);
  } else {
    for (int k = a.q - 1; k >= 0; --k)
      for (int l = a.wt - 1; l >= 0; --l) tsmqr(l, k);
  }
}

template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_upd_panel(UpdArgs a) {
  extern __shared__ __align__(16) double lds[];
  upd_panel<B, S>(a, a.items[blockIdx.x], lds);
}
template <int B, typename S>
__global__ __launch_bounds__(NT, 2) void k_upd_update(UpdArgs a) {
  extern __shared__ __align__(16) double lds[];
  upd_update<B, S>(a, a.items[blockIdx.x], lds);
}
template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_upd_t(UpdArgs a) {
  extern __shared__ __align__(16) double lds[];
  upd_t_body<B, S>(a, blockIdx.x, lds);
}
template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT, 2) void k_upd_apply(UpdArgs a) {
  extern __shared__ __align__(16) double lds[];
  upd_apply_body<B, S, TRANS>(a, blockIdx.x, lds);
}

// res[c] <- sqrt(res[c]^2 + |rows 0 .. mw-1 of column c|^2): solve.hip's k_resnorm with the running
// norm folded in — thread t sums the squares of rows t, t + NT, ... in fp64, the fixed tree of
// block_sum, then the old norm's square: the same bits on every run. Unscaled, as tqr_lstsq's norm.
template <typename S>
__global__ __launch_bounds__(NT) void k_upd_resnorm(const S* __restrict__ Bm, size_t ldb, int mw, S* __restrict__ res) {
  __shared__ double red[4];
  const S* c = Bm + (size_t)blockIdx.x * ldb;
  double s = 0.0;
  for (int i = (int)threadIdx.x; i < mw; i += NT) {
    const double v = (double)c[i];
    s = fma(v, v, s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const double r0 = (double)res[blockIdx.x];
    res[blockIdx.x] = (S)sqrt(fma(r0, r0, s));
  }
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
typedef void (*ufn)(UpdArgs);
template <int B, typename S>
static void upd_kernels_of(ufn* kp, ufn* ku, ufn* kt, ufn* kqt, ufn* kqn) {
  *kp = k_upd_panel<B, S>;
  *ku = k_upd_update<B, S>;
  *kt = k_upd_t<B, S>;
  *kqt = k_upd_apply<B, S, true>;
  *kqn = k_upd_apply<B, S, false>;
}

// The schedule: level L holds TSQRT(l,k) with 2k + l == L and the strips of TSMQR(l,j,k), j > k, with
// 2k + l + 1 == L. ip / iu: panel and update items in level order, off_p / off_u the levels' offsets.
static void upd_items(int q, int wt, int b, std::vector<Item>& ip, std::vector<Item>& iu, std::vector<long>& off_p,
                      std::vector<long>& off_u) {
  const int nstrips = (b + 63) / 64;
  const int nlevels = 2 * q + wt - 2;
  ip.clear(); iu.clear(); off_p.clear(); off_u.clear();
  for (int L = 0; L < nlevels; ++L) {
    off_p.push_back((long)ip.size());
    off_u.push_back((long)iu.size());
    for (int k = 0; k < q && 2 * k <= L; ++k) {
      const int l = L - 2 * k;
      if (l < wt) ip.push_back(Item{QRD, l, k, k});
      const int lu = l - 1;
      if (lu >= 0 && lu < wt)
        for (int j = k + 1; j < q; ++j)
          for (int s = 0; s < nstrips; ++s) iu.push_back(Item{DAPP | (s << 8), lu, j, k});
    }
  }
  off_p.push_back((long)ip.size());
  off_u.push_back((long)iu.size());
}

static bool upd_shape_ok(int n, int mw, int b) {
  return valid_b(b) && n > 0 && mw > 0 && n % b == 0 && mw % b == 0;
}
// item counts stay in an int (the host-only calls and the device item lists)
static bool upd_counts_ok(int n, int mw, int b) {
  const long long q = n / b, wt = mw / b, ns = (b + 63) / 64;
  return 2 * q + wt - 2 <= 0x7fffffffLL && q * wt <= 0x7fffffffLL && ns * wt * (q * (q - 1) / 2) <= 0x7fffffffLL &&
         q * wt * (b / (b < 32 ? b : 32)) <= 0x7fffffffLL;
}

}  // namespace tqr

using namespace tqr;

struct tqr_update {
  int n, mw, b, q, wt, dtype;
  size_t es, timg_bytes;           // element size; bytes of one set of T images (q * wt tiles)
  std::vector<long> off_p, off_u;  // per level offsets into the item arrays
  int nlevels = 0;
  bool ready = false;     // the device side below exists (a gfx950 was present at create)
  bool prepared = false;  // the apply's T images hold an update
  Item* d_items_p = nullptr;
  Item* d_items_u = nullptr;
  double* d_Tf = nullptr;  // the factorisation's T images (TSQRT -> its TSMQRs)
  double* d_Ta = nullptr;  // the apply's, from the prepare pass
  hipStream_t sP = nullptr, sU = nullptr;
  hipEvent_t evP = nullptr, evU = nullptr, evStart = nullptr;
  hipEvent_t evPrep = nullptr;  // the last tqr_update_rows / tqr_update_prepare
  hipEvent_t evApply[APPLY_NSLOT] = {};
  hipStream_t slotStream[APPLY_NSLOT] = {};
  int nslot = 0;  // slots holding an apply enqueued since the last rows / prepare
  ufn kp = nullptr, ku = nullptr, kt = nullptr, kqt = nullptr, kqn = nullptr;
  size_t ldsP = 0, ldsU = 0, ldsT = 0, ldsQ = 0;
  std::recursive_mutex mu;  // one enqueue sequence at a time (tqr_update_lstsq holds it over its parts)
};

static int upd_device_init(tqr_update* up, const std::vector<Item>& ip, const std::vector<Item>& iu) {
  if (hipMalloc(&up->d_items_p, std::max<size_t>(1, ip.size()) * sizeof(Item)) != hipSuccess ||
      hipMalloc(&up->d_items_u, std::max<size_t>(1, iu.size()) * sizeof(Item)) != hipSuccess ||
      hipMalloc(&up->d_Tf, up->timg_bytes) != hipSuccess || hipMalloc(&up->d_Ta, up->timg_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return TQR_ENOMEM;
  }
  if (!ip.empty()) HIPCHK(hipMemcpy(up->d_items_p, ip.data(), ip.size() * sizeof(Item), hipMemcpyHostToDevice));
  if (!iu.empty()) HIPCHK(hipMemcpy(up->d_items_u, iu.data(), iu.size() * sizeof(Item), hipMemcpyHostToDevice));
  HIPCHK(hipStreamCreateWithFlags(&up->sP, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&up->sU, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&up->evP, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&up->evU, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&up->evStart, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&up->evPrep, hipEventDisableTiming));
  for (int s = 0; s < APPLY_NSLOT; ++s) HIPCHK(hipEventCreateWithFlags(&up->evApply[s], hipEventDisableTiming));
  dispatch_b(up->b, [&](auto bb) {
    if (up->dtype == TQR_F64) upd_kernels_of<decltype(bb)::value, double>(&up->kp, &up->ku, &up->kt, &up->kqt, &up->kqn);
    else upd_kernels_of<decltype(bb)::value, float>(&up->kp, &up->ku, &up->kt, &up->kqt, &up->kqn);
  });
  up->ldsP = lds_panel(up->b);
  up->ldsU = lds_update(up->b);
  up->ldsT = lds_apply_t(up->b);
  up->ldsQ = lds_apply_q(up->b);
  HIPCHK(hipFuncSetAttribute((const void*)up->kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)up->ldsP));
  HIPCHK(hipFuncSetAttribute((const void*)up->ku, hipFuncAttributeMaxDynamicSharedMemorySize, (int)up->ldsU));
  HIPCHK(hipFuncSetAttribute((const void*)up->kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)up->ldsT));
  HIPCHK(hipFuncSetAttribute((const void*)up->kqt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)up->ldsQ));
  HIPCHK(hipFuncSetAttribute((const void*)up->kqn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)up->ldsQ));
  up->ready = true;
  return TQR_OK;
}

// cs waits for the handle's previous rows / prepare and for every apply enqueued since; mu held
static int upd_wait_all(tqr_update* up, hipStream_t cs) {
  HIPCHK(hipStreamWaitEvent(cs, up->evPrep, 0));
  for (int s = 0; s < up->nslot; ++s) HIPCHK(hipStreamWaitEvent(cs, up->evApply[s], 0));
  up->nslot = 0;
  return TQR_OK;
}

// the T pass into the apply's images on cs, then the handle's event; mu held
static int upd_enqueue_prepare(tqr_update* up, const void* dW, int lddw, const void* dtau_u, hipStream_t cs) {
  UpdArgs a = {};
  a.W = const_cast<void*>(dW); a.tau = const_cast<void*>(dtau_u); a.Tw = up->d_Ta; a.ldw = lddw;
  a.mw = up->mw; a.q = up->q; a.wt = up->wt;
  const unsigned grid = (unsigned)((size_t)up->q * up->wt * (up->b / (up->b < 32 ? up->b : 32)));
  hipLaunchKernelGGL(up->kt, dim3(grid), dim3(NT), up->ldsT, cs, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(up->evPrep, cs));
  up->prepared = true;
  return TQR_OK;
}

// The levels on the two side streams behind evStart (batch.hip's batch_enqueue for one matrix); mu held.
static int upd_enqueue_levels(tqr_update* up, void* dR, int lddr, void* dW, int lddw, void* dtau_u, hipStream_t cs) {
  UpdArgs a = {};
  a.R = dR; a.W = dW; a.tau = dtau_u; a.Tw = up->d_Tf; a.ldr = lddr; a.ldw = lddw;
  a.mw = up->mw; a.q = up->q; a.wt = up->wt;
  HIPCHK(hipEventRecord(up->evStart, cs));
  HIPCHK(hipStreamWaitEvent(up->sP, up->evStart, 0));
  HIPCHK(hipStreamWaitEvent(up->sU, up->evStart, 0));
  HIPCHK(hipEventRecord(up->evP, up->sP));
  HIPCHK(hipEventRecord(up->evU, up->sU));
  for (int L = 0; L < up->nlevels; ++L) {
    const long np = up->off_p[L + 1] - up->off_p[L];
    const long nu = up->off_u[L + 1] - up->off_u[L];
    // each stream waits for the other stream's previous level
    HIPCHK(hipStreamWaitEvent(up->sP, up->evU, 0));
    HIPCHK(hipStreamWaitEvent(up->sU, up->evP, 0));
    if (np) {
      a.items = up->d_items_p + up->off_p[L];
      hipLaunchKernelGGL(up->kp, dim3((unsigned)np), dim3(NT), up->ldsP, up->sP, a);
      HIPCHK(hipGetLastError());
    }
    if (nu) {
      a.items = up->d_items_u + up->off_u[L];
      hipLaunchKernelGGL(up->ku, dim3((unsigned)nu), dim3(NT), up->ldsU, up->sU, a);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(up->evP, up->sP));
    HIPCHK(hipEventRecord(up->evU, up->sU));
  }
  return TQR_OK;
}

static bool upd_rows_args_ok(const tqr_update* up, const void* dR, int lddr, const void* dW, int lddw, const void* dtau_u) {
  return up && dR && dW && dtau_u && lddr >= up->n && lddw >= up->mw && valid_ld(lddr, up->es) && valid_ld(lddw, up->es);
}

extern "C" {

int tqr_update_plan(int n, int mw, int b, int* nlevels, int* npanel, int* nupdate, int* nlaunch) {
  if (!upd_shape_ok(n, mw, b) || !upd_counts_ok(n, mw, b)) return TQR_EINVAL;
  std::vector<Item> ip, iu;
  std::vector<long> off_p, off_u;
  upd_items(n / b, mw / b, b, ip, iu, off_p, off_u);
  int launches = 1;  // the T pass of the prepare that tqr_update_rows ends with
  for (size_t L = 0; L + 1 < off_p.size(); ++L) launches += (off_p[L + 1] > off_p[L]) + (off_u[L + 1] > off_u[L]);
  if (nlevels) *nlevels = (int)off_p.size() - 1;
  if (npanel) *npanel = (int)ip.size();
  if (nupdate) *nupdate = (int)iu.size();
  if (nlaunch) *nlaunch = launches;
  return TQR_OK;
}

int tqr_update_level_items(int n, int mw, int b, int level, int* items, int cap) {
  if (!upd_shape_ok(n, mw, b) || !upd_counts_ok(n, mw, b) || level < 0 || level >= 2 * (n / b) + mw / b - 2 ||
      cap < 0 || (cap > 0 && !items))
    return TQR_EINVAL;
  std::vector<Item> ip, iu;
  std::vector<long> off_p, off_u;
  upd_items(n / b, mw / b, b, ip, iu, off_p, off_u);
  int cnt = 0;
  auto emit = [&](const Item& it) {
    if (cnt < cap) {
      items[4 * cnt] = it.ts; items[4 * cnt + 1] = it.l; items[4 * cnt + 2] = it.m; items[4 * cnt + 3] = it.k;
    }
    ++cnt;
  };
  for (long x = off_p[level]; x < off_p[level + 1]; ++x) emit(ip[x]);
  for (long x = off_u[level]; x < off_u[level + 1]; ++x) emit(iu[x]);
  return cnt;
}

int tqr_update_create(tqr_update** out, int n, int mw, int b, int dtype) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!upd_shape_ok(n, mw, b) || (dtype != TQR_F32 && dtype != TQR_F64) || !valid_ld(n, elem_size(dtype)) ||
      !valid_ld(mw, elem_size(dtype)) || !upd_counts_ok(n, mw, b))
    return TQR_EINVAL;
  tqr_update* up = new (std::nothrow) tqr_update();
  if (!up) return TQR_ENOMEM;
  up->n = n; up->mw = mw; up->b = b; up->q = n / b; up->wt = mw / b; up->dtype = dtype; up->es = elem_size(dtype);
  up->timg_bytes = (size_t)up->q * up->wt * (size_t)(b / (b < 32 ? b : 32)) * timg_doubles(b) * sizeof(double);
  std::vector<Item> ip, iu;
  upd_items(up->q, up->wt, b, ip, iu, up->off_p, up->off_u);
  up->nlevels = (int)up->off_p.size() - 1;
  // without a gfx950 the handle exists, holds no device memory, and every device call returns TQR_ENODEV
  if (current_device_is_gfx950() == TQR_OK) {
    const int st = upd_device_init(up, ip, iu);
    if (st != TQR_OK) { tqr_update_destroy(up); return st; }
  }
  *out = up;
  return TQR_OK;
}

size_t tqr_update_workspace_bytes(const tqr_update* up) { return up ? 2 * up->timg_bytes : 0; }

int tqr_update_rows(tqr_update* up, void* dR, int lddr, void* dW, int lddw, void* dtau_u, void* stream) {
  if (!upd_rows_args_ok(up, dR, lddr, dW, lddw, dtau_u)) return TQR_EINVAL;
  if (!up->ready) return TQR_ENODEV;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::recursive_mutex> lk(up->mu);
  int st = upd_wait_all(up, cs);
  if (st != TQR_OK) return st;
  st = upd_enqueue_levels(up, dR, lddr, dW, lddw, dtau_u, cs);
  // join the side streams, also behind a partly failed enqueue: the next call stays ordered after
  // whatever was enqueued
  const hipError_t e1 = hipStreamWaitEvent(cs, up->evP, 0);
  const hipError_t e2 = hipStreamWaitEvent(cs, up->evU, 0);
  if (st != TQR_OK) {
    (void)hipEventRecord(up->evPrep, cs);
    return st;
  }
  HIPCHK(e1);
  HIPCHK(e2);
  return upd_enqueue_prepare(up, dW, lddw, dtau_u, cs);
}

int tqr_update_prepare(tqr_update* up, const void* dW, int lddw, const void* dtau_u, void* stream) {
  if (!up || !dW || !dtau_u || lddw < up->mw || !valid_ld(lddw, up->es)) return TQR_EINVAL;
  if (!up->ready) return TQR_ENODEV;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::recursive_mutex> lk(up->mu);
  const int st = upd_wait_all(up, cs);
  if (st != TQR_OK) return st;
  return upd_enqueue_prepare(up, dW, lddw, dtau_u, cs);
}

int tqr_update_apply_q(tqr_update* up, int trans, const void* dW, int lddw, void* dCtop, int lddct, void* dCnew, int lddcn,
                       int nrhs, void* stream) {
  if (!up || !dW || !dCtop || !dCnew || nrhs < 1 || lddw < up->mw || lddct < up->n || lddcn < up->mw ||
      !valid_ld(lddw, up->es) || !valid_ld(lddct, up->es) || !valid_ld(lddcn, up->es) ||
      (trans != TQR_NOTRANS && trans != TQR_TRANS))
    return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::recursive_mutex> lk(up->mu);
  if (!up->prepared) return TQR_EINVAL;
  // cs waits for the last rows / prepare; the apply is recorded in the event slot of cs
  HIPCHK(hipStreamWaitEvent(cs, up->evPrep, 0));
  int slot = 0;
  while (slot < up->nslot && up->slotStream[slot] != cs) ++slot;
  if (slot == APPLY_NSLOT) {  // more streams than slots: queue behind slot 0's apply and take it over
    slot = 0;
    HIPCHK(hipStreamWaitEvent(cs, up->evApply[0], 0));
  }
  UpdArgs a = {};
  a.W = const_cast<void*>(dW); a.Tw = up->d_Ta; a.Ctop = dCtop; a.Cnew = dCnew;
  a.ldw = lddw; a.ldct = lddct; a.ldcn = lddcn; a.mw = up->mw; a.q = up->q; a.wt = up->wt; a.nrhs = nrhs;
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  hipLaunchKernelGGL(trans == TQR_TRANS ? up->kqt : up->kqn, dim3(grid), dim3(NT), up->ldsQ, cs, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(up->evApply[slot], cs));
  up->slotStream[slot] = cs;
  if (slot == up->nslot) up->nslot = slot + 1;
  return TQR_OK;
}

int tqr_update_lstsq(tqr_update* up, void* dR, int lddr, void* dW, int lddw, void* dtau_u, void* dD, int lddd, void* dBnew,
                     int lddb, int nrhs, void* dX, int lddx, void* dres, void* stream) {
  if (!upd_rows_args_ok(up, dR, lddr, dW, lddw, dtau_u) || !dD || !dBnew || !dX || nrhs < 1 || lddd < up->n ||
      lddx < up->n || lddb < up->mw || !valid_ld(lddd, up->es) || !valid_ld(lddx, up->es) || !valid_ld(lddb, up->es))
    return TQR_EINVAL;
  if (!up->ready) return TQR_ENODEV;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::recursive_mutex> lk(up->mu);
  int st;
  if ((st = tqr_update_rows(up, dR, lddr, dW, lddw, dtau_u, stream)) != TQR_OK) return st;
  if ((st = tqr_update_apply_q(up, TQR_TRANS, dW, lddw, dD, lddd, dBnew, lddb, nrhs, stream)) != TQR_OK) return st;
  if (dX != dD)
    HIPCHK(hipMemcpy2DAsync(dX, (size_t)lddx * up->es, dD, (size_t)lddd * up->es, (size_t)up->n * up->es, (size_t)nrhs,
                            hipMemcpyDeviceToDevice, cs));
  if ((st = tqr_trsm_r(up->dtype, TQR_NOTRANS, up->n, up->b, dR, lddr, dX, nrhs, lddx, stream)) != TQR_OK) return st;
  if (dres) {
    if (up->dtype == TQR_F64)
      hipLaunchKernelGGL(k_upd_resnorm<double>, dim3((unsigned)nrhs), dim3(NT), 0, cs, (const double*)dBnew, (size_t)lddb,
                         up->mw, (double*)dres);
    else
      hipLaunchKernelGGL(k_upd_resnorm<float>, dim3((unsigned)nrhs), dim3(NT), 0, cs, (const float*)dBnew, (size_t)lddb,
                         up->mw, (float*)dres);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

void tqr_update_destroy(tqr_update* up) {
  if (!up) return;
  // the last calls may still be using the workspace and the side streams
  if (up->evPrep) (void)hipEventSynchronize(up->evPrep);
  for (hipEvent_t e : up->evApply)
    if (e) (void)hipEventSynchronize(e);
  if (up->sP) (void)hipStreamSynchronize(up->sP);
  if (up->sU) (void)hipStreamSynchronize(up->sU);
  if (up->d_items_p) (void)hipFree(up->d_items_p);
  if (up->d_items_u) (void)hipFree(up->d_items_u);
  if (up->d_Tf) (void)hipFree(up->d_Tf);
  if (up->d_Ta) (void)hipFree(up->d_Ta);
  if (up->sP) (void)hipStreamDestroy(up->sP);
  if (up->sU) (void)hipStreamDestroy(up->sU);
  for (hipEvent_t e : {up->evP, up->evU, up->evStart, up->evPrep})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : up->evApply)
    if (e) (void)hipEventDestroy(e);
  delete up;
}

}  // extern "C"
