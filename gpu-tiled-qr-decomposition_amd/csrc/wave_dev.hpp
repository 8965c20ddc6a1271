// The wave engine's two kernel bodies and what its host side derives from the BFS wave plan, shared by
// the wave engine itself (engine.hip: k_panel / k_update, one matrix per launch) and the strided-batched
// factorisation (batch.hip: k_panel_batch / k_update_batch, blockIdx.y = the matrix). One body, so a
// batch member has the bits of a wave plan executed on it alone (include/tqr.h "batched").
//
//   wave_panel   one GEQRT (QRS) or TSQRT (QRD) task per 256-thread workgroup;
//   wave_update  one 64-column strip of one UNMQR (SAPP) / TSMQR (DAPP) task per workgroup;
//   wave_items   the item lists of the waves (panel items, update strip items, per-wave offsets);
//   lds_panel / lds_update / wave_tw_bytes: the kernels' dynamic LDS and a matrix's T workspace.
// Both bodies take resolved base pointers — the matrix, its compact tau, its T workspace — so a caller
// offsets them per matrix in 64 bits; inside a matrix the offsets are the engine's (tiles.hpp).
// The host side is also what plans.hip (a plan's wave items and workspace) and tileapi.hip (the LDS
// sizes of the kernels engine.hip's resolve hands them) include this header for.
// STAMP / STAMP_INIT: the `stamps` diagnostic build of engine.hip defines them before it includes this
// header; everywhere else they are empty.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "flow_list.hpp"
#include "gridscheduler.h"
#include "tiles.hpp"

#ifndef STAMP
#define STAMP_INIT
#define STAMP(i) do {} while (0)
#endif

namespace tqr {

// T image of reflector group g of tile (i, k) in a matrix's T workspace: [(k*p + i)*NG + g][TIMG]
template <int B>
__device__ __forceinline__ double* wave_tw(double* Tw, int p, int i, int k, int g) {
  using G = Geo<B>;
  return Tw + (((size_t)k * p + i) * G::NG + g) * G::TIMG;
}

// ---------------------------------------------------------------------------------------
// Panel body: GEQRT (QRS) and TSQRT (QRD) tasks, one workgroup each. lds: lds_panel(B) bytes.
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void wave_panel(S* A, S* tau, double* Tw, const Item it, size_t ldm, int m, int p, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, VP = G::VP, TP = G::TP, NG = G::NG;
  double* Vs = lds;
  double* Hs = Vs + G::VSZ;
  double* Ts = Hs + G::TSZ;
  double* Gs = Ts + G::TSZ;
  double* tauv = Gs + G::TSZ;
  double* scratch = tauv + IB + 2;
  double* Gp = scratch + 2 * 4 * 32 + 4 * 32 + 2 * 32 + G::TSZ;  // 4 partial Grams

  const int type = it.ts & 0xff, l = it.l, k = it.k;
  const int t = threadIdx.x, w = t >> 6;
  S* Rt = A + (size_t)k * B * ldm + (size_t)k * B;  // tile (k,k)
  double X[G::NKS];
  double H[G::NRI];

  if (type == QRS) {
    for (int g = 0; g < NG; ++g) {
      const int c0 = g * IB, ks0 = c0 / 4;
#pragma unroll 8
      for (int idx = t; idx < B * IB; idx += NT) {
        int r = idx % B, c = idx / B;
        Vs[r * VP + G::pc(c)] = r >= c0 ? ld(Rt + (size_t)(c0 + c) * ldm + r) : 0.0;
      }
      __syncthreads();
      panel_factor<B, false>(Vs, Hs, tauv, scratch, c0);
      // write back R / V of the panel, taus; then make V explicit (0 above, 1 on the diagonal)
      for (int idx = t; idx < B * IB; idx += NT) {
        int r = idx % B, c = idx / B, d = c0 + c;
        double v = Vs[r * VP + G::pc(c)];
        if (r >= c0) st(Rt + (size_t)d * ldm + r, v);
      }
      if (t < IB) st(tau + (size_t)k * m + (size_t)k * B + c0 + t, tauv[t]);
      __syncthreads();
      for (int idx = t; idx < B * IB; idx += NT) {
        int r = idx % B, c = idx / B, d = c0 + c;
        if (r <= d) Vs[r * VP + G::pc(c)] = r == d ? 1.0 : 0.0;
      }
      __syncthreads();
      build_t<B>(Vs, tauv, Gs, Ts, Gp, ks0);
      double* tg = wave_tw<B>(Tw, p, k, k, g);
      for (int idx = t; idx < G::TSZ; idx += NT) tg[idx] = Ts[idx];
      // trailing columns of the tile
      const int nstr = (B - c0 - IB) / 16;
      for (int s = w; s < nstr; s += NT / 64) {
        asm volatile("" ::: "memory");  // keep the V-image reads inside the loop (no LICM of ~1k LDS loads)
        const int col = c0 + IB + 16 * s;
        load_strip<B>(X, Rt, ldm, col, ks0);
        apply_group<B, false>(Vs, Ts, X, H, ks0);
        store_strip<B>(X, Rt, ldm, col, ks0);
      }
      __syncthreads();
    }
  } else {  // QRD: TSQRT of [R_kk ; tile (l,k)]
    S* Bt = A + (size_t)k * B * ldm + (size_t)l * B;
    STAMP_INIT
    for (int g = 0; g < NG; ++g) {
      const int c0 = g * IB;
#pragma unroll 8
      for (int idx = t; idx < B * IB; idx += NT) {
        int r = idx % B, c = idx / B;
        Vs[r * VP + G::pc(c)] = ld(Bt + (size_t)(c0 + c) * ldm + r);
      }
      for (int idx = t; idx < IB * IB; idx += NT) {
        int r = idx % IB, c = idx / IB;
        if (r <= c) Hs[r * TP + c] = ld(Rt + (size_t)(c0 + c) * ldm + c0 + r);
      }
      __syncthreads();
      STAMP(0);
      panel_factor<B, true>(Vs, Hs, tauv, scratch, c0);
      STAMP(1);
      for (int idx = t; idx < B * IB; idx += NT) {
        int r = idx % B, c = idx / B;
        st(Bt + (size_t)(c0 + c) * ldm + r, Vs[r * VP + G::pc(c)]);
      }
      for (int idx = t; idx < IB * IB; idx += NT) {
        int r = idx % IB, c = idx / IB;
        if (r <= c) st(Rt + (size_t)(c0 + c) * ldm + c0 + r, Hs[r * TP + c]);
      }
      if (t < IB) st(tau + (size_t)k * m + (size_t)l * B + c0 + t, tauv[t]);
      __syncthreads();
      STAMP(2);
      build_t<B>(Vs, tauv, Gs, Ts, Gp, 0);
      STAMP(3);
      double* tg = wave_tw<B>(Tw, p, l, k, g);
      for (int idx = t; idx < G::TSZ; idx += NT) tg[idx] = Ts[idx];
      const int nstr = (B - c0 - IB) / 16;
      for (int s = w; s < nstr; s += NT / 64) {
        asm volatile("" ::: "memory");  // keep the V-image reads inside the loop (no LICM of ~1k LDS loads)
        const int col = c0 + IB + 16 * s;
        load_strip<B>(X, Bt, ldm, col, 0);
        load_head<B>(H, Rt, ldm, c0, col);
        apply_group<B, true>(Vs, Ts, X, H, 0);
        store_strip<B>(X, Bt, ldm, col, 0);
        store_head<B>(H, Rt, ldm, c0, col);
      }
      __syncthreads();
      STAMP(4);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Update body: UNMQR (SAPP) and TSMQR (DAPP) on one 64-column strip, one workgroup each;
// wave w owns columns strip*64 + 16w .. +15 of the target tile(s). lds: lds_update(B) bytes.
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void wave_update(S* A, double* Tw, const Item it, size_t ldm, int p, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;

  const int type = it.ts & 0xff, strip = it.ts >> 8, l = it.l, j = it.m, k = it.k;
  const int w = threadIdx.x >> 6;
  const int col = strip * 64 + 16 * w;  // strip column inside the tile
  const bool active = col < B;
  double X[G::NKS];
  double H[G::NRI];

  if (type == DAPP) {
    const S* Vt = A + (size_t)k * B * ldm + (size_t)l * B;  // tile (l,k): V_B
    S* At = A + (size_t)j * B * ldm + (size_t)k * B;        // tile (k,j): head rows
    S* Bt = A + (size_t)j * B * ldm + (size_t)l * B;        // tile (l,j)
    if (active) load_strip<B>(X, Bt, ldm, col, 0);
    for (int g = 0; g < NG; ++g) {
      __syncthreads();
      stage_v_ts<B>(Vs, Vt, ldm, g * IB);
      stage_t<B>(Ts, wave_tw<B>(Tw, p, l, k, g));
      __syncthreads();
      if (active) {
        load_head<B>(H, At, ldm, g * IB, col);
        apply_group<B, true>(Vs, Ts, X, H, 0);
        store_head<B>(H, At, ldm, g * IB, col);
      }
    }
    if (active) store_strip<B>(X, Bt, ldm, col, 0);
  } else {  // SAPP
    const S* Vt = A + (size_t)k * B * ldm + (size_t)k * B;  // tile (k,k)
    S* Ct = A + (size_t)j * B * ldm + (size_t)k * B;        // tile (k,j)
    if (active) load_strip<B>(X, Ct, ldm, col, 0);
    for (int g = 0; g < NG; ++g) {
      __syncthreads();
      stage_v_ge<B>(Vs, Vt, ldm, g * IB);
      stage_t<B>(Ts, wave_tw<B>(Tw, p, k, k, g));
      __syncthreads();
      if (active) apply_group<B, false>(Vs, Ts, X, H, g * IB / 4);
    }
    if (active) store_strip<B>(X, Ct, ldm, col, 0);
  }
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
static inline size_t lds_panel(int b) {
  int ib = b < 32 ? b : 32;
  size_t d = (size_t)b * (ib + 2) + 8 * (size_t)ib * (ib + 1) + (ib + 2) + 2 * 4 * 32 + 4 * 32 + 2 * 32;
  return d * sizeof(double);
}
static inline size_t lds_update(int b) {
  int ib = b < 32 ? b : 32;
  return ((size_t)b * (ib + 2) + (size_t)ib * (ib + 1)) * sizeof(double);
}

// bytes of one matrix's T workspace: a Geo<b>::TIMG image per reflector group of every tile (i, k), k < kmax
static inline size_t wave_tw_bytes(int p, int kmax, int b) {
  const size_t ib = b < 32 ? b : 32;
  const size_t timg = (ib * (ib + 1) + 127) / 128 * 128;
  return (size_t)p * kmax * (b / ib) * timg * sizeof(double);
}
static_assert(Geo<256>::TIMG == 1152 && Geo<16>::TIMG == 384, "wave_tw_bytes mirrors Geo::TIMG");

// The waves of the reference DAG on a p x q tile grid (sched.c's BFS levels) as the kernels' items:
// wave L's panel tasks are ip[off_p[L] .. off_p[L+1]), its update tasks — one item per 64-column strip
// of the tile, the strip in bits 8.. of the type word — iu[off_u[L] .. off_u[L+1]). False: no memory.
static inline bool wave_items(int p, int q, int b, std::vector<Item>& ip, std::vector<Item>& iu, std::vector<long>& off_p,
                              std::vector<long>& off_u) {
  tqr_plan_t sp;
  if (tqr_sched_plan(p, q, &sp) != 0) return false;
  const int nstrips = (b + 63) / 64;
  ip.clear(); iu.clear(); off_p.clear(); off_u.clear();
  ip.reserve(sp.ntasks);
  iu.reserve(sp.ntasks * nstrips);
  for (int L = 0; L < sp.nlevels; ++L) {
    off_p.push_back((long)ip.size());
    off_u.push_back((long)iu.size());
    for (long x = sp.level_off[L]; x < sp.level_off[L + 1]; ++x) {
      const int* tk = sp.tasks + 4 * x;
      if (tk[0] == QRS || tk[0] == QRD) {
        ip.push_back(Item{tk[0], tk[1], tk[2], tk[3]});
      } else {
        for (int s = 0; s < nstrips; ++s) iu.push_back(Item{tk[0] | (s << 8), tk[1], tk[2], tk[3]});
      }
    }
  }
  off_p.push_back((long)ip.size());
  off_u.push_back((long)iu.size());
  tqr_sched_plan_free(&sp);
  return true;
}

}  // namespace tqr
