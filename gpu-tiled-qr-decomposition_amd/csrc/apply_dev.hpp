// Device helpers of the apply of Q / Q^T, shared by its two kernels: apply.hip's k_apply_q (one
// workgroup per strip) and apply_pipe.hip's k_apply_q_pipe (one workgroup per strip and step).
// Both stage the same V and T images and run the same apply_group calls on the same operands in the
// same order, so they compute the same bits.
#pragma once
#include "tiles.hpp"

namespace tqr {

struct ApplyArgs {
  const void* A;    // factorised matrix (S*): R, GEQRT V, TSQRT V_B
  const void* tau;  // compact tau (S*), m x kmax (prepare only)
  void* C;          // m x nrhs (S*)
  double* Tw;       // T images: [(tile (l,k)) * NG + g][TIMG], tiles l >= k only
  long lda, ldc;
  int m, p, kmax, nrhs;
};

// index of tile (l,k), l >= k, among the stored tiles: panel k's p - k tiles follow panel k-1's
__host__ __device__ inline size_t tile_slot(int l, int k, int p) {
  return (size_t)((long long)k * p - (long long)k * (k - 1) / 2 + (l - k));
}
template <int B>
__device__ __forceinline__ double* tg_ptr(const ApplyArgs& a, int l, int k, int g) {
  using G = Geo<B>;
  return a.Tw + (tile_slot(l, k, a.p) * G::NG + g) * G::TIMG;
}

// ---------------------------------------------------------------------------------------
// Strip / head traffic of C with ragged column counts: a lane whose column is >= nrhs (`on`
// false) loads zeros and stores nothing. The accesses go through a buffer resource based at
// the wave's first column of the row tile (wave-uniform, SGPRs) and one per-lane 32-bit byte
// offset (tiles.hpp head_off; 16 columns: below 2^30 by the leading-dimension bound), as the
// engine's *_buf helpers take them — a 64-bit pointer per lane and per tile costs the registers
// the strip needs at b = 256. AUX is the cache policy of those helpers. k_apply_q takes the
// default: nothing is handed to another workgroup, and the head rows are re-read by the next
// tile of the step. k_apply_q_pipe takes sc1 throughout.
// ---------------------------------------------------------------------------------------
template <int B, typename S, int AUX = 0>
__device__ __forceinline__ void load_rows(double (&X)[Geo<B>::NKS], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  if (on) {
    load_strip_buf<B, S, AUX>(X, rs, off, 0);
  } else {
#pragma unroll
    for (int ks = 0; ks < Geo<B>::NKS; ++ks) X[ks] = 0.0;
  }
}
template <int B, typename S, int AUX = 0>
__device__ __forceinline__ void store_rows(const double (&X)[Geo<B>::NKS], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  if (on) store_strip_buf<B, S, AUX>(X, rs, off, 0);
}
// Head rows of a group. REV (see stage_tq): register r of lane row x holds head row IB-1 - (4r + x)
// = 4 (NRI-1-r) + (3 - x): `off` is then the offset of lane row 3 - x, and the registers swap ends.
template <int B, typename S, bool REV, int AUX = 0>
__device__ __forceinline__ void load_hrows(double (&H)[Geo<B>::NRI], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  constexpr int NRI = Geo<B>::NRI;
  if (on) {
    double t[NRI];
    load_head_buf<B, S, AUX>(t, rs, off);
#pragma unroll
    for (int r = 0; r < NRI; ++r) H[r] = t[REV ? NRI - 1 - r : r];
  } else {
#pragma unroll
    for (int r = 0; r < NRI; ++r) H[r] = 0.0;
  }
}
template <int B, typename S, bool REV, int AUX = 0>
__device__ __forceinline__ void store_hrows(const double (&H)[Geo<B>::NRI], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  constexpr int NRI = Geo<B>::NRI;
  if (on) {
    double t[NRI];
#pragma unroll
    for (int r = 0; r < NRI; ++r) t[r] = H[REV ? NRI - 1 - r : r];
    store_head_buf<B, S, AUX>(t, rs, off);
  }
}
// ---------------------------------------------------------------------------------------
// The untransposed block reflector I - V T V^T (C <- Q C) on the unchanged apply_group of
// tiles.hpp, which computes W = -M^T Z from the UPPER triangle of the T image M (k-blocks k2 <= wi):
// Q needs W = -T Z, whose operand T^T is lower triangular. Relabel the group's IB reflectors in
// reverse order (J = the reversal permutation): the images hold V' = V J and M = J T^T J, which is
// upper triangular again, and the head rows are taken in reverse, H' = J H. Then Z' = H' + V'^T X =
// J Z, W' = -M^T Z' = -J T Z = J W, H' + W' = J (H + W) and X + V' W' = X + V W: the same MFMA
// stream and count as Q^T (no zero half of a full square), nothing new in tiles.hpp. REV selects it.
// ---------------------------------------------------------------------------------------
// T image of a group into LDS: as stored, or (REV) M[i][j] = T[IB-1-j][IB-1-i]
template <int B, bool REV>
__device__ __forceinline__ void stage_tq(double* Ts, const double* __restrict__ tg) {
  using g = Geo<B>;
  const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(tg);
  for (int idx = threadIdx.x; idx < g::IB * g::IB; idx += NT) {
    const int r = idx / g::IB, c = idx % g::IB;
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (unsigned)((r * g::TP + c) * sizeof(double)), 0, 0);
    Ts[REV ? (g::IB - 1 - c) * g::TP + (g::IB - 1 - r) : r * g::TP + c] = dbl_of(v[0], v[1]);
  }
}
// V image of group c0 / IB of a tile (tiles.hpp stage_v_ts / stage_v_ge: the same image; REV: its
// columns in reverse order) read through a buffer resource based at the group's first column,
// 32-bit offsets over its <= 32 columns (the leading-dimension bound) — per-lane 64-bit pointers
// that advance with the tile loops cost the registers the strip needs at b = 256. GE: every
// element of the tile column is loaded (R on and above the diagonal too: in range) and replaced
// by the explicit unit-lower trapezoid's 0 / 1.
template <int B, typename S, bool GE, bool REV>
__device__ __forceinline__ void stage_vq(double* Vs, const S* __restrict__ vt, size_t ldm, int c0) {
  using g = Geo<B>;
  const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(vt + (size_t)c0 * ldm);
#pragma unroll 8
  for (int idx = threadIdx.x; idx < B * g::IB; idx += NT) {
    const int r = idx % B, c = idx / B, d = c0 + c;
    const unsigned off = (unsigned)(((size_t)c * ldm + r) * sizeof(S));
    double v;
    if constexpr (sizeof(S) == 8) {
      const auto u = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
      v = dbl_of(u[0], u[1]);
    } else {
      v = (double)__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
    }
    if (GE) v = r < d ? 0.0 : (r == d ? 1.0 : v);
    Vs[r * g::VP + g::pc(REV ? g::IB - 1 - c : c)] = v;
  }
}

// ---------------------------------------------------------------------------------------
// The bodies of the two whole-factorisation kernels, on resolved arguments: apply.hip's k_apply_t /
// k_apply_q call them with blockIdx.x, apply_batch_dev.hpp's k_apply_t_batch / k_apply_q_batch (tsqr.hip,
// batch_apply.hip) with the base pointers of member blockIdx.y — the same code on the same operands, so
// the same bits.
// ---------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------
// prepare: T_g of every GEQRT tile (k,k) and TSQRT tile (l,k), row-major IB x TP images
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void apply_t_body(const ApplyArgs& a, const unsigned item, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;
  double* Gs = Ts + G::TSZ;
  double* tauv = Gs + G::TSZ;
  double* Gp = tauv + IB + 2;
  // item = slot(l,k) * NG + g; (uniform) search of the panel the slot belongs to
  int t = item / NG, k = 0;
  while (t >= a.p - k) {
    t -= a.p - k;
    ++k;
  }
  const int l = k + t, g = item % NG, c0 = g * IB;
  const bool ge = l == k;
  const S* A = (const S*)a.A;
  const S* tau = (const S*)a.tau;
  const size_t ldm = a.lda;
  const S* Vt = A + (size_t)k * B * ldm + (size_t)l * B;
  if (ge) stage_v_ge<B>(Vs, Vt, ldm, c0);
  else stage_v_ts<B>(Vs, Vt, ldm, c0);
  if (threadIdx.x < IB) tauv[threadIdx.x] = ld(tau + (size_t)k * a.m + (size_t)l * B + c0 + threadIdx.x);
  __syncthreads();
  build_t<B>(Vs, tauv, Gs, Ts, Gp, ge ? c0 / 4 : 0);
  double* tg = tg_ptr<B>(a, l, k, g);
  for (int idx = threadIdx.x; idx < G::TSZ; idx += NT) tg[idx] = Ts[idx];
}

// ---------------------------------------------------------------------------------------
// apply: C <- Q^T C (TRANS) or C <- Q C. The workgroup of `strip` owns columns 64 strip ..
// + 63, wave w its 16w .. 16w + 15. A wave with no column below nrhs does no MFMA work but
// takes part in every barrier of the staging.
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__device__ __forceinline__ void apply_q_body(const ApplyArgs& a, const unsigned strip, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;

  const S* A = (const S*)a.A;
  const size_t lda = a.lda, ldc = a.ldc;
  // (readfirstlane: the wave index and what derives from it — the wave's C pointer — in SGPRs)
  const int lane = threadIdx.x & 63, x = lane >> 4, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = strip * 64 + 16 * w, col = col0 + (lane & 15);
  const bool active = col0 < a.nrhs;  // wave-uniform
  const bool on = col < a.nrhs;
  // the wave's 16 columns of C (an idle wave's pointer is never used) and the lane's byte offset
  // of (row x, its column) in them
  S* Cw = (S*)a.C + (size_t)(active ? col0 : 0) * ldc;
  const unsigned coff = head_off<B, S>(ldc, 0);
  double X[G::NKS];
  double H[G::NRI];

  // UNMQR of tile (k,k) on C_k: groups ascending (Q^T) / descending (Q)
  auto unmqr = [&](int k) {
    const S* Vt = A + (size_t)k * B * lda + (size_t)k * B;
    const __amdgpu_buffer_rsrc_t rk = uniform_rsrc(Cw + (size_t)k * B);
    if (active) load_rows<B, S>(X, rk, coff, on);
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_vq<B, S, true, !TRANS>(Vs, Vt, lda, g * IB);
      stage_tq<B, !TRANS>(Ts, tg_ptr<B>(a, k, k, g));
      __syncthreads();
      if (active) apply_group<B, false>(Vs, Ts, X, H, g * IB / 4);
    }
    if (active) store_rows<B, S>(X, rk, coff, on);
  };
  // TSMQR of tile (l,k) on [C_k; C_l]: C_l's strip stays in registers over the groups, the 32
  // head rows of C_k are loaded and stored per group
  auto tsmqr = [&](int l, int k) {
    const S* Vt = A + (size_t)k * B * lda + (size_t)l * B;
    const __amdgpu_buffer_rsrc_t rk = uniform_rsrc(Cw + (size_t)k * B);
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(Cw + (size_t)l * B);
    if (active) load_rows<B, S>(X, rl, coff, on);
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_vq<B, S, false, !TRANS>(Vs, Vt, lda, g * IB);
      stage_tq<B, !TRANS>(Ts, tg_ptr<B>(a, l, k, g));
      __syncthreads();
      if (active) {
        // (Q: the head rows in reverse — this lane takes the rows of lane row 3 - x)
        const unsigned hoff = coff + (unsigned)((g * IB + (TRANS ? 0 : 3 - 2 * x)) * (int)sizeof(S));
        load_hrows<B, S, !TRANS>(H, rk, hoff, on);
        apply_group<B, true>(Vs, Ts, X, H, 0);
        store_hrows<B, S, !TRANS>(H, rk, hoff, on);
      }
    }
    if (active) store_rows<B, S>(X, rl, coff, on);
  };

  if constexpr (TRANS) {
    for (int k = 0; k < a.kmax; ++k) {
      unmqr(k);
      for (int l = k + 1; l < a.p; ++l) tsmqr(l, k);
    }
  } else {
    for (int k = a.kmax - 1; k >= 0; --k) {
      for (int l = a.p - 1; l > k; --l) tsmqr(l, k);
      unmqr(k);
    }
  }
}

}  // namespace tqr
