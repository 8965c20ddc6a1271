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

}  // namespace tqr
