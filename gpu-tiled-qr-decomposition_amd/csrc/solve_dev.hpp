// Device helpers of the triangular solve with R, shared by its kernels: solve.hip's k_trsm_r (one
// workgroup per strip), batch_apply.hip's k_trsm_r_batch (the same body, trsm_r_body below, per strip and
// batch member) and solve_pipe.hip's k_trsm_r_pipe (one workgroup per strip and tile row).
// All build the same operand images and run the same substitution, so they compute the same bits.
#pragma once
#include "tiles.hpp"

namespace tqr {

// ---------------------------------------------------------------------------------------
// Operand image of 32 target rows (group g of a tile row; b < 32: the tile's b rows) in the LDS V
// layout of tiles.hpp (b x VP doubles, column permutation pc), negated, so that accum_z forms
//   Z = H + V^T X_k = H - (the group's rows of op(R) tile) X_k :
//   TR  (X <- R^{-1} X):  V[kk][c] = -tile(g IB + c, kk)   — the group's 32 rows, transposed;
//   !TR (X <- R^{-T} X):  V[kk][c] = -tile(kk, g IB + c)   — the group's 32 columns as stored.
// The tile is read in IB x IB chunks kc0 <= kc < kc1 of the k index through a buffer resource
// based at the chunk (32-bit offsets over <= 32 columns: the leading-dimension bound), 32
// consecutive lanes on 32 consecutive elements of a column. DIAG (tile (k,k)): an element below
// the diagonal — the GEQRT V, whatever it holds — becomes 0 by a select.
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TR, bool DIAG>
__device__ __forceinline__ void stage_r(double* Vs, const S* __restrict__ rt, size_t ldm, int g, int kc0, int kc1) {
  using G = Geo<B>;
  constexpr int IB = G::IB, PER = IB * IB / NT, SB = G::NG < 4 ? G::NG : 4;
  static_assert(IB * IB % NT == 0, "whole passes of the workgroup over a chunk");
  // SB chunks per batch: all of a batch's loads are issued before its first LDS store (left to the
  // compiler, every load is waited for and stored before the next is issued — one memory round
  // trip per element). A batch that reaches past kc1 repeats the last chunk (the same values to
  // the same places) instead of branching around loads.
  for (int k0 = kc0; k0 < kc1; k0 += SB) {
    double v[SB][PER];
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int kc = k0 + u < kc1 ? k0 + u : kc1 - 1;
      const S* base = TR ? rt + (size_t)kc * IB * ldm + (size_t)g * IB : rt + (size_t)g * IB * ldm + (size_t)kc * IB;
      const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(base);
#pragma unroll
      for (int it = 0; it < PER; ++it) {
        const int idx = it * NT + threadIdx.x;
        const int ar = idx % IB, ac = idx / IB;  // (row, column) inside the chunk as stored
        const unsigned off = (unsigned)(((size_t)ac * ldm + ar) * sizeof(S));
        if constexpr (sizeof(S) == 8) {
          const auto w = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
          v[u][it] = dbl_of(w[0], w[1]);
        } else {
          v[u][it] = (double)__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
        }
      }
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int u = 0; u < SB; ++u) {
      const int kc = k0 + u < kc1 ? k0 + u : kc1 - 1;
#pragma unroll
      for (int it = 0; it < PER; ++it) {
        const int idx = it * NT + threadIdx.x;
        const int ar = idx % IB, ac = idx / IB;
        const int c = TR ? ar : ac, kk = kc * IB + (TR ? ac : ar);
        double e = v[u][it];
        if (DIAG) {
          const int row = TR ? g * IB + c : kk, colm = TR ? kk : g * IB + c;  // element of the tile
          e = row > colm ? 0.0 : e;
        }
        Vs[kk * G::VP + G::pc(c)] = -e;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// The IB x IB diagonal block of a group by substitution, on Z (the group's IB rows of the strip:
// Z[r] at lane row x = row 4r + x, every column on 4 lanes 16 apart). Vd = the image rows of the
// block's own k range: Vd[j][pc(i)] = -D(i, j) (TR) / -D(j, i) (!TR) — the lane of row i = 4r + x
// finds its NRI coefficients of step j contiguous at Vd[j * VP + x * NRI + r].
// Step j (descending for the upper triangle, ascending for its transpose): the lane holding row j
// divides by the diagonal entry itself, the quotient goes to the column's 4 lanes (ds_bpermute),
// and the rows still to be solved take z_i <- z_i - D_ij x_j. Rows already solved, and the
// coefficients on the other side of the diagonal, are excluded by selects (not by a zero factor:
// an inf or NaN there must not leak).
// ---------------------------------------------------------------------------------------
template <int B, bool TRANS>
__device__ __forceinline__ void subst(const double* __restrict__ Vd, double (&Z)[Geo<B>::NRI]) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NRI = G::NRI, VP = G::VP;
  const int lane = threadIdx.x & 63, x = lane >> 4;
  const unsigned vb = lds_base(Vd + x * NRI);
  // the lane's coefficients of step jj: the registers with a row still to be solved (upper triangle:
  // r <= j / 4, its transpose: r >= j / 4), in 16-B reads
  auto ldc = [&](double (&c)[NRI], int jj) {
    const int j = TRANS ? jj : IB - 1 - jj, jr = j >> 2;
    const int r0 = TRANS ? jr : 0, r1 = TRANS ? NRI - 1 : jr;
#pragma unroll
    for (int h = 0; h < NRI / 2; ++h)
      if (2 * h + 1 >= r0 && 2 * h <= r1) {
        const d2v_t t = lds_rd2(vb + (unsigned)((j * VP + 2 * h) * sizeof(double)));
        c[2 * h] = t.x;
        c[2 * h + 1] = t.y;
      }
  };
  double cf[NRI], cn[NRI];
  ldc(cf, 0);
#pragma unroll
  for (int jj = 0; jj < IB; ++jj) {
    // one step per scheduling region, the next step's coefficients read ahead (left free, the
    // scheduler hoists the reads of all IB steps: the chain is serial, the reads are not)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    const int j = TRANS ? jj : IB - 1 - jj, jr = j >> 2, jx = j & 3;
    const int r0 = TRANS ? jr : 0, r1 = TRANS ? NRI - 1 : jr;
    if (jj + 1 < IB) ldc(cn, jj + 1);
    double q = Z[jr] / -cf[jr];  // (lane row jx: z_j / D_jj; the image is negated)
    q = __shfl(q, 16 * jx + (lane & 15));
#pragma unroll
    for (int r = r0; r <= r1; ++r) {
      if (r == jr) Z[r] = x == jx ? q : ((TRANS ? x > jx : x < jx) ? fma(cf[r], q, Z[r]) : Z[r]);
      else Z[r] = fma(cf[r], q, Z[r]);
      // (the update belongs to this step: left to the compiler, the forward direction keeps every
      // step's quotient and coefficients in registers and updates a row only when its turn comes)
      asm volatile("" : "+v"(Z[r]));
    }
#pragma unroll
    for (int r = 0; r < NRI; ++r) cf[r] = cn[r];
  }
}

// Target rows of a tile row (32-bit offsets through the wave's resource, as apply.hip): a lane whose
// column is >= nrhs (`on` false) loads zeros and stores nothing. (Plain loads: the
// rows are the workgroup's own. solve_pipe.hip reads rows other workgroups stored with sc1 loads of
// its own.)
template <int B, typename S>
__device__ __forceinline__ void load_h(double (&H)[Geo<B>::NRI], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  if (on) {
    load_head_buf<B, S, 0>(H, rs, off);
  } else {
#pragma unroll
    for (int r = 0; r < Geo<B>::NRI; ++r) H[r] = 0.0;
  }
}
template <int B, typename S>
__device__ __forceinline__ void load_x(double (&X)[Geo<B>::NKS], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  if (on) {
    load_strip_buf<B, S, 0>(X, rs, off, 0);
  } else {
#pragma unroll
    for (int ks = 0; ks < Geo<B>::NKS; ++ks) X[ks] = 0.0;
  }
}

struct SolveArgs {
  const void* A;  // factorised matrix (S*): R in the upper triangle of the leading n x n block
  void* X;        // n x nrhs (S*)
  long lda, ldx;
  int nt, nrhs;   // nt = n / b tile rows
};

// ---------------------------------------------------------------------------------------
// The body of the whole-solve kernels, on resolved arguments: solve.hip's k_trsm_r calls it with
// blockIdx.x, batch_apply.hip's k_trsm_r_batch with the base pointers of member blockIdx.y: the same
// code on the same operands, so the same bits.
// solve: X <- R^{-T} X (TRANS) or X <- R^{-1} X. The workgroup of `strip` owns columns 64 strip ..
// + 63, wave w its 16w .. 16w + 15. A wave with no column below nrhs does no arithmetic but takes
// part in the staging and in every barrier.
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__device__ __forceinline__ void trsm_r_body(const SolveArgs& a, const int strip, double* lds) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG, NRI = G::NRI, NKS = G::NKS;
  double* Vs = lds;

  const S* A = (const S*)a.A;
  const size_t lda = a.lda, ldx = a.ldx;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = strip * 64 + 16 * w, col = col0 + (lane & 15);
  const bool active = col0 < a.nrhs;  // wave-uniform
  const bool on = col < a.nrhs;
  S* Xw = (S*)a.X + (size_t)(active ? col0 : 0) * ldx;
  const unsigned coff = head_off<B, S>(ldx, 0);
  double X[NKS];

  // tile (k,k) against X_k: per group (descending for R, ascending for R^T) first the groups
  // already solved — Z = X_g - (their columns of the group's rows of op(R)) X, the MFMA product over
  // those k-steps only — then the group's own block by substitution
  auto diag = [&](int k) {
    const S* Rt = A + (size_t)k * B * lda + (size_t)k * B;
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_r<B, S, !TRANS, true>(Vs, Rt, lda, g, TRANS ? 0 : g, TRANS ? g + 1 : NG);
      __syncthreads();
      if (active) {
        // (the group's registers by selects on the uniform g: X stays in registers at any NG)
        double Z[NRI];
#pragma unroll
        for (int r = 0; r < NRI; ++r) Z[r] = X[r];
#pragma unroll
        for (int gg = 1; gg < NG; ++gg)
#pragma unroll
          for (int r = 0; r < NRI; ++r) Z[r] = gg == g ? X[gg * NRI + r] : Z[r];
        accum_z<B>(Vs, X, Z, TRANS ? 0 : (g + 1) * NRI, TRANS ? g * NRI : NKS);
        subst<B, TRANS>(Vs + g * IB * G::VP, Z);
#pragma unroll
        for (int gg = 0; gg < NG; ++gg)
#pragma unroll
          for (int r = 0; r < NRI; ++r) X[gg * NRI + r] = gg == g ? Z[r] : X[gg * NRI + r];
      }
    }
  };
  // X_i -= (tile Rt of op(R)) X_k: per group the 32 target rows are loaded ahead of the staging,
  // updated by one pass of accum_z over the whole strip and stored
  auto update = [&](int i, const S* Rt) {
    const __amdgpu_buffer_rsrc_t ri = uniform_rsrc(Xw + (size_t)i * B);
    for (int g = 0; g < NG; ++g) {
      double H[NRI];
      const unsigned hoff = coff + (unsigned)(g * IB * (int)sizeof(S));
      if (active) load_h<B, S>(H, ri, hoff, on);
      __syncthreads();
      stage_r<B, S, !TRANS, false>(Vs, Rt, lda, g, 0, NG);
      __syncthreads();
      if (active) {
        accum_z<B>(Vs, X, H, 0, NKS);
        if (on) store_head_buf<B, S, 0>(H, ri, hoff);
      }
    }
  };
  auto step = [&](int k) {
    const __amdgpu_buffer_rsrc_t rk = uniform_rsrc(Xw + (size_t)k * B);
    if (active) load_x<B, S>(X, rk, coff, on);
    diag(k);
    if (active) {
      // fp32 storage: the updates use X_k as it is stored
      if constexpr (sizeof(S) == 4) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) X[ks] = (double)(float)X[ks];
      }
      if (on) store_strip_buf<B, S, 0>(X, rk, coff, 0);
    }
  };

  if constexpr (TRANS) {
    for (int k = 0; k < a.nt; ++k) {
      step(k);
      for (int i = k + 1; i < a.nt; ++i) update(i, A + (size_t)i * B * lda + (size_t)k * B);  // R_ki
    }
  } else {
    for (int k = a.nt - 1; k >= 0; --k) {
      step(k);
      for (int i = 0; i < k; ++i) update(i, A + (size_t)k * B * lda + (size_t)i * B);  // R_ik
    }
  }
}

// ---- host side, shared by the two units' launches -----------------------------------------------
// dynamic LDS (bytes): one operand image, b x (IB + 2) doubles (Geo<b>::VSZ)
static inline size_t lds_solve(int b) { return (size_t)b * ((b < 32 ? b : 32) + 2) * sizeof(double); }
static_assert(Geo<256>::VSZ * sizeof(double) == 69632 && Geo<16>::VSZ == 16 * 18, "host lds_solve mirrors Geo::VSZ");

}  // namespace tqr
