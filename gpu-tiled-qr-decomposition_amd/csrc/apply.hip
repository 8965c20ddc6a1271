// Apply Q or Q^T of a finished tiled factorisation to a separate matrix C (include/tqr.h
// "apply"): the ormqr to the plan's geqrf. Single GPU.
//
//   tqr_apply_prepare  k_apply_t: one workgroup per (tile, reflector group) rebuilds the group's
//                      T factor from the stored V and tau (tiles.hpp build_t, as the engine's
//                      k_build_t) into the handle's workspace — once per factorisation.
//   tqr_apply_q        k_apply_q: one 4-wave workgroup per 64 columns of C (a wave owns 16, the
//                      strip layout of the engine's k_update) walks the whole reflector sequence
//                      for its columns: per step k the UNMQR of tile (k,k) on C_k, then the TSMQR
//                      of every tile (l,k), l > k, on [C_k; C_l] — Q^T; the exact reverse for Q.
// The column strips of C are independent, so workgroups never communicate: the only
// synchronisation is the __syncthreads() around the LDS staging of a group's V and T.
// Every element of C is loaded and stored by one lane only (its column's lane with x = row mod
// 4), so the head rows a step stores and the next step reloads are ordered by program order.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

#include "solve.hpp"
#include "tiles.hpp"
#include "tqr.h"

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
// prepare: T_g of every GEQRT tile (k,k) and TSQRT tile (l,k), row-major IB x TP images
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_apply_t(ApplyArgs a) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  extern __shared__ __align__(16) double lds[];
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;
  double* Gs = Ts + G::TSZ;
  double* tauv = Gs + G::TSZ;
  double* Gp = tauv + IB + 2;
  // blockIdx.x = slot(l,k) * NG + g; (uniform) search of the panel the slot belongs to
  int t = blockIdx.x / NG, k = 0;
  while (t >= a.p - k) {
    t -= a.p - k;
    ++k;
  }
  const int l = k + t, g = blockIdx.x % NG, c0 = g * IB;
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
// Strip / head traffic of C with ragged column counts: a lane whose column is >= nrhs (`on`
// false) loads zeros and stores nothing. The accesses go through a buffer resource based at
// the wave's first column of the row tile (wave-uniform, SGPRs) and one per-lane 32-bit byte
// offset (tiles.hpp head_off; 16 columns: below 2^30 by the leading-dimension bound), as the
// engine's *_buf helpers take them — a 64-bit pointer per lane and per tile costs the registers
// the strip needs at b = 256. Default cache policy: nothing is handed to another workgroup, and
// the head rows are re-read by the next tile of the step.
// ---------------------------------------------------------------------------------------
template <int B, typename S>
__device__ __forceinline__ void load_rows(double (&X)[Geo<B>::NKS], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  if (on) {
    load_strip_buf<B, S, 0>(X, rs, off, 0);
  } else {
#pragma unroll
    for (int ks = 0; ks < Geo<B>::NKS; ++ks) X[ks] = 0.0;
  }
}
template <int B, typename S>
__device__ __forceinline__ void store_rows(const double (&X)[Geo<B>::NKS], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  if (on) store_strip_buf<B, S, 0>(X, rs, off, 0);
}
// Head rows of a group. REV (see stage_tq): register r of lane row x holds head row IB-1 - (4r + x)
// = 4 (NRI-1-r) + (3 - x): `off` is then the offset of lane row 3 - x, and the registers swap ends.
template <int B, typename S, bool REV>
__device__ __forceinline__ void load_hrows(double (&H)[Geo<B>::NRI], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  constexpr int NRI = Geo<B>::NRI;
  if (on) {
    double t[NRI];
    load_head_buf<B, S, 0>(t, rs, off);
#pragma unroll
    for (int r = 0; r < NRI; ++r) H[r] = t[REV ? NRI - 1 - r : r];
  } else {
#pragma unroll
    for (int r = 0; r < NRI; ++r) H[r] = 0.0;
  }
}
template <int B, typename S, bool REV>
__device__ __forceinline__ void store_hrows(const double (&H)[Geo<B>::NRI], __amdgpu_buffer_rsrc_t rs, unsigned off, bool on) {
  constexpr int NRI = Geo<B>::NRI;
  if (on) {
    double t[NRI];
#pragma unroll
    for (int r = 0; r < NRI; ++r) t[r] = H[REV ? NRI - 1 - r : r];
    store_head_buf<B, S, 0>(t, rs, off);
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
// apply: C <- Q^T C (TRANS) or C <- Q C. Workgroup blockIdx.x owns columns 64 blockIdx.x ..
// + 63, wave w its 16w .. 16w + 15. A wave with no column below nrhs does no MFMA work but
// takes part in every barrier of the staging.
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT, 2) void k_apply_q(ApplyArgs a) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  extern __shared__ __align__(16) double lds[];
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;

  const S* A = (const S*)a.A;
  const size_t lda = a.lda, ldc = a.ldc;
  // (readfirstlane: the wave index and what derives from it — the wave's C pointer — in SGPRs)
  const int lane = threadIdx.x & 63, x = lane >> 4, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = blockIdx.x * 64 + 16 * w, col = col0 + (lane & 15);
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

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
typedef void (*afn)(ApplyArgs);
template <int B, typename S>
static void apply_kernels(afn* t, afn* qt, afn* qn) {
  *t = k_apply_t<B, S>;
  *qt = k_apply_q<B, S, true>;
  *qn = k_apply_q<B, S, false>;
}
// dynamic LDS (bytes): k_apply_q holds a group's V image and T image (the engine's k_update),
// k_apply_t the V image, T, Gram, taus and four partial Grams (the engine's k_build_t)
static size_t lds_apply_q(int b) {
  const int ib = b < 32 ? b : 32;
  return ((size_t)b * (ib + 2) + (size_t)ib * (ib + 1)) * sizeof(double);
}
static size_t lds_apply_t(int b) {
  const int ib = b < 32 ? b : 32;
  return ((size_t)b * (ib + 2) + 6 * (size_t)ib * (ib + 1) + ib + 2) * sizeof(double);
}
static size_t timg_doubles(int b) {  // Geo<b>::TIMG
  const size_t ib = b < 32 ? b : 32;
  return (ib * (ib + 1) + 127) / 128 * 128;
}
static_assert(Geo<256>::TIMG == 1152 && Geo<16>::TIMG == 384, "host timg_doubles mirrors Geo::TIMG");
static bool apply_valid_b(int b) { return b == 16 || b == 32 || b == 64 || b == 128 || b == 256; }
// the library's leading-dimension bound (include/tqr.h): 32 * ld * sizeof(element) < 2^31
static bool apply_valid_ld(long ld, size_t es) { return ld > 0 && (size_t)32 * (size_t)ld * es <= 0x7fffffffull; }

}  // namespace tqr

using namespace tqr;

// applies of one handle on up to NSLOT distinct streams are tracked one event each, so that a
// later prepare can wait for all of them; further streams share slot 0 (and are ordered behind
// its previous apply)
static constexpr int APPLY_NSLOT = 8;

struct tqr_apply {
  int m, n, b, p, q, kmax, dtype;
  size_t es, ws_bytes;
  double* d_T = nullptr;
  afn kt = nullptr, kqt = nullptr, kqn = nullptr;
  bool prepared = false;
  std::mutex mu;  // the enqueue sequences of prepare / apply_q (event bookkeeping)
  hipEvent_t evPrep = nullptr;
  hipEvent_t evApply[APPLY_NSLOT] = {};
  hipStream_t slotStream[APPLY_NSLOT] = {};
  int nslot = 0;  // slots holding an apply enqueued since the last prepare
};

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "tqr: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return TQR_EHIP;                                                                    \
    }                                                                                     \
  } while (0)

extern "C" {

void tqr_apply_destroy(tqr_apply* ap) {
  if (!ap) return;
  if (ap->d_T) (void)hipFree(ap->d_T);
  if (ap->evPrep) (void)hipEventDestroy(ap->evPrep);
  for (hipEvent_t e : ap->evApply)
    if (e) (void)hipEventDestroy(e);
  delete ap;
}

int tqr_apply_create(tqr_apply** out, int m, int n, int b, int dtype) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!apply_valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || (dtype != TQR_F32 && dtype != TQR_F64) ||
      !apply_valid_ld(m, dtype == TQR_F64 ? 8 : 4))
    return TQR_EINVAL;
  int dev = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) return TQR_ENODEV;
  if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "tqr: device %d is %s, this build targets gfx950 only\n", dev, pr.gcnArchName);
    return TQR_ENODEV;
  }
  tqr_apply* ap = new (std::nothrow) tqr_apply();
  if (!ap) return TQR_ENOMEM;
  ap->m = m; ap->n = n; ap->b = b; ap->p = m / b; ap->q = n / b;
  ap->kmax = ap->p < ap->q ? ap->p : ap->q;
  ap->dtype = dtype;
  ap->es = dtype == TQR_F64 ? 8 : 4;
  const size_t ntiles = tile_slot(ap->kmax, ap->kmax, ap->p);  // tiles (l,k), l >= k, k < kmax
  ap->ws_bytes = ntiles * (size_t)(b / (b < 32 ? b : 32)) * timg_doubles(b) * sizeof(double);
#define TQR_K(BB)                                                                   \
  case BB:                                                                          \
    if (dtype == TQR_F64) apply_kernels<BB, double>(&ap->kt, &ap->kqt, &ap->kqn);   \
    else apply_kernels<BB, float>(&ap->kt, &ap->kqt, &ap->kqn);                     \
    break;
  switch (b) { TQR_K(16) TQR_K(32) TQR_K(64) TQR_K(128) TQR_K(256) }
#undef TQR_K
  if (hipFuncSetAttribute((const void*)ap->kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_t(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)ap->kqt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)ap->kqn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(b)) != hipSuccess) {
    tqr_apply_destroy(ap);
    return TQR_EHIP;
  }
  if (hipMalloc(&ap->d_T, ap->ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    tqr_apply_destroy(ap);
    return TQR_ENOMEM;
  }
  bool ok = hipEventCreateWithFlags(&ap->evPrep, hipEventDisableTiming) == hipSuccess;
  for (int s = 0; ok && s < APPLY_NSLOT; ++s)
    ok = hipEventCreateWithFlags(&ap->evApply[s], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    tqr_apply_destroy(ap);
    return TQR_EHIP;
  }
  *out = ap;
  return TQR_OK;
}

size_t tqr_apply_workspace_bytes(const tqr_apply* ap) { return ap ? ap->ws_bytes : 0; }

int tqr_apply_prepare(tqr_apply* ap, const void* dA, int ldda, const void* dtau, void* stream) {
  if (!ap || !dA || !dtau || ldda < ap->m || !apply_valid_ld(ldda, ap->es)) return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(ap->mu);
  // the workspace is rewritten: wait for every apply enqueued since the last prepare
  for (int s = 0; s < ap->nslot; ++s) HIPCHK(hipStreamWaitEvent(cs, ap->evApply[s], 0));
  ap->nslot = 0;
  ApplyArgs a;
  a.A = dA; a.tau = dtau; a.C = nullptr; a.Tw = ap->d_T; a.lda = ldda; a.ldc = 0;
  a.m = ap->m; a.p = ap->p; a.kmax = ap->kmax; a.nrhs = 0;
  const size_t ng = ap->b / (ap->b < 32 ? ap->b : 32);
  const size_t grid = tile_slot(ap->kmax, ap->kmax, ap->p) * ng;
  if (grid > 0x7fffffffull) return TQR_EINVAL;
  hipLaunchKernelGGL(ap->kt, dim3((unsigned)grid), dim3(NT), lds_apply_t(ap->b), cs, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ap->evPrep, cs));
  ap->prepared = true;
  return TQR_OK;
}

int tqr_apply_q(tqr_apply* ap, int trans, const void* dA, int ldda, void* dC, int nrhs, int lddc, void* stream) {
  if (!ap || !dA || !dC || nrhs < 1 || ldda < ap->m || lddc < ap->m || !apply_valid_ld(ldda, ap->es) ||
      !apply_valid_ld(lddc, ap->es) || (trans != TQR_NOTRANS && trans != TQR_TRANS))
    return TQR_EINVAL;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(ap->mu);
  if (!ap->prepared) return TQR_EINVAL;
  HIPCHK(hipStreamWaitEvent(cs, ap->evPrep, 0));
  int slot = 0;
  while (slot < ap->nslot && ap->slotStream[slot] != cs) ++slot;
  if (slot == APPLY_NSLOT) {  // more streams than slots: queue behind slot 0's apply and take it over
    slot = 0;
    HIPCHK(hipStreamWaitEvent(cs, ap->evApply[0], 0));
  }
  ApplyArgs a;
  a.A = dA; a.tau = nullptr; a.C = dC; a.Tw = ap->d_T; a.lda = ldda; a.ldc = lddc;
  a.m = ap->m; a.p = ap->p; a.kmax = ap->kmax; a.nrhs = nrhs;
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  hipLaunchKernelGGL(trans == TQR_TRANS ? ap->kqt : ap->kqn, dim3(grid), dim3(NT), lds_apply_q(ap->b), cs, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ap->evApply[slot], cs));
  ap->slotStream[slot] = cs;
  if (slot == ap->nslot) ap->nslot = slot + 1;
  return TQR_OK;
}

// Both gels directions on the handle's factorisation (include/tqr.h "solve"): the apply above and
// solve.hip's tqr_trsm_r / resnorm enqueued on `stream`, nothing allocated. The solve reads dA
// only (not the T workspace), so it needs none of the handle's events.
int tqr_lstsq(tqr_apply* ap, int trans, const void* dA, int ldda, void* dB, int nrhs, int lddb, void* dres,
              void* stream) {
  if (!ap || !dA || !dB || nrhs < 1 || ap->m < ap->n || ldda < ap->m || lddb < ap->m || !apply_valid_ld(ldda, ap->es) ||
      !apply_valid_ld(lddb, ap->es) || (trans != TQR_NOTRANS && trans != TQR_TRANS))
    return TQR_EINVAL;
  {
    std::lock_guard<std::mutex> lk(ap->mu);
    if (!ap->prepared) return TQR_EINVAL;
  }
  int st;
  if (trans == TQR_NOTRANS) {
    // B <- Q^T B; rows 0 .. n-1 <- R^{-1} of them; the residual norms from rows n .. m-1
    if ((st = tqr_apply_q(ap, TQR_TRANS, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
    if ((st = tqr_trsm_r(ap->dtype, TQR_NOTRANS, ap->n, ap->b, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
    return dres ? resnorm(ap->dtype, dB, lddb, ap->n, ap->m, nrhs, dres, stream) : TQR_OK;
  }
  // x = Q [R^{-T} c; 0]
  if (ap->m > ap->n)
    HIPCHK(hipMemset2DAsync((char*)dB + (size_t)ap->n * ap->es, (size_t)lddb * ap->es, 0, (size_t)(ap->m - ap->n) * ap->es,
                            (size_t)nrhs, (hipStream_t)stream));
  if ((st = tqr_trsm_r(ap->dtype, TQR_TRANS, ap->n, ap->b, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
  return tqr_apply_q(ap, TQR_NOTRANS, dA, ldda, dB, nrhs, lddb, stream);
}

}  // extern "C"
