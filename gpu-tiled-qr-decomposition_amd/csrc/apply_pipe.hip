// The apply of Q / Q^T spread over workgroups (include/tqr.h "pipelined apply"): the same tile
// operations as apply.hip's k_apply_q on the same operands in the same order, hence the same bits —
// but one workgroup per (64-column strip, step k) instead of one per strip, so a narrow C uses up to
// kmax CUs, not one.
//
// k_apply_q is a two-dimensional wavefront over (step k, row tile l): UNMQR(k) on C_k, then
// TSMQR(l, k) on [C_k; C_l] for l = k+1 .. p-1 (Q^T; the exact reverse for Q). Operation (k, l) needs
// C_k as (k, l-1) left it and C_l as step k-1 (Q: k+1) left it; nothing else touches those rows in
// between. k_apply_q_pipe gives step k of a strip to one workgroup, which runs k_apply_q's own unmqr /
// tsmqr — apply_dev.hpp's images, tiles.hpp's apply_group, group by group, the head rows of C_k loaded
// and stored per group through memory — and waits for C_l row tile by row tile:
//   Q^T, step k:  [wait (k-1, k)]  UNMQR(k);  l = k+1 .. p-1:  [wait (k-1, l)]  TSMQR(l, k)  publish (k, l)
//   Q,   step k:  l = p-1 .. k+1:  [wait (k+1, l)]  TSMQR(l, k)  publish (k, l);  UNMQR(k)  publish (k, k)
// (no wait in the first step of a direction: k = 0, or k = kmax-1). Flag (k, l) says "step k is done
// with C_l"; (k, k), used by Q only, "step k's UNMQR is done", which is when C_k is final for step k-1.
// Every row tile therefore receives the operations of k_apply_q in k_apply_q's order, and passes
// through memory between two of them exactly where it does there (fp32 storage: rounded to float at
// every store), so the critical path is about p + 2 kmax tile operations instead of all of them.
//
// The protocol between the workgroups — tickets, sc1 hand-over, epoch flags, bounded waits — is
// pipe_dev.hpp's. Here a work item is (strip, step) by pipe_ticket_map over the kmax steps, and the only
// producer of (strip, k) is (strip, k-1) for Q^T and (strip, k+1) for Q. Every load and store of C is an
// sc1 access, the workgroup's own rows included: every byte of C was stored or will be loaded by another
// workgroup. V, T and tau come from earlier launches: plain loads.
//
// k_form_q_pipe (tqr_apply_pipe_form_q) is the Q direction of the same on the first ncols columns of an
// identity that is never stored: only the (strip, step) items that meet non-zero data exist
// (form_q_ticket_map), and a row tile's first operation takes the 0 / 1 pattern from registers. Same
// flags, hand-over, bounded waits and handle.
#include <hip/hip_runtime.h>

#include <mutex>
#include <new>

#include "apply.hpp"
#include "apply_dev.hpp"
#include "host_common.hpp"
#include "pipe_dev.hpp"
#include "pipe_host.hpp"
#include "solve.hpp"
#include "tqr.h"

namespace tqr {

// ---------------------------------------------------------------------------------------
// Form Q (tqr_apply_pipe_form_q): Q applied to E = the first ncols columns of I_m, without the work on
// E's zero blocks. Strip s of E (columns 64 s .. min(64 s + 63, ncols - 1)) is non-zero in the row tiles
// jlo(s) .. jhi(s) only, and step k of Q touches the row tiles >= k: the steps k > jhi(s) would turn
// zeros into zeros and are no items. The items are (s, k) with k <= kf(s) = min(jhi(s), kmax - 1) —
// step k has the strips s >= smin(k) = floor(k b / 64), and exists if k b <= ncols - 1.
// ---------------------------------------------------------------------------------------
// steps that have items: k = 0 .. form_q_steps - 1
__host__ __device__ inline int form_q_steps(int kmax, int b, int ncols) {
  const int ka = (ncols - 1) / b + 1;
  return ka < kmax ? ka : kmax;
}
// Work item of ticket t: tickets go step-descending as pipe_ticket_map's for Q, over the active
// strips of each step only — so the one producer of (strip, step), which is (strip, step + 1) where step
// < kf(strip), has a smaller ticket. False: t is no ticket (t >= the item count). The search walks at
// most kmax counts, once per workgroup, in scalar registers that are free again before the tile loops.
__host__ __device__ inline bool form_q_ticket_map(int kmax, int b, int ncols, int t, int* strip, int* step) {
  const int nstrips = (ncols + 63) >> 6;
  for (int k = form_q_steps(kmax, b, ncols) - 1; k >= 0; --k) {
    const int smin = (k * b) >> 6, cnt = nstrips - smin;  // (k b <= ncols - 1: no overflow, cnt >= 1)
    if (t < cnt) {
      *strip = smin + t;
      *step = k;
      return true;
    }
    t -= cnt;
  }
  return false;
}
static inline long long form_q_items(int kmax, int b, int ncols) {
  const int nstrips = (ncols + 63) >> 6;
  long long n = 0;
  for (int k = form_q_steps(kmax, b, ncols) - 1; k >= 0; --k) n += nstrips - ((k * b) >> 6);
  return n;
}

struct ApplyPipeArgs {
  ApplyArgs q;      // k_apply_q's arguments (tau unused)
  long long nslot;  // flags per strip: the stored tiles (l,k), l >= k, k < kmax
  int epoch;        // this call's flag value
  int* ws;          // the handle's workspace: header, then the flags [strip][tile_slot(l, k, p)]
};

// ---------------------------------------------------------------------------------------
// One workgroup per ticket = (strip, step k): wave w owns columns 64 strip + 16w .. + 15 of C, a lane
// its column's rows x mod 4, as in k_apply_q. A wave with no column below nrhs does no MFMA work but
// takes part in the staging and in every barrier.
// ---------------------------------------------------------------------------------------
template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT) void k_apply_q_pipe(ApplyPipeArgs pa) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  constexpr int SC1 = 16;  // aux bits of every C access
  extern __shared__ __align__(16) double lds[];
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;
  __shared__ int s_tk, s_ok;
  const ApplyArgs& a = pa.q;

  const int tk = pipe_take_ticket(pa.ws, &s_tk), nstrips = (a.nrhs + 63) >> 6;
  if (tk < 0 || tk >= a.kmax * nstrips) return;  // (an earlier call of the handle timed out: tqr_apply_pipe_status)
  int strip, k;
  pipe_ticket_map(a.kmax, nstrips, TRANS, tk, &strip, &k);

  const size_t ldc = a.ldc;
  const int lane = threadIdx.x & 63, x = lane >> 4, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = strip * 64 + 16 * w, col = col0 + (lane & 15);
  const bool active = col0 < a.nrhs;  // wave-uniform
  // The staging and the MFMA loops leave few SGPRs at b = 256, so what only the hand-over reads sits
  // in VGPRs, which are plentiful at one workgroup per CU (solve_pipe.hip): the lane's column mask as
  // an integer instead of a mask pair, the strip's flags, the error word and the epoch.
  int on = col < a.nrhs;
  unsigned long long flv = (unsigned long long)(pa.ws + PIPE_HDR) + (unsigned long long)strip * (unsigned long long)pa.nslot * sizeof(int);
  unsigned long long errv = (unsigned long long)(pa.ws + PIPE_ERR);
  int epoch = pa.epoch, nact = a.nrhs - col0;
  asm volatile("" : "+v"(on), "+v"(flv), "+v"(errv), "+v"(epoch), "+v"(nact));
  // So do the operands' addresses, which the staging turns into wave-uniform resources by readfirstlane
  // (uniform_rsrc) once per group: tile column k of A, its leading dimension, and the T images.
  unsigned long long akv = (unsigned long long)((const S*)a.A + (size_t)k * B * (size_t)a.lda), ldav = (unsigned long long)a.lda;
  unsigned long long twv = (unsigned long long)a.Tw;
  asm volatile("" : "+v"(akv), "+v"(ldav), "+v"(twv));
  const S* const Ak = (const S*)akv;
  const size_t lda = ldav;
  ApplyArgs at = a;  // (tg_ptr reads Tw and p)
  at.Tw = (double*)twv;
  // one resource over the wave's 16 columns of C (an idle wave's is never used); a row tile is a byte
  // offset in it (below 2^31 by the leading-dimension bound), koff the workgroup's own C_k
  S* Cw = (S*)a.C + (size_t)(active ? col0 : 0) * ldc;
  const __amdgpu_buffer_rsrc_t rc = uniform_rsrc(Cw);
  const unsigned coff = head_off<B, S>(ldc, 0);
  const unsigned koff = coff + (unsigned)k * (unsigned)(B * sizeof(S));
  double X[G::NKS];
  double H[G::NRI];

  // Flags, as pointers indexed by the row tile l: fmine[l] is this step's (k, l) — slot tile_slot(k, k, p)
  // + l - k — and fprod[l] the producing step's (k', l), k' = k - 1 (Q^T) or k + 1 (Q); the first step
  // of a direction has no producer. Parked in VGPRs like the rest of the hand-over's values.
  constexpr int KP = TRANS ? -1 : 1;
  const bool first = TRANS ? k == 0 : k == a.kmax - 1;
  unsigned long long fmine = flv + (unsigned long long)((long long)tile_slot(k, k, a.p) - k) * sizeof(int);
  // (computed in the first step too, where k + KP is no step and the pointer is never used: a select
  // here kept `first` in a mask pair of SGPRs)
  unsigned long long fprod = flv + (unsigned long long)((long long)tile_slot(k + KP, k + KP, a.p) - (k + KP)) * sizeof(int);
  asm volatile("" : "+v"(fmine), "+v"(fprod));
  // all threads: the producing step has released row tile l of this strip in this call (false: error
  // or timeout, uniform)
  auto wait = [&](int l) { return pipe_wait((int*)fprod + l, epoch, (int*)errv, &s_ok); };
  // release row tile l
  auto publish = [&](int l) { pipe_publish((int*)fmine + l, epoch); };
  // k_apply_q's unmqr(k): tile (k,k) on C_k, groups ascending (Q^T) / descending (Q)
  auto unmqr = [&](const bool active) {
    const S* Vt = Ak + (size_t)k * B;
    if (active) load_rows<B, S, SC1>(X, rc, koff, on != 0);
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_vq<B, S, true, !TRANS>(Vs, Vt, lda, g * IB);
      stage_tq<B, !TRANS>(Ts, tg_ptr<B>(at, k, k, g));
      __syncthreads();
      if (active) apply_group<B, false>(Vs, Ts, X, H, g * IB / 4);
    }
    if (active) store_rows<B, S, SC1>(X, rc, koff, on != 0);
  };
  // k_apply_q's tsmqr(l, k): tile (l,k) on [C_k; C_l] — C_l's strip stays in registers over the groups,
  // the 32 head rows of C_k are loaded and stored per group
  auto tsmqr = [&](int l) {
    const S* Vt = Ak + (size_t)l * B;
    const unsigned loff = coff + (unsigned)l * (unsigned)(B * sizeof(S));
    if (active) load_rows<B, S, SC1>(X, rc, loff, on != 0);
    for (int gi = 0; gi < NG; ++gi) {
      const int g = TRANS ? gi : NG - 1 - gi;
      __syncthreads();
      stage_vq<B, S, false, !TRANS>(Vs, Vt, lda, g * IB);
      stage_tq<B, !TRANS>(Ts, tg_ptr<B>(at, l, k, g));
      __syncthreads();
      if (active) {
        // (Q: the head rows in reverse — this lane takes the rows of lane row 3 - x)
        const unsigned hoff = koff + (unsigned)((g * IB + (TRANS ? 0 : 3 - 2 * x)) * (int)sizeof(S));
        load_hrows<B, S, !TRANS, SC1>(H, rc, hoff, on != 0);
        apply_group<B, true>(Vs, Ts, X, H, 0);
        store_hrows<B, S, !TRANS, SC1>(H, rc, hoff, on != 0);
      }
    }
    if (active) store_rows<B, S, SC1>(X, rc, loff, on != 0);
  };

  // No byte of a row tile other than C_k is read before its flag is seen: the only such loads are
  // tsmqr's load_rows, behind wait. C_k itself was last stored by the producing step as its C_l, l = k
  // (Q^T: flag (k-1, k), awaited ahead of unmqr; Q: by nobody).
  if constexpr (TRANS) {
    if (!first && !wait(k)) return;
    unmqr(active);
    for (int l = k + 1; l < a.p; ++l) {
      if (!first && !wait(l)) return;
      tsmqr(l);
      publish(l);
    }
  } else {
    for (int l = a.p - 1; l > k; --l) {
      if (!first && !wait(l)) return;  // (l = k+1: flag (k+1, k+1), the producer's UNMQR)
      tsmqr(l);
      publish(l);
    }
    // (`active` anew from its parked operand: as one value it would have to outlive the loop above, a
    // lane-mask pair of SGPRs that spilled at b = 256)
    asm volatile("" : "+v"(nact));
    unmqr(__builtin_amdgcn_readfirstlane(nact) > 0);
    publish(k);
  }
}

// ---------------------------------------------------------------------------------------
// Form Q: k_apply_q_pipe<B, S, false> on form_q_ticket_map's items, with C = Q output-only (a.nrhs is
// ncols). Same thread layout, resources, flags, wait and publish, the same unmqr / tsmqr on the same
// operands; what differs is where a row tile's values come from the first time the call touches it:
// E's 0 / 1 pattern built in registers (synth_rows) instead of load_rows. That is C_k in every step —
// no step above k touches row tile k — and every C_l in the strip's first step kf, which therefore
// waits for nothing. A sibling kernel, not a template flag, for a measured reason: one body for both
// (a forceinline function template with a FORM flag, the two kernels one-line callers) kept every
// instantiation free of scratch and spills and within 4 VGPRs, but changed k_apply_q_pipe's register
// allocation and instruction order, and k_apply_q_pipe<256, double, false> came out 0.3 - 0.4 % slower
// than before on an MI355X, beyond its run-to-run spread, with the body's arguments by reference and
// by value alike (profiles/apply/refactor_ab.jsonl). The two share the protocol through
// pipe_dev.hpp's helpers only.
// ---------------------------------------------------------------------------------------
// stage_vq<B, S, false, true> (a TSMQR tile's V group, columns reversed: the same image) with the batch
// written out: up to eight loads issued, then their LDS writes, a scheduling barrier in between. In
// k_form_q_pipe<256, .> the compiler had turned stage_vq's unrolled loop into load - wait - write per
// element (256 exposed load latencies per tile operation, 1.5 x its time); k_apply_q_pipe gets the
// batch from the same loop by itself, and stage_vq stays as it is for it.
template <int B, typename S>
__device__ __forceinline__ void stage_vq_ts_rev(double* Vs, const S* __restrict__ vt, size_t ldm, int c0) {
  using g = Geo<B>;
  constexpr int N = B * g::IB / NT, U = N < 8 ? N : 8;  // elements per thread, per batch
  static_assert(B * g::IB % NT == 0 && N % U == 0, "whole batches");
  const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(vt + (size_t)c0 * ldm);
  for (int i0 = 0; i0 < N; i0 += U) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = threadIdx.x + (i0 + u) * NT, r = idx % B, c = idx / B;
      const unsigned off = (unsigned)(((size_t)c * ldm + r) * sizeof(S));
      if constexpr (sizeof(S) == 8) {
        const auto w = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
        v[u] = dbl_of(w[0], w[1]);
      } else {
        v[u] = (double)__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = threadIdx.x + (i0 + u) * NT, r = idx % B, c = idx / B;
      Vs[r * g::VP + g::pc(g::IB - 1 - c)] = v[u];
    }
  }
}

template <int B, typename S>
__global__ __launch_bounds__(NT) void k_form_q_pipe(ApplyPipeArgs pa) {
  using G = Geo<B>;
  constexpr int IB = G::IB, NG = G::NG;
  constexpr int SC1 = 16;  // aux bits of every C access
  extern __shared__ __align__(16) double lds[];
  double* Vs = lds;
  double* Ts = Vs + G::VSZ;
  __shared__ int s_tk, s_ok;
  const ApplyArgs& a = pa.q;

  const int tk = pipe_take_ticket(pa.ws, &s_tk);
  int strip, k;
  if (tk < 0 || !form_q_ticket_map(a.kmax, B, a.nrhs, tk, &strip, &k)) return;  // (tk < 0: k_apply_q_pipe)
  // the strip's first step kf = min(jhi, kmax - 1), jhi the row tile of its last column
  const int lastcol = strip * 64 + 63 < a.nrhs - 1 ? strip * 64 + 63 : a.nrhs - 1;
  const bool first = k == (lastcol / B < a.kmax - 1 ? lastcol / B : a.kmax - 1);

  // (k_apply_q_pipe's values, parked in VGPRs for its reasons)
  const size_t ldc = a.ldc;
  const int lane = threadIdx.x & 63, x = lane >> 4, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col0 = strip * 64 + 16 * w, col = col0 + (lane & 15);
  const bool active = col0 < a.nrhs;  // wave-uniform
  int on = col < a.nrhs;
  unsigned long long flv = (unsigned long long)(pa.ws + PIPE_HDR) + (unsigned long long)strip * (unsigned long long)pa.nslot * sizeof(int);
  unsigned long long errv = (unsigned long long)(pa.ws + PIPE_ERR);
  int epoch = pa.epoch, nact = a.nrhs - col0;
  asm volatile("" : "+v"(on), "+v"(flv), "+v"(errv), "+v"(epoch), "+v"(nact));
  unsigned long long akv = (unsigned long long)((const S*)a.A + (size_t)k * B * (size_t)a.lda), ldav = (unsigned long long)a.lda;
  unsigned long long twv = (unsigned long long)a.Tw;
  asm volatile("" : "+v"(akv), "+v"(ldav), "+v"(twv));
  const S* const Ak = (const S*)akv;
  const size_t lda = ldav;
  ApplyArgs at = a;  // (tg_ptr reads Tw and p)
  at.Tw = (double*)twv;
  S* Cw = (S*)a.C + (size_t)(active ? col0 : 0) * ldc;
  const __amdgpu_buffer_rsrc_t rc = uniform_rsrc(Cw);
  const unsigned coff = head_off<B, S>(ldc, 0);
  const unsigned koff = coff + (unsigned)k * (unsigned)(B * sizeof(S));
  double X[G::NKS];
  double H[G::NRI];

  // flags as in k_apply_q_pipe: fmine[l] is (k, l), fprod[l] is (k + 1, l) (never used in step kf)
  unsigned long long fmine = flv + (unsigned long long)((long long)tile_slot(k, k, a.p) - k) * sizeof(int);
  unsigned long long fprod = flv + (unsigned long long)((long long)tile_slot(k + 1, k + 1, a.p) - (k + 1)) * sizeof(int);
  asm volatile("" : "+v"(fmine), "+v"(fprod));
  auto wait = [&](int l) { return pipe_wait((int*)fprod + l, epoch, (int*)errv, &s_ok); };
  auto publish = [&](int l) { pipe_publish((int*)fmine + l, epoch); };
  // E's values in the lane's rows of row tile l: 1.0 where the global row equals the global column,
  // +0.0 elsewhere and in a masked lane (load_rows' zeros)
  auto synth_rows = [&](int l) {
    const int d = on != 0 ? col - (l * B + x) : -1;  // 4 x the lane's k-step that holds the diagonal
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) X[ks] = d == 4 * ks ? 1.0 : 0.0;
  };
  // k_apply_q_pipe's unmqr(k) for Q
  auto unmqr = [&](const bool active) {
    const S* Vt = Ak + (size_t)k * B;
    if (active) load_rows<B, S, SC1>(X, rc, koff, on != 0);
    for (int gi = 0; gi < NG; ++gi) {
      const int g = NG - 1 - gi;
      __syncthreads();
      stage_vq<B, S, true, true>(Vs, Vt, lda, g * IB);
      stage_tq<B, true>(Ts, tg_ptr<B>(at, k, k, g));
      __syncthreads();
      if (active) apply_group<B, false>(Vs, Ts, X, H, g * IB / 4);
    }
    if (active) store_rows<B, S, SC1>(X, rc, koff, on != 0);
  };
  // k_apply_q_pipe's tsmqr(l, k) for Q, C_l synthesised in step kf
  auto tsmqr = [&](int l) {
    const S* Vt = Ak + (size_t)l * B;
    const unsigned loff = coff + (unsigned)l * (unsigned)(B * sizeof(S));
    if (active) {
      if (first) synth_rows(l);
      else load_rows<B, S, SC1>(X, rc, loff, on != 0);
    }
    for (int gi = 0; gi < NG; ++gi) {
      const int g = NG - 1 - gi;
      __syncthreads();
      stage_vq_ts_rev<B, S>(Vs, Vt, lda, g * IB);
      stage_tq<B, true>(Ts, tg_ptr<B>(at, l, k, g));
      __syncthreads();
      if (active) {
        const unsigned hoff = koff + (unsigned)((g * IB + 3 - 2 * x) * (int)sizeof(S));
        load_hrows<B, S, true, SC1>(H, rc, hoff, on != 0);
        apply_group<B, true>(Vs, Ts, X, H, 0);
        store_hrows<B, S, true, SC1>(H, rc, hoff, on != 0);
      }
    }
    if (active) store_rows<B, S, SC1>(X, rc, loff, on != 0);
  };

  // C_k goes to memory ahead of everything: tsmqr takes its head rows from there group by group (other
  // lanes' rows of the wave's own columns), unmqr all of it. No byte of C is read that this call has
  // not stored: C_k here, every C_l by this step (kf) or behind the producer's flag.
  if (active) {
    synth_rows(k);
    store_rows<B, S, SC1>(X, rc, koff, on != 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int l = a.p - 1; l > k; --l) {
    if (!first && !wait(l)) return;  // (l = k+1: flag (k+1, k+1), the producer's UNMQR)
    tsmqr(l);
    publish(l);
  }
  asm volatile("" : "+v"(nact));  // (`active` anew, as in k_apply_q_pipe)
  unmqr(__builtin_amdgcn_readfirstlane(nact) > 0);
  publish(k);
}

typedef void (*apfn)(ApplyPipeArgs);
template <int B>
static apfn apipe_kernel(int dtype, int trans) {
  if (dtype == TQR_F64) return trans == TQR_TRANS ? k_apply_q_pipe<B, double, true> : k_apply_q_pipe<B, double, false>;
  return trans == TQR_TRANS ? k_apply_q_pipe<B, float, true> : k_apply_q_pipe<B, float, false>;
}
static apfn apipe_kernel_b(int b, int dtype, int trans) {
  return dispatch_b(b, [&](auto bb) { return apipe_kernel<decltype(bb)::value>(dtype, trans); });
}
template <int B>
static apfn aform_kernel(int dtype) {
  return dtype == TQR_F64 ? k_form_q_pipe<B, double> : k_form_q_pipe<B, float>;
}
static apfn aform_kernel_b(int b, int dtype) {
  return dispatch_b(b, [&](auto bb) { return aform_kernel<decltype(bb)::value>(dtype); });
}

}  // namespace tqr

using namespace tqr;

struct tqr_apply_pipe {
  int m, n, b, p, kmax, dtype, nrhs_max;
  size_t es;
  long long nslot;  // flags per strip
  apfn kn = nullptr, kt = nullptr, kf = nullptr;  // Q, Q^T, form-Q
  PipeCore core;
};

// tqr_apply_pipe_q's argument errors (everything but the handle's prepared state, which needs ap->mu)
static bool apply_pipe_args_ok(const tqr_apply_pipe* pp, const tqr_apply* ap, int trans, const void* dA, int ldda,
                               const void* dC, int nrhs, int lddc) {
  return pp && ap && dA && dC && (trans == TQR_NOTRANS || trans == TQR_TRANS) && nrhs >= 1 && nrhs <= pp->nrhs_max &&
         ldda >= pp->m && lddc >= pp->m && valid_ld(ldda, pp->es) && valid_ld(lddc, pp->es) && ap->m == pp->m &&
         ap->n == pp->n && ap->b == pp->b && ap->dtype == pp->dtype;
}

// One call of the handle, arguments valid: `kern` on `grid` workgroups, one per work item, ordered
// against ap's prepares and the handle's previous call (tqr_apply_pipe_q, tqr_apply_pipe_form_q)
static int apply_pipe_enqueue(tqr_apply_pipe* pp, tqr_apply* ap, apfn kern, unsigned grid, const void* dA, int ldda, void* dC,
                              int nrhs, int lddc, void* stream) {
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lp(pp->core.mu);  // (always pp's before ap's)
  std::lock_guard<std::mutex> la(ap->mu);
  if (!ap->prepared) return TQR_EINVAL;
  if (const int st = pipe_ready(pp->core)) return st;
  ApplyPipeArgs a;
  if (const int st = pipe_call_begin(pp->core, cs, &a.epoch)) return st;
  int slot = 0;
  HIPCHK(apply_enqueue_begin(ap, cs, &slot));
  a.q.A = dA; a.q.tau = nullptr; a.q.C = dC; a.q.Tw = ap->d_T; a.q.lda = ldda; a.q.ldc = lddc;
  a.q.m = pp->m; a.q.p = pp->p; a.q.kmax = pp->kmax; a.q.nrhs = nrhs;
  a.nslot = pp->nslot;
  a.ws = pp->core.d_ws;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), PIPE_LDS, cs, a);
  // evDone and ap's slot are both recorded whatever the launch did, so the next call and the next
  // prepare stay ordered after whatever was enqueued
  const int st = pipe_call_end(pp->core, cs, hipGetLastError(), a.epoch);
  const hipError_t ae = apply_enqueue_end(ap, cs, slot);
  if (st) return st;
  HIPCHK(ae);
  return TQR_OK;
}

extern "C" {

int tqr_apply_pipe_ticket(int kmax, int nstrips, int trans, int ticket, int* strip, int* step) {
  if (kmax < 1 || nstrips < 1 || (trans != TQR_NOTRANS && trans != TQR_TRANS) || !strip || !step || ticket < 0 ||
      (long long)ticket >= (long long)kmax * nstrips)
    return TQR_EINVAL;
  pipe_ticket_map(kmax, nstrips, trans == TQR_TRANS, ticket, strip, step);
  return TQR_OK;
}

void tqr_apply_pipe_destroy(tqr_apply_pipe* pp) {
  if (!pp) return;
  pipe_destroy(pp->core);
  delete pp;
}

int tqr_apply_pipe_create(tqr_apply_pipe** out, int m, int n, int b, int dtype, int nrhs_max) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  if (!valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || (dtype != TQR_F32 && dtype != TQR_F64) ||
      !valid_ld(m, elem_size(dtype)) || nrhs_max < 1)
    return TQR_EINVAL;
  const int p = m / b, q = n / b, kmax = p < q ? p : q;
  const size_t nstrips = ((size_t)nrhs_max + 63) / 64, items = nstrips * (size_t)kmax;
  if (items > 0x7fffffffull) return TQR_EINVAL;  // (one workgroup per item: the grid)
  tqr_apply_pipe* pp = new (std::nothrow) tqr_apply_pipe();
  if (!pp) return TQR_ENOMEM;
  pp->m = m; pp->n = n; pp->b = b; pp->p = p; pp->kmax = kmax; pp->dtype = dtype; pp->nrhs_max = nrhs_max;
  pp->es = elem_size(dtype);
  pp->nslot = (long long)tile_slot(kmax, kmax, p);
  pp->core.ws_bytes = ((size_t)PIPE_HDR + nstrips * (size_t)pp->nslot) * sizeof(int);
  pp->core.kern[0] = (const void*)(pp->kn = apipe_kernel_b(b, dtype, TQR_NOTRANS));
  pp->core.kern[1] = (const void*)(pp->kt = apipe_kernel_b(b, dtype, TQR_TRANS));
  pp->core.kern[2] = (const void*)(pp->kf = aform_kernel_b(b, dtype));
  // without a gfx950 the handle exists but holds no device memory: every call on it validates its
  // arguments and then returns TQR_ENODEV
  const int st = pipe_ready(pp->core);
  if (st != TQR_OK && st != TQR_ENODEV) {
    tqr_apply_pipe_destroy(pp);
    return st;
  }
  *out = pp;
  return TQR_OK;
}

size_t tqr_apply_pipe_workspace_bytes(const tqr_apply_pipe* pp) { return pp ? pp->core.ws_bytes : 0; }

int tqr_apply_pipe_q(tqr_apply_pipe* pp, tqr_apply* ap, int trans, const void* dA, int ldda, void* dC, int nrhs,
                     int lddc, void* stream) {
  if (!apply_pipe_args_ok(pp, ap, trans, dA, ldda, dC, nrhs, lddc)) return TQR_EINVAL;
  return apply_pipe_enqueue(pp, ap, trans == TQR_TRANS ? pp->kt : pp->kn, (unsigned)((nrhs + 63) / 64) * (unsigned)pp->kmax, dA,
                            ldda, dC, nrhs, lddc, stream);
}

int tqr_apply_pipe_form_q(tqr_apply_pipe* pp, tqr_apply* ap, const void* dA, int ldda, void* dQ, int ncols, int lddq,
                          void* stream) {
  if (!pp || ncols > pp->m || !apply_pipe_args_ok(pp, ap, TQR_NOTRANS, dA, ldda, dQ, ncols, lddq)) return TQR_EINVAL;
  // (at most the grid tqr_apply_pipe_create checked)
  return apply_pipe_enqueue(pp, ap, pp->kf, (unsigned)form_q_items(pp->kmax, pp->b, ncols), dA, ldda, dQ, ncols, lddq, stream);
}

int tqr_apply_pipe_form_q_items(int kmax, int b, int ncols) {
  if (kmax < 1 || !valid_b(b) || ncols < 1) return TQR_EINVAL;
  const long long n = form_q_items(kmax, b, ncols);
  return n > 0x7fffffffll ? TQR_EINVAL : (int)n;
}

int tqr_apply_pipe_form_q_ticket(int kmax, int b, int ncols, int ticket, int* strip, int* step) {
  if (kmax < 1 || !valid_b(b) || ncols < 1 || !strip || !step || ticket < 0) return TQR_EINVAL;
  int s, k;
  if (!form_q_ticket_map(kmax, b, ncols, ticket, &s, &k)) return TQR_EINVAL;
  *strip = s;
  *step = k;
  return TQR_OK;
}

int tqr_apply_pipe_status(tqr_apply_pipe* pp, void* stream) {
  return pp ? pipe_status(pp->core, stream, "apply: a wait for another workgroup's row tile") : TQR_EINVAL;
}

// tqr_lstsq (apply.hip) with the pipelined apply and the pipelined solve in place of tqr_apply_q and
// tqr_trsm_r: the same steps in the same order on `stream`, nothing allocated
int tqr_lstsq_pipe(tqr_apply_pipe* pp, tqr_solve* sv, tqr_apply* ap, int trans, const void* dA, int ldda, void* dB,
                   int nrhs, int lddb, void* dres, void* stream) {
  if (!pp || !sv || !ap) return TQR_EINVAL;
  if (!apply_pipe_args_ok(pp, ap, trans, dA, ldda, dB, nrhs, lddb) || ap->m < ap->n) return TQR_EINVAL;
  const SolveShape ss = solve_shape(sv);
  if (ss.n != ap->n || ss.b != ap->b || ss.dtype != ap->dtype || nrhs > ss.nrhs_max) return TQR_EINVAL;
  {
    std::lock_guard<std::mutex> lk(ap->mu);
    if (!ap->prepared) return TQR_EINVAL;
  }
  int st;
  if (trans == TQR_NOTRANS) {
    // B <- Q^T B; rows 0 .. n-1 <- R^{-1} of them; the residual norms from rows n .. m-1
    if ((st = tqr_apply_pipe_q(pp, ap, TQR_TRANS, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
    if ((st = tqr_solve_trsm_r(sv, TQR_NOTRANS, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
    return dres ? resnorm(ap->dtype, dB, lddb, ap->n, ap->m, nrhs, dres, stream) : TQR_OK;
  }
  // x = Q [R^{-T} c; 0]
  if (ap->m > ap->n)
    HIPCHK(hipMemset2DAsync((char*)dB + (size_t)ap->n * ap->es, (size_t)lddb * ap->es, 0, (size_t)(ap->m - ap->n) * ap->es,
                            (size_t)nrhs, (hipStream_t)stream));
  if ((st = tqr_solve_trsm_r(sv, TQR_TRANS, dA, ldda, dB, nrhs, lddb, stream)) != TQR_OK) return st;
  return tqr_apply_pipe_q(pp, ap, TQR_NOTRANS, dA, ldda, dB, nrhs, lddb, stream);
}

}  // extern "C"
