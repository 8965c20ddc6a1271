// What the kernels that hand rows from workgroup to workgroup share (solve_pipe.hip's k_trsm_r_pipe,
// apply_pipe.hip's k_apply_q_pipe and k_form_q_pipe): the layout of a handle's workspace, the launch's
// LDS reservation, the ticket map and the device side of the protocol. Its host side is pipe_host.hpp.
//
// Protocol between workgroups (MI355X_MICROARCH.md "Workgroup dispatch ... inter-workgroup
// visibility", "Valid forms", first table row; the engine's form, flow.hpp). Each kernel's file says
// what its work items are, which item produces what another waits for, and what a flag means; the rest
// is the same everywhere:
//   * work items come from one atomic ticket counter, never from blockIdx (pipe_take_ticket), and
//     every producer of an item has a smaller ticket (pipe_ticket_map, form_q_ticket_map). A workgroup
//     that waits holds a ticket, so everything it waits for was taken by a workgroup already running:
//     the smallest unfinished ticket never waits on an unfinished one, whatever the dispatch order and
//     however few workgroups are resident;
//   * every load and store of the rows that are handed over is an sc1 buffer access (L1-bypassing /
//     write-through), the workgroup's own rows included. To publish (pipe_publish), each wave drains
//     its stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, and one lane stores the flag
//     (sc1). A consumer's thread 0 polls that flag with sc1 loads and s_sleep (pipe_wait); the other
//     waves load the rows only behind the barrier thread 0 then joins;
//   * the table row holds at one workgroup per CU: the launch asks for PIPE_LDS bytes of LDS (more
//     than half a CU's 160 KiB), so two of these workgroups never share a CU;
//   * a flag holds the epoch of the call that set it and a call waits for its own epoch, so nothing
//     is reset between calls (pipe_call_begin starts the epochs over at INT_MAX); the ticket counter
//     is zeroed by a memset ahead of each launch, and the calls of one handle are serialised by an
//     event, as tqr_plan_execute's are;
//   * every spin is bounded (PIPE_TIMEOUT): on expiry the error word is set, the workgroup leaves
//     without publishing, and every workgroup that sees the word — in a spin or before it takes a
//     ticket — leaves too. The handle's status call reports it (pipe_status).
#pragma once
#include "tiles.hpp"

namespace tqr {

// workspace (ints): the ticket counter, the error word, padding to a 128-B line, then the flags
constexpr int PIPE_TICKET = 0, PIPE_ERR = 1, PIPE_HDR = 32;
// dynamic LDS of a launch: more than half of a CU's 160 KiB, whatever the operand images need
constexpr size_t PIPE_LDS = 96 * 1024;
static_assert(PIPE_LDS >= (Geo<256>::VSZ + Geo<256>::TSZ) * sizeof(double) && 2 * PIPE_LDS > 160 * 1024,
              "one workgroup per CU");
constexpr unsigned long long PIPE_TIMEOUT = 500000000ull;  // 5 s of s_memrealtime (100 MHz), as FLOW_TIMEOUT

// Work item of ticket t on n positions x nstrips strips: tickets go position by position in the order
// the routine needs them (TRANS: 0 first; else n-1 first), all strips of a position side by side — so
// the producers of (strip, pos), the positions ahead of it in the same strip, have smaller tickets.
// A position is a tile row of the solve, a step of the apply.
__host__ __device__ inline void pipe_ticket_map(int n, int nstrips, bool trans, int t, int* strip, int* pos) {
  const int q = t / nstrips;
  *strip = t - q * nstrips;
  *pos = trans ? q : n - 1 - q;
}

// (global-address-space accesses: a generic pointer would make them FLAT instructions, flow.hpp)
typedef __attribute__((address_space(1))) int pint;
__device__ __forceinline__ int ld_sc1(int* p) {
  return __hip_atomic_load((pint*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0 only: spin until *p >= target; false on error / timeout (flow.hpp spin_ge_i; inlined: a call
// here made the kernel keep wave-uniform values in VGPR lanes across it)
__device__ __forceinline__ bool pipe_spin_ge(int* p, int target, int* err) {
  if (ld_sc1(p) >= target) return true;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (ld_sc1(p) < target) {
    if (ld_sc1(err)) return false;
    __builtin_amdgcn_s_sleep(8);
    if (__builtin_amdgcn_s_memrealtime() - t0 > PIPE_TIMEOUT) {
      __hip_atomic_store((pint*)err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
  return true;
}

// All threads, first thing in a kernel: the workgroup's ticket (uniform), or -1 if an earlier call of
// the handle timed out and was not yet reported. s_tk: a __shared__ word of the kernel.
__device__ __forceinline__ int pipe_take_ticket(int* ws, int* s_tk) {
  if (threadIdx.x == 0)
    *s_tk = ld_sc1(ws + PIPE_ERR) ? -1 : __hip_atomic_fetch_add((pint*)(ws + PIPE_TICKET), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*s_tk);
}
// All threads: what `flag` stands for is final in this call (false: error or timeout, uniform). s_ok: a
// __shared__ word of the kernel.
__device__ __forceinline__ bool pipe_wait(int* flag, int epoch, int* err, int* s_ok) {
  if (threadIdx.x == 0) *s_ok = pipe_spin_ge(flag, epoch, err) ? 1 : 0;
  __syncthreads();
  // (thread 0 rewrites s_ok only behind the next barrier, which every thread reaches after this read)
  return *s_ok != 0;
}
// All threads: every wave's stores drained, a barrier, one lane's flag store
__device__ __forceinline__ void pipe_publish(int* flag, int epoch) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store((pint*)flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace tqr
