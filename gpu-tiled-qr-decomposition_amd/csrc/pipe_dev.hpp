// What the kernels that hand rows from workgroup to workgroup share (solve_pipe.hip's k_trsm_r_pipe,
// apply_pipe.hip's k_apply_q_pipe): the layout of a handle's workspace, the launch's LDS reservation,
// and the flag accesses of the protocol both files describe in their headers.
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

}  // namespace tqr
