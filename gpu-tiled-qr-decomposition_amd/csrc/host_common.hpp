// Host helpers every HIP unit of the library uses (engine.hip and the plan units through plan.hpp,
// apply.hip, apply_pipe.hip, solve.hip, solve_pipe.hip, batch.hip, tsqr.hip, batch_apply.hip): the error macro, the device check, the argument bounds of include/tqr.h and the
// dispatch on the tile size. Header-only; it includes HIP, so the planner (flowplan.cpp, built by g++)
// never sees it — the one thing the two share, valid_b, lives in flow_list.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <type_traits>

#include "flow_list.hpp"
#include "tqr.h"

#define HIPCHK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "tqr: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return TQR_EHIP;                                                                    \
    }                                                                                     \
  } while (0)

namespace tqr {

// TQR_OK if the current device is a gfx950, else TQR_ENODEV (no device: HIP's error state is cleared,
// so a host without a GPU can go on creating handles)
static inline int current_device_is_gfx950() {
  int dev = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess) {
    (void)hipGetLastError();
    return TQR_ENODEV;
  }
  if (strncmp(pr.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "tqr: device %d is %s, this build targets gfx950 only\n", dev, pr.gcnArchName);
    return TQR_ENODEV;
  }
  return TQR_OK;
}

// The library's leading-dimension bound (include/tqr.h): buffer resources are based at a strip's or a
// reflector group's first column and address at most 32 columns with 32-bit byte offsets (tiles.hpp
// load_strip_pair, flow.hpp), so 32 * ld * sizeof(element) must stay below 2^31 (ld <= 8,388,607 rows
// fp64, 16,777,215 fp32).
static inline bool valid_ld(long ld, size_t es) { return ld > 0 && (size_t)32 * (size_t)ld * es <= 0x7fffffffull; }

static inline size_t elem_size(int dtype) { return dtype == TQR_F64 ? 8 : 4; }

// f(std::integral_constant<int, b>) for a tile size that passed valid_b (flow_list.hpp): the one place
// a run-time b becomes a template argument.
template <typename F>
static inline auto dispatch_b(int b, F f) {
  switch (b) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    default: return f(std::integral_constant<int, 256>{});
  }
}

}  // namespace tqr
