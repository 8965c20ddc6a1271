// The strided layouts of a batch (include/tqr.h "batched", "batched apply and solve"), shared by
// batch.hip and batch_apply.hip: which (leading dimension, stride) pairs place `batch` members of
// rows x cols elements without overlap, and the byte count of a batch's T images. Host only, no HIP:
// plain functions of integers, so a stand-alone program can check them.
#pragma once
#include <cstddef>

namespace tqr {

// Members i = 0 .. batch-1 at element i * stride, column-major with leading dimension ld. With batch
// == 1 the stride is ignored; else one of two forms:
//   stacked          stride >= (cols-1) * ld + rows: one member after the other;
//   row-interleaved  stride >= rows and (batch-1) * stride + rows <= ld: the members are row blocks of
//                    one array under a common ld.
// (ld >= rows and the library's leading-dimension bound are the caller's checks; ld > 0 is assumed.)
static inline bool batch_stride_ok(int rows, int cols, int batch, long long ld, long long stride) {
  if (batch == 1) return true;
  const bool stacked = stride >= (long long)(cols - 1) * ld + rows;
  // (stride <= ld first: the product below then stays far inside 64 bits)
  const bool interleaved = stride >= rows && stride <= ld && (long long)(batch - 1) * stride + rows <= ld;
  return stacked || interleaved;
}

// batch * per bytes, per > 0; 0 if that does not fit a size_t
static inline size_t batch_total_bytes(int batch, size_t per) {
  if (batch < 1 || per == 0 || per > (size_t)-1 / (size_t)batch) return 0;
  return (size_t)batch * per;
}

}  // namespace tqr
