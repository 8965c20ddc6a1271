// Host side of a pipelined handle (tqr_solve, tqr_apply_pipe): the device workspace of pipe_dev.hpp's
// protocol, the event that serialises the handle's calls, the epoch bookkeeping around a launch and the
// status read. A handle holds one PipeCore beside its own shape fields; a call is
//   lock core.mu -> pipe_ready -> pipe_call_begin -> fill the arguments, launch -> pipe_call_end.
#pragma once
#include <climits>
#include <mutex>

#include "host_common.hpp"
#include "pipe_dev.hpp"

namespace tqr {

struct PipeCore {
  std::mutex mu;         // the enqueue sequence of a call (epoch, event bookkeeping)
  int* d_ws = nullptr;   // device workspace (null until a gfx950 was seen)
  size_t ws_bytes = 0;   // header and flags
  hipEvent_t evDone = nullptr;
  int epoch = 0;         // of the last call enqueued
  const void* kern[3] = {};  // the handle's kernels (null: none), for the LDS attribute
};

// The handle's device side, made on first need (at create where a device is present): the kernels' LDS
// attribute, the event and the zeroed workspace. mu held, or the handle not yet shared.
static inline int pipe_ready(PipeCore& c) {
  if (c.d_ws) return TQR_OK;
  if (const int st = current_device_is_gfx950()) return st;
  for (const void* k : c.kern)
    if (k) HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PIPE_LDS));
  if (!c.evDone) HIPCHK(hipEventCreateWithFlags(&c.evDone, hipEventDisableTiming));
  int* ws = nullptr;
  if (hipMalloc(&ws, c.ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return TQR_ENOMEM;
  }
  if (hipMemset(ws, 0, c.ws_bytes) != hipSuccess) {
    (void)hipFree(ws);
    return TQR_EHIP;
  }
  c.d_ws = ws;
  return TQR_OK;
}

// Ahead of a launch on stream cs, mu held and the core ready: cs waits for the handle's previous call,
// the ticket counter is zeroed, and *epoch_out is the flag value of this call.
static inline int pipe_call_begin(PipeCore& c, hipStream_t cs, int* epoch_out) {
  HIPCHK(hipStreamWaitEvent(cs, c.evDone, 0));  // the previous call of this handle (any stream)
  if (c.epoch == INT_MAX) {  // the epochs start over: behind the previous call, ahead of this one
    HIPCHK(hipMemsetAsync(c.d_ws + PIPE_HDR, 0, c.ws_bytes - PIPE_HDR * sizeof(int), cs));
    c.epoch = 0;
  }
  *epoch_out = c.epoch + 1;
  HIPCHK(hipMemsetAsync(c.d_ws + PIPE_TICKET, 0, sizeof(int), cs));  // (the error word stays: pipe_status)
  return TQR_OK;
}

// Behind the launch, launch_err its hipGetLastError(): evDone is recorded behind whatever was enqueued,
// so the next call stays ordered after it, and the epoch is committed only once the launch is enqueued.
static inline int pipe_call_end(PipeCore& c, hipStream_t cs, hipError_t launch_err, int epoch) {
  const hipError_t re = hipEventRecord(c.evDone, cs);
  HIPCHK(launch_err);
  c.epoch = epoch;
  HIPCHK(re);
  return TQR_OK;
}

// The handle's status call: waits for `stream` and for the handle's last call, and reports a timed-out
// wait once. `what` completes the message: "<routine>: a wait for another workgroup's <unit>".
static inline int pipe_status(PipeCore& c, void* stream, const char* what) {
  std::lock_guard<std::mutex> lk(c.mu);
  if (!c.d_ws) return TQR_OK;  // nothing was ever enqueued
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipEventSynchronize(c.evDone));  // the handle's last call, whatever its stream
  int err = 0;
  HIPCHK(hipMemcpy(&err, c.d_ws + PIPE_ERR, sizeof(int), hipMemcpyDeviceToHost));
  if (!err) return TQR_OK;
  fprintf(stderr, "tqr: pipelined %s timed out (error word %d)\n", what, err);
  HIPCHK(hipMemset(c.d_ws + PIPE_ERR, 0, sizeof(int)));  // reported once; the handle is usable again
  return TQR_EHIP;
}

static inline void pipe_destroy(PipeCore& c) {
  if (c.evDone) {
    (void)hipEventSynchronize(c.evDone);  // the last call may still be reading the workspace
    (void)hipEventDestroy(c.evDone);
  }
  if (c.d_ws) (void)hipFree(c.d_ws);
}

}  // namespace tqr
