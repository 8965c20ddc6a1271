// Host side of the apply handle (include/tqr.h "apply"), shared by apply.hip (tqr_apply_*, tqr_lstsq)
// and apply_pipe.hip (tqr_apply_pipe_*, tqr_lstsq_pipe): the handle itself and the event bookkeeping that orders every apply of a handle against its prepares.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

namespace tqr {

struct ApplyArgs;
typedef void (*afn)(ApplyArgs);

// applies of one handle on up to NSLOT distinct streams are tracked one event each, so that a
// later prepare can wait for all of them; further streams share slot 0 (and are ordered behind
// its previous apply)
constexpr int APPLY_NSLOT = 8;

// dynamic LDS (bytes): k_apply_q holds a group's V image and T image (the engine's k_update),
// k_apply_t the V image, T, Gram, taus and four partial Grams (the engine's k_build_t)
static inline size_t lds_apply_q(int b) {
  const int ib = b < 32 ? b : 32;
  return ((size_t)b * (ib + 2) + (size_t)ib * (ib + 1)) * sizeof(double);
}
static inline size_t lds_apply_t(int b) {
  const int ib = b < 32 ? b : 32;
  return ((size_t)b * (ib + 2) + 6 * (size_t)ib * (ib + 1) + ib + 2) * sizeof(double);
}
static inline size_t timg_doubles(int b) {  // Geo<b>::TIMG
  const size_t ib = b < 32 ? b : 32;
  return (ib * (ib + 1) + 127) / 128 * 128;
}
// bytes of the T workspace of one factorisation of p x kmax tiles: a T image per reflector group of
// every stored tile (l,k), l >= k, k < kmax (apply_dev.hpp tile_slot(kmax, kmax, p) of them)
static inline size_t apply_ws_bytes(int p, int kmax, int b) {
  const size_t ntiles = (size_t)((long long)kmax * p - (long long)kmax * (kmax - 1) / 2);
  return ntiles * (size_t)(b / (b < 32 ? b : 32)) * timg_doubles(b) * sizeof(double);
}

}  // namespace tqr

struct tqr_apply {
  int m, n, b, p, q, kmax, dtype;
  size_t es, ws_bytes;
  double* d_T = nullptr;
  tqr::afn kt = nullptr, kqt = nullptr, kqn = nullptr;
  bool prepared = false;
  std::mutex mu;  // the enqueue sequences of prepare / apply_q (event bookkeeping)
  hipEvent_t evPrep = nullptr;
  hipEvent_t evApply[tqr::APPLY_NSLOT] = {};
  hipStream_t slotStream[tqr::APPLY_NSLOT] = {};
  int nslot = 0;  // slots holding an apply enqueued since the last prepare
};

namespace tqr {

// Around the launch of an apply on stream cs, ap->mu held and ap prepared. begin: cs waits for the
// handle's last prepare, and *slot is the event slot of cs. end: the apply is recorded in that slot,
// so that the next prepare waits for it.
static inline hipError_t apply_enqueue_begin(tqr_apply* ap, hipStream_t cs, int* slot) {
  hipError_t e = hipStreamWaitEvent(cs, ap->evPrep, 0);
  if (e != hipSuccess) return e;
  int s = 0;
  while (s < ap->nslot && ap->slotStream[s] != cs) ++s;
  if (s == APPLY_NSLOT) {  // more streams than slots: queue behind slot 0's apply and take it over
    s = 0;
    e = hipStreamWaitEvent(cs, ap->evApply[0], 0);
  }
  *slot = s;
  return e;
}
static inline hipError_t apply_enqueue_end(tqr_apply* ap, hipStream_t cs, int slot) {
  const hipError_t e = hipEventRecord(ap->evApply[slot], cs);
  if (e != hipSuccess) return e;
  ap->slotStream[slot] = cs;
  if (slot == ap->nslot) ap->nslot = slot + 1;
  return hipSuccess;
}

}  // namespace tqr
