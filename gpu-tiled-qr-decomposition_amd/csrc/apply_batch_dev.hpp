// The apply's two whole-factorisation kernels with the member of a batch as a second grid dimension,
// shared by tsqr.hip (the member is a row domain of a level) and batch_apply.hip (the member is a
// matrix of a strided batch). blockIdx.y's offset is taken in 64 bits on the base pointers; inside a
// member the offsets are the apply's own, and the bodies are apply_dev.hpp's — the same code on the
// same operands as apply.hip's k_apply_t / k_apply_q, so the same bits. The kernels are templates:
// each unit that launches them holds its own instantiations.
#pragma once
#include "apply_dev.hpp"

namespace tqr {

struct ApplyBatchArgs {
  ApplyArgs a;                       // domain 0 of the launch
  long long sA, sTau, sC, sTw;       // elements (sTw: doubles) between consecutive domains
};

template <int B, typename S>
__device__ __forceinline__ ApplyArgs domain_args(const ApplyBatchArgs& ba) {
  ApplyArgs a = ba.a;
  const size_t i = blockIdx.y;
  a.A = (const S*)a.A + i * (size_t)ba.sA;
  a.tau = (const S*)a.tau + i * (size_t)ba.sTau;
  a.C = (S*)a.C + i * (size_t)ba.sC;
  a.Tw = a.Tw + i * (size_t)ba.sTw;
  return a;
}

template <int B, typename S>
__global__ __launch_bounds__(NT, 1) void k_apply_t_batch(ApplyBatchArgs ba) {
  extern __shared__ __align__(16) double lds[];
  const ApplyArgs a = domain_args<B, S>(ba);
  apply_t_body<B, S>(a, blockIdx.x, lds);
}

template <int B, typename S, bool TRANS>
__global__ __launch_bounds__(NT, 2) void k_apply_q_batch(ApplyBatchArgs ba) {
  extern __shared__ __align__(16) double lds[];
  const ApplyArgs a = domain_args<B, S>(ba);
  apply_q_body<B, S, TRANS>(a, blockIdx.x, lds);
}

}  // namespace tqr
