// The single-tile API (tqr_tile_geqrt / unmqr / tsqrt / tsmqr: the reference's four tile routines)
// and the tile batch (tqr_tile_batch). Host code only: every launch goes to a kernel that resolve
// (plan.hpp, engine.hip) hands over — the wave engine's k_panel / k_update and k_build_t — so no
// kernel is instantiated here.
#include <hip/hip_runtime.h>

#include <vector>

#include "gridscheduler.h"
#include "plan.hpp"
#include "tqr.h"
#include "wave_dev.hpp"  // (host side only: lds_panel, lds_update; NT)

using namespace tqr;

// ---- single-tile API ----------------------------------------------------------------------
// The tile(s) are copied into a small device matrix laid out as the corresponding corner of
// a tiled matrix, the task runs as a one-item wave, and the result is copied back.
namespace {
struct TileRun {
  int b, dtype, mr, nc;  // device matrix mr x nc (ld = mr)
  size_t es;
  void* dA = nullptr;
  void* dtau = nullptr;
  double* dT = nullptr;
  Item* dit = nullptr;
  kfn kp, ku, kt;
  int init(int b_, int dtype_, int p, int q) {
    b = b_; dtype = dtype_; mr = p * b; nc = q * b; es = elem_size(dtype);
    if (!valid_b(b) || (dtype != TQR_F64 && dtype != TQR_F32)) return TQR_EINVAL;
    int st = current_device_is_gfx950();
    if (st) return st;
    if ((st = resolve(b, dtype, &kp, &ku, &kt))) return st;
    int ib = b < 32 ? b : 32;
    if (hipMalloc(&dA, es * mr * nc) != hipSuccess || hipMalloc(&dtau, es * mr) != hipSuccess ||
        hipMalloc(&dT, sizeof(double) * (size_t)p * (b / ib) * timg_doubles(b)) != hipSuccess || hipMalloc(&dit, sizeof(Item) * 4) != hipSuccess)
      return TQR_ENOMEM;
    if (hipMemset(dA, 0, es * mr * nc) != hipSuccess || hipMemset(dtau, 0, es * mr) != hipSuccess) return TQR_EHIP;
    return TQR_OK;
  }
  ~TileRun() {
    if (dA) (void)hipFree(dA);
    if (dtau) (void)hipFree(dtau);
    if (dT) (void)hipFree(dT);
    if (dit) (void)hipFree(dit);
  }
  int put(const void* h, int ldm, int r, int c) {  // host tile -> device tile (r,c)
    return hipMemcpy2D((char*)dA + es * ((size_t)c * b * mr + (size_t)r * b), es * mr, h, es * ldm, es * b, b,
                       hipMemcpyHostToDevice) == hipSuccess ? TQR_OK : TQR_EHIP;
  }
  int get(void* h, int ldm, int r, int c) {
    return hipMemcpy2D(h, es * ldm, (char*)dA + es * ((size_t)c * b * mr + (size_t)r * b), es * mr, es * b, b,
                       hipMemcpyDeviceToHost) == hipSuccess ? TQR_OK : TQR_EHIP;
  }
  int put_tau(const void* h, int row0) {
    return hipMemcpy((char*)dtau + es * row0, h, es * b, hipMemcpyHostToDevice) == hipSuccess ? TQR_OK : TQR_EHIP;
  }
  int get_tau(void* h, int row0) {
    return hipMemcpy(h, (char*)dtau + es * row0, es * b, hipMemcpyDeviceToHost) == hipSuccess ? TQR_OK : TQR_EHIP;
  }
  int run(kfn k, Item item, int grid, size_t lds) {
    if (hipMemcpy(dit, &item, sizeof item, hipMemcpyHostToDevice) != hipSuccess) return TQR_EHIP;
    Args a;
    a.A = dA; a.tau = dtau; a.Tw = dT; a.items = dit; a.ldm = mr; a.m = mr; a.p = mr / b; a.kmax = 1;
    hipLaunchKernelGGL(k, dim3(grid), dim3(NT), lds, 0, a);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TQR_EHIP;
    return TQR_OK;
  }
  int ng() const { return b / (b < 32 ? b : 32); }
  int nstrips() const { return (b + 63) / 64; }
  int run_update(Item item) {
    for (int s = 0; s < nstrips(); ++s) {
      Item it2 = item;
      it2.ts |= s << 8;
      int st = run(ku, it2, 1, lds_update(b));
      if (st) return st;
    }
    return TQR_OK;
  }
};
}  // namespace

extern "C" {

int tqr_tile_geqrt(int dtype, void* blk, void* tau, int b, int ldm) {
  if (!blk || !tau || ldm < b) return TQR_EINVAL;
  TileRun tr;
  int st = tr.init(b, dtype, 1, 1);
  if (!st) st = tr.put(blk, ldm, 0, 0);
  if (!st) st = tr.run(tr.kp, Item{QRS, 0, 0, 0}, 1, lds_panel(b));
  if (!st) st = tr.get(blk, ldm, 0, 0);
  if (!st) st = tr.get_tau(tau, 0);
  return st;
}

int tqr_tile_unmqr(int dtype, void* C, const void* V, const void* tau, int b, int ldm) {
  if (!C || !V || !tau || ldm < b) return TQR_EINVAL;
  TileRun tr;
  int st = tr.init(b, dtype, 1, 2);
  if (!st) st = tr.put(V, ldm, 0, 0);
  if (!st) st = tr.put(C, ldm, 0, 1);
  if (!st) st = tr.put_tau(tau, 0);
  if (!st) st = tr.run(tr.kt, Item{QRS, 0, 0, 0}, tr.ng(), lds_build_t(b));
  if (!st) st = tr.run_update(Item{SAPP, 0, 1, 0});
  if (!st) st = tr.get(C, ldm, 0, 1);
  return st;
}

int tqr_tile_tsqrt(int dtype, void* A, void* Bm, void* tau, int b, int ldm) {
  if (!A || !Bm || !tau || ldm < b) return TQR_EINVAL;
  TileRun tr;
  int st = tr.init(b, dtype, 2, 1);
  if (!st) st = tr.put(A, ldm, 0, 0);
  if (!st) st = tr.put(Bm, ldm, 1, 0);
  if (!st) st = tr.run(tr.kp, Item{QRD, 1, 0, 0}, 1, lds_panel(b));
  if (!st) st = tr.get(A, ldm, 0, 0);
  if (!st) st = tr.get(Bm, ldm, 1, 0);
  if (!st) st = tr.get_tau(tau, b);
  return st;
}

int tqr_tile_tsmqr(int dtype, const void* V, void* A, void* Bm, const void* tau, int b, int ldm) {
  if (!V || !A || !Bm || !tau || ldm < b) return TQR_EINVAL;
  TileRun tr;
  int st = tr.init(b, dtype, 2, 2);
  if (!st) st = tr.put(V, ldm, 1, 0);
  if (!st) st = tr.put(A, ldm, 0, 1);
  if (!st) st = tr.put(Bm, ldm, 1, 1);
  if (!st) st = tr.put_tau(tau, b);
  if (!st) st = tr.run(tr.kt, Item{QRD, 1, 0, 0}, tr.ng(), lds_build_t(b));
  if (!st) st = tr.run_update(Item{DAPP, 1, 1, 0});
  if (!st) st = tr.get(A, ldm, 0, 1);
  if (!st) st = tr.get(Bm, ldm, 1, 1);
  return st;
}

// Batched independent tile updates (the reference's testDAPP microbenchmark, gpucalc.cu:1687-1774,
// generalised): nblocks copies of one tile (pair) updated by ONE launch of the update kernel.
int tqr_tile_batch(int dtype, int type, int b, int nblocks, const void* V, int ldv, const void* tau,
                   const void* blk, int ldb, void* out, int ldo, float* ms) {
  if ((type != SAPP && type != DAPP) || nblocks <= 0 || !V || !tau || !blk || !valid_b(b) ||
      (dtype != TQR_F32 && dtype != TQR_F64))
    return TQR_EINVAL;
  const int rows = type == DAPP ? 2 * b : b;  // rows of one block: [A; B] or C
  if (ldv < b || ldb < rows || (out && ldo < rows)) return TQR_EINVAL;
  // the batch lives in one 2b-row device matrix addressed by 32-bit buffer offsets
  if (elem_size(dtype) * 2 * b * ((size_t)(1 + nblocks) * b) > 0x7fffffffull) return TQR_EINVAL;
  int st = current_device_is_gfx950();
  if (st) return st;
  kfn kp, ku, kt;
  if ((st = resolve(b, dtype, &kp, &ku, &kt))) return st;
  const size_t es = elem_size(dtype);
  const int mr = 2 * b, ng = b / (b < 32 ? b : 32), nstrips = (b + 63) / 64;
  const size_t nc = (size_t)(1 + nblocks) * b;
  void *dA = nullptr, *dtau = nullptr;
  double* dT = nullptr;
  Item* dit = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<Item> items;
  items.push_back(type == DAPP ? Item{QRD, 1, 0, 0} : Item{QRS, 0, 0, 0});  // T factors of V
  for (int j = 1; j <= nblocks; ++j)
    for (int s = 0; s < nstrips; ++s) items.push_back(Item{type | (s << 8), type == DAPP ? 1 : 0, j, 0});
  auto fin = [&](int code) {
    if (dA) (void)hipFree(dA);
    if (dtau) (void)hipFree(dtau);
    if (dT) (void)hipFree(dT);
    if (dit) (void)hipFree(dit);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return code;
  };
  if (hipMalloc(&dA, es * mr * nc) != hipSuccess || hipMalloc(&dtau, es * mr) != hipSuccess ||
      hipMalloc(&dT, sizeof(double) * 2 * ng * timg_doubles(b)) != hipSuccess ||
      hipMalloc(&dit, sizeof(Item) * items.size()) != hipSuccess)
    return fin(TQR_ENOMEM);
  if (hipMemset(dA, 0, es * mr * nc) != hipSuccess || hipMemset(dtau, 0, es * mr) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return fin(TQR_EHIP);
  const int vrow = type == DAPP ? b : 0;  // V: tile (1,0) (TSQRT V_B) or tile (0,0) (GEQRT V)
  if (hipMemcpy2D((char*)dA + es * vrow, es * mr, V, es * ldv, es * b, b, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy((char*)dtau + es * vrow, tau, es * b, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dit, items.data(), sizeof(Item) * items.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fin(TQR_EHIP);
  for (int j = 1; j <= nblocks; ++j)
    if (hipMemcpy2D((char*)dA + es * (size_t)j * b * mr, es * mr, blk, es * ldb, es * rows, b, hipMemcpyHostToDevice) != hipSuccess)
      return fin(TQR_EHIP);
  Args a;
  a.A = dA; a.tau = dtau; a.Tw = dT; a.items = dit; a.ldm = mr; a.m = mr; a.p = 2; a.kmax = 1;
  hipLaunchKernelGGL(kt, dim3(ng), dim3(NT), lds_build_t(b), 0, a);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fin(TQR_EHIP);
  a.items = dit + 1;
  if (hipEventRecord(e0, 0) != hipSuccess) return fin(TQR_EHIP);
  hipLaunchKernelGGL(ku, dim3((unsigned)(items.size() - 1)), dim3(NT), lds_update(b), 0, a);
  if (hipGetLastError() != hipSuccess || hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)
    return fin(TQR_EHIP);
  float t = 0;
  if (hipEventElapsedTime(&t, e0, e1) != hipSuccess) return fin(TQR_EHIP);
  if (ms) *ms = t;
  if (out)
    for (int j = 1; j <= nblocks; ++j)
      if (hipMemcpy2D((char*)out + es * (size_t)(j - 1) * b * ldo, es * ldo, (char*)dA + es * (size_t)j * b * mr, es * mr,
                      es * rows, b, hipMemcpyDeviceToHost) != hipSuccess)
        return fin(TQR_EHIP);
  return fin(TQR_OK);
}

}  // extern "C"
