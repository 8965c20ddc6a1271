// Tall-skinny QR (include/tqr.h "tall-skinny"): a tree of strided-batched factorisations.
//
//   level 0       the D_0 = m / m_dom row domains of A itself, factorised by one tqr_batch on the
//                 row-interleaved layout (strideA = m_dom under the caller's ldda);
//   level l >= 1  the R factors of level l-1, fan of them stacked per domain in the handle's own W_l
//                 (k_gather, triangular, zero padding), factorised by one tqr_batch of (fan n) x n;
//   the root's R  copied into the upper triangle of A[0:n, 0:n] (k_scatter, triangular).
// After each level's factorisation its T factors are rebuilt (k_apply_t_batch) into the handle's
// per-level T workspace, one tqr_apply workspace per domain. C <- Q^T C walks the levels upwards —
// k_apply_q_batch on the level's domains, k_gather of the domains' top n rows into the next level's
// C_l — and scatters back down; C <- Q C is the exact reverse.
// k_apply_t_batch / k_apply_q_batch (apply_batch_dev.hpp, shared with batch_apply.hip) are apply.hip's
// kernels (the bodies of apply_dev.hpp) with the domain as a second grid dimension: blockIdx.y's offset
// is taken in 64 bits on the base pointers, and inside a domain the offsets are the apply's own. A
// domain therefore has the bytes tqr_apply_q computes on it alone. Every launch here is ordered by its
// stream only: no flags, counters or waits between workgroups.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "apply.hpp"
#include "apply_batch_dev.hpp"
#include "apply_dev.hpp"
#include "host_common.hpp"
#include "solve.hpp"
#include "tqr.h"

namespace tqr {

// (ApplyBatchArgs, k_apply_t_batch, k_apply_q_batch: apply_batch_dev.hpp, shared with batch_apply.hip)

// ---------------------------------------------------------------------------------------
// Gather / scatter: one thread per element, consecutive threads on consecutive rows of a column
// (coalesced), columns on blockIdx.y (strided when there are more than a grid's y holds).
// The "stack" side is a level's W_l or C_l: blocks of n rows, block j at row j * n. The "domain" side
// is the level below: block j is the top n rows of its domain j, at row j * dom.
// ---------------------------------------------------------------------------------------
struct CopyArgs {
  const void* src;
  void* dst;
  long lds, ldd;   // leading dimensions of src and dst
  long rows;       // rows of the stack side that the launch covers
  long dom;        // domain height of the domain side
  int n, ncols;    // block height; columns
  int nblk;        // real blocks (gather: blocks beyond are zero-filled)
};
constexpr int CT = 256;

// stack <- tops of the domains. TRI: only i <= j of a block is taken, below the diagonal zero.
template <typename S, bool TRI>
__global__ __launch_bounds__(CT) void k_gather(CopyArgs c) {
  const long r = (long)blockIdx.x * CT + threadIdx.x;
  if (r >= c.rows) return;
  const long blk = r / c.n;
  const int i = (int)(r - blk * c.n);
  const S* src = (const S*)c.src + blk * c.dom + i;
  S* dst = (S*)c.dst + r;
  for (int j = blockIdx.y; j < c.ncols; j += gridDim.y) {
    S v = S(0);
    if (blk < c.nblk && (!TRI || i <= j)) v = src[(size_t)j * c.lds];
    dst[(size_t)j * c.ldd] = v;
  }
}
// tops of the domains <- stack. TRI: only the elements i <= j are written.
template <typename S, bool TRI>
__global__ __launch_bounds__(CT) void k_scatter(CopyArgs c) {
  const long r = (long)blockIdx.x * CT + threadIdx.x;
  if (r >= c.rows) return;
  const long blk = r / c.n;
  const int i = (int)(r - blk * c.n);
  const S* src = (const S*)c.src + r;
  S* dst = (S*)c.dst + blk * c.dom + i;
  for (int j = blockIdx.y; j < c.ncols; j += gridDim.y)
    if (!TRI || i <= j) dst[(size_t)j * c.ldd] = src[(size_t)j * c.lds];
}
// E = [I_n; 0], rows x ncols
template <typename S>
__global__ __launch_bounds__(CT) void k_fill_e(CopyArgs c) {
  const long r = (long)blockIdx.x * CT + threadIdx.x;
  if (r >= c.rows) return;
  S* dst = (S*)c.dst + r;
  for (int j = blockIdx.y; j < c.ncols; j += gridDim.y) dst[(size_t)j * c.ldd] = r == j ? S(1) : S(0);
}

// ---------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------
typedef void (*abfn)(ApplyBatchArgs);
typedef void (*cfn)(CopyArgs);
struct TsqrKernels {
  abfn kt = nullptr, kqt = nullptr, kqn = nullptr;
  cfn gtri = nullptr, grect = nullptr, stri = nullptr, srect = nullptr, fill = nullptr;
};
template <int B, typename S>
static void tsqr_kernels(TsqrKernels* k) {
  k->kt = k_apply_t_batch<B, S>;
  k->kqt = k_apply_q_batch<B, S, true>;
  k->kqn = k_apply_q_batch<B, S, false>;
  k->gtri = k_gather<S, true>;
  k->grect = k_gather<S, false>;
  k->stri = k_scatter<S, true>;
  k->srect = k_scatter<S, false>;
  k->fill = k_fill_e<S>;
}

constexpr int kMaxGridY = 65535;
constexpr int kMaxLevels = 32;  // fan >= 2 and D_0 < 2^31

struct TsqrLevel {
  int rows = 0, ndom = 0;  // domain height, domains
  long ld = 0;             // leading dimension of W_l and C_l (levels >= 1): ndom * rows
  size_t bW = 0, bTau = 0, bT = 0, bC = 0, bBatch = 0;  // bytes (own pieces rounded to 256)
  size_t tper = 0;                                      // doubles of one domain's T workspace
  tqr_batch* bt = nullptr;
  char* dW = nullptr;
  char* dTau = nullptr;
  char* dC = nullptr;
  double* dT = nullptr;
};

struct TsqrShape {
  int m, n, b, dtype, m_dom, fan, nrhs_max;
  size_t ws_limit, es, own_bytes, ws_bytes;
  std::vector<TsqrLevel> lv;
};

static size_t round256(size_t x) { return (x + 255) / 256 * 256; }

// The resolved shape of a spec: defaults, levels, bytes. TQR_EINVAL for every argument error of
// include/tqr.h; host only.
static int tsqr_resolve(const tqr_tsqr_spec* sp, TsqrShape* sh) {
  if (!sp) return TQR_EINVAL;
  const int m = sp->m, n = sp->n, b = sp->b;
  if (!valid_b(b) || m <= 0 || n <= 0 || m % b || n % b || (sp->dtype != TQR_F32 && sp->dtype != TQR_F64) ||
      !valid_ld(m, elem_size(sp->dtype)) || m < n || sp->nrhs_max < 0 || sp->m_dom < 0 || sp->fan < 0)
    return TQR_EINVAL;
  const size_t es = elem_size(sp->dtype);
  int fan = sp->fan ? sp->fan : 4;
  if (fan < 2 || (long long)fan * n > 0x7fffffffLL || !valid_ld((long)fan * n, es)) return TQR_EINVAL;
  int m_dom = sp->m_dom;
  if (m_dom == 0) {
    // the smallest multiple of b that divides m and is >= max(4 n, 1024) (measured: DESIGN.md §19); none:
    // one domain
    m_dom = m;
    for (long long d = (std::max(4LL * n, 1024LL) + b - 1) / b * b; d < m; d += b)
      if (m % d == 0) { m_dom = (int)d; break; }
  }
  if (m_dom % b || m_dom < n || m_dom > m || m % m_dom) return TQR_EINVAL;
  sh->m = m; sh->n = n; sh->b = b; sh->dtype = sp->dtype; sh->m_dom = m_dom; sh->fan = fan;
  sh->nrhs_max = sp->nrhs_max; sh->ws_limit = sp->ws_limit; sh->es = es;
  sh->lv.clear();
  const int kmax = n / b;
  size_t own = 0, batch = 0;
  for (int D = m / m_dom, l = 0;; ++l) {
    TsqrLevel L;
    L.ndom = l == 0 ? D : (D + fan - 1) / fan;
    L.rows = l == 0 ? m_dom : fan * n;
    const long long ld = (long long)L.ndom * L.rows;
    if (l > 0 && (ld > 0x7fffffffLL || !valid_ld((long)ld, es))) return TQR_EINVAL;
    L.ld = l == 0 ? 0 : (long)ld;
    const int p = L.rows / b;
    int group = 0;
    if (tqr_batch_plan(L.rows, n, b, sp->dtype, L.ndom, sp->ws_limit, &group, nullptr, nullptr) != TQR_OK) return TQR_EINVAL;
    // the prepare's grid: one workgroup per (stored tile, reflector group) of a domain
    if (apply_ws_bytes(p, kmax, b) / (timg_doubles(b) * sizeof(double)) > 0x7fffffffull) return TQR_EINVAL;
    L.tper = apply_ws_bytes(p, kmax, b) / sizeof(double);
    L.bTau = round256((size_t)L.ndom * L.rows * kmax * es);
    L.bT = round256((size_t)L.ndom * L.tper * sizeof(double));
    L.bW = l == 0 ? 0 : round256((size_t)ld * n * es);
    L.bC = l == 0 ? 0 : round256((size_t)ld * sp->nrhs_max * es);
    // the level's tqr_batch: `group` T workspaces of the wave engine (include/tqr.h "batched")
    L.bBatch = (size_t)group * ((size_t)p * kmax * (b / (b < 32 ? b : 32)) * timg_doubles(b) * sizeof(double));
    own += L.bTau + L.bT + L.bW + L.bC;
    batch += L.bBatch;
    sh->lv.push_back(L);
    D = L.ndom;
    if (D == 1) break;
    if ((int)sh->lv.size() >= kMaxLevels) return TQR_EINVAL;
  }
  sh->own_bytes = own;
  sh->ws_bytes = own + batch;
  return TQR_OK;
}

}  // namespace tqr

using namespace tqr;

struct tqr_tsqr {
  TsqrShape sh;
  TsqrKernels k;
  bool ready = false;     // the device side exists (a gfx950 was present at create)
  bool factored = false;  // a factor has been enqueued successfully
  char* d_mem = nullptr;  // taus, W_l, T workspaces, C_l of every level
  hipEvent_t evDone = nullptr;
  std::mutex mu;  // one enqueue sequence at a time (the calls share the workspaces)
};

// ---- launches (mu held, arguments checked) ------------------------------------------------------
static int launch_copy(cfn k, const CopyArgs& c, hipStream_t cs) {
  if (c.rows <= 0 || c.ncols <= 0) return TQR_OK;
  const unsigned gx = (unsigned)((c.rows + CT - 1) / CT), gy = (unsigned)std::min(c.ncols, kMaxGridY);
  hipLaunchKernelGGL(k, dim3(gx, gy), dim3(CT), 0, cs, c);
  HIPCHK(hipGetLastError());
  return TQR_OK;
}

// the matrix of level l: the caller's A (l == 0) or W_l
static inline const char* level_mat(const tqr_tsqr* h, int l, const void* dA) { return l == 0 ? (const char*)dA : h->sh.lv[l].dW; }
static inline long level_ld(const tqr_tsqr* h, int l, long ldda) { return l == 0 ? ldda : h->sh.lv[l].ld; }

// T factors of every domain of level l; domains beyond a grid's y in consecutive launches
static int launch_prepare(tqr_tsqr* h, int l, const void* dA, long ldda, hipStream_t cs) {
  const TsqrShape& s = h->sh;
  const TsqrLevel& L = s.lv[l];
  const int p = L.rows / s.b, kmax = s.n / s.b;
  ApplyBatchArgs ba;
  ba.a.C = nullptr; ba.a.lda = level_ld(h, l, ldda); ba.a.ldc = 0;
  ba.a.m = L.rows; ba.a.p = p; ba.a.kmax = kmax; ba.a.nrhs = 0;
  ba.sA = L.rows; ba.sTau = (long long)L.rows * kmax; ba.sC = 0; ba.sTw = (long long)L.tper;
  const unsigned grid = (unsigned)(L.tper / timg_doubles(s.b));
  for (int d0 = 0; d0 < L.ndom; d0 += kMaxGridY) {
    const unsigned nd = (unsigned)std::min(kMaxGridY, L.ndom - d0);
    ba.a.A = level_mat(h, l, dA) + (size_t)d0 * L.rows * s.es;
    ba.a.tau = L.dTau + (size_t)d0 * L.rows * kmax * s.es;
    ba.a.Tw = L.dT + (size_t)d0 * L.tper;
    hipLaunchKernelGGL(h->k.kt, dim3(grid, nd), dim3(NT), lds_apply_t(s.b), cs, ba);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

// Q^T (trans) or Q of every domain of level l on the level's C: the caller's (l == 0) or C_l
static int launch_apply(tqr_tsqr* h, int l, int trans, const void* dA, long ldda, void* dC, long lddc, int nrhs,
                        hipStream_t cs) {
  const TsqrShape& s = h->sh;
  const TsqrLevel& L = s.lv[l];
  const int p = L.rows / s.b, kmax = s.n / s.b;
  char* C = l == 0 ? (char*)dC : L.dC;
  ApplyBatchArgs ba;
  ba.a.tau = nullptr; ba.a.lda = level_ld(h, l, ldda); ba.a.ldc = l == 0 ? lddc : L.ld;
  ba.a.m = L.rows; ba.a.p = p; ba.a.kmax = kmax; ba.a.nrhs = nrhs;
  ba.sA = L.rows; ba.sTau = 0; ba.sC = L.rows; ba.sTw = (long long)L.tper;
  const unsigned grid = ((unsigned)nrhs + 63u) / 64u;
  for (int d0 = 0; d0 < L.ndom; d0 += kMaxGridY) {
    const unsigned nd = (unsigned)std::min(kMaxGridY, L.ndom - d0);
    ba.a.A = level_mat(h, l, dA) + (size_t)d0 * L.rows * s.es;
    ba.a.C = C + (size_t)d0 * L.rows * s.es;
    ba.a.Tw = L.dT + (size_t)d0 * L.tper;
    hipLaunchKernelGGL(trans == TQR_TRANS ? h->k.kqt : h->k.kqn, dim3(grid, nd), dim3(NT), lds_apply_q(s.b), cs, ba);
    HIPCHK(hipGetLastError());
  }
  return TQR_OK;
}

// C_l <- the top n rows of level l-1's domains (zero padding), or the way back
static int launch_c_copy(tqr_tsqr* h, int l, bool up, void* dC, long lddc, int nrhs, hipStream_t cs) {
  const TsqrShape& s = h->sh;
  const TsqrLevel& L = s.lv[l];
  const TsqrLevel& Lp = s.lv[l - 1];
  char* below = l == 1 ? (char*)dC : Lp.dC;
  const long ldb = l == 1 ? lddc : Lp.ld;
  CopyArgs c;
  c.n = s.n; c.ncols = nrhs; c.nblk = Lp.ndom; c.dom = Lp.rows;
  if (up) {
    c.src = below; c.lds = ldb; c.dst = L.dC; c.ldd = L.ld; c.rows = L.ld;
    return launch_copy(h->k.grect, c, cs);
  }
  c.src = L.dC; c.lds = L.ld; c.dst = below; c.ldd = ldb; c.rows = (long)Lp.ndom * s.n;
  return launch_copy(h->k.srect, c, cs);
}

static int enqueue_factor(tqr_tsqr* h, void* dA, int ldda, hipStream_t cs) {
  const TsqrShape& s = h->sh;
  const int kmax = s.n / s.b, nlev = (int)s.lv.size();
  int st;
  for (int l = 0; l < nlev; ++l) {
    const TsqrLevel& L = s.lv[l];
    if (l > 0) {
      const TsqrLevel& Lp = s.lv[l - 1];
      CopyArgs c;
      c.src = level_mat(h, l - 1, dA); c.lds = level_ld(h, l - 1, ldda); c.dst = L.dW; c.ldd = L.ld;
      c.rows = L.ld; c.dom = Lp.rows; c.n = s.n; c.ncols = s.n; c.nblk = Lp.ndom;
      if ((st = launch_copy(h->k.gtri, c, cs)) != TQR_OK) return st;
    }
    void* mat = l == 0 ? dA : (void*)L.dW;
    if ((st = tqr_batch_execute(L.bt, mat, (int)level_ld(h, l, ldda), L.rows, L.dTau, (long long)L.rows * kmax, cs)) != TQR_OK)
      return st;
    if ((st = launch_prepare(h, l, dA, ldda, cs)) != TQR_OK) return st;
  }
  if (nlev > 1) {
    const TsqrLevel& L = s.lv[nlev - 1];
    CopyArgs c;
    c.src = L.dW; c.lds = L.ld; c.dst = dA; c.ldd = ldda; c.rows = s.n; c.dom = s.m_dom; c.n = s.n; c.ncols = s.n;
    c.nblk = 1;
    if ((st = launch_copy(h->k.stri, c, cs)) != TQR_OK) return st;
  }
  return TQR_OK;
}

static int enqueue_apply(tqr_tsqr* h, int trans, const void* dA, int ldda, void* dC, int nrhs, int lddc, hipStream_t cs) {
  const int nlev = (int)h->sh.lv.size();
  int st;
  if (trans == TQR_TRANS) {
    if ((st = launch_apply(h, 0, trans, dA, ldda, dC, lddc, nrhs, cs)) != TQR_OK) return st;
    for (int l = 1; l < nlev; ++l) {
      if ((st = launch_c_copy(h, l, true, dC, lddc, nrhs, cs)) != TQR_OK) return st;
      if ((st = launch_apply(h, l, trans, dA, ldda, dC, lddc, nrhs, cs)) != TQR_OK) return st;
    }
    for (int l = nlev - 1; l >= 1; --l)
      if ((st = launch_c_copy(h, l, false, dC, lddc, nrhs, cs)) != TQR_OK) return st;
    return TQR_OK;
  }
  for (int l = 1; l < nlev; ++l)
    if ((st = launch_c_copy(h, l, true, dC, lddc, nrhs, cs)) != TQR_OK) return st;
  for (int l = nlev - 1; l >= 1; --l) {
    if ((st = launch_apply(h, l, trans, dA, ldda, dC, lddc, nrhs, cs)) != TQR_OK) return st;
    if ((st = launch_c_copy(h, l, false, dC, lddc, nrhs, cs)) != TQR_OK) return st;
  }
  return launch_apply(h, 0, trans, dA, ldda, dC, lddc, nrhs, cs);
}

// The frame of every enqueueing call: mutual exclusion, the stream waits for the handle's previous
// call, and the call is marked also behind a partly failed enqueue. `need_factor`: TQR_EINVAL before
// the first factor.
template <typename F>
static int tsqr_call(tqr_tsqr* h, bool need_factor, void* stream, F enqueue) {
  if (!h->ready) return TQR_ENODEV;
  hipStream_t cs = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(h->mu);
  if (need_factor && !h->factored) return TQR_EINVAL;
  HIPCHK(hipStreamWaitEvent(cs, h->evDone, 0));
  const int st = enqueue(cs);
  const hipError_t e = hipEventRecord(h->evDone, cs);
  if (st != TQR_OK) return st;
  HIPCHK(e);
  return TQR_OK;
}

// argument errors shared by apply_q / form_q / lstsq: pointers, widths, leading dimensions
static bool tsqr_args_ok(const tqr_tsqr* h, const void* dA, int ldda, const void* dC, int nrhs, int lddc) {
  return h && dA && dC && nrhs >= 1 && nrhs <= h->sh.nrhs_max && ldda >= h->sh.m && lddc >= h->sh.m &&
         valid_ld(ldda, h->sh.es) && valid_ld(lddc, h->sh.es);
}

extern "C" {

int tqr_tsqr_plan(const tqr_tsqr_spec* spec, int* m_dom, int* fan, int* nlevels, int* domains, int cap, size_t* ws_bytes) {
  TsqrShape sh;
  const int st = tsqr_resolve(spec, &sh);
  if (st != TQR_OK) return st;
  if (m_dom) *m_dom = sh.m_dom;
  if (fan) *fan = sh.fan;
  if (nlevels) *nlevels = (int)sh.lv.size();
  if (domains)
    for (int l = 0; l < (int)sh.lv.size() && l < cap; ++l) domains[l] = sh.lv[l].ndom;
  if (ws_bytes) *ws_bytes = sh.ws_bytes;
  return TQR_OK;
}

void tqr_tsqr_destroy(tqr_tsqr* h) {
  if (!h) return;
  if (h->evDone) {
    (void)hipEventSynchronize(h->evDone);  // the last call may still be using the workspaces
    (void)hipEventDestroy(h->evDone);
  }
  for (TsqrLevel& L : h->sh.lv)
    if (L.bt) tqr_batch_destroy(L.bt);
  if (h->d_mem) (void)hipFree(h->d_mem);
  delete h;
}

int tqr_tsqr_create(tqr_tsqr** out, const tqr_tsqr_spec* spec) {
  if (!out) return TQR_EINVAL;
  *out = nullptr;
  tqr_tsqr* h = new (std::nothrow) tqr_tsqr();
  if (!h) return TQR_ENOMEM;
  int st = tsqr_resolve(spec, &h->sh);
  if (st != TQR_OK) { delete h; return st; }
  TsqrShape& s = h->sh;
  for (TsqrLevel& L : s.lv)
    if ((st = tqr_batch_create(&L.bt, L.rows, s.n, s.b, s.dtype, L.ndom, s.ws_limit)) != TQR_OK) {
      tqr_tsqr_destroy(h);
      return st;
    }
  // without a gfx950 the handle exists, holds no device memory, and every enqueueing call returns TQR_ENODEV
  if (current_device_is_gfx950() != TQR_OK) { *out = h; return TQR_OK; }
  dispatch_b(s.b, [&](auto bb) {
    if (s.dtype == TQR_F64) tsqr_kernels<decltype(bb)::value, double>(&h->k);
    else tsqr_kernels<decltype(bb)::value, float>(&h->k);
  });
  if (hipFuncSetAttribute((const void*)h->k.kt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_t(s.b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)h->k.kqt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(s.b)) != hipSuccess ||
      hipFuncSetAttribute((const void*)h->k.kqn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply_q(s.b)) != hipSuccess ||
      hipEventCreateWithFlags(&h->evDone, hipEventDisableTiming) != hipSuccess) {
    tqr_tsqr_destroy(h);
    return TQR_EHIP;
  }
  if (hipMalloc(&h->d_mem, std::max<size_t>(256, s.own_bytes)) != hipSuccess) {
    (void)hipGetLastError();
    tqr_tsqr_destroy(h);
    return TQR_ENOMEM;
  }
  char* at = h->d_mem;
  for (TsqrLevel& L : s.lv) {
    L.dTau = at; at += L.bTau;
    L.dT = (double*)at; at += L.bT;
    if (L.bW) { L.dW = at; at += L.bW; }
    if (L.bC) { L.dC = at; at += L.bC; }
  }
  h->ready = true;
  *out = h;
  return TQR_OK;
}

size_t tqr_tsqr_workspace_bytes(const tqr_tsqr* h) { return h ? h->sh.ws_bytes : 0; }

int tqr_tsqr_level(const tqr_tsqr* h, int level, void** dW, int* ldw, void** dtau, int* dom_rows, int* ndom) {
  if (!h || level < 0 || level >= (int)h->sh.lv.size()) return TQR_EINVAL;
  const TsqrLevel& L = h->sh.lv[level];
  if (dW) *dW = L.dW;
  if (ldw) *ldw = (int)L.ld;
  if (dtau) *dtau = L.dTau;
  if (dom_rows) *dom_rows = L.rows;
  if (ndom) *ndom = L.ndom;
  return TQR_OK;
}

int tqr_tsqr_factor(tqr_tsqr* h, void* dA, int ldda, void* stream) {
  if (!h || !dA || ldda < h->sh.m || !valid_ld(ldda, h->sh.es)) return TQR_EINVAL;
  return tsqr_call(h, false, stream, [&](hipStream_t cs) -> int {
    const int st = enqueue_factor(h, dA, ldda, cs);
    if (st == TQR_OK) h->factored = true;
    return st;
  });
}

int tqr_tsqr_apply_q(tqr_tsqr* h, int trans, const void* dA, int ldda, void* dC, int nrhs, int lddc, void* stream) {
  if (!tsqr_args_ok(h, dA, ldda, dC, nrhs, lddc) || (trans != TQR_NOTRANS && trans != TQR_TRANS)) return TQR_EINVAL;
  return tsqr_call(h, true, stream, [&](hipStream_t cs) -> int { return enqueue_apply(h, trans, dA, ldda, dC, nrhs, lddc, cs); });
}

int tqr_tsqr_form_q(tqr_tsqr* h, const void* dA, int ldda, void* dQ, int lddq, void* stream) {
  if (!h || !tsqr_args_ok(h, dA, ldda, dQ, h->sh.n, lddq)) return TQR_EINVAL;
  return tsqr_call(h, true, stream, [&](hipStream_t cs) -> int {
    CopyArgs c;
    c.src = nullptr; c.lds = 0; c.dst = dQ; c.ldd = lddq; c.rows = h->sh.m; c.dom = 0; c.n = h->sh.n; c.ncols = h->sh.n;
    c.nblk = 0;
    const int st = launch_copy(h->k.fill, c, cs);
    if (st != TQR_OK) return st;
    return enqueue_apply(h, TQR_NOTRANS, dA, ldda, dQ, h->sh.n, lddq, cs);
  });
}

int tqr_tsqr_lstsq(tqr_tsqr* h, int trans, const void* dA, int ldda, void* dB, int nrhs, int lddb, void* dres, void* stream) {
  if (!tsqr_args_ok(h, dA, ldda, dB, nrhs, lddb) || (trans != TQR_NOTRANS && trans != TQR_TRANS)) return TQR_EINVAL;
  const TsqrShape& s = h->sh;
  return tsqr_call(h, true, stream, [&](hipStream_t cs) -> int {
    int st;
    if (trans == TQR_NOTRANS) {
      // B <- Q^T B; rows 0 .. n-1 <- R^{-1} of them; the residual norms from rows n .. m-1
      if ((st = enqueue_apply(h, TQR_TRANS, dA, ldda, dB, nrhs, lddb, cs)) != TQR_OK) return st;
      if ((st = tqr_trsm_r(s.dtype, TQR_NOTRANS, s.n, s.b, dA, ldda, dB, nrhs, lddb, cs)) != TQR_OK) return st;
      return dres ? resnorm(s.dtype, dB, lddb, s.n, s.m, nrhs, dres, cs) : (int)TQR_OK;
    }
    // x = Q [R^{-T} c; 0]
    if (s.m > s.n)
      HIPCHK(hipMemset2DAsync((char*)dB + (size_t)s.n * s.es, (size_t)lddb * s.es, 0, (size_t)(s.m - s.n) * s.es, (size_t)nrhs, cs));
    if ((st = tqr_trsm_r(s.dtype, TQR_TRANS, s.n, s.b, dA, ldda, dB, nrhs, lddb, cs)) != TQR_OK) return st;
    return enqueue_apply(h, TQR_NOTRANS, dA, ldda, dB, nrhs, lddb, cs);
  });
}

}  // extern "C"
