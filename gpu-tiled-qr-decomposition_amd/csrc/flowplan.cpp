// Host planner of the persistent engine's task list (flowplan.hpp): the order knobs and their
// defaults, the start-time estimator that orders the list, the multi-GPU partition, the
// topological check, and the host-only C entry points that describe a list without a GPU.
#include "flowplan.hpp"

#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <queue>
#include <string>
#include <tuple>
#include <unordered_map>

#include "gridscheduler.h"

namespace tqr {

int flow_shape(int dtype, int b) {
  if (dtype != TQR_F64) return 8;
  const char* e = getenv("TQR_FLOW_SHAPE");
  if (e && strcmp(e, "w4") == 0) return 4;
  if (e && strcmp(e, "r") == 0 && b == 256) return 5;
  return 8;
}

// Is a flow task list topological for the engine's in-task waits? Every task must come after
// every task it waits on (in-order dequeue then guarantees progress, flow.hpp header):
//   panel (i,k):        panel (i-1,k); the chain segments of step k-1, column k, holding row i;
//   chain (k,j,s,e):    segment e-1 (head rows) or, for e = 0, GEQRT(k) and the step-(k-1)
//                       segment holding row k; for each of its rows i: panel (i,k) and the
//                       step-(k-1) segment holding row i.
// Segment boundaries are read from the list itself (any segment lengths).
// Host-pointer API lists (xfer.hpp) also hold UP(j, c) / DOWN(j, c): every step-0 task of tile
// column j (GEQRT(0) / TSQRT(i, 0) for j = 0, the chains of step 0 on j) must come after all
// UP(j, *); DOWN(j, c) after every chain of a step k < j on column j and every panel task of step j.
// (the positions are kept in hash maps under packed keys: k, s, e and the rows of a chain are 16-bit
// or narrower fields of the task word, a panel's row is any int, and steps and tile columns are
// checked against q <= 65536)
namespace {
using u64 = unsigned long long;
inline u64 key_panel(int i, int k) { return (u64)(unsigned)i << 24 | (u64)k; }                                      // k < q
inline u64 key_chain(int k, int j, int s, int x) { return (u64)k << 48 | (u64)j << 24 | (u64)s << 16 | (u64)(x & 0xffff); }  // x: e or row
}  // namespace
bool flow_list_topological(const std::vector<Item>& L, int p, int q, int ns) {
  if (q > (1 << 16)) return false;  // (a chain's step is a 16-bit field: no list of a wider grid exists)
  std::unordered_map<u64, int> ppos, cpos, rowpos;               // (i, k) / (k, j, s, e) / (k, j, s, row) -> position
  ppos.reserve(L.size());
  cpos.reserve(L.size());
  rowpos.reserve(4 * L.size());
  std::map<std::pair<int, int>, int> upos, dpos;                 // (j, c) -> position
  std::vector<int> uplast(q, -1);                                // last UP(j, *) of column j
  std::vector<int> collast(q, -1);                               // last task DOWN(j, *) waits for
  for (int x = 0; x < (int)L.size(); ++x) {
    const Item& it = L[x];
    const int ty = it.ts & 0xff;
    if (ty == T_CHAIN) {
      const int s = (it.ts >> 8) & 0xff, k = it.k & 0xffff, e = it.k >> 16, j = it.m, i0 = it.l & 0xffff, i1 = it.l >> 16;
      if (j < 0 || j >= q) return false;
      if (!cpos.emplace(key_chain(k, j, s, e), x).second) return false;
      if (e == 0) rowpos[key_chain(k, j, s, k)] = x;
      for (int i = i0; i < i1; ++i) rowpos[key_chain(k, j, s, i)] = x;
      if (k < j) collast[j] = std::max(collast[j], x);
    } else if (ty == QRS || ty == QRD) {
      if (it.k < 0 || it.k >= q) return false;
      if (!ppos.emplace(key_panel(it.l, it.k), x).second) return false;
      collast[it.k] = std::max(collast[it.k], x);
    } else if (ty == T_UP || ty == T_DOWN) {
      if (it.m < 0 || it.m >= q) return false;
      auto& mp = ty == T_UP ? upos : dpos;
      if (!mp.emplace(std::make_pair(it.m, (it.ts >> 8) & 0xff), x).second) return false;
      if (ty == T_UP) uplast[it.m] = std::max(uplast[it.m], x);
    } else {
      return false;
    }
  }
  auto before = [&](auto& mp, const auto& key, int x) {
    auto f = mp.find(key);
    return f != mp.end() && f->second < x;
  };
  const bool xfer = !upos.empty();
  if (xfer) {  // every column uploaded and downloaded by the same number of chunks
    const int nxc = (int)upos.size() / q;
    if ((int)upos.size() != nxc * q || dpos.size() != upos.size()) return false;
    for (int j = 0; j < q; ++j)
      for (int c = 0; c < nxc; ++c)
        if (!upos.count(std::make_pair(j, c)) || !dpos.count(std::make_pair(j, c))) return false;
  } else if (!dpos.empty()) {
    return false;
  }
  for (int x = 0; x < (int)L.size(); ++x) {
    const Item& it = L[x];
    const int ty = it.ts & 0xff;
    if (ty == T_CHAIN) {
      const int s = (it.ts >> 8) & 0xff, k = it.k & 0xffff, e = it.k >> 16, j = it.m, i0 = it.l & 0xffff, i1 = it.l >> 16;
      if (e > 0 && !before(cpos, key_chain(k, j, s, e - 1), x)) return false;
      if (e == 0 && !before(ppos, key_panel(k, k), x)) return false;
      if (e == 0 && k > 0 && !before(rowpos, key_chain(k - 1, j, s, k), x)) return false;
      if (xfer && k == 0 && !(uplast[j] < x)) return false;
      for (int i = i0; i < i1; ++i) {
        if (!before(ppos, key_panel(i, k), x)) return false;
        if (k > 0 && !before(rowpos, key_chain(k - 1, j, s, i), x)) return false;
      }
    } else if (ty == T_DOWN) {
      if (!(collast[it.m] < x)) return false;
    } else if (ty == QRS || ty == QRD) {
      const int i = it.l, k = it.k;
      if (i > k && !before(ppos, key_panel(i - 1, k), x)) return false;
      if (xfer && k == 0 && !(uplast[0] < x)) return false;
      if (k > 0)
        for (int s = 0; s < ns; ++s)
          if (!before(rowpos, key_chain(k - 1, k, s, i), x)) return false;
    }
  }
  (void)p;
  return true;
}

// Default tail (fp64 storage): the steps whose columns have at most kTailRows rows below the
// diagonal, i.e. whose chains are short and on the critical path. One element per segment lets a
// column's elements run on different workgroups, pipelined group by group through the head rows
// (Ac), instead of one after the other in one workgroup. Measured at 16384^2 (64 steps): tail 32
// 122.7-122.8 ms against 124.7-124.9 (24: 124.0, 40: 122.9-123.3, 48: 124.2-124.3; profiles/r04/
// tail/). fp32 storage keeps its head strip in registers across a segment, so one-element segments
// add a head load and store per element there: no gain at 16-32 steps of 128, slower beyond
// (48: +2.3 ms) — off for fp32. Tall matrices (65536 x 16384) never reach the tail rows.
constexpr int kTailRows = 31;
static int default_tail(int p, int kmax, int dtype) {
  if (dtype != TQR_F64) return 0;
  return std::max(0, std::min(kmax, kmax - (p - 1 - kTailRows)));
}
// Default panel lookahead (TQR_LA, chain elements): 2 for fp32 storage, whose run is paced by the
// panel groups (c5 465.8-466.4 vs 467.2-467.3 ms, two alternating rounds; 4: 466.2-466.5, 6:
// 467.7; round 4's earlier 4 vs 0: 469.0-469.1 vs 470.4-470.7), 0 for fp64 (2: +0.1-0.2 ms;
// profiles/r04/la_f32/).
static double default_la(int dtype) { return dtype == TQR_F32 ? 2.0 : 0.0; }
// Multi-rank defaults (4+ ranks, each launch covering its whole device — the plans of the 8-GPU
// run): besides 2-element segments (env_seglen), one-element segments in the last 7/16 of the steps
// (28 of 64 at 65536x16384) and the lookahead column's chains keyed 4 elements earlier. The model
// with round-5 chain costs (tools/sched_sim.py dist5): S(8) 6.41 against 6.16 with
// 2-element segments alone (tail 24 / 32: 6.35 / 6.39 with the keying, 6.38 at 32 without).
// Round 6 calibrated the model against the one-GPU rehearsals (tools/sched_sim.py calib,
// profiles/r06/model): measured / model 1.032-1.053 for 2 and 4 ranks; with that error the 8-GPU
// time is 92.0-93.9 ms with these defaults against 95.6-97.6 ms with 2-element segments alone
// (S(8) 6.19-6.32 vs 5.96-6.08), and the 4-rank rehearsal with these lists forced was predicted
// slower (602.8 vs 572.0 ms model) and measured slower (621.8 vs 602.1 ms) — the model carries the
// direction of the one-GPU cost; its 8-GPU gain (3.8 %) is a scale-free comparison of two lists
// under the same error. The lone UNMQR segments do not follow the tail on these plans (the model:
// no difference at 8 ranks, 89.2 ms either way): one-GPU plans only. TQR_DIST_DEFAULTS=r4 drops the
// 7/16 tail and the earlier keying (2-element segments only) for an A/B on an 8-GPU node. It is NOT
// round 4's list exactly: it takes the 2- and 3-rank branch below, whose ualone is 0, where round 4's
// lone UNMQR segments followed the tail.
struct MultiRankDefaults {
  int tail;
  double lac;   // < 0: the panel keying (TQR_LA's default)
  int ualone;   // < 0: follow the tail
};
static MultiRankDefaults multi_rank_defaults(int p, int kmax, int dtype, int world, bool full) {
  const char* e = getenv("TQR_DIST_DEFAULTS");
  const bool r4 = e && std::string(e) == "r4";
  if (world >= 4 && full && !r4) return {std::max(default_tail(p, kmax, dtype), 7 * kmax / 16), 4.0, 0};
  if (world > 1) return {default_tail(p, kmax, dtype), -1.0, 0};
  return {default_tail(p, kmax, dtype), -1.0, -1};
}
static FlowKnobs knobs_from_env(int seglen, int tail_default, double la_default, double lac_default, int ualone_default) {
  FlowKnobs kn;
  kn.seglen = std::max(1, seglen);
  kn.tail = tail_default;
  kn.la = la_default;
  const char* esl = getenv("TQR_SEGLEN_LA");
  kn.seglen_la = esl ? std::max(1, atoi(esl)) : kn.seglen;
  const char* e = getenv("TQR_LA_TAIL");
  kn.la_tail = e ? std::max(0, atoi(e)) : 0;
  if (const char* et = getenv("TQR_TAIL")) kn.tail = std::max(0, atoi(et));
  if (const char* ets = getenv("TQR_TAIL_SEGLEN")) kn.tail_sl = std::max(1, atoi(ets));
  kn.ualone = ualone_default >= 0 ? ualone_default : kn.tail;
  if (const char* eua = getenv("TQR_UNMQR_ALONE")) kn.ualone = std::max(0, atoi(eua));
  if (const char* eg = getenv("TQR_TG")) kn.Tg = atof(eg);
  if (const char* el = getenv("TQR_LAZY")) kn.lazy = atof(el);
  if (const char* ela = getenv("TQR_LA")) kn.la = atof(ela);
  kn.lac = lac_default >= 0.0 ? lac_default : kn.la;
  if (const char* elac = getenv("TQR_LAC")) kn.lac = atof(elac);  // lookahead column's chains (default: TQR_LA)
  return kn;
}
// Default window of the deep-lookahead order (window_order; TQR_DEPTH) by the plan's steps: a quarter
// of the steps plus 4, kept below the number of steps that precede the one-element tail, and only for
// 44 to 80 steps of a matrix that is not taller than wide (its last `tail` = kTailRows + 1 steps are
// the latency-bound ones the window is for). Measured on one MI355X, fp64, b = 256, alternating
// against depth 0, best of the depths tried in ms (profiles/window/depth_by_size.md): 44 steps -2.3
// at depth 11 (15: -0.5), 48 -3.2 at 16, 56 -3.9 at 18, 64 -3.6 at 20, 72 -3.1 at 22, 80 -1.3 at 24
// (of 219); 40 steps -0.7 at 6 and nothing at 12-14, 88 -1.0 at 22 and -0.5 at 26 (within the runs'
// spread), 96 nothing at 8-32. The model (tools/sched_sim.py window) has its best depth at 16-24 for
// 64 steps and predicts the gain at 44-72 steps, but also -3 ms at 80-96 steps, which the hardware
// does not give: the upper limit is the measured one. Taller than wide loses in both (96x64 tiles:
// +3.4 ms, model +0.6; 256x64: +26 ms): such a run has no latency-bound tail to hide, and the
// window only takes the bulk's workgroups early.
constexpr int kDepthMinSteps = 44, kDepthMaxSteps = 80;
static int default_depth(int kmax, int tail) {
  if (kmax < kDepthMinSteps || kmax > kDepthMaxSteps || tail != kTailRows + 1) return 0;
  return std::min(kmax / 4 + 4, kmax - tail - 1);
}
// Chain segment length (elements per chain task; TQR_SEGLEN overrides). 8, except for 4 and more
// ranks with a whole device each (1024+ workgroups in all): 2 — more, shorter chain tasks give
// each rank work it can start while its columns' wavefronts (the head rows going down a column)
// wait on other ranks' panels. The model of the 8-GPU run (tools/sched_sim_seglen.py, per-segment
// cost calibrated on one MI355X) gives S(8) 6.17 at length 2 against 5.44 at 8; one GPU pays
// 4.6 % for length 2 (65536x16384: 635.3 vs 607.6 ms), and so do the one-GPU rehearsals (4 ranks
// x 64 CUs: 645.8 vs 628.8 ms; model 600.5 vs 575.1), whose ranks have work to spare.
// full: the rank's launch covers its whole device (every rank must decide alike — tqr_dist_import
// checks the ranks' task-list signatures).
static int env_seglen(int world, bool full) {
  const char* sl = getenv("TQR_SEGLEN");
  return sl ? std::max(1, atoi(sl)) : (world >= 4 && full ? 2 : 8);
}
FlowKnobs flow_knobs(int p, int q, int dtype, int world, bool full, int seglen, int steps, int b) {
  const int kmax = flow_kmax(p, q, steps);
  const MultiRankDefaults mrd = multi_rank_defaults(p, kmax, dtype, world, full);
  FlowKnobs kn = knobs_from_env(seglen > 0 ? seglen : env_seglen(world, full), mrd.tail, default_la(dtype), mrd.lac, mrd.ualone);
  // the deep-lookahead default: only where window_order's costs were measured — one rank on a whole
  // device, fp64 storage, the 8-wave shape at b = 256 (8 groups, 2 strips), 8-element segments, no
  // step cap (the host-pointer list never takes the pass: build_flow_plan); TQR_DEPTH forces any
  // one-rank device list
  const bool measured = world == 1 && full && dtype == TQR_F64 && b == 256 && flow_shape(dtype, b) == 8 && kn.seglen == 8 &&
                        (steps <= 0 || steps >= std::min(p, q));  // (a cap at every step is tqr_plan_create's list, tqr.h)
  kn.depth = measured ? default_depth(kmax, kn.tail) : 0;
  if (const char* ed = getenv("TQR_DEPTH"); ed && world == 1) kn.depth = std::max(0, atoi(ed));
  return kn;
}

void build_flow_plan(int p, int q, int ns, int ng, const FlowKnobs& kn, FlowPlan& fp, const XferPlan* xp, int steps) {
  const int kmax = flow_kmax(p, q, steps);
  // segment length per chain: shorter segments for the lookahead column pipeline consecutive
  // elements on different workgroups at reflector-group granularity
  auto seglen_of = [&](int k, int j) { return seglen_of_chain(k, j, kmax, kn.seglen, kn.seglen_la, kn.la_tail, kn.tail, kn.tail_sl); };
  // host-pointer API: tile column j arrives (uploaded) at arrive(j); step-0 tasks start after it
  const bool xfer = xp && xp->nxc > 0;
  auto arrive = [&](int j) { return xfer ? (j + 1) * xp->tcol : 0.0; };
  // cost model (unit: one chain element): Tg = one panel group-step; tunable for experiments
  const double Tg = kn.Tg, Te = 1.0;
  const double lazy = kn.lazy;
  // lookahead (TQR_LA / TQR_LAC, unit: chain elements): panel tasks / the lookahead column's
  // chains are keyed this much earlier than their estimate (the critical path first)
  const double la = kn.la;
  const double lac = kn.lac;
  // fin_elem[k][i][j] (strips move together in the estimate): finish of chain element (i,j,k)
  auto id3 = [&](int k, int i, int j) { return ((size_t)k * p + i) * q + j; };
  std::vector<double> fin((size_t)kmax * p * q, 0.0), pstart((size_t)kmax * p, 0.0);
  auto fin_prev = [&](int k, int i, int j) { return k > 0 ? fin[id3(k - 1, i, j)] : 0.0; };
  struct T { double est; int ord; Item it; };
  std::vector<T> tl;
  if (xfer)  // uploads, in column order (one column's chunks together: they share the link)
    for (int j = 0; j < q; ++j)
      for (int c = 0; c < xp->nxc; ++c) tl.push_back({arrive(j) - xp->tcol, -1, Item{T_UP | (c << 8), 0, j, 0}});
  for (int k = 0; k < kmax; ++k) {
    // panel
    double ps = std::max(fin_prev(k, k, k), k == 0 ? arrive(0) : 0.0);
    pstart[(size_t)k * p + k] = ps;
    tl.push_back({ps - la, 0, Item{QRS, k, k, k}});
    for (int i = k + 1; i < p; ++i) {
      double st = std::max(fin_prev(k, i, k), pstart[(size_t)k * p + i - 1] + Tg);
      pstart[(size_t)k * p + i] = st;
      tl.push_back({st - la, 0, Item{QRD, i, k, k}});
    }
    // chains
    for (int j = k + 1; j < q; ++j) {
      double t0 = std::max({fin_prev(k, k, j), pstart[(size_t)k * p + k] + Tg, k == 0 ? arrive(j) : 0.0});
      double prev = t0 + 0.5 * Te;  // UNMQR
      fin[id3(k, k, j)] = prev;
      std::vector<double> seg_start;
      seg_start.push_back(t0);
      const int seglen = seglen_of(k, j);
      const bool ua = unmqr_alone(k, j, kmax, kn.ualone) && p - k - 1 > 0;  // segment 0: the UNMQR alone
      for (int i = k + 1; i < p; ++i) {
        double st = std::max({prev, fin_prev(k, i, j), pstart[(size_t)k * p + i] + Tg});
        if ((i - k - 1) % seglen == 0 && i > k + 1) seg_start.push_back(st);
        double f = std::max(st + Te, pstart[(size_t)k * p + i] + ng * Tg + Te / ng);
        fin[id3(k, i, j)] = f;
        prev = f;
      }
      const int nseg = nseg_of_chain(k, j, p, kmax, seglen, kn.ualone);
      if (ua) seg_start.insert(seg_start.begin(), t0);
      for (int e = 0; e < nseg; ++e) {
        const int er = ua ? e - 1 : e;  // the segment's run of rows
        int i0 = k + 1 + er * seglen, i1 = std::min(p, i0 + seglen);
        if (p - k - 1 == 0) { i0 = p; i1 = p; }
        if (er < 0) i0 = i1 = k + 1;  // (the UNMQR-only segment: no rows)
        // lazy keys (TQR_LAZY, default 1): a segment of a non-lookahead column is keyed by the
        // estimated completion of its first panel member, so a workgroup does not dequeue it
        // long before its V/T images exist (it would wait group by group); the lookahead
        // column k+1 feeds the next panel and stays eager
        double key = seg_start[std::min<size_t>(e, seg_start.size() - 1)];
        if (lazy > 0 && j != k + 1 && i0 < p) key = std::max(key, pstart[(size_t)k * p + i0] + lazy * ng * Tg);
        if (j == k + 1) key -= lac;
        for (int s = 0; s < ns; ++s)
          tl.push_back({key, 1,
                        Item{T_CHAIN | (s << 8), i0 | (i1 << 16), j, k | (e << 16)}});
      }
    }
  }
  if (xfer) {  // downloads: when tile column j is final (its last chain element, its panel)
    for (int j = 0; j < q; ++j) {
      double cf = 0.0;
      for (int k = 0; k < std::min(j, kmax); ++k) cf = std::max(cf, fin[id3(k, p - 1 > k ? p - 1 : k, j)]);
      if (j < kmax) cf = std::max(cf, pstart[(size_t)j * p + p - 1] + ng * Tg);
      for (int c = 0; c < xp->nxc; ++c) tl.push_back({cf, 2, Item{T_DOWN | (c << 8), 0, j, 0}});
    }
  }
  // bump every task's key past its dependencies' keys (tl is topological), so the
  // estimated-time order is topological by construction
  fp.missed = 0;
  {
    std::map<std::tuple<int, int, int, int, int>, int> idx;
    for (int x = 0; x < (int)tl.size(); ++x) {
      const Item& it = tl[x].it;
      int ty = it.ts & 0xff;
      if (ty == T_CHAIN) idx[std::make_tuple(T_CHAIN, it.k & 0xffff, it.m, (it.ts >> 8) & 0xff, it.k >> 16)] = x;
      else if (ty == T_UP || ty == T_DOWN) idx[std::make_tuple(ty, it.m, (it.ts >> 8) & 0xff, 0, 0)] = x;
      else idx[std::make_tuple(0, it.l, it.k, 0, 0)] = x;
    }
    auto seg_of = [&](int k, int j, int i) { return seg_of_row(k, j, i, kmax, seglen_of(k, j), kn.ualone); };
    auto nseg_of = [&](int k, int j) { return nseg_of_chain(k, j, p, kmax, seglen_of(k, j), kn.ualone); };
    for (int x = 0; x < (int)tl.size(); ++x) {
      const Item& it = tl[x].it;
      int ty = it.ts & 0xff;
      double key = tl[x].est;
      // (a dependency that is not in the list is a planner bug: counted, and the plan then takes the
      // step-major order below instead of bumping against some other task)
      auto bump = [&](const std::tuple<int, int, int, int, int>& dep) {
        const auto f = idx.find(dep);
        if (f == idx.end()) ++fp.missed;
        else key = std::max(key, tl[f->second].est + 1e-6);
      };
      auto bump_up = [&](int j) {
        if (xfer)
          for (int c = 0; c < xp->nxc; ++c) bump(std::make_tuple(T_UP, j, c, 0, 0));
      };
      if (ty == T_CHAIN) {
        int s = (it.ts >> 8) & 0xff, k = it.k & 0xffff, e = it.k >> 16, j = it.m, i0 = it.l & 0xffff, i1 = it.l >> 16;
        if (e > 0) bump(std::make_tuple(T_CHAIN, k, j, s, e - 1));
        else bump(std::make_tuple(0, k, k, 0, 0));
        if (e == 0 && k > 0) bump(std::make_tuple(T_CHAIN, k - 1, j, s, seg_of(k - 1, j, k)));
        if (k == 0) bump_up(j);
        for (int i = i0; i < i1; ++i) {
          bump(std::make_tuple(0, i, k, 0, 0));
          if (k > 0) bump(std::make_tuple(T_CHAIN, k - 1, j, s, seg_of(k - 1, j, i)));
        }
      } else if (ty == T_UP) {
      } else if (ty == T_DOWN) {
        const int j = it.m;
        for (int k = 0; k < std::min(j, kmax); ++k)
          for (int s = 0; s < ns; ++s)
            for (int e = 0; e < nseg_of(k, j); ++e) bump(std::make_tuple(T_CHAIN, k, j, s, e));
        if (j < kmax)
          for (int i = j; i < p; ++i) bump(std::make_tuple(0, i, j, 0, 0));
      } else {
        int i = it.l, k = it.k;
        if (i > k) bump(std::make_tuple(0, i - 1, k, 0, 0));
        if (k == 0) bump_up(0);
        if (k > 0)
          for (int s = 0; s < ns; ++s) bump(std::make_tuple(T_CHAIN, k - 1, k, s, seg_of(k - 1, k, i)));
      }
      tl[x].est = key;
    }
  }
  std::vector<T> sorted = tl;
  std::stable_sort(sorted.begin(), sorted.end(), [](const T& x, const T& y) {
    if (x.est != y.est) return x.est < y.est;
    return x.ord < y.ord;
  });
  fp.items.clear();
  for (auto& t : sorted) fp.items.push_back(t.it);
  fp.est_order = fp.missed == 0 && flow_list_topological(fp.items, p, q, ns);
  if (!fp.est_order) {  // step-major: always topological
    fp.items.clear();
    for (auto& t : tl) fp.items.push_back(t.it);
  }
  if (kn.depth > 0 && !xfer) window_order(fp.items, p, q, ns, ng, kn.depth);
}

// ---------------------------------------------------------------------------------------
// Deep-lookahead order (FlowKnobs::depth): list scheduling of the plan's own
// tasks, segments as they are, against a timing model of the engine on kWinW workgroups — the C++
// form of tools/sched_sim.py greedy_order(prio="window"), which it reproduces item for item.
// Each next list slot goes to the workgroup that frees first. A task is eligible once every task
// it waits on is in the list. Among the eligible tasks whose first useful work could start by
// then, the best class key wins:
//   panel (i, k)                    (0, k, i)
//   chain (k, j, s, e), j <= k + D  (1, j, k, e, s)   the columns left of the window first
//   every other chain               (2, k, j, e, s)   step-major bulk
// else the task that can start soonest. The estimator's order above ties the panel front to the
// bulk (with 256 workgroups it comes out step-major, only column k+1 favoured); here the panels
// and the chains that feed the next D panels overtake the bulk, so the late, latency-bound panels
// are done while the bulk still fills the machine. The times follow the engine's waits as
// sched_sim.py simulate() does (panel members per reflector group through Rr / Rc / Rt; chain
// elements per group behind the NEXT group's images, Tc of the tile's previous step, Ac of the
// previous segment's head rows). The planner has no device: the costs are constants, in us,
// measured at 16384^2 fp64, b = 256, ShapeW8 (profiles/r06/stamps/; tools/sched_sim.py P6).
// ---------------------------------------------------------------------------------------
namespace {
constexpr int kWinW = 256;         // workgroups: one per CU of an MI355X
// per panel reflector group (flowstamps_f64.txt, "per panel group"): panel_factor 28.45, build_t
// 10.29, trailing 15.88, panel I/O 12.03 in all — block in, R / V write-back, V/T images out
constexpr double kWinF = 28.5, kWinBt = 10.3, kWinT = 15.9;
constexpr double kWinIoIn = 4.0, kWinIoWb = 4.0, kWinIoImg = 4.0;
// per chain element (timeline_f64.txt): a reflector group of the asm chain body, the
// late strip load in the element's first group, the strip store in its hand-over group
constexpr double kWinC = 16.3, kWinELd = 5.0, kWinESt = 6.0;
constexpr double kWinDisp = 1.5;  // task dequeue (as tools/sched_sim.py P)

struct MinHeapD {
  std::vector<double> h;
  void push(double v) { h.push_back(v); std::push_heap(h.begin(), h.end(), std::greater<double>()); }
  double pop() { std::pop_heap(h.begin(), h.end(), std::greater<double>()); const double v = h.back(); h.pop_back(); return v; }
  double top() const { return h.front(); }
};
}  // namespace

void window_order(std::vector<Item>& L, int p, int q, int ns, int ng, int depth) {
  const int n = (int)L.size(), NG = std::max(1, ng);
  if (n == 0 || depth <= 0) return;
  int kmax = 0;
  for (const Item& it : L) {
    const int ty = it.ts & 0xff;
    if (ty != T_CHAIN && ty != QRS && ty != QRD) return;  // (transfer tasks: not modelled)
    kmax = std::max(kmax, (ty == T_CHAIN ? it.k & 0xffff : it.k) + 1);
  }
  struct Tk { int chain, i, k, j, s, e, i0, i1; };
  std::vector<Tk> tk(n);
  // panel (i, k) -> task; chain row (k, j, s, i) -> the task of the segment holding it
  std::vector<int> ptask((size_t)kmax * p, -1), rowtask((size_t)kmax * q * ns * p, -1);
  auto rt = [&](int k, int j, int s, int i) -> int& { return rowtask[(((size_t)k * q + j) * ns + s) * p + i]; };
  for (int x = 0; x < n; ++x) {
    const Item& it = L[x];
    if ((it.ts & 0xff) == T_CHAIN) {
      Tk t{1, 0, it.k & 0xffff, it.m, (it.ts >> 8) & 0xff, it.k >> 16, it.l & 0xffff, it.l >> 16};
      if (t.j < 0 || t.j >= q || t.s >= ns || t.i1 > p || t.i0 > t.i1 || t.i0 <= t.k || (t.e > 0 && t.i0 == t.i1)) return;
      for (int i = t.i0; i < t.i1; ++i) rt(t.k, t.j, t.s, i) = x;
      if (t.e == 0) rt(t.k, t.j, t.s, t.k) = x;  // (the UNMQR row)
      tk[x] = t;
    } else {
      if (it.l < 0 || it.l >= p || it.k < 0 || it.k >= kmax) return;
      ptask[(size_t)it.k * p + it.l] = x;
      tk[x] = Tk{0, it.l, it.k, it.k, 0, 0, 0, 0};
    }
  }
  // segment e - 1 of a chain task's segment e > 0: the one holding the row above its first
  std::vector<int> prevseg(n, -1);
  for (int x = 0; x < n; ++x) {
    const Tk& t = tk[x];
    if (!t.chain || t.e == 0) continue;
    const int pv = rt(t.k, t.j, t.s, t.i0 - 1);
    if (pv < 0 || tk[pv].e != t.e - 1) return;
    prevseg[x] = pv;
  }
  // wait targets of task x, without repeats; false: one is not in the list (keep the list)
  std::vector<int> dbuf;
  auto deps_of = [&](int x) {
    dbuf.clear();
    const Tk& t = tk[x];
    bool ok = true;
    auto add = [&](int d) { if (d < 0) ok = false; else dbuf.push_back(d); };
    if (!t.chain) {
      if (t.i > t.k) add(ptask[(size_t)t.k * p + t.i - 1]);
      if (t.k > 0)
        for (int s = 0; s < ns; ++s) add(rt(t.k - 1, t.k, s, t.i));
    } else {
      if (t.e == 0) {
        add(ptask[(size_t)t.k * p + t.k]);
        if (t.k > 0) add(rt(t.k - 1, t.j, t.s, t.k));
      } else {
        add(prevseg[x]);
      }
      for (int i = t.i0; i < t.i1; ++i) {
        add(ptask[(size_t)t.k * p + i]);
        if (t.k > 0) add(rt(t.k - 1, t.j, t.s, i));
      }
    }
    std::sort(dbuf.begin(), dbuf.end());
    dbuf.erase(std::unique(dbuf.begin(), dbuf.end()), dbuf.end());
    return ok;
  };
  std::vector<int> ndep(n), soff(n + 1, 0), succ;
  for (int x = 0; x < n; ++x) {
    if (!deps_of(x)) return;
    ndep[x] = (int)dbuf.size();
    for (int d : dbuf) ++soff[d + 1];
  }
  for (int x = 0; x < n; ++x) soff[x + 1] += soff[x];
  succ.resize(soff[n]);
  {
    std::vector<int> fill(soff.begin(), soff.end() - 1);
    for (int x = 0; x < n; ++x) {  // (in list order: a task's successors are released in that order)
      deps_of(x);
      for (int d : dbuf) succ[fill[d]++] = x;
    }
  }
  // model state: per panel and group Rr (R row published), Rc (images published), E (trailing
  // update done); Tc per tile strip (its element of the latest step done: the next step's task on
  // that tile is its only reader, and the one that overwrites it); per chain task the group ends of
  // its last element (the head rows the next segment waits for)
  std::vector<double> Rr((size_t)kmax * p * NG), Rc(Rr.size()), E(Rr.size()), Tc((size_t)p * q * ns, 0.0), G((size_t)n * NG, 0.0);
  auto pg = [&](int i, int k) { return ((size_t)k * p + i) * NG; };
  auto tc = [&](int i, int j, int s) -> double& { return Tc[((size_t)i * q + j) * ns + s]; };
  const int g1 = std::min(1, NG - 1);
  auto ready_time = [&](int x) {
    const Tk& t = tk[x];
    double r = 0.0;
    if (!t.chain) {
      if (t.k > 0)
        for (int s = 0; s < ns; ++s) r = std::max(r, tc(t.i, t.k, s));
      if (t.i > t.k) r = std::max(r, Rr[pg(t.i - 1, t.k)] - kWinIoIn - kWinF - kWinIoWb);
      return r;
    }
    const int i = t.e == 0 ? t.k : t.i0;
    r = std::max(Rc[pg(i, t.k)], Rc[pg(i, t.k) + g1]);
    if (t.k > 0) r = std::max(r, tc(i, t.j, t.s));
    if (t.e > 0) r = std::max(r, G[(size_t)prevseg[x] * NG + g1]);
    return r;
  };
  auto prio_key = [&](int x) -> unsigned long long {
    const Tk& t = tk[x];
    auto key = [](unsigned long long c, int a, int b, int e, int s) {
      return c << 56 | (unsigned long long)a << 40 | (unsigned long long)b << 24 | (unsigned long long)(e & 0xffff) << 8 | (unsigned)(s & 0xff);
    };
    if (!t.chain) return key(0, t.k, t.i, 0, 0);
    return t.j <= t.k + depth ? key(1, t.j, t.k, t.e, t.s) : key(2, t.k, t.j, t.e, t.s);
  };
  // place task x on a workgroup free at t0: the engine's timing rules (sched_sim.py simulate)
  auto place = [&](int x, double t0) {
    const Tk& t = tk[x];
    if (!t.chain) {
      double tt = t0;
      if (t.k > 0)
        for (int s = 0; s < ns; ++s) tt = std::max(tt, tc(t.i, t.k, s));
      const bool prev = t.i > t.k;
      const size_t me = pg(t.i, t.k), pv = prev ? pg(t.i - 1, t.k) : 0;
      for (int g = 0; g < NG; ++g) {
        double gs = g == 0 ? tt : E[me + g - 1];
        if (prev) gs = std::max(gs, Rr[pv + g]);
        Rr[me + g] = gs + kWinIoIn + kWinF + kWinIoWb;
        Rc[me + g] = Rr[me + g] + kWinBt + kWinIoImg;
        E[me + g] = (prev ? std::max(Rc[me + g], E[pv + g]) : Rc[me + g]) + kWinT;
      }
      return E[me + NG - 1];
    }
    double tt = t0;
    const double* hg = t.e > 0 ? &G[(size_t)prevseg[x] * NG] : nullptr;
    double* last = &G[(size_t)x * NG];
    const int nrows = (t.e == 0 ? 1 : 0) + (t.i1 - t.i0);
    auto row = [&](int idx) { return t.e == 0 ? (idx == 0 ? t.k : t.i0 + idx - 1) : t.i0 + idx; };
    for (int idx = 0; idx < nrows; ++idx) {
      const int i = row(idx);
      if (t.k > 0) tt = std::max(tt, tc(i, t.j, t.s));
      tt += kWinELd;
      const double* rc = &Rc[pg(i, t.k)];
      const double nxt = idx + 1 < nrows ? Rc[pg(row(idx + 1), t.k)] : 0.0;
      for (int g = 0; g < NG; ++g) {
        const double need = g + 1 < NG ? rc[g + 1] : nxt;
        double st = std::max({tt, rc[g], need});
        if (hg && idx == 0) st = std::max(st, hg[std::min(g + 1, NG - 1)]);
        tt = st + kWinC;
        last[g] = tt;
      }
      tt += kWinESt;
      tc(i, t.j, t.s) = tt;
    }
    return tt;
  };
  using NR = std::tuple<double, int, int>;             // (ready time, push count, task)
  using RD = std::pair<unsigned long long, int>;       // (class key, task): keys are unique
  std::priority_queue<NR, std::vector<NR>, std::greater<NR>> notready;
  std::priority_queue<RD, std::vector<RD>, std::greater<RD>> ready;
  MinHeapD workers;
  for (int w = 0; w < kWinW; ++w) workers.push(0.0);
  int cnt = 0;
  for (int x = 0; x < n; ++x)
    if (ndep[x] == 0) notready.emplace(ready_time(x), ++cnt, x);
  std::vector<Item> out;
  out.reserve(n);
  while (!notready.empty() || !ready.empty()) {
    const double tw = workers.top() + kWinDisp;
    while (!notready.empty() && std::get<0>(notready.top()) <= tw) {
      const int x = std::get<2>(notready.top());
      notready.pop();
      ready.emplace(prio_key(x), x);
    }
    int x;
    if (!ready.empty()) { x = ready.top().second; ready.pop(); }
    else { x = std::get<2>(notready.top()); notready.pop(); }
    out.push_back(L[x]);
    workers.push(place(x, workers.pop() + kWinDisp));
    for (int u = soff[x]; u < soff[x + 1]; ++u)
      if (--ndep[succ[u]] == 0) notready.emplace(ready_time(succ[u]), ++cnt, succ[u]);
  }
  // (a cycle or a lost task cannot pass: the list must hold every task once, in a topological order)
  if ((int)out.size() == n && flow_list_topological(out, p, q, ns)) L.swap(out);
}
// Multi-GPU: keep this rank's share of the global (topological) order — panel tasks of the tile
// columns it owns (column k on rank tile_owner(k, world); each forwards its images to the peers itself) and
// the chain tasks of its own tile columns. Every rank's list is the global order restricted, so
// the earliest unfinished task of the whole job can always progress: the multi-rank engine is
// deadlock-free like the single-GPU one.
// TQR_DIST_PART=cyclic: the round-2 partition j % world (A/B diagnostics; default snake)
int dist_cyclic() {
  const char* e = getenv("TQR_DIST_PART");
  return e && strcmp(e, "cyclic") == 0;
}
void partition_flow_plan(FlowPlan& fp, int rank, int world) {
  const int cyc = dist_cyclic();
  std::vector<Item> mine;
  for (const Item& it : fp.items) {
    const int ty = it.ts & 0xff;
    if (ty == T_CHAIN) {
      if (tile_owner(it.m, world, cyc) == rank) mine.push_back(it);
    } else if (tile_owner(it.k, world, cyc) == rank) {  // QRS(k,k) / QRD(l,k): tile column k
      mine.push_back(it);
    }
  }
  fp.items.swap(mine);
}

unsigned flow_list_hash(const std::vector<Item>& L) {
  unsigned h = 2166136261u;
  for (const Item& it : L)
    for (int v : {it.ts, it.l, it.m, it.k})
      for (int byte = 0; byte < 4; ++byte) h = (h ^ ((unsigned)v >> (8 * byte) & 0xffu)) * 16777619u;
  return h;
}

int flow_list(const tqr_flow_list_spec& sp, FlowPlan& fp, int steps) {
  if (steps > 0 && (steps > std::min(sp.M, sp.N) || sp.world != 1 || sp.nxc != 0)) return TQR_EINVAL;  // capped: one-GPU device lists
  if (sp.M <= 0 || sp.N <= 0 || !valid_b(sp.b) || (sp.dtype != TQR_F32 && sp.dtype != TQR_F64) || sp.world < 1 ||
      sp.rank >= sp.world || sp.nxc < 0 || sp.nxc > 255 || !(sp.tcol >= 0.0) || (sp.nxc > 0 && sp.world > 1))
    return TQR_EINVAL;
  const int sh = flow_shape(sp.dtype, sp.b);
  XferPlan xp;
  xp.nxc = sp.nxc;
  xp.tcol = sp.tcol;
  build_flow_plan(sp.M, sp.N, shape_ns(sh, sp.b), sp.b / shape_ib(sh, sp.b),
                  flow_knobs(sp.M, sp.N, sp.dtype, sp.world, sp.full != 0, sp.seglen, steps, sp.b), fp, sp.nxc > 0 ? &xp : nullptr, steps);
  if (sp.world > 1 && sp.rank >= 0) partition_flow_plan(fp, sp.rank, sp.world);
  return TQR_OK;
}

}  // namespace tqr

using namespace tqr;

// The older host-only entry points describe the fp64 list of whole-device ranks with the caller's
// segment length (>= 1); each is tqr_flow_list_export's list for that spec. M, N: tiles.
static tqr_flow_list_spec spec64(int M, int N, int b, int seglen, int world = 1, int rank = -1, int nxc = 0, double tcol = 0.0) {
  return tqr_flow_list_spec{M, N, b, TQR_F64, seglen, world, rank, 1, nxc, tcol};
}
static int list_check(const tqr_flow_list_spec& sp, int* ntasks, int* est_order) {
  FlowPlan fp;
  if (sp.seglen < 1 || flow_list(sp, fp) != TQR_OK) return TQR_EINVAL;
  if (ntasks) *ntasks = (int)fp.items.size();
  if (est_order) *est_order = fp.est_order;
  return TQR_OK;
}

extern "C" {

int tqr_flow_list_export_steps(const tqr_flow_list_spec* spec, int steps, int* items, int cap) {
  FlowPlan fp;
  if (!spec || flow_list(*spec, fp, std::max(0, steps)) != TQR_OK) return TQR_EINVAL;
  const int n = (int)fp.items.size();
  if (items)
    for (int x = 0; x < n && x < cap; ++x) {
      items[4 * x] = fp.items[x].ts; items[4 * x + 1] = fp.items[x].l;
      items[4 * x + 2] = fp.items[x].m; items[4 * x + 3] = fp.items[x].k;
    }
  return n;
}

int tqr_flow_list_export(const tqr_flow_list_spec* spec, int* items, int cap) {
  return tqr_flow_list_export_steps(spec, 0, items, cap);
}

int tqr_flow_plan_export(int M, int N, int b, int seglen, int* items, int cap) {
  if (seglen < 1) return TQR_EINVAL;
  const tqr_flow_list_spec sp = spec64(M, N, b, seglen);
  return tqr_flow_list_export(&sp, items, cap);
}

int tqr_flow_plan_check(int M, int N, int b, int seglen, int* ntasks, int* est_order) {
  return list_check(spec64(M, N, b, seglen), ntasks, est_order);
}

int tqr_flow_xfer_plan_check(int M, int N, int b, int seglen, int nxc, double tcol, int* ntasks, int* est_order) {
  if (nxc < 1) return TQR_EINVAL;
  return list_check(spec64(M, N, b, seglen, 1, -1, nxc, tcol), ntasks, est_order);
}

int tqr_dist_plan_check(int M, int N, int b, int seglen, int rank, int world, int* ntasks, int* nfwd) {
  if (rank < 0 || seglen < 1) return TQR_EINVAL;
  FlowPlan fp;
  if (flow_list(spec64(M, N, b, seglen, world, rank), fp) != TQR_OK) return TQR_EINVAL;
  if (ntasks) *ntasks = (int)fp.items.size();
  if (nfwd) {  // panel members that forward their images (the panel tasks, when world > 1)
    int c = 0;
    if (world > 1)
      for (auto& it : fp.items) c += (it.ts & 0xff) != T_CHAIN;
    *nfwd = c;
  }
  return TQR_OK;
}

int tqr_flow_strip_layout(int p, int q, int steps, int i, int j, int k) {
  if (p < 1 || q < 1 || steps < 0 || steps > std::min(p, q)) return TQR_EINVAL;
  const int kmax = flow_kmax(p, q, steps);
  if (k < 0 || k >= kmax || i < k || i >= p || j <= k || j >= q) return TQR_EINVAL;  // (a chain strip of step k)
  return strip_permuted(i, j, k, kmax) ? 1 : 0;
}

long tqr_flow_strip_offset(int layout, int pair, int lane, long ld) {
  if ((layout != 0 && layout != 1) || pair < 0 || pair >= 32 || lane < 0 || lane >= 64 || ld < 256 ||
      (size_t)ld * 8 * 16 >= ((size_t)1 << 31))
    return TQR_EINVAL;
  const size_t col = (size_t)ld * 8;
  return (long)(strip_lane_off(layout, lane, col) + ((pair & 1) ? strip_odd_off(layout, col) : 0u) + 64u * (unsigned)pair);
}

int tqr_flow_strip_width(void) { return shape_info(flow_shape(TQR_F64, 256)).sw; }

int tqr_flow_order_check(int M, int N, int b, const int* items, int n) {
  if (M <= 0 || N <= 0 || !valid_b(b) || !items || n <= 0) return TQR_EINVAL;
  std::vector<Item> L(n);
  for (int x = 0; x < n; ++x) L[x] = Item{items[4 * x], items[4 * x + 1], items[4 * x + 2], items[4 * x + 3]};
  return flow_list_topological(L, M, N, shape_ns(flow_shape(TQR_F64, b), b)) ? 1 : 0;
}

}  // extern "C"
