// Host planner of the persistent engine's task list (flowplan.hpp): the order knobs and their
// defaults, the start-time estimator that orders the list, the multi-GPU partition, the
// topological check, and the host-only C entry points that describe a list without a GPU.
#include "flowplan.hpp"

#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>

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
bool flow_list_topological(const std::vector<Item>& L, int p, int q, int ns) {
  std::map<std::pair<int, int>, int> ppos;                       // (i, k) -> position
  std::map<std::tuple<int, int, int, int>, int> cpos;            // (k, j, s, e) -> position
  std::map<std::tuple<int, int, int, int>, int> rowpos;          // (k, j, s, row) -> position
  std::map<std::pair<int, int>, int> upos, dpos;                 // (j, c) -> position
  std::vector<int> uplast(q, -1);                                // last UP(j, *) of column j
  std::vector<int> collast(q, -1);                               // last task DOWN(j, *) waits for
  for (int x = 0; x < (int)L.size(); ++x) {
    const Item& it = L[x];
    const int ty = it.ts & 0xff;
    if (ty == T_CHAIN) {
      const int s = (it.ts >> 8) & 0xff, k = it.k & 0xffff, e = it.k >> 16, j = it.m, i0 = it.l & 0xffff, i1 = it.l >> 16;
      if (j < 0 || j >= q) return false;
      if (!cpos.emplace(std::make_tuple(k, j, s, e), x).second) return false;
      if (e == 0) rowpos[std::make_tuple(k, j, s, k)] = x;
      for (int i = i0; i < i1; ++i) rowpos[std::make_tuple(k, j, s, i)] = x;
      if (k < j) collast[j] = std::max(collast[j], x);
    } else if (ty == QRS || ty == QRD) {
      if (it.k < 0 || it.k >= q) return false;
      if (!ppos.emplace(std::make_pair(it.l, it.k), x).second) return false;
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
      if (e > 0 && !before(cpos, std::make_tuple(k, j, s, e - 1), x)) return false;
      if (e == 0 && !before(ppos, std::make_pair(k, k), x)) return false;
      if (e == 0 && k > 0 && !before(rowpos, std::make_tuple(k - 1, j, s, k), x)) return false;
      if (xfer && k == 0 && !(uplast[j] < x)) return false;
      for (int i = i0; i < i1; ++i) {
        if (!before(ppos, std::make_pair(i, k), x)) return false;
        if (k > 0 && !before(rowpos, std::make_tuple(k - 1, j, s, i), x)) return false;
      }
    } else if (ty == T_DOWN) {
      if (!(collast[it.m] < x)) return false;
    } else if (ty == QRS || ty == QRD) {
      const int i = it.l, k = it.k;
      if (i > k && !before(ppos, std::make_pair(i - 1, k), x)) return false;
      if (xfer && k == 0 && !(uplast[0] < x)) return false;
      if (k > 0)
        for (int s = 0; s < ns; ++s)
          if (!before(rowpos, std::make_tuple(k - 1, k, s, i), x)) return false;
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
FlowKnobs flow_knobs(int p, int q, int dtype, int world, bool full, int seglen, int steps) {
  const MultiRankDefaults mrd = multi_rank_defaults(p, flow_kmax(p, q, steps), dtype, world, full);
  return knobs_from_env(seglen > 0 ? seglen : env_seglen(world, full), mrd.tail, default_la(dtype), mrd.lac, mrd.ualone);
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
                  flow_knobs(sp.M, sp.N, sp.dtype, sp.world, sp.full != 0, sp.seglen, steps), fp, sp.nxc > 0 ? &xp : nullptr, steps);
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

int tqr_flow_strip_width(void) { return shape_info(flow_shape(TQR_F64, 256)).sw; }

int tqr_flow_order_check(int M, int N, int b, const int* items, int n) {
  if (M <= 0 || N <= 0 || !valid_b(b) || !items || n <= 0) return TQR_EINVAL;
  std::vector<Item> L(n);
  for (int x = 0; x < n; ++x) L[x] = Item{items[4 * x], items[4 * x + 1], items[4 * x + 2], items[4 * x + 3]};
  return flow_list_topological(L, M, N, shape_ns(flow_shape(TQR_F64, b), b)) ? 1 : 0;
}

}  // extern "C"
