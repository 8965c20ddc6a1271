// Host planner of the persistent engine's task list (flowplan.cpp): which tasks a plan has, in
// which order every workgroup dequeues them, and the check that the order is topological for the
// engine's in-task waits — the deadlock-freedom condition (flow.hpp header). Pure host C++: built
// by g++ without HIP, so it can be compiled, run and sanitised without a device compiler.
#pragma once
#include <algorithm>
#include <vector>

#include "flow_list.hpp"
#include "tqr.h"

namespace tqr {

// Engine shape of the persistent kernel (flow_list.hpp FlowShape): 8 = ShapeW8 (one 8-wave workgroup per
// CU, 128-column strips, 32-reflector groups; the default), 4 = ShapeW4 (two 4-wave workgroups per
// CU, 64-column strips, 16-reflector groups; fp64 with TQR_FLOW_SHAPE=w4)
struct ShapeInfo {
  int nw, nt, sw, ib, wpc;
};
inline ShapeInfo shape_info(int shape) {
  return shape == 4   ? ShapeInfo{ShapeW4::NW, ShapeW4::NT, ShapeW4::SW, ShapeW4::IB, ShapeW4::WPC}
         : shape == 5 ? ShapeInfo{ShapeR::NW, ShapeR::NT, ShapeR::SW, ShapeR::IB, ShapeR::WPC}
                      : ShapeInfo{ShapeW8::NW, ShapeW8::NT, ShapeW8::SW, ShapeW8::IB, ShapeW8::WPC};
}
// fp64 default: ShapeW8 — ShapeW4 measured 138.6-139.0 vs 126.7-126.9 ms at 16384^2 (two alternating
// A/B rounds on one box, profiles/r04/shape_ab); TQR_FLOW_SHAPE=w4 selects it
// 5 = ShapeR (chain_res.hpp: one 4-wave workgroup per CU, one wave per SIMD with the whole register
// file, 64-column strips double-buffered in AGPRs, the head strip resident; fp64, b = 256;
// TQR_FLOW_SHAPE=r)
int flow_shape(int dtype, int b);
inline int shape_ib(int shape, int b) { return std::min(b, shape_info(shape).ib); }
inline int shape_ns(int shape, int b) { const int sw = shape_info(shape).sw; return (b + sw - 1) / sw; }

// ---------------------------------------------------------------------------------------
// Flow task list: panel tasks P(i,k) (i == k: GEQRT) and chain segments C(k,j,s,e), ordered
// by an as-soon-as-possible start-time estimate of the pipelined DAG (unit = one chain
// element), then checked to be topological (else the always-valid step-major order is used).
// ---------------------------------------------------------------------------------------
struct FlowPlan {
  std::vector<Item> items;
  bool est_order = false;
  int missed = 0;  // dependency lookups of the key bump that found no task (any: est_order = false)
};

// Host-pointer API: the persistent launch also carries the transfers (xfer.hpp). nxc chunks per
// tile column; tcol = one column's upload time in the estimator's unit (a chain element).
struct XferPlan {
  int nxc = 0;
  double tcol = 0.0;
};

// Order knobs of the flow task list, read from the environment ONCE per plan (flow_knobs) and
// kept with it: the host-API task list (hostpath.hip plan_xfer_list, built at the first host call) and
// the device's column-final counts (xfer.hpp, from FlowArgs) must see the same segment lengths as the
// plan's own list, whatever the environment says later.
//   seglen     chain segment length (TQR_SEGLEN, default 8; 2 on 4+ whole-device ranks)
//   seglen_la  the lookahead column's (j = k+1, the DAG's critical path: its chain elements feed
//              the next panel's members; TQR_SEGLEN_LA, default seglen)
//   la_tail    the last la_tail steps (TQR_LA_TAIL): their lookahead column runs one element per
//              segment, so the element that finishes the next diagonal tile runs beside the UNMQR
//              element instead of behind it
//   tail       the last `tail` steps (TQR_TAIL; default: flowplan.cpp default_tail): every chain
//              tail_sl elements per segment (TQR_TAIL_SEGLEN, default 1)
//   ualone     the last ualone steps (TQR_UNMQR_ALONE; default: tail): the lookahead column's UNMQR
//              element alone in segment 0 (flow_list.hpp unmqr_alone)
//   Tg         the estimator's panel group-step cost in chain elements (TQR_TG, default 1.4)
//   lazy       TQR_LAZY (default 1), la / lac: TQR_LA (default: flowplan.cpp default_la) / TQR_LAC
//              (see build_flow_plan)
//   depth      TQR_DEPTH: the deep-lookahead order's window in tile columns (flowplan.cpp window_order;
//              default: flowplan.cpp default_depth); 0: the estimator's list as it is. One-rank device
//              lists only (multi-rank plans and the host-pointer list keep theirs)
struct FlowKnobs {
  int seglen = 8, seglen_la = 8, la_tail = 0, tail = 0, tail_sl = 1, ualone = 0, depth = 0;
  double Tg = 1.4, lazy = 1.0, la = 0.0, lac = 0.0;
};
// The knobs of a plan of p x q tiles: the defaults of its dtype and of `world` ranks (full: each
// rank's launch covers its whole device — every rank must decide alike, tqr_dist_import checks the
// ranks' task-list signatures), then the environment's overrides. seglen <= 0: the default
// (TQR_SEGLEN, else by world and full); a positive value is used as it is.
// steps > 0: a capped plan (tqr_plan_create_steps) — the defaults that count steps back from the last
// one (tail, ualone, the multi-rank tail) count back from step steps - 1.
// b: the tile size (the deep-lookahead default holds for the shape its costs were measured on; 0: off)
FlowKnobs flow_knobs(int p, int q, int dtype, int world, bool full, int seglen, int steps = 0, int b = 0);
// Steps of a plan of p x q tiles: min(p, q), or the cap of a capped plan (1 <= steps <= min(p, q):
// only the leading `steps` tile columns get panels, every other column only their chains).
inline int flow_kmax(int p, int q, int steps) { return steps > 0 ? std::min(steps, std::min(p, q)) : std::min(p, q); }

// ns: chain strips per tile column, ng: reflector groups per tile (the engine shape's, shape_ns /
// b / shape_ib); steps: the cap (0: none), which must be the one the knobs were made for
void build_flow_plan(int p, int q, int ns, int ng, const FlowKnobs& kn, FlowPlan& fp, const XferPlan* xp = nullptr,
                     int steps = 0);
// Reorder a list of panel and chain tasks (no transfers) by list scheduling with a lookahead window
// of `depth` tile columns (flowplan.cpp). The list is replaced only by a topological permutation of
// itself; otherwise it stays as it is.
void window_order(std::vector<Item>& L, int p, int q, int ns, int ng, int depth);
// TQR_DIST_PART=cyclic: the round-2 partition j % world (A/B diagnostics; default snake)
int dist_cyclic();
void partition_flow_plan(FlowPlan& fp, int rank, int world);
bool flow_list_topological(const std::vector<Item>& L, int p, int q, int ns);
// FNV-1a of a list's items in order (a plan's signature: every knob that shapes the global list —
// segments, lookahead keys, TQR_LA / LAC / TG / LAZY — must agree across the ranks, tqr_dist_import)
unsigned flow_list_hash(const std::vector<Item>& L);
// The list of a spec (tqr.h tqr_flow_list_spec): what plan_create (nxc = 0) or plan_xfer_list
// builds for it, or with steps > 0 what tqr_plan_create_steps builds (world 1, nxc 0, steps <=
// min(M, N), else TQR_EINVAL). TQR_OK or TQR_EINVAL.
int flow_list(const tqr_flow_list_spec& sp, FlowPlan& fp, int steps = 0);

}  // namespace tqr
