// Task-list vocabulary of the persistent engine, shared by the host planner (flowplan.cpp, built
// without HIP) and the device code (flow.hpp): the task word, the task types beyond the reference's
// four, the engine shapes' constants, and the arithmetic of owners and chain segments that the
// planner and the kernels must agree on. Plain C++17: no HIP header, no device symbol.
#pragma once

#if defined(__HIPCC__)
#define TQR_HD __host__ __device__
#else
#define TQR_HD
#endif

namespace tqr {

// item = {type | strip << 8, l, m, k}  (reference Task fields, gridscheduler.h:13-17)
struct Item {
  int ts, l, m, k;
};

// the tile sizes the library is built for (every create and one-shot call checks its b with this)
inline bool valid_b(int b) { return b == 16 || b == 32 || b == 64 || b == 128 || b == 256; }

constexpr int T_CHAIN = 4;
constexpr int T_UP = 5, T_DOWN = 6;  // host <-> HBM transfer tasks (xfer.hpp)

// Engine shapes. ShapeW8 is the form of flow.hpp's header (one 8-wave workgroup per CU, 128-column
// chain strips, 32-reflector groups): the default. ShapeW4 (round 4, fp64 under TQR_FLOW_SHAPE=w4): TWO
// independent 4-wave workgroups per CU, 64-column chain strips, 16-reflector groups — half the LDS
// images (76 KiB per workgroup, so two fit in the CU's 160 KiB), the two workgroups running
// different tasks, so that one's strip hand-over, barrier skew and dependent-MFMA tails could run
// beside the other's MFMA stream. Measured: no gain — the chain loop alone is 3-4 % slower
// (tools/ubench/chain2_bench.hip: the hand-over's cost is not hidden by the co-resident workgroup,
// with or without the two out of phase) and the factorisation 9 % (138.6 vs 126.7 ms at 16384^2).
template <int NW_, int IB_, int WPC_>
struct FlowShape {
  static constexpr int NW = NW_, NT = 64 * NW_, SW = 16 * NW_, IB = IB_, WPC = WPC_;
};
using ShapeW8 = FlowShape<8, 32, 1>;
using ShapeW4 = FlowShape<4, 16, 2>;
using ShapeR = FlowShape<4, 32, 1>;  // one 4-wave workgroup per CU, 64-column strips, 32-reflector groups (chain_res.hpp)

// Multi-GPU (tile-column cyclic partition, one process per GPU): peer buffers opened by IPC.
struct PeerBufs {
  double* const* Wk;  // the peer's panel workspaces (IPC-opened into this process), one per k
  int* Rf;            // the peer's member flags
};

// Multi-GPU owner of tile column j (its panel and all its updates): "snake" order over the ranks
// (0..W-1, W-1..0, 0..W-1, ...), so that every rank's columns sum to the same index total — the
// chain work of a column grows with its index, and the plain cyclic j % W left the last rank 11 %
// more work at 65536x16384 on 8 ranks (tools/sched_sim.py dist: S(8) 5.39 vs 5.20).
// cyclic = 1 (TQR_DIST_PART=cyclic, A/B diagnostics only) restores j % W.
TQR_HD inline int tile_owner(int j, int world, int cyclic = 0) {
  const int blk = j / world, r = j - blk * world;
  if (cyclic) return r;
  return (blk & 1) ? world - 1 - r : r;
}

// Segment length of chain (k, j): the last `tail` steps' chains tail_sl elements per segment (their
// elements then pipeline group by group over workgroups instead of running one after the other in
// one: the factorisation's tail is a few short columns per step on the critical path); else the
// lookahead column (j = k+1) may use its own (seglen_la), and the last la_tail steps' lookahead
// column one element per segment (flowplan.hpp FlowKnobs).
TQR_HD inline int seglen_of_chain(int k, int j, int kmax, int seglen, int seglen_la, int la_tail,
                                  int tail = 0, int tail_sl = 1) {
  if (k >= kmax - tail) return tail_sl;
  if (j != k + 1) return seglen;
  return k >= kmax - la_tail ? 1 : seglen_la;
}
// The last `ualone` steps' lookahead column (j = k+1) runs its UNMQR element alone in segment 0:
// the element that finishes the next diagonal tile, TSMQR(k+1, k+1, k), then starts segment 1,
// pipelined group by group behind the UNMQR (Ac) instead of running after it in the same task.
TQR_HD inline bool unmqr_alone(int k, int j, int kmax, int ualone) { return j == k + 1 && k >= kmax - ualone; }
// segments of chain (k, j) with segment length sl: rows k+1 .. p-1 in runs of sl, after the
// UNMQR-only segment when unmqr_alone; the segment holding row i > k
TQR_HD inline int nseg_of_chain(int k, int j, int p, int kmax, int sl, int ualone) {
  const int rows = p - k - 1;
  if (rows <= 0) return 1;
  return (rows + sl - 1) / sl + (unmqr_alone(k, j, kmax, ualone) ? 1 : 0);
}
TQR_HD inline int seg_of_row(int k, int j, int i, int kmax, int sl, int ualone) {
  return (i - k - 1) / sl + (unmqr_alone(k, j, kmax, ualone) ? 1 : 0);
}

// Whole-line strips (plans with FlowArgs::chain_asm bit 4). The chain strip of tile
// (i, j) stored at step k is in the whole-line layout (below) iff its next reader is a TSMQR strip
// load, which reads with the map that wrote: the tile is neither step k+1's head row (i = k+1: its
// UNMQR strip and every head-row access) nor its panel column (j = k+1), and step k+1 exists (kmax =
// the plan's number of steps, a cap included). Everything else — UNMQR strips, head rows, the last
// step, hence all that the panel, the transfers and the caller see — is the standard layout. So a
// TSMQR strip load is whole-line at every step k >= 1 and standard at step 0.
TQR_HD inline bool strip_permuted(int i, int j, int k, int kmax) { return i > k + 1 && j > k + 1 && k + 1 < kmax; }
// The layouts of a wave's 16-column x 256-row fp64 strip block: the 16 B of lane (x, c) = (lane >> 4,
// lane & 15) in row pair p's access (tile rows 8 p + 2 x, + 1 of column c) lie at byte
//   strip_lane_off(layout, lane, col) + (p odd ? strip_odd_off(layout, col) : 0) + 64 p
// of the block, col = the bytes between two columns. Standard (0): column c, byte 64 p + 16 x — 16
// columns x 64 B per instruction, a column's four lanes 16 apart, which the CU's store path does not
// merge. Whole lines (1): column 2 x + (c >> 3), + 8 for odd p, line p >> 1, piece c & 7 — 8 columns x
// 128 B per instruction, each line from 8 consecutive lanes; a permutation of the block's 16-B pieces.
TQR_HD inline unsigned strip_lane_off(int layout, int lane, size_t col) {
  const unsigned x = (unsigned)lane >> 4, c = (unsigned)lane & 15;
  return layout ? (unsigned)((2 * x + (c >> 3)) * col + 16 * (c & 7)) : (unsigned)(c * col + 16 * x);
}
TQR_HD inline unsigned strip_odd_off(int layout, size_t col) { return layout ? (unsigned)(8 * col - 64) : 0u; }

}  // namespace tqr
