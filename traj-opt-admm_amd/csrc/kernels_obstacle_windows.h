// kernels_obstacle_windows.h -- tj_obstacle_windows: WHEN is the flown curve of every robot within a distance `dist` of the obstacle set, as certified time intervals.
//
// tj_obstacle_approach looks for one minimum per robot and prunes (segment, primitive) items against a best.  This query classifies windows of a segment's parameter
// against the UNION of all primitives and keeps everything that is not certified outside: the obstacle-side counterpart of kernels_proximity.h.  Hull formation and
// the restriction of the RAW hull (hull_restrict), the BVH walk with its leaf predicate (bvh_query), the certified GJK bound (gjk, gjk_separates), the attained point
// distance (obst_point_dist) and the total-order reductions are the siblings', unchanged.  The definition (include/trajadmm.h), per (owned robot u, segment tr):
//   window   [sa, sb] dyadic in [0, 1]; its net = the raw hull restricted to it; C(W) = the primitives bvh_query<1, PRIM> returns at m = dist for the net's box
//   per p    lo_p (certified |v|, else 0), ub_p = the largest obst_point_dist(b_i, p), h0_p / h5_p = obst_point_dist of b_0 / b_5
//   class    OUT: every candidate has lo_p > dist (an empty C(W) too) | IN: some ub_p <= dist | MIXED: the rest (in this order)
//   h0, h5   the smallest h0_p (h5_p) over C(W) with its primitive, ordered by (value, caller's index)
//   search   seed [0, 1]; a round takes the live windows in ascending sa: time width <= tol -> EDGE leaf, else halved, children left then right: OUT dropped, IN to the
//            leaves, MIXED to the next live set.  Stop: live empty | max_depth | live or leaves above max_windows (TRUNCATED: the lists of the last completed round).
//            What is live at the end joins the leaves as EDGE leaves.
//   merge    per robot the leaves in (segment, sa) order; adjacent iff prev.tr + prev.sb == next.tr + next.sa on doubles; a row per maximal chain
//
// THREE launches whatever the fleet's size, the number of primitives and the depth (a count-only call, cap == 0, ends after the second):
//   k_obwin_refine  one 64-thread block per (owned robot, segment): the seed and ALL rounds in the kernel on the unit's slices of global lists.  One evaluation is
//                   wave-cooperative: lane 0 restricts the raw hull into the wave's 18 doubles of LDS, every lane takes the box, the walk hands 64 candidates at a
//                   time to process(pt), which forms the candidate's four values per lane and accumulates per lane any_in, all_out and the two (value, index)
//                   minima (the candidate buffer flushes at 64: process runs several times per walk); behind the walk one ballot each and two total-order
//                   reductions.  The windows of a round are taken one after the other by the whole wave, so the lists are appended by lane 0 alone, counted in
//                   LDS.  Then the leaves are sorted by sa (win_sort) into the live lists' room and the segment's leaf count, work, depth, truncation and interior
//                   chain heads are stored.
//   k_obwin_count   one wave per owned robot: the chain heads over its segments' leaves in order (a segment's first leaf continues the chain of the segment
//                   before it or starts one) = the robot's row count, and its work; the counts are added up with one integer atomic per robot.
//   k_obwin_place   one wave per owned robot: win_rows_before over the robots before it gives its first row; the chain heads of a block of 64 leaves get their row
//                   index from win_row_index, and the lane of a head folds its chain left to right (WinChain), across segment boundaries, and writes the row where
//                   it belongs.  Rows beyond the caller's capacity are counted, not written.
// THE MERGE HALF is dev_query.h's, shared with kernels_proximity.h: the classes and flag bits (WIN_*), the rank sort with the interior heads, the row indexing, the
// chain fold with the flag rule.  THE PROTOCOL around it is dev_query.h's too, shared with kernels_sight_windows.h: the rounds behind the seed, the EDGE leaves, the sort and
// the unit's record (win_wave_rounds), whether a segment's first leaf is a head (win_seg_first_is_head), the count (win_seg_count) and the placing with the chain walk across
// segment boundaries, closest_time = -1 and index = -1 without a sample (win_seg_place).  This file's own: the evaluation (obwin_eval), the seed, how a leaf's (segment, sa, sb)
// map to position, time and width (ObwinKeys), and the row's robot and segments.
// bvh_query and walk_step contain __syncthreads(): the refine kernel is ONE wave per block, every lane reaches every call, and the trip counts of the loop over
// live windows and of the round loop are read from LDS behind a barrier (or loaded from one address by every lane), never taken from a lane's own arithmetic.
// Every loop is bounded by max_depth <= 40 and max_windows.  No polling, no workgroup waits on another, no cross-queue word, no float atomics, no ticket between
// blocks (which is why counting is a launch of its own).  Read-only: the kernels write the query's own buffers only; the walk's overflow bit goes to the queries'
// control block (walk_dev's copy of Dev).  LDS per block: WalkScratch::INTS ints + 18 doubles + four counters; the per-lane GJK's registers set the occupancy.
#pragma once
#include "kernels_obstacle_approach.h"

namespace tj {

constexpr int OW_THREADS = 64;    // one wave per (robot, segment): the walk is one wave's

struct ObwinLeaf { double sa, sb, h0, h5; int i0, i5, in, pad; };   // a live window (MIXED) or a kept one (IN, or an EDGE leaf): [sa, sb], h0 / h5 with their primitives

struct ObwinArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  const int* order;    // sorted primitive -> index in the caller's obstacle list
  double range, tol;   // range: dist
  int max_depth, max_windows;
  int row_cap;         // the caller's rows
  ObwinLeaf* list;     // [owned][S][2][max_windows] ping-pong live lists; behind the rounds the segment's leaves by sa
  ObwinLeaf* leaf;     // [owned][S][2 * max_windows] the kept list, in the order of the appends
  int* info;           // [owned][S][4] leaves, work, depth (+ 1 << 16: truncated), chain heads behind the first leaf
  int* robot;          // [owned][2] rows, work
  int* n_rows;         // [1]
};

// how a leaf's keys (sa, sb of segment t) map to the flight: tr + s, the position, exact in a double (9 + 40 bits) -- two leaves are adjacent exactly when these agree --
// and its time ((tr + s) / res) * piece_time; a leaf's width in time is formed from its own keys
struct ObwinKeys {
  double res, ptu;
  __device__ __forceinline__ double pos(int t, double s) const { return (double)t + s; }
  __device__ __forceinline__ double time(int t, double s) const { return win_time(res, ptu, pos(t, s)); }
  __device__ __forceinline__ double width(int, double sa, double sb) const { return ((sb - sa) / res) * ptu; }
};

// ONE evaluation, by the whole wave: the class of [sa, sb] of segment tr, and (not OUT) the window with its h0, h5.  P: the wave's 18 doubles.
template <int PRIM>
__device__ __forceinline__ int obwin_eval(const Dev& D, const ObwinArgs& A, const double* net, int tr, double sa, double sb, double* P, const WalkScratch& ws, ObwinLeaf& w) {
  const int lane = lane_id();
  __syncthreads();   // nobody reads the net of the window before this one any more
  if (lane == 0) hull_restrict<1>(D, net, tr, sa, sb, P);
  __syncthreads();
  QBox q;
  hull_box(P, 1, q);
  const double dist = A.range;
  bool any_in = false, all_out = true;
  double b0 = INFINITY, b5 = INFINITY;
  int k0 = INT_MAX, k5 = INT_MAX;
  bvh_query<1, PRIM>(D, q, dist, ws, nullptr, [&](int pt) {
    if (pt >= 0) {
      const auto prim = PrimOf<PRIM>::load(D, pt);
      const BodyHull hull{P};
      const V3 v = gjk(hull, prim);
      const double lo = gjk_separates(v, hull, prim) ? norm3(v.x, v.y, v.z) : 0.0;
      all_out = all_out && lo > dist;
      double ub = 0.0, h0 = 0.0, h5 = 0.0;
      for (int i = 0; i < 6; i++) {
        const double d = obst_point_dist<PRIM>(hull.get(i), prim);
        ub = fmax(ub, d);
        if (i == 0) h0 = d;
        if (i == 5) h5 = d;
      }
      any_in = any_in || ub <= dist;
      const int id = A.order[pt];
      if (h0 < b0 || (h0 == b0 && id < k0)) { b0 = h0; k0 = id; }
      if (h5 < b5 || (h5 == b5 && id < k5)) { b5 = h5; k5 = id; }
    }
  });
  if (ballot(!all_out) == 0ull) return WIN_OUT;   // (wave-uniform; a lane without a candidate has nothing against OUT)
  const bool in = ballot(any_in) != 0ull;
  wave_argmin(b0, k0);
  wave_argmin(b5, k5);
  w = ObwinLeaf{sa, sb, b0, b5, k0, k5, in ? 1 : 0, 0};
  return in ? WIN_IN : WIN_MIXED;
}

template <int PRIM>
__global__ __launch_bounds__(OW_THREADS) void k_obwin_refine(Dev D, ObwinArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18];
  __shared__ int walk[WalkScratch::INTS];
  __shared__ int s_leaf, s_live, s_next, s_work;
  const WalkScratch ws = WalkScratch::carve(walk);
  const double* net = A.net + (size_t)u * 3 * D.T;
  const int maxw = A.max_windows;
  const double tol = A.tol, ptu = A.pt[u], res = (double)D.res;
  const size_t unit = (size_t)ui * S + tr;
  ObwinLeaf* cur = A.list + unit * 2 * maxw;
  ObwinLeaf* nxt = cur + maxw;
  ObwinLeaf* leaf = A.leaf + unit * 2 * maxw;

  // ---- the seed: the whole segment ----
  {
    ObwinLeaf w;
    const int cls = obwin_eval<PRIM>(D, A, net, tr, 0.0, 1.0, P, ws, w);
    if (lane == 0) {
      s_leaf = cls == WIN_IN ? 1 : 0; s_live = cls == WIN_MIXED ? 1 : 0; s_next = 0; s_work = 1;
      if (cls == WIN_IN) leaf[0] = w;
      if (cls == WIN_MIXED) cur[0] = w;
    }
  }
  __syncthreads();
  const int kept = s_leaf, n = s_live;   // (LDS words behind a barrier: the same in every lane)

  // ---- the rounds, the EDGE leaves, the sort by sa and the unit's record ----
  win_wave_rounds<&ObwinLeaf::sa, &ObwinLeaf::sb>(cur, nxt, leaf, kept, n, false, maxw, A.max_depth, s_leaf, s_next, s_work, A.info + unit * 4,
      [&](const ObwinLeaf& w) { return ((w.sb - w.sa) / res) * ptu <= tol; },
      [&](const ObwinLeaf&, double sa, double sb, ObwinLeaf& kid) { return obwin_eval<PRIM>(D, A, net, tr, sa, sb, P, ws, kid); });
}

__global__ __launch_bounds__(OW_THREADS) void k_obwin_count(Dev D, ObwinArgs A) {
  win_seg_count<&ObwinLeaf::sa, &ObwinLeaf::sb>(A.list, A.info, (size_t)2 * A.max_windows, D.S, blockIdx.x, A.robot, A.n_rows, ObwinKeys{});
}

// the rows of robot slot ui at their final place (win_seg_place); the row's own: robot and the chain's segments
__global__ __launch_bounds__(OW_THREADS) void k_obwin_place(Dev D, ObwinArgs A, tj_obswin_row* out) {
  const int ui = blockIdx.x, u = D.u0 + ui;
  win_seg_place<&ObwinLeaf::sa, &ObwinLeaf::sb>(A.list, A.info, (size_t)2 * A.max_windows, D.S, ui, A.robot, A.row_cap, A.range, A.tol, (double)D.S, ObwinKeys{(double)D.res, A.pt[u]}, out,
      [&](tj_obswin_row& row, int first, int last) { row.robot = u; row.segment_first = first; row.segment_last = last; });
}

}  // namespace tj
