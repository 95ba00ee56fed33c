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
// chain fold with the flag rule.  This file's own: a leaf's times and width are formed from (segment, sa, sb) (obwin_time; ((sb - sa) / res) * ptu), whether a segment's
// first leaf is a head and where a chain goes on behind a segment's last leaf (obwin_first_is_head), and the row's index, segments and closest_time = -1 without a sample.
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

// tr + s: the position on the flight, exact in a double (9 + 40 bits); two leaves are adjacent exactly when these agree
__device__ __forceinline__ double obwin_pos(int tr, double s) { return (double)tr + s; }
__device__ __forceinline__ double obwin_time(const Dev& D, double ptu, int tr, double s) { return (obwin_pos(tr, s) / (double)D.res) * ptu; }

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
  ObwinLeaf* const sorted = cur;

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
  int kept = s_leaf, n = s_live, depth = 0;   // (LDS words behind a barrier: the same in every lane)
  bool truncated = false;

  // ---- the rounds ----
  while (n > 0 && depth < A.max_depth) {
    __syncthreads();   // everyone has read the counters before lane 0 writes them
    if (lane == 0) s_next = 0;   // (s_leaf goes on from the committed count)
    for (int i = 0; i < n; i++) {
      const ObwinLeaf w = cur[i];   // (one address for the wave)
      if (((w.sb - w.sa) / res) * ptu <= tol) {
        if (lane == 0) { const int at = s_leaf++; if (at < maxw) { ObwinLeaf e = w; e.in = 0; leaf[at] = e; } }
        continue;
      }
      const double sm = 0.5 * (w.sa + w.sb);
      for (int c = 0; c < 2; c++) {
        ObwinLeaf k;
        const int cls = obwin_eval<PRIM>(D, A, net, tr, c ? sm : w.sa, c ? w.sb : sm, P, ws, k);
        if (lane == 0) {
          s_work++;
          if (cls == WIN_IN) { const int at = s_leaf++; if (at < maxw) leaf[at] = k; }
          if (cls == WIN_MIXED) { const int at = s_next++; if (at < maxw) nxt[at] = k; }
        }
      }
    }
    __syncthreads();   // the lists are written, the counters final
    const int k2 = s_leaf, n2 = s_next;
    if (k2 > maxw || n2 > maxw) { truncated = true; break; }   // the committed lists stand: the appends of this round do not count
    kept = k2; n = n2; depth++;
    ObwinLeaf* t = cur; cur = nxt; nxt = t;
  }

  // ---- the live windows of the last completed round become EDGE leaves ----
  __syncthreads();
  for (int i = lane; i < n; i += OW_THREADS) { ObwinLeaf e = cur[i]; e.in = 0; leaf[kept + i] = e; }
  const int m = kept + n;   // <= 2 * max_windows
  __syncthreads();

  // ---- by sa into the live lists' room, which is free now, and the chain heads behind the first leaf ----
  const int heads = win_sort<&ObwinLeaf::sa, &ObwinLeaf::sb>(leaf, sorted, m);
  if (lane == 0) {
    int* info = A.info + unit * 4;
    info[0] = m; info[1] = s_work; info[2] = depth | (truncated ? 1 << 16 : 0); info[3] = heads;
  }
}

// does the first leaf of segment tr of robot slot ui start a chain (it does not where the last leaf of segment tr - 1 ends where it begins)
__device__ __forceinline__ bool obwin_first_is_head(const ObwinArgs& A, int S, int ui, int tr) {
  if (tr == 0) return true;
  const size_t prev = (size_t)ui * S + tr - 1;
  const int mp = A.info[prev * 4];
  if (mp == 0) return true;
  const size_t w = (size_t)2 * A.max_windows;
  return obwin_pos(tr - 1, A.list[prev * w + mp - 1].sb) != obwin_pos(tr, A.list[(prev + 1) * w].sa);
}

__global__ __launch_bounds__(OW_THREADS) void k_obwin_count(Dev D, ObwinArgs A) {
  const int ui = blockIdx.x, lane = lane_id(), S = D.S;
  int rows = 0, work = 0;
  for (int tr = lane; tr < S; tr += OW_THREADS) {
    const int* info = A.info + ((size_t)ui * S + tr) * 4;
    work += info[1];
    if (info[0] > 0) rows += info[3] + (obwin_first_is_head(A, S, ui, tr) ? 1 : 0);
  }
  rows = wave_sum(rows); work = wave_sum(work);
  if (lane == 0) {
    A.robot[2 * ui] = rows; A.robot[2 * ui + 1] = work;
    if (rows) atomicAdd(A.n_rows, rows);
  }
}

// the rows of robot slot ui at their final place: behind the rows of the robots before it, chain after chain in time order
__global__ __launch_bounds__(OW_THREADS) void k_obwin_place(Dev D, ObwinArgs A, tj_obswin_row* out) {
  const int ui = blockIdx.x, lane = lane_id(), S = D.S, u = D.u0 + ui;
  int base = win_rows_before(A.robot, 2, ui);   // the robot's first row
  const int windows = A.robot[2 * ui + 1];
  const double dist = A.range, tol = A.tol, ptu = A.pt[u], res = (double)D.res;
  const size_t per = (size_t)2 * A.max_windows;
  for (int tr = 0; tr < S; tr++) {
    const size_t unit = (size_t)ui * S + tr;
    const int m = A.info[unit * 4];   // (one address for the wave)
    if (m == 0) continue;
    const ObwinLeaf* sorted = A.list + unit * per;
    const bool first_head = obwin_first_is_head(A, S, ui, tr);
    for (int i0 = 0; i0 < m; i0 += OW_THREADS) {
      const int i = i0 + lane;
      const bool head = win_head<&ObwinLeaf::sa, &ObwinLeaf::sb>(sorted, i, m, first_head);
      const int r = win_row_index(head, base);
      if (head && r < A.row_cap) {   // (no lane leaves the block loop early: every lane reaches the next ballot)
        // the chain from leaf i of segment tr on, left to right, into the segments behind where it goes on
        tj_obswin_row row;
        WinChain ch;
        double end_g = 0.0, end_t = 0.0;
        int t = tr, k = i, mt = m, leaves = 0, dmax = 0;
        bool trunc = false;
        const ObwinLeaf* sl = sorted;
        for (;;) {
          if (k == 0 || leaves == 0) { const int dt = A.info[((size_t)ui * S + t) * 4 + 2]; dmax = max(dmax, dt & 0xffff); trunc = trunc || (dt >> 16) != 0; }
          const ObwinLeaf x = sl[k];
          const double ta = obwin_time(D, ptu, t, x.sa), tb = obwin_time(D, ptu, t, x.sb);
          ch.add(dist, ta, tb, ((x.sb - x.sa) / res) * ptu, x.in, x.h0, x.h5, x.i0, x.i5);
          end_g = obwin_pos(t, x.sb); end_t = tb;
          leaves++;
          if (k + 1 < mt) {
            if (sl[k + 1].sa != x.sb) break;
            k++;
          } else {
            if (t + 1 >= S) break;
            const int m2 = A.info[((size_t)ui * S + t + 1) * 4];
            if (m2 == 0) break;
            const ObwinLeaf* s2 = A.list + ((size_t)ui * S + t + 1) * per;
            if (end_g != obwin_pos(t + 1, s2[0].sa)) break;
            t++; k = 0; mt = m2; sl = s2;
          }
        }
        const bool found = ch.best_i != INT_MAX;
        ch.finish(row, obwin_time(D, ptu, tr, sorted[i].sa), end_t, obwin_pos(tr, sorted[i].sa) == 0.0, end_g == (double)S, trunc, tol);
        row.closest_time = found ? ch.best_t : -1.0;
        row.robot = u; row.index = found ? ch.best_i : -1; row.segment_first = tr; row.segment_last = t;
        row.leaves = leaves; row.depth = dmax; row.windows = windows;
        out[r] = row;
      }
    }
  }
}

}  // namespace tj
