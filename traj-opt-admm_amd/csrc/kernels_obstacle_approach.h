// kernels_obstacle_approach.h -- tj_obstacle_approach: how close the FLOWN CURVE of every robot comes to an obstacle primitive, when, and to which one.
//
// tj_audit's obs_clearance is the distance of a segment's 6-point HULL from the obstacles: what the solver constrains, a lower bound on what the vehicle does,
// without a time, and on the GJK's contact floor wherever a primitive lies inside a hull the curve itself stays clear of (an init file, tj_plan_init's
// output, a loaded state).  Here the hull bound drives tj_closest_approach's branch and bound (kernels_closest.h) over windows of ONE segment's parameter:
// an item is (segment tr, primitive i, window [sa, sb] in [0, 1]); its net is the RAW hull (hull_entry's sums) restricted to the window by bez_restrict
// (never the parent's net: rounding does not grow with depth; [0, 1] returns the raw hull bit for bit); lo(W) = |gjk(net's hull, primitive)| (hull = body 1, as
// k_audit) where the GJK's v SEPARATES the two (gjk_separates: v . (b_i - p_j) > 0 for all six points and all vertices), 0 otherwise; hi(W) = the smaller of
// b_0's and b_5's distance to the primitive, points of the curve at the window's ends: attained, at a known time.  Windows are dyadic: halving is exact, and
// with max_depth <= 40 none is ever unsplittable.  The definition (include/trajadmm.h), per owned robot u:
//   seeds    per segment the primitives k_audit's walk returns at m = range (the leaf predicate in fp64 on the primitives themselves), window [0, 1].
//            best = the smallest hi < range, equal values ordered by (hi, segment, index, s) (QBest, dev_query.h); live = {lo < range and lo < best.hi}
//   round d  every live item is halved at 0.5 * (sa + sb); both children are evaluated from the raw hull; best over (best, children of the round); then
//            live = the children with lo < best.hi -- against the round's FINAL best, so the set does not depend on the order of evaluation
//   bracket  lo_u = min(best.hi, min lo over live), hi_u = best.hi
//   stop     hi_u - lo_u <= tol | live empty | d == max_depth | more than max_windows live (TRUNCATED: the record of the last completed round)
//
// THREE launches whatever the fleet's size, the number of primitives and the depth:
//   k_obst_seed     one wave per (owned robot, segment): hull, BVH walk (bvh_query<1, PRIM> at m = range, the 49-axis cull is not used: DESIGN.md 3c), per
//                   candidate and lane hi and its end; a total-order reduction over the wave gives the row's best; the candidates are counted once per wave.
//   k_obst_append   the same walk again, now that every row of the robot is final: each wave reduces the robot's S rows to its best (S <= 504 records: less
//                   than one step of the walk), then per candidate and lane the certified lo; an item with lo < best.hi is appended to the robot's list with
//                   one integer atomic (append order is free: nothing downstream depends on it).  The row's smallest live lo goes to the row, so that the
//                   seed bracket is exact even where the list overflows.
//   k_obst_refine   one workgroup of OA_THREADS per owned robot runs ALL rounds (bnb_rounds, dev_query.h: the round loop of the branch-and-bound queries)
//                   over a ping-pong list in global memory (32-byte items + the children's lo).  A child (ObstSearch): the raw hull restricted in registers
//                   into the lane's column of one LDS tile, the per-lane GJK against the item's primitive.
// No float atomics, no workgroup waits on another, no polling, no cross-queue word, nothing of the iteration's scratch.  Read-only: the kernels write the
// query's own buffers only; the walk's overflow bit goes to the queries' control block, as k_audit's.  Hull and box, the restriction, the record QBest with its
// order, the bounded append and the round loop are dev_query.h's.
#pragma once
#include "kernels_closest.h"

namespace tj {

constexpr int OA_THREADS = 128;   // two waves: the per-lane GJK's registers, one 18-row tile of 128 columns

struct ObstItem { double sa, sb, lo; int tr, pt; };   // window [sa, sb] of segment tr against the SORTED primitive pt

struct ObstArgs {
  const double* net;     // [U][3][T]
  const double* pt;      // [U]
  const int* order;      // sorted primitive -> index in the caller's obstacle list
  double range, tol;
  int max_depth, max_windows, cap;
  QBest* row;            // [U][S] the best seed of the row (x: the position s in the segment, id: the caller's index of the primitive)
  double* row_lo;        // [U][S] the smallest lo among the row's live seeds (INFINITY: none)
  QBest* best;           // [U] the best seed of the robot
  ObstItem* list;        // [owned][2][cap] ping-pong live lists
  double* klo;           // [owned][2 * cap] lo of the round's children
  int* count;            // [U][2]: live seeds (may exceed max_windows: overflow), seeds evaluated
};

// distance of a point of the curve from a primitive: a cloud point directly; a triangle through the GJK of the one-point body (a point of the Minkowski
// difference: an upper bound on the true distance, attained to the triangle figure of DESIGN.md 3c)
template <int PRIM>
__device__ __forceinline__ double obst_point_dist(const V3& b, const typename PrimOf<PRIM>::Body& prim) {
  if constexpr (PRIM == 1) return norm3(b.x - prim.q.x, b.y - prim.q.y, b.z - prim.q.z);
  else { const V3 v = gjk(BodyPoint{b}, prim); return norm3(v.x, v.y, v.z); }
}

template <int PRIM>
__global__ __launch_bounds__(64) void k_obst_seed(Dev D, ObstArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18];
  __shared__ int walk[WalkScratch::INTS];
  QBox q;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, q);
  const double range = A.range;
  QBest mine{range, 0.0, INT_MAX, INT_MAX};
  int nev = 0;
  bvh_query<1, PRIM>(D, q, range, WalkScratch::carve(walk), nullptr, [&](int pt) {
    if (pt >= 0) {
      const auto prim = PrimOf<PRIM>::load(D, pt);
      const double h0 = obst_point_dist<PRIM>(V3{P[0], P[1], P[2]}, prim), h5 = obst_point_dist<PRIM>(V3{P[15], P[16], P[17]}, prim);
      const bool first = h0 <= h5;
      const QBest b{first ? h0 : h5, first ? 0.0 : 1.0, tr, A.order[pt]};
      nev++;
      if (b.hi < range && before(b, mine)) mine = b;
    }
  });
  wave_best(mine);
  nev = wave_sum(nev);
  if (lane == 0) {
    A.row[(size_t)u * S + tr] = mine;
    if (nev) atomicAdd(&A.count[2 * u + 1], nev);
  }
}

template <int PRIM>
__global__ __launch_bounds__(64) void k_obst_append(Dev D, ObstArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18];
  __shared__ int walk[WalkScratch::INTS];
  QBox q;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, q);
  const double range = A.range;
  QBest best{range, 0.0, INT_MAX, INT_MAX};
  for (int r = lane; r < S; r += 64) { const QBest b = A.row[(size_t)u * S + r]; if (before(b, best)) best = b; }
  wave_best(best);
  if (tr == 0 && lane == 0) A.best[u] = best;
  ObstItem* list = A.list + (size_t)ui * 2 * A.cap;
  double mlo = INFINITY;
  bvh_query<1, PRIM>(D, q, range, WalkScratch::carve(walk), nullptr, [&](int pt) {
    if (pt >= 0) {
      const auto prim = PrimOf<PRIM>::load(D, pt);
      const BodyHull hull{P};
      const V3 v = gjk(hull, prim);
      double lo = norm3(v.x, v.y, v.z);
      if (!gjk_separates(v, hull, prim)) lo = 0.0;
      if (lo < range && lo < best.hi) {
        mlo = fmin(mlo, lo);
        bnb_keep(A.count[2 * u], list, A.max_windows, ObstItem{0.0, 1.0, lo, tr, pt});
      }
    }
  });
  mlo = wave_min(mlo);
  if (lane == 0) A.row_lo[(size_t)u * S + tr] = mlo;
}

// The obstacle search of bnb_rounds (dev_query.h): a window of one segment's parameter is halved, a child is the raw hull restricted to it in the lane's column
// of the kernel's tile against the sorted primitive of the item.
template <int PRIM>
struct ObstSearch {
  using Item = ObstItem;
  using Best = QBest;
  static constexpr int ARITY = 2;
  static constexpr bool TERMINAL = false;   // dyadic windows, max_depth <= 40: none is ever unsplittable
  using Shared = BnbShared<QBest, OA_THREADS, false>;
  const Dev& D; const double* nu; const int* order; double range;
  double* cd;   // the lane's column of td
  __device__ __forceinline__ QBest none() const { return QBest{range, 0.0, INT_MAX, INT_MAX}; }
  __device__ __forceinline__ double eval(const ObstItem& w, int c, QBest& mine) const {
    const double sm = 0.5 * (w.sa + w.sb), sa = c ? sm : w.sa, sb = c ? w.sb : sm;
    hull_restrict<OA_THREADS>(D, nu, w.tr, sa, sb, cd);
    const auto prim = PrimOf<PRIM>::load(D, w.pt);
    const BodyHullS hull{cd, OA_THREADS};
    const V3 v = gjk(hull, prim);
    double lo = norm3(v.x, v.y, v.z);
    if (!gjk_separates(v, hull, prim)) lo = 0.0;
    const double h0 = obst_point_dist<PRIM>(hull.get(0), prim), h5 = obst_point_dist<PRIM>(hull.get(5), prim);
    const bool first = h0 <= h5;
    const QBest b{first ? h0 : h5, first ? sa : sb, w.tr, order[w.pt]};
    if (b.hi < range && before(b, mine)) mine = b;
    return lo;
  }
  __device__ __forceinline__ ObstItem child(const ObstItem& w, int c, double lo) const {
    const double sm = 0.5 * (w.sa + w.sb);
    return ObstItem{c ? sm : w.sa, c ? w.sb : sm, lo, w.tr, w.pt};
  }
};

template <int PRIM>
__global__ __launch_bounds__(OA_THREADS) void k_obst_refine(Dev D, ObstArgs A, tj_obstacle_robot* out) {
  const int tid = threadIdx.x, S = D.S, ui = blockIdx.x, u = D.u0 + ui;
  __shared__ double td[18 * OA_THREADS];
  __shared__ typename ObstSearch<PRIM>::Shared sh;
  const double res = (double)D.res, ptu = A.pt[u];
  ObstItem* cur = A.list + (size_t)ui * 2 * A.cap;
  sh.init();

  // the committed record: the seeds' bracket (every thread holds the same values)
  QBest best = A.best[u];
  double mlo = INFINITY;
  for (int r = tid; r < S; r += OA_THREADS) mlo = fmin(mlo, A.row_lo[(size_t)u * S + r]);
  sh.put_lo(mlo);
  __syncthreads();
  mlo = sh.lo(mlo);
  __syncthreads();
  double lo_u = fmin(best.hi, mlo);
  int n = A.count[2 * u], depth = 0;
  bool truncated = n > A.max_windows;
  bnb_rounds<OA_THREADS>(ObstSearch<PRIM>{D, A.net + (size_t)u * 3 * D.T, A.order, A.range, td + tid}, sh, A.tol, A.max_depth, A.max_windows,
                         cur, cur + A.cap, A.klo + (size_t)ui * 2 * A.cap, best, lo_u, n, depth, truncated);
  if (tid == 0) {
    tj_obstacle_robot r;
    const bool found = best.id != INT_MAX;
    r.lo = lo_u; r.hi = best.hi; r.time = found ? ((best.seg + best.x) / res) * ptu : -1.0;   // log_data's sigma * piece_time
    r.index = found ? best.id : -1; r.segment = found ? best.seg : -1;
    r.depth = depth; r.windows = A.count[2 * u + 1] + sh.ev; r.reserved = 0;   // the seeds evaluated and the rounds' children
    r.flags = bnb_flags(found, best.hi, lo_u, A.tol, n, truncated, D.offset) | (D.N == 0 ? TJ_OBSTACLE_CLEAR : 0);
    out[u] = r;
  }
}

}  // namespace tj
