// kernels_sight_windows.h -- tj_sight_windows: WHEN does the straight line between two robots at equal flight times, or between a robot and a fixed station, pass
// within a distance `dist` of the obstacle set, as certified time intervals.
//
// The robot-robot queries look at two robots and no obstacle, the obstacle queries at one robot and the obstacles.  This one classifies windows of a LINK's time axis
// against the UNION of all primitives: time, hover, the cuts at the partner's segment boundaries and the restriction of both RAW hulls are kernels_audit_timed.h's
// (timed_cuts, timed_span, timed_partner_fill: the expressions of tj_proximity_windows), the BVH walk with its fp64 leaf predicate, the certified GJK bound and the
// attained point distance kernels_obstacle_windows.h's (bvh_query, gjk / gjk_separates, obst_point_dist), the merge half and the protocol around it dev_query.h's (win_wave_rounds,
// win_seg_count, win_seg_place: tj_obstacle_windows' rounds, count and placing, stated once).  This file's own: the evaluation (sight_eval, sight_candidate, sight_sample), the
// seeds with their truncation test, the keys (SightKeys: a leaf's keys are times already) and the row's link, robot and partner.  The definition
// (include/trajadmm.h), per link k = (a, b) and segment tr of a:
//   window   W = [ca, cb] in segment tr of a and in ONE segment j of b (j == S: b hovers; a station: six times its point, no cuts)
//   body     L(W) = a_0..a_5, b_0..b_5: both raw hulls restricted to W.  The link at any time of W joins a point of conv{a_i} to a point of conv{b_i}: it lies in conv L
//   C(W)     the primitives bvh_query<1, PRIM> returns at m = dist for the box of the 12 points
//   per p    lo_p (certified |gjk(L, p)|, else 0); sample(a_0, b_0, p) = h0_p at lambda0_p and sample(a_5, b_5, p) = h5_p at lambda5_p: attained distances of a
//            point of the link at ca / cb; ub_p = the largest obst_point_dist(a_i + lambda (b_i - a_i), p), the net of the point that rides the link at lambda,
//            looked at for lambda0_p where h0_p <= dist and for lambda5_p where h5_p <= dist (its i = 0 / i = 5 term is h0_p / h5_p itself)
//   class    OUT: every candidate has lo_p > dist (an empty C(W) too) | IN: some ub_p <= dist | MIXED: the rest (in this order)
//   search   the seeds in time order: IN to the leaves, MIXED live; a round takes the live windows in ascending ca: prox_is_leaf -> EDGE leaf, else halved, children
//            left then right: OUT dropped, IN to the leaves, MIXED to the next live set.  Stop: live empty | max_depth | live or leaves above max_windows (TRUNCATED:
//            the lists of the last completed round; among the seeds alone: depth 0).  What is live at the end joins the leaves as EDGE leaves.
//   merge    per link the leaves of its segments by ca; adjacent iff prev.cb == next.ca on doubles; a row per maximal chain
//
// THREE launches whatever the number of links, the number of primitives and the depth (a count-only call, cap == 0, ends after the second):
//   k_sight_refine  one 64-thread block per (link, segment of a): lane 0 lists the seeds (timed_cuts), then the seeds and ALL rounds in the kernel on the unit's slices
//                   of global lists.  One evaluation is wave-cooperative: lane 0 restricts both raw hulls into the wave's 36 doubles of LDS, every lane takes the
//                   box, the walk hands 64 candidates at a time to process(pt), which runs per lane the GJK of the 12-point body, the two samples and the ub nets
//                   its samples ask for, and accumulates any_in, all_out and the two (value, index) minima; behind the walk one ballot each and two total-order
//                   reductions.  Lane 0 alone appends, counted in LDS.  Then the leaves are sorted by ca (win_sort) into the live lists' room.
//   k_sight_count   one wave per link: the chain heads over its segments' leaves = its row count, and its work; one integer atomic per link.
//   k_sight_place   one wave per link: win_rows_before gives its first row, win_row_index a head's row, the head's lane folds its chain (WinChain) across segments.
// k_obwin_refine's barrier rules hold: ONE wave per block, every lane reaches every call of bvh_query, the trip counts of the loops over seeds, live windows and rounds
// are read from LDS behind a barrier.  A link whose robot a is not owned ends before the first barrier with an empty record (a group asks every rank for the whole
// list).  No polling, no workgroup waits on another, no float atomics.  Read-only: the kernels write the query's own buffers only; the walk's overflow bit goes to the
// queries' control block.  LDS per block: WalkScratch::INTS ints + 36 doubles + four counters.
#pragma once
#include "kernels_obstacle_windows.h"
#include "kernels_proximity.h"

namespace tj {

constexpr int SW_THREADS = 64;    // one wave per (link, segment): the walk is one wave's

struct SightLeaf { double ca, cb, h0, h5; int i0, i5, in, j; };   // a seed (ca, cb, j), a live window (MIXED) or a kept one (IN, or an EDGE leaf): h0 / h5 with their primitives

struct SightArgs {
  const double* net;       // [U][3][T]
  const double* pt;        // [U]
  const int* order;        // sorted primitive -> index in the caller's obstacle list
  const int* links;        // [n_links][2] (a, b); b < 0: station -1 - b
  const double* stations;  // [n_stations][3]
  double range, tol;       // range: dist
  int max_depth, max_windows;
  int leaf_cap;            // leaves per unit: 2 * max_windows + S + 1 (the seeds alone may be all there is)
  int row_cap;             // the caller's rows
  SightLeaf* list;         // [n_links][S][leaf_cap] the seeds, then the ping-pong live lists (2 * max_windows); behind the rounds the segment's leaves by ca
  SightLeaf* leaf;         // [n_links][S][leaf_cap] the kept list, in the order of the appends
  int* info;               // [n_links][S][4] leaves, work, depth (+ 1 << 16: truncated), chain heads behind the first leaf
  int* link;               // [n_links][2] rows, work
  int* n_rows;             // [1]
};

// the link between x and y at one instant: the point at lambda, and the clamped parameter of the foot of z
struct SightLink {
  V3 x, e; double ee;
  __device__ __forceinline__ SightLink(const V3& x_, const V3& y) : x(x_), e{y.x - x_.x, y.y - x_.y, y.z - x_.z} { ee = e.x * e.x + e.y * e.y + e.z * e.z; }
  __device__ __forceinline__ V3 at(double l) const { return V3{x.x + l * e.x, x.y + l * e.y, x.z + l * e.z}; }
  __device__ __forceinline__ double proj(const V3& z) const { return ee == 0.0 ? 0.0 : clamp01(((z.x - x.x) * e.x + (z.y - x.y) * e.y + (z.z - x.z) * e.z) / ee); }
};

// sample(x, y, p): the attained distance of the link's point at lambda from p; exact for a cloud point, TJ_SIGHT_PROJECTIONS alternating projections for a triangle
// (the GJK of a one-point body gives the triangle's witness z - v for free).  ONE GJK call site: the last pass takes the value.
template <int PRIM>
__device__ __forceinline__ double sight_sample(const SightLink& ln, const typename PrimOf<PRIM>::Body& prim, double& lambda) {
  if constexpr (PRIM == 1) {
    lambda = ln.proj(prim.q);
    return obst_point_dist<PRIM>(ln.at(lambda), prim);
  } else {
    double l = 0.5, h = 0.0;
#pragma unroll 1
    for (int k = 0; k <= TJ_SIGHT_PROJECTIONS; k++) {
      const V3 z = ln.at(l);
      const V3 v = gjk(BodyPoint{z}, prim);
      if (k < TJ_SIGHT_PROJECTIONS) l = ln.proj(V3{z.x - v.x, z.y - v.y, z.z - v.z});
      else h = norm3(v.x, v.y, v.z);
    }
    lambda = l;
    return h;
  }
}

// one candidate, per lane: L = the 12 points (a_i at L[3 i], b_i at L[18 + 3 i])
template <int PRIM>
__device__ __forceinline__ void sight_candidate(const double* L, const typename PrimOf<PRIM>::Body& prim, double dist, double& lo, double& h0, double& h5, bool& in) {
  const BodyHull12 body{L};
  const V3 v = gjk(body, prim);
  lo = gjk_separates(v, body, prim) ? norm3(v.x, v.y, v.z) : 0.0;
  double l0 = 0.0, l5 = 0.0;
#pragma unroll 1
  for (int e = 0; e < 2; e++) {
    const int i = 5 * e;
    double l;
    const double h = sight_sample<PRIM>(SightLink(body.get(i), body.get(6 + i)), prim, l);
    if (e == 0) { h0 = h; l0 = l; } else { h5 = h; l5 = l; }
  }
  in = false;
#pragma unroll 1
  for (int e = 0; e < 2; e++) {
    const double l = e ? l5 : l0;
    if (in || !((e ? h5 : h0) <= dist)) continue;
    double ub = 0.0;
#pragma unroll 1
    for (int i = 0; i < 6; i++) ub = fmax(ub, obst_point_dist<PRIM>(SightLink(body.get(i), body.get(6 + i)).at(l), prim));
    in = ub <= dist;
  }
}

// what one evaluation reads of the link's two ends
struct SightEnds { const double* na; const double* nb; const double* station; double pta, ptb; };   // nb == nullptr: the station

// ONE evaluation, by the whole wave: the class of [ca, cb] in segment tr of a and segment j of b, and (not OUT) the window with its h0, h5.  L: the wave's 36 doubles.
template <int PRIM>
__device__ __forceinline__ int sight_eval(const Dev& D, const SightArgs& A, const SightEnds& E, int tr, int j, double ca, double cb, double* L, const WalkScratch& ws, SightLeaf& w) {
  const int lane = lane_id();
  __syncthreads();   // nobody reads the body of the window before this one any more
  if (lane == 0) {
    const TimedSpan sp = timed_span((double)D.res, E.pta, E.ptb, tr, j, ca, cb);
    hull_restrict<1>(D, E.na, tr, sp.sa, sp.sb, L);
    if (!E.nb) {
      for (int i = 0; i < 6; i++) for (int k = 0; k < 3; k++) L[18 + 3 * i + k] = E.station[k];
    } else if (j >= D.S) {
      timed_partner_fill<1>(D, E.nb, j, true, L + 18);
    } else {
      hull_restrict<1>(D, E.nb, j, sp.ra, sp.rb, L + 18);
    }
  }
  __syncthreads();
  QBox q, qb;
  hull_box(L, 1, q);
  hull_box(L + 18, 1, qb);
#pragma unroll
  for (int k = 0; k < 3; k++) { q.lo[k] = fmin(q.lo[k], qb.lo[k]); q.hi[k] = fmax(q.hi[k], qb.hi[k]); }
  const double dist = A.range;
  bool any_in = false, all_out = true;
  double b0 = INFINITY, b5 = INFINITY;
  int k0 = INT_MAX, k5 = INT_MAX;
  bvh_query<1, PRIM>(D, q, dist, ws, nullptr, [&](int pt) {
    if (pt >= 0) {
      const auto prim = PrimOf<PRIM>::load(D, pt);
      double lo, h0, h5; bool in;
      sight_candidate<PRIM>(L, prim, dist, lo, h0, h5, in);
      all_out = all_out && lo > dist;
      any_in = any_in || in;
      const int id = A.order[pt];
      if (h0 < b0 || (h0 == b0 && id < k0)) { b0 = h0; k0 = id; }
      if (h5 < b5 || (h5 == b5 && id < k5)) { b5 = h5; k5 = id; }
    }
  });
  if (ballot(!all_out) == 0ull) return WIN_OUT;   // (wave-uniform; a lane without a candidate has nothing against OUT)
  const bool in = ballot(any_in) != 0ull;
  wave_argmin(b0, k0);
  wave_argmin(b5, k5);
  w = SightLeaf{ca, cb, b0, b5, k0, k5, in ? 1 : 0, j};
  return in ? WIN_IN : WIN_MIXED;
}

template <int PRIM>
__global__ __launch_bounds__(SW_THREADS) void k_sight_refine(Dev D, SightArgs A) {
  const int lane = lane_id(), S = D.S;
  const int k = blockIdx.x / S, tr = blockIdx.x - k * S;
  const int a = A.links[2 * k], b = A.links[2 * k + 1];
  const size_t unit = (size_t)k * S + tr;
  if (a < D.u0 || a >= D.u1) {   // another rank's link: an empty record (the whole block leaves, before any barrier)
    if (lane < 4) A.info[unit * 4 + lane] = 0;
    return;
  }
  __shared__ double L[36];
  __shared__ int walk[WalkScratch::INTS];
  __shared__ int s_leaf, s_live, s_next, s_work;
  const WalkScratch ws = WalkScratch::carve(walk);
  const int maxw = A.max_windows;
  const double tol = A.tol, res = (double)D.res;
  const SightEnds E{A.net + (size_t)a * 3 * D.T, b >= 0 ? A.net + (size_t)b * 3 * D.T : nullptr, b >= 0 ? nullptr : A.stations + (size_t)(-1 - b) * 3, A.pt[a], b >= 0 ? A.pt[b] : A.pt[a]};
  SightLeaf* cur = A.list + unit * A.leaf_cap;
  SightLeaf* nxt = cur + maxw;
  SightLeaf* leaf = A.leaf + unit * A.leaf_cap;

  // ---- the seeds: segment tr's window of time cut at b's segment boundaries and arrival (a station: no cuts), listed by lane 0 at the head of the live list ----
  if (lane == 0) {
    const double t0 = (tr / res) * E.pta, t1 = ((tr + 1) / res) * E.pta;   // (timed_walk's window at level 0, bit for bit)
    int ns = 0;
    if (b < 0) cur[ns++] = SightLeaf{t0, t1, 0.0, 0.0, 0, 0, 0, S};
    else timed_cuts(t0, t1, E.ptb, res, S, [&](int j, bool, double ca, double cb) { cur[ns++] = SightLeaf{ca, cb, 0.0, 0.0, 0, 0, 0, j}; });
    s_leaf = 0; s_live = 0; s_next = ns; s_work = ns;
  }
  __syncthreads();
  const int ns = s_next;   // (an LDS word behind a barrier: the same in every lane; at most S + 1)
  for (int i = 0; i < ns; i++) {
    const SightLeaf s = cur[i];   // (one address for the wave; lane 0 stores at or below i only behind the evaluation's barriers)
    SightLeaf w;
    const int cls = sight_eval<PRIM>(D, A, E, tr, s.j, s.ca, s.cb, L, ws, w);
    if (lane == 0) {
      if (cls == WIN_IN) leaf[s_leaf++] = w;
      if (cls == WIN_MIXED) cur[s_live++] = w;
    }
  }
  __syncthreads();
  const int kept = s_leaf, n = s_live;   // (LDS words behind a barrier: the same in every lane)
  const bool truncated = n > maxw || kept > maxw;   // the seeds alone: no round, every seed that is not OUT is a leaf (at most S + 1: leaf_cap has room)

  // ---- the rounds, the EDGE leaves, the sort by ca and the unit's record ----
  win_wave_rounds<&SightLeaf::ca, &SightLeaf::cb>(cur, nxt, leaf, kept, n, truncated, maxw, A.max_depth, s_leaf, s_next, s_work, A.info + unit * 4,
      [&](const SightLeaf& w) { return prox_is_leaf(w.ca, w.cb, tol); },
      [&](const SightLeaf& w, double ca, double cb, SightLeaf& kid) { return sight_eval<PRIM>(D, A, E, tr, w.j, ca, cb, L, ws, kid); });
}

// a leaf's keys are times already: the position compared across a segment boundary, the time and the width follow from them alone
struct SightKeys {
  __device__ __forceinline__ double pos(int, double c) const { return c; }
  __device__ __forceinline__ double time(int, double c) const { return c; }
  __device__ __forceinline__ double width(int, double ca, double cb) const { return cb - ca; }
};

__global__ __launch_bounds__(SW_THREADS) void k_sight_count(Dev D, SightArgs A) {
  win_seg_count<&SightLeaf::ca, &SightLeaf::cb>(A.list, A.info, (size_t)A.leaf_cap, D.S, blockIdx.x, A.link, A.n_rows, SightKeys{});
}

// the rows of link k at their final place (win_seg_place); the row's own: the link and its two ends
__global__ __launch_bounds__(SW_THREADS) void k_sight_place(Dev D, SightArgs A, tj_sight_row* out) {
  const int k = blockIdx.x, S = D.S, a = A.links[2 * k], b = A.links[2 * k + 1];
  if (a < D.u0 || a >= D.u1) return;   // (another rank's link: no leaves; the whole block leaves)
  const double t_end = ((S - 1 + 1) / (double)D.res) * A.pt[a];   // the end of a's last segment, in the seeds' expression
  win_seg_place<&SightLeaf::ca, &SightLeaf::cb>(A.list, A.info, (size_t)A.leaf_cap, S, k, A.link, A.row_cap, A.range, A.tol, t_end, SightKeys{}, out,
      [&](tj_sight_row& row, int, int) { row.link = k; row.robot = a; row.partner = b; });
}

}  // namespace tj
