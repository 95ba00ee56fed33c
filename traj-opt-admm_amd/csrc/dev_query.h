// dev_query.h -- what the read-only queries on the held state share (tj_audit, tj_audit_timed, tj_closest_approach, tj_obstacle_approach, tj_pair_approach, tj_path_crossings, tj_flight_profile), each piece defined once.
//
// Every query works per (owned robot, segment) on the segment's 6-point hull (hull_entry's sums: the bits of the hull cache) and its box, and reduces per-lane candidates
// with a TOTAL order, so that a result is a function of the state alone: no float atomics, no dependence on the order of evaluation.
//   query_hull     the unit's hull into LDS and its box
//   box_near       the box-gap skip: is a 6-point hull's box within `range` of the unit's box on every axis
//   wave_argmin    the smallest (value, key) in lexicographic order over the wave, with whatever travels along
//   QBest          the record of the two branch-and-bound queries, ordered by (hi, segment, id, parameter): before, wave_best
//   wave_min / wave_sum, bnb_keep   the small reductions and the bounded append of a branch-and-bound round (kernels_closest.h describes the round)
#pragma once
#include <limits.h>
#include "../../include/trajadmm.h"
#include "kernels_sep.h"

namespace tj {

// a 6-point hull behind a stride: the unit's own hull (LDS, stride 1) or a lane's column of a transposed tile (stride = the tile's width)
struct BodyHullS {
  const double* p; int st;
  static constexpr int N = 6;
  __device__ __forceinline__ V3 get(int i) const { return V3{p[(3 * i) * st], p[(3 * i + 1) * st], p[(3 * i + 2) * st]}; }
};

// the unit's hull (segment tr of the robot whose control net is `net`) into P[18] and its box; one wave, ends behind a barrier
__device__ __forceinline__ void query_hull(const Dev& D, const double* net, int tr, double* P, QBox& q) {
  const int lane = lane_id();
  if (lane < 18) P[lane] = hull_entry(D, net, tr, lane / 3, lane % 3);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double lo = INFINITY, hi = -INFINITY;
    for (int j = 0; j < 6; j++) { const double v = P[3 * j + k]; if (v < lo) lo = v; if (v > hi) hi = v; }
    q.lo[k] = lo; q.hi[k] = hi;
  }
}

// Boxes further apart than `range` on an axis: the hulls are at least that far apart, and so is whatever lies inside them.  (Rounding is monotonic, so a true gap <= range
// never compares greater; the guard keeps a pair whose gap is within rounding of `range` in the GJK, whose |v| decides.)  p, st: the other hull, as BodyHullS.
__device__ __forceinline__ bool box_near(const double* p, int st, const QBox& q, double range) {
  bool near = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < 6; i++) { const double v = p[(3 * i + k) * st]; if (v < lo) lo = v; if (v > hi) hi = v; }
    const double gap = fmax(lo - q.hi[k], q.lo[k] - hi);
    near = near && !(gap > range * 1.000001 + 1e-9);
  }
  return near;
}

template <class T>
__device__ __forceinline__ void take_if(bool take, T& mine, T other) { if (take) mine = other; }

// minimum of (d, key) in lexicographic order over the wave, every `aux` travels with it; every lane ends with the same tuple
template <class... Aux>
__device__ __forceinline__ void wave_argmin(double& d, int& key, Aux&... aux) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double d2 = __shfl_xor(d, off); const int k2 = __shfl_xor(key, off);
    const bool take = d2 < d || (d2 == d && k2 < key);
    (take_if(take, aux, __shfl_xor(aux, off)), ...);   // (the shuffle is an argument: every lane takes part in it)
    take_if(take, d, d2); take_if(take, key, k2);
  }
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the best attained distance of a branch and bound: hi at parameter x (a time, or a position in the segment) of segment seg against id (a partner robot, or the caller's index
// of a primitive).  Nothing found: {range, 0, INT_MAX, INT_MAX}.  The order is total: equal distances go to the smaller (segment, id, parameter).
struct QBest { double hi, x; int seg, id; };
__device__ __forceinline__ bool before(const QBest& a, const QBest& b) {
  if (a.hi != b.hi) return a.hi < b.hi;
  if (a.seg != b.seg) return a.seg < b.seg;
  if (a.id != b.id) return a.id < b.id;
  return a.x < b.x;
}
__device__ __forceinline__ void wave_best(QBest& m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const QBest o{__shfl_xor(m.hi, off), __shfl_xor(m.x, off), __shfl_xor(m.seg, off), __shfl_xor(m.id, off)};
    if (before(o, m)) m = o;
  }
}

// pass 2 of a round keeps an item: one integer atomic on the workgroup's LDS counter, stored while the list has room (the counter goes on: more than maxw = truncated)
template <class Item>
__device__ __forceinline__ void bnb_keep(int& kept, Item* nxt, int maxw, const Item& item) {
  const int at = atomicAdd(&kept, 1);
  if (at < maxw) nxt[at] = item;
}

}  // namespace tj
