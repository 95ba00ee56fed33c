// kernels_zone_windows.h -- tj_zone_windows: WHEN is every robot's flown curve inside (or outside) a volume the caller names at query time, as certified time intervals.
//
// The siblings answer against what the scene or the state fixes: the obstacle set (kernels_obstacle_windows.h, kernels_sight_windows.h), the other robots
// (kernels_proximity.h), the robot's own dynamics (kernels_dynamics_windows.h).  A geofence, a no-fly box, an altitude band, a station's coverage ball are none of these:
// they never enter the BVH or the optimiser and change per question.  The fifth of the window queries: the raw position hull and its blossoming are dev_query.h's
// (hull_entry's sums, bez_restrict), the search loop and the placing of a slot's rows are dev_query.h's (WinSlotArgs, win_lane_search, win_slot_place: tj_dynamics_windows' word
// for word) and so is the merge half (WIN_*, win_sort, win_head, win_rows_before, win_row_index, WinChain with a leaf's faces in its id slots, WinRowFold, win_time).  This
// file's own: the evaluation (zonewin_eval), the zones with their staging in LDS, and the row.  The definition (include/trajadmm.h), per
// slot = (owned robot u, zone k):
//   net      b_0..b_5 = the raw hull of segment tr restricted to [sa, sb] (always from the RAW hull; [0, 1] returns it bit for bit)
//   PLANES   f_ij = dot3(n_j, b_i) - d_j over the zone's rows (n_j, d_j); lb = max_j min_i f_ij, ub = max_j max_i f_ij; g0 = max_j f_0j, g5 = max_j f_5j, each with its
//            face, the smallest j attaining it.  Every f_j is affine, so on the hull it lies between its extremes over the net, and a maximum of affine functions
//            between the maxima of both sides
//   BALL     e_i = b_i - c; ub = max_i norm3(e_i) - r; with d = e_0 + .. + e_5 per axis, left to right, lb = (min_i dot3(e_i, d) / norm3(d)) - r where norm3(d) > 0 and
//            the minimum is positive, else 0 - r (dynwin_eval's projection bound on e); g0 = norm3(e_0) - r, g5 = norm3(e_5) - r, face -1
//   class    INSIDE: OUT lb > level | IN ub <= level | MIXED; OUTSIDE: OUT ub < level | IN lb >= level | MIXED.  With sigma = +1 (INSIDE) / -1 (OUTSIDE) a leaf carries
//            sigma * g0 / sigma * g5 and WinChain::add takes sigma * level as the siblings' dist
//   search, merge   tj_dynamics_windows' (win_lane_search; the leaves by flight position tr + sa, adjacent iff prev.gb == next.ga, a row per maximal chain)
//
// TWO launches whatever the fleet, the zones and the depth (a count-only call, cap == 0, ends after the first):
//   k_zonewin_refine  grid (owned x n_zones), ONE wave per block.  The block's zone and its rows of the shape table are staged in LDS once; the block dispatches once on
//                     the zone's kind to a body templated on it (the branch is the block's).  Seeds and live windows are strided over the lanes, each lane halves its
//                     own window and evaluates both children in registers: the 18 net values stay in registers while the face loop, rolled, reads a row from LDS.
//   k_zonewin_place   one wave per slot (win_slot_place): win_rows_before over the slots before it gives its first row; blocks of 64 leaves through win_head / win_row_index; the lane
//                     of a head folds its chain left to right (WinChain) and writes the row at its final place.  Rows beyond the caller's capacity are counted only.
// The trip counts of the round loop, of the loop over live windows and of the face loop are read from LDS behind a barrier; every loop is bounded by max_depth <= 40,
// the list capacities and TJ_ZONEWIN_MAX_PLANES.  No float atomics, no polling, no workgroup waits on another, nothing of the iteration's scratch, no tj_stats counter,
// no launch count.  Read-only: the kernels write the query's own buffers only.
#pragma once
#include "dev_query.h"

namespace tj {

static_assert(sizeof(tj_zone) == 24 && sizeof(tj_zonewin_row) == 96, "the records' layout (include/trajadmm.h)");

constexpr int ZW_THREADS = WIN_LANES;   // one wave per slot

// a live window (MIXED) or a kept one (IN, or an EDGE leaf): [sa, sb] of segment tr; ga / gb = tr + sa / tr + sb, the position on the flight (the sort's and the chain's
// keys); g0 / g5 = sigma * the gauge attained at sa / sb, f0 / f5 its face there
// (-1 for a ball; bit-fields beside `in`: the leaf stays at the siblings' 56 bytes, and the search's frame with it)
struct ZoneLeaf { double sa, sb, ga, gb, g0, g5; int tr; int in : 8, f0 : 12, f5 : 12; };
static_assert(sizeof(ZoneLeaf) == 56 && TJ_ZONEWIN_MAX_PLANES < 2048, "a leaf's faces fit their bit-fields");

// dev_query.h's WinSlotArgs, the zones and their rows
struct ZonewinArgs : WinSlotArgs<ZoneLeaf> {
  const tj_zone* zones;     // [n_zones], checked on the host: first / count inside the table
  const double* shapes;     // [n_shapes][4]
  int n_zones;
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// ONE evaluation, in a lane's registers: the class of [sa, sb] of segment tr against the zone, and the window with its attained ends.  rows: the zone's rows in LDS
template <int KIND>
__device__ __forceinline__ int zonewin_eval(const Dev& D, const double* __restrict__ nu, int tr, double sa, double sb, const double* rows, int count, int sense, double level, ZoneLeaf& w) {
  double b[3][6];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double a[6];
#pragma unroll
    for (int i = 0; i < 6; i++) a[i] = hull_entry(D, nu, tr, i, k);
    bez_restrict(a, sa, sb, b[k]);
  }
  double lb, ub, g0, g5;
  int f0, f5;
  if constexpr (KIND == TJ_ZONE_PLANES) {
    lb = -INFINITY; ub = -INFINITY; g0 = -INFINITY; g5 = -INFINITY; f0 = 0; f5 = 0;
#pragma unroll 1
    for (int j = 0; j < count; j++) {   // (rolled: the net stays in registers, a face is four LDS words)
      const double nx = rows[4 * j], ny = rows[4 * j + 1], nz = rows[4 * j + 2], dj = rows[4 * j + 3];
      double mn = INFINITY, mx = -INFINITY, e0 = 0.0, e5 = 0.0;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const double f = dot3(nx, ny, nz, b[0][i], b[1][i], b[2][i]) - dj;
        mn = fmin(mn, f); mx = fmax(mx, f);
        if (i == 0) e0 = f;
        if (i == 5) e5 = f;
      }
      lb = fmax(lb, mn); ub = fmax(ub, mx);
      if (e0 > g0) { g0 = e0; f0 = j; }   // (the smallest j attaining the maximum)
      if (e5 > g5) { g5 = e5; f5 = j; }
    }
  } else {
    const double cx = rows[0], cy = rows[1], cz = rows[2], r = rows[3];
    double e[3][6];
#pragma unroll
    for (int i = 0; i < 6; i++) { e[0][i] = b[0][i] - cx; e[1][i] = b[1][i] - cy; e[2][i] = b[2][i] - cz; }
    double mx = -INFINITY, v0 = 0.0, v5 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const double v = norm3(e[0][i], e[1][i], e[2][i]);
      mx = fmax(mx, v);
      if (i == 0) v0 = v;
      if (i == 5) v5 = v;
    }
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      d[k] = e[k][0];
#pragma unroll
      for (int i = 1; i < 6; i++) d[k] = d[k] + e[k][i];
    }
    const double nd = norm3(d[0], d[1], d[2]);
    double m = INFINITY;
#pragma unroll
    for (int i = 0; i < 6; i++) m = fmin(m, dot3(e[0][i], e[1][i], e[2][i], d[0], d[1], d[2]));
    lb = (nd > 0.0 && m > 0.0 ? m / nd : 0.0) - r;
    ub = mx - r; g0 = v0 - r; g5 = v5 - r; f0 = -1; f5 = -1;
  }
  int cls;
  if (sense == TJ_ZONE_INSIDE) cls = lb > level ? WIN_OUT : (ub <= level ? WIN_IN : WIN_MIXED);
  else cls = ub < level ? WIN_OUT : (lb >= level ? WIN_IN : WIN_MIXED);
  const double sigma = sense == TJ_ZONE_INSIDE ? 1.0 : -1.0;
  w = ZoneLeaf{sa, sb, (double)tr + sa, (double)tr + sb, sigma * g0, sigma * g5, tr, cls == WIN_IN ? 1 : 0, f0, f5};
  return cls;
}

// the slot's search: dev_query.h's win_lane_search with zonewin_eval at the zone's kind as its evaluation
__global__ __launch_bounds__(ZW_THREADS) void k_zonewin_refine(Dev D, ZonewinArgs A) {
  const int ui = blockIdx.x / A.n_zones, k = blockIdx.x - ui * A.n_zones, u = D.u0 + ui, lane = lane_id();
  __shared__ int s_leaf, s_next, s_work;
  __shared__ int s_zone[4];                              // kind, sense, count
  __shared__ double s_level;
  __shared__ double s_rows[4 * TJ_ZONEWIN_MAX_PLANES];   // the block's zone: its rows of the shape table
  const tj_zone z = A.zones[k];
  const int count = z.count < TJ_ZONEWIN_MAX_PLANES ? z.count : TJ_ZONEWIN_MAX_PLANES;   // (the host has checked it: the clamp bounds the LDS index whatever it reads)
  for (int e = lane; e < 4 * count; e += ZW_THREADS) s_rows[e] = A.shapes[(size_t)4 * z.first + e];
  if (lane == 0) { s_zone[0] = z.kind; s_zone[1] = z.sense; s_zone[2] = count; s_level = z.level; }
  __syncthreads();
  const int kind = s_zone[0], sense = s_zone[1], n = s_zone[2];   // (LDS words behind a barrier: the branch and the face loop's trip count are the block's)
  const double level = s_level;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const auto search = [&](auto kd) {
    win_lane_search(D, A, blockIdx.x, u, s_leaf, s_next, s_work, [&](int tr, double sa, double sb, ZoneLeaf& w) { return zonewin_eval<decltype(kd)::value>(D, nu, tr, sa, sb, s_rows, n, sense, level, w); });
  };
  if (kind == TJ_ZONE_PLANES) search(std::integral_constant<int, TJ_ZONE_PLANES>{});
  else search(std::integral_constant<int, TJ_ZONE_BALL>{});
}

// the rows of a slot at their final place (win_slot_place): the slot's robot and zone, a leaf's faces as the chain's ids, and the row's own fields
__global__ __launch_bounds__(ZW_THREADS) void k_zonewin_place(Dev D, ZonewinArgs A, tj_zonewin_row* out) {
  const int slot = blockIdx.x, ui = slot / A.n_zones, k = slot - ui * A.n_zones, u = D.u0 + ui;
  const tj_zone z = A.zones[k];
  const double sigma = z.sense == TJ_ZONE_INSIDE ? 1.0 : -1.0;
  win_slot_place(D, A, slot, u, sigma * z.level, [](const ZoneLeaf& x, int& f0, int& f5) { f0 = x.f0; f5 = x.f5; },
                 [&](int r, const WinRowFold& f, const WinChain& ch, const ZoneLeaf& first, const ZoneLeaf& last, int leaves, int depth, int windows) {
                   tj_zonewin_row row;
                   f.put(row, sigma, ch);
                   row.robot = u; row.zone = k; row.sense = z.sense; row.face = ch.best_i;
                   row.segment_first = first.tr; row.segment_last = last.tr;
                   row.leaves = leaves; row.depth = depth; row.windows = windows;
                   out[r] = row;
                 });
}

}  // namespace tj
