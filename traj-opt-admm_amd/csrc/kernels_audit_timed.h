// kernels_audit_timed.h -- tj_audit_timed: how close do two robots get at EQUAL FLIGHT TIMES, with a certificate.
//
// tj_audit's pair_clearance is the solver's own pairing (equal segment indices: separate_self / self_step, Optimization3D_multi.h:246-259, Step.h:196-208).
// Decoupled robots carry their own piece_time, so equal indices are not equal times.  Here both robots are looked at in real time, with log_data's conventions
// (Main/multiPathPlanning3D.cpp:31-60): t = sigma * piece_time, sigma in [0, P] the piece parameter, time_weight == 1; segment tr of robot u is sigma in
// [tr / res, (tr + 1) / res] and its hull (hull_entry's sums) is the Bezier net of the flown quintic there; after P * piece_time_q robot q has arrived and
// stays at its last control point (a one-point body).
//
// For an owned robot u, its segment tr, a partner q != u and the level L (0..6):
//   the segment's window of time [T0, T1] = [tr / res, (tr + 1) / res] * piece_time_u is split into 2^L equal sub-windows; each is cut at q's segment boundaries
//   (j / res) * piece_time_q and at q's arrival, so that a window W = [ca, cb] lies in ONE segment of u and ONE segment of q (or in q's hover);
//   both quintics are restricted to W by blossoming (bez_restrict: b_i = the blossom with 5 - i arguments at W's start and i at its end, de Casteljau steps
//   (1 - s) * x + s * y); d_i = a_i - b_i is the Bezier net of p_u(t) - p_q(t) over W;
//   lo(W) = |gjk(conv{d_0..d_5}, {0})|: the curve lies in its hull, so no separation on W is smaller (up to GJK's stopping rule);
//   hi(W) = min(|d_0|, |d_5|): the end points lie on the curve, a separation attained at W's start / end.
// Per (robot, segment) the minima of lo and hi over partners and windows, capped at `range`; ties keep the smallest (partner, sub-window, cut).
//
// Exactness of the skip: a window is not evaluated when the boxes of the two RAW segment hulls are further apart than `range` on an axis -- both restricted
// nets lie in their raw hulls, so |d| >= hull distance >= box gap > range on the whole window, and neither minimum (both capped at `range`) can change
// (box_near, dev_query.h).
//
//   k_audit_timed         one wave per (owned robot, segment).  Lane = (partner of the pass, sub-window): 64 >> L partners per pass, 2^L sub-windows each, so level 6
//                         is one partner per pass and one sub-window per lane.  A lane walks the cuts of its sub-window (usually one or two), forms q's raw hull in its
//                         column of an LDS tile (stride 64 doubles: lane-consecutive, conflict-free), restricts both nets in registers, writes d to its column of a
//                         second tile and runs the per-lane GJK against the origin (timed_walk).  Lanes keep their own running minima; one total-order reduction
//                         (value, partner * 64 + sub-window) at the end (dev_query.h).
//   k_audit_timed_reduce  one wave per owned robot: its S rows -> the record.
// Read-only: the kernels write the audit's own buffers only (no tj_stats counter, no launch count).
#pragma once
#include "kernels_audit.h"

namespace tj {

struct AuditTimedArgs {
  const double* net;   // [U][3][T] control nets: the solver's own, or the copy a group assembled from the owners
  const double* pt;    // [U] piece_time of every robot: the solver's own, or the group's copy
  double range;
  int levels;
  double *row_lo, *row_hi, *row_time;   // [U][S]
  int *row_qlo, *row_qhi;               // [U][S] partner of the row's lo / hi, -1: nothing closer than range
};

__device__ __forceinline__ double clamp01(double x) { return fmin(fmax(x, 0.0), 1.0); }

// the certificate of a GJK result v = (nearest point of body 1) - (nearest point of body 2): v . (a_i - b_j) > 0 for every vertex pair, i.e. v is a separating
// direction and |v| a lower bound on the distance at rounding level.  Without it the bodies may touch, where the GJK stops at up to ~1e-5 instead
// of 0.  Shared by timed_window (body 2 = the origin: d - 0 is d, the bits of its first form) and kernels_obstacle_approach.h.
template <class B1, class B2>
__device__ __forceinline__ bool gjk_separates(const V3& v, const B1& b1, const B2& b2) {
  double m = INFINITY;
#pragma unroll
  for (int i = 0; i < B1::N; i++) {
    const V3 a = b1.get(i);
#pragma unroll
    for (int j = 0; j < B2::N; j++) {
      const V3 b = b2.get(j);
      m = fmin(m, v.x * (a.x - b.x) + v.y * (a.y - b.y) + v.z * (a.z - b.z));
    }
  }
  return m > 0.0;
}

// ---- the pieces of one window, shared with kernels_closest.h (one set of source expressions: the two kernels' windows carry the same bits) ----
// q's segment at t0: T(j) <= t0 < T(j + 1) in the very expressions the cuts use (the quotient only proposes); j == S: q has arrived
__device__ __forceinline__ int timed_first_segment(double t0, double ptq, double res, int S) {
  const double g = floor((t0 / ptq) * res);
  int j = g >= (double)S ? S : (g > 0.0 ? (int)g : 0);
  while (j > 0 && (j / res) * ptq > t0) j--;
  while (j < S && ((j + 1) / res) * ptq <= t0) j++;
  return j;
}

// THE CUTS of a window [t0, t1] of u's time at q's segment boundaries and arrival, in time order: f(j, hover, ca, cb) once per piece [ca, cb], which lies in segment j of q
// (j == S, hover: q has arrived).  The one loop of timed_walk and of kernels_sight_windows.h's seeds: adjacent pieces share an end bit for bit.
template <class F>
__device__ __forceinline__ void timed_cuts(double t0, double t1, double ptq, double res, int S, F&& f) {
  int j = timed_first_segment(t0, ptq, res, S);
  do {
    const bool hover = j >= S;
    const double Tj = (j / res) * ptq, Tj1 = ((j + 1) / res) * ptq;
    f(j, hover, fmax(t0, Tj), hover ? t1 : fmin(t1, Tj1));
    j++;
  } while (j <= S && (j / res) * ptq < t1);
}

// where a window [ca, cb] lies in segment tr of u (sa, sb) and in segment j of q (ra, rb), each in its segment's own parameter: what both raw hulls are restricted to
struct TimedSpan { double sa, sb, ra, rb; };
__device__ __forceinline__ TimedSpan timed_span(double res, double ptu, double ptq, int tr, int j, double ca, double cb) {
  const double T0u = (tr / res) * ptu, T1u = ((tr + 1) / res) * ptu, lenu = T1u - T0u;
  const double Tj = (j / res) * ptq, Tj1 = ((j + 1) / res) * ptq, lenq = Tj1 - Tj;
  return TimedSpan{clamp01((ca - T0u) / lenu), clamp01((cb - T0u) / lenu), clamp01((ca - Tj) / lenq), clamp01((cb - Tj) / lenq)};
}

// q's raw hull of segment j (hover: six times its last control point) into a lane's column of a tile of stride ST
template <int ST>
__device__ __forceinline__ void timed_partner_fill(const Dev& D, const double* nq, int j, bool hover, double* cq) {
  if (hover) {
#pragma unroll
    for (int k = 0; k < 3; k++) { const double v = hull_entry(D, nq, D.S - 1, 5, k); for (int i = 0; i < 6; i++) cq[(3 * i + k) * ST] = v; }
  } else {
    for (int e = 0; e < 18; e++) cq[e * ST] = hull_entry(D, nq, j, e / 3, e % 3);
  }
}

// the same, and whether its box is within `range` of the box of u's raw hull (the skip of the header comment)
__device__ __forceinline__ bool timed_partner_hull(const Dev& D, const double* nq, int j, bool hover, double* cq, const QBox& box, double range) {
  timed_partner_fill<64>(D, nq, j, hover, cq);
  return box_near(cq, 64, box, range);
}

// one window: u's raw hull pa (stride SP) restricted to [sa, sb], q's raw hull cq (stride SQ) to [ra, rb] (hover: as it is), the difference net to the column cd
// (stride SQ); lo = its hull's GJK distance from the origin, h0 / h5 = |d_0| / |d_5|; sep (kernels_closest.h): whether the GJK's v is a separating direction
template <int SP, int SQ>
__device__ __forceinline__ void timed_window(const double* pa, const double* cq, double* cd, bool hover, double sa, double sb, double ra, double rb, double& lo, double& h0, double& h5, bool* sep = nullptr) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double a[6], b[6], oa[6], ob[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { a[i] = pa[(3 * i + k) * SP]; b[i] = cq[(3 * i + k) * SQ]; }
    bez_restrict(a, sa, sb, oa);
    if (hover) {
#pragma unroll
      for (int i = 0; i < 6; i++) ob[i] = b[i];
    } else {
      bez_restrict(b, ra, rb, ob);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) cd[(3 * i + k) * SQ] = oa[i] - ob[i];
  }
  const V3 v = gjk(BodyHullS{cd, SQ}, BodyPoint{V3{0.0, 0.0, 0.0}});
  lo = norm3(v.x, v.y, v.z);
  h0 = norm3(cd[0], cd[SQ], cd[2 * SQ]); h5 = norm3(cd[15 * SQ], cd[16 * SQ], cd[17 * SQ]);
  // does v separate the origin from the hull (v . d_i > 0 for all six points)?  Only there is |v| a lower bound at rounding level
  if (sep) *sep = gjk_separates(v, BodyHullS{cd, SQ}, BodyPoint{V3{0.0, 0.0, 0.0}});
}

// THE WALK of one wave over the partners and cuts of (u, tr) at level L, the single source of the windows' bits (k_audit_timed at the caller's level, k_closest_seed at level
// 0): lane = (partner of the pass, sub-window), P / box the unit's hull and box (query_hull), cq / cd the lane's columns of two 18 x 64 tiles.  f(q, w, j, ca, cb, lo, h0, h5, sep)
// is called once per evaluated window [ca, cb] of sub-window w against segment j of partner q (j == S: q hovers); sep is the GJK's certificate where CERT asks for it.
template <bool CERT, class F>
__device__ __forceinline__ void timed_walk(const Dev& D, const double* net, const double* pt, double range, int L, int u, int tr, const double* P, const QBox& box,
                                           double* cq, double* cd, F&& f) {
  const int lane = lane_id(), S = D.S, U = D.U;
  const double res = (double)D.res, ptu = pt[u];
  const int N = 1 << L, per = 64 >> L, w = lane & (N - 1), ql = lane >> L;
  const double t0 = ((tr + w / (double)N) / res) * ptu, t1 = ((tr + (w + 1) / (double)N) / res) * ptu;   // (the last sub-window ends at T1u bit for bit)
  for (int base = 0; base < U; base += per) {
    const int q = base + ql;
    if (q >= U || q == u) continue;
    const double ptq = pt[q];
    const double* nq = net + (size_t)q * 3 * D.T;
    timed_cuts(t0, t1, ptq, res, S, [&](int j, bool hover, double ca, double cb) {
      if (timed_partner_hull(D, nq, j, hover, cq, box, range)) {
        const TimedSpan sp = timed_span(res, ptu, ptq, tr, j, ca, cb);
        double lo, h0, h5; bool sep = true;
        timed_window<1, 64>(P, cq, cd, hover, sp.sa, sp.sb, sp.ra, sp.rb, lo, h0, h5, CERT ? &sep : nullptr);
        f(q, w, j, ca, cb, lo, h0, h5, sep);
      }
    });
  }
}

__global__ __launch_bounds__(64) void k_audit_timed(Dev D, AuditTimedArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tq[18 * 64], td[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double range = A.range;
  double dlo = range, dhi = range, thi = 0.0; int klo = INT_MAX, khi = INT_MAX;
  if (D.multi()) {
    // lanes keep their own running minima (strict comparisons, ascending order)
    timed_walk<false>(D, A.net, A.pt, range, A.levels, u, tr, P, box, tq + lane, td + lane, [&](int q, int w, int, double ca, double cb, double lo, double h0, double h5, bool) {
      const bool first = h0 <= h5;
      const double hi = first ? h0 : h5;
      if (lo < range && lo < dlo) { dlo = lo; klo = q * 64 + w; }
      if (hi < range && hi < dhi) { dhi = hi; khi = q * 64 + w; thi = first ? ca : cb; }
    });
    wave_argmin(dlo, klo);
    wave_argmin(dhi, khi, thi);
  }
  if (lane == 0) {
    const size_t row = (size_t)u * S + tr;
    A.row_lo[row] = dlo; A.row_qlo[row] = klo == INT_MAX ? -1 : klo >> 6;
    A.row_hi[row] = dhi; A.row_qhi[row] = khi == INT_MAX ? -1 : khi >> 6;
    A.row_time[row] = khi == INT_MAX ? -1.0 : thi;
  }
}

// the S rows of an owned robot -> its record; equal values keep the smaller segment
__global__ __launch_bounds__(64) void k_audit_timed_reduce(Dev D, AuditTimedArgs A, tj_audit_timed_robot* out) {
  const int lane = lane_id(), S = D.S, u = D.u0 + blockIdx.x;
  double dlo = A.range, dhi = A.range, thi = -1.0;
  int slo = INT_MAX, qlo = -1, shi = INT_MAX, qhi = -1;
  for (int tr = lane; tr < S; tr += 64) {   // ascending segments per lane: a strict comparison keeps the first
    const size_t r = (size_t)u * S + tr;
    { const double d = A.row_lo[r]; const int i = A.row_qlo[r]; if (i >= 0 && d < dlo) { dlo = d; slo = tr; qlo = i; } }
    { const double d = A.row_hi[r]; const int i = A.row_qhi[r]; if (i >= 0 && d < dhi) { dhi = d; shi = tr; qhi = i; thi = A.row_time[r]; } }
  }
  wave_argmin(dlo, slo, qlo);
  wave_argmin(dhi, shi, thi, qhi);
  if (lane == 0) {
    tj_audit_timed_robot r;
    r.timed_lo = dlo; r.timed_hi = dhi; r.timed_time = qhi < 0 ? -1.0 : thi;
    r.timed_robot = qhi; r.timed_segment = qhi < 0 ? -1 : shi;
    r.lo_robot = qlo; r.lo_segment = qlo < 0 ? -1 : slo;
    r.levels = A.levels;
    // CONTACT names its partner (as tj_audit's contacts do); CLEAR is a statement about the lower bound alone.  One UAV: nothing to be near.
    r.flags = !D.multi() ? TJ_AUDIT_TIMED_CLEAR : ((qhi >= 0 && dhi <= D.offset ? TJ_AUDIT_TIMED_CONTACT : 0) | (dlo > D.offset ? TJ_AUDIT_TIMED_CLEAR : 0));
    out[u] = r;
  }
}

}  // namespace tj
