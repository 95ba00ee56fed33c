// kernels_audit.h -- tj_audit: a read-only report on the state the solver holds (clearances, dynamic limits, duration).
//
// The reference never reports these numbers; it only ever uses them inside its stages:
//   obstacle clearance   the GJK distance |v| between a segment's 6-point hull and an obstacle primitive -- the quantity Separate::opengjk
//                        (Separate.h:107-151) and the CCD clamp (Step.h:83-97) compare with their ranges;
//   robot-pair clearance the same between the hulls of two robots on the SAME segment index, the pairing of separate_self / self_step
//                        (Optimization3D_multi.h:246-259, Step.h:196-208).  Decoupled robots carry their own piece_time, so equal segment
//                        indices are not equal flight times: this is the solver's own notion of "the pair", not a continuous-time distance (kernels_audit_timed.h is);
//   speed / acceleration the two quantities bound_energy subtracts from vel_limit / acc_limit (Energy_admm.h:131-165), in the expressions and
//                        the association of the line search: its own functions (dev_common.h hull_speed / hull_accel).
//
//   k_audit         one wave per (owned robot, segment): hull with hull_entry's sums (the bits of the hull cache), BVH walk through
//                   bvh_query with m = range (a primitive closer than `range` to the hull has its box within `range` of the hull's box, so
//                   min(range, min over candidates) is exact), per batch of up to 64 candidates one per-lane GJK each, then the robots
//                   q != u of the same segment one per lane (lower robot index = body 1, as plane_pair), then the segment's 5 velocity
//                   and 4 acceleration terms.  Minima are reduced across the wave with a total order (distance, index; dev_query.h).
//   k_audit_reduce  one wave per owned robot: its S rows -> the robot's record.
//
// Read-only: the kernels write the audit's own buffers only.  The frontier arrays of the walk are the unit's own LDS (FRONT_CAP entries, as in every
// other user of bvh_query); the overflow bit goes to the queries' control block (Dev::ctl of the COPY the kernels receive: tj_api.hip), never to the
// solver's.  No `visits` counter is passed: tj_stats does not move.
#pragma once
#include "dev_query.h"

namespace tj {

struct AuditArgs {
  const double* net;     // [U][3][T] control nets the audit reads: the solver's own, or the copy a group assembled from the owners
  const int* order;      // sorted primitive -> index in the caller's obstacle list
  double range;
  double *row_obs, *row_pair, *row_speed, *row_accel;   // [U][S]
  int *row_prim, *row_q;                                 // [U][S] argmin primitive (caller's index) / robot, -1: nothing closer than range
};

template <int PRIM>
__global__ __launch_bounds__(64) void k_audit(Dev D, AuditArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tile[18 * 64];
  __shared__ int walk[WalkScratch::INTS];
  QBox q;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, q);
  const double range = A.range;
  const size_t row = (size_t)u * S + tr;

  // ---- obstacles: every primitive whose box is within `range` of the hull's box, one per lane ----
  double od = range; int oi = INT_MAX;
  bvh_query<1, PRIM>(D, q, range, WalkScratch::carve(walk), nullptr, [&](int pt) {
    if (pt >= 0) {
      const V3 v = gjk(BodyHull{P}, PrimOf<PRIM>::load(D, pt));
      const double d = norm3(v.x, v.y, v.z);
      const int idx = A.order[pt];
      if (d < range && (d < od || (d == od && idx < oi))) { od = d; oi = idx; }
    }
  });
  wave_argmin(od, oi);

  // ---- the other robots on this segment, one per lane ----
  double pd = range; int pq = INT_MAX;
  if (D.multi()) {
    for (int base = 0; base < D.U; base += 64) {
      const int qr = base + lane;
      bool live = qr < D.U && qr != u;
      __syncthreads();
      if (live) {
        const double* nq = A.net + (size_t)qr * 3 * D.T;
        for (int e = 0; e < 18; e++) tile[e * 64 + lane] = hull_entry(D, nq, tr, e / 3, e % 3);
        live = box_near(tile + lane, 64, q, range);
      }
      if (live) {
        const BodyHullS own{P, 1}, oth{tile + lane, 64};
        const bool first = u < qr;   // plane_pair's order: the hull of the lower robot index is body 1
        const V3 v = gjk(first ? own : oth, first ? oth : own);
        const double d = norm3(v.x, v.y, v.z);
        if (d < range && (d < pd || (d == pd && qr < pq))) { pd = d; pq = qr; }
      }
    }
    wave_argmin(pd, pq);
  }

  // ---- dynamic limits: the line search's own functions (dev_common.h hull_speed / hull_accel; Energy_admm.h:131-165), weight = the segment's table value ----
  const double w = seg_weight(D, tr), pt = D.piece_time[u];
  double sp = -1.0, ac = -1.0;
  if (lane < 5) sp = hull_speed(P, lane, w, pt);
  if (lane < 4) ac = hull_accel(P, lane, w, pt);
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) { sp = fmax(sp, __shfl_xor(sp, off)); ac = fmax(ac, __shfl_xor(ac, off)); }
  if (lane == 0) {
    A.row_obs[row] = od; A.row_prim[row] = oi == INT_MAX ? -1 : oi;
    A.row_pair[row] = pd; A.row_q[row] = pq == INT_MAX ? -1 : pq;
    A.row_speed[row] = sp; A.row_accel[row] = ac;
  }
}

// the S rows of an owned robot -> its record; equal values keep the smaller segment
__global__ __launch_bounds__(64) void k_audit_reduce(Dev D, AuditArgs A, tj_audit_robot* out) {
  const int lane = lane_id(), S = D.S, u = D.u0 + blockIdx.x;
  double od = A.range, pd = A.range, nsp = 1.0, nac = 1.0;   // nsp / nac: the negated maxima, so that one reduction serves all four
  int os = INT_MAX, oi = -1, ps = INT_MAX, pq = -1, ss = INT_MAX, as = INT_MAX;
  for (int tr = lane; tr < S; tr += 64) {   // ascending segments per lane: a strict comparison keeps the first
    const size_t r = (size_t)u * S + tr;
    { const double d = A.row_obs[r]; const int i = A.row_prim[r]; if (i >= 0 && d < od) { od = d; os = tr; oi = i; } }
    { const double d = A.row_pair[r]; const int i = A.row_q[r]; if (i >= 0 && d < pd) { pd = d; ps = tr; pq = i; } }
    { const double v = -A.row_speed[r]; if (v < nsp) { nsp = v; ss = tr; } }
    { const double v = -A.row_accel[r]; if (v < nac) { nac = v; as = tr; } }
  }
  wave_argmin(od, os, oi); wave_argmin(pd, ps, pq); wave_argmin(nsp, ss); wave_argmin(nac, as);
  if (lane == 0) {
    const double pt = D.piece_time[u];
    double dur = 0;
    for (int i = 0; i < D.P; i++) dur += 1.0 * pt;   // log_data's sum (time_weight == 1): piece_num * piece_time
    tj_audit_robot r;
    r.obs_clearance = od; r.obs_segment = oi < 0 ? -1 : os; r.obs_index = oi;
    r.pair_clearance = pd; r.pair_segment = pq < 0 ? -1 : ps; r.pair_robot = pq;
    r.speed = -nsp; r.accel = -nac; r.speed_segment = ss; r.accel_segment = as;
    r.duration = dur;
    // a contact names what is in contact: with range <= offset and nothing found, od == range <= offset is the search limit, not a clearance
    r.flags = (oi >= 0 && od <= D.offset ? TJ_AUDIT_OBS_CONTACT : 0) | (pq >= 0 && pd <= D.offset ? TJ_AUDIT_PAIR_CONTACT : 0) |
              (-nsp >= D.vel_limit ? TJ_AUDIT_SPEED : 0) | (-nac >= D.acc_limit ? TJ_AUDIT_ACCEL : 0);
    r.reserved = 0;
    out[u] = r;
  }
}

}  // namespace tj
