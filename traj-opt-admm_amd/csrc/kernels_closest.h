// kernels_closest.h -- tj_closest_approach: every robot's closest approach to another robot at EQUAL FLIGHT TIMES, converged to a tolerance.
//
// tj_audit_timed brackets the separation with a UNIFORM split of every segment's window of time (2^levels parts, levels <= 6).  Here the same certified
// bounds drive a branch and bound: a window W has lo(W) (GJK distance of the difference net's hull from the origin: nothing on W is closer) and hi(W) (an end
// point: a separation attained at a known time).  lo counts only where the GJK's v SEPARATES the origin from the hull (v . d_i > 0 for all six points); without
// that certificate the origin may be inside, where the GJK stops at up to ~1e-5 instead of 0, and lo(W) = 0.  A window whose lo is not below the smallest hi found so far cannot hold the minimum and is dropped; the
// others are halved.  Time, hover, hull formation, the cuts at the partner's segment boundaries, the restriction of both nets and the box skip are
// kernels_audit_timed.h's (timed_walk for the seeds, timed_window for the children: one set of source expressions); the record QBest with its order
// (hi, segment, partner, time) and the bounded append are dev_query.h's.  The definition (include/trajadmm.h), per owned robot u:
//   seeds    the windows (tr, q, j, ca, cb) k_audit_timed evaluates at levels = 0.  best = the smallest hi < range, ties by (segment, partner, time);
//            live = {lo < range and lo < best.hi}
//   round d  every live window is halved at cm = 0.5 * (ca + cb); cm == ca or cm == cb: it stays in the set as terminal.  Both children are evaluated by
//            restricting the RAW segment hulls (never the parent's net: rounding does not grow with depth).  best over (best, children of the round) in the
//            order (hi, segment, partner, time); then live = the children and terminals with lo < best.hi -- compared with the round's FINAL best, so the
//            set does not depend on the order of evaluation
//   bracket  lo_u = min(best.hi, min lo over live), hi_u = best.hi
//   stop     hi_u - lo_u <= tol | live empty | every live window terminal | d == max_depth | more than max_windows live (TRUNCATED: the record of the last
//            completed round is returned; `windows` counts the overflowing round's work too)
// The round loop itself -- two passes, three barriers, the truncation rule, the ping-pong lists -- is bnb_rounds (dev_query.h), one function for this query,
// tj_pair_approach, tj_obstacle_approach and tj_path_crossings; this file states the timed-window search it runs (TimedSearch).
//
// Four launches whatever the fleet's size and the depth:
//   k_audit_timed (levels 0), k_audit_timed_reduce   the level-0 bracket per robot: best (hi, segment, partner, time) and the smallest lo
//   k_closest_seed     one wave per (owned robot, segment), timed_walk at level 0 with the certificate (lane = partner of the pass).  A lane whose window has
//                      lo < best.hi appends it to the robot's list with one integer atomic on the robot's counter (append order is free: nothing
//                      downstream depends on it; the windows below best.hi are a handful per robot, so there is nothing for a ballot to save).  The
//                      number of windows evaluated is summed over the wave and added once.
//   k_closest_refine   one workgroup of CL_THREADS per owned robot runs ALL rounds on the robot's slice of a global buffer allocated on the first call (40-byte
//                      records; a live list is a few windows, read once per round: L2 traffic, no LDS staging).  A child: the raw hulls of (u, tr) and (q, j)
//                      into the lane's columns of two LDS tiles, timed_window into the third.  No workgroup waits on another; no polling, no cross-queue
//                      word, nothing of the iteration's scratch.
// Read-only: the kernels write the query's own buffers only (no tj_stats counter, no launch count).
#pragma once
#include "kernels_audit_timed.h"

namespace tj {

constexpr int CL_THREADS = 128;   // two waves: the per-lane GJK's registers and three 18-row tiles of 128 columns = 54 KB of LDS

struct ClosestWin { double ca, cb, lo; int tr, q, j, term; };   // one live window: [ca, cb] in segment tr of u and segment j of q (j == S: q hovers)

struct ClosestArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  double range, tol;
  int max_depth, max_windows;
  const tj_audit_timed_robot* seed;   // [U] the level-0 bracket
  ClosestWin* list;    // [U][2][TJ_CLOSEST_FRONTIER] ping-pong live lists
  double* klo;         // [U][2 * TJ_CLOSEST_FRONTIER] lo of the round's children
  int* count;          // [U][3]: live windows after seeding (may exceed max_windows: overflow), windows evaluated by the seeding, 1 = a live seed has no certificate (lo 0)
};

__global__ __launch_bounds__(64) void k_closest_seed(Dev D, ClosestArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tq[18 * 64], td[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double range = A.range, besthi = A.seed[u].timed_hi;
  ClosestWin* list = A.list + (size_t)u * 2 * TJ_CLOSEST_FRONTIER;
  int nev = 0;
  timed_walk<true>(D, A.net, A.pt, range, 0, u, tr, P, box, tq + lane, td + lane, [&](int q, int, int j, double ca, double cb, double lo, double, double, bool sep) {
    if (!sep) lo = 0.0;
    nev++;
    if (lo < range && lo < besthi) {
      if (!sep) atomicOr(&A.count[3 * u + 2], 1);
      bnb_keep(A.count[3 * u], list, A.max_windows, ClosestWin{ca, cb, lo, tr, q, j, 0});
    }
  });
  nev = wave_sum(nev);
  if (lane == 0 && nev) atomicAdd(&A.count[3 * u + 1], nev);
}

// The timed-window search of bnb_rounds (dev_query.h) by a workgroup of THREADS threads (k_closest_refine: a robot's windows; kernels_pair_approach.h: one pair's):
// a window is halved in time, a child is evaluated by timed_window on the raw hulls in the lane's columns of the kernel's three 18-row tiles.
template <int THREADS>
struct TimedSearch {
  using Item = ClosestWin;
  using Best = QBest;
  static constexpr int ARITY = 2;
  static constexpr bool TERMINAL = true;
  using Shared = BnbShared<QBest, THREADS, true>;
  const Dev& D; const double* net; const double* pt;
  const double* nu; double ptu, range;   // u's net and piece time
  double *cp, *cq, *cd;   // the lane's columns of tp, tq, td
  __device__ __forceinline__ QBest none() const { return QBest{range, 0.0, INT_MAX, INT_MAX}; }
  __device__ __forceinline__ bool terminal(const ClosestWin& w) const { const double cm = 0.5 * (w.ca + w.cb); return w.term || cm == w.ca || cm == w.cb; }
  __device__ __forceinline__ double eval(const ClosestWin& w, int c, QBest& mine) const {
    const int S = D.S;
    const double res = (double)D.res;
    const double cm = 0.5 * (w.ca + w.cb);
    const double ca = c ? cm : w.ca, cb = c ? w.cb : cm;
    const bool hover = w.j >= S;
    const double ptq = pt[w.q];
    for (int e = 0; e < 18; e++) cp[e * THREADS] = hull_entry(D, nu, w.tr, e / 3, e % 3);
    timed_partner_fill<THREADS>(D, net + (size_t)w.q * 3 * D.T, w.j, hover, cq);
    const TimedSpan sp = timed_span(res, ptu, ptq, w.tr, w.j, ca, cb);
    double lo, h0, h5; bool sep;
    timed_window<THREADS, THREADS>(cp, cq, cd, hover, sp.sa, sp.sb, sp.ra, sp.rb, lo, h0, h5, &sep);
    if (!sep) lo = 0.0;
    const bool first = h0 <= h5;
    const QBest b{first ? h0 : h5, first ? ca : cb, w.tr, w.q};
    if (b.hi < range && before(b, mine)) mine = b;
    return lo;
  }
  __device__ __forceinline__ ClosestWin child(const ClosestWin& w, int c, double lo) const {
    const double cm = 0.5 * (w.ca + w.cb);
    return terminal(w) ? ClosestWin{w.ca, w.cb, lo, w.tr, w.q, w.j, 1} : ClosestWin{c ? cm : w.ca, c ? w.cb : cm, lo, w.tr, w.q, w.j, 0};
  }
};

__global__ __launch_bounds__(CL_THREADS) void k_closest_refine(Dev D, ClosestArgs A, tj_closest_robot* out) {
  const int tid = threadIdx.x, u = D.u0 + blockIdx.x;
  __shared__ double tp[18 * CL_THREADS], tq[18 * CL_THREADS], td[18 * CL_THREADS];
  __shared__ TimedSearch<CL_THREADS>::Shared sh;
  const tj_audit_timed_robot seed = A.seed[u];
  ClosestWin* cur = A.list + (size_t)u * 2 * TJ_CLOSEST_FRONTIER;
  sh.init();

  // the committed record: the level-0 bracket (every thread holds the same values)
  QBest best{seed.timed_hi, seed.timed_time, seed.timed_robot < 0 ? INT_MAX : seed.timed_segment, seed.timed_robot < 0 ? INT_MAX : seed.timed_robot};
  double lo_u = A.count[3 * u + 2] ? 0.0 : fmin(seed.timed_lo, seed.timed_hi);   // min(best.hi, min lo over the live seeds): tj_audit_timed's, unless a live seed counts 0
  int n = A.count[3 * u], depth = 0;
  bool truncated = n > A.max_windows;
  if (D.multi())
    bnb_rounds<CL_THREADS>(TimedSearch<CL_THREADS>{D, A.net, A.pt, A.net + (size_t)u * 3 * D.T, A.pt[u], A.range, tp + tid, tq + tid, td + tid}, sh, A.tol, A.max_depth, A.max_windows,
                           cur, cur + TJ_CLOSEST_FRONTIER, A.klo + (size_t)u * 2 * TJ_CLOSEST_FRONTIER, best, lo_u, n, depth, truncated);
  if (tid == 0) {
    tj_closest_robot r;
    const bool found = best.id != INT_MAX;
    r.lo = lo_u; r.hi = best.hi; r.time = found ? best.x : -1.0;
    r.robot = found ? best.id : -1; r.segment = found ? best.seg : -1;
    r.depth = depth; r.windows = A.count[3 * u + 1] + sh.ev; r.reserved = 0;   // the seeding's windows and the rounds'
    r.flags = !D.multi() ? (TJ_CLOSEST_CLEAR | TJ_CLOSEST_CONVERGED) : bnb_flags(found, best.hi, lo_u, A.tol, n, truncated, D.offset);
    out[u] = r;
  }
}

}  // namespace tj
