// kernels_timing_margin.h -- tj_timing_margin: by how much may one robot run late or early against another before the two come within `dist`.
//
// tj_path_crossings compares two flown curves as curves and reports partner_time - time at the closest place; the tolerance a timetable has is smaller: contact
// begins at distance `dist`, not 0, and a robot that has arrived stays at its goal.  Here the objective is a TIME, subject to a distance constraint: per unordered
// pair u < q the infimum of the slip over all (x on u's path, y on q's path) with |x - y| <= dist, by the pair's own branch and bound over tj_path_crossings' items.
// The definition (include/trajadmm.h):
//   clock    T_r(g, s) = ((g + s) / res) * piece_time[r]; the last control point (g == S - 1, s == 1.0) has the clock set [T, +inf), every other point {T};
//            slip of two points = the distance of their clock sets = max(0, lo_u - hi_q, lo_q - hi_u)
//   item     CrossItem: (tr, j, [sa, sb], [ra, rb]), dyadic windows, both nets restricted from the RAW hulls (hull_restrict)
//   OUT      cross_lo(W) > dist (the GJK's |v| with its certificate, else 0): no contact inside, klo = +inf
//   klo(W)   not OUT: the distance of the windows' clock intervals, max(0, ta_u - tb_q, ta_q - tb_u), tb = +inf where the window ends on the last control point
//   corners  the four end-point pairs i, k in {0, 5} with norm3(a_i - b_k) <= dist, each with the slip of its two points
//   same time   not OUT and klo == 0 only: tau = max(ta_u, ta_q, 0), each robot's x = (tau - T(g, 0)) / (T(g + 1, 0) - T(g, 0)) clamped into the item's window
//            (tj_flight_profile's expressions), position = b_0 of the raw hull restricted to [x, x]; within dist: slip 0.0, stated, SAME_TIME
//   order    candidates with slip < max_slip, by (slip, segment, partner_segment, s, partner_s); a corner goes before a same-time candidate of the same place
//   seeds    every (tr, j) whose raw hull boxes pass box_near at dist, full windows, evaluated like a round's children: live = {klo < the seeds' FINAL best}
//   listed   some seed has a candidate, or is not OUT with klo < max_slip
//   round    bnb_rounds (dev_query.h) unchanged: ARITY 4, no terminal items, Best.hi = the slip, eval returns klo
//
// THREE launches whatever the fleet's size, the number of pairs and the depth (a count-only call ends after the second):
//   k_margin_mark     k_cross_mark's shape: one wave per (owned robot u, segment tr), lane = partner q > u; the corners first, the GJK only where klo < max_slip
//   k_pair_index      kernels_pair_approach.h's scan over the bitmask
//   k_margin_refine   k_cross_refine's shape: one workgroup of MG_THREADS per pair slot.  Pass A takes the corner candidates of every near seed (no GJK).  Pass B
//                     runs the GJK of every near seed, takes the same-time candidate of those that are not OUT with klo == 0 -- it needs "not OUT", so it cannot
//                     go into pass A -- and appends {not OUT and klo < pass A's best}.  A same-time candidate is the only thing pass B can add to the best, and its
//                     slip is 0: no seed has klo < 0, so the live set against the seeds' final best is then empty, and is set so.  Then ALL rounds.
// Read-only: the kernels write the query's own buffers only.  No float atomics, no polling, no workgroup waits on another, nothing of the iteration's scratch.
#pragma once
#include "kernels_path_crossing.h"

namespace tj {

constexpr int MG_THREADS = 128;   // two waves, as k_cross_refine: the per-lane GJK's registers, two 18-row tiles of 128 columns = 36 KB of LDS

// the best attained slip: hi between the point at s of u's segment seg and the point at ps of q's segment pseg.  Nothing found: {max_slip, 0, 0, INT_MAX, 0}.
// same: a same-time candidate (its slip is stated, not computed from its parameters).  The sample's distance does not travel with it (two registers through the GJK
// for every record held): margin_point at (seg, s) and (pseg, ps) gives a candidate's two points bit for bit -- a corner is five de Casteljau steps at its own
// parameter, whichever window it was a corner of --, so the record's distance is formed once, behind the rounds.
// key: (segment << 16) | partner_segment (piece_num * res <= 511), ordered as the pair is; INT_MAX: nothing found.
struct MarginBest {
  double hi, s, ps; int key, same;
  __device__ __forceinline__ MarginBest shuffled(int off) const { return MarginBest{__shfl_xor(hi, off), __shfl_xor(s, off), __shfl_xor(ps, off), __shfl_xor(key, off), __shfl_xor(same, off)}; }
  __device__ __forceinline__ bool found() const { return key != INT_MAX; }
  __device__ __forceinline__ int seg() const { return key >> 16; }
  __device__ __forceinline__ int pseg() const { return key & 0xffff; }
};
__device__ __forceinline__ bool before(const MarginBest& a, const MarginBest& b) {
  if (a.hi != b.hi) return a.hi < b.hi;
  if (a.key != b.key) return a.key < b.key;
  if (a.s != b.s) return a.s < b.s;
  if (a.ps != b.ps) return a.ps < b.ps;
  return a.same < b.same;
}

struct MarginArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  double range, tol;   // range: the contact distance `dist`
  double max_slip;
  int max_depth, max_windows;
  PairIndex ix;        // kernels_pair_approach.h's index of the listed pairs
  CrossItem* list;     // [cap][2][max_windows] ping-pong live lists
  double* klo;         // [cap][4 * max_windows] klo of the round's children
};

// the clocks of one pair: robot u's and partner q's piece times
struct MarginClock {
  double res, ptu, ptq; int S;
  __device__ __forceinline__ double at(double pt, int g, double s) const { return ((g + s) / res) * pt; }
  // the upper end of a point's clock set: the robot stays at its last control point
  __device__ __forceinline__ double end(double pt, int g, double s) const { return g == S - 1 && s == 1.0 ? INFINITY : at(pt, g, s); }
  // the distance of the windows' clock intervals
  __device__ __forceinline__ double klo(int tr, int j, double sa, double sb, double ra, double rb) const {
    return fmax(0.0, fmax(at(ptu, tr, sa) - end(ptq, j, rb), at(ptq, j, ra) - end(ptu, tr, sb)));
  }
};

// the four corner candidates of one item into the lane's best
__device__ __forceinline__ void margin_corners(const BodyHullS& a, const BodyHullS& b, const MarginClock& ck, int tr, int j, double sa, double sb, double ra, double rb,
                                               double dist, double max_slip, MarginBest& mine) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const V3 x = a.get(e & 2 ? 5 : 0), y = b.get(e & 1 ? 5 : 0);
    const double su = e & 2 ? sb : sa, sq = e & 1 ? rb : ra;
    const double slip = fmax(0.0, fmax(ck.at(ck.ptu, tr, su) - ck.end(ck.ptq, j, sq), ck.at(ck.ptq, j, sq) - ck.end(ck.ptu, tr, su)));
    const MarginBest c{slip, su, sq, (tr << 16) | j, 0};
    if (norm3(x.x - y.x, x.y - y.y, x.z - y.z) <= dist && slip < max_slip && before(c, mine)) mine = c;
  }
}

// where a robot is in segment g at clock value tau, kept inside [sa, sb]; and the point there: b_0 of the raw hull restricted to [x, x] (bez_restrict's row of five steps at x)
__device__ __forceinline__ double margin_param(const MarginClock& ck, double pt, int g, double tau, double sa, double sb) {
  const double t0 = ck.at(pt, g, 0.0), t1 = ck.at(pt, g + 1, 0.0);
  return fmin(fmax((tau - t0) / (t1 - t0), sa), sb);
}
__device__ __forceinline__ V3 margin_point(const Dev& D, const double* __restrict__ net, int g, double x) {
  const double ux = 1 - x;
  double o[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double r[6];
#pragma unroll
    for (int i = 0; i < 6; i++) r[i] = hull_entry(D, net, g, i, k);
#pragma unroll
    for (int s = 0; s < 5; s++)
#pragma unroll
      for (int m = 0; m < 5 - s; m++) r[m] = ux * r[m] + x * r[m + 1];
    o[k] = r[0];
  }
  return V3{o[0], o[1], o[2]};
}
// the same-time candidate of an item that is not OUT and whose clock intervals overlap
__device__ __forceinline__ void margin_same_time(const Dev& D, const double* nu, const double* nq, const MarginClock& ck, int tr, int j, double sa, double sb, double ra, double rb,
                                                 double dist, double max_slip, MarginBest& mine) {
  const double tau = fmax(fmax(ck.at(ck.ptu, tr, sa), ck.at(ck.ptq, j, ra)), 0.0);
  const double xu = margin_param(ck, ck.ptu, tr, tau, sa, sb), xq = margin_param(ck, ck.ptq, j, tau, ra, rb);
  const V3 x = margin_point(D, nu, tr, xu), y = margin_point(D, nq, j, xq);
  const MarginBest c{0.0, xu, xq, (tr << 16) | j, 1};
  if (norm3(x.x - y.x, x.y - y.y, x.z - y.z) <= dist && 0.0 < max_slip && before(c, mine)) mine = c;
}

// The margin search of bnb_rounds (dev_query.h): CrossSearch's items and nets; the objective is the slip
struct MarginSearch {
  using Item = CrossItem;
  using Best = MarginBest;
  static constexpr int ARITY = 4;
  static constexpr bool TERMINAL = false;   // dyadic windows, max_depth <= 40: none is ever unsplittable
  using Shared = BnbShared<MarginBest, MG_THREADS, false>;
  const Dev& D; const double* nu; const double* nq; double dist, max_slip; MarginClock ck;
  double *ca, *cb;   // the lane's columns of ta, tb
  __device__ __forceinline__ MarginBest none() const { return MarginBest{max_slip, 0.0, 0.0, INT_MAX, 0}; }
  __device__ __forceinline__ CrossItem child(const CrossItem& w, int c, double lo) const {
    const double sm = 0.5 * (w.sa + w.sb), rm = 0.5 * (w.ra + w.rb);
    return CrossItem{c & 1 ? sm : w.sa, c & 1 ? w.sb : sm, c & 2 ? rm : w.ra, c & 2 ? w.rb : rm, lo, w.tr, w.j};
  }
  __device__ __forceinline__ double eval(const CrossItem& w, int c, MarginBest& mine) const {
    const CrossItem k = child(w, c, 0.0);
    const BodyHullS ha{ca, MG_THREADS}, hb{cb, MG_THREADS};
    hull_restrict<MG_THREADS>(D, nu, w.tr, k.sa, k.sb, ca);
    hull_restrict<MG_THREADS>(D, nq, w.j, k.ra, k.rb, cb);
    const double lo = cross_lo(ha, hb);
    margin_corners(ha, hb, ck, w.tr, w.j, k.sa, k.sb, k.ra, k.rb, dist, max_slip, mine);
    if (lo > dist) return INFINITY;   // OUT
    const double klo = ck.klo(w.tr, w.j, k.sa, k.sb, k.ra, k.rb);
    if (klo == 0.0) margin_same_time(D, nu, nq, ck, w.tr, w.j, k.sa, k.sb, k.ra, k.rb, dist, max_slip, mine);
    return klo;
  }
};

__global__ __launch_bounds__(64) void k_margin_mark(Dev D, MarginArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tile[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double dist = A.range, max_slip = A.max_slip;
  unsigned* row = A.ix.mask + (size_t)ui * A.ix.words;
  const BodyHullS own{P, 1}, oth{tile + lane, 64};
  for (int base = ((u + 1) >> 6) << 6; base < D.U; base += 64) {
    const int q = base + lane;
    if (q <= u || q >= D.U) continue;   // (no barrier below: a lane reads its own column and the unit's hull only)
    const double* nq = A.net + (size_t)q * 3 * D.T;
    const MarginClock ck{(double)D.res, A.pt[u], A.pt[q], S};
    for (int j = 0; j < S; j++) {
      for (int e = 0; e < 18; e++) tile[e * 64 + lane] = hull_entry(D, nq, j, e / 3, e % 3);
      if (!box_near(tile + lane, 64, box, dist)) continue;
      MarginBest mine{max_slip, 0.0, 0.0, INT_MAX, 0};
      margin_corners(own, oth, ck, tr, j, 0.0, 1.0, 0.0, 1.0, dist, max_slip, mine);
      if (mine.found() || (ck.klo(tr, j, 0.0, 1.0, 0.0, 1.0) < max_slip && !(cross_lo(own, oth) > dist))) { atomicOr(&row[q >> 5], 1u << (q & 31)); break; }
    }
  }
}

__global__ __launch_bounds__(MG_THREADS) void k_margin_refine(Dev D, MarginArgs A, tj_margin_record* out) {
  const int p = blockIdx.x, tid = threadIdx.x, S = D.S;
  if (p >= *A.ix.n || p >= A.ix.cap) return;
  __shared__ double ta[18 * MG_THREADS], tb[18 * MG_THREADS];
  __shared__ MarginSearch::Shared sh;
  const int u = A.ix.who[2 * p], q = A.ix.who[2 * p + 1], maxw = A.max_windows;
  const double dist = A.range, max_slip = A.max_slip;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double* nq = A.net + (size_t)q * 3 * D.T;
  CrossItem* cur = A.list + (size_t)p * 2 * maxw;
  double* ca = ta + tid; double* cb = tb + tid;
  const MarginClock ck{(double)D.res, A.pt[u], A.pt[q], S};
  const MarginSearch search{D, nu, nq, dist, max_slip, ck, ca, cb};
  const BodyHullS ha{ca, MG_THREADS}, hb{cb, MG_THREADS};
  sh.init();

  // ---- the seeds, pass A: the corner candidates of every (tr, j) whose boxes are near; their number is the seeds evaluated ----
  MarginBest mine = search.none();
  int nev = 0;
  for (int i = tid; i < S * S; i += MG_THREADS) {
    const int tr = i / S, j = i - tr * S;
    QBox box;
    for (int e = 0; e < 18; e++) { ca[e * MG_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3); cb[e * MG_THREADS] = hull_entry(D, nq, j, e / 3, e % 3); }   // [0, 1]: the raw hulls
    hull_box(ca, MG_THREADS, box);
    if (!box_near(cb, MG_THREADS, box, dist)) continue;
    nev++;
    margin_corners(ha, hb, ck, tr, j, 0.0, 1.0, 0.0, 1.0, dist, max_slip, mine);
  }
  sh.put_best(mine);
  nev = wave_sum(nev);
  if (lane_id() == 0) sh.count(nev);
  __syncthreads();
  MarginBest best = sh.best(search.none());
  __syncthreads();   // everyone has read pass A's words before pass B writes them
  // ---- pass B: the seeds' GJK and same-time candidates; appended = {not OUT and klo < pass A's best} (the append's order is free) ----
  double mlo = INFINITY;
  mine = best;
  for (int i = tid; i < S * S; i += MG_THREADS) {
    const int tr = i / S, j = i - tr * S;
    QBox box;
    for (int e = 0; e < 18; e++) { ca[e * MG_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3); cb[e * MG_THREADS] = hull_entry(D, nq, j, e / 3, e % 3); }   // [0, 1]: the raw hulls
    hull_box(ca, MG_THREADS, box);
    if (!box_near(cb, MG_THREADS, box, dist)) continue;
    if (cross_lo(ha, hb) > dist) continue;   // OUT
    const double klo = ck.klo(tr, j, 0.0, 1.0, 0.0, 1.0);
    if (klo == 0.0) margin_same_time(D, nu, nq, ck, tr, j, 0.0, 1.0, 0.0, 1.0, dist, max_slip, mine);
    if (!(klo < best.hi)) continue;
    mlo = fmin(mlo, klo);
    bnb_keep(sh.kept, cur, maxw, CrossItem{0.0, 1.0, 0.0, 1.0, klo, tr, j});
  }
  sh.put_best(mine);
  sh.put_lo(mlo);
  __syncthreads();   // (also: the live list is written, `kept` is final)
  int n = sh.kept;
  mlo = sh.lo(mlo);
  best = sh.best(best);
  __syncthreads();   // everyone has read the seeding's words before the first round writes them
  if (best.hi == 0.0) { n = 0; mlo = INFINITY; }   // live against the seeds' FINAL best: no seed has klo < 0
  double lo_u = fmin(best.hi, mlo);
  int depth = 0;
  bool truncated = n > maxw;
  bnb_rounds<MG_THREADS>(search, sh, A.tol, A.max_depth, maxw, cur, cur + maxw, A.klo + (size_t)p * 4 * maxw, best, lo_u, n, depth, truncated);
  if (tid == 0) {
    tj_margin_record r;
    const bool found = best.found();
    const int seg = best.seg(), pseg = best.pseg();
    r.distance = -1.0;
    if (found) {
      const V3 x = margin_point(D, nu, seg, best.s), y = margin_point(D, nq, pseg, best.ps);
      r.distance = norm3(x.x - y.x, x.y - y.y, x.z - y.z);
    }
    r.lo = lo_u; r.hi = best.hi; r.s = found ? best.s : -1.0; r.partner_s = found ? best.ps : -1.0;
    r.time = found ? ck.at(ck.ptu, seg, best.s) : -1.0;
    r.partner_time = found ? ck.at(ck.ptq, pseg, best.ps) : -1.0;
    r.robot = u; r.partner = q; r.segment = found ? seg : -1; r.partner_segment = found ? pseg : -1;
    r.depth = depth; r.windows = sh.ev; r.reserved = 0;   // the seeds evaluated and the rounds' children
    r.flags = bnb_flags(found, best.hi, lo_u, A.tol, n, truncated, 0.0) |
              (found && seg == S - 1 && best.s == 1.0 ? TJ_MARGIN_ROBOT_END : 0) | (found && pseg == S - 1 && best.ps == 1.0 ? TJ_MARGIN_PARTNER_END : 0) |
              (found && best.same ? TJ_MARGIN_SAME_TIME : 0);
    out[p] = r;
  }
}

}  // namespace tj
