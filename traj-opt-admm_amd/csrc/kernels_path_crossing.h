// kernels_path_crossing.h -- tj_path_crossings: where the PATHS of two robots meet in space, whatever the time, and when each robot is there.
//
// Every other robot-against-robot query compares the robots at equal flight times (or equal segment indices); a fleet they all certify may still have two paths
// through one point a few tenths of a second apart.  Here the two flown curves are compared as curves: the minimum over all x on u's and all y on q's of |x - y|,
// per unordered pair u < q, by the pair's own branch and bound over TWO windows.  The definition (include/trajadmm.h):
//   item     (tr, j, [sa, sb], [ra, rb]): a window of segment tr of u and a window of segment j of q, both dyadic in the segments' local parameters
//   nets     the RAW hulls (hull_entry's sums) restricted to the windows by bez_restrict, never a parent's net; [0, 1] is the raw hull bit for bit
//   lo(W)    |v|, v = gjk(hull of u's net, hull of q's net) (u < q: u's is body 1, plane_pair's order) where gjk_separates holds over the 36 vertex pairs, else 0
//   hi(W)    the smallest of norm3(a_i - b_k), i, k in {0, 5}: points of the two curves at the windows' ends; order (hi, segment, partner_segment, s, partner_s)
//   seeds    every (tr, j) whose hull boxes pass box_near at `range`, full windows;  listed: some seed has lo < range or hi < range
//   round    every live item into its four quadrants, all children evaluated, best over the round, keep lo < best.hi (strict, the round's FINAL best)
//   bracket  lo = min(best.hi, min lo over live), hi = best.hi;  stop: hi - lo <= tol | live empty | max_depth | more than max_windows live (TRUNCATED)
//
// THREE launches whatever the fleet's size, the number of pairs and the depth (a count-only call, cap == 0, ends after the second):
//   k_cross_mark     one wave per (owned robot u, segment tr), lane = partner q > u of the pass; the lane walks q's S segments: raw hull into its column of an
//                    18-row tile, box_near, and where the boxes are near the seed's lo and hi.  The first seed with lo < range or hi < range sets the pair's bit in
//                    the [owned][words] bitmask with an integer atomic OR and ends the lane's walk.
//   k_pair_index     kernels_pair_approach.h's one-workgroup scan over the bitmask: pair p is the p-th set bit in (robot, partner) order.
//   k_cross_refine   one workgroup of CX_THREADS per pair slot; slots at or beyond n or cap exit at once.  The pair enumerates its own S^2 box tests, twice: pass A
//                    takes the four end-point distances of every seed (no GJK) for the pair's best; pass B runs the GJK of every seed and appends
//                    {lo < range and lo < best.hi} to the pair's list -- so no buffer is sized by S^2, and more than max_windows live seeds is the
//                    deterministic TRUNCATED rule at depth 0.  Then ALL rounds on ping-pong lists of 48-byte items plus the children's lo: lanes take the
//                    children strided (item 4 p + c = quadrant c of item p), restrict both raw hulls in registers into their columns of two 18-row LDS tiles,
//                    run the per-lane GJK on BodyHullS and gjk_separates; a total-order reduction over the workgroup gives the round's best; the keep pass is
//                    bnb_keep on an integer LDS counter.
// Read-only: the kernels write the query's own buffers only (no tj_stats counter, no launch count).  No float atomics, no polling, no workgroup waits on another,
// nothing of the iteration's scratch.
#pragma once
#include "kernels_pair_approach.h"

namespace tj {

constexpr int CX_THREADS = 128;   // two waves: the per-lane GJK's registers, two 18-row tiles of 128 columns = 36 KB of LDS

struct CrossItem { double sa, sb, ra, rb, lo; int tr, j; };   // window [sa, sb] of segment tr of u against window [ra, rb] of segment j of q

// the best attained distance: hi between the point at s of u's segment seg and the point at ps of q's segment pseg.  Nothing found: {range, 0, 0, INT_MAX, INT_MAX}
struct CrossBest { double hi, s, ps; int seg, pseg; };
__device__ __forceinline__ bool before(const CrossBest& a, const CrossBest& b) {
  if (a.hi != b.hi) return a.hi < b.hi;
  if (a.seg != b.seg) return a.seg < b.seg;
  if (a.pseg != b.pseg) return a.pseg < b.pseg;
  if (a.s != b.s) return a.s < b.s;
  return a.ps < b.ps;
}
__device__ __forceinline__ void wave_best(CrossBest& m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const CrossBest o{__shfl_xor(m.hi, off), __shfl_xor(m.s, off), __shfl_xor(m.ps, off), __shfl_xor(m.seg, off), __shfl_xor(m.pseg, off)};
    if (before(o, m)) m = o;
  }
}

struct CrossArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  double range, tol;
  int max_depth, max_windows, cap;
  int words;           // 32-bit words per bitmask row
  unsigned* mask;      // [owned][words] bit q of row u - u0: (u, q) is listed
  int* wordoff;        // [owned][words] listed pairs before this word in (robot, partner) order
  int* n;              // [1] listed pairs
  int* who;            // [cap][2] robot, partner of a slot
  CrossItem* list;     // [cap][2][max_windows] ping-pong live lists
  double* klo;         // [cap][4 * max_windows] lo of the round's children
};

// lo of one item: the GJK's |v| where v separates the two hulls, else 0
__device__ __forceinline__ double cross_lo(const BodyHullS& a, const BodyHullS& b) {
  const V3 v = gjk(a, b);
  return gjk_separates(v, a, b) ? norm3(v.x, v.y, v.z) : 0.0;
}

// the four attained candidates of one item into the lane's best
__device__ __forceinline__ void cross_hi(const BodyHullS& a, const BodyHullS& b, int tr, int j, double sa, double sb, double ra, double rb, double range, CrossBest& mine) {
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const V3 x = a.get(e & 2 ? 5 : 0), y = b.get(e & 1 ? 5 : 0);
    const CrossBest c{norm3(x.x - y.x, x.y - y.y, x.z - y.z), e & 2 ? sb : sa, e & 1 ? rb : ra, tr, j};
    if (c.hi < range && before(c, mine)) mine = c;
  }
}

// segment tr of `net` restricted to [sa, sb] into a column of stride ST
template <int ST>
__device__ __forceinline__ void cross_net(const Dev& D, const double* net, int tr, double sa, double sb, double* col) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double a[6], o[6];
#pragma unroll
    for (int i = 0; i < 6; i++) a[i] = hull_entry(D, net, tr, i, k);
    bez_restrict(a, sa, sb, o);
#pragma unroll
    for (int i = 0; i < 6; i++) col[(3 * i + k) * ST] = o[i];
  }
}

// the box of a 6-point hull behind a stride (query_hull's loops)
__device__ __forceinline__ void cross_box(const double* p, int st, QBox& q) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < 6; i++) { const double v = p[(3 * i + k) * st]; if (v < lo) lo = v; if (v > hi) hi = v; }
    q.lo[k] = lo; q.hi[k] = hi;
  }
}

__global__ __launch_bounds__(64) void k_cross_mark(Dev D, CrossArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tile[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double range = A.range;
  unsigned* row = A.mask + (size_t)ui * A.words;
  const BodyHullS own{P, 1}, oth{tile + lane, 64};
  for (int base = ((u + 1) >> 6) << 6; base < D.U; base += 64) {
    const int q = base + lane;
    if (q <= u || q >= D.U) continue;   // (no barrier below: a lane reads its own column and the unit's hull only)
    const double* nq = A.net + (size_t)q * 3 * D.T;
    for (int j = 0; j < S; j++) {
      for (int e = 0; e < 18; e++) tile[e * 64 + lane] = hull_entry(D, nq, j, e / 3, e % 3);
      if (!box_near(tile + lane, 64, box, range)) continue;
      CrossBest mine{range, 0.0, 0.0, INT_MAX, INT_MAX};
      cross_hi(own, oth, tr, j, 0.0, 1.0, 0.0, 1.0, range, mine);
      if (mine.seg != INT_MAX || cross_lo(own, oth) < range) { atomicOr(&row[q >> 5], 1u << (q & 31)); break; }
    }
  }
}

__global__ __launch_bounds__(CX_THREADS) void k_cross_refine(Dev D, CrossArgs A, tj_crossing_record* out) {
  constexpr int NW = CX_THREADS / 64;
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6, S = D.S;
  if (p >= *A.n || p >= A.cap) return;
  __shared__ double ta[18 * CX_THREADS], tb[18 * CX_THREADS];
  __shared__ CrossBest wbest[NW];
  __shared__ double wlo[NW];
  __shared__ int wev[NW], kept;
  const int u = A.who[2 * p], q = A.who[2 * p + 1], maxw = A.max_windows;
  const double range = A.range, res = (double)D.res;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double* nq = A.net + (size_t)q * 3 * D.T;
  CrossItem* cur = A.list + (size_t)p * 2 * maxw; CrossItem* nxt = cur + maxw;
  double* klo = A.klo + (size_t)p * 4 * maxw;
  double* ca = ta + tid; double* cb = tb + tid;
  const BodyHullS ha{ca, CX_THREADS}, hb{cb, CX_THREADS};
  const CrossBest none{range, 0.0, 0.0, INT_MAX, INT_MAX};

  // ---- the seeds, pass A: the pair's best over the end points of every (tr, j) whose boxes are near; their number is the seeds evaluated ----
  CrossBest mine = none;
  int nev = 0;
  for (int i = tid; i < S * S; i += CX_THREADS) {
    const int tr = i / S, j = i - tr * S;
    QBox box;
    for (int e = 0; e < 18; e++) { ca[e * CX_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3); cb[e * CX_THREADS] = hull_entry(D, nq, j, e / 3, e % 3); }   // [0, 1]: the raw hulls
    cross_box(ca, CX_THREADS, box);
    if (!box_near(cb, CX_THREADS, box, range)) continue;
    nev++;
    cross_hi(ha, hb, tr, j, 0.0, 1.0, 0.0, 1.0, range, mine);
  }
  wave_best(mine); nev = wave_sum(nev);
  if (lane == 0) { wbest[wave] = mine; wev[wave] = nev; }
  if (tid == 0) kept = 0;
  __syncthreads();
  CrossBest best = none;
  int windows = 0;
  for (int k = 0; k < NW; k++) { if (before(wbest[k], best)) best = wbest[k]; windows += wev[k]; }
  // ---- pass B: the seeds' lo; live = {lo < range and lo < best.hi} (the append's order is free: what follows reduces in a total order) ----
  double mlo = INFINITY;
  for (int i = tid; i < S * S; i += CX_THREADS) {
    const int tr = i / S, j = i - tr * S;
    QBox box;
    for (int e = 0; e < 18; e++) { ca[e * CX_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3); cb[e * CX_THREADS] = hull_entry(D, nq, j, e / 3, e % 3); }   // [0, 1]: the raw hulls
    cross_box(ca, CX_THREADS, box);
    if (!box_near(cb, CX_THREADS, box, range)) continue;
    const double lo = cross_lo(ha, hb);
    if (!(lo < range && lo < best.hi)) continue;
    mlo = fmin(mlo, lo);
    bnb_keep(kept, cur, maxw, CrossItem{0.0, 1.0, 0.0, 1.0, lo, tr, j});
  }
  mlo = wave_min(mlo);
  if (lane == 0) wlo[wave] = mlo;
  __syncthreads();   // (also: the live list is written, `kept` is final)
  int n = kept;
  for (int k = 0; k < NW; k++) mlo = fmin(mlo, wlo[k]);
  __syncthreads();   // everyone has read the seeding's words before the first round writes them
  double lo_u = fmin(best.hi, mlo);
  int depth = 0;
  bool truncated = n > maxw;

  while (!truncated && !(best.hi - lo_u <= A.tol) && n > 0 && depth < A.max_depth) {
    // ---- pass 1: the four quadrants of every live item, one child per lane ----
    mine = none;
    for (int i = tid; i < 4 * n; i += CX_THREADS) {
      const CrossItem w = cur[i >> 2];
      const int c = i & 3;
      const double sm = 0.5 * (w.sa + w.sb), rm = 0.5 * (w.ra + w.rb);
      const double sa = c & 1 ? sm : w.sa, sb = c & 1 ? w.sb : sm, ra = c & 2 ? rm : w.ra, rb = c & 2 ? w.rb : rm;
      cross_net<CX_THREADS>(D, nu, w.tr, sa, sb, ca);
      cross_net<CX_THREADS>(D, nq, w.j, ra, rb, cb);
      klo[i] = cross_lo(ha, hb);
      cross_hi(ha, hb, w.tr, w.j, sa, sb, ra, rb, range, mine);
    }
    wave_best(mine);
    if (lane == 0) wbest[wave] = mine;
    if (tid == 0) kept = 0;
    __syncthreads();   // (also: every klo of the round is written)
    CrossBest cand = best;
    for (int k = 0; k < NW; k++) if (before(wbest[k], cand)) cand = wbest[k];
    windows += 4 * n;
    // ---- pass 2: keep what can still hold something below the round's best ----
    mlo = INFINITY;
    for (int i = tid; i < 4 * n; i += CX_THREADS) {
      const double lo = klo[i];
      if (!(lo < cand.hi)) continue;
      const CrossItem w = cur[i >> 2];
      const int c = i & 3;
      const double sm = 0.5 * (w.sa + w.sb), rm = 0.5 * (w.ra + w.rb);
      mlo = fmin(mlo, lo);
      bnb_keep(kept, nxt, maxw, CrossItem{c & 1 ? sm : w.sa, c & 1 ? w.sb : sm, c & 2 ? rm : w.ra, c & 2 ? w.rb : rm, lo, w.tr, w.j});
    }
    mlo = wave_min(mlo);
    if (lane == 0) wlo[wave] = mlo;
    __syncthreads();   // (also: the new list is written, `kept` is final)
    const int m = kept;
    for (int k = 0; k < NW; k++) mlo = fmin(mlo, wlo[k]);
    __syncthreads();   // everyone has read the round's words before the next round writes them
    if (m > maxw) { truncated = true; break; }
    best = cand; lo_u = fmin(best.hi, mlo); n = m; depth++;
    CrossItem* t = cur; cur = nxt; nxt = t;
  }
  if (tid == 0) {
    tj_crossing_record r;
    const bool found = best.seg != INT_MAX;
    r.lo = lo_u; r.hi = best.hi; r.s = found ? best.s : -1.0; r.partner_s = found ? best.ps : -1.0;
    r.time = found ? ((best.seg + best.s) / res) * A.pt[u] : -1.0;            // log_data's sigma * piece_time, tj_obstacle_approach's expression
    r.partner_time = found ? ((best.pseg + best.ps) / res) * A.pt[q] : -1.0;
    r.robot = u; r.partner = q; r.segment = found ? best.seg : -1; r.partner_segment = found ? best.pseg : -1;
    r.depth = depth; r.windows = windows; r.reserved = 0;
    r.flags = (found && best.hi <= D.offset ? TJ_CROSSING_CONTACT : 0) | (lo_u > D.offset ? TJ_CROSSING_CLEAR : 0) |
              (best.hi - lo_u <= A.tol || (n == 0 && !truncated) ? TJ_CROSSING_CONVERGED : 0) | (truncated ? TJ_CROSSING_TRUNCATED : 0) |
              (found && best.seg == S - 1 && best.s == 1.0 ? TJ_CROSSING_ROBOT_END : 0) | (found && best.pseg == S - 1 && best.ps == 1.0 ? TJ_CROSSING_PARTNER_END : 0);
    out[p] = r;
  }
}

}  // namespace tj
