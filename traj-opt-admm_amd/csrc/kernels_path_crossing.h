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
//                    deterministic TRUNCATED rule at depth 0.  Then ALL rounds (bnb_rounds, dev_query.h: the round loop of the four branch-and-bound queries)
//                    on ping-pong lists of 48-byte items plus the children's lo.  A child (CrossSearch: item 4 p + c = quadrant c of item p): both raw hulls
//                    restricted in registers into the lane's columns of the two 18-row LDS tiles the seed passes used, the per-lane GJK on BodyHullS and
//                    gjk_separates.
// Read-only: the kernels write the query's own buffers only (no tj_stats counter, no launch count).  No float atomics, no polling, no workgroup waits on another,
// nothing of the iteration's scratch.
#pragma once
#include "kernels_pair_approach.h"

namespace tj {

constexpr int CX_THREADS = 128;   // two waves: the per-lane GJK's registers, two 18-row tiles of 128 columns = 36 KB of LDS

struct CrossItem { double sa, sb, ra, rb, lo; int tr, j; };   // window [sa, sb] of segment tr of u against window [ra, rb] of segment j of q

// the best attained distance: hi between the point at s of u's segment seg and the point at ps of q's segment pseg.  Nothing found: {range, 0, 0, INT_MAX, INT_MAX}
struct CrossBest {
  double hi, s, ps; int seg, pseg;
  __device__ __forceinline__ CrossBest shuffled(int off) const { return CrossBest{__shfl_xor(hi, off), __shfl_xor(s, off), __shfl_xor(ps, off), __shfl_xor(seg, off), __shfl_xor(pseg, off)}; }
};
__device__ __forceinline__ bool before(const CrossBest& a, const CrossBest& b) {
  if (a.hi != b.hi) return a.hi < b.hi;
  if (a.seg != b.seg) return a.seg < b.seg;
  if (a.pseg != b.pseg) return a.pseg < b.pseg;
  if (a.s != b.s) return a.s < b.s;
  return a.ps < b.ps;
}

struct CrossArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  double range, tol;
  int max_depth, max_windows;
  PairIndex ix;        // kernels_pair_approach.h's index of the listed pairs
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

// The crossing search of bnb_rounds (dev_query.h): an item is split into its four quadrants, a child is both raw hulls restricted to their windows in the lane's
// columns of the kernel's two tiles (ha, hb).
struct CrossSearch {
  using Item = CrossItem;
  using Best = CrossBest;
  static constexpr int ARITY = 4;
  static constexpr bool TERMINAL = false;   // dyadic windows, max_depth <= 40: none is ever unsplittable
  using Shared = BnbShared<CrossBest, CX_THREADS, false>;
  const Dev& D; const double* nu; const double* nq; double range;
  double *ca, *cb;   // the lane's columns of ta, tb
  __device__ __forceinline__ CrossBest none() const { return CrossBest{range, 0.0, 0.0, INT_MAX, INT_MAX}; }
  __device__ __forceinline__ CrossItem child(const CrossItem& w, int c, double lo) const {
    const double sm = 0.5 * (w.sa + w.sb), rm = 0.5 * (w.ra + w.rb);
    return CrossItem{c & 1 ? sm : w.sa, c & 1 ? w.sb : sm, c & 2 ? rm : w.ra, c & 2 ? w.rb : rm, lo, w.tr, w.j};
  }
  __device__ __forceinline__ double eval(const CrossItem& w, int c, CrossBest& mine) const {
    const CrossItem k = child(w, c, 0.0);
    const BodyHullS ha{ca, CX_THREADS}, hb{cb, CX_THREADS};
    hull_restrict<CX_THREADS>(D, nu, w.tr, k.sa, k.sb, ca);
    hull_restrict<CX_THREADS>(D, nq, w.j, k.ra, k.rb, cb);
    const double lo = cross_lo(ha, hb);
    cross_hi(ha, hb, w.tr, w.j, k.sa, k.sb, k.ra, k.rb, range, mine);
    return lo;
  }
};

__global__ __launch_bounds__(64) void k_cross_mark(Dev D, CrossArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tile[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double range = A.range;
  unsigned* row = A.ix.mask + (size_t)ui * A.ix.words;
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
  const int p = blockIdx.x, tid = threadIdx.x, S = D.S;
  if (p >= *A.ix.n || p >= A.ix.cap) return;
  __shared__ double ta[18 * CX_THREADS], tb[18 * CX_THREADS];
  __shared__ CrossSearch::Shared sh;
  const int u = A.ix.who[2 * p], q = A.ix.who[2 * p + 1], maxw = A.max_windows;
  const double range = A.range, res = (double)D.res;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double* nq = A.net + (size_t)q * 3 * D.T;
  CrossItem* cur = A.list + (size_t)p * 2 * maxw;
  double* ca = ta + tid; double* cb = tb + tid;
  const CrossSearch search{D, nu, nq, range, ca, cb};
  const BodyHullS ha{ca, CX_THREADS}, hb{cb, CX_THREADS};
  sh.init();

  // ---- the seeds, pass A: the pair's best over the end points of every (tr, j) whose boxes are near; their number is the seeds evaluated ----
  CrossBest mine = search.none();
  int nev = 0;
  for (int i = tid; i < S * S; i += CX_THREADS) {
    const int tr = i / S, j = i - tr * S;
    QBox box;
    for (int e = 0; e < 18; e++) { ca[e * CX_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3); cb[e * CX_THREADS] = hull_entry(D, nq, j, e / 3, e % 3); }   // [0, 1]: the raw hulls
    hull_box(ca, CX_THREADS, box);
    if (!box_near(cb, CX_THREADS, box, range)) continue;
    nev++;
    cross_hi(ha, hb, tr, j, 0.0, 1.0, 0.0, 1.0, range, mine);
  }
  sh.put_best(mine);
  nev = wave_sum(nev);
  if (lane_id() == 0) sh.count(nev);
  __syncthreads();
  CrossBest best = sh.best(search.none());
  // ---- pass B: the seeds' lo; live = {lo < range and lo < best.hi} (the append's order is free: what follows reduces in a total order) ----
  double mlo = INFINITY;
  for (int i = tid; i < S * S; i += CX_THREADS) {
    const int tr = i / S, j = i - tr * S;
    QBox box;
    for (int e = 0; e < 18; e++) { ca[e * CX_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3); cb[e * CX_THREADS] = hull_entry(D, nq, j, e / 3, e % 3); }   // [0, 1]: the raw hulls
    hull_box(ca, CX_THREADS, box);
    if (!box_near(cb, CX_THREADS, box, range)) continue;
    const double lo = cross_lo(ha, hb);
    if (!(lo < range && lo < best.hi)) continue;
    mlo = fmin(mlo, lo);
    bnb_keep(sh.kept, cur, maxw, CrossItem{0.0, 1.0, 0.0, 1.0, lo, tr, j});
  }
  sh.put_lo(mlo);
  __syncthreads();   // (also: the live list is written, `kept` is final)
  int n = sh.kept;
  mlo = sh.lo(mlo);
  __syncthreads();   // everyone has read the seeding's words before the first round writes them
  double lo_u = fmin(best.hi, mlo);
  int depth = 0;
  bool truncated = n > maxw;
  bnb_rounds<CX_THREADS>(search, sh, A.tol, A.max_depth, maxw, cur, cur + maxw, A.klo + (size_t)p * 4 * maxw, best, lo_u, n, depth, truncated);
  if (tid == 0) {
    tj_crossing_record r;
    const bool found = best.seg != INT_MAX;
    r.lo = lo_u; r.hi = best.hi; r.s = found ? best.s : -1.0; r.partner_s = found ? best.ps : -1.0;
    r.time = found ? ((best.seg + best.s) / res) * A.pt[u] : -1.0;            // log_data's sigma * piece_time, tj_obstacle_approach's expression
    r.partner_time = found ? ((best.pseg + best.ps) / res) * A.pt[q] : -1.0;
    r.robot = u; r.partner = q; r.segment = found ? best.seg : -1; r.partner_segment = found ? best.pseg : -1;
    r.depth = depth; r.windows = sh.ev; r.reserved = 0;   // the seeds evaluated and the rounds' children
    r.flags = bnb_flags(found, best.hi, lo_u, A.tol, n, truncated, D.offset) |
              (found && best.seg == S - 1 && best.s == 1.0 ? TJ_CROSSING_ROBOT_END : 0) | (found && best.pseg == S - 1 && best.ps == 1.0 ? TJ_CROSSING_PARTNER_END : 0);
    out[p] = r;
  }
}

}  // namespace tj
