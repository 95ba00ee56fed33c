// kernels_proximity.h -- tj_proximity_windows: WHEN is each directed robot pair within a distance `dist` at equal flight times, as certified time intervals.
//
// The branch-and-bound siblings look for one extremum and prune against a best.  This query classifies the whole time axis of a pair against a level and keeps
// everything that is not certified outside.  Time, hover, hull formation, the cuts at the partner's segment boundaries, the restriction of both RAW hulls and the box
// skip are kernels_audit_timed.h's (timed_walk at level 0 for the seeds, timed_window for the children: one set of source expressions).  The definition
// (include/trajadmm.h), per directed pair (u, q), u owned:
//   window   lo (the GJK's |v| with its certificate `sep`, 0 without one), h0 / h5 (the separations attained at ca / cb), and ub = the largest norm3(d_i) over the
//            six points of the same difference net (prox_ub reads the column timed_window filled): the curve lies in the net's hull and a norm is convex
//   class    OUT: sep && lo > dist | IN: ub <= dist | MIXED: the rest (prox_class, in this order)
//   listed   some level-0 seed that passes the box prefilter at range = dist is not OUT
//   search   kept = the IN seeds, live = the MIXED seeds.  A round: a live window with cb - ca <= tol, or whose midpoint is not strictly inside, goes to kept as an EDGE
//            leaf; every other is halved and both children are evaluated from the raw hulls: OUT dropped, IN to kept, MIXED to the next live set.  Stop: live empty |
//            max_depth | live or kept above max_windows (TRUNCATED: kept and live of the last completed round).  At the end the live windows become EDGE leaves.
//   merge    the leaves sorted by ca (distinct: the windows of a pair are disjoint); adjacent iff prev.cb == next.ca on doubles; a row per maximal chain
//
// At most five launches whatever the fleet's size, the number of pairs and the depth (a count-only call, cap == 0, ends after the second):
//   k_prox_mark     one wave per (owned robot, segment), timed_walk at level 0 with the certificate.  A window that is not OUT sets the pair's bit (integer atomic OR).
//   k_pair_index    kernels_pair_approach.h's: pair p is the p-th set bit of the bitmask, so the listing's order is a function of the state alone.
//   k_prox_seed     the walk again (the same bits).  A window of a listed pair whose slot is below cap is counted in the pair's `windows`; IN and MIXED windows are
//                   appended to the PAIR's seed list with their class, h0 and h5 (bnb_keep on the pair's counter; at most 2 S + 2 windows at level 0).
//   k_prox_refine   one wave per pair slot.  ALL rounds in the kernel on the pair's slices of global buffers (a ping-pong live list and the kept list, both counted in
//                   LDS as bnb_keep does), then the live windows join the kept list as EDGE leaves, the leaves are sorted by ca (win_sort: the order of the appends
//                   vanishes here) and the chain heads counted: the pair's row count (leaf 0 is a head: a pair's chains do not go on anywhere).
//   k_prox_place    one wave per pair slot: win_rows_before gives the pair's first row; the chain heads of a block of 64 leaves get their row index from
//                   win_row_index, and the lane of a head folds its chain left to right (WinChain) and writes the row where it belongs.  Rows beyond the caller's
//                   capacity are counted, not written.
// The classifying round loop is this file's (bnb_rounds prunes against a best and does not fit).  The bounded append and THE MERGE HALF are dev_query.h's, shared with
// kernels_obstacle_windows.h: the classes and flag bits (WIN_*), the rank sort with the interior heads, the row indexing, the chain fold with the flag rule.  This
// file's own: a leaf's times are its [ca, cb] and its width cb - ca, the next leaf is the next of the pair's list, a row has a partner and no index (the closest
// sample's ties end at the time).  LDS per wave: k_pair_refine's three 18-row tiles of 64 columns (27 KB), so the per-lane GJK's registers set the occupancy.
// Read-only: the kernels write the query's own buffers only (no tj_stats counter, no launch count).  No float atomics, no polling, no workgroup waits on another.
#pragma once
#include "kernels_pair_approach.h"

namespace tj {

constexpr int PX_THREADS = 64;    // one wave per pair

struct ProxSeed { double ca, cb, h0, h5; int tr, j, cls, pad; };   // a level-0 window of a listed pair that is not OUT
struct ProxWin { double ca, cb, h0, h5; int tr, j; };              // a live (MIXED) window: [ca, cb] in segment tr of u and segment j of q (j == S: q hovers)
struct ProxLeaf { double ca, cb, h0, h5; int in, pad; };           // a kept window: IN, or an EDGE leaf

struct ProxArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  double range, tol;   // range: dist
  int max_depth, max_windows;
  int seed_cap;        // seeds per pair slot (2 S + 2)
  int leaf_cap;        // leaves per pair slot (2 * max_windows + seed_cap)
  int row_cap;         // the caller's rows
  PairIndex ix;        // (ix.cap: the pair slots)
  int* count;          // [cap][2] seeds appended, windows evaluated by the seeding
  ProxSeed* seeds;     // [cap][seed_cap]
  ProxWin* list;       // [cap][2][max_windows] ping-pong live lists
  ProxLeaf* leaf;      // [cap][leaf_cap] the kept list, in the order of the appends
  ProxLeaf* sorted;    // [cap][leaf_cap] the leaves by ca
  int* info;           // [cap][4] rows, leaves, depth (+ 1 << 16: truncated), windows
  int* n_rows;         // [1]
};

// the largest control-vector norm of the difference net in a lane's column (stride ST): an upper bound of the separation over the window
template <int ST>
__device__ __forceinline__ double prox_ub(const double* cd) {
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < 6; i++) m = fmax(m, norm3(cd[(3 * i) * ST], cd[(3 * i + 1) * ST], cd[(3 * i + 2) * ST]));
  return m;
}
__device__ __forceinline__ int prox_class(bool sep, double lo, double ub, double dist) { return sep && lo > dist ? WIN_OUT : (ub <= dist ? WIN_IN : WIN_MIXED); }

__global__ __launch_bounds__(64) void k_prox_mark(Dev D, ProxArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tq[18 * 64], td[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double dist = A.range;
  unsigned* row = A.ix.mask + (size_t)ui * A.ix.words;
  timed_walk<true>(D, A.net, A.pt, dist, 0, u, tr, P, box, tq + lane, td + lane, [&](int q, int, int, double, double, double lo, double, double, bool sep) {
    if (!(sep && lo > dist)) atomicOr(&row[q >> 5], 1u << (q & 31));   // (not OUT, whatever ub says)
  });
}

__global__ __launch_bounds__(64) void k_prox_seed(Dev D, ProxArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tq[18 * 64], td[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double dist = A.range;
  const size_t row = (size_t)ui * A.ix.words;
  const double* cd = td + lane;
  timed_walk<true>(D, A.net, A.pt, dist, 0, u, tr, P, box, tq + lane, td + lane, [&](int q, int, int j, double ca, double cb, double lo, double h0, double h5, bool sep) {
    const unsigned m = A.ix.mask[row + (q >> 5)], bit = 1u << (q & 31);
    if (!(m & bit)) return;
    const int slot = A.ix.wordoff[row + (q >> 5)] + __popc(m & (bit - 1));
    if (slot >= A.ix.cap) return;
    atomicAdd(&A.count[2 * slot + 1], 1);
    const int cls = prox_class(sep, lo, prox_ub<64>(cd), dist);
    if (cls != WIN_OUT) bnb_keep(A.count[2 * slot], A.seeds + (size_t)slot * A.seed_cap, A.seed_cap, ProxSeed{ca, cb, h0, h5, tr, j, cls, 0});
  });
}

// one child [ca, cb] of a window in segment tr of u and segment j of q, from the raw hulls in the lane's columns of the three tiles (TimedSearch::eval's expressions)
__device__ __forceinline__ int prox_eval(const Dev& D, const double* nu, double ptu, const double* nq, double ptq, int tr, int j, double ca, double cb, double dist,
                                         double* cp, double* cq, double* cd, double& h0, double& h5) {
  const int S = D.S;
  const double res = (double)D.res;
  const bool hover = j >= S;
  for (int e = 0; e < 18; e++) cp[e * PX_THREADS] = hull_entry(D, nu, tr, e / 3, e % 3);
  timed_partner_fill<PX_THREADS>(D, nq, j, hover, cq);
  const TimedSpan sp = timed_span(res, ptu, ptq, tr, j, ca, cb);
  double lo; bool sep;
  timed_window<PX_THREADS, PX_THREADS>(cp, cq, cd, hover, sp.sa, sp.sb, sp.ra, sp.rb, lo, h0, h5, &sep);
  return prox_class(sep, lo, prox_ub<PX_THREADS>(cd), dist);
}

__device__ __forceinline__ bool prox_is_leaf(double ca, double cb, double tol) {
  const double cm = 0.5 * (ca + cb);
  return cb - ca <= tol || !(ca < cm && cm < cb);
}

__global__ __launch_bounds__(PX_THREADS) void k_prox_refine(Dev D, ProxArgs A) {
  const int p = blockIdx.x, tid = threadIdx.x;
  if (p >= *A.ix.n || p >= A.ix.cap) return;
  __shared__ double tp[18 * PX_THREADS], tq[18 * PX_THREADS], td[18 * PX_THREADS];
  __shared__ int s_kept, s_live, s_ev;
  const int u = A.ix.who[2 * p], q = A.ix.who[2 * p + 1], maxw = A.max_windows;
  const double dist = A.range, tol = A.tol;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double* nq = A.net + (size_t)q * 3 * D.T;
  const double ptu = A.pt[u], ptq = A.pt[q];
  const ProxSeed* seeds = A.seeds + (size_t)p * A.seed_cap;
  const int ns = min(A.count[2 * p], A.seed_cap);
  ProxWin* cur = A.list + (size_t)p * 2 * maxw;
  ProxWin* nxt = cur + maxw;
  ProxLeaf* leaf = A.leaf + (size_t)p * A.leaf_cap;
  ProxLeaf* sorted = A.sorted + (size_t)p * A.leaf_cap;
  if (tid == 0) { s_kept = 0; s_live = 0; s_ev = 0; }
  __syncthreads();

  // ---- the seeds: IN to the kept list (it holds every seed), MIXED to the live list ----
  for (int i = tid; i < ns; i += PX_THREADS) {
    const ProxSeed s = seeds[i];
    if (s.cls == WIN_IN) bnb_keep(s_kept, leaf, A.leaf_cap, ProxLeaf{s.ca, s.cb, s.h0, s.h5, 1, 0});
    else bnb_keep(s_live, cur, maxw, ProxWin{s.ca, s.cb, s.h0, s.h5, s.tr, s.j});
  }
  __syncthreads();
  int kept = s_kept, n = s_live, depth = 0;
  const bool seed_overflow = n > maxw || kept > maxw;
  bool truncated = seed_overflow;
  __syncthreads();   // everyone has read the counters before the first round writes them

  // ---- the rounds: every thread holds the same kept, n, depth, truncated ----
  while (!truncated && n > 0 && depth < A.max_depth) {
    if (tid == 0) s_live = 0;   // (s_kept goes on from the committed count)
    __syncthreads();
    for (int i = tid; i < 2 * n; i += PX_THREADS) {
      const ProxWin w = cur[i >> 1];
      const int c = i & 1;
      if (prox_is_leaf(w.ca, w.cb, tol)) {
        if (c == 0) bnb_keep(s_kept, leaf, maxw, ProxLeaf{w.ca, w.cb, w.h0, w.h5, 0, 0});
        continue;
      }
      const double cm = 0.5 * (w.ca + w.cb);
      const double ca = c ? cm : w.ca, cb = c ? w.cb : cm;
      double h0, h5;
      const int cls = prox_eval(D, nu, ptu, nq, ptq, w.tr, w.j, ca, cb, dist, tp + tid, tq + tid, td + tid, h0, h5);
      atomicAdd(&s_ev, 1);
      if (cls == WIN_IN) bnb_keep(s_kept, leaf, maxw, ProxLeaf{ca, cb, h0, h5, 1, 0});
      else if (cls == WIN_MIXED) bnb_keep(s_live, nxt, maxw, ProxWin{ca, cb, h0, h5, w.tr, w.j});
    }
    __syncthreads();   // the lists are written, the counters final
    const int k2 = s_kept, n2 = s_live;
    __syncthreads();   // everyone has read them
    if (k2 > maxw || n2 > maxw) {   // the committed lists stand: the appends of this round do not count
      truncated = true;
      break;
    }
    kept = k2; n = n2; depth++;
    ProxWin* t = cur; cur = nxt; nxt = t;
  }

  // ---- the live windows of the last completed round become EDGE leaves (an overflow among the seeds: straight from the seed list) ----
  if (seed_overflow) {
    if (tid == 0) s_kept = kept;
    __syncthreads();
    for (int i = tid; i < ns; i += PX_THREADS) {
      const ProxSeed s = seeds[i];
      if (s.cls == WIN_MIXED) bnb_keep(s_kept, leaf, A.leaf_cap, ProxLeaf{s.ca, s.cb, s.h0, s.h5, 0, 0});
    }
    __syncthreads();
    kept = s_kept;
  } else {
    for (int i = tid; i < n; i += PX_THREADS) {
      const ProxWin w = cur[i];
      leaf[kept + i] = ProxLeaf{w.ca, w.cb, w.h0, w.h5, 0, 0};
    }
    kept += n;
    __syncthreads();
  }
  const int m = kept;   // <= leaf_cap: at most 2 * max_windows from the rounds, at most seed_cap from the seeds alone

  // ---- by ca, and the chain heads: leaf 0 is one ----
  const int heads = win_sort<&ProxLeaf::ca, &ProxLeaf::cb>(leaf, sorted, m) + (m > 0 ? 1 : 0);
  if (tid == 0) {
    A.info[4 * p] = heads; A.info[4 * p + 1] = m; A.info[4 * p + 2] = depth | (truncated ? 1 << 16 : 0);
    A.info[4 * p + 3] = A.count[2 * p + 1] + s_ev;   // the seeding's windows and the rounds'
  }
}

// the rows of pair slot p at their final place: behind the rows of the slots before it, chain after chain in time order
__global__ __launch_bounds__(PX_THREADS) void k_prox_place(Dev D, ProxArgs A, tj_proximity_row* out) {
  const int p = blockIdx.x, lane = lane_id();
  const int np = min(*A.ix.n, A.ix.cap);
  if (p >= np) return;
  int base = win_rows_before(A.info, 4, p);   // the pair's first row
  const int heads = A.info[4 * p], m = A.info[4 * p + 1], dt = A.info[4 * p + 2], windows = A.info[4 * p + 3];
  if (p == np - 1 && lane == 0) *A.n_rows = base + heads;
  const int u = A.ix.who[2 * p], q = A.ix.who[2 * p + 1];
  const double dist = A.range, tol = A.tol;
  const double t_end = ((D.S - 1 + 1) / (double)D.res) * A.pt[u];   // the end of u's last segment, in the walk's expression
  const ProxLeaf* sorted = A.sorted + (size_t)p * A.leaf_cap;
  for (int i0 = 0; i0 < m; i0 += PX_THREADS) {
    const int i = i0 + lane;
    const bool head = win_head<&ProxLeaf::ca, &ProxLeaf::cb>(sorted, i, m, true);
    const int r = win_row_index(head, base);
    if (!head || r >= A.row_cap) continue;
    // the chain from leaf i on, left to right
    tj_proximity_row row;
    WinChain ch;
    double end = 0.0;
    int k = i;
    for (;;) {
      const ProxLeaf x = sorted[k];
      ch.add(dist, x.ca, x.cb, x.cb - x.ca, x.in, x.h0, x.h5);
      end = x.cb;
      k++;
      if (k >= m || sorted[k].ca != end) break;
    }
    const double t0 = sorted[i].ca;
    ch.finish(row, t0, end, t0 == 0.0, end == t_end, (dt >> 16) != 0, tol);
    row.closest_time = ch.best_t;
    row.robot = u; row.partner = q; row.leaves = k - i; row.depth = dt & 0xffff; row.windows = windows;
    out[r] = row;
  }
}

}  // namespace tj
