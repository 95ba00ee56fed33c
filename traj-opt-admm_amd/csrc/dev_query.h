// dev_query.h -- what the read-only queries on the held state share (tj_audit, tj_audit_timed, tj_closest_approach, tj_obstacle_approach, tj_obstacle_windows, tj_sight_windows, tj_pair_approach, tj_path_crossings, tj_timing_margin, tj_proximity_windows, tj_flight_profile, tj_peak_dynamics, tj_dynamics_windows, tj_zone_windows), each piece defined once.
//
// Every query works per (owned robot, segment) on the segment's 6-point hull (hull_entry's sums: the bits of the hull cache) and its box, and reduces per-lane candidates
// with a TOTAL order, so that a result is a function of the state alone: no float atomics, no dependence on the order of evaluation.
//   hull_box, query_hull   the box of a 6-point hull behind a stride; the unit's hull into LDS and its box
//   box_near       the box-gap skip: is a 6-point hull's box within `range` of the unit's box on every axis
//   bez_restrict, bez_restrict_n, hull_restrict   a quintic's Bezier net restricted to a window, the same for any degree; a segment's raw hull restricted into a lane's column of a tile
//   wave_argmin    the smallest (value, key) in lexicographic order over the wave, with whatever travels along
//   QBest          the record of the timed and the obstacle branch and bound, ordered by (hi, segment, id, parameter): before, shuffled
//   wave_best / wave_min / wave_sum, BnbShared   the reductions over a wave, and over a workgroup through its LDS words
//   bnb_keep, bnb_rounds, bnb_flags   the bounded append, THE ROUND LOOP of the five branch-and-bound queries, and their four common flag bits
//   WIN_*, win_sort, win_head, win_rows_before, win_row_index, WinChain, WinRowFold, win_time   THE MERGE HALF of the five window queries (tj_proximity_windows, tj_obstacle_windows, tj_sight_windows, tj_dynamics_windows, tj_zone_windows): the classes and
//                  the six flag bits, the leaves' rank sort with the interior chain heads, a head's row index, the fold of a chain into a row's common fields and flags, and a flight position's time
//   WinSlotArgs, win_lane_search, win_put, win_live_cap, win_leaf_cap, win_slot_place   THE SLOT QUERIES tj_dynamics_windows and tj_zone_windows: one lane-per-window search per slot by one wave, a template
//                  on the evaluation, and the slot's rows at their final place, a template on the row writer
//   win_wave_rounds, win_seg_first_is_head, win_seg_count, win_seg_place   THE WAVE-COOPERATIVE QUERIES tj_obstacle_windows and tj_sight_windows: the rounds of one (owner, segment) unit whose evaluation is the whole
//                  wave's, a template on the evaluation, and the owner's row count and rows with the chains that cross segment boundaries, templates on how a key maps to position and time
//                  (tj_proximity_windows uses the merge half only: its refine is lane-per-child with live and leaf types of its own and a seed kernel)
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

// the box of a 6-point hull behind a stride (min / max: exact)
__device__ __forceinline__ void hull_box(const double* p, int st, QBox& q) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < 6; i++) { const double v = p[(3 * i + k) * st]; if (v < lo) lo = v; if (v > hi) hi = v; }
    q.lo[k] = lo; q.hi[k] = hi;
  }
}

// the unit's hull (segment tr of the robot whose control net is `net`) into P[18] and its box; one wave, ends behind a barrier
__device__ __forceinline__ void query_hull(const Dev& D, const double* net, int tr, double* P, QBox& q) {
  const int lane = lane_id();
  if (lane < 18) P[lane] = hull_entry(D, net, tr, lane / 3, lane % 3);
  __syncthreads();
  hull_box(P, 1, q);
}

// Boxes further apart than `range` on an axis: the hulls are at least that far apart, and so is whatever lies inside them.  (Rounding is monotonic, so a true gap <= range
// never compares greater; the guard keeps a pair whose gap is within rounding of `range` in the GJK, whose |v| decides.)  p, st: the other hull, as BodyHullS.
__device__ __forceinline__ bool box_near(const double* p, int st, const QBox& q, double range) {
  QBox o;
  hull_box(p, st, o);
  bool near = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double gap = fmax(o.lo[k] - q.hi[k], q.lo[k] - o.hi[k]);
    near = near && !(gap > range * 1.000001 + 1e-9);
  }
  return near;
}

// the Bezier net of a quintic restricted to [sa, sb] of its parameter: o[i] = blossom(sa x (5 - i), sb x i).  Row s of the triangle (s steps at sa) has 6 - s points; 5 - s
// steps at sb take it to o[5 - s].  sa = 0, sb = 1 returns p bit for bit (1 * x + 0 * y).
__device__ __forceinline__ void bez_restrict(const double (&p)[6], double sa, double sb, double (&o)[6]) {
  const double ua = 1 - sa, ub = 1 - sb;
  double r[6];
#pragma unroll
  for (int m = 0; m < 6; m++) r[m] = p[m];
#pragma unroll
  for (int s = 0; s <= 5; s++) {
    double t[6];
#pragma unroll
    for (int m = 0; m <= 5 - s; m++) t[m] = r[m];
#pragma unroll
    for (int k = 5 - s; k > 0; k--)
#pragma unroll
      for (int m = 0; m < k; m++) t[m] = ub * t[m] + sb * t[m + 1];
    o[5 - s] = t[0];
#pragma unroll
    for (int m = 0; m < 5 - s; m++) r[m] = ua * r[m] + sa * r[m + 1];
  }
}

// the same for a net of N points (degree N - 1: the derivative nets of tj_peak_dynamics, N = 5, 4, 3): o[i] = blossom(sa x (N - 1 - i), sb x i), the steps and their order as
// above (N = 6 gives bez_restrict's bits); sa = 0, sb = 1 returns p bit for bit
template <int N>
__device__ __forceinline__ void bez_restrict_n(const double (&p)[N], double sa, double sb, double (&o)[N]) {
  const double ua = 1 - sa, ub = 1 - sb;
  double r[N];
#pragma unroll
  for (int m = 0; m < N; m++) r[m] = p[m];
#pragma unroll
  for (int s = 0; s < N; s++) {
    double t[N];
#pragma unroll
    for (int m = 0; m < N - s; m++) t[m] = r[m];
#pragma unroll
    for (int k = N - 1 - s; k > 0; k--)
#pragma unroll
      for (int m = 0; m < k; m++) t[m] = ub * t[m] + sb * t[m + 1];
    o[N - 1 - s] = t[0];
#pragma unroll
    for (int m = 0; m < N - 1 - s; m++) r[m] = ua * r[m] + sa * r[m + 1];
  }
}

// segment tr of `net` (hull_entry's sums) restricted to [sa, sb] into a column of stride ST; [0, 1] returns the raw hull bit for bit.  __restrict__: col is a
// lane's column of an LDS tile and never the net.  A caller that holds the column in a struct hides that from the compiler, which then reloads the control points
// and the basis behind every axis's stores (165 global loads per pair of hulls instead of 57: a fifth of tj_path_crossings' time where every pair crosses).
template <int ST>
__device__ __forceinline__ void hull_restrict(const Dev& D, const double* __restrict__ net, int tr, double sa, double sb, double* __restrict__ col) {
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
struct QBest {
  double hi, x; int seg, id;
  __device__ __forceinline__ QBest shuffled(int off) const { return QBest{__shfl_xor(hi, off), __shfl_xor(x, off), __shfl_xor(seg, off), __shfl_xor(id, off)}; }
};
__device__ __forceinline__ bool before(const QBest& a, const QBest& b) {
  if (a.hi != b.hi) return a.hi < b.hi;
  if (a.seg != b.seg) return a.seg < b.seg;
  if (a.id != b.id) return a.id < b.id;
  return a.x < b.x;
}
// the first in the record's total order over the wave (a record states its fields once, in shuffled)
template <class Best>
__device__ __forceinline__ void wave_best(Best& m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const Best o = m.shuffled(off);
    if (before(o, m)) m = o;
  }
}

// The LDS words of one workgroup's reductions, for the round and for a kernel's own seed passes.  A reduction is two halves around a barrier of the caller's: put_* (wave
// reduction, lane 0 stores) and the read (every thread folds the waves' words; a second barrier before the words are written again).  `ev` counts evaluated windows:
// integer adds from init() on, final behind any barrier that follows the last count().  TERM: the search has terminal items (one more word per wave).
template <int NW, bool TERM> struct BnbTermWords { int wterm[NW]; };
template <int NW> struct BnbTermWords<NW, false> {};
template <class Best, int THREADS, bool TERM>
struct BnbShared : BnbTermWords<THREADS / 64, TERM> {
  static constexpr int NW = THREADS / 64;
  Best wbest[NW];
  double wlo[NW];
  int kept, ev;
  __device__ __forceinline__ void init() { if (threadIdx.x == 0) { kept = 0; ev = 0; } __syncthreads(); }
  __device__ __forceinline__ void put_best(Best& m) { wave_best(m); if (lane_id() == 0) wbest[threadIdx.x >> 6] = m; }
  __device__ __forceinline__ Best best(Best m) const { for (int k = 0; k < NW; k++) if (before(wbest[k], m)) m = wbest[k]; return m; }
  __device__ __forceinline__ void put_lo(double& m) { m = wave_min(m); if (lane_id() == 0) wlo[threadIdx.x >> 6] = m; }
  __device__ __forceinline__ double lo(double m) const { for (int k = 0; k < NW; k++) m = fmin(m, wlo[k]); return m; }
  __device__ __forceinline__ void count(int k) { atomicAdd(&ev, k); }
};

// pass 2 of a round keeps an item: one integer atomic on the workgroup's LDS counter, stored while the list has room (the counter goes on: more than maxw = truncated)
template <class Item>
__device__ __forceinline__ void bnb_keep(int& kept, Item* nxt, int maxw, const Item& item) {
  const int at = atomicAdd(&kept, 1);
  if (at < maxw) nxt[at] = item;
}

// ALL ROUNDS of one branch and bound by a workgroup of THREADS threads, from the committed record (best, lo_u, n live items in cur, not truncated) to the one the
// search ends on; the children evaluated are added to sh.ev, which a kernel reads once, for its record, behind the rounds.
// cur / nxt: ping-pong lists of maxw items, klo: the children's lo (ARITY * maxw).  One round:
//   pass 1   lanes take the children strided (i = ARITY * item + child): lo to klo[i], the attained candidates into the lane's best; a total-order reduction gives the
//            round's best.  The children evaluated go to sh.ev: ARITY * n at once where nothing can be terminal, else one integer add per evaluated child
//   pass 2   the same children again: those with lo < best.hi -- the round's FINAL best, so the set does not depend on the order of evaluation -- are appended to nxt
//            (bnb_keep), reducing min lo and "every kept item is terminal"
//   end      more than maxw kept: TRUNCATED, the committed record stands (`windows` counts the overflowing round's work too); else commit and swap the lists
// stop: hi - lo <= tol | nothing live | every live item terminal | max_depth | truncated.  Every thread holds the same values on entry and on return.
// The Search states what differs:
//   Item, Best (ordered by before), ARITY, TERMINAL (can an item be unsplittable)
//   none()                 the Best of "nothing found"
//   terminal(w)            TERMINAL only: w cannot be split; it stays in the set with its lo, and nothing of it is evaluated
//   eval(w, c, mine)       lo of child c of w; folds the child's attained candidates into mine
//   child(w, c, lo)        child c of w as an Item (TERMINAL, terminal(w): w itself, marked)
template <int THREADS, class Search, class Shared>
__device__ __forceinline__ void bnb_rounds(const Search& s, Shared& sh, double tol, int max_depth, int maxw, typename Search::Item* cur, typename Search::Item* nxt, double* klo,
                                           typename Search::Best& best, double& lo_u, int& n, int& depth, bool& truncated) {
  using Item = typename Search::Item;
  using Best = typename Search::Best;
  constexpr int ARITY = Search::ARITY;
  const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  bool terminal = false;   // every live item is
  while (!truncated && !(best.hi - lo_u <= tol) && n > 0 && !terminal && depth < max_depth) {
    // ---- pass 1: the children, one per lane ----
    Best mine = s.none();
    for (int i = tid; i < ARITY * n; i += THREADS) {
      const Item w = cur[(unsigned)i / ARITY];
      const int c = (unsigned)i % ARITY;
      if constexpr (Search::TERMINAL) { if (s.terminal(w)) { klo[i] = c ? INFINITY : w.lo; continue; } sh.count(1); }
      klo[i] = s.eval(w, c, mine);
    }
    sh.put_best(mine);
    if (tid == 0) { sh.kept = 0; if constexpr (!Search::TERMINAL) sh.count(ARITY * n); }   // (nothing terminal: every child was evaluated)
    __syncthreads();   // (also: every klo of the round is written)
    const Best cand = sh.best(best);
    // ---- pass 2: keep what can still hold something below the round's best ----
    double mlo = INFINITY; int allterm = 1;
    for (int i = tid; i < ARITY * n; i += THREADS) {
      const double lo = klo[i];
      if constexpr (!Search::TERMINAL) if (!(lo < cand.hi)) continue;   // (the item is loaded for kept children only)
      const Item w = cur[(unsigned)i / ARITY];
      const int c = (unsigned)i % ARITY;
      if constexpr (Search::TERMINAL) {   // (the item's few words are loaded beside lo: a round of the timed search is latency)
        if (!(lo < cand.hi)) continue;    // (the second child of a terminal item has lo = INFINITY)
        allterm &= s.terminal(w) ? 1 : 0;
      }
      mlo = fmin(mlo, lo);
      bnb_keep(sh.kept, nxt, maxw, s.child(w, c, lo));
    }
    sh.put_lo(mlo);
    if constexpr (Search::TERMINAL) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) allterm &= __shfl_xor(allterm, off);
      if (lane == 0) sh.wterm[wave] = allterm;
    }
    __syncthreads();   // (also: the new list is written, `kept` is final)
    const int m = sh.kept;
    mlo = sh.lo(mlo);
    if constexpr (Search::TERMINAL) for (int k = 0; k < Shared::NW; k++) allterm &= sh.wterm[k];
    __syncthreads();   // everyone has read the round's words before the next round writes them
    if (m > maxw) { truncated = true; break; }
    best = cand; lo_u = fmin(best.hi, mlo); n = m; terminal = Search::TERMINAL && m > 0 && allterm; depth++;
    Item* t = cur; cur = nxt; nxt = t;
  }
}

// the four flag bits every branch-and-bound record has (the five headers' values agree); a query's own cases and bits stay at its call
constexpr int BNB_CONTACT = 1, BNB_CLEAR = 2, BNB_CONVERGED = 4, BNB_TRUNCATED = 8;
static_assert(TJ_CLOSEST_CONTACT == BNB_CONTACT && TJ_PAIR_CONTACT == BNB_CONTACT && TJ_OBSTACLE_CONTACT == BNB_CONTACT && TJ_CROSSING_CONTACT == BNB_CONTACT && TJ_MARGIN_CONTACT == BNB_CONTACT, "CONTACT");
static_assert(TJ_CLOSEST_CLEAR == BNB_CLEAR && TJ_PAIR_CLEAR == BNB_CLEAR && TJ_OBSTACLE_CLEAR == BNB_CLEAR && TJ_CROSSING_CLEAR == BNB_CLEAR && TJ_MARGIN_CLEAR == BNB_CLEAR, "CLEAR");
static_assert(TJ_CLOSEST_CONVERGED == BNB_CONVERGED && TJ_PAIR_CONVERGED == BNB_CONVERGED && TJ_OBSTACLE_CONVERGED == BNB_CONVERGED && TJ_CROSSING_CONVERGED == BNB_CONVERGED && TJ_MARGIN_CONVERGED == BNB_CONVERGED, "CONVERGED");
static_assert(TJ_CLOSEST_TRUNCATED == BNB_TRUNCATED && TJ_PAIR_TRUNCATED == BNB_TRUNCATED && TJ_OBSTACLE_TRUNCATED == BNB_TRUNCATED && TJ_CROSSING_TRUNCATED == BNB_TRUNCATED && TJ_MARGIN_TRUNCATED == BNB_TRUNCATED, "TRUNCATED");
__device__ __forceinline__ int bnb_flags(bool found, double hi, double lo, double tol, int n, bool truncated, double offset) {
  return (found && hi <= offset ? BNB_CONTACT : 0) | (lo > offset ? BNB_CLEAR : 0) | (hi - lo <= tol || (n == 0 && !truncated) ? BNB_CONVERGED : 0) | (truncated ? BNB_TRUNCATED : 0);
}

// ---- the merge half of the window queries (kernels_proximity.h, kernels_obstacle_windows.h, kernels_sight_windows.h, kernels_dynamics_windows.h, kernels_zone_windows.h): all classify windows against a level, keep leaves, sort them, merge adjacent
// leaves into chains and write a row per chain.  How a window is evaluated, the round loop, what a leaf's times are and where a chain goes on stay with each query. ----
constexpr int WIN_OUT = 0, WIN_IN = 1, WIN_MIXED = 2;   // a window's class against the level
constexpr int WIN_CERTAIN = 1, WIN_UNCERTAIN = 2, WIN_AT_START = 4, WIN_AT_END = 8, WIN_RESOLVED = 16, WIN_TRUNCATED = 32;   // a row's flag bits (the two headers' values agree)
static_assert(TJ_PROXIMITY_CERTAIN == WIN_CERTAIN && TJ_OBSWIN_CERTAIN == WIN_CERTAIN && TJ_PROXIMITY_UNCERTAIN == WIN_UNCERTAIN && TJ_OBSWIN_UNCERTAIN == WIN_UNCERTAIN, "CERTAIN, UNCERTAIN");
static_assert(TJ_PROXIMITY_AT_START == WIN_AT_START && TJ_OBSWIN_AT_START == WIN_AT_START && TJ_PROXIMITY_AT_END == WIN_AT_END && TJ_OBSWIN_AT_END == WIN_AT_END, "AT_START, AT_END");
static_assert(TJ_PROXIMITY_RESOLVED == WIN_RESOLVED && TJ_OBSWIN_RESOLVED == WIN_RESOLVED && TJ_PROXIMITY_TRUNCATED == WIN_TRUNCATED && TJ_OBSWIN_TRUNCATED == WIN_TRUNCATED, "RESOLVED, TRUNCATED");
static_assert(TJ_SIGHT_CERTAIN == WIN_CERTAIN && TJ_SIGHT_UNCERTAIN == WIN_UNCERTAIN && TJ_SIGHT_AT_START == WIN_AT_START && TJ_SIGHT_AT_END == WIN_AT_END && TJ_SIGHT_RESOLVED == WIN_RESOLVED && TJ_SIGHT_TRUNCATED == WIN_TRUNCATED, "tj_sight_windows' flags");
static_assert(TJ_DYNWIN_CERTAIN == WIN_CERTAIN && TJ_DYNWIN_UNCERTAIN == WIN_UNCERTAIN && TJ_DYNWIN_AT_START == WIN_AT_START && TJ_DYNWIN_AT_END == WIN_AT_END && TJ_DYNWIN_RESOLVED == WIN_RESOLVED && TJ_DYNWIN_TRUNCATED == WIN_TRUNCATED, "tj_dynamics_windows' flags");
static_assert(TJ_ZONEWIN_CERTAIN == WIN_CERTAIN && TJ_ZONEWIN_UNCERTAIN == WIN_UNCERTAIN && TJ_ZONEWIN_AT_START == WIN_AT_START && TJ_ZONEWIN_AT_END == WIN_AT_END && TJ_ZONEWIN_RESOLVED == WIN_RESOLVED && TJ_ZONEWIN_TRUNCATED == WIN_TRUNCATED, "tj_zone_windows' flags");

// is leaf i of m sorted leaves a chain head: it does not begin (member A) where the leaf before it ends (member B).  first: what the caller knows of leaf 0
template <auto A, auto B, class Leaf>
__device__ __forceinline__ bool win_head(const Leaf* sorted, int i, int m, bool first) { return i < m && (i == 0 ? first : sorted[i - 1].*B != sorted[i].*A); }
// one wave: leaf[0..m) by the start key A into sorted (rank sort: the keys are distinct, so a leaf's rank is the number of smaller keys and the order of the appends vanishes
// here), behind a barrier; returns the chain heads BEHIND leaf 0, in every lane (whether leaf 0 starts a chain is the caller's to say)
template <auto A, auto B, class Leaf>
__device__ __forceinline__ int win_sort(const Leaf* leaf, Leaf* sorted, int m) {
  const int lane = lane_id();
  for (int i = lane; i < m; i += 64) {
    const Leaf x = leaf[i];
    int rank = 0;
    for (int k = 0; k < m; k++) rank += leaf[k].*A < x.*A ? 1 : 0;
    sorted[rank] = x;
  }
  __syncthreads();
  int heads = 0;
  for (int i = 1 + lane; i < m; i += 64) heads += win_head<A, B>(sorted, i, m, false) ? 1 : 0;
  return wave_sum(heads);
}

// one wave: the rows of the slots before `slot` (counts[stride * k]: slot k's row count), in every lane
__device__ __forceinline__ int win_rows_before(const int* counts, int stride, int slot) {
  int off = 0;
  for (int k = lane_id(); k < slot; k += 64) off += counts[stride * k];
  return wave_sum(off);
}
// one step over a block of 64 leaves, every lane of the wave: a head's row index is base + the heads in the lanes below it; base moves behind the block's heads
__device__ __forceinline__ int win_row_index(bool head, int& base) {
  const unsigned long long mask = ballot(head);
  const int r = base + prefix_count(mask);
  base += __popcll(mask);
  return r;
}

// The fold of one chain, leaf after leaf in time order, into what a row of either query states.  A leaf is its times [ta, tb], its width in time, IN or not, and the
// separations attained at its ends (h0, h5) with the ids they were found against.  closest: the smallest of them in the total order (value, time, id); a row without an id
// leaves i0 / i5 at INT_MAX, where no id is ever smaller, so its ties end at the time.
struct WinChain {
  double first_hi = -1.0, last_lo = -1.0, within = 0.0, best = INFINITY, best_t = INFINITY; int best_i = INT_MAX; bool sure = false;
  __device__ __forceinline__ void add(double dist, double ta, double tb, double width, bool in, double h0, double h5, int i0 = INT_MAX, int i5 = INT_MAX) {
    const bool s0 = in || h0 <= dist, s5 = in || h5 <= dist;
    if (!sure && (s0 || s5)) { first_hi = s0 ? ta : tb; sure = true; }
    if (s0) last_lo = ta;
    if (s5) last_lo = tb;
    if (in) within += width;   // (summed in time order)
    if (h0 < best || (h0 == best && (ta < best_t || (ta == best_t && i0 < best_i)))) { best = h0; best_t = ta; best_i = i0; }
    if (h5 < best || (h5 == best && (tb < best_t || (tb == best_t && i5 < best_i)))) { best = h5; best_t = tb; best_i = i5; }
  }
  // the row's common fields and its flags, for a chain from t_first_lo to t_last_hi; closest_time and what else a query's row has stay at its call
  template <class Row>
  __device__ __forceinline__ void finish(Row& row, double t_first_lo, double t_last_hi, bool at_start, bool at_end, bool truncated, double tol) const {
    row.t_first_lo = t_first_lo; row.t_first_hi = first_hi; row.t_last_lo = last_lo; row.t_last_hi = t_last_hi; row.within_lo = within; row.closest = best;
    int flags = (sure ? WIN_CERTAIN : WIN_UNCERTAIN) | (at_start ? WIN_AT_START : 0) | (at_end ? WIN_AT_END : 0) | (truncated ? WIN_TRUNCATED : 0);
    if (sure && (at_start || first_hi - t_first_lo <= tol) && (at_end || t_last_hi - last_lo <= tol)) flags |= WIN_RESOLVED;
    row.flags = flags;
  }
};

// what WinChain::finish states of a row whose own fields are named otherwise (finish writes a member called `closest`: sigma * closest is such a row's `extreme`)
struct WinRowFold {
  double t_first_lo, t_first_hi, t_last_lo, t_last_hi, within_lo, closest; int flags;
  // into a row of a slot query: the times, the flags, extreme = sigma * closest at the chain's best_t
  template <class Row>
  __device__ __forceinline__ void put(Row& row, double sigma, const WinChain& ch) const {
    row.t_first_lo = t_first_lo; row.t_first_hi = t_first_hi; row.t_last_lo = t_last_lo; row.t_last_hi = t_last_hi; row.within_lo = within_lo;
    row.extreme = sigma * closest; row.extreme_time = ch.best_t; row.flags = flags;
  }
};

// the time of the flight position g = tr + s: ((tr + s) / res) * piece_time, every window query's expression
__device__ __forceinline__ double win_time(double res, double ptu, double g) { return (g / res) * ptu; }

// ---- THE LANE-PER-WINDOW SEARCH of the queries whose evaluation is a few dozen flops (kernels_dynamics_windows.h, kernels_zone_windows.h): one search per slot over the
// whole flight by one wave, the windows spread over the lanes.  A query states its evaluation, its leaf and where its slot's lists are; the seeds, the rounds, the bounded
// appends through LDS counters, a truncated round dropped whole, the EDGE leaves, the sort and the info record are here.
//   Leaf     sa, sb (the window of segment tr), ga, gb = tr + sa, tr + sb (the position on the flight: the sort's and the chain's keys), tr, in, g0, g5 (sigma * the value
//            attained at sa, sb) and what the query adds
//   eval     (tr, sa, sb, Leaf& w) -> WIN_OUT | WIN_IN | WIN_MIXED, and the window with its attained ends, in a lane's registers
//   WinSlotArgs   what the kernels of a slot query are handed whatever the query; a query derives its own from it (its gates, its zones and shapes)
constexpr int WIN_LANES = 64;   // one wave per slot
__device__ __forceinline__ size_t win_live_cap(int S, int maxw) { return (size_t)S + maxw; }
__device__ __forceinline__ size_t win_leaf_cap(int S, int maxw) { return (size_t)S + 2 * (size_t)maxw; }

// the appends of one evaluated window: IN to the kept list, MIXED to the next live list (a counter goes on past its list: that is how a round is found truncated)
template <class Leaf>
__device__ __forceinline__ void win_put(int cls, const Leaf& w, Leaf* leaf, int& s_leaf, int leaf_room, Leaf* nxt, int& s_next, int live_room) {
  if (cls == WIN_IN) { const int at = atomicAdd(&s_leaf, 1); if (at < leaf_room) leaf[at] = w; }
  if (cls == WIN_MIXED) { const int at = atomicAdd(&s_next, 1); if (at < live_room) nxt[at] = w; }
}

// what the kernels of a slot query are handed whatever the query; slot = (owned robot, the query's k-th gate or zone), robot-major
template <class L>
struct WinSlotArgs {
  using Leaf = L;
  const double* net;        // [U][3][T]
  const double* pt;         // [U]
  double tol;
  int max_depth, max_windows;
  int row_cap;              // the caller's rows
  Leaf* list;               // [slots][2][S + max_windows] ping-pong live lists; behind the rounds the slot's leaves by flight position
  Leaf* leaf;               // [slots][S + 2 * max_windows] the kept list, in the order of the appends
  int* info;                // [slots][4] leaves, work, depth (+ 1 << 16: truncated), rows; ONE integer atomicAdd of the rows into n_rows
  int* n_rows;              // [1]
};

// the seed, ALL rounds, the sort and the slot's counts of robot u's slot by one wave (the workgroup); s_*: the workgroup's LDS counters
template <class Leaf, class Eval>
__device__ __forceinline__ void win_lane_search(const Dev& D, const WinSlotArgs<Leaf>& A, size_t slot, int u, int& s_leaf, int& s_next, int& s_work, const Eval& eval) {
  const int S = D.S, maxw = A.max_windows, max_depth = A.max_depth;
  const double res = (double)D.res, ptu = A.pt[u], tol = A.tol;
  Leaf* const list = A.list + slot * 2 * win_live_cap(S, maxw);
  Leaf* const leaf = A.leaf + slot * win_leaf_cap(S, maxw);
  int* const info = A.info + slot * 4;
  const int lane = lane_id();
  const int kept_room = S + maxw;   // the kept leaves of a completed round
  Leaf* cur = list;
  Leaf* nxt = cur + win_live_cap(S, maxw);
  Leaf* const sorted = cur;

  // ---- the seeds: every segment at [0, 1], strided over the lanes (at most S appends: both lists have room) ----
  if (lane == 0) { s_leaf = 0; s_next = 0; s_work = S; }
  __syncthreads();
  for (int tr = lane; tr < S; tr += WIN_LANES) {
    Leaf w;
    const int cls = eval(tr, 0.0, 1.0, w);
    win_put(cls, w, leaf, s_leaf, S, cur, s_next, S);
  }
  __syncthreads();
  int kept = s_leaf, n = s_next, depth = 0;   // (LDS words behind a barrier: the same in every lane)
  bool truncated = false;

  // ---- the rounds: every lane halves its own live windows ----
  while (n > 0 && depth < max_depth) {
    __syncthreads();   // everyone has read the counters before lane 0 writes them
    if (lane == 0) s_next = 0;   // (s_leaf goes on from the committed count)
    __syncthreads();
    for (int i = lane; i < n; i += WIN_LANES) {
      const Leaf w = cur[i];
      if (((w.sb - w.sa) / res) * ptu <= tol) {
        const int at = atomicAdd(&s_leaf, 1);
        if (at < kept_room) { Leaf e = w; e.in = 0; leaf[at] = e; }
        continue;
      }
      atomicAdd(&s_work, 2);
      const double sm = 0.5 * (w.sa + w.sb);
      Leaf k;
      int cls = eval(w.tr, w.sa, sm, k);
      win_put(cls, k, leaf, s_leaf, kept_room, nxt, s_next, maxw);
      cls = eval(w.tr, sm, w.sb, k);
      win_put(cls, k, leaf, s_leaf, kept_room, nxt, s_next, maxw);
    }
    __syncthreads();   // the lists are written, the counters final
    const int k2 = s_leaf, n2 = s_next;
    if (k2 > kept_room || n2 > maxw) { truncated = true; break; }   // the committed lists stand: the appends of this round do not count
    kept = k2; n = n2; depth++;
    Leaf* t = cur; cur = nxt; nxt = t;
  }

  // ---- the live windows of the last completed round become EDGE leaves ----
  __syncthreads();
  for (int i = lane; i < n; i += WIN_LANES) { Leaf e = cur[i]; e.in = 0; leaf[kept + i] = e; }
  const int m = kept + n;   // <= S at depth 0, <= S + 2 * max_windows behind a round
  __syncthreads();

  // ---- by flight position into the live lists' room, which is free now, and the slot's rows ----
  const int heads = win_sort<&Leaf::ga, &Leaf::gb>(leaf, sorted, m);
  if (lane == 0) {
    const int rows = m > 0 ? heads + 1 : 0;
    info[0] = m; info[1] = s_work; info[2] = depth | (truncated ? 1 << 16 : 0); info[3] = rows;
    if (rows) atomicAdd(A.n_rows, rows);
  }
}

// the rows of robot u's slot at their final place: behind the rows of the slots before it, chain after chain in time order, by one wave.  L: sigma * the slot's level,
// what WinChain::add takes as the siblings' dist.  ids(leaf, i0, i5): the two ids a leaf carries (a query without ids leaves them at WinChain::add's INT_MAX);
// write(r, fold, chain, first, last, leaves, depth, windows): the query's own row r from the fold of the chain first..last
template <class Leaf, class Ids, class Write>
__device__ __forceinline__ void win_slot_place(const Dev& D, const WinSlotArgs<Leaf>& A, int slot, int u, double L, const Ids& ids, const Write& write) {
  const int lane = lane_id(), S = D.S;
  int base = win_rows_before(A.info + 3, 4, slot);   // the slot's first row
  const int* info = A.info + (size_t)slot * 4;
  const int m = info[0], windows = info[1], depth = info[2] & 0xffff;
  const bool trunc = (info[2] >> 16) != 0;
  const double tol = A.tol, ptu = A.pt[u], res = (double)D.res;
  const Leaf* sorted = A.list + (size_t)slot * 2 * win_live_cap(S, A.max_windows);
  for (int i0 = 0; i0 < m; i0 += WIN_LANES) {
    const int i = i0 + lane;
    const bool head = win_head<&Leaf::ga, &Leaf::gb>(sorted, i, m, true);
    const int r = win_row_index(head, base);
    if (head && r < A.row_cap) {   // (no lane leaves the block loop early: every lane reaches the next ballot)
      WinChain ch;
      int j = i, leaves = 0;
      Leaf x;
      for (;;) {
        x = sorted[j];
        int k0 = INT_MAX, k5 = INT_MAX;
        ids(x, k0, k5);
        ch.add(L, win_time(res, ptu, x.ga), win_time(res, ptu, x.gb), ((x.sb - x.sa) / res) * ptu, x.in != 0, x.g0, x.g5, k0, k5);
        leaves++;
        if (j + 1 >= m || sorted[j + 1].ga != x.gb) break;
        j++;
      }
      const Leaf first = sorted[i];
      WinRowFold f;
      ch.finish(f, win_time(res, ptu, first.ga), win_time(res, ptu, x.gb), first.ga == 0.0, x.gb == (double)S, trunc, tol);
      write(r, f, ch, first, x, leaves, depth, windows);
    }
  }
}

// ---- THE WAVE-COOPERATIVE QUERIES, whose evaluation walks the BVH and is the whole wave's (kernels_obstacle_windows.h, kernels_sight_windows.h): one 64-thread block per
// unit = (owner, segment) -- the owner a robot or a link -- refines the unit's windows one after the other, lane 0 alone appends, counted in LDS; then one wave per owner
// counts and places the owner's rows, whose chains cross segment boundaries.  A query states its evaluation, its seeds, its keys and its row.
//   Leaf     the key members A, B (the window's ends: the sort's and, within a segment, the chain's keys), h0, h5, i0, i5, in, and what the query adds
//   list     [units][per]: the unit's ping-pong live lists of maxw each at its head; behind the rounds the segment's leaves by key A
//   leaf     [units][per]: the kept list, in the order of the appends
//   info     [units][4]: leaves, work, depth (+ 1 << 16: truncated), chain heads behind the first leaf
//   owner    [owners][2]: rows, work; ONE integer atomicAdd of an owner's rows into n_rows
//   Keys     pos(t, key): the flight position compared ACROSS a segment boundary (within a segment the raw keys are compared); time(t, key), width(t, a, b): what
//            WinChain::add receives of a leaf of segment t

// ALL ROUNDS of one unit behind its seeds, the EDGE leaves, the sort and the unit's info record, by one wave (the workgroup).  kept, n: the seeds' leaves and live windows
// (LDS words read behind a barrier: the same in every lane); truncated: among the seeds alone, no round then.  narrow(w): the window is narrow enough to become an EDGE
// leaf; eval(w, a, b, kid) -> the class of the child [a, b] of w, and kid.  eval contains barriers: every lane reaches every call, and the trip counts of the loop over
// live windows and of the round loop are read from LDS behind a barrier (or loaded from one address by every lane), never taken from a lane's own arithmetic.
template <auto A, auto B, class Leaf, class Narrow, class Eval>
__device__ __forceinline__ void win_wave_rounds(Leaf* cur, Leaf* nxt, Leaf* leaf, int kept, int n, bool truncated, int maxw, int max_depth, int& s_leaf, int& s_next, int& s_work, int* info,
                                                const Narrow& narrow, const Eval& eval) {
  const int lane = lane_id();
  Leaf* const sorted = cur;
  int depth = 0;

  // ---- the rounds ----
  while (!truncated && n > 0 && depth < max_depth) {
    __syncthreads();   // everyone has read the counters before lane 0 writes them
    if (lane == 0) s_next = 0;   // (s_leaf goes on from the committed count)
    for (int i = 0; i < n; i++) {
      const Leaf w = cur[i];   // (one address for the wave)
      if (narrow(w)) {
        if (lane == 0) { const int at = s_leaf++; if (at < maxw) { Leaf e = w; e.in = 0; leaf[at] = e; } }
        continue;
      }
      const double mid = 0.5 * (w.*A + w.*B);
      for (int c = 0; c < 2; c++) {
        Leaf kid;
        const int cls = eval(w, c ? mid : w.*A, c ? w.*B : mid, kid);
        if (lane == 0) {
          s_work++;
          if (cls == WIN_IN) { const int at = s_leaf++; if (at < maxw) leaf[at] = kid; }
          if (cls == WIN_MIXED) { const int at = s_next++; if (at < maxw) nxt[at] = kid; }
        }
      }
    }
    __syncthreads();   // the lists are written, the counters final
    const int k2 = s_leaf, n2 = s_next;
    if (k2 > maxw || n2 > maxw) { truncated = true; break; }   // the committed lists stand: the appends of this round do not count
    kept = k2; n = n2; depth++;
    Leaf* t = cur; cur = nxt; nxt = t;
  }

  // ---- the live windows of the last completed round become EDGE leaves ----
  __syncthreads();
  for (int i = lane; i < n; i += WIN_LANES) { Leaf e = cur[i]; e.in = 0; leaf[kept + i] = e; }
  const int m = kept + n;   // <= 2 * max_windows behind a round; the seeds alone: what the caller's lists hold
  __syncthreads();

  // ---- by key A into the live lists' room, which is free now, and the chain heads behind the first leaf ----
  const int heads = win_sort<A, B>(leaf, sorted, m);
  if (lane == 0) { info[0] = m; info[1] = s_work; info[2] = depth | (truncated ? 1 << 16 : 0); info[3] = heads; }
}

// does the first leaf of segment tr of owner o start a chain (it does not where the last leaf of segment tr - 1 ends where it begins)
template <auto A, auto B, class Leaf, class Keys>
__device__ __forceinline__ bool win_seg_first_is_head(const Leaf* list, const int* info, size_t per, int S, int o, int tr, const Keys& key) {
  if (tr == 0) return true;
  const size_t prev = (size_t)o * S + tr - 1;
  const int mp = info[prev * 4];
  if (mp == 0) return true;
  return key.pos(tr - 1, list[prev * per + mp - 1].*B) != key.pos(tr, list[(prev + 1) * per].*A);
}

// one wave per owner: the chain heads over its segments' leaves in order (a segment's first leaf continues the chain of the segment before it or starts one) = the
// owner's row count, and its work; the counts are added up with one integer atomic per owner
template <auto A, auto B, class Leaf, class Keys>
__device__ __forceinline__ void win_seg_count(const Leaf* list, const int* info, size_t per, int S, int o, int* owner, int* n_rows, const Keys& key) {
  const int lane = lane_id();
  int rows = 0, work = 0;
  for (int tr = lane; tr < S; tr += WIN_LANES) {
    const int* unit = info + ((size_t)o * S + tr) * 4;
    work += unit[1];
    if (unit[0] > 0) rows += unit[3] + (win_seg_first_is_head<A, B>(list, info, per, S, o, tr, key) ? 1 : 0);
  }
  rows = wave_sum(rows); work = wave_sum(work);
  if (lane == 0) {
    owner[2 * o] = rows; owner[2 * o + 1] = work;
    if (rows) atomicAdd(n_rows, rows);
  }
}

// one wave per owner: its rows at their final place, behind the rows of the owners before it, chain after chain in time order.  The chain heads of a block of 64 leaves
// get their row index from win_row_index, and the lane of a head folds its chain left to right (WinChain), across segment boundaries, and writes the row where it
// belongs; rows beyond row_cap are counted, not written.  pos_end: the flight's last position, as key.pos gives it.  The row's common fields and flags, closest_time
// and index (-1 without a sample), leaves, depth and windows are set here; own(row, first segment, last segment) sets what else the query's row has.
template <auto A, auto B, class Leaf, class Keys, class Row, class Own>
__device__ __forceinline__ void win_seg_place(const Leaf* list, const int* info, size_t per, int S, int o, const int* owner, int row_cap, double dist, double tol, double pos_end,
                                              const Keys& key, Row* out, const Own& own) {
  const int lane = lane_id();
  int base = win_rows_before(owner, 2, o);   // the owner's first row
  const int windows = owner[2 * o + 1];
  for (int tr = 0; tr < S; tr++) {
    const size_t unit = (size_t)o * S + tr;
    const int m = info[unit * 4];   // (one address for the wave)
    if (m == 0) continue;
    const Leaf* sorted = list + unit * per;
    const bool first_head = win_seg_first_is_head<A, B>(list, info, per, S, o, tr, key);
    for (int i0 = 0; i0 < m; i0 += WIN_LANES) {
      const int i = i0 + lane;
      const bool head = win_head<A, B>(sorted, i, m, first_head);
      const int r = win_row_index(head, base);
      if (head && r < row_cap) {   // (no lane leaves the block loop early: every lane reaches the next ballot)
        // the chain from leaf i of segment tr on, left to right, into the segments behind where it goes on
        Row row;
        WinChain ch;
        double end_g = 0.0, end_t = 0.0;
        int t = tr, k = i, mt = m, leaves = 0, dmax = 0;
        bool trunc = false;
        const Leaf* sl = sorted;
        for (;;) {
          if (k == 0 || leaves == 0) { const int dt = info[((size_t)o * S + t) * 4 + 2]; dmax = max(dmax, dt & 0xffff); trunc = trunc || (dt >> 16) != 0; }
          const Leaf x = sl[k];
          const double ta = key.time(t, x.*A), tb = key.time(t, x.*B);
          ch.add(dist, ta, tb, key.width(t, x.*A, x.*B), x.in, x.h0, x.h5, x.i0, x.i5);
          end_g = key.pos(t, x.*B); end_t = tb;
          leaves++;
          if (k + 1 < mt) {
            if (sl[k + 1].*A != x.*B) break;   // (within a segment: the raw keys)
            k++;
          } else {
            if (t + 1 >= S) break;
            const int m2 = info[((size_t)o * S + t + 1) * 4];
            if (m2 == 0) break;
            const Leaf* s2 = list + ((size_t)o * S + t + 1) * per;
            if (end_g != key.pos(t + 1, s2[0].*A)) break;
            t++; k = 0; mt = m2; sl = s2;
          }
        }
        const bool found = ch.best_i != INT_MAX;
        ch.finish(row, key.time(tr, sorted[i].*A), end_t, key.pos(tr, sorted[i].*A) == 0.0, end_g == pos_end, trunc, tol);
        row.closest_time = found ? ch.best_t : -1.0;
        row.index = found ? ch.best_i : -1;
        row.leaves = leaves; row.depth = dmax; row.windows = windows;
        own(row, tr, t);
        out[r] = row;
      }
    }
  }
}

}  // namespace tj
