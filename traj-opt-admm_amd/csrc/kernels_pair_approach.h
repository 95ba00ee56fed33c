// kernels_pair_approach.h -- tj_pair_approach: the closest approach of EVERY robot pair that comes close at equal flight times, each pair converged on its own.
//
// tj_closest_approach answers per robot: its search prunes every partner's windows against the worst partner's hi, so the other partners' separations are never
// computed.  Here the same windows, the same certified lo, the same attained hi and the same search (TimedSearch, kernels_closest.h, in dev_query.h's round loop) run once per DIRECTED PAIR
// (u, q), u owned: the pair prunes against its own best.  The definition (include/trajadmm.h):
//   seeds(u, q)   the level-0 windows (tr, q, j, ca, cb) k_audit_timed evaluates for u against this q and that pass the box prefilter
//   listed        (u, q) has a row iff a seed has lo < range or hi < range; an unlisted pair is certified at least `range` apart over u's flight
//   search        tj_closest_approach's seeds / round / bracket / stop with the pair's windows; more than max_windows live IN THIS PAIR: TRUNCATED
//   rows          sorted by (robot, partner)
//
// At most four launches whatever the fleet's size, the number of pairs and the depth (a count-only call, cap == 0, ends after the second):
//   k_pair_mark     one wave per (owned robot, segment), timed_walk at level 0 with the certificate (lane = partner of the pass).  A window with lo < range or
//                   hi < range sets the pair's bit in the [owned][words] bitmask with an integer atomic OR.
//   k_pair_index    one workgroup: popcounts of the bitmask's words in (robot, partner) order, one exclusive scan over them.  Pair p is the p-th set bit: this
//                   is where the output order becomes a function of the state alone.  Writes n, the word offsets and (robot, partner) of the slots below cap.
//   k_pair_seed     the walk again (the same source expressions: the same bits).  A window of a listed pair whose slot is below cap is counted in the pair's
//                   `windows`, and, where lo < range or hi < range, appended with its lo, hi and time to the PAIR's seed list (bnb_keep on the pair's counter;
//                   a pair has at most 2 S windows at level 0: S of u's segments, each cut at most once per boundary of q, arrival included).
//   k_pair_refine   one wave per pair slot; slots at or beyond n or cap exit at once.  Round 0 over the pair's seeds: best in the order (hi, segment, partner,
//                   time), then live = {lo < range and lo < best.hi} into the pair's ping-pong slice; then the rounds (bnb_rounds<64>).
// The walk runs twice instead of once with a per-robot seed list (the shape the two-kernel siblings have): which pairs are among the first `cap` is known only
// after the index, a count-only call needs no list at all, and so every buffer is a function of cap and max_windows alone -- nothing scales with U^2 but the bitmask.
// One wave per pair: a pair's live set is a handful of windows (2 at most on the measured states); three 18-row tiles of 64 columns = 27 KB of LDS against
// k_closest_refine's 54 KB, so LDS never limits the waves per CU below what the registers of the per-lane GJK allow.
// Read-only: the kernels write the query's own buffers only (no tj_stats counter, no launch count).  No float atomics, no polling, no workgroup waits on another.
#pragma once
#include "kernels_closest.h"

namespace tj {

constexpr int PA_THREADS = 64;    // one wave per pair
constexpr int PA_INDEX = 256;     // threads of the one indexing workgroup

struct PairSeed { double ca, cb, lo, hi, thi; int tr, j; };   // a level-0 window of a listed pair with lo < range or hi < range: its bracket and the time of its hi sample

// the index of the listed pairs, shared with kernels_path_crossing.h: what k_pair_index reads and writes
struct PairIndex {
  int cap, words;      // the caller's rows; 32-bit words per bitmask row
  unsigned* mask;      // [owned][words] bit q of row u - u0: (u, q) is listed
  int* wordoff;        // [owned][words] listed pairs before this word in (robot, partner) order
  int* n;              // [1] listed pairs
  int* who;            // [cap][2] robot, partner of a slot
};

struct PairArgs {
  const double* net;   // [U][3][T]
  const double* pt;    // [U]
  double range, tol;
  int max_depth, max_windows;
  int seed_cap;        // seeds per pair slot (2 S + 2)
  PairIndex ix;
  int* count;          // [cap][2] seeds appended, windows evaluated
  PairSeed* seeds;     // [cap][seed_cap]
  ClosestWin* list;    // [cap][2][max_windows] ping-pong live lists
  double* klo;         // [cap][2 * max_windows] lo of the round's children
};

__device__ __forceinline__ bool pair_near(double lo, double hi, double range) { return lo < range || hi < range; }

__global__ __launch_bounds__(64) void k_pair_mark(Dev D, PairArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tq[18 * 64], td[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double range = A.range;
  unsigned* row = A.ix.mask + (size_t)ui * A.ix.words;
  timed_walk<true>(D, A.net, A.pt, range, 0, u, tr, P, box, tq + lane, td + lane, [&](int q, int, int, double, double, double lo, double h0, double h5, bool sep) {
    if (!sep) lo = 0.0;
    if (pair_near(lo, h0 <= h5 ? h0 : h5, range)) atomicOr(&row[q >> 5], 1u << (q & 31));
  });
}

// thread t takes the words [t * per, (t + 1) * per) of the bitmask, row after row: their order is the rows' order
__global__ __launch_bounds__(PA_INDEX) void k_pair_index(Dev D, PairIndex A) {
  const int tid = threadIdx.x, total = (D.u1 - D.u0) * A.words, per = (total + PA_INDEX - 1) / PA_INDEX;
  const int w0 = min(tid * per, total), w1 = min(w0 + per, total);
  __shared__ int part[PA_INDEX];
  int sum = 0;
  for (int w = w0; w < w1; w++) sum += __popc(A.mask[w]);
  part[tid] = sum;
  __syncthreads();
  int off = 0;
  for (int k = 0; k < tid; k++) off += part[k];
  if (tid == PA_INDEX - 1) *A.n = off + sum;
  for (int w = w0; w < w1; w++) {
    A.wordoff[w] = off;
    const int ui = w / A.words, q0 = (w - ui * A.words) * 32;
    for (unsigned m = A.mask[w]; m; m &= m - 1, off++)
      if (off < A.cap) { A.who[2 * off] = D.u0 + ui; A.who[2 * off + 1] = q0 + __ffs(m) - 1; }
  }
}

__global__ __launch_bounds__(64) void k_pair_seed(Dev D, PairArgs A) {
  const int lane = lane_id(), S = D.S;
  const int ui = blockIdx.x / S, tr = blockIdx.x - ui * S, u = D.u0 + ui;
  __shared__ double P[18], tq[18 * 64], td[18 * 64];
  QBox box;
  query_hull(D, A.net + (size_t)u * 3 * D.T, tr, P, box);
  const double range = A.range;
  const size_t row = (size_t)ui * A.ix.words;
  timed_walk<true>(D, A.net, A.pt, range, 0, u, tr, P, box, tq + lane, td + lane, [&](int q, int, int j, double ca, double cb, double lo, double h0, double h5, bool sep) {
    const unsigned m = A.ix.mask[row + (q >> 5)], bit = 1u << (q & 31);
    if (!(m & bit)) return;
    const int slot = A.ix.wordoff[row + (q >> 5)] + __popc(m & (bit - 1));
    if (slot >= A.ix.cap) return;
    if (!sep) lo = 0.0;
    atomicAdd(&A.count[2 * slot + 1], 1);
    const bool first = h0 <= h5;
    const double hi = first ? h0 : h5;
    if (pair_near(lo, hi, range)) bnb_keep(A.count[2 * slot], A.seeds + (size_t)slot * A.seed_cap, A.seed_cap, PairSeed{ca, cb, lo, hi, first ? ca : cb, tr, j});
  });
}

__global__ __launch_bounds__(PA_THREADS) void k_pair_refine(Dev D, PairArgs A, tj_pair_record* out) {
  const int p = blockIdx.x, tid = threadIdx.x;
  if (p >= *A.ix.n || p >= A.ix.cap) return;
  __shared__ double tp[18 * PA_THREADS], tq[18 * PA_THREADS], td[18 * PA_THREADS];
  __shared__ TimedSearch<PA_THREADS>::Shared sh;
  const int u = A.ix.who[2 * p], q = A.ix.who[2 * p + 1], maxw = A.max_windows;
  const double range = A.range;
  const PairSeed* seeds = A.seeds + (size_t)p * A.seed_cap;
  const int ns = min(A.count[2 * p], A.seed_cap);
  ClosestWin* cur = A.list + (size_t)p * 2 * maxw;
  sh.init();

  // ---- round 0: the pair's best over its seeds, then its live set against that best (the append's order is free: what follows reduces in a total order) ----
  QBest best{range, 0.0, INT_MAX, INT_MAX};
  for (int i = tid; i < ns; i += PA_THREADS) {
    const PairSeed s = seeds[i];
    const QBest b{s.hi, s.thi, s.tr, q};
    if (b.hi < range && before(b, best)) best = b;
  }
  wave_best(best);   // (one wave: the workgroup's)
  double mlo = INFINITY;
  for (int i = tid; i < ns; i += PA_THREADS) {
    const PairSeed s = seeds[i];
    if (!(s.lo < range && s.lo < best.hi)) continue;
    mlo = fmin(mlo, s.lo);
    bnb_keep(sh.kept, cur, maxw, ClosestWin{s.ca, s.cb, s.lo, s.tr, q, s.j, 0});
  }
  mlo = wave_min(mlo);
  __syncthreads();   // the live list is written, kept is final
  double lo_u = fmin(best.hi, mlo);
  int n = sh.kept, depth = 0;
  bool truncated = n > maxw;
  __syncthreads();   // everyone has read kept before the first round resets it
  bnb_rounds<PA_THREADS>(TimedSearch<PA_THREADS>{D, A.net, A.pt, A.net + (size_t)u * 3 * D.T, A.pt[u], range, tp + tid, tq + tid, td + tid}, sh, A.tol, A.max_depth, maxw,
                         cur, cur + maxw, A.klo + (size_t)p * 2 * maxw, best, lo_u, n, depth, truncated);
  if (tid == 0) {
    tj_pair_record r;
    const bool found = best.id != INT_MAX;
    r.lo = lo_u; r.hi = best.hi; r.time = found ? best.x : -1.0;
    r.robot = u; r.partner = q; r.segment = found ? best.seg : -1;
    r.depth = depth; r.windows = A.count[2 * p + 1] + sh.ev;   // the seeding's windows and the rounds'
    r.flags = bnb_flags(found, best.hi, lo_u, A.tol, n, truncated, D.offset);
    out[p] = r;
  }
}

}  // namespace tj
