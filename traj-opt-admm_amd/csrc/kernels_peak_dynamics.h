// kernels_peak_dynamics.h -- tj_peak_dynamics: the FLOWN CURVE's peak speed, acceleration and jerk with their times, its path length, and the factor its timetable could
// be scaled by.
//
// tj_audit's speed / accel are maxima over the control vectors of each segment's derivative nets (hull_speed / hull_accel): what bound_energy constrains, an upper bound on
// what the vehicle does, without a time.  Here that bound drives a MAXIMISING branch and bound over dyadic windows of one segment's parameter -- the shape of bnb_rounds
// (dev_query.h), which minimises with an absolute tolerance and stays as it is.  The definition (include/trajadmm.h), per owned robot u and quantity (degree n = 4, 3, 2):
//   net      the raw derivative net of segment tr from the raw hull P (hull_entry's sums), in hull_speed's / hull_accel's expressions (peak_raw), restricted to the window
//            by bez_restrict_n -- always from the RAW net, never a parent's: rounding does not grow with depth; [0, 1] returns the raw net bit for bit
//   bounds   ub(W) = max_i norm3(c_i) / den, at(W) = the larger of norm3(c_0) / den (at sa) and norm3(c_n) / den (at sb; a tie: sa); den = w pt | w w pt pt |
//            w w w pt pt pt, left to right (tj_audit's association: depth 0 gives its bits)
//   order    of attained candidates: larger value, then smaller segment, then smaller s (PeakBest): total, so nothing depends on the order of evaluation
//   seeds    every segment at [0, 1]; best = the first candidate; live = {ub > best.v}
//   round d  every live item is halved at 0.5 * (sa + sb); both children are evaluated; best over (best, children); live = children with ub > best.v -- the round's
//            FINAL best
//   bracket  lo = best.v, hi = max(best.v, max ub over live)
//   stop     hi - lo <= tol * hi | live empty | d == max_depth | more than max_windows live (TRUNCATED: the record of the last completed round, at seeding the seeds')
//   length   per segment the 2^L windows of the raw v net: len_lo = h * norm3((c_0 + .. + c_4) / 5) (the chord: a net's mean is its integral), len_hi =
//            (h * (|c_0| + .. + |c_4|)) / 5 (the control polygon), sums left to right; a segment's windows in the balanced binary tree over adjacent pairs, the segments
//            one after the other
//
// TWO launches whatever the fleet's size, the piece count and the depth:
//   k_peak_dynamics   grid (owned robots, 4), ONE wave per block: blocks y = 0..2 run ALL rounds of the search for speed, acceleration and jerk (lanes take the children
//                     strided; ping-pong lists in global memory; reductions by shuffles in the total order), block y = 3 the length bracket and the duration.  The four jobs
//                     have different trip counts: with one wave per workgroup every barrier is reached by the whole workgroup, whatever the others do.  Each block writes
//                     its own fields of the record; none waits for another.
//   k_peak_finish     one thread per owned robot: time_scale and the record's flags from the finished speed.hi / accel.hi.
// No float atomics, no polling, nothing of the iteration's scratch.  Read-only: the kernels write the query's own buffers only.
#pragma once
#include "dev_query.h"

namespace tj {

static_assert(sizeof(tj_peak) == 40 && sizeof(tj_dynamics_robot) == 160, "the records' layout (include/trajadmm.h)");
static_assert(TJ_PEAK_CONVERGED == BNB_CONVERGED && TJ_PEAK_TRUNCATED == BNB_TRUNCATED, "the per-peak flags are the branch-and-bound queries'");

struct PeakItem { double sa, sb; int tr, pad; };   // window [sa, sb] of segment tr

// the best attained value: v at parameter s of segment seg.  Nothing yet: {-INFINITY, 0, INT_MAX}.  The order is total: larger value, smaller segment, smaller s.
struct PeakBest {
  double v, s; int seg;
  __device__ __forceinline__ PeakBest shuffled(int off) const { return PeakBest{__shfl_xor(v, off), __shfl_xor(s, off), __shfl_xor(seg, off)}; }
};
__device__ __forceinline__ bool before(const PeakBest& a, const PeakBest& b) {
  if (a.v != b.v) return a.v > b.v;
  if (a.seg != b.seg) return a.seg < b.seg;
  return a.s < b.s;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}
// every lane's value summed in the balanced binary tree over adjacent lanes (lane 2k + lane 2k + 1, then pairs of those, ...): every lane ends with the same bits
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off);
  return v;
}

struct PeakArgs {
  const double* net;     // [U][3][T]
  const double* pt;      // [U]
  double tol;
  int max_depth, max_windows, levels, cap, kw;
  PeakItem* list;        // [owned][3][2][cap] ping-pong live lists
  double* kub;           // [owned][3][kw] ub of the seeds / of the round's children (kw >= 2 * cap and >= S)
};

// one axis of the raw derivative net of degree DEG from the raw hull's axis P[0..5]: hull_speed's and hull_accel's expressions, and the third difference
template <int DEG>
__device__ __forceinline__ void peak_raw(const double (&P)[6], double (&c)[DEG + 1]) {
#pragma unroll
  for (int i = 0; i <= DEG; i++) {
    if constexpr (DEG == 4) c[i] = 5 * (P[i + 1] - P[i]);
    else if constexpr (DEG == 3) c[i] = 20 * (P[i + 2] - 2 * P[i + 1] + P[i]);
    else c[i] = 60 * (P[i + 3] - 3 * P[i + 2] + 3 * P[i + 1] - P[i]);
  }
}
template <int DEG>
__device__ __forceinline__ double peak_den(double w, double pt) {
  if constexpr (DEG == 4) return w * pt;
  else if constexpr (DEG == 3) return w * w * pt * pt;
  else return w * w * w * pt * pt * pt;
}
// the derivative net of segment tr restricted to [sa, sb], per axis
template <int DEG>
__device__ __forceinline__ void peak_net(const Dev& D, const double* __restrict__ nu, int tr, double sa, double sb, double (&o)[3][DEG + 1]) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double a[6], c[DEG + 1];
#pragma unroll
    for (int i = 0; i < 6; i++) a[i] = hull_entry(D, nu, tr, i, k);
    peak_raw<DEG>(a, c);
    bez_restrict_n<DEG + 1>(c, sa, sb, o[k]);
  }
}
// ub of window [sa, sb] of segment tr; its attained candidate is folded into mine
template <int DEG>
__device__ __forceinline__ double peak_eval(const Dev& D, const double* __restrict__ nu, double ptu, int tr, double sa, double sb, PeakBest& mine) {
  double o[3][DEG + 1], v[DEG + 1];
  peak_net<DEG>(D, nu, tr, sa, sb, o);
  const double den = peak_den<DEG>(seg_weight(D, tr), ptu);
  double ub = -INFINITY;
#pragma unroll
  for (int i = 0; i <= DEG; i++) { v[i] = norm3(o[0][i], o[1][i], o[2][i]) / den; ub = fmax(ub, v[i]); }
  const bool first = v[0] >= v[DEG];
  const PeakBest b{first ? v[0] : v[DEG], first ? sa : sb, tr};
  if (before(b, mine)) mine = b;
  return ub;
}

// ALL rounds of one quantity's search by one wave (the workgroup); kept: the workgroup's LDS counter of bnb_keep
template <int DEG>
__device__ void peak_search(const Dev& D, const PeakArgs& A, int ui, int u, int q, int& kept, tj_peak* out) {
  const int lane = lane_id(), S = D.S, maxw = A.max_windows;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double ptu = A.pt[u];
  PeakItem* cur = A.list + ((size_t)ui * 3 + q) * 2 * A.cap;
  PeakItem* nxt = cur + A.cap;
  double* kub = A.kub + ((size_t)ui * 3 + q) * A.kw;
  const PeakBest none{-INFINITY, 0.0, INT_MAX};

  // ---- seeds: every segment at [0, 1] (pass 1: ub and the best; pass 2: keep against the final best) ----
  PeakBest best = none;
  for (int tr = lane; tr < S; tr += 64) kub[tr] = peak_eval<DEG>(D, nu, ptu, tr, 0.0, 1.0, best);
  wave_best(best);
  if (lane == 0) kept = 0;
  __syncthreads();
  double mub = -INFINITY;
  for (int tr = lane; tr < S; tr += 64) {
    const double ub = kub[tr];   // (this lane's own store)
    if (!(ub > best.v)) continue;
    mub = fmax(mub, ub);
    bnb_keep(kept, cur, maxw, PeakItem{0.0, 1.0, tr, 0});
  }
  mub = wave_max(mub);
  __syncthreads();   // the list is written, `kept` is final
  int n = kept;
  __syncthreads();   // everyone has read it before the next round resets it
  double hi = fmax(best.v, mub);
  int depth = 0, windows = S;
  bool truncated = n > maxw;

  while (!truncated && !(hi - best.v <= A.tol * hi) && n > 0 && depth < A.max_depth) {
    // ---- pass 1: the children, strided over the lanes ----
    PeakBest mine = none;
    for (int i = lane; i < 2 * n; i += 64) {
      const PeakItem w = cur[i >> 1];
      const double sm = 0.5 * (w.sa + w.sb);
      kub[i] = peak_eval<DEG>(D, nu, ptu, w.tr, (i & 1) ? sm : w.sa, (i & 1) ? w.sb : sm, mine);
    }
    wave_best(mine);
    const PeakBest cand = before(mine, best) ? mine : best;
    if (lane == 0) kept = 0;
    __syncthreads();
    windows += 2 * n;
    // ---- pass 2: keep what can still hold something above the round's best ----
    mub = -INFINITY;
    for (int i = lane; i < 2 * n; i += 64) {
      const double ub = kub[i];   // (this lane's own store)
      if (!(ub > cand.v)) continue;
      const PeakItem w = cur[i >> 1];
      const double sm = 0.5 * (w.sa + w.sb);
      mub = fmax(mub, ub);
      bnb_keep(kept, nxt, maxw, PeakItem{(i & 1) ? sm : w.sa, (i & 1) ? w.sb : sm, w.tr, 0});
    }
    mub = wave_max(mub);
    __syncthreads();   // the new list is written, `kept` is final
    const int m = kept;
    __syncthreads();
    if (m > maxw) { truncated = true; break; }   // the committed record stands; `windows` counts this round's work too
    best = cand; hi = fmax(best.v, mub); n = m; depth++;
    PeakItem* t = cur; cur = nxt; nxt = t;
  }
  if (lane == 0) {
    tj_peak r;
    r.lo = best.v; r.hi = hi; r.time = ((best.seg + best.s) / (double)D.res) * ptu;   // tj_obstacle_approach's expression
    r.segment = best.seg; r.depth = depth; r.windows = windows;
    r.flags = (hi - best.v <= A.tol * hi || (n == 0 && !truncated) ? BNB_CONVERGED : 0) | (truncated ? BNB_TRUNCATED : 0);
    *out = r;
  }
}

// the length bracket of robot u by one wave: lanes take a segment's windows strided, 64 adjacent windows are one subtree (wave_tree_sum), the subtrees' sums go to lane
// (window / 64) and are summed by the same tree: the balanced tree over 2^L windows, for 2^L below and above 64 (lanes without a window hold 0: x + 0 is x)
__device__ void peak_length(const Dev& D, const PeakArgs& A, int u, double& len_lo, double& len_hi) {
  const int lane = lane_id(), S = D.S, nwin = 1 << A.levels;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double h = 1.0 / nwin;
  double lo = 0.0, hi = 0.0;
  for (int tr = 0; tr < S; tr++) {
    double raw[3][5];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double a[6];
#pragma unroll
      for (int i = 0; i < 6; i++) a[i] = hull_entry(D, nu, tr, i, k);
      peak_raw<4>(a, raw[k]);
    }
    double slo = 0.0, shi = 0.0;
    for (int base = 0; base < nwin; base += 64) {
      const int j = base + lane;
      double wl = 0.0, wh = 0.0;
      if (j < nwin) {
        const double sa = j * h, sb = (j + 1) * h;
        double c[3][5], m[3], sum = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          bez_restrict_n<5>(raw[k], sa, sb, c[k]);
          m[k] = (c[k][0] + c[k][1] + c[k][2] + c[k][3] + c[k][4]) / 5;
        }
#pragma unroll
        for (int i = 0; i < 5; i++) sum = i ? sum + norm3(c[0][i], c[1][i], c[2][i]) : norm3(c[0][0], c[1][0], c[2][0]);
        wl = h * norm3(m[0], m[1], m[2]);
        wh = (h * sum) / 5;
      }
      wl = wave_tree_sum(wl); wh = wave_tree_sum(wh);
      if (lane == (base >> 6)) { slo = wl; shi = wh; }
    }
    lo += wave_tree_sum(slo); hi += wave_tree_sum(shi);
  }
  len_lo = lo; len_hi = hi;
}

__global__ __launch_bounds__(64) void k_peak_dynamics(Dev D, PeakArgs A, tj_dynamics_robot* out) {
  const int ui = blockIdx.x, u = D.u0 + ui, q = blockIdx.y;   // (q is the block's: every branch below is taken by the whole workgroup)
  __shared__ int kept;
  if (q == 0) peak_search<4>(D, A, ui, u, 0, kept, &out[u].speed);
  else if (q == 1) peak_search<3>(D, A, ui, u, 1, kept, &out[u].accel);
  else if (q == 2) peak_search<2>(D, A, ui, u, 2, kept, &out[u].jerk);
  else {
    double lo, hi;
    peak_length(D, A, u, lo, hi);
    if (lane_id() == 0) {
      const double pt = A.pt[u];
      double dur = 0;
      for (int i = 0; i < D.P; i++) dur += 1.0 * pt;   // tj_audit's sum: piece_num * piece_time
      out[u].length_lo = lo; out[u].length_hi = hi; out[u].duration = dur; out[u].length_levels = A.levels;
    }
  }
}

// behind k_peak_dynamics: what needs two of its blocks' results
__global__ __launch_bounds__(64) void k_peak_finish(Dev D, tj_dynamics_robot* out) {
  const int ui = blockIdx.x * 64 + threadIdx.x;
  if (ui >= D.u1 - D.u0) return;
  tj_dynamics_robot& r = out[D.u0 + ui];
  const double sp_lo = r.speed.lo, sp_hi = r.speed.hi, ac_lo = r.accel.lo, ac_hi = r.accel.hi;
  r.time_scale = fmax(sp_hi / D.vel_limit, sqrt(ac_hi / D.acc_limit));
  r.flags = (sp_lo >= D.vel_limit ? TJ_DYN_SPEED : 0) | (sp_hi < D.vel_limit ? TJ_DYN_SPEED_OK : 0) | (ac_lo >= D.acc_limit ? TJ_DYN_ACCEL : 0) | (ac_hi < D.acc_limit ? TJ_DYN_ACCEL_OK : 0);
}

}  // namespace tj
