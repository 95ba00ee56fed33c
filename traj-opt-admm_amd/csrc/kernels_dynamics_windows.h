// kernels_dynamics_windows.h -- tj_dynamics_windows: WHEN is every robot's flown curve over (or under) a level of speed, acceleration or jerk, as certified time intervals.
//
// tj_peak_dynamics names one peak per robot and quantity; a state that is not yet inside its limits exceeds them over stretches, often several per flight.  This is the
// interval counterpart, the fourth of the window queries (kernels_proximity.h, kernels_obstacle_windows.h, kernels_sight_windows.h): windows of a segment's parameter are
// classified against a level and only what is not certified on the far side is kept.  The derivative nets and their blossoming are kernels_peak_dynamics.h's, unchanged
// (peak_raw, peak_den, peak_net, bez_restrict_n); the search loop, the placing of a slot's rows and the merge half are dev_query.h's (WinSlotArgs, win_lane_search,
// win_slot_place; WIN_*, win_sort, win_head, win_rows_before, win_row_index, WinChain, WinRowFold, win_time).  This file's own: the evaluation (dynwin_eval), the gates and the row.  The definition
// (include/trajadmm.h), per slot = (owned robot u, gate k) with the gate's quantity (degree n = 4, 3, 2), sense and level:
//   net      c_0..c_n = the raw derivative net of segment tr restricted to [sa, sb] (always from the RAW net); a vector counts as norm3(c) / den (peak_den)
//   bounds   ub = max_i norm3(c_i) / den; lb = (min_i dot3(c_i, d) / norm3(d)) / den with d = c_0 + .. + c_n per axis, left to right, where norm3(d) > 0 and the
//            minimum is positive, else 0 (the derivative lies in the net's hull and |x| >= x . d / |d|); h0, h5 = norm3(c_0) / den, norm3(c_n) / den, attained at sa, sb
//   class    ABOVE: OUT ub < level | IN lb >= level | MIXED; BELOW: OUT lb > level | IN ub <= level | MIXED.  With sigma = -1 (ABOVE) / +1 (BELOW), g = sigma * value and
//            L = sigma * level, "within" is g <= L: a leaf carries sigma * h0 / sigma * h5 and WinChain::add takes L as the siblings' dist
//   search   ONE per slot over the whole flight.  Seeds: every segment at [0, 1]: IN to the leaves, MIXED to the live set (never truncated: the lists have room for S).
//            Round: a live window whose time width <= tol becomes an EDGE leaf, every other is halved and both children are evaluated.  Stop: live empty | max_depth |
//            after a round more than max_windows live or more than S + max_windows leaves (TRUNCATED: the lists of the last completed round).  What is live at the
//            end joins the leaves as EDGE leaves.
//   merge    the slot's leaves by flight position tr + sa (exact in a double: 9 + 40 bits); adjacent iff prev.gb == next.ga; a row per maximal chain
//
// An evaluation costs a few dozen flops where the siblings walk a BVH per evaluation, so the WINDOWS are spread over the lanes: every lane halves its own live window
// and evaluates both children in registers.  TWO launches whatever the fleet, the gates and the depth (a count-only call, cap == 0, ends after the first):
//   k_dynwin_refine  grid (owned x n_gates), ONE wave per block, which dispatches on its gate's quantity to a body templated on the degree (the branch is the block's).
//                    Seeds and the live windows of a round are strided over the lanes; appends go to the slot's ping-pong live lists and its kept list in global
//                    memory through LDS integer counters (k_prox_refine's way: the order of the appends vanishes in the rank sort, and a truncated round is dropped
//                    whole).  Behind the rounds win_sort into the live lists' room, which is free then, and the slot's row count (the interior heads + 1 where it
//                    has a leaf), work, depth and truncation bit; ONE integer atomicAdd of the row count into n_rows.
//   k_dynwin_place   one wave per slot (win_slot_place): win_rows_before over the slots before it gives its first row; blocks of 64 leaves through win_head / win_row_index; the lane
//                    of a head folds its chain left to right (WinChain) and writes the row at its final place.  Rows beyond the caller's capacity are counted only.
// The trip counts of the round loop and of the loop over live windows are read from LDS behind a barrier, never taken from a lane's own arithmetic; every loop is
// bounded by max_depth <= 40 and the list capacities.  No float atomics, no polling, no workgroup waits on another, nothing of the iteration's scratch, no tj_stats
// counter, no launch count.  Read-only: the kernels write the query's own buffers only.
#pragma once
#include "kernels_peak_dynamics.h"

namespace tj {

static_assert(sizeof(tj_dyn_gate) == 16 && sizeof(tj_dynwin_row) == 96, "the records' layout (include/trajadmm.h)");

constexpr int DW_THREADS = WIN_LANES;   // one wave per slot

// a live window (MIXED) or a kept one (IN, or an EDGE leaf): [sa, sb] of segment tr; ga / gb = tr + sa / tr + sb, the position on the flight (the sort's and the chain's
// keys); g0 / g5 = sigma * the value attained at sa / sb
struct DynLeaf { double sa, sb, ga, gb, g0, g5; int tr, in; };

// dev_query.h's WinSlotArgs and the gates
struct DynwinArgs : WinSlotArgs<DynLeaf> {
  const tj_dyn_gate* gates; // [n_gates], the levels resolved
  int n_gates;
};

// ONE evaluation, in a lane's registers: the class of [sa, sb] of segment tr against the gate, and the window with its attained ends
template <int DEG>
__device__ __forceinline__ int dynwin_eval(const Dev& D, const double* __restrict__ nu, double ptu, int tr, double sa, double sb, int sense, double level, DynLeaf& w) {
  double o[3][DEG + 1];
  peak_net<DEG>(D, nu, tr, sa, sb, o);
  const double den = peak_den<DEG>(seg_weight(D, tr), ptu);
  double ub = -INFINITY, v0 = 0.0, vn = 0.0;
#pragma unroll
  for (int i = 0; i <= DEG; i++) {
    const double v = norm3(o[0][i], o[1][i], o[2][i]) / den;
    ub = fmax(ub, v);
    if (i == 0) v0 = v;
    if (i == DEG) vn = v;
  }
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    d[k] = o[k][0];
#pragma unroll
    for (int i = 1; i <= DEG; i++) d[k] = d[k] + o[k][i];
  }
  const double nd = norm3(d[0], d[1], d[2]);
  double m = INFINITY;
#pragma unroll
  for (int i = 0; i <= DEG; i++) m = fmin(m, o[0][i] * d[0] + o[1][i] * d[1] + o[2][i] * d[2]);
  const double lb = nd > 0.0 && m > 0.0 ? (m / nd) / den : 0.0;
  int cls;
  if (sense == TJ_DYNWIN_ABOVE) cls = ub < level ? WIN_OUT : (lb >= level ? WIN_IN : WIN_MIXED);
  else cls = lb > level ? WIN_OUT : (ub <= level ? WIN_IN : WIN_MIXED);
  const double sigma = sense == TJ_DYNWIN_ABOVE ? -1.0 : 1.0;
  w = DynLeaf{sa, sb, (double)tr + sa, (double)tr + sb, sigma * v0, sigma * vn, tr, cls == WIN_IN ? 1 : 0};
  return cls;
}

// the slot's search: dev_query.h's win_lane_search with dynwin_eval at the gate's degree as its evaluation
__global__ __launch_bounds__(DW_THREADS) void k_dynwin_refine(Dev D, DynwinArgs A) {
  const int ui = blockIdx.x / A.n_gates, k = blockIdx.x - ui * A.n_gates, u = D.u0 + ui;
  __shared__ int s_leaf, s_next, s_work;
  const tj_dyn_gate g = A.gates[k];   // (the gate is the block's: every branch below is taken by the whole workgroup)
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const double ptu = A.pt[u];
  const auto search = [&](auto deg) {
    win_lane_search(D, A, blockIdx.x, u, s_leaf, s_next, s_work, [&](int tr, double sa, double sb, DynLeaf& w) { return dynwin_eval<decltype(deg)::value>(D, nu, ptu, tr, sa, sb, g.sense, g.level, w); });
  };
  if (g.quantity == TJ_DYNWIN_SPEED) search(std::integral_constant<int, 4>{});
  else if (g.quantity == TJ_DYNWIN_ACCEL) search(std::integral_constant<int, 3>{});
  else search(std::integral_constant<int, 2>{});
}

// the rows of a slot at their final place (win_slot_place): the slot's robot and gate, and the row's own fields
__global__ __launch_bounds__(DW_THREADS) void k_dynwin_place(Dev D, DynwinArgs A, tj_dynwin_row* out) {
  const int slot = blockIdx.x, ui = slot / A.n_gates, k = slot - ui * A.n_gates, u = D.u0 + ui;
  const tj_dyn_gate g = A.gates[k];
  const double sigma = g.sense == TJ_DYNWIN_ABOVE ? -1.0 : 1.0;
  win_slot_place(D, A, slot, u, sigma * g.level, [](const DynLeaf&, int&, int&) {},
                 [&](int r, const WinRowFold& f, const WinChain& ch, const DynLeaf& first, const DynLeaf& last, int leaves, int depth, int windows) {
                   tj_dynwin_row row;
                   f.put(row, sigma, ch);
                   row.robot = u; row.gate = k; row.quantity = g.quantity; row.sense = g.sense;
                   row.segment_first = first.tr; row.segment_last = last.tr;
                   row.leaves = leaves; row.depth = depth; row.windows = windows;
                   out[r] = row;
                 });
}

}  // namespace tj
