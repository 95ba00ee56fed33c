// kernels_flight_profile.h -- tj_flight_profile: where every robot is at the caller's flight times, how fast it moves there, and how far the NEAREST obstacle primitive
// and the nearest other robot are -- per sample, with no `range`.
//
// The five other queries (dev_query.h) answer with a minimum per robot or pair, and only inside `range`: their obstacle walk is bvh_query at a fixed m, which at
// m = +infinity makes every primitive a candidate.  A profile needs the nearest primitive however far it is, per sample.  The definition (include/trajadmm.h), per
// owned robot u and time t:
//   segment   j = timed_first_segment(t, piece_time[u], res, S), tj_audit_timed's rule; j == S: the robot has arrived and stays at hull_entry(S - 1, 5, .)
//   position  b_0 of bez_restrict(raw hull of segment j, s, s), s = clamp01((t - Tj) / (Tj1 - Tj)): five de Casteljau steps (1 - s) * x + s * y per axis
//   dynamics  tj_audit's nets v_i = 5 (P[i+1] - P[i]), a_i = 20 (P[i+2] - 2 P[i+1] + P[i]) evaluated at s by the same step; |v| / (w pt), |a| / (w pt)^2
//   obstacle  min over ALL primitives of obst_point_dist<PRIM>(position, primitive), equal values to the smallest caller index
//   robots    min over q != u of norm3(p_u(t) - p_q(t)), equal values to the smallest q
//
// TWO launches whatever the fleet's size, the number of samples and the number of primitives:
//   k_profile_points   one lane per (robot, sample), ALL robots: segment or hover, position, speed, accel.  The position goes to pos[sample][robot][3] (the partner
//                      scan needs every robot); an owned robot's lane also writes those fields of its record.
//   k_profile_nearest  eight lanes per (owned robot, sample), eight samples per wave: a depth-first NEAREST-NEIGHBOUR descent of the implicit 8-ary box pyramid with
//                      a shrinking bound, then the partner scan over pos (lanes strided over q), then the rest of the record.
//
// THE WALK.  A group of eight lanes owns one sample and a stack of (node, bound) in LDS.  A step pops the top; if its bound can still matter the eight lanes load the
// node's eight children (192 contiguous bytes of fp32 boxes: one dependent round trip per step), each forms its child's lower bound, the kept children are ranked
// across the group and pushed so that the NEAREST is on top.  A popped level-0 node is a leaf of eight primitives: one per lane, distance, group argmin by
// (distance, caller's index) into the running best.  The top level (up to 64 boxes) is pushed whole, its nearest box last.
//
// EXACTNESS.  The result equals the brute-force minimum over all primitives with ties to the smallest caller index, bit for bit, because a node is pruned only when
// no primitive under it can EQUAL or beat the final minimum in the computed distances:
//   * a stored box is the fp64 union of what lies under it rounded OUTWARD to fp32 (kernels_bvh.h), so it contains every primitive under it and the true distance
//     from the point to any of them is >= the true distance to the box;
//   * the bound is that distance formed in fp64 from exact inputs (float -> double is exact): per axis one subtraction, then three products, two sums and a square
//     root -- within a few units of 2^-53 RELATIVE of the true box distance, whatever the coordinates' magnitude (no cancellation of rounded values).  On the stack
//     it is rounded DOWN to fp32 (dev_f32_down): smaller still, never larger;
//   * the computed distance of a cloud point, norm3 of the difference, is likewise within a few 2^-53 relative of its true distance; a triangle's is the norm of
//     the GJK's v, a point of the Minkowski difference formed from barycentric weights: not below the true distance by more than a few 2^-53 of the COORDINATES;
//   * so for a primitive under a node: computed distance >= bound * (1 - 1e-15) - 1e-12 * |coordinates|.  The prune rule is bound > best * 1.000001 + 1e-9
//     (box_near's guard, dev_query.h): it holds only where every primitive under the node computes strictly above the running best, which is never below the
//     final minimum.  A primitive that ties the minimum has a bound <= its distance * (1 + 1e-15) and is always visited; the running best takes it by index.
//   The set of VISITED primitives depends on the order of the descent; the minimum over it, taken with the total order (distance, caller's index), does not.
//
// MEMORY.  Bounded by construction: depth-first, a pop removes one node and pushes at most its 8 children one level down, so the stack never holds more than the
// top level (<= 64) plus 8 per level below it: cap = 64 + 8 * (nlevels - 1) entries of 8 bytes per sample (the host sizes the launch's LDS from nlevels: 6 KiB per
// wave for 1 M primitives).  A store is also guarded against `cap`; the guard cannot fire.  No input -- equal distances, a sphere of primitives around the point
// -- can overflow anything: TJ_ERR_CAPACITY does not exist for this call.
// No float atomics, no polling, nothing of the iteration's scratch, no environment switch.  Read-only: the kernels write the query's own buffers only.
#pragma once
#include "kernels_bvh.h"   // dev_f32_down
#include "kernels_obstacle_approach.h"

namespace tj {

constexpr int FP_THREADS = 256;   // k_profile_points: one lane per (robot, sample)

struct ProfileArgs {
  const double* net;     // [U][3][T] control nets: the solver's own, or the copy a group assembled from the owners
  const double* pt;      // [U] piece_time of every robot: the solver's own, or the group's copy
  const int* order;      // sorted primitive -> index in the caller's obstacle list
  double* times;         // [K] the caller's times
  double* pos;           // [K][U][3] position of EVERY robot at every time
  int K, cap;            // samples; stack entries per sample (k_profile_nearest)
};

// one de Casteljau evaluation of a net of N points at s: N - 1 steps (1 - s) * x + s * y
template <int N>
__device__ __forceinline__ double profile_casteljau(double (&r)[N], double s) {
  const double us = 1 - s;
#pragma unroll
  for (int k = N - 1; k > 0; k--)
#pragma unroll
    for (int m = 0; m < k; m++) r[m] = us * r[m] + s * r[m + 1];
  return r[0];
}

__global__ __launch_bounds__(FP_THREADS) void k_profile_points(Dev D, ProfileArgs A, tj_profile_sample* out) {
  const int K = A.K, U = D.U, S = D.S;
  const int item = blockIdx.x * FP_THREADS + threadIdx.x;
  if (item >= U * K) return;
  const int u = item / K, k = item - u * K;
  const double t = A.times[k], ptu = A.pt[u], res = (double)D.res;
  const double* nu = A.net + (size_t)u * 3 * D.T;
  const int j = timed_first_segment(t, ptu, res, S);
  double p[3], v[3] = {0.0, 0.0, 0.0}, a[3] = {0.0, 0.0, 0.0}, speed = 0.0, accel = 0.0;
  if (j >= S) {
#pragma unroll
    for (int x = 0; x < 3; x++) p[x] = hull_entry(D, nu, S - 1, 5, x);
  } else {
    const double Tj = (j / res) * ptu, Tj1 = ((j + 1) / res) * ptu, s = clamp01((t - Tj) / (Tj1 - Tj));
#pragma unroll
    for (int x = 0; x < 3; x++) {
      double P[6], b[6], vn[5], an[4];
#pragma unroll
      for (int i = 0; i < 6; i++) { P[i] = hull_entry(D, nu, j, i, x); b[i] = P[i]; }
#pragma unroll
      for (int i = 0; i < 5; i++) vn[i] = 5 * (P[i + 1] - P[i]);
#pragma unroll
      for (int i = 0; i < 4; i++) an[i] = 20 * (P[i + 2] - 2 * P[i + 1] + P[i]);
      p[x] = profile_casteljau(b, s); v[x] = profile_casteljau(vn, s); a[x] = profile_casteljau(an, s);
    }
    const double w = seg_weight(D, j);
    speed = norm3(v[0], v[1], v[2]) / (w * ptu);
    accel = norm3(a[0], a[1], a[2]) / (w * w * ptu * ptu);
  }
  double* q = A.pos + ((size_t)k * U + u) * 3;
  q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
  if (u >= D.u0 && u < D.u1) {   // the rest of the record: k_profile_nearest
    tj_profile_sample& r = out[(size_t)u * K + k];
    r.time = t; r.x = p[0]; r.y = p[1]; r.z = p[2]; r.speed = speed; r.accel = accel; r.segment = j >= S ? S : j;
    r.flags = (j >= S ? TJ_PROFILE_HOVER : 0) | (speed >= D.vel_limit ? TJ_PROFILE_SPEED : 0) | (accel >= D.acc_limit ? TJ_PROFILE_ACCEL : 0);
  }
}

// the lower bound of a node: Euclidean distance from the point to the fp32 box, in fp64 (an empty padding box -- lo = +inf, hi = -inf -- is +infinity away)
__device__ __forceinline__ double profile_box_dist(const float* b, const double (&p)[3]) {
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = fmax(fmax((double)b[k] - p[k], p[k] - (double)b[3 + k]), 0.0);
  return norm3(d[0], d[1], d[2]);
}
// can a node whose bound is `b` hold a primitive that equals or beats `best`?  (the header's exactness argument; best = +infinity keeps everything)
__device__ __forceinline__ bool profile_keep(double b, double best) { return !(b > best * 1.000001 + 1e-9); }

// minimum of (d, key) in lexicographic order over a group of eight lanes (wave_argmin's order); every lane of the group ends with the same pair
__device__ __forceinline__ void group8_argmin(double& d, int& key) {
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) {
    const double d2 = __shfl_xor(d, off); const int k2 = __shfl_xor(key, off);
    const bool take = d2 < d || (d2 == d && k2 < key);
    take_if(take, d, d2); take_if(take, key, k2);
  }
}

constexpr int FP_LEVEL_SHIFT = 28;   // a stack entry's node: level << 28 | index in the level (level < MAX_LEVELS = 12; a level holds at most N / 8 < 2^28 boxes)

template <int PRIM>
__global__ __launch_bounds__(64) void k_profile_nearest(Dev D, ProfileArgs A, tj_profile_sample* out) {
  extern __shared__ unsigned long long fp_stack[];   // [8 samples][cap] entries: node | fp32 bound (rounded down) << 32
  const int lane = lane_id(), g = lane >> 3, sub = lane & 7, K = A.K, U = D.U, cap = A.cap;
  const int total = (D.u1 - D.u0) * K, item = blockIdx.x * 8 + g;
  const bool valid = item < total;
  const int it = min(item, total - 1), ui = it / K, k = it - ui * K, u = D.u0 + ui;
  double p[3];
  { const double* q = A.pos + ((size_t)k * U + u) * 3; p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
  unsigned long long* stack = fp_stack + (size_t)g * cap;

  // ---- the nearest primitive ----
  double od = INFINITY; int oi = INT_MAX;
  int sp = 0;   // (the same value in the eight lanes of a group)
  if (D.N > 0) {
    // the top level: every box, the nearest one last (on top)
    const int top = D.nlevels - 1, nt = D.lvl_n[top];
    const float* lvl = D.boxes + (size_t)D.lvl_off[top] * 6;
    double bd[8], nb = INFINITY; int nn = INT_MAX;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int node = 8 * r + sub;
      bd[r] = node < nt ? profile_box_dist(lvl + (size_t)node * 6, p) : INFINITY;
      if (node < nt && (bd[r] < nb || (bd[r] == nb && node < nn))) { nb = bd[r]; nn = node; }
    }
    group8_argmin(nb, nn);
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int node = 8 * r + sub;
      const bool keep = node < nt && node != nn;
      const unsigned m8 = (unsigned)(ballot(keep) >> (8 * g)) & 0xffu;
      const int at = sp + __popc(m8 & ((1u << sub) - 1u));
      if (keep && at < cap) stack[at] = (unsigned long long)(unsigned)(top << FP_LEVEL_SHIFT | node) | (unsigned long long)__float_as_uint(dev_f32_down(bd[r])) << 32;
      sp += __popc(m8);
    }
    if (sub == 0 && sp < cap) stack[sp] = (unsigned long long)(unsigned)(top << FP_LEVEL_SHIFT | nn) | (unsigned long long)__float_as_uint(dev_f32_down(nb)) << 32;
    sp++;
  }
  // the descent: wave-uniform loop, a group takes part while its stack holds something
  for (;;) {
    const bool active = valid && sp > 0;
    if (!__any(active)) break;
    __syncthreads();   // (a one-wave block: the group's pushes of the last step are in LDS before the pop)
    if (!active) continue;
    const unsigned long long e = stack[--sp];
    const double bound = (double)__uint_as_float((unsigned)(e >> 32));
    if (!profile_keep(bound, od)) continue;
    const int lv = (int)((unsigned)e >> FP_LEVEL_SHIFT), idx = (int)((unsigned)e & ((1u << FP_LEVEL_SHIFT) - 1u));
    if (lv == 0) {   // a leaf: eight primitives, one per lane
      const int pt = idx * 8 + sub;
      double d = INFINITY; int id = INT_MAX;
      if (pt < D.N) {
        bool near = true;
        if constexpr (PRIM == 3) near = profile_keep(profile_box_dist(D.leafbox + (size_t)pt * 6, p), od);   // the triangle's own box first: the GJK only where it can matter
        if (near) { d = obst_point_dist<PRIM>(V3{p[0], p[1], p[2]}, PrimOf<PRIM>::load(D, pt)); id = A.order[pt]; }
      }
      group8_argmin(d, id);
      if (d < od || (d == od && id < oi)) { od = d; oi = id; }
    } else {         // an inner node: its eight children, the kept ones pushed nearest on top
      const int cl = lv - 1, child = idx * 8 + sub;
      const bool live = child < D.lvl_n[cl];
      const double b = live ? profile_box_dist(D.boxes + ((size_t)D.lvl_off[cl] + child) * 6, p) : INFINITY;
      const bool keep = live && profile_keep(b, od);
      const double key = keep ? b : INFINITY;
      int rank = 0, n = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const double kj = __shfl(key, (lane & ~7) + j); const bool pj = __shfl((int)keep, (lane & ~7) + j) != 0;
        rank += pj && (kj < key || (kj == key && j < sub)); n += pj;
      }
      const int at = sp + n - 1 - rank;
      if (keep && at < cap) stack[at] = (unsigned long long)(unsigned)(cl << FP_LEVEL_SHIFT | child) | (unsigned long long)__float_as_uint(dev_f32_down(b)) << 32;
      sp += n;
    }
  }

  // ---- the nearest other robot at the same time: lanes strided over q, ascending per lane (a strict comparison keeps the first) ----
  double pd = INFINITY; int pq = INT_MAX;
  if (D.multi()) {
    const double* row = A.pos + (size_t)k * U * 3;
    for (int q = sub; q < U; q += 8) {
      if (q == u) continue;
      const double d = norm3(p[0] - row[3 * q], p[1] - row[3 * q + 1], p[2] - row[3 * q + 2]);
      if (d < pd) { pd = d; pq = q; }
    }
    group8_argmin(pd, pq);
  }
  if (valid && sub == 0) {
    tj_profile_sample& r = out[(size_t)u * K + k];
    r.obs_distance = od; r.obs_index = oi == INT_MAX ? -1 : oi;
    r.robot_distance = pd; r.robot = pq == INT_MAX ? -1 : pq;
    r.flags |= (oi != INT_MAX && od <= D.offset ? TJ_PROFILE_OBS_CONTACT : 0) | (pq != INT_MAX && pd <= D.offset ? TJ_PROFILE_PAIR_CONTACT : 0);
  }
}

}  // namespace tj
