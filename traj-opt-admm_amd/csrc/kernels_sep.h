// kernels_sep.h -- separating-plane construction ("z-update: GJK separating-plane projection"
// in BASELINE.json's vocabulary).
//
//   obstacle planes (obs_query_body / obs_solve_body, compaction in kernels_pairs.h): per (robot, Bezier segment)
//               hull -> static-BVH query -> 49-axis k-DOP cull; per candidate GJK -> plane (c,d).
//               Replaces BVH::DCDCollision (BVH.cpp:149-193),
//               aabb::Tree::query (AABB.cc:608-667), CCD::KDOPDCD (CCD.h:354-413) and
//               Separate::opengjk (Separate.h:18-163) as sequenced by separate_plane
//               (Optimization3D_multi.h:176-235 / Optimization3D_admm.h:69-197).
//   plane_pair  device function for one robot pair (hull-hull GJK + 1-D Newton on the offset),
//               used by kernels_pairs.h which replaces separate_self (Optimization3D_multi.h:237-342).
//
// The BVH is an implicit 8-ary box hierarchy over Morton-sorted primitives (points, or triangles for BASELINE config 5).
// A wave walks it level by level: 64 lanes test 8 frontier nodes x 8 children per step (coalesced 24-B fp32 boxes,
// rounded outward; 192 B per parent), survivors are compacted into the next frontier with ballot + popcount.  The tree
// shape is free: the candidate SET is defined by the reference's leaf predicate (AABB.cc:141, touching counts), which
// is evaluated here in fp64 on the primitives themselves (a point, or the exact box of a triangle's three vertices).
#pragma once
#include "dev_common.h"
#include "dev_linalg.h"
#include "dev_crmath.h"

namespace tj {

struct QBox { double lo[3], hi[3]; };

// THE box predicate of the walk, the leaves and the pair tiles: the box [lo, hi] is within m of the query box [qlo, qhi] -- rejected if hi + m < qlo or
// lo > qhi + m on any axis (query.overlaps(node), AABB.cc:141: touching counts).  fp64 bounds; an fp32 box (rounded outward) converts at the call.
// box_near_axis is the predicate on one axis, for a caller that forms its bounds axis by axis (the triangle leaf).
__device__ __forceinline__ bool box_near_axis(double lo, double hi, double qlo, double qhi, double m) { return !((hi + m < qlo) | (lo > qhi + m)); }
__device__ __forceinline__ bool box_near(const double* lo, const double* hi, const double* qlo, const double* qhi, double m) {
  bool hit = true;
#pragma unroll
  for (int k = 0; k < 3; k++) hit = hit & box_near_axis(lo[k], hi[k], qlo[k], qhi[k], m);
  return hit;
}
__device__ __forceinline__ bool box_near(const float* b, const QBox& q, double m) {   // b: lo.xyz, hi.xyz
  const double d[6] = {(double)b[0], (double)b[1], (double)b[2], (double)b[3], (double)b[4], (double)b[5]};
  return box_near(d, d + 3, q.lo, q.hi, m);
}

// ---- obstacle primitives as GJK bodies ----
template <int PRIM> struct PrimOf;
template <> struct PrimOf<1> {
  using Body = BodyPoint;
  static __device__ __forceinline__ Body load(const Dev& D, int i) { return BodyPoint{V3{D.px[i], D.py[i], D.pz[i]}}; }
};
template <> struct PrimOf<3> {
  using Body = BodyTri;
  static __device__ __forceinline__ Body load(const Dev& D, int i) {
    const double* t = D.tri + (size_t)i * 9;
    return BodyTri{V3{t[0], t[1], t[2]}, V3{t[3], t[4], t[5]}, V3{t[6], t[7], t[8]}};
  }
};

// Wave-cooperative query.  `process(pt)` is called by all 64 lanes with a candidate point index
// (or -1) and may use wave collectives.  Returns candidates found; adds visited boxes to *visits.
// BQ_UNROLL: chunks of 8 frontier nodes whose box loads are in flight together (4 in the plane query, whose kernel has
// registers to spare; 1 in the CCD query, where the per-lane GJK already fills the register file)
// The top level's boxes do not depend on the query: a caller can fetch its lane's box (bvh_top_box) TOGETHER with the record that
// holds the query box and hand it in -- one dependent round trip less at the head of the walk.
struct TopBox { float b[6]; };
constexpr int BVH_SKIP_MAX = 8;   // frontier nodes up to which a level pair is taken in one step (64 boxes per node)
__device__ __forceinline__ TopBox bvh_top_box(const Dev& D) {
  TopBox t{{0, 0, 0, 0, 0, 0}};
  if (D.N == 0) return t;
  const int top = D.nlevels - 1, lane = lane_id();
  const float* p = D.boxes + (size_t)(D.lvl_off[top] + min(lane, D.lvl_n[top] - 1)) * 6;
#pragma unroll
  for (int k = 0; k < 6; k++) t.b[k] = p[k];
  return t;
}
// The walk's LDS scratch, one wave's: the two frontiers and the candidate buffer (CAND = 128: the leaves flush at 64, and a chunk's up to 64 hits land behind
// up to 63 kept ones).  A kernel declares INTS ints (or counts DOUBLES into a buffer of doubles it carves) and hands carve() of them to bvh_query.
struct WalkScratch {
  static constexpr int CAND = 128, INTS = 2 * FRONT_CAP + CAND, DOUBLES = INTS / 2;
  int *fa, *fb, *cand;
  static __device__ __forceinline__ WalkScratch carve(void* p) { int* a = (int*)p; return WalkScratch{a, a + FRONT_CAP, a + 2 * FRONT_CAP}; }
};
// Lanes over a chunk of the frontier, FAN children per node (8: one level down; 64: the grandchildren, a level pair in one step): 64 / FAN frontier nodes
// per chunk, lane -> (the chunk's slot in the frontier, the child of that slot's node).  The leaves are the children of the last frontier at FAN 8.
template <int FAN> __device__ __forceinline__ int walk_slot(int base, int c, int lane) { return base + (64 / FAN) * c + lane / FAN; }
template <int FAN> __device__ __forceinline__ int walk_child(int node, int lane) { return node * FAN + lane % FAN; }
// ONE step of the walk: frontier cur[0, count) -> the survivors among its nodes' FAN-children on level lv, into nxt in frontier order; returns their number.
// Each step is a dependent global load (~0.7 us).  BQ_UNROLL chunks are therefore fetched together: all box loads of the group are issued first (branch-free,
// clamped addresses), then the chunks are tested and compacted one by one in frontier order (the order of the survivors, and with it of the candidate
// list, is unchanged).  More than FRONT_CAP survivors: ERR_FRONT_OVERFLOW, the step ends with what it has.
template <int FAN, int BQ_UNROLL>
__device__ __forceinline__ int walk_step(const Dev& D, const QBox& q, double m, int lv, const int* cur, int* nxt, int count, unsigned long long& nv) {
  constexpr int NODES = 64 / FAN;
  const int lane = lane_id(), nl = D.lvl_n[lv];
  const float* lvl = D.boxes + (size_t)D.lvl_off[lv] * 6;
  int ncount = 0; bool overflow = false;
  for (int base = 0; base < count && !overflow; base += NODES * BQ_UNROLL) {
    int child[BQ_UNROLL]; bool live[BQ_UNROLL]; float bx[BQ_UNROLL][6];
#pragma unroll
    for (int c = 0; c < BQ_UNROLL; c++) {
      const int slot = walk_slot<FAN>(base, c, lane);
      child[c] = walk_child<FAN>(cur[min(slot, count - 1)], lane);
      live[c] = slot < count && child[c] < nl;
      const float* b = lvl + (size_t)min(child[c], nl - 1) * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) bx[c][k] = b[k];
    }
#pragma unroll
    for (int c = 0; c < BQ_UNROLL; c++) {
      if (base + NODES * c >= count) break;
      const bool hit = live[c] & box_near(bx[c], q, m);
      const unsigned long long mask = ballot(hit);
      const int tot = __popcll(mask);
      if (ncount + tot > FRONT_CAP) { if (lane == 0) atomicOr(&D.ctl->error, ERR_FRONT_OVERFLOW); overflow = true; break; }
      if (hit) nxt[ncount + prefix_count(mask)] = child[c];
      ncount += tot;
      nv += FAN * min(NODES, count - (base + NODES * c));
    }
  }
  __syncthreads();
  return ncount;
}
template <int BQ_UNROLL, int PRIM, class F>
__device__ int bvh_query(const Dev& D, const QBox& q, double m, const WalkScratch& ws, unsigned long long* visits, F&& process, const TopBox* pre = nullptr) {
  const int lane = lane_id();
  if (D.N == 0) return 0;
  int top = D.nlevels - 1;
  int count = 0;
  unsigned long long nv = 0;
  {
    const int n = D.lvl_n[top];
    bool hit = false;
    if (lane < n) hit = box_near(pre ? pre->b : D.boxes + (size_t)(D.lvl_off[top] + lane) * 6, q, m);
    const unsigned long long mask = ballot(hit);
    if (hit) ws.fa[prefix_count(mask)] = lane;
    count = __popcll(mask);
    nv += n;
  }
  if (count == 0) { if (visits) *visits += nv; return 0; }   // wave-uniform: nothing of the obstacle set is near this box (the common case)
  __syncthreads();
  int* cur = ws.fa; int* nxt = ws.fb; int* const cand = ws.cand;
  auto step = [&](int ncount) { int* t = cur; cur = nxt; nxt = t; count = ncount; };
  // DOUBLE STEPS while the frontier is small (the top of a deep pyramid: 1 M primitives are five levels): the 64 GRANDchildren of a frontier node are tested by
  // the 64 lanes at once -- one dependent round trip per two levels instead of two.  A box contains its children's boxes (unions, rounded outward monotonically),
  // so a grandchild that is hit has a hit parent: the survivors at level lv - 1 are the same nodes in the same (ascending) order as after two single steps.
  while (top >= 2 && count <= BVH_SKIP_MAX && D.bvh_skip) {
    step(walk_step<64, BQ_UNROLL>(D, q, m, top - 2, cur, nxt, count, nv));
    top -= 2;
    if (count == 0) break;
  }
  for (int lv = top - 1; lv >= 0; lv--) step(walk_step<8, BQ_UNROLL>(D, q, m, lv, cur, nxt, count, nv));
  if constexpr (BQ_UNROLL == 4) TJ_TIC(D, K_SEP_OBS, 2);   // timing build: the plane query's walk is done, leaves next
  int nc = 0, found = 0;
  for (int base = 0; base < count; base += 8 * BQ_UNROLL) {
    int pts[BQ_UNROLL]; bool live[BQ_UNROLL]; double pp[BQ_UNROLL][3]; float lb[BQ_UNROLL][6];
#pragma unroll
    for (int c = 0; c < BQ_UNROLL; c++) {  // leaf boxes -> primitives: again all loads of the group first
      const int slot = walk_slot<8>(base, c, lane);
      const int pt = walk_child<8>(cur[min(slot, count - 1)], lane);
      pts[c] = pt; live[c] = slot < count && pt < D.N;
      const int pc = min(pt, D.N - 1);
      if constexpr (PRIM == 1) { pp[c][0] = D.px[pc]; pp[c][1] = D.py[pc]; pp[c][2] = D.pz[pc]; }
      else {
#pragma unroll
        for (int k = 0; k < 6; k++) lb[c][k] = D.leafbox[(size_t)pc * 6 + k];
      }
    }
#pragma unroll
    for (int c = 0; c < BQ_UNROLL; c++) {
      if (base + 8 * c >= count) break;
      bool hit;
      if constexpr (PRIM == 1) hit = live[c] & box_near(pp[c], pp[c], q.lo, q.hi, m);   // a point is its own box
      else {
        // fp32 pre-filter (conservative), then the exact box of the three vertices in fp64 (BVH::InitObstacle, BVH.cpp:26-46)
        hit = false;
        if (live[c] & box_near(lb[c], q, m)) {
          const double* t = D.tri + (size_t)pts[c] * 9;
          hit = true;
#pragma unroll
          for (int k = 0; k < 3; k++) {   // (axis by axis: with the three axes' bounds formed first, k_ccd_obs<3> took 3 more registers and k_ccd_lean<3> 2)
            double lo = INFINITY, hi = -INFINITY;
#pragma unroll
            for (int j = 0; j < 3; j++) { const double lv = t[3 * j + k]; if (lv < lo) lo = lv; if (lv > hi) hi = lv; }
            hit = hit & box_near_axis(lo, hi, q.lo[k], q.hi[k], m);
          }
        }
      }
      const unsigned long long mask = ballot(hit);
      if (hit) cand[nc + prefix_count(mask)] = pts[c];
      nc += __popcll(mask);
      found += __popcll(mask);
      __syncthreads();
      if (nc >= 64) {
        process(cand[lane]);
        const int left = nc - 64;
        const int keep = lane < left ? cand[64 + lane] : 0;
        __syncthreads();
        if (lane < left) cand[lane] = keep;
        nc = left;
        __syncthreads();
      }
    }
  }
  if constexpr (BQ_UNROLL == 4) TJ_TIC(D, K_SEP_OBS, 3);
  if (nc > 0) process(lane < nc ? cand[lane] : -1);
  if (visits) *visits += nv;
  return found;
}

// THE comparison of the 49-axis test (CCD::KDOPDCD CCD.h:354-413, SelfKDOPDCD :535-587, and their swept forms): the intervals [alo, ahi] and [blo, bhi] of two
// bodies on one axis are more than d apart.  Two bodies pass the test if no axis says so.
__device__ __forceinline__ bool kdop_apart(double alo, double ahi, double blo, double bhi, double d) { return (bhi < alo - d) | (ahi < blo - d); }

// The obstacle cull for up to 64 candidates held one per LANE (lanes [0, n)), done by the whole wave: lanes over the 49 AXES
// (axis and the hull's interval in registers), candidates one after the other with their vertices broadcast by v_readlane: the body-2 loop over
// _position.rows() of CCD::KDOPDCD (CCD.h:391-400), all axes without an early exit.  ~20 instructions per point candidate instead of a 49-step loop of
// dependent memory round trips per lane (118 us for a segment under an obstacle slab, once the whole tail of k_front at 256 robots); returns this lane's
// verdict.  axv = this lane's axis (x, y, z), lo_ax / hi_ax = hull interval on it.
template <class B>
__device__ __forceinline__ bool kdop_cull_wave(const B& body, int n, const V3& axv, double lo_ax, double hi_ax, double d, int lane) {
  unsigned long long pass = 0ull;
  for (int i = 0; i < n; i++) {   // wave-uniform
    double up = -INFINITY, lo = INFINITY;
#pragma unroll
    for (int v = 0; v < B::N; v++) {
      const V3 p = body.get(v);
      const double lv = axv.x * readlane_f64(p.x, i) + axv.y * readlane_f64(p.y, i) + axv.z * readlane_f64(p.z, i);
      if (lv < lo) lo = lv;
      if (lv > up) up = lv;
    }
    const bool sep = lane < 49 && kdop_apart(lo_ax, hi_ax, lo, up, d);
    if (ballot(sep) == 0ull) pass |= 1ull << i;
  }
  return (pass >> lane) & 1ull;
}
// The cull as the two obstacle walks call it from bvh_query's process(pt) (obs_query_body: hull intervals at offset + margin; ccd_obs_body: swept intervals at
// offset): this lane's axis and the hull's interval on it (klo / khi: the 49 intervals, LDS), fetched at the first candidate (wave-uniform) and kept in registers
// from then on; cull() loads the lane's candidate into qb and returns its verdict (false for a lane without one).  Candidates sit in lanes [0, ncand).
struct KdopLane {
  V3 axv{0, 0, 0}; double lo = 0, hi = 0; bool ready = false;
  template <int PRIM>
  __device__ __forceinline__ bool cull(const Dev& D, const double* klo, const double* khi, int pt, double d, int lane, typename PrimOf<PRIM>::Body& qb) {
    if (!ready) {
      const int ax = min(lane, 48);
      axv = V3{D.kdop[3 * ax], D.kdop[3 * ax + 1], D.kdop[3 * ax + 2]}; lo = klo[ax]; hi = khi[ax];
      ready = true;
    }
    const int ncand = __popcll(ballot(pt >= 0));
    qb = PrimOf<PRIM>::load(D, max(pt, 0));
    return kdop_cull_wave(qb, ncand, axv, lo, hi, d, lane) && pt >= 0;
  }
};

// witness to plane, first step of every form below: the unit normal c = v / |v| of the GJK witness vector v; false (no plane) if the bodies are farther apart than dist
__device__ __forceinline__ bool plane_normal(const V3& v, double dist, double& c0, double& c1, double& c2) {
  const double cn = norm3(v.x, v.y, v.z);
  if (cn > dist) return false;
  c0 = v.x / cn; c1 = v.y / cn; c2 = v.z / cn;
  return true;
}
// Separate::opengjk (Separate.h:18-163): plane (c,d) between a 6-point hull and an obstacle body of B::N vertices, from the GJK witness vector v of
// hull - body (Separate.h:107-151): rejected if |v| > dist; d0 = min_i(-c . B_i), the loop the reference keeps commented out at Separate.h:123-131 (one
// vertex, a cloud point: d0 = -c . q)
template <class B>
__device__ __forceinline__ bool plane_from_witness_body(const V3& v, const B& body, double dist, double offset, double& c0, double& c1, double& c2, double& dd) {
  if (!plane_normal(v, dist, c0, c1, c2)) return false;
  const V3 q0 = body.get(0);
  double d0 = -c0 * q0.x - c1 * q0.y - c2 * q0.z;
#pragma unroll
  for (int i = 1; i < B::N; i++) { const V3 q = body.get(i); const double d_ = -c0 * q.x - c1 * q.y - c2 * q.z; if (d0 > d_) d0 = d_; }
  dd = d0 - offset;
  return true;
}

__device__ __forceinline__ double dot_fixed3(double c0, double c1, double c2, const double* r, int st = 1) { return c0 * r[0] + (c1 * r[st] + c2 * r[2 * st]); }  // Eigen unrolled 3-term order (Separate.h:268,276); st: stride between r's entries
// the offset of the plane midway between two hulls along the unit normal c (Separate.h:262-280): d = (min over B of -c . B_i + max over A of -c . A_i) / 2
__device__ __forceinline__ double pair_midplane(double c0, double c1, double c2, const double* A, const double* Bq, int st) {
  double d0 = INFINITY, d1 = -INFINITY;
  for (int i = 0; i < 6; i++) { const double t = -dot_fixed3(c0, c1, c2, Bq + 3 * i * st, st); if (d0 > t) d0 = t; }
  for (int i = 0; i < 6; i++) { const double t = -dot_fixed3(c0, c1, c2, A + 3 * i * st, st); if (d1 < t) d1 = t; }
  return 0.5 * (d0 + d1);
}

// Separate::selfgjk (Separate.h:165-304) + Optimal_plane::optimal_d (Optimal_plane.h:13-71).
// A is the hull of the lower robot index.  Returns false if the hulls are farther than dist.
// capped = true when the Newton loop hit NEWTON_CAP.
// second half of plane_pair: from the GJK witness vector to the plane (separate so that a caller can act between the halves)
// cr_log out of line: the per-lane pair path lives in k_mid at its 256-register cap, where the inlined double-double pieces spill
__device__ __noinline__ double cr_log_call(double x) { return cr_log(x); }
// one barrier term of the offset Newton (Optimal_plane.h:13-71) at signed distance ds < m: its first and second derivative in the offset, before the side's sign.
// lg = log(ds / m), handed in: the lane path takes it from cr_log_call, the wave path from the inlined cr_log (both round like glibc's log, dev_crmath.h: the offset
// is then the reference's bit for bit)
__device__ __forceinline__ void offset_barrier_terms(double ds, double m, double lg, double& g1, double& g2) {
  g1 = -(2 * (ds - m) * lg + (ds - m) * (ds - m) / ds);
  g2 = -(2 * lg + 4 * (ds - m) / ds - (ds - m) * (ds - m) / (ds * ds));
}
__device__ inline bool plane_pair_finish(const V3& v, const double* A, const double* Bq, double dist, double m, double off, bool refine, double& e0, double& e1c, double& e2c, double& dpl, bool& capped, int* newton_iters = nullptr, int st = 1);
__device__ inline bool plane_pair(const double* A, const double* Bq, double dist, double m, double off, bool refine, double& e0, double& e1c, double& e2c, double& dpl, bool& capped, int* newton_iters = nullptr, int* gjk_iters = nullptr) {
  const V3 v = gjk(BodyHull{A}, BodyHull{Bq}, gjk_iters);
  return plane_pair_finish(v, A, Bq, dist, m, off, refine, e0, e1c, e2c, dpl, capped, newton_iters);
}
// st: stride between the entries of A / Bq (1: row-major [6][3] in global memory or LDS; the lane-per-pair path of large fleets keeps a transposed tile, BodyHullT)
__device__ inline bool plane_pair_finish(const V3& v, const double* A, const double* Bq, double dist, double m, double off, bool refine, double& e0, double& e1c, double& e2c, double& dpl, bool& capped, int* newton_iters, int st) {
  capped = false;
  if (!plane_normal(v, dist, e0, e1c, e2c)) return false;
  dpl = pair_midplane(e0, e1c, e2c, A, Bq, st);
  if (!refine) return true;
  int it = 0;
  for (; it < NEWTON_CAP; it++) {  // Newton on the offset until |grad| < 1e-2
    double grad = 0, hess = 0;
    for (int j = 0; j < 6; j++) {
      const double ds = (A[(3 * j) * st] * e0 + A[(3 * j + 1) * st] * e1c + A[(3 * j + 2) * st] * e2c) + dpl - 0.5 * off;
      if (ds < m) {
        double g1, g2;
        offset_barrier_terms(ds, m, cr_log_call(ds / m), g1, g2);
        grad += g1; hess += g2;
      }
    }
    for (int j = 0; j < 6; j++) {
      const double ds = -(Bq[(3 * j) * st] * e0 + Bq[(3 * j + 1) * st] * e1c + Bq[(3 * j + 2) * st] * e2c) - dpl - 0.5 * off;
      if (ds < m) {
        double g1, g2;
        offset_barrier_terms(ds, m, cr_log_call(ds / m), g1, g2);
        grad += -g1; hess += g2;
      }
    }
    const double dir = -grad / hess;
    dpl = dpl + 1.0 * dir;
    if (fabs(grad) < 1e-2) break;
  }
  capped = it == NEWTON_CAP;
  if (newton_iters) *newton_iters = it + 1;
  return true;
}

// plane_pair computed by a whole wave for ONE robot pair (all 64 lanes call it with the same arguments, A and Bq in
// LDS): wave-cooperative GJK, then the Newton refinement of the offset with its 12 barrier terms (the only
// transcendental work) evaluated by 12 lanes and summed in the reference's order.  Same expressions, same
// summation order as plane_pair => identical results.
__device__ __forceinline__ bool plane_pair_wave(const double* A, const double* Bq, double dist, double m, double off, int lane, double& e0, double& e1c, double& e2c, double& dpl,
                                       bool& capped, int* newton_iters, int* gjk_iters, const Dev* tic,
                                       GjkState& gst, bool resume, bool resume_finished) {   // resume: the query's first iterations were run elsewhere (spec_pair_body) and gst holds their state
  capped = false;
  bool gfin;
  V3 v;
#ifdef TJ_PHASE_TIMING
  long long prof[7] = {0, 0, 0, 0, 0, 0, 0};
  if (resume && resume_finished) v = gst.v; else v = gjk_wave_run(BodyHull{A}, BodyHull{Bq}, lane, gst, !resume, 50, gfin, tic ? prof : nullptr);
  if (tic && threadIdx.x == 0 && blockIdx.x < TJ_TIC_BLOCKS) for (int i = 0; i < 7; i++) tic->dbg[((size_t)K_OBS_SOLVE * TJ_TIC_BLOCKS + blockIdx.x) * TJ_TIC_SLOTS + i] = prof[i];
#else
  if (resume && resume_finished) v = gst.v; else v = gjk_wave_run(BodyHull{A}, BodyHull{Bq}, lane, gst, !resume, 50, gfin);
#endif
  if (gjk_iters) *gjk_iters = gst.k;
  TJ_ORDER(v.x);
  if (tic) TJ_TIC(*tic, K_SEP_SELF_SOLVE, 3);
  if (!plane_normal(v, dist, e0, e1c, e2c)) return false;
  dpl = pair_midplane(e0, e1c, e2c, A, Bq, 1);
  TJ_ORDER(dpl);
  if (tic) TJ_TIC(*tic, K_SEP_SELF_SOLVE, 4);
  const int j = lane < 6 ? lane : (lane < 12 ? lane - 6 : 0);
  const double* pt = lane < 6 ? A + 3 * j : Bq + 3 * j;
  const double px = pt[0], py = pt[1], pz = pt[2];
  int it = 0;
  for (; it < NEWTON_CAP; it++) {  // Newton on the offset until |grad| < 1e-2 (Optimal_plane.h:13-71)
    const double dp = px * e0 + py * e1c + pz * e2c;
    const double ds = lane < 6 ? dp + dpl - 0.5 * off : -dp - dpl - 0.5 * off;
    const bool act = lane < 12 && ds < m;
    double g1 = 0, g2 = 0;
    if (act) offset_barrier_terms(ds, m, cr_log(ds / m), g1, g2);
    const unsigned mask = (unsigned)__ballot(act);
    double grad = 0, hess = 0;
#pragma unroll
    for (int q = 0; q < 12; q++)
      if (mask & (1u << q)) {  // uniform
        const double a1 = gjk_rl(g1, q), a2 = gjk_rl(g2, q);
        if (q < 6) grad += a1; else grad += -a1;
        hess += a2;
      }
    const double dir = -grad / hess;
    dpl = dpl + 1.0 * dir;
    if (fabs(grad) < 1e-2) break;
  }
  capped = it == NEWTON_CAP;
  if (newton_iters) *newton_iters = it + 1;
  TJ_ORDER(dpl);
  if (tic) TJ_TIC(*tic, K_SEP_SELF_SOLVE, 5);
  return true;
}

__device__ inline bool plane_pair_wave(const double* A, const double* Bq, double dist, double m, double off, int lane, double& e0, double& e1c, double& e2c, double& dpl,
                                       bool& capped, int* newton_iters = nullptr, int* gjk_iters = nullptr, const Dev* tic = nullptr) {
  GjkState gst;
  return plane_pair_wave(A, Bq, dist, m, off, lane, e0, e1c, e2c, dpl, capped, newton_iters, gjk_iters, tic, gst, false, false);
}

// ---- obstacle planes in three steps --------------------------------------------------------------------------------
// (1) obs_query_body  one wave per (owned robot, segment): hull, BVH walk, k-DOP cull; the surviving points go to the
//                     segment's candidate list (traversal order, deterministic) and, one work item each, to a global list.
// (2) obs_solve_body  one wave per candidate (stride over the work list): wave-cooperative GJK hull-vs-point and the plane
//                     (c,d), written to the candidate's own slot with an epoch stamp.
// (3) compaction      kernels_pairs.h: stamped slots of a segment -> its plane list, in slot order.
// A segment next to an obstacle slab has > 100 candidates; solved inside the segment's own wave (64 divergent GJK paths
// per round) they made a 45 us tail on a 5 us kernel.  One wave per candidate runs them all at once.
// Plane order = candidate order = what the fused version produced, so downstream sums see the same sequence.
constexpr int OBS_SINGLE_MAX = 16;  // candidates of a segment that still get a wave each
// LDS of one unit, carved from a buffer the KERNEL owns: the union kernels run a different body per block, and function-local
// __shared__ arrays of exclusive branches are not overlaid by the compiler (their sizes add up, and with them go residency).
constexpr int OBS_P = 0, OBS_KLO = OBS_P + 18, OBS_KHI = OBS_KLO + 49, OBS_WALK = OBS_KHI + 49, OBS_LDS_DOUBLES = OBS_WALK + WalkScratch::DOUBLES;   // hull | its 49 intervals lo, hi | the walk's scratch: 1204
// A work item of the solve stage, two ints of Dev::obs_work: (segment, slot).  slot >= 0: the segment's candidate `slot`, for a whole wave; slot < 0: a batch of up to
// 64 candidates, one per lane, starting at candidate -(slot + 1).
struct ObsItem { int seg, first; bool batch; };
__device__ __forceinline__ int obs_item_slot(bool batched, int i) { return batched ? -(i * 64) - 1 : i; }   // item i of its segment
__device__ __forceinline__ ObsItem obs_item(int seg, int slot) { return ObsItem{seg, slot < 0 ? -(slot + 1) : slot, slot < 0}; }
// The plane slot of candidate i of a segment (Dev::oraw, Dev::ostamp): the solve wave leaves plane and epoch stamp there, the compaction (kernels_pairs.h)
// takes the slots stamped with this epoch in slot order.
__device__ __forceinline__ size_t obs_plane_slot(const Dev& D, size_t seg, int i) { return seg * D.cap_obs + i; }
__device__ __forceinline__ void obs_plane_store(const Dev& D, size_t sl, double c0, double c1, double c2, double dd, int epoch) {
  double* o = D.oraw + sl * 4;
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = dd;
  D.ostamp[sl] = epoch;
}
// use_cache: the hull cache (hullinfo: hull, box, 49 intervals -- the same expressions, written by k_linesearch / k_hullinfo) is
// valid for this robot; taking the record from there is ONE memory latency where recomputing costs two plus the projections.
// True in the iteration chains of the multi-robot modes, false in the stage API (the cache is rebuilt after this stage there).
// publish (coupled chain, Dev::xf_all; implies !use_cache): the unit also leaves the hull-cache record of its (robot, segment) -- what k_hullinfo would -- written through,
// and counts itself done on the segment's counter: the pair tiles of this launch wait for it
// FA (asynchronous front, Dev::fa_seq; implies publish): this launch runs next to the k_linesearch that commits the control net -- the unit fetches what does not depend
// on the net (its basis row, the top BVH boxes), waits for the robot's commit flag, reads the net past the caches (two robots' nets share cache lines) and forms the
// hull with hull_entry's sums in their order (same bits); everything it leaves for later kernels is written through (k_front's block then counts itself done).
template <int PRIM, bool FA = false>
__device__ __forceinline__ void obs_query_body(const Dev& D, int bid, double* lds, bool use_cache, bool publish = false) {
  const int u = D.u0 + bid / D.S, tr = bid % D.S;
  const int lane = lane_id();
  auto sti = [&](int* p, int v) { if constexpr (FA) xf_store_i(p, v); else *p = v; };
  double* P = lds + OBS_P; double* klo = lds + OBS_KLO; double* khi = lds + OBS_KHI;
  KdopLane kl;
  const double* net = D.spline + (size_t)u * 3 * D.T;
  TJ_TIC(D, K_SEP_OBS, 0);
  QBox q;
  const TopBox topb = bvh_top_box(D);   // travels with the segment's record
  if (use_cache && D.multi()) {
    const double* h = hull_record(D, u, tr);
    if (lane < 18) P[lane] = h[lane];
    if (lane < 49) { klo[lane] = h[HULL_KLO + lane]; khi[lane] = h[HULL_KHI + lane]; }
#pragma unroll
    for (int k = 0; k < 3; k++) { q.lo[k] = h[HULL_BOX + k]; q.hi[k] = h[HULL_BOX + 3 + k]; }
  } else {
    if constexpr (FA) {
      double bk[6] = {0, 0, 0, 0, 0, 0};
      const int e = min(lane, 17);
      const double* B = hull_row(D, tr, e / 3);
#pragma unroll
      for (int k = 0; k < 6; k++) bk[k] = B[k];
      const double* col = hull_col(D, net, tr, e % 3);
      fa_wait_flag(D, D.fa_commit(u), D.fa_seq);
      TJ_TIC(D, K_SEP_OBS, 6);
      if (lane < 18) P[lane] = hull_sum(bk, col, xf_load);
    } else
    if (lane < 18) P[lane] = hull_entry(D, net, tr, lane / 3, lane % 3);
    __syncthreads();
    if (lane < 49) { double lo, up; hull_kdop_axis(D, P, lane, lo, up); klo[lane] = lo; khi[lane] = up; }
#pragma unroll
    for (int k = 0; k < 3; k++) hull_box_axis(P, k, q.lo[k], q.hi[k]);
  }
  __syncthreads();
  if (publish) {   // the record's values are at hand (every lane holds the box, the intervals are in LDS)
    hull_record_put<true>(D, u, tr, lane, P[min(lane, 17)], lane == 0 ? q.lo[0] : (lane == 1 ? q.lo[1] : q.lo[2]), lane == 0 ? q.hi[0] : (lane == 1 ? q.hi[1] : q.hi[2]), klo[min(lane, 48)], khi[min(lane, 48)]);
    xf_signal(D, 0, tr);
  }
  TJ_TIC(D, K_SEP_OBS, 1);
  const double dist = D.offset + D.margin;
  const size_t seg = (size_t)u * D.S + tr;
  int* list = D.ocand + seg * D.cap_obs;
  int base = 0;
  unsigned long long visits = 0;
  const int found = bvh_query<4, PRIM>(D, q, dist, WalkScratch::carve(lds + OBS_WALK), &visits, [&](int pt) {
    typename PrimOf<PRIM>::Body qb;
    const bool ok = kl.template cull<PRIM>(D, klo, khi, pt, dist, lane, qb);
    const unsigned long long mask = ballot(ok);
    const int idx = base + prefix_count(mask);
    if (ok) {
      if (idx < D.cap_obs) sti(list + idx, pt);
      else atomicOr(&D.ctl->error, ERR_PLANE_OVERFLOW);
    }
    base += __popcll(mask);
  }, &topb);
  TJ_TIC(D, K_SEP_OBS, 4);
  const int cnt = min(base, D.cap_obs);
  if (cnt > 0 && lane < 18) { if constexpr (FA) xf_store(D.ohull + seg * 18 + lane, P[lane]); else D.ohull[seg * 18 + lane] = P[lane]; }   // read by the solve waves of this segment's candidates only
  // Work items: a segment with few candidates hands each one to its own wave (cooperative GJK, lowest latency); a
  // segment in a dense part of the cloud hands them over in batches of up to 64, one candidate per lane (per-lane GJK,
  // highest throughput): ObsItem.
  const bool batched = cnt > OBS_SINGLE_MAX;
  const int items = batched ? (cnt + 63) / 64 : cnt;
  int w0 = 0;
  if (lane == 0) {
    sti(D.ocand_n + seg, cnt);
    if (items > 0) w0 = atomicAdd(D.obs_work_n, items);
    unsigned long long* st = D.seg_stats + seg * 6;   // fire-and-forget atomics instead of a read-modify-write round trip
    atomicAdd(&st[0], visits); atomicAdd(&st[1], (unsigned long long)found);
  }
  w0 = __shfl(w0, 0);
  for (int i = lane; i < items; i += 64) { sti(D.obs_work + 2 * (size_t)(w0 + i), (int)seg); sti(D.obs_work + 2 * (size_t)(w0 + i) + 1, obs_item_slot(batched, i)); }
  TJ_TIC(D, K_SEP_OBS, 5);
}

// Separate::opengjk (Separate.h:18-163) for one candidate, by one wave
// FA (asynchronous front, Dev::fa_mid): the k_front whose lists this body reads ended while THIS launch was already running -- everything of it is read past the caches
template <int PRIM, bool FA = false>
__device__ __forceinline__ void obs_solve_body(const Dev& D, int bid, int nwaves) {
  const int lane = lane_id();
  __shared__ double P[18];
  auto ldi = [&](const int* p) { if constexpr (FA) return xf_load_i(p); else return *p; };
  const int n = ldi(D.obs_work_n);
  const double dist = D.offset + D.margin;
  const int epoch = D.ctl->epoch;
  for (int w = bid; w < n; w += nwaves) {
    const ObsItem it = obs_item(ldi(D.obs_work + 2 * (size_t)w), ldi(D.obs_work + 2 * (size_t)w + 1));
    __syncthreads();
    if (lane < 18) { if constexpr (FA) P[lane] = xf_load(D.ohull + (size_t)it.seg * 18 + lane); else P[lane] = D.ohull[(size_t)it.seg * 18 + lane]; }
    __syncthreads();
    const int mine = it.batch ? it.first + lane : it.first;            // candidate of this lane
    const bool live = !it.batch || mine < ldi(D.ocand_n + it.seg);
    const int pt = ldi(D.ocand + (size_t)it.seg * D.cap_obs + (live ? mine : it.first));
    const typename PrimOf<PRIM>::Body qb = PrimOf<PRIM>::load(D, pt);
    V3 v;
    if (it.batch) v = gjk(BodyHull{P}, qb);                            // one candidate per lane
    else v = gjk_wave(BodyHull{P}, qb, lane);                          // one candidate for the whole wave
    double c0, c1, c2, dd;
    if (plane_from_witness_body(v, qb, dist, D.offset, c0, c1, c2, dd) && live && (it.batch || lane == 0)) obs_plane_store(D, obs_plane_slot(D, it.seg, mine), c0, c1, c2, dd, epoch);
  }
}

template <int PRIM>
__global__ __launch_bounds__(64) void k_obs_query(Dev D) {
  if (TJ_DONE(D)) return;
  __shared__ double lds[OBS_LDS_DOUBLES];
  obs_query_body<PRIM>(D, blockIdx.x, lds, false);
}
template <int PRIM>
__global__ __launch_bounds__(64) void k_obs_solve(Dev D) {
  if (TJ_DONE(D)) return;
  obs_solve_body<PRIM>(D, blockIdx.x, gridDim.x);
}

}  // namespace tj
