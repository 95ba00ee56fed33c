// kernels_debug.h -- known-answer entry points: run the SAME device functions the hot-path kernels
// use (gjk, plane_from_witness_body, plane_pair, the k-DOP cull and comparison, swept-hull CCD predicates, chol / min-eig) on
// caller-supplied batches, one case per lane (or per workgroup for the LDS linear algebra), so the
// parity tests can compare them bit-for-bit against vectors produced by the reference
// (tests/golden/gjk_kat.npz, prims_kat.npz).
#pragma once
#include "dev_common.h"
#include "dev_linalg.h"
#include "kernels_sep.h"
#include "kernels_pairs.h"
#include "dev_optplane.h"

namespace tj {

template <int K>
struct BodyPts {  // K explicit points, row-major [K][3]
  const double* p;
  static constexpr int N = K;
  __device__ __forceinline__ V3 get(int i) const { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
};

template <int K1, int K2>
__global__ __launch_bounds__(64) void k_dbg_gjk(int n, const double* a, const double* b, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 v = gjk(BodyPts<K1>{a + (size_t)i * 3 * K1}, BodyPts<K2>{b + (size_t)i * 3 * K2});
  out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z;
}

// wave-cooperative variant (gjk_wave): one case per workgroup = one wavefront
template <int K1, int K2>
__global__ __launch_bounds__(64) void k_dbg_gjk_wave(int n, const double* a, const double* b, double* out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const V3 v = gjk_wave(BodyPts<K1>{a + (size_t)i * 3 * K1}, BodyPts<K2>{b + (size_t)i * 3 * K2}, lane_id());
  if (threadIdx.x == 0) { out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z; }
}
// gjk_wave interrupted after k_stop iterations, its state taken through memory (per case 32 doubles of `scratch`: the 20 doubles, then the ints) with the head start's own
// gjk_state_pack / gjk_state_unpack (kernels_pairs.h: the layout the product ships) and the loop continued from there: out = witness vector, iterations
template <int K1, int K2>
__global__ __launch_bounds__(64) void k_dbg_gjk_wave_split(int n, const double* a, const double* b, int k_stop, double* scratch, double* out) {
  static_assert(SPEC_STATE_DOUBLES * sizeof(double) + SPEC_STATE_INTS * sizeof(int) <= 32 * sizeof(double), "a case's state fits its 32 doubles of scratch");
  const int i = blockIdx.x;
  if (i >= n) return;
  const int lane = lane_id();
  const BodyPts<K1> ba{a + (size_t)i * 3 * K1}; const BodyPts<K2> bb{b + (size_t)i * 3 * K2};
  GjkState st; bool fin;
  V3 v = gjk_wave_run(ba, bb, lane, st, true, k_stop, fin);
  double* sd = scratch + (size_t)i * 32; int* si = (int*)(sd + SPEC_STATE_DOUBLES);
  if (lane == 0) gjk_state_pack<false>(st, fin, sd, si);
  __threadfence();
  __syncthreads();
  if (!fin) {
    GjkState r; bool fin1;
    gjk_state_unpack<false>(sd, si, lane, r, fin1);
    bool fin2;
    v = gjk_wave_run(ba, bb, lane, r, false, 50, fin2);
    st.k = r.k;
  }
  if (threadIdx.x == 0) { out[4 * i] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = (double)st.k; }
}
// plane_pair_wave: one robot pair per wavefront (the form k_sep_self_solve uses)
__global__ __launch_bounds__(64) void k_dbg_pair_wave(Dev D, int n, const double* P, const double* Q, double dist, double* out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  __shared__ double A[18], B[18];
  if (threadIdx.x < 18) { A[threadIdx.x] = P[(size_t)i * 18 + threadIdx.x]; B[threadIdx.x] = Q[(size_t)i * 18 + threadIdx.x]; }
  __syncthreads();
  double e0 = 0, e1 = 0, e2 = 0, dpl = 0; bool capped;
  const bool ok = plane_pair_wave(A, B, dist, D.margin, D.offset, lane_id(), e0, e1, e2, dpl, capped);
  if (threadIdx.x == 0) { double* o = out + (size_t)i * 5; o[0] = ok; o[1] = e0; o[2] = e1; o[3] = e2; o[4] = dpl; }
}

// what: 0 hull / point plane as obs_solve_body's batch path forms it -> out[5] = ok,c,d ; 1 plane_pair(P,Q) with Newton refine -> ok,c,d ;
//       3 k-DOP hull/hull: both hulls' intervals by hull_kdop_axis and kdop_apart, the arithmetic of pair_tile_filter (out[0] = pass)   (2, hull / point: k_dbg_kdop_wave)
__global__ __launch_bounds__(64) void k_dbg_planes(Dev D, int what, int n, const double* P, const double* Q, double dist, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* p = P + (size_t)i * 18;
  double* o = out + (size_t)i * 5;
  if (what == 0) {
    const BodyPoint q{V3{Q[3 * i], Q[3 * i + 1], Q[3 * i + 2]}};
    double c0 = 0, c1 = 0, c2 = 0, dd = 0;
    const bool ok = plane_from_witness_body(gjk(BodyHull{p}, q), q, dist, D.offset, c0, c1, c2, dd);
    o[0] = ok; o[1] = c0; o[2] = c1; o[3] = c2; o[4] = dd;
  } else if (what == 1) {
    double e0 = 0, e1 = 0, e2 = 0, dpl = 0; bool capped;
    const bool ok = plane_pair(p, Q + (size_t)i * 18, dist, D.margin, D.offset, true, e0, e1, e2, dpl, capped);
    o[0] = ok; o[1] = e0; o[2] = e1; o[3] = e2; o[4] = dpl;
  } else if (what == 3) {
    bool sep = false;
    for (int k = 0; k < 49; k++) {
      double alo, ahi, blo, bhi;
      hull_kdop_axis(D, p, k, alo, ahi); hull_kdop_axis(D, Q + (size_t)i * 18, k, blo, bhi);
      sep = sep | kdop_apart(alo, ahi, blo, bhi, dist);
    }
    o[0] = !sep;
  } else if (what == 5) {  // Optimal_plane::optimal_cd: o[1..4] = (c, d) in/out, o[0] = finished within the iteration caps
    double cx = o[1], cy = o[2], cz = o[3], d = o[4];
    o[0] = opt_plane_obstacle(p, Q[3 * i], Q[3 * i + 1], Q[3 * i + 2], D.margin, D.offset, cx, cy, cz, d);
    o[1] = cx; o[2] = cy; o[3] = cz; o[4] = d;
  } else {                 // Optimal_plane::self_optimal_cd
    double cx = o[1], cy = o[2], cz = o[3], d = o[4];
    o[0] = opt_plane_pair(p, Q + (size_t)i * 18, D.margin, D.offset, cx, cy, cz, d);
    o[1] = cx; o[2] = cy; o[3] = cz; o[4] = d;
  }
}

// Optimal_plane::self_optimal_cd by one wavefront per plane (opt_plane_pair_wave, the form k_keep uses for short lists)
__global__ __launch_bounds__(64) void k_dbg_optpair_wave(Dev D, int n, const double* P, const double* Q, double* out) {
  const int i = blockIdx.x;
  if (i >= n) return;
  double* o = out + (size_t)i * 5;
  double cx = o[1], cy = o[2], cz = o[3], d = o[4];
  __shared__ double te64[64];
  const bool ok = opt_plane_pair_wave(P + (size_t)i * 18, Q + (size_t)i * 18, D.margin, D.offset, lane_id(), cx, cy, cz, d, te64);
  if (lane_id() == 0) { o[0] = ok; o[1] = cx; o[2] = cy; o[3] = cz; o[4] = d; }
}

// swept-hull CCD predicates at steps (t1,u1): out[0] = GJKCCD(P,D,q), out[1] = SelfGJKCCD(P,D,Q,E)
__global__ __launch_bounds__(64) void k_dbg_ccd(int n, const double* P, const double* Dd, const double* Q, const double* E, const double* q, const double* tu, double d, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t1 = tu[2 * i], u1 = tu[2 * i + 1];
  const V3 v = gjk(BodySwept{P + (size_t)i * 18, Dd + (size_t)i * 18, t1}, BodyPoint{V3{q[3 * i], q[3 * i + 1], q[3 * i + 2]}});
  out[2 * i] = (v.x * v.x + v.y * v.y + v.z * v.z <= d * d);
  const V3 w = gjk(BodySwept{P + (size_t)i * 18, Dd + (size_t)i * 18, t1}, BodySwept{Q + (size_t)i * 18, E + (size_t)i * 18, u1});
  out[2 * i + 1] = (w.x * w.x + w.y * w.y + w.z * w.z <= d * d);
}

// triangle obstacle bodies (BASELINE config 5), one case per lane: out[i][8] = plane ok, c, d (hull P vs triangle, distance
// dist) | o[5], o[6]: the two k-DOP verdicts, left to k_dbg_kdop_wave | GJK CCD hit at off
__global__ __launch_bounds__(64) void k_dbg_tri(Dev D, int n, const double* P, const double* Dd, const double* tri, const double* t, double dist, double off, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* p = P + (size_t)i * 18; const double* dd = Dd + (size_t)i * 18; const double* q = tri + (size_t)i * 9;
  const BodyTri tb{V3{q[0], q[1], q[2]}, V3{q[3], q[4], q[5]}, V3{q[6], q[7], q[8]}};
  double* o = out + (size_t)i * 8;
  double c0 = 0, c1 = 0, c2 = 0, pd = 0;
  const bool ok = plane_from_witness_body(gjk(BodyHull{p}, tb), tb, dist, D.offset, c0, c1, c2, pd);
  o[0] = ok; o[1] = c0; o[2] = c1; o[3] = c2; o[4] = pd;
  const V3 v = gjk(BodySwept{p, dd, t[i]}, tb);
  o[7] = (v.x * v.x + v.y * v.y + v.z * v.z <= off * off);
}

// The obstacle k-DOP cull in the product's form, one wave per case: kdop_cull_wave (lanes over the axes, candidates by readlane) on the hull's intervals from
// hull_kdop_axis -- SWEPT: of conv{P, P + t D} from swept_kdop_axis, the swept record's --, `per` candidates (bodies[n][per][PRIM][3]) of which the first nc[i]
// (nc == nullptr: all) sit on the lanes; out[(i * per + j) * ostride] = candidate j's verdict
template <int PRIM, bool SWEPT>
__global__ __launch_bounds__(64) void k_dbg_kdop_wave(Dev D, int n, const double* P, const double* Dd, const double* t, const double* bodies, int per, const int* nc, double d, double* out, int ostride) {
  const int i = blockIdx.x, lane = lane_id();
  if (i >= n) return;
  __shared__ double H[18], PS[18];
  if (lane < 18) {
    H[lane] = P[(size_t)i * 18 + lane];
    if constexpr (SWEPT) PS[lane] = H[lane] + t[i] * Dd[(size_t)i * 18 + lane];
  }
  __syncthreads();
  const int ax = min(lane, 48);
  const V3 axv{D.kdop[3 * ax], D.kdop[3 * ax + 1], D.kdop[3 * ax + 2]};
  double lo, hi;
  if constexpr (SWEPT) swept_kdop_axis(axv, H, PS, lo, hi); else hull_kdop_axis(D, H, ax, lo, hi);
  const int m = nc ? min(nc[i], per) : per;
  const double* b = bodies + ((size_t)i * per + min(lane, per - 1)) * 3 * PRIM;
  typename PrimOf<PRIM>::Body qb;
  if constexpr (PRIM == 1) qb = BodyPoint{V3{b[0], b[1], b[2]}}; else qb = BodyTri{V3{b[0], b[1], b[2]}, V3{b[3], b[4], b[5]}, V3{b[6], b[7], b[8]}};
  const bool pass = kdop_cull_wave(qb, m, axv, lo, hi, d, lane);
  if (lane < m) out[((size_t)i * per + lane) * ostride] = pass;
}

// broad-phase known answers: one wavefront per caller-supplied query box, raw candidate list (sorted primitive indices,
// traversal order) of aabb::Tree::query(box, margin) (AABB.cc:608-667) on the static BVH.  The walk in each of the forms the product kernels instantiate:
// BQ_UNROLL 4 (k_front) or 1 (k_ccd, the audit, the seeds, the planner); PRE: the lane's top-level box fetched ahead of the query box and handed in (k_front, k_ccd)
template <int PRIM, int BQ_UNROLL, bool PRE>
__global__ __launch_bounds__(64) void k_dbg_query(Dev D, int nq, const double* boxes, double m, int cap, int* out_ids, int* out_n) {
  const int b = blockIdx.x;
  if (b >= nq) return;
  __shared__ int walk[WalkScratch::INTS];
  TopBox topb{};
  if constexpr (PRE) topb = bvh_top_box(D);
  QBox q;
  for (int k = 0; k < 3; k++) { q.lo[k] = boxes[6 * (size_t)b + k]; q.hi[k] = boxes[6 * (size_t)b + 3 + k]; }
  int base = 0;
  unsigned long long visits = 0;
  bvh_query<BQ_UNROLL, PRIM>(D, q, m, WalkScratch::carve(walk), &visits, [&](int pt) {
    const bool ok = pt >= 0;
    const unsigned long long mask = ballot(ok);
    const int idx = base + prefix_count(mask);
    if (ok && idx < cap) out_ids[(size_t)b * cap + idx] = pt;
    base += __popcll(mask);
  }, PRE ? &topb : nullptr);
  if (lane_id() == 0) out_n[b] = base;
}

// one workgroup per matrix: out[2*i] = LLT fails, out[2*i+1] = smallest eigenvalue
__global__ __launch_bounds__(64) void k_dbg_linalg(int nmat, int n, const double* mats, double* out) {
  extern __shared__ double sm[];
  double* A = sm; double* W = A + n * n; double* scr = W + n * n;
  const int tid = threadIdx.x;
  const double* src = mats + (size_t)blockIdx.x * n * n;
  for (int i = tid; i < n * n; i += 64) { A[i] = src[i]; W[i] = src[i]; }
  __syncthreads();
  bool ok = chol_lds(W, n, tid, 64);
  __syncthreads();
  bool agree = true;
  double r[19];
  const int row = min(tid, 18);
  if (n == 19) {  // the register variants k_grad uses must give the same verdict / the same bits
#pragma unroll
    for (int c = 0; c < 19; c++) r[c] = A[row * 19 + c];
    agree = chol_check_wave<19>(r) == ok;
#pragma unroll
    for (int c = 0; c < 19; c++) r[c] = A[row * 19 + c];
  }
  const double ev = min_eig_lds(A, n, scr, scr + n, scr + 2 * n, scr + 3 * n, tid, 64);
  if (n == 19) {   // the register copy fuses its products: same algorithm, agreement to rounding level of the matrix norm
    double nrm = 0;
    for (int i = 0; i < 361; i++) nrm = fmax(nrm, fabs(src[i]));
    agree = agree && fabs(min_eig_wave<19>(r, tid) - ev) <= 1e-13 * fmax(nrm, 1e-300);
  }
  if (tid == 0) { out[2 * blockIdx.x] = !agree ? 2.0 : ok ? 0.0 : 1.0; out[2 * blockIdx.x + 1] = ev; }
}

}  // namespace tj
