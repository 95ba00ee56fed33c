// kernels_pairs.h -- inter-robot separating planes.
//
// Replaces separate_self (Optimization3D_multi.h:237-342): BVH::SelfDCDCollision (BVH.cpp:252-287,
// a fresh dynamic AABB tree per segment), CCD::SelfKDOPDCD (CCD.h:535-587), Separate::selfgjk
// (Separate.h:165-304) and Optimal_plane::optimal_d (Optimal_plane.h:13-71).
//
//   k_hullinfo          per (robot, segment): hull, its AABB and its 49 k-DOP intervals, once.
//   k_sep_self_rows     one wavefront per (segment, lower robot p0): lanes over partners p1 > p0 for
//                       the box test; lanes over the 49 AXES for each box survivor (interval
//                       comparisons straight from the cache, no dot products, two coalesced loads
//                       per lane); pairs that pass go to a work list.
//   k_sep_self_solve    one wavefront per listed pair, solved cooperatively by its lanes (wave-cooperative
//                       GJK, the 12 barrier terms of the offset Newton on 12 lanes: plane_pair_wave).
//                       Each unordered pair is solved ONCE and
//                       the plane is stored for both robots, (c, d - off/2) and (-c, -d - off/2),
//                       in a dense [segment][robot][partner] slot table stamped with the current
//                       epoch (no clearing pass): pair_plane_store.
//                       sep_self_solve_body (also k_mid's pair waves) dispatches a wave to one of five regimes:
//                       pair_early_head_start (asynchronous front: a head-start pair solved under k_front's
//                       tail), pair_consumer / pair_lane_producer (large fleets: one pair per lane, long solves
//                       passed on to idle waves), pair_dedicated (a head-start pair continued from its saved
//                       GJK state), pair_generic (a static share of the list, a wave per pair).
//   k_sep_self_compact  per (robot, segment): the obstacle planes from the stamped candidate slots (slot order), then
//                       the stamped partner slots in ascending partner order into the robot's plane lists --
//                       deterministic order, no atomics.
// The per-segment tree of the reference is replaced by the all-pairs box test (U <= a few hundred):
// the pair SET is what matters, and it is defined by the same inclusive overlap predicate
// (AABB.cc:131-148).
#pragma once
#include "dev_common.h"
#include "dev_linalg.h"
#include "kernels_sep.h"

namespace tj {

__global__ __launch_bounds__(64) void k_hullinfo(Dev D) {
  if (TJ_DONE(D)) return;
  const int u = blockIdx.x / D.S, tr = blockIdx.x % D.S, lane = lane_id();
  __shared__ double P[18];
  if (lane < 18) P[lane] = hull_entry(D, D.spline + (size_t)u * 3 * D.T, tr, lane / 3, lane % 3);
  __syncthreads();
  hull_record_store<false>(D, u, tr, lane, P);
}

// One unit of the robot-pair broad phase = one wavefront = a TILE of the (lower robot p0, partner p1 > p0) triangle of one
// segment: R consecutive rows p0 (R = Dev::pair_rows: 2, 4, 8 or 16) against one aligned block of 64 partners.  A row per wave
// (round 1) and then a 64-partner chunk of a row per wave (35 680 one-wave workgroups per launch at 256 robots) were bound by
// workgroup dispatch and by one memory latency per handful of box tests; a tile loads the 64 partner boxes ONCE for R rows,
// and 25 440 units become 1 600.  Tiles of a segment: row blocks grouped by the column block g that holds their diagonal
// (rows [64g, 64g+64)); a row block of group g meets column blocks g .. nc-1.
__host__ __device__ inline int pair_units(int U, int R) {
  const int nc = (U + 63) / 64;
  int n = 0;
  for (int g = 0; 64 * g < U - 1; g++) { const int rows = min(64 * g + 64, U - 1) - 64 * g; n += ((rows + R - 1) / R) * (nc - g); }
  return n;
}
__host__ __device__ inline void pair_unit(int U, int R, int bid, int& tr, int& rb, int& cb) {
  const int per = pair_units(U, R), nc = (U + 63) / 64;
  tr = bid / per;
  int r = bid % per;
  rb = 0; cb = 0;
  for (int g = 0; 64 * g < U - 1; g++) {
    const int rows = min(64 * g + 64, U - 1) - 64 * g;
    const int cnt = ((rows + R - 1) / R) * (nc - g);
    if (r < cnt) { rb = 64 * g + (r / (nc - g)) * R; cb = 64 * (g + r % (nc - g)); return; }
    r -= cnt;
  }
}
constexpr int PAIR_CONSUMERS_MAX = 4096;            // bound on the waves that wait for passed-on pairs (all idle pair waves do: with 512 of them k_mid took 74 us on SCN-D, with 864 65)
constexpr unsigned long long PAIR_OVF_STOP = 1ull << 31;   // entry flag: the list ends here
constexpr int PAIR_LANE_GJK_CAP = 3;   // GJK iterations a lane spends on its pair before passing it on (large fleets, see sep_self_solve_body; 2 .. 4 measured alike, 8 slower)
constexpr int PT_FLIGHT = 8;   // pairs whose interval records a tile fetches together
constexpr int PAIR_ROWS_MAX = 16;
constexpr int PAIR_TILE_CAP = PAIR_ROWS_MAX * 64;

// The pair work list is S sub-lists, one per segment: sub-list tr occupies slots [tr * cap_seg, (tr + 1) * cap_seg) of pair_work
// and has its own counter pair_work_n[tr] (pair_work_n[S] is the cursor of the solve waves).  One global counter was hit by
// ~8 000 producer waves per iteration at 256 robots, and same-address atomics serialise (each waits for its return value):
// the plane stage of k_front was bound by that, not by its work.  Consumers index the concatenation: wprefix() leaves the
// exclusive prefix of the (clamped) counts in LDS, wslot() maps an item number to its slot.
__device__ __forceinline__ int pair_work_cap_seg(const Dev& D) { return D.cap_work / D.S; }
template <bool FA = false>   // FA: the counts were written while this launch was running (asynchronous front, Dev::fa_mid): read past the caches
__device__ __forceinline__ int pair_work_prefix(const Dev& D, int* pre, int lane) {   // one wave; pre[0..S]; returns the total
  const int S = D.S, cap = pair_work_cap_seg(D);
  int run = 0;
  for (int base = 0; base < S; base += 64) {
    const int tr = base + lane;
    const int c = tr < S ? min(FA ? xf_load_i(D.pair_work_n + tr) : D.pair_work_n[tr], cap) : 0;
    int x = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off); if (lane >= off) x += y; }
    if (tr < S) pre[tr] = run + x - c;
    run += __shfl(x, 63);
  }
  if (lane == 0) pre[S] = run;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
  return run;
}
__device__ __forceinline__ int pair_work_slot(const Dev& D, const int* pre, int w) {
  int lo = 0, hi = D.S;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pre[mid] <= w) lo = mid; else hi = mid; }
  return lo * pair_work_cap_seg(D) + (w - pre[lo]);
}

// Broad phase of one tile, shared by the plane stage (hull boxes / hull intervals) and the CCD selection (swept boxes / swept
// intervals).  Box test: lanes over the 64 partners (their boxes in registers, loaded once), loop over the R rows (boxes
// broadcast from LDS); hits are appended to list[] as (p0 << 16 | p1) in (p0, p1) order.  Then, per box survivor, lanes over the
// 49 axes against both robots' interval records; the records of FOUR pairs are fetched together -- the loop is a chain of
// memory latencies, not of arithmetic -- and the list is compacted in place.  The two comparisons are kernels_sep.h's box_near and
// kdop_apart, the ones of the one-pair-at-a-time forms (CCD.h:535-587), hence the same decisions.  Returns the number of pairs left in list[].
//   segbox  [6][U] lo.xyz, hi.xyz of every robot for this segment      rec(q) -> robot q's record, intervals lo at LO, hi at HI
//   [own0, own1): robots of this rank -- a pair is skipped unless it touches one (sharded contexts; pass 0, U otherwise)
template <bool FA = false, class RecOf>   // FA (asynchronous front): boxes and records were written (through) by blocks of a kernel that runs at the same time -- read past the caches
__device__ __forceinline__ int pair_tile_filter(const double* segbox, int U, int rb, int R, int cb, int own0, int own1, RecOf rec, int LO, int HI, double d,
                                                double* rowbox, int* list, int lane) {
  auto ldd = [&](const double* p) { if constexpr (FA) return xf_load(p); else return *p; };
  for (int i = lane; i < R * 6; i += 64) rowbox[i] = ldd(segbox + (size_t)(i % 6) * U + min(rb + i / 6, U - 1));
  const int p1 = cb + lane;
  const int pc = min(p1, U - 1);
  double bv[6];
#pragma unroll
  for (int k = 0; k < 6; k++) bv[k] = ldd(segbox + (size_t)k * U + pc);   // independent loads, no branch between them
  const bool own1p = p1 >= own0 && p1 < own1;
  blk_sync<true>();
  int n = 0;
  for (int r = 0; r < R; r++) {
    const int p0 = rb + r;
    if (p0 >= U - 1) break;   // uniform
    const bool listed = p1 < U && p1 > p0 && (own1p || (p0 >= own0 && p0 < own1));
    const bool hit = listed & box_near(bv, bv + 3, rowbox + 6 * r, rowbox + 6 * r + 3, d);
    const unsigned long long mask = ballot(hit);
    if (hit) list[n + prefix_count(mask)] = (p0 << 16) | p1;
    n += __popcll(mask);
  }
  blk_sync<true>();
  if (n == 0) return 0;
  const int ax = min(lane, 48);
  int m = 0;
  for (int base = 0; base < n; base += PT_FLIGHT) {
    int pr[PT_FLIGHT]; double alo[PT_FLIGHT], ahi[PT_FLIGHT], blo[PT_FLIGHT], bhi[PT_FLIGHT];
#pragma unroll
    for (int c = 0; c < PT_FLIGHT; c++) pr[c] = list[min(base + c, n - 1)];
#pragma unroll
    for (int c = 0; c < PT_FLIGHT; c++) {
      const double* a = rec(pr[c] >> 16); const double* b = rec(pr[c] & 0xffff);
      alo[c] = ldd(a + LO + ax); ahi[c] = ldd(a + HI + ax); blo[c] = ldd(b + LO + ax); bhi[c] = ldd(b + HI + ax);
    }
    blk_sync<true>();   // every lane has read this batch's list entries before the compaction overwrites earlier slots
#pragma unroll
    for (int c = 0; c < PT_FLIGHT; c++) {
      if (base + c >= n) break;
      const bool sep = lane < 49 && kdop_apart(alo[c], ahi[c], blo[c], bhi[c], d);
      if (ballot(sep) == 0ull) {
        if (lane == 0) list[m] = pr[c];
        m++;
      }
    }
  }
  blk_sync<true>();
  return m;
}

constexpr int PAIR_LDS_DOUBLES = PAIR_ROWS_MAX * 6 + PAIR_TILE_CAP / 2;   // rowbox | list
template <bool FA = false>   // FA (asynchronous front): the work items go out written through
__device__ __forceinline__ void sep_self_rows_body(const Dev& D, int bid, double* lds, bool wait_xf = false) {
  int tr, rb, cb;
  pair_unit(D.U, D.pair_rows, bid, tr, rb, cb);
  const int lane = lane_id();
  const int U = D.U;
  double* rowbox = lds; int* list = (int*)(lds + PAIR_ROWS_MAX * 6);
  const double dist = D.offset + 2 * D.margin;
  if (wait_xf) xf_wait_seg(D, 0, tr);   // sharded contexts (union kernel): the hull cache of the other ranks' robots is written by units at the head of this launch
  const int m = pair_tile_filter<FA>(D.hbox + (size_t)tr * 6 * U, U, rb, D.pair_rows, cb, D.u0, D.u1,   // (FA: boxes and interval records read past the caches -- a box line holds sixteen robots' entries, written by sixteen units)
                                 [&](int q) { return hull_record(D, q, tr); }, HULL_KLO, HULL_KHI, dist, rowbox, list, lane);
  if (m == 0) return;
  // hand the remaining pairs to the solve stage (k_mid / k_sep_self_solve): one work item per pair.  Solving them here,
  // one lane per pair, serialises up to 63 divergent GJK paths in one wave where many robots meet (measured: 87 us).
  int base = 0;
  if (lane == 0) base = atomicAdd(D.pair_work_n + tr, m);   // the segment's own counter
  base = __shfl(base, 0);
  const int cap = pair_work_cap_seg(D);
  for (int i = lane; i < m; i += 64) {
    const int w = base + i;
    if (w < cap) {
      const size_t sl = (size_t)tr * cap + w;
      if constexpr (FA) { xf_store_i(D.pair_work + 3 * sl, tr); xf_store_i(D.pair_work + 3 * sl + 1, list[i] >> 16); xf_store_i(D.pair_work + 3 * sl + 2, list[i] & 0xffff); }
      else { D.pair_work[3 * sl] = tr; D.pair_work[3 * sl + 1] = list[i] >> 16; D.pair_work[3 * sl + 2] = list[i] & 0xffff; }
    }
    else atomicOr(&D.ctl->error, ERR_PAIR_OVERFLOW);
  }
}

// ---- GJK head start ------------------------------------------------------------------------------------------------------
// Once the work list is spread evenly (sep_self_solve_body), k_mid is as long as its slowest robot pair: a pair of stacked hulls
// whose GJK takes 10 - 16 iterations of ~1.3 us while the machine idles; k_front in front of it lasts ~10 us whatever the pairs
// do.  In the steady phase of a run the slow pairs are the same from one iteration to the next (tests/devtools/
// gjk_persistence.py: 17 of 18 on SCN-C; in the first twenty iterations one to two thirds), and a GJK query is a pure function
// of the two hulls, which are final when k_front starts (hull cache).  So: k_mid lists the pairs whose query took at least
// max(SPEC_GJK_MIN, longest of the previous launch - SPEC_GJK_WINDOW) iterations; the next k_front carries SPEC_CAP extra
// one-wave blocks at the head of its grid, block b runs the first SPEC_GJK_BUDGET iterations of entry b's query (three: the
// blocks then end with the obstacle queries) and stores the loop state (GjkState, 20 doubles + 9 ints) under a tag (epoch, pair);
// wave b of k_mid is dedicated to entry b and continues the same loop at t = 0 of that kernel.  Same instructions on the same
// operands in the same order: the witness vector and the iteration count are those of an uninterrupted query (test: head start
// on / off, bitwise).  A listed pair that left the broad phase costs two waves that publish nothing; the list's order is free.
constexpr int SPEC_CAP = 128, SPEC_GJK_MIN = 5, SPEC_GJK_WINDOW = 10, SPEC_GJK_BUDGET = 3;
constexpr int SPEC_STATE_DOUBLES = 20, SPEC_STATE_INTS = 16;

// ---- a robot pair, its key and the words built from the key -- each stated once ----------------------------------------------
struct PairId { int tr, p0, q; };   // segment, lower robot, its partner (q > p0)
constexpr int PAIR_KEY_TR_BITS = 9, PAIR_KEY_ROBOT_BITS = 11;   // 9 + 11 + 11 bits; bit 31 stays free (PAIR_OVF_STOP)
__device__ __forceinline__ unsigned pair_key(const PairId& id) { return (unsigned)(id.tr | (id.p0 << PAIR_KEY_TR_BITS) | (id.q << (PAIR_KEY_TR_BITS + PAIR_KEY_ROBOT_BITS))); }
__device__ __forceinline__ PairId pair_unkey(unsigned key) {
  constexpr unsigned mt = (1u << PAIR_KEY_TR_BITS) - 1u, mr = (1u << PAIR_KEY_ROBOT_BITS) - 1u;
  return PairId{(int)(key & mt), (int)((key >> PAIR_KEY_TR_BITS) & mr), (int)((key >> (PAIR_KEY_TR_BITS + PAIR_KEY_ROBOT_BITS)) & mr)};
}
__device__ __forceinline__ bool pair_id_valid(const Dev& D, const PairId& id) { return id.tr < D.S && id.p0 < D.U && id.q < D.U; }   // (a key of this context's own lists always is)
// a 64-bit word that says which iteration it belongs to: the epoch in the upper half, and in the lower a pair's key (head-start tag, passed-on pair), SPEC_KEY_NONE
// or PAIR_OVF_STOP.  Readers poll until the upper half shows their epoch: no word is ever cleared.
constexpr unsigned SPEC_KEY_NONE = 0xffffffffu;   // asynchronous front: "this entry's block has run for the epoch in the upper half and has no pair" (a plain 0 could be a tag not written yet)
__device__ __forceinline__ unsigned long long pair_tag_word(int epoch, unsigned long long low) { return ((unsigned long long)(unsigned)epoch << 32) | low; }

// The published plane of a solved pair: (c, d - off/2) in robot p0's slot for partner q and (-c, -d - off/2) in q's slot for p0 of the dense
// [segment][robot][partner] table, both stamped with the epoch and marked in the rows' index words -- the five writers (three regimes of the pair solve below,
// two of k_keep) call this.  live = false (k_keep only: a refinement that returned NaN) publishes the inert form c = 0, d = huge in both slots instead.
// WT: written through (k_keep's asynchronous part: read by k_grad's compaction on another queue, possibly before the launch has ended).
template <bool WT = false>
__device__ __forceinline__ void pair_plane_store(const Dev& D, const PairId& id, double c0, double c1, double c2, double d, int epoch, bool live = true) {
  const int U = D.U;
  const double off = D.offset;
  const size_t s0 = ((size_t)id.tr * U + id.p0) * U + id.q, s1 = ((size_t)id.tr * U + id.q) * U + id.p0;
  double* q0 = D.pairplane + 4 * s0; double* q1 = D.pairplane + 4 * s1;
  auto put = [](double* p, double v) { if constexpr (WT) xf_store(p, v); else *p = v; };
  put(q0, live ? c0 : 0.0); put(q0 + 1, live ? c1 : 0.0); put(q0 + 2, live ? c2 : 0.0); put(q0 + 3, live ? d - 0.5 * off : 1e300);
  put(q1, live ? -c0 : 0.0); put(q1 + 1, live ? -c1 : 0.0); put(q1 + 2, live ? -c2 : 0.0); put(q1 + 3, live ? -d - 0.5 * off : 1e300);
  if constexpr (WT) { xf_store_i(&D.pairstamp[s0], epoch); xf_store_i(&D.pairstamp[s1], epoch); }
  else { D.pairstamp[s0] = epoch; D.pairstamp[s1] = epoch; }
  D.pair_mark(id.tr, id.p0, id.q); D.pair_mark(id.tr, id.q, id.p0);
}

// ---- a pair's two hulls, staged for one wave: lanes 0..17 hold the entries of A (robot p0's hull), lanes 18..35 those of B (robot q's) ------------------------
__device__ __forceinline__ void pair_hull_put(double* A, double* B, int lane, double v) { if (lane < 18) A[lane] = v; else if (lane < 36) B[lane - 18] = v; }
// this lane's entry from the hull records (FA: read past the caches)
template <bool FA>
__device__ __forceinline__ double pair_hull_fetch(const Dev& D, const PairId& id, int lane) {
  if (lane >= 36) return 0.0;
  const double* p = hull_record(D, lane < 18 ? id.p0 : id.q, id.tr) + (lane < 18 ? lane : lane - 18);
  if constexpr (FA) return xf_load(p); else return *p;
}
// ... and from the control nets, where the records of this iteration are not (yet) to be had: the operands of this lane's hull_sum.  A caller that must wait for
// the nets copies the basis row into registers BEFORE the wait and reads the net after it.
struct PairHullSrc { const double* row; const double* col; };
__device__ __forceinline__ PairHullSrc pair_hull_src(const Dev& D, const PairId& id, int lane) {
  const int r = lane < 18 ? id.p0 : id.q, e = min(lane < 18 ? lane : lane - 18, 17);
  return PairHullSrc{hull_row(D, id.tr, e / 3), hull_col(D, D.spline + (size_t)r * 3 * D.T, id.tr, e % 3)};
}

// ---- the saved state of a wave-cooperative GJK query (GjkState, 20 doubles + 8 ints, and whether the query had finished): ONE field table for the writer
// (spec_pair_body), the reader (spec_state_load) and the known-answer kernel (k_dbg_gjk_wave_split) ------------------------------------------------------------
constexpr int GJK_STATE_FIN = 8;   // index of the `finished` flag among the ints
template <class St, class FD, class FI>
__device__ __forceinline__ void gjk_state_fields(St& st, FD&& fd, FI&& fi) {
  fd(0, st.v.x); fd(1, st.v.y); fd(2, st.v.z);
  fd(3, st.s.v0.x); fd(4, st.s.v0.y); fd(5, st.s.v0.z); fd(6, st.s.v1.x); fd(7, st.s.v1.y); fd(8, st.s.v1.z);
  fd(9, st.s.v2.x); fd(10, st.s.v2.y); fd(11, st.s.v2.z); fd(12, st.s.v3.x); fd(13, st.s.v3.y); fd(14, st.s.v3.z);
  fd(15, st.s.l0); fd(16, st.s.l1); fd(17, st.s.l2); fd(18, st.s.l3); fd(19, st.wmax2);
  fi(0, st.s.n); fi(1, st.s.w0); fi(2, st.s.w1); fi(3, st.s.w2); fi(4, st.s.w3); fi(5, st.c1); fi(6, st.c2); fi(7, st.k);
}
// one lane stores (WT: written through)
template <bool WT>
__device__ __forceinline__ void gjk_state_pack(const GjkState& st, bool fin, double* sd, int* si) {
  auto puti = [&](int i, int v) { if constexpr (WT) xf_store_i(si + i, v); else si[i] = v; };
  gjk_state_fields(st, [&](int i, double v) { if constexpr (WT) xf_store(sd + i, v); else sd[i] = v; }, puti);
  puti(GJK_STATE_FIN, fin ? 1 : 0);
}
// the whole wave fetches (one load per lane, then broadcasts).  The values go straight back into vector registers: left in scalar ones (50 of them, live across
// the merge with the fresh query's start) they cost k_mid a stack frame.
__device__ __forceinline__ double spec_bcast(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  int vlo, vhi;
  asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=v"(vlo), "=v"(vhi) : "s"(lo), "s"(hi));
  return __hiloint2double(vhi, vlo);
}
template <bool FA>   // FA: read past the caches
__device__ __forceinline__ void gjk_state_unpack(const double* sd, const int* si, int lane, GjkState& st, bool& fin) {
  const double* px_ = sd + min(lane, SPEC_STATE_DOUBLES - 1);
  const int* py_ = si + (lane & (SPEC_STATE_INTS - 1));
  const double x = FA ? xf_load(px_) : *px_;
  const int y = FA ? xf_load_i(py_) : *py_;
  gjk_state_fields(st, [&](int i, double& f) { f = spec_bcast(x, i); }, [&](int i, int& f) { f = __builtin_amdgcn_readlane(y, i); });
  fin = __builtin_amdgcn_readlane(y, GJK_STATE_FIN) != 0;
}
template <bool FA = false>
__device__ __forceinline__ void spec_state_load(const Dev& D, int b, int lane, GjkState& st, bool& fin) {   // the state head-start entry b holds
  gjk_state_unpack<FA>(D.spec_state + (size_t)b * SPEC_STATE_DOUBLES, D.spec_sti + (size_t)b * SPEC_STATE_INTS, lane, st, fin);
}

// FA (asynchronous front): the launch runs next to the k_linesearch that commits the control nets -- the epoch is the begun iteration's (fa_early_begin's record, the
// control block still shows the running one), the block waits for its two robots' commit flags and forms the hulls from the nets read past the caches, and what
// it leaves for k_mid goes out written through.
template <bool FA = false>
__device__ __forceinline__ void spec_pair_body(const Dev& D, int b, double* lds, int fa_epoch = 0) {
  __builtin_amdgcn_s_setprio(3);   // the longest blocks of the launch, on SIMDs they share with four or five query waves
  const int lane = lane_id();
  const int epoch = FA ? fa_epoch : D.ctl->epoch, par = epoch & 1;
  auto tag_out = [&](unsigned long long v) { if constexpr (FA) __hip_atomic_store(D.spec_tag + b, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else D.spec_tag[b] = v; };
  const unsigned long long no_pair = FA ? pair_tag_word(epoch, SPEC_KEY_NONE) : 0ull;
  if (b == 0 && lane == 0) { if constexpr (FA) xf_store_i(D.spec_n + par, 0); else D.spec_n[par] = 0; }   // the list this iteration's k_mid fills
  const int n = min(D.spec_n[par ^ 1], SPEC_CAP);
  // every block leaves a tag, valid or not: the tags k_mid sees are always those of the k_front in front of it
  if (b >= n) { if (lane == 0) tag_out(no_pair); return; }
  const unsigned key = (unsigned)D.spec_list[(par ^ 1) * SPEC_CAP + b];
  const PairId id = pair_unkey(key);
  if (!pair_id_valid(D, id)) { if (lane == 0) tag_out(no_pair); return; }   // (cannot happen: the list is this context's own)
  const double* A = hull_record(D, id.p0, id.tr);
  const double* B = hull_record(D, id.q, id.tr);
  if constexpr (FA) {   // the records are written by this launch's obstacle units (later in the grid: not waited for): the two hulls from the nets, behind the robots' commit flags, read past the caches
    const PairHullSrc src = pair_hull_src(D, id, lane);
    double bk[6];
#pragma unroll
    for (int k = 0; k < 6; k++) bk[k] = src.row[k];
    fa_wait_flag(D, D.fa_commit(id.p0), D.fa_seq);
    fa_wait_flag(D, D.fa_commit(id.q), D.fa_seq);
    if (lane < 36) lds[lane] = hull_sum(bk, src.col, xf_load);
    blk_sync<true>();
    A = lds; B = lds + 18;
  } else
  if (D.xf_all || D.fa_units) {   // coupled chain: the records are being written by this launch's obstacle units (LATER in the grid: not waited for) -- the two hulls straight from the control nets
    if (lane < 36) { const PairHullSrc src = pair_hull_src(D, id, lane); lds[lane] = hull_sum(src.row, src.col); }
    blk_sync<true>();
    A = lds; B = lds + 18;
  } else if (D.xf && (id.p0 < D.u0 || id.p0 >= D.u1 || id.q < D.u0 || id.q >= D.u1)) xf_wait_seg(D, 0, id.tr);   // sharded contexts: a hull of another rank's robot comes from this launch's foreign units
  GjkState st; bool fin;
  gjk_wave_run(BodyHull{A}, BodyHull{B}, lane, st, true, D.spec_budget, fin);
  if (lane == 0) gjk_state_pack<FA>(st, fin, D.spec_state + (size_t)b * SPEC_STATE_DOUBLES, D.spec_sti + (size_t)b * SPEC_STATE_INTS);
  if constexpr (FA) sig_acked();   // asynchronous front: the dedicated wave of k_mid polls the TAG and then reads the state -- the state is in memory before the tag goes out
  if (lane == 0) tag_out(pair_tag_word(epoch, key));
  if constexpr (FA) sig_sent();
}

__global__ __launch_bounds__(64) void k_sep_self_rows(Dev D) {
  if (TJ_DONE(D)) return;
  __shared__ double lds[PAIR_LDS_DOUBLES];
  sep_self_rows_body(D, blockIdx.x, lds);
}

// ---- the pair solve: one wavefront per launched wave `bid` of `nwaves`, five regimes -------------------------------------------------------------------------
//   pair_early_head_start   (asynchronous front) a dedicated wave solves its head-start pair under k_front's tail, before the work list exists
//   pair_consumer           large fleets: an idle wave takes the pairs the lane producers pass on, one at a time, wave-cooperatively
//   pair_lane_producer      large fleets: one pair per LANE, a chunk of the work list per wave
//   pair_dedicated          wave b continues head-start entry b from its saved GJK state and publishes if the broad phase listed the pair again
//   pair_generic            a static share of the work list, one pair after the other, wave-cooperatively
// sep_self_solve_body decides which of them a wave runs.  A[18], B[18] (the staged hulls), wpre (the work list's prefix) and the tile are single buffers the
// dispatcher owns and hands down: function-local __shared__ arrays of exclusive branches would add up (see OBS_LDS_DOUBLES).
constexpr int PAIR_TILE_LANES = 32, PAIR_TILE_DOUBLES = 36 * PAIR_TILE_LANES;   // the lane producers' tile (pair_lane_producer)
struct PairSolve { bool ok, capped; double c0, c1, c2, d; int newton, gjk; };   // ok: the hulls are within range and (c, d) is their plane; capped: the offset Newton hit its cap; iteration counts
// plane_pair_wave for the staged pair (whole wave, uniform result).  resume: the query's first iterations were run elsewhere and gs holds their state
__device__ __forceinline__ PairSolve pair_solve_wave(const Dev& D, const double* A, const double* B, int lane, GjkState& gs, bool resume, bool resume_finished, const Dev* tic = nullptr) {
  PairSolve r{false, false, 0, 0, 0, 0, 0, 0};
  r.ok = plane_pair_wave(A, B, D.offset + 2 * D.margin, D.margin, D.offset, lane, r.c0, r.c1, r.c2, r.d, r.capped, &r.newton, &r.gjk, tic, gs, resume, resume_finished);
  return r;
}
// what a wave leaves of a solved pair (lane 0): the launch's longest query, the statistics, the plane
__device__ __forceinline__ void pair_result_store(const Dev& D, const PairId& id, const PairSolve& r, int epoch, int lane) {
  if (lane == 0 && r.gjk >= 6) atomicMax(&D.ctl->gjk_max, r.gjk);   // a handful of pairs per launch
  if (r.ok && lane == 0) {
    // statistics per (robot, segment): ~900 waves adding to ONE word of the control block serialise there (~13 ns each) and
    // the stores below wait for it
    unsigned long long* ps = D.pair_stats + 2 * ((size_t)id.p0 * D.S + id.tr);
    atomicAdd(ps, (unsigned long long)r.newton); atomicAdd(ps + 1, 1ull);
    if (r.capped) atomicOr(&D.ctl->error, ERR_LOOP_CAP);
    pair_plane_store(D, id, r.c0, r.c1, r.c2, r.d, epoch);
  }
}
// a query of at least spec_thr iterations (a few dozen pairs per launch) is a candidate for the next iteration's head start (list: k_mid only)
__device__ __forceinline__ void pair_note_slow(const Dev& D, const PairId& id, int gk, int epoch, int lane, bool list, int spec_thr) {
  if (lane == 0 && list && gk >= spec_thr) {
    const int slot = atomicAdd(&D.spec_n[epoch & 1], 1);
    if (slot < SPEC_CAP) D.spec_list[(epoch & 1) * SPEC_CAP + slot] = (int)pair_key(id);
  }
#ifdef TJ_PHASE_TIMING
  if (lane == 0 && gk >= 4) {   // (key, iterations) of the slower queries of this launch: tests/devtools/gjk_persistence.py
    long long* base = D.dbg + (size_t)K_SEP_SELF_ROWS * TJ_TIC_BLOCKS * TJ_TIC_SLOTS;
    const unsigned long long i = atomicAdd((unsigned long long*)base, 1ull);
    if (i < 4000) { base[8 + 2 * i] = (long long)pair_key(id); base[9 + 2 * i] = gk; }
  }
#endif
}

// Asynchronous front (FA): this launch started while k_front still runs.  A wave that may be DEDICATED to a head-start entry does not wait for k_front's end to begin: it
// polls its entry's tag (the entry's k_front block leaves it behind its acknowledged state -- a few microseconds after the pair's two robots have committed), and runs the
// rest of the pair's GJK and the offset Newton at once, from the saved state and the two hulls formed from the committed control nets (hull_sum: the records' bits).
// Only then does it wait -- like every other solve wave -- for k_front's end, to see whether the broad phase listed the pair again, and publishes (pair_dedicated).  The
// slow pairs of the previous iteration, which set this kernel's length, thus run under k_front's tail.  Returns whether entry b had a pair; r is its solve, A / B stay staged.
__device__ __forceinline__ bool pair_early_head_start(const Dev& D, int b, int lane, double* A, double* B, PairSolve& r) {
  const int epoch_now = D.ctl->epoch;
  unsigned long long tg = 0;
  if (!poll_until<4>([&] { tg = __hip_atomic_load(D.spec_tag + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return (int)(tg >> 32) == epoch_now; }, WAIT_2S)) {
    wait_failed(D, ERR_LOOP_CAP | ERR_XS_TIMEOUT);
    tg = pair_tag_word(epoch_now, SPEC_KEY_NONE);
  }
  const unsigned key = (unsigned)tg;
  const PairId id = pair_unkey(key);
  if (key == SPEC_KEY_NONE || !pair_id_valid(D, id)) return false;
  __builtin_amdgcn_s_setprio(3);
  if (lane < 36) { const PairHullSrc src = pair_hull_src(D, id, lane); pair_hull_put(A, B, lane, hull_sum(src.row, src.col, xf_load)); }
  GjkState hs; bool hs_fin = false;
  spec_state_load<true>(D, b, lane, hs, hs_fin);
  __syncthreads();
  r = pair_solve_wave(D, A, B, lane, hs, true, hs_fin);
  __builtin_amdgcn_s_setprio(0);
  return true;
}

// Long work list (hundreds of robots): a wave per pair is the lowest LATENCY but occupies 64 lanes for one chain of
// dependent steps; with thousands of pairs THROUGHPUT decides, and one pair per LANE (per-lane GJK + Newton, the same
// arithmetic: plane_pair == plane_pair_wave bit for bit) is ~20x cheaper per pair.  The switch is wave-uniform.
// Almost every pair is through after one or two GJK iterations, a few dozen per iteration need 10-16 (measured on the
// 256-robot scene: 98 % <= 2, 0.2 % >= 10) -- and a wave is as slow as its slowest lane, at ~2.8 us per per-lane iteration:
// 45 us of a lone lane with the rest of the machine idle.  When the list leaves at least half of the launched waves
// without a chunk, the lanes stop after PAIR_LANE_GJK_CAP iterations and pass an unfinished pair on (one 64-bit word
// tagged with the iteration's epoch, appended to a device-wide list); the idle waves take these pairs one each and solve
// them from the start with the wave-cooperative form, which reaches the same bits (plane_pair == plane_pair_wave).
// Cross-wave traffic is agent-scope atomics only, and every waiting wave polls a word of its OWN (consumer c takes the
// entries c, c + nc, ...): ~900 waves polling shared counters serialise at the memory side (~13 ns per access to one
// address) and starve the producers -- measured.  The producer that counts itself done last writes nc STOP entries behind
// the list, so every consumer's next word turns valid.  An append's returning add has been performed before its wave
// counts itself done; no fence (= no L2 write-back) is needed anywhere.
struct PairLanePlan { int lpw, np, nc; bool pass_on; };   // pairs (= active lanes) per producer wave, producer waves, consumer waves, whether long solves are passed on
__device__ __forceinline__ PairLanePlan pair_lane_plan(const Dev& D, int n, int nwaves) {
  const int lpw = min(D.pair_lpw, PAIR_TILE_LANES);   // (TJ_PAIR_LPW; 64 .. 8 lanes measured alike without the tile)
  const int np = min(nwaves, (n + lpw - 1) / lpw);      // waves that own a chunk of the list ("producers")
  return PairLanePlan{lpw, np, min(nwaves - np, PAIR_CONSUMERS_MAX), D.pair_pass_on && 2 * np <= nwaves};
}
// consumer c of pl.nc: the long solves, one per wave
template <bool FA>
__device__ __forceinline__ void pair_consumer(const Dev& D, int c, const PairLanePlan& pl, int nwaves, int epoch, int lane, double* A, double* B) {
  const int nc = pl.nc;
  if (c >= nc) return;
  TJ_TIC(D, K_SEP_SELF_SOLVE, 0);
  long long t_end = 0;   // one deadline for every entry of this wave: 5 ms + 1 us per launched wave
  for (int i = c;; i += nc) {
    unsigned long long e = 0;
    if (i >= D.cap_work + PAIR_CONSUMERS_MAX) return;
    const bool have = poll_until<16>([&] { e = __hip_atomic_load(&D.pair_ovf_list[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return (int)(e >> 32) == epoch; },
                                     t_end, WAIT_5MS + WAIT_SLACK * nwaves);
    if (!have) wait_failed(D, ERR_LOOP_CAP | ERR_PASS_TIMEOUT);
    if (!have || (e & PAIR_OVF_STOP)) { TJ_TIC(D, K_SEP_SELF_SOLVE, 2); return; }
    if (i == c) TJ_TIC(D, K_SEP_SELF_SOLVE, 1);
    const PairId id = pair_unkey((unsigned)e);
    __syncthreads();
    pair_hull_put(A, B, lane, pair_hull_fetch<FA>(D, id, lane));
    __syncthreads();
    GjkState gs;
    pair_result_store(D, id, pair_solve_wave(D, A, B, lane, gs, false, false), epoch, lane);
  }
}
// producer: lanes over a chunk of the work list, every lane its own pair.
// tile: PAIR_TILE_DOUBLES doubles of LDS in which every lane keeps its pair's two hulls, transposed (entry e of lane l at tile[e * PAIR_TILE_LANES + l]: conflict-free).
// The per-lane GJK and the offset Newton read a hull entry dozens of times; from global memory that was 36 scattered 8-byte loads per lane and GJK iteration -- the
// producers' GJK phase took 4 ... 58 us depending on what else the memory pipeline was doing (phase stamps, round 5), from LDS it does not depend on it.
template <bool FA>
__device__ __forceinline__ void pair_lane_producer(const Dev& D, int bid, int nwaves, int n, const PairLanePlan& pl, int epoch, int lane, const int* wpre, double* tile) {
  auto ldi = [&](const int* p) { if constexpr (FA) return xf_load_i(p); else return *p; };
  auto ldd = [&](const double* p) { if constexpr (FA) return xf_load(p); else return *p; };
  const double dist = D.offset + 2 * D.margin, m = D.margin, off = D.offset;
  const int lpw = pl.lpw, kcap = pl.pass_on ? PAIR_LANE_GJK_CAP : 50;
  unsigned long long nit_sum = 0, solved = 0; bool any_capped = false;
  TJ_TIC(D, K_SEP_SELF_SOLVE, 0);
  if (D.pair_prio) __builtin_amdgcn_s_setprio(3);   // the ~160 producer waves set k_mid's length at hundreds of robots: ahead of whatever shares their SIMD (TJ_PAIR_PRIO)
  for (int base = bid * lpw; base < n; base += nwaves * lpw) {
    const int w = base + lane;
    if (w < n && lane < lpw) {
      const size_t sl = (size_t)pair_work_slot(D, wpre, w);
      const PairId id{ldi(D.pair_work + 3 * sl), ldi(D.pair_work + 3 * sl + 1), ldi(D.pair_work + 3 * sl + 2)};
      const double* Ag = hull_record(D, id.p0, id.tr);
      const double* Bg = hull_record(D, id.q, id.tr);
      constexpr int hst = PAIR_TILE_LANES;
      {   // this lane's column of the tile (private to the lane: no synchronisation)
        double* col = tile + lane;
#pragma unroll 6
        for (int e = 0; e < 18; e++) { col[e * hst] = ldd(Ag + e); col[(18 + e) * hst] = ldd(Bg + e); }
        Ag = col; Bg = col + 18 * hst;
      }
      double e0, e1c, e2c, dpl; bool capped; int nit = 0;
      int gkl = 0; bool cut = false;
      const V3 vw = gjk(BodyHullT<hst>{Ag}, BodyHullT<hst>{Bg}, &gkl, kcap, &cut);
#ifdef TJ_PHASE_TIMING
      if (!cut) atomicAdd((unsigned long long*)&D.dbg[((size_t)K_SEP_SELF_ROWS * TJ_TIC_BLOCKS + min(gkl, 63)) * TJ_TIC_SLOTS], 1ull);   // histogram of GJK iterations per pair (lane path)
#endif
      TJ_ORDER(vw.x); TJ_TIC(D, K_SEP_SELF_SOLVE, 1);
      if (!cut && gkl >= 6) atomicMax(&D.ctl->gjk_max, gkl);
      if (cut) {   // pass the pair on NOW (the consumers start while this wave's other lanes refine their offsets): slot from a returning add, then the tagged entry
        const int slot = atomicAdd(&D.pair_ovf[0], 1);
        if (slot < D.cap_work) __hip_atomic_store(&D.pair_ovf_list[slot], pair_tag_word(epoch, pair_key(id)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else atomicOr(&D.ctl->error, ERR_PAIR_OVERFLOW);   // cannot happen (the list holds cap_work entries and there are at most that many pairs); never drop a pair silently
      }
      if (!cut && plane_pair_finish(vw, Ag, Bg, dist, m, off, true, e0, e1c, e2c, dpl, capped, &nit, hst)) {
        nit_sum += (unsigned long long)nit; solved++; any_capped = any_capped || capped;
        pair_plane_store(D, id, e0, e1c, e2c, dpl, epoch);
      }
    }
  }
  TJ_TIC(D, K_SEP_SELF_SOLVE, 3);
  if (pl.pass_on) {   // this producer's appends have all been performed (their adds returned); the last producer closes the list
    int last = 0;
    if (lane == 0) last = atomicAdd(&D.pair_ovf[1], 1) == pl.np - 1;
    if (__shfl(last, 0)) {
      const int cnt = min(__hip_atomic_load(&D.pair_ovf[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), D.cap_work);
      for (int j = lane; j < pl.nc; j += 64) __hip_atomic_store(&D.pair_ovf_list[cnt + j], pair_tag_word(epoch, PAIR_OVF_STOP), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (int o = 32; o > 0; o >>= 1) { nit_sum += __shfl_xor(nit_sum, o); solved += __shfl_xor(solved, o); }
  if (lane == 0 && solved) { unsigned long long* ps = D.pair_stats + 2 * (size_t)(bid % (D.U * D.S)); atomicAdd(ps, nit_sum); atomicAdd(ps + 1, solved); }
  if (any_capped) atomicOr(&D.ctl->error, ERR_LOOP_CAP);
}

// ---- one wave per pair -------------------------------------------------------------------------------------------------
// SCN-C lists ~3 000 pairs per iteration for 1 024 - 1 728 waves: a wave solves two or three, and what it pays per pair besides
// the arithmetic (2 - 6 us) were three dependent memory round trips (cursor -> work item -> hulls, ~0.9 us each: the lines were
// written by another XCD a kernel earlier).  So the assignment is STATIC (wave r of the Wg generic waves takes the items r,
// r + Wg, ...; at most five, n <= 4 nwaves here): lane j fetches the work item of the wave's j-th pair, all of them in one
// round trip, and the hulls of the next pair travel while the current one is solved.
// The pairs that were slow in the previous iteration do not wait in that queue: wave b of the first SPEC_CAP waves is
// DEDICATED to head-start entry b (spec_pair_body) -- it needs the tag only to know its pair, starts at t = 0
// from the saved GJK state, and publishes the plane if the broad phase listed the pair again (its segment's part of the work
// list is scanned while the GJK runs); the generic wave that meets the pair in the list skips it.
// At most half of the launched waves are dedicated (an entry beyond that stays with the generic wave that meets it in the list), so
// the generic waves are never fewer than nwaves / 2 and a wave's share of the list stays <= 8 items whatever TJ_N_SOLVE / TJ_HS_MIN say.
// The head-start tags as every solve wave holds them: lane l the tags of entries l and 64 + l (SPEC_CAP = 128: two per lane); v0 / v1: the entry's k_front block ran for
// this epoch, had a pair, and the entry has a dedicated wave; m0 / m1: the ballots of v0 / v1
struct SpecTags {
  unsigned long long t0, t1, m0, m1; bool v0, v1;
  __device__ __forceinline__ int count() const { return __popcll(m0) + __popcll(m1); }
  __device__ __forceinline__ bool dedicated(int b) const { return b < SPEC_CAP && (((b < 64 ? m0 >> b : m1 >> (b - 64)) & 1ull) != 0); }
  __device__ __forceinline__ unsigned key_of(int b) const { return (unsigned)(b < 64 ? __shfl(t0, b) : __shfl(t1, b - 64)); }
  __device__ __forceinline__ int below(int b) const {   // dedicated waves in front of wave b
    return b < 64 ? __popcll(m0 & ((1ull << b) - 1ull)) : (b < 128 ? __popcll(m0) + __popcll(m1 & ((1ull << (b - 64)) - 1ull)) : count());
  }
  __device__ __forceinline__ bool holds(unsigned long long want) const { return ballot((v0 && t0 == want) || (v1 && t1 == want)) != 0ull; }   // a dedicated wave has this pair
};
__device__ __forceinline__ SpecTags spec_tags(unsigned long long t0, unsigned long long t1, bool head_start, int epoch, int n_ded, int lane) {
  const bool v0 = head_start && (int)(t0 >> 32) == epoch && (unsigned)t0 != SPEC_KEY_NONE && lane < n_ded, v1 = head_start && (int)(t1 >> 32) == epoch && (unsigned)t1 != SPEC_KEY_NONE && 64 + lane < n_ded;
  return SpecTags{t0, t1, ballot(v0), ballot(v1), v0, v1};
}
// wave b, dedicated to head-start entry b with pair `key`.  have_early: the pair was solved under k_front's tail (pair_early_head_start: `early`, A / B staged)
template <bool FA>
__device__ __forceinline__ void pair_dedicated(const Dev& D, int b, unsigned key, bool have_early, const PairSolve& early, bool head_start, int spec_thr, int epoch, int lane,
                                               double* A, double* B, const int* wpre) {
  auto ldi = [&](const int* p) { if constexpr (FA) return xf_load_i(p); else return *p; };
  __builtin_amdgcn_s_setprio(3);   // k_mid's tail: ahead of whatever shares the SIMD
  TJ_TIC(D, K_SEP_SELF_SOLVE, 0);
  const PairId id = pair_unkey(key);
  if (!pair_id_valid(D, id)) return;   // (cannot happen)
  // in flight together: both hulls, the saved state, this segment's part of the work list
  GjkState hs; bool hs_fin = false;
  if (!have_early) {
    pair_hull_put(A, B, lane, pair_hull_fetch<FA>(D, id, lane));
    spec_state_load<FA>(D, b, lane, hs, hs_fin);
  }
  const int cnt = wpre[id.tr + 1] - wpre[id.tr];
  const int* wl = D.pair_work + 3 * (size_t)id.tr * pair_work_cap_seg(D);
  bool member = false;
  for (int i = lane; i < cnt; i += 64) member = member || (ldi(wl + 3 * i + 1) == id.p0 && ldi(wl + 3 * i + 2) == id.q);
  __syncthreads();
  TJ_TIC(D, K_SEP_SELF_SOLVE, 1);
  PairSolve r = early;
  if (!have_early) r = pair_solve_wave(D, A, B, lane, hs, true, hs_fin);
#ifdef TJ_PHASE_TIMING
  if (lane == 0 && blockIdx.x < TJ_TIC_BLOCKS) { D.dbg[((size_t)K_SEP_SELF_SOLVE * TJ_TIC_BLOCKS + blockIdx.x) * TJ_TIC_SLOTS + 6] = r.gjk + 1000; D.dbg[((size_t)K_SEP_SELF_SOLVE * TJ_TIC_BLOCKS + blockIdx.x) * TJ_TIC_SLOTS + 7] = r.ok ? r.newton : -1; }
#endif
  if (ballot(member)) {   // the broad phase listed the pair in this iteration too: the plane counts
    if (lane == 0) atomicAdd(&D.ctl->spec_taken, 1);
    pair_note_slow(D, id, r.gjk, epoch, lane, head_start, spec_thr);
    pair_result_store(D, id, r, epoch, lane);
  }
  TJ_TIC(D, K_SEP_SELF_SOLVE, 2);
}
// generic wave r of Wg: the work items r, r + Wg, ... of the n listed
template <bool FA>
__device__ __forceinline__ void pair_generic(const Dev& D, int r, int Wg, int n, const SpecTags& tags, bool head_start, int spec_thr, int epoch, int lane,
                                             double* A, double* B, const int* wpre) {
  auto ldi = [&](const int* p) { if constexpr (FA) return xf_load_i(p); else return *p; };
  if (r >= n) return;
  TJ_TIC(D, K_SEP_SELF_SOLVE, 0);
  // lane j: the wave's j-th work item (all of them in one round trip)
  int it_tr = 0, it_p0 = 0, it_q = 0;
  const int n_mine = (n - r + Wg - 1) / Wg;   // <= 8 (n <= 4 nwaves, Wg >= nwaves / 2)
  if (n_mine > 64) { if (lane == 0) atomicOr(&D.ctl->error, ERR_PAIR_OVERFLOW); return; }   // (cannot happen: a lane holds one item)
  if (lane < n_mine) {
    const size_t sl = (size_t)pair_work_slot(D, wpre, r + lane * Wg);
    it_tr = ldi(D.pair_work + 3 * sl); it_p0 = ldi(D.pair_work + 3 * sl + 1); it_q = ldi(D.pair_work + 3 * sl + 2);
  }
  auto item = [&](int j) { return PairId{__builtin_amdgcn_readlane(it_tr, j), __builtin_amdgcn_readlane(it_p0, j), __builtin_amdgcn_readlane(it_q, j)}; };
  PairId next = item(0);
  double hv = pair_hull_fetch<FA>(D, next, lane);
  for (int j = 0; j < n_mine; j++) {
    const bool first = j == 0;   // phase stamps (timing build only) describe a wave's first work item
    __syncthreads();
    pair_hull_put(A, B, lane, hv);
    __syncthreads();
    const PairId id = next;
    if (j + 1 < n_mine) {   // the next pair's hulls travel while this one is solved
      next = item(j + 1);
      hv = pair_hull_fetch<FA>(D, next, lane);
    }
    if (first) TJ_TIC(D, K_SEP_SELF_SOLVE, 1);
    if (head_start && tags.holds(pair_tag_word(epoch, pair_key(id)))) continue;   // a dedicated wave has this pair
    GjkState gs;
    const PairSolve s = pair_solve_wave(D, A, B, lane, gs, false, false,
#ifdef TJ_PHASE_LIGHT
                                        nullptr);
#else
                                        first ? &D : nullptr);
#endif
#ifdef TJ_PHASE_TIMING
    if (lane == 0 && first && blockIdx.x < TJ_TIC_BLOCKS) { D.dbg[((size_t)K_SEP_SELF_SOLVE * TJ_TIC_BLOCKS + blockIdx.x) * TJ_TIC_SLOTS + 6] = s.gjk; D.dbg[((size_t)K_SEP_SELF_SOLVE * TJ_TIC_BLOCKS + blockIdx.x) * TJ_TIC_SLOTS + 7] = s.ok ? s.newton : -1; }
#endif
    pair_note_slow(D, id, s.gjk, epoch, lane, head_start, spec_thr);
    pair_result_store(D, id, s, epoch, lane);
    if (first) TJ_TIC(D, K_SEP_SELF_SOLVE, 2);
  }
}

// FA (asynchronous front, Dev::fa_mid): the k_front of the same iteration ended while THIS launch was already running -- its work lists, head-start states and hull records are read past the caches
template <bool FA = false>
__device__ __forceinline__ void sep_self_solve_body(const Dev& D, int bid, int nwaves, bool head_start, double* tile) {   // head_start: k_mid only -- the k_front of the same iteration ran in front of it
  const int lane = lane_id();
  __shared__ double A[18], B[18];
  __shared__ int wpre[513];
  auto ldt = [&](const unsigned long long* p) { if constexpr (FA) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else return *p; };
  const int n_ded = min(nwaves / 2, SPEC_CAP);   // waves that may be dedicated to a head-start entry
  bool have_early = false; PairSolve early{false, false, 0, 0, 0, 0, 0, 0};
  if constexpr (FA) {
    if (head_start && bid < n_ded) have_early = pair_early_head_start(D, bid, lane, A, B, early);
    fa_wait_flag(D, D.fa_go(bid), D.fa_seq);   // k_front is through: its work lists, tags and records are complete (read past the caches below)
  }
  // the tags are issued first and used after the work list's prefix has arrived; the head-start list takes the pairs within SPEC_GJK_WINDOW iterations of the
  // previous launch's longest query, so that it holds the tail and not the first to report
  const unsigned long long spec_tag0 = head_start ? ldt(D.spec_tag + lane) : 0ull, spec_tag1 = head_start ? ldt(D.spec_tag + 64 + lane) : 0ull;
  const int spec_thr = head_start ? max(D.spec_min, D.ctl->gjk_prev - SPEC_GJK_WINDOW) : 0;
  const int n = pair_work_prefix<FA>(D, wpre, lane);
  const int epoch = D.ctl->epoch;
  if (n > 4 * nwaves) {   // large fleets: one pair per lane
    const PairLanePlan pl = pair_lane_plan(D, n, nwaves);
    if (pl.pass_on && bid >= pl.np) pair_consumer<FA>(D, bid - pl.np, pl, nwaves, epoch, lane, A, B);
    else pair_lane_producer<FA>(D, bid, nwaves, n, pl, epoch, lane, wpre, tile);
    return;
  }
  const SpecTags tags = spec_tags(spec_tag0, spec_tag1, head_start, epoch, n_ded, lane);
  if (tags.dedicated(bid)) pair_dedicated<FA>(D, bid, tags.key_of(bid), have_early, early, head_start, spec_thr, epoch, lane, A, B, wpre);
  else pair_generic<FA>(D, bid - tags.below(bid), nwaves - tags.count(), n, tags, head_start, spec_thr, epoch, lane, A, B, wpre);
}
__global__ __launch_bounds__(64) void k_sep_self_solve(Dev D) {
  if (TJ_DONE(D)) return;
  __shared__ double tile[PAIR_TILE_DOUBLES];
  sep_self_solve_body(D, blockIdx.x, gridDim.x, false, tile);
}

// per (owned robot, segment): obstacle planes from the stamped candidate slots (slot order), then -- multi-robot modes --
// the robot-pair planes from the stamped partner slots (ascending partner): deterministic lists, no atomics
// The loads are ordered so that the chain is three memory latencies long, not six: epoch, candidate count and the first 256
// partner stamps go out together; then the candidate stamps and the stamped partners' planes; then the candidates' planes.
// hand-over (k_grad's folded launch): besides the global lists the wave leaves its segment's planes -- the first `pst_cap` of each
// list -- and the two counts in LDS (pst_o / pst_s: [pst_cap][4], cnt: {obstacle planes, all planes}), so that the gradient that
// follows in the same block reads neither the counts nor the lists back from global memory; *fits is cleared if a list is longer.
__device__ __forceinline__ void compact_segment(const Dev& D, int u, int tr, int lane, double* pst_o = nullptr, double* pst_s = nullptr, int* cnt = nullptr, int pst_cap = 0, int* fits = nullptr) {   // one wave
  const int U = D.U, epoch = D.ctl->epoch;
  const size_t seg = (size_t)u * D.S + tr;
  const bool obs_part = !(D.optimal_plane && !D.multi());  // single-UAV "optimal_plane":1 -- k_keep wrote the obstacle plane list itself
  const bool pair_part = D.multi();
  const int n = obs_part ? D.ocand_n[seg] : 0;
  // the row's index words (Dev::pairbits): one per 64 partners, fetched with the candidate count -- the stamps and planes of the SET bits follow in the second trip
  const int W = (U + 63) >> 6;
  unsigned long long* bw = D.pairbits + ((size_t)tr * U + u) * W;
  unsigned long long wbits = 0;   // lane w: word w (W <= 32)
  if (pair_part && lane < W) wbits = bw[lane];
  double* outp = D.splanes + seg * D.cap_self * 4;
  int pbase = 0;
  if (pair_part) {
    for (int q0 = 0; q0 < U; q0 += 64) {
      const unsigned long long word = __shfl(wbits, q0 >> 6);
      if (word == 0ull) continue;   // (uniform) nobody stamped a slot of this chunk
      const int q = q0 + lane;
      const bool bit = (word >> lane) & 1ull;
      const size_t slot = ((size_t)tr * U + u) * U + min(q, U - 1);
      int st = 0; double v0 = 0, v1 = 0, v2 = 0, v3 = 0;
      if (bit && q < U) { st = D.pairstamp[slot]; const double* p = D.pairplane + 4 * slot; v0 = p[0]; v1 = p[1]; v2 = p[2]; v3 = p[3]; }   // stamp and plane in one trip
      const bool ok = bit && q < U && q != u && st == epoch;
      const unsigned long long mask = ballot(ok);
      const int idx = pbase + prefix_count(mask);
      if (ok) {
        if (idx < D.cap_self) {
          outp[4 * idx] = v0; outp[4 * idx + 1] = v1; outp[4 * idx + 2] = v2; outp[4 * idx + 3] = v3;
          if (pst_s && idx < pst_cap) { pst_s[4 * idx] = v0; pst_s[4 * idx + 1] = v1; pst_s[4 * idx + 2] = v2; pst_s[4 * idx + 3] = v3; }
        }
        else atomicOr(&D.ctl->error, ERR_PLANE_OVERFLOW);
      }
      pbase += __popcll(mask);
    }
    if (lane < W && wbits != 0ull) bw[lane] = 0ull;   // read: cleared for the next iteration (its writers run in a later kernel; this wave is the row's only reader)
  }
  if (obs_part) {
    double* out = D.oplanes + seg * D.cap_obs * 4;
    int base = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
      const int sl = s0 + lane, slc = min(sl, n - 1);
      const size_t slot = obs_plane_slot(D, seg, slc);
      const int stamp = D.ostamp[slot];
      const double* p = D.oraw + slot * 4;
      const double o0 = p[0], o1 = p[1], o2 = p[2], o3 = p[3];   // (issued with the stamp; the 64 candidate slots fetched with the first trip, whatever the count, measured slower)
      const bool ok = sl < n && stamp == epoch;
      const unsigned long long mask = ballot(ok);
      const int idx = base + prefix_count(mask);
      if (ok) {
        out[4 * idx] = o0; out[4 * idx + 1] = o1; out[4 * idx + 2] = o2; out[4 * idx + 3] = o3;
        if (pst_o && idx < pst_cap) { pst_o[4 * idx] = o0; pst_o[4 * idx + 1] = o1; pst_o[4 * idx + 2] = o2; pst_o[4 * idx + 3] = o3; }
      }
      base += __popcll(mask);
    }
    if (lane == 0) { D.ocount[seg] = base; atomicAdd(&D.seg_stats[seg * 6 + 4], (unsigned long long)base); }   // fire-and-forget
    if (cnt && lane == 0) { cnt[0] = base; if (base > pst_cap) *fits = 0; }
  } else if (cnt && lane == 0) *fits = 0;   // ("optimal_plane":1, single UAV: k_keep wrote the obstacle list itself -- the gradient reads it from global memory)
  if (pair_part && lane == 0) {
    D.scount[seg] = min(pbase, D.cap_self);
    atomicAdd(&D.seg_stats[seg * 6 + 5], (unsigned long long)pbase);
  }
  if (cnt && lane == 0) { const int ns = pair_part ? min(pbase, D.cap_self) : 0; cnt[1] = ns; if (ns > pst_cap) *fits = 0; }
}
__global__ __launch_bounds__(64) void k_sep_self_compact(Dev D) {
  if (TJ_DONE(D)) return;
  if (D.keep_async) keep_wait(D);   // (see k_grad)
  compact_segment(D, D.u0 + blockIdx.x / D.S, blockIdx.x % D.S, lane_id());
}

}  // namespace tj
