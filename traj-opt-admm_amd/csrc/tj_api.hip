// tj_api.hip -- host side of libtrajadmm.so: context, device memory, launch sequence of one ADMM
// iteration, and the C ABI declared in include/trajadmm.h.
//
// One iteration = the stage sequence of Optimization3D_multi::optimization_decouple
// (Optimization3D_multi.h:29-118) / Optimization3D_admm::optimization (Optimization3D_admm.h:29-67),
// enqueued with plain launches and no host synchronisation inside or between iterations: a linear chain on the context's
// stream, plus -- one context -- the Newton solve on a second stream next to the gradient kernel (Dev::xs_async, dev_common.h)
// and, inside a batch, the NEXT iteration's k_front on that stream next to the line search (Dev::fa).  A wait between the queues
// that runs out is healed, not reported (heal_check).  The stop test of the mains runs on the device (begin_body), so a converged problem turns the remaining launches into early-exit kernels.
//
// There is deliberately no CPU path in this file: every entry point either runs HIP kernels or
// fails with TJ_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/trajadmm.h"
#include "dev_common.h"
#include "host_tables.h"
#include "kernels_sep.h"
#include "kernels_pairs.h"
#include "kernels_keep.h"
#include "kernels_newton.h"
#include "kernels_step.h"
#ifdef TJ_KAT
#include "../../include/trajadmm_kat.h"
#include "kernels_debug.h"   // known-answer kernels: test build only (libtrajadmm_kat.so)
#endif
#include "kernels_plan.h"
#include "kernels_bvh.h"
#include "kernels_audit.h"
#include "kernels_audit_timed.h"
#include "kernels_closest.h"
#include "kernels_obstacle_approach.h"
#include "kernels_obstacle_windows.h"
#include "kernels_peak_dynamics.h"
#include "kernels_dynamics_windows.h"
#include "kernels_zone_windows.h"
#include "kernels_pair_approach.h"
#include "kernels_path_crossing.h"
#include "kernels_timing_margin.h"
#include "kernels_proximity.h"
#include "kernels_flight_profile.h"
#include "kernels_sight_windows.h"
#include "host_plan.h"
#include "host_launch.h"

using namespace tj;

#include <atomic>
// streams claimed by the contexts of this process whose kernels sleep across queues, per device (tj_create)
static std::atomic<int> g_async_queues[64];
static int hw_queue_budget() { const char* e = getenv("GPU_MAX_HW_QUEUES"); const int n = e ? atoi(e) : 4; return std::max(n, 2) - 1; }
// the budget's one door: n > 0 claims n queues of the device (false: no room and not forced -- nothing is taken), n < 0 hands them back
static bool queue_budget(int device, int n, bool forced = true) {
  std::atomic<int>& g = g_async_queues[std::min(std::max(device, 0), 63)];
  if (g.fetch_add(n) + n > hw_queue_budget() && n > 0 && !forced) { g.fetch_sub(n); return false; }
  return true;
}

// The cross-queue schedule of one context: the asynchronous Newton solve (Dev::xs_async) and front (Dev::fa) on stream2, the asynchronous plane refinement (Dev::keep_async) on
// stream3: the streams and the queue claim.  The pairing counters and flags that the launch sequence advances are SchedState's (host_launch.h, tj_ctx::ss).
struct CrossQueue {
  hipStream_t stream2 = nullptr, stream3 = nullptr;
  int hwq_claim = 0;   // hardware queues claimed out of the process's budget for contexts that sleep across queues (tj_create)
};
// The checkpoint a batch can be restored from (heal_check; the careful re-run of a coupled sharded group, tj_group_iterate), touched by checkpoint_take / _restore / _drop
// only.  Device half: the regions of `tab` and the control block, copied to an arena of tj_create (SchedState::ck_in_begin: taken by the next k_begin).  Host half: the flags that describe it.
struct Checkpoint { SnapRegion* tab = nullptr; int n = 0; Ctl* ctl = nullptr; bool begin_folded = false, maybe_deferred = false; int lsc_base = 0; };
// One device array of a context, declared once (device_arrays): its name, where its pointer lives, its element count and size, whether it is part of the checkpoint, and
// what tj_init_state fills it with (0: nothing).  tj_create allocates from the table, builds the checkpoint's region table from it and keeps it (tj_ctx::arrays); tj_init_state
// resets from it; every host copy or clear of a context array takes its bounds from it (array_clear, fetch, store, array_count).  No extent is written a second time.
constexpr int SNAP = 1;   // self-healing: what a batch's first state consists of (everything an iteration reads that an earlier iteration wrote and that is not rebuilt or re-stamped anyway)
constexpr int ZERO = 2, ONES = 4;   // tj_init_state: all-zero bytes / all-one bytes (ls_hist: -1, no line search yet; ls_tab: LS_TAB_EMPTY)
struct ArrayDecl { const char* name; void** slot; size_t n, elem; bool snap; int reset; };

// what a context holds for a row-listing query (tj_pair_approach, tj_path_crossings, tj_timing_margin; listed_run)
template <class Args, class Rec>
struct Listed { unsigned* mask = nullptr; int* wordoff = nullptr; int* n = nullptr; Args sized{}; Rec* out = nullptr; std::vector<void*> allocs; int cap = -1, mw = 0; };

// what a context holds for tj_proximity_windows (proximity_run): as Listed, with the row total
struct ProxHeld : Listed<ProxArgs, tj_proximity_row> { int* n_rows = nullptr; };

// the rows of a window query whose row total is counted on the device (obswin_run, sight_run, slot_run): the count, and the rows grown to the largest cap so far
template <class Row>
struct RowsHeld { int* n_rows = nullptr; Row* out = nullptr; std::vector<void*> out_allocs; int cap = 0; };

// what a context holds for tj_obstacle_windows (obswin_run): the per-segment lists grow with the largest max_windows so far
struct ObwinHeld : RowsHeld<tj_obswin_row> { ObwinArgs sized{}; std::vector<void*> allocs; int mw = 0; };

// what a context holds for tj_sight_windows (sight_run): the lists grow with the largest n_links x S x leaf_cap so far, the counters with the largest n_links x S, the links and stations with their counts
struct SightHeld : RowsHeld<tj_sight_row> { SightArgs sized{}; int* links = nullptr; double* stations = nullptr; std::vector<void*> allocs; size_t items = 0, units = 0; int n_links = 0, n_stations = 0; };

// what a context holds for a slot query (tj_dynamics_windows, tj_zone_windows; slot_run): the per-slot lists grow with the largest slots x (3 S + 4 max_windows) so far
template <class Args, class Row>
struct SlotHeld : RowsHeld<Row> { Args sized{}; std::vector<void*> allocs; size_t slots = 0, live = 0, leaf = 0; };

struct tj_ctx {
  tj_params prm;
  Dev d;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  bool maybe_deferred = false;                    // an iteration chain ran since the last flush
  std::vector<void*> allocs;
  std::vector<ArrayDecl> arrays;   // the declaration table (device_arrays): the slots point into d, which does not move
  std::string err;
  bool have_cloud = false, have_state = false;
  CrossQueue xq;
  SchedState ss;   // the host state of the launch sequence (host_launch.h): pairing counters, queue flags, cache flags
  HostPlan hp; PlanFacts facts{};   // the host half of the launch plan (host_plan.h; Dev holds the rest) and the device facts it was decided on.  The plan AS MADE by tj_create: the live
                                    // queue state is ss's (xs_two_queues, keep_two_queues, xs_fault start as planned; heal_check clears them there only)
  // Self-healing (heal_check): a wait between the queues that runs out (ERR_XS_TIMEOUT -- in practice a GPU shared with another process) must not fail a run.  snap_iters:
  // iterations enqueued since the first tj_iterate_async after a host look took the checkpoint.  TJ_HEAL=0: off (the bit is reported as TJ_ERR_NO_PROGRESS, as in round 5).
  bool heal_busy = false; long long snap_iters = 0; int async_fallbacks = 0; Checkpoint ck;
  bool hull_valid = false;   // Dev::fuse: the hull cache matches the control points (else k_hullinfo runs before the next iteration)
  long long launches = 0;    // kernels enqueued by the iteration schedules so far (tj_launch_count)
  bool begin_folded = false; // the last k_linesearch enqueued has already begun the next iteration (begin_next): the next phase 0 / iteration launches no k_begin
  // direct exchange between sharded contexts (Dev::xch): this rank's receive block (uncached), the peers' blocks as mapped here, the device table
  void* xch_block = nullptr; size_t xch_bytes = 0; bool xch_ipc_exported = false;
  std::vector<void*> xch_ipc_opened;
  XchPeers* xch_table = nullptr;
  // cloud-dependent allocations (rebuilt by tj_set_cloud)
  std::vector<void*> cloud_allocs;
  std::vector<int> cloud_order, cloud_rank;   // sorted position -> index in the caller's cloud, and its inverse (ids_to_caller, ids_to_sorted)
  double cloud_lo[3] = {0, 0, 0}, cloud_hi[3] = {0, 0, 0};   // bounding box of the cloud (planner bounds, Main/multiPathPlanning3D.cpp:211-218)
  double bvh_build_ms = 0;   // device time of the last BVH build (tj_get_build_info)
  int bvh_on_device = 0;
  // The read-only queries (dev_query.h; tj_audit, tj_audit_timed, tj_closest_approach, tj_obstacle_approach, tj_obstacle_windows, tj_pair_approach, tj_path_crossings, tj_flight_profile, tj_peak_dynamics): every buffer is allocated by the first call that needs it, and a call
  // whose allocations failed partway keeps what it got (query_buf).  Each query ends in a stream synchronise, so no two are in flight on one context, and they share: q_ctl, the
  // control block the BVH walk reports its overflow bit to (never the solver's); q_net [U][3][T] and q_pt [U], the staged copy of the control nets and piece times a group hands
  // in; q_order (sorted primitive -> caller's index), which belongs to the obstacle set and goes with it (cloud_allocs).  Per query: its rows / lists / counters and its records.
  Ctl* q_ctl = nullptr; double* q_net = nullptr; double* q_pt = nullptr; int* q_order = nullptr;
  AuditArgs audit{}; tj_audit_robot* audit_out = nullptr;
  AuditTimedArgs timed{}; tj_audit_timed_robot* timed_out = nullptr;
  ClosestArgs closest{}; tj_closest_robot* closest_out = nullptr;
  ObstArgs obst{}; tj_obstacle_robot* obst_out = nullptr;
  PeakArgs peak{}; tj_dynamics_robot* peak_out = nullptr;   // tj_peak_dynamics
  // tj_pair_approach, tj_path_crossings (listed_run): the bitmask, its offsets and n are the fleet's size (allocated once, as above); what is sized by the call's cap and
  // max_windows (the other buffers of `sized`, and out) grows with the largest call so far (cap, mw) and lives in allocs
  Listed<PairArgs, tj_pair_record> pair;
  Listed<CrossArgs, tj_crossing_record> cross;
  Listed<MarginArgs, tj_margin_record> margin;
  ProxHeld prox;   // tj_proximity_windows
  ObwinHeld obwin; // tj_obstacle_windows
  SightHeld sight; // tj_sight_windows
  SlotHeld<DynwinArgs, tj_dynwin_row> dynwin; tj_dyn_gate* dynwin_gates = nullptr;   // tj_dynamics_windows, and the gates of a call (their largest size from the start)
  SlotHeld<ZonewinArgs, tj_zonewin_row> zonewin; tj_zone* zonewin_zones = nullptr; double* zonewin_shapes = nullptr;   // tj_zone_windows, and the zone list and shape table of a call (the same)
  // tj_flight_profile: times [K], positions [K][U][3] and records [U][K] grow with the largest n_times so far (profile_cap) and live in profile_allocs
  ProfileArgs profile{}; tj_profile_sample* profile_out = nullptr;
  std::vector<void*> profile_allocs; int profile_cap = 0;
};

// EVERY environment switch of the library is read through this one function (tj_group.h included): TJ_TUNE="KEY=value,KEY=value" or, equivalently, TJ_KEY=value
// (an entry of TJ_TUNE wins over the single variable).  INTEGRATION.md lists them all with their kind -- feature switch, launch-shape switch (same bits), test hook --, and
// tests/test_abi_and_host.py::test_every_environment_switch_is_documented compares that table with the keys that appear here.
static const char* tune(const char* key) {
  static thread_local std::string hold;
  if (const char* t = getenv("TJ_TUNE")) {
    const std::string all(t), k(key);
    size_t pos = 0;
    while (pos < all.size()) {
      size_t end = all.find(',', pos); if (end == std::string::npos) end = all.size();
      const size_t eq = all.find('=', pos);
      if (eq != std::string::npos && eq < end && all.compare(pos, eq - pos, k) == 0) { hold = all.substr(eq + 1, end - eq - 1); return hold.c_str(); }
      pos = end + 1;
    }
  }
  return getenv((std::string("TJ_") + key).c_str());
}

namespace {

#define HIPCHK(c, call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
      return TJ_ERR_DEVICE;                                                                      \
    }                                                                                            \
  } while (0)

int dalloc_bytes(tj_ctx* c, void** p, size_t bytes, std::vector<void*>* list = nullptr) {
  void* q = nullptr;
  HIPCHK(c, hipMalloc(&q, bytes));
  HIPCHK(c, hipMemsetAsync(q, 0, bytes, c->stream));  // ordered on the solver's stream like every kernel and copy that follows
  (list ? *list : c->allocs).push_back(q);
  *p = q;
  return TJ_OK;
}
template <class T>
int dalloc(tj_ctx* c, T** p, size_t n, std::vector<void*>* list = nullptr) { return dalloc_bytes(c, (void**)p, std::max<size_t>(n, 1) * sizeof(T), list); }

int upload(tj_ctx* c, const void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return TJ_OK;
  // on the solver's stream (a non-blocking stream has no implicit ordering against the null stream), then waited for:
  // the host buffer may be reused as soon as this returns
  HIPCHK(c, hipMemcpyAsync((void*)dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return TJ_OK;
}

// ---- host access to the context's device arrays: the bounds come from the declaration table (tj_ctx::arrays), never from the caller ----
// elements [off, off + n) of array `dev` lie inside what the table declares for it; else TJ_ERR_DEVICE, the array named.  a: its declaration
template <class T>
int array_range(tj_ctx* c, const T* dev, size_t off, size_t n, const ArrayDecl** a = nullptr) {
  const ArrayDecl* e = nullptr;
  for (const ArrayDecl& x : c->arrays) if (*x.slot == (const void*)dev) e = &x;
  if (a) *a = e;
  if (e && e->elem == sizeof(T) && off <= e->n && n <= e->n - off) return TJ_OK;
  c->err = std::string("device array ") + (e ? e->name : "(not declared)") + ": elements [" + std::to_string(off) + ", " + std::to_string(off + n) + ") of " + std::to_string(sizeof(T)) + " bytes are outside its extent";
  return TJ_ERR_DEVICE;
}
template <class T>
size_t array_count(tj_ctx* c, const T* dev) { const ArrayDecl* a; return array_range(c, dev, 0, 0, &a) ? 0 : a->n; }
// the whole array to zero bytes, on the context's stream
template <class T>
int array_clear(tj_ctx* c, T* dev) {
  if (int r = array_range(c, dev, 0, 0)) return r;
  HIPCHK(c, hipMemsetAsync(dev, 0, array_count(c, dev) * sizeof(T), c->stream));
  return TJ_OK;
}
// elements [off, off + n) to the host, blocking (the caller has drained the context: QUIESCE) / from the host (upload: on the context's stream, waited for)
template <class T>
int fetch(tj_ctx* c, T* host, const T* dev, size_t off, size_t n) {
  if (int r = array_range(c, dev, off, n)) return r;
  HIPCHK(c, hipMemcpy(host, dev + off, n * sizeof(T), hipMemcpyDeviceToHost));
  return TJ_OK;
}
template <class T>
int store(tj_ctx* c, T* dev, size_t off, const T* host, size_t n) { const int r = array_range(c, dev, off, n); return r ? r : upload(c, dev + off, host, n * sizeof(T)); }

// ---- the templates of the read-only queries' host path (further down, with the rest of it) ----
// a buffer of the queries: allocated once; what an earlier call got before an allocation failed is kept, only the missing ones are retried
template <class T>
int query_buf(tj_ctx* c, T*& p, size_t n, std::vector<void*>* list = nullptr) { return p ? TJ_OK : dalloc(c, &p, n, list); }
// the kernels templated on the primitive kind, each launch written once: f(std::integral_constant<int, PRIM>)
template <class F>
void with_prim(const Dev& d, F&& f) { if (d.prim == 3) f(std::integral_constant<int, 3>{}); else f(std::integral_constant<int, 1>{}); }
// k_xsolve's register factorisation is inlined per size of the reduced system, 9P - 2 rows (kernels_newton.h); 61 rows -- the inlined form would spill -- and the
// LDS forms: the generic kernel, which calls it out of line.  f(std::integral_constant<int, N>): the launch, the attribute query and the LDS attribute all choose here
template <class F>
void with_xsolve(int P, F&& f) {
  switch (9 * P - 2) {
    case 16: f(std::integral_constant<int, 16>{}); break; case 25: f(std::integral_constant<int, 25>{}); break; case 34: f(std::integral_constant<int, 34>{}); break;
    case 43: f(std::integral_constant<int, 43>{}); break; case 52: f(std::integral_constant<int, 52>{}); break; default: f(std::integral_constant<int, 0>{}); break;
  }
}
void release_queues(tj_ctx* c) { if (c->xq.hwq_claim) { queue_budget(c->prm.device, -c->xq.hwq_claim); c->xq.hwq_claim = 0; } }
// the records of a query: zeroed before its launches (robots of other ranks stay zero), copied out after them; rows [U][S] likewise where the caller asked for them
template <class T>
int query_clear(tj_ctx* c, T* dev, size_t n, bool wanted = true) {
  if (wanted) HIPCHK(c, hipMemsetAsync(dev, 0, n * sizeof(T), c->stream));
  return TJ_OK;
}
template <class T>
int query_fetch(tj_ctx* c, T* host, const T* dev, size_t n) {
  if (host) HIPCHK(c, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return TJ_OK;
}

// ---- the iteration's launches: what is enqueued is decided by sequence_kernel (host_launch.h); issue() enqueues one record and is the only place that names a
// kernel of the iteration.  Every kernel it enqueues is counted (tj_launch_count: launches per iteration of a schedule, bench.py / tests); the counter clears are not.
#define TJ_LAUNCH(...) do { c->launches++; hipLaunchKernelGGL(__VA_ARGS__); } while (0)
void issue(tj_ctx* c, const Launch& l) {
  const hipStream_t s = l.queue == 1 ? c->xq.stream2 : (l.queue == 2 ? c->xq.stream3 : c->stream);
  if (l.kid == L_XF_CLEAR) { (void)hipMemsetAsync(c->d.xf_seg + (size_t)l.arg[0] * c->d.S * XF_SEG_STRIDE, 0, (size_t)c->d.S * XF_SEG_STRIDE * sizeof(int), s); return; }
  Dev d = c->d; apply_patch(d, l.patch);
  const dim3 grid(l.grid), block(l.block); const size_t lds = (size_t)l.lds; const int* a = l.arg;
  c->launches++;
  switch (l.kid) {
    case K_BEGIN: if (l.form) hipLaunchKernelGGL(k_begin, grid, block, lds, s, d, c->ck.tab, c->ck.n, c->ck.ctl); else hipLaunchKernelGGL(k_begin, grid, block, lds, s, d, nullptr, 0, nullptr); break;
    case K_HULLINFO: hipLaunchKernelGGL(k_hullinfo, grid, block, lds, s, d); break;
    case K_FRONT: with_prim(d, [&](auto prim) { if (l.form) hipLaunchKernelGGL((k_front<decltype(prim)::value, true>), grid, block, lds, s, d); else hipLaunchKernelGGL((k_front<decltype(prim)::value>), grid, block, lds, s, d); }); break;
    case K_SEP_OBS: with_prim(d, [&](auto prim) { hipLaunchKernelGGL((k_obs_query<decltype(prim)::value>), grid, block, lds, s, d); }); break;
    case K_OBS_SOLVE: with_prim(d, [&](auto prim) { hipLaunchKernelGGL((k_obs_solve<decltype(prim)::value>), grid, block, lds, s, d); }); break;
    case K_SEP_SELF_ROWS: hipLaunchKernelGGL(k_sep_self_rows, grid, block, lds, s, d); break;
    case K_MID: with_prim(d, [&](auto prim) { if (l.form) hipLaunchKernelGGL((k_mid<decltype(prim)::value, true>), grid, block, lds, s, d, a[0], a[1]); else hipLaunchKernelGGL((k_mid<decltype(prim)::value>), grid, block, lds, s, d, a[0], a[1]); }); break;
    case K_SEP_SELF_SOLVE: hipLaunchKernelGGL(k_sep_self_solve, grid, block, lds, s, d); break;
    case K_KEEP: hipLaunchKernelGGL(k_keep, grid, block, lds, s, d, a[0]); break;
    case K_SEP_SELF_COMPACT: hipLaunchKernelGGL(k_sep_self_compact, grid, block, lds, s, d); break;
    case K_GRAD: if (l.form) hipLaunchKernelGGL((k_grad<true>), grid, block, lds, s, d); else hipLaunchKernelGGL((k_grad<false>), grid, block, lds, s, d); break;
    case K_XSOLVE:
      if (l.form == FORM_BAND) hipLaunchKernelGGL(k_xsolve_band, grid, block, lds, s, d);
      else with_xsolve(d.P, [&](auto n) { hipLaunchKernelGGL((k_xsolve<decltype(n)::value>), grid, block, lds, s, d); });
      break;
    case K_XSOLVE_C2: if (l.form == FORM_BAND) hipLaunchKernelGGL(k_xsolve_c2_band, grid, block, lds, s, d); else hipLaunchKernelGGL(k_xsolve_c2, grid, block, lds, s, d); break;
    case K_CCD_PREP: hipLaunchKernelGGL(k_ccd_prep, grid, block, lds, s, d, a[0]); break;
    case K_CCD: with_prim(d, [&](auto prim) { hipLaunchKernelGGL((k_ccd_lean<decltype(prim)::value>), grid, block, lds, s, d); }); break;
    case K_CCD_OBS: with_prim(d, [&](auto prim) { hipLaunchKernelGGL((k_ccd_obs<decltype(prim)::value>), grid, block, lds, s, d); }); break;
    case K_CCD_SELF_PAIRS: hipLaunchKernelGGL(k_ccd_self_pairs, grid, block, lds, s, d); break;
    case K_CCD_SELF_SEQ: hipLaunchKernelGGL(k_ccd_self_seq, grid, block, lds, s, d); break;
    case K_LINESEARCH: hipLaunchKernelGGL(k_linesearch, grid, block, lds, s, d, c->hp.lsl, a[0]); break;
    case K_LS_COUPLED: hipLaunchKernelGGL(k_ls_coupled, grid, block, lds, s, d, c->hp.lsl, a[0], a[1], a[2], a[3]); break;
    case K_LS_COMMIT: hipLaunchKernelGGL(k_ls_commit, grid, block, lds, s, d, a[0]); break;
    case K_SLACK: hipLaunchKernelGGL(k_slack, grid, block, lds, s, d, a[0]); break;
    case L_XS_GATE: hipLaunchKernelGGL(k_xs_gate, grid, block, lds, s, d, a[0], a[1]); break;
    case L_KEEP_GATE: hipLaunchKernelGGL(k_keep_gate, grid, block, lds, s, d, a[0]); break;
    case L_FA_GATE: hipLaunchKernelGGL(k_fa_gate, grid, block, lds, s, d, a[0]); break;
    case L_XCH_WAIT: hipLaunchKernelGGL(k_xch_wait, grid, block, lds, s, d, a[0]); break;
  }
}
// sequence, then issue: one kernel id (returns whether it exists in this schedule) / a list of them
bool enqueue_kernel(tj_ctx* c, Sched sched, int chain_pos, int kid) {
  LaunchList l;
  const bool exists = sequence_kernel(c->d, c->hp, c->ss, sched, chain_pos, kid, l);
  for (int i = 0; i < l.n; i++) issue(c, l.v[i]);
  return exists;
}
int enqueue_list(tj_ctx* c, Sched sched, int chain_pos, const KernelList& list) {
  LaunchList l;
  sequence_list(c->d, c->hp, c->ss, sched, chain_pos, list, l);
  for (int i = 0; i < l.n; i++) issue(c, l.v[i]);
  HIPCHK(c, hipGetLastError());
  return TJ_OK;
}

// enqueue one stage (= one or more kernels)
int enqueue_stage(tj_ctx* c, int stage) {
  if (stage == TJ_STAGE_END) { hipLaunchKernelGGL(k_end, dim3(1), dim3(1), 0, c->stream, c->d); HIPCHK(c, hipGetLastError()); return TJ_OK; }
  if (stage < 0 || stage > TJ_STAGE_END) { c->err = "unknown stage"; return TJ_ERR_INVALID; }
  return enqueue_list(c, Sched::Stage, 0, kStageKernels[stage]);
}

// One iteration of the single-GPU schedule (Sched::Chain): a LINEAR chain on one stream / hardware queue
//   begin -> [hullinfo] -> front{obstacle planes | pair rows} -> mid{slack+dual of the PREVIOUS iteration | pair solves}
//         -> compact -> grad -> xsolve [-> xsolve_c2] -> ccd_prep -> ccd{obstacle CCD | pair CCD selection} -> seq -> line search
// Same-queue successors start back to back, so concurrency between independent stages comes from sharing a launch
// (union kernels), not from parallel streams.  The plane builders only read control points, which the previous line
// search already committed, so that iteration's slack/dual update (touches z, Lambda, t_z, tau only) is deferred into
// k_mid; flush_deferred() pays the last one before anything on the host looks at the state.  The iteration counter is
// committed by the next k_begin.  Plain launches: the host enqueues far ahead of the device, and a hipGraph replay of the
// same chain measured 4 us slower per iteration.
// (k0, k1: only kernels [k0, k1) of the stream order -- the lockstep enqueue of ranks that share a device, tj_group.h)
int enqueue_iteration(tj_ctx* c, int chain_pos = 0, int k0 = 0, int k1 = K_COUNT) {
  LaunchList l;
  for (int k = k0; k < k1; k++) sequence_kernel(c->d, c->hp, c->ss, Sched::Chain, chain_pos, k, l);
  for (int i = 0; i < l.n; i++) issue(c, l.v[i]);
  HIPCHK(c, hipGetLastError());
  c->maybe_deferred = true;
  return TJ_OK;
}


int ensure_hull_cache(tj_ctx* c);

// Pay a deferred slack/dual update (no-op kernels if nothing is owed).
int flush_deferred(tj_ctx* c) {
  if (!c->maybe_deferred) return TJ_OK;
  const Dev& d = c->d;
  TJ_LAUNCH(k_flush, dim3(1), dim3(1), 0, c->stream, d, c->begin_folded ? 1 : 0);   // (a begin folded into the last line search whose iteration was never enqueued is taken back)
  c->begin_folded = false;
  TJ_LAUNCH(k_slack, dim3((d.u1 - d.u0) * d.P), dim3(64), 0, c->stream, d, 1);   // (deferred: pays the update only where Ctl::slack_now says one is owed)
  HIPCHK(c, hipGetLastError());
  c->maybe_deferred = false;
  return TJ_OK;
}

// drain: pay a deferred slack/dual update, then wait for every queue of the context
#define QUIESCE_NOHEAL(c)                                       \
  do {                                                          \
    int qr_ = flush_deferred(c);                                \
    if (qr_) return qr_;                                        \
    HIPCHK(c, hipStreamSynchronize((c)->stream));               \
    if ((c)->xq.stream2) HIPCHK(c, hipStreamSynchronize((c)->xq.stream2)); \
    if ((c)->xq.stream3) HIPCHK(c, hipStreamSynchronize((c)->xq.stream3)); \
  } while (0)
// every host-visible read or write of solver state first drains the context -- and, where a batch ran on several queues, looks whether it has to be run again (heal_check:
// one 4-byte read-back; tj_sync alone does not look -- whoever reads a result afterwards does; tj_iterate uses the control block it reads anyway)
#define QUIESCE(c)                                              \
  do {                                                          \
    QUIESCE_NOHEAL(c);                                          \
    if ((c)->snap_iters > 0 && !(c)->heal_busy) { int hr_ = heal_check(c, -1); if (hr_) return hr_; } \
  } while (0)

// Restart the pairings of the cross-queue schedule (CrossQueue): device words and host counters together, every queue drained.  keep_go (tj_init_state): the go words
// xs_go / keep_go and their counters go on counting (nothing is in flight: they still match); the words in front of xs_go and fa_sync restart (begin_body zeroes keep_sync's counters).
int restart_pairings(tj_ctx* c, bool keep_go) {
  HIPCHK(c, hipMemsetAsync(c->d.xs_sync, 0, (keep_go ? (size_t)(c->d.xs_go() - c->d.xs_sync) : Dev::xs_sync_ints(c->d.U)) * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d.fa_sync, 0, Dev::fa_sync_ints(c->d.U) * sizeof(int), c->stream)); c->ss.fa_seq = 0; c->ss.fa_armed = c->ss.fa_mid_now = false;
  if (!keep_go) { HIPCHK(c, hipMemsetAsync(c->d.keep_sync, 0, Dev::keep_sync_ints() * sizeof(int), c->stream)); c->ss.xs_seq = c->ss.xs_seq_gated = c->ss.keep_seq = 0; }
  return TJ_OK;
}
// Checkpoint take: the host half now, the device half in the next k_begin (in_begin: the batch starts with one -- no begin folded) or in a k_snapshot launch now.
int checkpoint_take(tj_ctx* c, bool in_begin) {
  Checkpoint& k = c->ck;
  c->ss.ck_in_begin = in_begin; k.begin_folded = c->begin_folded; k.maybe_deferred = c->maybe_deferred; k.lsc_base = c->ss.lsc_base;
  if (!in_begin) { hipLaunchKernelGGL(k_snapshot, dim3(64, std::max(k.n, 1)), dim3(256), 0, c->stream, k.tab, k.n, 0, c->d.ctl, k.ctl); HIPCHK(c, hipGetLastError()); }
  return TJ_OK;
}
// Restore: both halves back (the control block keeps the abandoned run's epoch: k_snapshot), the caches outside the checkpoint stale.  What a folded begin zeroed (work
// lists, begin_body) is not in the checkpoint: such a fold is taken back as by any flush, so the next iteration starts with its own k_begin and counts the begun one once.
int checkpoint_restore(tj_ctx* c) {
  const Checkpoint& k = c->ck;
  hipLaunchKernelGGL(k_snapshot, dim3(64, std::max(k.n, 1)), dim3(256), 0, c->stream, k.tab, k.n, 1, c->d.ctl, k.ctl); HIPCHK(c, hipGetLastError());
  c->begin_folded = k.begin_folded; c->maybe_deferred = k.maybe_deferred; c->ss.lsc_base = k.lsc_base; c->hull_valid = c->ss.ccd_valid = c->ss.xf_used[0] = c->ss.xf_used[1] = false;
  return c->begin_folded ? flush_deferred(c) : TJ_OK;
}
void checkpoint_drop(tj_ctx* c) { c->ss.ck_in_begin = 0; }

// Self-healing (tj_ctx): the batch enqueued since the checkpoint is through.  No incident: drop the checkpoint.  ERR_XS_TIMEOUT: latch one queue (release the queue
// claim, clear the two-queue flags, restart the pairings), restore the checkpoint, enqueue the same iterations again and drain.
int heal_check(tj_ctx* c, int err_known) {
  int err = err_known;
  if (err < 0) HIPCHK(c, hipMemcpy(&err, &c->d.ctl->error, sizeof(int), hipMemcpyDeviceToHost));   // (every queue has drained: QUIESCE)
  const long long n = c->snap_iters; c->snap_iters = 0;
  if (!(err & ERR_XS_TIMEOUT)) { checkpoint_drop(c); return TJ_OK; }
  struct Busy { tj_ctx* c; ~Busy() { c->heal_busy = false; } } busy{c}; c->heal_busy = true;   // (reset on every exit)
  c->async_fallbacks++;
  release_queues(c);   // (the budget is free for another context)
  c->ss.xs_two_queues = c->ss.keep_two_queues = false; c->ss.xs_fault = 0;   // (the tickets / flags of the asynchronous solve work on one queue as well: TJ_XS_ONE_QUEUE's schedule)
  int r = restart_pairings(c, false);
  if (r || (r = checkpoint_restore(c))) return r;
  checkpoint_drop(c);   // (the run enqueued again stays on one queue: nothing of it is healed)
  if ((r = array_clear(c, c->d.xf_seg)) || (r = array_clear(c, c->d.spec_n))) return r;   // (spec_n: head-start lists of the abandoned iterations, launch shape only)
  if ((r = tj_iterate_async(c, (int)n))) return r;
  QUIESCE_NOHEAL(c);
  return TJ_OK;
}

// Phase `which` of a sharded iteration (Sched::Phase), split at the all-gathers (kPhaseKernels, host_launch.h).  The phases are linear chains on the context's stream as well and
// reuse the union kernels where the stages they join fall into the same phase (k_mid, k_ccd); the slack/dual update is the deferred one inside k_mid.
int enqueue_body(tj_ctx* c, int which, int chain_pos = 0) {
  const bool cpl = c->d.mode == TJ_MODE_MULTI_COUPLED;
  if (which == 1 && c->d.fuse) { int hr = ensure_hull_cache(c); if (hr) return hr; }   // fused phases: k_linesearch keeps the owned robots' hull cache; after a host write it is rebuilt once
  if (int r = enqueue_list(c, Sched::Phase, chain_pos, kPhaseKernels[cpl ? 1 : 0][which])) return r;
  // this iteration's slack/dual update is owed to the next k_mid (or the flush) -- in a followed coupled search only once the search is over (tj_coupled_search_pending says so):
  // a flush between two tables of candidates would pay the update on the uncommitted control net
  if (which == (cpl ? 5 : 2) && !(cpl && c->d.lsc_follow && c->d.u1 - c->d.u0 != c->d.U)) c->maybe_deferred = true;
  return TJ_OK;
}

int check_device_errors(tj_ctx* c, Ctl* out = nullptr) {
  Ctl h;
  const int fb0 = c->async_fallbacks;
  { int fr_ = flush_deferred(c); if (fr_) return fr_; }   // (in front of the copies: they are to see the state behind the last slack / dual update)
  HIPCHK(c, hipMemcpyAsync(&h, c->d.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
  QUIESCE_NOHEAL(c);
  if (c->snap_iters > 0 && !c->heal_busy) { int hr_ = heal_check(c, h.error); if (hr_) return hr_; }   // (the error word has come with the control block: no extra read-back)
  if (c->async_fallbacks != fb0) HIPCHK(c, hipMemcpy(&h, c->d.ctl, sizeof(Ctl), hipMemcpyDeviceToHost));   // the batch was run again on one queue (heal_check): what was copied above belongs to the abandoned attempt
  if (out) *out = h;
  if (h.error & ERR_PEER_TIMEOUT) { c->err = "tj_group: a peer rank's slice did not arrive within 2 s (flag transport); the group must be re-initialised"; return TJ_ERR_DEVICE; }
  if (h.error & (ERR_PLANE_OVERFLOW | ERR_FRONT_OVERFLOW | ERR_PAIR_OVERFLOW)) {
    c->err = "device list overflow (error bits " + std::to_string(h.error) + "): raise cap_obs/cap_self/cap_pairs";
    return TJ_ERR_CAPACITY;
  }
  if (h.error & ERR_LOOP_CAP) {
    c->err = "a device back-off/Newton/Armijo loop hit its cap (infeasible state)";
    if (h.error & ERR_LS_RANGE) c->err += ": coupled mode on a SHARDED context, no acceptable step among the 31 Armijo back-offs its exchange carries (one context follows the search to the reference's own end)";
    if (h.error & ERR_CCD_STUCK) c->err += ": a CCD clamp found contact at every step (the state itself is in collision; the reference loops forever here)";
    if (h.error & ERR_SLACK_ARMIJO) c->err += ": the slack update's Armijo search";
    if (h.error & ERR_PLANE_REFINE) c->err += ": optimal_plane, a plane refinement did not terminate within its caps";
    if (h.error & ERR_XS_TIMEOUT) c->err += ": NOT an infeasible state -- a wait between the queues of the context (asynchronous Newton solve / plane refinement) ran out after 2 s (GPU shared with other processes?); TJ_XS_ASYNC=0 TJ_KEEP_ASYNC=0 keep everything on the chain's queue";
    if (h.error & ERR_PASS_TIMEOUT) c->err += ": NOT an infeasible state -- a wave waiting for passed-on robot pairs timed out after 5 ms (GPU queue descheduled / shared with other processes); re-run the iteration or set TJ_PAIR_PASS_ON=0";
    return TJ_ERR_NO_PROGRESS;
  }
  if (h.order_unresolved) { c->err = "inter-robot CCD clamp: two acting pairs of a segment share a robot and the reference's pair order could not be replayed (fleet too large for the LDS-resident tree)"; return TJ_ERR_UNSUPPORTED; }
  if (h.error & ERR_NOT_SPD) { c->err = "coupled mode: the arrowhead Newton system is not positive definite (the reference has no fallback either)"; return TJ_ERR_NO_PROGRESS; }
  return TJ_OK;
}

// Dev::fuse: the iteration chain has no k_hullinfo (k_linesearch leaves the next iteration's hull cache); after the
// control points were set from the host the cache is rebuilt once here.
int ensure_hull_cache(tj_ctx* c) {
  if (!c->d.fuse || c->hull_valid) return TJ_OK;
  enqueue_kernel(c, Sched::Stage, 0, K_HULLINFO);
  HIPCHK(c, hipGetLastError());
  c->hull_valid = true; c->ss.hull_from_units = false;
  return TJ_OK;
}

bool ready(tj_ctx* c) {
  if (!c->have_cloud) { c->err = "tj_set_cloud has not been called"; return false; }
  if (!c->have_state) { c->err = "tj_init_state has not been called"; return false; }
  return true;
}

// Obstacle ids: the device holds positions of the build's sorted order, the caller speaks of indices into its own cloud / face list.  To the caller's (cloud_order), in place ...
void ids_to_caller(const tj_ctx* c, int* ids, size_t n) { for (size_t i = 0; i < n; i++) ids[i] = c->cloud_order[ids[i]]; }
// ... and back, through the inverse that the first call after set_obstacles makes; false: an id outside the caller's list
bool ids_to_sorted(tj_ctx* c, const int* ids, size_t n, int* sorted) {
  std::vector<int>& rank = c->cloud_rank;
  if (rank.size() != c->cloud_order.size()) { rank.resize(c->cloud_order.size()); for (size_t i = 0; i < rank.size(); i++) rank[c->cloud_order[i]] = (int)i; }
  for (size_t i = 0; i < n; i++) { if (ids[i] < 0 || (size_t)ids[i] >= rank.size()) return false; sorted[i] = rank[ids[i]]; }
  return true;
}
// the id list of (robot, segment) s, cap_obs slots each: its count n, and min(n, cap) ids in the caller's numbering
int fetch_ids(tj_ctx* c, const int* count, const int* list, size_t s, int cap, int* ids, int& n) {
  int r = fetch(c, &n, count, s, 1);
  if (r || std::min(n, cap) <= 0 || !ids) return r;
  if (!(r = fetch(c, ids, list, s * c->d.cap_obs, std::min(n, cap)))) ids_to_caller(c, ids, std::min(n, cap));
  return r;
}

}  // namespace

extern "C" {

void tj_default_params(tj_params* p, int mode, int uav_num, int piece_num) {
  memset(p, 0, sizeof(*p));
  p->mode = mode; p->uav_num = uav_num; p->piece_num = piece_num; p->res = 8;
  p->lambda = 10.0; p->margin = 0.1; p->offset = 0.1; p->mu = 0.1; p->vel_limit = 2.0; p->acc_limit = 2.0;
  p->ks = mode == TJ_MODE_SINGLE ? 1e-8 : 1e-3;  /* Main/admmPathPlanning3D.cpp:477, Main/multiPathPlanning3D.cpp:596 */ p->kt = 1.0; p->stop = 1e-2;
  p->device = 0; p->rank = 0; p->world = 1;
}

#ifdef TJ_PHASE_TIMING
// development build only (make timing): wall-clock stamps (10 ns ticks) the kernels left at their
// phase boundaries during the most recent launch; out is [K_COUNT][TJ_TIC_BLOCKS][TJ_TIC_SLOTS]
int tj_debug_phase_times(tj_ctx* c, long long* out) {
  if (!c || !out) return TJ_ERR_INVALID;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out, c->d.dbg, sizeof(long long) * K_COUNT * TJ_TIC_BLOCKS * TJ_TIC_SLOTS, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemsetAsync(c->d.dbg, 0, sizeof(long long) * K_COUNT * TJ_TIC_BLOCKS * TJ_TIC_SLOTS, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return K_COUNT;
}
#endif

int tj_host_tables(int piece_num, int res, double* convert, double* mdyn, double* basis, double* kdop) {
  if (piece_num < 1 || res < 1) return TJ_ERR_INVALID;
  HostTables t;
  build_tables(piece_num, res, 1, t);
  if (convert) memcpy(convert, t.convert.data(), t.convert.size() * 8);
  if (mdyn) memcpy(mdyn, t.mdyn, 36 * 8);
  if (basis) memcpy(basis, t.basis.data(), t.basis.size() * 8);
  if (kdop) memcpy(kdop, t.kdop, 147 * 8);
  return TJ_OK;
}

const char* tj_last_error(const tj_ctx* c) { return c ? c->err.c_str() : "null context"; }

}  // extern "C"

// ---- tj_create's steps ----
namespace {

const void* xsolve_fn(int P) { const void* f = nullptr; with_xsolve(P, [&](auto n) { f = (const void*)k_xsolve<decltype(n)::value>; }); return f; }

KernelFact kernel_fact(const void* f) {
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, f) != hipSuccess) { (void)hipGetLastError(); return KernelFact{0, 0, 0}; }
  return KernelFact{1, a.numRegs, (int)a.sharedSizeBytes};
}

// what the planner is told about the device (host_plan.h: PlanFacts) -- every runtime query the plan depends on is made here
int gather_facts(tj_ctx* c, PlanFacts& f) {
  hipDeviceProp_t prop;
  HIPCHK(c, hipGetDeviceProperties(&prop, c->prm.device));
  f = PlanFacts{};
  f.num_cu = prop.multiProcessorCount;
  f.xsolve = kernel_fact(xsolve_fn(c->prm.piece_num));
  f.grad[0] = kernel_fact((const void*)k_grad<false>); f.grad[1] = kernel_fact((const void*)k_grad<true>);
  f.front = kernel_fact((const void*)k_front<1, true>);
  const KernelFact f3 = kernel_fact((const void*)k_front<3, true>);
  if (f.front.ok && f3.ok) { f.front.regs = std::max(f.front.regs, f3.regs); f.front.lds = std::max(f.front.lds, f3.lds); }
  const char* cc = getenv("ROCPROF_COUNTER_COLLECTION");
  f.counters_on = (cc && cc[0] && strcmp(cc, "0") != 0 && strcasecmp(cc, "false") != 0) ? 1 : 0;
  f.prim = 1;
  return TJ_OK;
}

// the dynamic LDS every kernel of the plan may ask for
int set_lds_attributes(tj_ctx* c) {
  const Dev& d = c->d; const HostPlan& h = c->hp;
  auto set = [&](const void* f, size_t bytes) -> int { HIPCHK(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)); return TJ_OK; };
  int r;
  if ((r = set((const void*)k_grad<true>, h.lds_grad_of(true, d.res))) || (r = set((const void*)k_grad<false>, h.lds_grad)) ||
      (r = set(d.xs_band ? (const void*)k_xsolve_band : xsolve_fn(d.P), h.lds_xs)) ||
      (r = set((const void*)k_linesearch, h.lds_ls)) || (r = set((const void*)k_ls_coupled, h.lds_ls)) ||
      (r = set(d.xs_band ? (const void*)k_xsolve_c2_band : (const void*)k_xsolve_c2, h.lds_xs2)) || (r = set((const void*)k_ccd_self_seq, h.lds_seq))) return r;
  return TJ_OK;
}

// k_xsolve's overlap-add as a table: per entry of the reduced system the (at most two) piece-block entries that cover it, in piece order; -2: the time-time entry (every piece)
const char* build_xs_gather(int Pn, std::vector<int>& gt) {
  const int m = 9 * Pn - 3, n = m + 1;
  gt.assign((size_t)2 * n * n + 2 * n, -1);
  for (int idx = 0; idx < n * n; idx++) {   // the sources xs_entry would sum
    const int ga = xs_global(idx / n, m), gb = xs_global(idx % n, m);
    if (ga < 0 && gb < 0) { gt[2 * (size_t)idx] = -2; continue; }
    const XsCover c = xs_cover(ga, gb, Pn);
    if (c.hi - c.lo > 1) return "internal: an entry of the reduced system is covered by more than two piece blocks";
    for (int sp = c.lo; sp <= c.hi; sp++) gt[2 * (size_t)idx + (sp - c.lo)] = sp * 361 + xs_local(ga, sp) * 19 + xs_local(gb, sp);
  }
  for (int ra = 0; ra < n; ra++) {   // ... and xs_grad_entry
    const int ga = xs_global(ra, m);
    if (ga < 0) { gt[(size_t)2 * n * n + 2 * ra] = -2; continue; }
    const XsCover c = xs_cover(ga, Pn);
    if (c.hi - c.lo > 1) return "internal: a row of the reduced system is covered by more than two piece blocks";
    for (int sp = c.lo; sp <= c.hi; sp++) gt[(size_t)2 * n * n + 2 * ra + (sp - c.lo)] = sp * 19 + xs_local(ga, sp);
  }
  return nullptr;
}

// the constant tables of the kernels: built on the host, uploaded once
int upload_tables(tj_ctx* c) {
  Dev& d = c->d;
  HostTables t;
  build_tables(d.P, d.res, STEP_CAP, t);
  std::vector<int> gt;
  if (const char* bad = build_xs_gather(d.P, gt)) { c->err = bad; return TJ_ERR_INVALID; }
  auto put = [&](auto*& dst, const auto* src, size_t n) {
    std::remove_const_t<std::remove_reference_t<decltype(*dst)>>* q = nullptr;
    int r = dalloc(c, &q, n);
    if (!r) r = upload(c, q, src, n * sizeof(*q));
    dst = q;
    return r;
  };
  int r;
  if ((r = put(d.basis, t.basis.data(), t.basis.size())) || (r = put(d.convert, t.convert.data(), t.convert.size())) || (r = put(d.mdyn, t.mdyn, 36)) ||
      (r = put(d.kdop, t.kdop, 147)) || (r = put(d.pow08, t.pow08.data(), t.pow08.size())) || (r = put(d.xs_gather, gt.data(), gt.size()))) return r;
  return TJ_OK;
}

// The declaration table (ArrayDecl, at the top): one ARR per array, flags SNAP | ZERO | ONES.  What tj_init_state fills is what the mains start from: epochs and tags
// restart (ostamp, pairstamp, pairbits, ls_word, pair_ovf_list, spec_tag), counts and statistics are empty, the persistent plane tables are off.  The payload behind a
// zeroed count (oplanes, kobs_id, kobs_cd, kpair_list, kpair_cd, ...) and what every iteration rebuilds before reading it (lg, lh, hullinfo, ccdinfo, ...) is left alone.
template <class T>
ArrayDecl arr(const char* name, T*& p, size_t n, int flags = 0) { return ArrayDecl{name, (void**)&p, n, sizeof(T), (flags & SNAP) != 0, flags & (ZERO | ONES)}; }
#define ARR(member, ...) arr(#member, d.member, __VA_ARGS__)

std::vector<ArrayDecl> device_arrays(Dev& d) {
  const size_t U = d.U, S = d.S, P = d.P, T = d.T, owned = d.u1 - d.u0, n = 9 * P - 2, co = d.cap_obs, cs = d.cap_self;
  const bool multi = d.mode >= 1;
  std::vector<ArrayDecl> a = {
    ARR(spline, U * 3 * T, SNAP), ARR(p_slack, U * 18 * P, SNAP), ARR(p_lambda, U * 18 * P, SNAP), ARR(t_slack, U * P, SNAP), ARR(t_lambda, U * P, SNAP), ARR(piece_time, U, SNAP),
    ARR(oplanes, U * S * co * 4), ARR(ocount, U * S, ZERO), ARR(splanes, U * S * cs * 4), ARR(scount, U * S, ZERO),
    ARR(lg, U * P * 19), ARR(lh, U * P * 361), ARR(xdir, U * d.xs, SNAP | ZERO),
    ARR(k_obs, U), ARR(k_self, U), ARR(step_out, U, SNAP), ARR(ls_hist, U, SNAP | ONES), ARR(grad_cost, owned * P, ZERO), ARR(grad_perm, owned * P), ARR(ls_tab, U * LS_TAB_STRIDE, ONES), ARR(ls_word, U, ZERO),
    ARR(ccdinfo, U * S * CCD_STRIDE), ARR(pair_list, ACT_CAP),
    ARR(seg_stats, U * S * 6, SNAP | ZERO), ARR(pair_stats, U * S * 2, SNAP | ZERO), ARR(blk_stats, U * P + U, SNAP | ZERO),
    ARR(hullinfo, U * S * HULL_INFO_STRIDE), ARR(hbox, S * 6 * U), ARR(cbox, S * 6 * U), ARR(pairplane, multi ? S * U * U * 4 : 1),
    ARR(pairstamp, multi ? S * U * U : 1, ZERO), ARR(pairbits, multi ? S * U * ((U + 63) / 64) : 1, ZERO),
    ARR(pair_work, 3 * (size_t)d.cap_work), ARR(pair_work_n, S + 1), ARR(pair_ovf, 4, ZERO), ARR(seq_gmem_d, SeqLayout(d.U, ACT_CAP, true).tree_doubles), ARR(seq_gmem_i, SeqLayout(d.U, ACT_CAP, true).tree_ints),
    ARR(spec_n, 2, ZERO), ARR(spec_list, 2 * SPEC_CAP), ARR(spec_tag, SPEC_CAP, ZERO), ARR(spec_state, SPEC_CAP * SPEC_STATE_DOUBLES), ARR(spec_sti, SPEC_CAP * SPEC_STATE_INTS),
    ARR(pair_ovf_list, (size_t)d.cap_work + PAIR_CONSUMERS_MAX, ZERO), ARR(ctl, 1),
    ARR(ocand, U * S * co), ARR(ocand_n, U * S, ZERO), ARR(ohull, U * S * 18),
    ARR(obs_work, 2 * U * S * co), ARR(obs_work_n, 1), ARR(oraw, U * S * co * 4), ARR(ostamp, U * S * co, ZERO),
    ARR(grad_scr, owned * P * 16 * (co + cs)), ARR(xs_scr, d.xs_band ? owned * (n * n + 4 * n) : 1),
    ARR(xf_seg, 2 * S * XF_SEG_STRIDE, ZERO), ARR(xs_sync, Dev::xs_sync_ints(d.U)), ARR(keep_sync, Dev::keep_sync_ints()), ARR(fa_sync, Dev::fa_sync_ints(d.U))};
#ifdef TJ_PHASE_TIMING
  a.push_back(ARR(dbg, (size_t)K_COUNT * TJ_TIC_BLOCKS * TJ_TIC_SLOTS));
#endif
  if (d.optimal_plane) {   // the planes that persist across iterations: obstacle lists (single UAV) or the dense pair table
    const bool m0 = d.mode == 0;
    const int s0 = m0 ? SNAP : 0, s1 = m0 ? 0 : SNAP;
    a.insert(a.end(), {ARR(kobs_id, m0 ? U * S * co : 1, s0), ARR(kobs_n, U * S, s0 | ZERO), ARR(kobs_cd, m0 ? U * S * co * 4 : 1, s0),
                       ARR(kpair_on, m0 ? 1 : S * U * U, s1 | ZERO), ARR(kpair_list, m0 ? 1 : S * U * U, s1), ARR(kpair_n, 2, s1 | ZERO), ARR(kpair_cd, m0 ? 1 : S * U * U * 4, s1)});
  }
  if (d.mode == TJ_MODE_MULTI_COUPLED)
    a.insert(a.end(), {ARR(xL, U * (d.xs_band ? (n - 1) * BAND_BS + n : n * n)), ARR(xy, U * n), ARR(xg, U * n), ARR(xcorner, U * 4), ARR(k_obs_f, U), ARR(ls_e, (size_t)LSC_ROUNDS * U * LS_GROUPS)});
  return a;
}
#undef ARR

// build the table, allocate the arrays and, for those of the checkpoint, an arena each and the region table k_snapshot walks
int allocate_arrays(tj_ctx* c) {
  const std::vector<ArrayDecl>& arrays = c->arrays = device_arrays(c->d);
  int r;
  for (const ArrayDecl& a : arrays) if ((r = dalloc_bytes(c, a.slot, std::max<size_t>(a.n, 1) * a.elem))) return r;
  std::vector<SnapRegion> tab;
  for (const ArrayDecl& a : arrays) {
    if (!a.snap) continue;
    char* snap = nullptr;
    if ((r = dalloc(c, &snap, (a.n * a.elem + 15) / 16 * 16))) return r;
    tab.push_back(SnapRegion{(char*)*a.slot, snap, (unsigned long long)(a.n * a.elem)});
  }
  c->ck.n = (int)tab.size();
  if ((r = dalloc(c, &c->ck.tab, tab.size())) || (r = dalloc(c, &c->ck.ctl, 1)) || (r = upload(c, c->ck.tab, tab.data(), tab.size() * sizeof(SnapRegion)))) return r;
  return TJ_OK;
}

}  // namespace

extern "C" {

// validate -> device and stream -> facts -> plan -> claim queues (refused: plan again) -> streams (missing: downgrade) -> LDS attributes -> tables -> arrays
int tj_create(const tj_params* p, tj_ctx** out) {
  if (!p || !out) return TJ_ERR_INVALID;
  *out = nullptr;
  tj_ctx* c = new tj_ctx();
  *out = c;  // returned even on failure so the caller can read tj_last_error()
  c->prm = *p;
  if (const char* bad = plan_check_params(p)) { c->err = bad; return TJ_ERR_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { c->err = "no HIP device available (this library has no CPU fallback)"; return TJ_ERR_DEVICE; }
  HIPCHK(c, hipSetDevice(p->device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  int r;
  if ((r = gather_facts(c, c->facts))) return r;
  Plan pl = plan_context(p, c->facts, tune);
  if (!pl.err && pl.h.queues > 1) {   // contexts that sleep across queues claim their streams out of the process's budget (host_plan.h)
    if (queue_budget(p->device, pl.h.queues, pl.h.forced)) c->xq.hwq_claim = pl.h.queues;
    else { c->facts.claim_refused = 1; pl = plan_context(p, c->facts, tune); }
  }
  auto stream_for = [&](int wanted, hipStream_t& s) {   // (a stream that cannot be created is not an error: plan_downgrade)
    if (wanted && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s = nullptr; }
    return !wanted || s != nullptr;
  };
  if (!pl.err) { const bool s2 = stream_for(pl.d.xs_async, c->xq.stream2), s3 = stream_for(pl.d.keep_async, c->xq.stream3); plan_downgrade(pl, s2, s3); }
  c->d = pl.d; c->hp = pl.h;
  c->ss.xs_two_queues = pl.h.xs_two_queues; c->ss.keep_two_queues = pl.h.keep_two_queues; c->ss.xs_fault = pl.h.xs_fault;
  if (pl.err) { c->err = pl.msg; return pl.err; }
  if ((r = set_lds_attributes(c)) || (r = upload_tables(c)) || (r = allocate_arrays(c))) return r;
  return TJ_OK;
}

void tj_destroy(tj_ctx* c) {
  if (!c) return;
  release_queues(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->xq.stream2) { (void)hipStreamSynchronize(c->xq.stream2); (void)hipStreamDestroy(c->xq.stream2); }
  if (c->xq.stream3) { (void)hipStreamSynchronize(c->xq.stream3); (void)hipStreamDestroy(c->xq.stream3); }
  for (void* p : c->xch_ipc_opened) (void)hipIpcCloseMemHandle(p);
  if (c->xch_block) (void)hipFree(c->xch_block);
  for (void* p : c->allocs) hipFree(p);
  for (void* p : c->cloud_allocs) hipFree(p);
  for (void* p : c->pair.allocs) hipFree(p);
  for (void* p : c->cross.allocs) hipFree(p);
  for (void* p : c->margin.allocs) hipFree(p);
  for (void* p : c->prox.allocs) hipFree(p);
  const auto free_windows = [](auto& h) { for (void* p : h.allocs) hipFree(p); for (void* p : h.out_allocs) hipFree(p); };   // a window query's lists, and its rows (RowsHeld)
  free_windows(c->obwin); free_windows(c->sight); free_windows(c->dynwin); free_windows(c->zonewin);
  for (void* p : c->profile_allocs) hipFree(p);
  if (c->stream && c->own_stream) hipStreamDestroy(c->stream);
  delete c;
}

namespace {
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
};
int to_dev(tj_ctx* c, DevBuf& b, const void* src, size_t bytes) {
  HIPCHK(c, hipMalloc(&b.p, std::max<size_t>(bytes, 8)));
  if (src && bytes) return upload(c, b.p, src, bytes);
  return TJ_OK;
}
}  // namespace

namespace {
struct EvPair {   // the two timing events of the device build, destroyed on every exit
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EvPair() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
};
// verts: [n][prim][3] in the caller's order.  Everything that can be refused is checked BEFORE the current obstacle set is
// touched; from the first free on the context counts as "no obstacles" (have_cloud = false, N = 0) until a new set is
// completely built, so a failed call can never leave tj_iterate with a half-built hierarchy.
int set_obstacles(tj_ctx* c, const double* verts, int n, int prim) {
  Dev& d = c->d;
  if (prim == 3 && d.optimal_plane && d.mode == TJ_MODE_SINGLE) {
    c->err = "triangle obstacles with optimal_plane:1 in single-UAV mode are not supported (Optimal_plane::optimal_cd is defined for obstacle points only, Optimal_plane.h:160)";
    return TJ_ERR_UNSUPPORTED;
  }
  // pyramid geometry: level 0 = boxes over 8 consecutive primitives, up to a top level of <= 64 boxes
  std::vector<int> lvl_off, lvl_n;
  if (n > 0) { int cnt = (n + 7) / 8, off = 0; for (;;) { lvl_off.push_back(off); lvl_n.push_back(cnt); off += cnt; if (cnt <= 64) break; cnt = (cnt + 7) / 8; } }
  if ((int)lvl_n.size() > MAX_LEVELS) { c->err = "too many obstacle primitives for MAX_LEVELS"; return TJ_ERR_UNSUPPORTED; }
  QUIESCE(c);
  c->have_cloud = false;
  d.N = 0; d.nlevels = 0; if (!c->hp.bvh_skip_forced) d.bvh_skip = 0; d.px = d.py = d.pz = d.tri = nullptr; d.boxes = d.leafbox = nullptr;
  for (void* p : c->cloud_allocs) hipFree(p);
  c->cloud_allocs.clear();
  c->cloud_order.clear(); c->cloud_rank.clear();
  c->q_order = nullptr;
  if (n > 0) {
    for (int k = 0; k < 3; k++) { c->cloud_lo[k] = INFINITY; c->cloud_hi[k] = -INFINITY; }
    for (size_t i = 0; i < (size_t)n * prim; i++) for (int k = 0; k < 3; k++) { c->cloud_lo[k] = std::min(c->cloud_lo[k], verts[3 * i + k]); c->cloud_hi[k] = std::max(c->cloud_hi[k], verts[3 * i + k]); }
    const size_t nbox = (size_t)lvl_off.back() + lvl_n.back();
    float* boxes; int r;
    if ((r = dalloc(c, &boxes, nbox * 6, &c->cloud_allocs))) return r;
    double *px = nullptr, *py = nullptr, *pz = nullptr, *tri = nullptr; float* lb = nullptr;
    if (prim == 1) { if ((r = dalloc(c, &px, n, &c->cloud_allocs)) || (r = dalloc(c, &py, n, &c->cloud_allocs)) || (r = dalloc(c, &pz, n, &c->cloud_allocs))) return r; }
    else if ((r = dalloc(c, &tri, (size_t)n * 9, &c->cloud_allocs)) || (r = dalloc(c, &lb, (size_t)n * 6, &c->cloud_allocs))) return r;
    std::vector<int> order(n);
    c->bvh_on_device = tune("BVH_HOST") ? 0 : 1;   // TJ_BVH_HOST=1: the host build of host_tables.h (the checker of the device build)
    if (!c->bvh_on_device) {
      HostBvh b;
      build_bvh(verts, n, prim, b);
      if ((r = upload(c, boxes, b.boxes.data(), b.boxes.size() * 4))) return r;
      if (prim == 1) { if ((r = upload(c, px, b.px.data(), (size_t)n * 8)) || (r = upload(c, py, b.py.data(), (size_t)n * 8)) || (r = upload(c, pz, b.pz.data(), (size_t)n * 8))) return r; }
      else if ((r = upload(c, tri, b.tri.data(), (size_t)n * 72)) || (r = upload(c, lb, b.leafbox.data(), (size_t)n * 24))) return r;
      order = b.order;
      c->bvh_build_ms = 0;
    } else {
      // device build (kernels_bvh.h): bounds -> Morton keys -> stable radix sort -> gather -> box pyramid
      DevBuf dv, dpart, dlohi, dkA, dkB, dvA, dvB, dhist, d64a, d64b;
      const int nb_red = std::min(1024, (n + 255) / 256), nblocks = (n + RS_TILE - 1) / RS_TILE;
      if ((r = to_dev(c, dv, verts, (size_t)n * prim * 24)) || (r = to_dev(c, dpart, nullptr, (size_t)nb_red * 48)) || (r = to_dev(c, dlohi, nullptr, 48)) ||
          (r = to_dev(c, dkA, nullptr, (size_t)n * 8)) || (r = to_dev(c, dkB, nullptr, (size_t)n * 8)) || (r = to_dev(c, dvA, nullptr, (size_t)n * 4)) || (r = to_dev(c, dvB, nullptr, (size_t)n * 4)) ||
          (r = to_dev(c, dhist, nullptr, (size_t)256 * nblocks * 4)) || (r = to_dev(c, d64a, nullptr, (size_t)lvl_n[0] * 48)) || (r = to_dev(c, d64b, nullptr, (size_t)(lvl_n.size() > 1 ? lvl_n[1] : 1) * 48))) return r;
      EvPair ev;
      HIPCHK(c, hipEventCreate(&ev.e0)); HIPCHK(c, hipEventCreate(&ev.e1));
      hipStream_t s = c->stream;
      HIPCHK(c, hipEventRecord(ev.e0, s));
      const double* V = (const double*)dv.p;
      hipLaunchKernelGGL(k_bvh_bounds, dim3(nb_red), dim3(256), 0, s, V, n, prim, (double*)dpart.p);
      hipLaunchKernelGGL(k_bvh_bounds_final, dim3(1), dim3(64), 0, s, (const double*)dpart.p, nb_red, (double*)dlohi.p);
      unsigned long long *kA = (unsigned long long*)dkA.p, *kB = (unsigned long long*)dkB.p; int *vA = (int*)dvA.p, *vB = (int*)dvB.p;
      hipLaunchKernelGGL(k_bvh_keys, dim3((n + 255) / 256), dim3(256), 0, s, V, n, prim, (const double*)dlohi.p, kA, vA);
      for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(k_rsort_hist, dim3(nblocks), dim3(RS_THREADS), 0, s, kA, n, 8 * pass, nblocks, (int*)dhist.p);
        hipLaunchKernelGGL(k_rsort_scan, dim3(1), dim3(1024), 0, s, (int*)dhist.p, 256 * nblocks);
        hipLaunchKernelGGL(k_rsort_scatter, dim3(nblocks), dim3(RS_THREADS), 0, s, kA, vA, n, 8 * pass, nblocks, (const int*)dhist.p, kB, vB);
        std::swap(kA, kB); std::swap(vA, vB);
      }
      hipLaunchKernelGGL(k_bvh_gather, dim3((n + 255) / 256), dim3(256), 0, s, V, vA, n, prim, px, py, pz, tri, lb);
      double *cur = (double*)d64a.p, *prev = (double*)d64b.p;
      for (size_t lv = 0; lv < lvl_n.size(); lv++) {
        const int nchild = lv == 0 ? n : lvl_n[lv - 1];
        hipLaunchKernelGGL(k_bvh_level, dim3((lvl_n[lv] + 255) / 256), dim3(256), 0, s, (int)lv, lvl_n[lv], nchild, prim, px, py, pz, tri, prev, cur, boxes + (size_t)lvl_off[lv] * 6);
        std::swap(cur, prev);
      }
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(ev.e1, s));
      HIPCHK(c, hipStreamSynchronize(s));
      float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1)); c->bvh_build_ms = ms;
      HIPCHK(c, hipMemcpy(order.data(), vA, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    // the build succeeded: publish it
    c->cloud_order.swap(order);
    d.boxes = boxes; d.px = px; d.py = py; d.pz = pz; d.tri = tri; d.leafbox = lb;
    d.nlevels = (int)lvl_n.size();
    // two levels per step at the top of the walk (kernels_sep.h): pays where the pyramid is deep AND the query waves outnumber the resident slots, i.e. where a
    // query's latency is the launch's throughput (256 robots x 1 M primitives: k_front 40.2 -> 36.3 us, k_ccd 34.0 -> 31.0); 64 robots through 1 M points: no change
    if (!c->hp.bvh_skip_forced) d.bvh_skip = (d.nlevels >= 5 && (d.u1 - d.u0) * d.S > 3584) ? 1 : 0;
    for (int i = 0; i < d.nlevels; i++) { d.lvl_off[i] = lvl_off[i]; d.lvl_n[i] = lvl_n[i]; }
    d.N = n;
  }
  d.prim = prim;
  c->have_cloud = true;
  return TJ_OK;
}
}  // namespace

int tj_set_cloud(tj_ctx* c, const double* xyz, int n) {
  if (!c || n < 0 || (n > 0 && !xyz)) return TJ_ERR_INVALID;
  return set_obstacles(c, xyz, n, 1);
}

int tj_set_mesh(tj_ctx* c, const double* vertices, int n_vertices, const int* faces, int n_faces) {
  if (!c || n_vertices < 0 || n_faces < 0 || (n_faces > 0 && (!vertices || !faces))) return TJ_ERR_INVALID;
  std::vector<double> tri((size_t)n_faces * 9);
  for (int f = 0; f < n_faces; f++)
    for (int j = 0; j < 3; j++) {
      const int v = faces[3 * (size_t)f + j];
      if (v < 0 || v >= n_vertices) { c->err = "tj_set_mesh: face " + std::to_string(f) + " refers to vertex " + std::to_string(v); return TJ_ERR_INVALID; }
      for (int k = 0; k < 3; k++) tri[(size_t)f * 9 + 3 * j + k] = vertices[3 * (size_t)v + k];
    }
  return set_obstacles(c, tri.data(), n_faces, 3);
}

int tj_init_state(tj_ctx* c, const double* wp, double pt0) {
  if (!c || !wp) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  const int U = d.U, P = d.P, T = d.T;
  HostTables t;
  build_tables(P, d.res, 1, t);
  std::vector<double> spline((size_t)U * 3 * T), p_slack((size_t)U * 18 * P), zeros((size_t)U * 18 * P, 0.0), ts((size_t)U * P, pt0), tz((size_t)U * P, 0.0), ptv(U, pt0);
  for (int u = 0; u < U; u++) {
    double* s = &spline[(size_t)u * 3 * T];
    for (int a = 0; a < 3; a++) {
      auto W = [&](int k) { return wp[((size_t)u * (P + 1) + k) * 3 + a]; };
      double* col = s + T * a;
      col[0] = W(0);
      if (d.mode == TJ_MODE_SINGLE) {  // Main/admmPathPlanning3D.cpp:258-275
        for (int i = 0; i < P; i++) {
          const double head = 0.9 * W(i) + 0.1 * W(i + 1), tail = 0.9 * W(i + 1) + 0.1 * W(i);
          col[3 * i + 1] = W(i);
          for (int j = 1; j < 3; j++) col[j + 3 * i + 1] = double(2 - j) / 1 * head + (double)(j - 1) / 1 * tail;
          col[3 * (i + 1) + 1] = W(i + 1);
        }
      } else {  // Main/multiPathPlanning3D.cpp:363-375
        for (int k = 0; k < P; k++)
          for (int j = 0; j <= 3; j++) col[j + 3 * k + 1] = double(3 - j) / 3 * W(k) + (double)j / 3 * W(k + 1);
      }
      col[T - 1] = W(P);
      col[1] = col[0];
      col[T - 2] = col[T - 1];
    }
    for (int sp = 0; sp < P; sp++)
      for (int a = 0; a < 3; a++)
        for (int j = 0; j < 6; j++) {
          double acc = 0;
          for (int k = 0; k < 6; k++) acc += t.convert[sp * 36 + j * 6 + k] * s[sp * 3 + k + T * a];
          p_slack[(size_t)u * 18 * P + sp * 6 + j + 6 * P * a] = acc;
        }
  }
  QUIESCE(c);
  int r;
  // 1. the state
  if ((r = store(c, d.spline, 0, spline.data(), spline.size())) || (r = store(c, d.p_slack, 0, p_slack.data(), p_slack.size())) ||
      (r = store(c, d.p_lambda, 0, zeros.data(), zeros.size())) || (r = store(c, d.t_slack, 0, ts.data(), ts.size())) ||
      (r = store(c, d.t_lambda, 0, tz.data(), tz.size())) || (r = store(c, d.piece_time, 0, ptv.data(), ptv.size()))) return r;
  // 2. every array the table says is filled (device_arrays: ZERO, ONES).  The conditions this loop no longer states: xf_seg was cleared with Dev::xf only (without it nothing
  // reads the counters), pairstamp and pairbits in the multi-UAV modes and kpair_on outside mode 0 only (else each is the one-element placeholder, which nothing reads);
  // the optimal_plane tables are declared, and so filled, with optimal_plane only, as before
  for (const ArrayDecl& a : c->arrays)
    if (a.reset) HIPCHK(c, hipMemsetAsync(*a.slot, a.reset == ONES ? 0xff : 0, a.n * a.elem, c->stream));
  // 3. what is not a plain fill (the two stores come last: each waits for the stream, and so for every fill above)
  // direct exchange (the counters live in the exchange block, not in a context array): the push / arrival counts restart (the caller has every rank drained before any
  // rank calls this, and a barrier after: tj_group_init_state does; processes use their collective's barrier)
  if (c->xch_block) HIPCHK(c, hipMemsetAsync(d.xcnt, 0, 2 * XCH_MAX * sizeof(unsigned long long), c->stream));
  if ((r = restart_pairings(c, true))) return r;
  Ctl h; memset(&h, 0, sizeof(h)); h.gnorm = 1.0;  // Main/multiPathPlanning3D.cpp:594
  if ((r = store(c, d.ctl, 0, &h, 1))) return r;
  std::vector<int> idp(array_count(c, d.grad_perm));   // k_grad's launch order: no history, identity
  for (size_t i = 0; i < idp.size(); i++) idp[i] = (int)i;
  if ((r = store(c, d.grad_perm, 0, idp.data(), idp.size()))) return r;
  c->hull_valid = false; c->ss.ccd_valid = false;
  c->have_state = true;
  return TJ_OK;
}

// the six state arrays and their doubles per robot, in the argument order of tj_get_state / tj_set_state
struct StateArrays {
  struct { double* dev; size_t per; } v[6];
  explicit StateArrays(const Dev& d) : v{{d.spline, (size_t)3 * d.T}, {d.p_slack, (size_t)18 * d.P}, {d.p_lambda, (size_t)18 * d.P}, {d.t_slack, (size_t)d.P}, {d.t_lambda, (size_t)d.P}, {d.piece_time, 1}} {}
};

int tj_get_state(tj_ctx* c, int u, double* spline, double* p_slack, double* p_lambda, double* t_slack, double* t_lambda, double* piece_time) {
  if (!c || u < 0 || u >= c->d.U) return TJ_ERR_INVALID;
  QUIESCE(c);
  double* const host[6] = {spline, p_slack, p_lambda, t_slack, t_lambda, piece_time};
  const StateArrays st(c->d);
  for (int i = 0; i < 6; i++) if (host[i]) { int r = fetch(c, host[i], st.v[i].dev, u * st.v[i].per, st.v[i].per); if (r) return r; }
  return TJ_OK;
}

int tj_set_state(tj_ctx* c, int u, const double* spline, const double* p_slack, const double* p_lambda, const double* t_slack, const double* t_lambda, double piece_time) {
  if (!c || u < 0 || u >= c->d.U) return TJ_ERR_INVALID;
  QUIESCE(c);
  const double* const host[6] = {spline, p_slack, p_lambda, t_slack, t_lambda, &piece_time};
  const StateArrays st(c->d);
  for (int i = 0; i < 6; i++) if (host[i]) { int r = store(c, st.v[i].dev, u * st.v[i].per, host[i], st.v[i].per); if (r) return r; }
  c->hull_valid = false; c->ss.ccd_valid = false;
  c->have_state = true;
  return TJ_OK;
}

namespace {
// the parts of tj_iterate_async (also used by the lockstep enqueue of the ranks of a group that share a device, tj_group.h)
int iterate_async_prologue(tj_ctx* c, int n_iters) {
  if (c->hp.heal && n_iters > 0 && (c->ss.xs_two_queues || c->ss.keep_two_queues)) {   // self-healing: the state this batch starts from (one launch), unless iterations the host has not looked at yet are already outstanding
    if (c->snap_iters == 0 && !c->heal_busy) { int r = checkpoint_take(c, !c->begin_folded); if (r) return r; }   // (no begin folded: the batch's first launch is k_begin)
    if (!c->heal_busy) c->snap_iters += n_iters;
  }
  if (n_iters > 0) { int r = ensure_hull_cache(c); if (r) return r; }
  return TJ_OK;
}

// chain position of iteration i of a batch of n: inside a batch the begin work of iteration i+1 rides on iteration i's line search (chain_position, host_launch.h).
// Clears begin_folded: the fold it reports is consumed here
int iterate_async_pos(tj_ctx* c, int i, int n) {
  const int pos = chain_position(c->d, c->hp, true, i > 0 || c->begin_folded, i + 1 < n);
  c->begin_folded = false;
  return pos;
}
}  // namespace

int tj_iterate_async(tj_ctx* c, int n_iters) {
  if (!c || n_iters < 0) return TJ_ERR_INVALID;
  if (!ready(c)) return TJ_ERR_INVALID;
  { int r = iterate_async_prologue(c, n_iters); if (r) return r; }
  for (int i = 0; i < n_iters; i++)
    if (int r = enqueue_iteration(c, iterate_async_pos(c, i, n_iters))) return r;
  return TJ_OK;
}

int tj_sync(tj_ctx* c) {
  if (!c) return TJ_ERR_INVALID;
  QUIESCE_NOHEAL(c);   // (no read-back here: a batch that has to be run again -- heal_check -- is noticed by the next call that reads a result or the statistics)
  return TJ_OK;
}

void* tj_stream(tj_ctx* c) { return c ? (void*)c->stream : nullptr; }

int tj_set_stream(tj_ctx* c, void* hip_stream) {
  if (!c) return TJ_ERR_INVALID;
  QUIESCE(c);
  if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
  c->stream = (hipStream_t)hip_stream;
  c->own_stream = false;
  return TJ_OK;
}

int tj_profile_kernels(tj_ctx* c, int n_iters, double* ms, int* launches) {
  if (!c || !ms || n_iters < 0) return TJ_ERR_INVALID;
  if (!ready(c)) return TJ_ERR_INVALID;
  { int fr = flush_deferred(c); if (fr) return fr; }
  { int hr = ensure_hull_cache(c); if (hr) return hr; }
  std::vector<hipEvent_t> ev((size_t)n_iters * (K_COUNT + 1));
  for (auto& e : ev) HIPCHK(c, hipEventCreate(&e));
  std::vector<int> ran(K_COUNT, 0);
  c->ss.xs_same_queue_now = true;   // per-kernel events on one queue: the asynchronous solve follows k_grad there (its own time is then what the events show)
  for (int it = 0; it < n_iters; it++) {
    hipEvent_t* e = &ev[(size_t)it * (K_COUNT + 1)];
    HIPCHK(c, hipEventRecord(e[0], c->stream));
    const int pos = chain_position(c->d, c->hp, false, it > 0, it + 1 < n_iters);   // (the flush above has taken a folded begin back; the one-launch coupled search is profiled with a k_begin per iteration)
    for (int k = 0; k < K_COUNT; k++) {
      if (enqueue_kernel(c, Sched::Chain, pos, k)) ran[k]++;
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(e[k + 1], c->stream));
    }
  }
  c->ss.xs_same_queue_now = false;
  if (n_iters > 0) c->maybe_deferred = true;  // the last iteration's slack/dual update is still owed (paid by the flush below)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < K_COUNT; k++) ms[k] = 0;
  for (int it = 0; it < n_iters; it++)
    for (int k = 0; k < K_COUNT; k++) {
      float t = 0;
      HIPCHK(c, hipEventElapsedTime(&t, ev[(size_t)it * (K_COUNT + 1) + k], ev[(size_t)it * (K_COUNT + 1) + k + 1]));
      if (ran[k]) ms[k] += t;
    }
  for (auto& e : ev) hipEventDestroy(e);
  if (launches) for (int k = 0; k < K_COUNT; k++) launches[k] = ran[k];
  return check_device_errors(c);
}

long long tj_launch_count(tj_ctx* c) { return c ? c->launches : -1; }
int tj_kernel_count(void) { return K_COUNT; }
const char* tj_kernel_name(int i) { return (i >= 0 && i < K_COUNT) ? kKernelNames[i] : ""; }

int tj_iterate(tj_ctx* c, int n_iters, double* gnorm, int* iters_total, int* converged) {
  int r = tj_iterate_async(c, n_iters);
  if (r) return r;
  if ((r = flush_deferred(c))) return r;
  Ctl h;
  r = check_device_errors(c, &h);
  // the iteration counter of the last started iteration is committed by the next k_begin
  const int it = h.iter + h.pending;
  if (gnorm) *gnorm = h.gnorm;
  if (iters_total) *iters_total = it;
  if (converged) *converged = h.done || (c->d.stop > 0 && it > 1 && h.gnorm < c->d.stop);
  return r;
}

int tj_run_stage(tj_ctx* c, int stage) {
  if (!c) return TJ_ERR_INVALID;
  if (!ready(c)) return TJ_ERR_INVALID;
  int r = flush_deferred(c);
  if (r) return r;
  if ((r = enqueue_stage(c, stage))) return r;
  return check_device_errors(c);
}

int tj_phase_count(tj_ctx* c) { return c ? (c->d.mode == TJ_MODE_MULTI_COUPLED ? 6 : 3) : TJ_ERR_INVALID; }

int tj_iterate_phase_chained(tj_ctx* c, int phase, int more) {
  if (!c || phase < 0 || phase >= tj_phase_count(c)) return TJ_ERR_INVALID;
  if (!ready(c)) return TJ_ERR_INVALID;
  // eager launches: measured faster than three graph replays per iteration (a replay costs ~10-16 us of host time, a
  // plain launch ~3.5 us, and a phase has only 2-7 kernels).  No flush here: the slack/dual update an iteration owes is
  // paid by k_mid of the next iteration's phase 1 (or by tj_sync / any state access).
  // Decoupled / single-UAV schedules fold the next iteration's begin into the last phase's k_linesearch when the caller says one follows
  // (more != 0): that iteration's phase 0 then launches nothing.  A begin that was folded for an iteration the caller never enqueues is
  // taken back by the next flush (tj_sync, any state access).
  int pos = 0;   // (coupled mode commits in a phase of its own: no fold, chain_position's wide_coupled = false)
  if (phase == 0) { pos = chain_position(c->d, c->hp, false, c->begin_folded, false); if (c->d.mode != TJ_MODE_MULTI_COUPLED) c->begin_folded = false; }
  if (phase == 2 && more) { pos = chain_position(c->d, c->hp, false, false, true); if (pos) c->begin_folded = true; }
  if (phase == 0) c->ss.lsc_base = 0;
  return enqueue_body(c, phase, pos);
}

// Coupled mode, sharded contexts: the Armijo search on the summed energy to the reference's own end (Optimization3D_multi.h:605-636: no bound).  One exchange carries the
// candidates of LSC_ROUNDS rounds (steps 0.8^0 .. 0.8^30 in the first table).  With `follow` on, phase 5 commits nothing when none of them passes and the caller asks here
// (the stream is drained: this is the one host look of the schedule, paid only by callers that want the exact loop): pending = 1 -> run phase 4, exchange buffer 4, phase 5
// again -- they evaluate, carry and decide the NEXT rounds -- and ask again.  Every rank of the sharded run reads the same answer (same gathered table, same decision).
int tj_set_coupled_follow(tj_ctx* c, int on) {
  if (!c) return TJ_ERR_INVALID;
  if (c->d.mode != TJ_MODE_MULTI_COUPLED) { c->err = "tj_set_coupled_follow: coupled mode only"; return TJ_ERR_INVALID; }
  c->d.lsc_follow = on ? 1 : 0; c->ss.lsc_base = 0;
  return TJ_OK;
}
int tj_coupled_search_pending(tj_ctx* c, int* pending) {
  if (!c || !pending) return TJ_ERR_INVALID;
  *pending = 0;
  if (!c->d.lsc_follow || c->d.u1 - c->d.u0 == c->d.U) return TJ_OK;   // (one context follows the search inside its own launch: lsc_continue)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int p = 0;
  HIPCHK(c, hipMemcpy(&p, &c->d.ctl->lsc_pending, sizeof(int), hipMemcpyDeviceToHost));
  *pending = p ? 1 : 0;
  c->ss.lsc_base = p ? c->ss.lsc_base + LSC_ROUNDS : 0;
  if (!p) c->maybe_deferred = true;   // the step is committed: the iteration's slack/dual update is owed from here on
  return TJ_OK;
}
int tj_iterate_phase(tj_ctx* c, int phase) { return tj_iterate_phase_chained(c, phase, 0); }

int tj_exchange_buffer(tj_ctx* c, int what, void** dev_ptr, int* doubles_per_robot, int* first_owned, int* n_owned) {
  if (!c || what < 0 || what > 4) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  if (what >= 2 && d.mode != TJ_MODE_MULTI_COUPLED) { c->err = "tj_exchange_buffer: buffers 2..4 exist in coupled mode only"; return TJ_ERR_INVALID; }
  void* p = nullptr; int per = 0;
  switch (what) {
    case 0: p = d.spline; per = 3 * d.T; break;
    case 1: p = d.xdir; per = d.xs; break;
    case 2: p = d.xcorner; per = 4; break;                       // Schur-corner contributions of the shared piece_time
    case 3: p = d.k_obs_f; per = 1; break;                       // obstacle CCD exponent of every robot (as a double)
    case 4: p = d.ls_e; per = LSC_ROUNDS * LS_GROUPS; break;     // energies of the Armijo candidates
  }
  if (dev_ptr) *dev_ptr = p;
  if (doubles_per_robot) *doubles_per_robot = per;
  if (first_owned) *first_owned = d.u0;
  if (n_owned) *n_owned = d.u1 - d.u0;
  return TJ_OK;
}

int tj_get_planes(tj_ctx* c, int u, int* counts_obs, int* counts_self, double* planes, int cap) {
  if (!c || u < 0 || u >= c->d.U) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  std::vector<int> co(d.S), cs(d.S, 0);
  int r;
  if ((r = fetch(c, co.data(), d.ocount, (size_t)u * d.S, d.S)) || (d.mode >= 1 && (r = fetch(c, cs.data(), d.scount, (size_t)u * d.S, d.S)))) return r;
  int total = 0;
  for (int tr = 0; tr < d.S; tr++) total += co[tr] + cs[tr];
  if (counts_obs) memcpy(counts_obs, co.data(), d.S * sizeof(int));
  if (counts_self) memcpy(counts_self, cs.data(), d.S * sizeof(int));
  if (planes) {
    if (cap < total) { c->err = "tj_get_planes: buffer too small"; return TJ_ERR_INVALID; }
    size_t w = 0;
    for (int tr = 0; tr < d.S; tr++) {
      if (co[tr] && (r = fetch(c, planes + 4 * w, d.oplanes, ((size_t)u * d.S + tr) * d.cap_obs * 4, (size_t)co[tr] * 4))) return r;
      w += co[tr];
      if (cs[tr] && (r = fetch(c, planes + 4 * w, d.splanes, ((size_t)u * d.S + tr) * d.cap_self * 4, (size_t)cs[tr] * 4))) return r;
      w += cs[tr];
    }
  }
  return total;
}

int tj_get_candidates(tj_ctx* c, int u, int seg, int cap, int* ids, int* n_broad) {
  if (!c || u < 0 || u >= c->d.U || seg < 0 || seg >= c->d.S || cap < 0) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  const size_t s = (size_t)u * d.S + seg;
  int n = 0, r;
  if ((r = fetch_ids(c, d.ocand_n, d.ocand, s, cap, ids, n))) return r;
  if (n_broad) {
    unsigned long long st[6];
    if ((r = fetch(c, st, d.seg_stats, s * 6, 6))) return r;
    *n_broad = (int)st[1];
  }
  return n;
}

int tj_set_planes(tj_ctx* c, int u, const int* counts, const double* planes) {
  if (!c || u < 0 || u >= c->d.U || !counts) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  size_t w = 0;
  std::vector<int> zero(d.S, 0);
  for (int tr = 0; tr < d.S; tr++) {
    if (counts[tr] > d.cap_obs) { c->err = "tj_set_planes: more planes than cap_obs"; return TJ_ERR_CAPACITY; }
    if (counts[tr]) { int ur = store(c, d.oplanes, ((size_t)u * d.S + tr) * d.cap_obs * 4, planes + 4 * w, (size_t)counts[tr] * 4); if (ur) return ur; }
    w += counts[tr];
  }
  { int ur; if ((ur = store(c, d.ocount, (size_t)u * d.S, counts, d.S)) || (ur = store(c, d.scount, (size_t)u * d.S, zero.data(), d.S))) return ur; }
  return TJ_OK;
}

int tj_get_direction(tj_ctx* c, int u, double* direction, double* t_direction, double* wolfe, double* gn) {
  if (!c || u < 0 || u >= c->d.U) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  std::vector<double> rec(d.xs);
  if (int r = fetch(c, rec.data(), d.xdir, (size_t)u * d.xs, d.xs)) return r;
  if (direction) memcpy(direction, rec.data(), 3 * d.T * sizeof(double));
  if (t_direction) *t_direction = rec[3 * d.T];
  if (wolfe) *wolfe = rec[3 * d.T + 1];
  if (gn) *gn = rec[3 * d.T + 2];
  if (d.mode == TJ_MODE_MULTI_COUPLED) {  // one Newton system for all robots: report its global wolfe and gnorm
    Ctl h;
    if (int r = fetch(c, &h, d.ctl, 0, 1)) return r;
    if (wolfe) *wolfe = h.wolfe_c;
    if (gn) *gn = h.gnorm;
  }
  return TJ_OK;
}

int tj_set_direction(tj_ctx* c, int u, const double* direction, double t_direction, double wolfe, double gn) {
  if (!c || u < 0 || u >= c->d.U || !direction) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  std::vector<double> rec(d.xs, 0.0);
  memcpy(rec.data(), direction, 3 * d.T * sizeof(double));
  rec[3 * d.T] = t_direction; rec[3 * d.T + 1] = wolfe; rec[3 * d.T + 2] = gn;
  c->ss.ccd_valid = false;   // the swept-hull cache no longer matches: the next chained CCD stage rebuilds it (k_ccd_prep)
  return store(c, d.xdir, (size_t)u * d.xs, rec.data(), d.xs);
}

int tj_get_local_grad(tj_ctx* c, int u, int piece, double* g19, double* h361) {
  if (!c || u < 0 || u >= c->d.U || piece < 0 || piece >= c->d.P) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  const int r = g19 ? fetch(c, g19, d.lg, ((size_t)u * d.P + piece) * 19, 19) : TJ_OK;
  return (r || !h361) ? r : fetch(c, h361, d.lh, ((size_t)u * d.P + piece) * 361, 361);
}

int tj_get_energy(tj_ctx* c, double* energy) {
  if (!c || !energy) return TJ_ERR_INVALID;
  if (!ready(c)) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  DevBuf out;
  { int r = to_dev(c, out, nullptr, (size_t)d.U * 8); if (r) return r; }
  HIPCHK(c, hipMemsetAsync(out.p, 0, (size_t)d.U * 8, c->stream));
  HIPCHK(c, hipFuncSetAttribute((const void*)k_energy, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->hp.lds_ls));
  hipLaunchKernelGGL(k_energy, dim3(d.u1 - d.u0), dim3(LS_THREADS), c->hp.lds_ls, c->stream, d, c->hp.lsl, (double*)out.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(energy, out.p, (size_t)d.U * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return TJ_OK;
}

}  // extern "C"

namespace {
// ---- the read-only queries: one path for the fourteen (the kernels: kernels_zone_windows.h, kernels_dynamics_windows.h, kernels_sight_windows.h, kernels_audit.h, kernels_audit_timed.h, kernels_closest.h, kernels_obstacle_approach.h, kernels_obstacle_windows.h, kernels_pair_approach.h, kernels_path_crossing.h, kernels_timing_margin.h, kernels_proximity.h, kernels_flight_profile.h, kernels_peak_dynamics.h) ----
// The `*_run` functions serve the public call and the group's (tj_group.h).  net_host [U][3][T] / pt_host [U]: every robot's control points / piece_time as a group read them from
// the owners, or null = the context's own.  Argument checks in one precedence: null -> NaN -> limits -> no state -> sharded.
int query_nan(tj_ctx* c, const char* name, const char* what, double v) {
  if (v == v) return TJ_OK;
  c->err = std::string(name) + ": " + what + " is NaN"; return TJ_ERR_INVALID;
}
// is there a state to look at, and (owners: the query reads every robot's piece_time) does a sharded context get the owners' values handed in
int query_state(tj_ctx* c, const char* name, bool owners, bool handed_in) {
  if (!c->have_state) { c->err = "tj_init_state has not been called"; return TJ_ERR_INVALID; }
  if (owners && c->d.multi() && c->d.world > 1 && !handed_in) {
    c->err = std::string(name) + ": a sharded context does not hold the other ranks' piece_time as their owners have it; use tj_group_" + (name + 3);
    return TJ_ERR_UNSUPPORTED;
  }
  return TJ_OK;
}
double query_range(const Dev& d, double range) { return range > 0 ? range : d.offset + 2 * d.margin; }
// (range, tol, max_depth, max_windows) of the four branch-and-bound queries, checked (NaN, then the limits) and defaulted in one place from one table: the call's
// and its group call's name, the limits, the defaults, and the reason clause each limit's message ends on (the two row-listing queries size their lists by the call).
// first_is_offset: the first argument is a contact distance and defaults to offset, not to the audit range; tol_fraction > 0: the default tolerance is that fraction of
// the first argument over vel_limit (a time) instead of `tol`; inf_as_offset: of offset where the first argument is infinite (no time resolves 1 % of an infinite distance)
struct SearchSpec { const char* name; const char* group_name; int depth_limit, window_limit; double tol; int windows; const char* depth_why; const char* windows_why; bool first_is_offset = false; double tol_fraction = 0.0; bool inf_as_offset = false; };
const SearchSpec SEARCH_CLOSEST{"tj_closest_approach", "tj_group_closest_approach", TJ_CLOSEST_MAX_DEPTH, TJ_CLOSEST_FRONTIER, TJ_CLOSEST_TOL, TJ_CLOSEST_FRONTIER,
                                ": deeper windows cannot be halved in a double", ": the live list's capacity"},
                 SEARCH_PAIR{"tj_pair_approach", "tj_group_pair_approach", TJ_PAIR_MAX_DEPTH, TJ_PAIR_MAX_WINDOWS, TJ_PAIR_TOL, TJ_PAIR_FRONTIER,
                             ": deeper windows cannot be halved in a double", ""},
                 SEARCH_CROSSING{"tj_path_crossings", "tj_group_path_crossings", TJ_CROSSING_MAX_DEPTH, TJ_CROSSING_MAX_WINDOWS, TJ_CROSSING_TOL, TJ_CROSSING_FRONTIER,
                                 ": deeper windows cannot be halved in a double", ""},
                 SEARCH_MARGIN{"tj_timing_margin", "tj_group_timing_margin", TJ_MARGIN_MAX_DEPTH, TJ_MARGIN_MAX_WINDOWS, 0.0, TJ_MARGIN_FRONTIER,
                               ": deeper windows cannot be halved in a double", "", true, TJ_MARGIN_TOL_FRACTION},
                 SEARCH_PROXIMITY{"tj_proximity_windows", "tj_group_proximity_windows", TJ_PROXIMITY_MAX_DEPTH, TJ_PROXIMITY_MAX_WINDOWS, 0.0, TJ_PROXIMITY_FRONTIER,
                                  ": deeper windows cannot be halved in a double", "", true, TJ_PROXIMITY_TOL_FRACTION, true},
                 SEARCH_OBSTACLE{"tj_obstacle_approach", "tj_group_obstacle_approach", TJ_OBSTACLE_MAX_DEPTH, TJ_OBSTACLE_FRONTIER, TJ_OBSTACLE_TOL, TJ_OBSTACLE_FRONTIER,
                                 ": deeper windows are not dyadic in a double", ": the live list's capacity"},
                 SEARCH_OBSWIN{"tj_obstacle_windows", "tj_group_obstacle_windows", TJ_OBSWIN_MAX_DEPTH, TJ_OBSWIN_MAX_WINDOWS, 0.0, TJ_OBSWIN_FRONTIER,
                               ": deeper windows are not dyadic in a double", ": the in-kernel rank sort's bound", true, TJ_OBSWIN_TOL_FRACTION, true},
                 SEARCH_SIGHT{"tj_sight_windows", "tj_group_sight_windows", TJ_SIGHT_MAX_DEPTH, TJ_SIGHT_MAX_WINDOWS, 0.0, TJ_SIGHT_FRONTIER,
                              ": deeper windows cannot be halved in a double", ": the in-kernel rank sort's bound", true, TJ_SIGHT_TOL_FRACTION, true},
                 SEARCH_DYNWIN{"tj_dynamics_windows", "tj_group_dynamics_windows", TJ_DYNWIN_MAX_DEPTH, TJ_DYNWIN_MAX_WINDOWS, 0.0, TJ_DYNWIN_FRONTIER,
                               ": deeper windows are not dyadic in a double", ": the in-kernel rank sort's bound"},
                 SEARCH_ZONEWIN{"tj_zone_windows", "tj_group_zone_windows", TJ_ZONEWIN_MAX_DEPTH, TJ_ZONEWIN_MAX_WINDOWS, 0.0, TJ_ZONEWIN_FRONTIER,
                                ": deeper windows are not dyadic in a double", ": the in-kernel rank sort's bound", true, TJ_ZONEWIN_TOL_FRACTION};
struct SearchArgs {
  double range, tol; int max_depth, max_windows;
  template <class Args> void put(Args& a) const { a.range = range; a.tol = tol; a.max_depth = max_depth; a.max_windows = max_windows; }
};
int search_args(tj_ctx* c, const SearchSpec& q, double range, double tol, int max_depth, int max_windows, SearchArgs& a) {
  int r;
  if ((r = query_nan(c, q.name, q.first_is_offset ? "dist" : "range", range)) || (r = query_nan(c, q.name, "tol", tol))) return r;
  if (max_depth > q.depth_limit) { c->err = std::string(q.name) + ": max_depth must be 0.." + std::to_string(q.depth_limit) + " (or negative for the default)" + q.depth_why; return TJ_ERR_INVALID; }
  if (max_windows > q.window_limit) {
    c->err = std::string(q.name) + ": max_windows must be 1.." + std::to_string(q.window_limit) + " (or <= 0 for the default)" + q.windows_why;
    return TJ_ERR_INVALID;
  }
  const double first = q.first_is_offset ? (range > 0 ? range : c->d.offset) : query_range(c->d, range);
  a = SearchArgs{first, tol < 0 ? (q.tol_fraction > 0 ? (q.tol_fraction * (q.inf_as_offset && first == INFINITY ? c->d.offset : first)) / c->d.vel_limit : q.tol) : tol, max_depth < 0 ? q.depth_limit : max_depth, max_windows <= 0 ? q.windows : max_windows};
  return TJ_OK;
}
// sorted primitive -> index in the caller's obstacle list, made by whichever query needs it first
int ensure_order(tj_ctx* c) {
  int r;
  if (c->d.N > 0 && !c->q_order && ((r = dalloc(c, &c->q_order, c->d.N, &c->cloud_allocs)) || (r = upload(c, c->q_order, c->cloud_order.data(), (size_t)c->d.N * 4)))) return r;
  return TJ_OK;
}
// what the kernels read as the fleet's control nets and piece times: the staged copy of what a group handed in, or the context's own
int query_inputs(tj_ctx* c, const double* net_host, const double* pt_host, const double*& net, const double*& pt) {
  const Dev& d = c->d;
  const size_t net_n = (size_t)d.U * 3 * d.T;
  int r;
  if (net_host && ((r = query_buf(c, c->q_net, net_n)) || (r = upload(c, c->q_net, net_host, net_n * 8)))) return r;
  if (pt_host && ((r = query_buf(c, c->q_pt, d.U)) || (r = upload(c, c->q_pt, pt_host, (size_t)d.U * 8)))) return r;
  net = net_host ? c->q_net : d.spline; pt = pt_host ? c->q_pt : d.piece_time;
  return TJ_OK;
}
// the Dev of a query that walks the BVH: the walk reports a frontier overflow through Dev::ctl -- the queries' own block, zeroed for this call, never the solver's
int walk_dev(tj_ctx* c, Dev& da) {
  int r = query_buf(c, c->q_ctl, 1);
  if (r) return r;
  HIPCHK(c, hipMemsetAsync(c->q_ctl, 0, sizeof(Ctl), c->stream));
  da = c->d; da.ctl = c->q_ctl;
  return TJ_OK;
}
// the end of every query: the records (and whatever else is queued) are waited for; walk != null: the query of that name walked the BVH, and its overflow bit is read back
int query_finish(tj_ctx* c, const char* walk) {
  int err = 0;
  HIPCHK(c, hipGetLastError());
  if (walk) HIPCHK(c, hipMemcpyAsync(&err, &c->q_ctl->error, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (err & ERR_FRONT_OVERFLOW) { c->err = std::string(walk) + ": the BVH frontier of a segment overflowed at this range (more than " + std::to_string(FRONT_CAP) + " boxes of 8 primitives near one hull): lower `range`"; return TJ_ERR_CAPACITY; }
  return TJ_OK;
}

// ---- what the row-listing and the sampling queries share on the host (listed_run, proximity_run, obswin_run, sight_run, slot_run of dynwin_run and zonewin_run, profile_run) ----
// rows_finish ends every row-listing call; rows_args_ok, rows_begin and rows_end are the window queries' whose device counts the rows (proximity_run keeps its own tail: its *n = -1 rule)
// the refusal of a call whose buffers would exceed its query's byte budget, up front, nothing allocated.  what: the call's sizes in its words; advice: what to lower
int query_budget(tj_ctx* c, const std::string& what, size_t bytes, const char* budget, long long max_bytes, const char* advice) {
  if (bytes <= (size_t)max_bytes) return TJ_OK;
  c->err = what + " need " + std::to_string(bytes) + " bytes of device memory, more than " + budget + " (" + std::to_string(max_bytes) + "): " + advice;
  return TJ_ERR_INVALID;
}
// grow the buffers on `list`: the context is quiet, nothing reads the old ones.  They are freed, reset() puts the holder back to "nothing held" -- a failure keeps what
// it got on the list and starts over next time -- and alloc() -> rc allocates at the new sizes, which the caller records once this returns TJ_OK
template <class Reset, class Alloc>
int query_grow(std::vector<void*>& list, Reset&& reset, Alloc&& alloc) {
  for (void* p : list) hipFree(p);
  list.clear();
  reset();
  return alloc();
}
// the same for a Listed: grown to the largest cap and max_windows so far; alloc(sized, gc, gm, list) -> rc allocates everything but the rows
template <class Held, class Alloc>
int listed_grow(tj_ctx* c, Held& h, int cap, int mw, Alloc&& alloc) {
  if (cap <= h.cap && mw <= h.mw) return TJ_OK;
  const int gc = std::max(cap, h.cap), gm = std::max(mw, h.mw);
  const int r = query_grow(h.allocs, [&] { h.sized = {}; h.out = nullptr; h.cap = -1; h.mw = 0; }, [&] { const int e = alloc(h.sized, gc, gm, &h.allocs); return e ? e : query_buf(c, h.out, gc, &h.allocs); });
  if (!r) { h.cap = gc; h.mw = gm; }
  return r;
}
// the pair index of a call (kernels_pair_approach.h): the bitmask, its offsets and n are the fleet's size (allocated once) and cleared; ix gets their fields and the call's slots
template <class Held>
int pair_index_begin(tj_ctx* c, Held& h, int cap, PairIndex& ix) {
  const Dev& d = c->d;
  const int owned = d.u1 - d.u0, words = (d.U + 31) / 32;
  const size_t mask_n = (size_t)(owned > 0 ? owned : 1) * words;
  int r;
  if ((r = query_buf(c, h.mask, mask_n)) || (r = query_buf(c, h.wordoff, mask_n)) || (r = query_buf(c, h.n, 1))) return r;
  ix.cap = cap; ix.words = words; ix.mask = h.mask; ix.wordoff = h.wordoff; ix.n = h.n;
  return (r = query_clear(c, h.mask, mask_n)) ? r : query_clear(c, h.n, 1);
}
// behind a query's marking launch: pair p is the p-th set bit
void pair_index_launch(tj_ctx* c, const PairIndex& ix) { hipLaunchKernelGGL(k_pair_index, dim3(1), dim3(PA_INDEX), 0, c->stream, c->d, ix); }
// the end of a row-listing call whose total is known: min(cap, total) rows to the caller, then the capacity error in the call's words (what: "pairs are listed, the
// caller's rows hold" or "rows, the caller's hold").  silent: a count-only call, to which more rows than room are no error
template <class Rec>
int rows_finish(tj_ctx* c, const std::string& name, Rec* rows, const Rec* dev, int cap, int total, const char* what, bool silent) {
  int r;
  if (std::min(cap, total) > 0 && ((r = query_fetch(c, rows, dev, std::min(cap, total))) || (r = query_finish(c, nullptr)))) return r;
  if (total > cap && !silent) { c->err = name + ": " + std::to_string(total) + " " + what + " " + std::to_string(cap) + ": the first " + std::to_string(cap) + " were written"; return TJ_ERR_CAPACITY; }
  return TJ_OK;
}

// the first line of every row-listing call: a context, somewhere to put the count, and rows where there is room for any
template <class Rec>
bool rows_args_ok(const tj_ctx* c, const int* n, const Rec* rows, int cap) { return c && n && cap >= 0 && !(cap > 0 && !rows); }
// a RowsHeld before its call's launches: the device's row count, and the rows grown to the largest cap so far.  (Clearing the count stays with the caller, right before its launches.)
template <class Row>
int rows_begin(tj_ctx* c, RowsHeld<Row>& h, int cap) {
  int r = query_buf(c, h.n_rows, 1);
  if (!r && cap > h.cap) {
    if ((r = query_grow(h.out_allocs, [&] { h.out = nullptr; h.cap = 0; }, [&] { return query_buf(c, h.out, cap, &h.out_allocs); }))) return r;
    h.cap = cap;
  }
  return r;
}
// a RowsHeld behind its call's launches: the count is fetched and the call waited for, *n = the rows, min(cap, *n) of them go to the caller; more rows than cap are
// TJ_ERR_CAPACITY unless the call only counts (cap == 0 without rows).  walked: the query walked the BVH, and a frontier overflow ends the call here, worded for `dist`
// (query_finish words it for a `range`), *n untouched: no count is known
template <class Row>
int rows_end(tj_ctx* c, const SearchSpec& spec, RowsHeld<Row>& h, Row* rows, int cap, int* n, bool walked) {
  const std::string name = spec.name;
  int r, nr = 0;
  if ((r = query_fetch(c, &nr, h.n_rows, 1)) || (r = query_finish(c, walked ? spec.name : nullptr))) {
    if (walked && r == TJ_ERR_CAPACITY)
      c->err = name + ": the BVH frontier of a window overflowed at this dist (more than " + std::to_string(FRONT_CAP) + " boxes of 8 primitives near one window's box): lower `dist`";
    return r;
  }
  *n = nr;
  return rows_finish(c, name, rows, h.out, cap, nr, "rows, the caller's hold", cap == 0 && !rows);
}

int audit_run(tj_ctx* c, double range, const double* net_host, tj_audit_robot* out, double* seg_obs, double* seg_pair) {
  if (!c || !out) return TJ_ERR_INVALID;
  int r = query_state(c, "tj_audit", false, false);
  if (r) return r;
  const Dev& d = c->d;
  const size_t rows = (size_t)d.U * d.S;
  const int owned = d.u1 - d.u0;
  QUIESCE(c);
  AuditArgs& b = c->audit;
  if ((r = query_buf(c, b.row_obs, rows)) || (r = query_buf(c, b.row_pair, rows)) || (r = query_buf(c, b.row_speed, rows)) || (r = query_buf(c, b.row_accel, rows)) ||
      (r = query_buf(c, b.row_prim, rows)) || (r = query_buf(c, b.row_q, rows)) || (r = query_buf(c, c->audit_out, d.U)) || (r = ensure_order(c))) return r;
  AuditArgs a = b;
  const double* pt;
  Dev da;
  if ((r = query_inputs(c, net_host, nullptr, a.net, pt)) || (r = walk_dev(c, da))) return r;
  a.order = c->q_order; a.range = query_range(d, range);
  if ((r = query_clear(c, c->audit_out, d.U)) || (r = query_clear(c, a.row_obs, rows, seg_obs || seg_pair)) || (r = query_clear(c, a.row_pair, rows, seg_obs || seg_pair))) return r;
  if (owned > 0) {   // plain launches (here and in the other queries): not part of the iteration schedules, not counted by tj_launch_count
    with_prim(d, [&](auto prim) { hipLaunchKernelGGL(k_audit<decltype(prim)::value>, dim3(owned * d.S), dim3(64), 0, c->stream, da, a); });
    hipLaunchKernelGGL(k_audit_reduce, dim3(owned), dim3(64), 0, c->stream, da, a, c->audit_out);
  }
  if ((r = query_fetch(c, out, c->audit_out, d.U)) || (r = query_fetch(c, seg_obs, a.row_obs, rows)) || (r = query_fetch(c, seg_pair, a.row_pair, rows))) return r;
  return query_finish(c, "tj_audit");
}

// the buffers and arguments of k_audit_timed (tj_audit_timed, and the level-0 seed bound of tj_closest_approach); the caller has quiesced the context
int timed_setup(tj_ctx* c, double range, int levels, const double* net_host, const double* pt_host, AuditTimedArgs& a) {
  const Dev& d = c->d;
  const size_t rows = (size_t)d.U * d.S;
  AuditTimedArgs& b = c->timed;
  int r;
  if ((r = query_buf(c, b.row_lo, rows)) || (r = query_buf(c, b.row_hi, rows)) || (r = query_buf(c, b.row_time, rows)) || (r = query_buf(c, b.row_qlo, rows)) ||
      (r = query_buf(c, b.row_qhi, rows)) || (r = query_buf(c, c->timed_out, d.U))) return r;
  a = b;
  a.range = query_range(d, range); a.levels = levels;
  return query_inputs(c, net_host, pt_host, a.net, a.pt);
}
// k_audit_timed and its reduction: the two launches of tj_audit_timed, the first two of tj_closest_approach
void timed_launch(tj_ctx* c, const AuditTimedArgs& a) {
  const Dev& d = c->d;
  hipLaunchKernelGGL(k_audit_timed, dim3((d.u1 - d.u0) * d.S), dim3(64), 0, c->stream, d, a);
  hipLaunchKernelGGL(k_audit_timed_reduce, dim3(d.u1 - d.u0), dim3(64), 0, c->stream, d, a, c->timed_out);
}

int audit_timed_run(tj_ctx* c, double range, int levels, const double* net_host, const double* pt_host, tj_audit_timed_robot* out, double* seg_lo, double* seg_hi) {
  if (!c || !out) return TJ_ERR_INVALID;
  int r = query_nan(c, "tj_audit_timed", "range", range);
  if (r) return r;
  if (levels > 6) { c->err = "tj_audit_timed: levels must be 0..6 (or negative for the default): one segment's sub-windows are one wave wide"; return TJ_ERR_INVALID; }
  if ((r = query_state(c, "tj_audit_timed", true, net_host && pt_host))) return r;
  const Dev& d = c->d;
  const size_t rows = (size_t)d.U * d.S;
  QUIESCE(c);
  AuditTimedArgs a;
  if ((r = timed_setup(c, range, levels < 0 ? TJ_AUDIT_TIMED_LEVELS : levels, net_host, pt_host, a))) return r;
  if ((r = query_clear(c, c->timed_out, d.U)) || (r = query_clear(c, a.row_lo, rows, seg_lo || seg_hi)) || (r = query_clear(c, a.row_hi, rows, seg_lo || seg_hi))) return r;
  if (d.u1 > d.u0) timed_launch(c, a);   // two launches whatever the fleet's size
  if ((r = query_fetch(c, out, c->timed_out, d.U)) || (r = query_fetch(c, seg_lo, a.row_lo, rows)) || (r = query_fetch(c, seg_hi, a.row_hi, rows))) return r;
  return query_finish(c, nullptr);
}

int closest_run(tj_ctx* c, double range, double tol, int max_depth, int max_windows, const double* net_host, const double* pt_host, tj_closest_robot* out) {
  if (!c || !out) return TJ_ERR_INVALID;
  int r;
  SearchArgs sa;
  if ((r = search_args(c, SEARCH_CLOSEST, range, tol, max_depth, max_windows, sa)) || (r = query_state(c, "tj_closest_approach", true, net_host && pt_host))) return r;
  const Dev& d = c->d;
  const int owned = d.u1 - d.u0;
  QUIESCE(c);
  AuditTimedArgs t;
  ClosestArgs& b = c->closest;
  if ((r = timed_setup(c, range, 0, net_host, pt_host, t)) || (r = query_buf(c, b.list, (size_t)d.U * 2 * TJ_CLOSEST_FRONTIER)) || (r = query_buf(c, b.klo, (size_t)d.U * 2 * TJ_CLOSEST_FRONTIER)) ||
      (r = query_buf(c, b.count, (size_t)d.U * 3)) || (r = query_buf(c, c->closest_out, d.U))) return r;
  ClosestArgs a = b;
  a.net = t.net; a.pt = t.pt; sa.put(a);
  a.seed = c->timed_out;
  if ((r = query_clear(c, c->closest_out, d.U)) || (r = query_clear(c, a.count, (size_t)d.U * 3))) return r;
  if (owned > 0) {   // four launches whatever the fleet's size and the depth
    timed_launch(c, t);
    hipLaunchKernelGGL(k_closest_seed, dim3(owned * d.S), dim3(64), 0, c->stream, d, a);
    hipLaunchKernelGGL(k_closest_refine, dim3(owned), dim3(CL_THREADS), 0, c->stream, d, a, c->closest_out);
  }
  if ((r = query_fetch(c, out, c->closest_out, d.U))) return r;
  return query_finish(c, nullptr);
}

// ---- the three row-listing queries: what a query states (its search's table row, its byte budget and formula, its buffers, its launches), and the one path they share ----
struct PairQuery {
  using Args = PairArgs; using Rec = tj_pair_record;
  static constexpr const SearchSpec& spec = SEARCH_PAIR;
  static constexpr const char* budget = "TJ_PAIR_MAX_BYTES";
  static constexpr long long max_bytes = TJ_PAIR_MAX_BYTES;
  static auto& held(tj_ctx* c) { return c->pair; }
  // device bytes that depend on the call (include/trajadmm.h states the formula)
  static size_t bytes(const Dev& d, int cap, int mw) {
    return (size_t)cap * ((size_t)2 * mw * (sizeof(ClosestWin) + sizeof(double)) + (size_t)(2 * d.S + 2) * sizeof(PairSeed) + 4 * sizeof(int) + sizeof(tj_pair_record));
  }
  static int alloc(tj_ctx* c, Args& b, int gc, int gm, std::vector<void*>* l) {
    int r;
    if ((r = query_buf(c, b.ix.who, (size_t)gc * 2, l)) || (r = query_buf(c, b.count, (size_t)gc * 2, l)) || (r = query_buf(c, b.seeds, (size_t)gc * (2 * c->d.S + 2), l)) ||
        (r = query_buf(c, b.list, (size_t)gc * 2 * gm, l)) || (r = query_buf(c, b.klo, (size_t)gc * 2 * gm, l))) return r;
    return TJ_OK;
  }
  static int extra(tj_ctx*, Args&, double) { return TJ_OK; }   // (the query has no argument of its own)
  static int prepare(tj_ctx* c, Args& a) { a.seed_cap = 2 * c->d.S + 2; return query_clear(c, a.count, (size_t)a.ix.cap * 2, a.ix.cap > 0); }
  // two launches for the count, four for the rows, whatever the fleet's size, the number of pairs and the depth
  static void mark(tj_ctx* c, const Args& a, int units) { hipLaunchKernelGGL(k_pair_mark, dim3(units), dim3(64), 0, c->stream, c->d, a); }
  static void rows(tj_ctx* c, const Args& a, int units, Rec* out) {
    hipLaunchKernelGGL(k_pair_seed, dim3(units), dim3(64), 0, c->stream, c->d, a);
    hipLaunchKernelGGL(k_pair_refine, dim3(a.ix.cap), dim3(PA_THREADS), 0, c->stream, c->d, a, out);
  }
};
// tj_path_crossings (kernels_path_crossing.h): the rows (u, q > u) of the owned robots u
struct CrossQuery {
  using Args = CrossArgs; using Rec = tj_crossing_record;
  static constexpr const SearchSpec& spec = SEARCH_CROSSING;
  static constexpr const char* budget = "TJ_CROSSING_MAX_BYTES";
  static constexpr long long max_bytes = TJ_CROSSING_MAX_BYTES;
  static auto& held(tj_ctx* c) { return c->cross; }
  static size_t bytes(const Dev&, int cap, int mw) { return (size_t)cap * ((size_t)2 * mw * sizeof(CrossItem) + (size_t)4 * mw * sizeof(double) + 2 * sizeof(int) + sizeof(tj_crossing_record)); }
  template <class A>   // (MarginQuery's lists are the same)
  static int alloc(tj_ctx* c, A& b, int gc, int gm, std::vector<void*>* l) {
    int r;
    if ((r = query_buf(c, b.ix.who, (size_t)gc * 2, l)) || (r = query_buf(c, b.list, (size_t)gc * 2 * gm, l)) || (r = query_buf(c, b.klo, (size_t)gc * 4 * gm, l))) return r;
    return TJ_OK;
  }
  static int extra(tj_ctx*, Args&, double) { return TJ_OK; }
  static int prepare(tj_ctx*, Args&) { return TJ_OK; }
  // two launches for the count, three for the rows, whatever the fleet's size, the number of pairs and the depth
  static void mark(tj_ctx* c, const Args& a, int units) { hipLaunchKernelGGL(k_cross_mark, dim3(units), dim3(64), 0, c->stream, c->d, a); }
  static void rows(tj_ctx* c, const Args& a, int, Rec* out) { hipLaunchKernelGGL(k_cross_refine, dim3(a.ix.cap), dim3(CX_THREADS), 0, c->stream, c->d, a, out); }
};

// tj_timing_margin (kernels_timing_margin.h): the rows (u, q > u) of the owned robots u; the query's own argument is max_slip
struct MarginQuery {
  using Args = MarginArgs; using Rec = tj_margin_record;
  static constexpr const SearchSpec& spec = SEARCH_MARGIN;
  static constexpr const char* budget = "TJ_MARGIN_MAX_BYTES";
  static constexpr long long max_bytes = TJ_MARGIN_MAX_BYTES;
  static auto& held(tj_ctx* c) { return c->margin; }
  static size_t bytes(const Dev&, int cap, int mw) { return (size_t)cap * ((size_t)2 * mw * sizeof(CrossItem) + (size_t)4 * mw * sizeof(double) + 2 * sizeof(int) + sizeof(tj_margin_record)); }
  static int alloc(tj_ctx* c, Args& b, int gc, int gm, std::vector<void*>* l) { return CrossQuery::alloc(c, b, gc, gm, l); }   // (the same lists)
  static int extra(tj_ctx* c, Args& a, double max_slip) {
    const int r = query_nan(c, spec.name, "max_slip", max_slip);
    a.max_slip = max_slip > 0 ? max_slip : INFINITY;
    return r;
  }
  static int prepare(tj_ctx*, Args&) { return TJ_OK; }
  // two launches for the count, three for the rows, whatever the fleet's size, the number of pairs and the depth
  static void mark(tj_ctx* c, const Args& a, int units) { hipLaunchKernelGGL(k_margin_mark, dim3(units), dim3(64), 0, c->stream, c->d, a); }
  static void rows(tj_ctx* c, const Args& a, int, Rec* out) { hipLaunchKernelGGL(k_margin_refine, dim3(a.ix.cap), dim3(MG_THREADS), 0, c->stream, c->d, a, out); }
};

// mark the listed pairs, index them (k_pair_index: pair p is the p-th set bit), and, for a call with room, search each: n first, then min(cap, n) rows.  extra: the
// query's own argument, if it has one (Q::extra checks and stores it)
template <class Q>
int listed_run(tj_ctx* c, double range, double tol, int max_depth, int max_windows, double extra, const double* net_host, const double* pt_host, typename Q::Rec* rows, int cap, int* n) {
  if (!rows_args_ok(c, n, rows, cap)) return TJ_ERR_INVALID;
  const std::string name = Q::spec.name;
  int r;
  SearchArgs sa;
  typename Q::Args own{};   // checked here, with the other arguments; stored into the call's arguments once those exist (below)
  if ((r = Q::extra(c, own, extra)) || (r = search_args(c, Q::spec, range, tol, max_depth, max_windows, sa))) return r;
  const Dev& d = c->d;
  const int mw = sa.max_windows;
  if ((r = query_budget(c, name + ": cap " + std::to_string(cap) + " rows at max_windows " + std::to_string(mw), Q::bytes(d, cap, mw), Q::budget, Q::max_bytes,
                        "lower cap (rows beyond it are still counted) or max_windows")) ||
      (r = query_state(c, Q::spec.name, true, net_host && pt_host))) return r;
  *n = 0;
  if (!d.multi()) return TJ_OK;   // one UAV: no pair
  const int owned = d.u1 - d.u0;
  QUIESCE(c);
  auto& h = Q::held(c);
  if ((r = listed_grow(c, h, cap, mw, [&](typename Q::Args& b, int gc, int gm, std::vector<void*>* l) { return Q::alloc(c, b, gc, gm, l); }))) return r;
  typename Q::Args a = h.sized;
  if ((r = query_inputs(c, net_host, pt_host, a.net, a.pt))) return r;
  sa.put(a);
  Q::extra(c, a, extra);
  if ((r = pair_index_begin(c, h, cap, a.ix)) || (r = Q::prepare(c, a))) return r;
  if (owned > 0) {
    Q::mark(c, a, owned * d.S);
    pair_index_launch(c, a.ix);
    if (cap > 0) Q::rows(c, a, owned * d.S, h.out);
  }
  if ((r = query_fetch(c, n, h.n, 1)) || (r = query_finish(c, nullptr))) return r;
  return rows_finish(c, name, rows, h.out, cap, *n, "pairs are listed, the caller's rows hold", !rows);
}

// tj_proximity_windows (kernels_proximity.h): the rows of the directed pairs (u, q), u owned.  pair_cap: the slots of listed pairs, row_cap <= pair_cap: the caller's
// rows (the public call gives both its cap; a group gives every rank the whole cap in slots and what is left of it in rows).  n_pairs first, then the row total, then
// min(row_cap, n) rows.  Five launches for the rows, two for the count.
size_t proximity_bytes(const Dev& d, int cap, int mw) {
  const size_t seeds = (size_t)2 * d.S + 2;
  return (size_t)cap * ((size_t)2 * mw * sizeof(ProxWin) + 2 * ((size_t)2 * mw + seeds) * sizeof(ProxLeaf) + seeds * sizeof(ProxSeed) + 8 * sizeof(int) + sizeof(tj_proximity_row));
}
int proximity_run(tj_ctx* c, double dist, double tol, int max_depth, int max_windows, const double* net_host, const double* pt_host, tj_proximity_row* rows, int pair_cap, int row_cap,
                  int* n_pairs, int* n) {
  if (!c || !n || !n_pairs || pair_cap < 0 || row_cap < 0 || row_cap > pair_cap || (row_cap > 0 && !rows)) return TJ_ERR_INVALID;
  const SearchSpec& spec = SEARCH_PROXIMITY;
  const std::string name = spec.name;
  int r;
  SearchArgs sa;
  if ((r = search_args(c, spec, dist, tol, max_depth, max_windows, sa))) return r;
  const Dev& d = c->d;
  const int mw = sa.max_windows, cap = pair_cap;
  if ((r = query_budget(c, name + ": cap " + std::to_string(cap) + " pairs at max_windows " + std::to_string(mw), proximity_bytes(d, cap, mw), "TJ_PROXIMITY_MAX_BYTES", TJ_PROXIMITY_MAX_BYTES,
                        "lower cap or max_windows")) ||
      (r = query_state(c, spec.name, true, net_host && pt_host))) return r;
  *n_pairs = 0; *n = 0;
  if (!d.multi()) return TJ_OK;   // one UAV: no pair
  const int owned = d.u1 - d.u0, seed_cap = 2 * d.S + 2;
  QUIESCE(c);
  ProxHeld& h = c->prox;
  if ((r = query_buf(c, h.n_rows, 1)) ||
      (r = listed_grow(c, h, cap, mw, [&](ProxArgs& b, int gc, int gm, std::vector<void*>* l) {
         const size_t leaves = (size_t)gc * ((size_t)2 * gm + seed_cap);
         int e;   // (the first failure, or TJ_OK)
         (e = query_buf(c, b.ix.who, (size_t)gc * 2, l)) || (e = query_buf(c, b.count, (size_t)gc * 2, l)) || (e = query_buf(c, b.seeds, (size_t)gc * seed_cap, l)) ||
             (e = query_buf(c, b.list, (size_t)gc * 2 * gm, l)) || (e = query_buf(c, b.leaf, leaves, l)) || (e = query_buf(c, b.sorted, leaves, l)) || (e = query_buf(c, b.info, (size_t)gc * 4, l));
         return e;
       }))) return r;
  ProxArgs a = h.sized;
  if ((r = query_inputs(c, net_host, pt_host, a.net, a.pt))) return r;
  sa.put(a);
  a.seed_cap = seed_cap; a.leaf_cap = 2 * mw + seed_cap; a.row_cap = row_cap; a.n_rows = h.n_rows;
  if ((r = pair_index_begin(c, h, cap, a.ix)) || (r = query_clear(c, h.n_rows, 1)) || (r = query_clear(c, a.count, (size_t)cap * 2, cap > 0))) return r;
  if (owned > 0) {
    hipLaunchKernelGGL(k_prox_mark, dim3(owned * d.S), dim3(64), 0, c->stream, d, a);
    pair_index_launch(c, a.ix);
    if (cap > 0) {
      hipLaunchKernelGGL(k_prox_seed, dim3(owned * d.S), dim3(64), 0, c->stream, d, a);
      hipLaunchKernelGGL(k_prox_refine, dim3(cap), dim3(PX_THREADS), 0, c->stream, d, a);
      hipLaunchKernelGGL(k_prox_place, dim3(cap), dim3(PX_THREADS), 0, c->stream, d, a, h.out);
    }
  }
  int np = 0, nr = 0;
  if ((r = query_fetch(c, &np, h.n, 1)) || (r = query_fetch(c, &nr, h.n_rows, 1)) || (r = query_finish(c, nullptr))) return r;
  *n_pairs = np;
  if (np > cap) {   // rows are known only for pairs that were refined
    *n = -1;
    if (cap == 0 && !rows) return TJ_OK;   // the count-only call
    c->err = name + ": " + std::to_string(np) + " pairs are listed, the caller's slots hold " + std::to_string(cap) + ": nothing was written";
    return TJ_ERR_CAPACITY;
  }
  *n = nr;
  return rows_finish(c, name, rows, h.out, row_cap, nr, "rows, the caller's hold", false);
}

// tj_obstacle_windows (kernels_obstacle_windows.h): the rows of the owned robots from the context's own state (nothing of another robot is read, so a sharded context
// answers for its own and a group calls this rank after rank).  *n = the rows; min(cap, *n) of them are written.  TJ_ERR_CAPACITY has two causes: more rows than cap
// (*n is set, and exceeds cap) and a walk frontier overflow (*n is left untouched: no count is known).  Three launches for the rows, two for the count.
size_t obswin_bytes(const Dev& d, int owned, int cap, int mw) {
  return (size_t)owned * d.S * ((size_t)4 * mw * sizeof(ObwinLeaf) + 4 * sizeof(int)) + (size_t)owned * 2 * sizeof(int) + (size_t)cap * sizeof(tj_obswin_row);
}
int obswin_run(tj_ctx* c, double dist, double tol, int max_depth, int max_windows, tj_obswin_row* rows, int cap, int* n) {
  if (!rows_args_ok(c, n, rows, cap)) return TJ_ERR_INVALID;
  const SearchSpec& spec = SEARCH_OBSWIN;
  const std::string name = spec.name;
  int r;
  SearchArgs sa;
  if ((r = search_args(c, spec, dist, tol, max_depth, max_windows, sa))) return r;
  const Dev& d = c->d;
  const int mw = sa.max_windows, owned = d.u1 - d.u0;
  if ((r = query_budget(c, name + ": " + std::to_string(owned) + " robots of " + std::to_string(d.S) + " segments at max_windows " + std::to_string(mw) + " and cap " + std::to_string(cap),
                        obswin_bytes(d, owned, cap, mw), "TJ_OBSWIN_MAX_BYTES", TJ_OBSWIN_MAX_BYTES, "lower max_windows or cap")) ||
      (r = query_state(c, spec.name, false, false))) return r;
  if (d.N == 0 || owned <= 0) { *n = 0; return TJ_OK; }   // no obstacles: nothing is within any distance of them
  QUIESCE(c);
  ObwinHeld& h = c->obwin;
  const size_t units = (size_t)owned * d.S;
  if ((r = rows_begin(c, h, cap)) || (r = query_buf(c, h.sized.info, units * 4)) || (r = query_buf(c, h.sized.robot, (size_t)owned * 2)) || (r = ensure_order(c))) return r;
  if (mw > h.mw) {
    if ((r = query_grow(h.allocs, [&] { h.sized.list = nullptr; h.sized.leaf = nullptr; h.mw = 0; },
                        [&] { const int e = query_buf(c, h.sized.list, units * 2 * mw, &h.allocs); return e ? e : query_buf(c, h.sized.leaf, units * 2 * mw, &h.allocs); }))) return r;
    h.mw = mw;
  }
  ObwinArgs a = h.sized;
  Dev da;
  if ((r = query_inputs(c, nullptr, nullptr, a.net, a.pt)) || (r = walk_dev(c, da))) return r;
  a.order = c->q_order; sa.put(a); a.row_cap = cap; a.n_rows = h.n_rows;
  if ((r = query_clear(c, h.n_rows, 1))) return r;
  with_prim(d, [&](auto prim) { hipLaunchKernelGGL(k_obwin_refine<decltype(prim)::value>, dim3((unsigned)units), dim3(OW_THREADS), 0, c->stream, da, a); });
  hipLaunchKernelGGL(k_obwin_count, dim3(owned), dim3(OW_THREADS), 0, c->stream, da, a);
  if (cap > 0) hipLaunchKernelGGL(k_obwin_place, dim3(owned), dim3(OW_THREADS), 0, c->stream, da, a, h.out);
  return rows_end(c, spec, h, rows, cap, n, true);   // (a walk overflow ends there: *n stays untouched)
}

// tj_sight_windows (kernels_sight_windows.h): the rows of the links (a, b) whose a is owned, `link` = the caller's index; a link of another rank's robot has no row here
// (a group asks every rank for the whole list and places the rows by link).  The other end's net and piece_time are read, so a sharded context needs them handed in.
// *n = the rows; min(cap, *n) of them are written.  TJ_ERR_CAPACITY has two causes, as in obswin_run: more rows than cap (*n is set, and exceeds cap) and a walk frontier
// overflow (*n is left untouched).  Three launches for the rows, two for the count.
size_t sight_bytes(const Dev& d, int n_links, int n_stations, int cap, int mw) {
  return (size_t)n_links * d.S * ((size_t)2 * (2 * mw + d.S + 1) * sizeof(SightLeaf) + 4 * sizeof(int)) + (size_t)n_links * 4 * sizeof(int) + (size_t)n_stations * 3 * sizeof(double) + (size_t)cap * sizeof(tj_sight_row);
}
int sight_run(tj_ctx* c, const int* links, int n_links, const double* stations, int n_stations, double dist, double tol, int max_depth, int max_windows,
              const double* net_host, const double* pt_host, tj_sight_row* rows, int cap, int* n) {
  if (!rows_args_ok(c, n, rows, cap) || n_links < 0 || (n_links > 0 && !links) || n_stations < 0 || (n_stations > 0 && !stations)) return TJ_ERR_INVALID;
  const SearchSpec& spec = SEARCH_SIGHT;
  const std::string name = spec.name;
  int r;
  for (int k = 0; k < 3 * n_stations; k++) if ((r = query_nan(c, spec.name, "a station coordinate", stations[k]))) return r;
  SearchArgs sa;
  if ((r = search_args(c, spec, dist, tol, max_depth, max_windows, sa))) return r;
  const Dev& d = c->d;
  for (int k = 0; k < n_links; k++) {
    const int a = links[2 * k], b = links[2 * k + 1];
    if (a < 0 || a >= d.U || b == a || b >= d.U || b < -n_stations) {
      c->err = name + ": link " + std::to_string(k) + " = (" + std::to_string(a) + ", " + std::to_string(b) + "): a must be a robot, b another robot or -1 - s for one of the " + std::to_string(n_stations) + " stations";
      return TJ_ERR_INVALID;
    }
  }
  const int mw = sa.max_windows, leaf_cap = 2 * mw + d.S + 1;
  if ((r = query_budget(c, name + ": " + std::to_string(n_links) + " links of " + std::to_string(d.S) + " segments at max_windows " + std::to_string(mw) + " and cap " + std::to_string(cap),
                        sight_bytes(d, n_links, n_stations, cap, mw), "TJ_SIGHT_MAX_BYTES", TJ_SIGHT_MAX_BYTES, "lower max_windows, cap or the number of links")) ||
      (r = query_state(c, spec.name, true, net_host && pt_host))) return r;
  if (d.N == 0 || n_links == 0) { *n = 0; return TJ_OK; }   // no obstacles: no link is within any distance of them
  QUIESCE(c);
  SightHeld& h = c->sight;
  const size_t units = (size_t)n_links * d.S, items = units * leaf_cap;
  if ((r = rows_begin(c, h, cap)) || (r = ensure_order(c))) return r;
  if (items > h.items || units > h.units || n_links > h.n_links || n_stations > h.n_stations) {
    const size_t gi = std::max(items, h.items), gu = std::max(units, h.units);
    const int gl = std::max(n_links, h.n_links), gs = std::max(n_stations, h.n_stations);
    if ((r = query_grow(h.allocs, [&] { h.sized = {}; h.links = nullptr; h.stations = nullptr; h.items = 0; h.units = 0; h.n_links = 0; h.n_stations = 0; }, [&] {
           int e;   // (the first failure, or TJ_OK)
           (e = query_buf(c, h.sized.list, gi, &h.allocs)) || (e = query_buf(c, h.sized.leaf, gi, &h.allocs)) || (e = query_buf(c, h.sized.info, gu * 4, &h.allocs)) ||
               (e = query_buf(c, h.sized.link, (size_t)gl * 2, &h.allocs)) || (e = query_buf(c, h.links, (size_t)gl * 2, &h.allocs)) || (e = query_buf(c, h.stations, (size_t)gs * 3, &h.allocs));
           return e;
         }))) return r;
    h.items = gi; h.units = gu; h.n_links = gl; h.n_stations = gs;
  }
  SightArgs a = h.sized;
  Dev da;
  if ((r = query_inputs(c, net_host, pt_host, a.net, a.pt)) || (r = walk_dev(c, da)) || (r = upload(c, h.links, links, (size_t)n_links * 2 * sizeof(int))) ||
      (r = upload(c, h.stations, stations, (size_t)n_stations * 3 * sizeof(double)))) return r;
  a.order = c->q_order; a.links = h.links; a.stations = h.stations; sa.put(a); a.leaf_cap = leaf_cap; a.row_cap = cap; a.n_rows = h.n_rows;
  if ((r = query_clear(c, h.n_rows, 1))) return r;
  with_prim(d, [&](auto prim) { hipLaunchKernelGGL(k_sight_refine<decltype(prim)::value>, dim3((unsigned)units), dim3(SW_THREADS), 0, c->stream, da, a); });
  hipLaunchKernelGGL(k_sight_count, dim3(n_links), dim3(SW_THREADS), 0, c->stream, da, a);
  if (cap > 0) hipLaunchKernelGGL(k_sight_place, dim3(n_links), dim3(SW_THREADS), 0, c->stream, da, a, h.out);
  return rows_end(c, spec, h, rows, cap, n, true);   // (a walk overflow ends there: *n stays untouched)
}

// ---- the slot queries tj_dynamics_windows and tj_zone_windows (dev_query.h: WinSlotArgs, win_lane_search, win_slot_place): the rows of the owned robots from the
// context's own state, slot after slot = (robot, the call's k-th gate or zone); nothing of another robot is read, so a sharded context answers for its own and a group
// calls it rank after rank.  *n = the rows; min(cap, *n) of them are written.  Two launches for the rows, one for the count. ----
template <class Leaf, class Row>
size_t slot_bytes(const Dev& d, size_t slots, int cap, int mw) {
  return slots * (((size_t)3 * d.S + (size_t)4 * mw) * sizeof(Leaf) + 4 * sizeof(int)) + (size_t)cap * sizeof(Row);
}
// What a slot query's *_run hands on once its own arguments are checked, defaulted and packed.  sa: tol, max_depth, max_windows; per_robot of `noun` ("gates",
// "zones"): the slots of a robot; budget, max_bytes, advice: query_budget's.  own(a) -> rc: the call's uploads and the members `a` has beyond WinSlotArgs.
template <class Args, class Row, class Own>
int slot_run(tj_ctx* c, const SearchSpec& spec, const SearchArgs& sa, SlotHeld<Args, Row>& h, int per_robot, const char* noun, const char* budget, long long max_bytes, const char* advice,
             Own&& own, void (*refine)(Dev, Args), void (*place)(Dev, Args, Row*), Row* rows, int cap, int* n) {
  const std::string name = spec.name;
  const Dev& d = c->d;
  const int mw = sa.max_windows, owned = d.u1 - d.u0;
  const size_t slots = (size_t)std::max(owned, 0) * per_robot;
  int r;
  if ((r = query_budget(c, name + ": " + std::to_string(owned) + " robots x " + std::to_string(per_robot) + " " + noun + " of " + std::to_string(d.S) + " segments at max_windows " + std::to_string(mw) + " and cap " + std::to_string(cap),
                        slot_bytes<typename Args::Leaf, Row>(d, slots, cap, mw), budget, max_bytes, advice)) ||
      (r = query_state(c, spec.name, false, false))) return r;
  if (slots == 0) { *n = 0; return TJ_OK; }
  QUIESCE(c);
  const size_t live = slots * 2 * ((size_t)d.S + mw), leaf = slots * ((size_t)d.S + 2 * (size_t)mw);
  if ((r = rows_begin(c, h, cap))) return r;
  if (slots > h.slots || live > h.live || leaf > h.leaf) {
    const size_t gs = std::max(slots, h.slots), gv = std::max(live, h.live), gf = std::max(leaf, h.leaf);
    if ((r = query_grow(h.allocs, [&] { h.sized = {}; h.slots = 0; h.live = 0; h.leaf = 0; }, [&] {
           int e;   // (the first failure, or TJ_OK)
           (e = query_buf(c, h.sized.list, gv, &h.allocs)) || (e = query_buf(c, h.sized.leaf, gf, &h.allocs)) || (e = query_buf(c, h.sized.info, gs * 4, &h.allocs));
           return e;
         }))) return r;
    h.slots = gs; h.live = gv; h.leaf = gf;
  }
  Args a = h.sized;
  if ((r = query_inputs(c, nullptr, nullptr, a.net, a.pt)) || (r = own(a))) return r;
  a.tol = sa.tol; a.max_depth = sa.max_depth; a.max_windows = mw; a.row_cap = cap; a.n_rows = h.n_rows;
  if ((r = query_clear(c, h.n_rows, 1))) return r;
  hipLaunchKernelGGL(refine, dim3((unsigned)slots), dim3(WIN_LANES), 0, c->stream, d, a);
  if (cap > 0) hipLaunchKernelGGL(place, dim3((unsigned)slots), dim3(WIN_LANES), 0, c->stream, d, a, h.out);
  return rows_end(c, spec, h, rows, cap, n, false);
}

// tj_dynamics_windows (kernels_dynamics_windows.h): slot_run over (robot, gate).  gates == null with n_gates == 0: the two default gates.
int dynwin_run(tj_ctx* c, const tj_dyn_gate* gates, int n_gates, double tol, int max_depth, int max_windows, tj_dynwin_row* rows, int cap, int* n) {
  if (!rows_args_ok(c, n, rows, cap) || n_gates < 0 || (n_gates > 0 && !gates)) return TJ_ERR_INVALID;
  const SearchSpec& spec = SEARCH_DYNWIN;
  const std::string name = spec.name;
  const Dev& d = c->d;
  int r;
  if ((r = query_nan(c, spec.name, "tol", tol))) return r;
  for (int k = 0; k < n_gates; k++) if ((r = query_nan(c, spec.name, "a gate's level", gates[k].level))) return r;
  if (n_gates > TJ_DYNWIN_MAX_GATES) { c->err = name + ": n_gates must be 0.." + std::to_string(TJ_DYNWIN_MAX_GATES); return TJ_ERR_INVALID; }
  for (int k = 0; k < n_gates; k++)
    if (gates[k].quantity < TJ_DYNWIN_SPEED || gates[k].quantity > TJ_DYNWIN_JERK || gates[k].sense < TJ_DYNWIN_ABOVE || gates[k].sense > TJ_DYNWIN_BELOW) {
      c->err = name + ": gate " + std::to_string(k) + ": quantity must be TJ_DYNWIN_SPEED, ACCEL or JERK and sense TJ_DYNWIN_ABOVE or BELOW";
      return TJ_ERR_INVALID;
    }
  SearchArgs sa;
  if ((r = search_args(c, spec, 0.0, tol, max_depth, max_windows, sa))) return r;
  // the default tolerance, a design condition: the time in which a vehicle at the acceleration limit changes its speed by 1 % of the speed limit
  if (tol < 0) sa.tol = (TJ_DYNWIN_TOL_FRACTION * d.vel_limit) / d.acc_limit;
  std::vector<tj_dyn_gate> gl(gates, gates + n_gates);
  if (!gates) gl = {tj_dyn_gate{d.vel_limit, TJ_DYNWIN_SPEED, TJ_DYNWIN_ABOVE}, tj_dyn_gate{d.acc_limit, TJ_DYNWIN_ACCEL, TJ_DYNWIN_ABOVE}};
  const int ng = (int)gl.size();
  return slot_run(c, spec, sa, c->dynwin, ng, "gates", "TJ_DYNWIN_MAX_BYTES", TJ_DYNWIN_MAX_BYTES, "lower max_windows, cap or the number of gates", [&](DynwinArgs& a) {
    int e;   // (the first failure, or TJ_OK)
    (e = query_buf(c, c->dynwin_gates, TJ_DYNWIN_MAX_GATES)) || (e = upload(c, c->dynwin_gates, gl.data(), (size_t)ng * sizeof(tj_dyn_gate)));
    a.gates = c->dynwin_gates; a.n_gates = ng;
    return e;
  }, k_dynwin_refine, k_dynwin_place, rows, cap, n);
}

// tj_zone_windows (kernels_zone_windows.h): slot_run over (robot, zone).  The zone list and the shape rows the zones name are copied per call.
int zonewin_run(tj_ctx* c, const tj_zone* zones, int n_zones, const double* shapes, int n_shapes, double tol, int max_depth, int max_windows, tj_zonewin_row* rows, int cap, int* n) {
  if (!rows_args_ok(c, n, rows, cap) || n_zones < 0 || n_shapes < 0 || (n_zones > 0 && !zones) || (n_shapes > 0 && !shapes)) return TJ_ERR_INVALID;
  const SearchSpec& spec = SEARCH_ZONEWIN;
  const std::string name = spec.name;
  const Dev& d = c->d;
  int r;
  if ((r = query_nan(c, spec.name, "tol", tol))) return r;
  for (int k = 0; k < n_zones; k++) if (!std::isfinite(zones[k].level)) { c->err = name + ": zone " + std::to_string(k) + ": the level is NaN or infinite"; return TJ_ERR_INVALID; }
  for (size_t e = 0; e < (size_t)4 * n_shapes; e++) if (!std::isfinite(shapes[e])) { c->err = name + ": row " + std::to_string(e / 4) + " of the shape table holds a NaN or an infinite value"; return TJ_ERR_INVALID; }
  if (n_zones > TJ_ZONEWIN_MAX_ZONES) { c->err = name + ": n_zones must be 0.." + std::to_string(TJ_ZONEWIN_MAX_ZONES); return TJ_ERR_INVALID; }
  std::vector<tj_zone> zl(zones, zones + n_zones);      // the zones with `first` pointing into the packed rows
  std::vector<double> packed;                           // the rows the zones name, zone after zone: at most 64 x 32
  for (int k = 0; k < n_zones; k++) {
    const tj_zone& z = zones[k];
    const std::string zk = name + ": zone " + std::to_string(k) + ": ";
    if (z.kind < TJ_ZONE_PLANES || z.kind > TJ_ZONE_BALL || z.sense < TJ_ZONE_INSIDE || z.sense > TJ_ZONE_OUTSIDE) { c->err = zk + "kind must be TJ_ZONE_PLANES or BALL and sense TJ_ZONE_INSIDE or OUTSIDE"; return TJ_ERR_INVALID; }
    if (z.count < 1 || z.count > (z.kind == TJ_ZONE_BALL ? 1 : TJ_ZONEWIN_MAX_PLANES)) { c->err = zk + "count must be 1.." + std::to_string(TJ_ZONEWIN_MAX_PLANES) + " for planes and 1 for a ball"; return TJ_ERR_INVALID; }
    if (z.first < 0 || z.first > n_shapes - z.count) { c->err = zk + "rows first .. first + count - 1 must lie inside the shape table of " + std::to_string(n_shapes) + " rows"; return TJ_ERR_INVALID; }
    for (int j = 0; j < z.count; j++) {
      const double* row = shapes + (size_t)4 * (z.first + j);
      if (z.kind == TJ_ZONE_PLANES && row[0] == 0.0 && row[1] == 0.0 && row[2] == 0.0) { c->err = zk + "face " + std::to_string(j) + " has an all-zero normal"; return TJ_ERR_INVALID; }
      if (z.kind == TJ_ZONE_BALL && row[3] < 0.0) { c->err = zk + "the radius r must be >= 0"; return TJ_ERR_INVALID; }
    }
    zl[k].first = (int)(packed.size() / 4);
    packed.insert(packed.end(), shapes + (size_t)4 * z.first, shapes + (size_t)4 * (z.first + z.count));
  }
  SearchArgs sa;
  if ((r = search_args(c, spec, 0.0, tol, max_depth, max_windows, sa))) return r;   // (the default tolerance: TJ_ZONEWIN_TOL_FRACTION of offset over vel_limit, a design condition)
  return slot_run(c, spec, sa, c->zonewin, n_zones, "zones", "TJ_ZONEWIN_MAX_BYTES", TJ_ZONEWIN_MAX_BYTES, "lower max_windows, cap or the number of zones", [&](ZonewinArgs& a) {
    int e;   // (the first failure, or TJ_OK)
    (e = query_buf(c, c->zonewin_zones, TJ_ZONEWIN_MAX_ZONES)) || (e = query_buf(c, c->zonewin_shapes, (size_t)4 * TJ_ZONEWIN_MAX_ZONES * TJ_ZONEWIN_MAX_PLANES)) ||
        (e = upload(c, c->zonewin_zones, zl.data(), (size_t)n_zones * sizeof(tj_zone))) || (e = upload(c, c->zonewin_shapes, packed.data(), packed.size() * sizeof(double)));
    a.zones = c->zonewin_zones; a.shapes = c->zonewin_shapes; a.n_zones = n_zones;
    return e;
  }, k_zonewin_refine, k_zonewin_place, rows, cap, n);
}

// tj_flight_profile (kernels_flight_profile.h): the records [U][n_times] of the owned robots; positions of ALL robots from the nets and piece times handed in
int profile_run(tj_ctx* c, const double* times, int n_times, const double* net_host, const double* pt_host, tj_profile_sample* out) {
  if (!c || !times || !out || n_times < 1) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  if (n_times > TJ_PROFILE_MAX_SAMPLES || (long long)d.U * n_times > (long long)TJ_PROFILE_MAX_RECORDS) {
    c->err = "tj_flight_profile: n_times must be 1.." + std::to_string(TJ_PROFILE_MAX_SAMPLES) + " and uav_num * n_times at most " + std::to_string(TJ_PROFILE_MAX_RECORDS);
    return TJ_ERR_INVALID;
  }
  for (int k = 0; k < n_times; k++)
    if (!(times[k] >= 0.0) || times[k] == INFINITY) { c->err = "tj_flight_profile: times[" + std::to_string(k) + "] is NaN, negative or infinite"; return TJ_ERR_INVALID; }
  int r;
  if ((r = query_state(c, "tj_flight_profile", true, net_host && pt_host))) return r;
  const int owned = d.u1 - d.u0, K = n_times;
  const size_t recs = (size_t)d.U * K;
  QUIESCE(c);
  ProfileArgs& b = c->profile;
  if (K > c->profile_cap) {
    std::vector<void*>* l = &c->profile_allocs;
    if ((r = query_grow(*l, [&] { b.times = nullptr; b.pos = nullptr; c->profile_out = nullptr; c->profile_cap = 0; }, [&] {
           int e;   // (the first failure, or TJ_OK)
           (e = query_buf(c, b.times, (size_t)K, l)) || (e = query_buf(c, b.pos, recs * 3, l)) || (e = query_buf(c, c->profile_out, recs, l));
           return e;
         }))) return r;
    c->profile_cap = K;
  }
  if ((r = ensure_order(c))) return r;
  ProfileArgs a = b;
  if ((r = query_inputs(c, net_host, pt_host, a.net, a.pt)) || (r = upload(c, a.times, times, (size_t)K * 8))) return r;
  a.order = c->q_order; a.K = K;
  a.cap = d.N > 0 ? 64 + 8 * (d.nlevels - 1) : 1;   // the walk's stack per sample: the top level and eight per level below it (kernels_flight_profile.h)
  if ((r = query_clear(c, c->profile_out, recs))) return r;
  // two launches whatever the fleet's size, the number of samples and the number of primitives
  hipLaunchKernelGGL(k_profile_points, dim3((unsigned)((recs + FP_THREADS - 1) / FP_THREADS)), dim3(FP_THREADS), 0, c->stream, d, a, c->profile_out);
  if (owned > 0)
    with_prim(d, [&](auto prim) {
      hipLaunchKernelGGL(k_profile_nearest<decltype(prim)::value>, dim3((unsigned)(((size_t)owned * K + 7) / 8)), dim3(64), (size_t)8 * a.cap * sizeof(unsigned long long), c->stream, d, a, c->profile_out);
    });
  if ((r = query_fetch(c, out, c->profile_out, recs))) return r;
  return query_finish(c, nullptr);
}
}  // namespace

extern "C" {

int tj_audit(tj_ctx* c, double range, tj_audit_robot* out, double* seg_obs, double* seg_pair) { return audit_run(c, range, nullptr, out, seg_obs, seg_pair); }
int tj_audit_record_size(void) { return (int)sizeof(tj_audit_robot); }
int tj_audit_timed(tj_ctx* c, double range, int levels, tj_audit_timed_robot* records, double* seg_lo, double* seg_hi) { return audit_timed_run(c, range, levels, nullptr, nullptr, records, seg_lo, seg_hi); }
int tj_audit_timed_record_size(void) { return (int)sizeof(tj_audit_timed_robot); }
int tj_closest_approach(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_closest_robot* records) { return closest_run(c, range, tol, max_depth, max_windows, nullptr, nullptr, records); }
int tj_closest_record_size(void) { return (int)sizeof(tj_closest_robot); }
int tj_pair_approach(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_pair_record* rows, int cap, int* n) { return listed_run<PairQuery>(c, range, tol, max_depth, max_windows, 0.0, nullptr, nullptr, rows, cap, n); }
int tj_pair_record_size(void) { return (int)sizeof(tj_pair_record); }
int tj_path_crossings(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_crossing_record* rows, int cap, int* n) { return listed_run<CrossQuery>(c, range, tol, max_depth, max_windows, 0.0, nullptr, nullptr, rows, cap, n); }
int tj_crossing_record_size(void) { return (int)sizeof(tj_crossing_record); }
int tj_timing_margin(tj_ctx* c, double dist, double max_slip, double tol, int max_depth, int max_windows, tj_margin_record* rows, int cap, int* n) { return listed_run<MarginQuery>(c, dist, tol, max_depth, max_windows, max_slip, nullptr, nullptr, rows, cap, n); }
int tj_margin_record_size(void) { return (int)sizeof(tj_margin_record); }
int tj_proximity_windows(tj_ctx* c, double dist, double tol, int max_depth, int max_windows, tj_proximity_row* rows, int cap, int* n_pairs, int* n) { return proximity_run(c, dist, tol, max_depth, max_windows, nullptr, nullptr, rows, cap, cap, n_pairs, n); }
int tj_proximity_row_size(void) { return (int)sizeof(tj_proximity_row); }

// tj_obstacle_approach: every owned robot from the context's own state (a sharded context's own robots are current; nothing of another robot is read)
int tj_obstacle_approach(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_obstacle_robot* out) {
  if (!c || !out) return TJ_ERR_INVALID;
  int r;
  SearchArgs sa;
  if ((r = search_args(c, SEARCH_OBSTACLE, range, tol, max_depth, max_windows, sa)) || (r = query_state(c, "tj_obstacle_approach", false, false))) return r;
  const Dev& d = c->d;
  const int owned = d.u1 - d.u0;
  const size_t rows = (size_t)d.U * d.S, items = (size_t)(owned > 0 ? owned : 1) * 2 * TJ_OBSTACLE_FRONTIER;
  QUIESCE(c);
  ObstArgs& b = c->obst;
  if ((r = query_buf(c, b.row, rows)) || (r = query_buf(c, b.row_lo, rows)) || (r = query_buf(c, b.best, d.U)) || (r = query_buf(c, b.list, items)) || (r = query_buf(c, b.klo, items)) ||
      (r = query_buf(c, b.count, (size_t)d.U * 2)) || (r = query_buf(c, c->obst_out, d.U)) || (r = ensure_order(c))) return r;
  ObstArgs a = b;
  Dev da;
  if ((r = query_inputs(c, nullptr, nullptr, a.net, a.pt)) || (r = walk_dev(c, da))) return r;
  a.order = c->q_order; sa.put(a); a.cap = TJ_OBSTACLE_FRONTIER;
  if ((r = query_clear(c, c->obst_out, d.U)) || (r = query_clear(c, a.count, (size_t)d.U * 2))) return r;
  if (owned > 0)   // three launches whatever the fleet's size, the number of primitives and the depth
    with_prim(d, [&](auto prim) {
      constexpr int PRIM = decltype(prim)::value;
      hipLaunchKernelGGL(k_obst_seed<PRIM>, dim3(owned * d.S), dim3(64), 0, c->stream, da, a);
      hipLaunchKernelGGL(k_obst_append<PRIM>, dim3(owned * d.S), dim3(64), 0, c->stream, da, a);
      hipLaunchKernelGGL(k_obst_refine<PRIM>, dim3(owned), dim3(OA_THREADS), 0, c->stream, da, a, c->obst_out);
    });
  if ((r = query_fetch(c, out, c->obst_out, d.U))) return r;
  return query_finish(c, "tj_obstacle_approach");
}
int tj_obstacle_record_size(void) { return (int)sizeof(tj_obstacle_robot); }
int tj_obstacle_windows(tj_ctx* c, double dist, double tol, int max_depth, int max_windows, tj_obswin_row* rows, int cap, int* n) { return obswin_run(c, dist, tol, max_depth, max_windows, rows, cap, n); }
int tj_obswin_row_size(void) { return (int)sizeof(tj_obswin_row); }
int tj_sight_windows(tj_ctx* c, const int* links, int n_links, const double* stations, int n_stations, double dist, double tol, int max_depth, int max_windows, tj_sight_row* rows, int cap, int* n) {
  return sight_run(c, links, n_links, stations, n_stations, dist, tol, max_depth, max_windows, nullptr, nullptr, rows, cap, n);
}
int tj_sight_row_size(void) { return (int)sizeof(tj_sight_row); }

// tj_peak_dynamics: every owned robot from the context's own state, like tj_obstacle_approach.  Argument checks in the queries' precedence: null -> NaN -> limits -> no state
int tj_peak_dynamics(tj_ctx* c, double tol, int max_depth, int max_windows, int length_levels, tj_dynamics_robot* out) {
  if (!c || !out) return TJ_ERR_INVALID;
  int r;
  if ((r = query_nan(c, "tj_peak_dynamics", "tol", tol))) return r;
  if (max_depth > TJ_PEAK_MAX_DEPTH) { c->err = "tj_peak_dynamics: max_depth must be 0.." + std::to_string(TJ_PEAK_MAX_DEPTH) + " (or negative for the default): deeper windows are not dyadic in a double"; return TJ_ERR_INVALID; }
  if (max_windows > TJ_PEAK_FRONTIER) { c->err = "tj_peak_dynamics: max_windows must be 1.." + std::to_string(TJ_PEAK_FRONTIER) + " (or <= 0 for the default): the live list's capacity"; return TJ_ERR_INVALID; }
  if (length_levels > TJ_PEAK_MAX_LENGTH_LEVELS) { c->err = "tj_peak_dynamics: length_levels must be 0.." + std::to_string(TJ_PEAK_MAX_LENGTH_LEVELS) + " (or negative for the default)"; return TJ_ERR_INVALID; }
  if ((r = query_state(c, "tj_peak_dynamics", false, false))) return r;
  const Dev& d = c->d;
  const int owned = d.u1 - d.u0, kw = std::max(2 * TJ_PEAK_FRONTIER, d.S);
  const size_t lists = (size_t)(owned > 0 ? owned : 1) * 3;
  QUIESCE(c);
  PeakArgs& b = c->peak;
  if ((r = query_buf(c, b.list, lists * 2 * TJ_PEAK_FRONTIER)) || (r = query_buf(c, b.kub, lists * kw)) || (r = query_buf(c, c->peak_out, d.U))) return r;
  PeakArgs a = b;
  if ((r = query_inputs(c, nullptr, nullptr, a.net, a.pt))) return r;
  a.tol = tol < 0 ? TJ_PEAK_TOL : tol; a.max_depth = max_depth < 0 ? TJ_PEAK_MAX_DEPTH : max_depth; a.max_windows = max_windows <= 0 ? TJ_PEAK_FRONTIER : max_windows;
  a.levels = length_levels < 0 ? TJ_PEAK_LENGTH_LEVELS : length_levels; a.cap = TJ_PEAK_FRONTIER; a.kw = kw;
  if ((r = query_clear(c, c->peak_out, d.U))) return r;
  if (owned > 0) {   // two launches whatever the fleet's size, the piece count and the depth
    hipLaunchKernelGGL(k_peak_dynamics, dim3(owned, 4), dim3(64), 0, c->stream, d, a, c->peak_out);
    hipLaunchKernelGGL(k_peak_finish, dim3((owned + 63) / 64), dim3(64), 0, c->stream, d, c->peak_out);
  }
  if ((r = query_fetch(c, out, c->peak_out, d.U))) return r;
  return query_finish(c, nullptr);
}
int tj_dynamics_record_size(void) { return (int)sizeof(tj_dynamics_robot); }
int tj_dynamics_windows(tj_ctx* c, const tj_dyn_gate* gates, int n_gates, double tol, int max_depth, int max_windows, tj_dynwin_row* rows, int cap, int* n) { return dynwin_run(c, gates, n_gates, tol, max_depth, max_windows, rows, cap, n); }
int tj_dynwin_row_size(void) { return (int)sizeof(tj_dynwin_row); }
int tj_zone_windows(tj_ctx* c, const tj_zone* zones, int n_zones, const double* shapes, int n_shapes, double tol, int max_depth, int max_windows, tj_zonewin_row* rows, int cap, int* n) { return zonewin_run(c, zones, n_zones, shapes, n_shapes, tol, max_depth, max_windows, rows, cap, n); }
int tj_zonewin_row_size(void) { return (int)sizeof(tj_zonewin_row); }
int tj_flight_profile(tj_ctx* c, const double* times, int n_times, tj_profile_sample* out) { return profile_run(c, times, n_times, nullptr, nullptr, out); }
int tj_flight_profile_record_size(void) { return (int)sizeof(tj_profile_sample); }

int tj_get_steps(tj_ctx* c, double* step_self, double* step_obs, double* step_armijo) {
  if (!c) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  QUIESCE(c);
  std::vector<int> ko(array_count(c, d.k_obs)), ks(array_count(c, d.k_self));
  int r;
  if ((r = fetch(c, ko.data(), d.k_obs, 0, ko.size())) || (r = fetch(c, ks.data(), d.k_self, 0, ks.size()))) return r;
  auto p = [](int k) { double s = 1.0; for (int i = 0; i < k; i++) s *= 0.8; return s; };
  for (int u = 0; u < d.U; u++) { if (step_self) step_self[u] = p(ks[u]); if (step_obs) step_obs[u] = p(ko[u]); }
  if (step_armijo && (r = fetch(c, step_armijo, d.step_out, 0, array_count(c, d.step_out)))) return r;
  return TJ_OK;
}

// ---- "optimal_plane":1 : host access to the persistent plane tables (teacher-forced parity tests, checkpointing) ----
int tj_get_obs_cache(tj_ctx* c, int u, int seg, int cap, int* ids, double* cd) {
  if (!c || u < 0 || u >= c->d.U || seg < 0 || seg >= c->d.S || cap < 0) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  if (!d.optimal_plane || d.mode != 0) { c->err = "tj_get_obs_cache: needs optimal_plane and TJ_MODE_SINGLE"; return TJ_ERR_INVALID; }
  QUIESCE(c);
  const size_t s = (size_t)u * d.S + seg;
  int n = 0, r;
  if ((r = fetch_ids(c, d.kobs_n, d.kobs_id, s, cap, ids, n))) return r;
  if (std::min(n, cap) > 0 && cd && (r = fetch(c, cd, d.kobs_cd, s * d.cap_obs * 4, (size_t)std::min(n, cap) * 4))) return r;
  return n;
}
int tj_set_obs_cache(tj_ctx* c, int u, int seg, int n, const int* ids, const double* cd) {
  if (!c || u < 0 || u >= c->d.U || seg < 0 || seg >= c->d.S || n < 0 || (n > 0 && (!ids || !cd))) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  if (!d.optimal_plane || d.mode != 0) { c->err = "tj_set_obs_cache: needs optimal_plane and TJ_MODE_SINGLE"; return TJ_ERR_INVALID; }
  if (n > d.cap_obs) { c->err = "tj_set_obs_cache: more planes than cap_obs"; return TJ_ERR_CAPACITY; }
  QUIESCE(c);
  std::vector<int> tmp(std::max(n, 1));
  if (!ids_to_sorted(c, ids, n, tmp.data())) { c->err = "tj_set_obs_cache: obstacle id out of range"; return TJ_ERR_INVALID; }
  const size_t s = (size_t)u * d.S + seg;
  int r;
  if ((r = store(c, d.kobs_id, s * d.cap_obs, tmp.data(), n)) || (r = store(c, d.kobs_cd, s * d.cap_obs * 4, cd, (size_t)n * 4)) || (r = store(c, d.kobs_n, s, &n, 1))) return r;
  return TJ_OK;
}
int tj_get_pair_cache(tj_ctx* c, int* flags, double* cd) {
  if (!c || !flags || !cd) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  if (!d.optimal_plane || d.mode == 0) { c->err = "tj_get_pair_cache: needs optimal_plane and a multi-UAV mode"; return TJ_ERR_INVALID; }
  QUIESCE(c);
  const size_t n = array_count(c, d.kpair_on);   // [S][U][U]
  int r;
  if ((r = fetch(c, flags, d.kpair_on, 0, n)) || (r = fetch(c, cd, d.kpair_cd, 0, 4 * n))) return r;
  for (size_t i = 0; i < n; i++) if (!flags[i]) cd[4 * i] = cd[4 * i + 1] = cd[4 * i + 2] = cd[4 * i + 3] = 0.0;
  return TJ_OK;
}
int tj_set_pair_cache(tj_ctx* c, const int* flags, const double* cd) {
  if (!c || !flags || !cd) return TJ_ERR_INVALID;
  const Dev& d = c->d;
  if (!d.optimal_plane || d.mode == 0) { c->err = "tj_set_pair_cache: needs optimal_plane and a multi-UAV mode"; return TJ_ERR_INVALID; }
  QUIESCE(c);
  const size_t n = array_count(c, d.kpair_on);   // [S][U][U]
  std::vector<int> on(n, 0), list;
  for (int tr = 0; tr < d.S; tr++) for (int a = 0; a < d.U; a++) for (int b = a + 1; b < d.U; b++) {
    const size_t i = ((size_t)tr * d.U + a) * d.U + b;
    const bool mine = (a >= d.u0 && a < d.u1) || (b >= d.u0 && b < d.u1);   // a rank only tracks pairs that touch its robots
    if (flags[i] && mine) { on[i] = 1; list.push_back((int)i); }
  }
  const int cnt = (int)list.size();
  int r;
  if ((r = store(c, d.kpair_on, 0, on.data(), n)) || (r = store(c, d.kpair_cd, 0, cd, 4 * n)) || (r = store(c, d.kpair_list, 0, list.data(), cnt)) || (r = store(c, d.kpair_n, 0, &cnt, 1))) return r;  // [1] is re-snapshot by the next k_begin
  return TJ_OK;
}

// ---- initial-trajectory planner --------------------------------------------------------------------------
namespace {
// edge_collision for a batch of edges: cut into pieces no longer than `piece_len`, one wavefront per piece
int edges_hit(tj_ctx* c, int n, const double* edges, int n_prior, const double* prior, double d, double piece_len, std::vector<int>& hit) {
  hit.assign(n, 0);
  if (n == 0) return TJ_OK;
  std::vector<double> pieces; std::vector<int> owner;
  for (int e = 0; e < n; e++) {
    const double* a = edges + 6 * (size_t)e; const double* b = a + 3;
    const double len = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
    const int k = piece_len > 0 ? std::max(1, (int)std::ceil(len / piece_len)) : 1;
    for (int i = 0; i < k; i++) {
      for (int t = 0; t < 2; t++) {
        const double s = double(i + t) / k;
        for (int x = 0; x < 3; x++) pieces.push_back(i + t == 0 ? a[x] : (i + t == k ? b[x] : a[x] + s * (b[x] - a[x])));
      }
      owner.push_back(e);
    }
  }
  const int np = (int)owner.size();
  DevBuf dp, dow, dpr, dh; int r;
  if ((r = to_dev(c, dp, pieces.data(), pieces.size() * 8)) || (r = to_dev(c, dow, owner.data(), (size_t)np * 4)) || (r = to_dev(c, dpr, prior, (size_t)n_prior * 48)) ||
      (r = to_dev(c, dh, hit.data(), (size_t)n * 4))) return r;
  if (c->d.prim == 3) hipLaunchKernelGGL((k_edge_hit<3>), dim3(np), dim3(64), 0, c->stream, c->d, np, (const double*)dp.p, (const int*)dow.p, n_prior, (const double*)dpr.p, d, (int*)dh.p);
  else hipLaunchKernelGGL((k_edge_hit<1>), dim3(np), dim3(64), 0, c->stream, c->d, np, (const double*)dp.p, (const int*)dow.p, n_prior, (const double*)dpr.p, d, (int*)dh.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(hit.data(), dh.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return check_device_errors(c);
}
double halton(unsigned i, unsigned base) { double f = 1, r = 0; while (i) { f /= base; r += f * (i % base); i /= base; } return r; }
}  // namespace

int tj_edge_collision(tj_ctx* c, int n, const double* edges, int n_prior, const double* prior, double d, int* hit) {
  if (!c || n < 0 || n_prior < 0 || (n > 0 && (!edges || !hit)) || (n_prior > 0 && !prior)) return TJ_ERR_INVALID;
  if (!c->have_cloud) { c->err = "tj_edge_collision: call tj_set_cloud first"; return TJ_ERR_INVALID; }
  QUIESCE(c);
  double ext = 0;
  for (int k = 0; k < 3; k++) ext = std::max(ext, c->cloud_hi[k] - c->cloud_lo[k]);
  std::vector<int> h;
  int r = edges_hit(c, n, edges, n_prior, prior, d, c->d.N > 0 ? ext / 16 : 0.0, h);
  if (r) return r;
  for (int i = 0; i < n; i++) hit[i] = h[i];
  return TJ_OK;
}

int tj_plan_init(tj_ctx* c, int n_robots, const double* starts, const double* goals, double bound_scale, int nodes, int min_waypoints, int cap_waypoints, double* waypoints, int* n_waypoints) {
  if (!c || n_robots < 1 || !starts || !goals || !waypoints || !n_waypoints || cap_waypoints < 3) return TJ_ERR_INVALID;
  if (!c->have_cloud) { c->err = "tj_plan_init: call tj_set_cloud first"; return TJ_ERR_INVALID; }
  QUIESCE(c);
  const double d = c->d.offset + 0.5 * c->d.margin;   // the planner's clearance (OMPL.cpp:74, multiPathPlanning3D.cpp:127)
  if (bound_scale <= 0) bound_scale = c->d.mode == TJ_MODE_SINGLE ? 1.2 : 1.5;   // admmPathPlanning3D.cpp:203-204, multiPathPlanning3D.cpp:216-217
  if (min_waypoints < 3) min_waypoints = 6;
  int K0 = nodes > 0 ? nodes : 254;
  double lo[3], hi[3], ext = 0;
  for (int k = 0; k < 3; k++) {
    lo[k] = bound_scale * c->cloud_lo[k]; hi[k] = bound_scale * c->cloud_hi[k];
    if (c->d.N == 0) { lo[k] = -10; hi[k] = 10; }
    for (int u = 0; u < n_robots; u++) { lo[k] = std::min(lo[k], std::min(starts[3 * u + k], goals[3 * u + k])); hi[k] = std::max(hi[k], std::max(starts[3 * u + k], goals[3 * u + k])); }
    ext = std::max(ext, hi[k] - lo[k]);
  }
  const double piece_len = c->d.N > 0 ? ext / 16 : 0.0;
  std::vector<double> prior;                 // edges of the robots planned so far [.][6]
  std::vector<std::vector<double>> paths(n_robots);
  std::vector<int> hit;
  int r;
  for (int u = 0; u < n_robots; u++) {
    std::vector<double> path;
    for (int K = K0;; K = 2 * K + 2) {
      // roadmap nodes: start, goal, K Halton points of the bounds (deterministic; the reference samples with OMPL's RNG)
      const int V = K + 2;
      std::vector<double> P((size_t)V * 3);
      for (int k = 0; k < 3; k++) { P[k] = starts[3 * u + k]; P[3 + k] = goals[3 * u + k]; }
      for (int i = 0; i < K; i++) { const unsigned h = (unsigned)(i + 1 + 409 * u); P[3 * (i + 2)] = lo[0] + (hi[0] - lo[0]) * halton(h, 2); P[3 * (i + 2) + 1] = lo[1] + (hi[1] - lo[1]) * halton(h, 3); P[3 * (i + 2) + 2] = lo[2] + (hi[2] - lo[2]) * halton(h, 5); }
      // all-pairs visibility with the reference's motion validator, one device batch
      std::vector<double> E; std::vector<int> ea, eb;
      E.reserve((size_t)V * (V - 1) * 3);
      for (int a = 0; a < V; a++) for (int b = a + 1; b < V; b++) { for (int k = 0; k < 3; k++) E.push_back(P[3 * a + k]); for (int k = 0; k < 3; k++) E.push_back(P[3 * b + k]); ea.push_back(a); eb.push_back(b); }
      if ((r = edges_hit(c, (int)ea.size(), E.data(), (int)(prior.size() / 6), prior.data(), d, piece_len, hit))) return r;
      // Dijkstra by Euclidean length, node 0 -> node 1 (dense: V is a few hundred)
      std::vector<double> W((size_t)V * V, INFINITY), dist(V, INFINITY);
      for (size_t e = 0; e < ea.size(); e++) if (!hit[e]) {
        const double* a = &P[3 * ea[e]]; const double* b = &P[3 * eb[e]];
        const double w = std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
        W[(size_t)ea[e] * V + eb[e]] = W[(size_t)eb[e] * V + ea[e]] = w;
      }
      std::vector<int> prev(V, -1); std::vector<char> done(V, 0);
      dist[0] = 0;
      for (int it = 0; it < V; it++) {
        int best = -1;
        for (int v = 0; v < V; v++) if (!done[v] && dist[v] < INFINITY && (best < 0 || dist[v] < dist[best])) best = v;
        if (best < 0 || best == 1) break;
        done[best] = 1;
        for (int v = 0; v < V; v++) if (!done[v] && dist[best] + W[(size_t)best * V + v] < dist[v]) { dist[v] = dist[best] + W[(size_t)best * V + v]; prev[v] = best; }
      }
      if (dist[1] < INFINITY) {
        std::vector<int> idx;
        for (int v = 1; v != -1; v = prev[v]) idx.push_back(v);
        for (auto it = idx.rbegin(); it != idx.rend(); ++it) for (int k = 0; k < 3; k++) path.push_back(P[3 * *it + k]);
        break;
      }
      if (K > 1100) { c->err = "tj_plan_init: no collision-free path for robot " + std::to_string(u) + " (start or goal inside the clearance of an obstacle?)"; return TJ_ERR_NO_PROGRESS; }
    }
    // simplify_path (Main/multiPathPlanning3D.cpp:162-203): greedy shortcutting with the same predicate, one edge at a time
    {
      const int n = (int)path.size() / 3;
      std::vector<char> rm(n, 0);
      int prev = 0, next = 2;
      for (int i = 1; i < n - 1; i++) {
        double e6[6];
        for (int k = 0; k < 3; k++) { e6[k] = path[3 * prev + k]; e6[3 + k] = path[3 * next + k]; }
        if ((r = edges_hit(c, 1, e6, (int)(prior.size() / 6), prior.data(), d, piece_len, hit))) return r;
        if (hit[0]) { prev = i; next += 1; } else { next += 1; rm[i] = 1; }
      }
      std::vector<double> kept;
      for (int i = 0; i < n; i++) if (!rm[i]) for (int k = 0; k < 3; k++) kept.push_back(path[3 * i + k]);
      path.swap(kept);
    }
    // Corner rounding (ours).  The solver's initial control net puts control points at thirds of the polyline edges
    // (init_variable, Main/multiPathPlanning3D.cpp:363-375), so the hull of a piece cuts each corner W by the triangle
    // (W + (A-W)/3, W, W + (B-W)/3).  A fan of chords across that triangle is validated with the same predicate; where it
    // fails the two edges at W are halved by collinear way points, which shrinks the triangle by 2 per round.
    for (int round = 0; round < 6; round++) {
      const int n = (int)path.size() / 3;
      std::vector<double> fan; std::vector<int> corner;
      for (int i = 1; i < n - 1; i++) {
        const double* A = &path[3 * (i - 1)]; const double* W = &path[3 * i]; const double* B = &path[3 * (i + 1)];
        double a[3], b[3], cr[3];
        for (int k = 0; k < 3; k++) { a[k] = W[k] + (A[k] - W[k]) / 3; b[k] = W[k] + (B[k] - W[k]) / 3; }
        cr[0] = (a[1] - W[1]) * (b[2] - W[2]) - (a[2] - W[2]) * (b[1] - W[1]); cr[1] = (a[2] - W[2]) * (b[0] - W[0]) - (a[0] - W[0]) * (b[2] - W[2]); cr[2] = (a[0] - W[0]) * (b[1] - W[1]) - (a[1] - W[1]) * (b[0] - W[0]);
        if (cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2] < 1e-24) continue;   // straight through W: nothing is cut
        for (int sdiv = 1; sdiv <= 4; sdiv++) {
          for (int k = 0; k < 3; k++) fan.push_back(a[k]);
          for (int k = 0; k < 3; k++) fan.push_back(W[k] + (b[k] - W[k]) * sdiv / 4.0);
          corner.push_back(i);
        }
      }
      if (corner.empty()) break;
      if ((r = edges_hit(c, (int)corner.size(), fan.data(), (int)(prior.size() / 6), prior.data(), d, piece_len, hit))) return r;
      std::vector<char> bad(n, 0);
      bool any = false;
      for (size_t e = 0; e < corner.size(); e++) if (hit[e]) { bad[corner[e]] = 1; any = true; }
      if (!any) break;
      std::vector<double> np_;
      for (int i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) np_.push_back(path[3 * i + k]);
        if (i + 1 < n && (bad[i] || bad[i + 1])) for (int k = 0; k < 3; k++) np_.push_back(0.5 * (path[3 * i + k] + path[3 * (i + 1) + k]));
      }
      path.swap(np_);
    }
    for (size_t i = 0; i + 5 < path.size(); i += 3) for (int k = 0; k < 6; k++) prior.push_back(path[i + k]);   // this robot's edges are obstacles for the next
    paths[u] = path;
  }
  // Equal way-point counts.  The reference pads a shorter path with interpolated points between its LAST two way points
  // (Main/multiPathPlanning3D.cpp:297-322), which leaves a cluster of very short pieces that all get the same piece time;
  // here the extra points go to the edges with the longest sub-segments and sit uniformly inside an edge (collinear points:
  // the polyline and its validity are unchanged, the pieces come out as even as the corners allow).
  int max_size = min_waypoints;
  for (auto& p : paths) max_size = std::max(max_size, (int)p.size() / 3);
  if (max_size > cap_waypoints) { c->err = "tj_plan_init: path needs more way points than cap_waypoints"; return TJ_ERR_CAPACITY; }
  for (int u = 0; u < n_robots; u++) {
    std::vector<double>& p = paths[u];
    const int n = (int)p.size() / 3, extra = max_size - n;
    if (extra > 0) {
      // give the extra points to the edges greedily by largest sub-segment length, then place them uniformly inside each edge
      std::vector<double> len(n - 1); std::vector<int> parts(n - 1, 1);
      for (int i = 0; i + 1 < n; i++) len[i] = std::sqrt((p[3 * i] - p[3 * i + 3]) * (p[3 * i] - p[3 * i + 3]) + (p[3 * i + 1] - p[3 * i + 4]) * (p[3 * i + 1] - p[3 * i + 4]) + (p[3 * i + 2] - p[3 * i + 5]) * (p[3 * i + 2] - p[3 * i + 5]));
      for (int k = 0; k < extra; k++) {
        int best = 0;
        for (int i = 1; i + 1 < n; i++) if (len[i] / parts[i] > len[best] / parts[best]) best = i;
        parts[best]++;
      }
      std::vector<double> q;
      for (int i = 0; i + 1 < n; i++)
        for (int j = 0; j < parts[i]; j++)
          for (int k = 0; k < 3; k++) q.push_back(j == 0 ? p[3 * i + k] : p[3 * i + k] + (p[3 * i + 3 + k] - p[3 * i + k]) * (double(j) / parts[i]));
      for (int k = 0; k < 3; k++) q.push_back(p[3 * (n - 1) + k]);
      p.swap(q);
    }
    for (int i = 0; i < max_size * 3; i++) waypoints[(size_t)u * cap_waypoints * 3 + i] = p[i];
  }
  *n_waypoints = max_size;
  return TJ_OK;
}

int tj_get_build_info(tj_ctx* c, double* bvh_build_ms, int* built_on_device) {
  if (!c) return TJ_ERR_INVALID;
  if (bvh_build_ms) *bvh_build_ms = c->bvh_build_ms;
  if (built_on_device) *built_on_device = c->bvh_on_device;
  return TJ_OK;
}

int tj_get_stats(tj_ctx* c, tj_stats* s) {
  if (!c || !s) return TJ_ERR_INVALID;
  Ctl h;
  QUIESCE(c);
  const Dev& d = c->d;
  std::vector<unsigned long long> seg(array_count(c, d.seg_stats)), ps(array_count(c, d.pair_stats)), bs(array_count(c, d.blk_stats));
  int r;
  if ((r = fetch(c, &h, d.ctl, 0, 1)) || (r = fetch(c, seg.data(), d.seg_stats, 0, seg.size())) || (r = fetch(c, ps.data(), d.pair_stats, 0, ps.size())) ||
      (r = fetch(c, bs.data(), d.blk_stats, 0, bs.size()))) return r;
  unsigned long long tot[6] = {0, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < seg.size(); i++) tot[i % 6] += seg[i];
  s->iters = (unsigned long long)(h.iter + h.pending);
  s->nodes_dcd = tot[0]; s->cand_dcd = tot[1]; s->nodes_ccd = tot[2]; s->cand_ccd = tot[3]; s->planes_obs = tot[4]; s->planes_self = tot[5];
  unsigned long long pt[2] = {0, 0};
  for (size_t i = 0; i < ps.size(); i++) pt[i % 2] += ps[i];
  unsigned long long fails = 0, evals = 0;
  for (size_t i = 0; i < (size_t)d.U * d.P; i++) fails += bs[i];
  for (size_t i = (size_t)d.U * d.P; i < bs.size(); i++) evals += bs[i];
  s->energy_evals = evals; s->llt_fail_piece = fails; s->llt_fail_robot = h.llt_fail_robot; s->newton_iters = pt[0]; s->pair_solves = pt[1];
  s->pair_tests = d.mode >= 1 ? s->iters * (unsigned long long)(d.u1 - d.u0) * d.S * d.U : 0;
  s->order_ambiguous = h.order_ambiguous; s->error_bits = h.error; s->order_unresolved = h.order_unresolved;
  s->gjk_max_sum = h.gjk_max_sum + (unsigned long long)h.gjk_max;
  s->ls_giveups = h.ls_giveups; s->ls_helper_timeouts = h.ls_helper_timeouts;
  s->head_starts = h.spec_taken;
  s->async_fallbacks = c->async_fallbacks;
  return TJ_OK;
}

}  // extern "C"

// ---- direct exchange between sharded contexts (Dev::xch; include/trajadmm.h "tj_xch_*") ------------------------------------------------------------
// Each rank owns ONE uncached block: [U][3T] control points | [U][xs] direction records | [2][XCH_MAX] arrival counters.  Peers store into it (same
// process: plain peer access; other processes: hipIpc) from inside their producing kernels; this rank's k_front / k_ccd read it.
namespace {
size_t xch_rx1_off(const Dev& d) { return (size_t)d.U * 3 * d.T; }
size_t xch_cnt_off(const Dev& d) { return xch_rx1_off(d) + (size_t)d.U * d.xs; }
size_t xch_block_bytes(const Dev& d) { return (xch_cnt_off(d) + 2 * XCH_MAX) * sizeof(double); }
}  // namespace

int tj_xch_block(tj_ctx* c, void** base, size_t* bytes) {
  if (!c) return TJ_ERR_INVALID;
  Dev& d = c->d;
  if (!d.xf) { c->err = "tj_xch_block: the direct exchange exists for sharded decoupled contexts (world > 1) only"; return TJ_ERR_UNSUPPORTED; }
  if (d.u1 - d.u0 < 1) { c->err = "tj_xch_block: this rank owns no robot (more ranks than robots)"; return TJ_ERR_UNSUPPORTED; }
  if (d.world > XCH_MAX) { c->err = "tj_xch_block: more than 16 ranks"; return TJ_ERR_UNSUPPORTED; }
  if (!c->xch_block) {
    HIPCHK(c, hipSetDevice(c->prm.device));
    const size_t nb = xch_block_bytes(d);
    void* q = nullptr;
    // uncached: written by a remote GPU (or another process) while this rank's kernels run, read by them with system-scope loads
    if (hipExtMallocWithFlags(&q, nb, hipDeviceMallocUncached) != hipSuccess) {
      (void)hipGetLastError();
      if (hipExtMallocWithFlags(&q, nb, hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); c->err = "tj_xch_block: hipExtMallocWithFlags (uncached / fine-grained) failed"; return TJ_ERR_DEVICE; }
    }
    HIPCHK(c, hipMemset(q, 0, nb));
    HIPCHK(c, hipDeviceSynchronize());
    c->xch_block = q; c->xch_bytes = nb;
    d.rx[0] = (double*)q; d.rx[1] = (double*)q + xch_rx1_off(d); d.xcnt = (unsigned long long*)((double*)q + xch_cnt_off(d));
  }
  if (base) *base = c->xch_block;
  if (bytes) *bytes = c->xch_bytes;
  return TJ_OK;
}

int tj_xch_ipc_export(tj_ctx* c, void* handle64) {
  if (!c || !handle64) return TJ_ERR_INVALID;
  { int r = tj_xch_block(c, nullptr, nullptr); if (r) return r; }
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "the ABI hands the handle over as 64 bytes");
  hipIpcMemHandle_t h;
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, hipIpcGetMemHandle(&h, c->xch_block));
  memcpy(handle64, &h, 64);
  c->xch_ipc_exported = true;
  return TJ_OK;
}

int tj_xch_ipc_open(tj_ctx* c, const void* handle64, void** base) {
  if (!c || !handle64 || !base) return TJ_ERR_INVALID;
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, 64);
  HIPCHK(c, hipSetDevice(c->prm.device));
  void* p = nullptr;
  HIPCHK(c, hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  c->xch_ipc_opened.push_back(p);
  *base = p;
  return TJ_OK;
}

int tj_xch_attach(tj_ctx* c, int n_peers, const int* peer_ranks, void* const* peer_bases) {
  if (!c || n_peers < 0 || n_peers >= XCH_MAX || (n_peers > 0 && (!peer_ranks || !peer_bases))) return TJ_ERR_INVALID;
  { int r = tj_xch_block(c, nullptr, nullptr); if (r) return r; }
  Dev& d = c->d;
  if (n_peers != d.world - 1) { c->err = "tj_xch_attach: every other rank of the world must be attached"; return TJ_ERR_INVALID; }
  XchPeers t;
  memset(&t, 0, sizeof(t));
  t.n = n_peers;
  for (int q = 0; q < n_peers; q++) {
    if (peer_ranks[q] < 0 || peer_ranks[q] >= d.world || peer_ranks[q] == d.rank || !peer_bases[q]) { c->err = "tj_xch_attach: bad peer"; return TJ_ERR_INVALID; }
    t.rank[q] = peer_ranks[q];
    double* b = (double*)peer_bases[q];
    t.rx[q][0] = b; t.rx[q][1] = b + xch_rx1_off(d); t.cnt[q] = (unsigned long long*)(b + xch_cnt_off(d));
  }
  QUIESCE(c);
  if (!c->xch_table) { int r = dalloc(c, &c->xch_table, 1); if (r) return r; }
  { int r = upload(c, c->xch_table, &t, sizeof(t)); if (r) return r; }
  d.xp = c->xch_table;
  return TJ_OK;
}

int tj_xch_enable(tj_ctx* c, int on, int wait_mode) {
  if (!c || wait_mode < 0 || wait_mode > 2) return TJ_ERR_INVALID;
  Dev& d = c->d;
  if (on && (!d.xp || !c->xch_block)) { c->err = "tj_xch_enable: tj_xch_attach has not been called"; return TJ_ERR_INVALID; }
  QUIESCE(c);
  d.xch = on ? 1 : 0; d.xch_poll = (on && wait_mode == 1) ? 1 : 0; c->ss.xch_wait_kernel = on && wait_mode == 0;
  return TJ_OK;
}

#ifdef TJ_KAT
#include "tj_kat.h"   // the known-answer hooks: test build only
#endif
#include "tj_group.h"
