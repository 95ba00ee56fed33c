// host_launch.h -- the launch sequence of one iteration, decided in one pure function.
//
// sequence_kernel() takes a context's Dev and HostPlan, the host state of its schedules (SchedState), the schedule, the chain position and one kernel id, and
// says what is enqueued for it: a list of Launch records -- kernel, template form, queue, grid, block, dynamic LDS, scalar arguments and the Dev fields this
// launch overrides -- the gate kernels, k_xch_wait and the counter clears among them, in issue order.  It advances the state and returns whether the kernel
// exists in this schedule.  Like host_plan.h it makes no HIP runtime call, so it runs (and is tested, tests/test_launches.py) without a device; tj_api.hip's
// issue() turns a record into the launch and is the only place that names a kernel of the iteration.
#pragma once
#include "host_plan.h"

namespace tj {

// the schedule a launch belongs to:
//   Stage: the stage API (tj_run_stage) and the host's one-off launches -- every stage as its own kernels.
//   Chain: the single-context iteration, a linear chain on one queue in which independent stages share a launch (union kernels
//          k_front / k_mid / k_ccd instead of their constituents), the slack/dual update is the deferred one inside k_mid, and --
//          except in coupled mode -- the hull cache comes from k_linesearch (Dev::fuse); the asynchronous schedules (second and
//          third queue) belong to it alone.
//   Phase: the phases of a sharded iteration: union kernels as well, on the context's queue only.
enum class Sched { Stage, Chain, Phase };

// ---- the host state the sequence reads and advances (tj_ctx::ss; all ints: the test hook's record is this struct) ----
// The pairings of the cross-queue schedule each have a counter here that must match a monotonic word on the device: xs_seq <-> Dev::xs_go (k_grad opens the gate
// of its k_xsolve; xs_seq_gated: the last pairing a gate was launched for), keep_seq <-> Dev::keep_go (k_front opens the refinement's gate), fa_seq <->
// Dev::fa_sync (k_linesearch(i) <-> k_front(i + 1)).  Who resets what: restart_pairings the counters and fa_armed / fa_mid_now (with the device words),
// heal_check the two-queue flags and xs_fault (for good), checkpoint_restore the cache flags and lsc_base, tj_profile_kernels sets xs_same_queue_now around its run.
struct SchedState {
  int xs_seq = 0, xs_seq_gated = 0, keep_seq = 0, fa_seq = 0;
  int fa_armed = 0;            // the last k_linesearch enqueued belongs to pairing fa_seq: the next k_front goes to the second queue behind k_fa_gate
  int fa_mid_now = 0;          // the k_mid about to be enqueued waits for k_front itself (Dev::fa_mid)
  int hull_from_units = 0;     // the last k_linesearch published no hull cache: the next k_front forms the records
  int xs_two_queues = 0, keep_two_queues = 0;   // second / third queue in use (start as planned, HostPlan)
  int xs_same_queue_now = 0;   // tj_profile_kernels: everything on the chain's queue
  int xs_fault = 0;            // test hook TJ_XS_FAULT: the n-th gate reports a time-out
  int xf_used[2] = {0, 0};     // the cache units of k_front [0] / k_ccd [1] have counted themselves done since the last begin: a repeat of that launch before the next begin first zeroes the counters
  int ccd_valid = 0;           // Dev::fuse: the swept-hull cache of the owned robots matches their direction records (k_xsolve's tail wrote it; tj_set_direction / tj_set_state clear it)
  int ck_in_begin = 0;         // the checkpoint's device half rides in the next k_begin (checkpoint_take)
  int xch_wait_kernel = 0;     // direct exchange, wait mode 0: a one-wave k_xch_wait launch in front of k_front / k_ccd
  int lsc_base = 0;            // coupled mode, sharded context that follows the Armijo search (Dev::lsc_follow): first round of the table the next phases 4 / 5 evaluate and decide
};
constexpr int SCHED_STATE_INTS = sizeof(SchedState) / sizeof(int);

// ---- one enqueued thing ----
// what the sequence enqueues besides the kernels of the K_* enum (dev_common.h)
enum { L_XS_GATE = K_COUNT, L_KEEP_GATE, L_FA_GATE, L_XCH_WAIT, L_XF_CLEAR /* a memset of one half of Dev::xf_seg (arg 0), not a kernel */, L_COUNT };
// the Dev fields a launch overrides (every launch carries all of them; the rest of Dev is the context's)
struct DevPatch { int xs_async, keep_async, fa, xs_seq, keep_seq, fa_seq, fa_mid, fa_units, fa_nfront, fa_nls, c2_fold; };
inline void apply_patch(Dev& d, const DevPatch& p) {
  d.xs_async = p.xs_async; d.keep_async = p.keep_async; d.fa = p.fa; d.xs_seq = p.xs_seq; d.keep_seq = p.keep_seq; d.fa_seq = p.fa_seq; d.fa_mid = p.fa_mid;
  d.fa_units = p.fa_units; d.fa_nfront = p.fa_nfront; d.fa_nls = p.fa_nls; d.c2_fold = p.c2_fold;
}
// form: the template instance or argument form.  k_begin: 1 = takes the checkpoint; k_front / k_mid: 1 = the asynchronous front's waiting variant; k_grad: 1 = folded;
// k_xsolve: the inlined size N (0: generic), FORM_BAND: k_xsolve_band; k_xsolve_c2: FORM_BAND: k_xsolve_c2_band.  prim: the primitive kind of the kernels templated on it (else 0).
// queue: 0 = the context's, 1 = second, 2 = third.  arg: the scalar arguments behind Dev, in the kernel's order (pointers and the line-search layout are the issuer's).
constexpr int FORM_BAND = -1;
struct Launch { int kid, form, prim, queue, grid, block, lds, arg[4]; DevPatch patch; };
constexpr int LAUNCH_INTS = sizeof(Launch) / sizeof(int);
struct LaunchList {   // caller-provided, fixed: one iteration enqueues K_COUNT kernels at most, plus three gates, two waits, two clears and the rounds of the narrow coupled search
  static constexpr int CAP = K_COUNT + 7 + LSC_ROUNDS;
  Launch v[CAP]; int n = 0;
};

inline int xsolve_form(int P) { const int n = 9 * P - 2; return (n == 16 || n == 25 || n == 34 || n == 43 || n == 52) ? n : 0; }   // the sizes k_xsolve<N> is inlined for (kernels_newton.h)

// ---- chain position: bit 1 = this iteration's begin work was done by the previous line search (no k_begin launch); bit 2 = this iteration's line search also does
// the next iteration's begin work.  The begin rides on a line search that is ONE launch: k_linesearch (not coupled mode), or -- wide_coupled: the caller's schedule
// lets it -- the one-launch coupled search whose last block commits (lsc_wide, one context).  tj_iterate_async and the lockstep enqueue pass wide_coupled = true; the
// phases pass false (coupled mode commits in a phase of its own), and so does tj_profile_kernels, which therefore profiles the coupled chain with a k_begin per iteration.
inline int chain_position(const Dev& d, const HostPlan& h, bool wide_coupled, bool begun, bool next_follows) {
  const bool folds = d.mode != TJ_MODE_MULTI_COUPLED || (wide_coupled && h.lsc_wide && d.u1 - d.u0 == d.U);
  return folds ? ((begun ? 1 : 0) | (next_follows ? 2 : 0)) : 0;
}

// ---- the kernels of a stage (tj_run_stage) and of a phase of a sharded iteration, in issue order; which of them exist is sequence_kernel's ----
constexpr int SINGLE_ONLY = 0x100;   // listed for the single-UAV mode only
struct KernelList { int n; int k[7]; };
constexpr KernelList kStageKernels[TJ_STAGE_END] = {
  /* BEGIN */ {1, {K_BEGIN}}, /* PLANES_OBS */ {4, {K_SEP_OBS, K_OBS_SOLVE, K_KEEP | SINGLE_ONLY, K_SEP_SELF_COMPACT}},
  /* PLANES_SELF */ {5, {K_HULLINFO, K_SEP_SELF_ROWS, K_SEP_SELF_SOLVE, K_KEEP, K_SEP_SELF_COMPACT}}, /* GRAD */ {1, {K_GRAD}}, /* XSOLVE */ {2, {K_XSOLVE, K_XSOLVE_C2}},
  /* CCD_PREP */ {1, {K_CCD_PREP}}, /* CCD_OBS */ {1, {K_CCD_OBS}}, /* CCD_SELF */ {2, {K_CCD_SELF_PAIRS, K_CCD_SELF_SEQ}},
  /* LINESEARCH */ {3, {K_LINESEARCH, K_LS_COUPLED, K_LS_COMMIT}}, /* SLACK */ {1, {K_SLACK}}};
// decoupled / single: 3 phases, split at the all-gathers.  coupled ("decouple":0): 6 -- the arrowhead system, the shared CCD step and the Armijo test on the
// summed energy each need something from every robot (tj_iterate_phase, trajadmm.h)
//   phase 0: begin (stop test)                                                            -> all-gather control points
//   phase 1: hull cache (ALL robots), k_front {obstacle query | pair rows}, k_mid, compaction, gradient, Newton solve -> all-gather directions
//   phase 2: swept-hull cache (ALL robots), k_ccd, sequential pair clamp + gnorm, line search
constexpr KernelList kPhaseKernels[2][6] = {
  {{1, {K_BEGIN}}, {7, {K_HULLINFO, K_FRONT, K_MID, K_KEEP, K_SEP_SELF_COMPACT, K_GRAD, K_XSOLVE}}, {4, {K_CCD_PREP, K_CCD, K_CCD_SELF_SEQ, K_LINESEARCH}}, {0, {}}, {0, {}}, {0, {}}},
  {{1, {K_BEGIN}}, {7, {K_HULLINFO, K_FRONT, K_MID, K_KEEP, K_SEP_SELF_COMPACT, K_GRAD, K_XSOLVE}}, {1, {K_XSOLVE_C2}}, {3, {K_CCD_PREP, K_CCD, K_CCD_SELF_SEQ}}, {1, {K_LS_COUPLED}}, {1, {K_LS_COMMIT}}}};

// ---- the sequence: kernel `kid` of schedule `sched` at chain position `chain_pos` (chains and phases; 0 = an iteration on its own) ----
inline bool sequence_kernel(const Dev& d, const HostPlan& hp, SchedState& st, Sched sched, int chain_pos, int kid, LaunchList& out) {
  const bool on_chain = sched == Sched::Chain;       // the asynchronous schedules' tickets, flags and queues belong to the single-GPU chain; stage API and phases: plain
  const bool chained = sched != Sched::Stage;        // an iteration chain (one context, or the phases of a sharded schedule) as opposed to the stage API
  const bool keep2q = on_chain && st.keep_two_queues && !st.xs_same_queue_now;
  const bool fa2q = on_chain && d.fa && st.xs_two_queues && !st.xs_same_queue_now;
  const int owned = d.u1 - d.u0;
  const bool multi = d.mode >= 1, coupled = d.mode == 2, begins_next = (chain_pos & 2) != 0;
  const Grids g = plan_grids(d, hp.n_solve_env);   // (no layout reads a field of the patch)
  DevPatch p{};
  p.xs_async = on_chain ? d.xs_async : 0; p.keep_async = keep2q ? d.keep_async : 0; p.fa = on_chain ? d.fa : 0; p.c2_fold = d.c2_fold;
  p.fa_nfront = g.n_front; p.fa_nls = coupled ? owned * LSC_ROUNDS : owned * d.ls_help;
  // a record with the patch as it stands now
  auto emit = [&](int k, int form, int prim, int queue, int grid, int block, size_t lds = 0, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0) {
    if (out.n < LaunchList::CAP) out.v[out.n++] = Launch{k, form, prim, queue, grid, block, (int)lds, {a0, a1, a2, a3}, p};
  };
  auto clear = [&](int half) { if (out.n < LaunchList::CAP) out.v[out.n++] = Launch{L_XF_CLEAR, 0, 0, 0, 0, 0, 0, {half, 0, 0, 0}, DevPatch{}}; };   // (a memset: no Dev goes with it)
  auto arm_front = [&] { p.fa_seq = ++st.fa_seq; p.fa_units = 1; p.fa_mid = hp.fa_mid_ok ? 1 : 0; st.fa_armed = 1; };   // asynchronous front: the next k_front runs next to the line search about to be enqueued
  const int lsc_base = (owned != d.U && d.lsc_follow) ? st.lsc_base : 0;   // (a followed search of a sharded context: the rounds beyond the first table)
  switch (kid) {
    case K_BEGIN: if (chain_pos & 1) return false;
      if (st.ck_in_begin) { st.ck_in_begin = 0; emit(K_BEGIN, 1, 0, 0, 1 + 128, 256); }   // (checkpoint_take: the device half rides in this launch)
      else emit(K_BEGIN, 0, 0, 0, 1, 256);
      st.xf_used[0] = st.xf_used[1] = 0; return true;
    case K_HULLINFO: if ((chained && (d.fuse || d.xf_all)) || !multi) return false; emit(kid, 0, 0, 0, d.U * d.S, 64); return true;  // unfused sharded phases (coupled mode): always (all robots, after the gather)
    case K_FRONT: if (!chained) return false;
      if (d.xf) { if (st.xf_used[0]) clear(0); st.xf_used[0] = 1; }
      if (d.xch && st.xch_wait_kernel) emit(L_XCH_WAIT, 0, 0, 0, 1, 64, 0, 0);   // ranks sharing a device: the wait for the peers' control points is a launch of its own
      if (keep2q) p.keep_seq = ++st.keep_seq;   // this k_front opens the gate of the iteration's plane refinement (third queue)
      if (st.fa_armed && fa2q && (chain_pos & 1)) {   // asynchronous front: on the second queue, next to the k_linesearch just enqueued (pairing fa_seq), behind the residency gate
        st.fa_armed = 0;
        p.fa_seq = st.fa_seq; p.fa_units = 1; p.fa_mid = hp.fa_mid_ok ? 1 : 0; st.fa_mid_now = hp.fa_mid_ok ? 1 : 0;
        emit(L_FA_GATE, 0, 0, 1, 1, 64, 0, (int)((unsigned)st.fa_seq * (unsigned)p.fa_nls));
        emit(K_FRONT, 1, d.prim, 1, g.n_front, 64);
        return true;
      }
      p.fa_units = (on_chain && st.hull_from_units) ? 1 : 0;   // (the k_linesearch before it published no hull cache: one-queue emulation of the asynchronous front)
      emit(K_FRONT, 0, d.prim, 0, g.n_front, 64);
      if (keep2q) {
        p.keep_seq = 0;
        emit(L_KEEP_GATE, 0, 0, 2, 1, 64, 0, st.keep_seq);
        emit(K_KEEP, 0, 0, 2, d.keep_waves, 64, 0, 2);
      }
      return true;
    case K_SEP_OBS: if (chained) return false; emit(kid, 0, d.prim, 0, owned * d.S, 64); return true;  // stage API only
    case K_OBS_SOLVE: if (on_chain || !g.n_obs_solve) return false; emit(kid, 0, d.prim, 0, g.n_obs_solve, 64); return true;
    case K_SEP_SELF_ROWS: if (chained || !multi) return false; emit(kid, 0, 0, 0, g.n_rows, 64); return true;
    case K_MID: { if (!chained) return false;
      const bool wait = on_chain && st.fa_mid_now;   // asynchronous front, small grids: this launch starts while the iteration's k_front (pairing fa_seq) still runs -- its solve waves wait for it themselves (+ the watcher block)
      if (wait) { st.fa_mid_now = 0; p.fa_seq = st.fa_seq; p.fa_mid = 1; }
      emit(K_MID, wait ? 1 : 0, d.prim, 0, MidLayout(d, g.n_solve, g.n_obs_solve, wait, d.mid_order != 0).total, 64, 0, g.n_solve, g.n_obs_solve);
      return true; }
    case K_SEP_SELF_SOLVE: if (on_chain || !g.n_solve) return false; emit(kid, 0, 0, 0, g.n_solve, 64); return true;
    case K_KEEP:  // "optimal_plane":1 only; single UAV: a wave per segment, multi UAV: lanes over the switched-on pair slots
      if (!d.optimal_plane || (multi ? false : d.N == 0)) return false;
      emit(kid, 0, 0, 0, multi ? 1024 : owned * d.S, 64, 0, keep2q ? 1 : 0); return true;   // (asynchronous refinement: the new pairs only)
    case K_SEP_SELF_COMPACT: if (chained && hp.grad_fold) return false;   // iteration chains (single GPU and sharded phases): folded into k_grad
      emit(kid, 0, 0, 0, owned * d.S, 64); return true;
    case K_GRAD:
      if (p.xs_async && st.xs_two_queues && !st.xs_same_queue_now) p.xs_seq = ++st.xs_seq;   // this k_grad opens the gate of its k_xsolve
      if (chained && hp.grad_fold) emit(kid, 1, 0, 0, owned * d.P, GRAD_FOLD_THREADS, hp.lds_grad_of(true, d.res));
      else emit(kid, 0, 0, 0, owned * d.P, GRAD_THREADS, hp.lds_grad);
      return true;
    case K_XSOLVE: {
      if (!chained) p.c2_fold = 0;   // (the stage API's solve is followed by k_xsolve_c2)
      int q = 0;
      if (st.xs_seq_gated != st.xs_seq) {   // asynchronous solve: on the second queue, behind a gate that this iteration's k_grad opens (profiling: it simply follows k_grad on this queue)
        st.xs_seq_gated = st.xs_seq; q = 1;
        emit(L_XS_GATE, 0, 0, q, 1, 64, 0, st.xs_seq, (st.xs_fault > 0 && st.xs_seq == st.xs_fault) ? 1 : 0);
      }
      emit(kid, d.xs_band ? FORM_BAND : xsolve_form(d.P), 0, q, owned, d.xs_band ? XB_THREADS : XS_LOAD_THREADS, hp.lds_xs);
      if (chained && d.fuse && !d.xs_band) st.ccd_valid = 1;   // its tail has left the owned robots' swept-hull cache
      return true; }
    case K_XSOLVE_C2:
      if (coupled && chained && d.c2_fold) return false;   // k_xsolve has finished the arrowhead solve itself
      if (coupled) emit(kid, d.xs_band ? FORM_BAND : 0, 0, 0, owned, XS_THREADS, hp.lds_xs2);
      return coupled;
    case K_CCD_PREP: if (chained && d.xf_all) return false;                                // coupled chain: k_ccd's units build every robot's record
      if (chained && d.fuse && !d.xs_band && st.ccd_valid) return false;  // fused chains: k_xsolve's tail leaves the swept-hull cache
      if (chained && d.xf) { if (owned > 0) emit(kid, 0, 0, 0, owned * d.S, 64, 0, d.u0); }   // (the other ranks' robots: k_ccd's foreign units)
      else emit(kid, 0, 0, 0, d.U * d.S, 64, 0, 0);
      return true;
    case K_CCD: if (!chained) return false;
      if (d.xf) { if (st.xf_used[1]) clear(1); st.xf_used[1] = 1; }
      if (d.xch && st.xch_wait_kernel) emit(L_XCH_WAIT, 0, 0, 0, 1, 64, 0, 1);   // ranks sharing a device: the wait for the peers' direction records is a launch of its own
      emit(kid, 0, d.prim, 0, CcdLayout(d).total(), 64);   // (its layout counts the foreign units and the finisher of the folded pair replay)
      return true;
    case K_CCD_OBS: if (on_chain) return false; emit(kid, 0, d.prim, 0, owned * d.S, 64); return true;
    case K_CCD_SELF_PAIRS: if (on_chain || !multi) return false; emit(kid, 0, 0, 0, g.n_rows, 64); return true;
    case K_CCD_SELF_SEQ:
      if (chained && d.seq_fold) return false;   // the last block of k_ccd has done it
      if (!multi && on_chain) return false;   // single UAV: no pairs to replay, and k_xsolve has left gnorm = |g| itself -- one launch less in the chain
      emit(kid, 0, 0, 0, 1, 64, hp.lds_seq); return true;
    case K_LINESEARCH: if (coupled) return false;
      st.hull_from_units = 0;
      if (fa2q && begins_next) { arm_front(); st.hull_from_units = 1; }
      else if (on_chain && d.fa && hp.fa_emulate && begins_next) { p.fa_units = 1; st.hull_from_units = 1; }   // the next iteration of the batch follows: its k_front runs next to this launch
      emit(kid, 0, 0, 0, owned * d.ls_help, LS_THREADS, hp.lds_ls, begins_next ? 1 : 0);   // (begins_next: its last block runs begin_body)
      if (begins_next) st.xf_used[0] = st.xf_used[1] = 0;
      return true;
    // coupled mode ("decouple":0): evaluation rounds of the summed-energy Armijo search, commit
    case K_LS_COUPLED: if (!coupled) return false;
      st.hull_from_units = 0;
      if (fa2q && hp.lsc_wide && owned == d.U && begins_next) arm_front();
      if (hp.lsc_wide) { emit(kid, 0, 0, 0, owned * LSC_ROUNDS, LS_THREADS, hp.lds_ls, 0, LSC_ROUNDS, begins_next ? 1 : 0, lsc_base); if (begins_next) st.xf_used[0] = st.xf_used[1] = 0; }   // all rounds at once, one block per (robot, round)
      else for (int r = 0; r < LSC_ROUNDS; r++) emit(kid, 0, 0, 0, owned, LS_THREADS, hp.lds_ls, r, 1, 0, lsc_base);
      return true;
    case K_LS_COMMIT: if (!coupled) return false;
      if (!(hp.lsc_wide && owned == d.U)) emit(kid, 0, 0, 0, owned, 64, 0, lsc_base);   // (one context, all rounds in one launch: its last block commits)
      return true;
    case K_SLACK: if (on_chain) return false; emit(kid, 0, 0, 0, owned * d.P, 64, 0, 0); return true;
  }
  return false;
}

// the kernels of a list, in order
inline void sequence_list(const Dev& d, const HostPlan& hp, SchedState& st, Sched sched, int chain_pos, const KernelList& l, LaunchList& out) {
  for (int i = 0; i < l.n; i++)
    if (!(l.k[i] & SINGLE_ONLY) || d.mode == TJ_MODE_SINGLE) sequence_kernel(d, hp, st, sched, chain_pos, l.k[i] & ~SINGLE_ONLY, out);
}

}  // namespace tj
