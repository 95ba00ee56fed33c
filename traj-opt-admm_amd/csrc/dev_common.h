// dev_common.h -- device-side view of the solver (all pointers are HBM-resident), wave64
// helpers and small geometry routines shared by the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_gjk.h"

namespace tj {

constexpr int WAVE = 64;
// Bounds of the data-dependent device loops.  The reference has none; each bound below is placed where the reference's own loop
// can no longer end, so reaching it is true non-termination (reported, never silently different):
//  * back-off loops (`step *= 0.8`: Armijo Optimization3D_multi.h:792 / :486, CCD Step.h:89,229): 0.8^k by repeated
//    multiplication reaches its fixed point -- two denormal units, 1e-323 -- at k = 3332; an Armijo test that has not passed by
//    then (e - 1e-4*wolfe*step < E with step, hence E, no longer changing) never passes, a CCD contact still found there is a
//    contact of the state itself.  Dev::pow08 holds all 3333 values, so pow08[min(k, STEP_CAP)] IS the reference's step for any k.
//  * Newton on a pair plane's offset (Optimal_plane.h:23, exit |grad| < 1e-2 only): quadratically convergent on feasible
//    input; beyond NEWTON_CAP rounds the iterate is NaN or cycling (the reference spins).
constexpr int STEP_CAP = 3332;
constexpr int NEWTON_CAP = 4000;
constexpr int MAX_LEVELS = 12;     // 8-ary levels of the static BVH: 8^12 leaves
constexpr int FRONT_CAP = 1024;    // BFS frontier capacity per wave (LDS)

// error bits (Ctl::error)
enum : int {
  ERR_PLANE_OVERFLOW = 1,    // more separating planes for one segment than the configured capacity
  ERR_FRONT_OVERFLOW = 2,    // BVH frontier overflow (query box far larger than expected)
  ERR_LOOP_CAP = 4,          // a back-off / Newton / Armijo loop reached STEP_CAP / NEWTON_CAP: the reference's loop would not end (infeasible state)
  ERR_PAIR_OVERFLOW = 8,     // inter-robot CCD survivor list overflow
  ERR_NOT_SPD = 16,          // coupled mode: the arrowhead Newton system is not positive definite (the reference's
                             // SimplicialLLT has no fallback there either, Optimization3D_multi.h:553-557)
  // detail bits, set together with ERR_LOOP_CAP
  ERR_LS_RANGE = 32,         // coupled mode, SHARDED context: no step among the 8 * LSC_ROUNDS Armijo candidates its exchange carries (0.8^0 .. 0.8^30) was accepted
                             // (one context goes on to the reference's own end: kernels_ls.h lsc_continue)
  ERR_CCD_STUCK = 128,       // a CCD clamp found a contact at every step down to 0.8^STEP_CAP (the fixed point of step *= 0.8): the state itself is in collision (the
                             // reference spins forever there, Step.h:83-97)
  ERR_SLACK_ARMIJO = 256,    // the slack update's Armijo loop
  ERR_PLANE_REFINE = 64,     // "optimal_plane":1 -- a plane's Newton refinement hit PLANE_NEWTON_CAP / PLANE_BACKOFF_CAP
  ERR_PEER_TIMEOUT = 512,    // tj_group, flag transport: a peer's push did not arrive within 2 s (tj_group.h)
  ERR_PASS_TIMEOUT = 1024,   // large fleets: a wave waiting for passed-on robot pairs gave up after 5 ms (the queue was descheduled, e.g. several
                             // processes on one GPU); the pairs it would have taken are unsolved -- set together with ERR_LOOP_CAP
  ERR_XS_TIMEOUT = 2048,     // asynchronous Newton solve: a wait between the two queues of the context (tickets, gate, flags, the records k_ccd's units build) ran out (2 s)
};

#ifdef TJ_NO_DONE_CHECK
#define TJ_DONE(D) false
#else
// ... or a wait between the queues of the context has run out (ERR_XS_TIMEOUT: a GPU shared with another process): what is still enqueued of the batch then returns at
// once instead of running into one 2 s limit after the other -- the host restores the batch's first state and runs it again on one queue (tj_api.hip: heal_check)
#define TJ_DONE(D) ((D).ctl->done | ((D).ctl->error & ERR_XS_TIMEOUT))
#endif
struct Ctl {
  int iter;            // completed iterations (reference global `iter`)
  int done;            // stop test fired: iter>1 && gnorm<stop (Main/multiPathPlanning3D.cpp:633)
  int error;           // ERR_* bits
  int order_ambiguous; // segments whose inter-robot CCD result depended on pair order and were replayed in the reference's tree order (k_ccd_self_seq)
  int pending;         // an iteration was started by k_begin and is not yet counted in `iter`
  int epoch;           // bumped by every k_begin: stamp that marks this iteration's pair-plane slots as valid
  int slack_now;       // the slack/dual update of the PREVIOUS iteration is due (deferred so it overlaps the next planes)
  int slack_next;      // the iteration that k_begin just started still owes its slack/dual update
  int any_pair;        // robot pairs within `offset` at full step this iteration (entries of Dev::pair_list): work of the sequential CCD replay
  int order_unresolved; // segments whose pair order mattered but could not be replayed in the reference's tree order
  int ticket;          // k_linesearch blocks that have finished (the last one does the next iteration's k_begin work); + 65536 per robot that backed off
  int ls_quiet;        // iterations in a row in which every robot accepted the full step (k_linesearch: helpers stay home from LS_QUIET_ITERS on)
  int gjk_prev;        // gjk_max of the iteration before the running one (k_begin): the GJK head start's threshold follows it

  double gnorm;        // reference global `gnorm`
  // statistics for the algorithmic-byte model; accumulated over iterations
  unsigned long long llt_fail_piece, llt_fail_robot;  // PSD repairs taken (per-piece 19x19, per-robot reduced system)
  unsigned long long energy_evals;
  unsigned long long newton_iters, pair_solves;  // unused since the counters moved to Dev::pair_stats (kept for the layout)
  double wolfe_c;      // coupled mode: the global `wolfe` of update_spline (Optimization3D_multi.h:558)
  // coupled mode, one context: the Armijo decision, taken once by the last block of an evaluation round (kernels_ls.h)
  int lsf_epoch, lsf_r, lsf_c, ls_ticket;   // epoch it belongs to / accepted round and slot / arrival counter of the round's blocks
  double lsf_step;
  // length of the longest robot-pair GJK of the running iteration (only pairs with >= 6 iterations report: a handful per launch)
  // and the sum of these maxima over the iterations begun so far: the unit count of k_mid's critical path (bench.py critical_path)
  int gjk_max, spec_taken;   // spec_taken: GJK head starts k_mid continued from (kernels_pairs.h), summed over the iterations
  unsigned long long gjk_max_sum;
  // k_ccd's pair-selection blocks that have finished, counted in two levels (sixteen sub-counters, then this one: hundreds of returning
  // atomics on ONE address serialise at ~13 ns each); the last one runs the sequential pair replay + gnorm (Dev::seq_fold)
  int ccd_ticket, pad3;
  int ccd_sub[16];
  // direct exchange (Dev::xch): robots whose control points [0] / direction records [1] THIS rank has pushed to its peers so far -- every rank
  // pushes once per iteration, so a consumer expects xpush / owned rounds from every peer
  int xpush[2];
  // k_linesearch's helper protocol: primaries that gave up waiting for a post (10 us) and searched on alone / helpers that left after 5 ms without a word.
  // Both are zero on a GPU of the solver's own; a regression to the always-timeout path shows here (tj_stats) instead of only as a slower run.
  int ls_giveups, ls_helper_timeouts;
  int c2_cnt;          // coupled chain with the corner solve folded into k_xsolve (Dev::c2_fold): robots whose Schur-corner terms have been written (zeroed by begin_body)
  // coupled mode, SHARDED context whose caller follows the Armijo search beyond the candidates one exchange carries (Dev::lsc_follow, kernels_ls.h k_ls_commit):
  // 1 = none of the candidates gathered so far passes, nothing has been committed -- the caller evaluates, gathers and decides the next LSC_ROUNDS rounds;
  // lsc_e0: the summed E(x) of the search (formed with the first table, needed by the later ones)
  int lsc_pending, pad4;
  double lsc_e0;
};

// kernels of one iteration, in stream order (unit of tj_profile_kernels and of the phase stamps)
// Union kernels (K_FRONT, K_MID, K_CCD; kernels_step.h) replace their constituents in the single-GPU iteration graph.
enum { K_BEGIN = 0, K_HULLINFO, K_FRONT, K_SEP_OBS /* k_obs_query */, K_SEP_SELF_ROWS, K_MID, K_OBS_SOLVE, K_SEP_SELF_SOLVE,
       K_KEEP,                      // "optimal_plane":1 only: persistent planes, refined every iteration (kernels_keep.h)
       K_SEP_SELF_COMPACT, K_GRAD, K_XSOLVE,
       K_XSOLVE_C2,                 // coupled mode only ("decouple":0)
       K_CCD_PREP, K_CCD, K_CCD_OBS, K_CCD_SELF_PAIRS, K_CCD_SELF_SEQ, K_LINESEARCH,
       K_LS_COUPLED, K_LS_COMMIT,   // coupled mode only
       K_SLACK, K_COUNT };
constexpr const char* kKernelNames[] = {"k_begin", "k_hullinfo", "k_front", "k_obs_query", "k_sep_self_rows", "k_mid", "k_obs_solve", "k_sep_self_solve", "k_keep", "k_sep_self_compact",
                                        "k_grad", "k_xsolve", "k_xsolve_c2", "k_ccd_prep", "k_ccd", "k_ccd_obs", "k_ccd_self_pairs", "k_ccd_self_seq",
                                        "k_linesearch", "k_ls_coupled", "k_ls_commit", "k_slack"};   // tj_kernel_name
static_assert(sizeof(kKernelNames) / sizeof(kKernelNames[0]) == K_COUNT, "one name per kernel id");
constexpr int LS_HELP_MAX = 8;                 // k_linesearch: at most this many blocks per robot (16 candidates per super-round)
constexpr int LS_TAB_STRIDE = 3 * LS_HELP_MAX * 2;   // Dev::ls_tab per robot: three rotating sets (super-round % 3) of LS_HELP_MAX blocks x 2 candidates
constexpr unsigned LS_WORD_DONE = 0x7fffffffu;
constexpr int LS_QUIET_ITERS = 8;
constexpr int LS_NARROW_MIN_PLANES = 160;      // k_linesearch: a robot with at least this many planes evaluates a narrow first round (kernels_ls.h)
constexpr unsigned long long LS_TAB_EMPTY = ~0ull;   // a NaN no evaluation produces (and a false "empty" only sends the primary to its own evaluation)
constexpr int LSC_ROUNDS = 4;  // coupled Armijo search: rounds of 8 candidates evaluated per launch (steps 0.8^0 .. 0.8^30)

// Phase stamps for kernel tuning: compiled in only by `make timing` (-DTJ_PHASE_TIMING); thread 0 of
// a block stores the constant-rate wall clock at a phase boundary.  The product build has none.
constexpr int TJ_TIC_BLOCKS = 65536, TJ_TIC_SLOTS = 8;   // blocks per kernel that leave stamps (timing builds only)
#ifdef TJ_PHASE_TIMING
#define TJ_STAMP_(D, kid, slot, thr) do { if (threadIdx.x == (thr) && blockIdx.x < TJ_TIC_BLOCKS) (D).dbg[((size_t)(kid) * TJ_TIC_BLOCKS + blockIdx.x) * TJ_TIC_SLOTS + (slot)] = wall_clock64(); } while (0)
#define TJ_ORDER(v) asm volatile("" :: "v"(v))   /* the value is computed before the next stamp is taken */
#ifdef TJ_PHASE_LIGHT
/* A stamp costs its wave ~0.3 us (s_memrealtime + wait): three per GJK iteration made a slow pair look 60 % slower than it is.
   The light build (`make timing_light`) keeps what cannot distort a chain: the union kernels' block start / end, and for the block
   kernels the entry (TJ_TIC_ENTRY: first instruction, slot 7), the first phase stamp and the last one. */
#define TJ_LIGHT_KEEP(kid, slot) ((kid) == K_MID || (kid) == K_FRONT || (kid) == K_CCD || ((kid) == K_GRAD && ((slot) == 0 || (slot) == 6)) || ((kid) == K_XSOLVE && ((slot) == 0 || (slot) == 6)) || ((kid) == K_LINESEARCH && ((slot) == 0 || (slot) == 5 || (slot) == 6)))
#define TJ_TIC(D, kid, slot) do { if (TJ_LIGHT_KEEP(kid, slot)) TJ_STAMP_(D, kid, slot, 0); } while (0)
#define TJ_TIC_ENTRY(D, kid) TJ_STAMP_(D, kid, 7, 0)
#define TJ_TICB(D, kid, slot) do {} while (0)
#else
#define TJ_TIC(D, kid, slot) TJ_STAMP_(D, kid, slot, 0)
#define TJ_TIC_ENTRY(D, kid) do {} while (0)
#define TJ_TICB(D, kid, slot) TJ_STAMP_(D, kid, slot, 192)   /* first thread of k_grad's second wave group */
#endif
#else
#define TJ_TIC(D, kid, slot) do {} while (0)
#define TJ_TIC_ENTRY(D, kid) do {} while (0)
#define TJ_TICB(D, kid, slot) do {} while (0)
#define TJ_ORDER(v) do {} while (0)
#endif

// direct exchange between sharded contexts (tj_group "flag" transport, or processes that mapped each other's blocks through hipIpc): what a rank needs
// to know about its peers.  Lives in device memory (Dev::xp).
constexpr int XCH_MAX = 16;                    // ranks of a group
constexpr int XF_SEG_STRIDE = 32;              // ints between two segments' completion counters (Dev::xf_seg): a 128-byte line each
struct XchPeers {
  int n;                                       // peers (world - 1)
  int rank[XCH_MAX];                           // their ranks
  double* rx[XCH_MAX][2];                      // their receive buffers: [0] control points [U][3T], [1] direction records [U][xs]
  unsigned long long* cnt[XCH_MAX];            // their arrival counters [2][XCH_MAX] (kind, source rank)
};

struct Dev {
  // ---- parameters (3D.json + hard-coded constants of the mains) ----
  int mode, U, P, res, S, T, N;
  int u0, u1;  // robots owned by this rank: [u0,u1)
  int rank, world;
  // Sharded contexts: the hull cache / swept-hull cache of the robots OTHER ranks own is rebuilt on this rank from their control points / directions by
  // extra one-wave units at the head of k_front / k_ccd (kernels_step.h: xf_hull_body, xf_ccd_body); the pair tiles of the same launch wait for them.
  // xch = 0: the foreign slices are in place when the kernel starts (an all-gather by the caller, or tj_group's event / rccl transports, ran between the launches).
  // xch = 1: DIRECT exchange -- the producing kernels (k_linesearch / k_begin, k_xsolve) store an owned robot's slice straight into every peer's receive
  //          buffer and count it there; the foreign units wait for the owner's count, read the slice from the receive buffer and put it in place.
  int xf;                        // 1: cache units lead k_front / k_ccd: the other ranks' robots (world > 1 and Dev::fuse), or -- xf_all -- ALL robots
  int c2_fold;                   // coupled mode, one context, every robot's k_xsolve block resident at once: the block waits for all corner terms and finishes the arrowhead solve itself (no k_xsolve_c2 launch)
  int xf_all;                    // coupled mode, one context: nobody publishes a hull / swept-hull cache there (one block commits every robot, the direction comes from k_xsolve_c2),
                                 // so the obstacle units of k_front / k_ccd -- one per (robot, segment) -- publish that record themselves (write-through + the segment's counter) before
                                 // they walk, and the k_hullinfo / k_ccd_prep launches drop out of the chain
  __host__ __device__ int xf_want() const { return (xf_all || xs_async || fa_units) ? U : U - (u1 - u0); }                           // robots the units cover (= units per segment)
  __host__ __device__ int xf_units() const { return (xf && !xf_all) ? xf_want() * S : 0; }   // extra one-wave units in the grid (xf_all: the obstacle units of k_front / k_ccd publish their own robot's record instead)
  __host__ __device__ int xf_robot(int i) const { return xf_all ? i : (i < u0 ? i : i + (u1 - u0)); }
  int xch, xch_poll;             // xch_poll = 1: the foreign units poll the arrival counters themselves; 0: a k_xch_wait launch in front of the kernel has (ranks sharing a device)
  const XchPeers* xp;
  // completion counters of the foreign units, one per (kind, SEGMENT), each on a 128-byte line of its own ([2][S][XF_SEG_STRIDE] ints; zeroed by
  // begin_body): the units of segment tr add to word tr, fire and forget, and what reads that segment's records in the same launch -- its pair tiles, a
  // head start on it -- polls that word only.  (One set of sixteen words for everything, as k_ccd's selection blocks use, was a hot line here: 1 280 adds
  // and 450 polling waves on it made k_front 35 us long.)
  int* xf_seg;
  double* rx[2];                 // this rank's receive buffers (uncached memory, written by the peers)
  unsigned long long* xcnt;      // this rank's arrival counters [2][XCH_MAX]: robots of rank r whose slice of kind k has arrived, cumulative
  __host__ __device__ int n_foreign() const { return U - (u1 - u0); }
  __host__ __device__ int foreign_robot(int f) const { return f < u0 ? f : f + (u1 - u0); }            // f-th robot this rank does not own
  __host__ __device__ int owner_of(int u) const { int r = (int)(((long long)(u + 1) * world - 1) / U); while ((long long)r * U / world > u) r--; while ((long long)(r + 1) * U / world <= u) r++; return r; }
  __host__ __device__ int owned_by(int r) const { return (int)((long long)(r + 1) * U / world) - (int)((long long)r * U / world); }
  // ASYNCHRONOUS Newton solve (round 5; single-GPU chain, decoupled / single-UAV modes): k_xsolve runs on a SECOND hardware queue, released when k_mid has finished,
  // i.e. next to k_grad.  Its block of robot u sleeps until the robot's P piece blocks of k_grad have stored their 19 x 19 blocks (write-through) and taken a ticket,
  // solves, leaves direction record and swept-hull cache with write-through stores and raises the robot's flag; k_ccd -- next on the FIRST queue behind k_grad --
  // waits for the flags in its units.  The two kernel boundaries grad -> xsolve -> ccd (each ~5 us between the last useful instruction of one kernel and the first
  // of the next) disappear from the chain.  xs_sync: ints [U][32] tickets | [U][32] flags | [32] robots done | [32] xs_go -- a 128-byte line each; all but the last zeroed by begin_body.
  // The second queue's launch is released by a one-wave gate kernel in front of it (k_xs_gate: it sleeps on the word xs_go until k_grad's first block has stored this
  // chain link's sequence number xs_seq there -- an event recorded between k_mid and k_grad instead costs a 7 us marker on the first queue, measured).
  int xs_async, xs_seq; int* xs_sync;
  __host__ __device__ int* xs_go() const { return xs_sync + ((size_t)2 * U + 1) * 32; }
  __host__ __device__ int* xs_ticket(int u) const { return xs_sync + (size_t)u * 32; }
  __host__ __device__ int* xs_flag(int u) const { return xs_sync + ((size_t)U + u) * 32; }
  __host__ __device__ int* xs_done() const { return xs_sync + (size_t)2 * U * 32; }
  __host__ __device__ static size_t xs_sync_ints(int U_) { return ((size_t)2 * U_ + 2) * 32; }
  // "optimal_plane":1, multi-UAV, one context: the refinement of the planes stored before this iteration (k_keep part 2) needs nothing of this iteration's broad
  // phase -- only the committed control points -- and is as long as its slowest plane (tens of Newton rounds).  It runs on a THIRD queue from the start of the
  // iteration (gate: k_front's first block has started), next to k_front and k_mid; k_grad (its compaction reads the planes) waits for the waves' sixteen completion
  // counters.  keep_sync: ints [16][32] counters (zeroed by begin_body) | [32] go word.
  int keep_async, keep_seq, keep_waves; int* keep_sync;
  __host__ __device__ int* keep_go() const { return keep_sync + 16 * 32; }
  __host__ __device__ static size_t keep_sync_ints() { return 17 * 32; }
  // ASYNCHRONOUS FRONT (round 6; one context, all three modes, every block of the line-search kernel resident at once): inside a batch the NEXT iteration's k_front
  // runs on the second hardware queue next to this iteration's k_linesearch (coupled mode: the one-launch k_ls_coupled).  Its launch is held back by a one-wave gate
  // (k_fa_gate) until every block of the line search has started (residency counters: all of them are resident then, so a k_front block that sleeps on a flag can never
  // keep a line-search block off a compute unit); the primary block of robot u stores the accepted control net written through and raises the robot's COMMIT FLAG;
  // k_front's obstacle unit of (u, segment) prefetches what does not depend on the net, waits for the flag, forms hull / box / k-DOP intervals itself (the expressions of
  // k_hullinfo: same bits), publishes the record written through and counts itself on the segment's completion counter (xf_seg, kind 0) -- the pair tiles of the launch
  // wait for that count, a GJK head start for its two robots' flags.  The paired line search writes no hull cache (976 B x S per robot and launch: the units' job now).
  // Everything k_front leaves for later kernels goes out written through and every block counts itself done behind its acknowledged stores; the LAST block of the line
  // search -- the one that begins the next iteration -- waits for k_front (its end, or with fa_mid only its blocks' start), so the queue order k_linesearch -> k_mid still
  // holds what k_mid needs of the line search, and the two kernel boundaries k_linesearch -> k_front -> k_mid overlap k_front's work.
  //   fa      the context is eligible (tj_create)
  //   fa_units (per launch) k_linesearch: publish no hull cache -- the k_front that follows forms the records in its units; k_front: do so.  Set for the two launches of a
  //           pairing, and for the one-queue emulation of the schedule (TJ_FRONT_ASYNC_ONE_QUEUE=1: what the counter passes of tools/profile_round.sh run).  An unpaired
  //           k_linesearch -- the last of a batch, every one of a caller that asks for one iteration at a time -- publishes the cache as before and the next k_front reads it
  //   fa_seq  > 0: THIS launch is part of pairing number fa_seq (k_linesearch(i) <-> k_front(i + 1) [<-> k_mid(i + 1)]); all words below are monotonic in it -- nothing is reset
  //   fa_mid  (with fa_seq; grids of k_front that are resident all at once next to the last k_linesearch block): k_linesearch only waits until every k_front block has
  //           STARTED -- so that k_mid's waves, which then follow at once, can never keep a k_front block off the device -- and k_mid<FA> waits for k_front's end ITSELF: its
  //           first block (the watcher) polls the done counters and raises 64 go words, the pair / obstacle solve waves sleep on one of them and then read what k_front
  //           left past the caches; the slack blocks need nothing of k_front and start at once.  The second boundary (k_linesearch -> k_mid) then overlaps k_front's tail.
  //   fa_sync ints, a 128-byte line per word: [16] k_linesearch blocks started | [16] k_front blocks done | [16] k_front blocks started | [64] go words of k_mid |
  //           [U] commit flags | record {-, epoch, done} of the begun iteration
  int fa, fa_units, fa_seq, fa_mid, fa_nls, fa_nfront; int* fa_sync;
  __host__ __device__ int* fa_res(int i) const { return fa_sync + (size_t)(i & 15) * 32; }
  __host__ __device__ int* fa_fdone(int i) const { return fa_sync + (size_t)(16 + (i & 15)) * 32; }
  __host__ __device__ int* fa_fstart(int i) const { return fa_sync + (size_t)(32 + (i & 15)) * 32; }
  __host__ __device__ int* fa_go(int i) const { return fa_sync + (size_t)(48 + (i & 63)) * 32; }
  __host__ __device__ int* fa_commit(int u) const { return fa_sync + (size_t)(112 + u) * 32; }
  __host__ __device__ int* fa_rec() const { return fa_sync + (size_t)(112 + U) * 32; }
  __host__ __device__ static size_t fa_sync_ints(int U_) { return (size_t)(113 + U_) * 32; }
  int lsc_follow;   // coupled mode, sharded context: the caller follows the Armijo search to the reference's end (tj_coupled_search_pending); 0: ERR_LS_RANGE beyond 0.8^30 as in round 5
  int xs_band;  // long trajectories (piece_num > 10): the Newton solve runs on band storage (k_xsolve_band) and the swept-hull
                // cache comes from k_ccd_prep again
  int seq_tree; // k_ccd_self_seq has LDS for the reference's per-segment dynamic tree (dev_dyntree.h)
  int fuse;    // single-GPU iteration graph: k_linesearch leaves the next iteration's hull cache, so k_hullinfo is not
               // launched (the sharded schedule needs the cache for ALL robots after its all-gather and keeps the kernel;
               // folding k_ccd_prep into k_xsolve the same way was measured slower: 10 dependent segments per wave)
  double lambda, margin, offset, mu, vel_limit, acc_limit, ks, kt, stop;
  int cap_obs, cap_self, cap_pairs;
  int optimal_plane;  // "optimal_plane":1 (Optimization3D_admm.h:126-192 obstacle planes in mode 0, Optimization3D_multi.h:276-338 pair planes)
  // ---- tables (row-major 6x6) ----
  const double* basis;    // [S][36]
  const double* convert;  // [P][36]
  const double* mdyn;     // [36]
  const double* kdop;     // [49][3]
  const double* pow08;    // [STEP_CAP+1]  0.8^k by repeated multiplication, up to its fixed point
  // ---- obstacles: Morton-sorted primitives + implicit 8-ary box hierarchy ----
  // prim = 1: a point cloud (the reference's live path, BVH::InitPointcloud BVH.cpp:53-93); prim = 3: triangles (the
  // reference's dormant BVH::InitObstacle / Step::mix_step path, BVH.cpp:15-51, Step.h:313-411: BASELINE config 5)
  int prim;
  const double *px, *py, *pz;   // [N] sorted points (prim == 1)
  const double* tri;            // [N][9] sorted triangles, three vertices row-major (prim == 3)
  const float* leafbox;         // [N][6] outward-rounded fp32 box of each triangle: pre-filter before the exact fp64 test (prim == 3)
  int nlevels;                  // level 0 = boxes over 8 consecutive primitives; top level has <= 64 boxes
  int bvh_skip;                 // 1: the walk takes two levels per step while its frontier is small (kernels_sep.h bvh_query; TJ_BVH_SKIP=0: off -- same candidates, same order)
  int lvl_off[MAX_LEVELS], lvl_n[MAX_LEVELS];
  // Inner boxes are fp32, rounded OUTWARD (lo down, hi up): 24 B instead of 48 B per box visited.  A conservative box can
  // only add visits, never lose a primitive, and the leaf predicate is evaluated in fp64 on the primitive itself
  // (AABB.cc:131-148, touching counts) -- so the candidate SET and its order are exactly those of fp64 boxes.
  const float* boxes;           // [total][6] lo.xyz hi.xyz, padded slots are empty (lo=+inf, hi=-inf)
  // ---- ADMM state, column-major per robot like the reference's Eigen matrices ----
  double *spline;      // [U][3][T]
  double *p_slack;     // [U][3][6P]
  double *p_lambda;    // [U][3][6P]
  double *t_slack;     // [U][P]
  double *t_lambda;    // [U][P]
  double *piece_time;  // [U]
  // ---- per-iteration intermediates ----
  double *oplanes; int *ocount;   // obstacle planes  [U][S][cap_obs][4], [U][S]
  double *splanes; int *scount;   // inter-robot planes [U][S][cap_self][4], [U][S]
  // obstacle-plane pipeline (kernels_sep.h): candidate points per segment after the k-DOP cull, the segment's hull, one
  // (segment, slot) work item per candidate, and per-slot plane + epoch stamp before compaction into oplanes
  int *ocand, *ocand_n;           // [U][S][cap_obs], [U][S]
  double *ohull;                  // [U][S][18]
  int *obs_work, *obs_work_n;     // [U*S*cap_obs][2], [1]
  double *oraw; int *ostamp;      // [U][S][cap_obs][4], [U][S][cap_obs]
  double *hullinfo;               // [U][S][HULL_INFO_STRIDE] hull, AABB, k-DOP intervals of the current control net
  // the same AABBs / the swept pair boxes again, robot-minor [S][6][U] (lo.xyz, hi.xyz): the all-pairs box tests read
  // one component of 64 partners with one coalesced load instead of 64 strided 8-byte loads
  double *hbox, *cbox;
  double *pairplane; int *pairstamp;  // [S][U][U][4] plane of robot a against partner b, [S][U][U] epoch stamp
  // index of the stamped slots: bit b of word [S][U][ceil(U/64)] = "the slot of partner b may carry this iteration's stamp" -- set (atomicOr) by whoever stamps a
  // slot, read AND cleared by the one wave that compacts the row, which therefore looks at the stamps and planes of the set bits only (the dense row scan was
  // 1 KB of stamps + 2 KB of speculative planes per segment: 16.8 MB per launch at 256 robots).  A superset is enough: the stamp still decides.
  unsigned long long* pairbits;
  __device__ __forceinline__ void pair_mark(int tr, int a, int b) const { atomicOr(&pairbits[((size_t)tr * U + a) * ((U + 63) >> 6) + (b >> 6)], 1ull << (b & 63)); }
  int pair_rows;                   // rows per tile of the robot-pair broad phase (kernels_pairs.h)
  int mid_order;      // k_mid's grid: 0 slack | pair waves | obstacle solves; 1 (hundreds of robots) pair waves | obstacle solves | slack (kernels_step.h; TJ_MID_ORDER)
  const int* xs_gather;   // k_xsolve's overlap-add as a table (tj_create): [n*n][2] piece-block entries per entry of the reduced system, then [n][2] for the gradient; -1 none, -2 every piece (time entry)
  int pair_prio;      // large fleets: producer waves of k_mid run at wave priority 3 (TJ_PAIR_PRIO=0: off)
  int pair_lpw;       // large fleets, one pair per lane: pairs a producer wave of k_mid takes per pass (64 = every lane; TJ_PAIR_LPW)
  int pair_pass_on;   // 1 (default): large fleets pass long pair solves on to idle waves; TJ_PAIR_PASS_ON=0 keeps every pair on its lane (test hook: same bits either way)
  int* pair_ovf; unsigned long long* pair_ovf_list;   // large fleets: [0] pairs passed on by the lane solve, [1] producer waves done, [2] consumer cursor; entries (epoch << 32 | q << 20 | p0 << 9 | segment), cap_work of them
  int *pair_work; int *pair_work_n; int cap_work;  // (segment, p0, p1) triples that passed box + k-DOP this iteration
  // GJK head start (kernels_pairs.h: spec_pair_body): pairs whose GJK was long in one iteration get the first iterations of the
  // next one's query inside k_front, next to the broad phase; k_mid continues from the saved state.  0 = off (TJ_PAIR_HEAD_START=0: same bits).
  int seq_fold; double* seq_gmem_d; int* seq_gmem_i;   // > 0: k_ccd's last block finishes with k_ccd_self_seq's work (kernels_step.h); the value = acting pairs its sort holds
  int spec, spec_budget, spec_min; int* spec_n; int* spec_list; unsigned long long* spec_tag; double* spec_state; int* spec_sti;
  // "optimal_plane":1 -- planes that persist across iterations (the reference's is_seperate / seperate_c / seperate_d and
  // is_self_seperate / self_seperate_c / self_seperate_d tables, CCDUtils.cpp:30-36).  Obstacle planes (mode 0): a list per
  // (robot, segment) in insertion order, keyed by the sorted point index.  Pair planes (modes 1, 2): dense [S][U][U] table,
  // p0 < p1 only, plus the list of switched-on slots that k_keep strides over.
  int *kobs_id, *kobs_n; double *kobs_cd;       // [U][S][cap_obs], [U][S], [U][S][cap_obs][4]
  int *kpair_on, *kpair_list, *kpair_n; double *kpair_cd;  // [S][U][U], [S*U*U], [2] = {count, count at iteration start}, [S][U][U][4]
  int grad_npl; double* grad_scr;  // k_grad: planes its LDS buffer holds; per-block HBM staging [owned*P][16*(cap_obs+cap_self)] for larger segments
  double *lg, *lh;                // per-piece gradient [U][P][19] and Hessian [U][P][361] (after PSD repair)
  // search direction record per robot, robot-major so a rank's robots are one slice for the
  // all-gather: [U][xs], xs = 3T+4 : direction (T x 3 col-major), t_direction, wolfe, |g|, pad
  double *xdir; int xs;
  __host__ __device__ double* dirp(int u) const { return xdir + (size_t)u * xs; }
  __host__ __device__ double& tdir(int u) const { return xdir[(size_t)u * xs + 3 * T]; }
  __host__ __device__ double& wolfe(int u) const { return xdir[(size_t)u * xs + 3 * T + 1]; }
  __host__ __device__ double& gn(int u) const { return xdir[(size_t)u * xs + 3 * T + 2]; }
  __host__ __device__ bool multi() const { return mode >= 1; }     // robot-pair stages exist
  __host__ __device__ bool coupled() const { return mode == 2; }   // one piece_time for all robots
  // coupled mode (shared piece_time): per-robot Cholesky factor of the reduced block incl. the arrow row, the
  // forward-substituted right-hand side, the raw gradient, {Schur corner, Schur rhs, g_t} contributions,
  // and the per-(round, robot, candidate) energies of the Armijo search on the summed objective
  double *xL, *xy, *xg, *xcorner, *ls_e;
  double *k_obs_f;                // coupled + sharded: every robot's obstacle CCD exponent as a double (exchange buffer 3)
  double *xs_scr;                 // k_xsolve_band: per-robot dense scratch [owned][n*n + 4n] for the eigenvalue fallback
  int *k_obs, *k_self;            // [U] exponents: step = 0.8^k
  double *step_out;               // [U] accepted Armijo step (diagnostics)
  int *ls_hist; int ls_fast;      // [U] Armijo exponent each robot accepted in the previous iteration (-1: none yet) -- k_linesearch evaluates round 0 in the
                                  // team shape for a robot that took the full step last time (kernels_ls.h: x_energy_team); ls_fast = 0 (TJ_LS_FAST=0): never (same bits)
  // helper workgroups of k_linesearch (kernels_ls.h, "super-rounds"): with fewer robots than compute units the launch carries ls_help blocks per
  // robot; block h of a robot evaluates candidates 2h-1 and 2h of a super-round in the team shape on a CU of its own and posts the two energies.
  // k_grad's launch order (kernels_newton.h, grad_order_body): with more (robot, piece) blocks than compute units but fewer than twice as many, the
  // blocks beyond the first `num_cu` share a CU with an older block and run ~20 % slower (the SIMD issues its oldest wave first) -- they set the kernel's
  // length.  Every block leaves the wall-clock ticks it took; the next iteration's k_front ranks them and hands the late positions (and their
  // CU mates) to the cheapest items.  Which block computes which item changes no bit of any item.
  int grad_bal, num_cu;           // 1: k_grad maps blockIdx -> item through grad_perm; compute units of the device
  int *grad_cost, *grad_perm;     // [owned * P] ticks of the item's last block; [owned * P] item of launch position b (always a permutation: identity at the start)
  int ls_help_late;               // TJ_LS_HELP_LATE=<us> (test hook, same bits): helper blocks idle that long before they stage -- they then start AFTER the primary's commit, the case the late-start guard exists for
  int ls_help, ls_help_mute;      // blocks per robot (1 = none); host: compute units / owned robots, at most LS_HELP_MAX.  ls_help_mute (TJ_LS_HELP_MUTE=1, test hook): helpers leave at once
  double *ls_tab;                 // [U][3][LS_HELP_MAX][2] posted energies (set = super-round % 3) (all-ones = not there yet; reset by begin_body and, between super-rounds, by the robot's primary block)
  unsigned long long *ls_word;    // [U] (epoch << 32) | super-round the primary asks for (LS_WORD_DONE: the search is over, helpers leave)
  double *ccdinfo;                // [U][S][CCD_STRIDE] swept-hull cache of the current direction
  int *pair_list;                 // [ACT_CAP] inter-robot CCD: keys (segment, p0, p1) of the pairs within `offset` at full step; Ctl::any_pair counts them
  // per-(robot, segment) statistics slots {nodes_dcd, cand_dcd, nodes_ccd, cand_ccd, planes_obs, planes_self}:
  // each slot is only ever touched by the one wave that owns (robot, segment), so plain += suffices
  // (a shared counter would serialise ~10^4 atomics per iteration on one L2 word)
  unsigned long long* seg_stats;
  unsigned long long* blk_stats;    // [U*P] PSD repairs per piece (k_grad), then [U] energy evaluations per robot (line search): single-writer words, no atomics
  unsigned long long* pair_stats;   // [U*S][2] Optimal_plane::optimal_d iterations / robot pairs solved, spread over (lower robot, segment)
  Ctl* ctl;
  long long* dbg;  // phase stamps (TJ_PHASE_TIMING builds only, else null)
};
// P, D, obstacle box, pair box, 49 k-DOP intervals (lo,hi): 146 values in a record of 160 doubles = ten 128-byte lines of its own.  No line is shared between
// two records, so a record that another block of the SAME launch writes (sharded contexts: foreign units, then pair tiles) cannot sit half-stale in an L2
// that fetched the neighbouring record earlier in the launch.
constexpr int CCD_STRIDE = 160;
// the record's fields (helpers: "the swept-hull record", below): hull P[6][3], direction hull D[6][3], obstacle box lo / hi over {P, PD}, pair box lo / hi over {P, P + D}, interval minima, maxima
constexpr int CCD_P = 0, CCD_D = CCD_P + 18, CCD_OBOX = CCD_D + 18, CCD_PBOX = CCD_OBOX + 6, CCD_KLO = CCD_PBOX + 6, CCD_KHI = CCD_KLO + 49, CCD_REC = CCD_KHI + 49;
static_assert(CCD_REC == 146 && CCD_REC <= CCD_STRIDE, "the swept-hull record: 146 values in ten lines of its own");

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// ---- the signalling idiom of every cross-block / cross-queue protocol in this library ("Synchronisation protocols") ----
// PRODUCER: the records go out with write-through stores (agent / system scope: `global_store ... sc1`), the wave then waits until every one of them has been
// ACKNOWLEDGED (`s_waitcnt vmcnt(0)`: the counter is per wave; a barrier hands it to the other waves of a block) and only then issues the signal -- a relaxed atomic on a word
// of its own cache line.  CONSUMER: polls the word with a relaxed atomic load (`global_load ... sc1`) and reads the records afterwards, either past the caches (sc1 loads) or
// from lines its XCD's L2 cannot hold yet.  No fence instruction on either side (a release is `buffer_wbl2`: it writes back the whole L2 of the XCD, measured +14 us when
// every block of a large grid does it).  Every consumer waits through poll_until (below); every producer brackets its signal with sig_acked / sig_sent.  What the HIP memory
// model does not promise for relaxed atomics the ISA does; so that a compiler change cannot silently take it away, the sites are marked with `s_nop` immediates no compiler
// emits and tests/test_abi_and_host.py::test_signalling_sites_keep_their_order walks, in the disassembly of every kernel of the shipped code object, each marked region along
// its control flow: between "acknowledged" (0x2a1 + the s_waitcnt) and "sent" (0x2a2) there is no store but the signal itself, and a wait (0x2b1 ... 0x2b2) holds no memory
// access but the poll -- no record load, no store, no atomic (what a site does on a time-out comes after 0x2b2).
#define TJ_MARK_(imm) asm volatile("s_nop " #imm ::: "memory")
__device__ __forceinline__ void sig_acked() { TJ_MARK_(0x2a1); __builtin_amdgcn_s_waitcnt(0); asm volatile("" ::: "memory"); }   // every store this wave has issued is acknowledged
__device__ __forceinline__ void sig_sent() { TJ_MARK_(0x2a2); }                                                                   // the signal has been issued
// Limits of the waits, in ticks of the 100 MHz wall clock: a logic error or a lost peer must not hang the device.  2 s where the producer runs on another queue or
// device (a GPU shared with another process may leave that queue off the hardware for whole time slices: 5 ms was too short), 5 ms (+ 1 us per block / wave of a
// large launch: a profiler or a shared GPU stretches it) where it is a block of the same launch, 10 us where the waiter can go on without the signal.
constexpr long long WAIT_2S = 200000000ll, WAIT_5MS = 500000ll, WAIT_10US = 1000ll, WAIT_SLACK = 100ll;
// THE wait.  Polls once; after a failed poll it reads the clock (t_end == 0: the limit starts now; a caller may share one t_end over several waits) and loops
// sleep (none for SLEEP == 0), poll, deadline.  `poll` is the loop's only memory access -- an sc1 load of the signal word(s) -- and its result is wave-uniform.
// Returns whether the poll succeeded; what a site does on a time-out (error bits, counters, fallback values) it does after the call, outside the marked region.
template <int SLEEP, class Poll>
__device__ __forceinline__ bool poll_until(Poll&& poll, long long& t_end, long long ticks) {
  TJ_MARK_(0x2b1);
  bool ok = poll();
  if (!ok) {
    if (t_end == 0) t_end = wall_clock64() + ticks;
    for (;;) {
      if constexpr (SLEEP > 0) __builtin_amdgcn_s_sleep(SLEEP);
      if ((ok = poll())) break;
      if (wall_clock64() > t_end) break;
    }
  }
  TJ_MARK_(0x2b2);
  return ok;
}
template <int SLEEP, class Poll>
__device__ __forceinline__ bool poll_until(Poll&& poll, long long ticks) { long long t_end = 0; return poll_until<SLEEP>(poll, t_end, ticks); }
__device__ __forceinline__ unsigned long long ballot(bool p) { return __ballot(p); }
__device__ __forceinline__ int prefix_count(unsigned long long m) { return __popcll(m & ((1ull << lane_id()) - 1ull)); }

// a / b for 0 <= a < 2^20, b >= 1, exact: (a + 0.5) / b is at least 0.5 / b away from an integer and the float product is off by less than
// 0.13 / b.  The integer division by a run-time value is ~40 VALU instructions, and several per-lane index computations (segment ->
// piece, segment -> sub-segment) sit in front of the first load of a block.
__device__ __forceinline__ int div_small(int a, int b) { return (int)(((float)a + 0.5f) * (1.0f / (float)b)); }
// hull of segment tr of a T x 3 column-major control net: out[j*3+a] = sum_k basis[j][k] * net[3*piece+k][a]
// accumulated in k order from zero, as every variant in the reference does (e.g. Energy_admm.h:116-129); hull_sum: one such sum, B the basis row, col the piece's 6 coordinates
// ld: how a net entry is fetched -- plainly, or past the caches (xf_load, xch_load) where the net was written while the launch was running.  A caller that must
// wait for the net first fetches the basis row into registers before the wait and hands that copy in as B.
template <class Ld>
__device__ __forceinline__ double hull_sum(const double* B, const double* col, Ld&& ld) {
  double acc = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) acc += B[k] * ld(col + k);
  return acc;
}
__device__ __forceinline__ double hull_sum(const double* B, const double* col) { return hull_sum(B, col, [](const double* p) { return *p; }); }
// the operands of hull entry (j, a) of segment tr: its basis row and the 6 coordinates a of the segment's piece
__device__ __forceinline__ const double* hull_row(const Dev& D, int tr, int j) { return D.basis + (size_t)tr * 36 + j * 6; }
__device__ __forceinline__ const double* hull_col(const Dev& D, const double* net, int tr, int a) { return net + div_small(tr, D.res) * 3 + D.T * a; }
__device__ __forceinline__ double hull_entry(const Dev& D, const double* net, int tr, int j, int a) { return hull_sum(hull_row(D, tr, j), hull_col(D, net, tr, a)); }
// ---- the swept-hull record of a (robot, segment), its arithmetic written ONCE for its three writers (k_xsolve's tail, ccd_prep_segment, ccd_record_async: each keeps
// its own thread mapping, loads and stores) -- so every rank and every launch form holds the same bits.  BVH::CCDCollision box (BVH.cpp:195-250), SelfCCDCollision
// box (:289-330), k-DOP intervals of {P, P + D} (CCD.h:416-533).
// the third hull sum: basis * (net + dir), the box the reference uses for the cloud query (not P + Dh: the sum is taken per control point first)
__device__ __forceinline__ double hull_sum_pd(const double* B, const double* net, const double* dir) {
  double acc = 0;
#pragma unroll
  for (int k = 0; k < 6; k++) acc += B[k] * (net[k] + dir[k]);
  return acc;
}
struct HullTriple { double p, dh, pd; };   // one coordinate of the hull of the net, of the direction, and of net + direction
__device__ __forceinline__ HullTriple hull_triple(const double* B, const double* net, const double* dir) { return HullTriple{hull_sum(B, net), hull_sum(B, dir), hull_sum_pd(B, net, dir)}; }
// axis a of the two query boxes: the obstacle box over {P, PD} (lo, hi) and the robot-pair box over {P, P + Dh} (lo2, hi2); ps(j): coordinate a of point j of P + Dh
struct SweptBoxes { double lo, hi, lo2, hi2; };
template <class PS>
__device__ __forceinline__ SweptBoxes swept_boxes(const double* P, const double* PD, int a, PS&& ps) {
  SweptBoxes b{INFINITY, -INFINITY, INFINITY, -INFINITY};
  for (int j = 0; j < 6; j++) {
    double v = P[3 * j + a]; if (v < b.lo) b.lo = v; if (v > b.hi) b.hi = v; if (v < b.lo2) b.lo2 = v; if (v > b.hi2) b.hi2 = v;
    v = PD[3 * j + a]; if (v < b.lo) b.lo = v; if (v > b.hi) b.hi = v;
    v = ps(j); if (v < b.lo2) b.lo2 = v; if (v > b.hi2) b.hi2 = v;
  }
  return b;
}
// [lo, up] widened by the six points q (or q + d) along the k-DOP axis (x, y, z); a fresh interval starts at [+inf, -inf]
__device__ __forceinline__ void kdop_interval6(double x, double y, double z, const double* q, double& lo, double& up) {
  for (int i = 0; i < 6; i++) { const double lv = x * q[3 * i] + y * q[3 * i + 1] + z * q[3 * i + 2]; if (lv < lo) lo = lv; if (lv > up) up = lv; }
}
__device__ __forceinline__ void kdop_interval6_sum(double x, double y, double z, const double* q, const double* d, double& lo, double& up) {
  for (int i = 0; i < 6; i++) { const double lv = x * (q[3 * i] + d[3 * i]) + y * (q[3 * i + 1] + d[3 * i + 1]) + z * (q[3 * i + 2] + d[3 * i + 2]); if (lv < lo) lo = lv; if (lv > up) up = lv; }
}
// ---- direct exchange between sharded contexts (Dev::xch): producer side ---------------------------------------------------------------------
// Ordering without fences: a slice is stored with system-scope (write-through, uncached at the destination) stores, the wave then waits until every one of
// them has been ACKNOWLEDGED (s_waitcnt vmcnt(0): the counter is per wave), and only after that -- and after a barrier if several waves stored -- the
// arrival counter on the peer is bumped.  The consumer reads the counter and then the slice with system-scope loads (kernels_step.h: xch_wait_owner).
// A release fence instead would write back the whole L2 of the XCD from every block (measured in k_linesearch: +14 us).
__device__ __forceinline__ void xch_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ double xch_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
// robot u's slice of kind k (src[0, count), final; `per` doubles per robot in the receive buffer) to every peer, by the nth threads of one block (or one wave)
template <bool ONE_WAVE>
__device__ __forceinline__ void xch_push_robot(const Dev& D, int kind, int u, int per, const double* src, int count, int tid, int nth) {
  const XchPeers* xp = D.xp;
  const int np = xp->n;
  for (int q = 0; q < np; q++) {
    double* dst = xp->rx[q][kind] + (size_t)u * per;
    for (int i = tid; i < count; i += nth) xch_store(dst + i, src[i]);
  }
  sig_acked();
  if constexpr (!ONE_WAVE) __syncthreads();
  asm volatile("" ::: "memory");
  if (tid < np) __hip_atomic_fetch_add(xp->cnt[tid] + kind * XCH_MAX + D.rank, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  sig_sent();
  if (tid == 0) atomicAdd(&D.ctl->xpush[kind], 1);
}

// ---- consumer side ----
__device__ __forceinline__ void wait_failed(const Dev& D, int bits) { if (lane_id() == 0) atomicOr(&D.ctl->error, bits); }
// All `need` robots of rank r have pushed their slice of kind k for the launch that is running?  (Every rank pushes once per iteration, so the rounds
// THIS rank has pushed -- final when the kernel started -- are the rounds it may expect of a peer.)  One wave.
__device__ __forceinline__ void xch_wait_owner(const Dev& D, int kind, int r) {
  const unsigned long long need = (unsigned long long)(D.ctl->xpush[kind] / (D.u1 - D.u0)) * (unsigned long long)D.owned_by(r);
  const unsigned long long* w = D.xcnt + kind * XCH_MAX + r;
  if (!poll_until<4>([&] { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= need; }, WAIT_2S)) wait_failed(D, ERR_PEER_TIMEOUT);
}
// Foreign-robot units (kernels_step.h) leave their records with write-through stores, wait for the acknowledgements and count themselves done; the pair
// tiles of the same launch -- later in the grid, so every unit is resident or finished when a tile starts -- wait for the count.  Records are line
// aligned (HULL_INFO_STRIDE, CCD_STRIDE), so what a tile then loads cannot have been fetched by its XCD's L2 earlier in the launch.
__device__ __forceinline__ void xf_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double xf_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xf_store_i(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int xf_load_i(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int* xf_word(const Dev& D, int kind, int tr) { return D.xf_seg + ((size_t)kind * D.S + tr) * XF_SEG_STRIDE; }
__device__ __forceinline__ void xf_signal(const Dev& D, int kind, int tr) {
  sig_acked();
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(xf_word(D, kind, tr), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  sig_sent();
}
// every foreign unit of segment tr has left its record?  One wave.  (Direct exchange or an asynchronous solve: the units themselves may wait 2 s.)
__device__ __forceinline__ void xf_wait_seg(const Dev& D, int kind, int tr) {
  const int want = D.xf_want();
  const int* w = xf_word(D, kind, tr);
  const long long lim = (D.xch || D.xs_async) ? WAIT_2S + WAIT_2S / 20 : WAIT_5MS + WAIT_SLACK * gridDim.x;   // (2.1 s)
  if (!poll_until<2>([&] { return xf_load_i(w) >= want; }, lim)) wait_failed(D, ERR_LOOP_CAP | ERR_PASS_TIMEOUT);
}
// asynchronous Newton solve (Dev::xs_async): word *w has reached `want`.  One wave.
template <int SLEEP = 2>
__device__ __forceinline__ void xs_wait(const Dev& D, const int* w, int want) {
  if (!poll_until<SLEEP>([&] { return xf_load_i(w) >= want; }, WAIT_2S)) wait_failed(D, ERR_LOOP_CAP | ERR_XS_TIMEOUT);
}
// poll of sixteen counters, `stride` ints apart (one wave; lanes 0..15 load): their sum, wave-uniform
__device__ __forceinline__ int sum16(const int* base, int stride = 32) {
  int v = lane_id() < 16 ? xf_load_i(base + (size_t)lane_id() * stride) : 0;
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return __shfl(v, 0);
}
// asynchronous plane refinement (Dev::keep_async): every wave of the refinement launch (third queue) has left its planes?  Called by all threads of a block.
// (2 s: a refinement of thousands of rounds is legitimate -- the reference spins on such planes as well.)
__device__ __forceinline__ void keep_wait(const Dev& D) {
  if (threadIdx.x < 64 && !poll_until<8>([&] { return sum16(D.keep_sync) >= D.keep_waves; }, WAIT_2S)) wait_failed(D, ERR_LOOP_CAP | ERR_XS_TIMEOUT);
  __syncthreads();
  asm volatile("" ::: "memory");
}
// asynchronous front (Dev::fa_seq): the sixteen words at `base` (a 128-byte line each) sum to at least `want` (wrap-safe)?  One wave.
__device__ __forceinline__ void fa_wait16(const Dev& D, const int* base, int want) {
  if (!poll_until<4>([&] { return sum16(base) - want >= 0; }, WAIT_2S)) wait_failed(D, ERR_LOOP_CAP | ERR_XS_TIMEOUT);
}
// ... one word has reached `want` (a robot's commit flag)
__device__ __forceinline__ void fa_wait_flag(const Dev& D, const int* w, int want) {
  if (!poll_until<4>([&] { return xf_load_i(w) - want >= 0; }, WAIT_2S)) wait_failed(D, ERR_LOOP_CAP | ERR_XS_TIMEOUT);
}
// a block's stores (write-through) have been acknowledged -> it counts itself on one of sixteen words (fire and forget)
__device__ __forceinline__ void fa_count(int* w) {
  sig_acked();
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(w, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  sig_sent();
}
// a value that a kernel running at the same time on the other queue will read: written through when the solve is asynchronous
__device__ __forceinline__ void xs_out(bool wt, double* p, double v) { if (wt) xf_store(p, v); else *p = v; }

// ---- the hull record of a (robot, segment) (Dev::hullinfo, Dev::hbox), stated ONCE for its four writers: k_hullinfo, the foreign units (xf_hull_body), the
// publishing obstacle query (obs_query_body) and k_linesearch (ls_publish_hullinfo, which keeps its own thread mapping) -- tests/test_gpu_coupled.py compares what
// they leave bit for bit.  Record: hull P[6][3] at 0, box lo[3] at 18, hi[3] at 21, the 49 k-DOP intervals lo at 24, hi at 73 = 122 values in 128 doubles (eight
// 128-byte lines of its own, see CCD_STRIDE); hbox holds the boxes again as [segment][lo.xyz hi.xyz][robot] for the pair tiles.
constexpr int HULL_INFO_STRIDE = 128, HULL_BOX = 18, HULL_KLO = 24, HULL_KHI = 73;
__device__ __forceinline__ double* hull_record(const Dev& D, int u, int tr) { return D.hullinfo + ((size_t)u * D.S + tr) * HULL_INFO_STRIDE; }
__device__ __forceinline__ void hull_box_axis(const double* P, int a, double& lo, double& hi) {   // coordinate a of the hull's box
  lo = INFINITY; hi = -INFINITY;
  for (int j = 0; j < 6; j++) { const double v = P[3 * j + a]; if (v < lo) lo = v; if (v > hi) hi = v; }
}
__device__ __forceinline__ void hull_kdop_axis(const Dev& D, const double* P, int ax, double& lo, double& up) {   // the hull's interval on k-DOP axis ax
  lo = INFINITY; up = -INFINITY;
  kdop_interval6(D.kdop[3 * ax], D.kdop[3 * ax + 1], D.kdop[3 * ax + 2], P, lo, up);
}
// this lane's share of the record, one wave: hull entry p (lanes 0..17), coordinate `lane` of the box (0..2), interval on axis `lane` (0..48); other lanes' arguments are ignored.
// WT: written through (the record is read by a kernel, or by later blocks of this one, while the launch runs)
template <bool WT>
__device__ __forceinline__ void hull_record_put(const Dev& D, int u, int tr, int lane, double p, double blo, double bhi, double klo, double khi) {
  auto put = [](double* d, double v) { if constexpr (WT) xf_store(d, v); else *d = v; };
  double* o = hull_record(D, u, tr);
  if (lane < 18) put(o + lane, p);
  if (lane < 3) {
    put(o + HULL_BOX + lane, blo); put(o + HULL_BOX + 3 + lane, bhi);
    put(D.hbox + ((size_t)tr * 6 + lane) * D.U + u, blo); put(D.hbox + ((size_t)tr * 6 + 3 + lane) * D.U + u, bhi);
  }
  if (lane < 49) { put(o + HULL_KLO + lane, klo); put(o + HULL_KHI + lane, khi); }
}
// the record of the hull P (LDS, complete), computed and stored by one wave
template <bool WT>
__device__ __forceinline__ void hull_record_store(const Dev& D, int u, int tr, int lane, const double* P) {
  double blo = 0, bhi = 0, klo = 0, khi = 0;
  if (lane < 3) hull_box_axis(P, lane, blo, bhi);
  if (lane < 49) hull_kdop_axis(D, P, lane, klo, khi);
  hull_record_put<WT>(D, u, tr, lane, P[min(lane, 17)], blo, bhi, klo, khi);
}

// ---- the swept-hull record of a (robot, segment) (Dev::ccdinfo, Dev::cbox; fields CCD_P .. CCD_KHI above), stated ONCE for its writers -- ccd_prep_segment (k_ccd_prep, the
// publishing and foreign units), ccd_record_async and k_xsolve's tail, which keep their thread mappings, loads and waits -- and its readers (the two CCD stages, the replay);
// tests/test_gpu_coupled.py compares what the writers leave bit for bit.  cbox holds the pair boxes again as [segment][lo.xyz hi.xyz][robot] for the selection tiles.
// A writer hands its store in as put(double* dst, double v): plain, written through (xf_store), xs_out(wt, ...), or plain into an LDS copy of the record.
__device__ __forceinline__ double* swept_record(const Dev& D, int u, int tr) { return D.ccdinfo + ((size_t)u * D.S + tr) * CCD_STRIDE; }
__device__ __forceinline__ BodySwept swept_body(const double* rec, double step) { return BodySwept{rec + CCD_P, rec + CCD_D, step}; }   // conv{P, P + step * D}
// value e of the 36 hull values [P | D], both hulls' entry e < 18, axis a of the two boxes (the pair box also into the table), the interval on k-DOP axis ax
template <class Put>
__device__ __forceinline__ void swept_put_hull_value(double* rec, int e, double v, Put&& put) { put(rec + (e < CCD_D - CCD_P ? CCD_P + e : CCD_D + e - (CCD_D - CCD_P)), v); }
template <class Put>
__device__ __forceinline__ void swept_put_hull(double* rec, int e, double p, double dh, Put&& put) { swept_put_hull_value(rec, e, p, put); swept_put_hull_value(rec, CCD_D - CCD_P + e, dh, put); }
template <class Put, class PutBox>
__device__ __forceinline__ void swept_put_boxes(const Dev& D, double* rec, int u, int tr, int a, const SweptBoxes& b, Put&& put, PutBox&& put_cbox) {
  put(rec + CCD_OBOX + a, b.lo); put(rec + CCD_OBOX + 3 + a, b.hi); put(rec + CCD_PBOX + a, b.lo2); put(rec + CCD_PBOX + 3 + a, b.hi2);
  put_cbox(D.cbox + ((size_t)tr * 6 + a) * D.U + u, b.lo2); put_cbox(D.cbox + ((size_t)tr * 6 + 3 + a) * D.U + u, b.hi2);
}
// the swept hull's interval on the k-DOP axis k: over P and PS = P + step * D (CCD::KDOPCCD, CCD.h:415-533)
__device__ __forceinline__ void swept_kdop_axis(const V3& k, const double* P, const double* PS, double& lo, double& up) {
  lo = INFINITY; up = -INFINITY;
  kdop_interval6(k.x, k.y, k.z, P, lo, up);
  kdop_interval6(k.x, k.y, k.z, PS, lo, up);
}
template <class Put>
__device__ __forceinline__ void swept_put_interval(double* rec, int ax, double lo, double up, Put&& put) { put(rec + CCD_KLO + ax, lo); put(rec + CCD_KHI + ax, up); }
// one wave, the hulls P, Dh, PD and PS = P + Dh complete in LDS: this lane's share of the record `rec` of (u, tr) -- hull entries (lanes 0..17), box axis (0..2), interval on
// k-DOP axis `lane` (0..48; axis(): that axis, fetched by the caller where it wants the load) -- and of the box table
template <class Axis, class Put, class PutBox>
__device__ __forceinline__ void swept_record_put(const Dev& D, double* rec, int u, int tr, int lane, const double* P, const double* Dh, const double* PD, const double* PS,
                                                 Axis&& axis, Put&& put, PutBox&& put_cbox) {
  if (lane < 18) swept_put_hull(rec, lane, P[lane], Dh[lane], put);
  if (lane < 3) swept_put_boxes(D, rec, u, tr, lane, swept_boxes(P, PD, lane, [&](int j) { return PS[3 * j + lane]; }), put, put_cbox);
  if (lane < 49) {
    double lo, up;
    swept_kdop_axis(axis(), P, PS, lo, up);
    swept_put_interval(rec, lane, lo, up, put);
  }
}

__device__ __forceinline__ double seg_weight(const Dev& D, int tr) {
  int k = tr - D.res * div_small(tr, D.res);
  return (k + 1) / double(D.res) - k / double(D.res);
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }
// The two quantities bound_energy subtracts from vel_limit / acc_limit (Energy_admm.h:131-165): speed of velocity record b (0..4) and acceleration of record j (0..3)
// of a segment's 6-point hull Pp, weight w, piece time pt.  ONE association, norm3(5 d) / (w pt) and norm3(20 d2) / (w w pt pt), for the line search (kernels_ls.h) and
// the audit (kernels_audit.h), whose tests pin it bit for bit.  (k_grad's records, kernels_newton.h, follow Gradient_admm.h's association instead -- on purpose.)
__device__ __forceinline__ double hull_speed(const double* Pp, int b, double w, double pt) {
  const double vx = 5 * (Pp[3 * (b + 1)] - Pp[3 * b]), vy = 5 * (Pp[3 * (b + 1) + 1] - Pp[3 * b + 1]), vz = 5 * (Pp[3 * (b + 1) + 2] - Pp[3 * b + 2]);
  return norm3(vx, vy, vz) / (w * pt);
}
__device__ __forceinline__ double hull_accel(const double* Pp, int j, double w, double pt) {
  const double ax = 20 * (Pp[3 * (j + 2)] - 2 * Pp[3 * (j + 1)] + Pp[3 * j]), ay = 20 * (Pp[3 * (j + 2) + 1] - 2 * Pp[3 * (j + 1) + 1] + Pp[3 * j + 1]),
               az = 20 * (Pp[3 * (j + 2) + 2] - 2 * Pp[3 * (j + 1) + 2] + Pp[3 * j + 2]);
  return norm3(ax, ay, az) / (w * w * pt * pt);
}

// barrier b(d) = -(d-m)^2 ln(d/m) and its derivatives (Energy_admm.h:84-88, Gradient_admm.h:380-384)
__device__ __forceinline__ double barrier(double w, double d, double m) { return -w * (d - m) * (d - m) * log(d / m); }
__device__ __forceinline__ void barrier_d(double w, double d, double m, double& e1, double& e2) {
  e1 = -w * (2 * (d - m) * log(d / m) + (d - m) * (d - m) / d);
  e2 = -w * (2 * log(d / m) + 4 * (d - m) / d - (d - m) * (d - m) / (d * d));
}

// Integer powers x^3 .. x^6 evaluated in double-double and rounded once.  The reference calls
// std::pow(x, k) (glibc, < 0.53 ulp); a once-rounded product agrees with it except on near-ties,
// and costs ~10 instructions where the device pow() costs several hundred.
struct DD { double h, l; };
__device__ __forceinline__ DD dd_sq(double x) { const double h = x * x; return DD{h, fma(x, x, -h)}; }
__device__ __forceinline__ DD dd_mul_d(DD a, double x) { const double h = a.h * x; return DD{h, fma(a.h, x, -h) + a.l * x}; }
__device__ __forceinline__ DD dd_sq(DD a) { const double h = a.h * a.h; return DD{h, fma(a.h, a.h, -h) + 2 * (a.h * a.l)}; }
__device__ __forceinline__ double pow3(double x) { const DD r = dd_mul_d(dd_sq(x), x); return r.h + r.l; }
__device__ __forceinline__ double pow4(double x) { const DD r = dd_sq(dd_sq(x)); return r.h + r.l; }
__device__ __forceinline__ double pow5(double x) { DD q = dd_sq(dd_sq(x)); const double h = q.h + q.l; q = DD{h, (q.h - h) + q.l}; const DD r = dd_mul_d(q, x); return r.h + r.l; }
__device__ __forceinline__ double pow6(double x) { DD c = dd_mul_d(dd_sq(x), x); const double h = c.h + c.l; c = DD{h, (c.h - h) + c.l}; const DD r = dd_sq(c); return r.h + r.l; }

// Sum in the association order of Eigen's 2-wide vectorised reduction (Redux.h) -- used for the
// few scalars that feed Armijo / stop decisions (wolfe, |g|, consensus norms).
__device__ __forceinline__ double esum(const double* e, int n) {
  if (n == 0) return 0;
  int a2 = (n / 4) * 4, a1 = (n / 2) * 2;
  double r;
  if (a1) {
    double r0a = e[0], r0b = e[1];
    if (a1 > 2) {
      double r1a = e[2], r1b = e[3];
      for (int i = 4; i < a2; i += 4) { r0a += e[i]; r0b += e[i + 1]; r1a += e[i + 2]; r1b += e[i + 3]; }
      r0a += r1a; r0b += r1b;
      if (a1 > a2) { r0a += e[a2]; r0b += e[a2 + 1]; }
    }
    r = r0a + r0b;
    for (int i = a1; i < n; i++) r += e[i];
  } else {
    r = e[0];
    for (int i = 1; i < n; i++) r += e[i];
  }
  return r;
}

}  // namespace tj
