/* trajadmm.h -- C ABI of the MI355X-native ADMM inner loop (libtrajadmm.so).
 *
 * Drop-in boundary for the hot path of ruiqini/traj-opt-admm.  The reference has no plugin or
 * FFI layer; its narrowest seam is one static call per ADMM iteration from the two mains plus
 * ~30 namespace-scope globals (HighOrderCCD/Utils/CCDUtils.cpp:5-44).  Each entry point below
 * names the reference interface it replaces.  Plain pointers and sizes only; no C++ or torch
 * types.  All matrices use the reference's Eigen layout: column-major, i.e. a T x 3 control net
 * is stored as [x_0..x_{T-1}, y_0.., z_0..].
 *
 * A context owns all device memory (state, BVH, scratch) on one GPU; state stays resident in
 * HBM between calls.  Calls on one context must be serialised by the caller.  Every function
 * returns TJ_OK or a negative TJ_ERR_* code; tj_last_error() gives the message.
 * The library has NO CPU fallback: without a usable HIP device tj_create fails.
 */
#ifndef TRAJADMM_H
#define TRAJADMM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tj_ctx tj_ctx;

enum {
  TJ_OK = 0,
  TJ_ERR_INVALID = -1,      /* bad argument / call order */
  TJ_ERR_DEVICE = -2,       /* HIP runtime failure or no device */
  TJ_ERR_CAPACITY = -3,     /* a device-side list overflowed (raise cap_* in tj_params) */
  TJ_ERR_NO_PROGRESS = -4,  /* a back-off / Newton / Armijo loop reached the point where the reference's own loop can no longer end (the
                               fixed point of step *= 0.8 after 3332 factors; 4000 Newton rounds): infeasible state -- the reference
                               would spin forever there (Step.h:83-97, Optimal_plane.h:23) */
  TJ_ERR_UNSUPPORTED = -5
};

enum { TJ_MODE_SINGLE = 0,      /* Optimization3D_admm::optimization            (Optimization3D_admm.h:29-33)  */
       TJ_MODE_MULTI_DECOUPLE = 1, /* Optimization3D_multi::optimization_decouple (Optimization3D_multi.h:29-33) */
       TJ_MODE_MULTI_COUPLED = 2   /* Optimization3D_multi::optimization ("decouple":0, one piece_time shared by all robots;
                                      Optimization3D_multi.h:120-174, update_spline :508-639, Step::couple_self_step Step.h:112-182);
                                      tj_get_state returns the shared piece_time for every robot */ };

/* Replaces the parameter globals of CCDUtils.cpp:5-44 that the mains fill from Config_File/3D.json
 * (Main/admmPathPlanning3D.cpp:368-397, Main/multiPathPlanning3D.cpp:478-511) and hard-code
 * (ks, kt: admmPathPlanning3D.cpp:477-478, multiPathPlanning3D.cpp:596-597). */
typedef struct tj_params {
  int mode;            /* TJ_MODE_* */
  int uav_num;         /* global `uav_num` */
  int piece_num;       /* global `piece_num` (= waypoints - 1) */
  int res;             /* "res": segments per piece */
  double lambda;       /* "lambda" */
  double margin;       /* "margin" */
  double offset;       /* "offset" */
  double mu;           /* "mu" */
  double vel_limit;    /* "vel_limit" */
  double acc_limit;    /* "acc_limit" */
  double ks;           /* 1e-8 single / 1e-3 multi */
  double kt;           /* 1 */
  double stop;         /* "stop": device-side stop test iter>1 && gnorm<stop; <=0 disables it */
  int device;          /* HIP device ordinal */
  int rank, world;     /* robot sharding: this context owns robots [rank*U/world, (rank+1)*U/world) */
  int cap_obs;         /* max obstacle planes per (robot, segment); 0 = default 256 */
  int cap_self;        /* max inter-robot planes per (robot, segment); 0 = default min(uav_num - 1, 64) */
  int cap_pairs;       /* max inter-robot CCD candidate pairs per segment; 0 = default */
  int optimal_plane;   /* "optimal_plane" (global is_optimal_plane): 1 = separating planes persist across iterations and are refined
                          by Optimal_plane::optimal_cd (single UAV, obstacle planes: Optimization3D_admm.h:120-192) /
                          self_optimal_cd (multi UAV, robot-pair planes: Optimization3D_multi.h:276-338) instead of being
                          rebuilt by GJK every iteration */
} tj_params;

/* Fills *p with the shipped 3D.json values ("Config File/3D.json") and the mode's ks/kt. */
void tj_default_params(tj_params* p, int mode, int uav_num, int piece_num);

/* The constant tables the mains precompute into globals (init_variable, Main/admmPathPlanning3D.cpp:249-353):
 * convert[P][36] = convert_list (CCDUtils.h:137-170), mdyn[36] = M_dynamic (:172-227), basis[P*res][36] = the
 * subdivide_tree bases blossom(k/res,(k+1)/res) * convert_list[i] (:229-315), kdop[49][3] = normalised k-DOP axes
 * (CCDUtils.cpp:56-119).  Row-major; any pointer may be NULL.  Host only -- needs no context and no GPU. */
int tj_host_tables(int piece_num, int res, double* convert, double* mdyn, double* basis, double* kdop);

/* LIMITS the reference does not have (it sizes everything from the init file, Main/multiPathPlanning3D.cpp:342-467); each is checked
 * and REPORTED, never silently different:
 *   uav_num <= 2048                 TJ_ERR_UNSUPPORTED from tj_create (11-bit robot fields in packed pair keys).  The robot-pair plane tables
 *                                   are dense [segments][uav_num][uav_num] (84 MB at 256 robots, 6 GB at 2048).
 *   piece_num * res <= 511, res <= 16   TJ_ERR_UNSUPPORTED from tj_create.
 *   order-dependent robot-pair clamp (Step.h:213-251: two acting pairs of one segment share a robot): replayed in the reference's
 *                                   tree order for up to 256 acting pairs per segment and 512-1024 (folded replay) / 4096 acting pairs per
 *                                   iteration; beyond that tj_iterate FAILS (TJ_ERR_UNSUPPORTED / TJ_ERR_CAPACITY, error bit 8).
 *   obstacle CCD clamp              the reference's result depends on the order in which its dynamic tree emits the candidates once GJK's
 *                                   `<= offset` decision is not monotone in the step (swept hulls > 1e4 long: directions 1e5 x a real
 *                                   iteration's); there this library returns the largest first-clear exponent over the candidates
 *                                   (tests/golden/backoff_kat.npz pins the regime boundary).
 *   back-off loops                  followed to where the reference's own loop ends (step *= 0.8 to its fixed point 1e-323 after 3332 factors);
 *                                   TJ_ERR_NO_PROGRESS only where the reference would spin forever -- in all three modes since round 5 (the coupled search
 *                                   beyond 0.8^30 is continued by one block, tests/golden/coupled_long_kat.npz).  A SHARDED coupled context (world > 1)
 *                                   exchanges 31 steps at a time: tj_group follows the search by itself, a caller that drives the phases uses
 *                                   tj_set_coupled_follow / tj_coupled_search_pending (below); without them TJ_ERR_NO_PROGRESS (detail bit 32) beyond 0.8^30.
 *   cap_obs / cap_self / cap_pairs  list capacities of tj_params; an overflow is TJ_ERR_CAPACITY with the bit that says which.
 *   several processes per GPU       one context (world == 1) of a fleet up to about one robot per compute unit enqueues its Newton solve and the next iteration's
 *                                   k_front on a SECOND stream of its own, and "optimal_plane":1 its stored planes' refinement on a third: kernels
 *                                   of one queue sleep on words kernels of the other write.  Streams of ONE process run side by side; two PROCESSES that both do this on
 *                                   one GPU shut each other out (the device runs one process's waves at a time) until a 2 s limit fires.  Not an error since round 6:
 *                                   the library restores the state the batch started from, runs the batch again on ONE queue and keeps the one-queue chain for the
 *                                   life of the context (tj_stats.async_fallbacks counts it; same results bit for bit; the incident costs its 2 s once).  TJ_HEAL=0
 *                                   restores round 5's report (TJ_ERR_NO_PROGRESS, error bit 2048); TJ_XS_ASYNC=0 TJ_KEEP_ASYNC=0 avoid the stall up front.  Under
 *                                   rocprofv3's counter collection (which serialises dispatches across queues) the library keeps one queue by itself.  Several
 *                                   contexts in ONE process: HIP lets streams beyond GPU_MAX_HW_QUEUES (4) share hardware queues, where a sleeping kernel would keep another
 *                                   context's kernels back; the contexts that sleep across queues therefore claim their streams out of a per-device budget of that many
 *                                   minus one, and a context that does not fit keeps the one-queue chain from the start (same bits). */
int tj_create(const tj_params* p, tj_ctx** out);
void tj_destroy(tj_ctx* c);
const char* tj_last_error(const tj_ctx* c);

/* Replaces BVH::InitPointcloud (HighOrderCCD/BVH/BVH.cpp:53-93) + vertex_list: uploads the
 * obstacle cloud (row-major n x 3) and builds the static device BVH.  n may be 0 ("init_ob":0). */
int tj_set_cloud(tj_ctx* c, const double* xyz, int n);

/* Obstacles as a TRIANGLE mesh instead of a point cloud (BASELINE config 5).  Replaces BVH::InitObstacle(V, F)
 * (HighOrderCCD/BVH/BVH.cpp:15-51) -- a path the reference ships but never calls: its OBJ reader keeps `v` lines only
 * (CCDUtils.h:320-390) and its live narrow phase hard-wires one-vertex obstacle bodies.  Semantics here = that path with
 * the body-2 loops the reference left commented out enabled (Separate.h:123-131: d0 = min over the triangle's vertices;
 * CCD.h:448-458: k-DOP interval over its vertices; GJK / GJKDCD / KDOPDCD already take the body size from their arguments):
 * broad phase on the triangle's box (BVH.cpp:26-46), then k-DOP, then GJK hull-vs-triangle, CCD clamp like Step::mix_step
 * (Step.h:380-404).  A triangle with three equal vertices behaves bit for bit like the cloud point.
 * vertices is row-major n_vertices x 3, faces row-major n_faces x 3 (0-based).  Replaces any cloud set before. */
int tj_set_mesh(tj_ctx* c, const double* vertices, int n_vertices, const int* faces, int n_faces);

/* Replaces init_variable (Main/admmPathPlanning3D.cpp:249-353 single,
 * Main/multiPathPlanning3D.cpp:342-467 multi): waypoints is [uav_num][piece_num+1][3], already
 * in solver units; builds spline, p_slack = C x, zero duals, t_slack = piece_time = piece_time0,
 * and resets the iteration counter. */
int tj_init_state(tj_ctx* c, const double* waypoints, double piece_time0);

/* State of robot u: the six by-reference arguments of the reference call
 * (spline T x 3, p_slack / p_lambda 6P x 3 column-major, t_slack / t_lambda P, piece_time). */
int tj_get_state(tj_ctx* c, int u, double* spline, double* p_slack, double* p_lambda, double* t_slack, double* t_lambda, double* piece_time);
int tj_set_state(tj_ctx* c, int u, const double* spline, const double* p_slack, const double* p_lambda, const double* t_slack, const double* t_lambda, double piece_time);

/* The hot path.  Runs up to n_iters ADMM iterations entirely on the device (one call of
 * Optimization3D_admm::optimization / Optimization3D_multi::optimization_decouple each), with the
 * mains' stop test evaluated on the device before every iteration.  Outputs (any may be NULL):
 * gnorm = reference global `gnorm` after the last executed iteration, iters_total = reference
 * global `iter`, converged = stop test fired. */
int tj_iterate(tj_ctx* c, int n_iters, double* gnorm, int* iters_total, int* converged);

/* Same work, asynchronous: enqueue only (no host sync, no read-back).  tj_sync waits. */
int tj_iterate_async(tj_ctx* c, int n_iters);
int tj_sync(tj_ctx* c);
/* Stream the context enqueues on (hipStream_t as void*), for event timing by the caller. */
void* tj_stream(tj_ctx* c);
/* Enqueue on a caller-owned stream instead (e.g. the stream a collective library orders against).  (The asynchronous solve's second stream, where it is
 * in use, stays the context's own; whatever is enqueued on the caller's stream behind tj_iterate_async sees the iterations' results as on one stream --
 * the chain's last kernels wait for the second stream's inside the kernels.) */
int tj_set_stream(tj_ctx* c, void* hip_stream);
/* Runs n_iters iterations with a hipEvent pair around EVERY KERNEL on the context's stream and
 * returns the summed device time per kernel in milliseconds (ms[tj_kernel_count()]) and how often each
 * kernel was launched (launches[...], may be NULL).  Same work as tj_iterate; kernel i is tj_kernel_name(i),
 * the name rocprofv3 reports (tj::<name>). */
int tj_profile_kernels(tj_ctx* c, int n_iters, double* ms, int* launches);
int tj_kernel_count(void);
/* kernels the iteration schedules of this context have enqueued so far (tj_iterate*, tj_iterate_phase*, tj_group_iterate incl. the exchange
 * kernels / collectives of its transports): launches per iteration of a schedule = the difference over a batch / its iterations */
long long tj_launch_count(tj_ctx* c);
const char* tj_kernel_name(int i);

/* ---- stage-level access (teacher-forced parity tests, profiling) ---------------------------- */
enum { TJ_STAGE_BEGIN = 0, TJ_STAGE_PLANES_OBS = 1, TJ_STAGE_PLANES_SELF = 2, TJ_STAGE_GRAD = 3, TJ_STAGE_XSOLVE = 4,
       TJ_STAGE_CCD_PREP = 5, TJ_STAGE_CCD_OBS = 6, TJ_STAGE_CCD_SELF = 7, TJ_STAGE_LINESEARCH = 8, TJ_STAGE_SLACK = 9, TJ_STAGE_END = 10 };
int tj_run_stage(tj_ctx* c, int stage);
/* planes of robot u: counts[S] (obstacle planes first, then inter-robot), planes[total][4] = (cx,cy,cz,d);
 * returns total (>=0) or an error; planes may be NULL to query the size. */
int tj_get_planes(tj_ctx* c, int u, int* counts_obs, int* counts_self, double* planes, int cap);
/* broad phase of the last plane stage for (robot u, segment seg): ids[<= cap] = obstacle primitives (indices into the cloud /
 * face list given to tj_set_cloud / tj_set_mesh, BVH traversal order) that passed BVH::DCDCollision (BVH.cpp:149-193) AND the
 * k-DOP cull (CCD::KDOPDCD); *n_broad = how many the box query alone returned for this segment SINCE tj_init_state
 * (a running total: read it after exactly one plane stage).  Returns the number of ids. */
int tj_get_candidates(tj_ctx* c, int u, int seg, int cap, int* ids, int* n_broad);
/* teacher forcing: overwrite robot u's plane lists (obstacle list only is used; self list emptied) */
int tj_set_planes(tj_ctx* c, int u, const int* counts, const double* planes);
int tj_get_direction(tj_ctx* c, int u, double* direction, double* t_direction, double* wolfe, double* gn);
int tj_get_local_grad(tj_ctx* c, int u, int piece, double* g19, double* h361);
int tj_get_steps(tj_ctx* c, double* step_self, double* step_obs, double* step_armijo);
/* Energy_admm::spline_energy (HighOrderCCD/Energy_admm.h:16-44) of every OWNED robot at the current state, against the
 * separating planes of the last iteration (the lists the last tj_iterate built): energy[uav_num], robots of other ranks 0.
 * The value the line search calls E(x); the mains do not print it, parity tests compare it with the reference's. */
int tj_get_energy(tj_ctx* c, double* energy);
/* ---- tj_audit: is the trajectory the context holds collision-free and inside its limits?  A read-only query on the device
 * (csrc/kernels_audit.h); the reference never reports these numbers.  For every OWNED robot (robots of other ranks: all-zero records):
 *   obs_clearance   min over the robot's S segments and ALL obstacle primitives (points of tj_set_cloud, triangles of tj_set_mesh) of the GJK
 *                   distance |v| between the segment's 6-point hull and the primitive -- the quantity Separate::opengjk (Separate.h:107-151) and
 *                   the CCD clamp (Step.h:83-97) compare with their ranges -- searched up to `range`: min(range, exact minimum), never a sample.
 *                   obs_segment / obs_index: where it is attained (index as given to tj_set_cloud / face index of tj_set_mesh; equal distances:
 *                   the smallest (segment, index)); -1, -1 and obs_clearance == range when nothing is closer than range.  0.0 = a hull touches.
 *   pair_clearance  min over segments tr and robots q != u of the GJK distance between the hulls of (u, tr) and (q, tr): the SAME-SEGMENT pairing
 *                   of separate_self / self_step (Optimization3D_multi.h:246-259, Step.h:196-208).  Decoupled robots carry their own piece_time,
 *                   so this is the solver's own pairing, not a distance at equal flight times (that is tj_audit_timed, below).  pair_segment / pair_robot as above (smallest
 *                   (segment, q)); single-UAV mode: range, -1, -1.  A sharded context (world > 1) reads the other ranks' control points as its
 *                   last exchange left them; tj_group_audit reads every robot's from its owner.
 *   speed, accel    max over segments and j of |order (P[j+1] - P[j])| / (weight piece_time) and
 *                   |order (order - 1) (P[j+2] - 2 P[j+1] + P[j])| / (weight^2 piece_time^2): what bound_energy subtracts from vel_limit / acc_limit
 *                   (Energy_admm.h:131-165), in the line search's association; speed_segment / accel_segment: where (the smallest on ties).
 *   duration        piece_num * piece_time, log_data's "ccd time".
 *   flags           TJ_AUDIT_OBS_CONTACT a primitive was found (obs_index >= 0) and obs_clearance <= offset, TJ_AUDIT_PAIR_CONTACT a robot was found
 *                   (pair_robot >= 0) and pair_clearance <= offset (the reference's CCD treats such a state as in contact), TJ_AUDIT_SPEED
 *                   speed >= vel_limit, TJ_AUDIT_ACCEL accel >= acc_limit (bound_energy returns infinity).  A contact flag always names what is in
 *                   contact: with range < offset a robot alone in empty space reports obs_clearance == range, index -1 and NO contact, while a
 *                   primitive closer than that range still sets the flag.
 * range <= 0 or NaN: the solver's own plane range offset + 2 * margin.  range = +infinity is valid (every primitive is a candidate; the capacity
 * limit below applies, so it suits small obstacle sets) and reports what any range beyond the largest distance reports, with `range` itself
 * (infinity) where there is no obstacle or no other robot.  seg_obs / seg_pair (may be NULL): the per-segment minima [uav_num][S] (range where
 * nothing is closer; rows of other ranks 0).  Valid any time after tj_init_state -- straight after it included, and without obstacles.  Changes no
 * solver state, statistics or launch count.  A walk whose frontier overflows is TJ_ERR_CAPACITY (lower `range`), never a smaller answer. */
enum { TJ_AUDIT_OBS_CONTACT = 1, TJ_AUDIT_PAIR_CONTACT = 2, TJ_AUDIT_SPEED = 4, TJ_AUDIT_ACCEL = 8 };
typedef struct tj_audit_robot {
  double obs_clearance;  int obs_segment, obs_index;
  double pair_clearance; int pair_segment, pair_robot;
  double speed, accel;   int speed_segment, accel_segment;
  double duration;
  int flags, reserved;
} tj_audit_robot;
int tj_audit(tj_ctx* c, double range, tj_audit_robot* out, double* seg_obs, double* seg_pair);
int tj_audit_record_size(void);   /* sizeof(tj_audit_robot), for bindings that mirror the record */
/* ---- tj_audit_timed: how close do two robots get AT THE SAME FLIGHT TIME?  The distance at equal flight times that pair_clearance above is not
 * (csrc/kernels_audit_timed.h; read-only like tj_audit).  Time is log_data's (Main/multiPathPlanning3D.cpp:31-60): t = sigma * piece_time of the robot,
 * sigma in [0, piece_num]; a robot that has arrived (t > piece_num * piece_time) stays at its last control point.  For every OWNED robot u, every segment
 * tr, every other robot q: the segment's window of time is split into 2^levels equal sub-windows, each cut further at q's segment boundaries and at q's
 * arrival; on every resulting window W both flown quintics are restricted to W (de Casteljau) and d_i = a_i - b_i, the Bezier net of p_u(t) - p_q(t) over
 * W, gives
 *   lo(W) = GJK distance of conv{d_0..d_5} from the origin: the curve lies in its hull, no separation on W is smaller (as exact as the GJK: DESIGN.md 3c)
 *   hi(W) = min(|d_0|, |d_5|): the separation at W's start / end, attained at a known time.
 *   timed_lo <= the minimum separation of u from any other robot over u's flight <= timed_hi     (both capped: min(range, ...))
 *   timed_robot / timed_segment / timed_time   partner, u's segment and the real time of the timed_hi sample; lo_robot / lo_segment: where timed_lo is attained.
 *                   -1 (time -1.0) and the value `range` where nothing is closer than range.  Equal values: the smallest (segment, partner, window).
 *   levels          the level used.
 *   flags           TJ_AUDIT_TIMED_CONTACT a partner was found and timed_hi <= offset: the two ARE within offset at timed_time; TJ_AUDIT_TIMED_CLEAR
 *                   timed_lo > offset: separation certified.  Neither: undecided at this level -- raise `levels` (the bracket narrows by about 4x per
 *                   level from level 2 on; 7x and 2.4x over the first two steps, table below), or, beyond level 6 and for the separation itself rather than a
 *                   bracket, call tj_closest_approach (below).  Single-UAV mode: range, -1, -1 and CLEAR.
 * range <= 0: offset + 2 * margin; +infinity is valid.  levels 0..6; < 0: the default TJ_AUDIT_TIMED_LEVELS.  levels > 6, or a NaN range: TJ_ERR_INVALID.
 * The default is the smallest level at which timed_hi - timed_lo < offset / 10 (contact decided to a tenth of the contact distance) for every robot with a
 * partner in range on the final states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz and e2e_scn_b_coupled.npz (measured by tests/audit_timed_ref.py, the
 * numpy restatement; largest width over the three states per level):
 *   level   0        1        2        3        4        5        6
 *   width   1.98e-2  2.78e-3  1.16e-3  3.18e-4  8.18e-5  1.83e-5  4.73e-6      (offset / 10 = 1e-2: level 1)
 * seg_lo / seg_hi (may be NULL): per-segment values [uav_num][S] (range where nothing is closer; rows of other ranks 0).  Records of other ranks' robots are
 * all zero.  A plain SHARDED context (world > 1) does not hold the other ranks' piece_time as their owners have it and returns TJ_ERR_UNSUPPORTED rather than
 * answer from stale values: use tj_group_audit_timed, which reads every robot's control points and piece_time from its owner.  Fixed number of launches
 * (two kernels), no host loop over pairs.  Changes no solver state, statistics or launch count. */
#define TJ_AUDIT_TIMED_LEVELS 1
#define TJ_AUDIT_TIMED_CONTACT 1
#define TJ_AUDIT_TIMED_CLEAR 2
typedef struct tj_audit_timed_robot {
  double timed_lo, timed_hi, timed_time;
  int timed_robot, timed_segment;
  int lo_robot, lo_segment;
  int levels, flags;
} tj_audit_timed_robot;
int tj_audit_timed(tj_ctx* c, double range, int levels, tj_audit_timed_robot* records, double* seg_lo, double* seg_hi);
int tj_audit_timed_record_size(void);   /* sizeof(tj_audit_timed_robot) */
/* ---- tj_closest_approach: the closest approach of every robot to another robot AT THE SAME FLIGHT TIME, its time and its partner, converged to a tolerance
 * the caller names (csrc/kernels_closest.h; read-only like tj_audit_timed).  tj_audit_timed's bracket comes from a uniform split and ends at level 6 (4.73e-6
 * above); here the same certified bounds drive a branch and bound that halves only the windows that can still hold the minimum.  Time, hover after arrival,
 * hull formation, the cuts at the partner's segment boundaries, the restriction of both nets and the box skip are tj_audit_timed's, unchanged.  For every
 * OWNED robot u:
 *   seeds    the windows tj_audit_timed evaluates at levels = 0, each (u's segment tr, partner q, q's segment j or its hover, [ca, cb]) with the same box
 *            prefilter against `range`; hi(W) and the time of the hi sample as above; lo(W) as above where the GJK's v separates the origin from the hull
 *            (v . d_i > 0 for all six points), 0 where it does not (see the stated limit).  best = the smallest hi < range, equal values ordered by
 *            (segment, partner, time).  The live set is {W : lo(W) < range and lo(W) < best.hi}.
 *   round d  = 1, 2, ..: every live window is halved at cm = 0.5 * (ca + cb); if cm == ca or cm == cb it cannot be split and stays in the set as terminal
 *            (counted in lo, halved no more).  Both children are evaluated by restricting the RAW segment hulls of u and q to the child (the parent's net is
 *            never restricted: rounding does not accumulate with depth).  best is updated over all children of the round, in the order (hi, segment,
 *            partner, time); then the live set becomes the children and terminals with lo < best.hi -- strict, against the round's final best, so the SET
 *            does not depend on the order of evaluation.
 *   bracket  lo = min(best.hi, min of lo over the live set), hi = best.hi.  Sound: a dropped window had lo >= best.hi at that time, and best.hi only falls.
 *   stop     hi - lo <= tol (CONVERGED) | the live set is empty (CONVERGED) | every live window is terminal | d == max_depth | the live set after a round,
 *            or after the seeding, holds more than max_windows (TRUNCATED: the record is that of the last completed round -- for the seeds the levels = 0
 *            bracket with depth 0; `windows` counts the work of the overflowing round too).  Overflow is a property of the set's size: deterministic.
 *   lo <= the minimum separation of u from any other robot over u's flight <= hi; hi is attained at `time` against `robot`, in u's segment `segment`;
 *   -1, -1 (time -1.0, lo == hi == range) when nothing is closer than range.  depth: rounds of halving completed.  windows: windows evaluated for this robot
 *   (seeds + 2 per halved window): the work done.
 * range as tj_audit_timed (<= 0: offset + 2 * margin; +infinity valid).  tol < 0: TJ_CLOSEST_TOL; 0 is valid and means "until nothing can be split or
 * dropped".  max_depth < 0: TJ_CLOSEST_MAX_DEPTH; above it TJ_ERR_INVALID (40 = a 52-bit mantissa, less 9 bits for a time of up to 512 segment lengths, with a
 * margin of 3).  max_windows <= 0: TJ_CLOSEST_FRONTIER; above it TJ_ERR_INVALID.  NaN range or tol: TJ_ERR_INVALID.  Single-UAV mode: range, range, -1.0,
 * -1, -1, depth 0, CLEAR | CONVERGED.  A plain SHARDED context (world > 1) returns TJ_ERR_UNSUPPORTED like tj_audit_timed; tj_group_closest_approach reads every
 * robot's control points and piece_time from its owner.  Records of other ranks' robots are all zero.  Four launches whatever the fleet's size and the depth,
 * no host loop over rounds, pairs or robots.  Changes no solver state, statistics or launch count.
 * STATED LIMIT: DESIGN.md 3c's contact floor -- the GJK reports up to ~1e-5 instead of 0 for an origin inside the hull -- would put lo ABOVE the truth where
 * the true separation is below that floor.  So the GJK's value counts as a lower bound only with its own certificate, a separating plane; a window without one
 * counts lo = 0 and is never dropped, only halved: in contact lo = 0 and the search runs until hi <= tol, the windows are terminal or max_depth.  At depth 0
 * lo is tj_audit_timed's min(timed_lo, timed_hi) unless such a window is live.  hi, time and the CONTACT flag involve no GJK: hi is attained.
 * The default tolerance is measured (tests/closest_ref.py default_tolerance, the restatement): tol = 0 and max_depth = 40 at the default range on the final
 * states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz and e2e_scn_b_coupled.npz; per depth the largest hi - lo over the robots with a partner in range:
 *   depth   0        1        2        3        4        5        6        7        8        9        10       11       12       13       14       15       16       17
 *   width   1.98e-2  2.78e-3  1.16e-3  3.19e-4  8.18e-5  1.83e-5  4.73e-6  1.35e-6  2.64e-7  6.58e-8  1.68e-8  4.10e-9  1.24e-9  3.28e-10 7.95e-11 1.18e-11 2.50e-12 0
 * The floor is the first depth after which the width no longer shrinks by at least 2x.  Here it shrinks all the way: at depth 17 every live set has emptied
 * (hi == lo), so the floor is the last positive width, 2.50e-12 at depth 16 (the counted rounding slack of tests/audit_timed_ref.py is 1.5e-11 at S = 40), and
 * TJ_CLOSEST_TOL is the smallest power of ten >= 10 x that. */
#define TJ_CLOSEST_CONTACT   1   /* a partner was found and hi <= offset: the two ARE within offset at `time` */
#define TJ_CLOSEST_CLEAR     2   /* lo > offset: separation certified */
#define TJ_CLOSEST_CONVERGED 4   /* hi - lo <= tol, or nothing was left that could hold a smaller separation */
#define TJ_CLOSEST_TRUNCATED 8   /* the live set outgrew max_windows: the bracket of the last completed round is returned */
#define TJ_CLOSEST_MAX_DEPTH 40
#define TJ_CLOSEST_FRONTIER  4096
#define TJ_CLOSEST_TOL 1e-10
typedef struct tj_closest_robot {
  double lo, hi, time;     /* lo <= min separation of u from any other robot over u's flight <= hi; hi is attained at `time` */
  int robot, segment;      /* partner and u's segment of the hi sample; -1, -1 (time -1.0, lo == hi == range) when nothing is closer than range */
  int depth, flags;        /* rounds of halving completed */
  int windows, reserved;   /* windows evaluated for this robot (seeds + 2 per halved window): the work done */
} tj_closest_robot;
int tj_closest_approach(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_closest_robot* records);
int tj_closest_record_size(void);   /* sizeof(tj_closest_robot) */
/* ---- tj_pair_approach: the conflict graph -- EVERY pair of robots that comes close at equal flight times, each with its own converged separation and time
 * (csrc/kernels_pair_approach.h; read-only like tj_closest_approach).  tj_closest_approach returns one record per robot, its single worst partner, and prunes
 * every other partner's windows against that partner's hi: the other separations are never computed.  Here the answer is per DIRECTED PAIR (u, q), u owned,
 * q != u: how close does u come to q at equal flight times over u's flight.  Time, hover after arrival, hull formation, the cuts at q's segment boundaries,
 * the restriction of both raw nets, the box prefilter against `range`, the certificate rule for lo and the order (hi, segment, partner, time) are
 * tj_closest_approach's, unchanged.  For one directed pair:
 *   seeds    the level-0 windows (tr, q, j, [ca, cb]) tj_audit_timed evaluates for u against this q and that pass the box prefilter.
 *   listed   (u, q) is listed if and only if some seed has lo < range or hi < range.  A pair that is not listed is certified to be at least `range` apart over
 *            u's flight and produces no row.
 *   search   tj_closest_approach's seeds / round / bracket / stop with "the robot's windows" replaced by "the pair's windows": best = the pair's smallest
 *            hi < range; live = {lo < range and lo < best.hi}; live windows are halved, children are evaluated from the RAW hulls and kept against the round's
 *            FINAL pair best; terminal windows as there.  Stop: hi - lo <= tol | live empty | every live window terminal | max_depth | a live set of THIS PAIR
 *            above max_windows (TRUNCATED: the record of the last completed round; `windows` counts the overflowing round too).  Every field is a function of
 *            the state alone.
 *   record   lo <= the minimum separation of `robot` from `partner` over robot's flight <= hi; hi is attained at `time` in robot's segment `segment`; segment
 *            -1, time -1.0 and hi == range when no sample lies below range (the pair is listed for its lo).  Flags against `offset`, tj_closest_approach's
 *            meanings and values.  (u, q) and (q, u) are two rows: u's flight and q's flight end at different times.
 *   rows     sorted by (robot, partner) ascending; neither the order of evaluation nor that of any atomic append is visible in the output.
 * *n is the number of listed pairs.  *n > cap: TJ_ERR_CAPACITY, the first `cap` rows in order have been written and *n says what to allocate; cap = 0 with
 * rows == NULL is a valid count-only call.  range <= 0: offset + 2 * margin; +infinity is valid.  tol < 0: TJ_PAIR_TOL; 0 is valid.  max_depth < 0:
 * TJ_PAIR_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0: TJ_PAIR_FRONTIER; above TJ_PAIR_MAX_WINDOWS TJ_ERR_INVALID.  NaN range or tol, n == NULL,
 * cap < 0, rows == NULL with cap > 0, a call before tj_init_state: TJ_ERR_INVALID.  Single-UAV mode: *n = 0 and TJ_OK.  A plain SHARDED context (world > 1)
 * returns TJ_ERR_UNSUPPORTED like tj_closest_approach; tj_group_pair_approach reads every robot's control points and piece_time from its owner and returns
 * the owners' rows in (robot, partner) order, bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, and is a function of cap and max_windows (S = piece_num * res segments):
 *   cap * (2 * max_windows * (40 + 8) + (2 * S + 2) * 48 + 16 + 48) bytes     (live lists and their children's lo, the pairs' level-0 seeds, counters and rows)
 * plus the bitmask, owned * ceil(uav_num / 32) * 8 bytes (512 KB at 2048 robots).  A call whose figure exceeds TJ_PAIR_MAX_BYTES is refused up front with
 * TJ_ERR_INVALID: lower cap (rows beyond it are counted, not lost) or max_windows.  At the defaults a row costs 10 144 bytes at S = 40.
 * At most FOUR launches whatever the fleet's size, the number of pairs and the depth; no host loop over robots, pairs or rounds.  Changes no solver state,
 * statistics or launch count.  tj_closest_approach's STATED LIMIT (a window without the GJK's certificate counts lo = 0) holds here per pair.
 * The defaults are measured (tests/pair_approach_ref.py default_tolerance, the restatement, on the CPU): tol = 0 and max_depth = 40 at the default range on the
 * final states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz and e2e_scn_b_coupled.npz; per depth the largest hi - lo over the listed pairs:
 *   depth   0        1        2        3        4        5        6        7        8        9        10       11       12       13       14       15       16       17
 *   width   2.14e-2  3.61e-3  1.32e-3  3.19e-4  8.18e-5  1.83e-5  4.73e-6  1.35e-6  2.64e-7  6.58e-8  1.68e-8  4.10e-9  1.24e-9  3.28e-10 7.95e-11 1.18e-11 2.50e-12 0
 * The width shrinks all the way: the floor is the last positive width, 2.50e-12 at depth 16, and TJ_PAIR_TOL is the smallest power of ten >= 10 x that.
 *   state                 listed directed pairs   largest live set of any pair at any depth
 *   e2e_scn_b (8 UAVs)    14                      2
 *   e2e_scn_c3 (64 UAVs)  126                     2
 *   e2e_scn_b_coupled     14                      2
 * TJ_PAIR_FRONTIER is the next power of two >= 4 x the largest live set, and at least 64.  The listed pairs are what `cap` has to hold at the default range:
 * about two per robot on a converged state (each robot's neighbours in both directions). */
#define TJ_PAIR_CONTACT   1   /* hi < range was found and hi <= offset: the two ARE within offset at `time` */
#define TJ_PAIR_CLEAR     2   /* lo > offset: separation of this pair certified over robot's flight */
#define TJ_PAIR_CONVERGED 4   /* hi - lo <= tol, or nothing was left that could hold a smaller separation */
#define TJ_PAIR_TRUNCATED 8   /* the pair's live set outgrew max_windows: the bracket of the last completed round is returned */
#define TJ_PAIR_MAX_DEPTH 40
#define TJ_PAIR_FRONTIER  64
#define TJ_PAIR_MAX_WINDOWS 4096
#define TJ_PAIR_MAX_BYTES (1ll << 31)
#define TJ_PAIR_TOL 1e-10
typedef struct tj_pair_record {
  double lo, hi, time;            /* lo <= min separation of `robot` from `partner` over robot's flight <= hi */
  int robot, partner, segment, depth, flags, windows;
} tj_pair_record;
int tj_pair_approach(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_pair_record* rows, int cap, int* n);
int tj_pair_record_size(void);   /* sizeof(tj_pair_record) */
/* ---- tj_path_crossings: where the PATHS of two robots meet in space, whatever the time, and when each of the two is there
 * (csrc/kernels_path_crossing.h; read-only like tj_pair_approach).  Every other robot-against-robot query pairs the robots at equal segment indices (tj_audit)
 * or at equal real time (tj_audit_timed, tj_closest_approach, tj_pair_approach, tj_flight_profile): a fleet they all certify may still have two paths through one
 * point a few tenths of a second apart, safe only while every vehicle keeps its timetable.  Here the two flown curves are compared AS CURVES, with no reference
 * to time: one row per UNORDERED pair (u, q), u < q, u owned, whose minimum over all x on u's curve and all y on q's of |x - y| may lie below `range`.
 * A pair with CLEAR is separated in space: no timing error brings the two into contact.  A pair with CONTACT is separated by timing only, and
 * partner_time - time is the margin of that timing.  For one pair:
 *   item     (tr, j, [sa, sb], [ra, rb]): a window of segment tr of u and a window of segment j of q, both in the segments' local parameters in [0, 1].
 *            Windows are dyadic, so halving at 0.5 * (sa + sb) and 0.5 * (ra + rb) is exact, and with max_depth <= 40 no item is ever unsplittable: there
 *            are no terminal items (as in tj_obstacle_approach).
 *   nets     a_0..a_5 = u's raw hull of segment tr (hull_entry's sums) restricted to [sa, sb] by blossoming (bez_restrict), b_0..b_5 = q's of segment j
 *            restricted to [ra, rb]; always from the RAW hulls, never from a parent's net: rounding does not accumulate with depth.  [0, 1] returns the raw
 *            hull bit for bit.
 *   lo(W)    |v|, v = gjk(conv{a_i}, conv{b_k}) with u's net as body 1 (the lower robot index goes first: plane_pair's order), where v SEPARATES the two:
 *            v . (a_i - b_k) > 0 for all 36 vertex pairs, evaluated as (v.x * dx + v.y * dy) + v.z * dz.  Otherwise lo(W) = 0, and the item is never
 *            dropped, only split (tj_closest_approach's certificate and its reason: the GJK's contact floor).
 *   hi(W)    the smallest of the four distances norm3(a_i - b_k), i, k in {0, 5}: points of the two curves, at s = sa or sb and partner_s = ra or rb.
 *            Candidates and bests are ordered by the total order (hi, segment, partner_segment, s, partner_s).
 *   seeds    for every (tr, j) the pair of full windows [0, 1] x [0, 1] whose raw hull boxes are within `range` of each other on every axis (the box test
 *            of tj_audit's robot pairs, with its guard: a gap above range * 1.000001 + 1e-9 on an axis skips the seed).
 *   listed   (u, q) has a row if and only if some seed has lo < range or hi < range.  A pair without a row is certified at least `range` apart in space.
 *   search   best = the pair's smallest hi < range over the seeds; live = {lo < range and lo < best.hi}.  A round splits every live item into its four
 *            quadrants (both windows halved), evaluates all children, updates best over the whole round, and keeps the children with lo < best.hi --
 *            strict, against the round's FINAL best, so that every field (`windows` and `depth` included) is a function of the state alone.
 *   bracket  lo = min(best.hi, min of lo over the live set), hi = best.hi.
 *   stop     hi - lo <= tol (CONVERGED) | the live set is empty (CONVERGED) | depth == max_depth | the live set of this pair after a round, or after the
 *            seeding, holds more than max_windows (TRUNCATED: the record is that of the last completed round -- for the seeds their own bracket with
 *            depth 0; `windows` counts the work of the overflowing round too).
 *   record   lo <= the minimum distance of the two paths <= hi.  hi is the distance of u's curve at parameter `s` of `segment` from q's curve at `partner_s` of
 *            `partner_segment`.  time = ((segment + s) / res) * piece_time[robot] and partner_time = ((partner_segment + partner_s) / res) *
 *            piece_time[partner] -- tj_obstacle_approach's expression for a time -- say when each robot is at that place.  Listed for its lo only (no sample
 *            below range): segments -1, parameters and times -1.0, hi == range.  depth: rounds completed.  windows: seeds evaluated + 4 per split item.
 *   rows     sorted by (robot, partner) ascending; neither the order of evaluation nor that of any atomic append is visible in the output.
 * ROBOT_END / PARTNER_END: the hi sample is that robot's LAST control point (segment == S - 1, parameter == 1.0).  The robot stays at that point after
 * arriving (tj_audit_timed's hover), so partner_time - time then UNDERSTATES how long the two are near: the other robot must not pass that place at any
 * later time either.  tj_timing_margin gives the slip such a pair tolerates, with the arrived robot's stay counted.
 * *n is the number of listed pairs.  *n > cap: TJ_ERR_CAPACITY, the first `cap` rows in order have been written and *n says what to allocate; cap = 0 with
 * rows == NULL is a valid count-only call.  range <= 0: offset + 2 * margin; +infinity is valid.  tol < 0: TJ_CROSSING_TOL; 0 is valid.  max_depth < 0:
 * TJ_CROSSING_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0: TJ_CROSSING_FRONTIER; above TJ_CROSSING_MAX_WINDOWS TJ_ERR_INVALID.  NaN range or tol,
 * n == NULL, cap < 0, rows == NULL with cap > 0, a call before tj_init_state: TJ_ERR_INVALID.  Single-UAV mode: *n = 0 and TJ_OK.  A plain SHARDED context
 * (world > 1) returns TJ_ERR_UNSUPPORTED like tj_pair_approach: it does not hold the peers' piece_time.  tj_group_path_crossings computes the rows (u, q > u)
 * on u's owner with control points and piece_time read from the owners, and is bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, and is a function of cap and max_windows alone (nothing is sized by S^2: the pair's
 * kernel enumerates its own (tr, j) box tests):
 *   cap * (2 * max_windows * 48 + 4 * max_windows * 8 + 8 + 80) bytes     (live lists, their children's lo, the slots' pairs and the rows)
 * plus the bitmask and its offsets, owned * ceil(uav_num / 32) * 8 bytes.  A call whose figure exceeds TJ_CROSSING_MAX_BYTES is refused up front with
 * TJ_ERR_INVALID: lower cap (rows beyond it are counted, not lost) or max_windows.
 * At most THREE launches whatever the fleet's size, the number of pairs and the depth (two for a count-only call); no host loop over robots, pairs or
 * rounds.  Changes no solver state, statistics or launch count.
 * STATED LIMITS.  (1) A certified lo is the GJK's |v|, up to 1e-10 |v| relative above the hulls' distance (tj_obstacle_approach's limit, unchanged).
 * (2) Where the paths truly meet no window around the meeting point has a certificate: lo = 0 and hi falls by about half per round, so such a row ends at
 * max_depth or at hi <= tol, with CONTACT long before.  (3) Paths that run ALONGSIDE each other have a valley instead of a point: the live set grows with
 * the depth and the row is TRUNCATED with the last bracket, which is still sound.
 * The defaults are measured (tests/path_crossing_ref.py default_tolerance, the restatement, on the CPU): tol = 0 and max_depth = 40 at the default range on the
 * final states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz, e2e_scn_b_coupled.npz and of e2e_scn_c3.npz with z set to 0 (the fleets are stacked in z; flattened
 * they cross); per depth the largest hi - lo over the listed pairs:
 *   depth   0        1        2        3        4        5        6        7        8        9        10       11       12       13       14       15       16       17       18       19       20       21       22       23       24       25       26       27       28       29       30       31       32       33       34       35       36       37       38       39       40
 *   width   5.07e-2  4.69e-2  4.68e-2  3.94e-2  1.97e-2  1.04e-2  5.66e-3  2.84e-3  1.39e-3  7.06e-4  3.38e-4  1.62e-4  9.10e-5  4.26e-5  2.13e-5  1.14e-5  5.37e-6  2.68e-6  1.33e-6  6.76e-7  3.38e-7  1.76e-7  8.58e-8  4.40e-8  2.17e-8  1.07e-8  5.32e-9  2.76e-9  1.32e-9  6.83e-10 3.32e-10 1.66e-10 8.17e-11 4.20e-11 2.04e-11 1.04e-11 5.38e-12 2.75e-12 1.36e-12 6.63e-13 3.34e-13
 * and the same over the rows that are NOT in contact (hi > offset: the pairs separated in space, whose bracket closes on a positive distance):
 *   apart   2.15e-2  3.62e-3  1.36e-3  6.39e-4  5.78e-4  1.01e-4  2.07e-5  8.51e-6  2.15e-6  5.07e-7  1.12e-7  3.27e-8  8.06e-9  1.61e-9  5.09e-10 1.12e-10 3.01e-11 7.21e-12 0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0        0
 *   state                 listed pairs   rows in contact   largest live set of any pair at any depth
 *   e2e_scn_b (8 UAVs)    7              0                 6
 *   e2e_scn_c3 (64 UAVs)  63             0                 53
 *   e2e_scn_b_coupled     7              0                 7
 *   e2e_scn_c3_flat       2016           2016              59
 * A row in contact never closes its bracket where the paths meet (limit 2): its width is hi, halved per round down to 3.34e-13 at depth 40.  The rows that
 * are not in contact shrink all the way: their last positive width is 7.21e-12 at depth 17, and TJ_CROSSING_TOL is the smallest power of ten >= 10 x that.
 * TJ_CROSSING_FRONTIER is the next power of two >= 4 x the largest live set (59: stacked neighbours, which run alongside each other, hold up to 53 before their
 * bracket closes; the flattened fleet's 2016 crossings hold at most 59), and at least 64.  The listed pairs are what `cap` has to hold at the default range: about one per robot
 * on a fleet stacked in z, every pair where all paths cross. */
#define TJ_CROSSING_CONTACT     1    /* a sample was found and hi <= offset: the PATHS are within offset in space; the pair's separation rests on timing */
#define TJ_CROSSING_CLEAR       2    /* lo > offset: no timing error brings these two into contact */
#define TJ_CROSSING_CONVERGED   4    /* hi - lo <= tol, or nothing was left that could hold a smaller distance */
#define TJ_CROSSING_TRUNCATED   8    /* the pair's live set outgrew max_windows: the bracket of the last completed round is returned */
#define TJ_CROSSING_ROBOT_END   16   /* the hi sample is robot's last control point: it stays there after arriving */
#define TJ_CROSSING_PARTNER_END 32   /* the same for partner */
#define TJ_CROSSING_MAX_DEPTH 40
#define TJ_CROSSING_FRONTIER  256
#define TJ_CROSSING_MAX_WINDOWS 4096
#define TJ_CROSSING_MAX_BYTES (1ll << 31)
#define TJ_CROSSING_TOL 1e-10
typedef struct tj_crossing_record {
  double lo, hi;                  /* lo <= min distance of robot's path from partner's path <= hi */
  double s, partner_s;            /* local parameters of the hi sample in `segment` and `partner_segment` */
  double time, partner_time;      /* when robot / partner is at the hi sample; partner_time - time is the timing margin of the crossing */
  int robot, partner, segment, partner_segment, depth, flags, windows, reserved;
} tj_crossing_record;
int tj_path_crossings(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_crossing_record* rows, int cap, int* n);
int tj_crossing_record_size(void);   /* sizeof(tj_crossing_record) */
/* ---- tj_timing_margin: by how much may one robot run late or early against another before the two come within `dist`
 * (csrc/kernels_timing_margin.h; read-only like tj_path_crossings).  The timed queries say how close two robots come ON the timetable, tj_path_crossings how
 * close their paths are whatever the time; its partner_time - time is the timing gap at the spatially closest place, which overstates what the timetable
 * tolerates: contact begins at distance `dist`, not 0, and a robot that has arrived stays at its goal.  Here the objective is a TIME under a distance
 * constraint: one row per UNORDERED pair (u, q), u < q, u owned.
 *   clock    robot r at parameter s of segment g has the clock value T_r(g, s) = ((g + s) / res) * piece_time[r] (the expression used wherever a time is
 *            formed).  The last control point (g == S - 1, s == 1.0) has the clock set [T, +inf): the robot stays there (tj_audit_timed's hover).  Every other
 *            point has the one-value set {T}.  (Waiting at the start needs no set: a start's {0} gives the same gaps, every other clock being >= 0.)
 *   slip     of two points: the distance of their clock sets, max(0, lo_u - hi_q, lo_q - hi_u).
 *   margin   of the pair: the infimum of the slip over all (x on u's path, y on q's path) with |x - y| <= dist.  0: the two are within dist at equal flight
 *            times (one passing the other's goal after its arrival included).  +inf, or no row: the paths never come within dist.
 *   item     tj_path_crossings': (tr, j, [sa, sb], [ra, rb]), dyadic windows, both nets restricted from the RAW hulls by blossoming.
 *   OUT      lo(W) of tj_path_crossings (the GJK's |v| with its certificate, 0 without one) > dist: the item holds no contact, klo(W) = +inf.
 *   klo(W)   not OUT: the distance of the windows' clock intervals, max(0, ta_u - tb_q, ta_q - tb_u), ta = T(segment, window's start), tb = T(segment,
 *            window's end), or +inf where the window ends on the last control point.  The objective is linear in the parameters: exact as the window shrinks.
 *   corners  the four end-point pairs i, k in {0, 5}: a candidate where norm3(a_i - b_k) <= dist, with the slip of the two corner points.
 *   same time   only for an item that is not OUT with klo == 0 (its clock intervals overlap): tau = fmax(fmax(ta_u, ta_q), 0.0); each robot's parameter
 *            x = (tau - T(g, 0)) / (T(g + 1, 0) - T(g, 0)) clamped into the item's own window (tj_flight_profile's expressions); its position is b_0 of the
 *            raw hull restricted to [x, x].  Within dist: a candidate with slip 0.0 -- stated, not computed -- flagged SAME_TIME.  Without it an equal-time
 *            contact is never found: dyadic parameters of two robots with different piece_time never give equal clocks.
 *   order    candidates with slip < max_slip, by the total order (slip, segment, partner_segment, s, partner_s); of a corner and a same-time candidate at the
 *            same place the corner goes first.
 *   seeds    every (tr, j) whose raw hull boxes pass tj_audit's box test at dist, full windows, evaluated like a round's children.
 *   listed   (u, q) has a row if and only if some seed has a candidate, or is not OUT with klo < max_slip.  A pair without a row is certified: no slip below
 *            max_slip brings the two within dist.
 *   round    tj_path_crossings': every live item into its four quadrants, all children evaluated, best (the smallest slip) over the whole round, and the
 *            children with klo < best.hi are kept -- strict, against the round's FINAL best.  Nothing found: hi = max_slip.
 *   bracket  lo = min(best.hi, min of klo over the live set), hi = best.hi, both in seconds.
 *   stop     hi - lo <= tol (CONVERGED) | the live set is empty (CONVERGED) | depth == max_depth | more than max_windows live (TRUNCATED: the record of the
 *            last completed round; `windows` counts the overflowing round's work too).
 *   record   lo <= the pair's margin <= hi.  `distance` (<= dist) is that of the hi sample: u's curve at `s` of `segment` from q's at `partner_s` of
 *            `partner_segment`; time = T(segment, s), partner_time = T(partner_segment, partner_s).  No sample found: segments -1, parameters, times and
 *            distance -1.0, hi == max_slip.  depth: rounds completed.  windows: seeds evaluated + 4 per split item.  Rows sorted by (robot, partner).
 * *n, cap, the count-only call and TJ_ERR_CAPACITY as in tj_path_crossings.  dist <= 0: offset.  max_slip <= 0: +infinity.  tol < 0:
 * TJ_MARGIN_TOL_FRACTION * dist / vel_limit -- the margin is resolved to the time a robot at the speed limit needs for 1 % of the contact distance, 5e-4 s at
 * the shipped parameters: a design condition, stated as such; 0 is valid.  max_depth < 0: TJ_MARGIN_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0:
 * TJ_MARGIN_FRONTIER; above TJ_MARGIN_MAX_WINDOWS TJ_ERR_INVALID.  NaN dist, max_slip or tol, n == NULL, cap < 0, rows == NULL with cap > 0, a call before
 * tj_init_state: TJ_ERR_INVALID.  Single-UAV mode: *n = 0 and TJ_OK.  A plain SHARDED context (world > 1) returns TJ_ERR_UNSUPPORTED;
 * tj_group_timing_margin computes the rows (u, q > u) on u's owner with control points and piece_time read from the owners, and is bitwise one context's.
 * DEVICE MEMORY grows only and is a function of cap and max_windows alone:
 *   cap * (2 * max_windows * 48 + 4 * max_windows * 8 + 8 + 88) bytes     (live lists, their children's klo, the slots' pairs and the rows)
 * plus the bitmask and its offsets, owned * ceil(uav_num / 32) * 8 bytes.  A call whose figure exceeds TJ_MARGIN_MAX_BYTES is refused up front with
 * TJ_ERR_INVALID.  At most THREE launches whatever the fleet's size, the number of pairs and the depth (two for a count-only call).  Changes no solver
 * state, statistics or launch count.
 * STATED LIMITS.  (1) The optimum lies ON the boundary distance == dist, and that boundary is tangent there to the objective's level line, so the live set
 * grows by about sqrt(2) per round (3 -> 43 -> 1185 items at depths 0, 9 and 19 for two perpendicular straight paths) while the bracket halves: this query
 * ends at a tolerance in time and does not run to rounding.  (2) Paths that run alongside each other at about dist grow faster and end TRUNCATED; the
 * bracket returned is still sound.  (3) tj_path_crossings' limit 1, the GJK's 1e-10 relative, applies to the OUT decision.
 * The defaults are measured (tests/timing_margin_ref.py default_tolerance, the restatement, on the CPU): default dist, max_slip = +inf, the default tol,
 * max_depth = 40, the live set capped at TJ_MARGIN_MAX_WINDOWS only, on the final states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz,
 * e2e_scn_b_coupled.npz, of e2e_scn_c3.npz with z set to 0 (_flat: the fleet meets at one place at one time) and of that with piece_time[u] *= 1 + 0.03 * u
 * (_flat_staggered):
 *   state                       listed pairs   rows with hi == 0   truncated rows   largest live set   largest depth   widest bracket
 *   e2e_scn_b                   0              0                   0                0                  0               0.00e+00
 *   e2e_scn_c3                  0              0                   0                0                  0               0.00e+00
 *   e2e_scn_b_coupled           0              0                   0                0                  0               0.00e+00
 *   e2e_scn_c3_flat             2016           2016                0                0                  0               0.00e+00
 *   e2e_scn_c3_flat_staggered   2016           1                   0                2921               12              5.00e-04
 * The stacked fleets list nothing at dist = offset: they are apart in space.  The flattened fleet meets at one place at one time: every pair is found at slip 0
 * among the seeds.  Staggered, the slips range from 0 to 10.12 s; no row truncates at TJ_MARGIN_MAX_WINDOWS at the default tolerance, and every bracket
 * closes below it by depth 12.  At tol = 1e-6 instead, 47 of 119 pairs (every 17th) truncate with brackets up to 3.9e-4 wide (limit 1): the reason the
 * default is a tolerance in time and not a rounding floor.
 * TJ_MARGIN_FRONTIER is the next power of two >= 2 x the largest live set, at least 64, capped at TJ_MARGIN_MAX_WINDOWS. */
#define TJ_MARGIN_CONTACT     1    /* a sample was found and hi <= 0: the two are within dist on the timetable */
#define TJ_MARGIN_CLEAR       2    /* lo > 0: a positive margin is certified */
#define TJ_MARGIN_CONVERGED   4    /* hi - lo <= tol, or nothing was left that could hold a smaller slip */
#define TJ_MARGIN_TRUNCATED   8    /* the pair's live set outgrew max_windows: the bracket of the last completed round is returned */
#define TJ_MARGIN_ROBOT_END   16   /* the hi sample is robot's last control point */
#define TJ_MARGIN_PARTNER_END 32   /* the same for partner */
#define TJ_MARGIN_SAME_TIME   64   /* the hi sample is a same-time candidate: slip 0.0 stated */
#define TJ_MARGIN_MAX_DEPTH 40
#define TJ_MARGIN_FRONTIER  4096
#define TJ_MARGIN_MAX_WINDOWS 4096
#define TJ_MARGIN_MAX_BYTES (1ll << 31)
#define TJ_MARGIN_TOL_FRACTION 0.01
typedef struct tj_margin_record {
  double lo, hi;                  /* lo <= the slip the pair tolerates before coming within dist <= hi, in seconds */
  double distance;                /* of the hi sample, <= dist */
  double s, partner_s;            /* local parameters of the hi sample in `segment` and `partner_segment` */
  double time, partner_time;      /* the clock values of the hi sample */
  int robot, partner, segment, partner_segment, depth, flags, windows, reserved;
} tj_margin_record;
int tj_timing_margin(tj_ctx* c, double dist, double max_slip, double tol, int max_depth, int max_windows, tj_margin_record* rows, int cap, int* n);
int tj_margin_record_size(void);   /* sizeof(tj_margin_record) */
/* ---- tj_proximity_windows: FROM WHEN TO WHEN is each pair of robots within `dist` of each other at equal flight times
 * (csrc/kernels_proximity.h; read-only like tj_pair_approach).  tj_pair_approach returns one minimum per pair, tj_timing_margin one tolerable slip,
 * tj_flight_profile samples that certify nothing between them.  Here the whole time axis of a pair is classified against the level `dist` and everything
 * that is not certified outside is returned as time intervals: at dist = offset the conflict intervals of a state that is not yet collision-free, at a
 * radio range or a downwash radius the fleet's time-varying link graph, each edge with certified on and off times.  Rows are for one DIRECTED pair (u, q),
 * u owned, q != u, over u's flight (tj_pair_approach's convention: the two directions end at different times).  Time, hover after arrival, hull formation,
 * the cuts at q's segment boundaries and arrival, the restriction of both RAW hulls and the box prefilter are tj_audit_timed's and tj_closest_approach's,
 * unchanged.  For one directed pair:
 *   window   W = [ca, cb] in one segment of u and one segment of q (or q's hover), d_0..d_5 its difference net.  lo(W): the GJK's |v| with its certificate
 *            `sep` (v . d_i > 0 for all six points), 0 without one.  h0, h5 = norm3(d_0), norm3(d_5): the separations attained at ca and cb.
 *            ub(W) = the largest norm3(d_i), i = 0..5: the curve lies in the net's hull and a norm is convex, so no separation on W is larger.
 *   class    OUT: sep and lo > dist.  IN: ub <= dist.  MIXED: everything else.  (In this order.)
 *   seeds    the level-0 windows tj_audit_timed evaluates for u against this q that pass the box prefilter at range = dist; a window the prefilter skips is OUT.
 *   listed   (u, q) is listed if and only if some seed is not OUT.  A pair that is not listed is certified farther than dist apart over u's whole flight.
 *   search   kept = the IN seeds, live = the MIXED seeds.  One round: a live window with cb - ca <= tol, or whose midpoint cm = 0.5 * (ca + cb) does not lie
 *            strictly between its ends, is appended to kept as an EDGE leaf with its h0 and h5; every other live window is halved at cm and both children are
 *            evaluated from the RAW hulls: OUT children are dropped, IN children appended to kept with h0 and h5, MIXED children form the next live set.
 *   stop     the live set is empty | depth == max_depth | the live set or the kept list after a round, or after the seeding, holds more than max_windows
 *            (TRUNCATED: kept and live are those of the last completed round -- the appends of the overflowing round do not count, `windows` counts its work
 *            too, as the siblings do).  Whatever is live at the end joins the leaves as EDGE leaves (so a pair has at most 2 * max_windows leaves).
 *   merge    the pair's leaves ordered by ca (distinct: a pair's windows are disjoint).  Two consecutive leaves are adjacent exactly when prev.cb == next.ca
 *            on doubles: the cut and midpoint expressions are shared, so the ends agree bit for bit.  A row is a maximal chain of adjacent leaves.
 *   sure     every time of an IN leaf; of an EDGE leaf ca if h0 <= dist and cb if h5 <= dist: times at which the pair IS within dist.
 *   row      t_first_lo = the chain's start, t_last_hi = its end; t_first_hi = the earliest sure time, t_last_lo = the latest (both -1.0 without one);
 *            within_lo = the sum of the IN leaves' cb - ca in time order, left to right; closest, closest_time = the smallest attained end sample of the
 *            chain in the order (value, time) -- not converged: tj_pair_approach converges it; leaves = the chain's length; depth = the rounds the pair
 *            completed; windows = the pair's work, seeds evaluated + 2 per halved window, repeated on each of the pair's rows.
 * Every field is a function of the state alone.  Outside every row's [t_first_lo, t_last_hi] the separation of the pair is certified above dist over u's
 * flight; the pair first comes within dist in [t_first_lo, t_first_hi] and is last within dist in [t_last_lo, t_last_hi].  A listed pair may end with no
 * row (every child turned OUT).  Rows are sorted by (robot, partner, t_first_lo); neither the order of evaluation nor that of any atomic append is visible.
 * CAPACITY.  *n_pairs = the listed pairs, *n = the rows; listed pairs need `cap` slots and rows `cap` entries.  n_pairs > cap: TJ_ERR_CAPACITY and
 * *n = -1 (rows are known only for pairs that were refined; nothing is written).  n_pairs <= cap < *n: TJ_ERR_CAPACITY with the exact *n, the first `cap`
 * rows in order have been written.  cap = 0 with rows == NULL is the count-only call: TJ_OK, *n_pairs, and *n = -1 unless nothing is listed (two launches).
 * dist <= 0: offset.  +infinity is valid: every pair is IN for its whole flight, one row with AT_START | AT_END.  tol < 0:
 * TJ_PROXIMITY_TOL_FRACTION * dist / vel_limit -- tj_timing_margin's design condition, stated as such: the time a robot at the speed limit needs for 1 % of
 * dist, 5e-4 s at the shipped parameters (offset in place of an infinite dist); 0 is valid.  max_depth < 0: TJ_PROXIMITY_MAX_DEPTH; above it TJ_ERR_INVALID.
 * max_windows <= 0: TJ_PROXIMITY_FRONTIER; above TJ_PROXIMITY_MAX_WINDOWS TJ_ERR_INVALID.  NaN dist or tol, n == NULL, n_pairs == NULL, cap < 0,
 * rows == NULL with cap > 0, a call before tj_init_state: TJ_ERR_INVALID, the outputs untouched.  Single-UAV mode: 0 pairs, 0 rows and TJ_OK.  A plain
 * SHARDED context (world > 1) returns TJ_ERR_UNSUPPORTED like tj_pair_approach; tj_group_proximity_windows reads every robot's control points and piece_time
 * from its owner and returns the owners' rows one after the other, bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, and is a function of cap and max_windows (S = piece_num * res segments):
 *   cap * (2 * max_windows * 48 + 2 * (2 * max_windows + 2 * S + 2) * 40 + (2 * S + 2) * 48 + 32 + 80) bytes
 *   (live lists; the kept list and the sorted leaves; the pairs' level-0 seeds; the slots' pairs, counters and totals; the rows)
 * plus the bitmask and its offsets, owned * ceil(uav_num / 32) * 8 bytes.  A call whose figure exceeds TJ_PROXIMITY_MAX_BYTES is refused up front with
 * TJ_ERR_INVALID: lower cap or max_windows.  At the defaults a pair slot costs 141 680 bytes at S = 40.
 * At most FIVE launches whatever the fleet's size, the number of pairs and the depth (two for the count-only call); no host loop over robots, pairs or
 * rounds.  Changes no solver state, statistics or launch count.
 * STATED LIMITS.  (1) A certified lo is the GJK's |v|, up to 1e-10 |v| relative above the hull's distance (the siblings' limit, unchanged): it applies to
 * the OUT decision.  (2) Separation gaps shorter than a leaf are not resolved: an EDGE leaf, and a chain across it, may hold instants at which the pair is
 * farther than dist apart.  UNCERTAIN rows are grazes at the resolution tol: the pair may or may not come within dist inside the row.
 * The defaults are measured (tests/proximity_ref.py default_tolerance, the restatement, on the CPU): the default tol, max_depth = 40, the lists capped at
 * TJ_PROXIMITY_MAX_WINDOWS only, on the final states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz, e2e_scn_b_coupled.npz, of e2e_scn_c3.npz with z set to 0
 * (_flat) and of that with piece_time[u] *= 1 + 0.03 * u (_flat_staggered), at dist = offset = 0.1 and dist = 1.0 (widest bracket: the larger of
 * t_first_hi - t_first_lo and t_last_hi - t_last_lo over the CERTAIN rows):
 *   state                       dist   listed pairs   rows   uncertain   truncated   largest live set   largest kept list   largest depth   widest bracket
 *   e2e_scn_b                   0.1    0              0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b                   1.0    38             38     0           0           2                  27                  7               4.49e-03
 *   e2e_scn_c3                  0.1    0              0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_c3                  1.0    372            372    0           0           2                  80                  7               4.49e-03
 *   e2e_scn_b_coupled           0.1    0              0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b_coupled           1.0    38             38     0           0           2                  19                  7               4.49e-03
 *   e2e_scn_c3_flat             0.1    4032           4032   0           0           2                  29                  11              2.81e-04
 *   e2e_scn_c3_flat             1.0    4032           4032   0           0           2                  80                  7               4.49e-03
 *   e2e_scn_c3_flat_staggered   0.1    2              2      0           0           2                  17                  12              3.34e-04
 *   e2e_scn_c3_flat_staggered   1.0    704            782    0           0           3                  88                  9               4.98e-03
 * A level set is crossed at isolated times, so the live set stays at two or three windows; what grows is the kept list, by the IN windows of long stays
 * within dist (up to the 2 * S + 2 seeds of a pair that flies alongside).  TJ_PROXIMITY_FRONTIER is the next power of two >= 4 x the larger of the two list
 * maxima (88), and at least 64. */
#define TJ_PROXIMITY_CERTAIN   1    /* a sure time exists: the pair IS within dist in [t_first_hi, t_last_lo]'s ends */
#define TJ_PROXIMITY_UNCERTAIN 2    /* no sure time: t_first_hi == t_last_lo == -1.0, a graze at the resolution tol */
#define TJ_PROXIMITY_AT_START  4    /* the chain starts at time 0: nothing lies before it */
#define TJ_PROXIMITY_AT_END    8    /* the chain ends at the end of robot's flight */
#define TJ_PROXIMITY_RESOLVED  16   /* CERTAIN and both brackets are at most tol wide (a side closed by AT_START / AT_END counts as resolved) */
#define TJ_PROXIMITY_TRUNCATED 32   /* the pair's live set or kept list outgrew max_windows: the leaves of the last completed round are returned */
#define TJ_PROXIMITY_MAX_DEPTH 40
#define TJ_PROXIMITY_FRONTIER  512
#define TJ_PROXIMITY_MAX_WINDOWS 4096
#define TJ_PROXIMITY_MAX_BYTES (1ll << 31)
#define TJ_PROXIMITY_TOL_FRACTION 0.01
typedef struct tj_proximity_row {
  double t_first_lo, t_first_hi;   /* the pair first comes within dist in [t_first_lo, t_first_hi] */
  double t_last_lo,  t_last_hi;    /* ... and is last within dist in [t_last_lo, t_last_hi] */
  double within_lo;                /* seconds CERTIFIED within dist inside the row (sum of the IN leaves) */
  double closest, closest_time;    /* smallest attained sample of the row and its time (not converged: tj_pair_approach converges it) */
  int robot, partner, leaves, depth, flags, windows;
} tj_proximity_row;
int tj_proximity_windows(tj_ctx* c, double dist, double tol, int max_depth, int max_windows, tj_proximity_row* rows, int cap, int* n_pairs, int* n);
int tj_proximity_row_size(void);   /* sizeof(tj_proximity_row) */
/* ---- tj_obstacle_approach: how close the FLOWN CURVE of every robot comes to an obstacle primitive, when, and to which one, converged to a tolerance the
 * caller names (csrc/kernels_obstacle_approach.h; read-only like tj_audit).  tj_audit's obs_clearance is the distance of a segment's 6-point hull: what the
 * solver constrains and the right certificate for a converged state, but only a lower bound on what the vehicle does, without a time, and on the GJK's
 * contact floor wherever a primitive lies inside a hull -- which a control net that bulges at a corner (an init file, tj_plan_init's output, a
 * state from tj_set_state) does around points the curve misses by more than `offset`.  Here the same hull bound drives tj_closest_approach's branch and
 * bound.  Works in all three modes (single-UAV included), for clouds and meshes.  For every OWNED robot u:
 *   item     (segment tr, primitive i, window [sa, sb] in [0, 1] of the segment's local parameter).  Windows are dyadic, so halving at 0.5 * (sa + sb) is
 *            exact, and with max_depth <= 40 no window is ever unsplittable: there are no terminal items.  The real time of parameter s of segment tr is
 *            ((tr + s) / res) * piece_time[u] -- log_data's sigma * piece_time; this expression is used wherever a time is formed.
 *   net      b_0..b_5 = the segment's raw hull (hull_entry's sums) restricted to [sa, sb] by blossoming (bez_restrict), always from the RAW hull, never
 *            from the parent's net: rounding does not accumulate with depth.  [0, 1] returns the raw hull bit for bit.
 *   lo(W)    |v|, v = gjk(conv{b_0..b_5}, primitive) with the hull as body 1 and the primitive as body 2 (k_audit's order), where v SEPARATES them:
 *            v . (b_i - p_j) > 0 for all six hull points and all vertices of the primitive, evaluated as (v.x * dx + v.y * dy) + v.z * dz.  Otherwise
 *            lo(W) = 0, and the item is never dropped, only halved (tj_closest_approach's certificate and its reason: the GJK's contact floor).
 *   hi(W)    the smaller of the distances of b_0 and b_5 -- points of the curve, at s = sa and s = sb -- from the primitive; b_0's on equality.  A cloud
 *            point p: norm3(b - p).  A triangle: |gjk({b}, triangle)|, a point of the Minkowski difference: an upper bound on the true distance, attained to
 *            the triangle figure of DESIGN.md 3c.  Equal values are ordered by (hi, segment, index, s), index = the caller's.
 *   seeds    for every segment the primitives tj_audit's walk returns at m = range (the same predicate: the primitive's box within `range` of the hull's box
 *            on every axis, touching counts; the 49-axis cull is not used, for 3c's reason), window [0, 1].  best = the smallest hi < range over all
 *            seeds.  The live set is {W : lo(W) < range and lo(W) < best.hi}.
 *   round d  = 1, 2, ..: every live item is halved; both children are evaluated; best is updated over all children of the round; then the live set
 *            becomes the children with lo < best.hi -- strict, against the round's FINAL best, so the set, and with it every field of the record
 *            (`windows` and `depth` included), does not depend on the order of evaluation.
 *   bracket  lo = min(best.hi, min of lo over the live set), hi = best.hi.  Sound: a dropped item had lo >= best.hi at that time, and best.hi only falls.
 *   stop     hi - lo <= tol (CONVERGED) | the live set is empty (CONVERGED) | d == max_depth | the live set after a round, or after the seeding, holds
 *            more than max_windows (TRUNCATED: the record is that of the last completed round -- for the seeds their own bracket with depth 0;
 *            `windows` counts the work of the overflowing round too).  Overflow is a property of the set's size: deterministic.
 *   lo <= min over u's flight and all primitives of dist(p_u(t), primitive) <= hi; hi is attained at `time`, against primitive `index` (the point index
 *   of tj_set_cloud / the face index of tj_set_mesh), in segment `segment`.  depth: rounds completed.  windows: items evaluated (seeds + 2 per halved item).
 *   Nothing within range, an empty obstacle set, tj_set_cloud with n = 0: index -1, segment -1, time -1.0, lo == hi == range, depth 0, CLEAR | CONVERGED.
 *   Flags against `offset`, tj_closest_approach's meanings; CLEAR is lo > offset, so a search limited to range <= offset that finds nothing certifies
 *   nothing and does not set it (tj_audit's rule for its contact flag, mirrored) -- except where there are no obstacles at all.
 * STATED LIMIT: a certified lo is the GJK's |v|, which its stop rule (|v|^2 - v . w <= 1e-10 |v|^2) leaves up to 1e-10 |v| above the hull's distance: that,
 * relative, is how far lo may stand above the minimum.  hi, time and the CONTACT flag involve no GJK for a cloud (hi is attained); for a mesh hi carries it too.
 * range <= 0: offset + 2 * margin; +infinity is valid.  tol < 0: TJ_OBSTACLE_TOL; 0 is valid.  max_depth < 0: TJ_OBSTACLE_MAX_DEPTH; above it
 * TJ_ERR_INVALID.  max_windows <= 0: TJ_OBSTACLE_FRONTIER; above it TJ_ERR_INVALID.  NaN range or tol, records == NULL, a call before tj_init_state:
 * TJ_ERR_INVALID.  A walk frontier beyond its capacity (FRONT_CAP boxes of 8 primitives near one hull): TJ_ERR_CAPACITY, never a smaller answer.  A plain
 * SHARDED context (world > 1) answers for its owned robots -- its own state is current, and nothing of another robot is read; records of other ranks'
 * robots are all zero.  tj_group_obstacle_approach assembles the owners' records: bitwise one context's.  THREE launches whatever the fleet's size, the
 * number of primitives and the depth; no host loop over rounds or robots.  Changes no solver state, statistics or launch count.
 * The defaults are measured (tests/obstacle_approach_ref.py default_tolerance, the restatement, on the CPU): tol = 0 and max_depth = 40 at the default range
 * on the final states of tests/golden/e2e_scn_a.npz, e2e_scn_b.npz, e2e_scn_c3.npz and e2e_scn_b_coupled.npz with their scenes' clouds; per depth the largest
 * hi - lo over the robots with a primitive in range:
 *   depth   0        1        2        3        4        5        6        7        8        9        10       11       12       13       14       15       16       17       18       19
 *   width   1.35e-2  8.51e-3  4.92e-3  9.91e-4  5.96e-4  1.90e-4  3.33e-5  1.20e-5  2.65e-6  1.96e-7  1.96e-7  2.14e-8  6.27e-9  2.35e-9  5.59e-10 1.40e-10 4.77e-11 8.14e-12 3.71e-13 0
 * The width shrinks all the way: at depth 19 every live set has emptied (hi == lo), so the floor is the last positive width, 3.71e-13 at depth 18, and
 * TJ_OBSTACLE_TOL is the smallest power of ten >= 10 x that.  The largest live set any robot of these runs holds at any depth is 9 items;
 * TJ_OBSTACLE_FRONTIER is the next power of two >= 4 x that (real clouds are denser than the fixtures'), and at least 4096. */
#define TJ_OBSTACLE_CONTACT   1   /* a primitive was found and hi <= offset: the curve IS within offset of primitive `index` at `time` */
#define TJ_OBSTACLE_CLEAR     2   /* lo > offset: clearance of the flown curve certified */
#define TJ_OBSTACLE_CONVERGED 4   /* hi - lo <= tol, or nothing was left that could hold a smaller distance */
#define TJ_OBSTACLE_TRUNCATED 8   /* the live set outgrew max_windows: the bracket of the last completed round is returned */
#define TJ_OBSTACLE_MAX_DEPTH 40
#define TJ_OBSTACLE_FRONTIER  4096   /* measured maximum of the live set: 9 */
#define TJ_OBSTACLE_TOL 1e-11
typedef struct tj_obstacle_robot {
  double lo, hi, time;     /* lo <= min over u's flight and all primitives of dist(p_u(t), primitive) <= hi; hi is attained at `time` */
  int index, segment;      /* the primitive (caller's index) and u's segment of the hi sample; -1, -1 (time -1.0, lo == hi == range) when nothing is within range */
  int depth, flags;        /* rounds of halving completed */
  int windows, reserved;   /* items evaluated for this robot (seeds + 2 per halved item): the work done */
} tj_obstacle_robot;
int tj_obstacle_approach(tj_ctx* c, double range, double tol, int max_depth, int max_windows, tj_obstacle_robot* records);
int tj_obstacle_record_size(void);   /* sizeof(tj_obstacle_robot) */
/* ---- tj_obstacle_windows: FROM WHEN TO WHEN is the flown curve of every robot within `dist` of the obstacle set, as certified time intervals
 * (csrc/kernels_obstacle_windows.h; read-only like tj_obstacle_approach).  tj_audit gives a hull clearance without a time, tj_obstacle_approach one converged
 * minimum per robot (one time, one primitive), tj_flight_profile samples that certify nothing between them.  A state that is not yet collision-free -- an init
 * file, tj_plan_init's output, a state from tj_set_state, a run stopped early -- is in conflict with the obstacles over intervals, often several per robot: at
 * dist = offset these are the stretches of each flight to re-plan, at a sensor or safety radius the certified stretches in which the vehicle flies near
 * structure.  The obstacle-side counterpart of tj_proximity_windows: the union of ALL primitives is classified against the level `dist`.  Works in all three
 * modes (single-UAV included), for clouds and meshes.  For every OWNED robot u:
 *   window   W = (segment tr, [sa, sb] in [0, 1] of the segment's local parameter), dyadic (halving at 0.5 * (sa + sb) is exact; with max_depth <= 40 no window
 *            is ever unsplittable).  The real time of parameter s of segment tr is ((tr + s) / res) * piece_time[u] -- tj_obstacle_approach's expression, used
 *            wherever a time is formed.  The position on the flight g = tr + s is exact in a double (9 + 40 bits).
 *   net      b_0..b_5 = the segment's RAW hull restricted to [sa, sb] (bez_restrict), never a parent's net; [0, 1] returns the raw hull bit for bit.
 *   C(W)     the candidates: the primitives whose box is within dist of the box of the net on every axis, touching counts (the walk's leaf predicate in
 *            fp64; the 49-axis cull is not used).  A primitive within dist of any point of the curve on W is in C(W), so a primitive
 *            outside it is farther than dist from the curve on W.
 *   per p    of C(W): lo_p = the GJK's |v| (hull = body 1, primitive = body 2) where v separates the two (tj_obstacle_approach's certificate), 0 without it;
 *            ub_p = the largest distance of b_0..b_5 from p (the curve lies in the net's hull and the distance to a convex primitive is convex, so the
 *            distance to p on W is never larger); h0_p, h5_p = the distances of b_0 and b_5 from p, attained at sa and sb.  A point's distance from a cloud
 *            point is norm3(b - p), from a triangle |gjk({b}, triangle)| (tj_obstacle_approach's hi: an upper bound of the distance, so ub_p stays one).
 *   class    OUT: every candidate has lo_p > dist (an empty C(W) is OUT).  Else IN: some candidate has ub_p <= dist.  Else MIXED.
 *   h0, h5   of W: the smallest h0_p (h5_p) over C(W) with its primitive, ordered by (value, caller's index); +infinity and -1 for an empty set.  h0 <= dist
 *            if and only if some primitive of the whole set is within dist of the curve at sa; then h0 is the nearest primitive's distance.
 *   search   per (robot, segment), independent of every other segment.  Seed: the window [0, 1]; OUT: the segment contributes nothing, IN: it is a leaf,
 *            MIXED: it is the live set.  Round d = 1, 2, ..: the live windows in ascending sa; one whose time width ((sb - sa) / res) * piece_time[u] <= tol
 *            becomes an EDGE leaf with its h0 and h5; every other is halved and both children are evaluated, left then right: OUT children are dropped, IN
 *            children appended to the leaves with h0 and h5, MIXED children form the next live set.
 *   stop     the live set is empty | d == max_depth | the live set or the leaf list after a round holds more than max_windows (TRUNCATED: the lists are
 *            those of the last completed round, `windows` counts the overflowing round's work too).  Whatever is live at the end joins the leaves as EDGE
 *            leaves (so a segment has at most 2 * max_windows leaves).
 *   merge    per robot the leaves of its segments in (segment, sa) order: distinct and disjoint.  Two consecutive leaves are adjacent exactly when
 *            prev.tr + prev.sb == next.tr + next.sa on doubles (a chain crosses a segment boundary).  A row is a maximal chain of adjacent leaves.
 *   sure     every time of an IN leaf; of an EDGE leaf sa if h0 <= dist and sb if h5 <= dist: times at which the curve IS within dist of a primitive.
 *   row      t_first_lo = the chain's start, t_last_hi = its end; t_first_hi = the earliest sure time, t_last_lo = the latest (both -1.0 without one);
 *            within_lo = the sum of the IN leaves' time widths ((sb - sa) / res) * piece_time[u], left to right; closest, closest_time, index = the
 *            smallest attained end sample (h0 at sa, h5 at sb) of the chain in the order (value, time, index), index = the caller's index of its primitive
 *            (-1, closest = +infinity, closest_time = -1.0 where no end sample has a candidate) -- not converged: tj_obstacle_approach converges it;
 *            segment_first, segment_last = the segments of the chain's ends; leaves = the chain's length; depth = the most rounds completed by any segment
 *            with a leaf in the chain; windows = the ROBOT's work, seeds evaluated + 2 per halved window over all its segments, repeated on each of its rows.
 *   flags    CERTAIN (a sure time exists) or UNCERTAIN, AT_START (the chain starts at g == 0), AT_END (it ends at g == S), RESOLVED (CERTAIN, and
 *            t_first_hi - t_first_lo <= tol or AT_START, and t_last_hi - t_last_lo <= tol or AT_END), TRUNCATED (a segment of the chain was truncated).
 * Every field is a function of the state alone.  Outside every row of robot u the flown curve is certified farther than dist from every primitive.  Rows are
 * sorted by (robot, t_first_lo); no order of evaluation or of any append is visible.
 * dist <= 0: offset; +infinity is valid (every primitive is a candidate of every window: for small sets, tj_audit's remark).  tol < 0:
 * TJ_OBSWIN_TOL_FRACTION * dist / vel_limit -- tj_proximity_windows' design condition, stated as such: the time a robot at the speed limit needs for 1 % of
 * dist (offset in place of an infinite dist); 0 is valid.  max_depth < 0: TJ_OBSWIN_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0:
 * TJ_OBSWIN_FRONTIER; above TJ_OBSWIN_MAX_WINDOWS (it bounds the in-kernel rank sort) TJ_ERR_INVALID.  *n = the rows.  *n > cap: TJ_ERR_CAPACITY with the
 * exact *n, the first `cap` rows in order have been written.  cap == 0 with rows == NULL is the count-only call (two launches).  n == NULL, cap < 0, rows ==
 * NULL with cap > 0, NaN dist or tol, a call before tj_init_state: TJ_ERR_INVALID, the outputs untouched (precedence: null, NaN, limits, no state).  No
 * obstacles (tj_set_cloud with n = 0 included): 0 rows and TJ_OK.  A walk frontier beyond its capacity (more than FRONT_CAP boxes of 8 primitives within dist of one
 * window's box: lower dist): TJ_ERR_CAPACITY, never fewer rows; no count is known then, *n is left UNTOUCHED and nothing is written -- that, *n <= cap or unchanged,
 * tells it from the rows' TJ_ERR_CAPACITY, which always comes with *n > cap; tj_last_error names the cause.  A plain SHARDED
 * context (world > 1) answers for its owned robots, as tj_obstacle_approach does: nothing of another robot is read.  tj_group_obstacle_windows returns the
 * owners' rows one after the other, bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, and is a function of owned x S x max_windows (S = piece_num * res segments):
 *   owned * S * (4 * max_windows * 48 + 16) + owned * 8 + cap * 88 bytes
 *   (per segment the two live lists, which hold the sorted leaves afterwards, and 2 * max_windows leaves, 48 bytes a window; its four counters; the robots'
 *   row counts and work; the rows).  A call whose figure exceeds TJ_OBSWIN_MAX_BYTES is refused up front with TJ_ERR_INVALID: lower max_windows or cap.
 * At most THREE launches whatever the fleet's size, the number of primitives and the depth (two for the count-only call); no host loop over robots,
 * segments or rounds.  Changes no solver state, statistics or launch count.
 * STATED LIMITS.  (1) A certified lo_p is the GJK's |v|, up to 1e-10 |v| relative above the hull's distance (the siblings' limit): it applies to the OUT
 * decision.  (2) IN needs ONE primitive that covers the whole window; a window covered only by several primitives together is halved until one does, or ends
 * as an EDGE leaf.  (3) Gaps shorter than a leaf are not resolved; UNCERTAIN rows are grazes at the resolution tol.
 * The defaults are measured (tests/obstacle_windows_ref.py default_tolerance, the restatement, on the CPU): the default tol, max_depth = 40, the lists capped
 * at TJ_OBSWIN_MAX_WINDOWS only, on the final states of tests/golden/e2e_scn_a.npz, e2e_scn_b.npz, e2e_scn_c3.npz, e2e_scn_b_coupled.npz and on the same
 * runs' iteration-0 states (_init), with their scenes' clouds cropped as obstacle_approach_ref.default_tolerance crops them, at dist = offset = 0.1 and
 * dist = offset + 2 * margin (widest bracket: the larger of t_first_hi - t_first_lo and t_last_hi - t_last_lo over the CERTAIN rows):
 *   state                    dist   rows   uncertain   truncated   largest live set   largest leaf list   largest depth   widest bracket
 *   e2e_scn_a                0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_a                0.3    2      0           0           1                  6                   8               7.63e-04
 *   e2e_scn_a_init           0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_a_init           0.3    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b                0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b                0.3    48     0           0           3                  17                  9               1.12e-03
 *   e2e_scn_b_init           0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b_init           0.3    52     0           0           4                  25                  12              1.22e-03
 *   e2e_scn_c3               0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_c3               0.3    19     0           0           4                  16                  9               1.12e-03
 *   e2e_scn_c3_init          0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_c3_init          0.3    7      0           0           2                  13                  12              1.22e-03
 *   e2e_scn_b_coupled        0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b_coupled        0.3    47     0           0           3                  16                  9               1.12e-03
 *   e2e_scn_b_coupled_init   0.1    0      0           0           0                  0                   0               0.00e+00
 *   e2e_scn_b_coupled_init   0.3    52     0           0           4                  25                  12              1.22e-03
 * A level set is crossed at isolated times, so the live set of a segment stays at a few windows; what grows is its leaf list, by the IN windows of a
 * stay within dist that is resolved to tol at both ends.  The iteration-0 states of these scenes are clear of their clouds at offset, as their end states are.
 * TJ_OBSWIN_FRONTIER is the next power of two >= 4 x the larger of the two list maxima (25), and at least 64. */
#define TJ_OBSWIN_CERTAIN   1    /* a sure time exists: the curve IS within dist of a primitive at t_first_hi and at t_last_lo */
#define TJ_OBSWIN_UNCERTAIN 2    /* no sure time: t_first_hi == t_last_lo == -1.0, a graze at the resolution tol */
#define TJ_OBSWIN_AT_START  4    /* the chain starts at time 0: nothing lies before it */
#define TJ_OBSWIN_AT_END    8    /* the chain ends at the end of the robot's flight */
#define TJ_OBSWIN_RESOLVED  16   /* CERTAIN and both brackets are at most tol wide (a side closed by AT_START / AT_END counts as resolved) */
#define TJ_OBSWIN_TRUNCATED 32   /* a segment of the chain outgrew max_windows: its leaves of the last completed round are returned */
#define TJ_OBSWIN_MAX_DEPTH 40
#define TJ_OBSWIN_FRONTIER  128
#define TJ_OBSWIN_MAX_WINDOWS 1024
#define TJ_OBSWIN_MAX_BYTES (1ll << 31)
#define TJ_OBSWIN_TOL_FRACTION 0.01
typedef struct tj_obswin_row {
  double t_first_lo, t_first_hi;   /* the curve first comes within dist of the obstacles in [t_first_lo, t_first_hi] */
  double t_last_lo,  t_last_hi;    /* ... and is last within dist in [t_last_lo, t_last_hi] */
  double within_lo;                /* seconds CERTIFIED within dist inside the row (sum of the IN leaves) */
  double closest, closest_time;    /* smallest attained end sample of the row and its time (not converged: tj_obstacle_approach converges it) */
  int robot, index;                /* index: the primitive of `closest` (caller's index), -1 without one */
  int segment_first, segment_last; /* the segments of the chain's ends */
  int leaves, depth, flags, windows;
} tj_obswin_row;
int tj_obstacle_windows(tj_ctx* c, double dist, double tol, int max_depth, int max_windows, tj_obswin_row* rows, int cap, int* n);
int tj_obswin_row_size(void);   /* sizeof(tj_obswin_row) */
/* ---- tj_sight_windows: FROM WHEN TO WHEN does the straight line between two robots at equal flight times, or between a robot and a fixed station, pass within
 * `dist` of the obstacle set, as certified time intervals (csrc/kernels_sight_windows.h; read-only like tj_obstacle_windows).  The robot-robot queries look at
 * no obstacle and the obstacle queries at one robot; a planner that assigns radio or optical links, relays or tethers asks about the LINK: during which intervals
 * is the segment between the two ends blocked, or closer to structure than a Fresnel or tether clearance?  tj_flight_profile's samples certify nothing between
 * them, and a thin pillar crosses a link in milliseconds.  Works in all three modes (single-UAV: station links only), for clouds and meshes.
 * links [n_links][2]: link k = (a, b); a is a robot, b a robot other than a, or -1 - s for station s of stations [n_stations][3].  A link is directed: it is
 * looked at over a's flight, time 0 to (S / res) * piece_time[a] (tj_proximity_windows' convention: the two ends arrive at different times).  A partner that
 * has arrived hovers at its last control point; a station is six copies of its point and has no cuts.  Duplicate links are allowed and answered per index.
 * For every link k = (a, b) with a OWNED, and every segment tr of a:
 *   seeds    the segment's window of time [(tr / res) * pt_a, ((tr + 1) / res) * pt_a] cut at b's segment boundaries (j / res) * pt_b and at b's arrival
 *            (tj_audit_timed's cuts at level 0, the same expressions: adjacent windows share an end bit for bit).  A station: the one window.
 *   window   W = [ca, cb] lies in segment tr of a and in ONE segment j of b (j == S: b hovers).  a_0..a_5 = a's RAW hull of tr restricted to
 *            [sa, sb] = clamp01((ca - T0) / (T1 - T0)), .. and b_0..b_5 = b's raw hull of j restricted likewise to [ra, rb] (tj_proximity_windows' expressions,
 *            never a parent's net; a hover body and a station are not restricted).  L(W) = {a_0..a_5, b_0..b_5}: at every time of W the link joins a point of
 *            conv{a_i} to a point of conv{b_i}, so it lies in conv L(W).
 *   C(W)     the candidates: the primitives whose box is within dist of the box of the 12 points on every axis, touching counts (the walk's leaf predicate in
 *            fp64; the 49-axis cull is not used).  A primitive outside C(W) is farther than dist from the link on all of W.
 *   lo_p     |v|, v = gjk(L(W), p) (the 12 points = body 1), where v separates the two over all 12 points (tj_obstacle_approach's certificate); 0 without it.
 *   sample   (x, y, p), the attained distance of ONE point of the link with ends x, y from p: e = y - x; proj(z) = 0 if e.e == 0, else
 *            clamp01(((z - x) . e) / (e . e)).  A cloud point: lambda = proj(p).  A triangle: lambda = 0.5, then TJ_SIGHT_PROJECTIONS times z = x + lambda e,
 *            w = z - gjk({z}, triangle) (the GJK's witness on the triangle), lambda = proj(w).  Value: the distance of x + lambda e from p (norm3 for a cloud
 *            point, |gjk({.}, triangle)| for a triangle: tj_obstacle_approach's hi).  Any lambda in [0, 1] is a point of the link, so the value is an upper
 *            bound of the link's distance (exact for a cloud point); the projections only decide how soon a window is decided.
 *   h0_p, h5_p  = sample(a_0, b_0, p) with its lambda0_p: attained at ca; sample(a_5, b_5, p) with lambda5_p: attained at cb.
 *   ub_p     for lambda of {lambda0_p, lambda5_p}: the largest distance of a_i + lambda (b_i - a_i), i = 0..5, from p.  Both nets are over the same window of
 *            time, so these six points are the Bezier net of the point that rides the link at the FIXED lambda; the distance to a convex primitive is convex, so
 *            that point, and with it the link, is within this value of p on all of W.  ub_p is the smaller of the two; the term i = 0 at lambda0_p is h0_p
 *            itself (i = 5 at lambda5_p: h5_p), so a lambda whose sample is above dist cannot bring ub_p to dist and is not looked at.
 *   class    OUT: every candidate has lo_p > dist (an empty C(W) is OUT).  Else IN: some candidate has ub_p <= dist.  Else MIXED.
 *   h0, h5   of W: the smallest h0_p (h5_p) over C(W) with its primitive, ordered by (value, caller's index).
 *   search   per (link, segment of a), independent of every other.  The seeds in time order: IN seeds are leaves, MIXED seeds the live set.  Round d = 1, 2, ..:
 *            the live windows in ascending ca; one with cb - ca <= tol, or whose midpoint 0.5 * (ca + cb) is not strictly inside, becomes an EDGE leaf with its
 *            h0 and h5; every other is halved there and both children are evaluated from the raw hulls, left then right: OUT children are dropped, IN children
 *            appended to the leaves, MIXED children form the next live set.
 *   stop     the live set is empty | d == max_depth | the live set or the leaf list after a round holds more than max_windows (TRUNCATED: the lists are those
 *            of the last completed round, `windows` counts the overflowing round's work too).  More than max_windows MIXED or IN seeds: TRUNCATED at depth 0.
 *            Whatever is live at the end joins the leaves as EDGE leaves (a segment has at most max(2 * max_windows, S + 1) leaves).
 *   merge    per link the leaves of a's segments in ca order: distinct and disjoint.  Two consecutive leaves are adjacent exactly when prev.cb == next.ca on
 *            doubles (the segment ends and the cuts share their expressions, so a chain crosses segment boundaries).  A row is a maximal chain.
 *   sure     every time of an IN leaf; of an EDGE leaf ca if h0 <= dist and cb if h5 <= dist: times at which the link IS within dist of a primitive.
 *   row      t_first_lo = the chain's start, t_last_hi = its end; t_first_hi = the earliest sure time, t_last_lo = the latest (both -1.0 without one);
 *            within_lo = the sum of the IN leaves' cb - ca, left to right; closest, closest_time, index = the smallest attained end sample of the chain in the
 *            order (value, time, index), index = the caller's index of its primitive (-1, closest = +infinity, closest_time = -1.0 where no end sample has a
 *            candidate) -- not converged; link = k, robot = a, partner = b as given; leaves = the chain's length; depth = the most rounds completed by any
 *            segment with a leaf in the chain; windows = the LINK's work, seeds + 2 per halved window over all segments of a, repeated on each of its rows.
 *   flags    CERTAIN (a sure time exists) or UNCERTAIN, AT_START (t_first_lo == 0), AT_END (t_last_hi == (S / res) * pt_a), RESOLVED (CERTAIN, and
 *            t_first_hi - t_first_lo <= tol or AT_START, and t_last_hi - t_last_lo <= tol or AT_END), TRUNCATED (a segment of the chain was truncated).
 * Every field is a function of the state and the arguments alone.  Outside every row of link k the link is certified farther than dist from every primitive
 * over a's flight.  Rows are sorted by (link, t_first_lo); no order of evaluation or of any append is visible.
 * dist <= 0: offset; +infinity is valid.  tol < 0: TJ_SIGHT_TOL_FRACTION * dist / vel_limit -- every point of a link moves at most at the speed limit of its
 * ends, so the siblings' design condition carries over: the time such a point needs for 1 % of dist (offset in place of an infinite dist); 0 is valid.
 * max_depth < 0: TJ_SIGHT_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0: TJ_SIGHT_FRONTIER; above TJ_SIGHT_MAX_WINDOWS (it bounds the in-kernel rank
 * sort) TJ_ERR_INVALID.  *n = the rows.  *n > cap: TJ_ERR_CAPACITY with the exact *n, the first `cap` rows in order have been written.  cap == 0 with rows ==
 * NULL is the count-only call (two launches).  TJ_ERR_INVALID with the outputs untouched (precedence: null, NaN, limits, no state): n == NULL, cap < 0, rows ==
 * NULL with cap > 0, n_links < 0, links == NULL with n_links > 0, n_stations < 0, stations == NULL with n_stations > 0; a NaN dist, tol or station coordinate; a
 * link whose a is no robot, whose b == a or whose b is neither a robot nor a station; a call before tj_init_state.  n_links == 0 or no obstacles (tj_set_cloud
 * with n = 0 included): 0 rows and TJ_OK.  A walk frontier beyond its capacity (more than FRONT_CAP boxes of 8 primitives within dist of one window's box: lower
 * dist): TJ_ERR_CAPACITY, never fewer rows; no count is known then, *n is left UNTOUCHED and nothing is written; tj_last_error names the cause.  A plain SHARDED
 * context (world > 1) holds neither the other ranks' piece_time nor their current nets: TJ_ERR_UNSUPPORTED, tj_last_error names tj_group_sight_windows, which
 * answers each link on the rank that owns a with nets and piece_time from the owners, in (link, t_first_lo) order, bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, and is a function of n_links x S x max_windows (S = piece_num * res segments):
 *   n_links * S * (2 * (2 * max_windows + S + 1) * 48 + 16) + n_links * 16 + n_stations * 24 + cap * 88 bytes
 *   (per link and segment the live lists, which hold the seeds before and the sorted leaves afterwards, and the leaf list, 48 bytes a window, each with room for
 *   a segment whose S + 1 seeds are all there is; its four counters; the links with their row counts and work; the stations; the rows).  A call whose figure
 *   exceeds TJ_SIGHT_MAX_BYTES is refused up front with TJ_ERR_INVALID: lower max_windows, cap or the number of links.
 * At most THREE launches whatever the number of links, the number of primitives and the depth (two for the count-only call); no host loop over links,
 * segments or rounds.  Changes no solver state, statistics or launch count.
 * STATED LIMITS.  (1) A certified lo_p is the GJK's |v|, up to 1e-10 |v| relative above the hull's distance (the siblings' limit): it applies to the OUT
 * decision.  (2) conv L(W) holds more than the link's sweep (a link between distant ends has a long box: every primitive near it is a candidate of every
 * window), and IN needs ONE primitive and ONE fixed lambda that cover the whole window; anything else is halved until one does, or ends as an EDGE leaf.
 * (3) For a triangle the sample is an upper bound reached by TJ_SIGHT_PROJECTIONS alternating projections, not the link's distance.  (4) Gaps shorter than a
 * leaf are not resolved; UNCERTAIN rows are grazes at the resolution tol.
 * The defaults are measured (tests/sight_windows_ref.py default_tolerance, the restatement, on the CPU; nothing here is timed): the default tol, max_depth = 40,
 * the lists capped at TJ_SIGHT_MAX_WINDOWS only, on the final states of tests/golden/e2e_scn_b.npz, e2e_scn_c3.npz, e2e_scn_b_coupled.npz and on the same runs'
 * iteration-0 states (_init), with their scenes' clouds cropped as obstacle_approach_ref.default_tolerance crops them; the links (u, (u + 1) % U) and
 * (u, U - 1 - u) for every u and every robot to one station at the cropped cloud's centroid, 1.0 above its top; dist = offset = 0.1 and offset + 2 * margin
 * (widest bracket: the larger of t_first_hi - t_first_lo and t_last_hi - t_last_lo over the CERTAIN rows):
 *   state                    dist   rows   uncertain   truncated   largest live set   largest leaf list   largest depth   widest bracket
 *   e2e_scn_b                0.1    90     0           0           6                  20                  11              2.81e-04
 *   e2e_scn_b                0.3    72     0           0           4                  17                  9               1.12e-03
 *   e2e_scn_b_init           0.1    98     0           0           8                  25                  14              3.05e-04
 *   e2e_scn_b_init           0.3    80     0           0           4                  27                  12              1.22e-03
 *   e2e_scn_c3               0.1    126    0           0           4                  20                  11              2.81e-04
 *   e2e_scn_c3               0.3    85     0           0           4                  17                  9               1.12e-03
 *   e2e_scn_c3_init          0.1    125    0           0           4                  20                  14              3.05e-04
 *   e2e_scn_c3_init          0.3    73     0           0           2                  13                  12              1.22e-03
 *   e2e_scn_b_coupled        0.1    89     0           0           6                  21                  11              2.81e-04
 *   e2e_scn_b_coupled        0.3    72     0           0           4                  17                  9               1.12e-03
 *   e2e_scn_b_coupled_init   0.1    98     0           0           8                  25                  14              3.05e-04
 *   e2e_scn_b_coupled_init   0.3    80     0           0           4                  27                  12              1.22e-03
 * The same clouds with every point a triangle (the point and two vertices 0.02 along x and along y), per number of projections K: rows / UNCERTAIN rows /
 * largest leaf list:
 *   state                    dist   K = 1        K = 2        K = 3        K = 4        K = 5        K = 6
 *   e2e_scn_b                0.1    81/0/126     81/0/32      81/0/19      81/0/19      81/0/19      81/0/19
 *   e2e_scn_b                0.3    66/0/22      66/0/20      66/0/20      66/0/20      66/0/20      66/0/20
 *   e2e_scn_b_init           0.1    85/4/570     84/0/197     84/0/25      84/0/25      84/0/25      84/0/25
 *   e2e_scn_b_init           0.3    68/1/92      68/0/25      68/0/25      68/0/25      68/0/25      68/0/25
 *   e2e_scn_c3               0.1    90/0/49      90/0/15      90/0/15      90/0/15      90/0/15      90/0/15
 *   e2e_scn_c3               0.3    80/0/16      80/0/16      80/0/16      80/0/16      80/0/16      80/0/16
 *   e2e_scn_c3_init          0.1    90/0/253     90/0/20      90/0/20      90/0/20      90/0/20      90/0/20
 *   e2e_scn_c3_init          0.3    71/0/14      71/0/14      71/0/14      71/0/14      71/0/14      71/0/14
 *   e2e_scn_b_coupled        0.1    83/0/127     83/0/33      83/0/21      83/0/21      83/0/21      83/0/21
 *   e2e_scn_b_coupled        0.3    67/0/22      67/0/20      67/0/20      67/0/20      67/0/20      67/0/20
 *   e2e_scn_b_coupled_init   0.1    85/4/570     84/0/197     84/0/25      84/0/25      84/0/25      84/0/25
 *   e2e_scn_b_coupled_init   0.3    68/1/92      68/0/25      68/0/25      68/0/25      68/0/25      68/0/25
 * (K = 7 and 8, measured too, repeat K = 6.)  With one projection the iteration-0 states of e2e_scn_b even end TRUNCATED at TJ_SIGHT_MAX_WINDOWS: a sample far from
 * the link's nearest point leaves whole stretches undecided.  TJ_SIGHT_PROJECTIONS is the smallest K at which no state's triple differs from that of K + 1 and of K + 2 (3).  TJ_SIGHT_FRONTIER is the next power of two >= 4 x
 * the larger of the two list maxima over the cloud states and the triangulated states at TJ_SIGHT_PROJECTIONS (27), and at least 64. */
#define TJ_SIGHT_CERTAIN   1    /* a sure time exists: the link IS within dist of a primitive at t_first_hi and at t_last_lo */
#define TJ_SIGHT_UNCERTAIN 2    /* no sure time: t_first_hi == t_last_lo == -1.0, a graze at the resolution tol */
#define TJ_SIGHT_AT_START  4    /* the chain starts at time 0: nothing lies before it */
#define TJ_SIGHT_AT_END    8    /* the chain ends at the end of robot a's flight */
#define TJ_SIGHT_RESOLVED  16   /* CERTAIN and both brackets are at most tol wide (a side closed by AT_START / AT_END counts as resolved) */
#define TJ_SIGHT_TRUNCATED 32   /* a segment of the chain outgrew max_windows: its leaves of the last completed round are returned */
#define TJ_SIGHT_MAX_DEPTH 40
#define TJ_SIGHT_FRONTIER  128
#define TJ_SIGHT_MAX_WINDOWS 1024
#define TJ_SIGHT_MAX_BYTES (1ll << 31)
#define TJ_SIGHT_TOL_FRACTION 0.01
#define TJ_SIGHT_PROJECTIONS 3
typedef struct tj_sight_row {
  double t_first_lo, t_first_hi;   /* the link first comes within dist of the obstacles in [t_first_lo, t_first_hi] */
  double t_last_lo,  t_last_hi;    /* ... and is last within dist in [t_last_lo, t_last_hi] */
  double within_lo;                /* seconds CERTIFIED within dist inside the row (sum of the IN leaves) */
  double closest, closest_time;    /* smallest attained end sample of the row and its time (not converged) */
  int link, robot, partner;        /* the caller's index of the link, its robot a and its b as given (a robot, or -1 - station) */
  int index;                       /* the primitive of `closest` (caller's index), -1 without one */
  int leaves, depth, flags, windows;
} tj_sight_row;
int tj_sight_windows(tj_ctx* c, const int* links, int n_links, const double* stations, int n_stations, double dist, double tol, int max_depth, int max_windows,
                     tj_sight_row* rows, int cap, int* n);
int tj_sight_row_size(void);   /* sizeof(tj_sight_row) */
/* ---- tj_peak_dynamics: how fast every robot's FLOWN CURVE really gets -- peak speed, acceleration and jerk, converged, each with its flight time -- how long
 * its path is, and by how much its timetable could be compressed (csrc/kernels_peak_dynamics.h; read-only like tj_audit).  tj_audit's speed / accel are maxima
 * over the control vectors of each segment's derivative nets: what bound_energy constrains, but only an upper bound on what the vehicle does, without a time --
 * TJ_AUDIT_SPEED can be set for a curve that never reaches the limit (an init file, tj_plan_init's output).  Here that bound drives a maximising branch and
 * bound over windows of one segment's parameter.  Nothing of another robot is read: all three modes, single-UAV included.  For every OWNED robot u:
 *   nets     P[0..5] = the raw hull of segment tr (hull_entry's sums); per axis v_i = 5 * (P[i+1] - P[i]), i = 0..4 (degree 4), a_i = 20 * (P[i+2] - 2 * P[i+1]
 *            + P[i]), i = 0..3 (degree 3) -- hull_speed's and hull_accel's expressions -- and j_i = 60 * (P[i+3] - 3 * P[i+2] + 3 * P[i+1] - P[i]), i = 0..2
 *            (degree 2), all left to right.  A control vector c of a net counts as norm3(c) / den with den = w * pt (speed), w * w * pt * pt (acceleration),
 *            w * w * w * pt * pt * pt (jerk), left to right, w = the segment's weight, pt = piece_time[u]: tj_audit's association, so depth 0 gives its bits.
 *   window   W = [sa, sb], dyadic in the segment's local parameter (as in tj_obstacle_approach: halving at 0.5 * (sa + sb) is exact, max_depth <= 40).  The
 *            derivative net ITSELF is restricted to W by blossoming (bez_restrict_n: bez_restrict's steps for degree 4, 3, 2), always from the RAW derivative
 *            net, never from a parent's and never by differencing a restricted position net: rounding does not grow with depth and no window-width factor
 *            appears.  [0, 1] returns the raw net bit for bit.
 *   bounds   for the restricted net c_0..c_n: ub(W) = max_i norm3(c_i) / den (the curve lies in the hull of its net); at(W) = the larger of norm3(c_0) / den
 *            and norm3(c_n) / den -- values of the curve at s = sa and s = sb: attained; c_0's on equality.  Attained candidates are ordered: larger value,
 *            then smaller segment, then smaller s.  The real time of (tr, s) is ((tr + s) / res) * piece_time[u], tj_obstacle_approach's expression.
 *   search   one per robot and quantity.  Seeds: every segment at [0, 1]; best = the first attained candidate in that order; live = {W : ub(W) > best.value},
 *            strict.  Round d = 1, 2, ..: every live item is halved, both children are evaluated, best is updated over the round's children, then live = the
 *            children with ub > best.value -- the round's FINAL best, so nothing (`windows` and `depth` included) depends on the order of evaluation.
 *   bracket  lo = best.value, hi = max(best.value, max of ub over the live set): lo <= the curve's peak <= hi, lo attained at `time` in `segment`.
 *   stop     hi - lo <= tol * hi (relative: the three quantities have different units; CONVERGED) | the live set is empty (CONVERGED) | d == max_depth |
 *            the live set holds more than max_windows (TRUNCATED: the record of the last completed round -- for an overflow at seeding the seeds' own bracket
 *            with depth 0; `windows` counts the overflowing round's work too).
 *   length   real time cancels.  Level L (0 <= L <= TJ_PEAK_MAX_LENGTH_LEVELS): per segment the 2^L windows [j * h, (j + 1) * h], h = 1.0 / 2^L, each the raw v
 *            net restricted: len_lo(W) = h * norm3(m), m = (c_0 + c_1 + c_2 + c_3 + c_4) / 5 per axis -- the chord: the integral of a Bezier net is its mean --
 *            and len_hi(W) = (h * (norm3(c_0) + norm3(c_1) + norm3(c_2) + norm3(c_3) + norm3(c_4))) / 5 -- the control polygon; sums left to right.  A
 *            segment's windows are summed in the balanced binary tree over adjacent pairs, the segments one after the other, tr = 0..S-1.
 *            length_lo <= path length <= length_hi.
 *   duration = tj_audit's: piece_num * piece_time as its sum.  time_scale = fmax(speed.hi / vel_limit, sqrt(accel.hi / acc_limit)): multiplying the robot's
 *   piece_time by any factor >= time_scale keeps both peaks certified at or below their limits; a value < 1 is headroom.
 * STATED LIMIT: hi is sound up to the rounding of at most eight convex-combination steps ((1 - s) * x + s * y: relative 3 eps of the larger operand each),
 * norm3 and the division: hi >= true peak - 32 eps * (the robot's depth-0 hi of that quantity), eps = 2^-53.  The CPU test measures the excess on the four end
 * states and tiny()'s initial states against mpmath: at most 1.72e-16 = 1.5 eps of the depth-0 hi (at tol = 0, where hi == lo is the peak's own rounded value);
 * the test allows 64 eps.
 * tol < 0: TJ_PEAK_TOL; 0 is valid.  max_depth < 0: TJ_PEAK_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0: TJ_PEAK_FRONTIER; above it TJ_ERR_INVALID.
 * length_levels < 0: TJ_PEAK_LENGTH_LEVELS; above TJ_PEAK_MAX_LENGTH_LEVELS TJ_ERR_INVALID.  A NaN tol, records == NULL, a call before tj_init_state:
 * TJ_ERR_INVALID, records untouched.  A plain SHARDED context (world > 1) answers for its owned robots; records of other ranks' robots are all zero.
 * tj_group_peak_dynamics assembles the owners' records: bitwise one context's.  TWO launches whatever the fleet's size, the piece count and the depth; no host
 * loop over rounds or robots.  Changes no solver state, statistics or launch count.
 * The defaults are measured (tests/peak_dynamics_ref.py default_tolerance, the restatement, on the CPU): tol = 0 and max_depth = 40 on the final states of
 * tests/golden/e2e_scn_a.npz, e2e_scn_b.npz, e2e_scn_c3.npz and e2e_scn_b_coupled.npz; per depth the largest (hi - lo) / hi over robots and quantities, and
 * the largest live set:
 *   depth   0        1        2        3        4        5        6        7        8        9        10       11       12       13       14       15
 *   width   1.49e-2  7.88e-3  3.04e-4  5.04e-5  2.64e-5  9.48e-6  4.74e-6  1.73e-6  2.47e-7  1.11e-7  2.56e-8  6.72e-9  1.81e-9  4.56e-10 1.14e-10 2.78e-11
 *   live    3        2        2        2        2        2        2        2        2        2        2        2        2        2        2        2
 *   depth   16       17       18       19       20       21       22       23       24       25       26       27       28       29       30       31
 *   width   6.77e-12 1.72e-12 4.29e-13 1.10e-13 2.70e-14 7.12e-15 1.84e-15 6.89e-16 4.56e-16 3.44e-16 2.30e-16 2.28e-16 2.28e-16 1.15e-16 1.15e-16 0
 *   live    2        2        2        2        2        1        2        2        2        2        2        4        1        1        1        0
 * At depth 31 every live set has emptied (hi == lo): the floor is the last positive width, 1.15e-16 at depth 30, and TJ_PEAK_TOL is the smallest power of ten
 * >= 10 x that.  The largest live set is 4 items; TJ_PEAK_FRONTIER is the next power of two >= 4 x that, and at least 1024 (above every seed count in use: a
 * robot has piece_num * res seeds).  The largest (length_hi - length_lo) / length_hi per level on the same states:
 *   level   0        1        2        3        4        5        6
 *   width   1.69e-4  4.30e-5  1.08e-5  2.70e-6  6.76e-7  1.69e-7  4.23e-8
 * (a quarter per level); TJ_PEAK_LENGTH_LEVELS is the first below 1e-6 -- a micrometre per metre is beyond any use of a path length. */
#define TJ_PEAK_CONVERGED 4   /* hi - lo <= tol * hi, or nothing was left that could hold a larger value */
#define TJ_PEAK_TRUNCATED 8   /* the live set outgrew max_windows: the bracket of the last completed round is returned */
#define TJ_PEAK_MAX_DEPTH 40
#define TJ_PEAK_FRONTIER  1024   /* measured maximum of the live set: 4 */
#define TJ_PEAK_TOL 1e-14
#define TJ_PEAK_MAX_LENGTH_LEVELS 12
#define TJ_PEAK_LENGTH_LEVELS 4
#define TJ_DYN_SPEED    1   /* speed.lo >= vel_limit: the limit IS reached, at speed.time */
#define TJ_DYN_SPEED_OK 2   /* speed.hi < vel_limit: certified */
#define TJ_DYN_ACCEL    4   /* accel.lo >= acc_limit: the limit IS reached, at accel.time */
#define TJ_DYN_ACCEL_OK 8   /* accel.hi < acc_limit: certified */
typedef struct tj_peak {
  double lo, hi, time;     /* lo <= the quantity's peak over u's flight <= hi; lo is attained at `time` */
  int segment, depth;      /* the segment of the lo sample; rounds of halving completed */
  int windows, flags;      /* windows evaluated (seeds + 2 per halved item); TJ_PEAK_CONVERGED | TJ_PEAK_TRUNCATED */
} tj_peak;
typedef struct tj_dynamics_robot {
  tj_peak speed, accel, jerk;
  double length_lo, length_hi, duration, time_scale;
  int length_levels, flags;   /* the level the length bracket was formed at; TJ_DYN_* */
} tj_dynamics_robot;
int tj_peak_dynamics(tj_ctx* c, double tol, int max_depth, int max_windows, int length_levels, tj_dynamics_robot* records);
int tj_dynamics_record_size(void);   /* sizeof(tj_dynamics_robot) */
/* ---- tj_dynamics_windows: FROM WHEN TO WHEN is every robot's flown curve over (or under) a level of speed, acceleration or jerk, as certified time intervals
 * (csrc/kernels_dynamics_windows.h; read-only like tj_peak_dynamics).  tj_peak_dynamics names one peak per robot and quantity and time_scale; a state that is not
 * yet inside its limits -- an init file, tj_plan_init's output, a run stopped early, a timetable about to be compressed by a factor below time_scale -- exceeds a
 * limit over stretches, often several per flight, and re-timing or re-planning needs each with certified start and end times.  tj_flight_profile samples, and
 * samples certify nothing between them; tj_audit's speed / accel are control-vector maxima without a time.  The opposite sense, "when is the robot slower than a
 * level", gives hover and loiter stretches and hand-over points.  The interval counterpart of tj_peak_dynamics, as tj_obstacle_windows is tj_obstacle_approach's.
 * Nothing of another robot is read: all three modes, single-UAV included.  A gate k is (quantity q, sense, level); for every OWNED robot u and every gate:
 *   window   W = (segment tr, [sa, sb] in [0, 1] of the segment's local parameter), dyadic, as in tj_obstacle_windows; the real time of parameter s of segment
 *            tr is ((tr + s) / res) * piece_time[u], used wherever a time is formed.  The position on the flight tr + s is exact in a double (9 + 40 bits).
 *   net      c_0..c_n = tj_peak_dynamics' net: the raw derivative net of degree n = 4 (speed), 3 (acceleration), 2 (jerk) restricted to W by bez_restrict_n,
 *            always from the RAW net.  A vector c counts as norm3(c) / den, den in tj_peak_dynamics' association.
 *   bounds   ub(W) = max_i norm3(c_i) / den (at [0, 1] tj_audit's and tj_peak_dynamics' depth-0 bits).  lb(W): d = c_0 + c_1 + .. + c_n per axis, left to
 *            right; lb = (min_i dot3(c_i, d) / norm3(d)) / den where norm3(d) > 0 and the minimum is positive, else 0; dot3(c, d) = (c.x * d.x + c.y * d.y) +
 *            c.z * d.z.  The derivative lies in the hull of its net and |x| >= x . d / |d|, so lb <= the value on W <= ub.  h0, h5 = norm3(c_0) / den,
 *            norm3(c_n) / den: the values AT sa and sb, attained.
 *   class    ABOVE (within = value >= level): OUT if ub < level, else IN if lb >= level, else MIXED.  BELOW (within = value <= level): OUT if lb > level, else IN
 *            if ub <= level, else MIXED.  With sigma = -1 (ABOVE) / +1 (BELOW), g = sigma * value and L = sigma * level (negation is exact), "within" is
 *            g <= L for both senses, and the smallest g is the extreme value: the merge below is tj_obstacle_windows' with L as its dist and g as its distance.
 *   search   ONE per (robot, gate) over the whole flight.  Seeds: every segment at [0, 1]: IN to the leaves, MIXED to the live set, OUT dropped; seeding is
 *            never truncated.  Round d = 1, 2, ..: a live window whose time width ((sb - sa) / res) * piece_time[u] <= tol becomes an EDGE leaf with its h0 and
 *            h5; every other is halved at 0.5 * (sa + sb) and both children are evaluated from the raw net: OUT dropped, IN to the leaves, MIXED to the next
 *            live set.
 *   stop     the live set is empty | d == max_depth | after a round the live set holds more than max_windows or the leaves more than S + max_windows
 *            (TRUNCATED: the lists of the last completed round stand, `windows` counts the overflowing round's work too).  What is live at the end joins the
 *            leaves as EDGE leaves.
 *   merge    the leaves by flight position tr + sa: distinct and disjoint.  Two consecutive leaves are adjacent exactly when prev.tr + prev.sb == next.tr +
 *            next.sa on doubles (a chain crosses segment boundaries with no special case).  A row is a maximal chain.
 *   row      brackets, sure times, within_lo and flags by tj_obstacle_windows' rules word for word (a sure time: every time of an IN leaf; of an EDGE leaf sa
 *            if h0 is within the level and sb if h5 is).  extreme, extreme_time = ABOVE the largest, BELOW the smallest attained end sample of the chain and
 *            its time (equal values: the earlier time) -- not converged: tj_peak_dynamics converges the peak.  robot, gate (the index in `gates`), quantity,
 *            sense; segment_first, segment_last = the segments of the chain's ends; leaves = the chain's length; depth = the completed rounds of the (robot,
 *            gate) search; windows = its work, seeds + 2 per halved window; both repeated on each of its rows.
 *   flags    CERTAIN or UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED (the search of the row's robot and gate was truncated): tj_obstacle_windows' meanings.
 * Every field is a function of the state and the arguments alone; no order of evaluation or of any append is visible.  Rows are sorted by (robot, gate,
 * t_first_lo).  Outside every row of a gate the robot is certified on the other side of the level, up to the stated limits.
 * gates == NULL with n_gates == 0 selects the two default gates: (SPEED, ABOVE, vel_limit) and (ACCEL, ABOVE, acc_limit).  A non-null `gates` with n_gates == 0
 * is an empty list: 0 rows.  n_gates <= TJ_DYNWIN_MAX_GATES.  A NaN level, a quantity or a sense out of range: TJ_ERR_INVALID.  Any other level is valid:
 * level <= 0 ABOVE (and +infinity BELOW) gives the whole flight in one AT_START | AT_END row per robot, +infinity ABOVE none.  tol < 0:
 * (TJ_DYNWIN_TOL_FRACTION * vel_limit) / acc_limit -- a design condition, stated as such: the time in which a vehicle at the acceleration limit changes its speed
 * by 1 % of the speed limit, 0.01 s at the shipped parameters; 0 is valid.  max_depth < 0: TJ_DYNWIN_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0:
 * TJ_DYNWIN_FRONTIER; above TJ_DYNWIN_MAX_WINDOWS (it bounds the in-kernel rank sort) TJ_ERR_INVALID.  *n = the rows.  *n > cap: TJ_ERR_CAPACITY with the exact
 * *n, the first `cap` rows in order have been written.  cap == 0 with rows == NULL is the count-only call (one launch).  n == NULL, cap < 0, rows == NULL with
 * cap > 0, n_gates < 0, gates == NULL with n_gates > 0, a NaN tol or level, a call before tj_init_state: TJ_ERR_INVALID, the outputs untouched (precedence: null,
 * NaN, limits, no state).  A plain SHARDED context (world > 1) answers for its owned robots, as tj_peak_dynamics does.  tj_group_dynamics_windows returns the
 * owners' rows one after the other, bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, and is a function of owned x n_gates x (S, max_windows) (S = piece_num * res):
 *   owned * n_gates * ((3 * S + 4 * max_windows) * 56 + 16) + cap * 96 bytes
 *   (per (robot, gate) the two live lists of S + max_windows windows, which hold the sorted leaves afterwards, and S + 2 * max_windows leaves, 56 bytes a
 *   window; its four counters; the rows).  A call whose figure exceeds TJ_DYNWIN_MAX_BYTES is refused up front with TJ_ERR_INVALID: lower max_windows, cap or the
 *   number of gates.
 * TWO launches whatever the fleet's size, the number of gates and the depth (one for the count-only call); no host loop over robots, gates or rounds.  Changes
 * no solver state, statistics or launch count.
 * STATED LIMITS.  (1) ub and lb are sound up to rounding, in tj_peak_dynamics' terms: the roundings of the blossoming, norm3, the sum, the dot products and the
 * divisions, a small multiple of eps = 2^-53 of the robot's depth-0 ub of that quantity.  The CPU test measures, against the polynomial's real roots in mpmath,
 * the largest excess by which the truth contradicts a certified class (an OUT window or a gap holding a within time, an IN leaf holding an outside time), on
 * the four end states and tiny()'s initial states at the measurement's gates: no truly-within time outside a row (0), and 1.54 eps of the depth-0 ub inside
 * an IN leaf (a level the quantity touches: BELOW at 1.0 of the state's own jerk bound); the test allows the next power of two >= 16 x that, 32 eps.  (2) A quantity that EQUALS the level over an interval (a constant-speed line at exactly that speed; a hover at
 * level 0 BELOW is IN: ub = 0 <= 0) is resolved only down to tol, or ends TRUNCATED.  (3) Gaps shorter than a leaf are not resolved; UNCERTAIN rows are grazes at
 * the resolution tol.
 * The defaults are measured (tests/dynamics_windows_ref.py default_tolerance, the restatement, on the CPU; tools/dynamics_windows_measure.py prints the tables):
 * the default tol (0.01 s), max_depth = 40, the lists capped at TJ_DYNWIN_MAX_WINDOWS only, on the final states of tests/golden/e2e_scn_a.npz, e2e_scn_b.npz,
 * e2e_scn_c3.npz, e2e_scn_b_coupled.npz and on the same runs' iteration-0 states (_init); gates: all three quantities, both senses, levels 1.0 / 0.9 / 0.5 of
 * the limit (jerk: of the state's own largest depth-0 ub).  Per state the sums over its 18 gates of rows, UNCERTAIN rows and TRUNCATED rows, and the maxima of
 * the live set after a round >= 1, the leaf list, the depth and the widest bracket of a CERTAIN row:
 *   state                    rows   uncertain   truncated   largest live set   largest leaf list   largest depth   widest bracket
 *   e2e_scn_a                33     0           0           8                  47                  5               6.10e-03
 *   e2e_scn_a_init           26     0           0           12                 86                  9               9.77e-03
 *   e2e_scn_b                281    0           0           8                  58                  6               8.98e-03
 *   e2e_scn_b_init           105    0           0           2                  48                  9               9.77e-03
 *   e2e_scn_c3               2241   0           0           8                  62                  6               8.98e-03
 *   e2e_scn_c3_init          851    0           0           5                  70                  9               9.77e-03
 *   e2e_scn_b_coupled        281    0           0           8                  58                  6               8.98e-03
 *   e2e_scn_b_coupled_init   105    0           0           2                  48                  9               9.77e-03
 * A level set is crossed at isolated times, so the live set of a search stays at a few windows per crossing; what grows is the leaf list, by the IN windows of
 * a stay within the level.  TJ_DYNWIN_FRONTIER is the next power of two >= 4 x the largest live set, and at least 64. */
#define TJ_DYNWIN_SPEED 0
#define TJ_DYNWIN_ACCEL 1
#define TJ_DYNWIN_JERK  2
#define TJ_DYNWIN_ABOVE 0   /* within = value >= level */
#define TJ_DYNWIN_BELOW 1   /* within = value <= level */
#define TJ_DYNWIN_CERTAIN   1    /* a sure time exists: the quantity IS within the level at t_first_hi and at t_last_lo */
#define TJ_DYNWIN_UNCERTAIN 2    /* no sure time: t_first_hi == t_last_lo == -1.0, a graze at the resolution tol */
#define TJ_DYNWIN_AT_START  4    /* the chain starts at time 0: nothing lies before it */
#define TJ_DYNWIN_AT_END    8    /* the chain ends at the end of the robot's flight */
#define TJ_DYNWIN_RESOLVED  16   /* CERTAIN and both brackets are at most tol wide (a side closed by AT_START / AT_END counts as resolved) */
#define TJ_DYNWIN_TRUNCATED 32   /* the search of this robot and gate outgrew its lists: the leaves of the last completed round are returned */
#define TJ_DYNWIN_MAX_GATES 16
#define TJ_DYNWIN_MAX_DEPTH 40
#define TJ_DYNWIN_FRONTIER  64
#define TJ_DYNWIN_MAX_WINDOWS 1024
#define TJ_DYNWIN_MAX_BYTES (1ll << 31)
#define TJ_DYNWIN_TOL_FRACTION 0.01
typedef struct tj_dyn_gate { double level; int quantity, sense; } tj_dyn_gate;   /* TJ_DYNWIN_SPEED | ACCEL | JERK, TJ_DYNWIN_ABOVE | BELOW */
typedef struct tj_dynwin_row {
  double t_first_lo, t_first_hi;   /* the quantity first comes within the level in [t_first_lo, t_first_hi] */
  double t_last_lo,  t_last_hi;    /* ... and is last within it in [t_last_lo, t_last_hi] */
  double within_lo;                /* seconds CERTIFIED within the level inside the row (sum of the IN leaves) */
  double extreme, extreme_time;    /* ABOVE: the largest attained end sample of the chain, BELOW: the smallest; not converged: tj_peak_dynamics converges the peak */
  int robot, gate, quantity, sense;
  int segment_first, segment_last; /* the segments of the chain's ends */
  int leaves, depth, flags, windows;
} tj_dynwin_row;
int tj_dynamics_windows(tj_ctx* c, const tj_dyn_gate* gates, int n_gates, double tol, int max_depth, int max_windows, tj_dynwin_row* rows, int cap, int* n);
int tj_dynwin_row_size(void);   /* sizeof(tj_dynwin_row) */
/* ---- tj_zone_windows: FROM WHEN TO WHEN is every robot's flown curve inside (or outside) a volume the CALLER names at query time, as certified time intervals
 * (csrc/kernels_zone_windows.h; read-only like tj_dynamics_windows).  The window queries answer against the obstacle set (tj_obstacle_windows, tj_sight_windows), the
 * other robots (tj_proximity_windows) and the robot's own dynamics (tj_dynamics_windows): all fixed by the scene or the state.  A geofence the fleet must stay inside,
 * a no-fly box, an altitude band, the coverage ball of a ground station or a charging pad, a camera's work volume are none of these: they are no obstacles, never
 * enter the BVH or the optimiser, and change per question.  Sampling tj_flight_profile and testing points certifies nothing between the samples.  Nothing of another
 * robot is read: all three modes, single-UAV included.
 *   shapes   a table shapes[n_shapes][4] of doubles; a zone names rows first .. first + count - 1 of it.
 *   zone     TJ_ZONE_PLANES: the convex polytope that intersects the `count` half-spaces n_j . x <= d_j, a row is (nx, ny, nz, d), 1 <= count <=
 *            TJ_ZONEWIN_MAX_PLANES (an axis-aligned box is 6 rows, an altitude band 2, a one-sided fence 1).  Gauge g(x) = max_j (dot3(n_j, x) - d_j), faces left to
 *            right, dot3(n, x) = (n.x * x.x + n.y * x.y) + n.z * x.z; face(x) = the smallest j attaining it.  The library does NOT normalise: with unit normals g is
 *            metres, the signed distance inside the zone and next to a face, and a LOWER bound of the distance beyond an edge or a corner.
 *            TJ_ZONE_BALL: count == 1, the row is (cx, cy, cz, r).  Gauge g(x) = norm3(x - c) - r, the signed distance; face = -1.
 *   sense    TJ_ZONE_INSIDE: within means g <= level.  TJ_ZONE_OUTSIDE: within means g >= level.
 *   level    0 is the zone itself; -m with INSIDE is "inside with margin m"; -offset with OUTSIDE is "outside the fence, or within offset of it".
 * For every OWNED robot u and every zone k ONE search over the whole flight, tj_dynamics_windows' search word for word:
 *   window   W = (segment tr, [sa, sb] in [0, 1] of the segment's local parameter), dyadic; the real time of parameter s of segment tr is ((tr + s) / res) *
 *            piece_time[u], used wherever a time is formed.
 *   net      b_0..b_5 = the segment's raw 6-point hull (hull_entry's sums) restricted to W by bez_restrict, always from the RAW hull: [0, 1] returns it bit for bit.
 *   PLANES   f_ij = dot3(n_j, b_i) - d_j.  lb = max_j min_i f_ij, ub = max_j max_i f_ij; g0 = max_j f_0j and g5 = max_j f_5j, each with its face (the smallest j):
 *            attained at sa and sb.  Every f_j is affine, so on the hull it lies between its extremes over the net; a maximum of affine functions is then bounded by
 *            the maxima on both sides: lb <= g on W <= ub, and both tend to g as the window shrinks.
 *   BALL     e_i = b_i - c.  ub = max_i norm3(e_i) - r.  With d = e_0 + .. + e_5 per axis, left to right, lb = (min_i dot3(e_i, d) / norm3(d)) - r where norm3(d) > 0
 *            and the minimum is positive, else 0 - r: tj_dynamics_windows' projection bound on e (|x| >= x . d / |d| on the hull).  g0 = norm3(e_0) - r, g5 =
 *            norm3(e_5) - r.
 *   class    INSIDE: OUT if lb > level, IN if ub <= level, else MIXED.  OUTSIDE: OUT if ub < level, IN if lb >= level, else MIXED.  With sigma = +1 (INSIDE) / -1
 *            (OUTSIDE) a leaf carries sigma * g0 and sigma * g5 and the merge takes sigma * level as tj_obstacle_windows' dist (negation is exact): tj_dynamics_windows'
 *            BELOW / ABOVE.  "within" is sigma * g <= sigma * level for both senses, and the smallest sigma * g is the extreme sample.
 *   search   seeds: every segment at [0, 1]: IN to the leaves, MIXED to the live set, OUT dropped; seeding is never truncated.  Round d = 1, 2, ..: a live window whose
 *            time width ((sb - sa) / res) * piece_time[u] <= tol becomes an EDGE leaf with its g0 and g5; every other is halved at 0.5 * (sa + sb) and both children are
 *            evaluated from the raw hull.  Stop: the live set is empty | d == max_depth | after a round the live set holds more than max_windows or the leaves more
 *            than S + max_windows (TRUNCATED: the lists of the last completed round stand, `windows` counts the overflowing round's work too).  What is live at the
 *            end joins the leaves as EDGE leaves.
 *   merge    the leaves by flight position tr + sa; two consecutive leaves are adjacent exactly when prev.tr + prev.sb == next.tr + next.sa on doubles; a row is a
 *            maximal chain.
 *   row      brackets, sure times, within_lo and flags by tj_obstacle_windows' rules word for word (a sure time: every time of an IN leaf; of an EDGE leaf sa if g0 is
 *            within the level and sb if g5 is).  extreme, extreme_time, face = INSIDE the smallest, OUTSIDE the largest attained end sample of the gauge over the
 *            chain, its time and its face (equal values: the earlier time, then the smaller face) -- not converged.  robot, zone (the index in `zones`), sense;
 *            segment_first, segment_last, leaves, depth, windows as tj_dynamics_windows'.
 *   flags    CERTAIN or UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED: tj_obstacle_windows' meanings.
 * Every field is a function of the state and the arguments alone.  Rows are sorted by (robot, zone, t_first_lo).  Outside every row of a zone the robot is certified on
 * the other side of the level, up to the stated limits.
 * n_zones <= TJ_ZONEWIN_MAX_ZONES; n_zones == 0 gives 0 rows: there is no default zone.  tol < 0: (TJ_ZONEWIN_TOL_FRACTION * offset) / vel_limit -- a design
 * condition, stated as such: the time to fly 1 % of the contact distance at the speed limit, tj_obstacle_windows' at its default dist; 0 is valid.  max_depth < 0:
 * TJ_ZONEWIN_MAX_DEPTH; above it TJ_ERR_INVALID.  max_windows <= 0: TJ_ZONEWIN_FRONTIER; above TJ_ZONEWIN_MAX_WINDOWS (it bounds the in-kernel rank sort)
 * TJ_ERR_INVALID.  *n = the rows.  *n > cap: TJ_ERR_CAPACITY with the exact *n, the first `cap` rows in order have been written.  cap == 0 with rows == NULL is the
 * count-only call (one launch).  TJ_ERR_INVALID with the outputs untouched: n == NULL, cap < 0, rows == NULL with cap > 0, n_zones < 0 or n_shapes < 0, zones == NULL
 * with n_zones > 0, shapes == NULL with n_shapes > 0; a NaN tol, a non-finite level or shape value; n_zones above the limit, a kind or a sense
 * out of range, first / count outside the table or count outside the kind's range, an all-zero normal, r < 0, max_depth, max_windows; a call before tj_init_state
 * (precedence: null, NaN / non-finite, limits, no state).  A plain SHARDED context (world > 1) answers for its owned robots.  tj_group_zone_windows returns the owners'
 * rows one after the other, bitwise one context's.
 * DEVICE MEMORY is allocated by the first call that needs it, grows only, is freed by tj_destroy, and is a function of owned x n_zones x (S, max_windows):
 *   owned * n_zones * ((3 * S + 4 * max_windows) * 56 + 16) + cap * 96 bytes
 *   (per slot the two live lists of S + max_windows windows and S + 2 * max_windows leaves, 56 bytes a window; its four counters; the rows), and the zone list and
 *   the shape table, copied per call (at most 64 zones of 32 rows).  A call whose figure exceeds TJ_ZONEWIN_MAX_BYTES is refused up front with TJ_ERR_INVALID: lower
 *   max_windows, cap or the number of zones.
 * TWO launches whatever the fleet's size, the number of zones and the depth (one for the count-only call).  Changes no solver state, statistics or launch count.
 * STATED LIMITS.  (1) ub and lb are sound up to rounding: the roundings of the blossoming, dot3, norm3, the sum and the division, a small multiple of eps = 2^-53 of the
 * slot's scale -- the depth-0 largest |n_j| * |b_i| + |d_j| (PLANES), |e_i| + r (BALL).  The CPU test measures, against the real roots in mpmath of each face's
 * quintic f_j(x(s)) - level and of the degree-10 |x(s) - c|^2 - (r + level)^2, the largest excess by which the truth contradicts a certified class (a within time in
 * an OUT window or in a gap between rows, an outside time in an IN leaf): no truly-within time outside a row (0), and 0.283 eps of the slot's scale inside an IN leaf (e2e_scn_c3; 0 on the other states); the test allows the next power of two >= 16 x that, 8 eps.  (2) A gauge that EQUALS the level over an interval -- a flight at constant
 * altitude on a band's plane, a start or a goal on a face -- is resolved only down to tol, or ends TRUNCATED.  (3) Gaps shorter than a leaf are not resolved;
 * UNCERTAIN rows are grazes at the resolution tol.
 * The defaults are measured (tests/zone_windows_ref.py default_tolerance, the restatement, on the CPU; tools/zone_windows_measure.py prints the tables): the default
 * tol, max_depth = 40, the lists capped at TJ_ZONEWIN_MAX_WINDOWS only, on the final states of tests/golden/e2e_scn_a.npz, e2e_scn_b.npz, e2e_scn_c3.npz,
 * e2e_scn_b_coupled.npz and on the same runs' iteration-0 states (_init).  The zone set is built from each state: a box over the middle third of the fleet's bounding
 * box, the bounding box shrunk by offset (the fence), an altitude band of height 2 * offset through the mean z, a 32-face prism (30 sides around the vertical axis
 * through the bounding box's centre at the apothem of a quarter of its horizontal diagonal, floor and ceiling the box's), a ball at the fleet's centroid with a quarter
 * of the bounding box's diagonal as its radius; each in both senses at levels 0 and -offset: 20 zones.  Per state the sums over its zones of rows, UNCERTAIN rows and
 * TRUNCATED rows, and the maxima of the live set after a round >= 1, the leaf list, the depth and the widest bracket of a CERTAIN row:
 *   state                    rows   uncertain   truncated   largest live set   largest leaf list   largest depth   widest bracket
 *   e2e_scn_a                22     4           0           4                  72                  9               3.81e-04
 *   e2e_scn_a_init           17     0           0           2                  40                  14              3.05e-04
 *   e2e_scn_b                154    0           0           2                  52                  11              2.81e-04
 *   e2e_scn_b_init           157    0           0           14                 107                 14              3.05e-04
 *   e2e_scn_c3               1256   0           0           4                  52                  11              5.61e-04
 *   e2e_scn_c3_init          1284   6           0           73                 252                 14              3.05e-04
 *   e2e_scn_b_coupled        154    0           0           2                  52                  11              2.81e-04
 *   e2e_scn_b_coupled_init   157    0           0           14                 107                 14              3.05e-04
 * A level set is crossed at isolated times, so the live set of most searches stays at a few windows per crossing; the zones are built from the state's own bounding
 * box, so the topmost robot of an initial state flies at constant altitude ON the prism's ceiling (stated limit (2): e2e_scn_c3_init's robot 63 at z = 18.27, the
 * live set of 73 and the 6 UNCERTAIN rows; no other search of that state holds more than 4 windows).  TJ_ZONEWIN_FRONTIER is the next
 * power of two >= 4 x the largest live set (73), and at least 64: 512. */
#define TJ_ZONE_PLANES 0    /* the intersection of `count` half-spaces n_j . x <= d_j */
#define TJ_ZONE_BALL   1    /* |x - c| <= r */
#define TJ_ZONE_INSIDE  0   /* within = gauge <= level */
#define TJ_ZONE_OUTSIDE 1   /* within = gauge >= level */
#define TJ_ZONEWIN_CERTAIN   1    /* a sure time exists: the robot IS within the level at t_first_hi and at t_last_lo */
#define TJ_ZONEWIN_UNCERTAIN 2    /* no sure time: t_first_hi == t_last_lo == -1.0, a graze at the resolution tol */
#define TJ_ZONEWIN_AT_START  4    /* the chain starts at time 0: nothing lies before it */
#define TJ_ZONEWIN_AT_END    8    /* the chain ends at the end of the robot's flight */
#define TJ_ZONEWIN_RESOLVED  16   /* CERTAIN and both brackets are at most tol wide (a side closed by AT_START / AT_END counts as resolved) */
#define TJ_ZONEWIN_TRUNCATED 32   /* the search of this robot and zone outgrew its lists: the leaves of the last completed round are returned */
#define TJ_ZONEWIN_MAX_ZONES 64
#define TJ_ZONEWIN_MAX_PLANES 32
#define TJ_ZONEWIN_MAX_DEPTH 40
#define TJ_ZONEWIN_FRONTIER  512
#define TJ_ZONEWIN_MAX_WINDOWS 1024
#define TJ_ZONEWIN_MAX_BYTES (1ll << 31)
#define TJ_ZONEWIN_TOL_FRACTION 0.01
typedef struct tj_zone { double level; int kind, sense, first, count; } tj_zone;   /* TJ_ZONE_PLANES | BALL, TJ_ZONE_INSIDE | OUTSIDE, rows first .. first + count - 1 of the shape table */
typedef struct tj_zonewin_row {
  double t_first_lo, t_first_hi;   /* the robot first comes within the level in [t_first_lo, t_first_hi] */
  double t_last_lo,  t_last_hi;    /* ... and is last within it in [t_last_lo, t_last_hi] */
  double within_lo;                /* seconds CERTIFIED within the level inside the row (sum of the IN leaves) */
  double extreme, extreme_time;    /* INSIDE: the smallest attained end sample of the gauge (deepest), OUTSIDE: the largest; not converged */
  int robot, zone, sense, face;    /* face: of the extreme sample; -1 for a ball */
  int segment_first, segment_last; /* the segments of the chain's ends */
  int leaves, depth, flags, windows;
} tj_zonewin_row;
int tj_zone_windows(tj_ctx* c, const tj_zone* zones, int n_zones, const double* shapes, int n_shapes, double tol, int max_depth, int max_windows, tj_zonewin_row* rows, int cap, int* n);
int tj_zonewin_row_size(void);   /* sizeof(tj_zonewin_row) */
/* ---- tj_flight_profile: where every robot is at the flight times the caller names, how fast it moves there, how far the NEAREST obstacle primitive is --
 * with no `range`, however far -- and how far the nearest other robot is at the same time (csrc/kernels_flight_profile.h; read-only like tj_audit).  The other
 * queries answer with one minimum per robot or pair, and only inside `range`; this one is the curve against time: what a plot of clearance and speed, a look
 * for where a trajectory is tight, or a check of a sampled result file needs.  Every field is a function of the state alone.  Works in all three modes
 * (single-UAV included), for clouds and meshes.  For every OWNED robot u and every time t = times[k], record out[u * n_times + k]:
 *   time      The same real time t applies to every robot (equal flight times).  Time, segment boundaries and hover are tj_audit_timed's, unchanged:
 *             j = the segment with T(j) <= t < T(j + 1), T(j) = (j / res) * piece_time[u] in these very expressions; j == S: the robot has arrived.
 *             Then its position is hull_entry(S - 1, 5, .), its last control point -- the point tj_audit_timed's hover body is made of --, `segment` is S,
 *             speed = accel = 0 and HOVER is set.  Otherwise s = clamp01((t - T(j)) / (T(j + 1) - T(j))) is the position in segment j.
 *   position  per axis b_0 of the segment's raw hull (hull_entry's sums) restricted to [s, s] by blossoming (bez_restrict): five de Casteljau steps
 *             (1 - s) * x + s * y.  These are the bits tj_obstacle_approach attributes to a window that starts at s.
 *   dynamics  tj_audit's own nets, per axis v_i = 5 * (P[i+1] - P[i]), i = 0..4, and a_i = 20 * (P[i+2] - 2 * P[i+1] + P[i]), i = 0..3, each evaluated at s
 *             by the same step (four steps for v, three for a); speed = norm3(v) / (w * pt), accel = norm3(a) / (w * w * pt * pt), w the segment's
 *             weight, pt = piece_time[u].  At s == 0 these are tj_audit's first terms of the segment bit for bit: (1 - 0) * x + 0 * y is x.
 *   obstacle  obs_distance = the minimum over ALL primitives of the position's distance: a cloud point p: norm3(position - p); a triangle:
 *             |gjk({position}, triangle)|, with the limit stated for tj_obstacle_approach's hi.  Equal values go to the smallest caller index (the point
 *             index of tj_set_cloud / the face index of tj_set_mesh).  There is no `range` argument and no TJ_ERR_CAPACITY for this call, for any obstacle
 *             set: the walk is a nearest-neighbour descent of the box pyramid with a bounded stack, and it returns the brute-force minimum bit for bit.
 *             No obstacles: +infinity, index -1.
 *   robots    robot_distance = the minimum over q != u of norm3(p_u(t) - p_q(t)), every robot at its own segment or hover; equal values go to the smallest
 *             q.  Single-UAV mode: +infinity, robot -1.
 * times == NULL, out == NULL, n_times < 1, n_times > TJ_PROFILE_MAX_SAMPLES, uav_num * n_times > TJ_PROFILE_MAX_RECORDS, a NaN, negative or infinite time, a
 * call before tj_init_state: TJ_ERR_INVALID, and `out` is untouched.  A plain SHARDED multi-UAV context (world > 1) returns TJ_ERR_UNSUPPORTED like
 * tj_audit_timed: it does not hold the peers' piece_time.  tj_group_flight_profile reads control points and piece_time from the owners and is bitwise one
 * context's (unverified across distinct devices, like the other group queries); rows of robots a context does not own are all zero.  TWO launches whatever
 * uav_num, n_times and the number of primitives are; no host loop over samples or robots.  Changes no solver state, statistics or launch count. */
#define TJ_PROFILE_HOVER        1   /* the robot has arrived: it stays at its last control point */
#define TJ_PROFILE_OBS_CONTACT  2   /* obs_index >= 0 && obs_distance <= offset */
#define TJ_PROFILE_PAIR_CONTACT 4   /* robot >= 0 && robot_distance <= offset */
#define TJ_PROFILE_SPEED        8   /* speed >= vel_limit */
#define TJ_PROFILE_ACCEL        16  /* accel >= acc_limit */
#define TJ_PROFILE_MAX_SAMPLES  65536      /* n_times per call */
#define TJ_PROFILE_MAX_RECORDS  (1 << 24)  /* uav_num * n_times per call */
typedef struct tj_profile_sample {
  double time;                 /* the caller's t, echoed */
  double x, y, z;              /* position of the robot at t */
  double obs_distance;         /* distance to the NEAREST obstacle primitive, unbounded; +infinity with no obstacles */
  double robot_distance;       /* distance to the nearest OTHER robot's position at the same t; +infinity in single-UAV mode */
  double speed, accel;         /* |dp/dt|, |d2p/dt2| at t; 0, 0 while hovering */
  int obs_index;               /* caller's point index (tj_set_cloud) / face index (tj_set_mesh); -1 with no obstacles */
  int robot;                   /* the partner; -1 in single-UAV mode */
  int segment;                 /* the robot's segment at t; S while hovering */
  int flags;                   /* TJ_PROFILE_* */
} tj_profile_sample;
int tj_flight_profile(tj_ctx* c, const double* times, int n_times, tj_profile_sample* out /* [uav_num][n_times] */);
int tj_flight_profile_record_size(void);   /* sizeof(tj_profile_sample) */
/* teacher forcing of the CCD / line-search stages: overwrite robot u's search direction record (direction T x 3 column-major) */
int tj_set_direction(tj_ctx* c, int u, const double* direction, double t_direction, double wolfe, double gn);

/* ---- "optimal_plane":1 : the persistent plane tables (the reference globals is_seperate / seperate_c / seperate_d and
 * is_self_seperate / self_seperate_c / self_seperate_d, CCDUtils.cpp:30-36), for teacher-forced tests and checkpoints ---- */
/* single UAV: stored obstacle planes of (robot u, segment seg): ids = indices into the cloud given to tj_set_cloud,
 * cd[.][4] = (c, d); returns the number stored (may exceed cap; only min(n, cap) are written) */
int tj_get_obs_cache(tj_ctx* c, int u, int seg, int cap, int* ids, double* cd);
int tj_set_obs_cache(tj_ctx* c, int u, int seg, int n, const int* ids, const double* cd);
/* multi UAV: flags[S][U][U] (only p0 < p1 is used) and cd[S][U][U][4] = (c, d) of the plane between robots p0 and p1
 * before it is split into (c, d - offset/2) and (-c, -d - offset/2).  A sharded context (world > 1) tracks, returns and
 * accepts only the pairs that touch one of its own robots. */
int tj_get_pair_cache(tj_ctx* c, int* flags, double* cd);
int tj_set_pair_cache(tj_ctx* c, const int* flags, const double* cd);

/* counters since tj_init_state, for the algorithmic-byte model */
typedef struct tj_stats {
  unsigned long long iters, nodes_dcd, nodes_ccd, cand_dcd, cand_ccd, planes_obs, planes_self, energy_evals, pair_tests;
  unsigned long long llt_fail_piece, llt_fail_robot; /* PSD repairs taken: per-piece 19x19 blocks, per-robot reduced systems */
  unsigned long long newton_iters, pair_solves;      /* Optimal_plane::optimal_d iterations, robot pairs solved */
  int order_ambiguous; /* segments whose inter-robot clamp depended on pair order (two acting pairs sharing a robot): replayed in the
                          order of the reference's per-segment dynamic AABB tree (Step.h:213-251, AABB.cc:669-734) */
  int error_bits;      /* 1 plane list overflow, 2 BVH frontier overflow, 4 a loop hit its cap (detail: 32 coupled Armijo range, 64 plane
                          refinement, 128 CCD contact at every step = state in collision, 256 slack Armijo, 1024 a wait for passed-on pairs timed out, 2048 a wait of the asynchronous Newton solve timed out), 8 pair list overflow,
                          16 coupled Newton system not SPD, 512 tj_group: a peer's slice did not arrive */
  int order_unresolved; /* such segments for which the tree order could NOT be established (result may differ from the reference's;
                           tj_iterate returns TJ_ERR_UNSUPPORTED) -- 0 unless uav_num is in the thousands */
  int head_starts;      /* robot-pair GJK queries whose first iterations ran inside the broad-phase kernel and were continued by the solve
                           kernel (pairs that were slow in the previous iteration; same bits either way) */
  unsigned long long gjk_max_sum; /* sum over the iterations of the longest robot-pair GJK (iterations of openGJK's main loop; pairs below 6
                                     do not report): / iters = unit count of the pair stage's critical path */
  int ls_giveups;         /* line search, helper blocks: primaries that found a helper's post missing after 10 us and searched on alone (same result) */
  int ls_helper_timeouts; /* ... helper blocks that left after 5 ms without a word from their primary.  Both 0 on a GPU of the solver's own */
  int async_fallbacks;    /* batches that were run again on ONE hardware queue because a wait between the context's queues had run out (error bit 2048: a GPU shared with
                             another process).  The context keeps the one-queue chain from then on; the results are the same bits, the incident costs its 2 s limit once */
} tj_stats;
int tj_get_stats(tj_ctx* c, tj_stats* s);
/* the obstacle BVH of the last tj_set_cloud / tj_set_mesh: device time of the build (Morton keys, radix sort, box pyramid;
 * upload excluded) -- the counterpart of the reference's tree construction (BVH.cpp:53-93: 95 ms for 20k points) */
int tj_get_build_info(tj_ctx* c, double* bvh_build_ms, int* built_on_device);

/* (The known-answer hooks of the parity tests -- tj_kat_* -- are declared in trajadmm_kat.h and exist only in the TEST build
 * libtrajadmm_kat.so (-DTJ_KAT): the product library carries no test surface.) */

/* ---- initial-trajectory planner (replaces ompl_init + simplify_path + edge_collision, Main/multiPathPlanning3D.cpp:123-340
 * and HighOrderCCD/OMPL/OMPL.cpp; OMPL itself is not needed) -------------------------------------------------------------- */
/* The reference's motion validator for a batch of straight edges (OMPL.cpp:36-98, multiPathPlanning3D.cpp:123-160):
 * hit[i] = 1 if edge i = edges[i][2][3] comes within d of a cloud point (BVH::EdgeCollision + CCD::GJKDCD) or of one of
 * the prior edges (GJKDCD edge-edge).  The mains use d = offset + margin/2. */
int tj_edge_collision(tj_ctx* c, int n, const double* edges, int n_prior, const double* prior, double d, int* hit);
/* Plans way points for n_robots one after the other (a later robot treats the earlier robots' paths as obstacles, like
 * ompl_init): a deterministic roadmap -- start, goal and `nodes` Halton samples of bound_scale * bounding box of the cloud
 * (0 = the mains' 1.2 single / 1.5 multi), all-pairs visibility evaluated on the device with tj_edge_collision, shortest
 * path -- followed by the reference's simplify_path, a corner check (the hull of the solver's initial control net cuts every
 * corner; a fan of chords across the cut is validated and the edges at a failing corner are halved) and padding to a common
 * way-point count (>= min_waypoints, 0 = 6) by splitting the longest edges.  The reference plans with OMPL's randomised RRTConnect, so paths are not comparable point by point; what is kept
 * is the validity predicate, the post-processing and the output contract.  starts/goals are [n_robots][3]; waypoints is
 * [n_robots][cap_waypoints][3], the first *n_waypoints rows of each robot are written.  Any context with the cloud set
 * will do (tj_create with piece_num = 2 before the number of pieces is known). */
int tj_plan_init(tj_ctx* c, int n_robots, const double* starts, const double* goals, double bound_scale, int nodes, int min_waypoints, int cap_waypoints, double* waypoints, int* n_waypoints);

/* ---- robot sharding across GPUs (one context per rank) -------------------------------------- */
/* Device pointers + element counts of the buffers that must be all-gathered per iteration (robot-major, so a rank's owned
 * robots are one contiguous slice of doubles):
 *   what = 0  control points (spline, 3T doubles per robot)
 *   what = 1  search direction records (3T + 4: direction, t_direction, wolfe, |g|, the robot's share of the time gradient)
 * coupled mode ("decouple":0) only:
 *   what = 2  Schur-corner contributions of the shared piece_time (4 per robot)  -- the arrowhead system of update_spline,
 *             Optimization3D_multi.h:519-557: every rank eliminates its robots' blocks, the corner is their sum
 *   what = 3  obstacle CCD exponent of every robot (1)  -- Step::couple_self_step takes ONE step for all (Step.h:112-182)
 *   what = 4  energies of the Armijo candidates (4 rounds x 8 per robot)  -- the test is on the SUM over robots (:605-636) */
int tj_exchange_buffer(tj_ctx* c, int what, void** dev_ptr, int* doubles_per_robot, int* first_owned, int* n_owned);
/* Iteration split for external collectives.  Decoupled / single-UAV, 3 phases:
 *   phase 0 stop test | gather 0 | phase 1 planes, gradient, Newton direction | gather 1 | phase 2 CCD clamps, line search
 * coupled, 6 phases:
 *   phase 0 | gather 0 | phase 1 planes, gradient, per-robot elimination | gather 2 | phase 2 corner pivot + back substitution |
 *   gather 1 | phase 3 CCD clamps, shared step, gnorm | gather 3 | phase 4 Armijo candidates (all rounds) | gather 4 | phase 5 commit
 * Results are bitwise those of one unsharded context. */
int tj_phase_count(tj_ctx* c);
int tj_iterate_phase(tj_ctx* c, int phase);
/* The same with the caller saying whether another iteration follows in this batch (more != 0).  Decoupled / single-UAV schedules then run
 * the FUSED chain of one context inside the phases: phase 2's line search also does the next iteration's stop test and counter resets, so
 * that iteration's phase 0 launches nothing -- 6 kernels + the caller's 2 collectives per iteration (round 4: 10 + 2).  A begin that was
 * folded for an iteration the caller never enqueues is taken back by the next tj_sync / state access.  tj_iterate_phase(c, p) is
 * tj_iterate_phase_chained(c, p, 0).  The caches of the robots other ranks own (hull cache, swept-hull cache) are rebuilt from the gathered
 * buffers by extra units at the head of k_front / k_ccd (csrc/kernels_step.h), bitwise what the owner holds. */
int tj_iterate_phase_chained(tj_ctx* c, int phase, int more);

/* ---- direct exchange between sharded contexts (decoupled mode, world > 1; csrc/kernels_step.h) ---------------------------------------------
 * Instead of a collective between the phases, the PRODUCING kernels store an owned robot's slice straight into every peer's receive block
 * (k_linesearch / k_begin: control points for Optimization3D_multi.h:246-259 separate_self; k_xsolve: the direction record for Step.h:196-208
 * self_step) and bump an arrival counter there; the (foreign robot, segment) units at the head of the peers' k_front / k_ccd wait for the
 * count, read the slice and rebuild that robot's cache records.  With it a sharded iteration is the six-kernel chain of one context
 * (tj_iterate_async / tj_iterate work on the sharded context) -- nothing on the host, no launch for the exchange.  tj_group's "flag"
 * transport is this, wired inside one process; two or more PROCESSES (one per GPU, e.g. under torchrun) wire it through hipIpc:
 *   every rank:  tj_xch_ipc_export(c, handle)            64-byte handle of its receive block (allocated on first use, uncached memory)
 *                ... all-gather the handles with any host-side collective ...
 *                tj_xch_ipc_open(c, handle_of_peer, &base) for every other rank
 *                tj_xch_attach(c, world - 1, peer_ranks, peer_bases);  tj_xch_enable(c, 1, wait_mode)
 *   then tj_iterate_async / tj_iterate on every rank; every rank must run the same number of iterations per batch, and a host-side barrier
 *   must separate "every rank has drained its batch" from tj_init_state (which restarts the counters) and tj_init_state from the next batch.
 * wait_mode = 1: the foreign units poll the arrival counters themselves (ranks on distinct devices); 0: a one-wave launch in front of
 * k_front / k_ccd polls instead (ranks SHARING a device: polling units would hold the LDS the peer's producing kernel needs); 2: nobody polls --
 * the CALLER orders the streams (tj_group's event transport: an event recorded behind the producing kernel, waited for by the consumer's stream).
 * A push that does not arrive within 2 s fails the batch (TJ_ERR_DEVICE, error bit 512).  Results are bitwise those of one context.  UNVERIFIED ACROSS xGMI, like
 * tj_group on distinct devices: the tests run ranks and processes on one device. */
int tj_xch_block(tj_ctx* c, void** base, size_t* bytes);                 /* this rank's receive block (same-process wiring: hand `base` to the peers' tj_xch_attach) */
int tj_xch_ipc_export(tj_ctx* c, void* handle64);                        /* hipIpcGetMemHandle of the block */
int tj_xch_ipc_open(tj_ctx* c, const void* handle64, void** base);       /* hipIpcOpenMemHandle of a peer's block (closed by tj_destroy) */
int tj_xch_attach(tj_ctx* c, int n_peers, const int* peer_ranks, void* const* peer_bases);
int tj_xch_enable(tj_ctx* c, int on, int wait_mode);

/* ---- several GPUs under one process (csrc/tj_group.h) ------------------------------------------------------------------
 * What a maintainer of Main/multiPathPlanning3D.cpp would call instead of tj_create / tj_iterate to use N devices: the robots
 * of the per-robot loops (Optimization3D_multi.h:29-118, :120-174) are block-partitioned over n_ranks contexts, rank r on HIP
 * device devices[r] (NULL: device r; entries may repeat -- several ranks on one device, which is how the tests run it on a
 * one-GPU box).  tj_group_iterate runs the phase schedule above on every rank (one host thread per rank) and exchanges the
 * tj_exchange_buffer slices through one of three transports (csrc/tj_group.h):
 *   "event"  hipEventRecord behind the producing kernel / hipStreamWaitEvent in front of the consuming one: plain HIP stream semantics; THE DEFAULT.
 *            Decoupled mode: the slices travel by the direct exchange's in-kernel pushes (six kernels per iteration and rank, nothing launched for
 *            the exchange); coupled mode: a push kernel and an unpack kernel per exchange
 *   "flag"   decoupled mode: the DIRECT exchange above (tj_xch_*): the producing kernels push, the consuming kernels wait -- the fused
 *            six-kernel chain per rank, no launch and no host work for the exchange (ranks sharing a device: two one-wave wait launches);
 *            coupled mode: peer stores + a sequence flag polled by a small unpack kernel.  Opt-in until it has run across xGMI (a push
 *            that does not arrive within 2 s fails the batch with TJ_ERR_DEVICE / error bit 512)
 *   "rccl"   ncclCommInitAll + one in-place ncclAllGather per exchange on each rank's solver stream (the collective
 *            Optimization3D_multi's sharding would use over xGMI); librccl.so is opened at run time, only for this transport;
 *            needs distinct devices; uav_num not divisible by n_ranks: one grouped ncclBroadcast per owner instead
 * chosen by TJ_GROUP_TRANSPORT at tj_group_create or by tj_group_set_transport between batches.  Results are bitwise those of
 * one context.  tj_params.rank / world / device are ignored (set per rank).  Single-UAV mode has nothing to shard (n_ranks
 * must be 1).  UNVERIFIED ON HARDWARE: a group whose devices are all distinct (the configuration the feature exists for) has
 * not run yet -- no multi-GPU box was available to rounds 1-3; same-device groups are tested bitwise against one context. */
typedef struct tj_group tj_group;
/* Coupled mode ("decouple":0) on SHARDED contexts: the Armijo search on the summed energy has no bound in the reference (Optimization3D_multi.h:605-636); one exchange of
 * buffer 4 carries the candidates 0.8^0 .. 0.8^30.  Default: a search that needs more ends in TJ_ERR_NO_PROGRESS (error bit 32), as in round 5.  With follow = 1 phase 5
 * commits nothing in that case and the caller -- after phase 5 of every iteration -- asks tj_coupled_search_pending (it drains the context's stream: the one host look of the
 * schedule); while it answers 1: run phase 4, exchange buffer 4, phase 5 again (they evaluate, carry and decide the next 32 candidates) and ask again.  Every rank reads
 * the same answer.  tj_group does this by itself: a batch that runs into error bit 32 is run again from its first state with the followed search.  One context needs
 * neither call (its deciding block goes on alone). */
int tj_set_coupled_follow(tj_ctx* c, int on);
int tj_coupled_search_pending(tj_ctx* c, int* pending);
int tj_group_create(const tj_params* p, int n_ranks, const int* devices, tj_group** out);
void tj_group_destroy(tj_group* g);
int tj_group_size(tj_group* g);
tj_ctx* tj_group_ctx(tj_group* g, int rank);          /* rank's context: stats, planes, caches of the robots it owns */
const char* tj_group_last_error(tj_group* g);         /* g == NULL: why the last tj_group_create failed */
int tj_group_set_cloud(tj_group* g, const double* xyz, int n);   /* the obstacle BVH is replicated on every device */
int tj_group_set_mesh(tj_group* g, const double* vertices, int n_vertices, const int* faces, int n_faces);
int tj_group_init_state(tj_group* g, const double* waypoints, double piece_time0);
int tj_group_iterate(tj_group* g, int n_iters, double* gnorm, int* iters_total, int* converged);   /* like tj_iterate */
int tj_group_get_state(tj_group* g, int u, double* spline, double* p_slack, double* p_lambda, double* t_slack, double* t_lambda, double* piece_time);   /* from u's owner */
int tj_group_audit(tj_group* g, double range, tj_audit_robot* out, double* seg_obs, double* seg_pair);   /* tj_audit of every robot by its owner, against every robot's control points as its owner holds them: bitwise one context's */
int tj_group_audit_timed(tj_group* g, double range, int levels, tj_audit_timed_robot* records, double* seg_lo, double* seg_hi);   /* tj_audit_timed of every robot by its owner; every robot's control points AND piece_time are read from its owner: bitwise one context's */
int tj_group_closest_approach(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_closest_robot* records);   /* tj_closest_approach of every robot by its owner; control points and piece_time from the owners: bitwise one context's */
int tj_group_pair_approach(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_pair_record* rows, int cap, int* n);   /* tj_pair_approach of every robot by its owner, the ranks' rows one after the other: (robot, partner) order, bitwise one context's */
int tj_group_path_crossings(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_crossing_record* rows, int cap, int* n);   /* tj_path_crossings of every pair (u, q > u) by u's owner, the ranks' rows one after the other: (robot, partner) order, bitwise one context's */
int tj_group_timing_margin(tj_group* g, double dist, double max_slip, double tol, int max_depth, int max_windows, tj_margin_record* rows, int cap, int* n);   /* tj_timing_margin of every pair (u, q > u) by u's owner, in the same way */
int tj_group_proximity_windows(tj_group* g, double dist, double tol, int max_depth, int max_windows, tj_proximity_row* rows, int cap, int* n_pairs, int* n);   /* tj_proximity_windows of every robot by its owner, the ranks' rows one after the other: (robot, partner, t_first_lo) order, bitwise one context's; every rank gets `cap` pair slots and the rows' remaining room */
int tj_group_obstacle_approach(tj_group* g, double range, double tol, int max_depth, int max_windows, tj_obstacle_robot* records);   /* tj_obstacle_approach of every robot by its owner, from the owner's own state: bitwise one context's */
int tj_group_obstacle_windows(tj_group* g, double dist, double tol, int max_depth, int max_windows, tj_obswin_row* rows, int cap, int* n);   /* tj_obstacle_windows of every robot by its owner, from the owner's own state, the ranks' rows one after the other: (robot, t_first_lo) order, bitwise one context's */
int tj_group_sight_windows(tj_group* g, const int* links, int n_links, const double* stations, int n_stations, double dist, double tol, int max_depth, int max_windows, tj_sight_row* rows, int cap, int* n);   /* tj_sight_windows of every link by the rank that owns its robot a, nets and piece_time from the owners: (link, t_first_lo) order, bitwise one context's */
int tj_group_peak_dynamics(tj_group* g, double tol, int max_depth, int max_windows, int length_levels, tj_dynamics_robot* records);   /* tj_peak_dynamics of every robot by its owner, from the owner's own state: bitwise one context's */
int tj_group_dynamics_windows(tj_group* g, const tj_dyn_gate* gates, int n_gates, double tol, int max_depth, int max_windows, tj_dynwin_row* rows, int cap, int* n);   /* tj_dynamics_windows of every robot by its owner, from the owner's own state, the ranks' rows one after the other: (robot, gate, t_first_lo) order, bitwise one context's */
int tj_group_zone_windows(tj_group* g, const tj_zone* zones, int n_zones, const double* shapes, int n_shapes, double tol, int max_depth, int max_windows, tj_zonewin_row* rows, int cap, int* n);   /* tj_zone_windows of every robot by its owner, from the owner's own state, the ranks' rows one after the other: (robot, zone, t_first_lo) order, bitwise one context's */
int tj_group_flight_profile(tj_group* g, const double* times, int n_times, tj_profile_sample* out);   /* tj_flight_profile of every robot by its owner; control points and piece_time from the owners: bitwise one context's */
const char* tj_group_transport(tj_group* g);          /* "flag", "event" or "rccl" */
int tj_group_set_transport(tj_group* g, const char* name);   /* between batches; restarts the exchange sequence numbers */
/* event-timed cost of one exchange of each buffer kind (microseconds, slowest rank's average over `reps`): us[5], kinds 2..4
 * are zero outside coupled mode; all zero for one rank */
int tj_group_profile_exchange(tj_group* g, int reps, double* us);
/* 1 if librccl.so can be opened and exports the entry points the "rccl" transport binds (needs no GPU) */
int tj_rccl_available(void);
/* ranks the group's RCCL communicator reports (ncclCommCount); 0 unless the "rccl" transport is selected */
int tj_group_rccl_ranks(tj_group* g);
/* After a rank failed inside tj_group_iterate the ranks' exchange counts disagree: every tj_group_* call except
 * tj_group_init_state (which drains the streams and restarts the counters) and tj_group_destroy then returns TJ_ERR_DEVICE. */

#ifdef __cplusplus
}
#endif
#endif
