/* trajadmm_kat.h -- known-answer hooks of the parity tests.  TEST SURFACE ONLY: these entry points exist in
 * traj-opt-admm_amd/libtrajadmm_kat.so (the same translation unit as libtrajadmm.so compiled with -DTJ_KAT, csrc/Makefile) and
 * are absent from the product library.  tests/test_gpu_parity.py::test_kat_build_equals_product_build asserts that the two
 * builds run the hot path to the same bits. */
#ifndef TRAJADMM_KAT_H
#define TRAJADMM_KAT_H
#include "trajadmm.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- known-answer hooks: the device primitives of the hot path on caller-supplied batches -------
 * (host pointers; one case per GPU lane; used by the parity tests against tests/golden/) */
/* GJK witness vector (replaces gjk(), lib/opengjk/src/openGJK.c:754): n1 in {6,12}, n2 in {1,3,6,12} (3 = obstacle triangle);
 * a[n][n1][3], b[n][n2][3], v[n][3] */
int tj_kat_gjk(tj_ctx* c, int n, int n1, const double* a, int n2, const double* b, double* v);
/* the same query solved cooperatively by a whole wavefront (the form the inter-robot kernels use): must give the same bits */
int tj_kat_gjk_wave(tj_ctx* c, int n, int n1, const double* a, int n2, const double* b, double* v);
/* the same query interrupted after k_stop iterations, its loop state taken through memory and the loop continued (what the GJK head start of the
 * robot-pair stage does across two kernels): v_iters[4 n] = witness vector, iterations of the whole query */
int tj_kat_gjk_wave_split(tj_ctx* c, int n, int n1, const double* a, int n2, const double* b, int k_stop, double* v_iters);
/* what: 0 Separate::opengjk (Separate.h:18) P[n][6][3], Q = points [n][3] -> out[n][5] = ok,cx,cy,cz,d
 *       1 Separate::selfgjk + Optimal_plane::optimal_d (Separate.h:165, Optimal_plane.h:13), Q[n][6][3] -> ok,c,d
 *       2 CCD::KDOPDCD (CCD.h:354), 3 CCD::SelfKDOPDCD (CCD.h:535) -> out[n][5], out[.][0] = pass
 *       4 = 1 computed by one wavefront per pair (plane_pair_wave, the form k_sep_self_solve uses)
 *       5 Optimal_plane::optimal_cd (Optimal_plane.h:160), Q = points; 6 Optimal_plane::self_optimal_cd (:620), Q = hulls:
 *         7 = 6 computed by one wavefront per plane (opt_plane_pair_wave, the form k_keep uses for short lists);
 *         out[n][5] is IN/OUT, out[.][1..4] = the plane (c, d) to refine, out[.][0] = finished within the iteration caps */
int tj_kat_planes(tj_ctx* c, int what, int n, const double* P, const double* Q, double dist, double* out);
/* CCD::GJKCCD / SelfGJKCCD (CCD.h:116,227) on swept hulls, tu[n][2] = (tMax, _tMax): out[n][2] booleans */
int tj_kat_ccd(tj_ctx* c, int n, const double* P, const double* D, const double* Q, const double* E, const double* q, const double* tu, double d, double* out);
/* broad phase alone (replaces aabb::Tree::query(AABB, margin), AABB.cc:829-839 / :608-667, on the tree of BVH::InitPointcloud or
 * BVH::InitObstacle): boxes[nq][6] = lo.xyz, hi.xyz; counts[nq]; ids[nq][cap] = indices into the caller's cloud / face list.
 * A box whose walk overflows the frontier (FRONT_CAP boxes on one level), or that finds more than cap candidates, makes the call return TJ_ERR_CAPACITY.
 * That is an error of this call alone: the walk reports it through the read-only queries' control block, the solver's error word stays clear and the
 * context goes on answering.  Pending work of the context is waited for before the queries are launched. */
int tj_kat_query(tj_ctx* c, int nq, const double* boxes, double margin, int cap, int* counts, int* ids);
/* the same in each form of the walk the product kernels instantiate: unroll = 4 (the plane query) or 1 (the CCD query, the audit, the obstacle-approach seeds,
 * the planner); pre != 0: the lane's top-level box is fetched ahead of the query box and handed to the walk (the plane and CCD queries).  tj_kat_query is
 * unroll 4, pre 0.  ids come in the walk's own order: positions of the build's sorted order, ascending.  A frontier overflow is TJ_ERR_CAPACITY of this call
 * alone (reported through the read-only queries' control block): the context stays usable. */
int tj_kat_query_form(tj_ctx* c, int nq, const double* boxes, double margin, int cap, int unroll, int pre, int* counts, int* ids);
/* triangle obstacle bodies (tj_set_mesh): P, D [n][6][3] hull and direction hull, tri[n][3][3], t[n] step; out[n][8] =
 * plane ok, cx, cy, cz, d of Separate::opengjk with a 3-vertex body at distance dist | CCD::KDOPDCD(P, tri, dist) |
 * CCD::KDOPDCD({P, P + t D}, tri, off) | CCD::GJKDCD({P, P + t D}, tri, off)  -- the predicates Step::mix_step uses (Step.h:390-404) */
int tj_kat_tri(tj_ctx* c, int n, const double* P, const double* D, const double* tri, const double* t, double dist, double off, double* out);
/* the obstacle 49-axis cull in the form the obstacle walks run it (kdop_cull_wave: one wave per case, lanes over the axes, up to 64 candidates on the lanes):
 * prim 1 points / 3 triangles; P[n][6][3] hull; swept != 0: the intervals of conv{P, P + t D} (D[n][6][3], t[n]; both may be NULL otherwise);
 * bodies[n][per][prim][3], per <= 64; nc[n] = candidates of case i that take part (lanes [0, nc[i]); NULL: all per); out[n][per] = pass, 0 beyond nc[i].
 * tj_kat_planes' what 2 and tj_kat_tri's two k-DOP outputs are this call with one candidate per case. */
int tj_kat_kdop_wave(tj_ctx* c, int prim, int swept, int n, int per, const double* P, const double* D, const double* t, const double* bodies, const int* nc, double d, double* out);
/* dense LLT failure test + smallest eigenvalue (Eigen LLT / SelfAdjointEigenSolver as used at Gradient_admm.h:38-53): out[nmat][2] */
int tj_kat_linalg(tj_ctx* c, int nmat, int n, const double* mats, double* out);
/* the per-piece gradient and Hessian blocks of the whole fleet, written from the host: lg[U][P][19], lh[U][P][361] (row-major 19 x 19; local 0..17 = global
 * coordinates 9 piece .. 9 piece + 17, local 18 = the time variable) -- what tj_get_local_grad reads back and the only input of the Newton solve.  With
 * tj_run_stage(TJ_STAGE_XSOLVE) and tj_get_direction this feeds the product's own solve kernels any system.  Pending work of the context is waited for, no
 * kernel is launched.  TJ_ERR_INVALID: a null argument, or a context without cloud / state. */
int tj_kat_set_local_grad(tj_ctx* c, const double* lg, const double* lh);
/* the hull cache of the robot-pair stage as its last writer left it (k_hullinfo, k_front's units or k_linesearch -- which one depends on the schedule):
 * hullinfo[U][S][122] = hull 18, box lo/hi 6, the 49 k-DOP intervals lo, hi of every (robot, segment) record; hbox[S][6][U] = the boxes again as the
 * pair tiles read them.  Pending work of the context is waited for, no kernel is launched.  TJ_ERR_INVALID: a null argument, or a context without cloud / state. */
int tj_kat_get_hull_record(tj_ctx* c, double* hullinfo, double* hbox);
/* the swept-hull cache of the two CCD stages as its last writer left it (k_ccd_prep, k_xsolve's tail or k_ccd's units -- which one depends on the schedule):
 * ccdinfo[U][S][146] = hull P 18, direction hull D 18, obstacle box lo/hi 6, pair box lo/hi 6, the 49 k-DOP intervals lo, hi of every (robot, segment) record;
 * cbox[S][6][U] = the pair boxes again as the selection tiles read them.  Pending work of the context is waited for, no kernel is launched.  TJ_ERR_INVALID: a
 * null argument, or a context without cloud / state. */
int tj_kat_get_swept_record(tj_ctx* c, double* ccdinfo, double* cbox);

/* ---- the launch plan (csrc/host_plan.h) ------------------------------------------------------------
 * A flat record of ints: the device facts the plan was decided on (PlanFacts), then every decision of the plan, the LDS byte counts, the queue
 * request and the grid sizes (plan_record; the Python package names the entries: PLAN_FACTS, PLAN_FIELDS).
 *   c != NULL: that context's own record (p and facts are ignored): the plan as tj_create made it, plus the live Dev -- not what a self-heal latched off since.
 *   c == NULL: the pure planner on the caller's parameters and facts[] -- needs no device, like tj_host_tables; an unsupported shape gives its
 *              TJ_ERR_* code in the record's `err` entry and the text in msg.
 * Returns the number of ints written, 0 for bad arguments, -needed if cap is too small. */
int tj_kat_plan(const tj_ctx* c, const tj_params* p, const int* facts, int* out, int cap, char* msg, int msg_cap);

/* ---- the launch sequence (csrc/host_launch.h) ------------------------------------------------------
 * What the schedules enqueue for a list of calls (kid, sched, chain_pos) -- sched: 0 stage, 1 chain, 2 phase --, as flat records of ints; nothing is launched.
 * Per call: exists, number of records, the host state (SchedState) after the call, then the Launch records: kernel id (K_COUNT and up: the three gates, k_xch_wait,
 * the counter clear), form, primitive kind, queue, grid, block, dynamic LDS bytes, four scalar arguments, the eleven Dev fields the launch overrides (the Python
 * package names the entries: SCHED_STATE, LAUNCH_FIELDS).
 *   c != NULL: that context's own Dev, plan and state; its state is written to state[] and stays as it is (p, facts, lsc_follow are ignored).  One entry is read
 *              from state[] instead: xs_same_queue_now, which tj_profile_kernels sets around its run only -- nonzero asks for that run's sequence.
 *   c == NULL: the planner's Dev and plan on the caller's parameters and facts[] (as tj_kat_plan), Dev::lsc_follow = lsc_follow, from the start state in state[];
 *              needs no device.
 * Returns the number of ints written, 0 for bad arguments or a shape the planner refuses, -needed if cap is too small. */
int tj_kat_launches(const tj_ctx* c, const tj_params* p, const int* facts, int lsc_follow, int* state, const int* calls, int n_calls, int* out, int cap);

/* ---- the device arrays of a context (csrc/tj_api.hip: device_arrays) --------------------------------
 * The declaration table every allocation, checkpoint region, reset and host copy takes its sizes from, as four ints per array -- element count, element size in
 * bytes, 1 if the array is part of the checkpoint, what tj_init_state fills it with (0 nothing, 1 zero bytes, 2 one bytes) -- in declaration order, and the arrays'
 * names (the members of Dev) as one comma-joined string in names[].
 *   c != NULL: that context's own table (p and facts are ignored).
 *   c == NULL: the table of the planner's Dev on the caller's parameters and facts[] (as tj_kat_plan); needs no device.
 * Returns the number of arrays, 0 for bad arguments or a shape the planner refuses, -count if cap (ints) or names_cap (chars) is too small. */
int tj_kat_arrays(const tj_ctx* c, const tj_params* p, const int* facts, int* out, int cap, char* names, int names_cap);

#ifdef __cplusplus
}
#endif
#endif
