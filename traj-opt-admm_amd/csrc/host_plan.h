// host_plan.h -- the launch plan of a context, decided in one pure function.
//
// plan_context() takes the caller's tj_params, a handful of device facts (PlanFacts) and the switch reader, and returns everything tj_create needs to know before its
// first allocation: the launch-shape fields of Dev, the host-side ones (HostPlan), the LDS byte counts, how many hardware queues the context wants, and -- for
// a shape this version cannot run -- the error.  It makes no HIP runtime call and reads every switch of the plan in exactly one place, so it runs (and is tested)
// without a device.  tj_create plans, claims its queues, plans AGAIN with PlanFacts::claim_refused set if the claim was refused, and creates its streams; a stream
// that cannot be created downgrades the plan through plan_downgrade.  Two helpers live here because more than one place needs the same arithmetic: plan_grids
// (the grid sizes of the union kernels: the residency rule of Dev::fa_mid and sequence_kernel, host_launch.h) and plan_ls_help (tj_group.h re-decides it for ranks sharing a device).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace tj {

typedef const char* (*TuneFn)(const char* key);

// ---- what the planner is told about the device (tj_create: gather_facts; all ints, in this order in the test hook's record) ----
struct KernelFact { int ok, regs, lds; };   // hipFuncGetAttributes succeeded / numRegs / sharedSizeBytes (static)
struct PlanFacts {
  int num_cu;
  KernelFact xsolve;    // the k_xsolve<N> of this piece count
  KernelFact grad[2];   // k_grad<false>, k_grad<true>
  KernelFact front;     // k_front<1, true> (ok: this query), registers and LDS: the larger of it and k_front<3, true>
  int counters_on;      // rocprofv3's counter collection is active (ROCPROF_COUNTER_COLLECTION)
  int claim_refused;    // the queues the first plan asked for did not fit the process's budget
  int prim, n_obs;      // the obstacle set (plan_grids only; 1, 0 until tj_set_cloud / tj_set_mesh)
};
constexpr int PLAN_FACT_INTS = sizeof(PlanFacts) / sizeof(int);

// ---- the host-side half of the plan (tj_ctx::hp: kept as made; SchedState, host_launch.h, owns the live copies of xs_two_queues / keep_two_queues / xs_fault, hwq_refused is a record only) ----
struct HostPlan {
  size_t lds_grad = 0, lds_xs = 0, lds_xs2 = 0, lds_ls = 0, lds_seq = 0;
  LsLayout lsl;
  bool lsc_wide = false;     // coupled mode: k_ls_coupled evaluates all LSC_ROUNDS rounds in one launch (kernels_ls.h)
  bool grad_fold = true;     // k_grad compacts its own segments (one launch less); TJ_GRAD_FOLD=0 keeps k_sep_self_compact + the 192-thread k_grad
  int n_solve_env = 0;       // TJ_N_SOLVE: pair-solve waves of k_mid (launch-shape switch)
  bool fa_emulate = false, fa_mid_ok = false;   // TJ_FRONT_ASYNC_ONE_QUEUE=1 / Dev::fa_mid: k_front's grid is resident next to one k_linesearch block
  int fa_mid_front = 0;      // the k_front grid the residency rule of fa_mid_ok was decided for (0: not asked)
  bool hwq_refused = false;  // no room in the queue budget
  int queues = 1; bool forced = false;                 // streams the context wants (main + second + third) / an explicit TJ_XS_ASYNC=1 / TJ_KEEP_ASYNC=1 bypasses the budget
  bool xs_two_queues = false, keep_two_queues = false; // SchedState: stream2 / stream3 in use
  bool heal = true; int xs_fault = 0;                  // TJ_HEAL=0: self-healing off / test hook TJ_XS_FAULT: the n-th gate reports a time-out
  bool bvh_skip_forced = false, ls_help_forced = false; int ls_help_asked = 0;   // TJ_BVH_SKIP / TJ_LS_HELP are set (set_obstacles / tj_group.h decide otherwise)
  size_t lds_grad_of(bool fold, int res) const { return lds_grad + (fold ? grad_fold_extra_doubles(res) * sizeof(double) : 0); }   // dynamic LDS of k_grad<fold>
};

struct Plan { int err = TJ_OK; const char* msg = ""; Dev d; HostPlan h; };

// ---- grid sizes of the iteration's kernels (one wave per block) ----
struct Grids { int n_rows, n_ccd, n_xf, n_front, n_solve, n_obs_solve, n_mid_slack; };
inline Grids plan_grids(const Dev& d, int n_solve_env) {
  const bool multi = d.mode >= 1;
  Grids g;
  // Waves striding over the two device-built work lists.  k_mid holds ~1 wave per SIMD (VGPR bound), i.e. 1024 resident
  // waves: a larger grid adds no parallelism, only dispatch time for blocks that find no work (measured: with
  // 4096 + 1024 blocks the last ones started 50 us into a 60 us kernel).
  // Large fleets (one pair per lane, long solves passed on to idle waves -- sep_self_solve_body): half as many waves again, they
  // are the consumers of the passed-on pairs (SCN-D: k_mid 62 us with 1024, 58 with 1536, 62 with 2048).
  // Small fleets (a wave per pair, two or three pairs per wave): 1 728 = what is left of k_mid's 2 048 resident waves beside SCN-C's
  // 320 slack blocks (1 024: k_mid 31.5 us, 1 536: 28.2, 1 728: 27.6, 2 048: 27.6 before the static assignment; alike after it).
  g.n_solve = (multi && !d.optimal_plane) ? std::min(d.cap_work, n_solve_env > 0 ? n_solve_env : (d.U >= 192 ? 1536 : 1728)) : 0;  // "optimal_plane":1 -- k_keep finds and refines the pair planes
  g.n_obs_solve = d.N > 0 ? 1024 : 0;   // (512: SCN-E's k_mid 43.7 us, 1024: 38.3, 2048: 37.8; SCN-C indifferent)
  // the union kernels: their block layouts (kernels_step.h) say what each grid holds.  n_ccd: obstacle units + pair tiles, without the foreign units and k_ccd's finisher
  const FrontLayout lf(d); const CcdLayout lc(d);
  g.n_rows = lc.tiles();
  g.n_xf = d.xf_units();   // sharded contexts: one wave per (foreign robot, segment) at the head of k_front / k_ccd (kernels_step.h); coupled chain: per (robot, segment)
  g.n_ccd = lc.total() - lc.xf;
  g.n_front = lf.total();
  g.n_mid_slack = MidLayout::slack_blocks(d);
  return g;
}

// helper blocks of k_linesearch: one CU each, so as many per robot as `cus` compute units have to spare (64 robots on 256 CUs: 4).  TJ_LS_HELP (launch-shape switch,
// same bits; 1 = no helpers): more blocks per robot than the compute units hold at once would leave helpers waiting for a unit while every primary runs into its
// 10 us give-up per super-round, so it is clamped to the units there are
inline int plan_ls_help(const Dev& d, const HostPlan& h, int cus) {
  const int room = std::max(1, cus / std::max(1, d.u1 - d.u0));
  if (h.ls_help_forced) return std::min(std::max(1, std::min(LS_HELP_MAX, h.ls_help_asked)), room);
  return (d.ls_fast && d.mode != TJ_MODE_MULTI_COUPLED) ? std::min(LS_HELP_MAX, room) : 1;
}

// a stream the plan asked for could not be created: no stream2 -- the tickets and flags of the asynchronous solve work on one queue as well; no stream3 -- k_keep stays on the chain
inline void plan_downgrade(Plan& pl, bool have_stream2, bool have_stream3) {
  if (!have_stream2) pl.h.xs_two_queues = false;
  if (!have_stream3) { pl.d.keep_async = 0; pl.h.keep_two_queues = false; }
}

inline const char* plan_check_params(const tj_params* p) {
  if (p->uav_num < 1 || p->piece_num < 2 || p->res < 1 || p->mode < 0 || p->mode > 2 || p->world < 1 || p->rank < 0 || p->rank >= p->world)
    return "invalid tj_params (need uav_num>=1, piece_num>=2, res>=1, mode 0/1/2, 0<=rank<world)";
  if (p->mode == TJ_MODE_SINGLE && p->uav_num != 1) return "TJ_MODE_SINGLE requires uav_num == 1";
  return nullptr;
}

inline Plan plan_context(const tj_params* p, const PlanFacts& f, TuneFn tune) {
  Plan pl;
  Dev& d = pl.d; HostPlan& h = pl.h;
  memset(&d, 0, sizeof(d));
  auto fail = [&](const char* msg) { pl.err = TJ_ERR_UNSUPPORTED; pl.msg = msg; return pl; };
  auto flag = [](const char* e, int dflt) { return e ? (atoi(e) != 0 ? 1 : 0) : dflt; };   // a 0 / 1 switch, with its default where it is not set
  const bool coupled = p->mode == TJ_MODE_MULTI_COUPLED, decoupled = p->mode == TJ_MODE_MULTI_DECOUPLE, one = p->world == 1;
  d.mode = p->mode; d.U = p->uav_num; d.P = p->piece_num; d.res = p->res; d.S = d.P * d.res; d.T = 3 * d.P + 3; d.N = 0; d.prim = 1;
  // the fused chain (k_linesearch leaves the hull cache, k_xsolve's tail the swept-hull cache) -- sharded contexts too since round 5: the other ranks' robots
  // are handled by foreign units inside k_front / k_ccd (Dev::xf).  Coupled mode keeps its own kernels (and, sharded, k_hullinfo / k_ccd_prep for all robots).
  d.fuse = !coupled ? 1 : 0;
  d.rank = p->rank; d.world = p->world;
  d.xf = (!one && d.fuse && decoupled) ? 1 : 0;
  // coupled mode, one context: every robot's cache records by units inside k_front / k_ccd (two launches less per iteration; TJ_COUPLED_UNITS=0: k_hullinfo / k_ccd_prep)
  if (coupled && one && flag(tune("COUPLED_UNITS"), 1)) { d.xf = 1; d.xf_all = 1; }
  d.u0 = (int)((long long)p->rank * d.U / p->world); d.u1 = (int)((long long)(p->rank + 1) * d.U / p->world);
  const int owned = std::max(1, d.u1 - d.u0), items = (d.u1 - d.u0) * d.P;   // robots / (robot, piece) blocks of this rank
  d.lambda = p->lambda; d.margin = p->margin; d.offset = p->offset; d.mu = p->mu; d.vel_limit = p->vel_limit; d.acc_limit = p->acc_limit;
  d.ks = p->ks; d.kt = p->kt; d.stop = p->stop;
  d.cap_obs = p->cap_obs > 0 ? p->cap_obs : 256;
  d.cap_self = p->cap_self > 0 ? p->cap_self : std::max(1, std::min(d.U - 1, 64));  // neighbours within offset + 2 margin of ONE segment; k_grad's LDS grows with it
  d.cap_pairs = p->cap_pairs > 0 ? p->cap_pairs : d.U;
  d.optimal_plane = p->optimal_plane ? 1 : 0;
  d.pair_rows = d.U <= 128 ? 8 : 16;   // tile height: 64 robots -- 8 rows: k_front 13.3 -> 12.5 us, k_ccd 9.6 -> 8.7 (with eight interval records in flight); 256 robots -- 16 rows (8: +1.3 us, 4: +13)
  if (const char* e = tune("PAIR_ROWS")) { const int r = atoi(e); if (r == 2 || r == 4 || r == 8 || r == 16) d.pair_rows = r; }
  d.cap_work = d.mode >= 1 ? (int)std::min<long long>((long long)d.S * d.U * (d.U - 1) / 2 + 1, 1 << 22) : 1;  // robot pairs per iteration
  d.xs = 3 * d.T + 4;
  const int n = 9 * d.P - 2;
  d.grad_npl = std::min(d.cap_obs + d.cap_self, 64);   // what a batch of segments really carries (SCN-C: <= 40); more goes through grad_scr.  64: five workgroups per CU (96: four)
  if (const char* e = tune("GRAD_NPL")) { const int r = atoi(e); if (r >= 8 && r <= 4096) d.grad_npl = std::min(d.cap_obs + d.cap_self, r); }
  h.lds_grad = grad_lds_doubles(d.grad_npl, d.res) * sizeof(double);
  const size_t lds_max = 160 * 1024 - 1024;
  // long trajectories: the dense per-robot system no longer fits LDS -> band storage (decoupled / single-UAV modes)
  d.xs_band = (xsolve_lds_doubles(n) * sizeof(double) > lds_max || tune("XS_BAND")) ? 1 : 0;
  h.lds_xs = (d.xs_band ? xsolve_band_lds_doubles(n) : xsolve_lds_doubles(n)) * sizeof(double);
  h.lds_xs2 = (d.xs_band ? (size_t)(n - 1) * BAND_BS + 5 * (size_t)n : (size_t)n * n + 4 * (size_t)n) * sizeof(double);   // k_xsolve_c2 / k_xsolve_c2_band
  h.lsl = ls_layout(d.S, d.T, d.P, 120 * 1024);
  h.lds_ls = h.lsl.total * sizeof(double);
  if (d.U > 2048) return fail("more than 2048 robots are not supported (pair keys pack robot ids into 11 bits; the dense [S][U][U] plane tables are 5.4 GB + 0.7 GB there)");
  if (d.S > 511) return fail("more than 511 segments per robot are not supported by the line-search kernel");
  if (d.res > GRAD_MAXRES) return fail("res > 16 segments per piece is not supported by the gradient kernel");
  d.seq_tree = (decoupled && SeqLayout(d.U, ACT_CAP, true).lds_bytes() <= lds_max) ? 1 : 0;
  if (tune("NO_SEQ_TREE")) d.seq_tree = 0;  // test hook: behave like a fleet too large for the LDS-resident tree
  h.lds_seq = SeqLayout(d.U, ACT_CAP, d.seq_tree != 0).lds_bytes();
  // hundreds of robots: the 512-thread folded k_grad is limited to ~2 workgroups per CU by wave slots; the 192-thread one (5 per CU)
  // plus a separate compaction launch is faster once there are more pieces than that (SCN-D: k_grad 109 -> 72 + 14 us)
  h.grad_fold = flag(tune("GRAD_FOLD"), items <= 512) != 0;
  // the BVH walk's two-level steps are decided when the obstacle set is known (set_obstacles); TJ_BVH_SKIP=0 / 1 forces it (launch-shape switch, same bits)
  if (const char* e = tune("BVH_SKIP")) { h.bvh_skip_forced = true; d.bvh_skip = atoi(e) != 0; }
  d.mid_order = flag(tune("MID_ORDER"), (d.mode >= 1 && d.U >= 192) ? 1 : 0);   // k_mid's grid order (kernels_step.h): config 5 -15 us; small fleets: nothing or slightly worse.  Launch-shape switch (same bits)
  d.pair_prio = flag(tune("PAIR_PRIO"), 1);   // launch-shape switch (same bits)
  d.pair_lpw = 64;
  if (const char* e = tune("PAIR_LPW")) { const int r = atoi(e); if (r == 8 || r == 16 || r == 32 || r == 64) d.pair_lpw = r; }   // launch-shape switch (same bits)
  d.pair_pass_on = flag(tune("PAIR_PASS_ON"), 1);
  // GJK head start for last iteration's slow robot pairs (kernels_pairs.h: spec_pair_body); TJ_PAIR_HEAD_START=0 switches it off (test hook: same bits)
  d.spec = (d.mode >= 1 && !d.optimal_plane) ? flag(tune("PAIR_HEAD_START"), 1) : 0;
  // k_ccd's last block finishes with the sequential pair replay + gnorm (kernels_step.h): decoupled mode, when the replay's small
  // arrays fit k_ccd's static LDS buffer with room for at least 256 acting-pair keys (the value is that capacity)
  if (decoupled || (coupled && one)) {   // (coupled: one context only -- a sharded one exports its obstacle-CCD exponents from k_ccd_self_seq)
    const size_t buf = sizeof(double) * (size_t)(CCD_LDS_DOUBLES > PAIR_LDS_DOUBLES ? CCD_LDS_DOUBLES : PAIR_LDS_DOUBLES);
    int cap = 4096;
    while (cap >= 256 && SeqLayout(d.U, cap, true).small_bytes > buf) cap >>= 1;
    if (cap >= 256 && CcdLayout(d).tiles() < 65536) d.seq_fold = cap;   // (the finisher counts the selection blocks in 16 bits)
  }
  if (!flag(tune("SEQ_FOLD"), 1)) d.seq_fold = 0;   // launch-shape switch (same bits)
  if (const char* e = tune("N_SOLVE")) h.n_solve_env = std::max(1, atoi(e));
  d.spec_budget = SPEC_GJK_BUDGET; d.spec_min = SPEC_GJK_MIN;
  if (const char* e = tune("HS_BUDGET")) d.spec_budget = std::max(1, atoi(e));   // development hooks (same bits for any value)
  if (const char* e = tune("HS_MIN")) d.spec_min = std::max(1, atoi(e));
  d.ls_fast = flag(tune("LS_FAST"), 1);   // launch-shape switch (same bits): round 0 of k_linesearch in the team shape
  d.num_cu = f.num_cu;
  // coupled mode: the four evaluation rounds of the Armijo search in one launch where a block per (robot, round) gets a compute unit of its own
  // (TJ_LSC_WIDE: launch-shape switch, same bits) ...
  h.lsc_wide = flag(tune("LSC_WIDE"), coupled && owned * LSC_ROUNDS <= d.num_cu) != 0;
  // ... and the corner solve inside k_xsolve where every robot's block is resident at once (one block per compute unit: 242 registers x 8 waves), dense storage
  d.c2_fold = (coupled && one && d.U <= d.num_cu && !d.xs_band) ? flag(tune("C2_FOLD"), 1) : 0;   // launch-shape switch (same bits)
  // k_grad's launch order follows the items' last durations where blocks outnumber the compute units (kernels_newton.h: grad_order_body)
  // -- between one and two blocks per unit, the case it was measured on: SCN-C -1.5 us per iteration, the 64 hard robots -1.4; at five blocks per unit
  // (256 robots) longest-first ordering bought nothing in k_grad and the run was 1.5 % slower, so larger fleets keep the identity
  d.grad_bal = (owned * d.P > d.num_cu && owned * d.P < 2 * d.num_cu) ? 1 : 0;
  // asynchronous Newton solve (dev_common.h, Dev::xs_async): one context, decoupled / single-UAV chain with the swept-hull tail in k_xsolve.  TJ_XS_ASYNC=0: the
  // solve stays a link of the one-queue chain (launch-shape switch: same bits)
  d.xs_async = (one && !d.xs_band && (!coupled ? d.fuse != 0 : (d.c2_fold && d.xf_all))) ? 1 : 0;   // (coupled chain: with the corner solve in k_xsolve and k_ccd's units building the records already;
                                                                                                       //  sharded contexts keep the one-queue chain: tried in round 5, a tj_group of two ranks aborted -- not pursued)
  if (d.xs_async) {
    // Liveness: k_xsolve's blocks hold registers and LDS while they sleep on their tickets, and the k_grad blocks that hand the tickets out may still be waiting
    // for a compute unit.  Safe when the sleepers can never shut k_grad out: at most half as many robots as compute units (half the device stays free whatever
    // the dispatcher does), or at most one robot per unit AND a k_grad block fits a unit next to one k_xsolve block (a unit with two sleepers then implies a
    // unit with none).  Larger fleets keep the solve on the chain's queue (1 500 robots: the sleepers filled the device and every wait ran into its 5 ms limit).
    bool fits = false;
    const KernelFact &ax = f.xsolve, &ag = f.grad[h.grad_fold ? 1 : 0];
    if (ax.ok && ag.ok) {
      auto gran = [](int r) { return (r + 7) / 8 * 8; };
      const int wx = XS_LOAD_THREADS / 64, wg = (h.grad_fold ? GRAD_FOLD_THREADS : GRAD_THREADS) / 64;
      const size_t lx = h.lds_xs + (size_t)ax.lds, lg = h.lds_grad_of(h.grad_fold, d.res) + (size_t)ag.lds;
      fits = ((wx + 3) / 4) * gran(ax.regs) + ((wg + 3) / 4) * gran(ag.regs) <= 512 && lx + lg <= (size_t)160 * 1024 && (wx + 3) / 4 + (wg + 3) / 4 <= 8;
    }
    if (!(2 * owned <= d.num_cu || (owned <= d.num_cu && fits))) d.xs_async = 0;
  }
  // rocprofv3's counter collection (--pmc) serialises the dispatches of ALL queues, in an order of its own: a gate held back behind the kernel it waits for would run every
  // wait into its 2 s limit.  Under it the context keeps everything on the one queue (an explicit TJ_XS_ASYNC=1 / TJ_KEEP_ASYNC=1 overrides).
  const char* const e_xs = tune("XS_ASYNC");
  const char* const e_keep = tune("KEEP_ASYNC");
  const bool xs_on = e_xs ? atoi(e_xs) != 0 : !f.counters_on, keep_on = e_keep ? atoi(e_keep) != 0 : !f.counters_on;
  d.xs_async = d.xs_async && xs_on;
  // asynchronous plane refinement ("optimal_plane":1, multi-UAV decoupled mode, one context; TJ_KEEP_ASYNC=0: k_keep stays one launch between k_mid and k_grad -- same bits)
  d.keep_async = (d.optimal_plane && decoupled && one && keep_on) ? 1 : 0;
  d.keep_waves = 1024;
  // Hardware queues.  HIP maps a process's streams onto GPU_MAX_HW_QUEUES (4) hardware queues per device and lets further streams SHARE them; a gate kernel that sleeps at the
  // head of a shared queue keeps back whatever another context put behind it -- possibly the very kernel a gate of THAT context, asleep on a queue of this one, waits for:
  // measured with three default contexts in one process, two of them ran into the 2 s limit (and healed themselves).  So the contexts of a process that sleep across queues
  // claim their streams (main + second + third) out of a per-device budget of GPU_MAX_HW_QUEUES - 1 (the null stream has one); a context that does not fit keeps the one-queue
  // chain (same bits).  An explicit TJ_XS_ASYNC=1 / TJ_KEEP_ASYNC=1 overrides; self-healing stays the net under it.
  h.queues = 1 + d.xs_async + d.keep_async;
  h.forced = (e_xs && atoi(e_xs) != 0) || (e_keep && atoi(e_keep) != 0);
  if (f.claim_refused) { d.xs_async = 0; d.keep_async = 0; h.hwq_refused = true; }
  h.xs_two_queues = d.xs_async && tune("XS_ONE_QUEUE") == nullptr;   // (TJ_XS_ONE_QUEUE: the tickets and flags on the chain's queue)
  h.keep_two_queues = d.keep_async != 0;
  if (const char* e = tune("GRAD_BALANCE")) d.grad_bal = (atoi(e) != 0 && owned * d.P <= 65536) ? 1 : 0;   // launch-shape switch (same bits)
  if (const char* e = tune("LS_HELP")) { h.ls_help_forced = true; h.ls_help_asked = atoi(e); }
  d.ls_help = plan_ls_help(d, h, d.num_cu);
  if (const char* e = tune("LS_HELP_LATE")) d.ls_help_late = std::max(0, std::min(4000, atoi(e)));   // test hook (same bits): helper blocks idle that many microseconds before staging
  d.ls_help_mute = flag(tune("LS_HELP_MUTE"), 0);                                                          // test hook (same bits): the helpers never post, the primaries time out
  // asynchronous front (dev_common.h, Dev::fa): one context, decoupled mode, the asynchronous solve's second queue, and a k_linesearch grid that is resident all at once
  // (one block per compute unit at most -- the residency gate's premise).  TJ_FRONT_ASYNC=0: k_linesearch publishes the hull cache and k_front follows it on the chain's queue (same bits)
  d.fa = (d.xs_async && one && !d.optimal_plane &&
          (!coupled ? (d.fuse && owned * d.ls_help <= d.num_cu) : (h.lsc_wide && d.xf_all && owned * LSC_ROUNDS <= d.num_cu))) ? flag(tune("FRONT_ASYNC"), 1) : 0;   // (coupled: the one-launch search, whose last block commits every robot)
  h.fa_emulate = flag(tune("FRONT_ASYNC_ONE_QUEUE"), 0) != 0;   // the asynchronous front's data flow (k_front's units form the records, k_linesearch publishes none) on the chain's queue: counter passes
  if (d.fa) {
    // Dev::fa_mid: k_mid may start while k_front still runs only if k_front's whole grid is resident before k_mid's first wave is -- the last k_linesearch block waits
    // until every k_front block has started, so the grid must fit the device next to that one block: blocks per compute unit by LDS, registers and wave slots
    h.fa_mid_front = plan_grids(d, h.n_solve_env).n_front;
    if (f.front.ok) {
      const int by_lds = (int)(((size_t)160 * 1024) / std::max<size_t>((size_t)f.front.lds, 1)), by_regs = 4 * (512 / std::max((f.front.regs + 7) / 8 * 8, 8)), per_cu = std::min(std::min(by_lds, by_regs), 32);
      h.fa_mid_ok = (long long)h.fa_mid_front <= (long long)(d.num_cu - 1) * per_cu;
    }
    h.fa_mid_ok = h.fa_mid_ok && flag(tune("FRONT_ASYNC_MID"), 1);   // launch-shape switch (same bits): 0 = k_linesearch waits for k_front's end, k_mid follows plainly
  }
  h.heal = flag(tune("HEAL"), 1) != 0;
  if (const char* e = tune("XS_FAULT")) h.xs_fault = atoi(e);
  if (h.lds_grad_of(true, d.res) > lds_max || h.lds_xs > lds_max || h.lds_ls > lds_max || h.lds_seq > lds_max)
    return fail("problem does not fit the 160 KB LDS of one CU (segments per robot / fleet size too large for this version)");
  return pl;
}

#ifdef TJ_KAT
// the plan as a flat record of ints (test hook tj_kat_plan; the names are PLAN_FIELDS of the Python package, in this order)
inline int plan_record(const Plan& pl, const PlanFacts& f, int* out, int cap) {
  const Dev& d = pl.d; const HostPlan& h = pl.h;
  const Grids g = plan_grids(d, h.n_solve_env);
  const int v[] = {
    pl.err, d.mode, d.U, d.P, d.res, d.S, d.T, d.N, d.prim, d.u0, d.u1, d.rank, d.world, d.fuse, d.xf, d.xf_all, d.cap_obs, d.cap_self, d.cap_pairs, d.optimal_plane,
    d.pair_rows, d.cap_work, d.xs, d.grad_npl, d.xs_band, d.seq_tree, d.bvh_skip, d.pair_prio, d.mid_order, d.pair_lpw, d.pair_pass_on, d.spec, d.seq_fold, d.spec_budget,
    d.spec_min, d.ls_fast, d.num_cu, d.c2_fold, d.grad_bal, d.xs_async, d.keep_async, d.keep_waves, d.ls_help, d.ls_help_late, d.ls_help_mute, d.fa,
    h.grad_fold, h.n_solve_env, h.lsc_wide, h.fa_emulate, h.fa_mid_ok, h.fa_mid_front, h.hwq_refused, h.queues, h.forced, h.xs_two_queues, h.keep_two_queues, h.heal, h.xs_fault,
    (int)h.lds_grad, (int)h.lds_xs, (int)h.lds_xs2, (int)h.lds_ls, (int)h.lds_seq, (int)h.lsl.total, h.lsl.plane_cap, h.lsl.affine, h.lsl.groups,
    g.n_rows, g.n_ccd, g.n_xf, g.n_front, g.n_solve, g.n_obs_solve, g.n_mid_slack};
  const int nv = (int)(sizeof(v) / sizeof(int)), n = PLAN_FACT_INTS + nv;
  if (cap < n) return -n;
  memcpy(out, &f, sizeof(f)); memcpy(out + PLAN_FACT_INTS, v, sizeof(v));
  return n;
}
#endif

}  // namespace tj
