// cli_main.cpp -- `admmPathPlanning3D <mesh>` (-DTJ_CLI_SINGLE) and `multiPathPlanning3D <mesh>`
// (-DTJ_CLI_MULTI): the headless branches of the reference mains
// (Main/admmPathPlanning3D.cpp:355-547, Main/multiPathPlanning3D.cpp:470-695) with the per-iteration
// call replaced by the C ABI of libtrajadmm.so.  Same working-directory layout, same config keys,
// same result file.  `init:2` plans the way points with the library's device planner instead of OMPL,
// `decouple:0` selects the coupled multi-robot mode (one shared piece_time, Main/multiPathPlanning3D.cpp:674-677),
// `optimal_plane:1` the persistent-plane branch.  The GUI (`gui:1`) is outside the accelerated path and is rejected
// with a message instead of being silently ignored.  On convergence the trajectory duration and sampled arc length are printed
// like the mains' log_data ("ccd time:", "ccd len:").
//
// Extras (ours): --max-iter N, --dump-state FILE (control points; the reference never writes the
// trajectory), --sample-traj FILE (positions sampled like log_data, one "uav t x y z" per line),
// --batch N iterations per device batch (the stop test runs on the device before every iteration),
// --triangles (or the optional key "triangles":1 in 3D.json): obstacles are the TRIANGLES of the OBJ (`f` lines, tj_set_mesh)
// instead of its vertices as a point cloud.
// --audit [RANGE]: after the run (and after the "ccd len:" lines) one line per robot from tj_audit / tj_group_audit -- obstacle and robot-pair clearance
// (searched up to RANGE; default offset + 2 * margin), peak speed and acceleration, duration, flag word.  The result file is unchanged.
// --audit-timed [LEVELS]: after the --audit lines one line per robot from tj_audit_timed / tj_group_audit_timed -- the bracket of the closest approach to another robot at
// equal flight times (default range; LEVELS 0..6, default the library's), the partner / segment / time of its upper end, where its lower end lies, level, flag word.
// --closest-approach [TOL]: after the --audit-timed lines one line per robot from tj_closest_approach / tj_group_closest_approach -- the closest approach to another robot at
// equal flight times converged to TOL (default the library's; default range), its partner / segment / time, rounds, windows evaluated, flag word -- and a fleet summary
// (smallest hi, who, when, any contact).
// --obstacle-approach [TOL]: after the --closest-approach lines one line per robot from tj_obstacle_approach / tj_group_obstacle_approach -- the flown curve's closest
// approach to an obstacle primitive converged to TOL (default the library's; default range), the primitive / segment / time, rounds, items evaluated, flag word -- and a
// fleet summary (smallest hi, who, which primitive, when, any contact).  Works in the single-UAV main too.
// --obstacle-windows [DIST]: after the --obstacle-approach lines one line per row of tj_obstacle_windows / tj_group_obstacle_windows, sorted by (robot, start) -- every
// time interval in which a robot's flown curve is not certified farther than DIST (default `offset`) from the obstacles: the brackets of the first and the last
// time within DIST, the seconds certified within, the smallest attained sample with its time and primitive, the segments of the ends, leaves, rounds, windows
// evaluated, flag word -- and the fleet's line: rows, rows with a sure time, grazes, seconds certified within.  Works in the single-UAV main too.
// --pair-approach [TOL]: after the --obstacle-windows lines one line per LISTED directed robot pair from tj_pair_approach / tj_group_pair_approach, sorted by (robot,
// partner) -- every pair that comes within the default range at equal flight times, its closest approach converged to TOL (default the library's), segment / time,
// rounds, windows evaluated, flag word -- and the counts of pairs in contact, undecided and clear.
// --path-crossings [TOL]: after the --pair-approach lines one line per LISTED unordered robot pair from tj_path_crossings / tj_group_path_crossings, sorted by (robot,
// partner) -- every pair whose PATHS come within the default range in space, whatever the time: the bracket converged to TOL (default the library's), for each
// of the two robots segment / parameter / time of the closest sample, rounds, windows evaluated, flag word -- and the counts of pairs separated by timing only
// (contact in space), undecided and separated in space.
// --timing-margin [TOL]: after the --path-crossings lines one line per LISTED unordered robot pair from tj_timing_margin / tj_group_timing_margin, sorted by (robot,
// partner) -- every pair whose paths come within `offset` under some slip of the timetable: the slip's bracket in seconds converged to TOL (default the
// library's), the distance of the hi sample, for each of the two robots its segment / parameter / clock value, rounds, windows evaluated, flag word -- and the
// fleet's line: pairs listed, in contact on the timetable, with a certified positive margin, and the smallest hi.
// --proximity-windows [DIST]: after the --timing-margin lines one line per row of tj_proximity_windows / tj_group_proximity_windows, sorted by (robot, partner, start) --
// every time interval in which a directed robot pair is not certified farther than DIST apart (default `offset`) at equal flight times: the brackets of the first
// and the last time within DIST, the seconds certified within, the smallest attained sample and its time, leaves, rounds, windows evaluated, flag word -- and the
// fleet's line: listed pairs, rows, rows with a sure time, grazes, seconds certified within.
// --flight-profile K [FILE]: after the --proximity-windows lines K lines per robot from tj_flight_profile / tj_group_flight_profile on the grid t_k = (k / (K - 1)) * the
// longest robot's duration (K == 1: t = 0) -- "profile uav t x y z d_obs idx d_robot partner speed accel flags" at 17 digits: position, distance and index of the
// NEAREST obstacle primitive (no range), distance and index of the nearest other robot at the same time, speed, acceleration, flag word.  With FILE the lines go
// there instead, without the leading word (the layout of --sample-traj, extended).  Works in the single-UAV main and with --gpus.
// --peak-dynamics [TOL]: after the --flight-profile lines one line per robot from tj_peak_dynamics / tj_group_peak_dynamics -- the flown curve's peak speed, acceleration
// and jerk converged to the relative TOL (default the library's), each with its time, the path length's bracket, duration, time_scale, flag word -- and a fleet line with
// the largest time_scale and its robot.  Works in the single-UAV main and with --gpus.
// --dynamics-windows [FRACTION]: after the --peak-dynamics lines one line per row from tj_dynamics_windows / tj_group_dynamics_windows at the two default gates scaled --
// speed ABOVE FRACTION * vel_limit and acceleration ABOVE FRACTION * acc_limit, FRACTION default 1 -- "dynwin uav gate quantity sense first lo hi last lo hi within
// extreme time seg a b leaves depth windows flags" at 17 digits, and the fleet's line: rows, rows with a sure time, grazes, seconds certified over the level.
// Works in the single-UAV main and with --gpus.
// --zone-windows [LEVEL] with repeatable --zone-box X0 Y0 Z0 X1 Y1 Z1, --zone-ball X Y Z R and --zone-outside (applies to the zones after it): after the
// --dynamics-windows lines one line per row from tj_zone_windows / tj_group_zone_windows -- the time intervals in which a robot is inside (or outside) each zone at
// LEVEL (default 0, the zone itself), zones in solver units in the order given -- "zonewin uav zone sense face first lo hi last lo hi within extreme time seg a b
// leaves depth windows flags" at 17 digits, and the fleet's line: zones, rows, rows with a sure time, grazes, seconds certified within.  Works in the single-UAV main
// and with --gpus.
// --gpus N / --devices a,b,.. (multi-UAV main only): the robots are sharded over N devices by the library (tj_group, trajadmm.h);
// the trajectory is bitwise the one-device one.
#include <cctype>
#include <chrono>
#include <sstream>
#include "../../include/trajadmm.h"
#include "cli_common.h"

#if defined(TJ_CLI_MULTI)
static const bool kMulti = true;
#else
static const bool kMulti = false;
#endif

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "Syntax: " << argv[0] << " <mesh file> [--max-iter N] [--batch N] [--dump-state FILE] [--sample-traj FILE] [--triangles] [--audit [RANGE]] [--audit-timed [LEVELS]] [--closest-approach [TOL]] [--obstacle-approach [TOL]] [--obstacle-windows [DIST]] [--sight-windows [DIST]] [--sight-station X Y Z].. [--pair-approach [TOL]] [--path-crossings [TOL]] [--timing-margin [TOL]] [--proximity-windows [DIST]] [--flight-profile K [FILE]] [--peak-dynamics [TOL]] [--dynamics-windows [FRACTION]] [--zone-windows [LEVEL]] [--zone-box X0 Y0 Z0 X1 Y1 Z1].. [--zone-ball X Y Z R].. [--zone-outside] [--gpus N | --devices a,b,..]" << std::endl; return -1; }
  const std::string mesh = argv[1];
  long max_iter = 1000000; int batch = 8; std::string dump, sample_file; bool triangles = false;
  bool audit = false; double audit_range = 0;
  bool audit_timed = false; int audit_levels = -1;
  bool closest = false; double closest_tol = -1;
  bool obstacle = false; double obstacle_tol = -1;
  bool obswin = false; double obswin_dist = 0;
  bool sight = false; double sight_dist = 0; std::vector<double> sight_stations;   // (stations in solver units)
  bool pairs = false; double pairs_tol = -1;
  bool crossings = false; double crossings_tol = -1;
  bool margins = false; double margins_tol = -1;
  bool proximity = false; double proximity_dist = 0;
  int profile_samples = 0; std::string profile_file;
  bool dynamics = false; double dynamics_tol = -1;
  bool dynwin = false; double dynwin_fraction = 1;
  bool zonewin = false; double zonewin_level = 0; tjcli::ZoneList zone_list;   // (zones in solver units)
  std::vector<int> devices;   // empty: one context on device 0
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i];
    if (a == "--max-iter" && i + 1 < argc) max_iter = atol(argv[++i]);
    else if (a == "--batch" && i + 1 < argc) batch = atoi(argv[++i]);
    else if (a == "--dump-state" && i + 1 < argc) dump = argv[++i];
    else if (a == "--sample-traj" && i + 1 < argc) sample_file = argv[++i];
    else if (a == "--triangles") triangles = true;
    else if (a == "--audit") { audit = true; if (i + 1 < argc && argv[i + 1][0] != '-') audit_range = atof(argv[++i]); }
    else if (a == "--audit-timed") { audit_timed = true; if (i + 1 < argc && argv[i + 1][0] != '-') audit_levels = atoi(argv[++i]); }
    else if (a == "--closest-approach") { closest = true; if (i + 1 < argc && argv[i + 1][0] != '-') closest_tol = atof(argv[++i]); }
    else if (a == "--obstacle-approach") { obstacle = true; if (i + 1 < argc && argv[i + 1][0] != '-') obstacle_tol = atof(argv[++i]); }
    else if (a == "--obstacle-windows") { obswin = true; if (i + 1 < argc && argv[i + 1][0] != '-') obswin_dist = atof(argv[++i]); }
    else if (a == "--sight-windows") { sight = true; if (i + 1 < argc && argv[i + 1][0] != '-') sight_dist = atof(argv[++i]); }
    else if (a == "--sight-station" && i + 3 < argc) { for (int k = 0; k < 3; k++) sight_stations.push_back(atof(argv[++i])); }
    else if (a == "--pair-approach") { pairs = true; if (i + 1 < argc && argv[i + 1][0] != '-') pairs_tol = atof(argv[++i]); }
    else if (a == "--path-crossings") { crossings = true; if (i + 1 < argc && argv[i + 1][0] != '-') crossings_tol = atof(argv[++i]); }
    else if (a == "--timing-margin") { margins = true; if (i + 1 < argc && argv[i + 1][0] != '-') margins_tol = atof(argv[++i]); }
    else if (a == "--proximity-windows") { proximity = true; if (i + 1 < argc && argv[i + 1][0] != '-') proximity_dist = atof(argv[++i]); }
    else if (a == "--flight-profile" && i + 1 < argc) { profile_samples = atoi(argv[++i]); if (i + 1 < argc && argv[i + 1][0] != '-') profile_file = argv[++i]; if (profile_samples < 1) { std::cerr << "--flight-profile needs K >= 1" << std::endl; return -1; } }
    else if (a == "--peak-dynamics") { dynamics = true; if (i + 1 < argc && argv[i + 1][0] != '-') dynamics_tol = atof(argv[++i]); }
    else if (a == "--dynamics-windows") { dynwin = true; if (i + 1 < argc && argv[i + 1][0] != '-') dynwin_fraction = atof(argv[++i]); }
    else if (a == "--zone-windows") { zonewin = true; if (i + 1 < argc && (argv[i + 1][0] != '-' || isdigit((unsigned char)argv[i + 1][1]) || argv[i + 1][1] == '.')) zonewin_level = atof(argv[++i]); }
    else if (a == "--zone-box" && i + 6 < argc) { double v[6]; for (int k = 0; k < 6; k++) v[k] = atof(argv[++i]); zone_list.box(v); }
    else if (a == "--zone-ball" && i + 4 < argc) { double v[4]; for (int k = 0; k < 4; k++) v[k] = atof(argv[++i]); zone_list.ball(v); }
    else if (a == "--zone-outside") zone_list.sense = TJ_ZONE_OUTSIDE;
    else if (a == "--gpus" && i + 1 < argc) { const int n = atoi(argv[++i]); devices.clear(); for (int k = 0; k < n; k++) devices.push_back(k); }
    else if (a == "--devices" && i + 1 < argc) { devices.clear(); std::stringstream ss(argv[++i]); std::string t; while (std::getline(ss, t, ',')) devices.push_back(atoi(t.c_str())); }
    else { std::cerr << "unknown argument " << a << std::endl; return -1; }
  }
  tj_ctx* ctx = nullptr;
  tj_group* grp = nullptr;
  if (!kMulti && devices.size() > 1) { std::cerr << "error: a single UAV does not shard over devices" << std::endl; return 1; }
  try {
    auto j = tjcli::read_flat_json("Config_File/3D.json");
    const double lambda = tjcli::need(j, "lambda"), margin = tjcli::need(j, "margin"), offset = tjcli::need(j, "offset");
    const double mu = tjcli::need(j, "mu"), stop = tjcli::need(j, "stop"), vel = tjcli::need(j, "vel_limit"), acc = tjcli::need(j, "acc_limit");
    const int res = (int)tjcli::need(j, "res"), init = (int)tjcli::need(j, "init"), gui = (int)tjcli::need(j, "gui");
    const int optimal_plane = (int)tjcli::need(j, "optimal_plane"), if_exit = (int)tjcli::need(j, "exit"), init_ob = (int)tjcli::need(j, "init_ob");
    tjcli::need(j, "auto"); tjcli::need(j, "epsilon");
    const int decouple = (int)tjcli::need(j, "decouple");
    (void)if_exit;
    if (gui) throw std::runtime_error("gui:1 is not part of the accelerated path (use gui:0)");
    if (init != 1 && init != 2) throw std::runtime_error("init must be 1 (init/<mesh>_init_file.txt) or 2 (plan way points from start/goal pairs)");

    if (j.count("triangles") && j["triangles"] != 0) triangles = true;   // optional key (ours); the 16 reference keys stay mandatory
    const std::string model = std::string(kMulti ? "model/multiple/" : "model/single/") + mesh;
    std::vector<double> V; std::vector<int> F;
    if (triangles) tjcli::read_obj_mesh(model, V, F); else V = tjcli::read_obj_vertices(model);
    int U = 1, P = 0; std::vector<double> wp;
    if (kMulti) for (double& x : V) x *= 5;  // Main/multiPathPlanning3D.cpp:107
    const int N = init_ob ? (int)(triangles ? F.size() / 3 : V.size() / 3) : 0;
    auto set_obstacles = [&](tj_ctx* c) { return triangles ? tj_set_mesh(c, V.data(), (int)(V.size() / 3), F.data(), N) : tj_set_cloud(c, V.data(), N); };
    if (init == 1) {
      tjcli::read_waypoints("init/" + mesh + "_init_file.txt", kMulti, U, P, wp);
      if (kMulti) for (double& x : wp) x *= 5;  // :536
    } else {
      // "init":2 -- ompl_init (Main/multiPathPlanning3D.cpp:205-340, Main/admmPathPlanning3D.cpp:190-247) without OMPL: the
      // device planner of the library, in solver units, writing init/<mesh>_init_file.txt like the reference does
      std::vector<double> starts, goals;
      tjcli::read_start_goal("init/" + mesh + "_start_goal.txt", kMulti, starts, goals);
      U = (int)starts.size() / 3;
      tj_params pp; tj_ctx* pc = nullptr;
      tj_default_params(&pp, kMulti ? TJ_MODE_MULTI_DECOUPLE : TJ_MODE_SINGLE, U, 2);
      pp.margin = margin; pp.offset = offset;
      auto pchk = [&](int rc, const char* what) { if (rc < 0) { std::string m = std::string(what) + ": " + tj_last_error(pc); if (pc) tj_destroy(pc); throw std::runtime_error(m); } };
      pchk(tj_create(&pp, &pc), "tj_create");
      pchk(set_obstacles(pc), "tj_set_cloud / tj_set_mesh");
      const int cap = 256; int nw = 0;
      std::vector<double> buf((size_t)U * cap * 3);
      pchk(tj_plan_init(pc, U, starts.data(), goals.data(), 0.0, 0, 0, cap, buf.data(), &nw), "tj_plan_init");
      tj_destroy(pc);
      P = nw - 1;
      wp.assign((size_t)U * nw * 3, 0.0);
      for (int u = 0; u < U; u++) for (int k = 0; k < nw * 3; k++) wp[(size_t)u * nw * 3 + k] = buf[(size_t)u * cap * 3 + k];
      std::ofstream f("init/" + mesh + "_init_file.txt");   // one line per way point, all robots side by side (:324-333)
      for (int k = 0; k < nw; k++) { for (int u = 0; u < U; u++) for (int a = 0; a < 3; a++) f << wp[((size_t)u * nw + k) * 3 + a] << " "; f << std::endl; }
      std::cout << "ompl end\n";
    }
    if (kMulti) std::cout << "uav_num: " << U << "\n";
    std::cout << "time_obstacle build: " << N << (triangles ? " triangles" : " points") << std::endl;

    tj_params p;
    tj_default_params(&p, kMulti ? (decouple ? TJ_MODE_MULTI_DECOUPLE : TJ_MODE_MULTI_COUPLED) : TJ_MODE_SINGLE, U, P);
    p.optimal_plane = optimal_plane ? 1 : 0;  // persistent planes refined by Optimal_plane::optimal_cd / self_optimal_cd
    p.res = res; p.lambda = lambda; p.margin = margin; p.offset = offset; p.mu = mu; p.vel_limit = vel; p.acc_limit = acc; p.stop = stop;
    auto chk = [&](int rc, const char* what) { if (rc < 0) throw std::runtime_error(std::string(what) + ": " + (grp ? tj_group_last_error(grp) : tj_last_error(ctx))); };
    const bool group = devices.size() > 1;
    if (group) {
      if (tj_group_create(&p, (int)devices.size(), devices.data(), &grp) < 0) throw std::runtime_error(std::string("tj_group_create: ") + tj_group_last_error(nullptr));
      chk(triangles ? tj_group_set_mesh(grp, V.data(), (int)(V.size() / 3), F.data(), N) : tj_group_set_cloud(grp, V.data(), N), "tj_group_set_cloud / tj_group_set_mesh");
      chk(tj_group_init_state(grp, wp.data(), 20.0), "tj_group_init_state");
      std::cout << "devices: " << devices.size() << std::endl;
    } else {
      if (devices.size() == 1) p.device = devices[0];
      chk(tj_create(&p, &ctx), "tj_create");
      chk(set_obstacles(ctx), "tj_set_cloud / tj_set_mesh");
      chk(tj_init_state(ctx, wp.data(), 20.0), "tj_init_state");  // piece_time = 20 (admmPathPlanning3D.cpp:482)
    }
    auto get_state = [&](int u, double* s, double* pt) { return group ? tj_group_get_state(grp, u, s, nullptr, nullptr, nullptr, nullptr, pt) : tj_get_state(ctx, u, s, nullptr, nullptr, nullptr, nullptr, pt); };

    std::ofstream result("result/" + mesh + (kMulti ? "_result_file_multi.txt" : "_result_file_admm.txt"));
    double whole_ms = 0, gnorm = 1;
    int iter = 0, converged = 0;
    while (iter < max_iter && !converged) {
      const int n = (int)std::min<long>(batch, max_iter - iter);
      auto t0 = std::chrono::steady_clock::now();
      chk(group ? tj_group_iterate(grp, n, &gnorm, &iter, &converged) : tj_iterate(ctx, n, &gnorm, &iter, &converged), "tj_iterate");
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      whole_ms += ms;
      std::cout << "iter: " << iter << "\n" << "gnorm: " << gnorm << "\n" << "time:" << ms << std::endl;
    }
    if (converged) {
      result << "iter: " << iter << std::endl;
      result << "running time: " << whole_ms << std::endl;
      result << "point cloud size: " << V.size() / 3 << std::endl;
    }
    if (converged || !sample_file.empty()) {
      // log_data (Main/admmPathPlanning3D.cpp:33-77 called at :513; Main/multiPathPlanning3D.cpp:33-77 at :644-648).
      // Deviation: the multi main passes the never-updated global piece_time (20) in decoupled mode; each robot's
      // own piece_time is used here.
      const int T = 3 * P + 3;
      std::vector<double> conv((size_t)P * 36), s(3 * T);
      tj_host_tables(P, res, conv.data(), nullptr, nullptr, nullptr);
      std::ofstream sf;
      if (!sample_file.empty()) { sf.open(sample_file); sf.precision(17); }
      const double dt = kMulti ? 0.1 : 0.05;
      double whole_len = 0;
      for (int u = 0; u < U; u++) {
        double pt = 0, tt = 0, len = 0;
        chk(get_state(u, s.data(), &pt), "tj_get_state");
        std::vector<double> smp;
        tjcli::log_data(s.data(), P, conv.data(), pt, dt, tt, len, sample_file.empty() ? nullptr : &smp);
        std::cout << "ccd time:" << tt << std::endl << "ccd len:" << len << std::endl;
        whole_len += len;
        for (size_t k = 0; k + 2 < smp.size(); k += 3) sf << u << " " << (k / 3) * dt << " " << smp[k] << " " << smp[k + 1] << " " << smp[k + 2] << "\n";
      }
      (void)whole_len;
    }
    if (audit) {
      std::vector<tj_audit_robot> rec(U);
      chk(group ? tj_group_audit(grp, audit_range, rec.data(), nullptr, nullptr) : tj_audit(ctx, audit_range, rec.data(), nullptr, nullptr), "tj_audit");
      tjcli::print_audit(rec);
    }
    if (audit_timed) {
      std::vector<tj_audit_timed_robot> rec(U);
      chk(group ? tj_group_audit_timed(grp, 0.0, audit_levels, rec.data(), nullptr, nullptr) : tj_audit_timed(ctx, 0.0, audit_levels, rec.data(), nullptr, nullptr), "tj_audit_timed");
      tjcli::print_audit_timed(rec);
    }
    if (closest) {
      std::vector<tj_closest_robot> rec(U);
      chk(group ? tj_group_closest_approach(grp, 0.0, closest_tol, -1, 0, rec.data()) : tj_closest_approach(ctx, 0.0, closest_tol, -1, 0, rec.data()), "tj_closest_approach");
      tjcli::print_closest_approach(rec);
    }
    if (obstacle) {
      std::vector<tj_obstacle_robot> rec(U);
      chk(group ? tj_group_obstacle_approach(grp, 0.0, obstacle_tol, -1, 0, rec.data()) : tj_obstacle_approach(ctx, 0.0, obstacle_tol, -1, 0, rec.data()), "tj_obstacle_approach");
      tjcli::print_obstacle_approach(rec);
    }
    if (obswin) {
      std::vector<tj_obswin_row> rows;
      chk(tjcli::listed_rows([&](tj_obswin_row* out, int cap, int* n) {
            return group ? tj_group_obstacle_windows(grp, obswin_dist, -1.0, -1, 0, out, cap, n) : tj_obstacle_windows(ctx, obswin_dist, -1.0, -1, 0, out, cap, n); }, rows), "tj_obstacle_windows");
      tjcli::print_obstacle_windows(rows);
    }
    if (sight) {
      const int n_stations = (int)sight_stations.size() / 3;
      const std::vector<int> links = tjcli::sight_links(U, n_stations);
      const int n_links = (int)links.size() / 2;
      std::vector<tj_sight_row> rows;
      chk(tjcli::listed_rows([&](tj_sight_row* out, int cap, int* n) {
            return group ? tj_group_sight_windows(grp, links.data(), n_links, sight_stations.data(), n_stations, sight_dist, -1.0, -1, 0, out, cap, n)
                         : tj_sight_windows(ctx, links.data(), n_links, sight_stations.data(), n_stations, sight_dist, -1.0, -1, 0, out, cap, n); }, rows), "tj_sight_windows");
      tjcli::print_sight_windows(rows, n_links);
    }
    if (pairs) {
      std::vector<tj_pair_record> rows;
      chk(tjcli::listed_rows([&](tj_pair_record* out, int cap, int* n) {
            return group ? tj_group_pair_approach(grp, 0.0, pairs_tol, -1, 0, out, cap, n) : tj_pair_approach(ctx, 0.0, pairs_tol, -1, 0, out, cap, n); }, rows), "tj_pair_approach");
      tjcli::print_pair_approach(rows);
    }
    if (crossings) {
      std::vector<tj_crossing_record> rows;
      chk(tjcli::listed_rows([&](tj_crossing_record* out, int cap, int* n) {
            return group ? tj_group_path_crossings(grp, 0.0, crossings_tol, -1, 0, out, cap, n) : tj_path_crossings(ctx, 0.0, crossings_tol, -1, 0, out, cap, n); }, rows), "tj_path_crossings");
      tjcli::print_path_crossings(rows);
    }
    if (margins) {
      std::vector<tj_margin_record> rows;
      chk(tjcli::listed_rows([&](tj_margin_record* out, int cap, int* n) {   // (default dist and max_slip)
            return group ? tj_group_timing_margin(grp, 0.0, 0.0, margins_tol, -1, 0, out, cap, n) : tj_timing_margin(ctx, 0.0, 0.0, margins_tol, -1, 0, out, cap, n); }, rows), "tj_timing_margin");
      tjcli::print_timing_margin(rows);
    }
    if (proximity) {
      std::vector<tj_proximity_row> rows;
      int n_pairs = 0;
      chk(tjcli::proximity_windows_rows([&](double r, double t, int d, int w, tj_proximity_row* out, int cap, int* np, int* n) {
            return group ? tj_group_proximity_windows(grp, r, t, d, w, out, cap, np, n) : tj_proximity_windows(ctx, r, t, d, w, out, cap, np, n); }, proximity_dist, rows, n_pairs), "tj_proximity_windows");
      tjcli::print_proximity_windows(rows, n_pairs);
    }
    if (profile_samples > 0) {
      // the grid: K equal steps over the longest robot's duration, log_data's sum of piece_num times piece_time
      const int K = profile_samples;
      double longest = 0;
      for (int u = 0; u < U; u++) {
        double pt = 0, dur = 0;
        chk(get_state(u, nullptr, &pt), "tj_get_state");
        for (int i = 0; i < P; i++) dur += 1.0 * pt;
        longest = std::max(longest, dur);
      }
      std::vector<double> times(K);
      for (int k = 0; k < K; k++) times[k] = K > 1 ? (k / (double)(K - 1)) * longest : 0.0;
      std::vector<tj_profile_sample> rec((size_t)U * K);
      chk(group ? tj_group_flight_profile(grp, times.data(), K, rec.data()) : tj_flight_profile(ctx, times.data(), K, rec.data()), "tj_flight_profile");
      std::ofstream pf;
      if (!profile_file.empty()) pf.open(profile_file);
      tjcli::print_flight_profile(rec, U, K, profile_file.empty() ? std::cout : pf, profile_file.empty());
    }
    if (dynamics) {
      std::vector<tj_dynamics_robot> rec(U);
      chk(group ? tj_group_peak_dynamics(grp, dynamics_tol, -1, 0, -1, rec.data()) : tj_peak_dynamics(ctx, dynamics_tol, -1, 0, -1, rec.data()), "tj_peak_dynamics");
      tjcli::print_peak_dynamics(rec);
    }
    if (dynwin) {
      const tj_dyn_gate gates[2] = {{dynwin_fraction * vel, TJ_DYNWIN_SPEED, TJ_DYNWIN_ABOVE}, {dynwin_fraction * acc, TJ_DYNWIN_ACCEL, TJ_DYNWIN_ABOVE}};
      std::vector<tj_dynwin_row> rows;
      chk(tjcli::listed_rows([&](tj_dynwin_row* out, int cap, int* n) {
            return group ? tj_group_dynamics_windows(grp, gates, 2, -1.0, -1, 0, out, cap, n) : tj_dynamics_windows(ctx, gates, 2, -1.0, -1, 0, out, cap, n); }, rows), "tj_dynamics_windows");
      tjcli::print_dynamics_windows(rows);
    }
    if (zonewin) {
      for (tj_zone& z : zone_list.zones) z.level = zonewin_level;
      const int nz = (int)zone_list.zones.size(), ns = (int)zone_list.shapes.size() / 4;
      std::vector<tj_zonewin_row> rows;
      chk(tjcli::listed_rows([&](tj_zonewin_row* out, int cap, int* n) {
            return group ? tj_group_zone_windows(grp, zone_list.zones.data(), nz, zone_list.shapes.data(), ns, -1.0, -1, 0, out, cap, n)
                         : tj_zone_windows(ctx, zone_list.zones.data(), nz, zone_list.shapes.data(), ns, -1.0, -1, 0, out, cap, n); }, rows), "tj_zone_windows");
      tjcli::print_zone_windows(rows, nz);
    }
    if (!dump.empty()) {
      std::ofstream df(dump);
      df.precision(17);
      const int T = 3 * P + 3;
      std::vector<double> s(3 * T); double pt = 0;
      df << "uav_num " << U << " piece_num " << P << " iter " << iter << " gnorm " << gnorm << " converged " << converged << "\n";
      for (int u = 0; u < U; u++) {
        chk(get_state(u, s.data(), &pt), "tj_get_state");
        df << "uav " << u << " piece_time " << pt << "\n";
        for (int r = 0; r < T; r++) df << s[r] << " " << s[r + T] << " " << s[r + 2 * T] << "\n";
      }
    }
    if (grp) tj_group_destroy(grp);
    if (ctx) tj_destroy(ctx);
    return converged ? 0 : 2;
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    if (grp) tj_group_destroy(grp);
    if (ctx) tj_destroy(ctx);
    return 1;
  }
}
