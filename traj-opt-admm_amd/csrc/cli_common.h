// cli_common.h -- file formats of the reference's two command-line tools, kept verbatim so the
// binaries are drop-ins on the same working directory layout:
//   Config_File/3D.json          16 flat numeric keys (Main/admmPathPlanning3D.cpp:368-397)
//   model/{single,multiple}/<m>  OBJ, only `v` lines are used, reading stops at the first other
//                                line once more than 10 vertices were seen (CCDUtils.h:317-391)
//   init/<m>_init_file.txt       way points (admmPathPlanning3D.cpp:79-112, multiPathPlanning3D.cpp:78-121)
//   result/<m>_result_file_*.txt iter / running time / point cloud size (admmPathPlanning3D.cpp:507-510)
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace tjcli {

// flat JSON object with numeric values
inline std::map<std::string, double> read_flat_json(const std::string& path) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::stringstream ss; ss << f.rdbuf();
  const std::string s = ss.str();
  std::map<std::string, double> out;
  size_t i = 0;
  while ((i = s.find('"', i)) != std::string::npos) {
    size_t j = s.find('"', i + 1);
    if (j == std::string::npos) break;
    std::string key = s.substr(i + 1, j - i - 1);
    size_t c = s.find(':', j);
    if (c == std::string::npos) break;
    char* end = nullptr;
    double v = std::strtod(s.c_str() + c + 1, &end);
    if (end == s.c_str() + c + 1) throw std::runtime_error("bad value for key " + key + " in " + path);
    out[key] = v;
    i = (size_t)(end - s.c_str());
  }
  return out;
}

inline double need(const std::map<std::string, double>& j, const char* key) {
  auto it = j.find(key);
  if (it == j.end()) throw std::runtime_error(std::string("3D.json: missing key \"") + key + "\"");  // all 16 keys are mandatory in the reference
  return it->second;
}

inline std::vector<double> read_obj_vertices(const std::string& path) {
  FILE* fp = fopen(path.c_str(), "r");
  if (!fp) throw std::runtime_error("cannot open " + path);
  std::vector<double> v;
  char line[2048], type[2048];
  int count = 0;
  while (fgets(line, sizeof(line), fp)) {
    if (sscanf(line, "%s", type) != 1) continue;
    if (strcmp(type, "v") == 0) {
      std::istringstream ls(line + 1);
      double x, y, z;
      if (ls >> x >> y >> z) { v.push_back(x); v.push_back(y); v.push_back(z); count++; }
    } else if (count > 10) break;
  }
  fclose(fp);
  return v;
}

// Triangle-mesh front end (ours: `--triangles` / "triangles":1 in 3D.json; BASELINE config 5).  The reference's reader drops
// the faces (above) although the library it links has a triangle broad phase (BVH::InitObstacle, BVH.cpp:15-51).  Reads the
// WHOLE file: every `v x y z` and every `f` line (1-based or negative indices, `i`, `i/t`, `i//n`, `i/t/n` tokens; polygons
// are fan-triangulated).  F holds 0-based vertex indices, 3 per triangle.
inline void read_obj_mesh(const std::string& path, std::vector<double>& V, std::vector<int>& F) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("cannot open " + path);
  V.clear(); F.clear();
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    std::string type;
    if (!(ls >> type)) continue;
    if (type == "v") {
      double x, y, z;
      if (ls >> x >> y >> z) { V.push_back(x); V.push_back(y); V.push_back(z); }
    } else if (type == "f") {
      std::vector<int> idx; std::string tok;
      const int nv = (int)(V.size() / 3);
      while (ls >> tok) {
        const long i = strtol(tok.c_str(), nullptr, 10);   // stops at the first '/'
        if (i == 0) throw std::runtime_error(path + ": bad face token '" + tok + "'");
        const long v = i > 0 ? i - 1 : nv + i;
        if (v < 0 || v >= nv) throw std::runtime_error(path + ": face refers to vertex " + std::to_string(i) + " of " + std::to_string(nv));
        idx.push_back((int)v);
      }
      for (size_t k = 1; k + 1 < idx.size(); k++) { F.push_back(idx[0]); F.push_back(idx[k]); F.push_back(idx[k + 1]); }
    }
  }
}

// single: one "x y z" per line.  multi: 3*U numbers per line, U from the first line.
inline void read_waypoints(const std::string& path, bool multi, int& U, int& P, std::vector<double>& wp /*[U][P+1][3]*/) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("cannot open " + path);
  std::vector<std::vector<double>> rows;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream is(line);
    std::vector<double> r; double x;
    while (is >> x) r.push_back(x);
    if (!r.empty()) rows.push_back(r);
  }
  if (rows.size() < 3) throw std::runtime_error(path + ": need at least 3 way points");
  U = multi ? (int)rows[0].size() / 3 : 1;
  if (U < 1) throw std::runtime_error(path + ": first line has fewer than 3 numbers");
  P = (int)rows.size() - 1;
  wp.assign((size_t)U * (P + 1) * 3, 0.0);
  for (int k = 0; k <= P; k++) {
    if ((int)rows[k].size() < 3 * U) throw std::runtime_error(path + ": short line");
    for (int u = 0; u < U; u++) for (int a = 0; a < 3; a++) wp[((size_t)u * (P + 1) + k) * 3 + a] = rows[k][3 * u + a];
  }
}

// "init":2 -- start/goal pairs of the planner.  The reference hard-codes them (single: Main/admmPathPlanning3D.cpp:222-228,
// multi: four robots, Main/multiPathPlanning3D.cpp:251-267); init/<mesh>_start_goal.txt (ours: one "sx sy sz gx gy gz" line
// per robot, solver units) overrides them.
inline void read_start_goal(const std::string& path, bool multi, std::vector<double>& starts, std::vector<double>& goals) {
  starts.clear(); goals.clear();
  std::ifstream f(path);
  if (f) {
    double v[6];
    while (f >> v[0] >> v[1] >> v[2] >> v[3] >> v[4] >> v[5]) { starts.insert(starts.end(), v, v + 3); goals.insert(goals.end(), v + 3, v + 6); if (!multi) break; }
    if (starts.empty()) throw std::runtime_error(path + ": need six numbers per robot");
    return;
  }
  if (!multi) { starts = {2.7, 0, 0}; goals = {-2.7, 0, 0}; return; }
  starts = {2.5, 1.7, 0.5, 2.5, 1.7, -0.5, -2.5, 1.7, 0.5, -2.5, 1.7, -0.5};
  goals = {-2.5, 1.7, 0.5, -2.5, 1.7, -0.5, 2.5, 1.7, -0.5, 2.5, 1.7, 0.5};
}

// log_data (Main/admmPathPlanning3D.cpp:33-77, Main/multiPathPlanning3D.cpp:33-77): duration of a trajectory and
// the length of its polyline sampled every `dt` seconds of flight time (0.05 single, 0.1 multi), evaluated on the
// per-piece Bezier control points C_i x_i exactly like getPosFromBezier (:17-31).  spline is T x 3 column-major,
// convert is [P][36] row-major.  samples (optional) receives the sampled positions, 3 per point.
inline void log_data(const double* spline, int P, const double* convert, double piece_time, double dt,
                     double& time_out, double& len_out, std::vector<double>* samples = nullptr) {
  const int T = 3 * P + 3;
  static const double binom5[6] = {1, 5, 10, 10, 5, 1};
  std::vector<double> coeff((size_t)P * 18);  // [piece][axis][6]
  for (int i = 0; i < P; i++)
    for (int a = 0; a < 3; a++)
      for (int j = 0; j < 6; j++) {
        double acc = 0;
        for (int k = 0; k < 6; k++) acc += convert[(size_t)i * 36 + j * 6 + k] * spline[3 * i + k + T * a];
        coeff[(size_t)i * 18 + a * 6 + j] = acc;
      }
  time_out = 0;
  for (int i = 0; i < P; i++) time_out += 1.0 * piece_time;  // time_weight == 1 everywhere
  len_out = 0;
  double prev[3] = {0, 0, 0};
  bool have = false;
  for (double t = 0.0; t < P; t += dt / piece_time) {
    const int i = (int)std::floor(t);
    const double ct = t - i;
    double cur[3] = {0, 0, 0};
    for (int a = 0; a < 3; a++)
      for (int j = 0; j < 6; j++) cur[a] += binom5[j] * coeff[(size_t)i * 18 + a * 6 + j] * std::pow(ct, j) * std::pow(1 - ct, 5 - j);
    if (have) len_out += std::sqrt((cur[0] - prev[0]) * (cur[0] - prev[0]) + (cur[1] - prev[1]) * (cur[1] - prev[1]) + (cur[2] - prev[2]) * (cur[2] - prev[2]));
    if (samples) { samples->push_back(cur[0]); samples->push_back(cur[1]); samples->push_back(cur[2]); }
    for (int a = 0; a < 3; a++) prev[a] = cur[a];
    have = true;
  }
}

// --audit, --audit-timed: one line per robot
inline void print_audit(const std::vector<tj_audit_robot>& rec) {
  std::cout.precision(17);
  for (size_t u = 0; u < rec.size(); u++) {
    const tj_audit_robot& r = rec[u];
    std::cout << "audit uav " << u << " obs " << r.obs_clearance << " seg " << r.obs_segment << " id " << r.obs_index << " pair " << r.pair_clearance << " seg " << r.pair_segment
              << " uav " << r.pair_robot << " speed " << r.speed << " seg " << r.speed_segment << " accel " << r.accel << " seg " << r.accel_segment << " time " << r.duration
              << " flags " << r.flags << std::endl;
  }
}
inline void print_audit_timed(const std::vector<tj_audit_timed_robot>& rec) {
  std::cout.precision(17);
  for (size_t u = 0; u < rec.size(); u++) {
    const tj_audit_timed_robot& r = rec[u];
    std::cout << "audit-timed uav " << u << " lo " << r.timed_lo << " uav " << r.lo_robot << " seg " << r.lo_segment << " hi " << r.timed_hi << " uav " << r.timed_robot
              << " seg " << r.timed_segment << " time " << r.timed_time << " levels " << r.levels << " flags " << r.flags << std::endl;
  }
}

// --closest-approach: one line per robot and the fleet's summary (the robot with the smallest attained separation)
inline void print_closest_approach(const std::vector<tj_closest_robot>& rec) {
  std::cout.precision(17);
  int who = -1, contact = 0;
  for (size_t u = 0; u < rec.size(); u++) {
    const tj_closest_robot& r = rec[u];
    std::cout << "closest uav " << u << " lo " << r.lo << " hi " << r.hi << " uav " << r.robot << " seg " << r.segment << " time " << r.time << " depth " << r.depth
              << " windows " << r.windows << " flags " << r.flags << std::endl;
    if (r.robot >= 0 && (who < 0 || r.hi < rec[who].hi)) who = (int)u;
    contact |= r.flags & TJ_CLOSEST_CONTACT;
  }
  if (who < 0) std::cout << "closest fleet none contact 0" << std::endl;
  else std::cout << "closest fleet hi " << rec[who].hi << " uav " << who << " uav " << rec[who].robot << " time " << rec[who].time << " contact " << contact << std::endl;
}

// --pair-approach: one line per listed directed pair, in the library's (robot, partner) order, and the counts of pairs in contact, undecided and certified clear
inline void print_pair_approach(const std::vector<tj_pair_record>& rows) {
  std::cout.precision(17);
  int contact = 0, clear = 0;
  for (const tj_pair_record& r : rows) {
    std::cout << "pair uav " << r.robot << " uav " << r.partner << " lo " << r.lo << " hi " << r.hi << " seg " << r.segment << " time " << r.time << " depth " << r.depth
              << " windows " << r.windows << " flags " << r.flags << std::endl;
    contact += r.flags & TJ_PAIR_CONTACT ? 1 : 0;
    clear += !(r.flags & TJ_PAIR_CONTACT) && (r.flags & TJ_PAIR_CLEAR) ? 1 : 0;
  }
  std::cout << "pair fleet listed " << rows.size() << " contact " << contact << " undecided " << rows.size() - contact - clear << " clear " << clear << std::endl;
}
// a row-listing query: the count-only call, then the rows.  f(rows or null, cap, &n): the context's or the group's entry point, bound to its handle and to the
// query's leading arguments (tj_pair_approach, tj_path_crossings, tj_timing_margin, tj_obstacle_windows)
template <class Rec, class F>
inline int listed_rows(F&& f, std::vector<Rec>& rows) {
  int n = 0;
  const int rc = f(nullptr, 0, &n);
  if (rc < 0) return rc;
  rows.resize(n);
  return n ? f(rows.data(), n, &n) : rc;
}

// --path-crossings: one line per listed unordered pair, in the library's (robot, partner) order, and the counts of pairs whose separation rests on timing
// (contact in space), undecided and separated in space
inline void print_path_crossings(const std::vector<tj_crossing_record>& rows) {
  std::cout.precision(17);
  int contact = 0, clear = 0;
  for (const tj_crossing_record& r : rows) {
    std::cout << "crossing uav " << r.robot << " uav " << r.partner << " lo " << r.lo << " hi " << r.hi << " seg " << r.segment << " s " << r.s << " time " << r.time
              << " seg " << r.partner_segment << " s " << r.partner_s << " time " << r.partner_time << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    contact += r.flags & TJ_CROSSING_CONTACT ? 1 : 0;
    clear += !(r.flags & TJ_CROSSING_CONTACT) && (r.flags & TJ_CROSSING_CLEAR) ? 1 : 0;
  }
  std::cout << "crossing fleet listed " << rows.size() << " timing " << contact << " undecided " << rows.size() - contact - clear << " space " << clear << std::endl;
}

// --timing-margin: one line per listed unordered pair, in the library's (robot, partner) order, and the fleet's line: the pairs within dist on the timetable, the
// pairs with a certified positive margin, and the smallest hi -- the slip the whole fleet tolerates (inf: no pair listed)
inline void print_timing_margin(const std::vector<tj_margin_record>& rows) {
  std::cout.precision(17);
  int contact = 0, positive = 0;
  double smallest = INFINITY;
  for (const tj_margin_record& r : rows) {
    std::cout << "margin uav " << r.robot << " uav " << r.partner << " lo " << r.lo << " hi " << r.hi << " dist " << r.distance << " seg " << r.segment << " s " << r.s << " time " << r.time
              << " seg " << r.partner_segment << " s " << r.partner_s << " time " << r.partner_time << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    contact += r.flags & TJ_MARGIN_CONTACT ? 1 : 0;
    positive += !(r.flags & TJ_MARGIN_CONTACT) && (r.flags & TJ_MARGIN_CLEAR) ? 1 : 0;
    smallest = std::min(smallest, r.hi);
  }
  std::cout << "margin fleet listed " << rows.size() << " contact " << contact << " positive " << positive << " smallest " << smallest << std::endl;
}

// --proximity-windows: one line per row, in the library's (robot, partner, t_first_lo) order, and the fleet's line: listed pairs, rows, the rows with a sure time,
// the grazes, and the seconds certified within dist summed over the rows
inline void print_proximity_windows(const std::vector<tj_proximity_row>& rows, int n_pairs) {
  std::cout.precision(17);
  int certain = 0, uncertain = 0;
  double within = 0.0;
  for (const tj_proximity_row& r : rows) {
    std::cout << "proximity uav " << r.robot << " uav " << r.partner << " first " << r.t_first_lo << " " << r.t_first_hi << " last " << r.t_last_lo << " " << r.t_last_hi << " within " << r.within_lo
              << " closest " << r.closest << " time " << r.closest_time << " leaves " << r.leaves << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    certain += r.flags & TJ_PROXIMITY_CERTAIN ? 1 : 0;
    uncertain += r.flags & TJ_PROXIMITY_UNCERTAIN ? 1 : 0;
    within += r.within_lo;
  }
  std::cout << "proximity fleet listed " << n_pairs << " rows " << rows.size() << " certain " << certain << " uncertain " << uncertain << " within " << within << std::endl;
}
// the count-only call, then the rows with a slot per listed pair, once more if the rows are more than that (f: the context's or the group's entry point, bound to its handle)
template <class F>
inline int proximity_windows_rows(F&& f, double dist, std::vector<tj_proximity_row>& rows, int& n_pairs) {
  int n = 0;
  int rc = f(dist, -1.0, -1, 0, nullptr, 0, &n_pairs, &n);
  if (rc < 0 || n_pairs == 0) return rc;
  rows.resize(n_pairs);
  rc = f(dist, -1.0, -1, 0, rows.data(), n_pairs, &n_pairs, &n);
  if (rc == TJ_ERR_CAPACITY && n > (int)rows.size()) {
    rows.resize(n);
    rc = f(dist, -1.0, -1, 0, rows.data(), n, &n_pairs, &n);
  }
  rows.resize(rc < 0 || n < 0 ? 0 : n);
  return rc;
}

// --obstacle-windows: one line per row, in the library's (robot, t_first_lo) order, and the fleet's line: rows, the rows with a sure time, the grazes, and the
// seconds certified within dist summed over the rows
inline void print_obstacle_windows(const std::vector<tj_obswin_row>& rows) {
  std::cout.precision(17);
  int certain = 0, uncertain = 0;
  double within = 0.0;
  for (const tj_obswin_row& r : rows) {
    std::cout << "obswin uav " << r.robot << " first " << r.t_first_lo << " " << r.t_first_hi << " last " << r.t_last_lo << " " << r.t_last_hi << " within " << r.within_lo
              << " closest " << r.closest << " time " << r.closest_time << " id " << r.index << " seg " << r.segment_first << " " << r.segment_last << " leaves " << r.leaves
              << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    certain += r.flags & TJ_OBSWIN_CERTAIN ? 1 : 0;
    uncertain += r.flags & TJ_OBSWIN_UNCERTAIN ? 1 : 0;
    within += r.within_lo;
  }
  std::cout << "obswin fleet rows " << rows.size() << " certain " << certain << " uncertain " << uncertain << " within " << within << std::endl;
}

// --dynamics-windows: one line per row, in the library's (robot, gate, t_first_lo) order, and the fleet's line: rows, the rows with a sure time, the grazes, and the
// seconds certified within the level summed over the rows
inline void print_dynamics_windows(const std::vector<tj_dynwin_row>& rows) {
  std::cout.precision(17);
  int certain = 0, uncertain = 0;
  double within = 0.0;
  for (const tj_dynwin_row& r : rows) {
    std::cout << "dynwin uav " << r.robot << " gate " << r.gate << " quantity " << r.quantity << " sense " << r.sense << " first " << r.t_first_lo << " " << r.t_first_hi << " last " << r.t_last_lo << " "
              << r.t_last_hi << " within " << r.within_lo << " extreme " << r.extreme << " time " << r.extreme_time << " seg " << r.segment_first << " " << r.segment_last << " leaves " << r.leaves
              << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    certain += r.flags & TJ_DYNWIN_CERTAIN ? 1 : 0;
    uncertain += r.flags & TJ_DYNWIN_UNCERTAIN ? 1 : 0;
    within += r.within_lo;
  }
  std::cout << "dynwin fleet rows " << rows.size() << " certain " << certain << " uncertain " << uncertain << " within " << within << std::endl;
}

// --zone-windows: one line per row, in the library's (robot, zone, t_first_lo) order, and the fleet's line: zones, rows, the rows with a sure time, the grazes, and the
// seconds certified within the level summed over the rows.  The zones: every --zone-box (6 unit faces in the order -x, +x, -y, +y, -z, +z) and --zone-ball in the
// order given, each with the sense in force where it stands (--zone-outside) and the one LEVEL.
struct ZoneList {
  std::vector<tj_zone> zones; std::vector<double> shapes; int sense = TJ_ZONE_INSIDE;
  void box(const double* v) {
    zones.push_back(tj_zone{0.0, TJ_ZONE_PLANES, sense, (int)shapes.size() / 4, 6});
    for (int a = 0; a < 3; a++)
      for (int side = 0; side < 2; side++) {
        double row[4] = {0.0, 0.0, 0.0, side ? v[3 + a] : -v[a]};
        row[a] = side ? 1.0 : -1.0;
        shapes.insert(shapes.end(), row, row + 4);
      }
  }
  void ball(const double* v) {
    zones.push_back(tj_zone{0.0, TJ_ZONE_BALL, sense, (int)shapes.size() / 4, 1});
    shapes.insert(shapes.end(), v, v + 4);
  }
};
inline void print_zone_windows(const std::vector<tj_zonewin_row>& rows, int n_zones) {
  std::cout.precision(17);
  int certain = 0, uncertain = 0;
  double within = 0.0;
  for (const tj_zonewin_row& r : rows) {
    std::cout << "zonewin uav " << r.robot << " zone " << r.zone << " sense " << r.sense << " face " << r.face << " first " << r.t_first_lo << " " << r.t_first_hi << " last " << r.t_last_lo << " "
              << r.t_last_hi << " within " << r.within_lo << " extreme " << r.extreme << " time " << r.extreme_time << " seg " << r.segment_first << " " << r.segment_last << " leaves " << r.leaves
              << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    certain += r.flags & TJ_ZONEWIN_CERTAIN ? 1 : 0;
    uncertain += r.flags & TJ_ZONEWIN_UNCERTAIN ? 1 : 0;
    within += r.within_lo;
  }
  std::cout << "zonewin fleet zones " << n_zones << " rows " << rows.size() << " certain " << certain << " uncertain " << uncertain << " within " << within << std::endl;
}

// --sight-windows: one line per row, in the library's (link, t_first_lo) order, and the fleet's line: links, rows, the rows with a sure time, the grazes, and the
// seconds certified within dist summed over the rows.  The links: every directed robot pair in (a, b) order, then per robot every station of --sight-station.
inline std::vector<int> sight_links(int U, int n_stations) {
  std::vector<int> links;
  for (int a = 0; a < U; a++) for (int b = 0; b < U; b++) if (b != a) { links.push_back(a); links.push_back(b); }
  for (int a = 0; a < U; a++) for (int s = 0; s < n_stations; s++) { links.push_back(a); links.push_back(-1 - s); }
  return links;
}
inline void print_sight_windows(const std::vector<tj_sight_row>& rows, int n_links) {
  std::cout.precision(17);
  int certain = 0, uncertain = 0;
  double within = 0.0;
  for (const tj_sight_row& r : rows) {
    std::cout << "sight link " << r.link << " uav " << r.robot << " to " << r.partner << " first " << r.t_first_lo << " " << r.t_first_hi << " last " << r.t_last_lo << " " << r.t_last_hi << " within " << r.within_lo
              << " closest " << r.closest << " time " << r.closest_time << " id " << r.index << " leaves " << r.leaves << " depth " << r.depth << " windows " << r.windows << " flags " << r.flags << std::endl;
    certain += r.flags & TJ_SIGHT_CERTAIN ? 1 : 0;
    uncertain += r.flags & TJ_SIGHT_UNCERTAIN ? 1 : 0;
    within += r.within_lo;
  }
  std::cout << "sight fleet " << n_links << " rows " << rows.size() << " certain " << certain << " uncertain " << uncertain << " within " << within << std::endl;
}

// --obstacle-approach: one line per robot and the fleet's summary (the robot with the smallest attained distance), in the style of --closest-approach
inline void print_obstacle_approach(const std::vector<tj_obstacle_robot>& rec) {
  std::cout.precision(17);
  int who = -1, contact = 0;
  for (size_t u = 0; u < rec.size(); u++) {
    const tj_obstacle_robot& r = rec[u];
    std::cout << "obstacle uav " << u << " lo " << r.lo << " hi " << r.hi << " id " << r.index << " seg " << r.segment << " time " << r.time << " depth " << r.depth
              << " windows " << r.windows << " flags " << r.flags << std::endl;
    if (r.index >= 0 && (who < 0 || r.hi < rec[who].hi)) who = (int)u;
    contact |= r.flags & TJ_OBSTACLE_CONTACT;
  }
  if (who < 0) std::cout << "obstacle fleet none contact 0" << std::endl;
  else std::cout << "obstacle fleet hi " << rec[who].hi << " uav " << who << " id " << rec[who].index << " time " << rec[who].time << " contact " << contact << std::endl;
}

// --peak-dynamics: one line per robot and the fleet's summary (the robot with the largest time_scale), in the style of --obstacle-approach
inline void print_peak_dynamics(const std::vector<tj_dynamics_robot>& rec) {
  std::cout.precision(17);
  size_t who = 0;
  auto peak = [](const char* name, const tj_peak& p) {
    std::cout << " " << name << " lo " << p.lo << " hi " << p.hi << " seg " << p.segment << " time " << p.time << " depth " << p.depth << " windows " << p.windows << " flags " << p.flags;
  };
  for (size_t u = 0; u < rec.size(); u++) {
    const tj_dynamics_robot& r = rec[u];
    std::cout << "dynamics uav " << u;
    peak("speed", r.speed); peak("accel", r.accel); peak("jerk", r.jerk);
    std::cout << " length lo " << r.length_lo << " hi " << r.length_hi << " levels " << r.length_levels << " duration " << r.duration << " time_scale " << r.time_scale
              << " flags " << r.flags << std::endl;
    if (r.time_scale > rec[who].time_scale) who = u;
  }
  if (!rec.empty()) std::cout << "dynamics fleet time_scale " << rec[who].time_scale << " uav " << who << std::endl;
}

// --flight-profile: one line per robot and sample, robot after robot; `word`: the lines start with "profile " (standard output, next to the other queries' lines)
inline void print_flight_profile(const std::vector<tj_profile_sample>& rec, int U, int K, std::ostream& os, bool word) {
  os.precision(17);
  for (int u = 0; u < U; u++)
    for (int k = 0; k < K; k++) {
      const tj_profile_sample& r = rec[(size_t)u * K + k];
      os << (word ? "profile " : "") << u << " " << r.time << " " << r.x << " " << r.y << " " << r.z << " " << r.obs_distance << " " << r.obs_index << " " << r.robot_distance << " "
         << r.robot << " " << r.speed << " " << r.accel << " " << r.flags << "\n";
    }
  os.flush();
}

}  // namespace tjcli
