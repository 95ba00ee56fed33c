"""Python host-side mirror of the C ABI in include/trajadmm.h (libtrajadmm.so).

The reference is compiled C++ with no Python layer; this module exists for the test-suite,
bench.py and for Python callers, and is a thin ctypes binding -- all numerics run in the HIP
kernels behind the C ABI.  There is NO CPU fallback: importing works anywhere (so that
`-m "not gpu"` tests can check the exported symbols), but creating a `Solver` without the
built library or without a HIP device raises.

Method names follow the reference's driver vocabulary
(Optimization3D_multi::optimization_decouple and its stages, Optimization3D_multi.h:29-118).
"""
import ctypes as C
import os
import numpy as np

from . import scenes  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRAJADMM_LIB") or os.path.join(_HERE, "libtrajadmm.so")  # override: another BUILD of this library (e.g. `make timing`)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

EXPORTS = [
    "tj_default_params", "tj_create", "tj_destroy", "tj_last_error", "tj_set_cloud", "tj_set_mesh", "tj_init_state", "tj_get_state",
    "tj_set_state", "tj_iterate", "tj_iterate_async", "tj_sync", "tj_stream", "tj_run_stage", "tj_get_planes", "tj_get_candidates",
    "tj_set_planes", "tj_get_direction", "tj_set_direction", "tj_get_local_grad", "tj_get_steps", "tj_get_energy", "tj_get_stats", "tj_get_build_info", "tj_exchange_buffer",
    "tj_iterate_phase", "tj_iterate_phase_chained", "tj_set_coupled_follow", "tj_coupled_search_pending", "tj_launch_count", "tj_phase_count", "tj_xch_block", "tj_xch_ipc_export", "tj_xch_ipc_open", "tj_xch_attach", "tj_xch_enable", "tj_set_stream", "tj_host_tables", "tj_profile_kernels", "tj_kernel_count", "tj_kernel_name",
    "tj_get_obs_cache", "tj_set_obs_cache", "tj_get_pair_cache", "tj_set_pair_cache", "tj_edge_collision", "tj_plan_init",
    "tj_group_create", "tj_group_destroy", "tj_group_size", "tj_group_ctx", "tj_group_last_error", "tj_group_set_cloud", "tj_group_set_mesh",
    "tj_group_transport", "tj_group_set_transport", "tj_group_profile_exchange", "tj_rccl_available", "tj_group_rccl_ranks",
    "tj_group_init_state", "tj_group_iterate", "tj_group_get_state",
    "tj_audit", "tj_audit_record_size", "tj_group_audit",
    "tj_audit_timed", "tj_audit_timed_record_size", "tj_group_audit_timed",
    "tj_closest_approach", "tj_closest_record_size", "tj_group_closest_approach",
    "tj_obstacle_approach", "tj_obstacle_record_size", "tj_group_obstacle_approach",
    "tj_obstacle_windows", "tj_obswin_row_size", "tj_group_obstacle_windows",
    "tj_sight_windows", "tj_sight_row_size", "tj_group_sight_windows",
    "tj_pair_approach", "tj_pair_record_size", "tj_group_pair_approach",
    "tj_path_crossings", "tj_crossing_record_size", "tj_group_path_crossings",
    "tj_timing_margin", "tj_margin_record_size", "tj_group_timing_margin",
    "tj_proximity_windows", "tj_proximity_row_size", "tj_group_proximity_windows",
    "tj_flight_profile", "tj_flight_profile_record_size", "tj_group_flight_profile",
    "tj_peak_dynamics", "tj_dynamics_record_size", "tj_group_peak_dynamics",
    "tj_dynamics_windows", "tj_dynwin_row_size", "tj_group_dynamics_windows",
    "tj_zone_windows", "tj_zonewin_row_size", "tj_group_zone_windows",
]

STAGES = dict(begin=0, planes_obs=1, planes_self=2, grad=3, xsolve=4, ccd_prep=5, ccd_obs=6, ccd_self=7, linesearch=8, slack=9, end=10)


class TjParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("uav_num", C.c_int), ("piece_num", C.c_int), ("res", C.c_int),
                ("lambda_", C.c_double), ("margin", C.c_double), ("offset", C.c_double), ("mu", C.c_double),
                ("vel_limit", C.c_double), ("acc_limit", C.c_double), ("ks", C.c_double), ("kt", C.c_double),
                ("stop", C.c_double), ("device", C.c_int), ("rank", C.c_int), ("world", C.c_int),
                ("cap_obs", C.c_int), ("cap_self", C.c_int), ("cap_pairs", C.c_int), ("optimal_plane", C.c_int)]


class TjStats(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in ("iters", "nodes_dcd", "nodes_ccd", "cand_dcd", "cand_ccd", "planes_obs",
                                             "planes_self", "energy_evals", "pair_tests", "llt_fail_piece", "llt_fail_robot", "newton_iters", "pair_solves")] + \
               [("order_ambiguous", C.c_int), ("error_bits", C.c_int), ("order_unresolved", C.c_int), ("head_starts", C.c_int), ("gjk_max_sum", C.c_ulonglong),
                ("ls_giveups", C.c_int), ("ls_helper_timeouts", C.c_int), ("async_fallbacks", C.c_int)]


class TjAuditRobot(C.Structure):
    """mirror of tj_audit_robot (include/trajadmm.h); tj_audit_record_size() is its sizeof on the C side"""
    _fields_ = [("obs_clearance", C.c_double), ("obs_segment", C.c_int), ("obs_index", C.c_int),
                ("pair_clearance", C.c_double), ("pair_segment", C.c_int), ("pair_robot", C.c_int),
                ("speed", C.c_double), ("accel", C.c_double), ("speed_segment", C.c_int), ("accel_segment", C.c_int),
                ("duration", C.c_double), ("flags", C.c_int), ("reserved", C.c_int)]


AUDIT_FLAGS = dict(obs_contact=1, pair_contact=2, speed=4, accel=8)


def _records(struct, rec, only=None):
    """an array of C records -> dict of numpy arrays, one per field (`reserved` is dropped; only: the fields wanted)"""
    return {n: np.array([getattr(r, n) for r in rec], dtype=np.float64 if t is C.c_double else np.int32) for n, t in struct._fields_ if n != "reserved" and (only is None or n in only)}


def _audit(call, U, S, range, per_segment):
    """shared by Solver.audit / Group.audit: call(range, records, seg_obs, seg_pair) -> dict of numpy arrays [U] (+ [U][S])"""
    rec = (TjAuditRobot * U)()
    so = np.zeros((U, S)) if per_segment else None
    sp = np.zeros((U, S)) if per_segment else None
    call(C.c_double(0.0 if range is None else float(range)), rec, _d(so) if per_segment else None, _d(sp) if per_segment else None)
    out = _records(TjAuditRobot, rec)
    if per_segment:
        out["seg_obs"], out["seg_pair"] = so, sp
    return out


class TjAuditTimedRobot(C.Structure):
    """mirror of tj_audit_timed_robot (include/trajadmm.h); tj_audit_timed_record_size() is its sizeof on the C side"""
    _fields_ = [("timed_lo", C.c_double), ("timed_hi", C.c_double), ("timed_time", C.c_double),
                ("timed_robot", C.c_int), ("timed_segment", C.c_int), ("lo_robot", C.c_int), ("lo_segment", C.c_int),
                ("levels", C.c_int), ("flags", C.c_int)]


AUDIT_TIMED_FLAGS = dict(contact=1, clear=2)
AUDIT_TIMED_LEVELS = 1   # TJ_AUDIT_TIMED_LEVELS: what levels=None selects


def _audit_timed(call, U, S, range, levels, per_segment):
    """shared by Solver.audit_timed / Group.audit_timed: call(range, levels, records, seg_lo, seg_hi) -> dict of numpy arrays [U] (+ [U][S])"""
    rec = (TjAuditTimedRobot * U)()
    sl = np.zeros((U, S)) if per_segment else None
    sh = np.zeros((U, S)) if per_segment else None
    call(C.c_double(0.0 if range is None else float(range)), C.c_int(-1 if levels is None else int(levels)), rec,
         _d(sl) if per_segment else None, _d(sh) if per_segment else None)
    out = _records(TjAuditTimedRobot, rec)
    if per_segment:
        out["seg_lo"], out["seg_hi"] = sl, sh
    return out


class TjClosestRobot(C.Structure):
    """mirror of tj_closest_robot (include/trajadmm.h); tj_closest_record_size() is its sizeof on the C side"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("time", C.c_double), ("robot", C.c_int), ("segment", C.c_int),
                ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int), ("reserved", C.c_int)]


CLOSEST_FLAGS = dict(contact=1, clear=2, converged=4, truncated=8)
CLOSEST_TOL = 1e-10        # TJ_CLOSEST_TOL: what tol=None selects
CLOSEST_MAX_DEPTH = 40     # TJ_CLOSEST_MAX_DEPTH
CLOSEST_FRONTIER = 4096    # TJ_CLOSEST_FRONTIER


def _search_args(range, tol, max_depth, max_windows):
    """(range, tol, max_depth, max_windows) of the four branch-and-bound queries as the C side takes them; None selects the C side's default"""
    return (C.c_double(0.0 if range is None else float(range)), C.c_double(-1.0 if tol is None else float(tol)), C.c_int(-1 if max_depth is None else int(max_depth)),
            C.c_int(0 if max_windows is None else int(max_windows)))


def _approach(struct, call, U, range, tol, max_depth, max_windows):
    """shared by closest_approach / obstacle_approach of Solver and Group: call(range, tol, max_depth, max_windows, records) -> dict of numpy arrays [U]"""
    rec = (struct * U)()
    call(*_search_args(range, tol, max_depth, max_windows), rec)
    return _records(struct, rec)


def _listed_rows(struct, call, args):
    """shared by pair_approach / path_crossings of Solver and Group: call(*args, rows, cap, n).  The count-only call first, then the rows -> dict of numpy arrays [n]"""
    n = C.c_int(0)
    call(*args, None, C.c_int(0), C.byref(n))
    rec = (struct * max(n.value, 1))()
    if n.value:
        call(*args, rec, C.c_int(n.value), C.byref(n))
    return _records(struct, rec[:n.value])


class TjObstacleRobot(C.Structure):
    """mirror of tj_obstacle_robot (include/trajadmm.h); tj_obstacle_record_size() is its sizeof on the C side"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("time", C.c_double), ("index", C.c_int), ("segment", C.c_int),
                ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int), ("reserved", C.c_int)]


OBSTACLE_FLAGS = dict(contact=1, clear=2, converged=4, truncated=8)
OBSTACLE_TOL = 1e-11        # TJ_OBSTACLE_TOL: what tol=None selects
OBSTACLE_MAX_DEPTH = 40     # TJ_OBSTACLE_MAX_DEPTH
OBSTACLE_FRONTIER = 4096    # TJ_OBSTACLE_FRONTIER


class TjPeak(C.Structure):
    """mirror of tj_peak (include/trajadmm.h)"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("time", C.c_double), ("segment", C.c_int), ("depth", C.c_int), ("windows", C.c_int), ("flags", C.c_int)]


class TjDynamicsRobot(C.Structure):
    """mirror of tj_dynamics_robot (include/trajadmm.h); tj_dynamics_record_size() is its sizeof on the C side"""
    _fields_ = [("speed", TjPeak), ("accel", TjPeak), ("jerk", TjPeak), ("length_lo", C.c_double), ("length_hi", C.c_double), ("duration", C.c_double),
                ("time_scale", C.c_double), ("length_levels", C.c_int), ("flags", C.c_int)]


PEAK_FLAGS = dict(converged=4, truncated=8)                        # the flags of a TjPeak
PEAK_DYN_FLAGS = dict(speed=1, speed_ok=2, accel=4, accel_ok=8)    # the flags of a TjDynamicsRobot
PEAK_TOL = 1e-14            # TJ_PEAK_TOL: what tol=None selects (relative)
PEAK_MAX_DEPTH = 40         # TJ_PEAK_MAX_DEPTH
PEAK_FRONTIER = 1024        # TJ_PEAK_FRONTIER
PEAK_LENGTH_LEVELS = 4      # TJ_PEAK_LENGTH_LEVELS: what length_levels=None selects
PEAK_MAX_LENGTH_LEVELS = 12 # TJ_PEAK_MAX_LENGTH_LEVELS


def _peak_dynamics(call, U, tol, max_depth, max_windows, length_levels):
    """shared by Solver.peak_dynamics / Group.peak_dynamics: call(tol, max_depth, max_windows, length_levels, records) -> dict of numpy arrays [U]; a peak's fields
    under `speed_lo`, `speed_hi`, `speed_time`, `speed_segment`, `speed_depth`, `speed_windows`, `speed_flags` (and accel_, jerk_)"""
    rec = (TjDynamicsRobot * U)()
    call(C.c_double(-1.0 if tol is None else float(tol)), C.c_int(-1 if max_depth is None else int(max_depth)), C.c_int(0 if max_windows is None else int(max_windows)),
         C.c_int(-1 if length_levels is None else int(length_levels)), rec)
    out = {}
    for q in ("speed", "accel", "jerk"):
        for n, v in _records(TjPeak, [getattr(r, q) for r in rec]).items():
            out[q + "_" + n] = v
    out.update(_records(TjDynamicsRobot, rec, ("length_lo", "length_hi", "duration", "time_scale", "length_levels", "flags")))
    return out


class TjPairRecord(C.Structure):
    """mirror of tj_pair_record (include/trajadmm.h); tj_pair_record_size() is its sizeof on the C side"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("time", C.c_double), ("robot", C.c_int), ("partner", C.c_int), ("segment", C.c_int),
                ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int)]


PAIR_FLAGS = dict(contact=1, clear=2, converged=4, truncated=8)
PAIR_TOL = 1e-10           # TJ_PAIR_TOL: what tol=None selects
PAIR_MAX_DEPTH = 40        # TJ_PAIR_MAX_DEPTH
PAIR_FRONTIER = 64         # TJ_PAIR_FRONTIER: what max_windows=None selects
PAIR_MAX_WINDOWS = 4096    # TJ_PAIR_MAX_WINDOWS


class TjCrossingRecord(C.Structure):
    """mirror of tj_crossing_record (include/trajadmm.h); tj_crossing_record_size() is its sizeof on the C side"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("s", C.c_double), ("partner_s", C.c_double), ("time", C.c_double), ("partner_time", C.c_double),
                ("robot", C.c_int), ("partner", C.c_int), ("segment", C.c_int), ("partner_segment", C.c_int), ("depth", C.c_int), ("flags", C.c_int),
                ("windows", C.c_int), ("reserved", C.c_int)]


CROSSING_FLAGS = dict(contact=1, clear=2, converged=4, truncated=8, robot_end=16, partner_end=32)
CROSSING_TOL = 1e-10           # TJ_CROSSING_TOL: what tol=None selects
CROSSING_MAX_DEPTH = 40        # TJ_CROSSING_MAX_DEPTH
CROSSING_FRONTIER = 256        # TJ_CROSSING_FRONTIER: what max_windows=None selects
CROSSING_MAX_WINDOWS = 4096    # TJ_CROSSING_MAX_WINDOWS


class TjMarginRecord(C.Structure):
    """mirror of tj_margin_record (include/trajadmm.h); tj_margin_record_size() is its sizeof on the C side"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("distance", C.c_double), ("s", C.c_double), ("partner_s", C.c_double), ("time", C.c_double),
                ("partner_time", C.c_double), ("robot", C.c_int), ("partner", C.c_int), ("segment", C.c_int), ("partner_segment", C.c_int), ("depth", C.c_int),
                ("flags", C.c_int), ("windows", C.c_int), ("reserved", C.c_int)]


MARGIN_FLAGS = dict(contact=1, clear=2, converged=4, truncated=8, robot_end=16, partner_end=32, same_time=64)
MARGIN_TOL_FRACTION = 0.01   # TJ_MARGIN_TOL_FRACTION: tol=None selects this fraction of dist over vel_limit, a time
MARGIN_MAX_DEPTH = 40        # TJ_MARGIN_MAX_DEPTH
MARGIN_FRONTIER = 4096       # TJ_MARGIN_FRONTIER: what max_windows=None selects
MARGIN_MAX_WINDOWS = 4096    # TJ_MARGIN_MAX_WINDOWS


class TjProximityRow(C.Structure):
    """mirror of tj_proximity_row (include/trajadmm.h); tj_proximity_row_size() is its sizeof on the C side"""
    _fields_ = [("t_first_lo", C.c_double), ("t_first_hi", C.c_double), ("t_last_lo", C.c_double), ("t_last_hi", C.c_double), ("within_lo", C.c_double),
                ("closest", C.c_double), ("closest_time", C.c_double), ("robot", C.c_int), ("partner", C.c_int), ("leaves", C.c_int), ("depth", C.c_int),
                ("flags", C.c_int), ("windows", C.c_int)]


PROXIMITY_FLAGS = dict(certain=1, uncertain=2, at_start=4, at_end=8, resolved=16, truncated=32)
PROXIMITY_TOL_FRACTION = 0.01   # TJ_PROXIMITY_TOL_FRACTION: tol=None selects this fraction of dist over vel_limit, a time
PROXIMITY_MAX_DEPTH = 40        # TJ_PROXIMITY_MAX_DEPTH
PROXIMITY_FRONTIER = 512        # TJ_PROXIMITY_FRONTIER: what max_windows=None selects
PROXIMITY_MAX_WINDOWS = 4096    # TJ_PROXIMITY_MAX_WINDOWS


class TjObswinRow(C.Structure):
    """mirror of tj_obswin_row (include/trajadmm.h); tj_obswin_row_size() is its sizeof on the C side"""
    _fields_ = [("t_first_lo", C.c_double), ("t_first_hi", C.c_double), ("t_last_lo", C.c_double), ("t_last_hi", C.c_double), ("within_lo", C.c_double),
                ("closest", C.c_double), ("closest_time", C.c_double), ("robot", C.c_int), ("index", C.c_int), ("segment_first", C.c_int), ("segment_last", C.c_int),
                ("leaves", C.c_int), ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int)]


OBSWIN_FLAGS = dict(certain=1, uncertain=2, at_start=4, at_end=8, resolved=16, truncated=32)
OBSWIN_TOL_FRACTION = 0.01   # TJ_OBSWIN_TOL_FRACTION: tol=None selects this fraction of dist over vel_limit, a time
OBSWIN_MAX_DEPTH = 40        # TJ_OBSWIN_MAX_DEPTH
OBSWIN_FRONTIER = 128        # TJ_OBSWIN_FRONTIER: what max_windows=None selects
OBSWIN_MAX_WINDOWS = 1024    # TJ_OBSWIN_MAX_WINDOWS


class TjSightRow(C.Structure):
    """mirror of tj_sight_row (include/trajadmm.h); tj_sight_row_size() is its sizeof on the C side"""
    _fields_ = [("t_first_lo", C.c_double), ("t_first_hi", C.c_double), ("t_last_lo", C.c_double), ("t_last_hi", C.c_double), ("within_lo", C.c_double),
                ("closest", C.c_double), ("closest_time", C.c_double), ("link", C.c_int), ("robot", C.c_int), ("partner", C.c_int), ("index", C.c_int),
                ("leaves", C.c_int), ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int)]


SIGHT_FLAGS = dict(certain=1, uncertain=2, at_start=4, at_end=8, resolved=16, truncated=32)
SIGHT_TOL_FRACTION = 0.01   # TJ_SIGHT_TOL_FRACTION: tol=None selects this fraction of dist over vel_limit, a time
SIGHT_MAX_DEPTH = 40        # TJ_SIGHT_MAX_DEPTH
SIGHT_FRONTIER = 128        # TJ_SIGHT_FRONTIER: what max_windows=None selects
SIGHT_MAX_WINDOWS = 1024    # TJ_SIGHT_MAX_WINDOWS
SIGHT_PROJECTIONS = 3       # TJ_SIGHT_PROJECTIONS: the alternating projections of a triangle's sample


def sight_links(U, n_stations):
    """what links=None selects: every directed robot pair in (a, b) order, then per robot every station (-1 - s)"""
    return [(a, b) for a in range(U) for b in range(U) if b != a] + [(a, -1 - s) for a in range(U) for s in range(n_stations)]


def _sight_windows(call, U, links, stations, dist, tol, max_depth, max_windows):
    """shared by Solver.sight_windows / Group.sight_windows: call(links, n_links, stations, n_stations, dist, tol, max_depth, max_windows, rows, cap, n)"""
    st = np.zeros((0, 3)) if stations is None else np.ascontiguousarray(stations, dtype=np.float64).reshape(-1, 3)
    lk = np.ascontiguousarray(sight_links(U, len(st)) if links is None else links, dtype=np.int32).reshape(-1, 2)
    return _listed_rows(TjSightRow, call, (lk.ctypes.data_as(_ip), C.c_int(len(lk)), _d(st), C.c_int(len(st))) + _search_args(dist, tol, max_depth, max_windows))


class TjDynGate(C.Structure):
    """mirror of tj_dyn_gate (include/trajadmm.h)"""
    _fields_ = [("level", C.c_double), ("quantity", C.c_int), ("sense", C.c_int)]


class TjDynwinRow(C.Structure):
    """mirror of tj_dynwin_row (include/trajadmm.h); tj_dynwin_row_size() is its sizeof on the C side"""
    _fields_ = [("t_first_lo", C.c_double), ("t_first_hi", C.c_double), ("t_last_lo", C.c_double), ("t_last_hi", C.c_double), ("within_lo", C.c_double),
                ("extreme", C.c_double), ("extreme_time", C.c_double), ("robot", C.c_int), ("gate", C.c_int), ("quantity", C.c_int), ("sense", C.c_int),
                ("segment_first", C.c_int), ("segment_last", C.c_int), ("leaves", C.c_int), ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int)]


DYNWIN_FLAGS = dict(certain=1, uncertain=2, at_start=4, at_end=8, resolved=16, truncated=32)
DYNWIN_QUANTITIES = dict(speed=0, accel=1, jerk=2)   # TJ_DYNWIN_SPEED, TJ_DYNWIN_ACCEL, TJ_DYNWIN_JERK
DYNWIN_SENSES = dict(above=0, below=1)               # TJ_DYNWIN_ABOVE (within = value >= level), TJ_DYNWIN_BELOW (within = value <= level)
DYNWIN_TOL_FRACTION = 0.01   # TJ_DYNWIN_TOL_FRACTION: tol=None selects this fraction of vel_limit over acc_limit, a time
DYNWIN_MAX_GATES = 16        # TJ_DYNWIN_MAX_GATES
DYNWIN_MAX_DEPTH = 40        # TJ_DYNWIN_MAX_DEPTH
DYNWIN_FRONTIER = 64         # TJ_DYNWIN_FRONTIER: what max_windows=None selects
DYNWIN_MAX_WINDOWS = 1024    # TJ_DYNWIN_MAX_WINDOWS


def dynwin_gates(gates):
    """a list of (quantity, sense, level), quantity / sense by name (DYNWIN_QUANTITIES / DYNWIN_SENSES) or number -> a list of (int, int, float)"""
    return [(DYNWIN_QUANTITIES[q] if isinstance(q, str) else int(q), DYNWIN_SENSES[s] if isinstance(s, str) else int(s), float(level)) for q, s, level in gates]


def _dynamics_windows(call, gates, tol, max_depth, max_windows):
    """shared by Solver.dynamics_windows / Group.dynamics_windows: call(gates, n_gates, tol, max_depth, max_windows, rows, cap, n); gates=None: a null list, the
    two default gates; an empty list: no gate"""
    gl = None if gates is None else dynwin_gates(gates)
    arr = None if gl is None else (TjDynGate * max(len(gl), 1))(*[TjDynGate(level, q, s) for q, s, level in gl])
    return _listed_rows(TjDynwinRow, call, (arr, C.c_int(0 if gl is None else len(gl))) + _search_args(None, tol, max_depth, max_windows)[1:])


class TjZone(C.Structure):
    """mirror of tj_zone (include/trajadmm.h)"""
    _fields_ = [("level", C.c_double), ("kind", C.c_int), ("sense", C.c_int), ("first", C.c_int), ("count", C.c_int)]


class TjZonewinRow(C.Structure):
    """mirror of tj_zonewin_row (include/trajadmm.h); tj_zonewin_row_size() is its sizeof on the C side"""
    _fields_ = [("t_first_lo", C.c_double), ("t_first_hi", C.c_double), ("t_last_lo", C.c_double), ("t_last_hi", C.c_double), ("within_lo", C.c_double),
                ("extreme", C.c_double), ("extreme_time", C.c_double), ("robot", C.c_int), ("zone", C.c_int), ("sense", C.c_int), ("face", C.c_int),
                ("segment_first", C.c_int), ("segment_last", C.c_int), ("leaves", C.c_int), ("depth", C.c_int), ("flags", C.c_int), ("windows", C.c_int)]


ZONEWIN_FLAGS = dict(certain=1, uncertain=2, at_start=4, at_end=8, resolved=16, truncated=32)
ZONE_KINDS = dict(planes=0, ball=1)        # TJ_ZONE_PLANES (half-spaces n . x <= d), TJ_ZONE_BALL (|x - c| <= r)
ZONE_SENSES = dict(inside=0, outside=1)    # TJ_ZONE_INSIDE (within = gauge <= level), TJ_ZONE_OUTSIDE (within = gauge >= level)
ZONEWIN_TOL_FRACTION = 0.01   # TJ_ZONEWIN_TOL_FRACTION: tol=None selects this fraction of offset over vel_limit, a time
ZONEWIN_MAX_ZONES = 64        # TJ_ZONEWIN_MAX_ZONES
ZONEWIN_MAX_PLANES = 32       # TJ_ZONEWIN_MAX_PLANES
ZONEWIN_MAX_DEPTH = 40        # TJ_ZONEWIN_MAX_DEPTH
ZONEWIN_FRONTIER = 512        # TJ_ZONEWIN_FRONTIER: what max_windows=None selects
ZONEWIN_MAX_WINDOWS = 1024    # TJ_ZONEWIN_MAX_WINDOWS


def zone_planes(rows, sense="inside", level=0.0):
    """the convex polytope of the half-spaces n . x <= d: rows [count][4] of (nx, ny, nz, d), not normalised by the library -> a zone (kind, sense, level, rows)"""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 4)
    return ZONE_KINDS["planes"], ZONE_SENSES[sense] if isinstance(sense, str) else int(sense), float(level), rows


def zone_box(lo, hi, sense="inside", level=0.0):
    """the axis-aligned box lo <= x <= hi: 6 unit faces in the order -x, +x, -y, +y, -z, +z"""
    rows = []
    for a in range(3):
        n = [0.0, 0.0, 0.0]
        n[a] = -1.0
        rows.append(n + [-float(lo[a])])
        n = [0.0, 0.0, 0.0]
        n[a] = 1.0
        rows.append(n + [float(hi[a])])
    return zone_planes(rows, sense, level)


def zone_ball(center, r, sense="inside", level=0.0):
    """the ball |x - center| <= r"""
    return ZONE_KINDS["ball"], ZONE_SENSES[sense] if isinstance(sense, str) else int(sense), float(level), np.array([[center[0], center[1], center[2], r]], dtype=np.float64)


def zonewin_pack(zones):
    """zones as zone_planes / zone_box / zone_ball return them -> (a ctypes array of TjZone, the shape table [n_shapes][4] as a C-contiguous numpy array): every
    zone's rows one after the other, `first` the offset of its first"""
    arr = (TjZone * max(len(zones), 1))()
    table, first = [], 0
    for k, (kind, sense, level, rows) in enumerate(zones):
        arr[k] = TjZone(float(level), int(kind), int(sense), first, len(rows))
        table.append(np.asarray(rows, dtype=np.float64).reshape(-1, 4))
        first += len(rows)
    return arr, np.ascontiguousarray(np.concatenate(table) if table else np.zeros((0, 4)))


def _zone_windows(call, zones, tol, max_depth, max_windows):
    """shared by Solver.zone_windows / Group.zone_windows: call(zones, n_zones, shapes, n_shapes, tol, max_depth, max_windows, rows, cap, n)"""
    arr, table = zonewin_pack(list(zones))
    return _listed_rows(TjZonewinRow, call, (arr, C.c_int(len(zones)), table.ctypes.data_as(C.POINTER(C.c_double)) if len(table) else None, C.c_int(len(table))) +
                        _search_args(None, tol, max_depth, max_windows)[1:])


class TjProfileSample(C.Structure):
    """mirror of tj_profile_sample (include/trajadmm.h); tj_flight_profile_record_size() is its sizeof on the C side"""
    _fields_ = [("time", C.c_double), ("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("obs_distance", C.c_double), ("robot_distance", C.c_double),
                ("speed", C.c_double), ("accel", C.c_double), ("obs_index", C.c_int), ("robot", C.c_int), ("segment", C.c_int), ("flags", C.c_int)]


PROFILE_FLAGS = dict(hover=1, obs_contact=2, pair_contact=4, speed=8, accel=16)
PROFILE_MAX_SAMPLES = 65536     # TJ_PROFILE_MAX_SAMPLES
PROFILE_MAX_RECORDS = 1 << 24   # TJ_PROFILE_MAX_RECORDS


def profile_grid(piece_time, P, samples=None):
    """the default time grid of flight_profile: t_k = (k / (K - 1)) * the longest robot's duration, K = samples (None: 101; K == 1: t = 0); a robot's duration is
    log_data's sum of piece_num times 1.0 * piece_time"""
    K = 101 if samples is None else int(samples)
    longest = 0.0
    for pt in np.asarray(piece_time, dtype=np.float64).ravel():
        dur = 0.0
        for _ in range(P):
            dur += 1.0 * float(pt)
        longest = max(longest, dur)
    return np.array([(k / (K - 1)) * longest if K > 1 else 0.0 for k in range(K)], dtype=np.float64)


def _flight_profile(call, piece_times, U, P, times, samples):
    """shared by Solver.flight_profile / Group.flight_profile: call(times, n_times, records) -> dict of numpy arrays [U][K]"""
    if times is None:
        times = profile_grid(piece_times(), P, samples)
    elif samples is not None:
        raise ValueError("flight_profile: give times or samples, not both")
    t = np.ascontiguousarray(times, dtype=np.float64).ravel()
    K = t.size
    rec = (TjProfileSample * max(U * K, 1))()
    call(_d(t), C.c_int(K), rec)
    a = np.frombuffer(rec, dtype=np.dtype(TjProfileSample), count=U * K).reshape(U, K)
    return {n: np.array(a[n], dtype=np.float64 if ty is C.c_double else np.int32) for n, ty in TjProfileSample._fields_}


def merge_pairs(rows, rng, offset):
    """the directed rows of pair_approach -> one row per unordered pair a < b (`robot` = a, `partner` = b) with a listed direction: lo = min, hi = min over
    the two directions, a missing direction counting as `rng` (an unlisted direction is certified at least rng apart, so the merge is sound); `time`,
    `segment` and `of` (whose flight the hi sample belongs to) from the direction with the smaller hi, on equality from (a, b); depth = max, windows = sum;
    contact / truncated of either direction, clear / converged of both (a missing direction is converged, and clear iff rng > offset).  Pure numpy."""
    u, q = rows["robot"].astype(np.int64), rows["partner"].astype(np.int64)
    a, b = np.minimum(u, q), np.maximum(u, q)
    span = int(b.max()) + 1 if len(b) else 1
    key, ikey = np.unique(a * span + b, return_inverse=True)
    n = len(key)
    fwd, bwd = np.full(n, -1), np.full(n, -1)        # row index of (a, b) and of (b, a), -1: not listed
    fwd[ikey[u < q]] = np.flatnonzero(u < q); bwd[ikey[u > q]] = np.flatnonzero(u > q)
    either, both = PAIR_FLAGS["contact"] | PAIR_FLAGS["truncated"], PAIR_FLAGS["clear"] | PAIR_FLAGS["converged"]
    absent = dict(lo=rng, hi=rng, depth=0, windows=0, flags=PAIR_FLAGS["converged"] | (PAIR_FLAGS["clear"] if rng > offset else 0))

    def side(ix, name):
        v = rows[name][np.maximum(ix, 0)] if len(rows[name]) else np.zeros(n, dtype=rows[name].dtype)
        return np.where(ix >= 0, v, absent[name]) if name in absent else v

    take_f = (fwd >= 0) & ((bwd < 0) | (side(fwd, "hi") <= side(bwd, "hi")))
    src = np.where(take_f, fwd, bwd)
    ff, fb = side(fwd, "flags").astype(np.int32), side(bwd, "flags").astype(np.int32)
    return dict(robot=(key // span).astype(np.int32), partner=(key % span).astype(np.int32), lo=np.minimum(side(fwd, "lo"), side(bwd, "lo")),
                hi=np.minimum(side(fwd, "hi"), side(bwd, "hi")), time=side(src, "time"), segment=side(src, "segment"),
                of=np.where(take_f, key // span, key % span).astype(np.int32), depth=np.maximum(side(fwd, "depth"), side(bwd, "depth")).astype(np.int32),
                windows=(side(fwd, "windows") + side(bwd, "windows")).astype(np.int32), flags=((ff | fb) & either) | (ff & fb & both))


def _pair_approach(call, params, range, tol, max_depth, max_windows, symmetric):
    """shared by Solver.pair_approach / Group.pair_approach: call(range, tol, max_depth, max_windows, rows, cap, n)"""
    rows = _listed_rows(TjPairRecord, call, _search_args(range, tol, max_depth, max_windows))
    if not symmetric:
        return rows
    rng = float(range) if range is not None and range > 0 else params["offset"] + 2 * params["margin"]
    return merge_pairs(rows, rng, params["offset"])


def _path_crossings(call, range, tol, max_depth, max_windows):
    """shared by Solver.path_crossings / Group.path_crossings: call(range, tol, max_depth, max_windows, rows, cap, n); `gap` = partner_time - time, the timing
    margin of the crossing (0.0 where the pair is listed for its lo only)."""
    rows = _listed_rows(TjCrossingRecord, call, _search_args(range, tol, max_depth, max_windows))
    rows["gap"] = rows["partner_time"] - rows["time"]
    return rows


def _timing_margin(call, dist, max_slip, tol, max_depth, max_windows):
    """shared by Solver.timing_margin / Group.timing_margin: call(dist, max_slip, tol, max_depth, max_windows, rows, cap, n)"""
    d, t, md, mw = _search_args(dist, tol, max_depth, max_windows)
    return _listed_rows(TjMarginRecord, call, (d, C.c_double(0.0 if max_slip is None else float(max_slip)), t, md, mw))


def _proximity_windows(call, check, dist, tol, max_depth, max_windows):
    """shared by Solver.proximity_windows / Group.proximity_windows: call(dist, tol, max_depth, max_windows, rows, cap, n_pairs, n) -> the C side's return value,
    check(rc) raises on an error.  The count-only call sizes cap by the listed pairs; more rows than that (TJ_ERR_CAPACITY with the exact n) take one more call"""
    args = _search_args(dist, tol, max_depth, max_windows)
    pairs, n = C.c_int(0), C.c_int(0)
    check(call(*args, None, C.c_int(0), C.byref(pairs), C.byref(n)))
    cap = pairs.value
    rec = (TjProximityRow * max(cap, 1))()
    if cap:
        rc = call(*args, rec, C.c_int(cap), C.byref(pairs), C.byref(n))
        if rc == -3 and n.value > cap:
            cap = n.value
            rec = (TjProximityRow * cap)()
            rc = call(*args, rec, C.c_int(cap), C.byref(pairs), C.byref(n))
        check(rc)
    out = _records(TjProximityRow, rec[:max(n.value, 0)])
    out["n_pairs"] = pairs.value
    return out


class TrajAdmmError(RuntimeError):
    pass


# the known-answer hooks (include/trajadmm_kat.h) live in a TEST build of the same translation unit, never in the product library
KAT_EXPORTS = ["tj_kat_gjk", "tj_kat_gjk_wave", "tj_kat_gjk_wave_split", "tj_kat_planes", "tj_kat_ccd", "tj_kat_tri", "tj_kat_kdop_wave", "tj_kat_query", "tj_kat_query_form", "tj_kat_linalg", "tj_kat_plan", "tj_kat_launches", "tj_kat_set_local_grad", "tj_kat_get_hull_record", "tj_kat_get_swept_record", "tj_kat_arrays"]
KAT_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libtrajadmm_kat.so")
_lib = None
_kat_lib = None


def _open(path):
    if not os.path.exists(path):
        raise TrajAdmmError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(path)
    lib.tj_last_error.restype = C.c_char_p
    lib.tj_stream.restype = C.c_void_p
    lib.tj_group_last_error.restype = C.c_char_p
    lib.tj_group_ctx.restype = C.c_void_p
    return lib


def load_library(kat=False):
    """dlopen libtrajadmm.so (built by __graft_entry__.build() / csrc/Makefile).  Raises if absent.  kat=True: the test build
    libtrajadmm_kat.so (same sources + the tj_kat_* hooks), unless TRAJADMM_LIB points somewhere else."""
    global _lib, _kat_lib
    if kat and "TRAJADMM_LIB" not in os.environ:
        if _kat_lib is None:
            _kat_lib = _open(KAT_LIB_PATH)
        return _kat_lib
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def host_tables(piece_num, res=8):
    """(convert[P,6,6], mdyn[6,6], basis[P*res,6,6], kdop[49,3]) as the library precomputes them on the host
    (tj_host_tables; needs no GPU).  Row-major [row, col]."""
    lib = load_library()
    conv = np.zeros((piece_num, 6, 6)); M = np.zeros((6, 6)); basis = np.zeros((piece_num * res, 6, 6)); kd = np.zeros((49, 3))
    rc = lib.tj_host_tables(C.c_int(piece_num), C.c_int(res), _d(conv), _d(M), _d(basis), _d(kd))
    if rc < 0:
        raise TrajAdmmError(f"tj_host_tables failed ({rc})")
    return conv, M, basis, kd


def _i(a):
    return a.ctypes.data_as(_ip)


# the launch plan's record (tj_kat_plan, csrc/host_plan.h: plan_record): the device facts, then the plan
PLAN_FACTS = ("num_cu", "xsolve_ok", "xsolve_regs", "xsolve_lds", "grad_ok", "grad_regs", "grad_lds", "grad_fold_ok", "grad_fold_regs", "grad_fold_lds",
              "front_ok", "front_regs", "front_lds", "counters_on", "claim_refused", "prim", "n_obs")
PLAN_FIELDS = ("err", "mode", "U", "P", "res", "S", "T", "N", "prim", "u0", "u1", "rank", "world", "fuse", "xf", "xf_all", "cap_obs", "cap_self", "cap_pairs", "optimal_plane",
               "pair_rows", "cap_work", "xs", "grad_npl", "xs_band", "seq_tree", "bvh_skip", "pair_prio", "mid_order", "pair_lpw", "pair_pass_on", "spec", "seq_fold", "spec_budget",
               "spec_min", "ls_fast", "num_cu", "c2_fold", "grad_bal", "xs_async", "keep_async", "keep_waves", "ls_help", "ls_help_late", "ls_help_mute", "fa",
               "grad_fold", "n_solve_env", "lsc_wide", "fa_emulate", "fa_mid_ok", "fa_mid_front", "hwq_refused", "queues", "forced", "xs_two_queues", "keep_two_queues", "heal", "xs_fault",
               "lds_grad", "lds_xs", "lds_xs2", "lds_ls", "lds_seq", "lsl_total", "lsl_plane_cap", "lsl_affine", "lsl_groups",
               "n_rows", "n_ccd", "n_xf", "n_front", "n_solve", "n_obs_solve", "n_mid_slack")


def plan_record(params=None, facts=None, ctx=None):
    """(facts, plan, message) of a context (ctx: its tj_ctx pointer) or -- no GPU needed -- of the pure planner on a TjParams and a dict of PLAN_FACTS."""
    lib = load_library(kat=True)
    f = np.array([facts[k] for k in PLAN_FACTS] if facts else [0] * len(PLAN_FACTS), dtype=np.int32)
    out = np.zeros(len(PLAN_FACTS) + len(PLAN_FIELDS), dtype=np.int32)
    msg = C.create_string_buffer(512)
    n = lib.tj_kat_plan(ctx, C.byref(params) if params is not None else None, _i(f), _i(out), C.c_int(out.size), msg, C.c_int(512))
    if n != out.size:
        raise TrajAdmmError(f"tj_kat_plan returned {n}, the package knows {out.size} entries")
    v = [int(x) for x in out]
    return dict(zip(PLAN_FACTS, v)), dict(zip(PLAN_FIELDS, v[len(PLAN_FACTS):])), msg.value.decode()


# the declaration table of a context's device arrays (tj_kat_arrays, csrc/tj_api.hip: device_arrays): per array its name and these
ARRAY_FIELDS = ("n", "elem", "snap", "reset")   # element count, element size, part of the checkpoint, what tj_init_state fills it with (0 nothing, 1 zero bytes, 2 one bytes)


def arrays_record(params=None, facts=None, ctx=None):
    """[(name, n, elem, snap, reset), ...] of a context (ctx: its tj_ctx pointer) or -- no GPU needed -- of the planner's Dev on a TjParams and a dict of PLAN_FACTS."""
    lib = load_library(kat=True)
    f = np.array([facts[k] for k in PLAN_FACTS] if facts else [0] * len(PLAN_FACTS), dtype=np.int32)
    out = np.zeros(4 * 256, dtype=np.int32)
    names = C.create_string_buffer(8192)
    n = lib.tj_kat_arrays(ctx, C.byref(params) if params is not None else None, _i(f), _i(out), C.c_int(out.size), names, C.c_int(8192))
    if n <= 0:
        raise TrajAdmmError(f"tj_kat_arrays returned {n}")
    return [(name,) + tuple(int(x) for x in out[4 * i:4 * i + 4]) for i, name in enumerate(names.value.decode().split(","))]


# the launch sequence's records (tj_kat_launches, csrc/host_launch.h): SchedState, Launch, the ids beyond the K_* kernels, the schedules
SCHED_STATE = ("xs_seq", "xs_seq_gated", "keep_seq", "fa_seq", "fa_armed", "fa_mid_now", "hull_from_units", "xs_two_queues", "keep_two_queues", "xs_same_queue_now", "xs_fault",
               "xf_used0", "xf_used1", "ccd_valid", "ck_in_begin", "xch_wait_kernel", "lsc_base")
LAUNCH_FIELDS = ("kid", "form", "prim", "queue", "grid", "block", "lds", "arg0", "arg1", "arg2", "arg3",
                 "xs_async", "keep_async", "fa", "xs_seq", "keep_seq", "fa_seq", "fa_mid", "fa_units", "fa_nfront", "fa_nls", "c2_fold")
KERNELS = ("k_begin", "k_hullinfo", "k_front", "k_obs_query", "k_sep_self_rows", "k_mid", "k_obs_solve", "k_sep_self_solve", "k_keep", "k_sep_self_compact", "k_grad", "k_xsolve",
           "k_xsolve_c2", "k_ccd_prep", "k_ccd", "k_ccd_obs", "k_ccd_self_pairs", "k_ccd_self_seq", "k_linesearch", "k_ls_coupled", "k_ls_commit", "k_slack")   # tj_kernel_name, in id order
LAUNCH_EXTRA = ("k_xs_gate", "k_keep_gate", "k_fa_gate", "k_xch_wait", "xf_seg_clear")   # kid = len(KERNELS) + index; the last one is a memset, not a kernel
SCHED_STAGE, SCHED_CHAIN, SCHED_PHASE = 0, 1, 2


def launch_records(calls, state=None, params=None, facts=None, follow=0, ctx=None):
    """What the schedules enqueue for calls = [(kid, sched, chain_pos), ...] (tj_kat_launches; nothing is launched): (start state, [(exists, state after, [launch, ...]), ...]), states
    and launches as lists of ints in the order of SCHED_STATE / LAUNCH_FIELDS.  ctx: a context's own Dev, plan and state; else -- no GPU needed -- the planner's on a TjParams and a
    dict of PLAN_FACTS, from the start state given.  With ctx, of `state` only xs_same_queue_now is read (nonzero: the sequence of tj_profile_kernels)"""
    lib = load_library(kat=True)
    ns, nl = len(SCHED_STATE), len(LAUNCH_FIELDS)
    f = np.array([facts[k] for k in PLAN_FACTS] if facts else [0] * len(PLAN_FACTS), dtype=np.int32)
    st = np.array(list(state) if state is not None else [0] * ns, dtype=np.int32)
    cl = np.array(calls, dtype=np.int32).reshape(-1, 3)
    out = np.zeros(len(cl) * (2 + ns + 8 * nl) + 1, dtype=np.int32)
    n = lib.tj_kat_launches(ctx, C.byref(params) if params is not None else None, _i(f), C.c_int(follow), _i(st), _i(cl), C.c_int(len(cl)), _i(out), C.c_int(out.size))
    if n <= 0 and len(cl):
        raise TrajAdmmError(f"tj_kat_launches returned {n}")
    v, res, at = [int(x) for x in out[:n]], [], 0
    for _ in range(len(cl)):
        k = v[at + 1]
        body = at + 2 + ns
        res.append((v[at], v[at + 2:body], [v[body + i * nl:body + (i + 1) * nl] for i in range(k)]))
        at = body + k * nl
    if at != n:
        raise TrajAdmmError(f"tj_kat_launches wrote {n} ints, the package read {at}")
    return [int(x) for x in st], res


class Solver:
    """One ADMM problem resident on one GPU (one `tj_ctx`)."""

    def __init__(self, scene, params=None, device=0, rank=0, world=1, stop=None, kat=False, **caps):
        self.lib = load_library(kat)          # kat=True: the test build with the known-answer hooks (kat_* methods)
        p = dict(scenes.DEFAULT_PARAMS)
        if params:
            p.update(params)
        self.params = p
        self.mode, self.U, self.P = scene["mode"], scene["U"], scene["P"]
        self.res = p["res"]
        self.S, self.T = self.P * self.res, 3 * self.P + 3
        self.box_bytes, self.prim_vertices = 24, 1   # BVH box record; vertices per obstacle primitive (bench.py's byte model)
        tp = TjParams()
        self.lib.tj_default_params(C.byref(tp), self.mode, self.U, self.P)
        tp.res = self.res
        tp.lambda_, tp.margin, tp.offset, tp.mu = p["lam"], p["margin"], p["offset"], p["mu"]
        tp.vel_limit, tp.acc_limit, tp.ks, tp.kt = p["vel_limit"], p["acc_limit"], scene["ks"], p["kt"]
        tp.stop = p["stop"] if stop is None else stop
        tp.device, tp.rank, tp.world = device, rank, world
        for k, v in caps.items():
            setattr(tp, k, v)
        self._ctx = C.c_void_p()
        rc = self.lib.tj_create(C.byref(tp), C.byref(self._ctx))
        self._check(rc)
        if scene.get("tris") is not None:   # obstacle triangles [N][3][3] (BASELINE config 5): tj_set_mesh with an unshared vertex list
            verts = np.ascontiguousarray(scene["tris"], dtype=np.float64).reshape(-1, 3)
            self.N = verts.shape[0] // 3
            faces = np.arange(3 * self.N, dtype=np.int32).reshape(-1, 3)
            self._check(self.lib.tj_set_mesh(self._ctx, _d(verts), C.c_int(3 * self.N), _i(faces), C.c_int(self.N)))
            self.prim_vertices = 3
        else:
            cloud = np.ascontiguousarray(scene["cloud"], dtype=np.float64).reshape(-1, 3)
            self.N = cloud.shape[0]
            self._check(self.lib.tj_set_cloud(self._ctx, _d(cloud), C.c_int(self.N)))
        self._wp = np.ascontiguousarray(scene["waypoints"], dtype=np.float64)
        self._pt0 = float(p["piece_time0"])
        self.reset()

    def reset(self):
        """init_variable: back to the initial trajectory, iteration counter 0."""
        self._check(self.lib.tj_init_state(self._ctx, _d(self._wp), C.c_double(self._pt0)))

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self.lib.tj_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.tj_last_error(self._ctx).decode() if self._ctx.value else "tj_create failed"
            raise TrajAdmmError(f"libtrajadmm error {rc}: {msg}")
        return rc

    # ---- state ---------------------------------------------------------------------------
    def get_state(self):
        U, P, T = self.U, self.P, self.T
        st = dict(spline=np.zeros((U, 3, T)), p_slack=np.zeros((U, 3, 6 * P)), p_lambda=np.zeros((U, 3, 6 * P)),
                  t_slack=np.zeros((U, P)), t_lambda=np.zeros((U, P)), piece_time=np.zeros(U))
        for u in range(U):
            pt = C.c_double()
            self._check(self.lib.tj_get_state(self._ctx, u, _d(st["spline"][u]), _d(st["p_slack"][u]), _d(st["p_lambda"][u]),
                                              _d(st["t_slack"][u]), _d(st["t_lambda"][u]), C.byref(pt)))
            st["piece_time"][u] = pt.value
        return st

    def set_state(self, st):
        for u in range(self.U):
            a = [np.ascontiguousarray(st[k][u], dtype=np.float64) for k in ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda")]
            self._check(self.lib.tj_set_state(self._ctx, u, _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), _d(a[4]), C.c_double(float(st["piece_time"][u]))))

    # ---- hot path ------------------------------------------------------------------------
    def iterate(self, n=1):
        """n ADMM iterations on the device; returns (gnorm, iter, converged)."""
        g, it, cv = C.c_double(), C.c_int(), C.c_int()
        self._check(self.lib.tj_iterate(self._ctx, C.c_int(n), C.byref(g), C.byref(it), C.byref(cv)))
        return g.value, it.value, bool(cv.value)

    def iterate_async(self, n=1):
        self._check(self.lib.tj_iterate_async(self._ctx, C.c_int(n)))

    def sync(self):
        self._check(self.lib.tj_sync(self._ctx))

    def stream(self):
        return self.lib.tj_stream(self._ctx)

    def set_stream(self, hip_stream):
        self._check(self.lib.tj_set_stream(self._ctx, C.c_void_p(hip_stream)))

    def profile_kernels(self, n):
        """{kernel name: (device ms summed over n iterations, launches)} measured with hipEvents on the solver's stream"""
        self.lib.tj_kernel_name.restype = C.c_char_p
        nk = self.lib.tj_kernel_count()
        ms = np.zeros(nk); ln = np.zeros(nk, dtype=np.int32)
        self._check(self.lib.tj_profile_kernels(self._ctx, C.c_int(n), _d(ms), _i(ln)))
        return {self.lib.tj_kernel_name(i).decode(): (float(ms[i]), int(ln[i])) for i in range(nk)}

    def run_stage(self, name):
        self._check(self.lib.tj_run_stage(self._ctx, C.c_int(STAGES[name])))

    def phase_count(self):
        return self._check(self.lib.tj_phase_count(self._ctx))

    def launch_count(self):
        self.lib.tj_launch_count.restype = C.c_longlong
        return int(self.lib.tj_launch_count(self._ctx))

    def iterate_phase(self, phase, more=0):
        """more: another iteration follows in this batch (decoupled schedules then fold its begin into this one's line search)"""
        self._check(self.lib.tj_iterate_phase_chained(self._ctx, C.c_int(phase), C.c_int(1 if more else 0)))

    def set_coupled_follow(self, on=True):
        """coupled mode, sharded context: follow the Armijo search beyond the candidates one exchange carries (ask coupled_search_pending() after phase 5)"""
        self._check(self.lib.tj_set_coupled_follow(self._ctx, C.c_int(1 if on else 0)))

    def coupled_search_pending(self):
        p = C.c_int()
        self._check(self.lib.tj_coupled_search_pending(self._ctx, C.byref(p)))
        return bool(p.value)

    # ---- direct exchange between processes (include/trajadmm.h tj_xch_*) ----
    def xch_ipc_export(self):
        h = (C.c_ubyte * 64)()
        self._check(self.lib.tj_xch_ipc_export(self._ctx, h))
        return bytes(h)

    def xch_attach_ipc(self, handles, poll_in_kernel=True):
        """handles: {rank: 64-byte handle} of every OTHER rank; opens them, attaches and switches the direct exchange on"""
        ranks = sorted(handles)
        bases = (C.c_void_p * len(ranks))()
        for i, r in enumerate(ranks):
            b = C.c_void_p()
            hb = (C.c_ubyte * 64).from_buffer_copy(handles[r])
            self._check(self.lib.tj_xch_ipc_open(self._ctx, hb, C.byref(b)))
            bases[i] = b.value
        rk = np.ascontiguousarray(ranks, dtype=np.int32)
        self._check(self.lib.tj_xch_attach(self._ctx, C.c_int(len(ranks)), _i(rk), bases))
        self._check(self.lib.tj_xch_enable(self._ctx, C.c_int(1), C.c_int(1 if poll_in_kernel else 0)))

    def xch_enable(self, on, poll_in_kernel=True):
        self._check(self.lib.tj_xch_enable(self._ctx, C.c_int(1 if on else 0), C.c_int(1 if poll_in_kernel else 0)))

    # ---- stage-level views (same shapes as oracle.pyoracle.Engine) ---------------------------
    def stage_planes(self):
        self.run_stage("begin")
        self.run_stage("planes_obs")
        self.run_stage("planes_self")
        return self.get_planes()

    def get_planes(self):
        counts = np.zeros((self.U, self.S), dtype=np.int32)
        chunks = []
        for u in range(self.U):
            co = np.zeros(self.S, dtype=np.int32); cs = np.zeros(self.S, dtype=np.int32)
            n = self._check(self.lib.tj_get_planes(self._ctx, u, _i(co), _i(cs), None, 0))
            buf = np.zeros((max(n, 1), 4))
            self._check(self.lib.tj_get_planes(self._ctx, u, _i(co), _i(cs), _d(buf), C.c_int(n)))
            counts[u] = co + cs
            chunks.append(buf[:n])
        return counts, np.concatenate(chunks, axis=0)

    def get_candidates(self, u, cap=4096):
        """per segment: (obstacle ids that passed box query + k-DOP cull, number the box query alone returned since reset)"""
        out = []
        for tr in range(self.S):
            ids = np.zeros(cap, dtype=np.int32); nb = C.c_int()
            n = self._check(self.lib.tj_get_candidates(self._ctx, C.c_int(u), C.c_int(tr), C.c_int(cap), _i(ids), C.byref(nb)))
            out.append((ids[:n].copy(), nb.value))
        return out

    def set_planes(self, counts, planes):
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(self.U, self.S)
        planes = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        w = 0
        for u in range(self.U):
            n = int(counts[u].sum())
            blk = np.ascontiguousarray(planes[w:w + n]) if n else np.zeros((1, 4))
            self._check(self.lib.tj_set_planes(self._ctx, u, _i(np.ascontiguousarray(counts[u])), _d(blk)))
            w += n

    def stage_direction(self):
        self.run_stage("grad")
        self.run_stage("xsolve")
        out = dict(direction=np.zeros((self.U, 3, self.T)), t_direction=np.zeros(self.U), wolfe=np.zeros(self.U), gn=np.zeros(self.U))
        for u in range(self.U):
            a, b, c = C.c_double(), C.c_double(), C.c_double()
            self._check(self.lib.tj_get_direction(self._ctx, u, _d(out["direction"][u]), C.byref(a), C.byref(b), C.byref(c)))
            out["t_direction"][u], out["wolfe"][u], out["gn"][u] = a.value, b.value, c.value
        out["gnorm"] = float(np.sum(out["gn"]) / self.U) if self.mode == 1 else float(out["gn"][0])
        return out

    def get_direction(self, u):
        """robot u's direction record as the last Newton solve left it: (direction [3][T], t_direction, wolfe, gn)"""
        d = np.zeros((3, self.T)); t, w, g = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.tj_get_direction(self._ctx, C.c_int(u), _d(d), C.byref(t), C.byref(w), C.byref(g)))
        return d, t.value, w.value, g.value

    def set_direction(self, u, direction, t_direction, wolfe, gn):
        d = np.ascontiguousarray(direction, dtype=np.float64)
        self._check(self.lib.tj_set_direction(self._ctx, C.c_int(u), _d(d), C.c_double(t_direction), C.c_double(wolfe), C.c_double(gn)))

    def local_grad(self, u, sp):
        g = np.zeros(19); h = np.zeros((19, 19))
        self._check(self.lib.tj_get_local_grad(self._ctx, u, sp, _d(g), _d(h)))
        return g, h

    def stage_steps(self):
        self.run_stage("ccd_prep")
        self.run_stage("ccd_obs")
        self.run_stage("ccd_self")
        a = np.zeros(self.U); b = np.zeros(self.U)
        self._check(self.lib.tj_get_steps(self._ctx, _d(a), _d(b), None))
        return a, b

    def stage_linesearch(self):
        self.run_stage("linesearch")
        s = np.zeros(self.U)
        self._check(self.lib.tj_get_steps(self._ctx, None, None, _d(s)))
        return s

    def last_armijo_steps(self):
        """accepted Armijo step of every robot in the last iteration (diagnostic; tj_get_steps)"""
        s = np.zeros(self.U)
        self._check(self.lib.tj_get_steps(self._ctx, None, None, _d(s)))
        return s

    def stage_slack(self):
        self.run_stage("slack")
        self.run_stage("end")

    def stage_update_spline(self):
        """coupled mode (scene mode 2): Optimization3D_multi::update_spline as one stage -- arrowhead Newton
        system, CCD clamps, Armijo search on the summed energy, commit.  Returns (gnorm, wolfe)."""
        for st in ("grad", "xsolve", "ccd_prep", "ccd_obs", "ccd_self", "linesearch"):
            self.run_stage(st)
        t, w, g = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.tj_get_direction(self._ctx, 0, None, C.byref(t), C.byref(w), C.byref(g)))
        return g.value, w.value

    # ---- known-answer hooks (device primitives on caller batches) -------------------------------
    def _kat_gjk(self, fn, a, b, k, *extra):
        """the three GJK hooks: bodies a[n][n1][3], b[n][n2][3] in, (n, k) out"""
        a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        n = a.shape[0]; out = np.zeros((n, k))
        self._check(fn(self._ctx, C.c_int(n), C.c_int(a.shape[1]), _d(a), C.c_int(b.shape[1]), _d(b), *extra, _d(out)))
        return out

    def kat_gjk(self, a, b):
        return self._kat_gjk(self.lib.tj_kat_gjk, a, b, 3)

    def kat_gjk_wave(self, a, b):
        return self._kat_gjk(self.lib.tj_kat_gjk_wave, a, b, 3)

    def kat_gjk_wave_split(self, a, b, k_stop):
        """gjk_wave interrupted after k_stop iterations and continued from the state it left in memory: (witness vectors, iterations)"""
        out = self._kat_gjk(self.lib.tj_kat_gjk_wave_split, a, b, 4, C.c_int(k_stop))
        return out[:, :3], out[:, 3].astype(int)

    def _kat_rows(self, fn, arrays, k, head=(), mid=(), tail=()):
        """the hooks that take a list of float64 arrays of n cases each and give (n, k): fn(ctx, *head, n, *mid, *arrays, *tail, out)"""
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in arrays]
        n = arrs[0].shape[0]; out = np.zeros((n, k))
        self._check(fn(self._ctx, *head, C.c_int(n), *mid, *[_d(x) for x in arrs], *tail, _d(out)))
        return out

    def kat_hull_record(self):
        """the hull cache as its last writer left it: (hullinfo [U][S][122], hbox [S][6][U])"""
        info = np.zeros((self.U, self.S, 122)); hbox = np.zeros((self.S, 6, self.U))
        self._check(self.lib.tj_kat_get_hull_record(self._ctx, _d(info), _d(hbox)))
        return info, hbox

    # the swept-hull record's fields (csrc/dev_common.h: CCD_P .. CCD_KHI, CCD_REC), as slices of a record tj_kat_get_swept_record returns
    SWEPT_FIELDS = dict(P=slice(0, 18), D=slice(18, 36), obs_box=slice(36, 42), pair_box=slice(42, 48), k_lo=slice(48, 97), k_hi=slice(97, 146))
    SWEPT_REC = 146

    def kat_swept_record(self):
        """the swept-hull cache as its last writer left it: (ccdinfo [U][S][SWEPT_REC], cbox [S][6][U])"""
        info = np.zeros((self.U, self.S, self.SWEPT_REC)); cbox = np.zeros((self.S, 6, self.U))
        self._check(self.lib.tj_kat_get_swept_record(self._ctx, _d(info), _d(cbox)))
        return info, cbox

    def kat_planes(self, what, P, Q, dist):
        return self._kat_rows(self.lib.tj_kat_planes, (P, Q), 5, head=(C.c_int(what),), tail=(C.c_double(dist),))

    def kat_refine_planes(self, what, P, Q, cd):
        """what 5: Optimal_plane::optimal_cd (Q = points), 6: self_optimal_cd (Q = hulls); cd[n][4] = planes to refine.
        Returns (finished[n], refined cd[n][4])."""
        P = np.ascontiguousarray(P, dtype=np.float64); Q = np.ascontiguousarray(Q, dtype=np.float64)
        n = P.shape[0]; out = np.zeros((n, 5)); out[:, 1:] = cd
        self._check(self.lib.tj_kat_planes(self._ctx, C.c_int(what), C.c_int(n), _d(P), _d(Q), C.c_double(0.0), _d(out)))
        return out[:, 0] != 0, out[:, 1:].copy()

    # ---- "optimal_plane":1 : the persistent plane tables ----
    def get_obs_cache(self, u=0, cap=4096):
        """single UAV: per segment (ids into the scene's cloud, planes (c, d)) in insertion order"""
        out = []
        for tr in range(self.S):
            ids = np.zeros(cap, dtype=np.int32); cd = np.zeros((cap, 4))
            n = self.lib.tj_get_obs_cache(self._ctx, C.c_int(u), C.c_int(tr), C.c_int(cap), _i(ids), _d(cd))
            self._check(n)
            assert n <= cap
            out.append((ids[:n].copy(), cd[:n].copy()))
        return out

    def set_obs_cache(self, cache, u=0):
        for tr, (ids, cd) in enumerate(cache):
            ids = np.ascontiguousarray(ids, dtype=np.int32); cd = np.ascontiguousarray(cd, dtype=np.float64).reshape(-1, 4)
            self._check(self.lib.tj_set_obs_cache(self._ctx, C.c_int(u), C.c_int(tr), C.c_int(len(ids)), _i(ids), _d(cd)))

    def get_pair_cache(self):
        """multi UAV: flags [S][U][U] (p0 < p1) and planes [S][U][U][4] = (c, d) before the offset/2 split"""
        fl = np.zeros((self.S, self.U, self.U), dtype=np.int32); cd = np.zeros((self.S, self.U, self.U, 4))
        self._check(self.lib.tj_get_pair_cache(self._ctx, _i(fl), _d(cd)))
        return fl, cd

    def set_pair_cache(self, flags, cd):
        fl = np.ascontiguousarray(flags, dtype=np.int32); cd = np.ascontiguousarray(cd, dtype=np.float64)
        self._check(self.lib.tj_set_pair_cache(self._ctx, _i(fl), _d(cd)))

    # ---- initial-trajectory planner (replaces ompl_init / simplify_path / edge_collision) ----
    def edge_collision(self, edges, prior=None, d=None):
        """the reference's motion validator on a batch of straight edges [n][2][3] -> bool[n]"""
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1, 6)
        prior = np.zeros((0, 6)) if prior is None else np.ascontiguousarray(prior, dtype=np.float64).reshape(-1, 6)
        d = self.params["offset"] + 0.5 * self.params["margin"] if d is None else d
        hit = np.zeros(max(len(edges), 1), dtype=np.int32)
        self._check(self.lib.tj_edge_collision(self._ctx, C.c_int(len(edges)), _d(edges), C.c_int(len(prior)), _d(prior), C.c_double(d), _i(hit)))
        return hit[:len(edges)].astype(bool)

    def plan_init(self, starts, goals, nodes=0, min_waypoints=0, bound_scale=0.0, cap=256):
        """way points [n_robots][n][3] from start/goal pairs (tj_plan_init); n is common to all robots"""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3); goals = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        U = len(starts); wp = np.zeros((U, cap, 3)); n = C.c_int()
        self._check(self.lib.tj_plan_init(self._ctx, C.c_int(U), _d(starts), _d(goals), C.c_double(bound_scale), C.c_int(nodes), C.c_int(min_waypoints), C.c_int(cap), _d(wp), C.byref(n)))
        return wp[:, :n.value].copy()

    def kat_ccd(self, P, D, Q, E, q, tu, d):
        return self._kat_rows(self.lib.tj_kat_ccd, (P, D, Q, E, q, tu), 2, tail=(C.c_double(d),))

    def kat_query(self, boxes, margin, cap=2048, sort=True, unroll=4, pre=False):
        """raw broad-phase candidate SETS of caller-supplied query boxes [nq][6] (lo, hi): list of sorted id arrays (sort=False: in the walk's own order).
        unroll / pre: the form of the walk (tj_kat_query_form: 4 / False is the plane query's walk without a prefetched top box, tj_kat_query)"""
        boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
        nq = boxes.shape[0]; counts = np.zeros(nq, dtype=np.int32); ids = np.zeros((nq, cap), dtype=np.int32)
        if unroll == 4 and not pre:     # (tj_kat_query is tj_kat_query_form at 4 / 0: called by its own name so that both exports stay exercised)
            self._check(self.lib.tj_kat_query(self._ctx, C.c_int(nq), _d(boxes), C.c_double(margin), C.c_int(cap), _i(counts), _i(ids)))
        else:
            self._check(self.lib.tj_kat_query_form(self._ctx, C.c_int(nq), _d(boxes), C.c_double(margin), C.c_int(cap), C.c_int(unroll), C.c_int(bool(pre)), _i(counts), _i(ids)))
        return [np.sort(ids[q, :counts[q]]) if sort else ids[q, :counts[q]].copy() for q in range(nq)]

    def kat_tri(self, P, D, tri, t, dist, off):
        return self._kat_rows(self.lib.tj_kat_tri, (P, D, tri, t), 8, tail=(C.c_double(dist), C.c_double(off)))

    def kat_kdop_wave(self, P, bodies, d, D=None, t=None, nc=None):
        """the obstacle 49-axis cull as the walks run it, one wave per case: P[n][6][3], bodies[n][per][prim][3] (prim 1 or 3, per <= 64) -> pass[n][per];
        D, t: the swept hull conv{P, P + t D}; nc[n]: only the first nc[i] candidates of case i take part"""
        P = np.ascontiguousarray(P, dtype=np.float64); bodies = np.ascontiguousarray(bodies, dtype=np.float64)
        n, per, prim = bodies.shape[:3]
        swept = D is not None
        D = np.ascontiguousarray(D, dtype=np.float64) if swept else None; t = np.ascontiguousarray(t, dtype=np.float64) if swept else None
        nc = None if nc is None else np.ascontiguousarray(nc, dtype=np.int32)
        out = np.zeros((n, per))
        self._check(self.lib.tj_kat_kdop_wave(self._ctx, C.c_int(prim), C.c_int(swept), C.c_int(n), C.c_int(per), _d(P), _d(D) if swept else None, _d(t) if swept else None,
                                              _d(bodies), None if nc is None else _i(nc), C.c_double(d), _d(out)))
        return out

    def kat_linalg(self, mats):
        return self._kat_rows(self.lib.tj_kat_linalg, (mats,), 2, mid=(C.c_int(np.shape(mats)[1]),))

    def kat_set_local_grad(self, lg, lh):
        """the per-piece blocks of the whole fleet from the host (tj_kat_set_local_grad): lg[U][P][19], lh[U][P][19][19] -- what local_grad reads back and
        run_stage("xsolve") solves"""
        lg = np.ascontiguousarray(lg, dtype=np.float64); lh = np.ascontiguousarray(lh, dtype=np.float64)
        if lg.size != self.U * self.P * 19 or lh.size != self.U * self.P * 361:
            raise ValueError(f"kat_set_local_grad: lg[{self.U}][{self.P}][19] and lh[{self.U}][{self.P}][361] expected")
        self._check(self.lib.tj_kat_set_local_grad(self._ctx, _d(lg), _d(lh)))

    def energy(self):
        """Energy_admm::spline_energy of every owned robot at the current state (planes of the last iteration).  It is the line search's own evaluation: k_energy
        stages what k_linesearch stages and calls x_energy_group, the function every Armijo candidate is evaluated with (+inf where a hull point lies behind a
        plane or a limit is violated); tests/test_gpu_grad.py pins it to a 60-digit restatement of the objective"""
        e = np.zeros(self.U)
        self._check(self.lib.tj_get_energy(self._ctx, _d(e)))
        return e

    def audit(self, range=None, per_segment=False):
        """tj_audit: per robot obstacle / robot-pair clearance (GJK hull distances up to `range`; None = offset + 2 * margin) with where they
        are attained, peak speed / acceleration against the limits, duration and the flag word (AUDIT_FLAGS); robots of other ranks are zero.
        per_segment=True adds seg_obs / seg_pair [U][S].  Read-only, valid straight after construction."""
        return _audit(lambda r, rec, so, sp: self._check(self.lib.tj_audit(self._ctx, r, rec, so, sp)), self.U, self.S, range, per_segment)

    def audit_timed(self, range=None, levels=None, per_segment=False):
        """tj_audit_timed: per robot the bracket timed_lo <= closest approach to any other robot AT EQUAL FLIGHT TIMES <= timed_hi (searched up to
        `range`; None = offset + 2 * margin), the partner / own segment / real time of the timed_hi sample, where timed_lo is attained, the level
        used (levels 0..6: 2^levels sub-windows per segment; None = AUDIT_TIMED_LEVELS) and the flag word (AUDIT_TIMED_FLAGS: contact certain /
        separation certified / neither = raise levels).  per_segment=True adds seg_lo / seg_hi [U][S].  Read-only.  A sharded context raises
        (TJ_ERR_UNSUPPORTED): Group.audit_timed reads every robot's piece_time from its owner."""
        return _audit_timed(lambda r, l, rec, sl, sh: self._check(self.lib.tj_audit_timed(self._ctx, r, l, rec, sl, sh)), self.U, self.S, range, levels, per_segment)

    def closest_approach(self, range=None, tol=None, max_depth=None, max_windows=None):
        """tj_closest_approach: per robot lo <= closest approach to any other robot AT EQUAL FLIGHT TIMES <= hi, converged to `tol` (None: CLOSEST_TOL) by a
        branch and bound over tj_audit_timed's windows; `time`, `robot`, `segment` of the hi sample (-1 where nothing is closer than `range`), `depth` rounds,
        `windows` evaluated, `flags` (CLOSEST_FLAGS).  Dict of numpy arrays [U].  Read-only.  A sharded solver (world > 1) raises (TJ_ERR_UNSUPPORTED):
        Group.closest_approach reads every robot's piece_time from its owner."""
        return _approach(TjClosestRobot, lambda r, t, d, w, rec: self._check(self.lib.tj_closest_approach(self._ctx, r, t, d, w, rec)), self.U, range, tol, max_depth, max_windows)

    def pair_approach(self, range=None, tol=None, max_depth=None, max_windows=None, symmetric=False):
        """tj_pair_approach: one row per DIRECTED pair (robot, partner) that comes within `range` at equal flight times over robot's flight (an unlisted pair
        is certified at least `range` apart): lo <= the pair's closest approach <= hi converged to `tol` (None: PAIR_TOL) by the pair's own branch and bound,
        `time` / `segment` of the hi sample, `depth`, `windows`, `flags` (PAIR_FLAGS).  Dict of numpy arrays [n], sorted by (robot, partner).
        symmetric=True: one row per unordered pair (merge_pairs).  Read-only.  A sharded solver (world > 1) raises: use Group.pair_approach."""
        return _pair_approach(lambda r, t, d, w, rows, cap, n: self._check(self.lib.tj_pair_approach(self._ctx, r, t, d, w, rows, cap, n)), self.params,
                              range, tol, max_depth, max_windows, symmetric)

    def path_crossings(self, range=None, tol=None, max_depth=None, max_windows=None):
        """tj_path_crossings: one row per UNORDERED pair robot < partner whose PATHS come within `range` in space, whatever the time (a pair without a row is
        certified at least `range` apart in space): lo <= the paths' distance <= hi converged to `tol` (None: CROSSING_TOL) by the pair's own branch and
        bound, `segment` / `s` / `time` and `partner_segment` / `partner_s` / `partner_time` of the hi sample on either path, `gap` = partner_time - time
        (the timing margin of the crossing), `depth`, `windows`, `flags` (CROSSING_FLAGS).  Dict of numpy arrays [n], sorted by (robot, partner).  Read-only.
        A sharded solver (world > 1) raises: use Group.path_crossings."""
        return _path_crossings(lambda r, t, d, w, rows, cap, n: self._check(self.lib.tj_path_crossings(self._ctx, r, t, d, w, rows, cap, n)), range, tol, max_depth, max_windows)

    def timing_margin(self, dist=None, max_slip=None, tol=None, max_depth=None, max_windows=None):
        """tj_timing_margin: one row per UNORDERED pair robot < partner that some slip of the timetable below `max_slip` (None: any) may bring within `dist`
        (None: offset): lo <= the slip the pair tolerates <= hi in seconds, converged to `tol` (None: MARGIN_TOL_FRACTION * dist / vel_limit) by the pair's
        own branch and bound over two windows; hi == 0: within dist on the timetable.  `distance` of the hi sample, its `segment` / `s` / `time` and
        `partner_segment` / `partner_s` / `partner_time`, `depth`, `windows`, `flags` (MARGIN_FLAGS).  A pair without a row is certified: no slip below
        max_slip brings the two within dist.  Dict of numpy arrays [n], sorted by (robot, partner).  Read-only.  A sharded solver (world > 1) raises: use
        Group.timing_margin."""
        return _timing_margin(lambda *a: self._check(self.lib.tj_timing_margin(self._ctx, *a)), dist, max_slip, tol, max_depth, max_windows)

    def proximity_windows(self, dist=None, tol=None, max_depth=None, max_windows=None):
        """tj_proximity_windows: WHEN is each DIRECTED pair (robot, partner) within `dist` (None: offset) at equal flight times over robot's flight.  One row per
        maximal run of time that is not certified farther apart: the pair first comes within dist in [`t_first_lo`, `t_first_hi`] and is last within it in
        [`t_last_lo`, `t_last_hi`], resolved to `tol` (None: PROXIMITY_TOL_FRACTION * dist / vel_limit); `within_lo` seconds certified within, `closest` /
        `closest_time` the smallest attained sample, `leaves`, `depth`, `windows`, `flags` (PROXIMITY_FLAGS).  Outside every row the pair is certified above
        dist.  Dict of numpy arrays [n] sorted by (robot, partner, t_first_lo), plus `n_pairs` (the listed pairs).  Read-only.  A sharded solver (world > 1)
        raises: use Group.proximity_windows."""
        return _proximity_windows(lambda *a: self.lib.tj_proximity_windows(self._ctx, *a), self._check, dist, tol, max_depth, max_windows)

    def obstacle_approach(self, range=None, tol=None, max_depth=None, max_windows=None):
        """tj_obstacle_approach: per robot lo <= closest approach of the FLOWN CURVE to any obstacle primitive <= hi, converged to `tol` (None: OBSTACLE_TOL)
        by a branch and bound over windows of the segments' hulls; `time`, `index` (the caller's point / face index), `segment` of the hi sample (-1 where
        nothing is within `range`), `depth` rounds, `windows` evaluated, `flags` (OBSTACLE_FLAGS).  Dict of numpy arrays [U].  Read-only.  All modes; a
        sharded solver (world > 1) answers for its owned robots, the other records are zero."""
        return _approach(TjObstacleRobot, lambda r, t, d, w, rec: self._check(self.lib.tj_obstacle_approach(self._ctx, r, t, d, w, rec)), self.U, range, tol, max_depth, max_windows)

    def obstacle_windows(self, dist=None, tol=None, max_depth=None, max_windows=None):
        """tj_obstacle_windows: WHEN is each robot's FLOWN CURVE within `dist` (None: offset) of the obstacle set.  One row per certified time interval: the
        curve first comes within dist in [`t_first_lo`, `t_first_hi`] and is last within it in [`t_last_lo`, `t_last_hi`], resolved to `tol` (None:
        OBSWIN_TOL_FRACTION * dist / vel_limit); `within_lo` seconds certified within, `closest` / `closest_time` / `index` the smallest attained end sample
        and its primitive (the caller's index), `segment_first`, `segment_last`, `leaves`, `depth`, `windows`, `flags` (OBSWIN_FLAGS).  Outside every row of a
        robot its curve is certified farther than dist from every primitive.  Dict of numpy arrays [n] in (robot, t_first_lo) order.  Read-only.  All modes; a
        sharded solver (world > 1) answers for its owned robots."""
        return _listed_rows(TjObswinRow, lambda *a: self._check(self.lib.tj_obstacle_windows(self._ctx, *a)), _search_args(dist, tol, max_depth, max_windows))

    def sight_windows(self, links=None, stations=None, dist=None, tol=None, max_depth=None, max_windows=None):
        """tj_sight_windows: WHEN does the straight line of each link pass within `dist` (None: offset) of the obstacle set.  links [n][2]: (a, b), a a robot, b
        another robot or -1 - s for row s of stations [m][3] (None: sight_links, every directed pair, then per robot every station); a link is looked at over
        a's flight, b hovers once it has arrived.  One row per certified time interval, with obstacle_windows' fields and `link` (the index into links),
        `robot` = a, `partner` = b; `flags` (SIGHT_FLAGS).  Outside every row of a link it is certified farther than dist from every primitive.  Dict of numpy
        arrays [n] in (link, t_first_lo) order.  Read-only.  All modes (single-UAV: station links); a sharded solver (world > 1) is refused: Group.sight_windows."""
        return _sight_windows(lambda *a: self._check(self.lib.tj_sight_windows(self._ctx, *a)), self.U, links, stations, dist, tol, max_depth, max_windows)

    def peak_dynamics(self, tol=None, max_depth=None, max_windows=None, length_levels=None):
        """tj_peak_dynamics: per robot the FLOWN CURVE's peak speed, acceleration and jerk as brackets lo <= peak <= hi converged to the relative `tol` (None:
        PEAK_TOL) -- `speed_lo`, `speed_hi`, `speed_time` / `speed_segment` of the lo sample, `speed_depth`, `speed_windows`, `speed_flags` (PEAK_FLAGS), the same
        under accel_ and jerk_ --, the path length's bracket `length_lo` / `length_hi` at `length_levels` (None: PEAK_LENGTH_LEVELS), `duration`, `time_scale`
        (the smallest factor on piece_time that keeps both limits certified; < 1: headroom) and `flags` (PEAK_DYN_FLAGS).  Dict of numpy arrays [U].  Read-only.
        All modes; a sharded solver (world > 1) answers for its owned robots, the other records are zero."""
        return _peak_dynamics(lambda *a: self._check(self.lib.tj_peak_dynamics(self._ctx, *a)), self.U, tol, max_depth, max_windows, length_levels)

    def dynamics_windows(self, gates=None, tol=None, max_depth=None, max_windows=None):
        """tj_dynamics_windows: per (owned robot, gate) the certified time intervals of the flight in which the flown curve's speed, acceleration or jerk is over
        (`above`) or under (`below`) a level.  gates: a list of (quantity, sense, level), names (DYNWIN_QUANTITIES, DYNWIN_SENSES) or numbers; None: speed above
        vel_limit and acceleration above acc_limit.  A row: brackets `t_first_lo` <= first time within <= `t_first_hi` and `t_last_lo` <= last <= `t_last_hi`
        (-1 without a sure time), resolved to `tol` seconds (None: DYNWIN_TOL_FRACTION * vel_limit / acc_limit); `within_lo` seconds certified within, `extreme`
        / `extreme_time` the largest (above) or smallest (below) attained end sample, `robot`, `gate`, `quantity`, `sense`, `segment_first`, `segment_last`,
        `leaves`, `depth`, `windows`, `flags` (DYNWIN_FLAGS).  Outside every row of a gate the robot is certified on the other side of the level.  Dict of numpy
        arrays [n] in (robot, gate, t_first_lo) order.  Read-only.  All modes; a sharded solver (world > 1) answers for its owned robots."""
        return _dynamics_windows(lambda *a: self._check(self.lib.tj_dynamics_windows(self._ctx, *a)), gates, tol, max_depth, max_windows)

    def zone_windows(self, zones, tol=None, max_depth=None, max_windows=None):
        """tj_zone_windows: per (owned robot, zone) the certified time intervals of the flight in which the flown curve is inside (or outside) a volume named here.
        zones: a list of zone_box(lo, hi) / zone_ball(center, r) / zone_planes(rows), each with sense="inside" | "outside" and a level (0: the zone itself, -m
        inside: with margin m).  A row: brackets `t_first_lo` <= first time within <= `t_first_hi` and `t_last_lo` <= last <= `t_last_hi` (-1 without a sure time),
        resolved to `tol` seconds (None: ZONEWIN_TOL_FRACTION * offset / vel_limit); `within_lo` seconds certified within, `extreme` / `extreme_time` / `face` the
        smallest (inside) or largest (outside) attained end sample of the gauge, its time and face (-1 for a ball), `robot`, `zone`, `sense`, `segment_first`,
        `segment_last`, `leaves`, `depth`, `windows`, `flags` (ZONEWIN_FLAGS).  Outside every row of a zone the robot is certified on the other side of the level.
        Dict of numpy arrays [n] in (robot, zone, t_first_lo) order.  Read-only.  All modes; a sharded solver (world > 1) answers for its owned robots."""
        return _zone_windows(lambda *a: self._check(self.lib.tj_zone_windows(self._ctx, *a)), zones, tol, max_depth, max_windows)

    def piece_times(self):
        """piece_time of every robot as this context holds it"""
        out = np.zeros(self.U)
        for u in range(self.U):
            pt = C.c_double()
            self._check(self.lib.tj_get_state(self._ctx, C.c_int(u), None, None, None, None, None, C.byref(pt)))
            out[u] = pt.value
        return out

    def flight_profile(self, times=None, samples=None):
        """tj_flight_profile: per robot and flight time the position, the distance and caller's index of the NEAREST obstacle primitive (no range: however far),
        the distance and index of the nearest other robot at the same time, speed, acceleration, segment (S: arrived) and flags (PROFILE_FLAGS).  times: real
        times >= 0 [K]; None: profile_grid over the longest robot's duration with K = samples (None: 101).  Dict of numpy arrays [U][K].  Read-only.  All
        modes; a sharded multi-UAV solver (world > 1) raises (TJ_ERR_UNSUPPORTED): use Group.flight_profile."""
        return _flight_profile(lambda t, n, rec: self._check(self.lib.tj_flight_profile(self._ctx, t, n, rec)), self.piece_times, self.U, self.P, times, samples)

    def build_info(self):
        ms, dev = C.c_double(), C.c_int()
        self._check(self.lib.tj_get_build_info(self._ctx, C.byref(ms), C.byref(dev)))
        return dict(bvh_build_ms=ms.value, on_device=bool(dev.value))

    def stats(self):
        s = TjStats()
        self._check(self.lib.tj_get_stats(self._ctx, C.byref(s)))
        return {n: getattr(s, n) for n, _ in TjStats._fields_}

    def exchange_buffer(self, what):
        ptr, per, first, n = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.tj_exchange_buffer(self._ctx, what, C.byref(ptr), C.byref(per), C.byref(first), C.byref(n)))
        return ptr.value, per.value, first.value, n.value


class Group:
    """The same problem sharded over several devices by the library itself (`tj_group`, csrc/tj_group.h): one context per rank,
    peer stores + events between them, no torch on the path.  `devices` may repeat (several ranks on one GPU)."""

    def __init__(self, scene, devices, params=None, stop=None, **caps):
        self.lib = load_library()
        p = dict(scenes.DEFAULT_PARAMS)
        if params:
            p.update(params)
        self.params = p
        self.mode, self.U, self.P = scene["mode"], scene["U"], scene["P"]
        self.res = p["res"]
        self.S, self.T = self.P * self.res, 3 * self.P + 3
        tp = TjParams()
        self.lib.tj_default_params(C.byref(tp), self.mode, self.U, self.P)
        tp.res = self.res
        tp.lambda_, tp.margin, tp.offset, tp.mu = p["lam"], p["margin"], p["offset"], p["mu"]
        tp.vel_limit, tp.acc_limit, tp.ks, tp.kt = p["vel_limit"], p["acc_limit"], scene["ks"], p["kt"]
        tp.stop = p["stop"] if stop is None else stop
        for k, v in caps.items():
            setattr(tp, k, v)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self.n = len(dev)
        self._g = C.c_void_p()
        rc = self.lib.tj_group_create(C.byref(tp), C.c_int(self.n), _i(dev), C.byref(self._g))
        if rc < 0:
            raise TrajAdmmError(f"tj_group_create error {rc}: {self.lib.tj_group_last_error(None).decode()}")
        if scene.get("tris") is not None:
            verts = np.ascontiguousarray(scene["tris"], dtype=np.float64).reshape(-1, 3)
            n = verts.shape[0] // 3
            faces = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
            self._check(self.lib.tj_group_set_mesh(self._g, _d(verts), C.c_int(3 * n), _i(faces), C.c_int(n)))
        else:
            cloud = np.ascontiguousarray(scene["cloud"], dtype=np.float64).reshape(-1, 3)
            self._check(self.lib.tj_group_set_cloud(self._g, _d(cloud), C.c_int(cloud.shape[0])))
        self._wp = np.ascontiguousarray(scene["waypoints"], dtype=np.float64)
        self._pt0 = float(p["piece_time0"])
        self.reset()

    def reset(self):
        self._check(self.lib.tj_group_init_state(self._g, _d(self._wp), C.c_double(self._pt0)))

    def _check(self, rc):
        if rc < 0:
            raise TrajAdmmError(f"libtrajadmm group error {rc}: {self.lib.tj_group_last_error(self._g).decode()}")
        return rc

    def iterate(self, n=1):
        """n iterations on every rank; returns (gnorm, iterations so far, converged)"""
        g, it, cv = C.c_double(), C.c_int(), C.c_int()
        self._check(self.lib.tj_group_iterate(self._g, C.c_int(n), C.byref(g), C.byref(it), C.byref(cv)))
        return g.value, it.value, bool(cv.value)

    @property
    def transport(self):
        self.lib.tj_group_transport.restype = C.c_char_p
        return self.lib.tj_group_transport(self._g).decode()

    def set_transport(self, name):
        """"flag" | "event" | "rccl" (csrc/tj_group.h); between batches only"""
        self._check(self.lib.tj_group_set_transport(self._g, name.encode()))

    @property
    def rccl_ranks(self):
        """ranks RCCL's communicator reports for this group (0 unless the rccl transport is selected)"""
        return max(0, int(self.lib.tj_group_rccl_ranks(self._g)))

    def launch_counts(self):
        """kernels each rank's context has enqueued so far (tj_launch_count)"""
        self.lib.tj_launch_count.restype = C.c_longlong
        self.lib.tj_group_ctx.restype = C.c_void_p
        return [int(self.lib.tj_launch_count(C.c_void_p(self.lib.tj_group_ctx(self._g, C.c_int(r))))) for r in range(self.n)]

    def profile_exchange(self, reps=50):
        """event-timed microseconds of one exchange of each buffer kind (slowest rank's average)"""
        us = np.zeros(5)
        self._check(self.lib.tj_group_profile_exchange(self._g, C.c_int(reps), _d(us)))
        return us

    def get_state(self):
        """every robot's state from the rank that owns it"""
        U, P, T = self.U, self.P, self.T
        st = dict(spline=np.zeros((U, 3, T)), p_slack=np.zeros((U, 3, 6 * P)), p_lambda=np.zeros((U, 3, 6 * P)),
                  t_slack=np.zeros((U, P)), t_lambda=np.zeros((U, P)), piece_time=np.zeros(U))
        for u in range(U):
            pt = C.c_double()
            self._check(self.lib.tj_group_get_state(self._g, u, _d(st["spline"][u]), _d(st["p_slack"][u]), _d(st["p_lambda"][u]),
                                                    _d(st["t_slack"][u]), _d(st["t_lambda"][u]), C.byref(pt)))
            st["piece_time"][u] = pt.value
        return st

    def audit(self, range=None, per_segment=False):
        """tj_group_audit: Solver.audit of every robot from the rank that owns it (bitwise one context's)"""
        return _audit(lambda r, rec, so, sp: self._check(self.lib.tj_group_audit(self._g, r, rec, so, sp)), self.U, self.S, range, per_segment)

    def audit_timed(self, range=None, levels=None, per_segment=False):
        """tj_group_audit_timed: Solver.audit_timed of every robot from the rank that owns it (bitwise one context's)"""
        return _audit_timed(lambda r, l, rec, sl, sh: self._check(self.lib.tj_group_audit_timed(self._g, r, l, rec, sl, sh)), self.U, self.S, range, levels, per_segment)

    def closest_approach(self, range=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_closest_approach: Solver.closest_approach of every robot from the rank that owns it (bitwise one context's)"""
        return _approach(TjClosestRobot, lambda r, t, d, w, rec: self._check(self.lib.tj_group_closest_approach(self._g, r, t, d, w, rec)), self.U, range, tol, max_depth, max_windows)

    def pair_approach(self, range=None, tol=None, max_depth=None, max_windows=None, symmetric=False):
        """tj_group_pair_approach: Solver.pair_approach from the ranks that own the robots, in (robot, partner) order (bitwise one context's)"""
        return _pair_approach(lambda r, t, d, w, rows, cap, n: self._check(self.lib.tj_group_pair_approach(self._g, r, t, d, w, rows, cap, n)), self.params,
                              range, tol, max_depth, max_windows, symmetric)

    def path_crossings(self, range=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_path_crossings: Solver.path_crossings, every pair (u, q > u) from the rank that owns u, in (robot, partner) order (bitwise one context's)"""
        return _path_crossings(lambda r, t, d, w, rows, cap, n: self._check(self.lib.tj_group_path_crossings(self._g, r, t, d, w, rows, cap, n)), range, tol, max_depth, max_windows)

    def proximity_windows(self, dist=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_proximity_windows: Solver.proximity_windows from the ranks that own the robots, in (robot, partner, t_first_lo) order (bitwise one context's)"""
        return _proximity_windows(lambda *a: self.lib.tj_group_proximity_windows(self._g, *a), self._check, dist, tol, max_depth, max_windows)

    def timing_margin(self, dist=None, max_slip=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_timing_margin: Solver.timing_margin, every pair (u, q > u) from the rank that owns u, in (robot, partner) order (bitwise one context's)"""
        return _timing_margin(lambda *a: self._check(self.lib.tj_group_timing_margin(self._g, *a)), dist, max_slip, tol, max_depth, max_windows)

    def obstacle_approach(self, range=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_obstacle_approach: Solver.obstacle_approach of every robot from the rank that owns it (bitwise one context's)"""
        return _approach(TjObstacleRobot, lambda r, t, d, w, rec: self._check(self.lib.tj_group_obstacle_approach(self._g, r, t, d, w, rec)), self.U, range, tol, max_depth, max_windows)

    def obstacle_windows(self, dist=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_obstacle_windows: Solver.obstacle_windows of every robot from the rank that owns it, in (robot, t_first_lo) order (bitwise one context's)"""
        return _listed_rows(TjObswinRow, lambda *a: self._check(self.lib.tj_group_obstacle_windows(self._g, *a)), _search_args(dist, tol, max_depth, max_windows))

    def piece_times(self):
        """piece_time of every robot from the rank that owns it"""
        out = np.zeros(self.U)
        for u in range(self.U):
            pt = C.c_double()
            self._check(self.lib.tj_group_get_state(self._g, C.c_int(u), None, None, None, None, None, C.byref(pt)))
            out[u] = pt.value
        return out

    def sight_windows(self, links=None, stations=None, dist=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_sight_windows: Solver.sight_windows, each link answered by the rank that owns its robot a, in (link, t_first_lo) order (bitwise one context's)"""
        return _sight_windows(lambda *a: self._check(self.lib.tj_group_sight_windows(self._g, *a)), self.U, links, stations, dist, tol, max_depth, max_windows)

    def peak_dynamics(self, tol=None, max_depth=None, max_windows=None, length_levels=None):
        """tj_group_peak_dynamics: Solver.peak_dynamics of every robot from the rank that owns it (bitwise one context's)"""
        return _peak_dynamics(lambda *a: self._check(self.lib.tj_group_peak_dynamics(self._g, *a)), self.U, tol, max_depth, max_windows, length_levels)

    def dynamics_windows(self, gates=None, tol=None, max_depth=None, max_windows=None):
        """tj_group_dynamics_windows: Solver.dynamics_windows of every robot from the rank that owns it, in (robot, gate, t_first_lo) order (bitwise one context's)"""
        return _dynamics_windows(lambda *a: self._check(self.lib.tj_group_dynamics_windows(self._g, *a)), gates, tol, max_depth, max_windows)

    def zone_windows(self, zones, tol=None, max_depth=None, max_windows=None):
        """tj_group_zone_windows: Solver.zone_windows of every robot from the rank that owns it, in (robot, zone, t_first_lo) order (bitwise one context's)"""
        return _zone_windows(lambda *a: self._check(self.lib.tj_group_zone_windows(self._g, *a)), zones, tol, max_depth, max_windows)

    def flight_profile(self, times=None, samples=None):
        """tj_group_flight_profile: Solver.flight_profile of every robot from the rank that owns it (bitwise one context's)"""
        return _flight_profile(lambda t, n, rec: self._check(self.lib.tj_group_flight_profile(self._g, t, n, rec)), self.piece_times, self.U, self.P, times, samples)

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self.lib.tj_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
