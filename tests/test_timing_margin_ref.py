"""CPU (-m "not gpu"): the restatement tests/test_gpu_timing_margin.py holds the device to (tests/timing_margin_ref.py) is itself held to things that share
nothing with it -- straight nets give the analytic margin, every bracket is sound against the clock-set distances of sampled points of the flown curves
(np.longdouble, no GJK, no subdivision), the hi sample is where and when the row says, deeper searches nest, a truncated search returns the last completed
round, the neighbouring queries agree, the committed defaults are the measured ones -- and the host surface that needs no GPU.
Bars: in space audit_timed_ref's slack (two curves restricted to windows); in time TIME_EPS = 64 ulp of the longest flight, for clock values formed in double
here and in np.longdouble by the sampling.

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h, whose table the test reads back): the stacked end states list
nothing at dist = offset; e2e_scn_c3 flattened lists 2016 pairs, all at slip 0 among the seeds; flattened and staggered 2016 pairs, one at 0, none truncated,
largest live set 2921, depth at most 12, widest bracket 4.995e-4 -> TJ_MARGIN_FRONTIER = 4096 (2 x 2921 rounded up to a power of two, capped)."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import pair_approach_ref as Q
import path_crossing_ref as X
import timing_margin_ref as M
from conftest import ROOT
from query_kit import pkg_module as _pkg

OFFSET, VEL = 0.1, 2.0
INF = float("inf")
TOL = M.default_tol(OFFSET, VEL)
# (state, dist, pairs or None = all)
CASES = [("tiny", 0.1, None), ("tiny", 0.3, None), ("hard", 0.1, None), ("hard", 0.3, None),
         ("e2e_scn_c3_flat_staggered", 0.1, [(0, 1), (0, 32), (5, 40), (17, 50), (62, 63)])]


@functools.lru_cache(maxsize=None)
def state_of(name):
    pkg = _pkg()
    if name.startswith("e2e_"):
        return M.state_named("e2e_scn_c3", name[len("e2e_scn_c3"):])
    scene = pkg.scenes.tiny(mode=1) if name == "tiny" else pkg.scenes.hard()
    st = R.port_state(scene, 3)
    return st, scene["P"], 8


@functools.lru_cache(maxsize=None)
def ref_of(name):
    st, P, res = state_of(name)
    return M.Ref(_pkg(), R.prims(), st, P, res)


@functools.lru_cache(maxsize=None)
def rows_of(name, dist, tol, pairs, max_depth=M.MAX_DEPTH, max_windows=M.MAX_WINDOWS, max_slip=INF):
    return ref_of(name).rows(dist, max_slip, tol, max_depth, max_windows, pairs=list(pairs) if pairs is not None else None)


def _pairs(name, pairs):
    U = state_of(name)[0]["spline"].shape[0]
    return tuple(pairs) if pairs is not None else tuple((u, q) for u in range(U) for q in range(u + 1, U))


def time_eps(st, P):
    return 64 * T.EPS * P * float(np.max(st["piece_time"]))


def test_default_tolerance_at_the_shipped_parameters():
    assert TOL == 5e-4 == (M.TOL_FRACTION * OFFSET) / VEL


def test_two_straight_nets(pkg):
    """perpendicular lines at 2.5 and 1.25 units/s passing the crossing 1.88 s apart, z apart in height: the margin is gap - sqrt(dist^2 - z^2) *
    sqrt(1 / v_u^2 + 1 / v_q^2), inside [lo, hi]; z = 0.2 is not listed at dist = 0.1; the goal on the other's path; and the hover"""
    pr, tol = R.prims(), 1e-7
    for z, want in ((0.0, 1.79055728090), (0.05, 1.80254033)):
        scene, st = X.x_state(pkg, pkg.scenes, z)
        exact = 1.88 - math.sqrt(0.1 ** 2 - z ** 2) * math.sqrt(1 / 2.5 ** 2 + 1 / 1.25 ** 2)
        assert abs(exact - want) <= 1e-8
        r = M.rows_of(pkg, pr, st, 4, 8, 0.1, INF, tol)
        print(z, {k: v.tolist() for k, v in r.items()}, exact)
        assert len(r["robot"]) == 1 and r["lo"][0] - 1e-9 <= exact <= r["hi"][0] + 1e-9 and r["hi"][0] - r["lo"][0] <= tol
        assert r["flags"][0] == M.CLEAR | M.CONVERGED and r["distance"][0] <= 0.1
        if z == 0.0:
            assert abs(r["lo"][0] - 1.79055720568) <= 1e-11 and abs(r["hi"][0] - 1.79055729508) <= 1e-11
    scene, st = X.x_state(pkg, pkg.scenes, 0.2)
    assert len(M.rows_of(pkg, pr, st, 4, 8, 0.1, INF, tol)["robot"]) == 0
    scene, st = X.goal_on_path_state(pkg, pkg.scenes)                    # the partner at 0.625 units/s ends on the other's path at 8.0; the other passes at 2.12
    exact = 5.88 - 0.1 * math.sqrt(1 / 2.5 ** 2 + 1 / 0.625 ** 2)
    r = M.rows_of(pkg, pr, st, 4, 8, 0.1, INF, tol)
    assert abs(exact - 5.71508) <= 1e-5 and len(r["robot"]) == 1 and r["lo"][0] - 1e-9 <= exact <= r["hi"][0] + 1e-9 and r["hi"][0] - r["lo"][0] <= tol
    early = R.scaled_time_state(st, 1, 0.25)                             # the partner arrives at 1.0, BEFORE the other passes: it is there when the other comes
    r = M.rows_of(pkg, pr, early, 4, 8, 0.1, INF, tol)
    assert len(r["robot"]) == 1 and r["lo"][0] == 0.0 == r["hi"][0] and r["flags"][0] & M.CONTACT and r["flags"][0] & (M.PARTNER_END | M.SAME_TIME)
    off = M.rows_of(pkg, pr, early, 4, 8, 0.1, INF, tol, hover=False)   # without the end's clock set the two miss each other by about 1.12 - 0.04 s
    assert len(off["robot"]) == 1 and off["lo"][0] > 1.0 and off["flags"][0] & M.CLEAR and not off["flags"][0] & M.CONTACT


@pytest.mark.parametrize("name,dist,pairs", CASES)
def test_every_bracket_is_sound(pkg, name, dist, pairs):
    """lo <= the smallest clock-set distance over all sample pairs (21 per segment) within dist; a pair with no sample pair within dist + slack has no found
    row; the hi sample recomputed on the flown curves is within dist + slack, and its clock-set distance is hi"""
    st, P, res = state_of(name)
    ref, sl, te = ref_of(name), X.slack(P * res, st), time_eps(st, P)
    pairs = _pairs(name, pairs)
    rows = rows_of(name, dist, TOL, pairs)
    listed = {(int(u), int(q)): k for k, (u, q) in enumerate(zip(rows["robot"], rows["partner"]))}
    assert list(listed) == sorted(listed)
    found = 0
    for u, q in pairs:
        truth, wide = M.sampled_margin(pkg, ref, st, P, res, u, q, dist), M.sampled_margin(pkg, ref, st, P, res, u, q, dist + sl)
        if (u, q) not in listed:
            assert truth == INF, (u, q, truth)
            continue
        r = {n: rows[n][listed[(u, q)]] for n in M.FIELDS}
        print(name, dist, r, "sampled", truth)
        assert r["lo"] <= r["hi"] and r["lo"] <= truth + te, (u, q)
        if wide == INF:
            assert r["segment"] == -1, (u, q)
        if r["segment"] >= 0:
            found += 1
            d = X.point_at(pkg, st, P, res, u, r["segment"], r["s"]) - X.point_at(pkg, st, P, res, q, r["partner_segment"], r["partner_s"])
            assert float(np.sqrt((d * d).sum())) <= dist + sl and abs(float(np.sqrt((d * d).sum())) - r["distance"]) <= sl and r["distance"] <= dist, (u, q)
            assert r["time"] == ((r["segment"] + r["s"]) / res) * st["piece_time"][u] and r["partner_time"] == ((r["partner_segment"] + r["partner_s"]) / res) * st["piece_time"][q]
            slip = M.clock_set_distance(ref, r)
            assert (slip <= te and r["hi"] == 0.0) if r["flags"] & M.SAME_TIME else slip == r["hi"], (u, q, slip)
        else:
            assert r["hi"] == INF and (r["s"], r["partner_s"], r["time"], r["partner_time"], r["distance"], r["partner_segment"]) == (-1.0,) * 5 + (-1,)
    assert found > 0 or dist == 0.1


@pytest.mark.parametrize("name,dist,pairs", [("hard", 0.3, None), ("e2e_scn_c3_flat_staggered", 0.1, [(0, 1), (5, 40)])])
def test_deeper_searches_nest(pkg, name, dist, pairs):
    """as max_depth grows hi does not rise, windows does not fall (exactly: best only improves, work only adds) and lo does not fall: a child's clock
    intervals lie inside its parent's, the clock is monotonic in the parameter as computed, and a candidate's slip is at least its item's klo"""
    pairs = _pairs(name, pairs)
    prev = None
    for depth in (0, 1, 2, 4, 8, 12):
        rows = rows_of(name, dist, 0.0, pairs, depth)
        if prev is not None:
            assert np.array_equal(rows["robot"], prev["robot"]) and np.array_equal(rows["partner"], prev["partner"])
            assert np.all(rows["lo"] >= prev["lo"]) and np.all(rows["hi"] <= prev["hi"]) and np.all(rows["windows"] >= prev["windows"]), depth
        assert np.all(rows["depth"] <= depth)
        prev = rows
    assert len(prev["robot"]) > 0


def test_truncation_returns_the_last_completed_round(pkg):
    """the perpendicular crossing: the live set grows along the boundary; max_windows one below a round's size gives TRUNCATED with the previous round's record"""
    scene, st = X.x_state(pkg, pkg.scenes, 0.0)
    traces = {}
    full = M.rows_of(pkg, R.prims(), st, 4, 8, 0.1, INF, 0.0, 12, M.MAX_WINDOWS, traces=traces)
    sizes = [t[3] for t in traces[(0, 1)]]
    print("live set per depth", sizes)
    d = 10
    assert sizes[:10] == [3, 3, 4, 5, 9, 11, 12, 19, 30, 43] and sizes[d] > sizes[d - 1]
    cut = M.rows_of(pkg, R.prims(), st, 4, 8, 0.1, INF, 0.0, 12, sizes[d] - 1)
    prev = M.rows_of(pkg, R.prims(), st, 4, 8, 0.1, INF, 0.0, d - 1, M.MAX_WINDOWS)
    assert cut["flags"][0] & M.TRUNCATED and not full["flags"][0] & M.TRUNCATED and cut["depth"][0] == d - 1
    for n in M.FIELDS:
        if n not in ("flags", "windows"):
            assert cut[n][0] == prev[n][0], n
    assert cut["windows"][0] == prev["windows"][0] + 4 * sizes[d - 1]    # the overflowing round's work is counted


@pytest.mark.parametrize("name,dist", [("tiny", 0.3), ("hard", 0.3), ("hard", 0.1)])
def test_agrees_with_the_neighbouring_queries(pkg, name, dist):
    """a pair that tj_pair_approach (restated) finds within dist at equal flight times has margin hi == 0 (tol = 0: the search goes on until a same-time
    candidate or a corner at slip 0 is found); a pair whose tj_path_crossings row (restated) is certified above dist in space has no found sample"""
    st, P, res = state_of(name)
    timed = Q.pair_rows(pkg, R.prims(), st, P, res, INF, OFFSET, pkg.PAIR_TOL)
    both = {}
    for k in range(len(timed["robot"])):
        key = (min(int(timed["robot"][k]), int(timed["partner"][k])), max(int(timed["robot"][k]), int(timed["partner"][k])))
        both[key] = min(both.get(key, INF), float(timed["hi"][k]))
    space = X.rows_of(pkg, R.prims(), st, P, res, INF, OFFSET, pkg.CROSSING_TOL)
    apart = {(int(u), int(q)) for u, q, lo in zip(space["robot"], space["partner"], space["lo"]) if lo > dist}
    rows = rows_of(name, dist, 0.0, None)
    got = {(int(u), int(q)): k for k, (u, q) in enumerate(zip(rows["robot"], rows["partner"]))}
    close = [key for key, hi in both.items() if hi <= dist]
    print(name, dist, "within dist at equal times", close, "apart in space", sorted(apart), "listed", sorted(got))
    for key in close:
        assert key in got and rows["hi"][got[key]] == 0.0 and rows["flags"][got[key]] & M.CONTACT, key
    for key in apart:
        assert key not in got or rows["segment"][got[key]] == -1, key
    assert len(both) == len(space["robot"]) > 0 and (close or apart)


def test_defaults_are_the_measured_ones(pkg):
    tol, frontier, per = M.default_tolerance(pkg, R.prims())
    print("tol", tol, "frontier", frontier, "per state (listed, hi == 0, truncated, largest live set, largest depth, widest bracket)", per)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert tol == 5e-4 and pkg.MARGIN_TOL_FRACTION == M.TOL_FRACTION == float(re.search(r"#define TJ_MARGIN_TOL_FRACTION\s+(\S+)", hdr).group(1))
    assert frontier == pkg.MARGIN_FRONTIER == int(re.search(r"#define TJ_MARGIN_FRONTIER\s+(\S+)", hdr).group(1))
    assert pkg.MARGIN_MAX_DEPTH == M.MAX_DEPTH == int(re.search(r"#define TJ_MARGIN_MAX_DEPTH\s+(\S+)", hdr).group(1))
    assert pkg.MARGIN_MAX_WINDOWS == M.MAX_WINDOWS == int(re.search(r"#define TJ_MARGIN_MAX_WINDOWS\s+(\S+)", hdr).group(1))
    block = hdr[hdr.index("---- tj_timing_margin"):hdr.index("#define TJ_MARGIN_CONTACT")]
    for name, (listed, zero, truncated, live, depth, width) in per.items():
        m = re.search(r"\*\s+%s\s.*?(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\S+)\s*\n" % re.escape(name), block)
        assert m and tuple(int(m.group(i)) for i in range(1, 6)) == (listed, zero, truncated, live, depth) and float(m.group(6)) == float("%.2e" % width), (name, per[name])


def test_host_surface(pkg):
    """needs no GPU: the record's size on both sides, the flag values and constants, the exported symbols, the null checks"""
    lib = pkg.load_library()
    assert lib.tj_margin_record_size() == C.sizeof(pkg.TjMarginRecord) == 88
    for s in ("tj_timing_margin", "tj_margin_record_size", "tj_group_timing_margin"):
        assert s in pkg.EXPORTS and hasattr(lib, s), s
    assert pkg.MARGIN_FLAGS == dict(contact=M.CONTACT, clear=M.CLEAR, converged=M.CONVERGED, truncated=M.TRUNCATED, robot_end=M.ROBOT_END, partner_end=M.PARTNER_END,
                                    same_time=M.SAME_TIME)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    for n, v in pkg.MARGIN_FLAGS.items():
        assert int(re.search(r"#define TJ_MARGIN_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    assert [n for n, _ in pkg.TjMarginRecord._fields_ if n != "reserved"] == list(M.FIELDS)
    n = C.c_int(7)
    args = (C.c_double(0.0), C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n))
    assert lib.tj_timing_margin(None, *args) == -1 and lib.tj_group_timing_margin(None, *args) == -1
