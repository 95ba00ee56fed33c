"""CPU (-m "not gpu"): the restatement tests/test_gpu_path_crossing.py holds the device to (tests/path_crossing_ref.py) is itself held to the flown curves --
every row's bracket contains a sampled minimum that uses neither GJK nor subdivision, hi is attained where the row says, straight nets give the analytic
answer, deeper searches nest, the space-only distance never exceeds the equal-time one, the committed defaults are the measured ones -- and the host surface
that needs no GPU.  Bars: slack = K(S) * eps * max|coordinate| (counted in tests/audit_timed_ref.py: two curves restricted to windows, the same operations),
1e-10 relative for the GJK's stop rule on a certified lo (the header's stated limit 1) and the tolerance asked for.

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h, whose two tables the test reads back): the rows that are not in
contact shrink from 2.15e-2 at depth 0 to 7.21e-12 at depth 17 and are 0 from depth 18 -> TJ_CROSSING_TOL = 1e-10; the rows in contact halve hi per round down
to 3.34e-13 at depth 40; largest live set of any pair 59 -> TJ_CROSSING_FRONTIER = 256; listed pairs 7 / 63 / 7 / 2016 (the last: e2e_scn_c3 with z set to 0,
all of them in contact)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import pair_approach_ref as Q
import path_crossing_ref as X
from conftest import ROOT
from query_kit import pkg_module as _pkg

OFFSET, DEFAULT = 0.1, 0.1 + 2 * 0.1
INF = float("inf")
# (state, range, pairs or None = all)
CASES = [("tiny", INF, None), ("hard", INF, None), ("hard", DEFAULT, None),
         ("e2e_scn_b", DEFAULT, [(0, 1), (1, 2), (3, 4), (0, 7)]), ("e2e_scn_c3", DEFAULT, [(0, 1), (1, 2), (20, 21), (62, 63)]),
         ("e2e_scn_b_coupled", DEFAULT, [(0, 1), (1, 2), (3, 4), (0, 7)]), ("e2e_scn_c3_flat", DEFAULT, [(0, 1), (0, 32), (5, 40), (17, 50)])]


@functools.lru_cache(maxsize=None)
def state_of(name):
    pkg = _pkg()
    if name.startswith("e2e_"):
        flat = name.endswith("_flat")
        st, P, res = T.e2e_state(name[:-5] if flat else name)
        return (X.flattened(st) if flat else st), P, res
    scene = pkg.scenes.tiny(mode=1) if name == "tiny" else pkg.scenes.hard()
    st = R.port_state(scene, 3)
    return st, scene["P"], 8


@functools.lru_cache(maxsize=None)
def ref_of(name):
    st, P, res = state_of(name)
    return X.Ref(_pkg(), R.prims(), st, P, res)


@functools.lru_cache(maxsize=None)
def rows_of(name, rng, tol, pairs, max_depth=X.MAX_DEPTH, max_windows=X.MAX_WINDOWS):
    return ref_of(name).rows(rng, OFFSET, tol, max_depth, max_windows, pairs=list(pairs) if pairs is not None else None)


def _pairs(name, pairs):
    U = state_of(name)[0]["spline"].shape[0]
    return tuple(pairs) if pairs is not None else tuple((u, q) for u in range(U) for q in range(u + 1, U))


@pytest.mark.parametrize("name,rng,pairs", CASES)
def test_every_bracket_holds_the_sampled_minimum(pkg, name, rng, pairs):
    """soundness: lo <= the minimum over >= 400 samples per near segment pair (1e-10 relative + slack); CONVERGED rows: hi <= that minimum + tol + slack;
    a pair without a row is at least `range` apart.  Attained: the distance recomputed on the two flown curves at (segment, s) and (partner_segment,
    partner_s) equals hi to the slack."""
    st, P, res = state_of(name)
    ref, sl, tol = ref_of(name), X.slack(P * res, st), pkg.CROSSING_TOL
    pairs = _pairs(name, pairs)
    rows = rows_of(name, rng, tol, pairs)
    listed = {(int(u), int(q)): k for k, (u, q) in enumerate(zip(rows["robot"], rows["partner"]))}
    assert list(listed) == sorted(listed) and len(listed) > 0
    for u, q in pairs:
        truth = X.sampled_minimum(pkg, ref, st, P, res, u, q, rng)
        if (u, q) not in listed:
            assert truth >= rng - sl, (u, q, truth)
            continue
        k = listed[(u, q)]
        r = {n: rows[n][k] for n in X.FIELDS}
        print(name, r, "sampled", truth)
        assert r["lo"] <= r["hi"] and r["lo"] <= truth * (1 + 1e-10) + sl, (u, q)
        if r["flags"] & X.CONVERGED:
            assert r["hi"] <= truth + tol + sl, (u, q)
        if r["segment"] >= 0:
            d = X.point_at(pkg, st, P, res, u, r["segment"], r["s"]) - X.point_at(pkg, st, P, res, q, r["partner_segment"], r["partner_s"])
            assert abs(float(np.sqrt((d * d).sum())) - r["hi"]) <= sl, (u, q)
            assert r["time"] == ((r["segment"] + r["s"]) / res) * st["piece_time"][u] and r["partner_time"] == ((r["partner_segment"] + r["partner_s"]) / res) * st["piece_time"][q]
        else:
            assert r["hi"] == rng and (r["s"], r["partner_s"], r["time"], r["partner_time"], r["partner_segment"]) == (-1.0, -1.0, -1.0, -1.0, -1)


def test_two_straight_nets(pkg):
    """one net along x, the other along y at x = 0.3: crossing at z = 0, skew at z = 0.2, and the second net ENDING on the first path"""
    tol = pkg.CROSSING_TOL
    scene, st = X.x_state(pkg, pkg.scenes, 0.0)
    r = X.rows_of(pkg, R.prims(), st, 4, 8, INF, OFFSET, tol)
    assert len(r["robot"]) == 1 and r["lo"][0] == 0.0 and r["hi"][0] <= tol and r["depth"][0] >= 25
    assert r["flags"][0] & X.CONTACT and not r["flags"][0] & (X.CLEAR | X.TRUNCATED | X.ROBOT_END | X.PARTNER_END)
    # robot 0 is at x = 0.3 at sigma = 0.53 * 4 of 4 pieces with piece_time 1; robot 1 at y = 0 at sigma = 2 with piece_time 2
    assert abs(r["time"][0] - 0.53 * 4 * 1.0) <= 1e-9 and abs(r["partner_time"][0] - 0.5 * 4 * 2.0) <= 1e-9
    scene, st = X.x_state(pkg, pkg.scenes, 0.2)
    r = X.rows_of(pkg, R.prims(), st, 4, 8, INF, OFFSET, tol)
    assert len(r["robot"]) == 1 and r["lo"][0] <= 0.2 * (1 + 1e-10) + X.slack(32, st) and r["hi"][0] >= 0.2 - X.slack(32, st) and r["hi"][0] - r["lo"][0] <= tol
    assert r["flags"][0] & X.CLEAR and r["flags"][0] & X.CONVERGED and not r["flags"][0] & X.CONTACT
    assert len(X.rows_of(pkg, R.prims(), st, 4, 8, 0.15, OFFSET, tol)["robot"]) == 0          # 0.2 apart: no row at range 0.15
    scene, st = X.goal_on_path_state(pkg, pkg.scenes)
    r = X.rows_of(pkg, R.prims(), st, 4, 8, INF, OFFSET, tol)
    assert len(r["robot"]) == 1 and r["flags"][0] & X.PARTNER_END and r["flags"][0] & X.CONTACT and not r["flags"][0] & X.ROBOT_END
    assert (r["partner_segment"][0], r["partner_s"][0], r["partner_time"][0]) == (31, 1.0, 4 * 2.0) and r["hi"][0] <= tol + X.slack(32, st)


@pytest.mark.parametrize("name,rng,pairs", [("hard", INF, None), ("e2e_scn_c3_flat", DEFAULT, [(0, 1), (0, 32), (5, 40)])])
def test_deeper_searches_nest(pkg, name, rng, pairs):
    """as max_depth grows, lo does not fall, hi does not rise and windows does not fall.  hi and windows exactly: best only ever improves, work only
    adds.  lo in exact arithmetic; as computed, a child's certified lo is the GJK's |v| of a net restricted anew from the raw hull, which may stand up to
    1e-10 relative above its hull's distance (the header's stated limit 1) and carries the restriction's rounding: the bar is 1e-10 relative plus the slack."""
    pairs = _pairs(name, pairs)
    st, P, res = state_of(name)
    sl = X.slack(P * res, st)
    prev = None
    for depth in (0, 1, 2, 4, 8, 16, 40):
        rows = rows_of(name, rng, 0.0, pairs, depth)
        if prev is not None:
            assert np.array_equal(rows["robot"], prev["robot"]) and np.array_equal(rows["partner"], prev["partner"])
            assert np.all(rows["lo"] >= prev["lo"] * (1 - 1e-10) - sl) and np.all(rows["hi"] <= prev["hi"]) and np.all(rows["windows"] >= prev["windows"]), depth
        assert np.all(rows["depth"] <= depth)
        prev = rows
    assert len(prev["robot"]) > 0


@pytest.mark.parametrize("name", ["tiny", "hard", "e2e_scn_b"])
def test_never_further_than_at_equal_times(pkg, name):
    """for every pair the distance of the paths in space is at most their separation at equal flight times: crossing lo <= the smaller of the two directed
    tj_pair_approach hi (restated), up to slack"""
    st, P, res = state_of(name)
    sl = X.slack(P * res, st)
    timed = Q.pair_rows(pkg, R.prims(), st, P, res, INF, OFFSET, pkg.PAIR_TOL)
    both = {}
    for k in range(len(timed["robot"])):
        key = (min(int(timed["robot"][k]), int(timed["partner"][k])), max(int(timed["robot"][k]), int(timed["partner"][k])))
        both[key] = min(both.get(key, INF), float(timed["hi"][k]))
    rows = rows_of(name, INF, pkg.CROSSING_TOL, None)
    assert len(rows["robot"]) == len(both) > 0                       # at range = inf every pair is listed by both
    for k, key in enumerate(zip(rows["robot"].tolist(), rows["partner"].tolist())):
        assert rows["lo"][k] <= both[key] * (1 + 1e-10) + sl, key


def test_truncation_returns_the_last_completed_round(pkg):
    """a valley (two concentric arcs): the live set grows; max_windows one below a round's size gives TRUNCATED with the previous round's record"""
    scene, st = X.arcs_state(pkg, pkg.scenes)
    traces = {}
    full = X.rows_of(pkg, R.prims(), st, 4, 8, INF, OFFSET, 0.0, 3, X.MAX_WINDOWS, traces=traces)
    sizes = [t[3] for t in traces[(0, 1)]]
    print("live set per depth", sizes)
    d = 2
    assert sizes[d] > sizes[d - 1] > 64
    cut = X.rows_of(pkg, R.prims(), st, 4, 8, INF, OFFSET, 0.0, 3, sizes[d] - 1)
    prev = X.rows_of(pkg, R.prims(), st, 4, 8, INF, OFFSET, 0.0, d - 1, X.MAX_WINDOWS)
    assert cut["flags"][0] & X.TRUNCATED and not full["flags"][0] & X.TRUNCATED and cut["depth"][0] == d - 1
    for n in X.FIELDS:
        if n not in ("flags", "windows"):
            assert cut[n][0] == prev[n][0], n
    assert cut["windows"][0] == prev["windows"][0] + 4 * sizes[d - 1]    # the overflowing round's work is counted


def test_defaults_are_the_measured_ones(pkg):
    widths, clear_widths, tol, widest, frontier, per = X.default_tolerance(pkg, R.prims())
    print("widths per depth", ["%.3g" % w for w in widths], "not in contact", ["%.3g" % w for w in clear_widths], "tol", tol, "widest live set", widest,
          "frontier", frontier, "per state (listed, contact, live)", per)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert tol == pkg.CROSSING_TOL == float(re.search(r"#define TJ_CROSSING_TOL\s+(\S+)", hdr).group(1))
    assert frontier == pkg.CROSSING_FRONTIER == int(re.search(r"#define TJ_CROSSING_FRONTIER\s+(\S+)", hdr).group(1))
    assert pkg.CROSSING_MAX_DEPTH == X.MAX_DEPTH == int(re.search(r"#define TJ_CROSSING_MAX_DEPTH\s+(\S+)", hdr).group(1))
    assert pkg.CROSSING_MAX_WINDOWS == X.MAX_WINDOWS == int(re.search(r"#define TJ_CROSSING_MAX_WINDOWS\s+(\S+)", hdr).group(1))
    block = hdr[hdr.index("---- tj_path_crossings"):hdr.index("#define TJ_CROSSING_CONTACT")]
    row = re.search(r"\*\s+width((?:\s+\S+){41})\s*\n", block)                            # the header's first table: one width per depth 0..40
    assert [float(x) for x in row.group(1).split()] == [float("%.2e" % w) for w in widths]
    for name, (listed, contact, live) in per.items():                                     # the header's second table
        m = re.search(r"\*\s+%s\s.*?(\d+)\s+(\d+)\s+(\d+)\s*\n" % re.escape(name), block)
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (listed, contact, live), name


def test_host_surface(pkg):
    """needs no GPU: the record's size on both sides, the flag values, the exported symbols, the null checks"""
    lib = pkg.load_library()
    assert lib.tj_crossing_record_size() == C.sizeof(pkg.TjCrossingRecord) == 80
    for s in ("tj_path_crossings", "tj_crossing_record_size", "tj_group_path_crossings"):
        assert s in pkg.EXPORTS and hasattr(lib, s), s
    assert pkg.CROSSING_FLAGS == dict(contact=X.CONTACT, clear=X.CLEAR, converged=X.CONVERGED, truncated=X.TRUNCATED, robot_end=X.ROBOT_END, partner_end=X.PARTNER_END)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    for n, v in pkg.CROSSING_FLAGS.items():
        assert int(re.search(r"#define TJ_CROSSING_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    assert [n for n, _ in pkg.TjCrossingRecord._fields_ if n != "reserved"] == list(X.FIELDS)
    n = C.c_int(7)
    assert lib.tj_path_crossings(None, C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n)) == -1
    assert lib.tj_group_path_crossings(None, C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n)) == -1
