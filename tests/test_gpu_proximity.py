"""GPU (-m gpu): tj_proximity_windows -- during which time intervals every directed robot pair is within `dist` at EQUAL FLIGHT TIMES.

Expected values come from tests/proximity_ref.py: the Python restatement of the header's definition (closest_ref's windows, the classification OUT / IN / MIXED,
the search per pair, the merge of the leaves into rows, the row order).  Every field of every row is compared with == on doubles and ints, `windows`, `depth`
and `leaves` included, and so are the listed pairs and the number of rows: the bar tests/test_gpu_pair_approach.py holds.  The restatement itself is held
against the flown curves on the CPU (tests/test_proximity_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import audit_timed_ref as T
import proximity_ref as X
import timing_margin_ref as M
from audit_ref import prims
from query_kit import CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, close_to_six_digits, group_pair, loaded, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")
# tests/test_proximity_ref.py::test_truncation chooses these on the CPU: (dist, max_windows) at which some rows of the flattened fleet truncate and not all
TRUNCATING = ((0.1, 16), (1.0, 32))


def restated(pkg, slv, st, dist=None, tol=None, max_depth=None, max_windows=None, owned=None):
    p = slv.params
    d = p["offset"] if dist is None else dist
    return X.proximity_rows(pkg, prims(), st, slv.P, slv.res, d, X.default_tol(d, p["offset"], p["vel_limit"]) if tol is None else tol,
                            X.MAX_DEPTH if max_depth is None else max_depth, pkg.PROXIMITY_FRONTIER if max_windows is None else max_windows, owned)


def check(pkg, slv, dist=None, tol=None, max_depth=None, max_windows=None, st=None):
    """device rows == the restatement on the state the solver holds; returns the device's answer"""
    a = slv.proximity_windows(dist=dist, tol=tol, max_depth=max_depth, max_windows=max_windows)
    ref, n_pairs = restated(pkg, slv, slv.get_state() if st is None else st, dist, tol, max_depth, max_windows)
    assert set(a) == set(X.FIELDS) | {"n_pairs"}
    assert a["n_pairs"] == n_pairs, (dist, tol, max_depth, max_windows, a["n_pairs"], n_pairs)
    for n in ("robot", "partner") + X.FIELDS:
        assert np.array_equal(a[n], ref[n]), (dist, tol, max_depth, max_windows, n, a[n], ref[n])
    key = list(zip(a["robot"], a["partner"], a["t_first_lo"]))
    assert key == sorted(key)
    return a


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """after 0, 1 and 4 iterations; dist in {default, 1.0, inf}; tol = 0 with max_depth = 3: the depth stop and the EDGE leaves"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1 if name == "tiny" else 2)
    slv = pkg.Solver(scene, stop=0.0)
    edges = 0
    for it in (0, 1, 3):
        if it:
            slv.iterate(it)
        st = slv.get_state()
        for dist in (None, 1.0, INF):
            a = check(pkg, slv, dist, st=st)
            if dist == INF:
                F = pkg.PROXIMITY_FLAGS
                assert len(a["robot"]) == a["n_pairs"] == slv.U * (slv.U - 1) and np.all(a["depth"] == 0)
                assert np.all(a["flags"] == F["certain"] | F["at_start"] | F["at_end"] | F["resolved"])
        for dist in (None, 1.0):
            a = check(pkg, slv, dist, 0.0, 3, st=st)
            edges += int(np.sum(a["depth"] == 3))
    assert edges > 0
    slv.close()


def test_constructed_states(pkg, scenes):
    F = pkg.PROXIMITY_FLAGS
    # chase: contact rows around t_meet in both directions; robot 1 also meets the hovering robot 0 at t_goal
    scene, st, t_meet, t_goal = T.chase_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, st=st)
    tol = X.default_tol(0.1, 0.1, 2.0)
    rows = {(u, q): [k for k in range(len(a["robot"])) if (a["robot"][k], a["partner"][k]) == (u, q)] for u, q in ((0, 1), (1, 0))}
    assert len(rows[(0, 1)]) == 1 and len(rows[(1, 0)]) == 2
    for k, t in ((rows[(0, 1)][0], t_meet), (rows[(1, 0)][0], t_meet), (rows[(1, 0)][1], t_goal)):
        assert a["flags"][k] == F["certain"] | F["resolved"] and a["t_first_lo"][k] <= t <= a["t_last_hi"][k] and a["closest"][k] <= 0.1
        assert a["t_first_hi"][k] - a["t_first_lo"][k] <= tol and a["t_last_hi"][k] - a["t_last_lo"][k] <= tol
    slv.close()
    # crossing: the minimum separation is sqrt(5); above it one row per direction, below it nothing is listed
    scene, st = T.crossing_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, 2.5, st=st)
    assert list(zip(a["robot"], a["partner"])) == [(0, 1), (1, 0)] and np.all(a["flags"] == F["certain"] | F["resolved"])
    b = check(pkg, slv, 2.2, st=st)
    assert b["n_pairs"] == 0 and len(b["robot"]) == 0 and math.sqrt(5.0) > 2.2
    slv.close()
    # hover: robot 1 passes the place where robot 0 has been hovering since t = 2; robot 0's own flight is over before the two are near
    scene, st, t_meet = T.hover_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, st=st)
    assert list(zip(a["robot"], a["partner"])) == [(1, 0)] and a["t_first_lo"][0] > 2.0 and a["t_first_lo"][0] <= t_meet <= a["t_last_hi"][0]
    a = check(pkg, slv, 2.5, st=st)
    k = [k for k in range(len(a["robot"])) if a["robot"][k] == 0]
    assert len(k) == 1 and a["flags"][k[0]] & F["at_end"]                             # robot 0 ends its flight within 2.5 of robot 1
    slv.close()


@pytest.mark.parametrize("U", [64, 65, 130])
def test_fleet_sizes(pkg, scenes, U):
    """the partner passes at, just over and at twice a wave; the bitmask's rows at 2, 3 and 5 words"""
    slv = pkg.Solver(scenes.crossing(U, 500), stop=0.0)
    slv.iterate(2)
    st = slv.get_state()
    check(pkg, slv, st=st)
    a = check(pkg, slv, 1.0, st=st)
    assert len(a["robot"]) > 0
    slv.close()


def _call(lib, ctx, dist, tol, depth, windows, rows, cap, pairs, n, fn="tj_proximity_windows"):
    return getattr(lib, fn)(ctx, C.c_double(dist), C.c_double(tol), C.c_int(depth), C.c_int(windows), rows, C.c_int(cap), pairs, n)


def test_capacity(pkg, scenes):
    """a state with more rows than listed pairs: the count-only call, cap below n_pairs, cap between n_pairs and the rows, an exact cap"""
    scene, st, _, _ = T.chase_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    full = check(pkg, slv, st=st)
    n, n_pairs = len(full["robot"]), full["n_pairs"]
    assert (n_pairs, n) == (2, 3)

    def call(rows, cap):
        pairs, got = C.c_int(-7), C.c_int(-7)
        return _call(slv.lib, slv._ctx, 0.0, -1.0, -1, 0, rows, cap, C.byref(pairs), C.byref(got)), pairs.value, got.value

    assert call(None, 0) == (0, n_pairs, -1)
    rec = (pkg.TjProximityRow * n)()
    for k in range(n):
        rec[k].robot, rec[k].closest = -99, 123.5
    assert call(rec, n_pairs - 1) == (-3, n_pairs, -1)
    assert all((rec[k].robot, rec[k].closest) == (-99, 123.5) for k in range(n))       # more pairs than slots: nothing is written
    assert call(rec, n_pairs) == (-3, n_pairs, n)
    assert (rec[n - 1].robot, rec[n - 1].closest) == (-99, 123.5)                      # the sentinel behind the first cap rows is untouched
    for k in range(n_pairs):
        assert all(getattr(rec[k], f) == full[f][k] for f in X.FIELDS), k
    assert call(rec, n) == (0, n_pairs, n)
    assert all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in X.FIELDS)
    assert call(rec, 1) == (-3, n_pairs, -1) and call(rec, n) == (0, n_pairs, n)       # a smaller call after a larger one, and back
    slv.close()


@pytest.mark.parametrize("dist,max_windows", TRUNCATING)
def test_truncation(pkg, scenes, dist, max_windows):
    """robots 0..7 of the flattened fleet at the CPU test's truncating settings: at offset the lists overflow inside the rounds, at 1.0 among the seeds"""
    st, P, res = M.state_named("e2e_scn_c3", "_flat")
    slv = pkg.Solver(scenes.crossing(8, 500), stop=0.0)
    full = slv.get_state()
    full["spline"], full["piece_time"] = np.array(st["spline"][:8]), np.array(st["piece_time"][:8])
    slv.set_state(full)
    a = check(pkg, slv, dist, None, None, max_windows, st=full)
    cut = a["flags"] & pkg.PROXIMITY_FLAGS["truncated"] != 0
    assert cut.any() and not cut.all()
    assert (a["depth"][cut] > 0).any() if dist == 0.1 else (a["depth"][cut] == 0).any()
    slv.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, pairs, got = (pkg.TjProximityRow * 12)(), C.c_int(-7), C.c_int(-7)
        rec[0].robot = -99

        def call(d, t, depth, w, out=rec, cap=12, np_=C.byref(pairs), n=C.byref(got)):
            rc = _call(lib, ctx, d, t, depth, w, out, cap, np_, n)
            if rc == -1:
                assert (pairs.value, got.value, rec[0].robot) == (-7, -7, -99)              # the outputs are untouched
            return rc

        assert call(0.0, -1.0, -1, 0) == -1                                                 # before tj_init_state
        init()
        nan = float("nan")
        assert call(nan, -1.0, -1, 0) == -1 and call(0.0, nan, -1, 0) == -1 and call(0.0, -1.0, 41, 0) == -1 and call(0.0, -1.0, -1, 4097) == -1
        assert call(0.0, -1.0, -1, 0, n=None) == -1 and call(0.0, -1.0, -1, 0, np_=None) == -1 and call(0.0, -1.0, -1, 0, cap=-1) == -1 and call(0.0, -1.0, -1, 0, out=None) == -1
        assert call(0.0, -1.0, -1, 4096, cap=1 << 20) == -1 and b"TJ_PROXIMITY_MAX_BYTES" in lib.tj_last_error(ctx)   # refused up front, nothing allocated
        assert call(INF, -1.0, 40, 4096) == 0 and (pairs.value, got.value) == (6, 6) and call(0.0, 0.0, -1, 0) == 0       # still usable; the limits themselves are valid
    one = pkg.Solver(scenes.tiny(mode=0), stop=0.0)
    one.iterate(2)
    for dist in (None, INF):
        a = one.proximity_windows(dist=dist)
        assert set(a) == set(X.FIELDS) | {"n_pairs"} and a["n_pairs"] == 0 and all(len(a[f]) == 0 for f in X.FIELDS)
    one.close()


def test_proximity_windows_is_read_only(pkg, scenes):
    assert_read_only(pkg, scenes.hard(), lambda s: s.proximity_windows(dist=INF, tol=0.0),
                     lambda s: (s.proximity_windows(), s.proximity_windows(dist=1.0, max_depth=2, max_windows=1)))


def test_group_equals_one_context(pkg, scenes):
    """two ranks on one device (tests/test_gpu_group.py's way of building a group): bitwise one context's answer; a plain sharded context refuses"""
    scene = dict(scenes.hard(), mode=1)
    one, grp = group_pair(pkg, scene, 2)
    x = assert_group_equals(one, grp, lambda s, dist, tol: s.proximity_windows(dist=dist, tol=tol), ((None, None), (1.0, None), (INF, 0.0)))
    n = len(x["robot"])
    rec, pairs, got = (pkg.TjProximityRow * n)(), C.c_int(0), C.c_int(0)             # a cap that ends inside the second rank's rows
    rc = _call(grp.lib, grp._g, INF, 0.0, -1, 0, rec, n - 2, C.byref(pairs), C.byref(got), fn="tj_group_proximity_windows")
    assert (rc, pairs.value, got.value) == (-3, n, -1)
    grp.close(); one.close()
    assert_sharded_refuses(pkg, scenes, lambda half: half.proximity_windows(), "tj_group_proximity_windows")


def test_command_line(pkg, scenes, tmp_path):
    """--proximity-windows 1.0 (one context and a two-rank group): the printed rows are the library's on the dumped state, in its order -- doubles to 6
    significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly -- and the fleet's line counts them"""
    cli = CliCase(pkg, scenes, tmp_path)
    doubles = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "closest", "closest_time")
    for extra, lines in cli.queried(["--proximity-windows", "1.0"], "proximity "):
        got = [l.split() for l in lines if l.startswith("proximity uav ")]
        a = cli.slv.proximity_windows(dist=1.0)
        assert len(got) == len(a["robot"]) > 0 and all(len(w) == 25 for w in got)
        for k, w in enumerate(got):
            assert (int(w[2]), int(w[4])) == (a["robot"][k], a["partner"][k])
            for n, i in zip(doubles, (6, 7, 9, 10, 12, 14, 16)):
                assert close_to_six_digits(w[i], a[n][k]), (extra, k, n, w)
            assert [int(w[i]) for i in (18, 20, 22, 24)] == [a[n][k] for n in ("leaves", "depth", "windows", "flags")], (extra, k, w)
        fleet = [l.split() for l in lines if l.startswith("proximity fleet ")]
        assert len(fleet) == 1 and [int(fleet[0][i]) for i in (3, 5)] == [a["n_pairs"], len(a["robot"])]
    cli.close()
