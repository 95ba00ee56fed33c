"""GPU (-m gpu): tj_closest_approach -- every robot's closest approach to another robot at EQUAL FLIGHT TIMES, converged by branch and bound.

Expected values come from tests/closest_ref.py: the Python restatement of the header's definition (audit_timed_ref's windows, blossoming and the oracle's
GJK; the level-synchronous search written out).  Every field of every record is compared with == on doubles and ints, `windows` and `depth` included: the
bar tests/test_gpu_audit_timed.py holds.  The restatement itself is held against the flown curves on the CPU (tests/test_closest_ref.py)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import closest_ref as K
import pair_approach_ref as Q
from audit_ref import prims
from conftest import ROOT
from query_kit import CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, close_to_six_digits, group_pair, one_queue, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")


def check(pkg, slv, rng=None, tol=None, max_depth=None, max_windows=None, st=None):
    """device records == the restatement on the state the solver holds; returns the device's answer"""
    p = slv.params
    a = slv.closest_approach(range=rng, tol=tol, max_depth=max_depth, max_windows=max_windows)
    st = slv.get_state() if st is None else st
    rec = K.closest_records(pkg, prims(), st, slv.P, slv.res, p["offset"] + 2 * p["margin"] if rng is None else rng, p["offset"],
                            pkg.CLOSEST_TOL if tol is None else tol, K.MAX_DEPTH if max_depth is None else max_depth, K.FRONTIER if max_windows is None else max_windows)
    assert set(a) == set(K.FIELDS)
    for n in K.FIELDS:
        assert np.array_equal(a[n], rec[n]), (rng, tol, max_depth, max_windows, n, a[n], rec[n])
    return a


def test_record_size_and_default(pkg):
    lib = pkg.load_library()
    assert lib.tj_closest_record_size() == C.sizeof(pkg.TjClosestRobot) == 48
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert float(re.search(r"#define TJ_CLOSEST_TOL\s+(\S+)", hdr).group(1)) == pkg.CLOSEST_TOL
    assert pkg.CLOSEST_FLAGS == dict(contact=1, clear=2, converged=4, truncated=8)


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """initial state and after a few iterations; tol in {default, 1e-3, 0}, range in {default, 1.0, inf}, max_depth in {default, 0, 3}"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1 if name == "tiny" else 2)
    slv = pkg.Solver(scene, stop=0.0)
    for it in ((0, 4) if name != "tiny_coupled" else (3,)):
        if it:
            slv.iterate(it)
        st = slv.get_state()
        for rng in (None, 1.0, INF):
            for tol in (None, 1e-3, 0.0):
                check(pkg, slv, rng, tol, None, None, st)
            for depth in (0, 3):
                check(pkg, slv, rng, None, depth, None, st)
        check(pkg, slv, INF, 0.0, 3, None, st)
    slv.close()


def test_depth_zero_is_audit_timed_level_zero(pkg, scenes):
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(4)
    for rng in (None, 1.0, INF):
        a, t = slv.closest_approach(range=rng, max_depth=0), slv.audit_timed(range=rng, levels=0)
        assert np.array_equal(a["hi"], t["timed_hi"]) and np.array_equal(a["time"], t["timed_time"])
        assert np.array_equal(a["robot"], t["timed_robot"]) and np.array_equal(a["segment"], t["timed_segment"])
        assert np.array_equal(a["lo"], np.minimum(t["timed_lo"], t["timed_hi"])) and np.all(a["depth"] == 0)
    slv.close()


def test_constructed_states(pkg, scenes):
    tol = pkg.CLOSEST_TOL
    F = pkg.CLOSEST_FLAGS
    scene, st, t_meet, t_goal = T.chase_state(pkg, scenes)
    sl = T.slack(32, st["spline"])
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    a = check(pkg, slv, st=st)
    assert np.all(a["flags"] & F["contact"]) and np.all(a["hi"] <= 1e-5) and (a["robot"][0], a["robot"][1]) == (1, 0)
    assert abs(a["time"][0] - t_meet) <= 1e-5 and abs(T.separation_at(pkg, st, 4, 8, 0, 1, a["time"][0]) - a["hi"][0]) <= sl
    assert min(abs(a["time"][1] - t_meet), abs(a["time"][1] - t_goal)) <= 1e-5      # both are contacts at rounding level: which one is not pinned
    slv.close()
    scene, st = T.crossing_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    a = check(pkg, slv, INF, st=st)
    assert np.all(a["flags"] == F["clear"] | F["converged"]) and np.all(a["hi"] - a["lo"] <= tol) and abs(a["hi"][0] - math.sqrt(5.0)) <= tol + sl
    a = check(pkg, slv, st=st)                                                        # nothing within the default range
    assert np.all(a["robot"] == -1) and np.all(a["lo"] == a["hi"]) and np.all(a["time"] == -1.0) and np.all(a["flags"] == F["clear"] | F["converged"])
    slv.close()
    scene, st, t_meet = T.hover_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    a = check(pkg, slv, INF, st=st)
    assert a["flags"][1] & F["contact"] and a["robot"][1] == 0 and abs(a["time"][1] - t_meet) <= 1e-5
    assert a["flags"][0] & F["clear"] and a["lo"][0] > 1.99
    slv.close()


def test_beyond_level_six(pkg, scenes):
    """hard() after 4 iterations, everything in range: converged to the default tolerance, no worse than level 6's upper end, with less work than level 6"""
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(4)
    st = slv.get_state()
    tol, sl = pkg.CLOSEST_TOL, T.slack(slv.S, st["spline"])
    a = check(pkg, slv, INF, st=st)
    t6 = slv.audit_timed(range=INF, levels=6)
    assert np.all(a["robot"] >= 0) and np.all(a["flags"] & pkg.CLOSEST_FLAGS["converged"]) and np.all(a["hi"] - a["lo"] <= tol)
    assert np.all(a["hi"] <= t6["timed_hi"] + tol + sl)
    for u in range(slv.U):
        assert a["windows"][u] < K.level_window_count(pkg, st, slv.P, slv.res, u, INF, 6), u
    slv.close()


def test_wide_live_sets(pkg, scenes):
    """a live set wider than the refine workgroup's 128 threads (pair_approach_ref.orbit_state: two robots, the set doubles per round: 32, 64, 128, 256), so
    that lanes take more than one child per pass; then max_windows one below that size: TRUNCATED with the previous round's record.  With one partner the
    robot's search is the pair's: the record equals tj_pair_approach's row, which the same round loop produces with 64 threads"""
    scene, st = Q.orbit_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    traces = {}
    Q.pair_rows(pkg, prims(), st, slv.P, slv.res, INF, slv.params["offset"], 0.0, 4, Q.MAX_WINDOWS, traces=traces)
    sizes = [t[3] for t in traces[(0, 1)]]
    print("live set of (0, 1) per depth", sizes)
    assert sizes[2] <= 128 < sizes[3]
    T_ = pkg.CLOSEST_FLAGS["truncated"]
    for cap, depth, truncated in ((sizes[3], 3, False), (sizes[3] - 1, 2, True)):
        a = check(pkg, slv, INF, 0.0, 3, cap, st)
        assert np.all(a["depth"] == depth) and np.all((a["flags"] & T_ != 0) == truncated)
        p = slv.pair_approach(range=INF, tol=0.0, max_depth=3, max_windows=cap)
        assert list(zip(p["robot"], p["partner"])) == [(0, 1), (1, 0)]
        for n in ("lo", "hi", "time", "segment", "depth", "flags", "windows"):
            assert np.array_equal(a[n], p[n]), (cap, n, a[n], p[n])
    slv.close()


@pytest.mark.parametrize("U", [64, 65, 130])
def test_fleet_sizes(pkg, scenes, U):
    slv = pkg.Solver(scenes.crossing(U, 500), stop=0.0)
    slv.iterate(2)
    check(pkg, slv)
    slv.close()


@pytest.mark.parametrize("P,res", [(12, 8), (2, 16)])
def test_segment_counts_and_resolutions(pkg, scenes, P, res):
    scene = dict(scenes.hard(4, 3000, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    check(pkg, slv, st=st)
    slv.close()


def test_triangle_scene(pkg, scenes):
    slv = pkg.Solver(scenes.triangulate(scenes.tiny(mode=1)), stop=0.0)
    slv.iterate(3)
    check(pkg, slv)
    slv.close()


@pytest.mark.parametrize("name", ["crossing", "hard"])
def test_truncation(pkg, scenes, name):
    if name == "crossing":
        scene, st = T.crossing_state(pkg, scenes)
        slv = pkg.Solver(scene, stop=0.0)
        slv.set_state(st)
    else:
        slv = pkg.Solver(scenes.hard(), stop=0.0)
        slv.iterate(4)
        st = slv.get_state()
    sl = T.slack(slv.S, st["spline"])
    tv = T.truth(pkg, st, slv.P, slv.res)
    seen = 0
    for mw in (1, 2):
        a = check(pkg, slv, INF, None, None, mw, st)      # == the restatement under the same cap, the TRUNCATED bit included
        seen += int(np.sum(a["flags"] & pkg.CLOSEST_FLAGS["truncated"] != 0))
        for u in range(slv.U):
            assert a["lo"][u] <= tv[u][0] + sl, (mw, u, a["lo"][u], tv[u])
    assert name != "hard" or seen > 0
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_closest_approach_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    assert_read_only(pkg, scenes.hard(), lambda s: s.closest_approach(range=INF, tol=0.0),
                     lambda s: (s.closest_approach(), s.closest_approach(range=1.0, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    assert_group_equals(one, grp, lambda s, rng, tol: s.closest_approach(range=rng, tol=tol), ((None, None), (INF, 0.0)))
    grp.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec = (pkg.TjClosestRobot * 3)()
        call = lambda r, t, d, w, out=rec: lib.tj_closest_approach(ctx, C.c_double(r), C.c_double(t), C.c_int(d), C.c_int(w), out)
        assert call(0.0, -1.0, -1, 0) == -1                                   # before tj_init_state
        init()
        nan = float("nan")
        assert call(nan, -1.0, -1, 0) == -1 and call(0.0, nan, -1, 0) == -1 and call(0.0, -1.0, 41, 0) == -1 and call(0.0, -1.0, -1, 4097) == -1
        assert call(0.0, -1.0, -1, 0, None) == -1
        assert call(0.0, -1.0, 40, 4096) == 0 and call(0.0, 0.0, -1, 0) == 0     # still usable; the limits themselves are valid
    assert_sharded_refuses(pkg, scenes, lambda half: half.closest_approach(), "tj_group_closest_approach")
    one = pkg.Solver(scenes.tiny(mode=0), stop=0.0)
    one.iterate(2)
    F = pkg.CLOSEST_FLAGS
    for rng, r in ((None, 0.1 + 2 * 0.1), (0.05, 0.05)):
        a = one.closest_approach(range=rng)
        assert {n: a[n][0] for n in K.FIELDS} == K.single_uav_record(r) and a["flags"][0] == F["clear"] | F["converged"]
    one.close()


def test_command_line(pkg, scenes, tmp_path):
    """--closest-approach and --closest-approach 1e-6 (one context and a two-rank group): every printed field equals the library's answer on the dumped state --
    doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly; the summary line names the smallest hi"""
    cli = CliCase(pkg, scenes, tmp_path)
    names = ("lo", "hi", "robot", "segment", "time", "depth", "windows", "flags")
    for args, tol in ((["--closest-approach"], None), (["--closest-approach", "1e-6"], 1e-6)):
        for extra, lines in cli.queried(args, "closest "):
            got = [l.split() for l in lines if l.startswith("closest uav ")]
            assert len(got) == cli.scene["U"] and all(len(w) == 19 and int(w[2]) == u for u, w in enumerate(got))
            a = cli.slv.closest_approach(tol=tol)
            for u, w in enumerate(got):
                for k, n in enumerate(names):
                    if n in ("lo", "hi", "time"):
                        assert close_to_six_digits(w[4 + 2 * k], a[n][u]), (args, extra, u, n, w)
                    else:
                        assert int(w[4 + 2 * k]) == a[n][u], (args, extra, u, n, w)
            fleet = [l.split() for l in lines if l.startswith("closest fleet ")]
            assert len(fleet) == 1
            m = a["robot"] >= 0
            if m.any():
                who = int(np.flatnonzero(m)[np.argmin(a["hi"][m])])
                f = fleet[0]
                assert close_to_six_digits(f[3], a["hi"][who]) and int(f[5]) == who and int(f[7]) == a["robot"][who]
                assert int(f[11]) == int(np.any(a["flags"] & pkg.CLOSEST_FLAGS["contact"]))
            else:
                assert fleet[0][2] == "none"
    cli.close()
