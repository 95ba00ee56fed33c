"""GPU (-m gpu): tj_timing_margin -- the slip of the timetable every robot pair tolerates before the two come within the contact distance, each pair converged
by its own branch and bound over two windows.

Expected values come from tests/timing_margin_ref.py: the Python restatement of the header's definition (the crossings' items, nets, box test and GJK; the
clock sets, klo, the corner and same-time candidates, the listed rule, the round, the row order).  Every field of every row is compared with == on doubles
and ints, `windows` and `depth` included, and so is the number of rows.  The restatement itself is held against the flown curves on the CPU
(tests/test_timing_margin_ref.py).  Every case runs under its own time limit: a watchdog ends the process, so that nothing more is started on a device a
kernel hangs on."""
import ctypes as C
import faulthandler
import os
import re

import numpy as np
import pytest

import audit_ref as R
import path_crossing_ref as X
import timing_margin_ref as M
from audit_ref import prims
from conftest import ROOT
from query_kit import CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, close_to_six_digits, group_pair, loaded, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")
NAMES = M.FIELDS


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def resolved(pkg, slv, dist, max_slip, tol, max_depth, max_windows):
    p = slv.params
    dist = p["offset"] if dist is None else dist
    return (dist, INF if max_slip is None else max_slip, M.default_tol(dist, p["vel_limit"]) if tol is None else tol, M.MAX_DEPTH if max_depth is None else max_depth,
            pkg.MARGIN_FRONTIER if max_windows is None else max_windows)


def check(pkg, slv, dist=None, max_slip=None, tol=None, max_depth=None, max_windows=None, st=None, ref=None):
    """device rows == the restatement on the state the solver holds; returns the device's answer"""
    a = slv.timing_margin(dist=dist, max_slip=max_slip, tol=tol, max_depth=max_depth, max_windows=max_windows)
    ref = ref or M.Ref(pkg, prims(), slv.get_state() if st is None else st, slv.P, slv.res)
    want = ref.rows(*resolved(pkg, slv, dist, max_slip, tol, max_depth, max_windows))
    assert set(a) == set(NAMES)
    for n in ("robot", "partner") + M.FIELDS:
        assert np.array_equal(a[n], want[n]), (dist, max_slip, tol, max_depth, max_windows, n, a[n], want[n])
    assert list(zip(a["robot"], a["partner"])) == sorted(zip(a["robot"], a["partner"])) and np.all(a["robot"] < a["partner"])
    return a


def test_record_size_and_constants(pkg):
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert lib.tj_margin_record_size() == C.sizeof(pkg.TjMarginRecord) == 88
    for name, v in (("TOL_FRACTION", pkg.MARGIN_TOL_FRACTION), ("FRONTIER", pkg.MARGIN_FRONTIER), ("MAX_DEPTH", pkg.MARGIN_MAX_DEPTH), ("MAX_WINDOWS", pkg.MARGIN_MAX_WINDOWS)):
        assert float(re.search(r"#define TJ_MARGIN_%s\s+(\S+)" % name, hdr).group(1)) == v, name
    for n, v in pkg.MARGIN_FLAGS.items():
        assert int(re.search(r"#define TJ_MARGIN_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v


@pytest.mark.parametrize("name", ["tiny", "tiny_coupled", "hard"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """the initial state and the state after 3 iterations: dist in {default, 0.3}, tol in {default, 0 with max_depth <= 12, 5e-3}, max_depth in {0, 1, 5},
    max_slip in {inf, 0.8}: 0.8 drops the samples above it, and the pairs are still counted right"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1 if name == "tiny" else 2)
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 3):
        if it:
            slv.iterate(it)
        st = slv.get_state()
        ref = M.Ref(pkg, prims(), st, slv.P, slv.res)
        for dist in (None, 0.3):
            full = check(pkg, slv, dist, st=st, ref=ref)
            check(pkg, slv, dist, None, 0.0, 12, st=st, ref=ref)
            check(pkg, slv, dist, None, 5e-3, st=st, ref=ref)
            for depth in (0, 1, 5):
                check(pkg, slv, dist, None, None, depth, st=st, ref=ref)
            cut = check(pkg, slv, dist, 0.8, st=st, ref=ref)
            check(pkg, slv, dist, 0.8, 0.0, 5, st=st, ref=ref)
            assert len(cut["robot"]) <= len(full["robot"]) and np.all(cut["hi"] <= 0.8)
            if name == "hard" and it == 3 and dist == 0.3:
                # slips 0.735, 0.814, 0.907 and two pairs at 0: max_slip = 0.8 drops the samples of two pairs.  Both stay listed -- a seed of theirs is not OUT
                # with klo = 0 < max_slip -- and come back without a sample, certified: no slip below 0.8 brings them within dist
                print("hard, 3 iterations, dist 0.3: hi", full["hi"].tolist(), "with max_slip 0.8", cut["hi"].tolist(), cut["segment"].tolist())
                over = full["hi"] > 0.8
                assert int(np.sum(full["hi"] == 0.0)) == 2 and int(np.sum(over)) == 2 and len(cut["robot"]) == len(full["robot"]) == 5
                assert np.all(cut["segment"][over] == -1) and np.all(cut["lo"][over] == 0.8) and np.all(cut["hi"][over] == 0.8) and np.all(cut["hi"][~over] == full["hi"][~over])
                assert np.all(cut["flags"][over] == pkg.MARGIN_FLAGS["clear"] | pkg.MARGIN_FLAGS["converged"])
    slv.close()


def test_constructed_states(pkg, scenes):
    """the perpendicular crossing (the analytic margin), the skew pair, the goal on the other's path and the partner that arrives early; then each robot with
    its own piece_time: the places and `distance` stay, times and margins change"""
    F, tol = pkg.MARGIN_FLAGS, 1e-7
    scene, st = X.x_state(pkg, scenes, 0.0)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, None, None, tol, st=st)
    assert len(a["robot"]) == 1 and a["lo"][0] - 1e-9 <= 1.79055728090 <= a["hi"][0] + 1e-9 and a["hi"][0] - a["lo"][0] <= tol and a["flags"][0] == F["clear"] | F["converged"]
    check(pkg, slv, st=st)
    st2 = R.scaled_time_state(R.scaled_time_state(st, 0, 0.5), 1, 1.0)             # both twice as fast: the same places, half the clock values
    slv.set_state(st2)
    b = check(pkg, slv, None, None, 0.5 * tol, st=st2)
    for n in ("distance", "s", "partner_s", "segment", "partner_segment", "depth", "windows", "flags"):
        assert np.array_equal(a[n], b[n]), n
    assert b["hi"][0] == 0.5 * a["hi"][0] and b["lo"][0] == 0.5 * a["lo"][0] and b["time"][0] == 0.5 * a["time"][0] and b["partner_time"][0] == 0.5 * a["partner_time"][0]
    st3 = R.scaled_time_state(R.scaled_time_state(st, 0, 0.7), 1, 3.1)             # each its own
    slv.set_state(st3)
    c = check(pkg, slv, None, None, 1e-6, st=st3)
    assert len(c["robot"]) == 1 and c["distance"][0] <= 0.1 and c["hi"][0] != a["hi"][0]
    assert c["time"][0] == ((c["segment"][0] + c["s"][0]) / 8.0) * 0.7 and c["partner_time"][0] == ((c["partner_segment"][0] + c["partner_s"][0]) / 8.0) * 3.1
    slv.close()
    for z, n in ((0.05, 1), (0.2, 0)):
        scene, st = X.x_state(pkg, scenes, z)
        slv = loaded(pkg, scene, st)
        a = check(pkg, slv, None, None, tol, st=st)
        assert len(a["robot"]) == n and (n == 0 or a["lo"][0] - 1e-9 <= 1.80254033 + 1e-8 and 1.80254033 - 1e-8 <= a["hi"][0] + 1e-9)
        slv.close()
    scene, st = X.goal_on_path_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, None, None, tol, st=st)
    assert len(a["robot"]) == 1 and a["lo"][0] - 1e-9 <= 5.88 - 0.1 * (1 / 2.5 ** 2 + 1 / 0.625 ** 2) ** 0.5 <= a["hi"][0] + 1e-9
    early = R.scaled_time_state(st, 1, 0.25)                                        # the partner has arrived when the other passes its goal
    slv.set_state(early)
    a = check(pkg, slv, None, None, tol, st=early)
    assert len(a["robot"]) == 1 and a["hi"][0] == 0.0 == a["lo"][0] and a["flags"][0] & F["contact"] and a["flags"][0] & (F["partner_end"] | F["same_time"])
    slv.close()


def test_wide_live_sets(pkg, scenes):
    """hard's pair (0, 1) at dist = 0.3, tol = 0: the live set passes a wave (64) and the refine workgroup (128) (checked in the restatement first); then
    max_windows one below a round's size, and 8: TRUNCATED with the last completed round's record"""
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(3)
    st = slv.get_state()
    ref = M.Ref(pkg, prims(), st, slv.P, slv.res)
    traces = {}
    ref.rows(0.3, INF, 0.0, 11, M.MAX_WINDOWS, pairs=[(0, 1)], traces=traces)
    sizes = [t[3] for t in traces[(0, 1)]]
    print("live set of (0, 1) per depth", sizes)
    assert sizes == [6, 12, 14, 22, 32, 45, 64, 90, 123, 168, 239, 339]
    F = pkg.MARGIN_FLAGS["truncated"]
    a = check(pkg, slv, 0.3, None, 0.0, 11, sizes[11], st, ref)
    k = int(np.flatnonzero((a["robot"] == 0) & (a["partner"] == 1))[0])
    assert a["depth"][k] == 11 and not a["flags"][k] & F
    b = check(pkg, slv, 0.3, None, 0.0, 11, sizes[11] - 1, st, ref)
    prev = check(pkg, slv, 0.3, None, 0.0, 10, sizes[11], st, ref)
    assert b["flags"][k] & F and b["depth"][k] == 10 and b["windows"][k] == a["windows"][k]
    assert all(b[n][k] == prev[n][k] for n in M.FIELDS if n not in ("flags", "windows"))
    c = check(pkg, slv, 0.3, None, 0.0, 11, 8, st, ref)
    assert c["flags"][k] & F and c["depth"][k] == 0                                    # 6 seeds live, 12 children kept: the seeds' record
    slv.close()


def test_fleet_of_66(pkg, scenes):
    """partner indices beyond one and two 32-bit mask words, a second pass of 64 partners; rows in (robot, partner) order.  dist = 0.3 lists the stacked
    neighbours (0.25 apart in z), asserted in the restatement"""
    slv = pkg.Solver(scenes.crossing(66, 600), stop=0.0)
    slv.iterate(2)
    st = slv.get_state()
    want = M.Ref(pkg, prims(), st, slv.P, slv.res).rows(0.3, INF, M.default_tol(0.3, slv.params["vel_limit"]), 3, pkg.MARGIN_FRONTIER)
    assert len(want["robot"]) > 0 and want["partner"].max() >= 64 and np.any((want["partner"] >= 32) & (want["partner"] < 64))
    a = check(pkg, slv, 0.3, None, None, 3, st=st)
    assert np.array_equal(a["partner"], want["partner"])
    slv.close()


def test_capacity(pkg, scenes):
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(3)
    full = slv.timing_margin(dist=0.3, max_depth=6)
    n = len(full["robot"])
    assert n == 5
    lib = slv.lib

    def call(rows, cap):
        got = C.c_int(-7)
        return lib.tj_timing_margin(slv._ctx, C.c_double(0.3), C.c_double(0.0), C.c_double(-1.0), C.c_int(6), C.c_int(0), rows, C.c_int(cap), C.byref(got)), got.value

    assert call(None, 0) == (0, n)                                                  # count only
    rec = (pkg.TjMarginRecord * n)()
    rec[n - 1].robot, rec[n - 1].lo = -99, 123.5
    assert call(rec, n - 1) == (-3, n)
    assert (rec[n - 1].robot, rec[n - 1].lo) == (-99, 123.5)                        # the sentinel behind the first n - 1 rows is untouched
    for k in range(n - 1):
        assert all(getattr(rec[k], f) == full[f][k] for f in M.FIELDS), k
    assert call(rec, n) == (0, n)
    assert all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in M.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n) == (0, n)                       # a smaller call after a larger one, and back
    slv.close()


@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_group_equals_one_context(pkg, scenes, ranks):
    one, grp = group_pair(pkg, scenes.hard(), ranks)

    def ask(s, dist, slip, tol, depth):
        a = s.timing_margin(dist, slip, tol, depth)
        assert set(a) == set(NAMES)
        return a

    assert_group_equals(one, grp, ask, ((None, None, None, None), (0.3, None, 0.0, 6), (0.3, 0.8, None, None)))
    x, y = one.timing_margin(0.3, max_depth=6), grp.timing_margin(0.3, max_depth=6)
    n = len(x["robot"])
    assert n == 5 and all(np.array_equal(x[k], y[k]) for k in x)
    rec, got = (pkg.TjMarginRecord * n)(), C.c_int(0)                     # a cap that ends inside a later rank's rows
    rc = grp.lib.tj_group_timing_margin(grp._g, C.c_double(0.3), C.c_double(0.0), C.c_double(-1.0), C.c_int(6), C.c_int(0), rec, C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in M.FIELDS)
    grp.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjMarginRecord * 3)(), C.c_int(0)
        call = lambda r, m, t, d, w, out=rec, cap=3, n=C.byref(got): lib.tj_timing_margin(ctx, C.c_double(r), C.c_double(m), C.c_double(t), C.c_int(d), C.c_int(w), out, C.c_int(cap), n)
        assert call(0.0, 0.0, -1.0, -1, 0) == -1                              # before tj_init_state
        init()
        nan = float("nan")
        assert call(nan, 0.0, -1.0, -1, 0) == -1 and call(0.0, nan, -1.0, -1, 0) == -1 and b"max_slip" in lib.tj_last_error(ctx) and call(0.0, 0.0, nan, -1, 0) == -1
        assert call(0.0, 0.0, -1.0, 41, 0) == -1 and call(0.0, 0.0, -1.0, -1, 4097) == -1
        assert call(0.0, 0.0, -1.0, -1, 0, n=None) == -1 and call(0.0, 0.0, -1.0, -1, 0, cap=-1) == -1 and call(0.0, 0.0, -1.0, -1, 0, out=None) == -1
        assert call(0.0, 0.0, -1.0, -1, 4096, cap=1 << 20) == -1 and b"TJ_MARGIN_MAX_BYTES" in lib.tj_last_error(ctx)      # refused up front, nothing allocated
        assert call(INF, INF, 0.0, 3, 4096) == 0 and got.value == 3 and call(0.0, 0.0, 0.0, -1, 0) == 0                   # still usable; the limits themselves are valid
    assert_sharded_refuses(pkg, scenes, lambda half: half.timing_margin(), "tj_group_timing_margin")
    one = pkg.Solver(scenes.tiny(mode=0), stop=0.0)                       # single-UAV mode
    one.iterate(2)
    for dist in (None, INF):
        a = one.timing_margin(dist=dist)
        assert set(a) == set(NAMES) and all(len(v) == 0 for v in a.values())
    one.close()


def test_timing_margin_is_read_only(pkg, scenes):
    """state, statistics and launch count are untouched; the other queries answer the same before and after; an iteration after the call gives the bits of
    an iteration without it"""
    def held(s):
        return s.get_state(), s.stats(), s.launch_count(), s.audit(), s.pair_approach(), s.path_crossings(), s.flight_profile(samples=5)

    def same(x, y):
        if isinstance(x, dict):
            return set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x)
        return x == y

    def ask_sync(s):
        before = held(s)
        s.timing_margin(); s.timing_margin(dist=0.3, tol=0.0, max_depth=3); s.timing_margin(dist=1.0, max_slip=0.5, max_depth=2, max_windows=1)
        assert all(same(x, y) for x, y in zip(before, held(s)))

    assert_read_only(pkg, scenes.hard(), lambda s: s.timing_margin(dist=0.3), ask_sync)


def test_command_line(pkg, scenes, tmp_path):
    """--timing-margin and --timing-margin 1e-5 (one context and a two-rank group): the printed rows are the library's on the dumped state, in its order --
    doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly -- and the fleet line counts them.  The
    contact distance on the command line is the default, `offset`, which a fleet stacked in z never comes within in space: the scene is two robots in ONE
    plane whose paths cross at a right angle, the second's moved 6 units along itself: it passes the crossing at 80 % of its flight, the first at 50 %"""
    scene = dict(scenes.crossing(2, 600, dz=0.0))
    scene["waypoints"] = scene["waypoints"].copy()
    scene["waypoints"][1, :, 1] += 6.0
    cli = CliCase(pkg, scenes, tmp_path, scene)
    # margin uav U uav Q lo . hi . dist . seg . s . time . seg . s . time . depth . windows . flags .
    names = ("lo", "hi", "distance", "segment", "s", "time", "partner_segment", "partner_s", "partner_time", "depth", "windows", "flags")
    for args, tol in ((["--timing-margin"], None), (["--timing-margin", "1e-5"], 1e-5)):
        for extra, lines in cli.queried(args, "margin "):
            got = [l.split() for l in lines if l.startswith("margin uav ")]
            a = cli.slv.timing_margin(tol=tol)
            assert len(got) == len(a["robot"]) == 1 and all(len(w) == 29 for w in got) and a["lo"][0] > 1.0    # a positive margin of seconds
            for k, w in enumerate(got):
                assert (int(w[2]), int(w[4])) == (a["robot"][k], a["partner"][k])
                for i, n in enumerate(names):
                    if n in M.DOUBLES:
                        assert close_to_six_digits(w[6 + 2 * i], a[n][k]), (args, extra, k, n, w)
                    else:
                        assert int(w[6 + 2 * i]) == a[n][k], (args, extra, k, n, w)
            fleet = [l.split() for l in lines if l.startswith("margin fleet ")]
            assert len(fleet) == 1
            contact = int(np.sum(a["flags"] & 1 != 0)); positive = int(np.sum((a["flags"] & 3) == 2))
            assert [int(fleet[0][i]) for i in (3, 5, 7)] == [len(a["robot"]), contact, positive]
            assert float(fleet[0][9]) == (float("%.17g" % a["hi"].min()) if len(a["robot"]) else INF)
    cli.close()
