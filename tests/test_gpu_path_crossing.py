"""GPU (-m gpu): tj_path_crossings -- every unordered robot pair whose PATHS come close in space, whatever the time, each converged by its own branch and
bound over two windows.

Expected values come from tests/path_crossing_ref.py: the Python restatement of the header's definition (the seeds' box test, both nets restricted from the
raw hulls, the oracle's GJK with the certificate, the four end-point distances, the round over four quadrants, the listed rule, the row order).  Every field
of every row is compared with == on doubles and ints, `windows` and `depth` included, and so is the number of rows.  The restatement itself is held against
the flown curves on the CPU (tests/test_path_crossing_ref.py).  Every case runs under its own time limit: a watchdog ends the process, so that nothing more
is started on a device a kernel hangs on."""
import ctypes as C
import faulthandler
import os
import re

import numpy as np
import pytest

import audit_ref as R
import path_crossing_ref as X
from audit_ref import prims
from conftest import ROOT
from query_kit import CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, close_to_six_digits, group_pair, loaded, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")
NAMES = X.FIELDS + ("gap",)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(240, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def restated(pkg, slv, st, rng=None, tol=None, max_depth=None, max_windows=None, ref=None):
    p = slv.params
    ref = ref or X.Ref(pkg, prims(), st, slv.P, slv.res)
    return ref.rows(p["offset"] + 2 * p["margin"] if rng is None else rng, p["offset"], pkg.CROSSING_TOL if tol is None else tol,
                    X.MAX_DEPTH if max_depth is None else max_depth, pkg.CROSSING_FRONTIER if max_windows is None else max_windows)


def check(pkg, slv, rng=None, tol=None, max_depth=None, max_windows=None, st=None, ref=None):
    """device rows == the restatement on the state the solver holds; returns the device's answer"""
    a = slv.path_crossings(range=rng, tol=tol, max_depth=max_depth, max_windows=max_windows)
    want = restated(pkg, slv, slv.get_state() if st is None else st, rng, tol, max_depth, max_windows, ref)
    assert set(a) == set(NAMES)
    for n in ("robot", "partner") + X.FIELDS:
        assert np.array_equal(a[n], want[n]), (rng, tol, max_depth, max_windows, n, a[n], want[n])
    assert np.array_equal(a["gap"], want["partner_time"] - want["time"])
    assert list(zip(a["robot"], a["partner"])) == sorted(zip(a["robot"], a["partner"])) and np.all(a["robot"] < a["partner"])
    return a


def test_record_size_and_constants(pkg):
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert lib.tj_crossing_record_size() == C.sizeof(pkg.TjCrossingRecord) == 80
    for name, v in (("TOL", pkg.CROSSING_TOL), ("FRONTIER", pkg.CROSSING_FRONTIER), ("MAX_DEPTH", pkg.CROSSING_MAX_DEPTH), ("MAX_WINDOWS", pkg.CROSSING_MAX_WINDOWS)):
        assert float(re.search(r"#define TJ_CROSSING_%s\s+(\S+)" % name, hdr).group(1)) == v, name
    for n, v in pkg.CROSSING_FLAGS.items():
        assert int(re.search(r"#define TJ_CROSSING_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v


@pytest.mark.parametrize("name", ["tiny", "tiny_coupled", "hard"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """the initial state and the state after 3 iterations: default range at tol in {default, 0, 1e-3} and max_depth in {0, 1, 5, 40}; on tiny range = inf:
    all 3 pairs, all S^2 seeds"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1 if name == "tiny" else 2)
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 3):
        if it:
            slv.iterate(it)
        st = slv.get_state()
        ref = X.Ref(pkg, prims(), st, slv.P, slv.res)
        n = len(check(pkg, slv, st=st, ref=ref)["robot"])
        for tol in (0.0, 1e-3):
            check(pkg, slv, None, tol, st=st, ref=ref)
        for depth in (0, 1, 5, 40):
            check(pkg, slv, None, 0.0 if depth == 40 else None, depth, st=st, ref=ref)
        if name == "tiny":
            a = check(pkg, slv, INF, st=st, ref=ref)
            assert len(a["robot"]) == 3 and np.all(a["windows"] >= slv.S * slv.S)
            check(pkg, slv, INF, 1e-3, 5, st=st, ref=ref)
        else:
            assert n > 0
            check(pkg, slv, 1.0, None, 5, st=st, ref=ref)
    slv.close()


def test_constructed_states(pkg, scenes):
    """the X crossing, the skew pair, the goal on the other's path; then each robot with its own piece_time: the places stay, the times differ"""
    tol, F = pkg.CROSSING_TOL, pkg.CROSSING_FLAGS
    scene, st = X.x_state(pkg, scenes, 0.0)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, INF, st=st)
    assert len(a["robot"]) == 1 and a["lo"][0] == 0.0 and a["hi"][0] <= tol and a["depth"][0] >= 25 and a["flags"][0] & F["contact"] and not a["flags"][0] & F["clear"]
    assert abs(a["time"][0] - 2.12) <= 1e-9 and abs(a["partner_time"][0] - 4.0) <= 1e-9 and abs(a["gap"][0] - 1.88) <= 1e-9
    check(pkg, slv, st=st)
    st2 = R.scaled_time_state(R.scaled_time_state(st, 0, 0.7), 1, 3.1)
    slv.set_state(st2)
    b = check(pkg, slv, INF, st=st2)
    for n in ("lo", "hi", "s", "partner_s", "segment", "partner_segment", "depth", "windows", "flags"):
        assert np.array_equal(a[n], b[n]), n
    assert b["time"][0] == ((b["segment"][0] + b["s"][0]) / 8.0) * 0.7 != a["time"][0] and b["partner_time"][0] == ((b["partner_segment"][0] + b["partner_s"][0]) / 8.0) * 3.1
    slv.close()
    scene, st = X.x_state(pkg, scenes, 0.2)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, INF, st=st)
    assert len(a["robot"]) == 1 and a["lo"][0] <= 0.2 * (1 + 1e-10) + X.slack(32, st) and 0.2 - X.slack(32, st) <= a["hi"][0] and a["hi"][0] - a["lo"][0] <= tol
    assert a["flags"][0] == F["clear"] | F["converged"]
    assert len(check(pkg, slv, 0.15, st=st)["robot"]) == 0                            # 0.2 apart in space: no row at range 0.15
    slv.close()
    scene, st = X.goal_on_path_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, INF, st=st)
    assert len(a["robot"]) == 1 and a["flags"][0] & F["partner_end"] and a["flags"][0] & F["contact"] and not a["flags"][0] & F["robot_end"]
    assert (a["partner_segment"][0], a["partner_s"][0]) == (31, 1.0)
    slv.close()


def test_wide_live_sets(pkg, scenes):
    """two concentric arcs: a valley.  The pair's live set passes a wave (64) at the seeds and the refine workgroup (128) after one round (checked in the
    restatement first); then max_windows one below a round's size, and 8: TRUNCATED with the last completed round's record"""
    scene, st = X.arcs_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    ref = X.Ref(pkg, prims(), st, slv.P, slv.res)
    traces = {}
    ref.rows(INF, slv.params["offset"], 0.0, 2, X.MAX_WINDOWS, traces=traces)
    sizes = [t[3] for t in traces[(0, 1)]]
    print("live set of (0, 1) per depth", sizes)
    assert 64 < sizes[0] <= 128 < sizes[1] < sizes[2]
    a = check(pkg, slv, INF, 0.0, 2, sizes[2], st, ref)
    assert a["depth"][0] == 2 and not a["flags"][0] & pkg.CROSSING_FLAGS["truncated"]
    b = check(pkg, slv, INF, 0.0, 2, sizes[2] - 1, st, ref)
    prev = check(pkg, slv, INF, 0.0, 1, sizes[2], st, ref)
    assert b["flags"][0] & pkg.CROSSING_FLAGS["truncated"] and b["depth"][0] == 1 and b["windows"][0] == a["windows"][0]
    assert all(b[n][0] == prev[n][0] for n in X.FIELDS if n not in ("flags", "windows"))
    c = check(pkg, slv, INF, 0.0, 2, 8, st, ref)
    assert c["flags"][0] & pkg.CROSSING_FLAGS["truncated"] and c["depth"][0] == 0
    check(pkg, slv, INF, None, None, None, st, ref)                                    # the defaults: the frontier ends this valley
    slv.close()


def test_fleet_of_66(pkg, scenes):
    """partner indices beyond one and two 32-bit mask words, a second pass of 64 partners; rows in (robot, partner) order"""
    slv = pkg.Solver(scenes.crossing(66, 600), stop=0.0)
    slv.iterate(2)
    a = check(pkg, slv)
    assert len(a["robot"]) > 0 and a["partner"].max() >= 64 and np.any((a["partner"] >= 32) & (a["partner"] < 64))
    slv.close()


def test_capacity(pkg, scenes):
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(3)
    full = slv.path_crossings(range=INF, max_depth=6)
    n = len(full["robot"])
    assert n == slv.U * (slv.U - 1) // 2
    lib = slv.lib

    def call(rows, cap):
        got = C.c_int(-7)
        return lib.tj_path_crossings(slv._ctx, C.c_double(INF), C.c_double(-1.0), C.c_int(6), C.c_int(0), rows, C.c_int(cap), C.byref(got)), got.value

    assert call(None, 0) == (0, n)                                                  # count only
    rec = (pkg.TjCrossingRecord * n)()
    rec[n - 1].robot, rec[n - 1].lo = -99, 123.5
    assert call(rec, n - 1) == (-3, n)
    assert (rec[n - 1].robot, rec[n - 1].lo) == (-99, 123.5)                        # the sentinel behind the first n - 1 rows is untouched
    for k in range(n - 1):
        assert all(getattr(rec[k], f) == full[f][k] for f in X.FIELDS), k
    assert call(rec, n) == (0, n)
    assert all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in X.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n) == (0, n)                       # a smaller call after a larger one, and back
    slv.close()


@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_group_equals_one_context(pkg, scenes, ranks):
    one, grp = group_pair(pkg, scenes.hard(), ranks)

    def ask(s, rng, tol, depth):
        a = s.path_crossings(range=rng, tol=tol, max_depth=depth)
        assert set(a) == set(NAMES)
        return a

    x = assert_group_equals(one, grp, ask, ((None, None, None), (INF, 0.0, 6)))
    n = len(x["robot"])
    assert n == 6
    rec, got = (pkg.TjCrossingRecord * n)(), C.c_int(0)                   # a cap that ends inside a later rank's rows
    rc = grp.lib.tj_group_path_crossings(grp._g, C.c_double(INF), C.c_double(0.0), C.c_int(6), C.c_int(0), rec, C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in X.FIELDS)
    grp.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjCrossingRecord * 3)(), C.c_int(0)
        call = lambda r, t, d, w, out=rec, cap=3, n=C.byref(got): lib.tj_path_crossings(ctx, C.c_double(r), C.c_double(t), C.c_int(d), C.c_int(w), out, C.c_int(cap), n)
        assert call(0.0, -1.0, -1, 0) == -1                                   # before tj_init_state
        init()
        nan = float("nan")
        assert call(nan, -1.0, -1, 0) == -1 and call(0.0, nan, -1, 0) == -1 and call(0.0, -1.0, 41, 0) == -1 and call(0.0, -1.0, -1, 4097) == -1
        assert call(0.0, -1.0, -1, 0, n=None) == -1 and call(0.0, -1.0, -1, 0, cap=-1) == -1 and call(0.0, -1.0, -1, 0, out=None) == -1
        assert call(0.0, -1.0, -1, 4096, cap=1 << 20) == -1 and b"TJ_CROSSING_MAX_BYTES" in lib.tj_last_error(ctx)      # refused up front, nothing allocated
        assert call(INF, -1.0, 40, 4096) == 0 and got.value == 3 and call(0.0, 0.0, -1, 0) == 0                          # still usable; the limits themselves are valid
    assert_sharded_refuses(pkg, scenes, lambda half: half.path_crossings(), "tj_group_path_crossings")
    one = pkg.Solver(scenes.tiny(mode=0), stop=0.0)                       # single-UAV mode
    one.iterate(2)
    for rng in (None, INF):
        a = one.path_crossings(range=rng)
        assert set(a) == set(NAMES) and all(len(v) == 0 for v in a.values())
    one.close()


def test_path_crossings_is_read_only(pkg, scenes):
    """state, statistics and launch count are untouched; the other queries answer the same before and after; an iteration after the call gives the bits of
    an iteration without it"""
    def held(s):
        return s.get_state(), s.stats(), s.launch_count(), s.audit(), s.pair_approach(), s.flight_profile(samples=5)

    def same(x, y):
        if isinstance(x, dict):
            return set(x) == set(y) and all(np.array_equal(x[k], y[k]) for k in x)
        return x == y

    def ask_sync(s):
        before = held(s)
        s.path_crossings(); s.path_crossings(range=INF, tol=0.0, max_depth=3); s.path_crossings(range=1.0, max_depth=2, max_windows=1)
        assert all(same(x, y) for x, y in zip(before, held(s)))

    assert_read_only(pkg, scenes.hard(), lambda s: s.path_crossings(), ask_sync)


def test_command_line(pkg, scenes, tmp_path):
    """--path-crossings and --path-crossings 1e-6 (one context and a two-rank group): the printed rows are the library's on the dumped state, in its order --
    doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly -- and the summary line counts them"""
    cli = CliCase(pkg, scenes, tmp_path)
    # crossing uav U uav Q lo . hi . seg . s . time . seg . s . time . depth . windows . flags .
    names = ("lo", "hi", "segment", "s", "time", "partner_segment", "partner_s", "partner_time", "depth", "windows", "flags")
    for args, tol in ((["--path-crossings"], None), (["--path-crossings", "1e-6"], 1e-6)):
        for extra, lines in cli.queried(args, "crossing "):
            got = [l.split() for l in lines if l.startswith("crossing uav ")]
            a = cli.slv.path_crossings(tol=tol)
            assert len(got) == len(a["robot"]) > 0 and all(len(w) == 27 for w in got)
            for k, w in enumerate(got):
                assert (int(w[2]), int(w[4])) == (a["robot"][k], a["partner"][k])
                for i, n in enumerate(names):
                    if n in X.DOUBLES:
                        assert close_to_six_digits(w[6 + 2 * i], a[n][k]), (args, extra, k, n, w)
                    else:
                        assert int(w[6 + 2 * i]) == a[n][k], (args, extra, k, n, w)
            fleet = [l.split() for l in lines if l.startswith("crossing fleet ")]
            assert len(fleet) == 1
            contact = int(np.sum(a["flags"] & 1 != 0)); clear = int(np.sum((a["flags"] & 3) == 2))
            assert [int(fleet[0][i]) for i in (3, 5, 7, 9)] == [len(a["robot"]), contact, len(a["robot"]) - contact - clear, clear]
    cli.close()
