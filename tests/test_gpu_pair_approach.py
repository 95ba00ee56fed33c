"""GPU (-m gpu): tj_pair_approach -- every directed robot pair that comes close at EQUAL FLIGHT TIMES, each converged by its own branch and bound.

Expected values come from tests/pair_approach_ref.py: the Python restatement of the header's definition (closest_ref's windows and evaluation, the search per
pair, the listed rule, the row order).  Every field of every row is compared with == on doubles and ints, `windows` and `depth` included, and so is the number
of rows: the bar tests/test_gpu_closest.py holds.  The restatement itself is held against the flown curves on the CPU (tests/test_pair_approach_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import pair_approach_ref as Q
from audit_ref import prims
from query_kit import (CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, close_to_six_digits, group_pair, loaded, one_queue,
                       raw_context)

pytestmark = pytest.mark.gpu
INF = float("inf")


def restated(pkg, slv, st, rng=None, tol=None, max_depth=None, max_windows=None):
    p = slv.params
    return Q.pair_rows(pkg, prims(), st, slv.P, slv.res, p["offset"] + 2 * p["margin"] if rng is None else rng, p["offset"], pkg.PAIR_TOL if tol is None else tol,
                       Q.MAX_DEPTH if max_depth is None else max_depth, pkg.PAIR_FRONTIER if max_windows is None else max_windows)


def check(pkg, slv, rng=None, tol=None, max_depth=None, max_windows=None, st=None):
    """device rows == the restatement on the state the solver holds; returns the device's answer"""
    a = slv.pair_approach(range=rng, tol=tol, max_depth=max_depth, max_windows=max_windows)
    ref = restated(pkg, slv, slv.get_state() if st is None else st, rng, tol, max_depth, max_windows)
    assert set(a) == set(Q.FIELDS)
    for n in ("robot", "partner") + Q.FIELDS:
        assert np.array_equal(a[n], ref[n]), (rng, tol, max_depth, max_windows, n, a[n], ref[n])
    assert list(zip(a["robot"], a["partner"])) == sorted(zip(a["robot"], a["partner"]))
    return a


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """after 0, 1 and 4 iterations; range in {default, 1.0, inf}"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1 if name == "tiny" else 2)
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 1, 3):
        if it:
            slv.iterate(it)
        st = slv.get_state()
        for rng in (None, 1.0, INF):
            check(pkg, slv, rng, st=st)
        check(pkg, slv, INF, 0.0, 3, st=st)
    slv.close()


def test_depth_zero_is_audit_timed_level_zero(pkg, scenes):
    """per robot the smallest row in the order (hi, segment, partner, time) is tj_audit_timed's level-0 upper end, bit for bit, and the smallest lo its lower"""
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(4)
    for rng in (None, 1.0, INF):
        a, t = slv.pair_approach(range=rng, max_depth=0), slv.audit_timed(range=rng, levels=0)
        assert np.all(a["depth"] == 0)
        for u in range(slv.U):
            m = np.flatnonzero(a["robot"] == u)
            s = [k for k in m if a["segment"][k] >= 0]
            if not s:
                assert t["timed_robot"][u] == -1
            else:
                k = min(s, key=lambda k: (a["hi"][k], a["segment"][k], a["partner"][k], a["time"][k]))
                assert (a["hi"][k], a["time"][k], a["partner"][k], a["segment"][k]) == (t["timed_hi"][u], t["timed_time"][u], t["timed_robot"][u], t["timed_segment"][u]), u
            if len(m):
                assert a["lo"][m].min() == min(t["timed_lo"][u], t["timed_hi"][u]), u
    slv.close()


def test_constructed_states(pkg, scenes):
    tol, F = pkg.PAIR_TOL, pkg.PAIR_FLAGS
    scene, st, t_meet, t_goal = T.chase_state(pkg, scenes)
    sl = T.slack(32, st["spline"])
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, INF, st=st)
    assert list(zip(a["robot"], a["partner"])) == [(0, 1), (1, 0)] and np.all(a["flags"] & F["contact"]) and abs(a["time"][0] - t_meet) <= 1e-5
    assert min(abs(a["time"][1] - t_meet), abs(a["time"][1] - t_goal)) <= 1e-5      # robot 1 meets robot 0 twice, both at rounding level: which one is not pinned
    slv.close()
    scene, st = T.crossing_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, INF, st=st)
    assert len(a["robot"]) == 2 and np.all(a["flags"] == F["clear"] | F["converged"]) and abs(a["hi"][0] - math.sqrt(5.0)) <= tol + sl
    assert len(check(pkg, slv, st=st)["robot"]) == 0                                    # nothing within the default range: no row
    slv.close()
    scene, st, t_meet = T.hover_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, INF, st=st)
    assert list(zip(a["robot"], a["partner"])) == [(0, 1), (1, 0)]
    assert a["flags"][1] & F["contact"] and abs(a["time"][1] - t_meet) <= 1e-5 and a["flags"][0] & F["clear"] and not a["flags"][0] & F["contact"]
    slv.close()


@pytest.mark.parametrize("U", [64, 65, 130])
def test_fleet_sizes(pkg, scenes, U):
    """the partner passes at, just over and at twice a wave; the bitmask's rows at 2, 3 and 5 words"""
    slv = pkg.Solver(scenes.crossing(U, 500), stop=0.0)
    slv.iterate(2)
    a = check(pkg, slv)
    assert len(a["robot"]) > 0
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
    check(pkg, slv, INF, st=st)
    slv.close()


def test_wide_live_sets(pkg, scenes):
    """a pair whose live set passes twice the refine workgroup's 64 lanes (pair_approach_ref.orbit_state: the set doubles per round), then the same search
    with max_windows one below that size: TRUNCATED with the previous round's record"""
    scene, st = Q.orbit_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    traces = {}
    Q.pair_rows(pkg, prims(), st, slv.P, slv.res, INF, slv.params["offset"], 0.0, 4, Q.MAX_WINDOWS, traces=traces)
    sizes = [t[3] for t in traces[(0, 1)]]
    depth = next(d for d, n in enumerate(sizes) if n > 128)
    print("live set of (0, 1) per depth", sizes, "-> max_depth", depth)
    assert depth >= 1 and sizes[depth - 1] <= 128
    a = check(pkg, slv, INF, 0.0, depth, sizes[depth], st)
    assert np.all(a["depth"] == depth) and not np.any(a["flags"] & pkg.PAIR_FLAGS["truncated"])
    b = check(pkg, slv, INF, 0.0, depth, sizes[depth] - 1, st)
    assert b["flags"][0] & pkg.PAIR_FLAGS["truncated"] and b["depth"][0] == depth - 1 and b["windows"][0] == a["windows"][0]
    prev = check(pkg, slv, INF, 0.0, depth - 1, sizes[depth], st)
    assert (b["lo"][0], b["hi"][0], b["time"][0], b["segment"][0]) == (prev["lo"][0], prev["hi"][0], prev["time"][0], prev["segment"][0])
    slv.close()


def test_capacity(pkg, scenes):
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(4)
    full = slv.pair_approach(range=INF)
    n = len(full["robot"])
    assert n == slv.U * (slv.U - 1)
    lib = slv.lib

    def call(rows, cap):
        got = C.c_int(-7)
        return lib.tj_pair_approach(slv._ctx, C.c_double(INF), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rows, C.c_int(cap), C.byref(got)), got.value

    assert call(None, 0) == (0, n)
    rec = (pkg.TjPairRecord * n)()
    rec[n - 1].robot, rec[n - 1].lo = -99, 123.5
    assert call(rec, n - 1) == (-3, n)
    assert (rec[n - 1].robot, rec[n - 1].lo) == (-99, 123.5)                        # the sentinel behind the first n - 1 rows is untouched
    for k in range(n - 1):
        assert all(getattr(rec[k], f) == full[f][k] for f in Q.FIELDS), k
    assert call(rec, n) == (0, n)
    assert all(getattr(rec[n - 1], f) == full[f][n - 1] for f in Q.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n) == (0, n)                       # a smaller call after a larger one, and back
    slv.close()


def test_symmetry_in_coupled_mode(pkg, scenes):
    """all robots share piece_time, so both flights end together: (q, u) is listed with (u, q), and the two brackets overlap"""
    slv = pkg.Solver(scenes.tiny(mode=2), stop=0.0)
    slv.iterate(3)
    for rng in (None, 1.0):
        a = check(pkg, slv, rng)
        at = {(u, q): k for k, (u, q) in enumerate(zip(a["robot"], a["partner"]))}
        assert at or rng is None
        for (u, q), k in at.items():
            assert (q, u) in at, (u, q)
            assert a["lo"][k] <= a["hi"][at[(q, u)]] and a["lo"][at[(q, u)]] <= a["hi"][k]
        m = slv.pair_approach(range=rng, symmetric=True)
        ref = Q.merge_symmetric(a, slv.params["offset"] + 2 * slv.params["margin"] if rng is None else rng, slv.params["offset"])
        assert set(m) == set(ref) and all(np.array_equal(m[n], ref[n]) for n in ref)
    slv.close()


def test_triangle_scene(pkg, scenes):
    """obstacles do not matter"""
    slv = pkg.Solver(scenes.triangulate(scenes.tiny(mode=1)), stop=0.0)
    slv.iterate(3)
    check(pkg, slv)
    check(pkg, slv, 1.0)
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_pair_approach_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    assert_read_only(pkg, scenes.hard(), lambda s: s.pair_approach(range=INF, tol=0.0),
                     lambda s: (s.pair_approach(), s.pair_approach(range=1.0, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    x = assert_group_equals(one, grp, lambda s, rng, tol: s.pair_approach(range=rng, tol=tol), ((None, None), (INF, 0.0)))
    n = len(x["robot"])
    rec, got = (pkg.TjPairRecord * n)(), C.c_int(0)                       # a cap that ends inside a later rank's rows
    rc = grp.lib.tj_group_pair_approach(grp._g, C.c_double(INF), C.c_double(0.0), C.c_int(-1), C.c_int(0), rec, C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in Q.FIELDS)
    grp.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjPairRecord * 6)(), C.c_int(0)
        call = lambda r, t, d, w, out=rec, cap=6, n=C.byref(got): lib.tj_pair_approach(ctx, C.c_double(r), C.c_double(t), C.c_int(d), C.c_int(w), out, C.c_int(cap), n)
        assert call(0.0, -1.0, -1, 0) == -1                                   # before tj_init_state
        init()
        nan = float("nan")
        assert call(nan, -1.0, -1, 0) == -1 and call(0.0, nan, -1, 0) == -1 and call(0.0, -1.0, 41, 0) == -1 and call(0.0, -1.0, -1, 4097) == -1
        assert call(0.0, -1.0, -1, 0, n=None) == -1 and call(0.0, -1.0, -1, 0, cap=-1) == -1 and call(0.0, -1.0, -1, 0, out=None) == -1
        assert call(0.0, -1.0, -1, 4096, cap=1 << 20) == -1 and b"TJ_PAIR_MAX_BYTES" in lib.tj_last_error(ctx)      # refused up front, nothing allocated
        assert call(INF, -1.0, 40, 4096) == 0 and got.value == 6 and call(0.0, 0.0, -1, 0) == 0                                  # still usable; the limits themselves are valid
    assert_sharded_refuses(pkg, scenes, lambda half: half.pair_approach(), "tj_group_pair_approach")
    one = pkg.Solver(scenes.tiny(mode=0), stop=0.0)
    one.iterate(2)
    for rng in (None, INF):
        a = one.pair_approach(range=rng)
        assert set(a) == set(Q.FIELDS) and all(len(v) == 0 for v in a.values())
    one.close()


def test_command_line(pkg, scenes, tmp_path):
    """--pair-approach and --pair-approach 1e-6 (one context and a two-rank group): the printed rows are the library's on the dumped state, in its order --
    doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly -- and the summary line counts them"""
    cli = CliCase(pkg, scenes, tmp_path)
    names = ("lo", "hi", "segment", "time", "depth", "windows", "flags")
    for args, tol in ((["--pair-approach"], None), (["--pair-approach", "1e-6"], 1e-6)):
        for extra, lines in cli.queried(args, "pair "):
            got = [l.split() for l in lines if l.startswith("pair uav ")]
            a = cli.slv.pair_approach(tol=tol)
            assert len(got) == len(a["robot"]) and all(len(w) == 19 for w in got)
            for k, w in enumerate(got):
                assert (int(w[2]), int(w[4])) == (a["robot"][k], a["partner"][k])
                for i, n in enumerate(names):
                    if n in ("lo", "hi", "time"):
                        assert close_to_six_digits(w[6 + 2 * i], a[n][k]), (args, extra, k, n, w)
                    else:
                        assert int(w[6 + 2 * i]) == a[n][k], (args, extra, k, n, w)
            fleet = [l.split() for l in lines if l.startswith("pair fleet ")]
            assert len(fleet) == 1
            contact = int(np.sum(a["flags"] & 1 != 0)); clear = int(np.sum((a["flags"] & 3) == 2))
            assert [int(fleet[0][i]) for i in (3, 5, 7, 9)] == [len(a["robot"]), contact, len(a["robot"]) - contact - clear, clear]
    cli.close()
