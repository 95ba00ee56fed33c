"""GPU (-m gpu): tj_obstacle_windows -- during which time intervals every robot's flown curve is within `dist` of the obstacle set.

Expected values come from tests/obstacle_windows_ref.py: the Python restatement of the header's definition (audit_ref's hulls, audit_timed_ref's blossoming, the
oracle's GJK, the walk's box predicate by brute force over all primitives, the classification OUT / IN / MIXED against the union, the search per segment, the
merge of the leaves into rows across segment boundaries, the row order).  Every field of every row is compared with == on doubles and ints, `windows`, `depth`,
`leaves` and `index` included, and so is the number of rows.  The restatement itself is held against the flown curve on the CPU
(tests/test_obstacle_windows_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import audit_ref as R
import obstacle_approach_ref as O
import obstacle_windows_ref as W
from audit_ref import prims
from query_kit import CliCase, assert_group_equals, assert_read_only, close_to_six_digits, group_pair, loaded, one_queue, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")


def ref_for(pkg, slv, scene, st=None):
    return W.ref_of(pkg, prims(), slv.get_state() if st is None else st, slv.P, slv.res, O.prims_of(scene))


def check(pkg, slv, ref, dist=None, tol=None, max_depth=None, max_windows=None, owned=None):
    """device rows == the restatement `ref` (built on the state the solver holds); returns the device's answer"""
    p = slv.params
    d = p["offset"] if dist is None else dist
    a = slv.obstacle_windows(dist=dist, tol=tol, max_depth=max_depth, max_windows=max_windows)
    exp = ref.rows(d, W.default_tol(d, p["offset"], p["vel_limit"]) if tol is None else tol, W.MAX_DEPTH if max_depth is None else max_depth,
                   pkg.OBSWIN_FRONTIER if max_windows is None else max_windows, owned=owned)
    assert set(a) == set(W.FIELDS)
    for n in ("robot",) + W.FIELDS:
        assert np.array_equal(a[n], exp[n]), (dist, tol, max_depth, max_windows, n, a[n], exp[n])
    key = list(zip(a["robot"], a["t_first_lo"]))
    assert key == sorted(key)
    return a


def test_row_size(pkg):
    assert pkg.load_library().tj_obswin_row_size() == C.sizeof(pkg.TjObswinRow) == 88


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """after 0, 1 and 3 iterations; dist in {default, offset + 2 * margin}; tol = 0 with max_depth = 3: the depth stop and the EDGE leaves"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    big = slv.params["offset"] + 2 * slv.params["margin"]
    far = 0.5 if name == "tiny_single" else big   # (the single-UAV scene keeps its cloud 0.3 and more from the flight: one more distance, at which it has rows)
    rows = edges = 0
    for it in (0, 1, 2):   # (iterations 0, 1 and 3 of the run)
        if it:
            slv.iterate(it)
        ref = ref_for(pkg, slv, scene)
        for dist in (None, big, far):
            rows += len(check(pkg, slv, ref, dist)["robot"])
        a = check(pkg, slv, ref, far, 0.0, 3)
        edges += int(np.sum(a["depth"] == 3))
    assert rows > 0 and edges > 0
    slv.close()


@pytest.mark.parametrize("name", W.STATES)
def test_constructed_states(pkg, scenes, name):
    """the CPU file's states: the pierce row is a chain across a segment boundary; the 150-point cluster makes process(pt) run three times in one walk and
    accumulate across the calls; the two-point states merge into one row and split into two"""
    scene, st, dist, ref, rows, _ = W.built(pkg, scenes, prims(), name)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, ref, dist)
    for n in W.FIELDS:
        assert np.array_equal(a[n], rows[n]), n
    F = pkg.OBSWIN_FLAGS
    assert np.all(a["flags"] == F["certain"] | F["resolved"]) and len(a["robot"]) == (2 if name == "two_far" else 1)
    if name == "pierce":
        assert (a["segment_first"][0], a["segment_last"][0], a["index"][0]) == (24, 25, 77)
    if name == "cluster":
        assert np.sum(np.linalg.norm(scene["cloud"] - np.array([1.3, 0.0, 0.0]), axis=1) <= dist) == 150
        check(pkg, slv, ref, dist, 0.0, 6)
    slv.close()


def test_a_segment_with_a_second_block_of_leaves(pkg, scenes):
    """k_obwin_place indexes a segment's chain heads in blocks of 64 leaves; no other state of this file gives a segment more than 25.  The straight flight
    x = -5 + 2 t with tol = 0 and max_depth = 40, segment 25 (x in [1.25, 1.5]).  Points 77 and 78 at x = 1.3 and 1.325 with dist = 0.05 - 1e-11 are within
    dist over x in [1.25 + 1e-11, 1.375 - 1e-11]: one crossing just behind the segment's start and one just before its midpoint, so nearly every halving
    leaves an IN child behind and the chain has 68 leaves.  Point 79 at x = 1.45 adds a second chain, whose head is leaf 68.  Asserted on the restatement,
    so that the case cannot stop reaching the path: more than 64 leaves in one segment, a chain across leaf 64, a chain head in the second block."""
    dist = 0.05 - 1e-11
    scene, st = W.two_point_state(pkg, scenes, 0.025)
    scene["cloud"][79] = (1.45, 0.0, 0.0)
    slv = loaded(pkg, scene, st)
    ref = ref_for(pkg, slv, scene, st)
    found = ref.search(0, 25, dist, 0.0, 40, pkg.OBSWIN_FRONTIER)
    lv = found["leaves"]
    heads = [k for k in range(1, len(lv)) if lv[k - 1][1] != lv[k][0]]
    assert len(lv) > 64 and lv[63][1] == lv[64][0] and any(k > 64 for k in heads) and not found["truncated"]
    a = check(pkg, slv, ref, dist, 0.0, 40)
    assert list(a["leaves"]) == [heads[0], len(lv) - heads[0]] and list(a["segment_first"]) == list(a["segment_last"]) == [25, 25]
    assert np.all(a["flags"] == pkg.OBSWIN_FLAGS["certain"]) and np.all(a["depth"] == 40)
    slv.close()


@pytest.mark.parametrize("P,res", [(12, 8), (2, 16)])
def test_segment_counts_and_resolutions(pkg, scenes, P, res):
    scene = dict(scenes.hard(4, 3000, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    ref = ref_for(pkg, slv, scene, st)
    check(pkg, slv, ref)
    assert len(check(pkg, slv, ref, 0.3)["robot"]) > 0
    slv.close()


def test_per_robot_piece_time(pkg, scenes):
    """a decoupled state with piece_time[u] scaled by 1 + 0.03 * u: every time is formed with the robot's own piece_time"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    st = slv.get_state()
    st["piece_time"] = st["piece_time"] * (1 + 0.03 * np.arange(slv.U))
    slv.set_state(st)
    ref = ref_for(pkg, slv, scene, st)
    a = check(pkg, slv, ref, 0.3)
    assert len(set(a["robot"])) > 1
    slv.close()


def test_placement_across_a_wave_of_robots(pkg, scenes):
    """a fleet of 65 in which only robots 0, 31, 32 and 64 have rows (two each): the scan of the row counts crosses one wave, most robots contribute nothing"""
    base = scenes.crossing(65, 120)
    cloud = np.array(base["cloud"]) + np.array([0.0, 0.0, 80.0])                            # out of every range
    who = (0, 31, 32, 64)
    for k, u in enumerate(who):
        a, b = base["waypoints"][u][0], base["waypoints"][u][-1]
        cloud[2 * k], cloud[2 * k + 1] = a + (b - a) * 0.1, a + (b - a) * 0.8                # on u's line, 8 and 6 from the centre: 0.3 or more from every other line
    scene = dict(base, cloud=np.ascontiguousarray(cloud))
    slv = pkg.Solver(scene, stop=0.0)
    ref = ref_for(pkg, slv, scene)
    a = check(pkg, slv, ref)
    assert list(a["robot"]) == [0, 0, 31, 31, 32, 32, 64, 64]
    slv.close()


def test_triangles_and_degenerate_triangles(pkg, scenes):
    """a mesh; and triangles of three equal vertices, which must behave like the points: the same rows as the cloud's restatement, every field"""
    base = scenes.tiny(mode=1)
    scene = scenes.triangulate(base)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    ref = ref_for(pkg, slv, scene)
    assert len(check(pkg, slv, ref, 0.3)["robot"]) > 0
    check(pkg, slv, ref)
    slv.close()
    deg = scenes.triangulate(base, degenerate=True)
    slv = pkg.Solver(deg, stop=0.0)
    st = R.port_state(base, 2)
    slv.set_state(st)
    as_tris, as_cloud = ref_for(pkg, slv, deg, st), ref_for(pkg, slv, base, st)
    x = check(pkg, slv, as_tris, 0.3)
    y = check(pkg, slv, as_cloud, 0.3)
    assert len(x["robot"]) > 0 and all(np.array_equal(x[n], y[n]) for n in W.FIELDS)
    slv.close()


def test_truncation_and_capacity(pkg, scenes):
    """max_windows = 1 and 2 on the two-point state: TRUNCATED rows == the restatement's last completed round; cap below *n: TJ_ERR_CAPACITY, the exact *n and
    the first cap rows; the count-only call returns the same *n"""
    scene, st, dist, ref, rows, _ = W.built(pkg, scenes, prims(), "two_far")
    slv = loaded(pkg, scene, st)
    seen = 0
    for mw in (1, 2):
        a = check(pkg, slv, ref, dist, None, None, mw)
        seen += int(np.sum(a["flags"] & pkg.OBSWIN_FLAGS["truncated"] != 0))
    assert seen > 0
    full = check(pkg, slv, ref, dist)
    n = len(full["robot"])
    assert n == 2

    def call(rec, cap):
        got = C.c_int(-7)
        return slv.lib.tj_obstacle_windows(slv._ctx, C.c_double(dist), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rec, C.c_int(cap), C.byref(got)), got.value

    assert call(None, 0) == (0, n)
    rec = (pkg.TjObswinRow * n)()
    for k in range(n):
        rec[k].robot, rec[k].closest = -99, 123.5
    assert call(rec, 1) == (-3, n)
    assert (rec[1].robot, rec[1].closest) == (-99, 123.5)                                   # the sentinel behind the first cap rows is untouched
    assert all(getattr(rec[0], f) == full[f][0] for f in W.FIELDS)
    assert call(rec, n) == (0, n) and all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in W.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n + 3) == (0, n)                            # a smaller call after a larger one, and back
    slv.close()


def test_empty_and_infinite(pkg, scenes):
    """an empty cloud: 0 rows; dist = +infinity on a 200-point cloud: one row per robot, the whole flight, within_lo = the duration summed left to right"""
    scene = scenes.tiny(mode=1, n_points=200)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(1)
    ref = ref_for(pkg, slv, scene)
    a = check(pkg, slv, ref, INF)
    F = pkg.OBSWIN_FLAGS
    assert list(a["robot"]) == list(range(slv.U)) and np.all(a["flags"] & ~F["resolved"] == F["certain"] | F["at_start"] | F["at_end"])
    assert np.all(a["leaves"] == slv.S) and np.all(a["depth"] == 0) and np.all(a["windows"] == slv.S)
    pt = slv.get_state()["piece_time"]
    for u in range(slv.U):
        dur = 0.0
        for _ in range(slv.S):
            dur += ((1.0 - 0.0) / float(slv.res)) * float(pt[u])
        assert a["within_lo"][u] == dur and a["t_first_lo"][u] == 0.0 and a["t_last_hi"][u] == ((slv.S - 1 + 1.0) / float(slv.res)) * float(pt[u])
    cloud = np.zeros((0, 3))
    assert slv.lib.tj_set_cloud(slv._ctx, cloud.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(0)) == 0
    for dist in (None, INF):
        b = slv.obstacle_windows(dist=dist)
        assert set(b) == set(W.FIELDS) and all(len(b[f]) == 0 for f in W.FIELDS)
    slv.close()


def test_walk_overflow_is_an_error_for_a_context_and_for_a_group(pkg, scenes):
    """9000 points at dist = +infinity: every leaf box is a candidate, more than FRONT_CAP = 1024 boxes of 8, so the walk's frontier overflows.  One context and a
    group both return TJ_ERR_CAPACITY (-3) and leave *n untouched -- never fewer rows, never an empty answer -- and both answer as before afterwards.  Deliberate
    error returns: the walk sets its bit and ends (tests/test_gpu_audit.py::test_frontier_overflow_is_an_error_and_leaves_everything_usable)."""
    scene = scenes.tiny(mode=1, n_points=9000)
    assert scene["cloud"].shape[0] > 8 * 1024
    one = pkg.Solver(scene, stop=0.0)
    grp = pkg.Group(scene, [0, 0], stop=0.0)
    before = one.obstacle_windows(dist=0.3)
    assert len(before["robot"]) > 0
    rec = (pkg.TjObswinRow * 8)()
    rec[0].robot = -99
    for who, fn, handle in (("context", one.lib.tj_obstacle_windows, one._ctx), ("group", grp.lib.tj_group_obstacle_windows, grp._g)):
        for out, cap in ((None, 0), (rec, 8)):
            got = C.c_int(-7)
            rc = fn(handle, C.c_double(INF), C.c_double(-1.0), C.c_int(-1), C.c_int(0), out, C.c_int(cap), C.byref(got))
            assert (rc, got.value, rec[0].robot) == (-3, -7, -99), (who, cap, rc, got.value)
    for s in (one, grp):
        with pytest.raises(pkg.TrajAdmmError) as ei:
            s.obstacle_windows(dist=INF)
        assert "-3" in str(ei.value) and "dist" in str(ei.value)
        after = s.obstacle_windows(dist=0.3)
        assert all(np.array_equal(after[n], before[n]) for n in W.FIELDS)
    grp.close(); one.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_obstacle_windows_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    assert_read_only(pkg, scenes.hard(), lambda s: s.obstacle_windows(dist=1.0, tol=0.0, max_depth=4),
                     lambda s: (s.obstacle_windows(), s.obstacle_windows(dist=0.3, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    x = assert_group_equals(one, grp, lambda s, dist, tol: s.obstacle_windows(dist=dist, tol=tol, max_depth=6), ((None, None), (0.3, None), (0.3, 0.0)))
    n = len(x["robot"])
    assert n > 2
    rec, got = (pkg.TjObswinRow * n)(), C.c_int(0)                                          # a cap that ends inside the rows: the exact total, the first rows
    rc = grp.lib.tj_group_obstacle_windows(grp._g, C.c_double(0.3), C.c_double(0.0), C.c_int(6), C.c_int(0), rec, C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in W.FIELDS)
    grp.close(); one.close()


def test_sharded_context_answers_for_its_own_robots(pkg, scenes):
    scene = scenes.hard()
    one = pkg.Solver(scene, stop=0.0)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)
    x, y = one.obstacle_windows(dist=0.3), half.obstacle_windows(dist=0.3)
    mine = sorted(set(y["robot"]))
    assert 0 < len(mine) < scene["U"] and mine == list(range(mine[0], mine[-1] + 1))
    keep = np.isin(x["robot"], mine)
    for k in x:
        assert np.array_equal(x[k][keep], y[k]), k
    check(pkg, half, ref_for(pkg, one, scene), 0.3, owned=[int(u) for u in mine])
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    """the precedence: null, then NaN, then limits, then no state; the outputs stay untouched"""
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjObswinRow * 12)(), C.c_int(-7)
        rec[0].robot = -99
        nan = float("nan")

        def call(d, t, depth, w, out=rec, cap=12, n=C.byref(got)):
            rc = lib.tj_obstacle_windows(ctx, C.c_double(d), C.c_double(t), C.c_int(depth), C.c_int(w), out, C.c_int(cap), n)
            if rc == -1:
                assert (got.value, rec[0].robot) == (-7, -99)                                  # the outputs are untouched
            return rc, lib.tj_last_error(ctx)

        rc, msg = call(0.0, -1.0, -1, 0)                                                       # before tj_init_state
        assert rc == -1 and b"tj_init_state" in msg
        rc, msg = call(nan, -1.0, 41, 0)                                                       # NaN before the limits, the limits before the missing state
        assert rc == -1 and b"NaN" in msg
        rc, msg = call(0.0, -1.0, 41, 0)
        assert rc == -1 and b"max_depth" in msg
        assert call(nan, -1.0, -1, 0, n=None)[0] == -1 and call(0.0, -1.0, -1, 0, cap=-1)[0] == -1 and call(0.0, -1.0, -1, 0, out=None)[0] == -1
        init()
        assert call(nan, -1.0, -1, 0)[0] == -1 and call(0.0, nan, -1, 0)[0] == -1 and call(0.0, -1.0, 41, 0)[0] == -1 and call(0.0, -1.0, -1, pkg.OBSWIN_MAX_WINDOWS + 1)[0] == -1
        rc, msg = call(0.0, -1.0, -1, pkg.OBSWIN_MAX_WINDOWS, cap=1 << 25)                     # refused up front, nothing allocated
        assert rc == -1 and b"TJ_OBSWIN_MAX_BYTES" in msg
        for args in ((0.0, -1.0, 40, pkg.OBSWIN_MAX_WINDOWS), (0.05, 0.0, -1, 0), (INF, -1.0, 0, 1)):   # the limits themselves are valid; no obstacle set at all: 0 rows
            got.value = -7
            assert call(*args)[0] == 0 and got.value == 0 and rec[0].robot == -99


def test_command_line(pkg, scenes, tmp_path):
    """--obstacle-windows 0.3 (one context and a two-rank group): the printed rows are the library's on the dumped state, in its order -- doubles to 6
    significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly -- and the fleet's line counts them"""
    cli = CliCase(pkg, scenes, tmp_path)
    doubles = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "closest", "closest_time")
    ints = ("index", "segment_first", "segment_last", "leaves", "depth", "windows", "flags")
    for extra, lines in cli.queried(["--obstacle-windows", "0.3"], "obswin "):
        got = [l.split() for l in lines if l.startswith("obswin uav ")]
        a = cli.slv.obstacle_windows(dist=0.3)
        assert len(got) == len(a["robot"]) > 0 and all(len(w) == 28 for w in got)
        for k, w in enumerate(got):
            assert int(w[2]) == a["robot"][k]
            for n, i in zip(doubles, (4, 5, 7, 8, 10, 12, 14)):
                assert close_to_six_digits(w[i], a[n][k]), (extra, k, n, w)
            assert [int(w[i]) for i in (16, 18, 19, 21, 23, 25, 27)] == [a[n][k] for n in ints], (extra, k, w)
        fleet = [l.split() for l in lines if l.startswith("obswin fleet ")]
        assert len(fleet) == 1 and int(fleet[0][3]) == len(a["robot"])
    cli.close()
