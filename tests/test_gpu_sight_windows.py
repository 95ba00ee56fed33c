"""GPU (-m gpu): tj_sight_windows -- during which time intervals the straight line between two robots at equal flight times, or between a robot and a fixed
station, passes within `dist` of the obstacle set.

Expected values come from tests/sight_windows_ref.py: the Python restatement of the header's definition (audit_ref's hulls, audit_timed_ref's blossoming and
cuts, the oracle's GJK on the 12-point body, the walk's box predicate by brute force over all primitives, the samples, the fixed-lambda IN test, the search per
(link, segment), the merge across segment boundaries, the row order).  Every field of every row is compared with == on doubles and ints, and so is the number
of rows.  The restatement itself is held against the flown link on the CPU (tests/test_sight_windows_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import audit_ref as R
import obstacle_approach_ref as O
import sight_windows_ref as W
from audit_ref import prims
from query_kit import CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, close_to_six_digits, group_pair, loaded, one_queue, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def station_of(scene):
    """one station per scene: the obstacle set's centroid, 1.0 above its top"""
    X = O.prims_of(scene).reshape(-1, 3)
    s = X.mean(axis=0)
    s[2] = X[:, 2].max() + 1.0
    return s[None, :]


def ref_for(pkg, slv, scene, st=None, stations=None):
    return W.ref_of(pkg, prims(), slv.get_state() if st is None else st, slv.P, slv.res, O.prims_of(scene), station_of(scene) if stations is None else stations)


def check(pkg, slv, ref, links=None, dist=None, tol=None, max_depth=None, max_windows=None):
    """device rows == the restatement `ref` (built on the state the solver holds, with its stations); returns the device's answer"""
    p = slv.params
    d = p["offset"] if dist is None else dist
    a = slv.sight_windows(links=links, stations=ref.stations, dist=dist, tol=tol, max_depth=max_depth, max_windows=max_windows)
    exp = ref.rows(links, d, W.default_tol(d, p["offset"], p["vel_limit"]) if tol is None else tol, W.MAX_DEPTH if max_depth is None else max_depth,
                   pkg.SIGHT_FRONTIER if max_windows is None else max_windows)
    assert set(a) == set(W.FIELDS)
    for n in ("link",) + W.FIELDS:
        assert np.array_equal(a[n], exp[n]), (links, dist, tol, max_depth, max_windows, n, a[n], exp[n])
    key = list(zip(a["link"], a["t_first_lo"]))
    assert key == sorted(key)
    return a


def test_row_size(pkg):
    assert pkg.load_library().tj_sight_row_size() == C.sizeof(pkg.TjSightRow) == 88


RUN_LINKS = {"hard": [(0, 1), (3, 1), (2, 0), (1, -1), (2, -1)], "tiny": None, "tiny_coupled": None, "tiny_single": [(0, -1)]}
RUN_FAR = {"hard": 0.5, "tiny": 0.6, "tiny_coupled": 0.6, "tiny_single": 1.0}
RUN_EDGE = {"hard": None, "tiny": 0.6, "tiny_coupled": 0.6, "tiny_single": None}   # where max_depth = 3 leaves windows undecided (hard's cloud is dense: at 0.5 every seed is IN)


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """after 0, 1 and 3 iterations; dist in {default, offset + 2 * margin, a larger one}; tol = 0 with max_depth = 3: the depth stop and the EDGE leaves.
    hard(): a robot pair in both rank orders, a second pair and two station links; the tiny scenes: every link; the single-UAV scene: its station link"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    big, far, links = slv.params["offset"] + 2 * slv.params["margin"], RUN_FAR[name], RUN_LINKS[name]
    rows = edges = 0
    for it in (0, 1, 2):   # (iterations 0, 1 and 3 of the run)
        if it:
            slv.iterate(it)
        ref = ref_for(pkg, slv, scene)
        for dist in (None, big, far):
            rows += len(check(pkg, slv, ref, links, dist)["link"])
        a = check(pkg, slv, ref, links, RUN_EDGE[name], 0.0, 3)
        edges += int(np.sum(a["depth"] == 3))
    assert rows > 0 and edges > 0
    slv.close()


@pytest.mark.parametrize("name", W.STATES)
def test_constructed_states(pkg, scenes, name):
    """the CPU file's states: the pillar's row is a chain across a segment boundary of a, hover's across b's arrival, staggered's across b's segment cuts; the
    station's IN leaves come from a lambda far from both ends; the 150-point cluster makes process(pt) run three times in one walk"""
    scene, st, stations, links, dist, ref, rows, _ = W.built(pkg, scenes, prims(), name)
    slv = loaded(pkg, scene, st)
    a = check(pkg, slv, ref, links, dist)
    for n in W.FIELDS:
        assert np.array_equal(a[n], rows[n]), n
    F = pkg.SIGHT_FLAGS
    assert len(a["link"]) == (0 if name == "graze_out" else 1)
    if name not in ("graze_out", "graze_in"):
        assert np.all(a["flags"] == F["certain"] | F["resolved"])
    if name == "cluster":
        check(pkg, slv, ref, links, dist, 0.0, 6)
    slv.close()


def test_a_segment_with_a_second_block_of_leaves(pkg, scenes):
    """k_sight_place indexes a segment's chain heads in blocks of 64 leaves: the pillar's flight with tol = 0 and max_depth = 40 leaves more than 64 leaves in
    segment 25 of a and a second chain whose head lies in the second block (asserted on the restatement, so that the case cannot stop reaching the path)"""
    scene, st, dist = W.many_leaves_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    ref = ref_for(pkg, slv, scene, st, np.zeros((0, 3)))
    found = ref.search(0, 1, 25, dist, 0.0, 40, pkg.SIGHT_FRONTIER)
    lv = found["leaves"]
    heads = [k for k in range(1, len(lv)) if lv[k - 1][1] != lv[k][0]]
    assert len(lv) > 64 and lv[63][1] == lv[64][0] and any(k > 64 for k in heads) and not found["truncated"]
    a = check(pkg, slv, ref, [(0, 1)], dist, 0.0, 40)
    assert len(a["link"]) == 2 and np.all(a["flags"] == pkg.SIGHT_FLAGS["certain"]) and np.all(a["depth"] == 40) and a["leaves"].max() > 64
    slv.close()


@pytest.mark.parametrize("P,res", [(12, 8), (2, 16)])
def test_segment_counts_and_resolutions(pkg, scenes, P, res):
    scene = dict(scenes.hard(4, 1500, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    ref = ref_for(pkg, slv, scene, st)
    links = [(0, 2), (3, 1), (1, -1)]
    check(pkg, slv, ref, links)
    assert len(check(pkg, slv, ref, links, 0.3)["link"]) > 0
    slv.close()


def test_per_robot_piece_time(pkg, scenes):
    """a decoupled state with piece_time[u] scaled by 1 + 0.03 * u: the cuts fall at b's own segment boundaries, and a faster b arrives and hovers"""
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    st = slv.get_state()
    st["piece_time"] = st["piece_time"] * (1 + 0.03 * np.arange(slv.U))
    slv.set_state(st)
    ref = ref_for(pkg, slv, scene, st)
    a = check(pkg, slv, ref, None, 0.6)
    assert len(set(a["link"])) > 1 and a["windows"][a["partner"] >= 0].min() > slv.S        # a robot pair has more seeds than segments: b's cuts
    slv.close()


def test_placement_across_a_wave_of_links(pkg, scenes):
    """a fleet of 65 with one link per robot, of which only those of robots 0, 31, 32 and 64 have rows: the scan of the links' row counts crosses one wave"""
    base = scenes.crossing(65, 120)
    cloud = np.array(base["cloud"]) + np.array([0.0, 0.0, 80.0])                            # out of every range
    links = [(u, u + 1) for u in range(63)] + [(63, 62), (64, 63)]                            # (no link (63, 64): it is (64, 63)'s segment)
    who = (0, 31, 32, 64)
    for k, u in enumerate(who):
        at = [base["waypoints"][r][0] + (base["waypoints"][r][-1] - base["waypoints"][r][0]) * 0.1 for r in links[u]]
        cloud[k] = 0.5 * (at[0] + at[1])                                                     # on u's link, a tenth into the flights
    scene = dict(base, cloud=np.ascontiguousarray(cloud))
    slv = pkg.Solver(scene, stop=0.0)
    ref = ref_for(pkg, slv, scene, stations=np.zeros((0, 3)))
    a = check(pkg, slv, ref, links)
    assert sorted(set(a["robot"])) == list(who) and list(a["link"]) == sorted(a["link"])
    slv.close()


def test_triangles_and_degenerate_triangles(pkg, scenes):
    """a mesh; and triangles of three equal vertices, which must behave like the points: the same rows as the cloud's restatement, every field"""
    base = scenes.tiny(mode=1)
    scene = scenes.triangulate(base)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    ref = ref_for(pkg, slv, scene)
    assert len(check(pkg, slv, ref, None, 0.6)["link"]) > 0
    check(pkg, slv, ref)
    slv.close()
    deg = scenes.triangulate(base, degenerate=True)
    slv = pkg.Solver(deg, stop=0.0)
    st = R.port_state(base, 2)
    slv.set_state(st)
    as_tris, as_cloud = ref_for(pkg, slv, deg, st, station_of(base)), ref_for(pkg, slv, base, st)   # (one station: a mean over each point three times rounds differently)
    x = check(pkg, slv, as_tris, None, 0.6)
    y = check(pkg, slv, as_cloud, None, 0.6)
    assert len(x["link"]) > 0 and all(np.array_equal(x[n], y[n]) for n in W.FIELDS)
    slv.close()


def raw_call(slv, fn, handle, links, stations, dist, rec, cap, got):
    lk = np.ascontiguousarray(links, dtype=np.int32).reshape(-1, 2)
    st = np.ascontiguousarray(stations, dtype=np.float64).reshape(-1, 3)
    return fn(handle, lk.ctypes.data_as(_ip), C.c_int(len(lk)), st.ctypes.data_as(_dp), C.c_int(len(st)), C.c_double(dist), C.c_double(-1.0), C.c_int(-1), C.c_int(0),
              rec, C.c_int(cap), C.byref(got))


def test_truncation_capacity_and_link_lists(pkg, scenes):
    """max_windows = 1 and 2 on the cluster: TRUNCATED rows == the restatement's; cap below *n: TJ_ERR_CAPACITY, the exact *n, the first cap rows, the sentinel
    behind them untouched; the count-only call returns the same *n; duplicate and reordered links are answered per index"""
    scene, st, stations, links, dist, ref, rows, _ = W.built(pkg, scenes, prims(), "cluster")
    slv = loaded(pkg, scene, st)
    seen = 0
    for mw in (1, 2):
        a = check(pkg, slv, ref, links, dist, None, None, mw)
        seen += int(np.sum(a["flags"] & pkg.SIGHT_FLAGS["truncated"] != 0))
    assert seen > 0
    many = [(1, 0), (0, 1), (0, 1), (1, 0)]
    full = check(pkg, slv, ref, many, dist)
    n = len(full["link"])
    assert n == 4 and list(full["link"]) == [0, 1, 2, 3] and list(full["robot"]) == [1, 0, 0, 1]
    assert all(full[f][1] == full[f][2] == rows[f][0] for f in W.FIELDS if f != "link")

    def call(rec, cap):
        got = C.c_int(-7)
        return raw_call(slv, slv.lib.tj_sight_windows, slv._ctx, many, stations, dist, rec, cap, got), got.value

    assert call(None, 0) == (0, n)
    rec = (pkg.TjSightRow * n)()
    for k in range(n):
        rec[k].robot, rec[k].closest = -99, 123.5
    assert call(rec, 2) == (-3, n)
    assert (rec[2].robot, rec[2].closest) == (-99, 123.5)                                   # the sentinel behind the first cap rows is untouched
    assert all(getattr(rec[k], f) == full[f][k] for k in range(2) for f in W.FIELDS)
    assert call(rec, n) == (0, n) and all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in W.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n + 3) == (0, n)                            # a smaller call after a larger one, and back
    slv.close()


def test_empty_and_infinite(pkg, scenes):
    """dist = +infinity on a 200-point cloud: one row per link, a's whole flight; an empty cloud and an empty link list: 0 rows"""
    scene = scenes.tiny(mode=1, n_points=200)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(1)
    ref = ref_for(pkg, slv, scene)
    links = [(0, 1), (2, 0), (1, -1)]
    a = check(pkg, slv, ref, links, INF)
    F = pkg.SIGHT_FLAGS
    assert list(a["link"]) == [0, 1, 2] and np.all(a["flags"] & ~F["resolved"] == F["certain"] | F["at_start"] | F["at_end"])
    assert np.all(a["depth"] == 0) and np.all(a["leaves"] == a["windows"])
    pt = slv.get_state()["piece_time"]
    for k, (u, _) in enumerate(links):
        assert a["t_first_lo"][k] == 0.0 and a["t_last_hi"][k] == ((slv.S - 1 + 1.0) / float(slv.res)) * float(pt[u])
    b = slv.sight_windows(links=np.zeros((0, 2), dtype=np.int32), stations=ref.stations, dist=0.3)
    assert set(b) == set(W.FIELDS) and all(len(b[f]) == 0 for f in W.FIELDS)
    cloud = np.zeros((0, 3))
    assert slv.lib.tj_set_cloud(slv._ctx, cloud.ctypes.data_as(_dp), C.c_int(0)) == 0
    for dist in (None, INF):
        b = slv.sight_windows(links=links, stations=ref.stations, dist=dist)
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
    links, stations = [(0, 2), (2, 1), (1, -1)], station_of(scene)
    before = one.sight_windows(links=links, stations=stations, dist=0.4)
    assert len(before["link"]) > 0
    rec = (pkg.TjSightRow * 8)()
    rec[0].robot = -99
    for who, fn, handle in (("context", one.lib.tj_sight_windows, one._ctx), ("group", grp.lib.tj_group_sight_windows, grp._g)):
        for out, cap in ((None, 0), (rec, 8)):
            got = C.c_int(-7)
            rc = raw_call(one, fn, handle, links, stations, INF, out, cap, got)
            assert (rc, got.value, rec[0].robot) == (-3, -7, -99), (who, cap, rc, got.value)
    for s in (one, grp):
        with pytest.raises(pkg.TrajAdmmError) as ei:
            s.sight_windows(links=links, stations=stations, dist=INF)
        assert "-3" in str(ei.value) and "dist" in str(ei.value)
        after = s.sight_windows(links=links, stations=stations, dist=0.4)
        assert all(np.array_equal(after[n], before[n]) for n in W.FIELDS)
    grp.close(); one.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_sight_windows_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    scene = scenes.hard()
    links, stations = [(0, 1), (2, -1)], station_of(scene)
    assert_read_only(pkg, scene, lambda s: s.sight_windows(links, stations, dist=1.0, tol=0.0, max_depth=4),
                     lambda s: (s.sight_windows(links, stations), s.sight_windows(links, stations, dist=0.3, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    """links whose owners alternate between the ranks, a duplicate and two station links"""
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    links, stations = [(0, 1), (3, 0), (1, 2), (2, -1), (0, -1), (3, 0), (2, 1)], station_of(scene)
    x = assert_group_equals(one, grp, lambda s, dist, tol: s.sight_windows(links, stations, dist=dist, tol=tol, max_depth=6), ((None, None), (0.3, None), (0.3, 0.0)))
    n = len(x["link"])
    assert n > 2 and len(set(x["robot"])) > 2
    rec, got = (pkg.TjSightRow * n)(), C.c_int(0)                                          # a cap that ends inside the rows: the exact total, the first rows
    lk, st = np.ascontiguousarray(links, dtype=np.int32), np.ascontiguousarray(stations)
    rc = grp.lib.tj_group_sight_windows(grp._g, lk.ctypes.data_as(_ip), C.c_int(len(lk)), st.ctypes.data_as(_dp), C.c_int(1), C.c_double(0.3), C.c_double(0.0), C.c_int(6), C.c_int(0),
                                        rec, C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in W.FIELDS)
    grp.close(); one.close()


def test_sharded_context_is_refused(pkg, scenes):
    assert_sharded_refuses(pkg, scenes, lambda s: s.sight_windows(links=[(2, 3)], dist=0.3), "tj_group_sight_windows")


def test_bad_arguments(pkg, scenes):
    """the precedence: null, then NaN, then limits, then no state; the outputs stay untouched"""
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjSightRow * 12)(), C.c_int(-7)
        rec[0].robot = -99
        nan = float("nan")
        good = np.array([[0, 1], [2, -1]], dtype=np.int32)
        one_station = np.array([[0.0, 0.0, 5.0]])

        def call(d, t, depth, w, links=good, n_links=None, stations=one_station, n_stations=None, out=rec, cap=12, n=C.byref(got)):
            lk = None if links is None else np.ascontiguousarray(links, dtype=np.int32)
            st = None if stations is None else np.ascontiguousarray(stations, dtype=np.float64)
            rc = lib.tj_sight_windows(ctx, None if lk is None else lk.ctypes.data_as(_ip), C.c_int((0 if lk is None else len(lk)) if n_links is None else n_links),
                                      None if st is None else st.ctypes.data_as(_dp), C.c_int((0 if st is None else len(st)) if n_stations is None else n_stations),
                                      C.c_double(d), C.c_double(t), C.c_int(depth), C.c_int(w), out, C.c_int(cap), n)
            if rc == -1:
                assert (got.value, rec[0].robot) == (-7, -99)                                  # the outputs are untouched
            return rc, lib.tj_last_error(ctx)

        rc, msg = call(0.0, -1.0, -1, 0)                                                       # before tj_init_state
        assert rc == -1 and b"tj_init_state" in msg
        rc, msg = call(nan, -1.0, 41, 0)                                                       # NaN before the limits, the limits before the missing state
        assert rc == -1 and b"NaN" in msg
        rc, msg = call(0.0, -1.0, 41, 0, stations=[[0.0, nan, 0.0]])
        assert rc == -1 and b"NaN" in msg and b"station" in msg
        rc, msg = call(0.0, -1.0, 41, 0)
        assert rc == -1 and b"max_depth" in msg
        rc, msg = call(0.0, -1.0, -1, 0, links=[[0, 0]])                                       # a bad link before the missing state
        assert rc == -1 and b"link 0" in msg
        assert call(nan, -1.0, -1, 0, n=None)[0] == -1 and call(0.0, -1.0, -1, 0, cap=-1)[0] == -1 and call(0.0, -1.0, -1, 0, out=None)[0] == -1
        assert call(0.0, -1.0, -1, 0, n_links=-1)[0] == -1 and call(0.0, -1.0, -1, 0, links=None, n_links=2)[0] == -1 and call(0.0, -1.0, -1, 0, stations=None, n_stations=1)[0] == -1
        init()
        assert call(nan, -1.0, -1, 0)[0] == -1 and call(0.0, nan, -1, 0)[0] == -1 and call(0.0, -1.0, 41, 0)[0] == -1 and call(0.0, -1.0, -1, pkg.SIGHT_MAX_WINDOWS + 1)[0] == -1
        for bad in ([[3, 0]], [[-1, 0]], [[1, 1]], [[0, 3]], [[0, -2]], [[0, 1], [2, -1], [0, -3]]):
            assert call(0.0, -1.0, -1, 0, links=bad)[0] == -1, bad
        assert call(0.0, -1.0, -1, 0, links=[[0, -1]], stations=None)[0] == -1                 # no station at all
        rc, msg = call(0.0, -1.0, -1, pkg.SIGHT_MAX_WINDOWS, cap=1 << 25)                      # refused up front, nothing allocated
        assert rc == -1 and b"TJ_SIGHT_MAX_BYTES" in msg
        for args in ((0.0, -1.0, 40, pkg.SIGHT_MAX_WINDOWS), (0.05, 0.0, -1, 0), (INF, -1.0, 0, 1)):   # the limits themselves are valid; no obstacle set at all: 0 rows
            got.value = -7
            assert call(*args)[0] == 0 and got.value == 0 and rec[0].robot == -99


def test_command_line(pkg, scenes, tmp_path):
    """--sight-windows 0.6 --sight-station X Y Z (one context and a two-rank group): the printed rows are the library's on the dumped state for every directed
    pair and every robot's station link, in its order -- doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip),
    integers exactly -- and the fleet's line counts links and rows"""
    cli = CliCase(pkg, scenes, tmp_path)
    station = station_of(cli.scene)
    doubles = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "closest", "closest_time")
    ints = ("link", "robot", "partner", "index", "leaves", "depth", "windows", "flags")
    for extra, lines in cli.queried(["--sight-windows", "0.6", "--sight-station"] + ["%.17g" % v for v in station[0]], "sight "):
        got = [l.split() for l in lines if l.startswith("sight link ")]
        a = cli.slv.sight_windows(stations=station, dist=0.6)
        assert len(got) == len(a["link"]) > 0 and all(len(w) == 29 for w in got)
        for k, w in enumerate(got):
            for n, i in zip(doubles, (8, 9, 11, 12, 14, 16, 18)):
                assert close_to_six_digits(w[i], a[n][k]), (extra, k, n, w)
            assert [int(w[i]) for i in (2, 4, 6, 20, 22, 24, 26, 28)] == [a[n][k] for n in ints], (extra, k, w)
        fleet = [l.split() for l in lines if l.startswith("sight fleet ")]
        assert len(fleet) == 1 and int(fleet[0][2]) == 9 and int(fleet[0][4]) == len(a["link"])
    cli.close()
