"""GPU (-m gpu): tj_flight_profile -- position, dynamics, the NEAREST obstacle primitive (no range) and the nearest other robot at sampled flight times.

Expected values come from tests/flight_profile_ref.py: the Python restatement of the header's definition with BRUTE FORCE over every primitive and every
robot (no tree).  Every field of every record is compared with == on doubles and ints, on the state the solver holds.  The restatement itself is held
against the flown curve on the CPU (tests/test_flight_profile_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import flight_profile_ref as F
from audit_ref import prims
from conftest import ROOT
from query_kit import CliCase, assert_group_equals, assert_read_only, assert_sharded_refuses, group_pair, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")


def check(pkg, slv, scene, times, st=None):
    """device records == the restatement on the state the solver holds; returns the device's answer"""
    st = slv.get_state() if st is None else st
    a = slv.flight_profile(times=times)
    ref = F.profile(pkg, prims(), st, slv.P, slv.res, F.prims_of(scene), times, slv.params, multi=slv.mode >= 1)
    assert set(a) == set(F.FIELDS)
    for n in F.FIELDS:
        assert a[n].shape == ref[n].shape == (slv.U, len(times))
        bad = np.argwhere(a[n] != ref[n])
        assert len(bad) == 0, (n, bad[:5], a[n][tuple(bad[0])], ref[n][tuple(bad[0])])
    return a


def test_record_size_and_constants(pkg):
    """sizeof(tj_profile_sample): eight doubles and four ints, 80 bytes on every LP64 ABI -- the C side and the ctypes mirror agree; the header's constants are
    the package's"""
    lib = pkg.load_library()
    assert lib.tj_flight_profile_record_size() == C.sizeof(pkg.TjProfileSample) == 8 * 8 + 4 * 4
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    flags = {k.lower(): int(v) for k, v in re.findall(r"#define TJ_PROFILE_(HOVER|OBS_CONTACT|PAIR_CONTACT|SPEED|ACCEL)\s+(\d+)", hdr)}
    assert flags == pkg.PROFILE_FLAGS == dict(hover=1, obs_contact=2, pair_contact=4, speed=8, accel=16)
    assert int(re.search(r"#define TJ_PROFILE_MAX_SAMPLES\s+(\d+)", hdr).group(1)) == pkg.PROFILE_MAX_SAMPLES == 65536
    assert re.search(r"#define TJ_PROFILE_MAX_RECORDS\s+\(1 << 24\)", hdr) and pkg.PROFILE_MAX_RECORDS == 1 << 24


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """initial state and after 3 iterations; K in {1, 7, 9, 65}; the times include 0, the segment boundaries of robot 0 (all of them at K = 65), the longest
    duration and 1.5 times it, where every robot hovers"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 3):
        if it:
            slv.iterate(it)
        st = slv.get_state()
        for K in (1, 7, 9, 65):
            times = F.sample_times(st, slv.P, slv.res, K)
            a = check(pkg, slv, scene, times, st)
            if K >= 3:
                k = int(np.flatnonzero(times == 1.5 * F.durations(st, slv.P).max())[0])
                assert np.all(a["flags"][:, k] & pkg.PROFILE_FLAGS["hover"]) and np.all(a["segment"][:, k] == slv.S) and np.all(a["speed"][:, k] == 0.0)
        if name == "tiny_single":
            assert np.all(a["robot"] == -1) and np.all(a["robot_distance"] == INF)
    slv.close()


def test_default_grid(pkg, scenes):
    """times=None: the grid over the longest duration, 101 samples or `samples`"""
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    st = slv.get_state()
    a = slv.flight_profile()
    assert a["time"].shape == (slv.U, 101) and np.array_equal(a["time"][0], F.grid(st, slv.P, 101))
    b = slv.flight_profile(samples=5)
    assert np.array_equal(b["time"][1], F.grid(st, slv.P, 5)) and np.array_equal(slv.flight_profile(samples=1)["time"], np.zeros((slv.U, 1)))
    slv.close()


def test_per_robot_piece_time(pkg, scenes):
    """robots with their own piece_time: some hover while others still fly at the same t"""
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    st = R.scaled_time_state(R.scaled_time_state(R.port_state(scene, 3), 0, 0.37), 2, 3.3)
    slv.set_state(st)
    times = np.concatenate([F.sample_times(st, slv.P, slv.res, 65), [slv.P * 0.37, slv.P * 0.37 * 1.01, 2.0]])
    a = check(pkg, slv, scene, times, st)
    hov = (a["flags"] & pkg.PROFILE_FLAGS["hover"]) != 0
    assert np.any(hov[0] & ~hov[2]) and np.any(~hov[0])
    slv.close()


def test_triangles_and_degenerate_triangles(pkg, scenes):
    """a mesh; and triangles of three equal vertices, which must behave like the points: the cloud's restatement"""
    base = scenes.tiny(mode=1)
    scene = scenes.triangulate(base)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    st = slv.get_state()
    check(pkg, slv, scene, F.sample_times(st, slv.P, slv.res, 9), st)
    slv.close()
    deg = scenes.triangulate(base, degenerate=True)
    slv = pkg.Solver(deg, stop=0.0)
    st = R.port_state(base, 3)
    slv.set_state(st)
    times = F.sample_times(st, slv.P, slv.res, 9)
    check(pkg, slv, deg, times, st)
    check(pkg, slv, base, times, st)
    slv.close()


@pytest.mark.parametrize("n", [0, 1, 8, 9, 64, 65, 600, 4097])
def test_pyramid_depths(pkg, scenes, n):
    """obstacle sets of one leaf, one more than a leaf, one top level, one more than it, and 4 097: one node above a full 8^4"""
    scene = dict(scenes.tiny(mode=1, n_points=max(n, 600)))
    scene["cloud"] = np.ascontiguousarray(scene["cloud"][:n])
    slv = pkg.Solver(scene, stop=0.0)
    st = slv.get_state()
    a = check(pkg, slv, scene, F.sample_times(st, slv.P, slv.res, 9), st)
    if n == 0:
        assert np.all(a["obs_index"] == -1) and np.all(a["obs_distance"] == INF)
    slv.close()


def test_nothing_near(pkg, scenes):
    """the cloud 1e3 away: the nearest primitive is still found exactly, where tj_obstacle_approach at its default range reports -1"""
    scene = dict(scenes.tiny(mode=1))
    scene["cloud"] = np.ascontiguousarray(scene["cloud"] + np.array([1e3, 0.0, 0.0]))
    slv = pkg.Solver(scene, stop=0.0)
    st = slv.get_state()
    a = check(pkg, slv, scene, F.sample_times(st, slv.P, slv.res, 9), st)
    assert np.all(a["obs_index"] >= 0) and np.all(a["obs_distance"] > 900.0)
    assert np.all(slv.obstacle_approach()["index"] == -1)
    slv.close()


def exact_last_point(st, u):
    """the state with robot u's last control point on a grid of 2^-10 (hull_entry's sum returns it as it is: asserted by twin_cloud through the distances)"""
    st = {k: v.copy() for k, v in st.items()}
    st["spline"][u][:, -1] = np.round(st["spline"][u][:, -1] * 1024.0) / 1024.0
    return st


def test_bound_under_equal_distances(pkg, scenes):
    """4 096 points on a sphere of radius 2 around a hovering robot: no bound separates them, nothing overflows, and the answer is brute force's"""
    scene = dict(scenes.tiny(mode=1))
    st = R.port_state(scene, 0)
    H = R.hulls_of(pkg, st["spline"], scene["P"], 8)
    scene["cloud"] = F.sphere_cloud(H[1, -1, 5])
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    longest = float(F.durations(st, slv.P).max())
    a = check(pkg, slv, scene, np.array([1.25 * longest, 0.0, 0.5 * longest]), st)
    assert a["flags"][1, 0] & pkg.PROFILE_FLAGS["hover"] and abs(a["obs_distance"][1, 0] - 2.0) < 1e-12
    slv.close()


@pytest.mark.parametrize("i,j", [(40, 555), (555, 40)])
def test_exact_ties_of_primitives(pkg, scenes, i, j):
    """twin points at last_cp +- (0.5, 0, 0), exact in binary: bit-equal distances, the smaller caller index wins in both index orders"""
    scene = dict(scenes.tiny(mode=1))
    st = exact_last_point(R.port_state(scene, 0), 0)
    H = R.hulls_of(pkg, st["spline"], scene["P"], 8)
    assert np.array_equal(H[0, -1, 5], st["spline"][0][:, -1])
    scene["cloud"] = F.twin_cloud(scene["cloud"] + np.array([0.0, 0.0, 30.0]), H[0, -1, 5], i, j)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    longest = float(F.durations(st, slv.P).max())
    a = check(pkg, slv, scene, np.array([2.0 * longest, longest]), st)
    assert np.all(a["obs_index"][0] == min(i, j)) and np.all(a["obs_distance"][0] == 0.5)
    slv.close()


def test_exact_ties_of_robots(pkg, scenes):
    """three equally spaced collinear hovering robots: the middle one's partner is the smaller index"""
    lines = [((0, 0, 0), (8, 0, 0), 1.0), ((0, 2, 0), (8, 2, 0), 1.0), ((0, 4, 0), (8, 4, 0), 1.0)]
    scene, st = T.straight_state(pkg, scenes, lines)
    for u in range(3):   # the arrival points exactly (8, 2 u, 0)
        st["spline"][u][:, -1] = (8.0, 2.0 * u, 0.0)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    a = check(pkg, slv, scene, np.array([10.0, 0.5, 4.0]), st)
    assert a["robot"][1, 0] == 0 and a["robot_distance"][1, 0] == 2.0 and a["robot"][0, 0] == 1 and a["robot"][2, 0] == 1
    slv.close()


def test_partner_scan_wider_than_a_wave(pkg, scenes):
    scene = scenes.crossing(65, 512)
    slv = pkg.Solver(scene, stop=0.0)
    st = slv.get_state()
    check(pkg, slv, scene, F.sample_times(st, slv.P, slv.res, 9), st)
    slv.close()


def test_flight_profile_is_read_only(pkg, scenes):
    """state, tj_get_stats and tj_launch_count are unchanged by calls; 3 iterations after them give the bits of 3 iterations without them"""
    assert_read_only(pkg, scenes.hard(), lambda s: s.flight_profile(samples=9),
                     lambda s: (s.flight_profile(), s.flight_profile(samples=7), s.flight_profile(times=[0.0, 3.0])))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)

    def ask(s, how):   # 65 times chosen on the state the one context holds now, or the default grid of 9
        return s.flight_profile(samples=9) if how == "grid" else s.flight_profile(times=F.sample_times(one.get_state(), one.P, one.res, 65))

    assert_group_equals(one, grp, ask, (("times",), ("grid",)))
    grp.close(); one.close()


def test_sharded_context_is_unsupported_and_single_uav_has_no_partner(pkg, scenes):
    assert_sharded_refuses(pkg, scenes, lambda half: half.flight_profile(samples=3), "tj_group_flight_profile")
    scene = scenes.tiny(mode=0)
    slv = pkg.Solver(scene, stop=0.0)
    a = check(pkg, slv, scene, np.array([0.0, 1.0, 1e4]))
    assert np.all(a["robot"] == -1) and np.all(a["robot_distance"] == INF)
    slv.close()


def test_bad_arguments(pkg, scenes):
    """every invalid argument returns TJ_ERR_INVALID and leaves `out` untouched"""
    dp = C.POINTER(C.c_double)
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec = (pkg.TjProfileSample * (3 * 4))()
        C.memset(rec, 0xAB, C.sizeof(rec))
        mark = bytes(rec)

        def call(times, n=None, out=rec):
            t = None if times is None else np.ascontiguousarray(times, dtype=np.float64)
            return lib.tj_flight_profile(ctx, None if t is None else t.ctypes.data_as(dp), C.c_int(len(times) if n is None else n), out)

        assert call([0.0, 1.0]) == -1 and bytes(rec) == mark                                  # before tj_init_state
        init()
        nan = float("nan")
        for bad in ([nan], [0.0, nan], [-1e-300], [1.0, -2.0], [INF], [0.0, -INF]):
            assert call(bad) == -1, bad
        assert call(None, 2) == -1 and call([0.0], 1, None) == -1 and call([0.0], 0) == -1 and call([0.0], -3) == -1
        big = np.zeros(pkg.PROFILE_MAX_SAMPLES + 1)
        assert call(big) == -1
        assert bytes(rec) == mark
        assert call([0.0, 1.0, 2.0, 1e300]) == 0 and bytes(rec) != mark                       # valid: no obstacle set at all, +infinity and -1
        assert all(rec[i].obs_index == -1 and rec[i].obs_distance == INF for i in range(12))
    # uav_num * n_times above the limit, n_times itself within it
    tp2 = pkg.TjParams()
    lib.tj_default_params(C.byref(tp2), 1, 257, 2)
    ctx2 = C.c_void_p()
    assert lib.tj_create(C.byref(tp2), C.byref(ctx2)) == 0
    t = np.zeros(pkg.PROFILE_MAX_SAMPLES)
    one = (pkg.TjProfileSample * 1)()
    assert 257 * t.size > pkg.PROFILE_MAX_RECORDS and lib.tj_flight_profile(ctx2, t.ctypes.data_as(dp), C.c_int(t.size), one) == -1
    lib.tj_destroy(ctx2)


def test_against_the_other_kernels(pkg, scenes):
    """hard() after 3 iterations, a 257-sample grid: the smallest sampled obstacle distance is not below tj_obstacle_approach's lo (up to its stated 1e-10
    relative), the smallest sampled robot distance while the robot flies is not below tj_closest_approach's lo (whose bracket covers the robot's own flight).
    Both are sound: no tolerance."""
    slv = pkg.Solver(scenes.hard(), stop=0.0)
    slv.iterate(3)
    a = slv.flight_profile(samples=257)
    oa, cl = slv.obstacle_approach(tol=0.0), slv.closest_approach(tol=0.0)
    for u in range(slv.U):
        assert a["obs_distance"][u].min() >= oa["lo"][u] * (1 - 1e-10), u
        assert a["robot_distance"][u][a["segment"][u] < slv.S].min() >= cl["lo"][u], u
    slv.close()


def test_command_line(pkg, scenes, tmp_path):
    """--flight-profile 5 (one context and a two-rank group; to standard output and to a file): 5 lines per robot whose numbers are
    Solver.flight_profile(samples=5)'s on the dumped state -- times, positions, robot distances and dynamics to 1e-12, obstacle distances to 1e-6 (the CLI
    read the scene through the x0.2 / x5 file round trip), integers exactly; all other output is unchanged"""
    cli = CliCase(pkg, scenes, tmp_path)
    U = cli.scene["U"]
    plain = cli.run(["--obstacle-approach"])
    flags = ["--obstacle-approach", "--flight-profile", "5"]

    def runs():   # one context and a two-rank group to standard output, then one context to a file
        for extra, lines in cli.queried(flags, "profile ", against=plain):
            yield extra, lines, False
        yield next(cli.queried(flags + ["prof.txt"], "profile ", against=plain)) + (True,)

    for extra, lines, to_file in runs():
        if to_file:
            assert not [l for l in lines if l.startswith("profile ")]
            got = [l.split() for l in open(tmp_path / "prof.txt").read().split("\n") if l]
        else:
            at = [i for i, l in enumerate(lines) if l.startswith("obstacle ") or l.startswith("profile ")]
            assert [lines[i].split()[0] for i in at] == ["obstacle"] * (U + 1) + ["profile"] * (5 * U)      # after the query lines
            got = [l.split()[1:] for l in lines if l.startswith("profile ")]
        assert len(got) == 5 * U and all(len(w) == 12 for w in got)
        a = cli.slv.flight_profile(samples=5)
        names = ("time", "x", "y", "z", "obs_distance", "obs_index", "robot_distance", "robot", "speed", "accel", "flags")
        for r, w in enumerate(got):
            u, k = divmod(r, 5)
            assert int(w[0]) == u
            for n, s in zip(names, w[1:]):
                v = a[n][u, k]
                if n in F.INTS:
                    assert int(s) == v, (extra, u, k, n, w)
                else:
                    assert abs(float(s) - v) <= (1e-6 if n == "obs_distance" else 1e-12) * max(1.0, abs(v)), (extra, u, k, n, w)
    cli.close()
