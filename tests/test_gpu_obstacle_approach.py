"""GPU (-m gpu): tj_obstacle_approach -- the flown curve's closest approach to the obstacle primitives, converged by branch and bound.

Expected values come from tests/obstacle_approach_ref.py: the Python restatement of the header's definition (audit_ref's hulls, audit_timed_ref's blossoming, the
oracle's GJK, brute force over all primitives with the walk's box predicate, the level-synchronous search written out).  Every field of every record is
compared with == on doubles and ints, `windows` and `depth` included.  The restatement itself is held against the flown curve on the CPU
(tests/test_obstacle_approach_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_ref as R
import obstacle_approach_ref as O
from audit_ref import prims
from conftest import ROOT
from query_kit import CliCase, assert_group_equals, assert_read_only, close_to_six_digits, group_pair, one_queue, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")


def ref_for(pkg, slv, scene, st=None):
    return O.Ref(pkg, prims(), slv.get_state() if st is None else st, slv.P, slv.res, O.prims_of(scene))


def check(pkg, slv, ref, rng=None, tol=None, max_depth=None, max_windows=None, owned=None):
    """device records == the restatement `ref` (built on the state the solver holds); returns the device's answer"""
    p = slv.params
    a = slv.obstacle_approach(range=rng, tol=tol, max_depth=max_depth, max_windows=max_windows)
    rec = ref.records(p["offset"] + 2 * p["margin"] if rng is None else rng, p["offset"], pkg.OBSTACLE_TOL if tol is None else tol,
                      O.MAX_DEPTH if max_depth is None else max_depth, pkg.OBSTACLE_FRONTIER if max_windows is None else max_windows, owned=owned)
    assert set(a) == set(O.FIELDS)
    for n in O.FIELDS:
        assert np.array_equal(a[n], rec[n]), (rng, tol, max_depth, max_windows, n, a[n], rec[n])
    return a


def test_record_size_and_defaults(pkg):
    lib = pkg.load_library()
    assert lib.tj_obstacle_record_size() == C.sizeof(pkg.TjObstacleRobot) == 48
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert float(re.search(r"#define TJ_OBSTACLE_TOL\s+(\S+)", hdr).group(1)) == pkg.OBSTACLE_TOL
    assert int(re.search(r"#define TJ_OBSTACLE_FRONTIER\s+(\d+)", hdr).group(1)) == pkg.OBSTACLE_FRONTIER
    assert pkg.OBSTACLE_FLAGS == dict(contact=1, clear=2, converged=4, truncated=8)


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """initial state and after a few iterations; range in {default, 1.0, inf}, tol in {default, 1e-3, 0}, max_depth in {default, 0, 3}"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 3 if name == "hard" else 4):
        if it:
            slv.iterate(it)
        ref = ref_for(pkg, slv, scene)
        for rng in ((None, 1.0, INF) if it or name != "hard" else (None, 1.0)):   # (hard() at range inf is 160 000 seeds per robot for the restatement: once)
            for tol in (None, 1e-3, 0.0):
                check(pkg, slv, ref, rng, tol)
            for depth in (0, 3):
                check(pkg, slv, ref, rng, None, depth)
        check(pkg, slv, ref, 1.0, 0.0, 3)
    slv.close()


def test_triangles_and_degenerate_triangles(pkg, scenes):
    """a mesh; and triangles of three equal vertices, which must behave like the points: the same records as the cloud's restatement"""
    base = scenes.tiny(mode=1)
    scene = scenes.triangulate(base)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    ref = ref_for(pkg, slv, scene)
    for rng in (None, 1.0, INF):
        check(pkg, slv, ref, rng)
    check(pkg, slv, ref, 1.0, 0.0)
    check(pkg, slv, ref, None, None, 0)
    slv.close()
    deg = scenes.triangulate(base, degenerate=True)
    slv = pkg.Solver(deg, stop=0.0)
    st = R.port_state(base, 3)
    slv.set_state(st)
    as_tris, as_cloud = ref_for(pkg, slv, deg, st), ref_for(pkg, slv, base, st)
    for rng in (None, 1.0):
        check(pkg, slv, as_tris, rng)
        check(pkg, slv, as_cloud, rng)
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
    check(pkg, slv, ref, 1.0, 0.0)
    slv.close()


def test_fleet_of_65(pkg, scenes):
    scene = scenes.crossing(65, 500)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    ref = ref_for(pkg, slv, scene)
    check(pkg, slv, ref)
    check(pkg, slv, ref, 1.0)
    slv.close()


def test_truncation(pkg, scenes):
    """max_windows in {1, 2} on hard() after 4 iterations: == the restatement under the same cap, the TRUNCATED bit included; lo <= truth + slack"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(4)
    st = slv.get_state()
    ref = ref_for(pkg, slv, scene, st)
    X = O.prims_of(scene)
    sl = O.slack(slv.S, st, X)
    tv = O.truth(pkg, st, slv.P, slv.res, X)
    seen = 0
    for mw in (1, 2):
        a = check(pkg, slv, ref, 1.0, None, None, mw)
        seen += int(np.sum(a["flags"] & pkg.OBSTACLE_FLAGS["truncated"] != 0))
        for u in range(slv.U):
            assert a["lo"][u] <= tv[u][0] + sl, (mw, u, a["lo"][u], tv[u])
    assert seen > 0
    slv.close()


def test_depth_zero_against_audit(pkg, scenes):
    """max_depth = 0 against Solver.audit() at the same range: lo <= obs_clearance, == min(hi, obs_clearance) where no live seed lost its certificate (lo > 0);
    converged, hi >= obs_clearance - slack (the curve lies in its hulls)"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(4)
    st = slv.get_state()
    sl = O.slack(slv.S, st, O.prims_of(scene))
    for rng in (None, 1.0):
        a0, au, full = slv.obstacle_approach(range=rng, max_depth=0), slv.audit(range=rng), slv.obstacle_approach(range=rng)
        assert np.all(a0["depth"] == 0) and np.all(a0["lo"] <= au["obs_clearance"])
        m = a0["lo"] > 0.0
        assert np.array_equal(a0["lo"][m], np.minimum(a0["hi"], au["obs_clearance"])[m])
        assert np.all(full["flags"] & pkg.OBSTACLE_FLAGS["converged"]) and np.all(full["hi"] >= au["obs_clearance"] - sl)
    slv.close()


def test_constructed_states(pkg, scenes):
    """corner: tj_audit says OBS_CONTACT, the curve is clear; pierce: contact, lo == 0, the crossing time; miss: the known distance"""
    F, tol = pkg.OBSTACLE_FLAGS, pkg.OBSTACLE_TOL
    scene, st, k, tv = O.corner_state(pkg, scenes, prims())
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    sl = O.slack(slv.S, st, O.prims_of(scene))
    ref = ref_for(pkg, slv, scene, st)
    assert slv.audit()["flags"][0] & pkg.AUDIT_FLAGS["obs_contact"] and slv.audit()["obs_index"][0] == k
    for rng in (None, INF):
        a = check(pkg, slv, ref, rng)
        assert a["flags"][0] == F["clear"] | F["converged"] and a["index"][0] == k
        assert abs(a["hi"][0] - tv[0]) <= tol + sl and a["hi"][0] > slv.params["offset"]
    slv.close()
    scene, st, k, t_cross = O.pierce_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    ref = ref_for(pkg, slv, scene, st)
    for rng in (None, INF):
        a = check(pkg, slv, ref, rng)
        assert a["flags"][0] & F["contact"] and not a["flags"][0] & F["clear"] and a["index"][0] == k
        assert a["lo"][0] == 0.0 and a["hi"][0] <= 1e-5 and abs(a["time"][0] - t_cross) <= 1e-5
    slv.close()
    scene, st, k, d = O.miss_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    sl = O.slack(slv.S, st, O.prims_of(scene))
    ref = ref_for(pkg, slv, scene, st)
    for rng in (None, INF):
        a = check(pkg, slv, ref, rng)
        assert a["flags"][0] == F["clear"] | F["converged"] and a["index"][0] == k and abs(a["hi"][0] - d) <= tol + sl
    a = check(pkg, slv, ref, 0.2)
    assert {n: a[n][0] for n in O.FIELDS} == O.sentinel(0.2)
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_obstacle_approach_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    assert_read_only(pkg, scenes.hard(), lambda s: s.obstacle_approach(range=1.0, tol=0.0),
                     lambda s: (s.obstacle_approach(), s.obstacle_approach(range=1.0, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    assert_group_equals(one, grp, lambda s, rng, tol: s.obstacle_approach(range=rng, tol=tol), ((None, None), (1.0, 0.0)))
    grp.close(); one.close()


def test_sharded_context_answers_for_its_own_robots(pkg, scenes):
    scene = scenes.hard()
    one = pkg.Solver(scene, stop=0.0)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)
    x, y = one.obstacle_approach(range=1.0), half.obstacle_approach(range=1.0)
    mine = y["windows"] != 0                                                  # (every robot of hard() has thousands of seeds within 1.0)
    assert 0 < mine.sum() < scene["U"]
    for k in x:
        assert np.array_equal(x[k][mine], y[k][mine]), k
        assert np.all(y[k][~mine] == 0), k
    check(pkg, half, ref_for(pkg, one, scene), 1.0, owned=[int(u) for u in np.flatnonzero(mine)])
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec = (pkg.TjObstacleRobot * 3)()
        call = lambda r, t, d, w, out=rec: lib.tj_obstacle_approach(ctx, C.c_double(r), C.c_double(t), C.c_int(d), C.c_int(w), out)
        assert call(0.0, -1.0, -1, 0) == -1                                   # before tj_init_state
        init()
        nan = float("nan")
        assert call(nan, -1.0, -1, 0) == -1 and call(0.0, nan, -1, 0) == -1 and call(0.0, -1.0, 41, 0) == -1 and call(0.0, -1.0, -1, pkg.OBSTACLE_FRONTIER + 1) == -1
        assert call(0.0, -1.0, -1, 0, None) == -1
        # the limits themselves are valid; no obstacle set at all: the sentinel for every robot
        F = pkg.OBSTACLE_FLAGS
        for args, r in (((0.0, -1.0, 40, pkg.OBSTACLE_FRONTIER), 0.1 + 2 * 0.1), ((0.05, 0.0, -1, 0), 0.05), ((INF, -1.0, 0, 1), INF)):
            assert call(*args) == 0
            for u in range(3):
                got = {n: getattr(rec[u], n) for n in O.FIELDS}
                assert got == O.sentinel(r) and got["flags"] == F["clear"] | F["converged"], (args, u, got)
        cloud = np.zeros((0, 3))
        assert lib.tj_set_cloud(ctx, cloud.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(0)) == 0       # tj_set_cloud with n = 0: the same
        assert call(0.0, -1.0, -1, 0) == 0 and {n: getattr(rec[1], n) for n in O.FIELDS} == O.sentinel(0.1 + 2 * 0.1)


def test_command_line(pkg, scenes, tmp_path):
    """--obstacle-approach and --obstacle-approach 1e-6 (one context and a two-rank group): every printed field equals the library's answer on the dumped state --
    doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly; the summary line names the smallest hi;
    all other output is unchanged"""
    cli = CliCase(pkg, scenes, tmp_path)
    U = cli.scene["U"]
    names = ("lo", "hi", "index", "segment", "time", "depth", "windows", "flags")
    plain = cli.run(["--closest-approach"])
    for args, tol in ((["--obstacle-approach"], None), (["--obstacle-approach", "1e-6"], 1e-6)):
        for extra, lines in cli.queried(["--closest-approach"] + args, "obstacle ", against=plain):
            at = [i for i, l in enumerate(lines) if l.startswith("closest ") or l.startswith("obstacle ")]
            assert [lines[i].split()[0] for i in at] == ["closest"] * (U + 1) + ["obstacle"] * (U + 1)      # after the `closest` lines
            got = [l.split() for l in lines if l.startswith("obstacle uav ")]
            assert len(got) == U and all(len(w) == 19 and int(w[2]) == u for u, w in enumerate(got))
            a = cli.slv.obstacle_approach(tol=tol)
            for u, w in enumerate(got):
                for k, n in enumerate(names):
                    if n in ("lo", "hi", "time"):
                        assert close_to_six_digits(w[4 + 2 * k], a[n][u]), (args, extra, u, n, w)
                    else:
                        assert int(w[4 + 2 * k]) == a[n][u], (args, extra, u, n, w)
            fleet = [l.split() for l in lines if l.startswith("obstacle fleet ")]
            assert len(fleet) == 1
            m = a["index"] >= 0
            if m.any():
                who = int(np.flatnonzero(m)[np.argmin(a["hi"][m])])
                f = fleet[0]
                assert close_to_six_digits(f[3], a["hi"][who]) and int(f[5]) == who and int(f[7]) == a["index"][who]
                assert int(f[11]) == int(np.any(a["flags"] & pkg.OBSTACLE_FLAGS["contact"]))
            else:
                assert fleet[0][2] == "none"
    cli.close()
