"""CPU (-m "not gpu"): the restatement tests/test_gpu_obstacle_approach.py holds the device to (tests/obstacle_approach_ref.py) is itself held to the flown
curve: the bracket contains a truth that uses neither GJK nor subdivision, the box prefilter changes nothing, brackets nest with depth, tol = 0 runs until
nothing is left, depth 0 is tj_audit's hull clearance wherever that carries its certificate, and the three constructed single-UAV states give what they
were built for -- the corner is the case the call exists for: tj_audit says contact, the curve is clear.  Bars: slack = K(S) * eps * max|coordinate|
(counted in tests/audit_timed_ref.py) and the tolerance asked for -- nothing here is fitted to what the code returns.

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h): largest hi - lo per depth 0..19 over the four end-to-end end
states = 1.35e-2, 8.51e-3, 4.92e-3, 9.91e-4, 5.96e-4, 1.90e-4, 3.33e-5, 1.20e-5, 2.65e-6, 1.96e-7, 1.96e-7, 2.14e-8, 6.27e-9, 2.35e-9, 5.59e-10, 1.40e-10,
4.77e-11, 8.14e-12, 3.71e-13, 0 -> floor 3.71e-13 at depth 18 -> TJ_OBSTACLE_TOL = 1e-11; largest live set 9 -> TJ_OBSTACLE_FRONTIER = 4096."""
import functools
import os
import re

import numpy as np
import pytest

import audit_ref as R
import obstacle_approach_ref as O
from conftest import ROOT
from query_kit import pkg_module as _pkg

OFFSET = 0.1
INF = float("inf")
STATES = ["tiny0", "tiny1", "hard0", "hard3", "tiny_tri"]


@functools.lru_cache(maxsize=None)
def state_of(name):
    """(scene, state, P, res)"""
    pkg = _pkg()
    sc = pkg.scenes
    if name == "tiny0":
        scene, it = sc.tiny(mode=0), 3
    elif name == "tiny1":
        scene, it = sc.tiny(mode=1), 3
    elif name == "tiny_tri":
        scene, it = sc.triangulate(sc.tiny(mode=1)), 3
    else:
        scene, it = sc.hard(), int(name[4:])
    st = R.port_state(scene, it)
    assert R.valid_state(st, scene["U"])
    return scene, st, scene["P"], 8


@functools.lru_cache(maxsize=None)
def ref_of(name):
    scene, st, P, res = state_of(name)
    return O.Ref(_pkg(), R.prims(), st, P, res, O.prims_of(scene))


@functools.lru_cache(maxsize=None)
def truth_of(name):
    scene, st, P, res = state_of(name)
    return O.truth(_pkg(), st, P, res, O.prims_of(scene))


@pytest.mark.parametrize("name", STATES)
def test_bracket_holds_the_truth(pkg, name):
    """lo - slack <= truth <= hi + slack for every robot, everything in range, at the default tolerance and at 1e-3"""
    scene, st, P, res = state_of(name)
    sl = O.slack(P * res, st, O.prims_of(scene))
    tv = truth_of(name)
    for tol in (pkg.OBSTACLE_TOL, 1e-3):
        rec = ref_of(name).records(INF, OFFSET, tol, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER)
        for u in range(scene["U"]):
            print(name, tol, u, {n: rec[n][u] for n in O.FIELDS}, "truth", tv[u], "slack", sl)
        for u in range(scene["U"]):
            assert rec["index"][u] >= 0 and 0 <= rec["segment"][u] < P * res and not rec["flags"][u] & O.TRUNCATED
            assert rec["lo"][u] - sl <= tv[u][0] <= rec["hi"][u] + sl, (u, rec["lo"][u], tv[u], rec["hi"][u])
            assert rec["flags"][u] & O.CONVERGED and rec["hi"][u] - rec["lo"][u] <= tol


@pytest.mark.parametrize("name", ["tiny1", "hard3", "tiny_tri"])
def test_prefilter_changes_nothing(pkg, name):
    """the walk's box predicate against no filter at all: every field but the count of evaluated items is the same"""
    ref = ref_of(name)
    for rng in (0.3, 1.0):
        a = ref.records(rng, OFFSET, pkg.OBSTACLE_TOL, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER)
        b = ref.records(rng, OFFSET, pkg.OBSTACLE_TOL, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER, prefilter=False)
        for n in O.FIELDS:
            if n != "windows":
                assert np.array_equal(a[n], b[n]), (rng, n, a[n], b[n])
        assert np.all(a["windows"] <= b["windows"])


@pytest.mark.parametrize("name", STATES)
def test_brackets_nest_and_tol_zero_runs_out(pkg, name):
    """hi never rises from round to round, and lo never falls by more than the GJK's own stop rule allows: it ends at |v|^2 - v . w <= 1e-10 |v|^2
    (dev_gjk.h / orc_gjk.cpp eps_rel2), so a parent's |v| may stand up to 1e-10 |v| above its hull's distance, which its children then report (seen:
    1.3e-11 at 0.45 on tiny(mode=0)); plus the counted slack.  tol = 0 ends with an empty live set or at max_depth"""
    scene, st, P, res = state_of(name)
    sl = O.slack(P * res, st, O.prims_of(scene))
    traces = {}
    rec = ref_of(name).records(1.0, OFFSET, 0.0, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER, traces=traces)
    for u, tr in traces.items():
        for (d0, l0, h0, n0), (d1, l1, h1, n1) in zip(tr, tr[1:]):
            assert d1 == d0 + 1 and l1 >= l0 - 1e-10 * l0 - sl and h1 <= h0, (u, d0, l0, l1, h0, h1)
        assert tr[-1][3] == 0 or rec["depth"][u] == O.MAX_DEPTH, (u, tr[-1])
        assert bool(rec["flags"][u] & O.CONVERGED) == (tr[-1][3] == 0 or rec["hi"][u] - rec["lo"][u] <= 0.0)


@pytest.mark.parametrize("name", STATES)
def test_depth_zero_against_the_hull_clearance(pkg, name):
    """max_depth = 0: lo <= tj_audit's restated obs_clearance at the same range, and == min(hi, obs_clearance) wherever no live seed lost its certificate
    (such a seed counts lo = 0, so lo > 0 says there is none)"""
    scene, st, P, res = state_of(name)
    ref = ref_of(name)
    for rng in (0.3, 1.0):
        rec = ref.records(rng, OFFSET, pkg.OBSTACLE_TOL, 0, pkg.OBSTACLE_FRONTIER)
        d, ids = R.brute_obs(R.prims(), ref.H, O.prims_of(scene), rng)
        for u, (v, seg, k) in enumerate(R.robot_min(d, ids, rng)):
            assert rec["depth"][u] == 0 and rec["lo"][u] <= v, (u, rec["lo"][u], v)
            if rec["lo"][u] > 0.0:
                assert rec["lo"][u] == min(rec["hi"][u], v), (u, rec["lo"][u], rec["hi"][u], v)


def test_corner(pkg, scenes):
    """a primitive inside the hull of a corner the curve cuts: tj_audit (restated in corner_state) says OBS_CONTACT; the curve is clear, and says by how much"""
    scene, st, k, tv = O.corner_state(pkg, scenes, R.prims())
    X = O.prims_of(scene)
    tol, sl = pkg.OBSTACLE_TOL, O.slack(scene["P"] * 8, st, X)
    ref = O.Ref(pkg, R.prims(), st, scene["P"], 8, X)
    for rng in (0.3, INF):
        rec = ref.records(rng, OFFSET, tol, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER)
        print(rng, {n: rec[n][0] for n in O.FIELDS}, tv, sl)
        assert rec["flags"][0] == O.CLEAR | O.CONVERGED and rec["index"][0] == k
        assert abs(rec["hi"][0] - tv[0]) <= tol + sl and rec["hi"][0] > OFFSET and rec["lo"][0] > OFFSET


def test_pierce(pkg, scenes):
    """the straight flight through a cloud point: contact, lo == 0, hi <= 1e-5, the crossing time to 1e-5"""
    scene, st, k, t_cross = O.pierce_state(pkg, scenes)
    ref = O.Ref(pkg, R.prims(), st, scene["P"], 8, O.prims_of(scene))
    for rng in (0.3, INF):
        rec = ref.records(rng, OFFSET, pkg.OBSTACLE_TOL, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER)
        print(rng, {n: rec[n][0] for n in O.FIELDS})
        assert rec["flags"][0] & O.CONTACT and not rec["flags"][0] & O.CLEAR and rec["index"][0] == k
        assert rec["lo"][0] == 0.0 and rec["hi"][0] <= 1e-5 and abs(rec["time"][0] - t_cross) <= 1e-5


def test_miss(pkg, scenes):
    """the same line at a known perpendicular distance d > offset from one point"""
    scene, st, k, d = O.miss_state(pkg, scenes)
    X = O.prims_of(scene)
    tol, sl = pkg.OBSTACLE_TOL, O.slack(scene["P"] * 8, st, X)
    ref = O.Ref(pkg, R.prims(), st, scene["P"], 8, X)
    for rng in (0.3, INF):
        rec = ref.records(rng, OFFSET, tol, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER)
        print(rng, {n: rec[n][0] for n in O.FIELDS})
        assert rec["flags"][0] == O.CLEAR | O.CONVERGED and rec["index"][0] == k
        assert abs(rec["hi"][0] - d) <= tol + sl and abs(rec["time"][0] - 3.15) <= 1e-4
    rec = ref.records(0.2, OFFSET, tol, O.MAX_DEPTH, pkg.OBSTACLE_FRONTIER)      # nothing within 0.2: the sentinel
    assert {n: rec[n][0] for n in O.FIELDS} == O.sentinel(0.2)


def test_defaults_are_the_measured_ones(pkg):
    widths, floor, tol, biggest = O.default_tolerance(pkg, R.prims())
    print("widths per depth", ["%.3g" % w for w in widths], "floor", floor, "tol", tol, "largest live set", biggest)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert tol == pkg.OBSTACLE_TOL == float(re.search(r"#define TJ_OBSTACLE_TOL\s+(\S+)", hdr).group(1))
    want = max(4096, 1 << (4 * biggest - 1).bit_length())
    assert want == pkg.OBSTACLE_FRONTIER == int(re.search(r"#define TJ_OBSTACLE_FRONTIER\s+(\d+)", hdr).group(1))
    assert widths[floor] > 0 and (floor == O.MAX_DEPTH or widths[floor + 1] == 0.0 or not widths[floor + 1] <= widths[floor] / 2)
