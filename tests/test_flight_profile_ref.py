"""CPU: the restatement of tj_flight_profile (tests/flight_profile_ref.py) against the flown curve, against tj_audit's terms and against the other
queries' restatements; and the declarations.  The kernel itself is compared with the restatement by tests/test_gpu_flight_profile.py (-m gpu)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import closest_ref as CR
import flight_profile_ref as F
import obstacle_approach_ref as O
from conftest import ROOT

LD = np.longdouble
NAMES = ("tj_flight_profile", "tj_flight_profile_record_size", "tj_group_flight_profile")


def test_declared_exported_and_bound(pkg):
    """the header declares the three functions, the built library exports them and the package knows them (and mirrors the record and the constants)"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trajadmm.h")).read(), flags=re.S)
    lib = C.CDLL(pkg.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in pkg.EXPORTS, n
    assert lib.tj_flight_profile_record_size() == C.sizeof(pkg.TjProfileSample)
    raw = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    flags = {k.lower(): int(v) for k, v in re.findall(r"#define TJ_PROFILE_(HOVER|OBS_CONTACT|PAIR_CONTACT|SPEED|ACCEL)\s+(\d+)", raw)}
    assert flags == pkg.PROFILE_FLAGS == dict(hover=F.HOVER, obs_contact=F.OBS_CONTACT, pair_contact=F.PAIR_CONTACT, speed=F.SPEED, accel=F.ACCEL)
    assert int(re.search(r"#define TJ_PROFILE_MAX_SAMPLES\s+(\d+)", raw).group(1)) == pkg.PROFILE_MAX_SAMPLES == 65536
    assert re.search(r"#define TJ_PROFILE_MAX_RECORDS\s+\(1 << 24\)", raw) and pkg.PROFILE_MAX_RECORDS == 1 << 24
    assert hasattr(pkg.Solver, "flight_profile") and hasattr(pkg.Group, "flight_profile")
    assert [n for n, _ in pkg.TjProfileSample._fields_] == list(F.FIELDS)


@pytest.mark.parametrize("name", [n for n, _ in O.E2E])
def test_positions_and_dynamics_against_the_flown_curve(pkg, name):
    """the restatement's position against audit_timed_ref.curve_at (the Bezier points of `convert`, np.longdouble) and its speed / acceleration against
    audit_ref.curve_derivatives, at 12 times per robot inside its flight, on the four end-to-end end states; the bound is the counted slack of
    flight_profile_ref's docstring.  Largest differences observed, all on e2e_scn_c3 (pytest -s prints them per state), with their fraction of the bound: position 9.4e-15
    (1.4e-3), speed 3.7e-14 (9.8e-5), acceleration 9.4e-13 (1.2e-4): the bound counts every rounding at its worst and in one direction."""
    st, P, res = T.e2e_state(name)
    S, U = P * res, st["spline"].shape[0]
    M = float(np.abs(st["spline"]).max())
    rng = np.random.default_rng(17)
    worst = np.zeros(3); frac = np.zeros(3)
    for u in range(U):
        pt = float(st["piece_time"][u])
        times = rng.uniform(0.0, P * pt * (1 - 1e-9), 12)
        pos, speed, accel, seg = F.points(pkg, dict(spline=st["spline"][u:u + 1], piece_time=st["piece_time"][u:u + 1]), P, res, times)
        truth = T.curve_at(pkg, st["spline"][u], pt, P, res, times)
        for k, t in enumerate(times):
            j = int(seg[0, k])
            assert j < S
            kk = j % res
            w = (kk + 1) / float(res) - kk / float(res)
            f = (LD(t) / LD(pt)) * LD(res) - LD(j)                     # how far into segment j, in np.longdouble
            f = min(max(f, LD(0)), LD(1) - LD(1e-18))
            d1, d2 = R.curve_derivatives(pkg, st, P, res, u, j, f)
            errs = (float(np.abs(LD(1) * pos[0, k] - truth[k]).max()), abs(float(LD(speed[0, k]) - R.ldnorm(d1))), abs(float(LD(accel[0, k]) - R.ldnorm(d2))))
            bounds = (F.slack_pos(S, M), F.slack_speed(S, M, w, pt, speed[0, k]), F.slack_accel(S, M, w, pt, accel[0, k]))
            for i in range(3):
                worst[i] = max(worst[i], errs[i]); frac[i] = max(frac[i], errs[i] / bounds[i])
                assert errs[i] <= bounds[i], (name, u, k, i, errs[i], bounds[i])
    print("OBSERVED", name, "pos / speed / accel:", worst, "fraction of the bound:", frac)


def test_segment_starts_are_the_audit_terms(pkg, scenes):
    """at t = (j / res) * pt the profile's speed and acceleration ARE tj_audit's first terms of segment j: == on doubles"""
    scene = scenes.tiny(mode=1)
    st = R.port_state(scene, 3)
    P, res = scene["P"], 8
    S = P * res
    for u in range(scene["U"]):
        pt = float(st["piece_time"][u])
        times = np.array([(j / float(res)) * pt for j in range(S)])
        one = dict(spline=st["spline"][u:u + 1], piece_time=st["piece_time"][u:u + 1])
        _, speed, accel, seg = F.points(pkg, one, P, res, times)
        sp, ac = R.limit_terms(pkg, st, P, res, u)
        assert np.array_equal(seg[0], np.arange(S))
        assert np.array_equal(speed[0], sp[:, 0]) and np.array_equal(accel[0], ac[:, 0])


def test_profile_minima_against_the_other_queries(pkg, scenes):
    """sound inequalities between restatements, on hard() after 3 iterations and a 257-sample grid: the smallest sampled obstacle distance of a robot is not below
    tj_obstacle_approach's lo (up to its stated limit, 1e-10 relative: the GJK's stop rule), and the smallest sampled robot distance WHILE THE ROBOT FLIES is
    not below tj_closest_approach's lo (whose bracket covers the robot's own flight: after its arrival a partner may still come nearer)"""
    scene = scenes.hard()
    st = R.port_state(scene, 3)
    P, res, U = scene["P"], 8, scene["U"]
    p = R.params_of(pkg)
    pr = R.prims()
    X = F.prims_of(scene)
    prof = F.profile(pkg, pr, st, P, res, X, F.grid(st, P, 257), p)
    for rng in (R.default_range(p), 1.0):
        oa = O.Ref(pkg, pr, st, P, res, X).records(rng, p["offset"], 0.0, O.MAX_DEPTH, 4096)
        cl = CR.closest_records(pkg, pr, st, P, res, rng, p["offset"], 0.0)
        for u in range(U):
            assert prof["obs_distance"][u].min() >= oa["lo"][u] * (1 - 1e-10), (rng, u)
            flying = prof["segment"][u] < P * res
            assert prof["robot_distance"][u][flying].min() >= cl["lo"][u], (rng, u)


def test_constructed_sets_meet_their_preconditions():
    """twin_cloud: bit-equal distances from an exactly representable centre; sphere_cloud: 4 096 distances within rounding of the radius"""
    c = np.array([1.25, -3.0, 0.5])
    cloud = F.twin_cloud(np.random.default_rng(1).uniform(5, 9, (50, 3)), c, 7, 31)
    assert F.nearest_primitive(None, cloud, c) == (0.5, 7)
    assert F.nearest_primitive(None, F.twin_cloud(cloud, c, 31, 7), c) == (0.5, 7)
    sph = F.sphere_cloud(c)
    d = np.sqrt(((sph - c) ** 2).sum(axis=1))
    assert sph.shape == (4096, 3) and np.abs(d - 2.0).max() < 1e-14
