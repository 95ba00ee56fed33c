"""CPU (-m "not gpu"): the restatement tests/test_gpu_closest.py holds the device to (tests/closest_ref.py) is itself held to the flown curves: the
converged bracket contains a truth that uses neither GJK nor subdivision, its upper end is the separation of the two curves at the reported time, the
constructed states give what they were built for, a truncated search still brackets the truth, depth 0 is tj_audit_timed's level 0, and the default
tolerance is the measured one.  Bars: slack = K(S) * eps * max|coordinate| (counted in tests/audit_timed_ref.py) and the tolerance asked for -- nothing
here is fitted to what the code returns.

Measured (printed by test_default_tolerance_is_the_measured_one; recorded in include/trajadmm.h): largest hi - lo per depth 0..17 over the three
end-to-end end states = 1.98e-2, 2.78e-3, 1.16e-3, 3.19e-4, 8.18e-5, 1.83e-5, 4.73e-6, 1.35e-6, 2.64e-7, 6.58e-8, 1.68e-8, 4.10e-9, 1.24e-9, 3.28e-10,
7.95e-11, 1.18e-11, 2.50e-12, 0 -> floor 2.50e-12 at depth 16 -> TJ_CLOSEST_TOL = 1e-10."""
import functools
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import closest_ref as K
from conftest import ROOT
from query_kit import pkg_module as _pkg

OFFSET = 0.1
STATES = ["chase", "crossing", "hover", "hard"]


@functools.lru_cache(maxsize=None)
def state_of(name):
    pkg = _pkg()
    if name.startswith("e2e_"):
        return T.e2e_state(name)
    if name.startswith("hard"):
        scene = pkg.scenes.hard()
        st = R.port_state(scene, 5 if name == "hard" else int(name[4:]))
        assert len(set(st["piece_time"])) > 1
        return st, scene["P"], 8
    st = getattr(T, name + "_state")(pkg, pkg.scenes)[1]
    return st, 4, 8


@functools.lru_cache(maxsize=None)
def truth_of(name):
    st, P, res = state_of(name)
    return T.truth(_pkg(), st, P, res)


@functools.lru_cache(maxsize=None)
def records_of(name, tol, max_depth=K.MAX_DEPTH, max_windows=K.FRONTIER):
    st, P, res = state_of(name)
    return K.closest_records(_pkg(), R.prims(), st, P, res, np.inf, OFFSET, tol, max_depth, max_windows)


@pytest.mark.parametrize("tol", [None, 1e-3, 0.0])
@pytest.mark.parametrize("name", STATES)
def test_bracket_holds_the_truth_and_hi_is_attained(pkg, name, tol):
    """with everything in range: hi is the separation of the two flown curves at `time`, within slack; CONVERGED means hi - lo <= tol"""
    tol = pkg.CLOSEST_TOL if tol is None else tol
    st, P, res = state_of(name)
    sl = T.slack(P * res, st["spline"])
    tv = truth_of(name)
    rec = records_of(name, tol)
    for u in range(st["spline"].shape[0]):
        print(name, tol, u, {n: rec[n][u] for n in K.FIELDS}, "truth", tv[u])
        assert rec["robot"][u] >= 0 and 0 <= rec["segment"][u] < P * res
        assert abs(rec["hi"][u] - T.separation_at(pkg, st, P, res, u, int(rec["robot"][u]), rec["time"][u])) <= sl, u
        assert rec["hi"][u] >= rec["lo"][u]
        if rec["flags"][u] & K.CONVERGED and tv[u][0] > 1e-4:
            assert rec["hi"][u] - rec["lo"][u] <= tol, (u, rec["hi"][u] - rec["lo"][u])
        assert not rec["flags"][u] & K.TRUNCATED
        if tol > 0 and tv[u][0] > 1e-4:
            assert rec["flags"][u] & K.CONVERGED, (u, rec["depth"][u])     # (a separation above the GJK's contact floor converges long before depth 40)


@pytest.mark.parametrize("tol", [None, 1e-3, 0.0])
@pytest.mark.parametrize("name", STATES)
def test_lo_is_below_the_truth(pkg, name, tol):
    """lo <= truth + slack, with everything in range.  The states whose true separation is 0 (chase, hover robot 1) are where the GJK's contact floor would put |v| ABOVE the truth (up to ~1e-5 instead of 0,
    DESIGN.md 3c); the certificate on lo (closest_ref._Eval: |v| counts only where v separates the origin from the hull) keeps the window that holds the
    contact alive with lo = 0."""
    tol = pkg.CLOSEST_TOL if tol is None else tol
    st, P, res = state_of(name)
    sl = T.slack(P * res, st["spline"])
    tv = truth_of(name)
    rec = records_of(name, tol)
    for u in range(st["spline"].shape[0]):
        print(name, tol, u, "lo", rec["lo"][u], "hi", rec["hi"][u], "truth", tv[u][0], "slack", sl)
    for u in range(st["spline"].shape[0]):
        assert rec["lo"][u] <= tv[u][0] + sl, (u, rec["lo"][u], tv[u])


def test_constructed_states(pkg):
    """chase: contact on both, robot 0 at the meeting time; crossing: clear and converged on sqrt(5); hover: robot 1 meets the arrived robot 0, robot 0 is clear"""
    tol = pkg.CLOSEST_TOL
    st, P, res = state_of("chase")
    sl = T.slack(32, st["spline"])
    rec = records_of("chase", tol)
    assert np.all(rec["flags"] & K.CONTACT) and (rec["robot"][0], rec["robot"][1]) == (1, 0) and np.all(rec["hi"] <= 1e-5)
    assert abs(rec["time"][0] - 1.6) <= 1e-5 and min(abs(rec["time"][1] - 1.6), abs(rec["time"][1] - 6.4)) <= 1e-5
    st, P, res = state_of("crossing")
    rec = records_of("crossing", tol)
    for u in (0, 1):
        assert rec["flags"][u] == K.CLEAR | K.CONVERGED and rec["hi"][u] - rec["lo"][u] <= tol
    assert abs(rec["hi"][0] - math.sqrt(5.0)) <= tol + sl and abs(rec["time"][0] - 2.4) <= 1e-4
    st, P, res = state_of("hover")
    rec = records_of("hover", tol)
    assert rec["flags"][1] & K.CONTACT and rec["robot"][1] == 0 and abs(rec["time"][1] - 3.6) <= 1e-5 and rec["time"][1] > 4 * st["piece_time"][0]
    assert rec["flags"][0] & K.CLEAR and rec["lo"][0] > 1.99
    # nothing within the default range of the crossing: range, -1 and CLEAR | CONVERGED without a single halving
    st, P, res = state_of("crossing")
    rec = K.closest_records(pkg, R.prims(), st, P, res, 0.3, OFFSET, tol)
    for u in (0, 1):
        assert (rec["lo"][u], rec["hi"][u], rec["time"][u], rec["robot"][u], rec["segment"][u], rec["depth"][u], rec["flags"][u]) == (0.3, 0.3, -1.0, -1, -1, 0, K.CLEAR | K.CONVERGED)


@pytest.mark.parametrize("name", STATES)
def test_depth_zero_is_the_level_zero_bracket(pkg, name):
    st, P, res = state_of(name)
    for rng in (np.inf, 0.3):
        rec = K.closest_records(pkg, R.prims(), st, P, res, rng, OFFSET, pkg.CLOSEST_TOL, 0)
        ref, _ = T.restated(pkg, R.prims(), st, P, res, rng, OFFSET, 0)
        assert np.all(rec["depth"] == 0)
        assert np.array_equal(rec["hi"], ref["timed_hi"]) and np.array_equal(rec["time"], ref["timed_time"])
        assert np.array_equal(rec["robot"], ref["timed_robot"]) and np.array_equal(rec["segment"], ref["timed_segment"])
        anchor = np.minimum(ref["timed_lo"], ref["timed_hi"])   # (tj_audit_timed's lo is the GJK's |v| as it is; here a window without a separating plane counts 0)
        assert np.all((rec["lo"] == anchor) | ((rec["lo"] == 0.0) & (ref["timed_lo"] <= 1e-4)))


@pytest.mark.parametrize("name", ["hard4", "e2e_scn_b", "crossing"])
def test_truncation_keeps_a_sound_bracket(pkg, name):
    """max_windows = 1: the search gives up where more than one window could hold the minimum (hard() after 4 iterations and the SCN-B end state: TRUNCATED on
    most robots; the crossing never holds a second live window and is not truncated), and what it returns still brackets the truth"""
    st, P, res = state_of(name)
    sl = T.slack(P * res, st["spline"])
    tv = truth_of(name)
    rec = records_of(name, pkg.CLOSEST_TOL, K.MAX_DEPTH, 1)
    full = records_of(name, pkg.CLOSEST_TOL)
    assert np.any(rec["flags"] & K.TRUNCATED) == (name != "crossing")
    for u in range(st["spline"].shape[0]):
        assert rec["lo"][u] <= tv[u][0] + sl and rec["hi"][u] >= full["hi"][u] and rec["lo"][u] <= full["lo"][u] + sl
        if not rec["flags"][u] & K.TRUNCATED:
            assert all(rec[n][u] == full[n][u] for n in K.FIELDS)


def test_work_is_below_the_uniform_level_six(pkg):
    """the point of the search: converged to 1e-10 with fewer windows than tj_audit_timed evaluates for its 4.7e-6 at level 6"""
    st, P, res = state_of("hard")
    rec = records_of("hard", pkg.CLOSEST_TOL)
    for u in range(st["spline"].shape[0]):
        assert rec["windows"][u] < K.level_window_count(pkg, st, P, res, u, np.inf, 6)


def test_default_tolerance_is_the_measured_one(pkg):
    widths, floor, tol = K.default_tolerance(pkg, R.prims())
    print("widths per depth", ["%.3g" % w for w in widths], "floor", floor, "tol", tol)
    assert tol == pkg.CLOSEST_TOL
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert float(re.search(r"#define TJ_CLOSEST_TOL\s+(\S+)", hdr).group(1)) == tol
    assert all(b <= a / 2 for a, b in zip(widths[:floor], widths[1:floor + 1])) and widths[floor] > 0
