"""CPU (-m "not gpu"): the restatement tests/test_gpu_peak_dynamics.py holds the device to (tests/peak_dynamics_ref.py) is itself held to a truth that uses
neither nets' hulls nor subdivision: mpmath forms the polynomial d/ds |q(s)|^2 of every shortlisted segment, its real roots in [0, 1] and the ends give the
true peak; mpmath.quad of |v(s)| gives the true length.  States: the final states of the four end-to-end fixtures and tiny()'s initial states.

The margin on `hi` (and on the length bracket) is relative to the robot's depth-0 hi of the quantity: MARGIN = max(16 x the measured excess, 64 * 2^-53).  The
measured excess (test_bracket_holds_the_truth prints it: the largest (truth - hi) / hi0 over all states, robots and quantities) is 1.72e-16, 1.5 * 2^-53, at
tol = 0 where hi == lo is the rounded value of the peak itself -- 16 x that is 2.75e-15, below 64 * 2^-53 = 7.1e-15: hi never fell
below the truth by more than its own rounding -- so the margin is 64 * 2^-53; it is not taken from the device code.

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h): relative widths per depth 1.49e-2, 7.88e-3, 3.04e-4, ... 1.15e-16
at depth 30, 0 at depth 31 -> TJ_PEAK_TOL = 1e-14; largest live set 4 -> TJ_PEAK_FRONTIER = 1024; length widths per level 1.69e-4, 4.30e-5, 1.08e-5, 2.70e-6,
6.76e-7 -> TJ_PEAK_LENGTH_LEVELS = 4."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import peak_dynamics_ref as D
from conftest import ROOT
from query_kit import pkg_module as _pkg

EPS = 2.0 ** -53
MEASURED_EXCESS = 1.72e-16                  # the largest (truth - hi) / hi0 seen (tiny(mode=1)'s initial state, tol = 0)
MARGIN = max(16 * MEASURED_EXCESS, 64 * EPS)
STATES = ["e2e_scn_a", "e2e_scn_b", "e2e_scn_c3", "e2e_scn_b_coupled", "tiny0", "tiny1"]
VEL, ACC = 2.0, 2.0


@functools.lru_cache(maxsize=None)
def state_of(name):
    """(state, P, res)"""
    if name.startswith("e2e"):
        return T.e2e_state(name)
    scene = _pkg().scenes.tiny(mode=int(name[4:]))
    st = R.port_state(scene, 0)
    assert R.valid_state(st, scene["U"])
    return st, scene["P"], 8


@functools.lru_cache(maxsize=None)
def ref_of(name):
    st, P, res = state_of(name)
    return D.Ref(_pkg(), st, P, res)


@functools.lru_cache(maxsize=None)
def truth_of(name, u, q):
    return D.truth(ref_of(name), u, q)


@functools.lru_cache(maxsize=None)
def records_of(name, tol):
    raw = {}
    return ref_of(name).records(tol, D.MAX_DEPTH, _pkg().PEAK_FRONTIER, 0, VEL, ACC, owned=list(robots_of(name)), raw=raw), raw


def robots_of(name):
    """every robot of a small state, the first three of a large one: mpmath is the cost"""
    return range(min(ref_of(name).U, 3))


@pytest.mark.parametrize("name", STATES)
def test_bracket_holds_the_truth(pkg, name):
    """lo <= truth <= hi within MARGIN * hi0 at the default tolerance, at 1e-3 and at 0; the curve evaluated at the lo sample gives lo; `time` is that sample's"""
    import mpmath as mp
    ref = ref_of(name)
    worst = -np.inf
    for tol in (pkg.PEAK_TOL, 1e-3, 0.0):
        rec, raw = records_of(name, tol)
        for u in robots_of(name):
            for q, qn in enumerate(D.QUANTITIES):
                r = raw[(u, q)]
                tv, tseg, ts = truth_of(name, u, q)
                hi0 = ref.search(u, q, 0.0, 0, 1 << 20)["hi"]
                exc = float((tv - mp.mpf(r["hi"])) / mp.mpf(hi0)) if hi0 > 0 else 0.0
                worst = max(worst, exc)
                print(name, tol, u, qn, {n: r[n] for n in D.PEAK_FIELDS}, "truth", float(tv), tseg, ts, "excess", exc)
                assert mp.mpf(r["lo"]) <= tv + MARGIN * hi0 and tv <= mp.mpf(r["hi"]) + MARGIN * hi0, (u, qn, r["lo"], float(tv), r["hi"])
                assert not r["flags"] & D.TRUNCATED
                assert abs(D.value_at(ref, u, q, r["segment"], r["s"]) - mp.mpf(r["lo"])) <= MARGIN * hi0, (u, qn)
                assert r["time"] == ref.time_of(u, r["segment"], r["s"]) and 0 <= r["segment"] < ref.S and 0.0 <= r["s"] <= 1.0
                if tol > 0:
                    assert r["flags"] & D.CONVERGED and r["hi"] - r["lo"] <= tol * r["hi"]
                else:   # tol = 0 closes the bracket to the measured floor: TJ_PEAK_TOL is >= 10 x it
                    assert r["hi"] - r["lo"] <= (pkg.PEAK_TOL / 10) * r["hi"], (u, qn, r["lo"], r["hi"], r["depth"])
    print(name, "largest (truth - hi) / hi0:", worst)
    assert worst <= MEASURED_EXCESS, (name, worst)   # the figure recorded here, in the header and in DESIGN.md 3k is what is measured


@pytest.mark.parametrize("name", STATES)
def test_depth_zero_is_the_audit(pkg, name):
    """max_depth = 0: speed.hi / accel.hi and their segments are tj_audit's restated speed / accel (audit_ref.limits_of), bit for bit"""
    st, P, res = state_of(name)
    rec = ref_of(name).records(pkg.PEAK_TOL, 0, pkg.PEAK_FRONTIER, 0, VEL, ACC)
    hi_only = ref_of(name)
    for u, (sp, ss, ac, as_, dur) in enumerate(R.limits_of(pkg, st, P, res)):
        assert rec["speed_hi"][u] == sp and rec["accel_hi"][u] == ac and rec["duration"][u] == dur and rec["speed_depth"][u] == 0
        # the segment of the hull maximum: the first segment whose ub is the largest (tj_audit's); lo's segment is the attained sample's and may differ
        ub = hi_only.evaluate(u, 0, np.arange(hi_only.S), np.zeros(hi_only.S), np.ones(hi_only.S))[0]
        assert int(np.argmax(ub)) == ss and ub.max() == sp


@pytest.mark.parametrize("name", STATES)
def test_length(pkg, name):
    """mpmath.quad of |v(s)| lies in [length_lo, length_hi] at every level 0..7; the widths fall about 4 x per level (> 3 x from level 2 on); log_data's 0.1-step
    chord sum is <= length_hi"""
    import mpmath as mp
    st, P, res = state_of(name)
    ref = ref_of(name)
    for u in range(min(ref.U, 2)):   # (mpmath.quad is the cost: every state, its first two robots)
        tl = D.true_length(ref, u)
        chords = D.chord_sum(pkg, st, P, res, u)
        widths = []
        for L in range(8):
            lo, hi = ref.length(u, L)
            print(name, u, L, lo, hi, float(tl), chords)
            assert mp.mpf(lo) * (1 - MARGIN) <= tl <= mp.mpf(hi) * (1 + MARGIN), (u, L, lo, float(tl), hi)
            assert chords <= hi * (1 + MARGIN)
            widths.append(hi - lo)
        for L in range(2, 8):   # (a straight flight -- tiny()'s initial state -- has no width to shrink: chord and polygon agree to rounding)
            assert widths[L] < widths[L - 1] / 3 or widths[L - 1] <= 1e-12 * float(tl), (u, L, widths)
        assert chords <= float(tl) * (1 + 1e-15)


def test_restriction_of_the_whole_window_is_the_raw_net():
    rng = np.random.default_rng(5)
    for N in (6, 5, 4, 3):
        p = rng.standard_normal((7, N, 3))
        assert np.array_equal(D.bez_restrict(p, np.zeros(7), np.ones(7)), p)
    p = rng.standard_normal((7, 6, 3))
    sa, sb = rng.random(7) * 0.5, 0.5 + rng.random(7) * 0.5
    assert np.array_equal(D.bez_restrict(p, sa, sb), T.bez_restrict(p, sa, sb))          # degree 5: audit_timed_ref's bits


def test_constructed_states(pkg, scenes):
    """the straight flight at constant speed: every segment ties, segment 0 at time 0, nothing live at depth 0; the hover: all zero, no NaN"""
    scene, st = D.line_state(pkg, scenes)
    rec = D.Ref(pkg, st, scene["P"], 8).records(pkg.PEAK_TOL, D.MAX_DEPTH, pkg.PEAK_FRONTIER, pkg.PEAK_LENGTH_LEVELS, VEL, ACC)
    assert rec["speed_segment"][0] == 0 and rec["speed_time"][0] == 0.0 and rec["speed_depth"][0] == 0 and rec["speed_windows"][0] == scene["P"] * 8
    assert rec["speed_flags"][0] == D.CONVERGED and rec["speed_lo"][0] == rec["speed_hi"][0] > 0
    assert rec["accel_hi"][0] == 0.0 and rec["jerk_hi"][0] == 0.0 and rec["accel_flags"][0] == D.CONVERGED
    assert rec["length_lo"][0] == rec["length_hi"][0] == 5.0 * scene["P"]
    scene, st = D.hover_state(pkg, scenes)
    rec = D.Ref(pkg, st, scene["P"], 8).records(pkg.PEAK_TOL, D.MAX_DEPTH, pkg.PEAK_FRONTIER, pkg.PEAK_LENGTH_LEVELS, VEL, ACC)
    for n in D.FIELDS:
        assert np.all(np.isfinite(rec[n]))
    for q in D.QUANTITIES:
        assert rec[q + "_lo"][0] == rec[q + "_hi"][0] == 0.0 and rec[q + "_flags"][0] == D.CONVERGED and rec[q + "_depth"][0] == 0
    assert rec["time_scale"][0] == 0.0 and rec["length_hi"][0] == 0.0 and rec["flags"][0] == D.DYN_SPEED_OK | D.DYN_ACCEL_OK


def test_defaults_are_the_measured_ones(pkg):
    widths, floor, tol, biggest, frontier, lw, level, lives = D.default_tolerance(pkg)
    print("widths per depth", ["%.3g" % w for w in widths], "live sets", lives, "floor", floor, "tol", tol, "largest live set", biggest, "frontier", frontier)
    print("length widths per level", ["%.3g" % w for w in lw], "level", level)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert tol == pkg.PEAK_TOL == float(re.search(r"#define TJ_PEAK_TOL\s+(\S+)", hdr).group(1))
    assert frontier == pkg.PEAK_FRONTIER == int(re.search(r"#define TJ_PEAK_FRONTIER\s+(\d+)", hdr).group(1)) and frontier >= 1024
    assert level == pkg.PEAK_LENGTH_LEVELS == int(re.search(r"#define TJ_PEAK_LENGTH_LEVELS\s+(\d+)", hdr).group(1))
    assert D.MAX_DEPTH == pkg.PEAK_MAX_DEPTH == int(re.search(r"#define TJ_PEAK_MAX_DEPTH\s+(\d+)", hdr).group(1))
    assert D.MAX_LENGTH_LEVELS == pkg.PEAK_MAX_LENGTH_LEVELS == int(re.search(r"#define TJ_PEAK_MAX_LENGTH_LEVELS\s+(\d+)", hdr).group(1))
    assert widths[floor] > 0 and (floor == D.MAX_DEPTH or widths[floor + 1] == 0.0 or not widths[floor + 1] <= widths[floor] / 2)
    assert lw[level] < 1e-6 and (level == 0 or lw[level - 1] >= 1e-6)


def test_record_sizes(pkg):
    assert C.sizeof(pkg.TjPeak) == 40 and C.sizeof(pkg.TjDynamicsRobot) == 160
    assert pkg.load_library().tj_dynamics_record_size() == 160
    assert pkg.PEAK_FLAGS == dict(converged=D.CONVERGED, truncated=D.TRUNCATED)
    assert pkg.PEAK_DYN_FLAGS == dict(speed=D.DYN_SPEED, speed_ok=D.DYN_SPEED_OK, accel=D.DYN_ACCEL, accel_ok=D.DYN_ACCEL_OK)
