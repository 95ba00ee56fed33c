"""CPU (-m "not gpu"): the restatement tests/test_gpu_pair_approach.py holds the device to (tests/pair_approach_ref.py) is itself held to the flown curves --
every row's bracket contains a truth that uses neither GJK nor subdivision, every pair WITHOUT a row is at least `range` apart, the rows agree with the
per-robot search of tests/closest_ref.py, the committed defaults are the measured ones -- and the host surface that needs no GPU: the record's size, the
exported symbols, the symmetric merge.  Bars: slack = K(S) * eps * max|coordinate| (counted in tests/audit_timed_ref.py) and the tolerance asked for.

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h): largest hi - lo per depth 0..17 over the listed pairs of the three
end-to-end end states = 2.14e-2, 3.61e-3, 1.32e-3, 3.19e-4, 8.18e-5, 1.83e-5, 4.73e-6, 1.35e-6, 2.64e-7, 6.58e-8, 1.68e-8, 4.10e-9, 1.24e-9, 3.28e-10,
7.95e-11, 1.18e-11, 2.50e-12, 0 -> TJ_PAIR_TOL = 1e-10; largest live set of any pair 2 -> TJ_PAIR_FRONTIER = 64; listed directed pairs 14 / 126 / 14."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import closest_ref as K
import pair_approach_ref as Q
from conftest import ROOT
from query_kit import pkg_module as _pkg

LD = np.longdouble
OFFSET, DEFAULT = 0.1, 0.1 + 2 * 0.1
STATES = [("e2e_scn_b", DEFAULT), ("e2e_scn_c3", DEFAULT), ("e2e_scn_b_coupled", DEFAULT), ("chase", np.inf), ("crossing", np.inf), ("hover", np.inf)]


@functools.lru_cache(maxsize=None)
def state_of(name):
    pkg = _pkg()
    if name.startswith("e2e_"):
        return T.e2e_state(name)
    return getattr(T, name + "_state")(pkg, pkg.scenes)[1], 4, 8


@functools.lru_cache(maxsize=None)
def rows_of(name, rng, tol):
    st, P, res = state_of(name)
    return Q.pair_rows(_pkg(), R.prims(), st, P, res, rng, OFFSET, tol)


@functools.lru_cache(maxsize=None)
def curves_of(name, u, n=1001):
    """every robot's position [U][n][3] (longdouble) at n times over robot u's flight, and the times"""
    st, P, res = state_of(name)
    t = np.linspace(LD(0), LD(P) * LD(st["piece_time"][u]), n, dtype=LD)
    return t, np.stack([T.curve_at(_pkg(), st["spline"][q], st["piece_time"][q], P, res, t) for q in range(st["spline"].shape[0])])


def sampled(name, u, q):
    _, c = curves_of(name, u)
    d = c[u] - c[q]
    return float(np.sqrt((d * d).sum(axis=1)).min())


@pytest.mark.parametrize("name,rng", STATES)
def test_every_bracket_holds_the_truth(pkg, name, rng):
    """lo - slack <= the sampled separation of the pair over robot's flight (with the sample at the row's own time) <= hi + slack; hi is attained at `time`"""
    st, P, res = state_of(name)
    sl = T.slack(P * res, st["spline"])
    rows = rows_of(name, rng, pkg.PAIR_TOL)
    assert len(rows["robot"]) > 0
    assert list(zip(rows["robot"], rows["partner"])) == sorted(zip(rows["robot"], rows["partner"]))
    for k in range(len(rows["robot"])):
        u, q = int(rows["robot"][k]), int(rows["partner"][k])
        truth = sampled(name, u, q)
        print(name, u, q, {n: rows[n][k] for n in Q.FIELDS}, "sampled", truth)
        assert rows["lo"][k] <= rows["hi"][k] and not rows["flags"][k] & Q.TRUNCATED
        assert rows["lo"][k] - sl <= truth, (u, q)
        if rows["segment"][k] >= 0:
            at = T.separation_at(pkg, st, P, res, u, q, rows["time"][k])
            assert abs(at - rows["hi"][k]) <= sl and min(truth, at) <= rows["hi"][k] + sl, (u, q)
            assert 0 <= rows["time"][k] <= P * st["piece_time"][u] * (1 + 1e-15)
        else:
            assert rows["hi"][k] == rng and rows["time"][k] == -1.0


@pytest.mark.parametrize("name,rng", [s for s in STATES if s[1] != np.inf] + [("crossing", DEFAULT)])
def test_an_unlisted_pair_is_at_least_range_apart(pkg, name, rng):
    st, P, res = state_of(name)
    sl = T.slack(P * res, st["spline"])
    rows = rows_of(name, rng, pkg.PAIR_TOL)
    listed = set(zip(rows["robot"].tolist(), rows["partner"].tolist()))
    U = st["spline"].shape[0]
    for u in range(U):
        for q in range(U):
            if q != u and (u, q) not in listed:
                assert sampled(name, u, q) >= rng - sl, (u, q)
    if name == "crossing":
        assert not listed


@pytest.mark.parametrize("name,rng", STATES)
def test_rows_agree_with_the_per_robot_search(pkg, name, rng):
    """closest.lo <= min over partners of hi, min over partners of lo <= closest.hi, and the per-robot partner has a row"""
    st, P, res = state_of(name)
    rows = rows_of(name, rng, pkg.PAIR_TOL)
    rec = K.closest_records(pkg, R.prims(), st, P, res, rng, OFFSET, pkg.CLOSEST_TOL)
    seen = 0
    for u in range(st["spline"].shape[0]):
        m = rows["robot"] == u
        if rec["robot"][u] < 0:
            assert not np.any(rows["segment"][m] >= 0)      # nothing attained below range for this robot: no row of it names a sample either
            continue
        seen += 1
        assert m.any() and rec["robot"][u] in rows["partner"][m]
        assert rec["lo"][u] <= rows["hi"][m].min() and rows["lo"][m].min() <= rec["hi"][u]
    assert seen > 0


def test_constructed_states(pkg):
    tol = pkg.PAIR_TOL
    rows = rows_of("chase", np.inf, tol)
    assert list(zip(rows["robot"], rows["partner"])) == [(0, 1), (1, 0)] and np.all(rows["flags"] & Q.CONTACT) and abs(rows["time"][0] - 1.6) <= 1e-5
    st, P, res = state_of("crossing")
    rows = rows_of("crossing", np.inf, tol)
    assert np.all(rows["flags"] == Q.CLEAR | Q.CONVERGED) and abs(rows["hi"][0] - 5.0 ** 0.5) <= tol + T.slack(32, st["spline"])
    rows = rows_of("hover", np.inf, tol)
    assert rows["flags"][1] & Q.CONTACT and abs(rows["time"][1] - 3.6) <= 1e-5 and rows["flags"][0] & Q.CLEAR


def test_truncation_is_per_pair(pkg):
    """max_windows = 1 on the SCN-B end state: a pair that holds two live windows is TRUNCATED with the record of its last completed round, the others are untouched"""
    st, P, res = state_of("e2e_scn_b")
    full = rows_of("e2e_scn_b", DEFAULT, 0.0)
    cut = Q.pair_rows(pkg, R.prims(), st, P, res, DEFAULT, OFFSET, 0.0, Q.MAX_DEPTH, 1)
    t = (cut["flags"] & Q.TRUNCATED) != 0
    assert t.any() and not t.all()
    for n in Q.FIELDS:
        assert np.array_equal(cut[n][~t], full[n][~t]), n
    assert np.all(cut["depth"][t] < full["depth"][t]) and np.all(cut["lo"][t] <= full["lo"][t]) and np.all(cut["hi"][t] >= full["hi"][t])


def test_defaults_are_the_measured_ones(pkg):
    widths, floor, tol, widest, frontier, listed = Q.default_tolerance(pkg, R.prims())
    print("widths per depth", ["%.3g" % w for w in widths], "floor", floor, "tol", tol, "widest live set", widest, "frontier", frontier, "listed", listed)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert tol == pkg.PAIR_TOL == float(re.search(r"#define TJ_PAIR_TOL\s+(\S+)", hdr).group(1))
    assert frontier == pkg.PAIR_FRONTIER == int(re.search(r"#define TJ_PAIR_FRONTIER\s+(\S+)", hdr).group(1))
    assert pkg.PAIR_MAX_DEPTH == Q.MAX_DEPTH == int(re.search(r"#define TJ_PAIR_MAX_DEPTH\s+(\S+)", hdr).group(1))
    assert pkg.PAIR_MAX_WINDOWS == Q.MAX_WINDOWS == int(re.search(r"#define TJ_PAIR_MAX_WINDOWS\s+(\S+)", hdr).group(1))
    assert all(b <= a / 2 for a, b in zip(widths[:floor], widths[1:floor + 1])) and widths[floor] > 0
    assert listed == dict(e2e_scn_b=14, e2e_scn_c3=126, e2e_scn_b_coupled=14)      # the header's table


def test_host_surface(pkg):
    """needs no GPU: the record's size on both sides, the flag values, the exported symbols"""
    lib = pkg.load_library()
    assert lib.tj_pair_record_size() == C.sizeof(pkg.TjPairRecord) == 48
    for s in ("tj_pair_approach", "tj_pair_record_size", "tj_group_pair_approach"):
        assert s in pkg.EXPORTS and hasattr(lib, s), s
    assert pkg.PAIR_FLAGS == dict(contact=Q.CONTACT, clear=Q.CLEAR, converged=Q.CONVERGED, truncated=Q.TRUNCATED)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    for n, v in pkg.PAIR_FLAGS.items():
        assert int(re.search(r"#define TJ_PAIR_%s\s+(\d+)" % n.upper(), hdr).group(1)) == v
    n = C.c_int(7)
    assert lib.tj_pair_approach(None, C.c_double(0.0), C.c_double(-1.0), C.c_int(-1), C.c_int(0), None, C.c_int(0), C.byref(n)) == -1


def _rows(*rs):
    return {n: np.array([r[i] for r in rs], dtype=np.float64 if n in Q.FIELDS[:3] else np.int32) for i, n in enumerate(Q.FIELDS)}


def test_symmetric_merge(pkg):
    """hand-made rows (lo, hi, time, robot, partner, segment, depth, flags, windows): both directions, one direction, equal hi"""
    rng = 0.3
    rows = _rows((0.05, 0.06, 1.5, 0, 1, 3, 9, Q.CONTACT | Q.CONVERGED, 40),     # (0, 1) and (1, 0): the smaller hi is (1, 0)'s
                 (0.20, 0.25, 2.5, 0, 4, 5, 7, Q.CLEAR | Q.CONVERGED, 30),       # (0, 4) alone: (4, 0) counts as rng
                 (0.04, 0.05, 1.7, 1, 0, 4, 11, Q.CONTACT, 50),
                 (0.15, 0.20, 0.5, 2, 3, 1, 5, Q.CLEAR | Q.CONVERGED, 10),       # (2, 3) and (3, 2) with equal hi: (2, 3) gives the sample
                 (0.12, 0.20, 0.7, 3, 2, 2, 6, Q.CLEAR | Q.TRUNCATED, 12),
                 (0.28, 0.30, -1.0, 5, 2, -1, 0, Q.CLEAR | Q.CONVERGED, 2))      # (5, 2) alone, listed for its lo: hi == rng, nothing sampled
    m = pkg.merge_pairs(rows, rng, OFFSET)
    want = dict(robot=[0, 0, 2, 2], partner=[1, 4, 3, 5], lo=[0.04, 0.20, 0.12, 0.28], hi=[0.05, 0.25, 0.20, 0.30], time=[1.7, 2.5, 0.5, -1.0], segment=[4, 5, 1, -1],
                of=[1, 0, 2, 5], depth=[11, 7, 6, 0], windows=[90, 30, 22, 2],
                flags=[Q.CONTACT, Q.CLEAR | Q.CONVERGED, Q.CLEAR | Q.TRUNCATED, Q.CLEAR | Q.CONVERGED])
    assert set(m) == set(want)
    for n, v in want.items():
        assert np.array_equal(m[n], np.array(v)), (n, m[n], v)
    ref = Q.merge_symmetric(rows, rng, OFFSET)
    for n in want:
        assert np.array_equal(m[n], ref[n]), n
    assert pkg.merge_pairs(_rows((0.05, 0.06, 1.5, 0, 1, 3, 9, Q.CLEAR | Q.CONVERGED, 40)), 0.08, OFFSET)["flags"][0] == Q.CONVERGED   # rng <= offset: the missing side certifies nothing
    empty = pkg.merge_pairs(_rows(), rng, OFFSET)
    assert all(len(v) == 0 for v in empty.values())
