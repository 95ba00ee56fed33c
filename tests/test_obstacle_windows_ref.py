"""CPU (-m "not gpu"): the restatement tests/test_gpu_obstacle_windows.py holds the device to (tests/obstacle_windows_ref.py) is itself held to the flown curve:
closed forms on the straight flights (the distance is 2 |t - 3.15| on pierce_state), and on five constructed states a truth that uses neither GJK nor
subdivision -- every sample within dist lies inside a row, every sure time and every time inside an IN leaf IS within dist, a RESOLVED row's brackets hold the
first and the last crossing of the level.  Bars: slack = obstacle_approach_ref.slack (counted in tests/audit_timed_ref.py), the truth's grid step and the
tolerance asked for -- nothing here is fitted to what the code returns.

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h and DESIGN.md 3m): over the four end-to-end end states and their
iteration-0 states at dist = 0.1 and 0.3 the largest live set of a segment is 4 windows and the largest leaf list 25 -> TJ_OBSWIN_FRONTIER = 128; no row is
UNCERTAIN or TRUNCATED; the widest bracket is 1.22e-3 s at dist = 0.3 (tol = 1.5e-3 s)."""
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import obstacle_approach_ref as O
import obstacle_windows_ref as W
from conftest import ROOT

OFFSET, MARGIN, VEL = 0.1, 0.1, 2.0
TOL = W.default_tol(OFFSET, OFFSET, VEL)
N_GRID = 4001


def rows_of(pkg, scenes, name):
    return W.built(pkg, scenes, R.prims(), name)


def test_pierce_is_the_closed_form(pkg, scenes):
    """the distance is 2 |t - 3.15|: within 0.1 exactly over [3.10, 3.20], a chain across the boundary of segments 24 and 25 at 3.125"""
    scene, st, dist, ref, rows, leaves = rows_of(pkg, scenes, "pierce")
    assert dist == OFFSET and TOL == 5e-4 and len(rows["robot"]) == 1
    r = {n: rows[n][0] for n in W.FIELDS}
    assert r["t_first_lo"] <= 3.10 <= r["t_first_hi"] and r["t_last_lo"] <= 3.20 <= r["t_last_hi"]
    assert r["t_first_hi"] - r["t_first_lo"] <= TOL and r["t_last_hi"] - r["t_last_lo"] <= TOL
    assert r["flags"] == W.CERTAIN | W.RESOLVED
    edge = sum(b - a for a, b, is_in, _, _ in leaves[0][0] if not is_in)
    assert all(b - a <= TOL for a, b, is_in, _, _ in leaves[0][0] if not is_in)
    assert 0.1 - 2 * TOL - edge <= r["within_lo"] <= 0.1
    assert (r["segment_first"], r["segment_last"]) == (24, 25) and r["t_first_lo"] < 3.125 < r["t_last_hi"] and r["index"] == 77
    assert r["leaves"] == len(leaves[0][0]) and any(a == 3.125 for a, _, _, _, _ in leaves[0][0]) and any(b == 3.125 for _, b, _, _, _ in leaves[0][0])


def test_miss_is_the_closed_form(pkg, scenes):
    """the perpendicular distance is 0.25: nothing at dist = 0.1, one row at 0.3 whose half-width is sqrt(0.3^2 - 0.25^2) / 2 (the speed is 2)"""
    scene, st, dist, ref, rows, leaves = rows_of(pkg, scenes, "miss")
    none = ref.rows(OFFSET, TOL)
    assert all(len(none[n]) == 0 for n in W.FIELDS)
    assert dist == 0.3 and len(rows["robot"]) == 1
    hw = math.sqrt(0.09 - 0.0625) / 2
    assert rows["t_first_lo"][0] <= 3.15 - hw <= rows["t_first_hi"][0] and rows["t_last_lo"][0] <= 3.15 + hw <= rows["t_last_hi"][0]
    assert rows["flags"][0] == W.CERTAIN | W.RESOLVED and rows["index"][0] == 77
    assert abs(rows["closest"][0] - 0.25) <= 0.01 and rows["closest"][0] >= 0.25 - O.slack(ref.S, st, O.prims_of(scene))


def test_two_points_merge_and_split(pkg, scenes):
    near, far = rows_of(pkg, scenes, "two_near")[4], rows_of(pkg, scenes, "two_far")[4]
    assert len(near["robot"]) == 1 and near["t_first_lo"][0] <= 3.10 <= near["t_first_hi"][0] and near["t_last_lo"][0] <= 3.275 <= near["t_last_hi"][0]
    assert len(far["robot"]) == 2 and list(far["index"]) == [77, 78] and far["t_last_hi"][0] < far["t_first_lo"][1]
    assert far["windows"][0] == far["windows"][1]                                         # the robot's work, on each of its rows


@pytest.mark.parametrize("name", W.STATES)
def test_rows_are_sound_against_the_flown_curve(pkg, scenes, name):
    scene, st, dist, ref, rows, leaves = rows_of(pkg, scenes, name)
    X = O.prims_of(scene)
    sl = O.slack(ref.S, st, X)
    tol = W.default_tol(dist, OFFSET, VEL)
    assert len(rows["robot"]) > 0
    for u, (t, d, cross) in enumerate(W.truth(pkg, st, scene["P"], 8, X, dist, N_GRID)):
        step = float(t[1] - t[0])
        mine = np.flatnonzero(rows["robot"] == u)
        # every sample that IS within dist lies inside a row
        inside = np.zeros(len(t), dtype=bool)
        for k in mine:
            inside |= (t >= rows["t_first_lo"][k]) & (t <= rows["t_last_hi"][k])
        assert not np.any((d <= dist - sl) & ~inside), (name, u, t[(d <= dist - sl) & ~inside])
        # every sure time, and every sampled time inside an IN leaf, IS within dist
        sure = [rows[n][k] for k in mine for n in ("t_first_hi", "t_last_lo")]
        for chain in leaves.get(u, []):
            for a, b, is_in, h0, h5 in chain:
                if is_in:
                    sure += [a, b] + [float(x) for x in t[(t >= a) & (t <= b)]]
                else:
                    sure += ([a] if h0 <= dist else []) + ([b] if h5 <= dist else [])
        dn = W.nearest_at(pkg, st, scene["P"], 8, X, u, sure)
        assert np.all(dn <= dist + sl), (name, u, float(dn.max()))
        # a RESOLVED row's brackets hold the first and the last crossing of the level inside it, to the grid's step
        for k in mine:
            assert rows["flags"][k] & W.RESOLVED
            cs = [c for c in cross if rows["t_first_lo"][k] - step <= c <= rows["t_last_hi"][k] + step]
            assert len(cs) >= 2, (name, u, k, cross)
            assert rows["t_first_lo"][k] - step <= cs[0] <= rows["t_first_hi"][k] + step, (name, u, k, cs)
            assert rows["t_last_lo"][k] - step <= cs[-1] <= rows["t_last_hi"][k] + step, (name, u, k, cs)
            assert rows["t_first_hi"][k] - rows["t_first_lo"][k] <= tol and rows["t_last_hi"][k] - rows["t_last_lo"][k] <= tol


def test_truncation_keeps_the_last_completed_round(pkg, scenes):
    """max_windows = 1 and 2 on the cluster: TRUNCATED rows that still cover every sample within dist; a larger cap changes nothing once it does not bind"""
    scene, st, dist, ref, rows, _ = rows_of(pkg, scenes, "cluster")
    X = O.prims_of(scene)
    sl = O.slack(ref.S, st, X)
    t, d, _ = W.truth(pkg, st, scene["P"], 8, X, dist, N_GRID)[0]
    for mw in (1, 2):
        cut = ref.rows(dist, TOL, W.MAX_DEPTH, mw)
        assert np.any(cut["flags"] & W.TRUNCATED) and np.all(cut["depth"] < rows["depth"].max())
        inside = np.zeros(len(t), dtype=bool)
        for k in range(len(cut["robot"])):
            inside |= (t >= cut["t_first_lo"][k]) & (t <= cut["t_last_hi"][k])
        assert not np.any((d <= dist - sl) & ~inside)
    same = ref.rows(dist, TOL, W.MAX_DEPTH, W.MAX_WINDOWS)
    assert all(np.array_equal(same[n], rows[n]) for n in W.FIELDS)


def test_defaults_are_the_measured_ones(pkg):
    frontier, per = W.default_tolerance(pkg, R.prims())
    print("frontier", frontier, "per (state, dist): (rows, uncertain, truncated, largest live set, largest leaf list, largest depth, widest bracket)", per)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert W.default_tol(OFFSET, OFFSET, VEL) == 5e-4 == W.default_tol(math.inf, OFFSET, VEL)
    assert frontier == pkg.OBSWIN_FRONTIER == int(re.search(r"#define TJ_OBSWIN_FRONTIER\s+(\S+)", hdr).group(1))
    block = hdr[hdr.index("---- tj_obstacle_windows"):hdr.index("#define TJ_OBSWIN_CERTAIN")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    design = design[design.index("tj_obstacle_windows"):]
    assert len(per) == 16
    for (name, dist), v in per.items():
        pat = r"%s\s+%s\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\S+)\s*\n" % (re.escape(name), re.escape("%.1f" % dist))
        for where, txt in (("include/trajadmm.h", block), ("DESIGN.md", design)):
            m = re.search(pat, txt)
            assert m and tuple(int(m.group(i)) for i in range(1, 7)) == v[:6] and float(m.group(7)) == float("%.2e" % v[6]), (where, name, dist, v)
