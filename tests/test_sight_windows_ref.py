"""CPU (-m "not gpu"): the restatement tests/test_gpu_sight_windows.py holds the device to (tests/sight_windows_ref.py) is itself held to the flown link: closed
forms on the constructed states, and a truth that uses neither GJK nor subdivision (both ends from the quintics in np.longdouble on a dense grid, the segment
between them against every primitive by brute force) on the constructed states and on two golden states -- every sample outside all rows of a link is farther
than dist, every sure time and every sample inside an IN leaf IS within dist, within_lo does not exceed the sampled measure, a RESOLVED row's brackets hold the
first and the last crossing of the level.  Bars: 1e-12 on attained distances, the truth's grid step, obstacle_approach_ref.slack on the certified side and the
tolerance asked for -- nothing here is fitted to what the code returns.

Measured (tools/sight_windows_measure.py prints the header's two tables from default_tolerance; recorded in include/trajadmm.h and DESIGN.md 3n): over the three
multi-UAV end-to-end end states and their iteration-0 states at dist = 0.1 and 0.3 the largest live set of a segment is 8 windows and the largest leaf list 27 ->
TJ_SIGHT_FRONTIER = 128; no row is UNCERTAIN or TRUNCATED; with the clouds triangulated nothing changes from 3 projections on -> TJ_SIGHT_PROJECTIONS = 3.
test_defaults_are_the_measured_ones re-measures the e2e_scn_b rows of both tables (the e2e_scn_c3 cloud has five times the points: minutes per row) and
derives both constants from the tables as the header prints them."""
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import obstacle_approach_ref as O
import sight_windows_ref as W
from conftest import ROOT

OFFSET, MARGIN, VEL = 0.1, 0.1, 2.0
TOL = W.default_tol(OFFSET, OFFSET, VEL)
N_GRID = 4001


def rows_of(pkg, scenes, name):
    return W.built(pkg, scenes, R.prims(), name)


def one(rows, k=0):
    return {n: rows[n][k] for n in W.FIELDS}


def test_pillar_is_the_closed_form(pkg, scenes):
    """both ends at x = -5 + 2 t, the link spans y in [-1, 1], the point sits on its sweep: the distance is |x(t) - 1.3| = 2 |t - 3.15|, within 0.1 exactly over
    [3.10, 3.20] (the crossing itself is at 3.15).  One RESOLVED row, a chain across the boundary of a's segments 24 and 25 at 3.125."""
    scene, st, stations, links, dist, ref, rows, leaves = rows_of(pkg, scenes, "pillar")
    assert dist == OFFSET and TOL == 5e-4 and len(rows["link"]) == 1
    r = one(rows)
    assert r["t_first_lo"] <= 3.10 <= r["t_first_hi"] and r["t_last_lo"] <= 3.20 <= r["t_last_hi"]
    assert r["t_first_hi"] - r["t_first_lo"] <= TOL and r["t_last_hi"] - r["t_last_lo"] <= TOL
    assert r["flags"] == W.CERTAIN | W.RESOLVED and (r["link"], r["robot"], r["partner"], r["index"]) == (0, 0, 1, 0)
    assert all(b - a <= TOL for a, b, is_in, _, _ in leaves[0][0] if not is_in)
    edge = sum(b - a for a, b, is_in, _, _ in leaves[0][0] if not is_in)
    assert 0.1 - 2 * TOL - edge <= r["within_lo"] <= 0.1
    assert r["leaves"] == len(leaves[0][0]) and any(a == 3.125 for a, _, _, _, _ in leaves[0][0]) and any(b == 3.125 for _, b, _, _, _ in leaves[0][0])
    assert r["windows"] == sum(ref.search(0, 1, tr, dist, TOL, W.MAX_DEPTH, ref.frontier)["windows"] for tr in range(ref.S))


def test_graze(pkg, scenes):
    """the point dist + 1e-9 above the link's sweep: certified OUT everywhere, 0 rows; at dist - 1e-9: one row around the crossing at 3.15"""
    out, inn = rows_of(pkg, scenes, "graze_out")[6], rows_of(pkg, scenes, "graze_in")[6]
    assert all(len(out[n]) == 0 for n in W.FIELDS)
    assert len(inn["link"]) == 1 and inn["t_first_lo"][0] <= 3.15 <= inn["t_last_hi"][0] and inn["t_last_hi"][0] - inn["t_first_lo"][0] <= 2 * TOL
    assert 0.1 - 1e-9 - 1e-12 <= inn["closest"][0] <= 0.1 + 1e-6


def test_station_far_from_both_ends(pkg, scenes):
    """one UAV along x at speed 2, the station 10 up in y, the point at lambda = 0.37 of the link at t = 2.5: a point of the link at lambda is at (0.63 x, 3.7 + ..),
    so the row is centred on 2.5 and about 0.1 / 0.63 / 2 * 2 = 0.159 s long; the fixed-lambda IN test certifies its inside"""
    scene, st, stations, links, dist, ref, rows, leaves = rows_of(pkg, scenes, "station")
    assert links == [(0, -1)] and len(rows["link"]) == 1
    r = one(rows)
    assert r["flags"] == W.CERTAIN | W.RESOLVED and (r["robot"], r["partner"], r["index"]) == (0, -1, 77)
    half = 0.5 * (r["t_last_hi"] - r["t_first_lo"])
    assert abs(0.5 * (r["t_first_lo"] + r["t_last_hi"]) - 2.5) <= TOL and abs(half - 0.1 / 0.63 / 2.0) <= 2e-3
    assert r["within_lo"] >= 2 * half - 4 * TOL and r["closest"] <= 1e-12 and r["closest_time"] == 2.5


def test_hover_and_staggered(pkg, scenes):
    """hover: b arrives at t = 3.15 and the row goes on across its arrival cut; staggered: b's segment cuts fall inside the row"""
    scene, st, stations, links, dist, ref, rows, leaves = rows_of(pkg, scenes, "hover")
    assert len(rows["link"]) == 1 and rows["flags"][0] == W.CERTAIN | W.RESOLVED
    arrive = (ref.S / ref.rf) * float(st["piece_time"][1])
    assert abs(arrive - 3.15) < 1e-12 and rows["t_first_hi"][0] < arrive < rows["t_last_lo"][0]
    assert any(b == arrive for _, b, _, _, _ in leaves[0][0]) and any(a == arrive for a, _, _, _, _ in leaves[0][0])
    scene, st, stations, links, dist, ref, rows, leaves = rows_of(pkg, scenes, "staggered")
    assert len(rows["link"]) == 1 and rows["flags"][0] == W.CERTAIN | W.RESOLVED
    cuts = [(j / ref.rf) * float(st["piece_time"][1]) for j in range(ref.S + 1)]
    inside = [c for c in cuts if rows["t_first_lo"][0] < c < rows["t_last_hi"][0]]
    assert inside and all(any(a == c for a, _, _, _, _ in leaves[0][0]) for c in inside)
    assert all(c not in [(j / ref.rf) * float(st["piece_time"][0]) for j in range(ref.S + 1)] for c in inside)   # b's own cuts, not a's segment ends


def test_cluster_has_more_candidates_than_a_wave(pkg, scenes):
    scene, st, stations, links, dist, ref, rows, leaves = rows_of(pkg, scenes, "cluster")
    assert len(rows["link"]) == 1 and rows["flags"][0] == W.CERTAIN | W.RESOLVED
    assert np.sum(np.linalg.norm(scene["cloud"] - np.array([1.3, 0.0, 0.0]), axis=1) <= 0.05) == 150


def test_a_segment_with_a_second_block_of_leaves(pkg, scenes):
    scene, st, dist = W.many_leaves_state(pkg, scenes)
    ref = W.ref_of(pkg, R.prims(), st, scene["P"], 8, O.prims_of(scene))
    found = ref.search(0, 1, 25, dist, 0.0, 40, ref.frontier)
    lv = found["leaves"]
    heads = [k for k in range(1, len(lv)) if lv[k - 1][1] != lv[k][0]]
    assert len(lv) > 64 and lv[63][1] == lv[64][0] and any(k > 64 for k in heads) and not found["truncated"], (len(lv), heads)


def test_truncation_keeps_the_last_completed_round(pkg, scenes):
    scene, st, stations, links, dist, ref, rows, _ = rows_of(pkg, scenes, "cluster")
    for mw in (1, 2):
        cut = ref.rows(links, dist, TOL, W.MAX_DEPTH, mw)
        assert np.any(cut["flags"] & W.TRUNCATED) and np.all(cut["depth"] < rows["depth"].max())
        assert cut["t_first_lo"].min() <= rows["t_first_lo"][0] and cut["t_last_hi"].max() >= rows["t_last_hi"][0]
    same = ref.rows(links, dist, TOL, W.MAX_DEPTH, W.MAX_WINDOWS)
    assert all(np.array_equal(same[n], rows[n]) for n in W.FIELDS)


def sound(pkg, st, P, res, X, stations, links, dist, tol, rows, leaves, n_grid, need_rows=True):
    sl = O.slack(P * res, st, X)
    assert not need_rows or len(rows["link"]) > 0
    for k, ((a, b), (t, d, cross)) in enumerate(zip(links, W.truth(pkg, st, P, res, X, stations, links, dist, n_grid))):
        step = float(t[1] - t[0])
        mine = np.flatnonzero(rows["link"] == k)
        # every sampled time outside all rows of the link is farther than dist (the grid's last sample is P * piece_time in np.longdouble, the row's end
        # (S / res) * piece_time in a double: 1e-12 s, in which no end moves 1e-11, keeps the two on one side)
        inside = np.zeros(len(t), dtype=bool)
        for i in mine:
            inside |= (t >= rows["t_first_lo"][i] - 1e-12) & (t <= rows["t_last_hi"][i] + 1e-12)
        assert not np.any((d <= dist - sl) & ~inside), (k, t[(d <= dist - sl) & ~inside])
        # the sure times of CERTAIN rows, and every sampled time inside an IN leaf, ARE within dist
        sure = [rows[n][i] for i in mine for n in ("t_first_hi", "t_last_lo") if rows["flags"][i] & W.CERTAIN]
        for chain in leaves.get(k, []):
            for ca, cb, is_in, h0, h5 in chain:
                if is_in:
                    sure += [ca, cb] + [float(x) for x in t[(t >= ca) & (t <= cb)]]
        dn = W.nearest_at(pkg, st, P, res, X, stations, a, b, sure)
        assert np.all(dn <= dist + 1e-12), (k, float(dn.max()) - dist)
        for i in mine:
            # within_lo does not exceed the sampled measure plus one grid step
            row_in = (t >= rows["t_first_lo"][i]) & (t <= rows["t_last_hi"][i]) & (d <= dist + 1e-12)
            assert rows["within_lo"][i] <= step * int(np.sum(row_in)) + step, (k, i)
            # a RESOLVED row's brackets hold the first and the last crossing of the level inside it, to the grid's step
            if rows["flags"][i] & W.RESOLVED:
                cs = [c for c in cross if rows["t_first_lo"][i] - step <= c <= rows["t_last_hi"][i] + step]
                if not rows["flags"][i] & W.AT_START:
                    assert cs and rows["t_first_lo"][i] - step <= cs[0] <= rows["t_first_hi"][i] + step, (k, i, cs)
                    assert rows["t_first_hi"][i] - rows["t_first_lo"][i] <= tol
                if not rows["flags"][i] & W.AT_END:
                    assert cs and rows["t_last_lo"][i] - step <= cs[-1] <= rows["t_last_hi"][i] + step, (k, i, cs)
                    assert rows["t_last_hi"][i] - rows["t_last_lo"][i] <= tol


@pytest.mark.parametrize("name", W.STATES)
def test_rows_are_sound_against_the_flown_link(pkg, scenes, name):
    scene, st, stations, links, dist, ref, rows, leaves = rows_of(pkg, scenes, name)
    sound(pkg, st, scene["P"], 8, O.prims_of(scene), stations, links, dist, TOL, rows, leaves, N_GRID, need_rows=name != "graze_out")


@pytest.mark.parametrize("name", ["e2e_scn_b", "e2e_scn_b_coupled"])
def test_golden_states_are_sound(pkg, name):
    """the end state of a committed run over every sixth point of its cropped cloud: a robot pair and a station link at dist = offset + 2 * margin"""
    for label, st, P, res, X, station in W.measure_states(pkg):
        if label != name:
            continue
        X, stations, links, dist = np.ascontiguousarray(X[::6]), station[None, :], [(0, 1), (1, -1)], OFFSET + 2 * MARGIN
        tol = W.default_tol(dist, OFFSET, VEL)
        ref = W.ref_of(pkg, R.prims(), st, P, res, X, stations)
        leaves = {}
        rows = ref.rows(links, dist, tol, leaves=leaves)
        assert not np.any(rows["flags"] & W.TRUNCATED)
        sound(pkg, st, P, res, X, stations, links, dist, tol, rows, leaves, 2001)


def test_truth_on_triangles_is_the_segment_distance():
    """link_dist against closed forms: a link piercing a triangle, one parallel above it, one nearest to an edge, one nearest with an end"""
    tri = np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0]]])
    x = np.array([[0.5, 0.5, -1.0], [0.2, 0.2, 0.7], [3.0, 3.0, 0.0], [0.5, 0.5, 3.0]], dtype=W.LD)
    y = np.array([[0.5, 0.5, 1.0], [0.6, 0.3, 0.7], [3.0, 3.0, 5.0], [0.5, 0.5, 0.25]], dtype=W.LD)
    d = W.link_dist(x, y, tri)[:, 0]
    assert np.allclose(np.asarray(d, dtype=np.float64), [0.0, 0.7, math.sqrt(8.0), 0.25], atol=1e-15)


def _table(txt, pat):
    return re.search(pat, txt)


def test_defaults_are_the_measured_ones(pkg):
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    block = hdr[hdr.index("---- tj_sight_windows"):hdr.index("#define TJ_SIGHT_CERTAIN")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    design = design[design.index("### 3n"):]
    assert W.default_tol(OFFSET, OFFSET, VEL) == 5e-4 == W.default_tol(math.inf, OFFSET, VEL)
    # the constants follow from the tables as printed
    cloud = re.findall(r"\n \*   (e2e_\w+)\s+(0\.\d)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\S+)", block)
    tri = re.findall(r"\n \*   (e2e_\w+)\s+(0\.\d)((?:\s+\d+/\d+/\d+){6})", block)
    assert len(cloud) == 12 and len(tri) == 12
    assert all(int(r[4]) == 0 for r in cloud)                                                # no measurement state is TRUNCATED at the defaults
    per_k = {K: [r[2].split()[K - 1] for r in tri] for K in range(1, 7)}
    K0 = min(K for K in range(1, 5) if per_k[K] == per_k[K + 1] == per_k[K + 2])
    widest = max([int(r[5]) for r in cloud] + [int(r[6]) for r in cloud] + [int(c.split("/")[2]) for c in per_k[K0]])
    assert K0 == pkg.SIGHT_PROJECTIONS and W.frontier_of(widest) == pkg.SIGHT_FRONTIER
    # and the e2e_scn_b rows of both tables are what the restatement measures now
    pr = R.prims()
    for label, st, P, res, X, station in W.measure_states(pkg):
        if label not in ("e2e_scn_b", "e2e_scn_b_init"):
            continue
        ref = W.ref_of(pkg, pr, st, P, res, X, station[None, :], frontier=W.MAX_WINDOWS)
        mesh = W.ref_of(pkg, pr, st, P, res, W.as_triangles(X), station[None, :], frontier=W.MAX_WINDOWS)
        for dist in (OFFSET, OFFSET + 2 * MARGIN):
            v = W.measure(ref, dist, pkg.SIGHT_PROJECTIONS)
            print(label, dist, v)
            pat = r"%s\s+%s\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\S+)\s*\n" % (re.escape(label), re.escape("%.1f" % dist))
            for where, txt in (("include/trajadmm.h", block), ("DESIGN.md", design)):
                m = re.search(pat, txt)
                assert m and tuple(int(m.group(i)) for i in range(1, 7)) == v[:6] and float(m.group(7)) == float("%.2e" % v[6]), (where, label, dist, v)
            w = W.measure(mesh, dist, pkg.SIGHT_PROJECTIONS)
            row = [r for r in tri if r[0] == label and r[1] == "%.1f" % dist][0][2].split()
            assert row[pkg.SIGHT_PROJECTIONS - 1] == "%d/%d/%d" % (w[0], w[1], w[4]), (label, dist, w, row)
