"""CPU (-m "not gpu"): the restatement of tj_zone_windows (tests/zone_windows_ref.py) against the truth -- per segment the real roots in [0, 1] of each face's
quintic f_j(x(s)) - level and of the degree-10 |x(s) - c|^2 - (r + level)^2 in mpmath, the true set of times within the level -- on e2e_scn_a, e2e_scn_b and tiny()'s
initial states at the measurement's zones; against closed forms on a straight flight at constant speed; and the header's measured table and constants against a
re-measurement.

The margin of the truth assertions: the largest excess by which the truth contradicts a certified class was measured (tools/zone_windows_measure.py --all) at
0.283 eps (eps = 2^-53) of the slot's scale, inside an IN leaf of e2e_scn_c3, and at 0 on every other state; no truly-within time lay outside a row.  MARGIN is
the next power of two >= 16 x that."""
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import zone_windows_ref as Z
from conftest import ROOT

MEASURED_EXCESS = 0.283
MARGIN = 8
TOL = Z.default_tol(0.1, 2.0)
SMALL = ("e2e_scn_a", "e2e_scn_b")


def test_the_margin_follows_from_the_measurement():
    assert MARGIN == Z.next_pow2(math.ceil(16 * MEASURED_EXCESS)) and TOL == 0.0005


def _states(pkg, scenes):
    out = {n: T.e2e_state(n) for n in SMALL}
    for m in (0, 1, 2):
        scene = scenes.tiny(mode=m)
        out["tiny_mode%d" % m] = (R.port_state(scene, 0), scene["P"], 8)
    return out


def assert_against_truth(ref, u, k, zone, inside=None, tol=TOL, max_depth=Z.MAX_DEPTH, max_windows=Z.MAX_WINDOWS):
    """(a) coverage, (b) IN leaves, (c) the sure times, (d) tiling of the rows of (robot u, zone); returns (rows, chains, contradiction of coverage, of IN leaves) in eps"""
    import mpmath as mp
    kind, sense, level, _ = zone
    leaves = {}
    rows = ref.zone_rows(u, k, zone, tol, max_depth, max_windows, None, leaves)
    chains = leaves.get((u, k), [])
    truth = Z.true_within(ref, u, zone, inside)
    scale = ref.scale(u, zone)
    # (a), (b): no truly-within time outside the rows, no truly-outside time inside an IN leaf, beyond the margin
    cov, inn = Z.contradictions(ref, u, zone, chains, truth)
    print("robot %d zone %d: coverage %.3g eps, IN leaves %.3g eps" % (u, k, cov / Z.EPS, inn / Z.EPS))
    assert cov <= MARGIN * Z.EPS and inn <= MARGIN * Z.EPS, (u, k, cov / Z.EPS, inn / Z.EPS)
    # (d): the leaves of a chain touch on doubles, chains are maximal and disjoint, within_lo is the IN sum
    assert len(rows) == len(chains)
    sigma = 1.0 if sense == Z.INSIDE else -1.0
    for i, (row, chain) in enumerate(zip(rows, chains)):
        assert all(chain[j][1] == chain[j + 1][0] for j in range(len(chain) - 1)) and all(lf[0] < lf[1] for lf in chain)
        if i:
            assert chains[i - 1][-1][1] < chain[0][0]
        within = 0.0
        for ga, gb, is_in, _, _ in chain:
            if is_in:
                within += ((gb - ga) / ref.rf) * float(ref.pt[u])
        assert row["within_lo"] == within and row["leaves"] == len(chain)
        assert row["t_first_lo"] == ref.time_g(u, chain[0][0]) and row["t_last_hi"] == ref.time_g(u, chain[-1][1])
        # (c): the truth is within the level at the sure times t_first_hi and t_last_lo (each a leaf's end, in that leaf's segment), up to the margin
        if row["flags"] & Z.CERTAIN:
            sure = []
            for ga, gb, is_in, g0, g5 in chain:
                if is_in or sigma * g0 <= sigma * level:
                    sure.append((ga, int(ga)))
                if is_in or sigma * g5 <= sigma * level:
                    sure.append((gb, int(ga)))
            assert ref.time_g(u, sure[0][0]) == row["t_first_hi"] and ref.time_g(u, sure[-1][0]) == row["t_last_lo"]
            for g, tr in (sure[0], sure[-1]):
                v = Z.gauge_at(ref, u, zone, mp.mpf(g), tr)
                assert sigma * (v - mp.mpf(float(level))) <= MARGIN * Z.EPS * scale, (u, k, g, float(v))
    return rows, chains, cov / Z.EPS, inn / Z.EPS


@pytest.mark.parametrize("name", SMALL + ("tiny_mode0", "tiny_mode1", "tiny_mode2"))
def test_restatement_against_the_true_roots(pkg, scenes, name):
    """every robot of the state at the 20 measurement zones, the default tol: coverage, IN leaves, sure times, tiling; every figure is printed before it is
    asserted.  And union / complement consistency at level 0: where an IN leaf of a zone's INSIDE rows overlaps an IN leaf of its OUTSIDE rows the gauge is
    certified both <= 0 and >= 0, so it is 0 there up to the margin"""
    import mpmath as mp
    st, Pn, res = _states(pkg, scenes)[name]
    ref = Z.Ref(pkg, st, Pn, res)
    zones = Z.measurement_zones(ref)
    assert len(zones) == 20 and max(len(z[3]) for z in zones) == Z.MAX_PLANES
    n_rows, worst, overlaps = 0, 0.0, 0
    for u in range(ref.U):
        inside, ins = {}, {}
        for k, zone in enumerate(zones):
            key = (k // 4, zone[2])
            if key not in inside:
                inside[key] = Z.true_inside(ref, u, zone)
            rows, chains, cov, inn = assert_against_truth(ref, u, k, zone, inside[key])
            n_rows += len(rows)
            worst = max(worst, cov, inn)
            ins[k] = [(mp.mpf(lf[0]), mp.mpf(lf[1])) for c in chains for lf in c if lf[2]]
        for shape in range(5):
            k_in, k_out = 4 * shape, 4 * shape + 2                                           # (INSIDE, 0) and (OUTSIDE, 0) of the shape
            assert zones[k_in][1:3] == (Z.INSIDE, 0.0) and zones[k_out][1:3] == (Z.OUTSIDE, 0.0)
            both = Z.W._minus(ins[k_in], Z.W._minus(ins[k_in], ins[k_out]))                  # the intersection
            for lo, hi in both:
                overlaps += 1
                for tr in range(int(mp.floor(lo)), min(int(mp.ceil(hi)), ref.S)):
                    a, b = max(lo, mp.mpf(tr)), min(hi, mp.mpf(tr + 1))
                    for j in range(9):
                        v = abs(Z.gauge_at(ref, u, zones[k_in], a + (b - a) * j / 8, tr))
                        assert v <= MARGIN * Z.EPS * ref.scale(u, zones[k_in]), (u, shape, float(lo), float(hi), float(v))
    print("%s: rows %d, largest contradiction %.3g eps, certified-both overlaps %d" % (name, n_rows, worst, overlaps))
    assert n_rows > 0


def test_depth_stop_and_truncation_keep_the_coverage(pkg, scenes):
    """tol = 0 with max_depth = 3, and max_windows = 1: EDGE leaves and truncated searches still cover every truly-within time"""
    st, Pn, res = _states(pkg, scenes)["e2e_scn_b"]
    ref = Z.Ref(pkg, st, Pn, res)
    seen = 0
    for u in range(2):
        for k, zone in enumerate(Z.measurement_zones(ref)):
            inside = Z.true_inside(ref, u, zone)
            assert_against_truth(ref, u, k, zone, inside, 0.0, 3)
            rows = assert_against_truth(ref, u, k, zone, inside, TOL, Z.MAX_DEPTH, 1)[0]
            seen += sum(1 for r in rows if r["flags"] & Z.TRUNCATED)
    assert seen > 0


def _line(pkg, scenes):
    """peak_dynamics_ref.line_state: x = 5 sigma along the x axis, y = z = 0, every hull point exact: position is linear in time, x0 = 0, v = 5 / piece_time"""
    scene, st = Z.line_state(pkg, scenes)
    ref = Z.Ref(pkg, st, scene["P"], 8)
    assert not ref.H[0][:, :, 1:].any() and ref.H[0][0][0][0] == 0.0 and ref.H[0][-1][5][0] == 5.0 * scene["P"]
    return ref, 5.0 / float(ref.pt[0]), float(scene["P"]) * float(ref.pt[0])


def test_a_straight_flight_enters_and_leaves_a_slab_where_the_closed_form_says(pkg, scenes):
    ref, v, dur = _line(pkg, scenes)
    a, b = 3.3, 11.7
    slab = np.array([[-1.0, 0.0, 0.0, -a], [1.0, 0.0, 0.0, b]])
    t_in, t_out = a / v, b / v
    r = ref.rows([(Z.PLANES, Z.INSIDE, 0.0, slab)], TOL)
    assert len(r["robot"]) == 1 and r["flags"][0] == Z.CERTAIN | Z.RESOLVED
    assert r["t_first_lo"][0] <= t_in <= r["t_first_hi"][0] and r["t_last_lo"][0] <= t_out <= r["t_last_hi"][0]
    assert r["t_first_hi"][0] - r["t_first_lo"][0] <= TOL and r["t_last_hi"][0] - r["t_last_lo"][0] <= TOL
    assert abs(r["within_lo"][0] - (t_out - t_in)) <= 2 * TOL
    assert r["extreme"][0] < -0.5 * (b - a) + 5.0 / 8 and r["face"][0] in (0, 1)             # the deepest end sample: near the slab's middle, a segment's end
    o = ref.rows([(Z.PLANES, Z.OUTSIDE, 0.0, slab)], TOL)
    assert list(o["flags"]) == [Z.CERTAIN | Z.RESOLVED | Z.AT_START, Z.CERTAIN | Z.RESOLVED | Z.AT_END] and list(o["face"]) == [0, 1]
    assert o["t_first_lo"][0] == 0.0 and o["t_last_lo"][0] <= t_in <= o["t_last_hi"][0] and o["t_last_hi"][0] - o["t_last_lo"][0] <= TOL
    assert o["t_first_lo"][1] <= t_out <= o["t_first_hi"][1] and o["t_first_hi"][1] - o["t_first_lo"][1] <= TOL and o["t_last_hi"][1] == ref.time_g(0, float(ref.S))
    assert abs(o["within_lo"][0] - t_in) <= 2 * TOL and abs(o["within_lo"][1] - (dur - t_out)) <= 2 * TOL
    assert o["extreme"][0] == a and o["extreme_time"][0] == 0.0 and o["extreme"][1] == 25.0 - b    # the farthest end samples: the start and the goal
    # the margin: inside with 0.4 to spare is the slab shrunk by 0.4
    m = ref.rows([(Z.PLANES, Z.INSIDE, -0.4, slab)], TOL)
    assert len(m["robot"]) == 1 and m["t_first_lo"][0] <= (a + 0.4) / v <= m["t_first_hi"][0] and m["t_last_lo"][0] <= (b - 0.4) / v <= m["t_last_hi"][0]


def test_a_straight_flight_crosses_a_ball_centred_on_it_along_the_chord(pkg, scenes):
    ref, v, dur = _line(pkg, scenes)
    c, rad = 12.3, 4.1
    ball = np.array([[c, 0.0, 0.0, rad]])
    r = ref.rows([(Z.BALL, Z.INSIDE, 0.0, ball), (Z.BALL, Z.OUTSIDE, 0.0, ball)], TOL)
    assert list(r["zone"]) == [0, 1, 1] and np.all(r["face"] == -1) and np.all(r["flags"] & (Z.CERTAIN | Z.RESOLVED) == Z.CERTAIN | Z.RESOLVED)
    t_in, t_out = (c - rad) / v, (c + rad) / v
    assert r["t_first_lo"][0] <= t_in <= r["t_first_hi"][0] <= r["t_first_lo"][0] + TOL and r["t_last_lo"][0] <= t_out <= r["t_last_hi"][0] <= r["t_last_lo"][0] + TOL
    assert abs(r["within_lo"][0] - (t_out - t_in)) <= 2 * TOL
    assert r["t_last_lo"][1] <= t_in <= r["t_last_hi"][1] and r["t_first_lo"][2] <= t_out <= r["t_first_hi"][2]
    assert r["flags"][1] & Z.AT_START and r["flags"][2] & Z.AT_END


def test_the_whole_flight_and_nothing(pkg, scenes):
    st, Pn, res = _states(pkg, scenes)["tiny_mode1"]
    ref = Z.Ref(pkg, st, Pn, res)
    pts = ref.H.reshape(-1, 3)
    box = Z.box_rows(pts.min(axis=0) - 1.0, pts.max(axis=0) + 1.0)
    a = ref.rows([(Z.PLANES, Z.INSIDE, 0.0, box), (Z.PLANES, Z.OUTSIDE, 0.0, box), (Z.BALL, Z.INSIDE, 0.0, np.array([[0.0, 0.0, 0.0, 1e3]])), (Z.BALL, Z.INSIDE, -2e3, np.array([[0.0, 0.0, 0.0, 1e3]]))], TOL)
    assert sorted(zip(a["robot"], a["zone"])) == list(zip(a["robot"], a["zone"])) == [(u, k) for u in range(ref.U) for k in (0, 2)]
    assert np.all(a["flags"] == Z.CERTAIN | Z.AT_START | Z.AT_END | Z.RESOLVED) and np.all(a["windows"] == ref.S) and np.all(a["depth"] == 0)
    b = ref.rows(Z.measurement_zones(ref), TOL)
    key = list(zip(b["robot"], b["zone"], b["t_first_lo"]))
    assert key == sorted(key) and len(key) > 0


def test_depth_zero_net_is_the_raw_hull(pkg, scenes):
    """at [0, 1] the net is the raw hull bit for bit: a one-face zone's depth-0 bounds are the extremes of dot3(n, hull point) - d"""
    st, Pn, res = _states(pkg, scenes)["tiny_mode1"]
    ref = Z.Ref(pkg, st, Pn, res)
    tr = np.arange(ref.S)
    n = np.array([[0.6, 0.0, 0.8, 0.25]])
    for u in range(ref.U):
        ub, lb, g0, g5 = ref.bounds(u, (Z.PLANES, Z.INSIDE, 0.0, n), tr, np.zeros(ref.S), np.ones(ref.S))
        f = (0.6 * ref.H[u][:, :, 0] + 0.0 * ref.H[u][:, :, 1]) + 0.8 * ref.H[u][:, :, 2] - 0.25
        assert np.array_equal(ub, f.max(axis=1)) and np.array_equal(lb, f.min(axis=1)) and np.array_equal(g0, f[:, 0]) and np.array_equal(g5, f[:, 5])


def test_the_headers_table_and_frontier(pkg):
    """the e2e_scn_a and e2e_scn_b rows of the header's table are re-measured; TJ_ZONEWIN_FRONTIER is the next power of two >= 4 x the table's largest live set, at
    least 64; the header states the measured excess and the margin"""
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    block = hdr[hdr.index("tj_zone_windows: FROM WHEN TO WHEN"):hdr.index("#define TJ_ZONE_PLANES")]
    table = {m.group(1): tuple(int(x) for x in m.group(2).split()) + (float(m.group(3)),)
             for m in re.finditer(r"^ \*   (e2e_\w+)\s+((?:\d+\s+){6})(\d\.\d\de[-+]\d\d)$", block, flags=re.M)}
    assert len(table) == 8
    frontier, per = Z.default_tolerance(pkg, names=[e for e in Z.E2E if e[0] in SMALL])
    assert len(per) == 4
    for label, v in per.items():
        assert table[label][:6] == v[:6] and "%.2e" % v[6] == "%.2e" % table[label][6], (label, v, table[label])
    assert not any(v[2] for v in table.values())                                             # no measurement state is TRUNCATED
    assert pkg.ZONEWIN_FRONTIER == max(64, Z.next_pow2(4 * max(v[3] for v in table.values()))) == 512
    assert int(re.search(r"#define TJ_ZONEWIN_FRONTIER\s+(\d+)", hdr).group(1)) == pkg.ZONEWIN_FRONTIER
    assert "%.3g eps" % MEASURED_EXCESS in block and "%d eps" % MARGIN in block
