"""CPU (-m "not gpu"): the restatement of tj_dynamics_windows (tests/dynamics_windows_ref.py) against the truth -- per segment the real roots in [0, 1] of
|q(s)|^2 - (level den)^2 in mpmath, the true set of times within the level -- on the four end states and tiny()'s initial states at the measurement's gates; against
closed forms; and the header's measured table and constants against a re-measurement.

The margin of the truth assertions: the largest excess by which the truth contradicts a certified class was measured at 1.54 eps (eps = 2^-53) of the robot's
depth-0 ub, inside an IN leaf; no truly-within time lay outside a row.  MARGIN is the next power of two >= 16 x that."""
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import dynamics_windows_ref as W
from conftest import ROOT

MEASURED_EXCESS = 1.54
MARGIN = 32
TOL = W.default_tol(2.0, 2.0)


def test_the_margin_follows_from_the_measurement():
    assert MARGIN == W.next_pow2(math.ceil(16 * MEASURED_EXCESS)) and TOL == 0.01


def _states(pkg, scenes):
    out = {n: T.e2e_state(n) for n, _ in W.E2E}
    for m in (0, 1, 2):
        scene = scenes.tiny(mode=m)
        out["tiny_mode%d" % m] = (R.port_state(scene, 0), scene["P"], 8)
    return out


def assert_against_truth(ref, u, k, gate, tol=TOL, max_depth=W.MAX_DEPTH, max_windows=W.MAX_WINDOWS):
    """(a) coverage, (b) IN leaves, (c) brackets, (d) tiling of the rows of (robot u, gate); returns (rows, contradiction of coverage, of IN leaves) in eps"""
    import mpmath as mp
    q, sense, level = gate
    leaves = {}
    rows = ref.gate_rows(u, k, gate, tol, max_depth, max_windows, None, leaves)
    chains = leaves.get((u, k), [])
    truth = W.true_within(ref, u, gate)
    ub0 = ref.ub0(u, q)
    # (a), (b): no truly-within time outside the rows, no truly-outside time inside an IN leaf, beyond the margin
    cov, inn = W.contradictions(ref, u, gate, chains, truth)
    assert cov <= MARGIN * W.EPS and inn <= MARGIN * W.EPS, (u, gate, cov / W.EPS, inn / W.EPS)
    # (d): the leaves of a chain touch on doubles, chains are maximal and disjoint, within_lo is the IN sum
    assert len(rows) == len(chains)
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
        # (c): on CERTAIN | RESOLVED rows the brackets contain the first and the last true crossing inside the row.  The row starts at t_first_lo and ends at
        # t_last_hi, so that is: the truth is within at the sure times t_first_hi and t_last_lo (each a leaf's end, in that leaf's segment), up to the margin
        if row["flags"] & W.CERTAIN and row["flags"] & W.RESOLVED:
            sigma = -1.0 if sense == W.ABOVE else 1.0
            sure = []
            for ga, gb, is_in, h0, h5 in chain:
                if is_in or sigma * h0 <= sigma * level:
                    sure.append((ga, int(ga)))
                if is_in or sigma * h5 <= sigma * level:
                    sure.append((gb, int(ga)))
            assert ref.time_g(u, sure[0][0]) == row["t_first_hi"] and ref.time_g(u, sure[-1][0]) == row["t_last_lo"]
            inside = [(max(a, mp.mpf(chain[0][0])), min(b, mp.mpf(chain[-1][1]))) for a, b in truth if b >= chain[0][0] and a <= chain[-1][1]]
            for first, (g, tr), crossing in ((True, sure[0], inside[0][0] if inside else None), (False, sure[-1], inside[-1][1] if inside else None)):
                v = W.value_at(ref, u, q, mp.mpf(g), tr)
                near = abs(v - mp.mpf(float(level))) <= MARGIN * W.EPS * ub0
                assert near or (v >= level if sense == W.ABOVE else v <= level), (u, gate, g, float(v))
                if not near:
                    assert crossing is not None and (crossing <= g if first else crossing >= g), (u, gate, g, crossing)
    return rows, cov / W.EPS, inn / W.EPS


@pytest.mark.parametrize("name", [n for n, _ in W.E2E] + ["tiny_mode0", "tiny_mode1", "tiny_mode2"])
def test_restatement_against_the_true_roots(pkg, scenes, name):
    """every robot of the state at the 18 measurement gates, the default tol: coverage, IN leaves, brackets, tiling; the largest contradiction is printed"""
    st, Pn, res = _states(pkg, scenes)[name]
    ref = W.Ref(pkg, st, Pn, res)
    gates = W.measurement_gates(ref)
    assert len(gates) == 18
    n_rows, worst = 0, 0.0
    for u in range(ref.U):
        for k, gate in enumerate(gates):
            rows, cov, inn = assert_against_truth(ref, u, k, gate)
            n_rows += len(rows)
            worst = max(worst, cov, inn)
    print("%s: rows %d, largest contradiction %.3g eps" % (name, n_rows, worst))
    assert n_rows > 0


def test_depth_stop_and_truncation_keep_the_coverage(pkg, scenes):
    """tol = 0 with max_depth = 3, and max_windows = 1: EDGE leaves and truncated searches still cover every truly-within time"""
    st, Pn, res = _states(pkg, scenes)["e2e_scn_b"]
    ref = W.Ref(pkg, st, Pn, res)
    seen = 0
    for u in range(4):
        for k, gate in enumerate(W.measurement_gates(ref)):
            assert_against_truth(ref, u, k, gate, 0.0, 3)
            rows, _, _ = assert_against_truth(ref, u, k, gate, TOL, W.MAX_DEPTH, 1)
            seen += sum(1 for r in rows if r["flags"] & W.TRUNCATED)
    assert seen > 0


def test_hover_is_below_any_positive_level(pkg, scenes):
    scene, st = W.hover_state(pkg, scenes)
    ref = W.Ref(pkg, st, scene["P"], 8)
    a = ref.rows([(W.SPEED, W.BELOW, 0.1), (W.SPEED, W.ABOVE, 0.1), (W.ACCEL, W.BELOW, 0.0)], TOL)
    whole = W.CERTAIN | W.AT_START | W.AT_END | W.RESOLVED
    assert list(a["gate"]) == [0, 2] and list(a["flags"]) == [whole, whole] and list(a["robot"]) == [0, 0]
    dur = 0.0
    for _ in range(ref.S):
        dur += ((1.0 - 0.0) / 8.0) * float(ref.pt[0])
    assert a["within_lo"][0] == dur and abs(dur - ref.duration(0)) <= 1e-12 * dur and a["t_last_hi"][0] == ref.time_g(0, float(ref.S))
    assert a["extreme"][0] == 0.0 and a["extreme_time"][0] == 0.0 and a["leaves"][0] == ref.S and a["windows"][0] == ref.S and a["depth"][0] == 0


def test_line_is_above_three_quarters_of_its_speed_and_below_five_quarters(pkg, scenes):
    scene, st = W.line_state(pkg, scenes)
    ref = W.Ref(pkg, st, scene["P"], 8)
    v = W.line_speed(pkg, st, scene["P"])
    a = ref.rows([(W.SPEED, W.ABOVE, 0.75 * v), (W.SPEED, W.ABOVE, 1.25 * v), (W.SPEED, W.BELOW, 1.25 * v), (W.SPEED, W.BELOW, 0.75 * v)], TOL)
    whole = W.CERTAIN | W.AT_START | W.AT_END | W.RESOLVED
    assert list(a["gate"]) == [0, 2] and list(a["flags"]) == [whole, whole] and np.all(a["leaves"] == ref.S) and np.all(a["extreme"] == v)
    assert np.all(a["t_first_lo"] == 0.0) and np.all(a["t_last_hi"] == ref.time_g(0, float(ref.S))) and np.all(a["depth"] == 0)
    for gate in ((W.SPEED, W.ABOVE, v), (W.SPEED, W.BELOW, v)):                             # stated limit (2): equal to the level over the flight: no error
        b = ref.rows([gate], TOL)
        assert len(b["robot"]) <= ref.S


def test_uniform_acceleration_crosses_the_level_where_the_closed_form_says(pkg, scenes):
    """x = c sigma^2 at piece_time 1: speed 2 c t.  The solved control net is not dyadic (dynamics_windows_ref.accel_state), so the closed form holds to 1e-9 and
    the mpmath root is the truth: both are asserted.  ABOVE at 2.3 (c = 0.5): one row from t = 2.3 to the end; BELOW: one row from the start to t = 2.3"""
    scene, st, c = W.accel_state(pkg, scenes)
    ref = W.Ref(pkg, st, scene["P"], 8)
    level, dur = 2.3, float(scene["P"])
    t_cross = level / (2 * c)
    assert 0 < t_cross < dur
    for k, (sense, first, last) in enumerate(((W.ABOVE, t_cross, dur), (W.BELOW, 0.0, t_cross))):
        gate = (W.SPEED, sense, level)
        rows, _, _ = assert_against_truth(ref, 0, 0, gate)
        assert len(rows) == 1
        r = rows[0]
        assert r["flags"] == W.CERTAIN | W.RESOLVED | (W.AT_END if sense == W.ABOVE else W.AT_START)
        assert r["t_first_lo"] - 1e-9 <= first <= r["t_first_hi"] + 1e-9 and r["t_last_lo"] - 1e-9 <= last <= r["t_last_hi"] + 1e-9
        assert r["t_first_hi"] - r["t_first_lo"] <= TOL and r["t_last_hi"] - r["t_last_lo"] <= TOL
        truth = W.true_within(ref, 0, gate)
        assert len(truth) == 1 and abs(float(truth[0][0 if sense == W.ABOVE else 1]) / 8.0 - t_cross) < 1e-9
        assert abs(r["within_lo"] - (last - first)) <= 2 * TOL
    a = ref.rows([(W.ACCEL, W.ABOVE, 2 * c * 0.999), (W.ACCEL, W.ABOVE, 2 * c * 1.001), (W.JERK, W.ABOVE, 1e-6)], TOL)
    assert list(a["gate"]) == [0] and a["flags"][0] & (W.AT_START | W.AT_END) == W.AT_START | W.AT_END    # the acceleration is 2 c throughout, the jerk 0


def test_unbounded_levels_and_row_order(pkg, scenes):
    st, Pn, res = _states(pkg, scenes)["tiny_mode1"]
    ref = W.Ref(pkg, st, Pn, res)
    a = ref.rows([(W.SPEED, W.ABOVE, W.INF), (W.ACCEL, W.BELOW, W.INF), (W.JERK, W.ABOVE, -2.5), (W.SPEED, W.BELOW, -1.0), (W.SPEED, W.ABOVE, 0.0)], TOL)
    assert sorted(zip(a["robot"], a["gate"])) == list(zip(a["robot"], a["gate"])) == [(u, k) for u in range(ref.U) for k in (1, 2, 4)]
    assert np.all(a["flags"] == W.CERTAIN | W.AT_START | W.AT_END | W.RESOLVED) and np.all(a["windows"] == ref.S)
    b = ref.rows(W.measurement_gates(ref), TOL)
    key = list(zip(b["robot"], b["gate"], b["t_first_lo"]))
    assert key == sorted(key) and len(key) > 0


def test_depth_zero_ub_is_the_audits_bound(pkg, scenes):
    """at [0, 1] ub has tj_peak_dynamics' depth-0 bits (peak_dynamics_ref.Ref.evaluate's ub), which are tj_audit's"""
    st, Pn, res = _states(pkg, scenes)["tiny_mode1"]
    ref = W.Ref(pkg, st, Pn, res)
    tr = np.arange(ref.S)
    for u in range(ref.U):
        for q in range(3):
            assert np.array_equal(ref.bounds(u, q, tr, np.zeros(ref.S), np.ones(ref.S))[0], ref.evaluate(u, q, tr, np.zeros(ref.S), np.ones(ref.S))[0])


def test_the_headers_table_and_frontier(pkg):
    """the e2e_scn_b rows of the header's table are re-measured; TJ_DYNWIN_FRONTIER is the next power of two >= 4 x the table's largest live set, at least 64"""
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    block = hdr[hdr.index("tj_dynamics_windows: FROM WHEN TO WHEN"):hdr.index("#define TJ_DYNWIN_SPEED")]
    table = {m.group(1): tuple(int(x) for x in m.group(2).split()) + (float(m.group(3)),)
             for m in re.finditer(r"^ \*   (e2e_\w+)\s+((?:\d+\s+){6})(\d\.\d\de[-+]\d\d)$", block, flags=re.M)}
    assert len(table) == 8
    frontier, per = W.default_tolerance(pkg, names=[e for e in W.E2E if e[0] == "e2e_scn_b"])
    for label, v in per.items():
        assert table[label][:6] == v[:6] and "%.2e" % v[6] == "%.2e" % table[label][6], (label, v, table[label])
    assert not any(v[1] or v[2] for v in table.values())                                     # no measurement state is UNCERTAIN or TRUNCATED
    assert pkg.DYNWIN_FRONTIER == max(64, W.next_pow2(4 * max(v[3] for v in table.values()))) == 64
    assert int(re.search(r"#define TJ_DYNWIN_FRONTIER\s+(\d+)", hdr).group(1)) == pkg.DYNWIN_FRONTIER
    assert "1.54 eps" in block and "32 eps" in block
