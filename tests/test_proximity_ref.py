"""CPU (-m "not gpu"): the restatement tests/test_gpu_proximity.py holds the device to (tests/proximity_ref.py) is itself held to the flown curves, which
share nothing with its bounds: both curves of a pair are sampled densely in time with tests/flight_profile_ref.py's position expressions (the segment by the
rule T(j) <= t < T(j + 1), the point by de Casteljau steps at clamp01((t - T(j)) / (T(j + 1) - T(j))), after the arrival the last control point), no GJK, no
subdivision.  Every sample within dist lies in a row, every pair with such a sample is listed, the sure times attain dist, the IN leaves hold, two straight
lines give the entry and exit times in closed form, the leaves and the dropped windows tile the flight, and the committed defaults are the measured ones.
Bars: in space audit_timed_ref's counted slack (two curves restricted to windows).

Measured (printed by test_defaults_are_the_measured_ones; recorded in include/trajadmm.h, whose table the test reads back): the largest live set is 3, the
largest kept list 88 -> TJ_PROXIMITY_FRONTIER = 512."""
import functools
import math
import os
import re

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
import proximity_ref as X
import timing_margin_ref as M
from conftest import ROOT
from query_kit import pkg_module as _pkg

OFFSET, VEL = 0.1, 2.0
INF = float("inf")
SAMPLES = 20000
E2E = [(n + f, d) for n, f in X.STATES for d in X.DISTS]
BUILT = [("chase", 0.1), ("chase", 1.0), ("crossing", 2.5), ("crossing", 2.2), ("hover", 0.1), ("hover", 2.5)]
# test_truncation: the flattened fleet at dist = offset; at max_windows = 16 the kept list of some pairs overflows inside the rounds and that of others does not
# (chosen here, on the CPU: 8 truncates 3810 of 4032 rows, 16 truncates 518, at depths 2 .. 10; tests/test_gpu_proximity.py uses it on robots 0..7, where it
# truncates 32 of 56 rows, and adds (1.0, 32), which overflows among the seeds for 50 of 56)
TRUNC_DIST, TRUNC_WINDOWS = 0.1, 16


@functools.lru_cache(maxsize=None)
def measured(name, dist, max_windows=X.MAX_WINDOWS):
    """(state, P, res, rows, listed pairs, leaves, dropped) at the default tol; shared by the tests and never written to"""
    pkg = _pkg()
    for n, f in X.STATES:
        if n + f == name and max_windows == X.MAX_WINDOWS:
            st, P, res, rows, n_pairs, _, leaves, dropped = X.measured(pkg, R.prims(), n, f, dist, OFFSET, VEL)
            return st, P, res, rows, n_pairs, leaves, dropped
    if name in ("chase", "crossing", "hover"):
        st, P, res = getattr(T, name + "_state")(pkg, pkg.scenes)[1], 4, 8
    else:
        st, P, res = M.state_named("e2e_scn_c3", name[len("e2e_scn_c3"):])
    leaves, dropped = {}, {}
    rows, n_pairs = X.proximity_rows(pkg, R.prims(), st, P, res, dist, X.default_tol(dist, OFFSET, VEL), X.MAX_DEPTH, max_windows, leaves=leaves, dropped=dropped)
    return st, P, res, rows, n_pairs, leaves, dropped


def positions(pkg, st, P, res, u, t, end=False):
    """robot u at the times t [K] -> [K][3], flight_profile_ref's expressions vectorised: the segment j with T(j) <= t < T(j + 1), T(j) = (j / res) * pt (the
    quotient only proposes), the parameter clamp01((t - T(j)) / (T(j + 1) - T(j))), the point b_0 of the raw hull restricted to [s, s]; j == S: the last control
    point.  end=True: a time that IS a boundary T(j), j > 0, is taken as the END of segment j - 1 (s = 1) -- the same point of a continuous curve, other bits."""
    S, rf, pt = P * res, float(res), float(st["piece_time"][u])
    H = hulls(pkg, st, P, res)[u]
    t = np.asarray(t, dtype=np.float64)
    g = np.floor((t / pt) * rf)
    j = np.where(g >= S, S, np.where(g > 0, g, 0)).astype(np.int64)
    for _ in range(3):
        j = np.where((j > 0) & ((j / rf) * pt > t), j - 1, j)
        j = np.where((j < S) & (((j + 1) / rf) * pt <= t), j + 1, j)
    assert np.all(((j / rf) * pt <= t) & ((j == S) | (((j + 1) / rf) * pt > t)))
    if end:
        j = np.where((j > 0) & ((j / rf) * pt == t), j - 1, j)
    Tj, Tj1 = (j / rf) * pt, ((j + 1) / rf) * pt
    s = np.minimum(np.maximum((t - Tj) / (Tj1 - Tj), 0.0), 1.0)
    fly = j < S
    out = np.repeat(H[S - 1, 5][None, :], len(t), axis=0)
    if fly.any():
        out[fly] = T.bez_restrict(H[j[fly]], s[fly], s[fly])[:, 0]
    return out


_HULLS = {}


def hulls(pkg, st, P, res):
    """the raw hulls [U][S][6][3] of a state, formed once (the states of `measured` live as long as the process)"""
    key = id(st["spline"])
    if key not in _HULLS:
        _HULLS[key] = (st["spline"], R.hulls_of(pkg, np.asarray(st["spline"], dtype=np.float64), P, res))
    return _HULLS[key][1]


def norm3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def rows_by_pair(rows):
    by = {}
    for k, key in enumerate(zip(rows["robot"].tolist(), rows["partner"].tolist())):
        by.setdefault(key, []).append(k)
    return by


@pytest.mark.parametrize("name,dist", E2E + BUILT)
def test_rows_cover_the_flown_curves(pkg, name, dist):
    """coverage, attainment, certified inside and the tiling, on one dense sampling per state: at least SAMPLES times inside every robot's flight (one grid
    over the longest flight, fine enough for the shortest) plus every row's five times"""
    st, P, res, rows, n_pairs, leaves, dropped = measured(name, dist)
    U, S = st["spline"].shape[0], P * res
    sl = T.slack(S, st["spline"])
    flight = np.array([((S - 1 + 1) / float(res)) * float(p) for p in st["piece_time"]])
    K = int(math.ceil(SAMPLES * flight.max() / flight.min())) + 1
    own = np.concatenate([rows[n] for n in ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "closest_time")])
    t = np.unique(np.concatenate([np.linspace(0.0, flight.max(), K), own[own >= 0.0], flight]))
    pos = np.stack([positions(pkg, st, P, res, u, t) for u in range(U)])                     # [U][K][3]
    by = rows_by_pair(rows)
    assert n_pairs == len(leaves) and set(by) <= set(leaves)
    key = list(zip(rows["robot"].tolist(), rows["partner"].tolist(), rows["t_first_lo"].tolist()))
    assert key == sorted(key)
    checked = 0
    for u in range(U):
        mine = t <= flight[u]
        tu = t[mine]
        sep = norm3(pos[u][None, mine, :] - pos[:, mine, :])                                  # [U][k]
        for q in range(U):
            if q == u:
                continue
            near = sep[q] <= dist
            if (u, q) not in leaves:
                assert not near.any(), (u, q, "a sample within dist of a pair that is not listed", float(sep[q].min()))
                continue
            ks = by.get((u, q), [])
            lo, hi = rows["t_first_lo"][ks], rows["t_last_hi"][ks]
            if near.any():                                                                  # coverage: every such sample lies inside some row
                at = np.searchsorted(lo, tu[near], side="right") - 1
                assert np.all(at >= 0) and np.all(tu[near] <= hi[np.maximum(at, 0)]), (u, q)
            for k in ks:                                                                    # attainment
                for n in ("t_first_hi", "t_last_lo") + (("closest_time",) if rows["flags"][k] & X.CERTAIN else ()):
                    if rows[n][k] >= 0.0:
                        assert sep[q][np.searchsorted(tu, rows[n][k])] <= dist + sl, (u, q, n)
                assert (rows["flags"][k] & X.CERTAIN != 0) == (rows["t_first_hi"][k] >= 0.0) == (rows["t_last_lo"][k] >= 0.0) != bool(rows["flags"][k] & X.UNCERTAIN)
                assert rows["within_lo"][k] <= rows["t_last_hi"][k] - rows["t_first_lo"][k] and (rows["closest"][k] <= dist) == bool(rows["flags"][k] & X.CERTAIN)
                # closest is the sample at closest_time, bit for bit (at a segment boundary: of the segment that ends or of the one that starts there)
                tc = np.array([rows["closest_time"][k]])
                got = {float(norm3(positions(pkg, st, P, res, u, tc, eu) - positions(pkg, st, P, res, q, tc, eq))[0]) for eu in (False, True) for eq in (False, True)}
                assert rows["closest"][k] in got and max(got) - min(got) <= sl, (u, q, rows["closest"][k], got)
            for ca, cb, h0, h5, is_in in leaves[(u, q)]:                                    # certified inside
                if is_in:
                    a, b = np.searchsorted(tu, ca, side="left"), np.searchsorted(tu, cb, side="right")
                    assert np.all(sep[q][a:b] <= dist + sl), (u, q, ca, cb)
            # the tiling: leaves and dropped windows are disjoint; a gap between two chains is dropped windows end to end, or time no seed was evaluated
            # for (the box prefilter: certified by the samples above); the chains are exactly what the rows say
            tiles = sorted([(x[0], x[1], 1) for x in leaves[(u, q)]] + [(a, b, 0) for a, b in dropped[(u, q)]])
            assert all(tiles[i][1] <= tiles[i + 1][0] for i in range(len(tiles) - 1)), (u, q)
            chains = X.chains_of(leaves[(u, q)])
            assert [(c[0][0], c[-1][1], len(c)) for c in chains] == [(rows["t_first_lo"][k], rows["t_last_hi"][k], rows["leaves"][k]) for k in ks]
            for c0, c1 in zip(chains[:-1], chains[1:]):
                between = [x for x in tiles if c0[-1][1] <= x[0] and x[1] <= c1[0][0]]
                assert between and all(x[2] == 0 for x in between) and between[0][0] == c0[-1][1] and between[-1][1] == c1[0][0], (u, q)
            checked += 1
    assert checked == n_pairs
    print(name, dist, "pairs", n_pairs, "rows", len(rows["robot"]), "samples", len(t))


def test_two_straight_lines_in_closed_form(pkg):
    """crossing_state: |p_0(t) - p_1(t)|^2 = 7.8125 t^2 - 37.5 t + 50, minimum sqrt(5) at t = 2.4.  Above it the row brackets both roots of
    |.| = dist within tol plus the slack in time (the slack in space over the rate of change at the root, 1.25 and more); below it nothing is listed"""
    st, P, res, rows, n_pairs, _, _ = measured("crossing", 2.5)
    tol, sl = X.default_tol(2.5, OFFSET, VEL), T.slack(P * res, st["spline"])
    disc = math.sqrt(37.5 ** 2 - 4 * 7.8125 * (50 - 2.5 ** 2))
    t_in, t_out = (37.5 - disc) / 15.625, (37.5 + disc) / 15.625
    assert abs(t_in - 2.0) < 1e-12 and abs(t_out - 2.8) < 1e-12 and n_pairs == 2 and len(rows["robot"]) == 2
    for k in range(2):
        assert rows["flags"][k] == X.CERTAIN | X.RESOLVED
        assert rows["t_first_lo"][k] - sl <= t_in <= rows["t_first_hi"][k] + sl and rows["t_first_hi"][k] - rows["t_first_lo"][k] <= tol
        assert rows["t_last_lo"][k] - sl <= t_out <= rows["t_last_hi"][k] + sl and rows["t_last_hi"][k] - rows["t_last_lo"][k] <= tol
        assert math.sqrt(5.0) - sl <= rows["closest"][k] <= 2.5 and rows["within_lo"][k] <= t_out - t_in + 2 * sl
    assert measured("crossing", 2.2)[4] == 0 and len(measured("crossing", 2.2)[3]["robot"]) == 0 and math.sqrt(5.0) > 2.2


@pytest.mark.parametrize("name", ["e2e_scn_b", "chase", "hover"])
def test_an_infinite_distance_lists_every_flight_whole(pkg, name):
    st, P, res, rows, n_pairs, leaves, _ = measured(name, INF)
    U, S = st["spline"].shape[0], P * res
    assert n_pairs == len(rows["robot"]) == U * (U - 1)
    assert np.all(rows["flags"] == X.CERTAIN | X.AT_START | X.AT_END | X.RESOLVED) and np.all(rows["depth"] == 0)
    for k in range(len(rows["robot"])):
        flight = ((S - 1 + 1) / float(res)) * float(st["piece_time"][rows["robot"][k]])
        assert (rows["t_first_lo"][k], rows["t_first_hi"][k], rows["t_last_lo"][k], rows["t_last_hi"][k]) == (0.0, 0.0, flight, flight)
        # the leaves' lengths summed left to right: at most one rounding per leaf and per cut against the flight itself
        assert abs(rows["within_lo"][k] - flight) <= 2 * rows["leaves"][k] * T.EPS * flight and rows["windows"][k] == rows["leaves"][k]


def test_constructed_states_mean_what_they_say(pkg):
    st, P, res, rows, n_pairs, _, _ = measured("chase", 0.1)                  # the two meet at t = 1.6; robot 1 passes the hovering robot 0 at t = 6.4
    by = rows_by_pair(rows)
    assert n_pairs == 2 and [len(by[k]) for k in ((0, 1), (1, 0))] == [1, 2]
    for k, t in ((by[(0, 1)][0], 1.6), (by[(1, 0)][0], 1.6), (by[(1, 0)][1], 6.4)):
        assert rows["flags"][k] == X.CERTAIN | X.RESOLVED and rows["t_first_hi"][k] <= t <= rows["t_last_lo"][k]
    st, P, res, rows, n_pairs, _, _ = measured("hover", 0.1)                  # robot 0's own flight is over at t = 2; robot 1 meets it, hovering, at t = 3.6
    assert list(zip(rows["robot"], rows["partner"])) == [(1, 0)] and rows["t_first_lo"][0] > 2.0 and rows["t_first_hi"][0] <= 3.6 <= rows["t_last_lo"][0]
    st, P, res, rows, n_pairs, _, _ = measured("hover", 2.5)                  # robot 0 ends its flight 2 away from robot 1: a row that runs to its end
    k = rows_by_pair(rows)[(0, 1)]
    assert len(k) == 1 and rows["flags"][k[0]] & X.AT_END and rows["t_last_hi"][k[0]] == 2.0


def test_truncation(pkg):
    """the flattened fleet with the lists capped at TRUNC_WINDOWS: some rows truncate inside the rounds, not all; the truncated rows still cover the curves
    (robots 0..7 are sampled: 56 of the 4032 pairs)"""
    st, P, res, rows, n_pairs, leaves, _ = measured("e2e_scn_c3_flat", TRUNC_DIST, TRUNC_WINDOWS)
    cut = rows["flags"] & X.TRUNCATED != 0
    print("truncated rows", int(cut.sum()), "of", len(cut), "depths", sorted(set(rows["depth"][cut].tolist())))
    assert cut.any() and not cut.all() and (rows["depth"][cut] > 0).any()
    full = measured("e2e_scn_c3_flat", TRUNC_DIST)[3]
    assert not (full["flags"] & X.TRUNCATED).any()
    S = P * res
    by = rows_by_pair(rows)
    seen = 0
    for u in range(8):
        flight = ((S - 1 + 1) / float(res)) * float(st["piece_time"][u])
        t = np.linspace(0.0, flight, SAMPLES)
        pu = positions(pkg, st, P, res, u, t)
        for q in range(8):
            if q == u:
                continue
            near = norm3(pu - positions(pkg, st, P, res, q, t)) <= TRUNC_DIST
            assert (u, q) in leaves or not near.any()
            ks = by.get((u, q), [])
            seen += int(np.any(cut[ks]))
            if near.any():
                lo, hi = rows["t_first_lo"][ks], rows["t_last_hi"][ks]
                at = np.searchsorted(lo, t[near], side="right") - 1
                assert np.all(at >= 0) and np.all(t[near] <= hi[np.maximum(at, 0)]), (u, q)
    assert seen > 0


def test_defaults_are_the_measured_ones(pkg):
    frontier, per = X.default_tolerance(pkg, R.prims())
    print("frontier", frontier, "per (state, dist): (listed, rows, uncertain, truncated, largest live set, largest kept list, largest depth, widest bracket)", per)
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert X.default_tol(OFFSET, OFFSET, VEL) == 5e-4 == X.default_tol(INF, OFFSET, VEL)
    assert pkg.PROXIMITY_TOL_FRACTION == X.TOL_FRACTION == float(re.search(r"#define TJ_PROXIMITY_TOL_FRACTION\s+(\S+)", hdr).group(1))
    assert frontier == pkg.PROXIMITY_FRONTIER == int(re.search(r"#define TJ_PROXIMITY_FRONTIER\s+(\S+)", hdr).group(1))
    assert pkg.PROXIMITY_MAX_DEPTH == X.MAX_DEPTH == int(re.search(r"#define TJ_PROXIMITY_MAX_DEPTH\s+(\S+)", hdr).group(1))
    assert pkg.PROXIMITY_MAX_WINDOWS == X.MAX_WINDOWS == int(re.search(r"#define TJ_PROXIMITY_MAX_WINDOWS\s+(\S+)", hdr).group(1))
    block = hdr[hdr.index("---- tj_proximity_windows"):hdr.index("#define TJ_PROXIMITY_CERTAIN")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    design = design[design.index("tj_proximity_windows"):]
    for (name, dist), v in per.items():
        pat = r"%s\s+%s\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\S+)\s*\n" % (re.escape(name), re.escape("%.1f" % dist))
        for where, txt in (("include/trajadmm.h", block), ("DESIGN.md", design)):
            m = re.search(pat, txt)
            assert m and tuple(int(m.group(i)) for i in range(1, 8)) == v[:7] and float(m.group(8)) == float("%.2e" % v[7]), (where, name, dist, v)
