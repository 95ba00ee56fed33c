"""Reference values for tj_zone_windows that share no code with csrc/kernels_zone_windows.h (plain module: no fixtures, no tests).

  Ref.rows            the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_zone_windows.py.  Hulls by
                      audit_ref.hulls_of, the blossoming of a window from the RAW hull by peak_dynamics_ref.bez_restrict (N = 6), the search of
                      dynamics_windows_ref.Ref.search unchanged -- it depends on its query through bounds() and classify() only -- and:
                        PLANES      f_ij = dot3(n_j, b_i) - d_j; lb = max_j min_i, ub = max_j max_i; g0 / g5 = max_j f_0j / f_5j with the smallest j
                        BALL        e_i = b_i - c; ub = max_i norm3(e_i) - r; lb = (min_i dot3(e_i, d) / norm3(d)) - r with d = e_0 + .. + e_5 left to
                                    right where norm3(d) > 0 and the minimum is positive, else 0 - r; g0 / g5 = norm3(e_0) - r / norm3(e_5) - r, face -1
                        class       INSIDE: OUT lb > level | IN ub <= level | MIXED; OUTSIDE: OUT ub < level | IN lb >= level | MIXED
                        merge       dynamics_windows_ref's rules with g = sigma * gauge and L = sigma * level (sigma = +1 INSIDE, -1 OUTSIDE); the extreme
                                    sample in the total order (sigma * g, time, face)
                      A zone is (kind, sense, level, rows [count][4]), as the package's zone_box / zone_ball / zone_planes return it.
  truth               mpmath: per segment the real roots in [0, 1] of each face's quintic f_j(x(s)) - level, or of the degree-10 |x(s) - c|^2 - (r + level)^2,
                      give the true set of flight positions INSIDE the level; OUTSIDE is its complement.  A segment whose polynomial has Bernstein
                      coefficients of one sign in np.longdouble (with a relative margin) has no root and is classified by that sign without mpmath.
  constructed states  peak_dynamics_ref's line; the measurement's zone set.
  default_tolerance   the measured tables of the header and TJ_ZONEWIN_FRONTIER."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import dynamics_windows_ref as W
import peak_dynamics_ref as P
from obstacle_approach_ref import E2E

LD = np.longdouble
CERTAIN, UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED = 1, 2, 4, 8, 16, 32
PLANES, BALL = 0, 1
INSIDE, OUTSIDE = 0, 1
MAX_ZONES, MAX_PLANES, MAX_DEPTH, MAX_WINDOWS, TOL_FRACTION = 64, 32, 40, 1024, 0.01
DOUBLES = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "extreme", "extreme_time")
FIELDS = DOUBLES + ("robot", "zone", "sense", "face", "segment_first", "segment_last", "leaves", "depth", "flags", "windows")
OUT, IN, MIXED = 0, 1, 2
INF = math.inf
EPS = 2.0 ** -53
INT_MAX = 2 ** 31 - 1
MODES = W.MODES
next_pow2 = W.next_pow2
line_state = P.line_state


def default_tol(offset, vel_limit):
    """what tol < 0 selects: the time to fly 1 % of the contact distance at the speed limit"""
    return (TOL_FRACTION * offset) / vel_limit


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


class Ref(W.Ref):
    """the restatement on one state; the search is dynamics_windows_ref.Ref.search with a zone where it passes its quantity on"""

    def __init__(self, pkg, st, Pn, res):
        super().__init__(pkg, st, Pn, res)
        self.frontier = pkg.ZONEWIN_FRONTIER                                                 # what max_windows=None selects

    def gauges(self, u, zone, tr, sa, sb):
        """items (tr[n], sa[n], sb[n]) -> ub[n], lb[n], g0[n], g5[n], f0[n], f5[n]"""
        kind, rows = zone[0], np.asarray(zone[3], dtype=np.float64)
        b = P.bez_restrict(self.H[u][tr], sa, sb)                                            # [n][6][3], always from the raw hull
        if kind == PLANES:
            n = rows[:, None, :]                                                             # [c][1][4] against [n][1][6] -> f [n][c][6]
            f = dot3(n[None, :, :, 0], n[None, :, :, 1], n[None, :, :, 2], b[:, None, :, 0], b[:, None, :, 1], b[:, None, :, 2]) - n[None, :, :, 3]
            g0, g5 = f[:, :, 0], f[:, :, 5]
            f0, f5 = g0.argmax(axis=1), g5.argmax(axis=1)                                    # (the first = the smallest j attaining the maximum)
            return f.max(axis=2).max(axis=1), f.min(axis=2).max(axis=1), g0.max(axis=1), g5.max(axis=1), f0, f5
        c, r = rows[0, :3], rows[0, 3]
        e = b - c
        v = P.norm3(e)
        d = e[:, 0]
        for i in range(1, 6):
            d = d + e[:, i]
        nd = P.norm3(d)
        m = dot3(e[:, :, 0], e[:, :, 1], e[:, :, 2], d[:, None, 0], d[:, None, 1], d[:, None, 2]).min(axis=1)
        ok = (nd > 0.0) & (m > 0.0)
        lb = np.where(ok, np.where(ok, m, 0.0) / np.where(ok, nd, 1.0), 0.0) - r
        none = np.full(len(tr), -1)
        return v.max(axis=1) - r, lb, v[:, 0] - r, v[:, 5] - r, none, none

    def bounds(self, u, q, tr, sa, sb):
        return self.gauges(u, q, tr, sa, sb)[:4]

    def classify(self, sense, level, ub, lb):
        if sense == INSIDE:
            return np.where(lb > level, OUT, np.where(ub <= level, IN, MIXED))
        return np.where(ub < level, OUT, np.where(lb >= level, IN, MIXED))

    def zone_rows(self, u, k, zone, tol, max_depth, max_windows, traces=None, leaves_out=None):
        kind, sense, level, _ = zone
        found = self.search(u, zone, sense, level, tol, max_depth, max_windows, None if traces is None else traces.setdefault((u, k), []))
        flat = found["leaves"]
        if flat:                                                                             # the faces of the attained ends: the evaluation again, the same bits
            ev = self.gauges(u, zone, np.array([lf[2] for lf in flat]), np.array([lf[3] for lf in flat]), np.array([lf[4] for lf in flat]))
            assert all(ev[2][i] == lf[5] and ev[3][i] == lf[6] for i, lf in enumerate(flat))
            flat = [lf + (int(ev[4][i]), int(ev[5][i])) for i, lf in enumerate(flat)]
        sigma = 1.0 if sense == INSIDE else -1.0
        L = sigma * level
        chains = []
        for i, lf in enumerate(flat):
            if i:
                assert flat[i - 1][1] <= lf[0] and flat[i - 1][0] < lf[0], (flat[i - 1], lf)   # distinct, disjoint
            if i and flat[i - 1][1] == lf[0]:
                chains[-1].append(lf)
            else:
                chains.append([lf])
        rows = []
        for chain in chains:
            sure, within, best = [], 0.0, (INF, INF, INT_MAX)
            for ga, gb, tr, sa, sb, h0, h5, is_in, f0, f5 in chain:
                ta, tb = self.time_g(u, ga), self.time_g(u, gb)
                g0, g5 = sigma * h0, sigma * h5
                if is_in:
                    sure += [ta, tb]
                    within += self.width(u, sa, sb)
                else:
                    if g0 <= L:
                        sure.append(ta)
                    if g5 <= L:
                        sure.append(tb)
                best = min(best, (g0, ta, f0), (g5, tb, f5))
            first, last = chain[0], chain[-1]
            first_lo, last_hi = self.time_g(u, first[0]), self.time_g(u, last[1])
            first_hi, last_lo = (min(sure), max(sure)) if sure else (-1.0, -1.0)
            at_start, at_end = first[0] == 0.0, last[1] == float(self.S)
            flags = (CERTAIN if sure else UNCERTAIN) | (AT_START if at_start else 0) | (AT_END if at_end else 0) | (TRUNCATED if found["truncated"] else 0)
            if sure and (at_start or first_hi - first_lo <= tol) and (at_end or last_hi - last_lo <= tol):
                flags |= RESOLVED
            rows.append(dict(t_first_lo=first_lo, t_first_hi=first_hi, t_last_lo=last_lo, t_last_hi=last_hi, within_lo=within, extreme=sigma * best[0],
                             extreme_time=best[1], robot=u, zone=k, sense=sense, face=best[2], segment_first=first[2], segment_last=last[2],
                             leaves=len(chain), depth=found["depth"], flags=flags, windows=found["windows"]))
            if leaves_out is not None:
                leaves_out.setdefault((u, k), []).append([(lf[0], lf[1], lf[7], lf[5], lf[6]) for lf in chain])
        return rows

    def rows(self, zones, tol, max_depth=MAX_DEPTH, max_windows=None, owned=None, traces=None, leaves=None):
        """the rows as a dict of numpy arrays [n] in (robot, zone, t_first_lo) order.  zones: a list of (kind, sense, level, rows); tol, max_depth, max_windows:
        the resolved values.  traces: per (robot, zone) the search's trace; leaves: per (robot, zone), per row the chain as (ga, gb, is IN, g0, g5)"""
        max_windows = self.frontier if max_windows is None else max_windows
        out = []
        for u in (range(self.U) if owned is None else owned):
            for k, z in enumerate(zones):
                out += self.zone_rows(u, k, (int(z[0]), int(z[1]), float(z[2]), np.asarray(z[3], dtype=np.float64)), float(tol), max_depth, max_windows, traces, leaves)
        return {n: np.array([r[n] for r in out], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}

    def scale(self, u, zone):
        """the slot's scale, what the stated limit (1) is relative to: the depth-0 largest |n_j| * |b_i| + |d_j| (PLANES), |e_i| + r (BALL)"""
        rows = np.asarray(zone[3], dtype=np.float64)
        b = self.H[u].reshape(-1, 3)
        if zone[0] == PLANES:
            return float((P.norm3(rows[:, :3])[:, None] * P.norm3(b)[None, :] + np.abs(rows[:, 3])[:, None]).max())
        return float(P.norm3(b - rows[0, :3]).max() + rows[0, 3])


# ---- the truth: the polynomials' own roots ----------------------------------------------------------------------------------------------------------

def _roots01(power, mp):
    """the real roots in (0, 1) of the polynomial with power-basis coefficients power[0..n] (mpf)"""
    pw = list(power)
    big = max([abs(x) for x in pw] + [mp.mpf(0)])
    while pw and abs(pw[-1]) <= big * mp.mpf(10) ** -40:
        pw.pop()
    out = []
    if len(pw) > 1:
        try:
            roots = mp.polyroots(pw[::-1], maxsteps=500, extraprec=400)
        except mp.NoConvergence:
            roots = [mp.mpf(float(r.real)) for r in np.roots([float(x) for x in pw[::-1]]) if abs(r.imag) < 1e-7]
        out = [mp.re(r) for r in roots if abs(mp.im(r)) <= mp.mpf(10) ** -15 and 0 < mp.re(r) < 1]
    return out


def gauge_at(ref, u, zone, g, tr=None):
    """the gauge's true value at flight position g (mpf), with segment tr's polynomial (None: the segment that holds g)"""
    import mpmath as mp
    mp.mp.dps = 60
    tr = min(int(mp.floor(g)), ref.S - 1) if tr is None else tr
    s = g - tr
    x = [sum(mp.binomial(5, i) * s ** i * (1 - s) ** (5 - i) * mp.mpf(float(ref.H[u][tr][i][a])) for i in range(6)) for a in range(3)]
    rows = np.asarray(zone[3], dtype=np.float64)
    if zone[0] == PLANES:
        return max(sum(mp.mpf(float(r[a])) * x[a] for a in range(3)) - mp.mpf(float(r[3])) for r in rows)
    return mp.sqrt(sum((x[a] - mp.mpf(float(rows[0][a]))) ** 2 for a in range(3))) - mp.mpf(float(rows[0][3]))


def true_inside(ref, u, zone):
    """the true set of flight positions g = tr + s in [0, S] at which robot u's gauge is <= the zone's level: a sorted list of disjoint closed intervals
    (mpf), adjacent ones merged (isolated touching points are not listed).  The zone's sense plays no part: OUTSIDE is the complement (complement)."""
    import mpmath as mp
    mp.mp.dps = 60
    kind, _, level, rows = zone
    rows = np.asarray(rows, dtype=np.float64)
    out = []
    for tr in range(ref.S):
        H = ref.H[u][tr]                                                                     # [6][3]
        cuts = [mp.mpf(0), mp.mpf(1)]
        if kind == PLANES:
            f = (H.astype(LD) @ rows[:, :3].T.astype(LD)) - rows[:, 3].astype(LD) - LD(level)   # [6][c]: face j's Bernstein coefficients, those of a quintic
            scale = np.abs(H).max() * np.abs(rows[:, :3]).max() + np.abs(rows[:, 3]).max() + abs(level)
            if np.any(np.all(f > 1e-9 * scale, axis=0)):                                     # a face is positive throughout: outside
                continue
            for j in np.flatnonzero(~np.all(f < -1e-9 * scale, axis=0)):                     # (a face negative throughout has no root)
                c = [sum(mp.mpf(float(rows[j][a])) * mp.mpf(float(H[i][a])) for a in range(3)) - mp.mpf(float(rows[j][3])) - mp.mpf(float(level)) for i in range(6)]
                cuts += _roots01(P._bernstein_to_power(c, mp), mp)
        else:
            rad = mp.mpf(float(rows[0][3])) + mp.mpf(float(level))
            if rad < 0:
                continue
            e = H.astype(LD) - rows[0, :3].astype(LD)
            sq = np.zeros(11, dtype=LD)
            for i in range(6):
                for j in range(6):
                    sq[i + j] += LD(math.comb(5, i) * math.comb(5, j)) / LD(math.comb(10, i + j)) * (e[i] * e[j]).sum()
            b = sq - LD(float(rad)) ** 2
            scale = max(float(np.abs(sq).max()), float(rad) ** 2)
            if np.all(b > 1e-9 * scale):
                continue
            if not np.all(b < -1e-9 * scale):
                pw = [P._bernstein_to_power([mp.mpf(float(H[i][a])) - mp.mpf(float(rows[0][a])) for i in range(6)], mp) for a in range(3)]
                poly = [sum(t) for t in zip(*[P._polymul(p, p, mp) for p in pw])]
                poly[0] -= rad ** 2
                cuts += _roots01(poly, mp)
        cuts = sorted(set(cuts))
        for a, b2 in zip(cuts[:-1], cuts[1:]):
            if gauge_at(ref, u, zone, tr + (a + b2) / 2, tr) <= mp.mpf(float(level)):
                a, b2 = tr + a, tr + b2
                if out and out[-1][1] == a:
                    out[-1] = (out[-1][0], b2)
                else:
                    out.append((a, b2))
    return out


def complement(ref, inside):
    import mpmath as mp
    return W._minus([(mp.mpf(0), mp.mpf(ref.S))], inside)


def true_within(ref, u, zone, inside=None):
    inside = true_inside(ref, u, zone) if inside is None else inside
    return inside if zone[1] == INSIDE else complement(ref, inside)


def contradictions(ref, u, zone, chains, truth_set):
    """the largest excess, relative to the slot's scale, by which the truth contradicts a certified class: a truly-within position outside every row
    (certified on the other side), or a position of an IN leaf that is truly outside.  The excess of a piece is the largest of |gauge - level| over 9 equally
    spaced positions of it.  Returns (excess of coverage, excess of IN leaves)."""
    import mpmath as mp
    scale = ref.scale(u, zone)
    rows = [(mp.mpf(c[0][0]), mp.mpf(c[-1][1])) for c in chains]
    ins = [(mp.mpf(lf[0]), mp.mpf(lf[1])) for c in chains for lf in c if lf[2]]

    def excess(pieces):
        worst = 0.0
        for lo, hi in pieces:
            for tr in range(int(mp.floor(lo)), min(int(mp.ceil(hi)), ref.S)):                 # segment by segment: each piece with its own polynomial
                a, b = max(lo, mp.mpf(tr)), min(hi, mp.mpf(tr + 1))
                for k in range(9):
                    worst = max(worst, float(abs(gauge_at(ref, u, zone, a + (b - a) * k / 8, tr) - mp.mpf(float(zone[2])))))
        return worst / scale if scale > 0 else worst

    return excess(W._minus(truth_set, rows)), excess(W._minus(ins, truth_set))


# ---- the measurement's zone set ----------------------------------------------------------------------------------------------------------------------

def prism_rows(center, apothem, z_lo, z_hi, sides=30):
    """a prism of `sides` vertical faces with unit normals around the vertical axis through `center`, floor and ceiling: sides + 2 rows"""
    rows = []
    for i in range(sides):
        a = 2 * math.pi * i / sides
        nx, ny = math.cos(a), math.sin(a)
        rows.append([nx, ny, 0.0, nx * center[0] + ny * center[1] + apothem])
    return np.array(rows + [[0.0, 0.0, -1.0, -z_lo], [0.0, 0.0, 1.0, z_hi]])


def box_rows(lo, hi):
    """the package's zone_box rows: -x, +x, -y, +y, -z, +z"""
    return np.array([[-1.0, 0, 0, -lo[0]], [1.0, 0, 0, hi[0]], [0, -1.0, 0, -lo[1]], [0, 1.0, 0, hi[1]], [0, 0, -1.0, -lo[2]], [0, 0, 1.0, hi[2]]])


def measurement_shapes(ref, offset=0.1):
    """the five shapes built from the state: (kind, rows)"""
    pts = ref.H.reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    third = (hi - lo) / 3.0
    mean = pts.mean(axis=0)
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    mid = 0.5 * (lo + hi)
    return [(PLANES, box_rows(lo + third, hi - third)),
            (PLANES, box_rows(lo + offset, hi - offset)),
            (PLANES, np.array([[0.0, 0.0, -1.0, -(mean[2] - offset)], [0.0, 0.0, 1.0, mean[2] + offset]])),
            (PLANES, prism_rows(mid, 0.25 * float(np.sqrt(((hi - lo)[:2] ** 2).sum())), lo[2], hi[2])),
            (BALL, np.array([[mean[0], mean[1], mean[2], 0.25 * diag]]))]


def measurement_zones(ref, offset=0.1):
    """every shape in both senses at levels 0 and -offset: 20 zones"""
    return [(kind, sense, level, rows) for kind, rows in measurement_shapes(ref, offset) for sense in (INSIDE, OUTSIDE) for level in (0.0, -offset)]


def measurement_states(pkg, names=E2E):
    return W.measurement_states(pkg, names)


def default_tolerance(pkg, names=E2E, offset=0.1, vel_limit=2.0):
    """(frontier, per state: (rows, UNCERTAIN rows, TRUNCATED rows, largest live set after a round >= 1, largest leaf list, largest depth, widest bracket)): the
    default tol, max_depth = 40, the lists capped at MAX_WINDOWS only, over the state's 20 measurement zones.  The widest bracket is the largest of t_first_hi -
    t_first_lo and t_last_hi - t_last_lo over the CERTAIN rows.  The frontier is the next power of two >= 4 x the largest live set, at least 64."""
    per, widest = {}, 0
    tol = default_tol(offset, vel_limit)
    for label, st, Pn, res in measurement_states(pkg, names):
        ref = Ref(pkg, st, Pn, res)
        traces = {}
        rows = ref.rows(measurement_zones(ref, offset), tol, MAX_DEPTH, MAX_WINDOWS, traces=traces)
        live = max([t[1] for tr in traces.values() for t in tr if t[0] >= 1] + [0])
        kept = max([t[2] for tr in traces.values() for t in tr] + [0])
        sure = rows["flags"] & CERTAIN != 0
        width = max([0.0] + list(rows["t_first_hi"][sure] - rows["t_first_lo"][sure]) + list(rows["t_last_hi"][sure] - rows["t_last_lo"][sure]))
        per[label] = (len(rows["robot"]), int(np.sum(rows["flags"] & UNCERTAIN != 0)), int(np.sum(rows["flags"] & TRUNCATED != 0)), live, kept,
                      int(rows["depth"].max()) if len(rows["depth"]) else 0, float(width))
        widest = max(widest, live)
    return max(64, next_pow2(4 * max(widest, 1))), per


def measured_excess(pkg, states, offset=0.1, vel_limit=2.0, max_robots=None):
    """the largest contradiction (coverage, IN leaves) over `states` = [(label, state, P, res)] at the measurement's zones and the default tol, in units of
    eps = 2^-53 of the slot's scale"""
    worst = [0.0, 0.0]
    tol = default_tol(offset, vel_limit)
    for label, st, Pn, res in states:
        ref = Ref(pkg, st, Pn, res)
        zones = measurement_zones(ref, offset)
        for u in range(ref.U if max_robots is None else min(ref.U, max_robots)):
            inside = {}
            for k, zone in enumerate(zones):
                leaves = {}
                ref.zone_rows(u, k, zone, tol, MAX_DEPTH, MAX_WINDOWS, None, leaves)
                key = (k // 4, zone[2])                                                      # (the shape, the level): both senses share the roots
                if key not in inside:
                    inside[key] = true_inside(ref, u, zone)
                cov, inn = contradictions(ref, u, zone, leaves.get((u, k), []), true_within(ref, u, zone, inside[key]))
                worst = [max(worst[0], cov / EPS), max(worst[1], inn / EPS)]
    return worst
