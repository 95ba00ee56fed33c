"""Reference values for tj_dynamics_windows that share no code with csrc/kernels_dynamics_windows.h (plain module: no fixtures, no tests).

  Ref.rows            the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_dynamics_windows.py.  It builds on
                      peak_dynamics_ref.Ref's pieces -- hulls by audit_ref.hulls_of, the raw derivative nets, the blossoming of a window from the RAW net, den --
                      and adds:
                        bounds      ub = max_i norm3(c_i) / den; lb = (min_i dot3(c_i, d) / norm3(d)) / den with d = c_0 + .. + c_n left to right, where
                                    norm3(d) > 0 and the minimum is positive, else 0; h0, h5 = norm3(c_0) / den, norm3(c_n) / den
                        class       ABOVE: OUT ub < level | IN lb >= level | MIXED; BELOW: OUT lb > level | IN ub <= level | MIXED
                        search      one per (robot, gate) over the whole flight: seeds every segment at [0, 1]; a round turns a live window whose time width
                                    ((sb - sa) / res) * piece_time <= tol into an EDGE leaf and halves every other; OUT dropped, IN to the leaves, MIXED to the
                                    next live set.  Stop: live empty | depth == max_depth | after a round more than max_windows live or more than
                                    S + max_windows leaves (TRUNCATED: the lists of the last completed round; `windows` counts the overflowing round too).  The
                                    live windows end as EDGE leaves.
                        merge       the leaves by tr + sa; adjacent iff prev.tr + prev.sb == next.tr + next.sa; a row per maximal chain, tj_obstacle_windows'
                                    rules with g = sigma * value and L = sigma * level (sigma = -1 ABOVE, +1 BELOW)
  truth               mpmath: per segment the real roots in [0, 1] of |q(s)|^2 - (level * den)^2 on the raw net (peak_dynamics_ref's Bernstein-to-power
                      helpers) give the true set of flight positions within the level.  A segment whose |q|^2 - (level den)^2 has Bernstein coefficients of
                      one sign in np.longdouble (degree 2n, with a relative margin) has no root and is classified by that sign without mpmath.
  constructed states  peak_dynamics_ref's hover and line, and a uniform acceleration along x.
  default_tolerance   the measured tables of the header and TJ_DYNWIN_FRONTIER."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import peak_dynamics_ref as P
from obstacle_approach_ref import E2E

LD = np.longdouble
CERTAIN, UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED = 1, 2, 4, 8, 16, 32
SPEED, ACCEL, JERK = 0, 1, 2
ABOVE, BELOW = 0, 1
MAX_GATES, MAX_DEPTH, MAX_WINDOWS, TOL_FRACTION = 16, 40, 1024, 0.01
DOUBLES = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "extreme", "extreme_time")
FIELDS = DOUBLES + ("robot", "gate", "quantity", "sense", "segment_first", "segment_last", "leaves", "depth", "flags", "windows")
OUT, IN, MIXED = 0, 1, 2
INF = math.inf
EPS = 2.0 ** -53


def default_tol(vel_limit, acc_limit):
    """what tol < 0 selects: the time in which a vehicle at the acceleration limit changes its speed by 1 % of the speed limit"""
    return (TOL_FRACTION * vel_limit) / acc_limit


def default_gates(vel_limit, acc_limit):
    """what gates == NULL selects"""
    return [(SPEED, ABOVE, vel_limit), (ACCEL, ABOVE, acc_limit)]


class Ref(P.Ref):
    """the restatement on one state"""

    def __init__(self, pkg, st, Pn, res):
        super().__init__(pkg, st, Pn, res)
        self.frontier = pkg.DYNWIN_FRONTIER                                                  # what max_windows=None selects

    def bounds(self, u, q, tr, sa, sb):
        """items (tr[n], sa[n], sb[n]) -> ub[n], lb[n], h0[n], h5[n]"""
        net = P.bez_restrict(self.raw(u, q)[tr], sa, sb)                                     # [n][N][3], always from the raw net
        den = self.den(u, q, tr)
        v = P.norm3(net) / den[:, None]
        d = net[:, 0]
        for i in range(1, net.shape[1]):
            d = d + net[:, i]
        nd = P.norm3(d)
        m = ((net[:, :, 0] * d[:, None, 0] + net[:, :, 1] * d[:, None, 1]) + net[:, :, 2] * d[:, None, 2]).min(axis=1)
        ok = (nd > 0.0) & (m > 0.0)
        lb = np.where(ok, (np.where(ok, m, 0.0) / np.where(ok, nd, 1.0)) / den, 0.0)
        return v.max(axis=1), lb, v[:, 0], v[:, -1]

    def classify(self, sense, level, ub, lb):
        if sense == ABOVE:
            return np.where(ub < level, OUT, np.where(lb >= level, IN, MIXED))
        return np.where(lb > level, OUT, np.where(ub <= level, IN, MIXED))

    def width(self, u, sa, sb):
        return ((sb - sa) / self.rf) * float(self.pt[u])

    def time_g(self, u, g):
        return (g / self.rf) * float(self.pt[u])

    def search(self, u, q, sense, level, tol, max_depth, max_windows, trace=None):
        """the leaves of (robot u, gate): dict(leaves sorted by flight position: (ga, gb, tr, sa, sb, h0, h5, is IN), depth, windows, truncated).  trace receives
        (depth, size of the live set, size of the leaf list) after the seeds and after every round, the overflowing one included"""
        S = self.S
        tr = np.arange(S)
        sa, sb = np.zeros(S), np.ones(S)
        ub, lb, h0, h5 = self.bounds(u, q, tr, sa, sb)
        c = self.classify(sense, level, ub, lb)
        windows = S

        def items(keep, tr, sa, sb, h0, h5):
            return [(int(tr[k]), float(sa[k]), float(sb[k]), float(h0[k]), float(h5[k])) for k in np.flatnonzero(keep)]

        leaves = [w + (True,) for w in items(c == IN, tr, sa, sb, h0, h5)]
        live = items(c == MIXED, tr, sa, sb, h0, h5)
        if trace is not None:
            trace.append((0, len(live), len(leaves)))
        d, truncated = 0, False
        while live and d < max_depth:
            new, halve = list(leaves), []
            for w in live:
                if self.width(u, w[1], w[2]) <= tol:
                    new.append(w + (False,))
                else:
                    halve.append(w)
            nxt = []
            if halve:
                ltr = np.array([w[0] for w in halve]); la = np.array([w[1] for w in halve]); lz = np.array([w[2] for w in halve])
                sm = 0.5 * (la + lz)
                assert np.all((la < sm) & (sm < lz))
                ktr, ka, kb = np.concatenate([ltr, ltr]), np.concatenate([la, sm]), np.concatenate([sm, lz])
                ub, lb, h0, h5 = self.bounds(u, q, ktr, ka, kb)
                c = self.classify(sense, level, ub, lb)
                windows += len(ktr)
                new += [w + (True,) for w in items(c == IN, ktr, ka, kb, h0, h5)]
                nxt = items(c == MIXED, ktr, ka, kb, h0, h5)
            if trace is not None:
                trace.append((d + 1, len(nxt), len(new)))
            if len(nxt) > max_windows or len(new) > S + max_windows:
                truncated = True
                break
            d += 1
            leaves, live = new, nxt
        leaves = leaves + [w + (False,) for w in live]
        out = sorted((w[0] + w[1], w[0] + w[2]) + w for w in leaves)
        return dict(leaves=out, depth=d, windows=windows, truncated=truncated)

    def gate_rows(self, u, k, gate, tol, max_depth, max_windows, traces=None, leaves_out=None):
        q, sense, level = gate
        found = self.search(u, q, sense, level, tol, max_depth, max_windows, None if traces is None else traces.setdefault((u, k), []))
        flat = found["leaves"]
        sigma = -1.0 if sense == ABOVE else 1.0
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
            sure, within, best = [], 0.0, (INF, INF)
            for ga, gb, tr, sa, sb, h0, h5, is_in in chain:
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
                best = min(best, (g0, ta), (g5, tb))
            first, last = chain[0], chain[-1]
            first_lo, last_hi = self.time_g(u, first[0]), self.time_g(u, last[1])
            first_hi, last_lo = (min(sure), max(sure)) if sure else (-1.0, -1.0)
            at_start, at_end = first[0] == 0.0, last[1] == float(self.S)
            flags = (CERTAIN if sure else UNCERTAIN) | (AT_START if at_start else 0) | (AT_END if at_end else 0) | (TRUNCATED if found["truncated"] else 0)
            if sure and (at_start or first_hi - first_lo <= tol) and (at_end or last_hi - last_lo <= tol):
                flags |= RESOLVED
            rows.append(dict(t_first_lo=first_lo, t_first_hi=first_hi, t_last_lo=last_lo, t_last_hi=last_hi, within_lo=within, extreme=sigma * best[0],
                             extreme_time=best[1], robot=u, gate=k, quantity=q, sense=sense, segment_first=first[2], segment_last=last[2], leaves=len(chain),
                             depth=found["depth"], flags=flags, windows=found["windows"]))
            if leaves_out is not None:
                leaves_out.setdefault((u, k), []).append([(ga, gb, is_in, h0, h5) for ga, gb, _, _, _, h0, h5, is_in in chain])
        return rows

    def rows(self, gates, tol, max_depth=MAX_DEPTH, max_windows=None, owned=None, traces=None, leaves=None):
        """the rows as a dict of numpy arrays [n] in (robot, gate, t_first_lo) order.  gates: the resolved list of (quantity, sense, level); tol, max_depth,
        max_windows: the resolved values.  traces: per (robot, gate) the search's trace; leaves: per (robot, gate), per row the chain as (ga, gb, is IN, h0, h5)
        in flight position"""
        max_windows = self.frontier if max_windows is None else max_windows
        out = []
        for u in (range(self.U) if owned is None else owned):
            for k, gate in enumerate(gates):
                out += self.gate_rows(u, k, (int(gate[0]), int(gate[1]), float(gate[2])), float(tol), max_depth, max_windows, traces, leaves)
        return {n: np.array([r[n] for r in out], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}

    def ub0(self, u, q):
        """the robot's depth-0 ub of quantity q: what the stated limit (1) is relative to"""
        tr = np.arange(self.S)
        return float(self.bounds(u, q, tr, np.zeros(self.S), np.ones(self.S))[0].max())


# ---- the truth: the polynomial's own roots -----------------------------------------------------------------------------------------------------------

def _square_bernstein(net):
    """net [n + 1][3] (float64, the raw net) -> the Bernstein coefficients [2n + 1] of |q(s)|^2 in np.longdouble"""
    n = net.shape[0] - 1
    c = net.astype(LD)
    out = np.zeros(2 * n + 1, dtype=LD)
    for i in range(n + 1):
        for j in range(n + 1):
            out[i + j] += LD(math.comb(n, i) * math.comb(n, j)) / LD(math.comb(2 * n, i + j)) * (c[i] * c[j]).sum()
    return out


def _segment_within(net, rhs, sense, mp):
    """the sub-intervals [(a, b)] of [0, 1] (mpf) on which |q(s)|^2 >= rhs (ABOVE) or <= rhs (BELOW), rhs = (level den)^2 as an mpf, or -1 for a negative
    level (|q| >= level everywhere, <= nowhere)"""
    if rhs < 0:
        return [(mp.mpf(0), mp.mpf(1))] if sense == ABOVE else []
    b = _square_bernstein(net) - LD(float(rhs))
    scale = max(float(np.abs(_square_bernstein(net)).max()), float(rhs))
    if scale == 0.0:                                                                       # the quantity is 0 on the segment and the level is 0: equal
        return [(mp.mpf(0), mp.mpf(1))]
    if np.all(b > 1e-9 * scale) or np.all(b < -1e-9 * scale):                              # no root: one sign on [0, 1]
        return [(mp.mpf(0), mp.mpf(1))] if (b[0] > 0) == (sense == ABOVE) else []
    pw = [P._bernstein_to_power([mp.mpf(float(x)) for x in net[:, a]], mp) for a in range(3)]
    sq = [sum(t) for t in zip(*[P._polymul(p, p, mp) for p in pw])]
    sq[0] -= rhs
    big = max([abs(x) for x in sq] + [mp.mpf(0)])
    while sq and abs(sq[-1]) <= big * mp.mpf(10) ** -40:
        sq.pop()
    cuts = [mp.mpf(0), mp.mpf(1)]
    if len(sq) > 1:
        try:
            roots = mp.polyroots(sq[::-1], maxsteps=500, extraprec=400)
        except mp.NoConvergence:
            roots = [mp.mpf(float(r.real)) for r in np.roots([float(x) for x in sq[::-1]]) if abs(r.imag) < 1e-7]
        for r in roots:
            if abs(mp.im(r)) <= mp.mpf(10) ** -15 and 0 < mp.re(r) < 1:
                cuts.append(mp.re(r))
    cuts = sorted(set(cuts))
    val = (lambda s: mp.polyval(sq[::-1], s)) if sq else (lambda s: mp.mpf(0))
    out = []
    for a, b2 in zip(cuts[:-1], cuts[1:]):
        f = val((a + b2) / 2)
        if (f >= 0) if sense == ABOVE else (f <= 0):
            if out and out[-1][1] == a:
                out[-1] = (out[-1][0], b2)
            else:
                out.append((a, b2))
    return out


def true_within(ref, u, gate):
    """the true set of flight positions g = tr + s in [0, S] at which robot u's quantity is within the gate's level: a sorted list of disjoint closed
    intervals (mpf), adjacent ones merged (isolated touching points, sets of measure zero, are not listed)"""
    import mpmath as mp
    mp.mp.dps = 60
    q, sense, level = gate
    raw = ref.raw(u, q)
    out = []
    for tr in range(ref.S):
        den = mp.mpf(float(ref.den(u, q, np.array([tr]))[0]))
        rhs = mp.mpf(-1) if level < 0 else (mp.mpf(10) ** 400 if level == INF else (mp.mpf(float(level)) * den) ** 2)
        for a, b in _segment_within(raw[tr], rhs, sense, mp):
            a, b = tr + a, tr + b
            if out and out[-1][1] == a:
                out[-1] = (out[-1][0], b)
            else:
                out.append((a, b))
    return out


def value_at(ref, u, q, g, tr=None):
    """the quantity's true value at flight position g (mpf): peak_dynamics_ref.value_at's expression in segment tr (None: the segment that holds g; the jerk
    jumps at a piece boundary, so a caller that means the left-hand value there names the segment)"""
    import mpmath as mp
    tr = min(int(mp.floor(g)), ref.S - 1) if tr is None else tr
    mp.mp.dps = 60
    net = ref.raw(u, q)[tr]
    n = net.shape[0] - 1
    s = g - tr
    p = [sum(mp.binomial(n, i) * s ** i * (1 - s) ** (n - i) * mp.mpf(float(net[i, a])) for i in range(n + 1)) for a in range(3)]
    return mp.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2) / mp.mpf(float(ref.den(u, q, np.array([tr]))[0]))


def _minus(a, b):
    """interval lists (sorted, disjoint): a minus b, open pieces of positive length"""
    out = []
    for lo, hi in a:
        at = lo
        for x, y in b:
            if y <= at or x >= hi:
                continue
            if x > at:
                out.append((at, x))
            at = max(at, y)
        if at < hi:
            out.append((at, hi))
    return out


def contradictions(ref, u, gate, chains, truth_set):
    """the largest excess, relative to the robot's depth-0 ub of the quantity, by which the truth contradicts a certified class: a truly-within position
    outside every row (certified on the other side), or a position of an IN leaf that is truly outside.  The excess of a piece is the largest of
    |value - level| over 9 equally spaced positions of it.  Returns (excess of coverage, excess of IN leaves)."""
    import mpmath as mp
    q, sense, level = gate
    ub0 = ref.ub0(u, q)
    rows = [(mp.mpf(c[0][0]), mp.mpf(c[-1][1])) for c in chains]
    ins = [(mp.mpf(lf[0]), mp.mpf(lf[1])) for c in chains for lf in c if lf[2]]

    def excess(pieces):
        worst = 0.0
        for lo, hi in pieces:
            for tr in range(int(mp.floor(lo)), min(int(mp.ceil(hi)), ref.S)):                 # segment by segment: each piece with its own polynomial
                a, b = max(lo, mp.mpf(tr)), min(hi, mp.mpf(tr + 1))
                for k in range(9):
                    worst = max(worst, float(abs(value_at(ref, u, q, a + (b - a) * k / 8, tr) - mp.mpf(float(level)))))
        return worst / ub0 if ub0 > 0 else worst

    return excess(_minus(truth_set, rows)), excess(_minus(ins, truth_set))


# ---- constructed states ----------------------------------------------------------------------------------------------------------------------------

hover_state, line_state, scaled_state = P.hover_state, P.line_state, P.scaled_state


def line_speed(pkg, st, Pn):
    """the constant speed of line_state's flight"""
    ref = Ref(pkg, st, Pn, 8)
    return ref.ub0(0, SPEED)


def accel_state(pkg, scenes, c=0.5):
    """tiny(mode=0) with piece_time 1 flying x = c * sigma^2 along the x axis: uniform acceleration 2 c, speed 2 c t at real time t.  The control net is the
    least-squares solution of the Bezier points of sigma^2 piece by piece (the blossom of sigma^2 raised to degree 5: b_k = (C(k, 2) (i + 1)^2 + C(5 - k, 2) i^2 +
    k (5 - k) i (i + 1)) / 10 on piece i); the spline space holds every quadratic, the residual is asserted, but the solved variables are not dyadic: the
    closed form holds to 1e-9, not bit for bit, and the mpmath root stays the truth.  Returns (scene, state, c)."""
    scene = dict(scenes.tiny(mode=0))
    st = R.port_state(scene, 0)
    Pn = scene["P"]
    conv = pkg.host_tables(Pn, 8)[0]
    Tn = 3 * Pn + 3
    M, rhs = np.zeros((6 * Pn, Tn)), np.zeros(6 * Pn)
    for i in range(Pn):
        M[6 * i:6 * i + 6, 3 * i:3 * i + 6] = conv[i]
        for k in range(6):
            rhs[6 * i + k] = (math.comb(k, 2) * (i + 1) ** 2 + math.comb(5 - k, 2) * i ** 2 + k * (5 - k) * i * (i + 1)) / 10.0
    sol = np.linalg.lstsq(M, rhs, rcond=None)[0]
    assert np.abs(M @ sol - rhs).max() < 1e-11
    st["spline"][0] = 0.0
    st["spline"][0][0] = c * sol
    st["piece_time"][0] = 1.0
    assert R.valid_state(st, 1)
    return scene, st, c


# ---- the defaults, measured -----------------------------------------------------------------------------------------------------------------------

MODES = {"e2e_scn_a": 0, "e2e_scn_b": 1, "e2e_scn_c3": 1, "e2e_scn_b_coupled": 2}
FRACTIONS = (1.0, 0.9, 0.5)


def measurement_gates(ref, vel_limit=2.0, acc_limit=2.0):
    """all three quantities, both senses, levels 1.0 / 0.9 / 0.5 of the limit; for the jerk of the state's own largest depth-0 ub"""
    jerk = max(ref.ub0(u, JERK) for u in range(ref.U))
    return [(q, s, f * lim) for q, lim in ((SPEED, vel_limit), (ACCEL, acc_limit), (JERK, jerk)) for s in (ABOVE, BELOW) for f in FRACTIONS]


def measurement_states(pkg, names=E2E):
    """(label, state, P, res) of the named end states and of the same runs' iteration-0 states (_init)"""
    for name, scn in names:
        scene = getattr(pkg.scenes, scn)()
        final, Pn, res = T.e2e_state(name)
        init = R.port_state(dict(scene, mode=MODES.get(name, scene.get("mode", 1))), 0)
        yield name, final, Pn, res
        yield name + "_init", dict(spline=np.array(init["spline"]), piece_time=np.array(init["piece_time"])), Pn, res


def next_pow2(n):
    return 1 << max(n - 1, 0).bit_length()


def default_tolerance(pkg, names=E2E, vel_limit=2.0, acc_limit=2.0):
    """(frontier, per state: (rows, UNCERTAIN rows, TRUNCATED rows, largest live set after a round >= 1, largest leaf list, largest depth, widest bracket)): the
    default tol, max_depth = 40, the lists capped at MAX_WINDOWS only, over the state's 18 measurement gates.  The widest bracket is the largest of t_first_hi -
    t_first_lo and t_last_hi - t_last_lo over the CERTAIN rows.  The frontier is the next power of two >= 4 x the largest live set, at least 64."""
    per, widest = {}, 0
    tol = default_tol(vel_limit, acc_limit)
    for label, st, Pn, res in measurement_states(pkg, names):
        ref = Ref(pkg, st, Pn, res)
        traces = {}
        rows = ref.rows(measurement_gates(ref, vel_limit, acc_limit), tol, MAX_DEPTH, MAX_WINDOWS, traces=traces)
        live = max([t[1] for tr in traces.values() for t in tr if t[0] >= 1] + [0])
        kept = max([t[2] for tr in traces.values() for t in tr] + [0])
        sure = rows["flags"] & CERTAIN != 0
        width = max([0.0] + list(rows["t_first_hi"][sure] - rows["t_first_lo"][sure]) + list(rows["t_last_hi"][sure] - rows["t_last_lo"][sure]))
        per[label] = (len(rows["robot"]), int(np.sum(rows["flags"] & UNCERTAIN != 0)), int(np.sum(rows["flags"] & TRUNCATED != 0)), live, kept,
                      int(rows["depth"].max()) if len(rows["depth"]) else 0, float(width))
        widest = max(widest, live)
    return max(64, next_pow2(4 * max(widest, 1))), per


def measured_excess(pkg, states, vel_limit=2.0, acc_limit=2.0, max_robots=None):
    """the largest contradiction (coverage, IN leaves) over `states` = [(label, state, P, res)] at the measurement's gates and the default tol, in units of
    eps = 2^-53 of the depth-0 ub"""
    worst = [0.0, 0.0]
    tol = default_tol(vel_limit, acc_limit)
    for label, st, Pn, res in states:
        ref = Ref(pkg, st, Pn, res)
        gates = measurement_gates(ref, vel_limit, acc_limit)
        for u in range(ref.U if max_robots is None else min(ref.U, max_robots)):
            for k, gate in enumerate(gates):
                leaves = {}
                ref.gate_rows(u, k, gate, tol, MAX_DEPTH, MAX_WINDOWS, None, leaves)
                cov, inn = contradictions(ref, u, gate, leaves.get((u, k), []), true_within(ref, u, gate))
                worst = [max(worst[0], cov / EPS), max(worst[1], inn / EPS)]
    return worst
