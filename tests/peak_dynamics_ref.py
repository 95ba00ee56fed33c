"""Reference values for tj_peak_dynamics that share no code with csrc/kernels_peak_dynamics.h (plain module: no fixtures, no tests).

  Ref.records         the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_peak_dynamics.py.  Hulls by
                      audit_ref.hulls_of (hull_entry's sums); the raw derivative nets in hull_speed's / hull_accel's expressions (and the third difference
                      for the jerk); the net of a window by audit_timed_ref.bez_restrict's blossoming written for any degree, ALWAYS from the raw derivative
                      net (elementwise: the same IEEE operations); ub(W) = max_i norm3(c_i) / den, at(W) = the larger of norm3(c_0) / den (at sa) and
                      norm3(c_n) / den (at sb), den = w pt | w w pt pt | w w w pt pt pt left to right; the search level by level:
                        seeds     every segment, window [0, 1]; best = the first attained candidate in the order (larger value, smaller segment, smaller s);
                                  live = {ub > best.value}
                        round d   every live item is halved at sm = 0.5 * (sa + sb); both children are evaluated from the raw net; best over (best,
                                  children); live = children with ub > best.value -- against the round's FINAL best
                        bracket   lo = best.value, hi = max(best.value, max ub over live)
                        stop      hi - lo <= tol * hi | live empty | d == max_depth | more than max_windows live (TRUNCATED: the record of the last
                                  completed round -- at seeding the seeds' own bracket; `windows` still counts the round that overflowed)
                      the length: per segment the 2^L windows of the raw v net, len_lo = h * norm3(mean c), len_hi = (h * sum norm3(c_i)) / 5, a segment's
                      windows summed in the balanced binary tree over adjacent pairs, the segments one after the other.
  truth               mpmath: per segment the polynomial |q(s)|^2 of the raw net, the real roots of its derivative in [0, 1] and the ends; the length by
                      mpmath.quad of |v(s)|.  Segments are shortlisted in np.longdouble first (a dense grid: within 1e-3 of the robot's largest sample).
  constructed states  line, hover, scaled: each builder asserts its precondition on the CPU.
  default_tolerance   the measured TJ_PEAK_TOL, TJ_PEAK_FRONTIER and TJ_PEAK_LENGTH_LEVELS, the manner of obstacle_approach_ref.default_tolerance."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
from obstacle_approach_ref import E2E, floor_of

LD = np.longdouble
CONVERGED, TRUNCATED = 4, 8
DYN_SPEED, DYN_SPEED_OK, DYN_ACCEL, DYN_ACCEL_OK = 1, 2, 4, 8
MAX_DEPTH = 40
MAX_LENGTH_LEVELS = 12
QUANTITIES = ("speed", "accel", "jerk")
DEGREE = (4, 3, 2)
PEAK_FIELDS = ("lo", "hi", "time", "segment", "depth", "windows", "flags")
FIELDS = tuple(q + "_" + n for q in QUANTITIES for n in PEAK_FIELDS) + ("length_lo", "length_hi", "duration", "time_scale", "length_levels", "flags")
DOUBLES = tuple(q + "_" + n for q in QUANTITIES for n in PEAK_FIELDS[:3]) + ("length_lo", "length_hi", "duration", "time_scale")


def norm3(d):
    """dev_common.h norm3 on [...][3]"""
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def raw_net(H, q):
    """H [S][6][3] -> the raw derivative net [S][n + 1][3] of quantity q: hull_speed's, hull_accel's expressions and the third difference"""
    if q == 0:
        return np.stack([5 * (H[:, i + 1] - H[:, i]) for i in range(5)], axis=1)
    if q == 1:
        return np.stack([20 * (H[:, i + 2] - 2 * H[:, i + 1] + H[:, i]) for i in range(4)], axis=1)
    return np.stack([60 * (H[:, i + 3] - 3 * H[:, i + 2] + 3 * H[:, i + 1] - H[:, i]) for i in range(3)], axis=1)


def bez_restrict(p, sa, sb):
    """p [n][N][3], sa / sb [n] -> the Bezier nets over [sa, sb] of a curve of degree N - 1: o[i] = blossom(sa x (N - 1 - i), sb x i).  Row s of the triangle
    (s steps at sa) has N - s points; N - 1 - s steps at sb take it to o[N - 1 - s].  Every step is (1 - s) * x + s * y, left to right."""
    N = p.shape[1]
    sa = np.asarray(sa, dtype=np.float64)[:, None]; sb = np.asarray(sb, dtype=np.float64)[:, None]
    ua, ub = 1 - sa, 1 - sb
    r = [p[:, m, :] for m in range(N)]
    o = [None] * N
    for s in range(N):
        t = list(r[:N - s])
        for k in range(N - 1 - s, 0, -1):
            t = [ub * t[m] + sb * t[m + 1] for m in range(k)]
        o[N - 1 - s] = t[0]
        if s < N - 1:
            r = [ua * r[m] + sa * r[m + 1] for m in range(N - 1 - s)]
    return np.stack(o, axis=1)


def tree_sum(x):
    """the balanced binary tree over adjacent pairs of 2^L values"""
    x = np.asarray(x, dtype=np.float64)
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return float(x[0])


class Ref:
    """the restatement on one state"""

    def __init__(self, pkg, st, P, res):
        self.pt, self.P, self.S, self.rf = np.asarray(st["piece_time"], dtype=np.float64), P, P * res, float(res)
        self.H = np.ascontiguousarray(R.hulls_of(pkg, np.asarray(st["spline"], dtype=np.float64), P, res))
        self.U = self.H.shape[0]
        k = np.arange(self.S) % res
        self.w = (k + 1) / float(res) - k / float(res)                                  # the table value (seg_weight), not 1 / res
        self._raw, self._len = {}, {}

    def raw(self, u, q):
        if (u, q) not in self._raw:
            self._raw[(u, q)] = raw_net(self.H[u], q)
        return self._raw[(u, q)]

    def den(self, u, q, tr):
        w, pt = self.w[tr], float(self.pt[u])
        return w * pt if q == 0 else (w * w * pt * pt if q == 1 else w * w * w * pt * pt * pt)

    def evaluate(self, u, q, tr, sa, sb):
        """items (tr[n], sa[n], sb[n]) -> ub[n], at[n], s[n] (the parameter of the attained sample: sa on a tie)"""
        net = bez_restrict(self.raw(u, q)[tr], sa, sb)
        v = norm3(net) / self.den(u, q, tr)[:, None]
        first = v[:, 0] >= v[:, -1]
        return v.max(axis=1), np.where(first, v[:, 0], v[:, -1]), np.where(first, sa, sb)

    def time_of(self, u, tr, s):
        return ((tr + s) / self.rf) * float(self.pt[u])

    def search(self, u, q, tol, max_depth, max_windows, trace=None):
        """one tj_peak as a dict (+ s, live_empty, truncated); trace (a list) receives (depth, lo, hi, live) of every completed round"""
        tr = np.arange(self.S)
        sa, sb = np.zeros(self.S), np.ones(self.S)
        ub, at, s = self.evaluate(u, q, tr, sa, sb)
        windows = self.S

        def better(best, tr, at, s):
            k = np.lexsort((s, tr, -at))[0]
            return min(best, (-float(at[k]), int(tr[k]), float(s[k])))

        best = better((math.inf, math.inf, math.inf), tr, at, s)
        keep = ub > -best[0]
        live = (tr[keep], sa[keep], sb[keep], ub[keep])
        rec = dict(best=best, hi=max([-best[0]] + live[3].tolist()), depth=0)
        truncated = len(live[0]) > max_windows
        if trace is not None:
            trace.append((0, -best[0], rec["hi"], len(live[0])))
        d = 0
        while not truncated:
            lo, hi = -rec["best"][0], rec["hi"]
            if hi - lo <= tol * hi or len(live[0]) == 0 or d == max_depth:
                break
            ltr, sa, sb, _ = live
            sm = 0.5 * (sa + sb)
            ktr, ksa, ksb = np.concatenate([ltr, ltr]), np.concatenate([sa, sm]), np.concatenate([sm, sb])
            kub, kat, ks = self.evaluate(u, q, ktr, ksa, ksb)
            windows += len(ktr)
            best = better(rec["best"], ktr, kat, ks)
            keep = kub > -best[0]
            if int(keep.sum()) > max_windows:
                truncated = True
                break
            d += 1
            live = (ktr[keep], ksa[keep], ksb[keep], kub[keep])
            rec = dict(best=best, hi=max([-best[0]] + live[3].tolist()), depth=d)
            if trace is not None:
                trace.append((d, -best[0], rec["hi"], len(live[0])))
        nlo, seg, s_u = rec["best"]
        lo, hi = -nlo, rec["hi"]
        empty = len(live[0]) == 0 and not truncated
        return dict(lo=lo, hi=hi, time=self.time_of(u, seg, s_u), segment=seg, depth=rec["depth"], windows=windows, s=s_u,
                    flags=(CONVERGED if hi - lo <= tol * hi or empty else 0) | (TRUNCATED if truncated else 0))

    def length(self, u, L):
        """(length_lo, length_hi) of robot u at level L"""
        if (u, L) not in self._len:
            self._len[(u, L)] = self._length(u, L)
        return self._len[(u, L)]

    def _length(self, u, L):
        n = 1 << L
        h = 1.0 / n
        sa = np.arange(n) * h
        sb = (np.arange(n) + 1) * h
        raw = self.raw(u, 0)
        lo = hi = 0.0
        for tr in range(self.S):
            c = bez_restrict(np.broadcast_to(raw[tr], (n, 5, 3)), sa, sb)
            mean = ((((c[:, 0] + c[:, 1]) + c[:, 2]) + c[:, 3]) + c[:, 4]) / 5
            nn = norm3(c)
            lo += tree_sum(h * norm3(mean))
            hi += tree_sum((h * ((((nn[:, 0] + nn[:, 1]) + nn[:, 2]) + nn[:, 3]) + nn[:, 4])) / 5)
        return lo, hi

    def duration(self, u):
        dur = 0.0
        for _ in range(self.P):
            dur += 1.0 * float(self.pt[u])
        return dur

    def records(self, tol, max_depth, max_windows, L, vel_limit, acc_limit, owned=None, traces=None, raw=None):
        """per robot the record's fields under Solver.peak_dynamics' keys (robots outside `owned`: zero).  tol, max_depth, max_windows, L: the resolved values.
        traces / raw (dicts) receive per (u, quantity) the rounds' trace / the search's own dict"""
        out = {n: np.zeros(self.U, dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}
        for u in (range(self.U) if owned is None else owned):
            pk = []
            for q, name in enumerate(QUANTITIES):
                tr = [] if traces is not None else None
                r = self.search(u, q, float(tol), max_depth, max_windows, tr)
                pk.append(r)
                for n in PEAK_FIELDS:
                    out[name + "_" + n][u] = r[n]
                if traces is not None:
                    traces[(u, q)] = tr
                if raw is not None:
                    raw[(u, q)] = r
            out["length_lo"][u], out["length_hi"][u] = self.length(u, L)
            out["duration"][u] = self.duration(u)
            out["length_levels"][u] = L
            out["time_scale"][u] = max(pk[0]["hi"] / vel_limit, math.sqrt(pk[1]["hi"] / acc_limit))
            out["flags"][u] = ((DYN_SPEED if pk[0]["lo"] >= vel_limit else 0) | (DYN_SPEED_OK if pk[0]["hi"] < vel_limit else 0) |
                               (DYN_ACCEL if pk[1]["lo"] >= acc_limit else 0) | (DYN_ACCEL_OK if pk[1]["hi"] < acc_limit else 0))
        return out


# ---- the truth: the polynomial itself ---------------------------------------------------------------------------------------------------------------

def _bernstein_to_power(c, mp):
    """Bezier coefficients c[0..n] (mpf) -> power-basis coefficients a[0..n]: sum_k a_k s^k"""
    n = len(c) - 1
    return [mp.binomial(n, k) * sum((-1) ** (k - i) * mp.binomial(k, i) * c[i] for i in range(k + 1)) for k in range(n + 1)]


def _polymul(a, b, mp):
    out = [mp.mpf(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def _segment_peak(net, mp):
    """net [n + 1][3] (float64, the raw net) -> (max over s in [0, 1] of |q(s)|, argmax s) in mpmath: ends and the real roots of d/ds |q|^2"""
    pw = [_bernstein_to_power([mp.mpf(float(x)) for x in net[:, a]], mp) for a in range(3)]
    sq = [sum(t) for t in zip(*[_polymul(p, p, mp) for p in pw])]
    der = [k * sq[k] for k in range(1, len(sq))]
    big = max([abs(x) for x in der] + [mp.mpf(0)])
    while der and abs(der[-1]) <= big * mp.mpf(10) ** -40:
        der.pop()
    cand = [mp.mpf(0), mp.mpf(1)]
    if len(der) > 1:
        try:
            roots = mp.polyroots(der[::-1], maxsteps=500, extraprec=400)
        except mp.NoConvergence:
            roots = [mp.mpf(float(r.real)) for r in np.roots([float(x) for x in der[::-1]]) if abs(r.imag) < 1e-7]
        for r in roots:
            if abs(mp.im(r)) <= mp.mpf(10) ** -15 and -mp.mpf(10) ** -15 <= mp.re(r) <= 1 + mp.mpf(10) ** -15:
                cand.append(min(max(mp.re(r), mp.mpf(0)), mp.mpf(1)))
    val = lambda s: mp.sqrt(max(mp.polyval(sq[::-1], s), mp.mpf(0)))
    return max((val(s), -s) for s in cand)


def value_at(ref, u, q, tr, s):
    """|q(s)| / den of segment tr in mpmath (den: the double the restatement divides by)"""
    import mpmath as mp
    mp.mp.dps = 60
    net = ref.raw(u, q)[tr]
    n = net.shape[0] - 1
    s = mp.mpf(float(s))
    p = [sum(mp.binomial(n, i) * s ** i * (1 - s) ** (n - i) * mp.mpf(float(net[i, a])) for i in range(n + 1)) for a in range(3)]
    return mp.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2) / mp.mpf(float(ref.den(u, q, np.array([tr]))[0]))


def truth(ref, u, q):
    """(peak, segment, s) of robot u's quantity q: the shortlist (segments whose largest sample on a 33-point grid in np.longdouble is within 1e-3 of the
    robot's largest) by mpmath's roots"""
    import mpmath as mp
    mp.mp.dps = 60
    raw = ref.raw(u, q)
    n = raw.shape[1] - 1
    s = np.linspace(LD(0), LD(1), 33, dtype=LD)
    B = np.stack([LD(math.comb(n, i)) * s ** i * (1 - s) ** (n - i) for i in range(n + 1)])              # [n + 1][33]
    p = np.einsum("ik,sia->ska", B, raw.astype(LD))
    den = ref.den(u, q, np.arange(ref.S)).astype(LD)
    val = (np.sqrt((p * p).sum(axis=2)) / den[:, None]).max(axis=1)
    ubd = (np.sqrt((raw.astype(LD) ** 2).sum(axis=2)) / den[:, None]).max(axis=1)                       # the hull bound: no segment above the shortlist is missed
    best = (mp.mpf(-1), -1, 0.0)
    for tr in np.flatnonzero((val >= val.max() * (1 - LD(1e-3))) | (ubd >= val.max())):
        v, ns = _segment_peak(raw[tr], mp)
        v = v / mp.mpf(float(den[tr]))
        if v > best[0]:
            best = (v, int(tr), float(-ns))
    return best


def true_length(ref, u):
    """the path length of robot u: mpmath.quad of |v(s)| per segment (split in four: the integrand is smooth but for a stop)"""
    import mpmath as mp
    mp.mp.dps = 25
    raw = ref.raw(u, 0)
    total = mp.mpf(0)
    for tr in range(ref.S):
        c = [[mp.mpf(float(x)) for x in raw[tr, :, a]] for a in range(3)]

        def f(s):
            b = [mp.binomial(4, i) * s ** i * (1 - s) ** (4 - i) for i in range(5)]
            return mp.sqrt(sum(sum(bi * ci for bi, ci in zip(b, c[a])) ** 2 for a in range(3)))

        total += mp.quad(f, mp.linspace(0, 1, 5), method="gauss-legendre")
    return total


def chord_sum(pkg, st, P, res, u, step=0.1):
    """log_data's `ccd len` (Main/multiPathPlanning3D.cpp:31-76) restated: the chords between the positions at sigma = 0, step, 2 step, ... < P and the
    last one to sigma = P, in np.longdouble.  Inscribed in the curve: never longer than it."""
    n = int(math.ceil(P / step - 1e-9))
    sig = np.minimum(np.arange(n + 1, dtype=LD) * LD(step), LD(P))
    p = T.curve_at(pkg, st["spline"][u], 1.0, P, res, sig)
    d = np.diff(p, axis=0)
    return float(np.sqrt((d * d).sum(axis=1)).sum())


# ---- constructed states ----------------------------------------------------------------------------------------------------------------------------

def line_state(pkg, scenes):
    """tiny(mode=0) flying x = 5 * sigma along the x axis: the control net of that line (audit_timed_ref.linear_nets) is a vector of integers, the basis
    table is dyadic, so every hull point is exact and -- asserted here on the restatement's own nets -- every velocity control vector of every segment has
    the same bits, and every acceleration and jerk control vector is zero.  Returns (scene, state)."""
    scene = dict(scenes.tiny(mode=0))
    st = R.port_state(scene, 0)
    gs = T.linear_nets(pkg, scene["P"], 8)[1]
    net = np.round(5 * gs)
    assert np.abs(net - 5 * gs).max() < 1e-9
    st["spline"][0] = 0.0
    st["spline"][0][0] = net
    assert R.valid_state(st, 1)
    ref = Ref(pkg, st, scene["P"], 8)
    v = ref.raw(0, 0)
    assert np.all(v == v[0, 0]) and v[0, 0, 0] > 0 and not ref.raw(0, 1).any() and not ref.raw(0, 2).any()
    return scene, st


def hover_state(pkg, scenes):
    """tiny(mode=0) with all control points equal to (1, 2, 3)"""
    scene = dict(scenes.tiny(mode=0))
    st = R.port_state(scene, 0)
    st["spline"][0] = np.array([1.0, 2.0, 3.0])[:, None]
    assert R.valid_state(st, 1)
    return scene, st


def scaled_state(st, u, k):
    """`st` with robot u's control net multiplied by k: its speed, acceleration and jerk scale by k (up to rounding; the caller asserts the side of the
    limit it wanted on the restatement)"""
    st2 = {n: np.array(v) for n, v in st.items()}
    st2["spline"][u] = st2["spline"][u] * k
    return st2


# ---- the defaults, measured ------------------------------------------------------------------------------------------------------------------------

def next_pow2(n):
    return 1 << max(n - 1, 0).bit_length()


def default_tolerance(pkg, names=E2E, length_levels=6):
    """(relative widths per depth 0..40, floor depth, tolerance, largest live set up to the floor, frontier, length widths per level 0..length_levels (the
    rest 0: the level looked for lies below), level, live sets per depth): tol = 0
    and max_depth = 40 on the named end states; per depth the largest (hi - lo) / hi over robots and quantities (a search that has ended keeps its last
    bracket).  The floor: obstacle_approach_ref.floor_of -- on these states every live set empties (width 0 from depth 31 on), so it is the last depth
    with a positive width.  The largest live set is taken over the rounds up to the floor; the searches run 4096 windows wide, and none is truncated."""
    widths, lives = [0.0] * (MAX_DEPTH + 1), [0] * (MAX_DEPTH + 1)
    lw = [0.0] * (MAX_LENGTH_LEVELS + 1)
    for name, _ in names:
        st, P, res = T.e2e_state(name)
        ref = Ref(pkg, st, P, res)
        for u in range(ref.U):
            for q in range(3):
                tr = []
                ref.search(u, q, 0.0, MAX_DEPTH, 4096, tr)
                for d in range(MAX_DEPTH + 1):
                    _, l, h, n = tr[min(d, len(tr) - 1)]
                    widths[d] = max(widths[d], (h - l) / h if h > 0 else 0.0)
                    if d < len(tr):
                        lives[d] = max(lives[d], n)
            for L in range(length_levels + 1):
                lo, hi = ref.length(u, L)
                lw[L] = max(lw[L], (hi - lo) / hi if hi > 0 else 0.0)
    floor = floor_of(widths)
    tol = float("1e%d" % math.ceil(math.log10(10 * widths[floor])))
    biggest = max(lives[:floor + 1])
    level = min(L for L in range(length_levels + 1) if lw[L] < 1e-6)
    return widths, floor, tol, biggest, max(1024, next_pow2(4 * biggest)), lw, level, lives
