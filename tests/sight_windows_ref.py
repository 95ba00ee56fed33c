"""Reference values for tj_sight_windows that share no code with csrc/kernels_sight_windows.h (plain module: no fixtures, no tests).

  Ref.rows            the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_sight_windows.py.  Hulls are
                      audit_ref.hulls_of's, the restriction audit_timed_ref.bez_restrict from the RAW hulls, the cuts audit_timed_ref.pieces_of at level 0 (the
                      windows proximity_ref's seeds are made of), the GJK the ORACLE's (any point counts: the 12-point hull of two nets is body 1).  Its own:
                        body        L(W) = a_0..a_5, b_0..b_5: both nets over the same time window (a hovering partner and a station: six equal points)
                        candidates  the walk's leaf predicate by brute force over ALL primitives: the primitive's box within dist of L's box on every axis
                        per p       lo_p (certified |v| over all 12 points, else 0); sample(a_0, b_0, p) and sample(a_5, b_5, p) with their lambdas; ub_p
                        class       OUT: every candidate has lo_p > dist (an empty set too) | IN: some ub_p <= dist | MIXED: the rest (in this order)
                        search      per (link, segment of a): the seeds in time order, IN seeds are leaves, MIXED seeds live; rounds as proximity_ref's
                        merge       per link the leaves of all its segments by ca; adjacent iff prev.cb == next.ca; a row per maximal chain
  truth               nothing of GJK or subdivision in it: both ends of the link from `convert` in np.longdouble on a dense time grid, the segment between
                      them against every primitive by brute force (a point: its foot on the segment; a triangle: the ends against the triangle, the segment
                      against the three edges, and a piercing test).
  constructed states  pillar, graze_out, graze_in, station, hover, staggered, cluster: `built`.
  default_tolerance   the measured tables of the header, TJ_SIGHT_FRONTIER and TJ_SIGHT_PROJECTIONS."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import obstacle_approach_ref as O

LD = np.longdouble
CERTAIN, UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED = 1, 2, 4, 8, 16, 32
MAX_DEPTH, MAX_WINDOWS, TOL_FRACTION = 40, 1024, 0.01
DOUBLES = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "closest", "closest_time")
FIELDS = DOUBLES + ("link", "robot", "partner", "index", "leaves", "depth", "flags", "windows")
OUT, IN, MIXED = 0, 1, 2
INF = math.inf


def default_tol(dist, offset, vel_limit):
    """what tol < 0 selects: the time a point at the speed limit needs for 1 % of dist (of offset where dist is infinite)"""
    return (TOL_FRACTION * (offset if dist == INF else dist)) / vel_limit


def default_links(U, n_stations):
    """what links=None selects: every directed robot pair in (a, b) order, then per robot every station"""
    return [(a, b) for a in range(U) for b in range(U) if b != a] + [(a, -1 - s) for a in range(U) for s in range(n_stations)]


def _norms(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


class Ref(O.Ref):
    """the restatement on one state, one obstacle set and one set of stations; evaluations are kept per (a, b, tr, j, ca, cb, dist)"""

    def __init__(self, pkg, pr, st, P, res, X, stations=None, projections=None, frontier=None):
        super().__init__(pkg, pr, st, P, res, X)
        self.P, self.res = P, res
        self.HX = np.concatenate([self.H, np.repeat(self.H[:, self.S - 1:self.S, 5:6, :], 6, axis=2)], axis=1)   # row S: the hover body
        self.stations = np.zeros((0, 3)) if stations is None else np.ascontiguousarray(stations, dtype=np.float64).reshape(-1, 3)
        self.K = pkg.SIGHT_PROJECTIONS if projections is None else projections
        self.frontier = pkg.SIGHT_FRONTIER if frontier is None else frontier
        self._evals, self._bases = {}, {}

    # ---- distances of points Z [n][3] from the primitives near[n] ----
    def _pd(self, Z, near):
        if not self.tri:
            return _norms(Z - self.X[near])
        return _norms(self._gjk1(Z, near))

    def _gjk1(self, Z, near):
        """the oracle's GJK of the one-point body {z} against triangle near[k]: v = z - (its witness on the triangle)"""
        Z = np.ascontiguousarray(Z)
        Xi = np.ascontiguousarray(self.Xv[near])
        V = np.zeros((len(near), 3))
        zb, xb, vb, f = Z.ctypes.data, Xi.ctypes.data, V.ctypes.data, self.g.f
        for k in range(len(near)):
            f(1, zb + k * 24, 3, xb + k * 72, vb + k * 24)
        return V

    def _sample(self, x, y, near):
        """sample(x, y, p) for every p of near: (value [n], lambda [n])"""
        e = y - x
        ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]

        def proj(Zp):
            if ee == 0.0:
                return np.zeros(len(near))
            return np.minimum(np.maximum((((Zp[:, 0] - x[0]) * e[0] + (Zp[:, 1] - x[1]) * e[1]) + (Zp[:, 2] - x[2]) * e[2]) / ee, 0.0), 1.0)

        if not self.tri:
            lam = proj(self.X[near])
        else:
            lam = np.full(len(near), 0.5)
            for _ in range(self.K):
                Z = x[None, :] + lam[:, None] * e[None, :]
                lam = proj(Z - self._gjk1(Z, near))
        return self._pd(x[None, :] + lam[:, None] * e[None, :], near), lam

    def body_b(self, b, j, ra, rb):
        if b < 0:
            return np.repeat(self.stations[-1 - b][None, :], 6, axis=0)
        if j >= self.S:
            return self.HX[b, self.S]
        return T.bez_restrict(self.HX[b, j][None], [ra], [rb])[0]

    def window(self, a, b, tr, j, ca, cb, dist):
        """(class, h0, i0, h5, i5) of the window [ca, cb] in segment tr of a and segment j of b (j == S: b hovers, or is a station)"""
        key = (a, b, tr, j, ca, cb, dist)
        if key not in self._bases:
            self._bases[key] = self._base(a, b, tr, j, ca, cb, dist)
        base = self._bases[key]
        if base is None:
            return OUT, INF, -1, INF, -1
        key += (self.K if self.tri else 0,)                                                      # (only a triangle's samples depend on the projections)
        if key not in self._evals:
            self._evals[key] = self._classify(dist, *base)
        return self._evals[key]

    def _base(self, a, b, tr, j, ca, cb, dist):
        """(A, B, near) of a window that is not OUT, else None: what does not depend on the number of projections"""
        rf, ptu = self.rf, float(self.pt[a])
        T0u, T1u = (tr / rf) * ptu, ((tr + 1) / rf) * ptu
        lenu = T1u - T0u
        sa, sb = T.clamp01((ca - T0u) / lenu), T.clamp01((cb - T0u) / lenu)
        ra = rb = 0.0
        if b >= 0:
            ptq = float(self.pt[b])
            Tj, Tj1 = (j / rf) * ptq, ((j + 1) / rf) * ptq
            lenq = Tj1 - Tj
            ra, rb = T.clamp01((ca - Tj) / lenq), T.clamp01((cb - Tj) / lenq)
        A = T.bez_restrict(self.H[a, tr][None], [sa], [sb])[0]
        B = self.body_b(b, j, ra, rb)
        L = np.ascontiguousarray(np.concatenate([A, B], axis=0))                                  # [12][3]
        lo, hi = L.min(axis=0), L.max(axis=0)
        near = np.flatnonzero(~((self.phi + dist < lo) | (self.plo > hi + dist)).any(axis=1)) if self.N else np.zeros(0, dtype=np.int64)
        n = len(near)
        if n == 0:
            return None
        Xi = np.ascontiguousarray(self.Xv[near])                                                # [n][nv][3]
        f, nv = self.g.f, self.nv
        V = np.zeros((n, 3))
        lb, xb, vb = L.ctypes.data, Xi.ctypes.data, V.ctypes.data
        for k in range(n):
            f(12, lb, nv, xb + k * nv * 24, vb + k * 24)
        m = np.full(n, np.inf)
        for i in range(12):
            for v in range(nv):
                d = L[i][None, :] - Xi[:, v]
                m = np.minimum(m, (V[:, 0] * d[:, 0] + V[:, 1] * d[:, 1]) + V[:, 2] * d[:, 2])
        lo_p = np.where(m > 0.0, _norms(V), 0.0)
        return None if bool(np.all(lo_p > dist)) else (A, B, near)

    def _classify(self, dist, A, B, near):
        h0, l0 = self._sample(A[0], B[0], near)
        h5, l5 = self._sample(A[5], B[5], near)
        # ub_p at lambda0_p is looked at only where h0_p <= dist (its i = 0 term IS h0_p), likewise at lambda5_p: the smaller of those evaluated
        E = B - A
        is_in = False
        for h, lam in ((h0, l0), (h5, l5)):
            sel = np.flatnonzero(h <= dist)
            if is_in or len(sel) == 0:
                continue
            ub = np.zeros(len(sel))
            for i in range(6):
                ub = np.maximum(ub, self._pd(A[i][None, :] + lam[sel][:, None] * E[i][None, :], near[sel]))
            is_in = bool(np.any(ub <= dist))
        k0 = np.lexsort((near, h0))[0]
        k5 = np.lexsort((near, h5))[0]
        return (IN if is_in else MIXED), float(h0[k0]), int(near[k0]), float(h5[k5]), int(near[k5])

    def seeds(self, a, b, tr):
        """the level-0 windows (j, ca, cb) of segment tr of a against b, in time order"""
        if b < 0:
            ptu = float(self.pt[a])
            return [(self.S, ((tr + 0.0) / self.rf) * ptu, ((tr + 1.0) / self.rf) * ptu)]
        return [(j, ca, cb) for (_, j, ca, cb, _, _, _, _) in T.pieces_of(self.pt, self.P, self.res, a, tr, b, 0)]

    def search(self, a, b, tr, dist, tol, max_depth, max_windows, trace=None):
        """the leaves of segment tr of a on the link (a, b): dict(leaves sorted by ca: (ca, cb, h0, i0, h5, i5, is IN), depth, windows, truncated).  trace
        receives (depth, size of the live set, size of the leaf list) after the seeds and after every round, the overflowing one included"""
        seeds = self.seeds(a, b, tr)
        windows = len(seeds)
        kept, live = [], []
        for (j, ca, cb) in seeds:
            c, h0, i0, h5, i5 = self.window(a, b, tr, j, ca, cb, dist)
            if c == IN:
                kept.append((ca, cb, h0, i0, h5, i5, True))
            elif c == MIXED:
                live.append((j, ca, cb, h0, i0, h5, i5))
        truncated = len(live) > max_windows or len(kept) > max_windows
        if trace is not None:
            trace.append((0, len(live), len(kept)))
        d = 0
        while not truncated and live and d < max_depth:
            new, nxt = list(kept), []
            for (j, ca, cb, h0, i0, h5, i5) in live:
                cm = 0.5 * (ca + cb)
                if cb - ca <= tol or not (ca < cm < cb):
                    new.append((ca, cb, h0, i0, h5, i5, False))
                    continue
                for ka, kb in ((ca, cm), (cm, cb)):
                    c, g0, j0, g5, j5 = self.window(a, b, tr, j, ka, kb, dist)
                    windows += 1
                    if c == IN:
                        new.append((ka, kb, g0, j0, g5, j5, True))
                    elif c == MIXED:
                        nxt.append((j, ka, kb, g0, j0, g5, j5))
            if trace is not None:
                trace.append((d + 1, len(nxt), len(new)))
            if len(nxt) > max_windows or len(new) > max_windows:
                truncated = True
                break
            d += 1
            kept, live = new, nxt
        leaves = kept + [w[1:] + (False,) for w in live]
        return dict(leaves=sorted(leaves), depth=d, windows=windows, truncated=truncated)

    def link_rows(self, k, a, b, dist, tol, max_depth, max_windows, traces=None, leaves_out=None):
        segs = []
        for tr in range(self.S):
            trace = [] if traces is not None else None
            segs.append(self.search(a, b, tr, dist, tol, max_depth, max_windows, trace))
            if traces is not None:
                traces[(k, tr)] = trace
        windows = sum(s["windows"] for s in segs)
        flat = [(tr,) + lf for tr in range(self.S) for lf in segs[tr]["leaves"]]
        chains = []
        for i, lf in enumerate(flat):
            if i:
                p = flat[i - 1]
                assert p[1] < lf[1] and p[2] <= lf[1], (p, lf)                                  # distinct, disjoint, in time order across segments
            if i and flat[i - 1][2] == lf[1]:
                chains[-1].append(lf)
            else:
                chains.append([lf])
        t_end = ((self.S - 1 + 1) / self.rf) * float(self.pt[a])
        rows = []
        for chain in chains:
            sure, within, best = [], 0.0, (INF, INF, INF)
            for tr, ca, cb, h0, i0, h5, i5, is_in in chain:
                if is_in:
                    sure += [ca, cb]
                    within += cb - ca
                else:
                    if h0 <= dist:
                        sure.append(ca)
                    if h5 <= dist:
                        sure.append(cb)
                best = min(best, (h0, ca, i0), (h5, cb, i5))
            first_lo, last_hi = chain[0][1], chain[-1][2]
            first_hi, last_lo = (min(sure), max(sure)) if sure else (-1.0, -1.0)
            at_start, at_end = first_lo == 0.0, last_hi == t_end
            trs = sorted({lf[0] for lf in chain})
            flags = ((CERTAIN if sure else UNCERTAIN) | (AT_START if at_start else 0) | (AT_END if at_end else 0) |
                     (TRUNCATED if any(segs[tr]["truncated"] for tr in trs) else 0))
            if sure and (at_start or first_hi - first_lo <= tol) and (at_end or last_hi - last_lo <= tol):
                flags |= RESOLVED
            found = best[2] != INF
            rows.append(dict(t_first_lo=first_lo, t_first_hi=first_hi, t_last_lo=last_lo, t_last_hi=last_hi, within_lo=within, closest=best[0],
                             closest_time=best[1] if found else -1.0, link=k, robot=a, partner=b, index=best[2] if found else -1, leaves=len(chain),
                             depth=max(segs[tr]["depth"] for tr in trs), flags=flags, windows=windows))
            if leaves_out is not None:
                leaves_out.setdefault(k, []).append([(ca, cb, is_in, h0, h5) for _, ca, cb, h0, _, h5, _, is_in in chain])
        return rows

    def rows(self, links, dist, tol, max_depth=MAX_DEPTH, max_windows=None, traces=None, leaves=None):
        """the rows as a dict of numpy arrays [n] in (link, t_first_lo) order.  links: None (default_links) or [(a, b)]; dist, tol, max_depth, max_windows:
        the resolved values.  traces: per (link, segment) the search's trace; leaves: per link, per row the chain as (ca, cb, is IN, h0, h5)."""
        max_windows = self.frontier if max_windows is None else max_windows
        links = default_links(self.U, len(self.stations)) if links is None else [(int(a), int(b)) for a, b in links]
        out = []
        if self.N:
            for k, (a, b) in enumerate(links):
                out += self.link_rows(k, a, b, float(dist), float(tol), max_depth, max_windows, traces, leaves)
        return {n: np.array([r[n] for r in out], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}


def ref_of(pkg, pr, st, P, res, X, stations=None, **kw):
    return Ref(pkg, pr, st, P, res, X, stations, **kw)


# ---- the truth: the flown link itself against every primitive ------------------------------------------------------------------------------------

def _seg_seg(p0, p1, q0, q1):
    """squared distance of segments [p0, p1] (each [n][3]) from segments [q0, q1] (each [m][3]) -> [n][m], np.longdouble: the smallest of the four
    end-against-segment distances and, where the common perpendicular's feet lie inside both, its length"""
    def pt_seg(p, a, b):
        ab = b - a
        den = (ab * ab).sum(-1)
        t = np.clip(np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1), 0), 0, 1)
        d = p - (a + t[..., None] * ab)
        return (d * d).sum(-1)

    P0, P1, Q0, Q1 = p0[:, None, :], p1[:, None, :], q0[None], q1[None]
    best = np.minimum(np.minimum(pt_seg(P0, Q0, Q1), pt_seg(P1, Q0, Q1)), np.minimum(pt_seg(Q0, P0, P1), pt_seg(Q1, P0, P1)))
    u, v, w = P1 - P0, Q1 - Q0, P0 - Q0
    a, b, c, d, e = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1), (u * w).sum(-1), (v * w).sum(-1)
    den = a * c - b * b
    ok = den > 0
    s = np.where(ok, (b * e - c * d) / np.where(ok, den, 1), -1)
    t = np.where(ok, (a * e - b * d) / np.where(ok, den, 1), -1)
    inside = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    dd = w + s[..., None] * u - t[..., None] * v
    return np.where(inside, np.minimum(best, (dd * dd).sum(-1)), best)


def link_dist(x, y, X):
    """the distance of the segments [x_k, y_k] (each [n][3], np.longdouble) from the primitives X ([m][3] or [m][3][3]) -> [n][m]"""
    X = np.asarray(X, dtype=LD)
    if X.ndim == 2:
        e = y - x
        den = (e * e).sum(-1)[:, None]
        t = np.clip(np.where(den > 0, ((X[None] - x[:, None]) * e[:, None]).sum(-1) / np.where(den > 0, den, 1), 0), 0, 1)
        d = X[None] - (x[:, None] + t[..., None] * e[:, None])
        return np.sqrt((d * d).sum(-1))
    a, b, c = X[:, 0], X[:, 1], X[:, 2]
    best = np.minimum(O._point_tri(x, a, b, c), O._point_tri(y, a, b, c)) ** 2
    for q0, q1 in ((a, b), (b, c), (c, a)):
        best = np.minimum(best, _seg_seg(x, y, q0, q1))
    # a link that pierces the triangle's interior: the ends on opposite sides of its plane and the crossing inside the three edges
    nrm = np.cross(b - a, c - a)[None]
    sx, sy = ((x[:, None] - a[None]) * nrm).sum(-1), ((y[:, None] - a[None]) * nrm).sum(-1)
    cross = (sx * sy < 0)
    tt = sx / np.where(cross, sx - sy, 1)
    hit = x[:, None] + tt[..., None] * (y - x)[:, None]
    inside = cross & ((np.cross(b - a, hit - a[None]) * nrm).sum(-1) >= 0) & ((np.cross(c - b, hit - b[None]) * nrm).sum(-1) >= 0) & ((np.cross(a - c, hit - c[None]) * nrm).sum(-1) >= 0)
    return np.sqrt(np.where(inside, 0, best))


def nearest_at(pkg, st, P, res, X, stations, a, b, times):
    """the distance of the flown link (a, b) from the nearest primitive at real times `times` [n], np.longdouble"""
    tt = np.asarray(times, dtype=LD)
    if len(tt) == 0:
        return np.zeros(0, dtype=LD)
    x = T.curve_at(pkg, st["spline"][a], st["piece_time"][a], P, res, tt)
    y = T.curve_at(pkg, st["spline"][b], st["piece_time"][b], P, res, tt) if b >= 0 else np.repeat(np.asarray(stations, dtype=LD).reshape(-1, 3)[-1 - b][None], len(tt), axis=0)
    return np.concatenate([link_dist(x[c:c + 64], y[c:c + 64], X).min(axis=1) for c in range(0, len(tt), 64)])


def truth(pkg, st, P, res, X, stations, links, dist, n=4001):
    """per link: (t [n], d [n], crossings): the nearest-primitive distance of the flown link on a dense grid of a's flight [0, P * piece_time_a] in
    np.longdouble, and the times at which it crosses the level `dist` between two grid samples, each refined by bisection (ascending)"""
    X = np.asarray(X, dtype=np.float64)
    out = []
    for (a, b) in links:
        t = np.linspace(LD(0), LD(P) * LD(st["piece_time"][a]), n, dtype=LD)

        def nearest(tt):
            return nearest_at(pkg, st, P, res, X, stations, a, b, tt)

        d = nearest(t)
        cross = []
        for k in np.flatnonzero((d[:-1] <= dist) != (d[1:] <= dist)):
            lo, hi, ina = t[k], t[k + 1], d[k] <= dist
            for _ in range(60):
                m = (lo + hi) / 2
                if (nearest(np.array([m], dtype=LD))[0] <= dist) == ina:
                    lo = m
                else:
                    hi = m
            cross.append(float((lo + hi) / 2))
        out.append((t, d, cross))
    return out


# ---- constructed states ----------------------------------------------------------------------------------------------------------------------------

def _pair_state(pkg, scenes, lines, points):
    """two robots on straight lines (audit_timed_ref.straight_state, 5 pieces) over a cloud moved 50 up, out of every range, with `points` as its first points"""
    scene, st = T.straight_state(pkg, scenes, lines, P=5)
    cloud = np.ascontiguousarray(np.array(scene["cloud"]) + np.array([0.0, 0.0, 50.0]))
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cloud[:len(pts)] = pts
    return dict(scene, cloud=cloud), st


PILLAR = [((-5, 1, 0), (5, 1, 0), 1.0), ((-5, -1, 0), (5, -1, 0), 1.0)]   # both ends x = -5 + 2 t: the link is the segment y in [-1, 1] at x(t)
STATES = ("pillar", "graze_out", "graze_in", "station", "hover", "staggered", "cluster")
_BUILT = {}


def built(pkg, scenes, pr, name, offset=0.1, vel_limit=2.0):
    """(scene, state, stations, links, dist, Ref, rows at the defaults, leaves) of a constructed state, once per process (the tests share it and never write
    to it)"""
    if name not in _BUILT:
        dist, stations, links = offset, np.zeros((0, 3)), [(0, 1)]
        if name == "pillar":                      # the point (1.3, 0, 0) on the link's sweep: the distance is |x(t) - 1.3| = 2 |t - 3.15|, within 0.1 over [3.10, 3.20]
            scene, st = _pair_state(pkg, scenes, PILLAR, [(1.3, 0.0, 0.0)])
        elif name in ("graze_out", "graze_in"):   # the sweep is the strip z = 0, |y| <= 1: a point above it is its z away
            scene, st = _pair_state(pkg, scenes, PILLAR, [(1.3, 0.0, dist + (1e-9 if name == "graze_out" else -1e-9))])
        elif name == "station":                   # one UAV along x, the station 10 up in y: at t = 2.5 the link is x = 0, y in [0, 10], and the point sits at lambda = 0.37 of it
            scene, st = O._line_state(pkg, scenes, (-5, 0, 0), (5, 0, 0), 1.0)
            scene["cloud"][77] = (0.0, 3.7, 0.0)
            stations, links = np.array([[0.0, 10.0, 0.0]]), [(0, -1)]
        elif name == "hover":                     # b arrives at (1.3, -1, 0) at t = 5 * 0.63 = 3.15 and hovers while a passes over the point
            scene, st = _pair_state(pkg, scenes, [PILLAR[0], ((1.3, -4.15, 0), (1.3, -1, 0), 0.63)], [(1.3, 0.0, 0.0)])
        elif name == "staggered":                 # piece_time[u] *= 1 + 0.03 u: b lags, the link slants, and b's segment cuts fall between a's
            scene, st = _pair_state(pkg, scenes, PILLAR, [(1.3, 0.0, 0.0)])
            st["piece_time"] = st["piece_time"] * (1 + 0.03 * np.arange(2))
        elif name == "cluster":                   # 150 points within 0.05 of the pillar's point: more than two flushes of the walk's candidate buffer
            rng = np.random.default_rng(21)
            v = rng.normal(size=(150, 3))
            v = v / np.linalg.norm(v, axis=1)[:, None] * (0.05 * rng.uniform(0.0, 1.0, size=(150, 1)) ** (1.0 / 3.0))
            scene, st = _pair_state(pkg, scenes, PILLAR, np.array([1.3, 0.0, 0.0]) + v)
        else:
            raise KeyError(name)
        ref = ref_of(pkg, pr, st, scene["P"], 8, O.prims_of(scene), stations)
        leaves = {}
        rows = ref.rows(links, dist, default_tol(dist, offset, vel_limit), leaves=leaves)
        _BUILT[name] = (scene, st, stations, links, dist, ref, rows, leaves)
    return _BUILT[name]


def many_leaves_state(pkg, scenes):
    """the pillar's flight with tol = 0 and max_depth = 40, segment 25 of a (x in [1.25, 1.5]): points at x = 1.3 and 1.325 on the sweep with dist = 0.05 - 1e-11 are
    within dist over x in [1.25 + 1e-11, 1.375 - 1e-11], so nearly every halving leaves an IN child behind; a third point at x = 1.45 adds a second chain"""
    return _pair_state(pkg, scenes, PILLAR, [(1.3, 0.0, 0.0), (1.325, 0.0, 0.0), (1.45, 0.0, 0.0)]) + (0.05 - 1e-11,)


# ---- the defaults, measured -----------------------------------------------------------------------------------------------------------------------

E2E = tuple(e for e in O.E2E if e[0] != "e2e_scn_a")
MODES = {"e2e_scn_b": 1, "e2e_scn_c3": 1, "e2e_scn_b_coupled": 2}


def measure_links(U):
    """(u, (u + 1) % U) and (u, U - 1 - u) for every u (a link of a robot with itself is left out), and every robot to the station"""
    out = []
    for u in range(U):
        for q in ((u + 1) % U, U - 1 - u):
            if q != u and (u, q) not in out:
                out.append((u, q))
    return out + [(u, -1) for u in range(U)]


def measure_states(pkg, offset=0.1, margin=0.1):
    """(label, state, P, res, cropped cloud, station) of the final and iteration-0 states of the three multi-UAV end-to-end fixtures; the station is the
    cropped cloud's centroid raised 1.0 above its top"""
    big = offset + 2 * margin
    scene_of = dict(O.E2E)
    for name, _ in E2E:
        scene = getattr(pkg.scenes, scene_of[name])()
        final, P, res = T.e2e_state(name)
        init = R.port_state(dict(scene, mode=MODES[name]), 0)
        X = O.prims_of(scene)
        for label, st in ((name, final), (name + "_init", dict(spline=np.array(init["spline"]), piece_time=np.array(init["piece_time"])))):
            lo, hi = st["spline"].min(axis=(0, 2)) - 2 * big - 1.0, st["spline"].max(axis=(0, 2)) + 2 * big + 1.0
            sub = X[np.flatnonzero(((X >= lo) & (X <= hi)).all(axis=1))]
            station = sub.mean(axis=0)
            station[2] = sub[:, 2].max() + 1.0
            yield label, st, P, res, sub, station


def as_triangles(cloud, h=0.02):
    """tiny triangles around the cloud's points, in the caller's order (scenes.triangulate's shape: a point and two neighbours h away)"""
    c = np.asarray(cloud, dtype=np.float64)
    return np.ascontiguousarray(np.stack([c, c + np.array([h, 0.0, 0.0]), c + np.array([0.0, h, 0.0])], axis=1))


def measure(ref, dist, projections, offset=0.1, vel_limit=2.0):
    """(rows, UNCERTAIN rows, TRUNCATED rows, largest live set, largest leaf list of any segment, largest depth, widest bracket) of one state's Ref (built
    with frontier=MAX_WINDOWS) at the default tol, max_depth = 40 and the lists capped at MAX_WINDOWS only"""
    ref.K = projections
    traces = {}
    rows = ref.rows(measure_links(ref.U), dist, default_tol(dist, offset, vel_limit), MAX_DEPTH, MAX_WINDOWS, traces=traces)
    live = max([t[1] for tr in traces.values() for t in tr] + [0])
    kept = max([t[2] for tr in traces.values() for t in tr] + [0])
    sure = rows["flags"] & CERTAIN != 0
    width = max([0.0] + list(rows["t_first_hi"][sure] - rows["t_first_lo"][sure]) + list(rows["t_last_hi"][sure] - rows["t_last_lo"][sure]))
    return (len(rows["link"]), int(np.sum(rows["flags"] & UNCERTAIN != 0)), int(np.sum(rows["flags"] & TRUNCATED != 0)), live, kept,
            int(rows["depth"].max()) if len(rows["depth"]) else 0, float(width))


def frontier_of(widest):
    return max(64, 1 << max(0, math.ceil(math.log2(4 * max(widest, 1)))))


def default_tolerance(pkg, pr, projections=None, ks=(), offset=0.1, margin=0.1, vel_limit=2.0):
    """(frontier, per (state, dist): measure(...) on the clouds at `projections` (None: the package's), per (K, state, dist): (rows, uncertain, largest leaf
    list) on the same clouds triangulated for every K of ks).  The frontier is the next power of two >= 4 x the larger of the two list maxima over both
    tables' states, at least 64."""
    K0 = pkg.SIGHT_PROJECTIONS if projections is None else projections
    per, tri, widest = {}, {}, 0
    for label, st, P, res, X, station in measure_states(pkg, offset, margin):
        cloud = ref_of(pkg, pr, st, P, res, X, station[None, :], projections=K0, frontier=MAX_WINDOWS)
        mesh = ref_of(pkg, pr, st, P, res, as_triangles(X), station[None, :], projections=K0, frontier=MAX_WINDOWS) if ks else None
        for dist in (offset, offset + 2 * margin):
            per[(label, dist)] = v = measure(cloud, dist, K0, offset, vel_limit)
            widest = max(widest, v[3], v[4])
            for K in ks:
                w = measure(mesh, dist, K, offset, vel_limit)
                tri[(K, label, dist)] = (w[0], w[1], w[4])
                if K == K0:
                    widest = max(widest, w[3], w[4])
    return frontier_of(widest), per, tri
