"""Reference values for tj_obstacle_approach that share no code with csrc/kernels_obstacle_approach.h (plain module: no fixtures, no tests).

  Ref.records         the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_obstacle_approach.py.  Hulls by
                      audit_ref.hulls_of (hull_entry's sums); the net of a window by audit_timed_ref.bez_restrict from the RAW hull (elementwise blossoming:
                      the same IEEE operations); lo through the ORACLE's GJK (audit_ref.FastGjk, hull = body 1, primitive = body 2) with the certificate
                      v . (b_i - p_j) > 0 for all six hull points and all primitive vertices, 0 without it; hi = the smaller of b_0's and b_5's distance to the
                      primitive (a point: norm3(b - p); a triangle: the oracle's GJK of {b} against it); brute force over ALL primitives with the box
                      prefilter of the walk's leaf predicate; the search level by level:
                        seeds     every (segment tr, primitive i) that passes the prefilter at `range`, window [0, 1]; best = the smallest hi < range in the
                                  order (hi, segment, index, s); live = {lo < range and lo < best.hi}
                        round d   every live item is halved at sm = 0.5 * (sa + sb); both children are evaluated from the raw hull; best over (best,
                                  children); live = children with lo < best.hi -- against the round's FINAL best
                        bracket   lo_u = min(best.hi, min lo over live), hi_u = best.hi
                        stop      hi - lo <= tol | live empty | d == max_depth | more than max_windows live (TRUNCATED: the record of the last
                                  completed round; `windows` still counts the round that overflowed)
  truth               nothing of GJK or subdivision in it: the flown curve from `convert` in np.longdouble on a dense grid against every point (or the exact
                      point-triangle distance), the best few primitives refined locally in time.
  constructed states  corner, pierce, miss (single-UAV): each builder asserts its precondition on the CPU.
  default_tolerance   the measured TJ_OBSTACLE_TOL and the largest live set (TJ_OBSTACLE_FRONTIER), the manner of closest_ref.default_tolerance.
The slack is audit_timed_ref's (counted there); here one curve and a fixed primitive, so it is an over-count."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T

LD = np.longdouble
CONTACT, CLEAR, CONVERGED, TRUNCATED = 1, 2, 4, 8
MAX_DEPTH = 40
FIELDS = ("lo", "hi", "time", "index", "segment", "depth", "flags", "windows")


def prims_of(scene):
    """the obstacle primitives in the caller's order: [N][3] points or [N][3][3] triangles"""
    return np.ascontiguousarray(scene["tris"] if scene.get("tris") is not None else scene["cloud"], dtype=np.float64)


def _norm3(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


class Ref:
    """the restatement on one state and one obstacle set; seed evaluations are kept per (robot, range, prefilter): they do not depend on tol / depth / cap"""

    def __init__(self, pkg, pr, st, P, res, X):
        self.pt, self.S, self.rf = np.asarray(st["piece_time"], dtype=np.float64), P * res, float(res)
        self.H = np.ascontiguousarray(R.hulls_of(pkg, np.asarray(st["spline"], dtype=np.float64), P, res))
        self.U = self.H.shape[0]
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.N = self.X.shape[0]
        self.tri = self.X.ndim == 3
        self.nv = 3 if self.tri else 1
        self.Xv = self.X.reshape(self.N, self.nv, 3)
        self.plo, self.phi = self.Xv.min(axis=1), self.Xv.max(axis=1)
        self.g = R.FastGjk(pr)
        self._seeds = {}

    # ---- one batch of items (tr[n], i[n], sa[n], sb[n]) of robot u -> lo[n], hi[n], s[n] (the parameter of the hi sample) ----
    def evaluate(self, u, tr, i, sa, sb):
        n = len(tr)
        if n == 0:
            return np.zeros(0), np.zeros(0), np.zeros(0)
        net = np.ascontiguousarray(T.bez_restrict(self.H[u, tr], sa, sb))           # [n][6][3], always from the raw hull
        Xi = np.ascontiguousarray(self.Xv[i])                                        # [n][nv][3]
        f, nv = self.g.f, self.nv
        V = np.zeros((n, 3))
        nb, xb, vb = net.ctypes.data, Xi.ctypes.data, V.ctypes.data
        for k in range(n):
            f(6, nb + k * 144, nv, xb + k * nv * 24, vb + k * 24)
        lo = _norm3(V)
        m = np.full(n, np.inf)
        for a in range(6):
            for b in range(nv):
                d = net[:, a] - Xi[:, b]
                m = np.minimum(m, (V[:, 0] * d[:, 0] + V[:, 1] * d[:, 1]) + V[:, 2] * d[:, 2])
        lo = np.where(m > 0.0, lo, 0.0)                                                # no separating plane: the primitive may touch the hull
        if self.tri:
            e = np.ascontiguousarray(net[:, (0, 5)])                                  # [n][2][3]
            W = np.zeros((n, 2, 3))
            eb, wb = e.ctypes.data, W.ctypes.data
            for k in range(n):
                f(1, eb + k * 48, 3, xb + k * 72, wb + k * 48)
                f(1, eb + k * 48 + 24, 3, xb + k * 72, wb + k * 48 + 24)
            h0, h5 = _norm3(W[:, 0]), _norm3(W[:, 1])
        else:
            h0, h5 = _norm3(net[:, 0] - Xi[:, 0]), _norm3(net[:, 5] - Xi[:, 0])
        first = h0 <= h5
        return lo, np.where(first, h0, h5), np.where(first, sa, sb)

    def seeds(self, u, rng, prefilter=True):
        key = (u, rng, prefilter)
        if key not in self._seeds:
            trs, ids = [], []
            for tr in range(self.S):
                lo, hi = self.H[u, tr].min(axis=0), self.H[u, tr].max(axis=0)
                near = np.flatnonzero(~((self.phi + rng < lo) | (self.plo > hi + rng)).any(axis=1)) if prefilter else np.arange(self.N)
                trs.append(np.full(len(near), tr, dtype=np.int64)); ids.append(near)
            tr, i = (np.concatenate(trs), np.concatenate(ids)) if trs else (np.zeros(0, dtype=np.int64),) * 2
            self._seeds[key] = (tr, i) + self.evaluate(u, tr, i, np.zeros(len(tr)), np.ones(len(tr)))
        return self._seeds[key]

    def time_of(self, u, tr, s):
        return ((tr + s) / self.rf) * float(self.pt[u])

    def search(self, u, rng, tol, max_depth, max_windows, prefilter=True, trace=None):
        """the record of robot u as a dict; trace (a list) receives (depth, lo, hi, live) of every completed round"""
        tr, i, lo, hi, s = self.seeds(u, rng, prefilter)
        windows = len(tr)
        best = (rng, math.inf, math.inf, math.inf)                                    # (hi, segment, index, s): the total order of `best`

        def better(best, tr, i, hi, s):
            ok = np.flatnonzero(hi < rng)
            if len(ok):
                k = ok[np.lexsort((s[ok], i[ok], tr[ok], hi[ok]))[0]]
                best = min(best, (float(hi[k]), int(tr[k]), int(i[k]), float(s[k])))
            return best

        best = better(best, tr, i, hi, s)
        keep = (lo < rng) & (lo < best[0])
        live = (tr[keep], i[keep], np.zeros(int(keep.sum())), np.ones(int(keep.sum())), lo[keep])
        rec = dict(best=best, lo=min([best[0]] + live[4].tolist()), depth=0)
        truncated = len(live[0]) > max_windows
        if trace is not None:
            trace.append((0, rec["lo"], best[0], len(live[0])))
        d = 0
        while not truncated:
            if rec["best"][0] - rec["lo"] <= tol or len(live[0]) == 0 or d == max_depth:
                break
            ltr, li, sa, sb, _ = live
            sm = 0.5 * (sa + sb)
            ktr, ki = np.concatenate([ltr, ltr]), np.concatenate([li, li])
            ksa, ksb = np.concatenate([sa, sm]), np.concatenate([sm, sb])
            klo, khi, ks = self.evaluate(u, ktr, ki, ksa, ksb)
            windows += len(ktr)
            best = better(rec["best"], ktr, ki, khi, ks)
            keep = klo < best[0]
            if int(keep.sum()) > max_windows:
                truncated = True
                break
            d += 1
            live = (ktr[keep], ki[keep], ksa[keep], ksb[keep], klo[keep])
            rec = dict(best=best, lo=min([best[0]] + live[4].tolist()), depth=d)
            if trace is not None:
                trace.append((d, rec["lo"], best[0], len(live[0])))
        hi_u, seg, idx, s_u = rec["best"]
        found = idx != math.inf
        return dict(lo=rec["lo"], hi=hi_u, time=self.time_of(u, seg, s_u) if found else -1.0, index=idx if found else -1, segment=seg if found else -1,
                    depth=rec["depth"], windows=windows, live_empty=len(live[0]) == 0 and not truncated, truncated=truncated)

    def flags_of(self, r, offset, tol):
        return ((CONTACT if r["index"] >= 0 and r["hi"] <= offset else 0) | (CLEAR if r["lo"] > offset or self.N == 0 else 0) |
                (CONVERGED if r["hi"] - r["lo"] <= tol or r["live_empty"] else 0) | (TRUNCATED if r["truncated"] else 0))

    def records(self, rng, offset, tol, max_depth, max_windows, owned=None, prefilter=True, traces=None):
        """per robot the record's fields, in tj_obstacle_robot's names (robots outside `owned`: zero).  rng, tol, max_depth, max_windows: the resolved values."""
        out = {n: np.zeros(self.U, dtype=np.float64 if n in FIELDS[:3] else np.int32) for n in FIELDS}
        for u in (range(self.U) if owned is None else owned):
            tr = [] if traces is not None else None
            r = self.search(u, float(rng), float(tol), max_depth, max_windows, prefilter, tr)
            r["flags"] = self.flags_of(r, offset, tol)
            for n in FIELDS:
                out[n][u] = r[n]
            if traces is not None:
                traces[u] = tr
        return out


def sentinel(rng):
    return dict(lo=rng, hi=rng, time=-1.0, index=-1, segment=-1, depth=0, flags=CLEAR | CONVERGED, windows=0)


# ---- the truth: the flown curve itself against every primitive ----------------------------------------------------------------------------------

def _point_tri(p, a, b, c):
    """exact distance of points p [n][3] from triangles (a, b, c) [m][3] each -> [n][m], np.longdouble: the closest point by its Voronoi region
    (vertex, edge, face), written out; a degenerate triangle falls to its edges / vertices"""
    p = p[:, None, :]; a, b, c = a[None], b[None], c[None]

    def seg(p, a, b):
        ab = b - a
        den = (ab * ab).sum(-1)
        t = np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1), 0)
        t = np.clip(t, 0, 1)
        d = p - (a + t[..., None] * ab)
        return (d * d).sum(-1)

    best = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(-1)
    ok = nn > 0
    nd = ((p - a) * nrm).sum(-1)
    proj = p - (nd / np.where(ok, nn, 1))[..., None] * nrm                                  # the foot on the triangle's plane
    inside = ok & ((np.cross(b - a, proj - a) * nrm).sum(-1) >= 0) & ((np.cross(c - b, proj - b) * nrm).sum(-1) >= 0) & ((np.cross(a - c, proj - c) * nrm).sum(-1) >= 0)
    face = nd * nd / np.where(ok, nn, 1)
    return np.sqrt(np.where(inside, np.minimum(best, face), best))


def _dist(p, X):
    """curve points p [n][3] against primitives X ([m][3] or [m][3][3]) in np.longdouble -> [n][m]"""
    X = np.asarray(X, dtype=LD)
    if X.ndim == 3:
        return _point_tri(p, X[:, 0], X[:, 1], X[:, 2])
    d = p[:, None, :] - X[None]
    return np.sqrt((d * d).sum(-1))


def truth(pkg, st, P, res, X, n=2001, keep=12, rounds=4):
    """per robot u: (distance, primitive, time): the minimum over a dense time grid of [0, P * piece_time_u] and ALL primitives of dist(p_u(t), primitive),
    then the `keep` best primitives refined in time around their own best sample (`rounds` times a 41-point grid over the two neighbouring steps).
    An upper bound of the true minimum that converges to it from above."""
    X = np.asarray(X, dtype=np.float64)
    out = []
    for u in range(st["spline"].shape[0]):
        if X.shape[0] == 0:
            out.append((np.inf, -1, -1.0)); continue
        dur = LD(P) * LD(st["piece_time"][u])
        t = np.linspace(LD(0), dur, n, dtype=LD)
        pu = T.curve_at(pkg, st["spline"][u], st["piece_time"][u], P, res, t)
        dmin, kmin = np.full(X.shape[0], np.inf, dtype=LD), np.zeros(X.shape[0], dtype=np.int64)
        for c0 in range(0, n, 64):
            d = _dist(pu[c0:c0 + 64], X)
            k = d.argmin(axis=0)
            v = d[k, np.arange(X.shape[0])]
            upd = v < dmin
            dmin[upd], kmin[upd] = v[upd], k[upd] + c0
        best = (np.inf, -1, -1.0)
        for i in np.argsort(dmin)[:keep]:
            tc, h = t[kmin[i]], dur / (n - 1)
            val = dmin[i]
            for _ in range(rounds):
                tt = np.clip(np.linspace(tc - h, tc + h, 41, dtype=LD), 0, dur)
                d = _dist(T.curve_at(pkg, st["spline"][u], st["piece_time"][u], P, res, tt), X[i:i + 1])[:, 0]
                k = int(d.argmin())
                if d[k] <= val:
                    val, tc = d[k], tt[k]
                h = h / 20
            if float(val) < best[0]:
                best = (float(val), int(i), float(tc))
        out.append(best)
    return out


def slack(S, st, X):
    return T.slack(S, np.concatenate([np.abs(np.asarray(st["spline"])).ravel(), np.abs(np.asarray(X)).ravel(), [1.0]]))


# ---- constructed single-UAV states -----------------------------------------------------------------------------------------------------------------

def _line_state(pkg, scenes, a, b, pt):
    """the single-UAV scene tiny(mode=0) with its cloud moved 50 up (out of every range) and the straight flight a -> b at constant speed"""
    scene = dict(scenes.tiny(mode=0))
    scene["cloud"] = np.ascontiguousarray(scene["cloud"] + np.array([0.0, 0.0, 50.0]))
    st = R.port_state(scene, 0)
    P = scene["P"]
    g1, gs = T.linear_nets(pkg, P, 8)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    st["spline"][0] = a[:, None] * g1[None, :] + ((b - a) / P)[:, None] * gs[None, :]
    st["piece_time"][0] = pt
    assert R.valid_state(st, 1)
    return scene, st


def pierce_state(pkg, scenes):
    """the straight flight x = -5 -> 5 in 5 * 1.0 through cloud point 77 at x = 1.3: the crossing is at t = 3.15 (sigma = 3.15: 0.2 into segment 25, no
    dyadic parameter), and the distance is |x(t) - 1.3| = 2 |t - 3.15|, linear in time.  Returns (scene, state, 77, 3.15)."""
    scene, st = _line_state(pkg, scenes, (-5, 0, 0), (5, 0, 0), 1.0)
    scene["cloud"][77] = (1.3, 0.0, 0.0)
    p = T.curve_at(pkg, st["spline"][0], 1.0, scene["P"], 8, np.array([3.15], dtype=LD))[0]
    assert float(np.abs(p - np.array([1.3, 0, 0], dtype=LD)).max()) < 1e-12
    return scene, st, 77, 3.15


def miss_state(pkg, scenes, d=0.25):
    """the same flight with cloud point 77 at (1.3, d, 0): perpendicular distance d > offset, at t = 3.15.  Returns (scene, state, 77, d)."""
    scene, st = _line_state(pkg, scenes, (-5, 0, 0), (5, 0, 0), 1.0)
    scene["cloud"][77] = (1.3, d, 0.0)
    return scene, st, 77, d


def corner_state(pkg, scenes, pr, offset=0.1):
    """one sharp corner: the straight flight x = -100 -> 100 with two neighbouring control points pulled 40 up and 40 down in y.  The hulls of the
    segments at the turn bulge towards those control points, the flown curve cuts inside.  Cloud point 77 goes 0.9 of the way from the centroid of the
    hull whose vertex is furthest from the curve to that vertex: inside the hull (a convex combination of its vertices), 0.2 from the curve.  Asserted
    here: the restated tj_audit reports contact (obs_clearance <= offset against primitive 77, on the GJK's contact floor), the truth is above
    offset + 0.05.  Returns (scene, state, 77, truth of robot 0)."""
    scene, st = _line_state(pkg, scenes, (-100, 0, 0), (100, 0, 0), 1.0)
    P = scene["P"]
    st["spline"][0][1, 8] += 40.0
    st["spline"][0][1, 9] -= 40.0
    H = R.hulls_of(pkg, st["spline"], P, 8)
    t = np.linspace(LD(0), LD(P), 8001, dtype=LD)
    pu = np.asarray(T.curve_at(pkg, st["spline"][0], 1.0, P, 8, t), dtype=np.float64)
    far = np.array([[np.sqrt(((pu - H[0, tr, j]) ** 2).sum(axis=1)).min() for j in range(6)] for tr in range(P * 8)])
    tr, j = np.unravel_index(int(np.argmax(far)), far.shape)
    scene["cloud"][77] = 0.1 * H[0, tr].mean(axis=0) + 0.9 * H[0, tr, j]
    d, ids = R.brute_obs(pr, H, scene["cloud"], 0.3)
    v, seg, k = R.robot_min(d, ids, 0.3)[0]
    assert k == 77 and v <= 1e-4 and v <= offset, (v, seg, k)
    tv = truth(pkg, st, P, 8, scene["cloud"], n=4001)[0]
    assert tv[1] == 77 and tv[0] > offset + 0.05, tv
    assert R.valid_state(st, 1)
    return scene, st, 77, tv


# ---- the defaults, measured ------------------------------------------------------------------------------------------------------------------------

def floor_of(widths):
    """the last depth after which the width stops shrinking by 2x -- the last depth that still brought a halving -- or, where the widths reach 0
    (every live set has emptied: hi == lo), the last depth with a positive width"""
    pos = [d for d, w in enumerate(widths) if w > 0.0]
    if pos and pos[-1] + 1 < len(widths):
        return pos[-1]
    return max([d for d in range(1, len(widths)) if widths[d] <= widths[d - 1] / 2] or [0])


E2E = (("e2e_scn_a", "scn_a"), ("e2e_scn_b", "scn_b"), ("e2e_scn_c3", "scn_c3"), ("e2e_scn_b_coupled", "scn_b"))


def default_tolerance(pkg, pr, names=E2E, rng=0.1 + 2 * 0.1, offset=0.1):
    """(widths per depth 0..40, floor depth, tolerance, largest live set): tol = 0 and max_depth = 40 at the default range on the named end states with
    their scenes' obstacle sets; per depth the largest hi - lo over the robots with a primitive in range (a robot whose search has ended keeps its
    last bracket).  The floor: floor_of.  The tolerance is the smallest power of ten >= 10 x the width at the floor."""
    widths, biggest = [0.0] * (MAX_DEPTH + 1), 0
    for name, scn in names:
        st, P, res = T.e2e_state(name)
        X = prims_of(getattr(pkg.scenes, scn)())
        lo, hi = st["spline"].min(axis=(0, 2)) - 2 * rng - 1.0, st["spline"].max(axis=(0, 2)) + 2 * rng + 1.0
        sub = np.flatnonzero(((X >= lo) & (X <= hi)).all(axis=1))                 # (control nets bound their hulls up to the basis' overshoot: 1.0 is generous; asserted)
        ref = Ref(pkg, pr, st, P, res, X[sub])
        assert np.all(ref.H.min(axis=(0, 1, 2)) - rng > lo) and np.all(ref.H.max(axis=(0, 1, 2)) + rng < hi)
        traces = {}
        rec = ref.records(rng, offset, 0.0, MAX_DEPTH, 1 << 30, traces=traces)
        for u, tr in traces.items():
            biggest = max(biggest, max(t[3] for t in tr))
            if rec["index"][u] < 0:
                continue
            for d in range(MAX_DEPTH + 1):
                _, l, h, _ = tr[min(d, len(tr) - 1)]
                widths[d] = max(widths[d], h - l)
    floor = floor_of(widths)
    return widths, floor, float("1e%d" % math.ceil(math.log10(10 * widths[floor]))), biggest
