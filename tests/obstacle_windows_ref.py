"""Reference values for tj_obstacle_windows that share no code with csrc/kernels_obstacle_windows.h (plain module: no fixtures, no tests).

  Ref.rows            the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_obstacle_windows.py.  It builds on
                      obstacle_approach_ref.Ref's pieces -- hulls by audit_ref.hulls_of, the net of a window by audit_timed_ref.bez_restrict from the RAW hull,
                      the ORACLE's GJK (hull = body 1, primitive = body 2) with the certificate v . (b_i - p_j) > 0 -- and adds:
                        candidates  the walk's leaf predicate by brute force over ALL primitives: the primitive's box within dist of the net's box on every
                                    axis, touching counts
                        per p       lo_p (certified |v|, else 0), ub_p = the largest distance of b_0..b_5 from p, h0_p / h5_p = b_0's / b_5's (a point:
                                    norm3(b - p); a triangle: the oracle's GJK of {b} against it)
                        class       OUT: every candidate has lo_p > dist (an empty set too) | IN: some ub_p <= dist | MIXED: the rest (in this order)
                        h0, h5      the smallest h0_p (h5_p) with its primitive in the order (value, index)
                        search      per (robot, segment): seed [0, 1]; a round takes the live windows in ascending sa: time width
                                    ((sb - sa) / res) * piece_time <= tol -> EDGE leaf, else halved, children left then right: OUT dropped, IN to the leaves,
                                    MIXED to the next live set.  Stop: live empty | depth == max_depth | live or leaves above max_windows (TRUNCATED: the lists
                                    of the last completed round; `windows` counts the overflowing round too).  The live windows end as EDGE leaves.
                        merge       per robot the leaves in (segment, sa) order; adjacent iff prev.tr + prev.sb == next.tr + next.sa; a row per maximal chain
  truth               nothing of GJK or subdivision in it: the flown curve from `convert` in np.longdouble on a dense time grid against every primitive (a
                      point directly, a triangle by obstacle_approach_ref._point_tri): the nearest-primitive distance per sample and the crossings of the level
                      `dist`, refined by bisection.
  constructed states  obstacle_approach_ref's corner, pierce and miss, a two-point state and a dense cluster: `built` asserts on the CPU that none yields an
                      UNCERTAIN or TRUNCATED row at the defaults.
  default_tolerance   the measured table of the header and TJ_OBSWIN_FRONTIER.
The slack is obstacle_approach_ref.slack (counted there)."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import obstacle_approach_ref as O

LD = np.longdouble
CERTAIN, UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED = 1, 2, 4, 8, 16, 32
MAX_DEPTH, MAX_WINDOWS, TOL_FRACTION = 40, 1024, 0.01
DOUBLES = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "closest", "closest_time")
FIELDS = DOUBLES + ("robot", "index", "segment_first", "segment_last", "leaves", "depth", "flags", "windows")
OUT, IN, MIXED = 0, 1, 2
INF = math.inf


def default_tol(dist, offset, vel_limit):
    """what tol < 0 selects: the time a robot at the speed limit needs for 1 % of dist (of offset where dist is infinite)"""
    return (TOL_FRACTION * (offset if dist == INF else dist)) / vel_limit


def _norms(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


class Ref(O.Ref):
    """the restatement on one state and one obstacle set; evaluations are kept per (robot, segment, window, dist): they do not depend on tol / depth / cap"""

    def __init__(self, pkg, pr, st, P, res, X):
        super().__init__(pkg, pr, st, P, res, X)
        self.frontier = pkg.OBSWIN_FRONTIER                                                  # what max_windows=None selects
        self._evals = {}

    def window(self, u, tr, sa, sb, dist):
        """(class, h0, i0, h5, i5) of the window [sa, sb] of segment tr of robot u against the union of all primitives"""
        key = (u, tr, sa, sb, dist)
        if key not in self._evals:
            self._evals[key] = self._window(u, tr, sa, sb, dist)
        return self._evals[key]

    def _window(self, u, tr, sa, sb, dist):
        net1 = T.bez_restrict(self.H[u, tr][None], [sa], [sb])[0]                              # [6][3], always from the raw hull
        lo, hi = net1.min(axis=0), net1.max(axis=0)
        near = np.flatnonzero(~((self.phi + dist < lo) | (self.plo > hi + dist)).any(axis=1)) if self.N else np.zeros(0, dtype=np.int64)
        n = len(near)
        if n == 0:
            return OUT, INF, -1, INF, -1
        net = np.ascontiguousarray(np.broadcast_to(net1, (n, 6, 3)))
        Xi = np.ascontiguousarray(self.Xv[near])                                             # [n][nv][3]
        f, nv = self.g.f, self.nv
        V = np.zeros((n, 3))
        nb, xb, vb = net.ctypes.data, Xi.ctypes.data, V.ctypes.data
        for k in range(n):
            f(6, nb + k * 144, nv, xb + k * nv * 24, vb + k * 24)
        m = np.full(n, np.inf)
        for a in range(6):
            for b in range(nv):
                d = net[:, a] - Xi[:, b]
                m = np.minimum(m, (V[:, 0] * d[:, 0] + V[:, 1] * d[:, 1]) + V[:, 2] * d[:, 2])
        lo_p = np.where(m > 0.0, _norms(V), 0.0)
        if self.tri:
            W = np.zeros((n, 6, 3))
            wb = W.ctypes.data
            for k in range(n):
                for a in range(6):
                    f(1, nb + k * 144 + a * 24, 3, xb + k * 72, wb + k * 144 + a * 24)
            D = _norms(W)                                                                    # [n][6]
        else:
            D = _norms(net - Xi[:, 0][:, None, :])
        if bool(np.all(lo_p > dist)):
            return OUT, INF, -1, INF, -1
        ub = D.max(axis=1)
        k0 = np.lexsort((near, D[:, 0]))[0]
        k5 = np.lexsort((near, D[:, 5]))[0]
        return (IN if bool(np.any(ub <= dist)) else MIXED), float(D[k0, 0]), int(near[k0]), float(D[k5, 5]), int(near[k5])

    def width(self, u, sa, sb):
        return ((sb - sa) / self.rf) * float(self.pt[u])

    def search(self, u, tr, dist, tol, max_depth, max_windows, trace=None):
        """the leaves of segment tr of robot u: dict(leaves sorted by sa: (sa, sb, h0, i0, h5, i5, is IN), depth, windows, truncated).  trace receives
        (depth, size of the live set, size of the leaf list) after the seed and after every round, the overflowing one included"""
        c, h0, i0, h5, i5 = self.window(u, tr, 0.0, 1.0, dist)
        windows = 1
        leaves = [(0.0, 1.0, h0, i0, h5, i5, True)] if c == IN else []
        live = [(0.0, 1.0, h0, i0, h5, i5)] if c == MIXED else []
        if trace is not None:
            trace.append((0, len(live), len(leaves)))
        d, truncated = 0, False
        while live and d < max_depth:
            new, nxt = list(leaves), []
            for (sa, sb, h0, i0, h5, i5) in live:                                           # ascending sa: children are appended left then right
                if self.width(u, sa, sb) <= tol:
                    new.append((sa, sb, h0, i0, h5, i5, False))
                    continue
                sm = 0.5 * (sa + sb)
                assert sa < sm < sb
                for ka, kb in ((sa, sm), (sm, sb)):
                    c, g0, j0, g5, j5 = self.window(u, tr, ka, kb, dist)
                    windows += 1
                    if c == IN:
                        new.append((ka, kb, g0, j0, g5, j5, True))
                    elif c == MIXED:
                        nxt.append((ka, kb, g0, j0, g5, j5))
            if trace is not None:
                trace.append((d + 1, len(nxt), len(new)))
            if len(nxt) > max_windows or len(new) > max_windows:
                truncated = True
                break
            d += 1
            leaves, live = new, nxt
        leaves = leaves + [w + (False,) for w in live]
        return dict(leaves=sorted(leaves), depth=d, windows=windows, truncated=truncated)

    def robot_rows(self, u, dist, tol, max_depth, max_windows, traces=None, leaves_out=None):
        segs = []
        for tr in range(self.S):
            trace = [] if traces is not None else None
            segs.append(self.search(u, tr, dist, tol, max_depth, max_windows, trace))
            if traces is not None:
                traces[(u, tr)] = trace
        windows = sum(s["windows"] for s in segs)
        flat = [(tr,) + lf for tr in range(self.S) for lf in segs[tr]["leaves"]]           # (segment, sa) order
        chains = []
        for k, lf in enumerate(flat):
            if k:
                p = flat[k - 1]
                assert p[0] + p[2] <= lf[0] + lf[1] and (p[0], p[1]) < (lf[0], lf[1]), (p, lf)   # distinct, disjoint
            if k and flat[k - 1][0] + flat[k - 1][2] == lf[0] + lf[1]:
                chains[-1].append(lf)
            else:
                chains.append([lf])
        rows = []
        for chain in chains:
            sure, within, best = [], 0.0, (INF, INF, INF)
            for tr, sa, sb, h0, i0, h5, i5, is_in in chain:
                ta, tb = self.time_of(u, tr, sa), self.time_of(u, tr, sb)
                if is_in:
                    sure += [ta, tb]
                    within += self.width(u, sa, sb)
                else:
                    if h0 <= dist:
                        sure.append(ta)
                    if h5 <= dist:
                        sure.append(tb)
                best = min(best, (h0, ta, i0), (h5, tb, i5))
            first, last = chain[0], chain[-1]
            first_lo, last_hi = self.time_of(u, first[0], first[1]), self.time_of(u, last[0], last[2])
            first_hi, last_lo = (min(sure), max(sure)) if sure else (-1.0, -1.0)
            at_start, at_end = first[0] + first[1] == 0.0, last[0] + last[2] == float(self.S)
            trs = sorted({lf[0] for lf in chain})
            flags = ((CERTAIN if sure else UNCERTAIN) | (AT_START if at_start else 0) | (AT_END if at_end else 0) |
                     (TRUNCATED if any(segs[tr]["truncated"] for tr in trs) else 0))
            if sure and (at_start or first_hi - first_lo <= tol) and (at_end or last_hi - last_lo <= tol):
                flags |= RESOLVED
            rows.append(dict(t_first_lo=first_lo, t_first_hi=first_hi, t_last_lo=last_lo, t_last_hi=last_hi, within_lo=within, closest=best[0],
                             closest_time=best[1], robot=u, index=best[2], segment_first=first[0], segment_last=last[0], leaves=len(chain),
                             depth=max(segs[tr]["depth"] for tr in trs), flags=flags, windows=windows))
            if leaves_out is not None:
                leaves_out.setdefault(u, []).append([(self.time_of(u, tr, sa), self.time_of(u, tr, sb), is_in, h0, h5) for tr, sa, sb, h0, _, h5, _, is_in in chain])
        return rows

    def rows(self, dist, tol, max_depth=MAX_DEPTH, max_windows=None, owned=None, traces=None, leaves=None):
        """the rows as a dict of numpy arrays [n] in (robot, t_first_lo) order.  dist, tol, max_depth, max_windows: the resolved values.  traces: per (robot,
        segment) the search's trace; leaves: per robot, per row the chain as (time a, time b, is IN, h0, h5)."""
        max_windows = self.frontier if max_windows is None else max_windows
        out = []
        if self.N:
            for u in (range(self.U) if owned is None else owned):
                out += self.robot_rows(u, float(dist), float(tol), max_depth, max_windows, traces, leaves)
        return {n: np.array([r[n] for r in out], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}


def ref_of(pkg, pr, st, P, res, X):
    return Ref(pkg, pr, st, P, res, X)


# ---- the truth: the flown curve itself against every primitive ----------------------------------------------------------------------------------

def nearest_at(pkg, st, P, res, X, u, times):
    """the distance of robot u's flown curve from the nearest primitive at real times `times` [n], np.longdouble"""
    tt = np.asarray(times, dtype=LD)
    p = T.curve_at(pkg, st["spline"][u], st["piece_time"][u], P, res, tt)
    return np.concatenate([O._dist(p[c:c + 64], X).min(axis=1) for c in range(0, len(tt), 64)]) if len(tt) else np.zeros(0, dtype=LD)


def truth(pkg, st, P, res, X, dist, n=4001):
    """per robot u: (t [n], d [n], crossings): the nearest-primitive distance of the flown curve on a dense time grid of [0, P * piece_time_u] in np.longdouble,
    and the times at which it crosses the level `dist` between two grid samples, each refined by bisection (ascending)"""
    X = np.asarray(X, dtype=np.float64)
    out = []
    for u in range(st["spline"].shape[0]):
        dur = LD(P) * LD(st["piece_time"][u])
        t = np.linspace(LD(0), dur, n, dtype=LD)

        def nearest(tt):
            return nearest_at(pkg, st, P, res, X, u, tt)

        d = nearest(t)
        cross = []
        for k in np.flatnonzero((d[:-1] <= dist) != (d[1:] <= dist)):
            a, b, ina = t[k], t[k + 1], d[k] <= dist
            for _ in range(60):
                m = (a + b) / 2
                if (nearest(np.array([m], dtype=LD))[0] <= dist) == ina:
                    a = m
                else:
                    b = m
            cross.append(float((a + b) / 2))
        out.append((t, d, cross))
    return out


# ---- constructed single-UAV states ---------------------------------------------------------------------------------------------------------------

def two_point_state(pkg, scenes, gap):
    """pierce_state with cloud point 78 on the line too, `gap` along x behind point 77: at dist = 0.1 one merged row for gap < 0.2, two rows above"""
    scene, st, k, t_cross = O.pierce_state(pkg, scenes)
    scene["cloud"][78] = (1.3 + gap, 0.0, 0.0)
    return scene, st


def cluster_state(pkg, scenes, n=150, radius=0.05, seed=21):
    """pierce_state with cloud points 0..n-1 within `radius` of the point (1.3, 0, 0) of the line: more than two flushes of the walk's candidate buffer"""
    scene, st, k, t_cross = O.pierce_state(pkg, scenes)
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v = v / np.linalg.norm(v, axis=1)[:, None] * (radius * rng.uniform(0.0, 1.0, size=(n, 1)) ** (1.0 / 3.0))
    scene["cloud"][:n] = np.array([1.3, 0.0, 0.0]) + v
    assert np.all(np.linalg.norm(scene["cloud"][:n] - np.array([1.3, 0.0, 0.0]), axis=1) <= radius) and scene["cloud"].shape[0] > n
    return scene, st


STATES = ("corner", "pierce", "miss", "two_near", "two_far", "cluster")
_BUILT = {}


def built(pkg, scenes, pr, name, offset=0.1, vel_limit=2.0):
    """(scene, state, dist, Ref, rows at the defaults, leaves) of a constructed state, once per process (the tests share it and never write to it).  Asserted
    here: at the defaults the state yields no UNCERTAIN and no TRUNCATED row."""
    if name not in _BUILT:
        dist = offset
        if name == "corner":
            scene, st = O.corner_state(pkg, scenes, pr, offset)[:2]
            dist = 0.3                                                                       # (the curve stays about 0.2 from the point inside its hull)
        elif name == "pierce":
            scene, st = O.pierce_state(pkg, scenes)[:2]
        elif name == "miss":
            scene, st = O.miss_state(pkg, scenes)[:2]
            dist = 0.3
        elif name in ("two_near", "two_far"):
            scene, st = two_point_state(pkg, scenes, 0.15 if name == "two_near" else 0.5)
        else:
            scene, st = cluster_state(pkg, scenes)
        ref = ref_of(pkg, pr, st, scene["P"], 8, O.prims_of(scene))
        leaves = {}
        rows = ref.rows(dist, default_tol(dist, offset, vel_limit), leaves=leaves)
        assert not np.any(rows["flags"] & (UNCERTAIN | TRUNCATED)), (name, rows["flags"])
        _BUILT[name] = (scene, st, dist, ref, rows, leaves)
    return _BUILT[name]


# ---- the defaults, measured -----------------------------------------------------------------------------------------------------------------------

E2E = O.E2E
MODES = {"e2e_scn_a": 0, "e2e_scn_b": 1, "e2e_scn_c3": 1, "e2e_scn_b_coupled": 2}


def default_tolerance(pkg, pr, names=E2E, offset=0.1, margin=0.1, vel_limit=2.0):
    """(frontier, per (state, dist): (rows, UNCERTAIN rows, TRUNCATED rows, largest live set, largest leaf list of any segment, largest depth, widest
    bracket)): the default tol, max_depth = 40, the lists capped at MAX_WINDOWS only, on the named end states and the same runs' iteration-0 states (_init)
    with their scenes' clouds, cropped as obstacle_approach_ref.default_tolerance crops them.  The widest bracket is the largest of t_first_hi - t_first_lo and
    t_last_hi - t_last_lo over the CERTAIN rows.  The frontier is the next power of two >= 4 x the larger of the two list maxima, at least 64."""
    per, widest = {}, 0
    big = offset + 2 * margin
    for name, scn in names:
        scene = getattr(pkg.scenes, scn)()
        final, P, res = T.e2e_state(name)
        init = R.port_state(dict(scene, mode=MODES.get(name, scene.get("mode", 1))), 0)
        X = O.prims_of(scene)
        for label, st in ((name, final), (name + "_init", dict(spline=np.array(init["spline"]), piece_time=np.array(init["piece_time"])))):
            lo, hi = st["spline"].min(axis=(0, 2)) - 2 * big - 1.0, st["spline"].max(axis=(0, 2)) + 2 * big + 1.0
            sub = np.flatnonzero(((X >= lo) & (X <= hi)).all(axis=1))                      # (control nets bound their hulls up to the basis' overshoot: asserted)
            ref = ref_of(pkg, pr, st, P, res, X[sub])
            assert np.all(ref.H.min(axis=(0, 1, 2)) - big > lo) and np.all(ref.H.max(axis=(0, 1, 2)) + big < hi)
            for dist in (offset, big):
                traces = {}
                rows = ref.rows(dist, default_tol(dist, offset, vel_limit), MAX_DEPTH, MAX_WINDOWS, traces=traces)
                live = max([t[1] for tr in traces.values() for t in tr] + [0])
                kept = max([t[2] for tr in traces.values() for t in tr] + [0])
                sure = rows["flags"] & CERTAIN != 0
                width = max([0.0] + list(rows["t_first_hi"][sure] - rows["t_first_lo"][sure]) + list(rows["t_last_hi"][sure] - rows["t_last_lo"][sure]))
                per[(label, dist)] = (len(rows["robot"]), int(np.sum(rows["flags"] & UNCERTAIN != 0)), int(np.sum(rows["flags"] & TRUNCATED != 0)), live, kept,
                                      int(rows["depth"].max()) if len(rows["depth"]) else 0, float(width))
                widest = max(widest, live, kept)
    return max(64, 1 << max(0, math.ceil(math.log2(4 * max(widest, 1))))), per
