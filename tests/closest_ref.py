"""Reference values for tj_closest_approach that share no code with csrc/kernels_closest.h (plain module: no fixtures, no tests).

  closest_records     the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_closest.py.  Time, hover, hull
                      formation, the cuts, the restriction of both RAW segment hulls and the box skip are audit_timed_ref's (pieces_of at level 0,
                      bez_restrict, audit_ref.FastGjk = the oracle's GJK against the origin); what is new is the certificate on lo (see _Eval) and the search:
                        seeds     every level-0 window (tr, q, j, ca, cb) that passes the box prefilter, evaluated; best = the smallest hi < range in the
                                  order (hi, segment, partner, time); live = {lo < range and lo < best.hi}
                        round d   every live window is halved at cm = 0.5 * (ca + cb) (cm == ca or cm == cb: it stays, terminal); both children are
                                  evaluated from the raw hulls; best over (best, children); live = children and terminals with lo < best.hi
                        bracket   lo_u = min(best.hi, min lo over live), hi_u = best.hi
                        stop      hi - lo <= tol | live empty | every live window terminal | d == max_depth | more than max_windows live (TRUNCATED:
                                  the record of the last completed round; `windows` still counts the round that overflowed)
                      The rounds are level-synchronous and every comparison is against the round's final best: the live SET, and with it every field of
                      the record, is independent of the order of evaluation.
  default_tolerance   the measured TJ_CLOSEST_TOL (the manner of audit_timed_ref.default_level_widths).
The truth, the slack and the constructed states are audit_timed_ref's."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T

CONTACT, CLEAR, CONVERGED, TRUNCATED = 1, 2, 4, 8
MAX_DEPTH, FRONTIER = 40, 4096
FIELDS = ("lo", "hi", "time", "robot", "segment", "depth", "flags", "windows")


class _Eval:
    """lo, hi and the time of the hi sample of windows (tr, q, j, ca, cb) of robot u, from the raw hulls.  lo is the CERTIFIED lower bound: the GJK's |v| where
    its v separates the origin from the difference hull (v . d_i > 0 for all six points: the regime in which |v| is at rounding level), 0 otherwise (the GJK
    stops at up to ~1e-5 for an origin inside the hull, DESIGN.md 3c: its value is no lower bound there)"""

    def __init__(self, pkg, pr, spline, pt, P, res):
        self.pt, self.S, self.rf = np.asarray(pt, dtype=np.float64), P * res, float(res)
        H = R.hulls_of(pkg, np.asarray(spline, dtype=np.float64), P, res)
        self.H = H
        self.HX = np.concatenate([H, np.repeat(H[:, self.S - 1:self.S, 5:6, :], 6, axis=2)], axis=1)   # row S: the hover body
        self.g = R.FastGjk(pr)
        self.origin = np.zeros(3)

    def __call__(self, u, wins):
        """-> list of (lo, hi, time)"""
        if not wins:
            return []
        S, rf, ptu = self.S, self.rf, float(self.pt[u])
        A, B, SA, SB, RA, RB, HOV = [], [], [], [], [], [], []
        for (tr, q, j, ca, cb) in wins:
            ptq = float(self.pt[q])
            T0u, T1u = (tr / rf) * ptu, ((tr + 1) / rf) * ptu
            lenu = T1u - T0u
            Tj, Tj1 = (j / rf) * ptq, ((j + 1) / rf) * ptq
            lenq = Tj1 - Tj
            A.append(self.H[u, tr]); B.append(self.HX[q, j]); HOV.append(j >= S)
            SA.append(T.clamp01((ca - T0u) / lenu)); SB.append(T.clamp01((cb - T0u) / lenu))
            RA.append(T.clamp01((ca - Tj) / lenq)); RB.append(T.clamp01((cb - Tj) / lenq))
        A, B = np.array(A), np.array(B)
        ra_ = T.bez_restrict(A, SA, SB)
        rb_ = np.where(np.array(HOV)[:, None, None], B, T.bez_restrict(B, RA, RB))
        Dn = np.ascontiguousarray(ra_ - rb_)
        d0, d5 = Dn[:, 0], Dn[:, 5]
        h0 = np.sqrt((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2])
        h5 = np.sqrt((d5[:, 0] * d5[:, 0] + d5[:, 1] * d5[:, 1]) + d5[:, 2] * d5[:, 2])
        base, oa = Dn.ctypes.data, self.origin.ctypes.data
        out = []
        for n, (tr, q, j, ca, cb) in enumerate(wins):
            lo = self.g.dist(6, base + n * 144, 1, oa)
            v, d = self.g.v, Dn[n]
            if not float(np.min((v[0] * d[:, 0] + v[1] * d[:, 1]) + v[2] * d[:, 2])) > 0.0:   # no separating plane: the origin may be inside the hull
                lo = 0.0
            first = h0[n] <= h5[n]
            out.append((lo, float(h0[n] if first else h5[n]), ca if first else cb))
        return out


def seeds_of(ev, u, rng):
    """the windows tj_audit_timed evaluates at levels = 0 for robot u: same expressions, same box prefilter"""
    HX, S, rf, pt = ev.HX, ev.S, ev.rf, ev.pt
    U = HX.shape[0]
    blo, bhi = HX.min(axis=2), HX.max(axis=2)
    Tj = (np.arange(S + 2) / rf)[None, :] * pt[:, None]
    Tj[:, S + 1] = np.inf
    guard = rng * 1.000001 + 1e-9
    P, res = S // int(rf), int(rf)
    out = []
    for tr in range(S):
        gap = np.maximum(blo - bhi[u, tr], blo[u, tr] - bhi)
        near = ~(gap > guard).any(axis=2)
        cand = near & (Tj[:, :S + 1] <= Tj[u, tr + 1]) & (Tj[:, 1:] >= Tj[u, tr])
        cand[u] = False
        for q in np.flatnonzero(cand.any(axis=1)):
            for (w, j, ca, cb, sa, sb, ra, rb) in T.pieces_of(pt, P, res, u, tr, int(q), 0):
                if near[q, j]:
                    out.append((tr, int(q), j, ca, cb))
    return out


def search(ev, u, rng, tol, max_depth, max_windows, trace=None):
    """the record of robot u as a dict; trace (a list) receives (depth, lo, hi) of every completed round"""
    NONE = (rng, math.inf, math.inf, math.inf)                      # (hi, segment, partner, time): the total order of `best`
    seeds = seeds_of(ev, u, rng)
    vals = ev(u, seeds)
    windows = len(seeds)
    best = min([(hi, w[0], w[1], t) for w, (lo, hi, t) in zip(seeds, vals) if hi < rng] + [NONE])
    live = [(w, lo, False) for w, (lo, hi, t) in zip(seeds, vals) if lo < rng and lo < best[0]]   # (window, lo, terminal)
    rec = dict(best=best, lo=min([best[0]] + [l for _, l, _ in live]), depth=0)
    truncated = len(live) > max_windows
    if trace is not None:
        trace.append((0, rec["lo"], best[0]))
    d = 0
    while not truncated:
        if rec["best"][0] - rec["lo"] <= tol or not live or all(t for _, _, t in live) or d == max_depth:
            break
        kids, terms = [], []
        for (tr, q, j, ca, cb), lo, term in live:
            cm = 0.5 * (ca + cb)
            if term or cm == ca or cm == cb:
                terms.append(((tr, q, j, ca, cb), lo, True))
            else:
                kids += [(tr, q, j, ca, cm), (tr, q, j, cm, cb)]
        vals = ev(u, kids)
        windows += len(kids)
        best = min([rec["best"]] + [(hi, w[0], w[1], t) for w, (lo, hi, t) in zip(kids, vals) if hi < rng])
        nxt = [(w, lo, False) for w, (lo, hi, t) in zip(kids, vals) if lo < best[0]] + [x for x in terms if x[1] < best[0]]
        if len(nxt) > max_windows:
            truncated = True
            break
        d += 1
        live = nxt
        rec = dict(best=best, lo=min([best[0]] + [l for _, l, _ in live]), depth=d)
        if trace is not None:
            trace.append((d, rec["lo"], best[0]))
    hi, seg, q, t = rec["best"]
    found = q != math.inf
    return dict(lo=rec["lo"], hi=hi, time=t if found else -1.0, robot=q if found else -1, segment=seg if found else -1, depth=rec["depth"], windows=windows,
                live_empty=not live and not truncated, truncated=truncated)


def flags_of(r, offset, tol):
    return ((CONTACT if r["robot"] >= 0 and r["hi"] <= offset else 0) | (CLEAR if r["lo"] > offset else 0) |
            (CONVERGED if r["hi"] - r["lo"] <= tol or r["live_empty"] else 0) | (TRUNCATED if r["truncated"] else 0))


def closest_records(pkg, pr, st, P, res, rng, offset, tol, max_depth=MAX_DEPTH, max_windows=FRONTIER, owned=None, traces=None):
    """per robot the record's fields, in tj_closest_robot's names (robots outside `owned`: zero).  rng, tol, max_depth, max_windows: the resolved values."""
    U = st["spline"].shape[0]
    ev = _Eval(pkg, pr, st["spline"], st["piece_time"], P, res)
    out = {n: np.zeros(U, dtype=np.float64 if n in FIELDS[:3] else np.int32) for n in FIELDS}
    for u in (range(U) if owned is None else owned):
        tr = [] if traces is not None else None
        r = search(ev, u, float(rng), float(tol), max_depth, max_windows, tr)
        r["flags"] = flags_of(r, offset, tol)
        for n in FIELDS:
            out[n][u] = r[n]
        if traces is not None:
            traces[u] = tr
    return out


def single_uav_record(rng):
    return dict(lo=rng, hi=rng, time=-1.0, robot=-1, segment=-1, depth=0, flags=CLEAR | CONVERGED, windows=0)


def level_window_count(pkg, st, P, res, u, rng, L):
    """how many windows tj_audit_timed evaluates for robot u at level L (the uniform cost tj_closest_approach is set against)"""
    H = R.hulls_of(pkg, np.asarray(st["spline"], dtype=np.float64), P, res)
    S, rf, pt = P * res, float(res), np.asarray(st["piece_time"], dtype=np.float64)
    HX = np.concatenate([H, np.repeat(H[:, S - 1:S, 5:6, :], 6, axis=2)], axis=1)
    blo, bhi = HX.min(axis=2), HX.max(axis=2)
    guard = rng * 1.000001 + 1e-9
    n = 0
    for tr in range(S):
        near = ~(np.maximum(blo - bhi[u, tr], blo[u, tr] - bhi) > guard).any(axis=2)
        for q in range(H.shape[0]):
            if q != u and near[q].any():
                n += sum(1 for p in T.pieces_of(pt, P, res, u, tr, q, L) if near[q, p[1]])
    return n


def default_tolerance(pkg, pr, names=("e2e_scn_b", "e2e_scn_c3", "e2e_scn_b_coupled"), rng=0.1 + 2 * 0.1, offset=0.1):
    """(widths per depth 0..40, floor depth, tolerance): tol = 0 and max_depth = 40 on the named end states; per depth the largest hi - lo over the robots
    with a partner in range (a robot whose search has ended keeps its last bracket).  The floor is the first depth after which the width no longer shrinks
    by at least 2x; a width of exactly 0 (every live set has emptied: hi == lo, nothing is left to shrink) is the end of the table, so a sequence that
    shrinks all the way has its floor at the last depth with a positive width.  The tolerance is the smallest power of ten >= 10 x the width at the floor."""
    widths = [0.0] * (MAX_DEPTH + 1)
    for name in names:
        st, P, res = T.e2e_state(name)
        traces = {}
        rec = closest_records(pkg, pr, st, P, res, rng, offset, 0.0, MAX_DEPTH, FRONTIER, traces=traces)
        for u, tr in traces.items():
            if rec["robot"][u] < 0:
                continue
            for d in range(MAX_DEPTH + 1):
                _, lo, hi = tr[min(d, len(tr) - 1)]
                widths[d] = max(widths[d], hi - lo)
    floor = next((d for d in range(MAX_DEPTH) if widths[d + 1] == 0.0 or not widths[d + 1] <= widths[d] / 2), MAX_DEPTH)
    return widths, floor, 10.0 ** math.ceil(math.log10(10 * widths[floor]))
