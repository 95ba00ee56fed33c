"""Reference values for tj_timing_margin that share no code with csrc/kernels_timing_margin.h (plain module: no fixtures, no tests).

  Ref.rows            the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_timing_margin.py.  Items, nets,
                      the box test and the GJK with its certificate are path_crossing_ref.Ref's (the crossings' restatement: hulls by audit_ref.hulls_of,
                      windows by audit_timed_ref.bez_restrict from the RAW hulls, the oracle's GJK).  What is this query's own:
                        clock     T_r(g, s) = ((g + s) / res) * piece_time[r]; the last control point (g == S - 1, s == 1.0) has the clock set [T, +inf),
                                  every other point {T}; slip of two points = max(0, lo_u - hi_q, lo_q - hi_u)
                        OUT       cross_lo(W) > dist: klo = +inf.  Otherwise klo(W) = max(0, ta_u - tb_q, ta_q - tb_u), tb = +inf where the window ends
                                  on the last control point
                        corners   the four end-point pairs with norm3(a_i - b_k) <= dist, each with the slip of its two points
                        same time not OUT and klo == 0: tau = max(ta_u, ta_q, 0), each robot's x = (tau - T(g, 0)) / (T(g + 1, 0) - T(g, 0)) clamped
                                  into the item's window, position = b_0 of the raw hull restricted to [x, x]; within dist: slip 0.0, SAME_TIME
                        order     candidates with slip < max_slip by (slip, segment, partner_segment, s, partner_s), a corner before a same-time
                                  candidate of the same place
                        seeds     every (tr, j) whose raw hull boxes pass the box test at dist, full windows, evaluated like a round's children
                        listed    iff some seed has a candidate or is not OUT with klo < max_slip
                        round d   every live item into its four quadrants, best over (best, children), live = children with klo < best.hi -- the FINAL
                        bracket   lo = min(best.hi, min klo over live), hi = best.hi
                        stop      hi - lo <= tol | live empty | d == max_depth | more than max_windows live (TRUNCATED: the last completed round)
  sampled_margin      nothing of GJK or subdivision in it: both flown curves in np.longdouble on a grid per segment, the smallest clock-set distance over
                      all sample pairs within a distance.
  default_tolerance   the measured TJ_MARGIN_FRONTIER and the header's table.
The slack is audit_timed_ref's (two curves restricted to windows: the same operations)."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import path_crossing_ref as X

LD = np.longdouble
CONTACT, CLEAR, CONVERGED, TRUNCATED, ROBOT_END, PARTNER_END, SAME_TIME = 1, 2, 4, 8, 16, 32, 64
MAX_DEPTH, MAX_WINDOWS, TOL_FRACTION = 40, 4096, 0.01
DOUBLES = ("lo", "hi", "distance", "s", "partner_s", "time", "partner_time")
FIELDS = DOUBLES + ("robot", "partner", "segment", "partner_segment", "depth", "flags", "windows")
INF = math.inf
NONE = (INF, INF, INF, INF, 0, -1.0)   # behind the slip: (segment, partner_segment, s, partner_s, same time, distance)


def default_tol(dist, vel_limit):
    return (TOL_FRACTION * dist) / vel_limit


class Ref:
    """the restatement on one state; hover=False switches the last control point's clock set [T, +inf) off (every point {T}): tests only"""

    def __init__(self, pkg, pr, st, P, res, hover=True):
        self.x = X.Ref(pkg, pr, st, P, res)
        self.pt, self.S, self.rf, self.U, self.H, self.hover = self.x.pt, self.x.S, self.x.rf, self.x.U, self.x.H, hover

    def clock(self, r, g, s):
        return ((np.asarray(g, dtype=np.float64) + s) / self.rf) * float(self.pt[r])

    def clock_end(self, r, g, s):
        """the upper end of a point's clock set"""
        t = self.clock(r, g, s)
        return np.where((np.asarray(g) == self.S - 1) & (np.asarray(s) == 1.0), INF, t) if self.hover else t

    def evaluate(self, u, q, tr, j, sa, sb, ra, rb, dist, max_slip):
        """one batch of items -> klo[n] (+inf: OUT) and the candidates as a list of tuples (slip, segment, partner_segment, s, partner_s, same, distance)"""
        n = len(tr)
        if n == 0:
            return np.zeros(0), []
        lo, h, s, ps = self.x.evaluate(u, q, tr, j, sa, sb, ra, rb)
        out = lo > dist
        ta_u, tb_u, ta_q, tb_q = self.clock(u, tr, sa), self.clock_end(u, tr, sb), self.clock(q, j, ra), self.clock_end(q, j, rb)
        klo = np.where(out, INF, np.maximum(0.0, np.maximum(ta_u - tb_q, ta_q - tb_u)))
        cands = []
        for e in range(4):
            lo_u, hi_u, lo_q, hi_q = self.clock(u, tr, s[:, e]), self.clock_end(u, tr, s[:, e]), self.clock(q, j, ps[:, e]), self.clock_end(q, j, ps[:, e])
            slip = np.maximum(0.0, np.maximum(lo_u - hi_q, lo_q - hi_u))
            for k in np.nonzero((h[:, e] <= dist) & (slip < max_slip))[0]:
                cands.append((float(slip[k]), int(tr[k]), int(j[k]), float(s[k, e]), float(ps[k, e]), 0, float(h[k, e])))
        m = np.nonzero(~out & (klo == 0.0))[0]
        if len(m) and 0.0 < max_slip:
            tau = np.maximum(np.maximum(ta_u[m], ta_q[m]), 0.0)
            xs = []
            for r, g, a, b in ((u, tr[m], sa[m], sb[m]), (q, j[m], ra[m], rb[m])):
                t0, t1 = self.clock(r, g, 0.0), self.clock(r, g + 1, 0.0)
                xs.append(np.minimum(np.maximum((tau - t0) / (t1 - t0), a), b))
            pu = T.bez_restrict(self.H[u, tr[m]], xs[0], xs[0])[:, 0]
            pq = T.bez_restrict(self.H[q, j[m]], xs[1], xs[1])[:, 0]
            d = X._norm3(pu - pq)
            for k in np.nonzero(d <= dist)[0]:
                cands.append((0.0, int(tr[m[k]]), int(j[m[k]]), float(xs[0][k]), float(xs[1][k]), 1, float(d[k])))
        return klo, cands

    def search(self, u, q, dist, max_slip, tol, max_depth, max_windows, trace=None):
        """the record of the pair u < q as a dict, or None where it is not listed; trace receives (depth, lo, hi, live) of every completed round"""
        tr, j = self.x.seeds(u, q, dist)
        one, zero = np.ones(len(tr)), np.zeros(len(tr))
        klo, cands = self.evaluate(u, q, tr, j, zero, one, zero, one, dist, max_slip)
        if not (cands or np.any(klo < max_slip)):
            return None
        windows = len(tr)
        best = min([(max_slip,) + NONE] + cands)
        keep = klo < best[0]
        live = (tr[keep], j[keep], zero[keep], one[keep], zero[keep], one[keep], klo[keep])
        rec = dict(best=best, lo=min([best[0]] + live[6].tolist()), depth=0)
        truncated = len(live[0]) > max_windows
        if trace is not None:
            trace.append((0, rec["lo"], best[0], len(live[0])))
        d = 0
        while not truncated:
            if rec["best"][0] - rec["lo"] <= tol or len(live[0]) == 0 or d == max_depth:
                break
            ltr, lj, sa, sb, ra, rb, _ = live
            sm, rm = 0.5 * (sa + sb), 0.5 * (ra + rb)
            ktr, kj = np.tile(ltr, 4), np.tile(lj, 4)
            ksa, ksb = np.concatenate([sa, sm, sa, sm]), np.concatenate([sm, sb, sm, sb])
            kra, krb = np.concatenate([ra, ra, rm, rm]), np.concatenate([rm, rm, rb, rb])
            klo, cands = self.evaluate(u, q, ktr, kj, ksa, ksb, kra, krb, dist, max_slip)
            windows += len(ktr)
            best = min([rec["best"]] + cands)
            keep = klo < best[0]
            if int(keep.sum()) > max_windows:
                truncated = True
                if trace is not None:
                    trace.append((d + 1, None, None, int(keep.sum())))
                break
            d += 1
            live = (ktr[keep], kj[keep], ksa[keep], ksb[keep], kra[keep], krb[keep], klo[keep])
            rec = dict(best=best, lo=min([best[0]] + live[6].tolist()), depth=d)
            if trace is not None:
                trace.append((d, rec["lo"], best[0], len(live[0])))
        hi, seg, pseg, s_u, s_q, same, distance = rec["best"]
        found = seg != INF
        return dict(lo=rec["lo"], hi=hi, distance=distance if found else -1.0, s=s_u if found else -1.0, partner_s=s_q if found else -1.0,
                    time=((seg + s_u) / self.rf) * float(self.pt[u]) if found else -1.0, partner_time=((pseg + s_q) / self.rf) * float(self.pt[q]) if found else -1.0,
                    robot=u, partner=q, segment=seg if found else -1, partner_segment=pseg if found else -1, depth=rec["depth"], windows=windows,
                    live_empty=len(live[0]) == 0 and not truncated, truncated=truncated, found=found, same=bool(found and same))

    def flags_of(self, r, tol):
        return ((CONTACT if r["found"] and r["hi"] <= 0.0 else 0) | (CLEAR if r["lo"] > 0.0 else 0) |
                (CONVERGED if r["hi"] - r["lo"] <= tol or r["live_empty"] else 0) | (TRUNCATED if r["truncated"] else 0) |
                (ROBOT_END if r["found"] and r["segment"] == self.S - 1 and r["s"] == 1.0 else 0) |
                (PARTNER_END if r["found"] and r["partner_segment"] == self.S - 1 and r["partner_s"] == 1.0 else 0) | (SAME_TIME if r["same"] else 0))

    def rows(self, dist, max_slip, tol, max_depth=MAX_DEPTH, max_windows=MAX_WINDOWS, owned=None, pairs=None, traces=None):
        """the rows in (robot, partner) order as a dict of numpy arrays [n].  dist, max_slip, tol, max_depth, max_windows: the resolved values.  pairs: only these."""
        out = []
        todo = pairs if pairs is not None else [(u, q) for u in (range(self.U) if owned is None else owned) for q in range(u + 1, self.U)]
        for u, q in sorted(todo):
            tr = [] if traces is not None else None
            r = self.search(u, q, float(dist), float(max_slip), float(tol), max_depth, max_windows, tr)
            if r is None:
                continue
            r["flags"] = self.flags_of(r, tol)
            out.append(r)
            if traces is not None:
                traces[(u, q)] = tr
        return {n: np.array([r[n] for r in out], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}


def rows_of(pkg, pr, st, P, res, dist, max_slip, tol, max_depth=MAX_DEPTH, max_windows=MAX_WINDOWS, owned=None, pairs=None, traces=None, hover=True):
    return Ref(pkg, pr, st, P, res, hover).rows(dist, max_slip, tol, max_depth, max_windows, owned, pairs, traces)


# ---- the truth: the flown curves themselves -------------------------------------------------------------------------------------------------------

def sampled_margin(pkg, ref, st, P, res, u, q, dist, m=21):
    """the smallest clock-set distance over the m x m samples of every segment pair whose distance (np.longdouble) is <= dist: an upper bound of the pair's
    margin at the contact distance `dist`; inf without such a sample pair.  Clock sets as the definition's: the last sample of the last segment is [T, +inf)."""
    S = P * res
    a, b = X.segment_samples(pkg, st, P, res, u, m), X.segment_samples(pkg, st, P, res, q, m)
    par = np.linspace(LD(0), LD(1), m, dtype=LD)
    clock = lambda r: ((np.arange(S, dtype=LD)[:, None] + par[None, :]) / LD(res)) * LD(st["piece_time"][r])       # [S][m]
    cu, cq = clock(u), clock(q)
    eu, eq = cu.copy(), cq.copy()
    eu[S - 1, m - 1] = eq[S - 1, m - 1] = np.inf
    best = math.inf
    for tr in range(S):
        d = a[tr][None, :, None, :] - b[:, None, :, :]                                                             # [S][m][m][3]
        near = np.sqrt((d * d).sum(axis=-1)) <= dist
        if not near.any():
            continue
        slip = np.maximum(0, np.maximum(cu[tr][None, :, None] - eq[:, None, :], cq[:, None, :] - eu[tr][None, :, None]))
        best = min(best, float(slip[near].min()))
    return best


def clock_set_distance(ref, r):
    """the slip of a found row's sample, from its places alone"""
    u, q = int(r["robot"]), int(r["partner"])
    lo_u, hi_u = float(ref.clock(u, r["segment"], r["s"])), float(ref.clock_end(u, r["segment"], r["s"]))
    lo_q, hi_q = float(ref.clock(q, r["partner_segment"], r["partner_s"])), float(ref.clock_end(q, r["partner_segment"], r["partner_s"]))
    return max(0.0, lo_u - hi_q, lo_q - hi_u)


def staggered(st, step=0.03):
    out = {k: np.array(v) for k, v in st.items()}
    out["piece_time"] = out["piece_time"] * (1 + step * np.arange(len(out["piece_time"])))
    return out


# ---- the defaults, measured -----------------------------------------------------------------------------------------------------------------------

STATES = (("e2e_scn_b", ""), ("e2e_scn_c3", ""), ("e2e_scn_b_coupled", ""), ("e2e_scn_c3", "_flat"), ("e2e_scn_c3", "_flat_staggered"))


def state_named(name, form):
    st, P, res = T.e2e_state(name)
    if form.startswith("_flat"):
        st = X.flattened(st)
    if form.endswith("_staggered"):
        st = staggered(st)
    return st, P, res


def default_tolerance(pkg, pr, names=STATES, dist=0.1, vel_limit=2.0, pairs=None):
    """(tolerance, frontier, per state (listed pairs, rows with hi == 0, truncated rows, largest live set, largest depth, widest bracket)): default dist,
    max_slip = inf, the default tol, max_depth = 40, the live set capped at MAX_WINDOWS only.  The frontier is the next power of two >= 2 x the largest live
    set, at least 64, capped at MAX_WINDOWS.  pairs: a function (state's name, U) -> the pairs to search, or None = all."""
    tol, per, widest = default_tol(dist, vel_limit), {}, 0
    for name, form in names:
        st, P, res = state_named(name, form)
        traces = {}
        todo = pairs(name + form, st["spline"].shape[0]) if pairs else None
        rows = rows_of(pkg, pr, st, P, res, dist, INF, tol, MAX_DEPTH, MAX_WINDOWS, pairs=todo, traces=traces)
        big = max([t[3] for tr in traces.values() for t in tr] + [0])
        width = rows["hi"] - rows["lo"]
        per[name + form] = (len(rows["robot"]), int(np.sum(rows["hi"] == 0.0)), int(np.sum(rows["flags"] & TRUNCATED != 0)), big,
                            int(rows["depth"].max()) if len(width) else 0, float(np.nanmax(width)) if len(width) else 0.0)
        widest = max(widest, big)
    frontier = min(MAX_WINDOWS, max(64, 1 << max(0, math.ceil(math.log2(2 * max(widest, 1))))))
    return tol, frontier, per
