"""Reference values for tj_proximity_windows that share no code with csrc/kernels_proximity.h (plain module: no fixtures, no tests).

  proximity_rows      the Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_proximity.py.  Time, hover, hull formation,
                      the cuts, the restriction of both RAW segment hulls and the box skip are audit_timed_ref's and closest_ref's (pieces_of at level 0 through
                      closest_ref.seeds_of, bez_restrict, audit_ref.FastGjk = the oracle's GJK against the origin); what is new:
                        window    lo with its certificate `sep` (closest_ref._Eval's rule), h0 / h5 = the separations attained at ca / cb, ub = the largest
                                  norm3(d_i) over the six points of the same difference net
                        class     OUT: sep and lo > dist | IN: ub <= dist | MIXED: everything else (in this order)
                        listed    (u, q) is listed iff one of its level-0 seeds (those that pass the box prefilter at range = dist) is not OUT
                        search    kept = the IN seeds, live = the MIXED seeds.  A round: a live window with cb - ca <= tol, or whose midpoint
                                  cm = 0.5 * (ca + cb) is not strictly inside, goes to kept as an EDGE leaf; every other is halved, both children from the raw
                                  hulls: OUT dropped, IN to kept, MIXED to the next live set.  Stop: live empty | depth == max_depth | live or kept above
                                  max_windows (TRUNCATED: kept and live of the last completed round; `windows` counts the overflowing round too).  At the end
                                  the live windows become EDGE leaves.
                        merge     leaves by ca; adjacent iff prev.cb == next.ca (asserted: no overlap, ever); a row per maximal chain
                      Rows are sorted by (robot, partner, t_first_lo).
  default_tolerance   the measured table of the header and TJ_PROXIMITY_FRONTIER.
The truth, the slack and the constructed states are audit_timed_ref's."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T
import closest_ref as K
import timing_margin_ref as M

CERTAIN, UNCERTAIN, AT_START, AT_END, RESOLVED, TRUNCATED = 1, 2, 4, 8, 16, 32
MAX_DEPTH, MAX_WINDOWS, TOL_FRACTION = 40, 4096, 0.01
DOUBLES = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "closest", "closest_time")
FIELDS = DOUBLES + ("robot", "partner", "leaves", "depth", "flags", "windows")
OUT, IN, MIXED = 0, 1, 2
INF = math.inf


def default_tol(dist, offset, vel_limit):
    """what tol < 0 selects: the time a robot at the speed limit needs for 1 % of dist (of offset where dist is infinite)"""
    return (TOL_FRACTION * (offset if dist == INF else dist)) / vel_limit


class Eval(K._Eval):
    """closest_ref._Eval's windows with everything a classification needs: (lo, sep, h0, h5, ub) per window (tr, q, j, ca, cb) of robot u"""

    def __call__(self, u, wins):
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
        Dn = np.ascontiguousarray(ra_ - rb_)                                                     # [n][6][3]
        nrm = np.sqrt((Dn[:, :, 0] * Dn[:, :, 0] + Dn[:, :, 1] * Dn[:, :, 1]) + Dn[:, :, 2] * Dn[:, :, 2])   # [n][6]
        ub = nrm.max(axis=1)
        base, oa = Dn.ctypes.data, self.origin.ctypes.data
        out = []
        for n in range(len(wins)):
            lo = self.g.dist(6, base + n * 144, 1, oa)
            v, d = self.g.v, Dn[n]
            sep = float(np.min((v[0] * d[:, 0] + v[1] * d[:, 1]) + v[2] * d[:, 2])) > 0.0
            out.append((lo if sep else 0.0, sep, float(nrm[n, 0]), float(nrm[n, 5]), float(ub[n])))
        return out


def classify(v, dist):
    lo, sep, h0, h5, ub = v
    return OUT if sep and lo > dist else (IN if ub <= dist else MIXED)


def seeds_by_partner(ev, u, dist):
    """{q: ([window], [(lo, sep, h0, h5, ub)])} of robot u: closest_ref.seeds_of's windows at range = dist, evaluated once and filed under their partner"""
    seeds = K.seeds_of(ev, u, dist)
    out = {}
    for w, v in zip(seeds, ev(u, seeds)):
        ws, vs = out.setdefault(w[1], ([], []))
        ws.append(w); vs.append(v)
    return out


def search(ev, u, seeds, vals, dist, tol, max_depth, max_windows, trace=None, dropped=None):
    """the leaves of one directed pair from its seeds, or None if the pair is not listed.  A leaf: (ca, cb, h0, h5, is IN).  trace receives (depth, size of
    the live set, size of the kept list) after the seeding and after every round, the overflowing one included; dropped the OUT windows (ca, cb) of the
    seeding and of the completed rounds."""
    cls = [classify(v, dist) for v in vals]
    if all(c == OUT for c in cls):
        return None
    out_now = [(w[3], w[4]) for w, c in zip(seeds, cls) if c == OUT]
    windows = len(seeds)
    kept = [(w[3], w[4], v[2], v[3], True) for w, v, c in zip(seeds, vals, cls) if c == IN]
    live = [(w, v[2], v[3]) for w, v, c in zip(seeds, vals, cls) if c == MIXED]
    truncated = len(live) > max_windows or len(kept) > max_windows
    if trace is not None:
        trace.append((0, len(live), len(kept)))
    d = 0
    while not truncated and live and d < max_depth:
        kids, new = [], list(kept)
        for (tr, q, j, ca, cb), h0, h5 in live:
            cm = 0.5 * (ca + cb)
            if cb - ca <= tol or not (ca < cm < cb):
                new.append((ca, cb, h0, h5, False))
            else:
                kids += [(tr, q, j, ca, cm), (tr, q, j, cm, cb)]
        kv = ev(u, kids)
        windows += len(kids)
        nxt, out_round = [], []
        for w, v in zip(kids, kv):
            c = classify(v, dist)
            if c == OUT:
                out_round.append((w[3], w[4]))
            elif c == IN:
                new.append((w[3], w[4], v[2], v[3], True))
            elif c == MIXED:
                nxt.append((w, v[2], v[3]))
        if trace is not None:
            trace.append((d + 1, len(nxt), len(new)))
        if len(nxt) > max_windows or len(new) > max_windows:
            truncated = True
            break
        d += 1
        kept, live = new, nxt
        out_now += out_round
    if dropped is not None:
        dropped += out_now
    leaves = kept + [(w[3], w[4], h0, h5, False) for w, h0, h5 in live]
    return dict(leaves=sorted(leaves), depth=d, windows=windows, truncated=truncated)


def chains_of(leaves):
    """maximal chains of adjacent leaves (sorted by ca); the shared cut and midpoint expressions make adjacent ends agree bit for bit, anything else is a gap"""
    out = []
    for k, lf in enumerate(leaves):
        if k:
            assert leaves[k - 1][0] < lf[0] and leaves[k - 1][1] <= lf[0], (leaves[k - 1], lf)     # distinct keys, disjoint windows
        if k and leaves[k - 1][1] == lf[0]:
            out[-1].append(lf)
        else:
            out.append([lf])
    return out


def row_of(chain, dist, tol, t_end, r):
    """the fields of one chain; r: the pair's depth, windows, truncated"""
    sure = []
    within = 0.0
    best = (INF, INF)
    for ca, cb, h0, h5, is_in in chain:
        if is_in:
            sure += [ca, cb]
            within += cb - ca
        else:
            if h0 <= dist:
                sure.append(ca)
            if h5 <= dist:
                sure.append(cb)
        best = min(best, (h0, ca), (h5, cb))
    first_lo, last_hi = chain[0][0], chain[-1][1]
    first_hi, last_lo = (min(sure), max(sure)) if sure else (-1.0, -1.0)
    at_start, at_end = first_lo == 0.0, last_hi == t_end
    flags = (CERTAIN if sure else UNCERTAIN) | (AT_START if at_start else 0) | (AT_END if at_end else 0) | (TRUNCATED if r["truncated"] else 0)
    if sure and (at_start or first_hi - first_lo <= tol) and (at_end or last_hi - last_lo <= tol):
        flags |= RESOLVED
    return dict(t_first_lo=first_lo, t_first_hi=first_hi, t_last_lo=last_lo, t_last_hi=last_hi, within_lo=within, closest=best[0], closest_time=best[1],
                leaves=len(chain), depth=r["depth"], flags=flags, windows=r["windows"])


def proximity_rows(pkg, pr, st, P, res, dist, tol, max_depth=MAX_DEPTH, max_windows=None, owned=None, traces=None, leaves=None, dropped=None):
    """(rows as a dict of numpy arrays [n] in (robot, partner, t_first_lo) order, listed pairs).  dist, tol, max_depth, max_windows: the resolved values.
    traces / leaves / dropped (dicts): per listed pair the search's trace / its sorted leaves / its OUT windows."""
    max_windows = pkg.PROXIMITY_FRONTIER if max_windows is None else max_windows
    U, S = st["spline"].shape[0], P * res
    ev = Eval(pkg, pr, st["spline"], st["piece_time"], P, res)
    rows, n_pairs = [], 0
    for u in (range(U) if owned is None else owned):
        by = seeds_by_partner(ev, u, float(dist))
        t_end = ((S - 1 + 1) / float(res)) * float(ev.pt[u])
        for q in sorted(by):
            tr = [] if traces is not None else None
            out = [] if dropped is not None else None
            r = search(ev, u, by[q][0], by[q][1], float(dist), float(tol), max_depth, max_windows, tr, out)
            if r is None:
                continue
            if dropped is not None:
                dropped[(u, q)] = sorted(out)
            n_pairs += 1
            if traces is not None:
                traces[(u, q)] = tr
            if leaves is not None:
                leaves[(u, q)] = r["leaves"]
            for chain in chains_of(r["leaves"]):
                row = row_of(chain, float(dist), float(tol), t_end, r)
                row.update(robot=u, partner=q)
                rows.append(row)
    return {n: np.array([r[n] for r in rows], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}, n_pairs


# ---- the defaults, measured -----------------------------------------------------------------------------------------------------------------------

STATES = M.STATES
DISTS = (0.1, 1.0)


_MEASURED = {}


def measured(pkg, pr, name, form, dist, offset=0.1, vel_limit=2.0):
    """(state, P, res, rows, listed pairs, traces, leaves, dropped) of a named end state at the default tol, max_depth = 40 and the lists capped at
    MAX_WINDOWS only; computed once per process (the tests share it with default_tolerance, and never write to it)"""
    key = (name, form, dist, offset, vel_limit)
    if key not in _MEASURED:
        st, P, res = M.state_named(name, form)
        traces, leaves, dropped = {}, {}, {}
        rows, n_pairs = proximity_rows(pkg, pr, st, P, res, dist, default_tol(dist, offset, vel_limit), MAX_DEPTH, MAX_WINDOWS, traces=traces, leaves=leaves, dropped=dropped)
        _MEASURED[key] = (st, P, res, rows, n_pairs, traces, leaves, dropped)
    return _MEASURED[key]


def default_tolerance(pkg, pr, names=STATES, dists=DISTS, offset=0.1, vel_limit=2.0):
    """(frontier, per (state, dist): (listed pairs, rows, UNCERTAIN rows, TRUNCATED rows, largest live set, largest kept list, largest depth, widest
    bracket)): the default tol, max_depth = 40, the lists capped at MAX_WINDOWS only.  The widest bracket is the largest of t_first_hi - t_first_lo and
    t_last_hi - t_last_lo over the CERTAIN rows.  The frontier is the next power of two >= 4 x the larger of the two list maxima, at least 64."""
    per, widest = {}, 0
    for name, form in names:
        for dist in dists:
            _, _, _, rows, n_pairs, traces, _, _ = measured(pkg, pr, name, form, dist, offset, vel_limit)
            live = max([t[1] for tr in traces.values() for t in tr] + [0])
            kept = max([t[2] for tr in traces.values() for t in tr] + [0])
            sure = rows["flags"] & CERTAIN != 0
            width = max([0.0] + list(rows["t_first_hi"][sure] - rows["t_first_lo"][sure]) + list(rows["t_last_hi"][sure] - rows["t_last_lo"][sure]))
            per[(name + form, dist)] = (n_pairs, len(rows["robot"]), int(np.sum(rows["flags"] & UNCERTAIN != 0)), int(np.sum(rows["flags"] & TRUNCATED != 0)),
                                        live, kept, int(rows["depth"].max()) if len(rows["depth"]) else 0, float(width))
            widest = max(widest, live, kept)
    return max(64, 1 << max(0, math.ceil(math.log2(4 * max(widest, 1))))), per
