"""Reference values for tj_path_crossings that share no code with csrc/kernels_path_crossing.h (plain module: no fixtures, no tests).

  Ref.rows            the numpy / Python restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_path_crossing.py.  Hulls by
                      audit_ref.hulls_of (hull_entry's sums); the nets of an item by audit_timed_ref.bez_restrict from the RAW hulls (elementwise blossoming:
                      the same IEEE operations); lo through the ORACLE's GJK (audit_ref.FastGjk, 6 points against 6, the lower robot index = body 1) with the
                      certificate v . (a_i - b_k) > 0 over the 36 vertex pairs, 0 without it; hi = the smallest of the four end-point distances
                      norm3(a_i - b_k), i, k in {0, 5}; the search level by level, per unordered pair u < q:
                        seeds     every (tr, j) whose raw hull boxes pass the box test at `range`, both windows [0, 1]
                        listed    iff some seed has lo < range or hi < range
                        best      the smallest hi < range in the order (hi, segment, partner_segment, s, partner_s); live = {lo < range and lo < best.hi}
                        round d   every live item into its four quadrants (both windows halved), all children from the raw hulls; best over (best,
                                  children); live = children with lo < best.hi -- against the round's FINAL best
                        bracket   lo = min(best.hi, min lo over live), hi = best.hi
                        stop      hi - lo <= tol | live empty | d == max_depth | more than max_windows live (TRUNCATED: the record of the last completed
                                  round; `windows` still counts the round that overflowed)
  sampled_minimum     nothing of GJK or subdivision in it: both flown curves from `convert` in np.longdouble on a grid per segment, all pairs of samples.
  constructed states  lines_state (two straight nets), arcs_state (a valley: a wide live set).
  default_tolerance   the measured TJ_CROSSING_TOL and TJ_CROSSING_FRONTIER.
The slack is audit_timed_ref's (counted there for two curves restricted to windows: the same operations)."""
import math

import numpy as np

import audit_ref as R
import audit_timed_ref as T

LD = np.longdouble
CONTACT, CLEAR, CONVERGED, TRUNCATED, ROBOT_END, PARTNER_END = 1, 2, 4, 8, 16, 32
MAX_DEPTH, MAX_WINDOWS = 40, 4096
DOUBLES = ("lo", "hi", "s", "partner_s", "time", "partner_time")
FIELDS = DOUBLES + ("robot", "partner", "segment", "partner_segment", "depth", "flags", "windows")


def _norm3(d):
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


class Ref:
    """the restatement on one state"""

    def __init__(self, pkg, pr, st, P, res):
        self.pt, self.S, self.rf = np.asarray(st["piece_time"], dtype=np.float64), P * res, float(res)
        self.H = np.ascontiguousarray(R.hulls_of(pkg, np.asarray(st["spline"], dtype=np.float64), P, res))     # [U][S][6][3]
        self.U = self.H.shape[0]
        self.blo, self.bhi = self.H.min(axis=2), self.H.max(axis=2)                                            # [U][S][3]
        self.g = R.FastGjk(pr)

    def seeds(self, u, q, rng):
        """(tr[n], j[n]) in (tr, j) order: the segment pairs whose raw hull boxes are within `range` on every axis (box_near's expression and guard)"""
        gap = np.maximum(self.blo[q][None, :, :] - self.bhi[u][:, None, :], self.blo[u][:, None, :] - self.bhi[q][None, :, :])   # [S][S][3]
        near = ~(gap > rng * 1.000001 + 1e-9).any(axis=2)
        return np.nonzero(near)

    def evaluate(self, u, q, tr, j, sa, sb, ra, rb):
        """one batch of items -> lo[n] and the four attained candidates per item: h[n][4], s[n][4], ps[n][4]"""
        n = len(tr)
        if n == 0:
            return np.zeros(0), np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((0, 4))
        A = np.ascontiguousarray(T.bez_restrict(self.H[u, tr], sa, sb))              # [n][6][3], always from the raw hulls
        B = np.ascontiguousarray(T.bez_restrict(self.H[q, j], ra, rb))
        V = np.zeros((n, 3))
        f, ab, bb, vb = self.g.f, A.ctypes.data, B.ctypes.data, V.ctypes.data
        for k in range(n):
            f(6, ab + k * 144, 6, bb + k * 144, vb + k * 24)
        lo = _norm3(V)
        m = np.full(n, np.inf)
        for a in range(6):
            for b in range(6):
                d = A[:, a] - B[:, b]
                m = np.minimum(m, (V[:, 0] * d[:, 0] + V[:, 1] * d[:, 1]) + V[:, 2] * d[:, 2])
        lo = np.where(m > 0.0, lo, 0.0)                                               # no separating direction: the hulls may touch
        h = np.stack([_norm3(A[:, i] - B[:, k]) for i in (0, 5) for k in (0, 5)], axis=1)
        s = np.stack([sa, sa, sb, sb], axis=1)
        ps = np.stack([ra, rb, ra, rb], axis=1)
        return lo, h, s, ps

    def search(self, u, q, rng, tol, max_depth, max_windows, trace=None):
        """the record of the pair u < q as a dict, or None where it is not listed; trace receives (depth, lo, hi, live) of every completed round"""
        tr, j = self.seeds(u, q, rng)
        one, zero = np.ones(len(tr)), np.zeros(len(tr))
        lo, h, s, ps = self.evaluate(u, q, tr, j, zero, one, zero, one)
        if not (np.any(lo < rng) or np.any(h < rng)):
            return None
        windows = len(tr)

        def better(best, tr, j, h, s, ps):
            ok = np.nonzero(h < rng)
            if len(ok[0]):
                hh, ss, pp, tt, jj = h[ok], s[ok], ps[ok], tr[ok[0]], j[ok[0]]
                k = np.lexsort((pp, ss, jj, tt, hh))[0]
                best = min(best, (float(hh[k]), int(tt[k]), int(jj[k]), float(ss[k]), float(pp[k])))
            return best

        best = better((rng, math.inf, math.inf, math.inf, math.inf), tr, j, h, s, ps)   # (hi, segment, partner_segment, s, partner_s): the total order
        keep = (lo < rng) & (lo < best[0])
        live = (tr[keep], j[keep], zero[keep], one[keep], zero[keep], one[keep], lo[keep])
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
            klo, kh, ks, kps = self.evaluate(u, q, ktr, kj, ksa, ksb, kra, krb)
            windows += len(ktr)
            best = better(rec["best"], ktr, kj, kh, ks, kps)
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
        hi, seg, pseg, s_u, s_q = rec["best"]
        found = seg != math.inf
        return dict(lo=rec["lo"], hi=hi, s=s_u if found else -1.0, partner_s=s_q if found else -1.0,
                    time=((seg + s_u) / self.rf) * float(self.pt[u]) if found else -1.0, partner_time=((pseg + s_q) / self.rf) * float(self.pt[q]) if found else -1.0,
                    robot=u, partner=q, segment=seg if found else -1, partner_segment=pseg if found else -1, depth=rec["depth"], windows=windows,
                    live_empty=len(live[0]) == 0 and not truncated, truncated=truncated, found=found)

    def flags_of(self, r, offset, tol):
        return ((CONTACT if r["found"] and r["hi"] <= offset else 0) | (CLEAR if r["lo"] > offset else 0) |
                (CONVERGED if r["hi"] - r["lo"] <= tol or r["live_empty"] else 0) | (TRUNCATED if r["truncated"] else 0) |
                (ROBOT_END if r["found"] and r["segment"] == self.S - 1 and r["s"] == 1.0 else 0) |
                (PARTNER_END if r["found"] and r["partner_segment"] == self.S - 1 and r["partner_s"] == 1.0 else 0))

    def rows(self, rng, offset, tol, max_depth=MAX_DEPTH, max_windows=MAX_WINDOWS, owned=None, pairs=None, traces=None):
        """the rows in (robot, partner) order as a dict of numpy arrays [n].  rng, tol, max_depth, max_windows: the resolved values.  pairs: only these."""
        out = []
        todo = pairs if pairs is not None else [(u, q) for u in (range(self.U) if owned is None else owned) for q in range(u + 1, self.U)]
        for u, q in sorted(todo):
            tr = [] if traces is not None else None
            r = self.search(u, q, float(rng), float(tol), max_depth, max_windows, tr)
            if r is None:
                continue
            r["flags"] = self.flags_of(r, offset, tol)
            out.append(r)
            if traces is not None:
                traces[(u, q)] = tr
        return {n: np.array([r[n] for r in out], dtype=np.float64 if n in DOUBLES else np.int32) for n in FIELDS}


def rows_of(pkg, pr, st, P, res, rng, offset, tol, max_depth=MAX_DEPTH, max_windows=MAX_WINDOWS, owned=None, pairs=None, traces=None):
    return Ref(pkg, pr, st, P, res).rows(rng, offset, tol, max_depth, max_windows, owned, pairs, traces)


# ---- the truth: the flown curves themselves -------------------------------------------------------------------------------------------------------

def segment_samples(pkg, st, P, res, u, m):
    """[S][m][3] in np.longdouble: robot u's flown curve at m equally spaced parameters of every segment (ends included), from `convert`"""
    S = P * res
    sig = ((np.arange(S, dtype=LD)[:, None] + np.linspace(LD(0), LD(1), m, dtype=LD)[None, :]) / LD(res)).ravel()
    return T.curve_at(pkg, st["spline"][u], 1.0, P, res, sig).reshape(S, m, 3)


def sampled_minimum(pkg, ref, st, P, res, u, q, rng, m=21):
    """the smallest distance over m x m samples (>= 400) of every segment pair that passes the box test at rng: an upper bound of the true minimum of
    those segment pairs; inf without one"""
    tr, j = ref.seeds(u, q, rng)
    if len(tr) == 0:
        return math.inf
    a, b = segment_samples(pkg, st, P, res, u, m), segment_samples(pkg, st, P, res, q, m)
    best = math.inf
    for c0 in range(0, len(tr), 64):
        d = a[tr[c0:c0 + 64]][:, :, None, :] - b[j[c0:c0 + 64]][:, None, :, :]
        best = min(best, float(np.sqrt((d * d).sum(axis=-1)).min()))
    return best


def point_at(pkg, st, P, res, u, seg, s):
    """the flown curve's point at parameter s of segment seg, by de Casteljau on the piece's Bezier points in np.longdouble"""
    return T.curve_at(pkg, st["spline"][u], 1.0, P, res, np.array([(LD(seg) + LD(s)) / LD(res)], dtype=LD))[0]


def slack(S, st):
    return T.slack(S, np.concatenate([np.abs(np.asarray(st["spline"])).ravel(), [1.0]]))


# ---- constructed states ---------------------------------------------------------------------------------------------------------------------------

def lines_state(pkg, scenes, lines, P=4):
    """robot r flies the straight line lines[r] = (start, end, piece_time) at constant speed: collinear, equally spaced control points"""
    return T.straight_state(pkg, scenes, lines, P)


def x_state(pkg, scenes, z=0.0, pts=(1.0, 2.0)):
    """one net along x (y = 0, z = 0), the other along y at x = 0.3 and height z: the paths cross at (0.3, 0, .) -- no dyadic parameter of either --, z apart"""
    return lines_state(pkg, scenes, [((-5, 0, 0), (5, 0, 0), pts[0]), ((0.3, -5, z), (0.3, 5, z), pts[1])])


def goal_on_path_state(pkg, scenes):
    """the second net ENDS on the first path: robot 1 flies y = -5 -> 0 at x = 0.3 and stays there"""
    return lines_state(pkg, scenes, [((-5, 0, 0), (5, 0, 0), 1.0), ((0.3, -5, 0), (0.3, 0, 0), 2.0)])


def arcs_state(pkg, scenes, radius=3.0, gap=0.2, P=4):
    """a VALLEY instead of a point, hence a wide live set: two concentric quarter circles in the plane z = 0, `gap` apart (the spline space's least-squares
    fit of each arc: the radial error is asserted below 1e-6).  Every point of one path is `gap` from the other, to that error, so no item along the
    diagonal of the two parameters can be dropped against another until its hulls' sagittas fall below the fit's error: the live set about doubles per
    round.  (Two straight parallel nets would not do: their hulls are segments, lo == hi at the seeds and the live set is empty at depth 0.)"""
    scene = dict(scenes.hard(U=2, n_points=500, pieces=P))
    st = R.port_state(scene, 0)
    conv = pkg.host_tables(P, 8)[0]
    s = np.linspace(0.0, 1.0, 41)
    bern = np.stack([math.comb(5, k) * s ** k * (1 - s) ** (5 - k) for k in range(6)], axis=1)      # [41][6]
    A = np.zeros((P * len(s), 3 * P + 3))
    for i in range(P):
        A[i * len(s):(i + 1) * len(s), 3 * i:3 * i + 6] = bern @ conv[i]
    ang = (0.5 * math.pi / P) * (np.arange(P)[:, None] + s[None, :]).ravel()
    for r, rad in enumerate((radius, radius + gap)):
        target = rad * np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=1)
        net = np.linalg.lstsq(A, target, rcond=None)[0]                                              # [T][3]
        assert np.abs(np.sqrt(((A @ net) ** 2).sum(axis=1)) - rad).max() < 1e-6
        st["spline"][r] = net.T
    st["piece_time"][:] = (1.0, 1.5)
    assert R.valid_state(st, 2)
    return scene, st


def flattened(st):
    out = {k: np.array(v) for k, v in st.items()}
    out["spline"][:, 2, :] = 0.0
    return out


# ---- the defaults, measured -----------------------------------------------------------------------------------------------------------------------

STATES = (("e2e_scn_b", False), ("e2e_scn_c3", False), ("e2e_scn_b_coupled", False), ("e2e_scn_c3", True))


def default_tolerance(pkg, pr, names=STATES, rng=0.1 + 2 * 0.1, offset=0.1):
    """(widths per depth 0..40 over all listed pairs, the same over the rows not in contact, tolerance, largest live set of any pair at any depth,
    frontier, per state (listed pairs, rows in contact, largest live set)): tol = 0, max_depth = 40, the live set capped at MAX_WINDOWS only, at the default
    range on the named end states (True: z set to 0).  A pair whose search has ended keeps its last bracket.  The tolerance is the smallest power of ten
    >= 10 x the last positive width of the rows that are not in contact; the frontier the next power of two >= 4 x the largest live set, at least 64."""
    widths, clear_widths, widest, per = [0.0] * (MAX_DEPTH + 1), [0.0] * (MAX_DEPTH + 1), 0, {}
    for name, flat in names:
        st, P, res = T.e2e_state(name)
        if flat:
            st = flattened(st)
        traces = {}
        rows = rows_of(pkg, pr, st, P, res, rng, offset, 0.0, MAX_DEPTH, MAX_WINDOWS, traces=traces)
        big = 0
        for k, key in enumerate(zip(rows["robot"].tolist(), rows["partner"].tolist())):
            tr = [t for t in traces[key] if t[1] is not None]
            big = max(big, max(t[3] for t in traces[key]))
            for d in range(MAX_DEPTH + 1):
                _, lo, hi, _ = tr[min(d, len(tr) - 1)]
                widths[d] = max(widths[d], hi - lo)
                if not rows["flags"][k] & CONTACT:
                    clear_widths[d] = max(clear_widths[d], hi - lo)
        per[name + ("_flat" if flat else "")] = (len(rows["robot"]), int(np.sum(rows["flags"] & CONTACT != 0)), big)
        widest = max(widest, big)
    last = [w for w in clear_widths if w > 0.0][-1]
    tol = float("1e%d" % math.ceil(math.log10(10 * last)))
    frontier = max(64, 1 << max(0, math.ceil(math.log2(4 * max(widest, 1)))))
    return widths, clear_widths, tol, widest, frontier, per
