"""Reference values for tj_audit_timed that share no code with csrc/kernels_audit_timed.h (plain module: no fixtures, no tests).

  timed_rows, timed_records   the numpy restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_audit_timed.py: hulls by
                      audit_ref.hulls_of (hull_entry's sums), the windows enumerated in Python floats with every association written out, both nets restricted
                      by blossoming (bez_restrict: de Casteljau steps ub * x + sb * y, elementwise numpy = the same IEEE operations), the lower bound through
                      the ORACLE's GJK (oracle.pyoracle.Prims via audit_ref.FastGjk) of the six difference points against the origin.
  truth               nothing of GJK or subdivision in it: both flown curves evaluated from `convert` in np.longdouble on a dense time grid, minimum distance.
  constructed states  chase, crossing, hover: each builder asserts its precondition on the CPU with the truth function.

SLACK.  The bracket statements hold in exact arithmetic; in floating point they are tested up to slack = K(S) * eps * max|coordinate|, with K COUNTED, not tuned:
  hull formation     6 products + 6 sums per coordinate (hull_entry; the table's rows are convex weights)                    12 per curve ->  24
  restriction        5 de Casteljau levels, each a product pair and a sum, plus the shared 1 - s: 4 roundings per level       20 per curve ->  40
  difference         d_i = a_i - b_i                                                                                                          1
  window parameters  ca, cb, T0, Tj carry <= 2 roundings each relative to a time <= (S + 1) segment lengths, their difference and the
                     quotient one more each: |ds| <= 4 (S + 1) eps per parameter; a Bezier point moves by at most 5 * (largest control-point
                     step) <= 10 max|coordinate| per unit of parameter; 2 parameters x 2 curves                            -> 160 (S + 1)
  K(S) = 65 + 160 (S + 1).  (The GJK's own |v| is at rounding level for a point body outside the hull -- 1.2e-16, tests/test_audit_ref.py GJK_WORST_SEEN -- far
  inside this; for an origin INSIDE the difference hull it stops at up to ~1e-5 instead of 0: a stated limit of timed_lo)"""
import math

import numpy as np

import audit_ref as R

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def slack_k(S):
    return 65 + 160 * (S + 1)


def slack(S, coords):
    return slack_k(S) * EPS * float(np.max(np.abs(coords)))


def bez_restrict(p, sa, sb):
    """p [n][6][3], sa / sb [n] -> the Bezier nets over [sa, sb]: o[i] = blossom(sa x (5 - i), sb x i).  Row s of the triangle (s steps at sa) has 6 - s
    points; 5 - s steps at sb take it to o[5 - s].  Every step is (1 - s) * x + s * y, left to right."""
    sa = np.asarray(sa, dtype=np.float64)[:, None]; sb = np.asarray(sb, dtype=np.float64)[:, None]
    ua, ub = 1 - sa, 1 - sb
    r = [p[:, m, :] for m in range(6)]
    o = [None] * 6
    for s in range(6):
        t = list(r[:6 - s])
        for k in range(5 - s, 0, -1):
            t = [ub * t[m] + sb * t[m + 1] for m in range(k)]
        o[5 - s] = t[0]
        if s < 5:
            r = [ua * r[m] + sa * r[m + 1] for m in range(5 - s)]
    return np.stack(o, axis=1)


def clamp01(x):
    return min(max(x, 0.0), 1.0)


def pieces_of(pt, P, res, u, tr, q, L):
    """the windows of (u, tr) against partner q at level L, in the order (sub-window, cut): tuples (w, j, ca, cb, sa, sb, ra, rb); j == S: q hovers"""
    S, N, rf = P * res, 1 << L, float(res)
    ptu, ptq = float(pt[u]), float(pt[q])
    T0u, T1u = (tr / rf) * ptu, ((tr + 1) / rf) * ptu
    lenu = T1u - T0u
    out = []
    for w in range(N):
        t0, t1 = ((tr + w / float(N)) / rf) * ptu, ((tr + (w + 1) / float(N)) / rf) * ptu
        g = math.floor((t0 / ptq) * rf)
        j = S if g >= S else (int(g) if g > 0 else 0)
        while j > 0 and (j / rf) * ptq > t0:
            j -= 1
        while j < S and ((j + 1) / rf) * ptq <= t0:
            j += 1
        while True:
            hover = j >= S
            Tj, Tj1 = (j / rf) * ptq, ((j + 1) / rf) * ptq
            ca, cb = max(t0, Tj), (t1 if hover else min(t1, Tj1))
            lenq = Tj1 - Tj
            out.append((w, j, ca, cb, clamp01((ca - T0u) / lenu), clamp01((cb - T0u) / lenu), clamp01((ca - Tj) / lenq), clamp01((cb - Tj) / lenq)))
            j += 1
            if not (j <= S and (j / rf) * ptq < t1):
                break
    return out


def timed_rows(pkg, pr, spline, pt, P, res, rng, L, owned=None, prefilter=True):
    """per (robot, segment): dict of lo, qlo, hi, qhi, time [U][S] (rng / -1 / -1.0 where nothing is closer than rng).  prefilter=False evaluates every
    window (the kernel skips those whose raw hull boxes are further apart than rng: the two agree, which is its exactness argument)."""
    spline = np.asarray(spline, dtype=np.float64); pt = np.asarray(pt, dtype=np.float64)
    U, S = spline.shape[0], P * res
    H = R.hulls_of(pkg, spline, P, res)                               # [U][S][6][3]
    HX = np.concatenate([H, np.repeat(H[:, S - 1:S, 5:6, :], 6, axis=2)], axis=1)   # [U][S + 1][6][3]: row S = the hover body, six times the last control point
    blo, bhi = HX.min(axis=2), HX.max(axis=2)                         # [U][S + 1][3]
    rf = float(res)
    Tj = (np.arange(S + 2) / rf)[None, :] * pt[:, None]              # [U][S + 2] segment boundaries in time
    Tj[:, S + 1] = np.inf
    guard = rng * 1.000001 + 1e-9
    meta, A, B, SA, SB, RA, RB, HOV = [], [], [], [], [], [], [], []
    for u in (range(U) if owned is None else owned):
        for tr in range(S):
            gap = np.maximum(blo - bhi[u, tr], blo[u, tr] - bhi)      # [U][S + 1][3]
            near = ~(gap > guard).any(axis=2) if prefilter else np.ones((U, S + 1), dtype=bool)
            T0u, T1u = Tj[u, tr], Tj[u, tr + 1]
            cand = near & (Tj[:, :S + 1] <= T1u) & (Tj[:, 1:] >= T0u)
            cand[u] = False
            for q in np.flatnonzero(cand.any(axis=1)):
                for (w, j, ca, cb, sa, sb, ra, rb) in pieces_of(pt, P, res, u, tr, int(q), L):
                    if not near[q, j]:
                        continue
                    meta.append((u, tr, int(q), w, ca, cb))
                    A.append(H[u, tr]); B.append(HX[q, j]); SA.append(sa); SB.append(sb); RA.append(ra); RB.append(rb); HOV.append(j >= S)
    out = dict(lo=np.full((U, S), float(rng)), hi=np.full((U, S), float(rng)), time=np.full((U, S), -1.0),
               qlo=np.full((U, S), -1, dtype=np.int64), qhi=np.full((U, S), -1, dtype=np.int64))
    if not meta:
        return out
    A, B = np.array(A), np.array(B)
    ra_ = bez_restrict(A, SA, SB)
    rb_ = np.where(np.array(HOV)[:, None, None], B, bez_restrict(B, RA, RB))   # a hover body is not restricted: six equal points stay bit-equal
    Dn = np.ascontiguousarray(ra_ - rb_)                               # [n][6][3]
    d0, d5 = Dn[:, 0], Dn[:, 5]
    h0 = np.sqrt((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2])
    h5 = np.sqrt((d5[:, 0] * d5[:, 0] + d5[:, 1] * d5[:, 1]) + d5[:, 2] * d5[:, 2])
    g = R.FastGjk(pr)
    origin = np.zeros(3)
    base, oa = Dn.ctypes.data, origin.ctypes.data
    for n, (u, tr, q, w, ca, cb) in enumerate(meta):   # ascending (u, tr, q, w, cut): strict comparisons keep the first
        lo = g.dist(6, base + n * 144, 1, oa)
        first = h0[n] <= h5[n]
        hi = float(h0[n] if first else h5[n])
        if lo < rng and lo < out["lo"][u, tr]:
            out["lo"][u, tr], out["qlo"][u, tr] = lo, q
        if hi < rng and hi < out["hi"][u, tr]:
            out["hi"][u, tr], out["qhi"][u, tr], out["time"][u, tr] = hi, q, (ca if first else cb)
    return out


def timed_records(rows, rng, offset, L, multi=True, owned=None):
    """per robot the record's fields, in tj_audit_timed_robot's names; equal values keep the smallest segment"""
    U, S = rows["lo"].shape
    names = ("timed_lo", "timed_hi", "timed_time", "timed_robot", "timed_segment", "lo_robot", "lo_segment", "levels", "flags")
    out = {n: np.zeros(U, dtype=np.float64 if n in names[:3] else np.int32) for n in names}
    for u in (range(U) if owned is None else owned):
        lo, slo, qlo, hi, shi, qhi, th = rng, -1, -1, rng, -1, -1, -1.0
        for tr in range(S):
            if rows["qlo"][u, tr] >= 0 and rows["lo"][u, tr] < lo:
                lo, slo, qlo = rows["lo"][u, tr], tr, int(rows["qlo"][u, tr])
            if rows["qhi"][u, tr] >= 0 and rows["hi"][u, tr] < hi:
                hi, shi, qhi, th = rows["hi"][u, tr], tr, int(rows["qhi"][u, tr]), rows["time"][u, tr]
        flags = 2 if not multi else ((1 if qhi >= 0 and hi <= offset else 0) | (2 if lo > offset else 0))
        for n, v in zip(names, (lo, hi, th, qhi, shi, qlo, slo, L, flags)):
            out[n][u] = v
    return out


def restated(pkg, pr, st, P, res, rng, offset, L, owned=None, prefilter=True):
    """(records, rows) of a multi-UAV state"""
    rows = timed_rows(pkg, pr, st["spline"], st["piece_time"], P, res, rng, L, owned, prefilter)
    if owned is not None:   # rows of other ranks read 0
        mask = np.ones(rows["lo"].shape[0], dtype=bool); mask[list(owned)] = False
        rows["lo"][mask] = 0.0; rows["hi"][mask] = 0.0
    return timed_records(rows, rng, offset, L, True, owned), rows


# ---- the truth: the flown curves themselves -----------------------------------------------------------------------------------------------------

def curve_at(pkg, spline_u, pt_u, P, res, t):
    """positions [n][3] in np.longdouble of one robot at real times t [n]: piece i is the quintic Bezier curve over convert[i] @ net[3i : 3i + 6] in the
    piece parameter; sigma = t / piece_time, held at P after the arrival (log_data's conventions)"""
    conv = pkg.host_tables(P, res)[0]
    net = np.asarray(spline_u, dtype=LD).T                                        # [T][3]
    sig = np.minimum(np.asarray(t, dtype=LD) / LD(pt_u), LD(P))
    i = np.minimum(np.floor(sig).astype(np.int64), P - 1)
    s = sig - i
    Bz = np.stack([np.asarray(conv[k], dtype=LD) @ net[3 * k:3 * k + 6] for k in range(P)])   # [P][6][3]
    out = np.zeros((len(sig), 3), dtype=LD)
    for k in range(6):
        out += (LD(math.comb(5, k)) * s ** k * (1 - s) ** (5 - k))[:, None] * Bz[i, k]
    return out


def truth(pkg, st, P, res, n=4001):
    """per robot u: (minimum over q != u and n times per SEGMENT-FREE dense grid of [0, P * piece_time_u] of |p_u(t) - p_q(t)|, q, t) -- an upper bound of
    the true minimum separation over u's flight that converges to it from above"""
    U = st["spline"].shape[0]
    out = []
    for u in range(U):
        t = np.linspace(LD(0), LD(P) * LD(st["piece_time"][u]), n, dtype=LD)
        pu = curve_at(pkg, st["spline"][u], st["piece_time"][u], P, res, t)
        best = (np.inf, -1, -1.0)
        for q in range(U):
            if q == u:
                continue
            d = pu - curve_at(pkg, st["spline"][q], st["piece_time"][q], P, res, t)
            dist = np.sqrt((d * d).sum(axis=1))
            k = int(np.argmin(dist))
            if float(dist[k]) < best[0]:
                best = (float(dist[k]), q, float(t[k]))
        out.append(best)
    return out


def separation_at(pkg, st, P, res, u, q, t):
    t = np.array([t], dtype=LD)
    d = curve_at(pkg, st["spline"][u], st["piece_time"][u], P, res, t) - curve_at(pkg, st["spline"][q], st["piece_time"][q], P, res, t)
    return float(np.sqrt((d * d).sum()))


# ---- states ---------------------------------------------------------------------------------------------------------------------------------------

def e2e_state(name):
    """final state of a committed end-to-end fixture: dict(spline, piece_time) and (P, res)"""
    from conftest import gold
    g = gold(name + ".npz")
    return dict(spline=np.array(g["final_spline"]), piece_time=np.array(g["final_piece_time"])), g["final_spline"].shape[2] // 3 - 1, 8


def linear_nets(pkg, P, res):
    """(one[T], sig[T]): control-net coefficient vectors whose curves are the constant 1 and the piece parameter sigma itself (least squares on the Bezier
    points convert[i] @ net[3i : 3i + 6] = 1 and = i + k / 5; the spline space holds both, the residual is asserted)"""
    conv = pkg.host_tables(P, res)[0]
    T = 3 * P + 3
    M = np.zeros((6 * P, T)); one, sig = np.ones(6 * P), np.zeros(6 * P)
    for i in range(P):
        M[6 * i:6 * i + 6, 3 * i:3 * i + 6] = conv[i]
        sig[6 * i:6 * i + 6] = i + np.arange(6) / 5.0
    g1, gs = np.linalg.lstsq(M, one, rcond=None)[0], np.linalg.lstsq(M, sig, rcond=None)[0]
    assert np.abs(M @ g1 - one).max() < 1e-12 and np.abs(M @ gs - sig).max() < 1e-12
    return g1, gs


def straight_state(pkg, scenes, lines, P=4):
    """a two-robot state (hard()'s scene with `P` pieces: obstacles play no part) in which robot r flies the straight line lines[r] = (start[3], end[3],
    piece_time) at constant speed: position = start + (end - start) * sigma / P.  Returns (scene, state)."""
    scene = dict(scenes.hard(U=len(lines), n_points=500, pieces=P))
    st = R.port_state(scene, 0)
    g1, gs = linear_nets(pkg, P, 8)
    for r, (a, b, pt) in enumerate(lines):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        st["spline"][r] = a[:, None] * g1[None, :] + ((b - a) / P)[:, None] * gs[None, :]
        st["piece_time"][r] = pt
    assert R.valid_state(st, len(lines))
    return scene, st


def chase_state(pkg, scenes):
    """(a) same-lane chase: robot 0 flies x = 0 -> 10 in 4 * 1.0, robot 1 x = 2 -> 12 in 4 * 2.0 on the same line.  Same-segment hulls are >= 1.6875 apart
    (> offset + 2 * margin: tj_audit sees no pair), yet the two meet at t = 0.4 * duration_0 = 1.6 (x = 4).  A robot that starts ahead, takes twice as long and keeps its
    same-segment hulls clear of the other's necessarily ends beyond the other's goal: robot 1 also flies through x = 10 at t = 6.4, where robot 0 has been hovering since
    t = 4 -- a second contact, in robot 1's record only (robot 0's own flight is over).  Both asserted here with the truth function.  Returns (scene, state, 1.6, 6.4)."""
    scene, st = straight_state(pkg, scenes, [((0, 0, 0), (10, 0, 0), 1.0), ((2, 0, 0), (12, 0, 0), 2.0)])
    t_meet = 0.4 * 4 * 1.0
    t_goal = 0.8 * 4 * 2.0
    assert separation_at(pkg, st, 4, 8, 0, 1, t_meet) < 1e-12 and separation_at(pkg, st, 4, 8, 1, 0, t_goal) < 1e-12
    H = R.hulls_of(pkg, st["spline"], 4, 8)
    d, _ = R.all_pair(R.prims(), H)
    assert d.min() > 0.1 + 2 * 0.1 and abs(d.min() - 1.6875) < 1e-9
    return scene, st, t_meet, t_goal


def crossing_state(pkg, scenes):
    """(b) timing that makes it safe: robot 0 flies x = -5 -> 5 (y = 0) in 4 * 1.0, robot 1 y = -5 -> 5 (x = 0) in 4 * 2.0.  The paths cross at the origin and
    the same-segment hulls of segment 15 both end there (tj_audit: pair contact), but robot 0 passes at t = 2 and robot 1 at t = 4: the closest approach
    is sqrt(5) at t = 2.4.  Asserted here."""
    scene, st = straight_state(pkg, scenes, [((-5, 0, 0), (5, 0, 0), 1.0), ((0, -5, 0), (0, 5, 0), 2.0)])
    tv = truth(pkg, st, 4, 8)
    assert abs(tv[0][0] - math.sqrt(5.0)) < 1e-6 and abs(tv[0][2] - 2.4) < 1e-2 and tv[1][0] >= tv[0][0] - 1e-6
    d, _ = R.all_pair(R.prims(), R.hulls_of(pkg, st["spline"], 4, 8))
    assert d[0, 15] <= 1e-12 and d[0, 15] <= 0.1
    return scene, st


def hover_state(pkg, scenes):
    """(c) hover: robot 0 flies x = -5 -> 0 in 4 * 0.5 = 2 and stays at the origin; robot 1 flies y = -4.5 -> 5.5 (x = 0) in 4 * 2.0 and is at the origin at
    t = 3.6 > 2 (sigma_1 = 1.8, inside its segment 14).  While BOTH fly they stay 2 or more apart.  Asserted here."""
    scene, st = straight_state(pkg, scenes, [((-5, 0, 0), (0, 0, 0), 0.5), ((0, -4.5, 0), (0, 5.5, 0), 2.0)])
    assert separation_at(pkg, st, 4, 8, 1, 0, 3.6) < 1e-12
    tv = truth(pkg, st, 4, 8)
    assert tv[0][0] > 1.99 and tv[1][0] < 2e-3 and abs(tv[1][2] - 3.6) < 1e-2   # robot 0's own flight ends at t = 2: its record never meets robot 1
    return scene, st, 3.6


def default_level_widths(pkg, pr, names=("e2e_scn_b", "e2e_scn_c3", "e2e_scn_b_coupled"), rng=0.1 + 2 * 0.1, offset=0.1):
    """per level 0..6 the largest timed_hi - timed_lo over the robots with a partner in range (timed_robot >= 0) of the named end states, and the
    smallest level at which it is < offset / 10"""
    widths = []
    for L in range(7):
        worst = 0.0
        for name in names:
            st, P, res = e2e_state(name)
            rec, _ = restated(pkg, pr, st, P, res, rng, offset, L)
            m = rec["timed_robot"] >= 0
            if m.any():
                worst = max(worst, float((rec["timed_hi"][m] - rec["timed_lo"][m]).max()))
        widths.append(worst)
    return widths, next(L for L, w in enumerate(widths) if w < offset / 10)
