"""Reference values for tj_flight_profile that share no code with csrc/kernels_flight_profile.h (plain module: no fixtures, no tests).

  profile             the numpy restatement of include/trajadmm.h's definition, compared with == by tests/test_gpu_flight_profile.py.  Hulls by
                      audit_ref.hulls_of (hull_entry's sums); the segment of a time by audit_timed_ref's rule (pieces_of's first lines); the position by
                      audit_timed_ref.bez_restrict of the raw hull to [s, s] (its b_0: five steps (1 - s) * x + s * y); speed and acceleration from
                      tj_audit's nets (audit_ref.limit_terms' expressions) evaluated at s by the same step; the nearest primitive by BRUTE FORCE over every
                      primitive (a point: audit_ref.norm3's association; a triangle: the ORACLE's GJK of the one-point body against it, as
                      obstacle_approach_ref's hi), the smallest index among equal values; the nearest robot by brute force over every q != u.  No tree.
  slack_pos / _speed / _accel   the rounding slack of the restatement against the flown curve, COUNTED in the manner of audit_timed_ref.slack (below).
  sphere_cloud, twin_cloud      constructed obstacle sets (equal distances, exact ties).

SLACK, in units of eps * M, M = max |control-point coordinate| (the tables are exact for res = 2^k: dyadic rationals, host_tables.h):
  position   hull formation 12 (6 products + 6 sums, convex weights) + de Casteljau 5 levels x 4 roundings = 20 + the parameter: t, T(j), T(j + 1) carry <= 2
             roundings each relative to a time of <= S + 1 segment lengths, the difference and the quotient one more each: |ds| <= 4 (S + 1) eps, and the
             point moves by <= 5 x (largest hull step <= 2 M) = 10 M per unit of s: 40 (S + 1).                         K_pos = 32 + 40 (S + 1)
  speed      v_i = 5 (P[i+1] - P[i]), |v_i| <= 10 M: inputs 2 x 12, the difference's rounding 2, x 5, the product's rounding 10 -> 140; de Casteljau 4 levels
             x 4 roundings of <= 10 M = 160; the parameter: |dv/ds| <= 4 x 20 M, x 4 (S + 1) -> 320 (S + 1); per component, so x sqrt(3) < 2 for the norm;
             norm3 itself 3 roundings of sqrt(3) x 10 M -> 52.                                                           K_v = 652 + 640 (S + 1)
             speed = |v| / (w pt): three more roundings relative to the speed itself.
  accel      a_i = 20 (P[i+2] - 2 P[i+1] + P[i]), |a_i| <= 80 M: inputs 4 x 12, two roundings of <= 3 M and 4 M, x 20, the product's rounding 80 -> 1180;
             de Casteljau 3 levels x 4 x 80 = 960; the parameter: |da/ds| <= 3 x 160 M, x 4 (S + 1) -> 1920 (S + 1); x 2 for the norm; norm3 3 x sqrt(3) x
             80 -> 416.                                                                                                   K_a = 4696 + 3840 (S + 1)
             accel = |a| / (w w pt pt): five more roundings relative to the acceleration itself."""
import numpy as np

import audit_ref as R
import audit_timed_ref as T

EPS = float(np.finfo(np.float64).eps)
HOVER, OBS_CONTACT, PAIR_CONTACT, SPEED, ACCEL = 1, 2, 4, 8, 16
FLOATS = ("time", "x", "y", "z", "obs_distance", "robot_distance", "speed", "accel")
INTS = ("obs_index", "robot", "segment", "flags")
FIELDS = FLOATS + INTS


def prims_of(scene):
    """the obstacle primitives in the caller's order: [N][3] points or [N][3][3] triangles"""
    return np.ascontiguousarray(scene["tris"] if scene.get("tris") is not None else scene["cloud"], dtype=np.float64)


def segment_of(t, pt, res, S):
    """the segment j with T(j) <= t < T(j + 1), T(j) = (j / res) * pt in these very expressions (the quotient only proposes); S: arrived"""
    rf = float(res)
    g = np.floor((t / pt) * rf)
    j = S if g >= S else (int(g) if g > 0 else 0)
    while j > 0 and (j / rf) * pt > t:
        j -= 1
    while j < S and ((j + 1) / rf) * pt <= t:
        j += 1
    return j


def _casteljau(net, s):
    """net [n][m][3], s [n] -> [n][3]: m - 1 steps (1 - s) * x + s * y"""
    s = np.asarray(s, dtype=np.float64)[:, None]
    us = 1 - s
    r = [net[:, i, :] for i in range(net.shape[1])]
    while len(r) > 1:
        r = [us * r[i] + s * r[i + 1] for i in range(len(r) - 1)]
    return r[0]


def _norm3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def points(pkg, st, P, res, times):
    """(pos [U][K][3], speed [U][K], accel [U][K], segment [U][K]) of every robot at every time"""
    spline, pt = np.asarray(st["spline"], dtype=np.float64), np.asarray(st["piece_time"], dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    U, S, K, rf = spline.shape[0], P * res, len(times), float(res)
    H = R.hulls_of(pkg, spline, P, res)
    pos, speed, accel = np.zeros((U, K, 3)), np.zeros((U, K)), np.zeros((U, K))
    seg = np.zeros((U, K), dtype=np.int64)
    fly, nets, ss = [], [], []
    for u in range(U):
        ptu = float(pt[u])
        for k in range(K):
            t = float(times[k])
            j = segment_of(t, ptu, res, S)
            seg[u, k] = j
            if j == S:
                pos[u, k] = H[u, S - 1, 5]
                continue
            Tj, Tj1 = (j / rf) * ptu, ((j + 1) / rf) * ptu
            fly.append((u, k, j)); nets.append(H[u, j]); ss.append(T.clamp01((t - Tj) / (Tj1 - Tj)))
    if fly:
        Pn, s = np.array(nets), np.array(ss)
        b0 = T.bez_restrict(Pn, s, s)[:, 0]                                                      # [n][3]
        v = _casteljau(5 * (Pn[:, 1:] - Pn[:, :-1]), s)
        a = _casteljau(20 * (Pn[:, 2:] - 2 * Pn[:, 1:-1] + Pn[:, :-2]), s)
        nv, na = _norm3(v), _norm3(a)
        for n, (u, k, j) in enumerate(fly):
            kk = j % res
            w = (kk + 1) / float(res) - kk / float(res)                                           # the table value (seg_weight), not 1 / res
            ptu = float(pt[u])
            pos[u, k] = b0[n]
            speed[u, k] = float(nv[n]) / (w * ptu)
            accel[u, k] = float(na[n]) / (w * w * ptu * ptu)
    return pos, speed, accel, seg


def nearest_primitive(pr, X, p):
    """(distance, index) of the primitive of X nearest to the point p: every primitive, the smallest index among equal values; (inf, -1) for none"""
    if X.shape[0] == 0:
        return np.inf, -1
    if X.ndim == 2:
        d = _norm3(p[None, :] - X)
    else:
        g = R.FastGjk(pr)
        pp = np.ascontiguousarray(p, dtype=np.float64)
        pa, xb = pp.ctypes.data, X.ctypes.data
        d = np.array([g.dist(1, pa, 3, xb + i * 72) for i in range(X.shape[0])])
    i = int(np.argmin(d))                                                                         # (the first of equal values)
    return float(d[i]), i


def profile(pkg, pr, st, P, res, X, times, params, multi=True, owned=None):
    """the records as a dict of arrays [U][K] in tj_profile_sample's names (rows of robots outside `owned`: zero)"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64)
    pos, speed, accel, seg = points(pkg, st, P, res, times)
    U, K, S = pos.shape[0], pos.shape[1], P * res
    out = {n: np.zeros((U, K), dtype=np.float64 if n in FLOATS else np.int32) for n in FIELDS}
    for u in (range(U) if owned is None else owned):
        for k in range(K):
            od, oi = nearest_primitive(pr, X, pos[u, k])
            pd, pq = np.inf, -1
            if multi:
                for q in range(U):
                    if q != u:
                        d = R.norm3(pos[u, k] - pos[q, k])
                        if d < pd:
                            pd, pq = d, q
            flags = ((HOVER if seg[u, k] == S else 0) | (OBS_CONTACT if oi >= 0 and od <= params["offset"] else 0) |
                     (PAIR_CONTACT if pq >= 0 and pd <= params["offset"] else 0) | (SPEED if speed[u, k] >= params["vel_limit"] else 0) |
                     (ACCEL if accel[u, k] >= params["acc_limit"] else 0))
            for n, v in zip(FIELDS, (times[k], pos[u, k, 0], pos[u, k, 1], pos[u, k, 2], od, pd, speed[u, k], accel[u, k], oi, pq, seg[u, k], flags)):
                out[n][u, k] = v
    return out


def durations(st, P):
    """log_data's sum per robot: piece_num times 1.0 * piece_time"""
    out = []
    for pt in np.asarray(st["piece_time"], dtype=np.float64):
        d = 0.0
        for _ in range(P):
            d += 1.0 * float(pt)
        out.append(d)
    return np.array(out)


def grid(st, P, K):
    """Solver.flight_profile's default grid, restated: t_k = (k / (K - 1)) * the longest duration"""
    longest = float(durations(st, P).max())
    return np.array([(k / (K - 1)) * longest if K > 1 else 0.0 for k in range(K)])


def sample_times(st, P, res, K):
    """K times that include 0, segment boundaries of robot 0 (every one where K allows), the longest duration and 1.5 times it (all robots hover)"""
    pt0, S, rf = float(st["piece_time"][0]), P * res, float(res)
    longest = float(durations(st, P).max())
    must = [0.0, 1.5 * longest, longest] + [(j / rf) * pt0 for j in range(1, S + 1)]
    fill = list(np.random.default_rng(K).uniform(0.0, 1.2 * longest, K))
    return np.array((must + fill)[:K] if K < len(must) else must + fill[:K - len(must)])


# ---- slack against the flown curve (the module's docstring) ---------------------------------------------------------------------------------------

def slack_pos(S, M):
    return (32 + 40 * (S + 1)) * EPS * M


def slack_speed(S, M, w, pt, speed):
    return (652 + 640 * (S + 1)) * EPS * M / (w * pt) + 3 * EPS * speed


def slack_accel(S, M, w, pt, accel):
    return (4696 + 3840 * (S + 1)) * EPS * M / (w * w * pt * pt) + 5 * EPS * accel


# ---- constructed obstacle sets ----------------------------------------------------------------------------------------------------------------------

def sphere_cloud(centre, n=4096, radius=2.0, seed=5):
    """n points on a sphere around `centre`: all at (nearly) equal distance, so no bound can prune them apart"""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.ascontiguousarray(np.asarray(centre, dtype=np.float64)[None, :] + radius * v)


def twin_cloud(cloud, centre, i, j):
    """`cloud` with points i and j at centre +- (0.5, 0, 0): with a centre whose x is a multiple of 2^-40 below 2^10 both differences are exact, the distances
    bit-equal (asserted), and nothing else is nearer (asserted)"""
    c = np.asarray(centre, dtype=np.float64)
    out = np.array(cloud, dtype=np.float64)
    out[i] = c + np.array([0.5, 0.0, 0.0]); out[j] = c - np.array([0.5, 0.0, 0.0])
    d = _norm3(c[None, :] - out)
    assert d[i] == d[j] == 0.5 and np.sum(d <= 0.5) == 2, (d[i], d[j], np.sum(d <= 0.5))
    return np.ascontiguousarray(out)
