"""Reference values for tj_audit that share no code and no shortcut with csrc/kernels_audit.h (plain module: no fixtures, no tests).

  hulls_of, brute_obs, brute_pair, robot_min, limits_of   the numpy restatement tests/test_gpu_audit.py compares with ==.  brute_obs has two forms: the
                      prefiltered one (the device's box comparison, for large clouds) and the unfiltered one (every primitive against every hull);
                      tests/test_audit_ref.py shows on the CPU that they agree, which is the kernel's exactness argument.
  exact_distance      the Euclidean distance of two small convex hulls by enumeration of vertex subsets in np.longdouble -- nothing of GJK in it.
  curve_derivatives   velocity / acceleration of the flown curve from the Bezier points of `convert` (not the `basis` table hull_entry uses).
  constructed inputs  (contact, ties, threshold states): each builder asserts its own precondition on the CPU, so a GPU failure is not a mis-built input."""
import ctypes as C
from itertools import combinations
from math import comb

import numpy as np

LD = np.longdouble


def engines():
    """the CPU engines present: the port always, the reference's own code where oracle/_ref was built"""
    from oracle.pyoracle import available
    return ["port"] + (["ref"] if available("ref") else [])


def prims(params=None, kind=None):
    from oracle.pyoracle import Prims
    return Prims(kind or engines()[-1], params)


def norm3(v):
    """dev_common.h norm3: sqrt(x*x + y*y + z*z), left to right"""
    return float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def hulls_of(pkg, spline, P, res):
    """[U][S][6][3]: hull_entry's sum -- acc = 0, acc += basis[tr][j][k] * net[3 * piece + k][a] for k = 0..5"""
    basis = pkg.host_tables(P, res)[2]
    U, S = spline.shape[0], P * res
    H = np.zeros((U, S, 6, 3))
    for tr in range(S):
        sp = tr // res
        for k in range(6):
            H[:, tr] += basis[tr][None, :, k, None] * spline[:, None, :, 3 * sp + k]
    return H


class FastGjk:
    """Prims.gjk without the per-call array handling: bodies are rows of C-contiguous float64 arrays, addressed by pointer arithmetic"""

    def __init__(self, pr):
        self.f = getattr(pr.lib, pr.px + "gjk")
        self.f.restype = None
        self.f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.v = np.zeros(3)
        self.va = self.v.ctypes.data

    def dist(self, n1, a1, n2, a2):
        self.f(n1, a1, n2, a2, self.va)
        v = self.v
        return float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def all_obs(pr, H, prims_xyz):
    """unfiltered: (min |v| over ALL primitives, smallest index attaining it) per (robot, segment), no range"""
    H = np.ascontiguousarray(H, dtype=np.float64); X = np.ascontiguousarray(prims_xyz, dtype=np.float64)
    U, S = H.shape[:2]
    nv = 3 if X.ndim == 3 else 1
    g = FastGjk(pr)
    hb, xb, N = H.ctypes.data, X.ctypes.data, X.shape[0]
    d = np.full((U, S), np.inf); ids = np.full((U, S), -1, dtype=np.int64)
    for u in range(U):
        for tr in range(S):
            ha = hb + (u * S + tr) * 144
            best, bi = np.inf, -1
            for i in range(N):
                x = g.dist(6, ha, nv, xb + i * nv * 24)
                if x < best:
                    best, bi = x, i
            d[u, tr], ids[u, tr] = best, bi
    return d, ids


def cap(d, ids, rng):
    """min(range, minimum): nothing closer than `rng` -> (rng, -1)"""
    hit = d < rng
    return np.where(hit, d, rng), np.where(hit, ids, -1)


def brute_obs(pr, H, prims_xyz, rng, prefilter=True):
    """prims_xyz [N][3] points or [N][3][3] triangles -> (d[U][S], id[U][S]); id -1 and d = rng where nothing is closer.
    prefilter=True: only primitives whose point / box is within rng of the hull's box (the device's comparison, kernels_sep.h box_near);
    prefilter=False: every primitive against every hull."""
    prims_xyz = np.asarray(prims_xyz, dtype=np.float64)
    if not prefilter:
        return cap(*all_obs(pr, H, prims_xyz), rng)
    U, S = H.shape[:2]
    tri = prims_xyz.ndim == 3
    plo = prims_xyz.min(axis=1) if tri else prims_xyz
    phi = prims_xyz.max(axis=1) if tri else prims_xyz
    d = np.full((U, S), float(rng)); ids = np.full((U, S), -1, dtype=np.int64)
    for u in range(U):
        for tr in range(S):
            lo, hi = H[u, tr].min(axis=0), H[u, tr].max(axis=0)
            near = np.flatnonzero(~((phi + rng < lo) | (plo > hi + rng)).any(axis=1))
            for i in near:
                x = norm3(pr.gjk(H[u, tr], prims_xyz[i].reshape(-1, 3)))
                if x < rng and (x < d[u, tr] or (x == d[u, tr] and i < ids[u, tr])):
                    d[u, tr], ids[u, tr] = x, i
    return d, ids


def all_pair(pr, H):
    """unfiltered, no range: per (robot, segment) the smallest |v| to another robot's hull of the same segment and the smallest robot attaining it"""
    H = np.ascontiguousarray(H, dtype=np.float64)
    U, S = H.shape[:2]
    g = FastGjk(pr)
    hb = H.ctypes.data
    d = np.full((U, S), np.inf); ids = np.full((U, S), -1, dtype=np.int64)
    for tr in range(S):
        for a in range(U):   # plane_pair: the lower robot index is body 1
            aa = hb + (a * S + tr) * 144
            for b in range(a + 1, U):
                x = g.dist(6, aa, 6, hb + (b * S + tr) * 144)
                if x < d[a, tr]:
                    d[a, tr], ids[a, tr] = x, b       # (b ascends: a strict comparison keeps the smallest partner)
                if x < d[b, tr]:
                    d[b, tr], ids[b, tr] = x, a       # (a ascends, and every a < b comes before every partner > b of robot b)
    return d, ids


def brute_pair(pr, H, rng):
    return cap(*all_pair(pr, H), rng)


def robot_min(d, ids, rng):
    """(value, segment, index) per robot: smallest (segment, index) among equal distances"""
    out = []
    for u in range(d.shape[0]):
        best = (rng, -1, -1)
        for tr in range(d.shape[1]):
            if ids[u, tr] >= 0 and d[u, tr] < best[0]:
                best = (d[u, tr], tr, int(ids[u, tr]))
        out.append(best)
    return out


def limit_terms(pkg, st, P, res, u):
    """per segment the five speed terms [S][5] and the four acceleration terms [S][4] of robot u (Energy_admm.h:131-165 in the line search's association: dev_common.h hull_speed / hull_accel, shared by kernels_ls.h and kernels_audit.h)"""
    H = hulls_of(pkg, st["spline"][u:u + 1], P, res)[0]
    pt = st["piece_time"][u]
    sp, ac = np.zeros((P * res, 5)), np.zeros((P * res, 4))
    for tr in range(P * res):
        k = tr % res
        w = (k + 1) / float(res) - k / float(res)   # the table value (seg_weight), not 1 / res
        Pp = H[tr]
        for b in range(5):
            sp[tr, b] = norm3(5 * (Pp[b + 1] - Pp[b])) / (w * pt)
        for j in range(4):
            ac[tr, j] = norm3(20 * (Pp[j + 2] - 2 * Pp[j + 1] + Pp[j])) / (w * w * pt * pt)
    return sp, ac


def limits_of(pkg, st, P, res):
    """per robot (speed, segment, accel, segment, duration); maxima keep the smallest segment"""
    out = []
    for u in range(st["spline"].shape[0]):
        pt = st["piece_time"][u]
        sp, ac = limit_terms(pkg, st, P, res, u)
        ms, ma = sp.max(axis=1), ac.max(axis=1)
        dur = 0.0
        for _ in range(P):
            dur += 1.0 * pt
        out.append((float(ms.max()), int(np.argmax(ms)), float(ma.max()), int(np.argmax(ma)), dur))
    return out


# ---- the distance itself ----------------------------------------------------------------------------------------------------------------------

def _subsets(n, k):
    return np.array(list(combinations(range(n), k)), dtype=np.int64)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def exact_distance(A, B):
    """Euclidean distance between conv(A) and conv(B) (row lists of at most 6 points each, or 6 and 1 / 3), 0.0 where they meet.

    = the distance of the origin from conv{a_i - b_j}.  The nearest point of a polytope lies in the relative interior of a simplex spanned by at
    most 3 of its generating points, unless the origin is inside (then it is inside a tetrahedron of 4).  So: for every subset of 1, 2, 3 generating
    points the origin is projected onto the subset's affine hull (normal equations in np.longdouble, closed form); where all barycentric weights
    are >= 0 the POINT sum(w_i p_i) is formed and its norm kept -- such a point is in the hull whatever the solve's rounding was, so no candidate
    can be below the true distance by more than the rounding of that one sum, and the true face is among the candidates.  Every subset of 4 with a
    solid tetrahedron is tested for containing the origin.  (Near-degenerate subsets are skipped: a smaller subset covers them.)"""
    A = np.asarray(A, dtype=LD).reshape(-1, 3); B = np.asarray(B, dtype=LD).reshape(-1, 3)
    D = (A[:, None, :] - B[None, :, :]).reshape(-1, 3)
    n = D.shape[0]
    scale = max(LD(1e-300), np.abs(D).max())
    best = np.sqrt(_dot(D, D)).min()
    if n >= 2:
        idx = _subsets(n, 2)
        p0, e = D[idx[:, 0]], D[idx[:, 1]] - D[idx[:, 0]]
        ee = _dot(e, e)
        ok = ee > (LD(1e-14) * scale) ** 2
        t = np.where(ok, -_dot(p0, e) / np.where(ok, ee, 1), -1)
        ok &= (t >= 0) & (t <= 1)
        if ok.any():
            x = p0[ok] + t[ok, None] * e[ok]
            best = min(best, np.sqrt(_dot(x, x)).min())
    if n >= 3:
        idx = _subsets(n, 3)
        p0, e1, e2 = D[idx[:, 0]], D[idx[:, 1]] - D[idx[:, 0]], D[idx[:, 2]] - D[idx[:, 0]]
        g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        r1, r2 = -_dot(p0, e1), -_dot(p0, e2)
        det = g11 * g22 - g12 * g12
        ok = det > LD(1e-12) * g11 * g22
        ds = np.where(ok, det, 1)
        s, t = (r1 * g22 - r2 * g12) / ds, (g11 * r2 - g12 * r1) / ds
        ok &= (s >= 0) & (t >= 0) & (s + t <= 1)
        if ok.any():
            x = p0[ok] + s[ok, None] * e1[ok] + t[ok, None] * e2[ok]
            best = min(best, np.sqrt(_dot(x, x)).min())
    if n >= 4:
        idx = _subsets(n, 4)
        p0 = D[idx[:, 0]]
        e1, e2, e3 = D[idx[:, 1]] - p0, D[idx[:, 2]] - p0, D[idx[:, 3]] - p0
        c23, c31, c12 = np.cross(e2, e3), np.cross(e3, e1), np.cross(e1, e2)
        det = _dot(e1, c23)
        vol = np.sqrt(_dot(e1, e1) * _dot(e2, e2) * _dot(e3, e3))
        ok = np.abs(det) > LD(1e-9) * np.where(vol > 0, vol, 1)
        ds = np.where(ok, det, 1)
        a, b, c = -_dot(p0, c23) / ds, -_dot(p0, c31) / ds, -_dot(p0, c12) / ds   # Cramer: e1 a + e2 b + e3 c = -p0
        if (ok & (a >= 0) & (b >= 0) & (c >= 0) & (a + b + c <= 1)).any():
            return 0.0
    return float(best)


# ---- the flown curve -------------------------------------------------------------------------------------------------------------------------

def curve_derivatives(pkg, state, P, res, u, tr, frac=0.0):
    """(velocity[3], acceleration[3]) in np.longdouble of robot u's trajectory at the START of segment tr (frac in [0, 1): that far into it).
    Piece i is the quintic Bezier curve over the points convert[i] @ net[3i : 3i + 6] in the piece parameter s in [0, 1]; segment k of a piece is
    s in [k / res, (k + 1) / res]; real time is s * piece_time of the robot, so d/dt = (d/ds) / piece_time."""
    conv = pkg.host_tables(P, res)[0]
    i, k = tr // res, tr % res
    net = np.asarray(state["spline"][u], dtype=LD).T          # [T][3]
    B = np.asarray(conv[i], dtype=LD) @ net[3 * i:3 * i + 6]  # [6][3]
    s = (LD(k) + LD(frac)) / LD(res)
    pt = LD(state["piece_time"][u])
    d1 = sum(LD(comb(4, j)) * s ** j * (1 - s) ** (4 - j) * 5 * (B[j + 1] - B[j]) for j in range(5))
    d2 = sum(LD(comb(3, j)) * s ** j * (1 - s) ** (3 - j) * 20 * (B[j + 2] - 2 * B[j + 1] + B[j]) for j in range(4))
    return d1 / pt, d2 / (pt * pt)


def ldnorm(v):
    return np.sqrt(_dot(np.asarray(v, dtype=LD), np.asarray(v, dtype=LD)))


# ---- states and constructed inputs -------------------------------------------------------------------------------------------------------------

def port_state(scene, iters, params=None):
    from oracle.pyoracle import Engine
    e = Engine("port", scene, params)
    for _ in range(iters):
        e.iterate()
    return e.get_state()


def valid_state(st, U):
    """a state that may be uploaded: finite everywhere, positive piece_time, the fleet's size"""
    return st["spline"].shape[0] == U and all(np.all(np.isfinite(st[k])) for k in st) and np.all(st["piece_time"] > 0)


def params_of(pkg, params=None):
    p = dict(pkg.scenes.DEFAULT_PARAMS)
    p.update(params or {})
    return p


def default_range(p):
    return p["offset"] + 2 * p["margin"]


def face_of(hull):
    """three vertex indices of a hull that span a solid supporting face (every vertex on one side, the triangle not a sliver), or None"""
    for t in combinations(range(6), 3):
        a, b, c = hull[list(t)]
        nrm = np.cross(b - a, c - a)
        ln = np.linalg.norm(nrm)
        if ln < 1e-3 * np.linalg.norm(b - a) * np.linalg.norm(c - a):
            continue
        side = (hull - a) @ (nrm / ln)
        if np.all(side <= 1e-13) or np.all(side >= -1e-13):
            return t
    return None


def contact_cases(pkg, scenes):
    """tiny() after 5 port iterations with three cloud points moved: [100] onto a hull vertex of robot 0, [200] into a face of a hull of robot 1,
    [300] strictly inside a hull of robot 2 -- and the state the hulls belong to.  Returns (scene, state, [(robot, segment, cloud index, kind)]).
    Robot 2's inner control points carry a seeded wiggle of 0.05, so that its hulls are solid bodies (those of a nearly straight flight are slivers
    with no interior to speak of).  Precondition asserted here: exact_distance of each moved point from its hull is 0 (vertex), <= 1e-15 (face: the
    point is a rounded convex combination of three hull vertices) and 0 (inside: a tetrahedron of hull vertices contains it)."""
    scene = dict(scenes.tiny(mode=1))
    st = port_state(scene, 5)
    st["spline"][2][:, 2:-2] += np.random.default_rng(31).uniform(-0.05, 0.05, st["spline"][2][:, 2:-2].shape)   # robot 2 wiggles: solid hulls
    H = hulls_of(pkg, st["spline"], scene["P"], 8)
    cloud = scene["cloud"].copy()
    cases = []
    cloud[100] = H[0, 11, 2]; cases.append((0, 11, 100, "vertex"))
    tr_face = 19
    f = list(face_of(H[1, tr_face]) or (0, 2, 5))   # (a hull too thin to show a solid face: any triangle of its vertices, in the hull all the same)
    cloud[200] = (0.5 * H[1, tr_face, f[0]] + 0.3 * H[1, tr_face, f[1]]) + 0.2 * H[1, tr_face, f[2]]; cases.append((1, tr_face, 200, "face"))
    tr_in = 27
    cloud[300] = H[2, tr_in].mean(axis=0); cases.append((2, tr_in, 300, "inside"))   # the vertex mean: inside whatever the hull's shape
    scene["cloud"] = np.ascontiguousarray(cloud)
    assert exact_distance(H[0, 11], cloud[100]) == 0.0
    assert exact_distance(H[1, tr_face], cloud[200]) <= 1e-15
    assert exact_distance(H[2, tr_in], cloud[300]) == 0.0 and exact_distance(H[2, tr_in], H[2, tr_in].mean(axis=0) + [0, 0, 1.0]) > 0.5
    assert valid_state(st, scene["U"]) and np.all(np.isfinite(cloud))
    return scene, st, cases


def overlap_state(pkg, scenes, params=None, gap=None):
    """hard() at its initial state with robot 1's control net replaced by robot 0's shifted in z: gap=None -> by 1e-3 (the thin hulls of the two
    robots overlap or touch within 1e-3 on every segment: a penetration / contact state); gap=g -> exactly two parallel copies g apart, so every
    pair distance of robots 0 and 1 is g up to rounding.  Returns (scene, state)."""
    scene = dict(scenes.hard())
    st = port_state(scene, 0, params)
    st["spline"][1] = st["spline"][0]
    st["spline"][1][2] = st["spline"][0][2] + (1e-3 if gap is None else gap)
    assert valid_state(st, scene["U"])
    return scene, st


def tie_scene(scenes, H, u, tr, i, j, kind="twin"):
    """tiny() with two primitives at EQUAL distance from hull (u, tr) of the initial (straight, level) trajectory, written at indices i and j:
    kind "twin": the same point 0.02 above hull vertex 3 twice; "tris": the same triangle twice (a scene of triangles).  (A point above and its
    mirror image below the level hull are NOT equally far in floating point: 0.02 against 0.01999999999999999.)  Which of the two the BVH's sort
    puts first need not follow the caller's order; the tests run the pair at (i, j) = (40, 555) and at (555, 40).  The precondition (bit-equal distances, the robot's minimum) is asserted by
    tests/test_audit_ref.py and again by the GPU test before it uploads."""
    scene = dict(scenes.tiny(mode=1))
    v, up = H[u, tr, 3], np.array([0.0, 0.0, 0.02])
    if kind == "tris":
        scene = scenes.triangulate(scene)
        o = np.array([[0.03, 0.0, 0.0], [-0.02, 0.025, 0.01], [-0.01, -0.025, 0.02]])
        tris = scene["tris"].copy()
        tris[i] = v + up + o; tris[j] = v + up + o
        scene["tris"] = np.ascontiguousarray(tris)
        return scene
    cloud = scene["cloud"].copy()
    cloud[i] = v + up; cloud[j] = v + up
    scene["cloud"] = np.ascontiguousarray(cloud)
    return scene


def tie_precondition(pr, H, u, scene, i, j, rng=0.3):
    """the two primitives are equally far from robot u, bit for bit, and nothing is nearer; returns the expected record (value, segment, min(i, j))"""
    X = np.asarray(scene["tris"] if scene.get("tris") is not None else scene["cloud"], dtype=np.float64)
    d, ids = all_obs(pr, H[u:u + 1], X)
    v, tr, k = robot_min(*cap(d, ids, rng), rng)[0]
    assert k == min(i, j) and v < rng, (k, i, j, v)
    assert norm3(pr.gjk(H[u, tr], X[i].reshape(-1, 3))) == norm3(pr.gjk(H[u, tr], X[j].reshape(-1, 3))) == v
    return v, tr, k


def scaled_time_state(st, u, pt):
    out = {k: v.copy() for k, v in st.items()}
    out["piece_time"][u] = pt
    return out


def piece_time_for(pkg, st, P, res, u, p, want):
    """a piece_time for robot u under which exactly the flags in `want` (subset of {"speed", "accel"}) are expected: speed scales with 1 / pt and
    accel with 1 / pt^2, so with s1, a1 the peaks at pt = 1 the speed flag is set for pt <= s1 / vel_limit and the accel flag for pt <= sqrt(a1 /
    acc_limit).  Returns pt strictly inside the wanted interval (its geometric middle), or None if the interval is empty for this state."""
    one = scaled_time_state(st, u, 1.0)
    s1, _, a1, _, _ = limits_of(pkg, one, P, res)[u]
    ts, ta = s1 / p["vel_limit"], np.sqrt(a1 / p["acc_limit"])
    lo, hi = min(ts, ta), max(ts, ta)
    if want == set():
        pt = 2 * hi
    elif want == {"speed", "accel"}:
        pt = 0.5 * lo
    elif (want == {"speed"}) == (ts > ta):   # the wanted flag is the one with the larger threshold
        pt = float(np.sqrt(lo * hi))
    else:
        return None
    sp, _, ac, _, _ = limits_of(pkg, scaled_time_state(st, u, pt), P, res)[u]
    assert (sp >= p["vel_limit"]) == ("speed" in want) and (ac >= p["acc_limit"]) == ("accel" in want), (pt, sp, ac)
    return pt


def equal_minima_scene(pkg, scenes):
    """hard() with P = 12 (S = 96) at its initial straight trajectory, where a cloud point on a hull vertex gives |v| == 0.0 exactly: robot 1 gets
    one on the first vertex of segment 10 (index 1500) and one on the first vertex of segment 74 (index 700) -- 0.0 in segments 9, 10, 73, 74, rows 9
    and 73 in the same lane of the reduction; robot 2 gets one in segment 80 only (index 2200).  Returns (scene, state, d, ids) with the unfiltered
    brute force; the precondition is asserted here."""
    scene = dict(scenes.hard(4, 3000, pieces=12))
    st = port_state(scene, 0)
    H = hulls_of(pkg, st["spline"], 12, 8)
    cloud = scene["cloud"].copy()
    cloud[700] = H[1, 74, 0]; cloud[1500] = H[1, 10, 0]; cloud[2200] = H[2, 80, 0]
    scene["cloud"] = np.ascontiguousarray(cloud)
    d, ids = all_obs(prims(), H, cloud)
    assert d[1, 9] == d[1, 10] == d[1, 73] == d[1, 74] == 0.0 and ids[1, 9] == 1500 and ids[1, 73] == 700
    assert d[2, 79] == d[2, 80] == 0.0 and np.all(d[2, :79] > 0) and ids[2, 79] == 2200
    assert valid_state(st, 4) and np.all(np.isfinite(cloud))
    return scene, st, d, ids


def threshold_scene(pkg, scenes, params, gap, contact, between=False):
    """hard() under `params` with robots 0 and 1 as parallel copies `gap` apart and cloud point 77 `gap` below robot 3's path.  Returns (scene,
    state, rows_obs, rows_pair) (unfiltered, uncapped).  Precondition asserted here: robot 3's obstacle clearance and the pair clearance of robots 0
    and 1 (who name each other) are <= offset exactly if `contact`; with between=True both lie strictly between margin and offset and robot 3's
    nearest point is 77."""
    p = params_of(pkg, params)
    scene, st = overlap_state(pkg, scenes, params, gap=gap)
    H = hulls_of(pkg, st["spline"], 5, 8)
    cloud = scene["cloud"].copy()
    cloud[77] = H[3, 20, 3] + np.array([0.0, 0.0, -gap])
    scene["cloud"] = np.ascontiguousarray(cloud)
    pr = prims(params)
    rows_o, rows_p = all_obs(pr, H, cloud), all_pair(pr, H)
    rng = default_range(p)
    ro, rp = robot_min(*cap(*rows_o, rng), rng), robot_min(*cap(*rows_p, rng), rng)
    assert (ro[3][2] >= 0 and ro[3][0] <= p["offset"]) == contact, (gap, ro[3])
    assert (rp[0][0] <= p["offset"]) == contact == (rp[1][0] <= p["offset"]), (gap, rp[:2])
    assert (rp[0][2], rp[1][2]) == (1, 0) or not (contact or between), (gap, rp[:2])      # in contact, the two name each other
    if between:
        lo, hi = min(p["margin"], p["offset"]), max(p["margin"], p["offset"])
        assert lo < ro[3][0] < hi and ro[3][2] == 77 and lo < rp[0][0] < hi
    assert valid_state(st, 4) and np.all(np.isfinite(cloud))
    return scene, st, rows_o, rows_p


def threshold_gaps(p):
    """(gap, contact expected, between) per parameter set: between margin and offset (contact only where offset is the larger: a kernel that
    compares with margin answers the opposite), well below both, above both"""
    lo, hi = min(p["margin"], p["offset"]), max(p["margin"], p["offset"])
    return [(0.5 * (lo + hi), p["offset"] > p["margin"], True), (0.5 * lo, True, False), (hi + 0.02, False, False)]


def limit_piece_times(pkg, st, u, p):
    """piece_time values for robot u: one per flag combination that pure time scaling can reach (piece_time_for), and two that put its peak speed,
    then its peak acceleration, at the geometric mean of vel_limit and acc_limit -- between them, so swapped limits flip that flag.  Asserted
    here: the list shows each of the two flags set and clear, and at least one entry answers differently under swapped limits."""
    pts = [piece_time_for(pkg, st, 5, 8, u, p, want) for want in (set(), {"speed"}, {"accel"}, {"speed", "accel"})]
    s1, _, a1, _, _ = limits_of(pkg, scaled_time_state(st, u, 1.0), 5, 8)[u]
    mid = float(np.sqrt(p["vel_limit"] * p["acc_limit"]))
    pts = [x for x in pts if x is not None] + [s1 / mid, float(np.sqrt(a1 / mid))]
    seen, differs = set(), False
    for pt in pts:
        sp, _, ac, _, _ = limits_of(pkg, scaled_time_state(st, u, pt), 5, 8)[u]
        seen |= {("speed", sp >= p["vel_limit"]), ("accel", ac >= p["acc_limit"])}
        differs |= (sp >= p["vel_limit"]) != (sp >= p["acc_limit"]) or (ac >= p["acc_limit"]) != (ac >= p["vel_limit"])
    assert len(seen) == 4 and differs
    return pts


def range_corner_scene(pkg, scenes):
    """tiny() at its initial state with cloud point 123 moved 0.01 above a hull vertex of robot 1: at range 0.05 (< offset) robot 1 has a primitive
    within range, robots 0 and 2 have nothing within range, and no two robots are within range of each other (asserted here)"""
    scene = dict(scenes.tiny(mode=1))
    st = port_state(scene, 0)
    H = hulls_of(pkg, st["spline"], 5, 8)
    cloud = scene["cloud"].copy()
    cloud[123] = H[1, 17, 0] + np.array([0.0, 0.0, 0.01])
    scene["cloud"] = np.ascontiguousarray(cloud)
    pr = prims()
    ro = robot_min(*brute_obs(pr, H, cloud, 0.05, prefilter=False), 0.05)
    rp = robot_min(*brute_pair(pr, H, 0.05), 0.05)
    assert ro[1][2] == 123 and ro[1][0] < 0.05 and ro[0] == (0.05, -1, -1) == ro[2] and all(r == (0.05, -1, -1) for r in rp)
    assert valid_state(st, 3)
    return scene, st, H
