"""GPU (-m gpu): tj_audit -- obstacle / robot-pair clearance, dynamic limits, duration of the state the solver holds.

Expected values: oracle.pyoracle.Prims.gjk (the reference's own openGJK where oracle/_ref/libref.so is present, else the port, which is
pinned to it bit for bit) applied to hulls this file forms itself from host_tables with the ascending six-term sum, over EVERY primitive whose
point (or whose triangle's box) lies within `range` of the hull's box -- a numpy prefilter with the device's comparison, nothing sampled.
Distances and limits are compared with == on the doubles: same inputs, same expressions (no FMA contraction on either side)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
STATE = ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time")


def prims():
    from oracle.pyoracle import Prims, available
    return Prims("ref" if available("ref") else "port")


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


def brute_obs(pr, H, prims_xyz, rng):
    """prims_xyz [N][3] points or [N][3][3] triangles -> (d[U][S], id[U][S]); id -1 and d = rng where nothing is closer"""
    U, S = H.shape[:2]
    tri = prims_xyz.ndim == 3
    plo = prims_xyz.min(axis=1) if tri else prims_xyz
    phi = prims_xyz.max(axis=1) if tri else prims_xyz
    d = np.full((U, S), rng); ids = np.full((U, S), -1, dtype=np.int64)
    for u in range(U):
        for tr in range(S):
            lo, hi = H[u, tr].min(axis=0), H[u, tr].max(axis=0)
            near = np.flatnonzero(~((phi + rng < lo) | (plo > hi + rng)).any(axis=1))   # box_hit's comparison (kernels_sep.h)
            for i in near:
                x = norm3(pr.gjk(H[u, tr], prims_xyz[i].reshape(-1, 3)))
                if x < rng and (x < d[u, tr] or (x == d[u, tr] and i < ids[u, tr])):
                    d[u, tr], ids[u, tr] = x, i
    return d, ids


def brute_pair(pr, H, rng):
    U, S = H.shape[:2]
    d = np.full((U, S), rng); ids = np.full((U, S), -1, dtype=np.int64)
    for u in range(U):
        for tr in range(S):
            for q in range(U):
                if q == u:
                    continue
                a, b = (u, q) if u < q else (q, u)   # plane_pair: the lower robot index is body 1
                x = norm3(pr.gjk(H[a, tr], H[b, tr]))
                if x < rng and x < d[u, tr]:
                    d[u, tr], ids[u, tr] = x, q
    return d, ids


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


def check_clearances(pkg, slv, scene, rng, multi=True):
    p = slv.params
    r = p["offset"] + 2 * p["margin"] if rng is None else rng
    a = slv.audit(range=rng, per_segment=True)
    H = hulls_of(pkg, slv.get_state()["spline"], slv.P, slv.res)
    pr = prims()
    xyz = scene["tris"] if scene.get("tris") is not None else scene["cloud"]
    d, ids = brute_obs(pr, H, np.asarray(xyz, dtype=np.float64), r)
    assert np.array_equal(a["seg_obs"], d)
    for u, (v, tr, i) in enumerate(robot_min(d, ids, r)):
        assert (a["obs_clearance"][u], a["obs_segment"][u], a["obs_index"][u]) == (v, tr, i), u
    if multi:
        d, ids = brute_pair(pr, H, r)
        assert np.array_equal(a["seg_pair"], d)
        for u, (v, tr, q) in enumerate(robot_min(d, ids, r)):
            assert (a["pair_clearance"][u], a["pair_segment"][u], a["pair_robot"][u]) == (v, tr, q), u
    else:
        assert np.all(a["pair_clearance"] == r) and np.all(a["pair_segment"] == -1) and np.all(a["pair_robot"] == -1) and np.all(a["seg_pair"] == r)
    return a


@pytest.mark.parametrize("name", ["hard", "tiny"])
def test_clearances_equal_brute_force(pkg, scenes, name):
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 5):
        if it:
            slv.iterate(it)
        for rng in (None, 1.0) + ((100.0,) if name == "tiny" and it == 0 else ()):   # 100: the whole cloud of 600 points, still exact, no capacity error
            check_clearances(pkg, slv, scene, rng)
    slv.close()


def test_single_uav(pkg, scenes):
    scene = scenes.tiny(mode=0)
    slv = pkg.Solver(scene, stop=0.0)
    check_clearances(pkg, slv, scene, None, multi=False)
    slv.iterate(5)
    check_clearances(pkg, slv, scene, 1.0, multi=False)
    slv.close()


def test_triangles(pkg, scenes):
    base = scenes.tiny(mode=1)
    cloud = pkg.Solver(base, stop=0.0); deg = pkg.Solver(scenes.triangulate(base, degenerate=True), stop=0.0)
    for s in (cloud, deg):
        s.iterate(3)
    a, b = cloud.audit(range=1.0, per_segment=True), deg.audit(range=1.0, per_segment=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k   # three equal vertices = the cloud point, bit for bit
    cloud.close(); deg.close()
    scene = scenes.triangulate(base)
    slv = pkg.Solver(scene, stop=0.0)
    check_clearances(pkg, slv, scene, None)
    slv.iterate(3)
    check_clearances(pkg, slv, scene, 1.0)
    slv.close()


def limits_of(pkg, st, P, res):
    """Energy_admm.h:131-165 in the line search's association (kernels_ls.h): per robot (speed, segment, accel, segment, duration)"""
    H = hulls_of(pkg, st["spline"], P, res)
    out = []
    for u in range(H.shape[0]):
        pt = st["piece_time"][u]
        sp, ss, ac, acs = -1.0, -1, -1.0, -1
        for tr in range(P * res):
            k = tr % res
            w = (k + 1) / float(res) - k / float(res)   # the table value (seg_weight), not 1 / res
            Pp = H[u, tr]
            for b in range(5):
                v = 5 * (Pp[b + 1] - Pp[b])
                x = norm3(v) / (w * pt)
                if x > sp:
                    sp, ss = x, tr
            for j in range(4):
                v = 20 * (Pp[j + 2] - 2 * Pp[j + 1] + Pp[j])
                x = norm3(v) / (w * w * pt * pt)
                if x > ac:
                    ac, acs = x, tr
        dur = 0.0
        for _ in range(P):
            dur += 1.0 * pt
        out.append((sp, ss, ac, acs, dur))
    return out


def test_limits_and_what_the_solver_maintains(pkg, scenes):
    """speed / accel / duration equal the numpy restatement at the start and after 10 iterations of hard().  After those 10 iterations every speed < vel_limit and
    accel < acc_limit (bound_energy is infinite otherwise, so the line search never accepts such a state) and every clearance > offset (what the CCD clamp maintains:
    it rejects a step whose swept hull comes within offset).  Checked on the CPU before this assertion was written: 10 iterations of hard() with the port and with the
    unmodified reference, clearances by brute force -- both end with obstacle clearances 0.1235 ... 0.1594 and pair clearances 0.1447 ... 0.1579 (> offset = 0.1), speeds
    1.714 ... 1.822 and accelerations 1.976 ... 1.9985 (limits 2); the two engines agree to ~1e-12, so hard() at 10 iterations stays the case."""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 10):
        if it:
            slv.iterate(it)
        a = slv.audit()
        for u, (sp, ss, ac, acs, dur) in enumerate(limits_of(pkg, slv.get_state(), slv.P, slv.res)):
            assert (a["speed"][u], a["speed_segment"][u], a["accel"][u], a["accel_segment"][u], a["duration"][u]) == (sp, ss, ac, acs, dur), (it, u)
    p = slv.params
    assert np.all(a["speed"] < p["vel_limit"]) and np.all(a["accel"] < p["acc_limit"])
    assert np.all(a["obs_clearance"] > p["offset"]) and np.all(a["pair_clearance"] > p["offset"])
    assert np.all(a["flags"] == 0)
    slv.close()


def test_start_in_collision_is_reported(pkg, scenes):
    """one cloud point moved onto robot 1's straight initial path (the first hull vertex of segment 17 = the curve's point there): the audit straight after construction
    names it; no iteration is run"""
    scene = dict(scenes.tiny(mode=1))
    probe = pkg.Solver(scene, stop=0.0)
    H = hulls_of(pkg, probe.get_state()["spline"], probe.P, probe.res)
    probe.close()
    cloud = scene["cloud"].copy(); cloud[123] = H[1, 17, 0]
    scene["cloud"] = cloud
    slv = pkg.Solver(scene, stop=0.0)
    a = slv.audit()
    assert a["obs_clearance"][1] == 0.0 and a["obs_index"][1] == 123 and a["obs_segment"][1] in (16, 17)   # (the vertex is shared with the end of segment 16)
    assert a["flags"][1] & pkg.AUDIT_FLAGS["obs_contact"]
    assert a["obs_clearance"][1] == norm3(prims().gjk(H[1, a["obs_segment"][1]], cloud[123:124]))
    assert not (a["flags"][0] & pkg.AUDIT_FLAGS["obs_contact"])
    assert slv.stats()["iters"] == 0
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_audit_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        monkeypatch.setenv("TJ_XS_ASYNC", "0"); monkeypatch.setenv("TJ_FRONT_ASYNC", "0")
    scene = scenes.hard()

    def run(audited):   # one context at a time: a second live context may find the process's hardware-queue budget taken and keep the one-queue chain (tj_create)
        s = pkg.Solver(scene, stop=0.0)
        for k in range(3):
            if k == 1:   # right behind iterate_async: the audit drains the queues itself
                s.iterate_async(2)
                if audited:
                    s.audit(range=1.0, per_segment=True)
                else:
                    s.sync()
            else:
                s.iterate(2)
                if audited:
                    s.audit(); s.audit(range=1.0)
        out = s.get_state(), s.stats(), s.launch_count()
        s.close()
        return out

    (sa, ta, la), (sb, tb, lb) = run(True), run(False)
    for n in STATE:
        assert np.array_equal(sa[n], sb[n]), n
    assert ta == tb
    assert la == lb


@pytest.mark.parametrize("mode", [1, 2])
def test_sharded_audit_equals_one_context(pkg, scenes, mode):
    scene = dict(scenes.hard(), mode=mode)
    one = pkg.Solver(scene, stop=0.0)
    grp = pkg.Group(scene, [0, 0], stop=0.0)
    for it in (0, 3):
        if it:
            one.iterate(it); grp.iterate(it)
        for rng in (None, 1.0):
            x, y = one.audit(range=rng, per_segment=True), grp.audit(range=rng, per_segment=True)
            for k in x:
                assert np.array_equal(x[k], y[k]), (it, rng, k)
    grp.close(); one.close()
    one = pkg.Solver(scene, stop=0.0)   # (a fresh one: the sharded context below is at the initial state)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)   # a sharded context reports its own robots and zeroes the others
    x, y = one.audit(per_segment=True), half.audit(per_segment=True)
    for k in x:
        assert np.array_equal(x[k][2:], y[k][2:]) and not np.any(y[k][:2]), k
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    lib = pkg.load_library()
    tp = pkg.TjParams()
    lib.tj_default_params(C.byref(tp), 1, 3, 5)
    ctx = C.c_void_p()
    assert lib.tj_create(C.byref(tp), C.byref(ctx)) == 0
    rec = (pkg.TjAuditRobot * 3)()
    assert lib.tj_audit(ctx, C.c_double(0.0), rec, None, None) == -1          # before tj_init_state
    wp = np.ascontiguousarray(scenes.tiny(mode=1)["waypoints"])
    assert lib.tj_init_state(ctx, wp.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(20.0)) == 0
    assert lib.tj_audit(ctx, C.c_double(0.0), None, None, None) == -1         # NULL out
    assert lib.tj_audit(ctx, C.c_double(0.0), rec, None, None) == 0           # no obstacles set: valid, nothing within range
    assert all(r.obs_index == -1 and abs(r.obs_clearance - 0.3) < 1e-15 for r in rec)
    assert lib.tj_audit(None, C.c_double(0.0), rec, None, None) == -1
    lib.tj_destroy(ctx)
