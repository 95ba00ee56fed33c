"""GPU (-m gpu): tj_audit -- obstacle / robot-pair clearance, dynamic limits, duration of the state the solver holds.

Expected values come from tests/audit_ref.py: oracle.pyoracle.Prims.gjk (the reference's own openGJK where oracle/_ref/libref.so is present, else
the port, which is pinned to it bit for bit) applied to hulls formed from host_tables with the ascending six-term sum, over EVERY primitive and
every other robot -- no box filter, nothing sampled (tests/test_audit_ref.py shows on the CPU that the filtered form agrees).  Distances and
limits are compared with == on the doubles: same inputs, same expressions (no FMA contraction on either side).  The truth tests compare with an
exact distance that shares nothing with GJK, at the bars measured in tests/test_audit_ref.py."""
import ctypes as C

import numpy as np
import pytest

import audit_ref as R
from audit_ref import brute_obs, brute_pair, hulls_of, limits_of, norm3, prims, robot_min
from test_audit_ref import GJK_BAR
from query_kit import STATE, CliCase, assert_group_equals, assert_read_only, close_to_six_digits, group_pair, one_queue, raw_context
from test_oracle_params import PARAM_SETS

pytestmark = pytest.mark.gpu
DEFAULT_RANGE = 0.1 + 2 * 0.1   # offset + 2 * margin at the shipped values, in the library's association (0.30000000000000004)


def check_clearances(pkg, slv, scene, rng, multi=True):
    p = slv.params
    r = p["offset"] + 2 * p["margin"] if rng is None else rng
    a = slv.audit(range=rng, per_segment=True)
    H = hulls_of(pkg, slv.get_state()["spline"], slv.P, slv.res)
    pr = prims()
    xyz = scene["tris"] if scene.get("tris") is not None else scene["cloud"]
    d, ids = brute_obs(pr, H, np.asarray(xyz, dtype=np.float64), r, prefilter=False)
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
    d16, d17 = (norm3(prims().gjk(H[1, tr], cloud[123:124])) for tr in (16, 17))   # (the vertex is shared with the end of segment 16)
    assert min(d16, d17) == 0.0
    assert a["obs_clearance"][1] == 0.0 and a["obs_index"][1] == 123 and a["obs_segment"][1] == (16 if d16 <= d17 else 17)   # equal values: the smallest segment
    assert a["flags"][1] & pkg.AUDIT_FLAGS["obs_contact"]
    assert a["obs_clearance"][1] == norm3(prims().gjk(H[1, a["obs_segment"][1]], cloud[123:124]))
    assert not (a["flags"][0] & pkg.AUDIT_FLAGS["obs_contact"])
    assert slv.stats()["iters"] == 0
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_audit_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    assert_read_only(pkg, scenes.hard(), lambda s: s.audit(range=1.0, per_segment=True), lambda s: (s.audit(), s.audit(range=1.0)))


@pytest.mark.parametrize("mode", [1, 2])
def test_sharded_audit_equals_one_context(pkg, scenes, mode):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, 2)
    assert_group_equals(one, grp, lambda s, rng: s.audit(range=rng, per_segment=True), ((None,), (1.0,)))
    grp.close(); one.close()
    one = pkg.Solver(scene, stop=0.0)   # (a fresh one: the sharded context below is at the initial state)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)   # a sharded context reports its own robots and zeroes the others
    x, y = one.audit(per_segment=True), half.audit(per_segment=True)
    for k in x:
        assert np.array_equal(x[k][2:], y[k][2:]) and not np.any(y[k][:2]), k
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec = (pkg.TjAuditRobot * 3)()
        assert lib.tj_audit(ctx, C.c_double(0.0), rec, None, None) == -1          # before tj_init_state
        init()
        assert lib.tj_audit(ctx, C.c_double(0.0), None, None, None) == -1         # NULL out
        assert lib.tj_audit(ctx, C.c_double(0.0), rec, None, None) == 0           # no obstacles set: valid, nothing within range
        assert all(r.obs_index == -1 and abs(r.obs_clearance - 0.3) < 1e-15 for r in rec)
        assert lib.tj_audit(None, C.c_double(0.0), rec, None, None) == -1


# ---- sizes, tables, flags, ties, truth, errors (the shapes the tests above never reach) ----------------------------------------------------

def check_records(a, want_rows, kind, rng):
    d, ids = want_rows
    assert np.array_equal(a["seg_" + kind], d), kind
    names = ("obs_clearance", "obs_segment", "obs_index") if kind == "obs" else ("pair_clearance", "pair_segment", "pair_robot")
    for u, rec in enumerate(robot_min(d, ids, rng)):
        assert tuple(a[n][u] for n in names) == rec, (kind, u)


def check_limits(pkg, slv, a):
    for u, (sp, ss, ac, acs, dur) in enumerate(limits_of(pkg, slv.get_state(), slv.P, slv.res)):
        assert (a["speed"][u], a["speed_segment"][u], a["accel"][u], a["accel_segment"][u], a["duration"][u]) == (sp, ss, ac, acs, dur), u


def expected_flags(pkg, p, a_rows_obs, a_rows_pair, lim, rng, multi=True):
    """the header's flag word from the brute force and the restated limits: offset for both contacts, vel_limit for speed, acc_limit for accel"""
    F = pkg.AUDIT_FLAGS
    out = []
    ro, rp = robot_min(*a_rows_obs, rng), robot_min(*a_rows_pair, rng) if multi else None
    for u in range(len(lim)):
        f = F["obs_contact"] if ro[u][2] >= 0 and ro[u][0] <= p["offset"] else 0
        if multi and rp[u][2] >= 0 and rp[u][0] <= p["offset"]:
            f |= F["pair_contact"]
        f |= (F["speed"] if lim[u][0] >= p["vel_limit"] else 0) | (F["accel"] if lim[u][2] >= p["acc_limit"] else 0)
        out.append(f)
    return np.array(out)


@pytest.mark.parametrize("U", [64, 65, 70, 130])
def test_fleet_sizes_beyond_one_pair_batch(pkg, scenes, U):
    """k_audit's partner loop takes 64 robots per pass: a full single batch, a second batch of one robot, a partly filled one, three batches;
    qr == u in a later batch, the LDS tile reused.  crossing() stacks the fleet 0.25 apart, so at the start every inner robot is equidistant from
    both neighbours (checked on the CPU in tests/test_audit_ref.py): the smaller robot index is expected.  U = 130 also through a group of three
    ranks on one device (44 + 43 + 43 robots: owners in different batches) == one context."""
    scene = scenes.crossing(U, 600, seed=5)
    slv = pkg.Solver(scene, stop=0.0)
    grp = pkg.Group(scene, [0, 0, 0], stop=0.0) if U == 130 else None
    pr = prims()
    for it in (0, 3):
        if it:
            slv.iterate(it)
            if grp:
                grp.iterate(it)
        st = slv.get_state()
        assert R.valid_state(st, U)
        d, ids = R.all_pair(pr, hulls_of(pkg, st["spline"], slv.P, slv.res))
        if it == 0:
            assert np.sum(ids[1:U - 1, 20] == np.arange(0, U - 2)) > U // 2   # the tie between u - 1 and u + 1 goes to u - 1
        for rng in (None, 1.0):
            r = DEFAULT_RANGE if rng is None else rng
            a = slv.audit(range=rng, per_segment=True)
            check_records(a, R.cap(d, ids, r), "pair", r)
            if grp:
                g = grp.audit(range=rng, per_segment=True)
                for k in a:
                    assert np.array_equal(a[k], g[k]), (it, rng, k)
    if grp:
        grp.close()
    slv.close()


@pytest.mark.parametrize("P,res", [(9, 8), (12, 8), (20, 8), (3, 15), (3, 16), (2, 16)])
def test_segment_counts_and_tables(pkg, scenes, P, res):
    """S = 72, 96, 160 rows per robot (k_audit_reduce's lanes hold two or three rows each), res 15 / 16 (seg_weight and basis away from 1/8): the
    scene construction of test_piece_counts_and_resolutions_vs_oracle, state from the CPU engine after 3 iterations"""
    scene = dict(scenes.hard(4, 3000, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    pr = prims()
    H = hulls_of(pkg, st["spline"], P, res)
    rows_o, rows_p = R.all_obs(pr, H, scene["cloud"]), R.all_pair(pr, H)
    for rng in (None, 1.0):
        r = DEFAULT_RANGE if rng is None else rng
        a = slv.audit(range=rng, per_segment=True)
        check_records(a, R.cap(*rows_o, r), "obs", r)
        check_records(a, R.cap(*rows_p, r), "pair", r)
        check_limits(pkg, slv, a)
    slv.close()


def test_equal_minima_64_segments_apart_and_a_minimum_beyond_segment_64(pkg, scenes):
    """S = 96 (tests/audit_ref.py equal_minima_scene): robot 1 has |v| == 0.0 in segments 9, 10, 73 and 74 -- rows 9 and 73 sit in the same lane of
    the reduction: segment 9 is expected; robot 2's minimum lies in segment 79, a lane's second row"""
    scene, st, d, ids = R.equal_minima_scene(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)   # the very state the hulls were formed from
    a = slv.audit(per_segment=True)
    check_records(a, R.cap(d, ids, DEFAULT_RANGE), "obs", DEFAULT_RANGE)
    assert (a["obs_segment"][1], a["obs_index"][1], a["obs_segment"][2], a["obs_index"][2]) == (9, 1500, 79, 2200)
    slv.close()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_flags_and_default_range_at_sets_a_and_b(pkg, scenes, tag):
    """margin != offset and vel_limit != acc_limit (tests/test_oracle_params.py): the default range is offset + 2 * margin, contacts compare with
    offset, speed with vel_limit, accel with acc_limit.  Constructed states (tests/audit_ref.py threshold_scene, limit_piece_times; their
    preconditions run on the CPU in tests/test_audit_ref.py too) sit BETWEEN the values a swapped comparison would use, then below and above both;
    every one of the four flags is seen set and seen clear on the robot built for it, the other robots' words as the brute force says."""
    p = R.params_of(pkg, PARAM_SETS[tag])
    F = pkg.AUDIT_FLAGS
    rng = R.default_range(p)
    seen_set, seen_clear = set(), set()
    for gap, contact, between in R.threshold_gaps(p):
        scene, st, rows_o, rows_p = R.threshold_scene(pkg, scenes, PARAM_SETS[tag], gap, contact, between)
        rows_o, rows_p = R.cap(*rows_o, rng), R.cap(*rows_p, rng)
        slv = pkg.Solver(scene, PARAM_SETS[tag], stop=0.0)
        for pt in R.limit_piece_times(pkg, st, 2, p) if between else [st["piece_time"][2]]:   # robot 2's piece_time scaled: speed ~ 1 / pt, accel ~ 1 / pt^2
            s2 = R.scaled_time_state(st, 2, pt)
            assert R.valid_state(s2, 4)
            slv.set_state(s2)
            a = slv.audit(per_segment=True)                                  # range 0: the default
            check_records(a, rows_o, "obs", rng)
            check_records(a, rows_p, "pair", rng)
            check_limits(pkg, slv, a)
            exp = expected_flags(pkg, p, rows_o, rows_p, limits_of(pkg, s2, 5, 8), rng)
            assert np.array_equal(a["flags"], exp), (gap, pt, a["flags"], exp)
            assert bool(exp[3] & F["obs_contact"]) == contact and bool(exp[0] & F["pair_contact"]) == contact == bool(exp[1] & F["pair_contact"])
            for n in F:
                for u in range(4):
                    (seen_set if a["flags"][u] & F[n] else seen_clear).add((n, u))
        slv.close()
    for n, u in (("obs_contact", 3), ("pair_contact", 0), ("pair_contact", 1), ("speed", 2), ("accel", 2)):
        assert (n, u) in seen_set and (n, u) in seen_clear, (n, u)


def test_every_flag_is_seen_set_at_the_shipped_values(pkg, scenes):
    """PAIR_CONTACT names both robots; SPEED and ACCEL alone and together; at the defaults (offset 0.1, limits 2)"""
    p = R.params_of(pkg)
    F = pkg.AUDIT_FLAGS
    scene, st = R.overlap_state(pkg, scenes, gap=0.05)
    slv = pkg.Solver(scene, stop=0.0)
    H = hulls_of(pkg, st["spline"], 5, 8)
    pr = prims()
    rows_o, rows_p = R.cap(*R.all_obs(pr, H, scene["cloud"]), DEFAULT_RANGE), R.cap(*R.all_pair(pr, H), DEFAULT_RANGE)
    for want in (set(), {"speed"}, {"accel"}, {"speed", "accel"}):
        pt = R.piece_time_for(pkg, st, 5, 8, 3, p, want)
        if pt is None:
            continue
        s2 = R.scaled_time_state(st, 3, pt)
        slv.set_state(s2)
        a = slv.audit()
        exp = expected_flags(pkg, p, rows_o, rows_p, limits_of(pkg, s2, 5, 8), DEFAULT_RANGE)
        assert np.array_equal(a["flags"], exp), (want, a["flags"], exp)
        assert exp[0] & F["pair_contact"] and exp[1] & F["pair_contact"] and (a["pair_robot"][0], a["pair_robot"][1]) == (1, 0)
        assert not exp[2] & F["pair_contact"]
    slv.close()


@pytest.mark.parametrize("kind", ["twin", "tris"])
@pytest.mark.parametrize("i,j", [(40, 555), (555, 40)])
def test_equal_distances_report_the_callers_smaller_index(pkg, scenes, kind, i, j):
    """two primitives at bit-equal distance (the same point / the same triangle at two indices of the caller's list): obs_index is min(i, j)
    whatever order the BVH's sort gave them -- A.order undoes the sort"""
    tiny = scenes.tiny(mode=1)
    st = R.port_state(tiny, 0)
    H = hulls_of(pkg, st["spline"], 5, 8)
    scene = R.tie_scene(scenes, H, 1, 20, i, j, kind)
    v, tr, k = R.tie_precondition(prims(), H, 1, scene, i, j)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)   # the very state the hulls above were formed from
    a = slv.audit()
    assert (a["obs_clearance"][1], a["obs_segment"][1], a["obs_index"][1]) == (v, tr, min(i, j))
    slv.close()


def nearest_exact(H, X, u, seg, idx, value, bar):
    """the record names a primitive whose EXACT distance is `value` within `bar`, and no primitive is exactly closer by more than `bar`"""
    X = np.asarray(X, dtype=np.float64)
    e = R.exact_distance(H[u, seg], X[idx])
    assert abs(value - e) <= bar, (u, seg, idx, value, e)
    tri = X.ndim == 3
    plo, phi = (X.min(axis=1), X.max(axis=1)) if tri else (X, X)
    m = value + 1e-9
    for tr in range(H.shape[1]):
        lo, hi = H[u, tr].min(axis=0), H[u, tr].max(axis=0)
        for i in np.flatnonzero(~((phi + m < lo) | (plo > hi + m)).any(axis=1)):
            assert R.exact_distance(H[u, tr], X[i]) >= value - bar, (u, tr, i)


@pytest.mark.parametrize("name", ["hard10", "tiny_tri", "contact", "overlap"])
def test_clearances_are_distances(pkg, scenes, name):
    """the reported clearance against an exact Euclidean distance that shares nothing with GJK (tests/audit_ref.py exact_distance), at the bars
    measured on the CPU per class (tests/test_audit_ref.py GJK_BAR): cloud points, hull pairs and a point on a face at rounding level; triangles, a
    point on a vertex and a point inside a solid hull are the stated limits of openGJK's stopping rule (4.5e-13, 1e-5, 5.3e-7 seen)"""
    if name == "hard10":
        scene = scenes.hard(); slv = pkg.Solver(scene, stop=0.0); slv.iterate(10); X, kind = scene["cloud"], "point"
    elif name == "tiny_tri":
        scene = scenes.triangulate(scenes.tiny(mode=1)); slv = pkg.Solver(scene, stop=0.0); slv.iterate(3); X, kind = scene["tris"], "triangle"
    elif name == "contact":
        scene, st, cases = R.contact_cases(pkg, scenes); slv = pkg.Solver(scene, stop=0.0); slv.set_state(st); X, kind = scene["cloud"], None
    else:
        scene, st = R.overlap_state(pkg, scenes); slv = pkg.Solver(scene, stop=0.0); slv.set_state(st); X, kind = scene["cloud"], "point"
    a = slv.audit(range=1.0)
    H = hulls_of(pkg, slv.get_state()["spline"], slv.P, slv.res)
    for u in range(slv.U):
        assert a["obs_index"][u] >= 0 and a["pair_robot"][u] >= 0
        bar = GJK_BAR[kind or next(k for cu, _, _, k in cases if cu == u)]   # contact scene: one constructed case per robot, each at its own bar
        nearest_exact(H, X, u, a["obs_segment"][u], a["obs_index"][u], a["obs_clearance"][u], bar)
        seg, q = a["pair_segment"][u], a["pair_robot"][u]
        assert abs(a["pair_clearance"][u] - R.exact_distance(H[u, seg], H[q, seg])) <= GJK_BAR["pair"], (u, seg, q)
    if name == "contact":
        for u, tr, i, k in cases:
            assert a["obs_index"][u] == i and a["obs_clearance"][u] <= GJK_BAR[k] and a["flags"][u] & pkg.AUDIT_FLAGS["obs_contact"]
    if name == "overlap":
        assert a["pair_clearance"][0] <= 1e-3 + 1e-15 and a["flags"][0] & a["flags"][1] & pkg.AUDIT_FLAGS["pair_contact"]
    slv.close()


def test_frontier_overflow_is_an_error_and_leaves_everything_usable(pkg, scenes):
    """SCN-B (20 000 points = 2 500 leaf boxes > FRONT_CAP = 1 024) at range 100: every leaf is within range of every hull, the walk cannot hold them:
    TJ_ERR_CAPACITY -- never a smaller answer; the solver's own error bits, its state and the next audit are untouched, and the iterations
    after it are those of a solver that never audited.  One call."""
    scene = scenes.scn_b()
    slv = pkg.Solver(scene, stop=0.0); ref = pkg.Solver(scene, stop=0.0)
    slv.iterate(2); ref.iterate(2)
    before, st0 = slv.audit(per_segment=True), slv.get_state()
    with pytest.raises(pkg.TrajAdmmError) as ei:
        slv.audit(range=100.0)
    assert "-3" in str(ei.value) and "range" in str(ei.value)
    assert slv.stats()["error_bits"] == 0
    st1 = slv.get_state()
    for n in STATE:
        assert np.array_equal(st0[n], st1[n]), n
    after = slv.audit(per_segment=True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    slv.iterate(2); ref.iterate(2)
    sa, sb = slv.get_state(), ref.get_state()
    for n in STATE:
        assert np.array_equal(sa[n], sb[n]), n
    slv.close(); ref.close()


def test_replaced_obstacle_set(pkg, scenes):
    """audit, tj_set_cloud with a permuted shorter cloud, audit: the caller-index table belongs to the obstacle set and goes with it; then tj_set_mesh"""
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    st = slv.get_state()
    first = slv.audit(range=1.0)
    perm = np.random.default_rng(8).permutation(600)[:437]
    cloud2 = np.ascontiguousarray(scene["cloud"][perm])
    slv._check(slv.lib.tj_set_cloud(slv._ctx, cloud2.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(437)))
    scene2 = dict(scene, cloud=cloud2)
    fresh = pkg.Solver(scene2, stop=0.0); fresh.set_state(st)
    a, b = slv.audit(range=1.0, per_segment=True), fresh.audit(range=1.0, per_segment=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for u in range(slv.U):   # a robot whose nearest point was kept meets it again under its new index
        if first["obs_index"][u] >= 0 and first["obs_index"][u] in perm:
            assert a["obs_index"][u] >= 0 and perm[a["obs_index"][u]] == first["obs_index"][u] and a["obs_clearance"][u] == first["obs_clearance"][u], u
    H = hulls_of(pkg, st["spline"], 5, 8)
    check_records(a, brute_obs(prims(), H, cloud2, 1.0, prefilter=False), "obs", 1.0)
    fresh.close()
    tris = scenes.triangulate(scene2)["tris"][::-1][:300]
    verts = np.ascontiguousarray(tris, dtype=np.float64).reshape(-1, 3)
    faces = np.arange(900, dtype=np.int32).reshape(-1, 3)
    slv._check(slv.lib.tj_set_mesh(slv._ctx, verts.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(900), faces.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(300)))
    a = slv.audit(range=1.0, per_segment=True)
    check_records(a, brute_obs(prims(), H, np.ascontiguousarray(tris), 1.0, prefilter=False), "obs", 1.0)
    slv.close()


@pytest.mark.parametrize("name", ["tiny_multi_optplane", "tiny_single_optplane", "hard_coupled"])
def test_other_modes_on_one_context(pkg, scenes, name):
    """optimal_plane = 1 (multi and single UAV) and the coupled mode (one shared piece_time) on ONE context, initial state and after 3 iterations"""
    from conftest import scene_by_name
    if name == "hard_coupled":
        scene, caps = scene_by_name(scenes, name), {}
    else:
        scene, caps = scene_by_name(scenes, name[:-len("_optplane")]), dict(optimal_plane=1)
    slv = pkg.Solver(scene, stop=0.0, **caps)
    multi = scene["mode"] != 0
    for it in (0, 3):
        if it:
            slv.iterate(it)
        a = check_clearances(pkg, slv, scene, None if it else 1.0, multi=multi)
        check_limits(pkg, slv, a)
    if name == "hard_coupled":
        assert len(set(slv.get_state()["piece_time"])) == 1
    slv.close()


def test_range_corner_values(pkg, scenes):
    """range below offset: a robot with nothing within range reports range, -1 and NO contact (a contact names what is in contact), a robot with a
    primitive within that range still reports it; +infinity == any range beyond the largest distance; NaN == the default"""
    F = pkg.AUDIT_FLAGS
    scene, st, H = R.range_corner_scene(pkg, scenes)
    cloud = scene["cloud"]
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)   # the very state the hulls above were formed from
    a = slv.audit(range=0.05, per_segment=True)
    check_records(a, brute_obs(prims(), H, cloud, 0.05, prefilter=False), "obs", 0.05)
    assert a["obs_index"][1] == 123 and a["obs_clearance"][1] < 0.05 and a["flags"][1] & F["obs_contact"]
    for u in (0, 2):
        assert (a["obs_clearance"][u], a["obs_index"][u], a["obs_segment"][u]) == (0.05, -1, -1) and not a["flags"][u] & F["obs_contact"]
    assert np.all(a["pair_clearance"] == 0.05) and np.all(a["pair_robot"] == -1) and not np.any(a["flags"] & F["pair_contact"])
    x, y = slv.audit(range=100.0, per_segment=True), slv.audit(range=float("inf"), per_segment=True)
    for k in x:
        assert np.array_equal(x[k], y[k]), k
    x, y = slv.audit(range=None, per_segment=True), slv.audit(range=float("nan"), per_segment=True)
    for k in x:
        assert np.array_equal(x[k], y[k]), k
    slv.close()
    empty = pkg.Solver(dict(scenes.tiny(mode=0), cloud=np.zeros((0, 3))), stop=0.0)   # no obstacle, no other robot: +inf reports `range` itself
    a = empty.audit(range=float("inf"), per_segment=True)
    assert a["obs_clearance"][0] == np.inf == a["pair_clearance"][0] and (a["obs_index"][0], a["obs_segment"][0], a["pair_robot"][0]) == (-1, -1, -1)
    assert np.all(a["seg_obs"] == np.inf) and np.all(a["seg_pair"] == np.inf) and a["flags"][0] & 3 == 0 and np.isfinite(a["speed"][0])
    empty.close()


def parse_audit_lines(stdout):
    """'audit uav U obs X seg N id N pair X seg N uav N speed X seg N accel X seg N time X flags N' -> list of dicts in the record's names"""
    names = ("obs_clearance", "obs_segment", "obs_index", "pair_clearance", "pair_segment", "pair_robot", "speed", "speed_segment", "accel",
             "accel_segment", "duration", "flags")
    out = []
    for line in stdout.split("\n"):
        if line.startswith("audit uav "):
            w = line.split()
            assert len(w) == 27 and int(w[2]) == len(out), line
            out.append({n: (float if n in ("obs_clearance", "pair_clearance", "speed", "accel", "duration") else int)(w[4 + 2 * k]) for k, n in enumerate(names)})
    return out


@pytest.mark.parametrize("multi", [False, True])
def test_command_line_audit(pkg, scenes, tmp_path, multi):
    """--audit and --audit 1.0 on both mains (and through a two-rank group on the multi-UAV one): every printed field equals the library's audit
    of the dumped state -- doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly"""
    import torch
    scene = scenes.tiny(mode=1) if multi else scenes.tiny(0, n_points=3000)
    cli = CliCase(pkg, scenes, tmp_path, scene, "multiPathPlanning3D" if multi else "admmPathPlanning3D")
    two = ["--gpus", "2"] if torch.cuda.device_count() >= 2 else ["--devices", "0,0"]   # two ranks either way: tj_group_audit
    dumps = []
    for audit_args, rng in ((["--audit"], None), (["--audit", "1.0"], 1.0)):
        for extra in ([], two) if multi else ([],):
            lines = cli.run(audit_args + extra)
            got = parse_audit_lines("\n".join(lines))
            assert len(got) == scene["U"], lines[-40:]
            dumps.append(open(tmp_path / "state.txt").read())
            cli.load()
            a = cli.slv.audit(range=rng)
            for u, rec in enumerate(got):
                for n, v in rec.items():
                    if isinstance(v, int):
                        assert v == a[n][u], (audit_args, extra, u, n, v, a[n][u])
                    else:
                        assert close_to_six_digits(v, a[n][u]), (audit_args, extra, u, n, v, a[n][u])
            if not multi:
                assert all(rec["pair_robot"] == -1 and rec["pair_clearance"] == (DEFAULT_RANGE if rng is None else rng) for rec in got)
    assert len(set(dumps)) == 1                                # the audit and the group change nothing of the run
    cli.close()
