"""GPU (-m gpu): tj_zone_windows -- during which time intervals every robot's flown curve is inside (or outside) a volume the caller names.

Expected values come from tests/zone_windows_ref.py: the Python restatement of the header's definition (audit_ref's hulls, peak_dynamics_ref's blossoming, the
two gauges with their bounds, the classification OUT / IN / MIXED per sense, dynamics_windows_ref's search per (robot, zone) over the whole flight, the merge of
the leaves into rows, the row order).  Every field of every row is compared with == on doubles and ints, `windows`, `depth`, `leaves` and `face` included, and so
is the number of rows.  The restatement itself is held against the polynomials' real roots on the CPU (tests/test_zone_windows_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import audit_ref as R
import zone_windows_ref as Z
from query_kit import CliCase, assert_group_equals, assert_read_only, close_to_six_digits, group_pair, loaded, one_queue, raw_context

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


def ref_for(pkg, slv, st=None):
    return Z.Ref(pkg, slv.get_state() if st is None else st, slv.P, slv.res)


def check(pkg, slv, ref, zones, tol=None, max_depth=None, max_windows=None, owned=None):
    """device rows == the restatement `ref` (built on the state the solver holds); returns the device's answer"""
    p = slv.params
    a = slv.zone_windows(zones, tol=tol, max_depth=max_depth, max_windows=max_windows)
    exp = ref.rows(zones, Z.default_tol(p["offset"], p["vel_limit"]) if tol is None else tol, Z.MAX_DEPTH if max_depth is None else max_depth,
                   pkg.ZONEWIN_FRONTIER if max_windows is None else max_windows, owned=owned)
    assert set(a) == set(Z.FIELDS)
    for n in ("robot", "zone") + Z.FIELDS:
        assert np.array_equal(a[n], exp[n]), (tol, max_depth, max_windows, n, a[n], exp[n])
    key = list(zip(a["robot"], a["zone"], a["t_first_lo"]))
    assert key == sorted(key)
    return a


def full_set(pkg, ref, offset):
    """the measurement's 20 zones through the package's helpers (zone_planes / zone_ball), plus a one-face fence in both senses: 22 zones.  The prism has 32 faces"""
    out = []
    for kind, sense, level, rows in Z.measurement_zones(ref, offset):
        s = "inside" if sense == Z.INSIDE else "outside"
        out.append(pkg.zone_planes(rows, s, level) if kind == Z.PLANES else pkg.zone_ball(rows[0][:3], rows[0][3], s, level))
    mid = ref.H.reshape(-1, 3).mean(axis=0)
    fence = [[0.6, 0.8, 0.0, 0.6 * mid[0] + 0.8 * mid[1]]]
    assert max(len(z[3]) for z in out) == pkg.ZONEWIN_MAX_PLANES
    return out + [pkg.zone_planes(fence, "inside", 0.0), pkg.zone_planes(fence, "outside", -offset)]


def test_row_size(pkg):
    assert pkg.load_library().tj_zonewin_row_size() == C.sizeof(pkg.TjZonewinRow) == 96 and C.sizeof(pkg.TjZone) == 24


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """after 0, 1 and 3 iterations: the full zone set (boxes, a band, the 32-face prism, a ball, a 1-face fence, both senses, two levels), and the same with
    tol = 0 and max_depth = 3: the depth stop and the EDGE leaves"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    rows = edges = 0
    for it in (0, 1, 2):   # (iterations 0, 1 and 3 of the run)
        if it:
            slv.iterate(it)
        ref = ref_for(pkg, slv)
        zones = full_set(pkg, ref, slv.params["offset"])
        a = check(pkg, slv, ref, zones)
        rows += len(a["robot"])
        assert set(a["face"][a["zone"] >= 16][a["zone"][a["zone"] >= 16] < 20]) <= {-1}      # the ball's rows carry face -1
        a = check(pkg, slv, ref, zones, 0.0, 3)
        edges += int(np.sum((a["depth"] == 3) & (a["flags"] & pkg.ZONEWIN_FLAGS["resolved"] == 0)))
    assert rows > 0 and edges > 0
    slv.close()


def test_ball_centred_on_the_curve(pkg, scenes):
    """a ball whose centre is a point of robot 1's curve (a hull end point): the windows around it have the centre inside their hull, the lb = 0 - r branch, which
    is asserted on the restatement; both senses, and r = 0"""
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(1)
    ref = ref_for(pkg, slv)
    c = ref.H[1][7][5]
    tr = np.array([7, 8])
    ub, lb, _, _ = ref.bounds(1, (Z.BALL, Z.INSIDE, 0.0, np.array([[c[0], c[1], c[2], 0.25]])), tr, np.array([0.5, 0.0]), np.array([1.0, 0.5]))
    assert np.all(lb == -0.25) and np.all(ub > -0.25)
    zones = [pkg.zone_ball(c, 0.25), pkg.zone_ball(c, 0.25, "outside"), pkg.zone_ball(c, 0.0), pkg.zone_ball(c, 0.0, "outside"), pkg.zone_ball(c, 0.25, "inside", -0.1)]
    a = check(pkg, slv, ref, zones)
    assert {0, 1, 3} <= set(a["zone"][a["robot"] == 1]) and np.all(a["face"] == -1)
    check(pkg, slv, ref, zones, 0.0, 6)
    slv.close()


def _wide_state(pkg, scenes, P, res):
    scene = dict(scenes.hard(4, 3000, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    return slv, st


def test_seeds_wider_than_a_wave_and_placement_past_leaf_64(pkg, scenes):
    """P = 12, res = 8: 96 seeds per search.  A box that holds the whole flight: 96 IN seeds, one chain across leaf 64, depth 0, within_lo = the flight.  And a
    ball, found and asserted on the restatement so that the case cannot stop reaching the path, whose OUTSIDE splits a flight into two or more rows of more
    than 64 leaves together with a chain head in the second block of 64"""
    slv, st = _wide_state(pkg, scenes, 12, 8)
    assert slv.S == 96
    ref = ref_for(pkg, slv, st)
    F = pkg.ZONEWIN_FLAGS
    pts = ref.H.reshape(-1, 3)
    a = check(pkg, slv, ref, [pkg.zone_box(pts.min(axis=0) - 1.0, pts.max(axis=0) + 1.0)])
    assert len(a["robot"]) == slv.U and np.all(a["leaves"] == 96) and np.all(a["depth"] == 0) and np.all(a["windows"] == 96)
    assert np.all(a["flags"] == F["certain"] | F["at_start"] | F["at_end"] | F["resolved"]) and np.all(a["segment_last"] == 95)
    assert np.all(np.abs(a["within_lo"] - a["t_last_hi"]) <= 1e-12 * a["t_last_hi"]) and np.all(a["t_first_lo"] == 0.0)
    diag = float(np.sqrt(((pts.max(axis=0) - pts.min(axis=0)) ** 2).sum()))
    found = None
    for u in range(ref.U):
        for seg, frac in ((seg, f) for seg in (72, 80, 88) for f in (0.02, 0.05, 0.1, 0.2)):
            zone = pkg.zone_ball(ref.H[u][seg][0], frac * diag, "outside")
            lv = ref.search(u, zone, Z.OUTSIDE, 0.0, 0.0, 8, pkg.ZONEWIN_FRONTIER)["leaves"]
            heads = [i for i in range(1, len(lv)) if lv[i - 1][1] != lv[i][0]]
            if len(lv) > 64 and any(i > 64 for i in heads) and lv[63][1] == lv[64][0] and found is None:
                found = (u, zone, len(heads) + 1)
    assert found is not None
    u, zone, n_rows = found
    a = check(pkg, slv, ref, [zone], 0.0, 8)
    assert int(np.sum(a["robot"] == u)) == n_rows >= 2
    slv.close()


def test_two_pieces_at_res_16(pkg, scenes):
    slv, st = _wide_state(pkg, scenes, 2, 16)
    ref = ref_for(pkg, slv, st)
    assert len(check(pkg, slv, ref, full_set(pkg, ref, slv.params["offset"]))["robot"]) > 0
    slv.close()


def test_slots_wider_than_a_wave(pkg, scenes):
    """65 robots x 1 zone in which only robots 0, 31, 32 and 64 have rows (their nets moved by 150 along x into a box no other robot reaches): the scan of the row
    counts crosses one wave, most slots contribute nothing.  And 9 robots x 8 zones: 72 slots"""
    scene = scenes.crossing(65, 120)
    slv = pkg.Solver(scene, stop=0.0)
    st = {n: np.array(v) for n, v in slv.get_state().items()}
    who = (0, 31, 32, 64)
    assert np.abs(st["spline"]).max() < 50.0
    for u in who:
        st["spline"][u][0] += 150.0
    slv.set_state(st)
    ref = ref_for(pkg, slv, st)
    a = check(pkg, slv, ref, [pkg.zone_box([100.0, -1e3, -1e3], [200.0, 1e3, 1e3])])
    assert sorted(set(a["robot"])) == list(who) and len(a["robot"]) == 4
    slv.close()
    scene = scenes.crossing(9, 120)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(1)
    ref = ref_for(pkg, slv)
    a = check(pkg, slv, ref, full_set(pkg, ref, slv.params["offset"])[:8])
    assert len(set(zip(a["robot"], a["zone"]))) > 9
    slv.close()


def test_truncation_and_capacity(pkg, scenes):
    """a zone and a max_windows, chosen on the restatement, at which one slot truncates and the others do not: TRUNCATED rows == the restatement's last completed
    round; cap below *n: TJ_ERR_CAPACITY, the exact *n and the first cap rows; the count-only call returns the same *n; n_zones == 0: no row"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    ref = ref_for(pkg, slv)
    F = pkg.ZONEWIN_FLAGS
    zones = full_set(pkg, ref, slv.params["offset"])
    tol = Z.default_tol(slv.params["offset"], slv.params["vel_limit"])
    pick = None
    for z in zones:
        for mw in (1, 2, 3, 4, 6):
            r = ref.rows([z], tol, Z.MAX_DEPTH, mw)
            cut = set(r["robot"][r["flags"] & Z.TRUNCATED != 0])
            if len(cut) == 1 and len(set(r["robot"])) > 1 and pick is None:
                pick = (z, mw)
    assert pick is not None
    a = check(pkg, slv, ref, [pick[0]], None, None, pick[1])
    assert len(set(a["robot"][a["flags"] & F["truncated"] != 0])) == 1 and np.sum(a["flags"] & F["truncated"] == 0) > 0
    check(pkg, slv, ref, zones, None, None, 1)
    full = check(pkg, slv, ref, zones)
    n = len(full["robot"])
    assert n > 2
    arr, table = pkg.zonewin_pack(zones)

    def call(rec, cap, nz=len(zones)):
        got = C.c_int(-7)
        return slv.lib.tj_zone_windows(slv._ctx, arr, C.c_int(nz), table.ctypes.data_as(_dp), C.c_int(len(table)), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rec,
                                       C.c_int(cap), C.byref(got)), got.value

    assert call(None, 0) == (0, n)
    rec = (pkg.TjZonewinRow * (n + 3))()
    for k in range(n):
        rec[k].robot, rec[k].extreme = -99, 123.5
    assert call(rec, 2) == (-3, n)
    assert (rec[2].robot, rec[2].extreme) == (-99, 123.5)                                   # the sentinel behind the first cap rows is untouched
    assert all(getattr(rec[k], f) == full[f][k] for k in range(2) for f in Z.FIELDS)
    assert call(rec, n) == (0, n) and all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in Z.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n + 3) == (0, n)                            # a smaller call after a larger one, and back
    rec[0].robot = -99
    assert call(rec, n, 0) == (0, 0) and call(None, 0, 0) == (0, 0) and rec[0].robot == -99
    e = slv.zone_windows([])
    assert set(e) == set(Z.FIELDS) and all(len(e[f]) == 0 for f in Z.FIELDS)
    slv.close()


def test_gauge_equal_to_the_level(pkg, scenes):
    """stated limit (2): robot 0 of tiny() set to fly at the constant altitude 1.5, and altitude bands one of whose planes is z = 1.5, both senses, and a level that
    puts the other plane there: no error, == the restatement, whatever it is"""
    scene = scenes.tiny(mode=1)
    st = R.port_state(scene, 1)
    st["spline"][0][2] = 1.5
    slv = loaded(pkg, scene, st)
    ref = ref_for(pkg, slv, st)
    assert np.all(ref.H[0][:, :, 2] == 1.5)
    top = [[0.0, 0.0, -1.0, -1.25], [0.0, 0.0, 1.0, 1.5]]
    bottom = [[0.0, 0.0, -1.0, -1.5], [0.0, 0.0, 1.0, 1.75]]
    zones = [pkg.zone_planes(rows, s, level) for rows in (top, bottom) for s in ("inside", "outside") for level in (0.0, -0.25)]
    a = check(pkg, slv, ref, zones)
    assert 0 in set(a["robot"])
    check(pkg, slv, ref, zones, 0.0, 5)
    check(pkg, slv, ref, zones, None, None, 2)
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_zone_windows_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    zones = [pkg.zone_box([-1.0, -1.0, 0.0], [1.0, 1.0, 2.0]), pkg.zone_ball([0.0, 0.0, 1.0], 1.5, "outside"), pkg.zone_planes([[0.0, 0.0, 1.0, 1.0]], "inside", -0.1)]
    assert_read_only(pkg, scenes.hard(), lambda s: s.zone_windows(zones, tol=0.0, max_depth=4),
                     lambda s: (s.zone_windows(zones), s.zone_windows(zones, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
def test_group_equals_one_context(pkg, scenes, mode):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, 2)
    ref = ref_for(pkg, one)
    zones = full_set(pkg, ref, one.params["offset"])
    x = assert_group_equals(one, grp, lambda s, tol: s.zone_windows(zones, tol=tol, max_depth=6), ((None,), (0.0,)))
    n = len(x["robot"])
    assert n > 2
    arr, table = pkg.zonewin_pack(zones)
    rec, got = (pkg.TjZonewinRow * n)(), C.c_int(0)                                         # a cap that ends inside the rows: the exact total, the first rows
    rc = grp.lib.tj_group_zone_windows(grp._g, arr, C.c_int(len(zones)), table.ctypes.data_as(_dp), C.c_int(len(table)), C.c_double(0.0), C.c_int(6), C.c_int(0), rec,
                                       C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in Z.FIELDS)
    grp.close(); one.close()


def test_sharded_context_answers_for_its_own_robots(pkg, scenes):
    scene = scenes.hard()
    one = pkg.Solver(scene, stop=0.0)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)
    ref = ref_for(pkg, one)
    zones = full_set(pkg, ref, one.params["offset"])
    x, y = one.zone_windows(zones), half.zone_windows(zones)
    mine = sorted(set(y["robot"]))
    assert 0 < len(mine) < scene["U"] and mine == list(range(mine[0], mine[-1] + 1))
    keep = np.isin(x["robot"], mine)
    for k in x:
        assert np.array_equal(x[k][keep], y[k]), k
    check(pkg, half, ref, zones, owned=[int(u) for u in mine])
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    """the precedence: null, then NaN / non-finite, then limits, then no state; the outputs stay untouched"""
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjZonewinRow * 12)(), C.c_int(-7)
        rec[0].robot = -99
        nan, inf = float("nan"), float("inf")
        box = pkg.zone_box([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])

        def packed(*zones):
            arr, table = pkg.zonewin_pack(list(zones))
            return arr, len(zones), table, len(table)

        ok = packed(box)

        def call(z, t, depth, w, out=rec, cap=12, n=C.byref(got)):
            arr, nz, table, ns = z
            rc = lib.tj_zone_windows(ctx, arr, C.c_int(nz), None if table is None else table.ctypes.data_as(_dp), C.c_int(ns), C.c_double(t), C.c_int(depth), C.c_int(w), out,
                                     C.c_int(cap), n)
            if rc == -1:
                assert (got.value, rec[0].robot) == (-7, -99)                                  # the outputs are untouched
            return rc, lib.tj_last_error(ctx)

        def raw(kind, sense, first, count, rows, level=0.0):
            arr = (pkg.TjZone * 1)(pkg.TjZone(level, kind, sense, first, count))
            table = np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 4))
            return arr, 1, table, len(table)

        rc, msg = call(ok, -1.0, -1, 0)                                                        # before tj_init_state
        assert rc == -1 and b"tj_init_state" in msg
        rc, msg = call(packed(pkg.zone_box([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], level=nan)), -1.0, 41, 0)   # non-finite before the limits, the limits before the missing state
        assert rc == -1 and b"level" in msg
        rc, msg = call(packed(pkg.zone_ball([0.0, inf, 0.0], 1.0)), -1.0, 41, 0)
        assert rc == -1 and b"shape table" in msg
        assert call(packed(pkg.zone_ball([0.0, 0.0, 0.0], 1.0, level=-inf)), -1.0, -1, 0)[0] == -1 and call(packed(pkg.zone_planes([[0.0, 0.0, 1.0, nan]])), -1.0, -1, 0)[0] == -1
        rc, msg = call(ok, nan, 41, 0)
        assert rc == -1 and b"NaN" in msg
        rc, msg = call(ok, -1.0, 41, 0)
        assert rc == -1 and b"max_depth" in msg
        one = [1.0, 0.0, 0.0, 1.0]
        for bad, word in ((raw(2, 0, 0, 1, one), b"kind"), (raw(-1, 0, 0, 1, one), b"kind"), (raw(0, 2, 0, 1, one), b"sense"), (raw(0, -1, 0, 1, one), b"sense"),
                          (raw(0, 0, 0, 0, one), b"count"), (raw(0, 0, 0, 33, [one] * 33), b"count"), (raw(1, 0, 0, 2, [one] * 2), b"count"),
                          (raw(0, 0, 1, 1, one), b"shape table"), (raw(0, 0, -1, 1, one), b"shape table"), (raw(0, 0, 0, 2, one), b"shape table"),
                          (raw(0, 0, 0x7fffffff, 2, one), b"shape table"), (raw(0, 0, 0, 1, [0.0, 0.0, 0.0, 1.0]), b"all-zero"), (raw(1, 0, 0, 1, [0.0, 0.0, 0.0, -1.0]), b"radius")):
            rc, msg = call(bad, -1.0, -1, 0)
            assert rc == -1 and word in msg, (word, msg)
        rc, msg = call(packed(*[box] * (pkg.ZONEWIN_MAX_ZONES + 1)), -1.0, -1, 0)
        assert rc == -1 and b"n_zones" in msg
        assert call(ok, -1.0, -1, 0, n=None)[0] == -1 and call(ok, -1.0, -1, 0, cap=-1)[0] == -1 and call(ok, -1.0, -1, 0, out=None)[0] == -1
        assert call((None, 1, ok[2], ok[3]), -1.0, -1, 0)[0] == -1 and call((ok[0], -1, ok[2], ok[3]), -1.0, -1, 0)[0] == -1
        assert call((ok[0], 1, None, 6), -1.0, -1, 0)[0] == -1 and call((ok[0], 1, ok[2], -1), -1.0, -1, 0)[0] == -1
        init()
        assert call(packed(pkg.zone_ball([0.0, 0.0, 0.0], 1.0, level=nan)), -1.0, -1, 0)[0] == -1 and call(ok, nan, -1, 0)[0] == -1 and call(ok, -1.0, 41, 0)[0] == -1
        assert call(ok, -1.0, -1, pkg.ZONEWIN_MAX_WINDOWS + 1)[0] == -1 and call(raw(1, 0, 0, 1, [0.0, 0.0, 0.0, -1.0]), -1.0, -1, 0)[0] == -1
        rc, msg = call(ok, -1.0, -1, pkg.ZONEWIN_MAX_WINDOWS, cap=1 << 25)                     # refused up front, nothing allocated
        assert rc == -1 and b"TJ_ZONEWIN_MAX_BYTES" in msg
        far = packed(pkg.zone_ball([1e3, 1e3, 1e3], 0.0), pkg.zone_planes([[1.0, 0.0, 0.0, -1e3]]))
        for args in ((far, -1.0, 40, pkg.ZONEWIN_MAX_WINDOWS), (far, 0.0, -1, 0), ((None, 0, None, 0), -1.0, 0, 1), ((ok[0], 0, ok[2], ok[3]), -1.0, 0, 1)):   # the limits themselves are valid
            got.value = -7
            assert call(*args)[0] == 0 and got.value == 0 and rec[0].robot == -99
        got.value = -7
        everywhere = pkg.zone_planes([[0.0, 0.0, 1.0, 1e3]] * pkg.ZONEWIN_MAX_PLANES)
        assert call(packed(*[everywhere] * pkg.ZONEWIN_MAX_ZONES), -1.0, -1, 0, out=None, cap=0)[0] == 0 and got.value == 3 * pkg.ZONEWIN_MAX_ZONES


def test_command_line(pkg, scenes, tmp_path):
    """--zone-windows -0.05 --zone-box .. --zone-outside --zone-ball .. (one context and a two-rank group): the printed rows are the library's on the dumped state
    for the box INSIDE and the ball OUTSIDE at level -0.05, in its order -- doubles to 6 significant digits, integers exactly -- and the fleet's line counts them"""
    cli = CliCase(pkg, scenes, tmp_path)
    pts = Z.Ref(pkg, cli.slv.get_state(), cli.slv.P, cli.slv.res).H.reshape(-1, 3)
    lo, hi, mean = pts.min(axis=0), pts.max(axis=0), pts.mean(axis=0)
    box = [float("%.6g" % v) for v in list(lo + (hi - lo) / 3) + list(hi - (hi - lo) / 3)]
    ball = [float("%.6g" % v) for v in list(mean) + [0.25 * float(np.sqrt(((hi - lo) ** 2).sum()))]]
    doubles = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "extreme", "extreme_time")
    ints = ("robot", "zone", "sense", "face", "segment_first", "segment_last", "leaves", "depth", "windows", "flags")
    args = ["--zone-windows", "-0.05", "--zone-box"] + [repr(v) for v in box] + ["--zone-outside", "--zone-ball"] + [repr(v) for v in ball]
    for extra, lines in cli.queried(args, "zonewin "):
        got = [l.split() for l in lines if l.startswith("zonewin uav ")]
        a = cli.slv.zone_windows([pkg.zone_box(box[:3], box[3:], "inside", -0.05), pkg.zone_ball(ball[:3], ball[3], "outside", -0.05)])
        assert len(got) == len(a["robot"]) > 0 and all(len(w) == 32 for w in got) and set(a["zone"]) == {0, 1}
        for k, w in enumerate(got):
            for n, i in zip(doubles, (10, 11, 13, 14, 16, 18, 20)):
                assert close_to_six_digits(w[i], a[n][k], 1e-9), (extra, k, n, w)
            assert [int(w[i]) for i in (2, 4, 6, 8, 22, 23, 25, 27, 29, 31)] == [a[n][k] for n in ints], (extra, k, w)
        fleet = [l.split() for l in lines if l.startswith("zonewin fleet ")]
        assert len(fleet) == 1 and int(fleet[0][3]) == 2 and int(fleet[0][5]) == len(a["robot"])
    cli.close()
