"""GPU (-m gpu): tj_peak_dynamics -- the flown curve's peak speed, acceleration and jerk, its path length and its time_scale.

Expected values come from tests/peak_dynamics_ref.py: the Python restatement of the header's definition (audit_ref's hulls, the blossoming for every degree, the
level-synchronous maximising search and the length tree written out).  Every field of every record is compared with == on doubles and ints, `windows` and
`depth` included.  The restatement itself is held against mpmath on the CPU (tests/test_peak_dynamics_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import audit_ref as R
import peak_dynamics_ref as D
from query_kit import CliCase, assert_group_equals, assert_read_only, close_to_six_digits, group_pair, raw_context

pytestmark = pytest.mark.gpu


def ref_for(pkg, slv, st=None):
    return D.Ref(pkg, slv.get_state() if st is None else st, slv.P, slv.res)


def check(pkg, slv, ref, tol=None, max_depth=None, max_windows=None, levels=None, owned=None, call=None):
    """device records == the restatement `ref` (built on the state the solver holds); returns the device's answer"""
    p = slv.params
    a = (call or slv.peak_dynamics)(tol=tol, max_depth=max_depth, max_windows=max_windows, length_levels=levels)
    rec = ref.records(pkg.PEAK_TOL if tol is None else tol, D.MAX_DEPTH if max_depth is None else max_depth, pkg.PEAK_FRONTIER if max_windows is None else max_windows,
                      pkg.PEAK_LENGTH_LEVELS if levels is None else levels, p["vel_limit"], p["acc_limit"], owned=owned)
    assert set(a) == set(D.FIELDS)
    for n in D.FIELDS:
        assert np.array_equal(a[n], rec[n]), (tol, max_depth, max_windows, levels, n, a[n], rec[n])
    return a


def test_record_size(pkg):
    assert pkg.load_library().tj_dynamics_record_size() == C.sizeof(pkg.TjDynamicsRobot) == 160 and C.sizeof(pkg.TjPeak) == 40


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """initial state and after a few iterations; tol in {default, 1e-3, 0}, max_depth in {default, 0, 3}, length_levels in {default, 0, 3, 7}"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 3 if name == "hard" else 4):
        if it:
            slv.iterate(it)
        ref = ref_for(pkg, slv)
        for tol in (None, 1e-3, 0.0):
            check(pkg, slv, ref, tol)
        for depth in (0, 3):
            check(pkg, slv, ref, None, depth)
        for levels in (0, 3, 7):   # 7: 128 windows per segment, more than one wave
            check(pkg, slv, ref, 1e-3, None, None, levels)
        check(pkg, slv, ref, 0.0, 3, None, 0)
    slv.close()


def test_depth_zero_against_audit(pkg, scenes):
    """max_depth = 0: speed.hi / accel.hi are tj_audit's speed / accel bit for bit.  The record's segment is the ATTAINED sample's (the lower end), tj_audit's the
    hull maximum's: they are compared wherever the restatement says the two coincide (the attained sample lies in the first segment of the largest ub)"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    same = 0
    for it in (0, 4):
        if it:
            slv.iterate(it)
        a, au, ref = slv.peak_dynamics(max_depth=0), slv.audit(), ref_for(pkg, slv)
        assert np.array_equal(a["speed_hi"], au["speed"]) and np.array_equal(a["accel_hi"], au["accel"]) and np.array_equal(a["duration"], au["duration"])
        assert np.all(a["speed_depth"] == 0) and np.all(a["accel_depth"] == 0)
        for u in range(slv.U):
            for q, n in ((0, "speed"), (1, "accel")):
                ub = ref.evaluate(u, q, np.arange(ref.S), np.zeros(ref.S), np.ones(ref.S))[0]
                assert int(np.argmax(ub)) == au[n + "_segment"][u]
                attained = ref.search(u, q, 0.0, 0, 1 << 20)["segment"]
                assert a[n + "_segment"][u] == attained                    # every robot: the device's segment is the restatement's attained one
                if int(np.argmax(ub)) == attained:
                    assert a[n + "_segment"][u] == au[n + "_segment"][u]
                    same += 1
    assert same > 0
    slv.close()


@pytest.mark.parametrize("P,res", [(12, 8), (2, 16)])
def test_segment_counts_and_resolutions(pkg, scenes, P, res):
    """(12, 8): 96 seeds per robot, more than one wave"""
    scene = dict(scenes.hard(4, 3000, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    ref = ref_for(pkg, slv, st)
    check(pkg, slv, ref)
    check(pkg, slv, ref, 0.0, None, None, 7)
    check(pkg, slv, ref, None, 2, 2)
    slv.close()


def test_fleet_of_65(pkg, scenes):
    scene = scenes.crossing(65, 500)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    ref = ref_for(pkg, slv)
    check(pkg, slv, ref)
    check(pkg, slv, ref, 1e-3, 3, None, 0)
    slv.close()


def test_truncation(pkg, scenes):
    """max_windows in {1, 2} on hard() after 4 iterations; and on the 96-seed state (12 pieces) a cap one below the largest number of live seeds any search of
    the restatement holds: exactly the searches with more live seeds overflow AT SEEDING (depth 0, windows == the seed count, the seeds' own bracket), the
    others run on.  Everything == the restatement under the same cap, the TRUNCATED bit included"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(4)
    ref = ref_for(pkg, slv)
    seen = 0
    for mw in (1, 2):
        a = check(pkg, slv, ref, None, None, mw)
        seen += sum(int(np.sum(a[q + "_flags"] & D.TRUNCATED != 0)) for q in D.QUANTITIES)
    assert seen > 0
    slv.close()
    scene = dict(scenes.hard(4, 3000, pieces=12))
    slv = pkg.Solver(scene, stop=0.0)
    st = R.port_state(scene, 3)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    ref = ref_for(pkg, slv, st)
    live0 = live_seeds(ref, slv.U)
    cap = max(live0.values()) - 1
    assert 1 <= cap < slv.S == 96                                            # a cap below the seed count that some search overflows at seeding
    a = check(pkg, slv, ref, None, None, cap)
    for (u, q), n in live0.items():
        name = D.QUANTITIES[q]
        if n > cap:
            assert a[name + "_flags"][u] & D.TRUNCATED and a[name + "_depth"][u] == 0 and a[name + "_windows"][u] == slv.S, (u, name, n, cap)
            assert a[name + "_hi"][u] == ref.search(u, q, 0.0, 0, 1 << 20)["hi"]       # the seeds' own bracket
        else:
            assert a[name + "_windows"][u] > slv.S or n == 0 or a[name + "_flags"][u] & D.CONVERGED, (u, name, n, cap)
    slv.close()


def live_seeds(ref, U):
    """(robot, quantity) -> the number of live seeds of the restatement's search"""
    out = {}
    for u in range(U):
        for q in range(3):
            tr = []
            ref.search(u, q, 0.0, 0, 1 << 20, tr)
            out[(u, q)] = tr[0][3]
    return out


def test_constructed_states(pkg, scenes):
    """a straight flight at constant speed: every segment ties -> segment 0 at time 0, nothing live at depth 0, CONVERGED; all control points equal: every value
    0, time_scale 0, CONVERGED, no NaN; a net scaled to reach the speed limit and one just under it: each sets exactly its own flags"""
    F = pkg.PEAK_DYN_FLAGS
    scene, st = D.line_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    a = check(pkg, slv, ref_for(pkg, slv, st))
    assert a["speed_segment"][0] == 0 and a["speed_time"][0] == 0.0 and a["speed_depth"][0] == 0 and a["speed_windows"][0] == slv.S
    assert a["speed_flags"][0] == D.CONVERGED and a["speed_lo"][0] == a["speed_hi"][0] > 0 and a["accel_hi"][0] == 0.0 and a["jerk_hi"][0] == 0.0
    scene, st = D.hover_state(pkg, scenes)
    slv.set_state(st)
    a = check(pkg, slv, ref_for(pkg, slv, st))
    for n in D.FIELDS:
        assert np.all(np.isfinite(a[n])), n
    for q in D.QUANTITIES:
        assert a[q + "_lo"][0] == a[q + "_hi"][0] == 0.0 and a[q + "_flags"][0] == D.CONVERGED
    assert a["time_scale"][0] == 0.0 and a["flags"][0] == F["speed_ok"] | F["accel_ok"]
    slv.close()
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    st = R.port_state(scene, 3)
    vel = slv.params["vel_limit"]
    r0 = D.Ref(pkg, st, slv.P, slv.res).search(0, 0, 1e-12, D.MAX_DEPTH, 1 << 20)
    for k, want, wanted_not in ((1.02 * vel / r0["lo"], F["speed"], F["speed_ok"]), (0.98 * vel / r0["hi"], F["speed_ok"], F["speed"])):
        st2 = D.scaled_state(st, 0, k)
        slv.set_state(st2)
        a = check(pkg, slv, ref_for(pkg, slv, st2))
        assert a["flags"][0] & want and not a["flags"][0] & wanted_not, (k, a["flags"][0], a["speed_lo"][0], a["speed_hi"][0])
        if a["flags"][0] & F["speed"]:
            assert a["time_scale"][0] >= 1.0
    slv.close()


def test_peak_dynamics_is_read_only(pkg, scenes):
    assert_read_only(pkg, scenes.hard(), lambda s: s.peak_dynamics(tol=0.0),
                     lambda s: (s.peak_dynamics(), s.peak_dynamics(max_depth=2, max_windows=1, length_levels=7)))


def test_interleaved_with_the_other_queries(pkg, scenes):
    """peak_dynamics between audit, obstacle_approach and flight_profile on one context, in both orders: each returns what it returned first"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    calls = dict(peak=lambda: slv.peak_dynamics(), audit=lambda: slv.audit(), obstacle=lambda: slv.obstacle_approach(), profile=lambda: slv.flight_profile(samples=9))
    first = {n: f() for n, f in calls.items()}
    for order in (("peak", "audit", "peak", "obstacle", "peak", "profile", "peak"), ("profile", "peak", "obstacle", "peak", "audit", "peak")):
        for n in order:
            got = calls[n]()
            for k in first[n]:
                assert np.array_equal(got[k], first[n][k], equal_nan=True), (order, n, k)
    slv.close()


@pytest.mark.parametrize("mode,ranks", [(1, 1), (1, 2), (1, 3), (2, 2)])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    assert_group_equals(one, grp, lambda s, tol, levels: s.peak_dynamics(tol=tol, length_levels=levels), ((None, None), (0.0, 7)))
    grp.close(); one.close()


def test_sharded_context_answers_for_its_own_robots(pkg, scenes):
    scene = scenes.hard()
    one = pkg.Solver(scene, stop=0.0)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)
    x, y = one.peak_dynamics(), half.peak_dynamics()
    mine = y["speed_windows"] != 0
    assert 0 < mine.sum() < scene["U"]
    for k in x:
        assert np.array_equal(x[k][mine], y[k][mine]), k
        assert np.all(y[k][~mine] == 0), k
    check(pkg, half, ref_for(pkg, one), owned=[int(u) for u in np.flatnonzero(mine)])
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec = (pkg.TjDynamicsRobot * 3)()
        C.memset(rec, 0x5a, C.sizeof(rec))
        before = bytes(rec)
        call = lambda t, d, w, l, out=rec: lib.tj_peak_dynamics(ctx, C.c_double(t), C.c_int(d), C.c_int(w), C.c_int(l), out)
        assert call(-1.0, -1, 0, -1) == -1                                   # before tj_init_state
        init()
        assert call(float("nan"), -1, 0, -1) == -1 and call(-1.0, 41, 0, -1) == -1 and call(-1.0, -1, pkg.PEAK_FRONTIER + 1, -1) == -1 and call(-1.0, -1, 0, 13) == -1
        assert call(-1.0, -1, 0, -1, None) == -1
        assert bytes(rec) == before                                           # records untouched
        for args in ((-1.0, 40, pkg.PEAK_FRONTIER, 12), (0.0, 0, 1, 0), (-1.0, -1, 0, -1)):   # the limits themselves are valid
            assert call(*args) == 0
            assert rec[0].length_levels == (args[3] if args[3] >= 0 else pkg.PEAK_LENGTH_LEVELS) and rec[2].speed.windows >= 40


def test_command_line(pkg, scenes, tmp_path):
    """--peak-dynamics and --peak-dynamics 1e-6 (one context and a two-rank group): every printed field equals the library's answer on the dumped state -- doubles to
    6 significant digits (the CLI read the scene through the file round trip), integers exactly; the fleet line names the largest time_scale; other output unchanged"""
    cli = CliCase(pkg, scenes, tmp_path)
    for args, tol in ((["--peak-dynamics"], None), (["--peak-dynamics", "1e-6"], 1e-6)):
        for extra, lines in cli.queried(args, "dynamics "):
            words = [l.split() for l in lines if l.startswith("dynamics uav ")]
            assert len(words) == cli.scene["U"] and all(int(w[2]) == u for u, w in enumerate(words))
            a = cli.slv.peak_dynamics(tol=tol)
            for u, w in enumerate(words):
                at = {q: w.index(q) for q in ("speed", "accel", "jerk", "length")}
                for q in D.QUANTITIES:
                    f = dict(zip(w[at[q] + 1:at[q] + 15:2], w[at[q] + 2:at[q] + 15:2]))
                    for n, key in (("lo", "lo"), ("hi", "hi"), ("time", "time")):
                        assert close_to_six_digits(f[key], a[q + "_" + n][u], floor=1e-12), (args, extra, u, q, n, w)
                    assert int(f["seg"]) == a[q + "_segment"][u] and int(f["flags"]) == a[q + "_flags"][u]
                f = dict(zip(w[at["length"] + 1::2], w[at["length"] + 2::2]))
                for key, n in (("lo", "length_lo"), ("hi", "length_hi"), ("duration", "duration"), ("time_scale", "time_scale")):
                    assert close_to_six_digits(f[key], a[n][u]), (args, extra, u, n, w)
                assert int(f["levels"]) == a["length_levels"][u] and int(f["flags"]) == a["flags"][u]
            fleet = [l.split() for l in lines if l.startswith("dynamics fleet ")]
            assert len(fleet) == 1 and int(fleet[0][5]) == int(np.argmax(a["time_scale"])) and close_to_six_digits(fleet[0][3], a["time_scale"].max())
    cli.close()
