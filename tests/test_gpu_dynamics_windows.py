"""GPU (-m gpu): tj_dynamics_windows -- during which time intervals every robot's flown curve is over (or under) a level of speed, acceleration or jerk.

Expected values come from tests/dynamics_windows_ref.py: the Python restatement of the header's definition (peak_dynamics_ref's hulls, raw derivative nets and
blossoming, the bounds ub and lb, the classification OUT / IN / MIXED per sense, one search per (robot, gate) over the whole flight, the merge of the leaves
into rows, the row order).  Every field of every row is compared with == on doubles and ints, `windows`, `depth` and `leaves` included, and so is the number of
rows.  The restatement itself is held against the polynomial's real roots on the CPU (tests/test_dynamics_windows_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import audit_ref as R
import dynamics_windows_ref as W
from query_kit import CliCase, assert_group_equals, assert_read_only, close_to_six_digits, group_pair, loaded, one_queue, raw_context

pytestmark = pytest.mark.gpu
INF = float("inf")


def ref_for(pkg, slv, st=None):
    return W.Ref(pkg, slv.get_state() if st is None else st, slv.P, slv.res)


def check(pkg, slv, ref, gates=None, tol=None, max_depth=None, max_windows=None, owned=None):
    """device rows == the restatement `ref` (built on the state the solver holds); returns the device's answer"""
    p = slv.params
    a = slv.dynamics_windows(gates=gates, tol=tol, max_depth=max_depth, max_windows=max_windows)
    exp = ref.rows(W.default_gates(p["vel_limit"], p["acc_limit"]) if gates is None else pkg.dynwin_gates(gates),
                   W.default_tol(p["vel_limit"], p["acc_limit"]) if tol is None else tol, W.MAX_DEPTH if max_depth is None else max_depth,
                   pkg.DYNWIN_FRONTIER if max_windows is None else max_windows, owned=owned)
    assert set(a) == set(W.FIELDS)
    for n in ("robot", "gate") + W.FIELDS:
        assert np.array_equal(a[n], exp[n]), (gates, tol, max_depth, max_windows, n, a[n], exp[n])
    key = list(zip(a["robot"], a["gate"], a["t_first_lo"]))
    assert key == sorted(key)
    return a


def run_gates(slv, ref):
    """the defaults plus 0.9 and 0.5 of each limit in both senses, plus a jerk gate at half the fleet's largest depth-0 bound: 11 gates"""
    v, a = slv.params["vel_limit"], slv.params["acc_limit"]
    jerk = 0.5 * max(ref.ub0(u, W.JERK) for u in range(ref.U))
    return ([("speed", "above", v), ("accel", "above", a)] +
            [(q, s, f * lim) for f in (0.9, 0.5) for q, lim in (("speed", v), ("accel", a)) for s in ("above", "below")] + [("jerk", "above", jerk)])


def test_row_size(pkg):
    assert pkg.load_library().tj_dynwin_row_size() == C.sizeof(pkg.TjDynwinRow) == 96 and C.sizeof(pkg.TjDynGate) == 16


@pytest.mark.parametrize("name", ["hard", "tiny", "tiny_coupled", "tiny_single"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """after 0, 1 and 3 iterations: the default gates (a null list), the 11 gates of run_gates, and those with tol = 0 and max_depth = 3: the depth stop and the
    EDGE leaves"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode={"tiny": 1, "tiny_coupled": 2, "tiny_single": 0}[name])
    slv = pkg.Solver(scene, stop=0.0)
    rows = edges = 0
    for it in (0, 1, 2):   # (iterations 0, 1 and 3 of the run)
        if it:
            slv.iterate(it)
        ref = ref_for(pkg, slv)
        gates = run_gates(slv, ref)
        check(pkg, slv, ref)
        rows += len(check(pkg, slv, ref, gates)["robot"])
        a = check(pkg, slv, ref, gates, 0.0, 3)
        edges += int(np.sum((a["depth"] == 3) & (a["flags"] & pkg.DYNWIN_FLAGS["resolved"] == 0)))
    assert rows > 0 and edges > 0
    slv.close()


def test_scaled_state_lists_exactly_that_robot(pkg, scenes):
    """tiny(mode=1) after 3 iterations with robot 1's net scaled so that it is over both limits: the default gates list robot 1 alone, under both gates; the side
    of the limit is asserted on the restatement"""
    scene = scenes.tiny(mode=1)
    st = R.port_state(scene, 3)
    slv = pkg.Solver(scene, stop=0.0)
    p = slv.params
    base = W.Ref(pkg, st, slv.P, slv.res)
    # (the largest attained end sample of a depth-4 search at level 0: a lower bound of the peak)
    peaks = lambda ref, q: [max(max(lf[5], lf[6]) for lf in ref.search(u, q, W.ABOVE, 0.0, 0.0, 4, 1024)["leaves"]) for u in range(ref.U)]
    k = 1.5 * max(p["vel_limit"] / peaks(base, W.SPEED)[1], p["acc_limit"] / peaks(base, W.ACCEL)[1], 1.0)
    st2 = W.scaled_state(st, 1, k)
    ref = W.Ref(pkg, st2, slv.P, slv.res)
    sp, ac = peaks(ref, W.SPEED), peaks(ref, W.ACCEL)
    assert sp[1] > p["vel_limit"] and ac[1] > p["acc_limit"]
    assert all(ref.ub0(u, W.SPEED) < p["vel_limit"] and ref.ub0(u, W.ACCEL) < p["acc_limit"] for u in range(ref.U) if u != 1)
    slv.set_state({**slv.get_state(), **st2})
    a = check(pkg, slv, ref)
    assert set(a["robot"]) == {1} and set(a["gate"]) == {0, 1} and np.all(a["flags"] & pkg.DYNWIN_FLAGS["certain"] != 0)
    assert np.all(a["extreme"][a["gate"] == 0] > p["vel_limit"]) and np.all(a["within_lo"] > 0)
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
    """P = 12, res = 8: 96 seeds per search.  ABOVE at level 0: 96 IN seeds, one chain across leaf 64, within_lo = the flight.  And a speed level, found and
    asserted on the restatement so that the case cannot stop reaching the path, that splits a flight into two or more rows of more than 64 leaves together with a
    chain head in the second block of 64"""
    slv, st = _wide_state(pkg, scenes, 12, 8)
    assert slv.S == 96
    ref = ref_for(pkg, slv, st)
    F = pkg.DYNWIN_FLAGS
    a = check(pkg, slv, ref, [("speed", "above", 0.0), ("jerk", "above", -1.0)])
    assert len(a["robot"]) == 2 * slv.U and np.all(a["leaves"] == 96) and np.all(a["depth"] == 0) and np.all(a["windows"] == 96)
    assert np.all(a["flags"] == F["certain"] | F["at_start"] | F["at_end"] | F["resolved"]) and np.all(a["segment_last"] == 95)
    found = None
    for u in range(ref.U):
        for q, sense, frac in ((q, s, f) for q in (W.SPEED, W.ACCEL) for s in (W.ABOVE, W.BELOW) for f in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3)):
            level = frac * ref.ub0(u, q)
            lv = ref.search(u, q, sense, level, 0.0, 8, pkg.DYNWIN_FRONTIER)["leaves"]
            heads = [i for i in range(1, len(lv)) if lv[i - 1][1] != lv[i][0]]
            if len(lv) > 64 and any(i > 64 for i in heads) and lv[63][1] == lv[64][0] and found is None:
                found = (u, q, sense, level, len(heads) + 1)
    assert found is not None
    u, q, sense, level, n_rows = found
    a = check(pkg, slv, ref, [(q, sense, level)], 0.0, 8)
    assert int(np.sum(a["robot"] == u)) == n_rows >= 2
    slv.close()


def test_two_pieces_at_res_16(pkg, scenes):
    slv, st = _wide_state(pkg, scenes, 2, 16)
    ref = ref_for(pkg, slv, st)
    check(pkg, slv, ref)
    assert len(check(pkg, slv, ref, run_gates(slv, ref))["robot"]) > 0
    slv.close()


def test_slots_wider_than_a_wave(pkg, scenes):
    """65 robots x 1 gate in which only robots 0, 31, 32 and 64 have rows (their nets scaled by 4, the level 1.5 x the others' largest depth-0 bound): the scan of
    the row counts crosses one wave, most slots contribute nothing.  And 9 robots x 8 gates: 72 slots"""
    scene = scenes.crossing(65, 120)
    slv = pkg.Solver(scene, stop=0.0)
    st = slv.get_state()
    who = (0, 31, 32, 64)
    level = 1.5 * max(ref_for(pkg, slv, st).ub0(u, W.SPEED) for u in range(slv.U))
    for u in who:
        st = W.scaled_state(st, u, 4.0)
    slv.set_state(st)
    ref = ref_for(pkg, slv, st)
    a = check(pkg, slv, ref, [("speed", "above", level)])
    assert sorted(set(a["robot"])) == list(who)
    slv.close()
    scene = scenes.crossing(9, 120)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(1)
    ref = ref_for(pkg, slv)
    a = check(pkg, slv, ref, run_gates(slv, ref)[2:10])
    assert len(set(zip(a["robot"], a["gate"]))) > 9
    slv.close()


def test_per_robot_piece_time(pkg, scenes):
    """a decoupled state with piece_time[u] scaled by 1 + 0.03 * u: every time and every den is formed with the robot's own piece_time"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(2)
    st = slv.get_state()
    st["piece_time"] = st["piece_time"] * (1 + 0.03 * np.arange(slv.U))
    slv.set_state(st)
    ref = ref_for(pkg, slv, st)
    a = check(pkg, slv, ref, run_gates(slv, ref))
    assert len(set(a["robot"])) > 1
    slv.close()


def test_truncation_and_capacity(pkg, scenes):
    """max_windows = 1 on a state with crossings: TRUNCATED rows == the restatement's last completed round, while the seeds are never truncated (at level 0 all
    S seeds are leaves under max_windows = 1); cap below *n: TJ_ERR_CAPACITY, the exact *n and the first cap rows; the count-only call returns the same *n"""
    scene = scenes.hard()
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    ref = ref_for(pkg, slv)
    F = pkg.DYNWIN_FLAGS
    gates = run_gates(slv, ref)[2:]
    a = check(pkg, slv, ref, gates, None, None, 1)
    assert np.sum(a["flags"] & F["truncated"] != 0) > 0
    b = check(pkg, slv, ref, [("speed", "above", 0.0)], None, None, 1)
    assert np.all(b["leaves"] == slv.S) and np.all(b["flags"] & F["truncated"] == 0)
    full = check(pkg, slv, ref, gates)
    n = len(full["robot"])
    assert n > 2
    gl = pkg.dynwin_gates(gates)
    arr = (pkg.TjDynGate * len(gl))(*[pkg.TjDynGate(level, q, s) for q, s, level in gl])

    def call(rec, cap):
        got = C.c_int(-7)
        return slv.lib.tj_dynamics_windows(slv._ctx, arr, C.c_int(len(gl)), C.c_double(-1.0), C.c_int(-1), C.c_int(0), rec, C.c_int(cap), C.byref(got)), got.value

    assert call(None, 0) == (0, n)
    rec = (pkg.TjDynwinRow * (n + 3))()
    for k in range(n):
        rec[k].robot, rec[k].extreme = -99, 123.5
    assert call(rec, 2) == (-3, n)
    assert (rec[2].robot, rec[2].extreme) == (-99, 123.5)                                   # the sentinel behind the first cap rows is untouched
    assert all(getattr(rec[k], f) == full[f][k] for k in range(2) for f in W.FIELDS)
    assert call(rec, n) == (0, n) and all(getattr(rec[k], f) == full[f][k] for k in range(n) for f in W.FIELDS)
    assert call(rec, 1) == (-3, n) and call(rec, n + 3) == (0, n)                            # a smaller call after a larger one, and back
    slv.close()


def test_quantity_equal_to_the_level_and_closed_forms(pkg, scenes):
    """stated limit (2): the constant-speed line with a gate at exactly its speed, both senses: no error, == the restatement.  The line ABOVE 0.75 x its speed: the
    whole flight; ABOVE 1.25 x: no row.  The hover BELOW 0.1: one row, the whole flight"""
    F = pkg.DYNWIN_FLAGS
    whole = F["certain"] | F["at_start"] | F["at_end"] | F["resolved"]
    scene, st = W.line_state(pkg, scenes)
    slv = loaded(pkg, scene, st)
    ref = ref_for(pkg, slv, st)
    v = W.line_speed(pkg, st, slv.P)
    check(pkg, slv, ref, [("speed", "above", v), ("speed", "below", v)])
    check(pkg, slv, ref, [("speed", "above", v), ("speed", "below", v)], 0.0, 5)
    a = check(pkg, slv, ref, [("speed", "above", 0.75 * v), ("speed", "above", 1.25 * v)])
    assert list(a["gate"]) == [0] and a["flags"][0] == whole and a["leaves"][0] == slv.S and a["extreme"][0] == v
    scene, st = W.hover_state(pkg, scenes)
    slv.set_state({**slv.get_state(), **st})
    a = check(pkg, slv, ref_for(pkg, slv, st), [("speed", "below", 0.1)])
    assert list(a["flags"]) == [whole] and a["extreme"][0] == 0.0 and abs(a["t_last_hi"][0] - a["within_lo"][0]) <= 1e-12 * a["t_last_hi"][0]
    slv.close()


def test_empty_list_null_list_and_unbounded_levels(pkg, scenes):
    """gates = [] is an empty list: no row; gates = None is the null list: the two default gates, equal to naming them.  +inf ABOVE: no row; +inf BELOW and a
    negative level ABOVE: the whole flight, one row per robot; a negative level BELOW: no row"""
    scene = scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(1)
    ref = ref_for(pkg, slv)
    p = slv.params
    e = slv.dynamics_windows(gates=[])
    assert set(e) == set(W.FIELDS) and all(len(e[f]) == 0 for f in W.FIELDS)
    x, y = check(pkg, slv, ref), check(pkg, slv, ref, [("speed", "above", p["vel_limit"]), ("accel", "above", p["acc_limit"])])
    assert all(np.array_equal(x[f], y[f]) for f in W.FIELDS)
    a = check(pkg, slv, ref, [("speed", "above", INF), ("accel", "below", INF), ("jerk", "above", -2.5), ("speed", "below", -1.0)])
    F = pkg.DYNWIN_FLAGS
    assert sorted(zip(a["robot"], a["gate"])) == [(u, k) for u in range(slv.U) for k in (1, 2)]
    assert np.all(a["flags"] == F["certain"] | F["at_start"] | F["at_end"] | F["resolved"]) and np.all(a["leaves"] == slv.S) and np.all(a["depth"] == 0)
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_dynamics_windows_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    six = [(q, s, 1.0) for q in ("speed", "accel", "jerk") for s in ("above", "below")]
    assert_read_only(pkg, scenes.hard(), lambda s: s.dynamics_windows(gates=six, tol=0.0, max_depth=4),
                     lambda s: (s.dynamics_windows(), s.dynamics_windows(gates=six, max_depth=2, max_windows=1)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    six = [(q, s, 1.0) for q in ("speed", "accel", "jerk") for s in ("above", "below")]
    x = assert_group_equals(one, grp, lambda s, gates, tol: s.dynamics_windows(gates=gates, tol=tol, max_depth=6), ((None, None), (six, None), (six, 0.0)))
    n = len(x["robot"])
    assert n > 2
    gl = pkg.dynwin_gates(six)
    arr = (pkg.TjDynGate * len(gl))(*[pkg.TjDynGate(level, q, s) for q, s, level in gl])
    rec, got = (pkg.TjDynwinRow * n)(), C.c_int(0)                                          # a cap that ends inside the rows: the exact total, the first rows
    rc = grp.lib.tj_group_dynamics_windows(grp._g, arr, C.c_int(len(gl)), C.c_double(0.0), C.c_int(6), C.c_int(0), rec, C.c_int(n - 2), C.byref(got))
    assert (rc, got.value) == (-3, n) and all(getattr(rec[k], f) == x[f][k] for k in range(n - 2) for f in W.FIELDS)
    grp.close(); one.close()


def test_sharded_context_answers_for_its_own_robots(pkg, scenes):
    scene = scenes.hard()
    one = pkg.Solver(scene, stop=0.0)
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)
    gates = [("speed", "above", 0.0), ("accel", "below", 1.0)]
    x, y = one.dynamics_windows(gates=gates), half.dynamics_windows(gates=gates)
    mine = sorted(set(y["robot"]))
    assert 0 < len(mine) < scene["U"] and mine == list(range(mine[0], mine[-1] + 1))
    keep = np.isin(x["robot"], mine)
    for k in x:
        assert np.array_equal(x[k][keep], y[k]), k
    check(pkg, half, ref_for(pkg, one), gates, owned=[int(u) for u in mine])
    half.close(); one.close()


def test_bad_arguments(pkg, scenes):
    """the precedence: null, then NaN, then limits, then no state; the outputs stay untouched"""
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec, got = (pkg.TjDynwinRow * 12)(), C.c_int(-7)
        rec[0].robot = -99
        nan = float("nan")

        def gate_list(*gates):
            return (pkg.TjDynGate * max(len(gates), 1))(*[pkg.TjDynGate(level, q, s) for q, s, level in gates]), len(gates)

        ok = gate_list((0, 0, 1.0))

        def call(gates, t, depth, w, out=rec, cap=12, n=C.byref(got)):
            rc = lib.tj_dynamics_windows(ctx, gates[0], C.c_int(gates[1]), C.c_double(t), C.c_int(depth), C.c_int(w), out, C.c_int(cap), n)
            if rc == -1:
                assert (got.value, rec[0].robot) == (-7, -99)                                  # the outputs are untouched
            return rc, lib.tj_last_error(ctx)

        rc, msg = call(ok, -1.0, -1, 0)                                                        # before tj_init_state
        assert rc == -1 and b"tj_init_state" in msg
        rc, msg = call(gate_list((0, 0, nan)), -1.0, 41, 0)                                    # NaN before the limits, the limits before the missing state
        assert rc == -1 and b"NaN" in msg
        rc, msg = call(ok, nan, 41, 0)
        assert rc == -1 and b"NaN" in msg
        rc, msg = call(ok, -1.0, 41, 0)
        assert rc == -1 and b"max_depth" in msg
        rc, msg = call(gate_list((3, 0, 1.0)), -1.0, -1, 0)
        assert rc == -1 and b"quantity" in msg
        assert call(gate_list((0, 2, 1.0)), -1.0, -1, 0)[0] == -1 and call(gate_list((-1, 0, 1.0)), -1.0, -1, 0)[0] == -1
        many = gate_list(*[(0, 0, 1.0)] * (pkg.DYNWIN_MAX_GATES + 1))
        rc, msg = call(many, -1.0, -1, 0)
        assert rc == -1 and b"n_gates" in msg
        assert call(ok, -1.0, -1, 0, n=None)[0] == -1 and call(ok, -1.0, -1, 0, cap=-1)[0] == -1 and call(ok, -1.0, -1, 0, out=None)[0] == -1
        assert call((None, 1), -1.0, -1, 0)[0] == -1 and call((ok[0], -1), -1.0, -1, 0)[0] == -1
        init()
        assert call(gate_list((0, 0, nan)), -1.0, -1, 0)[0] == -1 and call(ok, nan, -1, 0)[0] == -1 and call(ok, -1.0, 41, 0)[0] == -1
        assert call(ok, -1.0, -1, pkg.DYNWIN_MAX_WINDOWS + 1)[0] == -1
        rc, msg = call(ok, -1.0, -1, pkg.DYNWIN_MAX_WINDOWS, cap=1 << 25)                      # refused up front, nothing allocated
        assert rc == -1 and b"TJ_DYNWIN_MAX_BYTES" in msg
        for args in ((gate_list((0, 0, INF)), -1.0, 40, pkg.DYNWIN_MAX_WINDOWS), (gate_list((1, 1, -1.0)), 0.0, -1, 0), (gate_list(), -1.0, 0, 1)):   # the limits themselves are valid
            got.value = -7
            assert call(*args)[0] == 0 and got.value == 0 and rec[0].robot == -99
        got.value = -7
        assert call(gate_list(*[(0, 0, 0.0)] * pkg.DYNWIN_MAX_GATES), -1.0, -1, 0, out=None, cap=0)[0] == 0 and got.value == 3 * pkg.DYNWIN_MAX_GATES


def test_command_line(pkg, scenes, tmp_path):
    """--dynamics-windows 0.5 (one context and a two-rank group): the printed rows are the library's on the dumped state at the two default gates scaled by 0.5,
    in its order -- doubles to 6 significant digits, integers exactly -- and the fleet's line counts them"""
    cli = CliCase(pkg, scenes, tmp_path)
    doubles = ("t_first_lo", "t_first_hi", "t_last_lo", "t_last_hi", "within_lo", "extreme", "extreme_time")
    ints = ("robot", "gate", "quantity", "sense", "segment_first", "segment_last", "leaves", "depth", "windows", "flags")
    for extra, lines in cli.queried(["--dynamics-windows", "0.5"], "dynwin "):
        got = [l.split() for l in lines if l.startswith("dynwin uav ")]
        p = cli.slv.params
        a = cli.slv.dynamics_windows(gates=[("speed", "above", 0.5 * p["vel_limit"]), ("accel", "above", 0.5 * p["acc_limit"])])
        assert len(got) == len(a["robot"]) > 0 and all(len(w) == 32 for w in got)
        for k, w in enumerate(got):
            for n, i in zip(doubles, (10, 11, 13, 14, 16, 18, 20)):
                assert close_to_six_digits(w[i], a[n][k]), (extra, k, n, w)
            assert [int(w[i]) for i in (2, 4, 6, 8, 22, 23, 25, 27, 29, 31)] == [a[n][k] for n in ints], (extra, k, w)
        fleet = [l.split() for l in lines if l.startswith("dynwin fleet ")]
        assert len(fleet) == 1 and int(fleet[0][3]) == len(a["robot"])
    cli.close()
