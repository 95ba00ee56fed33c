"""GPU (-m gpu): tj_audit_timed -- the bracket of every robot's closest approach to another robot at EQUAL FLIGHT TIMES.

Expected values come from tests/audit_timed_ref.py: the numpy restatement of the header's definition (windows enumerated in Python floats, blossoming
elementwise, the oracle's GJK against the origin).  Records and per-segment rows are compared with == on the doubles, the bar tests/test_gpu_audit.py
holds: same inputs, same expressions, no FMA contraction on either side.  The restatement itself is held against the flown curves on the CPU
(tests/test_audit_timed_ref.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import audit_ref as R
import audit_timed_ref as T
from audit_ref import prims
from conftest import ROOT
from query_kit import CliCase, assert_group_equals, assert_only_adds, assert_read_only, close_to_six_digits, group_pair, one_queue, raw_context

pytestmark = pytest.mark.gpu
DEFAULT_RANGE = 0.1 + 2 * 0.1


def check(pkg, slv, rng=None, levels=None, st=None):
    """device records and rows == the restatement on the state the solver holds; returns the device's answer"""
    p = slv.params
    r = p["offset"] + 2 * p["margin"] if rng is None else rng
    L = pkg.AUDIT_TIMED_LEVELS if levels is None else levels
    a = slv.audit_timed(range=rng, levels=levels, per_segment=True)
    st = slv.get_state() if st is None else st
    rec, rows = T.restated(pkg, prims(), st, slv.P, slv.res, r, p["offset"], L)
    assert np.array_equal(a["seg_lo"], rows["lo"]), (rng, levels, np.abs(a["seg_lo"] - rows["lo"]).max())
    assert np.array_equal(a["seg_hi"], rows["hi"]), (rng, levels, np.abs(a["seg_hi"] - rows["hi"]).max())
    for n in rec:
        assert np.array_equal(a[n], rec[n]), (rng, levels, n, a[n], rec[n])
    return a


def test_default_level_is_the_headers(pkg):
    lib = pkg.load_library()
    assert lib.tj_audit_timed_record_size() == C.sizeof(pkg.TjAuditTimedRobot) == 48
    hdr = open(os.path.join(ROOT, "include", "trajadmm.h")).read()
    assert "#define TJ_AUDIT_TIMED_LEVELS %d\n" % pkg.AUDIT_TIMED_LEVELS in hdr


@pytest.mark.parametrize("name", ["hard", "tiny"])
def test_equals_restatement_along_a_run(pkg, scenes, name):
    """initial state and after a few iterations (decoupled: every robot its own piece_time), levels 0, default and 6, default range and 1.0"""
    scene = scenes.hard() if name == "hard" else scenes.tiny(mode=1)
    slv = pkg.Solver(scene, stop=0.0)
    for it in (0, 4):
        if it:
            slv.iterate(it)
            assert name != "hard" or len(set(slv.get_state()["piece_time"])) > 1   # (tiny()'s three robots keep one value: the equal-time path)
        st = slv.get_state()
        for levels in (0, None, 6):
            for rng in (None, 1.0):
                check(pkg, slv, rng, levels, st)
    a = slv.audit_timed(levels=2)
    assert np.all(a["levels"] == 2)
    slv.close()


def test_triangle_scene_and_single_uav(pkg, scenes):
    scene = scenes.triangulate(scenes.tiny(mode=1))
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    check(pkg, slv, 1.0, None)
    check(pkg, slv, None, 3)
    slv.close()
    one = pkg.Solver(scenes.tiny(mode=0), stop=0.0)
    one.iterate(2)
    for rng, r in ((None, DEFAULT_RANGE), (0.05, 0.05)):
        a = one.audit_timed(range=rng, per_segment=True)
        assert (a["timed_lo"][0], a["timed_hi"][0], a["timed_robot"][0], a["timed_segment"][0], a["lo_robot"][0], a["lo_segment"][0]) == (r, r, -1, -1, -1, -1)
        assert a["flags"][0] == pkg.AUDIT_TIMED_FLAGS["clear"] and np.all(a["seg_lo"] == r) and np.all(a["seg_hi"] == r)
    one.close()


def test_chase_is_contact_where_the_same_segment_audit_is_clean(pkg, scenes):
    """(a) two robots on one line, the rear one twice as fast: tj_audit sees no pair within range (same-segment hulls 1.69 apart), tj_audit_timed
    reports contact on both, at a time inside the one sub-window that holds the meeting time"""
    scene, st, t_meet, t_goal = T.chase_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    old = slv.audit()
    assert not np.any(old["flags"] & pkg.AUDIT_FLAGS["pair_contact"]) and np.all(old["pair_robot"] == -1)
    for levels in (None, 0, 3, 6):
        a = check(pkg, slv, None, levels, st)
        L = pkg.AUDIT_TIMED_LEVELS if levels is None else levels
        assert np.all(a["flags"] == pkg.AUDIT_TIMED_FLAGS["contact"]), a["flags"]
        assert (a["timed_robot"][0], a["timed_robot"][1]) == (1, 0)
        for u in (0, 1):
            width = st["piece_time"][u] / 8 / (1 << L)       # one sub-window of robot u, in time
            ks = [np.floor(t / width) for t in ((t_meet,) if u == 0 else (t_meet, t_goal))]   # robot 1 also passes robot 0's goal while robot 0 hovers there (chase_state)
            assert any(k * width <= a["timed_time"][u] <= (k + 1) * width for k in ks), (levels, u, a["timed_time"][u])
            # the separation changes at 1.25 per unit of time at both contacts (2.5 against 1.25; 1.25 against the hovering robot): the nearer end of the window that
            # holds a zero is at most half a window's travel away
            assert a["timed_hi"][u] <= 1.25 * width / 2 + T.slack(32, st["spline"]), (u, a["timed_hi"][u])
    slv.close()


def test_crossing_is_clear_where_the_same_segment_audit_reports_contact(pkg, scenes):
    """(b) paths cross at right angles, the robots pass the crossing 2 apart in time: tj_audit reports PAIR_CONTACT (the hulls of segment 15 touch),
    tj_audit_timed certifies separation at the default level; with the whole space in range the bracket holds sqrt(5); (d) a range below offset
    with nothing near reports range, -1 and neither contact nor clearance"""
    scene, st = T.crossing_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    old = slv.audit()
    assert np.all(old["flags"] & pkg.AUDIT_FLAGS["pair_contact"])
    a = check(pkg, slv, None, None, st)
    assert np.all(a["flags"] == pkg.AUDIT_TIMED_FLAGS["clear"]) and np.all(a["timed_robot"] == -1) and np.all(a["timed_lo"] == DEFAULT_RANGE)
    a = check(pkg, slv, float("inf"), None, st)
    assert np.all(a["flags"] == pkg.AUDIT_TIMED_FLAGS["clear"])
    assert a["timed_lo"][0] <= np.sqrt(5.0) + 1e-12 and a["timed_hi"][0] >= np.sqrt(5.0) - 1e-12 and a["timed_hi"][0] - a["timed_lo"][0] < 0.05
    a = check(pkg, slv, 0.05, None, st)
    assert np.all(a["timed_lo"] == 0.05) and np.all(a["timed_hi"] == 0.05) and np.all(a["timed_robot"] == -1) and np.all(a["lo_robot"] == -1) and np.all(a["flags"] == 0)
    slv.close()


def test_contact_with_a_robot_that_has_arrived(pkg, scenes):
    """(c) robot 0 arrives at t = 2 and hovers; robot 1 flies through its goal at t = 3.6: contact on robot 1, attained against the hover body (a time
    beyond robot 0's duration); robot 0's own flight never comes near"""
    scene, st, t_meet = T.hover_state(pkg, scenes)
    slv = pkg.Solver(scene, stop=0.0)
    slv.set_state(st)
    for levels in (None, 6):
        a = check(pkg, slv, None, levels, st)
        assert a["flags"][1] == pkg.AUDIT_TIMED_FLAGS["contact"] and a["timed_robot"][1] == 0 and a["timed_segment"][1] == 14
        assert a["timed_time"][1] > 4 * st["piece_time"][0] and abs(a["timed_time"][1] - t_meet) <= st["piece_time"][1] / 8
        assert a["flags"][0] == pkg.AUDIT_TIMED_FLAGS["clear"] and a["timed_robot"][0] == -1
    a = check(pkg, slv, None, 0, st)
    assert a["flags"][1] == 0 and a["timed_lo"][1] <= 0.1 < a["timed_hi"][1]   # level 0: undecided -- the case the header sends to a higher level
    slv.close()


@pytest.mark.parametrize("U", [64, 65, 130])
def test_fleet_sizes_beyond_one_partner_pass(pkg, scenes, U):
    """partner passes of 64 >> level robots: U = 64, 65, 130 at levels 0 (64 per pass), default and 6 (one per pass)"""
    scene = scenes.crossing(U, 600, seed=5)
    slv = pkg.Solver(scene, stop=0.0)
    slv.iterate(3)
    st = slv.get_state()
    for levels in (0, None) + ((6,) if U == 65 else ()):
        check(pkg, slv, None, levels, st)
    slv.close()


@pytest.mark.parametrize("P,res", [(12, 8), (3, 16), (2, 16)])
def test_segment_counts_and_resolutions(pkg, scenes, P, res):
    scene = dict(scenes.hard(4, 3000, pieces=P))
    params = {"res": res}
    slv = pkg.Solver(scene, params, stop=0.0)
    st = R.port_state(scene, 3, params)
    assert R.valid_state(st, 4)
    slv.set_state(st)
    for levels in (None, 4):
        check(pkg, slv, None, levels, st)
    check(pkg, slv, 1.0, 0, st)
    slv.close()


@pytest.mark.parametrize("queues", ["default", "one"])
def test_audit_timed_is_read_only(pkg, scenes, monkeypatch, queues):
    if queues == "one":
        one_queue(monkeypatch)
    assert_read_only(pkg, scenes.hard(), lambda s: s.audit_timed(range=1.0, levels=6, per_segment=True),
                     lambda s: (s.audit_timed(), s.audit_timed(range=1.0, levels=0)))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("ranks", [2, 3])
def test_group_equals_one_context(pkg, scenes, mode, ranks):
    scene = dict(scenes.hard(), mode=mode)
    one, grp = group_pair(pkg, scene, ranks)
    assert_group_equals(one, grp, lambda s, rng, levels: s.audit_timed(range=rng, levels=levels, per_segment=True), ((None, None), (1.0, 4)))
    grp.close(); one.close()
    half = pkg.Solver(scene, stop=0.0, rank=1, world=2)   # a plain sharded context does not hold the other ranks' piece_time: it says so
    with pytest.raises(pkg.TrajAdmmError) as ei:
        half.audit_timed()
    assert "-5" in str(ei.value) and "tj_group_audit_timed" in str(ei.value)
    half.audit()                                           # and stays usable
    half.close()


def test_bad_arguments(pkg, scenes):
    with raw_context(pkg, scenes) as (lib, ctx, init):
        rec = (pkg.TjAuditTimedRobot * 3)()
        call = lambda r, l, out=rec: lib.tj_audit_timed(ctx, C.c_double(r), C.c_int(l), out, None, None)
        assert call(0.0, -1) == -1                                   # before tj_init_state
        init()
        assert call(0.0, 7) == -1 and call(float("nan"), -1) == -1 and call(0.0, -1, None) == -1
        assert lib.tj_audit_timed(None, C.c_double(0.0), C.c_int(-1), rec, None, None) == -1
        assert call(0.0, -1) == 0 and all(r.levels == pkg.AUDIT_TIMED_LEVELS for r in rec)   # still usable; no obstacles set: valid
        assert call(0.0, 6) == 0 and all(r.levels == 6 for r in rec)


def parse_timed_lines(stdout):
    """'audit-timed uav U lo X uav N seg N hi X uav N seg N time X levels N flags N' -> list of dicts in the record's names"""
    names = ("timed_lo", "lo_robot", "lo_segment", "timed_hi", "timed_robot", "timed_segment", "timed_time", "levels", "flags")
    out = []
    for line in stdout.split("\n"):
        if line.startswith("audit-timed uav "):
            w = line.split()
            assert len(w) == 21 and int(w[2]) == len(out), line
            out.append({n: (float if n in ("timed_lo", "timed_hi", "timed_time") else int)(w[4 + 2 * k]) for k, n in enumerate(names)})
    return out


def test_command_line(pkg, scenes, tmp_path):
    """--audit-timed and --audit-timed 4 on the multi-UAV main (one context and a two-rank group): every printed field equals the library's answer on
    the dumped state -- doubles to 6 significant digits (the CLI read the scene through the x0.2 / x5 file round trip), integers exactly; the lines come
    after the --audit lines, and without the flag the output is what it was (every line but the wall-clock ones)"""
    cli = CliCase(pkg, scenes, tmp_path)
    audited = cli.run(["--audit"])
    for args, levels in ((["--audit-timed"], None), (["--audit-timed", "4"], 4)):
        for extra, lines in cli.queried(["--audit"] + args, "audit-timed ", against=audited):   # everything else is the --audit run's output
            got = parse_timed_lines("\n".join(lines))
            assert len(got) == cli.scene["U"]
            first = min(i for i, l in enumerate(lines) if l.startswith("audit-timed "))
            assert all(not l.startswith("audit uav ") for l in lines[first:])   # after the --audit lines
            a = cli.slv.audit_timed(levels=levels)
            for u, rec in enumerate(got):
                for n, v in rec.items():
                    if isinstance(v, int):
                        assert v == a[n][u], (args, extra, u, n, v, a[n][u])
                    else:
                        assert close_to_six_digits(v, a[n][u]), (args, extra, u, n, v, a[n][u])
    assert_only_adds(audited, "audit uav ", cli.plain)
    assert_only_adds(cli.run(["--audit-timed"]), "audit-timed ", cli.plain)
    cli.close()
