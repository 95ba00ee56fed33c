"""The Armijo search and its commit (k_linesearch; coupled: k_ls_coupled / k_ls_commit, csrc/kernels_ls.h) against a 60-digit truth: PRODUCT kernels only, through the stage
API -- set_state -> stage_planes() -> set_planes -> set_direction -> stage_steps -> stage_linesearch -> get_state / stats.  tests/ls_ref.py holds the truth (mpmath, on
tests/grad_ref.py's energy), the yardstick (the same search in plain fp64), the measured thresholds and the cases; tests/test_ls_ref.py shows on the CPU that the truth's
trial point is the one its own derivative belongs to, that the project's CPU port accepts the truth's candidate and commits the same bits, that the cases reach the slots
claimed here and that eight planted one-line faults are each caught.

Per case (a row of the shape table x an accepting slot, ls_ref.ROWS):
  (a) verdict   the accepted exponent -- recovered from the returned step by repeated multiplication from step0 (what stage_steps() returned, with the t > 0 guard), it must
                hit a value exactly -- is the truth's on every decidable robot; energy_evals rises by sum_u (2 + k_u); error_bits == 0, ls_helper_timeouts == 0.
  (b) commit    bit for bit: spline == x + s d in numpy fp64 (one product, one sum, unfused), piece_time == t0 + s t_dir, the step the repeated product; every other state
                array untouched; coupled: one step and one time for every robot.
  (c) energies  for the accepting slot and the one before it (where the truth says they are measurable) the device's threshold w*_k is recovered by bisection on the
                search wolfe (ls_ref.measure_threshold: at most 64 probes, each set_state -> begin -> set_direction -> stage_steps -> stage_linesearch; decoupled: through the LAST
                robot's record, the wolfe every robot is compared against), and 1e-4 s_k w*_k is the truth's E_-1 - E_k within K r_class (A_-1 + A_k) + 4 ulp(|E_-1|), K = 8.
The search wolfe in coupled mode: the device forms wolfe_c = -(sum of the robots' records + t_dir x the corner entry) in the CCD stage's finisher; set_direction zeroes the
corner entry, so robot 0's record carries -W and the others 0.

Shapes, each asserted from the plan record, the lists and the counters (not assumed):
  super8          two robots, default: ls_help == 8, sixteen candidates per super-round (slots 15 | 16: the hand-over to the next super-round)
  super4          TJ_LS_HELP=4
  team0           TJ_LS_HELP=1 and ls_hist == 0 (a search that accepts candidate 0 on every robot runs first; its returned steps are step0: ls_hist is written next to them):
                  round 0 in the team shape, then one-wave rounds from k_first = 1
  wave            TJ_LS_FAST=0: one-wave rounds only;  wave_hist: TJ_LS_HELP=1 after reset() (ls_hist == -1)
  giveup          TJ_LS_HELP_MUTE=1: helpers never post, ls_giveups rises, the one-wave rounds take over at k_first = kb + 2
  late            TJ_LS_HELP_LATE=15: helpers stage after the primary's commit
  bound           synthetic lists of 96 planes (robot 0: the largest the team shape holds at S = 24) and 97 (robot 1: one-wave rounds)
  P11big, P11     lsl_affine == 0, lsl_groups == 4 (shadow waves); P11big: robot 0 carries more planes than lsl_plane_cap (global-list path)
  P2, res1, res16, single (mode 0), coupled (one launch: lsc_wide == 1) and coupled_rounds (TJ_LSC_WIDE=0)
  narrow          the narrow first round (W = hist + 2: E(x) and the full step; slots 1 | 8 | 9: the full rounds that follow from k_first = 1).  It needs Ctl::ls_quiet >= 1,
                  which only the folded begins of iterate() raise and every begin stage zeroes: the context iterates ten steady iterations (every robot takes the full step),
                  then no begin stage runs -- the lists are set, the clamps' exponents stand.  That ls_quiet survives the stage calls is shown by a counter: under
                  TJ_LS_HELP_MUTE=1 robot 1 (team shape) backs off and ls_giveups does NOT rise (ls_quiet >= LS_QUIET_ITERS: the helpers stayed home); after one begin stage
                  the same search gives up.  Robot 0 carries 349 planes (>= 160, beyond the team shape) and is primed to ls_hist == 0 before every search.

Observed on MI355X: DESIGN.md, "The Armijo search against a high-precision truth" (TJ_PRINT_OBSERVED=1 prints the ratios of (c) per row and slot).
"""
import math
import os

import numpy as np
import pytest
from mpmath import mp, mpf

import grad_ref as G
import ls_ref as L
from query_kit import STATE

pytestmark = pytest.mark.gpu
SWITCHES = ("TJ_LS_HELP", "TJ_LS_FAST", "TJ_LS_HELP_MUTE", "TJ_LS_HELP_LATE", "TJ_LSC_WIDE")
CASES = [(r[0], slot) for r in L.ROWS for slot in r[3]]


def _obs(what, val):
    if os.environ.get("TJ_PRINT_OBSERVED"):
        print("OBSERVED linesearch", what, val)


# ---- contexts: those of one row at a time ---------------------------------------------------------------------------------------------------
_CTX = {"row": None, "ctx": {}}


def close_all():
    for s in _CTX["ctx"].values():
        s.close()
    _CTX["ctx"] = {}


def team_fits(S, M):
    """ls_team_units: the team shape holds a robot whose units' terms fit two hull buffers"""
    return ((5 * S + 63) // 64 + (4 * S + 63) // 64 + (6 * M + 63) // 64) * 64 <= 2 * S * 18


def context(pkg, scenes, name, inp):
    _, tag, env, _, lists, _ = L.row(name)
    sh = G.shape(tag)
    if _CTX["row"] != name:
        close_all()
        _CTX["row"] = name
    par = inp["par"]
    key = (par["vel_limit"], par["acc_limit"])
    if key not in _CTX["ctx"]:
        with pytest.MonkeyPatch.context() as mp_:
            for v in SWITCHES:
                mp_.delenv(v, raising=False)
            for k, v in env.items():
                mp_.setenv(k, v)
            s = pkg.Solver(G.scene_of(scenes, sh[1], sh[2], G.fleet(sh)), par, stop=0.0)
        plan = s.plan = pkg.plan_record(ctx=s._ctx)[1]
        assert (plan["P"], plan["res"], plan["mode"]) == (sh[2], sh[3], sh[1])
        assert (plan["lsl_affine"], plan["lsl_groups"]) == ((0, 4) if sh[2] == 11 else (1, 8)), (name, plan["lsl_affine"], plan["lsl_groups"])
        assert plan["ls_fast"] == (0 if name == "wave" else 1)
        assert plan["ls_help"] == (1 if sh[1] == 2 or name in ("wave", "team0", "wave_hist") else 4 if name == "super4" else 8), (name, plan["ls_help"])
        assert plan["ls_help_mute"] == (1 if name in ("giveup", "narrow") else 0) and plan["ls_help_late"] == (15 if name == "late" else 0)
        if sh[1] == 2:
            assert plan["lsc_wide"] == (0 if name == "coupled_rounds" else 1)
        if name == "narrow":      # ten iterations in which every robot takes the full step: the folded begins count Ctl::ls_quiet up to 9; no begin stage from here on
            s.set_state(inp["st"])
            s.iterate(10)
            a, b = read_steps(s)
            assert [L.exponent_of(float(x), float(min(p, q))) for x, p, q in zip(s.last_armijo_steps(), a, b)] == [0] * s.U
        _CTX["ctx"][key] = s
    s = _CTX["ctx"][key]
    M = inp["counts"].sum(axis=1)
    S = inp["P"] * inp["res"]
    if lists == "bound":
        assert team_fits(S, int(M[0])) and not team_fits(S, int(M[0]) + 1) and int(M[1]) == int(M[0]) + 1 <= s.plan["lsl_plane_cap"]
    elif lists == "big":
        assert s.plan["lsl_plane_cap"] == L.LSL_PLANE_CAP_P11 and M[0] > s.plan["lsl_plane_cap"] >= M[1]
    elif lists == "syn":      # robot 0: beyond the team shape and LS_NARROW_MIN_PLANES = 160, LDS resident; robot 1: the team shape
        assert 160 <= M[0] <= s.plan["lsl_plane_cap"] and not team_fits(S, int(M[0])) and team_fits(S, int(M[1]))
    else:      # every list LDS resident; the team shape holds every robot -- but at P = 11 (four groups: never) and res = 1 (S = 3: two hull buffers hold not even the limit units)
        assert M.max() <= s.plan["lsl_plane_cap"], (name, M)
        if sh[1] != 2 and sh[2] != 11:
            assert all(team_fits(S, int(m)) == (tag != "res1") for m in M), (name, M)
    return s


def records_dev(inp, records):
    """what set_direction takes for the wolfe records of a case (coupled: see the module text)"""
    return [-w for w in records] if inp["mode"] == 2 else list(records)


def read_steps(s):
    """(step_self, step_pos) as the clamps' exponents stand, without running the CCD stage"""
    import ctypes as C
    a, b = np.zeros(s.U), np.zeros(s.U)
    s._check(s.lib.tj_get_steps(s._ctx, a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)), None))
    return a, b


def stage(s, inp, records, free=False):
    """the whole staging of a case -> the CCD stage's (step_self, step_pos).  free (the narrow row): no begin stage -- it would zero Ctl::ls_quiet --, hence no plane and
    no CCD stage either: the lists are set, the clamps' exponents stand as the last iteration left them"""
    s.set_state(inp["st"])
    if not free:
        s.stage_planes()
    s.set_planes(inp["counts"], inp["planes"])
    return direct(s, inp, records, free=free)


def direct(s, inp, records, dirs=None, t_dirs=None, free=False):
    rec = records_dev(inp, records)
    if not free:
        s.run_stage("begin")      # zeroes the clamps' exponents and the replay's lists: the CCD stage runs once per begin
    for u in range(inp["U"]):
        s.set_direction(u, (dirs or inp["dirs"])[u], (t_dirs or inp["t_dirs"])[u], rec[u], inp["gn"][u])
    return read_steps(s) if free else s.stage_steps()


def search(s, c, records, prime=None):
    """one search on the staged context -> (steps, state after, rise of energy_evals).  prime: see ls_ref.ROWS"""
    inp, free = c["inp"], prime == "quiet"
    if prime == "reset":
        s.reset()
        stage(s, inp, records)
    elif prime in ("hist0", "quiet"):
        s.set_state(inp["st"])
        pd, pt, pw = L.prime_of(inp)
        a, b = direct(s, inp, pw, pd, pt, free=free)
        first = s.stage_linesearch()
        want = [L.guard(float(inp["st"]["piece_time"][u]), pt[u], float(min(a[u], b[u])))[0] for u in range(inp["U"])]
        assert list(first) == want, ("the priming search did not accept its first candidate", first, want)      # ls_hist is written next to the step: 0 now
    s.set_state(inp["st"])
    a, b = direct(s, inp, records, free=free)
    assert np.array_equal(a, c["steps"][0]) and np.array_equal(b, c["steps"][1])
    before = s.stats()["energy_evals"]
    steps = s.stage_linesearch()
    st = s.stats()
    assert st["error_bits"] == 0 and st["ls_helper_timeouts"] == 0
    return steps, s.get_state(), st["energy_evals"] - before


def exponents(c, steps):
    """per unit the exponent of the returned step (None: no value of the repeated product); coupled: every robot returned the same step"""
    out = []
    for un in c["units"]:
        assert all(steps[u] == steps[un.robots[0]] for u in un.robots)
        out.append(L.exponent_of(float(steps[un.robots[0]]), un.step0))
    return out


@pytest.mark.parametrize("name,slot", CASES)
def test_search_and_commit_against_the_truth(pkg, scenes, name, slot):
    ctx = {}

    def steps_of(inp):
        s = ctx["s"] = context(pkg, scenes, name, inp)
        a, b = stage(s, inp, inp["wolfe"] if inp["mode"] != 2 else [inp["wolfe"][0]] + [0.0] * (inp["U"] - 1), free=name == "narrow")
        if inp["mode"] != 2 and name != "narrow":      # (the port's coupled CCD step belongs to its own update_spline, not to the stage API; narrow: no CCD stage runs)
            assert np.array_equal(a, inp["port_steps"][0]) and np.array_equal(b, inp["port_steps"][1]), (name, slot, a, b, inp["port_steps"])
        return a, b

    c = L.case(pkg, scenes, name, slot, steps_of)
    s, inp, units = ctx["s"], c["inp"], c["units"]
    assert s is context(pkg, scenes, name, inp)
    prime = c["prime"]
    r = L.class_r(c)
    want = L.expected(c, r=r)
    giveups = s.stats()["ls_giveups"]
    steps, post, evals = search(s, c, c["records"], prime)
    # (a) the verdict
    ks = exponents(c, steps)
    n_und = 0
    for un, k, w in zip(units, ks, want):
        assert k is not None, (name, slot, un.robots, "the step is no repeated product of step0", float(steps[un.robots[0]]), un.step0)
        if w["decidable"]:
            assert k == w["k"], (name, slot, un.robots, k, w["k"], w["margins"][-1])
        else:
            n_und += 1
    assert ks[c["target"]] == slot and want[c["target"]]["decidable"]
    assert n_und == 0, (name, slot, "undecidable searches", n_und)      # (at most 5 % are allowed over a class: tests/test_ls_ref.py counts them; here: none)
    assert evals == sum((2 + k) * len(un.robots) for un, k in zip(units, ks)), (name, slot, evals, ks)
    if name == "narrow":      # helpers that never post, a robot in the team shape that backs off, and no give-up: the helpers stayed home, Ctl::ls_quiet >= 8 stands
        assert ks[1] > 0 and s.stats()["ls_giveups"] == giveups and c["target"] == 0
    if name == "giveup":      # (elsewhere a give-up is allowed -- a helper that is not resident in time on a shared GPU -- and changes no verdict)
        assert s.stats()["ls_giveups"] > giveups
    # (b) the commit, bit for bit
    for un, k in zip(units, ks):
        step = L.step_back(un.step0, k)
        for u, (net, t) in zip(un.robots, L.commit(un, step)):
            assert steps[u] == step
            assert np.array_equal(post["spline"][u].view(np.int64), net.view(np.int64)), (name, slot, u, np.abs(post["spline"][u] - net).max())
            assert post["piece_time"][u] == t, (name, slot, u, post["piece_time"][u], t)
    for n in STATE[1:5]:
        assert np.array_equal(post[n].view(np.int64), inp["st"][n].view(np.int64)), (name, slot, n)
    if inp["mode"] == 2:
        assert len(set(post["piece_time"].tolist())) == 1 and len(set(steps.tolist())) == 1
    # (c) the candidate energies, measured through the search wolfe
    un, ti = units[c["target"]], c["target"]
    seen = {}
    for k in (slot - 1, slot):
        if k < 0 or not L.measurable(un, k):
            continue

        def probe(w):
            rec = list(c["records"])
            rec[0 if inp["mode"] == 2 else -1] = w
            got = exponents(c, search(s, c, rec, prime)[0])[ti]
            return L.KCAP + 1 if got is None else got

        lo, hi, n = L.measure_threshold(probe, k, float(un.wstar(k)))
        s_k = L.step_back(un.step0, k)
        with mp.workdps(L.DPS):
            drop = un.truth_energy(-1) - un.truth_energy(k)
            err = float(abs(mpf(L.C1) * mpf(s_k) * mpf(lo) - drop))
            ulp = math.ulp(abs(float(un.truth_energy(-1))))
        bar = L.threshold_bar(un, k, r)
        assert n <= 64 and (hi == math.nextafter(lo, math.inf) or n == 64), (name, slot, k, "the bisection did not end", lo, hi, n)
        assert err <= bar, (name, slot, k, err, bar, err / bar, (hi - lo) * L.C1 * s_k / ulp)
        seen[k] = float("%.2g" % (err / (r * (un.yard_energy(None, None)[1] + un.yard_energy(s_k, s_k)[1]))))
    assert slot in seen
    _obs((name, slot), dict(cls=inp["cls"], target=ti, ks=ks, ratio_to_r=seen, r_class_u=float("%.3g" % (r / L.U64)), step0=[un.step0 for un in units],
                            guard=[un.guarded for un in units], giveups=s.stats()["ls_giveups"] - giveups, inf=[sum(1 for m in w["margins"] if m[1] == math.inf) for w in want]))
    if (name, slot) == ("narrow", 9):      # the control: after a begin stage (ls_quiet = 0) the same search calls the helpers, who never post -- the same step, and a give-up
        s.run_stage("begin")
        again = search(s, c, c["records"], prime)[0]
        assert np.array_equal(again, steps) and s.stats()["ls_giveups"] > giveups
    if (name, slot) == CASES[-1]:
        close_all()
