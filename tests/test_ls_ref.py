"""CPU: tests/ls_ref.py checks itself -- the truth's trial point against the truth's own derivative, the project's CPU port inside the truth (verdict and committed
bits), the eight planted faults caught, and what the cases of tests/test_gpu_linesearch.py reach: every slot of the shape table, few undecidable comparisons, candidates at
+inf, the t > 0 guard in every mode and a CCD clamp."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import grad_ref as G
import ls_ref as L
from query_kit import STATE

ROWS = [r[0] for r in L.ROWS]


def port_steps(inp):
    return inp["port_steps"]


_CASES = {}


def case_of(pkg, scenes, name, slot):
    """(case, r_class, the truth's answer per unit)"""
    if (name, slot) not in _CASES:
        c = L.case(pkg, scenes, name, slot, port_steps)
        r = L.class_r(c)
        _CASES[name, slot] = (c, r, L.expected(c, r=r))
    return _CASES[name, slot]


def all_cases(pkg, scenes, rows=ROWS):
    return [case_of(pkg, scenes, name, slot) for name in rows for slot in L.row(name)[3]]


# ---- the restated trial point ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,slot", [("super8", 1), ("super8", 16), ("single", 8), ("coupled", 6)])
def test_truth_search_is_consistent_with_its_own_derivative(pkg, scenes, name, slot):
    """(E(x + s d, t + s t_dir) - E(x, t)) / s -> g . d as s -> 0 at 80 digits, g grad_ref's analytic gradient per piece: the restated trial point is the right one"""
    c, _, _ = case_of(pkg, scenes, name, slot)
    for un in c["units"]:
        with mp.workdps(80):
            gd, mag = mpf(0), mpf(0)
            for pr, d, td in zip(un.probs, un.dirs, un.t_dirs):
                for sp in range(pr["P"]):
                    g = G.piece_grad_hess(pr, sp, dps=80)[0]
                    for k in range(6):
                        for a in range(3):
                            term = g[3 * k + a] * mpf(float(d[a][3 * sp + k]))
                            gd += term; mag += abs(term)
                    gd += g[18] * mpf(td); mag += abs(g[18] * mpf(td))
            e0 = un._energy(G._M, None, None)
            for s in (mpf("1e-30"), mpf("1e-33")):
                q = (un._energy(G._M, s, s) - e0) / s
                assert abs(q - gd) <= mpf("1e-20") * mag, (name, slot, un.robots, float(q), float(gd))
            assert mag > 0


# ---- what the cases reach -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_cases_reach_their_slots(pkg, scenes, name):
    """every slot of the row has a case whose truth accepts it on the target, decidably; the slot and -- where there is one -- the slot before it are measurable; at most 5 %
    of the comparisons of the row are undecidable; at least two cases reject a candidate at +inf before they accept"""
    slots = L.row(name)[3]
    n_cmp = n_und = n_inf = 0
    for slot in slots:
        c, r, want = case_of(pkg, scenes, name, slot)
        t = c["target"]
        assert want[t]["k"] == slot and want[t]["decidable"], (name, slot, want[t]["k"], want[t]["margins"][-1])
        assert L.measurable(c["units"][t], slot) and (slot == 0 or not math.isfinite(float(c["units"][t].wstar(slot - 1))) or L.measurable(c["units"][t], slot - 1))
        for un, w in zip(c["units"], want):
            n_cmp += len(w["margins"]); n_und += sum(1 for m in w["margins"] if not m[3])
            assert L.yard_search(un, c["W"])[0] == w["k"] or not w["decidable"]      # the clean yardstick stands inside the truth
        n_inf += any(m[1] == math.inf for w in want for m in w["margins"])
        if c["prime"] in ("hist0", "quiet"):      # the priming search accepts its first candidate on every robot, decidably
            pw = L.prime_of(c["inp"])[2]
            for un in L.prime_units(c["inp"], *c["inp"]["prime_steps"]):
                assert L.truth_search(un, pw[-1]) == 0 and L.margins(un, pw[-1], 0, r)[0][3] and not un.guarded
    assert n_und <= 0.05 * n_cmp, (name, n_und, n_cmp)
    assert n_inf >= 2, (name, n_inf)


def test_cases_hold_the_guard_in_every_mode_and_a_ccd_clamp(pkg, scenes):
    guard, clamp = set(), 0
    for c, r, want in all_cases(pkg, scenes, ["super8", "single", "coupled_rounds", "wave"]):
        un = c["units"][c["target"]]
        if un.guarded:      # the step the accepted candidate is a multiple of IS the guard's
            t0 = float(c["inp"]["st"]["piece_time"][un.robots[0]])
            assert un.step0 == -0.95 * t0 / un.t_dirs[0] and un.step0 < min(np.min(c["steps"][0]), np.min(c["steps"][1]))
            guard.add(c["inp"]["mode"])
        elif c["inp"]["mode"] == 1 and un.step0 < 1.0:      # an obstacle scene's clamp: step0 = 0.8^j, j > 0
            assert L.exponent_of(un.step0, 1.0) > 0 and c["inp"]["st"]["spline"].shape[0] == 2
            clamp += 1
    assert guard == {0, 1, 2} and clamp >= 1, (guard, clamp)


def test_team_bound_lists_sit_at_the_bound():
    c = L.bound_counts()
    assert (c.sum(axis=1) == [96, 97]).all()


# ---- the project's CPU port -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ROWS if not n.startswith("coupled")])
def test_port_accepts_the_truths_candidate_and_commits_its_bits(pkg, scenes, name):
    """oracle.pyoracle.Engine through the same stage calls (modes 0 and 1: the port's coupled search is part of its update_spline, not a stage): the accepted exponent is the
    truth's on every decidable robot; spline, piece_time and the step are x + s d (unfused), t0 + s t_dir and the repeated product, bit for bit; nothing else moves"""
    from oracle.pyoracle import Engine
    tag = L.row(name)[1]
    sh = G.shape(tag)
    for slot in L.row(name)[3]:
        c, r, want = case_of(pkg, scenes, name, slot)
        inp = c["inp"]
        e = Engine("port", G.scene_of(scenes, sh[1], sh[2], G.fleet(sh)), inp["par"])
        e.set_state(inp["st"])
        e.stage_planes()
        e.set_planes(inp["counts"], inp["planes"])
        for u in range(inp["U"]):
            e.set_direction(u, inp["dirs"][u], inp["t_dirs"][u], c["records"][u], inp["gn"][u])
        a, b = e.stage_steps()
        assert np.array_equal(a, c["steps"][0]) and np.array_equal(b, c["steps"][1])
        steps = e.stage_linesearch()
        post = e.get_state()
        for un, w in zip(c["units"], want):
            u = un.robots[0]
            k = L.exponent_of(float(steps[u]), un.step0)
            assert k is not None and (k == w["k"] or not w["decidable"]), (name, slot, u, k, w["k"])
            net, t = L.commit(un, L.step_back(un.step0, k))[0]
            assert np.array_equal(post["spline"][u].view(np.int64), net.view(np.int64)) and post["piece_time"][u] == t, (name, slot, u)
        for n in STATE[1:5]:
            assert np.array_equal(post[n].view(np.int64), inp["st"][n].view(np.int64))


# ---- planted faults -------------------------------------------------------------------------------------------------------------------------
def faulted(c, fault):
    """per unit what the yardstick with the fault planted accepts and commits: (k or None where it accepts nothing, step, [(net, t)])"""
    inp, out = c["inp"], []
    for i, un in enumerate(c["units"]):
        if fault == "guard1" and un.guarded:
            u = un.robots[0]
            s0 = L.guard(float(inp["st"]["piece_time"][u]), un.t_dirs[0], float(min(np.min(c["steps"][0][un.robots]), np.min(c["steps"][1][un.robots]))), fault)[0]
            un = L.Unit(un.probs, un.dirs, un.t_dirs, s0, True, un.robots)
        W = c["W"] if inp["mode"] == 2 else L.search_wolfe(c["records"], un.robots[0], False, fault)
        try:
            k, step, _ = L.yard_search(un, W, fault, cap=60)
        except AssertionError:
            out.append((None, None, None))
            continue
        out.append((k, step, L.commit(un, step)))
    return out


def differs(c, want, got):
    for un, w, (k, step, nets) in zip(c["units"], want, got):
        if not w["decidable"]:
            continue
        if k != w["k"]:
            return "verdict"
        for (net, t), (tn, tt) in zip(nets, L.commit(un, w["step"])):
            if not np.array_equal(net.view(np.int64), tn.view(np.int64)) or t != tt:
                return "bits"
    return None


@pytest.mark.parametrize("fault", L.FAULTS)
def test_planted_fault_is_caught(pkg, scenes, fault):
    """each fault in the yardstick changes the accepted candidate or the committed bits of a decidable search on at least one case; without a fault, none"""
    rows = ["super8", "super4", "wave", "single", "coupled"]
    hits = []
    for c, r, want in all_cases(pkg, scenes, rows):
        assert differs(c, want, faulted(c, None)) is None
        how = differs(c, want, faulted(c, fault))
        if how:
            hits.append((c["row"], c["slot"], how))
    assert hits, fault
    print("fault", fault, "caught on", len(hits), "cases:", hits[:6])


# ---- measured thresholds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,slot", [("super8", 2), ("wave", 7), ("single", 8), ("coupled", 6)])
def test_measured_thresholds_hold_the_yardstick_and_expose_a_wrong_energy(pkg, scenes, name, slot):
    """tests/test_gpu_linesearch.py's assertion (c) with the yardstick in the device's place: the clean search's measured 1e-4 s_k w*_k is the truth's E_-1 - E_k inside
    the bar at the accepting slot and the one before it, in at most 64 probes; a search whose candidates keep the time t0, or take the previous step's trial point,
    misses the same bar by more than a factor 1000 (or leaves every bracket around the truth's threshold)"""
    c, r, want = case_of(pkg, scenes, name, slot)
    un = c["units"][c["target"]]

    def miss(k, fault):
        def search(w):
            try:
                return L.yard_search(un, w, fault, cap=60)[0]
            except AssertionError:
                return L.KCAP + 1
        try:
            lo, hi, n = L.measure_threshold(search, k, float(un.wstar(k)))
        except AssertionError:
            return math.inf
        assert n <= 64 and hi == math.nextafter(lo, math.inf)
        with mp.workdps(L.DPS):
            return float(abs(mpf(L.C1) * mpf(L.step_back(un.step0, k)) * mpf(lo) - (un.truth_energy(-1) - un.truth_energy(k)))) / L.threshold_bar(un, k, r)

    ks = [k for k in (slot - 1, slot) if k >= 0 and L.measurable(un, k)]
    assert slot in ks
    for k in ks:
        assert miss(k, None) <= 1.0, (name, slot, k)
    for fault in ("t_fixed", "prev_step"):
        assert max(miss(k, fault) for k in ks) > 1000.0, (name, slot, fault, [miss(k, fault) for k in ks])
