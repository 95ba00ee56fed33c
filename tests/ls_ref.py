"""The Armijo search on the x-objective (k_linesearch; coupled: k_ls_coupled / k_ls_commit, csrc/kernels_ls.h) restated three times over -- TEST INFRASTRUCTURE ONLY.

  truth      the search with every energy at DPS = 60 digits (mpmath).  The energy is tests/grad_ref.py's _piece_energy, evaluated at (x + s d, t0 + s t_dir); the
             objective is NOT restated here.  Inputs: the state, the plane lists, the direction record (d, t_dir, wolfe) and step0, all fp64 values.  For one unit --
             ONE robot in the decoupled modes, the FLEET (energies added in robot order) in the coupled mode:
               E_-1 = E(x, t0);   s_k = step0 0.8^k as the fp64 value of k multiplications (an input to the truth, as the segment weights are);
               E_k = E(x + s_k d, t0 + s_k t_dir);   w*_k = (E_-1 - E_k) / (1e-4 s_k)  (-inf where E_k = +inf: such a candidate never passes);
               accepted: the first k with wolfe <= w*_k.
             step0 arrives with the t > 0 guard applied (guard(): step0 = -0.95 t0 / t_dir where t0 + step0 t_dir <= 0, in fp64 -- the step is an input).
             REFERENCE QUIRK, kept: the decoupled search compares every robot against the global `wolfe`, which the LAST robot's Newton solve left (D.wolfe(D.U - 1),
             Optimization3D_multi.h:730,792) -- search_wolfe().  The coupled search has one wolfe of the whole system.
  yardstick  the same search in plain fp64, natural order: the trial net x + s d by one product and one sum per entry, the pieces' energies added in piece order, the
             robots' in robot order, the comparison written as the reference writes it: !(e - 1e-4*wolfe*step < E_k).
  faults     eight one-line faults that can be planted in the yardstick (FAULTS); tests/test_ls_ref.py shows that each changes the verdict or the committed bits.

Decidability (tests/test_gpu_grad.py's convention and factor).  r_class = the yardstick's worst |yardstick - truth| / A over the energies of a class at one shape
(A: grad_ref's magnitude sum of the energy), floored at u = 2^-53.  Comparison k is decidable when |E_-1 - 1e-4 wolfe s_k - E_k| > K r_class (A_-1 + A_k), K = 8; a
search is decidable when every comparison up to the accepted one is.

Measured thresholds.  measure_threshold() takes a search as a black box (wolfe -> accepted k) and returns the largest wolfe at which it still accepts candidate k or an
earlier one, by bisection: that is w*_k where w*_k is a strict running maximum of w*_0 .. w*_k (measurable()).  It works on the device and on the yardstick alike and
turns a pass / fail kernel into a measured one: 1e-4 s_k w*_k is E_-1 - E_k as the search under test computes it.

Cases (case()).  The state is one of grad_ref's (real_states / vary / binding_state), the lists the CPU port's own for it or grad_ref.synthetic_planes, the direction
the port's stage_direction() of that state times a scale per robot (d, t_dir and wolfe all scale).  The scale cannot place an acceptance on these states: in sigma = s c
the Armijo condition does not depend on c, and the first candidate's sigma_0 = step0 c is pinned by the CCD clamp (step0 falls as c grows: b3 at c = 1 and c = 20 starts
at sigma_0 = 0.64 and 0.70) or by the t > 0 guard (sigma_0 = 0.95 t0 / |t_dir|, whatever c).  So the scale is spent on giving every robot of a fleet the same wolfe record
(c_u = w_max / w_u: the searches then end at comparable depths under the ONE wolfe the decoupled search uses), and the slot is placed by the search wolfe, which is as
much an input of the kernel as the direction: W halfway between w*_k and the largest earlier threshold (fp64, choose_wolfe) -- the truth then accepts the chosen k with
half the spacing of two thresholds as room on either side, and k is measurable by construction.
"""
import math

import numpy as np
from mpmath import mp, mpf

import grad_ref as G

DPS = G.DPS
U64 = G.U64
K = 8.0
C1 = 1e-4
KCAP = 80            # no case of this file searches deeper (depth 31 and beyond in coupled mode: coupled_long_kat.npz)
FAULTS = ("pow", "t_fixed", "prev_step", "pair_swap", "round_min", "c1", "own_wolfe", "guard1")


# ---- the inputs' own arithmetic ---------------------------------------------------------------------------------------------------------
def step_back(step0, k, fault=None):
    """step0 0.8^k by k multiplications (the reference's repeated step *= 0.8)"""
    if fault == "pow":
        return step0 * 0.8 ** k
    for _ in range(k):
        step0 *= 0.8
    return step0


def guard(t0, t_dir, step0, fault=None):
    """the t > 0 guard (Optimization3D_multi.h:586-601) -> (step0, active)"""
    if t0 + step0 * t_dir <= 0:
        return -(1.0 if fault == "guard1" else 0.95) * t0 / t_dir, True
    return step0, False


def exponent_of(step, step0, cap=KCAP):
    """k with step == step0 0.8^k by repeated multiplication, bit for bit (None: the step is no such value)"""
    s = step0
    for k in range(cap + 1):
        if s == step:
            return k
        s *= 0.8
    return None


def search_wolfe(wolfes, u, coupled, fault=None):
    """the wolfe robot u's search compares against: decoupled -- the LAST robot's (reference quirk, see the module text); coupled -- the system's one value"""
    if coupled or fault != "own_wolfe":
        return float(wolfes[-1])
    return float(wolfes[u])


# ---- a unit: what one search decides over -------------------------------------------------------------------------------------------------
class Unit:
    """probs: grad_ref.problem() of each robot of the unit (one; coupled: the fleet), dirs [3][T] and t_dirs per robot, step0: with the guard applied"""

    def __init__(self, probs, dirs, t_dirs, step0, guarded=False, robots=None):
        self.probs, self.dirs, self.t_dirs, self.step0, self.guarded = probs, [np.asarray(d) for d in dirs], [float(t) for t in t_dirs], float(step0), guarded
        self.robots = robots
        self._truth, self._yard = {}, {}

    def steps(self, n, fault=None):
        return [step_back(self.step0, k, fault) for k in range(n)]

    # one energy of the unit in an arithmetic: s_x / s_t = None: at the state
    def _energy(self, ar, s_x, s_t, mags=False):
        tot, A = ar.num(0), 0.0
        for pr, d, td in zip(self.probs, self.dirs, self.t_dirs):
            t = ar.num(pr["t"]) if s_t is None else ar.num(pr["t"]) + ar.num(s_t) * ar.num(td)
            e_r = ar.num(0)
            for sp in range(pr["P"]):
                x = None
                if s_x is not None:
                    x = [[ar.num(pr["spline"][a][3 * sp + k]) + ar.num(s_x) * ar.num(d[a][3 * sp + k]) for a in range(3)] for k in range(6)]
                e = G._piece_energy(ar, pr, sp, x, t, mags=mags)
                if mags:
                    e, a1 = e
                    A += a1
                e_r += e
            tot += e_r
        return (tot, A) if mags else tot

    def truth_energy(self, k):
        """E_k at 60 digits (k = -1: E(x)); mp.inf where a limit or a plane is violated"""
        if k not in self._truth:
            with mp.workdps(DPS):
                s = None if k < 0 else step_back(self.step0, k)
                self._truth[k] = self._energy(G._M, s, s)
        return self._truth[k]

    def yard_energy(self, s_x, s_t):
        """(E, A) in fp64 at the trial net of step s_x and the time of step s_t"""
        key = (s_x, s_t)
        if key not in self._yard:
            try:
                self._yard[key] = self._energy(G._F, s_x, s_t, mags=True)
            except ZeroDivisionError:      # a flight time of exactly 0 (the planted guard fault only)
                self._yard[key] = (math.inf, 0.0)
        return self._yard[key]

    def wstar(self, k):
        """the truth's threshold of candidate k (mpf; -inf where E_k = +inf)"""
        with mp.workdps(DPS):
            e = self.truth_energy(k)
            if e == mp.inf:
                return -mp.inf
            return (self.truth_energy(-1) - e) / (mpf(C1) * mpf(step_back(self.step0, k)))


def truth_search(unit, wolfe, cap=KCAP):
    """the accepted k"""
    with mp.workdps(DPS):
        for k in range(cap + 1):
            if mpf(wolfe) <= unit.wstar(k):
                return k
    raise AssertionError("the truth accepts no candidate up to %d" % cap)


def measurable(unit, k):
    """w*_k is a strict running maximum of w*_0 .. w*_k"""
    with mp.workdps(DPS):
        return unit.wstar(k) != -mp.inf and all(unit.wstar(j) < unit.wstar(k) for j in range(k))


def round_of(k):
    """the candidates that share candidate k's round of eight one-wave evaluations: round 0 holds E(x) and 0 .. 6, round r the eight from 8 r - 1"""
    r = (k + 1) // 8
    return range(max(0, 8 * r - 1), 8 * r + 7)


def yard_search(unit, wolfe, fault=None, cap=KCAP):
    """-> (accepted k, its step, [(k, e_base, E_k, A_base, A_k, step)] of the comparisons made).  The search as the reference writes it, with a planted fault"""
    c1 = 1e-3 if fault == "c1" else C1
    e, A0 = unit.yard_energy(None, None)
    made = []

    def cand(k):
        j = k
        if fault == "pair_swap" and k >= 1:      # the two candidates a team evaluates side by side: (1, 2), (3, 4), ...
            j = k + 1 if k % 2 else k - 1
        s_t = step_back(unit.step0, j, fault)
        s_x = step_back(unit.step0, max(j - 1, 0), fault) if fault == "prev_step" else s_t
        ek, ak = unit.yard_energy(s_x, None if fault == "t_fixed" else s_t)
        return ek, ak

    step, k = unit.step0, 0
    while k <= cap:
        if fault == "pow":
            step = step_back(unit.step0, k, fault)
        ek, ak = cand(k)
        made.append((k, e, ek, A0, ak, step))
        if not (e - c1 * wolfe * step < ek):
            if fault == "round_min":      # the smallest energy of the accepting round instead of the first that passes
                best, st = (k, ek, step), step
                for j in round_of(k):
                    if j > k:
                        st = step_back(unit.step0, j)
                        ej, _ = cand(j)
                        if not (e - c1 * wolfe * st < ej) and ej < best[1]:
                            best = (j, ej, st)
                return best[0], best[2], made
            return k, step, made
        step *= 0.8
        k += 1
    raise AssertionError("the yardstick accepts no candidate up to %d" % cap)


def commit(unit, step):
    """what a search commits for the step it accepted: per robot (x + step d, one product and one sum per entry, unfused; t0 + step t_dir)"""
    return [(pr["spline"] + step * d, pr["t"] + step * td) for pr, d, td in zip(unit.probs, unit.dirs, unit.t_dirs)]


# ---- bars -----------------------------------------------------------------------------------------------------------------------------------
def energy_records(unit, kmax):
    """[(k, truth E_k, yardstick E_k, A_k)] for k = -1 .. kmax"""
    out = []
    for k in range(-1, kmax + 1):
        s = None if k < 0 else step_back(unit.step0, k)
        ye, ya = unit.yard_energy(s, s)
        out.append((k, unit.truth_energy(k), ye, ya))
    return out


def r_of(records):
    """the yardstick's worst |yardstick - truth| / A over energy records, floored at u; a truth of +inf must be the yardstick's too"""
    r = U64
    with mp.workdps(DPS):
        for k, te, ye, ya in records:
            if te == mp.inf or not math.isfinite(ye):
                assert te == mp.inf and ye == math.inf, ("the yardstick and the truth disagree on a violated limit", k)
                continue
            r = max(r, float(abs(mpf(ye) - te)) / ya)
    return r


def margins(unit, wolfe, k_acc, r):
    """per comparison k <= k_acc: (k, |E_-1 - 1e-4 wolfe s_k - E_k|, K r (A_-1 + A_k), decidable); a candidate at +inf is decidable"""
    out = []
    with mp.workdps(DPS):
        e0 = unit.truth_energy(-1)
        A0 = unit.yard_energy(None, None)[1]
        for k in range(k_acc + 1):
            s = step_back(unit.step0, k)
            ek = unit.truth_energy(k)
            if ek == mp.inf:
                out.append((k, math.inf, 0.0, True))
                continue
            gap = float(abs(e0 - mpf(C1) * mpf(wolfe) * mpf(s) - ek))
            bar = K * r * (A0 + unit.yard_energy(s, s)[1])
            out.append((k, gap, bar, gap > bar))
    return out


def threshold_bar(unit, k, r):
    """(c): |1e-4 s_k w*_k(measured) - (E_-1 - E_k)| <= K r (A_-1 + A_k) + 4 ulp(|E_-1|): the bisection's resolution and the two roundings of the comparison's left side"""
    s = step_back(unit.step0, k)
    e0 = float(unit.truth_energy(-1))
    return K * r * (unit.yard_energy(None, None)[1] + unit.yard_energy(s, s)[1]) + 4 * math.ulp(abs(e0))


# ---- measured thresholds ------------------------------------------------------------------------------------------------------------------------
def measure_threshold(search, k, guess, probes=64):
    """search: wolfe -> accepted k (a black box).  -> (lo, hi, probes used): the largest wolfe found at which it accepts k or an earlier candidate and the smallest found
    at which it accepts a later one.  guess: a value near the switch (the truth's w*_k): the bracket guess -+ h opens at h = 2^-30 |guess| and widens by 1024 until it holds
    the switch; then bisection to adjacent doubles or until `probes` are spent"""
    n, h = 0, max(abs(guess) * 2.0 ** -30, 1e-300)
    while True:
        lo, hi = guess - h, guess + h
        n += 2
        if search(lo) <= k and search(hi) > k:
            break
        h *= 1024.0
        assert n < 12, ("no bracket around the guess", k, guess, h)
    while n < probes:
        mid = lo + (hi - lo) / 2
        if not lo < mid < hi:
            break
        n += 1
        if search(mid) <= k:
            lo = mid
        else:
            hi = mid
    return lo, hi, n


# ---- the cases: rows of the shape table x accepting slots (tests/test_gpu_linesearch.py runs them on the device; tests/test_ls_ref.py asserts what they reach) ----------
# row = (name, grad_ref shape tag, environment of the context, accepting slots to hit, plane lists, how a search is primed)
#   lists: "own" the port's own for the state, "bound" synthetic lists of M = 96 / 97 planes (robot 0 / robot 1: the largest the team shape holds at S = 24 and one above),
#          "big" grad_ref.synthetic_counts beyond the line search's LDS plane capacity (716 at P = 11, asserted on the device)
#          "syn" grad_ref.synthetic_counts (robot 0: 319 planes, beyond the team shape and LS_NARROW_MIN_PLANES = 160; robot 1: below 43)
#   prime: None; "hist0": a search that accepts candidate 0 on every robot runs first (ls_hist == 0); "reset": the context is reset first (ls_hist == -1);
#          "quiet": the context has iterated through ten iterations in which every robot took the full step (Ctl::ls_quiet >= 8) and no begin stage runs afterwards;
#          every search is primed as under "hist0" -- the narrow first round of k_linesearch (W = hist + 2)
ROWS = [
    ("super8", "res8", {}, (0, 1, 2, 15, 16, 17, 18), "own", None),
    ("super4", "res8", {"TJ_LS_HELP": "4"}, (7, 8, 9), "own", None),
    ("team0", "res8", {"TJ_LS_HELP": "1"}, (0, 1, 7), "own", "hist0"),
    ("wave", "res8", {"TJ_LS_FAST": "0"}, (0, 6, 7, 14, 15), "own", None),
    ("wave_hist", "res8", {"TJ_LS_HELP": "1"}, (0, 7), "own", "reset"),
    ("giveup", "res8", {"TJ_LS_HELP_MUTE": "1"}, (1, 2, 9, 10), "own", None),
    ("late", "res8", {"TJ_LS_HELP_LATE": "15"}, (2, 16), "own", None),
    ("bound", "res8", {}, (0, 2), "bound", None),
    ("narrow", "res8", {"TJ_LS_HELP_MUTE": "1"}, (0, 1, 8, 9), "syn", "quiet"),
    ("P11big", "P11", {}, (0, 3), "big", None),
    ("P11", "P11", {}, (2, 3, 6, 7), "own", None),
    ("P2", "P2", {}, (0, 7), "own", None),
    ("res1", "res1", {}, (0, 7), "own", None),
    ("res16", "res16", {}, (0, 7), "own", None),
    ("single", "single", {}, (0, 1, 8, 11), "own", None),      # (11: the guard's slot in mode 0)
    ("coupled", "coupled", {}, (0, 6, 7, 30), "own", None),
    ("coupled_rounds", "coupled", {"TJ_LSC_WIDE": "0"}, (0, 6, 7, 30), "own", None),
]
LSL_PLANE_CAP_P11 = 716
# the classes a slot may be placed on, in the order tried (rotated by the slot: neighbouring slots land on different states).  b3: per-robot times, seeded duals, a CCD
# clamp; a12: a late state, no clamp; c_tight: limits that bind (candidates at +inf); a3: an early state, the t > 0 guard sets step0
CLASSES = ("b3", "a12", "c_tight", "a3")
FALLBACK = ("c_dense", "b0")      # tried after them (res = 1 accepts the first candidate on these only)
# slots placed on a class by hand: what a row must reach beyond its slots -- two cases that reject a candidate at +inf, the guard once per mode
TARGET = {"narrow": 0}      # the robot whose lists put it into the narrow round
FIRST = {("narrow", 0): "a12", ("narrow", 1): "a12", ("narrow", 8): "a12", ("narrow", 9): "a12", ("single", 8): "c_dense", ("single", 11): "a3", ("coupled", 7): "b3", ("coupled_rounds", 30): "a3", ("bound", 0): "b3", ("res1", 0): "b0", ("res16", 0): "b3"}


def row(name):
    return next(r for r in ROWS if r[0] == name)


def bound_counts():
    c = np.full((2, 24), 4, dtype=np.int32)
    c[1, 0] = 5
    return c


_INPUTS = {}


def inputs(pkg, scenes, tag, cls, lists="own", scale=1.0):
    """the inputs of a search but step0: state, parameters, plane lists, and the port's direction record of that state times a scale per robot -- scale w_ref / w_u, so that
    every robot's record carries the same wolfe (a fleet's searches then end at comparable depths under the one wolfe the decoupled search uses).  Coupled: the port's
    update_spline direction, scale 1 (its CCD step is the port's only for its own direction).  port_steps: the port's (step_self, step_pos) for these directions"""
    key = (tag, cls, lists, scale)
    if key in _INPUTS:
        return _INPUTS[key]
    import ctypes as C
    from oracle.pyoracle import Engine
    sh = G.shape(tag)
    _, mode, P, res, _ = sh
    U = G.fleet(sh)
    st, par, kind = G.case(pkg, scenes, sh, cls)
    e = Engine("port", G.scene_of(scenes, mode, P, U), par)
    e.set_state(st)
    counts, planes = e.stage_planes()
    if lists == "bound":
        counts = bound_counts()
    elif lists == "big":
        counts = G.synthetic_counts(U, P, res, big=LSL_PLANE_CAP_P11)
    elif lists == "syn":
        counts = G.synthetic_counts(U, P, res)
    elif kind == "none":
        counts = np.zeros((U, P * res), dtype=np.int32)
    if lists != "own" or kind == "none":
        planes = G.synthetic_planes(pkg, par, P, st, counts, 5) if counts.sum() else np.zeros((0, 4))
        e.set_planes(counts, planes)
    if mode == 2:
        assert scale == 1.0
        e.stage_update_spline()
        d = dict(direction=np.zeros((U, 3, 3 * P + 3)), t_direction=np.zeros(U), wolfe=np.zeros(U), gn=np.zeros(U))
        for u in range(U):
            a, b, c = C.c_double(), C.c_double(), C.c_double()
            e._f("get_direction")(C.c_int(u), d["direction"][u].ctypes.data_as(C.POINTER(C.c_double)), C.byref(a), C.byref(b), C.byref(c))
            d["t_direction"][u], d["wolfe"][u], d["gn"][u] = a.value, b.value, c.value
        info = np.zeros(4)
        e._f("coupled_info")(info.ctypes.data_as(C.POINTER(C.c_double)))
        cs = np.ones(U)
        port_steps = (np.full(U, info[1]), np.full(U, info[2]))
    else:
        d = e.stage_direction()
        cs = scale * d["wolfe"].max() / d["wolfe"]
    out = dict(tag=tag, cls=cls, mode=mode, P=P, res=res, U=U, st=st, par=par, counts=np.array(counts), planes=np.array(planes),
               dirs=[d["direction"][u] * cs[u] for u in range(U)], t_dirs=[float(d["t_direction"][u] * cs[u]) for u in range(U)],
               wolfe=[float(d["wolfe"][u] * cs[u]) for u in range(U)], gn=[float(g) for g in d["gn"]])
    if mode != 2:
        for u in range(U):
            e.set_direction(u, out["dirs"][u], out["t_dirs"][u], out["wolfe"][u], out["gn"][u])
        port_steps = e.stage_steps()
        pd, pt, pw = prime_of(out)
        for u in range(U):
            e.set_direction(u, pd[u], pt[u], pw[u], out["gn"][u])
        a, b = e.stage_steps()
        out["prime_steps"] = (np.array(a), np.array(b))
    out["port_steps"] = (np.array(port_steps[0]), np.array(port_steps[1]))
    out["probs"] = G.problems(pkg, par, P, st, out["counts"], out["planes"])
    out["_units"] = {}
    _INPUTS[key] = out
    return out


def units_of(inp, step_self, step_pos):
    """the searches of a fleet for the CCD steps given: one Unit per robot, coupled: one for the fleet (its step: the smallest of all).  Kept per steps: the energies of a
    unit do not depend on the wolfe a case chooses, so every slot of every row on the same inputs shares them"""
    key = (tuple(np.asarray(step_self).tolist()), tuple(np.asarray(step_pos).tolist()))
    if key not in inp["_units"]:
        U = inp["U"]
        if inp["mode"] == 2:
            s0, g = guard(float(inp["st"]["piece_time"][0]), inp["t_dirs"][0], float(min(np.min(step_self), np.min(step_pos))))
            us = [Unit(inp["probs"], inp["dirs"], inp["t_dirs"], s0, g, robots=list(range(U)))]
        else:
            us = []
            for u in range(U):
                s0, g = guard(float(inp["st"]["piece_time"][u]), inp["t_dirs"][u], float(min(step_self[u], step_pos[u])))
                us.append(Unit([inp["probs"][u]], [inp["dirs"][u]], [inp["t_dirs"][u]], s0, g, robots=[u]))
        inp["_units"][key] = us
    return inp["_units"][key]


def yard_thresholds(unit, n):
    """w*_0 .. w*_(n-1) as the yardstick sees them (fp64; -inf at a violated limit)"""
    e0 = unit.yard_energy(None, None)[0]
    out = []
    for k in range(n):
        s = step_back(unit.step0, k)
        ek = unit.yard_energy(s, s)[0]
        out.append((e0 - ek) / (C1 * s) if math.isfinite(ek) else -math.inf)
    return out


def choose_wolfe(unit, k):
    """a wolfe at which the search accepts candidate k with room on both sides: halfway between w*_k and the largest earlier threshold (fp64; None where w*_k is no strict
    running maximum, or not positive)"""
    ws = yard_thresholds(unit, k + 1)
    prev = max(ws[:k], default=-math.inf)
    if not (math.isfinite(ws[k]) and ws[k] > prev and ws[k] > 0):
        return None
    return 0.9 * ws[k] if prev < 0.8 * ws[k] else prev + (ws[k] - prev) / 2


def place(inp, units, slot, target):
    """the wolfe records of a case that puts unit `target`'s acceptance on `slot` -> (search wolfe W, records per robot as set_direction takes them) or None where the slot
    cannot be placed there (not measurable, or another robot's search would not end)"""
    W = choose_wolfe(units[target], slot)
    if W is None:
        return None
    try:
        for un in units:
            yard_search(un, W, cap=40)
    except AssertionError:
        return None
    if inp["mode"] == 2:      # one wolfe of the whole system: robot 0's record carries it, the others 0 (the device adds the records up, see tests/test_gpu_linesearch.py)
        return W, [W] + [0.0] * (inp["U"] - 1)
    return W, inp["wolfe"][:-1] + [W]


def case(pkg, scenes, row_name, slot, steps_of):
    """the case of (row, slot): the first class (CLASSES rotated by the slot) and target robot on which the slot can be placed.  steps_of(inputs) -> (step_self, step_pos):
    the CCD stage's answer for those inputs (the port's: inputs["port_steps"]; on the device: its own stage_steps, which also leaves the context staged).
    -> dict(inp, units, target, slot, W, records)"""
    name, tag, env, slots, lists, prime = row(row_name)
    U = G.fleet(G.shape(tag))
    rot = slots.index(slot) + len(name)
    order = [CLASSES[(rot + i) % len(CLASSES)] for i in range(len(CLASSES))] + list(FALLBACK)
    if (name, slot) in FIRST:
        order.insert(0, FIRST[name, slot])
    for cls in order:
        inp = inputs(pkg, scenes, tag, cls, lists)
        a, b = steps_of(inp)
        units = units_of(inp, a, b)
        for j in range(len(units)):
            target = TARGET.get(name, (rot + j) % len(units))
            got = place(inp, units, slot, target)
            if got is not None:
                return dict(row=name, inp=inp, units=units, target=target, slot=slot, W=got[0], records=got[1], steps=(np.array(a), np.array(b)), prime=prime)
    raise AssertionError(("no class places the slot", row_name, slot))


PRIME_EPS = 2.0 ** -10


def prime_of(inp):
    """the search that primes ls_hist == 0: the same state along the port's direction times PRIME_EPS, against its own wolfe record -- a Newton step a thousand times
    shortened passes the Armijo test at once, on every robot (asserted where it is used) -> (dirs, t_dirs, wolfe records)"""
    return [d * PRIME_EPS for d in inp["dirs"]], [t * PRIME_EPS for t in inp["t_dirs"]], [w * PRIME_EPS for w in inp["wolfe"]]


def prime_units(inp, step_self, step_pos):
    dirs, t_dirs, _ = prime_of(inp)
    return units_of(dict(inp, dirs=dirs, t_dirs=t_dirs, _units={}), step_self, step_pos)


def expected(c, wolfe=None, r=None):
    """the truth's answer to a case: per unit (k, step, decidable, margins); wolfe: another search wolfe than the case's (the probes of a measurement)"""
    W = c["W"] if wolfe is None else wolfe
    out = []
    for un in c["units"]:
        k = truth_search(un, W)
        m = margins(un, W, k, r if r is not None else U64)
        out.append(dict(k=k, step=step_back(un.step0, k), decidable=all(x[3] for x in m), margins=m))
    return out


# candidates every class of a shape is measured over for r_class, whatever slots its cases use (beyond them: the candidates a case's own truth holds)
DEPTH = {"res8": 20, "P11": 9, "P2": 9, "res1": 9, "res16": 9, "single": 12, "coupled": 31}


def class_r(c):
    """r_class of a case: the yardstick's worst |yardstick - truth| / A over the class -- every unit of the case's inputs, candidates -1 .. DEPTH of the shape (the lists
    beyond the LDS capacity: 5, an energy costs ten times as much there) -- and over every further candidate the case's own searches look at; floored at u"""
    inp = c["inp"]
    key = ("r", tuple(un.step0 for un in c["units"]))
    if key not in inp:
        depth = 5 if inp["counts"].sum() > 1000 else DEPTH[inp["tag"]]
        inp[key] = r_of([rec for un in c["units"] for rec in energy_records(un, depth)])
    own = [rec for un in c["units"] for rec in energy_records(un, truth_search(un, c["W"]))]
    return max(inp[key], r_of(own))
