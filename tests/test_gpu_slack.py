"""The slack (z) and dual update (slack_body, csrc/kernels_step.h) against a 60-digit truth: PRODUCT kernels only, through the stage API -- set_state -> run_stage("begin") ->
stage_slack() -> get_state() -- and, for the two deferred launch forms, through whole iterations.  tests/slack_ref.py holds the truth (mpmath), the yardstick (the same formulas in
plain fp64), the error measure and the cases; tests/test_slack_ref.py shows on the CPU that the truth's derivatives are the finite differences of its energy, that the project's CPU
port lies inside these bars, that the cases meet the conditions relied on here and that eight planted one-line faults each miss the bars by more than a factor 1000.

Shapes (slack_ref.SHAPES), the smallest at which each form exists: P = 2 (both n = 13 mappings, no n = 19), 3, 5, 11 (the P6 strides of the slack arrays beyond one wave's worth of
rows) with two robots in mode 1; mode 0 (scn_a, one robot, ks = 1e-8) and mode 2 (four robots, one shared piece_time) at P = 3.  One context per shape and (mu, kt), closed when
the shape changes.  Classes (the base shape P = 3 runs every state, the others the later ones): real (the port oracle's states after 0, 3, 12 iterations), dual (seeded duals, slack moved by 0.3 sigma), tsmall (t_slack x 0.3 and x 0.01 -- mode 0:
x 0.03 and x 0.01 --: every piece repaired, the t > 0 guard sets the step, four to seven back-offs), tlarge (x 5), edge (per-piece scales that put the smallest eigenvalue ten
eigenvalue bars below and above 0: the repaired twin, and a definite one so close to singular that the search backs off about a hundred times), param (mu in {0.01, 0.1, 10}, kt in
{0.1, 1, 10} on real and tsmall states).

Per case: every decidable piece's four outputs inside K r_class (K = 8; r_class the yardstick's worst over the class at the shape, never the device's own output); the accepted
step, recovered by projecting the device's update on the truth's direction, is the truth's step0 0.8^k with the truth's k -- an Armijo-undecidable piece may land on a neighbouring k
and must be inside the bars for that k; a repaired piece matches the truth's shifted solve at ONE dsigma within the eigenvalue bar (slack_ref.fit_shift); the two fixed control
points of a boundary piece keep z bit for bit and their duals move by mu (C x - z) to the roundings of that expression; the spline and piece_time are untouched; error_bits == 0;
and the forms reached (n and lo, repaired, guard, k) are asserted from the truth's records.

Launch forms.  The stage API runs k_slack(deferred = 0).
  (a) k_slack(deferred = 1): set_state(S); iterate(1) -- the flush pays the update -- against the truth at (post spline, post piece_time, S's slack and duals); the bars are the
      yardstick's on those inputs.
  (b) k_mid's slack range: set_state(S); iterate(2) leaves every state array bit for bit equal to set_state(S); iterate(1); iterate(1), under TJ_MID_ORDER = 0 and 1 (mid_order
      asserted from the plan record), from a real and from a tsmall state (the repaired path).  In the first sequence iteration 1's update runs inside k_mid, in the second in the
      flush; slack_body is one function, so the bits must agree.  This is the route taken: the phase API cannot show k_mid's update alone, because any state access in a begun
      iteration flushes -- k_flush hands the BEGUN iteration's owed update to k_slack(deferred = 1), which would pay it on the state before that iteration's x-update.

Observed on MI355X (TJ_PRINT_OBSERVED=1 prints them), over all shapes: largest ratio to r_class (primal, dual); r_class of the primal in units of u (smallest .. largest over
the shapes); pieces repaired; largest k (with the guard active); undecidable pieces; largest |dsigma| over the eigenvalue bar:
  class           ratio (primal, dual)   r_class (u)          repaired   largest k (guard)   undecidable   dsigma / bar
  real            (2.8, 2.4)             275 .. 1.6e5         0          0   (-)             0             -
  dual            (1.2, 1.0)             1.6 .. 84            43         6   (6)             0             3.5e-4
  tsmall          (3.2, 3.1)             53 .. 8.1e5          126        11  (8)             0             0.041
  tlarge          (2.3, 1.6)             2.8 .. 10.5          0          1   (-)             0             -
  edge            (1.2, 1.2)             2.5e10 .. 4.0e13     57         101 (-)             0             6.4e-4
  param           (1.3, 1.2)             12.5 .. 3.1e4        13         7   (6)             0             2.3e-4
  (a) real        (1.0, 0.64)            21 .. 65             0          0   (-)             0             -
  (a) tsmall      (1.7, 1.6)             55 .. 1.0e3          25         6   (6)             0             0.02
K = 8 in every cell; no class came near it, so the bar stands as the siblings' (the largest, 3.2, is P = 3's tsmall: the project's CPU port reads 3.1 there against the same truth).
In most cells the device shows the port's own figure: slack_body keeps the reference's order of operations.  The edge class's r_class is the price of its definition: ten eigenvalue
bars above 0 the system's condition number is 1e11, the yardstick itself is 1e-3 from the truth, and what that twin pins is the hundred-step search, not the direction's digits.
The repaired pieces' fitted dsigma stays below 5 % of the eigenvalue bar: min_eig_lds is far inside the project's bar on these systems (|H|_max up to 1e12 at t_slack x 0.01).
"""
import math
import os

import numpy as np
import pytest
from mpmath import mp, mpf

from query_kit import STATE
import slack_ref as S

pytestmark = pytest.mark.gpu
TAGS = [sh[0] for sh in S.SHAPES]


def _obs(what, val):
    if os.environ.get("TJ_PRINT_OBSERVED"):
        print("OBSERVED slack", what, val)


# ---- contexts: those of one shape at a time -----------------------------------------------------------------------------------------------
_CTX = {"tag": None, "ctx": {}}


def close_all():
    for s in _CTX["ctx"].values():
        s.close()
    _CTX["ctx"] = {}


def context(pkg, scenes, sh, par):
    if _CTX["tag"] != sh[0]:
        close_all()
        _CTX["tag"] = sh[0]
    key = (par["mu"], par["kt"])
    if key not in _CTX["ctx"]:
        s = pkg.Solver(S.scene_of(scenes, sh), par, stop=0.0)
        plan = pkg.plan_record(ctx=s._ctx)[1]
        assert (plan["mode"], plan["P"], plan["U"]) == sh[1:]
        _CTX["ctx"][key] = s
    return _CTX["ctx"][key]


def same_bits(a, b, names=STATE):
    return all(np.array_equal(a[n].view(np.int64), b[n].view(np.int64)) for n in names)


# ---- one state's update on the device against its records ---------------------------------------------------------------------------------
def recovered_k(tr, out):
    """the accepted step as the projection of the device's update on the truth's direction, in back-offs of the truth's first step: (k, how far from a whole number)"""
    with mp.workdps(S.DPS):
        c = tr["c"]
        d = tr["dirz"] + [tr["t_dir"]]
        dev = [mpf(out["z1"][i]) - c["z"][i] for i in range(18)] + [mpf(out["t1"]) - c["tz"]]
        step = sum(p * q for p, q in zip(dev, d)) / sum(q * q for q in d)
        if not step > 0:
            return -1, math.inf
        x = float(mp.log(step / tr["step0"]) / mp.log(mpf(4) / 5))
        return int(round(x)), abs(x - round(x))


def check_fixed_points(tr, out):
    """a boundary piece's two fixed control points: z' == z bit for bit, and the dual moves by mu (C x - z) to the roundings of that expression (a six-term product sum, a
    difference, a product) and of the final sum"""
    sp, P = tr["pr"]["sp"], tr["pr"]["P"]
    fixed = (0, 1) if sp == 0 else ((4, 5) if sp == P - 1 else ())
    pr, c = tr["pr"], tr["c"]
    with mp.workdps(S.DPS):
        for j in fixed:
            for a in range(3):
                i = j + 6 * a
                assert np.float64(out["z1"][i]).view(np.int64) == np.float64(pr["z"][i]).view(np.int64), (sp, j, a)
                mag = sum(abs(pr["C"][j][k] * pr["x"][k][a]) for k in range(6))
                tol = float(c["mu"]) * S.U64 * (8 * mag + 2 * abs(pr["z"][i])) + 2 * S.U64 * abs(out["lam1"][i])
                assert abs(float(mpf(out["lam1"][i]) - c["lam"][i] - c["mu"] * (c["cx"][i] - c["z"][i]))) <= tol, (sp, j, a)
    return len(fixed)


def check_pieces(recs, post, r, where):
    """every piece of one state -> (worst primal / r, worst dual / r, repaired, largest k, undecidable, worst |dsigma| / bar)"""
    wp = wd = ws = 0.0
    n_rep = n_und = kmax = n_fixed = 0
    for u, sp, tr, yd in recs:
        out = S.state_outputs(post, u, sp)
        n_fixed += check_fixed_points(tr, out)
        if tr["why"] == "eigenvalue":
            n_und += 1
            continue
        k, frac = recovered_k(tr, out)
        assert frac < 0.25, (where, u, sp, k, frac)
        if tr["undecidable"]:
            n_und += 1
            assert abs(k - tr["k"]) <= 1, (where, u, sp, k, tr["k"])
        else:
            assert k == tr["k"], (where, u, sp, k, tr["k"])
        m = S.measure(tr, out, k=k)
        assert S.inside(m, r), (where, u, sp, "k", k, "primal", m[0] / r[0], "dual", m[2] / r[1], "dsigma/bar", m[3])
        wp, wd, ws = max(wp, m[0] / r[0]), max(wd, m[2] / r[1]), max(ws, abs(m[3]))
        n_rep += tr["repaired"]; kmax = max(kmax, k)
    assert n_und <= 0.05 * len(recs), (where, n_und)
    assert n_fixed == 4 * len({u for u, _, _, _ in recs})      # two boundary pieces per robot, two fixed points each
    return wp, wd, n_rep, kmax, n_und, ws


def forms(recs):
    """what the case reaches, from the truth's records"""
    dec = [tr for _, _, tr, _ in recs if not tr["undecidable"]]
    return dict(n={(tr["n"], tr["lo"]) for tr in dec}, repaired={tr["repaired"] for tr in dec}, guard={tr["guard"] for tr in dec}, k={tr["k"] for tr in dec},
                guard_k=max([tr["k"] for tr in dec if tr["guard"]] + [-1]))


@pytest.mark.parametrize("tag,cls", [(t, c) for t in TAGS for c in S.CLASSES])
def test_update_against_the_truth(pkg, scenes, tag, cls):
    sh = S.shape(tag)
    P = sh[2]
    r = S.class_bars(pkg, scenes, sh, cls)
    seen = dict(n=set(), repaired=set(), guard=set(), k=set(), guard_k=-1)
    worst = [0.0, 0.0, 0, 0, 0, 0.0]
    for case in S.cases(pkg, scenes, sh, cls):
        _, name, st, par = case
        recs = S.case_records(pkg, scenes, sh, case)
        s = context(pkg, scenes, sh, par)
        s.set_state(st)
        s.run_stage("begin")
        s.stage_slack()
        post = s.get_state()
        assert s.stats()["error_bits"] == 0
        assert same_bits(post, st, ("spline", "piece_time"))
        w = check_pieces(recs, post, r, (tag, cls, name))
        worst = [max(worst[0], w[0]), max(worst[1], w[1]), worst[2] + w[2], max(worst[3], w[3]), worst[4] + w[4], max(worst[5], w[5])]
        f = forms(recs)
        assert f["n"] == ({(13, 2), (13, 0)} if P == 2 else {(13, 2), (13, 0), (19, 0)}), (tag, cls, name, f["n"])      # both n = 13 mappings, and n = 19 where there is one
        for key in ("n", "repaired", "guard", "k"):
            seen[key] |= f[key]
        seen["guard_k"] = max(seen["guard_k"], f["guard_k"])
    # the forms the class is there for
    if cls == "real":
        assert seen["repaired"] == {False} and 0 in seen["k"] and False in seen["guard"]
    if cls == "tlarge":
        assert seen["repaired"] == {False}
    if cls == "tsmall":
        assert seen["repaired"] == {True} and seen["guard_k"] >= 4
    if cls == "edge":
        assert seen["repaired"] == {False, True} and max(seen["k"]) >= 50 and seen["guard"] == {False}
    if cls == "dual" and sh[1] != 0:
        assert len(seen["k"]) >= 2
    _obs((tag, cls), dict(primal=float("%.2g" % worst[0]), dual=float("%.2g" % worst[1]), r_primal_u=float("%.3g" % (r[0] / S.U64)), r_dual_u=float("%.3g" % (r[1] / S.U64)),
                          repaired=worst[2], kmax=worst[3], undecidable=worst[4], dsigma_over_bar=float("%.2g" % worst[5]), guard_kmax=seen["guard_k"]))
    if (tag, cls) == (TAGS[-1], S.CLASSES[-1]):
        close_all()


# ---- the deferred launch forms ---------------------------------------------------------------------------------------------------------------
def _start_states(pkg, scenes, sh):
    """a real state of the shape (after three iterations) and a tsmall one (after twelve, t_slack x 0.3 -- mode 0: x 0.03)"""
    real = next(c for c in S.cases(pkg, scenes, sh, "real") if c[1] == "it3")
    small = next(c for c in S.cases(pkg, scenes, sh, "tsmall") if c[1].startswith("it12") and not c[1].endswith("*0.01"))
    return [("real", real[2], real[3]), ("tsmall", small[2], small[3])]


@pytest.mark.parametrize("tag", ["P2", "P3", "single", "coupled"])
def test_deferred_update_in_the_flush_against_the_truth(pkg, scenes, tag):
    """(a): k_slack(deferred = 1).  The update does not touch the spline, so the iteration's post spline and piece_time with the start's slack and duals are its inputs"""
    close_all()
    sh = S.shape(tag)
    ks = S.scene_of(scenes, sh)["ks"]
    for kind, st, par in _start_states(pkg, scenes, sh):
        s = pkg.Solver(S.scene_of(scenes, sh), par, stop=0.0)
        s.set_state(st)
        s.iterate(1)
        post = s.get_state()
        assert s.stats()["error_bits"] == 0
        s.close()
        hybrid = {n: (post[n] if n in ("spline", "piece_time") else st[n]) for n in STATE}
        recs = []
        for u, row in enumerate(S.problems(pkg, par, ks, sh[2], hybrid)):
            for sp, pr in enumerate(row):
                tr = S.truth(pr)
                yd = S.yard(pr, kmin=tr["k"])
                recs.append((u, sp, S.decide(tr, yd), yd))
        r = S.bars([(tr, yd) for _, _, tr, yd in recs])
        w = check_pieces(recs, post, r, (tag, "flush", kind))
        f = forms(recs)
        assert f["repaired"] == ({False} if kind == "real" else {True}), (tag, kind, f)
        _obs((tag, "flush", kind), dict(primal=float("%.2g" % w[0]), dual=float("%.2g" % w[1]), r_primal_u=float("%.3g" % (r[0] / S.U64)), r_dual_u=float("%.3g" % (r[1] / S.U64)),
                                        repaired=w[2], kmax=w[3], undecidable=w[4], dsigma_over_bar=float("%.2g" % w[5]), guard_kmax=f["guard_k"]))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tag", ["P2", "P3", "single", "coupled"])
def test_update_inside_k_mid_equals_the_flush_bitwise(pkg, scenes, monkeypatch, tag, order):
    """(b): iterate(2) pays iteration 1's update in k_mid's slack range, iterate(1); iterate(1) in the flush's k_slack(deferred = 1)"""
    close_all()
    sh = S.shape(tag)
    monkeypatch.setenv("TJ_MID_ORDER", str(order))
    for kind, st, par in _start_states(pkg, scenes, sh):
        ends = []
        for batches in ((2,), (1, 1)):
            s = pkg.Solver(S.scene_of(scenes, sh), par, stop=0.0)
            plan = pkg.plan_record(ctx=s._ctx)[1]
            assert plan["mid_order"] == order and plan["n_mid_slack"] == sh[2] * sh[3], (plan["mid_order"], plan["n_mid_slack"])
            s.set_state(st)
            for n in batches:
                s.iterate(n)
            ends.append(s.get_state())
            assert s.stats()["error_bits"] == 0
            s.close()
        assert same_bits(ends[0], ends[1]), (tag, order, kind, [n for n in STATE if not np.array_equal(ends[0][n], ends[1][n])])
        assert not same_bits(ends[0], st, ("p_slack", "t_slack", "p_lambda", "t_lambda"))
