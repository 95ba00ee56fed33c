"""CPU: tests/slack_ref.py checks itself -- the truth's derivatives against finite differences of the truth's energy, the project's CPU oracle inside the yardstick's bars on
every case, the conditions on the inputs that tests/test_gpu_slack.py relies on, and eight planted one-line faults outside the bars.

Planted faults, base shape (P = 3, two robots), the factor by which the faulty yardstick misses K r_class on the class named (test_planted_fault_misses_the_bars prints them):
  cross4     the cross term's -5 g1/t taken with 4                          tsmall   3.7e12
  corner20   the corner's 30 dyn/t^2 taken with 20                          tsmall   6.9e15
  kt010      0.11 kt t^-0.9 taken with 0.1                                  tlarge   3.5e12
  lo_swap    the first and the last piece's lo swapped                      real     1.9e12
  shift001   the repair's + 0.01 dropped (the shifted matrix is singular)   tsmall   inf (no factorisation)
  guard1     the guard's 0.95 taken as 1 (t' = 0)                           tsmall   inf (no finite energy)
  dual_prez  the dual ascent formed with the pre-step z                     dual     6.3e13
  backoff05  the back-off factor 0.8 taken as 0.5                           tsmall   1.8e12
"""
import numpy as np
import pytest
from mpmath import mp, mpf

import slack_ref as S

TAGS = [sh[0] for sh in S.SHAPES]


def _cases(pkg, scenes, tag):
    sh = S.shape(tag)
    return [(c, S.case_records(pkg, scenes, sh, c)) for c in S.cases(pkg, scenes, sh)]


# ---- derivatives --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,name,piece", [("dual", "it12", (0, 1)), ("tsmall", "it12*0.01", (1, 0)), ("param", "mu10,kt0.1,tsmall", (0, 2))])
def test_analytic_derivatives_equal_central_differences(pkg, scenes, cls, name, piece):
    """all 19 unknowns of one piece per class (the cross row -5 g1/t and the corner 30 dyn/t^2 + 0.11 kt t^-0.9 + mu among them): every entry to 1e-20 of the largest"""
    sh = S.shape(S.BASE)
    c = next(c for c in S.cases(pkg, scenes, sh) if c[:2] == (cls, name))
    pr = S.problem(pkg, c[3], S.scene_of(scenes, sh)["ks"], sh[2], c[2], *piece)
    g, H = S.grad_hess(pr)
    fg, fH = S.fd_grad_hess(pr)
    with mp.workdps(80):
        gm, hm = max(abs(v) for v in g), max(abs(v) for row in H for v in row)
        assert all(g[i] != 0 for i in range(19)) and all(H[18][i] != 0 for i in range(19))
        for i in range(19):
            assert abs(fg[i] - g[i]) <= mpf("1e-20") * gm, (cls, i)
            for k in range(19):
                assert abs(fH[i][k] - H[i][k]) <= mpf("1e-20") * hm, (cls, i, k)


# ---- the port -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["P2", "P3", "single", "coupled"])      # (every class, mode and mapping; P = 5, 11 are the same formulas on more pieces)
def test_port_oracle_lies_inside_the_yardsticks_bars(pkg, scenes, tag):
    """the project's CPU port (the oracle's stage_slack) on every case: on every decidable piece its four outputs lie within K r_class of the truth at the truth's k, as the
    device's must -- the restatement and the formulas the product ports are the same update -- and the stage leaves the spline and piece_time alone"""
    from oracle.pyoracle import Engine
    sh = S.shape(tag)
    cases = _cases(pkg, scenes, tag)
    rb = {cls: S.class_bars(pkg, scenes, sh, cls) for cls in S.CLASSES}
    for c, recs in cases:
        cls, name, st, par = c
        e = Engine("port", S.scene_of(scenes, sh), par)      # (one engine is live at a time: the port keeps its state in globals)
        e.set_state(st)
        e.stage_slack()
        post = e.get_state()
        assert np.array_equal(post["spline"], st["spline"]) and np.array_equal(post["piece_time"], st["piece_time"])
        rp, rd = rb[cls]
        for u, sp, tr, yd in recs:
            if tr["undecidable"]:
                continue
            m = S.measure(tr, S.state_outputs(post, u, sp))
            assert S.inside(m, rb[cls]), (tag, cls, name, u, sp, m[0] / rp, m[2] / rd, m[3])


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_cases_meet_what_the_gpu_tests_rely_on(pkg, scenes, tag):
    sh = S.shape(tag)
    P = sh[2]
    cases = _cases(pkg, scenes, tag)
    by = {cls: [(c, r) for c, recs in cases if c[0] == cls for r in recs] for cls in S.CLASSES}
    assert all(by[cls] for cls in S.CLASSES)
    dec = lambda cls: [tr for _, (_, _, tr, _) in by[cls] if not tr["undecidable"]]
    assert not any(tr["repaired"] for tr in dec("real") + dec("tlarge"))
    assert all(tr["repaired"] for tr in dec("tsmall"))
    assert max(tr["k"] for tr in dec("tsmall") if tr["guard"]) >= 4
    assert any(tr["k"] == 0 and not tr["guard"] for cls in S.CLASSES for tr in dec(cls))
    # the edge twins: indefinite below, definite above, both decidable in the eigenvalue -- ten bars from 0
    for c, (_, _, tr, _) in by["edge"]:
        assert tr["why"] != "eigenvalue" and tr["repaired"] == c[1].endswith("-"), (tag, c[1])
        assert 5 * tr["ebar"] < abs(float(tr["ev"])) < 20 * tr["ebar"], (tag, c[1], float(tr["ev"]), tr["ebar"])
    # both n = 13 mappings and n = 19 in every case (P = 2: the two n = 13 ones alone)
    for c, recs in cases:
        forms = {(tr["n"], tr["lo"]) for _, _, tr, _ in recs}
        assert forms == ({(13, 2), (13, 0)} if P == 2 else {(13, 2), (13, 0), (19, 0)}), (tag, c[:2])
        und = sum(tr["undecidable"] for _, _, tr, _ in recs)
        assert und <= 0.05 * len(recs), (tag, c[:2], [tr["why"] for _, _, tr, _ in recs])
        for _, _, tr, yd in recs:
            # the guard's own comparison t + x_t <= 0 is far from a tie, and the search ends below the loop cap
            assert abs(float(tr["c"]["tz"] + tr["t_dir"])) > 1e-6 * float(tr["c"]["tz"]) and tr["k"] < S.LOOP_CAP
            assert tr["undecidable"] or (yd["k"] == tr["k"] and yd["guard"] == tr["guard"] and yd["repaired"] == tr["repaired"]), (tag, c[:2])
    # the dual class moves every block: non-zero duals, a slack away from C x
    for _, (_, _, tr, _) in by["dual"]:
        assert all(v != 0 for v in tr["c"]["lam"]) and tr["c"]["lt"] != 0


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------
FAULT_CASES = {"cross4": "tsmall", "corner20": "tsmall", "kt010": "tlarge", "lo_swap": "real", "shift001": "tsmall", "guard1": "tsmall", "dual_prez": "dual", "backoff05": "tsmall"}


@pytest.mark.parametrize("fault", S.FAULTS)
def test_planted_fault_misses_the_bars(pkg, scenes, fault):
    """each fault in the yardstick, on the class named, is at least 1000 bars out; the clean yardstick is inside them (at 1.0 by construction).  The repair's fitted shift is
    granted to the faulty yardstick as it is to the device"""
    assert set(FAULT_CASES) == set(S.FAULTS) and len(S.FAULTS) >= 8
    cases = _cases(pkg, scenes, S.BASE)
    cls = FAULT_CASES[fault]
    rp, rd = S.class_bars(pkg, scenes, S.shape(S.BASE), cls)
    worst = clean = 0.0
    for c, recs in cases:
        if c[0] != cls:
            continue
        for u, sp, tr, yd in recs:
            if tr["undecidable"]:
                continue
            m = S.measure(tr, yd)
            clean = max(clean, m[0] / rp, m[2] / rd)
            m = S.measure(tr, S.yard(tr["pr"], fault))
            worst = max(worst, m[0] / rp, m[2] / rd)
    print("PLANTED", fault, cls, "misses K r_class by a factor %.3g" % (worst / S.K))
    assert clean <= 1.0
    assert worst > 1000 * S.K, (fault, worst)
