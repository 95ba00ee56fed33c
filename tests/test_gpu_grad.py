"""The per-piece gradient and Hessian blocks (k_grad) and the line search's energy (x_energy_group, through k_energy) against a 60-digit truth: PRODUCT kernels only,
through the stage API -- set_state -> stage_planes() or set_planes() -> run_stage("grad") -> local_grad(u, sp) for every block, energy() for every robot -- and, for the
folded launch, through one iteration of the default chain.  tests/grad_ref.py holds the truth (mpmath), the yardstick (the same formulas in plain fp64) and the states;
tests/test_grad_ref.py shows on the CPU that the truth's derivatives are the finite differences of its energy, that the inputs meet the conditions relied on here
(mask words, plane counts, undecidable blocks) and that six planted one-line faults each miss these bars by more than a factor 1000.

Shapes (grad_ref.SHAPES; fleets of two, mode 0: one robot): res = 1, 7, 8, 9, 15, 16 at P = 3; P = 2, 5, 11 at res = 8; mode 0 (scn_a), mode 2 and parameter set A at
P = 3, res = 8.  Classes: (a) the oracle's states after 0, 3, 12 iterations and (b) the same with per-robot times and seeded slack / dual blocks, on the lists the
device builds for them; (c) limits that bind, twice -- c_dense: every record within a margin of the peak, every mask word full; c_tight: the state's own pace, few
records close to the limit, idle segments between active ones, indefinite blocks -- on empty lists; syn: synthetic lists with 0 .. 100 planes per segment; syn_npl8: the
same under TJ_GRAD_NPL=8; (d) a violated limit, a hull point behind a plane, and their twins just on the finite side (energy only).  The base shape (res = 8, P = 3)
runs every state of (a) and (b), the others a12 and b12 (after twelve iterations every scene carries planes).

Bars.  |device - truth| <= K r_class A per entry, A the entry's magnitude sum and r_class the yardstick's worst |yardstick - truth| / A over the same case (floored
at u = 2^-53), for the gradient, the Hessian and the energy alike; K = 8 for every cell.  A block is repaired iff the truth's smallest eigenvalue (mpmath.eigsy) is not
positive -- counted through the rise of llt_fail_piece -- and a repaired block's diagonal is the truth's plus ONE shift: the 19 recovered shifts agree within the
entries' own bars plus the two roundings of the repair's additions (the blocks are read back after the repair, so "bit for bit" is decidable only up to that).  The
device takes the eigenvalue of ITS block, so against the truth's -lambda_min + 0.01 the shift may differ by the eigenvalue bar 1e-12 max(1, |H|_max) plus what the entries'
errors move an eigenvalue by (Weyl: |dH|_F <= K r_class |A|_F); the eigenvalue bar itself is asserted where it is decidable without that: the smallest eigenvalue of the
repaired block as read back (mpmath.eigsy) is 0.01 within the bar -- it is 0.01 + (lambda_min(H_dev) - ev).  Blocks whose lambda_min lies within that bar of 0 are left out of the
repaired / unrepaired assertion (none occurs; at most 5 % are allowed).  energy() is +inf exactly where the truth is.

Forms, asserted from the plan record and the lists, not assumed:
  k_grad    one-group launch: every stage-API case (tj_run_stage never folds).  Folded launch (grad_fold == 1): test_default_chain, one iteration of the default chain at
            res = 8, 16 (the second basis register), modes 0, 1, 2 -- a batch of one iteration arms no asynchronous front (only a FOLLOWING iteration's k_front runs
            next to the line search), so get_planes() returns the lists that iteration's k_grad consumed.
            LDS staging: the device's own lists (no segment of theirs exceeds grad_npl).  Several batches and the HBM staging path (a segment above grad_npl): syn (65, 100 > 64), syn_npl8 (17 > 8).
  energy    affine layout with eight groups: every shape but P = 11 (lsl_affine == 0, lsl_groups == 4).  Four-pass loop: robot 0 of syn (>= 43 planes); its tail alone:
            robot 1 (< 43).  Global-list path: P = 11's robot 0 carries more planes than lsl_plane_cap (716 there), the only shape of this file where a list can.

Observed on MI355X (TJ_PRINT_OBSERVED=1 prints them): largest |device - truth| / (r_class A) over all shapes; r_class in units of u (smallest .. largest over the shapes);
blocks repaired; largest |lambda_min(repaired block) - 0.01| over the eigenvalue bar:
  class       launch      blocks   energy   r_class blocks (u)   r_class energy (u)   repaired   eigenvalue
  a0, a3      one-group   1.0      0.32     50 .. 70             1 .. 2.6             0          -
  a12         one-group   1.0      1.0      2.5e3 .. 2.1e6       1.3 .. 282           41         1.3e-4
  b0, b3      one-group   1.0      0.022    50 .. 70             1                    0          -
  b12         one-group   1.0      1.0      31 .. 8.5e4          1 .. 30              4          5.5e-5
  c_dense     one-group   1.0      0.70     5.2e2 .. 5.4e5       1                    0          -
  c_tight     one-group   1.0      5.3      1.2e3 .. 9.1e5       1.9 .. 119           19         6.5e-5
  syn         one-group   1.0      1.0      51 .. 1.6e3          1 .. 2.8             0          -
  syn_npl8    one-group   1.0      1.0      51 .. 1.6e3          1 .. 2.8             0          -
  a12         folded      1.0      -        8.4e4 .. 3.1e5       -                    15         < 1e-3
  (d)         k_energy    -        1.04     -                    -                    -          -
K = 8 in every cell.  The blocks never leave the yardstick's own worst (1.0: the hulls, the distances and the records are the same operations in both, and the error
of an entry is dominated by the rounding of d and of d/m under the logarithm -- which is also why r_class reaches 1e6 u where a record or a hull point sits at 2 % of the
margin: b'' grows like 1/d^2).  The energy's 5.3 is res = 1's c_tight: the yardstick landed within 1.9 u of the truth there, the device's butterfly sum within 10 u; with
the next largest at 1.04 a bar of twice the largest observation would be 10, and 8 -- the Newton solve's factor -- holds with room, so it is kept.
"""
import math
import os

import numpy as np
import pytest
from mpmath import mp, mpf

import grad_ref as G

pytestmark = pytest.mark.gpu
K = 8.0


def _obs(what, val):
    if os.environ.get("TJ_PRINT_OBSERVED"):
        print("OBSERVED grad", what, val)


# ---- contexts: those of one shape at a time ---------------------------------------------------------------------------------------------
_CTX = {"tag": None, "ctx": {}}


def close_all():
    for s in _CTX["ctx"].values():
        s.close()
    _CTX["ctx"] = {}


def context(pkg, scenes, sh, par, npl=None):
    if _CTX["tag"] != sh[0]:
        close_all()
        _CTX["tag"] = sh[0]
    key = (par["vel_limit"], par["acc_limit"], npl)
    if key not in _CTX["ctx"]:
        with pytest.MonkeyPatch.context() as mp_:
            mp_.delenv("TJ_GRAD_NPL", raising=False)
            if npl:
                mp_.setenv("TJ_GRAD_NPL", str(npl))
            s = pkg.Solver(G.scene_of(scenes, sh[1], sh[2], G.fleet(sh)), par, stop=0.0)
        s.plan = pkg.plan_record(ctx=s._ctx)[1]
        assert s.plan["grad_npl"] == (npl or 64) and s.plan["res"] == sh[3] and s.plan["P"] == sh[2]
        assert (s.plan["lsl_affine"], s.plan["lsl_groups"]) == ((0, 4) if sh[2] == 11 else (1, 8)), (sh[0], s.plan["lsl_affine"], s.plan["lsl_groups"])
        _CTX["ctx"][key] = s
    return _CTX["ctx"][key]


def staging_forms(counts, npl, res):
    """which of k_grad's plane paths the lists reach: the batches of a block are filled greedily up to npl planes, a longer segment goes through the HBM scratch"""
    forms = set()
    for row in np.asarray(counts).reshape(-1, res):
        sb, nb = 0, 0
        while sb < res:
            se, tot = sb, 0
            while se < res and (se == sb or tot + row[se] <= npl):
                tot += row[se]; se += 1
            if tot > 0:
                nb += 1
                forms.add("hbm" if tot > npl else "lds")
            sb = se
        if nb > 1:
            forms.add("batches")
    return forms


def read_blocks(s):
    return [[s.local_grad(u, sp) for sp in range(s.P)] for u in range(s.U)]


# ---- one case on the device, its truth (kept per (shape, class): syn_npl8 shares syn's) -------------------------------------------------
_TRUTH = {}


def truth_of(key, pkg, par, P, st, counts, planes):
    if key not in _TRUTH:
        probs = G.problems(pkg, par, P, st, counts, planes)
        blocks, ener = G.fleet_truth(probs)
        _TRUTH[key] = (np.array(counts), np.array(planes), blocks, ener, G.bars(blocks, ener))
    c, p, blocks, ener, bars = _TRUTH[key]
    assert np.array_equal(c, counts) and np.array_equal(p, planes)      # the same inputs
    return blocks, ener, bars


def run_case(pkg, scenes, tag, cls):
    sh = G.shape(tag)
    _, mode, P, res, _ = sh
    U = G.fleet(sh)
    npl = 8 if cls == "syn_npl8" else None
    st, par, kind = G.case(pkg, scenes, sh, "syn" if npl else cls)
    s = context(pkg, scenes, sh, par, npl)
    s.set_state(st)
    counts, planes = s.stage_planes()
    if kind == "own":
        assert counts.sum() > 0 and "lds" in staging_forms(counts, s.plan["grad_npl"], res) <= {"lds", "batches"}
    elif kind == "none":
        counts, planes = np.zeros((U, P * res), dtype=np.int32), np.zeros((0, 4))
        s.set_planes(counts, planes)
    else:
        counts = G.synthetic_counts(U, P, res, big=s.plan["lsl_plane_cap"] if P == 11 else 0)
        planes = G.synthetic_planes(pkg, par, P, st, counts, 5)
        s.set_planes(counts, planes)
        assert ({"lds", "hbm", "batches"} if res >= 7 else {"hbm"}) <= staging_forms(counts, s.plan["grad_npl"], res)      # (res = 1: a block is one segment, one batch)
        assert counts[0].sum() >= 43 and (U == 1 or counts[1].sum() < 43)                       # the energy's four-pass loop, and its tail alone
        assert P != 11 or counts[0].sum() > s.plan["lsl_plane_cap"] >= counts[1].sum()          # the energy's global-list path next to the LDS-resident one
    before = s.stats()["llt_fail_piece"]
    s.run_stage("grad")
    dev = read_blocks(s)
    rise = s.stats()["llt_fail_piece"] - before
    E = s.energy()
    assert s.stats()["error_bits"] == 0
    blocks, ener, bars = truth_of((tag, "syn" if npl else cls), pkg, par, P, st, counts, planes)
    return dev, rise, E, blocks, ener, bars


def check_blocks(dev, rise, blocks, rb, where):
    """every entry inside its bar; repaired iff the truth says so; one shift on the diagonal, the truth's -> (worst entry ratio, worst |lambda_min(repaired block) - 0.01| over
    the eigenvalue bar, repaired blocks)"""
    worst, worst_s, n_rep, n_und = 0.0, 0.0, 0, 0
    for u, row in enumerate(blocks):
        for sp, b in enumerate(row):
            g, H = dev[u][sp]
            assert np.array_equal(H, H.T), (where, u, sp)
            r_all, r_off = G.block_ratio(b, g, H, rb), G.block_ratio(b, g, H, rb, diag=False)
            assert r_off <= K, (where, u, sp, r_off)
            worst = max(worst, r_off)
            with mp.workdps(G.DPS):
                sh = [mpf(float(H[i][i])) - b["H"][i][i] for i in range(19)]
                hmax = max(abs(float(b["H"][i][k])) for i in range(19) for k in range(19))
                ebar = G.EIG_BAR * max(1.0, hmax)
                slack = [K * rb * b["AH"][i][i] + 2 * G.U64 * abs(H[i][i]) for i in range(19)]      # the entry's own bar, and the two roundings of H_ii - ev + 0.01
                one_shift = float(max(sh) - min(sh)) <= 2 * max(slack)
                # the device's eigenvalue is that of ITS block: lambda_min moves by at most |dH|_2 <= |dH|_F <= K r |A|_F (Weyl) against the truth's ...
                weyl = K * rb * float(np.linalg.norm(b["AH"]))
                as_repaired = one_shift and all(abs(sh[i] - b["shift"]) <= ebar + weyl + slack[i] for i in range(19))
                s_err = 0.0
                if as_repaired and (b["repaired"] or b["undecidable"]):
                    # ... and held to the eigenvalue bar itself on the block it was taken from: the repaired block is H_dev + (0.01 - ev) I, so ITS smallest eigenvalue is
                    # 0.01 + (lambda_min(H_dev) - ev) -- 0.01 within the bar (and the diagonal's roundings)
                    lmin_r = G.repair(H.tolist())[0]
                    s_err = float(abs(lmin_r - mpf("0.01"))) / (ebar + max(2 * G.U64 * abs(H[i][i]) for i in range(19)))
                    as_repaired = s_err <= 1.0
            as_plain = r_all <= K
            if b["undecidable"]:
                n_und += 1
                assert as_plain or as_repaired, (where, u, sp)
            elif b["repaired"]:
                n_rep += 1
                assert as_repaired, (where, u, sp, s_err, [float(x) for x in sh])
                worst_s = max(worst_s, s_err)
            else:
                assert as_plain, (where, u, sp, r_all)
                worst = max(worst, r_all)
    assert n_rep <= rise <= n_rep + n_und, (where, rise, n_rep, n_und)
    assert n_und <= 0.05 * sum(len(r) for r in blocks), (where, n_und)
    return worst, worst_s, n_rep


def check_energy(E, ener, re, where):
    worst = 0.0
    for u, en in enumerate(ener):
        r = G.energy_ratio(en, float(E[u]), re)
        assert r <= K, (where, u, float(E[u]), float(en[0]), r)
        worst = max(worst, r)
    return worst


CASES = [(sh[0], cls) for sh in G.SHAPES for cls in (G.CLASSES_BASE if sh[0] == G.BASE else G.CLASSES) + ("syn_npl8",)]


@pytest.mark.parametrize("tag,cls", CASES)
def test_blocks_and_energy_against_the_truth(pkg, scenes, tag, cls):
    dev, rise, E, blocks, ener, (rb, re) = run_case(pkg, scenes, tag, cls)
    wb, ws, n_rep = check_blocks(dev, rise, blocks, rb, (tag, cls))
    we = check_energy(E, ener, re, (tag, cls))
    _obs((tag, cls), dict(blocks=float("%.2g" % wb), energy=float("%.2g" % we), eig_over_bar=float("%.2g" % ws), repaired=n_rep,
                          r_blocks_u=float("%.3g" % (rb / G.U64)), r_energy_u=float("%.3g" % (re / G.U64))))
    if (tag, cls) == CASES[-1]:
        close_all()


@pytest.mark.parametrize("tag", ["res8", "res16", "single", "coupled"])
def test_default_chain(pkg, scenes, tag):
    """the folded launch: one iteration of the default chain from the oracle's state after twelve, the blocks it left against the truth at that state for the plane SET
    the iteration built (the truth does not depend on the order of a list)"""
    sh = G.shape(tag)
    st, par, _ = G.case(pkg, scenes, sh, "a12")
    s = pkg.Solver(G.scene_of(scenes, sh[1], sh[2], G.fleet(sh)), par, stop=0.0)
    assert pkg.plan_record(ctx=s._ctx)[1]["grad_fold"] == 1
    s.set_state(st)
    before = s.stats()["llt_fail_piece"]
    s.iterate(1)
    dev = read_blocks(s)
    counts, planes = s.get_planes()
    rise = s.stats()["llt_fail_piece"] - before
    assert s.stats()["error_bits"] == 0
    s.close()
    assert counts.sum() > 0
    blocks, ener, (rb, re) = truth_of((tag, "chain"), pkg, par, sh[2], st, counts, planes)
    wb, ws, n_rep = check_blocks(dev, rise, blocks, rb, (tag, "chain"))
    _obs((tag, "chain"), dict(blocks=float("%.2g" % wb), repaired=n_rep, r_blocks_u=float("%.3g" % (rb / G.U64))))


def test_violated_states_have_infinite_energy(pkg, scenes):
    """(d): energy() is exactly +inf where a limit is violated or a hull point lies behind a plane, and inside the bars on the twin just on the finite side"""
    sh = G.shape(G.BASE)
    st, par, _ = G.case(pkg, scenes, sh, "c_tight")
    s = context(pkg, scenes, sh, par)
    zero = (np.zeros((2, 24), dtype=np.int32), np.zeros((0, 4)))
    edge = G.edge_time(pkg, par, 3, st, 0)
    seen = []

    def one(s, tw, par, counts, planes, want_inf, what):
        s.set_state(tw)
        s.stage_planes()
        s.set_planes(counts, planes)
        E = s.energy()
        probs = G.problems(pkg, par, 3, tw, counts, planes)
        ener = []
        for pr in probs:
            yE, AE = G.yard_energy(pr)
            ener.append((G.robot_energy(pr), AE, yE))
        assert (ener[0][0] == mp.inf) == want_inf and ener[1][0] != mp.inf
        assert (E[0] == math.inf) == want_inf and math.isfinite(E[1]), (what, E)
        re = max([G.U64] + [G.energy_ratio(en, en[2]) for en in ener if en[0] != mp.inf])
        seen.append((what, check_energy(E, ener, re, what)))
        assert s.stats()["error_bits"] == 0

    for f, want_inf in ((1 - 1e-9, True), (1 + 1e-9, False)):
        tw = {k: v.copy() for k, v in st.items()}
        tw["piece_time"][0] = edge * f
        one(s, tw, par, *zero, want_inf, ("limit", want_inf))
    st, par, _ = G.case(pkg, scenes, sh, "syn")
    s = context(pkg, scenes, sh, par)
    counts = G.synthetic_counts(2, 3, 8)
    for d, want_inf in ((-1e-9, True), (1e-9, False)):
        one(s, st, par, counts, G.synthetic_planes(pkg, par, 3, st, counts, 5, behind=(0, 0, d)), want_inf, ("plane", want_inf))
    _obs("violated", seen)
    close_all()
