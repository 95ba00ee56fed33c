"""CPU: tests/grad_ref.py checks itself -- the truth's derivatives against finite differences of the truth's energy, the project's CPU oracle inside the yardstick's
bars, the six planted faults outside them, and the conditions on the inputs that tests/test_gpu_grad.py relies on."""
import numpy as np
import pytest
from mpmath import mp, mpf

import grad_ref as G

K = 8.0      # tests/test_gpu_grad.py's factor


def _oracle_case(pkg, scenes, sh, cls):
    """the case with the CPU oracle's own plane lists where the device would build them (the same sets: tests/test_gpu_parity.py)"""
    from oracle.pyoracle import Engine
    st, par, kind = G.case(pkg, scenes, sh, cls)
    _, mode, P, res, _ = sh
    U = G.fleet(sh)
    e = None
    if kind == "own":
        e = Engine("port", G.scene_of(scenes, mode, P, U), par)
        e.set_state(st)
        counts, planes = e.stage_planes()
    elif kind == "none":
        counts, planes = np.zeros((U, P * res), dtype=np.int32), np.zeros((0, 4))
    else:
        counts = G.synthetic_counts(U, P, res)
        planes = G.synthetic_planes(pkg, par, P, st, counts, 5)
    return G.problems(pkg, par, P, st, counts, planes), e


_TRUTH = {}


def _truth(pkg, scenes, tag, cls):
    if (tag, cls) not in _TRUTH:
        probs, e = _oracle_case(pkg, scenes, G.shape(tag), cls)
        blocks, ener = G.fleet_truth(probs)
        _TRUTH[tag, cls] = (probs, blocks, ener, G.bars(blocks, ener), e)
    return _TRUTH[tag, cls]


# ---- derivatives ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,block", [("a12", (0, 1)), ("b3", (1, 0)), ("c_dense", (0, 1)), ("c_tight", (0, 1)), ("syn", (0, 0))])
def test_analytic_derivatives_equal_central_differences(pkg, scenes, cls, block):
    """one block per state class at P = 2, res = 4 (the formulas do not depend on the size; 760 energies at 80 digits per block): every entry to 1e-20 of its magnitude sum"""
    sh = ("fd", 1, 2, 4, None)
    st, par, kind = G.case(pkg, scenes, sh, cls)
    if kind == "syn":
        counts = np.array([[5, 0, 3, 17, 1, 4, 0, 3], [1, 0, 3, 0, 0, 4, 0, 0]], dtype=np.int32)
        planes = G.synthetic_planes(pkg, par, 2, st, counts, 5)
    elif kind == "own":
        from oracle.pyoracle import Engine
        e = Engine("port", G.scene_of(scenes, 1, 2, 2), par)
        e.set_state(st)
        counts, planes = e.stage_planes()
    else:
        counts, planes = np.zeros((2, 8), dtype=np.int32), np.zeros((0, 4))
    u, sp = block
    pr = G.problems(pkg, par, 2, st, counts, planes)[u]
    g, H, Ag, AH = G.piece_grad_hess(pr, sp)
    assert kind == "none" or sum(len(p) for p in pr["planes"][sp * 4:sp * 4 + 4]) > 0
    fg, fH = G.fd_grad_hess(pr, sp)
    with mp.workdps(80):
        for i in range(19):
            assert Ag[i] > 0 and abs(fg[i] - g[i]) <= mpf("1e-20") * Ag[i], (cls, i)
            for k in range(19):
                assert abs(fH[i][k] - H[i][k]) <= mpf("1e-20") * AH[i][k] or (AH[i][k] == 0 and H[i][k] == 0 and abs(fH[i][k]) < mpf("1e-25")), (cls, i, k)
        assert any(H[18][i] != 0 for i in range(18)) or kind != "none"      # the limit records reach the time column in both (c) states


def test_piece_energies_add_up_to_the_robot_energy(pkg, scenes):
    probs, blocks, ener, _, _ = _truth(pkg, scenes, G.BASE, "b3")
    with mp.workdps(G.DPS):
        for pr, en in zip(probs, ener):
            assert sum(G.piece_energy(pr, sp) for sp in range(pr["P"])) == en[0] and en[0] != mp.inf


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["a3", "a12"])
def test_oracle_lies_inside_the_yardsticks_bars(pkg, scenes, cls):
    probs, blocks, ener, (rb, re), e = _truth(pkg, scenes, G.BASE, cls)
    assert sum(len(p) for pr in probs for p in pr["planes"]) > 0
    for u, row in enumerate(blocks):
        for sp, b in enumerate(row):
            g, h = e.local_grad(u, sp)
            assert G.block_ratio(b, g, h, rb) <= K, (cls, u, sp)
        assert G.energy_ratio(ener[u], e.spline_energy(u), re) <= K, (cls, u)


# ---- planted faults -------------------------------------------------------------------------------------------------------------------------
FAULT_CASES = {"acc_tsign": "c_tight", "bit63": "c_dense", "lastplane": "syn", "e2term": "a12", "mu1818": "a12", "lam_z_piece": "b3"}


@pytest.mark.parametrize("fault", G.FAULTS)
def test_planted_fault_misses_the_bars(pkg, scenes, fault):
    """each fault in the yardstick, on the class where it bites, is at least 1000 bars out (blocks; lam_z_piece: the energy, the only place z meets Lambda)"""
    assert set(FAULT_CASES) == set(G.FAULTS)
    probs, blocks, ener, (rb, re), _ = _truth(pkg, scenes, G.BASE, FAULT_CASES[fault])
    if fault == "lam_z_piece":
        worst = max(G.energy_ratio(en, G.yard_energy(pr, fault)[0], re) for pr, en in zip(probs, ener))
    else:
        worst = max(G.block_ratio(b, *G.yard_grad_hess(pr, sp, fault), rb) for pr, row in zip(probs, blocks) for sp, b in enumerate(row))
        clean = max(G.block_ratio(b, *G.yard_grad_hess(pr, sp), rb) for pr, row in zip(probs, blocks) for sp, b in enumerate(row))
        assert clean <= 1.0
    assert worst > 1000 * K, (fault, worst)


# ---- the conditions on the inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["res8", "res16"])
def test_binding_limits_fill_the_mask_words(pkg, scenes, tag):
    sh = G.shape(tag)
    _, mode, P, res, _ = sh
    nw = (9 * res + 63) // 64
    none = (np.zeros((2, P * res), dtype=np.int32), np.zeros((0, 4)))
    st, par, _ = G.case(pkg, scenes, sh, "c_dense")
    for pr in G.problems(pkg, par, P, st, *none):
        for sp in range(P):
            bits, bad = G.active_records(pr, sp)
            assert not bad
            assert all(bits[64 * w:64 * w + 64].sum() >= 3 for w in range(nw)), (tag, sp)                                   # every mask word of every block
            assert all(bits[9 * ((64 * w - 1) // 9):9 * ((64 * w - 1) // 9) + 9].any() for w in range(1, nw)), (tag, sp)   # the 9-bit group across each word boundary
            assert res != 8 or (bits[63] and bits[64])
    st, par, _ = G.case(pkg, scenes, sh, "c_tight")
    gaps = 0
    for pr in G.problems(pkg, par, P, st, *none):
        for sp in range(P):
            bits, bad = G.active_records(pr, sp)
            assert not bad
            seg = bits.reshape(res, 9).any(axis=1)
            gaps += any(not seg[i] and seg[:i].any() and seg[i + 1:].any() for i in range(res))
    assert gaps >= 1      # a segment with no active record between two that have some


def test_synthetic_lists_hold_the_counts_the_kernels_branch_on(pkg, scenes):
    for tag in ("res8", "P11", "res1", "single"):
        _, mode, P, res, _ = G.shape(tag)
        c = G.synthetic_counts(G.fleet(G.shape(tag)), P, res, big=716 if tag == "P11" else 0)
        assert set(np.unique(c)) <= set(G.SYN_COUNTS) and c.max() <= 256
        assert {64, 65, 100} <= set(c[0]) and c[0].sum() >= 43
        if tag == "P11":
            assert c[0].sum() > 716
        if res >= 8:
            assert set(G.SYN_COUNTS) == set(np.unique(c))
            piece = c[0].reshape(P, res)
            assert any(0 < min(r[i - 1], r[i + 1]) and r[i] == 0 for r in piece for i in range(1, res - 1))      # a 0 between two non-zero counts
            assert any(r.max() <= 64 < r.sum() for r in piece)                                                     # a piece of short lists in two batches
            assert any(64 in r and 65 in r for r in piece)
        if c.shape[0] > 1:
            assert 0 < c[1].sum() < 43
    # some of a segment's six points inside the barrier's range, others beyond it, none behind the plane
    probs, _, _, _, _ = _truth(pkg, scenes, G.BASE, "syn")
    inside = outside = 0
    for pr in probs:
        for tr, pls in enumerate(pr["planes"]):
            x = pr["spline"][:, 3 * (tr // 8):3 * (tr // 8) + 6].T
            d = (pr["basis"][tr] @ x) @ pls[:, :3].T + pls[:, 3]
            assert (d > 0).all()
            inside += (d < pr["margin"]).sum(); outside += (d >= pr["margin"]).sum()
    assert inside > 200 and outside > 200


@pytest.mark.parametrize("tag", [G.BASE, "res16"])
def test_few_blocks_are_undecidable_and_some_are_repaired(pkg, scenes, tag):
    """at most 5 % of a shape's blocks have a smallest eigenvalue within the eigenvalue bar of 0 (here: none), and the (c) states hold indefinite blocks"""
    classes = G.CLASSES_BASE if tag == G.BASE else G.CLASSES
    und = tot = rep = 0
    for cls in classes:
        blocks = _truth(pkg, scenes, tag, cls)[1]
        for row in blocks:
            for b in row:
                tot += 1; und += b["undecidable"]; rep += b["repaired"] and not b["undecidable"]
    assert und <= 0.05 * tot and rep >= 1, (und, rep, tot)


def test_violated_states_have_infinite_truth_and_finite_twins(pkg, scenes):
    sh = G.shape(G.BASE)
    st, par, _ = G.case(pkg, scenes, sh, "c_tight")
    none = (np.zeros((2, 24), dtype=np.int32), np.zeros((0, 4)))
    edge = G.edge_time(pkg, par, 3, st, 0)
    for f, inf in ((1 - 1e-9, True), (1 + 1e-9, False)):
        tw = {k: v.copy() for k, v in st.items()}
        tw["piece_time"][0] = edge * f
        pr = G.problems(pkg, par, 3, tw, *none)
        assert (G.robot_energy(pr[0]) == mp.inf) == inf and G.robot_energy(pr[1]) != mp.inf
        assert (G.yard_energy(pr[0])[0] == np.inf) == inf
    st, par, _ = G.case(pkg, scenes, sh, "syn")
    counts = G.synthetic_counts(2, 3, 8)
    for d, inf in ((-1e-9, True), (1e-9, False)):
        pr = G.problems(pkg, par, 3, st, counts, G.synthetic_planes(pkg, par, 3, st, counts, 5, behind=(0, 0, d)))
        assert (G.robot_energy(pr[0]) == mp.inf) == inf and G.robot_energy(pr[1]) != mp.inf
