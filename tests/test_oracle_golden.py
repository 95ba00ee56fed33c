"""CPU: the oracle restatement (oracle/liboracle.so) against golden vectors produced by the
unmodified reference (tests/golden/make_golden.py).  This is what pins the oracle on machines where
/root/reference does not exist."""
import numpy as np
import pytest

from conftest import backoff_exponent, canon, check_scene_matches_fixture, gold, maxdiff, rel, scene_by_name
from oracle.pyoracle import Engine, Prims
from query_kit import STATE


@pytest.mark.parametrize("P", [2, 5])
def test_tables_bit_exact(scenes, P):
    g = gold(f"tables_P{P}.npz")
    sc = dict(scenes.tiny(1)); sc["P"] = P; sc["waypoints"] = sc["waypoints"][:, :P + 1]
    e = Engine("port", sc)
    conv, M, basis = e.tables()
    assert np.array_equal(conv, g["convert"])      # C2 junction blocks (CCDUtils.h:137-170)
    assert np.array_equal(M, g["mdyn"])            # jerk Gram matrix, same rounding (CCDUtils.h:172-227)
    assert np.array_equal(basis, g["basis"])       # blossom subdivision x conversion
    assert np.array_equal(e.kdop_axes(), g["kdop"])


@pytest.mark.parametrize("shape", ["6v1", "6v6", "12v1", "12v12"])
def test_gjk_witness_bit_exact(shape):
    g = gold("gjk_kat.npz")
    pr = Prims("port")
    A, B, V = g[f"gjk_{shape}_a"], g[f"gjk_{shape}_b"], g[f"gjk_{shape}_v"]
    for a, b, v in zip(A, B, V):
        got = pr.gjk(a, b)
        assert np.array_equal(got, v) or (np.isnan(got).all() and np.isnan(v).all()), (shape, got, v)


def test_planes_kdop_ccd_primitives():
    g = gold("prims_kat.npz")
    pr = Prims("port")
    for i in range(len(g["P"])):
        ok, cd = pr.plane_obs(g["P"][i], g["q"][i], 0.2)
        assert ok == bool(g["plane_obs"][i, 0])
        if ok:
            assert np.array_equal(cd, g["plane_obs"][i, 1:])            # bitwise: same GJK path, same rounding
        ok, cd = pr.plane_self(g["P"][i], g["Q"][i], 0.3, refine=True)
        assert ok == bool(g["plane_self"][i, 0])
        if ok:
            assert np.array_equal(cd[:3], g["plane_self"][i, 1:4])
            want = g["plane_self"][i, 4]
            # Newton on the offset (libm log only).  When no barrier term is active the reference
            # divides 0/0 and returns NaN (Optimal_plane.h:63-66); that quirk is reproduced.
            assert (np.isnan(want) and np.isnan(cd[3])) or abs(cd[3] - want) <= 1e-14
        assert pr.kdop_dcd(g["P"][i], g["q"][i], 0.2) == bool(g["kdop_dcd"][i])
        assert pr.kdop_self_dcd(g["P"][i], g["Q"][i], 0.3) == bool(g["kdop_self_dcd"][i])
    for i in range(len(g["ccd_P"])):
        a, da, b, db, pt = g["ccd_P"][i], g["ccd_D"][i], g["ccd_Q"][i], g["ccd_E"][i], g["ccd_q"][i]
        t1, u1 = g["ccd_t"][i]
        assert pr.kdop_ccd(a, da, pt, 0.1, 0.0, t1) == bool(g["kdop_ccd"][i])
        assert pr.gjk_ccd(a, da, pt, 0.1, 0.0, t1) == bool(g["gjk_ccd"][i])
        assert pr.self_kdop_ccd(a, da, b, db, 0.1, t1, u1) == bool(g["self_kdop_ccd"][i])
        assert pr.self_gjk_ccd(a, da, b, db, 0.1, t1, u1) == bool(g["self_gjk_ccd"][i])


def test_dynamic_tree_pair_order():
    """the inter-robot step clamp is order dependent (Step.h:184-256): the oracle must reproduce the
    pair ORDER of the reference's incrementally balanced tree, not just the set"""
    g = gold("prims_kat.npz")
    pr = Prims("port")
    for lo, hi, pairs, n in zip(g["tree_lo"], g["tree_hi"], g["tree_pairs"], g["tree_npairs"]):
        got = pr.self_pairs(lo, hi, 0.1)
        assert np.array_equal(got, pairs[:n])


def test_llt_and_min_eigenvalue():
    g = gold("prims_kat.npz")
    pr = Prims("port")
    for m, f, ev in zip(g["llt_mats"], g["llt_fails"], g["min_eig"]):
        assert pr.llt_fails(m) == bool(f)
        assert abs(pr.min_eig(m) - ev) <= 1e-12 * max(1.0, np.abs(m).max())


@pytest.mark.parametrize("name", ["tiny_multi", "tiny_single", "hard", "scn_c"])
def test_stages_teacher_forced(scenes, name):
    """every stage of one ADMM iteration, started from the reference's own state (tol 1e-12 abs per
    SURVEY 8c; planes / gnorm / CCD steps are bit-exact)"""
    g = gold(f"stages_{name}.npz")
    scene = scene_by_name(scenes, name)
    check_scene_matches_fixture(scene, g)
    port_teacher_forced(scene, g)


def port_teacher_forced(scene, g, params=None):
    """the port through the kept iterations of a decoupled / single-UAV stage fixture, each stage started from the reference's state"""
    e = Engine("port", scene, params)
    for it in g["kept"]:
        k = f"it{it}_"
        e.set_state({n: g[k + "pre_" + n] for n in ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time")})
        counts, planes = e.stage_planes()
        assert np.array_equal(counts, g[k + "counts"])
        assert np.array_equal(planes, g[k + "planes_raw"])       # same order, same bits
        d = e.stage_direction()
        assert maxdiff(d["gn"], g[k + "gn"]) <= 1e-12 * max(1.0, np.abs(g[k + "gn"]).max())  # |g|: whole gradient assembly
        assert maxdiff(d["direction"], g[k + "direction"]) <= 1e-10
        assert maxdiff(d["wolfe"], g[k + "wolfe"]) <= 1e-9 * max(1.0, np.abs(g[k + "wolfe"]).max())
        s_self, s_pos = e.stage_steps()
        assert np.array_equal(s_self, g[k + "step_self"]) and np.array_equal(s_pos, g[k + "step_pos"])
        arm = e.stage_linesearch()
        if scene["mode"] == 1:
            assert maxdiff(arm, g[k + "step_armijo"]) <= 1e-12
        st = e.get_state()
        assert maxdiff(st["spline"], g[k + "mid_spline"]) <= 1e-10
        e.set_state({n: (g[k + "mid_" + n] if n in ("spline", "piece_time") else g[k + "pre_" + n])
                     for n in ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time")})
        e.stage_slack()
        st = e.get_state()
        for n in st:
            assert maxdiff(st[n], g[k + "post_" + n]) <= 1e-12 * max(1.0, np.abs(g[k + "post_" + n]).max()), (it, n)


def test_long_armijo_loops_end_where_the_references_do(scenes):
    """A fleet stacked at exactly the barrier's range: in iteration 0 the reference's Armijo loop (Optimization3D_multi.h:792) ends by
    rounding only -- 519 ... 559 back-offs for robots whose energy is ~1e-45, 3 268 (step 2e-317, where 1e-4*wolfe*step underflows) for
    robots whose energy is exactly 0.  The oracle has to take the same number of factors (its loop bound lies beyond the fixed point of
    step *= 0.8)."""
    g = gold("stages_stack030.npz")
    scene = scene_by_name(scenes, "stack030")
    check_scene_matches_fixture(scene, g)
    want0 = backoff_exponent(g["it0_step_armijo"])
    assert want0.max() == 3268 and np.sum(want0 > 500) >= 60     # the fixture is what its name says
    e = Engine("port", scene)
    for it in g["kept"]:
        k = f"it{it}_"
        e.set_state({n: g[k + "pre_" + n] for n in ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time")})
        counts, planes = e.stage_planes()
        assert np.array_equal(counts, g[k + "counts"]) and np.array_equal(planes, g[k + "planes_raw"])
        e.stage_direction()
        s_self, s_pos = e.stage_steps()
        assert np.array_equal(s_self, g[k + "step_self"]) and np.array_equal(s_pos, g[k + "step_pos"])
        arm = e.stage_linesearch()
        assert np.array_equal(arm, g[k + "step_armijo"]), (it, backoff_exponent(arm), backoff_exponent(g[k + "step_armijo"]))


def test_ccd_backoffs_follow_the_reference(scenes):
    """Step::position_step / self_step (Step.h:89, :229) on directions scaled by 1 ... 1e21: up to 177 factors of 0.8 per robot, and --
    beyond the scale at which GJK on the swept hull loses the 0.1 offset -- the reference's clamp stops acting; same steps bit for bit
    (the port walks the candidates in the reference's own tree order, so it follows even where that order matters: scales > 1e5)"""
    g = gold("backoff_kat.npz")
    scene = scenes.hard()
    e = Engine("port", scene)
    e.set_state({n: g["pre_" + n] for n in ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time")})
    e.stage_planes(); e.stage_direction()
    assert backoff_exponent(g["step_pos"]).max() >= 170
    for i, sc in enumerate(g["scales"]):
        for u in range(scene["U"]):
            e.set_direction(u, g["direction"][u] * sc, float(g["t_direction"][u]), float(g["wolfe"][u]), float(g["gn"][u]))
        a, b = e.stage_steps()
        assert np.array_equal(a, g["step_self"][i]) and np.array_equal(b, g["step_pos"][i]), (sc, a, b)


@pytest.mark.parametrize("name", ["scn_b", "scn_a", "scn_c3"])
def test_end_to_end_vs_reference(scenes, name):
    """free-running to the mains' stop test: same iteration count, final control points AND final energy within 1e-8
    (scn_c3: 64 UAVs, 100 000 points -- north_star's sentence at its own fleet size, on a scene whose reference envelope is 6e-11)"""
    g = gold(f"e2e_{name}.npz")
    scene = scene_by_name(scenes, name)
    check_scene_matches_fixture(scene, g)
    e = Engine("port", scene)
    gn = []
    for it in range(200):
        gn.append(e.iterate())
        if it > 1 and gn[-1] < 1e-2:
            break
    assert len(gn) == int(g["iters"])
    st = e.get_state()
    assert rel(st["spline"], g["final_spline"]) <= 1e-8           # BASELINE.json tolerance
    assert rel(st["piece_time"], g["final_piece_time"]) <= 1e-8
    # the residual gradient norm is a difference of nearly cancelling terms: compare loosely
    assert abs(gn[-1] - g["gnorm_hist"][-1]) <= 1e-3 * g["gnorm_hist"][-1]
    # Energy_admm::spline_energy of every robot at the final state, against the separating planes of that state
    e.stage_planes()
    en = np.array([e.spline_energy(u) for u in range(scene["U"])])
    # the reference moves its own energies by `energy_env` under a 1-ulp input change (5.8e-8 on scn_c3, 1.1e-8 on scn_b): 1e-8 where that allows
    assert np.max(np.abs(en - g["final_energy"]) / np.abs(g["final_energy"])) <= max(1e-8, 3 * float(g["energy_env"]))


def test_triangle_body_primitives_vs_reference():
    """3-vertex obstacle bodies (BASELINE config 5): gjk 6v3 / 12v3 witness vectors, CCD::KDOPDCD and CCD::GJKDCD booleans from
    the unmodified reference; planes derived from its witness vectors (tests/golden/make_golden.py:plane_from_witness)"""
    g = gold("tri_kat.npz")
    pr = Prims("port")
    for nm in ("6v3", "12v3"):
        for a, b, v in zip(g[f"gjk_{nm}_a"], g[f"gjk_{nm}_b"], g[f"gjk_{nm}_v"]):
            got = pr.gjk(a, b)
            assert np.array_equal(got, v) or (np.isnan(got).all() and np.isnan(v).all())
    for i in range(len(g["P"])):
        ok, cd = pr.plane_tri(g["P"][i], g["tri"][i], 0.2)
        w = g["plane_tri"][i]
        assert ok == bool(w[0]) and (not ok or np.array_equal(cd, w[1:]))
        sw = np.concatenate([g["P"][i], g["P"][i] + g["t"][i] * g["D"][i]])
        assert pr.kdop_general(g["P"][i], g["tri"][i], 0.2) == bool(g["kdop_dcd_tri"][i])
        assert pr.kdop_general(sw, g["tri"][i], 0.1) == bool(g["kdop_ccd_tri"][i])
        assert pr.gjk_dcd_general(sw, g["tri"][i], 0.1) == bool(g["gjk_ccd_tri"][i])


@pytest.mark.parametrize("name", ["hard", "tiny_single"])
def test_degenerate_triangles_are_the_point_cloud_in_the_oracle(scenes, name):
    """a triangle with three equal vertices must be the cloud point, bit for bit, through whole iterations"""
    sc = scene_by_name(scenes, name)
    a = Engine("port", sc)
    st = []
    for it in range(6):
        a.iterate(); st.append(a.get_state())
    b = Engine("port", scenes.triangulate(sc, degenerate=True))
    for it in range(6):
        b.iterate()
        sb = b.get_state()
        for n in sb:
            assert np.array_equal(st[it][n], sb[n]), (it, n)


def test_inter_robot_clamp_in_the_references_tree_order():
    """Step::self_step where many colliding pairs of one segment share robots (order dependent, Step.h:213-251)"""
    from conftest import ccd_order_case
    g = gold("ccd_order_kat.npz")
    for seed in g["seeds"]:
        scene, dirs = ccd_order_case(int(seed))
        assert np.allclose([scene["cloud"].sum(), np.abs(scene["cloud"]).sum()], g[f"s{seed}_cloud_sum"], rtol=1e-13)
        assert np.array_equal(dirs, g[f"s{seed}_dirs"])
        e = Engine("port", scene)
        e.stage_planes()
        for u in range(scene["U"]):
            e.set_direction(u, dirs[u], 0.0, 1.0, 1.0)
        s_self, s_pos = e.stage_steps()
        assert np.array_equal(s_self, g[f"s{seed}_step_self"]) and np.array_equal(s_pos, g[f"s{seed}_step_pos"])


def test_single_uav_newton_solve_is_eigens_simplicial_llt():
    """Optimization3D_admm.h:470-475: SimplicialLLT with AMD ordering on h0.sparseView().  The oracle's restatement
    (oracle/orc_amd.cpp) must give Eigen's permutation and Eigen's solution BIT FOR BIT on the reduced systems of real runs
    (changing sparsity patterns as barriers switch on) and on synthetic band-arrow patterns."""
    g = gold("amd_kat.npz")
    pr = Prims("port")
    for H, b, order, x in zip(g["H"], g["g"], g["order"], g["x"]):
        ok, got, o = pr.sparse_llt_solve(H, b)
        assert ok and np.array_equal(o, order) and np.array_equal(got, x)


def test_single_uav_piece_hessians_bitwise(scenes):
    """per-piece 19x19 Hessian blocks BEFORE the PSD shift (Gradient_admm.h:67-164), incl. Eigen's evaluation order of
    `e2*d_x*d_x^T + e1*A^T*h_p*A` (depth-1 GEMM with alpha = e2; the triple product through two GEMM calls): bit-exact.
    What is left between the oracle and the reference on the single-UAV path is the smallest eigenvalue of the PSD
    repair (Eigen's vectorised Householder sums in an order that depends on memory alignment; both are within 1e-16 of
    the matrix norm of the true value, i.e. they differ by an ulp of the diagonal they shift)."""
    g = gold("amd_kat.npz")
    k = 0
    for sc in (scenes.scn_a(n_points=20000, seed=7), scene_by_name(scenes, "hard_single")):
        e = Engine("port", sc)
        U, P, T = 1, sc["P"], 3 * sc["P"] + 3
        for _ in range(3):
            flat = g["lh_state"][k]
            sizes = [("spline", (U, 3, T)), ("p_slack", (U, 3, 6 * P)), ("p_lambda", (U, 3, 6 * P)), ("t_slack", (U, P)), ("t_lambda", (U, P)), ("piece_time", (U,))]
            st, w = {}, 0
            for name, shp in sizes:
                n = int(np.prod(shp)); st[name] = flat[w:w + n].reshape(shp); w += n
            e.set_state(st)
            e.stage_planes()
            for spc in range(P):
                # the fixture holds Eigen's column-major memory, i.e. [col][row]; the reference's blocks are symmetric only up to
                # rounding (entry (r,c) and (c,r) associate ((e1*w_r)*h_p)*w_c differently) and the solvers read the LOWER triangle
                assert np.array_equal(e.local_grad(0, spc)[1], g["lh_blocks"][k][spc].T), (k, spc)
            k += 1


SINGLE_FLOOR = 5e-8


@pytest.mark.parametrize("name,floor", [("scn_a", 1e-8), ("scn_a_seed7", SINGLE_FLOOR), ("hard_single", SINGLE_FLOOR)])
def test_single_uav_free_running_vs_reference(scenes, name, floor):
    """Single-UAV mode (ks = 1e-8, Newton system conditioned ~1e8) to the mains' stop test against the unmodified reference:
    same iteration count; final control points within max(floor, 3 x the reference's own 1-ulp envelope).
    floor: 1e-8 (BASELINE's bar) on the golden SCN-A; 5e-8 on the other seeds.  With the AMD-ordered sparse solve and Eigen's
    evaluation order of the Hessian terms restated, the oracle differs from the reference in ONE quantity: the smallest
    eigenvalue of the per-piece PSD repair (both within 1e-16 of the block's norm of the true value, i.e. an ulp of the diagonal
    they shift).  The reference amplifies such an ulp ~1e6-fold over the 40-55 iterations of these runs (its own mid-run 1-ulp
    divergence reaches 2e-8 on SCN-A, `div_hist` in the fixtures), so 1e-8 is met or missed by a factor ~2 depending on the seed;
    measured here: 2e-9 (SCN-A), 1.2e-8 (seed 7), 5e-6 on hard_single, whose own envelope is 2e-5."""
    g = gold(f"envelope_{name}.npz")
    scene = {"scn_a": scenes.scn_a, "scn_a_seed7": lambda: scenes.scn_a(n_points=20000, seed=7), "hard_single": lambda: scene_by_name(scenes, "hard_single")}[name]()
    check_scene_matches_fixture(scene, g)
    e = Engine("port", scene)
    gn = []
    for it in range(200):
        gn.append(e.iterate())
        if it > 1 and gn[-1] < 1e-2:
            break
    assert len(gn) == int(g["iters"])
    env = rel(g["final_spline_pert"], g["final_spline"])
    assert rel(e.get_state()["spline"], g["final_spline"]) <= max(floor, 3 * env), (rel(e.get_state()["spline"], g["final_spline"]), env)


def envelope_check(g, snapshots, final, iters):
    """Shared by the CPU (oracle) and GPU (HIP) tests of the headline scene.  `g` = tests/golden/envelope_scn_c.npz, made
    from two runs of the unmodified reference whose inputs differ by ONE ULP.  An implementation must (1) track the
    reference's control points at the early snapshot iterations as closely as the reference tracks itself (floor 1e-10: a
    different libm / summation order is a perturbation of the same kind as the 1-ulp input change), (2) converge in the
    reference's iteration count +-1, (3) end no farther from the reference than 3x the reference's own 1-ulp envelope.
    The fixture also records that this envelope is ~1e-2 >> 1e-8: BASELINE's end-to-end 1e-8 is not attainable on this
    scene by anything that is not bit-identical to the reference in every operation, the reference under a 1-ulp input
    change included."""
    div = g["div_hist"]
    assert div[int(g["iters"]) - 1] > 1e-4, "fixture: the reference no longer leaves itself on this scene -- tighten this test to 1e-8"
    for it in g["snap"]:
        tol = max(1e-10, 30 * float(div[it]))
        assert rel(snapshots[int(it)], g[f"it{it}_spline"]) <= tol, (int(it), rel(snapshots[int(it)], g[f"it{it}_spline"]), tol)
    assert abs(iters - int(g["iters"])) <= 1
    env = rel(g["final_spline_pert"], g["final_spline"])
    assert rel(final, g["final_spline"]) <= 3 * env, (rel(final, g["final_spline"]), env)
    # ... and no farther than 20x the distance this repository's CPU restatement ends at (1.2e-5, measured against this very
    # fixture; the HIP path: 4.7e-5 in round 2): the envelope alone (3.6e-2) would let a 100x regression through
    assert rel(final, g["final_spline"]) <= 20 * 1.2e-5, rel(final, g["final_spline"])


def test_headline_scene_free_running_within_reference_envelope(scenes):
    g = gold("envelope_scn_c.npz")
    scene = scene_by_name(scenes, "scn_c")
    check_scene_matches_fixture(scene, g)
    e = Engine("port", scene)
    gn, snaps = [], {}
    for it in range(200):
        gn.append(e.iterate())
        if it in g["snap"]:
            snaps[it] = e.get_state()["spline"]
        if it > 1 and gn[-1] < 1e-2:
            break
    envelope_check(g, snaps, e.get_state()["spline"], len(gn))


# ---- coupled mode ("decouple":0): Optimization3D_multi::optimization, one shared piece_time ----------------


def test_coupled_stages_teacher_forced(scenes):
    """planes -> update_spline (arrowhead Newton system, couple_self_step, Armijo on the summed energy) ->
    slack/dual, each started from the reference's own state"""
    g = gold("stages_hard_coupled.npz")
    scene = scene_by_name(scenes, "hard_coupled")
    check_scene_matches_fixture(scene, g)
    port_coupled_teacher_forced(scene, g)


def port_coupled_teacher_forced(scene, g, params=None):
    e = Engine("port", scene, params)
    for it in g["kept"]:
        k = f"it{it}_"
        e.set_state({n: g[k + "pre_" + n] for n in STATE})
        counts, planes = e.stage_planes()
        assert np.array_equal(counts, g[k + "counts"])
        assert np.array_equal(canon(counts, planes), g[k + "planes"])
        gnorm, wolfe = e.stage_update_spline()
        assert abs(gnorm - g[k + "gnorm"]) <= 1e-11 * max(1.0, float(g[k + "gnorm"]))
        assert abs(wolfe - g[k + "wolfe"]) <= 1e-9 * max(1.0, abs(float(g[k + "wolfe"])))
        st = e.get_state()
        assert maxdiff(st["spline"], g[k + "mid_spline"]) <= 1e-10
        assert maxdiff(st["piece_time"], g[k + "mid_piece_time"]) <= 1e-10
        e.set_state({n: (g[k + "mid_" + n] if n in ("spline", "piece_time") else g[k + "pre_" + n]) for n in STATE})
        e.stage_slack()
        st = e.get_state()
        for n in st:
            assert maxdiff(st[n], g[k + "post_" + n]) <= 1e-12 * max(1.0, np.abs(g[k + "post_" + n]).max()), (it, n)


def test_coupled_end_to_end_vs_reference(scenes):
    g = gold("e2e_scn_b_coupled.npz")
    scene = scene_by_name(scenes, "scn_b_coupled")
    check_scene_matches_fixture(scene, g)
    e = Engine("port", scene)
    gn = []
    for it in range(200):
        gn.append(e.iterate())
        if it > 1 and gn[-1] < 1e-2:
            break
    assert len(gn) == int(g["iters"])
    st = e.get_state()
    assert rel(st["spline"], g["final_spline"]) <= 1e-8
    assert rel(st["piece_time"], g["final_piece_time"]) <= 1e-8
    assert np.all(st["piece_time"] == st["piece_time"][0])   # one piece_time for every robot
