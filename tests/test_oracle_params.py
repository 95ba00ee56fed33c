"""CPU: the solver away from the shipped Config_File/3D.json values.

The shipped values pair up -- margin == offset (0.1), vel_limit == acc_limit (2.0), kt == 1, lambda == 1/mu (10, 0.1) -- so a
kernel that swaps, drops or inverts one of them computes the same numbers there.  Sets A and B break every pair (in opposite
directions where there is one).  The fixtures tests/golden/*_params[AB].npz come from the unmodified reference under these sets
(tests/golden/make_golden.py --params-only, which holds the same two dicts).  Each stage fixture also records a TWIN CHECK: the
reference rerun on the same kept iterations with margin/offset swapped, vel/acc swapped, lambda/mu inverted, kt = 1, and each
value alone scaled by 1 + 1e-3, and how far every output then moves.  This module checks that the port reproduces the fixtures
(it is the oracle tests/test_gpu_params.py compares the full-size scene with) and that every twin moves some output at least
100x beyond the bar the GPU test asserts, so the GPU test would catch each of those mistakes."""
import numpy as np
import pytest

from conftest import check_scene_matches_fixture, gold, rel, scene_by_name
from oracle.pyoracle import Engine, Prims
from test_oracle_golden import port_coupled_teacher_forced, port_teacher_forced
from test_oracle_optplane import port_persistent_plane_stage

PARAMS_A = dict(res=8, lam=20.0, margin=0.14, offset=0.06, mu=0.25, vel_limit=1.2, acc_limit=2.5, kt=2.5, piece_time0=20.0, stop=1e-2)
PARAMS_B = dict(res=8, lam=4.0, margin=0.06, offset=0.115, mu=0.05, vel_limit=0.9, acc_limit=0.8, kt=0.4, piece_time0=20.0, stop=1e-2)
PARAM_SETS = {"A": PARAMS_A, "B": PARAMS_B}
PARAM_FIELDS = ("lam", "margin", "offset", "mu", "vel_limit", "acc_limit", "ks", "kt", "piece_time0", "res")
STAGE_FIXTURES = [(name, tag) for tag in ("A", "B") for name in ("hard", "hard_single", "hard_coupled")]
TWINS = ["swap_margin_offset", "swap_vel_acc", "lam_mu_inverse", "kt_one"] + \
        [f"scale_{k}" for k in ("lam", "margin", "offset", "mu", "vel_limit", "acc_limit", "kt")]

# The bars tests/test_gpu_params.py asserts, per scene and output, normalised as the twin check records them: 0 = bit-exact.  They
# are those of the same mode at the shipped values (test_gpu_parity.py::_teacher_forced with the `hard` / single-UAV direction bar,
# test_gpu_coupled.py::test_coupled_stages_teacher_forced_vs_reference).
GPU_TOL_DIR = {"hard": 1e-9, "hard_single": 1e-11}
GPU_BARS = {
    "hard": dict(planes=0.0, gn=1e-13, direction=1e-9, steps=0.0, armijo=1e-10, mid=1e-9, post=1e-12),
    "hard_single": dict(planes=0.0, gn=1e-13, direction=1e-11, steps=0.0, mid=1e-11, post=1e-12),
    "hard_coupled": dict(planes=1e-13, gn=1e-11, mid=1e-9, post=1e-12),
}


def param_array(scene, params):
    p = dict(params); p["ks"] = scene["ks"]
    return np.array([float(p[k]) for k in PARAM_FIELDS])


def stage_fixture(scenes, name, tag):
    g = gold(f"stages_{name}_params{tag}.npz")
    scene = scene_by_name(scenes, name)
    check_scene_matches_fixture(scene, g)
    return scene, g


def velacc_distances(scene, g, params):
    """d = limit - |derivative| of every velocity / acceleration record (Energy_admm::bound_energy) at the kept iterations' pre states"""
    e = Engine("port", scene, params)
    _, _, basis = e.tables()
    res = params["res"]
    out = {}
    for it in g["kept"]:
        sp, pt = g[f"it{it}_pre_spline"], g[f"it{it}_pre_piece_time"]
        v, a = [], []
        for u in range(scene["U"]):
            for tr in range(e.S):
                w = ((tr % res) + 1) / res - (tr % res) / res
                P = basis[tr] @ sp[u][:, (tr // res) * 3:(tr // res) * 3 + 6].T
                v += [params["vel_limit"] - np.linalg.norm(5 * (P[j + 1] - P[j])) / (w * pt[u]) for j in range(5)]
                a += [params["acc_limit"] - np.linalg.norm(20 * (P[j + 2] - 2 * P[j + 1] + P[j])) / (w * w * pt[u] * pt[u]) for j in range(4)]
        out[int(it)] = (np.array(v), np.array(a))
    return out


def test_sets_break_every_coincidence_of_the_shipped_values():
    for tag, p in PARAM_SETS.items():
        assert p["margin"] != p["offset"] and p["vel_limit"] != p["acc_limit"] and p["kt"] != 1.0
        assert not 0.5 < p["lam"] * p["mu"] < 2.0, tag
    assert PARAMS_A["margin"] > PARAMS_A["offset"] and PARAMS_B["offset"] > PARAMS_B["margin"]
    assert (PARAMS_A["vel_limit"] < PARAMS_A["acc_limit"]) != (PARAMS_B["vel_limit"] < PARAMS_B["acc_limit"])
    assert max(PARAMS_A["offset"], PARAMS_B["offset"]) < 0.13          # below the `hard` scenes' clearance (dz = clear = 0.13)


def test_fixtures_record_the_modules_sets(scenes):
    for name, tag in STAGE_FIXTURES:
        scene, g = stage_fixture(scenes, name, tag)
        assert np.array_equal(g["params"], param_array(scene, PARAM_SETS[tag])), (name, tag)
    for name in ("tiny_multi", "tiny_single"):
        g = gold(f"optplane_stages_{name}_paramsA.npz")
        assert np.array_equal(g["params"], param_array(scene_by_name(scenes, name), PARAMS_A))
    g = gold("e2e_scn_b_paramsA.npz")
    assert np.array_equal(g["params"], param_array(scenes.scn_b(), PARAMS_A))
    g = gold("prims_params_kat.npz")
    for tag, p in PARAM_SETS.items():
        assert np.array_equal(g[f"{tag}_params"], param_array(scenes.hard(), p))


@pytest.mark.parametrize("name,tag", STAGE_FIXTURES)
def test_velocity_and_acceleration_barriers_are_active(scenes, name, tag):
    """the limits bind on few segments: make sure each fixture has velocity AND acceleration records inside the barrier range in
    some kept iteration, and none outside the feasible set at iteration 0"""
    scene, g = stage_fixture(scenes, name, tag)
    p = PARAM_SETS[tag]
    dist = velacc_distances(scene, g, p)
    v0, a0 = dist[0]
    assert v0.min() > 0 and a0.min() > 0
    assert any((v < p["margin"]).any() for v, _ in dist.values()), "no velocity record in the barrier range"
    assert any((a < p["margin"]).any() for _, a in dist.values()), "no acceleration record in the barrier range"


@pytest.mark.parametrize("name,tag", STAGE_FIXTURES)
def test_port_reproduces_the_reference_at_sets_a_and_b(scenes, name, tag):
    scene, g = stage_fixture(scenes, name, tag)
    if scene["mode"] == 2:
        port_coupled_teacher_forced(scene, g, PARAM_SETS[tag])
    else:
        port_teacher_forced(scene, g, PARAM_SETS[tag])


@pytest.mark.parametrize("name,tag", STAGE_FIXTURES)
def test_every_twin_moves_an_output_far_beyond_the_gpu_bar(scenes, name, tag):
    """a swapped, inverted, dropped or 0.1 % wrong parameter moves at least one output by >= 100x the GPU test's bar for it (any
    difference on a bit-exact output)"""
    _, g = stage_fixture(scenes, name, tag)
    assert list(g["twin_names"]) == TWINS
    bars = GPU_BARS[name]
    outs = list(g["twin_outputs"])
    for twin, row in zip(g["twin_names"], g["twin_diff"]):
        ratio = [(np.inf if d > 0 else 0.0) if bars[o] == 0 else d / bars[o] for o, d in zip(outs, row) if o in bars]
        assert max(ratio) >= 100, (twin, dict(zip(outs, row)))


@pytest.mark.parametrize("name", ["tiny_multi", "tiny_single"])
def test_port_persistent_planes_at_set_a(scenes, name):
    g = gold(f"optplane_stages_{name}_paramsA.npz"); scene = scene_by_name(scenes, name)
    check_scene_matches_fixture(scene, g)
    port_persistent_plane_stage(scene, g, PARAMS_A)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_port_primitives_at_sets_a_and_b(scenes, tag):
    """pair planes with the offset Newton, the optimal_plane refinements and the planner's motion validator at d = offset + margin/2"""
    g = gold("prims_params_kat.npz"); p = PARAM_SETS[tag]
    pr = Prims("port", p)
    dist = p["offset"] + 2 * p["margin"]
    newton = 0
    for P, Q, want in zip(g[f"{tag}_P"], g[f"{tag}_Q"], g[f"{tag}_plane_self"]):
        ok, cd = pr.plane_self(P, Q, dist, refine=True)
        assert ok == bool(want[0])
        if ok:
            assert np.array_equal(cd[:3], want[1:4])
            assert (np.isnan(want[4]) and np.isnan(cd[3])) or abs(cd[3] - want[4]) <= 1e-14
            newton += int(np.isfinite(want[4]))
    assert newton >= 100
    for P, q, cin, cout in zip(g[f"{tag}_P_obs"], g[f"{tag}_q_obs"], g[f"{tag}_in_obs"], g[f"{tag}_out_obs"]):
        assert np.array_equal(pr.optimal_cd(P, q, cin), cout)
    for P, Q, cin, cout in zip(g[f"{tag}_P_self"], g[f"{tag}_Q_self"], g[f"{tag}_in_self"], g[f"{tag}_out_self"]):
        assert np.array_equal(pr.self_optimal_cd(P, Q, cin), cout)
    scene = scenes.hard()
    check_scene_matches_fixture(scene, g)
    e = Engine("port", scene, p)
    hit = g[f"{tag}_hit_cloud"]
    assert 0.1 < hit.mean() < 0.9
    assert np.array_equal(e.edge_collision(g[f"{tag}_edges"]), hit)
    assert np.array_equal(e.edge_collision(g[f"{tag}_edges"], g[f"{tag}_prior"]), g[f"{tag}_hit_all"])


def test_port_end_to_end_at_set_a(scenes):
    g = gold("e2e_scn_b_paramsA.npz")
    scene = scenes.scn_b()
    check_scene_matches_fixture(scene, g)
    e = Engine("port", scene, PARAMS_A)
    gn = []
    for it in range(200):
        gn.append(e.iterate())
        if it > 1 and gn[-1] < PARAMS_A["stop"]:
            break
    assert len(gn) == int(g["iters"])
    st = e.get_state()
    assert rel(st["spline"], g["final_spline"]) <= 1e-8
    assert rel(st["piece_time"], g["final_piece_time"]) <= 1e-8
    e.stage_planes()
    en = np.array([e.spline_energy(u) for u in range(scene["U"])])
    assert np.max(np.abs(en - g["final_energy"]) / np.abs(g["final_energy"])) <= max(1e-8, 3 * float(g["energy_env"]))
