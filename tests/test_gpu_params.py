"""GPU (-m gpu): the HIP path at the non-default parameter sets A and B of tests/test_oracle_params.py, against fixtures of the
unmodified reference taken under those sets (tests/golden/*_params[AB].npz).  At the shipped 3D.json values margin == offset,
vel_limit == acc_limit, kt == 1 and lambda == 1/mu, so a swapped, dropped or inverted parameter is invisible there; the twin
check recorded in every stage fixture shows that each such mistake moves an output >= 100x beyond the bars asserted here
(tests/test_oracle_params.py::test_every_twin_moves_an_output_far_beyond_the_gpu_bar).  Bars are those of the same mode at the
shipped values."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import TOL_GNORM_FULL, TOL_STATE_FULL, check_scene_matches_fixture, gold, observe_iteration, rel, scene_by_name
from query_kit import STATE
from test_gpu_coupled import _coupled_teacher_forced
from test_gpu_optplane import _persistent_plane_stage, assert_bits
from test_gpu_parity import _teacher_forced
from test_oracle_params import GPU_TOL_DIR, PARAM_SETS, PARAMS_A, PARAMS_B, STAGE_FIXTURES
from test_planner import _wall_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,tag", STAGE_FIXTURES)
def test_stages_teacher_forced_at_sets_a_and_b(pkg, scenes, name, tag):
    g = gold(f"stages_{name}_params{tag}.npz")
    scene = scene_by_name(scenes, name)
    check_scene_matches_fixture(scene, g)
    if scene["mode"] == 2:
        _coupled_teacher_forced(pkg, scene, g, params=PARAM_SETS[tag])
    else:
        _teacher_forced(pkg, scene, g, tol_dir=GPU_TOL_DIR[name], params=PARAM_SETS[tag])


@pytest.mark.parametrize("name", ["tiny_multi", "tiny_single"])
def test_persistent_plane_stage_at_set_a(pkg, scenes, name):
    g = gold(f"optplane_stages_{name}_paramsA.npz")
    scene = scene_by_name(scenes, name)
    check_scene_matches_fixture(scene, g)
    _persistent_plane_stage(pkg, scene, g, f"{name}_paramsA", params=PARAMS_A)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_known_answers_at_sets_a_and_b(pkg, scenes, tag):
    """pair planes with the offset Newton (per lane and wave-cooperative), the optimal_plane refinements and the motion validator
    on a context created with the set"""
    g = gold("prims_params_kat.npz"); p = PARAM_SETS[tag]
    s = pkg.Solver(scenes.tiny(1), params=p, stop=0.0, kat=True)
    P, Q, want = g[f"{tag}_P"], g[f"{tag}_Q"], g[f"{tag}_plane_self"]
    dist = p["offset"] + 2 * p["margin"]
    for what in (1, 4):
        out = s.kat_planes(what, P, Q, dist)
        assert np.array_equal(out[:, 0], want[:, 0]), what
        ok = out[:, 0] == 1
        assert np.array_equal(out[ok, 1:4], want[ok, 1:4]), what
        assert_bits(out[ok, 4], want[ok, 4], f"kat_planes {what} offsets", f"prims_params_kat {tag}")
    fin, out = s.kat_refine_planes(5, g[f"{tag}_P_obs"], g[f"{tag}_q_obs"], g[f"{tag}_in_obs"])
    assert fin.all()
    assert_bits(out, g[f"{tag}_out_obs"], "optimal_cd", f"prims_params_kat {tag}")
    for what in (6, 7):
        fin, out = s.kat_refine_planes(what, g[f"{tag}_P_self"], g[f"{tag}_Q_self"], g[f"{tag}_in_self"])
        assert fin.all()
        assert_bits(out, g[f"{tag}_out_self"], f"self_optimal_cd ({what})", f"prims_params_kat {tag}")
    assert s.stats()["error_bits"] == 0
    s.close()
    scene = scenes.hard()
    check_scene_matches_fixture(scene, g)
    s = pkg.Solver(scene, params=p, stop=0.0)
    assert np.array_equal(s.edge_collision(g[f"{tag}_edges"]), g[f"{tag}_hit_cloud"])
    assert np.array_equal(s.edge_collision(g[f"{tag}_edges"], g[f"{tag}_prior"]), g[f"{tag}_hit_all"])
    assert s.stats()["error_bits"] == 0
    s.close()


def test_end_to_end_at_set_a(pkg, scenes):
    """free-running with the device stop test under set A: same iteration count as the reference, control points within 1e-8,
    energies within the reference's own 1-ulp envelope (as test_gpu_parity.py::test_end_to_end_vs_reference)"""
    g = gold("e2e_scn_b_paramsA.npz")
    scene = scenes.scn_b()
    check_scene_matches_fixture(scene, g)
    s = pkg.Solver(scene, params=PARAMS_A)
    gnorm, iters, conv = s.iterate(200)
    assert conv and iters == int(g["iters"])
    st = s.get_state()
    assert rel(st["spline"], g["final_spline"]) <= max(1e-8, 3 * float(g["spline_env"]))
    assert rel(st["piece_time"], g["final_piece_time"]) <= 1e-8
    assert s.stats()["error_bits"] == 0
    s.close()
    s = pkg.Solver(scene, params=PARAMS_A, stop=0.0)
    s.set_state(st)
    s.stage_planes()
    en = s.energy()
    assert np.max(np.abs(en - g["final_energy"]) / np.abs(g["final_energy"])) <= max(1e-8, 3 * float(g["energy_env"]))
    assert s.stats()["error_bits"] == 0
    s.close()


def test_full_size_scn_c_at_set_b_vs_oracle(pkg, scenes):
    """SCN-C size (64 UAVs, 100k points): two whole iterations under set B, each started from the port's state (the port is pinned
    to the reference at set B by tests/test_oracle_params.py)"""
    from oracle.pyoracle import Engine
    scene = scenes.scn_c()
    o = Engine("port", scene, PARAMS_B)
    s = pkg.Solver(scene, params=PARAMS_B, stop=0.0)
    for it in range(2):
        s.set_state(o.get_state())
        go = o.iterate()
        gg, _, _ = s.iterate(1)
        observe_iteration(s.get_state(), o.get_state(), gg, go, TOL_STATE_FULL, TOL_GNORM_FULL, it)
    assert s.stats()["error_bits"] == 0
    s.close()


def test_group_passes_the_set_to_every_rank(pkg, scenes):
    """tj_group_create copies the parameters into each rank's context: two ranks on one device under set A equal one context"""
    scene = scenes.hard(4, 4000)
    ref = pkg.Solver(scene, params=PARAMS_A, stop=0.0)
    grp = pkg.Group(scene, [0, 0], params=PARAMS_A, stop=0.0)
    for batch in (1, 4):
        g0, _, _ = ref.iterate(batch)
        g, _, _ = grp.iterate(batch)
        a, b = ref.get_state(), grp.get_state()
        for n in STATE:
            assert np.array_equal(a[n], b[n]), n
        assert g == g0
    assert ref.stats()["error_bits"] == 0
    ref.close(); grp.close()


def _config_a(**over):
    """Config_File/3D.json with set A's values, all 16 keys (the mains fix kt = 1 and piece_time = 20)"""
    c = {"auto": 0, "init": 1, "gui": 0, "optimal_plane": 0, "decouple": 1, "res": PARAMS_A["res"], "vel_limit": PARAMS_A["vel_limit"],
         "acc_limit": PARAMS_A["acc_limit"], "lambda": PARAMS_A["lam"], "epsilon": 0.1, "margin": PARAMS_A["margin"],
         "offset": PARAMS_A["offset"], "stop": PARAMS_A["stop"], "exit": 0, "init_ob": 1, "mu": PARAMS_A["mu"]}
    c.update(over)
    assert len(c) == 16
    return json.dumps(c)


def test_cli_drop_in_at_set_a(pkg, scenes, tmp_path):
    scene = scenes.scn_b()
    mesh = "x.obj"
    scenes.write_reference_files(scene, str(tmp_path), mesh)
    os.makedirs(tmp_path / "Config_File", exist_ok=True)
    (tmp_path / "Config_File" / "3D.json").write_text(_config_a())
    exe = os.path.join(ROOT, "traj-opt-admm_amd", "multiPathPlanning3D")
    r = subprocess.run(["timeout", "-k", "10", "240", exe, mesh, "--dump-state", "state.txt", "--max-iter", "300"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    res = open(tmp_path / "result" / (mesh + "_result_file_multi.txt")).read().split("\n")
    iters = int(res[0].split()[1])
    lines = open(tmp_path / "state.txt").read().strip().split("\n")
    s = pkg.Solver(scene, params=dict(PARAMS_A, kt=1.0, piece_time0=20.0))
    g, it, conv = s.iterate(300)
    assert conv and abs(it - iters) <= 1 and s.stats()["error_bits"] == 0
    T = 3 * scene["P"] + 3
    cli_spline = np.array([[float(x) for x in l.split()] for l in lines if len(l.split()) == 3 and l[0] not in "u"]).reshape(scene["U"], T, 3)
    assert rel(cli_spline, s.get_state()["spline"].transpose(0, 2, 1)) <= 1e-6       # x0.2 / x5 file round trip is not bit exact
    s.close()


def test_cli_init_2_at_set_a_plans_edges_the_reference_accepts(pkg, scenes, tmp_path):
    """`"init":2` under set A: every planned edge is clear by the reference's predicate at A's clearance offset + margin/2"""
    from oracle.pyoracle import Engine
    sc, starts, goals = _wall_scene(scenes)
    mesh = "x.obj"
    scenes.write_reference_files(dict(sc, mode=1), str(tmp_path), mesh)
    os.remove(tmp_path / "init" / (mesh + "_init_file.txt"))
    with open(tmp_path / "init" / (mesh + "_start_goal.txt"), "w") as f:
        for a, b in zip(starts, goals):
            f.write(" ".join("%.17g" % v for v in list(a) + list(b)) + "\n")
    os.makedirs(tmp_path / "Config_File", exist_ok=True)
    (tmp_path / "Config_File" / "3D.json").write_text(_config_a(init=2))
    exe = os.path.join(ROOT, "traj-opt-admm_amd", "multiPathPlanning3D")
    r = subprocess.run(["timeout", "-k", "10", "240", exe, mesh, "--max-iter", "400"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout[-500:]
    rows = [l.split() for l in open(tmp_path / "init" / (mesh + "_init_file.txt")).read().strip().split("\n")]
    wp = np.array(rows, dtype=float).reshape(len(rows), len(starts), 3).transpose(1, 0, 2) * 5.0    # the reader multiplies by 5
    o = Engine("port", dict(sc, U=len(starts), waypoints=sc["waypoints"][:len(starts)]), PARAMS_A)
    d = PARAMS_A["offset"] + 0.5 * PARAMS_A["margin"]
    prior = np.zeros((0, 6))
    for u in range(len(starts)):
        edges = np.concatenate([wp[u, :-1], wp[u, 1:]], axis=1)
        edges = edges[np.linalg.norm(edges[:, :3] - edges[:, 3:], axis=1) > 0]
        assert not o.edge_collision(edges, prior, d).any(), u
        prior = np.concatenate([prior, edges], axis=0)
