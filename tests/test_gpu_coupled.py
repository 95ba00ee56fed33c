"""GPU (-m gpu): coupled mode ("decouple":0, TJ_MODE_MULTI_COUPLED) through the C ABI, against golden vectors of the
unmodified reference (Optimization3D_multi::optimization, Optimization3D_multi.h:120-174 / update_spline :508-639 /
Step::couple_self_step Step.h:112-182) and against the CPU oracle.  Tolerances as in test_gpu_parity.py: planes 1e-13,
teacher-forced stages 1e-9 abs on control points, slack/dual 1e-12 rel, end-to-end 1e-8 rel (BASELINE.json)."""
import numpy as np
import pytest

from conftest import canon, check_scene_matches_fixture, gold, maxdiff, rel, scene_by_name
from query_kit import STATE

pytestmark = pytest.mark.gpu


def test_coupled_stages_teacher_forced_vs_reference(pkg, scenes):
    g = gold("stages_hard_coupled.npz")
    scene = scene_by_name(scenes, "hard_coupled")
    check_scene_matches_fixture(scene, g)
    _coupled_teacher_forced(pkg, scene, g)


def _coupled_teacher_forced(pkg, scene, g, params=None):
    s = pkg.Solver(scene, params=params, stop=0.0)
    for it in g["kept"]:
        k = f"it{it}_"
        s.set_state({n: g[k + "pre_" + n] for n in STATE})
        counts, planes = s.stage_planes()
        assert np.array_equal(counts, g[k + "counts"]), f"it{it}: plane counts differ"
        assert maxdiff(canon(counts, planes), g[k + "planes"]) <= 1e-13
        gnorm, wolfe = s.stage_update_spline()
        assert abs(gnorm - g[k + "gnorm"]) <= 1e-11 * max(1.0, float(g[k + "gnorm"]))
        assert abs(wolfe - g[k + "wolfe"]) <= 1e-9 * max(1.0, abs(float(g[k + "wolfe"])))
        st = s.get_state()
        assert maxdiff(st["spline"], g[k + "mid_spline"]) <= 1e-9
        assert maxdiff(st["piece_time"], g[k + "mid_piece_time"]) <= 1e-9      # same CCD exponent, same Armijo halvings
        s.set_state({n: (g[k + "mid_" + n] if n in ("spline", "piece_time") else g[k + "pre_" + n]) for n in STATE})
        s.stage_slack()
        st = s.get_state()
        for n in STATE:
            assert maxdiff(st[n], g[k + "post_" + n]) <= 1e-12 * max(1.0, np.abs(g[k + "post_" + n]).max()), (it, n)
    assert s.stats()["error_bits"] == 0
    s.close()


@pytest.mark.parametrize("name", ["hard_coupled", "scn_b_coupled"])
def test_coupled_iterations_vs_oracle_live(pkg, scenes, name):
    """every iteration of a longer run, each started from the oracle's state, through the iteration chain"""
    from oracle.pyoracle import Engine
    scene = scene_by_name(scenes, name)
    o = Engine("port", scene)
    s = pkg.Solver(scene, stop=0.0)
    for it in range(14):
        s.set_state(o.get_state())
        go = o.iterate()
        gg, _, _ = s.iterate(1)
        a, b = s.get_state(), o.get_state()
        assert abs(gg - go) <= 1e-10 * max(1.0, go), (it, gg, go)
        for n in STATE:
            tol = 1e-9 if n in ("spline", "piece_time") else 1e-9 * max(1.0, np.abs(b[n]).max())
            assert maxdiff(a[n], b[n]) <= tol, (it, n, maxdiff(a[n], b[n]))
        assert np.all(a["piece_time"] == a["piece_time"][0])
    assert s.stats()["error_bits"] == 0
    s.close()


def test_coupled_end_to_end_vs_reference(pkg, scenes):
    """free-running with the device-side stop test: same iteration count as the reference, final control points and
    shared piece_time within fp64 rel-tol 1e-8"""
    g = gold("e2e_scn_b_coupled.npz")
    scene = scene_by_name(scenes, "scn_b_coupled")
    check_scene_matches_fixture(scene, g)
    s = pkg.Solver(scene)
    gnorm, iters, conv = s.iterate(200)
    assert conv and iters == int(g["iters"])
    st = s.get_state()
    assert rel(st["spline"], g["final_spline"]) <= 1e-8
    assert rel(st["piece_time"], g["final_piece_time"]) <= 1e-8
    assert abs(gnorm - g["gnorm_hist"][-1]) <= 1e-3 * g["gnorm_hist"][-1]
    assert s.stats()["error_bits"] == 0
    s.close()


def test_coupled_mode_sharded_equals_unsharded(pkg, scenes):
    """"decouple":0 with the robots split over two contexts (ranks 0/2 and 1/2 on the same GPU; the five per-iteration exchanges
    done by plain device copies -- the schedule bench.py --coupled runs over RCCL): the arrowhead system is solved by per-rank
    elimination + the gathered Schur-corner terms, the shared CCD step and the Armijo test on the summed energy use gathered
    exponents / energies.  State must be BITWISE equal to the single-context run."""
    import ctypes as C
    import importlib
    sharding = importlib.import_module("traj-opt-admm_amd.sharding")
    scene = dict(scenes.hard(4, 4000)); scene["mode"] = 2
    ref = pkg.Solver(scene, stop=0.0)
    r0 = pkg.Solver(scene, stop=0.0, rank=0, world=2)
    r1 = pkg.Solver(scene, stop=0.0, rank=1, world=2)
    assert r0.phase_count() == 6
    from conftest import hip_runtime
    hip = hip_runtime()   # the runtime instance libtrajadmm.so is linked against
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def exchange(what):
        p0, per, f0, n0 = r0.exchange_buffer(what)
        p1, _, f1, n1 = r1.exchange_buffer(what)
        r0.sync(); r1.sync()
        assert hip.hipMemcpy(p0 + f1 * per * 8, p1 + f1 * per * 8, n1 * per * 8, 3) == 0
        assert hip.hipMemcpy(p1 + f0 * per * 8, p0 + f0 * per * 8, n0 * per * 8, 3) == 0

    for it in range(8):
        ref.iterate(1)
        for phase, what in sharding.COUPLED_SCHEDULE:
            r0.iterate_phase(phase); r1.iterate_phase(phase)
            if what is not None:
                exchange(what)
        r0.sync(); r1.sync()
        a = ref.get_state(); b0 = r0.get_state(); b1 = r1.get_state()
        h = scene["U"] // 2
        for n in STATE:
            assert np.array_equal(a[n][:h], b0[n][:h]), (it, n)
            assert np.array_equal(a[n][h:], b1[n][h:]), (it, n)
    assert np.all(b0["piece_time"][:h] == b1["piece_time"][h:][0])      # one piece_time for the whole fleet
    assert ref.stats()["error_bits"] == 0 and r0.stats()["error_bits"] == 0 and r1.stats()["error_bits"] == 0
    for x in (ref, r0, r1):
        x.close()


def test_coupled_armijo_search_follows_the_reference_beyond_31_steps(pkg, scenes):
    """The coupled Armijo search on the summed energy (Optimization3D_multi.h:605-636) has no bound in the reference; the HIP path's evaluation launches cover
    the steps 0.8^0 .. 0.8^30 and round 4 reported TJ_ERR_NO_PROGRESS beyond.  Now the deciding block goes on alone (kernels_ls.h: lsc_continue) to the
    reference's own end.  Fixture from the unmodified reference (tests/golden/make_golden.py: make_coupled_long): three teacher-forced states whose search
    takes 42, 63 and 51 back-offs -- the state after update_spline (a different exponent would move piece_time by 20 %), gnorm, wolfe, and the state after
    the slack update; the evaluation count says the continuation really ran.  Tolerances as in test_coupled_stages_teacher_forced_vs_reference."""
    g = gold("coupled_long_kat.npz")
    for ci, (U, amp, seed, dz) in enumerate(g["cases"]):
        scene = dict(scenes.crossing(int(U), 2000, seed=int(seed), dz=float(dz)), mode=2)
        scene["cloud"] = scene["cloud"] + np.array([0.0, 0.0, 1e9])
        k = f"c{ci}_"
        assert np.allclose([scene["cloud"].sum(), np.abs(scene["cloud"]).sum()], g[k + "cloud_sum"], rtol=1e-13)
        s = pkg.Solver(scene, stop=0.0)
        s.set_state({n: g[k + "pre_" + n] for n in STATE})
        s.stage_planes()
        e0 = s.stats()["energy_evals"]
        gnorm, wolfe = s.stage_update_spline()
        assert abs(gnorm - g[k + "gnorm"]) <= 1e-11 * max(1.0, float(g[k + "gnorm"]))
        assert abs(wolfe - g[k + "wolfe"]) <= 1e-9 * max(1.0, abs(float(g[k + "wolfe"])))
        st = s.get_state()
        evals = (s.stats()["energy_evals"] - e0) // int(U)            # 2 + accepted exponent, per robot
        assert evals - 2 > 31, (ci, evals)
        scale = max(1.0, np.abs(g[k + "mid_spline"]).max())
        assert maxdiff(st["spline"], g[k + "mid_spline"]) <= 1e-9 * scale, (ci, maxdiff(st["spline"], g[k + "mid_spline"]))
        assert maxdiff(st["piece_time"], g[k + "mid_piece_time"]) <= 1e-9, (ci, st["piece_time"][0], g[k + "mid_piece_time"][0], evals)
        assert s.stats()["error_bits"] == 0, ci
        # ... and the whole iteration through the chain (one-launch search, its last block continuing, committing and beginning the next iteration)
        s.close()
        s = pkg.Solver(scene, stop=0.0)   # (a fresh context: the stage calls above left a slack update owed)
        s.set_state({n: g[k + "pre_" + n] for n in STATE})
        s.iterate(1)
        st = s.get_state()
        # Bars at ~10x what the chain shows against the reference (round 6; round 5 asserted 1e-6 of each array's LARGEST entry -- 30 absolute on these robots, 1e7 apart):
        # control points 9e-16 absolute, the shared piece_time bit for bit; the slack / dual blocks element by element 1.3e-7 relative (floor 1) on the first case --
        # the displaced z (amp 1e3 ... 1e5) makes the slack update's Newton step amplify the control points' last bit -- and <= 6e-11 on the other two.
        assert maxdiff(st["spline"], g[k + "post_spline"]) <= 1e-14, (ci, maxdiff(st["spline"], g[k + "post_spline"]))
        assert maxdiff(st["piece_time"], g[k + "post_piece_time"]) <= 1e-14, (ci, maxdiff(st["piece_time"], g[k + "post_piece_time"]))
        for n in ("p_slack", "p_lambda", "t_slack", "t_lambda"):
            erel = float((np.abs(st[n] - g[k + "post_" + n]) / np.maximum(np.abs(g[k + "post_" + n]), 1.0)).max())
            assert erel <= (2e-6 if ci == 0 else 1e-9), (ci, n, erel)
        assert s.stats()["error_bits"] == 0, ci
        s.close()


def test_sharded_coupled_armijo_search_follows_the_reference_beyond_31_steps(pkg, scenes):
    """Round 6: the coupled Armijo search of SHARDED contexts to the reference's own end.  One exchange carries the candidates 0.8^0 .. 0.8^30; round 5 reported
    TJ_ERR_NO_PROGRESS (error bit 32) beyond.  Now (a) two contexts driven by the caller with tj_set_coupled_follow: phase 5 commits nothing while no gathered candidate
    passes, the caller asks tj_coupled_search_pending and repeats phase 4 / exchange 4 / phase 5 for the next 32 candidates; (b) tj_group by itself: the batch that ran
    into bit 32 is run again from its first state with the followed search.  On the reference's own long searches (coupled_long_kat.npz: 42, 63 and 51 back-offs) both end
    bit for bit in the state of ONE context -- whose result is pinned to the reference by the test above -- with no error bit; without `follow` the old report stands."""
    import ctypes as C
    import importlib
    sharding = importlib.import_module("traj-opt-admm_amd.sharding")
    from conftest import hip_runtime
    hip = hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    g = gold("coupled_long_kat.npz")
    for ci, (U, amp, seed, dz) in enumerate(g["cases"]):
        scene = dict(scenes.crossing(int(U), 2000, seed=int(seed), dz=float(dz)), mode=2)
        scene["cloud"] = scene["cloud"] + np.array([0.0, 0.0, 1e9])
        k = f"c{ci}_"
        pre = {n: g[k + "pre_" + n] for n in STATE}
        one = pkg.Solver(scene, stop=0.0)
        one.set_state(pre)
        one.iterate(1)
        so, evals_one = one.get_state(), one.stats()["energy_evals"] // int(U)
        assert evals_one - 2 > 31 and one.stats()["error_bits"] == 0
        one.close()
        h = int(U) // 2
        # (a) two contexts, the schedule driven from here
        for follow in (True, False):
            r0 = pkg.Solver(scene, stop=0.0, rank=0, world=2); r1 = pkg.Solver(scene, stop=0.0, rank=1, world=2)
            r0.set_state(pre); r1.set_state(pre)
            if follow:
                r0.set_coupled_follow(True); r1.set_coupled_follow(True)

            def exchange(what):
                p0, per, f0, n0 = r0.exchange_buffer(what)
                p1, _, f1, n1 = r1.exchange_buffer(what)
                r0.sync(); r1.sync()
                assert hip.hipMemcpy(p0 + f1 * per * 8, p1 + f1 * per * 8, n1 * per * 8, 3) == 0
                assert hip.hipMemcpy(p1 + f0 * per * 8, p0 + f0 * per * 8, n0 * per * 8, 3) == 0

            for phase, what in sharding.COUPLED_SCHEDULE:
                r0.iterate_phase(phase); r1.iterate_phase(phase)
                if what is not None:
                    exchange(what)
            extra = 0
            if follow:
                while True:
                    pa, pb = r0.coupled_search_pending(), r1.coupled_search_pending()
                    assert pa == pb
                    if not pa:
                        break
                    r0.iterate_phase(4); r1.iterate_phase(4); exchange(4); r0.iterate_phase(5); r1.iterate_phase(5)
                    extra += 1
                assert extra == (evals_one - 2) // 32, (ci, extra, evals_one)   # candidates 0 .. 30 in the first table, 32 more per further one
            r0.sync(); r1.sync()
            e0, e1 = r0.stats()["error_bits"], r1.stats()["error_bits"]
            if follow:
                assert e0 == 0 and e1 == 0, (ci, e0, e1)
                b0, b1 = r0.get_state(), r1.get_state()
                for n in STATE:
                    assert np.array_equal(so[n][:h], b0[n][:h]) and np.array_equal(so[n][h:], b1[n][h:]), (ci, n)
            else:
                assert (e0 & 32) and (e1 & 32), (ci, e0, e1)   # the round-5 report, for callers that do not follow
            r0.close(); r1.close()
        # (b) tj_group (two ranks on this device): the library follows by itself
        grp = pkg.Group(scene, [0, 0], stop=0.0)
        grp.lib.tj_group_ctx.restype = C.c_void_p
        for r in range(2):
            ctx = C.c_void_p(grp.lib.tj_group_ctx(grp._g, r))
            for u in range(int(U)):
                a = [np.ascontiguousarray(pre[n][u], dtype=np.float64) for n in ("spline", "p_slack", "p_lambda", "t_slack", "t_lambda")]
                assert grp.lib.tj_set_state(ctx, u, *[x.ctypes.data_as(C.POINTER(C.c_double)) for x in a], C.c_double(float(pre["piece_time"][u]))) == 0
        grp.iterate(1)
        sg = grp.get_state()
        for n in STATE:
            assert np.array_equal(so[n], sg[n]), (ci, n)
        grp.close()


def test_coupled_chain_with_cache_units_changes_no_bit(pkg, scenes, monkeypatch):
    """coupled mode, one context: every robot's hull cache / swept-hull cache is built by units at the head of k_front / k_ccd (round 5: the k_hullinfo and
    k_ccd_prep launches drop out of the chain: 10 -> 8 kernels per iteration); TJ_COUPLED_UNITS=0 launches the two kernels as before.  Same bits."""
    scene = dict(scenes.crossing(12, 4000, seed=23, name="crossing-U12-coupled"), mode=2)
    monkeypatch.delenv("TJ_COUPLED_UNITS", raising=False)
    # the default since the second half of round 5: the Newton solve on a second queue next to k_grad (one gate launch more per iteration) -- same bits as the one-queue chain
    monkeypatch.setenv("TJ_XS_ASYNC", "1")   # explicit: the default takes the second queue only where the process's hardware-queue budget allows (GPU_MAX_HW_QUEUES)
    e = pkg.Solver(scene, stop=0.0)
    l0 = e.launch_count(); e.iterate(12); le = e.launch_count() - l0
    se, te = e.get_state(), e.stats()
    e.close()
    monkeypatch.setenv("TJ_XS_ASYNC", "0")   # (the launch counts below are those of the one-queue chain)
    a = pkg.Solver(scene, stop=0.0)
    l0 = a.launch_count(); a.iterate(12); la = a.launch_count() - l0
    for n in se:
        assert np.array_equal(se[n], a.get_state()[n]), f"{n} differs between the asynchronous solve and the one-queue coupled chain"
    assert te["error_bits"] == 0 and le == la + 12 + 11, (le, la)   # one gate per iteration for the solve + one per pairing k_ls_coupled(i) / k_front(i + 1) for the asynchronous front (round 6)
    monkeypatch.setenv("TJ_COUPLED_UNITS", "0")
    b = pkg.Solver(scene, stop=0.0)
    l0 = b.launch_count(); b.iterate(12); lb = b.launch_count() - l0
    sa, sb = a.get_state(), b.get_state()
    for n in sa:
        assert np.array_equal(sa[n], sb[n]), n
    assert a.stats()["error_bits"] == 0 and b.stats()["error_bits"] == 0
    assert lb - la == 2 * 12 and la <= 6 * 12 + 4, (la, lb)    # k_front, k_mid, k_grad, k_xsolve (finishes the arrowhead solve itself), k_ccd (replays the pairs itself), k_ls_coupled
    # ... and with the corner solve / the pair replay as launches of their own (TJ_C2_FOLD=0, TJ_SEQ_FOLD=0): same bits
    monkeypatch.setenv("TJ_C2_FOLD", "0"); monkeypatch.setenv("TJ_SEQ_FOLD", "0")
    c = pkg.Solver(scene, stop=0.0)
    l0 = c.launch_count(); c.iterate(12); lc = c.launch_count() - l0
    sc = c.get_state()
    for n in sa:
        assert np.array_equal(sa[n], sc[n]), n
    assert lc - lb == 2 * 12
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["decoupled", "coupled"])
def test_hull_record_writers_agree_bitwise(pkg, scenes, monkeypatch, mode):
    """The hull cache of the robot-pair stage (per (robot, segment): hull, box, 49 k-DOP intervals; and the box table) has several writers that must leave the
    same bits (dev_common.h: hull_record_store and its pieces).  Which one wrote the record a batch leaves behind depends on the schedule:
      decoupled   the LAST line search of a batch (ls_publish_hullinfo) -- with the asynchronous front and without it (TJ_FRONT_ASYNC=0); the records that
                  k_front's units leave in the earlier iterations of a batch are overwritten by it and are pinned through the state hashes only;
      coupled     the line search publishes nothing, so after one more iteration the record of the state after 3 iterations is the one the 4th iteration's
                  front left: the publishing obstacle units (obs_query_body) in their asynchronous and plain forms, or, with TJ_COUPLED_UNITS=0, k_hullinfo
                  launched inside the chain.
    Each is compared with what k_hullinfo writes for the same state through the stage API (set_state, then the stage planes_self, whose first launch it is)."""
    scene = dict(scenes.crossing(12, 4000, seed=23, name="crossing-U12-hullrec"), mode=mode)
    for k in ("TJ_FRONT_ASYNC", "TJ_COUPLED_UNITS"):
        monkeypatch.delenv(k, raising=False)

    def chain(env, plan_want):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = pkg.Solver(scene, stop=0.0, kat=True)
        for k in env:
            monkeypatch.delenv(k)
        plan = pkg.plan_record(ctx=s._ctx)[1]
        for k, v in plan_want.items():
            assert plan[k] == v, (env, k, plan[k])
        s.iterate(3)
        st = s.get_state()
        if mode == 2:
            s.iterate(1)
        rec = s.kat_hull_record()
        assert s.stats()["error_bits"] == 0
        return s, st, rec

    runs = [chain({}, {"xf_all": 1} if mode == 2 else {"fuse": 1}), chain({"TJ_FRONT_ASYNC": "0"}, {"fa": 0})]
    if mode == 2:
        runs.append(chain({"TJ_COUPLED_UNITS": "0"}, {"xf_all": 0}))
    s0, st0, _ = runs[0]
    for _, st, _ in runs[1:]:
        for n in STATE:
            assert np.array_equal(st0[n], st[n]), n
    s0.set_state(st0)
    s0.run_stage("begin")
    s0.run_stage("planes_self")
    info_k, hbox_k = s0.kat_hull_record()
    assert np.all(np.isfinite(info_k)) and np.any(info_k[:, :, :18] != 0.0)
    for i, (_, _, (info, hbox)) in enumerate(runs):
        assert np.array_equal(info, info_k), (i, int(np.sum(info != info_k)))
        assert np.array_equal(hbox, hbox_k), (i, int(np.sum(hbox != hbox_k)))
    for s, _, _ in runs:
        s.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["decoupled", "coupled"])
def test_swept_record_writers_agree_bitwise(pkg, scenes, monkeypatch, mode):
    """The swept-hull cache of the two CCD stages (per (robot, segment): hull P, direction hull D, obstacle box, pair box, 49 k-DOP intervals; and the pair-box
    table) has several writers that must leave the same bits (dev_common.h: swept_record_put and its pieces).  The line search does not touch the cache, so after
    one more iteration it still holds what that iteration's writer made of the state before it and of the direction tj_get_direction then reports:
      decoupled   the obstacle units of k_ccd behind the asynchronous solve (ccd_record_async), or, with TJ_XS_ASYNC=0, k_xsolve's tail;
      coupled     the publishing obstacle units of k_ccd (ccd_prep_segment, written through), or, with TJ_COUPLED_UNITS=0, k_ccd_prep launched inside the chain.
    Each is compared with what k_ccd_prep writes through the stage API for that state and that direction (set_state, set_direction, then the stage ccd_prep)."""
    scene = dict(scenes.crossing(12, 4000, seed=23, name="crossing-U12-sweptrec"), mode=mode)
    for k in ("TJ_XS_ASYNC", "TJ_KEEP_ASYNC", "TJ_COUPLED_UNITS"):
        monkeypatch.delenv(k, raising=False)

    def chain(env, plan_want):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = pkg.Solver(scene, stop=0.0, kat=True)
        for k in env:
            monkeypatch.delenv(k)
        plan = pkg.plan_record(ctx=s._ctx)[1]
        for k, v in plan_want.items():
            assert plan[k] == v, (env, k, plan[k])
        s.iterate(3)
        st = s.get_state()
        s.iterate(1)
        rec = s.kat_swept_record()
        dirs = [s.get_direction(u) for u in range(s.U)]
        assert s.stats()["error_bits"] == 0
        return s, st, rec, dirs

    if mode == 1:
        runs = [chain({}, {"xs_async": 1, "fuse": 1}), chain({"TJ_XS_ASYNC": "0"}, {"xs_async": 0, "fuse": 1})]
    else:
        runs = [chain({}, {"xf_all": 1}), chain({"TJ_COUPLED_UNITS": "0"}, {"xf_all": 0})]
    s0, st0, _, dirs0 = runs[0]
    for _, st, _, dirs in runs[1:]:
        for n in STATE:
            assert np.array_equal(st0[n], st[n]), n
        for u in range(s0.U):
            assert np.array_equal(dirs0[u][0], dirs[u][0]), u
    s0.set_state(st0)
    for u, (d, t, w, g) in enumerate(dirs0):
        s0.set_direction(u, d, t, w, g)
    s0.run_stage("begin")
    s0.run_stage("ccd_prep")
    info_k, cbox_k = s0.kat_swept_record()
    assert np.all(np.isfinite(info_k)) and np.all(np.isfinite(cbox_k)) and np.any(info_k[:, :, pkg.Solver.SWEPT_FIELDS["D"]] != 0.0)
    for i, (_, _, (info, cbox), _) in enumerate(runs):
        assert np.array_equal(info, info_k), (i, int(np.sum(info != info_k)))
        assert np.array_equal(cbox, cbox_k), (i, int(np.sum(cbox != cbox_k)))
    for s, _, _, _ in runs:
        s.close()
