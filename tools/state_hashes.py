#!/usr/bin/env python3
"""State hashes of the standard scenes after a fixed number of iterations (GPU only): run it with two builds of the library (TRAJADMM_LIB=<other .so>) to see whether a
change moved a bit anywhere.   python tools/state_hashes.py [iterations] [plan fields]      prints: scene, sha256 of the state, error bits, pair planes, pair solves per iteration,
energy evaluations, the line search's LDS layout as the context planned it (ls_layout: plane_cap / affine / groups) and the plan fields asked for (comma separated names of PLAN_FIELDS, e.g.
xs_async,fuse,c2_fold,xf_all: whether a TJ_* switch of the run took effect on that leg)

The P<n> legs (eight robots, `pieces` = n, res = 8) walk the layouts of the line search (kernels_ls.h ls_layout), each at the smallest `pieces` that has it -- found with
the planner (tj_kat_plan), not by hand: 7 = eight groups, affine trial hulls, planes in LDS (plane_cap 133); 8 = the same with plane_cap 0 (planes read from global memory);
10 = eight groups, hulls from the basis; 11 = four groups; 19 = two groups; 27 = one group; P20c = two groups in the coupled mode (a round in four passes).
fleet256 (the scene of test_passing_long_pair_solves_on_changes_no_bit) is the one leg in the one-pair-per-lane regime of the pair solve, with its passed-on consumers:
pair_solves / iterations must exceed 4096 there.
H8tri / H8tri-c: H8's cloud as obstacle triangles (BASELINE config 5's geometry), decoupled and coupled -- the PRIM == 3 paths of the walk, the cull and the solve."""
import sys, os, importlib, hashlib, ctypes as C
import numpy as np
ROOT = os.environ.get("GRAFT_REPO_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("traj-opt-admm_amd"); sc = pkg.scenes
n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
extra = [k for k in (sys.argv[2].split(",") if len(sys.argv) > 2 else []) if k]
kat = C.CDLL(pkg.KAT_LIB_PATH)   # the test build next to the library under test (same sources, same context record): only its tj_kat_plan reads the plan


def ls_layout(s):
    out = np.zeros(len(pkg.PLAN_FACTS) + len(pkg.PLAN_FIELDS), dtype=np.int32)
    got = kat.tj_kat_plan(s._ctx, None, None, out.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(out.size), None, C.c_int(0))
    assert got == out.size, got
    plan = dict(zip(pkg.PLAN_FIELDS, (int(x) for x in out[len(pkg.PLAN_FACTS):])))
    return f"plane_cap {plan['lsl_plane_cap']} affine {plan['lsl_affine']} groups {plan['lsl_groups']}" + "".join(f" {k} {plan[k]}" for k in extra)


def layout_leg(pieces, mode=1):
    return lambda: dict(sc.crossing(8, 4000, seed=5, pieces=pieces), mode=mode)


for name, mk, kw in (("A", sc.scn_a, {}), ("B", sc.scn_b, {}), ("C", sc.scn_c, {}), ("H8", lambda: sc.hard(8, 8000), {}), ("Bc", lambda: dict(sc.scn_b(), mode=2), {}), ("Cc", lambda: dict(sc.scn_c(), mode=2), {}),
                     ("B-optplane", sc.scn_b, {"optimal_plane": 1}), ("fleet100", lambda: sc.crossing(100, 20000, seed=121), {}), ("fleet256", lambda: sc.crossing(256, 20000, seed=31), {}), ("P7", lambda: sc.crossing(8, 8000, seed=5, pieces=7), {}),
                     ("P8", layout_leg(8), {}), ("P10", layout_leg(10), {}), ("P11", layout_leg(11), {}), ("P19", layout_leg(19), {}), ("P27", layout_leg(27), {}), ("P20c", layout_leg(20, mode=2), {}),
                     ("H8tri", lambda: sc.triangulate(sc.hard(8, 8000), size=0.025), {}), ("H8tri-c", lambda: dict(sc.triangulate(sc.hard(8, 8000), size=0.025), mode=2), {})):
    s = pkg.Solver(mk(), stop=0.0, **kw)
    for b in (1, n // 2, n - 1 - n // 2):
        s.iterate_async(b); s.sync()
    st, t = s.get_state(), s.stats()
    h = hashlib.sha256()
    for k in sorted(st): h.update(np.ascontiguousarray(st[k]).tobytes())
    print(f"{name:11s} {h.hexdigest()[:20]} err {t['error_bits']} planes_self {t['planes_self']} pair_solves/it {t['pair_solves'] / n:.1f} evals {t['energy_evals']}   {ls_layout(s)}", flush=True)
    s.close()
