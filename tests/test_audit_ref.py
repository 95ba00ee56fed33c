"""CPU: the reference values tests/test_gpu_audit.py holds tj_audit to (tests/audit_ref.py) are themselves checked here, without a GPU --
the prefiltered brute force equals the unfiltered one (the kernel's exactness argument), the GJK's |v| is the Euclidean distance (against an
enumeration that shares nothing with GJK), the restated speed / acceleration terms are the derivatives of the flown curve, and every
constructed input of the GPU tests has the property it was built for.  States come from the CPU engine (oracle.pyoracle.Engine("port"))."""
import numpy as np
import pytest

import audit_ref as R
from conftest import scene_by_name
from test_oracle_params import PARAM_SETS

# |openGJK's |v| - exact_distance| per case class: the worst value seen with the REFERENCE's openGJK (oracle/_ref/libref.so; the port is pinned
# to it bit for bit) on the cases of test_gjk_norm_is_the_distance, and the bar derived from it: 16x, floor 1e-15 (one rounding of a norm of size
# ~1).  tests/test_gpu_audit.py imports GJK_BAR for the device's clearances.  Two classes are FINDINGS, far off rounding level, and are stated
# limits of obs_clearance -- they do not widen the bars of the other classes:
#   triangle   openGJK stops on its relative tolerance with a simplex that is not yet the nearest face: |v| up to 4.5e-13 ABOVE the distance
#   vertex, inside   a primitive on a hull vertex / inside a solid hull: |v| is 1e-5 / 5.3e-7 where the distance is 0 (the same stopping rule; on
#              the straight initial trajectory, whose hulls are segments, it IS 0.0 -- test_start_in_collision_is_reported).  A point on a
#              triangle of hull vertices (face) is at rounding level, 3.7e-17, and keeps the floor.
GJK_WORST_SEEN = {"point": 1.2e-16, "pair": 8.9e-16, "triangle": 4.5e-13, "vertex": 1.0e-5, "inside": 5.3e-7, "face": 3.7e-17}
GJK_BAR = {k: max(16 * v, 1e-15) for k, v in GJK_WORST_SEEN.items()}

# |float64 restatement - longdouble curve| relative to the robot's peak speed / acceleration, worst over test_limit_terms_are_the_curves_derivatives
LIMITS_WORST_SEEN = 4.7e-13
LIMITS_BAR = max(16 * LIMITS_WORST_SEEN, 1e-15)


def states(pkg, scenes):
    """(name, scene, params, state) on which the CPU checks run"""
    tiny, hard = scenes.tiny(mode=1), scenes.hard()
    out = []
    for it in (0, 5):
        out.append((f"hard{it}", hard, None, R.port_state(hard, it)))
        out.append((f"tiny{it}", tiny, None, R.port_state(tiny, it)))
    tri = scenes.triangulate(tiny)
    out.append(("tiny_tri5", tri, None, R.port_state(tri, 5)))
    hs = scene_by_name(scenes, "hard_single")
    out.append(("hard_single5", hs, None, R.port_state(hs, 5)))
    for tag in ("A", "B"):
        out.append((f"hard{tag}5", hard, PARAM_SETS[tag], R.port_state(hard, 5, PARAM_SETS[tag])))
    return out


@pytest.fixture(scope="module")
def cpu_states(pkg, scenes):
    return states(pkg, scenes)


def prim_array(scene):
    return np.asarray(scene["tris"] if scene.get("tris") is not None else scene["cloud"], dtype=np.float64)


@pytest.mark.parametrize("engine", R.engines())
def test_prefiltered_brute_force_equals_unfiltered(pkg, cpu_states, engine):
    """the kernel's exactness argument without a GPU: restricting the candidates to primitives whose point / box lies within `range` of the hull's
    box (what bvh_query's last comparison keeps) loses no primitive closer than `range` -- values and indices, at the default range, 1.0 and 0.05
    (below every offset used)"""
    pr = R.prims(kind=engine)
    for name, scene, params, st in cpu_states:
        p = R.params_of(pkg, params)
        H = R.hulls_of(pkg, st["spline"], scene["P"], p["res"])
        X = prim_array(scene)
        d, ids = R.all_obs(pr, H, X)
        assert np.all(ids >= 0) and np.all(np.isfinite(d))
        for rng in (R.default_range(p), 1.0, 0.05):
            want = R.cap(d, ids, rng)
            got = R.brute_obs(pr, H, X, rng, prefilter=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, rng)
            if name == "tiny5":   # the slow literal form (Prims.gjk per call) agrees with the pointer form
                lit = R.brute_obs(pr, H[:1, :8], X, rng, prefilter=False)
                assert np.array_equal(lit[0], want[0][:1, :8]) and np.array_equal(lit[1], want[1][:1, :8])


def gjk_cases(pkg, scenes):
    """(class, A, B) for the truth check"""
    out = []
    hard = scenes.hard()
    st = R.port_state(hard, 5)
    H = R.hulls_of(pkg, st["spline"], 5, 8)
    cloud = hard["cloud"]
    for u in range(4):
        for tr in range(40):
            lo, hi = H[u, tr].min(0), H[u, tr].max(0)
            near = np.flatnonzero(~((cloud + 0.3 < lo) | (cloud > hi + 0.3)).any(axis=1))
            out += [("point", H[u, tr], cloud[i:i + 1]) for i in near[:12]]
    for tr in range(0, 40, 3):
        out += [("pair", H[a, tr], H[b, tr]) for a in range(4) for b in range(a + 1, 4)]
    tri = scenes.triangulate(scenes.tiny(mode=1))
    Ht = R.hulls_of(pkg, R.port_state(tri, 5)["spline"], 5, 8)
    T = tri["tris"]
    for u in range(3):
        for tr in range(40):
            lo, hi = Ht[u, tr].min(0), Ht[u, tr].max(0)
            near = np.flatnonzero(~((T.max(1) + 0.5 < lo) | (T.min(1) > hi + 0.5)).any(axis=1))
            out += [("triangle", Ht[u, tr], T[i]) for i in near[:6]]
    scene, st, cases = R.contact_cases(pkg, scenes)
    Hc = R.hulls_of(pkg, st["spline"], 5, 8)
    out += [(kind, Hc[u, tr], scene["cloud"][i:i + 1]) for u, tr, i, kind in cases]
    _, so = R.overlap_state(pkg, scenes)
    Ho = R.hulls_of(pkg, so["spline"], 5, 8)
    out += [("pair", Ho[0, tr], Ho[1, tr]) for tr in range(0, 40, 8)]
    return out


@pytest.mark.parametrize("engine", R.engines())
def test_gjk_norm_is_the_distance(pkg, scenes, engine):
    """|v| of openGJK against exact_distance.  Measured with the reference's openGJK: point 1.2e-16 (1 391 cloud points within 0.3 of a hull's box,
    hard() after 5 iterations), pair 8.9e-16 (hull pairs of hard(), coordinates ~4, so one rounding of a coordinate difference is 4.4e-16; the two
    parallel hulls 1e-3 apart of overlap_state: 2e-19), triangle 4.5e-13 (3 of 86 cases above 1e-15, all with |v| too LARGE: a finding), vertex
    1.0e-5 and inside 5.3e-7 (findings), face 3.7e-17.  Bars: GJK_BAR above, 16x each class's worst, floor 1e-15.  The port's GJK -- what a machine
    without the reference falls back to -- is held to the same bars."""
    pr = R.prims(kind=engine)
    worst = {}
    for kind, A, B in gjk_cases(pkg, scenes):
        x = R.norm3(pr.gjk(A, np.asarray(B).reshape(-1, 3)))
        worst[kind] = max(worst.get(kind, 0.0), abs(x - R.exact_distance(A, B)))
    print("GJK vs exact, worst per class:", worst)
    for kind, w in worst.items():
        assert w <= GJK_BAR[kind], (kind, w)


def test_exact_distance_on_known_answers():
    """the enumeration itself: unit cube against points, a parallel square, an edge-edge configuration, containment"""
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=float)[:6]   # a wedge of the unit cube
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.0]])
    assert R.exact_distance(sq, [[0.25, 0.25, 2.0]]) == 2.0
    assert R.exact_distance(sq, [[2.0, 0.5, 0.0]]) == 1.0
    assert abs(R.exact_distance(sq, [[2.0, 2.0, 1.0]]) - np.sqrt(3.0)) <= 2.3e-16
    assert R.exact_distance(sq, sq + [0, 0, 0.5]) == 0.5
    assert abs(R.exact_distance([[0, 0, 0], [1, 0, 0.0]], [[0.5, -1, 1], [0.5, 1, 1.0]]) - 1.0) <= 1e-18
    assert R.exact_distance(cube, [[0.2, 0.2, 0.2]]) == 0.0
    assert R.exact_distance(cube, cube * 0.5 + 0.1) == 0.0


def test_limit_terms_are_the_curves_derivatives(pkg, scenes):
    """the j = 0 speed / acceleration term of every segment is |velocity| / |acceleration| of the flown curve at the segment's start, with the robot's
    OWN piece_time and the segment's table weight; the segment's largest term bounds |v|, |a| at 16 interior parameters (the derivative's control
    polygon).  States: hard() after 5 iterations (decoupled: four different piece_time), set A after 5, P = 3 at res = 15 and 16 after 3.
    Measured here, relative to the robot's peak speed / acceleration: 4.7e-13 at worst (an acceleration term: the second difference of coordinates
    ~4 cancels three to four digits; speed terms alone ~4e-14); LIMITS_BAR is 16x that, 7.5e-12."""
    cases = [(scenes.hard(), None, 5), (scenes.hard(), PARAM_SETS["A"], 5), (dict(scenes.hard(4, 3000, pieces=3)), {"res": 15}, 3),
             (dict(scenes.hard(4, 3000, pieces=3)), {"res": 16}, 3)]
    worst = 0.0
    for scene, params, its in cases:
        st = R.port_state(scene, its, params)
        P, res = scene["P"], R.params_of(pkg, params)["res"]
        if params is None:
            assert len(set(st["piece_time"])) == scene["U"]          # every robot its own piece_time
        lim = R.limits_of(pkg, st, P, res)
        for u in range(scene["U"]):
            sp, ac = R.limit_terms(pkg, st, P, res, u)
            assert lim[u][0] == sp.max() and lim[u][2] == ac.max()
            for tr in range(P * res):
                v, a = R.curve_derivatives(pkg, st, P, res, u, tr)
                worst = max(worst, float(abs(sp[tr, 0] - R.ldnorm(v)) / lim[u][0]), float(abs(ac[tr, 0] - R.ldnorm(a)) / lim[u][2]))
                for f in np.arange(1, 17) / 17.0:
                    v, a = R.curve_derivatives(pkg, st, P, res, u, tr, f)
                    assert R.ldnorm(v) <= sp[tr].max() * (1 + LIMITS_BAR) and R.ldnorm(a) <= ac[tr].max() * (1 + LIMITS_BAR), (u, tr, f)
    print("limits vs curve, worst relative to the peak:", worst)
    assert worst <= LIMITS_BAR


def test_constructed_inputs_have_the_property_they_were_built_for(pkg, scenes):
    """contact_cases, overlap_state, equal_minima_scene, range_corner_scene, threshold_scene (sets A and B: contact seen expected and not expected)
    and limit_piece_times assert their own preconditions; the tied primitives (a duplicated point, a duplicated triangle) are the nearest of their robot at
    bit-equal distance from both indices; crossing() fleets start with every inner robot equidistant from both neighbours"""
    pr = R.prims()
    scene, st, cases = R.contact_cases(pkg, scenes)
    assert len(cases) == 3
    _, so = R.overlap_state(pkg, scenes, gap=0.08)
    Ho = R.hulls_of(pkg, so["spline"], 5, 8)
    assert all(abs(R.norm3(pr.gjk(Ho[0, tr], Ho[1, tr])) - 0.08) <= 1e-15 for tr in range(40))
    tiny = scenes.tiny(mode=1)
    H = R.hulls_of(pkg, R.port_state(tiny, 0)["spline"], 5, 8)
    for kind in ("twin", "tris"):
        for i, j in ((40, 555), (555, 40)):
            R.tie_precondition(pr, H, 1, R.tie_scene(scenes, H, 1, 20, i, j, kind), i, j)
    R.equal_minima_scene(pkg, scenes)
    R.range_corner_scene(pkg, scenes)
    for tag in ("A", "B"):
        p = R.params_of(pkg, PARAM_SETS[tag])
        seen = set()
        for gap, contact, between in R.threshold_gaps(p):
            _, st_t, _, _ = R.threshold_scene(pkg, scenes, PARAM_SETS[tag], gap, contact, between)
            seen.add(contact)
            if between:
                R.limit_piece_times(pkg, st_t, 2, p)
        assert seen == {True, False}
    for U in (64, 65):
        sc = scenes.crossing(U, 600, seed=5)
        Hc = R.hulls_of(pkg, R.port_state(sc, 0)["spline"], 5, 8)
        g = R.FastGjk(pr)
        base = Hc.ctypes.data
        ties = 0
        for u in range(1, U - 1):
            lo, hi = (g.dist(6, base + ((u - 1) * 40 + 20) * 144, 6, base + (u * 40 + 20) * 144), g.dist(6, base + (u * 40 + 20) * 144, 6, base + ((u + 1) * 40 + 20) * 144))
            ties += lo == hi
        assert ties > 0   # equidistant neighbours exist bit for bit: the expected partner is the smaller robot (all_pair keeps it)
