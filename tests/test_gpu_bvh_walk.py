"""GPU (-m gpu): the BVH build (csrc/kernels_bvh.h, and host_tables.h under TJ_BVH_HOST=1) and the walk (csrc/kernels_sep.h bvh_query) against brute force.

Every product kernel that looks at obstacles gets its candidates from bvh_query; a candidate the walk loses is invisible to all of them.  The walk ends in fp64
tests on the primitives themselves and its order is the Morton sort's, so the answer is a plain numpy expression (tests/bvh_ref.py, checked on the CPU by
tests/test_bvh_ref.py) and every comparison here is np.array_equal on the SEQUENCE a query returns (sort=False): that pins the candidate set, the build's order
and the compaction's order at once.  Covered: pyramids of one to five levels, top levels of 64 and of 9 boxes, partial last nodes on every level, the radix
sort's tile edges (2 048), the walk's four forms (unroll 4 / 1, with and without the prefetched top box), the two-levels-per-step loop on and off, points and
triangles, coordinates far from the origin (where outward rounding moves a box by up to 0.06), axes without extent, 1 000 equal keys, float32 denormals, and
the frontier's capacity at 1 024 against 1 025.  Not covered: the walk's `visits` counter."""
import numpy as np
import pytest

import bvh_ref as B

pytestmark = pytest.mark.gpu
FORMS = ((4, False), (4, True), (1, False), (1, True))      # tj_kat_query | k_front | the audit, the seeds, the planner | k_ccd


def solver(pkg, scenes, verts, monkeypatch, skip=None, host=False):
    sc = dict(scenes.tiny(1))
    sc["tris" if verts.ndim == 3 else "cloud"] = verts
    monkeypatch.delenv("TJ_BVH_SKIP", raising=False); monkeypatch.delenv("TJ_BVH_HOST", raising=False)
    if skip is not None:
        monkeypatch.setenv("TJ_BVH_SKIP", skip)                 # read when the context is created
    if host:
        monkeypatch.setenv("TJ_BVH_HOST", "1")
    s = pkg.Solver(sc, stop=0.0, kat=True)
    assert s.build_info()["on_device"] == (not host)
    return s


def flat(seqs):
    return np.array([len(x) for x in seqs]), (np.concatenate(seqs) if len(seqs) else np.zeros(0, dtype=np.int64))


def check(pkg, scenes, name, monkeypatch, host=False, answers_of=None):
    verts, boxes, margins = B.case(name)
    want = [flat(a) for a in B.answers(answers_of or name)]
    deep = len(B.level_counts(len(verts))) >= 3
    for skip in (("1", "0") if deep else (None,)):              # the two-levels-per-step loop exists from three levels on (default: off below five)
        s = solver(pkg, scenes, verts, monkeypatch, skip, host)
        for unroll, pre in FORMS:
            for m, (wn, wids) in zip(margins, want):
                gn, gids = flat(s.kat_query(boxes, m, sort=False, unroll=unroll, pre=pre))
                assert np.array_equal(gn, wn), (name, skip, unroll, pre, m, np.flatnonzero(gn != wn)[:8])
                assert np.array_equal(gids, wids), (name, skip, unroll, pre, m)
        assert s.stats()["error_bits"] == 0
        s.close()


@pytest.mark.parametrize("name", B.POINT_CASES)
def test_point_cloud_walk_is_brute_force_at_every_depth(pkg, scenes, name, monkeypatch):
    check(pkg, scenes, name, monkeypatch)


@pytest.mark.parametrize("name", B.TRI_CASES)
def test_triangle_walk_is_brute_force(pkg, scenes, name, monkeypatch):
    """tri4097_degenerate: three equal vertices per triangle -- its sequences are the point cloud's"""
    check(pkg, scenes, name, monkeypatch, answers_of="pt4097" if name == "tri4097_degenerate" else None)


@pytest.mark.parametrize("name", ["pt2049", "pt32769"])
def test_host_build_gives_the_same_sequences(pkg, scenes, name, monkeypatch):
    check(pkg, scenes, name, monkeypatch, host=True)


@pytest.mark.parametrize("name", B.EDGE_CASES)
def test_magnitude_and_degenerate_extent(pkg, scenes, name, monkeypatch):
    check(pkg, scenes, name, monkeypatch)


@pytest.mark.parametrize("skip", [None, "1"])
def test_frontier_capacity_at_1024_against_1025(pkg, scenes, monkeypatch, skip):
    """cubes [-h, h]^3 at margin 0.2 over the 20 000-point cloud, h on either side of the edge (neighbouring doubles, found by bisection on the restated boxes):
    1 024 leaf boxes in the frontier succeed and equal brute force, 1 025 are TJ_ERR_CAPACITY (-3) in every form -- deliberate error returns, after which the
    context answers again.  skip = "1": the same with the two-levels-per-step loop switched on.  That loop's own capacity check cannot fire (it runs on at most
    BVH_SKIP_MAX = 8 nodes of 64 grandchildren: 512 <= FRONT_CAP), so the edge is the single steps' in both settings."""
    b = B.built("pt20000")
    h0, f0, h1, f1 = B.capacity_edge(b, 0.2)
    assert f0 <= B.FRONT_CAP < f1, (f0, f1)
    ok, bad = np.array([[-h0] * 3 + [h0] * 3]), np.array([[-h1] * 3 + [h1] * 3])
    want = B.candidate_lists(b, ok, 0.2)[0]
    assert 0 < len(want) <= 8192
    s = solver(pkg, scenes, B.case("pt20000")[0], monkeypatch, skip)
    for unroll, pre in FORMS:
        assert np.array_equal(s.kat_query(ok, 0.2, cap=8192, sort=False, unroll=unroll, pre=pre)[0], want), (unroll, pre, f0)
        with pytest.raises(pkg.TrajAdmmError) as ei:
            s.kat_query(bad, 0.2, cap=8192, sort=False, unroll=unroll, pre=pre)
        assert "error -3" in str(ei.value) and "margin" in str(ei.value) and "range" not in str(ei.value), (unroll, pre, str(ei.value))
        assert s.stats()["error_bits"] == 0
        assert np.array_equal(s.kat_query(ok, 0.2, cap=8192, sort=False, unroll=unroll, pre=pre)[0], want), ("after the overflow", unroll, pre)
    s.close()
