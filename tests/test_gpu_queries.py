"""GPU (-m gpu): the four read-only queries (audit, audit_timed, closest_approach, obstacle_approach) against each other on ONE context.

They share the staged copy of the nets and piece times a group hands in and one control block for the BVH walk's overflow bit (csrc/tj_api.hip), and
closest_approach runs k_audit_timed at level 0 into audit_timed's rows.  What each returns is pinned by its own test module; here: in whatever order
they are called, each returns what it returned first, a group returns what one context does, and a refused call leaves nothing behind for another."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QUERIES = {
    "audit": lambda s: s.audit(per_segment=True),
    "audit_timed": lambda s: s.audit_timed(per_segment=True),
    "closest": lambda s: s.closest_approach(),
    "obstacle": lambda s: s.obstacle_approach(),
    "audit_timed_L6": lambda s: s.audit_timed(levels=6),
    "audit_timed_default": lambda s: s.audit_timed(),
}
ORDER = ("audit", "audit_timed", "closest", "obstacle")


def same(x, y, what):
    assert x.keys() == y.keys(), what
    for k in x:
        assert np.array_equal(x[k], y[k]), (what, k)


def test_the_four_queries_in_any_order(pkg, scenes):
    scene = scenes.tiny(mode=1)
    first = None
    for ranks in (1, 2, 3):
        ctx = pkg.Solver(scene, stop=0.0) if ranks == 1 else pkg.Group(scene, [0] * ranks, stop=0.0)
        ctx.iterate(3)
        got = {n: QUERIES[n](ctx) for n in ORDER}
        for n in reversed(ORDER):
            same(QUERIES[n](ctx), got[n], (ranks, "reversed", n))
        got["audit_timed_L6"] = QUERIES["audit_timed_L6"](ctx)
        for n in ("closest", "audit_timed_default", "audit_timed_L6"):   # closest_approach reuses the timed buffers at level 0 in between
            r = QUERIES[n](ctx)
            got.setdefault(n, r)
            same(r, got[n], (ranks, "levels", n))
        for k in got["audit_timed_default"]:   # (per_segment only adds keys)
            assert np.array_equal(got["audit_timed_default"][k], got["audit_timed"][k]), (ranks, k)
        if first is None:
            first = got
        for n in got:
            same(got[n], first[n], (ranks, "one context", n))
        ctx.close()


def test_an_overflow_does_not_leak_through_the_shared_control_block(pkg, scenes):
    """the scene and method of test_gpu_audit.py::test_frontier_overflow_is_an_error_and_leaves_everything_usable: SCN-B at range 100 overflows the walk's
    frontier (TJ_ERR_CAPACITY = -3).  The bit one query's walk set is not seen by the other query's next call.  Two deliberate error returns."""
    slv = pkg.Solver(scenes.scn_b(), stop=0.0)
    slv.iterate(2)
    obst, aud = slv.obstacle_approach(), slv.audit()
    for bad, good, want, name in ((slv.audit, slv.obstacle_approach, obst, "audit"), (slv.obstacle_approach, slv.audit, aud, "obstacle_approach")):
        with pytest.raises(pkg.TrajAdmmError) as ei:
            bad(range=100.0)
        assert "-3" in str(ei.value) and "range" in str(ei.value), name
        assert slv.stats()["error_bits"] == 0
        same(good(), want, "after " + name)
        assert slv.stats()["error_bits"] == 0
    slv.close()
