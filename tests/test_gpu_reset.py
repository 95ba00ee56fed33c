"""GPU (-m gpu): reset() -- tj_init_state on a context that has run -- gives a fresh context.  Which arrays it refills is stated by the declaration table
(csrc/tj_api.hip: device_arrays; tests/test_arrays.py pins the table), and this is the behaviour the table has to keep: a context that iterated, was reset and
iterates again ends, bit for bit, where a new context ends.  bench.py times exactly that sequence (warm-up, reset, timed iterations)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the fields of stats() that count work.  Left out by name: head_starts, async_fallbacks, ls_giveups, ls_helper_timeouts, gjk_max_sum, order_* describe the launch
# shape, the queues or the host's history and are no result of the iterations; pair_tests is a formula of iters
COUNTED = ("iters", "nodes_dcd", "cand_dcd", "nodes_ccd", "cand_ccd", "planes_obs", "planes_self", "energy_evals", "newton_iters", "pair_solves",
           "llt_fail_piece", "llt_fail_robot", "error_bits")


def _caches(s, mode):
    if mode == 0:
        return [a for ids, cd in s.get_obs_cache() for a in (ids, cd)]
    return list(s.get_pair_cache())


@pytest.mark.parametrize("optimal_plane", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reset_context_equals_fresh_context(pkg, scenes, mode, optimal_plane):
    scene = dict(scenes.tiny(mode, U=3)); scene["mode"] = mode
    a = pkg.Solver(scene, stop=0.0, optimal_plane=optimal_plane)
    a.iterate(5); a.reset(); a.iterate(3)
    b = pkg.Solver(scene, stop=0.0, optimal_plane=optimal_plane)
    b.iterate(3)
    sa, sb = a.get_state(), b.get_state()
    for k in sb:
        assert np.array_equal(sa[k], sb[k]), k
    (ca, pa), (cb, pb) = a.get_planes(), b.get_planes()
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb)
    assert np.array_equal(a.last_armijo_steps(), b.last_armijo_steps())
    assert np.array_equal(a.energy(), b.energy())
    if optimal_plane:
        xa, xb = _caches(a, mode), _caches(b, mode)
        assert len(xa) == len(xb) and all(np.array_equal(p, q) for p, q in zip(xa, xb))
    ta, tb = a.stats(), b.stats()
    assert {k: ta[k] for k in COUNTED} == {k: tb[k] for k in COUNTED}
    assert tb["iters"] == 3 and tb["error_bits"] == 0
    a.close(); b.close()
