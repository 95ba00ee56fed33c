"""GPU: what a context enqueues is the pure launch sequence (csrc/host_launch.h) at the context's own plan, facts and state -- for a batch of three iterations
and for tj_profile_kernels(2), at the small shapes of tests/test_gpu_plan.py: the records of the live context equal the pure function's, tj_launch_count grows by
the number of kernel records, and the per-kernel counts of the profile are the sequence's."""
import gc

import pytest

from test_plan import params

pytestmark = pytest.mark.gpu

SHAPES = [((0, 1, 2, 1), {}), ((1, 2, 2, 1), {}), ((2, 2, 2, 1), {}), ((1, 8, 5, 8), dict(optimal_plane=1)), ((1, 8, 5, 8), dict(rank=1, world=2))]
IDS = ["single", "decoupled", "coupled", "optplane", "rank1of2"]


def chain_pos(plan, wide_coupled, begun, more):
    """chain_position of csrc/host_launch.h"""
    folds = plan["mode"] != 2 or (wide_coupled and plan["lsc_wide"] and plan["u1"] - plan["u0"] == plan["U"])
    return ((1 if begun else 0) | (2 if more else 0)) if folds else 0


@pytest.fixture
def ctx(pkg, scenes, request):
    gc.collect()   # (solvers of earlier tests that were dropped unclosed give their queues back)
    (mode, U, P, res), kw = request.param
    scene = dict(scenes.scn_a(n_points=600, pieces=P) if mode == 0 else scenes.crossing(U, 600, pieces=P), mode=mode)
    s = pkg.Solver(scene, params={"res": res}, stop=0.0, kat=True, **kw)
    s.iterate(1)   # the hull cache is built, nothing is folded or deferred behind its flush
    facts, plan, _ = pkg.plan_record(ctx=s._ctx)
    tp = params(pkg, mode, U, P, res, kw.get("optimal_plane", 0), kw.get("rank", 0), kw.get("world", 1))
    assert pkg.plan_record(tp, facts)[1] == plan
    yield pkg, s, tp, facts, plan
    s.close()


def both(pkg, s, tp, facts, calls, profiling=False):
    """the sequence of the live context and of the pure function from the same start state: (state, records), equal"""
    flag = [1 if (profiling and k == "xs_same_queue_now") else 0 for k in pkg.SCHED_STATE]
    state, live = pkg.launch_records(calls, state=flag, ctx=s._ctx)
    _, pure = pkg.launch_records(calls, state=state, params=tp, facts=facts)
    assert live == pure
    return state, live


def kernel_records(pkg, recs):
    clear = len(pkg.KERNELS) + pkg.LAUNCH_EXTRA.index("xf_seg_clear")
    return sum(1 for _, _, ls in recs for l in ls if l[0] != clear)


@pytest.mark.parametrize("ctx", SHAPES, ids=IDS, indirect=True)
def test_a_batch_enqueues_the_pure_sequence(ctx):
    pkg, s, tp, facts, plan = ctx
    nk = len(pkg.KERNELS)
    calls = [(k, pkg.SCHED_CHAIN, chain_pos(plan, True, i > 0, i + 1 < 3)) for i in range(3) for k in range(nk)]
    state, recs = both(pkg, s, tp, facts, calls)
    n0 = s.launch_count()
    s.iterate_async(3)
    grew = s.launch_count() - n0
    after, _ = pkg.launch_records([], ctx=s._ctx)
    s.sync()
    assert grew == kernel_records(pkg, recs) and grew >= 3 * 5
    assert after == recs[-1][1]   # the context's state went where the sequence said
    assert s.stats()["error_bits"] == 0


@pytest.mark.parametrize("ctx", SHAPES, ids=IDS, indirect=True)
def test_the_profile_enqueues_the_pure_sequence(ctx):
    pkg, s, tp, facts, plan = ctx
    nk = len(pkg.KERNELS)
    calls = [(k, pkg.SCHED_CHAIN, chain_pos(plan, False, it > 0, it + 1 < 2)) for it in range(2) for k in range(nk)]
    state, recs = both(pkg, s, tp, facts, calls, profiling=True)
    assert state[pkg.SCHED_STATE.index("xs_same_queue_now")] == 1 and all(l[3] == 0 for _, _, ls in recs for l in ls)   # one queue
    n0 = s.launch_count()
    prof = s.profile_kernels(2)
    grew = s.launch_count() - n0
    assert grew == kernel_records(pkg, recs) + 2   # (+ k_flush and k_slack of the flush that ends the profile)
    counts = [sum(recs[it * nk + k][0] for it in range(2)) for k in range(nk)]
    assert [prof[name][1] for name in pkg.KERNELS] == counts
    assert s.stats()["error_bits"] == 0
