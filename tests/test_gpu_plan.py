"""GPU: a context's launch plan is the pure planner's (csrc/host_plan.h) at the device's own facts, and the queue budget feeds back into it through one
re-plan.  Contexts are created and destroyed only: no iteration runs."""
import ctypes as C
import gc
import os

import pytest

from test_plan import params

pytestmark = pytest.mark.gpu


class Ctx:
    def __init__(self, pkg, *shape, **kw):
        self.pkg, self.lib, self.tp, self.ctx = pkg, pkg.load_library(kat=True), params(pkg, *shape, **kw), C.c_void_p()
        rc = self.lib.tj_create(C.byref(self.tp), C.byref(self.ctx))
        assert rc == 0, self.lib.tj_last_error(self.ctx).decode()
        self.facts, self.plan, _ = pkg.plan_record(ctx=self.ctx)

    def pure(self, **facts):
        return self.pkg.plan_record(self.tp, dict(self.facts, **facts))[1]

    def close(self):
        if self.ctx:
            self.lib.tj_destroy(self.ctx)
            self.ctx = None


@pytest.fixture
def make(pkg):
    gc.collect()   # (solvers of earlier tests that were dropped unclosed give their queues back)
    made = []
    def mk(*shape, **kw):
        made.append(Ctx(pkg, *shape, **kw))
        return made[-1]
    yield mk
    for c in made:
        c.close()


@pytest.mark.parametrize("shape,kw", [((0, 1, 2, 1), {}), ((1, 2, 2, 1), {}), ((2, 2, 2, 1), {}), ((1, 8, 5, 8), dict(optimal_plane=1)), ((1, 8, 5, 8), dict(rank=1, world=2))],
                         ids=["single", "decoupled", "coupled", "optplane", "rank1of2"])
def test_context_plan_is_the_pure_planner_at_the_device_facts(make, shape, kw):
    c = make(*shape, **kw)
    assert c.facts["num_cu"] > 0 and c.facts["xsolve_ok"] and c.facts["grad_ok"] and c.facts["grad_fold_ok"] and c.facts["front_ok"]
    assert c.plan == c.pure()
    assert c.plan["err"] == 0 and (c.plan["mode"], c.plan["U"], c.plan["P"], c.plan["res"]) == shape


def test_queue_budget_refusal_and_release(make):
    """default (8, 5, 8) contexts ask for two queues each: the one that no longer fits the process's budget gets the refused-claim plan (one queue), and
    once a holder is closed the next context gets its queues again"""
    budget = max(int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), 2) - 1   # the rule of hw_queue_budget() (csrc/tj_api.hip): keep the two alike
    ctxs = []
    while not (ctxs and ctxs[-1].facts["claim_refused"]):
        assert 2 * len(ctxs) <= budget, "a context that does not fit the budget was not refused"
        ctxs.append(make(1, 8, 5, 8))
    first, last = ctxs[0], ctxs[-1]
    assert len(ctxs) >= 2 and not first.facts["claim_refused"]
    assert (first.plan["queues"], first.plan["xs_async"], first.plan["xs_two_queues"], first.plan["hwq_refused"]) == (2, 1, 1, 0) and first.plan == first.pure()
    assert last.plan == last.pure(claim_refused=1) and last.plan != last.pure(claim_refused=0)
    assert (last.plan["queues"], last.plan["xs_async"], last.plan["fa"], last.plan["xs_two_queues"], last.plan["hwq_refused"]) == (2, 0, 0, 0, 1)
    first.close()
    third = make(1, 8, 5, 8)
    assert not third.facts["claim_refused"] and third.plan == first.plan
