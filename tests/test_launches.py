"""CPU: what one iteration enqueues (csrc/host_launch.h) is decided by one pure function, run here through the test build's tj_kat_launches with no device.
tests/golden/launches_kat.json holds what launch_kernel did before the pure function existed, recorded on an MI355X from a build of the parent commit that
logged every call: (kernel id, schedule, chain position) -> the returned bool, the host state before and after, and every launch and counter clear it issued."""
import json
import os

import pytest

from conftest import GOLD
from test_plan import params

DOC = json.load(open(os.path.join(GOLD, "launches_kat.json")))
ROWS = DOC["rows"]


def replay(pkg, monkeypatch, row):
    """every recorded call of a context through the pure function: [(recorded call, before, exists, state after, launches)]"""
    monkeypatch.delenv("TJ_TUNE", raising=False)
    for k, v in row["env"].items():
        monkeypatch.setenv("TJ_" + k, str(v))
    tp = params(pkg, *(row[k] for k in ("mode", "U", "P", "res", "optimal_plane", "rank", "world")))
    out = []
    for seg in row["segments"]:
        calls, at = seg["calls"], 0
        while at < len(calls):   # runs of calls between which the host did not touch the state go through the hook together
            end = at + 1
            while end < len(calls) and "b" not in calls[end]:
                end += 1
            state, got = pkg.launch_records([c["c"][:3] for c in calls[at:end]], state=calls[at]["b"], params=tp, facts=row["facts"], follow=row["follow"])
            for c, (exists, after, launches) in zip(calls[at:end], got):
                out.append((seg["entry"], c, state, exists, after, launches))
                state = after
            at = end
    return out


def test_recording_covers_the_sequence(pkg):
    assert len(DOC["parent_commit"]) == 40 and DOC["compiler"]
    assert tuple(DOC["state"]) == pkg.SCHED_STATE and tuple(DOC["launch"]) == pkg.LAUNCH_FIELDS and tuple(DOC["kernels"]) == pkg.KERNELS + pkg.LAUNCH_EXTRA
    for r in ROWS:
        assert tuple(r["facts"]) == pkg.PLAN_FACTS
    calls = [c for r in ROWS for s in r["segments"] for c in s["calls"]]
    launches = [l for c in calls for l in c.get("l", [])]
    assert len(ROWS) >= 38 and len(calls) >= 3000
    # both outcomes of every existence rule (k_grad and k_xsolve exist in every schedule; the union kernels exist in every schedule that lists them: no stage does)
    K = {n: i for i, n in enumerate(DOC["kernels"])}
    for name in pkg.KERNELS:
        seen = {c["c"][3] for c in calls if c["c"][0] == K[name]}
        assert seen == ({1} if name in ("k_grad", "k_xsolve", "k_front", "k_mid", "k_ccd") else {0, 1}), (name, seen)
    # ... in each of the three schedules, both bits of the chain position, all three queues, the gates and the counter clear
    assert {c["c"][1] for c in calls} == {pkg.SCHED_STAGE, pkg.SCHED_CHAIN, pkg.SCHED_PHASE}
    assert {c["c"][2] for c in calls} == {0, 1, 2, 3}
    assert {c["c"][2] for c in calls if c["c"][1] == pkg.SCHED_PHASE} == {0, 1, 2}
    assert {l[3] for l in launches} == {0, 1, 2}
    for name in ("k_xs_gate", "k_keep_gate", "k_fa_gate", "xf_seg_clear"):
        assert any(l[0] == K[name] for l in launches), name
    # the forms: both variants of the templates, the checkpoint in k_begin, the band solve, both primitive kinds, the narrow and the wide coupled search
    form = lambda name: {l[1] for l in launches if l[0] == K[name]}
    assert form("k_begin") == {0, 1} and form("k_front") == {0, 1} and form("k_mid") == {0, 1} and form("k_grad") == {0, 1} and form("k_xsolve") == {-1, 16, 43}
    assert {l[2] for l in launches if l[0] == K["k_front"]} == {1, 3}
    assert {l[8] for l in launches if l[0] == K["k_ls_coupled"]} == {1, 4}
    # every field of the state moves somewhere, except what only a group sets (xch_wait_kernel) and a search that went on beyond its first table (lsc_base)
    for i, name in enumerate(pkg.SCHED_STATE):
        vals = {c[k][i] for c in calls for k in ("a", "b") if k in c}
        assert len(vals) >= 2 or name in ("xch_wait_kernel", "lsc_base"), name
    # the entry points and contexts the recording exists for
    entries = {s["entry"] for r in ROWS for s in r["segments"]}
    assert entries >= {"batch3", "single", "profile2", "stages", "phases", "folded_batch", "folded_flushed", "batch3_healed", "phases3"}
    assert any(r["facts"]["claim_refused"] for r in ROWS) and any(r["world"] == 2 and r["follow"] for r in ROWS) and any(r["optimal_plane"] for r in ROWS)
    assert {r["obstacles"] for r in ROWS} == {"cloud", "mesh", "none"} and {r["mode"] for r in ROWS} == {0, 1, 2} and max(r["U"] for r in ROWS) == 256
    switches = {f"{k}={v}" for r in ROWS for k, v in r["env"].items()}
    assert switches >= {"XS_ASYNC=0", "XS_ONE_QUEUE=1", "KEEP_ASYNC=0", "FRONT_ASYNC=0", "FRONT_ASYNC_ONE_QUEUE=1", "FRONT_ASYNC_MID=0", "GRAD_FOLD=0", "SEQ_FOLD=0", "C2_FOLD=0",
                        "COUPLED_UNITS=0", "LSC_WIDE=0", "LSC_WIDE=1", "XS_BAND=1", "XS_FAULT=2"}


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_sequence_reproduces_the_recorded_launches(pkg, monkeypatch, row):
    n = 0
    for entry, c, before, exists, after, launches in replay(pkg, monkeypatch, row):
        where = (entry, n, pkg.KERNELS[c["c"][0]], c["c"])
        assert exists == c["c"][3], where
        want = c.get("a", before)
        assert after == want, (where, {k: (g, w) for k, g, w in zip(pkg.SCHED_STATE, after, want) if g != w})
        want = c.get("l", [])
        assert len(launches) == len(want), (where, launches, want)
        for got, rec in zip(launches, want):
            assert got == rec, (where, {k: (g, w) for k, g, w in zip(pkg.LAUNCH_FIELDS, got, rec) if g != w})
        n += 1
    assert n == sum(len(s["calls"]) for s in row["segments"])
