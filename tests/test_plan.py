"""CPU: the launch plan of a context (csrc/host_plan.h) is decided by one pure function, run here through the test build's tj_kat_plan with no device.
tests/golden/schedule_kat.json holds what tj_create decided before the planner existed, recorded on an MI355X: parameters, switches and the device facts it saw
-> every field of the plan."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLD

DOC = json.load(open(os.path.join(GOLD, "schedule_kat.json")))
ROWS = DOC["rows"]
UNSUPPORTED = -5


def _row_id(r):
    sw = ",".join(f"{k}={v}" for k, v in r["env"].items())
    tags = [f"m{r['mode']}-U{r['U']}-P{r['P']}-r{r['res']}"] + (["optplane"] if r["optimal_plane"] else []) + ([f"rank{r['rank']}of{r['world']}"] if r["world"] > 1 else []) + \
           ([sw] if sw else []) + (["counters"] if r["counters_on"] else []) + (["refused" if r["facts"]["claim_refused"] else "second"] if r["holder"] else [])
    return "-".join(tags)


def params(pkg, mode, U, P, res, optimal_plane=0, rank=0, world=1):
    tp = pkg.TjParams()
    pkg.load_library(kat=True).tj_default_params(C.byref(tp), mode, U, P)
    tp.res, tp.optimal_plane, tp.rank, tp.world = res, optimal_plane, rank, world
    return tp


def plan(pkg, monkeypatch, row, facts=None, env=None):
    monkeypatch.delenv("TJ_TUNE", raising=False)
    for k, v in (row["env"] if env is None else env).items():
        monkeypatch.setenv("TJ_" + k, str(v))
    return pkg.plan_record(params(pkg, *(row[k] for k in ("mode", "U", "P", "res", "optimal_plane", "rank", "world"))), facts or row["facts"])


def test_recording_covers_the_plan(pkg):
    assert len(DOC["parent_commit"]) == 40 and DOC["compiler"]
    assert len(ROWS) >= 90
    for r in ROWS:
        assert tuple(r["facts"]) == pkg.PLAN_FACTS and tuple(r["plan"]) == pkg.PLAN_FIELDS
    # the cases the recording exists for are in it: both outcomes of every edge
    seen = lambda k: {r["plan"][k] for r in ROWS}
    for k in ("xs_band", "pair_rows", "mid_order", "grad_bal", "lsc_wide", "xs_async", "keep_async", "fa", "fa_mid_ok", "hwq_refused", "forced", "xf", "xf_all", "c2_fold", "grad_fold", "seq_tree"):
        assert len(seen(k)) >= 2, k
    assert any(r["facts"]["counters_on"] for r in ROWS) and any(r["facts"]["claim_refused"] for r in ROWS)


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_planner_reproduces_the_recorded_decisions(pkg, monkeypatch, row):
    facts, got, msg = plan(pkg, monkeypatch, row)
    assert facts == row["facts"]
    assert got == row["plan"], {k: (got[k], row["plan"][k]) for k in got if got[k] != row["plan"][k]}
    assert msg == ""


@pytest.mark.parametrize("shape,text", [
    ((1, 2049, 5, 8), "more than 2048 robots are not supported (pair keys pack robot ids into 11 bits; the dense [S][U][U] plane tables are 5.4 GB + 0.7 GB there)"),
    ((0, 1, 64, 8), "more than 511 segments per robot are not supported by the line-search kernel"),
    ((1, 8, 5, 17), "res > 16 segments per piece is not supported by the gradient kernel"),
    ((0, 1, 60, 8), "problem does not fit the 160 KB LDS of one CU (segments per robot / fleet size too large for this version)"),   # 480 segments, res 8, one robot: only the LDS fit fails
], ids=["U2049", "S512", "res17", "lds"])
def test_unsupported_shapes(pkg, monkeypatch, shape, text):
    monkeypatch.delenv("TJ_TUNE", raising=False)
    _, got, msg = pkg.plan_record(params(pkg, *shape), ROWS[0]["facts"])
    assert got["err"] == UNSUPPORTED and msg == text


def test_unsupported_precedence(pkg, monkeypatch):
    """U > 2048, then S > 511, then res > 16, then the LDS fit"""
    monkeypatch.delenv("TJ_TUNE", raising=False)
    msg = lambda *shape: pkg.plan_record(params(pkg, *shape), ROWS[0]["facts"])[2]
    assert msg(1, 2049, 32, 17).startswith("more than 2048 robots")
    assert msg(1, 2048, 32, 17).startswith("more than 511 segments")
    assert msg(1, 2048, 30, 17).startswith("res > 16")
    assert msg(1, 2048, 60, 8).startswith("problem does not fit")


@pytest.mark.parametrize("prim", [1, 3])
@pytest.mark.parametrize("grad_bal", [0, 1])
@pytest.mark.parametrize("spec", [0, 1])
def test_front_grid_is_the_one_the_residency_rule_used(pkg, monkeypatch, prim, grad_bal, spec):
    """Dev::fa_mid is sound only if the k_front grid of the rule is the grid launch_kernel launches: both come from plan_grids"""
    row = next(r for r in ROWS if (r["mode"], r["U"], r["P"], r["res"]) == (1, 64, 5, 8) and not r["env"] and not r["holder"] and not r["counters_on"])
    facts = dict(row["facts"], prim=prim, n_obs=1000)
    _, got, _ = plan(pkg, monkeypatch, row, facts, env={"GRAD_BALANCE": grad_bal, "PAIR_HEAD_START": spec})
    assert (got["fa"], got["grad_bal"], got["spec"], got["prim"], got["N"]) == (1, grad_bal, spec, prim, 1000)
    assert got["n_rows"] == row["plan"]["n_rows"] == 320 and got["n_ccd"] == 64 * 40 + 320 and got["n_obs_solve"] == 1024
    assert got["n_front"] == got["fa_mid_front"] == got["n_ccd"] + 128 * spec + 5 * grad_bal
