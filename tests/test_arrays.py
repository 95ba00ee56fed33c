"""CPU: every device array of a context is declared once (csrc/tj_api.hip: device_arrays) -- name, extent, element size, checkpoint membership, what tj_init_state
fills it with -- and allocation, the checkpoint's regions, the reset and every host copy read that one table.  The test build hands the table out with no device
(tj_kat_arrays on the pure planner's Dev).  tests/golden/arrays_kat.json holds the tables of the commit before the declarations carried names and resets: extents,
sizes and checkpoint flags dumped from its device_arrays, the reset column written down by hand from its tj_init_state."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLD

DOC = json.load(open(os.path.join(GOLD, "arrays_kat.json")))
SHAPES = DOC["shapes"]
ROWS = json.load(open(os.path.join(GOLD, "schedule_kat.json")))["rows"]   # (the shapes' device facts are rows of the plan's recording)
# what tj_init_state uploads instead of filling: the initial state
UPLOADED = {"spline", "p_slack", "p_lambda", "t_slack", "t_lambda", "piece_time"}
# Checkpointed arrays that a reset leaves as they are, and why that is sound.  The lists: nothing reads an entry beyond the count, and the count is reset;
# kpair_cd: read only where kpair_on is set.  step_out: kernels only write it (the accepted step of the last line search, a diagnostic the host reads)
GOVERNED_BY = {"kobs_id": "kobs_n", "kobs_cd": "kobs_n", "kpair_list": "kpair_n", "kpair_cd": "kpair_on"}
WRITE_ONLY = {"step_out"}


def _shape_id(s):
    return f"m{s['mode']}-U{s['U']}-P{s['P']}-r{s['res']}" + ("-optplane" if s["optimal_plane"] else "") + (f"-rank{s['rank']}of{s['world']}" if s["world"] > 1 else "")


def params(pkg, mode, U, P, res, optimal_plane=0, rank=0, world=1):
    tp = pkg.TjParams()
    pkg.load_library(kat=True).tj_default_params(C.byref(tp), mode, U, P)
    tp.res, tp.optimal_plane, tp.rank, tp.world = res, optimal_plane, rank, world
    return tp


def table(pkg, monkeypatch, s):
    for k in [k for k in os.environ if k.startswith("TJ_")]:
        monkeypatch.delenv(k)
    return pkg.arrays_record(params(pkg, *(s[k] for k in ("mode", "U", "P", "res", "optimal_plane", "rank", "world"))), ROWS[s["facts_row"]]["facts"])


def test_recording_takes_every_branch_of_the_declarations():
    assert len(DOC["parent_commit"]) == 40 and DOC["fields"] == ["name", "n", "elem", "snap", "reset"]
    assert {s["mode"] for s in SHAPES} == {0, 1, 2} and {s["optimal_plane"] for s in SHAPES} == {0, 1} and {2, 7} <= {s["P"] for s in SHAPES}
    n_of = lambda s, name: {a[0]: a[1] for a in s["arrays"]}.get(name)
    assert {n_of(s, "xs_scr") == 1 for s in SHAPES} == {True, False}, "band and dense x-solve storage"
    assert {n_of(s, "xL") == s["U"] * (9 * s["P"] - 2) ** 2 for s in SHAPES if s["mode"] == 2} == {True, False}, "coupled factor: dense and band"
    assert any(s["world"] > 1 and n_of(s, "grad_cost") != s["U"] * s["P"] for s in SHAPES), "a rank that owns fewer robots than the fleet"
    assert any(s["U"] == 65 and n_of(s, "pairbits") == s["P"] * s["res"] * 65 * 2 for s in SHAPES), "two words per row of pairbits"
    for s in SHAPES:   # the optimal_plane tables: real in their own mode, one-element placeholders in the other
        if s["optimal_plane"]:
            assert (n_of(s, "kobs_id") > 1) == (s["mode"] == 0) and (n_of(s, "kpair_on") > 1) == (s["mode"] != 0)
        else:
            assert n_of(s, "kobs_id") is None and n_of(s, "kpair_on") is None


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_table_is_the_recorded_one(pkg, monkeypatch, shape):
    got = table(pkg, monkeypatch, shape)
    want = [tuple(a) for a in shape["arrays"]]
    assert [a[0] for a in got] == [a[0] for a in want]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_names_are_unique_and_the_checkpoint_is_reset(pkg, monkeypatch, shape):
    got = table(pkg, monkeypatch, shape)
    names = [a[0] for a in got]
    assert len(set(names)) == len(names)
    assert UPLOADED <= set(names)
    reset = {name: r for name, _, _, _, r in got}
    assert all(r in (0, 1, 2) for r in reset.values()) and not [n for n in UPLOADED if reset[n]], "the uploaded state is not filled as well"
    for name, _, elem, snap, r in got:
        assert elem in (4, 8) or name == "ctl"
        if not snap or r or name in UPLOADED:
            continue   # every checkpointed array is one the table resets or tj_init_state uploads ...
        # ... or one a reset cannot leave stale: nobody reads it before a kernel writes it, or the count / flags in front of it are reset
        assert name in WRITE_ONLY or reset[GOVERNED_BY[name]] == 1, name


def test_bad_arguments(pkg):
    lib = pkg.load_library(kat=True)
    out = (C.c_int * 8)(); names = C.create_string_buffer(16)
    assert lib.tj_kat_arrays(None, None, None, out, 8, names, 16) == 0
    tp = params(pkg, 1, 8, 5, 8)
    f = (C.c_int * len(pkg.PLAN_FACTS))(*[ROWS[4]["facts"][k] for k in pkg.PLAN_FACTS])
    n = lib.tj_kat_arrays(None, C.byref(tp), f, out, 8, names, 16)   # too small: the count, negated, nothing written
    assert n < -50 and names.value == b"" and list(out) == [0] * 8
    tp = params(pkg, 1, 2049, 5, 8)                                   # a shape the planner refuses
    assert lib.tj_kat_arrays(None, C.byref(tp), f, out, 8, names, 16) == 0
