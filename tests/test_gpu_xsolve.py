"""The x-update's Newton solve on systems the test chose: the PRODUCT kernels (k_xsolve<N>, k_xsolve<0>, k_xsolve_band, k_xsolve_c2, k_xsolve_c2_band) fed
through the known-answer setter tj_kat_set_local_grad, run alone by the stage API and read back with tj_get_direction, against tests/xsolve_ref.py: a 60-digit
decimal solve is the truth, the exact-form double solve (IEEE sqrt and /) is the yardstick.  tests/test_xsolve_ref.py shows on the CPU that the reference
meets the conditions relied on here and that five planted one-line faults each miss these bars.

One context per (mode, P, storage) on scenes.hard(8, 3000, pieces=P) (mode 0: scn_a(4000), one robot), res = 4; begin and grad run once, then per batch
set -> xsolve -> read.  Sizes: every kernel form and its edges -- P = 2..6 k_xsolve<16..52>, 7 k_xsolve<0> (pairwise register form, n = 61), 8..10 the LDS
form, 11, 12 the first band sizes, 20 (n = 178: more rows than two passes of 64 lanes), 31 (n = 277).

(a) accuracy: per system eta = ||g - H x||_2 / (||H||_F ||x||_2 + ||g||_2) and the forward error against the decimal solve, both evaluated in decimal.  The
    device may be at most 8 times the exact form's worst over the same class at the same P (FAST replaces a correctly rounded sqrt and a division by a
    refined reciprocal root of 1-2 ulp and a multiplication: up to ~3x per entry, 8 leaves a factor above 2), and eta never above (3n + 1) u.
(b) mode 1's fallback: failing robots (first non-positive pivot at 0, 1, 17, 18, m/2, m-1, m; a first pivot of exactly 0) next to SPD ones.
(c) default storage against TJ_XS_BAND=1 at P = 2..10, every record bit for bit, in all three modes (coupled: npiv = n-1 against last_pivot = false).
(d) placement: permuted over the robots, and alone in a fleet of one, a system's record keeps its bits.

Coupled mode: tj_get_direction's wolfe and gn are the fleet's totals, which k_ccd_self_seq -- a later stage -- forms from the per-robot partial sums; the
xsolve stage alone does not produce them, so mode 2 checks direction and t_direction.  The chain-only forms (c2_fold inside k_xsolve, the asynchronous
tickets) cannot be reached through the stage API: they stay covered by test_gpu_coupled.py's bitwise comparison (TJ_C2_FOLD=0) and the end-to-end tests.

Observed on MI355X (TJ_PRINT_OBSERVED=1 prints them), largest ratio to the exact form's class bar, (eta, forward error):
  mode form                      spd1e2       spd1e8       spd1e12      real
  0    registers (P = 2, 6, 7)   (1.5, 1.5)   (1.3, 1.6)   (0.98, 2.5)  (1.4, 1.1)
  0    LDS (P = 8)               (1.3, 0.86)  (0.68, 0.66) (0.61, 0.76) (1.1, 1.0)
  0    band (P = 11, 20)         (1.5, 2.8)   (1.8, 1.5)   (1.8, 1.1)   (0.57, 1.2)
  1    registers (P = 2 .. 7)    (1.5, 1.5)   (1.3, 1.7)   (1.6, 2.5)   (1.8, 1.6)
  1    LDS (P = 8 .. 10)         (1.4, 1.1)   (1.0, 1.2)   (1.4, 1.0)   (1.3, 1.4)
  1    band (P = 11 .. 31)       (1.5, 2.8)   (1.8, 1.5)   (1.8, 1.1)   (2.0, 2.0)
  2    registers (P = 2, 6, 7)   (0.99, 1.7)  (1.4, 1.0)   (1.1, 1.1)   (1.2, 0.96)
  2    LDS (P = 8)               (1.3, 1.3)   (0.94, 0.8)  (1.3, 0.4)   (1.0, 0.94)
  2    band (P = 11, 20)         (1.1, 0.95)  (1.3, 1.2)   (1.6, 0.99)  (2.4, 0.91)
(b): recovered shift off by at most 0.0022 of its bound; eta of the shifted systems at most 2.3 times the exact form's (P = 31).
The bar is 8 in every cell.  With four systems per class instead of eight, P = 2's spd1e12 class read 8.5 in forward error -- and so does the exact form
against itself once the system is scaled by 3 (tests/xsolve_ref.py, _PLAN_A): the spread of the yardstick, not an error of the device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import xsolve_ref as X

pytestmark = pytest.mark.gpu

PS = {1: (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 20, 31), 0: (2, 6, 7, 8, 11, 20), 2: (2, 6, 7, 8, 11, 20)}
PS_BOTH = tuple(range(2, 11))      # sizes the dense and the band storage share
FIELDS = ("direction", "t_direction", "wolfe", "gn")


def _obs(what, val):
    if os.environ.get("TJ_PRINT_OBSERVED"):
        print("OBSERVED xsolve", what, val)


# ---- the systems, built once per (mode, P): every slot entry carries its blocks, so a system keeps its bits wherever it is placed ------
_BATCHES = {}


def _entry(tag, H, g, seed):
    lg, lh = X.split(H, g, np.random.default_rng([seed, 9]))
    return dict(tag=tag, H=H, g=g, lg=lg, lh=lh)


def batches(scenes, mode, P):
    """{"a": [batch], "b": [batch], "clean": batch}; a batch is a list of U slot entries"""
    key = (mode, P)
    if key in _BATCHES:
        return _BATCHES[key]
    lg, lh = X.real(scenes, P, mode, U=8 if mode == 2 else 4)
    reals = [X.assemble(lg[u], lh[u]) for u in range(lg.shape[0])]
    out = {}
    if mode == 2:
        out["a"] = [[_entry(cls, H, g, 1000 * b + u) for u, (H, g) in enumerate(zip(Hs, gs))] for b, (cls, Hs, gs) in enumerate(X.cases_coupled(P, reals))]
        out["zero"] = [_entry("spd1e2", X.spd(P, 1e2, 300 + u), X.rhs(P, "zero"), 300 + u) for u in range(8)]
    else:
        ent = [_entry(cls, H, g, i) for i, (cls, H, g) in enumerate(X.cases_a(P, reals))]
        out["a"] = [ent[i:i + 8] for i in range(0, len(ent), 8)] if mode == 1 else [[e] for e in ent]
    if mode == 1:
        fill = [_entry("fill", X.spd(P, X.cond_for(P, 1e8), 200 + j), X.rhs(P, "random", 200 + j), 200 + j) for j in range(8)]
        fails = [_entry(name, H, g, 400 + i) for i, (name, H, g) in enumerate(X.cases_b(P))]
        out["clean"] = fill
        out["b"] = []
        for i in range(0, len(fails), 4):
            b = list(fill)
            for j, f in enumerate(fails[i:i + 4]):
                b[2 * j] = f
            out["b"].append(b)
    _BATCHES[key] = out
    return out


# ---- running a batch on the product kernels -------------------------------------------------------------------------------------
def make(pkg, scenes, mode, P, U=8, band=False):
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("TJ_XS_BAND", raising=False)
        if band:
            mp.setenv("TJ_XS_BAND", "1")
        scene = X.real_scene(scenes, P, mode, U)
        s = pkg.Solver(scene, {"res": 4}, stop=0.0, kat=True)
    plan = pkg.plan_record(ctx=s._ctx)[1]
    assert plan["xs_band"] == (1 if (band or P >= 11) else 0), (P, band, plan["xs_band"])
    s.run_stage("begin"); s.run_stage("grad")
    return s


def solve(s, batch):
    """set the batch's blocks, run the solve alone, read every robot's record; returns (records, rise of llt_fail_robot)"""
    assert len(batch) == s.U
    before = s.stats()["llt_fail_robot"]
    s.kat_set_local_grad(np.stack([e["lg"] for e in batch]), np.stack([e["lh"] for e in batch]))
    s.run_stage("xsolve")
    recs = []
    for u in range(s.U):
        d = np.zeros((3, s.T)); a, b, c = C.c_double(), C.c_double(), C.c_double()
        s._check(s.lib.tj_get_direction(s._ctx, u, d.ctypes.data_as(C.POINTER(C.c_double)), C.byref(a), C.byref(b), C.byref(c)))
        recs.append(dict(direction=d, t_direction=a.value, wolfe=b.value, gn=c.value))
    st = s.stats()
    assert st["error_bits"] == 0, st["error_bits"]
    return recs, st["llt_fail_robot"] - before


_RUNS = {}


def runs(pkg, scenes, mode, P, band):
    """every batch of (mode, P) through one context of the given storage: {"a": [(records, fails)], "b": [...], "clean": (records, fails), "zero": ...}"""
    key = (mode, P, band)
    if key not in _RUNS:
        bt = batches(scenes, mode, P)
        s = make(pkg, scenes, mode, P, U=1 if mode == 0 else 8, band=band)
        out = {k: [solve(s, b) for b in bt[k]] for k in ("a", "b") if k in bt}
        for k in ("clean", "zero"):
            if k in bt:
                out[k] = solve(s, bt[k])
        s.close()
        _RUNS[key] = out
    return _RUNS[key]


def same_bits(ra, rb, fields=FIELDS):
    return all(np.array_equal(np.asarray(ra[f]), np.asarray(rb[f])) for f in fields)


def check_record(e, rec, coupled=False):
    """the record's own consistency: fixed rows zero, and (decoupled, single) wolfe and gn against the device's own x and g within the summation bound"""
    T = rec["direction"].shape[1]
    assert not rec["direction"][:, [0, 1, T - 2, T - 1]].any()
    x = X.unrecord(rec["direction"], rec["t_direction"])
    if coupled:
        return x
    g = e["g"]; n = len(g)
    if not np.any(g):
        assert not np.any(x) and rec["wolfe"] == 0 and rec["gn"] == 0      # (-0.0 passes)
        return x
    terms = x * g
    assert abs(rec["wolfe"] - math.fsum(terms)) <= X.sum_bound(terms), (e["tag"], rec["wolfe"])
    gn = math.sqrt(math.fsum(g * g))
    assert abs(rec["gn"] - gn) <= (n + 2) * X.U64 * gn, (e["tag"], rec["gn"], gn)
    return x


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,P", [(mo, P) for mo in (1, 0) for P in PS[mo]])
def test_spd_accuracy(pkg, scenes, mode, P):
    bt = batches(scenes, mode, P)
    out = runs(pkg, scenes, mode, P, False)
    ents = [e for b in bt["a"] for e in b]
    recs = [r for rs, fails in out["a"] for r in rs]
    assert all(fails == 0 for _, fails in out["a"])      # llt_fail_robot unchanged
    xs = [check_record(e, r) for e, r in zip(ents, recs)]
    cases = [(e["tag"], e["H"], e["g"]) for e in ents]
    bars, hp = X.bars_a(cases)
    ratios = X.check_a(cases, xs, bars, hp)
    _obs(("a", mode, P), {k: (float("%.2g" % v[0]), float("%.2g" % v[1])) for k, v in ratios.items()})


@pytest.mark.parametrize("P", PS[2])
def test_spd_accuracy_coupled(pkg, scenes, P):
    bt = batches(scenes, 2, P)
    out = runs(pkg, scenes, 2, P, False)
    assert all(fails == 0 for _, fails in out["a"])
    sols = []
    for b, (rs, _) in zip(bt["a"], out["a"]):
        xs = [check_record(e, r, coupled=True) for e, r in zip(b, rs)]
        assert len({r["t_direction"] for r in rs}) == 1      # the shared time direction: the same bits on every robot
        sols.append(([x[:-1] for x in xs], xs[0][-1]))
    cases = [(b[0]["tag"], [e["H"] for e in b], [e["g"] for e in b]) for b in bt["a"]]
    bars, hp = X.bars_coupled(cases)
    ratios = X.check_coupled(cases, sols, bars, hp)
    _obs(("a", 2, P), {k: (float("%.2g" % v[0]), float("%.2g" % v[1])) for k, v in ratios.items()})
    rs, fails = out["zero"]
    assert fails == 0 and not any(r["direction"].any() or r["t_direction"] != 0 for r in rs)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PS[1])
def test_failing_pivots_take_the_eigen_shift(pkg, scenes, P):
    """this also holds min_eig_lds to its bar at n = 16 .. 277, the band kernel's HBM scratch path with 256 threads included"""
    bt = batches(scenes, 1, P)
    out = runs(pkg, scenes, 1, P, False)
    clean, fails0 = out["clean"]
    assert fails0 == 0
    cases, xs = [], []
    for b, (rs, fails) in zip(bt["b"], out["b"]):
        failing = [u for u, e in enumerate(b) if e["tag"] != "fill"]
        assert fails == len(failing), (fails, failing)
        for u, (e, r) in enumerate(zip(b, rs)):
            x = check_record(e, r)
            if u in failing:
                cases.append((e["tag"], e["H"], e["g"])); xs.append(x)
            else:
                assert same_bits(r, clean[u]), (P, u)      # an SPD robot does not see its neighbours fail
    assert {c[0] for c in cases} == {n for n, _, _ in X.cases_b(P)}
    worst_s, worst_e = X.check_b(cases, xs)
    _obs(("b", P), dict(shift_error_over_bound=float("%.2g" % worst_s), eta_ratio=float("%.2g" % worst_e)))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,P", [(mo, P) for mo in (1, 0, 2) for P in PS_BOTH])
def test_storage_forms_agree_bitwise(pkg, scenes, mode, P):
    """registers (batched, pairwise) and LDS against the band form, on the batches of (a) and (b)"""
    a = runs(pkg, scenes, mode, P, False)
    b = runs(pkg, scenes, mode, P, True)
    fields = FIELDS[:2] if mode == 2 else FIELDS
    for k in ("a", "b"):
        for (ra, fa), (rb, fb) in zip(a.get(k, []), b.get(k, [])):
            assert fa == fb
            for u, (x, y) in enumerate(zip(ra, rb)):
                assert same_bits(x, y, fields), (mode, P, k, u)
    for k in ("clean", "zero"):
        if k in a:
            assert a[k][1] == b[k][1] and all(same_bits(x, y, fields) for x, y in zip(a[k][0], b[k][0])), (mode, P, k)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (2, 6, 7, 8, 11, 31))
def test_placement_changes_no_bit(pkg, scenes, P):
    bt = batches(scenes, 1, P)
    base = runs(pkg, scenes, 1, P, False)["b"][0]      # failing and SPD robots interleaved
    batch = bt["b"][0]
    perm = np.random.default_rng(P).permutation(8)
    s = make(pkg, scenes, 1, P)
    rs, fails = solve(s, [batch[i] for i in perm])
    s.close()
    assert fails == base[1]
    for slot, i in enumerate(perm):
        assert same_bits(rs[slot], base[0][i]), (P, slot, i)
    one = make(pkg, scenes, 1, P, U=1)
    for i in (0, 1):      # a failing robot and an SPD one, each alone in a fleet of one
        r1, f1 = solve(one, [batch[i]])
        assert same_bits(r1[0], base[0][i]) and f1 == (1 if batch[i]["tag"] != "fill" else 0), (P, i)
    one.close()


def test_setter_rejects_bad_arguments(pkg, scenes):
    s = make(pkg, scenes, 1, 2)
    lg = np.zeros((8, 2, 19)); lh = np.zeros((8, 2, 361))
    dp = C.POINTER(C.c_double)
    assert s.lib.tj_kat_set_local_grad(s._ctx, None, lh.ctypes.data_as(dp)) < 0
    assert s.lib.tj_kat_set_local_grad(s._ctx, lg.ctypes.data_as(dp), None) < 0
    assert s.lib.tj_kat_set_local_grad(None, lg.ctypes.data_as(dp), lh.ctypes.data_as(dp)) < 0
    with pytest.raises(ValueError):
        s.kat_set_local_grad(lg[:4], lh)
    tp = pkg.TjParams(); raw = C.c_void_p()      # a context without cloud and state is not ready
    s.lib.tj_default_params(C.byref(tp), 1, 8, 2)
    assert s.lib.tj_create(C.byref(tp), C.byref(raw)) >= 0
    assert s.lib.tj_kat_set_local_grad(raw, lg.ctypes.data_as(dp), lh.ctypes.data_as(dp)) < 0
    s.lib.tj_destroy(raw)
    rng = np.random.default_rng(0)
    lg = rng.normal(size=lg.shape); lh = rng.normal(size=lh.shape)
    s.kat_set_local_grad(lg, lh)
    for u in (0, 7):
        g, h = s.local_grad(u, 1)
        assert np.array_equal(g, lg[u, 1]) and np.array_equal(h.ravel(), lh[u, 1])
    s.close()
