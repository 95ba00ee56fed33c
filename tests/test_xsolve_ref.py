"""tests/xsolve_ref.py, the CPU restatement of the per-robot Newton solve, against itself, against the CPU oracle's real systems, and against the conditions
tests/test_gpu_xsolve.py relies on -- so that the reference alone meets them -- plus the sensitivity of the accuracy bar: five one-line faults planted
into the exact-form double solve must each miss it.  No GPU.

What the oracle's real blocks look like (found here, asserted below): nothing lies outside pattern(P); inside it entries are missing wherever a piece has no active plane
(different axes then do not couple), and the time variable couples with NO coordinate -- the arrow row of every real system is zero but for
its corner (the cross terms of Gradient_admm's blocks are zero).  The scenes therefore never exercise the arrow row's update; the generated systems fill it."""
import numpy as np
import pytest

import xsolve_ref as X

PS_MODE1 = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 20, 31)
PS_OTHER = (2, 6, 7, 8, 11, 20)
PS_ALL = PS_MODE1


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("P", PS_ALL)
def test_assemble_inverts_split_bitwise(P):
    rng = np.random.default_rng(P)
    for H in (X.spd(P, 1e8), X.indefinite(P, 1)):
        g = X.rhs(P, "random", 7)
        lg, lh = X.split(H, g, rng)
        H2, g2 = X.assemble(lg, lh)
        assert _bits(H2, H) and _bits(g2, g)
        n, m, _ = X.dims(P)
        if P > 1:      # a doubly covered entry is really split, and not half and half
            a, b = lh[0][9][9], lh[1][0][0]
            assert a != 0 and b != 0 and a != b and a + b == H[3][3]
        assert sum(lh[sp][18][18] != 0 for sp in range(P)) == 1


@pytest.mark.parametrize("P", PS_ALL)
def test_generators_fill_the_pattern(P):
    pat = X.pattern(P)
    n, m, _ = X.dims(P)
    assert pat[m].all() and pat[:, m].all() and np.array_equal(pat, pat.T)
    for i in range(m):      # a skyline of at most 17 below the diagonal, reaching 17 somewhere
        lo = np.flatnonzero(pat[i, :m])[0]
        assert i - lo <= X.BW and pat[i, lo:i + 1].all()
    assert any(pat[i, i - X.BW] for i in range(X.BW, m)) or m <= X.BW
    mats = [X.spd(P, c) for c in X.CONDS] + [X.indefinite(P, k) for k in X.indefinite_ks(P)] + [X.zero_first_pivot(P)]
    for H in mats[:-1]:
        assert np.array_equal(H != 0, pat) and _bits(H, H.T)
    Z = mats[-1]
    assert Z[0, 0] == 0.0 and np.array_equal((Z != 0) | np.eye(n, dtype=bool), pat)


@pytest.mark.parametrize("mode,P", [(1, P) for P in PS_MODE1] + [(mo, P) for mo in (0, 2) for P in PS_OTHER])
def test_real_systems_and_the_oracle_direction(scenes, mode, P):
    """the assembled real blocks lie inside pattern(P) (see the module docstring for what they leave empty), and the decimal solve of them gives the oracle's own
    direction record: normwise to cond * 64 n u, in modes 0 and 1 per robot, in mode 2 through the arrowhead system"""
    import ctypes as C
    from oracle.pyoracle import _d
    lg, lh, e = X.real(scenes, P, mode, want_engine=True)
    n, m, T = X.dims(P)
    pat = X.pattern(P)
    sys_ = []
    for u in range(e.U):
        H, g = X.assemble(lg[u], lh[u])
        assert not ((H != 0) & ~pat).any()
        assert (np.diag(H) > 0).all()
        assert H[m, m] > 0 and not H[m, :m].any() and not H[:m, m].any()
        sys_.append((np.tril(H) + np.tril(H, -1).T, g))
    if mode == 2:
        e.stage_update_spline()
        got = dict(direction=np.zeros((e.U, 3, T)), t=np.zeros(e.U))
        for u in range(e.U):
            a, b, c = C.c_double(), C.c_double(), C.c_double()
            e._f("get_direction")(C.c_int(u), _d(got["direction"][u]), C.byref(a), C.byref(b), C.byref(c))
            got["t"][u] = a.value
        xs, t, _ = X.coupled_hp([s[0] for s in sys_], [s[1] for s in sys_])
        cond = max(np.linalg.cond(s[0]) for s in sys_)
        want = np.concatenate([np.array([float(v) for v in x]) for x in xs] + [[float(t)]])
        have = np.concatenate([X.unrecord(got["direction"][u], got["t"][u])[:m] for u in range(e.U)] + [[-got["t"][0]]])
        assert np.linalg.norm(have - want) <= cond * 64 * n * X.U64 * np.linalg.norm(want)
        return
    got = e.stage_direction()
    for u, (H, g) in enumerate(sys_):
        x, piv = X.solve_hp(H, g)
        shift = 0.0
        if mode == 1 and not all(p > 0 for p in piv):      # the oracle took the eigen-shift fallback
            shift = 0.01 - float(np.linalg.eigvalsh(H)[0])
            x, _ = X.solve_hp(H, g, shift)
        cond = np.linalg.cond(H + shift * np.eye(n))
        want = X.record(np.array([float(v) for v in x]), g)
        tol = cond * 64 * n * X.U64
        have = X.unrecord(got["direction"][u], got["t_direction"][u])
        assert np.linalg.norm(have - np.array([float(v) for v in x])) <= tol * np.linalg.norm(have)
        assert not got["direction"][u][:, [0, 1, T - 2, T - 1]].any()
        assert abs(got["wolfe"][u] - want["wolfe"]) <= tol * np.sum(np.abs(have * g)) and abs(got["gn"][u] - want["gn"]) <= tol * want["gn"]


@pytest.mark.parametrize("P", PS_ALL)
def test_spd_classes_meet_what_the_gpu_tests_rely_on(P):
    """every exact pivot of the double-rounded matrix clears 100 n u max(diag); the exact form succeeds with a backward error within (3n + 1) u"""
    n, m, _ = X.dims(P)
    for cond in X.CONDS:
        for seed in range(3):
            H = X.spd(P, X.cond_for(P, cond), seed); g = X.rhs(P, "random", seed)
            x_hp, piv = X.solve_hp(H, g)
            assert float(min(piv)) > 100 * n * X.U64 * H.diagonal().max(), (cond, float(min(piv)))
            ok, x, _ = X.solve_f64(H, g)
            assert ok and X.eta(H, g, x) <= X.eta_cap(n)
    assert X.cond_for(2, 1e12) == 1e12 and X.cond_for(P, 1e8) == 1e8 and X.cond_for(P, 1e2) == 1e2


@pytest.mark.parametrize("P", PS_MODE1)
def test_failing_systems_fail_where_they_are_built_to(P):
    n, m, _ = X.dims(P)
    ks = X.indefinite_ks(P)
    assert {0, 1, m // 2, m - 1, m} <= set(ks) and ({17, 18} <= set(ks) or n <= 18)
    for k in ks:
        H = X.indefinite(P, k)
        assert np.linalg.eigvalsh(H)[0] <= -1e-6 * np.abs(H).max()
        ok, _, at = X.solve_f64(H, X.rhs(P, "random"))
        _, piv = X.solve_hp(H, X.rhs(P, "random"))
        assert not ok and at == k
        assert [i for i, p in enumerate(piv) if p <= 0][0] == k
    Z = X.zero_first_pivot(P)
    assert np.linalg.eigvalsh(Z)[0] <= -1e-6 * np.abs(Z).max()
    ok, _, at = X.solve_f64(Z, X.rhs(P, "random"))
    assert not ok and at == 0 and X.solve_hp(Z, X.rhs(P, "random"))[0] is None


def test_coupled_solves_agree():
    """the arrowhead system through the per-robot Schur complements, in decimal and in double, against one dense numpy solve of the whole system"""
    P = 3
    n, m, _ = X.dims(P)
    Hs = [X.spd(P, 1e2, u) for u in range(4)]; gs = [X.rhs(P, "random", u) for u in range(4)]
    N = 4 * m + 1
    A = np.zeros((N, N)); b = np.zeros(N)
    for u in range(4):
        s = slice(u * m, (u + 1) * m)
        A[s, s] = Hs[u][:m, :m]; A[N - 1, s] = A[s, N - 1] = Hs[u][m, :m]; A[N - 1, N - 1] += Hs[u][m, m]
        b[s] = gs[u][:m]; b[N - 1] += gs[u][m]
    want = np.linalg.solve(A, b)
    xs, t, _ = X.coupled_hp(Hs, gs)
    hp = np.array([float(v) for x in xs for v in x] + [float(t)])
    xf, tf = X.coupled_f64(Hs, gs)
    f64 = np.concatenate(xf + [[tf]])
    assert np.linalg.norm(hp - want) <= 1e-11 * np.linalg.norm(want) and np.linalg.norm(f64 - want) <= 1e-11 * np.linalg.norm(want)
    assert X.coupled_eta(Hs, gs, xf, tf) <= X.eta_cap(N)
    assert X.coupled_forward_error(xf, tf, xs, t) <= 1e-11


@pytest.mark.parametrize("P", (2, 7, 8, 11))
def test_planted_faults_miss_the_bar(P):
    """sensitivity: the exact-form solve passes check_a / check_b on the cases the GPU tests use; with one fault planted it misses them.  jreach reduced by one,
    the arrow row's update dropped, one refinement step of the reciprocal root removed (this one at cond = 1e2 alone), a back substitution that stops one
    short of the band's edge, an eigen-shift of 0.01 without -lambda_min."""
    rng = np.random.default_rng(P)
    n = X.dims(P)[0]
    reals = [(X.spd(P, 1e3, 77), X.rhs(P, "random", 77))]      # (a stand-in: this test is about the generated classes)
    cases = X.cases_a(P, reals)
    bars, hp = X.bars_a(cases)
    ratios = X.check_a(cases, [X.solve_f64(H, g)[1] for _, H, g in cases], bars, hp)
    assert max(max(r) for r in ratios.values()) == 1.0
    low = [c for c in cases if c[0] == "spd1e2"]
    lbars, lhp = X.bars_a(low)
    for mut, sub, sbars, shp in (("jreach", cases, bars, hp), ("arrow", cases, bars, hp), ("bandedge", cases, bars, hp), ("rsqrt", low, lbars, lhp)):
        if mut == "bandedge" and n <= X.BW + 1:
            continue      # (n = 16: no entry sits 17 below the diagonal)
        with np.errstate(all="ignore"):
            xs = [X.newton_f64(H, g, 0, mut)[0] for _, H, g in sub]
        with pytest.raises(AssertionError):
            X.check_a(sub, xs, sbars, shp)
    fails = X.cases_b(P)
    X.check_b(fails, [X.newton_f64(H, g, 1)[0] for _, H, g in fails])
    with np.errstate(all="ignore"):
        xs = [X.newton_f64(H, g, 1, "shift")[0] for _, H, g in fails]
    with pytest.raises(AssertionError):
        X.check_b(fails, xs)
