"""The x-update's per-robot Newton solve (csrc/kernels_newton.h: k_xsolve<N>, k_xsolve<0>, k_xsolve_band, k_xsolve_c2, k_xsolve_c2_band; csrc/dev_linalg.h)
restated on the CPU: the structural pattern of the reduced system, its assembly from the per-piece blocks in the device's order of sums and the inverse of
that assembly, a 60-digit `decimal` solve that is the truth, the exact-form double solve that is the yardstick of the accuracy bar, the arrowhead system
of coupled mode, the direction record, seeded generators of systems that fill the whole permitted pattern, and the metrics the tests assert.  Plain
numpy / decimal; no GPU, no library of the project except (for `real`) the CPU oracle.

Reduced system of one robot with P pieces: n = 9P - 2 unknowns, m = n - 1 control-point coordinates + the time variable (reduced index m).  Reduced index
r < m is global coordinate r + 6; piece sp covers globals 9 sp .. 9 sp + 17 as its locals 0 .. 17 and the time variable as its local 18.

Conditioning classes.  spd(P, cond) grades the diagonal of L0 from 1 down to cond^-1/2, so cond(H) ~ cond and the smallest exact pivot is 1 / cond, with
max(diag) about 1.  The tests need every exact pivot of the double-rounded matrix above 100 n u max(diag); the 1e12 class misses that from n = 97 on
(100 n u = 1.1e-12 there), so cond_for(P, cond) = min(cond, 1 / (256 n u)) lowers it: 1e12 up to P = 4, 8.2e11 at P = 5 (n = 43), 2.3e11 at P = 11, 1.3e11
at P = 31 (n = 277).  The 1e2 and 1e8 classes keep their cond at every P.  tests/test_xsolve_ref.py checks every case."""
import math
from decimal import Decimal, localcontext

import numpy as np

U64 = 2.0 ** -53          # unit roundoff of a double
BW = 17                   # half-bandwidth of the band forms (XS_BAND)
PREC = 60                 # decimal digits of the high-precision solve
CONDS = (1e2, 1e8, 1e12)
RHS_KINDS = ("random", "e0", "e16", "e17", "e18", "em1", "em", "zero")


def dims(P):
    n = 9 * P - 2
    return n, n - 1, 3 * P + 3      # n, m, T


def _covering(r, P, m):
    """pieces that cover reduced index r (the time variable: all of them)"""
    if r == m:
        return list(range(P))
    g = r + 6
    return list(range(max(0, (g - 17 + 8) // 9), min(P - 1, g // 9) + 1))


def _piece_index(sp, P):
    """(reduced indices, locals) of piece sp: its locals whose global coordinate is an unknown, then the time variable"""
    n, m, _ = dims(P)
    loc = [a for a in range(18) if 0 <= 9 * sp + a - 6 < m]
    return np.array([9 * sp + a - 6 for a in loc] + [m]), np.array(loc + [18])


def pattern(P):
    """bool [n][n]: entry (i, j) is structural iff some piece covers both; the last row and column are dense"""
    n, m, _ = dims(P)
    pat = np.zeros((n, n), dtype=bool)
    for sp in range(P):
        red, _ = _piece_index(sp, P)
        pat[np.ix_(red, red)] = True
    return pat


def assemble(lg, lh):
    """reduced H[n][n], g[n] of one robot from its blocks lg[P][19], lh[P][19][19], with the device's sums in the device's order: 0 + first covering piece +
    second, the time-time entry over all P pieces in piece order (k_xsolve's gather, xs_entry).  Bit for bit what the kernels factor."""
    lg = np.asarray(lg, dtype=np.float64); lh = np.asarray(lh, dtype=np.float64).reshape(len(lg), 19, 19)
    P = len(lg)
    n = dims(P)[0]
    H = np.zeros((n, n)); g = np.zeros(n)
    for sp in range(P):      # piece order; every entry meets its covering pieces in ascending order
        red, loc = _piece_index(sp, P)
        H[np.ix_(red, red)] += lh[sp][np.ix_(loc, loc)]
        g[red] += lg[sp][loc]
    return H, g


def split(A, g, rng):
    """the inverse of assemble: blocks lg[P][19], lh[P][19][19] with assemble(lg, lh) == (A, g) bit for bit.  A doubly covered entry a goes out as
    a1 = fl(t a), t random in [1/2, 4/5], and a2 = a - a1 (exact, Sterbenz), the larger share to either piece at random; the time-time entry goes into one
    piece.  The locals no unknown belongs to (the fixed end points) are filled with junk the kernels must not read."""
    A = np.asarray(A, dtype=np.float64); g = np.asarray(g, dtype=np.float64)
    n = A.shape[0]; m = n - 1; P = (n + 2) // 9
    assert dims(P)[0] == n and np.array_equal(A, A.T)
    lh = rng.uniform(-1e3, 1e3, (P, 19, 19)); lg = rng.uniform(-1e3, 1e3, (P, 19))
    t = rng.uniform(0.5, 0.8, (n, n)); t = np.tril(t) + np.tril(t, -1).T
    swap = rng.random((n, n)) < 0.5; swap = np.tril(swap) | np.tril(swap, -1).T
    tg = rng.uniform(0.5, 0.8, n); sg = rng.random(n) < 0.5
    cov = [_covering(r, P, m) for r in range(n)]
    home = int(rng.integers(P))      # the piece that carries the time-time entry and the time gradient
    for sp in range(P):
        red, loc = _piece_index(sp, P)
        for i, a in zip(red, loc):
            if i == m:
                lg[sp][18] = g[m] if sp == home else 0.0
            else:
                c = cov[i]
                if len(c) == 1:
                    lg[sp][a] = g[i]
                else:
                    g1 = g[i] * tg[i]; first = (sp == c[0]) != bool(sg[i])
                    lg[sp][a] = g1 if first else g[i] - g1
            for j, b in zip(red, loc):
                if i == m and j == m:
                    lh[sp][18][18] = A[m][m] if sp == home else 0.0
                    continue
                c = [s for s in cov[i] if s in cov[j]]
                if len(c) == 1:
                    lh[sp][a][b] = A[i][j]
                else:
                    a1 = A[i][j] * t[i][j]; first = (sp == c[0]) != bool(swap[i][j])
                    lh[sp][a][b] = a1 if first else A[i][j] - a1
    return lg, lh


# ---- the truth: band-and-arrow LDL^T in decimal ------------------------------------------------------
def _dec(a):
    return [Decimal(float(v)) for v in a]


def solve_hp(H, g, shift=0.0, npiv=None):
    """(x, pivots) of (H + shift I) x = g in `decimal` at PREC digits: band (half-width 17) and arrow L D L^T and both substitutions, O(n 18^2 + n n / 2).
    pivots[k] = a_kk - sum_j l_kj^2 of the Cholesky factorisation (= D_k; no root is taken, so an indefinite matrix factors too); x is None if a pivot is
    exactly zero (the pivots up to it are returned).  npiv = n - 1: the last pivot is left as the Schur complement and (L, D, y) are returned instead of x
    (coupled mode's per-robot half)."""
    H = np.asarray(H, dtype=np.float64); n = H.shape[0]; m = n - 1
    with localcontext() as ctx:
        ctx.prec = PREC
        sh = Decimal(float(shift))
        lo = [max(0, i - BW) for i in range(n)]; lo[m] = 0
        L = [dict() for _ in range(n)]      # L[i][j], unit lower, inside band + arrow
        C = [dict() for _ in range(n)]      # C[i][j] = L[i][j] D[j]
        D = []
        for i in range(n):
            Li = L[i]; Ci = C[i]
            for j in range(lo[i], i + 1):
                s = Decimal(float(H[i, j])) + (sh if i == j else 0)
                Lj = L[j]
                for k in range(max(lo[i], lo[j]), j):
                    s -= Ci[k] * Lj[k]
                if j < i:
                    if D[j] == 0:
                        return None, D
                    Ci[j] = s; Li[j] = s / D[j]
                else:
                    D.append(s)
        y = _dec(g)
        for i in range(n):
            for k in range(lo[i], i):
                y[i] -= L[i][k] * y[k]
        if npiv is not None and npiv == n - 1:
            return L, D, y
        if any(d == 0 for d in D):
            return None, D
        x = [y[i] / D[i] for i in range(n)]
        for j in range(n - 1, -1, -1):
            for i in range(lo[j], j):
                x[i] -= L[j][i] * x[j]
        return x, D


def coupled_hp(Hs, gs):
    """the arrowhead system of coupled mode (Optimization3D_multi::update_spline): the block diagonal of the robots' m x m parts with ONE shared last row,
    whose diagonal and right-hand side are the sums over robots, solved through the per-robot Schur complements in decimal.  Returns (xs[U][m], t, corner)."""
    with localcontext() as ctx:
        ctx.prec = PREC
        parts = [solve_hp(H, g, npiv=np.asarray(H).shape[0] - 1) for H, g in zip(Hs, gs)]
        n = np.asarray(Hs[0]).shape[0]; m = n - 1
        corner = sum(p[1][m] for p in parts); rhs = sum(p[2][m] for p in parts)      # D[m] = h_tt - sum l_mk^2 d_k, y[m] the reduced rhs
        t = rhs / corner
        xs = []
        for L, D, y in parts:
            x = [y[i] / D[i] for i in range(m)]
            for i in range(m):
                x[i] -= L[m][i] * t
            for j in range(m - 1, -1, -1):
                for i in range(max(0, j - BW), j):
                    x[i] -= L[j][i] * x[j]
            xs.append(x)
        return xs, t, corner


# ---- the yardstick: the exact form in double -------------------------------------------------------------
MUTATIONS = ("jreach", "arrow", "rsqrt", "bandedge", "shift")


def _rsqrt_model(x, steps):
    """a reciprocal root as the FAST forms build it (pivot_rsqrt): a seed 2^-23 off -- the accuracy AMD's ISA manuals state for V_RSQ_F64, (2**29) ULP -- refined by
    Newton steps r += r/2 (1 - x r^2): two reach rounding level, one leaves 1.5 * 2^-46"""
    r = (1.0 / math.sqrt(x)) * (1.0 + 2.0 ** -23)
    for _ in range(steps):
        r = r + 0.5 * r * (1.0 - (x * r) * r)
    return r


def factor_f64(H, g, npiv=None, mutate=None):
    """the device's right-looking loop in its EXACT form (IEEE sqrt and /, a - l l rounded twice), in plain double: column k reaches rows up to
    min(k + 17, 9 ((k + 6) / 9) + 11, m - 1) plus the arrow row; the right-hand side rides along.  Returns (ok, first failing pivot or -1, L, y): L lower with
    the roots on the diagonal.  npiv = n - 1 leaves the Schur complement in L[m][m] and y[m] (coupled mode).  mutate: one of MUTATIONS (sensitivity checks only)."""
    A = np.array(H, dtype=np.float64); y = np.array(g, dtype=np.float64)
    n = A.shape[0]; m = n - 1
    npiv = n if npiv is None else npiv
    for k in range(npiv):
        x = A[k, k]
        if x <= 0:
            return False, k, A, y
        if mutate == "rsqrt":
            rs = _rsqrt_model(x, 1); s = None     # one refinement step where pivot_rsqrt takes two
        else:
            s = math.sqrt(x)
        A[k, k] = s if s is not None else 1.0 / rs
        if k == m:
            y[k] = y[k] / s if s is not None else y[k] * rs
            break
        jhi = min(k + BW, 9 * ((k + 6) // 9) + 11 - (1 if mutate == "jreach" else 0), m - 1)
        col = A[k + 1:jhi + 1, k] / s if s is not None else A[k + 1:jhi + 1, k] * rs
        la = A[m, k] / s if s is not None else A[m, k] * rs
        yk = y[k] / s if s is not None else y[k] * rs
        A[k + 1:jhi + 1, k] = col; A[m, k] = la; y[k] = yk
        A[k + 1:jhi + 1, k + 1:jhi + 1] -= np.outer(col, col)
        if mutate != "arrow":
            A[m, k + 1:jhi + 1] -= la * col
        A[m, m] -= la * la
        y[k + 1:jhi + 1] -= yk * col
        y[m] -= yk * la
    return True, -1, A, y


def backsolve_f64(L, y, mutate=None):
    """x = L^-T y, column oriented like the device's forms: the arrow row first, then row j down the band"""
    x = np.array(y, dtype=np.float64); n = len(x); m = n - 1
    x[m] = x[m] / L[m, m]
    x[:m] -= x[m] * L[m, :m]
    for j in range(m - 1, -1, -1):
        x[j] = x[j] / L[j, j]
        lo = max(0, j - BW + (1 if mutate == "bandedge" else 0))
        x[lo:j] -= x[j] * L[j, lo:j]
    return x


def solve_f64(H, g, mutate=None):
    """(ok, x, first failing pivot): the exact form's solve of H x = g in double, None where a pivot is not positive"""
    ok, k, L, y = factor_f64(H, g, mutate=mutate)
    return (True, backsolve_f64(L, y, mutate), -1) if ok else (False, None, k)


def newton_f64(H, g, mode, mutate=None):
    """the solve with mode 1's fallback (xs_wave0): on a failing pivot the diagonal is shifted by 0.01 - lambda_min and the factorisation repeated unchecked.
    Returns (x, failed)"""
    ok, x, _ = solve_f64(H, g, mutate)
    if ok:
        return x, False
    H = np.array(H, dtype=np.float64)
    if mode == 1:
        ev = float(np.linalg.eigvalsh(H)[0])
        if ev < 0:
            H[np.diag_indices_from(H)] += (0.01 if mutate == "shift" else -ev * 1.0 + 0.01 * 1.0)
    with np.errstate(all="ignore"):
        A = H.copy(); y = np.array(g, dtype=np.float64)     # not re-checked: a pivot <= 0 ends the device's loop where it stands
        ok, _, L, y = factor_f64(A, y, mutate=mutate)
        return backsolve_f64(L, y, mutate), True


def coupled_f64(Hs, gs):
    """coupled mode in the exact form: each robot's block with npiv = n - 1, the corner and its right-hand side summed in robot order, the corner's pivot, the
    back substitution per robot.  Returns (xs[U][m], t)"""
    parts = [factor_f64(H, g, npiv=np.asarray(H).shape[0] - 1) for H, g in zip(Hs, gs)]
    assert all(p[0] for p in parts)
    m = np.asarray(Hs[0]).shape[0] - 1
    corner = 0.0; rhs = 0.0
    for _, _, L, y in parts:
        corner += L[m, m]; rhs += y[m]
    lc = math.sqrt(corner)
    xs = []
    for _, _, L, y in parts:
        L = L.copy(); y = y.copy(); L[m, m] = lc; y[m] = rhs / lc
        xs.append(backsolve_f64(L, y))
    return [x[:m] for x in xs], float(xs[0][m])


# ---- the direction record ------------------------------------------------------------------------
def record(x, g, coupled=False):
    """what tj_get_direction returns for a solution x of H x = g (the direction is -x): direction[3][T] (rows 0, 1, T-2, T-1 zero; unknown 3 (row - 2) + axis),
    t_direction, and -- decoupled and single (xs_wave0) -- wolfe = -sum d_i g_i = x.g over all n, gn = sqrt(sum g_i^2).  coupled: wolfe and gn are this robot's
    partial sums over its m control-point unknowns, sum d_i g_i and sum g_i^2 (k_xsolve_c2; a later stage completes them across robots)."""
    x = np.asarray(x, dtype=np.float64); g = np.asarray(g, dtype=np.float64)
    n = len(x); m = n - 1; T = (m + 12) // 3
    d = -x
    direction = np.zeros((3, T))
    direction[:, 2:T - 2] = d[:m].reshape(T - 4, 3).T
    if coupled:
        return dict(direction=direction, t_direction=d[m], wolfe=float(np.sum(d[:m] * g[:m])), gn=float(np.sum(g[:m] * g[:m])))
    return dict(direction=direction, t_direction=d[m], wolfe=-float(np.sum(d * g)), gn=math.sqrt(float(np.sum(g * g))))


def unrecord(direction, t_direction):
    """the solution x the device computed, from its record"""
    direction = np.asarray(direction, dtype=np.float64); T = direction.shape[1]
    return -np.concatenate([direction[:, 2:T - 2].T.reshape(-1), [t_direction]])


# ---- generators (seeded; inside pattern(P), every structural entry non-zero) --------------------------
def _l0(P, rng, diag):
    """lower factor inside the lower pattern (a skyline: L0 D L0^T stays inside it): the given diagonal, every structural entry below it non-zero and
    small against its column's diagonal"""
    n = dims(P)[0]
    low = np.tril(pattern(P), -1)
    mag = rng.uniform(0.05, 0.25, (n, n)) * rng.choice([-1.0, 1.0], (n, n))
    return np.where(low, mag * diag[None, :], 0.0) + np.diag(diag)


def _sym(L0, D):
    H = np.tril((L0 * D[None, :]) @ L0.T)
    return H + np.tril(H, -1).T


def spd(P, cond, seed=0):
    """SPD, cond(H) ~ cond: L0's diagonal graded from 1 to cond^-1/2 in random order"""
    rng = np.random.default_rng([P, int(round(math.log10(cond))), seed, 1])
    n = dims(P)[0]
    diag = cond ** (-0.5 * rng.permutation(n) / (n - 1))
    return _sym(_l0(P, rng, diag), np.ones(n))


def indefinite(P, k, seed=0):
    """D[k] = -1 is the first (and only) negative entry of H = L0 D L0^T, L0 unit-scaled: the exact form's first non-positive pivot is pivot k"""
    rng = np.random.default_rng([P, k, seed, 2])
    n = dims(P)[0]
    D = rng.uniform(0.5, 2.0, n); D[k] = -1.0
    return _sym(_l0(P, rng, np.ones(n)), D)


def indefinite_ks(P):
    n, m, _ = dims(P)
    return sorted({0, 1, 17, 18, m // 2, m - 1, m} & set(range(n)))


def zero_first_pivot(P, seed=0):
    """H[0][0] == 0.0 exactly (the very first pivot fails on `x <= 0` with equality), one later negative D entry"""
    H = indefinite(P, dims(P)[1] // 2, seed + 100)
    H[0, 0] = 0.0
    return H


def rhs(P, kind, seed=0):
    n, m, _ = dims(P)
    g = np.zeros(n)
    if kind == "random":
        return np.random.default_rng([P, seed, 3]).normal(0.0, 1.0, n)
    if kind != "zero":
        g[{"e0": 0, "e16": min(16, m), "e17": min(17, m), "e18": min(18, m), "em1": m - 1, "em": m}[kind]] = 1.0
    return g


def real_scene(scenes, P, mode, U=4):
    if mode == 0:
        return scenes.scn_a(n_points=4000, pieces=P)
    return dict(scenes.hard(U, 3000, pieces=P), mode=mode)


def real(scenes, P, mode, U=4, iters=2, want_engine=False):
    """the blocks the CPU oracle produces on real_scene after `iters` iterations, as the device holds them: Engine.local_grad with the per-piece PSD repair of
    Gradient_admm::global_spline_gradient applied (the oracle's own LLT test and smallest eigenvalue).  (lg[U][P][19], lh[U][P][19][19]) [+ the engine, its
    planes of this iteration in place]"""
    from oracle.pyoracle import Engine, Prims
    scene = real_scene(scenes, P, mode, U)
    prims = Prims("port")
    e = Engine("port", scene, {"res": 4})
    for _ in range(iters):
        e.iterate()
    e.stage_planes()
    lg = np.zeros((e.U, P, 19)); lh = np.zeros((e.U, P, 19, 19))
    for u in range(e.U):
        for sp in range(P):
            g, h = e.local_grad(u, sp)
            if prims.llt_fails(h):
                ev = prims.min_eig(h)
                if ev < 0:
                    for i in range(19):
                        h[i, i] = h[i, i] - ev * 1.0 + 0.01 * 1.0
            lg[u, sp], lh[u, sp] = g, h
    return (lg, lh, e) if want_engine else (lg, lh)


# ---- metrics, in decimal ---------------------------------------------------------------------------
def _norm(v):
    return sum((a * a for a in v), Decimal(0)).sqrt()


def _matvec(H, xd):
    """H x exactly (up to PREC digits) for a double matrix and a decimal vector, over the non-zeros of H"""
    out = []
    for row in np.asarray(H):
        nz = np.flatnonzero(row)
        out.append(sum((Decimal(float(row[j])) * xd[j] for j in nz), Decimal(0)))
    return out


def eta(H, g, x, shift=0.0):
    """normwise backward error ||g - (H + shift I) x||_2 / (||H + shift I||_F ||x||_2 + ||g||_2) of a double x, evaluated in decimal (0 for 0 / 0)"""
    with localcontext() as ctx:
        ctx.prec = PREC
        xd = _dec(x); gd = _dec(g); sh = Decimal(float(shift))
        Hx = _matvec(H, xd)
        r = [gd[i] - Hx[i] - sh * xd[i] for i in range(len(xd))]
        Hd = np.asarray(H)
        fro2 = sum((Decimal(float(v)) ** 2 for v in Hd[Hd != 0]), Decimal(0))
        if shift:
            fro2 += sum(((Decimal(float(Hd[i, i])) + sh) ** 2 - Decimal(float(Hd[i, i])) ** 2 for i in range(len(xd))), Decimal(0))
        den = fro2.sqrt() * _norm(xd) + _norm(gd)
        return float(_norm(r) / den) if den else 0.0


def forward_error(x, x_hp):
    """||x - x_hp||_2 / ||x_hp||_2 in decimal (0 for 0 / 0)"""
    with localcontext() as ctx:
        ctx.prec = PREC
        xd = _dec(x)
        den = _norm(x_hp)
        num = _norm([a - b for a, b in zip(xd, x_hp)])
        return float(num / den) if den else float(num)


def applied_shift(H, g, x):
    """s = x.(g - H x) / x.x in decimal: the multiple of the identity a solve of (H + s I) x = g added"""
    with localcontext() as ctx:
        ctx.prec = PREC
        xd = _dec(x); gd = _dec(g)
        Hx = _matvec(H, xd)
        return float(sum((xd[i] * (gd[i] - Hx[i]) for i in range(len(xd))), Decimal(0)) / sum((a * a for a in xd), Decimal(0)))


def eta_cap(n):
    return (3 * n + 1) * U64


def coupled_eta(Hs, gs, xs, t):
    """eta of the whole arrowhead system for per-robot solutions xs[U][m] and the shared t"""
    with localcontext() as ctx:
        ctx.prec = PREC
        m = len(xs[0]); td = Decimal(float(t))
        r2 = Decimal(0); x2 = td * td; g2 = Decimal(0); f2 = Decimal(0)
        rt = Decimal(0); gt = Decimal(0); htt = Decimal(0)
        for H, g, x in zip(Hs, gs, xs):
            H = np.asarray(H); xd = _dec(x) + [td]; gd = _dec(g)
            Hx = _matvec(H, xd)
            r2 += sum(((gd[i] - Hx[i]) ** 2 for i in range(m)), Decimal(0))
            rt += gd[m] - Hx[m]; gt += gd[m]; htt += Decimal(float(H[m, m]))
            x2 += sum((a * a for a in xd[:m]), Decimal(0)); g2 += sum((a * a for a in gd[:m]), Decimal(0))
            Hm = H.copy(); Hm[m, m] = 0.0
            f2 += sum((Decimal(float(v)) ** 2 for v in Hm[Hm != 0]), Decimal(0))
        r2 += rt * rt; g2 += gt * gt; f2 += htt * htt
        den = f2.sqrt() * x2.sqrt() + g2.sqrt()
        return float(r2.sqrt() / den) if den else 0.0


def coupled_forward_error(xs, t, xs_hp, t_hp):
    with localcontext() as ctx:
        ctx.prec = PREC
        a = [v for x in xs for v in _dec(x)] + [Decimal(float(t))]
        b = [v for x in xs_hp for v in x] + [t_hp]
        den = _norm(b); num = _norm([p - q for p, q in zip(a, b)])
        return float(num / den) if den else float(num)


def sum_bound(terms):
    """(n + 2) u sum|terms|: the bound on a recursive sum of n rounded products, any order"""
    terms = np.asarray(terms, dtype=np.float64)
    return (len(terms) + 2) * U64 * float(np.sum(np.abs(terms)))


# ---- the cases the tests run, and their checks (shared by the CPU sensitivity test and the GPU tests) ---------
def cond_for(P, cond):
    """the class's conditioning at P pieces: the nominal one, lowered where the smallest exact pivot 1 / cond would not clear 100 n u max(diag) by a factor
    above two (max(diag) is about 1): min(cond, 1 / (256 n u)).  That lowers the 1e12 class from P = 5 (n = 43: 8.2e11) to P = 31 (n = 277: 1.3e11)."""
    return min(cond, 1.0 / (256 * dims(P)[0] * U64))


CLASSES = ("spd1e2", "spd1e8", "spd1e12", "real")
# every class meets every right-hand side of RHS_KINDS (the real class its own gradient in place of e16), each system with a matrix of its own: seven non-zero
# systems per class and P.  The class bar is the MAXIMUM of the exact form's error over them, and it needs that many: at cond ~ 1e12 the exact form's own
# forward error moves by more than 8x under a change of rounding alone (P = 2, the same system scaled by 3: 4.0e-7 -> 5.0e-6), so a bar taken from four
# systems was missed by a correct solve.
_PLAN_A = tuple((cls, "own" if (cls == "real" and kind == "e16") else kind) for kind in RHS_KINDS for cls in CLASSES)


def _class_matrix(P, cls, seed, reals):
    if cls == "real":
        H, g = reals[seed % len(reals)]
        return np.tril(H) + np.tril(H, -1).T, g      # (the solvers read the lower triangle)
    cond = {"spd1e2": 1e2, "spd1e8": 1e8, "spd1e12": 1e12}[cls]
    return spd(P, cond_for(P, cond), seed), None


def cases_a(P, reals):
    """the thirty-two systems of the accuracy test, in slot order (four batches of eight, two of every class in each): (class, H, g).  reals: [(H, g)]
    assembled real systems of this P"""
    out = []
    for i, (cls, kind) in enumerate(_PLAN_A):
        H, g_own = _class_matrix(P, cls, i, reals)
        out.append((cls, H, g_own if kind == "own" else rhs(P, kind, i)))
    return out


def cases_coupled(P, reals):
    """coupled mode: two fleets of eight per class (a fleet is ONE arrowhead system, so it carries one class): the eight RHS_KINDS over the robots, then
    random right-hand sides.  reals: the eight real systems of the mode-2 oracle.  [(class, [H] * 8, [g] * 8)]"""
    out = []
    for cls in CLASSES:
        for b in range(2):
            Hs, gs = [], []
            for u in range(8):
                H, g_own = _class_matrix(P, cls, 8 * b + u, reals)
                Hs.append(H)
                gs.append(g_own if (cls == "real" and b == 0) else rhs(P, RHS_KINDS[u] if b == 0 else "random", 8 * b + u))
            out.append((cls, Hs, gs))
    return out


def cases_b(P):
    """the failing systems of mode 1: indefinite(P, k) for every k in range, zero_first_pivot(P); random right-hand sides.  [(name, H, g)]"""
    out = [("indefinite%d" % k, indefinite(P, k), rhs(P, "random", 50 + k)) for k in indefinite_ks(P)]
    return out + [("zero_first_pivot", zero_first_pivot(P), rhs(P, "random", 49))]


def measure(H, g, x, x_hp=None, shift=0.0):
    """(eta, forward error against the decimal solve) of a double solution x"""
    if x_hp is None:
        x_hp, _ = solve_hp(H, g, shift)
    return eta(H, g, x, shift), forward_error(x, x_hp)


def bars_a(cases):
    """per class (max eta, max forward error) of the exact-form double solve over the class's systems, and the decimal solutions.  {class: (eta, fe)}, [x_hp]"""
    bars = {}; hp = []
    for cls, H, g in cases:
        ok, x, _ = solve_f64(H, g)
        assert ok, cls
        xh, piv = solve_hp(H, g)
        e, f = measure(H, g, x, xh)
        b = bars.get(cls, (0.0, 0.0))
        bars[cls] = (max(b[0], e), max(b[1], f)); hp.append(xh)
    return bars, hp


FACTOR = 8.0      # the device may be at most this many times the exact form's error (FAST: reciprocal root of 1-2 ulp and a multiplication for sqrt and /: up to ~3x per entry)


def check_a(cases, xs, bars, hp):
    """the accuracy bar on solutions xs of `cases`: eta <= min(FACTOR * class eta, (3n + 1) u), forward error <= FACTOR * class forward error.  Returns the largest
    ratios to the class bars {class: (eta ratio, fe ratio)}; raises AssertionError on a miss.  A zero right-hand side must give zeros (either sign)."""
    ratios = {}
    for (cls, H, g), x, xh in zip(cases, xs, hp):
        n = len(g)
        assert x is not None and np.all(np.isfinite(x)), cls
        if not np.any(g):
            assert not np.any(x), (cls, "zero right-hand side")
            continue
        e, f = measure(H, g, x, xh)
        be, bf = bars[cls]
        r = ratios.get(cls, (0.0, 0.0))
        ratios[cls] = (max(r[0], e / be), max(r[1], f / bf))
        assert e <= eta_cap(n), (cls, "eta above (3n + 1) u", e / U64)
        assert e <= FACTOR * be, (cls, "eta", e / U64, "exact form's", be / U64)
        assert f <= FACTOR * bf, (cls, "forward error", f, "exact form's", bf)
    return ratios


def bars_coupled(cases):
    bars = {}; hp = []
    for cls, Hs, gs in cases:
        xs, t = coupled_f64(Hs, gs)
        xh, th, _ = coupled_hp(Hs, gs)
        e, f = coupled_eta(Hs, gs, xs, t), coupled_forward_error(xs, t, xh, th)
        b = bars.get(cls, (0.0, 0.0))
        bars[cls] = (max(b[0], e), max(b[1], f)); hp.append((xh, th))
    return bars, hp


def check_coupled(cases, sols, bars, hp):
    """check_a for coupled fleets: sols = [(xs[8][m], t)]; the cap is (3N + 1) u for the N = 8 m + 1 unknowns of the arrowhead system"""
    ratios = {}
    for (cls, Hs, gs), (xs, t), (xh, th) in zip(cases, sols, hp):
        N = len(Hs) * (len(gs[0]) - 1) + 1
        e, f = coupled_eta(Hs, gs, xs, t), coupled_forward_error(xs, t, xh, th)
        be, bf = bars[cls]
        r = ratios.get(cls, (0.0, 0.0))
        ratios[cls] = (max(r[0], e / be), max(r[1], f / bf))
        assert e <= eta_cap(N), (cls, "eta above (3N + 1) u", e / U64)
        assert e <= FACTOR * be, (cls, "eta", e / U64, "exact form's", be / U64)
        assert f <= FACTOR * bf, (cls, "forward error", f, "exact form's", bf)
    return ratios


def check_b(cases, xs):
    """mode 1's fallback on solutions xs of failing systems: the applied shift s = x.(g - H x) / x.x is 0.01 - lambda_min within 1e-12 max(1, max|H|) (the
    project's bar for min_eig_lds) + (3n + 1) u max|H|, and x solves (H + s I) x = g to the accuracy bar: eta <= min(FACTOR * the exact form's on the same
    shifted systems, (3n + 1) u).  Returns (largest shift error / its bound, largest eta ratio)."""
    want = []; bar = 0.0
    for name, H, g in cases:
        lam = float(np.linalg.eigvalsh(H)[0])
        assert lam <= -1e-6 * np.abs(H).max(), name
        s0 = -lam * 1.0 + 0.01 * 1.0
        Hs = H.copy(); Hs[np.diag_indices_from(Hs)] += s0
        ok, xf, _ = solve_f64(Hs, g)
        assert ok, name
        bar = max(bar, eta(Hs, g, xf)); want.append(s0)
    worst_s = worst_e = 0.0
    for (name, H, g), x, s0 in zip(cases, xs, want):
        n = len(g); hmax = float(np.abs(H).max())
        assert x is not None and np.all(np.isfinite(x)), name
        s = applied_shift(H, g, x)
        tol = 1e-12 * max(1.0, hmax) + eta_cap(n) * hmax
        worst_s = max(worst_s, abs(s - s0) / tol)
        assert abs(s - s0) <= tol, (name, "applied shift", s, "0.01 - lambda_min", s0)
        e = eta(H, g, x, s)
        worst_e = max(worst_e, e / bar)
        assert e <= eta_cap(n) and e <= FACTOR * bar, (name, "eta of the shifted system", e / U64, "exact form's", bar / U64)
    return worst_s, worst_e
